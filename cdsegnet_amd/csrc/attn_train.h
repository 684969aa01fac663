// What the training attention kernels share (train.hip: the four backward kernels; attention_drop.hip: the dropout
// forward): the LDS images of a patch-head, the 16-bit fragment helpers, and the dropout mask of include/cdseg.h.
#pragma once
#include "common.h"

namespace cdseg_attn_train {

constexpr int HD = 16;        // head dim
constexpr int BW_WAVES = 16;  // waves per block of the fp32 kernels (1 block per CU: the LDS holds K + V or Q + dO)
constexpr int BW_MAXL = 1024;

// fp32 image: LDS rows are 16 floats; the four 16-byte chunks of a row are XOR-swizzled with (row >> 1) & 3 (conflict-free
// float4 operand reads, like attn_f32_kernel's K image).
__device__ __forceinline__ int bw_off(int row, int chunk) { return row * 64 + ((chunk ^ ((row >> 1) & 3)) << 4); }
__device__ __forceinline__ float bw_elem(const char* base, int row, int d) {
  return *reinterpret_cast<const float*>(base + bw_off(row, d >> 2) + (d & 3) * 4);
}

constexpr int B16_WAVES = 8;
constexpr int B16_IMG = BW_MAXL * 32;  // one 16-bit operand of a patch-head

typedef __attribute__((ext_vector_type(4))) short b16_s16x4_t;
typedef __attribute__((address_space(3))) b16_s16x4_t b16_lds_s16x4_t;

// byte offset of (row, 4-dim chunk c4) in a row-major 16-bit image: rows are 32 bytes; the two 16-byte halves are swapped
// for rows with bit 3 set
__device__ __forceinline__ int b16_off(int row, int c4) { return row * 32 + ((((c4 >> 1) ^ (row >> 3)) & 1) << 4) + ((c4 & 1) << 3); }

// A operand = rows 0 .. 15 of X^T for the 16 rows (k-slots) of X the lane's half wave covers: two transposing reads
__device__ __forceinline__ bf16x8_t b16_tr_pair(unsigned a0, unsigned a1) {
  const b16_s16x4_t v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<b16_lds_s16x4_t*>(a0));
  const b16_s16x4_t v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<b16_lds_s16x4_t*>(a1));
  return __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
}

// q * c rounded once to the 16-bit type, as attn_bf16_kernel prepares its B operand (flags 0)
__device__ __forceinline__ uint4 b16_prescale(uint4 r, float c) {
  float lo, hi;
  unpack_bf16x2(r.x, lo, hi); r.x = pack_bf16x2(lo * c, hi * c);
  unpack_bf16x2(r.y, lo, hi); r.y = pack_bf16x2(lo * c, hi * c);
  unpack_bf16x2(r.z, lo, hi); r.z = pack_bf16x2(lo * c, hi * c);
  unpack_bf16x2(r.w, lo, hi); r.w = pack_bf16x2(lo * c, hi * c);
  return r;
}

__device__ __forceinline__ bf16x8_t b16_frag(uint4 u) { return __builtin_bit_cast(bf16x8_t, u); }

// registers 8 mf .. 8 mf + 7 of a 32 x 32 accumulator as the 16-bit B fragment of k-slots 8 h .. 8 h + 7 (no saturation)
__device__ __forceinline__ bf16x8_t b16_pack8(const float* x) {
  return b16_frag(make_uint4(pack_bf16x2_inrange(x[0], x[1]), pack_bf16x2_inrange(x[2], x[3]), pack_bf16x2_inrange(x[4], x[5]),
                             pack_bf16x2_inrange(x[6], x[7])));
}

// ---- the dropout mask (include/cdseg.h, "dropout"): Philox4x32-10 keyed by seed, upper counter words = offset.
// One call is a 4 x 4 block of a patch-head's (query, key) plane: word = query & 3, byte = key & 3.  Every kernel's lane
// holds either four keys of one query (one word) or four queries of one key (one byte of each word) per 16 / 32-wide tile,
// so a call feeds four accumulator elements in both orientations.
struct DropP {
  uint32_t k0, k1, c2, c3;  // seed (low, high), offset (low, high)
  uint32_t thr;             // keep iff byte < thr
  float inv_keep;           // 256 / thr
};

__device__ __forceinline__ uint4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return make_uint4(c0, c1, c2, c3);
}

// the call of the 4 x 4 block (queries 4 ib .. 4 ib + 3, keys 4 jb .. 4 jb + 3) of (patch, head)
__device__ __forceinline__ uint4 drop_block(const DropP& d, int patch, int head, int ib, int jb) {
  return philox4x32_10((uint32_t)jb | ((uint32_t)ib << 8) | ((uint32_t)head << 16), (uint32_t)patch, d.c2, d.c3, d.k0, d.k1);
}
__device__ __forceinline__ uint32_t drop_word(uint4 w, int i) {
  i &= 3;
  return i == 0 ? w.x : i == 1 ? w.y : i == 2 ? w.z : w.w;
}
__device__ __forceinline__ float drop_factor(const DropP& d, uint32_t word, int byte) {
  return ((word >> (8 * (byte & 3))) & 255u) < d.thr ? d.inv_keep : 0.f;
}
// one query, keys 4 jb .. 4 jb + 3
__device__ __forceinline__ void drop_keys4(const DropP& d, int patch, int head, int query, int jb, float* f) {
  const uint32_t w = drop_word(drop_block(d, patch, head, query >> 2, jb), query);
#pragma unroll
  for (int r = 0; r < 4; ++r) f[r] = drop_factor(d, w, r);
}
// one key, queries 4 ib .. 4 ib + 3
__device__ __forceinline__ void drop_queries4(const DropP& d, int patch, int head, int ib, int key, float* f) {
  const uint4 w = drop_block(d, patch, head, ib, key >> 2);
  f[0] = drop_factor(d, w.x, key); f[1] = drop_factor(d, w.y, key); f[2] = drop_factor(d, w.z, key); f[3] = drop_factor(d, w.w, key);
}

// The 32 x 32 tiles of the 16-bit kernels: a lane holds four 4-blocks per tile (registers 4 c .. 4 c + 3, c = 0 .. 3), and the
// four lanes of a quad (lanes 4 a .. 4 a + 3: consecutive queries / keys of one block row / column, the same half wave) hold
// the same four blocks.  Lane c of the quad evaluates block c and the quad exchanges the words by DPP quad broadcasts: one
// Philox call per lane and tile instead of four.  Call sites are wave-uniform (every lane of the wave is active).
template <int C>
__device__ __forceinline__ uint32_t quad_bcast(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, C * 0x55, 0xf, 0xf, true);  // quad_perm: [C, C, C, C]
}
template <int C>
__device__ __forceinline__ uint4 quad_bcast4(uint4 w) {
  return make_uint4(quad_bcast<C>(w.x), quad_bcast<C>(w.y), quad_bcast<C>(w.z), quad_bcast<C>(w.w));
}
// one query (lane & 3 == query & 3), keys 4 (jb0 + 2 c) .. + 3 into f[4 c .. 4 c + 3]
__device__ __forceinline__ void drop_keys16(const DropP& d, int patch, int head, int query, int jb0, float* f) {
  const uint4 mine = drop_block(d, patch, head, query >> 2, jb0 + 2 * (query & 3));
  const uint32_t w[4] = {drop_word(quad_bcast4<0>(mine), query), drop_word(quad_bcast4<1>(mine), query),
                         drop_word(quad_bcast4<2>(mine), query), drop_word(quad_bcast4<3>(mine), query)};
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) f[4 * c + r] = drop_factor(d, w[c], r);
}
// one key (lane & 3 == key & 3), queries 4 (ib0 + 2 c) .. + 3 into f[4 c .. 4 c + 3]
__device__ __forceinline__ void drop_queries16(const DropP& d, int patch, int head, int ib0, int key, float* f) {
  const uint4 mine = drop_block(d, patch, head, ib0 + 2 * (key & 3), key >> 2);
  const uint4 w[4] = {quad_bcast4<0>(mine), quad_bcast4<1>(mine), quad_bcast4<2>(mine), quad_bcast4<3>(mine)};
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    f[4 * c] = drop_factor(d, w[c].x, key); f[4 * c + 1] = drop_factor(d, w[c].y, key);
    f[4 * c + 2] = drop_factor(d, w[c].z, key); f[4 * c + 3] = drop_factor(d, w[c].w, key);
  }
}

}  // namespace cdseg_attn_train

// host side: threshold of a rate (include/cdseg.h); false for a rate outside [0, 1)
static inline bool cdseg_drop_threshold(double rate, uint64_t seed, uint64_t offset, cdseg_attn_train::DropP* d) {
  if (!(rate >= 0.0 && rate < 1.0)) return false;
  int t = (int)(256.0 * (1.0 - rate) + 0.5);
  if (t < 1) t = 1;
  d->k0 = (uint32_t)seed; d->k1 = (uint32_t)(seed >> 32); d->c2 = (uint32_t)offset; d->c3 = (uint32_t)(offset >> 32);
  d->thr = (uint32_t)t;
  d->inv_keep = 256.0f / (float)t;
  return true;
}
