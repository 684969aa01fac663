// Training-time dropout (include/cdseg.h, "dropout"): the attention forward with the mask between the softmax and P V, and
// element dropout behind a Linear.
//
// ref: point_transformer_v3m1_base.py:282-288, :1038-1047 (flash_attn_varlen_*_func(..., dropout_p=attn_drop)),
//      :293-294, :1052-1053 (proj_drop), :316-322 (MLP.drop).
//
// The two forward kernels are the q-side kernels of the recompute-P backward (train.hip) with V in the place of K in the
// second product: K and V of the patch-head in LDS, a wave owns query tiles, sweep 1 leaves the row statistics (m, l) of the
// UNMASKED softmax, sweep 2 recomputes the scores and feeds f o P (f = M / keep) from the accumulator registers into
// O^T += V^T (f o P)^T.  So forward and backward evaluate the mask at the same (query, key) registers and round at the same
// points (16-bit form: f o P is rounded once, as the MFMA operand).  Training kernels: two score sweeps instead of the
// inference kernel's one, not tuned.
#include <mutex>

#include "attn_train.h"
#include "common.h"
#include "route.h"

namespace {

using namespace cdseg_attn_train;

struct AttnDropP {
  const void* q; const void* k; const void* v;
  const int32_t* q_gidx; const int32_t* kv_gidx; const int32_t* widx; const int32_t* patch_start;
  void* out;
  int ldq, ldk, ldv, ldo;
  float scale;
};

constexpr int FW_LDS = 2 * BW_MAXL * 64;
constexpr int FW16_LDS = 2 * B16_IMG;

__global__ __launch_bounds__(BW_WAVES * 64) void attn_drop_f32_kernel(AttnDropP p, DropP d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Ks = smem;
  char* Vs = smem + BW_MAXL * 64;
  const float* pq = (const float*)p.q;
  const float* pk = (const float*)p.k;
  const float* pv = (const float*)p.v;
  const int patch = blockIdx.x, head = blockIdx.y;
  const int ps = p.patch_start[patch], L = p.patch_start[patch + 1] - ps;
  const int nt = (L + 15) >> 4, Lp = nt << 4;
  if ((int)blockIdx.z * BW_WAVES >= nt) return;  // (block-uniform) a slice without tiles
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int s = tid; s < Lp; s += BW_WAVES * 64) {
    float4 kk[4], vv[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) kk[c] = vv[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (s < L) {
      const long r = p.kv_gidx[ps + s];
      const float4* kp = reinterpret_cast<const float4*>(pk + r * p.ldk + head * HD);
      const float4* vp = reinterpret_cast<const float4*>(pv + r * p.ldv + head * HD);
#pragma unroll
      for (int c = 0; c < 4; ++c) { kk[c] = kp[c]; vv[c] = vp[c]; }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      *reinterpret_cast<float4*>(Ks + bw_off(s, c)) = kk[c];
      *reinterpret_cast<float4*>(Vs + bw_off(s, c)) = vv[c];
    }
  }
  __syncthreads();
  const int ql = lane & 15, g = lane >> 4;
  const float c2 = p.scale * 1.44269504088896340736f;
  for (int qt = blockIdx.z * BW_WAVES + wave; qt < nt; qt += BW_WAVES * gridDim.z) {  // blockIdx.z: 1, 2 or 4 slices of the query tiles
    const int qslot = qt * 16 + ql;
    const bool valid = qslot < L;
    float qf[4] = {0.f, 0.f, 0.f, 0.f};  // B operand: (query ql, head dims 4 g .. 4 g + 3)
    if (valid) {
      const long qrow = p.q_gidx[ps + qslot];
      const float4 t = *reinterpret_cast<const float4*>(pq + qrow * p.ldq + head * HD + 4 * g);
      qf[0] = t.x * c2; qf[1] = t.y * c2; qf[2] = t.z * c2; qf[3] = t.w * c2;
    }
    auto tile = [&](int kt) {  // S'^T of key tile kt: rows = keys 4 g + r, column = query ql
      const float4 kf = *reinterpret_cast<const float4*>(Ks + bw_off(kt * 16 + ql, g));
      const float ka[4] = {kf.x, kf.y, kf.z, kf.w};
      f32x4_t sc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < 4; ++t) sc = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[t], qf[t], sc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (kt * 16 + 4 * g + r >= L) sc[r] = -INFINITY;
      return sc;
    };
    // ---- sweep 1: online (m, l) over the lane's keys, then across the four lane groups of the query
    float m = -INFINITY, l = 0.f;
    for (int kt = 0; kt < nt; ++kt) {
      const f32x4_t sc = tile(kt);
      const float mn = fmaxf(m, fmaxf(fmaxf(sc[0], sc[1]), fmaxf(sc[2], sc[3])));
      if (mn > -INFINITY) {
        l *= exp2f(m - mn);
#pragma unroll
        for (int r = 0; r < 4; ++r) l += exp2f(sc[r] - mn);
        m = mn;
      }
    }
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
      const float m2 = __shfl_xor(m, off, 64), l2 = __shfl_xor(l, off, 64);
      const float mn = fmaxf(m, m2);
      if (mn > -INFINITY) l = l * exp2f(m - mn) + l2 * exp2f(m2 - mn);
      m = mn;
    }
    const float il = 1.0f / l;
    // ---- sweep 2: O^T (rows = head dims 4 g + r, column = query ql) += V^T (f o P)^T
    f32x4_t o = {0.f, 0.f, 0.f, 0.f};
    for (int kt = 0; kt < nt; ++kt) {
      const f32x4_t sc = tile(kt);
      float f[4], pr[4];
      drop_keys4(d, patch, head, qslot, 4 * kt + g, f);
#pragma unroll
      for (int r = 0; r < 4; ++r) pr[r] = exp2f(sc[r] - m) * il * f[r];  // (masked keys: exp2(-inf) = 0)
#pragma unroll
      for (int t = 0; t < 4; ++t)  // k-slot g of MFMA t <-> key 4 g + t: A = V[key][head dim ql], B = register t
        o = __builtin_amdgcn_mfma_f32_16x16x4f32(bw_elem(Vs, kt * 16 + 4 * g + t, ql), pr[t], o, 0, 0, 0);
    }
    if (valid) {
      const int w = p.widx[ps + qslot];  // padding duplicates have no output row
      if (w >= 0) *reinterpret_cast<float4*>((float*)p.out + (long)w * p.ldo + head * HD + 4 * g) = make_float4(o[0], o[1], o[2], o[3]);
    }
  }
}

// The 16-bit form: attn_bwd16_q_kernel's tiles (32 x 32, v_mfma_f32_32x32x16 of the build's 16-bit type), q' = q * fp32(scale
// log2 e) rounded once as in attn_bf16_kernel (flags 0), fp32 statistics with the exact row maximum, f o P rounded to the
// 16-bit type as the MFMA operand (without saturation: it is at most 256), fp32 accumulator, output rounded like every 16-bit
// store of the library (saturating in the half build).  blockIdx.z deals the query tiles to 1, 2 or 4 blocks.
__global__ __launch_bounds__(B16_WAVES * 64, 4) void attn_drop16_kernel(AttnDropP p, DropP d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Ks = smem;
  char* Vs = smem + B16_IMG;
  const bf16_t* pq = (const bf16_t*)p.q;
  const bf16_t* pk = (const bf16_t*)p.k;
  const bf16_t* pv = (const bf16_t*)p.v;
  const unsigned lds_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  const int patch = blockIdx.x, head = blockIdx.y;
  const int ps = p.patch_start[patch], L = p.patch_start[patch + 1] - ps;
  const int nt = (L + 31) >> 5;
  if ((int)blockIdx.z * B16_WAVES >= nt) return;  // (block-uniform) a slice without tiles
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < nt * 64; i += B16_WAVES * 64) {  // (row, 16-byte half)
    const int s = i >> 1, hs = i & 1;
    uint4 kk = make_uint4(0, 0, 0, 0), vv = kk;
    if (s < L) {
      const long r = p.kv_gidx[ps + s];
      kk = *reinterpret_cast<const uint4*>(pk + r * p.ldk + head * HD + hs * 8);
      vv = *reinterpret_cast<const uint4*>(pv + r * p.ldv + head * HD + hs * 8);
    }
    const int o = b16_off(s, 2 * hs);
    *reinterpret_cast<uint4*>(Ks + o) = kk;
    *reinterpret_cast<uint4*>(Vs + o) = vv;
  }
  __syncthreads();
  const int ql = lane & 31, h = lane >> 5;
  const float c2 = p.scale * 1.44269504088896340736f;
  const int row_off = b16_off(ql, 2 * h);  // A operand of S'^T: key ql of the tile, head dims 8 h .. 8 h + 7
  // V^T fragments: the lane's 16-lane group reads keys 4 h + {0 .. 3} (and + 8) of a 16-key half tile
  const unsigned tr0 = lds_base + B16_IMG + b16_off(4 * h + ((lane & 15) >> 2), lane & 3);
  const unsigned tr1 = lds_base + B16_IMG + b16_off(4 * h + ((lane & 15) >> 2) + 8, lane & 3);
  const f32x16_t zero16 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int qt = blockIdx.z * B16_WAVES + wave; qt < nt; qt += B16_WAVES * gridDim.z) {
    const int qslot = qt * 32 + ql;
    const bool valid = qslot < L;
    uint4 qraw = make_uint4(0, 0, 0, 0);  // B operand: (query ql, head dims 8 h .. 8 h + 7)
    if (valid) {
      const long qrow = p.q_gidx[ps + qslot];
      qraw = *reinterpret_cast<const uint4*>(pq + qrow * p.ldq + head * HD + 8 * h);
    }
    const bf16x8_t qf = b16_frag(b16_prescale(qraw, c2));
    // ---- sweep 1: online (m', l) over the lane's keys (rows (r & 3) + 8 (r >> 2) + 4 h of each tile)
    float m = -INFINITY, l = 0.f;
    for (int kt = 0; kt < nt; ++kt) {
      f32x16_t sc = mfma_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(Ks + kt * 1024 + row_off), qf, zero16);
      if (kt == nt - 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h >= L) sc[r] = -INFINITY;
      }
      float mn = m;
#pragma unroll
      for (int r = 0; r < 16; ++r) mn = fmaxf(mn, sc[r]);
      if (mn > -INFINITY) {
        l *= __builtin_amdgcn_exp2f(m - mn);
#pragma unroll
        for (int r = 0; r < 16; ++r) l += __builtin_amdgcn_exp2f(sc[r] - mn);
        m = mn;
      }
    }
    {
      const float m2 = __shfl_xor(m, 32, 64), l2 = __shfl_xor(l, 32, 64);
      const float mn = fmaxf(m, m2);
      if (mn > -INFINITY) l = l * __builtin_amdgcn_exp2f(m - mn) + l2 * __builtin_amdgcn_exp2f(m2 - mn);
      m = mn;
    }
    const float il = 1.0f / l;
    // ---- sweep 2: O^T (rows = head dims, column = query ql) += V^T (f o P)^T; -m' is the MFMA's C operand
    const float nm = valid ? -m : 0.f;
    const f32x16_t negm = {nm, nm, nm, nm, nm, nm, nm, nm, nm, nm, nm, nm, nm, nm, nm, nm};
    f32x16_t o = zero16;
    for (int kt = 0; kt < nt; ++kt) {
      const f32x16_t sc = mfma_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(Ks + kt * 1024 + row_off), qf, negm);
      float pr[16], f[16];  // registers 4 c .. 4 c + 3: keys 32 kt + 8 c + 4 h + {0 .. 3}
      drop_keys16(d, patch, head, qslot, 8 * kt + h, f);
#pragma unroll
      for (int r = 0; r < 16; ++r) pr[r] = __builtin_amdgcn_exp2f(sc[r]) * (il * f[r]);
      if (kt == nt - 1) {  // keys past the end of a ragged patch (their K rows are zero: s' = 0, not -inf)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h >= L) pr[r] = 0.f;
      }
#pragma unroll
      for (int mf = 0; mf < 2; ++mf)
        o = mfma_32x32x16_bf16(b16_tr_pair(tr0 + kt * 1024 + mf * 512, tr1 + kt * 1024 + mf * 512), b16_pack8(pr + 8 * mf), o);
    }
    if (valid) {  // rows 4 h + (r & 3) + 8 (r >> 2), r < 8
      const int w = p.widx[ps + qslot];
      if (w >= 0) {
        bf16_t* op = (bf16_t*)p.out + (long)w * p.ldo + head * HD + 4 * h;
        *reinterpret_cast<uint2*>(op) = make_uint2(pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]));
        *reinterpret_cast<uint2*>(op + 8) = make_uint2(pack_bf16x2(o[4], o[5]), pack_bf16x2(o[6], o[7]));
      }
    }
  }
}

// ---- element dropout: y[r][c] = x[r][c] * f.  A thread owns 16 consecutive columns of a row = one Philox call
// (counter (c >> 4, r)): four 16-byte accesses where VEC, scalar ones otherwise and on a ragged last group.
template <bool VEC>
__global__ __launch_bounds__(256) void dropout_kernel(const float* x, int ldx, float* y, int ldy, long m, int c, int groups, DropP d) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= m * groups) return;
  const long row = t / groups;
  const int grp = (int)(t - row * groups), col0 = grp * 16;
  const uint4 w4 = philox4x32_10((uint32_t)grp, (uint32_t)row, d.c2, d.c3, d.k0, d.k1);
  const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
  const float* xr = x + row * ldx + col0;
  float* yr = y + row * ldy + col0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (VEC && col0 + 4 * q + 3 < c) {
      float4 v = *reinterpret_cast<const float4*>(xr + 4 * q);
      v.x *= drop_factor(d, w[q], 0); v.y *= drop_factor(d, w[q], 1); v.z *= drop_factor(d, w[q], 2); v.w *= drop_factor(d, w[q], 3);
      *reinterpret_cast<float4*>(yr + 4 * q) = v;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (col0 + 4 * q + e < c) yr[4 * q + e] = xr[4 * q + e] * drop_factor(d, w[q], e);
    }
  }
}

}  // namespace

extern "C" int cdseg_attention_drop(const void* q, const void* k, const void* v, int ldq, int ldk, int ldv, const int32_t* q_gidx,
                                    const int32_t* kv_gidx, const int32_t* widx, const int32_t* patch_start, int num_patches,
                                    int num_heads, int max_len, float scale, void* out, int ldo, int dtype, double rate,
                                    uint64_t seed, uint64_t offset, void* stream) {
  DropP d;
  if (!cdseg_drop_threshold(rate, seed, offset, &d)) return CDSEG_ERR_ARG;
  if (dtype != CDSEG_F32 && dtype != CDSEG_BF16) return CDSEG_ERR_ARG;
  if (max_len > CDSEG_MAX_PATCH || num_heads > 65535) return CDSEG_ERR_ARG;
  if (num_patches <= 0 || num_heads <= 0) return CDSEG_OK;
  if (max_len <= 0) return CDSEG_ERR_ARG;
  if (!q || !k || !v || !out || !q_gidx || !kv_gidx || !widx || !patch_start) return CDSEG_ERR_ARG;
  const int per16 = dtype == CDSEG_F32 ? 3 : 7;  // 16-byte rows
  if ((ldq | ldk | ldv | ldo) & per16) return CDSEG_ERR_ARG;
  if ((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15) != 0) return CDSEG_ERR_ARG;
  if (d.thr >= 256)  // nothing is dropped: cdseg_attention, bit for bit
    return cdseg_attention(q, k, v, ldq, ldk, ldv, q_gidx, kv_gidx, widx, patch_start, num_patches, num_heads, max_len, scale, out, ldo,
                           dtype, stream);
  AttnDropP p;
  p.q = q; p.k = k; p.v = v; p.q_gidx = q_gidx; p.kv_gidx = kv_gidx; p.widx = widx; p.patch_start = patch_start; p.out = out;
  p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo; p.scale = scale;
  static std::once_flag attr_once;
  static bool attr_ok = false;
  std::call_once(attr_once, [] {
    attr_ok = hipFuncSetAttribute((const void*)attn_drop_f32_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, FW_LDS) == hipSuccess &&
              hipFuncSetAttribute((const void*)attn_drop16_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, FW16_LDS) == hipSuccess;
  });
  if (!attr_ok) return CDSEG_ERR_LAUNCH;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == CDSEG_BF16) {
    int split = 1;  // as cdseg_attention_bwd: slices of a patch-head's query tiles while the launch does not fill the chip
    while (split < 4 && (long)num_patches * num_heads * split * 2 <= 512) split *= 2;
    cdseg_route_rec(CDSEG_RK_ATTN_DROP_B16, 32, 32, split, 0, 0, CDSEG_BF16 << CDSEG_ROUTE_F_CT_SHIFT, B16_WAVES);
    hipLaunchKernelGGL(attn_drop16_kernel, dim3((unsigned)num_patches, (unsigned)num_heads, (unsigned)split), dim3(B16_WAVES * 64), FW16_LDS,
                       s, p, d);
  } else {
    int split = 1;  // one block per CU (128 KiB of LDS): slices while the launch leaves CUs idle
    while (split < 4 && (long)num_patches * num_heads * split * 2 <= 256) split *= 2;
    cdseg_route_rec(CDSEG_RK_ATTN_DROP_F32, 16, 16, split, 0, 0, CDSEG_F32 << CDSEG_ROUTE_F_CT_SHIFT, BW_WAVES);
    hipLaunchKernelGGL(attn_drop_f32_kernel, dim3((unsigned)num_patches, (unsigned)num_heads, (unsigned)split), dim3(BW_WAVES * 64), FW_LDS,
                       s, p, d);
  }
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

extern "C" int cdseg_dropout(const float* x, int ldx, float* y, int ldy, long m, int c, double rate, uint64_t seed, uint64_t offset,
                             void* stream) {
  DropP d;
  if (!cdseg_drop_threshold(rate, seed, offset, &d)) return CDSEG_ERR_ARG;
  if (m < 0 || c < 0 || m >= (1l << 32)) return CDSEG_ERR_ARG;
  if (m == 0 || c == 0) return CDSEG_OK;
  if (!x || !y || ldx < c || ldy < c || ((((uintptr_t)x) | ((uintptr_t)y)) & 3)) return CDSEG_ERR_ARG;
  const int groups = (c + 15) / 16;
  const bool vec = !((((uintptr_t)x) | ((uintptr_t)y)) & 15) && !((ldx | ldy) & 3);
  const long threads = m * groups;
  if ((threads + 255) / 256 > 0x7fffffffl) return CDSEG_ERR_UNSUPPORTED;
  cdseg_route_rec(CDSEG_RK_DROPOUT_F32, 0, 0, 1, 0, 0, CDSEG_F32 << CDSEG_ROUTE_F_CT_SHIFT, vec ? 16 : 4);
  const dim3 grid((unsigned)((threads + 255) / 256));
  if (vec) hipLaunchKernelGGL(dropout_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, ldx, y, ldy, m, c, groups, d);
  else hipLaunchKernelGGL(dropout_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, ldx, y, ldy, m, c, groups, d);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}
