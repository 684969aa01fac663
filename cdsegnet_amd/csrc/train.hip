// Training path: the backward of a PTv3 Block (attention core, LayerNorm, GELU; weight / bias gradients of the Linears and
// of the submanifold conv).
//
// ref: pointcept/models/default.py:424-493 (training forward), engines/train.py:216-271 (loss.backward()); what
//      autograd differentiates here: point_transformer_v3m1_base.py:246-296 (SerializedAttention core),
//      :399-428 (Block: x += proj(attn); x += fc2(GELU(fc1(LN(x))))).
//
// The fp32 kernels are those of the 1e-3 parity mode's backward, written to pin the arithmetic and the index plumbing
// (slot plan, padding duplicates) against the reference's autograd: the attention core and the weight gradients run on
// the fp32 matrix pipe (v_mfma_f32_16x16x4_f32); LayerNorm / GELU are row kernels.  The attention core also exists in the
// build's 16-bit type (attn_bwd16_*_kernel below, v_mfma_f32_32x32x16_{bf16,f16}): the recompute-P backward of
// attn_bf16_kernel, what the reference's flash-attention path computes in a training step.
#include <mutex>

#include "attn_train.h"
#include "common.h"
#include "route.h"
#include "wgrad_partition.h"

namespace {

using namespace cdseg_attn_train;  // HD, BW_WAVES, BW_MAXL, the LDS images, the 16-bit fragment helpers, the dropout mask

struct AttnBwdP {
  const float* q; const float* k; const float* v; const float* dout;
  const int32_t* q_gidx; const int32_t* kv_gidx; const int32_t* widx; const int32_t* patch_start;
  float* dq; float* dk; float* dv;
  float* stats;  // (slot, head, {m (log2 units of the prescaled scores), 1 / l, D})
  int ldq, ldk, ldv, lddo, lddq, lddk, lddv;
  int num_heads;
  float scale;
};

// The attention backward on the fp32 matrix pipe (v_mfma_f32_16x16x4_f32), exact fp32 like the parity mode's forward
// (attn_f32_kernel).  With s_ij = scale q_i.k_j, P = softmax_j(s), dP_ij = dO_i.v_j, D_i = sum_j P_ij dP_ij,
// dS = P o (dP - D):   dQ = scale dS K,   dK = scale dS^T Q,   dV = P^T dO.
// One block = one (patch, head); two kernels, each in the orientation that needs no transposition:
//   q kernel  (K, V of the patch-head in LDS; a wave owns 16-query tiles): S^T = K Q^T and dP^T = V dO^T come out of the
//             MFMA with a query per lane column and 4 keys per lane - sweep 1 keeps the running (max, sum, sum P dP) of
//             the online softmax and leaves (m, 1 / l, D) per query, sweep 2 recomputes them and feeds dS^T STRAIGHT from
//             the accumulator registers into dQ^T += K^T dS^T (MFMA t takes k-slot kq <-> key 4 kq + t, which is register
//             t of lane group kq: no permute);
//   kv kernel (Q', dO and the statistics in LDS; a wave owns 16-key tiles): S = Q' K^T, dP = dO V^T with a key per lane
//             column, then dV^T += dO^T P and dK^T += Q'^T dS the same way.
// Q is prescaled by scale * log2(e) so that P = exp2(s' - m'); 20 + 16 MFMAs per 16 x 16 (query, key) tile.
// LDS rows are 16 floats; the four 16-byte chunks of a row are XOR-swizzled with (row >> 1) & 3 (conflict-free float4
// operand reads, like attn_f32_kernel's K image): bw_off / bw_elem of attn_train.h.
//
// DROP (cdseg_attention_drop_bwd): the forward was O = ((M / keep) o P) V with the mask M of include/cdseg.h.  Each kernel
// regenerates the mask factors f = M / keep of its tile from (seed, offset, patch, head, query, key) and uses
//   dP = (dO V^T) o f,   D = sum_j P dP,   dS = P (dP - D),   dV = (f o P)^T dO;
// the statistics (m, l) are those of the unmasked softmax.  The mask is a second kernel argument: kernel<DropP> takes it,
// kernel<> is the kernel as it was (same arguments, same code).
__device__ __forceinline__ DropP drop_arg() { return DropP{}; }
__device__ __forceinline__ DropP drop_arg(const DropP& d) { return d; }

template <typename... MASK>
__global__ __launch_bounds__(BW_WAVES * 64) void attn_bwd_q_mfma_kernel(AttnBwdP p, MASK... drop) {
  constexpr bool DROP = sizeof...(MASK) != 0;
  [[maybe_unused]] const DropP d = drop_arg(drop...);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Ks = smem;
  char* Vs = smem + BW_MAXL * 64;
  const int patch = blockIdx.x, head = blockIdx.y;
  const int ps = p.patch_start[patch], L = p.patch_start[patch + 1] - ps;
  const int nt = (L + 15) >> 4, Lp = nt << 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int s = tid; s < Lp; s += BW_WAVES * 64) {
    float4 kk[4], vv[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) kk[c] = vv[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (s < L) {
      const long r = p.kv_gidx[ps + s];
      const float4* kp = reinterpret_cast<const float4*>(p.k + r * p.ldk + head * HD);
      const float4* vp = reinterpret_cast<const float4*>(p.v + r * p.ldv + head * HD);
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
  for (int qt = wave; qt < nt; qt += BW_WAVES) {
    const int qslot = qt * 16 + ql;
    const bool valid = qslot < L;
    long qrow = 0;
    float qf[4] = {0.f, 0.f, 0.f, 0.f}, gf[4] = {0.f, 0.f, 0.f, 0.f};  // B operands: (query ql, head dims 4 g .. 4 g + 3)
    if (valid) {
      qrow = p.q_gidx[ps + qslot];
      const float4 t = *reinterpret_cast<const float4*>(p.q + qrow * p.ldq + head * HD + 4 * g);
      qf[0] = t.x * c2; qf[1] = t.y * c2; qf[2] = t.z * c2; qf[3] = t.w * c2;
      const int w = p.widx[ps + qslot];  // the slot's output row; padding duplicates have none: dO = 0
      if (w >= 0) {
        const float4 u = *reinterpret_cast<const float4*>(p.dout + (long)w * p.lddo + head * HD + 4 * g);
        gf[0] = u.x; gf[1] = u.y; gf[2] = u.z; gf[3] = u.w;
      }
    }
    auto tile = [&](int kt, f32x4_t& sc, f32x4_t& dp) {  // S'^T and dP^T of key tile kt: rows = keys 4 g + r, column = query ql
      const int key = kt * 16 + ql;
      const float4 kf = *reinterpret_cast<const float4*>(Ks + bw_off(key, g));
      const float4 vf = *reinterpret_cast<const float4*>(Vs + bw_off(key, g));
      const float ka[4] = {kf.x, kf.y, kf.z, kf.w}, va[4] = {vf.x, vf.y, vf.z, vf.w};
      sc = f32x4_t{0.f, 0.f, 0.f, 0.f};
      dp = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        sc = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[t], qf[t], sc, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_16x16x4f32(va[t], gf[t], dp, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (kt * 16 + 4 * g + r >= L) sc[r] = -INFINITY;
      if constexpr (DROP) {  // dP o f: keys 4 (4 kt + g) + r of query qslot
        float f[4];
        drop_keys4(d, patch, head, qslot, 4 * kt + g, f);
#pragma unroll
        for (int r = 0; r < 4; ++r) dp[r] *= f[r];
      }
    };
    // ---- sweep 1: online (m, l, sum e dP) over the lane's keys, then across the four lane groups of the query
    float m = -INFINITY, l = 0.f, dn = 0.f;
    for (int kt = 0; kt < nt; ++kt) {
      f32x4_t sc, dp;
      tile(kt, sc, dp);
      const float mt = fmaxf(fmaxf(sc[0], sc[1]), fmaxf(sc[2], sc[3]));
      const float mn = fmaxf(m, mt);
      if (mn > -INFINITY) {
        const float a = exp2f(m - mn);
        l *= a; dn *= a;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = exp2f(sc[r] - mn);
          l += e;
          dn = fmaf(e, dp[r], dn);
        }
        m = mn;
      }
    }
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
      const float m2 = __shfl_xor(m, off, 64), l2 = __shfl_xor(l, off, 64), d2 = __shfl_xor(dn, off, 64);
      const float mn = fmaxf(m, m2);
      if (mn > -INFINITY) {
        const float a = exp2f(m - mn), b = exp2f(m2 - mn);
        l = l * a + l2 * b;
        dn = dn * a + d2 * b;
      }
      m = mn;
    }
    const float il = 1.0f / l, D = dn * il;
    if (valid && g == 0) {
      float* st = p.stats + ((long)(ps + qslot) * p.num_heads + head) * 3;
      st[0] = m; st[1] = il; st[2] = D;
    }
    // ---- sweep 2: dQ^T (rows = head dims 4 g + r, column = query ql) += K^T dS^T
    f32x4_t dq = {0.f, 0.f, 0.f, 0.f};
    for (int kt = 0; kt < nt; ++kt) {
      f32x4_t sc, dp;
      tile(kt, sc, dp);
      float ds[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) ds[r] = exp2f(sc[r] - m) * il * (dp[r] - D);  // (masked keys: exp2(-inf) = 0)
#pragma unroll
      for (int t = 0; t < 4; ++t)  // k-slot g of MFMA t <-> key 4 g + t: A = K[key][head dim ql], B = register t
        dq = __builtin_amdgcn_mfma_f32_16x16x4f32(bw_elem(Ks, kt * 16 + 4 * g + t, ql), ds[t], dq, 0, 0, 0);
    }
    if (valid) {
      float* o = p.dq + qrow * p.lddq + head * HD + 4 * g;  // a point padded into two slots collects both
#pragma unroll
      for (int r = 0; r < 4; ++r) atomicAdd(o + r, dq[r] * p.scale);
    }
  }
}

template <typename... MASK>
__global__ __launch_bounds__(BW_WAVES * 64) void attn_bwd_kv_mfma_kernel(AttnBwdP p, MASK... drop) {
  constexpr bool DROP = sizeof...(MASK) != 0;
  [[maybe_unused]] const DropP d = drop_arg(drop...);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Qs = smem;                                                     // Q' = Q * scale * log2(e)
  char* Gs = smem + BW_MAXL * 64;                                      // dO
  float* sm = reinterpret_cast<float*>(smem + 2 * BW_MAXL * 64);       // m
  float* sil = sm + BW_MAXL;                                           // 1 / l
  float* sD = sil + BW_MAXL;                                           // D
  const int patch = blockIdx.x, head = blockIdx.y;
  const int ps = p.patch_start[patch], L = p.patch_start[patch + 1] - ps;
  const int nt = (L + 15) >> 4, Lp = nt << 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float c2 = p.scale * 1.44269504088896340736f;
  for (int s = tid; s < Lp; s += BW_WAVES * 64) {
    float4 qq[4], gg[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) qq[c] = gg[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    float m = INFINITY, il = 0.f, D = 0.f;  // slots past the end: P = exp2(0 - inf) = 0
    if (s < L) {
      const long r = p.q_gidx[ps + s];
      const float4* qp = reinterpret_cast<const float4*>(p.q + r * p.ldq + head * HD);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float4 t = qp[c];
        qq[c] = make_float4(t.x * c2, t.y * c2, t.z * c2, t.w * c2);
      }
      const int w = p.widx[ps + s];
      if (w >= 0) {
        const float4* gp = reinterpret_cast<const float4*>(p.dout + (long)w * p.lddo + head * HD);
#pragma unroll
        for (int c = 0; c < 4; ++c) gg[c] = gp[c];
      }
      const float* st = p.stats + ((long)(ps + s) * p.num_heads + head) * 3;
      m = st[0]; il = st[1]; D = st[2];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      *reinterpret_cast<float4*>(Qs + bw_off(s, c)) = qq[c];
      *reinterpret_cast<float4*>(Gs + bw_off(s, c)) = gg[c];
    }
    sm[s] = m; sil[s] = il; sD[s] = D;
  }
  __syncthreads();
  const int kl = lane & 15, g = lane >> 4;
  for (int kt = wave; kt < nt; kt += BW_WAVES) {
    const int kslot = kt * 16 + kl;
    const bool valid = kslot < L;
    long krow = 0;
    float kf[4] = {0.f, 0.f, 0.f, 0.f}, vf[4] = {0.f, 0.f, 0.f, 0.f};  // B operands: (key kl, head dims 4 g .. 4 g + 3)
    if (valid) {
      krow = p.kv_gidx[ps + kslot];
      const float4 a = *reinterpret_cast<const float4*>(p.k + krow * p.ldk + head * HD + 4 * g);
      const float4 b = *reinterpret_cast<const float4*>(p.v + krow * p.ldv + head * HD + 4 * g);
      kf[0] = a.x; kf[1] = a.y; kf[2] = a.z; kf[3] = a.w;
      vf[0] = b.x; vf[1] = b.y; vf[2] = b.z; vf[3] = b.w;
    }
    f32x4_t dk = {0.f, 0.f, 0.f, 0.f}, dv = {0.f, 0.f, 0.f, 0.f};  // rows = head dims 4 g + r, column = key kl
    for (int qt = 0; qt < nt; ++qt) {
      const int qrow = qt * 16 + kl;  // A operand row = query qt * 16 + (lane & 15)
      const float4 qa4 = *reinterpret_cast<const float4*>(Qs + bw_off(qrow, g));
      const float4 ga4 = *reinterpret_cast<const float4*>(Gs + bw_off(qrow, g));
      const float qa[4] = {qa4.x, qa4.y, qa4.z, qa4.w}, ga[4] = {ga4.x, ga4.y, ga4.z, ga4.w};
      f32x4_t sc = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};  // rows = queries 4 g + r, column = key kl
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        sc = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[t], kf[t], sc, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[t], vf[t], dp, 0, 0, 0);
      }
      const float4 m4 = *reinterpret_cast<const float4*>(sm + qt * 16 + 4 * g);
      const float4 i4 = *reinterpret_cast<const float4*>(sil + qt * 16 + 4 * g);
      const float4 D4 = *reinterpret_cast<const float4*>(sD + qt * 16 + 4 * g);
      const float ms[4] = {m4.x, m4.y, m4.z, m4.w}, is[4] = {i4.x, i4.y, i4.z, i4.w}, Ds[4] = {D4.x, D4.y, D4.z, D4.w};
      float pr[4], ds[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        pr[r] = exp2f(sc[r] - ms[r]) * is[r];
        if constexpr (!DROP) ds[r] = pr[r] * (dp[r] - Ds[r]);
      }
      if constexpr (DROP) {  // queries 4 (4 qt + g) + r of key kslot: dS from the masked dP, then f o P for dV
        float f[4];
        drop_queries4(d, patch, head, 4 * qt + g, kslot, f);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          ds[r] = pr[r] * (dp[r] * f[r] - Ds[r]);
          pr[r] *= f[r];
        }
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {  // k-slot g of MFMA t <-> query 4 g + t: A = dO / Q' [query][head dim kl], B = register t
        const int qq = qt * 16 + 4 * g + t;
        dv = __builtin_amdgcn_mfma_f32_16x16x4f32(bw_elem(Gs, qq, kl), pr[t], dv, 0, 0, 0);
        dk = __builtin_amdgcn_mfma_f32_16x16x4f32(bw_elem(Qs, qq, kl), ds[t], dk, 0, 0, 0);
      }
    }
    if (valid) {
      float* ok = p.dk + krow * p.lddk + head * HD + 4 * g;
      float* ov = p.dv + krow * p.lddv + head * HD + 4 * g;
      const float ln2 = 0.69314718055994530942f;  // Q' carries scale * log2(e): dK = scale dS^T Q = ln 2 dS^T Q'
#pragma unroll
      for (int r = 0; r < 4; ++r) { atomicAdd(ok + r, dk[r] * ln2); atomicAdd(ov + r, dv[r]); }
    }
  }
}

constexpr int BW_Q_LDS = 2 * BW_MAXL * 64;
constexpr int BW_KV_LDS = 2 * BW_MAXL * 64 + 3 * BW_MAXL * 4;

// ------------------------------------------------------------------------------------ 16-bit attention backward
// The recompute-P backward of attn_bf16_kernel on the 16-bit matrix pipe (v_mfma_f32_32x32x16_{bf16,f16}).  The function
// differentiated is the one that kernel computes: q' = q * fp32(scale * log2 e) rounded ONCE to the 16-bit type (treated
// as the identity in the chain rule), s' = q'.k, P = exp2(s' - m') / l.  Rounding points are flash-attention's: P and
// dS = P o (dP - D) are rounded to the 16-bit type as MFMA operands and nowhere else; the statistics (m', l, D) and every
// accumulator are fp32.  Unlike the forward's loop this one always subtracts the exact row maximum, so rows with |s'| of
// hundreds come out finite.  dO is never clamped and dS is converted WITHOUT saturation (half build): a scaled gradient
// beyond half's range reaches dq / dk / dv as inf / NaN, which is what a GradScaler looks for.
// Same two-kernel split and slot plan as the fp32 form, 32 x 32 (query, key) tiles, 8 waves, two blocks per CU; blockIdx.z
// deals a patch-head's tiles to 1, 2 or 4 blocks (results differ by the order of the fp32 atomics only):
//   q kernel  (K, V row-major in LDS, 32 KB each; a wave owns 32-query tiles): S'^T = K Q'^T and dP^T = V dO^T have a query
//             per lane column and 16 keys per lane.  Sweep 1: online (m', l, sum e dP) -> M = m' + log2 l and D per query
//             (P = exp2(s' - M): the normalisation costs nothing per score).  Sweep 2: -M is the MFMA's C operand, dS^T goes
//             from the accumulator registers into dQ^T += K^T dS^T as the B operand (k-slots <-> keys as in the forward's
//             P V product) and K^T is two ds_read_b64_tr_b16 of the row-major K;
//   kv kernel (Q', dO row-major in LDS, -M and D per query; a wave owns 32-key tiles): S' - M = Q' K^T + (-M) and
//             dP = dO V^T with a key per lane column, then dV^T += dO^T P and dK^T += Q'^T dS the same way.
// The transposed products use rows 0 .. 15 (the head dims) of the 32-row MFMA; rows 16 .. 31 repeat them and are dropped.
// 2 + 4 and 6 MFMAs per tile against 16 + 17 v_exp_f32 and 24 conversions: like the forward, VALU-bound.
// LDS rows are 32 bytes; the two 16-byte halves are swapped for rows with bit 3 set (conflict-free 16-byte operand reads,
// the forward's K image).  Every (slot, head, dim) result leaves with one fp32 atomic, as in the fp32 form.
// Reproducibility (both forms, any blockIdx.z split): the buffers start at zero and a row sits in at most TWO slots - the
// padding plan copies the tail of the previous patch once - so a dq / dk / dv element receives at most two adds, and
// 0 + a + b = 0 + b + a in fp32: the result does not depend on the order the atomics arrive in
// (tests/test_gpu_deterministic.py pins this on launches whose rows sit in at most two slots; a plan that put a row into
// three slots would need a per-row reduce).
constexpr int B16_Q_LDS = 2 * B16_IMG;
constexpr int B16_KV_LDS = 2 * B16_IMG + 2 * BW_MAXL * 4;

struct AttnBwd16P {
  const bf16_t* q; const bf16_t* k; const bf16_t* v; const bf16_t* dout;
  const int32_t* q_gidx; const int32_t* kv_gidx; const int32_t* widx; const int32_t* patch_start;
  float* dq; float* dk; float* dv;
  float* stats;  // (slot, head, {M = m' + log2 l, D})
  int ldq, ldk, ldv, lddo, lddq, lddk, lddv;
  int num_heads;
  float scale;
};

template <typename... MASK>
__global__ __launch_bounds__(B16_WAVES * 64, 4) void attn_bwd16_q_kernel(AttnBwd16P p, MASK... drop) {
  constexpr bool DROP = sizeof...(MASK) != 0;
  [[maybe_unused]] const DropP d = drop_arg(drop...);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Ks = smem;
  char* Vs = smem + B16_IMG;
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
      kk = *reinterpret_cast<const uint4*>(p.k + r * p.ldk + head * HD + hs * 8);
      vv = *reinterpret_cast<const uint4*>(p.v + r * p.ldv + head * HD + hs * 8);
    }
    const int o = b16_off(s, 2 * hs);
    *reinterpret_cast<uint4*>(Ks + o) = kk;
    *reinterpret_cast<uint4*>(Vs + o) = vv;
  }
  __syncthreads();
  const int ql = lane & 31, h = lane >> 5;
  const float c2 = p.scale * 1.44269504088896340736f;
  const int row_off = b16_off(ql, 2 * h);  // A operand of S'^T / dP^T: key ql of the tile, head dims 8 h .. 8 h + 7
  // K^T fragments: the lane's 16-lane group reads keys 4 h + {0 .. 3} (and + 8) of a 16-key half tile
  const unsigned tr0 = lds_base + b16_off(4 * h + ((lane & 15) >> 2), lane & 3);
  const unsigned tr1 = lds_base + b16_off(4 * h + ((lane & 15) >> 2) + 8, lane & 3);
  const f32x16_t zero16 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  // (DROP) dP o f: registers 4 c .. 4 c + 3 are keys 32 kt + 8 c + 4 h + {0 .. 3} of the lane's query
  auto drop_dp = [&](int kt, int query, f32x16_t& dp) {
    float f[16];
    drop_keys16(d, patch, head, query, 8 * kt + h, f);
#pragma unroll
    for (int r = 0; r < 16; ++r) dp[r] *= f[r];
  };
  for (int qt = blockIdx.z * B16_WAVES + wave; qt < nt; qt += B16_WAVES * gridDim.z) {
    const int qslot = qt * 32 + ql;
    const bool valid = qslot < L;
    long qrow = 0;
    uint4 qraw = make_uint4(0, 0, 0, 0), graw = qraw;  // B operands: (query ql, head dims 8 h .. 8 h + 7)
    if (valid) {
      qrow = p.q_gidx[ps + qslot];
      qraw = *reinterpret_cast<const uint4*>(p.q + qrow * p.ldq + head * HD + 8 * h);
      const int w = p.widx[ps + qslot];  // the slot's output row; padding duplicates have none: dO = 0
      if (w >= 0) graw = *reinterpret_cast<const uint4*>(p.dout + (long)w * p.lddo + head * HD + 8 * h);
    }
    const bf16x8_t qf = b16_frag(b16_prescale(qraw, c2)), gf = b16_frag(graw);
    // ---- sweep 1: online (m', l, sum e dP) over the lane's keys (rows (r & 3) + 8 (r >> 2) + 4 h of each tile)
    float m = -INFINITY, l = 0.f, dn = 0.f;
    for (int kt = 0; kt < nt; ++kt) {
      f32x16_t sc = mfma_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(Ks + kt * 1024 + row_off), qf, zero16);
      f32x16_t dp = mfma_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(Vs + kt * 1024 + row_off), gf, zero16);
      if constexpr (DROP) drop_dp(kt, qslot, dp);
      if (kt == nt - 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h >= L) sc[r] = -INFINITY;
      }
      float mn = m;
#pragma unroll
      for (int r = 0; r < 16; ++r) mn = fmaxf(mn, sc[r]);
      if (mn > -INFINITY) {
        const float a = __builtin_amdgcn_exp2f(m - mn);
        l *= a; dn *= a;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float e = __builtin_amdgcn_exp2f(sc[r] - mn);
          l += e;
          dn = fmaf(e, dp[r], dn);
        }
        m = mn;
      }
    }
    {
      const float m2 = __shfl_xor(m, 32, 64), l2 = __shfl_xor(l, 32, 64), d2 = __shfl_xor(dn, 32, 64);
      const float mn = fmaxf(m, m2);
      if (mn > -INFINITY) {
        const float a = __builtin_amdgcn_exp2f(m - mn), b = __builtin_amdgcn_exp2f(m2 - mn);
        l = l * a + l2 * b;
        dn = dn * a + d2 * b;
      }
      m = mn;
    }
    const float M = m + __builtin_amdgcn_logf(l), D = dn / l;  // (v_log_f32 = log2)
    if (valid && h == 0) {
      float* st = p.stats + ((long)(ps + qslot) * p.num_heads + head) * 2;
      st[0] = M; st[1] = D;
    }
    // ---- sweep 2: dQ^T (rows = head dims, column = query ql) += K^T dS^T
    const float nm = valid ? -M : 0.f;
    const f32x16_t negm = {nm, nm, nm, nm, nm, nm, nm, nm, nm, nm, nm, nm, nm, nm, nm, nm};
    f32x16_t dq = zero16;
    for (int kt = 0; kt < nt; ++kt) {
      const f32x16_t sc = mfma_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(Ks + kt * 1024 + row_off), qf, negm);
      f32x16_t dp = mfma_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(Vs + kt * 1024 + row_off), gf, zero16);
      if constexpr (DROP) drop_dp(kt, qslot, dp);
      float ds[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) ds[r] = __builtin_amdgcn_exp2f(sc[r]) * (dp[r] - D);
      if (kt == nt - 1) {  // keys past the end of a ragged patch (their K rows are zero: s' = 0, not -inf)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h >= L) ds[r] = 0.f;
      }
#pragma unroll
      for (int mf = 0; mf < 2; ++mf) {
        const bf16x8_t kT = b16_tr_pair(tr0 + kt * 1024 + mf * 512, tr1 + kt * 1024 + mf * 512);
        dq = mfma_32x32x16_bf16(kT, b16_pack8(ds + 8 * mf), dq);
      }
    }
    if (valid) {  // rows 4 h + (r & 3) + 8 (r >> 2), r < 8; a point padded into two slots collects both
      float* o = p.dq + qrow * p.lddq + head * HD + 4 * h;
#pragma unroll
      for (int r = 0; r < 8; ++r) atomicAdd(o + (r & 3) + 8 * (r >> 2), dq[r] * p.scale);
    }
  }
}

template <typename... MASK>
__global__ __launch_bounds__(B16_WAVES * 64, 4) void attn_bwd16_kv_kernel(AttnBwd16P p, MASK... drop) {
  constexpr bool DROP = sizeof...(MASK) != 0;
  [[maybe_unused]] const DropP d = drop_arg(drop...);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Qs = smem;                                                   // Q' = round16(Q * scale * log2 e)
  char* Gs = smem + B16_IMG;                                         // dO
  float* sNM = reinterpret_cast<float*>(smem + 2 * B16_IMG);         // -M (-inf for the slots past the end: P = 0)
  float* sD = sNM + BW_MAXL;
  const unsigned lds_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  const int patch = blockIdx.x, head = blockIdx.y;
  const int ps = p.patch_start[patch], L = p.patch_start[patch + 1] - ps;
  const int nt = (L + 31) >> 5;
  if ((int)blockIdx.z * B16_WAVES >= nt) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float c2 = p.scale * 1.44269504088896340736f;
  for (int i = tid; i < nt * 64; i += B16_WAVES * 64) {
    const int s = i >> 1, hs = i & 1;
    uint4 qq = make_uint4(0, 0, 0, 0), gg = qq;
    float nM = -INFINITY, D = 0.f;
    if (s < L) {
      const long r = p.q_gidx[ps + s];
      qq = b16_prescale(*reinterpret_cast<const uint4*>(p.q + r * p.ldq + head * HD + hs * 8), c2);
      const int w = p.widx[ps + s];
      if (w >= 0) gg = *reinterpret_cast<const uint4*>(p.dout + (long)w * p.lddo + head * HD + hs * 8);
      const float* st = p.stats + ((long)(ps + s) * p.num_heads + head) * 2;
      nM = -st[0]; D = st[1];
    }
    const int o = b16_off(s, 2 * hs);
    *reinterpret_cast<uint4*>(Qs + o) = qq;
    *reinterpret_cast<uint4*>(Gs + o) = gg;
    if (hs == 0) { sNM[s] = nM; sD[s] = D; }
  }
  __syncthreads();
  const int kl = lane & 31, h = lane >> 5;
  const int row_off = b16_off(kl, 2 * h);
  const unsigned tr0 = lds_base + b16_off(4 * h + ((lane & 15) >> 2), lane & 3);
  const unsigned tr1 = lds_base + b16_off(4 * h + ((lane & 15) >> 2) + 8, lane & 3);
  const f32x16_t zero16 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int kt = blockIdx.z * B16_WAVES + wave; kt < nt; kt += B16_WAVES * gridDim.z) {
    const int kslot = kt * 32 + kl;
    const bool valid = kslot < L;
    long krow = 0;
    uint4 kraw = make_uint4(0, 0, 0, 0), vraw = kraw;  // B operands: (key kl, head dims 8 h .. 8 h + 7)
    if (valid) {
      krow = p.kv_gidx[ps + kslot];
      kraw = *reinterpret_cast<const uint4*>(p.k + krow * p.ldk + head * HD + 8 * h);
      vraw = *reinterpret_cast<const uint4*>(p.v + krow * p.ldv + head * HD + 8 * h);
    }
    const bf16x8_t kf = b16_frag(kraw), vf = b16_frag(vraw);
    f32x16_t dk = zero16, dv = zero16;  // rows = head dims, column = key kl
    for (int qt = 0; qt < nt; ++qt) {
      // rows = queries (r & 3) + 8 (r >> 2) + 4 h of the tile: their -M is the C operand, so S' - M leaves the MFMA
      f32x16_t cm, Dr;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 a = *reinterpret_cast<const float4*>(sNM + qt * 32 + 8 * j + 4 * h);
        const float4 b = *reinterpret_cast<const float4*>(sD + qt * 32 + 8 * j + 4 * h);
        cm[4 * j] = a.x; cm[4 * j + 1] = a.y; cm[4 * j + 2] = a.z; cm[4 * j + 3] = a.w;
        Dr[4 * j] = b.x; Dr[4 * j + 1] = b.y; Dr[4 * j + 2] = b.z; Dr[4 * j + 3] = b.w;
      }
      const f32x16_t sc = mfma_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(Qs + qt * 1024 + row_off), kf, cm);
      const f32x16_t dp = mfma_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(Gs + qt * 1024 + row_off), vf, zero16);
      float pr[16], ds[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        pr[r] = __builtin_amdgcn_exp2f(sc[r]);
        if constexpr (!DROP) ds[r] = pr[r] * (dp[r] - Dr[r]);
      }
      if constexpr (DROP) {  // registers 4 c .. 4 c + 3 are queries 32 qt + 8 c + 4 h + {0 .. 3} of the lane's key
        float f[16];
        drop_queries16(d, patch, head, 8 * qt + h, kslot, f);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          ds[r] = pr[r] * (dp[r] * f[r] - Dr[r]);
          pr[r] *= f[r];
        }
      }
#pragma unroll
      for (int mf = 0; mf < 2; ++mf) {
        const unsigned o0 = tr0 + qt * 1024 + mf * 512, o1 = tr1 + qt * 1024 + mf * 512;
        dv = mfma_32x32x16_bf16(b16_tr_pair(o0 + B16_IMG, o1 + B16_IMG), b16_pack8(pr + 8 * mf), dv);
        dk = mfma_32x32x16_bf16(b16_tr_pair(o0, o1), b16_pack8(ds + 8 * mf), dk);
      }
    }
    if (valid) {
      float* ok = p.dk + krow * p.lddk + head * HD + 4 * h;
      float* ov = p.dv + krow * p.lddv + head * HD + 4 * h;
      const float ln2 = 0.69314718055994530942f;  // Q' carries scale * log2(e): dK = scale dS^T Q = ln 2 dS^T Q'
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        atomicAdd(ok + (r & 3) + 8 * (r >> 2), dk[r] * ln2);
        atomicAdd(ov + (r & 3) + 8 * (r >> 2), dv[r]);
      }
    }
  }
}

// ---- LayerNorm backward: dx = (1/sigma) (dyg - mean(dyg) - xhat mean(dyg xhat)), dyg = dy * gamma.  One wave per row, 16 rows
// per wave; d gamma / d beta are summed over the block's 64 rows in registers + LDS and leave with ONE atomic per column
// and block (the first version issued one atomic per element onto C addresses: 82 of a 450 ms training step).
// Rows wider than LNB_MAXC (no layer of the model has them) get the same block sums in passes of LNB_MAXC columns.
constexpr int LNB_ROWS = 16, LNB_MAXC = 512;

// DET (deterministic form, c <= LNB_MAXC): the block's (dgamma, dbeta) partial rows go to ws[block][2][c] with plain stores;
// layernorm_det_reduce_kernel adds them by ascending block index.  The in-block part is the same in both forms.
template <bool DET>
__device__ __forceinline__ void layernorm_bwd_body(const float* __restrict__ x, int ldx, const float* __restrict__ gamma, float eps,
                                                   const float* __restrict__ dy, int lddy, float* dx, int lddx, int accumulate,
                                                   float* dgamma, float* dbeta, long m, int c, float* ws) {
  __shared__ float red[2][4][LNB_MAXC];
  __shared__ float rstat[4][LNB_ROWS][2];  // wide rows: (mean, 1 / sigma) of the wave's rows, for the column passes below
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long row0 = ((long)blockIdx.x * 4 + wave) * LNB_ROWS;
  const bool sums = DET || ((dgamma || dbeta) && c <= LNB_MAXC);
  const bool wide = !DET && (dgamma || dbeta) && c > LNB_MAXC;
  float pg[LNB_MAXC / 64], pb[LNB_MAXC / 64];
#pragma unroll
  for (int t = 0; t < LNB_MAXC / 64; ++t) pg[t] = pb[t] = 0.f;
  for (int r = 0; r < LNB_ROWS; ++r) {
    const long row = row0 + r;
    if (row >= m) break;
    const float* xr = x + row * ldx;
    const float* gr = dy + row * lddy;
    float s = 0.f, ss = 0.f;
    for (int j = lane; j < c; j += 64) { const float t = xr[j]; s += t; }
    s = wave_sum(s);
    const float mean = s / c;
    for (int j = lane; j < c; j += 64) { const float t = xr[j] - mean; ss = fmaf(t, t, ss); }
    ss = wave_sum(ss);
    const float rstd = rsqrtf(ss / c + eps);
    float a = 0.f, b = 0.f;
    for (int j = lane; j < c; j += 64) {
      const float xh = (xr[j] - mean) * rstd, dg = gr[j] * gamma[j];
      a += dg;
      b = fmaf(dg, xh, b);
    }
    a = wave_sum(a) / c;
    b = wave_sum(b) / c;
    if (sums) {
#pragma unroll
      for (int t = 0; t < LNB_MAXC / 64; ++t) {
        const int j = lane + 64 * t;
        if (j < c) {
          const float xh = (xr[j] - mean) * rstd, g = gr[j], dg = g * gamma[j];
          const float v = rstd * (dg - a - xh * b);
          float* o = dx + row * lddx + j;
          *o = accumulate ? *o + v : v;
          pg[t] = fmaf(g, xh, pg[t]);
          pb[t] += g;
        }
      }
    } else {
      for (int j = lane; j < c; j += 64) {
        const float xh = (xr[j] - mean) * rstd, dg = gr[j] * gamma[j];
        const float v = rstd * (dg - a - xh * b);
        float* o = dx + row * lddx + j;
        *o = accumulate ? *o + v : v;
      }
      if (wide && lane == 0) { rstat[wave][r][0] = mean; rstat[wave][r][1] = rstd; }
    }
  }
  if (wide) {  // (block-uniform) rows wider than LNB_MAXC: the block sums of the narrow form, LNB_MAXC columns at a time.
    // (One atomic per row and element, as this branch used to issue, is a serial fp32 chain of m adds per column: at
    // m = 777 its error was nine times that of the narrow form - tests/test_gpu_train_fp32.py, layernorm (777, 640).)
    __syncthreads();
    const long left = m - row0;
    const int nrows = left < 0 ? 0 : left < LNB_ROWS ? (int)left : LNB_ROWS;
    for (int cb = 0; cb < c; cb += LNB_MAXC) {
#pragma unroll
      for (int t = 0; t < LNB_MAXC / 64; ++t) pg[t] = pb[t] = 0.f;
      for (int r = 0; r < nrows; ++r) {
        const float* xr = x + (row0 + r) * ldx;
        const float* gr = dy + (row0 + r) * lddy;
        const float mean = rstat[wave][r][0], rstd = rstat[wave][r][1];
#pragma unroll
        for (int t = 0; t < LNB_MAXC / 64; ++t) {
          const int j = cb + lane + 64 * t;
          if (j < c) {
            const float g = gr[j];
            pg[t] = fmaf(g, (xr[j] - mean) * rstd, pg[t]);
            pb[t] += g;
          }
        }
      }
#pragma unroll
      for (int t = 0; t < LNB_MAXC / 64; ++t) { red[0][wave][lane + 64 * t] = pg[t]; red[1][wave][lane + 64 * t] = pb[t]; }
      __syncthreads();
      for (int j = threadIdx.x; j < LNB_MAXC && cb + j < c; j += 256) {
        if (dgamma) atomicAdd(dgamma + cb + j, (red[0][0][j] + red[0][1][j]) + (red[0][2][j] + red[0][3][j]));
        if (dbeta) atomicAdd(dbeta + cb + j, (red[1][0][j] + red[1][1][j]) + (red[1][2][j] + red[1][3][j]));
      }
      __syncthreads();  // (red is refilled by the next pass)
    }
    return;
  }
  if (!sums) return;  // (block-uniform)
#pragma unroll
  for (int t = 0; t < LNB_MAXC / 64; ++t) {
    const int j = lane + 64 * t;
    if (j < c) { red[0][wave][j] = pg[t]; red[1][wave][j] = pb[t]; }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < c; j += 256) {
    const float g = (red[0][0][j] + red[0][1][j]) + (red[0][2][j] + red[0][3][j]);
    const float b = (red[1][0][j] + red[1][1][j]) + (red[1][2][j] + red[1][3][j]);
    if constexpr (DET) {
      float* o = ws + (long)blockIdx.x * 2 * c + j;
      o[0] = g; o[c] = b;
    } else {
      if (dgamma) atomicAdd(dgamma + j, g);
      if (dbeta) atomicAdd(dbeta + j, b);
    }
  }
}

__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ gamma,
                                                            float eps, const float* __restrict__ dy, int lddy, float* dx, int lddx,
                                                            int accumulate, float* dgamma, float* dbeta, long m, int c) {
  layernorm_bwd_body<false>(x, ldx, gamma, eps, dy, lddy, dx, lddx, accumulate, dgamma, dbeta, m, c, nullptr);
}

__global__ __launch_bounds__(256) void layernorm_bwd_det_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ gamma,
                                                                float eps, const float* __restrict__ dy, int lddy, float* dx, int lddx,
                                                                int accumulate, long m, int c, float* ws) {
  layernorm_bwd_body<true>(x, ldx, gamma, eps, dy, lddy, dx, lddx, accumulate, nullptr, nullptr, m, c, ws);
}

// Thread i < c: column i of dgamma, thread c + j: column j of dbeta: t = p[0]; t += p[1]; ... by ascending block index, then ONE add onto
// the existing content.  The loads of a column are independent of each other (only the adds are a chain).
__global__ __launch_bounds__(64) void layernorm_det_reduce_kernel(const float* __restrict__ ws, long nblocks, int c, float* dgamma,
                                                                  float* dbeta) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= 2 * c) return;
  float* out = i < c ? dgamma : dbeta;
  if (!out) return;
  const float* p = ws + i;
  float t = p[0];
#pragma unroll 16
  for (long b = 1; b < nblocks; ++b) t += p[b * 2 * c];
  const int j = i < c ? i : i - c;
  out[j] = out[j] + t;
}

// ---- exact (erf) GELU backward on the pre-activation: dx = dy * (Phi(u) + u phi(u))
__global__ void gelu_bwd_kernel(const float* __restrict__ u, const float* __restrict__ dy, float* __restrict__ dx, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float t = u[i];
  const float cdf = 0.5f * (1.0f + erff(t * 0.70710678118654752440f));
  const float pdf = 0.39894228040143267794f * expf(-0.5f * t * t);
  dx[i] = dy[i] * (cdf + t * pdf);
}

// ---- weight gradient of a Linear / of one kernel offset of a submanifold conv:
//        dW[n][k] += sum_m dY[m][n] * X[row(m)][k],   row(m) = xidx ? xidx[m] (-1: no neighbour, skipped) : m
//      (+ db[n] += sum_m dY[m][n]).   ref: what autograd does for nn.Linear (ptv3.py:399-428) and spconv.SubMConv3d
//      (ptv3.py:356-362) weights; dW = dY^T X is a GEMM whose reduction runs over the ROWS (10^5 .. 10^6), so the rows are
//      split over blockIdx.z and the partial tiles are added with fp32 atomics (summation order not fixed: ~1e-7 relative).
//      v_mfma_f32_16x16x4_f32 straight from global memory: A[i][kk] = dY[m0 + kk][n0 + i], B[kk][j] = X[row(m0 + kk)][k0 + j]
//      (lane = i + 16 kk); a block is 4 waves = a 64 (n) x 64 (k) tile of dW.  Not tuned (first slice).
struct WgradP {
  const float* dy; const float* x; const int32_t* xidx; float* dw; float* db;
  long M, rows_per_split, idx_stride;  // idx_stride: elements between the index rows of consecutive offsets (conv form)
  int N, K, lddy, ldx, lddw;
  int splits, dw_off_stride;           // blockIdx.z = offset * splits + split; offset o adds o * dw_off_stride to dw
};

// DET (deterministic form): the block's partial dW tile goes to ws_dw[blockIdx.z][N][K] and its db partial to
// ws_db[split][N] with plain stores (every element of both is written by exactly one thread: a split without live rows
// stores zeros); wgrad_det_reduce_kernel adds them in ascending split order.  Same tiling, loop and row partition.
template <bool DET>
__device__ __forceinline__ void wgrad_body(const WgradP& p, float* ws_dw, float* ws_db) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i16 = lane & 15, kq = lane >> 4;
  const int n0 = blockIdx.x * 64 + wave * 16, k0 = blockIdx.y * 64;
  if (n0 >= p.N) return;
  const int off = blockIdx.z / p.splits;  // kernel offset (conv form; 0 for a Linear)
  const long m_begin = (long)(blockIdx.z - off * p.splits) * p.rows_per_split;
  const long m_end = min(p.M, m_begin + p.rows_per_split);
  const int32_t* xidx = p.xidx ? p.xidx + off * p.idx_stride : nullptr;
  float* dw = p.dw + (long)off * p.dw_off_stride;
  f32x4_t acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;
  bool kt_ok[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) kt_ok[t] = k0 + 16 * t < p.K;
#pragma unroll 4
  for (long m0 = m_begin; m0 < m_end; m0 += 4) {
    const long m = m0 + kq;
    float a = 0.f, b[4] = {0.f, 0.f, 0.f, 0.f};
    if (m < m_end) {
      a = p.dy[m * p.lddy + n0 + i16];
      const long row = xidx ? (long)xidx[m] : m;
      if (row >= 0) {
        const float* xr = p.x + row * p.ldx + k0 + i16;
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if (kt_ok[t]) b[t] = xr[16 * t];
      }
    }
    bsum += a;
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[t], acc[t], 0, 0, 0);
  }
  // D[i][j]: lane holds j = lane & 15, i = 4 (lane >> 4) + r
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (!kt_ok[t]) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if constexpr (DET) ws_dw[((long)blockIdx.z * p.N + n0 + 4 * kq + r) * p.K + k0 + 16 * t + i16] = acc[t][r];
      else atomicAdd(dw + (long)(n0 + 4 * kq + r) * p.lddw + k0 + 16 * t + i16, acc[t][r]);
    }
  }
  if (p.db && blockIdx.y == 0 && off == 0) {
    bsum += __shfl_xor(bsum, 16, 64);
    bsum += __shfl_xor(bsum, 32, 64);
    if (lane < 16) {
      if constexpr (DET) ws_db[(long)blockIdx.z * p.N + n0 + lane] = bsum;  // (off == 0: blockIdx.z is the split)
      else atomicAdd(p.db + n0 + lane, bsum);
    }
  }
}

__global__ __launch_bounds__(256) void wgrad_kernel(WgradP p) { wgrad_body<false>(p, nullptr, nullptr); }
__global__ __launch_bounds__(256) void wgrad_det_kernel(WgradP p, float* ws_dw, float* ws_db) { wgrad_body<true>(p, ws_dw, ws_db); }

// The fixed-order reduce of both deterministic weight gradients (fp32 and 16-bit operands leave the same fp32 partials):
// one thread per dW element (offset, n, k), then per db element:  t = p[0]; t += p[1]; ... by ascending split index, then ONE
// add onto the existing content (dw / db keep their accumulate-into contract).  No block waits for another: this is a launch
// of its own behind the partial kernel on the same stream.
struct WgradReduceP {
  const float* ws_dw; const float* ws_db; float* dw; float* db;
  int N, K, lddw, splits, noff, dw_off_stride;
};

__global__ __launch_bounds__(256) void wgrad_det_reduce_kernel(WgradReduceP r) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long nk = (long)r.N * r.K, total = nk * r.noff;
  if (i < total) {
    const long off = i / nk, e = i - off * nk;
    const int n = (int)(e / r.K), k = (int)(e - (long)n * r.K);
    const float* p = r.ws_dw + off * r.splits * nk + e;
    float t = p[0];
#pragma unroll 8
    for (int s = 1; s < r.splits; ++s) t += p[s * nk];
    float* o = r.dw + off * r.dw_off_stride + (long)n * r.lddw + k;
    *o = *o + t;
  } else if (r.db && i < total + r.N) {
    const int n = (int)(i - total);
    const float* p = r.ws_db + n;
    float t = p[0];
#pragma unroll 8
    for (int s = 1; s < r.splits; ++s) t += p[(long)s * r.N];
    r.db[n] = r.db[n] + t;
  }
}

// ---- the same weight gradient on 16-bit operands (the AMP step): dY and X are of the build's 16-bit type, products are
//      exact and every sum is fp32 (v_mfma_f32_32x32x16_{f16,bf16} accumulators, fp32 atomics; nothing is rounded to 16 bits).
//      The reduction index m is the ROW index of both operands, so both MFMA operands are column reads of row-major tiles:
//      a chunk of W16_ROWS rows of dY [rows][32 TN] and of (gathered) X [rows][32 TK] is staged row-major in LDS with 16-byte
//      loads and read with ds_read_b64_tr_b16 (as attn_bwd16_kv_kernel reads its transposed operands).
//      LDS image: one [W16_ROWS][32 columns] sub-image (64-byte rows, 4 KiB) per 32 columns.  A transposed read of a 32-lane
//      half takes rows r .. r + 3 x 32 columns = 256 contiguous bytes: all 64 banks once.
//      A block is 4 waves = a (32 TN) x (32 TK) tile of dW in 32 x 32 sub-tiles; wave w owns sub-tiles w, w + 4, ...
//      Columns past N / K are staged as zeros (C = 16 runs as a zero-padded 32-wide tile) and never stored.
//      Two LDS buffers: chunk c + 1 is loaded into registers while chunk c feeds the MFMAs, one barrier per chunk.  The
//      barrier also votes on whether chunk c + 1 has any live row (conv offsets are sparse): a dead chunk is not staged.
//      EXEC is all ones at every transposed read: branches around them are block- or wave-uniform, tiles are padded.
constexpr int W16_ROWS = 64;       // rows of a chunk (4 MFMA k-steps of 16)
constexpr int W16_SUB = W16_ROWS * 64;  // bytes of one 32-column sub-image

struct Wgrad16P {
  const bf16_t* dy; const bf16_t* x; const int32_t* xidx; float* dw; float* db;
  long M, rows_per_split, idx_stride;
  int N, K, lddy, ldx, lddw;
  int splits, dw_off_stride;
};

template <int TN, int TK, bool DET>
__device__ __forceinline__ void wgrad16_body(const Wgrad16P& p, float* ws_dw, float* ws_db) {
  constexpr int IMG = (TN + TK) * W16_SUB;               // one buffer: TN sub-images of dY, then TK of X
  constexpr int CN = TN * 4, CK = TK * 4;                // 16-byte column chunks per staged row
  constexpr int RN = 256 / CN, RK = 256 / CK;            // rows a pass of the block's 256 threads covers
  constexpr int NSUB = TN * TK, SPW = (NSUB + 3) / 4;    // sub-tiles, sub-tiles per wave
  __shared__ __attribute__((aligned(16))) char smem[2 * IMG];
  const unsigned lds_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * (32 * TN), k0 = blockIdx.y * (32 * TK);
  const int off = blockIdx.z / p.splits;
  const long m_begin = (long)(blockIdx.z - off * p.splits) * p.rows_per_split;
  const long m_end = min(p.M, m_begin + p.rows_per_split);
  const int32_t* xidx = p.xidx ? p.xidx + off * p.idx_stride : nullptr;
  float* dw = p.dw + (long)off * p.dw_off_stride;
  const bool want_db = p.db && blockIdx.y == 0 && off == 0;
  // staging: thread -> (row tid / CN + j RN, chunk tid % CN) of dY, (row tid / CK + j RK, chunk tid % CK) of X
  const int cn = tid % CN, rn = tid / CN, ck = tid % CK, rk = tid / CK;
  const bool n_ok = n0 + 8 * cn < p.N, k_ok = k0 + 8 * ck < p.K;
  const bf16_t* dyp = p.dy + n0 + 8 * cn;
  const bf16_t* xp = p.x + k0 + 8 * ck;
  const int st_n = (cn >> 2) * W16_SUB + rn * 64 + (cn & 3) * 16;
  const int st_k = (TN + (ck >> 2)) * W16_SUB + rk * 64 + (ck & 3) * 16;
  uint4 gn[TN], gk[TK];
  int32_t ridx[TK];  // gathered form: the thread's row indices of the chunk the next fetch() stages, loaded a chunk ahead
  float bsum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  auto fetch_idx = [&](long m0) {
#pragma unroll
    for (int j = 0; j < TK; ++j) {
      const long m = m0 + rk + j * RK;
      ridx[j] = (xidx && m < m_end) ? xidx[m] : -1;
    }
  };
  auto fetch = [&](long m0) -> bool {  // chunk m0 .. m0 + 63 into registers; true: this thread saw a live row
    bool live = false;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const long m = m0 + rn + j * RN;
      gn[j] = make_uint4(0, 0, 0, 0);
      if (n_ok && m < m_end) gn[j] = *reinterpret_cast<const uint4*>(dyp + m * p.lddy);
    }
#pragma unroll
    for (int j = 0; j < TK; ++j) {
      const long m = m0 + rk + j * RK;
      gk[j] = make_uint4(0, 0, 0, 0);
      const long row = xidx ? (long)ridx[j] : (m < m_end ? m : -1);
      if (row >= 0) {
        live = true;
        if (k_ok) gk[j] = *reinterpret_cast<const uint4*>(xp + row * p.ldx);
      }
    }
    fetch_idx(m0 + W16_ROWS);  // (the indices arrive while this chunk's rows do: the gather never waits for them)
    return live || want_db;
  };
  // operands: lane (i = lane & 31, h = lane >> 5) holds rows 8 h .. 8 h + 7 of a 16-row k-step at column i of its sub-image;
  // its 16-lane group g reads columns 16 (g & 1) ..: lane 4 q + pp of the group addresses row q, columns 4 pp .. 4 pp + 3
  const int tr = (8 * (lane >> 5) + ((lane & 15) >> 2)) * 64 + ((lane >> 4) & 1) * 32 + (lane & 3) * 8;
  int sub_n[SPW], sub_k[SPW];
#pragma unroll
  for (int j = 0; j < SPW; ++j) {
    const int s = wave + 4 * j;
    sub_n[j] = s % TN; sub_k[j] = (s / TN) % TK;  // (a wave without a sub-tile repeats one and stores nothing)
  }
  f32x16_t acc[SPW];
#pragma unroll
  for (int j = 0; j < SPW; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  const bool has_work = wave < NSUB;  // wave-uniform
  fetch_idx(m_begin);
  bool live = __syncthreads_or(fetch(m_begin)) != 0;
  int buf = 0;
  for (long m0 = m_begin; m0 < m_end; m0 += W16_ROWS) {
    if (live) {  // block-uniform
      char* img = smem + buf * IMG;
#pragma unroll
      for (int j = 0; j < TN; ++j) *reinterpret_cast<uint4*>(img + st_n + j * RN * 64) = gn[j];
#pragma unroll
      for (int j = 0; j < TK; ++j) *reinterpret_cast<uint4*>(img + st_k + j * RK * 64) = gk[j];
      if (want_db) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          float lo, hi;
          unpack_bf16x2(gn[j].x, lo, hi); bsum[0] += lo; bsum[1] += hi;
          unpack_bf16x2(gn[j].y, lo, hi); bsum[2] += lo; bsum[3] += hi;
          unpack_bf16x2(gn[j].z, lo, hi); bsum[4] += lo; bsum[5] += hi;
          unpack_bf16x2(gn[j].w, lo, hi); bsum[6] += lo; bsum[7] += hi;
        }
      }
    }
    const bool was_live = live;
    const bool mine = m0 + W16_ROWS < m_end ? fetch(m0 + W16_ROWS) : false;  // next chunk's loads fly over the MFMAs below
    live = __syncthreads_or(mine) != 0;
    if (was_live && has_work) {
      const unsigned img = lds_base + buf * IMG + tr;
#pragma unroll
      for (int ks = 0; ks < W16_ROWS / 16; ++ks) {
#pragma unroll
        for (int j = 0; j < SPW; ++j) {
          const unsigned a = img + sub_n[j] * W16_SUB + ks * 1024, b = img + (TN + sub_k[j]) * W16_SUB + ks * 1024;
          acc[j] = mfma_32x32x16_bf16(b16_tr_pair(a, a + 256), b16_tr_pair(b, b + 256), acc[j]);
        }
      }
    }
    if (was_live) buf ^= 1;
  }
  // D[i][jj]: lane holds column jj = lane & 31 (k), rows i = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (n)
#pragma unroll
  for (int j = 0; j < SPW; ++j) {
    if (wave + 4 * j >= NSUB) continue;
    const int kk = k0 + 32 * sub_k[j] + (lane & 31);
    const int nb = n0 + 32 * sub_n[j] + 4 * (lane >> 5);
    if (kk >= p.K) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int nn = nb + (r & 3) + 8 * (r >> 2);
      if (nn < p.N) {
        if constexpr (DET) ws_dw[((long)blockIdx.z * p.N + nn) * p.K + kk] = acc[j][r];
        else atomicAdd(dw + (long)nn * p.lddw + kk, acc[j][r]);
      }
    }
  }
  if (want_db) {  // (block-uniform) the threads' column sums: one fp32 sum per column in LDS, one atomic per column
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);  // [RN][32 TN]
#pragma unroll
    for (int e = 0; e < 8; ++e) red[rn * (32 * TN) + 8 * cn + e] = bsum[e];
    __syncthreads();
    if (tid < 32 * TN && n0 + tid < p.N) {
      float s = 0.f;
      for (int r = 0; r < RN; ++r) s += red[r * (32 * TN) + tid];
      if constexpr (DET) ws_db[(long)blockIdx.z * p.N + n0 + tid] = s;  // (off == 0: blockIdx.z is the split)
      else atomicAdd(p.db + n0 + tid, s);
    }
  }
}

template <int TN, int TK>
__global__ __launch_bounds__(256) void wgrad16_kernel(Wgrad16P p) { wgrad16_body<TN, TK, false>(p, nullptr, nullptr); }

// deterministic form (see wgrad_body): partial tiles and db partials to the workspace, reduced by wgrad_det_reduce_kernel
template <int TN, int TK>
__global__ __launch_bounds__(256) void wgrad16_det_kernel(Wgrad16P p, float* ws_dw, float* ws_db) {
  wgrad16_body<TN, TK, true>(p, ws_dw, ws_db);
}

// ---- segment sum: out[j] = sum of src rows seg_start[j] .. seg_start[j + 1] - 1 in ascending row order, fp32: the backward
//      of the unpooling gather child[cluster] (children of a pooled row are contiguous in the plan's physical order) without
//      atomics.  A wave covers 64 / cw coarse rows x cw columns (cw = 16, 32 or 64 lanes per row: coalesced row reads).
__global__ __launch_bounds__(256) void segment_sum_kernel(const float* __restrict__ src, int ld, const int32_t* __restrict__ seg,
                                                          long m, int c, float* __restrict__ out, int ldo, int cw) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rpw = 64 / cw;
  const long j = ((long)blockIdx.x * 4 + wave) * rpw + lane / cw;
  if (j >= m) return;
  const int a = seg[j], b = seg[j + 1];
  for (int col = lane % cw; col < c; col += cw) {
    float t = 0.f;
    for (int i = a; i < b; ++i) t += src[(long)i * ld + col];
    out[j * ldo + col] = t;
  }
}

}  // namespace

extern "C" size_t cdseg_attention_bwd_ws_bytes(long num_slots, int num_heads) {
  return (size_t)num_slots * num_heads * 3 * sizeof(float);
}

// drop: NULL = cdseg_attention_bwd; else the mask of cdseg_attention_drop_bwd (the kernel<DropP> instantiations)
static int attention_bwd_launch(const void* q, const void* k, const void* v, int ldq, int ldk, int ldv, const int32_t* q_gidx,
                                const int32_t* kv_gidx, const int32_t* widx, const int32_t* patch_start, int num_patches,
                                int num_heads, long num_slots, int max_len, float scale, const void* dout, int lddo, void* dq,
                                void* dk, void* dv, int lddq, int lddk, int lddv, int dtype, void* ws, size_t ws_bytes, void* stream,
                                const DropP* drop) {
  if (num_patches <= 0 || num_heads <= 0) return CDSEG_OK;
  if (dtype != CDSEG_F32 && dtype != CDSEG_BF16) return CDSEG_ERR_UNSUPPORTED;
  // the patch-head lives in LDS (like the forward): a longer patch would write past the staged K / V / statistics
  if (max_len <= 0 || max_len > CDSEG_MAX_PATCH) return CDSEG_ERR_UNSUPPORTED;
  if (!q || !k || !v || !dout || !dq || !dk || !dv || !patch_start) return CDSEG_ERR_ARG;
  // 16-byte operand loads (float4 / eight 16-bit values): 16-byte aligned rows
  const int op_mask = dtype == CDSEG_F32 ? 3 : 7;
  if (((ldq | ldk | ldv | lddo) & op_mask) || ((lddq | lddk | lddv) & 3)) return CDSEG_ERR_ARG;
  const long row = (long)num_heads * 16;  // a row is num_heads heads of 16 channels: a shorter stride overlaps the next row
  if (ldq < row || ldk < row || ldv < row || lddo < row || lddq < row || lddk < row || lddv < row) return CDSEG_ERR_ARG;
  if ((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)dout | (uintptr_t)dq | (uintptr_t)dk | (uintptr_t)dv) & 15) != 0)
    return CDSEG_ERR_ARG;
  if (!ws || ws_bytes < cdseg_attention_bwd_ws_bytes(num_slots, num_heads)) return CDSEG_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((unsigned)num_patches, (unsigned)num_heads);
  if (dtype == CDSEG_BF16) {
    AttnBwd16P p;
    p.q = (const bf16_t*)q; p.k = (const bf16_t*)k; p.v = (const bf16_t*)v; p.dout = (const bf16_t*)dout;
    p.q_gidx = q_gidx; p.kv_gidx = kv_gidx; p.widx = widx; p.patch_start = patch_start;
    p.dq = (float*)dq; p.dk = (float*)dk; p.dv = (float*)dv; p.stats = (float*)ws;
    p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.lddo = lddo; p.lddq = lddq; p.lddk = lddk; p.lddv = lddv;
    p.num_heads = num_heads; p.scale = scale;
    static std::once_flag attr16_once;
    static bool attr16_ok = false;
    std::call_once(attr16_once, [] {
      attr16_ok = hipFuncSetAttribute((const void*)attn_bwd16_q_kernel<>, hipFuncAttributeMaxDynamicSharedMemorySize, B16_Q_LDS) == hipSuccess &&
                  hipFuncSetAttribute((const void*)attn_bwd16_kv_kernel<>, hipFuncAttributeMaxDynamicSharedMemorySize, B16_KV_LDS) == hipSuccess;
    });
    if (!attr16_ok) return CDSEG_ERR_LAUNCH;
    // A patch-head is cut into `split` slices of its query (q kernel) / key (kv kernel) tiles, each a block that stages the
    // whole patch-head, while the launch does not fill the chip's 2 x 256 block slots: one block per patch-head left a single
    // scene's launches (at most 236 blocks) with two waves per SIMD, the deep stages with a quarter of the CUs
    int split = 1;
    while (split < 4 && (long)num_patches * num_heads * split * 2 <= 512) split *= 2;
    const dim3 grid16((unsigned)num_patches, (unsigned)num_heads, (unsigned)split);
    if (drop) {
      static std::once_flag drop16_once;
      static bool drop16_ok = false;
      std::call_once(drop16_once, [] {
        drop16_ok = hipFuncSetAttribute((const void*)attn_bwd16_q_kernel<DropP>, hipFuncAttributeMaxDynamicSharedMemorySize, B16_Q_LDS) == hipSuccess &&
                    hipFuncSetAttribute((const void*)attn_bwd16_kv_kernel<DropP>, hipFuncAttributeMaxDynamicSharedMemorySize, B16_KV_LDS) == hipSuccess;
      });
      if (!drop16_ok) return CDSEG_ERR_LAUNCH;
      cdseg_route_rec(CDSEG_RK_ATTN_BWD16_Q_DROP, 32, 32, split, 0, 0, CDSEG_BF16 << CDSEG_ROUTE_F_CT_SHIFT, B16_WAVES);
      hipLaunchKernelGGL(attn_bwd16_q_kernel<DropP>, grid16, dim3(B16_WAVES * 64), B16_Q_LDS, s, p, *drop);
      cdseg_route_rec(CDSEG_RK_ATTN_BWD16_KV_DROP, 32, 32, split, 0, 0, CDSEG_BF16 << CDSEG_ROUTE_F_CT_SHIFT, B16_WAVES);
      hipLaunchKernelGGL(attn_bwd16_kv_kernel<DropP>, grid16, dim3(B16_WAVES * 64), B16_KV_LDS, s, p, *drop);
      CDSEG_CHECK_LAUNCH();
      return CDSEG_OK;
    }
    cdseg_route_rec(CDSEG_RK_ATTN_BWD16_Q, 32, 32, split, 0, 0, CDSEG_BF16 << CDSEG_ROUTE_F_CT_SHIFT, B16_WAVES);
    hipLaunchKernelGGL(attn_bwd16_q_kernel<>, grid16, dim3(B16_WAVES * 64), B16_Q_LDS, s, p);
    cdseg_route_rec(CDSEG_RK_ATTN_BWD16_KV, 32, 32, split, 0, 0, CDSEG_BF16 << CDSEG_ROUTE_F_CT_SHIFT, B16_WAVES);
    hipLaunchKernelGGL(attn_bwd16_kv_kernel<>, grid16, dim3(B16_WAVES * 64), B16_KV_LDS, s, p);
    CDSEG_CHECK_LAUNCH();
    return CDSEG_OK;
  }
  AttnBwdP p;
  p.q = (const float*)q; p.k = (const float*)k; p.v = (const float*)v; p.dout = (const float*)dout;
  p.q_gidx = q_gidx; p.kv_gidx = kv_gidx; p.widx = widx; p.patch_start = patch_start;
  p.dq = (float*)dq; p.dk = (float*)dk; p.dv = (float*)dv; p.stats = (float*)ws;
  p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.lddo = lddo; p.lddq = lddq; p.lddk = lddk; p.lddv = lddv;
  p.num_heads = num_heads; p.scale = scale;
  static std::once_flag attr_once;  // (one device per process: one process per GPU)
  static bool attr_ok = false;
  std::call_once(attr_once, [] {
    attr_ok = hipFuncSetAttribute((const void*)attn_bwd_q_mfma_kernel<>, hipFuncAttributeMaxDynamicSharedMemorySize, BW_Q_LDS) == hipSuccess &&
              hipFuncSetAttribute((const void*)attn_bwd_kv_mfma_kernel<>, hipFuncAttributeMaxDynamicSharedMemorySize, BW_KV_LDS) == hipSuccess;
  });
  if (!attr_ok) return CDSEG_ERR_LAUNCH;
  if (drop) {
    static std::once_flag drop_once;
    static bool drop_ok = false;
    std::call_once(drop_once, [] {
      drop_ok = hipFuncSetAttribute((const void*)attn_bwd_q_mfma_kernel<DropP>, hipFuncAttributeMaxDynamicSharedMemorySize, BW_Q_LDS) == hipSuccess &&
                hipFuncSetAttribute((const void*)attn_bwd_kv_mfma_kernel<DropP>, hipFuncAttributeMaxDynamicSharedMemorySize, BW_KV_LDS) == hipSuccess;
    });
    if (!drop_ok) return CDSEG_ERR_LAUNCH;
    cdseg_route_rec(CDSEG_RK_ATTN_BWD_Q_DROP, 16, 16, 1, 0, 0, CDSEG_F32 << CDSEG_ROUTE_F_CT_SHIFT, BW_WAVES);
    hipLaunchKernelGGL(attn_bwd_q_mfma_kernel<DropP>, grid, dim3(BW_WAVES * 64), BW_Q_LDS, s, p, *drop);
    cdseg_route_rec(CDSEG_RK_ATTN_BWD_KV_DROP, 16, 16, 1, 0, 0, CDSEG_F32 << CDSEG_ROUTE_F_CT_SHIFT, BW_WAVES);
    hipLaunchKernelGGL(attn_bwd_kv_mfma_kernel<DropP>, grid, dim3(BW_WAVES * 64), BW_KV_LDS, s, p, *drop);
    CDSEG_CHECK_LAUNCH();
    return CDSEG_OK;
  }
  cdseg_route_rec(CDSEG_RK_ATTN_BWD_Q, 16, 16, 1, 0, 0, CDSEG_F32 << CDSEG_ROUTE_F_CT_SHIFT, BW_WAVES);
  hipLaunchKernelGGL(attn_bwd_q_mfma_kernel<>, grid, dim3(BW_WAVES * 64), BW_Q_LDS, s, p);
  cdseg_route_rec(CDSEG_RK_ATTN_BWD_KV, 16, 16, 1, 0, 0, CDSEG_F32 << CDSEG_ROUTE_F_CT_SHIFT, BW_WAVES);
  hipLaunchKernelGGL(attn_bwd_kv_mfma_kernel<>, grid, dim3(BW_WAVES * 64), BW_KV_LDS, s, p);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

extern "C" int cdseg_attention_bwd(const void* q, const void* k, const void* v, int ldq, int ldk, int ldv,
                                   const int32_t* q_gidx, const int32_t* kv_gidx, const int32_t* widx,
                                   const int32_t* patch_start, int num_patches, int num_heads, long num_slots, int max_len,
                                   float scale, const void* dout, int lddo, void* dq, void* dk, void* dv, int lddq, int lddk,
                                   int lddv, int dtype, void* ws, size_t ws_bytes, void* stream) {
  return attention_bwd_launch(q, k, v, ldq, ldk, ldv, q_gidx, kv_gidx, widx, patch_start, num_patches, num_heads, num_slots, max_len,
                              scale, dout, lddo, dq, dk, dv, lddq, lddk, lddv, dtype, ws, ws_bytes, stream, nullptr);
}

// The dropout backward (include/cdseg.h): a threshold of 256 drops nothing and is cdseg_attention_bwd's launch.
extern "C" int cdseg_attention_drop_bwd(const void* q, const void* k, const void* v, int ldq, int ldk, int ldv,
                                        const int32_t* q_gidx, const int32_t* kv_gidx, const int32_t* widx,
                                        const int32_t* patch_start, int num_patches, int num_heads, long num_slots, int max_len,
                                        float scale, const void* dout, int lddo, void* dq, void* dk, void* dv, int lddq, int lddk,
                                        int lddv, int dtype, void* ws, size_t ws_bytes, double rate, uint64_t seed, uint64_t offset,
                                        void* stream) {
  DropP d;
  if (!cdseg_drop_threshold(rate, seed, offset, &d)) return CDSEG_ERR_ARG;
  if (max_len > CDSEG_MAX_PATCH || num_heads > 65535) return CDSEG_ERR_ARG;
  return attention_bwd_launch(q, k, v, ldq, ldk, ldv, q_gidx, kv_gidx, widx, patch_start, num_patches, num_heads, num_slots, max_len,
                              scale, dout, lddo, dq, dk, dv, lddq, lddk, lddv, dtype, ws, ws_bytes, stream, d.thr >= 256 ? nullptr : &d);
}

// The fp32 entry points check what they are given before any launch, like the 16-bit and the deterministic forms: the
// required pointers are there, and every fp32 pointer (optional ones included; NULL passes) is 4-byte aligned.
template <typename... P>
static bool f32_aligned(const P*... ptr) { return ((((uintptr_t)ptr) | ...) & 3) == 0; }

static bool wgrad_args_ok(const float* x, const int32_t* xidx, const float* dy, const float* dw, const float* db) {
  return x && dy && dw && f32_aligned(x, xidx, dy, dw, db);
}

// A row stride shorter than the row makes consecutive rows overlap: for an input a wrong sum, for an output (dx, dw) adds
// onto the neighbouring rows' elements.  Every entry point below refuses it before any launch (include/cdseg.h).
static bool wgrad_lds_ok(int ldx, int k, int lddy, int n, int lddw) { return ldx >= k && lddy >= n && lddw >= k; }

extern "C" int cdseg_layernorm_bwd(const float* x, int ldx, const float* gamma, float eps, const float* dy, int lddy, float* dx,
                                   int lddx, int accumulate, float* dgamma, float* dbeta, long m, int c, void* stream) {
  if (m <= 0) return CDSEG_OK;
  if (c <= 0 || !x || !gamma || !dy || !dx) return CDSEG_ERR_ARG;
  if (!f32_aligned(x, gamma, dy, dx, dgamma, dbeta)) return CDSEG_ERR_ARG;
  if (ldx < c || lddy < c || lddx < c) return CDSEG_ERR_ARG;
  cdseg_route_rec(CDSEG_RK_LN_BWD, 4 * LNB_ROWS, c, 1, 0, 0, CDSEG_F32 << CDSEG_ROUTE_F_CT_SHIFT, 0);
  hipLaunchKernelGGL(layernorm_bwd_kernel, dim3((unsigned)cdiv(m, 4 * LNB_ROWS)), dim3(256), 0, (hipStream_t)stream, x, ldx, gamma, eps, dy,
                     lddy, dx, lddx, accumulate, dgamma, dbeta, m, c);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

extern "C" int cdseg_gelu_bwd(const float* u, const float* dy, float* dx, long n, void* stream) {
  if (n <= 0) return CDSEG_OK;
  if (!u || !dy || !dx || !f32_aligned(u, dy, dx)) return CDSEG_ERR_ARG;
  hipLaunchKernelGGL(gelu_bwd_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, u, dy, dx, n);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

// Row partition: a function of the shape only (csrc/wgrad_partition.h: no device query), shared by the default and the
// deterministic launches and reported by cdseg_wgrad_partition.
static void launch_wgrad_reduce(const float* ws_dw, const float* ws_db, float* dw, float* db, int N, int K, int lddw, int splits,
                                int noff, int dw_off_stride, hipStream_t stream) {
  WgradReduceP r;
  r.ws_dw = ws_dw; r.ws_db = ws_db; r.dw = dw; r.db = db; r.N = N; r.K = K; r.lddw = lddw; r.splits = splits; r.noff = noff;
  r.dw_off_stride = dw_off_stride;
  const long threads = (long)N * K * noff + N;
  hipLaunchKernelGGL(wgrad_det_reduce_kernel, dim3((unsigned)cdiv(threads, 256)), dim3(256), 0, stream, r);
}

static int launch_wgrad(WgradP p, int noff, hipStream_t stream, float* ws = nullptr) {
  const cdseg_wgrad::Partition q = cdseg_wgrad::partition_f32(p.M, p.N, p.K, noff);
  p.rows_per_split = q.rows_per_split;
  p.splits = q.splits;
  const dim3 grid((unsigned)cdiv(p.N, 64), (unsigned)cdiv(p.K, 64), (unsigned)(q.splits * noff));
  if (ws) {
    float* ws_db = ws + (size_t)noff * q.splits * p.N * p.K;
    cdseg_route_rec(CDSEG_RK_WGRAD_DET, 64, 64, q.splits, 0, cdseg_route_rows(q.rows_per_split), CDSEG_F32 << CDSEG_ROUTE_F_CT_SHIFT, noff);
    hipLaunchKernelGGL(wgrad_det_kernel, grid, dim3(256), 0, stream, p, ws, ws_db);
    launch_wgrad_reduce(ws, ws_db, p.dw, p.db, p.N, p.K, p.lddw, q.splits, noff, p.dw_off_stride, stream);
  } else {
    cdseg_route_rec(CDSEG_RK_WGRAD, 64, 64, q.splits, 0, cdseg_route_rows(q.rows_per_split), CDSEG_F32 << CDSEG_ROUTE_F_CT_SHIFT, noff);
    hipLaunchKernelGGL(wgrad_kernel, grid, dim3(256), 0, stream, p);
  }
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

extern "C" int cdseg_linear_wgrad(const float* x, int ldx, const int32_t* xidx, const float* dy, int lddy, long m, int k, int n,
                                  float* dw, int lddw, float* db, void* stream) {
  if (m <= 0 || n <= 0 || k <= 0) return CDSEG_OK;
  if (!wgrad_args_ok(x, xidx, dy, dw, db) || !wgrad_lds_ok(ldx, k, lddy, n, lddw)) return CDSEG_ERR_ARG;
  if ((n & 15) || (k & 15)) return CDSEG_ERR_UNSUPPORTED;
  WgradP p;
  p.dy = dy; p.x = x; p.xidx = xidx; p.dw = dw; p.db = db; p.M = m; p.N = n; p.K = k; p.lddy = lddy; p.ldx = ldx; p.lddw = lddw;
  p.idx_stride = 0; p.dw_off_stride = 0;
  return launch_wgrad(p, 1, (hipStream_t)stream);
}

extern "C" int cdseg_conv_wgrad(const float* x, int ldx, const int32_t* nbr_kmajor, int kvol, const float* dy, int lddy, long m,
                                int cin, int cout, float* dw, float* db, void* stream) {
  if (m <= 0 || kvol <= 0 || cin <= 0 || cout <= 0) return CDSEG_OK;
  if (!nbr_kmajor || !wgrad_args_ok(x, nbr_kmajor, dy, dw, db) || !wgrad_lds_ok(ldx, cin, lddy, cout, cin)) return CDSEG_ERR_ARG;
  if ((cin & 15) || (cout & 15)) return CDSEG_ERR_UNSUPPORTED;
  WgradP p;
  p.dy = dy; p.x = x; p.xidx = nbr_kmajor; p.dw = dw; p.db = db; p.M = m; p.N = cout; p.K = cin; p.lddy = lddy; p.ldx = ldx;
  p.lddw = kvol * cin; p.idx_stride = m; p.dw_off_stride = cin;
  return launch_wgrad(p, kvol, (hipStream_t)stream);
}

template <int TN, int TK>
static void launch_wgrad16_tile(const Wgrad16P& p, int noff, hipStream_t stream, float* ws_dw, float* ws_db) {
  const dim3 grid((unsigned)cdiv(p.N, 32 * TN), (unsigned)cdiv(p.K, 32 * TK), (unsigned)(p.splits * noff));
  if (ws_dw) {
    cdseg_route_rec(cdseg_route_template_id<CDSEG_RF_WGRAD16, TN, TK, 1>(), 32 * TN, 32 * TK, p.splits, 0, cdseg_route_rows(p.rows_per_split),
                    CDSEG_BF16 << CDSEG_ROUTE_F_CT_SHIFT, noff);
    hipLaunchKernelGGL((wgrad16_det_kernel<TN, TK>), grid, dim3(256), 0, stream, p, ws_dw, ws_db);
  } else {
    cdseg_route_rec(cdseg_route_template_id<CDSEG_RF_WGRAD16, TN, TK, 0>(), 32 * TN, 32 * TK, p.splits, 0, cdseg_route_rows(p.rows_per_split),
                    CDSEG_BF16 << CDSEG_ROUTE_F_CT_SHIFT, noff);
    hipLaunchKernelGGL((wgrad16_kernel<TN, TK>), grid, dim3(256), 0, stream, p);
  }
}

// Tile: the narrowest of 32 / 64 / 128 columns that covers N (K), so the narrow stages read dY and X once (C = 32: dW 96 x 32
// is one tile); 128 x 128 would need 64 KiB of LDS, the deep stages take 128 x 64.  Rows are split over the grid as in
// launch_wgrad: ~2 blocks per CU, at least 512 rows (8 chunks) per block so a tile's atomics stay rare next to its loads
// (cdseg_wgrad::partition_16).
static int launch_wgrad16(Wgrad16P p, int noff, hipStream_t stream, float* ws = nullptr) {
  const cdseg_wgrad::Partition q = cdseg_wgrad::partition_16(p.M, p.N, p.K, noff);
  if (q.splits < 0) return CDSEG_ERR_UNSUPPORTED;
  p.rows_per_split = q.rows_per_split;
  p.splits = q.splits;
  float* ws_db = ws ? ws + (size_t)noff * q.splits * p.N * p.K : nullptr;
  switch (q.tn * 8 + q.tk) {
    case 1 * 8 + 1: launch_wgrad16_tile<1, 1>(p, noff, stream, ws, ws_db); break;
    case 1 * 8 + 2: launch_wgrad16_tile<1, 2>(p, noff, stream, ws, ws_db); break;
    case 1 * 8 + 4: launch_wgrad16_tile<1, 4>(p, noff, stream, ws, ws_db); break;
    case 2 * 8 + 1: launch_wgrad16_tile<2, 1>(p, noff, stream, ws, ws_db); break;
    case 2 * 8 + 2: launch_wgrad16_tile<2, 2>(p, noff, stream, ws, ws_db); break;
    case 2 * 8 + 4: launch_wgrad16_tile<2, 4>(p, noff, stream, ws, ws_db); break;
    case 4 * 8 + 1: launch_wgrad16_tile<4, 1>(p, noff, stream, ws, ws_db); break;
    default: launch_wgrad16_tile<4, 2>(p, noff, stream, ws, ws_db); break;
  }
  if (ws) launch_wgrad_reduce(ws, ws_db, p.dw, p.db, p.N, p.K, p.lddw, q.splits, noff, p.dw_off_stride, stream);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

static bool wgrad16_args_ok(const void* x, int ldx, const void* xidx, const void* dy, int lddy, const void* dw, const void* db) {
  if (!x || !dy || !dw) return false;
  if ((ldx | lddy) & 7) return false;  // 16-byte operand loads: eight 16-bit values
  return ((((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dw | (uintptr_t)db | (uintptr_t)xidx) & 15) == 0);
}

extern "C" int cdseg_linear_wgrad16(const void* x, int ldx, const int32_t* xidx, const void* dy, int lddy, long m, int k, int n,
                                    float* dw, int lddw, float* db, void* stream) {
  if (m <= 0 || n <= 0 || k <= 0) return CDSEG_OK;
  if (!wgrad16_args_ok(x, ldx, xidx, dy, lddy, dw, db) || !wgrad_lds_ok(ldx, k, lddy, n, lddw)) return CDSEG_ERR_ARG;
  if ((n & 15) || (k & 15)) return CDSEG_ERR_UNSUPPORTED;
  Wgrad16P p;
  p.dy = (const bf16_t*)dy; p.x = (const bf16_t*)x; p.xidx = xidx; p.dw = dw; p.db = db; p.M = m; p.N = n; p.K = k; p.lddy = lddy;
  p.ldx = ldx; p.lddw = lddw; p.idx_stride = 0; p.dw_off_stride = 0;
  return launch_wgrad16(p, 1, (hipStream_t)stream);
}

extern "C" int cdseg_conv_wgrad16(const void* x, int ldx, const int32_t* nbr_kmajor, int kvol, const void* dy, int lddy, long m,
                                  int cin, int cout, float* dw, float* db, void* stream) {
  if (m <= 0 || kvol <= 0) return CDSEG_OK;
  if (!nbr_kmajor || !wgrad16_args_ok(x, ldx, nbr_kmajor, dy, lddy, dw, db) || !wgrad_lds_ok(ldx, cin, lddy, cout, cin))
    return CDSEG_ERR_ARG;
  if ((cin & 15) || (cout & 15)) return CDSEG_ERR_UNSUPPORTED;
  Wgrad16P p;
  p.dy = (const bf16_t*)dy; p.x = (const bf16_t*)x; p.xidx = nbr_kmajor; p.dw = dw; p.db = db; p.M = m; p.N = cout; p.K = cin;
  p.lddy = lddy; p.ldx = ldx; p.lddw = kvol * cin; p.idx_stride = m; p.dw_off_stride = cin;
  return launch_wgrad16(p, kvol, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------ deterministic forms
// Fixed summation order (include/cdseg.h): partial results to a caller-provided workspace with plain stores, then a reduce
// launch that adds them by ascending split / block index and adds the total ONCE onto dw / db / dgamma / dbeta.
extern "C" int cdseg_wgrad_partition(long m, int n, int k, int kvol, int dtype, long* rows_per_split, int* splits) {
  if (dtype != CDSEG_F32 && dtype != CDSEG_BF16) return CDSEG_ERR_UNSUPPORTED;
  if (m < 0 || n <= 0 || k <= 0 || kvol <= 0) return CDSEG_ERR_ARG;
  const cdseg_wgrad::Partition q = dtype == CDSEG_F32 ? cdseg_wgrad::partition_f32(m, n, k, kvol) : cdseg_wgrad::partition_16(m, n, k, kvol);
  if (q.splits < 0) return CDSEG_ERR_UNSUPPORTED;
  if (rows_per_split) *rows_per_split = q.rows_per_split;
  if (splits) *splits = q.splits;
  return CDSEG_OK;
}

extern "C" size_t cdseg_wgrad_det_ws_bytes(long m, int n, int k, int kvol, int dtype) {
  long rows = 0;
  int splits = 0;
  if (cdseg_wgrad_partition(m, n, k, kvol, dtype, &rows, &splits) != CDSEG_OK) return 0;
  return cdseg_wgrad::det_ws_floats(n, k, kvol, splits) * sizeof(float);
}

static int wgrad_det(const void* x, int ldx, const int32_t* xidx, int kvol, const void* dy, int lddy, long m, int k, int n, float* dw,
                     int lddw, long idx_stride, int dw_off_stride, float* db, int dtype, void* ws, size_t ws_bytes, void* stream) {
  if (dtype != CDSEG_F32 && dtype != CDSEG_BF16) return CDSEG_ERR_UNSUPPORTED;
  if (dtype == CDSEG_BF16) {
    if (!wgrad16_args_ok(x, ldx, xidx, dy, lddy, dw, db)) return CDSEG_ERR_ARG;
  } else if (!x || !dy || !dw || ((((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dw | (uintptr_t)db | (uintptr_t)xidx) & 3) != 0)) {
    return CDSEG_ERR_ARG;
  }
  if (((uintptr_t)ws & 15) != 0 || !wgrad_lds_ok(ldx, k, lddy, n, lddw)) return CDSEG_ERR_ARG;
  if ((n & 15) || (k & 15)) return CDSEG_ERR_UNSUPPORTED;
  long rows = 0;
  int splits = 0;
  const int st = cdseg_wgrad_partition(m, n, k, kvol, dtype, &rows, &splits);
  if (st != CDSEG_OK) return st;
  if (!ws || ws_bytes < cdseg_wgrad::det_ws_floats(n, k, kvol, splits) * sizeof(float)) return CDSEG_ERR_WORKSPACE;
  if (dtype == CDSEG_BF16) {
    Wgrad16P p;
    p.dy = (const bf16_t*)dy; p.x = (const bf16_t*)x; p.xidx = xidx; p.dw = dw; p.db = db; p.M = m; p.N = n; p.K = k; p.lddy = lddy;
    p.ldx = ldx; p.lddw = lddw; p.idx_stride = idx_stride; p.dw_off_stride = dw_off_stride;
    return launch_wgrad16(p, kvol, (hipStream_t)stream, (float*)ws);
  }
  WgradP p;
  p.dy = (const float*)dy; p.x = (const float*)x; p.xidx = xidx; p.dw = dw; p.db = db; p.M = m; p.N = n; p.K = k; p.lddy = lddy;
  p.ldx = ldx; p.lddw = lddw; p.idx_stride = idx_stride; p.dw_off_stride = dw_off_stride;
  return launch_wgrad(p, kvol, (hipStream_t)stream, (float*)ws);
}

extern "C" int cdseg_linear_wgrad_det(const void* x, int ldx, const int32_t* xidx, const void* dy, int lddy, long m, int k, int n,
                                      float* dw, int lddw, float* db, int dtype, void* ws, size_t ws_bytes, void* stream) {
  if (m <= 0 || n <= 0 || k <= 0) return CDSEG_OK;
  return wgrad_det(x, ldx, xidx, 1, dy, lddy, m, k, n, dw, lddw, 0, 0, db, dtype, ws, ws_bytes, stream);
}

extern "C" int cdseg_conv_wgrad_det(const void* x, int ldx, const int32_t* nbr_kmajor, int kvol, const void* dy, int lddy, long m,
                                    int cin, int cout, float* dw, float* db, int dtype, void* ws, size_t ws_bytes, void* stream) {
  if (m <= 0 || kvol <= 0 || cin <= 0 || cout <= 0) return CDSEG_OK;
  if (!nbr_kmajor) return CDSEG_ERR_ARG;
  return wgrad_det(x, ldx, nbr_kmajor, kvol, dy, lddy, m, cin, cout, dw, kvol * cin, m, cin, db, dtype, ws, ws_bytes, stream);
}

extern "C" size_t cdseg_layernorm_bwd_det_ws_bytes(long m, int c) { return cdseg_wgrad::ln_det_ws_floats(m, c) * sizeof(float); }

extern "C" int cdseg_layernorm_bwd_det(const float* x, int ldx, const float* gamma, float eps, const float* dy, int lddy, float* dx,
                                       int lddx, int accumulate, float* dgamma, float* dbeta, long m, int c, void* ws, size_t ws_bytes,
                                       void* stream) {
  if (m <= 0 || c <= 0) return CDSEG_OK;
  if (!x || !gamma || !dy || !dx) return CDSEG_ERR_ARG;
  if (!f32_aligned(x, gamma, dy, dx, dgamma, dbeta) || ldx < c || lddy < c || lddx < c) return CDSEG_ERR_ARG;
  if (c > LNB_MAXC) return CDSEG_ERR_UNSUPPORTED;  // (the default form's per-element-atomic path: no fixed order)
  if (((uintptr_t)ws & 3) != 0) return CDSEG_ERR_ARG;
  if (!ws || ws_bytes < cdseg_layernorm_bwd_det_ws_bytes(m, c)) return CDSEG_ERR_WORKSPACE;
  const long nblocks = cdseg_wgrad::ln_blocks(m);
  cdseg_route_rec(CDSEG_RK_LN_BWD_DET, 0, c, (int)nblocks, 0, 0, CDSEG_F32 << CDSEG_ROUTE_F_CT_SHIFT, 0);
  hipLaunchKernelGGL(layernorm_bwd_det_kernel, dim3((unsigned)nblocks), dim3(256), 0, (hipStream_t)stream, x, ldx, gamma, eps, dy, lddy,
                     dx, lddx, accumulate, m, c, (float*)ws);
  if (dgamma || dbeta)
    hipLaunchKernelGGL(layernorm_det_reduce_kernel, dim3((unsigned)cdiv(2 * c, 64)), dim3(64), 0, (hipStream_t)stream, (const float*)ws,
                       nblocks, c, dgamma, dbeta);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

extern "C" int cdseg_segment_sum(const float* src, int ld, const int32_t* seg_start, long m, int c, float* out, int ldo, void* stream) {
  if (m <= 0 || c <= 0) return CDSEG_OK;
  if (!src || !seg_start || !out || !f32_aligned(src, out) || ((uintptr_t)seg_start & 3) || ld < c || ldo < c) return CDSEG_ERR_ARG;
  const int cw = c <= 16 ? 16 : c <= 32 ? 32 : 64;
  const long rows_per_block = 4 * (64 / cw);
  hipLaunchKernelGGL(segment_sum_kernel, dim3((unsigned)cdiv(m, rows_per_block)), dim3(256), 0, (hipStream_t)stream, src, ld, seg_start, m,
                     c, out, ldo, cw);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}
