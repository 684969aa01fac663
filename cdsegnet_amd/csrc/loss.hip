// Fused segmentation loss: cross entropy + multi-class Lovasz-Softmax over the classes present, forward and backward.
// ref: pointcept/models/losses/misc.py:95-132 (CrossEntropyLoss), losses/lovasz.py:118-165, 210-265 (Lovasz-Softmax,
// classes = "present", whole batch), restated in cdsegnet_amd/losses.py.  Definition, tie rule and limits: include/cdseg.h.
//
// Passes:
//   phase 0   label histogram (integer atomics), read by the host: n_valid, the present classes, their ranks.
//   phase 1   row pass     softmax per row, the row's CE term, one 64-bit key per (row, present class)
//             sort         ONE rocPRIM radix sort of all keys: class rank | inverted error | row | foreground bit
//             scan pass    per (class, 1024-key chunk): foreground count; then carry-in, the Jaccard differences, the chunk's
//                          share of L_c and the scatter of coef to (row, class rank)
//             finish       CE, L_c and the mean over classes, summed in a fixed order by one block
//   backward  one launch: softmax again, dlogits for both upstream scalars.
// Row -> lane map of the row pass and the backward: a row is owned by a group of G lanes, lane l of the group holds the
// columns l, l + G, ...  G = 16 with one / two columns a lane for C <= 16 / 32 (four rows a wave: a 13-wide row on a whole
// wave would idle 51 lanes), G = 64 with one / two / four columns a lane for C <= 64 / 128 / 256 (a 200-wide row is 4
// registers a lane, never one lane's 200).  Loads are contiguous across the group, every reduction is an xor butterfly
// inside it.  The softmax, the Jaccard differences and every sum are evaluated in fp64 and rounded to fp32 once (memory and
// the sort bound the passes, not the arithmetic).  No float atomics anywhere; every sum has an order that depends on the
// shape only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>

#include "common.h"
#include "route.h"

namespace {

constexpr int LOSS_MAX_C = 256;
constexpr long LOSS_MAX_N = 1L << 24;
constexpr int ROWS_PER_BLOCK = 256;  // row pass / backward: rows of one block (one CE partial each)
constexpr int CHUNK = 1024;          // scan pass: keys of one block (256 threads x 4)
constexpr uint32_t ERR_MAX_BITS = 0x3FFFFFFFu;  // err lies in [0, 1]: its fp32 bits fit 30 bits
constexpr uint32_t FIELD_IGNORED = 0x7FFFFFFFu; // ignored rows sort behind every valid row of their class segment

// key: [63:56] class rank | [55:25] ERR_MAX_BITS - bits(err) (descending err; ignored rows: FIELD_IGNORED) | [24:1] row | [0] fg
__device__ __forceinline__ uint64_t make_key(int rank, uint32_t field, long row, int fg) {
  return ((uint64_t)rank << 56) | ((uint64_t)field << 25) | ((uint64_t)row << 1) | (uint64_t)fg;
}

struct LossTab {
  int16_t rank[LOSS_MAX_C];  // class -> rank among the present classes, -1 = absent
  int32_t count[LOSS_MAX_C]; // rank -> rows of that class (T of the Jaccard terms)
};

inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <int G>
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <int G>
__device__ __forceinline__ float group_max(float v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

__global__ void __launch_bounds__(256) loss_hist_kernel(const int64_t* __restrict__ labels, long n, int c, long ignore,
                                                        int32_t* __restrict__ hist) {
  __shared__ int32_t h[LOSS_MAX_C + 1];
  for (int i = threadIdx.x; i <= c; i += 256) h[i] = 0;
  __syncthreads();
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long lab = labels[i];
    if (lab == ignore) continue;
    atomicAdd(&h[(lab >= 0 && lab < c) ? (int)lab : c], 1);  // slot c: labels outside [0, c) that are not `ignore`
  }
  __syncthreads();
  for (int i = threadIdx.x; i <= c; i += 256)
    if (h[i]) atomicAdd(&hist[i], h[i]);
}

// softmax of one row on a group of G lanes, E columns a lane; returns the row maximum and the sum of exp(x - max).
// Evaluated in fp64 (a few hundred exponentials a row next to a sort of as many 64-bit keys: the row pass is 7 % of the
// forward at 480 k x 200 and moves 2.3 TB/s, profiles/NOTES.md) so that what the fp32
// results carry is one rounding, not the error of an fp32 exp / sum / divide chain.
template <int G, int E>
__device__ __forceinline__ void row_softmax(const float* __restrict__ row, int c, int gl, float (&x)[E], double (&p)[E],
                                            float& mx, double& sum) {
  mx = -INFINITY;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int col = gl + e * G;
    x[e] = col < c ? row[col] : -INFINITY;
    mx = fmaxf(mx, x[e]);
  }
  mx = group_max<G>(mx);
  sum = 0.0;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    p[e] = gl + e * G < c ? exp((double)x[e] - (double)mx) : 0.0;
    sum += p[e];
  }
  sum = group_sum<G>(sum);
#pragma unroll
  for (int e = 0; e < E; ++e) p[e] /= sum;
}

template <int G, int E>
__global__ void __launch_bounds__(256) loss_rows_kernel(const float* __restrict__ logits, int ldl,
                                                        const int64_t* __restrict__ labels, long n, int c, long ignore,
                                                        LossTab tab, int np, uint64_t* __restrict__ keys,
                                                        double* __restrict__ ce_part) {
  constexpr int GROUPS = 256 / G;
  __shared__ double part[GROUPS];
  const int g = threadIdx.x / G, gl = threadIdx.x % G;
  int rk[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int col = gl + e * G;
    rk[e] = col < c ? (int)tab.rank[col] : -1;
  }
  double ce = 0.0;
  const long base = (long)blockIdx.x * ROWS_PER_BLOCK;
  for (int it = 0; it < ROWS_PER_BLOCK / GROUPS; ++it) {
    const long i = base + (long)it * GROUPS + g;
    if (i >= n) break;  // (uniform in the group)
    const long lab = labels[i];
    const bool valid = lab != ignore && lab >= 0 && lab < c;
    float x[E], mx;
    double p[E], sum;
    row_softmax<G, E>(logits + i * (long)ldl, c, gl, x, p, mx, sum);
    float xy = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int col = gl + e * G;
      if (valid && col == (int)lab) xy = x[e];
      if (rk[e] >= 0) {
        const int fg = valid && col == (int)lab;
        const float err = (float)fabs((fg ? 1.0 : 0.0) - p[e]);
        uint32_t bits = __float_as_uint(err);
        bits = bits > ERR_MAX_BITS ? ERR_MAX_BITS : bits;  // (a NaN row: the CE term carries the NaN)
        keys[i * (long)np + rk[e]] = make_key(rk[e], valid ? ERR_MAX_BITS - bits : FIELD_IGNORED, i, fg);
      }
    }
    xy = group_sum<G>(xy);  // one lane holds the label's logit, the others 0
    if (valid) ce += (log(sum) + (double)mx) - (double)xy;
  }
  if (gl == 0) part[g] = ce;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = part[0];
    for (int k = 1; k < GROUPS; ++k) t += part[k];
    ce_part[blockIdx.x] = t;
  }
}

__device__ __forceinline__ int block_sum_i32(int v, int* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const int t = sh[0] + sh[1] + sh[2] + sh[3];
  __syncthreads();
  return t;
}

// foreground rows of every (class segment, chunk): segment r = keys [r * n, r * n + n_valid) of the sorted array
__global__ void __launch_bounds__(256) loss_chunk_count_kernel(const uint64_t* __restrict__ keys, long n, int n_valid, int chunks,
                                                               int32_t* __restrict__ chunk_fg) {
  __shared__ int sh[4];
  const int r = blockIdx.x / chunks, j = blockIdx.x % chunks;
  const uint64_t* seg = keys + (long)r * n;
  int cnt = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int k = j * CHUNK + threadIdx.x * 4 + e;
    if (k < n_valid) cnt += (int)(seg[k] & 1u);
  }
  cnt = block_sum_i32(cnt, sh);
  if (threadIdx.x == 0) chunk_fg[blockIdx.x] = cnt;
}

// carry-in from the chunks before, F_k, the Jaccard difference d_k in closed form, the chunk's share of L_c, coef scatter.
// With I = T - F (foreground rows still ahead) and U = T + B (the union so far):  jac_k = 1 - I_k / U_k, hence
//   d_k = 1 / U_k on a foreground row (I drops by one),  d_k = I_k / (U_{k-1} U_k) on a background row (U grows by one):
// no difference of two nearly equal quotients is ever formed.
__global__ void __launch_bounds__(256) loss_scan_kernel(const uint64_t* __restrict__ keys, long n, int n_valid, int chunks,
                                                        const int32_t* __restrict__ chunk_fg, LossTab tab, int np,
                                                        float* __restrict__ coef, double* __restrict__ l_part) {
  __shared__ int sh[4];
  __shared__ double shf[4];
  const int r = blockIdx.x / chunks, j = blockIdx.x % chunks;
  const uint64_t* seg = keys + (long)r * n;
  int carry = 0;
  for (int q = threadIdx.x; q < j; q += 256) carry += chunk_fg[r * chunks + q];
  carry = block_sum_i32(carry, sh);
  uint64_t key[4];
  int fgs[4], mine = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int k = j * CHUNK + threadIdx.x * 4 + e;
    key[e] = k < n_valid ? seg[k] : 0;
    fgs[e] = (int)(key[e] & 1u);
    mine += fgs[e];
  }
  // exclusive scan of the threads' counts: inside the wave, then across the four waves
  int incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o, 64);
    if ((int)(threadIdx.x & 63) >= o) incl += up;
  }
  if ((threadIdx.x & 63) == 63) sh[threadIdx.x >> 6] = incl;
  __syncthreads();
  int before = carry + incl - mine;
  for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) before += sh[w];
  const int T = tab.count[r];
  const double inv_p = 1.0 / (double)np;
  double acc = 0.0;
  int F = before;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int k = j * CHUNK + threadIdx.x * 4 + e;
    if (k < n_valid) {
      F += fgs[e];
      const int U = T + (k + 1 - F);  // T + B_k
      const double d = fgs[e] ? 1.0 / (double)U : (double)(T - F) / ((double)(U - 1) * (double)U);
      const uint32_t field = (uint32_t)(key[e] >> 25) & 0x7FFFFFFFu;
      const float err = field <= ERR_MAX_BITS ? __uint_as_float(ERR_MAX_BITS - field) : 0.f;
      acc += (double)err * d;
      const long row = (long)((key[e] >> 1) & 0xFFFFFFu);
      if (row < n) coef[row * (long)np + r] = (float)((fgs[e] ? -d : d) * inv_p);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) shf[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) l_part[blockIdx.x] = ((shf[0] + shf[1]) + shf[2]) + shf[3];
}

// out[0] = CE, out[1] = Lovasz: the fp64 partials added in ascending order by one block, rounded to fp32 once
__global__ void __launch_bounds__(256) loss_finish_kernel(const double* __restrict__ ce_part, int ce_parts,
                                                          const double* __restrict__ l_part, int chunks, int np, int n_valid,
                                                          float* __restrict__ out) {
  __shared__ double sc[256], sl[256];
  const int t = threadIdx.x;
  double a = 0.0;
  for (int q = t; q < ce_parts; q += 256) a += ce_part[q];
  sc[t] = a;
  double l = 0.0;
  if (t < np)
    for (int q = 0; q < chunks; ++q) l += l_part[t * chunks + q];
  sl[t] = l;
  __syncthreads();
  if (t == 0) {
    double ce = 0.0, lv = 0.0;
    for (int q = 0; q < 256; ++q) ce += sc[q];
    for (int q = 0; q < np; ++q) lv += sl[q];
    out[0] = (float)(ce / (double)n_valid);
    out[1] = (float)(lv / (double)np);
  }
}

template <int G, int E>
__global__ void __launch_bounds__(256) loss_bwd_kernel(const float* __restrict__ logits, int ldl,
                                                       const int64_t* __restrict__ labels, long n, int c, long ignore,
                                                       LossTab tab, int np, const float* __restrict__ coef,
                                                       const float* __restrict__ g_ce, const float* __restrict__ g_lov,
                                                       double inv_valid, float* __restrict__ dlogits, int lddl) {
  constexpr int GROUPS = 256 / G;
  const int g = threadIdx.x / G, gl = threadIdx.x % G;
  int rk[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int col = gl + e * G;
    rk[e] = col < c ? (int)tab.rank[col] : -1;
  }
  const double gce = (double)(g_ce ? g_ce[0] : 0.f) * inv_valid, glov = (double)(g_lov ? g_lov[0] : 0.f);
  const long base = (long)blockIdx.x * ROWS_PER_BLOCK;
  for (int it = 0; it < ROWS_PER_BLOCK / GROUPS; ++it) {
    const long i = base + (long)it * GROUPS + g;
    if (i >= n) break;
    const long lab = labels[i];
    const bool valid = lab != ignore && lab >= 0 && lab < c;
    float* drow = dlogits + i * (long)lddl;
    if (!valid) {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int col = gl + e * G;
        if (col < c) drow[col] = 0.f;
      }
      continue;
    }
    float x[E], mx;
    double p[E], sum, cf[E], s = 0.0;
    row_softmax<G, E>(logits + i * (long)ldl, c, gl, x, p, mx, sum);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      cf[e] = rk[e] >= 0 ? (double)coef[i * (long)np + rk[e]] : 0.0;
      s += cf[e] * p[e];
    }
    s = group_sum<G>(s);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int col = gl + e * G;
      if (col < c) drow[col] = (float)(gce * (p[e] - (col == (int)lab ? 1.0 : 0.0)) + glov * (p[e] * (cf[e] - s)));
    }
  }
}

// rocPRIM's temporary storage for `total` keys sorted on bits [0, end_bit); false when the query itself fails (it asks the
// runtime for the device's sort configuration: without a device it fails for every size beyond one block)
bool sort_tmp_bytes(size_t total, unsigned end_bit, size_t& bytes) {
  bytes = 0;
  rocprim::double_buffer<uint64_t> db((uint64_t*)nullptr, (uint64_t*)nullptr);
  return rocprim::radix_sort_keys(nullptr, bytes, db, total, 0u, end_bit, (hipStream_t)0, false) == hipSuccess;
}

int rank_bits(int np) {  // bits of the largest class rank
  int msb = 0;
  while ((1 << msb) < np) ++msb;
  return msb;
}

// host side of the one read: ranks of the present classes, their row counts, n_valid.  Returns P, or -1 (inconsistent counts)
int build_tab(const int32_t* hist_host, long n, int c, LossTab& tab, long& n_valid) {
  int np = 0;
  n_valid = 0;
  for (int k = 0; k < LOSS_MAX_C; ++k) {
    tab.rank[k] = -1;
    tab.count[k] = 0;
  }
  for (int k = 0; k < c; ++k) {
    if (hist_host[k] < 0) return -1;
    if (hist_host[k] > 0) {
      tab.rank[k] = (int16_t)np;
      tab.count[np++] = hist_host[k];
      n_valid += hist_host[k];
    }
  }
  if (hist_host[c] != 0 || n_valid > n) return -1;
  return np;
}

int check_common(const float* logits, int ldl, const int64_t* labels, long n, int c) {
  if (!logits || !labels || n <= 0 || c <= 0 || ldl < c) return CDSEG_ERR_ARG;
  if (((uintptr_t)logits & 3) || ((uintptr_t)labels & 7)) return CDSEG_ERR_ARG;
  if (n >= LOSS_MAX_N || c > LOSS_MAX_C) return CDSEG_ERR_UNSUPPORTED;
  return CDSEG_OK;
}

template <typename F>
void launch_by_width(int c, F&& f) {
  if (c <= 16) f(std::integral_constant<int, 16>(), std::integral_constant<int, 1>());
  else if (c <= 32) f(std::integral_constant<int, 16>(), std::integral_constant<int, 2>());
  else if (c <= 64) f(std::integral_constant<int, 64>(), std::integral_constant<int, 1>());
  else if (c <= 128) f(std::integral_constant<int, 64>(), std::integral_constant<int, 2>());
  else f(std::integral_constant<int, 64>(), std::integral_constant<int, 4>());
}

}  // namespace

extern "C" {

size_t cdseg_seg_loss_ws_bytes(long n, int c) {
  if (n <= 0 || c <= 0) return 0;
  const size_t total = (size_t)n * (size_t)c;
  const size_t chunks = ((size_t)n + CHUNK - 1) / CHUNK;
  // the sort's share: the larger of rocPRIM's needs at the two ends, every class present and one class present.  Phase 1
  // asks again for the keys it really sorts and refuses a short workspace before its first launch, so a size in between
  // that needed more (rocPRIM picks among three algorithms by size) would be an error code, never an overrun.  Without a
  // device the query fails and the share counts as 0: the figure is then a lower bound (and phase 1 fails at its own query).
  size_t tmp_all = 0, tmp_one = 0;
  if (!sort_tmp_bytes(total, 64u, tmp_all)) tmp_all = 0;
  if (!sort_tmp_bytes((size_t)n, 56u, tmp_one)) tmp_one = 0;
  return 2 * al256(total * sizeof(uint64_t)) + al256(std::max(tmp_all, tmp_one)) + al256((size_t)c * chunks * 4) +
         al256((size_t)c * chunks * 8) + al256((((size_t)n + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK) * 8) + 256;
}

int cdseg_seg_loss_fwd(const float* logits, int ldl, const int64_t* labels, long n, int c, long ignore_index, int phase,
                       int32_t* hist, const int32_t* hist_host, float* out, float* coef, void* ws, size_t ws_bytes,
                       void* stream) {
  const int st = check_common(logits, ldl, labels, n, c);
  if (st != CDSEG_OK) return st;
  if (phase != 0 && phase != 1) return CDSEG_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (phase == 0) {
    if (!hist || ((uintptr_t)hist & 3)) return CDSEG_ERR_ARG;
    if (hipMemsetAsync(hist, 0, (size_t)(c + 1) * sizeof(int32_t), s) != hipSuccess) return CDSEG_ERR_LAUNCH;
    const int blocks = (int)std::min<long>((n + 255) / 256, 1024);
    hipLaunchKernelGGL(loss_hist_kernel, dim3(blocks), dim3(256), 0, s, labels, n, c, ignore_index, hist);
    CDSEG_CHECK_LAUNCH();
    return CDSEG_OK;
  }
  if (!hist_host || !out || !coef || ((uintptr_t)out & 3) || ((uintptr_t)coef & 3)) return CDSEG_ERR_ARG;
  LossTab tab;
  long n_valid = 0;
  const int np = build_tab(hist_host, n, c, tab, n_valid);
  if (np <= 0) return CDSEG_ERR_ARG;  // bad labels, counts beyond n, or no valid row (no fused form: the caller's torch path)
  if (!ws || ((uintptr_t)ws & 15)) return ws ? CDSEG_ERR_ARG : CDSEG_ERR_WORKSPACE;
  if (ws_bytes < cdseg_seg_loss_ws_bytes(n, c)) return CDSEG_ERR_WORKSPACE;
  const size_t total = (size_t)n * (size_t)np;
  const int chunks = (int)((n_valid + CHUNK - 1) / CHUNK);
  const int row_blocks = (int)((n + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK);
  char* w = (char*)ws;
  uint64_t* k0 = (uint64_t*)w;
  w += al256(total * sizeof(uint64_t));
  uint64_t* k1 = (uint64_t*)w;
  w += al256(total * sizeof(uint64_t));
  int32_t* chunk_fg = (int32_t*)w;
  w += al256((size_t)np * chunks * 4);
  double* l_part = (double*)w;
  w += al256((size_t)np * chunks * 8);
  double* ce_part = (double*)w;
  w += al256((size_t)row_blocks * 8);
  size_t tmp_bytes = ws_bytes - (size_t)(w - (char*)ws), tmp_need = 0;
  const unsigned end_bit = (unsigned)(56 + rank_bits(np));
  if (!sort_tmp_bytes(total, end_bit, tmp_need)) return CDSEG_ERR_LAUNCH;  // (no launch has been made yet)
  if (tmp_need > tmp_bytes) return CDSEG_ERR_WORKSPACE;

  launch_by_width(c, [&](auto G, auto E) {
    cdseg_route_rec(cdseg_route_template_id<CDSEG_RF_LOSS, decltype(G)::value, decltype(E)::value, 0>(), ROWS_PER_BLOCK, c, 1, 0, 0,
                    CDSEG_F32 << CDSEG_ROUTE_F_CT_SHIFT, np);
    hipLaunchKernelGGL((loss_rows_kernel<decltype(G)::value, decltype(E)::value>), dim3(row_blocks), dim3(256), 0, s, logits, ldl,
                       labels, n, c, ignore_index, tab, np, k0, ce_part);
  });
  CDSEG_CHECK_LAUNCH();
  rocprim::double_buffer<uint64_t> db(k0, k1);
  if (rocprim::radix_sort_keys(w, tmp_bytes, db, total, 0u, end_bit, s, false) != hipSuccess) return CDSEG_ERR_LAUNCH;
  const uint64_t* sorted = db.current();
  hipLaunchKernelGGL(loss_chunk_count_kernel, dim3(np * chunks), dim3(256), 0, s, sorted, n, (int)n_valid, chunks, chunk_fg);
  hipLaunchKernelGGL(loss_scan_kernel, dim3(np * chunks), dim3(256), 0, s, sorted, n, (int)n_valid, chunks, chunk_fg, tab, np, coef,
                     l_part);
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(256), 0, s, ce_part, row_blocks, l_part, chunks, np, (int)n_valid, out);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_seg_loss_bwd(const float* logits, int ldl, const int64_t* labels, long n, int c, long ignore_index,
                       const int32_t* hist_host, const float* coef, const float* g_ce, const float* g_lovasz, float* dlogits,
                       int lddl, void* stream) {
  const int st = check_common(logits, ldl, labels, n, c);
  if (st != CDSEG_OK) return st;
  if (!hist_host || !coef || !dlogits || lddl < c || ((uintptr_t)coef & 3) || ((uintptr_t)dlogits & 3)) return CDSEG_ERR_ARG;
  if (((uintptr_t)g_ce & 3) || ((uintptr_t)g_lovasz & 3)) return CDSEG_ERR_ARG;
  LossTab tab;
  long n_valid = 0;
  const int np = build_tab(hist_host, n, c, tab, n_valid);
  if (np <= 0) return CDSEG_ERR_ARG;
  const int row_blocks = (int)((n + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK);
  const double inv_valid = 1.0 / (double)n_valid;
  launch_by_width(c, [&](auto G, auto E) {
    cdseg_route_rec(cdseg_route_template_id<CDSEG_RF_LOSS, decltype(G)::value, decltype(E)::value, 1>(), ROWS_PER_BLOCK, c, 1, 0, 0,
                    CDSEG_F32 << CDSEG_ROUTE_F_CT_SHIFT, np);
    hipLaunchKernelGGL((loss_bwd_kernel<decltype(G)::value, decltype(E)::value>), dim3(row_blocks), dim3(256), 0,
                       (hipStream_t)stream, logits, ldl, labels, n, c, ignore_index, tab, np, coef, g_ce, g_lovasz, inv_valid,
                       dlogits, lddl);
  });
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

}  // extern "C"
