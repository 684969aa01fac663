// Skip-connection options of SerializedUnpooling: the post-activation skip scale of the 'add' mode and FreeU's Fourier filter
// of the skip feature.
// ref: ptv3.py:42-100 (Fourier_filter / freeU), :607-626 (scaling, FreeU, merge).  Definitions and limits: include/cdseg.h.
//
// The reference filters x (1, C, N) with a 2-D FFT whose mask is constant along the channel-frequency axis and scales the
// N-frequencies 0 and -1 only.  The real part it keeps is therefore, per channel c and REFERENCE row n (theta_n = 2 pi n / N):
//   y[n][c] = x[n][c] + k (S0_c + A_c cos theta_n + B_c sin theta_n),   k = (float32(s) - 1) / N,
//   S0_c = sum_m x[m][c],  A_c = sum_m x[m][c] cos theta_m,  B_c = sum_m x[m][c] sin theta_m
// - three column sums (cdseg_skip_stats) and one element-wise pass (cdseg_skip_merge) that also applies the skip scale f and
// adds the unpooled child row.  The operator is I + k P with P symmetric: its backward is the same pair of calls.
// On the vector path (c a multiple of 4, operands aligned for 4 elements per access) the thread map of csrc/colsum.h
// (colsum::RowMap), a thread keeps ONE column group for its lifetime; the scalar path (any other c or alignment) moves one
// element per access with the same arithmetic.
// Arithmetic: cos / sin in fp64 (sincospi(2 n / N)), every element-wise expression in fp64 from the stored operands and rounded
// to fp32 once.  The sums are accumulated in fp64 in the fixed order of csrc/colsum.h: chunks (its blocks) of 64 rows at least,
// the chunk partials (workspace) added in 16 segments of consecutive chunks (SEGS = 16: 256 chunks are 16 of 16).  No float atomics: a
// sum is a function of (n, c), the path and the data alone.
#include <hip/hip_runtime.h>

#include "colsum.h"
#include "common.h"
#include "route.h"

namespace {

using colsum::aligned;

constexpr int SK_THREADS = colsum::THREADS;
constexpr int SK_WIDTH = 1;         // any c in [1, 512]
constexpr int SK_SEGS = 16;         // the finish of the statistics
constexpr long SK_MAX_GRID = 4096;  // merge: grid-strided beyond

struct SkP {
  const void* src;         // stats: the skip feature, fp32 or the build's 16-bit type
  float* x;                // merge: the fp32 stream, in place
  const float* child;
  const int32_t* ref; const int32_t* cluster;
  const double* stats;     // merge: [S0 A B] (3 c), or the folded [u0 u1 u2]
  double* ws;
  double k, f, inv_n2;     // inv_n2 = 2 / N: theta_n / pi = n inv_n2
  long n, rows_per_chunk;
  int c, ld, ldchild, folded;
};

__device__ __forceinline__ void sk_angle(const SkP& p, long row, double& cs, double& sn) {
  const long n = p.ref ? (long)p.ref[row] : row;
  sincospi((double)n * p.inv_n2, &sn, &cs);
}

template <bool LP>
__device__ __forceinline__ void sk_load4(const void* base, long off, double v[4]) {
  if constexpr (LP) {
    const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const bf16_t*>(base) + off);
    float a, b, c, d;
    unpack_bf16x2(u.x, a, b);
    unpack_bf16x2(u.y, c, d);
    v[0] = a; v[1] = b; v[2] = c; v[3] = d;
  } else {
    const float4 u = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(base) + off);
    v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
  }
}

// ws[chunk][3 c] = the chunk's [S0 A B].
template <bool LP>
__global__ __launch_bounds__(SK_THREADS) void sk_stats_kernel(SkP p) {
  const colsum::RowMap t(p.c);
  const int c = p.c, R = t.R, l = t.l;
  double acc[3][4] = {};  // S0, A, B
  if (t.active) {
    const long row0 = (long)blockIdx.x * p.rows_per_chunk;
    const long row1 = row0 + p.rows_per_chunk < p.n ? row0 + p.rows_per_chunk : p.n;
    for (long i = row0 + t.r; i < row1; i += R) {
      double v[4], cs, sn;
      sk_load4<LP>(p.src, i * p.ld + 4 * l, v);
      sk_angle(p, i, cs, sn);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc[0][e] += v[e];
        acc[1][e] += v[e] * cs;
        acc[2][e] += v[e] * sn;
      }
    }
  }
  colsum::block_fold<3>(acc, t, c, p.ws + (long)blockIdx.x * 3 * c);
}

template <bool LP>
__global__ __launch_bounds__(SK_THREADS) void sk_stats_scalar_kernel(SkP p) {
  const int c = p.c;
  const long row0 = (long)blockIdx.x * p.rows_per_chunk;
  const long row1 = row0 + p.rows_per_chunk < p.n ? row0 + p.rows_per_chunk : p.n;
  for (int j = threadIdx.x; j < c; j += SK_THREADS) {
    double s0 = 0.0, a = 0.0, b = 0.0;
    for (long i = row0; i < row1; ++i) {
      double cs, sn;
      sk_angle(p, i, cs, sn);
      const long off = i * p.ld + j;
      const double v = LP ? (double)bf16_to_f32(reinterpret_cast<const bf16_t*>(p.src)[off])
                          : (double)reinterpret_cast<const float*>(p.src)[off];
      s0 += v;
      a += v * cs;
      b += v * sn;
    }
    double* w = p.ws + (long)blockIdx.x * 3 * c;
    w[j] = s0;
    w[c + j] = a;
    w[2 * c + j] = b;
  }
}

// One element of the merge: v = x; with stats v += k (S0 + A cos + B sin), all of it times f (folded: only the added term is
// times f, x carries f already); then + child.
__device__ __forceinline__ float sk_element(const SkP& p, double x, double s0, double a, double b, double cs, double sn,
                                            bool filt, bool has_child, double ch) {
  double v;
  if (filt) {
    const double t = p.k * (s0 + a * cs + b * sn);
    v = p.folded ? x + p.f * t : p.f * (x + t);
  } else {
    v = p.f * x;
  }
  if (has_child) v += ch;
  return (float)v;
}

__global__ __launch_bounds__(SK_THREADS) void sk_merge_kernel(SkP p) {
  const colsum::RowMap t(p.c);
  if (!t.active) return;
  const int c = p.c, R = t.R, r = t.r, l = t.l;
  const bool filt = p.stats != nullptr, has_child = p.child != nullptr;
  double s0[4] = {0.0, 0.0, 0.0, 0.0}, a[4] = {0.0, 0.0, 0.0, 0.0}, b[4] = {0.0, 0.0, 0.0, 0.0};
  if (filt) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s0[e] = p.stats[4 * l + e];
      a[e] = p.stats[c + 4 * l + e];
      b[e] = p.stats[2 * c + 4 * l + e];
    }
  }
  for (long i = (long)blockIdx.x * R + r; i < p.n; i += (long)gridDim.x * R) {
    float* xp = p.x + i * p.ld + 4 * l;
    const float4 xv = *reinterpret_cast<const float4*>(xp);
    const float x4[4] = {xv.x, xv.y, xv.z, xv.w};
    float c4[4] = {0.f, 0.f, 0.f, 0.f};
    if (has_child) {
      const float4 cv = *reinterpret_cast<const float4*>(p.child + (long)p.cluster[i] * p.ldchild + 4 * l);
      c4[0] = cv.x; c4[1] = cv.y; c4[2] = cv.z; c4[3] = cv.w;
    }
    double cs = 1.0, sn = 0.0;
    if (filt) sk_angle(p, i, cs, sn);
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = sk_element(p, (double)x4[e], s0[e], a[e], b[e], cs, sn, filt, has_child, (double)c4[e]);
    *reinterpret_cast<float4*>(xp) = make_float4(o[0], o[1], o[2], o[3]);
  }
}

__global__ __launch_bounds__(SK_THREADS) void sk_merge_scalar_kernel(SkP p) {
  const long total = p.n * p.c;
  const bool filt = p.stats != nullptr, has_child = p.child != nullptr;
  for (long t = (long)blockIdx.x * SK_THREADS + threadIdx.x; t < total; t += (long)gridDim.x * SK_THREADS) {
    const long i = t / p.c;
    const int j = (int)(t - i * p.c);
    double cs = 1.0, sn = 0.0, s0 = 0.0, a = 0.0, b = 0.0;
    if (filt) {
      sk_angle(p, i, cs, sn);
      s0 = p.stats[j]; a = p.stats[p.c + j]; b = p.stats[2 * p.c + j];
    }
    const double ch = has_child ? (double)p.child[(long)p.cluster[i] * p.ldchild + j] : 0.0;
    float* xp = p.x + i * p.ld + j;
    *xp = sk_element(p, (double)*xp, s0, a, b, cs, sn, filt, has_child, ch);
  }
}

// u[j][o] = sum_i W[o][i] stats[j][i], j = 0..2: block o, lane q adds i = q, q + 64, ... by ascending i, the 64 lane sums are
// added by ascending lane.
template <bool LP>
__global__ __launch_bounds__(64) void sk_fold_kernel(const void* __restrict__ w, int ldw, int cin, int cout,
                                                     const double* __restrict__ stats, double* __restrict__ u) {
  __shared__ double red[3 * 64];
  const int o = blockIdx.x, q = threadIdx.x;
  double t[3] = {0.0, 0.0, 0.0};
  for (int i = q; i < cin; i += 64) {
    const long off = (long)o * ldw + i;
    const double wv = LP ? (double)bf16_to_f32(reinterpret_cast<const bf16_t*>(w)[off]) : (double)reinterpret_cast<const float*>(w)[off];
#pragma unroll
    for (int j = 0; j < 3; ++j) t[j] += wv * stats[j * cin + i];
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) red[j * 64 + q] = t[j];
  __syncthreads();
  if (q < 3) {
    double v = red[q * 64];
    for (int e = 1; e < 64; ++e) v += red[q * 64 + e];
    u[q * cout + o] = v;
  }
}

}  // namespace

extern "C" {

int cdseg_skip_partition(long n, int c, long* rows_per_chunk, int* chunks) {
  if (n < 0 || !rows_per_chunk || !chunks) return CDSEG_ERR_ARG;
  if (!colsum::width_ok(c, SK_WIDTH)) return CDSEG_ERR_UNSUPPORTED;
  const colsum::Partition q = colsum::partition(n, colsum::MIN_ROWS_SWEEP);
  *rows_per_chunk = q.rows_per_block;
  *chunks = q.blocks;
  return CDSEG_OK;
}

size_t cdseg_skip_stats_ws_bytes(long n, int c) {
  return colsum::width_ok(c, SK_WIDTH) ? colsum::ws_bytes(n, 3, c, colsum::MIN_ROWS_SWEEP) : 0;
}

int cdseg_skip_stats(const void* x, int dtype, int ldx, long n, int c, const int32_t* ref_of_row, long n_total, double* stats,
                     void* ws, size_t ws_bytes, void* stream) {
  if (n < 0 || (dtype != CDSEG_F32 && dtype != CDSEG_BF16)) return CDSEG_ERR_ARG;
  if (!colsum::width_ok(c, SK_WIDTH)) return CDSEG_ERR_UNSUPPORTED;
  if (n >= (1L << 31) || n_total >= (1L << 31)) return CDSEG_ERR_UNSUPPORTED;  // the row map is int32
  if (n == 0) return CDSEG_OK;
  const bool lp = dtype == CDSEG_BF16;
  if (!x || !stats || ldx < c || n_total < n || !aligned(lp ? 1 : 3, x) || !aligned(3, ref_of_row) || !aligned(7, stats))
    return CDSEG_ERR_ARG;
  if (ws && !aligned(15, ws)) return CDSEG_ERR_ARG;
  if (!ws || ws_bytes < cdseg_skip_stats_ws_bytes(n, c)) return CDSEG_ERR_WORKSPACE;
  SkP p = {};
  p.src = x; p.ref = ref_of_row; p.ws = (double*)ws; p.n = n; p.c = c; p.ld = ldx; p.inv_n2 = 2.0 / (double)n_total;
  const colsum::Partition part = colsum::partition(n, colsum::MIN_ROWS_SWEEP);
  const int chunks = part.blocks;
  p.rows_per_chunk = part.rows_per_block;
  hipStream_t q = (hipStream_t)stream;
  const bool vec = (c & 3) == 0 && (ldx & 3) == 0 && aligned(lp ? 7 : 15, x);
  const int rflags = (vec ? CDSEG_ROUTE_F_VEC_OK : 0) | (dtype << CDSEG_ROUTE_F_CT_SHIFT);
  if (vec && lp) {
    cdseg_route_rec(CDSEG_RK_SK_STATS_B16, 0, c, chunks, 0, 0, rflags, 0);
    hipLaunchKernelGGL(sk_stats_kernel<true>, dim3((unsigned)chunks), dim3(SK_THREADS), 0, q, p);
  } else if (vec) {
    cdseg_route_rec(CDSEG_RK_SK_STATS_F32, 0, c, chunks, 0, 0, rflags, 0);
    hipLaunchKernelGGL(sk_stats_kernel<false>, dim3((unsigned)chunks), dim3(SK_THREADS), 0, q, p);
  } else if (lp) {
    cdseg_route_rec(CDSEG_RK_SK_STATS_SCALAR_B16, 0, c, chunks, 0, 0, rflags, 0);
    hipLaunchKernelGGL(sk_stats_scalar_kernel<true>, dim3((unsigned)chunks), dim3(SK_THREADS), 0, q, p);
  } else {
    cdseg_route_rec(CDSEG_RK_SK_STATS_SCALAR_F32, 0, c, chunks, 0, 0, rflags, 0);
    hipLaunchKernelGGL(sk_stats_scalar_kernel<false>, dim3((unsigned)chunks), dim3(SK_THREADS), 0, q, p);
  }
  CDSEG_CHECK_LAUNCH();
  colsum::launch_reduce<SK_SEGS>(p.ws, chunks, 3 * c, stats, -1.0, q);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_skip_fold(const void* w, int dtype, int ldw, int cout, int cin, const double* stats, double* u, void* stream) {
  if (dtype != CDSEG_F32 && dtype != CDSEG_BF16) return CDSEG_ERR_ARG;
  if (!colsum::width_ok(cin, SK_WIDTH) || !colsum::width_ok(cout, SK_WIDTH)) return CDSEG_ERR_UNSUPPORTED;
  const bool lp = dtype == CDSEG_BF16;
  if (!w || !stats || !u || ldw < cin || !aligned(lp ? 1 : 3, w) || !aligned(7, stats) || !aligned(7, u)) return CDSEG_ERR_ARG;
  if (lp) {
    cdseg_route_rec(CDSEG_RK_SK_FOLD_B16, cout, cin, 1, 0, 0, CDSEG_BF16 << CDSEG_ROUTE_F_CT_SHIFT, 0);
    hipLaunchKernelGGL(sk_fold_kernel<true>, dim3((unsigned)cout), dim3(64), 0, (hipStream_t)stream, w, ldw, cin, cout, stats, u);
  } else {
    cdseg_route_rec(CDSEG_RK_SK_FOLD_F32, cout, cin, 1, 0, 0, CDSEG_F32 << CDSEG_ROUTE_F_CT_SHIFT, 0);
    hipLaunchKernelGGL(sk_fold_kernel<false>, dim3((unsigned)cout), dim3(64), 0, (hipStream_t)stream, w, ldw, cin, cout, stats, u);
  }
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_skip_merge(float* x, int ldx, long n, int c, const double* stats, int folded, double s, long n_total, double f,
                     const int32_t* ref_of_row, const float* child, int ldchild, const int32_t* cluster, long n_child, void* stream) {
  if (n < 0) return CDSEG_ERR_ARG;
  if (!colsum::width_ok(c, SK_WIDTH)) return CDSEG_ERR_UNSUPPORTED;
  if (n >= (1L << 31) || n_total >= (1L << 31) || n_child >= (1L << 31)) return CDSEG_ERR_UNSUPPORTED;
  if (n == 0) return CDSEG_OK;
  if (!x || ldx < c || !aligned(3, x) || !aligned(3, ref_of_row) || !aligned(3, child) || !aligned(3, cluster) ||
      !aligned(7, stats) || (stats && n_total < n) || (folded && !stats) || (child && (!cluster || n_child <= 0 || ldchild < c)) ||
      (!child && cluster) || !(f == f) || !(s == s))
    return CDSEG_ERR_ARG;
  SkP p = {};
  p.x = x; p.ld = ldx; p.n = n; p.c = c; p.stats = stats; p.folded = folded ? 1 : 0; p.f = f; p.ref = stats ? ref_of_row : nullptr;
  p.child = child; p.ldchild = ldchild; p.cluster = cluster;
  if (stats) {
    p.k = ((double)(float)s - 1.0) / (double)n_total;  // the reference's mask is a float32 tensor
    p.inv_n2 = 2.0 / (double)n_total;
  }
  const bool vec = (c & 3) == 0 && (ldx & 3) == 0 && aligned(15, x) && (!child || ((ldchild & 3) == 0 && aligned(15, child)));
  if (vec) {
    const unsigned grid = colsum::row_grid(n, c, 4, SK_MAX_GRID);  // about four rows a thread
    cdseg_route_rec(CDSEG_RK_SK_MERGE, 0, c, 1, 0, 0, CDSEG_ROUTE_F_VEC_OK | (CDSEG_F32 << CDSEG_ROUTE_F_CT_SHIFT), 0);
    hipLaunchKernelGGL(sk_merge_kernel, dim3(grid), dim3(SK_THREADS), 0, (hipStream_t)stream, p);
  } else {
    const unsigned grid = colsum::elem_grid(n * c, 4, SK_MAX_GRID);  // about four elements a thread
    cdseg_route_rec(CDSEG_RK_SK_MERGE_SCALAR, 0, c, 1, 0, 0, CDSEG_F32 << CDSEG_ROUTE_F_CT_SHIFT, 0);
    hipLaunchKernelGGL(sk_merge_scalar_kernel, dim3(grid), dim3(SK_THREADS), 0, (hipStream_t)stream, p);
  }
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

}  // extern "C"
