// Train-mode BatchNorm1d + GELU (forward and backward) and the pooling maximum with its arg-max (forward and backward).
// ref: what torch autograd runs for nn.BatchNorm1d(training) -> nn.GELU at the stems, SerializedPooling.norm and the two
// projections of SerializedUnpooling (ptv3.py:464-555, 597-663), nn.SyncBatchNorm under engines/train.py:275-276, and
// torch_scatter.segment_csr(reduce="max") with its arg-max backward (ptv3.py:510-515).  Definitions and limits: include/cdseg.h.
//
// All kernels are memory-bound row sweeps over fp32 (rows, c) tensors with a row stride, c a multiple of 16 in [16, 512], on
// the thread map of csrc/colsum.h (colsum::RowMap): a thread keeps ONE column group for its lifetime, so the per-channel
// operands (mean, invstd, gamma, beta) are loaded once into registers.
// Arithmetic: fp64 throughout, one rounding per fp32 output.  Reductions (statistics, backward sums): the fixed order of
// csrc/colsum.h over the blocks of cdseg_bn_partition, the block partials added in one chain (SEGS = 1).  No float atomics:
// every sum is a function of (m, c) and the data alone.
#include <hip/hip_runtime.h>

#include "colsum.h"
#include "common.h"

namespace {

using colsum::aligned;
using colsum::ld_ok;
using colsum::row_grid;

constexpr int BN_THREADS = colsum::THREADS;
constexpr int BN_WIDTH = 16;        // c = 16, 32, .. 512
constexpr long BN_MAX_GRID = 2048;  // the row sweeps: grid-strided beyond

// Element-wise arithmetic: fp64 from the fp32 operands, ONE rounding to fp32 at the store (as in csrc/loss.hip: memory bounds
// these passes, not the arithmetic).  In fp32 the chain x_hat -> z -> GELU'(z) -> g - k1 - x_hat k2 -> gamma invstd (...) is
// six roundings of 2^-24 each: measured at 2e-7 of dx on a two-row column where torch's own fp32 chain happened to lose
// 3e-8 - over the fp64 yardstick of tests/test_gpu_norm.py.  What remains is the fp32 rounding of mean and invstd themselves.
__device__ __forceinline__ void bn_z(float x, float mean, float invstd, float gamma, float beta, double& xh, double& z) {
  xh = ((double)x - (double)mean) * (double)invstd;
  z = fma((double)gamma, xh, (double)beta);
}

// GELU(t) = t Phi(t), Phi(t) = erfc(-t / sqrt 2) / 2: no cancellation on the negative tail
__device__ __forceinline__ double gelu_fwd(double t) { return t * (0.5 * erfc(t * -0.70710678118654752440)); }

// GELU'(t) = Phi(t) + t phi(t)
__device__ __forceinline__ double gelu_grad(double t) {
  return 0.5 * erfc(t * -0.70710678118654752440) + t * (0.39894228040143267794 * exp(-0.5 * t * t));
}

struct BnP {
  const float* x; const float* dy; const float* mean; const float* invstd; const float* gamma; const float* beta;
  long m, rows_per_block;
  int c, ldx, lddy;
  double* ws;
};

// MODE 0: per-channel sum x, sum x^2.  MODE 1: sum g, sum g x_hat with g = dy GELU'(z).  ws[block][2 c].
template <int MODE>
__global__ __launch_bounds__(BN_THREADS) void bn_partial_kernel(BnP p) {
  const colsum::RowMap t(p.c);
  const int c = p.c, R = t.R, l = t.l;
  double acc[2][4] = {};
  if (t.active) {
    const long row0 = (long)blockIdx.x * p.rows_per_block;
    const long row1 = row0 + p.rows_per_block < p.m ? row0 + p.rows_per_block : p.m;
    float4 mu = {0.f, 0.f, 0.f, 0.f}, is = mu, ga = mu, be = mu;
    if constexpr (MODE == 1) {
      mu = *reinterpret_cast<const float4*>(p.mean + 4 * l);
      is = *reinterpret_cast<const float4*>(p.invstd + 4 * l);
      ga = *reinterpret_cast<const float4*>(p.gamma + 4 * l);
      be = *reinterpret_cast<const float4*>(p.beta + 4 * l);
    }
#pragma unroll 2  // (MODE 1 carries an fp64 erfc and exp per element: registers, not loads in flight, are what is scarce)
    for (long i = row0 + t.r; i < row1; i += R) {
      const float4 v = *reinterpret_cast<const float4*>(p.x + i * p.ldx + 4 * l);
      const float xv[4] = {v.x, v.y, v.z, v.w};
      if constexpr (MODE == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const double d = (double)xv[e];
          acc[0][e] += d;
          acc[1][e] += d * d;  // (exact: a 48-bit product)
        }
      } else {
        const float4 d4 = *reinterpret_cast<const float4*>(p.dy + i * p.lddy + 4 * l);
        const float dv[4] = {d4.x, d4.y, d4.z, d4.w};
        const float m4[4] = {mu.x, mu.y, mu.z, mu.w}, i4[4] = {is.x, is.y, is.z, is.w};
        const float g4[4] = {ga.x, ga.y, ga.z, ga.w}, b4[4] = {be.x, be.y, be.z, be.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          double xh, z;
          bn_z(xv[e], m4[e], i4[e], g4[e], b4[e], xh, z);
          const double g = (double)dv[e] * gelu_grad(z);
          acc[0][e] += g;
          acc[1][e] += g * xh;
        }
      }
    }
  }
  colsum::block_fold<2>(acc, t, c, p.ws + (long)blockIdx.x * 2 * c);
}

__global__ __launch_bounds__(64) void bn_finish_kernel(const double* __restrict__ stats, int c, double eps, double momentum,
                                                       float* __restrict__ mean, float* __restrict__ invstd, float* running_mean,
                                                       float* running_var) {
#pragma clang fp contract(off)
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= c) return;
  const double n = stats[2 * c], s1 = stats[j], s2 = stats[c + j];
  const double mu = s1 / n;
  // n^2 var = n s2 - s1^2 with both products carried as exact (high, low) pairs: the cancellation then loses nothing beyond
  // the rounding s2 itself carries.  (s2 / n - mu^2 rounds mu^2 and the quotient as well: for a column 1000 + 0.01 N(0, 1)
  // that is 2e-10 against var + eps = 1e-3, i.e. 2e-7 of dx - three times what fp32 torch loses at m = 2.)
  const double ph = s1 * s1, pl = fma(s1, s1, -ph);
  const double ah = n * s2, al = fma(n, s2, -ah);
  double var = ((ah - ph) + (al - pl)) / (n * n);
  if (var < 0.0) var = 0.0;  // (rounding of the sums; a NaN stays a NaN)
  mean[j] = (float)mu;
  invstd[j] = (float)(1.0 / sqrt(var + eps));
  if (running_mean) running_mean[j] = (float)((1.0 - momentum) * (double)running_mean[j] + momentum * mu);
  if (running_var) {
    const double unbiased = n > 1.0 ? var * (n / (n - 1.0)) : var;
    running_var[j] = (float)((1.0 - momentum) * (double)running_var[j] + momentum * unbiased);
  }
}

struct BnEwP {
  const float* x; const float* dy; const float* mean; const float* invstd; const float* gamma; const float* beta;
  const double* gsums; const double* count;
  float* out;
  long m;
  int c, ldx, lddy, ldo;
};

// MODE 0: y = GELU(z).  MODE 1: dx = gamma invstd (g - sum g / n - x_hat sum g x_hat / n).
template <int MODE>
__global__ __launch_bounds__(BN_THREADS) void bn_rows_kernel(BnEwP p) {
  const colsum::RowMap t(p.c);
  if (!t.active) return;
  const int c = p.c, R = t.R, r = t.r, l = t.l;
  const float4 mu = *reinterpret_cast<const float4*>(p.mean + 4 * l);
  const float4 is = *reinterpret_cast<const float4*>(p.invstd + 4 * l);
  const float4 ga = *reinterpret_cast<const float4*>(p.gamma + 4 * l);
  const float4 be = *reinterpret_cast<const float4*>(p.beta + 4 * l);
  const float m4[4] = {mu.x, mu.y, mu.z, mu.w}, i4[4] = {is.x, is.y, is.z, is.w};
  const float g4[4] = {ga.x, ga.y, ga.z, ga.w}, b4[4] = {be.x, be.y, be.z, be.w};
  double k1[4] = {0.0, 0.0, 0.0, 0.0}, k2[4] = {0.0, 0.0, 0.0, 0.0}, gi[4] = {0.0, 0.0, 0.0, 0.0};
  if constexpr (MODE == 1) {
    const double n = p.count[0];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      k1[e] = p.gsums[4 * l + e] / n;
      k2[e] = p.gsums[c + 4 * l + e] / n;
      gi[e] = (double)g4[e] * (double)i4[e];
    }
  }
#pragma unroll 2
  for (long i = (long)blockIdx.x * R + r; i < p.m; i += (long)gridDim.x * R) {
    const float4 v = *reinterpret_cast<const float4*>(p.x + i * p.ldx + 4 * l);
    const float xv[4] = {v.x, v.y, v.z, v.w};
    float o[4];
    if constexpr (MODE == 0) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        double xh, z;
        bn_z(xv[e], m4[e], i4[e], g4[e], b4[e], xh, z);
        o[e] = (float)gelu_fwd(z);
      }
    } else {
      const float4 d4 = *reinterpret_cast<const float4*>(p.dy + i * p.lddy + 4 * l);
      const float dv[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        double xh, z;
        bn_z(xv[e], m4[e], i4[e], g4[e], b4[e], xh, z);
        const double g = (double)dv[e] * gelu_grad(z);
        o[e] = (float)(gi[e] * ((g - k1[e]) - xh * k2[e]));
      }
    }
    *reinterpret_cast<float4*>(p.out + i * p.ldo + 4 * l) = make_float4(o[0], o[1], o[2], o[3]);
  }
}

// out[j] = max over the rows seg[j] .. seg[j + 1] - 1, arg[j] = the first row (ascending) that holds it.  A later row takes
// over only when strictly larger (torch_scatter's rule); a NaN never does, and a run of NaNs only leaves arg = -1 (no row
// equals the -inf it reports, which is what an `y == out` mask finds too).
__global__ __launch_bounds__(BN_THREADS) void segment_max_arg_kernel(const float* __restrict__ y, int ldy,
                                                                     const int32_t* __restrict__ seg, long m, int c,
                                                                     float* __restrict__ out, int ldo, int32_t* __restrict__ arg,
                                                                     int lda) {
  const colsum::RowMap t(c);
  if (!t.active) return;
  const int R = t.R, r = t.r, l = t.l;
  for (long j = (long)blockIdx.x * R + r; j < m; j += (long)gridDim.x * R) {
    const int s = seg[j], e = seg[j + 1];
    float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int32_t am[4] = {-1, -1, -1, -1};
    for (int i = s; i < e; ++i) {
      const float4 v = *reinterpret_cast<const float4*>(y + (long)i * ldy + 4 * l);
      const float xv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (xv[k] > mx[k] || (am[k] < 0 && xv[k] == mx[k])) { mx[k] = xv[k]; am[k] = i; }
    }
    // (cdseg_segment_max's epilogue with scale 1, shift 0: the same bits, a -0 maximum included)
#pragma unroll
    for (int k = 0; k < 4; ++k) mx[k] = __builtin_fmaf(mx[k], 1.0f, 0.0f);
    *reinterpret_cast<float4*>(out + j * ldo + 4 * l) = make_float4(mx[0], mx[1], mx[2], mx[3]);
    *reinterpret_cast<int4*>(arg + j * lda + 4 * l) = make_int4(am[0], am[1], am[2], am[3]);
  }
}

__global__ __launch_bounds__(BN_THREADS) void segment_max_bwd_kernel(const float* __restrict__ dout, int lddo,
                                                                     const int32_t* __restrict__ arg, int lda,
                                                                     const int32_t* __restrict__ cluster, long n, int c,
                                                                     float* __restrict__ dy, int lddy) {
  const colsum::RowMap t(c);
  if (!t.active) return;
  const int R = t.R, r = t.r, l = t.l;
#pragma unroll 2
  for (long i = (long)blockIdx.x * R + r; i < n; i += (long)gridDim.x * R) {
    const long j = cluster[i];
    const int4 a = *reinterpret_cast<const int4*>(arg + j * lda + 4 * l);
    const float4 d = *reinterpret_cast<const float4*>(dout + j * lddo + 4 * l);
    const int32_t ii = (int32_t)i;
    *reinterpret_cast<float4*>(dy + i * lddy + 4 * l) =
        make_float4(a.x == ii ? d.x : 0.f, a.y == ii ? d.y : 0.f, a.z == ii ? d.z : 0.f, a.w == ii ? d.w : 0.f);
  }
}


}  // namespace

extern "C" {

int cdseg_bn_partition(long m, int c, long* rows_per_block, int* blocks) {
  if (m < 0 || !rows_per_block || !blocks) return CDSEG_ERR_ARG;
  if (!colsum::width_ok(c, BN_WIDTH)) return CDSEG_ERR_UNSUPPORTED;
  const colsum::Partition q = colsum::partition(m, colsum::MIN_ROWS_BN);
  *rows_per_block = q.rows_per_block;
  *blocks = q.blocks;
  return CDSEG_OK;
}

size_t cdseg_bn_ws_bytes(long m, int c) {
  return colsum::width_ok(c, BN_WIDTH) ? colsum::ws_bytes(m, 2, c, colsum::MIN_ROWS_BN) : 0;
}

int cdseg_bn_stats(const float* x, int ldx, long m, int c, double* stats, void* ws, size_t ws_bytes, void* stream) {
  if (m < 0) return CDSEG_ERR_ARG;
  if (!colsum::width_ok(c, BN_WIDTH)) return CDSEG_ERR_UNSUPPORTED;
  if (m == 0) return CDSEG_OK;
  if (!x || !stats || !aligned(15, x) || ((uintptr_t)stats & 7) || !ld_ok(ldx, c)) return CDSEG_ERR_ARG;
  if (ws && !aligned(15, ws)) return CDSEG_ERR_ARG;
  if (!ws || ws_bytes < cdseg_bn_ws_bytes(m, c)) return CDSEG_ERR_WORKSPACE;
  BnP p = {};
  p.x = x; p.m = m; p.c = c; p.ldx = ldx; p.ws = (double*)ws;
  const colsum::Partition q = colsum::partition(m, colsum::MIN_ROWS_BN);
  p.rows_per_block = q.rows_per_block;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(bn_partial_kernel<0>, dim3((unsigned)q.blocks), dim3(BN_THREADS), 0, s, p);
  colsum::launch_reduce<1>(p.ws, q.blocks, 2 * c, stats, (double)m, s);  // (and stats[2 c] = m)
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_bn_finish(const double* stats, int c, double eps, double momentum, float* mean, float* invstd, float* running_mean,
                    float* running_var, void* stream) {
  if (!colsum::width_ok(c, BN_WIDTH)) return CDSEG_ERR_UNSUPPORTED;
  if (!stats || !mean || !invstd || ((uintptr_t)stats & 7) || !aligned(15, mean, invstd)) return CDSEG_ERR_ARG;
  if ((((uintptr_t)running_mean | (uintptr_t)running_var) & 3) || !(eps >= 0.0) || !(momentum >= 0.0 && momentum <= 1.0))
    return CDSEG_ERR_ARG;
  hipLaunchKernelGGL(bn_finish_kernel, dim3((unsigned)cdiv(c, 64)), dim3(64), 0, (hipStream_t)stream, stats, c, eps, momentum, mean,
                     invstd, running_mean, running_var);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_bn_gelu_fwd(const float* x, int ldx, long m, int c, const float* mean, const float* invstd, const float* gamma,
                      const float* beta, float* y, int ldy, void* stream) {
  if (m < 0) return CDSEG_ERR_ARG;
  if (!colsum::width_ok(c, BN_WIDTH)) return CDSEG_ERR_UNSUPPORTED;
  if (m == 0) return CDSEG_OK;
  if (!x || !mean || !invstd || !gamma || !beta || !y || !aligned(15, x, mean, invstd, gamma, beta, y) || !ld_ok(ldx, c) ||
      !ld_ok(ldy, c))
    return CDSEG_ERR_ARG;
  BnEwP p = {};
  p.x = x; p.mean = mean; p.invstd = invstd; p.gamma = gamma; p.beta = beta; p.out = y; p.m = m; p.c = c; p.ldx = ldx; p.ldo = ldy;
  hipLaunchKernelGGL(bn_rows_kernel<0>, dim3(row_grid(m, c, 4, BN_MAX_GRID)), dim3(BN_THREADS), 0, (hipStream_t)stream, p);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_bn_gelu_bwd_sums(const float* x, int ldx, const float* dy, int lddy, long m, int c, const float* mean,
                           const float* invstd, const float* gamma, const float* beta, double* gsums, void* ws, size_t ws_bytes,
                           void* stream) {
  if (m < 0) return CDSEG_ERR_ARG;
  if (!colsum::width_ok(c, BN_WIDTH)) return CDSEG_ERR_UNSUPPORTED;
  if (m == 0) return CDSEG_OK;
  if (!x || !dy || !mean || !invstd || !gamma || !beta || !gsums || !aligned(15, x, dy, mean, invstd, gamma, beta) ||
      ((uintptr_t)gsums & 7) || !ld_ok(ldx, c) || !ld_ok(lddy, c))
    return CDSEG_ERR_ARG;
  if (ws && !aligned(15, ws)) return CDSEG_ERR_ARG;
  if (!ws || ws_bytes < cdseg_bn_ws_bytes(m, c)) return CDSEG_ERR_WORKSPACE;
  BnP p = {};
  p.x = x; p.dy = dy; p.mean = mean; p.invstd = invstd; p.gamma = gamma; p.beta = beta;
  p.m = m; p.c = c; p.ldx = ldx; p.lddy = lddy; p.ws = (double*)ws;
  const colsum::Partition q = colsum::partition(m, colsum::MIN_ROWS_BN);
  p.rows_per_block = q.rows_per_block;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(bn_partial_kernel<1>, dim3((unsigned)q.blocks), dim3(BN_THREADS), 0, s, p);
  colsum::launch_reduce<1>(p.ws, q.blocks, 2 * c, gsums, -1.0, s);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_bn_gelu_bwd_dx(const float* x, int ldx, const float* dy, int lddy, long m, int c, const float* mean, const float* invstd,
                         const float* gamma, const float* beta, const double* gsums, const double* count, float* dx, int lddx,
                         void* stream) {
  if (m < 0) return CDSEG_ERR_ARG;
  if (!colsum::width_ok(c, BN_WIDTH)) return CDSEG_ERR_UNSUPPORTED;
  if (m == 0) return CDSEG_OK;
  if (!x || !dy || !mean || !invstd || !gamma || !beta || !gsums || !count || !dx ||
      !aligned(15, x, dy, mean, invstd, gamma, beta, dx) || (((uintptr_t)gsums | (uintptr_t)count) & 7) || !ld_ok(ldx, c) ||
      !ld_ok(lddy, c) || !ld_ok(lddx, c))
    return CDSEG_ERR_ARG;
  BnEwP p = {};
  p.x = x; p.dy = dy; p.mean = mean; p.invstd = invstd; p.gamma = gamma; p.beta = beta; p.gsums = gsums; p.count = count;
  p.out = dx; p.m = m; p.c = c; p.ldx = ldx; p.lddy = lddy; p.ldo = lddx;
  hipLaunchKernelGGL(bn_rows_kernel<1>, dim3(row_grid(m, c, 4, BN_MAX_GRID)), dim3(BN_THREADS), 0, (hipStream_t)stream, p);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_segment_max_arg(const float* y, int ldy, const int32_t* seg_start, long m, int c, float* out, int ldo, int32_t* arg,
                          int lda, void* stream) {
  if (m < 0) return CDSEG_ERR_ARG;
  if (!colsum::width_ok(c, BN_WIDTH)) return CDSEG_ERR_UNSUPPORTED;
  if (m >= (1L << 31)) return CDSEG_ERR_UNSUPPORTED;
  if (m == 0) return CDSEG_OK;
  if (!y || !seg_start || !out || !arg || !aligned(15, y, out, arg) || ((uintptr_t)seg_start & 3) || !ld_ok(ldy, c) ||
      !ld_ok(ldo, c) || !ld_ok(lda, c))
    return CDSEG_ERR_ARG;
  hipLaunchKernelGGL(segment_max_arg_kernel, dim3(row_grid(m, c, 2, BN_MAX_GRID)), dim3(BN_THREADS), 0, (hipStream_t)stream, y, ldy,
                     seg_start, m, c, out, ldo, arg, lda);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_segment_max_bwd(const float* dout, int lddo, const int32_t* arg, int lda, const int32_t* cluster, long n, int c,
                          float* dy, int lddy, void* stream) {
  if (n < 0) return CDSEG_ERR_ARG;
  if (!colsum::width_ok(c, BN_WIDTH)) return CDSEG_ERR_UNSUPPORTED;
  if (n >= (1L << 31)) return CDSEG_ERR_UNSUPPORTED;
  if (n == 0) return CDSEG_OK;
  if (!dout || !arg || !cluster || !dy || !aligned(15, dout, arg, dy) || ((uintptr_t)cluster & 3) || !ld_ok(lddo, c) ||
      !ld_ok(lda, c) || !ld_ok(lddy, c))
    return CDSEG_ERR_ARG;
  hipLaunchKernelGGL(segment_max_bwd_kernel, dim3(row_grid(n, c, 4, BN_MAX_GRID)), dim3(BN_THREADS), 0, (hipStream_t)stream, dout, lddo,
                     arg, lda, cluster, n, c, dy, lddy);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

}  // extern "C"
