// The gate of the Feature Fusion Module (CrossBlock), forward and backward.
// ref: ptv3.py:1196-1206 - q_point.feat = q_shortcut + feat_scale * attn, or (1 - feat_scale) * q_shortcut + feat_scale * attn,
// feat_scale a number, a learned scalar or a learned per-channel vector behind a sigmoid; attn has been through DropPath.
// Definitions and limits: include/cdseg.h.
//
// With s = q_shortcut, a = the projected attention output, m = the per-row DropPath factor (mask / keep, or none) and the two
// per-channel vectors alpha, gamma the caller derives from the mode:
//   forward   y = alpha s + gamma m a
//   backward  ds = alpha dy,  da = gamma m dy,  sums = [sum_r dy m a (c), sum_r dy s (c)]
// Memory-bound row sweeps over contiguous fp32 (rows, c) tensors, c in [1, 512].  Vector path (c a multiple of 4 and every
// tensor and vector 16-byte aligned - every caller in this package): thread map as in norm.hip, a row is covered by L = c / 4
// lanes of 16 bytes each, a 256-thread block holds R = 256 / L rows at a time, a thread keeps ONE column group for its
// lifetime, so alpha and gamma are loaded once into registers.  Scalar path (any other c or alignment): one element per access,
// a thread owns whole columns of its block's rows.
// Arithmetic: every element-wise expression is evaluated in fp64 from the fp32 operands and rounded to fp32 once (the sweep is
// bound by memory, not by the arithmetic).  The two column sums are accumulated in fp64 and returned in fp64.  Block b owns the
// rows [b rows_per_block, ...); a thread adds its rows by ascending index, the R row slots of a block are added by ascending
// slot through LDS (scalar path: one thread adds a column's rows by ascending index), the block partials (workspace) by ascending
// block index by a second launch.  No float atomics: every sum is a function of (rows, c), the path and the data alone.
#include <hip/hip_runtime.h>

#include "common.h"
#include "route.h"

namespace {

constexpr int FG_THREADS = 256;
constexpr int FG_MIN_C = 1, FG_MAX_C = 512;
constexpr long FG_MIN_ROWS = 64;    // rows of a block at least (the bottleneck of one scene: ~2 k rows -> 32 blocks)
constexpr long FG_MAX_BLOCKS = 256; // block partials at most: the chain of the ascending reduce
constexpr long FG_MAX_GRID = 4096;  // forward: grid-strided beyond

inline void fg_partition(long rows, long& rows_per_block, int& blocks) {
  long rpb = (rows + FG_MAX_BLOCKS - 1) / FG_MAX_BLOCKS;
  rpb = rpb < FG_MIN_ROWS ? FG_MIN_ROWS : (rpb + 63) / 64 * 64;
  rows_per_block = rpb;
  blocks = rows > 0 ? (int)((rows + rpb - 1) / rpb) : 0;
}

struct FgP {
  const float* s; const float* a; const float* m; const float* dy; const float* alpha; const float* gamma;
  float* y; float* ds; float* da;
  double* ws;
  long rows, rows_per_block;
  int c;
};

// y = alpha s + gamma m a (a NULL: y = alpha s).  y may be s: an element is read and written by the same thread.
__global__ __launch_bounds__(FG_THREADS) void fg_fwd_kernel(FgP p) {
  const int c = p.c, L = c >> 2, R = FG_THREADS / L;
  const int r = (int)threadIdx.x / L, l = (int)threadIdx.x - r * L;
  if (r >= R) return;
  const float4 al = *reinterpret_cast<const float4*>(p.alpha + 4 * l);
  const float4 ga = *reinterpret_cast<const float4*>(p.gamma + 4 * l);
  const double a4[4] = {al.x, al.y, al.z, al.w}, g4[4] = {ga.x, ga.y, ga.z, ga.w};
  for (long i = (long)blockIdx.x * R + r; i < p.rows; i += (long)gridDim.x * R) {
    const long off = i * c + 4 * l;
    const float4 sv = *reinterpret_cast<const float4*>(p.s + off);
    const float s4[4] = {sv.x, sv.y, sv.z, sv.w};
    float o[4];
    if (p.a) {
      const float4 av = *reinterpret_cast<const float4*>(p.a + off);
      const float v4[4] = {av.x, av.y, av.z, av.w};
      const double mr = p.m ? (double)p.m[i] : 1.0;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (float)(a4[e] * (double)s4[e] + g4[e] * mr * (double)v4[e]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (float)(a4[e] * (double)s4[e]);
    }
    *reinterpret_cast<float4*>(p.y + off) = make_float4(o[0], o[1], o[2], o[3]);
  }
}

// ds = alpha dy, da = gamma m dy; ws[block][2 c] = the block's sums of dy m a and of dy s.  ds may be dy.
__global__ __launch_bounds__(FG_THREADS) void fg_bwd_kernel(FgP p) {
  __shared__ double red[FG_THREADS * 8];  // R row slots x 2 c sums (R * c <= 1024)
  const int c = p.c, L = c >> 2, R = FG_THREADS / L;
  const int r = (int)threadIdx.x / L, l = (int)threadIdx.x - r * L;
  if (r < R) {
    double u[4] = {0.0, 0.0, 0.0, 0.0}, w[4] = {0.0, 0.0, 0.0, 0.0};
    const long row0 = (long)blockIdx.x * p.rows_per_block;
    const long row1 = row0 + p.rows_per_block < p.rows ? row0 + p.rows_per_block : p.rows;
    const float4 al = *reinterpret_cast<const float4*>(p.alpha + 4 * l);
    const float4 ga = *reinterpret_cast<const float4*>(p.gamma + 4 * l);
    const double a4[4] = {al.x, al.y, al.z, al.w}, g4[4] = {ga.x, ga.y, ga.z, ga.w};
    for (long i = row0 + r; i < row1; i += R) {
      const long off = i * c + 4 * l;
      const float4 dv = *reinterpret_cast<const float4*>(p.dy + off);
      const float4 sv = *reinterpret_cast<const float4*>(p.s + off);
      const float4 av = *reinterpret_cast<const float4*>(p.a + off);
      const float d4[4] = {dv.x, dv.y, dv.z, dv.w}, s4[4] = {sv.x, sv.y, sv.z, sv.w}, v4[4] = {av.x, av.y, av.z, av.w};
      const double mr = p.m ? (double)p.m[i] : 1.0;
      float os[4], oa[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double d = (double)d4[e], dm = d * mr;  // (exact: a 48-bit product)
        os[e] = (float)(a4[e] * d);
        oa[e] = (float)(g4[e] * dm);
        u[e] += dm * (double)v4[e];
        w[e] += d * (double)s4[e];
      }
      *reinterpret_cast<float4*>(p.ds + off) = make_float4(os[0], os[1], os[2], os[3]);
      *reinterpret_cast<float4*>(p.da + off) = make_float4(oa[0], oa[1], oa[2], oa[3]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      red[r * 2 * c + 4 * l + e] = u[e];
      red[r * 2 * c + c + 4 * l + e] = w[e];
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < 2 * c; j += FG_THREADS) {
    double t = red[j];
    for (int q = 1; q < R; ++q) t += red[q * 2 * c + j];
    p.ws[(long)blockIdx.x * 2 * c + j] = t;
  }
}

// The scalar path of the two kernels above: any c, 4-byte aligned operands, the same arithmetic.
__global__ __launch_bounds__(FG_THREADS) void fg_fwd_scalar_kernel(FgP p) {
  const long total = p.rows * p.c;
  for (long t = (long)blockIdx.x * FG_THREADS + threadIdx.x; t < total; t += (long)gridDim.x * FG_THREADS) {
    const long i = t / p.c;
    const int j = (int)(t - i * p.c);
    double v = (double)p.alpha[j] * (double)p.s[t];
    if (p.a) v += (double)p.gamma[j] * (p.m ? (double)p.m[i] : 1.0) * (double)p.a[t];
    p.y[t] = (float)v;
  }
}

__global__ __launch_bounds__(FG_THREADS) void fg_bwd_scalar_kernel(FgP p) {
  const int c = p.c;
  const long row0 = (long)blockIdx.x * p.rows_per_block;
  const long row1 = row0 + p.rows_per_block < p.rows ? row0 + p.rows_per_block : p.rows;
  for (int j = threadIdx.x; j < c; j += FG_THREADS) {
    const double al = (double)p.alpha[j], ga = (double)p.gamma[j];
    double u = 0.0, w = 0.0;
    for (long i = row0; i < row1; ++i) {
      const long off = i * c + j;
      const double d = (double)p.dy[off], dm = d * (p.m ? (double)p.m[i] : 1.0);
      const double sv = (double)p.s[off], av = (double)p.a[off];  // (read before ds is written: ds may be dy)
      p.ds[off] = (float)(al * d);
      p.da[off] = (float)(ga * dm);
      u += dm * av;
      w += d * sv;
    }
    p.ws[(long)blockIdx.x * 2 * c + j] = u;
    p.ws[(long)blockIdx.x * 2 * c + c + j] = w;
  }
}

// Thread i < 2 c: t = p[0]; t += p[1]; ... by ascending block index.
__global__ __launch_bounds__(64) void fg_reduce_kernel(const double* __restrict__ ws, int blocks, int c, double* __restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= 2 * c) return;
  const double* p = ws + i;
  double t = p[0];
  for (int b = 1; b < blocks; ++b) t += p[(long)b * 2 * c];
  out[i] = t;
}

int fg_width_status(int c) { return (c < FG_MIN_C || c > FG_MAX_C) ? CDSEG_ERR_UNSUPPORTED : CDSEG_OK; }

template <typename... P>
bool fg_aligned(uintptr_t mask, const P*... ptr) { return ((((uintptr_t)ptr) | ...) & mask) == 0; }

}  // namespace

extern "C" {

size_t cdseg_fuse_gate_ws_bytes(long rows, int c) {
  if (rows <= 0 || fg_width_status(c) != CDSEG_OK) return 0;
  long rpb;
  int blocks;
  fg_partition(rows, rpb, blocks);
  return (size_t)blocks * 2 * (size_t)c * sizeof(double);
}

int cdseg_fuse_gate_fwd(const float* s, const float* a, const float* m, const float* alpha, const float* gamma, float* y,
                        long rows, int c, void* stream) {
  if (rows < 0) return CDSEG_ERR_ARG;
  const int st = fg_width_status(c);
  if (st != CDSEG_OK) return st;
  if (rows == 0) return CDSEG_OK;
  if (!s || !alpha || !gamma || !y || !fg_aligned(3, s, a, m, alpha, gamma, y) || (m && !a)) return CDSEG_ERR_ARG;
  FgP p = {};
  p.s = s; p.a = a; p.m = m; p.alpha = alpha; p.gamma = gamma; p.y = y; p.rows = rows; p.c = c;
  if ((c & 3) == 0 && fg_aligned(15, s, a, alpha, gamma, y)) {
    const int R = FG_THREADS / (c >> 2);
    long blocks = (rows + (long)R * 4 - 1) / ((long)R * 4);  // about four rows a thread
    blocks = blocks < 1 ? 1 : (blocks > FG_MAX_GRID ? FG_MAX_GRID : blocks);
    cdseg_route_rec(CDSEG_RK_FG_FWD, 0, c, 1, 0, 0, CDSEG_ROUTE_F_VEC_OK | (CDSEG_F32 << CDSEG_ROUTE_F_CT_SHIFT), 0);
    hipLaunchKernelGGL(fg_fwd_kernel, dim3((unsigned)blocks), dim3(FG_THREADS), 0, (hipStream_t)stream, p);
  } else {
    long blocks = (rows * c + (long)FG_THREADS * 4 - 1) / ((long)FG_THREADS * 4);  // about four elements a thread
    blocks = blocks < 1 ? 1 : (blocks > FG_MAX_GRID ? FG_MAX_GRID : blocks);
    cdseg_route_rec(CDSEG_RK_FG_FWD_SCALAR, 0, c, 1, 0, 0, CDSEG_F32 << CDSEG_ROUTE_F_CT_SHIFT, 0);
    hipLaunchKernelGGL(fg_fwd_scalar_kernel, dim3((unsigned)blocks), dim3(FG_THREADS), 0, (hipStream_t)stream, p);
  }
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_fuse_gate_bwd(const float* dy, const float* s, const float* a, const float* m, const float* alpha, const float* gamma,
                        float* ds, float* da, double* sums, long rows, int c, void* ws, size_t ws_bytes, void* stream) {
  if (rows < 0) return CDSEG_ERR_ARG;
  const int st = fg_width_status(c);
  if (st != CDSEG_OK) return st;
  if (rows == 0) return CDSEG_OK;
  if (!dy || !s || !a || !alpha || !gamma || !ds || !da || !sums || !fg_aligned(3, dy, s, a, m, alpha, gamma, ds, da) ||
      ((uintptr_t)sums & 7))
    return CDSEG_ERR_ARG;
  if (ws && !fg_aligned(15, ws)) return CDSEG_ERR_ARG;
  if (!ws || ws_bytes < cdseg_fuse_gate_ws_bytes(rows, c)) return CDSEG_ERR_WORKSPACE;
  FgP p = {};
  p.dy = dy; p.s = s; p.a = a; p.m = m; p.alpha = alpha; p.gamma = gamma; p.ds = ds; p.da = da; p.ws = (double*)ws;
  p.rows = rows; p.c = c;
  int blocks;
  fg_partition(rows, p.rows_per_block, blocks);
  hipStream_t q = (hipStream_t)stream;
  if ((c & 3) == 0 && fg_aligned(15, dy, s, a, alpha, gamma, ds, da)) {
    cdseg_route_rec(CDSEG_RK_FG_BWD, 0, c, blocks, 0, 0, CDSEG_ROUTE_F_VEC_OK | (CDSEG_F32 << CDSEG_ROUTE_F_CT_SHIFT), 0);
    hipLaunchKernelGGL(fg_bwd_kernel, dim3((unsigned)blocks), dim3(FG_THREADS), 0, q, p);
  } else {
    cdseg_route_rec(CDSEG_RK_FG_BWD_SCALAR, 0, c, blocks, 0, 0, CDSEG_F32 << CDSEG_ROUTE_F_CT_SHIFT, 0);
    hipLaunchKernelGGL(fg_bwd_scalar_kernel, dim3((unsigned)blocks), dim3(FG_THREADS), 0, q, p);
  }
  CDSEG_CHECK_LAUNCH();
  hipLaunchKernelGGL(fg_reduce_kernel, dim3((unsigned)cdiv(2 * c, 64)), dim3(64), 0, q, (const double*)ws, blocks, c, sums);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

}  // extern "C"
