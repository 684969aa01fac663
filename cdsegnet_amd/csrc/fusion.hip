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
// tensor and vector 16-byte aligned - every caller in this package): the thread map of csrc/colsum.h (colsum::RowMap), a thread
// keeps ONE column group for its lifetime, so alpha and gamma are loaded once into registers.  Scalar path (any other c or
// alignment): one element per access, a thread owns whole columns of its block's rows.
// Arithmetic: every element-wise expression is evaluated in fp64 from the fp32 operands and rounded to fp32 once (the sweep is
// bound by memory, not by the arithmetic).  The two column sums are accumulated in fp64 and returned in fp64, in the fixed order
// of csrc/colsum.h: 64-row blocks at least, the block partials (workspace) added in one chain (SEGS = 1).  No float atomics:
// every sum is a function of (rows, c), the path and the data alone.
#include <hip/hip_runtime.h>

#include "colsum.h"
#include "common.h"
#include "route.h"

namespace {

using colsum::aligned;

constexpr int FG_THREADS = colsum::THREADS;
constexpr int FG_WIDTH = 1;         // any c in [1, 512]
constexpr long FG_MAX_GRID = 4096;  // forward: grid-strided beyond

struct FgP {
  const float* s; const float* a; const float* m; const float* dy; const float* alpha; const float* gamma;
  float* y; float* ds; float* da;
  double* ws;
  long rows, rows_per_block;
  int c;
};

// y = alpha s + gamma m a (a NULL: y = alpha s).  y may be s: an element is read and written by the same thread.
__global__ __launch_bounds__(FG_THREADS) void fg_fwd_kernel(FgP p) {
  const colsum::RowMap t(p.c);
  if (!t.active) return;
  const int c = p.c, R = t.R, r = t.r, l = t.l;
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
  const colsum::RowMap t(p.c);
  const int c = p.c, R = t.R, l = t.l;
  double acc[2][4] = {};  // [0]: dy m a, [1]: dy s
  if (t.active) {
    const long row0 = (long)blockIdx.x * p.rows_per_block;
    const long row1 = row0 + p.rows_per_block < p.rows ? row0 + p.rows_per_block : p.rows;
    const float4 al = *reinterpret_cast<const float4*>(p.alpha + 4 * l);
    const float4 ga = *reinterpret_cast<const float4*>(p.gamma + 4 * l);
    const double a4[4] = {al.x, al.y, al.z, al.w}, g4[4] = {ga.x, ga.y, ga.z, ga.w};
    for (long i = row0 + t.r; i < row1; i += R) {
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
        acc[0][e] += dm * (double)v4[e];
        acc[1][e] += d * (double)s4[e];
      }
      *reinterpret_cast<float4*>(p.ds + off) = make_float4(os[0], os[1], os[2], os[3]);
      *reinterpret_cast<float4*>(p.da + off) = make_float4(oa[0], oa[1], oa[2], oa[3]);
    }
  }
  colsum::block_fold<2>(acc, t, c, p.ws + (long)blockIdx.x * 2 * c);
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

}  // namespace

extern "C" {

size_t cdseg_fuse_gate_ws_bytes(long rows, int c) {
  return colsum::width_ok(c, FG_WIDTH) ? colsum::ws_bytes(rows, 2, c, colsum::MIN_ROWS_SWEEP) : 0;
}

int cdseg_fuse_gate_fwd(const float* s, const float* a, const float* m, const float* alpha, const float* gamma, float* y,
                        long rows, int c, void* stream) {
  if (rows < 0) return CDSEG_ERR_ARG;
  if (!colsum::width_ok(c, FG_WIDTH)) return CDSEG_ERR_UNSUPPORTED;
  if (rows == 0) return CDSEG_OK;
  if (!s || !alpha || !gamma || !y || !aligned(3, s, a, m, alpha, gamma, y) || (m && !a)) return CDSEG_ERR_ARG;
  FgP p = {};
  p.s = s; p.a = a; p.m = m; p.alpha = alpha; p.gamma = gamma; p.y = y; p.rows = rows; p.c = c;
  if ((c & 3) == 0 && aligned(15, s, a, alpha, gamma, y)) {
    const unsigned grid = colsum::row_grid(rows, c, 4, FG_MAX_GRID);  // about four rows a thread
    cdseg_route_rec(CDSEG_RK_FG_FWD, 0, c, 1, 0, 0, CDSEG_ROUTE_F_VEC_OK | (CDSEG_F32 << CDSEG_ROUTE_F_CT_SHIFT), 0);
    hipLaunchKernelGGL(fg_fwd_kernel, dim3(grid), dim3(FG_THREADS), 0, (hipStream_t)stream, p);
  } else {
    const unsigned grid = colsum::elem_grid(rows * c, 4, FG_MAX_GRID);  // about four elements a thread
    cdseg_route_rec(CDSEG_RK_FG_FWD_SCALAR, 0, c, 1, 0, 0, CDSEG_F32 << CDSEG_ROUTE_F_CT_SHIFT, 0);
    hipLaunchKernelGGL(fg_fwd_scalar_kernel, dim3(grid), dim3(FG_THREADS), 0, (hipStream_t)stream, p);
  }
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_fuse_gate_bwd(const float* dy, const float* s, const float* a, const float* m, const float* alpha, const float* gamma,
                        float* ds, float* da, double* sums, long rows, int c, void* ws, size_t ws_bytes, void* stream) {
  if (rows < 0) return CDSEG_ERR_ARG;
  if (!colsum::width_ok(c, FG_WIDTH)) return CDSEG_ERR_UNSUPPORTED;
  if (rows == 0) return CDSEG_OK;
  if (!dy || !s || !a || !alpha || !gamma || !ds || !da || !sums || !aligned(3, dy, s, a, m, alpha, gamma, ds, da) ||
      ((uintptr_t)sums & 7))
    return CDSEG_ERR_ARG;
  if (ws && !aligned(15, ws)) return CDSEG_ERR_ARG;
  if (!ws || ws_bytes < cdseg_fuse_gate_ws_bytes(rows, c)) return CDSEG_ERR_WORKSPACE;
  FgP p = {};
  p.dy = dy; p.s = s; p.a = a; p.m = m; p.alpha = alpha; p.gamma = gamma; p.ds = ds; p.da = da; p.ws = (double*)ws;
  p.rows = rows; p.c = c;
  const colsum::Partition part = colsum::partition(rows, colsum::MIN_ROWS_SWEEP);
  const int blocks = part.blocks;
  p.rows_per_block = part.rows_per_block;
  hipStream_t q = (hipStream_t)stream;
  if ((c & 3) == 0 && aligned(15, dy, s, a, alpha, gamma, ds, da)) {
    cdseg_route_rec(CDSEG_RK_FG_BWD, 0, c, blocks, 0, 0, CDSEG_ROUTE_F_VEC_OK | (CDSEG_F32 << CDSEG_ROUTE_F_CT_SHIFT), 0);
    hipLaunchKernelGGL(fg_bwd_kernel, dim3((unsigned)blocks), dim3(FG_THREADS), 0, q, p);
  } else {
    cdseg_route_rec(CDSEG_RK_FG_BWD_SCALAR, 0, c, blocks, 0, 0, CDSEG_F32 << CDSEG_ROUTE_F_CT_SHIFT, 0);
    hipLaunchKernelGGL(fg_bwd_scalar_kernel, dim3((unsigned)blocks), dim3(FG_THREADS), 0, q, p);
  }
  CDSEG_CHECK_LAUNCH();
  colsum::launch_reduce<1>(p.ws, blocks, 2 * c, sums, -1.0, q);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

}  // extern "C"
