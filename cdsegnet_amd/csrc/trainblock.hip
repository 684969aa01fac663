// Native executor for one PTv3 Block of the TRAINING step (ref: ptv3.py:399-428 under autograd, engines/train.py:216-271):
// forward with a tape and backward, each ONE host call that issues every launch of the Block on the caller's stream - the
// counterpart of csrc/runtime.hip for cdsegnet_amd/train_graph.py, whose autograd graph pays ~20 Python nodes per Block and
// leaves the residual adds, the stochastic-depth masks, the GELU, the timestep rows, the gradient zero fills, the weight
// transposes and the 16-bit round trips to torch device ops.
//
// The products are the library's own entry points, called as the autograd graph calls them (cdseg_gemm dense and gathered,
// cdseg_layernorm / _bwd[_det], cdseg_attention / _bwd, cdseg_linear_wgrad[16][_det], cdseg_conv_wgrad[16][_det]).  New
// here: the row kernels for what torch did (residual, scale_cast, add_layernorm, gelu_fwd, gelu_bwd_cast, the per-scene column
// sums of dt_rows), the derive kernel of cdseg_train_block_prepare, and the four kernels of the row level (a Mix3D batch trained on
// every point: io->n_conv, row_vox, row_start - gather_first, residual_rows, run_sum, scatter_first).  All of them: 16-byte loads
// and stores, wave64, grid-stride loops, no LDS, no float atomics, no scratch.
#include <cstring>

#include "common.h"
#include "route.h"
#include "workspace.h"

namespace {

inline bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

constexpr int ROW_BLOCK = 256;
constexpr long ROW_MAX_BLOCKS = 4096;

inline unsigned row_grid(long items) {
  long b = (items + ROW_BLOCK - 1) / ROW_BLOCK;
  if (b < 1) b = 1;
  return (unsigned)(b > ROW_MAX_BLOCKS ? ROW_MAX_BLOCKS : b);
}

// 16-bit stores of four values (8 bytes per chunk; two chunks share a 16-byte line of the row)
__device__ __forceinline__ void store4_sat(bf16_t* p, float4 v) {
  uint2 u;
  u.x = pack_bf16x2(v.x, v.y);
  u.y = pack_bf16x2(v.z, v.w);
  *reinterpret_cast<uint2*>(p) = u;
}
// without saturation: beyond the 16-bit type's range the value becomes inf (torch's `.to`), which a GradScaler has to see
__device__ __forceinline__ void store4_nosat(bf16_t* p, float4 v) {
  uint2 u;
  u.x = pack_bf16x2_inrange(v.x, v.y);
  u.y = pack_bf16x2_inrange(v.z, v.w);
  *reinterpret_cast<uint2*>(p) = u;
}

__device__ __forceinline__ int scene_of(const int32_t* __restrict__ offs, int nb, long row) {
  int lo = 0, hi = nb - 1;  // offs[lo] <= row < offs[hi + 1]
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((long)offs[mid] <= row) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// ---------------------------------------------------------------- residual: out = x + mask[row] * a + t_rows[scene(row)]
// (out may be x: every element is read and written by the same thread)
__global__ void residual_kernel(const float* x, const float* a, const float* __restrict__ mask,
                                const float* __restrict__ t_rows, const int32_t* __restrict__ offs, int nb, float* out, long n,
                                int c) {
#pragma clang fp contract(off)
  const int nchunk = c >> 2;
  const long total = n * nchunk;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const long row = t / nchunk;
    const int ch = (int)(t - row * nchunk);
    float4 v = *reinterpret_cast<const float4*>(x + 4 * t);
    if (a) {
      float4 p = *reinterpret_cast<const float4*>(a + 4 * t);
      if (mask) {
        const float m = mask[row];
        p.x = p.x * m; p.y = p.y * m; p.z = p.z * m; p.w = p.w * m;
      }
      v.x = v.x + p.x; v.y = v.y + p.y; v.z = v.z + p.z; v.w = v.w + p.w;
    }
    if (t_rows) {
      const float4 r = *reinterpret_cast<const float4*>(t_rows + (long)scene_of(offs, nb, row) * c + 4 * ch);
      v.x = v.x + r.x; v.y = v.y + r.y; v.z = v.z + r.z; v.w = v.w + r.w;
    }
    *reinterpret_cast<float4*>(out + 4 * t) = v;
  }
}

// ---------------------------------------------------------------- the row level above the voxels (Mix3D, every point a row)
// n rows in voxel order, the rows of a voxel contiguous: row_vox (n) is the voxel of a row, row_start (nv + 1) the first row of
// every voxel's run.  Rows of c floats, c a multiple of 4; one thread per 16-byte chunk, consecutive lanes on consecutive
// chunks, so a wave covers 256 / c voxels (or rows) and a run's rows are walked by the lanes of its columns.

// gather_first: out[v] = cast(x[row_start[v]])  (16-bit: saturating, the forward's operand cast)
template <bool LP>
__global__ void gather_first_kernel(const float* __restrict__ x, const int32_t* __restrict__ row_start, void* __restrict__ out,
                                    long nv, int c) {
  const int nchunk = c >> 2;
  const long total = nv * nchunk;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const long v = t / nchunk;
    const int ch = (int)(t - v * nchunk);
    const float4 val = *reinterpret_cast<const float4*>(x + (long)row_start[v] * c + 4 * ch);
    if (LP) store4_sat((bf16_t*)out + 4 * t, val);
    else *reinterpret_cast<float4*>((float*)out + 4 * t) = val;
  }
}

// residual_rows: out[i] = x[i] + a[row_vox[i]] + t_rows[scene(i)]  (a: one row per voxel; out may be x)
__global__ void residual_rows_kernel(const float* x, const float* __restrict__ a, const int32_t* __restrict__ row_vox,
                                     const float* __restrict__ t_rows, const int32_t* __restrict__ offs, int nb, float* out, long n,
                                     int c) {
#pragma clang fp contract(off)
  const int nchunk = c >> 2;
  const long total = n * nchunk;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const long row = t / nchunk;
    const int ch = (int)(t - row * nchunk);
    float4 v = *reinterpret_cast<const float4*>(x + 4 * t);
    const float4 p = *reinterpret_cast<const float4*>(a + (long)row_vox[row] * c + 4 * ch);
    v.x = v.x + p.x; v.y = v.y + p.y; v.z = v.z + p.z; v.w = v.w + p.w;
    if (t_rows) {
      const float4 r = *reinterpret_cast<const float4*>(t_rows + (long)scene_of(offs, nb, row) * c + 4 * ch);
      v.x = v.x + r.x; v.y = v.y + r.y; v.z = v.z + r.z; v.w = v.w + r.w;
    }
    *reinterpret_cast<float4*>(out + 4 * t) = v;
  }
}

// run_sum: out[v] = 0 + dx[row_start[v]] + ... + dx[row_start[v + 1] - 1], in ascending row order
__global__ void run_sum_kernel(const float* __restrict__ dx, const int32_t* __restrict__ row_start, float* __restrict__ out, long nv,
                               int c) {
#pragma clang fp contract(off)
  const int nchunk = c >> 2;
  const long total = nv * nchunk;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const long v = t / nchunk;
    const int ch = (int)(t - v * nchunk);
    const long r0 = row_start[v], r1 = row_start[v + 1];
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long r = r0; r < r1; ++r) {
      const float4 d = *reinterpret_cast<const float4*>(dx + r * c + 4 * ch);
      s.x = s.x + d.x; s.y = s.y + d.y; s.z = s.z + d.z; s.w = s.w + d.w;
    }
    *reinterpret_cast<float4*>(out + 4 * t) = s;
  }
}

// scatter_first: the conv's data gradient g (one row per voxel) belongs to the FIRST row of the voxel's run.
// ACC: dx[i] += g[row_vox[i]] on first rows, the other rows untouched; else dx[i] = g[row_vox[i]] or 0 (every row written)
template <bool ACC>
__global__ void scatter_first_kernel(const float* __restrict__ g, const int32_t* __restrict__ row_vox,
                                     const int32_t* __restrict__ row_start, float* dx, long n, int c) {
#pragma clang fp contract(off)
  const int nchunk = c >> 2;
  const long total = n * nchunk;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const long row = t / nchunk;
    const int ch = (int)(t - row * nchunk);
    const long v = row_vox[row];
    const bool first = (long)row_start[v] == row;
    if (ACC) {
      if (first) {
        float4 d = *reinterpret_cast<const float4*>(dx + 4 * t);
        const float4 p = *reinterpret_cast<const float4*>(g + v * c + 4 * ch);
        d.x = d.x + p.x; d.y = d.y + p.y; d.z = d.z + p.z; d.w = d.w + p.w;
        *reinterpret_cast<float4*>(dx + 4 * t) = d;
      }
    } else {
      float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
      if (first) p = *reinterpret_cast<const float4*>(g + v * c + 4 * ch);
      *reinterpret_cast<float4*>(dx + 4 * t) = p;
    }
  }
}

// ---------------------------------------------------------------- scale_cast: out = cast_nosat(mask[row] * dy)
template <bool LP>
__global__ void scale_cast_kernel(const float* __restrict__ dy, const float* __restrict__ mask, void* __restrict__ out, long n,
                                  int c) {
  const int nchunk = c >> 2;
  const long total = n * nchunk;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    float4 v = *reinterpret_cast<const float4*>(dy + 4 * t);
    if (mask) {
      const float m = mask[t / nchunk];
      v.x = v.x * m; v.y = v.y * m; v.z = v.z * m; v.w = v.w * m;
    }
    if (LP) store4_nosat((bf16_t*)out + 4 * t, v);
    else *reinterpret_cast<float4*>((float*)out + 4 * t) = v;
  }
}

// ---------------------------------------------------------------- GELU (erf form, torch.nn.GELU()), forward and backward
// libm's erff / expf: these results are compared with torch's fp32 op against fp64 (the A&S erf of common.h is for results
// that are rounded to 16 bits next)
__device__ __forceinline__ float gelu_exact(float u) { return 0.5f * u * (1.0f + erff(u * 0.70710678118654752440f)); }
__device__ __forceinline__ float gelu_grad(float u) {
  const float cdf = 0.5f * (1.0f + erff(u * 0.70710678118654752440f));
  const float pdf = 0.39894228040143267794f * expf(-0.5f * u * u);
  return cdf + u * pdf;
}

template <bool LP>
__global__ void gelu_fwd_kernel(const float* __restrict__ u, void* __restrict__ g, long nchunks) {
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < nchunks; t += (long)gridDim.x * blockDim.x) {
    float4 v = *reinterpret_cast<const float4*>(u + 4 * t);
    v.x = gelu_exact(v.x); v.y = gelu_exact(v.y); v.z = gelu_exact(v.z); v.w = gelu_exact(v.w);
    if (LP) store4_sat((bf16_t*)g + 4 * t, v);
    else *reinterpret_cast<float4*>((float*)g + 4 * t) = v;
  }
}

template <bool LP>
__global__ void gelu_bwd_cast_kernel(const float* __restrict__ u, const float* __restrict__ dg, void* __restrict__ du, long nchunks) {
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < nchunks; t += (long)gridDim.x * blockDim.x) {
    const float4 v = *reinterpret_cast<const float4*>(u + 4 * t);
    float4 d = *reinterpret_cast<const float4*>(dg + 4 * t);
    d.x = d.x * gelu_grad(v.x); d.y = d.y * gelu_grad(v.y); d.z = d.z * gelu_grad(v.z); d.w = d.w * gelu_grad(v.w);
    if (LP) store4_nosat((bf16_t*)du + 4 * t, d);
    else *reinterpret_cast<float4*>((float*)du + 4 * t) = d;
  }
}

// ---------------------------------------------------------------- add_layernorm: x1 = x + mask[row] * a;  h = LN(x1)
// The row layout and the arithmetic of the LayerNorm are those of layernorm_kernel (csrc/elementwise.hip): TPR lanes share a
// row, each keeps its <= MAXV float4 chunks in registers, two-pass statistics.  Grid-stride over row groups.
template <int MAXV, bool LP>
__global__ void add_layernorm_kernel(const float* __restrict__ x, const float* __restrict__ a, const float* __restrict__ mask,
                                     const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                     float* __restrict__ x1, void* __restrict__ h, long n, int c, int tpr) {
  const int lane = threadIdx.x & 63;
  const int rpw = 64 / tpr;
  const int sub = lane % tpr;
  const int nchunk = c >> 2;
  const long waves = ((long)gridDim.x * blockDim.x) >> 6;
  const long groups = (n + rpw - 1) / rpw;
  for (long wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6; wave < groups; wave += waves) {
    const long row = wave * rpw + lane / tpr;
    const bool active = row < n;
    const float m = (active && mask) ? mask[row] : 1.0f;
    float4 v[MAXV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      const int ch = sub + i * tpr;
      if (active && ch < nchunk) {
        const float4 xv = *reinterpret_cast<const float4*>(x + row * c + 4 * ch);
        float4 p = *reinterpret_cast<const float4*>(a + row * c + 4 * ch);
        {
#pragma clang fp contract(off)
          if (mask) { p.x = p.x * m; p.y = p.y * m; p.z = p.z * m; p.w = p.w * m; }
          v[i].x = xv.x + p.x; v[i].y = xv.y + p.y; v[i].z = xv.z + p.z; v[i].w = xv.w + p.w;
        }
        *reinterpret_cast<float4*>(x1 + row * c + 4 * ch) = v[i];
        s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
      } else {
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    for (int o = tpr >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float mean = s / (float)c;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      const int ch = sub + i * tpr;
      if (ch < nchunk) {
        const float d0 = v[i].x - mean, d1 = v[i].y - mean, d2 = v[i].z - mean, d3 = v[i].w - mean;
        q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
      }
    }
    for (int o = tpr >> 1; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
    const float rstd = 1.0f / sqrtf(q / (float)c + eps);
    if (!active) continue;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      const int ch = sub + i * tpr;
      if (ch < nchunk) {
        const float4 g = *reinterpret_cast<const float4*>(gamma + 4 * ch);
        const float4 b = *reinterpret_cast<const float4*>(beta + 4 * ch);
        float4 y;
        y.x = (v[i].x - mean) * rstd * g.x + b.x;
        y.y = (v[i].y - mean) * rstd * g.y + b.y;
        y.z = (v[i].z - mean) * rstd * g.z + b.z;
        y.w = (v[i].w - mean) * rstd * g.w + b.w;
        if (LP) store4_sat((bf16_t*)h + row * c + 4 * ch, y);
        else *reinterpret_cast<float4*>((float*)h + row * c + 4 * ch) = y;
      }
    }
  }
}

// ---------------------------------------------------------------- scene sums: dt_rows[b] = sum of the rows of scene b
// The gradient of the per-scene timestep rows: one column sum over up to n rows per scene.  (cdseg_segment_sum walks a run
// with one thread per column - right for the <= 8 children of a pooled row, ~3.5 ms per Block on a 120 k-row scene.)  Two
// launches without atomics, in an order fixed by (n, num_scenes): rows are cut into chunks of R; thread (chunk, scene,
// 4 columns) adds the rows of its chunk that belong to its scene (four interleaved partial sums, added pairwise); then thread
// (scene, 4 columns) adds the chunk partials by ascending chunk index.
__global__ void scene_sum_partial_kernel(const float* __restrict__ dx, const int32_t* __restrict__ offs, int nb, long n, int c,
                                         int R, long chunks, float* __restrict__ partial) {
  const int nchunk = c >> 2;
  const long total = chunks * nb * nchunk;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const int cq = (int)(t % nchunk);
    const long kb = t / nchunk;
    const int b = (int)(kb % nb);
    const long k = kb / nb;
    long lo = k * R, hi = lo + R;
    if (hi > n) hi = n;
    if (lo < (long)offs[b]) lo = offs[b];
    if (hi > (long)offs[b + 1]) hi = offs[b + 1];
    float4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    long r = lo;
    for (; r + 4 <= hi; r += 4) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 v = *reinterpret_cast<const float4*>(dx + (r + j) * c + 4 * cq);
        acc[j].x += v.x; acc[j].y += v.y; acc[j].z += v.z; acc[j].w += v.w;
      }
    }
    for (int j = 0; r < hi; ++r, ++j) {
      const float4 v = *reinterpret_cast<const float4*>(dx + r * c + 4 * cq);
      if (j == 0) { acc[0].x += v.x; acc[0].y += v.y; acc[0].z += v.z; acc[0].w += v.w; }
      else if (j == 1) { acc[1].x += v.x; acc[1].y += v.y; acc[1].z += v.z; acc[1].w += v.w; }
      else { acc[2].x += v.x; acc[2].y += v.y; acc[2].z += v.z; acc[2].w += v.w; }
    }
    float4 o;
    o.x = (acc[0].x + acc[1].x) + (acc[2].x + acc[3].x);
    o.y = (acc[0].y + acc[1].y) + (acc[2].y + acc[3].y);
    o.z = (acc[0].z + acc[1].z) + (acc[2].z + acc[3].z);
    o.w = (acc[0].w + acc[1].w) + (acc[2].w + acc[3].w);
    *reinterpret_cast<float4*>(partial + (k * nb + b) * c + 4 * cq) = o;
  }
}

__global__ void scene_sum_final_kernel(const float* __restrict__ partial, int nb, int c, long chunks, float* __restrict__ out) {
  const int nchunk = c >> 2;
  const long total = (long)nb * nchunk;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const int cq = (int)(t % nchunk);
    const long b = t / nchunk;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long k = 0; k < chunks; ++k) {
      const float4 v = *reinterpret_cast<const float4*>(partial + (k * nb + b) * c + 4 * cq);
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    *reinterpret_cast<float4*>(out + b * c + 4 * cq) = acc;
  }
}

// ---------------------------------------------------------------- derive: every derived weight of a Block in one launch
// Segment s writes `count` output elements at dst: kind 0 = copy / cast of src (rows x cols), 1 = transpose (dst (cols, rows)),
// 2 = the conv's data-gradient kernel dst[ci][o][co] = src[co][26 - o][ci] (rows = cout, cols = cin).  A thread owns 16 bytes
// of output (4 fp32 / 8 16-bit values); segment sizes are multiples of that.
constexpr int DERIVE_MAX_SEG = 13;
struct DeriveP {
  const void* src[DERIVE_MAX_SEG];
  void* dst[DERIVE_MAX_SEG];
  long first_group[DERIVE_MAX_SEG + 1];  // prefix sums of the 16-byte output groups
  int rows[DERIVE_MAX_SEG], cols[DERIVE_MAX_SEG];
  unsigned char kind[DERIVE_MAX_SEG], src_lp[DERIVE_MAX_SEG], dst_lp[DERIVE_MAX_SEG];
  int nseg;
};

__device__ __forceinline__ float derive_load(const void* src, bool lp, long i) {
  return lp ? bf16_to_f32(((const bf16_t*)src)[i]) : ((const float*)src)[i];
}

__device__ __forceinline__ long derive_src_index(int kind, int rows, int cols, long o) {
  if (kind == 0) return o;
  if (kind == 1) {  // dst (cols, rows)
    const long r = o / rows;
    return (o - r * rows) * cols + r;
  }
  // dst (cin = cols, 27, cout = rows)
  const long ci = o / (27L * rows);
  const long rem = o - ci * 27L * rows;
  const long off = rem / rows, co = rem - off * rows;
  return (co * 27 + (26 - off)) * cols + ci;
}

__global__ void derive_kernel(DeriveP p) {
  const long total = p.first_group[p.nseg];
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    int s = 0;
    while (s + 1 < p.nseg && t >= p.first_group[s + 1]) ++s;
    const long gidx = t - p.first_group[s];
    const int rows = p.rows[s], cols = p.cols[s], kind = p.kind[s];
    const bool slp = p.src_lp[s] != 0;
    if (p.dst_lp[s]) {
      const long o = gidx * 8;
      float f[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = derive_load(p.src[s], slp, derive_src_index(kind, rows, cols, o + j));
      uint4 u;  // fp32 source: the library's cast (saturating in the half build), as ops.cast of the weight; a 16-bit source
      if (slp) {  // passes unchanged (every value is representable: no clamp, an inf stays what it is)
        u.x = pack_bf16x2_inrange(f[0], f[1]); u.y = pack_bf16x2_inrange(f[2], f[3]);
        u.z = pack_bf16x2_inrange(f[4], f[5]); u.w = pack_bf16x2_inrange(f[6], f[7]);
      } else {
        u.x = pack_bf16x2(f[0], f[1]); u.y = pack_bf16x2(f[2], f[3]); u.z = pack_bf16x2(f[4], f[5]); u.w = pack_bf16x2(f[6], f[7]);
      }
      *reinterpret_cast<uint4*>((bf16_t*)p.dst[s] + o) = u;
    } else {
      const long o = gidx * 4;
      float4 v;
      v.x = derive_load(p.src[s], slp, derive_src_index(kind, rows, cols, o));
      v.y = derive_load(p.src[s], slp, derive_src_index(kind, rows, cols, o + 1));
      v.z = derive_load(p.src[s], slp, derive_src_index(kind, rows, cols, o + 2));
      v.w = derive_load(p.src[s], slp, derive_src_index(kind, rows, cols, o + 3));
      *reinterpret_cast<float4*>((float*)p.dst[s] + o) = v;
    }
  }
}

// ---------------------------------------------------------------- layouts (host, functions of the shape only; workspace.h)
// the six matrices: (out, in) with in = 27 * C for the conv
enum { M_CONV = 0, M_CPE, M_QKV, M_PROJ, M_FC1, M_FC2, M_COUNT };
const int MAT_PARAM[M_COUNT] = {CDSEG_TB_CONV_W, CDSEG_TB_CPE_W, CDSEG_TB_QKV_W, CDSEG_TB_PROJ_W, CDSEG_TB_FC1_W, CDSEG_TB_FC2_W};

inline void mat_shape(const cdseg_train_block_desc* d, int m, long* out, long* in) {
  const long C = d->channels, H = d->hidden;
  switch (m) {
    case M_CONV: *out = C; *in = C; break;  // per offset; 27 offsets
    case M_CPE: *out = C; *in = C; break;
    case M_QKV: *out = 3 * C; *in = C; break;
    case M_PROJ: *out = C; *in = C; break;
    case M_FC1: *out = H; *in = C; break;
    default: *out = C; *in = H; break;
  }
}

struct Derived {
  void* t[M_COUNT];    // transposed (conv: mirrored, transposed) in mm_dtype
  void* w16[M_COUNT];  // 16-bit forward weights (mm_dtype 16-bit only)
  size_t total;
};

Derived carve_derived(const cdseg_train_block_desc* d, void* base) {
  Carver c{(char*)base, 0};
  Derived D;
  const size_t e = esz(d->mm_dtype);
  for (int m = 0; m < M_COUNT; ++m) {
    long o, i;
    mat_shape(d, m, &o, &i);
    const size_t elems = (size_t)o * i * (m == M_CONV ? 27 : 1);
    D.t[m] = c.take(elems * e);
    D.w16[m] = d->mm_dtype == CDSEG_BF16 ? c.take(elems * 2) : nullptr;
  }
  D.total = align_up(c.off, 256);
  return D;
}

struct Tape {
  void *xc16, *yc, *z, *x0, *h1, *qkv, *o, *x1, *h2, *u, *g;
  size_t total;
};

// what the autograd graph saves, and where a 16-bit copy is the operand only that copy
Tape carve_tape(const cdseg_train_block_desc* d, long n, void* base) {
  Carver c{(char*)base, 0};
  Tape T;
  const size_t C = d->channels, H = d->hidden, N = (size_t)n;
  const size_t em = esz(d->mm_dtype), ea = esz(d->attn_dtype);
  T.xc16 = d->mm_dtype == CDSEG_BF16 ? c.take(N * C * 2) : nullptr;  // fp32: x_conv itself (an input of the node)
  T.yc = c.take(N * C * em);
  T.z = c.take(N * C * 4);
  T.x0 = c.take(N * C * 4);
  T.h1 = c.take(N * C * em);
  T.qkv = c.take(N * 3 * C * ea);
  T.o = c.take(N * C * em);  // proj's operand (mm type); with fp32 products on a 16-bit core: the widened output
  T.x1 = c.take(N * C * 4);
  T.h2 = c.take(N * C * em);
  T.u = c.take(N * H * 4);
  T.g = c.take(N * H * em);
  T.total = align_up(c.off, 256);
  return T;
}

struct Scratch {
  void *ws, *f0, *f1, *h0, *aux;
  size_t ws_bytes, aux_bytes, total;
};

Scratch carve_scratch(const cdseg_train_block_desc* d, long n, long slots, void* base) {
  Carver c{(char*)base, 0};
  Scratch S;
  const long C = d->channels, H = d->hidden;
  const long wide = 3 * C > H ? 3 * C : H;
  S.ws_bytes = 0;
  const long widths[3] = {C, 3 * C, H};
  for (long w : widths) {
    const size_t b = gemm_ws_rule(n, w, w, w == C, false);  // (N = C: the sparse conv, gathered; no GEMM here fuses a LayerNorm)
    if (b > S.ws_bytes) S.ws_bytes = b;
  }
  S.ws = S.ws_bytes ? c.take(S.ws_bytes) : nullptr;
  S.f0 = c.take((size_t)n * wide * 4);
  S.f1 = c.take((size_t)n * wide * 4);
  S.h0 = c.take((size_t)n * wide * 2);
  S.aux_bytes = cdseg_attention_bwd_ws_bytes(slots > 0 ? slots : 0, d->heads);
  if (d->deterministic) {
    const int dt = d->mm_dtype;
    for (int m = 0; m < M_COUNT; ++m) {
      long o, i;
      mat_shape(d, m, &o, &i);
      const size_t b = cdseg_wgrad_det_ws_bytes(n, (int)o, (int)i, m == M_CONV ? 27 : 1, dt);
      if (b > S.aux_bytes) S.aux_bytes = b;
    }
    const size_t b = cdseg_layernorm_bwd_det_ws_bytes(n, (int)C);
    if (b > S.aux_bytes) S.aux_bytes = b;
  }
  if (S.aux_bytes < 256) S.aux_bytes = 256;
  S.aux = c.take(S.aux_bytes);
  S.total = align_up(c.off, 256);
  return S;
}

struct Grads {
  size_t off[CDSEG_TB_PARAMS], total;
};

inline size_t param_elems(const cdseg_train_block_desc* d, int p) {
  const size_t C = d->channels, H = d->hidden;
  switch (p) {
    case CDSEG_TB_CONV_W: return C * 27 * C;
    case CDSEG_TB_CPE_W: case CDSEG_TB_PROJ_W: return C * C;
    case CDSEG_TB_QKV_W: return 3 * C * C;
    case CDSEG_TB_QKV_B: return 3 * C;
    case CDSEG_TB_FC1_W: case CDSEG_TB_FC2_W: return H * C;
    case CDSEG_TB_FC1_B: return H;
    default: return C;
  }
}

Grads carve_grads(const cdseg_train_block_desc* d) {
  Grads G;
  size_t off = 0;
  for (int p = 0; p < CDSEG_TB_PARAMS; ++p) {
    G.off[p] = off;
    off = align_up(off + param_elems(d, p) * 4, 256);
  }
  G.total = off;
  return G;
}

bool desc_ok(const cdseg_train_block_desc* d) {
  if (!d) return false;
  if (d->channels <= 0 || (d->channels & 15) || d->hidden <= 0 || (d->hidden & 15)) return false;
  if (d->heads <= 0 || d->channels != d->heads * CDSEG_HEAD_DIM) return false;
  if ((d->mm_dtype != CDSEG_F32 && d->mm_dtype != CDSEG_BF16) || (d->attn_dtype != CDSEG_F32 && d->attn_dtype != CDSEG_BF16))
    return false;
  return true;
}

bool desc_ptrs_ok(const cdseg_train_block_desc* d) {
  for (int p = 0; p < CDSEG_TB_PARAMS; ++p)
    if (!d->param[p] || !al16(d->param[p])) return false;
  for (int m = 0; m < M_COUNT; ++m)
    if (d->shadow16[m] && !al16(d->shadow16[m])) return false;
  if (!d->derived || !al16(d->derived) || d->derived_bytes < carve_derived(d, nullptr).total) return false;
  return true;
}

bool io_ok(const cdseg_train_block_desc* d, const cdseg_train_block_io* io, bool forward) {
  if (!io || !io->x_in || !io->x_conv || !io->nbr || !io->gidx || !io->widx || !io->patch_start || !io->tape || !io->scratch ||
      (forward && !io->x_out))  // (the backward does not read x_out)
    return false;
  if (io->max_len <= 0 || io->max_len > CDSEG_MAX_PATCH || io->num_patches <= 0 || io->num_slots <= 0) return false;
  if (io->t_rows && (!io->scene_offs || io->num_scenes <= 0)) return false;
  if (!al16(io->x_in) || !al16(io->x_conv) || !al16(io->x_out) || !al16(io->tape) || !al16(io->scratch) || !al16(io->t_rows))
    return false;
  if ((((uintptr_t)io->mask1 | (uintptr_t)io->mask2 | (uintptr_t)io->nbr | (uintptr_t)io->gidx | (uintptr_t)io->widx |
        (uintptr_t)io->patch_start | (uintptr_t)io->scene_offs) & 3) != 0)
    return false;
  // the row level (Mix3D): all three or none; the tape and the scratch are sized by n >= n_conv and gain nothing
  if (io->n_conv == 0 ? (io->row_vox || io->row_start) : (io->n_conv < 1 || io->n_conv > io->n || !io->row_vox || !io->row_start))
    return false;
  if ((((uintptr_t)io->row_vox | (uintptr_t)io->row_start) & 3) != 0) return false;
  if (io->tape_bytes < carve_tape(d, io->n, nullptr).total) return false;
  if (io->scratch_bytes < carve_scratch(d, io->n, io->num_slots, nullptr).total) return false;
  return true;
}

// the forward weight of matrix m in mm_dtype
inline const void* fwd_weight(const cdseg_train_block_desc* d, const Derived& D, int m) {
  if (d->mm_dtype != CDSEG_BF16) return d->param[MAT_PARAM[m]];
  return d->shadow16[m] ? d->shadow16[m] : D.w16[m];
}

// out (n, N) = A (n, K) W^T + bias through cdseg_gemm, as ops.gemm sets it up
int gemm(const cdseg_train_block_desc* d, const Scratch& S, long n, const void* A, const void* W, const float* bias, int N, int K,
         void* out, int out_dtype, const int32_t* nbr, void* stream) {
  cdseg_gemm_args a;
  std::memset(&a, 0, sizeof(a));
  a.A = A; a.W = W; a.bias = bias; a.out = out;
  a.M = n; a.N = N; a.K = K; a.kvol = nbr ? 27 : 1;
  a.lda = K; a.ldo = N;
  a.a_dtype = a.compute_dtype = d->mm_dtype;
  a.out_dtype = out_dtype;
  a.nbr = nbr; a.nbr_kmajor = nbr ? 1 : 0;
  a.ln_eps = 1e-5f;
  const size_t want = gemm_ws_rule(n, N, N, nbr != nullptr, false);
  if (want && S.ws) { a.ws = S.ws; a.ws_bytes = S.ws_bytes; }
  return cdseg_gemm(&a, stream);
}

int ln_fwd(const float* x, const float* g, const float* b, float eps, const float* res, void* out, int out_dtype, long n, int c,
           void* stream) {
  return cdseg_layernorm(x, CDSEG_F32, c, g, b, eps, res, c, nullptr, out, out_dtype, c, nullptr, 0, 0, n, c, stream);
}

int ln_bwd(const cdseg_train_block_desc* d, const Scratch& S, const float* x, const float* g, float eps, const float* dy, float* dx,
           int accumulate, float* dg, float* db, long n, void* stream) {
  const int c = d->channels;
  if (d->deterministic)
    return cdseg_layernorm_bwd_det(x, c, g, eps, dy, c, dx, c, accumulate, dg, db, n, c, S.aux, S.aux_bytes, stream);
  return cdseg_layernorm_bwd(x, c, g, eps, dy, c, dx, c, accumulate, dg, db, n, c, stream);
}

// dw (N, K) += dy^T x, db += column sums; x and dy in mm_dtype
int lin_wgrad(const cdseg_train_block_desc* d, const Scratch& S, const void* x, const void* dy, long n, int K, int N, float* dw,
              float* db, void* stream) {
  if (d->deterministic)
    return cdseg_linear_wgrad_det(x, K, nullptr, dy, N, n, K, N, dw, K, db, d->mm_dtype, S.aux, S.aux_bytes, stream);
  if (d->mm_dtype == CDSEG_BF16) return cdseg_linear_wgrad16(x, K, nullptr, dy, N, n, K, N, dw, K, db, stream);
  return cdseg_linear_wgrad((const float*)x, K, nullptr, (const float*)dy, N, n, K, N, dw, K, db, stream);
}

// chunk length of the scene sums: about sqrt(n) rows (both launches then walk about sqrt(n) values per thread), at least 64
// and at least num_scenes, so that the (chunks, num_scenes, c) partials fit a scratch buffer of 3 n c floats
inline int scene_sum_rows(long n, int nb) {
  long r = 64;
  while (r * r < n) r += 32;
  return (int)(r > nb ? r : nb);
}

int scene_sums(const float* dx, const int32_t* offs, int nb, long n, int c, float* partial, size_t partial_bytes, float* out,
               void* stream) {
  const int R = scene_sum_rows(n, nb);
  const long chunks = (n + R - 1) / R;
  if ((size_t)chunks * nb * c * sizeof(float) > partial_bytes) return CDSEG_ERR_ARG;
  hipLaunchKernelGGL(scene_sum_partial_kernel, dim3(row_grid(chunks * nb * (c >> 2))), dim3(ROW_BLOCK), 0, (hipStream_t)stream, dx, offs,
                     nb, n, c, R, chunks, partial);
  hipLaunchKernelGGL(scene_sum_final_kernel, dim3(row_grid((long)nb * (c >> 2))), dim3(ROW_BLOCK), 0, (hipStream_t)stream, partial, nb, c,
                     chunks, out);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cast_nosat(const float* src, void* dst, long n, int c, void* stream) {
  return cdseg_scale_cast(src, nullptr, dst, CDSEG_BF16, n, c, stream);
}

}  // namespace

#define TB_TRY(expr)                          \
  do {                                        \
    const int rc__ = (expr);                  \
    if (rc__ != CDSEG_OK) return rc__;        \
  } while (0)

// ================================================================ row kernels on their own
extern "C" int cdseg_residual(const float* x, const float* a, const float* mask, const float* t_rows, const int32_t* scene_offs,
                              int num_scenes, float* out, long n, int c, void* stream) {
  if (n <= 0) return CDSEG_OK;
  if (!x || !out || c <= 0 || (c & 3) || !al16(x) || !al16(a) || !al16(out) || !al16(t_rows)) return CDSEG_ERR_ARG;
  if ((mask && !a) || (t_rows && (!scene_offs || num_scenes <= 0))) return CDSEG_ERR_ARG;
  hipLaunchKernelGGL(residual_kernel, dim3(row_grid(n * (c >> 2))), dim3(ROW_BLOCK), 0, (hipStream_t)stream, x, a, mask, t_rows,
                     scene_offs, num_scenes, out, n, c);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

extern "C" int cdseg_gather_first(const float* x, const int32_t* row_start, void* out, int out_dtype, long nv, int c, void* stream) {
  if (nv <= 0) return CDSEG_OK;
  if (!x || !row_start || !out || c <= 0 || (c & 3) || !al16(x) || !al16(out) || ((uintptr_t)row_start & 3)) return CDSEG_ERR_ARG;
  if (out_dtype != CDSEG_F32 && out_dtype != CDSEG_BF16) return CDSEG_ERR_ARG;
  const dim3 grid(row_grid(nv * (c >> 2))), block(ROW_BLOCK);
  if (out_dtype == CDSEG_BF16) {
    cdseg_route_rec(CDSEG_RK_GATHER_FIRST_B16, 0, c, 1, 0, 0, CDSEG_BF16 << CDSEG_ROUTE_F_CT_SHIFT, 0);
    hipLaunchKernelGGL(gather_first_kernel<true>, grid, block, 0, (hipStream_t)stream, x, row_start, out, nv, c);
  } else {
    cdseg_route_rec(CDSEG_RK_GATHER_FIRST_F32, 0, c, 1, 0, 0, CDSEG_F32 << CDSEG_ROUTE_F_CT_SHIFT, 0);
    hipLaunchKernelGGL(gather_first_kernel<false>, grid, block, 0, (hipStream_t)stream, x, row_start, out, nv, c);
  }
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

extern "C" int cdseg_residual_rows(const float* x, const float* a, const int32_t* row_vox, const float* t_rows,
                                   const int32_t* scene_offs, int num_scenes, float* out, long n, int c, void* stream) {
  if (n <= 0) return CDSEG_OK;
  if (!x || !a || !row_vox || !out || c <= 0 || (c & 3) || !al16(x) || !al16(a) || !al16(out) || !al16(t_rows) ||
      ((uintptr_t)row_vox & 3))
    return CDSEG_ERR_ARG;
  if (t_rows && (!scene_offs || num_scenes <= 0)) return CDSEG_ERR_ARG;
  hipLaunchKernelGGL(residual_rows_kernel, dim3(row_grid(n * (c >> 2))), dim3(ROW_BLOCK), 0, (hipStream_t)stream, x, a, row_vox,
                     t_rows, scene_offs, num_scenes, out, n, c);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

extern "C" int cdseg_run_sum(const float* dx, const int32_t* row_start, float* out, long nv, int c, void* stream) {
  if (nv <= 0) return CDSEG_OK;
  if (!dx || !row_start || !out || c <= 0 || (c & 3) || !al16(dx) || !al16(out) || ((uintptr_t)row_start & 3)) return CDSEG_ERR_ARG;
  hipLaunchKernelGGL(run_sum_kernel, dim3(row_grid(nv * (c >> 2))), dim3(ROW_BLOCK), 0, (hipStream_t)stream, dx, row_start, out, nv,
                     c);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

extern "C" int cdseg_scatter_first(const float* g, const int32_t* row_vox, const int32_t* row_start, float* dx, int accumulate,
                                   long n, int c, void* stream) {
  if (n <= 0) return CDSEG_OK;
  if (!g || !row_vox || !row_start || !dx || c <= 0 || (c & 3) || !al16(g) || !al16(dx) ||
      (((uintptr_t)row_vox | (uintptr_t)row_start) & 3))
    return CDSEG_ERR_ARG;
  const dim3 grid(row_grid(n * (c >> 2))), block(ROW_BLOCK);
  if (accumulate) {
    cdseg_route_rec(CDSEG_RK_SCATTER_FIRST_ACC, 0, c, 1, 0, 0, CDSEG_F32 << CDSEG_ROUTE_F_CT_SHIFT, 0);
    hipLaunchKernelGGL(scatter_first_kernel<true>, grid, block, 0, (hipStream_t)stream, g, row_vox, row_start, dx, n, c);
  } else {
    cdseg_route_rec(CDSEG_RK_SCATTER_FIRST_SET, 0, c, 1, 0, 0, CDSEG_F32 << CDSEG_ROUTE_F_CT_SHIFT, 0);
    hipLaunchKernelGGL(scatter_first_kernel<false>, grid, block, 0, (hipStream_t)stream, g, row_vox, row_start, dx, n, c);
  }
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

extern "C" int cdseg_scale_cast(const float* dy, const float* mask, void* out, int out_dtype, long n, int c, void* stream) {
  if (n <= 0) return CDSEG_OK;
  if (!dy || !out || c <= 0 || (c & 3) || !al16(dy) || !al16(out)) return CDSEG_ERR_ARG;
  if (out_dtype != CDSEG_F32 && out_dtype != CDSEG_BF16) return CDSEG_ERR_ARG;
  const dim3 grid(row_grid(n * (c >> 2))), block(ROW_BLOCK);
  if (out_dtype == CDSEG_BF16) {
    cdseg_route_rec(CDSEG_RK_SCALE_CAST_B16, 0, c, 1, 0, 0, CDSEG_BF16 << CDSEG_ROUTE_F_CT_SHIFT, 0);
    hipLaunchKernelGGL(scale_cast_kernel<true>, grid, block, 0, (hipStream_t)stream, dy, mask, out, n, c);
  } else {
    cdseg_route_rec(CDSEG_RK_SCALE_CAST_F32, 0, c, 1, 0, 0, CDSEG_F32 << CDSEG_ROUTE_F_CT_SHIFT, 0);
    hipLaunchKernelGGL(scale_cast_kernel<false>, grid, block, 0, (hipStream_t)stream, dy, mask, out, n, c);
  }
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

extern "C" int cdseg_add_layernorm(const float* x, const float* a, const float* mask, const float* gamma, const float* beta,
                                   float eps, float* x1, void* h, int out_dtype, long n, int c, void* stream) {
  if (n <= 0) return CDSEG_OK;
  if (!x || !a || !gamma || !beta || !x1 || !h || c <= 0 || (c & 3) || c > 2048) return CDSEG_ERR_ARG;
  if (!al16(x) || !al16(a) || !al16(gamma) || !al16(beta) || !al16(x1) || !al16(h)) return CDSEG_ERR_ARG;
  if (out_dtype != CDSEG_F32 && out_dtype != CDSEG_BF16) return CDSEG_ERR_ARG;
  const int nchunk = c >> 2;
  int tpr = 1;
  while (tpr < nchunk && tpr < 64) tpr <<= 1;
  const int maxv = (nchunk + tpr - 1) / tpr;
  const int rpw = 64 / tpr;
  const long groups = (n + rpw - 1) / rpw;
  const dim3 grid(row_grid(groups * 64)), block(ROW_BLOCK);
  hipStream_t s = (hipStream_t)stream;
#define ALN_LAUNCH(MV)                                                                                                        \
  do {                                                                                                                        \
    if (out_dtype == CDSEG_BF16) {                                                                                            \
      cdseg_route_rec(cdseg_route_template_id<CDSEG_RF_ADD_LN, MV, 1>(), rpw, c, 1, 0, 0, CDSEG_BF16 << CDSEG_ROUTE_F_CT_SHIFT, tpr); \
      hipLaunchKernelGGL((add_layernorm_kernel<MV, true>), grid, block, 0, s, x, a, mask, gamma, beta, eps, x1, h, n, c, tpr); \
    } else {                                                                                                                  \
      cdseg_route_rec(cdseg_route_template_id<CDSEG_RF_ADD_LN, MV, 0>(), rpw, c, 1, 0, 0, CDSEG_F32 << CDSEG_ROUTE_F_CT_SHIFT, tpr); \
      hipLaunchKernelGGL((add_layernorm_kernel<MV, false>), grid, block, 0, s, x, a, mask, gamma, beta, eps, x1, h, n, c, tpr); \
    }                                                                                                                         \
  } while (0)
  if (maxv <= 1) ALN_LAUNCH(1);
  else if (maxv <= 2) ALN_LAUNCH(2);
  else if (maxv <= 4) ALN_LAUNCH(4);
  else ALN_LAUNCH(8);
#undef ALN_LAUNCH
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

extern "C" int cdseg_gelu_fwd(const float* u, void* g, int out_dtype, long count, void* stream) {
  if (count <= 0) return CDSEG_OK;
  if (!u || !g || (count & 3) || !al16(u) || !al16(g)) return CDSEG_ERR_ARG;
  if (out_dtype != CDSEG_F32 && out_dtype != CDSEG_BF16) return CDSEG_ERR_ARG;
  const long nchunks = count >> 2;
  const dim3 grid(row_grid(nchunks)), block(ROW_BLOCK);
  if (out_dtype == CDSEG_BF16) {
    cdseg_route_rec(CDSEG_RK_GELU_FWD_B16, 0, 0, 1, 0, 0, CDSEG_BF16 << CDSEG_ROUTE_F_CT_SHIFT, 0);
    hipLaunchKernelGGL(gelu_fwd_kernel<true>, grid, block, 0, (hipStream_t)stream, u, g, nchunks);
  } else {
    cdseg_route_rec(CDSEG_RK_GELU_FWD_F32, 0, 0, 1, 0, 0, CDSEG_F32 << CDSEG_ROUTE_F_CT_SHIFT, 0);
    hipLaunchKernelGGL(gelu_fwd_kernel<false>, grid, block, 0, (hipStream_t)stream, u, g, nchunks);
  }
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

extern "C" int cdseg_gelu_bwd_cast(const float* u, const float* dg, void* du, int out_dtype, long count, void* stream) {
  if (count <= 0) return CDSEG_OK;
  if (!u || !dg || !du || (count & 3) || !al16(u) || !al16(dg) || !al16(du)) return CDSEG_ERR_ARG;
  if (out_dtype != CDSEG_F32 && out_dtype != CDSEG_BF16) return CDSEG_ERR_ARG;
  const long nchunks = count >> 2;
  const dim3 grid(row_grid(nchunks)), block(ROW_BLOCK);
  if (out_dtype == CDSEG_BF16) {
    cdseg_route_rec(CDSEG_RK_GELU_BWD_CAST_B16, 0, 0, 1, 0, 0, CDSEG_BF16 << CDSEG_ROUTE_F_CT_SHIFT, 0);
    hipLaunchKernelGGL(gelu_bwd_cast_kernel<true>, grid, block, 0, (hipStream_t)stream, u, dg, du, nchunks);
  } else {
    cdseg_route_rec(CDSEG_RK_GELU_BWD_CAST_F32, 0, 0, 1, 0, 0, CDSEG_F32 << CDSEG_ROUTE_F_CT_SHIFT, 0);
    hipLaunchKernelGGL(gelu_bwd_cast_kernel<false>, grid, block, 0, (hipStream_t)stream, u, dg, du, nchunks);
  }
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

// ================================================================ sizes
extern "C" int cdseg_train_block_bytes(const cdseg_train_block_desc* d, long n, long slots, size_t* tape, size_t* scratch,
                                       size_t* derived, size_t* grads) {
  if (!desc_ok(d) || n < 0 || slots < 0) return CDSEG_ERR_ARG;
  if (tape) *tape = carve_tape(d, n, nullptr).total;
  if (scratch) *scratch = carve_scratch(d, n, slots, nullptr).total;
  if (derived) *derived = carve_derived(d, nullptr).total;
  if (grads) *grads = carve_grads(d).total;
  return CDSEG_OK;
}

extern "C" int cdseg_train_block_grad_offsets(const cdseg_train_block_desc* d, size_t* offsets18_host) {
  if (!desc_ok(d) || !offsets18_host) return CDSEG_ERR_ARG;
  const Grads G = carve_grads(d);
  for (int p = 0; p < CDSEG_TB_PARAMS; ++p) offsets18_host[p] = G.off[p];
  return CDSEG_OK;
}

// ================================================================ prepare
extern "C" int cdseg_train_block_prepare(const cdseg_train_block_desc* d, void* stream) {
  if (!desc_ok(d) || !desc_ptrs_ok(d)) return CDSEG_ERR_ARG;
  const Derived D = carve_derived(d, d->derived);
  const bool lp = d->mm_dtype == CDSEG_BF16;
  const long per = lp ? 8 : 4;  // output elements of a 16-byte group
  DeriveP p;
  std::memset(&p, 0, sizeof(p));
  int s = 0;
  long groups = 0;
  for (int m = 0; m < M_COUNT; ++m) {
    long o, i;
    mat_shape(d, m, &o, &i);
    const long elems = o * i * (m == M_CONV ? 27 : 1);
    // the 16-bit transposes come from the copy the forward multiplies with (the optimizer's shadow when there is one)
    const void* src = (lp && d->shadow16[m]) ? d->shadow16[m] : (const void*)d->param[MAT_PARAM[m]];
    const bool src_lp = lp && d->shadow16[m];
    p.src[s] = src; p.dst[s] = D.t[m]; p.rows[s] = (int)o; p.cols[s] = (int)i; p.kind[s] = m == M_CONV ? 2 : 1;
    p.src_lp[s] = src_lp; p.dst_lp[s] = lp;
    p.first_group[s] = groups;
    groups += elems / per;
    ++s;
    if (lp && !d->shadow16[m]) {
      p.src[s] = d->param[MAT_PARAM[m]]; p.dst[s] = D.w16[m]; p.rows[s] = (int)o; p.cols[s] = (int)(i * (m == M_CONV ? 27 : 1));
      p.kind[s] = 0; p.src_lp[s] = 0; p.dst_lp[s] = 1;
      p.first_group[s] = groups;
      groups += elems / per;
      ++s;
    }
  }
  p.first_group[s] = groups;
  p.nseg = s;
  hipLaunchKernelGGL(derive_kernel, dim3(row_grid(groups)), dim3(ROW_BLOCK), 0, (hipStream_t)stream, p);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

// ================================================================ forward
extern "C" int cdseg_train_block_forward(const cdseg_train_block_desc* d, const cdseg_train_block_io* io, void* stream) {
  if (!desc_ok(d) || !io) return CDSEG_ERR_ARG;
  if (io->n <= 0) return CDSEG_OK;
  if (!desc_ptrs_ok(d) || !io_ok(d, io, true)) return CDSEG_ERR_ARG;
  const long n = io->n;
  const int C = d->channels, H = d->hidden, MM = d->mm_dtype, AT = d->attn_dtype;
  const bool lp = MM == CDSEG_BF16;
  const Derived D = carve_derived(d, d->derived);
  const Tape T = carve_tape(d, n, io->tape);
  const Scratch S = carve_scratch(d, n, io->num_slots, io->scratch);
  const float* const* P = d->param;

  // ---- CPE: x0 = x_in + LN(Linear(conv(x_conv))) [+ t_rows[scene]]
  // (row level: the whole CPE runs on the nc voxels - the conv reads the first row of every voxel - and row i adds
  // LN(z)[row_vox[i]]; the voxel rows of x_conv live in the tape's 16-bit slot or, fp32, in scratch: the backward gathers again)
  const bool rows = io->n_conv > 0;
  const long nc = rows ? io->n_conv : n;
  const void* xc = io->x_conv;
  if (rows) {
    xc = lp ? T.xc16 : S.h0;
    TB_TRY(cdseg_gather_first(io->x_conv, io->row_start, (void*)xc, MM, nc, C, stream));
  } else if (lp) {
    TB_TRY(cdseg_cast(io->x_conv, CDSEG_F32, T.xc16, CDSEG_BF16, n * C, stream));
    xc = T.xc16;
  }
  TB_TRY(gemm(d, S, nc, xc, fwd_weight(d, D, M_CONV), P[CDSEG_TB_CONV_B], C, C, T.yc, MM, io->nbr, stream));
  TB_TRY(gemm(d, S, nc, T.yc, fwd_weight(d, D, M_CPE), P[CDSEG_TB_CPE_B], C, C, T.z, CDSEG_F32, nullptr, stream));
  if (rows) {
    TB_TRY(ln_fwd((const float*)T.z, P[CDSEG_TB_CPE_LN_G], P[CDSEG_TB_CPE_LN_B], d->eps_cpe, nullptr, S.f0, CDSEG_F32, nc, C, stream));
    TB_TRY(cdseg_residual_rows(io->x_in, (const float*)S.f0, io->row_vox, io->t_rows, io->scene_offs, io->num_scenes, (float*)T.x0, n,
                               C, stream));
  } else {
    TB_TRY(ln_fwd((const float*)T.z, P[CDSEG_TB_CPE_LN_G], P[CDSEG_TB_CPE_LN_B], d->eps_cpe, io->x_in, T.x0, CDSEG_F32, n, C, stream));
    if (io->t_rows)
      TB_TRY(cdseg_residual((const float*)T.x0, nullptr, nullptr, io->t_rows, io->scene_offs, io->num_scenes, (float*)T.x0, n, C, stream));
  }

  // ---- attention branch: x1 = x0 + mask1 * proj(attention(qkv(LN1(x0))))
  TB_TRY(ln_fwd((const float*)T.x0, P[CDSEG_TB_NORM1_G], P[CDSEG_TB_NORM1_B], d->eps_norm1, nullptr, T.h1, MM, n, C, stream));
  TB_TRY(gemm(d, S, n, T.h1, fwd_weight(d, D, M_QKV), P[CDSEG_TB_QKV_B], 3 * C, C, T.qkv, AT, nullptr, stream));
  const size_t ea = esz(AT);
  const char* q = (const char*)T.qkv;
  // the core's output: proj's operand as it is when both are 16 bit (or both fp32); fp32 products on a 16-bit core widen it
  void* o_core = (AT == MM) ? T.o : S.h0;
  TB_TRY(cdseg_attention(q, q + C * ea, q + 2 * C * ea, 3 * C, 3 * C, 3 * C, io->gidx, io->gidx, io->widx, io->patch_start,
                         io->num_patches, d->heads, io->max_len, d->attn_scale, o_core, C, AT, stream));
  if (AT != MM) TB_TRY(cdseg_cast(o_core, AT, T.o, MM, n * C, stream));
  TB_TRY(gemm(d, S, n, T.o, fwd_weight(d, D, M_PROJ), P[CDSEG_TB_PROJ_B], C, C, S.f0, CDSEG_F32, nullptr, stream));
  TB_TRY(cdseg_add_layernorm((const float*)T.x0, (const float*)S.f0, io->mask1, P[CDSEG_TB_NORM2_G], P[CDSEG_TB_NORM2_B],
                             d->eps_norm2, (float*)T.x1, T.h2, MM, n, C, stream));

  // ---- MLP branch: x_out = x1 + mask2 * fc2(GELU(fc1(h2)))
  TB_TRY(gemm(d, S, n, T.h2, fwd_weight(d, D, M_FC1), P[CDSEG_TB_FC1_B], H, C, T.u, CDSEG_F32, nullptr, stream));
  TB_TRY(cdseg_gelu_fwd((const float*)T.u, T.g, MM, n * H, stream));
  TB_TRY(gemm(d, S, n, T.g, fwd_weight(d, D, M_FC2), P[CDSEG_TB_FC2_B], C, H, S.f1, CDSEG_F32, nullptr, stream));
  TB_TRY(cdseg_residual((const float*)T.x1, (const float*)S.f1, io->mask2, nullptr, nullptr, 0, io->x_out, n, C, stream));
  return CDSEG_OK;
}

// ================================================================ backward
extern "C" int cdseg_train_block_backward(const cdseg_train_block_desc* d, const cdseg_train_block_io* io, const float* dy,
                                          float* dx_in, float* dx_conv, float* dt_rows, void* grad_slab, void* stream) {
  if (!desc_ok(d) || !io) return CDSEG_ERR_ARG;
  if (io->n <= 0) return CDSEG_OK;
  if (!desc_ptrs_ok(d) || !io_ok(d, io, false)) return CDSEG_ERR_ARG;
  if (!dy || !dx_in || !grad_slab || !al16(dy) || !al16(dx_in) || !al16(dx_conv) || !al16(dt_rows) || !al16(grad_slab))
    return CDSEG_ERR_ARG;
  const bool same = io->x_conv == io->x_in;
  if ((!same && !dx_conv) || (io->t_rows && !dt_rows)) return CDSEG_ERR_ARG;
  if (io->t_rows && (long)io->num_scenes > io->n) return CDSEG_ERR_ARG;  // (no more scenes than rows: the scene sums' partials)
  const long n = io->n;
  const int C = d->channels, H = d->hidden, MM = d->mm_dtype, AT = d->attn_dtype;
  const bool lp = MM == CDSEG_BF16;
  hipStream_t s = (hipStream_t)stream;
  const Derived D = carve_derived(d, d->derived);
  const Tape T = carve_tape(d, n, io->tape);
  const Scratch S = carve_scratch(d, n, io->num_slots, io->scratch);
  const Grads G = carve_grads(d);
  const float* const* P = d->param;
  auto grad = [&](int p) { return (float*)((char*)grad_slab + G.off[p]); };
  if (hipMemsetAsync(grad_slab, 0, G.total, s) != hipSuccess) return CDSEG_ERR_LAUNCH;

  // ---- x_out = x1 + mask2 * hm:  d hm = mask2 * dy  (the operand of fc2's two products)
  const void* dhm = dy;
  if (lp) {
    TB_TRY(cdseg_scale_cast(dy, io->mask2, S.h0, CDSEG_BF16, n, C, stream));
    dhm = S.h0;
  } else if (io->mask2) {
    TB_TRY(cdseg_scale_cast(dy, io->mask2, S.f0, CDSEG_F32, n, C, stream));
    dhm = S.f0;
  }
  TB_TRY(lin_wgrad(d, S, T.g, dhm, n, H, C, grad(CDSEG_TB_FC2_W), grad(CDSEG_TB_FC2_B), stream));
  TB_TRY(gemm(d, S, n, dhm, D.t[M_FC2], nullptr, H, C, S.f1, CDSEG_F32, nullptr, stream));  // d g
  void* du = lp ? S.h0 : S.f0;
  TB_TRY(cdseg_gelu_bwd_cast((const float*)T.u, (const float*)S.f1, du, MM, n * H, stream));
  TB_TRY(lin_wgrad(d, S, T.h2, du, n, C, H, grad(CDSEG_TB_FC1_W), grad(CDSEG_TB_FC1_B), stream));
  TB_TRY(gemm(d, S, n, du, D.t[M_FC1], nullptr, C, H, S.f1, CDSEG_F32, nullptr, stream));  // d h2
  // ---- d x1 = dy + LN2'(x1)^T d h2, built in dx_in
  if (hipMemcpyAsync(dx_in, dy, (size_t)n * C * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return CDSEG_ERR_LAUNCH;
  TB_TRY(ln_bwd(d, S, (const float*)T.x1, P[CDSEG_TB_NORM2_G], d->eps_norm2, (const float*)S.f1, dx_in, 1, grad(CDSEG_TB_NORM2_G),
                grad(CDSEG_TB_NORM2_B), n, stream));
  // ---- x1 = x0 + mask1 * a:  d a = mask1 * d x1
  const void* da = dx_in;
  if (lp) {
    TB_TRY(cdseg_scale_cast(dx_in, io->mask1, S.h0, CDSEG_BF16, n, C, stream));
    da = S.h0;
  } else if (io->mask1) {
    TB_TRY(cdseg_scale_cast(dx_in, io->mask1, S.f0, CDSEG_F32, n, C, stream));
    da = S.f0;
  }
  TB_TRY(lin_wgrad(d, S, T.o, da, n, C, C, grad(CDSEG_TB_PROJ_W), grad(CDSEG_TB_PROJ_B), stream));
  TB_TRY(gemm(d, S, n, da, D.t[M_PROJ], nullptr, C, C, S.f1, CDSEG_F32, nullptr, stream));  // d o (fp32)
  const void* dout = S.f1;
  if (AT == CDSEG_BF16) {
    TB_TRY(cast_nosat((const float*)S.f1, S.h0, n, C, stream));
    dout = S.h0;
  }
  // ---- attention core: fp32 dq / dk / dv += at the gathered rows of a zeroed buffer
  float* dqkv = (float*)S.f0;
  if (hipMemsetAsync(dqkv, 0, (size_t)n * 3 * C * 4, s) != hipSuccess) return CDSEG_ERR_LAUNCH;
  const size_t ea = esz(AT);
  const char* q = (const char*)T.qkv;
  TB_TRY(cdseg_attention_bwd(q, q + C * ea, q + 2 * C * ea, 3 * C, 3 * C, 3 * C, io->gidx, io->gidx, io->widx, io->patch_start,
                             io->num_patches, d->heads, io->num_slots, io->max_len, d->attn_scale, dout, C, dqkv, dqkv + C,
                             dqkv + 2 * C, 3 * C, 3 * C, 3 * C, AT, S.aux, S.aux_bytes, stream));
  const void* dq_op = dqkv;
  if (lp) {
    TB_TRY(cast_nosat(dqkv, S.h0, n, 3 * C, stream));
    dq_op = S.h0;
  }
  TB_TRY(lin_wgrad(d, S, T.h1, dq_op, n, C, 3 * C, grad(CDSEG_TB_QKV_W), grad(CDSEG_TB_QKV_B), stream));
  TB_TRY(gemm(d, S, n, dq_op, D.t[M_QKV], nullptr, C, 3 * C, S.f1, CDSEG_F32, nullptr, stream));  // d h1
  // ---- d x0 = d x1 + LN1'(x0)^T d h1, in place
  TB_TRY(ln_bwd(d, S, (const float*)T.x0, P[CDSEG_TB_NORM1_G], d->eps_norm1, (const float*)S.f1, dx_in, 1, grad(CDSEG_TB_NORM1_G),
                grad(CDSEG_TB_NORM1_B), n, stream));
  // (dt_rows: the scene sums of d x0; S.f1 - d h1, consumed by the LayerNorm backward above - takes the chunk partials)
  if (io->t_rows)
    TB_TRY(scene_sums(dx_in, io->scene_offs, io->num_scenes, n, C, (float*)S.f1, (size_t)n * (3 * C > H ? 3 * C : H) * 4, dt_rows, stream));
  // ---- CPE: x0 = x_in + LN(z), z = Linear(yc), yc = conv(x_conv)
  // (row level: the CPE term of a voxel was read by every row of its run - its gradient is the run's sum in ascending row
  // order, and everything down to the conv's data gradient has nc rows; S.f1 is free once the scene sums are out)
  const bool rows = io->n_conv > 0;
  const long nc = rows ? io->n_conv : n;
  const float* dcpe = dx_in;
  if (rows) {
    TB_TRY(cdseg_run_sum(dx_in, io->row_start, (float*)S.f1, nc, C, stream));
    dcpe = (const float*)S.f1;
  }
  float* dz = (float*)S.f0;
  TB_TRY(ln_bwd(d, S, (const float*)T.z, P[CDSEG_TB_CPE_LN_G], d->eps_cpe, dcpe, dz, 0, grad(CDSEG_TB_CPE_LN_G),
                grad(CDSEG_TB_CPE_LN_B), nc, stream));
  const void* dz_op = dz;
  if (lp) {
    TB_TRY(cast_nosat(dz, S.h0, nc, C, stream));
    dz_op = S.h0;
  }
  TB_TRY(lin_wgrad(d, S, T.yc, dz_op, nc, C, C, grad(CDSEG_TB_CPE_W), grad(CDSEG_TB_CPE_B), stream));
  TB_TRY(gemm(d, S, nc, dz_op, D.t[M_CPE], nullptr, C, C, S.f1, CDSEG_F32, nullptr, stream));  // d yc
  const void* dyc = S.f1;
  if (lp) {
    TB_TRY(cast_nosat((const float*)S.f1, S.h0, nc, C, stream));
    dyc = S.h0;
  }
  const void* xc = lp ? (const void*)T.xc16 : (const void*)io->x_conv;
  if (rows && !lp) {  // the fp32 voxel rows of x_conv are not on the tape: gathered again (S.h0 is idle with fp32 products)
    TB_TRY(cdseg_gather_first(io->x_conv, io->row_start, S.h0, CDSEG_F32, nc, C, stream));
    xc = S.h0;
  }
  if (d->deterministic)
    TB_TRY(cdseg_conv_wgrad_det(xc, C, io->nbr, 27, dyc, C, nc, C, C, grad(CDSEG_TB_CONV_W), grad(CDSEG_TB_CONV_B), MM, S.aux,
                                S.aux_bytes, stream));
  else if (lp)
    TB_TRY(cdseg_conv_wgrad16(xc, C, io->nbr, 27, dyc, C, nc, C, C, grad(CDSEG_TB_CONV_W), grad(CDSEG_TB_CONV_B), stream));
  else
    TB_TRY(cdseg_conv_wgrad((const float*)xc, C, io->nbr, 27, (const float*)dyc, C, nc, C, C, grad(CDSEG_TB_CONV_W),
                            grad(CDSEG_TB_CONV_B), stream));
  float* dxc = (same || rows) ? (float*)S.f0 : dx_conv;
  TB_TRY(gemm(d, S, nc, dyc, D.t[M_CONV], nullptr, C, C, dxc, CDSEG_F32, io->nbr, stream));
  if (rows) TB_TRY(cdseg_scatter_first(dxc, io->row_vox, io->row_start, same ? dx_in : dx_conv, same ? 1 : 0, n, C, stream));
  else if (same) TB_TRY(cdseg_residual(dx_in, dxc, nullptr, nullptr, nullptr, 0, dx_in, n, C, stream));
  return CDSEG_OK;
}
