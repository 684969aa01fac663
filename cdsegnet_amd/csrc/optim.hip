// Fused optimizer step (include/cdseg.h, "fused optimizer step"): one read of the gradients for the clip norm and the
// non-finite flag, one pass for unscale + clip + AdamW + the 16-bit weight copy.  HBM-bound: 16-byte loads / stores per lane
// where a tensor's pointers allow it, no transcendental per element (the bias corrections come from one fp64 pow per block
// and tensor).  Every float sum runs in an order fixed by the chunk list: no atomics, no block waits for another.
#include <math.h>

#include <algorithm>

#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / CDSEG_WAVE;
constexpr int MAX_BLOCKS = 2048;  // 256 CUs x 8 blocks: the chunks beyond are grid-strided
constexpr long MAX_N = 1L << 31;  // chunk starts are int32

static_assert(CDSEG_OPT_CHUNK % (4 * THREADS) == 0, "a chunk is whole float4 rounds of the block");

struct OptGroups {
  cdseg_opt_group g[CDSEG_OPT_MAX_GROUPS];
};

inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

// workspace: [tensor table][per-chunk sum of squares, fp64][per-chunk non-finite flag]
struct WsLayout {
  size_t tab, part, flag, total;
};
inline WsLayout ws_layout(int count, long nchunks) {
  WsLayout L;
  L.tab = 0;
  L.part = al256((size_t)count * sizeof(cdseg_opt_tensor));
  L.flag = L.part + al256((size_t)nchunks * sizeof(double));
  L.total = L.flag + al256((size_t)nchunks * sizeof(int32_t));
  return L;
}

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ int nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// sum over the chunk of (g * inv_scale)^2 and the non-finite flag of the raw g.  Order: a lane adds its elements by ascending
// index in fp32 (one 16-byte load = x, y, z, w in this order), lanes through the 64-wide butterfly in fp64, the four waves by
// ascending wave index; the block's partial is a plain store.
__global__ __launch_bounds__(THREADS) void grad_sq_kernel(const cdseg_opt_tensor* __restrict__ tab,
                                                          int count, const int32_t* __restrict__ chunks, long nchunks,
                                                          const float* __restrict__ grad_scale, double* __restrict__ part,
                                                          int32_t* __restrict__ flag) {
#pragma clang fp contract(off)
  __shared__ double s_sum[WAVES];
  __shared__ int s_bad[WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float inv = grad_scale ? (float)(1.0 / (double)grad_scale[0]) : 1.f;
  for (long c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int ti = chunks[2 * c];
    const long start = chunks[2 * c + 1];
    double total = 0.0;
    int any = 0;
    // (uniform per block; an entry outside the table - a chunk list made for other sizes - is never followed)
    const bool live = (unsigned)ti < (unsigned)count && start >= 0 && start < tab[ti].n && !(tab[ti].flags & CDSEG_OPT_SKIP);
    if (live) {
      const cdseg_opt_tensor t = tab[ti];
      const long left = t.n - start;
      const int cnt = left < CDSEG_OPT_CHUNK ? (int)left : CDSEG_OPT_CHUNK;
      const float* g = t.g + start;
      float acc = 0.f;
      int bad = 0;
      if (aligned16(t.g)) {
        const int nvec = cnt >> 2;
        for (int i = tid; i < nvec; i += THREADS) {
          const float4 q = reinterpret_cast<const float4*>(g)[i];
          bad |= nonfinite(q.x) | nonfinite(q.y) | nonfinite(q.z) | nonfinite(q.w);
          const float a = q.x * inv, b = q.y * inv, cc = q.z * inv, d = q.w * inv;
          acc += a * a;
          acc += b * b;
          acc += cc * cc;
          acc += d * d;
        }
        const int i = 4 * nvec + tid;  // the tail of 1 - 3 elements
        if (tid < (cnt & 3)) {
          bad |= nonfinite(g[i]);
          const float a = g[i] * inv;
          acc += a * a;
        }
      } else {
        for (int i = tid; i < cnt; i += THREADS) {
          bad |= nonfinite(g[i]);
          const float a = g[i] * inv;
          acc += a * a;
        }
      }
      const double w = wave_sum_f64((t.flags & CDSEG_OPT_CLIP) ? (double)acc : 0.0);
      const int wb = __any(bad);
      if (lane == 0) {
        s_sum[wave] = w;
        s_bad[wave] = wb;
      }
      __syncthreads();
      if (tid == 0) {
        for (int k = 0; k < WAVES; ++k) {
          total += s_sum[k];
          any |= s_bad[k];
        }
      }
      __syncthreads();
    }
    if (tid == 0) {
      part[c] = total;
      flag[c] = any;
    }
  }
}

// one block: lane t adds the partials of chunks [t L, (t + 1) L) by ascending chunk index (L = ceil(nchunks / 256)), lane 0
// then adds the 256 lane sums by ascending lane - every partial enters in ascending chunk order, in fp64.
// out[0] = norm, out[1] = clip_coef (torch's clip_grad_norm_: fp32 min(1, max_norm / (norm + 1e-6))), out[2] = non-finite flag
__global__ __launch_bounds__(THREADS) void grad_norm_finish_kernel(const double* __restrict__ part, const int32_t* __restrict__ flag,
                                                                   long nchunks, float max_norm, float* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double s_sum[THREADS];
  __shared__ int s_bad[THREADS];
  const int tid = threadIdx.x;
  const long per = (nchunks + THREADS - 1) / THREADS;
  const long lo = tid * per, hi = lo + per < nchunks ? lo + per : nchunks;
  double s = 0.0;
  int bad = 0;
  for (long c = lo; c < hi; ++c) {
    s += part[c];
    bad |= flag[c];
  }
  s_sum[tid] = s;
  s_bad[tid] = bad;
  __syncthreads();
  if (tid == 0) {
    double total = 0.0;
    int any = 0;
    for (int k = 0; k < THREADS; ++k) {
      total += s_sum[k];
      any |= s_bad[k];
    }
    const float norm = (float)sqrt(total);
    out[0] = norm;
    out[1] = fminf(1.f, max_norm / (norm + 1e-6f));
    out[2] = any ? 1.f : 0.f;
  }
}

__global__ void step_advance_kernel(const cdseg_opt_tensor* __restrict__ tab, int count, const float* __restrict__ found_inf) {
  if (found_inf && found_inf[0] != 0.f) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  if (!(tab[i].flags & CDSEG_OPT_SKIP)) tab[i].step[0] += 1.f;
}

// what one block needs of a tensor's group and step counter (fp64 on lane 0, broadcast through LDS)
struct StepConsts {
  float b1, omb1, b2, omb2, decay, step_size, bc2_sqrt, eps;
};

struct Upd {
  float inv, coef;
  bool scale, clip;
  StepConsts k;
  // every rounding is written out: the same inputs give the same bits whichever path (16-byte or scalar) an element takes
  __device__ __forceinline__ void operator()(float& p, float g, float& m, float& v) const {
#pragma clang fp contract(off)
    if (scale) g = g * inv;
    if (clip) g = g * coef;
    m = __builtin_fmaf(k.omb1, g, k.b1 * m);
    v = __builtin_fmaf(k.omb2 * g, g, k.b2 * v);
    const float denom = sqrtf(v) / k.bc2_sqrt + k.eps;
    p = __builtin_fmaf(-k.step_size, m / denom, p * k.decay);
  }
};

__global__ __launch_bounds__(THREADS) void adamw_kernel(const cdseg_opt_tensor* __restrict__ tab, int count, const int32_t* __restrict__ chunks,
                                                        long nchunks, OptGroups groups, const float* __restrict__ grad_scale,
                                                        const float* __restrict__ found_inf, const float* __restrict__ clip_coef) {
  if (found_inf && found_inf[0] != 0.f) return;  // a skipped step writes nothing
  __shared__ StepConsts s_k;
  const int tid = threadIdx.x;
  Upd u;
  u.scale = grad_scale != nullptr;
  u.clip = clip_coef != nullptr;
  u.inv = u.scale ? (float)(1.0 / (double)grad_scale[0]) : 1.f;
  const float coef = u.clip ? clip_coef[0] : 1.f;
  int cur = -1;
  for (long c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int ti = chunks[2 * c];
    const long start = chunks[2 * c + 1];
    if ((unsigned)ti >= (unsigned)count) continue;  // (uniform per block; as in grad_sq_kernel)
    const cdseg_opt_tensor t = tab[ti];
    if ((t.flags & CDSEG_OPT_SKIP) || start < 0 || start >= t.n) continue;
    if (ti != cur) {
      cur = ti;
      __syncthreads();  // (the previous tensor's constants have been read)
      if (tid == 0) {
        const cdseg_opt_group gr = groups.g[t.group];
        const double step = (double)t.step[0];  // already advanced
        const double bc1 = 1.0 - pow(gr.beta1, step), bc2 = 1.0 - pow(gr.beta2, step);
        StepConsts k;
        k.b1 = (float)gr.beta1;
        k.omb1 = (float)(1.0 - gr.beta1);
        k.b2 = (float)gr.beta2;
        k.omb2 = (float)(1.0 - gr.beta2);
        k.decay = (float)(1.0 - gr.lr * gr.weight_decay);
        k.step_size = (float)(gr.lr / bc1);
        k.bc2_sqrt = (float)sqrt(bc2);
        k.eps = (float)gr.eps;
        s_k = k;
      }
      __syncthreads();
      u.k = s_k;
    }
    u.clip = clip_coef != nullptr && (t.flags & CDSEG_OPT_CLIP);
    u.coef = coef;
    const long left = t.n - start;
    const int cnt = left < CDSEG_OPT_CHUNK ? (int)left : CDSEG_OPT_CHUNK;
    float* p = t.p + start;
    const float* g = t.g + start;
    float* m = t.m + start;
    float* v = t.v + start;
    bf16_t* p16 = t.p16 ? (bf16_t*)t.p16 + start : nullptr;
    const bool vec = aligned16(t.p) && aligned16(t.g) && aligned16(t.m) && aligned16(t.v) && aligned16(t.p16);
    if (vec) {
      const int nvec = cnt >> 2;
#pragma unroll 2
      for (int i = tid; i < nvec; i += THREADS) {
        float4 P = reinterpret_cast<float4*>(p)[i];
        const float4 G = reinterpret_cast<const float4*>(g)[i];
        float4 M = reinterpret_cast<float4*>(m)[i];
        float4 V = reinterpret_cast<float4*>(v)[i];
        u(P.x, G.x, M.x, V.x);
        u(P.y, G.y, M.y, V.y);
        u(P.z, G.z, M.z, V.z);
        u(P.w, G.w, M.w, V.w);
        reinterpret_cast<float4*>(p)[i] = P;
        reinterpret_cast<float4*>(m)[i] = M;
        reinterpret_cast<float4*>(v)[i] = V;
        if (p16) {
          // the conversion of cdseg_cast, two elements per instruction (saturating in the IEEE-half build)
          reinterpret_cast<uint2*>(p16)[i] = make_uint2(pack_bf16x2(P.x, P.y), pack_bf16x2(P.z, P.w));
        }
      }
    }
    // scalar path: the whole chunk, or the 16-byte path's tail of 1 - 3 elements
    for (int i = (vec ? (cnt & ~3) : 0) + tid; i < cnt; i += THREADS) {
      float P = p[i], M = m[i], V = v[i];
      u(P, g[i], M, V);
      p[i] = P;
      m[i] = M;
      v[i] = V;
      if (p16) p16[i] = f32_to_bf16(P);
    }
  }
}

// every check of the tensor table and the groups, before any launch
int check_table(const cdseg_opt_tensor* t, int count, const cdseg_opt_group* groups, int ngroups) {
  if (!t || count <= 0) return CDSEG_ERR_ARG;
  if (groups) {
    if (ngroups <= 0) return CDSEG_ERR_ARG;
    if (ngroups > CDSEG_OPT_MAX_GROUPS) return CDSEG_ERR_UNSUPPORTED;
  }
  for (int i = 0; i < count; ++i) {
    const cdseg_opt_tensor& e = t[i];
    if (!e.p || !e.g || !e.m || !e.v || !e.step || e.n <= 0) return CDSEG_ERR_ARG;
    if (((uintptr_t)e.p | (uintptr_t)e.g | (uintptr_t)e.m | (uintptr_t)e.v | (uintptr_t)e.step) & 3) return CDSEG_ERR_ARG;
    if ((uintptr_t)e.p16 & 1) return CDSEG_ERR_ARG;
    if (groups && (e.group < 0 || e.group >= ngroups)) return CDSEG_ERR_ARG;
    if (e.flags & ~(CDSEG_OPT_CLIP | CDSEG_OPT_SKIP)) return CDSEG_ERR_ARG;
    if (e.n >= MAX_N) return CDSEG_ERR_UNSUPPORTED;
  }
  return CDSEG_OK;
}

// the chunk count of the table must be the one the caller's (device) chunk list was made for
int check_work(const cdseg_opt_tensor* t, int count, const int32_t* chunks_dev, long nchunks, const void* ws, size_t ws_bytes) {
  if (!chunks_dev || ((uintptr_t)chunks_dev & 3)) return CDSEG_ERR_ARG;
  long want = 0;
  for (int i = 0; i < count; ++i) want += (t[i].n + CDSEG_OPT_CHUNK - 1) / CDSEG_OPT_CHUNK;
  if (nchunks != want) return CDSEG_ERR_ARG;
  if (!ws) return CDSEG_ERR_WORKSPACE;
  if ((uintptr_t)ws & 15) return CDSEG_ERR_ARG;
  if (ws_bytes < cdseg_opt_ws_bytes(count, nchunks)) return CDSEG_ERR_WORKSPACE;
  return CDSEG_OK;
}

}  // namespace

extern "C" {

int cdseg_opt_chunks(const long* n_host, int count, int32_t* chunks_host, long* nchunks) {
  if (!n_host || count <= 0 || !nchunks) return CDSEG_ERR_ARG;
  long k = 0;
  for (int i = 0; i < count; ++i) {
    if (n_host[i] <= 0) return CDSEG_ERR_ARG;
    if (n_host[i] >= MAX_N) return CDSEG_ERR_UNSUPPORTED;
    for (long s = 0; s < n_host[i]; s += CDSEG_OPT_CHUNK, ++k) {
      if (chunks_host) {
        chunks_host[2 * k] = i;
        chunks_host[2 * k + 1] = (int32_t)s;
      }
    }
  }
  *nchunks = k;
  return CDSEG_OK;
}

size_t cdseg_opt_ws_bytes(int count, long nchunks) {
  if (count <= 0 || nchunks <= 0) return 0;
  return ws_layout(count, nchunks).total;
}

int cdseg_grad_norm(const cdseg_opt_tensor* tensors_host, int count, const int32_t* chunks_dev, long nchunks,
                    const float* grad_scale, float max_norm, float* out, void* ws, size_t ws_bytes, void* stream) {
  int st = check_table(tensors_host, count, nullptr, 0);
  if (st != CDSEG_OK) return st;
  if (!out || ((uintptr_t)out & 3) || ((uintptr_t)grad_scale & 3) || !(max_norm >= 0.f)) return CDSEG_ERR_ARG;
  if ((st = check_work(tensors_host, count, chunks_dev, nchunks, ws, ws_bytes)) != CDSEG_OK) return st;
  const WsLayout L = ws_layout(count, nchunks);
  hipStream_t s = (hipStream_t)stream;
  cdseg_opt_tensor* tab = (cdseg_opt_tensor*)((char*)ws + L.tab);
  double* part = (double*)((char*)ws + L.part);
  int32_t* flag = (int32_t*)((char*)ws + L.flag);
  if (hipMemcpyAsync(tab, tensors_host, (size_t)count * sizeof(cdseg_opt_tensor), hipMemcpyHostToDevice, s) != hipSuccess)
    return CDSEG_ERR_LAUNCH;
  const int blocks = (int)std::min<long>(nchunks, MAX_BLOCKS);
  hipLaunchKernelGGL(grad_sq_kernel, dim3(blocks), dim3(THREADS), 0, s, tab, count, chunks_dev, nchunks, grad_scale, part, flag);
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(THREADS), 0, s, part, flag, nchunks, max_norm, out);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_adamw_step(const cdseg_opt_tensor* tensors_host, int count, const cdseg_opt_group* groups_host, int ngroups,
                     const int32_t* chunks_dev, long nchunks, const float* grad_scale, const float* found_inf,
                     const float* clip_coef, void* ws, size_t ws_bytes, void* stream) {
  if (!groups_host) return CDSEG_ERR_ARG;
  int st = check_table(tensors_host, count, groups_host, ngroups);
  if (st != CDSEG_OK) return st;
  for (int i = 0; i < ngroups; ++i) {
    const cdseg_opt_group& g = groups_host[i];
    if (!(g.lr >= 0.0) || !(g.beta1 >= 0.0 && g.beta1 < 1.0) || !(g.beta2 >= 0.0 && g.beta2 < 1.0) || !(g.eps >= 0.0) ||
        !(g.weight_decay >= 0.0))
      return CDSEG_ERR_ARG;
  }
  if (((uintptr_t)grad_scale | (uintptr_t)found_inf | (uintptr_t)clip_coef) & 3) return CDSEG_ERR_ARG;
  if ((st = check_work(tensors_host, count, chunks_dev, nchunks, ws, ws_bytes)) != CDSEG_OK) return st;
  const WsLayout L = ws_layout(count, nchunks);
  hipStream_t s = (hipStream_t)stream;
  cdseg_opt_tensor* tab = (cdseg_opt_tensor*)((char*)ws + L.tab);
  if (hipMemcpyAsync(tab, tensors_host, (size_t)count * sizeof(cdseg_opt_tensor), hipMemcpyHostToDevice, s) != hipSuccess)
    return CDSEG_ERR_LAUNCH;
  OptGroups groups = {};
  for (int i = 0; i < ngroups; ++i) groups.g[i] = groups_host[i];
  hipLaunchKernelGGL(step_advance_kernel, dim3((count + THREADS - 1) / THREADS), dim3(THREADS), 0, s, tab, count, found_inf);
  const int blocks = (int)std::min<long>(nchunks, MAX_BLOCKS);
  hipLaunchKernelGGL(adamw_kernel, dim3(blocks), dim3(THREADS), 0, s, tab, count, chunks_dev, nchunks, groups, grad_scale, found_inf,
                     clip_coef);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

}  // extern "C"
