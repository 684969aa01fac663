// Train-time data pipeline on the device: the transform lists of the reference's train / val
// datasets, ref: configs/{scannet,scannet200,nuscenes}/CDSegNet.py `data.train.transform` / `data.val.transform`,
// pointcept/datasets/transform.py.  One streaming pass per kernel over (n,3) rows; a thread per row (24-byte float64 rows:
// the three 8-byte accesses of a wave cover one contiguous 1.5 KiB span, every fetched line is fully used).
//
// Coordinates (and normals) are float64 from the first transform to GridSample.  EVERY float64 operation below is a
// single correctly rounded add / multiply / divide in the written order - contraction is off for the whole file - so the
// results are bit-equal to a numpy restatement that performs the same operations (tests/traintime_restatement.py).
// GridSample itself reuses cdseg_voxelize_f64 / cdseg_sort_pairs / cdseg_pool_level / cdseg_max_run.
#include "common.h"

#pragma clang fp contract(off)

namespace {

inline dim3 g1(long n, int bs = 256) { return dim3((unsigned)((n + bs - 1) / bs)); }
inline dim3 gcap(long n, int bs = 256, long cap = 1024) {
  long b = (n + bs - 1) / bs;
  return dim3((unsigned)(b > cap ? cap : (b < 1 ? 1 : b)));
}

// ---- 1. bounding box of an (n,3) float32 / float64 array -> 6 doubles [min xyz, max xyz] in device memory
// (exact for both types).  Doubles go through an order-preserving integer image: one atomicMin / atomicMax per wave.
__device__ __forceinline__ unsigned long long ord_u64(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double ord_f64(unsigned long long u) {
  return __longlong_as_double((long long)((u >> 63) ? (u & 0x7fffffffffffffffull) : ~u));
}
template <typename T>
__global__ void bbox_kernel(const T* __restrict__ xyz, long n, unsigned long long* __restrict__ acc6) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (; i < n; i += stride)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double v = (double)xyz[3 * i + a];
      lo[a] = fmin(lo[a], v);
      hi[a] = fmax(hi[a], v);
    }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo[a] = fmin(lo[a], __shfl_xor(lo[a], o, 64));
      hi[a] = fmax(hi[a], __shfl_xor(hi[a], o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
      atomicMin(&acc6[a], ord_u64(lo[a]));
      atomicMax(&acc6[3 + a], ord_u64(hi[a]));
    }
  }
}
__global__ void bbox_finish_kernel(const unsigned long long* __restrict__ acc6, double* __restrict__ out6) {
  if (threadIdx.x < 6) out6[threadIdx.x] = ord_f64(acc6[threadIdx.x]);
}

// ---- 2. float64 affine: t = x - c ; t = R t ; t += c ; t *= scale ; flips.  Every stage optional.
// centre: CDSEG_TT_CENTER_*  (host triple, or derived from a device bounding box: no host read between the steps)
struct AffP {
  double r[9];   // row-major R: out_j = (t0 R[j][0] + t1 R[j][1]) + t2 R[j][2]
  double c[3];
  double scale;
  int center, rotate, add_back, apply_scale, flipx, flipy;
};
template <typename TI, typename TO>
__global__ void affine_kernel(const TI* __restrict__ in, const double* __restrict__ mm6, AffP p, long n,
                              TO* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double c[3] = {p.c[0], p.c[1], p.c[2]};
  if (p.center >= CDSEG_TT_CENTER_BBOX) {
    c[0] = (mm6[0] + mm6[3]) / 2.0;
    c[1] = (mm6[1] + mm6[4]) / 2.0;
    c[2] = p.center == CDSEG_TT_CENTER_BBOX ? (mm6[2] + mm6[5]) / 2.0 : (p.center == CDSEG_TT_CENTER_SHIFT_Z ? mm6[2] : 0.0);
  }
  double t[3] = {(double)in[3 * i], (double)in[3 * i + 1], (double)in[3 * i + 2]};
  if (p.center != CDSEG_TT_CENTER_NONE) { t[0] = t[0] - c[0]; t[1] = t[1] - c[1]; t[2] = t[2] - c[2]; }
  if (p.rotate) {
    double o[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) o[j] = (t[0] * p.r[3 * j] + t[1] * p.r[3 * j + 1]) + t[2] * p.r[3 * j + 2];
    t[0] = o[0]; t[1] = o[1]; t[2] = o[2];
  }
  if (p.add_back) { t[0] = t[0] + c[0]; t[1] = t[1] + c[1]; t[2] = t[2] + c[2]; }
  if (p.apply_scale) { t[0] = t[0] * p.scale; t[1] = t[1] * p.scale; t[2] = t[2] * p.scale; }
  if (p.flipx) t[0] = -t[0];
  if (p.flipy) t[1] = -t[1];
  out[3 * i] = (TO)t[0]; out[3 * i + 1] = (TO)t[1]; out[3 * i + 2] = (TO)t[2];
}

// ---- 3. RandomJitter: coord += clip(sigma * z, -clip, clip)   (transform.py:338-346); z float32 (device draws) or float64
template <typename TZ>
__global__ void jitter_kernel(double* __restrict__ coord, const TZ* __restrict__ z, double sigma, double clip, long n3) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n3) return;
  const double j = fmin(fmax(sigma * (double)z[i], -clip), clip);
  coord[i] = coord[i] + j;
}

// ---- 4. ElasticDistortion blur: zero-padded 3-tap box filter along one axis of a (d0,d1,d2,3) float32 grid, accumulated
// in float64 with the float32 weight 1/3 and rounded to float32 per pass (scipy.ndimage.convolve, transform.py:750-769)
__global__ void blur3_kernel(const float* __restrict__ in, int d0, int d1, int d2, int axis, float* __restrict__ out) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)d0 * d1 * d2 * 3;
  if (t >= total) return;
  const long cell = t / 3;
  const int z = (int)(cell % d2), y = (int)((cell / d2) % d1), x = (int)(cell / ((long)d2 * d1));
  const int pos = axis == 0 ? x : (axis == 1 ? y : z), len = axis == 0 ? d0 : (axis == 1 ? d1 : d2);
  const long stride = axis == 0 ? (long)d1 * d2 * 3 : (axis == 1 ? (long)d2 * 3 : 3);
  const double w = (double)(1.0f / 3.0f);
  double acc = 0.0;
  if (pos > 0) acc = acc + w * (double)in[t - stride];
  acc = acc + w * (double)in[t];
  if (pos + 1 < len) acc = acc + w * (double)in[t + stride];
  out[t] = (float)acc;
}

// ---- 5. ElasticDistortion apply: trilinear interpolation of the blurred grid on the axes
// ax_a(k) = k < d_a - 1 ? k * step_a + start_a : stop_a   (numpy's linspace), fill value 0 outside, coord += value * magnitude
// (scipy RegularGridInterpolator(method="linear", bounds_error=False, fill_value=0), transform.py:771-783)
struct ElaP {
  double start[3], step[3], stop[3];
  double magnitude;
  int d[3];
};
__device__ __forceinline__ double ela_axis(const ElaP& p, int a, int k) {
  return k < p.d[a] - 1 ? (double)k * p.step[a] + p.start[a] : p.stop[a];
}
__global__ void elastic_kernel(double* __restrict__ coord, const float* __restrict__ noise, ElaP p, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double x[3] = {coord[3 * i], coord[3 * i + 1], coord[3 * i + 2]};
  int k[3];
  double w1[3], w0[3];
  bool inside = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    inside = inside && x[a] >= p.start[a] && x[a] <= p.stop[a];  // NaN: outside
    int j = (int)floor((x[a] - p.start[a]) / p.step[a]);
    j = j < 0 ? 0 : (j > p.d[a] - 2 ? p.d[a] - 2 : j);
    while (j > 0 && x[a] < ela_axis(p, a, j)) --j;                 // the division above may be off by one cell
    while (j < p.d[a] - 2 && x[a] >= ela_axis(p, a, j + 1)) ++j;
    const double g0 = ela_axis(p, a, j), g1v = ela_axis(p, a, j + 1);
    k[a] = j;
    w1[a] = (x[a] - g0) / (g1v - g0);
    w0[a] = 1.0 - w1[a];
  }
  if (!inside) return;  // fill value 0: coord += 0
  double v[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int corner = 0; corner < 8; ++corner) {  // itertools.product order: axis 0 slowest
    const int b0 = corner >> 2, b1 = (corner >> 1) & 1, b2 = corner & 1;
    const double wgt = ((b0 ? w1[0] : w0[0]) * (b1 ? w1[1] : w0[1])) * (b2 ? w1[2] : w0[2]);
    const long cell = ((long)(k[0] + b0) * p.d[1] + (k[1] + b1)) * p.d[2] + (k[2] + b2);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) v[ch] = v[ch] + (double)noise[3 * cell + ch] * wgt;
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) coord[3 * i + ch] = x[ch] + v[ch] * p.magnitude;
}

// ---- 6. colour chain on (n,3) float32 in 0..255, in the reference's types (transform.py:385-431):
// auto contrast in float32, translation and jitter added in float64, clipped to [0, 255], rounded to float32
struct ColP {
  double tr[3];
  double noise_mul;  // std * 255
  float blend, one_minus_blend;
  int contrast, translate, jitter, noise_f64;
};
__global__ void color_kernel(float* __restrict__ color, const double* __restrict__ mm6, const void* __restrict__ noise,
                             ColP p, long n3) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n3) return;
  const int ch = (int)(i % 3);
  float c = color[i];
  if (p.contrast) {
    const float lo = (float)mm6[ch], hi = (float)mm6[3 + ch];
    const float scale = 255.0f / (hi - lo);
    const float contrast = (c - lo) * scale;
    c = p.one_minus_blend * c + p.blend * contrast;
  }
  if (p.translate) c = (float)fmin(fmax(p.tr[ch] + (double)c, 0.0), 255.0);
  if (p.jitter) {
    const double z = p.noise_f64 ? ((const double*)noise)[i] : (double)((const float*)noise)[i];
    c = (float)fmin(fmax(z * p.noise_mul + (double)c, 0.0), 255.0);
  }
  color[i] = c;
}

// ---- 7. GridSample(mode="train") pick: voxel v keeps its member r[v] % count[v]   (transform.py:834-838)
__global__ void voxel_pick_kernel(const int32_t* __restrict__ idx_sort, const int32_t* __restrict__ seg_start, long m,
                                  const int64_t* __restrict__ r, int32_t* __restrict__ out) {
  const long v = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= m) return;
  const int s = seg_start[v], c = seg_start[v + 1] - s;
  const int64_t rv = r[v] < 0 ? 0 : r[v];
  out[v] = idx_sort[s + (int)(rv % c)];
}

// ---- 8. SphereCrop key: float64 squared distance to row `center`, as its (order-preserving, non-negative) bit image
__global__ void dist_key_kernel(const double* __restrict__ coord, long n, long center, int64_t* __restrict__ key) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double dx = coord[3 * i] - coord[3 * center], dy = coord[3 * i + 1] - coord[3 * center + 1],
               dz = coord[3 * i + 2] - coord[3 * center + 2];
  const double d2 = (dx * dx + dy * dy) + dz * dz;
  key[i] = (d2 == d2) ? __double_as_longlong(d2) : 0x7ff8000000000000ll;  // NaN sorts last
}

// ---- 9. integer companion of cdseg_randn: the same Philox4x32-10 stream, out[4 t + i] = word i of thread t
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
  const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
  const uint32_t n1 = (uint32_t)p1;
  const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
  const uint32_t n3 = (uint32_t)p0;
  c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}
__global__ void rand_int_kernel(int64_t* __restrict__ out, long n, uint64_t seed, uint64_t offset,
                                const int32_t* __restrict__ bound_dev, uint32_t bound) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (4 * t >= n) return;
  uint32_t c[4] = {(uint32_t)t, (uint32_t)(t >> 32), (uint32_t)offset, (uint32_t)(offset >> 32)};
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  const uint32_t b = bound_dev ? (uint32_t)max(*bound_dev, 0) : bound;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (4 * t + i < n) out[4 * t + i] = (int64_t)(b ? c[i] % b : c[i]);
}

}  // namespace

extern "C" {

int cdseg_tt_bbox(const void* xyz, int is_f64, long n, void* ws12, void* stream) {
  if (n <= 0 || !xyz || !ws12) return CDSEG_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* acc = (unsigned long long*)ws12;
  if (hipMemsetAsync(acc, 0xff, 3 * 8, s) != hipSuccess || hipMemsetAsync(acc + 3, 0, 3 * 8, s) != hipSuccess)
    return CDSEG_ERR_LAUNCH;
  if (is_f64) hipLaunchKernelGGL(bbox_kernel<double>, gcap(n), dim3(256), 0, s, (const double*)xyz, n, acc);
  else hipLaunchKernelGGL(bbox_kernel<float>, gcap(n), dim3(256), 0, s, (const float*)xyz, n, acc);
  hipLaunchKernelGGL(bbox_finish_kernel, dim3(1), dim3(64), 0, s, acc, (double*)ws12 + 6);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_tt_affine(const void* in, int in_f64, long n, int center, const double* center3_host, const double* bbox6_dev,
                    const double* rot9_host, int add_back, double scale, int apply_scale, int flipx, int flipy, void* out,
                    int out_f64, void* stream) {
  if (n <= 0) return CDSEG_OK;
  if (!in || !out || center < CDSEG_TT_CENTER_NONE || center > CDSEG_TT_CENTER_SHIFT_XY) return CDSEG_ERR_ARG;
  if (center == CDSEG_TT_CENTER_HOST && !center3_host) return CDSEG_ERR_ARG;
  if (center >= CDSEG_TT_CENTER_BBOX && !bbox6_dev) return CDSEG_ERR_ARG;
  AffP p;
  p.center = center;
  p.rotate = rot9_host != nullptr;
  p.add_back = add_back && center != CDSEG_TT_CENTER_NONE;
  p.apply_scale = apply_scale;
  p.scale = scale;
  p.flipx = flipx;
  p.flipy = flipy;
  for (int i = 0; i < 9; ++i) p.r[i] = rot9_host ? rot9_host[i] : 0.0;
  for (int i = 0; i < 3; ++i) p.c[i] = center == CDSEG_TT_CENTER_HOST ? center3_host[i] : 0.0;
  hipStream_t s = (hipStream_t)stream;
  if (in_f64 && out_f64)
    hipLaunchKernelGGL((affine_kernel<double, double>), g1(n), dim3(256), 0, s, (const double*)in, bbox6_dev, p, n, (double*)out);
  else if (in_f64)
    hipLaunchKernelGGL((affine_kernel<double, float>), g1(n), dim3(256), 0, s, (const double*)in, bbox6_dev, p, n, (float*)out);
  else if (out_f64)
    hipLaunchKernelGGL((affine_kernel<float, double>), g1(n), dim3(256), 0, s, (const float*)in, bbox6_dev, p, n, (double*)out);
  else
    hipLaunchKernelGGL((affine_kernel<float, float>), g1(n), dim3(256), 0, s, (const float*)in, bbox6_dev, p, n, (float*)out);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_tt_jitter(double* coord, const void* z, int z_f64, double sigma, double clip, long n, void* stream) {
  if (n <= 0) return CDSEG_OK;
  if (!coord || !z || !(clip > 0)) return CDSEG_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (z_f64) hipLaunchKernelGGL(jitter_kernel<double>, g1(3 * n), dim3(256), 0, s, coord, (const double*)z, sigma, clip, 3 * n);
  else hipLaunchKernelGGL(jitter_kernel<float>, g1(3 * n), dim3(256), 0, s, coord, (const float*)z, sigma, clip, 3 * n);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_tt_blur3(const float* in, int d0, int d1, int d2, int axis, float* out, void* stream) {
  if (!in || !out || in == out || d0 <= 0 || d1 <= 0 || d2 <= 0 || axis < 0 || axis > 2) return CDSEG_ERR_ARG;
  hipLaunchKernelGGL(blur3_kernel, g1((long)d0 * d1 * d2 * 3), dim3(256), 0, (hipStream_t)stream, in, d0, d1, d2, axis, out);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_tt_elastic(double* coord, long n, const float* noise, const int* dims3_host, const double* start3_host,
                     const double* step3_host, const double* stop3_host, double magnitude, void* stream) {
  if (n <= 0) return CDSEG_OK;
  if (!coord || !noise || !dims3_host || !start3_host || !step3_host || !stop3_host) return CDSEG_ERR_ARG;
  ElaP p;
  for (int a = 0; a < 3; ++a) {
    if (dims3_host[a] < 2 || !(step3_host[a] > 0) || !(stop3_host[a] > start3_host[a])) return CDSEG_ERR_ARG;
    p.d[a] = dims3_host[a];
    p.start[a] = start3_host[a];
    p.step[a] = step3_host[a];
    p.stop[a] = stop3_host[a];
  }
  p.magnitude = magnitude;
  hipLaunchKernelGGL(elastic_kernel, g1(n), dim3(256), 0, (hipStream_t)stream, coord, noise, p, n);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_tt_color(float* color, long n, const double* bbox6_dev, double blend, int contrast, const double* tr3_host,
                   const void* noise, int noise_f64, double noise_mul, void* stream) {
  if (n <= 0) return CDSEG_OK;
  if (!color || (contrast && !bbox6_dev)) return CDSEG_ERR_ARG;
  ColP p;
  p.contrast = contrast;
  p.blend = (float)blend;  // the reference multiplies float32 arrays by the Python floats blend and 1 - blend
  p.one_minus_blend = (float)(1.0 - blend);
  p.translate = tr3_host != nullptr;
  for (int i = 0; i < 3; ++i) p.tr[i] = tr3_host ? tr3_host[i] : 0.0;
  p.jitter = noise != nullptr;
  p.noise_f64 = noise_f64;
  p.noise_mul = noise_mul;
  hipLaunchKernelGGL(color_kernel, g1(3 * n), dim3(256), 0, (hipStream_t)stream, color, bbox6_dev, noise, p, 3 * n);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_tt_voxel_pick(const int32_t* idx_sort, const int32_t* seg_start, long m, const int64_t* r, int32_t* out,
                        void* stream) {
  if (m <= 0) return CDSEG_OK;
  if (!idx_sort || !seg_start || !r || !out) return CDSEG_ERR_ARG;
  hipLaunchKernelGGL(voxel_pick_kernel, g1(m), dim3(256), 0, (hipStream_t)stream, idx_sort, seg_start, m, r, out);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_tt_dist_key(const double* coord, long n, long center, int64_t* key, void* stream) {
  if (n <= 0) return CDSEG_OK;
  if (!coord || !key || center < 0 || center >= n) return CDSEG_ERR_ARG;
  hipLaunchKernelGGL(dist_key_kernel, g1(n), dim3(256), 0, (hipStream_t)stream, coord, n, center, key);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_rand_int(int64_t* out, long n, uint64_t seed, uint64_t offset, const int32_t* bound_dev, uint32_t bound,
                   void* stream) {
  if (n <= 0) return CDSEG_OK;
  if (!out) return CDSEG_ERR_ARG;
  const long threads = (n + 3) / 4;
  hipLaunchKernelGGL(rand_int_kernel, g1(threads), dim3(256), 0, (hipStream_t)stream, out, n, seed, offset, bound_dev, bound);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

}  // extern "C"
