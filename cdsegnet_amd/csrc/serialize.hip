// Integer side of the hot path: space-filling-curve codes, orders, pooling clusters,
// sparse-conv neighbour tables, attention padding plans.  All HBM-bound index work:
// coalesced loads/stores, no LDS needed; sorting/scanning uses rocPRIM device primitives.
//
// Reference behaviour restated (bit-exact, see tests/test_gpu_serialization.py):
//   pointcept/models/utils/serialization/z_order.py:40-50,66-101   z-order key
//   pointcept/models/utils/serialization/hilbert.py:91-198          Skilling Hilbert key
//   pointcept/models/utils/serialization/default.py:8-24            order dispatch + batch bits
//   pointcept/models/utils/structure.py:47-102                      Point.serialization
//   .../point_transformer_v3m1_base.py:188-244                      get_padding_and_inverse
//   .../point_transformer_v3m1_base.py:477-492                      pooling clusters
#include "common.h"

#ifndef CDSEG_MERGE_SORT_LIMIT
#define CDSEG_MERGE_SORT_LIMIT 262144
#endif
#include "curves.h"

#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace {

template <typename G, typename B>
__global__ void encode_kernel(const G* __restrict__ grid, const B* __restrict__ batch, long n, int depth,
                              int order_id, int64_t* __restrict__ code) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t x = (uint32_t)grid[3 * i + 0], y = (uint32_t)grid[3 * i + 1], z = (uint32_t)grid[3 * i + 2];
  uint64_t k = curve_key(order_id, x, y, z, depth);
  if (batch) k |= ((uint64_t)batch[i]) << (3 * depth);
  code[i] = (int64_t)k;
}

// all four curves at once from an int32 grid (engine plan)
__global__ void encode4_kernel(const int32_t* __restrict__ grid, const int32_t* __restrict__ batch, long n,
                               int depth, int64_t* __restrict__ code /* (4, n) */) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t x = (uint32_t)grid[3 * i + 0], y = (uint32_t)grid[3 * i + 1], z = (uint32_t)grid[3 * i + 2];
  const uint64_t b = ((uint64_t)batch[i]) << (3 * depth);
#pragma unroll
  for (int o = 0; o < 4; ++o) code[(long)o * n + i] = (int64_t)(b | curve_key(o, x, y, z, depth));
}

template <typename G>
__global__ void grid_max_kernel(const G* __restrict__ grid, long n3, unsigned long long* __restrict__ out) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  long long m = 0;
  for (; i < n3; i += stride) {
    long long v = (long long)grid[i];
    m = v > m ? v : m;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    long long t = __shfl_xor(m, o, 64);
    m = t > m ? t : m;
  }
  __shared__ long long wmax[4];
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {  // one atomic per block (thousands of same-address 64-bit atomics cost ~50 us)
    for (int w = 1; w < 4; ++w) m = wmax[w] > m ? wmax[w] : m;
    atomicMax(out, (unsigned long long)m);
  }
}

__global__ void offset2batch_kernel(const int64_t* __restrict__ offset, int nb, long n, int32_t* __restrict__ batch) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int lo = 0, hi = nb - 1;  // first b with offset[b] > i
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if (offset[mid] > i) hi = mid; else lo = mid + 1;
  }
  batch[i] = lo;
}

// keys of several curves concatenated for ONE sort: key = (slot << end_bit) | code, value = point index
struct CurveRows {
  int r[4];
};
__global__ void tag_keys_kernel(const int64_t* __restrict__ codes /* rows of n */, CurveRows rows, int count, long n,
                                int end_bit, uint64_t* __restrict__ keys, int32_t* __restrict__ vals) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * count) return;
  const int c = (int)(t / n);
  const long i = t - (long)c * n;
  keys[t] = ((uint64_t)c << end_bit) | (uint64_t)codes[(long)rows.r[c] * n + i];
  vals[t] = (int32_t)i;
}

__global__ void iota_kernel(int32_t* __restrict__ v, long n) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = (int32_t)i;
}

__global__ void invert_perm_kernel(const int32_t* __restrict__ perm, long n, int32_t* __restrict__ inv) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) inv[perm[i]] = (int32_t)i;
}

__global__ void widen_kernel(const int32_t* __restrict__ src, long n, int64_t* __restrict__ dst) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

// dst[i, :] = src[idx[i], :] for rows of `row_words` 32-bit words; idx < 0 -> zeros
__global__ void gather_rows_kernel(const uint32_t* __restrict__ src, const int32_t* __restrict__ idx, long n_out,
                                   int row_words, uint32_t* __restrict__ dst) {
  long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long total = n_out * row_words;
  if (t >= total) return;
  long r = t / row_words;
  int c = (int)(t - r * row_words);
  int s = idx[r];
  dst[t] = s >= 0 ? src[(long)s * row_words + c] : 0u;
}

// dst[idx[i], :] = src[i, :]
__global__ void scatter_rows_kernel(const uint32_t* __restrict__ src, const int32_t* __restrict__ idx, long n_in,
                                    int row_words, uint32_t* __restrict__ dst) {
  long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long total = n_in * row_words;
  if (t >= total) return;
  long r = t / row_words;
  int c = (int)(t - r * row_words);
  int d = idx[r];
  if (d >= 0) dst[(long)d * row_words + c] = src[t];
}

// stage-0 plan: sorted grid (int32) + batch from the sort permutation
template <typename G>
__global__ void gather_grid_kernel(const G* __restrict__ grid, const int32_t* __restrict__ perm,
                                   const int64_t* __restrict__ zcode_sorted, long n, int depth,
                                   int32_t* __restrict__ grid_out, int32_t* __restrict__ batch_out) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long s = perm[i];
  grid_out[3 * i + 0] = (int32_t)grid[3 * s + 0];
  grid_out[3 * i + 1] = (int32_t)grid[3 * s + 1];
  grid_out[3 * i + 2] = (int32_t)grid[3 * s + 2];
  batch_out[i] = (int32_t)(((uint64_t)zcode_sorted[i]) >> (3 * depth));
}

// flags for one pooling level: a new cluster starts where the shifted z code changes
__global__ void level_flag_kernel(const int64_t* __restrict__ zc, long n, int shift, int32_t* __restrict__ flag) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  flag[i] = (i == 0 || (zc[i] >> shift) != (zc[i - 1] >> shift)) ? 1 : 0;
}

// cluster = inclusive_scan(flag) - 1 ; seg_start[cluster] = i at run starts ; count = last + 1
__global__ void level_finish_kernel(const int32_t* __restrict__ incl, const int32_t* __restrict__ flag, long n,
                                    int32_t* __restrict__ cluster, int32_t* __restrict__ seg_start,
                                    int32_t* __restrict__ count) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int c = incl[i] - 1;
  cluster[i] = c;
  if (flag[i]) seg_start[c] = (int32_t)i;
  if (i == n - 1) {
    seg_start[c + 1] = (int32_t)n;
    *count = c + 1;
  }
}

// ---- coarse-level curve orders WITHOUT sorting.  A pooled level's code on any of the four curves is the fine code
// shifted right (ref: ptv3.py:503-514 - SerializedPooling shifts the parent codes and arg-sorts them); z-order and
// Hilbert keys are hierarchical, so the fine points of one coarse cell are contiguous in EVERY fine curve order and
// the coarse order is the fine order with each point replaced by its cluster id and consecutive duplicates removed.
// One flag / scan / compact pass covers all levels x curves (segments back to back; each yields exactly m_l flags).
struct CoarseP {
  const int32_t* cluster[8];  // per level: fine point -> cluster id
  const int32_t* order[3];    // per curve: rank -> fine point
  long n0;
  int nlev, ncurve;
};

__device__ __forceinline__ bool coarse_head(const CoarseP& p, long i, int32_t* v_out) {
  const long per = (long)p.ncurve * p.n0;
  const int l = (int)(i / per);
  const long r = i - (long)l * per;
  const int c = (int)(r / p.n0);
  const long j = r - (long)c * p.n0;
  const int32_t* cl = p.cluster[l];
  const int32_t* od = p.order[c];
  const int32_t v = cl[od[j]];
  *v_out = v;
  return j == 0 || cl[od[j - 1]] != v;
}

__global__ void coarse_flag_kernel(CoarseP p, long total, int32_t* __restrict__ flag) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  int32_t v;
  flag[i] = coarse_head(p, i, &v) ? 1 : 0;
}

__global__ void coarse_compact_kernel(CoarseP p, long total, const int32_t* __restrict__ pos, int32_t* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  int32_t v;
  if (coarse_head(p, i, &v)) out[pos[i] - 1] = v;
}

// ---- all pooling levels of a scene in one flag / scan / finish pass (levels back to back in one array)
struct LevelsP {
  int shift[8];
  int nlev, nb;
  long n;
};

__global__ void levels_flag_kernel(const int64_t* __restrict__ zc, LevelsP p, int32_t* __restrict__ flag,
                                   int32_t* __restrict__ meta) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0) meta[p.nlev * (1 + p.nb)] = 0;  // duplicate-voxel counter, filled by levels_finish_kernel
  if (t >= p.n * p.nlev) return;
  const int l = (int)(t / p.n);
  const long i = t - (long)l * p.n;
  const int sh = p.shift[l];
  flag[t] = (i == 0 || (zc[i] >> sh) != (zc[i - 1] >> sh)) ? 1 : 0;
}

// cluster (L,n), seg_start (L,n+1), meta (L, 1+nb): [count, cluster id of the last point of every batch element], then ONE
// trailing int: the number of points whose (batch, voxel) code equals their predecessor's - the model's input contract is
// one point per voxel (GridSample; SURVEY 7: the kernel maps and the derived coarse orders assume it), so the host turns a
// non-zero count into an error with the read it already does for the pooled sizes
__global__ void levels_finish_kernel(const int64_t* __restrict__ zc, const int32_t* __restrict__ incl,
                                     const int32_t* __restrict__ flag, LevelsP p,
                                     const int32_t* __restrict__ last_idx, int32_t* __restrict__ cluster,
                                     int32_t* __restrict__ seg_start, int32_t* __restrict__ meta) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= p.n * p.nlev) return;
  const int l = (int)(t / p.n);
  const long i = t - (long)l * p.n;
  if (l == 0 && i > 0 && zc[i] == zc[i - 1]) atomicAdd(&meta[p.nlev * (1 + p.nb)], 1);
  const int base = l ? incl[(long)l * p.n - 1] : 0;
  const int c = incl[t] - base - 1;
  cluster[t] = c;
  int32_t* seg = seg_start + (long)l * (p.n + 1);
  if (flag[t]) seg[c] = (int32_t)i;
  if (i == p.n - 1) {
    seg[c + 1] = (int32_t)p.n;
    meta[l * (1 + p.nb)] = c + 1;
  }
  for (int b = 0; b < p.nb; ++b)
    if (last_idx[b] == i) meta[l * (1 + p.nb) + 1 + b] = c;
}

// link between two pooled levels a (finer) and b from their links to level 0:
//   cluster_ab[j] = cluster_0b[seg_0a[j]] (j < m_a);  seg_ab[k] = cluster_0a[seg_0b[k]] (k < m_b), seg_ab[m_b] = m_a
__global__ void link_derive_kernel(const int32_t* __restrict__ cl0a, const int32_t* __restrict__ seg0a, long ma,
                                   const int32_t* __restrict__ cl0b, const int32_t* __restrict__ seg0b, long mb,
                                   int32_t* __restrict__ cluster_ab, int32_t* __restrict__ seg_ab) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < ma) cluster_ab[t] = cl0b[seg0a[t]];
  if (t < mb) seg_ab[t] = cl0a[seg0b[t]];
  if (t == mb) seg_ab[mb] = (int32_t)ma;
}

// pooled level arrays from the first fine point of every cluster
__global__ void pool_gather_kernel(const int32_t* __restrict__ seg_start, long m, long n_fine, int pd,
                                   const int32_t* __restrict__ grid_f, const int32_t* __restrict__ batch_f,
                                   const int64_t* __restrict__ code_f /* (4,n_fine) */,
                                   int32_t* __restrict__ grid_c, int32_t* __restrict__ batch_c,
                                   int64_t* __restrict__ code_c /* (4,m) */) {
  long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const long h = seg_start[j];
  grid_c[3 * j + 0] = grid_f[3 * h + 0] >> pd;
  grid_c[3 * j + 1] = grid_f[3 * h + 1] >> pd;
  grid_c[3 * j + 2] = grid_f[3 * h + 2] >> pd;
  batch_c[j] = batch_f[h];
#pragma unroll
  for (int o = 0; o < 4; ++o) code_c[(long)o * m + j] = code_f[(long)o * n_fine + h] >> (3 * pd);
}

__global__ void gather_i32_kernel(const int32_t* __restrict__ src, const int32_t* __restrict__ idx, long n,
                                  int32_t* __restrict__ dst) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[idx[i]];
}

// neighbour table by binary search in the sorted (batch | z-order) codes.
// one thread per (point, offset); column a*k*k + b*k + c  <->  (dx,dy,dz) = (a-r, b-r, c-r)
__global__ void nbr_table_kernel(const int64_t* __restrict__ zc, const int32_t* __restrict__ grid,
                                 const int32_t* __restrict__ batch, long n, int depth, int ksize, int kmajor,
                                 int32_t* __restrict__ nbr) {
  const int kv = ksize * ksize * ksize;
  long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * kv) return;
  // offset-major output: a wave = one offset of 64 consecutive z-ordered points, whose neighbours are again close in
  // z-order, so the lanes' binary searches walk the same cache lines (and the stores coalesce)
  const long i = kmajor ? t % n : t / kv;
  const int o = kmajor ? (int)(t / n) : (int)(t - i * kv);
  const int r = ksize >> 1;
  const int a = o / (ksize * ksize), b = (o / ksize) % ksize, c = o % ksize;
  const int x = grid[3 * i + 0] + a - r, y = grid[3 * i + 1] + b - r, z = grid[3 * i + 2] + c - r;
  const int lim = 1 << depth;
  int res = -1;
  if (o == kv / 2) {
    res = (int)i;
  } else if (x >= 0 && y >= 0 && z >= 0 && x < lim && y < lim && z < lim) {
    const int64_t key = (int64_t)((((uint64_t)batch[i]) << (3 * depth)) | z_key((uint32_t)x, (uint32_t)y, (uint32_t)z, depth));
    long lo = 0, hi = n;  // lower_bound
    while (lo < hi) {
      long mid = (lo + hi) >> 1;
      if (zc[mid] < key) lo = mid + 1; else hi = mid;
    }
    if (lo < n && zc[lo] == key) res = (int)lo;
  }
  nbr[kmajor ? (long)o * n + i : t] = res;
}

// ---- kernel map from the parent level's map (pooling depth 1).  The target cell g + d (|d| <= ksize/2 <= 2) lies in
// one of the 27 parent cells around the point's own parent; if that parent cell is empty so is the target, otherwise
// the target is one of its <= 8 children, which are contiguous in z-order (one cache line of codes) and identified by
// the octant bits.  Replaces a log2(n)-deep binary search per (point, offset) by ~3 dependent, mostly cached reads.
__global__ void nbr_from_parent_kernel(const int64_t* __restrict__ zc, const int32_t* __restrict__ grid,
                                       const int32_t* __restrict__ cluster, const int32_t* __restrict__ pnbr /* (27,m) */,
                                       const int32_t* __restrict__ seg, long n, long m, int depth, int ksize, int kmajor,
                                       int32_t* __restrict__ nbr) {
  const int kv = ksize * ksize * ksize;
  long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * kv) return;
  const long i = kmajor ? t % n : t / kv;
  const int o = kmajor ? (int)(t / n) : (int)(t - i * kv);
  const int r = ksize >> 1;
  const int a = o / (ksize * ksize), b = (o / ksize) % ksize, c = o % ksize;
  const int gx = grid[3 * i], gy = grid[3 * i + 1], gz = grid[3 * i + 2];
  const int x = gx + a - r, y = gy + b - r, z = gz + c - r;
  const int lim = 1 << depth;
  int res = -1;
  if (o == kv / 2) {
    res = (int)i;
  } else if (x >= 0 && y >= 0 && z >= 0 && x < lim && y < lim && z < lim) {
    const int dx = (x >> 1) - (gx >> 1), dy = (y >> 1) - (gy >> 1), dz = (z >> 1) - (gz >> 1);
    const int par = pnbr[(long)((dx + 1) * 9 + (dy + 1) * 3 + (dz + 1)) * m + cluster[i]];
    if (par >= 0) {
      const int64_t oct = (int64_t)(((x & 1) << 2) | ((y & 1) << 1) | (z & 1));  // z-order: x -> bit 2, y -> 1, z -> 0
      const int e = seg[par + 1];
      for (int j = seg[par]; j < e; ++j) {
        const int64_t cj = zc[j] & 7;
        if (cj == oct) { res = j; break; }
        if (cj > oct) break;
      }
    }
  }
  nbr[kmajor ? (long)o * n + i : t] = res;
}

// The same with the parents' child_info words (first child row << 8 | octant occupancy, cdseg_child_info): the target
// is first + popcount(occupancy below its octant) - two dependent reads per (point, offset), no scan of the children
__global__ void nbr_from_info_kernel(const int32_t* __restrict__ grid, const int32_t* __restrict__ cluster,
                                     const int32_t* __restrict__ pnbr /* (27,m) */, const int64_t* __restrict__ cinfo,
                                     long n, long m, int depth, int ksize, int kmajor, int32_t* __restrict__ nbr) {
  const int kv = ksize * ksize * ksize;
  long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * kv) return;
  const long i = kmajor ? t % n : t / kv;
  const int o = kmajor ? (int)(t / n) : (int)(t - i * kv);
  const int r = ksize >> 1;
  const int a = o / (ksize * ksize), b = (o / ksize) % ksize, c = o % ksize;
  const int gx = grid[3 * i], gy = grid[3 * i + 1], gz = grid[3 * i + 2];
  const int x = gx + a - r, y = gy + b - r, z = gz + c - r;
  const int lim = 1 << depth;
  int res = -1;
  if (o == kv / 2) {
    res = (int)i;
  } else if (x >= 0 && y >= 0 && z >= 0 && x < lim && y < lim && z < lim) {
    const int dx = (x >> 1) - (gx >> 1), dy = (y >> 1) - (gy >> 1), dz = (z >> 1) - (gz >> 1);
    const int par = pnbr[(long)((dx + 1) * 9 + (dy + 1) * 3 + (dz + 1)) * m + cluster[i]];
    if (par >= 0) {
      const int64_t info = cinfo[par];
      const int occ = (int)(info & 255), oct = ((x & 1) << 2) | ((y & 1) << 1) | (z & 1);
      if ((occ >> oct) & 1) res = (int)(info >> 8) + __popc(occ & ((1 << oct) - 1));
    }
  }
  nbr[kmajor ? (long)o * n + i : t] = res;
}

// k = 3, offset-major output: ONE thread per point.  Along an axis the targets g - 1, g, g + 1 fall into only two of the
// three parent cells around the point's parent (which two depends on the parity of g), so a point touches 8 parent cells,
// not 27: 8 map reads + 8 child_info reads produce all 27 entries, the point's grid / cluster words are read once, the 27
// stores are coalesced across threads (row i of every offset), and there is no 64-bit division per entry (the per-entry
// form above spent 127 us on the 960k-point level of an 8-scene batch: 0.8 TB/s of its output).
__global__ __launch_bounds__(256) void nbr3_from_info_point_kernel(const int32_t* __restrict__ grid, const int32_t* __restrict__ cluster,
                                                                   const int32_t* __restrict__ pnbr /* (27,m) */,
                                                                   const int64_t* __restrict__ cinfo, long n, long m, int depth,
                                                                   int32_t* __restrict__ nbr /* (27,n) */) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int gx = grid[3 * i], gy = grid[3 * i + 1], gz = grid[3 * i + 2];
  const int cl = cluster[i];
  const int lim = 1 << depth;
  // per axis: parent offset of the target at +-1 in the direction that leaves the parent cell (the other two stay inside)
  const int px = (gx & 1) ? 1 : -1, py = (gy & 1) ? 1 : -1, pz = (gz & 1) ? 1 : -1;
  int64_t info[8];  // parent cells (ax, ay, az) with a. in {0 = own, 1 = the neighbour}
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int dx = (q & 4) ? px : 0, dy = (q & 2) ? py : 0, dz = (q & 1) ? pz : 0;
    const int par = pnbr[(long)((dx + 1) * 9 + (dy + 1) * 3 + (dz + 1)) * m + cl];
    info[q] = par >= 0 ? cinfo[par] : 0;  // occupancy 0: no children
  }
#pragma unroll
  for (int o = 0; o < 27; ++o) {
    const int a = o / 9, b = (o / 3) % 3, c = o % 3;
    const int x = gx + a - 1, y = gy + b - 1, z = gz + c - 1;
    int res = -1;
    if (o == 13) {
      res = (int)i;
    } else if (x >= 0 && y >= 0 && z >= 0 && x < lim && y < lim && z < lim) {
      // the target leaves the parent cell along an axis iff it moved in that axis' "outward" direction
      const int q = (((x >> 1) != (gx >> 1)) ? 4 : 0) | (((y >> 1) != (gy >> 1)) ? 2 : 0) | (((z >> 1) != (gz >> 1)) ? 1 : 0);
      const int64_t w = info[q];
      const int occ = (int)(w & 255), oct = ((x & 1) << 2) | ((y & 1) << 1) | (z & 1);
      if ((occ >> oct) & 1) res = (int)(w >> 8) + __popc(occ & ((1 << oct) - 1));
    }
    nbr[(long)o * n + i] = res;
  }
}

// attention slot plan (ptv3.py:188-244 in scatter form).  For padded slot p of batch element b:
//   local < n_b  : rank = local                       (real slot, its output is kept)
//   local >= n_b : rank = local - K                   (borrowed from the previous patch's tail)
// gidx[p] = order[offs[b] + rank] (order == nullptr -> identity), widx[p] = real ? gidx[p] : -1
__global__ void pad_plan_kernel(const int32_t* __restrict__ order, const int32_t* __restrict__ offs,
                                const int32_t* __restrict__ offs_pad, int nb, int K, long n_pad,
                                int32_t* __restrict__ gidx, int32_t* __restrict__ widx) {
  long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pad) return;
  int lo = 0, hi = nb - 1;  // first b with offs_pad[b+1] > p
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if (offs_pad[mid + 1] > p) hi = mid; else lo = mid + 1;
  }
  const int b = lo;
  const int local = (int)(p - offs_pad[b]);
  const int nbp = offs[b + 1] - offs[b];
  const bool real = local < nbp;
  const int rank = offs[b] + (real ? local : local - K);
  const int g = order ? order[rank] : rank;
  gidx[p] = g;
  widx[p] = real ? g : -1;
}

// all slot plans of a scene (every level x curve x patch size) in one launch
struct PadBatchP {
  const int32_t* order[CDSEG_PAD_BATCH_MAX];
  const int32_t* offs[CDSEG_PAD_BATCH_MAX];
  const int32_t* offs_pad[CDSEG_PAD_BATCH_MAX];
  int K[CDSEG_PAD_BATCH_MAX];
  long start[CDSEG_PAD_BATCH_MAX + 1];  // prefix sums of n_pad = offsets into gidx / widx
  int count, nb;
};

__global__ void pad_plan_batch_kernel(PadBatchP b, int32_t* __restrict__ gidx, int32_t* __restrict__ widx) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= b.start[b.count]) return;
  int j = 0;
  while (j + 1 < b.count && b.start[j + 1] <= t) ++j;
  const long p = t - b.start[j];
  const int32_t* offs = b.offs[j];
  const int32_t* offs_pad = b.offs_pad[j];
  int lo = 0, hi = b.nb - 1;  // first batch element with offs_pad[e+1] > p
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if (offs_pad[mid + 1] > p) hi = mid; else lo = mid + 1;
  }
  const int local = (int)(p - offs_pad[lo]);
  const bool real = local < offs[lo + 1] - offs[lo];
  const int rank = offs[lo] + (real ? local : local - b.K[j]);
  const int g = b.order[j] ? b.order[j][rank] : rank;
  gidx[t] = g;
  widx[t] = real ? g : -1;
}

// slot plan of a collated batch whose elements read DIFFERENT curves: padded slot s of batch element b takes its entry
// from the slot plan of curve choice[b] (all sources are slot plans of the same level and patch key, so slot s means the
// same position in each).  The choices travel in the launch arguments; plain 4-byte accesses (the sources are arena views)
struct SlotsSelectP {
  const int32_t* g[4];
  const int32_t* w[4];
  unsigned char choice[CDSEG_SLOTS_SELECT_MAX];
  int nb;
};

__global__ void slots_select_kernel(SlotsSelectP p, const int32_t* __restrict__ offs_pad, long n_pad,
                                    int32_t* __restrict__ gidx, int32_t* __restrict__ widx) {
  const long s = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_pad) return;
  int lo = 0, hi = p.nb - 1;  // first batch element with offs_pad[e+1] > s
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if (offs_pad[mid + 1] > s) hi = mid; else lo = mid + 1;
  }
  const int c = p.choice[lo];
  const int32_t* g = c == 0 ? p.g[0] : c == 1 ? p.g[1] : c == 2 ? p.g[2] : p.g[3];
  const int32_t* w = c == 0 ? p.w[0] : c == 1 ? p.w[1] : c == 2 ? p.w[2] : p.w[3];
  gidx[s] = g[s];
  widx[s] = w[s];
}

inline dim3 grid1d(long n, int bs = 256) { return dim3((unsigned)((n + bs - 1) / bs)); }

}  // namespace

extern "C" {

int cdseg_grid_max(const void* grid, int elem_bytes, long n3, int64_t* out_dev, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(out_dev, 0, sizeof(int64_t), s) != hipSuccess) return CDSEG_ERR_LAUNCH;
  if (n3 <= 0) return CDSEG_OK;
  int blocks = (int)((n3 + 255) / 256);
  if (blocks > 128) blocks = 128;
  if (elem_bytes == 8)
    hipLaunchKernelGGL(grid_max_kernel<int64_t>, dim3(blocks), dim3(256), 0, s, (const int64_t*)grid, n3,
                       (unsigned long long*)out_dev);
  else if (elem_bytes == 4)
    hipLaunchKernelGGL(grid_max_kernel<int32_t>, dim3(blocks), dim3(256), 0, s, (const int32_t*)grid, n3,
                       (unsigned long long*)out_dev);
  else
    return CDSEG_ERR_ARG;
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_offset2batch(const int64_t* offset, int nb, long n, int32_t* batch, void* stream) {
  if (n <= 0) return CDSEG_OK;
  if (nb <= 0) return CDSEG_ERR_ARG;
  hipLaunchKernelGGL(offset2batch_kernel, grid1d(n), dim3(256), 0, (hipStream_t)stream, offset, nb, n, batch);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_encode(const void* grid, int grid_elem_bytes, const void* batch, int batch_elem_bytes, long n, int depth,
                 int order_id, int64_t* code, void* stream) {
  if (n <= 0) return CDSEG_OK;
  if (depth < 0 || depth > 16 || order_id < 0 || order_id > 3) return CDSEG_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (batch == nullptr) batch_elem_bytes = 8;
#define LAUNCH_ENC(G, B)                                                                                       \
  hipLaunchKernelGGL((encode_kernel<G, B>), grid1d(n), dim3(256), 0, s, (const G*)grid, (const B*)batch, n, depth, \
                     order_id, code)
  if (grid_elem_bytes == 8 && batch_elem_bytes == 8) LAUNCH_ENC(int64_t, int64_t);
  else if (grid_elem_bytes == 8 && batch_elem_bytes == 4) LAUNCH_ENC(int64_t, int32_t);
  else if (grid_elem_bytes == 4 && batch_elem_bytes == 8) LAUNCH_ENC(int32_t, int64_t);
  else if (grid_elem_bytes == 4 && batch_elem_bytes == 4) LAUNCH_ENC(int32_t, int32_t);
  else return CDSEG_ERR_ARG;
#undef LAUNCH_ENC
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_encode4(const int32_t* grid, const int32_t* batch, long n, int depth, int64_t* code4, void* stream) {
  if (n <= 0) return CDSEG_OK;
  if (depth < 0 || depth > 16) return CDSEG_ERR_ARG;
  hipLaunchKernelGGL(encode4_kernel, grid1d(n), dim3(256), 0, (hipStream_t)stream, grid, batch, n, depth, code4);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

// rocPRIM's default switches to merge sort (block sort + ~13 merge passes at 864 k keys) up to 1 M items; these keys have
// 30-40 significant bits, i.e. 4-5 Onesweep passes: merge sort only where it wins (a few block-sort tiles)
using SortConfig = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config, rocprim::default_config,
                                              CDSEG_MERGE_SORT_LIMIT>;

size_t cdseg_sort_ws_bytes(long n) {
  size_t bytes = 0;
  (void)rocprim::radix_sort_pairs<SortConfig>(nullptr, bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                              (const int32_t*)nullptr, (int32_t*)nullptr, (size_t)n, 0u, 64u,
                                              (hipStream_t)0, false);
  size_t scan_bytes = 0;
  (void)rocprim::inclusive_scan(nullptr, scan_bytes, (const int32_t*)nullptr, (int32_t*)nullptr, (size_t)n,
                          rocprim::plus<int32_t>(), (hipStream_t)0, false);
  if (scan_bytes > bytes) bytes = scan_bytes;
  // + room for an iota value array and a flag / scan pair used by the callers below
  return bytes + 3 * (size_t)n * sizeof(int32_t) + 1024;
}

// keys are non-negative int64 codes; vals_in == nullptr -> iota.  Stable LSD radix sort (rocPRIM).
int cdseg_sort_pairs(const int64_t* keys_in, int64_t* keys_out, const int32_t* vals_in, int32_t* vals_out, long n,
                     int end_bit, void* ws, size_t ws_bytes, void* stream) {
  if (n <= 0) return CDSEG_OK;
  hipStream_t s = (hipStream_t)stream;
  if (end_bit <= 0 || end_bit > 64) end_bit = 64;
  char* w = (char*)ws;
  size_t need = cdseg_sort_ws_bytes(n);
  if (ws_bytes < need) return CDSEG_ERR_WORKSPACE;
  const int32_t* vin = vals_in;
  size_t off = 0;
  if (!vin) {
    int32_t* io = (int32_t*)w;
    hipLaunchKernelGGL(iota_kernel, grid1d(n), dim3(256), 0, s, io, n);
    vin = io;
    off = (((size_t)n * sizeof(int32_t)) + 255) & ~(size_t)255;
  }
  size_t tmp_bytes = ws_bytes - off;
  hipError_t e = rocprim::radix_sort_pairs<SortConfig>(w + off, tmp_bytes, (const uint64_t*)keys_in, (uint64_t*)keys_out,
                                                       vin, vals_out, (size_t)n, 0u, (unsigned)end_bit, s, false);
  if (e != hipSuccess) return CDSEG_ERR_LAUNCH;
  return CDSEG_OK;
}

// Orders of `count` (<= 4) curves of the same points with ONE radix sort: codes (4, n) int64 (row r = curve r), rows[count]
// the curve rows wanted, orders (count, n) int32 out.  The keys carry the slot in the bits above end_bit, so the sorted
// array is the concatenation of the per-curve orders (Onesweep's cost is mostly fixed: 3 sorts of 864 k keys 480 us,
// one of 2.6 M keys ~ 200 us).  ws: cdseg_sort_curves_ws_bytes(n, count).
size_t cdseg_sort_curves_ws_bytes(long n, int count) {
  const size_t total = (size_t)n * (size_t)(count > 0 ? count : 1);
  return cdseg_sort_ws_bytes((long)total) + 2 * total * sizeof(uint64_t) + total * sizeof(int32_t) + 4096;
}

int cdseg_sort_curves(const int64_t* codes, const int* rows_host, int count, long n, int end_bit, int32_t* orders, void* ws,
                      size_t ws_bytes, void* stream) {
  if (n <= 0 || count <= 0) return CDSEG_OK;
  if (!codes || !rows_host || !orders || !ws || count > 4 || end_bit <= 0 || end_bit + 2 > 64) return CDSEG_ERR_ARG;
  if (ws_bytes < cdseg_sort_curves_ws_bytes(n, count)) return CDSEG_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const size_t total = (size_t)n * count;
  char* w = (char*)ws;
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  uint64_t* kin = (uint64_t*)w;
  uint64_t* kout = (uint64_t*)(w + al(total * 8));
  int32_t* vin = (int32_t*)(w + 2 * al(total * 8));
  char* tmp = w + 2 * al(total * 8) + al(total * 4);
  size_t tmp_bytes = ws_bytes - (size_t)(tmp - w);
  CurveRows rows4 = {{0, 0, 0, 0}};
  for (int c = 0; c < count; ++c) {
    if (rows_host[c] < 0 || rows_host[c] > 3) return CDSEG_ERR_ARG;
    rows4.r[c] = rows_host[c];
  }
  hipLaunchKernelGGL(tag_keys_kernel, grid1d((long)total), dim3(256), 0, s, codes, rows4, count, n, end_bit, kin, vin);
  hipError_t e = rocprim::radix_sort_pairs<SortConfig>(tmp, tmp_bytes, kin, kout, vin, orders, total, 0u,
                                                       (unsigned)(end_bit + 2), s, false);
  if (e != hipSuccess) return CDSEG_ERR_LAUNCH;
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_invert_perm(const int32_t* perm, long n, int32_t* inv, void* stream) {
  if (n <= 0) return CDSEG_OK;
  hipLaunchKernelGGL(invert_perm_kernel, grid1d(n), dim3(256), 0, (hipStream_t)stream, perm, n, inv);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_widen_i32(const int32_t* src, long n, int64_t* dst, void* stream) {
  if (n <= 0) return CDSEG_OK;
  hipLaunchKernelGGL(widen_kernel, grid1d(n), dim3(256), 0, (hipStream_t)stream, src, n, dst);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_gather_rows(const void* src, const int32_t* idx, long n_out, int row_bytes, void* dst, void* stream) {
  if (n_out <= 0) return CDSEG_OK;
  if (row_bytes <= 0 || (row_bytes & 3)) return CDSEG_ERR_ARG;
  const int rw = row_bytes / 4;
  hipLaunchKernelGGL(gather_rows_kernel, grid1d(n_out * rw), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)src,
                     idx, n_out, rw, (uint32_t*)dst);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_scatter_rows(const void* src, const int32_t* idx, long n_in, int row_bytes, void* dst, void* stream) {
  if (n_in <= 0) return CDSEG_OK;
  if (row_bytes <= 0 || (row_bytes & 3)) return CDSEG_ERR_ARG;
  const int rw = row_bytes / 4;
  hipLaunchKernelGGL(scatter_rows_kernel, grid1d(n_in * rw), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)src,
                     idx, n_in, rw, (uint32_t*)dst);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_gather_i32(const int32_t* src, const int32_t* idx, long n, int32_t* dst, void* stream) {
  if (n <= 0) return CDSEG_OK;
  hipLaunchKernelGGL(gather_i32_kernel, grid1d(n), dim3(256), 0, (hipStream_t)stream, src, idx, n, dst);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_plan_gather_grid(const void* grid, int grid_elem_bytes, const int32_t* perm, const int64_t* zcode_sorted,
                           long n, int depth, int32_t* grid_out, int32_t* batch_out, void* stream) {
  if (n <= 0) return CDSEG_OK;
  hipStream_t s = (hipStream_t)stream;
  if (grid_elem_bytes == 8)
    hipLaunchKernelGGL(gather_grid_kernel<int64_t>, grid1d(n), dim3(256), 0, s, (const int64_t*)grid, perm,
                       zcode_sorted, n, depth, grid_out, batch_out);
  else if (grid_elem_bytes == 4)
    hipLaunchKernelGGL(gather_grid_kernel<int32_t>, grid1d(n), dim3(256), 0, s, (const int32_t*)grid, perm,
                       zcode_sorted, n, depth, grid_out, batch_out);
  else
    return CDSEG_ERR_ARG;
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

// One pooling level over the z-sorted codes: cluster id per fine point, run starts, count.
// shift = 3 * pooling_depth bits.  ws: >= cdseg_sort_ws_bytes(n).
int cdseg_pool_level(const int64_t* zcode_sorted, long n, int shift, int32_t* cluster, int32_t* seg_start,
                     int32_t* count_dev, void* ws, size_t ws_bytes, void* stream) {
  if (n <= 0) return CDSEG_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (ws_bytes < cdseg_sort_ws_bytes(n)) return CDSEG_ERR_WORKSPACE;
  char* w = (char*)ws;
  const size_t arr = (((size_t)n * sizeof(int32_t)) + 255) & ~(size_t)255;
  int32_t* flag = (int32_t*)w;
  int32_t* incl = (int32_t*)(w + arr);
  char* tmp = w + 2 * arr;
  size_t tmp_bytes = ws_bytes - 2 * arr;
  hipLaunchKernelGGL(level_flag_kernel, grid1d(n), dim3(256), 0, s, zcode_sorted, n, shift, flag);
  hipError_t e = rocprim::inclusive_scan(tmp, tmp_bytes, (const int32_t*)flag, incl, (size_t)n,
                                         rocprim::plus<int32_t>(), s, false);
  if (e != hipSuccess) return CDSEG_ERR_LAUNCH;
  hipLaunchKernelGGL(level_finish_kernel, grid1d(n), dim3(256), 0, s, incl, flag, n, cluster, seg_start, count_dev);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

size_t cdseg_coarse_orders_ws_bytes(long n0, int nlev, int ncurve) {
  const size_t total = (size_t)n0 * nlev * ncurve;
  size_t scan_bytes = 0;
  (void)rocprim::inclusive_scan(nullptr, scan_bytes, (const int32_t*)nullptr, (int32_t*)nullptr, total,
                                rocprim::plus<int32_t>(), (hipStream_t)0, false);
  return 2 * ((total * sizeof(int32_t) + 255) & ~(size_t)255) + scan_bytes + 1024;
}

// clusters: nlev device pointers (fine point -> cluster id of level l); orders: ncurve device pointers (rank -> fine
// point); out: int32, level l / curve c at offset ncurve * sum_{l' < l} m_l' + c * m_l.
int cdseg_coarse_orders(const int32_t* const* clusters, int nlev, const int32_t* const* orders, int ncurve, long n0,
                        int32_t* out, void* ws, size_t ws_bytes, void* stream) {
  if (n0 <= 0 || nlev <= 0 || ncurve <= 0) return CDSEG_OK;
  if (nlev > 8 || ncurve > 3 || !clusters || !orders || !out) return CDSEG_ERR_ARG;
  if (ws_bytes < cdseg_coarse_orders_ws_bytes(n0, nlev, ncurve)) return CDSEG_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  CoarseP p;
  for (int l = 0; l < 8; ++l) p.cluster[l] = l < nlev ? clusters[l] : nullptr;
  for (int c = 0; c < 3; ++c) p.order[c] = c < ncurve ? orders[c] : nullptr;
  p.n0 = n0; p.nlev = nlev; p.ncurve = ncurve;
  const long total = n0 * nlev * ncurve;
  char* w = (char*)ws;
  const size_t arr = (((size_t)total * sizeof(int32_t)) + 255) & ~(size_t)255;
  int32_t* flag = (int32_t*)w;
  int32_t* pos = (int32_t*)(w + arr);
  hipLaunchKernelGGL(coarse_flag_kernel, grid1d(total), dim3(256), 0, s, p, total, flag);
  size_t scan_bytes = ws_bytes - 2 * arr;
  hipError_t e = rocprim::inclusive_scan((void*)(w + 2 * arr), scan_bytes, (const int32_t*)flag, pos, (size_t)total,
                                         rocprim::plus<int32_t>(), s, false);
  if (e != hipSuccess) return CDSEG_ERR_LAUNCH;
  hipLaunchKernelGGL(coarse_compact_kernel, grid1d(total), dim3(256), 0, s, p, total, pos, out);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

size_t cdseg_pool_levels_ws_bytes(long n, int nlev) {
  const size_t total = (size_t)n * nlev;
  size_t scan_bytes = 0;
  (void)rocprim::inclusive_scan(nullptr, scan_bytes, (const int32_t*)nullptr, (int32_t*)nullptr, total,
                                rocprim::plus<int32_t>(), (hipStream_t)0, false);
  return 2 * ((total * sizeof(int32_t) + 255) & ~(size_t)255) + scan_bytes + 1024;
}

// All pooling levels over the z-sorted level-0 codes in one pass.  shifts (host, nlev <= 8): 3 * cumulative pooling
// depth per level; last_idx (nb, device): index of the last point of every batch element.
// cluster (nlev, n), seg_start (nlev, n + 1), meta nlev * (1 + nb) + 1 int32 = [count, cluster of last_idx[b] ...] per
// level, then the number of duplicate (batch, voxel) codes.
int cdseg_pool_levels(const int64_t* zcode_sorted, long n, const int* shifts, int nlev, const int32_t* last_idx, int nb,
                      int32_t* cluster, int32_t* seg_start, int32_t* meta, void* ws, size_t ws_bytes, void* stream) {
  if (n <= 0 || nlev <= 0) return CDSEG_ERR_ARG;
  if (nlev > 8 || nb <= 0 || !shifts || !last_idx) return CDSEG_ERR_ARG;
  if (ws_bytes < cdseg_pool_levels_ws_bytes(n, nlev)) return CDSEG_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  LevelsP p;
  for (int l = 0; l < 8; ++l) p.shift[l] = l < nlev ? shifts[l] : 0;
  p.nlev = nlev; p.nb = nb; p.n = n;
  const long total = n * nlev;
  char* w = (char*)ws;
  const size_t arr = (((size_t)total * sizeof(int32_t)) + 255) & ~(size_t)255;
  int32_t* flag = (int32_t*)w;
  int32_t* incl = (int32_t*)(w + arr);
  size_t scan_bytes = ws_bytes - 2 * arr;
  hipLaunchKernelGGL(levels_flag_kernel, grid1d(total), dim3(256), 0, s, zcode_sorted, p, flag, meta);
  hipError_t e = rocprim::inclusive_scan((void*)(w + 2 * arr), scan_bytes, (const int32_t*)flag, incl, (size_t)total,
                                         rocprim::plus<int32_t>(), s, false);
  if (e != hipSuccess) return CDSEG_ERR_LAUNCH;
  hipLaunchKernelGGL(levels_finish_kernel, grid1d(total), dim3(256), 0, s, zcode_sorted, incl, flag, p, last_idx, cluster,
                     seg_start, meta);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_link_derive(const int32_t* cluster_0a, const int32_t* seg_0a, long ma, const int32_t* cluster_0b,
                      const int32_t* seg_0b, long mb, int32_t* cluster_ab, int32_t* seg_ab, void* stream) {
  if (ma <= 0 || mb <= 0) return CDSEG_ERR_ARG;
  const long t = (ma > mb + 1 ? ma : mb + 1);
  hipLaunchKernelGGL(link_derive_kernel, grid1d(t), dim3(256), 0, (hipStream_t)stream, cluster_0a, seg_0a, ma,
                     cluster_0b, seg_0b, mb, cluster_ab, seg_ab);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_pool_gather(const int32_t* seg_start, long m, long n_fine, int pooling_depth, const int32_t* grid_f,
                      const int32_t* batch_f, const int64_t* code4_f, int32_t* grid_c, int32_t* batch_c,
                      int64_t* code4_c, void* stream) {
  if (m <= 0) return CDSEG_OK;
  hipLaunchKernelGGL(pool_gather_kernel, grid1d(m), dim3(256), 0, (hipStream_t)stream, seg_start, m, n_fine,
                     pooling_depth, grid_f, batch_f, code4_f, grid_c, batch_c, code4_c);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_nbr_table(const int64_t* zcode_sorted, const int32_t* grid, const int32_t* batch, long n, int depth,
                    int ksize, int kmajor, int32_t* nbr, void* stream) {
  if (n <= 0) return CDSEG_OK;
  if (ksize != 3 && ksize != 5) return CDSEG_ERR_ARG;
  const long total = n * ksize * ksize * ksize;
  hipLaunchKernelGGL(nbr_table_kernel, grid1d(total), dim3(256), 0, (hipStream_t)stream, zcode_sorted, grid, batch, n,
                     depth, ksize, kmajor, nbr);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

// Same table as cdseg_nbr_table, derived from the parent level (pooling depth 1): cluster (n) fine point -> parent,
// parent_nbr3 (27, m) OFFSET-MAJOR 3x3x3 map of the parent level, seg_start (m + 1) children runs.
int cdseg_nbr_table_from_parent(const int64_t* zcode_sorted, const int32_t* grid, const int32_t* cluster,
                                const int32_t* parent_nbr3, const int32_t* seg_start, long n, long m, int depth, int ksize,
                                int kmajor, int32_t* nbr, void* stream) {
  if (n <= 0) return CDSEG_OK;
  if ((ksize != 3 && ksize != 5) || m <= 0) return CDSEG_ERR_ARG;
  const long total = n * ksize * ksize * ksize;
  hipLaunchKernelGGL(nbr_from_parent_kernel, grid1d(total), dim3(256), 0, (hipStream_t)stream, zcode_sorted, grid,
                     cluster, parent_nbr3, seg_start, n, m, depth, ksize, kmajor, nbr);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_nbr_table_from_info(const int32_t* grid, const int32_t* cluster, const int32_t* parent_nbr3,
                              const int64_t* child_info, long n, long m, int depth, int ksize, int kmajor, int32_t* nbr,
                              void* stream) {
  if (!grid || !cluster || !parent_nbr3 || !child_info || !nbr) return CDSEG_ERR_ARG;
  if (n <= 0) return CDSEG_OK;
  if ((ksize != 3 && ksize != 5) || m <= 0) return CDSEG_ERR_ARG;
  const long total = n * ksize * ksize * ksize;
  if (ksize == 3 && kmajor) {
    hipLaunchKernelGGL(nbr3_from_info_point_kernel, grid1d(n), dim3(256), 0, (hipStream_t)stream, grid, cluster, parent_nbr3,
                       child_info, n, m, depth, nbr);
  } else {
    hipLaunchKernelGGL(nbr_from_info_kernel, grid1d(total), dim3(256), 0, (hipStream_t)stream, grid, cluster, parent_nbr3,
                       child_info, n, m, depth, ksize, kmajor, nbr);
  }
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

int cdseg_pad_plan(const int32_t* order, const int32_t* offs, const int32_t* offs_pad, int nb, int patch, long n_pad,
                   int32_t* gidx, int32_t* widx, void* stream) {
  if (n_pad <= 0) return CDSEG_OK;
  if (nb <= 0 || patch <= 0) return CDSEG_ERR_ARG;
  hipLaunchKernelGGL(pad_plan_kernel, grid1d(n_pad), dim3(256), 0, (hipStream_t)stream, order, offs, offs_pad, nb,
                     patch, n_pad, gidx, widx);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

// count (<= CDSEG_PAD_BATCH_MAX) slot plans at once: plan j uses orders[j] (NULL = identity), offs[j], offs_pad[j],
// patch[j], n_pad[j]; its gidx / widx start at sum_{i<j} n_pad[i] of the output arrays.
int cdseg_pad_plan_batch(int count, const int32_t* const* orders, const int32_t* const* offs,
                         const int32_t* const* offs_pad, const int* patch, const long* n_pad, int nb, int32_t* gidx,
                         int32_t* widx, void* stream) {
  if (count <= 0) return CDSEG_OK;
  if (count > CDSEG_PAD_BATCH_MAX || nb <= 0) return CDSEG_ERR_ARG;
  PadBatchP b;
  b.count = count;
  b.nb = nb;
  b.start[0] = 0;
  for (int j = 0; j < count; ++j) {
    if (patch[j] <= 0 || n_pad[j] < 0) return CDSEG_ERR_ARG;
    b.order[j] = orders[j]; b.offs[j] = offs[j]; b.offs_pad[j] = offs_pad[j]; b.K[j] = patch[j];
    b.start[j + 1] = b.start[j] + n_pad[j];
  }
  if (b.start[count] == 0) return CDSEG_OK;
  hipLaunchKernelGGL(pad_plan_batch_kernel, grid1d(b.start[count]), dim3(256), 0, (hipStream_t)stream, b, gidx, widx);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

// out[s] = src[choice[b(s)]][s] for every padded slot s of batch element b: the slot plan of a collated batch whose
// elements read different curves, composed from the per-curve slot plans of one level and patch key.
int cdseg_slots_select(const int32_t* const* gidx_src, const int32_t* const* widx_src, int nsrc, const int32_t* offs_pad,
                       int nb, const unsigned char* choice_host, long n_pad, int32_t* gidx, int32_t* widx, void* stream) {
  if (!gidx_src || !widx_src || !choice_host || nsrc < 1 || nsrc > 4 || nb <= 0 || n_pad < 0) return CDSEG_ERR_ARG;
  if (nb > CDSEG_SLOTS_SELECT_MAX) return CDSEG_ERR_UNSUPPORTED;
  SlotsSelectP p;
  for (int c = 0; c < 4; ++c) {
    p.g[c] = c < nsrc ? gidx_src[c] : nullptr;
    p.w[c] = c < nsrc ? widx_src[c] : nullptr;
  }
  for (int b = 0; b < CDSEG_SLOTS_SELECT_MAX; ++b) p.choice[b] = 0;
  for (int b = 0; b < nb; ++b) {
    const int c = choice_host[b];
    if (c >= nsrc || !p.g[c] || !p.w[c]) return CDSEG_ERR_ARG;  // a chosen source must exist
    p.choice[b] = (unsigned char)c;
  }
  p.nb = nb;
  if (n_pad == 0) return CDSEG_OK;
  if (!offs_pad || !gidx || !widx) return CDSEG_ERR_ARG;
  hipLaunchKernelGGL(slots_select_kernel, grid1d(n_pad), dim3(256), 0, (hipStream_t)stream, p, offs_pad, n_pad, gidx, widx);
  CDSEG_CHECK_LAUNCH();
  return CDSEG_OK;
}

}  // extern "C"
