// Per-channel fp64 sums over the rows of a (rows, c) tensor in an order fixed by the shape, no atomics: the ONE skeleton under
// the reductions of csrc/norm.hip (BatchNorm statistics and backward sums), csrc/fusion.hip (the gate's backward) and
// csrc/skip.hip (the skip statistics).  Each of them keeps its row loop, its arithmetic and its parameter struct.
//
// The order of a sum of NS quantities per channel:
//   1. partition(rows, min_rows): block b owns the rows [b rows_per_block, (b + 1) rows_per_block) - at most 256 blocks;
//   2. RowMap: a row is covered by L = c / 4 lanes of 16 bytes, a 256-thread block holds R = 256 / L rows at a time (threads
//      beyond R L idle: only where L does not divide 256, c = 48 ..); a thread keeps ONE column group for its lifetime and adds
//      its rows row0 + r, row0 + r + R, .. by ascending index (the kernel's own loop);
//   3. block_fold<NS>: the R row slots of a block are added by ascending slot through LDS -> ws[block][NS c]
//      (the scalar paths write ws[block][NS c] themselves, one thread adding a column's rows by ascending index);
//   4. reduce_kernel<SEGS>, a second launch, adds the block partials: SEGS = 1 by ascending block index in one chain; SEGS = 16
//      by ascending block index inside each of 16 segments of ceil(blocks / 16) consecutive blocks, then the segment sums by
//      ascending segment.  The two give different bits: an op states its SEGS once and keeps it.
// Every sum is therefore a function of (rows, c), the path and the data alone.
// The host part is plain C++ (no HIP, no device query); tools/host_checks/colsum_partition_main.cpp compiles it on its own
// under the address / undefined-behaviour sanitizers.
#ifndef CDSEG_COLSUM_H
#define CDSEG_COLSUM_H
#include <cstddef>
#include <cstdint>

namespace colsum {

constexpr int THREADS = 256;      // block size of every kernel on the thread map
constexpr int MAX_C = 512;        // widest row
constexpr long MAX_BLOCKS = 256;  // block partials at most: what the second launch adds per output
constexpr long MIN_ROWS_BN = 256;    // rows of a block at least: BatchNorm (m = 5003 -> 20 blocks),
constexpr long MIN_ROWS_SWEEP = 64;  // the gate and the skip statistics (the bottleneck of one scene: ~2 k rows -> 32 blocks)

struct Partition {
  long rows_per_block;  // min_rows, or a multiple of 64 beyond it (the last block may be shorter)
  int blocks;           // no empty block; 0 for rows <= 0
};

inline Partition partition(long rows, long min_rows) {
  long rpb = (rows + MAX_BLOCKS - 1) / MAX_BLOCKS;
  rpb = rpb < min_rows ? min_rows : (rpb + 63) / 64 * 64;
  return {rpb, rows > 0 ? (int)((rows + rpb - 1) / rpb) : 0};
}

// the workspace of steps 3 and 4: blocks x nsums x c doubles
inline size_t ws_bytes(long rows, int nsums, int c, long min_rows) {
  if (rows <= 0 || nsums <= 0 || c <= 0) return 0;
  return (size_t)partition(rows, min_rows).blocks * (size_t)nsums * (size_t)c * sizeof(double);
}

// c = multiple, 2 multiple, .. up to MAX_C (multiple 1: any width from 1)
inline bool width_ok(int c, int multiple) { return c >= multiple && c <= MAX_C && c % multiple == 0; }

// every pointer (NULL included) on a (mask + 1)-byte boundary
template <typename... P>
inline bool aligned(uintptr_t mask, const P*... ptr) { return ((((uintptr_t)ptr) | ...) & mask) == 0; }

// a row stride that covers the row and keeps 16-byte lanes aligned
inline bool ld_ok(int ld, int c) { return ld >= c && (ld & 3) == 0; }

// grid of a grid-strided sweep over `total` items, about `per_thread` a thread, 1 .. max_grid blocks
inline unsigned elem_grid(long total, long per_thread, long max_grid) {
  const long blocks = (total + THREADS * per_thread - 1) / (THREADS * per_thread);
  return (unsigned)(blocks < 1 ? 1 : (blocks > max_grid ? max_grid : blocks));
}

// the same over rows on the thread map: a block holds R = 256 / (c / 4) rows at a time
inline unsigned row_grid(long rows, int c, int rows_per_thread, long max_grid) {
  const long per_block = (long)(THREADS / (c >> 2)) * rows_per_thread;
  const long blocks = (rows + per_block - 1) / per_block;
  return (unsigned)(blocks < 1 ? 1 : (blocks > max_grid ? max_grid : blocks));
}

}  // namespace colsum

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace colsum {

// Step 2.  c a multiple of 4; the thread's columns are 4 l .. 4 l + 3.
struct RowMap {
  int L, R, r, l;
  bool active;  // r < R
  __device__ explicit RowMap(int c)
      : L(c >> 2), R(THREADS / L), r((int)threadIdx.x / L), l((int)threadIdx.x - r * L), active(r < R) {}
};

// Step 3.  acc[s][e]: the thread's sum s of column 4 l + e (idle threads pass anything: they only reach the barrier).
template <int NS>
__device__ __forceinline__ void block_fold(const double (&acc)[NS][4], const RowMap& t, int c, double* __restrict__ ws_block) {
  __shared__ double red[THREADS * 4 * NS];  // R row slots x NS c sums (R c <= 1024)
  if (t.active) {
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int e = 0; e < 4; ++e) red[(t.r * NS + s) * c + 4 * t.l + e] = acc[s][e];
  }
  __syncthreads();
  for (int j = threadIdx.x; j < NS * c; j += THREADS) {
    double v = red[j];
    for (int q = 1; q < t.R; ++q) v += red[q * NS * c + j];
    ws_block[j] = v;
  }
}

// Step 4: out[i] = the sum of ws[b][i] over the blocks b, i < count; rows >= 0: out[count] = rows as well (the row count behind
// BatchNorm's statistics).  SEGS = 1 is one chain per output, bound by the latency of its loads (45 us measured at 256
// partials).  SEGS = 16 cuts it: thread (g, o) of a block adds segment g of output blockIdx * 16 + o (the segments' loads are in
// flight together), thread (0, o) then adds the segment sums.
template <int SEGS>
inline constexpr int REDUCE_OUTS = SEGS == 1 ? 64 : 16;  // outputs of a block, SEGS threads for each

template <int SEGS, int OUTS = REDUCE_OUTS<SEGS>>
static __global__ __launch_bounds__(OUTS * SEGS) void reduce_kernel(const double* __restrict__ ws, int blocks, int count,
                                                                    double* __restrict__ out, double rows) {
  const int o = (int)threadIdx.x % OUTS, g = (int)threadIdx.x / OUTS;
  const int i = blockIdx.x * OUTS + o;
  if (i == 0 && g == 0 && rows >= 0.0) out[count] = rows;
  const int seg = (blocks + SEGS - 1) / SEGS;
  const int b0 = g * seg, b1 = b0 + seg < blocks ? b0 + seg : blocks;
  double t = 0.0;
  if (i < count && b0 < b1) {
    const double* p = ws + i;
    t = p[(long)b0 * count];
#pragma unroll(SEGS == 1 ? 32 : 16)
    for (int b = b0 + 1; b < b1; ++b) t += p[(long)b * count];
  }
  if constexpr (SEGS == 1) {
    if (i < count) out[i] = t;
  } else {
    __shared__ double red[SEGS][OUTS];
    red[g][o] = t;
    __syncthreads();
    if (g == 0 && i < count) {
      double v = red[0][o];
      const int segs = (blocks + seg - 1) / seg;
      for (int q = 1; q < segs; ++q) v += red[q][o];
      out[i] = v;
    }
  }
}

template <int SEGS>
static inline void launch_reduce(const double* ws, int blocks, int count, double* out, double rows, hipStream_t stream) {
  constexpr int OUTS = REDUCE_OUTS<SEGS>;
  hipLaunchKernelGGL(reduce_kernel<SEGS>, dim3((unsigned)((count + OUTS - 1) / OUTS)), dim3(OUTS * SEGS), 0, stream, ws, blocks, count,
                     out, rows);
}

}  // namespace colsum
#endif  // __HIPCC__
#endif
