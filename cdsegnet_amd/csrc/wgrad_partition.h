// Row partition of the weight-gradient launches (csrc/train.hip) and the workspace arithmetic of their deterministic forms.
// Plain host C++ (no HIP, no device query): a function of the shape only, so that two runs, two machines and the
// diagnostic entry point cdseg_wgrad_partition agree on where the split boundaries are.  Also compiled on its own by
// tools/host_checks/wgrad_partition_main.cpp (address / undefined-behaviour sanitizers).
#ifndef CDSEG_WGRAD_PARTITION_H
#define CDSEG_WGRAD_PARTITION_H
#include <cstddef>

namespace cdseg_wgrad {

struct Partition {
  long rows_per_split;  // rows m_begin = split * rows_per_split .. of a split (the last one may be shorter)
  int splits;           // blocks along the rows per (tile, kernel offset); < 0: the launch is not supported
  int tn, tk;           // 16-bit form: tile = 32 tn x 32 tk; fp32 form: 2 x 2 (64 x 64)
};

inline long cdiv_l(long a, long b) { return (a + b - 1) / b; }

// fp32 form (wgrad_kernel): 64 x 64 tiles, ~8 blocks per CU, at least 1024 rows per block, split length a multiple of 4
inline Partition partition_f32(long M, int N, int K, int noff) {
  Partition q{0, 0, 2, 2};
  if (M <= 0 || N <= 0 || K <= 0 || noff <= 0) return q;
  const long tiles = cdiv_l(N, 64) * cdiv_l(K, 64) * noff;
  long splits = (2048 + tiles - 1) / tiles;
  const long max_splits = (M + 1023) / 1024;
  if (splits > max_splits) splits = max_splits;
  if (splits < 1) splits = 1;
  q.rows_per_split = ((M + splits - 1) / splits + 3) & ~3L;
  q.splits = (int)((M + q.rows_per_split - 1) / q.rows_per_split);
  return q;
}

// 16-bit form (wgrad16_kernel<TN, TK>): the narrowest of 32 / 64 / 128 columns that covers N (K), 128 x 128 -> 128 x 64;
// ~2 blocks per CU, at least 512 rows per block, split length a multiple of the 64-row chunk
inline Partition partition_16(long M, int N, int K, int noff) {
  Partition q{0, 0, 0, 0};
  if (M <= 0 || N <= 0 || K <= 0 || noff <= 0) return q;
  q.tn = N > 64 ? 4 : N > 32 ? 2 : 1;
  q.tk = K > 64 ? 4 : K > 32 ? 2 : 1;
  if (q.tn == 4 && q.tk == 4) q.tk = 2;
  const long tiles = cdiv_l(N, 32 * q.tn) * cdiv_l(K, 32 * q.tk) * noff;
  long splits = (512 + tiles - 1) / tiles;
  const long max_splits = (M + 511) / 512;
  if (splits > max_splits) splits = max_splits;
  if (splits < 1) splits = 1;
  q.rows_per_split = ((M + splits - 1) / splits + 63) / 64 * 64;
  splits = (M + q.rows_per_split - 1) / q.rows_per_split;
  q.splits = splits * noff > 65535 ? -1 : (int)splits;
  return q;
}

// Workspace of the deterministic forms, in floats: one (N x K) partial tile image per (offset, split), then one N-vector
// of bias partials per split.
inline size_t det_ws_floats(int N, int K, int noff, int splits) {
  return (size_t)noff * (size_t)splits * (size_t)N * (size_t)K + (size_t)splits * (size_t)N;
}

// LayerNorm backward, deterministic form: one (dgamma, dbeta) row pair per 64-row block
inline long ln_blocks(long m) { return m <= 0 ? 0 : cdiv_l(m, 64); }
inline size_t ln_det_ws_floats(long m, int c) { return (size_t)ln_blocks(m) * 2 * (size_t)(c > 0 ? c : 0); }

}  // namespace cdseg_wgrad
#endif
