// Stand-alone check of the host arithmetic behind the deterministic weight gradient (csrc/wgrad_partition.h): the row
// partition and the workspace sizes over a sweep of shapes.  Built on its own with the address and undefined-behaviour
// sanitizers (no GPU, nothing loaded into Python):
//   hipcc -x c++ -std=c++20 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//         tools/host_checks/wgrad_partition_main.cpp -o /tmp/wgrad_partition_check && /tmp/wgrad_partition_check
// Checks for every shape: the splits cover rows 0 .. M - 1 without a gap or an empty split, the split length keeps the
// kernels' granularity (4 rows fp32, 64 rows 16-bit), the workspace grows with the split count, no signed overflow.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../cdsegnet_amd/csrc/wgrad_partition.h"

static int fails = 0;
#define EXPECT(c)                                                                   \
  do {                                                                              \
    if (!(c)) { std::printf("FAIL %s (line %d)\n", #c, __LINE__); ++fails; }        \
  } while (0)

static void check(long M, int N, int K, int noff, bool lp) {
  const cdseg_wgrad::Partition q = lp ? cdseg_wgrad::partition_16(M, N, K, noff) : cdseg_wgrad::partition_f32(M, N, K, noff);
  if (q.splits < 0) {  // more blocks along z than a grid holds: reported, not launched
    EXPECT(lp);
    return;
  }
  EXPECT(q.splits >= 1 && q.rows_per_split >= 1);
  EXPECT(q.rows_per_split % (lp ? 64 : 4) == 0);
  EXPECT((long)(q.splits - 1) * q.rows_per_split < M);  // the last split has a row
  EXPECT((long)q.splits * q.rows_per_split >= M);       // and the splits reach the end
  EXPECT((long)q.splits * noff <= 65535);
  // the workspace really holds what the kernels index: fill it the way they do
  const size_t n = cdseg_wgrad::det_ws_floats(N, K, noff, q.splits);
  if (n <= (size_t)1 << 24) {
    std::vector<float> ws(n, 0.f);
    float* ws_db = ws.data() + (size_t)noff * q.splits * N * K;
    for (int z = 0; z < noff * q.splits; ++z) ws[((size_t)z * N + (N - 1)) * K + (K - 1)] = 1.f;
    for (int s = 0; s < q.splits; ++s) ws_db[(size_t)s * N + N - 1] = 1.f;
  }
  EXPECT(cdseg_wgrad::det_ws_floats(N, K, noff, q.splits + 1) > n);
}

int main() {
  const long Ms[] = {1, 3, 4, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4100, 5003, 120000, 1000003, 400000000L};
  const int Cs[] = {16, 32, 48, 64, 96, 128, 192, 256, 512, 2048};
  const int offs[] = {1, 27, 125};
  long cases = 0;
  for (long M : Ms)
    for (int N : Cs)
      for (int K : Cs)
        for (int noff : offs)
          for (int lp = 0; lp < 2; ++lp) { check(M, N, K, noff, lp != 0); ++cases; }
  // degenerate shapes give an empty partition, not a division by zero
  EXPECT(cdseg_wgrad::partition_f32(0, 16, 16, 1).splits == 0);
  EXPECT(cdseg_wgrad::partition_16(5, 0, 16, 1).splits == 0);
  EXPECT(cdseg_wgrad::ln_det_ws_floats(0, 32) == 0 && cdseg_wgrad::ln_det_ws_floats(65, 32) == 2 * 2 * 32);
  EXPECT(cdseg_wgrad::ln_blocks(64) == 1 && cdseg_wgrad::ln_blocks(120000) == 1875);
  std::printf("%ld shapes checked, %d failures\n", cases, fails);
  return fails ? 1 : 0;
}
