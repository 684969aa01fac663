// Stand-alone check of the host arithmetic behind the fixed-order column sums (csrc/colsum.h): the row partition, the
// workspace size and the two grid helpers over a sweep of row counts.  Built on its own with the address and
// undefined-behaviour sanitizers (no GPU, nothing loaded into Python):
//   g++ -std=c++20 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/host_checks/colsum_partition_main.cpp -o /tmp/colsum_partition_check && /tmp/colsum_partition_check
// Checks for both minimum block lengths (256: BatchNorm, 64: the gate and the skip statistics) and rows 0 .. 4e8: at most 256
// blocks, the blocks cover rows 0 .. rows - 1 without a gap or an empty block, the block length is the minimum or a multiple of
// 64, the workspace of the widest case (c = 512, three sums) is blocks * 3 * 512 * 8 bytes, no signed overflow anywhere.
#include <cstdio>
#include <initializer_list>

#include "../../cdsegnet_amd/csrc/colsum.h"

static int fails = 0;
#define EXPECT(c)                                                                   \
  do {                                                                              \
    if (!(c)) { std::printf("FAIL %s (line %d)\n", #c, __LINE__); ++fails; }        \
  } while (0)

static void check(long rows, long min_rows) {
  const colsum::Partition q = colsum::partition(rows, min_rows);
  EXPECT(q.blocks >= 0 && q.blocks <= colsum::MAX_BLOCKS);
  EXPECT(q.rows_per_block == min_rows || (q.rows_per_block > min_rows && q.rows_per_block % 64 == 0));
  if (rows == 0) {
    EXPECT(q.blocks == 0 && colsum::ws_bytes(rows, 3, 512, min_rows) == 0);
    return;
  }
  EXPECT((long)(q.blocks - 1) * q.rows_per_block < rows);  // the last block has a row
  EXPECT((long)q.blocks * q.rows_per_block >= rows);       // and the blocks reach the end
  const size_t bytes = colsum::ws_bytes(rows, 3, 512, min_rows);
  EXPECT(bytes == (size_t)q.blocks * 3 * 512 * 8 && bytes <= (size_t)256 * 3 * 512 * 8);
}

int main() {
  long cases = 0;
  for (long min_rows : {colsum::MIN_ROWS_BN, colsum::MIN_ROWS_SWEEP}) {
    for (long rows = 0; rows <= 70000; ++rows, ++cases) check(rows, min_rows);           // every count past the 256-block edge
    for (long rows = 70000; rows <= 400000000L; rows += 9973, ++cases) check(rows, min_rows);
    for (long e = 6; e <= 28; ++e)                                                        // around the powers of two
      for (long d = -65; d <= 65; ++d, ++cases) check((1L << e) + d, min_rows);
    check(400000000L, min_rows);
  }
  // the documented examples and the degenerate inputs
  EXPECT(colsum::partition(5003, colsum::MIN_ROWS_BN).blocks == 20 && colsum::partition(2100, colsum::MIN_ROWS_SWEEP).blocks == 33);
  EXPECT(colsum::partition(20000, colsum::MIN_ROWS_SWEEP).rows_per_block == 128);
  EXPECT(colsum::partition(33001, colsum::MIN_ROWS_SWEEP).rows_per_block == 192);
  EXPECT(colsum::ws_bytes(-1, 2, 32, 64) == 0 && colsum::ws_bytes(100, 2, 0, 64) == 0 && colsum::ws_bytes(100, 0, 32, 64) == 0);
  EXPECT(colsum::width_ok(16, 16) && colsum::width_ok(512, 16) && !colsum::width_ok(24, 16) && !colsum::width_ok(528, 16));
  EXPECT(colsum::width_ok(1, 1) && colsum::width_ok(511, 1) && !colsum::width_ok(0, 1) && !colsum::width_ok(-4, 1) && !colsum::width_ok(513, 1));
  EXPECT(colsum::ld_ok(32, 32) && colsum::ld_ok(40, 32) && !colsum::ld_ok(28, 32) && !colsum::ld_ok(34, 32));
  const int x = 0;
  EXPECT(colsum::aligned(15, (const char*)nullptr, (const int*)nullptr) && colsum::aligned(3, &x) && !colsum::aligned(3, (const char*)&x + 1));
  // the grids: 1 .. max_grid blocks, enough of them below the cap (256 threads; c = 48: 12 lanes a row, 21 rows a block)
  EXPECT(colsum::row_grid(0, 32, 4, 2048) == 1 && colsum::row_grid(1, 512, 4, 4096) == 1 && colsum::row_grid(400000000L, 512, 4, 4096) == 4096);
  EXPECT(colsum::row_grid(120000, 32, 4, 2048) == 938 && colsum::row_grid(33001, 512, 4, 4096) == 4096 && colsum::row_grid(1000, 48, 2, 2048) == 24);
  EXPECT(colsum::elem_grid(0, 4, 4096) == 1 && colsum::elem_grid(1025, 4, 4096) == 2 && colsum::elem_grid(400000000L * 512, 4, 4096) == 4096);
  std::printf("%ld row counts checked, %d failures\n", cases, fails);
  return fails ? 1 : 0;
}
