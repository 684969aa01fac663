// Host-side sizing shared by the entry points that carve a caller's buffer (csrc/runtime.hip, csrc/trainblock.hip) and the
// ONE rule that sizes cdseg_gemm's workspace (csrc/gemm.hip exports it as cdseg_gemm_ws_bytes).  Functions of the shape only.
#pragma once
#include <cstddef>

#include "../../include/cdseg.h"

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline size_t esz(int dtype) { return dtype == CDSEG_BF16 ? 2 : 4; }

// hands out 256-byte aligned pieces of `base` (nullptr: only the offsets, for the size queries)
struct Carver {
  char* base;
  size_t off;
  void* take(size_t bytes) {
    off = align_up(off, 256);
    void* p = base ? base + off : nullptr;
    off += bytes;
    return p;
  }
};

// ---------------------------------------------------------------- cdseg_gemm's workspace
// The workspace is more than storage: launch_bn (csrc/gemm.hip) splits K only with one (`can_fix = p.ws && ...`), takes
// fewer slices from a smaller one (`while (smax * M * N * 4 > ws_bytes) --smax`) and refuses a fused LayerNorm over several
// column tiles without one (CDSEG_ERR_WORKSPACE).  So this rule decides which plan runs; it mirrors these lines of launch_bn:
// `if (can_fix && blocks < 256 && ...)`: K is split while the output tiles are fewer than the 256 CUs
constexpr long GEMM_WS_FULL_GRID = 256;
// `bm = deep ? 256 : (tall ? 128 : 64)`, `bn = ... 128`: the default 64 x 128 tile.  Launches on other tiles are gated by
// this one all the same (it is the rule the callers have always applied).
constexpr long GEMM_WS_BM = 64, GEMM_WS_BN = 128;
// `wide` / `sq`: the gathered deep convs (N >= 256) on 128 x 256 and 256 x 256 tiles, one block per CU, which split K
// (`splits = 256 / blocks`) past the first gate
constexpr long GEMM_WS_DEEP_BM = 128, GEMM_WS_DEEP_BN = 256;
// (M, N) fp32 planes asked for.  `if (smax > split_max) smax = split_max`: launch_bn uses at most split_max = 16 of them
// (CDSEG_GEMM_SPLIT_MAX; 32 until round 6).  32 stays here: halving it changes every scratch size, a change of its own.
constexpr size_t GEMM_WS_PLANES = 32;
// `splits = (int)(256 / blocks)`: past the first gate a deep conv has at least 32 tiles of 256 x 256, so at most 8 slices
constexpr size_t GEMM_WS_DEEP_PLANES = 8;
// `else if (ln && gn > 1) p.fix = 2`: LayerNorm rows wider than one 128-column tile are finished from one whole plane
constexpr long GEMM_WS_LN_BN = 128;
// the split-K branches stop asking here (`while (smax > 1 && smax * M * N * 4 > ws_bytes) --smax` takes what fits)
constexpr size_t GEMM_WS_CAP = (size_t)64 << 20;

// Bytes for a GEMM of M x N (gathered: nbr != NULL; fused_ln: ln_pre or ln_post), 0 = pass NULL.  Nw: the widest N of the
// GEMMs that share the workspace (N itself for one GEMM; a Block gates on its narrowest product and sizes for its widest).
inline size_t gemm_ws_rule(long M, long N, long Nw, bool gathered, bool fused_ln) {
  auto tiles = [&](long bm, long bn) { return ((M + bm - 1) / bm) * ((N + bn - 1) / bn); };
  auto capped = [](size_t b) { return b < GEMM_WS_CAP ? b : GEMM_WS_CAP; };
  if (tiles(GEMM_WS_BM, GEMM_WS_BN) < GEMM_WS_FULL_GRID) return capped(GEMM_WS_PLANES * M * Nw * 4);
  if (gathered && N >= GEMM_WS_DEEP_BN && tiles(GEMM_WS_DEEP_BM, GEMM_WS_DEEP_BN) < GEMM_WS_FULL_GRID)
    return capped(GEMM_WS_DEEP_PLANES * M * N * 4);
  if (fused_ln && N > GEMM_WS_LN_BN) return (size_t)M * N * 4;
  return 0;
}
