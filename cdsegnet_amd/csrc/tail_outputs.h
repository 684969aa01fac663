// Which outputs the register-resident Block tail (tail_rr_kernel, csrc/blockrr.hip) is asked for, and whether it can form the
// seg head's logits itself.  Plain host C++ (no HIP): the chooser is compiled stand-alone by tests/test_cpu_tail_liveness.py.
#pragma once
#include <cstdint>

#include "../../include/cdseg.h"

// LDS of one tail workgroup: the three weight images (Wp, W1, W2: 9 C^2 16-bit values) and 8 C fp32 parameters
constexpr int tail_rr_lds_bytes(int C) { return 9 * C * C * 2 + 8 * C * 4; }
// the head's weights behind them: class row k at k * (C + 4) floats (padded: the 16 class rows an A operand reads fall into
// different banks), then the bias
constexpr int tail_logits_lds_bytes(int C, int classes) { return classes * (C + 4) * 4 + classes * 4; }
// rr_grid runs two workgroups per CU up to this much LDS each (160 KB per CU)
constexpr int TAIL_RR_LDS_TWO_PER_CU = 80 * 1024;

// CDSEG_OK when tail_rr_kernel<C, LOGITS> exists for this request; decided before any launch
inline int tail_logits_status(int C, int classes, int ld_logits, const void* logits, const void* head_w, const void* out_idx) {
  if (!logits || !head_w || classes <= 0) return CDSEG_ERR_ARG;
  if (C != 64) return CDSEG_ERR_UNSUPPORTED;                      // (the only width a shipped model ends on)
  if (classes % 4 || classes > 32) return CDSEG_ERR_UNSUPPORTED;  // 16-byte logit groups; two 16-class MFMA tiles
  if (tail_rr_lds_bytes(C) + tail_logits_lds_bytes(C, classes) > TAIL_RR_LDS_TWO_PER_CU) return CDSEG_ERR_UNSUPPORTED;
  if (ld_logits < classes || (ld_logits & 3) || ((uintptr_t)logits & 15)) return CDSEG_ERR_UNSUPPORTED;
  if (((uintptr_t)head_w | (uintptr_t)out_idx) & 3) return CDSEG_ERR_ARG;
  return CDSEG_OK;
}
