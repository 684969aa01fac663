"""GPU: cdseg_gemm against fp64, addressed by ROUTE - which kernel the host-side chooser (csrc/gemm.hip launch_bn) picked.

launch_bn routes a call among some fifty template instantiations by thresholds on M, N, K, kvol, the epilogue, the workspace
and the alignment of the operands.  A numerical test only guards the kernel it happens to run; a retuned threshold moves it
onto another one without turning anything red.  Every case of ROUTE_CASES therefore does two things: it compares the result
with an fp64 gather + matmul, and it asserts the launch record (include/cdseg.h cdseg_route_*) - kernel name, split-K or not,
fix, xmode, vec_ok - against the route written in the table, which was read off the chooser's rule by hand.  A case whose
route moves fails and has to be re-pointed at the edge it was guarding; test_every_compiled_gemm_variant_is_reached_or_
accounted_for fails when a compiled kernel is left without a case.

Shapes are no workload shapes: for every reachable kernel the smallest M its rule admits, that M + 1 and a k * BM + 1, the
smallest N, an N with a ragged last column tile and an N % 4 != 0 (the scalar epilogue), where the rule admits them; both
kernel-map layouts; K below 64, a power of two from 64 up, and no power of two (the gather then divides).

Bounds (derived, not tuned; A ~ N(0, 1), W ~ N(0, 1) / sqrt(kvol K), so that |out| = O(1)):
  fp32 output      2e-5 sqrt(kvol K) + 1e-5: fp32 accumulation of kvol K exactly representable products (test_gemm_plain's);
  16-bit output    that + one rounding of the result to nearest: |ref| 2^-8 (bfloat16, 8 significant bits) or |ref| 2^-11 (half);
  fp32x3           test_gemm_fp32x3_is_as_good_as_fp32_on_fp32_operands': twice the fp32 bound, and 8 x the exact-fp32 kernel's
                   own error + 2e-6;
  LayerNorm        x = acc + bias + res is held to the fp32 bound d.  y = LN(x): a perturbation of at most d per element moves
                   x - mean by at most 2 d and the standard deviation s by at most d, so |dy| <= (2 d / s) (1 + |y|) to first
                   order; asserted with s = the smallest row deviation, |y| = the largest normalised value, times 1.05 for the
                   second order, plus 4e-6 (1 + |y|) for the kernel's own fp32 arithmetic, all times the largest |gamma|.
Every output lies in guard bands, every A in NaN guards and every workspace is exact-size (tests/guard_bands.py): an index
slip lands in memory the test owns and shows as a damaged band or a NaN, not as a fault."""
import collections
import ctypes
import time

import pytest
import torch

from cdsegnet_amd import _lib
from tests.guard_bands import banded, exact_workspace, poisoned_input

pytestmark = pytest.mark.gpu

R = collections.namedtuple("R", "ct M N K kvol lay epi ws out kernel split fix xmode vec")
# ct   compute type: b16 = the build's 16-bit type (run in both builds), f32, x3 = fp32 operands as three half products
# lay  kernel map: "-" none (plain GEMM), "row" = (M, kvol), "off" = (kvol, M)
# epi  "bias": out = acc + bias;  "ln": out = acc + bias + res, ln_out = LayerNorm(out)
# ws   a split-K workspace of 16 M N floats is given (1) or not (0);  out: fp32 or "lp" = the build's 16-bit type
# then the route the rule gives: catalogue name, split-K (splits > 1), fix, xmode, vec_ok
ROUTE_CASES = [
    R("b16", 1, 4, 8, 1, "-", "bias", 1, "f32", "gemm_kernel<b16,32,kshort,plain,64>", False, 0, 0, True),
    R("b16", 63, 20, 24, 1, "-", "bias", 1, "lp", "gemm_kernel<b16,32,kshort,plain,64>", False, 0, 0, True),
    R("b16", 129, 30, 64, 1, "-", "bias", 1, "f32", "gemm_kernel<b16,32,kshort,plain,64>", False, 0, 0, False),
    R("b16", 1, 36, 8, 1, "-", "bias", 1, "lp", "gemm_kernel<b16,64,kshort,plain,64>", False, 0, 0, True),
    R("b16", 65, 33, 24, 1, "-", "bias", 1, "f32", "gemm_kernel<b16,64,kshort,plain,64>", False, 0, 0, False),
    R("b16", 129, 64, 64, 1, "-", "bias", 1, "f32", "gemm_kernel<b16,64,kshort,plain,64>", False, 0, 0, True),
    R("b16", 1, 68, 8, 1, "-", "bias", 1, "f32", "gemm_kernel<b16,128,kshort,plain,64>", False, 0, 0, True),
    R("b16", 65, 132, 24, 1, "-", "bias", 1, "lp", "gemm_kernel<b16,128,kshort,plain,64>", False, 0, 0, True),
    R("b16", 129, 130, 64, 1, "-", "bias", 1, "f32", "gemm_kernel<b16,128,kshort,plain,64>", False, 0, 0, False),
    R("b16", 2, 260, 64, 1, "-", "bias", 1, "f32", "gemm_kernel<b16,128,kshort,plain,64>", False, 0, 0, True),
    R("b16", 1, 4, 72, 1, "-", "bias", 1, "f32", "gemm_kernel<b16,32,klong,plain,64>", False, 0, 0, True),
    R("b16", 65, 30, 200, 1, "-", "bias", 1, "f32", "gemm_kernel<b16,32,klong,plain,64>", False, 0, 0, False),
    R("b16", 129, 20, 128, 1, "-", "bias", 1, "lp", "gemm_kernel<b16,32,klong,plain,64>", False, 0, 0, True),
    R("b16", 1, 36, 72, 1, "-", "bias", 1, "lp", "gemm_kernel<b16,64,klong,plain,64>", False, 0, 0, True),
    R("b16", 129, 33, 200, 1, "-", "bias", 1, "f32", "gemm_kernel<b16,64,klong,plain,64>", False, 0, 0, False),
    R("b16", 65, 64, 128, 1, "-", "bias", 1, "f32", "gemm_kernel<b16,64,klong,plain,64>", False, 0, 0, True),
    R("b16", 1, 68, 72, 1, "-", "bias", 1, "f32", "gemm_kernel<b16,128,klong,plain,64>", False, 0, 0, True),
    R("b16", 129, 132, 200, 1, "-", "bias", 1, "lp", "gemm_kernel<b16,128,klong,plain,64>", False, 0, 0, True),
    R("b16", 127, 132, 128, 1, "-", "bias", 1, "f32", "gemm_kernel<b16,128,klong,plain,64>", False, 0, 0, True),
    R("b16", 129, 130, 72, 1, "-", "bias", 1, "f32", "gemm_kernel<b16,128,klong,plain,64>", False, 0, 0, False),
    R("b16", 130, 132, 2048, 1, "-", "bias", 1, "f32", "gemm_dma_kernel<64,plain,128,2,ring>", True, 1, 0, True),
    R("b16", 130, 132, 2048, 1, "-", "bias", 0, "f32", "gemm_dma_kernel<64,plain,128,2,ring>", False, 0, 0, True),
    R("b16", 130, 20, 2048, 1, "-", "bias", 1, "lp", "gemm_kernel<b16,32,klong,plain,64>", True, 1, 0, True),
    R("b16", 65, 36, 2056, 1, "-", "bias", 1, "f32", "gemm_kernel<b16,64,klong,plain,64>", True, 1, 0, True),
    R("b16", 130, 130, 2048, 1, "-", "bias", 1, "f32", "gemm_dma_kernel<64,plain,128,2,ring>", False, 0, 0, False),
    R("b16", 129, 132, 2056, 1, "-", "bias", 1, "f32", "gemm_kernel<b16,128,klong,plain,64>", True, 1, 0, True),
    R("b16", 129, 128, 128, 1, "-", "ln", 1, "f32", "gemm_kernel<b16,128,klong,plain,64>", False, 0, 0, True),
    R("b16", 65, 32, 72, 1, "-", "ln", 1, "f32", "gemm_kernel<b16,32,klong,plain,64>", False, 0, 0, True),
    R("b16", 127, 132, 128, 1, "-", "ln", 1, "f32", "gemm_kernel<b16,128,klong,plain,64>", False, 2, 0, True),
    R("b16", 129, 256, 72, 1, "-", "ln", 1, "f32", "gemm_kernel<b16,128,klong,plain,64>", False, 2, 0, True),
    R("b16", 65, 512, 128, 1, "-", "ln", 1, "f32", "gemm_kernel<b16,128,klong,plain,64>", False, 2, 0, True),
    R("b16", 70, 64, 2048, 1, "-", "ln", 1, "f32", "gemm_kernel<b16,64,klong,plain,64>", True, 2, 0, True),
    R("b16", 129, 132, 2048, 1, "-", "ln", 1, "f32", "gemm_dma_kernel<64,plain,128,2,ring>", True, 2, 0, True),
    R("b16", 129, 1024, 512, 1, "-", "bias", 1, "f32", "gemm_dma_kernel<64,plain,128,2,ring>", False, 0, 1, True),
    R("b16", 1, 4, 8, 8, "row", "bias", 1, "f32", "gemm_kernel<b16,32,kshort,gather,64>", False, 0, 0, True),
    R("b16", 65, 30, 8, 8, "off", "bias", 1, "f32", "gemm_kernel<b16,32,kshort,gather,64>", False, 0, 0, False),
    R("b16", 129, 36, 64, 1, "off", "bias", 1, "lp", "gemm_kernel<b16,64,kshort,gather,64>", False, 0, 0, True),
    R("b16", 65, 33, 8, 8, "row", "bias", 1, "f32", "gemm_kernel<b16,64,kshort,gather,64>", False, 0, 0, False),
    R("b16", 129, 68, 8, 8, "row", "bias", 1, "f32", "gemm_kernel<b16,128,kshort,gather,64>", False, 0, 0, True),
    R("b16", 65, 130, 8, 8, "off", "bias", 1, "f32", "gemm_kernel<b16,128,kshort,gather,64>", False, 0, 0, False),
    R("b16", 1, 132, 16, 4, "off", "bias", 1, "lp", "gemm_kernel<b16,128,kshort,gather,64>", False, 0, 0, True),
    R("b16", 1, 4, 8, 27, "row", "bias", 1, "f32", "gemm_kernel<b16,32,klong,gather,64>", False, 0, 0, True),
    R("b16", 64, 30, 24, 27, "off", "bias", 1, "f32", "gemm_kernel<b16,32,klong,gather,64>", False, 0, 0, False),
    R("b16", 63, 36, 64, 27, "off", "bias", 1, "lp", "gemm_kernel<b16,64,klong,gather,64>", True, 1, 0, True),
    R("b16", 64, 33, 96, 8, "row", "bias", 1, "f32", "gemm_kernel<b16,64,klong,gather,64>", False, 0, 0, False),
    R("b16", 64, 68, 32, 125, "row", "bias", 1, "f32", "gemm_kernel<b16,128,klong,gather,64>", True, 1, 0, True),
    R("b16", 1, 132, 192, 27, "off", "bias", 1, "f32", "gemm_kernel<b16,128,klong,gather,64>", True, 1, 0, True),
    R("b16", 129, 64, 64, 27, "off", "ln", 1, "f32", "gemm_kernel<b16,64,klong,gather,64>", True, 2, 0, True),
    R("b16", 129, 132, 64, 27, "row", "ln", 1, "f32", "gemm_dma_kernel<128,gather,128,2,ring>", True, 2, 0, True),
    R("b16", 65, 4, 8, 27, "row", "bias", 1, "f32", "gemm_kernel<b16,32,klong,gather,128>", False, 0, 0, True),
    R("b16", 129, 20, 24, 27, "off", "bias", 1, "lp", "gemm_kernel<b16,32,klong,gather,128>", True, 1, 0, True),
    R("b16", 257, 30, 32, 125, "off", "bias", 1, "f32", "gemm_kernel<b16,32,klong,gather,128>", False, 0, 0, False),
    R("b16", 65, 36, 96, 27, "off", "bias", 1, "f32", "gemm_kernel<b16,64,klong,gather,128>", True, 1, 0, True),
    R("b16", 129, 64, 128, 27, "row", "bias", 1, "lp", "gemm_kernel<b16,64,klong,gather,128>", True, 1, 0, True),
    R("b16", 257, 33, 8, 125, "row", "bias", 1, "f32", "gemm_kernel<b16,64,klong,gather,128>", False, 0, 0, False),
    R("b16", 65, 128, 64, 27, "off", "bias", 1, "f32", "gemm_kernel<b16,128,klong,gather,128>", True, 1, 0, True),
    R("b16", 129, 132, 32, 27, "row", "bias", 1, "lp", "gemm_kernel<b16,128,klong,gather,128>", True, 1, 0, True),
    R("b16", 257, 68, 24, 27, "off", "bias", 1, "f32", "gemm_kernel<b16,128,klong,gather,128>", True, 1, 0, True),
    R("b16", 129, 130, 96, 27, "off", "bias", 1, "f32", "gemm_kernel<b16,128,klong,gather,128>", False, 0, 0, False),
    R("b16", 129, 132, 192, 27, "row", "bias", 0, "f32", "gemm_kernel<b16,128,klong,gather,128>", False, 0, 0, True),
    R("b16", 257, 320, 320, 8, "off", "bias", 1, "f32", "gemm_kernel<b16,128,klong,gather,128>", True, 1, 1, True),
    R("b16", 8193, 32, 32, 27, "off", "bias", 1, "f32", "gemm_kernel<b16,32,klong,gather,128>", True, 1, 2, True),
    R("f32", 1, 4, 8, 1, "-", "bias", 1, "f32", "gemm_kernel<f32,32,kshort,plain,64>", False, 0, 0, True),
    R("f32", 63, 20, 24, 1, "-", "bias", 1, "f32", "gemm_kernel<f32,32,kshort,plain,64>", False, 0, 0, True),
    R("f32", 129, 30, 64, 1, "-", "bias", 1, "f32", "gemm_kernel<f32,32,kshort,plain,64>", False, 0, 0, False),
    R("f32", 1, 36, 8, 1, "-", "bias", 1, "f32", "gemm_kernel<f32,64,kshort,plain,64>", False, 0, 0, True),
    R("f32", 65, 33, 24, 1, "-", "bias", 1, "f32", "gemm_kernel<f32,64,kshort,plain,64>", False, 0, 0, False),
    R("f32", 129, 64, 64, 1, "-", "bias", 1, "f32", "gemm_kernel<f32,64,kshort,plain,64>", False, 0, 0, True),
    R("f32", 1, 68, 8, 1, "-", "bias", 1, "f32", "gemm_kernel<f32,128,kshort,plain,64>", False, 0, 0, True),
    R("f32", 65, 132, 24, 1, "-", "bias", 1, "f32", "gemm_kernel<f32,128,kshort,plain,64>", False, 0, 0, True),
    R("f32", 129, 130, 64, 1, "-", "bias", 1, "f32", "gemm_kernel<f32,128,kshort,plain,64>", False, 0, 0, False),
    R("f32", 2, 260, 64, 1, "-", "bias", 1, "f32", "gemm_kernel<f32,128,kshort,plain,64>", False, 0, 0, True),
    R("f32", 1, 4, 72, 1, "-", "bias", 1, "f32", "gemm_kernel<f32,32,klong,plain,64>", False, 0, 0, True),
    R("f32", 65, 30, 200, 1, "-", "bias", 1, "f32", "gemm_kernel<f32,32,klong,plain,64>", False, 0, 0, False),
    R("f32", 129, 20, 128, 1, "-", "bias", 1, "f32", "gemm_kernel<f32,32,klong,plain,64>", False, 0, 0, True),
    R("f32", 1, 36, 72, 1, "-", "bias", 1, "f32", "gemm_kernel<f32,64,klong,plain,64>", False, 0, 0, True),
    R("f32", 129, 33, 200, 1, "-", "bias", 1, "f32", "gemm_kernel<f32,64,klong,plain,64>", False, 0, 0, False),
    R("f32", 65, 64, 128, 1, "-", "bias", 1, "f32", "gemm_kernel<f32,64,klong,plain,64>", False, 0, 0, True),
    R("f32", 1, 68, 72, 1, "-", "bias", 1, "f32", "gemm_kernel<f32,128,klong,plain,64>", False, 0, 0, True),
    R("f32", 129, 132, 200, 1, "-", "bias", 1, "f32", "gemm_kernel<f32,128,klong,plain,64>", False, 0, 0, True),
    R("f32", 127, 132, 128, 1, "-", "bias", 1, "f32", "gemm_kernel<f32,128,klong,plain,64>", False, 0, 0, True),
    R("f32", 129, 130, 72, 1, "-", "bias", 1, "f32", "gemm_kernel<f32,128,klong,plain,64>", False, 0, 0, False),
    R("f32", 130, 132, 1024, 1, "-", "bias", 1, "f32", "gemm_kernel<f32,128,klong,plain,64>", True, 1, 0, True),
    R("f32", 130, 132, 1024, 1, "-", "bias", 0, "f32", "gemm_kernel<f32,128,klong,plain,64>", False, 0, 0, True),
    R("f32", 130, 20, 1024, 1, "-", "bias", 1, "f32", "gemm_kernel<f32,32,klong,plain,64>", True, 1, 0, True),
    R("f32", 65, 36, 1032, 1, "-", "bias", 1, "f32", "gemm_kernel<f32,64,klong,plain,64>", True, 1, 0, True),
    R("f32", 130, 130, 1024, 1, "-", "bias", 1, "f32", "gemm_kernel<f32,128,klong,plain,64>", False, 0, 0, False),
    R("f32", 129, 132, 1032, 1, "-", "bias", 1, "f32", "gemm_kernel<f32,128,klong,plain,64>", True, 1, 0, True),
    R("f32", 129, 128, 128, 1, "-", "ln", 1, "f32", "gemm_kernel<f32,128,klong,plain,64>", False, 0, 0, True),
    R("f32", 65, 32, 72, 1, "-", "ln", 1, "f32", "gemm_kernel<f32,32,klong,plain,64>", False, 0, 0, True),
    R("f32", 127, 132, 128, 1, "-", "ln", 1, "f32", "gemm_kernel<f32,128,klong,plain,64>", False, 2, 0, True),
    R("f32", 129, 256, 72, 1, "-", "ln", 1, "f32", "gemm_kernel<f32,128,klong,plain,64>", False, 2, 0, True),
    R("f32", 65, 512, 128, 1, "-", "ln", 1, "f32", "gemm_kernel<f32,128,klong,plain,64>", False, 2, 0, True),
    R("f32", 70, 64, 1024, 1, "-", "ln", 1, "f32", "gemm_kernel<f32,64,klong,plain,64>", True, 2, 0, True),
    R("f32", 129, 132, 1024, 1, "-", "ln", 1, "f32", "gemm_kernel<f32,128,klong,plain,64>", True, 2, 0, True),
    R("f32", 129, 1024, 256, 1, "-", "bias", 1, "f32", "gemm_kernel<f32,128,klong,plain,64>", False, 0, 1, True),
    R("f32", 1, 4, 8, 8, "row", "bias", 1, "f32", "gemm_kernel<f32,32,kshort,gather,64>", False, 0, 0, True),
    R("f32", 65, 30, 8, 8, "off", "bias", 1, "f32", "gemm_kernel<f32,32,kshort,gather,64>", False, 0, 0, False),
    R("f32", 129, 36, 64, 1, "off", "bias", 1, "f32", "gemm_kernel<f32,64,kshort,gather,64>", False, 0, 0, True),
    R("f32", 65, 33, 8, 8, "row", "bias", 1, "f32", "gemm_kernel<f32,64,kshort,gather,64>", False, 0, 0, False),
    R("f32", 129, 68, 8, 8, "row", "bias", 1, "f32", "gemm_kernel<f32,128,kshort,gather,64>", False, 0, 0, True),
    R("f32", 65, 130, 8, 8, "off", "bias", 1, "f32", "gemm_kernel<f32,128,kshort,gather,64>", False, 0, 0, False),
    R("f32", 1, 132, 16, 4, "off", "bias", 1, "f32", "gemm_kernel<f32,128,kshort,gather,64>", False, 0, 0, True),
    R("f32", 1, 4, 8, 27, "row", "bias", 1, "f32", "gemm_kernel<f32,32,klong,gather,64>", True, 1, 0, True),
    R("f32", 64, 30, 24, 27, "off", "bias", 1, "f32", "gemm_kernel<f32,32,klong,gather,64>", False, 0, 0, False),
    R("f32", 63, 36, 64, 27, "off", "bias", 1, "f32", "gemm_kernel<f32,64,klong,gather,64>", True, 1, 0, True),
    R("f32", 64, 33, 96, 8, "row", "bias", 1, "f32", "gemm_kernel<f32,64,klong,gather,64>", False, 0, 0, False),
    R("f32", 64, 68, 32, 125, "row", "bias", 1, "f32", "gemm_kernel<f32,128,klong,gather,64>", True, 1, 0, True),
    R("f32", 1, 132, 192, 27, "off", "bias", 1, "f32", "gemm_kernel<f32,128,klong,gather,64>", True, 1, 0, True),
    R("f32", 129, 64, 64, 27, "off", "ln", 1, "f32", "gemm_kernel<f32,64,klong,gather,64>", True, 2, 0, True),
    R("f32", 129, 132, 64, 27, "row", "ln", 1, "f32", "gemm_kernel<f32,128,klong,gather,64>", True, 2, 0, True),
    R("f32", 65, 4, 8, 27, "row", "bias", 1, "f32", "gemm_kernel<f32,32,klong,gather,128>", True, 1, 0, True),
    R("f32", 129, 20, 24, 27, "off", "bias", 1, "f32", "gemm_kernel<f32,32,klong,gather,128>", True, 1, 0, True),
    R("f32", 257, 30, 32, 125, "off", "bias", 1, "f32", "gemm_kernel<f32,32,klong,gather,128>", False, 0, 0, False),
    R("f32", 65, 36, 96, 27, "off", "bias", 1, "f32", "gemm_kernel<f32,64,klong,gather,128>", True, 1, 0, True),
    R("f32", 129, 64, 128, 27, "row", "bias", 1, "f32", "gemm_kernel<f32,64,klong,gather,128>", True, 1, 0, True),
    R("f32", 257, 33, 8, 125, "row", "bias", 1, "f32", "gemm_kernel<f32,64,klong,gather,128>", False, 0, 0, False),
    R("f32", 65, 128, 64, 27, "off", "bias", 1, "f32", "gemm_kernel<f32,128,klong,gather,128>", True, 1, 0, True),
    R("f32", 129, 132, 32, 27, "row", "bias", 1, "f32", "gemm_kernel<f32,128,klong,gather,128>", True, 1, 0, True),
    R("f32", 257, 68, 24, 27, "off", "bias", 1, "f32", "gemm_kernel<f32,128,klong,gather,128>", True, 1, 0, True),
    R("f32", 129, 130, 96, 27, "off", "bias", 1, "f32", "gemm_kernel<f32,128,klong,gather,128>", False, 0, 0, False),
    R("f32", 129, 132, 192, 27, "row", "bias", 0, "f32", "gemm_kernel<f32,128,klong,gather,128>", False, 0, 0, True),
    R("f32", 257, 320, 320, 8, "off", "bias", 1, "f32", "gemm_kernel<f32,128,klong,gather,128>", True, 1, 1, True),
    R("f32", 8193, 32, 32, 27, "off", "bias", 1, "f32", "gemm_kernel<f32,32,klong,gather,128>", True, 1, 2, True),
    R("x3", 1, 4, 8, 1, "-", "bias", 1, "f32", "gemm_kernel<x3,32,kshort,plain,64>", False, 0, 0, True),
    R("x3", 63, 20, 24, 1, "-", "bias", 1, "f32", "gemm_kernel<x3,32,kshort,plain,64>", False, 0, 0, True),
    R("x3", 129, 30, 64, 1, "-", "bias", 1, "f32", "gemm_kernel<x3,32,kshort,plain,64>", False, 0, 0, False),
    R("x3", 1, 36, 8, 1, "-", "bias", 1, "f32", "gemm_kernel<x3,64,kshort,plain,64>", False, 0, 0, True),
    R("x3", 65, 33, 24, 1, "-", "bias", 1, "f32", "gemm_kernel<x3,64,kshort,plain,64>", False, 0, 0, False),
    R("x3", 129, 64, 64, 1, "-", "bias", 1, "f32", "gemm_kernel<x3,64,kshort,plain,64>", False, 0, 0, True),
    R("x3", 1, 68, 8, 1, "-", "bias", 1, "f32", "gemm_kernel<x3,128,kshort,plain,64>", False, 0, 0, True),
    R("x3", 65, 132, 24, 1, "-", "bias", 1, "f32", "gemm_kernel<x3,128,kshort,plain,64>", False, 0, 0, True),
    R("x3", 129, 130, 64, 1, "-", "bias", 1, "f32", "gemm_kernel<x3,128,kshort,plain,64>", False, 0, 0, False),
    R("x3", 2, 260, 64, 1, "-", "bias", 1, "f32", "gemm_kernel<x3,128,kshort,plain,64>", False, 0, 0, True),
    R("x3", 1, 4, 72, 1, "-", "bias", 1, "f32", "gemm_kernel<x3,32,klong,plain,64>", False, 0, 0, True),
    R("x3", 65, 30, 200, 1, "-", "bias", 1, "f32", "gemm_kernel<x3,32,klong,plain,64>", False, 0, 0, False),
    R("x3", 129, 20, 128, 1, "-", "bias", 1, "f32", "gemm_kernel<x3,32,klong,plain,64>", False, 0, 0, True),
    R("x3", 1, 36, 72, 1, "-", "bias", 1, "f32", "gemm_kernel<x3,64,klong,plain,64>", False, 0, 0, True),
    R("x3", 129, 33, 200, 1, "-", "bias", 1, "f32", "gemm_kernel<x3,64,klong,plain,64>", False, 0, 0, False),
    R("x3", 65, 64, 128, 1, "-", "bias", 1, "f32", "gemm_kernel<x3,64,klong,plain,64>", False, 0, 0, True),
    R("x3", 1, 68, 72, 1, "-", "bias", 1, "f32", "gemm_kernel<x3,128,klong,plain,64>", False, 0, 0, True),
    R("x3", 129, 132, 200, 1, "-", "bias", 1, "f32", "gemm_kernel<x3,128,klong,plain,64>", False, 0, 0, True),
    R("x3", 127, 132, 128, 1, "-", "bias", 1, "f32", "gemm_kernel<x3,128,klong,plain,64>", False, 0, 0, True),
    R("x3", 129, 130, 72, 1, "-", "bias", 1, "f32", "gemm_kernel<x3,128,klong,plain,64>", False, 0, 0, False),
    R("x3", 130, 132, 1024, 1, "-", "bias", 1, "f32", "gemm_kernel<x3,128,klong,plain,64>", True, 1, 0, True),
    R("x3", 130, 132, 1024, 1, "-", "bias", 0, "f32", "gemm_kernel<x3,128,klong,plain,64>", False, 0, 0, True),
    R("x3", 130, 20, 1024, 1, "-", "bias", 1, "f32", "gemm_kernel<x3,32,klong,plain,64>", True, 1, 0, True),
    R("x3", 65, 36, 1032, 1, "-", "bias", 1, "f32", "gemm_kernel<x3,64,klong,plain,64>", True, 1, 0, True),
    R("x3", 130, 130, 1024, 1, "-", "bias", 1, "f32", "gemm_kernel<x3,128,klong,plain,64>", False, 0, 0, False),
    R("x3", 129, 132, 1032, 1, "-", "bias", 1, "f32", "gemm_kernel<x3,128,klong,plain,64>", True, 1, 0, True),
    R("x3", 129, 128, 128, 1, "-", "ln", 1, "f32", "gemm_kernel<x3,128,klong,plain,64>", False, 0, 0, True),
    R("x3", 65, 32, 72, 1, "-", "ln", 1, "f32", "gemm_kernel<x3,32,klong,plain,64>", False, 0, 0, True),
    R("x3", 127, 132, 128, 1, "-", "ln", 1, "f32", "gemm_kernel<x3,128,klong,plain,64>", False, 2, 0, True),
    R("x3", 129, 256, 72, 1, "-", "ln", 1, "f32", "gemm_kernel<x3,128,klong,plain,64>", False, 2, 0, True),
    R("x3", 65, 512, 128, 1, "-", "ln", 1, "f32", "gemm_kernel<x3,128,klong,plain,64>", False, 2, 0, True),
    R("x3", 70, 64, 1024, 1, "-", "ln", 1, "f32", "gemm_kernel<x3,64,klong,plain,64>", True, 2, 0, True),
    R("x3", 129, 132, 1024, 1, "-", "ln", 1, "f32", "gemm_kernel<x3,128,klong,plain,64>", True, 2, 0, True),
    R("x3", 129, 1024, 256, 1, "-", "bias", 1, "f32", "gemm_kernel<x3,128,klong,plain,64>", False, 0, 1, True),
    R("x3", 1, 4, 8, 8, "row", "bias", 1, "f32", "gemm_kernel<x3,32,kshort,gather,64>", False, 0, 0, True),
    R("x3", 65, 30, 8, 8, "off", "bias", 1, "f32", "gemm_kernel<x3,32,kshort,gather,64>", False, 0, 0, False),
    R("x3", 129, 36, 64, 1, "off", "bias", 1, "f32", "gemm_kernel<x3,64,kshort,gather,64>", False, 0, 0, True),
    R("x3", 65, 33, 8, 8, "row", "bias", 1, "f32", "gemm_kernel<x3,64,kshort,gather,64>", False, 0, 0, False),
    R("x3", 129, 68, 8, 8, "row", "bias", 1, "f32", "gemm_kernel<x3,128,kshort,gather,64>", False, 0, 0, True),
    R("x3", 65, 130, 8, 8, "off", "bias", 1, "f32", "gemm_kernel<x3,128,kshort,gather,64>", False, 0, 0, False),
    R("x3", 1, 132, 16, 4, "off", "bias", 1, "f32", "gemm_kernel<x3,128,kshort,gather,64>", False, 0, 0, True),
    R("x3", 1, 4, 8, 27, "row", "bias", 1, "f32", "gemm_kernel<x3,32,klong,gather,64>", True, 1, 0, True),
    R("x3", 64, 30, 24, 27, "off", "bias", 1, "f32", "gemm_kernel<x3,32,klong,gather,64>", False, 0, 0, False),
    R("x3", 63, 36, 64, 27, "off", "bias", 1, "f32", "gemm_kernel<x3,64,klong,gather,64>", True, 1, 0, True),
    R("x3", 64, 33, 96, 8, "row", "bias", 1, "f32", "gemm_kernel<x3,64,klong,gather,64>", False, 0, 0, False),
    R("x3", 64, 68, 32, 125, "row", "bias", 1, "f32", "gemm_kernel<x3,128,klong,gather,64>", True, 1, 0, True),
    R("x3", 1, 132, 192, 27, "off", "bias", 1, "f32", "gemm_kernel<x3,128,klong,gather,64>", True, 1, 0, True),
    R("x3", 129, 64, 64, 27, "off", "ln", 1, "f32", "gemm_kernel<x3,64,klong,gather,64>", True, 2, 0, True),
    R("x3", 129, 132, 64, 27, "row", "ln", 1, "f32", "gemm_kernel<x3,128,klong,gather,64>", True, 2, 0, True),
    R("x3", 65, 4, 8, 27, "row", "bias", 1, "f32", "gemm_kernel<x3,32,klong,gather,128>", True, 1, 0, True),
    R("x3", 129, 20, 24, 27, "off", "bias", 1, "f32", "gemm_kernel<x3,32,klong,gather,128>", True, 1, 0, True),
    R("x3", 257, 30, 32, 125, "off", "bias", 1, "f32", "gemm_kernel<x3,32,klong,gather,128>", False, 0, 0, False),
    R("x3", 65, 36, 96, 27, "off", "bias", 1, "f32", "gemm_kernel<x3,64,klong,gather,128>", True, 1, 0, True),
    R("x3", 129, 64, 128, 27, "row", "bias", 1, "f32", "gemm_kernel<x3,64,klong,gather,128>", True, 1, 0, True),
    R("x3", 257, 33, 8, 125, "row", "bias", 1, "f32", "gemm_kernel<x3,64,klong,gather,128>", False, 0, 0, False),
    R("x3", 65, 128, 64, 27, "off", "bias", 1, "f32", "gemm_kernel<x3,128,klong,gather,128>", True, 1, 0, True),
    R("x3", 129, 132, 32, 27, "row", "bias", 1, "f32", "gemm_kernel<x3,128,klong,gather,128>", True, 1, 0, True),
    R("x3", 257, 68, 24, 27, "off", "bias", 1, "f32", "gemm_kernel<x3,128,klong,gather,128>", True, 1, 0, True),
    R("x3", 129, 130, 96, 27, "off", "bias", 1, "f32", "gemm_kernel<x3,128,klong,gather,128>", False, 0, 0, False),
    R("x3", 129, 132, 192, 27, "row", "bias", 0, "f32", "gemm_kernel<x3,128,klong,gather,128>", False, 0, 0, True),
    R("x3", 257, 320, 320, 8, "off", "bias", 1, "f32", "gemm_kernel<x3,128,klong,gather,128>", True, 1, 1, True),
    R("x3", 8193, 32, 32, 27, "off", "bias", 1, "f32", "gemm_kernel<x3,32,klong,gather,128>", True, 1, 2, True),
    R("b16", 128, 68, 128, 1, "-", "bias", 1, "f32", "gemm_dma_kernel<64,plain,128,2,ring>", False, 0, 0, True),
    R("b16", 129, 65, 192, 1, "-", "bias", 1, "lp", "gemm_dma_kernel<64,plain,128,2,ring>", False, 0, 0, False),
    R("b16", 257, 132, 128, 1, "-", "bias", 1, "lp", "gemm_dma_kernel<64,plain,128,2,ring>", False, 0, 0, True),
    R("b16", 129, 260, 192, 1, "-", "bias", 1, "f32", "gemm_dma_kernel<64,plain,128,2,ring>", False, 0, 0, True),
    R("b16", 128, 132, 128, 1, "-", "ln", 1, "f32", "gemm_dma_kernel<64,plain,128,2,ring>", False, 2, 0, True),
    R("b16", 129, 512, 192, 1, "-", "ln", 1, "f32", "gemm_dma_kernel<64,plain,128,2,ring>", False, 2, 0, True),
    R("b16", 16384, 68, 128, 1, "-", "bias", 1, "f32", "gemm_dma_kernel<128,plain,128,2,ring>", False, 0, 0, True),
    R("b16", 16385, 132, 192, 1, "-", "bias", 1, "lp", "gemm_dma_kernel<128,plain,128,2,ring>", False, 0, 0, True),
    R("b16", 2048, 1024, 128, 1, "-", "bias", 1, "f32", "gemm_dma_kernel<128,plain,128,2,ring>", False, 0, 0, True),
    R("b16", 2049, 1028, 128, 1, "-", "bias", 1, "lp", "gemm_dma_kernel<128,plain,128,2,ring>", False, 0, 0, True),
    R("b16", 2049, 1026, 128, 1, "-", "bias", 1, "f32", "gemm_dma_kernel<128,plain,128,2,ring>", False, 0, 0, False),
    R("b16", 16383, 68, 128, 1, "-", "bias", 1, "f32", "gemm_dma_kernel<64,plain,128,2,ring>", False, 0, 0, True),
    R("b16", 2047, 1024, 128, 1, "-", "bias", 1, "f32", "gemm_dma_kernel<64,plain,128,2,ring>", False, 0, 0, True),
    R("b16", 128, 68, 64, 27, "row", "bias", 1, "f32", "gemm_dma_kernel<128,gather,128,2,ring>", True, 1, 0, True),
    R("b16", 129, 128, 64, 27, "off", "bias", 1, "lp", "gemm_dma_kernel<128,gather,128,2,ring>", True, 1, 0, True),
    R("b16", 257, 132, 128, 8, "off", "bias", 1, "f32", "gemm_dma_kernel<128,gather,128,2,ring>", True, 1, 0, True),
    R("b16", 129, 65, 256, 27, "row", "bias", 1, "f32", "gemm_dma_kernel<128,gather,128,2,ring>", False, 0, 0, False),
    R("b16", 129, 260, 512, 8, "off", "bias", 0, "f32", "gemm_dma_kernel<128,gather,128,2,ring>", False, 0, 0, True),
    R("b16", 257, 128, 128, 27, "off", "bias", 0, "lp", "gemm_dma_kernel<128,gather,128,2,ring>", False, 0, 0, True),
    R("b16", 127, 128, 64, 27, "off", "bias", 1, "f32", "gemm_kernel<b16,128,klong,gather,128>", True, 1, 0, True),
    R("b16", 129, 512, 512, 27, "off", "bias", 1, "f32", "gemm_dma_kernel<128,gather,128,2,ring>", True, 1, 1, True),
    R("b16", 8193, 68, 64, 8, "off", "bias", 1, "f32", "gemm_dma_kernel<128,gather,128,2,ring>", True, 1, 2, True),
    R("b16", 512, 320, 320, 27, "off", "bias", 1, "f32", "gemm_kernel<b16,128,klong,gather,256>", True, 1, 1, True),
    R("b16", 513, 320, 320, 27, "row", "bias", 1, "lp", "gemm_kernel<b16,128,klong,gather,256>", True, 1, 1, True),
    R("b16", 769, 320, 320, 27, "off", "bias", 0, "f32", "gemm_kernel<b16,128,klong,gather,256>", False, 0, 0, True),
    R("b16", 512, 256, 192, 27, "off", "bias", 1, "lp", "gemm_kernel<b16,128,klong,gather,256>", True, 1, 1, True),
    R("b16", 513, 258, 96, 27, "row", "bias", 1, "f32", "gemm_kernel<b16,128,klong,gather,256>", False, 0, 0, False),
    R("b16", 769, 256, 32, 125, "off", "bias", 0, "f32", "gemm_kernel<b16,128,klong,gather,256>", False, 0, 0, True),
    R("b16", 511, 320, 320, 27, "off", "bias", 1, "f32", "gemm_kernel<b16,128,klong,gather,128>", True, 1, 1, True),
    R("b16", 5000, 256, 64, 27, "off", "bias", 1, "lp", "gemm_dma_kernel<256,gather,256,2,sq>", True, 1, 0, True),
    R("b16", 5001, 512, 64, 27, "row", "bias", 1, "f32", "gemm_dma_kernel<256,gather,256,2,sq>", True, 1, 0, True),
    R("b16", 5121, 256, 128, 27, "off", "bias", 1, "f32", "gemm_dma_kernel<256,gather,256,2,sq>", True, 1, 0, True),
    R("b16", 5121, 512, 64, 27, "off", "bias", 1, "lp", "gemm_dma_kernel<256,gather,256,2,sq>", True, 1, 0, True),
    R("b16", 4999, 256, 64, 27, "off", "bias", 1, "f32", "gemm_dma_kernel<128,gather,128,2,ring>", True, 1, 0, True),
    R("b16", 5000, 256, 64, 27, "off", "bias", 0, "f32", "gemm_dma_kernel<128,gather,128,2,ring>", False, 0, 0, True),
    R("b16", 5000, 260, 64, 27, "off", "bias", 1, "f32", "gemm_dma_kernel<128,gather,128,2,ring>", True, 1, 0, True),
    R("b16", 16385, 256, 64, 27, "off", "bias", 1, "lp", "gemm_dma_kernel<256,gather,256,2,sq>", True, 1, 2, True),
    R("b16", 8000, 128, 64, 27, "off", "bias", 1, "lp", "gemm_dma_kernel<256,gather,128,2,sq>", True, 1, 0, True),
    R("b16", 8001, 128, 64, 27, "row", "bias", 0, "f32", "gemm_dma_kernel<256,gather,128,2,sq>", False, 0, 0, True),
    R("b16", 8193, 128, 128, 27, "off", "bias", 0, "lp", "gemm_dma_kernel<256,gather,128,2,sq>", False, 0, 0, True),
    R("b16", 32767, 128, 64, 27, "off", "bias", 0, "lp", "gemm_dma_kernel<256,gather,128,2,sq>", False, 0, 2, True),
    R("b16", 32768, 128, 64, 27, "off", "bias", 0, "lp", "gemm_dma_kernel<128,gather,128,2,ring>", False, 0, 2, True),
    R("b16", 7999, 128, 64, 27, "off", "bias", 1, "f32", "gemm_dma_kernel<128,gather,128,2,ring>", True, 1, 0, True),
]

# Compiled but behind a constant of the product build that is "off": no caller can reach them, so no case can.  name -> reason
OFF = {
    "gemm_dma_kernel<128,gather,256,3,ring>": "CDSEG_CONV_WIDE = 0 in the product build",
    "gemm_kernel<x3,32,kshort,plain,128>": "CDSEG_X3_TALL_MIN_M = 0",
    "gemm_kernel<x3,64,kshort,plain,128>": "CDSEG_X3_TALL_MIN_M = 0",
    "gemm_kernel<x3,128,kshort,plain,128>": "CDSEG_X3_TALL_MIN_M = 0",
    "gemm_kernel<x3,32,klong,plain,128>": "CDSEG_X3_TALL_MIN_M = 0",
    "gemm_kernel<x3,64,klong,plain,128>": "CDSEG_X3_TALL_MIN_M = 0",
    "gemm_kernel<x3,128,klong,plain,128>": "CDSEG_X3_TALL_MIN_M = 0",
    # the row tile of the LDS-DMA loop is 64 (plain, few rows) or 128 (plain with many rows, every gathered call) unless
    # CDSEG_GEMM_DMA_BM forces one
    "gemm_dma_kernel<256,plain,128,2,ring>": "CDSEG_GEMM_DMA_BM = 0",
    "gemm_dma_kernel<64,gather,128,2,ring>": "CDSEG_GEMM_DMA_BM = 0",
    "gemm_dma_kernel<256,gather,128,2,ring>": "CDSEG_GEMM_DMA_BM = 0",
}

# The catalogue's kernels outside cdseg_gemm that no caller can reach either (every other one of them is asserted from the record
# by a test: tests/test_gpu_ops.py, test_gpu_cpe_head_stream.py, test_gpu_deep512_rows64.py, test_gpu_attention_range.py)
OFF_OTHER = {
    "cpe_head_fused_kernel<32,128>": "CDSEG_HEAD_STREAM = 1: from 65 536 rows the persistent kernel runs, below them the 64-row one",
    "cpe_head_fused_kernel<64,128>": "CDSEG_HEAD_STREAM = 1: from 65 536 rows the persistent kernel runs, below them the 64-row one",
}

F32, B16, X3 = 0, 1, 2  # include/cdseg.h CDSEG_F32 / CDSEG_BF16 / CDSEG_F32X3
CPU_REF_MACS = 1e8      # above this the fp64 reference runs on the device (rocBLAS, independent of this library)


def report(name, **kw):
    print(f"[measure] {name}: " + ", ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in kw.items()))


def _variants(c):
    return ("bf16", "f16") if c.ct == "b16" else ("bf16",)  # fp32 / fp32x3 kernels do not depend on the 16-bit type


def _id(c, variant):
    return (f"{variant}-{c.ct}-{c.M}x{c.N}x{c.K}" + (f"-kvol{c.kvol}{c.lay}" if c.lay != "-" else "") +
            (f"-{c.epi}" if c.epi != "bias" else "") + ("" if c.ws else "-nows") + ("-out16" if c.out == "lp" else ""))


PARAMS = [pytest.param(c, v, id=_id(c, v)) for c in ROUTE_CASES for v in _variants(c)]
assert len({p.id for p in PARAMS}) == len(PARAMS), "two cases with the same id"


def _lp(variant):
    return torch.bfloat16 if variant == "bf16" else torch.float16


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _random_map(c, g, n_src):
    """(kvol, M) int32 as test_deep_conv_group_skipping_random_map builds it: -1 entries, whole dead 16-row groups, one
    offset nobody has (from four offsets up), tiles with few live offsets; M is never a multiple of every tile."""
    M, kvol = c.M, c.kvol
    ngrp = (M + 15) // 16
    grp_on = torch.rand(kvol, ngrp, generator=g) > 0.35
    if kvol >= 4:
        grp_on[3] = False
    if ngrp >= 7:
        grp_on[:, : ngrp // 7] &= torch.rand(kvol, 1, generator=g) > 0.5
    row_on = (torch.rand(kvol, M, generator=g) > 0.5) & grp_on.repeat_interleave(16, dim=1)[:, :M]
    if kvol < 4:
        row_on[:, 0] = True  # (a map of one to three offsets keeps something alive)
    return torch.where(row_on, torch.randint(0, n_src, (kvol, M), generator=g), torch.full((kvol, M), -1)).int()


def _args(c, variant, A, W, out, *, bias=None, nbr=None, ws=None, res=None, ln=None, ln_out=None):
    a = _lib.GemmArgs()
    lp = _lp(variant)
    dt = lambda t: B16 if t.dtype == lp else F32
    assert all(t.dtype in (lp, torch.float32) for t in (A, W, out))
    a.A, a.W, a.out = A.data_ptr(), W.data_ptr(), out.data_ptr()
    a.bias = bias.data_ptr() if bias is not None else None
    a.M, a.N, a.K, a.kvol = c.M, c.N, c.K, c.kvol
    a.lda, a.ldo = A.stride(0), out.stride(0)
    a.a_dtype, a.out_dtype = dt(A), dt(out)
    a.compute_dtype = {"b16": B16, "f32": F32, "x3": X3}[c.ct]
    if nbr is not None:
        a.nbr, a.nbr_kmajor = nbr.data_ptr(), 1 if c.lay == "off" else 0
    if ws is not None:
        a.ws, a.ws_bytes = ws.data_ptr(), ws.numel()
    if res is not None:
        a.res, a.ldres = res.data_ptr(), res.stride(0)
    if ln is not None:
        a.ln_post_g, a.ln_post_b = ln[0].data_ptr(), ln[1].data_ptr()
        a.ln_out, a.ldln, a.ln_out_dtype, a.ln_eps = ln_out.data_ptr(), ln_out.stride(0), F32, 1e-5
    return a


def _launch(lib, a):
    """cdseg_gemm with recording on -> (status, launches recorded, records)."""
    from cdsegnet_amd import ops
    prev = lib.cdseg_route_enable(1)
    lib.cdseg_route_clear()
    rc = lib.cdseg_gemm(ctypes.byref(a), _stream())
    count, routes = ops.route_read(lib)
    lib.cdseg_route_enable(prev)
    return rc, count, routes


def _route_of(r):
    return (r.kernel, r.splits > 1, r.fix, r.xmode, r.vec_ok)


def _check_flags(c, r):
    """The rest of the record, which follows from the case itself."""
    pow2 = c.K & (c.K - 1) == 0
    assert r.gather == (c.lay != "-") and r.compute == {"b16": B16, "f32": F32, "x3": X3}[c.ct]
    assert r.kdiv == (not pow2) and r.kshift_lt6 == (pow2 and c.K < 64) and not r.partials
    f = r.kernel.split("<")[1].rstrip(">").split(",")  # gemm_kernel<ct,bn,k,g,bm> / gemm_dma_kernel<bm,g,bn,stages,loop>
    bm, bn = (int(f[4]), int(f[1])) if r.kernel.startswith("gemm_kernel<") else (int(f[0]), int(f[2]))
    assert (r.bm, r.bn) == (bm, bn)


@pytest.mark.parametrize("c,variant", PARAMS)
def test_gemm_route_vs_fp64(c, variant):
    lp = _lp(variant)
    op_dt = lp if c.ct == "b16" else torch.float32
    gather = c.lay != "-"
    ktot = c.kvol * c.K
    g = torch.Generator().manual_seed(c.M * 7919 + c.N * 31 + c.K + c.kvol)
    n_src = c.M // 2 + 5 if gather else c.M  # the gather source is not the output's row count
    A = torch.randn(n_src, c.K, generator=g)
    if c.ct == "x3":
        A[:, ::3] *= 1e-4  # small activations next to O(1) ones (not representable in 16 bits either way)
    W = torch.randn(c.N, ktot, generator=g) / ktot ** 0.5
    bias = torch.randn(c.N, generator=g)
    if c.ct == "b16":  # operands already rounded to the build's 16-bit type
        A, W = A.to(lp).float(), W.to(lp).float()
    nbr = _random_map(c, g, n_src) if gather else None
    res = torch.randn(c.M, c.N, generator=g) if c.epi == "ln" else None
    lng, lnb = 1 + 0.1 * torch.randn(c.N, generator=g), 0.1 * torch.randn(c.N, generator=g)

    # ---- fp64 reference: gather + matmul per offset
    on_dev = float(c.M) * c.N * ktot > CPU_REF_MACS
    rd = "cuda" if on_dev else "cpu"
    A64, W64 = A.to(rd).double(), W.to(rd).double().view(c.N, c.kvol, c.K)
    ref = bias.to(rd).double().repeat(c.M, 1)
    if gather:
        nb = nbr.to(rd).long()
        for o in range(c.kvol):
            rows = torch.where((nb[o] >= 0)[:, None], A64[nb[o].clamp(min=0)], torch.zeros((), dtype=torch.float64, device=rd))
            ref += rows @ W64[:, o, :].t()
    else:
        ref += A64 @ W64[:, 0, :].t()
    if res is not None:
        ref += res.to(rd).double()
    ref = ref.cpu()

    # ---- the call: out in guard bands, A in NaN guards, the workspace exact
    Ad, a_band = poisoned_input(A.cuda().to(op_dt), name="A")
    Wd, bd = W.cuda().to(op_dt).contiguous(), bias.cuda()
    out_dt = lp if c.out == "lp" else torch.float32
    out, o_band = banded((c.M, c.N), out_dt, fill=-77.0, name="out")
    nd = None
    if gather:
        nd = (nbr if c.lay == "off" else nbr.t()).contiguous().cuda()
    ws = wsb = None
    if c.ws:
        ws, wsb = exact_workspace(16 * c.M * c.N * 4)
    resd = res.cuda() if res is not None else None
    ln_out = l_band = None
    if c.epi == "ln":
        ln_out, l_band = banded((c.M, c.N), torch.float32, fill=-55.0, name="ln_out")
    lib = _lib.load(variant)
    a = _args(c, variant, Ad, Wd, out, bias=bd, nbr=nd, ws=ws, res=resd,
              ln=(lng.cuda(), lnb.cuda()) if c.epi == "ln" else None, ln_out=ln_out)
    rc, count, routes = _launch(lib, a)
    assert rc == 0, _lib.ERRORS.get(rc, rc)
    torch.cuda.synchronize()
    for b in (o_band, a_band, l_band, wsb):
        if b is not None:
            b.check()

    # ---- numbers
    got = out.double().cpu()
    err = (got - ref).abs().max().item()
    bound = 2e-5 * ktot ** 0.5 + 1e-5
    extra = {}
    if c.ct == "x3":
        exact, e_band = banded((c.M, c.N), torch.float32, fill=-77.0, name="exact")
        c32 = c._replace(ct="f32")
        a32 = _args(c32, variant, Ad, Wd, exact, bias=bd, nbr=nd, ws=ws, res=resd,
                    ln=(lng.cuda(), lnb.cuda()) if c.epi == "ln" else None, ln_out=ln_out.clone() if ln_out is not None else None)
        assert lib.cdseg_gemm(ctypes.byref(a32), _stream()) == 0
        torch.cuda.synchronize()
        e_band.check()
        err32 = (exact.double().cpu() - ref).abs().max().item()
        extra["exact_fp32_err"] = err32
        bound = min(2 * bound, 8 * err32 + 2e-6)
    tol = bound + (ref.abs() * (2.0 ** -8 if lp == torch.bfloat16 else 2.0 ** -11) if c.out == "lp" else 0.0)
    worst = ((got - ref).abs() / tol).max().item()
    report(f"route gemm {_id(c, variant)}", max_err=err, bound=bound, err_over_bound=worst, kernel=routes[0].kernel if routes else "-",
           splits=routes[0].splits if routes else 0, **extra)
    assert not got.isnan().any(), "a NaN reached the output: an operand was read outside its rows"
    assert worst < 1.0, (err, bound)
    if c.epi == "ln":
        y = torch.nn.functional.layer_norm(ref, (c.N,), None, None, 1e-5)
        s_min = ref.std(dim=1, unbiased=False).min().item()
        y_max = y.abs().max().item()
        d = 2e-5 * ktot ** 0.5 + 1e-5
        if c.ct == "x3":
            d *= 2
        ln_bound = lng.abs().max().item() * (1.05 * (2 * d / s_min) * (1 + y_max) + 4e-6 * (1 + y_max)) + 1e-6
        ln_err = (ln_out.double().cpu() - (y * lng.double() + lnb.double())).abs().max().item()
        report(f"route gemm {_id(c, variant)} ln_out", max_err=ln_err, bound=ln_bound, err_over_bound=ln_err / ln_bound)
        assert ln_err < ln_bound

    # ---- the route
    assert count == 1 and len(routes) == 1, (count, routes)
    assert _route_of(routes[0]) == (c.kernel, c.split, c.fix, c.xmode, c.vec), routes[0]
    _check_flags(c, routes[0])


@pytest.mark.parametrize("variant", _lib.VARIANTS)
def test_every_compiled_gemm_variant_is_reached_or_accounted_for(variant):
    """Self-contained: replays the LAUNCHES of ROUTE_CASES (zero operands, valid all -1 maps, no reference), collects the
    recorded kernels and holds them against the catalogue of compiled GEMM kernels minus OFF."""
    from cdsegnet_amd import ops
    lib = _lib.load(variant)
    lp = _lp(variant)
    catalogue = {n for n in ops.route_catalog(lib) if n.startswith(("gemm_kernel<", "gemm_dma_kernel<"))}
    assert set(OFF) <= catalogue, set(OFF) - catalogue  # a reason for a kernel that is not compiled is stale
    assert set(OFF_OTHER) <= set(ops.route_catalog(lib)) - catalogue
    reached = {}
    for c in ROUTE_CASES:
        op_dt = lp if c.ct == "b16" else torch.float32
        gather = c.lay != "-"
        A = torch.zeros(c.M // 2 + 5 if gather else c.M, c.K + 8, dtype=op_dt, device="cuda")[:, :c.K]
        W = torch.zeros(c.N, c.kvol * c.K, dtype=op_dt, device="cuda")
        out = torch.zeros(c.M, (c.N + 7) // 8 * 8, dtype=lp if c.out == "lp" else torch.float32, device="cuda")[:, :c.N]
        nbr = torch.full((c.kvol, c.M) if c.lay == "off" else (c.M, c.kvol), -1, dtype=torch.int32, device="cuda") if gather else None
        ws = torch.empty(16 * c.M * c.N * 4, dtype=torch.uint8, device="cuda") if c.ws else None
        res = torch.zeros(c.M, c.N, device="cuda") if c.epi == "ln" else None
        ln = (torch.ones(c.N, device="cuda"), torch.zeros(c.N, device="cuda")) if c.epi == "ln" else None
        a = _args(c, variant, A, W, out, bias=torch.zeros(c.N, device="cuda"), nbr=nbr, ws=ws, res=res, ln=ln,
                  ln_out=torch.empty(c.M, c.N, device="cuda") if ln else None)
        rc, count, routes = _launch(lib, a)
        assert rc == 0 and count == 1, (c, rc, count)
        reached.setdefault(routes[0].kernel, c)
    torch.cuda.synchronize()
    assert not (set(reached) - catalogue), "a recorded name the catalogue does not have"
    reached_off = {k: reached[k] for k in reached if k in OFF}
    assert not reached_off, f"listed as switched off, yet a case reaches it: {reached_off}"
    missing = sorted(catalogue - set(reached) - set(OFF))
    assert not missing, f"compiled GEMM kernels that no case of ROUTE_CASES runs and OFF does not explain: {missing}"
    # and the table itself claims nothing else
    assert {c.kernel for c in ROUTE_CASES} == set(reached)


@pytest.mark.parametrize("variant", _lib.VARIANTS)
def test_layernorm_epilogue_refuses_rows_wider_than_512_before_any_launch(variant):
    """include/cdseg.h: the fused LayerNorm finishes complete rows through the workspace up to N = 512; wider rows are
    CDSEG_ERR_UNSUPPORTED - nothing is launched, nothing is recorded and the outputs keep their fill."""
    lp = _lp(variant)
    lib = _lib.load(variant)
    for ct in ("b16", "f32", "x3"):
        c = R(ct, 65, 516, 128, 1, "-", "ln", 1, "f32", None, False, 0, 0, True)
        op_dt = lp if ct == "b16" else torch.float32
        A = torch.ones(c.M, c.K, dtype=op_dt, device="cuda")
        W = torch.ones(c.N, c.K, dtype=op_dt, device="cuda")
        out, o_band = banded((c.M, c.N), torch.float32, fill=-77.0, name="out")
        ln_out, l_band = banded((c.M, c.N), torch.float32, fill=-55.0, name="ln_out")
        ws, wsb = exact_workspace(16 * c.M * c.N * 4)
        a = _args(c, variant, A, W, out, bias=torch.zeros(c.N, device="cuda"), ws=ws, res=torch.zeros(c.M, c.N, device="cuda"),
                  ln=(torch.ones(c.N, device="cuda"), torch.zeros(c.N, device="cuda")), ln_out=ln_out)
        rc, count, routes = _launch(lib, a)
        torch.cuda.synchronize()
        assert rc == -4 and count == 0, (ct, rc, count)
        assert bool((out == -77.0).all()) and bool((ln_out == -55.0).all())
        o_band.check(); l_band.check(); wsb.check()
        assert bool((ws == 0xA5).all()), "the workspace was written"
