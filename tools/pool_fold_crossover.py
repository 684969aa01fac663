#!/usr/bin/env python3
"""Where the two folds of cdseg_pool_fused_n cross (csrc/pool.hip POOL_SCAN_RATIO): the strip walk against the segmented
maximum across the child lanes, each forced through ops.pool_fused_fold, at mean run lengths 2, 4, 8 and 16 on the fine row
counts of a collated 24-scene forward, next to cdseg_gemm + cdseg_segment_max.  Runs are n / m or n / m + 1 children, shuffled.
The inputs rotate through three copies so that a launch finds its rows in HBM, not in the 256 MiB last-level cache.
usage: python tools/pool_fold_crossover.py [scenes=24] [f16|bf16]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdsegnet_amd import _lib, ops  # noqa: E402
from tools.bench_gemm import time_op  # noqa: E402

scenes = int(sys.argv[1]) if len(sys.argv) > 1 else 24
variant = sys.argv[2] if len(sys.argv) > 2 else "f16"
T = torch.float16 if variant == "f16" else torch.bfloat16
dev = torch.device("cuda")
g = torch.Generator().manual_seed(0)
with _lib.use(variant):
    for n, cin, cout in ((120000 * scenes, 32, 64), (55818 * scenes, 64, 128)):
        w = (torch.randn(cout, cin, device=dev) / cin ** 0.5).to(T)
        b, sc, sh = torch.randn(cout, device=dev), torch.rand(cout, device=dev) + 0.5, torch.randn(cout, device=dev)
        img = ops.pool_fused_pack(w)
        xs = [torch.randn(n, cin, device=dev).to(T) for _ in range(3)]
        y = torch.empty(n, cout, dtype=T, device=dev)
        for ratio in (2, 4, 8, 16):
            m = n // ratio
            runs = torch.full((m,), n // m, dtype=torch.int64)
            runs[: n - int(runs.sum())] += 1
            runs = runs[torch.randperm(m, generator=g)]
            seg = torch.cat([torch.zeros(1, dtype=torch.int64), runs.cumsum(0)]).int().to(dev)
            o1, o2 = torch.empty(m, cout, device=dev), torch.empty(m, cout, dtype=T, device=dev)
            k = [0]

            def x():
                k[0] += 1
                return xs[k[0] % 3]

            t_g = time_op(lambda: ops.gemm(x(), w, y, bias=b), 12)
            t_s = time_op(lambda: ops.segment_max(y, seg, m, sc, sh, ops.ACT_GELU, o1, o2), 12)
            t = {}
            for name, fold in (("walk", ops.POOL_FOLD_WALK), ("scan", ops.POOL_FOLD_SCAN)):
                with ops.pool_fused_fold(fold):
                    t[name] = time_op(lambda: ops.pool_fused(x(), img, b, seg, m, sc, sh, ops.ACT_GELU, o1, o2), 12)
            mb = (n * cin * 2 + m * cout * 6) / 1e6
            print(f"{variant} {cin}->{cout} n={n} ratio {ratio:2d} m={m}: gemm {t_g:.1f} + segment max {t_s:.1f} = {t_g + t_s:.1f} us; "
                  f"walk {t['walk']:.1f} us ({mb / t['walk']:.2f} TB/s), scan {t['scan']:.1f} us ({mb / t['scan']:.2f} TB/s) "
                  f"on {mb:.0f} MB", flush=True)
