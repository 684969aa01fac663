#!/usr/bin/env python3
"""SerializedUnpooling (mode "add") of the two wide n-decoder stages on the shapes of a collated forward: the two cdseg_gemm
launches (child projection to fp32, skip projection with the gathered add) against cdseg_unpool_fused (csrc/pool.hip).
The skip inputs rotate through three copies so that a launch finds its rows in HBM, not in the last-level cache.
usage: python tools/bench_unpool.py [scenes=24] [f16|bf16]"""
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
    for name, n, m, ks, kp, c in (("n_dec0.up", 120000 * scenes, 55818 * scenes, 32, 64, 64),
                                  ("n_dec1.up", 55818 * scenes, 14293 * scenes, 64, 128, 64)):
        runs = torch.full((m,), n // m, dtype=torch.int64)
        runs[: n - int(runs.sum())] += 1
        runs = runs[torch.randperm(m, generator=g)]
        seg = torch.cat([torch.zeros(1, dtype=torch.int64), runs.cumsum(0)]).int().to(dev)
        cluster = torch.repeat_interleave(torch.arange(m), runs).int().to(dev)
        xs = [torch.randn(n, ks, device=dev).to(T) for _ in range(3)]
        xp = torch.randn(m, kp, device=dev).to(T)
        ws, wp = (torch.randn(c, ks, device=dev) / ks ** 0.5).to(T), (torch.randn(c, kp, device=dev) / kp ** 0.5).to(T)
        ps = [torch.randn(c, device=dev), torch.rand(c, device=dev) + 0.5, torch.randn(c, device=dev)]
        pp = [torch.randn(c, device=dev), torch.rand(c, device=dev) + 0.5, torch.randn(c, device=dev)]
        img_s, img_p = ops.unpool_fused_pack(ws), ops.unpool_fused_pack(wp)
        child = torch.empty(m, c, device=dev)
        x, xc = torch.empty(n, c, device=dev), torch.empty(n, c, dtype=T, device=dev)
        k = [0]

        def skip():
            k[0] += 1
            return xs[k[0] % 3]

        t_c = time_op(lambda: ops.gemm(xp, wp, child, bias=pp[0], scale=pp[1], shift=pp[2], act=ops.ACT_GELU), 12)
        t_s = time_op(lambda: ops.gemm(skip(), ws, x, bias=ps[0], scale=ps[1], shift=ps[2], act=ops.ACT_GELU, add_src=child,
                                       add_idx=cluster, out2=xc, out2_pre_add=True), 12)
        t_f = time_op(lambda: ops.unpool_fused(skip(), img_s, *ps, xp, img_p, *pp, seg, m, ops.ACT_GELU, x, xc), 12)
        mb = (n * (ks * 2 + c * 6) + m * kp * 2) / 1e6
        print(f"{variant} {name}: n={n} m={m} ({ks}, {kp}, {c}): child gemm {t_c:.1f} + skip gemm {t_s:.1f} = {t_c + t_s:.1f} us; "
              f"fused {t_f:.1f} us ({mb / t_f:.2f} TB/s on {mb:.0f} MB)", flush=True)
