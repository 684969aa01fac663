#!/usr/bin/env python3
"""Train-mode BatchNorm + GELU and the pooling maximum, forward + backward per site: the kernels of csrc/norm.hip
(`model.train_norm = "fused"`) against the torch chain they replace, at the site shapes of a 120 k-point ScanNet scene.
Fused and torch alternate in one process; HIP events; median (min - max) of `runs` timed repetitions after a warm-up.
Achieved bytes/s are counted from the shapes (fp32): BatchNorm + GELU forward 12 bytes an element (x twice, y once), backward
20 (x and dy twice, dx once); pooling maximum forward n c 4 + m c 8, backward n c 4 + m c 8 + n 4.
usage: python tools/bench_norm.py [runs=11]"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cdsegnet_amd import train_graph as tg  # noqa: E402

RUNS = int(sys.argv[1]) if len(sys.argv) > 1 else 11
assert RUNS >= 9
# (rows, channels): stem and the four pooling norms, then the unpooling pairs (child rows at the coarse level, skip rows at the fine)
BN_SITES = [("stem", 120000, 32), ("pool 1", 52200, 64), ("pool 2", 14640, 128), ("pool 3", 3804, 256), ("pool 4", 991, 512),
            ("unpool 3 child", 991, 256), ("unpool 3 skip", 3804, 256), ("unpool 2 child", 3804, 128), ("unpool 2 skip", 14640, 128),
            ("unpool 1 child", 14640, 64), ("unpool 1 skip", 52200, 64), ("unpool 0 child", 52200, 64), ("unpool 0 skip", 120000, 64)]
POOL_SITES = [("pool 1", 120000, 52200, 64), ("pool 2", 52200, 14640, 128), ("pool 3", 14640, 3804, 256), ("pool 4", 3804, 991, 512)]


def timed(fn):
    """(forward ms, backward ms) of one repetition; fn() -> (output, gradient to feed)."""
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    e[0].record()
    y, dy = fn()
    e[1].record()
    y.backward(dy)
    e[2].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])


def compare(name, variants, fwd_bytes, bwd_bytes):
    t = {k: [] for k in variants}
    for rep in range(RUNS + 2):
        for k, fn in variants.items():  # alternate
            r = timed(fn)
            if rep >= 2:
                t[k].append(r)
    line = [f"{name:28s}"]
    for k in variants:
        a = np.array(t[k]) * 1e3  # us
        for j, (what, nbytes) in enumerate((("fwd", fwd_bytes), ("bwd", bwd_bytes))):
            med = float(np.median(a[:, j]))
            line.append(f"{k} {what} {med:7.1f} us ({a[:, j].min():.1f} - {a[:, j].max():.1f}) {nbytes / med / 1e6:6.2f} TB/s")
    print(" | ".join(line), flush=True)


def main():
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    print(f"fused against torch per site, forward + backward, {RUNS} runs each, median (min - max)")
    for name, m, c in BN_SITES:
        x = (0.5 + torch.randn(m, c, generator=g)).to(dev).requires_grad_(True)
        dy = torch.randn(m, c, generator=g).to(dev)
        bn = torch.nn.BatchNorm1d(c, eps=1e-3, momentum=0.01).to(dev).train()

        def run(mode):
            x.grad = bn.weight.grad = bn.bias.grad = None
            return tg._bn_gelu(x, bn, mode), dy

        compare(f"bn+gelu {name} {m}x{c}", {"fused": lambda: run("fused"), "torch": lambda: run("torch")}, 12 * m * c, 20 * m * c)
    for name, n, m, c in POOL_SITES:
        # synthetic link: every pooled row gets n // m children, the first n % m one more (contiguous, like the plan's)
        lens = torch.full((m,), n // m, dtype=torch.int64)
        lens[: n % m] += 1
        seg = torch.zeros(n + 1, dtype=torch.int32)
        seg[1:m + 1] = lens.cumsum(0).int()
        cluster = torch.repeat_interleave(torch.arange(m, dtype=torch.int32), lens)
        seg, cluster = seg.to(dev), cluster.to(dev)
        y = torch.randn(n, c, generator=g).to(dev).requires_grad_(True)
        dout = torch.randn(m, c, generator=g).to(dev)

        def pool(fn):
            y.grad = None
            return fn.apply(y, seg, cluster, m), dout

        compare(f"segment max {name} {n}->{m}x{c}", {"fused": lambda: pool(tg._SegmentMaxArg), "torch": lambda: pool(tg._SegmentMax)},
                4 * n * c + 8 * m * c, 4 * n * c + 8 * m * c + 4 * n)


if __name__ == "__main__":
    main()
