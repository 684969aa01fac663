#!/usr/bin/env python3
"""Weight gradient dW = dY^T X: the fp32 kernel (cdseg_linear_wgrad / cdseg_conv_wgrad) against the 16-bit one
(cdseg_linear_wgrad16 / cdseg_conv_wgrad16, both builds) in one process, HIP events around each call, dw / db zeroed outside
the timed region.  Dense shapes: qkv / fc1 / fc2 at the five stage widths with the row counts tools/bench_train_block.py
uses; conv form at C = 32 .. 512 on a synthetic room's kernel map (the room thinned to the stage's row count) and the stem
(6 -> 16 padded channels, 125 offsets, 32 outputs).
usage: python tools/bench_wgrad.py [reps=9] [variants=f16,bf16]
Prints median (min - max) in ms per shape and the ratio fp32 / 16-bit."""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cdsegnet_amd import _lib, ops, synth

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
variants = sys.argv[2].split(",") if len(sys.argv) > 2 else ["f16", "bf16"]
dev = torch.device("cuda")
STAGES = [(32, 120000), (64, 56000), (128, 20000), (256, 6000), (512, 1500)]
g = torch.Generator().manual_seed(0)


def rnd(*sh, s=1.0):
    return (torch.randn(*sh, generator=g) * s).to(dev)


def events(fn, make_out):
    ms = []
    for _ in range(reps + 2):
        out = make_out()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ops.bind_stream()
        e0.record()
        fn(*out)
        e1.record()
        ops.unbind_stream()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = sorted(ms[2:])
    return ms[len(ms) // 2], ms[0], ms[-1]


def fmt(r):
    return f"{r[0]:8.3f} ({r[1]:.3f} - {r[2]:.3f})"


def row(name, x, dy, make_out, call):
    """call(x, dy, *out) in fp32 and in every 16-bit variant on the same values (rounded)."""
    base = events(lambda *o: call(x, dy, *o), make_out)
    line = f"{name:34s} fp32 {fmt(base)}"
    for v in variants:
        with _lib.use(v):
            x16, dy16 = ops.cast(x, ops.LP_DTYPES[v]), ops.cast(dy, ops.LP_DTYPES[v])
            r = events(lambda *o: call(x16, dy16, *o), make_out)
        line += f" | {v} {fmt(r)} = {base[0] / r[0]:5.2f}x"
    print(line, flush=True)


def kernel_map(n_req, ksize):
    sc = synth.room_scene(3, n_req)
    grid = torch.as_tensor(sc["grid_coord"]).to(dev).int().contiguous()
    n = grid.shape[0]
    batch = torch.zeros(n, dtype=torch.int32, device=dev)
    depth = int(ops.grid_max(grid.long()).item()).bit_length()
    zs, perm0 = ops.sort_pairs(ops.encode(grid.long(), batch.long(), depth, "z"))
    gz = ops.gather_rows(grid, perm0)
    return ops.nbr_table(zs, gz, batch, depth, ksize, True).contiguous()


print(f"weight gradient, ms: median (min - max) of {reps} runs; ratio = fp32 median / 16-bit median")
for C, M in STAGES:
    for name, K, N in (("qkv", C, 3 * C), ("fc1", C, 4 * C), ("fc2", 4 * C, C)):
        x, dy = rnd(M, K), rnd(M, N, s=0.1)
        row(f"{name} C={C} M={M} dW {N}x{K}", x, dy,
            lambda: (torch.zeros(N, K, device=dev), torch.zeros(N, device=dev)),
            lambda a, b, dw, db: ops.linear_wgrad(a, b, dw, db))
for C, M in STAGES:
    nbr = kernel_map(M, 3)
    n = nbr.shape[1]
    live = float((nbr >= 0).float().mean()) * 27
    x, dy = rnd(n, C), rnd(n, C, s=0.1)
    row(f"conv C={C} M={n} ({live:.1f} of 27 live)", x, dy,
        lambda: (torch.zeros(C, 27, C, device=dev), torch.zeros(C, device=dev)),
        lambda a, b, dw, db: ops.conv_wgrad(a, nbr, b, dw, db))
nbr = kernel_map(120000, 5)
n = nbr.shape[1]
x, dy = rnd(n, 16), rnd(n, 32, s=0.1)
x[:, 6:] = 0
row(f"stem 16->32 k=5 M={n}", x, dy, lambda: (torch.zeros(32, 125, 16, device=dev),),
    lambda a, b, dw: ops.conv_wgrad(a, nbr, b, dw, None))
