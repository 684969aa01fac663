#!/usr/bin/env python3
"""The optimizer step alone on the full-width model's parameter tensors (508 tensors, 101.4 M parameters for scannet) with
random gradients: torch.optim.AdamW (foreach, fused=True) against cdsegnet_amd.optim.FusedAdamW (plain, with GradScaler's
grad_scale / found_inf attributes, with the in-step clip, with the 16-bit weight copies).  Every variant owns a copy of the
parameters and shares the gradients; the variants alternate inside one process, HIP events around each `step()`, median of
`reps` after a warm-up.  `host` is the wall time until `step()` returns with the device left running (no synchronisation).
Traffic floor of the update: 7 x 4 B per parameter (read p, g, m, v; write p, m, v) at the measured 6.3 TB/s copy rate.
usage: python tools/bench_optimizer.py [dataset=scannet] [reps=9]"""
import json, os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cdsegnet_amd import configs
from cdsegnet_amd.optim import FusedAdamW
from cdsegnet_amd.registry import build_model
import cdsegnet_amd.models  # noqa: F401

dataset = sys.argv[1] if len(sys.argv) > 1 else "scannet"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
dev = torch.device("cuda")
model = build_model(configs.cdsegnet_config(dataset))
shapes = [(k, tuple(p.shape)) for k, p in model.named_parameters()]
del model
gen = torch.Generator(device=dev).manual_seed(0)
grads = [torch.randn(s, device=dev, generator=gen) * 1e-2 for _, s in shapes]
init = [torch.randn(s, device=dev, generator=gen) * 0.05 for _, s in shapes]
total = sum(g.numel() for g in grads)


def groups(ps):
    blk = [p for (k, _), p in zip(shapes, ps) if "block" in k]
    rest = [p for (k, _), p in zip(shapes, ps) if "block" not in k]
    return [dict(params=rest, lr=0.002), dict(params=blk, lr=0.0002)]


def variant(name):
    ps = [torch.nn.Parameter(t.clone()) for t in init]
    for p, g in zip(ps, grads):
        p.grad = g
    kw = dict(lr=0.002, weight_decay=0.05)
    pre = None
    if name == "torch foreach":
        opt = torch.optim.AdamW(groups(ps), foreach=True, **kw)
    elif name == "torch fused":
        opt = torch.optim.AdamW(groups(ps), fused=True, **kw)
    elif name == "FusedAdamW":
        opt = FusedAdamW(groups(ps), **kw)
    elif name == "FusedAdamW + scaler":
        opt = FusedAdamW(groups(ps), **kw)
        scale, found = torch.full((), 1.0, device=dev), torch.zeros((), device=dev)

        def pre():
            opt.grad_scale, opt.found_inf = scale, found
    elif name == "FusedAdamW + clip":
        opt = FusedAdamW(groups(ps), max_grad_norm=1e9, **kw)
    elif name == "FusedAdamW + clip + shadow f16":
        opt = FusedAdamW(groups(ps), max_grad_norm=1e9, shadow16="f16", **kw)
    else:
        raise ValueError(name)
    return name, opt, pre, ps


names = ["torch foreach", "torch fused", "FusedAdamW", "FusedAdamW + scaler", "FusedAdamW + clip", "FusedAdamW + clip + shadow f16"]
variants = [variant(n) for n in names]
dev_ms = {n: [] for n in names}
host_ms = {n: [] for n in names}
for rep in range(reps + 2):
    for name, opt, pre, _ in variants:
        if pre is not None:
            pre()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        opt.step()
        e1.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        if rep >= 2:
            dev_ms[name].append(e0.elapsed_time(e1))
            host_ms[name].append((t1 - t0) * 1e3)
floor = 7 * 4 * total / 6.3e12 * 1e3
print(f"optimizer step, {dataset}: {len(shapes)} tensors, {total} parameters; traffic floor {floor:.2f} ms (28 B per parameter at 6.3 TB/s)")
out = {}
for n in names:
    d, h = np.array(dev_ms[n]), np.array(host_ms[n])
    out[n] = dict(median_ms=float(np.median(d)), min_ms=float(d.min()), max_ms=float(d.max()), host_ms=float(np.median(h)))
    print(f"  {n:34s} events: median {np.median(d):7.3f} ms (min {d.min():.3f}, max {d.max():.3f});  host until step() returns: {np.median(h):6.3f} ms")
# does step() wait for the device?  Queue ~10 ms of GEMMs in front of it and time the call alone: a step that only enqueues
# returns in its host time above, one that synchronises returns after the GEMMs
a = torch.randn(8192, 8192, device=dev)
busy = {}
for name, opt, pre, _ in variants:
    if name not in ("torch foreach", "FusedAdamW", "FusedAdamW + clip + shadow f16"):
        continue
    ts = []
    for _ in range(5):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(4):
            a @ a
        e1.record()
        t0 = time.perf_counter()
        opt.step()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        ts.append(((t1 - t0) * 1e3, e0.elapsed_time(e1)))
    busy[name] = dict(step_call_ms=float(np.median([t[0] for t in ts])), queued_ms=float(np.median([t[1] for t in ts])))
    print(f"  {name:34s} step() call behind {busy[name]['queued_ms']:.1f} ms of queued GEMMs returns after {busy[name]['step_call_ms']:.3f} ms")
print(json.dumps(dict(metric="optimizer_step_ms", dataset=dataset, tensors=len(shapes), parameters=total, floor_ms=floor, variants=out, behind_queued_work=busy)))
