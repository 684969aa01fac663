#!/usr/bin/env python3
"""The segmentation loss alone (cross entropy + multi-class Lovasz-Softmax, forward and backward) under HIP events, for both
paths: the torch criteria of cdsegnet_amd/losses.py and the fused HIP loss (losses.FusedCriteria -> csrc/loss.hip).
usage: python tools/bench_loss.py [points=120000,480000] [classes=16,20,200] [repeats=9] [paths=torch,fused]
Per (points, classes): median of `repeats` timed forward+backward passes after one warm-up, min - max, for each path, and the
fused path's forward / backward split.  Logits are random normal, labels uniform over the classes with 1 row in 10 ignored."""
import os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cdsegnet_amd.losses import build_criteria

points = [int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "120000,480000").split(",")]
classes = [int(v) for v in (sys.argv[2] if len(sys.argv) > 2 else "16,20,200").split(",")]
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 9
paths = (sys.argv[4] if len(sys.argv) > 4 else "torch,fused").split(",")  # (one path alone: for a kernel trace of it)
dev = torch.device("cuda")
cfg = [dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1),
       dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


for n in points:
    for c in classes:
        g = torch.Generator().manual_seed(n + c)
        logits = (torch.randn(n, c, generator=g) * 2.0).to(dev).requires_grad_(True)
        labels = torch.randint(0, c, (n,), generator=g)
        labels[torch.arange(n) % 10 == 9] = -1
        labels = labels.to(dev)
        row = {}
        for mode in paths:
            crit = build_criteria(cfg, "EW", 2, mode)
            point = dict(n_pred=logits, n_target=labels, loss_mode="train")
            fwd, bwd, vals = [], [], []
            for it in range(repeats + 1):
                logits.grad = None
                tf, loss = timed(lambda: crit(point))
                tb, _ = timed(loss.backward)
                if it:
                    fwd.append(tf), bwd.append(tb)
                vals.append(float(loss.detach()))
            tot = np.array(fwd) + np.array(bwd)
            row[mode] = (np.median(tot), tot.min(), tot.max(), np.median(fwd), np.median(bwd), vals[-1])
        if len(row) < 2:
            for mode, r in row.items():
                print(f"loss N={n} C={c}: {mode} {r[0]:.2f} ms ({r[1]:.2f} - {r[2]:.2f}; fwd {r[3]:.2f}, bwd {r[4]:.2f})", flush=True)
            continue
        t, f = row["torch"], row["fused"]
        print(f"loss N={n} C={c}: torch {t[0]:.2f} ms ({t[1]:.2f} - {t[2]:.2f}; fwd {t[3]:.2f}, bwd {t[4]:.2f}) | fused {f[0]:.2f} ms "
              f"({f[1]:.2f} - {f[2]:.2f}; fwd {f[3]:.2f}, bwd {f[4]:.2f}) | speed-up {t[0] / f[0]:.1f}x | loss torch {t[5]:.6f} "
              f"fused {f[5]:.6f} | peak memory {torch.cuda.max_memory_allocated() / 2**30:.2f} GiB", flush=True)
