#!/usr/bin/env python3
"""One full-width training step (forward under autograd, loss.backward(), AdamW) on a synthetic ScanNet-shaped batch, fp32
with a 16-bit attention core, or under AMP (16-bit attention core, Linears and sparse convs; train_precision), on the HIP kernels (cdsegnet_amd/train_graph.py).  Not a BASELINE metric - the reference publishes no training throughput -
a first number for the training row of SURVEY 8(f4).
usage: python tools/bench_train_step.py [scenes=1] [points=120000] [steps=4] [dataset=scannet|scannet200|nuscenes]
       [train_precision=fp32|fp16-attn|bf16-attn|fp16-amp|bf16-amp] [det] [fused] [fusednorm] [fusedopt] [shadow] [nativeblock]
       [mix3d|mix3d-rows] [attn_drop=R] [proj_drop=R]
A trailing `det` sets train_deterministic = True (fixed-order gradient reductions: bit-reproducible steps), a trailing `fused`
sets train_loss = "fused" (cross entropy + Lovasz on the HIP loss kernels instead of the torch criteria), a trailing `fusednorm` sets train_norm =
"fused" (train-mode BatchNorm + GELU and the pooling maximum on the kernels of csrc/norm.hip), a trailing `fusedopt`
takes cdsegnet_amd.optim.FusedAdamW in torch.optim.AdamW's place, and `shadow` (with `fusedopt` under an AMP precision) lets it
keep the 16-bit weight copies the forward multiplies with.  A trailing `nativeblock` sets train_block = "native" (every Block one
autograd node on the executor of csrc/trainblock.hip).  A trailing `mix3d` merges the scenes pairwise into one batch element each
(Mix3D: the merged rooms share voxels) and trains them in the default train_mix3d = "fold"; `mix3d-rows` sets train_mix3d =
"rows" on the same batch (every point a row of its own).  Trailing `attn_drop=R` / `proj_drop=R` set the backbone's dropout rates
(default 0, as in every shipped config)."""
import os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cdsegnet_amd import configs, synth
from cdsegnet_amd.param_init import fill_state_dict
from cdsegnet_amd.registry import build_model
import cdsegnet_amd.models  # noqa: F401

scenes = int(sys.argv[1]) if len(sys.argv) > 1 else 1
points = int(sys.argv[2]) if len(sys.argv) > 2 else 120000
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 4
dataset = sys.argv[4] if len(sys.argv) > 4 else "scannet"
train_precision = sys.argv[5] if len(sys.argv) > 5 else "fp32"
deterministic = "det" in sys.argv[6:]
fused = "fused" in sys.argv[6:]
fusednorm = "fusednorm" in sys.argv[6:]
fusedopt = "fusedopt" in sys.argv[6:]
shadow = "shadow" in sys.argv[6:]
nativeblock = "nativeblock" in sys.argv[6:]
mix3d = "rows" if "mix3d-rows" in sys.argv[6:] else ("fold" if "mix3d" in sys.argv[6:] else None)
if shadow and not (fusedopt and train_precision.endswith("-amp")):
    sys.exit("`shadow` needs `fusedopt` and an AMP train_precision (the fp32 step multiplies with the fp32 weights)")
dev = torch.device("cuda")
cfg = configs.cdsegnet_config(dataset)
drops = {k: float(a.split("=", 1)[1]) for a in sys.argv[6:] for k in ("attn_drop", "proj_drop") if a.startswith(k + "=")}
cfg["backbone"].update(drops)
cfg["criteria"] = [dict(type="MSELoss", loss_weight=1.0, ignore_index=-1, batch_sample_point=-1),
                   dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1),
                   dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)]
model = build_model(cfg)
model.load_state_dict(fill_state_dict(model.state_dict(), seed=0), strict=True)
model = model.to(dev).train()
model.train_precision = train_precision
model.train_deterministic = deterministic
if fused:
    model.train_loss = "fused"
if fusednorm:
    model.train_norm = "fused"
if nativeblock:
    model.train_block = "native"
sc = synth.collate([(synth.lidar_scene(i, points) if dataset == "nuscenes" else synth.room_scene(i, points)) for i in range(scenes)])
inp = {k: torch.as_tensor(sc[k]).to(dev) for k in ("coord", "grid_coord", "feat", "offset")}
inp["segment"] = (torch.as_tensor(np.asarray(sc["segment"]).astype(np.int64)) % cfg["num_classes"]).to(dev)
if mix3d is not None:  # point_collate_fn's merge: offset[1:-1:2] + offset[-1]
    model.train_mix3d = mix3d
    inp["offset"] = torch.cat([inp["offset"][1:-1:2], inp["offset"][-1:]])
n = inp["feat"].shape[0]
named = dict(model.named_parameters())
groups = [dict(params=[p for k, p in named.items() if "block" not in k], lr=0.002),
          dict(params=[p for k, p in named.items() if "block" in k], lr=0.0002)]
if fusedopt:
    from cdsegnet_amd.optim import FusedAdamW
    opt = FusedAdamW(groups, lr=0.002, weight_decay=0.05, shadow16={"fp16-amp": "f16", "bf16-amp": "bf16"}[train_precision] if shadow else None)
else:
    opt = torch.optim.AdamW(groups, lr=0.002, weight_decay=0.05)
times, losses = [], []
for it in range(steps + 1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    opt.zero_grad(set_to_none=True)
    loss = model(inp)["loss"]
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    loss.backward()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    opt.step()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    losses.append(float(loss.detach()))
    if it:
        times.append((t1 - t0, t2 - t1, t3 - t2))
t = np.median(np.array(times), axis=0) * 1e3
tot = np.array(times).sum(1) * 1e3  # run-to-run spread of the whole step
print(f"training step, {dataset}, full width, {train_precision}{', deterministic' if deterministic else ''}{', fused loss' if fused else ''}{', fused norm' if fusednorm else ''}{', FusedAdamW' if fusedopt else ''}{' + 16-bit weight copies' if shadow else ''}{', native Blocks' if nativeblock else ''}{''.join(f', {k} {v}' for k, v in drops.items())}, {scenes} scene(s), {n} points: forward {t[0]:.1f} ms, backward {t[1]:.1f} ms, "
      f"AdamW {t[2]:.1f} ms = {t.sum():.1f} ms/step (steps {tot.min():.1f} - {tot.max():.1f}) = {n / t.sum() * 1e3 / 1e6:.2f} M points/s; peak memory "
      f"{torch.cuda.max_memory_allocated() / 2**30:.1f} GiB; loss over the steps {[round(v, 4) for v in losses]}")
if mix3d is not None:
    print(f"Mix3D, train_mix3d = {mix3d!r}: {len(inp['offset'])} batch element(s), N = %d points in V = %d voxels" % model._train_graph.last_shared)
if nativeblock:
    tbs = [ent[3] for ent in model._train_graph._native.values()]
    print(f"native Blocks: {len(tbs)} descriptors, persistent derived-weights buffers {sum(tb.derived_bytes for tb in tbs) / 2**20:.1f} MiB "
          f"(Block matrices in fp32: {sum(4 * tb.params[i].numel() for tb in tbs for i in (0, 2, 8, 10, 14, 16)) / 2**20:.1f} MiB)")
