#!/usr/bin/env python3
"""Cost of the Feature Fusion Module options on one 120 k-point ScanNet-shaped room at full width: `inference` ms (`fp16+head`) and
the training step ms (forward, backward, FusedAdamW; `fp16-amp`, native Block) for every setting named, in ONE process with the
rows alternating, 3 + 8 / 2 + 8 timed calls per row (wall time, a device synchronisation around every call), median and
min - max of the 8.
usage: python tools/bench_fusion.py [--root DIR] [--out FILE.json] [SETTING ...]
SETTING: default | channel_scale | b_channel_scale | bidir | bidir_b_channel_scale (default: all five).  --root: the checkout whose
package is measured (default: this one) - `--root <a checkout of another commit, built> default` measures that commit's
default model with the same script, e.g. the parent's next to this one's, one process each, alternating."""
import argparse, json, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", default=None)
ap.add_argument("settings", nargs="*")
args = ap.parse_args()
root, out = os.path.abspath(args.root), args.out
settings = args.settings or ["default", "channel_scale", "b_channel_scale", "bidir", "bidir_b_channel_scale"]
here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if root != here:
    sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") != here]
sys.path.insert(0, root)
import numpy as np
import torch
import cdsegnet_amd
assert os.path.abspath(cdsegnet_amd.__file__).startswith(root), cdsegnet_amd.__file__
from cdsegnet_amd import configs, synth
from cdsegnet_amd.param_init import fill_state_dict
from cdsegnet_amd.registry import build_model
import cdsegnet_amd.models  # noqa: F401
from cdsegnet_amd.optim import FusedAdamW

KW = dict(default={}, channel_scale=dict(tm_feat="channel_scale"), b_channel_scale=dict(tm_feat="b_channel_scale"),
          bidir=dict(tm_bidirectional=True), bidir_b_channel_scale=dict(tm_feat="b_channel_scale", tm_bidirectional=True))
CRIT = [dict(type="MSELoss", loss_weight=1.0, ignore_index=-1, batch_sample_point=-1),
        dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1),
        dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)]
dev = torch.device("cuda")
sc = synth.room_scene(0, 120000)
inp = {k: torch.as_tensor(sc[k]).to(dev) for k in ("coord", "grid_coord", "feat", "offset")}
inp["offset_host"] = [int(v) for v in sc["offset"]]
seg = (torch.as_tensor(np.asarray(sc["segment"]).astype(np.int64)) % 20).to(dev)
models, opts = {}, {}
for s in settings:
    cfg = configs.cdsegnet_config("scannet", **KW[s]) if KW[s] else configs.cdsegnet_config("scannet")
    cfg["criteria"] = CRIT
    m = build_model(cfg)
    m.load_state_dict(fill_state_dict(m.state_dict(), seed=0), strict=True)
    models[s] = m.to(dev)
    print("built", s, flush=True)
res = {s: dict(infer=[], train=[]) for s in settings}
# inference, fp16+head
for s in settings:
    models[s].eval(); models[s].precision = "fp16+head"
ROUNDS, WARM = 8, 3
with torch.no_grad():
    for r in range(ROUNDS + WARM):
        for s in settings:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            models[s].inference(dict(inp), eval=False)
            torch.cuda.synchronize(); t = (time.perf_counter() - t0) * 1e3
            if r >= WARM:
                res[s]["infer"].append(t)
    print("inference done", {s: round(float(np.median(res[s]["infer"])), 3) for s in settings}, flush=True)
for s in settings:
    m = models[s]; m._drop_engine(); m.train(); m.train_precision = "fp16-amp"; m.train_block = "native"
    named = dict(m.named_parameters())
    opts[s] = FusedAdamW([dict(params=[p for k, p in named.items() if "block" not in k], lr=0.002),
                          dict(params=[p for k, p in named.items() if "block" in k], lr=0.0002)], lr=0.002, weight_decay=0.05)
tinp = dict(inp, segment=seg); tinp.pop("offset_host")
for r in range(ROUNDS + 2):
    for s in settings:
        torch.cuda.synchronize(); t0 = time.perf_counter()
        opts[s].zero_grad(set_to_none=True)
        loss = models[s](tinp)["loss"]; loss.backward(); opts[s].step()
        torch.cuda.synchronize(); t = (time.perf_counter() - t0) * 1e3
        if r >= 2:
            res[s]["train"].append(t)
summary = {s: {k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for k, v in res[s].items()} for s in settings}
if out:
    json.dump(dict(root=root, summary=summary, raw=res), open(out, "w"), indent=1)
for s in settings:
    print(s, {k: {a: round(b, 3) for a, b in v.items()} for k, v in summary[s].items()}, flush=True)
