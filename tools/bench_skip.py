#!/usr/bin/env python3
"""Cost of the skip-connection options on one 120 k-point ScanNet-shaped room at full width: `inference` ms (`fp16+head`) for
the default model, "add" + skip_connection_scale (the c-decoder alone, which a single-step inference does not run),
skip_connection_scale_i (three n-decoder stages take the merge pass) and s_factor on all four n-decoder stages, in ONE process with the rows
alternating, 3 + 10 timed calls per row (wall time, a device synchronisation around every call), median and min - max of the
10.  Every row but the first is labelled FASTER / NOT faster than the default by its median.
usage: python tools/bench_skip.py [--out FILE.json] [SETTING ...]      SETTING: default | add_scale | scale_i | s_factor"""
import argparse, json, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("settings", nargs="*")
args = ap.parse_args()
settings = args.settings or ["default", "add_scale", "scale_i", "s_factor"]
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from cdsegnet_amd import configs, synth
from cdsegnet_amd.param_init import fill_state_dict
from cdsegnet_amd.registry import build_model
import cdsegnet_amd.models  # noqa: F401

KW = dict(default={}, add_scale=dict(skip_connection_mode="add", skip_connection_scale=True),
          scale_i=dict(skip_connection_scale_i=True), s_factor=dict(s_factor=[0.9, 0.8, 1.1, 0.95]))
dev = torch.device("cuda")
sc = synth.room_scene(0, 120000)
inp = {k: torch.as_tensor(sc[k]).to(dev) for k in ("coord", "grid_coord", "feat", "offset")}
inp["offset_host"] = [int(v) for v in sc["offset"]]
models = {}
for s in settings:
    m = build_model(configs.cdsegnet_config("scannet", **KW[s]))
    m.load_state_dict(fill_state_dict(m.state_dict(), seed=0), strict=True)
    models[s] = m.to(dev).eval()
    models[s].precision = "fp16+head"
res = {s: [] for s in settings}
ROUNDS, WARM = 10, 3
with torch.no_grad():
    for r in range(ROUNDS + WARM):
        for s in settings:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            models[s].inference(dict(inp), eval=False)
            torch.cuda.synchronize(); t = (time.perf_counter() - t0) * 1e3
            if r >= WARM:
                res[s].append(t)
summary = {s: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for s, v in res.items()}
if args.out:
    json.dump(dict(summary=summary, raw=res), open(args.out, "w"), indent=1)
for s in settings:
    label = ""
    if s != settings[0]:
        label = "FASTER" if summary[s]["median"] < summary[settings[0]]["median"] else "NOT faster"
    print(s, {a: round(b, 3) for a, b in summary[s].items()}, label, flush=True)
