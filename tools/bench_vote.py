"""Test-time voting with the REAL model: what TestPipeline.segment costs per scan, and what sharing the plan between the
fragments of an augmentation (share_plan) and per-fragment draws inside collated forwards (fragment_draws="fragment") change.

Two scans: a raw indoor room through the ScanNet test block (13 augmentations) with the ScanNet CDSegNet config at full width,
and a raw LiDAR sweep through the nuScenes test block (ten lists) with the nuScenes config (the same widths, 4 input
channels); weights from param_init.fill_state_dict, noise from the device RNG (like bench.py: no host RNG in the step).

Rows, per scan:
  default         segment(...)                                         one forward and one plan per fragment
  share_plan      segment(..., share_plan=True)                        one plan per augmentation
  batch4          segment(..., fragment_batch=4)                       4 fragments per forward, one set of draws per forward
  batch4+fragment segment(..., fragment_batch=4, share_plan=True, fragment_draws="fragment")
                                                                       4 fragments per forward, every fragment its own draws
The rows alternate in ONE process, every run between two device synchronisations: one warm-up run of every row (workspaces,
allocator pools; reported, not compared), then --runs (2) timed runs of every row.  The margin of a row is the difference
between its timed runs.  Per row the report also gives `plans_built` (Engine.plans_built) and the blocking host reads of one
run (Tensor.item / .tolist / .cpu on a device tensor and Event.synchronize, counted by wrappers installed here).

usage: python tools/bench_vote.py [--rows default,share_plan,batch4,batch4+fragment] [--runs 2] [--room-voxels 60000]
       [--sweep-points 24000]  ->  text report + one JSON line on stdout"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.getcwd())
import cdsegnet_amd.models  # noqa: E402,F401
from cdsegnet_amd import configs, testtime  # noqa: E402
from cdsegnet_amd.param_init import fill_state_dict  # noqa: E402
from cdsegnet_amd.registry import build_model  # noqa: E402
from tools.bench_testtime import room, sweep  # noqa: E402

ROWS = {
    "default": dict(),
    "share_plan": dict(share_plan=True),
    "batch4": dict(fragment_batch=4),
    "batch4+fragment": dict(fragment_batch=4, share_plan=True, fragment_draws="fragment"),
}


class HostReads:
    """Counts the calls that make the host wait for the device."""

    def __init__(self):
        self.n = 0
        for cls, names in ((torch.Tensor, ("item", "tolist", "cpu")), (torch.cuda.Event, ("synchronize",))):
            for name in names:
                setattr(cls, name, self._wrap(getattr(cls, name), cls is torch.Tensor))

    def _wrap(self, fn, tensor):
        def counted(obj, *a, **k):
            if not tensor or obj.is_cuda:
                self.n += 1
            return fn(obj, *a, **k)
        return counted


def full_model(dataset, dev):
    cfg = configs.cdsegnet_config(dataset)
    model = build_model(cfg)
    model.load_state_dict(fill_state_dict(model.state_dict(), seed=1), strict=True)
    model = model.to(dev).eval()
    model.noise_source = "device"
    return model, cfg["num_classes"]


def run_scan(name, tp, model, k, raw, rows, runs, reads):
    scene = tp.prepare(raw)
    frags = [g["num_fragments"] for g in scene.augs]
    print(f"{name}: {scene.n_raw} raw points, {len(scene.augs)} augmentations, {sum(frags)} fragments {frags}, "
          f"{scene.augs[0]['num_voxels']} rows in a fragment of the first", flush=True)
    del scene
    eng = model.engine()
    res = {r: dict(ms=[]) for r in rows}
    for rep in range(runs + 1):
        for r in rows:
            torch.manual_seed(17)
            p0, h0 = getattr(eng, "plans_built", None), reads.n
            torch.cuda.synchronize()
            t = time.perf_counter()
            tp.segment(model, raw, k, **ROWS[r])
            torch.cuda.synchronize()
            ms = 1e3 * (time.perf_counter() - t)
            if rep == 0:
                res[r]["warmup_ms"] = ms
            else:
                res[r]["ms"].append(ms)
            res[r]["plans_built"] = None if p0 is None else eng.plans_built - p0
            res[r]["host_reads"] = reads.n - h0
    base = res.get("default")
    for r in rows:
        ms = res[r]["ms"]
        res[r]["margin_ms"] = max(ms) - min(ms)
        line = (f"{name} {r:16s}: " + ", ".join(f"{v:8.2f}" for v in ms) + f" ms (margin {res[r]['margin_ms']:.2f}, warm-up "
                f"{res[r]['warmup_ms']:.2f}), plans_built {res[r]['plans_built']}, host reads {res[r]['host_reads']}")
        if base is not None and r != "default":
            # faster only if every run of the row beats every run of the default row by more than both margins
            gap = min(base["ms"]) - max(ms)
            verdict = "FASTER" if gap > max(res[r]["margin_ms"], base["margin_ms"]) else "NOT faster"
            res[r]["verdict"] = verdict
            line += f" -> {verdict} than default (slowest run {gap:+.2f} ms against default's fastest)"
        print(line, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--room-voxels", type=int, default=60000)
    ap.add_argument("--sweep-points", type=int, default=24000)
    ap.add_argument("--scans", default="room,sweep")
    args = ap.parse_args()
    rows = [r for r in args.rows.split(",") if r]
    for r in rows:
        if r not in ROWS:
            raise SystemExit(f"unknown row {r!r}: {list(ROWS)}")
    dev = torch.device("cuda")
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(here, "tests", "golden", "test_blocks.json")) as f:
        blocks = json.load(f)
    reads = HostReads()
    report = dict(rows=rows, runs=args.runs)
    if "room" in args.scans:
        raw = {k: torch.as_tensor(v).to(dev) for k, v in room(args.room_voxels, 11).items()}
        model, k = full_model("scannet", dev)
        report["room"] = run_scan("room ", testtime.TestPipeline(blocks["scannet"]), model, k, raw, rows, args.runs, reads)
        del model, raw
        torch.cuda.empty_cache()
    if "sweep" in args.scans:
        raw = {k: torch.as_tensor(v).to(dev) for k, v in sweep(args.sweep_points, 12).items()}
        model, k = full_model("nuscenes", dev)
        report["sweep"] = run_scan("sweep", testtime.TestPipeline(blocks["nuscenes"]), model, k, raw, rows, args.runs, reads)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
