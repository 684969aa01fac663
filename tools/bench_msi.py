"""Multi-step inference (MSAI / MSFI) with the REAL model: what the DDIM steps cost, and what computing the n-encoder once
(`reuse_encoder=True`) changes.

Two workloads, the ScanNet CDSegNet config at full width, weights from param_init.fill_state_dict, noise from the device RNG
(like bench.py: no host RNG in the step):
  forward   one 120 k-point synthetic room: model.inference_ddim(step, mode="avg"), every run between two HIP events
  pipeline  the raw 150 k-point room of tools/bench_vote.py through the ScanNet test block (13 augmentations):
            TestPipeline.segment(inference_mode="MSAI", step, share_plan=True), raw scan -> labels, wall clock between two
            device synchronisations; and, for --hand-step (4), a hand loop of `inference_ddim` per fragment + softmax_vote on the
            prepared scene (what one writes without inference_mode=)
Rows: step in --steps (1,4,10) x reuse_encoder off / on.  The rows alternate in ONE process: one warm-up run of every row
(workspaces, allocator pools; reported, not compared), then --runs (2) timed runs of every row; a row reports its median and
its spread (slowest - fastest run).  `on` is FASTER than `off` only if its slowest run beats off's fastest by more than both
spreads; otherwise the report says NOT faster.  A tree whose inference_ddim has no `reuse_encoder` argument runs the `off`
rows alone (for comparisons with an earlier commit).

usage: python tools/bench_msi.py [--workloads forward,pipeline] [--steps 1,4,10] [--runs 2] [--points 120000]
       [--room-voxels 60000] [--max-fragments N] [--hand-step 4]  ->  text report + one JSON line on stdout"""
import argparse
import inspect
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.getcwd())
import cdsegnet_amd.models  # noqa: E402,F401
from cdsegnet_amd import ops, synth, testtime  # noqa: E402
from tools.bench_testtime import room  # noqa: E402
from tools.bench_vote import full_model  # noqa: E402


def summarise(name, res, pairs):
    for r, v in res.items():
        v["median_ms"] = statistics.median(v["ms"])
        v["spread_ms"] = max(v["ms"]) - min(v["ms"])
        print(f"{name} {r:18s}: " + ", ".join(f"{x:9.2f}" for x in v["ms"]) + f" ms (median {v['median_ms']:.2f}, spread "
              f"{v['spread_ms']:.2f}, warm-up {v['warmup_ms']:.2f})" + (f" {v['stats']}" if v.get("stats") else ""), flush=True)
    for new, base in pairs:
        if new in res and base in res:
            a, b = res[new], res[base]
            gap = min(b["ms"]) - max(a["ms"])
            verdict = "FASTER" if gap > max(a["spread_ms"], b["spread_ms"]) else "NOT faster"
            a["verdict"] = f"{verdict} than {base}"
            print(f"{name} {new:18s} -> {verdict} than {base}: median {b['median_ms'] - a['median_ms']:+.2f} ms "
                  f"({100.0 * (1 - a['median_ms'] / b['median_ms']):+.1f} %), slowest run {gap:+.2f} ms against its fastest",
                  flush=True)


def alternate(rows, runs):
    """rows: {label: fn -> ms}; one warm-up and `runs` timed runs of every row, alternating."""
    res = {r: dict(ms=[]) for r in rows}
    for rep in range(runs + 1):
        for r, fn in rows.items():
            torch.manual_seed(17)
            ms = fn()
            if rep == 0:
                res[r]["warmup_ms"] = ms
            else:
                res[r]["ms"].append(ms)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="forward,pipeline")
    ap.add_argument("--steps", default="1,4,10")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--room-voxels", type=int, default=60000)
    ap.add_argument("--max-fragments", type=int, default=None)
    ap.add_argument("--hand-step", type=int, default=4)
    args = ap.parse_args()
    steps = [int(s) for s in args.steps.split(",") if s]
    dev = torch.device("cuda")
    model, k = full_model("scannet", dev)
    T = model.T
    has_flag = "reuse_encoder" in inspect.signature(model.inference_ddim).parameters
    flags = (False, True) if has_flag else (False,)
    eng = model.engine()
    report = dict(steps=steps, runs=args.runs, reuse_encoder_available=has_flag)
    pairs = [(f"step{s} on", f"step{s} off") for s in steps]

    if "forward" in args.workloads:
        sc = synth.room_scene(3, args.points)
        inp = {key: torch.as_tensor(sc[key]).to(dev) for key in ("coord", "grid_coord", "feat", "offset")}
        inp["offset_host"] = [int(v) for v in sc["offset"]]
        print(f"forward: {inp['feat'].shape[0]} points", flush=True)

        def forward(step, flag):
            def run():
                kw = dict(reuse_encoder=True) if flag else {}
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                model.inference_ddim(dict(inp), T=T, step=step, eval=False, mode="avg", **kw)
                b.record()
                torch.cuda.synchronize()
                return a.elapsed_time(b)
            return run

        rows = {f"step{s} {'on' if f else 'off'}": forward(s, f) for s in steps for f in flags}
        res = alternate(rows, args.runs)
        summarise("forward ", res, pairs)
        report["forward"] = res

    if "pipeline" in args.workloads:
        here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        with open(os.path.join(here, "tests", "golden", "test_blocks.json")) as f:
            tp = testtime.TestPipeline(json.load(f)["scannet"])
        raw = {key: torch.as_tensor(v).to(dev) for key, v in room(args.room_voxels, 11).items()}
        scene = tp.prepare(raw, max_fragments=args.max_fragments)
        frags = [g["num_fragments"] for g in scene.augs]
        print(f"pipeline: {scene.n_raw} raw points, {len(scene.augs)} augmentations, {sum(frags)} fragments, "
              f"{scene.augs[0]['num_voxels']} rows in a fragment of the first", flush=True)
        has_mode = "inference_mode" in inspect.signature(tp.segment).parameters

        def segment(step, flag):
            def run():
                torch.cuda.synchronize()
                t = time.perf_counter()
                tp.segment(model, raw, k, max_fragments=args.max_fragments, share_plan=True, inference_mode="MSAI", step=step,
                           reuse_encoder=flag)
                torch.cuda.synchronize()
                return 1e3 * (time.perf_counter() - t)
            return run

        def hand_loop():
            torch.cuda.synchronize()
            t = time.perf_counter()
            sc_ = tp.prepare(raw, max_fragments=args.max_fragments)
            pred = torch.zeros((sc_.n, k), dtype=torch.float32, device=dev)
            for d in sc_.fragments:
                o = model.inference_ddim(dict(d), T=T, step=args.hand_step, eval=False, mode="avg")["seg_logits"]
                ops.softmax_vote(o, d["index"], pred)
            labels = ops.argmax_rows(pred)
            if sc_.inverse is not None:
                labels = ops.gather_i32(labels, sc_.inverse)
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t)

        rows = {}
        if has_mode:
            rows.update({f"step{s} {'on' if f else 'off'}": segment(s, f) for s in steps for f in flags})
        rows[f"step{args.hand_step} hand loop"] = hand_loop
        res = alternate(rows, args.runs)
        summarise("pipeline", res, pairs + [(f"step{args.hand_step} off", f"step{args.hand_step} hand loop")])
        report["pipeline"] = res
    report["msi_stats_last"] = getattr(eng, "msi_stats", None)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
