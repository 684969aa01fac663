"""Cost of the test-time pipeline AROUND the model: fragments of every augmentation + the softmax votes, with a stub model
that returns ready logits (so that nothing but the pipeline is timed).

  new       TestPipeline.prepare (dense fragments, one cdseg_fragments_build per augmentation) + TestPipeline.vote (one
            cdseg_softmax_vote_fragments per forward)
  baseline  room:  testtime.prepare_test_fragments + testtime._vote, the hand-written ScanNet path (per fragment: a
                   fragment_select, three gathers, a center_shift, a host-to-device offset, a softmax_vote)
            sweep: the nuScenes block cannot be written with that API; the baseline is the same first pass and augmentations
                   followed by the per-fragment ops of the hand-written path without its CenterShift (fragment_select, three
                   gathers, the offset copy, a softmax_vote per fragment)
Both paths run in this process, alternating, each repetition between two HIP events on the stream; the report gives the
median of the event times, the median wall time (with the synchronise), and the library calls per scene.

usage: python tools/bench_testtime.py [--reps 7] [--fragment-batch 1]  ->  text report + one JSON line on stdout"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
from cdsegnet_amd import ops, synth, testtime  # noqa: E402


class StubModel:
    """inference_many -> views of one ready logits buffer: the model costs nothing."""

    def __init__(self, num_classes, device):
        self.k, self.dev, self.buf = num_classes, device, None

    def inference_many(self, dicts, lanes=4, noise_level=None):
        rows = max(d["feat"].shape[0] for d in dicts)
        if self.buf is None or self.buf.shape[0] < rows:
            self.buf = torch.randn(rows, self.k, device=self.dev)
        return [dict(seg_logits=self.buf[:d["feat"].shape[0]]) for d in dicts]


class Counting:
    def __init__(self, real):
        self._real, self.calls = real, 0

    def __getattr__(self, name):
        v = getattr(self._real, name)
        if not callable(v) or name in ("bind_stream", "unbind_stream"):
            return v

        def counted(*a, **k):
            self.calls += 1
            return v(*a, **k)
        return counted


def room(n_voxels, seed):
    """A raw indoor scan: every occupied 2 cm voxel holds 1-4 raw points."""
    sc = synth.room_scene(3, n_voxels)
    rng = np.random.default_rng(seed)
    src = np.repeat(np.arange(len(sc["coord"])), rng.integers(1, 5, len(sc["coord"])))
    coord = (sc["coord"][src] + rng.uniform(-0.008, 0.008, (len(src), 3))).astype(np.float32)
    return dict(coord=coord, color=((sc["feat"][src, :3] + 1) * 127.5).astype(np.float32), normal=sc["feat"][src, 3:].astype(np.float32))


def sweep(n_points, seed):
    """A raw LiDAR sweep with near returns: a quarter of the points have 1-3 neighbours within a few centimetres."""
    sc = synth.lidar_scene(3, n_points)
    rng = np.random.default_rng(seed)
    base = sc["coord"]
    rep = np.where(rng.random(len(base)) < 0.25, rng.integers(2, 5, len(base)), 1)
    src = np.repeat(np.arange(len(base)), rep)
    coord = (base[src] + rng.uniform(-0.03, 0.03, (len(src), 3))).astype(np.float32)
    return dict(coord=coord, strength=rng.random((len(src), 1)).astype(np.float32), segment=rng.integers(0, 16, len(src)))


def sweep_baseline(tp, raw, model, k):
    """The nuScenes block with the per-fragment ops of the hand-written path (see the module docstring)."""
    plan, o = tp.plan, testtime.ops
    scene = testtime.TestScene()
    st = dict(coord=raw["coord"], strength=raw["strength"], color=None, normal=None, segment=raw["segment"])
    o.bind_stream()
    try:
        tp._grid_sample_train(st, scene, 1, plan["transform"][1][1], 0, None)
        idxs, dicts = [], []
        for steps in plan["augs"]:
            c, _ = tp._augment(steps, st["coord"], None)
            feat = tp._collect(st, c, None)
            gs = testtime.grid_sample_test(c, plan["voxelize"]["grid_size"])
            for i in range(gs["num_fragments"]):
                idx = testtime.fragment(gs, i)
                m = idx.numel()
                idxs.append(idx)
                dicts.append(dict(coord=o.gather_rows(c, idx), grid_coord=o.gather_rows(gs["grid_coord"], idx),
                                  feat=o.gather_rows(feat, idx), index=idx,
                                  offset=torch.tensor([m], dtype=torch.int64, device=c.device), offset_host=[m]))
    finally:
        o.unbind_stream()
    labels, pred = testtime._vote(model, st["coord"].shape[0], k, idxs, dicts, c.device, None, 4)
    return o.gather_i32(labels, scene.inverse), pred


def measure(name, paths, reps):
    """paths: {label: fn}; alternating repetitions, HIP events + wall clock; returns {label: dict(event_ms, wall_ms, calls)}."""
    out = {k: dict(event=[], wall=[]) for k in paths}
    for fn in paths.values():  # warm-up: workspaces, allocator
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for label, fn in paths.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t = time.perf_counter()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            out[label]["wall"].append(1e3 * (time.perf_counter() - t))
            out[label]["event"].append(a.elapsed_time(b))
    res = {}
    for label, fn in paths.items():
        proxy = Counting(ops)
        testtime.ops = proxy
        try:
            fn()
        finally:
            testtime.ops = ops
        res[label] = dict(event_ms=statistics.median(out[label]["event"]), wall_ms=statistics.median(out[label]["wall"]),
                          calls=proxy.calls)
        print(f"{name} {label:9s}: {res[label]['event_ms']:8.2f} ms between events, {res[label]['wall_ms']:8.2f} ms wall, "
              f"{proxy.calls} library calls from the pipeline")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--fragment-batch", type=int, default=1)
    ap.add_argument("--room-voxels", type=int, default=60000)
    ap.add_argument("--sweep-points", type=int, default=24000)
    args = ap.parse_args()
    dev = torch.device("cuda")
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(here, "tests", "golden", "test_blocks.json")) as f:
        blocks = json.load(f)
    report = {}

    raw = {k: torch.as_tensor(v).to(dev) for k, v in room(args.room_voxels, 11).items()}
    tp, model = testtime.TestPipeline(blocks["scannet"]), StubModel(20, dev)
    gsize = blocks["scannet"]["test_cfg"]["voxelize"]["grid_size"]
    scene = tp.prepare(raw)
    print(f"room: {scene.n_raw} raw points, 13 augmentations, {len(scene.fragments)} fragments "
          f"({[g['num_fragments'] for g in scene.augs]}), {scene.augs[0]['num_voxels']} voxels in the first")

    def room_new():
        return tp.vote(model, tp.prepare(raw), 20, fragment_batch=args.fragment_batch)

    def room_old():
        idxs, dicts = testtime.prepare_test_fragments(raw["coord"], raw["color"], raw["normal"], gsize)
        return testtime._vote(model, raw["coord"].shape[0], 20, idxs, dicts, dev, None, 4)

    a, b = room_new(), room_old()
    if args.fragment_batch == 1:
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "the two paths must vote alike"
    report["room"] = measure("room ", dict(new=room_new, baseline=room_old), args.reps)
    report["room"].update(points=scene.n_raw, fragments=len(scene.fragments))
    del scene

    raw = {k: torch.as_tensor(v).to(dev) for k, v in sweep(args.sweep_points, 12).items()}
    tp, model = testtime.TestPipeline(blocks["nuscenes"]), StubModel(16, dev)
    scene = tp.prepare(raw)
    print(f"sweep: {scene.n_raw} raw points -> {scene.n} after the 2.5 cm pass, 10 augmentations, {len(scene.fragments)} fragments "
          f"({[g['num_fragments'] for g in scene.augs]})")

    def sweep_new():
        return tp.vote(model, tp.prepare(raw), 16, fragment_batch=args.fragment_batch)

    def sweep_old():
        return sweep_baseline(tp, raw, model, 16)

    a, b = sweep_new(), sweep_old()
    if args.fragment_batch == 1:
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "the two paths must vote alike"
    report["sweep"] = measure("sweep", dict(new=sweep_new, baseline=sweep_old), args.reps)
    report["sweep"].update(points=scene.n_raw, fragments=len(scene.fragments))
    report["fragment_batch"] = args.fragment_batch
    print(json.dumps(report))


if __name__ == "__main__":
    main()
