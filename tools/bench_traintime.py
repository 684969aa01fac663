"""Time the device train-time pipeline (cdsegnet_amd/traintime.py) per scene next to its numpy restatement on one host thread.

    python tools/bench_traintime.py [--points 150000 300000] [--scenes 6] [--no-host]

The transform list is the ScanNet train list as recorded in tests/golden/traintime_A_raw.npz (cfg_json).  The raw cloud is
a synth.room_scene blown up to an un-voxelised scan: every voxel point plus jittered copies, colours 0..255, unit normals.
Device time: HIP events around each scene (generated draws, a new scene_index per scene) - it includes the gaps the three
host reads per scene leave on the stream; wall time per scene is printed next to it.  Host time: the restatement replaying
the draws the device run generated (tests/traintime_restatement.py, the same operations in numpy), OMP / BLAS threads = 1.
"""
import argparse
import json
import os
import sys
import time

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from cdsegnet_amd import synth, traintime  # noqa: E402


def raw_scan(n_raw, seed):
    base = synth.room_scene(seed, target_points=int(n_raw / 1.5))
    rng = np.random.default_rng(seed + 1)
    m = len(base["coord"])
    extra = rng.integers(0, m, n_raw - m)
    rows = np.concatenate([np.arange(m), extra])
    coord = base["coord"][rows].astype(np.float64)
    coord[m:] += rng.uniform(-0.01, 0.01, (n_raw - m, 3))
    perm = rng.permutation(n_raw)
    rows, coord = rows[perm], coord[perm]
    return dict(coord=coord.astype(np.float32), color=np.round((base["feat"][rows, :3] + 1) * 127.5).astype(np.float32),
                normal=base["feat"][rows, 3:].astype(np.float32), segment=base["segment"][rows])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[150000, 300000])
    ap.add_argument("--scenes", type=int, default=6)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    torch.set_num_threads(1)
    cfg = json.loads(str(np.load(os.path.join(ROOT, "tests", "golden", "traintime_A_raw.npz"))["cfg_json"]))
    tf = traintime.TrainTransform(cfg, seed=0)
    for n in args.points:
        raw = raw_scan(n, 3)
        rawd = {k: torch.as_tensor(v).cuda() for k, v in raw.items()}
        for w in range(2):
            tf(rawd, 1000 + w)
        torch.cuda.synchronize()
        ms, wall, outs = [], [], []
        for s in range(args.scenes):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            out = tf(rawd, s)
            e1.record()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(e0.elapsed_time(e1))
            outs.append(out["coord"].shape[0])
        res = dict(raw_points=n, out_points_median=int(np.median(outs)), device_ms_median=round(float(np.median(ms)), 3),
                   device_ms_min=round(float(np.min(ms)), 3), wall_ms_median=round(float(np.median(wall)), 3), scenes=args.scenes)
        if not args.no_host:
            import traintime_restatement as R
            trace = {}
            tf(rawd, 0, trace=trace)
            torch.cuda.synchronize()
            record = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in trace["draws"].items()}
            host = []
            for _ in range(2):
                t0 = time.perf_counter()
                R.run(cfg, raw, record)
                host.append((time.perf_counter() - t0) * 1e3)
            res["host_restatement_ms_1thread"] = round(float(np.min(host)), 1)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
