"""Record the reference's nuScenes TEST block on a synthetic sweep -> tests/golden/testtime_nuscenes.npz, and the ``data.test``
dicts of the three shipped CDSegNet configs -> tests/golden/test_blocks.json (data and settings only).

Runs ONLY where the reference checkout is available (environment variable CDSEG_REFERENCE): it imports the reference's
pointcept/datasets/transform.py by file and runs the real transform classes of configs/nuscenes/CDSegNet.py in the order of
pointcept/datasets/defaults.py:98-132 (transform, every aug_transform list on a copy, test_cfg.voxelize, post_transform per
fragment).  ``np.random.randint`` - the member pick of the train-mode GridSample - is recorded.

testtime_nuscenes.npz
  coord / strength / segment   the raw sweep (N rows), seed
  1.r_reference                the recorded np.random.randint(0, count.max(), count.size), one per voxel in the REFERENCE's
                               (FNV hash) voxel order
  1.r                          the same pick restated for this project's voxel order (packed integer key, members in row
                               order): the member rank of the row the reference kept, one per voxel - the ``draws`` record of
                               cdsegnet_amd.testtime.TestPipeline ("<position of the GridSample>.r")
  kept                         raw row of every row of the transformed scan, in the reference's row order (n rows)
  inverse                      the reference's ``inverse`` (N,), origin_segment (N,), grid025_raw (N,3) every raw row's voxel
  aug<a>_coord                 the augmented cloud (n,3) in the reference's dtype; aug<a>_grid (n,3) every row's voxel at the
                               test grid size; aug<a>_feat (n,4) the collected features scattered back by ``index``;
                               aug<a>_frag_index (F,m) the fragments' ``index`` rows; aug<a>_frag_sizes
The sweep: LiDAR-like points plus jittered copies of a subset, so that the 0.025 m pass drops >= 20 % of the rows, the 0.05 m
voxels hold 1, 2 and >= 3 rows and some augmentation has >= 4 fragments (asserted below).
"""
import json
import os
import runpy
import sys
from copy import deepcopy

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("CDSEG_REFERENCE")
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

from tools.make_traintime_golden import Recorder, load_reference_transforms  # noqa: E402

SEED = 5


def sweep(rng):
    """~1000 LiDAR-like points + near copies (same 2.5 cm voxel: dropped by the first pass) + far copies (neighbouring 2.5 cm
    voxels of the same 5 cm voxel: several fragments)."""
    from cdsegnet_amd import synth
    base = synth.lidar_scene(3, 1000)["coord"].astype(np.float64)
    base = base + rng.uniform(-0.02, 0.02, base.shape)
    n0 = len(base)
    near = base[rng.choice(n0, 450, replace=False)]
    near = np.repeat(near, 2, 0) + rng.uniform(-0.004, 0.004, (900, 3))
    far_src = base[rng.choice(n0, 160, replace=False)]
    reps = rng.integers(1, 9, len(far_src))
    far = np.repeat(far_src, reps, 0)
    far = far + rng.uniform(-0.03, 0.03, far.shape)
    coord = np.concatenate([base, near, far]).astype(np.float32)
    coord = coord[rng.permutation(len(coord))]
    n = len(coord)
    return dict(coord=coord, strength=rng.random((n, 1)).astype(np.float32), segment=rng.integers(0, 16, n).astype(np.int64))


def json_ready(x):
    if isinstance(x, dict):
        return {k: json_ready(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [json_ready(v) for v in x]
    if isinstance(x, (np.integer,)):
        return int(x)
    if isinstance(x, (np.floating,)):
        return float(x)
    return x


def register_scannet200_constants():
    """configs/scannet200/CDSegNet.py imports its class names through the pointcept.datasets package, whose __init__ pulls in
    the whole training stack: register that one module by file under bare parent packages instead."""
    import importlib.util
    import types
    dotted = "pointcept.datasets.preprocessing.scannet.meta_data.scannet200_constants"
    parts = dotted.split(".")
    for i in range(2, len(parts)):
        name = ".".join(parts[:i])
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
            sys.modules[name].__path__ = []
    spec = importlib.util.spec_from_file_location(dotted, os.path.join(REF, *parts) + ".py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules[dotted] = mod
    spec.loader.exec_module(mod)


def test_blocks():
    register_scannet200_constants()
    out = {}
    for name in ("scannet", "scannet200", "nuscenes"):
        cfg = runpy.run_path(os.path.join(REF, f"configs/{name}/CDSegNet.py"))["data"]["test"]
        cfg = json_ready(dict(cfg))
        cfg.pop("data_root", None)  # a path of the machine that trains, not a setting of the pipeline
        out[name] = cfg
    return out


def packed_pick(grid_raw, kept):
    """The member rank (rows ascending) of the kept row of every voxel, voxels in packed-key order."""
    g = grid_raw.astype(np.int64)
    key = (g[:, 0] << 42) | (g[:, 1] << 21) | g[:, 2]
    order = np.argsort(key, kind="stable")
    ks = key[order]
    start = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
    end = np.concatenate([start[1:], [len(ks)]])
    is_kept = np.zeros(len(g), dtype=bool)
    is_kept[kept] = True
    r = np.empty(len(start), dtype=np.int64)
    for v, (s, e) in enumerate(zip(start, end)):
        hit = np.flatnonzero(is_kept[order[s:e]])
        assert len(hit) == 1
        r[v] = hit[0]
    return r


def main():
    if not REF or not os.path.isdir(REF):
        raise SystemExit("set CDSEG_REFERENCE to the reference checkout")
    T = load_reference_transforms()
    blocks = test_blocks()
    with open(os.path.join(OUT, "test_blocks.json"), "w") as f:
        json.dump(blocks, f, indent=1, sort_keys=True)
        f.write("\n")
    cfg = runpy.run_path(os.path.join(REF, "configs/nuscenes/CDSegNet.py"))["data"]["test"]
    tc = cfg["test_cfg"]
    raw = sweep(np.random.default_rng(2027))
    n_raw = len(raw["coord"])

    def run_transform(segment):
        np.random.seed(SEED)
        with Recorder() as rec:
            data = T.Compose(cfg["transform"])(dict(coord=raw["coord"].copy(), strength=raw["strength"].copy(), segment=segment.copy()))
        draws = [v for name, v in rec.log if name == "randint"]
        assert len(draws) == 1
        return data, draws[0]

    # pass 1 carries the raw row in ``segment`` (the transform gathers it like any point key), pass 2 is the real one
    probe, r_a = run_transform(np.arange(n_raw, dtype=np.int64))
    kept = probe["segment"].astype(np.int64)
    data, r_b = run_transform(raw["segment"])
    assert np.array_equal(r_a, r_b) and np.array_equal(data["coord"], raw["coord"][kept])
    assert np.array_equal(data["origin_segment"], raw["segment"]) and np.array_equal(data["segment"], raw["segment"][kept])
    inverse = np.asarray(data["inverse"]).astype(np.int64)
    assert np.array_equal(kept[inverse][kept], kept)
    # every raw row's voxel of the first pass: the same GridSample with return_grid_coord on a copy
    gcfg = dict(cfg["transform"][1], return_grid_coord=True)
    np.random.seed(SEED)
    g = T.TRANSFORMS.build(gcfg)(dict(coord=raw["coord"].copy(), strength=raw["strength"].copy(), segment=raw["segment"].copy()))
    grid_raw = g["grid_coord"][g["inverse"]].astype(np.int32)
    n = len(kept)
    fx = dict(coord=raw["coord"], strength=raw["strength"], segment=raw["segment"], seed=np.int64(SEED), kept=kept.astype(np.int32),
              inverse=inverse.astype(np.int32), origin_segment=np.asarray(data["origin_segment"]).astype(np.int64),
              grid025_raw=grid_raw)
    fx["1.r_reference"] = np.asarray(r_a).astype(np.int64)
    fx["1.r"] = packed_pick(grid_raw, kept)
    assert 1.0 - n / n_raw >= 0.2, (n, n_raw)

    scan = dict(coord=data["coord"], strength=data["strength"])  # what defaults.py:103-109 leaves in the dict
    voxelize = T.TRANSFORMS.build(tc["voxelize"])
    post = T.Compose(tc["post_transform"])
    most, counts_seen = 0, set()
    for a, lst in enumerate(tc["aug_transform"]):
        d = T.Compose(lst)(deepcopy(scan))
        fx[f"aug{a}_coord"] = np.asarray(d["coord"])
        parts = voxelize(d)
        grid = np.full((n, 3), -1, dtype=np.int64)
        feat = np.zeros((n, 4), dtype=np.float32)
        index, sizes = [], []
        for part in parts:
            idx = np.asarray(part["index"])
            grid[idx] = part["grid_coord"]
            out = post(part)
            assert out["feat"].dtype.is_floating_point and tuple(out["feat"].shape) == (len(idx), 4)
            assert np.array_equal(out["coord"].numpy(), np.asarray(d["coord"])[idx].astype(np.float32))
            feat[idx] = out["feat"].numpy()
            index.append(idx.astype(np.int32))
            sizes.append(len(idx))
        assert (grid >= 0).all() and len(set(sizes)) == 1
        fx[f"aug{a}_grid"] = grid.astype(np.int32)
        fx[f"aug{a}_feat"] = feat
        fx[f"aug{a}_frag_index"] = np.stack(index)
        fx[f"aug{a}_frag_sizes"] = np.array(sizes, dtype=np.int64)
        _, cnt = np.unique(grid, axis=0, return_counts=True)
        counts_seen |= set(np.minimum(cnt, 3).tolist())
        most = max(most, len(parts))
        print(f"aug {a}: coord {fx[f'aug{a}_coord'].dtype}, {len(parts)} fragments of {sizes[0]} rows")
    fx["num_aug"] = np.int64(len(tc["aug_transform"]))
    assert counts_seen == {1, 2, 3} and most >= 4, (counts_seen, most)
    path = os.path.join(OUT, "testtime_nuscenes.npz")
    np.savez_compressed(path, **fx)
    size = os.path.getsize(path)
    print(f"{n_raw} raw rows -> {n} ({100 * (1 - n / n_raw):.1f} % dropped); {os.path.basename(path)}: {size} bytes")
    assert size < (1 << 20), size


if __name__ == "__main__":
    main()
