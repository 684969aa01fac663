"""Record the reference's train-time transform lists on synthetic scans -> tests/golden/traintime_*.npz (data only).

Runs ONLY where the reference checkout is available (environment variable CDSEG_REFERENCE): it imports the reference's
pointcept/datasets/transform.py by file, wraps ``random.random`` and the ``np.random`` functions the transforms call so that
every draw is logged, and runs the real transform classes of configs/{scannet,nuscenes}/CDSegNet.py stage by stage.

Per fixture <tag> three files (each below the size limit of a committed file):
  traintime_<tag>_raw.npz    raw coord / color / normal / strength / segment, cfg_json (the transform list), the scalar draws
                             and the small array draws under "<i>.<name>" (cdsegnet_amd/traintime.py)
  traintime_<tag>_draws.npz  the (n,3) normal draws of RandomJitter / ChromaticJitter under "<i>.normal"
  traintime_<tag>_ref.npz    the reference's state before GridSample (pre_coord in the reference's dtype, pre_color,
                             pre_normal, pre_index, pre_grid = every row's voxel), GridSample's selection (grid_sel = rows of the pre-GridSample state,
                             grid_coord of those rows), SphereCrop's (crop_sel = rows of the GridSample output, crop_center)

Fixtures: A - ScanNet train list, a seed where a rotation fires (float64 chain); B - a seed where none fires (float32
chain) and the dropout applies; C - grid_size 0.1, SphereCrop(point_max=2048): most voxels hold >= 2 points, the crop cuts;
D - the edges: the elastic coin fails, every voxel holds one point, N <= point_max; E - the nuScenes train list with strength.
"""
import importlib.util
import json
import os
import random
import runpy
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("CDSEG_REFERENCE")  # the reference checkout (Pointcept + CDSegNet), as for oracle/make_golden.py
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

# draws each transform consumes, in order: (function, field)
CONSUMES = {
    "RandomDropout": [("random", "coin"), ("choice", "idx")],
    "RandomRotate": [("random", "coin"), ("uniform", "angle")],
    "RandomScale": [("uniform", "scale")],
    "RandomFlip": [("rand", "coin_x"), ("rand", "coin_y")],
    "RandomJitter": [("randn", "normal")],
    "ElasticDistortion": [("random", "coin"), ("randn", "noise0"), ("randn", "noise1")],
    "ChromaticAutoContrast": [("rand", "coin"), ("rand", "blend")],
    "ChromaticTranslation": [("rand", "coin"), ("rand", "rand")],
    "ChromaticJitter": [("rand", "coin"), ("randn", "normal")],
    "GridSample": [("randint", "r")],
    "SphereCrop": [("randint", "center")],
}


class Recorder:
    """Logs (function name, value) of every draw the reference's transforms make."""

    def __init__(self):
        self.log = []
        self._saved = []

    def _wrap(self, mod, name):
        fn = getattr(mod, name)
        self._saved.append((mod, name, fn))

        def wrapped(*a, **k):
            v = fn(*a, **k)
            self.log.append((name, np.array(v)))
            return v
        setattr(mod, name, wrapped)

    def __enter__(self):
        self._wrap(random, "random")
        for name in ("uniform", "rand", "randn", "choice", "randint"):
            self._wrap(np.random, name)
        return self

    def __exit__(self, *exc):
        for mod, name, fn in self._saved:
            setattr(mod, name, fn)


def load_reference_transforms():
    sys.path.insert(0, REF)
    spec = importlib.util.spec_from_file_location("_ref_transform", os.path.join(REF, "pointcept/datasets/transform.py"))
    T = importlib.util.module_from_spec(spec)
    sys.modules["_ref_transform"] = T  # the reference's Registry infers its scope from the defining module
    spec.loader.exec_module(T)
    return T


def room_cloud(rng, n, lattice=None):
    """Points on the walls, floor and ceiling of a 4 x 3 x 2.5 m room offset from the origin, axis-aligned normals.
    lattice: spacing of a jittered volume lattice instead (every point alone in its 2 cm voxel after the augmentations)."""
    dims = np.array([4.0, 3.0, 2.5])
    if lattice is not None:
        cells = np.stack(np.meshgrid(*[np.arange(int(d / lattice)) for d in dims], indexing="ij"), -1).reshape(-1, 3)
        coord = cells[rng.permutation(len(cells))[:n]] * lattice + rng.uniform(0.0, 0.005, (n, 3))
        normal = np.eye(3)[rng.integers(0, 3, n)]
    else:
        axis = rng.choice(3, n, p=[15 / 59, 20 / 59, 24 / 59])  # by area: x walls, y walls, floor + ceiling
        side = rng.integers(0, 2, n)
        coord = rng.random((n, 3)) * dims
        coord[np.arange(n), axis] = side * dims[axis]
        normal = np.zeros((n, 3))
        normal[np.arange(n), axis] = 1.0 - 2.0 * side
    coord = (coord + np.array([1.5, -0.7, 0.3])).astype(np.float32)
    color = rng.integers(0, 256, (n, 3)).astype(np.float32)
    segment = rng.integers(0, 20, n).astype(np.int64)
    return dict(coord=coord, color=color, normal=normal.astype(np.float32), segment=segment)


def lidar_cloud(rng, n):
    from cdsegnet_amd import synth
    sc = synth.lidar_scene(3, n)
    m = len(sc["coord"])
    coord = (sc["coord"] + rng.uniform(-0.02, 0.02, (m, 3))).astype(np.float32)
    return dict(coord=coord, strength=rng.random((m, 1)).astype(np.float32), segment=rng.integers(0, 16, m).astype(np.int64))


def run_reference(T, cfg, raw, seed):
    """The reference's transforms one by one -> (draws by field, recorded stages)."""
    random.seed(seed)
    np.random.seed(seed)
    data = {k: v.copy() for k, v in raw.items()}
    n = len(raw["coord"])
    data["segment"] = np.arange(n, dtype=np.int64)  # carries the raw row through every selection
    draws, ref = {}, {}
    with Recorder() as rec:
        for i, c in enumerate(cfg):
            if c["type"] in ("ToTensor", "Collect"):
                continue
            t = T.TRANSFORMS.build(dict(c))
            mark = len(rec.log)
            if c["type"] == "GridSample":
                ref["pre_coord"], ref["pre_index"] = data["coord"].copy(), data["segment"].copy()
                for k in ("color", "normal"):
                    if k in data:
                        ref["pre_" + k] = data[k].copy()
                data["segment"] = np.arange(len(data["coord"]), dtype=np.int64)
                # every row's voxel: a second GridSample with return_inverse on a copy, outside the recorded stream
                state, keep = np.random.get_state(), len(rec.log)
                probe = T.TRANSFORMS.build(dict(c, return_inverse=True))({k: v.copy() for k, v in data.items()})
                ref["pre_grid"] = probe["grid_coord"][probe["inverse"]].astype(np.int32)
                np.random.set_state(state)
                del rec.log[keep:]
            if c["type"] == "SphereCrop":
                ref["crop_applied"] = np.int64(len(data["coord"]) > c["point_max"])
                data["segment"] = np.arange(len(data["coord"]), dtype=np.int64)
            data = t(data)
            if c["type"] == "GridSample":
                ref["grid_sel"], ref["grid_coord"] = data["segment"].copy(), data["grid_coord"].copy()
            if c["type"] == "SphereCrop":
                ref["crop_sel"] = data["segment"].copy()
            used = rec.log[mark:]
            names = CONSUMES.get(c["type"], [])
            assert len(used) <= len(names), (c["type"], [u[0] for u in used])
            for (fn, field), (got, val) in zip(names, used):
                assert fn == got, (c["type"], fn, got)
                if field.startswith("noise"):
                    val = val.astype(np.float32)  # transform.py:757
                draws[f"{i}.{field}"] = val
    ref["out_count"] = np.int64(len(data["coord"]))
    return draws, ref


def save(tag, cfg, raw, draws, ref, seed):
    big = {k: v for k, v in draws.items() if k.endswith(".normal")}
    small = {k: v for k, v in draws.items() if k not in big}
    files = {"raw": dict(raw, cfg_json=np.array(json.dumps(cfg)), seed=np.int64(seed), **small), "draws": big, "ref": ref}
    for part, arrays in files.items():
        path = os.path.join(OUT, f"traintime_{tag}_{part}.npz")
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        assert size < (1 << 20), (path, size)
        print(f"  {os.path.basename(path)}: {size} bytes")


def record_mix3d():
    """point_collate_fn's offsets (pointcept/datasets/utils.py:44-55) for 1..6 scenes, with the coin below and above mix_prob."""
    import torch
    spec = importlib.util.spec_from_file_location("_ref_dataset_utils", os.path.join(REF, "pointcept/datasets/utils.py"))
    U = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(U)
    rng = np.random.default_rng(7)
    out, case, real = {}, 0, random.random
    try:
        for nb in range(1, 7):
            sizes = rng.integers(5, 40, nb)
            for coin in (0.3, 0.9):
                random.random = lambda coin=coin: coin
                batch = U.point_collate_fn([dict(coord=torch.zeros(int(k), 3), offset=torch.tensor([int(k)])) for k in sizes], mix_prob=0.8)
                out[f"{case}.sizes"], out[f"{case}.coin"] = sizes.astype(np.int64), np.float64(coin)
                out[f"{case}.offset"] = batch["offset"].numpy().astype(np.int64)
                case += 1
    finally:
        random.random = real
    np.savez_compressed(os.path.join(OUT, "traintime_mix3d.npz"), mix_prob=np.float64(0.8), cases=np.int64(case), **out)
    print(f"mix3d: {case} cases")


def find(T, cfg, raw, want, seeds=range(400)):
    for seed in seeds:
        draws, ref = run_reference(T, cfg, raw, seed)
        if want(draws, ref):
            return seed, draws, ref
    raise SystemExit("no seed satisfies the fixture's condition")


def main():
    if not REF or not os.path.isdir(REF):
        raise SystemExit("set CDSEG_REFERENCE to the reference checkout")
    T = load_reference_transforms()
    scannet = runpy.run_path(os.path.join(REF, "configs/scannet/CDSegNet.py"))["data"]["train"]["transform"]
    nuscenes = runpy.run_path(os.path.join(REF, "configs/nuscenes/CDSegNet.py"))["data"]["train"]["transform"]
    scannet, nuscenes = [dict(c) for c in scannet], [dict(c) for c in nuscenes]
    pos = {c["type"]: i for i, c in enumerate(scannet)}
    rot = [i for i, c in enumerate(scannet) if c["type"] == "RandomRotate"]
    drop, ela, gsi, crop = pos["RandomDropout"], pos["ElasticDistortion"], pos["GridSample"], pos["SphereCrop"]

    def fired(d):
        return [f"{i}.angle" in d for i in rot]

    def sub(cfg, **changes):
        out = [dict(c) for c in cfg]
        for typ, kv in changes.items():
            out[pos[typ]].update(kv)
        return out

    rng = np.random.default_rng(2026)
    cases = [
        ("A", scannet, room_cloud(rng, 12000), lambda d, r: all(fired(d)) and f"{ela}.noise1" in d and f"{drop}.idx" not in d),
        ("B", scannet, room_cloud(rng, 12000), lambda d, r: not any(fired(d)) and f"{drop}.idx" in d and f"{ela}.noise1" in d),
        ("C", sub(scannet, GridSample=dict(grid_size=0.1), SphereCrop=dict(point_max=2048)), room_cloud(rng, 12000),
         lambda d, r: any(fired(d)) and f"{ela}.noise1" in d and int(r["crop_applied"]) == 1),
        ("D", scannet, room_cloud(rng, 12000, lattice=0.1),
         lambda d, r: f"{ela}.noise0" not in d and len(r["grid_sel"]) == len(r["pre_coord"]) and int(r["crop_applied"]) == 0),
        ("E", nuscenes, lidar_cloud(rng, 6000), lambda d, r: True),
    ]
    for tag, cfg, raw, want in cases:
        seed, draws, ref = find(T, cfg, raw, want)
        print(f"{tag}: seed {seed}, {len(raw['coord'])} raw rows -> {int(ref['out_count'])}, pre-GridSample coord {ref['pre_coord'].dtype}")
        save(tag, cfg, raw, draws, ref, seed)
    record_mix3d()


if __name__ == "__main__":
    main()
