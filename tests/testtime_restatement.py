"""TEST INFRASTRUCTURE - numpy restatement of the device test-time pipeline (cdsegnet_amd/testtime.py TestPipeline,
csrc/testtime.hip): the same operations in the same order and precision, with stable sorts and the packed voxel key, so the
GPU tests compare integers and bit patterns; the CPU tests compare THIS against the fixture recorded from the reference's own
transform classes (tools/make_testtime_golden.py).

A rotation is np.dot with the float64 matrix, like the reference (the device's fused multiply-adds give the same bits for the
configs' multiples of pi / 2, see tta_kernel); everything else is one correctly rounded operation per step.
"""
import numpy as np

from cdsegnet_amd import testtime as tt

F32, F64 = np.float32, np.float64


def voxel_grid(coord, grid_size):
    """floor(float64(coord) / grid_size) - min, int64 (n,3)."""
    g = np.floor(np.asarray(coord).astype(F64) / F64(grid_size)).astype(np.int64)
    return g - g.min(0)


def voxel_runs(grid):
    """Stable sort by the packed key -> (idx_sort, start (m,), count (m,), cluster (n,) = voxel rank of every SORTED position)."""
    key = (grid[:, 0] << 42) | (grid[:, 1] << 21) | grid[:, 2]
    idx_sort = np.argsort(key, kind="stable")
    ks = key[idx_sort]
    first = np.concatenate([[True], ks[1:] != ks[:-1]])
    start = np.flatnonzero(first)
    count = np.diff(np.concatenate([start, [len(ks)]]))
    return idx_sort, start, count, np.cumsum(first) - 1


def grid_sample_train(coord, grid_size, r):
    """-> (pick (m,) rows kept, in voxel key order; inverse (n,) voxel rank of every row; grid (n,3))."""
    grid = voxel_grid(coord, grid_size)
    idx_sort, start, count, cluster = voxel_runs(grid)
    r = np.asarray(r, dtype=np.int64).reshape(-1)
    r = r[np.arange(len(start)) % len(r)]
    pick = idx_sort[start + r % count]
    inverse = np.empty(len(grid), dtype=np.int64)
    inverse[idx_sort] = cluster
    return pick, inverse, grid


def center_shift(coord, apply_z):
    """In the array's own precision (transform.py:142-155)."""
    t = coord.dtype.type
    mn, mx = coord.min(0), coord.max(0)
    shift = np.array([(mn[0] + mx[0]) / t(2), (mn[1] + mx[1]) / t(2), mn[2] if apply_z else t(0)], dtype=coord.dtype)
    return coord - shift


def augment(steps, coord, normal=None):
    """One aug_transform list (parse_test's steps) under numpy's promotions."""
    for kind, v in steps:
        if kind == "rotate":
            rot = np.array(tt._rot_z(v), dtype=F64)
            coord = np.dot(coord, rot.T)
            normal = None if normal is None else np.dot(normal, rot.T)
        elif kind == "scale":
            coord = (coord.astype(F64) * F64(v)).astype(coord.dtype)
        else:
            coord = coord * np.array([-1, -1, 1], dtype=coord.dtype)
            normal = None if normal is None else normal * np.array([-1, -1, 1], dtype=normal.dtype)
    return coord, normal


def fragments(coord, grid_size, max_fragments=None):
    """GridSample(mode="test"): (grid (n,3), index (F,m)): fragment f holds member f % count_v of voxel v, voxels in key order."""
    grid = voxel_grid(coord, grid_size)
    idx_sort, start, count, _ = voxel_runs(grid)
    nfrag = int(count.max()) if max_fragments is None else min(int(count.max()), max_fragments)
    index = np.stack([idx_sort[start + f % count] for f in range(nfrag)])
    return grid, index


def pipeline(cfg_data_test, raw, r=None, max_fragments=None):
    """The whole of TestPipeline.prepare on numpy arrays.  raw: coord (+ color, normal | strength, segment); r: the member pick of
    the train-mode GridSample (needed when the transform list holds one).  -> dict(n, coord, segment, pick, inverse,
    origin_segment, grid, augs=[dict(coord, grid, index (F,m), frag_coord (F,m,3) f32, frag_grid, frag_feat)])."""
    plan = tt.parse_test(cfg_data_test)
    n_raw = len(raw["coord"])
    st = {k: (np.asarray(raw[k]).astype(F32).reshape(n_raw, -1) if raw.get(k) is not None else None)
          for k in ("coord", "color", "normal", "strength")}
    st["segment"] = np.asarray(raw["segment"]).reshape(n_raw) if raw.get("segment") is not None else None
    out = dict(pick=None, inverse=None, origin_segment=None, grid=None)
    for typ, o in plan["transform"]:
        if typ == "CenterShift":
            st["coord"] = center_shift(st["coord"], o["apply_z"])
        elif typ == "NormalizeColor":
            if st["color"] is not None:
                st["color"] = st["color"] / F32(127.5) + F32(-1.0)
        elif typ == "Copy":
            for src, dst in o["keys_dict"].items():
                out[dst] = st[src].copy()
        else:
            out["pick"], out["inverse"], out["grid"] = grid_sample_train(st["coord"], o["grid_size"], r)
            for k in st:
                if st[k] is not None:
                    st[k] = st[k][out["pick"]]
    out.update(n=len(st["coord"]), coord=st["coord"], segment=st["segment"], augs=[])
    for steps in plan["augs"]:
        c, nrm = augment(steps, st["coord"], st["normal"])
        parts = [c if k == "coord" else (nrm if k == "normal" else st[k]) for k in plan["feat_keys"]]
        feat = np.concatenate([p.astype(F32) for p in parts], 1)
        grid, index = fragments(c, plan["voxelize"]["grid_size"], max_fragments)
        fc = c[index]  # (F,m,3) in c's dtype
        if plan["shift"]:
            fc = np.stack([center_shift(x, False) for x in fc])
        out["augs"].append(dict(coord=c, grid=grid, index=index.astype(np.int32), frag_coord=fc.astype(F32),
                                frag_grid=grid[index].astype(np.int32), frag_feat=feat[index]))
    return out
