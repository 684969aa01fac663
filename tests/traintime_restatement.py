"""TEST INFRASTRUCTURE - numpy restatement of the device train-time pipeline (cdsegnet_amd/traintime.py, csrc/traintime.hip).

It performs the device's float64 operations one by one in the device's order (numpy never fuses a multiply and an add), with
stable sorts, so the GPU tests compare integers and bit patterns; the CPU tests compare THIS against fixtures recorded from
the reference's own transform classes (tools/make_traintime_golden.py), within the float32 rounding of the reference chain.
Every stage is a function of its own so that a test can feed it a stage input recorded from the reference.
"""
import numpy as np

from cdsegnet_amd import traintime as tt

F32, F64 = np.float32, np.float64


def bbox(x):
    x = np.asarray(x)
    return np.concatenate([x.min(0), x.max(0)]).astype(F64)


def center_shift(coord, apply_z):
    mm = bbox(coord)
    c = np.array([(mm[0] + mm[3]) / 2.0, (mm[1] + mm[4]) / 2.0, mm[2] if apply_z else 0.0])
    return coord - c


def rotate(xyz, rot, center=None):
    """(xyz - c) R^T + c with out_j = (t0 R[j][0] + t1 R[j][1]) + t2 R[j][2]; center: None (no translation), "bbox", or 3 numbers."""
    t = np.asarray(xyz, dtype=F64)
    c = None
    if isinstance(center, str):
        mm = bbox(t)
        c = np.array([(mm[0] + mm[3]) / 2.0, (mm[1] + mm[4]) / 2.0, (mm[2] + mm[5]) / 2.0])
    elif center is not None:
        c = np.asarray(center, dtype=F64)
    if c is not None:
        t = t - c
    r = np.asarray(rot, dtype=F64)
    o = np.stack([(t[:, 0] * r[j, 0] + t[:, 1] * r[j, 1]) + t[:, 2] * r[j, 2] for j in range(3)], 1)
    return o + c if c is not None else o


def flip(xyz, fx, fy):
    out = np.array(xyz, dtype=F64)
    if fx:
        out[:, 0] = -out[:, 0]
    if fy:
        out[:, 1] = -out[:, 1]
    return out


def jitter(coord, z, sigma, clip):
    return coord + np.minimum(np.maximum(F64(sigma) * np.asarray(z, dtype=F64), -clip), clip)


def blur(noise):
    """Box filter along x, y, z, twice: float64 accumulation left to right with the float32 weight 1/3, float32 per pass."""
    w = F64(F32(1.0) / F32(3.0))
    a = np.asarray(noise, dtype=F32)
    for _ in range(2):
        for axis in range(3):
            x = np.moveaxis(a, axis, 0).astype(F64)
            acc = np.zeros_like(x)
            acc[1:] = acc[1:] + w * x[:-1]
            acc = acc + w * x
            acc[:-1] = acc[:-1] + w * x[1:]
            a = np.moveaxis(acc.astype(F32), 0, axis)
    return np.ascontiguousarray(a)


def elastic_apply(coord, noise_blurred, granularity, magnitude):
    dim, start, step, stop = tt.elastic_axes(bbox(coord), granularity)
    assert tuple(dim) == tuple(noise_blurred.shape[:3]), (dim, noise_blurred.shape)
    return elastic_interp(coord, noise_blurred, start, step, stop, magnitude)


def elastic_interp(coord, noise_blurred, start, step, stop, magnitude):
    """coord + trilinear(noise)(coord) * magnitude on the axes linspace(start, stop, dim); unchanged outside them."""
    dim = noise_blurred.shape[:3]
    n = coord.shape[0]
    inside = np.ones(n, dtype=bool)
    ks, w0s, w1s = [], [], []
    for a in range(3):
        ax = np.arange(dim[a]).astype(F64) * step[a] + start[a]
        ax[-1] = stop[a]
        assert np.array_equal(ax, np.linspace(start[a], stop[a], dim[a]))  # the device's axis formula IS numpy's linspace
        x = coord[:, a]
        inside &= (x >= start[a]) & (x <= stop[a])
        j = np.clip(np.floor((x - start[a]) / step[a]), 0, dim[a] - 2).astype(np.int64)
        for _ in range(2):
            j = np.where((j > 0) & (x < ax[j]), j - 1, j)
        for _ in range(2):
            j = np.where((j < dim[a] - 2) & (x >= ax[np.minimum(j + 1, dim[a] - 1)]), j + 1, j)
        w1 = (x - ax[j]) / (ax[j + 1] - ax[j])
        ks.append(j)
        w1s.append(w1)
        w0s.append(1.0 - w1)
    v = np.zeros((n, 3), dtype=F64)
    for corner in range(8):
        b = (corner >> 2, (corner >> 1) & 1, corner & 1)
        wgt = ((w1s[0] if b[0] else w0s[0]) * (w1s[1] if b[1] else w0s[1])) * (w1s[2] if b[2] else w0s[2])
        v = v + noise_blurred[ks[0] + b[0], ks[1] + b[1], ks[2] + b[2]].astype(F64) * wgt[:, None]
    out = coord + v * F64(magnitude)
    return np.where(inside[:, None], out, coord)


def color_chain(color, blend=None, tr=None, noise=None, noise_mul=0.0):
    c = np.array(color, dtype=F32)
    if blend is not None:
        lo, hi = c.min(0), c.max(0)
        scale = F32(255.0) / (hi - lo)
        contrast = (c - lo) * scale
        c = F32(1.0 - float(blend)) * c + F32(blend) * contrast
    if tr is not None:
        c = np.minimum(np.maximum(np.asarray(tr, dtype=F64).reshape(1, 3) + c.astype(F64), 0.0), 255.0).astype(F32)
    if noise is not None:
        c = np.minimum(np.maximum(np.asarray(noise, dtype=F64) * F64(noise_mul) + c.astype(F64), 0.0), 255.0).astype(F32)
    return c


def grid_sample(coord, grid_size, r):
    """-> dict(grid (n,3) int32 per input row, key_order: voxel keys ascending, seg_start, idx_sort, pick (m,) input rows)."""
    grid = np.floor(np.asarray(coord, dtype=F64) / F64(grid_size)).astype(np.int64)
    grid -= grid.min(0)
    key = (grid[:, 0] << 42) | (grid[:, 1] << 21) | grid[:, 2]
    idx_sort = np.argsort(key, kind="stable")
    ks = key[idx_sort]
    first = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
    seg_start = np.concatenate([first, [len(ks)]])
    count = np.diff(seg_start)
    m = len(count)
    r = np.asarray(r, dtype=np.int64).reshape(-1)
    r = r[np.arange(m) % len(r)]
    pick = idx_sort[seg_start[:-1] + np.maximum(r, 0) % count]
    return dict(grid=grid.astype(np.int32), idx_sort=idx_sort, seg_start=seg_start, count=count, pick=pick)


def sphere_crop(coord, center, point_max):
    """Rows of the point_max nearest points to row `center`, in (float64 squared distance, row) order."""
    d = np.asarray(coord, dtype=F64) - np.asarray(coord, dtype=F64)[center]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return np.argsort(d2, kind="stable")[:point_max], d2


def run(transform_cfg, raw, draws, trace=None):
    """The whole pipeline with recorded draws.  raw: numpy arrays.  -> the output dict (numpy), `trace` (a dict, if given)
    receives the state before GridSample (coord float64, color, normal, index) and the GridSample / SphereCrop selections."""
    steps = tt.parse(transform_cfg)
    host = tt.HostDraws(draws, 0, 0)
    n = raw["coord"].shape[0]
    st = dict(coord=raw["coord"].astype(F64), normal=None if raw.get("normal") is None else raw["normal"].astype(F64),
              color=None if raw.get("color") is None else raw["color"].astype(F32).copy(),
              strength=None if raw.get("strength") is None else raw["strength"].astype(F32).reshape(n, -1),
              segment=None if raw.get("segment") is None else np.asarray(raw["segment"]).reshape(n),
              index=np.arange(n, dtype=np.int32), grid_coord=None)

    def gather(idx):
        for k in ("coord", "normal", "color", "strength", "segment", "index", "grid_coord"):
            if st[k] is not None:
                st[k] = st[k][idx]

    for i, (typ, o) in enumerate(steps):
        if typ == "CenterShift":
            st["coord"] = center_shift(st["coord"], o["apply_z"])
        elif typ == "RandomDropout":
            if host.scalar(i, "coin") < o["dropout_application_ratio"]:
                gather(np.asarray(draws[f"{i}.idx"]).reshape(-1).astype(np.int64))
        elif typ == "RandomRotate":
            if not host.scalar(i, "coin") > o["p"]:
                rot = tt.rotation_matrix(o["axis"], host.scalar(i, "angle"))
                st["coord"] = rotate(st["coord"], rot, "bbox" if o["center"] is None else o["center"])
                if st["normal"] is not None:
                    st["normal"] = rotate(st["normal"], rot)
        elif typ == "RandomScale":
            st["coord"] = st["coord"] * F64(host.scalar(i, "scale"))
        elif typ == "RandomFlip":
            fx, fy = host.scalar(i, "coin_x") < o["p"], host.scalar(i, "coin_y") < o["p"]
            st["coord"] = flip(st["coord"], fx, fy)
            if st["normal"] is not None:
                st["normal"] = flip(st["normal"], fx, fy)
        elif typ == "RandomJitter":
            st["coord"] = jitter(st["coord"], draws[f"{i}.normal"], o["sigma"], o["clip"])
        elif typ == "ElasticDistortion":
            if host.scalar(i, "coin") < 0.95:
                for k, (gran, mag) in enumerate(o["distortion_params"]):
                    st["coord"] = elastic_apply(st["coord"], blur(draws[f"{i}.noise{k}"]), gran, mag)
        elif typ in tt._CHROMA:
            if st["color"] is not None and host.scalar(i, "coin") < o["p"]:
                if typ == "ChromaticAutoContrast":
                    st["color"] = color_chain(st["color"], blend=host.scalar(i, "blend") if o["blend_factor"] is None else o["blend_factor"])
                elif typ == "ChromaticTranslation":
                    st["color"] = color_chain(st["color"], tr=(host.vec3(i, "rand") - 0.5) * 255 * 2 * o["ratio"])
                else:
                    st["color"] = color_chain(st["color"], noise=draws[f"{i}.normal"], noise_mul=o["std"] * 255)
        elif typ == "NormalizeColor":
            if st["color"] is not None:
                st["color"] = st["color"] / F32(127.5) + F32(-1.0)
        elif typ == "GridSample":
            if trace is not None:
                trace.update(pre_coord=st["coord"].copy(), pre_color=None if st["color"] is None else st["color"].copy(),
                             pre_normal=None if st["normal"] is None else st["normal"].copy(), pre_index=st["index"].copy())
            gs = grid_sample(st["coord"], o["grid_size"], draws[f"{i}.r"])
            st["grid_coord"] = gs["grid"]
            if trace is not None:
                trace["gridsample"] = gs
            gather(gs["pick"])
        elif typ == "SphereCrop":
            if st["coord"].shape[0] > o["point_max"]:
                sel, _ = sphere_crop(st["coord"], host.index(i, "center", st["coord"].shape[0]), o["point_max"])
                if trace is not None:
                    trace["crop_input_index"] = st["index"].copy()
                gather(sel)
        elif typ == "Collect":
            coord32 = st["coord"].astype(F32)
            feat = np.concatenate([(coord32 if k == "coord" else st[k]).astype(F32).reshape(len(coord32), -1) for k in o["feat_keys"]], 1)
            m = coord32.shape[0]
            return dict(coord=coord32, coord64=st["coord"], grid_coord=st["grid_coord"], segment=st["segment"], feat=feat,
                        offset=np.array([m], dtype=np.int64), index=st["index"])
    raise AssertionError("no Collect")
