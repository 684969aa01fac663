"""Train-time data pipeline on the GPU: raw scan -> the dict the training forward takes.

ref: configs/{scannet,scannet200,nuscenes}/CDSegNet.py (the ``train`` and ``val`` dataset blocks), pointcept/datasets/
transform.py, pointcept/datasets/utils.py:44-55 (point_collate_fn).  The reference runs these transform lists with numpy /
scipy in CPU dataloader workers; here every per-point step is a device kernel (csrc/traintime.hip) and GridSample reuses the
test-time pipeline's voxel keys, radix sort and run segmentation (csrc/testtime.hip, csrc/serialize.hip).

    tf = TrainTransform(cfg.data.train.transform, seed=0)        # the reference's list of dict(type=..., ...), unchanged
    batch = collate([tf(raw_a, 0), tf(raw_b, 1)], mix_prob=0.8)  # -> model(batch)

Supported types (everything the six shipped lists use): CenterShift, RandomDropout, RandomRotate, RandomScale (isotropic),
RandomFlip, RandomJitter, ElasticDistortion, ChromaticAutoContrast, ChromaticTranslation, ChromaticJitter,
GridSample(mode="train", return_grid_coord=True), SphereCrop(mode="random"), NormalizeColor, ToTensor, Collect.  Any other
type or option raises NotImplementedError when the TrainTransform is constructed.

Numerics.  The reference's coordinates become float64 at the first rotation that fires (np.dot with a float64 matrix,
transform.py:251) and stay float32 otherwise; here coordinates and normals are float64 from the first transform to the
output, where they are rounded to float32 once.  Rotation matrices, the elastic grid axes and every other scalar are computed
on the host with numpy, as the reference does; no float64 kernel contracts a multiply and an add, so the device results are
bit-equal to tests/traintime_restatement.py, a numpy restatement with the same operation order.  Colour stays float32 with
the reference's promotions.  Against the reference itself the float64 chain differs by a few float32 ulps of the largest
coordinate (profiles/NOTES.md), which moves a point that sits on a voxel face into the neighbouring voxel.

GridSample: voxels are keyed by the packed (x,y,z) integer, the sort is stable, so the members of a voxel are in row order
(numpy's default argsort in the reference is unstable) and the output rows are in key order.  Voxel membership and counts
equal the reference's; WHICH member integer r picks does not.  SphereCrop keeps the point_max rows nearest the centre row
in (distance, row) order.  RandomDropout keeps a uniformly random subset of int(n (1 - ratio)) rows.

Draws.  ``draws=None``: the scalar draws (coins, angles, scale, blend, colour shift, crop centre) come from a host
``random.Random`` keyed by (seed, scene_index), in the reference's consumption order; the per-row / per-voxel / per-cell
draws are generated on the device by the library's Philox (cdseg_randn, cdseg_rand_int) keyed by (seed, scene_index) with
one stream per transform - equal (seed, scene_index) gives equal output and no draw is a host-to-device copy of N values.
The sequence is NOT numpy's Mersenne-Twister stream of the reference and does not try to be.
``draws=`` a record: the pipeline is a pure function of (raw, record).  A record is a mapping; the draws of the transform at
position i of the list are stored under "<i>.<name>", in the order the reference consumes them:
    RandomDropout          <i>.coin   random.random()          applied when coin < dropout_application_ratio
                           <i>.idx    np.random.choice(...)    rows kept, in this order            (only when applied)
    RandomRotate           <i>.coin   random.random()          SKIPPED when coin > p
                           <i>.angle  np.random.uniform(a, b)  in units of pi                      (only when applied)
    RandomScale            <i>.scale  np.random.uniform(lo, hi)
    RandomFlip             <i>.coin_x, <i>.coin_y  np.random.rand()   flipped when coin < p
    RandomJitter           <i>.normal np.random.randn(n, 3)
    ElasticDistortion      <i>.coin   random.random()          applied when coin < 0.95
                           <i>.noise<k> np.random.randn(*noise_dim, 3).astype(float32), pair k     (only when applied)
    ChromaticAutoContrast  <i>.coin   np.random.rand()         applied when coin < p
                           <i>.blend  np.random.rand()         (only when applied and blend_factor is None)
    ChromaticTranslation   <i>.coin   np.random.rand() ; <i>.rand np.random.rand(1, 3)             (only when applied)
    ChromaticJitter        <i>.coin   np.random.rand() ; <i>.normal np.random.randn(n, 3)          (only when applied)
    GridSample             <i>.r      np.random.randint(0, count.max(), count.size); voxel v (in key order) uses
                                      r[v % len(r)]
    SphereCrop             <i>.center np.random.randint(n), taken modulo n                         (only when n > point_max)
Chromatic* draws are only consumed when the scan has colour, like the reference.

Host reads per scene (each one synchronises the stream): the voxel count of GridSample, and the bounding box of every
ElasticDistortion application (two for the shipped parameters) for ``noise_dim``: 3 for the ScanNet train list, 1 for
every val list and the nuScenes train list.  Nothing else synchronises.
"""
import random

import numpy as np
import torch

from . import ops

_CHROMA = ("ChromaticAutoContrast", "ChromaticTranslation", "ChromaticJitter")
_POINT_KEYS = ("coord", "color", "normal", "strength", "segment")
# type -> {option: default}; an option outside this table is rejected
_OPTIONS = {
    "CenterShift": dict(apply_z=True),
    "RandomDropout": dict(dropout_ratio=0.2, dropout_application_ratio=0.5),
    "RandomRotate": dict(angle=None, center=None, axis="z", always_apply=False, p=0.5),
    "RandomScale": dict(scale=None, anisotropic=False),
    "RandomFlip": dict(p=0.5),
    "RandomJitter": dict(sigma=0.01, clip=0.05),
    "ElasticDistortion": dict(distortion_params=None),
    "ChromaticAutoContrast": dict(p=0.2, blend_factor=None),
    "ChromaticTranslation": dict(p=0.95, ratio=0.05),
    "ChromaticJitter": dict(p=0.95, std=0.005),
    "GridSample": dict(grid_size=0.05, hash_type="fnv", mode="train", keys=("coord", "color", "normal", "segment"),
                       return_inverse=False, return_grid_coord=False, return_min_coord=False, return_displacement=False,
                       project_displacement=False),
    "SphereCrop": dict(point_max=80000, sample_rate=None, mode="random"),
    "NormalizeColor": dict(),
    "ToTensor": dict(),
    "Collect": dict(keys=None, offset_keys_dict=None, feat_keys=None),
}


def _reject(msg):
    raise NotImplementedError("cdsegnet_amd.traintime: " + msg)


def parse(transform_cfg):
    """Validate the reference's transform list -> [(type, options with defaults filled in)].  Raises NotImplementedError
    for every type / option the device pipeline does not implement."""
    steps = []
    for i, cfg in enumerate(transform_cfg):
        cfg = dict(cfg)
        typ = cfg.pop("type", None)
        if typ not in _OPTIONS:
            _reject(f"transform {i}: type {typ!r} is not supported")
        unknown = set(cfg) - set(_OPTIONS[typ])
        if unknown:
            _reject(f"transform {i} ({typ}): option(s) {sorted(unknown)} are not supported")
        o = dict(_OPTIONS[typ], **cfg)
        if typ == "RandomRotate":
            if o["axis"] not in ("x", "y", "z"):
                _reject(f"RandomRotate axis {o['axis']!r}")
            o["angle"] = [-1, 1] if o["angle"] is None else list(o["angle"])
            if o["center"] is not None and len(o["center"]) != 3:
                _reject("RandomRotate center must be None or three numbers")
            if o["always_apply"]:
                o["p"] = 1
        elif typ == "RandomScale":
            if o["anisotropic"]:
                _reject("RandomScale(anisotropic=True)")
            o["scale"] = [0.95, 1.05] if o["scale"] is None else list(o["scale"])
        elif typ == "RandomJitter":
            if not o["clip"] > 0:
                _reject("RandomJitter clip must be positive")
        elif typ == "ElasticDistortion":
            if o["distortion_params"] is None:
                o["distortion_params"] = [[0.2, 0.4], [0.8, 1.6]]
            o["distortion_params"] = [[float(g), float(m)] for g, m in o["distortion_params"]]
        elif typ == "GridSample":
            if o["mode"] != "train":
                _reject(f"GridSample(mode={o['mode']!r}): the test mode lives in cdsegnet_amd.testtime")
            if not o["return_grid_coord"]:
                _reject("GridSample(return_grid_coord=False): the model needs grid_coord")
            for k in ("return_inverse", "return_min_coord", "return_displacement", "project_displacement"):
                if o[k]:
                    _reject(f"GridSample({k}=True)")
            if o["hash_type"] not in ("fnv", "ravel"):
                _reject(f"GridSample(hash_type={o['hash_type']!r})")
            if not set(o["keys"]) <= set(_POINT_KEYS):
                _reject(f"GridSample(keys={o['keys']!r})")
            if not float(o["grid_size"]) > 0:
                _reject("GridSample grid_size must be positive")
        elif typ == "SphereCrop":
            if o["mode"] != "random":
                _reject(f"SphereCrop(mode={o['mode']!r})")
            if o["sample_rate"] is not None:
                _reject("SphereCrop(sample_rate=...)")
        elif typ == "Collect":
            if o["offset_keys_dict"] is not None:
                _reject("Collect(offset_keys_dict=...)")
            if o["keys"] is None or tuple(o["keys"]) != ("coord", "grid_coord", "segment"):
                _reject(f"Collect(keys={o['keys']!r}): only (coord, grid_coord, segment)")
            if not o["feat_keys"] or not set(o["feat_keys"]) <= {"coord", "color", "normal", "strength"}:
                _reject(f"Collect(feat_keys={o['feat_keys']!r})")
            if i != len(transform_cfg) - 1:
                _reject("Collect must be the last transform")
        steps.append((typ, o))
    types = [t for t, _ in steps]
    if not types or types[-1] != "Collect":
        _reject("the list must end with Collect")
    if types.count("GridSample") != 1:
        _reject("the list must hold exactly one GridSample")
    g = types.index("GridSample")
    for t in types[g + 1:]:
        if t not in ("SphereCrop", "CenterShift", "NormalizeColor", "ToTensor", "Collect"):
            _reject(f"{t} after GridSample")
    if "SphereCrop" in types[:g]:
        _reject("SphereCrop before GridSample")
    return steps


def rotation_matrix(axis, angle_pi):
    """rot_t of RandomRotate for angle = angle_pi * pi, with numpy's cos / sin (transform.py:233-240)."""
    angle = angle_pi * np.pi
    c, s = np.cos(angle), np.sin(angle)
    if axis == "x":
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    if axis == "y":
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def elastic_axes(bbox6, granularity):
    """noise_dim (3 ints) and the linspace parameters (start, step, stop: 3 doubles each) of one ElasticDistortion
    application from the float64 bounding box [min xyz, max xyz] (transform.py:753-779)."""
    bbox6 = np.asarray(bbox6, dtype=np.float64)
    cmin = bbox6[:3]
    dim = ((bbox6[3:] - cmin) // granularity).astype(int) + 3
    start = cmin - granularity
    stop = cmin + granularity * (dim - 2)
    step = (stop - start) / (dim - 1)
    return dim, start, step, stop


def host_rng(seed, scene_index):
    return random.Random((int(seed) << 32) ^ (int(scene_index) & 0xFFFFFFFF))


def philox_key(seed, scene_index):
    return ((int(scene_index) & 0xFFFFFFFF) << 32) | (int(seed) & 0xFFFFFFFF)


class HostDraws:
    """The scalar draws of one scene: recorded ones from a record, generated ones from random.Random(seed, scene_index).
    Shared by the device pipeline and by tests (it never touches the GPU)."""

    def __init__(self, record, seed, scene_index, made=None):
        self.record = record
        self.rng = None if record is not None else host_rng(seed, scene_index)
        self.made = made  # a dict: receives every generated draw under its record name

    def _keep(self, i, name, v):
        if self.made is not None:
            self.made[f"{i}.{name}"] = v
        return v

    def scalar(self, i, name, lo=0.0, hi=1.0):
        if self.record is not None:
            return float(np.asarray(_field(self.record, i, name)).reshape(-1)[0])
        return self._keep(i, name, lo + (hi - lo) * self.rng.random())

    def vec3(self, i, name):
        if self.record is not None:
            return np.asarray(_field(self.record, i, name), dtype=np.float64).reshape(3)
        return self._keep(i, name, np.array([self.rng.random() for _ in range(3)]))

    def index(self, i, name, n):
        if self.record is not None:
            return int(np.asarray(_field(self.record, i, name)).reshape(-1)[0]) % n
        return self._keep(i, name, self.rng.randrange(n))


def _field(record, i, name):
    key = f"{i}.{name}"
    if key not in record:
        raise KeyError(f"draws record lacks {key!r}")
    return record[key]


def _dev(x, dtype, device):
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=dtype).contiguous()
    return torch.as_tensor(np.ascontiguousarray(x)).to(device=device, dtype=dtype).contiguous()


class TrainTransform:
    def __init__(self, transform_cfg, seed=0):
        self.steps = parse(transform_cfg)
        self.seed = int(seed)

    # -- per-row / per-voxel / per-cell draws: from the record, or Philox streams keyed by (seed, scene, transform, k)
    def _normal(self, st, i, name, shape, k=0, dtype=torch.float64):
        if st["record"] is not None:
            z = _dev(_field(st["record"], i, name), dtype, st["dev"])
            if tuple(z.shape) != tuple(shape):
                raise ValueError(f"draws record {i}.{name}: shape {tuple(z.shape)}, the pipeline needs {tuple(shape)}")
            return z
        return st["host"]._keep(i, name, ops.randn(tuple(shape), st["key"], 16 * i + k, st["dev"]))

    def _gather(self, st, idx):
        for k in ("coord", "normal", "color", "strength", "segment", "index", "grid_coord"):
            if st.get(k) is not None:
                st[k] = ops.gather_rows(st[k], idx) if st[k].dim() > 1 else _gather1(st[k], idx)
        st["n"] = int(idx.numel())

    @torch.no_grad()
    def __call__(self, raw, scene_index, draws=None, trace=None):
        """raw: dict of device tensors (coord (N,3) float32, segment (N,), color / normal or strength) -> dict(coord float32,
        grid_coord int32, segment, feat float32, offset, offset_host, index = the raw row of every output row).  trace: a dict
        that receives the state before GridSample (pre_coord float64, pre_index), GridSample's sort / runs / picks and,
        with draws=None, the generated draws as a record ("draws")."""
        if "sampled_index" in raw:
            _reject("sampled_index (the data-efficient ScanNet split)")
        coord = raw["coord"]
        if not (isinstance(coord, torch.Tensor) and coord.is_cuda):
            raise ValueError("raw['coord'] must be a device tensor")
        if coord.dtype != torch.float32 or coord.dim() != 2 or coord.shape[1] != 3 or coord.shape[0] == 0:
            raise ValueError("raw['coord'] must be a non-empty (N, 3) float32 tensor")
        dev, n = coord.device, coord.shape[0]
        st = dict(dev=dev, n=n, record=draws, key=philox_key(self.seed, scene_index), grid_coord=None, trace=trace)
        host = st["host"] = HostDraws(draws, self.seed, scene_index, made={} if (trace is not None and draws is None) else None)
        if host.made is not None:
            trace["draws"] = host.made  # the generated draws as a record: replaying it reproduces this call
        ops.bind_stream()
        try:
            st["coord"] = ops.tt_affine(coord, out_dtype=torch.float64)  # exact widening
            st["normal"] = ops.tt_affine(raw["normal"].float(), out_dtype=torch.float64) if raw.get("normal") is not None else None
            st["color"] = raw["color"].float().contiguous().clone() if raw.get("color") is not None else None
            st["strength"] = raw["strength"].float().reshape(n, -1).contiguous() if raw.get("strength") is not None else None
            st["segment"] = raw["segment"].reshape(n).contiguous() if raw.get("segment") is not None else None
            st["index"] = torch.arange(n, dtype=torch.int32, device=dev)
            i = 0
            while i < len(self.steps):
                typ, o = self.steps[i]
                if typ in _CHROMA:
                    i = self._chroma(st, host, i)
                    continue
                getattr(self, "_" + typ)(st, host, i, o)
                i += 1
            return st["out"]
        finally:
            ops.unbind_stream()

    # ---------------------------------------------------------------- coordinate transforms
    def _CenterShift(self, st, host, i, o):
        st["coord"] = ops.tt_affine(st["coord"], center=ops.TT_CENTER_SHIFT_Z if o["apply_z"] else ops.TT_CENTER_SHIFT_XY,
                                    bbox=ops.tt_bbox(st["coord"]))

    def _RandomDropout(self, st, host, i, o):
        if not host.scalar(i, "coin") < o["dropout_application_ratio"]:
            return
        n = st["n"]
        keep = int(n * (1 - o["dropout_ratio"]))
        if st["record"] is not None:
            idx = _dev(_field(st["record"], i, "idx"), torch.int32, st["dev"]).reshape(-1)
            if idx.numel() != keep:
                raise ValueError(f"draws record {i}.idx holds {idx.numel()} rows, int(n (1 - ratio)) = {keep}")
        else:  # random 32-bit keys, stable radix sort: the first `keep` rows of the order are a uniform subset
            keys = ops.rand_int(n, st["key"], 16 * i, st["dev"])
            idx = host._keep(i, "idx", ops.sort_pairs(keys, None, end_bit=32)[1][:keep].contiguous())
        self._gather(st, idx)

    def _RandomRotate(self, st, host, i, o):
        if host.scalar(i, "coin") > o["p"]:
            return
        rot = rotation_matrix(o["axis"], host.scalar(i, "angle", o["angle"][0], o["angle"][1]))
        if o["center"] is None:
            st["coord"] = ops.tt_affine(st["coord"], center=ops.TT_CENTER_BBOX, bbox=ops.tt_bbox(st["coord"]), rot=rot,
                                        add_back=True)
        else:
            st["coord"] = ops.tt_affine(st["coord"], center=ops.TT_CENTER_HOST, center3=o["center"], rot=rot, add_back=True)
        if st["normal"] is not None:
            st["normal"] = ops.tt_affine(st["normal"], rot=rot)

    def _RandomScale(self, st, host, i, o):
        st["coord"] = ops.tt_affine(st["coord"], scale=host.scalar(i, "scale", o["scale"][0], o["scale"][1]))

    def _RandomFlip(self, st, host, i, o):
        fx = host.scalar(i, "coin_x") < o["p"]
        fy = host.scalar(i, "coin_y") < o["p"]
        if fx or fy:
            st["coord"] = ops.tt_affine(st["coord"], flipx=fx, flipy=fy)
            if st["normal"] is not None:
                st["normal"] = ops.tt_affine(st["normal"], flipx=fx, flipy=fy)

    def _RandomJitter(self, st, host, i, o):
        ops.tt_jitter(st["coord"], self._normal(st, i, "normal", (st["n"], 3)), o["sigma"], o["clip"])

    def _ElasticDistortion(self, st, host, i, o):
        if not host.scalar(i, "coin") < 0.95:
            return
        for k, (gran, mag) in enumerate(o["distortion_params"]):
            bbox = ops.tt_bbox(st["coord"]).cpu().numpy()  # host read: noise_dim is a shape
            dim, start, step, stop = elastic_axes(bbox, gran)
            noise = self._normal(st, i, f"noise{k}", (int(dim[0]), int(dim[1]), int(dim[2]), 3), k, torch.float32)
            ops.tt_elastic(st["coord"], ops.tt_blur(noise), start, step, stop, mag)

    # ---------------------------------------------------------------- colour: consecutive Chromatic* steps, one launch
    def _chroma(self, st, host, i):
        """Runs the Chromatic* steps starting at position i (auto contrast, translation, jitter, each at most once and in
        that order, share one launch) and returns the position after them."""
        rank = {t: k for k, t in enumerate(_CHROMA)}
        args, last = {}, -1
        while i < len(self.steps) and self.steps[i][0] in _CHROMA and rank[self.steps[i][0]] > last:
            typ, o = self.steps[i]
            last = rank[typ]
            if st["color"] is not None and host.scalar(i, "coin") < o["p"]:
                if typ == "ChromaticAutoContrast":
                    args["bbox"] = ops.tt_bbox(st["color"])
                    args["blend"] = host.scalar(i, "blend") if o["blend_factor"] is None else o["blend_factor"]
                elif typ == "ChromaticTranslation":
                    args["tr"] = (host.vec3(i, "rand") - 0.5) * 255 * 2 * o["ratio"]
                else:
                    args["noise"] = self._normal(st, i, "normal", (st["n"], 3))
                    args["noise_mul"] = o["std"] * 255
            i += 1
        if args:
            ops.tt_color(st["color"], **args)
        return i

    def _NormalizeColor(self, st, host, i, o):
        if st["color"] is not None:
            st["color"] = ops.div_add(st["color"], 127.5, -1.0)

    # ---------------------------------------------------------------- GridSample / SphereCrop
    def _GridSample(self, st, host, i, o):
        grid, key, _ = ops.voxelize_any(st["coord"], o["grid_size"])
        key_sorted, idx_sort = ops.sort_pairs(key, None, end_bit=63)
        _, seg_start, count = ops.pool_level(key_sorted, 0)
        m = int(count.item())  # host read: the number of voxels is the size of everything downstream
        if st["record"] is not None:
            r = _dev(_field(st["record"], i, "r"), torch.int64, st["dev"]).reshape(-1)
            if r.numel() != m:
                r = r[torch.arange(m, device=st["dev"]) % r.numel()].contiguous()
        else:
            r = host._keep(i, "r", ops.rand_int(m, st["key"], 16 * i, st["dev"], bound_dev=ops.max_run(seg_start, m)))
        pick = ops.tt_voxel_pick(idx_sort, seg_start, m, r)
        st["grid_coord"] = grid
        if st["trace"] is not None:
            st["trace"].update(pre_coord=st["coord"], pre_index=st["index"], grid=grid, idx_sort=idx_sort, seg_start=seg_start,
                               num_voxels=m, pick=pick)
        self._gather(st, pick)

    def _SphereCrop(self, st, host, i, o):
        n = st["n"]
        if n <= o["point_max"]:
            return
        key = ops.tt_dist_key(st["coord"], host.index(i, "center", n))
        self._gather(st, ops.sort_pairs(key, None, end_bit=63)[1][:o["point_max"]].contiguous())

    # ---------------------------------------------------------------- output
    def _ToTensor(self, st, host, i, o):
        pass

    def _Collect(self, st, host, i, o):
        n, dev = st["n"], st["dev"]
        coord = ops.tt_affine(st["coord"], out_dtype=torch.float32)
        parts = []
        for k in o["feat_keys"]:
            if k != "coord" and st.get(k) is None:
                raise KeyError(f"Collect(feat_keys=...): the scan has no {k!r}")
            parts.append(coord if k == "coord" else st[k])
        feat = parts[0].float() if parts[0].dtype != torch.float64 else ops.tt_affine(parts[0], out_dtype=torch.float32)
        for p in parts[1:]:
            feat = ops.collect_feat(feat, p if p.dtype == torch.float64 else p.float())
        st["out"] = dict(coord=coord, grid_coord=st["grid_coord"], segment=st["segment"], feat=feat,
                         offset=torch.tensor([n], dtype=torch.int64).to(dev, non_blocking=True), offset_host=[n],
                         index=st["index"])


def _gather1(x, idx):
    """x[idx] for a 1-D int32 / int64 / float32 tensor through the library's row gather."""
    return ops.gather_rows(x.reshape(-1, 1), idx).reshape(-1)


def mix3d_offsets(sizes, mix):
    """Cumulative offsets of scenes of ``sizes`` points; mix: the reference's Mix3D merge, offset[1:-1:2] + [offset[-1]]
    (pointcept/datasets/utils.py:50-55) - neighbouring scenes are merged pairwise into one point cloud."""
    off = list(np.cumsum(np.asarray(sizes, dtype=np.int64)))
    return [int(v) for v in (off[1:-1:2] + [off[-1]] if mix else off)]


def collate(dicts, mix_prob=0.0, rng=None):
    """point_collate_fn (pointcept/datasets/utils.py:44-55) on TrainTransform outputs: per-point arrays concatenated,
    cumulative offsets, and with probability mix_prob (one draw of ``rng.random()``, rng a random.Random - default the
    module ``random``, as in the reference) the Mix3D offset merge.  ``index`` stays per scene (raw rows of that scene)."""
    if not dicts:
        raise ValueError("collate needs at least one scene")
    rng = random if rng is None else rng
    out = {}
    for k in ("coord", "grid_coord", "segment", "feat", "index"):
        if all(d.get(k) is not None for d in dicts):
            out[k] = torch.cat([d[k] for d in dicts], 0)
    sizes = [int(d["offset_host"][-1]) for d in dicts]
    off = mix3d_offsets(sizes, rng.random() < mix_prob)
    out["offset_host"] = off
    out["offset"] = torch.tensor(off, dtype=torch.int64).to(dicts[0]["coord"].device, non_blocking=True)
    return out
