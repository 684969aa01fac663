"""Test-time pipeline around the model on the GPU: raw scan -> labels.

ref: configs/scannet/CDSegNet.py:253-398 (the ``test`` dataset block), pointcept/datasets/defaults.py:98-132
(prepare_test_data), pointcept/datasets/transform.py, pointcept/engines/test.py:197-279.  Per scene the reference
  1. transform:        CenterShift(apply_z=True), NormalizeColor                      (transform.py:142-155, :113-117)
  2. aug_transform:    13 test-time augmentations of the WHOLE scan: rotation about z by {0, 1/2, 1, 3/2} pi, each
                       plain / scaled 0.95 / scaled 1.05, plus one x-y flip            (:259-328)
  3. test_cfg.voxelize GridSample(grid_size, mode="test") on every augmented scan: ``count.max()`` fragments, fragment
                       i holds member ``i % count`` of every voxel                     (:821-897)
  4. post_transform:   CenterShift(apply_z=False) per fragment, ToTensor, Collect(keys=(coord, grid_coord, index),
                       feat_keys=(color, normal))                                      (:142-155, :27-50)
  5. tester:           model.inference on every fragment, pred[index] += softmax(logits), arg-max
                                                                                       (engines/test.py:197-279)
on CPU dataloader workers with numpy; here every step is a device kernel (csrc/testtime.hip) and the fragments of
all augmentations go through ``inference_many``.

Differences that cannot matter: voxels are keyed by a packed (x,y,z) integer instead of the FNV-1a hash (any injective
key forms the same groups); the sort is stable, so the members of a voxel are in original index order (numpy's default
argsort in the reference is unstable, i.e. platform dependent - SURVEY.md 8f): the per-point voxel coordinates are
compared exactly with the reference's (tests/golden/tta_pipeline.npz), fragment membership as sets per voxel.
Numerics follow numpy's promotions: a rotation multiplies float32 rows by a float64 matrix, so rotated coordinates
and normals are float64 from there on (GridSample divides float64), the flip stays float32.
"""
import math

import torch

from . import dist as cdist
from . import ops
from .traintime import _dev, _field, philox_key


def _rot_z(angle_pi):
    """rot_t of RandomRotateTargetAngle(axis="z") for angle = angle_pi * pi, with numpy's cos / sin VALUES
    (cos(pi/2) = 6.1e-17, not 0: the reference multiplies by exactly these doubles) - transform.py:272-279."""
    a = angle_pi * math.pi
    c, s = math.cos(a), math.sin(a)
    return [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]


# configs/scannet/CDSegNet.py:278-398 (the same list in the scannet200 config; the nuScenes config has its OWN test block -
# ten scale / flip lists, no rotation, no CenterShift, no colour - which TestPipeline below takes from the config):
# (rotation angle / pi, scale, flip)
SCANNET_TTA = ([(a, None, False) for a in (0, 0.5, 1, 1.5)] + [(a, 0.95, False) for a in (0, 0.5, 1, 1.5)] +
               [(a, 1.05, False) for a in (0, 0.5, 1, 1.5)] + [(None, None, True)])


def apply_aug(coord, normal, aug):
    """One aug_transform entry on the (already centre-shifted) scan: (coord', normal')."""
    angle, scale, flip = aug
    if angle is not None:
        rot = _rot_z(angle)
        return ops.tta_apply(coord, rot=rot, scale=scale), (None if normal is None else ops.tta_apply(normal, rot=rot))
    if flip:
        return ops.tta_apply(coord, flip=True), (None if normal is None else ops.tta_apply(normal, flip=True))
    return coord, normal


def grid_sample_test(coord, grid_size):
    """-> dict(grid_coord int32 (N,3), idx_sort, seg_start, num_voxels, num_fragments)."""
    n = coord.shape[0]
    grid, key, _ = ops.voxelize_any(coord, grid_size)
    key_sorted, idx_sort = ops.sort_pairs(key, None, end_bit=63)
    _, seg_start, count = ops.pool_level(key_sorted, 0)
    m = int(count.item())
    frags = int(ops.max_run(seg_start, m).item())
    return dict(grid_coord=grid, idx_sort=idx_sort, seg_start=seg_start, num_voxels=m, num_fragments=frags, n=n)


def fragment(gs, i):
    """Indices (into the raw cloud) of fragment i: one point per voxel."""
    return ops.fragment_select(gs["idx_sort"], gs["seg_start"], gs["num_voxels"], i)


def _fragment_dicts(gs, coord, feat, max_fragments=None):
    nfrag = gs["num_fragments"] if max_fragments is None else min(gs["num_fragments"], max_fragments)
    idxs, dicts = [], []
    for i in range(nfrag):
        idx = fragment(gs, i)
        m = idx.numel()
        idxs.append(idx)
        # post_transform: CenterShift(apply_z=False) on the fragment's own coordinates, Collect
        c = ops.center_shift(ops.gather_rows(coord, idx), apply_z=False)
        dicts.append(dict(coord=c, grid_coord=ops.gather_rows(gs["grid_coord"], idx), feat=ops.gather_rows(feat, idx),
                          index=idx, offset=torch.tensor([m], dtype=torch.int64, device=coord.device), offset_host=[m]))
    return idxs, dicts


def _vote(model, n, num_classes, idxs, dicts, device, noise_level, lanes):
    if hasattr(model, "inference_many"):
        outs = model.inference_many(dicts, lanes=lanes, noise_level=noise_level)
    else:
        outs = [model.inference(d, eval=False, noise_level=noise_level) for d in dicts]
    ops.bind_stream()
    try:
        pred = torch.zeros((n, num_classes), dtype=torch.float32, device=device)
        for idx, o in zip(idxs, outs):
            ops.softmax_vote(o["seg_logits"], idx, pred)
        labels = ops.argmax_rows(pred)
    finally:
        ops.unbind_stream()
    return labels, pred


@torch.no_grad()
def segment_scene(model, coord, feat, grid_size, num_classes, noise_level=None, max_fragments=None, lanes=4):
    """Fragmented inference + softmax voting of one scan whose ``coord`` / ``feat`` are already normalised (steps 3-5,
    no augmentation).  coord (N,3) f32, feat (N,C) f32 on the GPU.  Returns (labels int32 (N,), pred (N, classes) f32).
    The fragments are independent scenes for the model, so they go through ``inference_many`` (up to ``lanes`` in
    flight); the votes are accumulated afterwards in fragment order, exactly like the reference's loop."""
    ops.bind_stream()
    try:
        gs = grid_sample_test(coord, grid_size)
        idxs, dicts = _fragment_dicts(gs, coord.float().contiguous(), feat.float().contiguous(), max_fragments)
    finally:
        ops.unbind_stream()
    return _vote(model, gs["n"], num_classes, idxs, dicts, coord.device, noise_level, lanes)


@torch.no_grad()
def prepare_test_fragments(coord, color, normal, grid_size, augs=SCANNET_TTA, max_fragments=None):
    """Steps 1-4 of the reference's test pipeline on the device: raw ``coord`` (N,3) f32 in metres, ``color`` (N,3) f32
    in 0..255, ``normal`` (N,3) f32 (or None: feat = colour only).  Returns (index lists, fragment dicts) over ALL
    augmentations in the reference's order (aug-major, fragment-minor), ready for model.inference / inference_many."""
    ops.bind_stream()
    try:
        coord0 = ops.center_shift(coord.float().contiguous(), apply_z=True)
        color0 = ops.div_add(color, 127.5, -1.0)
        idxs, dicts = [], []
        for aug in augs:
            c, nrm = apply_aug(coord0, normal, aug)
            feat = color0 if nrm is None else ops.collect_feat(color0, nrm)
            gs = grid_sample_test(c, grid_size)
            ii, dd = _fragment_dicts(gs, c, feat, max_fragments)
            idxs += ii
            dicts += dd
    finally:
        ops.unbind_stream()
    return idxs, dicts


@torch.no_grad()
def segment_scene_tta(model, coord, color, normal, grid_size, num_classes, augs=SCANNET_TTA, noise_level=None,
                      max_fragments=None, lanes=4):
    """The reference tester's per-scene work, raw scan -> labels (steps 1-5 with the config's 13 augmentations)."""
    idxs, dicts = prepare_test_fragments(coord, color, normal, grid_size, augs, max_fragments)
    return _vote(model, coord.shape[0], num_classes, idxs, dicts, coord.device, noise_level, lanes)


# ---------------------------------------------------------------------------------------------------------------------
# The test pipeline from the config: TestPipeline(cfg.data.test)
_POINT_KEYS = ("coord", "color", "normal", "strength", "segment")
_GRID_OPTIONS = dict(grid_size=0.05, hash_type="fnv", mode="train", keys=("coord", "color", "normal", "segment"),
                     return_inverse=False, return_grid_coord=False, return_min_coord=False, return_displacement=False,
                     project_displacement=False)
# type -> {option: default} (the reference classes' own defaults); an option outside this table is rejected
_TEST_OPTIONS = {
    "CenterShift": dict(apply_z=True),
    "NormalizeColor": dict(),
    "Copy": dict(keys_dict=None),
    "GridSample": _GRID_OPTIONS,
    "RandomRotateTargetAngle": dict(angle=(1 / 2, 1, 3 / 2), center=None, axis="z", always_apply=False, p=0.75),
    "RandomScale": dict(scale=None, anisotropic=False),
    "RandomFlip": dict(p=0.5),
    "ToTensor": dict(),
    "Collect": dict(keys=None, offset_keys_dict=None, feat_keys=None),
}
_ALLOWED = {"transform": ("CenterShift", "NormalizeColor", "Copy", "GridSample"),
            "aug_transform": ("RandomRotateTargetAngle", "RandomScale", "RandomFlip"),
            "post_transform": ("CenterShift", "ToTensor", "Collect"), "test_cfg.voxelize": ("GridSample",)}


def _reject(msg):
    raise NotImplementedError("cdsegnet_amd.testtime: " + msg)


def _step(where, i, cfg):
    cfg = dict(cfg)
    typ = cfg.pop("type", None)
    if typ not in _ALLOWED[where.split("[")[0]]:
        _reject(f"{where} {i}: type {typ!r} is not supported")
    unknown = set(cfg) - set(_TEST_OPTIONS[typ])
    if unknown:
        _reject(f"{where} {i} ({typ}): option(s) {sorted(unknown)} are not supported")
    return typ, dict(_TEST_OPTIONS[typ], **cfg)


def _check_grid(where, o, mode):
    if o["mode"] != mode:
        _reject(f"{where}: GridSample(mode={o['mode']!r}), this position takes mode={mode!r}")
    for k in ("return_min_coord", "return_displacement", "project_displacement"):
        if o[k]:
            _reject(f"{where}: GridSample({k}=True)")
    if o["hash_type"] not in ("fnv", "ravel"):
        _reject(f"{where}: GridSample(hash_type={o['hash_type']!r})")
    if "coord" not in o["keys"] or not set(o["keys"]) <= set(_POINT_KEYS):
        _reject(f"{where}: GridSample(keys={o['keys']!r})")
    if not float(o["grid_size"]) > 0:
        _reject(f"{where}: GridSample grid_size must be positive")


def parse_test(cfg_data_test):
    """Validate the reference's ``data.test`` dict -> dict(transform, augs, voxelize, shift, feat_keys).  Raises
    NotImplementedError, naming the item, for everything the device pipeline does not implement."""
    cfg = dict(cfg_data_test)
    tc = cfg.get("test_cfg")
    if tc is None:
        _reject("the test block has no test_cfg")
    tc = dict(tc)
    transform = []
    for i, c in enumerate(cfg.get("transform") or []):
        typ, o = _step("transform", i, c)
        if typ == "Copy":
            o["keys_dict"] = dict(o["keys_dict"] or dict(coord="origin_coord", segment="origin_segment"))
            bad = [k for k in o["keys_dict"] if k not in _POINT_KEYS]
            if bad:
                _reject(f"transform {i}: Copy of {bad}: only the point keys {_POINT_KEYS}")
        elif typ == "GridSample":
            _check_grid(f"transform {i}", o, "train")
            if not o["return_inverse"]:
                _reject(f"transform {i}: GridSample(return_inverse=False): the votes could not be mapped back to the scan")
        transform.append((typ, o))
    types = [t for t, _ in transform]
    if types.count("GridSample") > 1:
        _reject("transform: more than one GridSample")
    if "GridSample" in types and "Copy" in types[types.index("GridSample"):]:
        _reject("transform: Copy after GridSample")
    # -- aug_transform: every list is deterministic, and its steps run in order under numpy's promotions
    if not tc.get("aug_transform"):
        _reject("test_cfg.aug_transform is empty (the reference runs one pass per list)")
    augs = []
    for a, lst in enumerate(tc["aug_transform"]):
        steps, f64 = [], False
        for i, c in enumerate(lst):
            where = f"aug_transform[{a}]"
            typ, o = _step(where, i, c)
            if typ == "RandomRotateTargetAngle":
                p = 1 if o["always_apply"] else o["p"]
                if p != 1:
                    _reject(f"{where} {i}: RandomRotateTargetAngle(p={o['p']}) is not deterministic: p != 1")
                if len(o["angle"]) != 1:
                    _reject(f"{where} {i}: RandomRotateTargetAngle(angle={list(o['angle'])}): more than one target angle")
                if o["center"] is None:
                    _reject(f"{where} {i}: RandomRotateTargetAngle(center=None) (the bounding-box centre)")
                if [float(v) for v in o["center"]] != [0.0, 0.0, 0.0]:
                    _reject(f"{where} {i}: RandomRotateTargetAngle(center={list(o['center'])}): only [0, 0, 0]")
                if o["axis"] != "z":
                    _reject(f"{where} {i}: RandomRotateTargetAngle(axis={o['axis']!r}): only 'z'")
                if f64:
                    _reject(f"{where} {i}: a second RandomRotateTargetAngle in one list")
                f64 = True
                steps.append(("rotate", float(o["angle"][0])))
            elif typ == "RandomScale":
                if o["anisotropic"]:
                    _reject(f"{where} {i}: RandomScale(anisotropic=True)")
                lo, hi = o["scale"] if o["scale"] is not None else (0.95, 1.05)
                if lo != hi:
                    _reject(f"{where} {i}: RandomScale(scale=[{lo}, {hi}]) is not deterministic: a scale range with lo != hi")
                steps.append(("scale", float(lo)))
            else:
                if o["p"] != 1:
                    _reject(f"{where} {i}: RandomFlip(p={o['p']}) is not deterministic: p != 1")
                steps.append(("flip", None))
        augs.append(steps)
    # -- voxelize / crop
    if tc.get("crop") is not None:
        _reject("test_cfg.crop: only None")
    if tc.get("voxelize") is None:
        _reject("test_cfg.voxelize=None")
    _, vox = _step("test_cfg.voxelize", 0, tc["voxelize"])
    _check_grid("test_cfg.voxelize", vox, "test")
    if not vox["return_grid_coord"]:
        _reject("test_cfg.voxelize: GridSample(return_grid_coord=False): the model needs grid_coord")
    if vox["return_inverse"]:
        _reject("test_cfg.voxelize: GridSample(return_inverse=True)")
    # -- post_transform
    shift, feat_keys = False, None
    post = list(tc.get("post_transform") or [])
    for i, c in enumerate(post):
        typ, o = _step("post_transform", i, c)
        if typ == "CenterShift":
            if o["apply_z"]:
                _reject(f"post_transform {i}: CenterShift(apply_z=True)")
            if shift or feat_keys is not None:
                _reject(f"post_transform {i}: CenterShift must come once, before Collect")
            shift = True
        elif typ == "Collect":
            if o["offset_keys_dict"] is not None:
                _reject("post_transform: Collect(offset_keys_dict=...)")
            if o["keys"] is None or tuple(o["keys"]) != ("coord", "grid_coord", "index"):
                _reject(f"post_transform: Collect(keys={o['keys']!r}): only (coord, grid_coord, index)")
            if not o["feat_keys"] or not set(o["feat_keys"]) <= {"coord", "color", "normal", "strength"}:
                _reject(f"post_transform: Collect(feat_keys={o['feat_keys']!r})")
            if i != len(post) - 1:
                _reject("post_transform: Collect must be the last transform")
            feat_keys = tuple(o["feat_keys"])
    if feat_keys is None:
        _reject("post_transform must end with Collect")
    if shift and "coord" in feat_keys:
        _reject("post_transform: CenterShift together with 'coord' in Collect(feat_keys=...)")
    return dict(transform=transform, augs=augs, voxelize=vox, shift=shift, feat_keys=feat_keys)


def _check_inference_mode(inference_mode, step, reuse_encoder):
    """The tester's cfg.inference_mode / cfg.step (ref: engines/test.py:212-258), checked before any device work."""
    if inference_mode not in ("SSI", "MSAI", "MSFI"):
        raise ValueError(f"inference_mode={inference_mode!r}: 'SSI', 'MSAI' or 'MSFI'")
    if isinstance(step, bool) or int(step) != step or step < 1:
        raise ValueError(f"step={step!r}: an integer, at least 1")
    if reuse_encoder and inference_mode == "SSI":
        raise ValueError("reuse_encoder=True needs inference_mode 'MSAI' or 'MSFI' (SSI runs the n-encoder once anyway)")


class TestScene:
    """What ``TestPipeline.prepare`` returns for one scan.

    augs        one dict per aug_transform list with the DENSE fragments of that augmented scan: index (F,m) int32 (rows
                of the transformed scan), coord (F,m,3) float32, grid_coord (F,m,3) int32, feat (F,m,C) float32,
                num_voxels m, num_fragments F, offset (1,) int64 on the device, shared_geometry True: GridSample(mode=
                "test") picks member i % count of every voxel in voxel-key order (transform.py:867-895), so all F fragments
                hold one point per voxel over the same voxels in the same row order - grid_coord is F copies of one grid
    fragments   the flat list of per-fragment dicts in the reference's order (aug-major, fragment-minor): zero-copy views
                of the arrays above (coord, grid_coord, feat, index) with offset / offset_host, ready for model.inference
    n           rows of the transformed scan = rows the votes cover;  n_raw: rows of the raw scan
    segment     labels of the transformed scan's rows (or None)
    inverse     (n_raw,) int32, the transformed-scan row of every raw point's voxel, and origin_segment (n_raw,) - when the
                transform list holds GridSample(return_inverse=True) / Copy(segment -> origin_segment); else None
    copies      every key a Copy produced (origin_segment among them)
    """
    __test__ = False  # (not a pytest class)

    def __init__(self):
        self.augs, self.fragments, self.copies = [], [], {}
        self.n = self.n_raw = 0
        self.segment = self.inverse = self.origin_segment = None
        self.trace = {}

    def collated(self, a, f0, k):
        """Fragments f0 .. f0+k-1 of augmentation a as ONE batch of k scenes: views, nothing is copied.  The dict carries the
        augmentation's ``shared_geometry`` mark: every element of the batch has the same grid."""
        g = self.augs[a]
        m, k = g["num_voxels"], min(k, g["num_fragments"] - f0)
        if k == 1:
            return self.fragments[g["first"] + f0]
        sl = slice(f0, f0 + k)
        ends = [m * (j + 1) for j in range(k)]
        return dict(coord=g["coord"][sl].reshape(k * m, 3), grid_coord=g["grid_coord"][sl].reshape(k * m, 3),
                    feat=g["feat"][sl].reshape(k * m, -1), index=g["index"][sl],
                    offset=torch.arange(m, k * m + 1, m, dtype=torch.int64, device=g["coord"].device), offset_host=ends,
                    shared_geometry=bool(g.get("shared_geometry")))


class TestPipeline:
    """The reference's test-time data pipeline, built from its own ``data.test`` dict (configs/*/CDSegNet.py; ref:
    pointcept/datasets/defaults.py:98-132 prepare_test_data, datasets/transform.py, engines/test.py:197-279):

        tp = TestPipeline(cfg.data.test)
        labels, pred = tp.segment(model, raw, num_classes)           # raw: dict of device tensors
        counts = tp.evaluate(labels, tp.prepare(raw), num_classes, ignore_index)

    Supported (everything the three shipped CDSegNet configs use; anything else raises NotImplementedError at construction):
      transform        CenterShift, NormalizeColor, Copy(keys_dict) of point keys, GridSample(mode="train",
                       return_inverse=True) with hash_type fnv / ravel (voxels are keyed by the packed integer coordinate;
                       any injective key forms the same voxels).  Every point key the scan has is sub-sampled.
      aug_transform    lists of RandomRotateTargetAngle(angle=[a], center=[0,0,0], axis="z", p=1), RandomScale(scale=[s, s]),
                       RandomFlip(p=1), applied in order under numpy's promotions: a rotation makes the cloud float64 (and
                       rotates the normals), a scale of a float32 cloud is float32(float64(x) * s), a flip negates x and y
      test_cfg         voxelize = GridSample(mode="test", return_grid_coord=True); crop = None; post_transform = optional
                       CenterShift(apply_z=False), ToTensor, Collect(keys=(coord, grid_coord, index), feat_keys of coord,
                       color, normal, strength)
    A post-transform CenterShift together with "coord" in feat_keys is REJECTED (the feature would be the per-fragment
    shifted coordinate; no shipped config asks for it).

    The random member pick of the train-mode GridSample comes from the library's Philox keyed by (seed, scene_index), as
    in TrainTransform; ``draws={"<i>.r": r}`` (i = the GridSample's position in ``transform``) injects it: voxel v in key
    order keeps its member r[v % len(r)] % count_v, members in row order.
    Per augmentation ``prepare`` makes a fixed number of library calls, whatever the number of fragments."""
    __test__ = False

    def __init__(self, cfg_data_test, seed=0):
        self.plan = parse_test(cfg_data_test)
        self.seed = int(seed)

    # ------------------------------------------------------------------------------------------------ prepare
    def _grid_sample_train(self, st, scene, i, o, scene_index, draws):
        dev = st["coord"].device
        grid, key, _ = ops.voxelize_any(st["coord"], o["grid_size"])
        key_sorted, idx_sort = ops.sort_pairs(key, None, end_bit=63)
        cluster, seg_start, count = ops.pool_level(key_sorted, 0)
        m = int(count.item())  # host read: the size of everything downstream
        if draws is not None:
            r = _dev(_field(draws, i, "r"), torch.int64, dev).reshape(-1)
            if r.numel() != m:
                r = r[torch.arange(m, device=dev) % r.numel()].contiguous()
        else:
            r = ops.rand_int(m, philox_key(self.seed, scene_index), 16 * i, dev, bound_dev=ops.max_run(seg_start, m))
        pick = ops.tt_voxel_pick(idx_sort, seg_start, m, r)
        scene.inverse = ops.voxel_inverse(idx_sort, cluster)
        scene.trace.update(pick=pick, grid=grid, r=r)
        for k in _POINT_KEYS:
            if st.get(k) is not None:
                st[k] = ops.gather_rows(st[k].reshape(st[k].shape[0], -1), pick).reshape((m,) + tuple(st[k].shape[1:]))

    def _augment(self, steps, coord, normal):
        i = 0
        while i < len(steps):
            kind, v = steps[i]
            if kind == "rotate":
                scale = steps[i + 1][1] if i + 1 < len(steps) and steps[i + 1][0] == "scale" else None
                rot = _rot_z(v)
                coord = ops.tta_apply(coord, rot=rot, scale=scale)  # float32 -> float64 (parse allows one rotation)
                normal = None if normal is None else ops.tta_apply(normal, rot=rot)
                i += 1 if scale is None else 2
                continue
            if kind == "scale":
                coord = ops.tt_affine(coord, scale=v, out_dtype=coord.dtype)
            else:
                coord = ops.tt_affine(coord, flipx=True, flipy=True, out_dtype=coord.dtype)
                normal = None if normal is None else ops.tt_affine(normal, flipx=True, flipy=True, out_dtype=normal.dtype)
            i += 1
        return coord, normal

    def _collect(self, st, coord, normal):
        parts = []
        for k in self.plan["feat_keys"]:
            p = coord if k == "coord" else (normal if k == "normal" else st.get(k))
            if p is None:
                raise KeyError(f"Collect(feat_keys=...): the scan has no {k!r}")
            parts.append(p)
        feat = parts[0] if parts[0].dtype == torch.float32 else ops.tt_affine(parts[0], out_dtype=torch.float32)
        for p in parts[1:]:
            feat = ops.collect_feat(feat, p if p.dtype == torch.float64 else p.float())
        return feat.contiguous()

    @torch.no_grad()
    def prepare(self, raw, scene_index=0, draws=None, max_fragments=None):
        """raw: dict of device tensors - coord (N,3) float32, color (N,3) in 0..255 and normal (N,3), or strength (N,1),
        optional segment (N,) -> TestScene."""
        coord = raw["coord"]
        if not isinstance(coord, torch.Tensor):
            raise ValueError("raw['coord'] must be a device tensor")
        ops._need_gpu(coord)
        if coord.dim() != 2 or coord.shape[1] != 3 or coord.shape[0] == 0:
            raise ValueError("raw['coord'] must be a non-empty (N, 3) tensor")
        n_raw, dev = coord.shape[0], coord.device
        scene = TestScene()
        scene.n_raw = n_raw
        st = dict(coord=coord.float().contiguous())
        for k in ("color", "normal", "strength"):
            st[k] = raw[k].float().reshape(n_raw, -1).contiguous() if raw.get(k) is not None else None
        st["segment"] = raw["segment"].reshape(n_raw).contiguous() if raw.get("segment") is not None else None
        ops.bind_stream()
        try:
            for i, (typ, o) in enumerate(self.plan["transform"]):
                if typ == "CenterShift":
                    st["coord"] = ops.center_shift(st["coord"], apply_z=o["apply_z"])
                elif typ == "NormalizeColor":
                    if st["color"] is not None:
                        st["color"] = ops.div_add(st["color"], 127.5, -1.0)
                elif typ == "Copy":
                    for src, dst in o["keys_dict"].items():
                        if st.get(src) is None:
                            raise KeyError(f"Copy: the scan has no {src!r}")
                        scene.copies[dst] = st[src]  # (no later step writes in place: the alias is the copy)
                else:
                    self._grid_sample_train(st, scene, i, o, scene_index, draws)
            scene.n = st["coord"].shape[0]
            scene.segment = st["segment"]
            scene.origin_segment = scene.copies.get("origin_segment")
            scene.trace["coord"] = st["coord"]
            vox = self.plan["voxelize"]
            for steps in self.plan["augs"]:
                c, nrm = self._augment(steps, st["coord"], st["normal"])
                feat = self._collect(st, c, nrm)
                gs = grid_sample_test(c, vox["grid_size"])
                m = gs["num_voxels"]
                nfrag = gs["num_fragments"] if max_fragments is None else min(gs["num_fragments"], max_fragments)
                index, fc, fg, ff = ops.fragments_build(gs["idx_sort"], gs["seg_start"], m, nfrag, gs["grid_coord"], feat, c,
                                                        center_shift=self.plan["shift"])
                off = torch.full((1,), m, dtype=torch.int64, device=dev)  # a device fill, no host-to-device copy
                scene.augs.append(dict(index=index, coord=fc, grid_coord=fg, feat=ff, num_voxels=m, num_fragments=nfrag,
                                       offset=off, first=len(scene.fragments), aug_coord=c, shared_geometry=True))
                scene.fragments += [dict(coord=fc[f], grid_coord=fg[f], feat=ff[f], index=index[f], offset=off, offset_host=[m],
                                         shared_geometry=True) for f in range(nfrag)]
        finally:
            ops.unbind_stream()
        return scene

    # ------------------------------------------------------------------------------------------------ model + vote
    @torch.no_grad()
    def vote(self, model, scene, num_classes, noise_level=None, lanes=4, fragment_batch=1, share_plan=False,
             fragment_draws="batch", inference_mode="SSI", step=1, reuse_encoder=False):
        """model.inference on every fragment (``fragment_batch`` consecutive fragments of one augmentation per forward),
        pred[index] += softmax(logits) in the reference's order, arg-max, and ``[inverse]`` when the scene has one.

        share_plan      True: the fragments of an augmentation share their geometry (``prepare`` marks them; no grid is
                        compared here), so the model's plan is built once per (augmentation, group size) - at most two per
                        augmentation, one at fragment_batch=1 - before the forwards are issued, and handed to
                        ``inference_many(plans=...)``: no forward builds a plan or reads from the device.  Same votes, bit
                        for bit.
        fragment_draws  "batch" (default): a collated forward takes ONE set of random draws, the reference's own batching |
                        "fragment" (needs share_plan=True): every fragment of a collated forward takes its own draws - noise
                        rows and order shuffles - in fragment order, as fragment_batch=1 does: k fragments then compute what
                        k forwards of the reference's protocol compute, at the launch count of one forward.
        inference_mode  the tester's cfg.inference_mode (ref: engines/test.py:212-258): "SSI" (default) one backbone call per
                        forward | "MSAI" / "MSFI": every fragment (or collated group) runs ``step`` DDIM steps through
                        ``inference_ddim_many(mode="avg" / "final")``; plans, batches and per-fragment draws as for SSI
                        (a plan serves all step + 1 backbone calls).  ``reuse_encoder``: see ``model.inference_ddim``."""
        _check_inference_mode(inference_mode, step, reuse_encoder)
        multi = inference_mode != "SSI"
        if multi and not hasattr(model, "inference_ddim_many"):
            raise ValueError(f"inference_mode={inference_mode!r} needs a model with inference_ddim_many()")
        if fragment_draws not in ("batch", "fragment"):
            raise ValueError(f"fragment_draws={fragment_draws!r}: 'batch' or 'fragment'")
        if fragment_draws == "fragment" and not share_plan:
            raise ValueError("fragment_draws='fragment' needs share_plan=True")
        if share_plan and not (hasattr(model, "plan") and hasattr(model, "inference_many")):
            raise ValueError("share_plan=True needs a model with plan() and inference_many()")
        k = max(1, int(fragment_batch))
        groups = [(a, f0) for a, g in enumerate(scene.augs) for f0 in range(0, g["num_fragments"], k)]
        dicts = [scene.collated(a, f0, k) for a, f0 in groups]

        def forwards(draws=None, plans=None):
            if multi:
                return model.inference_ddim_many(dicts, step=int(step), mode="avg" if inference_mode == "MSAI" else "final",
                                                 lanes=lanes, noise_level=noise_level, draws=draws, plans=plans,
                                                 reuse_encoder=reuse_encoder)
            if draws is None and plans is None:
                return model.inference_many(dicts, lanes=lanes, noise_level=noise_level)
            return model.inference_many(dicts, lanes=lanes, noise_level=noise_level, draws=draws, plans=plans)

        if share_plan:
            built = {}
            for (a, f0), d in zip(groups, dicts):
                if not scene.augs[a].get("shared_geometry"):
                    raise ValueError(f"share_plan=True: augmentation {a} is not marked as sharing geometry")
                key = (a, len(d["offset_host"]))
                if key not in built:
                    built[key] = model.plan(d)
            plans = [built[(a, len(d["offset_host"]))] for (a, _), d in zip(groups, dicts)]
            draws = None
            if fragment_draws == "fragment":  # in fragment order, from this one thread, before anything is issued
                eng = model.engine()
                if multi:
                    draws = [eng.predraw_fragments(d, noise_level, int(step) + 1, always_noise=True) for d in dicts]
                else:
                    draws = [eng.predraw_fragments(d, noise_level) for d in dicts]
            outs = forwards(draws, plans)
            del plans, built  # (the lanes have been joined: nothing reads the plans any more)
        elif multi or hasattr(model, "inference_many"):
            outs = forwards()
        else:
            outs = [model.inference(d, eval=False, noise_level=noise_level) for d in dicts]
        dev = scene.augs[0]["coord"].device
        ops.bind_stream()
        try:
            pred = torch.zeros((scene.n, num_classes), dtype=torch.float32, device=dev)
            for d, o in zip(dicts, outs):
                idx = d["index"] if d["index"].dim() == 2 else d["index"].reshape(1, -1)
                ops.softmax_vote_fragments(o["seg_logits"].float(), idx, pred)
            labels = ops.argmax_rows(pred)
            if scene.inverse is not None:
                labels = ops.gather_i32(labels, scene.inverse)
        finally:
            ops.unbind_stream()
        return labels, pred

    @torch.no_grad()
    def segment(self, model, raw, num_classes, scene_index=0, noise_level=None, lanes=4, fragment_batch=1, max_fragments=None,
                draws=None, share_plan=False, fragment_draws="batch", inference_mode="SSI", step=1, reuse_encoder=False):
        """Raw scan -> (labels int32, pred float32 (scene.n, num_classes) summed softmax votes).  The labels are for the
        ORIGINAL points when the transform list produced ``inverse`` (pred[inverse], engines/test.py:269-272), else for
        the transformed scan's points.  fragment_batch=1 is the reference's protocol, one fragment per forward;
        fragment_batch=k collates k consecutive fragments of one augmentation (views, no copy).  The fragments of an
        augmentation share their geometry, so the serialization depth of the batch is the single forward's; what is per
        batch by default is the random draws (the reference's own batching, ``inference_many(batch=...)``).  With
        share_plan=True and fragment_draws="fragment" every fragment takes its own draws and the batch computes what k
        single forwards compute (see ``vote``).  inference_mode / step / reuse_encoder: multi-step voting, see ``vote``."""
        _check_inference_mode(inference_mode, step, reuse_encoder)  # (before any device work)
        scene = self.prepare(raw, scene_index, draws, max_fragments)
        return self.vote(model, scene, num_classes, noise_level, lanes, fragment_batch, share_plan, fragment_draws,
                         inference_mode, step, reuse_encoder)

    @torch.no_grad()
    def evaluate(self, labels_or_votes, scene, num_classes, ignore_index=-1, reduce=True):
        """(3, K) int64 [intersection, union, target] of one scene against ``origin_segment`` (when the scene has
        ``inverse``) or ``segment``; summed over ranks like evaluate.evaluate_scene.  labels_or_votes: the summed votes
        (scene.n, K) - arg-max here, mapped through ``inverse`` by the counting kernel (ops.iou_counts(pred_idx=inverse)) -
        or the 1-D labels ``segment`` returned (already those of the target's points)."""
        x = labels_or_votes
        target = scene.origin_segment if scene.inverse is not None else scene.segment
        if target is None:
            raise KeyError("evaluate: the scene has no segment" + (" to Copy to origin_segment" if scene.inverse is not None else ""))
        target = target.to(torch.int32).contiguous()
        ops.bind_stream()
        try:
            if x.dim() == 2:
                rows, pred_idx = ops.argmax_rows(x.float().contiguous()), scene.inverse
            else:
                rows, pred_idx = x.to(torch.int32).contiguous(), None
            if rows.numel() != (scene.n if pred_idx is not None or scene.inverse is None else target.numel()):
                raise ValueError(f"evaluate: {rows.numel()} labels for {target.numel()} targets")
            raw = ops.iou_counts(rows, target, num_classes, ignore_index, pred_idx=pred_idx)
        finally:
            ops.unbind_stream()
        counts = torch.stack([raw[0], raw[1] + raw[2] - raw[0], raw[2]])
        return cdist.reduce_counts(counts) if reduce else counts
