"""Train-time pipeline, host side: the numpy restatement of the device pipeline (tests/traintime_restatement.py) against
fixtures recorded from the reference's own transform classes (tools/make_traintime_golden.py -> tests/golden/traintime_*),
the Mix3D offsets against the reference's point_collate_fn, the constructor's rejections and the host draws.

Bounds (none taken from the code under test): the reference chain has at most 8 float32 roundings per coordinate, so the
pre-GridSample coordinates agree within 8 float32 ulps of the scene's largest |coordinate|; colours within 8 float32 ulps
of 255; normals within 4 float32 ulps of 1.  grid_coord is equal on every row except rows whose reference coordinate lies
within the measured coordinate error of a voxel face; those are at most 0.1 % of the rows.
"""
import json

import numpy as np
import pytest
import torch

import traintime_restatement as R
from cdsegnet_amd import traintime as tt
from helpers import load_fixture

TAGS = ("A", "B", "C", "D", "E")
_CACHE = {}


def load_case(tag):
    """(cfg, raw, draws, ref, restatement output, restatement trace) - computed once, shared, never modified."""
    if tag not in _CACHE:
        raw_f, draws_f, ref_f = (load_fixture(f"traintime_{tag}_{part}.npz") for part in ("raw", "draws", "ref"))
        cfg = json.loads(str(raw_f["cfg_json"]))
        raw = {k: raw_f[k] for k in ("coord", "color", "normal", "strength", "segment") if k in raw_f.files}
        draws = {k: raw_f[k] for k in raw_f.files if k[0].isdigit()}
        draws.update({k: draws_f[k] for k in draws_f.files})
        ref = {k: ref_f[k] for k in ref_f.files}
        trace = {}
        out = R.run(cfg, raw, draws, trace)
        _CACHE[tag] = (cfg, raw, draws, ref, out, trace)
    return _CACHE[tag]


def _grid_size(cfg):
    return [c for c in cfg if c["type"] == "GridSample"][0]["grid_size"]


def test_fixtures_cover_the_branches_they_are_meant_to():
    kinds = {t: load_case(t) for t in TAGS}
    rot = lambda cfg, d: [f"{i}.angle" in d for i, c in enumerate(cfg) if c["type"] == "RandomRotate"]  # noqa: E731
    ela = lambda cfg: [i for i, c in enumerate(cfg) if c["type"] == "ElasticDistortion"][0]  # noqa: E731
    cfg, raw, d, ref, out, tr = kinds["A"]
    assert all(rot(cfg, d)) and ref["pre_coord"].dtype == np.float64 and len(raw["coord"]) == 12000
    cfg, raw, d, ref, out, tr = kinds["B"]
    assert not any(rot(cfg, d)) and ref["pre_coord"].dtype == np.float32 and len(ref["pre_coord"]) == int(12000 * 0.8)
    cfg, raw, d, ref, out, tr = kinds["C"]
    assert np.mean(tr["gridsample"]["count"] >= 2) > 0.5 and int(ref["crop_applied"]) == 1 and len(out["coord"]) == 2048
    cfg, raw, d, ref, out, tr = kinds["D"]
    assert f"{ela(cfg)}.noise0" not in d and float(d[f"{ela(cfg)}.coin"]) >= 0.95
    assert tr["gridsample"]["count"].max() == 1 and int(ref["crop_applied"]) == 0 and len(out["coord"]) == 12000
    cfg, raw, d, ref, out, tr = kinds["E"]
    assert "strength" in raw and out["feat"].shape[1] == 4


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_matches_the_reference_before_gridsample(tag):
    cfg, raw, draws, ref, out, tr = load_case(tag)
    assert np.array_equal(tr["pre_index"], ref["pre_index"])
    big = np.float32(np.abs(ref["pre_coord"]).max())
    err = float(np.abs(tr["pre_coord"] - ref["pre_coord"].astype(np.float64)).max())
    ulps = err / float(np.spacing(big))
    msg = f"[measure] traintime {tag}: pre-GridSample coord max |diff| {err:.3e} m = {ulps:.2f} float32 ulps of {float(big):.3f}"
    assert ulps <= 8.0, msg
    if "pre_color" in ref:
        e = float(np.abs(tr["pre_color"].astype(np.float64) - ref["pre_color"].astype(np.float64)).max()) / float(np.spacing(np.float32(255)))
        msg += f"; colour {e:.2f} ulps of 255"
        assert e <= 8.0, msg
    if "pre_normal" in ref:
        e = float(np.abs(tr["pre_normal"] - ref["pre_normal"].astype(np.float64)).max()) / float(np.spacing(np.float32(1)))
        msg += f"; normal {e:.2f} ulps of 1"
        assert e <= 4.0, msg
    print(msg)


@pytest.mark.parametrize("tag", TAGS)
def test_gridsample_voxels_counts_and_picks_match_the_reference(tag):
    cfg, raw, draws, ref, out, tr = load_case(tag)
    gsize = _grid_size(cfg)
    gs = tr["gridsample"]
    err = float(np.abs(tr["pre_coord"] - ref["pre_coord"].astype(np.float64)).max())
    differ = np.any(gs["grid"] != ref["pre_grid"], axis=1)
    scaled = ref["pre_coord"].astype(np.float64) / gsize
    face = (np.abs(scaled - np.round(scaled)) * gsize).min(1)  # distance of the reference coordinate to the nearest voxel face
    print(f"[measure] traintime {tag}: {int(differ.sum())} of {len(differ)} rows in another voxel than the reference "
          f"(coordinate error {err:.3e} m)")
    assert np.all(face[differ] <= err), "a row away from every voxel face landed in another voxel"
    assert differ.mean() <= 0.001
    keep = ~differ
    # voxel sets and per-voxel counts over the compared rows
    va, ca = np.unique(gs["grid"][keep], axis=0, return_counts=True)
    vb, cb = np.unique(ref["pre_grid"][keep], axis=0, return_counts=True)
    assert np.array_equal(va, vb) and np.array_equal(ca, cb)
    if not differ.any():
        assert len(gs["count"]) == len(ref["grid_sel"]) and np.array_equal(np.sort(gs["count"]), np.sort(ca))
        # the reference picked one row of every voxel
        assert np.array_equal(np.unique(ref["pre_grid"][ref["grid_sel"]], axis=0), vb)
        assert np.array_equal(ref["pre_grid"][ref["grid_sel"]], ref["grid_coord"])
    # every picked row is a member of its voxel; voxels are in key order, one pick each
    picked = gs["grid"][gs["pick"]].astype(np.int64)
    key = (picked[:, 0] << 42) | (picked[:, 1] << 21) | picked[:, 2]
    assert np.all(np.diff(key) > 0) and len(key) == len(gs["count"])
    for v in (0, len(key) // 2, len(key) - 1):
        members = gs["idx_sort"][gs["seg_start"][v]:gs["seg_start"][v + 1]]
        assert gs["pick"][v] in members and np.all(np.diff(members) > 0)  # stable: members in row order


@pytest.mark.parametrize("tag", ("A", "C", "D"))
def test_sphere_crop_membership_from_the_recorded_stage_input(tag):
    cfg, raw, draws, ref, out, tr = load_case(tag)
    i, c = [(i, c) for i, c in enumerate(cfg) if c["type"] == "SphereCrop"][0]
    crop_in = ref["pre_coord"][ref["grid_sel"]]
    if not int(ref["crop_applied"]):
        assert len(crop_in) <= c["point_max"] and np.array_equal(ref["crop_sel"], np.arange(len(crop_in)))
        assert len(out["coord"]) == len(tr["gridsample"]["count"])  # identity in the restatement too
        return
    center = int(draws[f"{i}.center"])
    sel, d2 = R.sphere_crop(crop_in, center, c["point_max"])
    cut = np.sort(d2)[c["point_max"] - 1]
    a, b = set(sel.tolist()), set(ref["crop_sel"].tolist())
    assert len(a) == len(b) == c["point_max"]
    assert all(d2[r] == cut for r in a ^ b), "the crops differ on rows that are not tied at the cut-off distance"
    assert center in a and np.all(d2[sel] <= cut)


def test_restatement_blur_equals_scipy_and_axes_equal_linspace():
    scipy_ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    noise = rng.standard_normal((7, 5, 4, 3)).astype(np.float32)
    want = noise
    for _ in range(2):
        for shape in ((3, 1, 1, 1), (1, 3, 1, 1), (1, 1, 3, 1)):
            want = scipy_ndimage.convolve(want, np.ones(shape, dtype=np.float32) / 3, mode="constant", cval=0)
    got = R.blur(noise)
    assert np.abs(got - want).max() <= np.spacing(np.float32(np.abs(want).max()))
    dim, start, step, stop = tt.elastic_axes([1.0, -2.0, 0.25, 5.3, 1.1, 2.9], 0.2)
    assert list(dim) == [24, 18, 16]
    for a in range(3):
        ax = np.arange(dim[a]) * step[a] + start[a]
        ax[-1] = stop[a]
        assert np.array_equal(ax, np.linspace(start[a], stop[a], dim[a]))


def test_mix3d_offsets_equal_point_collate_fn():
    fx = load_fixture("traintime_mix3d.npz")
    mix_prob = float(fx["mix_prob"])

    class Coin:
        def __init__(self, v):
            self.v = v

        def random(self):
            return self.v

    merged = 0
    for c in range(int(fx["cases"])):
        sizes, coin, want = fx[f"{c}.sizes"], float(fx[f"{c}.coin"]), fx[f"{c}.offset"]
        assert tt.mix3d_offsets(sizes, coin < mix_prob) == want.tolist()
        dicts = [dict(coord=torch.zeros(int(k), 3), grid_coord=torch.zeros(int(k), 3, dtype=torch.int32), feat=torch.zeros(int(k), 6),
                      segment=torch.zeros(int(k), dtype=torch.int64), index=torch.arange(int(k), dtype=torch.int32),
                      offset=torch.tensor([int(k)]), offset_host=[int(k)]) for k in sizes]
        got = tt.collate(dicts, mix_prob=mix_prob, rng=Coin(coin))
        assert got["offset"].tolist() == want.tolist() == got["offset_host"] and got["coord"].shape[0] == int(sizes.sum())
        merged += len(want) < len(sizes)
    assert merged >= 4  # the fixture holds merged and unmerged batches


SCANNET_VAL = [dict(type="CenterShift", apply_z=True),
               dict(type="GridSample", grid_size=0.02, hash_type="fnv", mode="train", return_grid_coord=True),
               dict(type="CenterShift", apply_z=False), dict(type="NormalizeColor"), dict(type="ToTensor"),
               dict(type="Collect", keys=("coord", "grid_coord", "segment"), feat_keys=("color", "normal"))]


def _with(i, **kw):
    cfg = [dict(c) for c in SCANNET_VAL]
    cfg[i].update(kw)
    return cfg


@pytest.mark.parametrize("cfg", [
    [dict(type="RandomScale", scale=[0.9, 1.1], anisotropic=True)] + SCANNET_VAL,
    [dict(type="RandomShift")] + SCANNET_VAL,
    [dict(type="RandomRotateTargetAngle", angle=[0.5], axis="z")] + SCANNET_VAL,
    [dict(type="SphereCrop", point_max=100, mode="random")] + SCANNET_VAL,        # before GridSample
    SCANNET_VAL[:2] + [dict(type="SphereCrop", point_max=100, mode="center")] + SCANNET_VAL[2:],
    SCANNET_VAL[:2] + [dict(type="SphereCrop", point_max=100, mode="all")] + SCANNET_VAL[2:],
    SCANNET_VAL[:2] + [dict(type="SphereCrop", sample_rate=0.5, mode="random")] + SCANNET_VAL[2:],
    _with(1, return_inverse=True), _with(1, return_displacement=True), _with(1, mode="test"), _with(1, return_grid_coord=False),
    _with(0, apply_y=True),                                                       # an option the transform does not have
    _with(5, keys=("coord", "grid_coord", "segment", "inverse")),
    SCANNET_VAL[:-1],                                                             # no Collect
    [dict(type="RandomRotate", axis="w")] + SCANNET_VAL,
])
def test_unsupported_types_and_options_are_rejected_at_construction(cfg):
    with pytest.raises(NotImplementedError):
        tt.TrainTransform(cfg)


def test_the_shipped_lists_are_accepted():
    for tag in ("A", "E"):
        cfg = load_case(tag)[0]
        assert len(tt.TrainTransform(cfg, seed=3).steps) == len(cfg)
    assert [t for t, _ in tt.TrainTransform(SCANNET_VAL).steps][1] == "GridSample"


def test_host_draws_are_a_function_of_seed_and_scene_index():
    def seq(seed, scene):
        h = tt.HostDraws(None, seed, scene)
        return [h.scalar(1, "coin"), h.scalar(2, "angle", -1, 1), *h.vec3(3, "rand"), h.index(4, "center", 1000)]
    assert seq(5, 11) == seq(5, 11)
    assert seq(5, 11) != seq(5, 12) and seq(5, 11) != seq(6, 11)
    assert tt.philox_key(5, 11) == tt.philox_key(5, 11) and len({tt.philox_key(s, i) for s in range(4) for i in range(4)}) == 16
    s = seq(0, 0)
    assert 0 <= s[0] < 1 and -1 <= s[1] < 1 and 0 <= s[-1] < 1000
    # a record replaces the generator entirely, and a missing field is an error, not a silent draw
    h = tt.HostDraws({"1.coin": np.array(0.25)}, 0, 0)
    assert h.scalar(1, "coin") == 0.25
    with pytest.raises(KeyError):
        h.scalar(2, "coin")
