"""CPU: the config-driven test pipeline (cdsegnet_amd.testtime.TestPipeline) - what it accepts and rejects, and the numpy
restatement of the device pipeline (tests/testtime_restatement.py) against the fixture recorded from the reference's own
transform classes on the nuScenes test block (tests/golden/testtime_nuscenes.npz, tools/make_testtime_golden.py)."""
import copy
import json
import os

import numpy as np
import pytest

from cdsegnet_amd import testtime as tt
from tests import testtime_restatement as R
from tests.helpers import GOLDEN, load_fixture


def blocks():
    with open(os.path.join(GOLDEN, "test_blocks.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def fx():
    return load_fixture("testtime_nuscenes.npz")


@pytest.fixture(scope="module")
def restated(fx):
    raw = dict(coord=fx["coord"], strength=fx["strength"], segment=fx["segment"])
    return R.pipeline(blocks()["nuscenes"], raw, r=fx["1.r"])


def test_the_three_shipped_test_blocks_are_accepted():
    b = blocks()
    assert sorted(b) == ["nuscenes", "scannet", "scannet200"]
    plans = {k: tt.TestPipeline(v).plan for k, v in b.items()}
    for k in ("scannet", "scannet200"):
        p = plans[k]
        assert [t for t, _ in p["transform"]] == ["CenterShift", "NormalizeColor"] and p["shift"] and p["feat_keys"] == ("color", "normal")
        # the 13 lists are SCANNET_TTA
        want = [([("rotate", float(a))] if a is not None else []) + ([("scale", s)] if s is not None else []) + ([("flip", None)] if f else [])
                for a, s, f in tt.SCANNET_TTA]
        assert p["augs"] == want
    assert plans["scannet"]["augs"] == plans["scannet200"]["augs"]
    p = plans["nuscenes"]
    assert [t for t, _ in p["transform"]] == ["Copy", "GridSample"] and not p["shift"] and p["feat_keys"] == ("coord", "strength")
    assert p["transform"][1][1]["grid_size"] == 0.025 and p["voxelize"]["grid_size"] == 0.05
    scales = (0.9, 0.95, 1.0, 1.05, 1.1)
    assert p["augs"] == [[("scale", s)] for s in scales] + [[("scale", s), ("flip", None)] for s in scales]


def _edit(name, fn):
    cfg = copy.deepcopy(blocks()[name])
    fn(cfg)
    return cfg


REJECTED = [
    ("scale range", "nuscenes", lambda c: c["test_cfg"]["aug_transform"][0][0].update(scale=[0.9, 1.1]), "lo != hi"),
    ("flip p", "nuscenes", lambda c: c["test_cfg"]["aug_transform"][5][1].update(p=0.5), "p != 1"),
    ("rotate p", "scannet", lambda c: c["test_cfg"]["aug_transform"][1][0].update(p=0.75), "p != 1"),
    ("two angles", "scannet", lambda c: c["test_cfg"]["aug_transform"][1][0].update(angle=[0.5, 1]), "more than one target angle"),
    ("center none", "scannet", lambda c: c["test_cfg"]["aug_transform"][1][0].update(center=None), "center=None"),
    ("crop", "scannet", lambda c: c["test_cfg"].update(crop=dict(type="SphereCrop", point_max=1000)), "test_cfg.crop"),
    ("unknown type", "scannet", lambda c: c["transform"].append(dict(type="RandomJitter")), "RandomJitter"),
    ("unknown option", "nuscenes", lambda c: c["transform"][1].update(colour=True), "colour"),
    ("anisotropic", "nuscenes", lambda c: c["test_cfg"]["aug_transform"][0][0].update(anisotropic=True), "anisotropic"),
    ("voxelize train", "nuscenes", lambda c: c["test_cfg"]["voxelize"].update(mode="train"), "mode='train'"),
    ("voxelize no grid", "nuscenes", lambda c: c["test_cfg"]["voxelize"].update(return_grid_coord=False), "return_grid_coord"),
    ("transform test mode", "nuscenes", lambda c: c["transform"][1].update(mode="test"), "mode='test'"),
    ("no inverse", "nuscenes", lambda c: c["transform"][1].update(return_inverse=False), "return_inverse"),
    ("displacement", "nuscenes", lambda c: c["transform"][1].update(return_displacement=True), "return_displacement"),
    ("collect keys", "scannet", lambda c: c["test_cfg"]["post_transform"][2].update(keys=("coord", "grid_coord")), "Collect(keys"),
    ("feat key", "scannet", lambda c: c["test_cfg"]["post_transform"][2].update(feat_keys=("color", "displacement")), "feat_keys"),
    ("shift + coord feature", "scannet", lambda c: c["test_cfg"]["post_transform"][2].update(feat_keys=("coord", "color")),
     "CenterShift together with 'coord'"),
    ("post shift z", "scannet", lambda c: c["test_cfg"]["post_transform"][0].update(apply_z=True), "apply_z=True"),
]


@pytest.mark.parametrize("what,name,fn,names", REJECTED, ids=[r[0] for r in REJECTED])
def test_unsupported_items_are_rejected_at_construction_by_name(what, name, fn, names):
    with pytest.raises(NotImplementedError) as e:
        tt.TestPipeline(_edit(name, fn))
    assert names in str(e.value), str(e.value)


def test_restated_transform_pass_equals_the_reference(fx, restated):
    """GridSample(0.025, mode="train", return_inverse=True) with the recorded pick: the kept rows, every row's voxel, and
    ``inverse`` up to the voxel numbering."""
    n_raw = len(fx["coord"])
    kept = fx["kept"].astype(np.int64)
    assert len(kept) <= 0.8 * n_raw  # the fixture exercises the pass
    assert np.array_equal(np.sort(restated["pick"]), np.sort(kept))
    assert np.array_equal(restated["grid"], fx["grid025_raw"])
    assert np.array_equal(restated["origin_segment"], fx["origin_segment"])
    # one kept row per voxel, and inverse names the kept row of every raw row's voxel - in both numberings
    grid = fx["grid025_raw"]
    for rows, inverse in ((kept, fx["inverse"].astype(np.int64)), (restated["pick"], restated["inverse"])):
        assert inverse.shape == (n_raw,) and inverse.min() == 0 and inverse.max() == len(rows) - 1
        assert len(np.unique(grid[rows], axis=0)) == len(rows)
        assert np.array_equal(grid[rows][inverse], grid)
    # the same map from raw row to kept raw row
    assert np.array_equal(restated["pick"][restated["inverse"]], kept[fx["inverse"].astype(np.int64)])
    assert np.array_equal(restated["segment"], fx["segment"][restated["pick"]])


def test_restated_augmentations_and_fragments_equal_the_reference(fx, restated):
    """Per augmentation, compared in raw-row space (the reference orders the kept rows by its FNV hash, the restatement by
    the packed key): augmented coordinates with their dtype, every row's voxel, features scattered back by index, fragment
    sizes, and fragment membership as sets per voxel."""
    kept = fx["kept"].astype(np.int64)
    o_ref, o_me = np.argsort(kept), np.argsort(restated["pick"])
    assert int(fx["num_aug"]) == len(restated["augs"]) == 10
    seen, most = set(), 0
    for a, g in enumerate(restated["augs"]):
        want = fx[f"aug{a}_coord"]
        assert g["coord"].dtype == want.dtype == np.float32
        assert np.array_equal(g["coord"][o_me], want[o_ref]), a
        assert np.array_equal(g["grid"][o_me], fx[f"aug{a}_grid"][o_ref]), a
        nfrag, m = g["index"].shape
        assert [m] * nfrag == fx[f"aug{a}_frag_sizes"].tolist(), a
        feat = np.zeros((restated["n"], 4), dtype=np.float32)
        for f in range(nfrag):
            feat[g["index"][f]] = g["frag_feat"][f]
            assert np.array_equal(g["frag_grid"][f], g["grid"][g["index"][f]])
            assert np.array_equal(g["frag_coord"][f], g["coord"][g["index"][f]])  # no post-transform CenterShift in this block
        assert np.array_equal(feat[o_me], fx[f"aug{a}_feat"][o_ref]), a

        def members(index, grid, rows):
            out = {}
            for part in index:
                cells = [tuple(c) for c in grid[part]]
                assert len(set(cells)) == len(cells)  # one row per voxel and fragment
                for c, i in zip(cells, rows[part]):
                    out.setdefault(c, set()).add(int(i))
            return out
        mine = members(g["index"], g["grid"], restated["pick"])
        ref = members(fx[f"aug{a}_frag_index"], fx[f"aug{a}_grid"], kept)
        assert mine == ref, a
        sizes = [len(v) for v in mine.values()]
        assert max(sizes) == nfrag
        seen |= set(min(s, 3) for s in sizes)
        most = max(most, nfrag)
    assert seen == {1, 2, 3} and most >= 4  # the fixture holds voxels of 1, 2 and >= 3 rows and >= 4 fragments


def test_scale_of_a_float32_cloud_rounds_the_float64_product(fx):
    x = fx["coord"]
    got, _ = R.augment([("scale", 1.05)], x)
    assert got.dtype == np.float32 and np.array_equal(got, (x.astype(np.float64) * 1.05).astype(np.float32))
    assert not np.array_equal(got, x * np.float32(1.05))  # the two roundings differ on this cloud


# ------------------------------------------------------------------------------------------------ host logic, emulated ops
class EmulatedOps:
    """tests/emu_ops.py plus torch emulations of the ops TestPipeline adds or borrows from the train side: the host logic of
    prepare / vote / evaluate runs on the CPU (the kernels themselves are tested on the GPU, tests/test_gpu_testpipeline.py)."""

    def __getattr__(self, name):
        from tests import emu_ops
        return getattr(emu_ops, name)

    def _need_gpu(self, *ts):
        pass

    def tt_affine(self, xyz, scale=None, flipx=False, flipy=False, out_dtype=None, **kw):
        import torch
        assert not kw
        t = xyz.double()
        if scale is not None:
            t = t * scale
        sign = torch.tensor([-1.0 if flipx else 1.0, -1.0 if flipy else 1.0, 1.0], dtype=torch.float64)
        return (t * sign).to(out_dtype)

    def tt_voxel_pick(self, idx_sort, seg_start, m, r):
        s = seg_start[:m + 1].long()
        return idx_sort[s[:-1] + r[:m] % (s[1:] - s[:-1])].int()

    def voxel_inverse(self, idx_sort, cluster):
        import torch
        out = torch.empty(idx_sort.numel(), dtype=torch.int32)
        out[idx_sort.long()] = cluster[:idx_sort.numel()].int()
        return out

    def fragments_build(self, idx_sort, seg_start, m, frags, grid, feat, coord, center_shift=False):
        import torch
        idx = torch.stack([self.fragment_select(idx_sort, seg_start, m, f) for f in range(frags)]).long()
        c = coord[idx]
        if center_shift:
            c = torch.stack([self.center_shift(x, apply_z=False) for x in c])
        return idx.int(), c.float(), grid[idx], feat[idx]

    def softmax_vote_fragments(self, logits, index, pred):
        k, m = index.shape
        for f in range(k):
            self.softmax_vote(logits[f * m:(f + 1) * m], index[f], pred)
        return pred

    def gather_i32(self, src, idx):
        return src[idx.long()]


def test_segment_and_evaluate_host_logic_on_emulated_ops(fx, monkeypatch):
    """TestPipeline.segment (fragment_batch 1 and 2) and evaluate with the mini LiDAR model on the emulated op layer: the
    labels of the ORIGINAL points equal a manual loop over the restatement's fragments (model.inference per fragment, same
    seed, softmax, add, arg-max, [inverse]); the counters equal numpy's; every vote row sums to its number of fragments."""
    import torch
    import cdsegnet_amd.models  # noqa: F401
    from cdsegnet_amd import engine as engine_mod
    from cdsegnet_amd.registry import build_model
    from tests import emu_ops
    from tests.helpers import fixture_cfg, fixture_state_dict
    monkeypatch.setattr(engine_mod, "ops", emu_ops)
    monkeypatch.setattr(tt, "ops", EmulatedOps())
    mfx = load_fixture("mini_e2e_lidar.npz")
    mcfg = fixture_cfg(mfx)
    model = build_model(copy.deepcopy(mcfg))
    model.load_state_dict(fixture_state_dict(mfx), strict=True)
    model = model.eval()
    model.precision = "fp32"
    k = mcfg["num_classes"]
    cfg = copy.deepcopy(blocks()["nuscenes"])
    lists = cfg["test_cfg"]["aug_transform"]
    cfg["test_cfg"]["aug_transform"] = [lists[1], lists[9]]
    segment = fx["segment"].copy()
    segment[::29] = -1
    raw = dict(coord=torch.as_tensor(fx["coord"]), strength=torch.as_tensor(fx["strength"]), segment=torch.as_tensor(segment))
    draws = {"1.r": fx["1.r"]}
    tp = tt.TestPipeline(cfg)
    torch.manual_seed(3)
    labels, pred = tp.segment(model, raw, k, draws=draws, max_fragments=2)
    want = R.pipeline(cfg, dict(coord=fx["coord"], strength=fx["strength"], segment=segment), r=fx["1.r"], max_fragments=2)
    torch.manual_seed(3)
    votes = torch.zeros((want["n"], k))
    for g in want["augs"]:
        for f in range(g["index"].shape[0]):
            d = dict(coord=torch.as_tensor(g["frag_coord"][f]), grid_coord=torch.as_tensor(g["frag_grid"][f]),
                     feat=torch.as_tensor(g["frag_feat"][f]), offset=torch.tensor([g["index"].shape[1]]))
            votes[torch.as_tensor(g["index"][f]).long()] += torch.softmax(model.inference(d, eval=False)["seg_logits"].float(), -1)
    manual = votes.argmax(1).numpy()[want["inverse"]]
    assert labels.shape == (len(fx["coord"]),) and np.array_equal(labels.numpy(), manual)
    scene = tp.prepare(raw, draws=draws, max_fragments=2)
    keep = segment != -1
    p, t = manual[keep], segment[keep]
    inter, area_p, area_t = np.bincount(t[p == t], minlength=k), np.bincount(p, minlength=k), np.bincount(t, minlength=k)
    for x in (labels, pred):
        assert np.array_equal(tp.evaluate(x, scene, k, ignore_index=-1).numpy(), np.stack([inter, area_p + area_t - inter, area_t]))
    held = sum(torch.bincount(g["index"].reshape(-1).long(), minlength=scene.n) for g in scene.augs).double()
    for fb in (1, 2):
        _, pr = tp.vote(model, scene, k, fragment_batch=fb)
        assert torch.isfinite(pr).all() and ((pr.double().sum(1) - held).abs() <= 1e-5 * held).all()
