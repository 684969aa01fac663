"""GPU: the config-driven test pipeline (cdsegnet_amd.testtime.TestPipeline) and its kernels (csrc/testtime.hip:
cdseg_fragments_build, cdseg_softmax_vote_fragments, cdseg_voxel_inverse).  Integer outputs and float bit patterns are compared
exactly: against the numpy restatement (tests/testtime_restatement.py, itself pinned to the reference by
tests/test_cpu_testpipeline.py), against the existing per-fragment ops, and end to end with the mini LiDAR model."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from tests import testtime_restatement as R
from tests.helpers import GOLDEN, fixture_cfg, fixture_state_dict, load_fixture

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from cdsegnet_amd import ops as _ops
    assert torch.cuda.is_available()
    return _ops


@pytest.fixture(scope="module")
def tt():
    from cdsegnet_amd import testtime
    return testtime


@pytest.fixture(scope="module")
def blocks():
    with open(os.path.join(GOLDEN, "test_blocks.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def nus():
    return load_fixture("testtime_nuscenes.npz")


def dev(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x)
    return (t if dtype is None else t.to(dtype)).cuda().contiguous()


def bits(t):
    """Integer image of a float tensor: equality of bit patterns (-0.0 != 0.0, NaN == NaN)."""
    t = t.contiguous()
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def nus_raw(fx):
    return dict(coord=dev(fx["coord"]), strength=dev(fx["strength"]), segment=dev(fx["segment"]))


# ------------------------------------------------------------------------------------------------ pipeline
def test_device_pipeline_equals_the_restatement_on_the_nuscenes_fixture(ops, tt, blocks, nus):
    """TestPipeline(nuScenes test block).prepare with the recorded pick: kept rows, inverse, and per augmentation the augmented
    cloud (with its dtype) and the dense fragments, bit for bit."""
    want = R.pipeline(blocks["nuscenes"], dict(coord=nus["coord"], strength=nus["strength"], segment=nus["segment"]), r=nus["1.r"])
    scene = tt.TestPipeline(blocks["nuscenes"]).prepare(nus_raw(nus), draws={"1.r": nus["1.r"]})
    torch.cuda.synchronize()
    assert scene.n == want["n"] and scene.n_raw == len(nus["coord"])
    assert np.array_equal(scene.trace["pick"].cpu().numpy(), want["pick"])
    assert scene.inverse.dtype == torch.int32 and np.array_equal(scene.inverse.cpu().numpy(), want["inverse"])
    assert np.array_equal(scene.origin_segment.cpu().numpy(), nus["origin_segment"])
    assert np.array_equal(scene.segment.cpu().numpy(), want["segment"])
    assert len(scene.augs) == len(want["augs"]) == 10
    pos = 0
    for a, (g, w) in enumerate(zip(scene.augs, want["augs"])):
        c = g["aug_coord"].cpu().numpy()
        assert c.dtype == w["coord"].dtype and np.array_equal(c.view(np.int32), w["coord"].view(np.int32)), a
        assert g["index"].dtype == torch.int32 and np.array_equal(g["index"].cpu().numpy(), w["index"]), a
        assert g["grid_coord"].dtype == torch.int32 and np.array_equal(g["grid_coord"].cpu().numpy(), w["frag_grid"]), a
        for k, wk in (("coord", "frag_coord"), ("feat", "frag_feat")):
            got = g[k].cpu().numpy()
            assert got.dtype == np.float32 and got.shape == w[wk].shape and np.array_equal(got.view(np.int32), w[wk].view(np.int32)), (a, k)
        # the flat list: zero-copy views in aug-major, fragment-minor order
        nfrag, m = w["index"].shape
        assert (g["num_fragments"], g["num_voxels"], g["first"]) == (nfrag, m, pos)
        for f in range(nfrag):
            d = scene.fragments[pos + f]
            for k in ("coord", "grid_coord", "feat", "index"):
                assert d[k].data_ptr() == g[k][f].data_ptr() and d[k].shape == g[k][f].shape and d[k].is_contiguous()
            assert d["offset"].tolist() == [m] and d["offset"].dtype == torch.int64 and d["offset_host"] == [m]
        pos += nfrag
    assert len(scene.fragments) == pos


def test_default_pick_is_keyed_by_seed_and_scene(tt, blocks, nus):
    """draws=None: the member pick comes from the library's Philox keyed by (seed, scene_index) - equal keys, equal scenes;
    every pick is a member of its voxel."""
    tp = tt.TestPipeline(blocks["nuscenes"], seed=3)
    raw = nus_raw(nus)
    a, b, c = tp.prepare(raw, 5), tp.prepare(raw, 5), tp.prepare(raw, 6)
    pa, pb, pc = (s.trace["pick"].cpu().numpy() for s in (a, b, c))
    assert np.array_equal(pa, pb) and not np.array_equal(pa, pc)
    grid = nus["grid025_raw"]
    assert np.array_equal(grid[pa][a.inverse.cpu().numpy()], grid) and np.array_equal(grid[pc][c.inverse.cpu().numpy()], grid)


@pytest.mark.parametrize("grid", ["config", "fixture"])
def test_scannet_block_equals_prepare_test_fragments(tt, blocks, grid):
    """The ScanNet test block through TestPipeline against the hand-written path (prepare_test_fragments: one
    fragment_select, three gathers and a center_shift per fragment), fragment by fragment, bit for bit."""
    fx = load_fixture("tta_pipeline.npz")
    cfg = copy.deepcopy(blocks["scannet"])
    if grid == "fixture":
        cfg["test_cfg"]["voxelize"]["grid_size"] = float(fx["grid_size"])
    gsize = cfg["test_cfg"]["voxelize"]["grid_size"]
    coord, color, normal = dev(fx["coord"]), dev(fx["color"]), dev(fx["normal"])
    idxs, dicts = tt.prepare_test_fragments(coord, color, normal, gsize)
    scene = tt.TestPipeline(cfg).prepare(dict(coord=coord, color=color, normal=normal))
    torch.cuda.synchronize()
    assert scene.inverse is None and scene.n == len(fx["coord"])
    assert len(scene.fragments) == len(dicts) and len(scene.augs) == 13
    if grid == "fixture":
        assert max(g["num_fragments"] for g in scene.augs) >= 2
    for i, (idx, d, s) in enumerate(zip(idxs, dicts, scene.fragments)):
        assert same(s["index"], idx), i
        assert same(s["coord"], d["coord"].float()), i
        assert same(s["grid_coord"], d["grid_coord"]) and same(s["feat"], d["feat"]), i
        assert same(s["offset"], d["offset"]) and s["offset_host"] == d["offset_host"], i


# ------------------------------------------------------------------------------------------------ kernels
def _layout(m, mixed, seed):
    """A voxel sort of n rows into m runs: all counts 1, or counts 1..9 with a 9 (m > 1) in a random permutation of rows."""
    rng = np.random.default_rng(seed)
    count = rng.integers(1, 10, m) if mixed else np.ones(m, dtype=np.int64)
    if mixed:
        count[rng.integers(0, m)] = 9
    n = int(count.sum())
    seg = np.concatenate([[0], np.cumsum(count)]).astype(np.int32)
    return n, int(count.max()), dev(rng.permutation(n).astype(np.int32)), dev(seg), rng


@pytest.mark.parametrize("mixed", [False, True], ids=["counts1", "counts1to9"])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 1000])
def test_fragments_build_equals_the_composition_of_the_per_fragment_ops(ops, m, mixed):
    """cdseg_fragments_build against fragment_select + gather_rows (+ center_shift(apply_z=False)) + .float() per fragment:
    float32 / float64 coordinates, C = 4 (16-byte rows) / 6 (8-byte accesses) / 5 (4-byte), with and without the shift."""
    n, nfrag, idx_sort, seg, rng = _layout(m, mixed, 100 * m + mixed)
    assert nfrag == (9 if mixed else 1)
    grid = dev(rng.integers(0, 1 << 20, (n, 3)).astype(np.int32))
    xyz = rng.normal(0, 20, (n, 3))
    for cdt in (torch.float32, torch.float64):
        coord = dev(xyz, cdt)
        for c in (4, 6, 5):
            feat = dev(rng.normal(size=(n, c)).astype(np.float32))
            for shift in (False, True):
                index, fc, fg, ff = ops.fragments_build(idx_sort, seg, m, nfrag, grid, feat, coord, center_shift=shift)
                assert index.shape == (nfrag, m) and fc.shape == (nfrag, m, 3) and fc.dtype == torch.float32
                assert fg.shape == (nfrag, m, 3) and ff.shape == (nfrag, m, c)
                for f in range(nfrag):
                    idx = ops.fragment_select(idx_sort, seg, m, f)
                    cc = ops.gather_rows(coord, idx)
                    if shift:
                        cc = ops.center_shift(cc, apply_z=False)
                    tag = (str(cdt), c, shift, f)
                    assert same(index[f], idx), tag
                    assert same(fc[f], cc.float()), tag
                    assert same(fg[f], ops.gather_rows(grid, idx)) and same(ff[f], ops.gather_rows(feat, idx)), tag


def test_fragments_build_and_vote_of_nothing_are_no_ops(ops):
    e = lambda *s, dt=torch.float32: torch.empty(s, dtype=dt, device="cuda")  # noqa: E731
    index, fc, fg, ff = ops.fragments_build(e(0, dt=torch.int32), torch.zeros(1, dtype=torch.int32, device="cuda"), 0, 0,
                                            e(0, 3, dt=torch.int32), e(0, 4), e(0, 3), center_shift=True)
    assert index.shape == (0, 0) and ff.shape == (0, 0, 4)
    pred = torch.ones(3, 5, device="cuda")
    ops.softmax_vote_fragments(e(0, 5), e(2, 0, dt=torch.int32), pred)
    assert torch.equal(pred, torch.ones(3, 5, device="cuda"))
    assert ops.voxel_inverse(e(0, dt=torch.int32), e(0, dt=torch.int32)).shape == (0,)


@pytest.mark.parametrize("c", [13, 16, 20, 200])
@pytest.mark.parametrize("k", [1, 2, 5])
def test_softmax_vote_fragments_equals_successive_softmax_votes(ops, k, c):
    """One launch for k collated fragments against k softmax_vote launches in fragment order: the same sums, bit for bit
    (members repeat across fragments: voxels of fewer than k rows are voted for more than once)."""
    m = 333
    n, nfrag, idx_sort, seg, rng = _layout(m, True, 7 * k + c)
    index = torch.stack([ops.fragment_select(idx_sort, seg, m, f) for f in range(k)])
    logits = dev((rng.normal(size=(k * m, c)) * 4).astype(np.float32))
    start = dev(rng.random((n, c)).astype(np.float32))
    want = start.clone()
    for f in range(k):
        ops.softmax_vote(logits[f * m:(f + 1) * m], index[f], want)
    got = ops.softmax_vote_fragments(logits, index, start.clone())
    assert same(got, want)
    untouched = np.setdiff1d(np.arange(n), index.cpu().numpy().ravel())
    assert torch.equal(got[dev(untouched)], start[dev(untouched)])


def test_voxel_inverse_is_the_scatter_of_the_cluster_ranks(ops):
    n, _, idx_sort, seg, rng = _layout(700, True, 3)
    cluster = dev(np.repeat(np.arange(700), np.diff(seg.cpu().numpy())).astype(np.int32))
    want = torch.empty(n, dtype=torch.int32, device="cuda")
    want[idx_sort.long()] = cluster
    assert same(ops.voxel_inverse(idx_sort, cluster), want)


# ------------------------------------------------------------------------------------------------ call count
class CountingOps:
    """Stands in for cdsegnet_amd.ops inside cdsegnet_amd.testtime and counts the library calls."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        v = getattr(self._real, name)
        if not callable(v) or name in ("bind_stream", "unbind_stream"):
            return v

        def counted(*a, **k):
            self.calls.append(name)
            return v(*a, **k)
        return counted


def test_prepare_makes_the_same_number_of_library_calls_whatever_the_fragment_count(ops, tt, blocks, monkeypatch):
    """Two scans whose largest voxel holds 2 and 9 points: 2 and 9 fragments per augmentation, the same ops.* calls."""
    rng = np.random.default_rng(4)
    base = (np.stack(np.meshgrid(np.arange(12), np.arange(10), np.arange(3), indexing="ij"), -1).reshape(-1, 3) * 0.1 + 0.011)
    calls, frags = [], []
    for most in (2, 9):
        extra = np.repeat(base[17:18], most - 1, 0)  # exact copies: one voxel under every augmentation
        coord = np.concatenate([base, extra]).astype(np.float32)
        n = len(coord)
        raw = dict(coord=dev(coord), color=dev(rng.integers(0, 256, (n, 3)).astype(np.float32)),
                   normal=dev(rng.normal(size=(n, 3)).astype(np.float32)))
        proxy = CountingOps(ops)
        monkeypatch.setattr(tt, "ops", proxy)
        scene = tt.TestPipeline(blocks["scannet"]).prepare(raw)
        monkeypatch.setattr(tt, "ops", ops)
        assert [g["num_fragments"] for g in scene.augs] == [most] * 13
        calls.append(proxy.calls)
        frags.append(len(scene.fragments))
    assert frags == [26, 117]
    assert calls[0] == calls[1] and calls[0].count("fragments_build") == 13
    assert "fragment_select" not in calls[0] and "gather_rows" not in calls[0]


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def mini():
    """The 4-channel mini model of tests/golden/mini_e2e_lidar.npz in fp32, and a three-list cut of the nuScenes test block
    (scale 0.9; scale 1; scale 1.1 + flip)."""
    import cdsegnet_amd.models  # noqa: F401
    from cdsegnet_amd.registry import build_model
    fx = load_fixture("mini_e2e_lidar.npz")
    cfg = fixture_cfg(fx)
    model = build_model(copy.deepcopy(cfg))
    model.load_state_dict(fixture_state_dict(fx), strict=True)
    model = model.cuda().eval()
    model.precision = "fp32"
    return model, cfg["num_classes"]


def _block3(blocks):
    cfg = copy.deepcopy(blocks["nuscenes"])
    lists = cfg["test_cfg"]["aug_transform"]
    cfg["test_cfg"]["aug_transform"] = [lists[0], lists[2], lists[9]]
    return cfg


def test_segment_equals_a_manual_loop_and_evaluate_equals_numpy(ops, tt, blocks, nus, mini):
    """segment(fragment_batch=1): the labels of the ORIGINAL points equal a manual loop over the restatement's fragments
    (model.inference per fragment under the same seed, softmax, add, arg-max, [inverse]); evaluate's counters equal numpy's
    intersection / union / target on those labels."""
    model, k = mini
    cfg = _block3(blocks)
    segment = nus["segment"].copy()
    segment[::37] = -1  # ignored rows
    raw = dict(nus_raw(nus), segment=dev(segment))
    draws = {"1.r": nus["1.r"]}
    tp = tt.TestPipeline(cfg)
    torch.manual_seed(11)
    labels, pred = tp.segment(model, raw, k, draws=draws, fragment_batch=1)
    # -- the manual loop
    want = R.pipeline(cfg, dict(coord=nus["coord"], strength=nus["strength"], segment=segment), r=nus["1.r"])
    torch.manual_seed(11)
    votes = torch.zeros((want["n"], k), dtype=torch.float32, device="cuda")
    for g in want["augs"]:
        nfrag, m = g["index"].shape
        for f in range(nfrag):
            d = dict(coord=dev(g["frag_coord"][f]), grid_coord=dev(g["frag_grid"][f]), feat=dev(g["frag_feat"][f]),
                     offset=dev(np.array([m], dtype=np.int64)))
            logits = model.inference(d, eval=False)["seg_logits"]
            votes[dev(g["index"][f]).long()] += torch.softmax(logits.float(), -1)
    manual = votes.argmax(1).cpu().numpy()[want["inverse"]]
    got = labels.cpu().numpy()
    print(f"[measure] segment vs manual loop: {int((got != manual).sum())} of {len(manual)} labels differ, "
          f"max vote difference {float((pred - votes).abs().max()):.3e}")
    assert labels.dtype == torch.int32 and got.shape == (len(nus["coord"]),) and pred.shape == (want["n"], k)
    assert np.array_equal(got, manual)
    # -- evaluate
    scene = tp.prepare(raw, draws=draws)
    keep = segment != -1
    p, t = manual[keep], segment[keep]
    inter = np.bincount(t[p == t], minlength=k)
    area_p, area_t = np.bincount(p, minlength=k), np.bincount(t, minlength=k)
    ref = np.stack([inter, area_p + area_t - inter, area_t])
    for x in (labels, pred):
        counts = tp.evaluate(x, scene, k, ignore_index=-1)
        assert counts.dtype == torch.int64 and np.array_equal(counts.cpu().numpy(), ref)
    assert ref[2].sum() == keep.sum() and ref[0].sum() > 0


@pytest.mark.parametrize("fragment_batch", [1, 3])
def test_every_vote_row_sums_to_the_number_of_fragments_that_hold_the_point(tt, blocks, nus, mini, fragment_batch):
    model, k = mini
    tp = tt.TestPipeline(_block3(blocks))
    raw, draws = nus_raw(nus), {"1.r": nus["1.r"]}
    torch.manual_seed(5)
    labels, pred = tp.segment(model, raw, k, draws=draws, fragment_batch=fragment_batch)
    scene = tp.prepare(raw, draws=draws)
    held = torch.zeros(scene.n, dtype=torch.float64, device="cuda")
    for g in scene.augs:
        held += torch.bincount(g["index"].reshape(-1).long(), minlength=scene.n)
    assert held.min() >= len(scene.augs) and held.max() > held.min()
    assert torch.isfinite(pred).all() and (pred >= 0).all()
    err = ((pred.double().sum(1) - held).abs() / held).max().item()
    print(f"[measure] fragment_batch={fragment_batch}: max |row sum - fragments| / fragments = {err:.3e}")
    assert err <= 1e-5
    assert labels.shape == (scene.n_raw,) and int(labels.min()) >= 0 and int(labels.max()) < k
