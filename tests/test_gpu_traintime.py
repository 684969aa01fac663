"""Train-time pipeline on the device (cdsegnet_amd/traintime.py, csrc/traintime.hip) against its numpy restatement
(tests/traintime_restatement.py) with the fixtures' recorded draws injected: the float64 kernels use no fused multiply-add
and the restatement performs the same operations in the same order, so every comparison here is exact (bit patterns and
integers).  The restatement itself is held to the reference in tests/test_cpu_traintime.py."""
import numpy as np
import pytest
import torch

import traintime_restatement as R
from cdsegnet_amd import ops
from cdsegnet_amd import traintime as tt
from oracle import philox
from test_cpu_traintime import TAGS, load_case

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _up(raw):
    return {k: torch.as_tensor(v).to(DEV) for k, v in raw.items()}


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64 if x.dtype == np.float64 else np.int32)


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("tag", TAGS)
def test_device_pipeline_equals_the_restatement_bit_for_bit(tag):
    cfg, raw, draws, ref, want, wtrace = load_case(tag)
    trace = {}
    got = tt.TrainTransform(cfg)(_up(raw), 0, draws=draws, trace=trace)
    torch.cuda.synchronize()
    assert np.array_equal(_np(trace["pre_index"]), wtrace["pre_index"])
    assert np.array_equal(_bits(_np(trace["pre_coord"])), _bits(wtrace["pre_coord"])), "float64 coordinates before GridSample"
    gs = wtrace["gridsample"]
    assert trace["num_voxels"] == len(gs["count"])
    assert np.array_equal(_np(trace["grid"]), gs["grid"])
    assert np.array_equal(_np(trace["seg_start"])[:len(gs["seg_start"])], gs["seg_start"])
    assert np.array_equal(_np(trace["idx_sort"]), gs["idx_sort"])
    assert np.array_equal(_np(trace["pick"]), gs["pick"])
    assert got["index"].dtype == torch.int32 and np.array_equal(_np(got["index"]), want["index"])  # crop membership AND order
    assert got["grid_coord"].dtype == torch.int32 and np.array_equal(_np(got["grid_coord"]), want["grid_coord"])
    assert np.array_equal(_np(got["segment"]), want["segment"]) and np.array_equal(want["segment"], raw["segment"][want["index"]])
    assert got["coord"].dtype == torch.float32 and np.array_equal(_bits(_np(got["coord"])), _bits(want["coord"]))
    assert got["feat"].dtype == torch.float32 and np.array_equal(_bits(_np(got["feat"])), _bits(want["feat"]))
    assert got["offset"].tolist() == got["offset_host"] == [len(want["coord"])]


@pytest.mark.parametrize("n", [1, 257, 1500])
def test_bbox_affine_jitter_and_colour_kernels_at_their_edges(n):
    rng = np.random.default_rng(n)
    x32 = (rng.standard_normal((n, 3)) * 3 + 1).astype(np.float32)
    x64 = rng.standard_normal((n, 3)) * 3 - 2
    for x in (x32, x64):
        assert np.array_equal(_np(ops.tt_bbox(torch.as_tensor(x).to(DEV))), R.bbox(x))
    rot = tt.rotation_matrix("y", 0.37)
    xd = torch.as_tensor(x64).to(DEV)
    bb = ops.tt_bbox(xd)
    got = ops.tt_affine(xd, center=ops.TT_CENTER_BBOX, bbox=bb, rot=rot, add_back=True, scale=1.07, flipx=True)
    want = R.flip(R.rotate(x64, rot, "bbox") * 1.07, True, False)
    assert np.array_equal(_bits(_np(got)), _bits(want))
    got = ops.tt_affine(torch.as_tensor(x32).to(DEV), center=ops.TT_CENTER_HOST, center3=[0.5, -1.0, 2.0], rot=rot, add_back=True,
                        flipy=True)
    assert np.array_equal(_bits(_np(got)), _bits(R.flip(R.rotate(x32.astype(np.float64), rot, [0.5, -1.0, 2.0]), False, True)))
    for apply_z, mode in ((True, ops.TT_CENTER_SHIFT_Z), (False, ops.TT_CENTER_SHIFT_XY)):
        got = ops.tt_affine(xd, center=mode, bbox=bb, out_dtype=torch.float32)
        assert np.array_equal(_bits(_np(got)), _bits(R.center_shift(x64, apply_z).astype(np.float32)))
    z = rng.standard_normal((n, 3)) * 4  # sigma z beyond the clip on many rows
    for zz in (z, z.astype(np.float32)):
        got = ops.tt_jitter(torch.as_tensor(x64).to(DEV), torch.as_tensor(zz).to(DEV), 0.005, 0.02)
        assert np.array_equal(_bits(_np(got)), _bits(R.jitter(x64, zz, 0.005, 0.02)))
        assert np.abs(_np(got) - x64).max() <= 0.02 + 1e-12
    col = rng.integers(0, 256, (n, 3)).astype(np.float32)
    if n > 1:  # (a single colour has hi == lo: the contrast stage divides by zero, in the reference too)
        cd = torch.as_tensor(col).to(DEV)
        got = ops.tt_color(cd.clone(), bbox=ops.tt_bbox(cd), blend=0.3, tr=[3.0, -200.0, 250.0], noise=torch.as_tensor(z).to(DEV),
                           noise_mul=0.05 * 255)
        want = R.color_chain(R.color_chain(R.color_chain(col, blend=0.3), tr=[3.0, -200.0, 250.0]), noise=z, noise_mul=0.05 * 255)
        assert np.array_equal(_bits(_np(got)), _bits(want)) and want.min() == 0.0 and want.max() == 255.0  # both clips are hit
    cd = torch.as_tensor(col).to(DEV)  # translation + float32 noise
    got = ops.tt_color(cd.clone(), tr=[1.5, 0.0, -1.5], noise=torch.as_tensor(z.astype(np.float32)).to(DEV), noise_mul=2.0)
    want = R.color_chain(R.color_chain(col, tr=[1.5, 0.0, -1.5]), noise=z.astype(np.float32), noise_mul=2.0)
    assert np.array_equal(_bits(_np(got)), _bits(want))


@pytest.mark.parametrize("dims", [(3, 3, 3), (5, 4, 7), (43, 33, 18)])
def test_elastic_blur_and_trilinear_apply(dims):
    rng = np.random.default_rng(sum(dims))
    noise = rng.standard_normal(dims + (3,)).astype(np.float32)
    blurred = R.blur(noise)
    blurred_dev = ops.tt_blur(torch.as_tensor(noise).to(DEV))
    assert np.array_equal(_bits(_np(blurred_dev)), _bits(blurred))
    g = 0.2
    start = np.array([1.0, -2.0, 0.25]) - g
    dim = np.array(dims)
    stop = start + g * (dim - 1)
    step = (stop - start) / (dim - 1)
    n = 777
    pts = start + rng.random((n, 3)) * (stop - start)
    pts[0] = start                                  # the first corner of the grid
    pts[1] = stop                                   # the last corner: on the outermost cell, still inside
    pts[2] = [stop[0], start[1], (start[2] + stop[2]) / 2]
    pts[3] = stop + [1e-9, 0.0, 0.0]                # just outside along x: fill value 0, the point does not move
    pts[4] = start - [0.0, 0.0, 0.5]                # outside along z
    pts[5] = start + step * [1, 2, 1]               # exactly on interior grid lines
    want = R.elastic_interp(pts, blurred, start, step, stop, 1.6)
    got = ops.tt_elastic(torch.as_tensor(pts).to(DEV), blurred_dev, start, step, stop, 1.6)
    assert np.array_equal(_bits(_np(got)), _bits(want))
    assert np.array_equal(want[3], pts[3]) and np.array_equal(want[4], pts[4]) and not np.array_equal(want[1], pts[1])


def _device_gridsample(coord64, grid_size, r):
    c = torch.as_tensor(coord64).to(DEV)
    grid, key, _ = ops.voxelize_any(c, grid_size)
    key_sorted, idx_sort = ops.sort_pairs(key, None, end_bit=63)
    _, seg_start, count = ops.pool_level(key_sorted, 0)
    m = int(count.item())
    return m, ops.tt_voxel_pick(idx_sort, seg_start, m, torch.as_tensor(np.asarray(r, dtype=np.int64)).to(DEV)), ops.max_run(seg_start, m)


def test_voxel_pick_fullest_voxel_single_voxel_and_one_point():
    rng = np.random.default_rng(5)
    coord = rng.random((900, 3)) * [1.0, 0.5, 0.3]
    coord[:37] = [0.512, 0.251, 0.101] + rng.random((37, 3)) * 0.01   # 37+ rows in one 5 cm voxel: the fullest one
    probe = R.grid_sample(coord, 0.05, np.zeros(1, dtype=np.int64))
    cmax = int(probe["count"].max())
    assert cmax >= 37 and (probe["count"] == 1).any()
    for r in (np.full(len(probe["count"]), cmax - 1), rng.integers(0, cmax, len(probe["count"])), np.zeros(len(probe["count"]))):
        want = R.grid_sample(coord, 0.05, r)
        m, pick, mx = _device_gridsample(coord, 0.05, r)
        assert m == len(want["count"]) and int(mx.item()) == cmax and np.array_equal(_np(pick), want["pick"])
        full = int(np.argmax(want["count"]))
        assert want["pick"][full] == want["idx_sort"][want["seg_start"][full] + int(r[full]) % cmax]
    one = rng.random((300, 3)) * 0.04 + 3.005  # a single-voxel cloud: member r % 300
    for r in ([0], [299], [300], [7 * 300 + 13]):
        m, pick, mx = _device_gridsample(one, 0.05, r)
        assert m == 1 and int(mx.item()) == 300 and _np(pick).tolist() == [r[0] % 300]
    m, pick, mx = _device_gridsample(one[:1], 0.05, [5])
    assert m == 1 and _np(pick).tolist() == [0]


@pytest.mark.parametrize("n", [2, 300, 1025])
def test_sphere_crop_keeps_all_but_the_farthest_row(n):
    rng = np.random.default_rng(n)
    coord = rng.standard_normal((n, 3))
    if n > 2:
        coord[n // 2] = coord[0]  # a tie at distance 0 with the centre row: (distance, row) order
    cd = torch.as_tensor(coord).to(DEV)
    key = ops.tt_dist_key(cd, 0)
    order = _np(ops.sort_pairs(key, None, end_bit=63)[1])
    sel, d2 = R.sphere_crop(coord, 0, n - 1)
    assert np.array_equal(_bits(d2), _np(key)) and np.array_equal(order[:n - 1], sel)
    assert order[-1] == np.argmax(d2) and order[0] == 0 and (n == 2 or order[1] == n // 2)
    # through the pipeline: point_max == n - 1 drops exactly the farthest row from the drawn centre
    coord[n // 2] += 0.5  # (no two rows in one voxel)
    cfg = [dict(type="GridSample", grid_size=1e-4, mode="train", return_grid_coord=True), dict(type="SphereCrop", point_max=n - 1, mode="random"),
           dict(type="ToTensor"), dict(type="Collect", keys=("coord", "grid_coord", "segment"), feat_keys=("coord",))]
    raw = dict(coord=torch.as_tensor(coord.astype(np.float32)).to(DEV), segment=torch.arange(n, device=DEV))
    out = tt.TrainTransform(cfg)(raw, 0, draws={"0.r": np.zeros(1, dtype=np.int64), "1.center": np.array(3 % n)})
    want = R.run(cfg, dict(coord=coord.astype(np.float32), segment=np.arange(n)), {"0.r": np.zeros(1, dtype=np.int64), "1.center": np.array(3 % n)})
    assert out["coord"].shape[0] == n - 1 and np.array_equal(_np(out["index"]), want["index"])
    assert np.array_equal(_np(out["segment"]), want["index"])


@pytest.mark.parametrize("n", [1, 6, 1027])
def test_rand_int_is_the_philox_stream_of_randn(n):
    seed, offset = 0x1234567811223344, 0x9_0000_0007
    nt = (n + 3) // 4
    t = np.arange(nt, dtype=np.uint64)
    ctr = np.stack([(t & np.uint64(0xFFFFFFFF)).astype(np.uint32), (t >> np.uint64(32)).astype(np.uint32),
                    np.full(nt, offset & 0xFFFFFFFF, dtype=np.uint32), np.full(nt, offset >> 32, dtype=np.uint32)], -1)
    key = np.stack([np.full(nt, seed & 0xFFFFFFFF, dtype=np.uint32), np.full(nt, seed >> 32, dtype=np.uint32)], -1)
    words = philox.philox4x32_10(ctr, key).reshape(-1)[:n].astype(np.int64)
    assert np.array_equal(_np(ops.rand_int(n, seed, offset, DEV)), words)
    assert np.array_equal(_np(ops.rand_int(n, seed, offset, DEV, bound=37)), words % 37)
    bd = torch.tensor([1000003], dtype=torch.int32, device=DEV)
    assert np.array_equal(_np(ops.rand_int(n, seed, offset, DEV, bound_dev=bd)), words % 1000003)


def test_generated_draws_are_reproducible_bounded_and_complete():
    cfg, raw, _, _, _, _ = load_case("C")
    rawd = _up(raw)
    tf = tt.TrainTransform(cfg, seed=11)
    ta, tb, tc = {}, {}, {}
    a, b = tf(rawd, 4, trace=ta), tf(rawd, 4, trace=tb)
    c = tt.TrainTransform(cfg, seed=12)(rawd, 4, trace=tc)
    d = tf(rawd, 5)
    for k in ("coord", "grid_coord", "segment", "feat", "index"):
        assert torch.equal(a[k], b[k]), k
    assert a["offset_host"] == b["offset_host"] and a["coord"].shape[0] == 2048
    assert not (a["index"].shape == c["index"].shape and torch.equal(a["index"], c["index"]))
    assert not (a["index"].shape == d["index"].shape and torch.equal(a["index"], d["index"]))
    assert bool(torch.isfinite(a["coord"]).all()) and bool(torch.isfinite(a["feat"]).all())
    # the generated draws, replayed as a record through the restatement, give the same output: nothing else is random
    record = {k: (_np(v) if isinstance(v, torch.Tensor) else v) for k, v in ta["draws"].items()}
    want = R.run(cfg, raw, record)
    assert np.array_equal(_np(a["index"]), want["index"]) and np.array_equal(_bits(_np(a["feat"])), _bits(want["feat"]))
    assert np.array_equal(_bits(_np(a["coord"])), _bits(want["coord"]))
    # every pick lies inside its voxel, and different seeds pick different members
    for t in (ta, tc):
        grid, pick = _np(t["grid"]), _np(t["pick"])
        vox = np.unique(grid, axis=0)
        assert len(pick) == t["num_voxels"] == len(vox) and np.array_equal(grid[pick], vox)  # key order = lexicographic order
        seg, srt = _np(t["seg_start"]), _np(t["idx_sort"])
        pos = np.searchsorted(seg[:t["num_voxels"] + 1], np.argsort(srt, kind="stable")[pick], side="right") - 1
        assert np.array_equal(pos, np.arange(t["num_voxels"]))
    # jitter within its clip; dropout keeps exactly int(n (1 - ratio)) distinct rows
    n = raw["coord"].shape[0]
    tail = [dict(type="GridSample", grid_size=0.02, mode="train", return_grid_coord=True), dict(type="ToTensor"),
            dict(type="Collect", keys=("coord", "grid_coord", "segment"), feat_keys=("coord",))]
    tj = {}
    tt.TrainTransform([dict(type="RandomJitter", sigma=0.005, clip=0.007)] + tail, seed=3)(dict(coord=rawd["coord"]), 0, trace=tj)
    moved = _np(tj["pre_coord"]) - raw["coord"].astype(np.float64)
    assert np.abs(moved).max() <= 0.007 + 1e-9 and (np.abs(moved) >= 0.007 - 1e-9).mean() > 0.05  # the clip binds (1.4 sigma)
    assert 0.003 < moved.std() < 0.005 and abs(moved.mean()) < 2e-4
    for ratio in (0.2, 0.37):
        td = {}
        out = tt.TrainTransform([dict(type="RandomDropout", dropout_ratio=ratio, dropout_application_ratio=1.0)] + tail, seed=3)(
            dict(coord=rawd["coord"], segment=rawd["segment"]), 9, trace=td)
        kept = _np(td["pre_index"])
        assert len(kept) == int(n * (1 - ratio)) == len(np.unique(kept)) and kept.min() >= 0 and kept.max() < n
        assert not np.array_equal(kept, np.sort(kept))  # a random subset in random order, not a prefix
        assert np.array_equal(_np(out["segment"]), raw["segment"][_np(out["index"])])


def test_two_scenes_through_transform_and_collate_train_the_mini_model():
    from test_gpu_train import _mini_training_model
    cfg = load_case("C")[0]
    tf = tt.TrainTransform(cfg, seed=1)
    dicts = []
    for scene, tag in enumerate(("C", "B")):
        raw = dict(load_case(tag)[1])
        raw["segment"] = raw["segment"] % 13
        dicts.append(tf(_up(raw), scene))
    batch = tt.collate(dicts, mix_prob=0.0)
    assert batch["offset_host"] == [2048, 4096] and batch["feat"].shape == (4096, 6) and batch["grid_coord"].dtype == torch.int32
    model, _ = _mini_training_model(dict(sd_seed=7), torch.device(DEV))
    torch.manual_seed(3)
    inp = {k: batch[k] for k in ("coord", "grid_coord", "feat", "offset", "segment")}
    loss = model(inp)["loss"]
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
