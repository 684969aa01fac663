"""GPU: test-time voting on shared geometry - cdseg_slots_select against numpy, a plan shared by the forwards of an augmentation
(the same logits bit for bit, on one stream and on lanes), collated forwards under per-fragment draws against the oracle's
single-fragment forwards, and the optional geometry check.  The host logic is tested on the CPU (tests/test_cpu_vote_shared.py)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import vote_shared_common as C
from tests.helpers import load_fixture

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from cdsegnet_amd import ops as _ops
    assert torch.cuda.is_available()
    return _ops


def dev(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x)
    return (t if dtype is None else t.to(dtype)).cuda().contiguous()


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ cdseg_slots_select
def _padded(sizes, K):
    """offs, offs_pad of the reference's padding (ptv3.py:188-250): an element of more than K points pads to a multiple of K."""
    offs, offs_pad = [0], [0]
    for c in sizes:
        offs.append(offs[-1] + c)
        offs_pad.append(offs_pad[-1] + ((c + K - 1) // K * K if c > K else c))
    return np.asarray(offs, dtype=np.int32), np.asarray(offs_pad, dtype=np.int32)


SELECT_CASES = [
    ("B1_pads_to_8", [5], 4),
    ("B3_unpadded_4_10", [3, 4, 10], 4),
    ("B24", [3, 4, 5, 10] * 6, 4),
    ("K1024", [1000, 1024, 1030], 1024),
    ("npad255", [3, 252], 4),
    ("npad256", [4, 252], 4),
    ("npad257", [1, 256], 4),
]


@pytest.mark.parametrize("name,sizes,K", SELECT_CASES, ids=[c[0] for c in SELECT_CASES])
def test_slots_select_equals_numpy(ops, name, sizes, K):
    """Four slot plans of one level (ops.pad_plan on four random orders) composed element by element: all elements on one
    source (that source bit for bit, the other sources NULL), every element on another source, every source used."""
    rng = np.random.default_rng(len(sizes) * 1000 + K)
    nb = len(sizes)
    offs, offs_pad = _padded(sizes, K)
    n_pad = int(offs_pad[-1])
    if name.startswith("npad"):
        assert n_pad == int(name[4:])
    offs_d, offs_pad_d = dev(offs), dev(offs_pad)
    srcs = []
    for _ in range(4):
        order = np.concatenate([a + rng.permutation(b - a) for a, b in zip(offs[:-1], offs[1:])]).astype(np.int32)
        srcs.append(ops.pad_plan(dev(order), offs_d, offs_pad_d, K, n_pad))
    host = [(g.cpu().numpy(), w.cpu().numpy()) for g, w in srcs]
    elem = np.repeat(np.arange(nb), np.diff(offs_pad))  # batch element of every padded slot
    assert any((w == -1).any() for _, w in host) == any(c > K and c % K for c in sizes)

    def check(choice, sources):
        g, w = ops.slots_select(sources, offs_pad_d, choice, n_pad)
        torch.cuda.synchronize()
        assert g.dtype == w.dtype == torch.int32 and g.shape == w.shape == (n_pad,)
        pick = np.asarray(choice)[elem]
        want_g = np.stack([h[0] for h in host])[pick, np.arange(n_pad)]
        want_w = np.stack([h[1] for h in host])[pick, np.arange(n_pad)]
        assert np.array_equal(g.cpu().numpy(), want_g) and np.array_equal(w.cpu().numpy(), want_w), choice
        return g, w

    for c in (0, 2, 3):  # all equal: the source itself, the others absent
        g, w = check([c] * nb, [srcs[i] if i == c else None for i in range(c + 1)])
        assert torch.equal(g, srcs[c][0]) and torch.equal(w, srcs[c][1])
    check([(b + 1) % 4 for b in range(nb)], srcs if nb >= 4 else [srcs[i] if i in {(b + 1) % 4 for b in range(nb)} else None
                                                                   for i in range(4)])  # neighbours differ
    if nb >= 4:
        choice = list(rng.permutation(np.arange(nb) % 4))  # every source used, in no order
        assert set(choice) == {0, 1, 2, 3}
        check(choice, srcs)
    else:
        for shift in range(4):  # every source used over the calls
            choice = [(shift + b) % 4 for b in range(nb)]
            check(choice, [srcs[i] if i in set(choice) else None for i in range(4)])
    for (g, w), (hg, hw) in zip(srcs, host):  # the sources are read only
        assert np.array_equal(g.cpu().numpy(), hg) and np.array_equal(w.cpu().numpy(), hw)


def test_slots_select_refuses_before_any_launch(ops):
    """A chosen NULL source is CDSEG_ERR_ARG, more than CDSEG_SLOTS_SELECT_MAX elements CDSEG_ERR_UNSUPPORTED - both
    returned by the host code before a launch: the output buffers keep their fill."""
    from cdsegnet_amd import _lib
    lib = _lib.load()
    assert ops.SLOTS_SELECT_MAX == 64
    sizes, K = [5, 3, 4], 4
    offs, offs_pad = _padded(sizes, K)
    n_pad = int(offs_pad[-1])
    offs_pad_d = dev(offs_pad)
    src = ops.pad_plan(None, dev(offs), offs_pad_d, K, n_pad)
    with pytest.raises(_lib.CdsegError, match="CDSEG_ERR_ARG"):
        ops.slots_select([src, None], offs_pad_d, [0, 1, 0], n_pad)
    with pytest.raises(_lib.CdsegError, match="CDSEG_ERR_ARG"):
        ops.slots_select([src], offs_pad_d, [0, 1, 0], n_pad)  # a choice beyond the sources
    many = ops.SLOTS_SELECT_MAX + 1
    offs_many = dev(np.arange(many + 1, dtype=np.int32))
    one = ops.pad_plan(None, offs_many, offs_many, K, many)
    with pytest.raises(_lib.CdsegError, match="CDSEG_ERR_UNSUPPORTED"):
        ops.slots_select([one], offs_many, [0] * many, many)
    offs_cap = offs_many[:many].contiguous()  # the cap itself is served
    at_cap = ops.pad_plan(None, offs_cap, offs_cap, K, many - 1)
    g, w = ops.slots_select([at_cap], offs_cap, [0] * (many - 1), many - 1)
    assert torch.equal(g, at_cap[0]) and torch.equal(w, at_cap[1])
    # the raw entry point: outputs untouched after the refusals
    out_g = torch.full((n_pad,), -7, dtype=torch.int32, device="cuda")
    out_w = torch.full((n_pad,), -7, dtype=torch.int32, device="cuda")
    gs = (ctypes.c_void_p * 2)(src[0].data_ptr(), None)
    ws = (ctypes.c_void_p * 2)(src[1].data_ptr(), None)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    r = lib.cdseg_slots_select(gs, ws, 2, offs_pad_d.data_ptr(), 3, bytes([0, 1, 0]), n_pad, out_g.data_ptr(), out_w.data_ptr(), st)
    assert r == -1
    r = lib.cdseg_slots_select(gs, ws, 1, offs_many.data_ptr(), many, bytes(many), n_pad, out_g.data_ptr(), out_w.data_ptr(), st)
    assert r == -4
    torch.cuda.synchronize()
    assert bool((out_g == -7).all()) and bool((out_w == -7).all())


def test_randn_fills_a_row_slice_like_a_fresh_tensor(ops):
    whole = torch.zeros((30, 4), dtype=torch.float32, device="cuda")
    for j in range(3):
        ops.randn((10, 4), 123, 40 + j, whole.device, out=whole[10 * j:10 * (j + 1)])
    for j in range(3):
        assert bits_equal(whole[10 * j:10 * (j + 1)], ops.randn((10, 4), 123, 40 + j, whole.device))


# ------------------------------------------------------------------------------------------------ the mini model, the sweep
@pytest.fixture(scope="module")
def world():
    """The mini LiDAR model on the GPU, the three-list nuScenes pipeline and the prepared 2599-point sweep."""
    from cdsegnet_amd import testtime as tt
    fx = load_fixture("testtime_nuscenes.npz")
    model, cfg, sd = C.mini_model("cuda")
    tp = tt.TestPipeline(C.block_cut())
    raw = dict(coord=dev(fx["coord"]), strength=dev(fx["strength"]), segment=dev(fx["segment"]))
    draws = {"1.r": fx["1.r"]}
    scene = tp.prepare(raw, draws=draws)
    torch.cuda.synchronize()
    assert len(scene.augs) == 3 and len(fx["coord"]) == 2599
    return dict(model=model, cfg=cfg, sd=sd, tp=tp, raw=raw, draws=draws, scene=scene, k=cfg["num_classes"],
                ch=cfg["c_in_channels"])


def _frag_draws(world):
    return [C.fragment_draws(f, d["feat"].shape[0], world["ch"]) for f, d in enumerate(world["scene"].fragments)]


@pytest.mark.parametrize("precision", ["fp32", "fp16+head"])
def test_shared_plan_gives_every_fragment_the_same_logits_bit_for_bit(world, precision):
    """fragment_batch = 1 under injected draws: every fragment's logits with one plan per augmentation equal those of the
    forwards that build their own, bit for bit - on the default lanes and with lanes=3; vote(share_plan=True) builds 3 plans
    where the default builds one per fragment."""
    model, scene, tp, k = world["model"], world["scene"], world["tp"], world["k"]
    model.precision = precision
    try:
        eng = model.engine()
        frags = scene.fragments
        draws = _frag_draws(world)
        base = model.inference_many([dict(d) for d in frags], draws=[dict(d) for d in draws])
        torch.cuda.synchronize()
        before = eng.plans_built
        plans = [model.plan(frags[g["first"]]) for g in scene.augs]
        assert eng.plans_built - before == 3
        per_frag = [plans[a] for a, g in enumerate(scene.augs) for _ in range(g["num_fragments"])]
        for lanes in (4, 3, 1):
            outs = model.inference_many([dict(d) for d in frags], draws=[dict(d) for d in draws], plans=per_frag, lanes=lanes)
            torch.cuda.synchronize()
            assert eng.plans_built - before == 3  # no forward built a plan
            for f, (o, b) in enumerate(zip(outs, base)):
                assert bits_equal(o["seg_logits"], b["seg_logits"]), (lanes, f)
        del plans, per_frag
        # the pipeline: plans per vote, the same labels
        torch.manual_seed(5)
        before = eng.plans_built
        labels0, pred0 = tp.vote(model, scene, k)
        assert eng.plans_built - before == len(frags) > 3
        torch.manual_seed(5)
        before = eng.plans_built
        labels1, pred1 = tp.vote(model, scene, k, share_plan=True)
        assert eng.plans_built - before == 3
        torch.cuda.synchronize()
        assert torch.equal(labels0, labels1) and torch.equal(pred0, pred1)
    finally:
        model.precision = "fp32"


@pytest.fixture(scope="module")
def oracle_logits(world):
    """The oracle's single-fragment logits of fragments 0..2 of every list under that fragment's draws: computed once."""
    from oracle import model as OM
    cfg, sd, scene = world["cfg"], world["sd"], world["scene"]
    out = {}
    for g in scene.augs:
        for j in range(3):
            f = g["first"] + j
            d = scene.fragments[f]
            m = d["feat"].shape[0]
            inp = dict(coord=d["coord"].cpu().numpy(), grid_coord=d["grid_coord"].cpu().numpy(), feat=d["feat"].cpu().numpy(),
                       offset=np.array([m], dtype=np.int64))
            out[f] = OM.inference(cfg["backbone"], sd, inp, C.fragment_draws(f, m, world["ch"]), T=cfg["T"]).numpy()
    return out


def test_a_batch_of_three_fragments_under_their_own_draws_equals_three_oracle_forwards(world, oracle_logits):
    """fragment_batch = 3, fragment_draws = "fragment", fp32: in every group the three fragments differ in every one of the 8
    order shuffles (tests/vote_shared_common.py); each fragment's slice of the collated logits is held to the project's fp32
    bound (tests/test_gpu_e2e.py: max |logit - oracle| < 1e-3, arg-max agreement > 99.9 %) against the oracle's forward of
    that fragment alone under its draws, and so is the single device forward.  A wrong curve moves the oracle's logits by
    3e-2 on this fixture (tests/test_cpu_vote_shared.py).  The maximum |batched - single| is printed, not bounded."""
    model, scene, ch = world["model"], world["scene"], world["ch"]
    assert model.precision == "fp32"
    worst = 0.0
    for a, g in enumerate(scene.augs):
        f0, m = g["first"], g["num_voxels"]
        for p in range(C.N_DRAWS):
            assert len({tuple(C.fragment_perms(f0 + j)[p]) for j in range(3)}) >= 2
        d3 = scene.collated(a, 0, 3)
        assert d3["shared_geometry"] and d3["offset_host"] == [m, 2 * m, 3 * m]
        plan = model.plan(d3)
        out = model.inference(dict(d3), eval=False, draws=C.group_draws(f0, 3, m, ch), plan=plan)["seg_logits"]
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        for j in range(3):
            ref = oracle_logits[f0 + j]
            single = model.inference(dict(scene.fragments[f0 + j]), eval=False, draws=C.fragment_draws(f0 + j, m, ch))["seg_logits"]
            single = single.cpu().numpy()
            got = out[j * m:(j + 1) * m]
            err_b, err_s = float(np.abs(got - ref).max()), float(np.abs(single - ref).max())
            agree_b = float((got.argmax(1) == ref.argmax(1)).mean())
            agree_s = float((single.argmax(1) == ref.argmax(1)).mean())
            worst = max(worst, float(np.abs(got - single).max()))
            print(f"[measure] list {a} fragment {j}: batched vs oracle {err_b:.3e} (arg-max {agree_b:.4f}), "
                  f"single vs oracle {err_s:.3e} (arg-max {agree_s:.4f}), batched vs single {float(np.abs(got - single).max()):.3e}")
            assert err_b < 1e-3 and agree_b > 0.999, (a, j, err_b, agree_b)
            assert err_s < 1e-3 and agree_s > 0.999, (a, j, err_s, agree_s)
        del plan
    print(f"[measure] max |batched - single| over {3 * len(scene.augs)} fragments = {worst:.3e}")


@pytest.mark.parametrize("noise_source", ["torch_cpu", "device"])
def test_faithful_batches_vote_what_fragment_batch_1_votes(world, noise_source):
    """segment-level: fragment_batch=3 with fragment_draws="fragment" against fragment_batch=1 under one seed, fp32 - the
    generator ends in the same state and every summed vote agrees within what two forwards inside the fp32 bound can differ:
    |softmax(z + d) - softmax(z)| <= 2 max|d| per class and vote, d < 2e-3."""
    model, scene, tp, k = world["model"], world["scene"], world["tp"], world["k"]
    model.noise_source = noise_source
    try:
        torch.manual_seed(9)
        labels1, pred1 = tp.vote(model, scene, k, share_plan=True)
        state1 = torch.get_rng_state()
        torch.manual_seed(9)
        labels3, pred3 = tp.vote(model, scene, k, fragment_batch=3, share_plan=True, fragment_draws="fragment")
        state3 = torch.get_rng_state()
        torch.cuda.synchronize()
    finally:
        model.noise_source = "torch_cpu"
    assert torch.equal(state1, state3)
    held = torch.zeros(scene.n, dtype=torch.float32, device="cuda")
    for g in scene.augs:
        held += torch.bincount(g["index"].reshape(-1).long(), minlength=scene.n)
    err = ((pred3 - pred1).abs().max(1).values / held).max().item()
    print(f"[measure] {noise_source}: max |vote difference| per held fragment = {err:.3e}, "
          f"{int((labels1 != labels3).sum())} of {labels1.numel()} labels differ")
    assert err <= 4e-3


def test_check_shared_geometry_refuses_a_grid_that_differs_in_one_row(world):
    from cdsegnet_amd._lib import CdsegError
    model, scene = world["model"], world["scene"]
    frag = scene.fragments[1]
    m = frag["feat"].shape[0]
    plan = model.plan(frag)
    draws = C.fragment_draws(1, m, world["ch"])
    base = model.inference(dict(frag), eval=False, draws=dict(draws), plan=plan)["seg_logits"]
    model.check_shared_geometry = True
    try:
        same = model.inference(dict(frag), eval=False, draws=dict(draws), plan=plan)["seg_logits"]  # the untouched dict passes
        assert bits_equal(same, base)
        moved = dict(frag, grid_coord=frag["grid_coord"].clone())
        moved["grid_coord"][m // 2, 2] += 1
        with pytest.raises(CdsegError, match="check_shared_geometry"):
            model.inference(moved, eval=False, draws=dict(draws), plan=plan)
    finally:
        model.check_shared_geometry = False
    with pytest.raises(CdsegError, match="points"):  # the host-side check is always on
        model.inference(dict(scene.fragments[-1]), eval=False, plan=plan)
