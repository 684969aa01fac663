"""GPU: multi-step voting (MSAI / MSFI) - cdseg_msi_step against the three kernels it replaces, the n-encoder computed once
(`reuse_encoder`) against the un-hoisted loop under the draws D' and against the CPU oracle, `inference_ddim_many` against the
sequential calls, and TestPipeline.vote(inference_mode=...) against a hand loop.  The host logic is tested on the CPU
(tests/test_cpu_msi.py)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from tests import msi_common as M
from tests import vote_shared_common as C
from tests.helpers import fixture_cfg, fixture_input, fixture_state_dict, load_fixture, tiny_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from cdsegnet_amd import ops as _ops
    assert torch.cuda.is_available()
    return _ops


def dev(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x)
    return (t if dtype is None else t.to(dtype)).cuda().contiguous()


def to_dev(inp):
    return {k: torch.as_tensor(v).cuda() for k, v in inp.items()}


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ cdseg_msi_step
COEF = (0.9712, 0.3187, 0.9479, 0.2383)  # sqrt(ab_prev), sqrt(1 - ab), sqrt(ab), sqrt(1 - ab_prev) of some cosine step


def _kernel_case(ops, n, c, first_row):
    """Every combination of the two halves on (n, 6) / (n, c) arrays that start at row `first_row` of a larger allocation
    (row 1: 24 / 4c bytes into it - the 6-channel pair then sits 8 bytes off a 16-byte boundary)."""
    g = torch.Generator().manual_seed(100 * n + c)
    rows = n + first_row

    def arr(cols):
        return torch.randn((rows, cols), generator=g).cuda()[first_row:]

    xt, eps, acc0, logits = arr(6), arr(6), arr(c), arr(c)
    assert xt.is_contiguous() and (xt.data_ptr() % 16 == 8) == (first_row == 1)
    scale = float(1.0 / 3)
    for final in (False, True):
        want_x = ops.ddim_update(xt, eps, *COEF, final=final)
        for mode in (ops.MSI_SET, ops.MSI_ADD, ops.MSI_MEAN):
            s = ops.axpy(acc0, logits, 1.0)
            want_a = {ops.MSI_SET: logits, ops.MSI_ADD: s, ops.MSI_MEAN: ops.axpy(torch.zeros_like(s), s, scale)}[mode]
            x, a = xt.clone(), acc0.clone()  # (clones of a slice start on an allocation boundary: the aligned layout)
            if first_row:
                x, a = arr(6), arr(c)
                x.copy_(xt), a.copy_(acc0)
            ops.msi_step(x, eps, *COEF, final=final, acc=a, logits=logits, acc_mode=mode, scale=scale)
            assert bits_equal(x, want_x) and bits_equal(a, want_a), (n, c, first_row, final, mode)
            # each NULL half leaves the other array alone
            x2, a2 = x.clone(), acc0.clone()
            ops.msi_step(None, None, acc=a2, logits=logits, acc_mode=mode, scale=scale)
            assert bits_equal(a2, want_a) and bits_equal(x2, x)
        x3, a3 = xt.clone(), acc0.clone()
        ops.msi_step(x3, eps, *COEF, final=final)
        assert bits_equal(x3, want_x) and bits_equal(a3, acc0)
    # the two arrays of a pair at different offsets from a 16-byte boundary: the scalar path
    if first_row:
        x4 = arr(6)
        x4.copy_(xt)
        e4, l4, a4 = eps.clone(), logits.clone(), arr(c)
        a4.copy_(acc0)
        ops.msi_step(x4, e4, *COEF, final=False, acc=a4, logits=l4, acc_mode=ops.MSI_ADD)
        assert bits_equal(x4, ops.ddim_update(xt, eps, *COEF, final=False)) and bits_equal(a4, ops.axpy(acc0, logits, 1.0))
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", [13, 16, 20, 200])
@pytest.mark.parametrize("n", [1, 3, 257, 2599])
def test_msi_step_equals_the_three_kernels_bit_for_bit(ops, n, c):
    """Fails without the feature: the entry point does not exist.  Head-only sizes (n = 1: 6 and 13 floats), sizes that are no
    multiple of four, more than one block (2599 x 200 / 4 groups), both halves in one grid."""
    _kernel_case(ops, n, c, 0)
    _kernel_case(ops, n, c, 1)


def test_msi_step_refuses_before_any_launch(ops):
    """CDSEG_ERR_ARG for a negative count, a NULL array with a positive count and an unknown acc_mode; the buffers keep their
    sentinel."""
    from cdsegnet_amd import _lib
    lib = _lib.load()
    n = 300
    bufs = [torch.full((n,), -7.0, dtype=torch.float32, device="cuda") for _ in range(4)]
    x, e, a, l = (ctypes.c_void_p(b.data_ptr()) for b in bufs)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    null = ctypes.c_void_p(None)

    def call(c_xt=x, eps=e, n_c=n, acc=a, logits=l, n_l=n, mode=1):
        return lib.cdseg_msi_step(c_xt, eps, n_c, 0.9, 0.3, 0.95, 0.2, 0, acc, logits, n_l, mode, 0.5, st)

    assert call(n_c=-1) == -1 and call(n_l=-1) == -1
    assert call(c_xt=null) == -1 and call(logits=null) == -1
    assert call(mode=3) == -1 and call(mode=-1) == -1
    assert call(eps=null, acc=null) == 0  # nothing to do is no error
    assert call(n_c=0, n_l=0) == 0
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b == -7.0).all())
    with pytest.raises(ValueError, match="msi_step"):
        ops.msi_step(bufs[0], bufs[1][:10])
    with pytest.raises(ValueError, match="msi_step"):
        ops.msi_step(bufs[0].double(), bufs[1].double())


# ------------------------------------------------------------------------------------------------ the mini room model
def _build(precision):
    import cdsegnet_amd.models  # noqa: F401
    from cdsegnet_amd.registry import build_model
    fx = load_fixture("mini_ddim_avg2.npz")
    cfg = copy.deepcopy(fixture_cfg(fx))
    cfg["backbone"]["enable_flash"] = False
    model = build_model(cfg)
    model.load_state_dict(fixture_state_dict(fx), strict=True)
    model = model.cuda().eval()
    model.precision = precision
    return fx, cfg, model


def _ddim(model, cfg, inp, draws, step, mode, **kw):
    d = None if draws is None else dict(draws)
    out = model.inference_ddim(dict(inp), T=cfg["T"], step=step, eval=False, mode=mode, draws=d, **kw)["seg_logits"]
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("precision", ["fp32", "fp16", "bf16", "fp32x3", "fp16+head", "bf16+head"])
def test_reuse_encoder_equals_the_unhoisted_loop_under_d_prime(precision):
    """mini_ddim_avg2 (step 2, MSAI, its recorded draws) and a step-3 MSFI run under seeded draws: the n-encoder computed once
    gives, bit for bit, what the loop that recomputes it gives when every later call repeats the first call's n-branch
    shuffles - and counts one n-encoder where that loop counts one per backbone call."""
    fx, cfg, model = _build(precision)
    inp = to_dev(fixture_input(fx))
    eng = model.engine()
    draws = dict(noise=torch.from_numpy(fx["noise"]), perms=[p for p in fx["perms"]])
    d3 = M.seeded_draws(11, inp["feat"].shape[0], cfg["c_in_channels"], 4)
    assert M.differs_somewhere(draws) and M.differs_somewhere(d3)
    for d, step, mode in ((draws, int(fx["step"]), str(fx["mode"])), (d3, 3, "final")):
        calls = step + 1
        hoisted = _ddim(model, cfg, inp, d, step, mode, reuse_encoder=True)
        assert eng.msi_stats == dict(backbone_calls=calls, n_encoders=1, c_decoders=calls - 1)
        plain = _ddim(model, cfg, inp, M.d_prime(d), step, mode)
        assert eng.msi_stats == dict(backbone_calls=calls, n_encoders=calls, c_decoders=calls - 1)
        assert bits_equal(hoisted, plain), (precision, step, mode)
        assert not bits_equal(_ddim(model, cfg, inp, d, step, mode), plain)  # D is another outcome
        plan = model.plan(inp)  # ... and on a plan that outlives the call
        assert bits_equal(_ddim(model, cfg, inp, d, step, mode, reuse_encoder=True, plan=plan), plain)
        del plan


def test_reuse_encoder_matches_the_oracle_under_d_prime():
    """oracle.model.inference_ddim on mini_ddim_avg2's input under D' against the device with reuse_encoder=True, fp32: the
    bound of test_inference_ddim_matches_reference_golden, 5e-5 (the recorded draws measure 1.1e-6 to 1.3e-6 there)."""
    from oracle import model as OM
    fx, cfg, model = _build("fp32")
    draws = dict(noise=torch.from_numpy(fx["noise"]), perms=[p for p in fx["perms"]])
    ref = OM.inference_ddim(cfg["backbone"], cfg, fixture_state_dict(fx), fixture_input(fx), M.d_prime(draws),
                            step=int(fx["step"]), mode=str(fx["mode"]), flash_semantics=False).numpy()
    out = _ddim(model, cfg, to_dev(fixture_input(fx)), draws, int(fx["step"]), str(fx["mode"]), reuse_encoder=True)
    err = float(np.abs(out.cpu().numpy() - ref).max())
    print(f"[measure] reuse_encoder=True vs oracle under D': max_abs_err={err:.3e}")
    assert err < 5e-5


@pytest.mark.parametrize("noise_source", ["torch_cpu", "device"])
def test_the_generator_ends_in_the_same_state_with_the_flag_on_and_off(noise_source):
    fx, cfg, model = _build("fp32")
    model.noise_source = noise_source
    inp = to_dev(fixture_input(fx))
    states = []
    for flag in (False, True):
        torch.manual_seed(7)
        model.inference_ddim(dict(inp), T=cfg["T"], step=3, eval=False, mode="avg", noise_level=0.05, reuse_encoder=flag)
        states.append(torch.get_rng_state())
    torch.cuda.synchronize()
    assert torch.equal(states[0], states[1])


# ------------------------------------------------------------------------------------------------ inference_ddim_many
def test_inference_ddim_many_equals_the_sequential_calls_bit_for_bit():
    """Four scenes (the fixture's room and three degenerate ones) under predrawn draws, on one and on three lanes, with and
    without the hoisted encoder; with plans= no call builds a plan."""
    fx, cfg, model = _build("fp32")
    eng = model.engine()
    dicts = [to_dev(fixture_input(fx))] + [to_dev(tiny_inputs(k)) for k in ("small", "seven_and_many", "collapses_early")]
    for d in dicts:
        d["offset_host"] = [int(v) for v in d["offset"].cpu()]
    step = 2
    draws = [M.seeded_draws(40 + i, d["feat"].shape[0], cfg["c_in_channels"], step + 1) for i, d in enumerate(dicts)]
    for mode, reuse in (("avg", False), ("final", True)):
        want = [_ddim(model, cfg, d, dr, step, mode, reuse_encoder=reuse) for d, dr in zip(dicts, draws)]
        for lanes in (1, 3):
            outs = model.inference_ddim_many([dict(d) for d in dicts], step=step, mode=mode, lanes=lanes,
                                             draws=[dict(dr) for dr in draws], reuse_encoder=reuse)
            torch.cuda.synchronize()
            for i, (o, w) in enumerate(zip(outs, want)):
                assert bits_equal(o["seg_logits"], w), (mode, lanes, i)
        plans = [model.plan(d) for d in dicts]
        before = eng.plans_built
        outs = model.inference_ddim_many([dict(d) for d in dicts], step=step, mode=mode, lanes=3,
                                         draws=[dict(dr) for dr in draws], plans=plans, reuse_encoder=reuse)
        torch.cuda.synchronize()
        assert eng.plans_built == before
        for i, (o, w) in enumerate(zip(outs, want)):
            assert bits_equal(o["seg_logits"], w), (mode, "plans", i)
        del plans
    # without injected draws: taken up front in scene order, so a seed gives what the sequential calls give
    torch.manual_seed(21)
    want = [_ddim(model, cfg, d, None, step, "avg") for d in dicts]
    state = torch.get_rng_state()
    torch.manual_seed(21)
    outs = model.inference_ddim_many([dict(d) for d in dicts], step=step, mode="avg", lanes=3)
    torch.cuda.synchronize()
    assert torch.equal(state, torch.get_rng_state())
    for i, (o, w) in enumerate(zip(outs, want)):
        assert bits_equal(o["seg_logits"], w), i


# ------------------------------------------------------------------------------------------------ the pipeline
@pytest.fixture(scope="module")
def world():
    """The mini LiDAR model on the GPU, the three-list nuScenes pipeline and the prepared 2599-point sweep (as
    tests/test_gpu_vote_shared.py builds them)."""
    from cdsegnet_amd import testtime as tt
    fx = load_fixture("testtime_nuscenes.npz")
    model, cfg, sd = C.mini_model("cuda")
    tp = tt.TestPipeline(C.block_cut())
    raw = dict(coord=dev(fx["coord"]), strength=dev(fx["strength"]), segment=dev(fx["segment"]))
    scene = tp.prepare(raw, draws={"1.r": fx["1.r"]})
    torch.cuda.synchronize()
    assert len(scene.augs) == 3 and len(fx["coord"]) == 2599
    return dict(model=model, cfg=cfg, sd=sd, tp=tp, scene=scene, k=cfg["num_classes"], ch=cfg["c_in_channels"])


def test_vote_msai_equals_a_hand_loop_bit_for_bit(world, ops):
    model, cfg, scene, tp, k = world["model"], world["cfg"], world["scene"], world["tp"], world["k"]
    eng = model.engine()
    torch.manual_seed(5)
    pred = torch.zeros((scene.n, k), dtype=torch.float32, device="cuda")
    for d in scene.fragments:
        o = model.inference_ddim(dict(d), T=cfg["T"], step=2, eval=False, mode="avg")["seg_logits"]
        ops.softmax_vote(o, d["index"], pred)
    labels = ops.argmax_rows(pred)
    if scene.inverse is not None:
        labels = ops.gather_i32(labels, scene.inverse)
    state = torch.get_rng_state()
    torch.manual_seed(5)
    before = eng.plans_built
    labels1, pred1 = tp.vote(model, scene, k, inference_mode="MSAI", step=2, lanes=1)
    assert eng.plans_built - before == len(scene.fragments) > 3
    assert torch.equal(state, torch.get_rng_state())
    torch.cuda.synchronize()
    assert bits_equal(pred1, pred) and torch.equal(labels1, labels)
    torch.manual_seed(5)  # lanes: the draws are taken up front in fragment order
    labels4, pred4 = tp.vote(model, scene, k, inference_mode="MSAI", step=2)
    assert bits_equal(pred4, pred) and torch.equal(labels4, labels)
    torch.manual_seed(5)  # one plan per augmentation, whatever the number of steps
    before = eng.plans_built
    labels2, pred2 = tp.vote(model, scene, k, inference_mode="MSAI", step=2, lanes=1, share_plan=True)
    assert eng.plans_built - before == 3
    torch.cuda.synchronize()
    assert bits_equal(pred2, pred) and torch.equal(labels2, labels)
    torch.manual_seed(5)  # the hoisted encoder votes something else under the same seed, from the same generator state
    labels3, pred3 = tp.vote(model, scene, k, inference_mode="MSAI", step=2, share_plan=True, reuse_encoder=True)
    assert torch.equal(state, torch.get_rng_state()) and eng.msi_stats == dict(backbone_calls=3, n_encoders=1, c_decoders=2)
    assert not bits_equal(pred3, pred)


def test_vote_ssi_is_the_default_path_and_bad_arguments_raise(world):
    model, scene, tp, k = world["model"], world["scene"], world["tp"], world["k"]
    torch.manual_seed(6)
    labels0, pred0 = tp.vote(model, scene, k)
    torch.manual_seed(6)
    labels1, pred1 = tp.vote(model, scene, k, inference_mode="SSI")
    torch.cuda.synchronize()
    assert bits_equal(pred0, pred1) and torch.equal(labels0, labels1)
    with pytest.raises(ValueError, match="inference_mode"):
        tp.vote(model, scene, k, inference_mode="MSXI")
    with pytest.raises(ValueError, match="step"):
        tp.vote(model, scene, k, inference_mode="MSFI", step=0)
    with pytest.raises(ValueError, match="reuse_encoder"):
        tp.vote(model, scene, k, reuse_encoder=True)


def test_a_faithful_batch_of_three_fragments_runs_three_oracle_msfi_loops(world):
    """One augmentation, fragment_batch = 3, fragment_draws = "fragment", share_plan, MSFI with one step, fp32: every
    fragment's rows of the collated logits, and the fragment's own inference_ddim under its own draws, against the oracle's
    inference_ddim of that fragment - the suite's fp32 bound (max |logit - oracle| < 1e-3, arg-max agreement > 99.9 %), as
    test_a_batch_of_three_fragments_under_their_own_draws_equals_three_oracle_forwards holds SSI to.  The draws are the
    pipeline's own: predraw_fragments under a seed, which equal three multi-step predraws in fragment order.
    max |batched - single| is printed, not bounded."""
    from oracle import model as OM
    model, cfg, sd, scene, ch = world["model"], world["cfg"], world["sd"], world["scene"], world["ch"]
    assert model.precision == "fp32"
    eng = model.engine()
    a, g = 1, scene.augs[1]
    f0, m = g["first"], g["num_voxels"]
    d3 = scene.collated(a, 0, 3)
    torch.manual_seed(8)
    gd = eng.predraw_fragments(d3, None, 2, always_noise=True)
    state = torch.get_rng_state()
    torch.manual_seed(8)
    singles = [eng.predraw(scene.fragments[f0 + j], None, 2, always_noise=True) for j in range(3)]
    assert torch.equal(state, torch.get_rng_state())
    assert len(gd["perms"]) == 16 and torch.equal(gd["noise"], torch.cat([s["noise"] for s in singles], 0))
    for p in range(16):
        assert [list(q) for q in gd["perms"][p]] == [list(s["perms"][p]) for s in singles]
    assert any(len({tuple(q) for q in gd["perms"][p]}) >= 2 for p in range(16))
    # the pipeline's route: one collated multi-step forward on the augmentation's plan
    plan = model.plan(d3)
    before = eng.plans_built
    out = model.inference_ddim_many([dict(d3)], step=1, mode="final", draws=[dict(gd)], plans=[plan])[0]["seg_logits"]
    torch.cuda.synchronize()
    assert eng.plans_built == before
    out = out.cpu().numpy()
    worst = 0.0
    for j in range(3):
        d = scene.fragments[f0 + j]
        inp = dict(coord=d["coord"].cpu().numpy(), grid_coord=d["grid_coord"].cpu().numpy(), feat=d["feat"].cpu().numpy(),
                   offset=np.array([m], dtype=np.int64))
        od = dict(noise=singles[j]["noise"], perms=[np.asarray(p) for p in singles[j]["perms"]])
        ref = OM.inference_ddim(cfg["backbone"], cfg, sd, inp, od, step=1, mode="final").numpy()
        single = model.inference_ddim(dict(d), T=cfg["T"], step=1, eval=False, mode="final",
                                      draws=dict(singles[j]))["seg_logits"].cpu().numpy()
        got = out[j * m:(j + 1) * m]
        err_b, err_s = float(np.abs(got - ref).max()), float(np.abs(single - ref).max())
        agree_b = float((got.argmax(1) == ref.argmax(1)).mean())
        agree_s = float((single.argmax(1) == ref.argmax(1)).mean())
        worst = max(worst, float(np.abs(got - single).max()))
        print(f"[measure] fragment {j}: batched vs oracle {err_b:.3e} (arg-max {agree_b:.4f}), single vs oracle {err_s:.3e} "
              f"(arg-max {agree_s:.4f}), batched vs single {float(np.abs(got - single).max()):.3e}")
        assert err_b < 1e-3 and agree_b > 0.999, (j, err_b, agree_b)
        assert err_s < 1e-3 and agree_s > 0.999, (j, err_s, agree_s)
    del plan
    print(f"[measure] max |batched - single| over 3 fragments = {worst:.3e}")
    # ... and vote() takes that route: the same seed, the first group's votes
    torch.manual_seed(8)
    before = eng.plans_built
    tp = world["tp"]
    one = copy.copy(scene)
    one.augs = [dict(g, first=0, num_fragments=3, index=g["index"][:3], coord=g["coord"][:3], grid_coord=g["grid_coord"][:3],
                     feat=g["feat"][:3])]
    one.fragments = scene.fragments[f0:f0 + 3]
    _, pred = tp.vote(model, one, world["k"], fragment_batch=3, share_plan=True, fragment_draws="fragment",
                      inference_mode="MSFI", step=1)
    assert eng.plans_built - before == 1
    from cdsegnet_amd import ops as _ops
    want = torch.zeros_like(pred)
    _ops.softmax_vote_fragments(torch.as_tensor(out).cuda(), d3["index"], want)
    torch.cuda.synchronize()
    assert bits_equal(pred, want)
