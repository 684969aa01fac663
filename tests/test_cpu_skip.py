"""CPU: the skip-connection options - skip_connection_mode "add" / "cat_all", skip_connection_scale(_i), b_factor / s_factor
(FreeU) - at the model layer, in the restatement of the reference's Fourier filter (tests/skip_restatement.py) and in the host
logic of the inference engine and the training graph, driven on the PyTorch-CPU emulation of the op layer
(tests/emu_skip_ops.py) against the reference's recordings (tools/make_skip_golden.py).  The kernels themselves:
tests/test_gpu_skip.py."""
import warnings

import numpy as np
import pytest
import torch

import cdsegnet_amd.engine as engine_mod
import cdsegnet_amd.models as models
import cdsegnet_amd.train_graph as tg
from cdsegnet_amd import configs
from cdsegnet_amd.registry import build_model
from tests import emu_skip_ops, skip_restatement as R
from tests.helpers import fixture_input, load_fixture
from tests.skip_helpers import INFER, S, ddim_draws, fixture_model, ssi_draws, train_draws

NS = (2, 3, 4, 5, 64, 777, 3001)
SCALES = (0.9, 0.8, 1.1, 1.37)
# worst |closed form - FFT restatement| over NS x SCALES on (N, 64) features uniform in [-11, 11], measured on the CPU
# (profiles/NOTES.md, "Skip-connection options"): against the fp64 FFT with s rounded to float32 1.65e-13 (N = 777), against the
# fp32 FFT - the reference's own arithmetic - 8.37e-6 (N = 3001: the FFT's rounding, growing with N)
MEASURED_FP64, MEASURED_FP32 = 1.65e-13, 8.37e-6


@pytest.fixture()
def emulated(monkeypatch):
    monkeypatch.setattr(engine_mod, "ops", emu_skip_ops)
    monkeypatch.setattr(tg, "ops", emu_skip_ops)
    del emu_skip_ops.calls[:]


def _inp(fx):
    return {k: torch.as_tensor(v) for k, v in fixture_input(fx).items()}


def _features(n):
    g = torch.Generator().manual_seed(100 + n)
    return torch.rand(n, 64, generator=g) * 22 - 11


# ------------------------------------------------------------------------------------------ model layer
@pytest.mark.parametrize("tag", list(INFER))
def test_every_fixture_configuration_constructs(tag):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = build_model(configs.mini_config(**INFER[tag]))
        full = build_model(configs.cdsegnet_config("scannet", **INFER[tag]))
    mode = INFER[tag].get("skip_connection_mode", "cat")
    # no parameter is added: the keys are those of the same mode with every other switch at its default
    plain = build_model(configs.mini_config(skip_connection_mode=mode))
    assert list(model.state_dict()) == list(plain.state_dict())
    if mode == "cat":
        assert list(model.state_dict()) == list(build_model(configs.mini_config()).state_dict())
        assert list(full.state_dict()) == list(build_model(configs.cdsegnet_config("scannet")).state_dict())
    ups = list(engine_mod.skip_modules(model.backbone))
    assert len(ups) == 6 and [u.s for u in ups[:4]] == list(reversed(INFER[tag].get("s_factor", [1.0] * 4)))
    assert [u.b for u in ups[:4]] == list(reversed(INFER[tag].get("b_factor", [1.0] * 4)))


def test_training_configuration_constructs_and_scales():
    bb = build_model(configs.mini_config(skip_connection_mode="add", skip_connection_scale_i=True, s_factor=S)).backbone
    n_ups = [getattr(bb._n_dec, f"dec{s}").up for s in range(4)]
    assert [u.skip_connection_mode for u in n_ups] == ["add"] * 4
    assert [u.skip_scale for u in n_ups] == [0.8 ** s for s in range(4)]
    assert [u.skip_filter for u in n_ups] == [0.9, 0.8, 1.1, None]
    c_ups = [getattr(bb._c_dec, f"dec{s}").up for s in range(2)]
    # the reference's quirk: skip_connection_scale_i=False still scales by 0.8^(0-1) = 1.25 (ptv3.py:610-611)
    assert [u.skip_scale for u in c_ups] == [2 ** -0.5 * 1.25] * 2 and [u.skip_connection_mode for u in c_ups] == ["add"] * 2


def test_bad_factors_and_modes_are_value_errors():
    for bad in ("0.9", None, float("nan"), True):
        with pytest.raises(ValueError):
            models.SerializedUnpooling(32, 16, 32, s=bad)
        with pytest.raises(ValueError):
            models.SerializedUnpooling(32, 16, 32, b=bad)
    with pytest.raises(ValueError):
        configs.mini_config(skip_connection_mode="sum")
    with pytest.raises(ValueError):
        configs.mini_config(s_factor=[0.9, 0.8])
    for keep in ("enable_rpe", "tm_restomer"):  # out of scope: still rejected
        cfg = configs.mini_config()
        cfg["backbone"][keep] = True
        with pytest.raises(NotImplementedError):
            build_model(cfg)


def test_b_factor_warns_once_and_runs_no_filter(monkeypatch):
    monkeypatch.setattr(models, "_B_FACTOR_WARNED", False)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        model = build_model(configs.mini_config(b_factor=[1.2, 1.2, 1.2, 1.2]))
        build_model(configs.mini_config(b_factor=[1.2, 1.0, 1.0, 1.4]))
    msgs = [str(x.message) for x in w if "b_factor" in str(x.message)]
    assert len(msgs) == 1 and "point_transformer_v3m1_base.py:81-96" in msgs[0] and "none" in msgs[0]
    assert all(u.skip_filter is None for u in engine_mod.skip_modules(model.backbone))


# ------------------------------------------------------------------------------------------ the restatement
def test_closed_form_equals_the_fp64_fft():
    worst = 0.0
    for n in NS:
        x = _features(n)
        for s in SCALES:
            worst = max(worst, float((R.closed_filter(x, s) - R.fft_filter(x, s, torch.float64)).abs().max()))
    print(f"closed form vs fp64 FFT (s rounded to float32): worst {worst:.3g}")
    assert worst <= 10 * MEASURED_FP64
    # without the rounding of s the two differ by the rounding of s (1.37 is the worst of SCALES: 2.6e-7 measured)
    x = _features(64)
    d = float((R.closed_filter(x, 1.37, round_s=False) - R.fft_filter(x, 1.37, torch.float64)).abs().max())
    assert 1e-9 < d < 10 * 2.6e-7


def test_closed_form_equals_the_fp32_fft_of_the_reference():
    worst = 0.0
    for n in NS:
        x = _features(n)
        for s in SCALES:
            worst = max(worst, float((R.closed_filter(x, s) - R.fft_filter(x, s, torch.float32).double()).abs().max()))
    print(f"closed form vs fp32 FFT: worst {worst:.3g}")
    assert worst <= 1.5 * MEASURED_FP32


def test_filter_is_self_adjoint_and_row_maps_permute():
    g = torch.Generator().manual_seed(5)
    x, y = torch.randn(37, 8, generator=g).double(), torch.randn(37, 8, generator=g).double()
    a = (R.closed_filter(x, 0.8) * y).sum()
    b = (x * R.closed_filter(y, 0.8)).sum()
    assert abs(float(a - b)) < 1e-12 * abs(float(a))
    perm = torch.randperm(37, generator=g)  # physical row r holds reference row perm[r]
    want = R.closed_filter(x, 0.8)
    have = R.closed_filter(x[perm], 0.8, ref=perm)
    assert float((have - want[perm]).abs().max()) < 1e-13


# ------------------------------------------------------------------------------------------ host logic, inference
EXPECT = {  # tag -> the calls of one single-step inference (n-decoder stages 3, 2, 1, 0; the c-decoder is not run)
    "add_scale": [],
    "cat_scale_i": ["skip_merge"] * 3,  # stage 0 has f = 0.8^0 = 1: the one-GEMM path
    "cat_all_s": ["skip_stats", "skip_fold", "skip_merge"] * 3,  # stage 3 has s = 1
    "cat_s_b_batch2": ["skip_stats", "skip_merge"] * 3,
    "b_only": [],
}


@pytest.mark.parametrize("tag", list(INFER))
def test_engine_host_logic_vs_the_reference(emulated, tag):
    fx = load_fixture(f"skip_infer_{tag}.npz")
    model, cfg = fixture_model(fx)
    model.precision = "fp32"
    out = model.inference(_inp(fx), eval=False, draws=ssi_draws(fx))["seg_logits"].numpy()
    calls = list(emu_skip_ops.calls)
    plan = model.engine().last_plan
    assert [c[0] for c in calls] == EXPECT[tag]
    assert np.abs(out - fx["logits"]).max() < 2e-4  # (the bounds of tests/test_engine_host_logic.py)
    out = model.inference_ddim(_inp(fx), T=cfg["T"], step=2, eval=False, mode="avg", draws=ddim_draws(fx))["seg_logits"].numpy()
    assert np.abs(out - fx["ddim_logits"]).max() < 2e-5
    if tag == "add_scale":  # two c-decoders of two 'add' stages each, f = 2^-0.5 * 1.25, no filter
        extra = emu_skip_ops.calls[len(calls):]
        assert [c[0] for c in extra] == ["skip_merge"] * 4
        assert all(abs(c[1]["f"] - 2 ** -0.5 * 1.25) < 1e-15 and not c[1]["stats"] and c[1]["child"] for c in extra)
    n0 = plan.levels[0].n
    for name, d in calls:
        # N is the row count of the whole (collated) batch at that level, the row map at level 0 is the plan's perm0
        if name != "skip_fold" and d.get("stats", True) and d["n"] == n0:
            assert d["n_total"] == n0 and d["ref"] is plan.perm0
        if name == "skip_merge":
            assert d["folded"] == (tag == "cat_all_s") and d["child"] == (tag != "cat_all_s")


def test_row_map_above_level_0_is_the_rank_on_the_pooling_curve(emulated, monkeypatch):
    fx = load_fixture("skip_infer_cat_s_b_batch2.npz")
    model, _ = fixture_model(fx)
    model.precision = "fp32"
    seen = []
    real = engine_mod.Engine._skip_ref

    def spy(self, plan, parent):
        ref = real(self, plan, parent)
        seen.append((parent, ref))
        return ref

    monkeypatch.setattr(engine_mod.Engine, "_skip_ref", spy)
    model.inference(_inp(fx), eval=False, draws=ssi_draws(fx))
    assert len(seen) == 3
    for parent, ref in seen:
        if parent.parent is None:
            continue
        order = parent.level.order(parent.parent.curves[0])  # rank -> physical row, under the curve that pooled the level
        if order is None:
            assert ref is None
        else:
            assert torch.equal(ref.long()[order.long()], torch.arange(parent.level.n))


def test_default_model_calls_no_new_entry_point(emulated):
    fx = load_fixture("skip_infer_b_only.npz")
    model, cfg = fixture_model(fx, b_factor=[1.0] * 4)
    model.precision = "fp32"
    a = model.inference(_inp(fx), eval=False, draws=ssi_draws(fx))["seg_logits"]
    model.inference_ddim(_inp(fx), T=cfg["T"], step=2, eval=False, mode="avg", draws=ddim_draws(fx))
    assert emu_skip_ops.calls == []
    # ... and b_factor alone changes nothing: the same bits
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        bmodel, _ = fixture_model(fx)
    bmodel.precision = "fp32"
    b = bmodel.inference(_inp(fx), eval=False, draws=ssi_draws(fx))["seg_logits"]
    assert torch.equal(a, b) and emu_skip_ops.calls == []


def test_per_fragment_draws_on_a_filtering_model_raise_before_any_work(emulated, monkeypatch):
    fx = load_fixture("skip_infer_cat_s_b_batch2.npz")
    model, _ = fixture_model(fx)
    model.precision = "fp32"
    model.inference(_inp(fx), eval=False, draws=ssi_draws(fx))  # (builds the engine)
    eng = model.engine()
    monkeypatch.setattr(eng, "prepare", lambda dev: pytest.fail("device work before the check"))
    d = ssi_draws(fx)
    d["perms"] = [[p, p] for p in d["perms"]]  # one permutation per batch element
    inp = dict(_inp(fx), shared_geometry=True)
    with pytest.raises(ValueError, match="per-fragment"):
        eng._setup(inp, None, d, 1)
    # a model that only scales takes per-fragment draws as before
    fx2 = load_fixture("skip_infer_cat_scale_i.npz")
    m2, _ = fixture_model(fx2)
    assert not any(u.skip_filter is not None for u in engine_mod.skip_modules(m2.backbone))


# ------------------------------------------------------------------------------------------ host logic, training
def _train_inp(fx):
    return {k: torch.as_tensor(fx[k]) for k in ("coord", "grid_coord", "feat", "offset", "segment")}


def test_training_step_on_the_emulated_ops_vs_the_reference(emulated):
    fx = load_fixture("skip_train_step.npz")
    model, _ = fixture_model(fx, train=True)
    out = model(_train_inp(fx), draws=train_draws(fx))
    assert abs(float(out["loss"].detach()) - float(fx["loss"])) < 2e-5
    assert float((out["n_pred"].detach() - torch.as_tensor(fx["n_pred"])).abs().max()) < 1e-4
    assert float((out["c_pred"].detach() - torch.as_tensor(fx["c_pred"])).abs().max()) < 1e-4
    out["loss"].backward()
    named = dict(model.named_parameters())
    names = [str(n) for n in fx["grad_names"]]
    assert names == list(named)
    gn = np.array([float(named[k].grad.norm()) if named[k].grad is not None else -1.0 for k in names])
    ref = fx["grad_norms"]
    assert (gn >= 0).all()
    assert (np.abs(gn - ref) <= 1e-3 * ref + 1e-5 * ref.max()).all()
    checked = 0
    for k in fx.files:
        if k.startswith("g."):
            r = fx[k]
            assert float((named[k[2:]].grad - torch.as_tensor(r)).abs().max()) <= 1e-3 * float(np.abs(r).max()), k
            checked += 1
    assert checked == 10


def test_training_forward_with_the_filter_vs_the_reference_and_its_backward(emulated):
    """The reference cannot differentiate through freeU (an in-place write, ptv3.py:96): its training-mode forward is the
    recording, the backward is held to autograd on the fp64 closed form."""
    fx = load_fixture("skip_train_fwd_s.npz")
    model, _ = fixture_model(fx, train=True)
    out = model(_train_inp(fx), draws=train_draws(fx))
    assert abs(float(out["loss"].detach()) - float(fx["loss"])) < 2e-5
    assert float((out["n_pred"].detach() - torch.as_tensor(fx["n_pred"])).abs().max()) < 1e-4
    assert float((out["c_pred"].detach() - torch.as_tensor(fx["c_pred"])).abs().max()) < 1e-4
    stats_calls = [c for c in emu_skip_ops.calls if c[0] == "skip_stats"]
    assert len(stats_calls) == 3  # stages 2, 1, 0 (s = 1.1, 0.8, 0.9); stage 3 has s = 1
    out["loss"].backward()
    assert len([c for c in emu_skip_ops.calls if c[0] == "skip_stats"]) == 6  # the backward is the same pair of calls
    g = torch.Generator().manual_seed(9)
    x = torch.randn(41, 16, generator=g, requires_grad=True)
    dy = torch.randn(41, 16, generator=g)
    ref = torch.randperm(41, generator=g).to(torch.int32)
    tg._SkipFilter.apply(x, ref, 0.8).backward(dy)
    x64 = x.detach().double().requires_grad_(True)
    (R.closed_filter(x64, 0.8, ref=ref) * dy.double()).sum().backward()
    assert float((x.grad.double() - x64.grad).abs().max()) < 1e-6


def test_folded_mix3d_batch_on_a_filtering_model_raises(emulated):
    fx = load_fixture("train_step_mix3d.npz")
    cfg = configs.mini_config(s_factor=S)
    cfg["backbone"]["enable_flash"] = False
    model = build_model(cfg).train()
    inp = {k: torch.as_tensor(fx[k]) for k in ("coord", "grid_coord", "feat", "offset", "segment")}
    model.train_mix3d = "fold"
    with pytest.raises(ValueError, match="fold"):
        model(inp)
