"""CPU: multi-step voting (MSAI / MSFI) on the emulated op layer (tests/emu_ops.py + a torch restatement of `msi_step` written
from the three emulations it replaces): the n-encoder computed once (`reuse_encoder`), the skipped last c-decoder, the
multi-step `predraw`, and the pipeline's argument checks (they run before any device work).  The HIP kernel and the lanes are
tested on the GPU (tests/test_gpu_msi.py)."""
import copy
import types

import numpy as np
import pytest
import torch

import cdsegnet_amd.engine as engine_mod
import cdsegnet_amd.models  # noqa: F401
from cdsegnet_amd.registry import build_model
from oracle import model as OM
from tests import emu_ops
from tests import msi_common as M
from tests.helpers import fixture_cfg, fixture_input, fixture_state_dict, load_fixture


def _emu_with_msi_step():
    """tests/emu_ops.py as it is, plus `msi_step`: ddim_update into c_xt, axpy(alpha 1) into acc, and for the mean the second
    axpy from zero - the three emulations the fused launch replaces, writing in place as the kernel does."""
    mod = types.ModuleType("emu_ops_msi")
    mod.__dict__.update({k: v for k, v in vars(emu_ops).items() if not k.startswith("__")})
    mod.MSI_SET, mod.MSI_ADD, mod.MSI_MEAN = 0, 1, 2
    mod.msi_calls = []

    def msi_step(c_xt=None, eps=None, sqrt_ab_prev=0.0, sqrt_1m_ab=0.0, sqrt_ab=1.0, sqrt_1m_ab_prev=0.0, final=False,
                 acc=None, logits=None, acc_mode=1, scale=1.0):
        assert acc_mode in (0, 1, 2)
        mod.msi_calls.append((eps is not None, acc is not None, acc_mode))
        if eps is not None:
            c_xt.copy_(emu_ops.ddim_update(c_xt, eps, sqrt_ab_prev, sqrt_1m_ab, sqrt_ab, sqrt_1m_ab_prev, final))
        if acc is not None:
            if acc_mode == 0:
                acc.copy_(logits)
            else:
                s = emu_ops.axpy(acc, logits, 1.0)
                acc.copy_(s if acc_mode == 1 else emu_ops.axpy(torch.zeros_like(s), s, scale))

    mod.msi_step = msi_step
    return mod


@pytest.fixture()
def emulated(monkeypatch):
    mod = _emu_with_msi_step()
    monkeypatch.setattr(engine_mod, "ops", mod)
    return mod


def _model(name="mini_ddim_avg2", precision="fp32"):
    fx = load_fixture(name + ".npz")
    cfg = copy.deepcopy(fixture_cfg(fx))
    cfg["backbone"]["enable_flash"] = False
    model = build_model(cfg)
    model.load_state_dict(fixture_state_dict(fx), strict=True)
    model.eval()
    model.precision = precision
    inp = {k: torch.as_tensor(v) for k, v in fixture_input(fx).items()}
    draws = dict(noise=torch.from_numpy(fx["noise"]), perms=[p for p in fx["perms"]])
    return fx, cfg, model, inp, draws


def _ddim(model, cfg, inp, draws, step, mode, **kw):
    d = None if draws is None else dict(draws, noise=draws["noise"].clone())
    return model.inference_ddim(dict(inp), T=cfg["T"], step=step, eval=False, mode=mode, draws=d, **kw)["seg_logits"]


# ------------------------------------------------------------------------------------------ hoist = un-hoisted under D'
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_reuse_encoder_equals_the_unhoisted_loop_under_d_prime(emulated, precision):
    """Fails without the feature: `reuse_encoder` and `msi_stats` do not exist."""
    fx, cfg, model, inp, draws = _model(precision=precision)
    step, mode = int(fx["step"]), str(fx["mode"])
    assert step == 2 and mode == "avg" and M.differs_somewhere(draws)
    eng = model.engine()
    hoisted = _ddim(model, cfg, inp, draws, step, mode, reuse_encoder=True)
    assert eng.msi_stats == dict(backbone_calls=3, n_encoders=1, c_decoders=2)
    plain = _ddim(model, cfg, inp, M.d_prime(draws), step, mode)
    assert eng.msi_stats == dict(backbone_calls=3, n_encoders=3, c_decoders=2)
    assert torch.equal(hoisted, plain)
    other = _ddim(model, cfg, inp, draws, step, mode)  # D itself is another outcome
    assert not torch.equal(other, plain)
    # step 3, MSFI, seeded draws
    d3 = M.seeded_draws(11, inp["feat"].shape[0], cfg["c_in_channels"], 4)
    assert M.differs_somewhere(d3)
    hoisted = _ddim(model, cfg, inp, d3, 3, "final", reuse_encoder=True)
    assert eng.msi_stats == dict(backbone_calls=4, n_encoders=1, c_decoders=3)
    assert torch.equal(hoisted, _ddim(model, cfg, inp, M.d_prime(d3), 3, "final"))
    assert eng.msi_stats == dict(backbone_calls=4, n_encoders=4, c_decoders=3)


def test_the_fused_glue_and_the_three_ops_give_the_same_logits(emulated, monkeypatch):
    """The last call's c-decoder and DDIM update are gone and the glue is one call per step; an op layer without `msi_step`
    (tests/emu_ops.py as it is) runs the three element-wise ops and computes the same bits."""
    fx, cfg, model, inp, draws = _model()
    a = _ddim(model, cfg, inp, draws, 2, "avg")
    # one launch per backbone call: (ddim, no sum) (ddim, sum) (no ddim, mean)
    assert emulated.msi_calls == [(True, False, 1), (True, True, 1), (False, True, 2)]
    del emulated.msi_calls[:]
    f = _ddim(model, cfg, inp, draws, 2, "final")
    assert emulated.msi_calls == [(True, False, 1), (True, False, 1)]  # nothing is left to do after the last call
    monkeypatch.setattr(engine_mod, "ops", emu_ops)
    assert torch.equal(a, _ddim(model, cfg, inp, draws, 2, "avg"))
    assert torch.equal(f, _ddim(model, cfg, inp, draws, 2, "final"))
    assert model.engine().msi_stats == dict(backbone_calls=3, n_encoders=3, c_decoders=2)


def test_single_step_inference_counts_one_encoder_and_no_c_decoder(emulated):
    fx, cfg, model, inp, draws = _model()
    model.inference(dict(inp), eval=False, draws=dict(noise=draws["noise"], perms=draws["perms"][:8]))
    assert model.engine().msi_stats == dict(backbone_calls=1, n_encoders=1, c_decoders=0)


# ------------------------------------------------------------------------------------------ hoist vs the oracle
def test_reuse_encoder_matches_the_oracle_under_d_prime(emulated):
    """The oracle's multi-step loop under D' against the engine with reuse_encoder=True under D: the bound of
    test_engine_inference_ddim (tests/test_engine_host_logic.py), 2e-5."""
    fx, cfg, model, inp, draws = _model()
    ref = OM.inference_ddim(cfg["backbone"], cfg, fixture_state_dict(fx), fixture_input(fx), M.d_prime(draws),
                            step=int(fx["step"]), mode=str(fx["mode"]), flash_semantics=False).numpy()
    out = _ddim(model, cfg, inp, draws, int(fx["step"]), str(fx["mode"]), reuse_encoder=True).numpy()
    err = float(np.abs(out - ref).max())
    print(f"[measure] emulated engine, reuse_encoder=True vs oracle under D': {err:.3e}")
    assert err < 2e-5
    assert float(np.abs(ref - fx["logits"]).max()) > 2e-5  # D' is not D: the recorded logits are another outcome


# ------------------------------------------------------------------------------------------ the generator
@pytest.mark.parametrize("noise_level", [None, 0.05])
def test_the_generator_ends_in_the_same_state_with_the_flag_on_and_off(emulated, noise_level):
    fx, cfg, model, inp, _ = _model()
    states, outs = [], []
    for flag in (False, True):
        torch.manual_seed(7)
        outs.append(model.inference_ddim(dict(inp), T=cfg["T"], step=3, eval=False, mode="avg", noise_level=noise_level,
                                         reuse_encoder=flag)["seg_logits"])
        states.append(torch.get_rng_state())
    assert torch.equal(states[0], states[1])
    assert not torch.equal(outs[0], outs[1])  # (the later calls' n-branch shuffles were drawn and ignored)
    torch.manual_seed(7)  # the same consumption as the reference's: feat noise, c noise, 8 shuffles per call
    if noise_level is not None:
        torch.randn(tuple(inp["feat"].shape))
    torch.normal(0, 1, size=(inp["feat"].shape[0], cfg["c_in_channels"]), dtype=torch.float32)
    for _ in range(8 * 4):
        torch.randperm(4)
    assert torch.equal(states[0], torch.get_rng_state())


def test_predraw_of_a_multi_step_inference(emulated):
    fx, cfg, model, inp, _ = _model()
    eng = model.engine()
    torch.manual_seed(3)
    d = eng.predraw(inp, None, n_backbone_calls=3, always_noise=True)
    state = torch.get_rng_state()
    assert len(d["perms"]) == 24 and tuple(d["noise"].shape) == (inp["feat"].shape[0], cfg["c_in_channels"])
    torch.manual_seed(3)
    noise = torch.normal(0, 1, size=tuple(d["noise"].shape), dtype=torch.float32)
    perms = [torch.randperm(4).tolist() for _ in range(24)]
    assert torch.equal(state, torch.get_rng_state())
    assert torch.equal(noise, d["noise"]) and perms == [list(p) for p in d["perms"]]
    # the predrawn draws give what the seeded call gives, and the defaults are the single-step draws
    torch.manual_seed(3)
    want = model.inference_ddim(dict(inp), T=cfg["T"], step=2, eval=False, mode="final")["seg_logits"]
    got = model.inference_ddim(dict(inp), T=cfg["T"], step=2, eval=False, mode="final", draws=d)["seg_logits"]
    assert torch.equal(want, got)
    torch.manual_seed(3)
    d1 = eng.predraw(inp)
    assert len(d1["perms"]) == 8
    # device-RNG stream ids: the window of a multi-step inference holds one id per draw of its loop
    base = eng.reserve_rng()
    d10 = eng.predraw(inp, None, n_backbone_calls=11, always_noise=True)
    assert d10["rng_base"] == base + eng.RNG_RESERVE and eng.reserve_rng() == d10["rng_base"] + 13


def test_condition_false_accepts_the_flag(emulated):
    fx = load_fixture("mini_ptv3_room.npz")
    cfg = copy.deepcopy(fixture_cfg(fx))
    cfg["backbone"]["enable_flash"] = False
    model = build_model(cfg)
    model.load_state_dict(fixture_state_dict(fx), strict=True)
    model.eval()
    model.precision = "fp32"
    inp = {k: torch.as_tensor(v) for k, v in fixture_input(fx).items()}
    draws = dict(perms=[p for p in fx["perms"]])
    a = model.inference_ddim(dict(inp), T=cfg["T"], step=2, eval=False, draws=dict(draws))["seg_logits"]
    b = model.inference_ddim(dict(inp), T=cfg["T"], step=2, eval=False, draws=dict(draws), reuse_encoder=True)["seg_logits"]
    assert torch.equal(a, b)
    assert model.engine().msi_stats == dict(backbone_calls=1, n_encoders=1, c_decoders=0)


# ------------------------------------------------------------------------------------------ the pipeline's argument checks
def test_pipeline_refuses_bad_multi_step_arguments_before_any_device_work():
    """No model, no scene, no device: the three checks come first, in `vote` and in `segment`."""
    import cdsegnet_amd.testtime as tt
    from tests import vote_shared_common as C
    tp = tt.TestPipeline(C.block_cut())
    for call in (lambda **kw: tp.vote(None, None, 16, **kw), lambda **kw: tp.segment(None, None, 16, **kw)):
        with pytest.raises(ValueError, match="inference_mode"):
            call(inference_mode="MSXI")
        with pytest.raises(ValueError, match="inference_mode"):
            call(inference_mode="msai")
        for bad in (0, -1, 1.5):
            with pytest.raises(ValueError, match="step"):
                call(inference_mode="MSAI", step=bad)
        with pytest.raises(ValueError, match="reuse_encoder"):
            call(inference_mode="SSI", reuse_encoder=True)
    model = build_model(copy.deepcopy(fixture_cfg(load_fixture("mini_ddim_avg2.npz"))))
    for bad in (0, -2):
        with pytest.raises(ValueError, match="step"):
            model.inference_ddim_many([dict()], step=bad)
    with pytest.raises(ValueError):
        model.inference_ddim_many([dict()], mode="mean")
    assert model.inference_ddim_many([]) == []
