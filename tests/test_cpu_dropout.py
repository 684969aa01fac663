"""CPU: attention and projection dropout (`attn_drop`, `proj_drop`) - the mask restatement (tests/dropout_mask.py) against the
Philox stream and against the rate, the constructor plumbing, and the training graph on the emulated op layer
(tests/emu_dropout_ops.py, held to `cdsegnet_amd.ops` by signature here)."""
import threading
import warnings

import numpy as np
import pytest
import torch

import cdsegnet_amd.engine as engine
import cdsegnet_amd.models as models
import cdsegnet_amd.train_graph as tg
from cdsegnet_amd import configs, ops, synth
from cdsegnet_amd.param_init import fill_state_dict
from cdsegnet_amd.registry import build_model
from oracle import philox
from tests import dropout_mask as DM
from tests import emu_dropout_ops
from tests.test_cpu_emu_signatures import emulated_constants, emulated_functions, signature_difference

SEED, OFFSET = 0xFEDC_BA98_7654_3210, 0x0123_4567_89AB_CDEF


# ------------------------------------------------------------------------------------------ the restatement
def _byte(seed, offset, t_lo, t_hi, word, byte):
    """One byte of W(t) of include/cdseg.h, straight from oracle/philox.py."""
    ctr = np.array([t_lo, t_hi, offset & 0xFFFFFFFF, offset >> 32], dtype=np.uint32)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)
    w = int(philox.philox4x32_10(ctr, key)[word])
    return (w >> (8 * byte)) & 255


@pytest.mark.parametrize("p,h,i,j", [(0, 0, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (0, 1, 5, 6), (2, 1, 3, 4), (2, 0, 4, 3),
                                     (1, 31, 1023, 1023), (1, 31, 1023, 0), (1, 31, 0, 1023), (7, 3, 517, 258)])
def test_attention_mask_takes_the_bytes_the_header_names(p, h, i, j):
    t_lo = (j >> 2) | ((i >> 2) << 8) | (h << 16)
    want = _byte(SEED, OFFSET, t_lo, p, i & 3, j & 3)
    lens = [4] * p + [max(i, j) + 1]  # (patch p of the launch)
    got = DM.attention_bytes(SEED, OFFSET, lens[p], p, h)[i, j]
    assert int(got) == want
    assert DM.attention_site(p, h, i, j) == (t_lo, p, i & 3, j & 3)
    for rate in (0.1, 0.5):
        T = DM.threshold(rate)
        if h < 32 and lens[p] <= 64:
            assert bool(DM.attention_mask(SEED, OFFSET, rate, lens, h + 1)[p][h][i, j]) == (want < T)
        else:
            assert bool(got < T) == (want < T)


@pytest.mark.parametrize("r,c", [(0, 0), (0, 15), (0, 16), (3, 5), (999, 199), (512, 2047)])
def test_element_mask_takes_the_bytes_the_header_names(r, c):
    want = _byte(SEED, OFFSET, c >> 4, r, (c >> 2) & 3, c & 3)
    assert DM.element_site(r, c) == (c >> 4, r, (c >> 2) & 3, c & 3)
    for rate in (0.1, 0.5):
        assert bool(DM.element_mask(SEED, OFFSET, rate, r + 1, c + 1)[r, c]) == (want < DM.threshold(rate))


def test_thresholds():
    assert [DM.threshold(r) for r in (0.0, 0.1, 0.25, 0.5, 1.0 / 1024, 1.0 / 256, 0.999)] == [256, 230, 192, 128, 256, 255, 1]
    for r in (0.0, 0.1, 0.25, 0.5, 0.73, 0.999):
        assert ops.dropout_keep(r) == DM.keep_prob(r) == emu_dropout_ops.dropout_keep(r)
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(Exception, match="rate"):
            ops.dropout_keep(bad)


@pytest.mark.parametrize("rate", [0.1, 0.25, 0.5])
def test_kept_fraction_is_the_effective_keep_probability(rate):
    """>= 2^20 elements of each mask: within 5 standard deviations sqrt(k (1 - k) / n) of dropout_keep(rate)."""
    k = ops.dropout_keep(rate)
    att = DM.attention_mask(SEED, OFFSET, rate, [1024], 1)[0]
    ele = DM.element_mask(SEED, OFFSET, rate, 1024, 1024)
    for what, m in (("attention", att), ("element", ele)):
        n = m.size
        assert n >= 2 ** 20
        assert abs(float(m.mean()) - k) <= 5 * np.sqrt(k * (1 - k) / n), (what, float(m.mean()), k)
    assert not np.array_equal(att[0], ele)  # (two layouts, not one)


# ------------------------------------------------------------------------------------------ the emulation follows ops
@pytest.mark.parametrize("name", sorted(emulated_functions("emu_dropout_ops")))
def test_emulated_dropout_op_has_the_signature_of_the_real_op(name):
    import types
    real = getattr(ops, name, None)
    assert isinstance(real, types.FunctionType), f"cdsegnet_amd.ops has no function {name}"
    diff = signature_difference(emulated_functions("emu_dropout_ops")[name], real)
    assert diff is None, f"tests/emu_dropout_ops.py {name}: {diff}"


def test_the_emulation_defines_the_new_ops():
    assert set(emulated_functions("emu_dropout_ops")) == {"attention_drop", "attention_drop_bwd", "dropout", "dropout_keep"}
    assert not emulated_constants("emu_dropout_ops")


# ------------------------------------------------------------------------------------------ construction
DROP_MODULES = (models.SerializedAttention, models.SerializedCrossAttention, models.Block, models.CrossBlock, models.TransferModule,
                models.PointTransformerV3)


def _rates_of(model):
    found = {}
    for name, m in model.named_modules():
        if isinstance(m, DROP_MODULES):
            found.setdefault(type(m).__name__, []).append((m.attn_drop, m.proj_drop))
    return found


@pytest.mark.parametrize("which", ["mini", "scannet"])
def test_rates_reach_every_module(which):
    cfg = configs.mini_config() if which == "mini" else configs.model_config("scannet")
    base = build_model(cfg)
    assert all(r == (0.0, 0.0) for rs in _rates_of(base).values() for r in rs)
    cfg["backbone"]["attn_drop"], cfg["backbone"]["proj_drop"] = 0.1, 0.25
    model = build_model(cfg)
    found = _rates_of(model)
    assert set(found) == {c.__name__ for c in DROP_MODULES}, set(found)
    for cls, rs in found.items():
        assert all(r == (0.1, 0.25) and type(r[0]) is float and type(r[1]) is float for r in rs), (cls, rs)
    nblocks = sum(isinstance(m, (models.Block, models.CrossBlock)) for m in model.modules())
    assert len(found["Block"]) + len(found["CrossBlock"]) == nblocks
    assert len(found["SerializedAttention"]) == len(found["Block"])
    # no parameter, no buffer: the schema is the rate-0 model's
    assert list(model.state_dict()) == list(base.state_dict())
    assert sum(p.numel() for p in model.parameters()) == sum(p.numel() for p in base.parameters())
    assert [k for k, _ in model.named_buffers()] == [k for k, _ in base.named_buffers()]


@pytest.mark.parametrize("key", ["attn_drop", "proj_drop"])
@pytest.mark.parametrize("bad", [-0.1, 1.0, 1.5, float("nan"), "0.1", None, True, 0.5j])
def test_bad_rates_raise_value_error(key, bad):
    cfg = configs.mini_config()
    cfg["backbone"][key] = bad
    with pytest.raises(ValueError, match=key):
        build_model(cfg)
    with pytest.raises(ValueError, match=key):
        models.Block(32, 2, **{key: bad})
    with pytest.raises(ValueError, match=key):
        models.SerializedAttention(32, 2, 48, **{key: bad})
    with pytest.raises(ValueError, match=key):
        models.SerializedCrossAttention(32, 32, 2, 48, 48, **{key: bad})


def test_rejected_switches_stay_rejected():
    for key in ("enable_rpe", "tm_restomer", "pdnorm_bn", "pdnorm_ln", "cls_mode"):
        cfg = configs.mini_config()
        cfg["backbone"].update({key: True, "attn_drop": 0.1})
        with pytest.raises(NotImplementedError, match=key):
            build_model(cfg)


# ------------------------------------------------------------------------------------------ the graph on the emulated op layer
class _Log:
    """Wraps the three dropout ops of the emulation: (op, seed, offset, rate) of every call, from any thread."""

    def __init__(self, monkeypatch):
        self.calls = []
        lock = threading.Lock()

        def wrap(name, nseed):
            fn = getattr(emu_dropout_ops, name)

            def wrapped(*a, **k):
                rate, seed, offset = a[nseed - 1], a[nseed], a[nseed + 1]
                with lock:
                    self.calls.append((name, seed, offset, rate))
                return fn(*a, **k)

            monkeypatch.setattr(emu_dropout_ops, name, wrapped)

        wrap("attention_drop", 12)
        wrap("attention_drop_bwd", 15)
        wrap("dropout", 2)

    def take(self):
        out, self.calls = self.calls, []
        return out


@pytest.fixture()
def emulated(monkeypatch):
    monkeypatch.setattr(engine, "ops", emu_dropout_ops)
    monkeypatch.setattr(tg, "ops", emu_dropout_ops)
    return _Log(monkeypatch)


def _model(attn_drop, proj_drop, seed=4):
    cfg = configs.mini_config()
    cfg["backbone"].update(enable_flash=False, attn_drop=attn_drop, proj_drop=proj_drop, drop_path=0.0)
    cfg["criteria"] = [dict(type="MSELoss", loss_weight=1.0, ignore_index=-1, batch_sample_point=-1),
                       dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1)]
    cfg["loss_type"] = "EW"
    model = build_model(cfg)
    model.load_state_dict(fill_state_dict(model.state_dict(), seed=seed))
    return cfg, model.train()


def _batch(cfg):
    a = synth.room_scene(1, 400, num_classes=cfg["num_classes"])
    inp = {k: torch.as_tensor(a[k]) for k in ("coord", "grid_coord", "feat")}
    inp["segment"] = torch.as_tensor(a["segment"].astype(np.int64))
    n = len(a["coord"])
    inp["offset"] = torch.as_tensor(np.array([n]))
    noise = np.random.default_rng(0).standard_normal((n, cfg["c_in_channels"])).astype(np.float32)
    return inp, dict(ts=np.array([[17]]), noise=noise, perms=[[0, 1, 2, 3]] * 8)


def _nsites(model):
    return 4 * sum(isinstance(m, (models.Block, models.CrossBlock)) for m in model.modules())


def test_rate_0_and_eval_mode_never_reach_the_dropout_ops(emulated):
    cfg, model = _model(0.0, 0.0)
    inp, draws = _batch(cfg)
    l0 = model(inp, draws=dict(draws))["loss"]
    l0.backward()
    assert emulated.take() == [] and model._train_graph.dropout_sites == []
    cfg, dropped = _model(0.2, 0.2)
    dropped.eval()
    with torch.no_grad():
        l1 = dropped(inp, draws=dict(draws))["loss"]
    assert emulated.take() == [] and dropped._train_graph.dropout_sites == []
    cfg, fresh = _model(0.0, 0.0)  # (the training forward above moved `model`'s BatchNorm statistics)
    fresh.eval()
    with torch.no_grad():
        assert float(fresh(inp, draws=dict(draws))["loss"]) == float(l1)  # dropout is the identity in eval mode


def test_every_site_draws_once_per_forward_and_the_backward_reuses_its_pair(emulated):
    cfg, model = _model(0.2, 0.3)
    inp, draws = _batch(cfg)
    torch.manual_seed(11)
    loss = model(inp, draws=dict(draws))["loss"]
    fwd = emulated.take()
    sites = model._train_graph.dropout_sites
    assert len(sites) == _nsites(model) == len(fwd)
    assert len({name for name, _, _ in sites}) == len(sites), "a site was visited twice"
    assert all(s == 11 for _, s, _ in sites)
    assert [o for _, _, o in sites] == list(range(len(sites))), "every site takes the next offset"
    assert [(s, o) for _, s, o, _ in fwd] == [(s, o) for _, s, o in sites]
    kinds = {n.rsplit(".", 1)[-1] if not n.endswith((".drop.0", ".drop.1")) else "mlp_drop" for n, _, _ in sites}
    assert kinds == {"attn_drop", "proj_drop", "mlp_drop"}
    assert {r for op, _, _, r in fwd if op == "attention_drop"} == {0.2} and {r for op, _, _, r in fwd if op == "dropout"} == {0.3}
    nattn = sum(op == "attention_drop" for op, _, _, _ in fwd)
    assert 4 * nattn == len(fwd)
    loss.backward()
    bwd = emulated.take()
    assert all(op in ("attention_drop_bwd", "dropout") for op, _, _, _ in bwd)
    assert sorted((s, o, r) for _, s, o, r in bwd) == sorted((s, o, r) for _, s, o, r in fwd), "the backward reuses each site's pair"
    assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    # the counter goes on under the same seed, restarts under another one, and the same seed again gives the same pairs
    l2 = model(inp, draws=dict(draws))["loss"]
    assert [o for _, _, o in model._train_graph.dropout_sites] == list(range(len(sites), 2 * len(sites)))
    assert float(l2.detach()) != float(loss.detach())
    torch.manual_seed(12)
    l3 = model(inp, draws=dict(draws))["loss"]
    assert [(s, o) for _, s, o in model._train_graph.dropout_sites] == [(12, o) for o in range(len(sites))]
    torch.manual_seed(11)
    l4 = model(inp, draws=dict(draws))["loss"]
    assert model._train_graph.dropout_sites == sites
    assert float(l4.detach()) == float(loss.detach()) and float(l3.detach()) != float(loss.detach())
    # a pinned forward takes (seed, first offset) from the draws and leaves the counter alone
    l5 = model(inp, draws=dict(draws, dropout=(11, 0)))["loss"]
    assert model._train_graph.dropout_sites == sites and float(l5.detach()) == float(loss.detach())
    model(inp, draws=dict(draws))
    assert model._train_graph.dropout_sites[0][2] == len(sites)
    emulated.take()


def test_native_mode_runs_dropout_blocks_as_their_autograd_chain_and_warns_once(emulated, monkeypatch):
    cfg, model = _model(0.2, 0.2)
    inp, draws = _batch(cfg)
    ref = float(model(inp, draws=dict(draws, dropout=(5, 100)))["loss"])
    model.train_block = "native"
    monkeypatch.setattr(tg, "_warned_native_dropout", False)
    for name in ("train_block_forward", "train_block_backward"):
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("the native executor was reached"))
    with pytest.warns(UserWarning, match="autograd chain") as rec:
        got = float(model(inp, draws=dict(draws, dropout=(5, 100)))["loss"])
    assert sum("autograd chain" in str(w.message) for w in rec) == 1
    assert got == ref
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        model(inp, draws=dict(draws, dropout=(5, 100)))  # once per process
