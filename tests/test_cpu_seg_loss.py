"""CPU: the fused segmentation loss's host side - argument checks of the entry points (before any launch, so they run without
a GPU), the workspace query, the `train_loss` switch, the routing decisions that need no device, and the closed form the
kernels implement against fp64 autograd of cdsegnet_amd/losses.py (the oracle of tests/test_gpu_seg_loss.py, pinned where it
can run)."""
import ctypes

import numpy as np
import pytest
import torch

from cdsegnet_amd import _lib, configs
from tests.test_gpu_seg_loss import IGNORE, make_case, oracle

OK, ERR_ARG, ERR_WS, ERR_UNSUP = 0, -1, -3, -4


@pytest.fixture(scope="module", params=_lib.VARIANTS)
def lib(request):
    import os
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib.LIB_PATH_F16)):
        from cdsegnet_amd.build import build_library
        build_library()
    return _lib.load(request.param)


def _hist(c, counts):
    h = (ctypes.c_int32 * (c + 1))()
    for k, v in counts.items():
        h[k] = v
    return h


P = 0x10000  # a non-null, 16-byte aligned address that is never dereferenced: every check below fails before a launch


def test_entry_points_check_their_arguments_before_any_launch(lib):
    n, c = 1000, 20
    ws = lib.cdseg_seg_loss_ws_bytes(n, c)
    h = _hist(c, {0: 400, 7: 500})
    fwd = lambda **k: lib.cdseg_seg_loss_fwd(*[k.get(a, d) for a, d in (  # noqa: E731
        ("logits", P), ("ldl", c), ("labels", P), ("n", n), ("c", c), ("ignore", -1), ("phase", 1), ("hist", None), ("hist_host", h),
        ("out", P), ("coef", P), ("ws", P), ("ws_bytes", ws), ("stream", None))])
    bwd = lambda **k: lib.cdseg_seg_loss_bwd(*[k.get(a, d) for a, d in (  # noqa: E731
        ("logits", P), ("ldl", c), ("labels", P), ("n", n), ("c", c), ("ignore", -1), ("hist_host", h), ("coef", P), ("g_ce", P),
        ("g_lov", P), ("dlogits", P), ("lddl", c), ("stream", None))])
    for call in (fwd, bwd):
        assert call(logits=None) == ERR_ARG and call(labels=None) == ERR_ARG
        assert call(n=0) == ERR_ARG and call(c=0) == ERR_ARG and call(ldl=c - 1) == ERR_ARG
        assert call(logits=P + 2) == ERR_ARG and call(labels=P + 4) == ERR_ARG
        assert call(n=1 << 24) == ERR_UNSUP and call(c=257, ldl=257) == ERR_UNSUP
        assert call(hist_host=None) == ERR_ARG
        assert call(hist_host=_hist(c, {})) == ERR_ARG                  # no valid row: no fused form
        assert call(hist_host=_hist(c, {0: 400, c: 1})) == ERR_ARG      # a label outside the classes
        assert call(hist_host=_hist(c, {0: 600, 1: 500})) == ERR_ARG    # more rows than n
        assert call(coef=None) == ERR_ARG
    assert fwd(n=(1 << 24) - 1, ws_bytes=0) == ERR_WS and fwd(c=256, ldl=256, hist_host=_hist(256, {3: 5}), ws_bytes=0) == ERR_WS
    assert fwd(phase=2) == ERR_ARG and fwd(phase=0, hist=None) == ERR_ARG and fwd(out=None) == ERR_ARG
    assert fwd(ws=None) == ERR_WS and fwd(ws_bytes=ws - 1) == ERR_WS and fwd(ws=P + 8) == ERR_ARG
    assert bwd(dlogits=None) == ERR_ARG and bwd(lddl=c - 1) == ERR_ARG and bwd(g_ce=P + 1) == ERR_ARG


def test_workspace_query_is_monotone(lib):
    ns, cs = (1, 63, 65, 1000, 4099, 120000, 480000), (1, 13, 16, 20, 64, 200, 256)
    sizes = np.array([[lib.cdseg_seg_loss_ws_bytes(n, c) for c in cs] for n in ns], dtype=np.float64)
    assert (sizes > 0).all() and (np.diff(sizes, axis=0) >= 0).all() and (np.diff(sizes, axis=1) >= 0).all()
    assert sizes[-1, -2] >= 2 * 8 * 480000 * 200  # two buffers of 64-bit keys, one per (row, class)
    assert lib.cdseg_seg_loss_ws_bytes(0, 20) == 0 and lib.cdseg_seg_loss_ws_bytes(10, 0) == 0


def test_switch_defaults_to_torch_and_validates():
    from cdsegnet_amd.losses import Criteria, FusedCriteria, build_criteria
    from cdsegnet_amd.registry import build_model
    from cdsegnet_amd.train_graph import resolve_train_loss
    import cdsegnet_amd.models  # noqa: F401
    model = build_model(configs.mini_config())
    assert model.train_loss == "torch" and "train_loss" not in model.state_dict()
    assert resolve_train_loss(model) == "torch"
    model.train_loss = "fused"
    assert resolve_train_loss(model) == "fused"
    model.train_loss = "hip"
    with pytest.raises(ValueError, match="train_loss"):
        resolve_train_loss(model)
    with pytest.raises(ValueError, match="train_loss"):
        build_criteria([], train_loss="hip")
    cfg = [dict(type="CrossEntropyLoss", ignore_index=-1), dict(type="LovaszLoss", mode="multiclass", ignore_index=-1)]
    assert type(build_criteria(cfg)) is Criteria and type(build_criteria(cfg, "GLS", 2, "torch")) is Criteria
    assert type(build_criteria(cfg, train_loss="fused")) is FusedCriteria


def test_fused_criteria_route_to_torch_off_the_device_and_for_unfusable_pairs(monkeypatch):
    """CPU tensors and pairs the kernels do not cover take the torch path: same object calls, same bits, the fused ops are never
    reached (so the CPU emulation of the ops that the host-logic tests swap in needs no such op)."""
    from cdsegnet_amd import ops
    from cdsegnet_amd.losses import build_criteria
    for name in ("seg_loss_plan", "seg_loss"):
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("a fused op was reached"))
    ce, lv = dict(type="CrossEntropyLoss", ignore_index=-1), dict(type="LovaszLoss", mode="multiclass", ignore_index=-1)
    mse = dict(type="MSELoss", ignore_index=-1, batch_sample_point=-1)
    fusable = build_criteria([mse, ce, lv], "GLS", 2, "fused")
    assert fusable._pair() is not None
    for a, b in ((dict(ce, weight=[1.0] * 13), lv), (dict(ce, label_smoothing=0.1), lv), (dict(ce, reduction="sum"), lv),
                 (ce, dict(lv, ignore_index=-2)), (dict(ce, ignore_index=0), dict(lv, ignore_index=0)),
                 (dict(ce, ignore_index=None), dict(lv, ignore_index=None)), (dict(ce, pred="c_pred"), lv)):
        assert build_criteria([mse, a, b], "GLS", 2, "fused")._pair() is None, (a, b)
    assert build_criteria([mse, ce], "EW", 2, "fused")._pair() is None
    t, labels, _ = make_case(65, 13, "ignore7")
    g = torch.Generator().manual_seed(1)
    c_pred, c_target = torch.randn(65, 6, generator=g), torch.randn(65, 6, generator=g)
    res = []
    for mode in ("torch", "fused"):
        for loss_type in ("EW", "GLS"):
            x = t.clone().requires_grad_(True)
            point = dict(n_pred=x, n_target=labels, c_pred=c_pred, c_target=c_target, loss_mode="train")
            loss = build_criteria([mse, ce, lv], loss_type, 2, mode)(point)
            loss.backward()
            res.append((mode, loss_type, loss.detach(), x.grad))
    for (_, _, l0, g0), (_, _, l1, g1) in zip(res[:2], res[2:]):
        assert torch.equal(l0, l1) and torch.equal(g0, g1)


SHAPES = [(1, 13, "ignore7"), (65, 13, "ignore7"), (63, 16, "lone"), (1000, 20, "half"), (1000, 20, "single"), (4099, 200, "ignore7"),
          (4099, 200, "strided")]


@pytest.mark.parametrize("n,c,variant", SHAPES, ids=[f"{n}x{c}-{v}" for n, c, v in SHAPES])
def test_closed_form_equals_fp64_autograd_of_the_criteria(n, c, variant):
    """The oracle (loss, dCE, dLovasz in closed form, jac a constant) against autograd through cdsegnet_amd/losses.py in fp64,
    with ignored rows and absent classes.  (Random fp64 errors do not tie, so the criteria's unstable sort gives the same
    order.)"""
    from cdsegnet_amd.losses import CrossEntropyLoss, LovaszLoss
    t, labels, win = make_case(n, c, variant)
    logits = (t if win is None else t[:, win[0]:win[1]]).double()
    o = oracle(logits, labels)
    x = logits.clone().requires_grad_(True)
    point = dict(n_pred=x, n_target=labels)
    ce = CrossEntropyLoss(ignore_index=IGNORE)(point)
    lv = LovaszLoss("multiclass", ignore_index=IGNORE)(point)
    g_ce, = torch.autograd.grad(ce, x, retain_graph=True)
    g_lv, = torch.autograd.grad(lv, x)
    assert abs(float(ce.detach() - o["ce"])) < 1e-13 and abs(float(lv.detach() - o["lovasz"])) < 1e-13
    assert float((g_ce - o["d_ce"]).abs().max()) < 1e-15 and float((g_lv - o["d_lovasz"]).abs().max()) < 1e-15
