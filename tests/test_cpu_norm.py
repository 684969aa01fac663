"""CPU: what `model.train_norm = "fused"` promises without a device - the entry points of csrc/norm.hip reject bad arguments
before any launch (both builds), the row partition of the two reduction passes is a function of (m, c) alone, the mode
switch validates, and on the emulated op layer (tests/emu_norm_ops.py) the fused training step is the torch step up to fp32
rounding, with one fused BatchNorm call per training-mode BatchNorm module the forward passes and one arg-max call per pooling.
"""
import ctypes

import numpy as np
import pytest
import torch

from cdsegnet_amd import _lib

OK, ERR_ARG, ERR_WS, ERR_UNSUPPORTED = 0, -1, -3, -4
P = ctypes.c_void_p
BUF, ODD8, ODD4 = P(1 << 20), P((1 << 20) + 8), P((1 << 20) + 4)  # 16-byte aligned; 8 bytes off; 4 bytes off


@pytest.fixture(params=list(_lib.VARIANTS))
def lib(request):
    return _lib.load(request.param)


def _partition(lib, m, c):
    rows, blocks = ctypes.c_long(-7), ctypes.c_int(-7)
    st = lib.cdseg_bn_partition(m, c, ctypes.byref(rows), ctypes.byref(blocks))
    return st, rows.value, blocks.value


WIDTHS = [16, 32, 48, 64, 128, 256, 512]


def test_partition_is_a_function_of_the_shape_and_covers_every_row_once(lib):
    from tests import emu_norm_ops
    for c in WIDTHS:
        for m in [1, 2, 63, 64, 65, 255, 256, 257, 777, 5003, 52200, 65536, 65537, 120000, 1 << 22]:
            st, rows, blocks = _partition(lib, m, c)
            assert st == OK and (rows, blocks) == _partition(lib, m, c)[1:]          # asked twice: the same answer
            assert (rows, blocks) == emu_norm_ops.bn_partition(m, c)                # the restated rule
            assert rows >= 256 and blocks <= 256
            # block b = rows [b rows, min((b + 1) rows, m)): disjoint, ascending, every row exactly once, no empty block
            assert (blocks - 1) * rows < m <= blocks * rows
            assert lib.cdseg_bn_ws_bytes(m, c) == blocks * 2 * c * 8
    st, rows, blocks = _partition(lib, 5003, 32)
    assert blocks >= 4                                                              # what the summation-order test needs
    assert _partition(lib, 0, 32) == (OK, 256, 0) and lib.cdseg_bn_ws_bytes(0, 32) == 0
    for c in (0, 8, 24, 528, 1024):
        assert _partition(lib, 100, c) == (ERR_UNSUPPORTED, -7, -7) and lib.cdseg_bn_ws_bytes(100, c) == 0
    assert _partition(lib, -1, 32)[0] == ERR_ARG
    assert lib.cdseg_bn_partition(100, 32, None, None) == ERR_ARG
    from cdsegnet_amd import ops
    got = ops.bn_partition(5003, 32)
    assert (got.rows_per_block, got.blocks) == tuple(got) == (rows, blocks)


@pytest.mark.skipif(torch.cuda.is_available(), reason="stand-in pointers: only where nothing can be launched")
def test_entry_points_check_their_arguments_before_any_launch(lib):
    """Pointers are never dereferenced on these paths: aligned non-null integers stand in for device memory.  With a device a
    check that has regressed would launch on them, so this runs only where torch sees none."""
    M, C = 5003, 32
    need = lib.cdseg_bn_ws_bytes(M, C)
    assert need == 20 * 2 * C * 8
    # ---- cdseg_bn_stats(x, ldx, m, c, stats, ws, ws_bytes, stream)
    st = lib.cdseg_bn_stats
    assert st(None, C, 0, C, None, None, 0, None) == OK                           # m = 0: nothing to do
    assert st(BUF, C, M, C, BUF, None, need, None) == ERR_WS
    assert st(BUF, C, M, C, BUF, BUF, need - 1, None) == ERR_WS
    assert st(BUF, C, M, C, BUF, ODD8, need + 8, None) == ERR_ARG                 # workspace not 16-byte aligned
    assert st(None, C, M, C, BUF, BUF, need, None) == ERR_ARG
    assert st(BUF, C, M, C, None, BUF, need, None) == ERR_ARG
    assert st(ODD8, C, M, C, BUF, BUF, need, None) == ERR_ARG                     # x: 16-byte loads
    assert st(BUF, C, M, C, ODD4, BUF, need, None) == ERR_ARG                     # stats: fp64
    assert st(BUF, C + 2, M, C, BUF, BUF, need, None) == ERR_ARG                  # stride not a multiple of 4
    assert st(BUF, C - 4, M, C, BUF, BUF, need, None) == ERR_ARG                  # stride below c
    assert st(BUF, C, -1, C, BUF, BUF, need, None) == ERR_ARG
    for c in (8, 24, 528):
        assert st(BUF, 1024, M, c, BUF, BUF, 1 << 30, None) == ERR_UNSUPPORTED
    # ---- cdseg_bn_finish(stats, c, eps, momentum, mean, invstd, running_mean, running_var, stream)
    fin = lib.cdseg_bn_finish
    assert fin(None, C, 1e-3, 0.01, BUF, BUF, None, None, None) == ERR_ARG
    assert fin(BUF, C, 1e-3, 0.01, None, BUF, None, None, None) == ERR_ARG
    assert fin(BUF, C, 1e-3, 0.01, BUF, None, None, None, None) == ERR_ARG
    assert fin(ODD4, C, 1e-3, 0.01, BUF, BUF, None, None, None) == ERR_ARG
    assert fin(BUF, C, 1e-3, 0.01, ODD8, BUF, None, None, None) == ERR_ARG
    assert fin(BUF, C, 1e-3, 0.01, BUF, BUF, P((1 << 20) + 2), None, None) == ERR_ARG
    assert fin(BUF, C, -1.0, 0.01, BUF, BUF, None, None, None) == ERR_ARG
    assert fin(BUF, C, 1e-3, 1.5, BUF, BUF, None, None, None) == ERR_ARG
    assert fin(BUF, C, 1e-3, float("nan"), BUF, BUF, None, None, None) == ERR_ARG
    assert fin(BUF, 24, 1e-3, 0.01, BUF, BUF, None, None, None) == ERR_UNSUPPORTED
    # ---- cdseg_bn_gelu_fwd(x, ldx, m, c, mean, invstd, gamma, beta, y, ldy, stream)
    fwd = lib.cdseg_bn_gelu_fwd
    assert fwd(None, C, 0, C, None, None, None, None, None, C, None) == OK
    good = [BUF, C, M, C, BUF, BUF, BUF, BUF, BUF, C, None]
    for i in (0, 4, 5, 6, 7, 8):                                                  # every pointer: NULL, then misaligned
        for bad in (None, ODD8):
            a = list(good)
            a[i] = bad
            assert fwd(*a) == ERR_ARG, (i, bad)
    for i in (1, 9):
        for bad in (C + 1, C - 4):
            a = list(good)
            a[i] = bad
            assert fwd(*a) == ERR_ARG, (i, bad)
    assert fwd(BUF, 1024, M, 40, BUF, BUF, BUF, BUF, BUF, 1024, None) == ERR_UNSUPPORTED
    # ---- cdseg_bn_gelu_bwd_sums(x, ldx, dy, lddy, m, c, mean, invstd, gamma, beta, gsums, ws, ws_bytes, stream)
    sums = lib.cdseg_bn_gelu_bwd_sums
    assert sums(None, C, None, C, 0, C, None, None, None, None, None, None, 0, None) == OK
    good = [BUF, C, BUF, C, M, C, BUF, BUF, BUF, BUF, BUF, BUF, need, None]
    for i in (0, 2, 6, 7, 8, 9):
        for bad in (None, ODD8):
            a = list(good)
            a[i] = bad
            assert sums(*a) == ERR_ARG, (i, bad)
    for i, bad in ((10, None), (10, ODD4), (1, C + 2), (3, C - 4), (11, ODD8)):
        a = list(good)
        a[i] = bad
        assert sums(*a) == ERR_ARG, (i, bad)
    assert sums(*(good[:11] + [None, need, None])) == ERR_WS
    assert sums(*(good[:11] + [BUF, need - 1, None])) == ERR_WS
    assert sums(BUF, 1024, BUF, 1024, M, 520, BUF, BUF, BUF, BUF, BUF, BUF, 1 << 30, None) == ERR_UNSUPPORTED
    # ---- cdseg_bn_gelu_bwd_dx(x, ldx, dy, lddy, m, c, mean, invstd, gamma, beta, gsums, count, dx, lddx, stream)
    dxf = lib.cdseg_bn_gelu_bwd_dx
    assert dxf(None, C, None, C, 0, C, None, None, None, None, None, None, None, C, None) == OK
    good = [BUF, C, BUF, C, M, C, BUF, BUF, BUF, BUF, BUF, BUF, BUF, C, None]
    for i in (0, 2, 6, 7, 8, 9, 12):
        for bad in (None, ODD8):
            a = list(good)
            a[i] = bad
            assert dxf(*a) == ERR_ARG, (i, bad)
    for i, bad in ((10, None), (10, ODD4), (11, None), (11, ODD4), (1, C + 2), (3, C + 2), (13, C - 4)):
        a = list(good)
        a[i] = bad
        assert dxf(*a) == ERR_ARG, (i, bad)
    assert dxf(BUF, 16, BUF, 16, M, 8, BUF, BUF, BUF, BUF, BUF, BUF, BUF, 16, None) == ERR_UNSUPPORTED
    # ---- cdseg_segment_max_arg(y, ldy, seg_start, m, c, out, ldo, arg, lda, stream)
    sma = lib.cdseg_segment_max_arg
    assert sma(None, C, None, 0, C, None, C, None, C, None) == OK
    good = [BUF, C, BUF, 100, C, BUF, C, BUF, C, None]
    for i in (0, 2, 5, 7):
        for bad in (None, P((1 << 20) + 2) if i == 2 else ODD8):
            a = list(good)
            a[i] = bad
            assert sma(*a) == ERR_ARG, (i, bad)
    for i in (1, 6, 8):
        a = list(good)
        a[i] = C + 2
        assert sma(*a) == ERR_ARG, i
    assert sma(BUF, C, BUF, 1 << 31, C, BUF, C, BUF, C, None) == ERR_UNSUPPORTED    # arg is int32
    assert sma(BUF, 24, BUF, 100, 24, BUF, 24, BUF, 24, None) == ERR_UNSUPPORTED
    # ---- cdseg_segment_max_bwd(dout, lddo, arg, lda, cluster, n, c, dy, lddy, stream)
    smb = lib.cdseg_segment_max_bwd
    assert smb(None, C, None, C, None, 0, C, None, C, None) == OK
    good = [BUF, C, BUF, C, BUF, 100, C, BUF, C, None]
    for i in (0, 2, 4, 7):
        for bad in (None, P((1 << 20) + 2) if i == 4 else ODD8):
            a = list(good)
            a[i] = bad
            assert smb(*a) == ERR_ARG, (i, bad)
    for i in (1, 3, 8):
        a = list(good)
        a[i] = C - 4
        assert smb(*a) == ERR_ARG, i
    assert smb(BUF, C, BUF, C, BUF, 1 << 31, C, BUF, C, None) == ERR_UNSUPPORTED
    assert smb(BUF, 1024, BUF, 1024, BUF, 100, 1024, BUF, 1024, None) == ERR_UNSUPPORTED


def test_ops_need_a_gpu():
    from cdsegnet_amd import ops
    if not torch.cuda.is_available():
        with pytest.raises(_lib.CdsegError):
            ops.bn_stats(torch.zeros(4, 16))
        with pytest.raises(_lib.CdsegError):
            ops.segment_max_arg(torch.zeros(4, 16), torch.zeros(3, dtype=torch.int32), 2)


def test_train_norm_validation():
    """train_norm: "torch" by default, "fused" accepted, anything else raises at the forward; not part of the state_dict."""
    import cdsegnet_amd.models  # noqa: F401
    from cdsegnet_amd import configs
    from cdsegnet_amd.registry import build_model
    from cdsegnet_amd.train_graph import TRAIN_NORMS, resolve_train_norm
    model = build_model(configs.mini_config())
    assert TRAIN_NORMS == ("torch", "fused")
    assert model.train_norm == "torch" and resolve_train_norm(model) == "torch" and "train_norm" not in model.state_dict()
    model.train_norm = "fused"
    assert resolve_train_norm(model) == "fused"
    for bad in ("Fused", None, True, "hip"):
        model.train_norm = bad
        with pytest.raises(ValueError, match="train_norm"):
            resolve_train_norm(model)
    del model.train_norm
    assert resolve_train_norm(model) == "torch"  # (a model object from before the attribute)


# ------------------------------------------------------------------------------------------ the step on the emulated ops
def _mini(monkeypatch):
    import cdsegnet_amd.engine as engine
    import cdsegnet_amd.train_graph as tg
    from cdsegnet_amd import configs
    from cdsegnet_amd.param_init import fill_state_dict
    from cdsegnet_amd.registry import build_model
    from tests import emu_norm_ops
    from tests.helpers import load_fixture
    monkeypatch.setattr(engine, "ops", emu_norm_ops)
    monkeypatch.setattr(tg, "ops", emu_norm_ops)
    fx = load_fixture("train_step_mini.npz")
    cfg = configs.mini_config()
    cfg["backbone"]["enable_flash"] = False
    cfg["criteria"] = [dict(type="MSELoss", loss_weight=1.0, ignore_index=-1, batch_sample_point=-1),
                       dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1),
                       dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)]
    model = build_model(cfg)
    model.load_state_dict(fill_state_dict(model.state_dict(), seed=int(fx["sd_seed"])))
    model.train()
    masks = {str(k): [fx[f"mask.{i}.{j}"] for j in range(int(fx["mask_counts"][i]))] for i, k in enumerate(fx["mask_names"])}
    draws = dict(ts=fx["ts"], noise=fx["noise"], perms=[list(p) for p in fx["perms"]], masks=masks)
    inp = {k: torch.as_tensor(fx[k]) for k in ("coord", "grid_coord", "feat", "offset", "segment")}
    return model, inp, draws, emu_norm_ops


def test_fused_step_on_the_emulated_ops_equals_the_torch_step(monkeypatch):
    """The recorded mini step (tests/golden/train_step_mini.npz) in both modes from the same state: the same loss, gradients
    and BatchNorm buffers up to fp32 rounding (bound: the 1e-3 sanity bound and metric of the whole-step tests - the same sums
    in another order; the loss, a single fp32 number of order 1, within 1e-5); the fused mode calls the BatchNorm forward once
    per training-mode BatchNorm module (every one of them advances num_batches_tracked), the arg-max once per pooling module,
    and reaches F.batch_norm nowhere; the real ops are never touched."""
    import torch.nn.functional as F
    from cdsegnet_amd import models
    from cdsegnet_amd import ops as real_ops
    model, inp, draws, emu = _mini(monkeypatch)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    calls = {"bn_fwd": 0, "bn_bwd": 0, "arg": 0, "arg_bwd": 0, "batch_norm": 0}

    def counted(key, fn):
        def f(*a, **kw):
            calls[key] += 1
            return fn(*a, **kw)
        return f

    for name, key in (("bn_gelu_fwd", "bn_fwd"), ("bn_gelu_bwd", "bn_bwd"), ("segment_max_arg", "arg"), ("segment_max_bwd", "arg_bwd")):
        monkeypatch.setattr(emu, name, counted(key, getattr(emu, name)))
        monkeypatch.setattr(real_ops, name, lambda *a, **k: pytest.fail("the device ops were reached"))
    monkeypatch.setattr(F, "batch_norm", counted("batch_norm", F.batch_norm))

    def run(mode):
        model.load_state_dict(state)
        model.zero_grad(set_to_none=True)
        model.train_norm = mode
        for k in calls:
            calls[k] = 0
        out = model(inp, draws={**draws, "masks": {k: list(v) for k, v in draws["masks"].items()}})
        out["loss"].backward()
        grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
        bufs = {k: v.detach().clone() for k, v in model.state_dict().items() if "running_" in k or "num_batches" in k}
        return float(out["loss"].detach()), grads, bufs, dict(calls)

    l0, g0, b0, c0 = run("torch")
    l1, g1, b1, c1 = run("fused")
    bns = [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm1d)]
    moved = sum(int(b1[k]) == int(state[k]) + 1 for k in b1 if k.endswith("num_batches_tracked"))
    pools = sum(isinstance(m, models.SerializedPooling) for m in model.modules())
    assert c0 == {"bn_fwd": 0, "bn_bwd": 0, "arg": 0, "arg_bwd": 0, "batch_norm": c0["batch_norm"]} and c0["batch_norm"] == moved
    assert 0 < moved <= len(bns) and pools > 0
    assert c1 == {"bn_fwd": moved, "bn_bwd": moved, "arg": pools, "arg_bwd": pools, "batch_norm": 0}, c1
    assert abs(l0 - l1) <= 1e-5 * abs(l0)
    assert set(g0) == set(g1) and len(g0) > 400
    top = max(float(g.abs().max()) for g in g0.values())
    worst = max(float((g0[k] - g1[k]).abs().max()) / (float(g0[k].abs().max()) + 1e-3 * top) for k in g0)
    print(f"[measure] emulated step fused vs torch: loss {l0:.8f} / {l1:.8f}, worst gradient difference {worst:.3e}")
    assert worst < 1e-3
    for k in b0:
        if k.endswith("num_batches_tracked"):
            assert torch.equal(b0[k], b1[k]), k
        else:
            assert float((b0[k] - b1[k]).abs().max()) <= 1e-5 * float(b0[k].abs().max()), k


def test_eval_mode_and_unsupported_widths_keep_the_torch_path(monkeypatch):
    """Eval mode always normalises with the running statistics through torch; a width the kernels do not cover (20) and
    momentum = None stay on torch's train-mode batch norm (which refuses the latter, as before); with local statistics one row raises like torch."""
    import cdsegnet_amd.train_graph as tg
    from tests import emu_norm_ops
    monkeypatch.setattr(tg, "ops", emu_norm_ops)
    reached = []
    real = emu_norm_ops.bn_stats
    monkeypatch.setattr(emu_norm_ops, "bn_stats", lambda x: (reached.append(tuple(x.shape)), real(x))[1])
    g = torch.Generator().manual_seed(0)
    x = torch.randn(50, 32, generator=g)
    bn = torch.nn.BatchNorm1d(32, eps=1e-3, momentum=0.01)
    want = torch.nn.functional.gelu(torch.nn.BatchNorm1d(32, eps=1e-3, momentum=0.01)(x))
    got = tg._bn_gelu(x, bn, "fused")
    assert reached == [(50, 32)] and float((got - want).detach().abs().max()) < 1e-5 and int(bn.num_batches_tracked) == 1
    bn.eval()
    tg._bn_gelu(x, bn, "fused")
    assert reached == [(50, 32)] and int(bn.num_batches_tracked) == 1
    bn20 = torch.nn.BatchNorm1d(20)
    tg._bn_gelu(torch.randn(50, 20, generator=g), bn20, "fused")
    assert reached == [(50, 32)] and int(bn20.num_batches_tracked) == 1
    with pytest.raises(TypeError, match="momentum"):  # (momentum = None: torch's functional form, which has no cumulative average)
        tg._bn_gelu(x, torch.nn.BatchNorm1d(32, momentum=None), "fused")
    assert reached == [(50, 32)]
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        tg._bn_gelu(x[:1], torch.nn.BatchNorm1d(32), "fused")


def test_emulated_ops_agree_with_autograd():
    """The emulation itself (what the CPU and the two-rank tests stand on): BatchNorm + GELU forward / backward and the arg-max
    pooling against torch autograd in fp64."""
    from tests import emu_norm_ops as E
    g = torch.Generator().manual_seed(1)
    x, dy = torch.randn(300, 32, generator=g) + 0.5, torch.randn(300, 32, generator=g)
    gamma, beta = torch.rand(32, generator=g) + 0.5, torch.randn(32, generator=g)
    stats = E.bn_stats(x)
    rm, rv = torch.zeros(32), torch.ones(32)
    mean, invstd = E.bn_finish(stats, 1e-3, 0.01, rm, rv)
    y = E.bn_gelu_fwd(x, mean, invstd, gamma, beta)
    dx, gs = E.bn_gelu_bwd(x, dy, mean, invstd, gamma, beta, stats[64:])
    xd, gd, bd = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    rm64, rv64 = torch.zeros(32, dtype=torch.float64), torch.ones(32, dtype=torch.float64)
    y64 = torch.nn.functional.gelu(torch.nn.functional.batch_norm(xd, rm64, rv64, gd, bd, True, 0.01, 1e-3))
    y64.backward(dy.double())
    for got, want in ((y, y64.detach()), (dx, xd.grad), (gs[32:], gd.grad), (gs[:32], bd.grad), (rm, rm64), (rv, rv64)):
        assert float((got.double() - want).abs().max()) <= 2e-6 * float(want.abs().max())
    seg = torch.tensor([0, 3, 4, 9, 10], dtype=torch.int32)
    v = torch.randn(10, 16, generator=g)
    v[1, :8] = v[0, :8]
    v[4:9, 3] = 2.0
    out, arg = E.segment_max_arg(v, seg, 4)
    cl = torch.repeat_interleave(torch.arange(4), torch.tensor([3, 1, 5, 1]))
    for j in range(4):
        rows = torch.nonzero(cl == j).flatten()
        assert torch.equal(out[j], v[rows].max(0).values)
        assert torch.equal(arg[j].long(), rows[(v[rows] == out[j]).int().argmax(0)])  # the first maximal row
    d = E.segment_max_bwd(torch.ones(4, 16), arg, cl.int())
    assert torch.equal(d.sum(0), torch.full((16,), 4.0)) and float(d[1, :8].sum()) == 0.0 and float(d[5:9, 3].sum()) == 0.0
