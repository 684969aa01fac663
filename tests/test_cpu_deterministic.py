"""CPU: what the deterministic training mode promises without a device - the row partition of the weight-gradient launches
(host code: a function of the shape only), the workspace sizes, the argument checks of the `_det` entry points (before any
launch), the mode switch, and the summation-order contract restated in fp32 numpy.

The order contract (include/cdseg.h): split s leaves its partial in the workspace; the reduce computes t = p[0]; t += p[1];
... by ascending split index, then dw = dw + t.  `_replay` below is that sentence in numpy.
"""
import ctypes

import numpy as np
import pytest
import torch

from cdsegnet_amd import _lib

PARTITION_SIG = _lib.SIGNATURES["cdseg_wgrad_partition"]  # (the feature's first symbol: absent before it)
F32, LP16 = _lib.F32, _lib.BF16


@pytest.fixture(params=list(_lib.VARIANTS))
def lib(request):
    return _lib.load(request.param)


def _rule(m, n, k, kvol, lp):
    """The launch rule of csrc/train.hip restated: (rows_per_split, splits)."""
    cdiv = lambda a, b: (a + b - 1) // b  # noqa: E731
    if not lp:
        tiles = cdiv(n, 64) * cdiv(k, 64) * kvol
        splits = max(1, min(cdiv(2048, tiles), cdiv(m, 1024)))
        rows = (cdiv(m, splits) + 3) // 4 * 4
    else:
        tn = 4 if n > 64 else 2 if n > 32 else 1
        tk = 4 if k > 64 else 2 if k > 32 else 1
        if tn == 4 and tk == 4:
            tk = 2
        tiles = cdiv(n, 32 * tn) * cdiv(k, 32 * tk) * kvol
        splits = max(1, min(cdiv(512, tiles), cdiv(m, 512)))
        rows = cdiv(cdiv(m, splits), 64) * 64
    return rows, cdiv(m, rows)


MS = [1, 1024, 1025, 2100, 4100, 5003, 120000]
SHAPES = [(32, 96, 1), (96, 32, 1), (64, 192, 1), (512, 512, 1), (16, 16, 1), (2048, 512, 1),
          (32, 32, 27), (64, 64, 27), (128, 128, 27), (16, 32, 125), (512, 512, 27)]


@pytest.mark.parametrize("lp", [False, True], ids=["fp32", "16-bit"])
def test_partition_equals_the_launch_rule(lp):
    """ops.wgrad_partition (host only, no GPU) against the restated rule: M = 1, the split thresholds 1024 / 1025, several
    splits, a full scene; the Linear form and the conv form with 27 and 125 offsets.  Both builds agree."""
    from cdsegnet_amd import ops
    dtype = torch.bfloat16 if lp else torch.float32
    for m in MS:
        for k, n, kvol in SHAPES:
            want = _rule(m, n, k, kvol, lp)
            got = ops.wgrad_partition(m, n, k, kvol, dtype)
            assert tuple(got) == want and (got.rows_per_split, got.splits) == want, (m, n, k, kvol, lp, tuple(got), want)
            assert (got.splits - 1) * got.rows_per_split < m <= got.splits * got.rows_per_split
            with _lib.use("f16"):
                assert tuple(ops.wgrad_partition(m, n, k, kvol, torch.float16 if lp else torch.float32)) == want
    # where the issue's GPU cases stand: at least three splits, else nothing order-dependent would run
    assert ops.wgrad_partition(4100, 96, 32, 1, torch.float32).splits >= 3
    assert ops.wgrad_partition(2100, 96, 32, 1, torch.bfloat16).splits >= 3
    assert ops.wgrad_partition(5003, 192, 64, 1, torch.bfloat16).splits >= 3


def test_partition_rejects_what_it_cannot_describe(lib):
    rows, splits = ctypes.c_long(-7), ctypes.c_int(-7)
    f = lib.cdseg_wgrad_partition
    assert f(100, 32, 32, 1, 7, ctypes.byref(rows), ctypes.byref(splits)) == -4   # no such dtype
    assert f(100, 0, 32, 1, F32, ctypes.byref(rows), ctypes.byref(splits)) == -1
    assert f(100, 32, 32, 0, F32, ctypes.byref(rows), ctypes.byref(splits)) == -1
    assert (rows.value, splits.value) == (-7, -7)                                   # nothing written on failure
    assert f(100, 32, 32, 1, F32, None, None) == 0                                  # outputs are optional
    assert f(0, 32, 32, 1, F32, ctypes.byref(rows), ctypes.byref(splits)) == 0 and splits.value == 0


def test_workspace_sizes_are_monotone_in_the_split_count(lib):
    """More rows -> at least as many splits -> at least as large a workspace; the size is (kvol splits n k + splits n) floats."""
    for dtype in (F32, LP16):
        for k, n, kvol in SHAPES:
            prev_s, prev_b = 0, 0
            for m in sorted(MS + [2, 500, 3000, 60000]):
                rows, splits = ctypes.c_long(0), ctypes.c_int(0)
                assert lib.cdseg_wgrad_partition(m, n, k, kvol, dtype, ctypes.byref(rows), ctypes.byref(splits)) == 0
                b = lib.cdseg_wgrad_det_ws_bytes(m, n, k, kvol, dtype)
                assert b == 4 * (kvol * splits.value * n * k + splits.value * n)
                assert splits.value >= prev_s and b >= prev_b and (b > prev_b) == (splits.value > prev_s)
                prev_s, prev_b = splits.value, b
    assert lib.cdseg_wgrad_det_ws_bytes(100, 32, 32, 1, 7) == 0
    assert lib.cdseg_layernorm_bwd_det_ws_bytes(1, 32) == 4 * 2 * 32
    assert lib.cdseg_layernorm_bwd_det_ws_bytes(64, 32) == 4 * 2 * 32
    assert lib.cdseg_layernorm_bwd_det_ws_bytes(65, 32) == 2 * 4 * 2 * 32
    assert lib.cdseg_layernorm_bwd_det_ws_bytes(120000, 512) == 1875 * 4 * 2 * 512


def test_det_entry_points_check_their_arguments_before_any_launch(lib):
    """Pointers are never dereferenced on these paths: aligned non-null integers stand in for device memory.  A null
    workspace and one that is a byte short: CDSEG_ERR_WORKSPACE (-3); a misaligned x: CDSEG_ERR_ARG (-1)."""
    p = ctypes.c_void_p
    buf, odd, odd2 = p(1 << 20), p((1 << 20) + 8), p((1 << 20) + 2)
    lin, conv, ln = lib.cdseg_linear_wgrad_det, lib.cdseg_conv_wgrad_det, lib.cdseg_layernorm_bwd_det
    M, K, N = 4100, 32, 96
    for dtype in (F32, LP16):
        need = lib.cdseg_wgrad_det_ws_bytes(M, N, K, 1, dtype)
        need27 = lib.cdseg_wgrad_det_ws_bytes(M, N, K, 27, dtype)
        assert need > 0 and need27 > need
        assert lin(buf, K, None, buf, N, 0, K, N, buf, K, None, dtype, None, 0, None) == 0            # m = 0: nothing to do
        assert lin(buf, K, None, buf, N, M, K, N, buf, K, buf, dtype, None, need, None) == -3         # null workspace
        assert lin(buf, K, None, buf, N, M, K, N, buf, K, buf, dtype, buf, need - 1, None) == -3      # one byte short
        assert conv(buf, K, buf, 27, buf, N, M, K, N, buf, buf, dtype, None, need27, None) == -3
        assert conv(buf, K, buf, 27, buf, N, M, K, N, buf, buf, dtype, buf, need27 - 1, None) == -3
        assert conv(buf, K, buf, 27, buf, N, M, K, N, buf, buf, dtype, buf, need, None) == -3         # the Linear form's size
        assert conv(buf, K, None, 27, buf, N, M, K, N, buf, buf, dtype, buf, need27, None) == -1      # no kernel map
        bad = odd if dtype == LP16 else odd2
        assert lin(bad, K, None, buf, N, M, K, N, buf, K, buf, dtype, buf, need, None) == -1          # misaligned x
        assert conv(bad, K, buf, 27, buf, N, M, K, N, buf, buf, dtype, buf, need27, None) == -1
        assert lin(None, K, None, buf, N, M, K, N, buf, K, buf, dtype, buf, need, None) == -1
        assert lin(buf, K, None, buf, N, M, K, N, buf, K, buf, dtype, odd, need + 8, None) == -1      # workspace not 16-byte aligned
        assert lin(buf, 40, None, buf, N, M, 40, N, buf, 40, buf, dtype, buf, 1 << 30, None) == -4    # k = 40
        assert lin(buf, K, None, buf, N, M, K, N, buf, K, buf, 7, buf, 1 << 30, None) == -4           # no such dtype
    assert lin(buf, 36, None, buf, N, M, K, N, buf, K, buf, LP16, buf, 1 << 30, None) == -1           # 16-bit: ldx % 8
    # LayerNorm
    need = lib.cdseg_layernorm_bwd_det_ws_bytes(5000, 32)
    assert ln(buf, 32, buf, 1e-5, buf, 32, buf, 32, 0, buf, buf, 0, 32, None, 0, None) == 0
    assert ln(buf, 32, buf, 1e-5, buf, 32, buf, 32, 0, buf, buf, 5000, 32, None, need, None) == -3
    assert ln(buf, 32, buf, 1e-5, buf, 32, buf, 32, 0, buf, buf, 5000, 32, buf, need - 1, None) == -3
    assert ln(None, 32, buf, 1e-5, buf, 32, buf, 32, 0, buf, buf, 5000, 32, buf, need, None) == -1
    assert ln(buf, 576, buf, 1e-5, buf, 576, buf, 576, 0, buf, buf, 5000, 576, buf, 1 << 30, None) == -4  # wider than 512
    # segment sum
    seg = lib.cdseg_segment_sum
    assert seg(buf, 32, buf, 0, 32, buf, 32, None) == 0
    assert seg(None, 32, buf, 10, 32, buf, 32, None) == -1 and seg(buf, 32, None, 10, 32, buf, 32, None) == -1


def test_ops_take_the_keyword_and_need_a_gpu():
    import inspect
    from cdsegnet_amd import ops
    for fn in (ops.linear_wgrad, ops.conv_wgrad, ops.layernorm_bwd):
        assert inspect.signature(fn).parameters["deterministic"].default is False
    if not torch.cuda.is_available():
        with pytest.raises(_lib.CdsegError):
            ops.segment_sum(torch.zeros(4, 16), torch.zeros(3, dtype=torch.int32), 2)


def test_mode_switch_follows_torch_unless_overridden():
    """train_deterministic: None follows torch.are_deterministic_algorithms_enabled(), True / False override; not a part of
    the state_dict; anything else raises."""
    from cdsegnet_amd import configs
    from cdsegnet_amd.registry import build_model
    from cdsegnet_amd.ops import det_kw as _det_kw
    from cdsegnet_amd.train_graph import resolve_deterministic
    import cdsegnet_amd.models  # noqa: F401
    model = build_model(configs.mini_config())
    assert model.train_deterministic is None and "train_deterministic" not in model.state_dict()
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        torch.use_deterministic_algorithms(False)
        assert resolve_deterministic(model) is False
        torch.use_deterministic_algorithms(True, warn_only=True)
        assert resolve_deterministic(model) is True
        model.train_deterministic = False
        assert resolve_deterministic(model) is False
        torch.use_deterministic_algorithms(False)
        model.train_deterministic = True
        assert resolve_deterministic(model) is True
        model.train_deterministic = "yes"
        with pytest.raises(ValueError, match="train_deterministic"):
            resolve_deterministic(model)
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn)
    assert _det_kw(False) == {} and _det_kw(True) == {"deterministic": True}  # (the default call carries no new keyword)


# ------------------------------------------------------------------------------------------ the order contract in numpy
def _replay(partials, into):
    """t = p[0]; t += p[1]; ...; into + t - every operation in fp32."""
    t = np.float32(partials[0])
    for p in partials[1:]:
        t = np.float32(t + np.float32(p))
    return np.float32(np.float32(into) + t)


def test_numpy_replay_of_the_reduce_order_on_the_cancellation_input():
    """One live row per split with products 2^24, 1, -2^24, 1 (dy = +-2^12, x = 2^12, and dy = x = 1): the documented order
    gives exactly 1.0 - (2^24 + 1) rounds back to 2^24 in fp32, the -2^24 cancels it, the last 1 survives.  Other orders of
    the same four numbers give 0.0 or 2.0, so the input tells the orders apart."""
    big = np.float32(2 ** 12) * np.float32(2 ** 12)
    assert big == np.float32(2 ** 24) and np.float32(2 ** 24) + np.float32(1) == np.float32(2 ** 24)
    parts = [big, np.float32(1), -big, np.float32(1)]
    assert _replay(parts, 0.0) == np.float32(1.0)
    assert _replay(parts, 5.0) == np.float32(6.0)                      # ONE add onto the existing content
    assert _replay([parts[0], parts[2], parts[1], parts[3]], 0.0) == np.float32(2.0)
    assert _replay([parts[0], parts[1], parts[3], parts[2]], 0.0) == np.float32(0.0)
    # adding every partial onto the existing content (what atomics do) is another sum than the total added once
    t = np.float32(5.0)
    for p in parts:
        t = np.float32(t + p)
    assert t != _replay(parts, 5.0)
    # the values are representable in both 16-bit types
    for t16 in (torch.float16, torch.bfloat16):
        assert float(torch.tensor(4096.0).to(t16)) == 4096.0 and float(torch.tensor(-4096.0).to(t16)) == -4096.0
