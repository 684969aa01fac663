"""CPU: the fp32 training entry points (csrc/train.hip cdseg_linear_wgrad, cdseg_conv_wgrad, cdseg_layernorm_bwd,
cdseg_gelu_bwd) reject bad arguments before they launch anything, like their 16-bit and deterministic forms
(tests/test_cpu_wgrad16.py, tests/test_cpu_deterministic.py), in both builds.

Runs only where torch sees no device: the pointers are stand-in integers, and a check that has regressed would LAUNCH on
them.  Without a device that shows up as another error code; with one it would be a write through a wild pointer.
"""
import ctypes

import pytest
import torch

from cdsegnet_amd import _lib

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="stand-in pointers: only where nothing can be launched")

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4


@pytest.fixture(params=list(_lib.VARIANTS))
def lib(request):
    return _lib.load(request.param)


P = ctypes.c_void_p
BUF, ODD = P(1 << 20), P((1 << 20) + 2)  # (4-byte aligned; 2 bytes off)


def test_linear_wgrad_checks_its_arguments_before_any_launch(lib):
    lin = lib.cdseg_linear_wgrad
    # (x, ldx, xidx, dy, lddy, m, k, n, dw, lddw, db, stream)
    assert lin(BUF, 32, None, BUF, 48, 0, 32, 48, BUF, 32, None, None) == OK      # m = 0: nothing to do
    assert lin(None, 32, None, None, 48, 0, 32, 48, None, 32, None, None) == OK   # (before the pointers are looked at)
    assert lin(BUF, 32, None, BUF, 48, 100, 0, 48, BUF, 32, None, None) == OK     # k = 0
    assert lin(BUF, 32, None, BUF, 48, 100, 32, 0, BUF, 32, None, None) == OK     # n = 0
    assert lin(None, 32, None, BUF, 48, 100, 32, 48, BUF, 32, None, None) == ERR_ARG  # x
    assert lin(BUF, 32, None, None, 48, 100, 32, 48, BUF, 32, None, None) == ERR_ARG  # dy
    assert lin(BUF, 32, None, BUF, 48, 100, 32, 48, None, 32, None, None) == ERR_ARG  # dw
    assert lin(ODD, 32, None, BUF, 48, 100, 32, 48, BUF, 32, None, None) == ERR_ARG
    assert lin(BUF, 32, None, ODD, 48, 100, 32, 48, BUF, 32, None, None) == ERR_ARG
    assert lin(BUF, 32, None, BUF, 48, 100, 32, 48, ODD, 32, None, None) == ERR_ARG
    assert lin(BUF, 32, ODD, BUF, 48, 100, 32, 48, BUF, 32, None, None) == ERR_ARG   # xidx
    assert lin(BUF, 32, None, BUF, 48, 100, 32, 48, BUF, 32, ODD, None) == ERR_ARG   # db
    assert lin(BUF, 32, None, BUF, 24, 100, 32, 24, BUF, 32, None, None) == ERR_UNSUPPORTED  # n = 24: not a multiple of 16
    assert lin(BUF, 40, None, BUF, 48, 100, 40, 48, BUF, 40, None, None) == ERR_UNSUPPORTED  # k = 40
    assert lin(None, 40, None, BUF, 48, 100, 40, 48, BUF, 40, None, None) == ERR_ARG  # (the pointers come first, as in the 16-bit form)


def test_conv_wgrad_checks_its_arguments_before_any_launch(lib):
    conv = lib.cdseg_conv_wgrad
    # (x, ldx, nbr_kmajor, kvol, dy, lddy, m, cin, cout, dw, db, stream)
    assert conv(BUF, 32, BUF, 27, BUF, 48, 0, 32, 48, BUF, None, None) == OK
    assert conv(BUF, 32, BUF, 0, BUF, 48, 100, 32, 48, BUF, None, None) == OK
    assert conv(BUF, 32, None, 27, BUF, 48, 100, 32, 48, BUF, None, None) == ERR_ARG  # a conv without its kernel map
    assert conv(None, 32, BUF, 27, BUF, 48, 100, 32, 48, BUF, None, None) == ERR_ARG
    assert conv(BUF, 32, BUF, 27, None, 48, 100, 32, 48, BUF, None, None) == ERR_ARG
    assert conv(BUF, 32, BUF, 27, BUF, 48, 100, 32, 48, None, None, None) == ERR_ARG
    assert conv(ODD, 32, BUF, 27, BUF, 48, 100, 32, 48, BUF, None, None) == ERR_ARG
    assert conv(BUF, 32, ODD, 27, BUF, 48, 100, 32, 48, BUF, None, None) == ERR_ARG
    assert conv(BUF, 32, BUF, 27, ODD, 48, 100, 32, 48, BUF, None, None) == ERR_ARG
    assert conv(BUF, 32, BUF, 27, BUF, 48, 100, 32, 48, ODD, None, None) == ERR_ARG
    assert conv(BUF, 32, BUF, 27, BUF, 48, 100, 32, 48, BUF, ODD, None) == ERR_ARG
    assert conv(BUF, 32, BUF, 27, BUF, 24, 100, 32, 24, BUF, None, None) == ERR_UNSUPPORTED
    assert conv(BUF, 40, BUF, 27, BUF, 48, 100, 40, 48, BUF, None, None) == ERR_UNSUPPORTED


def test_layernorm_bwd_checks_its_arguments_before_any_launch(lib):
    ln = lib.cdseg_layernorm_bwd
    # (x, ldx, gamma, eps, dy, lddy, dx, lddx, accumulate, dgamma, dbeta, m, c, stream)
    assert ln(BUF, 96, BUF, 1e-5, BUF, 96, BUF, 96, 0, None, None, 0, 96, None) == OK
    assert ln(BUF, 96, BUF, 1e-5, BUF, 96, BUF, 96, 0, None, None, 10, 0, None) == ERR_ARG   # c <= 0
    assert ln(BUF, 96, BUF, 1e-5, BUF, 96, BUF, 96, 0, None, None, 10, -16, None) == ERR_ARG
    for i in (0, 2, 4, 6):  # x, gamma, dy, dx: required
        a = [BUF, 96, BUF, 1e-5, BUF, 96, BUF, 96, 0, BUF, BUF, 10, 96, None]
        a[i] = None
        assert ln(*a) == ERR_ARG, i
    for i in (0, 2, 4, 6, 9, 10):  # ... and dgamma, dbeta: 4-byte aligned
        a = [BUF, 96, BUF, 1e-5, BUF, 96, BUF, 96, 1, BUF, BUF, 10, 96, None]
        a[i] = ODD
        assert ln(*a) == ERR_ARG, i


def test_gelu_bwd_checks_its_arguments_before_any_launch(lib):
    gelu = lib.cdseg_gelu_bwd
    assert gelu(BUF, BUF, BUF, 0, None) == OK
    assert gelu(None, None, None, -5, None) == OK
    for i in range(3):
        a = [BUF, BUF, BUF, 100, None]
        a[i] = None
        assert gelu(*a) == ERR_ARG, i
        a[i] = ODD
        assert gelu(*a) == ERR_ARG, i
