"""CPU: the boundary of the 16-bit weight gradient and of the AMP training modes - what can be checked without a device: the
entry points reject bad arguments before they launch anything, the binding mirrors the fp32 forms, the mode table."""
import ctypes

import pytest

from cdsegnet_amd import _lib


@pytest.fixture(params=list(_lib.VARIANTS))
def lib(request):
    return _lib.load(request.param)


def test_signatures_mirror_the_fp32_forms():
    for name in ("cdseg_linear_wgrad", "cdseg_conv_wgrad"):
        assert _lib.SIGNATURES[name + "16"] == _lib.SIGNATURES[name]


def test_entry_points_check_their_arguments_before_any_launch(lib):
    """Pointers are never dereferenced on these paths: aligned non-null integers stand in for device memory."""
    p = ctypes.c_void_p
    buf, odd = p(1 << 20), p((1 << 20) + 8)
    lin, conv = lib.cdseg_linear_wgrad16, lib.cdseg_conv_wgrad16
    assert lin(buf, 32, None, buf, 48, 0, 32, 48, buf, 32, None, None) == 0       # m = 0: nothing to do
    assert conv(buf, 32, buf, 27, buf, 48, 0, 32, 48, buf, None, None) == 0
    assert lin(buf, 36, None, buf, 48, 100, 32, 48, buf, 32, None, None) == -1    # ldx not a multiple of 8 elements
    assert lin(buf, 32, None, buf, 44, 100, 32, 48, buf, 32, None, None) == -1    # lddy
    assert lin(odd, 32, None, buf, 48, 100, 32, 48, buf, 32, None, None) == -1    # x not 16-byte aligned
    assert lin(buf, 32, None, odd, 48, 100, 32, 48, buf, 32, None, None) == -1    # dy
    assert lin(buf, 32, None, buf, 48, 100, 32, 48, odd, 32, None, None) == -1    # dw
    assert lin(buf, 32, odd, buf, 48, 100, 32, 48, buf, 32, None, None) == -1     # xidx
    assert lin(buf, 32, None, buf, 48, 100, 32, 48, buf, 32, odd, None) == -1     # db
    assert lin(None, 32, None, buf, 48, 100, 32, 48, buf, 32, None, None) == -1
    assert conv(buf, 36, buf, 27, buf, 48, 100, 32, 48, buf, None, None) == -1
    assert conv(buf, 32, None, 27, buf, 48, 100, 32, 48, buf, None, None) == -1   # a conv without its kernel map
    assert lin(buf, 32, None, buf, 24, 100, 32, 24, buf, 32, None, None) == -4    # n = 24: not a multiple of 16
    assert lin(buf, 40, None, buf, 48, 100, 40, 48, buf, 40, None, None) == -4    # k = 40
    assert conv(buf, 32, buf, 27, buf, 24, 100, 32, 24, buf, None, None) == -4
    assert conv(buf, 40, buf, 27, buf, 48, 100, 40, 48, buf, None, None) == -4


def test_train_precision_table():
    from cdsegnet_amd.train_graph import TRAIN_PRECISIONS
    assert TRAIN_PRECISIONS == {"fp32": None, "fp16-attn": "f16", "bf16-attn": "bf16", "fp16-amp": "f16", "bf16-amp": "bf16"}
    assert "fp16" not in TRAIN_PRECISIONS  # the bare name keeps raising ValueError at forward
