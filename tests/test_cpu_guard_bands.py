"""CPU: the guard-band helper itself (tests/guard_bands.py) on CPU tensors - a clean run passes, a write into each guard
region and each workspace band is reported with its coordinates, the alignment options hold, NaN guards stay outside."""
import pytest
import torch

from tests import guard_bands as GB

DTYPES = [torch.float32, torch.bfloat16, torch.float16]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("align", [0, 8])
def test_clean_run_passes_and_alignment_is_as_promised(dtype, align):
    inner, band = GB.banded((37, 20), dtype, fill=-3.0, align=align, device="cpu")
    assert tuple(inner.shape) == (37, 20) and inner.data_ptr() % 16 == align
    assert bool((inner == -3.0).all())
    inner.copy_(torch.randn(37, 20).to(dtype))  # the whole inner view, its corners included
    band.check()
    assert band.damaged() is None
    for which in ("front", "behind", "left", "right"):
        assert band.region(which).numel() > 0 and bool((band.region(which) == -3.0).all())
    assert band.region("front").shape[0] == 256 and band.region("behind").shape[0] == 256
    assert band.region("left").shape[1] >= 8 and band.region("right").shape[1] >= 8


def test_row_stride_option_and_the_stride_that_keeps_only_8_byte_alignment():
    es = 2
    inner, band = GB.banded((5, 36), torch.bfloat16, fill=1.0, ld=36 + 8 + 8 + 8, device="cpu")
    assert inner.stride(0) == 60 and inner.data_ptr() % 16 == 0
    assert (inner.stride(0) * es) % 16 == 8 and inner[1].data_ptr() % 16 == 8  # ld % 4 == 0 only: rows alternate 0 / 8
    band.check()
    with pytest.raises(AssertionError):
        GB.banded((5, 36), torch.bfloat16, fill=1.0, ld=40, device="cpu")  # no room for the guard columns


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_write_into_each_guard_region_is_reported_with_its_coordinates(dtype):
    n, c, rows = 9, 12, 256
    for which, (r, col) in {"front": (rows - 1, 11), "behind": (rows + n, 10), "left": (rows + 4, 7), "right": (rows + 4, 20)}.items():
        inner, band = GB.banded((n, c), dtype, fill=-777.25, device="cpu")
        c0 = band.c0
        assert c0 == 8  # 8 guard columns are whole 16-byte groups of both element sizes
        band.buf[r, col] = 5.0
        d = band.damaged()
        assert d == (r, col, which, 1), (which, d)
        with pytest.raises(AssertionError) as e:
            band.check()
        msg = str(e.value)
        assert f"(row {r}, column {col})" in msg and f"inner (row {r - rows}, column {col - c0})" in msg and f"'{which}'" in msg


def test_damage_is_compared_as_bits():
    inner, band = GB.banded((4, 8), torch.float32, fill=0.0, device="cpu")
    band.buf[0, 0] = -0.0  # equal as a number, different bits
    assert band.damaged() == (0, 0, "front", 1)
    inner, band = GB.banded((4, 8), torch.float32, fill=float("nan"), device="cpu")
    band.check()  # NaN guards equal themselves as bits
    band.buf[-1, -1] = 0.0
    assert band.damaged()[2] == "behind"


def test_first_damaged_element_is_named_when_there_are_several():
    inner, band = GB.banded((4, 8), torch.float16, fill=2.0, device="cpu")
    band.buf[300, 3] = 0.0
    band.buf[10, 5] = 0.0
    band.buf[10, 2] = 0.0
    assert band.damaged() == (10, 2, "front", 3)


@pytest.mark.parametrize("nbytes", [0, 16, 1000, 4096 * 100 + 16])
def test_exact_workspace_is_exact_aligned_and_reports_both_bands(nbytes):
    view, band = GB.exact_workspace(nbytes, device="cpu")
    assert view.numel() == nbytes and view.data_ptr() % 256 == 0 and view.dtype == torch.uint8
    guard = max(64 << 10, nbytes // 4)
    assert band.start >= guard and band.buf.numel() - band.start - nbytes >= guard
    assert bool((band.buf == 0xA5).all())
    view.zero_()  # every byte of the view, the first and the last included
    band.check()
    band.buf[band.start - 3] = 0
    assert band.damaged() == ("front", -3, 1)
    with pytest.raises(AssertionError, match="3 byte\\(s\\) in front"):
        band.check()
    band.buf[band.start - 3] = 0xA5
    band.buf[band.start + nbytes + 5] = 1
    assert band.damaged() == ("behind", 5, 1)
    with pytest.raises(AssertionError, match="at byte 5 behind its end"):
        band.check()


def test_exact_workspaces_serves_fresh_exact_views():
    ws = GB.ExactWorkspaces()
    a, b = ws(100, "cpu"), ws(100, "cpu")
    assert a.numel() == b.numel() == 100 and a.data_ptr() != b.data_ptr()
    ws.check(at_least=2)
    with pytest.raises(AssertionError):
        ws.check(at_least=3)
    ws.served[1].buf[0] = 0
    with pytest.raises(AssertionError):
        ws.check()


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_in_a_poisoned_guard_does_not_reach_the_inner_view(dtype):
    t = torch.randn(11, 24).to(dtype)
    inner, band = GB.poisoned_input(t, align=8 if dtype != torch.float32 else 0, ld=48)
    assert GB.same_bits(inner, t) and bool(torch.isfinite(inner).all()) and inner.stride(0) == 48
    for which in ("front", "behind", "left", "right"):
        assert bool(torch.isnan(band.region(which)).all())
    band.check()
    # a reduction over the inner view alone is finite; over the whole buffer it is not
    assert bool(torch.isfinite(inner.float().sum())) and not bool(torch.isfinite(band.buf.float().sum()))
    with pytest.raises(AssertionError):
        GB.poisoned_input(torch.arange(4).view(2, 2))  # index operands are never poisoned


def test_guard_index_holds_valid_entries():
    idx = torch.tensor([3, 1, 4, 1, 5], dtype=torch.int32)
    inner, check = GB.guard_index(idx, rows=4)
    assert torch.equal(inner, idx)
    whole = torch.cat([torch.full((4,), 3, dtype=torch.int32), idx, torch.full((4,), 5, dtype=torch.int32)])
    assert inner.data_ptr() == inner._base.data_ptr() + 16 and torch.equal(inner._base, whole)
    check()
    inner2, check2 = GB.guard_index(idx.view(5, 1).expand(5, 3).contiguous(), none=-1, rows=2)
    assert bool((inner2._base[:2] == -1).all()) and bool((inner2._base[-2:] == -1).all())
    inner2._base[0, 0] = 7
    with pytest.raises(AssertionError):
        check2()


@pytest.mark.parametrize("dtype,align", [(torch.float32, 0), (torch.float32, 4), (torch.float32, 8), (torch.float32, 12),
                                         (torch.float64, 0), (torch.float64, 8), (torch.bfloat16, 2), (torch.float16, 8)])
@pytest.mark.parametrize("n", [1, 5, 4096])
def test_banded_vector_has_the_alignment_class_asked_for_and_reports_both_sides(dtype, align, n):
    inner, band = GB.banded_vector(n, dtype, fill=-3.0, align=align, device="cpu")
    assert inner.dim() == 1 and inner.numel() == n and inner.is_contiguous() and inner.data_ptr() % 16 == align
    assert band.region("left").numel() >= 256 and band.region("right").numel() >= 256
    assert band.region("front").numel() == 0 and band.region("behind").numel() == 0
    inner.copy_(torch.randn(n).to(dtype))  # every element, the first and the last included
    band.check()
    c0 = band.c0
    band.buf[0, c0 - 1] = 1.0
    assert band.damaged() == (0, c0 - 1, "left", 1)
    with pytest.raises(AssertionError, match="inner \\(row 0, column -1\\), in the 'left' guard"):
        band.check()
    band.buf[0, c0 - 1] = -3.0
    band.buf[0, c0 + n] = 1.0
    assert band.damaged() == (0, c0 + n, "right", 1)
    with pytest.raises(AssertionError, match=f"inner \\(row 0, column {n}\\), in the 'right' guard"):
        band.check()


def test_banded_vector_refuses_an_alignment_the_element_size_cannot_have():
    for dtype, align in ((torch.float32, 2), (torch.float64, 4), (torch.float32, 16)):
        with pytest.raises(AssertionError):
            GB.banded_vector(8, dtype, fill=0.0, align=align, device="cpu")


def test_poisoned_vector_keeps_the_values_between_nan_guards():
    t = torch.randn(37, dtype=torch.float64)
    inner, band = GB.poisoned_vector(t, align=8)
    assert GB.same_bits(inner, t) and inner.data_ptr() % 16 == 8
    assert bool(torch.isnan(band.region("left")).all()) and bool(torch.isnan(band.region("right")).all())
    band.check()
    with pytest.raises(AssertionError):
        GB.poisoned_vector(torch.arange(4))  # index operands are never poisoned
    with pytest.raises(AssertionError):
        GB.poisoned_vector(torch.zeros(2, 2))


def test_banded_admits_the_4_byte_alignment_class_of_fp32_with_an_odd_row_stride():
    inner, band = GB.banded((5, 16), torch.float32, fill=2.0, cols=0, align=4, ld=17, device="cpu")
    assert inner.data_ptr() % 16 == 4 and inner.stride(0) == 17 and band.c0 == 1
    inner.zero_()
    band.check()
    band.buf[256 + 2, 0] = 0.0  # the one guard column in front of row 2 (= the element behind row 1)
    assert band.damaged() == (258, 0, "left", 1)
