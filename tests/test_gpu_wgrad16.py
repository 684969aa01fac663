"""GPU: the 16-bit weight gradient (csrc/train.hip wgrad16_kernel; cdseg_linear_wgrad16 / cdseg_conv_wgrad16), both builds.

The main check is exact: integer operands in [-3, 3] are exact in bfloat16 and in half, every product is an integer and every
sum stays far below 2^24, so fp32 accumulation is exact in ANY order and dw / db must EQUAL the integer result (computed in
fp64, which is exact on these integers, and compared as int64).  Ordinary values are checked against fp64 with the unchanged
fp32 kernel's own error as the yardstick.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests.helpers import load_fixture
from tests.test_gpu_ops import LP, _library_variant, _physical, dev, ops, report  # noqa: F401  (fixtures: lp="f16" -> the half build)

pytestmark = pytest.mark.gpu

LPS = pytest.mark.parametrize("lp", ["bf16", "f16"])


def _ints(rng, *shape):
    return torch.as_tensor(rng.integers(-3, 4, size=shape)).float()


def _exact(dy, x, xidx=None):
    """(dw, db) as int64: fp64 products and sums of small integers are exact."""
    dy, x = dy.double(), x.double()
    if xidx is not None:
        live = (xidx >= 0).double()[:, None]
        x = x[xidx.clamp(min=0).long()] * live
    return (dy.T @ x).round().long(), dy.sum(0).round().long()


def _eq(got, want):
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all())
    return bool((got.round().long() == want.cpu()).all()) and bool((got == got.round()).all())


DENSE = [(1, 16, 16), (17, 16, 48), (33, 32, 96), (1023, 64, 192), (1025, 64, 256), (4097, 128, 128), (5003, 32, 96),
         (2049, 512, 64), (700, 512, 2048)]


@LPS
@pytest.mark.parametrize("M,K,N", DENSE, ids=[f"{m}x{k}x{n}" for m, k, n in DENSE])
def test_dense_exact_on_integers(ops, lp, M, K, N):
    """Contiguous operands, then strided ones: dy and x column slices of wider 16-bit buffers, dw a view with lddw > k."""
    rng = np.random.default_rng(M + 7 * K + 13 * N)
    x, dy = _ints(rng, M, K), _ints(rng, M, N)
    want_w, want_b = _exact(dy, x)
    x16, dy16 = dev(x, LP()), dev(dy, LP())
    dw = torch.zeros(N, K, device="cuda")
    db = torch.zeros(N, device="cuda")
    ops.linear_wgrad(x16, dy16, dw, db)
    torch.cuda.synchronize()
    assert _eq(dw, want_w) and _eq(db, want_b)
    xw = dev(_ints(rng, M, K + 24), LP())
    dyw = dev(_ints(rng, M, N + 16), LP())
    xw[:, 8:8 + K] = x16
    dyw[:, 16:] = dy16
    wide = torch.zeros(N, K + 12, device="cuda")
    db2 = torch.zeros(N, device="cuda")
    ops.linear_wgrad(xw[:, 8:8 + K], dyw[:, 16:], wide[:, 4:4 + K], db2)
    torch.cuda.synchronize()
    assert _eq(wide[:, 4:4 + K], want_w) and _eq(db2, want_b)
    assert float(wide[:, :4].abs().max()) == 0 and float(wide[:, 4 + K:].abs().max()) == 0


@LPS
@pytest.mark.parametrize("M,R,K,N", [(1000, 300, 32, 96), (4500, 5000, 64, 64), (130, 64, 16, 16), (2100, 900, 128, 48)])
def test_gathered_exact_on_integers(ops, lp, M, R, K, N):
    """xidx with -1 entries, repeated rows and a stretch of consecutive -1 that covers whole 64-row chunks (the skip path);
    the bias gradient still counts the rows of the skipped chunks."""
    rng = np.random.default_rng(M + R)
    x, dy = _ints(rng, R, K), _ints(rng, M, N)
    idx = rng.integers(0, R, size=M)
    idx[rng.random(M) < 0.3] = -1
    idx[5:9] = idx[4]
    a = min(64, M // 4)
    idx[a:a + min(M // 2, 200)] = -1  # >= 64 consecutive, from a chunk boundary on when M allows
    idx = torch.as_tensor(idx, dtype=torch.int32)
    want_w, want_b = _exact(dy, x, idx)
    dw = torch.zeros(N, K, device="cuda")
    db = torch.zeros(N, device="cuda")
    ops.linear_wgrad(dev(x, LP()), dev(dy, LP()), dw, db, xidx=idx.cuda())
    dw_nob = torch.zeros(N, K, device="cuda")
    ops.linear_wgrad(dev(x, LP()), dev(dy, LP()), dw_nob, None, xidx=idx.cuda())  # (without db the dead chunks ARE skipped)
    torch.cuda.synchronize()
    assert _eq(dw, want_w) and _eq(db, want_b) and _eq(dw_nob, want_w)


_MAPS = {}


def _kernel_map(ops, name, ksize):
    """Offset-major kernel map of a fixture cloud (computed once per cloud and size, never modified)."""
    if (name, ksize) not in _MAPS:
        fx = load_fixture(f"serialization_{name}.npz")
        zs, perm0, g0, b0, depth, p = _physical(ops, fx)
        _MAPS[(name, ksize)] = ops.nbr_table(zs, g0, b0, depth, ksize, True).contiguous()
    return _MAPS[(name, ksize)]


CONV = [(16, 16, 3), (32, 32, 3), (64, 64, 3), (128, 128, 3), (16, 32, 5)]


@LPS
@pytest.mark.parametrize("name", ["room1500", "batch2"])
@pytest.mark.parametrize("cin,cout,ksize", CONV, ids=[f"{a}-{b}-k{k}" for a, b, k in CONV])
def test_conv_form_exact_on_integers(ops, lp, name, cin, cout, ksize):
    """All kvol offsets in one launch on a real kernel map == the loop over offsets == kvol calls of the linear form on
    dw3[:, o, :]; db = the column sums of dy.  (16, 32, 5) is the stem: 6 channels padded to 16 with ten zero channels."""
    nbr = _kernel_map(ops, name, ksize)
    kvol, M = nbr.shape
    assert kvol == ksize ** 3
    rng = np.random.default_rng(cin + cout + kvol)
    x, dy = _ints(rng, M, cin), _ints(rng, M, cout)
    if ksize == 5:
        x[:, 6:] = 0
    x16, dy16 = dev(x, LP()), dev(dy, LP())
    dw3 = torch.zeros(cout, kvol, cin, device="cuda")
    db = torch.zeros(cout, device="cuda")
    ops.conv_wgrad(x16, nbr, dy16, dw3, db)
    torch.cuda.synchronize()
    nb = nbr.cpu()
    for o in range(kvol):
        want_w, _ = _exact(dy, x, nb[o])
        assert _eq(dw3[:, o, :], want_w), o
    assert _eq(db, dy.double().sum(0).long())
    lin = torch.zeros(cout, kvol, cin, device="cuda")
    for o in range(kvol if ksize == 3 else 27):  # (the stem: the first 27 of its 125 offsets)
        ops.linear_wgrad(x16, dy16, lin[:, o, :], None, xidx=nbr[o])
    torch.cuda.synchronize()
    n = kvol if ksize == 3 else 27
    assert bool((lin[:, :n] == dw3[:, :n]).all())


@LPS
def test_accumulates_into_dw_and_db(ops, lp):
    rng = np.random.default_rng(2)
    M, K, N = 777, 48, 80
    x, dy = _ints(rng, M, K), _ints(rng, M, N)
    want_w, want_b = _exact(dy, x)
    pre_w, pre_b = _ints(rng, N, K) * 5, _ints(rng, N) * 7
    dw, db = pre_w.cuda().clone(), pre_b.cuda().clone()
    x16, dy16 = dev(x, LP()), dev(dy, LP())
    ops.linear_wgrad(x16, dy16, dw, db)
    torch.cuda.synchronize()
    assert _eq(dw, pre_w.long() + want_w) and _eq(db, pre_b.long() + want_b)
    ops.linear_wgrad(x16, dy16, dw, db)
    torch.cuda.synchronize()
    assert _eq(dw, pre_w.long() + 2 * want_w) and _eq(db, pre_b.long() + 2 * want_b)


def _metric(g, g64):
    return float((g.double().cpu() - g64).abs().max()) / float(g64.abs().max())


@LPS
@pytest.mark.parametrize("M,K,N", [(20000, 64, 192), (1500, 512, 512)])
def test_fp32_accumulation_on_ordinary_values(ops, lp, M, K, N):
    """Gaussian x, dy = 0.1 N(0, 1), rounded to the 16-bit type; oracle fp64 on the rounded values.  Bound: 3 x E32, the same
    metric of the unchanged fp32 kernel on the same (widened) values: both kernels add the same exactly representable products
    in fp32 in different orders, which the factor covers; a 16-bit rounding of any partial sum would be hundreds of E32."""
    g = torch.Generator().manual_seed(M + K)
    x16 = torch.randn(M, K, generator=g).to(LP())
    dy16 = (0.1 * torch.randn(M, N, generator=g)).to(LP())
    w64, b64 = dy16.double().T @ x16.double(), dy16.double().sum(0)
    out = {}
    for name, t in (("fp32", torch.float32), ("16-bit", LP())):
        dw = torch.zeros(N, K, device="cuda")
        db = torch.zeros(N, device="cuda")
        ops.linear_wgrad(x16.cuda().to(t), dy16.cuda().to(t), dw, db)
        torch.cuda.synchronize()
        out[name] = (_metric(dw, w64), _metric(db, b64))
    (e32w, e32b), (e16w, e16b) = out["fp32"], out["16-bit"]
    report(f"wgrad16 {M}x{K}x{N} ({lp})", E32_dw=e32w, err16_dw=e16w, E32_db=e32b, err16_db=e16b)
    assert e16w <= 3 * e32w, (e16w, e32w)
    assert e16b <= 3 * e32b, (e16b, e32b)


@LPS
def test_overflow_in_dy_is_visible_in_half_and_finite_in_bfloat16(ops, lp):
    """One dy element is what the unsaturated cast of 1e6 gives (inf in half, 1e6 in bfloat16): an arithmetic inf, which must
    show in that column's dw row and db entry and nowhere else."""
    rng = np.random.default_rng(4)
    M, K, N = 300, 32, 48
    x, dy = _ints(rng, M, K), _ints(rng, M, N)
    x[:, 0] = 1  # (no 0 * inf in the affected row's first column: inf, not only NaN)
    dy[123, 21] = 1e6
    dy16 = dy.to(LP())
    assert bool(torch.isinf(dy16[123, 21])) == (lp == "f16")
    dw = torch.zeros(N, K, device="cuda")
    db = torch.zeros(N, device="cuda")
    ops.linear_wgrad(dev(x, LP()), dy16.cuda(), dw, db)
    torch.cuda.synchronize()
    fw, fb = torch.isfinite(dw).cpu(), torch.isfinite(db).cpu()
    other = torch.ones(N, dtype=torch.bool)
    other[21] = False
    assert bool(fw[other].all()) and bool(fb[other].all())
    if lp == "f16":
        assert not bool(fw[21].any()) and not bool(fb[21])
    else:
        assert bool(fw.all()) and bool(fb.all())


@LPS
def test_argument_checks(ops, lp):
    from cdsegnet_amd import _lib
    lpt = LP()
    other = torch.bfloat16 if lpt == torch.float16 else torch.float16
    rng = np.random.default_rng(1)
    M, K, N = 100, 32, 48
    x, dy = _ints(rng, M, K), _ints(rng, M, N)
    x16, dy16 = dev(x, lpt), dev(dy, lpt)
    dw = torch.zeros(N, K, device="cuda")
    with pytest.raises(_lib.CdsegError, match="share a dtype"):
        ops.linear_wgrad(x16, dy.cuda(), dw)
    with pytest.raises(_lib.CdsegError, match="share a dtype"):
        ops.linear_wgrad(x.cuda(), dy16, dw)
    with pytest.raises(_lib.CdsegError, match="do not belong to the active build"):
        ops.linear_wgrad(dev(x, other), dev(dy, other), dw)
    with pytest.raises(_lib.CdsegError, match="fp32"):
        ops.linear_wgrad(x16, dy16, torch.zeros(N, K, dtype=lpt, device="cuda"))
    nbr = torch.full((27, M), -1, dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.CdsegError, match="share a dtype"):
        ops.conv_wgrad(x16, nbr, dy.cuda(), torch.zeros(N, 27, K, device="cuda"))
    with pytest.raises(_lib.CdsegError, match="fp32"):
        ops.conv_wgrad(x16, nbr, dy16, torch.zeros(N, 27, K, dtype=lpt, device="cuda"))
    wide = torch.zeros(M, K + 4, dtype=lpt, device="cuda")  # rows of K + 4 elements: 8- but not 16-byte aligned
    with pytest.raises(_lib.CdsegError, match="16-byte aligned"):
        ops.linear_wgrad(wide[:, :K], dy16, dw)
    # the entry point checks the same rules itself
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    dy24 = torch.zeros(M, 24, dtype=lpt, device="cuda")
    assert lib.cdseg_linear_wgrad16(p(wide), K + 4, None, p(dy16), N, M, K, N, p(dw), K, None, None) == -1  # CDSEG_ERR_ARG
    assert lib.cdseg_linear_wgrad16(p(x16), K, None, p(dy24), 24, M, K, 24, p(dw), K, None, None) == -4  # CDSEG_ERR_UNSUPPORTED
    assert lib.cdseg_conv_wgrad16(p(x16), K, p(nbr), 27, p(dy24), 24, M, K, 24, p(dw), None, None) == -4
    assert lib.cdseg_linear_wgrad16(p(x16), K, None, p(dy16), N, 0, K, N, p(dw), K, None, None) == 0  # empty: nothing written
    torch.cuda.synchronize()
    assert float(dw.abs().max()) == 0
    ops.linear_wgrad(x.cuda(), dy.cuda(), dw)  # fp32 calls behave as before
    torch.cuda.synchronize()
    assert _eq(dw, _exact(dy, x)[0])
