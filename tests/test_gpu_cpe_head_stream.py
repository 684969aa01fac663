"""GPU: the wide-stage Block head as a persistent, pipelined kernel (csrc/mlp.hip, cpe_head_stream_kernel).

From 65 536 rows upward cdseg_cpe_head_fused runs min(tiles, 512) persistent workgroups over 128-row tiles, with the
weights and parameter vectors resident in LDS and the next tile's rows in flight; below, the one-tile-per-workgroup 64-row
kernel.  Every output element is the same chain of MFMA products in the same order, the row statistics are the same sums
and the rounding points are the same, so the results must agree BIT for BIT with both references.  No tolerance anywhere.

References, the same for every case:
  (a) the ops.gemm sequence of test_cpe_head_fused_equals_linear_ln_qkv_sequence (cpe Linear with LN_cpe + residual +
      t bias + LN1 in its epilogue, then the qkv Linear);
  (b) the same rows through ops.cpe_head_fused in chunks of fewer than 65 536 rows: the 64-row kernel.
With CDSEG_ATTN_V_BF16 (IEEE-half build) the GEMM writes no bfloat16 v, so the v third is compared with (b) alone.

Sizes.  65 536 is the first n on the new path, 65 535 the last on the old one.  The grid is min(tiles, 512) workgroups
(2 per CU): n = 300 001 is 2 344 tiles of 128 rows = 4 or 5 tiles per workgroup (unequal trip counts, the rule asked for
being "some workgroups run three or more") with a 97-row last tile; 300 001 + 64 at C = 32 ends in a 33-row tile; 300 033
= 2 344 * 128 + 1 ends in a ONE-row tile of the 128-row form.
"""
import pytest
import torch

from tests.test_gpu_ops import LP, LPS, _library_variant, dev, ops  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

CHUNK = 65000  # rows per reference launch of (b): below the 65 536-row threshold
PAD = 256      # sentinel rows behind row n


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _case(ops, lp, n, C, tb):
    """Inputs and both references for one (build, n, C, t bias): computed once per case, shared by all its checks (plain
    call, repeated call, strided views), never written to."""
    bf = LP()
    g = torch.Generator(device="cuda").manual_seed(n * 5 + C + tb)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    d = dict(y=r(n, C).to(bf), wl=(r(C, C) / C ** 0.5).to(bf), wq=(r(3 * C, C) / C ** 0.5).to(bf), bl=r(C), bq=r(3 * C),
             lnp=(r(C), r(C)), ln1=(r(C), r(C)), cb=r(C) if tb else None, x0=r(n, C))
    # (a)
    xa = d["x0"].clone()
    h = torch.empty(n, C, dtype=bf, device="cuda")
    ops.gemm(d["y"], d["wl"], xa, bias=d["bl"], ln_pre=d["lnp"], res=xa, colbias=d["cb"], ln_post=d["ln1"], ln_out=h)
    qa = torch.empty(n, 3 * C, dtype=bf, device="cuda")
    ops.gemm(h, d["wq"], qa, bias=d["bq"])
    # (b), without and (half build) with the v third as bfloat16
    flagsets = [0, ops.ATTN_V_BF16] if lp == "f16" else [0]
    xb, qb = d["x0"].clone(), {f: torch.empty(n, 3 * C, dtype=bf, device="cuda") for f in flagsets}
    for f in flagsets:
        xb.copy_(d["x0"])
        with ops.record_routes() as rr:
            for a in range(0, n, CHUNK):
                b = min(a + CHUNK, n)
                ops.cpe_head_fused(d["y"][a:b], d["wl"], d["bl"], d["lnp"], xb[a:b], d["cb"], d["ln1"], d["wq"], d["bq"], qb[f][a:b],
                                   qkv_flags=f)
        assert rr.count == -(-n // CHUNK) and set(rr.kernels()) == {f"cpe_head_fused_kernel<{C},64>"}, rr.routes
    torch.cuda.synchronize()
    d.update(xa=xa, qa=qa, xb=xb, qb=qb, flagsets=flagsets)
    return d


def _run(ops, d, x, qkv, y=None, flags=0):
    ops.cpe_head_fused(d["y"] if y is None else y, d["wl"], d["bl"], d["lnp"], x, d["cb"], d["ln1"], d["wq"], d["bq"], qkv,
                       qkv_flags=flags)


def _check(d, C, x, qkv, flags, what):
    assert _same(x, d["xa"]), f"{what}: x differs from the GEMM sequence"
    assert _same(x, d["xb"]), f"{what}: x differs from the 64-row kernel"
    assert _same(qkv, d["qb"][flags]), f"{what}: qkv differs from the 64-row kernel"
    cols = 2 * C if flags else 3 * C  # (a) has no bfloat16 v
    assert _same(qkv[:, :cols].contiguous(), d["qa"][:, :cols].contiguous()), f"{what}: qkv differs from the GEMM sequence"


SIZES = [(65536, 64), (65535, 64), (65536, 32), (65535, 32), (300001, 64), (300001 + 64, 32), (300033, 64), (300033, 32)]


@LPS
@pytest.mark.parametrize("tb", [True, False], ids=["tbias", "no-tbias"])
@pytest.mark.parametrize("n,C", SIZES)
def test_stream_head_equals_gemm_sequence_and_64_row_kernel_bit_for_bit(ops, lp, n, C, tb):
    d = _case(ops, lp, n, C, tb)
    bf = LP()
    for flags in d["flagsets"]:
        x, qkv = d["x0"].clone(), torch.full((n, 3 * C), float("nan"), dtype=bf, device="cuda")
        with ops.record_routes() as rr:
            _run(ops, d, x, qkv, flags=flags)
        # the launch record: the persistent kernel from 65 536 rows, the 64-row kernel one row below
        want = (f"cpe_head_stream_kernel<{C}>", 128) if n >= 65536 else (f"cpe_head_fused_kernel<{C},64>", 64)
        assert [(r.kernel, r.aux) for r in rr.routes] == [want], (n, C, rr.routes)
        _check(d, C, x, qkv, flags, f"flags={flags}")
        # the same call again: equal bits
        x2, qkv2 = d["x0"].clone(), torch.full((n, 3 * C), float("nan"), dtype=bf, device="cuda")
        _run(ops, d, x2, qkv2, flags=flags)
        assert _same(x, x2) and _same(qkv, qkv2), "two calls on the same inputs differ"
    _strided_views_and_sentinel_rows(ops, d, n, C)


def _strided_views_and_sentinel_rows(ops, d, n, C):
    """x with ldx = C + 4, qkv a column slice (8-byte aligned, not 16) of a buffer with ldqkv = 3C + 8, y a row-offset view
    (16-byte aligned base, not a tile multiple); 256 sentinel rows behind row n and the padding columns stay untouched."""
    bf = LP()
    flags = d["flagsets"][-1]
    ybuf = torch.empty(n + 3, C, dtype=bf, device="cuda")
    ybuf[3:].copy_(d["y"])
    y = ybuf[3:]
    xbuf = torch.full((n + PAD, C + 4), -777.25, device="cuda")
    xbuf[:n, :C].copy_(d["x0"])
    qbuf = torch.full((n + PAD, 3 * C + 8), -3.0, dtype=bf, device="cuda")
    x, qkv = xbuf[:n, :C], qbuf[:n, 4:4 + 3 * C]
    assert x.stride(0) == C + 4 and qkv.stride(0) == 3 * C + 8 and y.data_ptr() % 16 == 0 and qkv.data_ptr() % 16 == 8
    _run(ops, d, x, qkv, y=y, flags=flags)
    torch.cuda.synchronize()
    _check(d, C, x.contiguous(), qkv.contiguous(), flags, "strided")
    assert bool((xbuf[n:] == -777.25).all()) and bool((xbuf[:, C:] == -777.25).all()), "x written outside its rows / columns"
    assert bool((qbuf[n:] == -3.0).all()) and bool((qbuf[:, :4] == -3.0).all()) and bool((qbuf[:, 4 + 3 * C:] == -3.0).all()), \
        "qkv written outside its rows / columns"
    assert _same(ybuf[3:], d["y"]), "y must stay untouched"
