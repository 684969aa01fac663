"""GPU: the C = 512 Block head / tail on 64-row tiles (csrc/deep.hip, deep_head_kernel / deep_tail_kernel <512, 64, 2>).

From ops.DEEP512_ROWS64_MIN rows upward a workgroup of 8 waves owns a 64-row tile and every wave 64 output channels (two of
the per-wave weight streams of the image), so a weight byte is fetched once per 64 rows; below, 16 waves own a 32-row tile.
Every output element is the same chain of products in the same order, and the LayerNorm statistics are the same sixteen
32-channel partials added by the same tree, so the two forms must agree BIT for BIT.  Rows are independent: the reference
is the same rows run in chunks below the threshold (32-row form).  No tolerance.

Cases: n at the threshold and at the 24-scene stage size (neither a multiple of 64: a ragged last tile), with and without
the timestep bias, in place (x_out == x) and with the residual read from one buffer and written to another (x_out != x; a
workspace is passed to the tail, which must not split at this height).  The head's third input form - y as raw split-K
partial planes - has no binding of its own: it runs inside the native Block executor, i.e. in
test_twenty_four_scenes_collated_vs_oracle (18.6 k rows on the C = 512 stage).
"""
import pytest
import torch

from tests.test_gpu_ops import LP, LPS, _deep_case, _library_variant, dev, ops, report  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

C = 512
CHUNK = 4000  # rows per reference launch: below the threshold, not a multiple of 32 (chunks end in ragged 32-row tiles too)


def _i16(t):
    return t.view(torch.int16)


@LPS
@pytest.mark.parametrize("two_buffers", [False, True], ids=["in-place", "x_out"])
@pytest.mark.parametrize("tb", [True, False], ids=["tbias", "no-tbias"])
@pytest.mark.parametrize("M", ["threshold", 778 * 24, 778 * 32 + 37], ids=["threshold", "24-scenes", "32-scenes+37"])
def test_deep512_rows64_equals_the_32_row_form_bit_for_bit(ops, lp, M, tb, two_buffers):
    M = ops.DEEP512_ROWS64_MIN if M == "threshold" else M
    assert M >= ops.DEEP512_ROWS64_MIN and M % 64 and CHUNK < ops.DEEP512_ROWS64_MIN
    d, bf = _deep_case(M, C, M * 13 + C + tb, tb)
    D = lambda k, dt=None: None if d[k] is None else dev(d[k], dt)  # noqa: E731
    himg, timg = ops.block_rr_pack(C, D("wl", bf), D("wq", bf), D("wp", bf), D("w1", bf), D("w2", bf))
    y, o, x0, cb = D("y", bf), D("o", bf), D("x0"), D("cb")
    bl, lnp, ln1, bq = D("bl"), (D("g1"), D("e1")), (D("g2"), D("e2")), D("bq")
    bp, g3, e3, b1, b2 = D("bp"), D("g3"), D("e3"), D("b1"), D("b2")
    nan = lambda *s, dt=torch.float32: torch.full(s, float("nan"), dtype=dt, device="cuda")  # noqa: E731

    def head(rows, x_in, x_out, qkv):
        a, b = rows
        if two_buffers:
            ops.cpe_head_rr2(y[a:b], himg, bl, lnp, x_in[a:b], x_out[a:b], cb, ln1, bq, qkv[a:b], qkv_flags=ops.ATTN_V_BF16)
        else:
            x_out[a:b] = x_in[a:b]
            ops.cpe_head_rr(y[a:b], himg, bl, lnp, x_out[a:b], cb, ln1, bq, qkv[a:b], qkv_flags=ops.ATTN_V_BF16)

    def tail(rows, x_in, x_out, xc, ws):
        a, b = rows
        if two_buffers:
            ops.attn_tail_rr2(o[a:b], timg, bp, g3, e3, b1, b2, x_in[a:b], x_out[a:b], xc[a:b], ws=ws)
        else:
            x_out[a:b] = x_in[a:b]
            ops.attn_tail_rr(o[a:b], timg, bp, g3, e3, b1, b2, x_out[a:b], xc[a:b])

    chunks = [(a, min(a + CHUNK, M)) for a in range(0, M, CHUNK)]
    # ---- head: x, qkv
    x_new, qkv_new = nan(M, C), nan(M, 3 * C, dt=bf)
    with ops.record_routes() as rr:
        head((0, M), x0, x_new, qkv_new)
    # the launch record: 64-row tiles (8 waves, NS = 2) from DEEP512_ROWS64_MIN rows, one workgroup per tile
    assert [(r.kernel, r.bm, r.aux) for r in rr.routes] == [("deep_head_kernel<512,64,2>", 64, 1)], rr.routes
    x_ref, qkv_ref = nan(M, C), nan(M, 3 * C, dt=bf)
    with ops.record_routes() as rr:
        for r in chunks:
            head(r, x0, x_ref, qkv_ref)
    assert rr.count == len(chunks) and set(rr.kernels()) == {"deep_head_kernel<512,32,1>"}, rr.routes
    torch.cuda.synchronize()
    assert torch.equal(x0, D("x0")), "the rows read must stay untouched"
    assert bool(torch.isfinite(x_new).all()) and bool(torch.isfinite(qkv_new[:, :2 * C].float()).all())
    same_hx, same_q = torch.equal(x_new, x_ref), torch.equal(_i16(qkv_new), _i16(qkv_ref))
    # ---- tail: x, xc (the reference chunks get no workspace: the unsplit 32-row form)
    ws = torch.empty(4 * M * C * 4 + 64, dtype=torch.uint8, device="cuda") if two_buffers else None
    xt_new, xc_new = nan(M, C), nan(M, C, dt=bf)
    with ops.record_routes() as rr:
        tail((0, M), x0, xt_new, xc_new, ws)
    assert [(r.kernel, r.bm, r.aux) for r in rr.routes] == [("deep_tail_kernel<512,64,2>", 64, 1)], rr.routes  # no split, workspace or not
    xt_ref, xc_ref = nan(M, C), nan(M, C, dt=bf)
    with ops.record_routes() as rr:
        for r in chunks:
            tail(r, x0, xt_ref, xc_ref, None)
    assert rr.count == len(chunks) and {(r.kernel, r.aux) for r in rr.routes} == {("deep_tail_kernel<512,32,1>", 1)}, rr.routes
    torch.cuda.synchronize()
    assert bool(torch.isfinite(xt_new).all())
    same_tx, same_xc = torch.equal(xt_new, xt_ref), torch.equal(_i16(xc_new), _i16(xc_ref))
    report(f"deep512 rows64 M={M} tb={int(tb)} two_buffers={int(two_buffers)} {lp}", head_x=int(same_hx), qkv=int(same_q),
           tail_x=int(same_tx), xc=int(same_xc), head_x_maxdiff=float((x_new - x_ref).abs().max()),
           tail_x_maxdiff=float((xt_new - xt_ref).abs().max()))
    assert same_hx and same_q
    assert same_tx and same_xc
