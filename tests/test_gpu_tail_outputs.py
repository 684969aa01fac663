"""GPU: the wide stages' Block tail writes what is read (csrc/blockrr.hip, cdseg_attn_tail_rr_ex, cdseg_block_io.flags / logits).

  * CDSEG_BLOCK_X_DEAD: the fp32 rows are read as the residual and left as they are; xc is BIT-equal to the unflagged call.
  * logits: the model's last tail forms the fp32 seg head on the row it holds in registers and stores neither x nor xc.
    Reference: the fp64 product of the fp32 x that the unflagged call stores with the fp32 head weights; bound per element
    (C + 2) 2^-24 (sum_c |W_kc x_c| + |b_k|) - C products and C additions of fp32 rounding 2^-24 each, first order, whatever
    the order of summation (the bound of the conformance tests).  cdseg_gemm's fp32 product is held to the same bound, so
    the bound is not vacuous.
  * every buffer lies in guard bands with non-contiguous rows (tests/guard_bands.py); the route record names the kernel and,
    in its aux word, what the launch left unwritten.
Both library builds."""
import copy

import numpy as np
import pytest
import torch

from cdsegnet_amd import _lib
from tests import guard_bands as GB
from tests.helpers import load_fixture
from tests.test_gpu_ops import LP, LPS, _library_variant, dev, ops  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SMALL = [1, 15, 16, 17, 31, 32, 33, 257]
# one n beyond a full grid of 32-row tiles (8 waves x 256 CUs x 3 / 2 workgroups per CU): the grid-stride loop runs twice
BIG = {32: 196608 + 33, 64: 131072 + 33}
EPS = 2.0 ** -24


def _case(C, n, seed):
    g = torch.Generator().manual_seed(seed)
    bf = LP()
    r = lambda *sh, s=1.0: torch.randn(*sh, generator=g) * s  # noqa: E731
    d = dict(o=r(n, C).to(bf), wp=r(C, C, s=C ** -0.5).to(bf), w1=r(4 * C, C, s=C ** -0.5).to(bf),
             w2=r(C, 4 * C, s=(4 * C) ** -0.5).to(bf), bp=r(C, s=0.3), g=1.0 + 0.1 * r(C), e=0.1 * r(C), b1=r(4 * C, s=0.3),
             b2=r(C, s=0.3), x0=r(n, C))
    return {k: v.cuda() for k, v in d.items()}


def _tail(ops, d, timg, *, flags=0, head=None, xc=True, logits_shape=None, ld_logits=None, num_classes=None):
    """One cdseg_attn_tail_rr_ex between guard bands: o and x inside NaN guards with padded rows, xc and the logits inside
    bands of a fill pattern.  -> dict(x, xc, logits, bands, route)."""
    n, C = d["x0"].shape
    bf = LP()
    o, oband = GB.poisoned_input(d["o"], name="o")
    x, xband = GB.poisoned_input(d["x0"], name="x")
    xcv, cband = GB.banded((n, C), bf, fill=-3.0, name="xc") if xc else (None, None)
    lg = lband = None
    kw = {}
    if head is not None:
        W, b, idx = head
        rows, k = logits_shape or (n, W.shape[0])
        lg, lband = GB.banded((rows, k), torch.float32, fill=-777.25, cols=8, name="logits")
        kw = dict(logits=lg, head_w=W, head_b=b, out_idx=idx, ld_logits=ld_logits, num_classes=num_classes)
    with ops.record_routes() as rr:
        ops.attn_tail_rr_ex(o, timg, d["bp"], d["g"], d["e"], d["b1"], d["b2"], x, xcv, flags=flags, **kw)
    torch.cuda.synchronize()
    for b_ in (oband, xband, cband, lband):
        if b_ is not None:
            b_.check()
    assert GB.same_bits(o, d["o"]), "the attention output is an input"
    return dict(x=x, xc=xcv, logits=lg, routes=rr.routes)


def _timg(ops, d, C):
    return ops.block_rr_pack(C, None, None, d["wp"], d["w1"], d["w2"])[1]


@LPS
@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("size", ["small", "second-pass"])
def test_x_dead_stores_xc_alone_bit_equal_and_leaves_x_as_read(ops, lp, C, size):
    for n in (SMALL if size == "small" else [BIG[C]]):
        d = _case(C, n, 1000 * C + n)
        timg = _timg(ops, d, C)
        ref = _tail(ops, d, timg)
        assert [(r.kernel, r.aux) for r in ref["routes"]] == [(f"tail_rr_kernel<{C}>", 0)]
        plain_x, plain_xc = d["x0"].clone(), torch.empty((n, C), dtype=LP(), device="cuda")
        ops.attn_tail_rr(d["o"], timg, d["bp"], d["g"], d["e"], d["b1"], d["b2"], plain_x, plain_xc)
        assert GB.same_bits(ref["x"], plain_x) and GB.same_bits(ref["xc"], plain_xc), "flags = 0 is cdseg_attn_tail_rr"
        assert not torch.equal(ref["x"], d["x0"]) and bool(torch.isfinite(ref["x"]).all())
        got = _tail(ops, d, timg, flags=ops.BLOCK_X_DEAD)
        assert GB.same_bits(got["xc"], ref["xc"]), f"n = {n}: xc differs from the unflagged call"
        assert GB.same_bits(got["x"], d["x0"]), f"n = {n}: x was written"
        assert [(r.kernel, r.aux & ops.TAIL_AUX_X_SKIPPED) for r in got["routes"]] == [(f"tail_rr_kernel<{C}>", 1)]
        assert not got["routes"][0].aux & ops.TAIL_AUX_LOGITS


def _bound(x, W, b):
    """fp64 reference logits and the per-element bound (C + 2) 2^-24 (sum_c |W_kc x_c| + |b_k|)."""
    x64, W64 = x.double().cpu(), W.double().cpu()
    b64 = torch.zeros(W.shape[0], dtype=torch.float64) if b is None else b.double().cpu()
    return x64 @ W64.t() + b64, (x.shape[1] + 2) * EPS * (x64.abs() @ W64.abs().t() + b64.abs())


@LPS
@pytest.mark.parametrize("classes", [4, 16, 20])
@pytest.mark.parametrize("size", ["small", "second-pass"])
def test_logits_from_the_tail_within_the_fp32_summation_bound(ops, lp, classes, size):
    C = 64
    worst = worst_gemm = 0.0
    for n in (SMALL if size == "small" else [BIG[C]]):
        d = _case(C, n, 77 * classes + n)
        timg = _timg(ops, d, C)
        g = torch.Generator().manual_seed(n + classes)
        W = (torch.randn(classes, C, generator=g) * C ** -0.5).cuda()
        b = (torch.randn(classes, generator=g) * 0.3).cuda()
        ref = _tail(ops, d, timg)  # the fp32 rows the unflagged call stores: bit-identical to what the kernel holds
        want, bound = _bound(ref["x"], W, b)
        for permuted in (False, True):
            idx = torch.randperm(n, generator=g).to(torch.int32).cuda() if permuted else None
            got = _tail(ops, d, timg, head=(W, b, idx), xc=permuted)  # (xc may be NULL)
            assert GB.same_bits(got["x"], d["x0"]), "x was written"
            if permuted:
                assert bool((got["xc"] == -3.0).all()), "xc was written"
            lg = got["logits"].double().cpu()
            w_, b_ = want, bound
            if permuted:
                w_, b_ = torch.empty_like(want), torch.empty_like(bound)
                w_[idx.cpu().long()], b_[idx.cpu().long()] = want, bound
            frac = ((lg - w_).abs() / b_).max().item()
            worst = max(worst, frac)
            assert frac <= 1.0, f"n = {n}, classes = {classes}, permuted = {permuted}: {frac:.3f} of the bound"
            assert [(r.kernel, bool(r.aux & ops.TAIL_AUX_LOGITS)) for r in got["routes"]] == [("tail_rr_kernel<64>", True)]
        out = torch.empty((n, classes), dtype=torch.float32, device="cuda")
        ops.gemm(ref["x"].contiguous(), W, out, bias=b)
        worst_gemm = max(worst_gemm, ((out.double().cpu() - want).abs() / bound).max().item())
        assert worst_gemm <= 1.0
    print(f"[measure] logits in the tail, classes = {classes}, {size}: worst used fraction of the bound {worst:.3f} "
          f"(cdseg_gemm fp32: {worst_gemm:.3f})")


@LPS
@pytest.mark.parametrize("C,classes,ld_shift", [(64, 13, 0), (64, 24, 0), (64, 200, 0), (64, 20, 2), (32, 16, 0)],
                         ids=["13", "24", "200", "unaligned-ld", "C32"])
def test_a_head_that_does_not_fit_is_refused_before_any_launch(ops, lp, C, classes, ld_shift):
    n = 257
    d = _case(C, n, classes)
    timg = _timg(ops, d, C)
    W = torch.randn(classes, C).cuda()
    x = d["x0"].clone()
    xc = torch.full((n, C), -3.0, dtype=LP(), device="cuda")
    buf = torch.full((n, classes + 8), -777.25, dtype=torch.float32, device="cuda")
    lg = buf[:, :classes] if ld_shift == 0 else buf.view(-1)[:n * (classes + ld_shift)].view(n, classes + ld_shift)[:, :classes]
    with ops.record_routes() as rr:
        with pytest.raises(_lib.CdsegError, match="CDSEG_ERR_UNSUPPORTED"):
            ops.attn_tail_rr_ex(d["o"], timg, d["bp"], d["g"], d["e"], d["b1"], d["b2"], x, xc, logits=lg, head_w=W,
                                head_b=None, out_idx=None)
    torch.cuda.synchronize()
    assert rr.count == 0, "a launch was recorded"
    assert GB.same_bits(x, d["x0"]) and bool((xc == -3.0).all()) and bool((buf == -777.25).all())


# ------------------------------------------------------------------ the Block executor
def _block_on_fixture(ops, C, seed):
    """cdseg_block_forward on the kernel map of a golden cloud's level 0 (the setup of tests/test_gpu_workspace_contract.py's
    _native_block on tests/golden/serialization_room1500.npz): run(**block_forward keywords) -> (x, xc_out)."""
    from oracle import model as OM
    from oracle import serialization as S
    rng = np.random.default_rng(seed)
    bf, H = LP(), C // 16
    fx = load_fixture("serialization_room1500.npz")
    grid = np.unique(np.asarray(fx["grid_coord"], dtype=np.int64)[np.asarray(fx["batch"]) == 0], axis=0)
    n = len(grid)
    nbr = OM.subm_neighbors(grid, np.zeros(n, dtype=np.int64), 3)
    pad, unpad, cu = S.padding_plan(np.array([n]), 1024)
    perm = rng.permutation(n)
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    order, inverse = perm[pad], unpad[inv]
    w16 = lambda *sh: dev(rng.standard_normal(sh).astype(np.float32) * sh[-1] ** -0.5, bf)  # noqa: E731
    vec = lambda k, one=False: dev((rng.standard_normal(k) * 0.1 + (1.0 if one else 0.0)).astype(np.float32))  # noqa: E731
    t = dict(cpe_conv_w=dev(rng.standard_normal((C, 27 * C)).astype(np.float32) * (13 * C) ** -0.5, bf), cpe_conv_b=vec(C),
             cpe_lin_w=w16(C, C), cpe_lin_b=vec(C), cpe_ln_g=vec(C, True), cpe_ln_b=vec(C), norm1_g=vec(C, True), norm1_b=vec(C),
             qkv_w=w16(3 * C, C), qkv_b=vec(3 * C), proj_w=w16(C, C), proj_b=vec(C), norm2_g=vec(C, True), norm2_b=vec(C),
             fc1_w=w16(4 * C, C), fc1_b=vec(4 * C), fc2_w=w16(C, 4 * C), fc2_b=vec(C))
    if ops.subm_conv3_ok(torch.empty((1, C), dtype=bf, device="meta")):
        t["cpe_conv_wimg"] = ops.subm_conv3_pack(t["cpe_conv_w"])
    himg, t["tail_img"] = ops.block_rr_pack(C, t["cpe_lin_w"], t["qkv_w"], t["proj_w"], t["fc1_w"], t["fc2_w"])
    if ops.block_rr_head_on(C):
        t["head_img"] = himg
    desc = ops.make_block_desc(bf, C, H, 4 * C, 16 ** -0.5, 1e-5, t)
    x_in = torch.as_tensor(rng.standard_normal((n, C)).astype(np.float32)).to(bf).float()
    wi = np.full(len(order), -1, dtype=np.int32)
    wi[inverse] = np.arange(n, dtype=np.int32)
    gidx, widx, nbrd, cud = dev(order.astype(np.int32)), dev(wi), dev(nbr.T.astype(np.int32)), dev(np.asarray(cu, dtype=np.int32))
    scratch = torch.empty(int(ops.block_scratch_bytes(desc, n)) + 4096, dtype=torch.uint8, device="cuda")

    def run(**kw):
        x, xc_in = dev(x_in), dev(x_in, bf)
        xc_out = torch.full((n, C), -3.0, dtype=bf, device="cuda")
        ops.bind_stream()
        try:
            with ops.record_routes() as rr:
                done = ops.block_forward(desc, n, x, xc_in, xc_out, None, nbrd, gidx, widx, cud, len(cu) - 1,
                                         int(np.diff(cu).max()), scratch, **kw)
        finally:
            ops.unbind_stream()
        torch.cuda.synchronize()
        return x, xc_out, done, rr.routes

    return n, dev(x_in), run


@LPS
@pytest.mark.parametrize("C", [32, 64])
def test_block_forward_flagged_against_unflagged(ops, lp, C):
    n, x_in, run = _block_on_fixture(ops, C, 5 + C)
    x0, xc0, done0, routes0 = run()
    x1, xc1, done1, routes1 = run(flags=ops.BLOCK_X_DEAD)
    assert done0 is True and done1 is True
    assert GB.same_bits(xc0, xc1) and bool(torch.isfinite(xc1.float()).all())
    assert routes0[-1].kernel == routes1[-1].kernel == f"tail_rr_kernel<{C}>"
    assert routes0[-1].aux == 0 and routes1[-1].aux == ops.TAIL_AUX_X_SKIPPED
    assert [r.kernel for r in routes0] == [r.kernel for r in routes1]
    assert not torch.equal(x0, x1), "the flagged tail stored x"  # (x1 holds the head's rows: nobody reads them)


@LPS
@pytest.mark.parametrize("classes", [16, 20])
def test_block_forward_with_the_logit_fields_against_block_forward_and_gemm(ops, lp, classes):
    C = 64
    n, x_in, run = _block_on_fixture(ops, C, 9 + classes)
    g = torch.Generator().manual_seed(classes)
    W = (torch.randn(classes, C, generator=g) * C ** -0.5).cuda()
    b = (torch.randn(classes, generator=g) * 0.3).cuda()
    idx = torch.randperm(n, generator=g).to(torch.int32).cuda()
    x0, xc0, _, _ = run()
    want = torch.full((n, classes), -777.25, dtype=torch.float32, device="cuda")
    ops.gemm(x0, W, want, bias=b, out_idx=idx)
    lg, band = GB.banded((n, classes), torch.float32, fill=-777.25, name="logits")
    x1, xc1, done, routes = run(logits=lg, head_w=W, head_b=b, out_idx=idx)
    band.check()
    assert done is True and routes[-1].kernel == "tail_rr_kernel<64>" and routes[-1].aux & ops.TAIL_AUX_LOGITS
    assert bool((xc1 == -3.0).all()), "xc_out was written"
    _, bound = _bound(x0, W, b)
    bnd = torch.empty_like(bound)
    bnd[idx.cpu().long()] = bound
    frac = ((lg.double().cpu() - want.double().cpu()).abs() / (2 * bnd)).max().item()
    print(f"[measure] block_forward logits against block_forward + gemm, classes = {classes}: {frac:.3f} of twice the bound")
    assert frac <= 1.0
    # a head that does not fit: refused before the Block's first launch, the caller's buffers as they were
    W13 = torch.randn(13, C).cuda()
    lg13 = torch.full((n, 16), -777.25, dtype=torch.float32, device="cuda")
    x2, xc2, done2, routes2 = run(logits=lg13[:, :13], head_w=W13, head_b=None, out_idx=None)
    assert done2 is False and routes2 == [] and GB.same_bits(x2, x_in) and bool((xc2 == -3.0).all())
    assert bool((lg13 == -777.25).all())


# ------------------------------------------------------------------ the engine
def _mini(classes):
    """The mini architecture with the shipped width of the last decoder stage (C = 64), random-init weights by name."""
    import cdsegnet_amd.models  # noqa: F401
    from cdsegnet_amd import configs
    from cdsegnet_amd.param_init import fill_state_dict
    from cdsegnet_amd.registry import build_model
    cfg = configs.mini_config(num_classes=classes)
    cfg["backbone"].update(n_dec_channels=(64, 32, 32, 64), n_dec_num_head=(4, 2, 2, 4))
    model = build_model(cfg)
    model.load_state_dict(fill_state_dict(model.state_dict(), seed=classes))
    return model.cuda().eval()


def _scene(classes):
    from cdsegnet_amd import synth
    sc = synth.collate([synth.room_scene(21, 3000, num_classes=classes)])
    return {k: torch.as_tensor(sc[k]).cuda() for k in ("coord", "grid_coord", "feat", "offset")}


def _spy_blocks(monkeypatch, ops):
    """What every block_forward of a forward was asked for: (xc_out is x, flags, logits given, returned)."""
    seen, real = [], ops.block_forward

    def spy(desc, n, x, xc_in, xc_out, *a, **k):
        r = real(desc, n, x, xc_in, xc_out, *a, **k)
        seen.append((xc_out.data_ptr() == x.data_ptr(), k.get("flags", 0), k.get("logits") is not None, r))
        return r

    monkeypatch.setattr(ops, "block_forward", spy)
    return seen


@pytest.mark.parametrize("precision,classes", [("fp16+head", 20), ("bf16+head", 16), ("bf16", 20)])
def test_engine_logits_from_the_tail_and_dead_x(monkeypatch, precision, classes):
    import cdsegnet_amd.ops as O
    from cdsegnet_amd import engine as E
    model, inp = _mini(classes), _scene(classes)
    model.precision = precision
    eng = model.engine()
    torch.manual_seed(3)
    draws = eng.predraw(inp)  # (the same shuffles and noise in every run)

    def forward(dead, gate):
        monkeypatch.setattr(E, "LOGITS_IN_TAIL_MIN_ROWS", gate)
        eng.dead_outputs = dead
        out = model.inference(dict(inp), eval=False, draws=copy.deepcopy(draws))["seg_logits"].clone()
        torch.cuda.synchronize()
        return out

    assert E.LOGITS_IN_TAIL_MIN_ROWS >= 65_536
    default_gate = E.LOGITS_IN_TAIL_MIN_ROWS
    all_live = forward(False, default_gate)
    seen = _spy_blocks(monkeypatch, O)
    pruned = forward(True, default_gate)
    assert torch.equal(all_live, pruned), "leaving dead rows unwritten changed the logits"
    n_dead = sum(1 for alias, flags, lg, _ in seen if flags & O.BLOCK_X_DEAD)
    # the last Block of n_enc0..3, c_enc0..1 and n_dec3..1 (this precision without "+head": of n_dec0 too)
    assert n_dead == (9 if precision.endswith("+head") else 10), seen
    assert not any(lg for _, _, lg, _ in seen), "3 000 rows are below the gate"
    assert seen[-1][0] == precision.endswith("+head"), "an fp32 head reads x: the last Block makes no 16-bit copy"
    if not precision.endswith("+head"):
        return
    del seen[:]
    fused = forward(True, 0)
    assert seen[-1][2] and seen[-1][3] is True, "the last Block was not asked for the logits"
    # twice the bound: both sides are fp32 sums of the same products in different orders.  The rows are not kept by the fused
    # forward, so the bound's magnitude term comes from the head's weights and the largest row of the unfused forward's input
    head = eng._eng("n_head")
    W, b = head.w["n_head.w"], head.w["n_head.b"]
    x_last = {}
    real_gemm = O.gemm

    def keep(A, Wt, out, **k):
        if Wt is W:
            x_last["x"] = A.clone()
            x_last["idx"] = k.get("out_idx")
        return real_gemm(A, Wt, out, **k)

    monkeypatch.setattr(O, "gemm", keep)
    again = forward(True, default_gate)
    assert torch.equal(again, pruned)
    _, bound = _bound(x_last["x"], W, b)
    bnd = torch.empty_like(bound)
    bnd[x_last["idx"].cpu().long()] = bound
    frac = ((fused.double().cpu() - pruned.double().cpu()).abs() / (2 * bnd)).max().item()
    print(f"[measure] engine, {precision}, {classes} classes: logits from the tail against the head's GEMM, "
          f"{frac:.3f} of twice the bound")
    assert frac <= 1.0


def test_engine_scannet200_keeps_the_gemm_and_makes_no_16_bit_copy(monkeypatch):
    import cdsegnet_amd.ops as O
    from cdsegnet_amd import engine as E
    model, inp = _mini(200), _scene(200)
    monkeypatch.setattr(E, "LOGITS_IN_TAIL_MIN_ROWS", 0)
    seen = _spy_blocks(monkeypatch, O)
    torch.manual_seed(3)
    out = model.inference(dict(inp), eval=False)["seg_logits"]  # (default precision: "fp16+head")
    torch.cuda.synchronize()
    assert out.shape[1] == 200 and bool(torch.isfinite(out).all())
    assert not any(lg for _, _, lg, _ in seen) and seen[-1][0], seen[-1]
