"""GPU: every host-side kernel chooser OUTSIDE cdseg_gemm and the Block forward, addressed by ROUTE (include/cdseg.h
cdseg_route_*, csrc/route.h): the row kernels (layernorm, add_layernorm and the glue of csrc/trainblock.hip), the weight
gradients and the attention backward of csrc/train.hip, the level kernels of csrc/pool.hip, the loss, skip and fusion kernels.

These launchers pick a template instantiation by width, dtype, alignment or a mode switch.  A numerical test guards the
kernel it happens to run; a case here does three things: it runs between guard bands (tests/guard_bands.py; NaN guards
around gathered operands), compares with an independent reference, and asserts the launch record - kernel name, splits, aux -
against the route written next to the case, which was read off the chooser's rule by hand.
test_every_catalogued_variant_outside_the_gemm_is_reached_or_accounted_for replays the launches on zero operands and fails
when a catalogued kernel is left without a case.  (tests/test_gpu_level_fused.py asserts the pooling folds and both unpool
shapes over its whole pattern list; the cases here are its smallest ones.)

Shapes are the smallest at which a kernel can still go wrong, no workload sizes.

Bounds, none of them fitted to the kernels' output:
  integers         operands in [-3, 3]: every product and partial sum is an exactly representable integer, so the result
                   must EQUAL the integer result whatever the order of the adds (tests/test_gpu_wgrad16.py).
  LayerNorm        |kernel - fp64| <= 3 E_ref + 2^-24 max |ref|, E_ref = the error of torch's own fp32 F.layer_norm (+ res +
                   colbias) on the same device and values (the form of test_add_layernorm_vs_fp64_within_three_times_torch;
                   the factor covers another summation order of the same fp32 products).  E_ref, max |ref| and the kernel's
                   error are each the maximum over ALL row counts of a case: a single row of four channels is no sample of
                   torch's error (it can be exactly 0, which would turn the bound into half an ulp).
  16-bit output    that + one rounding to nearest of the reference: |ref| 2^-8 (bfloat16) or |ref| 2^-11 (half), per element.
  constant row     every element 0.5: each partial sum and the mean are exact in fp32 in any order, the variance is exactly
                   0 and only eps keeps 1 / sigma finite - the row must equal beta (+ res + colbias) to the same bound.
  the others       each family's own yardstick, imported from the test file that owns the family.
Every err / bound is printed with the [measure] convention before it is asserted."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cdsegnet_amd import _lib
from cdsegnet_amd import ops as O
from tests import guard_bands as GB
from tests import skip_restatement as SR
from tests import test_gpu_attention_bwd16 as B16
from tests import test_gpu_dropout as DR
from tests import test_gpu_fusion as FU
from tests import test_gpu_level_fused as LF
from tests import test_gpu_seg_loss as SL
from tests import test_gpu_skip as SK
from tests import test_gpu_train_block as TB
from tests import test_gpu_train_fp32 as TF
from tests.test_gpu_ops import LP, _library_variant, report  # noqa: F401  (fixture: lp="f16" -> the half build)
from tests.test_gpu_wgrad16 import _eq, _exact, _ints, _kernel_map

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EPS = 1e-5
EPS16 = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
BOTH = ("bf16", "f16")


def _sync():
    torch.cuda.synchronize()


def _z(t, zero):
    """The census replays a case's launches on zero operands."""
    return torch.zeros_like(t) if zero else t


def _routes(rr, want):
    """The recorded kernels of a case, asserted against the route written next to it."""
    assert rr.count == len(want) and rr.kernels() == list(want), (want, rr.routes)
    return rr.routes


# ============================================================================================ layernorm / add_layernorm
# C -> (MAXV, lanes per row) by cdseg_layernorm's rule: chunks = C / 4, tpr = the power of two >= chunks up to 64, MAXV = the
# instantiation that holds ceil(chunks / tpr) chunks per lane.  4: one lane a row; 20: five chunks on eight lanes (idle lanes);
# 256 / 512 / 1024 / 2048: full passes of MAXV 1 / 2 / 4 / 8; 260 / 520 / 1028 / 2044: a ragged last pass of 2 / 4 (3 used) /
# 8 (5 used) / 8
LN_ROUTE = {4: (1, 1), 20: (1, 8), 256: (1, 64), 260: (2, 64), 512: (2, 64), 520: (4, 64), 1024: (4, 64), 1028: (8, 64),
            2044: (8, 64), 2048: (8, 64)}
LN_FORMS = ("f32", "in16", "out2", "res", "inplace")  # in16 / out2: x / the second output in the build's 16-bit type;
#                                                        res: + res + colbias with out aliasing res, as cdseg_block_forward calls it


def _ln_rows(tpr):
    """With r = 64 / tpr rows per wave: 1, r - 1 (where >= 1), r + 1, 4 r + 1 (more than one wave, a partial last one)."""
    r = 64 // tpr
    return sorted({1, r + 1, 4 * r + 1} | ({r - 1} if r > 1 else set()))


def _ln_finish(name, runs, lp):
    """runs: per row count (fp32 output or None, ref, torch's fp32 result, 16-bit output or None, constant row or None, its
    target or None), all fp64 on the host."""
    e_ref = max(float((t32 - ref).abs().max()) for _, ref, t32, _, _, _ in runs)
    top = max(float(ref.abs().max()) for _, ref, _, _, _, _ in runs)
    bound = 3 * e_ref + U * top
    if any(got is not None for got, *_ in runs):
        err = max(float((got - ref).abs().max()) for got, ref, _, _, _, _ in runs)
        report(name, kernel_err=err, E_ref=e_ref, bound=bound, err_over_bound=err / bound)
        assert all(bool(torch.isfinite(got).all()) for got, *_ in runs), name
        assert err <= bound, (name, err, e_ref, top)
    for got, ref, _, got16, const, target in runs:
        if got16 is not None:
            worst = float(((got16 - ref).abs() / (bound + ref.abs() * EPS16[lp])).max())
            report(name + f" 16-bit output, {ref.shape[0]} rows", E_ref=e_ref, bound=bound, err_over_bound=worst)
            assert bool(torch.isfinite(got16).all()) and worst <= 1.0, (name, worst)
        if const is not None and got is not None:
            d = float((got[const] - target).abs().max())
            report(name + " constant row", err=d, bound=bound, err_over_bound=d / bound)
            assert bool(torch.isfinite(got[const]).all()) and d <= bound, (name, d, bound)
        if const is not None and got16 is not None:
            d = float(((got16[const] - target).abs() / (bound + target.abs() * EPS16[lp])).max())
            report(name + " constant row, 16-bit output", err_over_bound=d)
            assert bool(torch.isfinite(got16[const]).all()) and d <= 1.0, (name, d)


def _layernorm_case(c, form, lp, zero=False):
    mv, tpr = LN_ROUTE[c]
    lpt = LP()
    rows = _ln_rows(tpr)
    g = torch.Generator().manual_seed(100 * c + LN_FORMS.index(form))
    gamma, beta, colb = 1 + 0.3 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
    gd, bd, cd = gamma.cuda(), beta.cuda(), colb.cuda()
    runs, recorded = [], []
    for m in rows:
        x = _z(0.5 + torch.randn(m, c, generator=g), zero)
        const = m // 2 if m == rows[-1] and not zero else None
        if const is not None:
            x[const] = 0.5
        if form == "in16":
            x = x.to(lpt).float()
        res = torch.randn(m, c, generator=g) if form == "res" else None
        xsrc = x.cuda().to(lpt) if form == "in16" else x.cuda()
        ref = F.layer_norm(x.double(), (c,), gamma.double(), beta.double(), EPS)
        t32 = F.layer_norm(xsrc.float(), (c,), gd, bd, EPS)
        target = beta.double()
        if res is not None:
            ref, t32, target = ref + res.double() + colb.double(), t32 + res.cuda() + cd, target + res[m // 2].double() + colb.double()
        bands = []
        if form == "inplace":
            xin, b = GB.banded((m, c), torch.float32, fill=-77.0, name="x = out")
            xin.copy_(xsrc)
            out = xin
        else:
            xin, b = GB.poisoned_input(xsrc, name="x")
            bands.append(b)
            out, b = GB.banded((m, c), torch.float32, fill=-77.0, name="out")
        bands.append(b)
        resd = None
        if res is not None:
            out.copy_(res.cuda())
            resd = out
        out2 = None
        if form == "out2":
            out2, b = GB.banded((m, c), lpt, fill=-77.0, name="out2")
            bands.append(b)
        with O.record_routes() as rr:
            O.layernorm(xin, gd, bd, out, eps=EPS, res=resd, colbias=cd if res is not None else None, out2=out2)
        _sync()
        for b in bands:
            b.check()
        r, = _routes(rr, [f"layernorm_kernel<{mv}>"])
        assert (r.aux, r.bm, r.bn, r.splits, r.compute) == (tpr, 64 // tpr, c, 1, O.BF16 if form == "in16" else O.F32), r
        recorded.append(r.kernel)
        runs.append((out.double().cpu(), ref, t32.double().cpu(), out2.double().cpu() if out2 is not None else None, const,
                     target if const is not None else None))
    if not zero:
        _ln_finish(f"layernorm C={c} {form} ({lp}) rows={rows}", runs, lpt)
    return recorded


LN_PARAMS = [(c, f, lp) for c in LN_ROUTE for f in LN_FORMS for lp in (BOTH if f in ("in16", "out2") else BOTH[:1])]


@pytest.mark.parametrize("c,form,lp", LN_PARAMS, ids=[f"{c}-{f}-{lp}" for c, f, lp in LN_PARAMS])
def test_layernorm_route_vs_fp64(c, form, lp):
    _layernorm_case(c, form, lp)


def _add_layernorm_case(c, out, masked, lp, zero=False):
    """cdseg_add_layernorm through the C ABI (x1 and h between guard bands, x and a between NaN rows, the mask inside a NaN
    buffer): x1 = x + m a bit-equal to torch, h = LN(x1) against fp64."""
    mv, tpr = LN_ROUTE[c]
    lpt = LP()
    lib = _lib.load()
    hdt, code = (torch.float32, O.F32) if out == "fp32" else (lpt, O.BF16)
    rows = _ln_rows(tpr)
    g = torch.Generator().manual_seed(100 * c + 7 * masked + (out != "fp32"))
    gamma, beta = (1 + 0.3 * torch.randn(c, generator=g)).cuda(), (0.1 * torch.randn(c, generator=g)).cuda()
    runs, recorded = [], []
    for m in rows:
        x, a = _z(0.5 + torch.randn(m, c, generator=g), zero), _z(torch.randn(m, c, generator=g), zero)
        const = m // 2 if m == rows[-1] and not zero else None
        if const is not None:
            x[const], a[const] = 0.25, 0.25  # (x1 = 0.25 + mask * 0.25 is constant along the row and exact)
        mask = None
        if masked:
            mbuf = torch.full((m + 128,), float("nan"), device="cuda")
            mask = mbuf[64:64 + m]
            mask.copy_(TB._mask(m, g, zero_rows=m > 1))
            if const is not None:
                mask[const] = 1.0
        xd, xb = GB.poisoned_input(x.cuda(), cols=0, name="x")
        ad, ab = GB.poisoned_input(a.cuda(), cols=0, name="a")
        x1, x1b = GB.banded((m, c), torch.float32, cols=0, fill=-77.0, name="x1")
        h, hb = GB.banded((m, c), hdt, cols=0, fill=-77.0, name="h")
        assert all(t.is_contiguous() for t in (xd, ad, x1, h))
        with O.record_routes() as rr:
            O.check(lib.cdseg_add_layernorm(O._ptr(xd), O._ptr(ad), O._ptr(mask), O._ptr(gamma), O._ptr(beta), EPS, O._ptr(x1),
                                            O._ptr(h), code, m, c, O._stream()), "add_layernorm")
        _sync()
        for b in (xb, ab, x1b, hb):
            b.check()
        r, = _routes(rr, [f"add_layernorm_kernel<{mv},{'f32' if out == 'fp32' else 'b16'}>"])
        assert (r.aux, r.bm, r.bn, r.splits, r.compute) == (tpr, 64 // tpr, c, 1, code), r
        recorded.append(r.kernel)
        want = xd + (ad if mask is None else ad * mask[:, None])
        assert TB._bits(x1.contiguous(), want), "x1 = x + m a, the multiply and the add rounded separately"
        ref = F.layer_norm(want.double(), (c,), gamma.double(), beta.double(), EPS).cpu()
        t32 = F.layer_norm(want, (c,), gamma, beta, EPS).double().cpu()
        got = h.double().cpu()
        f32 = hdt == torch.float32
        runs.append((got if f32 else None, ref, t32, None if f32 else got, const, beta.double().cpu() if const is not None else None))
    if not zero:
        _ln_finish(f"add_layernorm C={c} h={out} mask={masked} ({lp}) rows={rows}", runs, lpt)
    return recorded


ALN_PARAMS = [(c, o, mk, lp) for c in LN_ROUTE for o, lp in (("fp32", "bf16"), ("lp", "bf16"), ("lp", "f16")) for mk in (False, True)]


@pytest.mark.parametrize("c,out,masked,lp", ALN_PARAMS, ids=[f"{c}-{o}-{'mask' if mk else 'nomask'}-{lp}" for c, o, mk, lp in ALN_PARAMS])
def test_add_layernorm_route_vs_fp64(c, out, masked, lp):
    _add_layernorm_case(c, out, masked, lp)


# ============================================================================================ 16-bit weight gradient
# (N, K) -> (tn, tk) of cdseg_wgrad::partition_16: the narrowest of 32 / 64 / 128 columns that covers N (K); 128 x 128 -> 128 x 64
W16 = [(16, 16, 1, 1), (32, 48, 1, 2), (32, 64, 1, 2), (16, 80, 1, 4), (32, 512, 1, 4), (48, 32, 2, 1), (64, 64, 2, 2),
       (48, 128, 2, 4), (96, 32, 4, 1), (128, 128, 4, 2)]
W16_M = (1, 63, 65, 513, 1025)
W16_SPLITS = {1: 1, 63: 1, 65: 1, 513: 2, 1025: 3}  # at most ceil(M / 512) row splits (every shape here has few tiles)
W16_FORMS = ("linear", "gathered", "conv")
W16_CONV = [(16, 16), (32, 64), (64, 64), (128, 128)]  # <1,1>, <1,2>, <2,2>, <4,2>: the model's conv tiles and the new <1,2>


def _wgrad16_case(N, K, tn, tk, form, lp, zero=False, rows=W16_M):
    lpt = LP()
    conv = form == "conv"
    kvol = 27 if conv else 1
    full = _kernel_map(O, "batch2", 3) if conv else None
    recorded = []
    for M in rows:
        rng = np.random.default_rng(M + 7 * K + 13 * N + W16_FORMS.index(form))
        R = M // 2 + 3 if form == "gathered" else M
        x, dy = _z(_ints(rng, R, K), zero), _z(_ints(rng, M, N), zero)
        part = O.wgrad_partition(M, N, K, kvol, lpt)
        assert part.splits == W16_SPLITS[M], (M, tuple(part))
        idx = want3 = None
        if form == "gathered":
            idx = rng.integers(0, R, size=M)
            idx[rng.random(M) < 0.3] = -1
            if M > 64:
                idx[64:64 + min(M - 64, 70)] = -1  # a dead 64-row chunk from a chunk boundary on (the skip path)
            idx = torch.as_tensor(idx, dtype=torch.int32)
        if conv:
            assert full.shape[0] == 27 and full.shape[1] >= M
            nb = full[:, :M].clone()
            nb[nb >= M] = -1  # the first M voxels of the fixture cloud: neighbours behind them count as absent
            nb = nb.contiguous()
            assert M == 1 or int((nb >= 0).sum()) > M  # (more than the centre offset is alive)
            want3 = torch.stack([_exact(dy, x, nb[o].cpu())[0] for o in range(27)], 1)
            want_b = dy.double().sum(0).round().long()
        else:
            want_w, want_b = _exact(dy, x, idx)
        for det in (False, True):
            xd, xb = GB.poisoned_input(x.cuda().to(lpt), name="x")
            dyd, dyb = GB.poisoned_input(dy.cuda().to(lpt), name="dy")
            dw, wb = GB.banded((N, kvol * K), torch.float32, cols=0 if conv else 8, fill=-77.0, name="dw")
            dbuf, bb = GB.banded((1, N), torch.float32, cols=0, fill=-77.0, name="db")
            dw.zero_(), dbuf.zero_()
            db = dbuf[0]
            checks = []
            with O.record_routes() as rr:
                if conv:
                    nbd, chk = GB.guard_index(nb, none=-1)
                    O.conv_wgrad(xd, nbd, dyd, dw.view(N, 27, K), db, **O.det_kw(det))
                else:
                    idxd = None
                    if idx is not None:
                        idxd, chk = GB.guard_index(idx.cuda(), none=-1)
                        checks.append(chk)
                    O.linear_wgrad(xd, dyd, dw, db, xidx=idxd, **O.det_kw(det))
            _sync()
            for b in (xb, dyb, wb, bb):
                b.check()
            for chk in checks:
                chk()
            r, = _routes(rr, [f"wgrad16{'_det' if det else ''}_kernel<{tn},{tk}>"])
            assert (r.bm, r.bn, r.aux, r.compute) == (32 * tn, 32 * tk, kvol, O.BF16), r
            assert (r.splits, r.xmode) == (part.splits, part.rows_per_split), (r, tuple(part))
            recorded.append(r.kernel)
            if zero:
                continue
            what = f"wgrad16 {form} M={M} N={N} K={K} det={det} ({lp})"
            assert not bool(torch.isnan(dw).any()), what + ": a NaN reached dw - an operand was read outside its rows"
            if conv:
                assert _eq(dw.view(N, 27, K), want3), what
            else:
                assert _eq(dw, want_w), what
            assert _eq(db, want_b), what + " db"
    return recorded


W16_PARAMS = [(n, k, tn, tk, f, lp) for n, k, tn, tk in W16 for f in W16_FORMS[:2] for lp in BOTH] + \
             [(n, k, tn, tk, "conv", lp) for n, k, tn, tk in W16 if (n, k) in W16_CONV for lp in BOTH]


@pytest.mark.parametrize("N,K,tn,tk,form,lp", W16_PARAMS, ids=[f"{n}x{k}-{f}-{lp}" for n, k, _, _, f, lp in W16_PARAMS])
def test_wgrad16_route_exact_on_integers(N, K, tn, tk, form, lp):
    got = _wgrad16_case(N, K, tn, tk, form, lp)
    assert len(got) == 2 * len(W16_M)
    report(f"wgrad16 {N}x{K} {form} ({lp})", launches=len(got), exact=1)


# ============================================================================================ attention backward and dropout
# (patches, heads) -> the slices of a patch-head.  The 16-bit forms (attn_bwd16 and attn_drop16 alike) double the split
# while patches * heads * split * 2 <= 512: 4 up to 128 patch-heads, 2 up to 256, 1 above.  The fp32 dropout forward does the
# same against 256: 4 up to 64 patch-heads, 2 up to 128, 1 above.  The fp32 backward cuts nothing.  Both sides of every edge:
#             patches heads split16 split of attn_drop_f32
ATTN_SPLIT = [(32, 2, 4, 4), (13, 5, 4, 2), (64, 2, 4, 2), (43, 3, 2, 1), (128, 2, 2, 1), (257, 1, 1, 1)]
ATTN_LENS = (1, 17, 33, 64, 5, 70)  # one slot, ragged tiles, a full 64-key tile, more than one tile
RATE = 0.5


def _attn_inputs(P, H, lpt):
    lens = [ATTN_LENS[i % len(ATTN_LENS)] for i in range(P)]
    rng = np.random.default_rng(1000 * P + H)
    return B16._case(lens, H, 0, False, lpt, rng, 1.0)


def _attn16_case(P, H, s16, lp, zero=False):
    lpt = LP()
    launch, (q, k, v, do) = _attn_inputs(P, H, lpt)
    if zero:
        q, k, v, do = (np.zeros_like(a) for a in (q, k, v, do))
    assert (s16 == 1 or P * H * s16 <= 512) and (s16 == 4 or P * H * 2 * s16 > 512)  # on which side of the rule the case sits
    b16 = O.BF16
    with O.record_routes() as rr:
        plain = B16._kernel(lpt, q, k, v, do, launch, H)
    rec = _routes(rr, ["attn_bwd16_q_kernel<>", "attn_bwd16_kv_kernel<>"])
    assert all((r.splits, r.compute) == (s16, b16) for r in rec), rec
    with O.record_routes() as rr:
        drop = DR._run(lpt, q, k, v, do, launch, H, RATE)
    rec2 = _routes(rr, ["attn_drop16_kernel", "attn_bwd16_q_kernel<DropP>", "attn_bwd16_kv_kernel<DropP>"])
    assert all((r.splits, r.compute) == (s16, b16) for r in rec2), rec2
    if not zero:
        B16._compare(f"{P} patches x {H} heads, split {s16} ({lp})", plain, launch, q, k, v, do, H, lpt)
        masks = DR._masks(RATE, DR._lens(launch), H)
        exact = DR._oracle(q, k, v, do, launch, H, lpt, masks, RATE)
        emul = DR._oracle(q, k, v, do, launch, H, lpt, masks, RATE, "emul")
        for tn, g, g64, ge in zip(DR.NAMES, drop, exact, emul):
            assert np.isfinite(g).all() and np.abs(g64).max() > 0, tn
            err, eref = B16._metric(g, g64), B16._metric(ge, g64)
            bound = 2 * eref + launch.max_len * U
            report(f"attn drop16 {P}x{H} split {s16} {tn} ({lp})", kernel_err=err, E_ref=eref, bound=bound, err_over_bound=err / bound)
            assert err <= bound, (tn, err, eref, bound)
    return [r.kernel for r in rec + rec2]


def _attn32_case(P, H, s32, zero=False):
    launch, (q, k, v, do) = _attn_inputs(P, H, torch.bfloat16)  # (dyadic inputs: exact in fp32)
    if zero:
        q, k, v, do = (np.zeros_like(a) for a in (q, k, v, do))
    with O.record_routes() as rr:
        drop = DR._run(torch.float32, q, k, v, do, launch, H, RATE)
    rec = _routes(rr, ["attn_drop_f32_kernel", "attn_bwd_q_mfma_kernel<DropP>", "attn_bwd_kv_mfma_kernel<DropP>"])
    assert [r.splits for r in rec] == [s32, 1, 1] and all(r.compute == O.F32 for r in rec), rec
    with O.record_routes() as rr:
        plain = DR._run(torch.float32, q, k, v, do, launch, H, None)
    rec2 = _routes(rr, ["attn_f32_kernel", "attn_bwd_q_mfma_kernel<>", "attn_bwd_kv_mfma_kernel<>"])
    assert all(r.splits == 1 for r in rec2[1:]), rec2
    if not zero:
        masks = DR._masks(RATE, DR._lens(launch), H)
        exact = DR._oracle(q, k, v, do, launch, H, None, masks, RATE)
        exact_plain = DR._oracle(q, k, v, do, launch, H, None, None, RATE)
        for tn, g, g64, gp, gp64 in zip(DR.NAMES, drop, exact, plain, exact_plain):
            assert np.isfinite(g).all() and np.abs(g64).max() > 0, tn
            err, base = B16._metric(g, g64), B16._metric(gp, gp64)
            bound = 2 * base + launch.max_len * U
            report(f"attn drop fp32 {P}x{H} split {s32} {tn}", kernel_err=err, plain_kernel_err=base, bound=bound, err_over_bound=err / bound)
            assert err <= bound, (tn, err, base, bound)
    return [r.kernel for r in rec + rec2[1:]]


@pytest.mark.parametrize("lp", BOTH)
@pytest.mark.parametrize("P,H,s16,s32", ATTN_SPLIT, ids=[f"{p}x{h}" for p, h, _, _ in ATTN_SPLIT])
def test_attention_16_bit_split_route_vs_fp64(P, H, s16, s32, lp):
    _attn16_case(P, H, s16, lp)


@pytest.mark.parametrize("P,H,s16,s32", ATTN_SPLIT, ids=[f"{p}x{h}" for p, h, _, _ in ATTN_SPLIT])
def test_attention_fp32_dropout_split_route_vs_fp64(P, H, s16, s32):
    _attn32_case(P, H, s32)


# ============================================================================================ the other families
# One minimal case per instantiation, each with the reference and the yardstick of the test file that owns the family.
ROWS, WIDTH = 65, 20  # the glue kernels: more than one 64-row group, five 16-byte chunks a row


def _runs(n_vox, g):
    runs = torch.randint(1, 4, (n_vox,), generator=g)
    start = torch.cat([torch.zeros(1, dtype=torch.int64), runs.cumsum(0)]).int()
    return runs, start


def _gather_first_case(out, lp, zero=False):
    lpt, variant = LP(), None if out == "f32" else lp
    g = torch.Generator().manual_seed(3)
    runs, start = _runs(ROWS, g)
    x = _z(torch.randn(int(start[-1]), WIDTH, generator=g), zero)
    xd, xb = GB.poisoned_input(x.cuda(), cols=0, name="x")
    sd, chk = GB.guard_index(start.cuda())
    with O.record_routes() as rr:
        got = O.gather_first(xd, sd, variant)
    _sync()
    xb.check(), chk()
    rec = _routes(rr, [f"gather_first_kernel<{'f32' if out == 'f32' else 'b16'}>"])
    want = x[start[:-1].long()]
    assert TB._bits(got.cpu(), want if out == "f32" else want.to(lpt))
    return [r.kernel for r in rec]


def _scatter_first_case(mode, zero=False):
    g = torch.Generator().manual_seed(4)
    runs, start = _runs(ROWS, g)
    n = int(start[-1])
    row_vox = torch.repeat_interleave(torch.arange(ROWS), runs).int()
    grad = _z(torch.randn(ROWS, WIDTH, generator=g), zero)
    pre = torch.randn(n, WIDTH, generator=g)
    gd, gb = GB.poisoned_input(grad.cuda(), cols=0, name="g")
    dx, db = GB.banded((n, WIDTH), torch.float32, cols=0, fill=-77.0, name="dx")
    lib = _lib.load()
    if mode == "acc":
        dx.copy_(pre)
    voxd, vox_chk = GB.guard_index(row_vox.cuda())
    startd, start_chk = GB.guard_index(start.cuda())
    with O.record_routes() as rr:
        O.check(lib.cdseg_scatter_first(O._ptr(gd), O._ptr(voxd), O._ptr(startd), O._ptr(dx), int(mode == "acc"), n, WIDTH,
                                        O._stream()), "scatter_first")
    _sync()
    gb.check(), db.check(), vox_chk(), start_chk()
    rec = _routes(rr, [f"scatter_first_kernel<{mode}>"])
    want = pre.clone() if mode == "acc" else torch.zeros(n, WIDTH)
    want[start[:-1].long()] += grad
    got = dx.cpu().contiguous()
    bad = (GB.bits(got) != GB.bits(want)).any(1).nonzero().flatten().tolist()
    assert not bad, (f"{len(bad)} rows differ, the first {bad[:5]} (first rows of a run: {sorted(set(bad) & set(start[:-1].tolist()))[:5]}), "
                     f"max |diff| {float((got - want).abs().max())}")
    return [r.kernel for r in rec]


def _scale_cast_case(out, lp, zero=False):
    lpt, variant = LP(), None if out == "f32" else lp
    g = torch.Generator().manual_seed(5)
    dy = _z(torch.randn(ROWS, WIDTH, generator=g) * 300.0, zero).cuda()
    m = TB._mask(ROWS, g).cuda()
    with O.record_routes() as rr:
        got = O.scale_cast(dy, m, variant)
    rec = _routes(rr, [f"scale_cast_kernel<{'f32' if out == 'f32' else 'b16'}>"])
    want = dy * m[:, None]
    assert TB._bits(got, want if out == "f32" else want.to(lpt))
    return [r.kernel for r in rec]


def _gelu_case(out, lp, zero=False):
    lpt, variant = LP(), None if out == "f32" else lp
    g = torch.Generator().manual_seed(6)
    u = _z(2.0 * torch.randn(ROWS, WIDTH, generator=g), zero).cuda()
    dg = torch.randn(ROWS, WIDTH, generator=g).cuda()
    with O.record_routes() as rr:
        gg, du = O.gelu_fwd(u, variant), O.gelu_bwd_cast(u, dg, variant)
    _sync()
    arm = "f32" if out == "f32" else "b16"
    rec = _routes(rr, [f"gelu_fwd_kernel<{arm}>", f"gelu_bwd_cast_kernel<{arm}>"])
    if not zero:
        u64 = u.double().requires_grad_(True)
        g64 = F.gelu(u64)
        g64.backward(dg.double())
        u32 = u.clone().requires_grad_(True)
        g32 = F.gelu(u32)
        g32.backward(dg)
        g32, du32 = g32.detach(), u32.grad
        if variant is not None:
            g32, du32 = g32.to(lpt), du32.to(lpt)
        TB._assert_vs_torch(f"gelu {out} ({lp})", [("g", gg, g32, g64.detach()), ("du", du, du32, u64.grad)])
    return [r.kernel for r in rec]


def _wgrad32_case(det, zero=False):
    M, N, K = 65, 16, 16
    rng = np.random.default_rng(9)
    x, dy = _z(_ints(rng, M, K), zero), _z(_ints(rng, M, N), zero)
    part = O.wgrad_partition(M, N, K, 1, torch.float32)
    xd, xb = GB.poisoned_input(x.cuda(), name="x")
    dyd, dyb = GB.poisoned_input(dy.cuda(), name="dy")
    dw, wb = GB.banded((N, K), torch.float32, fill=-77.0, name="dw")
    dbuf, bb = GB.banded((1, N), torch.float32, cols=0, fill=-77.0, name="db")
    dw.zero_(), dbuf.zero_()
    with O.record_routes() as rr:
        O.linear_wgrad(xd, dyd, dw, dbuf[0], **O.det_kw(det))
    _sync()
    for b in (xb, dyb, wb, bb):
        b.check()
    r, = _routes(rr, ["wgrad_det_kernel" if det else "wgrad_kernel"])
    assert (r.bm, r.bn, r.splits, r.xmode, r.aux) == (64, 64, part.splits, part.rows_per_split, 1), r
    want_w, want_b = _exact(dy, x)
    assert _eq(dw, want_w) and _eq(dbuf[0], want_b)
    return [r.kernel]


def _layernorm_bwd_case(det, zero=False):
    M, C = 65, 48
    x, gamma, dy, pre = TF._ln_inputs(M, C, [], 7)
    x, dy = _z(x, zero), _z(dy, zero)
    dx, dg, db = torch.zeros(M, C, device="cuda"), torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    with O.record_routes() as rr:
        O.layernorm_bwd(x, gamma, dy, dx, eps=EPS, dgamma=dg, dbeta=db, **O.det_kw(det))
    _sync()
    rec = _routes(rr, ["layernorm_bwd_det_kernel" if det else "layernorm_bwd_kernel"])
    assert rec[0].bn == C
    if not zero:
        _, dx64, dg64, db64 = TF._ln_autograd(x, gamma, dy, torch.float64)
        _, dxt, dgt, dbt = TF._ln_autograd(x, gamma, dy, torch.float32)
        TF._assert_vs_torch(f"layernorm_bwd ({M}, {C}) det={det}", [("dx", dx, dxt, dx64, None), ("dgamma", dg, dgt, dg64, None),
                                                                    ("dbeta", db, dbt, db64, None)])
    return [r.kernel for r in rec]


def _pool_case(cin, cout, fold, lp, zero=False):
    """The smallest cases of tests/test_gpu_level_fused.py: one wave's group and a row, both folds forced; bits of the two
    launches the kernel replaces."""
    m = 17
    d = LF.pool_case(lp, cin, cout, m, "mixed", "normal")
    bf = LP()
    xi, xband = GB.poisoned_input(_z(d["x"], zero), rows=64, name="x")
    out, band = GB.banded((m, cout), torch.float32, rows=64, fill=-7.0, name="out")
    out2, band2 = GB.banded((m, cout), bf, rows=64, fill=-7.0, name="out2")
    seg, seg_check = GB.guard_index(d["seg"], rows=64)
    with O.pool_fused_fold(fold), O.record_routes() as rr:
        O.pool_fused(xi, d["img"], d["b"], seg, m, d["sc"], d["sh"], O.ACT_GELU, out, out2)
    _sync()
    band.check(), band2.check(), xband.check(), seg_check()
    r, = _routes(rr, [f"pool_fused_kernel<{cin},{cout},{'scan' if fold == O.POOL_FOLD_SCAN else 'walk'}>"])
    assert (r.fix, r.aux) == (fold, fold), r
    if not zero:
        assert GB.same_bits(out, d["ref"]) and GB.same_bits(out2, d["ref2"])
    return [r.kernel]


def _unpool_case(ks, kp, lp, zero=False):
    n, c = 100, 64
    d = LF.unpool_case(lp, ks, kp, c, n, "mixed")
    bf, m = LP(), d["m"]
    xs, xsb = GB.poisoned_input(_z(d["xs"], zero), rows=64, name="skip_x")
    xp, xpb = GB.poisoned_input(_z(d["xp"], zero), rows=64, name="coarse_x")
    out, band = GB.banded((n, c), torch.float32, rows=64, fill=-7.0, name="x")
    out2, band2 = GB.banded((n, c), bf, rows=64, fill=-7.0, name="xc")
    seg, seg_check = GB.guard_index(d["seg"], rows=64)
    with O.record_routes() as rr:
        O.unpool_fused(xs, d["img_s"], *d["ps"], xp, d["img_p"], *d["pp"], seg, m, O.ACT_GELU, out, out2)
    _sync()
    for b in (xsb, xpb, band, band2):
        b.check()
    seg_check()
    r, = _routes(rr, [f"unpool_fused_kernel<{ks},{kp}>"])
    if not zero:
        assert GB.same_bits(out, d["ref"]) and GB.same_bits(out2, d["ref2"])
    return [r.kernel]


# classes -> <G, E> of launch_by_width (csrc/loss.hip): 16 lanes a row up to 32 classes, 64 above; E classes a lane
LOSS_WIDTHS = {13: (16, 1), 20: (16, 2), 40: (64, 1), 100: (64, 2), 200: (64, 4)}


def _loss_case(c, lp, zero=False):
    n = 65
    G, E = LOSS_WIDTHS[c]
    t, labels, win, o, tor = SL.reference(n, c, "ignore7")
    with O.record_routes() as rr:
        got, saved = SL.fused(O, _z(t, zero), labels, win)
    rec = _routes(rr, [f"loss_rows_kernel<{G},{E}>", f"loss_bwd_kernel<{G},{E}>", f"loss_bwd_kernel<{G},{E}>"])
    assert all((r.bn, r.aux) == (c, len(o["present"])) for r in rec), rec
    if not zero:
        for k in ("ce", "lovasz", "d_ce", "d_lovasz"):
            top, e_ref, e_ker = float(o[k].abs().max()), float((tor[k] - o[k]).abs().max()), float((got[k] - o[k]).abs().max())
            bound = 2.0 * e_ref + U * top
            report(f"seg_loss C={c} <{G},{E}> {k} ({lp})", kernel_err=e_ker, E_ref=e_ref, bound=bound, err_over_bound=e_ker / bound)
            assert e_ker <= bound, (k, e_ker, e_ref, top)
    return [r.kernel for r in rec]


def _skip_case(c, dtype, lp, zero=False):
    """c = 20: the 16-byte arms; c = 30: the scalar ones.  dtype "b16": the stats and the fold read 16-bit operands."""
    n = 65
    lpt = LP() if dtype == "b16" else None
    x, child, cluster, ref = SK._case(n, c, 7 * n + c, lpt)
    x = _z(x, zero)
    xd, refd = x.cuda(), ref.cuda()
    arm, sc = ("b16" if lpt is not None else "f32"), ("_scalar" if c % 4 else "")
    w = torch.randn(c, c, generator=torch.Generator().manual_seed(n + c)) / c ** 0.5
    if lpt is not None:
        w = w.to(lpt)
    with O.record_routes() as rr:
        st = O.skip_stats(xd, refd)
        u = O.skip_fold(w.cuda(), st)
    _sync()
    rec = _routes(rr, [f"sk_stats{sc}_kernel<{arm}>", f"sk_fold_kernel<{arm}>"])
    assert rec[0].vec_ok == (c % 4 == 0) and rec[0].splits == O.skip_partition(n, c)[1], rec
    names = [r.kernel for r in rec]
    if not zero:
        want = SR.stats(x, ref)
        scale = x.double().abs().sum(0).repeat(3)
        rel = float(((st.cpu() - want).abs() / scale).max())
        want_u = (want.view(3, c) @ w.double().t()).reshape(-1)
        rel_u = float(((u.cpu() - want_u).abs() / (scale.view(3, c) @ w.double().abs().t()).reshape(-1)).max())
        report(f"skip stats / fold {n}x{c} {arm}", stats_rel=rel, fold_rel=rel_u, bound=SK.STATS_REL)
        assert rel <= SK.STATS_REL and rel_u <= SK.STATS_REL
    if lpt is None:  # the merge works on the fp32 stream
        y = xd.clone()
        with O.record_routes() as rr:
            O.skip_merge(y, st, 0.8, 0.75, refd, None, child.cuda(), cluster.cuda())
        _sync()
        rec = _routes(rr, [f"sk_merge{sc}_kernel"])
        assert rec[0].vec_ok == (c % 4 == 0)
        names.append(rec[0].kernel)
        if not zero:
            want_y = SR.merge(x, SR.stats(x, ref), 0.8, 0.75, ref, None, child, cluster)
            mag = torch.maximum((0.75 * x.double().abs()).clamp(min=1e-30),
                                abs(0.75 * SR.k_of(0.8, n)) * SR.wave(SR.stats(x, ref), n, ref).abs())
            mag = torch.maximum(mag, child.double()[cluster.long()].abs())
            worst = [0.0]
            SK._check_merge(f"merge {n}x{c}", y, want_y, torch.maximum(mag, want_y.abs()), worst)
            report(f"skip merge {n}x{c}", ulps=worst[0], bound=SK.ULPS)
    return names


def _fusion_case(c, zero=False):
    """c = 32: the 16-byte arms; c = 30: the scalar ones."""
    rows = 65
    s, a, dy, m, alpha, gamma = FU._operands(rows, c, True, 1000 * rows + c)
    s, a, dy = _z(s, zero), _z(a, zero), _z(dy, zero)
    sc = "_scalar" if c % 4 else ""
    with O.record_routes() as rr:
        y = O.fuse_gate_fwd(s, a, alpha, gamma, m)
        ds, da, sums = O.fuse_gate_bwd(dy, s, a, alpha, gamma, m)
    _sync()
    rec = _routes(rr, [f"fg_fwd{sc}_kernel", f"fg_bwd{sc}_kernel"])
    assert all(r.vec_ok == (c % 4 == 0) for r in rec), rec
    if not zero:
        d = lambda t: t.double()  # noqa: E731
        m2 = m[:, None]
        FU._within(f"route fwd {rows}x{c}", y, alpha * s + gamma * (m2 * a), d(alpha) * d(s) + d(gamma) * (d(m2) * d(a)))
        FU._within(f"route bwd ds {rows}x{c}", ds, alpha * dy, d(alpha) * d(dy))
        FU._within(f"route bwd da {rows}x{c}", da, gamma * (dy * m2), d(gamma) * (d(dy) * d(m2)))
        FU._within(f"route bwd sum dy m a {rows}x{c}", sums[:c], ((dy * m2) * a).sum(0), ((d(dy) * d(m2)) * d(a)).sum(0))
        FU._within(f"route bwd sum dy s {rows}x{c}", sums[c:], (dy * s).sum(0), (d(dy) * d(s)).sum(0))
    return [r.kernel for r in rec]


# name -> (the case, its arguments, builds it runs in)
OTHER = {}
for _o in ("f32", "b16"):
    _b = BOTH if _o == "b16" else BOTH[:1]
    OTHER[f"gather_first-{_o}"] = (_gather_first_case, (_o,), _b, True)
    OTHER[f"scale_cast-{_o}"] = (_scale_cast_case, (_o,), _b, True)
    OTHER[f"gelu-{_o}"] = (_gelu_case, (_o,), _b, True)
    OTHER[f"skip-20-{_o}"] = (_skip_case, (20, _o), _b, True)
    OTHER[f"skip-30-{_o}"] = (_skip_case, (30, _o), _b, True)
for _mode in ("acc", "set"):
    OTHER[f"scatter_first-{_mode}"] = (_scatter_first_case, (_mode,), BOTH[:1], False)
for _det in (False, True):
    OTHER[f"wgrad-fp32-{'det' if _det else 'atomic'}"] = (_wgrad32_case, (_det,), BOTH[:1], False)
    OTHER[f"layernorm_bwd-{'det' if _det else 'atomic'}"] = (_layernorm_bwd_case, (_det,), BOTH[:1], False)
for _cin, _cout in ((32, 64), (64, 128)):
    OTHER[f"pool-{_cin}-{_cout}-walk"] = (_pool_case, (_cin, _cout, O.POOL_FOLD_WALK), BOTH, True)
    OTHER[f"pool-{_cin}-{_cout}-scan"] = (_pool_case, (_cin, _cout, O.POOL_FOLD_SCAN), BOTH, True)
    OTHER[f"unpool-{_cin}-{_cout}"] = (_unpool_case, (_cin, _cout), BOTH, True)
for _c in LOSS_WIDTHS:
    OTHER[f"loss-{_c}"] = (_loss_case, (_c,), BOTH, True)
for _c in (32, 30):
    OTHER[f"fusion-{_c}"] = (_fusion_case, (_c,), BOTH[:1], False)
OTHER_PARAMS = [(name, lp) for name, (_, _, builds, _) in OTHER.items() for lp in builds]


def _other(name, lp, zero=False):
    fn, args, _, takes_lp = OTHER[name]
    return fn(*args, lp, zero=zero) if takes_lp else fn(*args, zero=zero)


@pytest.mark.parametrize("name,lp", OTHER_PARAMS, ids=[f"{n}-{lp}" for n, lp in OTHER_PARAMS])
def test_other_family_route_vs_its_reference(name, lp):
    assert _other(name, lp)


# ============================================================================================ the census
# Compiled and catalogued, yet behind a constant or a rule that no caller can get past: name -> why.  (Empty: every kernel of
# these choosers is reachable through the public ABI.)
OFF = {}
# the catalogue's families that belong to cdseg_gemm (tests/test_gpu_routes.py) and to the forward (tests/test_gpu_ops.py,
# test_gpu_cpe_head_stream.py, test_gpu_deep512_rows64.py, test_gpu_attention_range.py, test_gpu_dropout.py)
ELSEWHERE = ("gemm_kernel<", "gemm_dma_kernel<", "mlp_fused_kernel<", "cpe_head_stream_kernel<", "cpe_head_fused_kernel<",
             "deep_head_kernel<", "deep_tail_kernel<", "head_rr_kernel<", "tail_rr_kernel<", "conv_ll_kernel<", "attn_bf16_kernel<",
             "attn_x3_kernel", "attn_f32_kernel", "dropout_kernel")


# the kernels that read or write the build's 16-bit type (next to those with "b16" in their name): the second build's duty
LP_FAMILIES = ("layernorm_kernel<", "wgrad16_kernel<", "wgrad16_det_kernel<", "attn_bwd16_", "attn_drop16_kernel", "pool_fused_kernel<",
               "unpool_fused_kernel<")


def _table(lp):
    """Every case of this module that runs in build `lp`: (the kernels its route names, a replay on zero operands)."""
    first = lp == BOTH[0]
    for c, f, b in LN_PARAMS:
        if b == lp:
            yield {f"layernorm_kernel<{LN_ROUTE[c][0]}>"}, lambda c=c, f=f: _layernorm_case(c, f, lp, zero=True)
    for c, o, mk, b in ALN_PARAMS:
        if b == lp and not mk:
            yield ({f"add_layernorm_kernel<{LN_ROUTE[c][0]},{'f32' if o == 'fp32' else 'b16'}>"},
                   lambda c=c, o=o: _add_layernorm_case(c, o, False, lp, zero=True))
    for n, k, tn, tk, f, b in W16_PARAMS:
        if b == lp and f != "gathered":
            yield ({f"wgrad16_kernel<{tn},{tk}>", f"wgrad16_det_kernel<{tn},{tk}>"},
                   lambda n=n, k=k, tn=tn, tk=tk, f=f: _wgrad16_case(n, k, tn, tk, f, lp, zero=True, rows=(65,)))
    for P, H, s16, s32 in ATTN_SPLIT[:1]:
        yield ({"attn_bwd16_q_kernel<>", "attn_bwd16_kv_kernel<>", "attn_drop16_kernel", "attn_bwd16_q_kernel<DropP>",
                "attn_bwd16_kv_kernel<DropP>"}, lambda P=P, H=H, s=s16: _attn16_case(P, H, s, lp, zero=True))
        if first:
            yield ({"attn_drop_f32_kernel", "attn_bwd_q_mfma_kernel<DropP>", "attn_bwd_kv_mfma_kernel<DropP>",
                    "attn_bwd_q_mfma_kernel<>", "attn_bwd_kv_mfma_kernel<>"}, lambda P=P, H=H, s=s32: _attn32_case(P, H, s, zero=True))
    for name, b in OTHER_PARAMS:
        if b == lp:
            yield None, lambda name=name: _other(name, lp, zero=True)


@pytest.mark.parametrize("lp", BOTH)
def test_every_catalogued_variant_outside_the_gemm_is_reached_or_accounted_for(lp):
    """Self-contained: replays the launches of the case tables above on zero operands, collects the recorded kernels and holds
    them against the catalogue minus the GEMM and forward families and minus OFF.  The fp32-only cases run in the first build
    alone (their kernels do not depend on the 16-bit type), so the second build is held to the kernels with a 16-bit arm."""
    catalogue = {n for n in O.route_catalog() if not n.startswith(ELSEWHERE)}
    assert set(OFF) <= catalogue, set(OFF) - catalogue  # a reason for a kernel that is not compiled is stale
    reached, named = set(), set()
    for names, replay in _table(lp):
        got = set(replay())
        assert got, "a case that records nothing"
        if names is not None:
            assert got == names, (names, got)  # the table names a kernel the run does not reach (or the reverse)
        named |= got if names is None else names
        reached |= got
    assert not (reached - catalogue), f"recorded names the catalogue does not have: {sorted(reached - catalogue)}"
    assert not (reached & set(OFF)), f"listed as unreachable, yet a case reaches it: {sorted(reached & set(OFF))}"
    assert named == reached
    want = catalogue if lp == BOTH[0] else {k for k in catalogue if "b16" in k or k.startswith(LP_FAMILIES)}
    missing = sorted(want - reached - set(OFF))
    assert not missing, f"catalogued kernels that no case of this module runs and OFF does not explain: {missing}"
