"""GPU: the skip-connection options - the kernels of csrc/skip.hip against the fp64 restatement (tests/skip_restatement.py),
and skip_connection_mode "add" / "cat_all", skip_connection_scale(_i) and s_factor / b_factor end to end (inference engine,
training graph) against the reference's recordings (tools/make_skip_golden.py -> tests/golden/skip_*.npz).  Host logic on the
CPU: tests/test_cpu_skip.py."""
import warnings

import numpy as np
import pytest
import torch

import cdsegnet_amd.models  # noqa: F401
import cdsegnet_amd.ops as O
import cdsegnet_amd.train_graph as tg
from cdsegnet_amd import _lib
from cdsegnet_amd.optim import FusedAdamW
from tests import colsum_rule, guard_bands as GB, skip_restatement as R
from tests.helpers import fixture_input, load_fixture
from tests.skip_helpers import INFER, ddim_draws, fixture_model, ssi_draws, train_draws

pytestmark = pytest.mark.gpu

# The kernels evaluate every output in fp64 from the stored operands and round once, the restatement does the same on the CPU
# with another summation order: the two fp64 values differ by ~1e-13 relative to the largest term, so the fp32 results differ
# where that moves a rounding boundary - by one unit in the last place of the LARGEST TERM of the expression (the sum itself
# may cancel).  Measured worst case over every case below: 0 ulp (the same bits); twice that is no bound for other data, so the
# assertion stands at the smallest non-zero value of the measure, one ulp.
ULPS = 1.0
# [S0 A B] in fp64 against the restatement's fp64 sums, relative to sum |x|: both add in blocks (the kernel: a lane's rows, the
# row slots, at most 256 chunks; torch: pairwise), so either is within (a few hundred) * 2^-53 ~ 5e-14 of the exact sum, and
# cos / sin of the two differ by ~1e-15 (the rounding of 2 pi m / N)
STATS_REL = 1e-12


def _ulp(mag):
    """One fp32 unit in the last place at magnitude `mag` (fp64 tensor)."""
    e = torch.floor(torch.log2(mag.clamp(min=2.0 ** -126)))
    return torch.exp2(e - 23.0)


def _case(n, c, seed, lp=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, generator=g) * 3 + 0.5
    if lp is not None:
        x = x.to(lp)
    m = max(1, n // 3)
    child = torch.randn(m, c, generator=g)
    cluster = torch.randint(0, m, (n,), generator=g).to(torch.int32)
    ref = torch.randperm(n, generator=g).to(torch.int32)
    return x, child, cluster, ref


def _check_merge(name, have, want, mag, worst):
    err = (have.double().cpu() - want.float().double()).abs() / _ulp(mag)
    w = float(err.max())
    worst[0] = max(worst[0], w)
    assert w <= ULPS, f"{name}: {w} ulp"


NS = [2, 3, 5, 63, 64, 65, 777, 3001, 16449]  # 64 rows a chunk up to 16384 rows (3001: 47 chunks, more than the finish adds in one
# segment); 16449 rows: 129 chunks of 128
CS = [64, 128, 256, 20, 30]  # 20: five 16-byte lanes a row; 30: the scalar path


@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("n", NS)
def test_kernels_vs_the_fp64_restatement(n, c):
    rpc, chunks = O.skip_partition(n, c)
    assert (rpc, chunks) == ((64, -(-n // 64)) if n <= 16384 else (128, -(-n // 128)))
    worst = [0.0]
    for variant, lp in (("bf16", None), ("bf16", torch.bfloat16), ("f16", torch.float16)):
        with _lib.use(variant):
            x, child, cluster, ref = _case(n, c, 7 * n + c, lp)
            xd, chd, cld, refd = x.cuda(), child.cuda(), cluster.cuda(), ref.cuda()
            for rmap, rmapd in ((None, None), (ref, refd)):
                with O.record_routes() as rr:
                    st = O.skip_stats(xd, rmapd)
                # the launch record: the 16-byte arm for a width that is a multiple of four, else the scalar one
                arm = f"sk_stats{'_scalar' if c % 4 else ''}_kernel<{'f32' if lp is None else 'b16'}>"
                assert rr.count == 1 and rr.kernels() == [arm] and rr.routes[0].splits == chunks, rr.routes
                want = R.stats(x, rmap)
                scale = x.double().abs().sum(0).repeat(3)
                rel = float(((st.cpu() - want).abs() / scale).max())
                assert rel <= STATS_REL, f"stats {n}x{c} {lp}: {rel}"
                assert GB.same_bits(st, O.skip_stats(xd, rmapd))  # two runs, the same bits
                if lp is not None:
                    continue
                x64 = x.double()
                for s, f, with_child, with_stats in ((0.8, 1.0, True, True), (1.1, 0.8838834764831844, True, True),
                                                     (0.9, 1.25, False, True), (1.0, 0.64, True, False), (1.0, 0.8, False, False)):
                    y = xd.clone()
                    with O.record_routes() as rr:
                        O.skip_merge(y, st if with_stats else None, s, f, rmapd, None, chd if with_child else None,
                                     cld if with_child else None)
                    assert rr.kernels() == [f"sk_merge{'_scalar' if c % 4 else ''}_kernel"], rr.routes
                    want_y = R.merge(x, R.stats(x, rmap) if with_stats else None, s, f, rmap, None,
                                     child if with_child else None, cluster if with_child else None)
                    mag = (abs(f) * x64.abs()).clamp(min=1e-30)
                    if with_stats:
                        mag = torch.maximum(mag, abs(f * R.k_of(s, n)) * R.wave(R.stats(x, rmap), n, rmap).abs())
                    if with_child:
                        mag = torch.maximum(mag, child.double()[cluster.long()].abs())
                    _check_merge(f"merge {n}x{c} s={s} f={f} child={with_child}", y, want_y, torch.maximum(mag, want_y.abs()), worst)
                # folded: x + f k (u0 + u1 cos + u2 sin)
                w = torch.randn(c, c, generator=torch.Generator().manual_seed(n + c)) / c ** 0.5
                with O.record_routes() as rr:
                    u = O.skip_fold(w.cuda(), st)
                assert rr.kernels() == ["sk_fold_kernel<f32>"], rr.routes
                want_u = (R.stats(x, rmap).view(3, c) @ w.double().t()).reshape(-1)
                assert float(((u.cpu() - want_u).abs() / (scale.view(3, c) @ w.double().abs().t()).reshape(-1)).max()) <= STATS_REL
                y = xd.clone()
                O.skip_merge(y, u, 0.8, 0.75, rmapd, folded=True)
                want_y = R.merge(x, want_u, 0.8, 0.75, rmap, folded=True)
                mag = torch.maximum(x64.abs(), abs(0.75 * R.k_of(0.8, n)) * R.wave(want_u, n, rmap).abs())
                _check_merge(f"folded {n}x{c}", y, want_y, torch.maximum(mag, want_y.abs()), worst)
    print(f"[measure] skip kernels {n}x{c}: worst merge error {worst[0]:.3f} ulp")


def test_sixteen_bit_stats_read_the_stored_values():
    """The stats of a 16-bit feature are the stats of those 16-bit values (fp64 sums): bit-equal to the fp32 path on the same
    values on the vector path, where both add in the same order."""
    for variant, lp in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        with _lib.use(variant):
            x, _, _, ref = _case(777, 128, 3, lp)
            assert GB.same_bits(O.skip_stats(x.cuda(), ref.cuda()), O.skip_stats(x.float().cuda(), ref.cuda()))


def test_stats_are_added_in_sixteen_segments_of_chunks():
    """S0 = stats[:c] of a feature that is zero except four rows holding 2^60, -2^60, 1, 1: in fp64 a 1 added to +-2^60 is lost,
    so the sum tells the order.  Expected values: the order of csrc/colsum.h restated in tests/colsum_rule.py (64-row chunks,
    R = 32 row slots at c = 32, 16 segments of consecutive chunks), never the kernel's output.  n = 2100: 33 chunks, segments
    of 3.  Chunks 0, 2, 3, 4 holding 2^60, 1, -2^60, 1: segment 0 = 2^60 (+ 1 lost), segment 1 = -2^60 (+ 1 lost) -> 0.0, where
    one ascending chain over the chunks gives 1.0.  Chunks 0, 3, 5, 6 holding 2^60, -2^60, 1, 1: 2^60, -2^60 (+ 1 lost), 1 ->
    1.0 (a chain: 2.0).  n = 64, rows 0, 32, 1, 2 holding 2^60, 1, -2^60, 1: rows 0 and 32 are one thread's, the row slots of a
    chunk ascending -> 1.0 (ascending rows: 2.0).  The first two also on the 16-bit vector path of the bf16 build, where
    2^60 and 1 are exact; IEEE half spans 2^-24 .. 2^15 only, so no two of its values lose one another in an fp64 sum and
    the f16 build has no such leg."""
    c, big = 32, 2.0 ** 60
    assert tuple(O.skip_partition(2100, c)) == (64, 33)

    def row(chunk):
        return 64 * chunk + (17 * chunk + 5) % 64

    cases = ((2100, [row(b) for b in (0, 2, 3, 4)], [big, 1.0, -big, 1.0], 0.0, 1.0),
             (2100, [row(b) for b in (0, 3, 5, 6)], [big, -big, 1.0, 1.0], 1.0, 2.0),
             (64, [0, 32, 1, 2], [big, 1.0, -big, 1.0], 1.0, 1.0))
    for n, where, vals, want, chain in cases:
        column = [0.0] * n
        for r, v in zip(where, vals):
            column[r] = v
        restated = colsum_rule.ordered_sum(column, c, colsum_rule.MIN_ROWS_SWEEP, 16)
        assert restated == want and colsum_rule.ordered_sum(column, c, colsum_rule.MIN_ROWS_SWEEP, 1) == chain
        x = torch.tensor(column, dtype=torch.float32)[:, None].repeat(1, c)
        legs = [(v, None) for v in _lib.VARIANTS] + ([("bf16", torch.bfloat16)] if n == 2100 else [])
        for variant, lp in legs:
            with _lib.use(variant):
                with O.record_routes() as rr:
                    st = O.skip_stats((x if lp is None else x.to(lp)).cuda())
            assert rr.kernels() == [f"sk_stats_kernel<{'f32' if lp is None else 'b16'}>"], rr.routes
            print(f"[measure] skip S0 {n}x{c} rows {where} {variant} {lp}: {st[:2].tolist()} .. (restated {restated})")
            assert torch.equal(st[:c], torch.full((c,), restated, dtype=torch.float64, device="cuda")), (n, where, variant, lp, st[:c])


def test_row_map_permutes_and_backward_is_the_transpose():
    n, c = 3001, 64
    x, _, _, ref = _case(n, c, 11)
    xd, refd = x.cuda(), ref.cuda()
    # physical row r holds reference row ref[r]: filtering the permuted rows under the map = permuting the filtered rows.  The
    # sums are added in another order, so the stats agree to fp64 rounding and the outputs to the kernels' one ulp
    y_id = O.skip_merge(xd.clone(), O.skip_stats(xd), 0.8)
    inv = torch.empty_like(ref)
    inv[ref.long()] = torch.arange(n, dtype=torch.int32)
    xp = x[inv.long()]  # row m of xp... reference row m of x lives at physical row r with ref[r] = m
    y_map = O.skip_merge(xd.clone(), O.skip_stats(xd, refd), 0.8, ref_of_row=refd)
    y_perm = O.skip_merge(xp.cuda().clone(), O.skip_stats(xp.cuda()), 0.8)
    assert float(((y_map.cpu() - y_perm.cpu()[ref.long()]).double().abs() / _ulp(x.double().abs())).max()) <= ULPS
    assert not torch.equal(y_map, y_id)
    # the training node: its backward equals the transpose of the restatement (the filter is self-adjoint)
    xg = xd.clone().requires_grad_(True)
    dy = torch.randn(n, c, generator=torch.Generator().manual_seed(2))
    out = tg._SkipFilter.apply(xg, refd, 0.8)
    out.backward(dy.cuda())
    x64 = x.double().requires_grad_(True)
    (R.closed_filter(x64, 0.8, ref=ref) * dy.double()).sum().backward()
    assert float(((xg.grad.cpu().double() - x64.grad.float().double()).abs() / _ulp(dy.double().abs())).max()) <= ULPS
    xg2 = xd.clone().requires_grad_(True)
    tg._SkipFilter.apply(xg2, refd, 0.8).backward(dy.cuda())
    assert GB.same_bits(xg.grad, xg2.grad) and GB.same_bits(out.detach(), O.skip_merge(xd.clone(), O.skip_stats(xd, refd), 0.8,
                                                                                    ref_of_row=refd))


@pytest.mark.parametrize("n,c", [(1, 64), (65, 128), (257, 256), (300, 20), (130, 30)])
def test_kernels_write_only_what_they_were_given(n, c):
    x, child, cluster, ref = _case(n, c, 5)
    lib = _lib.load()
    xin, xinb = GB.poisoned_input(x.cuda(), name="x")  # (a row stride: guard columns left and right)
    refg, refchk = GB.guard_index(ref.cuda())
    clg, clchk = GB.guard_index(cluster.cuda())
    chin, chb = GB.poisoned_input(child.cuda(), name="child")
    stats, sb = GB.banded((1, 3 * c), torch.float64, rows=8, cols=0, fill=float("nan"), name="stats")
    nbytes = lib.cdseg_skip_stats_ws_bytes(n, c)
    assert nbytes == -(-n // 64) * 3 * c * 8
    ws, wb = GB.exact_workspace(nbytes)
    args = (O._ptr(xin), O.F32, xin.stride(0), n, c, O._ptr(refg), n, O._ptr(stats), O._ptr(ws))
    O.check(lib.cdseg_skip_stats(*args, ws.numel(), O._stream()), "skip_stats")
    assert GB.same_bits(stats.reshape(-1), O.skip_stats(x.cuda(), ref.cuda()))
    u, ub = GB.banded((1, 3 * c), torch.float64, rows=8, cols=0, fill=float("nan"), name="u")
    w = torch.randn(c, c, generator=torch.Generator().manual_seed(1)).cuda()
    O.check(lib.cdseg_skip_fold(O._ptr(w), O.F32, c, c, c, O._ptr(stats), O._ptr(u), O._stream()), "skip_fold")
    st = stats.reshape(-1).clone()
    O.check(lib.cdseg_skip_merge(O._ptr(xin), xin.stride(0), n, c, O._ptr(st), 0, 0.8, n, 0.75, O._ptr(refg), O._ptr(chin),
                                 chin.stride(0), O._ptr(clg), child.shape[0], O._stream()), "skip_merge")
    want = O.skip_merge(x.cuda().clone(), st, 0.8, 0.75, ref.cuda(), None, child.cuda(), cluster.cuda())
    assert GB.same_bits(xin, want)
    for b in (xinb, chb, sb, ub, wb):
        b.check()
    refchk()
    clchk()
    # the stated preconditions come back as status codes, before any launch
    assert lib.cdseg_skip_stats(*args, max(ws.numel() - 1, 0), O._stream()) == -3  # CDSEG_ERR_WORKSPACE
    assert lib.cdseg_skip_stats(O._ptr(xin), O.F32, xin.stride(0), n, 516, O._ptr(refg), n, O._ptr(stats), O._ptr(ws), ws.numel(),
                                O._stream()) == -4  # CDSEG_ERR_UNSUPPORTED
    assert lib.cdseg_skip_stats(O._ptr(xin), O.F32, c - 1, n, c, O._ptr(refg), n, O._ptr(stats), O._ptr(ws), ws.numel(),
                                O._stream()) == -1  # CDSEG_ERR_ARG: a row stride below the width
    assert lib.cdseg_skip_merge(O._ptr(xin), xin.stride(0), n, c, None, 1, 0.8, n, 0.75, None, None, 0, None, 0, O._stream()) == -1
    assert lib.cdseg_skip_merge(O._ptr(xin), xin.stride(0), n, c, None, 0, 0.8, n, 0.75, None, O._ptr(chin), chin.stride(0), None,
                                child.shape[0], O._stream()) == -1  # child without cluster
    torch.cuda.synchronize()
    assert GB.same_bits(xin, want)
    for b in (xinb, chb, sb, ub, wb):
        b.check()


# ------------------------------------------------------------------------------------------ inference vs the reference
def _dev(fx):
    return {k: torch.as_tensor(v).cuda() for k, v in fixture_input(fx).items()}


def _report(name, out, ref):
    err = float(np.abs(out - ref).max())
    agree = float((out.argmax(1) == ref.argmax(1)).mean())
    print(f"[measure] {name}: max_abs_err={err:.3e} argmax_agreement={agree:.5f}")
    return err, agree


def _model(fx, **override):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model, cfg = fixture_model(fx, **override)
    return model.cuda(), cfg


@pytest.mark.parametrize("tag", list(INFER))
def test_inference_matches_the_reference_recordings(tag):
    fx = load_fixture(f"skip_infer_{tag}.npz")
    model, cfg = _model(fx)
    model.precision = "fp32"
    inp = _dev(fx)
    kw = dict(T=cfg["T"], step=2, eval=False, mode="avg")
    ssi = model.inference(dict(inp), eval=False, draws=ssi_draws(fx))["seg_logits"]
    err, agree = _report(f"skip {tag} fp32 vs reference", ssi.cpu().numpy(), fx["logits"])
    assert err < 1e-3 and agree > 0.999  # tests/test_gpu_fusion.py: the fp32 logit bound of its recordings
    msi = model.inference_ddim(dict(inp), draws=ddim_draws(fx), **kw)["seg_logits"]
    err, _ = _report(f"skip {tag} fp32 multi-step vs reference", msi.cpu().numpy(), fx["ddim_logits"])
    assert err < 5e-5  # ... and its multi-step bound
    # the same logits, bit for bit: with a shared plan, with the hoisted n-encoder
    plan = model.plan(dict(inp))
    built = model.engine().plans_built
    assert torch.equal(ssi, model.inference(dict(inp), eval=False, draws=ssi_draws(fx), plan=plan)["seg_logits"])
    assert torch.equal(msi, model.inference_ddim(dict(inp), draws=ddim_draws(fx), plan=plan, **kw)["seg_logits"])
    assert model.engine().plans_built == built
    d = ddim_draws(fx)
    perms = [np.array(p) for p in d["perms"]]
    for call in (1, 2):  # draws that repeat the first call's n-branch shuffles
        for j in (1, 3, 4, 6, 7):
            perms[8 * call + j] = perms[j]
    a = model.inference_ddim(dict(inp), draws=dict(d, perms=list(perms)), **kw)["seg_logits"]
    b = model.inference_ddim(dict(inp), draws=dict(d, perms=list(perms)), reuse_encoder=True, **kw)["seg_logits"]
    assert model.engine().msi_stats["n_encoders"] == 1 and torch.equal(a, b)
    if len(fx["offset"]) == 2:  # inference_many(batch=2) on the two rooms = the collated inference under the same draws
        n0 = int(fx["offset"][0])
        n1 = int(fx["offset"][1]) - n0
        parts = [{k: (v[:n0] if k != "offset" else torch.tensor([n0], device=v.device)) for k, v in inp.items()},
                 {k: (v[n0:] if k != "offset" else torch.tensor([n1], device=v.device)) for k, v in inp.items()}]
        outs = model.inference_many(parts, batch=2, draws=[ssi_draws(fx)])
        assert torch.equal(ssi, torch.cat([o["seg_logits"] for o in outs]))
    # 16-bit trunks against the fp32 HIP logits: the bounds tests/test_gpu_e2e.py uses for the mini model
    ref = ssi.cpu().numpy()
    for precision, tol, min_agree in (("fp16+head", 3e-3, 0.9965), ("bf16+head", 0.04, 0.985)):
        model.precision = precision
        model.count_saturation = precision.startswith("fp16")
        out = model.inference(dict(inp), eval=False, draws=ssi_draws(fx))["seg_logits"].cpu().numpy()
        err, agree = _report(f"skip {tag} {precision} vs fp32", out, ref)
        assert np.isfinite(out).all() and err < tol and agree > min_agree
        if model.count_saturation:
            assert model.engine().saturation_count == 0
        model.count_saturation = False


def test_b_factor_alone_changes_no_bit():
    fx = load_fixture("skip_infer_b_only.npz")
    inp = _dev(fx)
    outs = []
    for override in ({}, dict(b_factor=[1.0] * 4)):
        model, cfg = _model(fx, **override)
        model.precision = "fp32"
        outs.append(model.inference(dict(inp), eval=False, draws=ssi_draws(fx))["seg_logits"])
        outs.append(model.inference_ddim(dict(inp), T=cfg["T"], step=2, eval=False, mode="avg", draws=ddim_draws(fx))["seg_logits"])
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3])


def test_default_model_calls_no_new_entry_point(monkeypatch):
    fx = load_fixture("skip_infer_b_only.npz")
    model, cfg = _model(fx, b_factor=[1.0] * 4)
    inp = _dev(fx)
    seen = []
    for name in ("skip_stats", "skip_fold", "skip_merge", "skip_partition"):
        monkeypatch.setattr(O, name, lambda *a, _n=name, **k: seen.append(_n))
    model.inference(dict(inp), eval=False, draws=ssi_draws(fx))
    model.inference_ddim(dict(inp), T=cfg["T"], step=2, eval=False, mode="avg", draws=ddim_draws(fx))
    tfx = load_fixture("skip_train_step.npz")
    tm, _ = fixture_model(tfx, train=True, skip_connection_mode="cat", skip_connection_scale_i=False)
    tm = tm.cuda()
    tm(_train_inp(tfx), draws=train_draws(tfx))["loss"].backward()
    torch.cuda.synchronize()
    assert seen == []


# ------------------------------------------------------------------------------------------ training
def _train_inp(fx):
    return {k: torch.as_tensor(fx[k]).cuda() for k in ("coord", "grid_coord", "feat", "offset", "segment")}


def _groups(model):
    named = dict(model.named_parameters())
    return [dict(params=[p for k, p in named.items() if "block" not in k], lr=0.002),
            dict(params=[p for k, p in named.items() if "block" in k], lr=0.0002)]


@pytest.mark.parametrize("train_block", ["autograd", "native"])
def test_training_step_matches_the_reference_recording(train_block):
    """'add' + skip_connection_scale_i against the reference's recorded step, with the bounds of tests/test_gpu_train.py."""
    fx = load_fixture("skip_train_step.npz")
    model, _ = fixture_model(fx, train=True)
    model = model.cuda()
    model.train_block = train_block
    named = dict(model.named_parameters())
    out = model(_train_inp(fx), draws=train_draws(fx))
    e_loss = abs(float(out["loss"].detach()) - float(fx["loss"]))
    e_n = float((out["n_pred"].detach().cpu() - torch.as_tensor(fx["n_pred"])).abs().max())
    e_c = float((out["c_pred"].detach().cpu() - torch.as_tensor(fx["c_pred"])).abs().max())
    out["loss"].backward()
    torch.cuda.synchronize()
    names = [str(n) for n in fx["grad_names"]]
    assert names == list(named) and all(named[k].grad is not None for k in names)
    gn = np.array([float(named[k].grad.norm()) for k in names])
    ref = fx["grad_norms"]
    rel = np.abs(gn - ref) / (ref + 1e-3 * ref.max())
    worst_full, checked = 0.0, 0
    for k in fx.files:
        if k.startswith("g."):
            r = fx[k]
            worst_full = max(worst_full, float((named[k[2:]].grad.cpu() - torch.as_tensor(r)).abs().max()) / float(np.abs(r).max()))
            checked += 1
    print(f"[measure] skip training step ({train_block}) vs reference: loss err {e_loss:.3e}, n_pred err {e_n:.3e}, c_pred err "
          f"{e_c:.3e}, worst gradient-norm rel err {rel.max():.3e}, worst of {checked} full gradients rel {worst_full:.3e}")
    assert e_loss < 1e-4 and e_n < 1e-3 and e_c < 1e-3
    assert rel.max() < 1e-3 and checked == 10 and worst_full < 1e-3


@pytest.mark.parametrize("train_block", ["autograd", "native"])
def test_training_forward_with_the_filter_matches_the_reference(train_block):
    """With s_factor the reference has a training-mode forward only (its freeU writes in place: no backward)."""
    fx = load_fixture("skip_train_fwd_s.npz")
    model, _ = fixture_model(fx, train=True)
    model = model.cuda()
    model.train_block = train_block
    out = model(_train_inp(fx), draws=train_draws(fx))
    e_loss = abs(float(out["loss"].detach()) - float(fx["loss"]))
    e_n = float((out["n_pred"].detach().cpu() - torch.as_tensor(fx["n_pred"])).abs().max())
    e_c = float((out["c_pred"].detach().cpu() - torch.as_tensor(fx["c_pred"])).abs().max())
    print(f"[measure] skip training forward with s_factor ({train_block}) vs reference: loss err {e_loss:.3e}, n_pred err "
          f"{e_n:.3e}, c_pred err {e_c:.3e}")
    assert e_loss < 1e-4 and e_n < 1e-3 and e_c < 1e-3
    out["loss"].backward()
    torch.cuda.synchronize()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())


def _seeded_steps(fx, steps, seed=11):
    model, _ = fixture_model(fx, train=True)
    model = model.cuda()
    model.train_deterministic = True
    opt = FusedAdamW(_groups(model), lr=0.002, weight_decay=0.05)
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)
    grads = None
    for _ in range(steps):
        opt.zero_grad()
        model(_train_inp(fx))["loss"].backward()
        grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
        opt.step()
    torch.cuda.synchronize()
    return model, grads


def test_seeded_deterministic_steps_are_bit_equal():
    fx = load_fixture("skip_train_fwd_s.npz")
    (m1, g1), (m2, g2) = _seeded_steps(fx, 2), _seeded_steps(fx, 2)
    assert all(GB.same_bits(g1[k], g2[k]) for k in g1)
    assert all(GB.same_bits(p.detach(), q.detach()) for p, q in zip(m1.parameters(), m2.parameters()))
