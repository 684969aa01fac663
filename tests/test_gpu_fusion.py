"""GPU: the Feature Fusion Module options - the gate kernels of csrc/fusion.hip against fp64, and the learned fusion scales and
bidirectional fusion end to end (inference engine, training graph) against the reference's recordings
(tools/make_fusion_golden.py -> tests/golden/fusion_*.npz).  Host logic on the CPU: tests/test_cpu_fusion.py."""
import math

import numpy as np
import pytest
import torch

import cdsegnet_amd.models  # noqa: F401
import cdsegnet_amd.ops as O
from cdsegnet_amd import _lib
from cdsegnet_amd.optim import FusedAdamW
from tests import colsum_rule, guard_bands as GB
from tests.fusion_helpers import INFER_TAGS, ddim_draws, infer_model, ssi_draws, train_draws, train_model
from tests.helpers import fixture_input, load_fixture

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ kernels vs fp64
def _ulp(ref):
    """One fp32 unit in the last place of every element of the fp64 tensor `ref` (0 for 0)."""
    a = ref.abs()
    e = torch.floor(torch.log2(torch.where(a > 0, a, torch.ones_like(a)))).clamp_(min=-126.0)
    return torch.where(a > 0, torch.exp2(e - 23.0), torch.zeros_like(a))


def _within(name, mine, theirs, ref):
    """The issue's rule, element by element: |mine - ref| <= 2 |torch fp32 - ref| + one fp32 ulp of ref."""
    em, et = (mine.double() - ref).abs(), (theirs.double() - ref).abs()
    print(f"[measure] {name}: kernel max err {float(em.max()):.3e}, torch fp32 max err {float(et.max()):.3e}, "
          f"max |ref| {float(ref.abs().max()):.3e}")
    assert bool((em <= 2 * et + _ulp(ref)).all()), name


def _operands(rows, c, masked, seed):
    g = torch.Generator().manual_seed(seed)
    s, a, dy = (torch.randn(rows, c, generator=g).cuda() for _ in range(3))
    m = ((torch.rand(rows, generator=g) > 0.3).float() / 0.7).cuda() if masked else None
    alpha, gamma = torch.randn(c, generator=g), torch.randn(c, generator=g)
    for v, special in ((alpha, {0: 0.0, 1: 1.0, 2: -1.5}), (gamma, {0: 1.0, 1: 0.0, 3: -0.25})):
        for j, x in special.items():  # vectors holding 0, 1 and negative values
            if j < c:
                v[j] = x
    return s, a, dy, m, alpha.cuda(), gamma.cuda()


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("c", [32, 128, 512])
@pytest.mark.parametrize("rows", [1, 3, 64, 65, 257])
def test_gate_kernels_vs_fp64(rows, c, masked):
    s, a, dy, m, alpha, gamma = _operands(rows, c, masked, 1000 * rows + c + masked)
    d = lambda t: t.double()  # noqa: E731
    m2 = None if m is None else m[:, None]
    ma64 = d(a) if m is None else d(m2) * d(a)
    ma32 = a if m is None else m2 * a
    # forward
    with O.record_routes() as rr:
        y = O.fuse_gate_fwd(s, a, alpha, gamma, m)
    assert rr.kernels() == ["fg_fwd_kernel"] and rr.routes[0].vec_ok, rr.routes  # (the 16-byte arm: these widths divide by 4)
    _within(f"fwd {rows}x{c}", y, alpha * s + gamma * ma32, d(alpha) * d(s) + d(gamma) * ma64)
    assert torch.equal(O.fuse_gate_fwd(s, None, alpha, gamma), O.fuse_gate_fwd(s, a, alpha, torch.zeros_like(gamma)))  # (a NULL: alpha s)
    # y aliasing s
    s2 = s.clone()
    assert O.fuse_gate_fwd(s2, a, alpha, gamma, m, out=s2) is s2 and GB.same_bits(s2, y)
    # backward
    with O.record_routes() as rr:
        ds, da, sums = O.fuse_gate_bwd(dy, s, a, alpha, gamma, m)
    assert rr.kernels() == ["fg_bwd_kernel"] and rr.routes[0].vec_ok, rr.routes
    dm64 = d(dy) if m is None else d(dy) * d(m2)
    dm32 = dy if m is None else dy * m2
    _within(f"bwd ds {rows}x{c}", ds, alpha * dy, d(alpha) * d(dy))
    _within(f"bwd da {rows}x{c}", da, gamma * dm32, d(gamma) * dm64)
    assert sums.dtype == torch.float64 and sums.shape == (2 * c,)
    _within(f"bwd sum dy m a {rows}x{c}", sums[:c], (dm32 * a).sum(0), (dm64 * d(a)).sum(0))
    _within(f"bwd sum dy s {rows}x{c}", sums[c:], (dy * s).sum(0), (d(dy) * d(s)).sum(0))
    # two runs are bit-equal (fixed summation order, no atomics)
    ds2, da2, sums2 = O.fuse_gate_bwd(dy, s, a, alpha, gamma, m)
    assert GB.same_bits(ds, ds2) and GB.same_bits(da, da2) and GB.same_bits(sums, sums2)


@pytest.mark.parametrize("rows,c", [(20000, 32), (33001, 512)])
def test_gate_kernels_many_rows(rows, c):
    """Beyond 16384 rows a block of the backward owns more than 64 rows (256 block partials at most: 20000 -> 128, 33001 -> 192
    rows a block), and beyond 4096 blocks the forward strides over its grid (C = 512: two rows a block at a time, 33001 rows)."""
    s, a, dy, m, alpha, gamma = _operands(rows, c, True, rows + c)
    d = lambda t: t.double()  # noqa: E731
    m2 = m[:, None]
    rpb, blocks = colsum_rule.partition(rows, colsum_rule.MIN_ROWS_SWEEP)
    assert rpb == (128 if rows == 20000 else 192) and blocks == -(-rows // rpb)
    assert _lib.load().cdseg_fuse_gate_ws_bytes(rows, c) == blocks * 2 * c * 8
    _within(f"fwd {rows}x{c}", O.fuse_gate_fwd(s, a, alpha, gamma, m), alpha * s + gamma * (m2 * a), d(alpha) * d(s) + d(gamma) * (d(m2) * d(a)))
    ds, da, sums = O.fuse_gate_bwd(dy, s, a, alpha, gamma, m)
    _within(f"bwd ds {rows}x{c}", ds, alpha * dy, d(alpha) * d(dy))
    _within(f"bwd da {rows}x{c}", da, gamma * (dy * m2), d(gamma) * (d(dy) * d(m2)))
    _within(f"bwd sum dy m a {rows}x{c}", sums[:c], ((dy * m2) * a).sum(0), ((d(dy) * d(m2)) * d(a)).sum(0))
    _within(f"bwd sum dy s {rows}x{c}", sums[c:], (dy * s).sum(0), (d(dy) * d(s)).sum(0))
    r = O.fuse_gate_bwd(dy, s, a, alpha, gamma, m)
    assert GB.same_bits(ds, r[0]) and GB.same_bits(da, r[1]) and GB.same_bits(sums, r[2])


def test_gate_sums_are_added_in_the_documented_order():
    """s = 1, a = 0, alpha = gamma = 1: sums[c:] = sum_r dy, and dy is zero except four rows holding 2^60, 1, -2^60, 1, so in
    fp64 the sum tells the order (a 1 added to 2^60 is lost).  Expected values: the order of csrc/colsum.h restated in
    tests/colsum_rule.py (64-row blocks, R = 32 row slots at c = 32, one chain over the blocks), never the kernel's output.
    (a) one row in each of blocks 0 .. 3: ((2^60 + 1) - 2^60) + 1 = 1.0; with the middle two swapped (2^60 - 2^60) + 1 + 1 = 2.0.
    (b) inside one block, rows 0, 32, 1, 2: rows 0 and 32 are one thread's (slot 0: 2^60 + 1 = 2^60), then the slots ascending,
    (2^60 - 2^60) + 1 = 1.0; a plain ascending-row sum would give 2.0."""
    c, big = 32, 2.0 ** 60
    lib = _lib.load()
    s, a, one = torch.ones(300, c).cuda(), torch.zeros(300, c).cuda(), torch.ones(c).cuda()
    assert lib.cdseg_fuse_gate_ws_bytes(300, c) == 5 * 2 * c * 8  # 5 blocks of 64 rows
    block_rows = [64 * b + (17 * b + 5) % 64 for b in range(4)]
    for rows, where, vals, want in ((300, block_rows, [big, 1.0, -big, 1.0], 1.0), (300, block_rows, [big, -big, 1.0, 1.0], 2.0),
                                    (64, [0, 32, 1, 2], [big, 1.0, -big, 1.0], 1.0)):
        column = [0.0] * rows
        for r, v in zip(where, vals):
            column[r] = v
        restated = colsum_rule.ordered_sum(column, c, colsum_rule.MIN_ROWS_SWEEP, 1)
        assert restated == want and math.fsum(column) == 2.0  # (the exact sum is 2 in every placement)
        dy = torch.tensor(column, dtype=torch.float32)[:, None].repeat(1, c).cuda()
        with O.record_routes() as rr:
            _, _, sums = O.fuse_gate_bwd(dy, s[:rows], a[:rows], one, one)
        assert rr.kernels() == ["fg_bwd_kernel"], rr.routes
        print(f"[measure] gate sums {rows}x{c} rows {where}: {sums[c:].tolist()[:2]} .. (restated {restated})")
        assert torch.equal(sums[c:], torch.full((c,), restated, dtype=torch.float64, device="cuda")), sums[c:]
        assert torch.equal(sums[:c], torch.zeros(c, dtype=torch.float64, device="cuda"))


@pytest.mark.parametrize("rows,c,shift", [(3, 30, 0), (65, 1, 0), (130, 511, 0), (257, 32, 1), (70, 36, 3)])
def test_gate_kernels_scalar_path(rows, c, shift):
    """A width that is no multiple of 4, or operands off a 16-byte boundary (`shift` floats), take the scalar path: the same
    rule against fp64, y aliasing s, bit-equal runs, and nothing written outside the outputs."""
    s0, a0, dy0, m0, alpha0, gamma0 = _operands(rows, c, True, 31 * rows + c)

    def off(t):  # the same values at an address `shift` floats behind a 16-byte boundary
        buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
        start = (-buf.data_ptr() // 4) % 4 + shift
        v = buf[start:start + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 * shift and v.is_contiguous()
        return v

    s, a, dy, m, alpha, gamma = (off(t) for t in (s0, a0, dy0, m0, alpha0, gamma0))
    lib = _lib.load()
    d = lambda t: t.double()  # noqa: E731
    m2 = m[:, None]
    # guard rows around the outputs; with a shift the inner views are moved off the boundary inside their bands
    n_el = rows * c
    y_flat, yb = GB.banded((1, n_el + 4), torch.float32, rows=64, cols=0, fill=float("nan"), name="y")
    ds_flat, dsb = GB.banded((1, n_el + 4), torch.float32, rows=64, cols=0, fill=float("nan"), name="ds")
    da_flat, dab = GB.banded((1, n_el + 4), torch.float32, rows=64, cols=0, fill=float("nan"), name="da")
    y, ds, da = (f.reshape(-1)[shift:shift + n_el].view(rows, c) for f in (y_flat, ds_flat, da_flat))
    sums, sb = GB.banded((1, 2 * c), torch.float64, rows=8, cols=0, fill=float("nan"), name="sums")
    ws, wb = GB.exact_workspace(lib.cdseg_fuse_gate_ws_bytes(rows, c))
    with O.record_routes() as rr:
        O.check(lib.cdseg_fuse_gate_fwd(O._ptr(s), O._ptr(a), O._ptr(m), O._ptr(alpha), O._ptr(gamma), O._ptr(y), rows, c, O._stream()),
                "fuse_gate_fwd")
        O.check(lib.cdseg_fuse_gate_bwd(O._ptr(dy), O._ptr(s), O._ptr(a), O._ptr(m), O._ptr(alpha), O._ptr(gamma), O._ptr(ds),
                                        O._ptr(da), O._ptr(sums), rows, c, O._ptr(ws), ws.numel(), O._stream()), "fuse_gate_bwd")
    assert rr.kernels() == ["fg_fwd_scalar_kernel", "fg_bwd_scalar_kernel"] and not any(r.vec_ok for r in rr.routes), rr.routes
    for b in (yb, dsb, dab, sb, wb):
        b.check()
    for f in (y_flat, ds_flat, da_flat):  # the slack inside the inner row, in front of and behind the shifted view
        flat = f.reshape(-1)
        assert bool(torch.isnan(flat[:shift]).all()) and bool(torch.isnan(flat[shift + n_el:]).all())
    _within(f"scalar fwd {rows}x{c}+{shift}", y, alpha * s + gamma * (m2 * a), d(alpha) * d(s) + d(gamma) * (d(m2) * d(a)))
    _within(f"scalar bwd ds {rows}x{c}+{shift}", ds, alpha * dy, d(alpha) * d(dy))
    _within(f"scalar bwd da {rows}x{c}+{shift}", da, gamma * (dy * m2), d(gamma) * (d(dy) * d(m2)))
    sm = sums.reshape(-1)
    _within(f"scalar bwd sum dy m a {rows}x{c}+{shift}", sm[:c], ((dy * m2) * a).sum(0), ((d(dy) * d(m2)) * d(a)).sum(0))
    _within(f"scalar bwd sum dy s {rows}x{c}+{shift}", sm[c:], (dy * s).sum(0), (d(dy) * d(s)).sum(0))
    # y aliasing s; a second run gives the same bits
    s2 = off(s0)
    O.check(lib.cdseg_fuse_gate_fwd(O._ptr(s2), O._ptr(a), O._ptr(m), O._ptr(alpha), O._ptr(gamma), O._ptr(s2), rows, c, O._stream()),
            "fuse_gate_fwd")
    assert GB.same_bits(s2, y)
    first = (ds.clone(), da.clone(), sm.clone())
    O.check(lib.cdseg_fuse_gate_bwd(O._ptr(dy), O._ptr(s), O._ptr(a), O._ptr(m), O._ptr(alpha), O._ptr(gamma), O._ptr(ds), O._ptr(da),
                                    O._ptr(sums), rows, c, O._ptr(ws), ws.numel(), O._stream()), "fuse_gate_bwd")
    assert GB.same_bits(ds, first[0]) and GB.same_bits(da, first[1]) and GB.same_bits(sm, first[2])
    if shift == 0:  # the public wrappers take such a width as it is
        assert GB.same_bits(O.fuse_gate_fwd(s0, a0, alpha0, gamma0, m0), y)


@pytest.mark.parametrize("rows,c", [(1, 32), (65, 128), (257, 512), (300, 36)])
def test_gate_kernels_write_only_what_they_were_given(rows, c):
    s, a, dy, m, alpha, gamma = _operands(rows, c, True, 7)
    lib = _lib.load()
    # (contiguous rows: the entry points know no row stride; guard rows in front and behind)
    y, yb = GB.banded((rows, c), torch.float32, cols=0, fill=float("nan"), name="y")
    O.check(lib.cdseg_fuse_gate_fwd(O._ptr(s), O._ptr(a), O._ptr(m), O._ptr(alpha), O._ptr(gamma), O._ptr(y), rows, c, O._stream()),
            "fuse_gate_fwd")
    yb.check()
    assert GB.same_bits(y, O.fuse_gate_fwd(s, a, alpha, gamma, m))
    ds, dsb = GB.banded((rows, c), torch.float32, cols=0, fill=float("nan"), name="ds")
    da, dab = GB.banded((rows, c), torch.float32, cols=0, fill=float("nan"), name="da")
    sums, sb = GB.banded((1, 2 * c), torch.float64, rows=8, cols=0, fill=float("nan"), name="sums")
    nbytes = lib.cdseg_fuse_gate_ws_bytes(rows, c)
    assert nbytes == -(-rows // 64) * 2 * c * 8  # (rows <= 16384: 64-row blocks)
    ws, wb = GB.exact_workspace(nbytes)
    O.check(lib.cdseg_fuse_gate_bwd(O._ptr(dy), O._ptr(s), O._ptr(a), O._ptr(m), O._ptr(alpha), O._ptr(gamma), O._ptr(ds), O._ptr(da),
                                    O._ptr(sums), rows, c, O._ptr(ws), ws.numel(), O._stream()), "fuse_gate_bwd")
    for b in (dsb, dab, sb, wb):
        b.check()
    r = O.fuse_gate_bwd(dy, s, a, alpha, gamma, m)
    assert GB.same_bits(ds, r[0]) and GB.same_bits(da, r[1]) and GB.same_bits(sums.reshape(-1), r[2])
    # the stated preconditions come back as status codes, before any launch
    assert lib.cdseg_fuse_gate_bwd(O._ptr(dy), O._ptr(s), O._ptr(a), O._ptr(m), O._ptr(alpha), O._ptr(gamma), O._ptr(ds), O._ptr(da),
                                   O._ptr(sums), rows, c, O._ptr(ws), max(ws.numel() - 1, 0), O._stream()) == -3  # CDSEG_ERR_WORKSPACE
    assert lib.cdseg_fuse_gate_fwd(O._ptr(s), O._ptr(a), O._ptr(m), O._ptr(alpha), O._ptr(gamma), O._ptr(y), rows, 516, O._stream()) \
        == -4  # CDSEG_ERR_UNSUPPORTED
    for b in (yb, dsb, dab, sb, wb):
        b.check()


# ------------------------------------------------------------------------------------------ inference vs the reference
def _dev(fx):
    return {k: torch.as_tensor(v).cuda() for k, v in fixture_input(fx).items()}


def _report(name, out, ref):
    err = float(np.abs(out - ref).max())
    agree = float((out.argmax(1) == ref.argmax(1)).mean())
    print(f"[measure] {name}: max_abs_err={err:.3e} argmax_agreement={agree:.5f}")
    return err, agree


@pytest.mark.parametrize("tag", INFER_TAGS)
def test_inference_matches_the_reference_recordings(tag):
    fx = load_fixture(f"fusion_infer_{tag}.npz")
    model, cfg = infer_model(fx)
    model = model.cuda()
    model.precision = "fp32"
    inp = _dev(fx)
    ssi = model.inference(dict(inp), eval=False, draws=ssi_draws(fx))["seg_logits"]
    err, agree = _report(f"fusion {tag} fp32 vs reference", ssi.cpu().numpy(), fx["logits"])
    assert err < 1e-3 and agree > 0.999  # tests/test_gpu_e2e.py: the fp32 logit bound of the mini goldens
    msi = model.inference_ddim(dict(inp), T=cfg["T"], step=2, eval=False, mode="avg", draws=ddim_draws(fx))["seg_logits"]
    err, _ = _report(f"fusion {tag} fp32 multi-step vs reference", msi.cpu().numpy(), fx["ddim_logits"])
    assert err < 5e-5  # ... and its multi-step bound
    # the same logits, bit for bit: with a shared plan, through inference_many(batch=2), with the hoisted n-encoder
    plan = model.plan(dict(inp))
    built = model.engine().plans_built
    assert torch.equal(ssi, model.inference(dict(inp), eval=False, draws=ssi_draws(fx), plan=plan)["seg_logits"])
    assert torch.equal(msi, model.inference_ddim(dict(inp), T=cfg["T"], step=2, eval=False, mode="avg", draws=ddim_draws(fx),
                                                 plan=plan)["seg_logits"])
    assert model.engine().plans_built == built
    n0 = int(fx["offset"][0])
    n1 = int(fx["offset"][1]) - n0
    parts = [{k: (v[:n0] if k != "offset" else torch.tensor([n0], device=v.device)) for k, v in inp.items()},
             {k: (v[n0:] if k != "offset" else torch.tensor([n1], device=v.device)) for k, v in inp.items()}]
    outs = model.inference_many(parts, batch=2, draws=[ssi_draws(fx)])
    assert torch.equal(ssi, torch.cat([o["seg_logits"] for o in outs]))
    d = ddim_draws(fx)
    perms = [np.array(p) for p in d["perms"]]
    for call in (1, 2):  # draws that repeat the first call's n-branch shuffles
        for j in (1, 3, 4, 6, 7):
            perms[8 * call + j] = perms[j]
    kw = dict(T=cfg["T"], step=2, eval=False, mode="avg")
    a = model.inference_ddim(dict(inp), draws=dict(d, perms=list(perms)), **kw)["seg_logits"]
    b = model.inference_ddim(dict(inp), draws=dict(d, perms=list(perms)), reuse_encoder=True, **kw)["seg_logits"]
    assert model.engine().msi_stats["n_encoders"] == 1 and torch.equal(a, b)
    # 16-bit trunks against the fp32 HIP logits: the bounds tests/test_gpu_e2e.py uses for the mini model
    ref = ssi.cpu().numpy()
    for precision, tol, min_agree in (("fp16+head", 3e-3, 0.9965), ("bf16+head", 0.04, 0.985)):
        model.precision = precision
        model.count_saturation = precision.startswith("fp16")
        out = model.inference(dict(inp), eval=False, draws=ssi_draws(fx))["seg_logits"].cpu().numpy()
        err, agree = _report(f"fusion {tag} {precision} vs fp32", out, ref)
        assert np.isfinite(out).all() and err < tol and agree > min_agree
        if model.count_saturation:
            assert model.engine().saturation_count == 0
        model.count_saturation = False


def test_full_width_tail_kernels_carry_the_folded_gate():
    """At full width the cross blocks' proj + MLP run on the streamed-weight tail kernels (C = 512 for cross_block2, C = 128 for
    cross_block1), which the mini fixtures never reach: bidirectional + "b_channel_scale" with seeded feat_scales and the
    fixtures' gain on attn.proj, `fp16+head` with the tail images against the same engine without them (the proj GEMM + MLP path
    the recordings pin) and against fp32, within the full-size 16-bit bound of tests/test_gpu_e2e.py (6e-3); the default fusion
    on the same weights is more than 0.1 away, so a tail that ignored the gate could not pass."""
    from cdsegnet_amd import configs
    from cdsegnet_amd.param_init import fill_state_dict
    from cdsegnet_amd.registry import build_model
    fx = load_fixture("full_e2e_8k.npz")
    inp = _dev(fx)
    draws = lambda: dict(noise=torch.from_numpy(fx["noise"]), perms=[p for p in fx["perms"]])  # noqa: E731

    def make(**kw):
        model = build_model(configs.cdsegnet_config("scannet", **kw))
        sd = fill_state_dict(model.state_dict(), seed=0)
        g = torch.Generator().manual_seed(9)
        for k in sd:
            if k.endswith("feat_scale"):
                sd[k] = torch.randn(sd[k].shape, generator=g)
            elif "._tm_dec0." in k and ".attn.proj." in k:
                sd[k] = sd[k] * 16.0
        model.load_state_dict(sd, strict=True)
        return model.cuda().eval()

    def run(model, precision, strip=False):
        model.precision = precision
        eng = model.engine()
        eng.prepare(torch.device("cuda", torch.cuda.current_device()))
        tails = [k for k in eng.w if k in ("x.tail_img", "x1.tail_img")]
        if strip:
            for k in tails:
                del eng.w[k]
        out = model.inference(dict(inp), eval=False, draws=draws())["seg_logits"].cpu().numpy()
        model._drop_engine()
        return out, tails

    model = make(tm_feat="b_channel_scale", tm_bidirectional=True)
    ref, _ = run(model, "fp32")
    a, tails = run(model, "fp16+head")
    b, _ = run(model, "fp16+head", strip=True)
    assert sorted(tails) == ["x.tail_img", "x1.tail_img"]
    base, _ = run(make(), "fp32")
    e_a, _ = _report("full width fusion fp16+head (tail kernels) vs fp32", a, ref)
    e_b, _ = _report("full width fusion fp16+head (proj GEMM + MLP) vs fp32", b, ref)
    e_0, _ = _report("full width default fusion vs bidirectional + b_channel_scale", base, ref)
    assert e_a < 6e-3 and e_b < 6e-3 and e_0 > 0.1


# ------------------------------------------------------------------------------------------ training vs the reference
def _train_inp(fx):
    return {k: torch.as_tensor(fx[k]).cuda() for k in ("coord", "grid_coord", "feat", "offset", "segment")}


def _groups(model):
    named = dict(model.named_parameters())
    return [dict(params=[p for k, p in named.items() if "block" not in k], lr=0.002),
            dict(params=[p for k, p in named.items() if "block" in k], lr=0.0002)]


@pytest.mark.parametrize("train_norm", ["torch", "fused"])
@pytest.mark.parametrize("train_block", ["autograd", "native"])
def test_training_step_matches_the_reference_recording(train_block, train_norm):
    """Bidirectional + "b_channel_scale" against the reference's recorded step, with the bounds of tests/test_gpu_train.py."""
    fx = load_fixture("fusion_train_step.npz")
    model, sd = train_model(fx)
    model = model.cuda()
    model.train_block, model.train_norm = train_block, train_norm
    named = dict(model.named_parameters())
    opt = torch.optim.AdamW(_groups(model), lr=0.002, weight_decay=0.05)
    opt.zero_grad()
    out = model(_train_inp(fx), draws=train_draws(fx))
    e_loss = abs(float(out["loss"].detach()) - float(fx["loss"]))
    e_n = float((out["n_pred"].detach().cpu() - torch.as_tensor(fx["n_pred"])).abs().max())
    e_c = float((out["c_pred"].detach().cpu() - torch.as_tensor(fx["c_pred"])).abs().max())
    out["loss"].backward()
    torch.cuda.synchronize()
    names = [str(n) for n in fx["grad_names"]]
    assert names == list(named) and all(named[k].grad is not None for k in names) and len(names) == 538
    gn = np.array([float(named[k].grad.norm()) for k in names])
    ref = fx["grad_norms"]
    rel = np.abs(gn - ref) / (ref + 1e-3 * ref.max())
    worst_full, checked = 0.0, 0
    for k in fx.files:
        if k.startswith("g."):
            r = fx[k]
            assert named[k[2:]].grad.shape == r.shape
            worst_full = max(worst_full, float((named[k[2:]].grad.cpu() - torch.as_tensor(r)).abs().max()) / float(np.abs(r).max()))
            checked += 1
    print(f"[measure] fusion training step ({train_block}, {train_norm}) vs reference: loss err {e_loss:.3e}, n_pred err {e_n:.3e}, "
          f"c_pred err {e_c:.3e}, worst gradient-norm rel err over 538 parameters {rel.max():.3e}, worst of {checked} full gradients "
          f"rel {worst_full:.3e}")
    assert e_loss < 1e-4 and e_n < 1e-3 and e_c < 1e-3
    assert rel.max() < 1e-3 and checked == 12 and worst_full < 1e-3
    opt.step()
    torch.cuda.synchronize()
    worst, nchk = 0.0, 0
    for i, k in enumerate(names):
        if ref[i] < 1e-4 * ref.max():
            continue
        dn = float((named[k].detach().cpu() - sd[k].float()).norm())
        worst = max(worst, abs(dn - float(fx["step_norms"][i])) / max(float(fx["step_norms"][i]), 1e-12))
        if "p1." + k in fx.files:
            assert float((named[k].detach().cpu() - torch.as_tensor(fx["p1." + k])).abs().max()) < 5e-6
            nchk += 1
    print(f"[measure] fusion first AdamW step vs reference: worst step-norm rel err {worst:.3e} ({nchk} parameters compared in full)")
    assert worst < 2e-2 and nchk == 3


def test_training_step_amp_close_to_fp32():
    """fp16-amp against the fp32 run: the whole-step bound of tests/test_gpu_train_amp.py."""
    from tests.test_gpu_train_amp import LOSS_CAP
    fx = load_fixture("fusion_train_step.npz")
    model, _ = train_model(fx)
    model = model.cuda()
    losses, grads = {}, {}
    for tp in ("fp32", "fp16-amp"):
        model.train_precision = tp
        model.zero_grad()
        loss = model(_train_inp(fx), draws=train_draws(fx))["loss"]
        loss.backward()
        losses[tp] = float(loss.detach())
        grads[tp] = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    assert all(bool(torch.isfinite(g).all()) for g in grads["fp16-amp"].values())
    cos = min(float(torch.nn.functional.cosine_similarity(grads["fp32"][k].flatten().double(), grads["fp16-amp"][k].flatten().double(), 0))
              for k in grads["fp32"] if k.endswith("feat_scale"))
    print(f"[measure] fusion training step fp16-amp vs fp32: loss diff {abs(losses['fp16-amp'] - losses['fp32']):.3e}, "
          f"min cosine of the feat_scale gradients {cos:.5f}")
    assert abs(losses["fp16-amp"] - losses["fp32"]) < LOSS_CAP["fp16-amp"]
    assert abs(losses["fp32"] - float(fx["loss"])) < 1e-4


def _seeded_steps(fx, steps, seed=11):
    model, _ = train_model(fx)
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
    return model, opt, grads


def test_seeded_deterministic_steps_are_bit_equal():
    fx = load_fixture("fusion_train_step.npz")
    (m1, _, g1), (m2, _, g2) = _seeded_steps(fx, 2), _seeded_steps(fx, 2)
    assert all(GB.same_bits(g1[k], g2[k]) for k in g1)
    assert all(GB.same_bits(p.detach(), q.detach()) for p, q in zip(m1.parameters(), m2.parameters()))
    assert all(bool(g1[k].abs().max() > 0) for k in g1 if k.endswith("feat_scale"))  # FusedAdamW took the new parameters


def test_prepared_gate_follows_the_weights():
    """Train, infer, train on, infer again: the second logits differ from the first and equal, bit for bit, those of a freshly
    built model loaded with the same state_dict - the folded gate is rebuilt with every weight version."""
    fx = load_fixture("fusion_train_step.npz")
    model, opt, _ = _seeded_steps(fx, 3)
    inp = {k: v for k, v in _train_inp(fx).items() if k != "segment"}
    ifx = load_fixture("fusion_infer_bidir_channel_scale.npz")
    draws = lambda: dict(noise=torch.from_numpy(ifx["noise"]), perms=[p for p in ifx["perms"]])  # noqa: E731 (same scene)
    model.eval()
    model.precision = "fp32"
    first = model.inference(dict(inp), eval=False, draws=draws())["seg_logits"].clone()
    before = {k: p.detach().clone() for k, p in model.named_parameters() if k.endswith("feat_scale")}
    model.train()
    opt.zero_grad()
    torch.manual_seed(5)
    model(_train_inp(fx))["loss"].backward()
    opt.step()
    model.eval()
    after = {k: p.detach() for k, p in model.named_parameters() if k.endswith("feat_scale")}
    assert len(before) == 2 and all(not torch.equal(before[k], after[k]) for k in before)
    second = model.inference(dict(inp), eval=False, draws=draws())["seg_logits"]
    assert not torch.equal(first, second)
    fresh, _ = train_model(fx)
    fresh.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()}, strict=True)
    fresh = fresh.cuda().eval()
    fresh.precision = "fp32"
    assert torch.equal(second, fresh.inference(dict(inp), eval=False, draws=draws())["seg_logits"])


# ------------------------------------------------------------------------------------------ the default is untouched
# Library calls (functions of cdsegnet_amd.ops, by name) of a default mini model - one `inference` of tests/golden/
# mini_e2e_room.npz in the default precision and one training step of tests/golden/train_step_mini.npz - counted on the commit
# BEFORE the fusion options existed (tests/fusion_call_counter.py; the host helper det_kw, 225 calls there, is not counted).
DEFAULT_INFERENCE_CALLS = [list(x) for x in (
    ("attention", 1), ("bind_stream", 3), ("block_forward", 19), ("current_stream_id", 103), ("dt", 19),
    ("gather_pad_cast", 2), ("gemm", 22), ("is_lp", 3), ("layernorm", 3), ("mlp_fused", 1), ("mlp_fused_ok", 1),
    ("nbr_table_from_info", 1), ("record_event", 4), ("segment_max", 6), ("set_f32x3", 2), ("subm_conv3", 2),
    ("subm_conv3_ok", 2), ("unbind_stream", 1), ("wait_event", 2), ("workspace", 23),
)]
DEFAULT_TRAIN_STEP_CALLS = [list(x) for x in (
    ("attention", 22), ("attention_bwd", 22), ("child_info", 4), ("coarse_orders", 1), ("conv_wgrad", 25),
    ("current_stream_id", 446), ("dt", 498), ("encode", 1), ("encode4", 1), ("gemm", 312),
    ("grid_max", 1), ("layernorm", 68), ("layernorm_bwd", 68), ("linear_wgrad", 132), ("link_derive", 4), ("nbr_table", 1),
    ("nbr_table_from_info", 5), ("offset2batch", 1), ("pad_plan_batch", 1), ("plan_gather_grid", 1), ("pool_gather", 4),
    ("pool_levels", 1), ("record_event", 2), ("segment_max", 6), ("sort_curves", 1), ("sort_pairs", 1), ("workspace", 316),
)]


def test_default_model_makes_the_same_library_calls(monkeypatch):
    from tests.fusion_call_counter import default_model_calls
    infer, train = default_model_calls(monkeypatch.setattr)
    print("[measure] default inference calls:", infer)
    print("[measure] default training-step calls:", train)
    assert not any(n.startswith("fuse_gate") for n, _ in infer + train)
    assert infer == DEFAULT_INFERENCE_CALLS
    assert train == DEFAULT_TRAIN_STEP_CALLS
