"""GPU: the fused optimizer step (cdsegnet_amd/optim.py FusedAdamW on csrc/optim.hip), both builds of the library.

The update against an fp64 restatement, judged by what torch.optim.AdamW(foreach=True) itself loses on the same device and
inputs; the exact properties (unscale, clip, skip, run-to-run, the 16-bit copies) bit for bit; the clip norm against fp64;
the GradScaler protocol; the whole training step of tests/golden/train_step_mini.npz.

Every comparison prints its figures as a `[measure]` line before it asserts (kernel error, torch error, ratio; the bound is
2 x torch's error with a floor of one fp32 ulp).  profiles/NOTES.md, "Fused optimizer step", keeps the record: on an MI355X
the ratios are 0.69 - 1.40 for the update (worst on m, both errors below one ulp) and 1.00 for the clip norm."""
import math

import numpy as np
import pytest
import torch

from cdsegnet_amd import ops as O
from cdsegnet_amd.optim import FusedAdamW, shadow16
from tests.helpers import load_fixture
from tests.test_gpu_ops import LP, _library_variant, ops, report  # noqa: F401  (fixtures: lp="f16" -> the half build)

pytestmark = pytest.mark.gpu

LPS = pytest.mark.parametrize("lp", ["bf16", "f16"])
CHUNK = 8192  # CDSEG_OPT_CHUNK
SIZES = [1, 3, 4, 5, 255, 257, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7]
CARVED = 8     # the CHUNK + 1 tensor starts one float into a larger buffer: the scalar path, across a chunk boundary
GROUPS = [dict(lr=2e-3, weight_decay=0.05), dict(lr=2e-4, weight_decay=0.0)]  # tensor i belongs to group i % 2
BETAS, EPS = (0.9, 0.999), 1e-8
ULP = 2.0 ** -23


def _inputs(seed, p_mag=1.0, g_mag=1.0, steps=3):
    """fp32 CPU inputs: initial parameters and one gradient per tensor and step (magnitudes spread over a decade)."""
    gen = torch.Generator().manual_seed(seed)
    p0 = [torch.randn(n, generator=gen) * p_mag for n in SIZES]
    gs = [[torch.randn(n, generator=gen) * (g_mag * 10.0 ** float(torch.rand((), generator=gen))) for n in SIZES] for _ in range(steps)]
    return p0, gs


def _params(p0, carve=True, two_d=False):
    out = []
    for i, t in enumerate(p0):
        if carve and i == CARVED:
            buf = torch.zeros(t.numel() + 9, device="cuda")
            p = buf[1:1 + t.numel()]
            p.copy_(t)
            assert p.data_ptr() % 16 == 4
        else:
            p = t.cuda()
        if two_d:
            p = p.view(-1, 1)
        out.append(torch.nn.Parameter(p))
    return out


def _groups(params):
    return [dict(params=params[0::2], **GROUPS[0]), dict(params=params[1::2], **GROUPS[1])]


def _fused(params, **kw):
    return FusedAdamW(_groups(params), lr=1.0, betas=BETAS, eps=EPS, **kw)


def _set_grads(params, grads, mul=None):
    for i, (p, g) in enumerate(zip(params, grads)):
        g = g.cuda().view_as(p)
        p.grad = g if mul is None or mul[i] is None else g * mul[i]


def _state(opt, params):
    return ([p.detach().flatten() for p in params], [opt.state[p]["exp_avg"].flatten() for p in params],
            [opt.state[p]["exp_avg_sq"].flatten() for p in params])


def _oracle_step(p, g, m, v, t, lr, wd):
    """The update in fp64 on fp32 inputs (include/cdseg.h; torch.optim.AdamW's definition)."""
    m = BETAS[0] * m + (1 - BETAS[0]) * g
    v = BETAS[1] * v + (1 - BETAS[1]) * g * g
    bc1, bc2 = 1 - BETAS[0] ** t, 1 - BETAS[1] ** t
    p = p * (1 - lr * wd) - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + EPS)
    return p, m, v


def _oracle(p0, gs, scale=1.0):
    ps = [t.double().cuda() for t in p0]
    ms, vs = [torch.zeros_like(t) for t in ps], [torch.zeros_like(t) for t in ps]
    for t, grads in enumerate(gs, 1):
        for i, g in enumerate(grads):
            grp = GROUPS[i % 2]
            ps[i], ms[i], vs[i] = _oracle_step(ps[i], g.double().cuda() / scale, ms[i], vs[i], t, grp["lr"], grp["weight_decay"])
    return ps, ms, vs


def _rel(xs, refs):
    """Max-norm relative error of the concatenated tensors."""
    x, r = torch.cat([t.double().flatten() for t in xs]), torch.cat([t.flatten() for t in refs])
    return float((x - r).abs().max() / r.abs().max())


def _judge(what, mine, theirs, oracle):
    """The rule: for p, m and v the kernel's error against fp64 is at most twice torch's, with a floor of one fp32 ulp of the
    largest magnitude.  Prints every figure before it asserts."""
    rows = []
    for name, a, b, o in zip("pmv", mine, theirs, oracle):
        ea, eb = _rel(a, o), _rel(b, o)
        rows.append((name, ea, eb))
        print(f"[measure] {what} {name}: kernel {ea:.3e}, torch {eb:.3e}, ratio {ea / eb if eb else float('inf'):.2f}")
    for name, ea, eb in rows:
        assert ea <= max(2 * eb, ULP), (what, name, ea, eb)


def _torch_run(p0, gs, scale=None):
    """torch.optim.AdamW(foreach=True) on the same device and inputs; a scale is taken out the way GradScaler.unscale_ does."""
    params = _params(p0, carve=False)
    opt = torch.optim.AdamW(_groups(params), lr=1.0, betas=BETAS, eps=EPS, foreach=True)
    for grads in gs:
        _set_grads(params, grads)
        if scale is not None:
            inv = torch.full((), scale, device="cuda").double().reciprocal().float()
            torch._amp_foreach_non_finite_check_and_unscale_([p.grad for p in params], torch.zeros((), device="cuda"), inv)
        opt.step()
    return params, opt


# ------------------------------------------------------------------------------------------ the update against fp64
CASES = [("mag1", 1.0, None, 1.0), ("mag1e-6", 1e-6, None, 1.0), ("mag6e4", 6e4, None, 1.0),
         ("scale1", 1.0, 1.0, 1.0), ("scale1e-6", 1e-6, 1e-6, 1.0), ("scale6e4", 6e4, 6e4, 1.0),
         ("p0", 1.0, None, 0.0)]


@LPS
@pytest.mark.parametrize("name,g_mag,scale,p_mag", CASES, ids=[c[0] for c in CASES])
def test_update_against_fp64_is_as_good_as_torch(ops, lp, name, g_mag, scale, p_mag):
    """Ten tensors (1 .. 3 chunks + 7, one of them on the scalar path), two groups, three steps.  mag*: gradients of that
    magnitude as they are; scale*: gradients carrying that GradScaler scale, taken out inside the step; p0: from p = 0, where
    the parameters ARE the updates."""
    p0, gs = _inputs(11, p_mag=p_mag, g_mag=g_mag)
    params = _params(p0)
    opt = _fused(params)
    for grads in gs:
        _set_grads(params, grads)
        if scale is not None:
            opt.grad_scale, opt.found_inf = torch.full((), scale, device="cuda"), torch.zeros((), device="cuda")
        opt.step()
    tparams, topt = _torch_run(p0, gs, scale)
    torch.cuda.synchronize()
    assert all(float(opt.state[p]["step"]) == 3.0 for p in params)
    _judge(f"update {name} {lp}", _state(opt, params), _state(topt, tparams), _oracle(p0, gs, 1.0 if scale is None else float(np.float32(scale))))


# ------------------------------------------------------------------------------------------ exact properties
def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _run(p0, gs, mul=None, scale=None, found=None, **kw):
    params = _params(p0)
    opt = _fused(params, **kw)
    norms = []
    for grads in gs:
        _set_grads(params, grads, mul)
        if scale is not None:
            opt.grad_scale, opt.found_inf = torch.full((), scale, device="cuda"), torch.full((), found or 0.0, device="cuda")
        opt.step()
        if opt.max_grad_norm is not None:
            norms.append((opt.last_grad_norm.clone(), opt.last_clip_coef.clone()))
    return params, opt, norms


@LPS
def test_power_of_two_scale_equals_pre_divided_gradients(ops, lp):
    p0, gs = _inputs(12)
    scaled = [[g * 65536.0 for g in grads] for grads in gs]
    pa, oa, na = _run(p0, scaled, scale=65536.0, max_grad_norm=1.0)
    pb, ob, nb = _run(p0, gs, max_grad_norm=1.0)
    torch.cuda.synchronize()
    for x, y in zip(_state(oa, pa), _state(ob, pb)):
        assert _equal(x, y)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(na, nb))
    assert float(na[0][1]) < 1.0  # (the clip was active)


@LPS
def test_clipped_run_equals_pre_multiplied_gradients_and_leaves_the_rest_alone(ops, lp):
    p0, gs = _inputs(13)
    subset = [i for i in range(len(SIZES)) if i % 3 != 1]
    pa = _params(p0)
    oa = _fused(pa, max_grad_norm=0.5, clip_params=[pa[i] for i in subset])
    pb, pc = _params(p0), _params(p0)
    ob, oc = _fused(pb), _fused(pc)
    for grads in gs:
        _set_grads(pa, grads)
        oa.step()
        coef = oa.last_clip_coef.clone()
        _set_grads(pb, grads, [coef if i in subset else None for i in range(len(SIZES))])  # g * coef: one fp32 rounding
        ob.step()
        _set_grads(pc, grads)
        oc.step()
        assert 0.0 < float(coef) < 1.0
    torch.cuda.synchronize()
    for x, y in zip(_state(oa, pa), _state(ob, pb)):
        assert _equal(x, y)
    rest = [i for i in range(len(SIZES)) if i not in subset]
    for name, x, y in zip("pmv", _state(oa, pa), _state(oc, pc)):
        assert _equal([x[i] for i in rest], [y[i] for i in rest])
        if name != "p":  # (the clip did act on the subset; p itself is nearly invariant under a rescaled gradient)
            assert not any(torch.equal(x[i], y[i]) for i in subset)


@LPS
def test_found_inf_leaves_every_buffer_untouched(ops, lp):
    p0, gs = _inputs(14)
    params = _params(p0, two_d=True)
    opt = _fused(params, max_grad_norm=1.0, shadow16=lp)
    _set_grads(params, gs[0])
    opt.step()
    snap = [t.clone() for t in (opt._m, opt._v, opt._steps, opt._p16)] + [p.detach().clone() for p in params]
    _set_grads(params, gs[1])
    params[3].grad[2, 0] = float("inf")
    opt.grad_scale, opt.found_inf = torch.full((), 65536.0, device="cuda"), torch.ones((), device="cuda")
    opt.step()
    torch.cuda.synchronize()
    now = [opt._m, opt._v, opt._steps, opt._p16] + [p.detach() for p in params]
    assert all(torch.equal(a.view(torch.int16 if a.element_size() == 2 else torch.int32), b.view(torch.int16 if b.element_size() == 2 else torch.int32))
               for a, b in zip(snap, now))
    assert float(opt.last_nonfinite) == 1.0 and float(opt._steps.max()) == 1.0
    del opt.grad_scale, opt.found_inf
    _set_grads(params, gs[2])
    opt.step()  # and the optimizer goes on afterwards
    torch.cuda.synchronize()
    assert float(opt._steps.min()) == 2.0 and float(opt.last_nonfinite) == 0.0 and not torch.equal(params[3].detach(), snap[4 + 3])


@LPS
def test_two_runs_in_different_allocations_give_equal_bits(ops, lp):
    p0, gs = _inputs(15)
    pa, oa, na = _run(p0, gs, scale=1024.0, max_grad_norm=0.7)
    pad = torch.empty(12345, device="cuda")  # (moves the second run's allocations)
    pb, ob, nb = _run(p0, gs, scale=1024.0, max_grad_norm=0.7)
    torch.cuda.synchronize()
    assert {p.data_ptr() for p in pa}.isdisjoint({p.data_ptr() for p in pb}) and pad.numel()
    for x, y in zip(_state(oa, pa), _state(ob, pb)):
        assert _equal(x, y)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(na, nb))


@LPS
def test_16_bit_copies_equal_the_library_cast(ops, lp):
    """p16 == ops.cast(p) after every step, also at +-1e5 (beyond half's range: the half build saturates at 65504)."""
    p0, gs = _inputs(16)
    for t in p0:
        t[::3] = 1e5
        t[1::7] = -1e5
    params = _params(p0, two_d=True)
    opt = _fused(params, shadow16=lp)
    for k in range(3):
        assert all(torch.equal(shadow16(p, LP()), ops.cast(p.detach(), LP())) for p in params)
        _set_grads(params, gs[k])
        opt.step()
    torch.cuda.synchronize()
    for p in params:
        s = shadow16(p, LP())
        assert s is not None and s.dtype == LP() and s.shape == p.shape and torch.equal(s, ops.cast(p.detach(), LP()))
        assert bool(torch.isfinite(s.float()).all())
    big = float(shadow16(params[9], LP()).float().abs().max())
    assert big == 65504.0 if lp == "f16" else 9e4 < big < 1.1e5


@LPS
@pytest.mark.parametrize("how", ["in_place", "load_state_dict"])
def test_a_skipped_step_never_validates_a_stale_copy(ops, lp, how):
    """A weight that moved since the last step (in place: `_version` moves, shadow16() is None; or the optimizer's
    load_state_dict, which forgets every copy) followed by a step that found_inf skips on the device: afterwards the copy is
    either not handed out or equals the cast of the weight as it is now - with and without a gradient on that weight."""
    p0, gs = _inputs(18)
    params = _params(p0, two_d=True)
    opt = _fused(params, shadow16=lp)
    _set_grads(params, gs[0])
    opt.step()
    with torch.no_grad():
        for p in params:
            p.mul_(1.5)                      # (what model.load_state_dict's copy_, a clamp or an EMA swap do)
    if how == "load_state_dict":
        opt.load_state_dict(opt.state_dict())
    assert all(shadow16(p, LP()) is None for p in params)
    _set_grads(params, gs[1])
    params[2].grad = None                    # one weight without a gradient
    before = [p.detach().clone() for p in params]
    opt.grad_scale, opt.found_inf = torch.full((), 1.0, device="cuda"), torch.ones((), device="cuda")
    opt.step()
    torch.cuda.synchronize()
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, params))  # skipped
    for p in params:
        s = shadow16(p, LP())
        assert s is None or torch.equal(s, ops.cast(p.detach(), LP()))
    assert all(shadow16(p, LP()) is not None for i, p in enumerate(params))  # (and the step did make them current again)
    opt.found_inf = torch.zeros((), device="cuda")
    opt.step()                               # a step that is taken: the kernel's own copies
    torch.cuda.synchronize()
    assert all(torch.equal(shadow16(p, LP()), ops.cast(p.detach(), LP())) for p in params)
    assert not torch.equal(before[0], params[0].detach()) and torch.equal(before[2], params[2].detach())


# ------------------------------------------------------------------------------------------ the clip norm
@LPS
@pytest.mark.parametrize("scale", [1.0, 6e4])
def test_clip_norm_against_fp64(ops, lp, scale):
    """The norm of the unscaled gradients of a subset against fp64; bound: twice the error of torch's clip_grad_norm_ on the
    gradients GradScaler.unscale_ leaves, floor 2^-22 relative."""
    p0, gs = _inputs(17, g_mag=scale)
    subset = [i for i in range(len(SIZES)) if i != 4]
    params = _params(p0)
    opt = _fused(params, max_grad_norm=1.0, clip_params=[params[i] for i in subset])
    _set_grads(params, gs[0])
    opt.grad_scale, opt.found_inf = torch.full((), scale, device="cuda"), torch.zeros((), device="cuda")
    opt.step()
    s64 = float(np.float32(scale))
    want = math.sqrt(sum(float((gs[0][i].double() / s64).square().sum()) for i in subset))
    tp = _params(p0, carve=False)
    _set_grads(tp, gs[0])
    inv = torch.full((), scale, device="cuda").double().reciprocal().float()
    torch._amp_foreach_non_finite_check_and_unscale_([p.grad for p in tp], torch.zeros((), device="cuda"), inv)
    tnorm = float(torch.nn.utils.clip_grad_norm_([tp[i] for i in subset], 1.0))
    torch.cuda.synchronize()
    e_mine, e_torch = abs(float(opt.last_grad_norm) - want) / want, abs(tnorm - want) / want
    coef = float(opt.last_clip_coef)
    print(f"[measure] clip norm scale {scale:g} {lp}: kernel {e_mine:.3e}, torch {e_torch:.3e}, norm {want:.6e}, coef {coef:.6e}")
    assert e_mine <= max(2 * e_torch, 2.0 ** -22)
    assert abs(coef - 1.0 / (want + 1e-6)) <= 2.0 ** -21 * coef and float(opt.last_nonfinite) == 0.0


# ------------------------------------------------------------------------------------------ GradScaler
def _toy(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.GELU(), torch.nn.Linear(32, 4)).cuda()


@LPS
def test_grad_scaler_flow_skips_on_inf_steps_like_torch_and_unscales_once(ops, lp):
    mine, theirs = _toy(5), _toy(5)
    kw = dict(lr=2e-3, betas=BETAS, eps=EPS, weight_decay=0.05)
    opts = [FusedAdamW(mine.parameters(), **kw), torch.optim.AdamW(theirs.parameters(), foreach=True, **kw)]
    scalers = [torch.amp.GradScaler("cuda", init_scale=65536.0), torch.amp.GradScaler("cuda", init_scale=65536.0)]
    gen = torch.Generator().manual_seed(6)
    start = [p.detach().clone() for p in mine.parameters()]
    # step 1: an inf in one gradient - the step is skipped, the scale halved
    x = torch.randn(8, 16, generator=gen).cuda()
    for model, opt, sc in zip((mine, theirs), opts, scalers):
        opt.zero_grad()
        sc.scale(model(x).square().mean()).backward()
        model[0].weight.grad[1, 2] = float("inf")
        sc.step(opt)
        sc.update()
    torch.cuda.synchronize()
    assert all(torch.equal(a, p.detach()) for a, p in zip(start, mine.parameters()))
    assert scalers[0].get_scale() == scalers[1].get_scale() == 32768.0
    assert not hasattr(opts[0], "grad_scale") and all(float(v["step"]) == 0.0 for v in opts[0]._views)
    # steps 2 and 3: clean; 3 with scaler.unscale_ in front (grad_scale is None then: no second unscale)
    p64 = [p.double() for p in start]
    m64, v64 = [torch.zeros_like(p) for p in p64], [torch.zeros_like(p) for p in p64]
    for t, unscale_first in ((1, False), (2, True)):
        x = torch.randn(8, 16, generator=gen).cuda()
        scaled = []
        for model, opt, sc in zip((mine, theirs), opts, scalers):
            opt.zero_grad()
            sc.scale(model(x).square().mean()).backward()
            scaled.append([p.grad.detach().clone() for p in model.parameters()])
            if unscale_first:
                sc.unscale_(opt)
            sc.step(opt)
            sc.update()
        # the oracle follows the kernel's own trajectory: its gradients at the kernel's parameters
        for i, g in enumerate(scaled[0]):
            p64[i], m64[i], v64[i] = _oracle_step(p64[i], g.double() / 32768.0, m64[i], v64[i], t, 2e-3, 0.05)
        torch.cuda.synchronize()
        assert scalers[0].get_scale() == scalers[1].get_scale() == 32768.0
        if t == 1:  # both models were bit-equal going in: same gradients, one oracle judges both
            assert all(torch.equal(a, b) for a, b in zip(*scaled))
            _judge(f"GradScaler step {lp}", _state(opts[0], list(mine.parameters())), _state(opts[1], list(theirs.parameters())),
                   (p64, m64, v64))
    # after the second clean step the two trajectories differ by rounding only (1e-7 a step, carried through one backward);
    # a second unscale would shrink the gradient, and with it m, by a factor 32768
    for a, b in zip(_state(opts[0], list(mine.parameters())), _state(opts[1], list(theirs.parameters()))):
        for x_, y_ in zip(a, b):
            assert float((x_ - y_).abs().max()) <= 1e-4 * float(y_.abs().max())
    for a, o in zip(_state(opts[0], list(mine.parameters())), (p64, m64, v64)):
        assert _rel(a, o) < 1e-5


# ------------------------------------------------------------------------------------------ the whole step
def test_first_step_on_the_recorded_training_step(ops):
    """tests/test_gpu_train.py's check of the first AdamW step (two learning-rate groups) with FusedAdamW in torch's place:
    the same bounds against the reference's recorded step."""
    from tests.test_gpu_attention_bwd16 import _draws, _inp
    from tests.test_gpu_train import _mini_training_model
    fx = load_fixture("train_step_mini.npz")
    model, sd = _mini_training_model(fx, torch.device("cuda"))
    named = dict(model.named_parameters())
    blk = [p for k, p in named.items() if "block" in k]
    rest = [p for k, p in named.items() if "block" not in k]
    opt = FusedAdamW([dict(params=rest, lr=0.002), dict(params=blk, lr=0.0002)], lr=0.002, weight_decay=0.05)
    opt.zero_grad()
    model(_inp(fx), draws=_draws(fx))["loss"].backward()
    opt.step()
    torch.cuda.synchronize()
    names = [str(n) for n in fx["grad_names"]]
    ref = fx["grad_norms"]
    worst, nchk = 0.0, 0
    for i, k in enumerate(names):
        if ref[i] < 1e-4 * ref.max():
            continue
        dn = float((named[k].detach().cpu() - sd[k].float()).norm())
        worst = max(worst, abs(dn - float(fx["step_norms"][i])) / max(float(fx["step_norms"][i]), 1e-12))
        if "p1." + k in fx.files:
            assert float((named[k].detach().cpu() - torch.as_tensor(fx["p1." + k])).abs().max()) < 5e-6
            nchk += 1
    print(f"[measure] first FusedAdamW step vs reference: worst step-norm rel err {worst:.3e} ({nchk} parameters compared in full)")
    assert worst < 2e-2 and nchk == 2
    no_grad = [k for k, p in named.items() if p.grad is None]
    assert all(torch.equal(named[k].detach().cpu(), sd[k].float()) and named[k] not in opt.state for k in no_grad)


@pytest.mark.parametrize("tp,lp", [("fp16-amp", "f16"), ("bf16-amp", "bf16")])
def test_amp_steps_with_shadow_copies_equal_the_steps_without(ops, monkeypatch, tp, lp):
    """Three AMP steps under GradScaler with shadow16 on and off: bit-equal losses and parameters (fixed-order gradient
    reductions, so that two runs can be compared at all).  With current copies the forward casts no weight; after
    load_state_dict it casts again until the next step."""
    from tests.test_gpu_attention_bwd16 import _draws, _inp, _mini_model
    fx = load_fixture("train_step_mini.npz")
    inp = _inp(fx)
    cast = O.cast
    weights, hits = set(), []

    def counted(src, dtype):
        if src.data_ptr() in weights:
            hits.append(src.data_ptr())
        return cast(src, dtype)

    monkeypatch.setattr(O, "cast", counted)

    def forward(model):
        hits.clear()
        with torch.autocast("cuda", enabled=True):
            loss = model(inp, draws=_draws(fx))["loss"]
        return loss, len(hits)

    def train(model, opt, scaler, loss):
        opt.zero_grad()
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()

    runs = []
    for shadow in (lp, None):
        torch.manual_seed(1)
        model, _ = _mini_model(fx, torch.device("cuda"), False)
        model.train_precision, model.train_deterministic = tp, True
        weights.clear()
        weights.update(p.data_ptr() for p in model.parameters() if p.dim() >= 2)
        opt = FusedAdamW(model.parameters(), lr=0.002, weight_decay=0.05, shadow16=shadow)
        scaler = torch.amp.GradScaler("cuda")
        losses, casts = [], []
        for _ in range(3):
            loss, n = forward(model)
            train(model, opt, scaler, loss)
            losses.append(loss.detach().clone())
            casts.append(n)
        torch.cuda.synchronize()
        runs.append((losses, [p.detach().clone() for p in model.parameters()], casts, scaler.get_scale()))
        if shadow is not None:
            casts.append(forward(model)[1])           # current copies
            opt.load_state_dict(opt.state_dict())
            loss, n = forward(model)                  # forgotten: the forward casts again ...
            casts.append(n)
            train(model, opt, scaler, loss)
            casts.append(forward(model)[1])           # ... until the next step
            torch.cuda.synchronize()
    (la, pa, ca, sa), (lb, pb, cb, sb) = runs
    print(f"[measure] {tp}: weight casts per forward with shadows {ca}, without {cb}; scale {sa}; losses {[float(v) for v in la]}")
    assert cb[0] > 0 and cb == [cb[0]] * 3
    assert ca == [0, 0, 0, 0, cb[0], 0]
    assert sa == sb and all(bool(torch.isfinite(v)) for v in la)
    assert all(torch.equal(a, b) for a, b in zip(la, lb))
    assert all(torch.equal(a, b) for a, b in zip(pa, pb))
