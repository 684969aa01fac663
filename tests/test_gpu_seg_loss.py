"""GPU: the fused segmentation loss (csrc/loss.hip: cross entropy + multi-class Lovasz-Softmax, forward and backward;
ops.seg_loss / ops.seg_loss_bwd, losses.FusedCriteria, `model.train_loss = "fused"`), in both builds of the library.

The yardstick is an fp64 oracle of the definition in include/cdseg.h, written out below with a STABLE descending sort (ties by
ascending row index).  Accuracy is measured against the project's own torch criteria: E_ref = the error of that fp32 path
against the oracle on the same input and device, and the kernels must stay within 2 * E_ref + 2^-24 * max|reference| on CE,
Lovasz and dlogits under each upstream scalar.  Every figure is printed as a [measure] line before it is asserted;
profiles/NOTES.md ("Fused segmentation loss") keeps the worst ratios.
"""
import numpy as np
import pytest
import torch

from tests.helpers import load_fixture

pytestmark = pytest.mark.gpu

IGNORE = -1
BUILDS = pytest.mark.parametrize("lp", ["bf16", "f16"])


@pytest.fixture(autouse=True)
def _library_variant(request):
    """lp="f16" runs against the IEEE-half build of the library (the loss kernels are fp32 / fp64 in both)."""
    from cdsegnet_amd import _lib
    params = getattr(getattr(request.node, "callspec", None), "params", {})
    with _lib.use("f16" if params.get("lp") == "f16" else "bf16"):
        yield


# ------------------------------------------------------------------------------------------ the oracle
def oracle(logits, labels, ignore=IGNORE, p_fp32=False):
    """fp64, on the CPU: dict(ce, lovasz, d_ce, d_lovasz, coef) of the definition: valid rows label != ignore, p = softmax,
    CE = -mean log p[i, y_i]; per present class err = |fg - p[:, c]| sorted descending with ties by ascending row
    (torch.sort(stable=True, descending=True)), jac_k = 1 - (T - F_k) / (T + B_k), d = first differences, L_c = sum err d,
    Lovasz = mean L_c; coef = -+ d / P, d_ce = (p - onehot) / n_valid, d_lovasz = p (coef - sum_k coef p).
    p_fp32: the errors are taken from p rounded to fp32 (the definition's p is an fp32 value: what decides a TIE is equality
    of fp32 numbers); CE and the softmax factor of the gradients keep the unrounded p."""
    x = torch.as_tensor(logits).detach().cpu().double()
    y = torch.as_tensor(labels).detach().cpu().long()
    n, c = x.shape
    p = torch.softmax(x, 1)
    p_err = p.float().double() if p_fp32 else p
    valid = y != ignore
    idx = torch.nonzero(valid).flatten()
    nv = int(valid.sum())
    yv = y[idx]
    ce = -torch.log(p[idx, yv]).sum() / nv
    d_ce = torch.zeros_like(p)
    d_ce[idx] = p[idx] / nv
    d_ce[idx, yv] -= 1.0 / nv
    present = torch.unique(yv).tolist()
    coef = torch.zeros_like(p)
    terms = []
    for cls in present:
        fg = (yv == cls).double()
        err = (fg - p_err[idx, cls]).abs()
        err_s, order = torch.sort(err, stable=True, descending=True)
        fg_s = fg[order]
        total = fg_s.sum()
        jac = 1.0 - (total - fg_s.cumsum(0)) / (total + (1.0 - fg_s).cumsum(0))
        d = torch.cat([jac[:1], jac[1:] - jac[:-1]])
        terms.append((err_s * d).sum())
        coef[idx[order], cls] = torch.where(fg_s > 0, -d, d) / len(present)
    lov = torch.stack(terms).mean()
    d_lov = p * (coef - (coef * p).sum(1, keepdim=True))
    d_lov[~valid] = 0.0
    return dict(ce=ce, lovasz=lov, d_ce=d_ce, d_lovasz=d_lov, coef=coef, present=present, n_valid=nv)


# ------------------------------------------------------------------------------------------ inputs
NS, CS = (1, 63, 65, 1000, 4099), (13, 16, 20, 200)
VARIANTS = ("ignore7", "half", "single", "lone", "strided")
SHAPES = [(n, c, v) for n in NS for c in CS for v in VARIANTS]


def make_case(n, c, variant):
    """logits (N, C) fp32 and labels int64 on the CPU.  ignore7: every seventh row ignored; half: labels from every other class
    only (absent classes) + ignored rows; single: one present class; lone: one class holds exactly one row; strided: the
    logits are a column window of a wider tensor (row stride C + 9)."""
    g = torch.Generator().manual_seed(1000 * n + 10 * c + VARIANTS.index(variant))
    logits = torch.randn(n, c, generator=g) * 2.0
    labels = torch.randint(0, c, (n,), generator=g)
    rows = torch.arange(n)
    if variant in ("ignore7", "half", "strided"):
        if variant == "half":
            labels = (labels // 2) * 2
        labels[rows % 7 == 3] = IGNORE
    elif variant == "single":
        labels[:] = c - 2
    elif variant == "lone":
        labels = torch.where(labels == 5, labels + 1, labels)
        labels[n // 2] = 5
    if variant == "strided":
        wide = torch.randn(n, c + 9, generator=g)
        wide[:, 3:3 + c] = logits
        return wide, labels, (3, 3 + c)
    return logits, labels, None


_REF = {}


def reference(n, c, variant):
    """The oracle and the torch criteria's fp32 results on the device for one case - computed once, shared by the builds."""
    key = (n, c, variant)
    if key not in _REF:
        from cdsegnet_amd.losses import CrossEntropyLoss, LovaszLoss
        t, labels, win = make_case(n, c, variant)
        logits = t if win is None else t[:, win[0]:win[1]]
        o = oracle(logits, labels)
        x = logits.cuda().contiguous().requires_grad_(True)
        point = dict(n_pred=x, n_target=labels.cuda())
        ce_t = CrossEntropyLoss(ignore_index=IGNORE)(point)
        lv_t = LovaszLoss("multiclass", ignore_index=IGNORE)(point)
        g_ce, = torch.autograd.grad(ce_t, x, retain_graph=True)
        g_lv, = torch.autograd.grad(lv_t, x)
        tor = dict(ce=ce_t.detach().double().cpu(), lovasz=lv_t.detach().double().cpu(), d_ce=g_ce.double().cpu(),
                   d_lovasz=g_lv.double().cpu())
        _REF[key] = (t, labels, win, o, tor)
    return _REF[key]


def fused(ops, t, labels, win, g=(1.0, 1.0)):
    dev_t = t.cuda()
    logits = dev_t if win is None else dev_t[:, win[0]:win[1]]
    ce, lv, saved = ops.seg_loss(logits, labels.cuda(), IGNORE)
    one = lambda v: torch.tensor(v, dtype=torch.float32, device="cuda")  # noqa: E731
    d_ce = ops.seg_loss_bwd(logits, saved, one(g[0]), None)
    d_lv = ops.seg_loss_bwd(logits, saved, None, one(g[1]))
    torch.cuda.synchronize()
    return dict(ce=ce.double().cpu(), lovasz=lv.double().cpu(), d_ce=d_ce.double().cpu(), d_lovasz=d_lv.double().cpu()), saved


@pytest.fixture(scope="module")
def ops():
    from cdsegnet_amd import ops as _ops
    assert torch.cuda.is_available()
    return _ops


# ------------------------------------------------------------------------------------------ accuracy
@BUILDS
@pytest.mark.parametrize("n,c,variant", SHAPES, ids=[f"{n}x{c}-{v}" for n, c, v in SHAPES])
def test_fused_loss_is_as_accurate_as_the_torch_criteria(ops, lp, n, c, variant):
    """kernel error <= 2 * E_ref + 2^-24 * max|reference| for CE, Lovasz and dlogits under each upstream scalar, E_ref = the
    error of cdsegnet_amd/losses.py's torch criteria (fp32, same device, same input) against the fp64 oracle."""
    t, labels, win, o, tor = reference(n, c, variant)
    with ops.record_routes() as rr:
        got, saved = fused(ops, t, labels, win)
    assert saved["n_valid"] == o["n_valid"] and saved["present"] == len(o["present"])
    # the launch record: 16 lanes a row up to 32 classes (one or two classes a lane), 64 lanes with four classes each at 200
    arm = {13: "16,1", 16: "16,1", 20: "16,2", 200: "64,4"}[c]
    assert rr.kernels() == [f"loss_rows_kernel<{arm}>", f"loss_bwd_kernel<{arm}>", f"loss_bwd_kernel<{arm}>"], rr.routes
    worst = 0.0
    for k in ("ce", "lovasz", "d_ce", "d_lovasz"):
        top = float(o[k].abs().max())
        e_ref = float((tor[k] - o[k]).abs().max())
        e_ker = float((got[k] - o[k]).abs().max())
        bound = 2.0 * e_ref + 2.0 ** -24 * top
        ratio = e_ker / bound if bound > 0 else (0.0 if e_ker == 0 else float("inf"))
        worst = max(worst, ratio)
        print(f"[measure] seg_loss {lp} N={n} C={c} {variant} {k}: kernel err {e_ker:.3e}, torch err E_ref {e_ref:.3e}, "
              f"max|ref| {top:.3e}, err / bound {ratio:.3f}")
        assert e_ker <= bound, (k, e_ker, e_ref, top)
    print(f"[measure] seg_loss {lp} N={n} C={c} {variant}: worst err / bound {worst:.3f}")
    if variant in ("ignore7", "half", "strided"):  # ignored rows: exact zeros
        dead = labels == IGNORE
        assert float(got["d_ce"][dead].abs().max() if dead.any() else 0.0) == 0.0
        assert float(got["d_lovasz"][dead].abs().max() if dead.any() else 0.0) == 0.0


@BUILDS
def test_upstream_scalars_scale_the_gradient(ops, lp):
    """dlogits = g_ce * dCE + g_lovasz * dLovasz in ONE launch, g_* read on the device."""
    t, labels, win, o, _ = reference(1000, 20, "ignore7")
    logits = t.cuda()
    ce, lv, saved = ops.seg_loss(logits, labels.cuda(), IGNORE)
    g = ops.seg_loss_bwd(logits, saved, torch.tensor(0.75, device="cuda"), torch.tensor(-2.5, device="cuda")).double().cpu()
    want = 0.75 * o["d_ce"] + (-2.5) * o["d_lovasz"]
    err = float((g - want).abs().max()) / float(want.abs().max())
    print(f"[measure] seg_loss_bwd {lp} both upstream scalars: rel err {err:.3e}")
    assert err < 1e-6


# ------------------------------------------------------------------------------------------ the tie rule
def _tie_check(ops, name, logits, labels, lp):
    o = oracle(logits, labels, p_fp32=True)
    got, saved = fused(ops, logits, labels, None)
    coef = torch.zeros_like(o["coef"])
    coef[:, o["present"]] = saved["coef"].double().cpu()
    coef[labels == IGNORE] = 0.0
    out = {}
    for k, a, b in (("ce", got["ce"], o["ce"]), ("lovasz", got["lovasz"], o["lovasz"]), ("coef", coef, o["coef"]),
                    ("d_ce", got["d_ce"], o["d_ce"]), ("d_lovasz", got["d_lovasz"], o["d_lovasz"])):
        # relative to the reference's maximum, but not below fp32's smallest normal number: the results are fp32, and a saturated
        # softmax has an fp64 gradient of 1e-72 that is 0 in fp32
        top = max(float(b.abs().max()), 2.0 ** -126)
        out[k] = float((a - b).abs().max()) / top
        print(f"[measure] seg_loss {lp} tie rule, {name} {k}: rel err vs the stable-order oracle {out[k]:.3e} (max|ref| {top:.3e})")
        assert out[k] <= 1e-6, (k, out[k])
    return o, got


@BUILDS
def test_ties_break_by_ascending_row_index_all_errors_equal(ops, lp):
    """37 rows, C = 2, logits all zero, labels alternating: every p is exactly 0.5 in fp32 and fp64, every error ties, the
    loss is exactly 0.5, and the gradient depends on the tie order alone.  The yardstick is the stable-order oracle, NOT the
    torch path (torch's unstable sort lands elsewhere: 0.0089 away on a gradient whose maximum is 0.013, measured on a CPU)."""
    logits = torch.zeros(37, 2)
    labels = torch.arange(37) % 2
    o, got = _tie_check(ops, "all-equal", logits, labels, lp)
    assert abs(float(o["lovasz"]) - 0.5) < 1e-15 and float(got["lovasz"]) == 0.5
    assert float(o["d_lovasz"].abs().max()) > 1e-3  # (the rule is observable here)


@BUILDS
def test_ties_break_by_ascending_row_index_saturated_and_duplicated_rows(ops, lp):
    """Saturated logits (+80 on one column, -80 elsewhere: p is exactly 1 / 0 as an fp32 value) on 300 rows, every row present
    several times with different labels: foreground and background rows tie at errors 0 and 1.  A saturated softmax has a
    zero gradient, so the order is checked on coef (the scatter of the Jaccard differences) as well.  Then the same with
    small integer logits on duplicated rows (equal rows give equal p, bit for bit; p is not saturated, so dlogits shows
    the order too)."""
    g = torch.Generator().manual_seed(5)
    c = 5
    hot = torch.randint(0, c, (60,), generator=g).repeat(5)
    logits = torch.full((300, c), -80.0)
    logits[torch.arange(300), hot] = 80.0
    labels = torch.randint(0, c, (300,), generator=g)
    labels[::11] = IGNORE
    _tie_check(ops, "saturated", logits, labels, lp)
    base = torch.randint(0, 2, (40, c), generator=g).float()
    logits = base.repeat(6, 1)
    labels = torch.randint(0, c, (240,), generator=g)
    labels[::13] = IGNORE
    o, _ = _tie_check(ops, "duplicated", logits, labels, lp)
    assert float(o["d_lovasz"].abs().max()) > 1e-4


# ------------------------------------------------------------------------------------------ bit reproducibility
@BUILDS
def test_four_calls_give_the_same_bits(ops, lp):
    t, labels, win, _, _ = reference(4099, 200, "ignore7")
    runs = []
    for _ in range(4):
        logits = t.cuda()
        ce, lv, saved = ops.seg_loss(logits, labels.cuda(), IGNORE)
        g = ops.seg_loss_bwd(logits, saved, torch.tensor(1.0, device="cuda"), torch.tensor(1.0, device="cuda"))
        runs.append((ce.clone(), lv.clone(), g))
    torch.cuda.synchronize()
    for ce, lv, g in runs[1:]:
        assert torch.equal(ce, runs[0][0]) and torch.equal(lv, runs[0][1]) and torch.equal(g, runs[0][2])
    assert bool(torch.isfinite(runs[0][2]).all())


def test_labels_outside_the_classes_raise(ops):
    from cdsegnet_amd import _lib
    with pytest.raises(_lib.CdsegError, match="outside"):
        ops.seg_loss(torch.zeros(8, 4, device="cuda"), torch.tensor([0, 1, 2, 3, 4, -1, 0, 1], device="cuda"), IGNORE)


# ------------------------------------------------------------------------------------------ routing
def _count_calls(monkeypatch):
    """Wraps the fused path's two ops; returns the counters dict(plan=[...], loss=[...], bwd=[...]): FusedCriteria falls back
    to torch silently by design, so a test of the fused path has to see that the kernels were reached."""
    from cdsegnet_amd import ops as O
    calls = dict(plan=[], loss=[], bwd=[])
    for key, name in (("plan", "seg_loss_plan"), ("loss", "seg_loss"), ("bwd", "seg_loss_bwd")):
        real = getattr(O, name)
        monkeypatch.setattr(O, name, lambda *a, _real=real, _key=key, **k: calls[_key].append(1) or _real(*a, **k))
    return calls


def _cfg(ce=None, lv=None):
    return [dict(type="MSELoss", loss_weight=1.0, ignore_index=-1, batch_sample_point=-1),
            dict(dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1), **(ce or {})),
            dict(dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1), **(lv or {}))]


def _criteria_point(labels_all_ignored=False):
    fx = load_fixture("train_step_mini.npz")
    seg = torch.as_tensor(fx["segment"]).cuda()
    if labels_all_ignored:
        seg = torch.full_like(seg, -1)
    mk = lambda k: torch.as_tensor(fx[k]).cuda().requires_grad_(True)  # noqa: E731
    return dict(n_pred=mk("n_pred"), c_pred=mk("c_pred"), c_target=torch.as_tensor(fx["noise"]).cuda(), n_target=seg,
                offset=torch.as_tensor(fx["offset"]).cuda(), loss_mode="train")


ROUTED = {"weighted-ce": (dict(weight="per class"), None, False),
          "label-smoothing": (dict(label_smoothing=0.1), None, False),
          "ignore-mismatch": (None, dict(ignore_index=-2), False),
          "all-ignored": (None, None, True)}


@pytest.mark.parametrize("name", list(ROUTED))
@pytest.mark.parametrize("loss_type", ["EW", "GLS"])
def test_unfusable_configurations_take_the_torch_path_bit_for_bit(ops, monkeypatch, name, loss_type):
    from cdsegnet_amd.losses import Criteria, FusedCriteria, build_criteria
    ce, lv, dead = ROUTED[name]
    cfg = _cfg(ce, lv)
    if ce and "weight" in ce:
        cfg[1]["weight"] = [1.0 + 0.1 * i for i in range(_criteria_point()["n_pred"].shape[1])]
    calls = _count_calls(monkeypatch)
    res = []
    for mode in ("torch", "fused"):
        crit = build_criteria(cfg, loss_type, 2, mode)
        assert type(crit) is (FusedCriteria if mode == "fused" else Criteria)
        point = _criteria_point(dead)
        loss = crit(point)
        loss.backward()
        res.append((loss.detach(), point["n_pred"].grad, point["c_pred"].grad))
    # (the empty batch is found by the histogram read, the others before any launch; phase 1 and the backward never run)
    assert len(calls["plan"]) == (1 if dead else 0) and not calls["loss"] and not calls["bwd"]
    for a, b in zip(*res):
        assert torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0))  # (the empty batch: torch's nan stands)


@pytest.mark.parametrize("loss_type", ["EW", "GLS"])
def test_fused_criteria_match_the_torch_criteria_and_use_the_kernels(ops, monkeypatch, loss_type):
    """The shipped triple on the reference's recorded predictions: the fused path is taken (ops.seg_loss and ops.seg_loss_bwd are reached), loss and
    d loss / d prediction agree with the torch path to fp32 rounding; eval mode under no_grad as well."""
    from cdsegnet_amd.losses import build_criteria
    calls = _count_calls(monkeypatch)
    res = []
    for mode in ("torch", "fused"):
        crit = build_criteria(_cfg(), loss_type, 2, mode)
        point = _criteria_point()
        loss = crit(point)
        loss.backward()
        with torch.no_grad():
            ev = crit(dict(n_pred=point["n_pred"].detach(), n_target=point["n_target"], loss_mode="eval"))
        res.append((loss.detach().double(), point["n_pred"].grad.double(), point["c_pred"].grad.double(), ev.double()))
    assert len(calls["plan"]) == 2 and len(calls["loss"]) == 2 and len(calls["bwd"]) == 1  # (train + eval; one backward)
    (l0, gn0, gc0, e0), (l1, gn1, gc1, e1) = res
    e_l, e_e = abs(float(l1 - l0)), abs(float(e1 - e0))
    e_n = float((gn1 - gn0).abs().max()) / float(gn0.abs().max())
    e_c = float((gc1 - gc0).abs().max()) / float(gc0.abs().max())
    print(f"[measure] fused vs torch criteria, {loss_type}: loss diff {e_l:.3e}, eval loss diff {e_e:.3e}, d n_pred rel {e_n:.3e}, "
          f"d c_pred rel {e_c:.3e}")
    assert e_l < 1e-6 and e_e < 1e-6 and e_n < 1e-5 and e_c < 1e-5


# ------------------------------------------------------------------------------------------ the whole step
def _mini(loss_type=None):
    from tests.test_gpu_train import _mini_training_model
    fx = load_fixture("train_step_mini.npz")
    model, sd = _mini_training_model(fx, torch.device("cuda"))
    if loss_type is not None:
        model.loss_type = loss_type
    masks = {str(k): [fx[f"mask.{i}.{j}"] for j in range(int(fx["mask_counts"][i]))] for i, k in enumerate(fx["mask_names"])}
    draws = dict(ts=fx["ts"], noise=fx["noise"], perms=[list(p) for p in fx["perms"]], masks=masks)
    inp = {k: torch.as_tensor(fx[k]).to("cuda") for k in ("coord", "grid_coord", "feat", "offset", "segment")}
    return fx, model, draws, inp


@pytest.mark.parametrize("loss_type", ["EW", "GLS"])
def test_fused_step_loss_is_within_1e6_of_the_torch_step(monkeypatch, loss_type):
    fx, model, draws, inp = _mini(loss_type)
    calls = _count_calls(monkeypatch)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    losses = {}
    for mode in ("torch", "fused"):
        model.load_state_dict(state)
        model.train()
        model.train_loss = mode
        losses[mode] = float(model(inp, draws=dict(draws))["loss"].detach().double())
    diff = abs(losses["fused"] - losses["torch"])
    print(f"[measure] whole step {loss_type}: torch loss {losses['torch']:.9f}, fused loss {losses['fused']:.9f}, diff {diff:.3e}")
    assert len(calls["loss"]) == 1  # (the fused step did run the kernels, the torch step did not)
    assert diff < 1e-6


def test_whole_training_step_with_the_fused_loss_matches_the_reference_train_step(monkeypatch):
    """tests/test_gpu_train.py's comparison with the reference's recorded step, `train_loss = "fused"`, the same bounds: loss
    within 1e-4, the norm of every one of the 508 parameter gradients within 1e-3 relative."""
    fx, model, draws, inp = _mini()
    calls = _count_calls(monkeypatch)
    model.train_loss = "fused"
    named = dict(model.named_parameters())
    out = model(inp, draws=draws)
    e_loss = abs(float(out["loss"].detach()) - float(fx["loss"]))
    out["loss"].backward()
    torch.cuda.synchronize()
    names = [str(n) for n in fx["grad_names"]]
    assert all(named[k].grad is not None for k in names) and len(names) == 508
    gn = np.array([float(named[k].grad.norm()) for k in names])
    ref = fx["grad_norms"]
    rel = np.abs(gn - ref) / (ref + 1e-3 * ref.max())
    print(f"[measure] whole training step, fused loss, vs reference: loss err {e_loss:.3e}, worst gradient-norm rel err over 508 "
          f"parameters {rel.max():.3e}")
    assert len(calls["loss"]) == 1 and len(calls["bwd"]) == 1
    assert e_loss < 1e-4 and rel.max() < 1e-3


def test_two_seeded_deterministic_steps_with_the_fused_loss_are_bit_equal(monkeypatch):
    fx, model, draws, inp = _mini()
    calls = _count_calls(monkeypatch)
    model.train_loss, model.train_deterministic = "fused", True
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    runs = []
    for _ in range(2):
        model.load_state_dict(state)
        model.train()
        model.train_loss, model.train_deterministic = "fused", True
        model.zero_grad(set_to_none=True)
        torch.manual_seed(3)
        out = model(inp, draws=dict(draws))
        out["loss"].backward()
        torch.cuda.synchronize()
        runs.append((out["loss"].detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters()
                                                     if p.grad is not None}))
    (l1, g1), (l2, g2) = runs
    assert len(calls["loss"]) == 2 and len(calls["bwd"]) == 2
    assert bool(torch.isfinite(l1)) and torch.equal(l1, l2)
    diff = [k for k in g1 if not torch.equal(g1[k], g2[k])]
    assert len(g1) > 400 and set(g1) == set(g2) and not diff, diff[:8]


def test_inference_eval_loss_follows_the_switch(ops, monkeypatch):
    fx, model, draws, inp = _mini()
    calls = _count_calls(monkeypatch)
    model.eval()
    out = {}
    for mode in ("torch", "fused"):
        model.train_loss = mode
        torch.manual_seed(2)
        out[mode] = float(model.inference(dict(inp), eval=True)["loss"])
    assert len(calls["plan"]) == 1 and len(calls["loss"]) == 1 and not calls["bwd"]
    print(f"[measure] inference(eval=True) loss: torch {out['torch']:.9f}, fused {out['fused']:.9f}")
    assert abs(out["fused"] - out["torch"]) < 1e-5 * max(1.0, abs(out["torch"]))
    model.train_loss = "hip"
    with pytest.raises(ValueError, match="train_loss"):
        model.inference(dict(inp), eval=True)
    model.train()
    with pytest.raises(ValueError, match="train_loss"):
        model(inp, draws=draws)
