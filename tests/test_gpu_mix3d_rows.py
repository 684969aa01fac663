"""GPU: Mix3D batches trained on every point (`DefaultSegmentorV2.train_mix3d = "rows"`; cdsegnet_amd.engine.RowLevel, the row
fields of the native Block in csrc/trainblock.hip).

In this order: (1) the four row kernels are BIT-EXACT against torch expressions; (2) one Block on a row level - the native
executor and the autograd graph - against an fp64 torch restatement written here, the bound of tests/test_gpu_train_block.py
(native <= 3 E_auto + 2^-24); (3) zeroed row fields leave the native executor what it is without them, and row fields that
describe one row per voxel give the same Block; (4) a whole "rows" step: native against autograd, and two seeded
deterministic steps bit-equal; (5) the reference's own recorded step on a merged batch, in both train_block modes.

Every figure is printed with report(...) before it is asserted.
"""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cdsegnet_amd import engine as EN
from cdsegnet_amd import ops as O
from cdsegnet_amd import train_graph as TG
from tests.helpers import load_fixture
from tests.test_gpu_ops import LP, _library_variant, dev, ops, report  # noqa: F401  (fixtures: lp="f16" -> the half build)
from tests.test_gpu_train_block import NAMES18, U, _bits, _block_params, _err, _graph, _sync

pytestmark = pytest.mark.gpu

PATCH = 128


# ------------------------------------------------------------------------------------------ (1) the row kernels, bit-exact
def _runs(lengths):
    lengths = np.asarray(lengths, dtype=np.int64)
    row_start = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    row_vox = np.repeat(np.arange(len(lengths)), lengths).astype(np.int32)
    return dev(row_vox), dev(row_start)


RUN_SHAPES = {
    "no-duplicates": [1] * 300,                                      # n_conv = n through the rows path
    "run-at-row-0": [3, 1, 1, 2] + [1] * 250,
    "run-at-the-last-row": [1] * 700 + [2, 1, 3, 1, 2],             # more than one block of 256 threads per column chunk
    "mixed": list(np.random.default_rng(5).choice([1, 1, 1, 2, 2, 3, 5], 777)),
}


@pytest.mark.parametrize("C", (16, 32, 48))
@pytest.mark.parametrize("shape", list(RUN_SHAPES))
def test_row_kernels_are_bit_equal_to_torch(ops, shape, C):
    lengths = RUN_SHAPES[shape]
    row_vox, row_start = _runs(lengths)
    nv, n = len(lengths), int(sum(lengths))
    g = torch.Generator().manual_seed(n + C)
    x = dev(torch.randn(n, C, generator=g))
    a = dev(torch.randn(nv, C, generator=g))
    first, vox = row_start[:-1].long(), row_vox.long()
    # gather_first
    assert _bits(ops.gather_first(x, row_start), x[first])
    # residual_rows, with and without the per-scene rows; in place
    offs = dev(np.array([0, n // 3, n], dtype=np.int32))
    t_rows = dev(torch.randn(2, C, generator=g))
    scene = (torch.arange(n, device="cuda") >= n // 3).long()
    assert _bits(ops.residual_rows(x, a, row_vox), x + a[vox])
    assert _bits(ops.residual_rows(x, a, row_vox, t_rows, offs), (x + a[vox]) + t_rows[scene])
    y = x.clone()
    assert _bits(ops.residual_rows(y, a, row_vox, out=y), x + a[vox])
    # run_sum: 0 + the run's rows in ascending order
    want = torch.zeros(nv, C, device="cuda")
    length = (row_start[1:] - row_start[:-1]).long()
    for k in range(int(length.max())):
        has = length > k
        want[has] = want[has] + x[first[has] + k]
    assert _bits(ops.run_sum(x, row_start), want)
    # scatter_first: a new tensor with zero rows, and accumulated
    z = torch.zeros(n, C, device="cuda")
    z[first] = a
    assert _bits(ops.scatter_first(a, row_vox, row_start), z)
    acc = x.clone()
    ops.scatter_first(a, row_vox, row_start, acc)
    want = x.clone()
    want[first] = x[first] + a
    _sync()
    assert _bits(acc, want)


@pytest.mark.parametrize("lp", ["bf16", "f16"])
def test_gather_first_casts_like_the_forward_cast(ops, lp):
    """The 16-bit variants round to nearest even and SATURATE (the conv's forward operand, like ops.cast)."""
    row_vox, row_start = _runs(RUN_SHAPES["mixed"])
    n = int(row_start[-1])
    x = dev(torch.randn(n, 32, generator=torch.Generator().manual_seed(1)) * 50.0)
    x[int(row_start[3]), :4] = torch.tensor([1e30, -1e30, 70000.0, -70000.0], device="cuda")
    got = ops.gather_first(x, row_start, lp)
    assert got.dtype == LP() and _bits(got, ops.cast(x[row_start[:-1].long()].contiguous(), LP()))
    assert bool(torch.isfinite(got.float()).all())


# ------------------------------------------------------------------------------------------ (2) one Block on a row level
_CASES = {}


def _rows_batch():
    """N = 1200 points, V = 960 voxels: element 0 holds 660 voxels of a room, 239 of them twice and one three times, in a shuffled
    caller order; element 1 (300 points) has no shared voxel."""
    from cdsegnet_amd import synth
    rng = np.random.default_rng(12)
    a = np.unique(np.asarray(synth.room_scene(31, 2500)["grid_coord"], dtype=np.int64), axis=0)
    b = np.unique(np.asarray(synth.room_scene(32, 1200)["grid_coord"], dtype=np.int64), axis=0)
    assert len(a) >= 660 and len(b) >= 300
    a, b = a[rng.permutation(len(a))[:660]], b[rng.permutation(len(b))[:300]]
    twice = a[rng.choice(660, 239, replace=False)]
    e0 = np.concatenate([a, twice, twice[:1]])
    e0 = e0[rng.permutation(len(e0))]
    grid = np.concatenate([e0, b])
    return grid, np.array([len(e0), len(grid)], dtype=np.int64)


def _rows_case(C, H, distinct, with_t):
    """The row level of `_rows_batch` from the engine's own plan builder, the inputs of one Block on it (built once, never
    modified) and the fp64 torch-autograd restatement: the CPE on the first row of every voxel, gathered to the rows."""
    key = (C, H, distinct, with_t)
    if key in _CASES:
        return _CASES[key]
    from oracle import model as OM
    from tests.test_gpu_attention_bwd16 import _mini_model
    if "plan" not in _CASES:
        grid_np, offset_np = _rows_batch()
        model, _ = _mini_model(load_fixture("train_step_mini.npz"), torch.device("cuda"), True)
        graph = TG.TrainGraph(model)
        grid, offset = dev(grid_np), dev(offset_np)
        keep, rep, offset_u = TG.voxel_representatives(grid, offset)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            plan = graph._rows_plan(grid, offset_np.tolist(), keep, rep, offset_u)
        rows = plan.rows
        n, nv = rows.n, rows.voxels.n
        assert (n, nv) == (1200, 960) and isinstance(rows, EN.RowLevel)
        row_start = rows.row_start.long().cpu().numpy()
        length = np.diff(row_start)
        assert length.max() == 3 and (length == 3).sum() == 1
        batch = rows.batch.long().cpu().numpy()
        assert (np.diff(row_start)[rows.voxels.batch.cpu().numpy() == 1] == 1).all()  # element 1: no shared voxel
        curve = 2
        gidx, widx = rows.slots(curve, PATCH, True)
        cu = rows.pad_host(PATCH, True)[3]
        order = gidx.long().cpu().numpy()
        w = widx.long().cpu().numpy()
        inverse = np.empty(n, dtype=np.int64)
        inverse[w[w >= 0]] = np.nonzero(w >= 0)[0]
        assert (order[inverse] == np.arange(n)).all() and len(cu) > 8
        # at least one voxel's run straddles a patch boundary: its rows sit in different patches
        patch_of = np.searchsorted(cu, inverse, side="right") - 1
        vox = rows.row_vox.long().cpu().numpy()
        split = [v for v in np.nonzero(length > 1)[0] if len(set(patch_of[row_start[v]:row_start[v + 1]])) > 1]
        assert split, "no voxel's run straddles a patch boundary"
        gv = rows.voxels.grid.long().cpu().numpy()
        nbr = OM.subm_neighbors(gv, rows.voxels.batch.long().cpu().numpy(), 3)
        assert (nbr[:, 13] == np.arange(nv)).all() and (nbr < 0).any()
        assert (rows.voxels.nbr(3, True).long().cpu().numpy() == nbr.T).all()
        _CASES["plan"] = dict(rows=rows, plan=plan, graph=graph, n=n, nv=nv, curve=curve, cu=np.asarray(cu), order=order, inverse=inverse,
                              nbr=nbr, batch=batch, vox=vox, first=row_start[:-1], straddling=len(split))
    pl = _CASES["plan"]
    n, B = pl["n"], 2
    rng = np.random.default_rng(C + 7 * n)
    params = _block_params(C, H, rng)
    x_in, dy = rng.standard_normal((n, C)).astype(np.float32), rng.standard_normal((n, C)).astype(np.float32)
    x_conv = rng.standard_normal((n, C)).astype(np.float32) if distinct else None
    t_rows = (0.5 * rng.standard_normal((B, C))).astype(np.float32) if with_t else None
    m1, m2 = ((rng.random(n) < 0.7).astype(np.float32) / np.float32(0.7) for _ in range(2))
    m1[0], m2[n - 1] = 0.0, 0.0
    P = [torch.as_tensor(p).double().requires_grad_(True) for p in params]
    xi = torch.as_tensor(x_in).double().requires_grad_(True)
    xc = torch.as_tensor(x_conv).double().requires_grad_(True) if distinct else xi
    tr = torch.as_tensor(t_rows).double().requires_grad_(True) if with_t else None
    ln = lambda v, i: F.layer_norm(v, (C,), P[i], P[i + 1], 1e-5)  # noqa: E731
    cpe_v = ln(F.linear(OM.subm_conv3d(xc[torch.as_tensor(pl["first"])], pl["nbr"], P[0], P[1]), P[2], P[3]), 4)
    x0 = xi + cpe_v[torch.as_tensor(pl["vox"])]
    if with_t:
        x0 = x0 + tr[torch.as_tensor(pl["batch"])]
    qkv = F.linear(ln(x0, 6), P[8], P[9])
    L3 = qkv[torch.as_tensor(pl["order"])].reshape(-1, 3, C)
    feat = OM._patch_attention(L3[:, 0], L3[:, 1], L3[:, 2], pl["cu"], H, (C // H) ** -0.5)
    a = F.linear(feat[torch.as_tensor(pl["inverse"])], P[10], P[11])
    x1 = x0 + a * torch.as_tensor(m1).double()[:, None]
    h = F.linear(F.gelu(F.linear(ln(x1, 12), P[14], P[15])), P[16], P[17])
    y = x1 + h * torch.as_tensor(m2).double()[:, None]
    (y * torch.as_tensor(dy).double()).sum().backward()
    ref = {"y": y.detach(), "dx_in": xi.grad}
    if distinct:
        ref["dx_conv"] = xc.grad
    if with_t:
        ref["dt_rows"] = tr.grad
    ref.update({k: p.grad for k, p in zip(NAMES18, P)})
    _CASES[key] = dict(pl=pl, params=params, x_in=x_in, x_conv=x_conv, t_rows=t_rows, m1=m1, m2=m2, dy=dy, ref=ref)
    return _CASES[key]


def _run_rows_block(case, C, H, tp, mode):
    from cdsegnet_amd import models
    pl = case["pl"]
    n = pl["n"]
    with_t = case["t_rows"] is not None
    blk = models.Block(C, H, patch_size=PATCH, enable_flash=True, T_dim=C if with_t else -1, drop_path=0.0).cuda()
    with torch.no_grad():
        for name, p in zip(NAMES18, case["params"]):
            dict(blk.named_parameters())[name].copy_(torch.as_tensor(p))
        if with_t:  # the timestep Linear as the identity: t_rows = t_scene exactly, and t_scene.grad = dt_rows
            blk.t_mlp.weight.copy_(torch.eye(C))
            blk.t_mlp.bias.zero_()
    x_in = torch.as_tensor(case["x_in"]).cuda().requires_grad_(True)
    x_conv = torch.as_tensor(case["x_conv"]).cuda().requires_grad_(True) if case["x_conv"] is not None else None
    t_scene = torch.as_tensor(case["t_rows"]).cuda().requires_grad_(True) if with_t else None
    st = TG._St(pl["rows"], x_in, [pl["curve"]], torch.arange(n, dtype=torch.int32).cuda())
    st.conv = x_conv
    masks = {"blk.drop_path.0": [case["m1"].copy(), case["m2"].copy()]}
    y = _graph(tp, mode)._block(st, blk, "blk", t_scene, masks).x
    y.backward(torch.as_tensor(case["dy"]).cuda())
    _sync()
    out = {"y": y.detach(), "dx_in": x_in.grad}
    if x_conv is not None:
        out["dx_conv"] = x_conv.grad
    if with_t:
        out["dt_rows"] = t_scene.grad
    named = dict(blk.named_parameters())
    out.update({k: named[k].grad for k in NAMES18})
    assert all(v is not None for v in out.values())
    return out


@pytest.mark.parametrize("tp,lp", [("fp32", "bf16"), ("fp16-amp", "f16"), ("bf16-amp", "bf16")])
@pytest.mark.parametrize("C,H,distinct,with_t", [(16, 1, False, True), (32, 2, True, False)], ids=["C16-same-t", "C32-xconv"])
def test_block_on_a_row_level_vs_fp64_within_three_times_autograd(ops, tp, lp, C, H, distinct, with_t):
    """y, the input gradients and all 18 parameter gradients of one Block whose rows are the 1200 points of 960 voxels: the
    native executor (n_conv, row_vox, row_start) and the autograd graph against the fp64 restatement; per tensor
    native <= 3 E_auto + 2^-24 (metric: max |g - g64| / max |g64|), and the autograd graph itself close to fp64."""
    case = _rows_case(C, H, distinct, with_t)
    auto = _run_rows_block(case, C, H, tp, "autograd")
    nat = _run_rows_block(case, C, H, tp, "native")
    assert set(auto) == set(nat) == set(case["ref"])
    worst, over, worst_auto = ("", 0.0), [], 0.0
    for k, g64 in case["ref"].items():
        assert nat[k].dtype == torch.float32 and nat[k].shape == auto[k].shape and bool(torch.isfinite(nat[k]).all()), k
        e, ea = _err(nat[k], g64), _err(auto[k], g64)
        worst_auto = max(worst_auto, ea)
        used = e / (3 * ea + U)
        if used > worst[1]:
            worst = (k, used)
        if e > 3 * ea + U:
            over.append((k, e, ea))
    report(f"rows Block {tp} C={C} xconv={distinct} t={with_t}", straddling_runs=case["pl"]["straddling"],
           y_err=_err(nat["y"], case["ref"]["y"]), y_E_auto=_err(auto["y"], case["ref"]["y"]),
           dx_err=_err(nat["dx_in"], case["ref"]["dx_in"]), dx_E_auto=_err(auto["dx_in"], case["ref"]["dx_in"]),
           worst_bound_used=worst[1], worst_tensor=worst[0], worst_E_auto=worst_auto)
    assert not over, over
    # the yardstick measures the same function: fp32 sums of at most 27 * C + 4 C products, 16-bit operands rounded to 2^-8
    assert worst_auto < (1e-4 if tp == "fp32" else 5e-2)
    if distinct:  # the conv's data gradient lands on the first row of a run only
        first = torch.zeros(case["pl"]["n"], dtype=torch.bool)
        first[torch.as_tensor(case["pl"]["first"])] = True
        for got in (nat, auto):
            assert not bool(got["dx_conv"].cpu()[~first].any()) and bool(got["dx_conv"].cpu()[first].any())


# ------------------------------------------------------------------------------------------ (3) zeroed row fields
def test_zeroed_row_fields_are_the_executor_without_them(ops):
    """tests/test_gpu_train_block.py's Block case (two scenes, a distinct x_conv, timestep rows, dropped rows) through the
    native executor with the three fields zero / NULL, and again with row fields that describe the SAME rows (one row per
    voxel: n_conv = n, row_vox = iota, row_start = iota): the first is today's executor launch for launch (the same code
    path as before the fields existed), the second runs the row kernels - a gather of every row, a sum over runs of one row, a
    scatter onto every row - and has to give the same y and gradients up to the order of fp32 roundings."""
    from tests.test_gpu_train_block import _case, _run_block
    case = _case(32, 2, "130+77", True, True, "dropped")
    a, _ = _run_block(case, 32, 2, "fp32", "native")
    io = O._lib.TrainBlockIO()
    assert (io.n_conv, io.row_vox, io.row_start) == (0, None, None)
    n = case["plan"]["n"]
    iota = torch.arange(n + 1, dtype=torch.int32).cuda()
    fwd, bwd = O.train_block_forward, O.train_block_backward
    seen = []
    try:
        O.train_block_forward = lambda *a_, **k: (seen.append("f"), fwd(*a_, rows=(iota[:n], iota)))[1]
        O.train_block_backward = lambda *a_, **k: (seen.append("b"), bwd(*a_, rows=(iota[:n], iota)))[1]
        b, _ = _run_block(case, 32, 2, "fp32", "native")
    finally:
        O.train_block_forward, O.train_block_backward = fwd, bwd
    assert seen == ["f", "b"] and set(a) == set(b)
    c, _ = _run_block(case, 32, 2, "fp32", "native")
    worst = 0.0
    for k in a:
        if k in ("y", "dx_in", "dx_conv", "dt_rows"):  # order-fixed in the default mode (the parameter gradients use atomics)
            assert _bits(a[k], c[k]), k
        worst = max(worst, _err(b[k], a[k].double()))
    report("zeroed row fields vs one-row runs", worst_rel_diff=worst)
    # the same fp32 sums; what may differ is the order of the weight gradients' atomics and whether x_in is added inside the
    # LayerNorm kernel or behind it: a few units of 2^-24 on the largest value, never a structural difference (which is O(1))
    assert worst < 1e-5


# ------------------------------------------------------------------------------------------ (4) whole steps
_STEP = {}


def _mix3d_batch():
    """Three rooms of the recorded mini model's input format: a and b merged into element 0 (Mix3D), c on its own."""
    if not _STEP:
        from cdsegnet_amd import synth
        a, b, c = (synth.room_scene(s, 1500) for s in (41, 42, 43))
        cat = lambda k: np.concatenate([a[k], b[k], c[k]])  # noqa: E731
        na, nb, nc = (len(s["coord"]) for s in (a, b, c))
        inp = {k: torch.as_tensor(cat(k)).cuda() for k in ("coord", "grid_coord", "feat")}
        inp["segment"] = (torch.as_tensor(cat("segment").astype(np.int64)) % 13).cuda()
        inp["offset"] = torch.as_tensor(np.array([na + nb, na + nb + nc])).cuda()
        n = na + nb + nc
        g = torch.Generator().manual_seed(22)
        draws = dict(ts=torch.randint(0, 1000, (2, 1), generator=g), noise=torch.randn(n, 6, generator=g),
                     perms=[torch.randperm(4, generator=g).tolist() for _ in range(8)])
        _STEP.update(inp=inp, draws=draws, n=n)
    return _STEP["inp"], dict(_STEP["draws"]), _STEP["n"]


@pytest.mark.parametrize("tp,lp", [("fp32", "bf16"), ("fp16-amp", "f16")])
def test_rows_step_native_vs_autograd(ops, tp, lp):
    """A whole "rows" step on a Mix3D batch, seeded draws: the native mode against the autograd mode by the metric and bound of
    tests/test_gpu_train_block.py's two-room step (per tensor max |a - b| / (max |a| + 1e-3 top) < 1e-3)."""
    from tests.test_gpu_deterministic import _model, _step
    inp, draws, n = _mix3d_batch()
    model = _model(tp, False)
    model.train_mix3d = "rows"
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}

    def run(mode):
        model.load_state_dict(state)
        model.train_block = mode
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return _step(model, inp, draws)

    l0, g0 = run("autograd")
    n_rows, n_vox = model._train_graph.last_shared
    l1, g1 = run("native")
    assert (n_rows, n_vox) == model._train_graph.last_shared and n_rows == n and n_vox < n
    assert bool(torch.isfinite(l1)) and set(g0) == set(g1) and len(g0) > 400
    top = max(float(g.abs().max()) for g in g0.values())
    per = {k: float((g0[k] - g1[k]).abs().max()) / (float(g0[k].abs().max()) + 1e-3 * top) for k in g0}
    worst = max(per, key=per.get)
    report(f"rows step {tp}: native vs autograd", N=n_rows, V=n_vox, loss_autograd=float(l0), loss_native=float(l1),
           loss_rel_diff=abs(float(l0) - float(l1)) / abs(float(l0)), worst_rel_diff=per[worst], worst_tensor=worst)
    assert all(bool(torch.isfinite(g).all()) for g in g1.values())
    assert per[worst] < 1e-3
    assert abs(float(l0) - float(l1)) <= 1e-3 * abs(float(l0))


@pytest.mark.parametrize("mode", ["autograd", "native"])
def test_rows_steps_are_bit_reproducible(ops, mode):
    """train_deterministic = True: two seeded "rows" steps (forward, backward, fused AdamW), twice - bit-equal losses,
    gradients and parameters."""
    from cdsegnet_amd.optim import FusedAdamW
    from tests.test_gpu_deterministic import _model
    inp, _, n = _mix3d_batch()

    def two_steps():
        model = _model("fp32", True)
        model.train_mix3d, model.train_block = "rows", mode
        opt = FusedAdamW(model.parameters(), lr=0.002, weight_decay=0.05)
        torch.manual_seed(991)
        losses = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for _ in range(2):
                opt.zero_grad(set_to_none=True)
                loss = model(inp)["loss"]
                loss.backward()
                grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
                opt.step()
                losses.append(loss.detach().clone())
        _sync()
        assert model._train_graph.last_shared[1] < model._train_graph.last_shared[0] == n
        return losses, grads, {k: v.detach().clone() for k, v in model.state_dict().items()}

    (la, ga, sa), (lb, gb, sb) = two_steps(), two_steps()
    assert all(bool(torch.isfinite(x)) for x in la) and all(torch.equal(x, y) for x, y in zip(la, lb))
    assert set(ga) == set(gb) and len(ga) > 400
    diff = [k for k in ga if not torch.equal(ga[k], gb[k])] + [k for k in sa if not torch.equal(sa[k], sb[k])]
    report(f"rows deterministic {mode}", loss0=float(la[0]), loss1=float(la[1]), tensors_differing=len(diff))
    assert not diff, diff[:8]


# ------------------------------------------------------------------------------------------ (5) the reference's recorded step
@pytest.mark.parametrize("mode", ["autograd", "native"])
def test_recorded_mix3d_step_meets_the_reference_bound(ops, monkeypatch, mode):
    """tests/test_gpu_train.py's comparison against a recorded reference step, run as it is (the same assertions and bounds:
    loss, both predictions, 508 gradient norms, eight gradients in full, the first AdamW step) on
    tests/golden/train_step_mix3d.npz - the reference's step on a batch whose element 0 is two merged rooms (2140 points,
    17 % of element 0's rows in shared voxels, some voxels with three rows, element 0 across two 1024-slot patches) - with
    train_mix3d = "rows", in both train_block modes."""
    from tests import test_gpu_train as T
    build, load = T._mini_training_model, T.load_fixture
    calls = {"fwd": 0, "rows": 0}
    fwd = O.train_block_forward

    def rows_model(fx, dev_):
        model, sd = build(fx, dev_)
        model.train_mix3d, model.train_block = "rows", mode
        return model, sd

    def counted(*a, **k):
        calls["fwd"] += 1
        calls["rows"] += "rows" in k
        return fwd(*a, **k)

    monkeypatch.setattr(T, "_mini_training_model", rows_model)
    monkeypatch.setattr(T, "load_fixture", lambda name: load("train_step_mix3d.npz"))
    monkeypatch.setattr(O, "train_block_forward", counted)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        T.test_whole_training_step_matches_the_reference_train_step()
    if mode == "native":  # every Block went through the executor, the four level-0 Blocks with the row fields
        assert calls["fwd"] > 4 and calls["rows"] == 4, calls
    else:
        assert calls["fwd"] == 0
