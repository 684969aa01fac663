"""GPU: `model.train_norm = "fused"` - the kernels of csrc/norm.hip (train-mode BatchNorm + GELU forward / backward with fp64
statistics in a fixed order, the pooling maximum with its arg-max and the one-launch backward), the autograd functions
`_BnGelu` / `_SegmentMaxArg` of cdsegnet_amd/train_graph.py, and the whole training step in the fused mode.

Accuracy yardstick (tests/test_gpu_train_fp32.py's): metric max |g - g64| / max |g64| against torch autograd in fp64 on the same
fp32 values; bound 3 E_torch + 2^-24 with E_torch = the same metric of torch's own fp32 ops on the same device and values (the
same products summed in another order, plus the final rounding).  Three column kinds are measured SEPARATELY, never pooled (a
pooled maximum is dominated by the large-offset column): ordinary columns 0.5 + N(0, 1), one constant column (3.0: its dgamma
must be exactly 0), one column 1000 + 0.01 N(0, 1).

Every figure is printed with report(...) before it is asserted; profiles/NOTES.md ("Train-mode BatchNorm + GELU and pooling
maximum in HIP") keeps one run's lines.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import load_fixture
from tests.test_gpu_deterministic import _batch, _model, _step
from tests.test_gpu_ops import _library_variant, _physical, dev, ops, report  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EPS, MOM = 1e-3, 0.01  # the model's BatchNorm1d(eps=1e-3, momentum=0.01)
CONST_COL, BIG_COL = 3, 7
KINDS = ("ordinary", "constant", "offset")


def _cols(c):
    """column indices of the three kinds"""
    ordinary = [j for j in range(c) if j not in (CONST_COL, BIG_COL)]
    return {"ordinary": ordinary, "constant": [CONST_COL], "offset": [BIG_COL]}


def _data(m, c, seed):
    g = torch.Generator().manual_seed(seed)
    x = 0.5 + torch.randn(m, c, generator=g)
    x[:, CONST_COL] = 3.0
    x[:, BIG_COL] = 1000.0 + 0.01 * torch.randn(m, generator=g)
    dy = torch.randn(m, c, generator=g)
    gamma = 0.5 + torch.rand(c, generator=g)
    beta = 0.5 * torch.randn(c, generator=g)
    rm, rv = 0.1 * torch.randn(c, generator=g), 0.5 + torch.rand(c, generator=g)
    return [t.cuda() for t in (x, dy, gamma, beta, rm, rv)]


def _torch_chain(x, dy, gamma, beta, rm, rv, dtype):
    """torch's own train-mode batch norm -> GELU and its autograd in `dtype` on the device: (y, dx, dgamma, dbeta, rm, rv).
    One row, where F.batch_norm refuses to train: the same chain written out (biased variance 0, which the running variance
    takes as it is: `n > 1.0 ? var * (n / (n - 1.0)) : var` in bn_finish_kernel)."""
    xr, gr, br = (t.detach().to(dtype).clone().requires_grad_(True) for t in (x, gamma, beta))
    if x.shape[0] == 1:
        mu, var = xr.mean(0), xr.var(0, unbiased=False)
        y = F.gelu(gr * (xr - mu) / torch.sqrt(var + EPS) + br)
        y.backward(dy.to(dtype))
        return dict(y=y.detach(), dx=xr.grad, dgamma=gr.grad, dbeta=br.grad, rm=(1 - MOM) * rm.to(dtype) + MOM * mu.detach(),
                    rv=(1 - MOM) * rv.to(dtype) + MOM * var.detach())
    rm, rv = rm.to(dtype).clone(), rv.to(dtype).clone()
    y = F.gelu(F.batch_norm(xr, rm, rv, gr, br, True, MOM, EPS))
    y.backward(dy.to(dtype))
    return dict(y=y.detach(), dx=xr.grad, dgamma=gr.grad, dbeta=br.grad, rm=rm, rv=rv)


def _err(got, want, cols):
    """max |g - g64| / max |g64| over the columns of one kind (last dimension)."""
    g, w = got.double()[..., cols], want.double()[..., cols]
    top = float(w.abs().max())
    e = float((g - w).abs().max())
    return e / top if top > 0 else (0.0 if e == 0 else float("inf"))


def _one_row_dx_scale(dy, gamma, beta, invstd):
    """max |gamma invstd g| of a one-row batch, g = dy GELU'(beta) (x_hat = 0): the scale of the two terms of
    dx = gamma invstd (g - g / 1 - 0) that cancel.  dx is exactly 0 there, so the relative metric has no denominator; the kernel
    (which recomputes g in fp64 in each of its two passes) is held to 2^-24 of this scale, the unit roundoff of an fp32 result."""
    b = beta.double()
    g = dy.double() * (0.5 * torch.special.erfc(-b * 0.5 ** 0.5) + b * torch.exp(-0.5 * b * b) / (2 * np.pi) ** 0.5)
    return float((gamma.double() * invstd.double() * g).abs().max())


def _check_kinds(name, ours, c, ref64, ref32, keys, one_row_scale=None):
    """one_row_scale: `_one_row_dx_scale` of a one-row batch (dx is then judged on that scale, see there)."""
    if one_row_scale is not None:
        assert float(ref64["dx"].abs().max()) == 0.0
        report(f"{name} dx (exactly 0)", max_abs=float(ours["dx"].abs().max()), bound=U * one_row_scale)
        assert float(ours["dx"].abs().max()) <= U * one_row_scale, name
        keys = tuple(k for k in keys if k != "dx")
    for kind, cols in _cols(c).items():
        for k in keys:
            if kind == "constant" and k == "dgamma":
                assert float(ours[k][cols].abs().max()) == 0.0, (name, "dgamma of the constant column must be exactly 0")
                continue
            e, e_t = _err(ours[k], ref64[k], cols), _err(ref32[k], ref64[k], cols)
            report(f"{name} {kind} {k}", fused=e, torch=e_t, bound=3 * e_t + U)
            assert e <= 3 * e_t + U, (name, kind, k, e, e_t)


def _fused(ops, x, dy, gamma, beta, rm, rv, y=None, dx=None):
    """The op layer end to end on one rank: statistics, finish, forward, backward."""
    c = x.shape[1]
    rm, rv = rm.clone(), rv.clone()
    stats = ops.bn_stats(x)
    mean, invstd = ops.bn_finish(stats, EPS, MOM, rm, rv)
    y = ops.bn_gelu_fwd(x, mean, invstd, gamma, beta, out=y)
    dx, gs = ops.bn_gelu_bwd(x, dy, mean, invstd, gamma, beta, stats[2 * c:], out=dx)
    torch.cuda.synchronize()
    return dict(y=y, dx=dx, dgamma=gs[c:].float(), dbeta=gs[:c].float(), rm=rm, rv=rv, stats=stats, gsums=gs, mean=mean, invstd=invstd)


MS = [1, 2, 63, 64, 65, 777, 5003]
CS = [16, 32, 48, 64, 128, 256, 512]


@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("m", MS)
def test_bn_gelu_forward_and_backward_against_fp64(ops, m, c):
    """y, dx, dgamma, dbeta and the running buffers after one call, per column kind, on column slices of wider buffers (row
    stride c + 8, 16 bytes into the row) whose neighbouring columns must keep their content."""
    x, dy, gamma, beta, rm, rv = _data(m, c, 1000 * m + c)
    wide = [torch.full((m, c + 8), -7.0, device="cuda") for _ in range(4)]
    xs, dys, ys, dxs = (w[:, 4:4 + c] for w in wide)
    xs.copy_(x)
    dys.copy_(dy)
    ours = _fused(ops, xs, dys, gamma, beta, rm, rv, y=ys, dx=dxs)
    for w in wide:
        assert bool((w[:, :4] == -7.0).all()) and bool((w[:, 4 + c:] == -7.0).all())
    assert float(ours["stats"][2 * c]) == float(m)
    ref64, ref32 = _torch_chain(x, dy, gamma, beta, rm, rv, torch.float64), _torch_chain(x, dy, gamma, beta, rm, rv, torch.float32)
    _check_kinds(f"bn_gelu {m}x{c}", ours, c, ref64, ref32, ("y", "dx", "dgamma", "dbeta", "rm", "rv"),
                 _one_row_dx_scale(dy, gamma, beta, ours["invstd"]) if m == 1 else None)
    # the contiguous call gives the same bits as the strided one
    again = _fused(ops, x, dy, gamma, beta, rm, rv)
    for k in ("y", "dx", "gsums", "stats", "rm", "rv"):
        assert torch.equal(again[k], ours[k]), k


def test_summation_order_is_ascending_block_index(ops):
    """x is zero except one row in each of blocks 0 .. 3 of ops.bn_partition, holding 2^60, 1, -2^60, 1: in fp64,
    ((2^60 + 1) - 2^60) + 1 = 1.0 exactly in the documented order, 0.0 or 2.0 in others.  The same through dy for the backward
    sums: gamma = 0 and beta = 10 make GELU'(z) exactly 1 (g = dy), mean = 0 and invstd = 1 make x_hat = x = 1."""
    m, c = 5003, 32
    part = ops.bn_partition(m, c)
    assert part.blocks >= 4 and (part.blocks - 1) * part.rows_per_block < m <= part.blocks * part.rows_per_block
    vals = [2.0 ** 60, 1.0, -(2.0 ** 60), 1.0]
    rows = [b * part.rows_per_block + (17 * b + 5) % part.rows_per_block for b in range(4)]
    x = torch.zeros(m, c, device="cuda")
    for r, v in zip(rows, vals):
        x[r] = v
    stats = ops.bn_stats(x)
    torch.cuda.synchronize()
    assert torch.equal(stats[:c], torch.ones(c, dtype=torch.float64, device="cuda")), stats[:c]
    assert torch.equal(stats[c:2 * c], torch.full((c,), 2.0 ** 121 + 2.0, dtype=torch.float64, device="cuda"))
    assert float(stats[2 * c]) == m
    # another placement of the same four values: 2^60, -2^60 in blocks 0, 1 -> (0) + 1 + 1 = 2.0
    x2 = torch.zeros(m, c, device="cuda")
    for r, v in zip(rows, [vals[0], vals[2], vals[1], vals[3]]):
        x2[r] = v
    assert torch.equal(ops.bn_stats(x2)[:c], torch.full((c,), 2.0, dtype=torch.float64, device="cuda"))
    dy = x.clone()
    one, zero = torch.ones(c, device="cuda"), torch.zeros(c, device="cuda")
    count = torch.tensor([float(m)], dtype=torch.float64, device="cuda")
    _, gs = ops.bn_gelu_bwd(torch.ones(m, c, device="cuda"), dy, zero, one, zero, torch.full((c,), 10.0, device="cuda"), count)
    torch.cuda.synchronize()
    assert torch.equal(gs, torch.ones(2 * c, dtype=torch.float64, device="cuda")), gs


def test_two_calls_give_the_same_bits(ops):
    for m, c in ((5003, 32), (777, 512), (20000, 48)):
        x, dy, gamma, beta, rm, rv = _data(m, c, 5)
        a, b = _fused(ops, x, dy, gamma, beta, rm, rv), _fused(ops, x, dy, gamma, beta, rm, rv)
        for k in a:
            assert torch.equal(a[k], b[k]), (m, c, k)


def test_shard_merge_equals_the_statistics_of_all_rows(ops):
    """Three row shards of unequal size, one of them empty (a rank without rows): statistics and backward sums per shard, added
    in shard order by the merge function of the SyncBN path; y and dx per shard against the fp64 oracle of the concatenation."""
    from cdsegnet_amd.train_graph import merge_shards
    m, c = 3001, 64
    x, dy, gamma, beta, rm, rv = _data(m, c, 77)
    cuts = [(0, 1900), (1900, 1900), (1900, m)]
    stats = merge_shards([ops.bn_stats(x[a:b]) for a, b in cuts])
    assert float(stats[2 * c]) == m
    rm1, rv1 = rm.clone(), rv.clone()
    mean, invstd = ops.bn_finish(stats, EPS, MOM, rm1, rv1)
    ys = [ops.bn_gelu_fwd(x[a:b], mean, invstd, gamma, beta) for a, b in cuts]
    locals_ = []

    def hook(gs):
        locals_.append(gs)
        return gs

    for a, b in cuts:  # first pass of every shard: its own sums
        ops.bn_gelu_bwd(x[a:b], dy[a:b], mean, invstd, gamma, beta, stats[2 * c:], hook=hook)
    total = merge_shards(locals_[:3])
    dxs = [ops.bn_gelu_bwd(x[a:b], dy[a:b], mean, invstd, gamma, beta, stats[2 * c:], hook=lambda gs: total)[0] for a, b in cuts]
    torch.cuda.synchronize()
    assert ys[1].shape == (0, c) and dxs[1].shape == (0, c) and float(locals_[1].abs().max()) == 0.0
    ours = dict(y=torch.cat(ys), dx=torch.cat(dxs), dgamma=total[c:].float(), dbeta=total[:c].float(), rm=rm1, rv=rv1)
    ref64, ref32 = _torch_chain(x, dy, gamma, beta, rm, rv, torch.float64), _torch_chain(x, dy, gamma, beta, rm, rv, torch.float32)
    _check_kinds("shard merge 3001x64", ours, c, ref64, ref32, ("y", "dx", "dgamma", "dbeta", "rm", "rv"))


def test_non_finite_dy_reaches_dx(ops):
    x, dy, gamma, beta, rm, rv = _data(300, 32, 9)
    dy[17, 5] = float("inf")
    dx = _fused(ops, x, dy, gamma, beta, rm, rv)["dx"]
    assert not bool(torch.isfinite(dx[:, 5]).all()) and bool(torch.isfinite(dx[:, :5]).all()) and bool(torch.isfinite(dx[:, 6:]).all())


# ------------------------------------------------------------------------------------------ pooling maximum
def _first_max(y, out, cl, m):
    n, c = y.shape
    rows = torch.arange(n, device=y.device)[:, None].expand(n, c)
    cand = torch.where(y == out[cl], rows, torch.full_like(rows, n))
    return torch.full((m, c), n, dtype=torch.long, device=y.device).scatter_reduce(0, cl[:, None].expand(n, c), cand, "amin")


@pytest.mark.parametrize("c", [16, 64, 512])
def test_segment_max_arg_and_backward_on_the_pooling_link(ops, c):
    """The pooling link of `room1500` with planted exact ties: first / middle / last child of a run all equal to the maximum
    (arg = the first), middle and last only (arg = the middle), one run with all values equal.  out = cdseg_segment_max's
    bits, arg = the first maximal row; dy = `_SegmentMax.backward`'s result on the same input (every non-zero element bit for bit,
    the zeros as zeros of either sign: 0 * dout is -0 under a negative dout) - with an inf in dout arriving at
    its child (planted on a one-child run for the bit comparison: torch's mask * dout form turns the SIBLINGS of an inf into
    0 * inf = nan, where this kernel writes the 0 the definition says; that difference is asserted on a second dout)."""
    from cdsegnet_amd.train_graph import _SegmentMax, _SegmentMaxArg
    fx = load_fixture("serialization_room1500.npz")
    zs = _physical(ops, fx)[0]
    cluster, seg, cnt = ops.pool_level(zs, 3)
    m, n = int(cnt.item()), zs.numel()
    lens = (seg[1:m + 1] - seg[:m]).cpu()
    long_runs = torch.nonzero(lens >= 3).flatten().tolist()
    single = torch.nonzero(lens == 1).flatten().tolist()
    assert len(long_runs) >= 3 and single and int(lens.sum()) == n and int(lens.min()) >= 1
    g = torch.Generator().manual_seed(c)
    y = torch.randn(n, c, generator=g).cuda()
    sh = seg.cpu().tolist()
    ja, jb, jc = long_runs[0], long_runs[1], long_runs[2]
    a0, a1 = sh[ja], sh[ja + 1]
    y[[a0, (a0 + a1 - 1) // 2, a1 - 1]] = 9.0
    b0, b1 = sh[jb], sh[jb + 1]
    y[[(b0 + b1 - 1) // 2, b1 - 1]] = 9.0
    y[sh[jc]:sh[jc + 1]] = -2.5
    out, arg = ops.segment_max_arg(y, seg, m)
    one = torch.ones(c, device="cuda")
    want = torch.empty(m, c, device="cuda")
    ops.segment_max(y, seg, m, one, torch.zeros_like(one), ops.ACT_NONE, want)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    cl = cluster.long()
    assert torch.equal(arg.long(), _first_max(y, want, cl, m))
    assert bool((arg[ja] == a0).all()) and bool((arg[jb] == (b0 + b1 - 1) // 2).all()) and bool((arg[jc] == sh[jc]).all())
    # backward
    dout = torch.randn(m, c, generator=g).cuda()
    dout[single[0], 3] = float("inf")
    yr = y.clone().requires_grad_(True)
    _SegmentMax.apply(yr, seg, cluster, m).backward(dout)
    dy = ops.segment_max_bwd(dout, arg, cluster)
    torch.cuda.synchronize()
    # (value equality: where torch's mask * dout form leaves a 0 of dout's sign, the kernel writes the +0 of the definition)
    assert torch.equal(dy, yr.grad)
    assert bool(((dy != 0) == (yr.grad != 0)).all()) and bool((dy[dy != 0].view(torch.int32) == yr.grad[dy != 0].view(torch.int32)).all())
    assert float(dy[sh[single[0]], 3]) == float("inf")
    yr2 = y.clone().requires_grad_(True)
    _SegmentMaxArg.apply(yr2, seg, cluster, m).backward(dout)
    assert torch.equal(yr2.grad, dy)
    dout2 = dout.clone()
    dout2[ja, 1] = float("inf")
    dy2 = ops.segment_max_bwd(dout2, arg, cluster)
    assert float(dy2[a0, 1]) == float("inf") and float(dy2[a0 + 1:a1, 1].abs().max()) == 0.0
    assert int((dy2 != 0).sum()) <= m * c and bool((dy2[:, 0] != 0).sum() <= m)


# ------------------------------------------------------------------------------------------ autograd functions
def test_autograd_functions_against_the_torch_chain(ops):
    """`_bn_gelu(..., "fused")` (-> `_BnGelu`) under torch.autograd: y, dx, dgamma, dbeta and the module's buffers per column
    kind; `_SegmentMaxArg` gives `_SegmentMax`'s output and gradient bits."""
    from cdsegnet_amd import train_graph as tg
    for m, c in ((777, 32), (4100, 128)):
        x, dy, gamma, beta, rm, rv = _data(m, c, 31 + c)
        bn = torch.nn.BatchNorm1d(c, eps=EPS, momentum=MOM).cuda().train()
        with torch.no_grad():
            bn.weight.copy_(gamma)
            bn.bias.copy_(beta)
            bn.running_mean.copy_(rm)
            bn.running_var.copy_(rv)
        xr = x.clone().requires_grad_(True)
        y = tg._bn_gelu(xr, bn, "fused")
        assert type(y.grad_fn).__name__.startswith("_BnGelu")
        y.backward(dy)
        torch.cuda.synchronize()
        assert int(bn.num_batches_tracked) == 1
        ours = dict(y=y.detach(), dx=xr.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, rm=bn.running_mean, rv=bn.running_var)
        ref64, ref32 = _torch_chain(x, dy, gamma, beta, rm, rv, torch.float64), _torch_chain(x, dy, gamma, beta, rm, rv, torch.float32)
        _check_kinds(f"_BnGelu {m}x{c}", ours, c, ref64, ref32, ("y", "dx", "dgamma", "dbeta", "rm", "rv"))
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        tg._bn_gelu(torch.zeros(1, 32, device="cuda"), torch.nn.BatchNorm1d(32).cuda(), "fused")


# ------------------------------------------------------------------------------------------ the whole step
def _counted(monkeypatch, O):
    calls = {"bn_fwd": 0, "bn_bwd": 0, "arg": 0, "arg_bwd": 0, "batch_norm": 0}
    seen = []

    def counted(key, fn, keep=False):
        def f(*a, **kw):
            calls[key] += 1
            if keep and len(seen) < 2:
                seen.append(a[0].detach().clone())
            return fn(*a, **kw)
        return f

    # (monkeypatch.setattr raises where the attribute does not exist: the model ignores an unknown train_norm silently)
    monkeypatch.setattr(O, "bn_gelu_fwd", counted("bn_fwd", O.bn_gelu_fwd, keep=True))
    monkeypatch.setattr(O, "bn_gelu_bwd", counted("bn_bwd", O.bn_gelu_bwd))
    monkeypatch.setattr(O, "segment_max_arg", counted("arg", O.segment_max_arg))
    monkeypatch.setattr(O, "segment_max_bwd", counted("arg_bwd", O.segment_max_bwd))
    monkeypatch.setattr(F, "batch_norm", counted("batch_norm", F.batch_norm))
    return calls, seen


def _buffers(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items() if "running_" in k or "num_batches" in k}


def test_whole_step_fused_against_torch(ops, monkeypatch):
    """The mini model on two synthetic rooms, both modes from the same state: the same loss and gradients up to rounding (metric
    and 1e-3 sanity bound of tests/test_gpu_deterministic.py::test_whole_step_is_bit_reproducible), the BatchNorm buffers
    likewise, and those of the two stems - whose input is the same tensor in both modes - against their fp64 definition
    within the yardstick; one fused BatchNorm call per training-mode BatchNorm module the forward passes, one arg-max call per
    pooling module, no F.batch_norm call left."""
    from cdsegnet_amd import models
    from cdsegnet_amd import ops as O
    inp, draws, n = _batch()
    model = _model("fp32", False).train()
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    calls, seen = _counted(monkeypatch, O)

    def run(mode):
        model.load_state_dict(state)
        model.train_norm = mode
        for k in calls:
            calls[k] = 0
        loss, grads = _step(model, inp, dict(draws))
        return loss, grads, _buffers(model), dict(calls)

    l0, g0, b0, c0 = run("torch")
    l1, g1, b1, c1 = run("fused")
    moved = sum(int(b1[k]) == int(state[k]) + 1 for k in b1 if k.endswith("num_batches_tracked"))
    pools = sum(isinstance(mod, models.SerializedPooling) for mod in model.modules())
    assert c0["batch_norm"] == moved and c0["bn_fwd"] == c0["arg"] == 0
    assert c1 == {"bn_fwd": moved, "bn_bwd": moved, "arg": pools, "arg_bwd": pools, "batch_norm": 0}, c1
    assert moved > 0 and pools > 0 and set(g0) == set(g1) and len(g0) > 400
    top = max(float(g.abs().max()) for g in g0.values())
    worst = max(float((g0[k] - g1[k]).abs().max()) / (float(g0[k].abs().max()) + 1e-3 * top) for k in g0)
    worst_buf = max(float((b0[k].double() - b1[k].double()).abs().max()) / float(b0[k].double().abs().max()) for k in b0
                    if not k.endswith("num_batches_tracked"))
    report("whole step fused vs torch", loss_torch=float(l0), loss_fused=float(l1), worst_grad_rel_diff=worst, worst_buffer_rel_diff=worst_buf)
    assert bool(torch.isfinite(l1)) and abs(float(l0) - float(l1)) <= 1e-3 * abs(float(l0))
    assert worst < 1e-3 and worst_buf < 1e-3
    assert all(torch.equal(b0[k], b1[k]) for k in b0 if k.endswith("num_batches_tracked"))
    # the stems: input captured at the first two fused calls (c-branch, then n-branch embedding)
    assert len(seen) == 2
    for x, name in zip(seen, ("backbone._c_embedding.stem.norm", "backbone._n_embedding.stem.norm")):
        xd = x.double()
        mean, var = xd.mean(0), xd.var(0, unbiased=True)
        for buf, v in (("running_mean", mean), ("running_var", var)):
            k = f"{name}.{buf}"
            want = (1 - MOM) * state[k].double() + MOM * v
            e, e_t = _err(b1[k], want, slice(None)), _err(b0[k], want, slice(None))
            report(f"whole step {k}", fused=e, torch=e_t, bound=3 * e_t + U)
            assert e <= 3 * e_t + U, (k, e, e_t)


def test_recorded_step_in_the_fused_mode_meets_the_reference_bound(ops, monkeypatch):
    """tests/test_gpu_train.py's comparison against the reference's recorded step (`train_step_mini.npz`), run as it is on a
    model with train_norm = "fused": the same assertions, the same bounds."""
    from cdsegnet_amd import ops as O
    from tests import test_gpu_train as T
    build = T._mini_training_model

    def fused_model(fx, dev_):
        model, sd = build(fx, dev_)
        model.train_norm = "fused"
        return model, sd

    calls, _ = _counted(monkeypatch, O)
    monkeypatch.setattr(T, "_mini_training_model", fused_model)
    T.test_whole_training_step_matches_the_reference_train_step()
    assert calls["bn_fwd"] > 0 and calls["bn_fwd"] == calls["bn_bwd"] and calls["arg"] > 0 and calls["batch_norm"] == 0, calls


@pytest.mark.parametrize("tp", ["fp32", "fp16-amp"])
def test_fused_step_is_bit_reproducible_in_the_deterministic_mode(ops, monkeypatch, tp):
    """train_deterministic = True with the fused sites: two passes give bit-equal loss, .grad and BatchNorm buffers."""
    from cdsegnet_amd import ops as O
    inp, draws, n = _batch()
    model = _model(tp, True).train()
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    calls, _ = _counted(monkeypatch, O)
    runs = []
    for _ in range(2):
        model.load_state_dict(state)
        model.train_precision, model.train_deterministic, model.train_norm = tp, True, "fused"
        loss, grads = _step(model, inp, dict(draws))
        runs.append((loss, grads, _buffers(model)))
    (l1, g1, b1), (l2, g2, b2) = runs
    assert calls["bn_fwd"] > 0 and calls["batch_norm"] == 0
    assert bool(torch.isfinite(l1)) and torch.equal(l1, l2)
    assert set(g1) == set(g2) and len(g1) > 400
    diff = [k for k in g1 if not torch.equal(g1[k], g2[k])] + [k for k in b1 if not torch.equal(b1[k], b2[k])]
    assert not diff, diff[:8]
