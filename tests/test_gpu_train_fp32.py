"""GPU: the DEFAULT fp32 training kernels (csrc/train.hip wgrad_kernel, layernorm_bwd_kernel, gelu_bwd_kernel,
attn_bwd_{q,kv}_mfma_kernel) and the fp32 autograd functions of cdsegnet_amd/train_graph.py, at every width the model runs
(C = 16 .. 512, 16 and 32 heads, fc1 / fc2 / qkv shapes, 27-offset convs up to 512 channels) and at the row counts where the
kernels change path (1 row, the 16-row wave, the 64-row block, split boundaries, a last split that is no multiple of 4).

References are plain torch / numpy definitions of the operation in fp64 on the same fp32 values; none calls cdsegnet_amd.ops.

Bounds, none of them a constant fitted to the kernels' output:
  (a) integers in [-3, 3]: every partial sum is an integer far below 2^24, so fp32 accumulation is exact in ANY order (atomics
      included) and the result must EQUAL the integer result.
  (b) ordinary values: per element |g - g64| <= 1.01 (R + S) 2^-24 (|dy|^T |x|)[n][k], R = rows per split and S = splits of
      ops.wgrad_partition: R fused multiply-adds then S atomic adds, each within 2^-24 of a partial sum that |dy|^T |x| bounds.
      Derived, so it holds for every summation order; one dropped row or one wrong operand element exceeds it many times over.
  (c), (d) LayerNorm / GELU backward: metric max |g - g64| / max |g64| per tensor; bound 3 E_torch + 2^-24, E_torch = the same
      metric of torch's own fp32 backward on the same device and values (the form and margin of
      tests/test_gpu_deterministic.py::test_layernorm_bwd_is_bit_repeatable_and_matches_torch: the same mathematics in another
      order of operations, plus the final rounding).
  (e) attention backward: 2 E_ref + L 2^-24 (the form tests/test_gpu_attention_bwd16.py documents), E_ref = the error of the
      same dense per-patch softmax attention written in torch and differentiated by autograd in float32 on the device.

Every figure is printed with report(...) before it is asserted; profiles/NOTES.md ("fp32 training kernels against fp64")
keeps one run's lines.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_attention_bwd16 import SCALE, Launch, _case, _grads, _kernel
from tests.test_gpu_attention_bwd16 import _metric as _np_metric
from tests.test_gpu_deterministic import _kernel_map
from tests.test_gpu_ops import _library_variant, dev, ops, report  # noqa: F401  (fixtures)
from tests.test_gpu_wgrad16 import _eq, _exact, _ints

pytestmark = pytest.mark.gpu

F32 = torch.float32
U = 2.0 ** -24  # half an ulp of 1.0: the unit roundoff of fp32


def _sync():
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ (a) exact on integers
def _premise(M, *ts):
    """Operands are integers in [-3, 3]: a product is at most 9, a pre-filled element at most 21, and two launches into it stay
    far below 2^24 - every partial sum is an exactly representable integer whatever the order of the adds."""
    assert all(float(t.abs().max()) <= 3 and bool((t == t.round()).all()) for t in ts)
    assert 21 + 2 * 9 * M < 2 ** 20


def _want(dy, x, xidx=None):
    """tests/test_gpu_wgrad16.py's _exact on the device (fp64 there is exact on these integers too) -> int64 on the host."""
    w, b = _exact(dy, x, xidx)
    return w.cpu(), b.cpu()


DENSE = [(1, 16, 16), (3, 16, 48), (1027, 48, 80), (4101, 32, 96), (2050, 64, 256), (2050, 128, 512), (3075, 256, 512),
         (2103, 512, 256), (2103, 512, 1536), (2103, 512, 2048), (2103, 2048, 512)]


ROUTED = [(1, 16, 16), (2050, 64, 256)]  # the shapes whose launch record is asserted: one split, several


def _partition(ops, M, N, K, kvol=1):
    part = ops.wgrad_partition(M, N, K, kvol, F32)
    assert (part.splits - 1) * part.rows_per_split < M <= part.splits * part.rows_per_split, tuple(part)
    return part


@pytest.mark.parametrize("M,K,N", DENSE, ids=[f"{m}x{k}x{n}" for m, k, n in DENSE])
def test_default_wgrad_exact_on_integers(ops, M, K, N):
    """ops.linear_wgrad, default mode, fp32: contiguous; without db; strided operands into a pre-filled dw view with lddw > K
    (twice: twice the sum, neighbouring columns untouched); gathered with -1 entries, repeated rows and a dead stretch that
    starts at a split boundary."""
    part = _partition(ops, M, N, K)
    if M >= 2050:
        assert part.splits >= 2, tuple(part)
    if M == 2103:  # the last split ends inside a 4-row MFMA step
        assert (M - (part.splits - 1) * part.rows_per_split) % 4 != 0, tuple(part)
    rng = np.random.default_rng(M + 7 * K + 13 * N)
    x, dy = _ints(rng, M, K), _ints(rng, M, N)
    _premise(M, x, dy)
    xd, dyd = x.cuda(), dy.cuda()
    want_w, want_b = _want(dyd, xd)
    dw, db, dw_nob = torch.zeros(N, K, device="cuda"), torch.zeros(N, device="cuda"), torch.zeros(N, K, device="cuda")
    with ops.record_routes() as rr:
        ops.linear_wgrad(xd, dyd, dw, db)
    ops.linear_wgrad(xd, dyd, dw_nob, None)
    _sync()
    assert _eq(dw, want_w) and _eq(db, want_b), "contiguous"
    assert _eq(dw_nob, want_w), "db = None"
    if (M, K, N) in ROUTED:  # the launch record: the atomic kernel, then the fixed-order one, on the partition asked for above
        assert rr.count == 1 and rr.kernels() == ["wgrad_kernel"], rr.routes
        assert (rr.routes[0].splits, rr.routes[0].xmode, rr.routes[0].aux) == (part.splits, part.rows_per_split, 1), rr.routes
        dw_det, db_det = torch.zeros(N, K, device="cuda"), torch.zeros(N, device="cuda")
        with ops.record_routes() as rr:
            ops.linear_wgrad(xd, dyd, dw_det, db_det, deterministic=True)
        _sync()
        assert _eq(dw_det, want_w) and _eq(db_det, want_b), "deterministic"
        assert rr.count == 1 and rr.kernels() == ["wgrad_det_kernel"], rr.routes
        assert (rr.routes[0].splits, rr.routes[0].xmode, rr.routes[0].aux) == (part.splits, part.rows_per_split, 1), rr.routes
    # strided operands, pre-filled results
    xw, dyw = _ints(rng, M, K + 24).cuda(), _ints(rng, M, N + 16).cuda()
    xw[:, 8:8 + K] = xd
    dyw[:, 16:] = dyd
    pre_w, pre_b = _ints(rng, N, K + 12) * 5, _ints(rng, N) * 7
    wide, db = pre_w.cuda().clone(), pre_b.cuda().clone()
    for times in (1, 2):
        ops.linear_wgrad(xw[:, 8:8 + K], dyw[:, 16:], wide[:, 4:4 + K], db)
        _sync()
        assert _eq(wide[:, 4:4 + K], pre_w[:, 4:4 + K].long() + times * want_w), f"strided, call {times}"
        assert _eq(db, pre_b.long() + times * want_b), f"strided db, call {times}"
    assert torch.equal(wide[:, :4].cpu(), pre_w[:, :4]) and torch.equal(wide[:, 4 + K:].cpu(), pre_w[:, 4 + K:])
    # gathered
    R = max(1, M // 2)
    xs = _ints(rng, R, K)
    idx = rng.integers(0, R, size=M)
    idx[rng.random(M) < 0.3] = -1
    if M >= 9:
        idx[5:9] = idx[4]
    if part.splits >= 2:
        a = part.rows_per_split  # split 1 starts dead
        idx[a:a + 200] = -1
    idx = torch.as_tensor(idx, dtype=torch.int32).cuda()
    want_w, want_b = _want(dyd, xs.cuda(), idx)
    dw, db, dw_nob = torch.zeros(N, K, device="cuda"), torch.zeros(N, device="cuda"), torch.zeros(N, K, device="cuda")
    ops.linear_wgrad(xs.cuda(), dyd, dw, db, xidx=idx)
    ops.linear_wgrad(xs.cuda(), dyd, dw_nob, None, xidx=idx)
    _sync()
    assert _eq(dw, want_w) and _eq(db, want_b) and _eq(dw_nob, want_w), "gathered"


CONV = [(128, 128, 3, "batch2"), (256, 256, 3, "room1500"), (512, 512, 3, "room1500"), (512, 512, 3, "tiny64"), (16, 32, 5, "batch2")]


@pytest.mark.parametrize("cin,cout,ksize,name", CONV, ids=[f"{a}-{b}-k{k}-{n}" for a, b, k, n in CONV])
def test_default_conv_wgrad_exact_on_integers(ops, cin, cout, ksize, name):
    """ops.conv_wgrad, default mode, on real kernel maps into a pre-filled dw3 / db: every offset against the gathered product
    (lddw = kvol * cin up to 27 * 512, dw_off_stride = cin).  (16, 32, 5) is the stem: x columns 6 .. are zero."""
    nbr = _kernel_map(ops, name, ksize)
    kvol, M = nbr.shape
    assert kvol == ksize ** 3
    _partition(ops, M, cout, cin, kvol)
    rng = np.random.default_rng(cin + cout + kvol + M)
    x, dy = _ints(rng, M, cin), _ints(rng, M, cout)
    if ksize == 5:
        x[:, 6:] = 0
    _premise(M, x, dy)
    xd, dyd = x.cuda(), dy.cuda()
    pre_w, pre_b = _ints(rng, cout, kvol, cin) * 3, _ints(rng, cout) * 7
    dw3, db = pre_w.cuda().clone(), pre_b.cuda().clone()
    ops.conv_wgrad(xd, nbr, dyd, dw3, db)
    _sync()
    got = dw3.cpu()
    for o in range(kvol):
        assert _eq(got[:, o, :], pre_w[:, o, :].long() + _want(dyd, xd, nbr[o])[0]), o
    assert _eq(db, pre_b.long() + dy.double().sum(0).long())


# ------------------------------------------------------------------------------------------ (b) ordinary values
def _rel(g, g64):
    return float((g.double() - g64).abs().max()) / float(g64.abs().max())


def _assert_within_chain_bound(what, g, g64, mass, part):
    """|g - g64| <= 1.01 (R + S) 2^-24 mass, element by element.  Returns the largest fraction of the bound that is used."""
    bound = 1.01 * (part.rows_per_split + part.splits) * U * mass
    diff = (g.double() - g64).abs()
    assert bool(torch.isfinite(g).all()), what
    used = float((diff / bound.clamp_min(1e-300)).max())
    over = int((diff > bound).sum())
    report(f"wgrad fp32 {what}", bound_used=used, elements_over=over, of=diff.numel())
    assert over == 0, (what, used, over)
    return used


ORDINARY = [(2103, 512, 2048), (2103, 2048, 512), (5003, 48, 96)]


@pytest.mark.parametrize("M,K,N", ORDINARY, ids=[f"{m}x{k}x{n}" for m, k, n in ORDINARY])
def test_default_wgrad_on_ordinary_values_within_the_derived_bound(ops, M, K, N):
    """x = N(0, 1), dy = 0.1 N(0, 1) in fp32, oracle fp64 on the same values (torch's float64 product on the device)."""
    part = _partition(ops, M, N, K)
    g = torch.Generator().manual_seed(M + K)
    x, dy = torch.randn(M, K, generator=g).cuda(), (0.1 * torch.randn(M, N, generator=g)).cuda()
    x64, dy64 = x.double(), dy.double()
    w64, b64 = dy64.T @ x64, dy64.sum(0)
    dw, db = torch.zeros(N, K, device="cuda"), torch.zeros(N, device="cuda")
    ops.linear_wgrad(x, dy, dw, db)
    _sync()
    t_w, t_b = dy.T @ x, dy.sum(0)  # torch's fp32 on the device: reported, not asserted
    report(f"wgrad fp32 {M}x{K}x{N} vs torch fp32", kernel_dw=_rel(dw, w64), torch_dw=_rel(t_w, w64),
           ratio_dw=_rel(dw, w64) / _rel(t_w, w64), kernel_db=_rel(db, b64), torch_db=_rel(t_b, b64),
           ratio_db=_rel(db, b64) / max(_rel(t_b, b64), 1e-300), rows_per_split=part.rows_per_split, splits=part.splits)
    _assert_within_chain_bound(f"{M}x{K}x{N} dw", dw, w64, dy64.abs().T @ x64.abs(), part)
    _assert_within_chain_bound(f"{M}x{K}x{N} db", db, b64, dy64.abs().sum(0), part)


def test_default_conv_wgrad_on_ordinary_values_within_the_derived_bound(ops):
    cin = cout = 256
    nbr = _kernel_map(ops, "room1500", 3)
    kvol, M = nbr.shape
    part = _partition(ops, M, cout, cin, kvol)
    g = torch.Generator().manual_seed(M)
    x, dy = torch.randn(M, cin, generator=g).cuda(), (0.1 * torch.randn(M, cout, generator=g)).cuda()
    dy64 = dy.double()
    dw3, db = torch.zeros(cout, kvol, cin, device="cuda"), torch.zeros(cout, device="cuda")
    ops.conv_wgrad(x, nbr, dy, dw3, db)
    _sync()
    w64, mass, t_w = (torch.empty(cout, kvol, cin, dtype=dt, device="cuda") for dt in (torch.float64, torch.float64, F32))
    for o in range(kvol):
        live = (nbr[o] >= 0)[:, None]
        xo = x[nbr[o].clamp(min=0).long()] * live
        w64[:, o], mass[:, o], t_w[:, o] = dy64.T @ xo.double(), dy64.abs().T @ xo.double().abs(), dy.T @ xo
    report(f"conv wgrad fp32 {cin}-{cout}-k3 room1500 vs torch fp32", kernel_dw=_rel(dw3, w64), torch_dw=_rel(t_w, w64),
           ratio_dw=_rel(dw3, w64) / _rel(t_w, w64), rows_per_split=part.rows_per_split, splits=part.splits)
    _assert_within_chain_bound("conv 256-256-k3 dw", dw3, w64, mass, part)
    _assert_within_chain_bound("conv 256-256-k3 db", db, dy64.sum(0), dy64.abs().sum(0), part)


# ------------------------------------------------------------------------------------------ (c) LayerNorm backward
EPS = 1e-5


def _ln_inputs(M, C, const_rows, seed):
    """x = 0.5 + N(0, 1), gamma = 1 + 0.3 N(0, 1), dy = N(0, 1); `const_rows` hold 3.0 in every element: their mean is exact
    and their variance exactly zero in fp32, so only eps keeps 1 / sigma finite."""
    g = torch.Generator().manual_seed(seed)
    x, gamma, dy = 0.5 + torch.randn(M, C, generator=g), 1 + 0.3 * torch.randn(C, generator=g), torch.randn(M, C, generator=g)
    x[const_rows] = 3.0
    pre = dict(dx=torch.randn(M, C, generator=g), dg=torch.randn(C, generator=g), db=torch.randn(C, generator=g))
    return x.cuda(), gamma.cuda(), dy.cuda(), {k: v.cuda() for k, v in pre.items()}


def _ln_autograd(x, gamma, dy, dtype):
    """(y, dx, dgamma, dbeta) of F.layer_norm by torch autograd on the device in `dtype`, on the same fp32 values."""
    xr, gr = (t.detach().to(dtype).clone().requires_grad_(True) for t in (x, gamma))  # (.to alone returns the fp32 input itself)
    br = torch.zeros_like(gr).requires_grad_(True)
    y = F.layer_norm(xr, (x.shape[1],), gr, br, EPS)
    y.backward(dy.to(dtype))
    return y.detach(), xr.grad, gr.grad, br.grad


def _err(g, g64, rows=None):
    """max |g - g64| / max |g64| (over `rows` when given)."""
    if rows is not None:
        g, g64 = g[rows], g64[rows]
    top = float(g64.abs().max())
    assert top > 0
    return float((g.double() - g64).abs().max()) / top


def _assert_vs_torch(what, pairs):
    """pairs: (tensor name, kernel result, torch fp32 result, fp64 oracle, rows or None).  kernel <= 3 E_torch + 2^-24."""
    for tn, got, t32, g64, rows in pairs:
        assert bool(torch.isfinite(got).all()), (what, tn)
        e, et = _err(got, g64, rows), _err(t32, g64, rows)
        report(f"{what} {tn}", kernel_err=e, E_torch=et, bound=3 * et + U)
        assert e <= 3 * et + U, (what, tn, e, et)


def _const_rows(M):
    return [0, M // 2, M - 1] if M >= 15 else []


_LN_C = (16, 32, 48, 64, 96, 128, 256, 512, 640)  # 640: rows wider than LNB_MAXC, the per-element-atomic branch
LN_CASES = [(M, C, "plain", None) for C in _LN_C for M in (65, 777)]
LN_CASES += [(M, C, "plain", None) for M in (1, 15, 16, 17, 63, 64) for C in (48, 512)]
LN_CASES += [(1, 48, "plain", [0]), (1, 512, "plain", [0]), (17, 640, "plain", None), (1, 640, "plain", None)]
LN_CASES += [(M, C, v, None) for (M, C) in ((65, 96), (777, 512), (65, 640))
             for v in ("strided", "accumulate", "dgamma-only", "dbeta-only", "neither")]


@pytest.mark.parametrize("M,C,variant,const", LN_CASES,
                         ids=[f"{m}x{c}-{v}" + ("-const" if k else "") for m, c, v, k in LN_CASES])
def test_layernorm_bwd_vs_fp64_within_three_times_torch(ops, M, C, variant, const):
    """ops.layernorm_bwd, default mode.  strided: x / dy / dx are column slices of wider buffers (dx's neighbours stay);
    accumulate: the same, accumulate=True into a pre-filled dx and pre-filled dgamma / dbeta (they are added to);
    dgamma-only / dbeta-only / neither: the other pointer(s) NULL (neither: no block sums at all).  dx is measured
    separately over the constant rows and over the rest.  (On an MI355X torch's own dgamma is 2e-5 .. 2e-4 off at C = 48 and
    C = 96, so that one bound is loose at those two widths; everywhere else E_torch is 1 - 3e-7.  profiles/NOTES.md.)"""
    const = _const_rows(M) if const is None else const
    rest = [r for r in range(M) if r not in set(const)]
    x, gamma, dy, pre = _ln_inputs(M, C, const, 1000 * M + C)
    _, dx64, dg64, db64 = _ln_autograd(x, gamma, dy, torch.float64)
    _, dxt, dgt, dbt = _ln_autograd(x, gamma, dy, F32)
    strided, acc = variant in ("strided", "accumulate"), variant == "accumulate"
    want_g, want_b = variant != "dbeta-only" and variant != "neither", variant != "dgamma-only" and variant != "neither"
    if strided:
        xw, dyw = torch.randn(M, C + 24, device="cuda"), torch.randn(M, C + 16, device="cuda")
        xw[:, 8:8 + C] = x
        dyw[:, 16:] = dy
        xk, dyk = xw[:, 8:8 + C], dyw[:, 16:]
        dxw = torch.randn(M, C + 12, device="cuda")
        dxw[:, 4:4 + C] = pre["dx"]
        before = dxw.clone()
        dx = dxw[:, 4:4 + C]
    else:
        xk, dyk, dx = x, dy, pre["dx"].clone()
    dg = (pre["dg"].clone() if acc else torch.zeros(C, device="cuda")) if want_g else None
    db = (pre["db"].clone() if acc else torch.zeros(C, device="cuda")) if want_b else None
    ops.layernorm_bwd(xk, gamma, dyk, dx, accumulate=acc, eps=EPS, dgamma=dg, dbeta=db)
    _sync()
    if strided:
        assert torch.equal(dxw[:, :4], before[:, :4]) and torch.equal(dxw[:, 4 + C:], before[:, 4 + C:])
    if acc:  # what is compared is pre-filled + gradient, for the kernel, for torch's fp32 and for the oracle alike
        dx64, dxt = pre["dx"].double() + dx64, pre["dx"] + dxt
        dg64, dgt, db64, dbt = pre["dg"].double() + dg64, pre["dg"] + dgt, pre["db"].double() + db64, pre["db"] + dbt
    pairs = []
    if rest:
        pairs.append(("dx", dx, dxt, dx64, rest))
    if const:
        pairs.append(("dx (constant rows)", dx, dxt, dx64, const))
    if want_g and rest:  # (a constant row's normalised input is exactly zero: no dgamma without an ordinary row)
        pairs.append(("dgamma", dg, dgt, dg64, None))
    if want_b:
        pairs.append(("dbeta", db, dbt, db64, None))
    _assert_vs_torch(f"layernorm_bwd ({M}, {C}) {variant}", pairs)


# ------------------------------------------------------------------------------------------ (d) GELU backward
_SPECIAL = [0.0] + [s * v for v in (1e-30, 1e-8, 0.5, 3.0, 6.0, 10.0, 40.0, 1e4, 1e20) for s in (1.0, -1.0)]


def _gelu_grad64(u, dy):
    """dy (Phi(u) + u phi(u)) in fp64; Phi through erfc so that the lower tail does not cancel."""
    u, dy = u.double(), dy.double()
    cdf = 0.5 * torch.special.erfc(-u * 0.5 ** 0.5)
    pdf = torch.exp(-0.5 * u * u) / (2 * np.pi) ** 0.5
    return dy * (cdf + u * pdf)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_gelu_bwd_vs_closed_form_within_three_times_torch(ops, n):
    """Pre-activations 0, +-1e-30 .. +-1e20 (u^2 overflows to inf at 1e20: exp(-inf) = 0, no NaN) and a bulk of 2 N(0, 1).
    n = 1: every special value in a launch of its own, compared as one vector."""
    g = torch.Generator().manual_seed(n)
    sp = torch.tensor(_SPECIAL)
    if n == 1:
        u = sp.clone()
    else:
        u = torch.cat([sp, 2 * torch.randn(n - len(sp), generator=g)])[torch.randperm(n, generator=g)]
    dy = torch.randn(u.numel(), generator=g)
    ud, dyd = u.cuda(), dy.cuda()
    if n == 1:
        got = torch.cat([ops.gelu_bwd(ud[i:i + 1].clone(), dyd[i:i + 1].clone()) for i in range(u.numel())])
    else:
        got = ops.gelu_bwd(ud, dyd)
    _sync()
    ur = ud.clone().requires_grad_(True)
    F.gelu(ur).backward(dyd)
    assert got.shape == ud.shape
    _assert_vs_torch(f"gelu_bwd n={n}", [("dx", got, ur.grad, _gelu_grad64(ud, dyd), None)])


# ------------------------------------------------------------------------------------------ (e) attention backward
def _f32_values(*arrays):
    return tuple(np.asarray(a, dtype=np.float32).astype(np.float64) for a in arrays)


def _attn_case(lens, H, dup, cross, seed):
    """tests/test_gpu_attention_bwd16.py's _case with lp = float32: the operands keep the full fp32 mantissa.  Padding
    duplicates of the last patch are redrawn WITHOUT replacement (a row sits in at most two slots, as in the padding plan)."""
    rng = np.random.default_rng(seed)
    launch, (q, k, v, do) = _case(lens, H, dup, cross, F32, rng, 1.0)
    if dup:
        patches = list(launch.patches)
        gq, gkv, widx = (a.copy() for a in patches[-1])
        own = len(gq) - dup
        pick = rng.choice(own, dup, replace=False)
        gq[own:], gkv[own:] = gq[pick], gkv[pick]
        assert bool((widx[own:] == -1).all())
        patches[-1] = (gq, gkv, widx)
        launch = Launch(patches)
        assert int(np.bincount(launch.gq).max()) == 2
    q, k, v, do = _f32_values(q, k, v, do)
    assert np.abs(q - torch.as_tensor(q).bfloat16().double().numpy()).max() > 0  # (not 16-bit values)
    return launch, (q, k, v, do)


def _torch_f32_grads(q, k, v, do, launch, H):
    """E_ref's subject: dense softmax attention per patch and head in torch, fp32 on the device, differentiated by autograd."""
    qd, kd, vd = (dev(a, F32).requires_grad_(True) for a in (q, k, v))
    dod = dev(do, F32)
    C = q.shape[1]
    loss = 0.0
    for gq, gkv, widx in launch.patches:
        L = len(gq)
        iq, ikv = dev(gq).long(), dev(gkv).long()
        qi, ki, vi = (t.view(L, H, 16).transpose(0, 1) for t in (qd[iq], kd[ikv], vd[ikv]))
        p = torch.softmax((qi @ ki.transpose(1, 2)) * SCALE, -1)
        o = (p @ vi).transpose(0, 1).reshape(L, C)
        live = dev(widx >= 0)
        loss = loss + (o * (dod[dev(np.where(widx >= 0, widx, 0)).long()] * live[:, None])).sum()
    loss.backward()
    return tuple(t.grad.cpu().double().numpy() for t in (qd, kd, vd))


def _attn_assert(name, got, ref32, exact, launch):
    for tn, g, gr, g64 in zip(("dq", "dk", "dv"), got, ref32, exact):
        assert np.isfinite(g).all() and np.isfinite(g64).all() and np.abs(g64).max() > 0, (name, tn)
        err, eref = _np_metric(g, g64), _np_metric(gr, g64)
        bound = 2 * eref + launch.max_len * U
        report(f"attn bwd fp32 {name} {tn}", kernel_err=err, E_ref=eref, bound=bound)
        assert err <= bound, (name, tn, err, eref, bound)


# (name, patch lengths, heads, padding duplicates, cross attention, packed views of one (n, 3C) buffer, also through _Attention)
ATTN = [("L700-H16", [700], 16, 0, False, True, False),
        ("L1024-300-H32-dups", [1024, 300], 32, 40, False, True, True),
        ("ragged-H16", [1, 15, 16, 17, 33], 16, 0, False, False, False),
        ("cross-H16", [512, 65], 16, 0, True, False, False)]


@pytest.mark.parametrize("name,lens,H,dup,cross,packed,core", ATTN, ids=[c[0] for c in ATTN])
def test_attention_bwd_fp32_at_deep_head_counts(ops, name, lens, H, dup, cross, packed, core):
    """ops.attention_bwd on fp32 tensors at 16 and 32 heads (C = 256 / 512).  cross: nkv = n + 50 rows, separate q and kv
    buffers.  core: once more through train_graph.attention_core(None, ...), i.e. _Attention's views of the packed qkv."""
    launch, (q, k, v, do) = _attn_case(lens, H, dup, cross, sum(lens) + 31 * H + dup)
    assert (k.shape[0] == q.shape[0] + 50) == cross
    exact = _grads(q, k, v, do, launch, H, F32, mode="noround")
    ref32 = _torch_f32_grads(q, k, v, do, launch, H)
    with ops.record_routes() as rr:
        got = _kernel(F32, q, k, v, do, launch, H, packed=packed, dtype=F32)
    _attn_assert(name, got, ref32, exact, launch)
    assert rr.count == 2 and rr.kernels() == ["attn_bwd_q_mfma_kernel<>", "attn_bwd_kv_mfma_kernel<>"], rr.routes
    assert all(r.splits == 1 and r.compute == ops.F32 for r in rr.routes), rr.routes  # (the fp32 form cuts no patch-head)
    if core:
        from cdsegnet_amd import train_graph
        C = 16 * H
        qkv = dev(np.concatenate([q, k, v], 1), F32).requires_grad_(True)
        gq, gkv, widx, ps = launch.device()
        out = train_graph.attention_core(None, qkv, None, C, gq, gkv, widx, ps, launch.ps.tolist(), H, launch.max_len, SCALE)
        assert out.dtype == F32 and out.shape == (q.shape[0], C)
        out.backward(dev(do, F32))
        _sync()
        g = qkv.grad.cpu().double().numpy()
        _attn_assert(name + " via _Attention", (g[:, :C], g[:, C:2 * C], g[:, 2 * C:]), ref32, exact, launch)


# ------------------------------------------------------------------------------------------ (f) the fp32 autograd functions
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "no-bias"])
def test_linear_function_exact_on_integers(ops, bias):
    """train_graph._Linear at fc1's shape: y, dx, dw, db equal the integer results; x without a gradient gets none."""
    from cdsegnet_amd.train_graph import _Linear
    M, K, N = 2103, 512, 2048
    rng = np.random.default_rng(N + bias)
    x, w, b, dy = _ints(rng, M, K), _ints(rng, N, K), _ints(rng, N), _ints(rng, M, N)
    _premise(max(M, K, N), x, w, b, dy)
    x64, w64, dy64 = x.cuda().double(), w.cuda().double(), dy.cuda().double()
    want_y = x64 @ w64.T + (b.cuda().double() if bias else 0.0)
    for x_grad in (True, False):
        xr, wr = x.cuda().requires_grad_(x_grad), w.cuda().requires_grad_(True)
        br = b.cuda().requires_grad_(True) if bias else None
        y = _Linear.apply(xr, wr, br)
        y.backward(dy.cuda())
        _sync()
        assert y.dtype == F32 and torch.equal(y.detach().double(), want_y)
        assert torch.equal(wr.grad.double(), dy64.T @ x64)
        if bias:
            assert torch.equal(br.grad.double(), dy64.sum(0))
        if x_grad:
            assert torch.equal(xr.grad.double(), dy64 @ w64)
        else:
            assert xr.grad is None


@pytest.mark.parametrize("cin,cout,ksize", [(128, 128, 3), (6, 32, 5)], ids=["128-128-k3", "stem-6-32-k5"])
def test_subm_conv_function_exact_on_integers(ops, cin, cout, ksize):
    """train_graph._SubMConv on `batch2` (two batch elements: the mirrored-map identity nbr[o][i] = j <=> nbr[kvol-1-o][j] = i,
    which the data gradient relies on, is exercised across a batch boundary): y, dx, dw5, db equal torch's fp64 autograd of
    the plain b + sum_o x[nbr[o]] W_o^T on integers.  The stem's 6 channels are padded to 16 inside; dw5 comes back unpadded."""
    from cdsegnet_amd.train_graph import _SubMConv
    nbr = _kernel_map(ops, "batch2", ksize)
    kvol, M = nbr.shape
    rng = np.random.default_rng(cin + cout + kvol)
    x, w5, b, dy = _ints(rng, M, cin), _ints(rng, cout, ksize, ksize, ksize, cin), _ints(rng, cout), _ints(rng, M, cout)
    assert 9 * kvol * max(cin, cout) < 2 ** 20 and 9 * M < 2 ** 20
    x64, w64, b64 = (t.cuda().double().requires_grad_(True) for t in (x, w5, b))
    w3 = w64.view(cout, kvol, cin)
    y64 = b64.expand(M, cout)
    for o in range(kvol):
        live = (nbr[o] >= 0).double()[:, None]
        y64 = y64 + (x64[nbr[o].clamp(min=0).long()] * live) @ w3[:, o, :].T
    y64.backward(dy.cuda().double())
    xr, wr, br = (t.cuda().requires_grad_(True) for t in (x, w5, b))
    y = _SubMConv.apply(xr, wr, br, nbr)
    y.backward(dy.cuda())
    _sync()
    assert y.dtype == F32 and torch.equal(y.detach().double(), y64.detach())
    assert xr.grad.shape == x.shape and torch.equal(xr.grad.double(), x64.grad)
    assert wr.grad.shape == w5.shape and torch.equal(wr.grad.double(), w64.grad)
    assert torch.equal(br.grad.double(), b64.grad)
    assert float(x64.grad.abs().max()) > 0 and float(w64.grad.abs().max()) > 0


def test_layernorm_function_vs_fp64_within_three_times_torch(ops):
    """train_graph._LayerNorm at C = 512: y, dx, dgamma, dbeta against fp64 F.layer_norm under the bound of the kernel test."""
    from cdsegnet_amd.train_graph import _LayerNorm
    M, C = 777, 512
    const = _const_rows(M)
    rest = [r for r in range(M) if r not in set(const)]
    x, gamma, dy, pre = _ln_inputs(M, C, const, 5)
    beta = pre["db"]
    o64, t32 = _ln_autograd(x, gamma, dy, torch.float64), _ln_autograd(x, gamma, dy, F32)
    xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = _LayerNorm.apply(xr, gr, br, EPS)
    y.backward(dy)
    _sync()
    y64, yt = o64[0] + beta.double(), t32[0] + beta
    _assert_vs_torch("_LayerNorm (777, 512)", [("y", y.detach(), yt, y64, None), ("dx", xr.grad, t32[1], o64[1], rest),
                                               ("dx (constant rows)", xr.grad, t32[1], o64[1], const),
                                               ("dgamma", gr.grad, t32[2], o64[2], None), ("dbeta", br.grad, t32[3], o64[3], None)])


def test_segment_max_function_sends_the_gradient_to_the_first_maximum(ops):
    """train_graph._SegmentMax on the device at C = 512: values from {-2 .. 2} (ties in most segments and channels), one
    segment of eight equal rows, one-child segments.  Forward and gradient compared exactly with a loop over the segments:
    the gradient goes to the FIRST child that holds the maximum and to no other."""
    from cdsegnet_amd.train_graph import _SegmentMax
    rng = np.random.default_rng(8)
    C = 512
    lens = np.concatenate([[1, 8, 1, 3], rng.integers(1, 9, 300), [1]])
    m, n = len(lens), int(lens.sum())
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    cluster = np.repeat(np.arange(m), lens).astype(np.int32)
    y = rng.integers(-2, 3, (n, C)).astype(np.float32)
    y[seg[1]:seg[2]] = 1.0  # a whole segment of equal values
    dout = rng.standard_normal((m, C)).astype(np.float32)
    want_out, want_grad = np.empty((m, C), np.float32), np.zeros((n, C), np.float32)
    cols = np.arange(C)
    ties = 0
    for j in range(m):
        a, b = seg[j], seg[j + 1]
        first = y[a:b].argmax(0)  # (numpy: the first occurrence)
        want_out[j] = y[a + first, cols]
        want_grad[a + first, cols] = dout[j]
        ties += int(((y[a:b] == want_out[j]).sum(0) > 1).sum())
    assert ties > m * C // 4 and int((lens == 1).sum()) >= 3
    yr = dev(y).requires_grad_(True)
    out = _SegmentMax.apply(yr, dev(seg), dev(cluster), m)
    out.backward(dev(dout))
    _sync()
    assert np.array_equal(out.detach().cpu().numpy(), want_out)
    assert np.array_equal(yr.grad.cpu().numpy(), want_grad)
