"""GPU: the deterministic training mode (`DefaultSegmentorV2.train_deterministic`; csrc/train.hip `_det` kernels), both builds
of the library where 16-bit operands are involved.

What is checked, in this order: the deterministic weight gradient is EXACT on integers (any order is exact there: this pins
indexing, the workspace layout and the accumulate-into contract); its summation ORDER is the documented one (an input whose
fp32 sum is 1.0 in that order and 0.0 / 2.0 in others, built from ops.wgrad_partition); results are bit-REPEATABLE; it is as
ACCURATE as the default kernel (the yardstick is the unchanged default kernel's own error against fp64, margin 3 as in
tests/test_gpu_wgrad16.py: the same products in another order); the WHOLE STEP and three AdamW steps are bit-reproducible.

Every figure is printed with report(...) before it is asserted; profiles/NOTES.md ("Deterministic training") is where they are kept.
"""
import numpy as np
import pytest
import torch

from tests.helpers import load_fixture
from tests.test_gpu_ops import LP, _library_variant, _physical, dev, ops, report  # noqa: F401  (fixtures: lp="f16" -> the half build)
from tests.test_gpu_wgrad16 import _eq, _exact, _ints, _kernel_map, _metric

pytestmark = pytest.mark.gpu

# operand types: "fp32", or the 16-bit type of the bfloat16 / the half build
KINDS = pytest.mark.parametrize("lp", ["fp32", "bf16", "f16"])


def _t(lp):
    return torch.float32 if lp == "fp32" else LP()


def _splits(ops, m, n, k, kvol, t):
    return ops.wgrad_partition(m, n, k, kvol, t)


# ------------------------------------------------------------------------------------------ exact on integers
DENSE = [("fp32", 4100, 32, 96), ("bf16", 2100, 32, 96), ("f16", 2100, 32, 96), ("bf16", 5003, 64, 192), ("f16", 5003, 64, 192)]


@pytest.mark.parametrize("lp,M,K,N", DENSE, ids=[f"{a}-{m}x{k}x{n}" for a, m, k, n in DENSE])
def test_dense_and_gathered_exact_on_integers(ops, lp, M, K, N):
    """Dense form on strided views into a pre-filled dw / db (adding twice gives twice the sum), then the gathered form with
    -1 entries, repeated rows and a dead stretch that covers whole chunks of one split."""
    t = _t(lp)
    part = _splits(ops, M, N, K, 1, t)
    assert part.splits >= 3, tuple(part)  # (fewer: nothing order-dependent would be exercised)
    rng = np.random.default_rng(M + 7 * K + 13 * N)
    x, dy = _ints(rng, M, K), _ints(rng, M, N)
    want_w, want_b = _exact(dy, x)
    xw, dyw = dev(_ints(rng, M, K + 24), t), dev(_ints(rng, M, N + 16), t)
    xw[:, 8:8 + K] = dev(x, t)
    dyw[:, 16:] = dev(dy, t)
    pre_w, pre_b = _ints(rng, N, K + 12) * 5, _ints(rng, N) * 7
    wide, db = pre_w.cuda().clone(), pre_b.cuda().clone()
    ops.linear_wgrad(xw[:, 8:8 + K], dyw[:, 16:], wide[:, 4:4 + K], db, deterministic=True)
    torch.cuda.synchronize()
    assert _eq(wide[:, 4:4 + K], pre_w[:, 4:4 + K].long() + want_w) and _eq(db, pre_b.long() + want_b)
    ops.linear_wgrad(xw[:, 8:8 + K], dyw[:, 16:], wide[:, 4:4 + K], db, deterministic=True)
    torch.cuda.synchronize()
    assert _eq(wide[:, 4:4 + K], pre_w[:, 4:4 + K].long() + 2 * want_w) and _eq(db, pre_b.long() + 2 * want_b)
    assert torch.equal(wide[:, :4].cpu(), pre_w[:, :4]) and torch.equal(wide[:, 4 + K:].cpu(), pre_w[:, 4 + K:])
    # gathered
    R = M // 2
    xs = _ints(rng, R, K)
    idx = rng.integers(0, R, size=M)
    idx[rng.random(M) < 0.3] = -1
    idx[5:9] = idx[4]
    a = part.rows_per_split  # split 1 starts dead: 200 rows without a neighbour
    idx[a:a + 200] = -1
    idx = torch.as_tensor(idx, dtype=torch.int32)
    want_w, want_b = _exact(dy, xs, idx)
    dw, db = torch.zeros(N, K, device="cuda"), torch.zeros(N, device="cuda")
    dw_nob = torch.zeros(N, K, device="cuda")
    ops.linear_wgrad(dev(xs, t), dev(dy, t), dw, db, xidx=idx.cuda(), deterministic=True)
    ops.linear_wgrad(dev(xs, t), dev(dy, t), dw_nob, None, xidx=idx.cuda(), deterministic=True)
    torch.cuda.synchronize()
    assert _eq(dw, want_w) and _eq(db, want_b) and _eq(dw_nob, want_w)


@KINDS
@pytest.mark.parametrize("cin,cout,ksize", [(32, 32, 3), (16, 32, 5)], ids=["32-32-k3", "stem-16-32-k5"])
def test_conv_form_exact_on_integers(ops, lp, cin, cout, ksize):
    """All kernel offsets of the `batch2` fixture's map in one launch, into a pre-filled dw3 / db.  A split all of whose rows
    lack the offset's neighbour stores zeros (edge offsets of the stem have such splits)."""
    t = _t(lp)
    nbr = _kernel_map(ops, "batch2", ksize)
    kvol, M = nbr.shape
    assert _splits(ops, M, cout, cin, kvol, t).splits >= 3
    rng = np.random.default_rng(cin + cout + kvol)
    x, dy = _ints(rng, M, cin), _ints(rng, M, cout)
    if ksize == 5:
        x[:, 6:] = 0
    pre_w, pre_b = _ints(rng, cout, kvol, cin) * 3, _ints(rng, cout) * 7
    dw3, db = pre_w.cuda().clone(), pre_b.cuda().clone()
    ops.conv_wgrad(dev(x, t), nbr, dev(dy, t), dw3, db, deterministic=True)
    torch.cuda.synchronize()
    nb = nbr.cpu()
    for o in range(kvol):
        assert _eq(dw3[:, o, :], pre_w[:, o, :].long() + _exact(dy, x, nb[o])[0]), o
    assert _eq(db, pre_b.long() + dy.double().sum(0).long())


# ------------------------------------------------------------------------------------------ the order is the documented one
def _order_input(part, M, K, N, big_dy, big_x):
    """One live row per split 0 .. 3 with products big, 1, -big, 1 in every (n, k); zeros elsewhere."""
    x, dy = torch.zeros(M, K), torch.zeros(M, N)
    r = part.rows_per_split
    rows = [0 * r + 5, 1 * r + 1, 2 * r + 70, min(M - 1, 3 * r + 3)]
    assert all(s * r <= rows[s] < min(M, (s + 1) * r) for s in range(4))
    for s, (a, b) in enumerate([(big_dy, big_x), (1.0, 1.0), (-big_dy, big_x), (1.0, 1.0)]):
        dy[rows[s]], x[rows[s]] = a, b
    return x, dy


@KINDS
@pytest.mark.parametrize("form", ["linear", "conv"])
def test_summation_order_is_ascending_split_index(ops, lp, form):
    """dy = +-2^12, x = 2^12 and dy = x = 1 (exact in half and bfloat16): products 2^24, 1, -2^24, 1 in splits 0 .. 3.  In
    fp32 (2^24 + 1) - 2^24 + 1 = 1.0 in the documented order only (tests/test_cpu_deterministic.py replays it in numpy; other
    orders give 0.0 or 2.0), so dw must be exactly 1.0 everywhere - and exactly 6.0 on a dw pre-filled with 5.0: the total is
    added ONCE onto the existing content.

    db: a column sum of those dy values is 2^12 + 1 - 2^12 + 1 = 2.0 in every order, so that run checks db == 2.0 as an
    indexing check only.  The ORDER of db is pinned by a second input on which a split's db partial is a sum over all its
    rows: every row of split 0 holds dy = 2^24 / rows_per_split (2^15 at 512 rows, 2^14 at 1024: exact in half and
    bfloat16, every running sum a multiple of it below 2^24 + 1, so exact), split 2 the negative, splits 1 and 3 one row
    with dy = 1, x = 0 everywhere: db partials 2^24, 1, -2^24, 1 -> db == 1.0 in ascending split order (0.0 or 2.0 in others),
    6.0 onto a pre-filled 5.0, for fp32 and for both 16-bit builds; dw stays what it was."""
    t = _t(lp)
    M, K, N = (4096 if lp == "fp32" else 2048), 32, 96  # four splits of 1024 / 512 rows in either form
    kvol = 1 if form == "linear" else 27
    part = _splits(ops, M, N, K, kvol, t)
    assert part.splits == 4 and 4 * part.rows_per_split == M, tuple(part)

    def launch(x, dy, fill):
        db = torch.full((N,), fill, device="cuda")
        if form == "linear":
            dw = torch.full((N, K), fill, device="cuda")
            ops.linear_wgrad(dev(x, t), dev(dy, t), dw, db, deterministic=True)
        else:  # every offset reads the row itself: 27 copies of the linear problem
            nbr = torch.arange(M, dtype=torch.int32, device="cuda").repeat(27, 1).contiguous()
            dw = torch.full((N, 27, K), fill, device="cuda")
            ops.conv_wgrad(dev(x, t), nbr, dev(dy, t), dw, db, deterministic=True)
        torch.cuda.synchronize()
        return dw.cpu(), db.cpu()

    r = part.rows_per_split
    per_row = 2.0 ** 24 / r
    assert per_row * r == 2.0 ** 24 and float(torch.tensor(per_row).to(t)) == per_row
    for fill in (0.0, 5.0):
        dw, db = launch(*_order_input(part, M, K, N, 2.0 ** 12, 2.0 ** 12), fill)
        report(f"order input {form} ({lp}) fill={fill}", dw_min=float(dw.min()), dw_max=float(dw.max()), db_min=float(db.min()),
               db_max=float(db.max()))
        assert bool((dw == fill + 1.0).all()), (float(dw.min()), float(dw.max()))
        assert bool((db == fill + 2.0).all()), (float(db.min()), float(db.max()))  # (indexing only: 2.0 in every order)
        dy = torch.zeros(M, N)
        dy[0:r], dy[2 * r:3 * r] = per_row, -per_row
        dy[r + 1], dy[3 * r + 3] = 1.0, 1.0
        dw, db = launch(torch.zeros(M, K), dy, fill)
        report(f"db order input {form} ({lp}) fill={fill}", db_min=float(db.min()), db_max=float(db.max()))
        assert bool((db == fill + 1.0).all()), (float(db.min()), float(db.max()))
        assert bool((dw == fill).all())


def test_layernorm_block_order_is_ascending(ops):
    """The same construction over LayerNorm's 64-row blocks: column entries 2^24, 1, -2^24, 1 of dy in blocks 0 .. 3 (one live
    row each) and zeros elsewhere -> dbeta is exactly 1.0, and 6.0 on a dbeta pre-filled with 5.0.  (dgamma multiplies by the
    normalised input, which is not exact: its order is the same code path.)"""
    m, c = 4 * 64 + 9, 48  # a fifth, partial block of zeros
    g = torch.Generator().manual_seed(1)
    x, gamma = torch.randn(m, c, generator=g), torch.randn(c, generator=g)
    dy = torch.zeros(m, c)
    for row, v in ((3, 2.0 ** 24), (64 + 17, 1.0), (128 + 63, -2.0 ** 24), (192 + 32, 1.0)):
        dy[row] = v
    for fill in (0.0, 5.0):
        dx = torch.empty(m, c, device="cuda")
        dg, db = torch.zeros(c, device="cuda"), torch.full((c,), fill, device="cuda")
        ops.layernorm_bwd(x.cuda(), gamma.cuda(), dy.cuda(), dx, dgamma=dg, dbeta=db, deterministic=True)
        torch.cuda.synchronize()
        assert bool((db.cpu() == fill + 1.0).all()), db.cpu()
        assert bool(torch.isfinite(dg).all()) and bool(torch.isfinite(dx).all())


# ------------------------------------------------------------------------------------------ repeatable
def _four_equal(fn):
    first = fn()
    for _ in range(3):
        again = fn()
        for a, b in zip(first, again):
            assert torch.equal(a, b)
    return first


@KINDS
def test_wgrad_is_bit_repeatable_on_gaussian_data(ops, lp):
    t = _t(lp)
    M, K, N = 20000, 64, 192
    assert _splits(ops, M, N, K, 1, t).splits >= 3
    g = torch.Generator().manual_seed(5)
    x, dy = dev(torch.randn(M, K, generator=g), t), dev(0.1 * torch.randn(M, N, generator=g), t)
    nbr = _kernel_map(ops, "batch2", 3)
    xc, dyc = dev(torch.randn(nbr.shape[1], 32, generator=g), t), dev(torch.randn(nbr.shape[1], 32, generator=g), t)

    def run():
        dw, db = torch.zeros(N, K, device="cuda"), torch.zeros(N, device="cuda")
        ops.linear_wgrad(x, dy, dw, db, deterministic=True)
        dw3, db3 = torch.zeros(32, 27, 32, device="cuda"), torch.zeros(32, device="cuda")
        ops.conv_wgrad(xc, nbr, dyc, dw3, db3, deterministic=True)
        torch.cuda.synchronize()
        return dw, db, dw3, db3

    _four_equal(run)


@pytest.mark.parametrize("m,c", [(200, 16), (5000, 32), (3000, 512)])
def test_layernorm_bwd_is_bit_repeatable_and_matches_torch(ops, m, c):
    g = torch.Generator().manual_seed(m + c)
    x, gamma, dy = torch.randn(m, c, generator=g), torch.randn(c, generator=g), torch.randn(m, c, generator=g)
    xd, gd, dyd = x.cuda(), gamma.cuda(), dy.cuda()

    def run(**kw):
        dx = torch.empty(m, c, device="cuda")
        dg, db = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda")
        ops.layernorm_bwd(xd, gd, dyd, dx, dgamma=dg, dbeta=db, **kw)
        torch.cuda.synchronize()
        return dx, dg, db

    dx, dg, db = _four_equal(lambda: run(deterministic=True))
    dx0, dg0, db0 = run()
    assert torch.equal(dx, dx0)  # dx is the default form's
    xr, gr, br = x.double().requires_grad_(True), gamma.double().requires_grad_(True), torch.zeros(c, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.layer_norm(xr, (c,), gr, br, 1e-5).backward(dy.double())
    e_det = (_metric(dg, gr.grad), _metric(db, br.grad))
    e_def = (_metric(dg0, gr.grad), _metric(db0, br.grad))
    report(f"layernorm_bwd det ({m}, {c})", det_dgamma=e_det[0], default_dgamma=e_def[0], det_dbeta=e_det[1], default_dbeta=e_def[1])
    # Same per-block partial sums, another order of adding the <= m / 64 of them: 3 x the default form's own error, the
    # margin of the weight-gradient test.  Plus 2^-24: any fp32 result carries up to half an ulp of its own final rounding
    # (<= 2^-24 of the largest element in this metric), a term that does not shrink with the default form's realised error -
    # which is a maximum over only c columns (16 at the smallest shape) and can come out below half an ulp by chance.
    assert e_det[0] <= 3 * e_def[0] + 2.0 ** -24 and e_det[1] <= 3 * e_def[1] + 2.0 ** -24


def test_segment_sum_on_the_pooling_link(ops):
    """out[j] = the sum of the contiguous children of pooled row j (`room1500`, one pooling step): exact on integers against
    index_add, a strided source, every lane layout (c = 16, 32, 48, 96, 512), repeatable on Gaussian data and within fp32
    round-off of fp64."""
    fx = load_fixture("serialization_room1500.npz")
    zs = _physical(ops, fx)[0]
    cluster, seg, cnt = ops.pool_level(zs, 3)
    m, n = int(cnt.item()), zs.numel()
    cl = cluster.long().cpu()
    assert int(seg[m].item()) == n and bool((cl[1:] >= cl[:-1]).all())  # children are contiguous
    rng = np.random.default_rng(0)
    for c in (16, 32, 48, 96, 512):
        src = _ints(rng, n, c + 8)
        want = torch.zeros(m, c).index_add_(0, cl, src[:, 4:4 + c])
        got = ops.segment_sum(src.cuda()[:, 4:4 + c], seg, m)
        torch.cuda.synchronize()
        assert got.shape == (m, c) and torch.equal(got.cpu(), want), c
    g = torch.Generator().manual_seed(2)
    src = torch.randn(n, 64, generator=g)
    sd = src.cuda()
    (out,) = _four_equal(lambda: (ops.segment_sum(sd, seg, m),))
    want = torch.zeros(m, 64, dtype=torch.float64).index_add_(0, cl, src.double())
    # at most eight children per pooled row: seven fp32 adds, each within 2^-24 of a partial sum <= the run's sum of |src|
    mass = torch.zeros(m, 64, dtype=torch.float64).index_add_(0, cl, src.double().abs())
    assert int(torch.bincount(cl).max()) <= 8
    assert _metric(out, want) <= 7 * 2.0 ** -24 * float(mass.max()) / float(want.abs().max())


def test_gather_runs_backward_is_the_segment_sum(ops):
    """The autograd function of the deterministic unpooling gather and of the Mix3D fold: forward x[idx], backward the sum
    over each run - with and without the stable sort (`fold_runs`: rep in arbitrary order)."""
    from cdsegnet_amd.train_graph import _GatherRuns, fold_runs
    rng = np.random.default_rng(3)
    m, n, c = 700, 1900, 32
    rep = torch.as_tensor(np.concatenate([np.arange(m), rng.integers(0, m, n - m)])).cuda()  # every row at least once
    x = _ints(rng, m, c).cuda().requires_grad_(True)
    dy = _ints(rng, n, c).cuda()
    perm, seg = fold_runs(rep, m)
    y = _GatherRuns.apply(x, rep, seg, perm)
    assert torch.equal(y, x.detach()[rep])
    y.backward(dy)
    want = torch.zeros(m, c).index_add_(0, rep.cpu(), dy.cpu())
    assert torch.equal(x.grad.cpu(), want)
    srt = torch.sort(rep).values  # already contiguous runs: no permutation
    x.grad = None
    _GatherRuns.apply(x, srt, seg, None).backward(dy)
    assert torch.equal(x.grad.cpu(), torch.zeros(m, c).index_add_(0, srt.cpu(), dy.cpu()))


@pytest.mark.parametrize("lp", ["fp32", "bf16", "f16"])
@pytest.mark.parametrize("name", ["dups", "cross"])
def test_attention_bwd_is_bit_repeatable_as_it_is(ops, lp, name):
    """ops.attention_bwd UNCHANGED: every (slot, head, dim) result leaves with one atomic and a row sits in at most two slots
    (the padding plan copies the tail of the previous patch once), so an element of the zeroed dq / dk / dv receives at most
    two adds, which commute.  `dups` and `cross` of tests/test_gpu_attention_bwd16.py (lengths, heads, number of duplicates,
    values): padding duplicates, and launches small enough for the 16-bit form's 4-way blockIdx.z split.  If this fails on a device the fix is a per-row reduce in slot
    order, not a tolerance."""
    from tests import test_gpu_attention_bwd16 as A
    case = {c[0]: c for c in A.CASES}[name]
    _, lens, H, dup, cross, packed, sigma_k = case
    lpt = LP()
    rng = np.random.default_rng(sum(lens) + 31 * H + dup)
    launch, (q16, k16, v16, do16) = A._case(lens, H, dup, cross, lpt, rng, sigma_k)
    # that helper draws the last patch's padding duplicates WITH replacement, so a few rows sit in three slots - one more than
    # the padding plan ever produces and than the argument covers: same case, duplicates redrawn without replacement
    patches = list(launch.patches)
    gq, gkv, widx = (a.copy() for a in patches[-1])
    own = len(gq) - dup
    pick = rng.choice(own, dup, replace=False)
    gq[own:], gkv[own:] = gq[pick], gkv[pick]
    assert bool((widx[own:] == -1).all())
    patches[-1] = (gq, gkv, widx)
    launch = A.Launch(patches)
    mult = max(int(np.bincount(np.concatenate([p[i] for p in launch.patches])).max()) for i in (0, 1))
    assert mult == 2  # the premise: some rows sit in two slots, none in three
    dtype = torch.float32 if lp == "fp32" else None
    first = A._kernel(lpt, q16, k16, v16, do16, launch, H, packed=packed, dtype=dtype)
    assert all(np.isfinite(g).all() and np.abs(g).max() > 0 for g in first)
    for _ in range(3):
        again = A._kernel(lpt, q16, k16, v16, do16, launch, H, packed=packed, dtype=dtype)
        for tn, a, b in zip(("dq", "dk", "dv"), first, again):
            assert np.array_equal(a, b), tn


# ------------------------------------------------------------------------------------------ accurate
@KINDS
@pytest.mark.parametrize("M,K,N", [(20000, 64, 192), (6000, 512, 512)])
def test_accuracy_against_the_default_kernel(ops, lp, M, K, N):
    """Gaussian x, dy = 0.1 N(0, 1) rounded to the operand type; oracle fp64 on the rounded values; metric max |g - g64| /
    max |g64|.  Bound: 3 x the error of the UNCHANGED default kernel on the same values (same products, other order of the
    fp32 sums - the margin tests/test_gpu_wgrad16.py uses for that)."""
    t = _t(lp)
    assert _splits(ops, M, N, K, 1, t).splits >= 3
    g = torch.Generator().manual_seed(M + K)
    x16, dy16 = torch.randn(M, K, generator=g).to(t), (0.1 * torch.randn(M, N, generator=g)).to(t)
    w64, b64 = dy16.double().T @ x16.double(), dy16.double().sum(0)
    out = {}
    for mode in (False, True):
        dw, db = torch.zeros(N, K, device="cuda"), torch.zeros(N, device="cuda")
        ops.linear_wgrad(x16.cuda(), dy16.cuda(), dw, db, **({"deterministic": True} if mode else {}))
        torch.cuda.synchronize()
        out[mode] = (_metric(dw, w64), _metric(db, b64))
    (e0w, e0b), (e1w, e1b) = out[False], out[True]
    report(f"wgrad det {M}x{K}x{N} ({lp})", default_dw=e0w, det_dw=e1w, default_db=e0b, det_db=e1b)
    assert e1w <= 3 * e0w, (e1w, e0w)
    assert e1b <= 3 * e0b, (e1b, e0b)


# ------------------------------------------------------------------------------------------ the whole step
_SCENES = {}


def _batch():
    """Two synthetic rooms of about 4 000 points each (built once, never modified): level 0 has >= 3 splits in both forms."""
    if not _SCENES:
        from cdsegnet_amd import synth
        sc = synth.collate([synth.room_scene(11, 4000), synth.room_scene(12, 4100)])
        inp = {k: torch.as_tensor(sc[k]).cuda() for k in ("coord", "grid_coord", "feat", "offset")}
        inp["segment"] = (torch.as_tensor(np.asarray(sc["segment"]).astype(np.int64)) % 13).cuda()
        n = inp["feat"].shape[0]
        g = torch.Generator().manual_seed(21)
        draws = dict(ts=torch.randint(0, 1000, (2, 1), generator=g), noise=torch.randn(n, 6, generator=g),
                     perms=[torch.randperm(4, generator=g).tolist() for _ in range(8)])
        _SCENES["inp"], _SCENES["draws"], _SCENES["n"] = inp, draws, n
    return _SCENES["inp"], dict(_SCENES["draws"]), _SCENES["n"]


def _model(tp, det):
    from tests.test_gpu_attention_bwd16 import _mini_model
    fx = load_fixture("train_step_mini.npz")
    model, sd = _mini_model(fx, torch.device("cuda"), True)
    model.train_precision = tp
    model.train_deterministic = det
    return model


def _step(model, inp, draws, seed=3):
    """Forward + backward with fixed draws; the stochastic-depth masks come from the seeded device generator."""
    model.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    out = model(inp, draws=draws)
    out["loss"].backward()
    torch.cuda.synchronize()
    return out["loss"].detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("tp", ["fp32", "fp16-amp", "bf16-amp"])
def test_whole_step_is_bit_reproducible(ops, tp):
    """Two forward + backward passes in the deterministic mode: bit-equal loss and bit-equal .grad of every parameter; the
    loss is bit-equal to the default mode's (the forward is untouched); the default mode's gradients are reported next to it
    (how many tensors differ between two default passes: the non-determinism the mode removes, when the device shows it)."""
    inp, draws, n = _batch()
    assert ops.wgrad_partition(n, 48, 16, 1, torch.float32).splits >= 3 and ops.wgrad_partition(n, 48, 16, 1, torch.bfloat16).splits >= 3
    model = _model(tp, True)
    model.train(True)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}  # (BatchNorm buffers move with every forward)

    def run(det):
        model.load_state_dict(state)
        model.train_precision, model.train_deterministic = tp, det
        return _step(model, inp, draws)

    l1, g1 = run(True)
    l2, g2 = run(True)
    assert bool(torch.isfinite(l1)) and torch.equal(l1, l2)
    assert set(g1) == set(g2) and len(g1) > 400
    diff = [k for k in g1 if not torch.equal(g1[k], g2[k])]
    assert not diff, diff[:8]
    l0, g0 = run(False)
    l0b, g0b = run(False)
    assert torch.equal(l0, l1) and torch.equal(l0, l0b)
    assert set(g0) == set(g1)
    # (biases in front of a BatchNorm have a zero gradient up to rounding: measured against the largest gradient as well,
    # like the gradient norms in tests/test_gpu_train.py)
    top = max(float(g.abs().max()) for g in g0.values())
    worst = max(float((g0[k] - g1[k]).abs().max()) / (float(g0[k].abs().max()) + 1e-3 * top) for k in g0)
    report(f"whole step {tp}: deterministic vs default", loss=float(l1), tensors=len(g1),
           default_tensors_differing_between_two_runs=sum(not torch.equal(g0[k], g0b[k]) for k in g0),
           worst_rel_diff_det_vs_default=worst)
    assert worst < 1e-3  # (sanity: the same gradients up to summation order)


def test_mix3d_batch_with_shared_voxels_is_bit_reproducible(ops, monkeypatch):
    """Two rooms merged into one batch element (Mix3D: both grids start at 0, voxels coincide) and a third on its own: the
    training forward folds the surplus points onto their voxel's first point, and in the deterministic mode the fold's
    gradient is a segment sum after a stable sort of rep.  Two passes: bit-equal loss and gradients; the fold did go
    through ops.segment_sum (a call whose output has one row per kept voxel)."""
    import warnings
    from cdsegnet_amd import ops as O
    from cdsegnet_amd import synth
    from cdsegnet_amd.train_graph import voxel_representatives
    a, b, c = (synth.room_scene(s, 1500, num_classes=13) for s in (1, 2, 3))
    cat = lambda k: np.concatenate([a[k], b[k], c[k]])  # noqa: E731
    na, nb, nc = len(a["coord"]), len(b["coord"]), len(c["coord"])
    inp = {k: torch.as_tensor(cat(k)).cuda() for k in ("coord", "grid_coord", "feat")}
    inp["segment"] = torch.as_tensor(cat("segment").astype(np.int64)).cuda()
    inp["offset"] = torch.as_tensor(np.array([na + nb, na + nb + nc])).cuda()
    n = na + nb + nc
    keep, rep, _ = voxel_representatives(inp["grid_coord"], inp["offset"])
    assert 0 < len(keep) < n, "the two merged rooms must share voxels"
    g = torch.Generator().manual_seed(8)
    draws = dict(ts=torch.randint(0, 1000, (2, 1), generator=g), noise=torch.randn(n, 6, generator=g),
                 perms=[torch.randperm(4, generator=g).tolist() for _ in range(8)])
    folds = []
    seg_sum = O.segment_sum

    def counted(src, seg, m):
        folds.append(int(m))
        return seg_sum(src, seg, m)

    monkeypatch.setattr(O, "segment_sum", counted)
    model = _model("fp32", True)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    runs = []
    for _ in range(2):
        model.load_state_dict(state)
        model.train_deterministic = True
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # ("... points in already occupied voxels (Mix3D): folded ...")
            runs.append(_step(model, inp, dict(draws)))
    (l1, g1), (l2, g2) = runs
    assert folds.count(len(keep)) >= 2 * 2, folds  # n_pred and c_pred, two passes
    assert bool(torch.isfinite(l1)) and torch.equal(l1, l2)
    diff = [k for k in g1 if not torch.equal(g1[k], g2[k])]
    assert len(g1) > 400 and set(g1) == set(g2) and not diff, diff[:8]


def test_recorded_step_in_the_deterministic_mode_meets_the_reference_bound(ops, monkeypatch):
    """tests/test_gpu_train.py's comparison against the reference's recorded step (`train_step_mini.npz`, padded plan, fp32),
    run as it is on a model with train_deterministic = True: the same assertions, the same bounds."""
    from cdsegnet_amd import ops as O
    from tests import test_gpu_train as T
    build = T._mini_training_model
    calls = {"det": 0, "default": 0}
    wgrad, ln = O.linear_wgrad, O.layernorm_bwd

    def counted(fn):
        def f(*a, **kw):
            calls["det" if kw.get("deterministic") else "default"] += 1
            return fn(*a, **kw)
        return f

    def det_model(fx, dev_):
        model, sd = build(fx, dev_)
        model.train_deterministic = True
        return model, sd

    monkeypatch.setattr(T, "_mini_training_model", det_model)
    monkeypatch.setattr(O, "linear_wgrad", counted(wgrad))
    monkeypatch.setattr(O, "layernorm_bwd", counted(ln))
    T.test_whole_training_step_matches_the_reference_train_step()
    assert calls["det"] > 100 and calls["default"] == 0, calls


# ------------------------------------------------------------------------------------------ training
def _train_three_steps(det, seed):
    inp, _, n = _batch()
    model = _model("fp32", det)
    named = dict(model.named_parameters())
    opt = torch.optim.AdamW([dict(params=[p for k, p in named.items() if "block" not in k], lr=0.002),
                             dict(params=[p for k, p in named.items() if "block" in k], lr=0.0002)], lr=0.002, weight_decay=0.05)
    torch.manual_seed(seed)
    losses = []
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        loss = model(inp)["loss"]  # random draws: timesteps, noise, shuffles (CPU generator), masks (device generator)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    torch.cuda.synchronize()
    return losses, {k: v.detach().clone() for k, v in model.state_dict().items()}


def _assert_same_run(a, b):
    (la, sa), (lb, sb) = a, b
    assert la == lb and np.isfinite(la).all(), (la, lb)
    diff = [k for k in sa if not torch.equal(sa[k], sb[k])]
    assert not diff, diff[:8]


def test_three_adamw_steps_twice_give_the_same_parameters(ops):
    """The same state_dict, the same torch.manual_seed, three AdamW steps on random draws, twice: bit-equal parameters and
    buffers (train_deterministic = True)."""
    a = _train_three_steps(True, 54421566)
    b = _train_three_steps(True, 54421566)
    _assert_same_run(a, b)
    report("three AdamW steps, deterministic", l0=a[0][0], l1=a[0][1], l2=a[0][2])


def test_the_mode_is_picked_up_from_torch(ops, monkeypatch):
    """train_deterministic = None under torch.use_deterministic_algorithms(True, warn_only=True): the deterministic entry
    points run (counted), and the two runs are bit-equal."""
    from cdsegnet_amd import ops as O
    calls = {"det": 0, "default": 0}
    wgrad = O.linear_wgrad

    def counted(*a, **kw):
        calls["det" if kw.get("deterministic") else "default"] += 1
        return wgrad(*a, **kw)

    monkeypatch.setattr(O, "linear_wgrad", counted)
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        torch.use_deterministic_algorithms(True, warn_only=True)
        a = _train_three_steps(None, 7)
        b = _train_three_steps(None, 7)
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn)
    assert calls["det"] > 100 and calls["default"] == 0, calls
    _assert_same_run(a, b)
    calls["det"] = 0
    _train_three_steps(None, 7)  # the flag is off again: the default kernels
    assert calls["det"] == 0 and calls["default"] > 100, calls
