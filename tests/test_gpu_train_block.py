"""GPU: the native training Block (`DefaultSegmentorV2.train_block = "native"`; csrc/trainblock.hip), through the C ABI, both
builds of the library where 16 bit is involved.

In this order: (1) the glue kernels that replace torch device ops are BIT-EXACT against the torch expressions (residual,
scale / cast without saturation, the derived weights); (2) GELU forward / backward and add_layernorm against fp64 with torch's
own fp32 error on the same values as the yardstick (3 E_torch + 2^-24, the form of tests/test_gpu_train_fp32.py); (3) one whole
Block, forward and backward, against fp64 torch autograd on the oracle restatement with the AUTOGRAD mode's own error on the
same inputs as the yardstick (3 E_auto + 2^-24); (4) the recorded reference step and a two-room step against the autograd
mode; (5) determinism; (6) GradScaler overflow; (7) structure (one call per Block, prepare once per weight version).

Every figure is printed with report(...) before it is asserted; profiles/NOTES.md ("Native training Block") keeps them.
"""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cdsegnet_amd import ops as O
from cdsegnet_amd import train_graph as TG
from tests.helpers import load_fixture
from tests.test_gpu_attention_bwd16 import _draws, _inp, _mini_model
from tests.test_gpu_ops import LP, _library_variant, dev, ops, report  # noqa: F401  (fixtures: lp="f16" -> the half build)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
LPS = pytest.mark.parametrize("lp", ["bf16", "f16"])
ROWS = (1, 63, 64, 65, 777)
WIDTHS = (32, 64, 512)


def _sync():
    torch.cuda.synchronize()


def _err(g, g64):
    top = float(g64.abs().max())
    assert top > 0
    return float((g.double().cpu() - g64.double().cpu()).abs().max()) / top


def _bits(a, b):
    """Bit equality (NaNs and signed zeros included)."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _bits_nan(a, b):
    """Bit equality everywhere except that a NaN may differ from a NaN in sign / payload (0 * inf, NaN * m: which NaN a
    product returns is not part of any contract, and torch's cast canonicalises it)."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool((na == nb).all()) and _bits(torch.where(na, torch.zeros_like(a), a), torch.where(nb, torch.zeros_like(b), b))


def _mask(n, g, zero_rows=True):
    """A stochastic-depth row mask already divided by the keep probability 0.7, with dropped (zero) rows."""
    m = (torch.rand(n, generator=g) < 0.7).float() / 0.7
    if zero_rows and n > 1:
        m[n // 2] = 0.0
    return m


# ------------------------------------------------------------------------------------------ (1) glue kernels, bit-exact
@pytest.mark.parametrize("C", WIDTHS)
def test_residual_forward_and_backward_are_bit_equal_to_torch(ops, C):
    """out = x + a * m (+ t_rows[scene]) and da = m * dy against the torch expressions of `TrainGraph._block`: the multiply and
    the add are rounded separately, so every bit agrees.  Two scenes of unequal length; a mask with zero rows, whose rows of
    da are exactly zero."""
    g = torch.Generator().manual_seed(C)
    for n in ROWS:
        x, a, dy = (torch.randn(n, C, generator=g).cuda() for _ in range(3))
        m = _mask(n, g).cuda()
        n0 = max(1, n // 3) if n > 1 else 1
        offs_host = [0, n] if n == 1 else [0, n0, n]
        offs = torch.tensor(offs_host, dtype=torch.int32).cuda()
        t_rows = torch.randn(len(offs_host) - 1, C, generator=g).cuda()
        batch = torch.repeat_interleave(torch.arange(len(offs_host) - 1), torch.tensor(np.diff(offs_host))).cuda()
        assert _bits(ops.residual(x, a), x + a)
        assert _bits(ops.residual(x, a, m), x + a * m[:, None])
        assert _bits(ops.residual(x, a, m, t_rows, offs), (x + a * m[:, None]) + t_rows[batch])
        assert _bits(ops.residual(x, None, None, t_rows, offs), x + t_rows[batch])
        xin = x.clone()
        assert ops.residual(xin, a, m, out=xin) is xin and _bits(xin, x + a * m[:, None])  # in place
        da = ops.scale_cast(dy, m)
        assert _bits(da, dy * m[:, None])
        if n > 1:
            assert bool((da[m == 0] == 0).all()) and int((m == 0).sum()) >= 1  # a dropped row: da = 0 exactly
        _sync()
    report(f"residual / scale C={C}", rows=str(ROWS), bit_equal=1)


@LPS
@pytest.mark.parametrize("C", WIDTHS)
def test_cast_without_saturation_is_torchs_cast(ops, lp, C):
    """The non-saturating cast (every dy of the AMP backward) against torch's `.to`: values beyond 65504, infs and a NaN
    included - in the half build they become inf where the library's own cast clamps."""
    g = torch.Generator().manual_seed(7 * C)
    for n in ROWS:
        dy = torch.randn(n, C, generator=g) * 300.0
        flat = dy.view(-1)
        flat[0], flat[1], flat[2], flat[3] = 70000.0, -1e6, float("inf"), float("-inf")
        flat[4], flat[5], flat[6] = 65504.0, 65520.0, float("nan")
        dy = dy.cuda()
        m = _mask(n, g, zero_rows=False).cuda()
        got = ops.scale_cast(dy, None, lp)
        assert got.dtype == LP() and _bits(got, dy.to(LP()))
        assert _bits_nan(ops.scale_cast(dy, m, lp), (dy * m[:, None]).to(LP()))  # (0 * inf where m = 0)
        if lp == "f16":
            assert bool(torch.isinf(got.view(-1)[:4]).all()) and float(got.view(-1)[4]) == 65504.0 and bool(torch.isinf(got.view(-1)[5]))
            assert float(ops.cast(dy, LP()).view(-1)[0]) == 65504.0  # (the library's cast saturates: why this kernel exists)
        _sync()
    report(f"cast without saturation {lp} C={C}", rows=str(ROWS), bit_equal=1)


def _block_params(C, H, rng, hidden=None):
    """The 18 parameters of a Block (module order) with the gains of tests/test_gpu_train.py's whole-Block test."""
    hidden = 4 * C if hidden is None else hidden
    wide = min(1.0, (64 / C) ** 0.5)
    shapes = [(C, 3, 3, 3, C), (C,), (C, C), (C,), (C,), (C,), (C,), (C,), (3 * C, C), (3 * C,), (C, C), (C,), (C,), (C,),
              (hidden, C), (hidden,), (C, hidden), (C,)]
    out = []
    for i, shape in enumerate(shapes):
        scale = {1: 0.1, 2: 0.3 * wide, 5: 0.3 * wide / 27 ** 0.5}[len(shape)]
        gain = 1.0 if i in (4, 6, 12) else 0.0  # LayerNorm weights
        out.append((rng.standard_normal(shape) * scale + gain).astype(np.float32))
    return out


@pytest.mark.parametrize("C,H", [(32, 2), (64, 4), (512, 32)])
@pytest.mark.parametrize("mode", ["fp32", "bf16", "f16", "f16-shadow"])
def test_derived_weights_are_the_transposes_and_the_mirrored_conv_kernel(ops, C, H, mode):
    """cdseg_train_block_prepare (one launch) against `w.t().contiguous()` and the flip / permute expression of
    `train._conv_bwd_weight`, bit for bit; under AMP the 16-bit forms are the library's cast of the weight, and with the
    optimizer's 16-bit copies the transposes are taken from those copies (no forward copy is made)."""
    from cdsegnet_amd import _lib
    from cdsegnet_amd.train import _conv_bwd_weight
    rng = np.random.default_rng(C)
    params = [torch.as_tensor(p).cuda() for p in _block_params(C, H, rng)]
    params[2].view(-1)[0] = 1e6  # beyond half: the 16-bit weight is the SATURATING cast
    variant = None if mode == "fp32" else mode.split("-")[0]
    with _lib.use(variant or "bf16"):
        shadows = None
        if mode.endswith("shadow"):
            t16 = ops.LP_DTYPES[variant]
            shadows = [(params[i] * 1.5).to(t16) for i in ops.TB_MATRICES]  # distinguishable from cast(w)
        tb = ops.TrainBlock(params, H, 0.25, (1e-5, 1e-5, 1e-5), variant, variant, False, shadows)
        tb.derived.fill_(0x5A)
        ops.train_block_prepare(tb)
        _sync()
        views = ops.train_block_derived_views(tb)
        for j, i in enumerate(ops.TB_MATRICES):
            w = params[i]
            if variant is not None:
                w16 = shadows[j] if shadows else ops.cast(w.reshape(w.shape[0], -1), ops.LP_DTYPES[variant])
                w = w16.reshape(w.shape)
                if shadows:
                    assert bool((views[j][1].view(torch.uint8) == 0x5A).all())  # untouched: the forward reads the shadow
                else:
                    assert _bits(views[j][1], w16.reshape(w.shape[0], -1)), i
            want = _conv_bwd_weight(w.reshape(C, 27 * C), C, C) if i == 0 else w.t().contiguous()
            assert _bits(views[j][0], want), (mode, i)
    report(f"derived weights C={C} {mode}", derived_bytes=tb.derived_bytes, weight_bytes=4 * sum(params[i].numel() for i in ops.TB_MATRICES))


# ------------------------------------------------------------------------------------------ (2) GELU, add_layernorm vs fp64
def _assert_vs_torch(what, pairs):
    """pairs: (tensor name, kernel result, torch fp32 result, fp64 oracle).  kernel <= 3 E_torch + 2^-24."""
    for tn, got, t32, g64 in pairs:
        assert bool(torch.isfinite(got.float()).all()), (what, tn)
        e, et = _err(got, g64), _err(t32, g64)
        report(f"{what} {tn}", kernel_err=e, E_torch=et, bound=3 * et + U)
        assert e <= 3 * et + U, (what, tn, e, et)


@pytest.mark.parametrize("out", ["fp32", "bf16", "f16"])
@pytest.mark.parametrize("C", WIDTHS)
def test_gelu_forward_and_backward_vs_fp64_within_three_times_torch(ops, out, C):
    """g = GELU(u) and du = dg GELU'(u) on u = 2 N(0, 1) (the tails included), fp64 oracle and torch's fp32 op on the same
    device values; a 16-bit output is compared with torch's fp32 result cast to that type."""
    from cdsegnet_amd import _lib
    variant = None if out == "fp32" else out
    g = torch.Generator().manual_seed(C + 1)
    with _lib.use(variant or "bf16"):
        for n in ROWS:
            u = (2.0 * torch.randn(n, 4 * C, generator=g)).cuda()
            dg = torch.randn(n, 4 * C, generator=g).cuda()
            u64 = u.double().requires_grad_(True)
            g64 = F.gelu(u64)
            g64.backward(dg.double())
            u32 = u.clone().requires_grad_(True)
            g32 = F.gelu(u32)
            g32.backward(dg)
            to = (lambda t: t) if variant is None else (lambda t: t.to(ops.LP_DTYPES[variant]))
            got_g, got_du = ops.gelu_fwd(u, variant), ops.gelu_bwd_cast(u, dg, variant)
            _sync()
            assert got_g.dtype == to(u).dtype and got_du.dtype == to(u).dtype
            _assert_vs_torch(f"gelu {out} {n}x{4 * C}", [("g", got_g, to(g32.detach()), g64.detach()), ("du", got_du, to(u32.grad), u64.grad)])
    if out == "f16":  # an inf in dg stays an inf (the library's cast would clamp it)
        with _lib.use("f16"):
            dg = torch.full((1, 16), 7e4).cuda()
            assert bool(torch.isinf(ops.gelu_bwd_cast(torch.full((1, 16), 3.0).cuda(), dg, "f16")).all())


@pytest.mark.parametrize("out", ["fp32", "bf16", "f16"])
@pytest.mark.parametrize("C", WIDTHS)
def test_add_layernorm_vs_fp64_within_three_times_torch(ops, out, C):
    """x1 = x + m a (bit-equal to torch) and h = LN(x1) in one pass: h against fp64 F.layer_norm of the same x1, with torch's
    fp32 F.layer_norm as the yardstick."""
    from cdsegnet_amd import _lib
    variant = None if out == "fp32" else out
    g = torch.Generator().manual_seed(C + 2)
    gamma, beta = (1 + 0.3 * torch.randn(C, generator=g)).cuda(), (0.1 * torch.randn(C, generator=g)).cuda()
    with _lib.use(variant or "bf16"):
        for n in ROWS:
            x, a = (0.5 + torch.randn(n, C, generator=g)).cuda(), torch.randn(n, C, generator=g).cuda()
            for m in (None, _mask(n, g).cuda()):
                x1, h = ops.add_layernorm(x, a, m, gamma, beta, 1e-5, variant)
                _sync()
                want = x + (a if m is None else a * m[:, None])
                assert _bits(x1, want)
                h64 = F.layer_norm(want.double(), (C,), gamma.double(), beta.double(), 1e-5)
                h32 = F.layer_norm(want, (C,), gamma, beta, 1e-5)
                if variant is not None:
                    h32 = h32.to(ops.LP_DTYPES[variant])
                assert h.dtype == h32.dtype
                _assert_vs_torch(f"add_layernorm {out} {n}x{C} mask={m is not None}", [("h", h, h32, h64)])


# ------------------------------------------------------------------------------------------ (3) one whole Block
class _Level:
    """What `TrainGraph._block` asks of a plan level, from a hand-built plan."""

    def __init__(self, nbr_k, gidx, widx, cu, offs_host, batch):
        self.n = int(batch.numel())
        self._nbr, self._gidx, self._widx, self.batch, self.offs_host = nbr_k, gidx, widx, batch, list(offs_host)
        self._cu = np.asarray(cu, dtype=np.int32)
        self._cu_dev = torch.as_tensor(self._cu).cuda()
        self._offs_dev = torch.tensor(self.offs_host, dtype=torch.int32).cuda()

    def nbr(self, ksize, kmajor=False):
        assert ksize == 3 and kmajor
        return self._nbr

    def slots(self, curve, patch_size, enable_flash):
        return self._gidx, self._widx

    def pad(self, patch_size, enable_flash):
        lens = np.diff(self._cu)
        return (patch_size, int(self._cu[-1]), self._offs_dev, None, self._cu_dev, int(lens.max()), float((lens * lens).sum()))

    def pad_host(self, patch_size, enable_flash):
        return (patch_size, None, None, self._cu)


_PLANS, _REFS = {}, {}
PATCH = 64
ROW_CONFIGS = {"1": [1], "65": [65], "200": [200], "130+77": [130, 77]}


def _plan(rows):
    """Scenes of `rows` points each from synth.room_scene (a real kernel map with -1 entries), one batch; patch size 64: several
    patches, a padded last patch that borrows from the one before; any serialization order per scene.  Built once per shape."""
    key = tuple(rows)
    if key not in _PLANS:
        from cdsegnet_amd import synth
        from oracle import model as OM
        from oracle import serialization as S
        from tests.test_gpu_train import _slot_plan
        rng = np.random.default_rng(sum(rows))
        grids, batch = [], []
        for b, nb in enumerate(rows):
            sc = synth.room_scene(20 + b, max(400, 3 * nb))
            gc = np.asarray(sc["grid_coord"], dtype=np.int64)
            assert len(gc) >= nb and len(np.unique(gc, axis=0)) == len(gc)
            grids.append(gc[:nb])
            batch.append(np.full(nb, b, dtype=np.int64))
        grid, batch = np.concatenate(grids), np.concatenate(batch)
        n = len(grid)
        nbr = OM.subm_neighbors(grid, batch, 3)
        assert (nbr < 0).any() and (nbr[:, 13] == np.arange(n)).all()
        offset = np.cumsum(rows)
        pad, unpad, cu = S.padding_plan(offset, PATCH)
        offs = np.concatenate([[0], offset])
        perm = np.concatenate([offs[b] + rng.permutation(rows[b]) for b in range(len(rows))])
        inv = np.empty(n, dtype=np.int64)
        inv[perm] = np.arange(n)
        order, inverse = perm[pad], unpad[inv]
        d = torch.device("cuda")
        gidx, widx = _slot_plan(order, inverse, d)
        lv = _Level(torch.as_tensor(nbr.T.astype(np.int32)).contiguous().to(d), gidx, widx, cu, offs.tolist(),
                    torch.as_tensor(batch.astype(np.int32)).to(d))
        _PLANS[key] = dict(n=n, nbr=nbr, order=order, inverse=inverse, cu=np.asarray(cu), batch=batch, lv=lv, B=len(rows))
    return _PLANS[key]


NAMES18 = ["cpe.0.weight", "cpe.0.bias", "cpe.1.weight", "cpe.1.bias", "cpe.2.weight", "cpe.2.bias", "norm1.0.weight", "norm1.0.bias",
           "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias", "norm2.0.weight", "norm2.0.bias",
           "mlp.0.fc1.weight", "mlp.0.fc1.bias", "mlp.0.fc2.weight", "mlp.0.fc2.bias"]


def _case(C, H, rows_key, distinct, with_t, masks):
    """Inputs (numpy, built once and never modified) and the fp64 torch-autograd reference of one Block case."""
    key = (C, H, rows_key, distinct, with_t, masks)
    if key in _REFS:
        return _REFS[key]
    from oracle import model as OM
    plan = _plan(ROW_CONFIGS[rows_key])
    n, B = plan["n"], plan["B"]
    rng = np.random.default_rng(C + 7 * n)
    params = _block_params(C, H, rng)
    x_in, dy = rng.standard_normal((n, C)).astype(np.float32), rng.standard_normal((n, C)).astype(np.float32)
    x_conv = rng.standard_normal((n, C)).astype(np.float32) if distinct else None
    t_rows = (0.5 * rng.standard_normal((B, C))).astype(np.float32) if with_t else None
    if masks == "none":
        m1 = m2 = None
    elif masks == "kept":
        m1 = m2 = np.full(n, 1.0 / 0.7, dtype=np.float32)
    else:
        m1, m2 = ((rng.random(n) < 0.7).astype(np.float32) / np.float32(0.7) for _ in range(2))
        if n > 1:
            m1[0], m2[n - 1] = 0.0, 0.0
    # ---- fp64 torch autograd on the oracle restatement (oracle/train.py block_full_grads, with x_conv, t_rows and masks)
    P = [torch.as_tensor(p).double().requires_grad_(True) for p in params]
    xi = torch.as_tensor(x_in).double().requires_grad_(True)
    xc = torch.as_tensor(x_conv).double().requires_grad_(True) if distinct else xi
    tr = torch.as_tensor(t_rows).double().requires_grad_(True) if with_t else None
    ln = lambda v, i: F.layer_norm(v, (C,), P[i], P[i + 1], 1e-5)  # noqa: E731
    x0 = xi + ln(F.linear(OM.subm_conv3d(xc, plan["nbr"], P[0], P[1]), P[2], P[3]), 4)
    if with_t:
        x0 = x0 + tr[torch.as_tensor(plan["batch"])]
    qkv = F.linear(ln(x0, 6), P[8], P[9])
    L3 = qkv[torch.as_tensor(plan["order"])].reshape(-1, 3, C)
    feat = OM._patch_attention(L3[:, 0], L3[:, 1], L3[:, 2], plan["cu"], H, (C // H) ** -0.5)
    a = F.linear(feat[torch.as_tensor(plan["inverse"])], P[10], P[11])
    x1 = x0 + (a if m1 is None else a * torch.as_tensor(m1).double()[:, None])
    h = F.linear(F.gelu(F.linear(ln(x1, 12), P[14], P[15])), P[16], P[17])
    y = x1 + (h if m2 is None else h * torch.as_tensor(m2).double()[:, None])
    (y * torch.as_tensor(dy).double()).sum().backward()
    ref = {"y": y.detach(), "dx_in": xi.grad}
    if distinct:
        ref["dx_conv"] = xc.grad
    if with_t:
        ref["dt_rows"] = tr.grad
    ref.update({k: p.grad for k, p in zip(NAMES18, P)})
    _REFS[key] = dict(plan=plan, params=params, x_in=x_in, x_conv=x_conv, t_rows=t_rows, m1=m1, m2=m2, dy=dy, ref=ref)
    return _REFS[key]


def _graph(tp, mode, training=True, det=False):
    """A TrainGraph with only what `_block` reads (no model, no engine)."""
    tg = TG.TrainGraph.__new__(TG.TrainGraph)
    tg.model = types.SimpleNamespace(training=training)
    tg.attn_variant = TG.TRAIN_PRECISIONS[tp]
    tg.mm_variant = TG.TRAIN_PRECISIONS[tp] if tp.endswith("-amp") else None
    tg.det, tg.train_block, tg._native = det, mode, {}
    return tg


def _run_block(case, C, H, tp, mode, training=True, drop_prob=0.0, use_masks=True):
    """The Block through `TrainGraph._block` in `mode`: (results by name, the Block module)."""
    from cdsegnet_amd import models
    plan = case["plan"]
    n = plan["n"]
    with_t = case["t_rows"] is not None
    blk = models.Block(C, H, patch_size=PATCH, enable_flash=True, T_dim=C if with_t else -1, drop_path=drop_prob).cuda()
    with torch.no_grad():
        for name, p in zip(NAMES18, case["params"]):
            dict(blk.named_parameters())[name].copy_(torch.as_tensor(p))
        if with_t:  # the timestep Linear as the identity: t_rows = t_scene exactly, and t_scene.grad = dt_rows
            blk.t_mlp.weight.copy_(torch.eye(C))
            blk.t_mlp.bias.zero_()
    x_in = torch.as_tensor(case["x_in"]).cuda().requires_grad_(True)
    x_conv = torch.as_tensor(case["x_conv"]).cuda().requires_grad_(True) if case["x_conv"] is not None else None
    t_scene = torch.as_tensor(case["t_rows"]).cuda().requires_grad_(True) if with_t else None
    st = TG._St(plan["lv"], x_in, [0], torch.arange(n, dtype=torch.int32).cuda())
    st.conv = x_conv
    masks = None
    if use_masks and case["m1"] is not None:
        masks = {"blk.drop_path.0": [case["m1"].copy(), case["m2"].copy()]}
    tg = _graph(tp, mode, training)
    y = tg._block(st, blk, "blk", t_scene, masks).x
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
    return out, blk


BLOCK_CASES = []
for _ci, (_C, _H) in enumerate([(32, 2), (64, 4), (512, 32)]):
    for _j, _rk in enumerate(ROW_CONFIGS):
        BLOCK_CASES.append((_C, _H, _rk, bool(_j % 2), bool(((_j // 2) + _ci) % 2), ("none", "kept", "dropped")[(_j + _ci) % 3]))
PRECISIONS = pytest.mark.parametrize("tp,lp", [("fp32", "bf16"), ("fp16-attn", "f16"), ("fp16-amp", "f16"), ("bf16-amp", "bf16")])


def test_block_cases_cover_every_option_at_every_width():
    for C in (32, 64, 512):
        mine = [c for c in BLOCK_CASES if c[0] == C]
        assert {c[2] for c in mine} == set(ROW_CONFIGS) and {c[3] for c in mine} == {False, True}
        assert {c[4] for c in mine} == {False, True} and {c[5] for c in mine} == {"none", "kept", "dropped"}


@PRECISIONS
@pytest.mark.parametrize("C,H,rows,distinct,with_t,masks", BLOCK_CASES,
                         ids=[f"C{c}-n{r}-{'xconv' if d else 'same'}-{'t' if t else 'not'}-{m}" for c, _, r, d, t, m in BLOCK_CASES])
def test_whole_block_forward_and_backward_vs_fp64_within_three_times_autograd(ops, tp, lp, C, H, rows, distinct, with_t, masks):
    """y, dx_in, dx_conv, dt_rows and all 18 parameter gradients of the native Block against fp64 torch autograd on the oracle
    restatement; the yardstick per tensor is the AUTOGRAD mode's error on the same inputs, build and precision, measured
    here: native <= 3 E_auto + 2^-24 (metric: max |g - g64| / max |g64|)."""
    case = _case(C, H, rows, distinct, with_t, masks)
    auto, _ = _run_block(case, C, H, tp, "autograd")
    nat, _ = _run_block(case, C, H, tp, "native")
    assert set(auto) == set(nat) == set(case["ref"])
    worst, over = ("", 0.0), []
    for k, g64 in case["ref"].items():
        assert nat[k].dtype == torch.float32 and nat[k].shape == auto[k].shape and bool(torch.isfinite(nat[k]).all()), k
        e, ea = _err(nat[k], g64), _err(auto[k], g64)
        used = e / (3 * ea + U)
        if used > worst[1]:
            worst = (k, used)
        if e > 3 * ea + U:
            over.append((k, e, ea))
    report(f"whole Block {tp} C={C} rows={rows} xconv={distinct} t={with_t} masks={masks}", tensors=len(nat),
           y_err=_err(nat["y"], case["ref"]["y"]), y_E_auto=_err(auto["y"], case["ref"]["y"]),
           dx_err=_err(nat["dx_in"], case["ref"]["dx_in"]), dx_E_auto=_err(auto["dx_in"], case["ref"]["dx_in"]),
           worst_bound_used=worst[1], worst_tensor=worst[0])
    assert not over, over


def test_eval_mode_makes_droppath_the_identity(ops):
    """A Block with drop_path = 0.3 on a model in eval mode: no mask is drawn, the result is bit-equal to the masks = None
    case of the same Block in training mode with drop_path = 0."""
    case = _case(32, 2, "65", False, False, "none")
    a, _ = _run_block(case, 32, 2, "fp32", "native", training=False, drop_prob=0.3)
    b, _ = _run_block(case, 32, 2, "fp32", "native", training=True, drop_prob=0.0)
    assert _bits(a["y"], b["y"]) and _bits(a["dx_in"], b["dx_in"])


# ------------------------------------------------------------------------------------------ (4) the recorded reference step
def test_recorded_step_in_the_native_mode_meets_the_reference_bound(ops, monkeypatch):
    """tests/test_gpu_train.py's comparison against the reference's recorded step (`train_step_mini.npz`, fp32), run as it is
    on a model with train_block = "native": the same assertions, the same bounds; every Block went through the executor."""
    from tests import test_gpu_train as T
    build = T._mini_training_model
    calls = {"fwd": 0, "bwd": 0}
    fwd, bwd = O.train_block_forward, O.train_block_backward

    def native_model(fx, dev_):
        model, sd = build(fx, dev_)
        model.train_block = "native"
        return model, sd

    monkeypatch.setattr(T, "_mini_training_model", native_model)
    monkeypatch.setattr(O, "train_block_forward", lambda *a: (calls.__setitem__("fwd", calls["fwd"] + 1), fwd(*a))[1])
    monkeypatch.setattr(O, "train_block_backward", lambda *a: (calls.__setitem__("bwd", calls["bwd"] + 1), bwd(*a))[1])
    T.test_whole_training_step_matches_the_reference_train_step()
    assert calls["fwd"] == calls["bwd"] > 0, calls


@pytest.mark.parametrize("norm", ["torch", "fused"])
@pytest.mark.parametrize("tp,lp", [("fp32", "bf16"), ("fp16-amp", "f16")])
def test_two_room_step_native_vs_autograd(ops, tp, lp, norm):
    """Two 4 k-point rooms, seeded draws: the native mode against the autograd mode by the metric and bound of the whole-step
    comparison in tests/test_gpu_deterministic.py (per tensor max |a - b| / (max |a| + 1e-3 top) < 1e-3; fp32: the same sums in
    the same kernels, AMP: the same roundings up to the GELU's and LayerNorm's last bit)."""
    from tests.test_gpu_deterministic import _batch, _model, _step
    inp, draws, n = _batch()
    model = _model(tp, False)
    model.train_norm = norm
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}

    def run(mode):
        model.load_state_dict(state)
        model.train_block = mode
        return _step(model, inp, draws)

    l0, g0 = run("autograd")
    l1, g1 = run("native")
    assert bool(torch.isfinite(l1)) and set(g0) == set(g1) and len(g0) > 400
    top = max(float(g.abs().max()) for g in g0.values())
    per = {k: float((g0[k] - g1[k]).abs().max()) / (float(g0[k].abs().max()) + 1e-3 * top) for k in g0}
    worst = max(per, key=per.get)
    report(f"two-room step {tp} norm={norm}: native vs autograd", loss_autograd=float(l0), loss_native=float(l1),
           loss_rel_diff=abs(float(l0) - float(l1)) / abs(float(l0)), worst_rel_diff=per[worst], worst_tensor=worst)
    assert all(bool(torch.isfinite(g).all()) for g in g1.values())
    assert per[worst] < 1e-3
    assert abs(float(l0) - float(l1)) <= 1e-3 * abs(float(l0))


# ------------------------------------------------------------------------------------------ (5) determinism
def _two_steps(tp, seed, shadow=None, det=True):
    """Two seeded native steps with the fused AdamW: (losses, gradients of the second step, parameters afterwards)."""
    from cdsegnet_amd.optim import FusedAdamW
    from tests.test_gpu_deterministic import _batch, _model
    inp, _, n = _batch()
    model = _model(tp, det)
    model.train_block = "native"
    opt = FusedAdamW(model.parameters(), lr=0.002, weight_decay=0.05, **({"shadow16": shadow} if shadow else {}))
    torch.manual_seed(seed)
    losses = []
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        loss = model(inp)["loss"]
        loss.backward()
        grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
        opt.step()
        losses.append(loss.detach().clone())
    _sync()
    return losses, grads, {k: v.detach().clone() for k, v in model.state_dict().items()}


@pytest.mark.parametrize("tp,lp", [("fp32", "bf16"), ("fp16-amp", "f16")])
def test_native_steps_are_bit_reproducible(ops, tp, lp):
    """train_deterministic = True: two seeded native steps, twice - bit-equal losses, gradients and post-AdamW parameters."""
    (la, ga, sa), (lb, gb, sb) = _two_steps(tp, 991), _two_steps(tp, 991)
    assert all(bool(torch.isfinite(x)) for x in la) and all(torch.equal(x, y) for x, y in zip(la, lb))
    assert set(ga) == set(gb) and len(ga) > 400
    diff = [k for k in ga if not torch.equal(ga[k], gb[k])] + [k for k in sa if not torch.equal(sa[k], sb[k])]
    report(f"native deterministic {tp}", loss0=float(la[0]), loss1=float(la[1]), tensors_differing=len(diff))
    assert not diff, diff[:8]


def test_shadow_copies_give_the_same_loss(ops):
    """fp16-amp with FusedAdamW(shadow16="f16") against no shadows: the optimizer's 16-bit copies are the library's cast of the
    weights, so both losses of two steps are bit-equal (the second step reads copies the first step's update wrote)."""
    lp = "f16"  # noqa: F841  (documentation: the half build, selected by the model's train_precision)
    (la, _, _), (lb, _, _) = _two_steps("fp16-amp", 5, shadow="f16"), _two_steps("fp16-amp", 5)
    report("native shadow16 on / off", loss0_on=float(la[0]), loss0_off=float(lb[0]), loss1_on=float(la[1]), loss1_off=float(lb[1]))
    assert torch.equal(la[0], lb[0]) and torch.equal(la[1], lb[1])


# ------------------------------------------------------------------------------------------ (6) overflow
def test_run_step_with_a_scale_that_overflows_half(ops):
    """The reference trainer's run_step (engines/train.py:216-271, the sequence of tests/test_gpu_train_amp.py) in the native
    mode, fp16-amp, with an initial loss scale of 2^24: the first backward leaves a non-finite value in the gradients (the
    unsaturated cast of a dy), the scaler skips that step and every parameter keeps its bits, the scale halves, and within 25
    steps one proceeds and moves the parameters."""
    fx = load_fixture("train_step_mini.npz")
    model, _ = _mini_model(fx, torch.device("cuda"), False)
    model.train_precision, model.train_block = "fp16-amp", "native"
    opt = torch.optim.AdamW(model.parameters(), lr=0.002, weight_decay=0.05)
    scaler = torch.cuda.amp.GradScaler(init_scale=2.0 ** 24)
    inp = _inp(fx)
    skipped, moved, first_nonfinite = 0, 0.0, None
    for step in range(25):
        before = {k: p.detach().clone() for k, p in model.named_parameters()}
        with torch.cuda.amp.autocast(enabled=True):
            loss = model(inp, draws=_draws(fx))["loss"]
        assert loss.dtype == torch.float32 and bool(torch.isfinite(loss))
        opt.zero_grad()
        scaler.scale(loss).backward()
        nonfinite = sum(int((~torch.isfinite(p.grad)).sum()) for p in model.parameters() if p.grad is not None)
        if step == 0:
            first_nonfinite = nonfinite
        scaler.step(opt)
        scale = scaler.get_scale()
        scaler.update()
        _sync()
        if scaler.get_scale() == scale:
            assert nonfinite == 0
            moved = max(float((p.detach() - before[k]).abs().max()) for k, p in model.named_parameters())
            break
        assert nonfinite > 0 and scaler.get_scale() == scale / 2
        assert all(torch.equal(p.detach(), before[k]) for k, p in model.named_parameters()), "a skipped step moved parameters"
        skipped += 1
    report("native run_step fp16-amp, init_scale 2^24", loss=float(loss.detach()), nonfinite_grad_values_first_step=first_nonfinite,
           skipped_steps=skipped, final_scale=scaler.get_scale(), max_param_move=moved)
    assert first_nonfinite > 0 and skipped >= 1 and moved > 1e-5


# ------------------------------------------------------------------------------------------ (7) structure
def test_one_forward_and_one_backward_call_per_block_and_prepare_once_per_weight_version(ops, monkeypatch):
    """With the ops counted: a native step makes exactly one train_block_forward and one train_block_backward per Block; no
    ops.gemm / layernorm / attention / *_wgrad / layernorm_bwd / attention_bwd call is made from inside a Block (forward: inside
    `TrainGraph._block`; backward: inside `_NativeBlock.backward`); prepare runs once per Block per weight version - twice over
    two optimizer steps, not again for a second forward without a step; an in-place weight change between forward and backward
    raises."""
    from cdsegnet_amd import models
    fx = load_fixture("train_step_mini.npz")
    model, _ = _mini_model(fx, torch.device("cuda"), False)
    model.train_block = "native"
    blocks = sum(isinstance(m, models.Block) for m in model.modules())
    assert blocks > 0
    calls = {"fwd": 0, "bwd": 0, "prepare": 0, "inside": [], "outside": 0}
    state = {"in_block": 0}

    def counted(key, fn):
        def f(*a, **kw):
            calls[key] += 1
            return fn(*a, **kw)
        return f

    def guarded(name, fn):
        def f(*a, **kw):
            if state["in_block"]:
                calls["inside"].append(name)
            else:
                calls["outside"] += 1
            return fn(*a, **kw)
        return f

    def bracket(fn):
        def f(*a, **kw):
            state["in_block"] += 1
            try:
                return fn(*a, **kw)
            finally:
                state["in_block"] -= 1
        return f

    monkeypatch.setattr(O, "train_block_forward", counted("fwd", O.train_block_forward))
    monkeypatch.setattr(O, "train_block_backward", counted("bwd", O.train_block_backward))
    monkeypatch.setattr(O, "train_block_prepare", counted("prepare", O.train_block_prepare))
    for name in ("gemm", "layernorm", "attention", "linear_wgrad", "conv_wgrad", "layernorm_bwd", "attention_bwd", "cast"):
        monkeypatch.setattr(O, name, guarded(name, getattr(O, name)))
    monkeypatch.setattr(TG.TrainGraph, "_block", bracket(TG.TrainGraph._block))
    monkeypatch.setattr(TG._NativeBlock, "backward", staticmethod(bracket(TG._NativeBlock.backward)))
    opt = torch.optim.AdamW(model.parameters(), lr=0.002, weight_decay=0.05)
    inp = _inp(fx)

    loss = model(inp, draws=_draws(fx))["loss"]
    assert (calls["fwd"], calls["bwd"], calls["prepare"]) == (blocks, 0, blocks)
    loss.backward()
    _sync()
    assert (calls["fwd"], calls["bwd"], calls["prepare"]) == (blocks, blocks, blocks)
    assert calls["inside"] == [] and calls["outside"] > 0  # (the stems, pooling, the cross Block still go through ops.*)
    model(inp, draws=_draws(fx))  # a second forward without a step: the derived weights are current
    assert calls["prepare"] == blocks
    opt.step()
    loss = model(inp, draws=_draws(fx))["loss"]
    assert calls["prepare"] == 2 * blocks
    loss.backward()
    opt.step()
    loss = model(inp, draws=_draws(fx))["loss"]
    assert calls["prepare"] == 3 * blocks and calls["fwd"] == 4 * blocks and calls["bwd"] == 2 * blocks
    with torch.no_grad():
        next(p for k, p in model.named_parameters() if "block" in k and k.endswith("fc2.weight")).mul_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()
    _sync()
    report("native structure", blocks=blocks, forward_calls_per_step=blocks, backward_calls_per_step=blocks, prepare_per_weight_version=blocks)
