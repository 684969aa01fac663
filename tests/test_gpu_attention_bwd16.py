"""GPU: the 16-bit attention backward (csrc/train.hip attn_bwd16_*_kernel) and the 16-bit attention core of the training step
(`DefaultSegmentorV2.train_precision`), both builds of the library.

Oracle (this file): fp64 numpy on the 16-bit-rounded q, k, v, dout, with q' = round16(fp32(q) * fp32(scale log2 e)) as the
kernels round it and no other rounding - the exact gradient of the function the 16-bit forward computes (the q' rounding is
the identity in the chain rule):  s' = q'.k,  P = exp2(s' - m') / l,  dP = dO v^T,  D = sum_j P dP,  dS = P (dP - D),
dq = c ln 2 dS k,  dk = ln 2 dS^T q',  dv = P^T dO,  c = fp32(scale log2 e).

Tolerance.  It is set against the reference's arithmetic, not against the kernel: E_ref is the error, against that oracle, of
an fp64 emulation that rounds P and dS to the 16-bit type where flash-attention does (P as the operand of dv, dS as the
operand of dq and dk; statistics and everything else exact).  Metric per tensor: max |g - g64| / max |g64|.  The kernel must
stay within 2 E_ref + L 2^-24 (L = the longest patch: fp32 accumulation over L slots on the same scale; the factor 2 covers
accumulation order and values that round to the neighbouring 16-bit number in fp32 but not in fp64).
"""
import ctypes
import threading

import numpy as np
import pytest
import torch

from cdsegnet_amd import ops as O
from tests.helpers import load_fixture
from tests.test_gpu_attention_range import Launch, _assign_shifts, _base_rows, _c32, _make_patches, _r16
from tests.test_gpu_ops import LP, _library_variant, dev, ops, report  # noqa: F401  (fixtures: lp="f16" -> the half build)

pytestmark = pytest.mark.gpu

LPS = pytest.mark.parametrize("lp", ["bf16", "f16"])
SCALE = 0.25
LN2 = float(np.log(2.0))


def _r16ns(x, lp):
    """Round to the 16-bit type WITHOUT saturation (torch's cast: beyond half's range -> inf), as float64."""
    return torch.as_tensor(np.asarray(x, dtype=np.float64)).float().to(lp).double().numpy()


def _q_eff(q16, lp, scale=SCALE):
    """q' as the kernels compute it: the fp32 product with fp32(scale log2 e), then ONE rounding to the 16-bit type."""
    return _r16((torch.as_tensor(q16).float() * _c32(scale)).double().numpy(), lp)


def _grads(q16, k16, v16, do16, launch, H, lp, mode="exact", scale=SCALE):
    """fp64 dq (q rows), dk, dv (kv rows) on the launch's slot plan.  mode: "exact" (the oracle), "emul" (P and dS rounded to
    the 16-bit type where flash-attention rounds them), "noround" (the oracle without the q' rounding)."""
    c = _c32(scale)
    qe = q16 * c if mode == "noround" else _q_eff(q16, lp, scale)
    dq, dk, dv = np.zeros_like(q16), np.zeros_like(k16), np.zeros_like(v16)
    for gq, gkv, widx in launch.patches:
        live = widx >= 0
        for h in range(H):
            sl = slice(16 * h, 16 * h + 16)
            K, V = k16[gkv][:, sl], v16[gkv][:, sl]
            dO = np.where(live[:, None], do16[np.where(live, widx, 0)][:, sl], 0.0)
            S = qe[gq][:, sl] @ K.T
            P = np.exp2(S - S.max(1, keepdims=True))
            P /= P.sum(1, keepdims=True)
            dP = dO @ V.T
            D = (P * dP).sum(1, keepdims=True)
            dS = P * (dP - D)
            Pv = P
            if mode == "emul":
                Pv, dS = _r16ns(P, lp), _r16ns(dS, lp)
            np.add.at(dq[:, sl], gq, c * LN2 * (dS @ K))
            np.add.at(dk[:, sl], gkv, LN2 * (dS.T @ qe[gq][:, sl]))
            np.add.at(dv[:, sl], gkv, Pv.T @ dO)
    return dq, dk, dv


def _kernel(lp, q16, k16, v16, do16, launch, H, packed=False, scale=SCALE, dtype=None):
    """ops.attention_bwd on the device -> fp64 (dq, dk, dv).  packed: q / k / v are strided views of one (n, 3C) buffer and
    dq / dk / dv views of one fp32 (n, 3C) buffer (the training graph's layout).  dtype: torch.float32 runs the fp32 form."""
    t = dtype or lp
    n, C = q16.shape
    if packed:
        assert k16.shape == q16.shape
        qkv = dev(np.concatenate([q16, k16, v16], 1), t)
        q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
        g = torch.zeros(n, 3 * C, dtype=torch.float32, device="cuda")
        dq, dk, dv = g[:, :C], g[:, C:2 * C], g[:, 2 * C:]
    else:
        q, k, v = dev(q16, t), dev(k16, t), dev(v16, t)
        dq = torch.zeros(q16.shape, dtype=torch.float32, device="cuda")
        dk, dv = (torch.zeros(k16.shape, dtype=torch.float32, device="cuda") for _ in range(2))
    gq, gkv, widx, ps = launch.device()
    O.attention_bwd(q, k, v, gq, gkv, widx, ps, launch.ps.tolist(), H, scale, dev(do16, t), dq, dk, dv)
    torch.cuda.synchronize()
    return tuple(x.cpu().double().numpy() for x in (dq, dk, dv))


def _metric(g, g64):
    return float(np.abs(g - g64).max()) / max(float(np.abs(g64).max()), 1e-300)


def _compare(name, got, launch, q16, k16, v16, do16, H, lp, enforce=True, extra=None):
    """Kernel error, E_ref and their ratio per tensor; asserts error <= 2 E_ref + L 2^-24 (+ extra[tensor]).  Returns the worst
    ratio."""
    exact = _grads(q16, k16, v16, do16, launch, H, lp, "exact")
    emul = _grads(q16, k16, v16, do16, launch, H, lp, "emul")
    worst = 0.0
    for i, (tn, g, g64, ge) in enumerate(zip(("dq", "dk", "dv"), got, exact, emul)):
        assert np.isfinite(g64).all()
        if enforce:
            assert np.isfinite(g).all(), f"{name} {tn}: not finite"
        if not np.abs(g64).max() > 0:  # (a launch of 1-slot patches: dS = 0)
            assert not enforce or np.abs(g).max() == 0
            continue
        err, eref = _metric(g, g64), _metric(ge, g64)
        bound = 2 * eref + launch.max_len * 2.0 ** -24 + (extra[i] if extra else 0.0)
        ratio = err / max(eref, 1e-300)
        worst = max(worst, ratio)
        report(f"attn bwd16 {name} {tn}", kernel_err=err, E_ref=eref, ratio=ratio, bound=bound)
        if enforce:
            assert err <= bound, (name, tn, err, eref, bound)
    return worst


def _inputs(n, nkv, H, lp, rng, sigma_k=1.0, dout_mag=0.1):
    q16 = _r16(rng.standard_normal((n, 16 * H)), lp)
    k16 = _r16(rng.standard_normal((nkv, 16 * H)) * sigma_k, lp)
    v16 = _r16(rng.standard_normal((nkv, 16 * H)), lp)
    do16 = _r16(rng.standard_normal((n, 16 * H)) * dout_mag, lp)
    return q16, k16, v16, do16


# (name, patch lengths, heads, padding duplicates of the last patch, cross attention, packed strided views, sigma of k)
CASES = [
    ("L700", [700], 2, 0, False, True, 1.0),
    ("L1024-1024-300", [1024, 1024, 300], 4, 0, False, True, 3.0),
    ("L64-1-130", [64, 1, 130], 8, 0, False, False, 1.0),
    ("ragged", [1, 31, 32, 33, 63, 65], 2, 0, False, True, 3.0),
    ("dups", [200, 1024, 300], 2, 100, False, True, 1.0),
    ("cross", [512, 65, 1024], 2, 40, True, False, 3.0),
]


def _case(lens, H, dup, cross, lp, rng, sigma_k, dout_mag=0.1):
    n = sum(lens) - dup
    nkv = n + 50 if cross else n  # cross attention: keys / values are rows of another, longer tensor
    kv_rows = rng.permutation(nkv)[:n] if cross else None
    patches, _ = _make_patches(lens, 0, rng, dup_last=dup, cross=cross, kv_rows=kv_rows)
    launch = Launch(patches)
    return launch, _inputs(n, nkv, H, lp, rng, sigma_k, dout_mag)


@LPS
@pytest.mark.parametrize("name,lens,H,dup,cross,packed,sigma_k", CASES, ids=[c[0] for c in CASES])
def test_gradients_vs_fp64_within_twice_the_reference_rounding(ops, lp, name, lens, H, dup, cross, packed, sigma_k):
    """dq / dk / dv of ordinary scores (|s'| up to about 10-20), dout of magnitude 0.1: ragged lengths, padding duplicates
    (slots with widx = -1 whose rows also sit elsewhere in the patch), cross attention with another row count, strided views
    of a packed qkv buffer."""
    lpt = LP()
    rng = np.random.default_rng(sum(lens) + 31 * H + dup)
    launch, (q16, k16, v16, do16) = _case(lens, H, dup, cross, lpt, rng, sigma_k)
    with ops.record_routes() as rr:
        got = _kernel(lpt, q16, k16, v16, do16, launch, H, packed=packed)
    worst = _compare(name, got, launch, q16, k16, v16, do16, H, lpt)
    report(f"attn bwd16 {name} worst ratio ({lp})", ratio=worst)
    # the launch record: the plain pair, every patch-head cut in four (at most 24 patch-heads here: 24 * 4 * 2 <= 512)
    assert len(lens) * H <= 24
    assert rr.count == 2 and rr.kernels() == ["attn_bwd16_q_kernel<>", "attn_bwd16_kv_kernel<>"], rr.routes
    assert all(r.splits == 4 and r.compute == ops.BF16 for r in rr.routes), rr.routes


@LPS
def test_tiny_dout_is_reported_not_asserted(ops, lp):
    """dout of about 1e-6: in the half build dS falls into half's subnormals, where the kernel's conversion and the
    emulation may differ - the ratio is measured; only finiteness is required."""
    lpt = LP()
    rng = np.random.default_rng(11)
    launch, (q16, k16, v16, do16) = _case([700, 130], 2, 0, False, lpt, rng, 1.0, dout_mag=1e-6)
    got = _kernel(lpt, q16, k16, v16, do16, launch, 2, packed=True)
    assert all(np.isfinite(g).all() for g in got)
    worst = _compare("tiny-dout", got, launch, q16, k16, v16, do16, 2, lpt, enforce=False)
    report(f"attn bwd16 tiny dout worst ratio ({lp})", ratio=worst)


@LPS
@pytest.mark.parametrize("lens", [[1, 17, 1024, 45], [1024, 100, 1024, 33]], ids=["L1-17-1024-45", "L1024-100-1024-33"])
def test_range_rows_are_finite_and_within_the_bound(ops, lp, lens):
    """Rows built like tests/test_gpu_attention_range.py's: exact scores s' = M_row + delta with M = +-130 .. +-2000, rows on
    both sides of den = 1e+-30, mixed tiles.  A backward that ran the forward's unshifted softmax without its redo would
    return inf / inf here; this one subtracts the exact row maximum."""
    H = 2
    lpt = LP()
    rng = np.random.default_rng(sum(lens))
    dup = 24
    n = sum(lens) - dup
    patches, _ = _make_patches(lens, 0, rng, dup_last=dup)
    launch = Launch(patches)
    qp, k, v = _base_rows(n, H, rng)
    rows = _assign_shifts(launch, qp, k, H, lpt)
    assert rows["over"] and rows["under"] and rows["mixed"] and rows["thr"], rows
    q16, k16, v16 = _r16(qp / _c32(), lpt), _r16(k, lpt), _r16(v, lpt)
    do16 = _r16(rng.standard_normal((n, 16 * H)) * 0.1, lpt)
    assert np.abs(_q_eff(q16, lpt)[:, ::16]).max() > 1000
    got = _kernel(lpt, q16, k16, v16, do16, launch, H, packed=True)
    worst = _compare(f"range {lens}", got, launch, q16, k16, v16, do16, H, lpt)
    report(f"attn bwd16 range worst ratio ({lp})", ratio=worst)


@LPS
def test_rows_in_two_patches_collect_both(ops, lp):
    """Rows that sit in two patches (live in the first, padding duplicates in the second) receive the sum of both patches'
    dq / dk / dv: against the oracle, and against two single-patch launches added up (fp32 atomic order: L 2^-24)."""
    H = 2
    lpt = LP()
    rng = np.random.default_rng(5)
    a = rng.permutation(300)
    b_own = 300 + rng.permutation(150)
    b_dup = rng.choice(a, 50, replace=False)
    pa = (a, a.copy(), a.copy())
    gb = np.concatenate([b_own, b_dup])
    pb = (gb, gb.copy(), np.concatenate([b_own, np.full(50, -1)]))
    both = Launch([pa, pb])
    q16, k16, v16, do16 = _inputs(450, 450, H, lpt, rng)
    got = _kernel(lpt, q16, k16, v16, do16, both, H, packed=True)
    _compare("two-patches", got, both, q16, k16, v16, do16, H, lpt)
    parts = [_kernel(lpt, q16, k16, v16, do16, Launch([p]), H, packed=True) for p in (pa, pb)]
    exact = _grads(q16, k16, v16, do16, both, H, lpt)
    for tn, g, ga, gb_, g64 in zip(("dq", "dk", "dv"), got, parts[0], parts[1], exact):
        if tn != "dq":  # (as queries the duplicates carry no output gradient; as keys they collect the second patch's)
            assert np.abs(gb_[b_dup]).max() > 0 and np.abs(ga[b_dup]).max() > 0
        d = float(np.abs(g - (ga + gb_)).max()) / float(np.abs(g64).max())
        report(f"attn bwd16 two patches vs two launches {tn}", rel_diff=d)
        assert d <= both.max_len * 2.0 ** -24, (tn, d)


@LPS
def test_agrees_with_the_fp32_form(ops, lp):
    """The fp32 form on the same 16-bit values widened to fp32: identical operands apart from q', so the two forms differ by
    no more than the 16-bit form's bound plus what the q' rounding itself moves (oracle with and without that rounding)."""
    H = 2
    lpt = LP()
    rng = np.random.default_rng(9)
    launch, (q16, k16, v16, do16) = _case([700, 1024, 33], H, 20, False, lpt, rng, 1.0)
    g16 = _kernel(lpt, q16, k16, v16, do16, launch, H, packed=True)
    g32 = _kernel(lpt, q16, k16, v16, do16, launch, H, packed=True, dtype=torch.float32)
    exact = _grads(q16, k16, v16, do16, launch, H, lpt, "exact")
    emul = _grads(q16, k16, v16, do16, launch, H, lpt, "emul")
    noround = _grads(q16, k16, v16, do16, launch, H, lpt, "noround")
    for tn, a, b, g64, ge, gn in zip(("dq", "dk", "dv"), g16, g32, exact, emul, noround):
        mag = float(np.abs(g64).max())
        diff = float(np.abs(a - b).max()) / mag
        moved = float(np.abs(g64 - gn).max()) / mag
        bound = 2 * _metric(ge, g64) + launch.max_len * 2.0 ** -24 + moved
        report(f"attn bwd16 vs fp32 form {tn}", diff=diff, q_rounding_moves=moved, bound=bound)
        assert diff <= bound, (tn, diff, bound)


@LPS
def test_overflowing_dout_is_visible_in_half_and_finite_in_bfloat16(ops, lp):
    """One dout element of 1e6 through the autograd function (fp32 dout in): the half core turns it into inf (torch's cast,
    no clamp in the kernel) and dq / dk / dv of THAT patch-head are not finite - what a GradScaler looks for - while the other
    patch-heads stay finite; the bfloat16 core computes finite gradients within the bound."""
    from cdsegnet_amd import train_graph
    H = 2
    C = 16 * H
    lpt = LP()
    rng = np.random.default_rng(3)
    launch, (q16, k16, v16, do16) = _case([300, 200], H, 0, False, lpt, rng, 1.0)
    row = int(launch.patches[1][2][17])  # an output row of patch 1; head 1
    dout = do16.copy()
    dout[row, 16 + 5] = 1e6
    qkv = dev(np.concatenate([q16, k16, v16], 1), torch.float32).requires_grad_(True)
    gq, gkv, widx, ps = launch.device()
    out = train_graph.attention_core(lp, qkv, None, C, gq, gkv, widx, ps, launch.ps.tolist(), H, launch.max_len, SCALE)
    assert out.dtype == torch.float32
    out.backward(dev(dout, torch.float32))
    torch.cuda.synchronize()
    g = qkv.grad.cpu().double().numpy()
    got = (g[:, :C], g[:, C:2 * C], g[:, 2 * C:])
    rows1 = launch.patches[1][0]
    hit = np.zeros((g.shape[0], C), dtype=bool)
    hit[np.ix_(rows1, np.arange(16, 32))] = True
    if lp == "f16":
        assert any(not np.isfinite(x[hit]).all() for x in got), "the overflow left no trace"
        for x in got:
            assert np.isfinite(x[~hit]).all(), "the overflow leaked into another patch-head"
    else:
        _compare("dout-1e6", got, launch, q16, k16, v16, _r16ns(dout, lpt), H, lpt)


@LPS
def test_argument_checks(ops, lp):
    from cdsegnet_amd import _lib
    H = 2
    lpt = LP()
    other = torch.bfloat16 if lpt == torch.float16 else torch.float16
    rng = np.random.default_rng(1)
    launch, (q16, k16, v16, do16) = _case([64, 33], H, 0, False, lpt, rng, 1.0)
    n, C = q16.shape
    gq, gkv, widx, ps = launch.device()
    psh = launch.ps.tolist()

    def call(q, k, v, do, psh_=psh, grads=None):
        dq, dk, dv = grads or tuple(torch.zeros(n, C, dtype=torch.float32, device="cuda") for _ in range(3))
        ops.attention_bwd(q, k, v, gq, gkv, widx, ps, psh_, H, SCALE, do, dq, dk, dv)
        torch.cuda.synchronize()
        return dq

    q, k, v, do = (dev(x, lpt) for x in (q16, k16, v16, do16))
    assert torch.isfinite(call(q, k, v, do)).all()  # a 16-bit call no longer raises "exact-fp32 mode only"
    with pytest.raises(_lib.CdsegError, match="do not belong to the active build"):
        call(*(dev(x, other) for x in (q16, k16, v16, do16)))
    with pytest.raises(_lib.CdsegError, match="share a dtype"):
        call(q, k, v, do.float())
    with pytest.raises(_lib.CdsegError, match="share a dtype"):
        call(q.float(), k, v, do)
    wide = torch.zeros(n, C + 4, dtype=lpt, device="cuda")  # rows of C + 4 elements: 8- but not 16-byte aligned
    wide[:, :C] = q
    with pytest.raises(_lib.CdsegError, match="16-byte aligned"):
        call(wide[:, :C], k, v, do)
    with pytest.raises(_lib.CdsegError, match="fp32"):
        call(q, k, v, do, grads=tuple(torch.zeros(n, C, dtype=lpt, device="cuda") for _ in range(3)))
    with pytest.raises(_lib.CdsegError, match="at most 1024"):
        call(q, k, v, do, psh_=[0, 1025])
    # the entry point checks the same rules itself
    lib = _lib.load()
    g = [torch.zeros(n, C, dtype=torch.float32, device="cuda") for _ in range(3)]
    ws = torch.empty(lib.cdseg_attention_bwd_ws_bytes(int(psh[-1]), H), dtype=torch.uint8, device="cuda")

    def raw(ldq, max_len, npatch=len(psh) - 1):
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        return lib.cdseg_attention_bwd(p(wide if ldq != C else q), p(k), p(v), ldq, C, C, p(gq), p(gkv), p(widx), p(ps), npatch, H,
                                       int(psh[-1]), max_len, SCALE, p(do), C, p(g[0]), p(g[1]), p(g[2]), C, C, C, _lib.BF16, p(ws),
                                       ws.numel(), None)

    assert raw(C + 4, launch.max_len) == -1  # CDSEG_ERR_ARG
    assert raw(C, 1025) == -4  # CDSEG_ERR_UNSUPPORTED
    assert raw(C, launch.max_len, npatch=0) == 0  # empty launch
    torch.cuda.synchronize()
    assert all(float(x.abs().max()) == 0 for x in g)


# ------------------------------------------------------------------------------------------ the whole training step
def _mini_model(fx, dev_, enable_flash):
    """tests/test_gpu_train.py's _mini_training_model, with the attention plan of choice: enable_flash = False is what the
    fixture was recorded with (equal-length padded patches), True is what the shipped configs train with (ragged last patches)."""
    from cdsegnet_amd import configs
    from cdsegnet_amd.param_init import fill_state_dict
    from cdsegnet_amd.registry import build_model
    import cdsegnet_amd.models  # noqa: F401
    from tests.test_gpu_train import _mini_training_model
    if not enable_flash:
        return _mini_training_model(fx, dev_)
    cfg = configs.mini_config()
    cfg["backbone"]["enable_flash"] = True
    cfg["criteria"] = [dict(type="MSELoss", loss_weight=1.0, ignore_index=-1, batch_sample_point=-1),
                       dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1),
                       dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)]
    model = build_model(cfg)
    sd = fill_state_dict(model.state_dict(), seed=int(fx["sd_seed"]))
    model.load_state_dict(sd)
    return model.to(dev_).train(), sd


def _draws(fx):
    masks = {str(k): [fx[f"mask.{i}.{j}"] for j in range(int(fx["mask_counts"][i]))] for i, k in enumerate(fx["mask_names"])}
    return dict(ts=fx["ts"], noise=fx["noise"], perms=[list(p) for p in fx["perms"]], masks=masks)


class _Calls:
    """Wraps ops.attention / ops.attention_bwd (the training graph calls them through the module): dtype and form of every
    launch.  k is a view of the packed qkv (row stride 3 C: self attention) or of the packed kv (2 C: cross attention)."""

    def __init__(self, monkeypatch):
        self.log = []
        self.lock = threading.Lock()  # (autograd runs backward on a thread of its own)
        fwd, bwd = O.attention, O.attention_bwd

        def attention(q, k, *a, **kw):
            self._add("fwd", q, k)
            return fwd(q, k, *a, **kw)

        def attention_bwd(q, k, *a, **kw):
            self._add("bwd", q, k)
            return bwd(q, k, *a, **kw)

        monkeypatch.setattr(O, "attention", attention)
        monkeypatch.setattr(O, "attention_bwd", attention_bwd)

    def _add(self, what, q, k):
        form = {3: "self", 2: "cross"}[k.stride(0) // k.shape[1]]
        with self.lock:
            self.log.append((what, q.dtype, form))

    def check(self, dtype):
        assert self.log and all(d == dtype for _, d, _ in self.log), {(w, d) for w, d, _ in self.log}
        for what in ("fwd", "bwd"):
            assert {f for w, _, f in self.log if w == what} == {"self", "cross"}, what
        assert sum(w == "fwd" for w, _, _ in self.log) == sum(w == "bwd" for w, _, _ in self.log)
        n = len(self.log)
        self.log.clear()
        return n


TPS = pytest.mark.parametrize("tp,lp", [("bf16-attn", "bf16"), ("fp16-attn", "f16")])
LOSS_CAP = {"fp16-attn": 0.012, "bf16-attn": 0.04}  # tests/test_gpu_e2e.py's whole-trunk 16-bit logit bounds (sanity cap)


def _inp(fx):
    return {k: torch.as_tensor(fx[k]).cuda() for k in ("coord", "grid_coord", "feat", "offset", "segment")}


@TPS
@pytest.mark.parametrize("flash", [False, True], ids=["padded", "flash"])
def test_step_routes_every_attention_launch_through_the_16_bit_core(ops, monkeypatch, tp, lp, flash):
    """Forward + backward with train_precision set: every attention launch (self and cross, forward and backward) is 16-bit of
    the chosen type and none is fp32; fp32 finite loss, finite gradients on the same parameters as the fp32 step.  On the
    fixture's plan (padded): the loss within the sanity cap of the recorded fp32 loss, distances to the recorded step
    reported, and "fp32" afterwards reproduces the fixture's loss."""
    fx = load_fixture("train_step_mini.npz")
    model, _ = _mini_model(fx, torch.device("cuda"), flash)
    calls = _Calls(monkeypatch)
    inp = _inp(fx)
    model.zero_grad()
    model(inp, draws=_draws(fx))["loss"].backward()
    torch.cuda.synchronize()
    calls.check(torch.float32)
    have32 = {k for k, p in model.named_parameters() if p.grad is not None}
    model.zero_grad()
    assert model.train_precision == "fp32" and "train_precision" not in model.state_dict()
    model.train_precision = tp
    out = model(inp, draws=_draws(fx))
    loss = out["loss"]
    assert loss.dtype == torch.float32 and bool(torch.isfinite(loss))
    loss.backward()
    torch.cuda.synchronize()
    nlaunch = calls.check(LP())
    named = dict(model.named_parameters())
    assert {k for k, p in named.items() if p.grad is not None} == have32
    assert all(bool(torch.isfinite(p.grad).all()) for p in named.values() if p.grad is not None)
    if not flash:
        e_loss = abs(float(loss.detach()) - float(fx["loss"]))
        names = [str(n) for n in fx["grad_names"]]
        gn = np.array([float(named[k].grad.norm()) for k in names])
        ref = fx["grad_norms"]
        rel = np.abs(gn - ref) / (ref + 1e-3 * ref.max())
        cos = 1.0
        for k in fx.files:
            if k.startswith("g."):
                a, b = named[k[2:]].grad.cpu().double().flatten(), torch.as_tensor(fx[k]).double().flatten()
                cos = min(cos, float(a @ b / (a.norm() * b.norm())))
        report(f"train step {tp} vs the reference's recorded fp32 step", attention_launches=nlaunch, loss_diff=e_loss,
               worst_grad_norm_rel=float(rel.max()), min_cosine_of_8_full_grads=cos)
        assert e_loss < LOSS_CAP[tp], e_loss
        model.zero_grad()
        model.train_precision = "fp32"
        l32 = float(model(inp, draws=_draws(fx))["loss"].detach())
        assert abs(l32 - float(fx["loss"])) < 1e-4
    else:
        report(f"train step {tp} flash plan", attention_launches=nlaunch, loss=float(loss.detach()))


def test_invalid_train_precision_raises(ops):
    fx = load_fixture("train_step_mini.npz")
    model, _ = _mini_model(fx, torch.device("cuda"), False)
    model.train_precision = "fp16"
    with pytest.raises(ValueError, match="train_precision"):
        model(_inp(fx), draws=_draws(fx))
    model.train_precision = "fp32"
    assert bool(torch.isfinite(model(_inp(fx), draws=_draws(fx))["loss"]))


@TPS
@pytest.mark.parametrize("flash", [False, True], ids=["padded", "flash"])
def test_reference_run_step_with_amp_and_grad_scaler_performs_the_step(ops, monkeypatch, tp, lp, flash):
    """The reference trainer's run_step (engines/train.py:216-271) with cfg.enable_amp = True around a 16-bit attention core:
    the scaler finds no overflow (scale unchanged by update()) and the parameters move."""
    fx = load_fixture("train_step_mini.npz")
    model, _ = _mini_model(fx, torch.device("cuda"), flash)
    model.train_precision = tp
    calls = _Calls(monkeypatch)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    opt = torch.optim.AdamW(model.parameters(), lr=0.002, weight_decay=0.05)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=0.002, total_steps=10)
    scaler = torch.cuda.amp.GradScaler()
    with torch.cuda.amp.autocast(enabled=True):
        loss = model(_inp(fx), draws=_draws(fx))["loss"]
    assert loss.dtype == torch.float32
    opt.zero_grad()
    scaler.scale(loss).backward()
    scaler.step(opt)
    scale = scaler.get_scale()
    scaler.update()
    assert scaler.get_scale() == scale, "the scaler found an overflow"
    sched.step()
    torch.cuda.synchronize()
    calls.check(LP())  # (the step did run on the 16-bit core)
    moved = max(float((p.detach() - before[k]).abs().max()) for k, p in model.named_parameters())
    report(f"run_step {tp} {'flash' if flash else 'padded'}", loss=float(loss.detach()), scale=scale, max_param_move=moved)
    assert moved > 1e-5


@TPS
@pytest.mark.parametrize("flash", [False, True], ids=["padded", "flash"])
def test_four_steps_on_one_batch_descend(ops, monkeypatch, tp, lp, flash):
    fx = load_fixture("train_step_mini.npz")
    model, _ = _mini_model(fx, torch.device("cuda"), flash)
    model.train_precision = tp
    calls = _Calls(monkeypatch)
    opt = torch.optim.AdamW(model.parameters(), lr=0.002, weight_decay=0.05)
    inp = _inp(fx)
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss = model(inp, draws=_draws(fx))["loss"]
        loss.backward()
        assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in model.parameters())
        losses.append(float(loss.detach()))
        opt.step()
    torch.cuda.synchronize()
    calls.check(LP())
    report(f"4 steps {tp} {'flash' if flash else 'padded'}", l0=losses[0], l1=losses[1], l2=losses[2], l3=losses[3])
    assert np.isfinite(losses).all() and all(b < a for a, b in zip(losses, losses[1:])), losses
