"""GPU: attention dropout and element dropout (include/cdseg.h "dropout"; csrc/attention_drop.hip, the mask variants of the
four attention backward kernels in csrc/train.hip), both builds of the library.

The mask is restated in tests/dropout_mask.py from the header's text on top of oracle/philox.py.  The fp64 oracle is that of
tests/test_gpu_attention_bwd16.py with the mask:  P = softmax over all keys,  O = (f o P) V  with f = M / keep,
dP = (dO V^T) o f,  D = sum_j P dP,  dS = P (dP - D),  dq = c ln 2 dS k,  dk = ln 2 dS^T q',  dv = (f o P)^T dO.

Tolerances.  16-bit: that file's rule, kernel error <= 2 E_ref + L 2^-24 per tensor (metric max |x - x64| / max |x64|), E_ref
the error of an fp64 emulation that rounds where flash-attention rounds: f o P as the operand of dv and of the forward's P V,
dS as the operand of dq and dk, and - the forward's output being a tensor of the 16-bit type there as here - the stored O.
fp32: the existing ops.attention / ops.attention_bwd run on the same inputs in the same test and are measured against the
UNMASKED oracle; the dropout kernels must stay within twice that error plus L 2^-24 (the mask adds one multiplication per
element and no accumulation step).
"""
import ctypes

import numpy as np
import pytest
import torch

from cdsegnet_amd import _lib
from cdsegnet_amd import ops as O
from tests import dropout_mask as DM
from tests import guard_bands as GB
from tests.test_gpu_attention_bwd16 import LN2, SCALE, _case, _metric, _q_eff, _r16ns
from tests.test_gpu_attention_range import Launch, _c32, _make_patches, _r16
from tests.test_gpu_ops import LP, _library_variant, dev, ops, report  # noqa: F401  (fixtures: lp="f16" -> the half build)

pytestmark = pytest.mark.gpu

LPS = pytest.mark.parametrize("lp", ["bf16", "f16"])
SEED, OFFSET = 0x1234_5678_9ABC_DEF0, 0x0FED_CBA9_8765_4321  # (both halves of both words in use)

_MASKS = {}


def _masks(rate, lens, H, seed=SEED, offset=OFFSET):
    """The helper's masks of a launch, computed once per (site, rate, lengths, heads) and shared."""
    key = (seed, offset, rate, tuple(int(x) for x in lens), H)
    if key not in _MASKS:
        m = DM.attention_mask(seed, offset, rate, lens, H)
        for a in m:
            a.setflags(write=False)
        _MASKS[key] = m
    return _MASKS[key]


def _lens(launch):
    return np.diff(launch.ps).tolist()


# ------------------------------------------------------------------------------------------ fp64 oracle with the mask
def _oracle(q, k, v, do, launch, H, lp, masks, rate, mode="exact", scale=SCALE):
    """fp64 (out (q rows), dq, dk, dv).  lp: the 16-bit type (q' rounded once as the kernels do), or None for the fp32 form.
    masks None: no dropout.  mode "emul": the 16-bit roundings of the module docstring."""
    c = _c32(scale)
    qe = q * c if lp is None else _q_eff(q, lp, scale)
    f_keep = float(DM.inv_keep(rate)) if masks is not None else 1.0
    out = np.zeros_like(q)
    dq, dk, dv = np.zeros_like(q), np.zeros_like(k), np.zeros_like(v)
    for p, (gq, gkv, widx) in enumerate(launch.patches):
        live = widx >= 0
        for h in range(H):
            sl = slice(16 * h, 16 * h + 16)
            K, V = k[gkv][:, sl], v[gkv][:, sl]
            dO = np.where(live[:, None], do[np.where(live, widx, 0)][:, sl], 0.0)
            S = qe[gq][:, sl] @ K.T
            P = np.exp2(S - S.max(1, keepdims=True))
            P /= P.sum(1, keepdims=True)
            f = masks[p][h] * f_keep if masks is not None else 1.0
            dP = (dO @ V.T) * f
            D = (P * dP).sum(1, keepdims=True)
            dS = P * (dP - D)
            Pf = P * f
            if mode == "emul":
                Pf, dS = _r16ns(Pf, lp), _r16ns(dS, lp)
            o = Pf @ V
            if mode == "emul":
                o = _r16(o, lp)
            out[widx[live], sl] = o[live]
            np.add.at(dq[:, sl], gq, c * LN2 * (dS @ K))
            np.add.at(dk[:, sl], gkv, LN2 * (dS.T @ qe[gq][:, sl]))
            np.add.at(dv[:, sl], gkv, Pf.T @ dO)
    return out, dq, dk, dv


def _run(t, q, k, v, do, launch, H, rate, packed=False, seed=SEED, offset=OFFSET, scale=SCALE):
    """The dropout ops (rate is None: the existing ops.attention / ops.attention_bwd) on the device -> fp64 (out, dq, dk, dv).
    packed: q / k / v are strided views of one (n, 3 C) buffer and dq / dk / dv views of one fp32 (n, 3 C) buffer."""
    n, C = q.shape
    if packed:
        qkv = dev(np.concatenate([q, k, v], 1), t)
        qd, kd, vd = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
        g = torch.zeros(n, 3 * C, dtype=torch.float32, device="cuda")
        dq, dk, dv = g[:, :C], g[:, C:2 * C], g[:, 2 * C:]
    else:
        qd, kd, vd = dev(q, t), dev(k, t), dev(v, t)
        dq = torch.zeros(q.shape, dtype=torch.float32, device="cuda")
        dk, dv = (torch.zeros(k.shape, dtype=torch.float32, device="cuda") for _ in range(2))
    gq, gkv, widx, ps = launch.device()
    out = torch.zeros(n, C, dtype=t, device="cuda")
    dod = dev(do, t)
    if rate is None:
        O.attention(qd, kd, vd, gq, gkv, widx, ps, H, launch.max_len, scale, out)
        O.attention_bwd(qd, kd, vd, gq, gkv, widx, ps, launch.ps.tolist(), H, scale, dod, dq, dk, dv)
    else:
        O.attention_drop(qd, kd, vd, gq, gkv, widx, ps, H, launch.max_len, scale, out, rate, seed, offset)
        O.attention_drop_bwd(qd, kd, vd, gq, gkv, widx, ps, launch.ps.tolist(), H, scale, dod, dq, dk, dv, rate, seed, offset)
    torch.cuda.synchronize()
    return tuple(x.cpu().double().numpy() for x in (out, dq, dk, dv))


# ------------------------------------------------------------------------------------------ 1. the mask, bit for bit
J0 = [0, 3, 4, 15, 16, 31, 32, -1]  # -1: the patch's last slot
MASK_LENS = [32, 64, 1024]
MASK_RATE = 0.25


def _identity_launch(lens, rng):
    patches, n = _make_patches(lens, 0, rng)
    return Launch(patches), n


@LPS
@pytest.mark.parametrize("form", ["fp32", "lp"])
@pytest.mark.parametrize("H", [2, 32])
def test_forward_draws_the_mask_of_the_header(ops, lp, form, H):
    """q = 0: P = 1 / L exactly.  v is zero except a one at (slot j0_d, head dim d) for the d-th j0 of the list, so output
    (row of slot i, head h, dim d) = M[i, j0_d] / (keep L): zero / non-zero pattern and value, every row, every head."""
    t = torch.float32 if form == "fp32" else LP()
    rng = np.random.default_rng(H)
    launch, n = _identity_launch(MASK_LENS, rng)
    masks = _masks(MASK_RATE, MASK_LENS, H)
    q = np.zeros((n, 16 * H))
    k = rng.standard_normal((n, 16 * H))  # (q = 0: the keys do not matter)
    v = np.zeros((n, 16 * H))
    for gq, gkv, widx in launch.patches:
        for d, j0 in enumerate(J0):
            v[gkv[j0 % len(gkv)], d::16] = 1.0
    out = _run(t, q, k, v, np.zeros_like(q), launch, H, MASK_RATE)[0]
    f = float(DM.inv_keep(MASK_RATE))
    for p, (gq, gkv, widx) in enumerate(launch.patches):
        L = len(gq)
        val = np.float32(f) / np.float32(L)  # (L is a power of two: exact)
        val = float(val) if form == "fp32" else float(_r16(np.array([float(val)]), LP())[0])
        for h in range(H):
            got = out[widx][:, 16 * h:16 * h + 16]  # (slot i, dim d)
            for d, j0 in enumerate(J0):
                want = np.where(masks[p][h][:, j0 % L], val, 0.0)
                bad = np.flatnonzero(got[:, d] != want)
                assert bad.size == 0, (f"patch {p} (L = {L}) head {h} key {j0 % L}: {bad.size} queries differ, first {bad[:5]}: "
                                       f"got {got[bad[:5], d]}, want {want[bad[:5]]}")
            assert not got[:, len(J0):].any()


@LPS
@pytest.mark.parametrize("form", ["fp32", "lp"])
@pytest.mark.parametrize("H", [2, 32])
def test_backward_draws_the_same_mask(ops, lp, form, H):
    """The same q = 0 input, v = 1, dout one-hot in (row of slot i0, dim 0 of every head).
    kv side: dv[key j, dim 0] = M[i0, j] / (keep L), pattern and value.
    q side:  dP[i0, j] = M[i0, j] / keep, D = mean_j dP, dS = (dP - D) / L, and with k one-hot at (slot j0_d, dim d):
             dq[i0, d] = scale (M[i0, j0_d] / keep - D) / L - the mask row decides the sign."""
    t = torch.float32 if form == "fp32" else LP()
    rng = np.random.default_rng(100 + H)
    launch, n = _identity_launch(MASK_LENS, rng)
    masks = _masks(MASK_RATE, MASK_LENS, H)
    q = np.zeros((n, 16 * H))
    v = np.ones((n, 16 * H))
    k = np.zeros((n, 16 * H))
    do = np.zeros((n, 16 * H))
    i0s = []
    for gq, gkv, widx in launch.patches:
        L = len(gq)
        i0 = min(37, L - 1)
        i0s.append(i0)
        do[widx[i0], 0::16] = 1.0
        for d, j0 in enumerate(J0):
            k[gkv[j0 % L], d::16] = 1.0
    _, dq, dk, dv = _run(t, q, k, v, do, launch, H, MASK_RATE)
    f = float(DM.inv_keep(MASK_RATE))
    assert not dk.any()  # (q = 0)
    for p, (gq, gkv, widx) in enumerate(launch.patches):
        L, i0 = len(gq), i0s[p]
        val = np.float32(f) / np.float32(L)
        val = float(val) if form == "fp32" else float(_r16(np.array([float(val)]), LP())[0])
        for h in range(H):
            row = masks[p][h][i0]  # (L,) keep of (i0, j)
            got = dv[gkv][:, 16 * h]
            want = np.where(row, val, 0.0)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, f"dv: patch {p} head {h} query {i0}: {bad.size} keys differ, first {bad[:5]}"
            D = row.sum() * f / L
            for d, j0 in enumerate(J0):  # (dim d is set in the one key j0_d only)
                want_q = SCALE * (row[j0 % L] * f - D) / L
                gotq = dq[gq[i0], 16 * h + d]
                assert abs(gotq - want_q) <= 2.0 ** -7 * abs(SCALE * f / L), (p, h, d, gotq, want_q)
                assert (gotq > 0) == bool(row[j0 % L])


# ------------------------------------------------------------------------------------------ 2. forward and gradients against fp64
# (name, patch lengths, heads, padding duplicates of the last patch, cross attention, packed strided views, sigma of k)
CASES = [
    ("ragged", [1, 31, 32, 33, 63, 65], 2, 0, False, True, 3.0),
    ("L64-1-130", [64, 1, 130], 8, 0, False, False, 1.0),
    ("dups", [200, 1024, 300], 2, 100, False, True, 1.0),
    ("cross", [512, 65, 1024], 2, 40, True, False, 3.0),
]
NAMES = ("out", "dq", "dk", "dv")


@LPS
@pytest.mark.parametrize("rate", [0.1, 0.5])
@pytest.mark.parametrize("name,lens,H,dup,cross,packed,sigma_k", CASES, ids=[c[0] for c in CASES])
def test_16_bit_forward_and_gradients_vs_fp64(ops, lp, name, lens, H, dup, cross, packed, sigma_k, rate):
    lpt = LP()
    rng = np.random.default_rng(sum(lens) + 31 * H + dup)
    launch, (q, k, v, do) = _case(lens, H, dup, cross, lpt, rng, sigma_k)
    masks = _masks(rate, _lens(launch), H)
    got = _run(lpt, q, k, v, do, launch, H, rate, packed=packed and not cross)
    exact = _oracle(q, k, v, do, launch, H, lpt, masks, rate)
    emul = _oracle(q, k, v, do, launch, H, lpt, masks, rate, "emul")
    for tn, g, g64, ge in zip(NAMES, got, exact, emul):
        assert np.isfinite(g).all(), tn
        if not np.abs(g64).max() > 0:
            assert np.abs(g).max() == 0
            continue
        err, eref = _metric(g, g64), _metric(ge, g64)
        bound = 2 * eref + launch.max_len * 2.0 ** -24
        report(f"attn drop16 {name} rate {rate} {tn} ({lp})", kernel_err=err, E_ref=eref, bound=bound)
        assert err <= bound, (name, tn, err, eref, bound)


@pytest.mark.parametrize("rate", [0.1, 0.5])
@pytest.mark.parametrize("name,lens,H,dup,cross,packed,sigma_k", CASES, ids=[c[0] for c in CASES])
def test_fp32_forward_and_gradients_vs_fp64(ops, name, lens, H, dup, cross, packed, sigma_k, rate):
    rng = np.random.default_rng(sum(lens) + 31 * H + dup)
    launch, (q, k, v, do) = _case(lens, H, dup, cross, torch.bfloat16, rng, sigma_k)  # (dyadic inputs: exact in fp32)
    masks = _masks(rate, _lens(launch), H)
    pk = packed and not cross
    got = _run(torch.float32, q, k, v, do, launch, H, rate, packed=pk)
    plain = _run(torch.float32, q, k, v, do, launch, H, None, packed=pk)
    exact = _oracle(q, k, v, do, launch, H, None, masks, rate)
    exact_plain = _oracle(q, k, v, do, launch, H, None, None, rate)
    for tn, g, g64, gp, gp64 in zip(NAMES, got, exact, plain, exact_plain):
        assert np.isfinite(g).all(), tn
        if not np.abs(g64).max() > 0:
            assert np.abs(g).max() == 0
            continue
        err, base = _metric(g, g64), _metric(gp, gp64)
        bound = 2 * base + launch.max_len * 2.0 ** -24
        report(f"attn drop fp32 {name} rate {rate} {tn}", kernel_err=err, existing_kernel_err=base, bound=bound)
        assert err <= bound, (name, tn, err, base, bound)


# ------------------------------------------------------------------------------------------ 3. rate 0 and the threshold edge
@LPS
@pytest.mark.parametrize("form", ["fp32", "lp"])
def test_rate_0_is_the_existing_attention_bit_for_bit(ops, lp, form):
    t = torch.float32 if form == "fp32" else LP()
    rng = np.random.default_rng(7)
    launch, (q, k, v, do) = _case([200, 1024, 300], 2, 100, False, LP(), rng, 1.0)
    assert O.dropout_keep(0.0) == 1.0 and O.dropout_keep(1.0 / 1024) == 1.0 and O.dropout_keep(1.0 / 256) == 255.0 / 256
    a = _run(t, q, k, v, do, launch, 2, 0.0, packed=True)
    b = _run(t, q, k, v, do, launch, 2, None, packed=True)
    for tn, x, y in zip(NAMES, a, b):
        assert np.array_equal(x, y), tn
    c = _run(t, q, k, v, do, launch, 2, 1.0 / 1024, packed=True)  # (T would still be 256: nothing is dropped)
    assert all(np.array_equal(x, y) for x, y in zip(c, b))
    x = dev(rng.standard_normal((77, 40)), torch.float32)
    assert GB.same_bits(O.dropout(x, 0.0, SEED, OFFSET), x)


# ------------------------------------------------------------------------------------------ 4. element dropout
@pytest.mark.parametrize("m,c", [(1, 16), (77, 32), (1000, 200), (513, 2048), (33, 7)])
def test_element_dropout_is_x_times_the_mask(ops, m, c):
    rng = np.random.default_rng(m + c)
    rate = 0.25
    x = rng.standard_normal((m, c)).astype(np.float32)
    f = DM.inv_keep(rate)
    want = np.where(DM.element_mask(SEED, OFFSET, rate, m, c), x * f, np.float32(0.0))
    xd = dev(x)
    y = O.dropout(xd, rate, SEED, OFFSET)
    assert np.array_equal(y.cpu().numpy(), want)
    kept = float((y != 0).float().mean())
    report(f"dropout ({m}, {c})", kept=kept, keep=O.dropout_keep(rate))
    # a strided view (odd row stride and a column shift: the scalar path), then in place
    buf = torch.full((m, c + 5), 7.0, device="cuda")
    view = buf[:, 3:3 + c]
    view.copy_(xd)
    out = torch.full((m, c + 9), -3.0, device="cuda")
    O.dropout(view, rate, SEED, OFFSET, out=out[:, 1:1 + c])
    assert np.array_equal(out[:, 1:1 + c].cpu().numpy(), want)
    assert bool((out[:, :1] == -3.0).all()) and bool((out[:, 1 + c:] == -3.0).all())
    O.dropout(view, rate, SEED, OFFSET, out=view)
    assert np.array_equal(view.cpu().numpy(), want)
    assert bool((buf[:, :3] == 7.0).all()) and bool((buf[:, 3 + c:] == 7.0).all())
    O.dropout(xd, rate, SEED, OFFSET, out=xd)
    assert np.array_equal(xd.cpu().numpy(), want)
    # its own backward
    dy = rng.standard_normal((m, c)).astype(np.float32)
    dx = O.dropout(dev(dy), rate, SEED, OFFSET)
    assert np.array_equal(dx.cpu().numpy(), np.where(DM.element_mask(SEED, OFFSET, rate, m, c), dy * f, np.float32(0.0)))


# ------------------------------------------------------------------------------------------ 5. memory contract
@LPS
@pytest.mark.parametrize("form", ["fp32", "lp"])
@pytest.mark.parametrize("lens", [[1], [1024, 1, 33]], ids=["L1", "L1024-1-33"])
def test_attention_entry_points_between_guard_bands(ops, monkeypatch, lp, form, lens):
    t = torch.float32 if form == "fp32" else LP()
    H = 2
    C = 16 * H
    rng = np.random.default_rng(len(lens))
    launch, (q, k, v, do) = _case(lens, H, 0, False, LP(), rng, 1.0)
    n = q.shape[0]
    ins = [GB.poisoned_input(dev(x, t), name=nm) for x, nm in zip((q, k, v, do), ("q", "k", "v", "dout"))]
    (qd, kd, vd, dod) = (i[0] for i in ins)
    idx = launch.device()
    gq, cq = GB.guard_index(idx[0])
    gkv, ckv = GB.guard_index(idx[1])
    widx, cw = GB.guard_index(idx[2], none=-1)
    ps, cp = GB.guard_index(idx[3])
    out, ob = GB.banded((n, C), t, fill=-77.0, name="out")
    grads = [GB.banded((n, C), torch.float32, fill=0.0, name=nm) for nm in ("dq", "dk", "dv")]
    served = GB.ExactWorkspaces()
    monkeypatch.setattr(O, "_scratch", served)
    O.attention_drop(qd, kd, vd, gq, gkv, widx, ps, H, launch.max_len, SCALE, out, 0.5, SEED, OFFSET)
    for g, _ in grads:
        g.zero_()
    O.attention_drop_bwd(qd, kd, vd, gq, gkv, widx, ps, launch.ps.tolist(), H, SCALE, dod, grads[0][0], grads[1][0], grads[2][0],
                         0.5, SEED, OFFSET)
    torch.cuda.synchronize()
    ob.check()
    for _, b in grads:
        b.check()
    for _, b in ins:
        b.check()
    for c in (cq, ckv, cw, cp):
        c()
    served.check(at_least=1)
    masks = _masks(0.5, _lens(launch), H)
    want = _oracle(q, k, v, do, launch, H, None if form == "fp32" else LP(), masks, 0.5)
    got = (out,) + tuple(g for g, _ in grads)
    for tn, g, w in zip(NAMES, got, want):
        g = g.cpu().double().numpy()
        assert np.isfinite(g).all(), tn  # (no NaN of a guard was read)
        if np.abs(w).max() > 0:
            assert _metric(g, w) < (1e-4 if form == "fp32" else 0.05), tn


@pytest.mark.parametrize("m,c", [(1, 1), (1, 16), (300, 50)])
def test_dropout_between_guard_bands(ops, m, c):
    rng = np.random.default_rng(m)
    x = rng.standard_normal((m, c)).astype(np.float32)
    want = np.where(DM.element_mask(SEED, OFFSET, 0.5, m, c), x * DM.inv_keep(0.5), np.float32(0.0))
    for align, cols in ((0, 8), (8, 3)):
        xi, xb = GB.poisoned_input(dev(x), cols=cols, align=align)
        y, yb = GB.banded((m, c), torch.float32, fill=-77.0, cols=cols, align=align)
        O.dropout(xi, 0.5, SEED, OFFSET, out=y)
        torch.cuda.synchronize()
        xb.check()
        yb.check()
        assert np.array_equal(y.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------ 6. determinism, argument checks
@LPS
def test_equal_sites_give_equal_bits_and_another_offset_another_mask(ops, lp):
    rng = np.random.default_rng(2)
    launch, (q, k, v, do) = _case([130, 64], 2, 0, False, LP(), rng, 1.0)
    for t in (torch.float32, LP()):
        a = _run(t, q, k, v, do, launch, 2, 0.5)
        b = _run(t, q, k, v, do, launch, 2, 0.5)
        c = _run(t, q, k, v, do, launch, 2, 0.5, offset=OFFSET + 1)
        d = _run(t, q, k, v, do, launch, 2, 0.5, seed=SEED + 1)
        assert np.array_equal(a[0], b[0]), "forward"
        for x, y in zip(a[1:], b[1:]):  # (a row sits in one slot here: one atomic per element)
            assert np.array_equal(x, y)
        assert not np.array_equal(a[0], c[0]) and not np.array_equal(a[0], d[0]) and not np.array_equal(c[0], d[0])
    x = dev(rng.standard_normal((64, 64)), torch.float32)
    assert torch.equal(O.dropout(x, 0.5, 1, 2), O.dropout(x, 0.5, 1, 2))
    assert not torch.equal(O.dropout(x, 0.5, 1, 2), O.dropout(x, 0.5, 1, 3))


@LPS
def test_argument_checks(ops, lp):
    H = 2
    C = 16 * H
    lpt = LP()
    rng = np.random.default_rng(1)
    launch, (q16, k16, v16, do16) = _case([64, 33], H, 0, False, lpt, rng, 1.0)
    n = q16.shape[0]
    gq, gkv, widx, ps = launch.device()
    psh = launch.ps.tolist()
    q, k, v, do = (dev(x, lpt) for x in (q16, k16, v16, do16))
    out = torch.zeros(n, C, dtype=lpt, device="cuda")
    g = [torch.zeros(n, C, dtype=torch.float32, device="cuda") for _ in range(3)]
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(_lib.CdsegError, match="rate"):
            ops.attention_drop(q, k, v, gq, gkv, widx, ps, H, launch.max_len, SCALE, out, bad, 1, 2)
        with pytest.raises(_lib.CdsegError, match="rate"):
            ops.attention_drop_bwd(q, k, v, gq, gkv, widx, ps, psh, H, SCALE, do, *g, bad, 1, 2)
        with pytest.raises(_lib.CdsegError, match="rate"):
            ops.dropout(g[0], bad, 1, 2)
        with pytest.raises(_lib.CdsegError, match="rate"):
            ops.dropout_keep(bad)
    with pytest.raises(_lib.CdsegError, match="share a dtype"):
        ops.attention_drop(q, k, v.float(), gq, gkv, widx, ps, H, launch.max_len, SCALE, out, 0.5, 1, 2)
    # the entry points check the same rules themselves, before any launch
    lib = _lib.load()
    ws = torch.empty(lib.cdseg_attention_bwd_ws_bytes(int(psh[-1]), H), dtype=torch.uint8, device="cuda")
    wide = torch.zeros(n, C + 4, dtype=lpt, device="cuda")  # rows of C + 4 elements: 8- but not 16-byte aligned
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def fwd(rate=0.5, ldq=C, max_len=launch.max_len, ldo=C):
        return lib.cdseg_attention_drop(p(wide if ldq != C else q), p(k), p(v), ldq, C, C, p(gq), p(gkv), p(widx), p(ps), len(psh) - 1,
                                        H, max_len, SCALE, p(wide if ldo != C else out), ldo, _lib.BF16, rate, 1, 2, None)

    def bwd(rate=0.5, ldq=C, max_len=launch.max_len):
        return lib.cdseg_attention_drop_bwd(p(wide if ldq != C else q), p(k), p(v), ldq, C, C, p(gq), p(gkv), p(widx), p(ps),
                                            len(psh) - 1, H, int(psh[-1]), max_len, SCALE, p(do), C, p(g[0]), p(g[1]), p(g[2]), C, C, C,
                                            _lib.BF16, p(ws), ws.numel(), rate, 1, 2, None)

    ERR_ARG = -1
    for f in (fwd, bwd):
        assert f(rate=1.0) == ERR_ARG and f(rate=-0.5) == ERR_ARG and f(rate=float("nan")) == ERR_ARG
        assert f(ldq=C + 4) == ERR_ARG
        assert f(max_len=1025) == ERR_ARG
    assert fwd(ldo=C + 4) == ERR_ARG
    x = torch.zeros(8, 16, device="cuda")
    assert lib.cdseg_dropout(p(x), 16, p(x), 16, 8, 16, 1.0, 1, 2, None) == ERR_ARG
    assert lib.cdseg_dropout(p(x), 8, p(x), 16, 8, 16, 0.5, 1, 2, None) == ERR_ARG  # ld < c
    assert lib.cdseg_dropout(None, 16, p(x), 16, 8, 16, 0.5, 1, 2, None) == ERR_ARG
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0 and all(float(t.abs().max()) == 0 for t in g) and float(x.abs().max()) == 0


# ------------------------------------------------------------------------------------------ 7. one Block, one cross block
# `TrainGraph._block` / `_cross_block` in the autograd mode on tests/test_gpu_train_block.py's hand-built plan (two scenes, a
# real kernel map, patch size 64 with a padded last patch) against an fp64 torch chain that applies the helper's masks at the
# sites the graph reports (`TrainGraph.dropout_sites`).
BLOCK_ROWS = [160, 140]
BLOCK_RATE = 0.25
BLOCK_SITE = (0x5EED_0000_0000_0007, 1000)  # (seed, first offset) of the pinned forward


def _init_params(mod, rng):
    """tests/test_gpu_train.py's scales: vectors 0.1 (LayerNorm weights around 1), matrices 0.3, the 27-offset kernel 0.3 / sqrt 27."""
    with torch.no_grad():
        for name, p in mod.named_parameters():
            scale = {1: 0.1, 2: 0.3, 5: 0.3 / 27 ** 0.5}[p.dim()]
            v = rng.standard_normal(tuple(p.shape)) * scale
            if p.dim() == 1 and name.endswith(".weight"):
                v = v + 1.0
            p.copy_(torch.as_tensor(v, dtype=torch.float32))


def _attn64(q, k, v, plan, H, scale, rate, site):
    """fp64 attention on the plan's slots with the site's mask (site None: no dropout)."""
    from tests.emu_dropout_ops import _patch_attention_drop
    order = torch.as_tensor(plan["order"])
    seed, offset = site if site is not None else (0, 0)
    o = _patch_attention_drop(q[order], k[order], v[order], np.asarray(plan["cu"], dtype=np.int64), H, scale,
                              rate if site is not None else 0.0, seed, offset)
    return o[torch.as_tensor(plan["inverse"])]


def _drop64(x, rate, site):
    if site is None:
        return x
    m = DM.element_mask(site[0], site[1], rate, x.shape[0], x.shape[1])
    return x * (torch.as_tensor(m).double() * float(DM.inv_keep(rate)))


def _mlp64(h, mlp, rate, sites, name):
    import torch.nn.functional as F
    h = _drop64(F.gelu(mlp.fc1(h)), rate, sites.get(name + ".mlp.0.drop.0"))
    return _drop64(mlp.fc2(h), rate, sites.get(name + ".mlp.0.drop.1"))


def _cpe64(x, seq, plan):
    from oracle import model as OM
    return seq[2](seq[1](OM.subm_conv3d(x, plan["nbr"], seq[0].weight, seq[0].bias)))


def _block64(blk, plan, x_in, dy, H, sites):
    """-> {name: fp64 tensor}: y, dx_in and every parameter gradient of the Block with the masks of `sites` ({} = no dropout)."""
    import copy
    b = copy.deepcopy(blk).cpu().double()
    C = x_in.shape[1]
    xi = torch.as_tensor(x_in).double().requires_grad_(True)
    x0 = xi + _cpe64(xi, b.cpe, plan)
    qkv = b.attn.qkv(b.norm1[0](x0))
    o = _attn64(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], plan, H, b.attn.scale, BLOCK_RATE, sites.get("blk.attn.attn_drop"))
    x1 = x0 + _drop64(b.attn.proj(o), BLOCK_RATE, sites.get("blk.attn.proj_drop"))
    y = x1 + _mlp64(b.norm2[0](x1), b.mlp[0], BLOCK_RATE, sites, "blk")
    (y * torch.as_tensor(dy).double()).sum().backward()
    out = {"y": y.detach(), "dx_in": xi.grad}
    out.update({k: p.grad for k, p in b.named_parameters()})
    return out


def _cross64(cb, plan, xq_in, xkv_in, dy, H, sites):
    import copy
    b = copy.deepcopy(cb).cpu().double()
    C = xq_in.shape[1]
    xq0 = torch.as_tensor(xq_in).double().requires_grad_(True)
    xkv0 = torch.as_tensor(xkv_in).double().requires_grad_(True)
    xq = xq0 + _cpe64(xq0, b.q_cpe, plan)
    xkv = xkv0 + _cpe64(xkv0, b.kv_cpe, plan)
    q = b.attn.q(b.q_norm1[0](xq))
    kv = b.attn.kv(b.kv_norm1[0](xkv))
    o = _attn64(q, kv[:, :C], kv[:, C:], plan, H, b.attn.scale, BLOCK_RATE, sites.get("blk.attn.attn_drop"))
    x = xq + b.tm_feat * _drop64(b.attn.proj(o), BLOCK_RATE, sites.get("blk.attn.proj_drop"))
    y = x + _mlp64(b.q_norm2[0](x), b.mlp[0], BLOCK_RATE, sites, "blk")
    (y * torch.as_tensor(dy).double()).sum().backward()
    out = {"y": y.detach(), "dx_q": xq0.grad, "dx_kv": xkv0.grad}
    out.update({k: p.grad for k, p in b.named_parameters()})
    return out


def _run_graph(mod, plan, xs, dy, tp, rates, cross):
    """The module through TrainGraph in the autograd mode -> ({name: fp32 result}, {site name: (seed, offset)})."""
    import cdsegnet_amd.train_graph as TG
    from tests.test_gpu_train_block import _graph
    for m in (mod, mod.attn):
        m.attn_drop, m.proj_drop = rates
    mod.zero_grad()
    n = plan["n"]
    g = _graph(tp, "autograd", True)
    g._site, g.dropout_sites = [BLOCK_SITE[0], BLOCK_SITE[1], True], []
    ins = [torch.as_tensor(x).cuda().requires_grad_(True) for x in xs]
    rows = torch.arange(n, dtype=torch.int32).cuda()
    if cross:
        qst, kvst = (TG._St(plan["lv"], x, [0], rows) for x in ins)
        g._cross_block(qst, kvst, mod, "blk", None)
        y = qst.x
    else:
        st = TG._St(plan["lv"], ins[0], [0], rows)
        st.conv = None
        y = g._block(st, mod, "blk", None, None).x
    y.backward(torch.as_tensor(dy).cuda())
    torch.cuda.synchronize()
    out = {"y": y.detach()}
    out.update(dict(zip(("dx_q", "dx_kv") if cross else ("dx_in",), (x.grad for x in ins))))
    out.update({k: p.grad for k, p in mod.named_parameters()})
    assert all(v is not None for v in out.values()), [k for k, v in out.items() if v is None]
    return {k: v.cpu().double() for k, v in out.items()}, {name: (s, o) for name, s, o in g.dropout_sites}


BLOCK_TPS = pytest.mark.parametrize("tp,lp", [("fp32", "bf16"), ("fp16-amp", "f16"), ("bf16-amp", "bf16")])


@BLOCK_TPS
@pytest.mark.parametrize("cross", [False, True], ids=["block", "cross_block"])
def test_block_with_dropout_vs_fp64_chain_with_the_helpers_masks(ops, tp, lp, cross):
    """C = 32, H = 2, 300 rows in two scenes, attn_drop = proj_drop = 0.25, drop path off: output, input gradients and every
    parameter gradient.  fp32: tests/test_gpu_train.py's Block bounds (|y - y64| < 1e-3; gradients < 1e-3 max(1, max |g64|)).
    AMP: the bound of that mode's Block test (tests/test_gpu_train_block.py): error <= 3 E_auto + 2^-24 per tensor, E_auto the
    error of the same module WITHOUT dropout in the same mode against the fp64 chain without masks, measured here."""
    from cdsegnet_amd import models
    from tests.test_gpu_train_block import PATCH, _plan
    C, H = 32, 2
    plan = _plan(BLOCK_ROWS)
    n = plan["n"]
    rng = np.random.default_rng(77 + cross)
    if cross:
        mod = models.CrossBlock(C, C, H, PATCH, PATCH, enable_flash=True, attn_drop=BLOCK_RATE, proj_drop=BLOCK_RATE).cuda()
    else:
        mod = models.Block(C, H, patch_size=PATCH, enable_flash=True, attn_drop=BLOCK_RATE, proj_drop=BLOCK_RATE).cuda()
    _init_params(mod, rng)
    xs = [rng.standard_normal((n, C)).astype(np.float32) for _ in range(2 if cross else 1)]
    dy = rng.standard_normal((n, C)).astype(np.float32)
    ref_fn = (lambda sites: _cross64(mod, plan, xs[0], xs[1], dy, H, sites)) if cross else \
        (lambda sites: _block64(mod, plan, xs[0], dy, H, sites))
    got, sites = _run_graph(mod, plan, xs, dy, tp, (BLOCK_RATE, BLOCK_RATE), cross)
    assert sorted(o for _, o in sites.values()) == [BLOCK_SITE[1] + i for i in range(4)] and len(sites) == 4
    assert set(sites) == {"blk.attn.attn_drop", "blk.attn.proj_drop", "blk.mlp.0.drop.0", "blk.mlp.0.drop.1"}
    ref = ref_fn(sites)
    assert set(got) == set(ref)
    plain, no_sites = _run_graph(mod, plan, xs, dy, tp, (0.0, 0.0), cross)
    assert no_sites == {}
    ref_plain = ref_fn({})
    assert float((ref["y"] - ref_plain["y"]).abs().max()) > 0.1  # (the masks do something)
    over = []
    for k, g64 in ref.items():
        assert bool(torch.isfinite(got[k]).all()), k
        if tp == "fp32":
            e = float((got[k] - g64).abs().max()) / (1.0 if k == "y" else max(1.0, float(g64.abs().max())))
            bound = 1e-3
            base = float((plain[k] - ref_plain[k]).abs().max()) / (1.0 if k == "y" else max(1.0, float(ref_plain[k].abs().max())))
        else:
            e = float((got[k] - g64).abs().max()) / float(g64.abs().max())
            base = float((plain[k] - ref_plain[k]).abs().max()) / float(ref_plain[k].abs().max())
            bound = 3 * base + 2.0 ** -24
        report(f"{'cross block' if cross else 'Block'} dropout {tp} {k}", err=e, err_without_dropout=base, bound=bound)
        if e > bound:
            over.append((k, e, bound))
    assert not over, over


# ------------------------------------------------------------------------------------------ 8. the model honours the switches
def _drop_model(fx, attn_drop, proj_drop):
    from cdsegnet_amd import configs
    from cdsegnet_amd.param_init import fill_state_dict
    from cdsegnet_amd.registry import build_model
    import cdsegnet_amd.models  # noqa: F401
    cfg = configs.mini_config()
    cfg["backbone"].update(enable_flash=False, attn_drop=attn_drop, proj_drop=proj_drop, drop_path=0.0)
    cfg["criteria"] = [dict(type="MSELoss", loss_weight=1.0, ignore_index=-1, batch_sample_point=-1),
                       dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1),
                       dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)]
    model = build_model(cfg)
    model.load_state_dict(fill_state_dict(model.state_dict(), seed=int(fx["sd_seed"])))
    return model.cuda().train()


def _step(model, inp, draws):
    model.zero_grad(set_to_none=True)
    loss = model(inp, draws=dict(draws))["loss"]
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def test_the_model_honours_attn_drop_and_proj_drop(ops, monkeypatch):
    """The mini model of train_step_mini.npz with attn_drop = proj_drop = 0.2, drop_path = 0, recorded noise and order draws.
    Fails without the feature: the two rates were accepted and ignored, so every seed gave the same loss."""
    import warnings
    import cdsegnet_amd.train_graph as TG
    from tests.helpers import load_fixture
    fx = load_fixture("train_step_mini.npz")
    inp = {k: torch.as_tensor(fx[k]).cuda() for k in ("coord", "grid_coord", "feat", "offset", "segment")}
    draws = dict(ts=fx["ts"], noise=fx["noise"], perms=[list(p) for p in fx["perms"]])
    model, plain = _drop_model(fx, 0.2, 0.2), _drop_model(fx, 0.0, 0.0)
    # eval mode: the loss of the rate-0 model, bit for bit (before any training forward moves the BatchNorm statistics)
    model.eval(), plain.eval()
    with torch.no_grad():
        le, lp0 = model(inp, draws=dict(draws))["loss"], plain(inp, draws=dict(draws))["loss"]
    assert GB.same_bits(le.reshape(1), lp0.reshape(1)) and model._train_graph.dropout_sites == []
    model.train(), plain.train()
    model.train_deterministic = True  # (fixed-order reductions: the gradients of equal steps are equal bit for bit)
    torch.manual_seed(101)
    la, ga = _step(model, inp, draws)
    sites_a = list(model._train_graph.dropout_sites)
    assert len(sites_a) == 4 * sum(type(m).__name__ in ("Block", "CrossBlock") for m in model.modules())
    torch.manual_seed(202)
    lb, _ = _step(model, inp, draws)
    torch.manual_seed(101)
    lc, gc = _step(model, inp, draws)
    lplain, _ = _step(plain, inp, draws)
    report("mini model, attn_drop = proj_drop = 0.2", loss_seed_101=float(la), loss_seed_202=float(lb), loss_rate_0=float(lplain))
    assert bool(torch.isfinite(la)) and bool(torch.isfinite(lb))
    assert float(la) != float(lb) and float(la) != float(lplain), "the rates do nothing"
    assert model._train_graph.dropout_sites == sites_a
    assert GB.same_bits(la.reshape(1), lc.reshape(1)) and set(ga) == set(gc)
    assert all(GB.same_bits(ga[k], gc[k]) for k in ga), [k for k in ga if not GB.same_bits(ga[k], gc[k])][:5]
    # train_block = "native": Blocks with a rate run as their autograd chain, with one warning
    model.train_deterministic = None
    pin = dict(draws, dropout=(101, 0))
    l0, g0 = _step(model, inp, pin)
    model.train_block = "native"
    monkeypatch.setattr(TG, "_warned_native_dropout", False)
    with pytest.warns(UserWarning, match="autograd chain") as rec:
        l1, g1 = _step(model, inp, pin)
    assert sum("autograd chain" in str(w.message) for w in rec) == 1
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _step(model, inp, pin)
    # (the metric and bound of tests/test_gpu_train_block.py's native-vs-autograd step)
    top = max(float(g.abs().max()) for g in g0.values())
    per = {k: float((g0[k] - g1[k]).abs().max()) / (float(g0[k].abs().max()) + 1e-3 * top) for k in g0}
    worst = max(per, key=per.get)
    report("mini model with dropout: native vs autograd", loss_autograd=float(l0), loss_native=float(l1), worst_rel_diff=per[worst])
    assert set(g0) == set(g1) and per[worst] < 1e-3 and abs(float(l0) - float(l1)) <= 1e-3 * abs(float(l0))


@LPS
def test_the_new_kernels_record_their_routes(ops, lp):
    """The launch record names the dropout kernels (appended to the catalogue as it was then: earlier ids keep their meaning),
    and a rate whose threshold is 256 records the existing forward kernel and the plain backward pair."""
    rng = np.random.default_rng(4)
    launch, (q, k, v, do) = _case([130, 64], 2, 0, False, LP(), rng, 1.0)
    names = O.route_catalog()
    new = ["attn_drop_f32_kernel", "attn_drop16_kernel", "attn_bwd_q_mfma_kernel<DropP>", "attn_bwd_kv_mfma_kernel<DropP>",
           "attn_bwd16_q_kernel<DropP>", "attn_bwd16_kv_kernel<DropP>", "dropout_kernel"]
    at = names.index(new[0])  # (in one block behind the forward attention kernels; later work appended behind them)
    assert names[at:at + len(new)] == new and names[at - 1] == "attn_f32_kernel"
    with O.record_routes() as rr:
        _run(torch.float32, q, k, v, do, launch, 2, 0.5)
    assert rr.kernels() == [new[0], new[2], new[3]]
    with O.record_routes() as rr:
        _run(LP(), q, k, v, do, launch, 2, 0.5)
    assert rr.kernels() == [new[1], new[4], new[5]]
    with O.record_routes() as rr:
        O.dropout(dev(rng.standard_normal((5, 7)), torch.float32), 0.5, 1, 2)
        _run(torch.float32, q, k, v, do, launch, 2, 0.0)
    assert rr.kernels() == [new[6], "attn_f32_kernel", "attn_bwd_q_mfma_kernel<>", "attn_bwd_kv_mfma_kernel<>"]
