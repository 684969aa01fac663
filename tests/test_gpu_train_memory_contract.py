"""GPU: guard bands and per-operand strides on the TRAINING path (tests/test_gpu_memory_contract.py holds the inference path).

The training kernels add onto gradients that lie next to each other in one slab: a store one row or one column off does not
crash, it adds a small number to a neighbour's gradient and the step still descends.  Every entry point below is called
  1. as its existing test calls it (contiguous, exact-size operands), checked against that test's fp64 reference under that
     test's own bound (helpers and bounds are imported, never restated);
  2. "strided": every output inside GB.banded (256 guard rows, 8 guard columns) or GB.banded_vector, every floating-point input
     inside GB.poisoned_input / GB.poisoned_vector (NaN guards), every index operand through GB.guard_index, every operand
     that has a row stride on a DIFFERENT one: bands intact, inputs unchanged as bits, every output finite, and the result
     BIT-equal to call 1 wherever the summation order is fixed or the sums are exact (the atomic weight gradients run on
     integer-valued operands, where fp32 sums are exact in any order);
  3. in the weakest layout the entry point's host checks admit (quoted in the docstrings), against the fp64 reference;
  4. once per documented precondition that the host code rejects, through the return code, with every output keeping its fill.

Entry points and legs.  All four: cdseg_layernorm_bwd, cdseg_layernorm_bwd_det, cdseg_linear_wgrad, cdseg_conv_wgrad,
cdseg_linear_wgrad16, cdseg_conv_wgrad16, cdseg_linear_wgrad_det, cdseg_conv_wgrad_det, cdseg_segment_sum,
cdseg_attention_bwd (non-dropout instantiations, fp32 and 16-bit), cdseg_bn_stats, cdseg_bn_finish, cdseg_bn_gelu_fwd,
cdseg_bn_gelu_bwd_sums, cdseg_bn_gelu_bwd_dx, cdseg_segment_max_arg, cdseg_segment_max_bwd.
cdseg_gelu_bwd has no row stride: its leg 2 is the guarded-vector call, its leg 3 the 4-byte aligned base it admits.
cdseg_conv_wgrad* take a contiguous dw (no lddw): dw sits between guard rows only.
The row kernels of csrc/trainblock.hip (cdseg_residual, _residual_rows, _gather_first, _run_sum, _scatter_first, _scale_cast,
_add_layernorm, _gelu_fwd, _gelu_bwd_cast) and the optimizer's flat tensors (cdseg_grad_norm, cdseg_adamw_step) have no row
stride and their host checks admit one alignment only (16 bytes; the optimizer: 4 bytes, which is its leg 3): legs 1, 2 and 4,
rows between guard rows (cols = 0) and vectors between guard elements.  cdseg_seg_loss_fwd / _bwd: all four.
The cdseg_tt_* entry points and cdseg_rand_int (csrc/traintime.hip) have no row stride and their host checks hold no pointer to
an alignment: leg 2 is every array between guard elements on a 16-byte aligned base, leg 3 the same on a base that is only
element-aligned (+4 bytes for fp32 / int32, +8 for fp64 / int64), leg 4 their NULL / range checks.
"""
import ctypes

import numpy as np
import pytest
import torch
import traintime_restatement as R

from cdsegnet_amd import _lib
from cdsegnet_amd import traintime as tt
from oracle import philox
from tests import guard_bands as GB
from tests import test_gpu_attention_bwd16 as A16
from tests import test_gpu_norm as NM
from tests import test_gpu_optim as OPT
from tests import test_gpu_seg_loss as SL
from tests import test_gpu_train_fp32 as T32
from tests import test_gpu_traintime as TT
from tests import test_gpu_train_block as TB
from tests.test_gpu_memory_contract import Mem, _lds
from tests.test_gpu_ops import LP, _library_variant, _physical, dev, ops, report  # noqa: F401  (fixtures)
from tests.test_gpu_wgrad16 import _eq, _exact, _ints, _kernel_map

pytestmark = pytest.mark.gpu

NAN = float("nan")
F32 = torch.float32
KINDS = pytest.mark.parametrize("lp", ["fp32", "bf16", "f16"])  # operand type; "f16" selects the IEEE-half build


def _t(lp):
    return F32 if lp == "fp32" else LP()


class TMem(Mem):
    """Mem with guarded 1-D vectors (gamma, db, statistics)."""

    def vout(self, n, *, fill, align=0, name="vec", dtype=F32, pre=None):
        inner, band = GB.banded_vector(n, dtype, fill=fill, align=align, name=name)
        self.bands.append(band)
        if pre is not None:
            inner.copy_(pre)
        return inner

    def rmw(self, pre, *, fill=-777.25, name="out", **kw):
        """An output that the kernel ADDS onto (or updates in place), starting as `pre`, between guards of a finite, non-zero
        fill: an add that lands on a guard changes its bits (NaN guards would swallow it: NaN + x is the same NaN)."""
        inner = self.out(tuple(pre.shape), pre.dtype, fill=fill, name=name, **kw)
        inner.copy_(pre)
        return inner

    def vin(self, t, *, align=0, name="vec"):
        inner, band = GB.poisoned_vector(t, align=align, name=name)
        self.bands.append(band)
        self.inputs.append((inner, t.clone(), name))
        return inner


def _err(rc):
    torch.cuda.synchronize()
    return _lib.ERRORS.get(rc, rc)


def _finite(*ts):
    return all(bool(torch.isfinite(t.float()).all()) for t in ts if t is not None)


def _exact_scratch(ops, monkeypatch):
    """ops._scratch served by exact-size guarded views (the per-call workspaces of the deterministic forms and of
    attention_bwd are asked for there)."""
    ws = GB.ExactWorkspaces()
    monkeypatch.setattr(ops, "_scratch", ws)
    return ws


# ====================================================================================================== LayerNorm backward
LN_SHAPES = [(1, 16, False), (65, 48, False), (257, 512, False), (65, 640, False), (1, 16, True), (65, 48, True), (257, 512, True)]


def _ln_call(ops, x, gamma, dy, layout, det, acc, pre, want_g=True, want_b=True):
    """One layernorm_bwd.  layout None: the existing test's call; "strided": x / dy / dx on strides of their own between
    guards; "weak": odd strides c + 1 / c + 3 / c + 1 on bases at +4 bytes, gamma / dgamma / dbeta at +4 / +8 / +12 bytes.
    -> (dx, dgamma, dbeta) clones."""
    M, C = x.shape
    mem = TMem()
    z = torch.zeros(C, device="cuda")
    pg, pb = (pre["dg"], pre["db"]) if acc else (z, z)
    if layout is None:
        xk, dyk, gk = x, dy, gamma
        dx = pre["dx"].clone() if acc else torch.full((M, C), NAN, device="cuda")
        dg, db = pg.clone(), pb.clone()
    else:
        if layout == "strided":
            kw = [dict(ld=_lds(C, F32, "strided", s)) for s in range(3)]
            al = (0, 0, 0)
        else:
            kw = [dict(ld=C + 1, align=4, cols=0), dict(ld=C + 3, align=4, cols=0), dict(ld=C + 1, align=4, cols=0)]
            al = (4, 8, 12)
        xk, dyk = mem.inp(x, name="x", **kw[0]), mem.inp(dy, name="dy", **kw[1])
        gk = mem.vin(gamma, align=al[0], name="gamma")
        dx = mem.rmw(pre["dx"], name="dx", **kw[2]) if acc else mem.out((M, C), F32, name="dx", **kw[2])
        dg, db = mem.vout(C, fill=-5.0, align=al[1], name="dgamma", pre=pg), mem.vout(C, fill=-5.0, align=al[2], name="dbeta", pre=pb)
    # a pointer that is not passed: the vector stays where it would have been and must keep its fill
    ops.layernorm_bwd(xk, gk, dyk, dx, accumulate=acc, eps=T32.EPS, dgamma=dg if want_g else None, dbeta=db if want_b else None,
                      **ops.det_kw(det))
    mem.check()
    if not want_g:
        assert GB.same_bits(dg, pg), "dgamma = NULL, and the vector in its place was written"
    if not want_b:
        assert GB.same_bits(db, pb), "dbeta = NULL, and the vector in its place was written"
    assert _finite(dx, dg, db), "a guard element reached a result, or an element was never written"
    return dx.clone(), dg.clone(), db.clone()


@pytest.mark.parametrize("M,C,det", LN_SHAPES, ids=[f"{m}x{c}-{'det' if d else 'default'}" for m, c, d in LN_SHAPES])
def test_layernorm_bwd_guard_bands_strides_and_odd_rows(ops, monkeypatch, M, C, det):
    """cdseg_layernorm_bwd / cdseg_layernorm_bwd_det.  A wave per row, 16 rows per wave, 64 per block: one row, one block plus
    a row, four blocks plus a row; (65, 640) is the wide branch above LNB_MAXC = 512 (default form only).  Host checks:
    `!f32_aligned(x, gamma, dy, dx, dgamma, dbeta)` (4 bytes) and `ldx < c || lddy < c || lddx < c` - the accesses are
    scalar, so the weakest layout is an odd stride on a base at +4 bytes.  dx depends on its own row alone: bit-equal in
    every layout; dgamma / dbeta are bit-equal in the deterministic form (block partials added by ascending index) and
    where one block holds all rows.  Bound: test_layernorm_bwd_vs_fp64_within_three_times_torch's (3 E_torch + 2^-24)."""
    ws = _exact_scratch(ops, monkeypatch)
    x, gamma, dy, pre = T32._ln_inputs(M, C, [], 1000 * M + C)
    _, dx64, dg64, db64 = T32._ln_autograd(x, gamma, dy, torch.float64)
    _, dxt, dgt, dbt = T32._ln_autograd(x, gamma, dy, F32)

    def versus_fp64(what, got, acc, want_g=True, want_b=True):
        a = 1.0 if acc else 0.0
        pairs = [("dx", got[0], a * pre["dx"] + dxt, a * pre["dx"].double() + dx64, None)]
        if want_g:
            pairs.append(("dgamma", got[1], a * pre["dg"] + dgt, a * pre["dg"].double() + dg64, None))
        if want_b:
            pairs.append(("dbeta", got[2], a * pre["db"] + dbt, a * pre["db"].double() + db64, None))
        T32._assert_vs_torch(f"layernorm_bwd ({M}, {C}) {'det ' if det else ''}{what}", pairs)

    fixed = det or M <= 64
    for acc in (False, True):
        base = _ln_call(ops, x, gamma, dy, None, det, acc, pre)
        versus_fp64(f"contiguous acc={acc}", base, acc)
        for layout in ("strided", "weak"):
            got = _ln_call(ops, x, gamma, dy, layout, det, acc, pre)
            assert GB.same_bits(got[0], base[0]), f"{layout}: dx differs from the contiguous call"
            if fixed:
                assert GB.same_bits(got[1], base[1]) and GB.same_bits(got[2], base[2]), f"{layout}: dgamma / dbeta differ"
            versus_fp64(f"{layout} acc={acc}", got, acc)
    for want_g, want_b in ((True, False), (False, True), (False, False)):
        got = _ln_call(ops, x, gamma, dy, "strided", det, True, pre, want_g, want_b)
        versus_fp64(f"strided dgamma={want_g} dbeta={want_b}", got, True, want_g, want_b)
    if det:
        ws.check(at_least=9)


def _p(t):
    """A tensor, an address or None -> what a c_void_p parameter takes."""
    return None if t is None else (t if isinstance(t, int) else t.data_ptr())


def _ln_raw(ops, det, x, gamma, dy, dx, dg, db, m, c, ld, ws=None, ws_bytes=0):
    lib = _lib.load()
    ldx, lddy, lddx = ld
    P = _p
    if det:
        return _err(lib.cdseg_layernorm_bwd_det(P(x), ldx, P(gamma), 1e-5, P(dy), lddy, P(dx), lddx, 0, P(dg), P(db), m, c, P(ws),
                                                ws_bytes, ops._stream()))
    return _err(lib.cdseg_layernorm_bwd(P(x), ldx, P(gamma), 1e-5, P(dy), lddy, P(dx), lddx, 0, P(dg), P(db), m, c, ops._stream()))


@pytest.mark.parametrize("det", [False, True], ids=["default", "det"])
def test_layernorm_bwd_refuses_what_its_kernel_cannot_take(ops, det):
    """include/cdseg.h: CDSEG_ERR_ARG for a NULL operand, a pointer that is not 4-byte aligned and a stride shorter than the
    row (rows would overlap: dx of row r + 1 lands on the tail of row r); the deterministic form also CDSEG_ERR_UNSUPPORTED
    above 512 columns, CDSEG_ERR_WORKSPACE for a short or NULL workspace and CDSEG_ERR_ARG for one that is not 4-byte aligned.
    Every output keeps its fill."""
    M, C = 70, 48
    g = torch.Generator().manual_seed(3)
    x, dy, gamma = torch.randn(M, C, generator=g).cuda(), torch.randn(M, C, generator=g).cuda(), torch.randn(C, generator=g).cuda()
    mem = TMem()
    dx = mem.out((M, C), F32, fill=-5.0, name="dx")
    dg, db = mem.vout(C, fill=-5.0, name="dgamma"), mem.vout(C, fill=-5.0, name="dbeta")
    nbytes = _lib.load().cdseg_layernorm_bwd_det_ws_bytes(M, C)
    assert nbytes == 2 * 2 * C * 4  # two 64-row blocks x (dgamma, dbeta)
    wsv, wsb = GB.exact_workspace(nbytes)
    def run(**kw):
        o = dict(x=x, gamma=gamma, dy=dy, dx=dx, dg=dg, db=db, ld=(C, C, dx.stride(0)), ws=wsv, ws_bytes=nbytes)
        o.update(kw)
        return _ln_raw(ops, det, o["x"], o["gamma"], o["dy"], o["dx"], o["dg"], o["db"], M, C, o["ld"], o["ws"], o["ws_bytes"])

    cases = [("ldx < c", dict(ld=(C - 1, C, dx.stride(0)))), ("lddy < c", dict(ld=(C, C - 4, dx.stride(0)))),
             ("lddx < c", dict(ld=(C, C, C - 1))), ("lddx = 0", dict(ld=(C, C, 0))),
             ("x at +2 bytes", dict(x=x.data_ptr() + 2)), ("dx at +2 bytes", dict(dx=dx.data_ptr() + 2)),
             ("gamma at +1 byte", dict(gamma=gamma.data_ptr() + 1)), ("dbeta at +2 bytes", dict(db=db.data_ptr() + 2)),
             ("x NULL", dict(x=None)), ("gamma NULL", dict(gamma=None)), ("dy NULL", dict(dy=None)), ("dx NULL", dict(dx=None))]
    for what, kw in cases:
        assert run(**kw) == "CDSEG_ERR_ARG", what
    if det:
        assert run(ws=wsv.data_ptr() + 2) == "CDSEG_ERR_ARG", "ws at +2 bytes"
        assert run(ws_bytes=nbytes - 1) == "CDSEG_ERR_WORKSPACE" and run(ws=None) == "CDSEG_ERR_WORKSPACE"
        xw, dxw = torch.randn(2, 640, device="cuda"), mem.out((2, 640), F32, fill=-5.0, name="dx640")
        nb640 = _lib.load().cdseg_layernorm_bwd_det_ws_bytes(2, 640)
        wide, _ = GB.exact_workspace(nb640)
        assert _ln_raw(ops, True, xw, torch.ones(640, device="cuda"), xw, dxw, None, None, 2, 640, (640, 640, dxw.stride(0)), wide,
                       nb640) == "CDSEG_ERR_UNSUPPORTED"
        assert bool((dxw == -5.0).all())
    mem.check()
    wsb.check()
    assert bool((dx == -5.0).all()) and bool((dg == -5.0).all()) and bool((db == -5.0).all()) and bool((wsv == GB.WorkspaceBand.FILL).all())
    assert run() == 0  # the same operands with nothing wrong run
    mem.check()
    assert _finite(dx) and not bool((dg == -5.0).any())


# ====================================================================================================== GELU backward
@pytest.mark.parametrize("n", [1, 255, 257])
def test_gelu_bwd_between_guard_elements(ops, n):
    """cdseg_gelu_bwd (one thread per element, 256-thread blocks: one element, a block less one, a block plus one; no row
    stride).  Host check: `!u || !dy || !dx || !f32_aligned(u, dy, dx)` - bases at +4 / +8 / +12 bytes are admitted.
    Bound: test_gelu_bwd_vs_closed_form_within_three_times_torch's."""
    g = torch.Generator().manual_seed(n)
    u, dy = (2 * torch.randn(n, generator=g)).cuda(), torch.randn(n, generator=g).cuda()
    base = ops.gelu_bwd(u, dy)
    ur = u.clone().requires_grad_(True)
    torch.nn.functional.gelu(ur).backward(dy)
    want = T32._gelu_grad64(u, dy)
    T32._assert_vs_torch(f"gelu_bwd n={n} contiguous", [("dx", base, ur.grad, want, None)])
    lib = _lib.load()
    for al in ((0, 0, 0), (4, 8, 12)):
        mem = TMem()
        uk, dyk = mem.vin(u, align=al[0], name="u"), mem.vin(dy, align=al[1], name="dy")
        dx = mem.vout(n, fill=-777.25, align=al[2], name="dx")
        assert lib.cdseg_gelu_bwd(uk.data_ptr(), dyk.data_ptr(), dx.data_ptr(), n, ops._stream()) == 0
        mem.check()
        assert GB.same_bits(dx, base), al
    mem = TMem()
    dx = mem.vout(n, fill=-5.0, name="dx")
    for what, a in (("u at +2 bytes", (u.data_ptr() + 2, dy.data_ptr(), dx.data_ptr())),
                    ("dx at +1 byte", (u.data_ptr(), dy.data_ptr(), dx.data_ptr() + 1)), ("dy NULL", (u.data_ptr(), None, dx.data_ptr()))):
        assert _err(lib.cdseg_gelu_bwd(*a, n, ops._stream())) == "CDSEG_ERR_ARG", what
    mem.check()
    assert bool((dx == -5.0).all())


# ====================================================================================================== weight gradients
def _wgrad_call(ops, lp, det, x, dy, idx, layout, pre_w, pre_b, conv=False):
    """One linear_wgrad / conv_wgrad on integer-valued operands (exact in any summation order).  x (R, K), dy (M, N) CPU
    floats; idx: None, xidx (M) or the (kvol, M) kernel map (device int32).  dw / db start as pre_w / pre_b between guards that
    hold -0.0: the kernels ADD onto dw and db, a NaN guard would swallow an add, and a tile column past K carries an exact
    +0.0 (it is staged as zeros) - of all fills only -0.0 changes its bits under `+ 0.0` as under any other add or store.  layouts:
      None     the existing tests' call: contiguous operands.
      strided  x, dy, dw on strides of their own (multiples of 8) between guard rows and columns, db between guard elements.
      weak     fp32: odd strides k + 1 / n + 3 / k + 1 on bases at +4 bytes, db at +12 bytes; 16-bit: x and dy at the minimum
               stride (k, n: multiples of 16) and an odd lddw = k + 1 (only ldx / lddy are held to multiples of 8).
    -> (dw, db) clones."""
    t = _t(lp)
    N, K = dy.shape[1], x.shape[1]
    mem = TMem()
    wshape = tuple(pre_w.shape)
    w2 = (N, pre_w.numel() // N)  # conv: (cout, kvol * cin), contiguous (the entry point has no lddw)
    if layout is None:
        xk, dyk, ik = dev(x, t), dev(dy, t), idx
        dw, db = pre_w.cuda().clone(), pre_b.cuda().clone()
    else:
        if layout == "strided":
            kx, ky, kwd, ab = dict(ld=_lds(K, t, "strided", 0)), dict(ld=_lds(N, t, "strided", 1)), dict(ld=_lds(K, F32, "strided", 2)), 0
        elif t == F32:
            kx, ky, kwd, ab = dict(ld=K + 1, align=4, cols=0), dict(ld=N + 3, align=4, cols=0), dict(ld=K + 1, align=4, cols=0), 12
        else:
            kx, ky, kwd, ab = dict(cols=0), dict(cols=0), dict(ld=K + 1, cols=0), 0
        if conv:
            kwd = dict(cols=0)
        xk, dyk = mem.inp(dev(x, t), name="x", **kx), mem.inp(dev(dy, t), name="dy", **ky)
        ik = None if idx is None else mem.index(idx, none=-1)
        dw = mem.rmw(pre_w.cuda().view(w2), fill=-0.0, name="dw", **kwd).view(wshape)
        db = mem.vout(N, fill=-0.0, align=ab, name="db", pre=pre_b.cuda())
    kw = ops.det_kw(det)
    if conv:
        ops.conv_wgrad(xk, ik, dyk, dw, db, **kw)
    else:
        ops.linear_wgrad(xk, dyk, dw, db, xidx=ik, **kw)
    mem.check()
    return dw.clone(), db.clone()


def _wgrad_legs(ops, lp, det, x, dy, idx, what, conv=False):
    """Legs 1 - 3 of one weight-gradient shape -> None.  `idx` as in _wgrad_call."""
    rng = np.random.default_rng(x.shape[0] + dy.shape[1])
    M, N, K = dy.shape[0], dy.shape[1], x.shape[1]
    T32._premise(M, x, dy)
    xd, dyd = x.cuda(), dy.cuda()
    if conv:
        kvol = idx.shape[0]
        want_w = torch.stack([_exact(dyd, xd, idx[o])[0] for o in range(kvol)], 1).cpu()  # (cout, kvol, cin)
        want_b = dy.double().sum(0).long()
        pre_w = _ints(rng, N, kvol, K) * 5
    else:
        want_w, want_b = (a.cpu() for a in _exact(dyd, xd, idx))
        pre_w = _ints(rng, N, K) * 5
    pre_b = _ints(rng, N) * 7
    zero_w, zero_b = torch.zeros_like(pre_w), torch.zeros_like(pre_b)
    base_w, base_b = _wgrad_call(ops, lp, det, x, dy, idx, None, zero_w, zero_b, conv)
    assert _eq(base_w, want_w) and _eq(base_b, want_b), f"{what}: contiguous"
    for layout in ("strided", "weak"):
        dw, db = _wgrad_call(ops, lp, det, x, dy, idx, layout, pre_w, pre_b, conv)
        assert _eq(dw, pre_w.long() + want_w) and _eq(db, pre_b.long() + want_b), f"{what}: {layout}, pre-filled dw / db"
        assert GB.same_bits(dw - pre_w.cuda(), base_w) and GB.same_bits(db - pre_b.cuda(), base_b), f"{what}: {layout} differs as bits"
    # db = NULL: a vector stands where db would have been and keeps its content
    mem = TMem()
    t = _t(lp)
    spare = mem.vout(N, fill=-7.0, name="db (not passed)")
    dw = mem.rmw(pre_w.cuda().view(N, -1), fill=-0.0, name="dw", cols=0 if conv else 8).view(pre_w.shape)
    ik = None if idx is None else mem.index(idx, none=-1)
    xk, dyk = mem.inp(dev(x, t), name="x", ld=_lds(K, t, "strided", 3)), mem.inp(dev(dy, t), name="dy", ld=_lds(N, t, "strided", 4))
    if conv:
        ops.conv_wgrad(xk, ik, dyk, dw, None, **ops.det_kw(det))
    else:
        ops.linear_wgrad(xk, dyk, dw, None, xidx=ik, **ops.det_kw(det))
    mem.check()
    assert _eq(dw, pre_w.long() + want_w) and bool((spare == -7.0).all()), f"{what}: db = NULL"


# (M, K, N): wgrad_kernel's 64 x 64 tiles in 16-column quarters (`kt_ok[t] = k0 + 16 * t < p.K`), one row, rows inside a
# 4-row MFMA step, one split less a row, two and three splits whose last one is short (partition_f32: M = 1025, 2051)
F32_DENSE = [(1, 16, 16), (5, 16, 80), (1023, 80, 16), (1025, 64, 64), (2051, 48, 96)]


def _gather_idx(rng, M, R, dead=None):
    idx = rng.integers(0, R, size=M)
    idx[rng.random(M) < 0.3] = -1
    if M >= 9:
        idx[5:9] = idx[4]
    for a, b in dead or ():
        idx[a:b] = -1
    return torch.as_tensor(idx, dtype=torch.int32).cuda()


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("M,K,N", F32_DENSE, ids=[f"{m}x{k}x{n}" for m, k, n in F32_DENSE])
def test_linear_wgrad_fp32_guard_bands_and_strides(ops, monkeypatch, M, K, N, det):
    """cdseg_linear_wgrad / cdseg_linear_wgrad_det (CDSEG_F32), dense and gathered (xidx with -1 and repeated rows, x with
    another row count).  Host checks: `wgrad_args_ok` (x, dy, dw there; every pointer 4-byte aligned), `wgrad_lds_ok`
    (ldx >= k, lddy >= n, lddw >= k), `(n & 15) || (k & 15)`; nothing holds a stride to a multiple: the weak layout is odd
    strides on bases at +4 bytes.  Exact on integers (test_default_wgrad_exact_on_integers), so the atomic form is compared
    as bits too."""
    ws = _exact_scratch(ops, monkeypatch)
    part = T32._partition(ops, M, N, K)
    assert part.splits == {1025: 2, 2051: 3}.get(M, 1) and part.rows_per_split % 4 == 0, tuple(part)
    rng = np.random.default_rng(M + 7 * K + 13 * N)
    x, dy = _ints(rng, M, K), _ints(rng, M, N)
    _wgrad_legs(ops, "fp32", det, x, dy, None, f"dense {M}x{K}x{N}")
    R = max(1, M // 2) + 3
    _wgrad_legs(ops, "fp32", det, _ints(rng, R, K), dy, _gather_idx(rng, M, R), f"gathered {M}x{K}x{N}")
    if det:
        ws.check(at_least=8)


CONV = [(16, 32, 3), (32, 16, 3), (16, 32, 5)]


@KINDS
@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("cin,cout,ksize", CONV, ids=[f"{a}-{b}-k{k}" for a, b, k in CONV])
def test_conv_wgrad_guard_bands_and_strides(ops, monkeypatch, lp, cin, cout, ksize, det):
    """cdseg_conv_wgrad / cdseg_conv_wgrad16 / cdseg_conv_wgrad_det on the `batch2` kernel map, kvol = 27 and 125 (the stem):
    `dw_off_stride = cin`, `idx_stride = m`, lddw = kvol * cin - offset o writes columns o * cin .. (o + 1) * cin - 1 of a
    dw row and no other (every offset is compared with its own gathered product).  nbr_kmajor sits between -1 rows."""
    ws = _exact_scratch(ops, monkeypatch)
    nbr = _kernel_map(ops, "batch2", ksize)
    M = nbr.shape[1]
    rng = np.random.default_rng(cin + cout + ksize)
    x, dy = _ints(rng, M, cin), _ints(rng, M, cout)
    _wgrad_legs(ops, lp, det, x, dy, nbr, f"conv {cin}-{cout}-k{ksize} {lp}", conv=True)
    if det:
        ws.check(at_least=4)


# (M, K, N): one per tile instantiation of launch_wgrad16's switch (tn, tk from partition_16: 32 / 64 / 128 columns, 128 x 128
# -> 128 x 64); every N and K leaves columns past the end of a tile ("staged as zeros and never stored"); M inside a 64-row
# chunk, across it, and two splits (513 rows: 320 + 193)
W16_DENSE = [(1, 16, 16, (1, 1)), (63, 48, 16, (1, 2)), (65, 96, 16, (1, 4)), (513, 16, 48, (2, 1)), (65, 48, 48, (2, 2)),
             (63, 512, 48, (2, 4)), (513, 16, 96, (4, 1)), (513, 96, 512, (4, 2))]


@pytest.mark.parametrize("lp", ["bf16", "f16"])
@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("M,K,N,tile", W16_DENSE, ids=[f"{m}x{k}x{n}-tile{a}x{b}" for m, k, n, (a, b) in W16_DENSE])
def test_linear_wgrad16_guard_bands_and_strides(ops, monkeypatch, lp, M, K, N, tile, det):
    """cdseg_linear_wgrad16 / cdseg_linear_wgrad_det (CDSEG_BF16).  Host checks: `wgrad16_args_ok` (`(ldx | lddy) & 7`, every
    pointer 16-byte aligned), `wgrad_lds_ok`; lddw is held to nothing but lddw >= k.  The gathered form has whole 64-row
    chunks of -1 between live ones (the `__syncthreads_or` vote skips them; db still counts their rows).  Exact on integers
    (test_dense_exact_on_integers)."""
    ws = _exact_scratch(ops, monkeypatch)
    tn, tk = (4 if N > 64 else 2 if N > 32 else 1), (4 if K > 64 else 2 if K > 32 else 1)
    assert (tn, 2 if (tn, tk) == (4, 4) else tk) == tile
    assert ops.wgrad_partition(M, N, K, 1, LP()).splits == (2 if M == 513 else 1)
    rng = np.random.default_rng(M + 7 * K + 13 * N)
    x, dy = _ints(rng, M, K), _ints(rng, M, N)
    _wgrad_legs(ops, lp, det, x, dy, None, f"dense16 {M}x{K}x{N}")
    Mg = 513
    R = 100
    idx = _gather_idx(rng, Mg, R, dead=[(64, 192), (256, 320), (448, 513)])
    _wgrad_legs(ops, lp, det, _ints(rng, R, K), _ints(rng, Mg, N), idx, f"gathered16 {Mg}x{K}x{N}")
    if det:
        ws.check(at_least=8)


def _wgrad_raw(ops, fn, lp16, x, dy, dw, db, *, xidx, ld, m, k, n, kvol, det=None):
    """The C ABI of the six weight-gradient entry points: fn in linear / conv, det None or (dtype code, ws, ws_bytes)."""
    lib = _lib.load()
    P = _p
    ldx, lddy, lddw = ld
    tail = () if det is None else (det[0], P(det[1]), det[2])
    if fn == "linear":
        f = lib.cdseg_linear_wgrad_det if det else lib.cdseg_linear_wgrad16 if lp16 else lib.cdseg_linear_wgrad
        return _err(f(P(x), ldx, P(xidx), P(dy), lddy, m, k, n, P(dw), lddw, P(db), *tail, ops._stream()))
    f = lib.cdseg_conv_wgrad_det if det else lib.cdseg_conv_wgrad16 if lp16 else lib.cdseg_conv_wgrad
    return _err(f(P(x), ldx, P(xidx), kvol, P(dy), lddy, m, k, n, P(dw), P(db), *tail, ops._stream()))


@KINDS
@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
def test_weight_gradients_refuse_what_their_kernels_cannot_take(ops, lp, det):
    """include/cdseg.h, all six entry points: a stride shorter than its row (ldx < k, lddy < n, lddw < k: dw rows would overlap
    and every tile add onto its neighbour's), misaligned pointers (4 bytes for fp32, 16 for the 16-bit forms), ldx / lddy that
    are no multiples of 8 (16-bit), n or k that are no multiples of 16 (CDSEG_ERR_UNSUPPORTED), NULL operands, and for the
    deterministic forms a workspace that is short, NULL or not 16-byte aligned.  dw, db and the workspace keep their fill."""
    t = _t(lp)
    M, K, N, kvol = 70, 32, 48, 27
    rng = np.random.default_rng(1)
    x, dy = dev(_ints(rng, M, K + 16), t)[:, :K], dev(_ints(rng, M, N + 16), t)[:, :N]
    nbr = torch.full((kvol, M), -1, dtype=torch.int32, device="cuda")
    mem = TMem()
    dw = mem.out((N, K), F32, fill=-5.0, name="dw")
    dw3 = mem.out((N, kvol * K), F32, fill=-5.0, cols=0, name="dw3")
    db = mem.vout(N, fill=-5.0, name="db")
    code = ops.F32 if t == F32 else ops.BF16
    lib = _lib.load()
    need = {f: lib.cdseg_wgrad_det_ws_bytes(M, N, K, kv, code) for f, kv in (("linear", 1), ("conv", kvol))}
    wsv, wsb = GB.exact_workspace(max(need.values()))
    mis = 2 if t == F32 else 8  # bytes: not 4-byte / not 16-byte aligned

    def run(fn, **kw):
        d = None
        if det:
            d = (kw.pop("code", code), kw.pop("ws", wsv), kw.pop("ws_bytes", need[fn]))
        out = dw if fn == "linear" else dw3
        o = dict(x=x, dy=dy, dw=out, db=db, xidx=nbr if fn == "conv" else None, ld=(sx, sy, sw), k=K, n=N)
        o.update(kw)
        return _wgrad_raw(ops, fn, t != F32, o["x"], o["dy"], o["dw"], o["db"], xidx=o["xidx"], ld=o["ld"], m=M, k=o["k"], n=o["n"],
                          kvol=kvol, det=d)

    sx, sy, sw = x.stride(0), dy.stride(0), dw.stride(0)
    short = 8 if t != F32 else 1  # (16-bit: the stride stays a multiple of 8, so that the new check is what refuses it)
    for fn in ("linear", "conv"):
        bad = [("ldx < k", dict(ld=(K - short, sy, sw))), ("lddy < n", dict(ld=(sx, N - short, sw))), ("ldx = 0", dict(ld=(0, sy, sw))),
               ("x misaligned", dict(x=x.data_ptr() + mis)), ("dy misaligned", dict(dy=dy.data_ptr() + mis)),
               ("dw misaligned", dict(dw=(dw if fn == "linear" else dw3).data_ptr() + mis)), ("db misaligned", dict(db=db.data_ptr() + mis)),
               ("x NULL", dict(x=None)), ("dy NULL", dict(dy=None)), ("dw NULL", dict(dw=None))]
        if fn == "linear":
            bad += [("lddw < k", dict(ld=(sx, sy, K - 1))), ("lddw = 0", dict(ld=(sx, sy, 0)))]
        else:
            bad += [("nbr NULL", dict(xidx=0)), ("nbr misaligned", dict(xidx=nbr.data_ptr() + mis))]
        if t != F32:
            bad += [("ldx % 8", dict(ld=(sx + 4, sy, sw))), ("lddy % 8", dict(ld=(sx, sy + 4, sw)))]
        if det:
            bad += [("ws misaligned", dict(ws=wsv.data_ptr() + 8))]
        for what, kw in bad:
            assert run(fn, **kw) == "CDSEG_ERR_ARG", (fn, what)
        assert run(fn, k=K - 8) == "CDSEG_ERR_UNSUPPORTED" and run(fn, n=N - 8) == "CDSEG_ERR_UNSUPPORTED", fn
        if det:
            assert run(fn, ws_bytes=need[fn] - 1) == "CDSEG_ERR_WORKSPACE" and run(fn, ws=None) == "CDSEG_ERR_WORKSPACE", fn
            assert run(fn, code=7) == "CDSEG_ERR_UNSUPPORTED", fn
    mem.check()
    wsb.check()
    assert all(bool((o == -5.0).all()) for o in (dw, dw3, db)) and bool((wsv == GB.WorkspaceBand.FILL).all())
    for o in (dw, dw3, db):
        o.zero_()
    assert run("linear") == 0 and run("conv") == 0  # the same operands with nothing wrong run
    mem.check()
    wsb.check()
    want_w, want_b = _exact(dy.float(), x.float())
    assert _eq(dw, want_w) and _eq(db, 2 * want_b) and bool((dw3 == 0).all())  # (a map of -1: no neighbour anywhere)


# ====================================================================================================== segment sum
def _segsum_raw(ops, src, seg, m, c, out, ld=None):
    ls, lo = ld or (src.stride(0), out.stride(0))
    return _err(_lib.load().cdseg_segment_sum(_p(src), ls, _p(seg), m, c, _p(out), lo, ops._stream()))


@pytest.mark.parametrize("m", [1, 37])
@pytest.mark.parametrize("c", [16, 32, 48, 512])
def test_segment_sum_guard_bands_strides_and_refusals(ops, m, c):
    """cdseg_segment_sum: cw = 16 / 32 / 64 lanes per pooled row (c = 16, 32, 48 and 512: a lane walks 8 columns), 4 * 64 / cw
    rows per block; runs of 1 to 8 rows, one of 70 and an empty one.  Host check: `!f32_aligned(src, out) ||
    ((uintptr_t)seg_start & 3) || ld < c || ldo < c` - scalar accesses, so the weak layout is odd strides on bases at +4
    bytes.  Ascending row order: bit-equal in every layout; exact on integers against index_add
    (test_segment_sum_on_the_pooling_link)."""
    rng = np.random.default_rng(m + c)
    counts = rng.integers(1, 9, size=m)
    counts[m // 2] = 70
    if m > 2:
        counts[1] = 0
    seg = torch.as_tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32)
    n = int(seg[-1])
    src = _ints(rng, n, c)
    want = torch.zeros(m, c).index_add_(0, torch.repeat_interleave(torch.arange(m), torch.as_tensor(counts)), src)
    base = ops.segment_sum(src.cuda(), seg.cuda(), m)
    torch.cuda.synchronize()
    assert torch.equal(base.cpu(), want)
    for layout in ("strided", "weak"):
        mem = TMem()
        if layout == "strided":
            s, out = mem.inp(src.cuda(), ld=_lds(c, F32, "strided", 0), name="src"), mem.out((m, c), F32, ld=_lds(c, F32, "strided", 1))
        else:
            s, out = mem.inp(src.cuda(), ld=c + 1, align=4, cols=0, name="src"), mem.out((m, c), F32, ld=c + 3, align=4, cols=0)
        assert _segsum_raw(ops, s, mem.index(seg.cuda()), m, c, out) == 0
        mem.check()
        assert GB.same_bits(out, base), layout
    mem = TMem()
    out, s, sg = mem.out((m, c), F32, fill=-5.0), src.cuda(), seg.cuda()
    for what, kw in (("ld < c", dict(ld=(c - 1, out.stride(0)))), ("ldo < c", dict(ld=(c, c - 1))), ("ldo = 0", dict(ld=(c, 0)))):
        assert _segsum_raw(ops, s, sg, m, c, out, **kw) == "CDSEG_ERR_ARG", what
    for what, a in (("src at +2 bytes", (s.data_ptr() + 2, sg, out)), ("out at +2 bytes", (s, sg, out.data_ptr() + 2)),
                    ("seg_start at +2 bytes", (s, sg.data_ptr() + 2, out)), ("src NULL", (None, sg, out)), ("seg_start NULL", (s, None, out)),
                    ("out NULL", (s, sg, None))):
        assert _segsum_raw(ops, a[0], a[1], m, c, a[2], ld=(c, out.stride(0))) == "CDSEG_ERR_ARG", what
    mem.check()
    assert bool((out == -5.0).all())


# ====================================================================================================== attention backward
# (name, patch lengths, heads, padding duplicates of the last patch, cross attention): the 16-bit launch cuts a patch-head into
# `split` slices by `while (split < 4 && num_patches * H * split * 2 <= 512) split *= 2`: 3 patches x 2 heads -> 4, 40 x 2 -> 4 as
# well (320 <= 512 doubles once more), 70 x 2 -> 2 (560 > 512), 9 x 32 -> 1
_RAGGED40, _RAGGED70 = [3 + (7 * i) % 15 for i in range(40)], [3 + (7 * i) % 15 for i in range(70)]
ATTN = [("split4-1024-1-33", [1024, 1, 33], 2, 0, False, 4), ("split4-40-patches-dups", _RAGGED40, 2, 3, False, 4),
        ("split2-70-patches-dups", _RAGGED70, 2, 3, False, 2),
        ("split1-9-patches-H32-cross", [20, 33, 17, 40, 16, 31, 32, 1, 25], 32, 0, True, 1)]


def _attn_call(ops, t, q, k, v, do, launch, H, layout, packed):
    """ops.attention_bwd.  layout None: test_gpu_attention_bwd16's _kernel call.  strided: seven strides of their own;
    weak: ldq / ldk / ldv / lddo at the minimum (the row, H * 16) and lddq / lddk / lddv multiples of 4 but not of 8.
    packed: q, k, v are views of one poisoned (n, 3C) buffer, dq, dk, dv views of one banded (n, 3C) buffer."""
    C = 16 * H
    gq, gkv, widx, ps = launch.device()
    mem = TMem()
    qd, kd, vd, dod = (dev(a, t) for a in (q, k, v, do))
    if layout is None:
        dq, dk, dv = (torch.zeros(a.shape, device="cuda") for a in (q, k, v))
    elif packed:
        qkv = mem.inp(torch.cat([qd, kd, vd], 1), ld=_lds(3 * C, t, "strided", 0), name="qkv")
        qd, kd, vd = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
        dod = mem.inp(dod, ld=_lds(C, t, "strided", 1), name="dout")
        g = mem.out((q.shape[0], 3 * C), F32, fill=-5.0, ld=_lds(3 * C, F32, "ld4", 2), name="dqkv")
        g.zero_()
        dq, dk, dv = g[:, :C], g[:, C:2 * C], g[:, 2 * C:]
    else:
        lay = (lambda s: dict(ld=_lds(C, t, "strided", s))) if layout == "strided" else (lambda s: dict(cols=0))
        qd, kd, vd, dod = (mem.inp(a, name=nm, **lay(s)) for s, (a, nm) in enumerate(((qd, "q"), (kd, "k"), (vd, "v"), (dod, "dout"))))
        glay = (lambda s: dict(ld=_lds(C, F32, "strided", s))) if layout == "strided" else (lambda s: dict(ld=_lds(C, F32, "ld4", s)))
        dq, dk, dv = (mem.out(a.shape, F32, fill=-5.0, name=nm, **glay(4 + s)) for s, (a, nm) in enumerate(((q, "dq"), (k, "dk"), (v, "dv"))))
        for o in (dq, dk, dv):
            o.zero_()
    if layout is not None:
        gq, gkv, widx, ps = mem.index(gq), mem.index(gkv), mem.index(widx, none=-1), mem.index(ps)
    ops.attention_bwd(qd, kd, vd, gq, gkv, widx, ps, launch.ps.tolist(), H, A16.SCALE, dod, dq, dk, dv)
    mem.check()
    assert _finite(dq, dk, dv), "a guard row of q / k / v / dout reached a gradient"
    return dq.clone(), dk.clone(), dv.clone()


@KINDS
@pytest.mark.parametrize("name,lens,H,dup,cross,split", ATTN, ids=[c[0] for c in ATTN])
def test_attention_bwd_guard_bands_seven_strides_and_exact_workspace(ops, monkeypatch, lp, name, lens, H, dup, cross, split):
    """cdseg_attention_bwd, fp32 (attn_bwd_*_mfma_kernel<>) and 16-bit (attn_bwd16_*_kernel<>).  Host checks: `((ldq | ldk |
    ldv | lddo) & op_mask) || ((lddq | lddk | lddv) & 3)` with op_mask 3 (fp32) / 7 (16-bit), every pointer 16-byte aligned,
    every stride >= num_heads * 16, `ws_bytes < cdseg_attention_bwd_ws_bytes(num_slots, num_heads)`.  The workspace is served
    at exactly that size.  A row sits in at most two slots, so the atomic adds commute
    (test_attention_bwd_is_bit_repeatable_as_it_is): every layout is bit-equal to the contiguous call.  Bounds: 2 E_ref + L 2^-24
    of test_gpu_attention_bwd16 (16-bit) and of test_attention_bwd_fp32_at_deep_head_counts (fp32)."""
    ws = _exact_scratch(ops, monkeypatch)
    t = _t(lp)
    rng = np.random.default_rng(sum(lens) + 31 * H + dup)
    if t == F32:
        launch, (q, k, v, do) = T32._attn_case(lens, H, dup, cross, sum(lens) + 31 * H + dup)
    else:
        launch, (q, k, v, do) = A16._case(lens, H, dup, cross, t, rng, 1.0)
        if dup:  # (a row in at most two slots, as in the padding plan: test_attention_bwd_is_bit_repeatable_as_it_is)
            patches = list(launch.patches)
            gq, gkv, widx = (a.copy() for a in patches[-1])
            own = len(gq) - dup
            pick = rng.choice(own, dup, replace=False)
            gq[own:], gkv[own:] = gq[pick], gkv[pick]
            patches[-1] = (gq, gkv, widx)
            launch = A16.Launch(patches)
    assert (k.shape[0] == q.shape[0] + 50) == cross
    with ops.record_routes() as rr:
        base = _attn_call(ops, t, q, k, v, do, launch, H, None, False)
    assert rr.count == 2 and all(r.splits == (1 if t == F32 else split) for r in rr.routes), rr.routes
    if t == F32:
        exact = A16._grads(q, k, v, do, launch, H, F32, mode="noround")
        ref32 = T32._torch_f32_grads(q, k, v, do, launch, H)
    layouts = [("strided", False), ("weak", False)] + ([] if cross else [("packed", True)])
    for layout, packed in [(None, False)] + layouts:
        got = base if layout is None else _attn_call(ops, t, q, k, v, do, launch, H, layout, packed)
        for a, b, tn in zip(got, base, ("dq", "dk", "dv")):
            assert GB.same_bits(a, b), f"{layout}: {tn} differs from the contiguous call"
        host = tuple(g.cpu().double().numpy() for g in got)
        if t == F32:
            T32._attn_assert(f"{name} {layout}", host, ref32, exact, launch)
        else:
            A16._compare(f"{name} {layout}", host, launch, q, k, v, do, H, t)
    ws.check(at_least=1 + len(layouts))
    for b in ws.served:
        assert b.nbytes == max(1, _lib.load().cdseg_attention_bwd_ws_bytes(int(launch.ps[-1]), H))


@KINDS
def test_attention_bwd_refuses_strides_and_bases_it_cannot_take(ops, lp):
    """include/cdseg.h: CDSEG_ERR_ARG for an operand stride that is no multiple of 4 (fp32) / 8 (16-bit), a gradient stride
    that is no multiple of 4, any of the seven below the row (num_heads * 16), a pointer that is not 16-byte aligned or NULL;
    CDSEG_ERR_WORKSPACE for a short or NULL workspace; CDSEG_ERR_UNSUPPORTED for max_len > 1024 and another dtype."""
    t = _t(lp)
    H, L = 2, 20
    C = 16 * H
    g = torch.Generator().manual_seed(0)
    q, k, v, do = (dev(torch.randn(L, C + 16, generator=g), t)[:, :C] for _ in range(4))
    mem = TMem()
    dq, dk, dv = (mem.out((L, C), F32, fill=-5.0, name=nm) for nm in ("dq", "dk", "dv"))
    ar = torch.arange(L, dtype=torch.int32, device="cuda")
    ps = torch.tensor([0, L], dtype=torch.int32, device="cuda")
    lib = _lib.load()
    need = lib.cdseg_attention_bwd_ws_bytes(L, H)
    wsv, wsb = GB.exact_workspace(need)
    P = _p
    lds0 = dict(ldq=q.stride(0), ldk=k.stride(0), ldv=v.stride(0), lddo=do.stride(0), lddq=dq.stride(0), lddk=dk.stride(0), lddv=dv.stride(0))

    def run(**kw):
        o = dict(q=q, k=k, v=v, do=do, dq=dq, dk=dk, dv=dv, ws=wsv, ws_bytes=need, max_len=L, code=ops.dt(q), **lds0)
        o.update(kw)
        return _err(lib.cdseg_attention_bwd(P(o["q"]), P(o["k"]), P(o["v"]), o["ldq"], o["ldk"], o["ldv"], P(ar), P(ar), P(ar), P(ps), 1, H,
                                            L,
                                            o["max_len"], 0.25, P(o["do"]), o["lddo"], P(o["dq"]), P(o["dk"]), P(o["dv"]), o["lddq"],
                                            o["lddk"], o["lddv"], o["code"], P(o["ws"]), o["ws_bytes"], ops._stream()))

    per16 = 16 // q.element_size()
    for name, ld in lds0.items():
        assert run(**{name: C - per16}) == "CDSEG_ERR_ARG", f"{name} below the row"
        assert run(**{name: 0}) == "CDSEG_ERR_ARG", f"{name} = 0"
        assert run(**{name: ld + 2}) == "CDSEG_ERR_ARG", f"{name} % 4"
    if t != F32:
        for name in ("ldq", "ldk", "ldv", "lddo"):
            assert run(**{name: lds0[name] + 4}) == "CDSEG_ERR_ARG", f"{name} % 8 (16-bit operands)"
    for name, ten in dict(q=q, k=k, v=v, do=do, dq=dq, dk=dk, dv=dv).items():
        assert run(**{name: ten.data_ptr() + 8}) == "CDSEG_ERR_ARG", f"{name} at +8 bytes"
        assert run(**{name: None}) == "CDSEG_ERR_ARG", f"{name} NULL"
    assert run(ws_bytes=need - 1) == "CDSEG_ERR_WORKSPACE" and run(ws=None) == "CDSEG_ERR_WORKSPACE"
    assert run(max_len=1025) == "CDSEG_ERR_UNSUPPORTED" and run(code=7) == "CDSEG_ERR_UNSUPPORTED"
    mem.check()
    wsb.check()
    assert all(bool((o == -5.0).all()) for o in (dq, dk, dv)) and bool((wsv == GB.WorkspaceBand.FILL).all())
    for o in (dq, dk, dv):
        o.zero_()
    assert run() == 0
    mem.check()
    wsb.check()
    assert _finite(dq, dk, dv) and float(dv.abs().max()) > 0


# ====================================================================================================== BatchNorm + GELU
def _bn_raw(ops, x, dy, gamma, beta, rm, rv, layout):
    """The five BatchNorm entry points through the C ABI (the op layer allocates statistics, sums and workspaces itself).
    strided: x, dy, y, dx on strides of their own; weak: `ld_ok`'s minimum beyond the row, ld = c + 4, and the fp64 vectors
    (stats, gsums) 8- but not 16-byte aligned, the running buffers at +4 / +12 bytes.  -> dict as test_gpu_norm's _fused."""
    lib = _lib.load()
    m, c = x.shape
    mem = TMem()
    weak = layout == "weak"
    lay = (lambda s: dict(ld=c + 4, cols=0)) if weak else (lambda s: dict(ld=_lds(c, F32, "strided", s)))
    xk, dyk = mem.inp(x, name="x", **lay(0)), mem.inp(dy, name="dy", **lay(1))
    y, dx = mem.out((m, c), F32, name="y", **lay(2)), mem.out((m, c), F32, name="dx", **lay(3))
    gk, bk = mem.vin(gamma, name="gamma"), mem.vin(beta, name="beta")
    a8 = 8 if weak else 0
    stats = mem.vout(2 * c + 1, fill=NAN, align=a8, dtype=torch.float64, name="stats")
    gsums = mem.vout(2 * c, fill=NAN, align=a8, dtype=torch.float64, name="gsums")
    mean, invstd = mem.vout(c, fill=NAN, name="mean"), mem.vout(c, fill=NAN, name="invstd")
    rmk = mem.vout(c, fill=-5.0, align=4 if weak else 0, name="running_mean", pre=rm)  # (updated in place: finite guards)
    rvk = mem.vout(c, fill=-5.0, align=12 if weak else 0, name="running_var", pre=rv)
    need = lib.cdseg_bn_ws_bytes(m, c)
    assert need == ops.bn_partition(m, c).blocks * 2 * c * 8
    ws1, b1 = GB.exact_workspace(need)
    ws2, b2 = GB.exact_workspace(need)
    P, st = _p, ops._stream()
    assert lib.cdseg_bn_stats(P(xk), xk.stride(0), m, c, P(stats), P(ws1), need, st) == 0
    assert lib.cdseg_bn_finish(P(stats), c, NM.EPS, NM.MOM, P(mean), P(invstd), P(rmk), P(rvk), st) == 0
    assert lib.cdseg_bn_gelu_fwd(P(xk), xk.stride(0), m, c, P(mean), P(invstd), P(gk), P(bk), P(y), y.stride(0), st) == 0
    assert lib.cdseg_bn_gelu_bwd_sums(P(xk), xk.stride(0), P(dyk), dyk.stride(0), m, c, P(mean), P(invstd), P(gk), P(bk), P(gsums), P(ws2),
                                      need, st) == 0
    count = stats[2 * c:]
    assert lib.cdseg_bn_gelu_bwd_dx(P(xk), xk.stride(0), P(dyk), dyk.stride(0), m, c, P(mean), P(invstd), P(gk), P(bk), P(gsums), P(count),
                                    P(dx), dx.stride(0), st) == 0
    mem.check()
    b1.check()
    b2.check()
    out = dict(y=y, dx=dx, stats=stats, gsums=gsums, mean=mean, invstd=invstd, rm=rmk, rv=rvk)
    assert _finite(*out.values()), "a guard element reached a result, or an element was never written"
    out.update(dgamma=gsums[c:].float(), dbeta=gsums[:c].float())
    return {k: v.clone() for k, v in out.items()}


@pytest.mark.parametrize("m", [1, 255, 257, 5003])
@pytest.mark.parametrize("c", [16, 48, 512])
def test_bn_gelu_chain_guard_bands_and_strides(ops, m, c):
    """cdseg_bn_stats, cdseg_bn_finish, cdseg_bn_gelu_fwd, cdseg_bn_gelu_bwd_sums, cdseg_bn_gelu_bwd_dx.  colsum::partition with
    MIN_ROWS_BN = 256: one row, a block less a row, a block plus a row, and 5003 rows = 20 blocks.  Host checks: `!ld_ok(ldx,
    c)` = `ld >= c && (ld & 3) == 0`, fp32 operands and vectors 16-byte aligned, `(uintptr_t)stats & 7`, running buffers
    `& 3`, the workspace 16-byte aligned and at least cdseg_bn_ws_bytes.  The sums are fp64 in an order fixed by (m, c): every
    result is bit-equal to the op layer's contiguous call in both layouts.  Bound: test_bn_gelu_forward_and_backward_against_fp64's.
    One row: test_gpu_norm's own one-row reference and bound (_one_row_dx_scale)."""
    assert ops.bn_partition(m, c).blocks == {1: 1, 255: 1, 257: 2, 5003: 20}[m]
    x, dy, gamma, beta, rm, rv = NM._data(m, c, 1000 * m + c)
    base = NM._fused(ops, x, dy, gamma, beta, rm, rv)
    ref64, ref32 = NM._torch_chain(x, dy, gamma, beta, rm, rv, torch.float64), NM._torch_chain(x, dy, gamma, beta, rm, rv, F32)
    keys = ("y", "dx", "dgamma", "dbeta", "rm", "rv")
    one_row = NM._one_row_dx_scale(dy, gamma, beta, base["invstd"]) if m == 1 else None
    NM._check_kinds(f"bn_gelu {m}x{c} contiguous", base, c, ref64, ref32, keys, one_row)
    for layout in ("strided", "weak"):
        got = _bn_raw(ops, x, dy, gamma, beta, rm, rv, layout)
        for k in ("y", "dx", "stats", "gsums", "mean", "invstd", "rm", "rv"):
            assert GB.same_bits(got[k], base[k]), f"{layout}: {k} differs from the contiguous call"
        NM._check_kinds(f"bn_gelu {m}x{c} {layout}", got, c, ref64, ref32, keys, one_row)


def test_bn_entry_points_refuse_what_their_kernels_cannot_take(ops):
    """include/cdseg.h: CDSEG_ERR_ARG for a row stride below the row or no multiple of 4, an fp32 operand or vector that is not
    16-byte aligned, statistics that are not 8-byte aligned, m < 0, a workspace that is not 16-byte aligned; CDSEG_ERR_WORKSPACE
    for a short or NULL one; CDSEG_ERR_UNSUPPORTED for a width that is no multiple of 16 or above 512.  Outputs keep their fill."""
    lib = _lib.load()
    m, c = 300, 32
    x, dy, gamma, beta, rm, rv = NM._data(m, c, 1)
    mem = TMem()
    y = mem.out((m, c), F32, fill=-5.0, name="y / dx")
    stats = mem.vout(2 * c + 1, fill=-5.0, dtype=torch.float64, name="stats / gsums")
    mean, invstd = mem.vout(c, fill=-5.0, name="mean"), mem.vout(c, fill=-5.0, name="invstd")
    good = torch.ones(2 * c + 1, dtype=torch.float64, device="cuda")
    need = lib.cdseg_bn_ws_bytes(m, c)
    ws, wb = GB.exact_workspace(need)
    P, st = _p, ops._stream()
    ldy = y.stride(0)

    def stats_(x=x, ld=c, m=m, c=c, stats=stats, ws=ws, nb=need):
        return _err(lib.cdseg_bn_stats(P(x), ld, m, c, P(stats), P(ws), nb, st))

    def finish(stats=good, c=c, mean=mean, invstd=invstd, rm=None, eps=1e-3, mom=0.01):
        return _err(lib.cdseg_bn_finish(P(stats), c, eps, mom, P(mean), P(invstd), P(rm), None, st))

    def fwd(x=x, ld=c, m=m, c=c, mean=gamma, y=y, ldy=ldy):
        return _err(lib.cdseg_bn_gelu_fwd(P(x), ld, m, c, P(mean), P(gamma), P(gamma), P(beta), P(y), ldy, st))

    def sums(x=x, ld=c, dy=dy, lddy=c, m=m, c=c, gs=stats, ws=ws, nb=need):
        return _err(lib.cdseg_bn_gelu_bwd_sums(P(x), ld, P(dy), lddy, m, c, P(gamma), P(gamma), P(gamma), P(beta), P(gs), P(ws), nb, st))

    def dxf(x=x, ld=c, dy=dy, lddy=c, m=m, c=c, gs=good, count=good, dx=y, lddx=ldy):
        return _err(lib.cdseg_bn_gelu_bwd_dx(P(x), ld, P(dy), lddy, m, c, P(gamma), P(gamma), P(gamma), P(beta), P(gs), P(count), P(dx),
                                             lddx, st))

    A, U_, W = "CDSEG_ERR_ARG", "CDSEG_ERR_UNSUPPORTED", "CDSEG_ERR_WORKSPACE"
    for f in (stats_, fwd, sums, dxf):
        assert f(ld=c - 4) == A and f(ld=c + 2) == A and f(ld=0) == A, f.__name__
        assert f(x=x.data_ptr() + 8) == A and f(x=None) == A and f(m=-1) == A, f.__name__
        assert f(c=c + 8) == U_ and f(c=528) == U_ and f(c=0) == U_, f.__name__
    assert stats_(stats=stats.data_ptr() + 4) == A and sums(gs=stats.data_ptr() + 4) == A and dxf(gs=good.data_ptr() + 4) == A
    assert dxf(count=good.data_ptr() + 4) == A and dxf(count=None) == A
    for f in (stats_, sums):
        assert f(ws=ws.data_ptr() + 8) == A and f(nb=need - 1) == W and f(ws=None) == W, f.__name__
    assert sums(lddy=c - 4) == A and sums(dy=dy.data_ptr() + 4) == A and dxf(lddy=c + 2) == A and dxf(dy=None) == A
    assert fwd(ldy=c - 4) == A and fwd(ldy=ldy + 2) == A and fwd(y=y.data_ptr() + 8) == A and fwd(mean=gamma.data_ptr() + 4) == A
    assert dxf(lddx=c - 4) == A and dxf(lddx=ldy + 1) == A and dxf(dx=y.data_ptr() + 4) == A
    assert finish(stats=good.data_ptr() + 4) == A and finish(mean=mean.data_ptr() + 8) == A and finish(invstd=None) == A
    assert finish(rm=rm.data_ptr() + 2) == A and finish(eps=-1.0) == A and finish(mom=1.5) == A and finish(c=24) == U_
    mem.check()
    wb.check()
    assert all(bool((o == -5.0).all()) for o in (y, stats, mean, invstd)) and bool((ws == GB.WorkspaceBand.FILL).all())
    assert stats_() == 0 and finish(stats=stats) == 0 and fwd(mean=mean) == 0  # the same operands with nothing wrong run
    mem.check()
    wb.check()
    assert float(stats[2 * c]) == m and _finite(y, mean, invstd)


# ====================================================================================================== pooling maximum
def _pool_runs(m, seed):
    """m runs of 1 to 8 rows, one of 70 (> 64) and, from three runs on, runs of exactly one row -> (seg int32, cluster int32)."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(1, 9, size=m)
    counts[m // 2] = 70
    if m >= 3:
        counts[0] = counts[m - 1] = 1
    seg = torch.as_tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32)
    return seg, torch.repeat_interleave(torch.arange(m, dtype=torch.int32), torch.as_tensor(counts))


@pytest.mark.parametrize("m", [1, 255, 257, 5003])
@pytest.mark.parametrize("c", [16, 48, 512])
def test_segment_max_arg_and_bwd_guard_bands_and_strides(ops, m, c):
    """cdseg_segment_max_arg / cdseg_segment_max_bwd.  Host checks: `!aligned(15, y, out, arg) || ((uintptr_t)seg_start & 3) ||
    !ld_ok(ldy, c) || !ld_ok(ldo, c) || !ld_ok(lda, c)` (the backward: dout, arg, dy and cluster alike).  arg is banded as int32
    on a stride of its own (fill -1) and is the backward's input where it lies; seg_start and cluster carry edge copies.
    Both are row sweeps on colsum's thread map (`row_grid`, grid-strided), not block sums: m pooled rows at the row counts of
    the BatchNorm group.  Planted ties (the first maximal row wins).  Reference: test_segment_max_arg_and_backward_on_the_pooling_link's - out = the
    bits of cdseg_segment_max, arg = _first_max, dy = _SegmentMax's autograd."""
    from cdsegnet_amd.train_graph import _SegmentMax
    seg, cluster = _pool_runs(m, m + c)
    n = int(seg[-1])
    g = torch.Generator().manual_seed(m + c)
    y = torch.randn(n, c, generator=g)
    a0 = int(seg[m // 2])
    y[[a0 + 3, a0 + 40, a0 + 69]] = 9.0  # a tie inside the long run: the first of the three wins
    y, segd, cld = y.cuda(), seg.cuda(), cluster.cuda()
    out, arg = ops.segment_max_arg(y, segd, m)
    want = torch.empty(m, c, device="cuda")
    one = torch.ones(c, device="cuda")
    ops.segment_max(y, segd, m, one, torch.zeros_like(one), ops.ACT_NONE, want)
    torch.cuda.synchronize()
    assert GB.same_bits(out, want) and torch.equal(arg.long(), NM._first_max(y, want, cld.long(), m))
    assert bool((arg[m // 2] == a0 + 3).all())
    dout = torch.randn(m, c, generator=g).cuda()
    dy = ops.segment_max_bwd(dout, arg, cld)
    yr = y.clone().requires_grad_(True)
    _SegmentMax.apply(yr, segd, cld, m).backward(dout)
    torch.cuda.synchronize()
    assert torch.equal(dy, yr.grad)
    lib = _lib.load()
    P, st = _p, ops._stream()
    for layout in ("strided", "weak"):
        lay = (lambda s, dt=F32: dict(ld=c + 4, cols=0)) if layout == "weak" else (lambda s, dt=F32: dict(ld=_lds(c, dt, "strided", s)))
        mem = TMem()
        yk = mem.inp(y, name="y", **lay(0))
        o, a = mem.out((m, c), F32, name="out", **lay(1)), mem.out((m, c), torch.int32, fill=-1, name="arg", **lay(2, torch.int32))
        assert lib.cdseg_segment_max_arg(P(yk), yk.stride(0), P(mem.index(segd)), m, c, P(o), o.stride(0), P(a), a.stride(0), st) == 0
        mem.check()
        assert GB.same_bits(o, out) and torch.equal(a, arg), layout
        dk, d = mem.inp(dout, name="dout", **lay(3)), mem.out((n, c), F32, name="dy", **lay(4))
        assert lib.cdseg_segment_max_bwd(P(dk), dk.stride(0), P(a), a.stride(0), P(mem.index(cld)), n, c, P(d), d.stride(0), st) == 0
        mem.check()
        assert torch.equal(a, arg), "the backward wrote its index operand"
        assert GB.same_bits(d, dy), layout


def test_segment_max_arg_and_bwd_refuse_what_their_kernels_cannot_take(ops):
    """include/cdseg.h: CDSEG_ERR_ARG for a stride below the row or no multiple of 4, y / out / arg / dout / dy that are not 16-byte
    aligned, seg_start / cluster that are not 4-byte aligned, NULL operands, a negative count; CDSEG_ERR_UNSUPPORTED for a width
    that is no multiple of 16 or above 512 and for 2^31 rows.  Outputs keep their fill."""
    lib = _lib.load()
    m, c = 5, 32
    seg, cluster = _pool_runs(m, 0)
    n = int(seg[-1])
    y, dout, segd, cld = torch.randn(n, c, device="cuda"), torch.randn(m, c, device="cuda"), seg.cuda(), cluster.cuda()
    mem = TMem()
    out, dy = mem.out((m, c), F32, fill=-5.0, name="out"), mem.out((n, c), F32, fill=-5.0, name="dy")
    arg = mem.out((m, c), torch.int32, fill=-7, name="arg")
    P, st = _p, ops._stream()
    lo, la, ld_ = out.stride(0), arg.stride(0), dy.stride(0)

    def fwd(y=y, ldy=c, seg=segd, m=m, c=c, out=out, ldo=lo, arg=arg, lda=la):
        return _err(lib.cdseg_segment_max_arg(P(y), ldy, P(seg), m, c, P(out), ldo, P(arg), lda, st))

    def bwd(dout=dout, lddo=c, arg=arg, lda=la, cl=cld, n=n, c=c, dy=dy, lddy=ld_):
        return _err(lib.cdseg_segment_max_bwd(P(dout), lddo, P(arg), lda, P(cl), n, c, P(dy), lddy, st))

    A, U_ = "CDSEG_ERR_ARG", "CDSEG_ERR_UNSUPPORTED"
    for name in ("ldy", "ldo", "lda"):
        assert fwd(**{name: c - 4}) == A and fwd(**{name: c + 2}) == A and fwd(**{name: 0}) == A, name
    for name in ("lddo", "lda", "lddy"):
        assert bwd(**{name: c - 4}) == A and bwd(**{name: c + 2}) == A and bwd(**{name: 0}) == A, name
    for name, t in (("y", y), ("out", out), ("arg", arg)):
        assert fwd(**{name: t.data_ptr() + 8}) == A and fwd(**{name: None}) == A, name
    for name, t in (("dout", dout), ("arg", arg), ("dy", dy)):
        assert bwd(**{name: t.data_ptr() + 8}) == A and bwd(**{name: None}) == A, name
    assert fwd(seg=segd.data_ptr() + 2) == A and fwd(seg=None) == A and bwd(cl=cld.data_ptr() + 2) == A and bwd(cl=None) == A
    assert fwd(m=-1) == A and bwd(n=-1) == A
    for f, cnt in ((fwd, "m"), (bwd, "n")):
        assert f(c=c + 8) == U_ and f(c=528) == U_ and f(**{cnt: 1 << 31}) == U_, f.__name__
    mem.check()
    assert bool((out == -5.0).all()) and bool((dy == -5.0).all()) and bool((arg == -7).all())
    assert fwd() == 0 and bwd() == 0  # the same operands with nothing wrong run
    mem.check()
    assert _finite(out, dy) and int(arg.min()) >= 0


# ====================================================================================================== row kernels (csrc/trainblock.hip)
# These entry points know no row stride: rows are contiguous, so every operand sits between guard ROWS (GB.banded with cols = 0)
# or guard elements (vectors), and the host checks (`(c & 3)`, `!al16(...)`, `(count & 3)`) admit nothing weaker than the
# guarded call itself - leg 3 is leg 2 for them.  n * (c / 4) items over ROW_BLOCK = 256 threads: one row, 65 rows, and the n
# at which the item count is one more than a multiple of 256 (c = 4: 257; c = 516: 129; c = 32 has none, 8 n is even).
ROW_SHAPES = [(1, 4), (65, 4), (257, 4), (1, 32), (65, 32), (1, 516), (65, 516), (129, 516)]
ROW_IDS = [f"{n}x{c}" for n, c in ROW_SHAPES]


def _rows_out(mem, shape, dtype, name):
    """(a finite fill: a row copied over from an input's NaN guard would not show against NaN guards of the output; an element
    that was never written shows in the bit comparison with the contiguous call)"""
    return mem.out(shape, dtype, name=name, cols=0, fill=-777.25)


def _code(ops, out):
    return ops.F32 if out == "fp32" else ops.BF16


@KINDS
@pytest.mark.parametrize("n,c", ROW_SHAPES, ids=ROW_IDS)
def test_elementwise_row_kernels_between_guard_rows(ops, lp, n, c):
    """cdseg_residual (every optional operand present and absent, in place), cdseg_scale_cast, cdseg_gelu_fwd,
    cdseg_gelu_bwd_cast, the latter three with fp32 and 16-bit outputs.  References: the torch expressions of
    test_residual_forward_and_backward_are_bit_equal_to_torch / test_cast_without_saturation_is_torchs_cast (bit-equal) and
    test_gelu_forward_and_backward_vs_fp64_within_three_times_torch's bound."""
    lib = _lib.load()
    variant = None if lp == "fp32" else lp
    odt = _t(lp)
    g = torch.Generator().manual_seed(n + c)
    x, a, dy = (torch.randn(n, c, generator=g).cuda() for _ in range(3))
    m = TB._mask(n, g).cuda()
    offs_host = [0, n] if n == 1 else [0, max(1, n // 3), n]
    offs = torch.tensor(offs_host, dtype=torch.int32).cuda()
    t_rows = torch.randn(len(offs_host) - 1, c, generator=g).cuda()
    batch = torch.repeat_interleave(torch.arange(len(offs_host) - 1), torch.tensor(np.diff(offs_host))).cuda()
    P, st = _p, ops._stream()
    # residual: (a, mask, t_rows) present / absent
    for ua, um, ut in ((1, 0, 0), (1, 1, 0), (1, 1, 1), (0, 0, 1)):
        want = x
        if ua:
            want = x + (a * m[:, None] if um else a)
        if ut:
            want = want + t_rows[batch]
        base = ops.residual(x, a if ua else None, m if um else None, t_rows if ut else None, offs if ut else None)
        assert TB._bits(base, want), (ua, um, ut)
        mem = TMem()
        xk, ak, tk = mem.inp(x, name="x", cols=0), mem.inp(a, name="a", cols=0), mem.inp(t_rows, name="t_rows", cols=0)
        mk, ok, out = mem.vin(m, name="mask"), mem.index(offs), _rows_out(mem, (n, c), F32, "out")
        assert lib.cdseg_residual(P(xk), P(ak) if ua else None, P(mk) if um else None, P(tk) if ut else None, P(ok) if ut else None,
                                  len(offs_host) - 1 if ut else 0, P(out), n, c, st) == 0
        mem.check()
        assert GB.same_bits(out, base), (ua, um, ut)
    mem = TMem()
    xio = mem.rmw(x, name="x (in place)", cols=0)
    assert lib.cdseg_residual(P(xio), P(mem.inp(a, name="a", cols=0)), P(mem.vin(m, name="mask")), None, None, 0, P(xio), n, c, st) == 0
    mem.check()
    assert TB._bits(xio.contiguous(), x + a * m[:, None])
    # scale_cast (no saturation), with and without the mask
    for um in (0, 1):
        base = ops.scale_cast(dy, m if um else None, variant)
        assert TB._bits_nan(base, (dy * m[:, None] if um else dy).to(odt))
        mem = TMem()
        out = _rows_out(mem, (n, c), odt, "out")
        assert lib.cdseg_scale_cast(P(mem.inp(dy, name="dy", cols=0)), P(mem.vin(m, name="mask")) if um else None, P(out), _code(ops, lp),
                                    n, c, st) == 0
        mem.check()
        assert GB.same_bits(out, base), um
    # GELU forward and backward on the flat (n * c) elements
    u = (2.0 * torch.randn(n, c, generator=g)).cuda()
    u64 = u.double().requires_grad_(True)
    g64 = torch.nn.functional.gelu(u64)
    g64.backward(dy.double())
    u32 = u.clone().requires_grad_(True)
    g32 = torch.nn.functional.gelu(u32)
    g32.backward(dy)
    to = lambda t: t.to(odt)  # noqa: E731
    base_g, base_du = ops.gelu_fwd(u, variant), ops.gelu_bwd_cast(u, dy, variant)
    TB._assert_vs_torch(f"gelu {lp} {n}x{c} contiguous",
                        [("g", base_g, to(g32.detach()), g64.detach()), ("du", base_du, to(u32.grad), u64.grad)])
    mem = TMem()
    uk, dk = mem.inp(u, name="u", cols=0), mem.inp(dy, name="dg", cols=0)
    og, od = _rows_out(mem, (n, c), odt, "g"), _rows_out(mem, (n, c), odt, "du")
    assert lib.cdseg_gelu_fwd(P(uk), P(og), _code(ops, lp), n * c, st) == 0
    assert lib.cdseg_gelu_bwd_cast(P(uk), P(dk), P(od), _code(ops, lp), n * c, st) == 0
    mem.check()
    assert GB.same_bits(og, base_g) and GB.same_bits(od, base_du)


@KINDS
@pytest.mark.parametrize("n,c", ROW_SHAPES, ids=ROW_IDS)
def test_run_row_kernels_between_guard_rows(ops, lp, n, c):
    """cdseg_gather_first (fp32 and saturating 16-bit output), cdseg_residual_rows (with and without the per-scene rows),
    cdseg_run_sum, cdseg_scatter_first in both accumulate modes, on runs of 1 to 5 rows with a run at row 0 and at the last
    row.  row_start / row_vox / scene_offs are index operands with edge copies around them (the ABI knows no "none" for
    them).  References: the torch expressions of test_row_kernels_are_bit_equal_to_torch, bit for bit."""
    lib = _lib.load()
    variant = None if lp == "fp32" else lp
    odt = _t(lp)
    rng = np.random.default_rng(n + c)
    lengths, left = ([3], n - 5) if n >= 7 else ([], n)
    while left > 0:
        k = min(left, int(rng.choice([1, 1, 2, 3, 5])))
        lengths.append(k)
        left -= k
    lengths += [2] if n >= 7 else []
    nv = len(lengths)
    row_start = torch.as_tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int32).cuda()
    row_vox = torch.as_tensor(np.repeat(np.arange(nv), lengths), dtype=torch.int32).cuda()
    assert int(row_start[-1]) == n
    g = torch.Generator().manual_seed(n + c)
    x, a = torch.randn(n, c, generator=g).cuda() * 50.0, torch.randn(nv, c, generator=g).cuda()
    first, vox = row_start[:-1].long(), row_vox.long()
    offs_host = [0, n] if n == 1 else [0, max(1, n // 3), n]
    offs = torch.tensor(offs_host, dtype=torch.int32).cuda()
    t_rows = torch.randn(len(offs_host) - 1, c, generator=g).cuda()
    scene = torch.repeat_interleave(torch.arange(len(offs_host) - 1), torch.tensor(np.diff(offs_host))).cuda()
    P, st = _p, ops._stream()
    # gather_first
    base = ops.gather_first(x, row_start, variant)
    assert TB._bits(base, x[first] if variant is None else ops.cast(x[first].contiguous(), odt))
    mem = TMem()
    out = _rows_out(mem, (nv, c), odt, "out")
    assert lib.cdseg_gather_first(P(mem.inp(x, name="x", cols=0)), P(mem.index(row_start)), P(out), _code(ops, lp), nv, c, st) == 0
    mem.check()
    assert GB.same_bits(out, base)
    if lp != "fp32":
        return  # (the other three are fp32 only: once is enough)
    # residual_rows
    for ut in (0, 1):
        want = (x + a[vox]) + t_rows[scene] if ut else x + a[vox]
        base = ops.residual_rows(x, a, row_vox, t_rows if ut else None, offs if ut else None)
        assert TB._bits(base, want), ut
        mem = TMem()
        out = _rows_out(mem, (n, c), F32, "out")
        assert lib.cdseg_residual_rows(P(mem.inp(x, name="x", cols=0)), P(mem.inp(a, name="a", cols=0)), P(mem.index(row_vox)),
                                       P(mem.inp(t_rows, name="t_rows", cols=0)) if ut else None, P(mem.index(offs)) if ut else None,
                                       len(offs_host) - 1 if ut else 0, P(out), n, c, st) == 0
        mem.check()
        assert GB.same_bits(out, base), ut
    # run_sum
    want = torch.zeros(nv, c, device="cuda")
    length = (row_start[1:] - row_start[:-1]).long()
    for k in range(int(length.max())):
        has = length > k
        want[has] = want[has] + x[first[has] + k]
    base = ops.run_sum(x, row_start)
    assert TB._bits(base, want)
    mem = TMem()
    out = _rows_out(mem, (nv, c), F32, "out")
    assert lib.cdseg_run_sum(P(mem.inp(x, name="dx", cols=0)), P(mem.index(row_start)), P(out), nv, c, st) == 0
    mem.check()
    assert GB.same_bits(out, base)
    # scatter_first: set (the other rows become zero) and accumulate (the other rows keep their bits)
    z = torch.zeros(n, c, device="cuda")
    z[first] = a
    assert TB._bits(ops.scatter_first(a, row_vox, row_start), z)
    acc_want = x.clone()
    acc_want[first] = x[first] + a
    for acc, want in ((0, z), (1, acc_want)):
        mem = TMem()
        dx = mem.rmw(x, name="dx", cols=0) if acc else _rows_out(mem, (n, c), F32, "dx")
        assert lib.cdseg_scatter_first(P(mem.inp(a, name="g", cols=0)), P(mem.index(row_vox)), P(mem.index(row_start)), P(dx), acc, n, c,
                                       st) == 0
        mem.check()
        assert TB._bits(dx.contiguous(), want), acc


ALN_SHAPES = [(1, 4), (65, 32), (65, 64), (1, 516), (65, 516), (65, 512), (5, 1024), (5, 2048)]


@KINDS
@pytest.mark.parametrize("n,c", ALN_SHAPES, ids=[f"{n}x{c}" for n, c in ALN_SHAPES])
def test_add_layernorm_between_guard_rows(ops, lp, n, c):
    """cdseg_add_layernorm with and without the mask, h in fp32 and in the 16-bit type: tpr = the power of two >= c / 4 (<= 64)
    lanes per row, MV = ceil(c / 4 / tpr) chunks per lane in {1, 2, 4, 8}: c = 64 (1), 512 (2), 1024 (4), 2048 (8), and 516 (3
    chunks in the MV = 4 instantiation, the last lane's chunks past the row).  Reference and bound:
    test_add_layernorm_vs_fp64_within_three_times_torch's (x1 bit-equal to torch, h <= 3 E_torch + 2^-24)."""
    lib = _lib.load()
    variant = None if lp == "fp32" else lp
    odt = _t(lp)
    g = torch.Generator().manual_seed(n + c)
    gamma, beta = (1 + 0.3 * torch.randn(c, generator=g)).cuda(), (0.1 * torch.randn(c, generator=g)).cuda()
    x, a = (0.5 + torch.randn(n, c, generator=g)).cuda(), torch.randn(n, c, generator=g).cuda()
    P, st = _p, ops._stream()
    for m in (None, TB._mask(n, g).cuda()):
        with ops.record_routes() as rr:
            x1, h = ops.add_layernorm(x, a, m, gamma, beta, 1e-5, variant)
        if c in (64, 512, 1024, 2048):
            mv = {64: 1, 512: 2, 1024: 4, 2048: 8}[c]
            assert rr.count == 1 and f"<{mv}," in rr.kernels()[0].replace(" ", ""), rr.kernels()
        want = x + (a if m is None else a * m[:, None])
        assert TB._bits(x1, want)
        h64 = torch.nn.functional.layer_norm(want.double(), (c,), gamma.double(), beta.double(), 1e-5)
        h32 = torch.nn.functional.layer_norm(want, (c,), gamma, beta, 1e-5).to(odt)
        TB._assert_vs_torch(f"add_layernorm {lp} {n}x{c} mask={m is not None} contiguous", [("h", h, h32, h64)])
        mem = TMem()
        ox, oh = _rows_out(mem, (n, c), F32, "x1"), _rows_out(mem, (n, c), odt, "h")
        assert lib.cdseg_add_layernorm(P(mem.inp(x, name="x", cols=0)), P(mem.inp(a, name="a", cols=0)),
                                       None if m is None else P(mem.vin(m, name="mask")), P(mem.vin(gamma, name="gamma")),
                                       P(mem.vin(beta, name="beta")), 1e-5, P(ox), P(oh), _code(ops, lp), n, c, st) == 0
        mem.check()
        assert GB.same_bits(ox, x1) and GB.same_bits(oh, h)


def test_row_kernels_refuse_what_they_cannot_take(ops):
    """include/cdseg.h / the host checks of csrc/trainblock.hip: CDSEG_ERR_ARG for `c & 3` (`count & 3` for the two GELU entry
    points), an fp32 or 16-bit operand that is not 16-byte aligned, an index array that is not 4-byte aligned, a NULL operand,
    a mask without a, per-scene rows without their offsets, another out_dtype, c > 2048 (add_layernorm).  Outputs keep their fill."""
    lib = _lib.load()
    n, c = 9, 8
    x, a = torch.randn(n, c, device="cuda"), torch.randn(n, c, device="cuda")
    vec, m = torch.ones(c, device="cuda"), torch.ones(n, device="cuda")
    idx = torch.arange(n + 1, dtype=torch.int32, device="cuda")
    mem = TMem()
    out, out2 = mem.out((n, c), F32, fill=-5.0, cols=0, name="out"), mem.out((n, c), F32, fill=-5.0, cols=0, name="x1")
    P, st, A = _p, ops._stream(), "CDSEG_ERR_ARG"
    X, O, I = P(x), P(out), P(idx)
    calls = {
        "residual": lambda x=X, a=P(a), mask=None, t=None, offs=None, ns=0, out=O, c=c:
            lib.cdseg_residual(x, a, mask, t, offs, ns, out, n, c, st),
        "gather_first": lambda x=X, rs=I, out=O, code=ops.F32, c=c: lib.cdseg_gather_first(x, rs, out, code, n, c, st),
        "residual_rows": lambda x=X, a=P(a), rv=I, t=None, offs=None, ns=0, out=O, c=c:
            lib.cdseg_residual_rows(x, a, rv, t, offs, ns, out, n, c, st),
        "run_sum": lambda x=X, rs=I, out=O, c=c: lib.cdseg_run_sum(x, rs, out, n, c, st),
        "scatter_first": lambda x=X, rv=I, rs=I, out=O, c=c: lib.cdseg_scatter_first(x, rv, rs, out, 0, n, c, st),
        "scale_cast": lambda x=X, mask=None, out=O, code=ops.F32, c=c: lib.cdseg_scale_cast(x, mask, out, code, n, c, st),
        "add_layernorm": lambda x=X, a=P(a), g=P(vec), b=P(vec), x1=P(out2), out=O, code=ops.F32, c=c:
            lib.cdseg_add_layernorm(x, a, None, g, b, 1e-5, x1, out, code, n, c, st),
        "gelu_fwd": lambda x=X, out=O, code=ops.F32, count=n * c: lib.cdseg_gelu_fwd(x, out, code, count, st),
        "gelu_bwd_cast": lambda x=X, a=P(a), out=O, code=ops.F32, count=n * c: lib.cdseg_gelu_bwd_cast(x, a, out, code, count, st),
    }
    for name, f in calls.items():
        assert _err(f(x=X + 8)) == A and _err(f(x=None)) == A and _err(f(out=O + 8)) == A and _err(f(out=None)) == A, name
        if "gelu" in name:
            assert _err(f(count=n * c - 2)) == A, name
        else:
            assert _err(f(c=c - 2)) == A and _err(f(c=0)) == A, name
        if name in ("gather_first", "scale_cast", "add_layernorm", "gelu_fwd", "gelu_bwd_cast"):
            assert _err(f(code=7)) == A, name
        if name in ("residual", "residual_rows", "add_layernorm", "gelu_bwd_cast"):
            assert _err(f(a=P(a) + 8)) == A, name
        if name in ("gather_first", "run_sum", "scatter_first"):
            assert _err(f(rs=I + 2)) == A and _err(f(rs=None)) == A, name
        if name in ("residual_rows", "scatter_first"):
            assert _err(f(rv=I + 2)) == A and _err(f(rv=None)) == A, name
        if name in ("residual", "residual_rows"):
            assert _err(f(t=X, offs=None, ns=1)) == A and _err(f(t=X, offs=I, ns=0)) == A and _err(f(t=X + 8, offs=I, ns=1)) == A, name
    assert _err(calls["residual"](a=None, mask=P(m))) == A and _err(calls["residual_rows"](a=None)) == A
    f = calls["add_layernorm"]
    assert _err(f(g=P(vec) + 8)) == A and _err(f(b=None)) == A and _err(f(x1=P(out2) + 8)) == A and _err(f(c=2052)) == A
    mem.check()
    assert bool((out == -5.0).all()) and bool((out2 == -5.0).all())
    assert _err(calls["add_layernorm"]()) == 0  # the same operands with nothing wrong run
    mem.check()
    assert _finite(out, out2)


# ====================================================================================================== fused segmentation loss
def _loss_raw(ops, logits, labels, kw_logits, kw_dlogits):
    """cdseg_seg_loss_fwd (phase 0: the label histogram, phase 1: the loss) and cdseg_seg_loss_bwd under each upstream scalar,
    through the C ABI: logits poisoned on ldl, labels between edge copies, hist / out / the scalars between guard elements, coef
    (n, present; no stride of its own) between guard rows, the workspace at exactly cdseg_seg_loss_ws_bytes, dlogits banded on
    lddl.  -> dict as test_gpu_seg_loss's fused()."""
    lib = _lib.load()
    n, c = logits.shape
    mem = TMem()
    lg, lb = mem.inp(logits, name="logits", **kw_logits), mem.index(labels)
    hist = mem.vout(c + 1, fill=-7, dtype=torch.int32, name="hist")
    P, st, ign = _p, ops._stream(), SL.IGNORE
    assert lib.cdseg_seg_loss_fwd(P(lg), lg.stride(0), P(lb), n, c, ign, 0, P(hist), None, None, None, None, 0, st) == 0
    mem.check()
    hl = hist.tolist()
    hist_host = (ctypes.c_int32 * (c + 1))(*hl)
    present = sum(1 for v in hl[:c] if v)
    out, coef = mem.vout(2, fill=NAN, name="out"), mem.out((n, present), F32, cols=0, name="coef")
    need = lib.cdseg_seg_loss_ws_bytes(n, c)
    ws, wb = GB.exact_workspace(need)
    assert lib.cdseg_seg_loss_fwd(P(lg), lg.stride(0), P(lb), n, c, ign, 1, None, hist_host, P(out), P(coef), P(ws), need, st) == 0
    mem.check()
    wb.check()
    one = mem.vin(torch.ones(1, device="cuda"), name="g")
    d = []
    for which in (0, 1):
        dl = mem.out((n, c), F32, name="dlogits", **kw_dlogits)
        assert lib.cdseg_seg_loss_bwd(P(lg), lg.stride(0), P(lb), n, c, ign, hist_host, P(coef), None if which else P(one),
                                      P(one) if which else None, P(dl), dl.stride(0), st) == 0
        d.append(dl)
    mem.check()
    assert _finite(out, *d), "a guard element reached a result, or an element was never written"
    return dict(ce=out[0].double().cpu(), lovasz=out[1].double().cpu(), d_ce=d[0].double().cpu(), d_lovasz=d[1].double().cpu()), sum(hl[:c])


LOSS_SHAPES = [(1, 13), (65, 16), (65, 17)]


@pytest.mark.parametrize("lp", ["bf16", "f16"])
@pytest.mark.parametrize("variant", ["strided", "ignore7"])
@pytest.mark.parametrize("n,c", LOSS_SHAPES, ids=[f"{n}x{c}" for n, c in LOSS_SHAPES])
def test_seg_loss_guard_bands_and_strides(ops, lp, n, c, variant):
    """cdseg_seg_loss_fwd / cdseg_seg_loss_bwd at test_gpu_seg_loss's smallest case and on both sides of launch_by_width's first
    boundary (`c <= 16`: 16 lanes a row with one class each, then two).  Host checks: `ldl < c`, `lddl < c`, `(uintptr_t)logits
    & 3`, `(uintptr_t)labels & 7`, out / coef / dlogits / the scalars `& 3`, ws `& 15` and at least cdseg_seg_loss_ws_bytes:
    nothing holds a stride to a multiple, so the weak layouts are odd strides - lddl == c against a wide odd ldl and the
    reverse.  The sums run in a fixed order (test_four_calls_give_the_same_bits): every layout is bit-equal to the op layer's
    call.  Bound: test_fused_loss_is_as_accurate_as_the_torch_criteria's (2 E_ref + 2^-24 max |reference|)."""
    t, labels, win, o, tor = SL.reference(n, c, variant)
    base, saved = SL.fused(ops, t, labels, win)
    logits = (t if win is None else t[:, win[0]:win[1]]).cuda().contiguous()

    def versus_oracle(what, got):
        for k in ("ce", "lovasz", "d_ce", "d_lovasz"):
            top, e_ref, e_ker = float(o[k].abs().max()), float((tor[k] - o[k]).abs().max()), float((got[k] - o[k]).abs().max())
            report(f"seg_loss {n}x{c} {variant} {what} {k}", kernel_err=e_ker, E_ref=e_ref, bound=2.0 * e_ref + 2.0 ** -24 * top)
            assert e_ker <= 2.0 * e_ref + 2.0 ** -24 * top, (what, k, e_ker, e_ref, top)

    versus_oracle("contiguous", base)
    layouts = {"strided": (dict(ld=_lds(c, F32, "strided", 0)), dict(ld=_lds(c, F32, "strided", 1))),
               "ldl wide and odd, lddl == c": (dict(ld=c + 9, align=4, cols=0), dict(cols=0)),
               "ldl == c, lddl wide and odd": (dict(cols=0), dict(ld=c + 9, align=4, cols=0))}
    for what, (kl, kd) in layouts.items():
        got, n_valid = _loss_raw(ops, logits, labels.cuda(), kl, kd)
        assert n_valid == o["n_valid"] == saved["n_valid"]
        for k in got:
            assert torch.equal(got[k], base[k]), f"{what}: {k} differs from the op layer's call"
        versus_oracle(what, got)
        dead = labels == SL.IGNORE
        if bool(dead.any()):  # ignored rows: exact zeros
            assert float(got["d_ce"][dead].abs().max()) == 0.0 and float(got["d_lovasz"][dead].abs().max()) == 0.0


def test_seg_loss_refuses_what_its_kernels_cannot_take(ops):
    """include/cdseg.h: CDSEG_ERR_ARG for ldl < c, lddl < c, logits / out / coef / dlogits / a scalar that is not 4-byte aligned,
    labels that are not 8-byte aligned, a NULL operand, another phase, a workspace that is not 16-byte aligned;
    CDSEG_ERR_WORKSPACE for a short or NULL one; CDSEG_ERR_UNSUPPORTED above the class limit.  Outputs keep their fill."""
    lib = _lib.load()
    n, c = 65, 16
    t, labels, win = SL.make_case(n, c, "ignore7")
    logits, lb = t.cuda(), labels.cuda()
    hl = torch.bincount(labels[labels >= 0], minlength=c).tolist() + [0]
    hist_host = (ctypes.c_int32 * (c + 1))(*hl)
    present = sum(1 for v in hl[:c] if v)
    mem = TMem()
    hist = mem.vout(c + 1, fill=-7, dtype=torch.int32, name="hist")
    out, coef = mem.vout(2, fill=-5.0, name="out"), mem.out((n, present), F32, fill=-5.0, cols=0, name="coef")
    dl = mem.out((n, c), F32, fill=-5.0, name="dlogits")
    cf = torch.zeros(n, present, device="cuda")
    one = torch.ones(1, device="cuda")
    need = lib.cdseg_seg_loss_ws_bytes(n, c)
    ws, wb = GB.exact_workspace(need)
    P, st, A, W = _p, ops._stream(), "CDSEG_ERR_ARG", "CDSEG_ERR_WORKSPACE"

    def fwd(phase, lg=logits, ldl=c, lab=lb, c=c, hist=hist, hh=hist_host, out=out, coef=coef, ws=ws, nb=need):
        return _err(lib.cdseg_seg_loss_fwd(P(lg), ldl, P(lab), n, c, -1, phase, P(hist), hh, P(out), P(coef), P(ws), nb, st))

    def bwd(lg=logits, ldl=c, lab=lb, c=c, hh=hist_host, coef=cf, g=one, dl=dl, lddl=dl.stride(0)):
        return _err(lib.cdseg_seg_loss_bwd(P(lg), ldl, P(lab), n, c, -1, hh, P(coef), P(g), None, P(dl), lddl, st))

    for f in (lambda **kw: fwd(0, **kw), lambda **kw: fwd(1, **kw), bwd):
        assert f(ldl=c - 1) == A and f(ldl=0) == A and f(lg=logits.data_ptr() + 2) == A and f(lg=None) == A
        assert f(lab=lb.data_ptr() + 4) == A and f(lab=None) == A and f(c=0) == A and f(c=257, ldl=260) == "CDSEG_ERR_UNSUPPORTED"
    assert fwd(2) == A and fwd(0, hist=None) == A and fwd(0, hist=hist.data_ptr() + 2) == A
    assert fwd(1, hh=None) == A and fwd(1, out=None) == A and fwd(1, out=out.data_ptr() + 2) == A and fwd(1, coef=coef.data_ptr() + 2) == A
    assert fwd(1, ws=ws.data_ptr() + 8) == A and fwd(1, ws=None) == W and fwd(1, nb=need - 1) == W
    assert bwd(lddl=c - 1) == A and bwd(lddl=0) == A and bwd(dl=dl.data_ptr() + 2) == A and bwd(dl=None) == A
    assert bwd(coef=cf.data_ptr() + 2) == A and bwd(coef=None) == A and bwd(g=one.data_ptr() + 2) == A and bwd(hh=None) == A
    mem.check()
    wb.check()
    assert bool((hist == -7).all()) and all(bool((o_ == -5.0).all()) for o_ in (out, coef, dl)) and bool((ws == GB.WorkspaceBand.FILL).all())
    assert fwd(0) == 0 and fwd(1) == 0 and bwd(coef=coef) == 0  # the same operands with nothing wrong run
    mem.check()
    wb.check()
    assert hist.tolist() == hl and _finite(out, dl)


# ====================================================================================================== fused optimizer step
OPT_SIZES = [OPT.CHUNK - 1, OPT.CHUNK, OPT.CHUNK + 1]  # a chunk less one element, one chunk, a chunk and one element
OPT_NORM = 1.0


def _opt_raw(ops, p0, grads, aligns, found=0.0, state=None):
    """cdseg_grad_norm + cdseg_adamw_step through the C ABI: every p, g, m, v, 16-bit copy and step counter of the three tensors
    in a guarded 1-D buffer of its own (aligns: data_ptr() % 16 of p, g, m, v and of the 16-bit copy), the norm's three outputs and
    the AMP scalars between guard elements, the workspace at exactly cdseg_opt_ws_bytes.  Tensor i belongs to group i % 2 and
    is clipped, as in test_gpu_optim.  state: (m, v, steps) to continue from.  -> (p, m, v, p16, step lists; out; Mem)."""
    lib = _lib.load()
    count = len(p0)
    mem = TMem()
    ap, ag, am, av, a16 = aligns
    z = lambda n: torch.zeros(n, device="cuda")  # noqa: E731
    ps = [mem.vout(t.numel(), fill=-5.0, align=ap, name=f"p[{i}]", pre=t.cuda()) for i, t in enumerate(p0)]
    gs = [mem.vin(t.cuda(), align=ag, name=f"g[{i}]") for i, t in enumerate(grads)]
    old = (lambda k, i, n: z(n)) if state is None else (lambda k, i, n: state[k][i])
    ms = [mem.vout(t.numel(), fill=-5.0, align=am, name=f"m[{i}]", pre=old(0, i, t.numel())) for i, t in enumerate(p0)]
    vs = [mem.vout(t.numel(), fill=-5.0, align=av, name=f"v[{i}]", pre=old(1, i, t.numel())) for i, t in enumerate(p0)]
    p16 = [mem.vout(t.numel(), fill=-7.0, align=a16, dtype=LP(), name=f"p16[{i}]") for i, t in enumerate(p0)]
    steps = [mem.vout(1, fill=-5.0, align=ap, name=f"step[{i}]", pre=z(1) if state is None else state[2][i]) for i in range(count)]
    out = mem.vout(3, fill=NAN, name="out")
    fnd = mem.vin(torch.full((1,), found, device="cuda"), name="found_inf")
    scale = mem.vin(torch.full((1,), 4.0, device="cuda"), name="grad_scale", align=4)
    table = (_lib.OptTensor * count)()
    for i, e in enumerate(table):
        e.p, e.g, e.m, e.v, e.p16, e.step = (t[i].data_ptr() for t in (ps, gs, ms, vs, p16, steps))
        e.n, e.group, e.flags = p0[i].numel(), i % 2, 1  # CDSEG_OPT_CLIP
    groups = (_lib.OptGroup * 2)()
    for ge, g in zip(groups, OPT.GROUPS):
        ge.lr, ge.beta1, ge.beta2, ge.eps, ge.weight_decay = g["lr"], OPT.BETAS[0], OPT.BETAS[1], OPT.EPS, g["weight_decay"]
    sizes = (ctypes.c_long * count)(*[t.numel() for t in p0])
    nch = ctypes.c_long()
    assert lib.cdseg_opt_chunks(sizes, count, None, ctypes.byref(nch)) == 0 and nch.value == 1 + 1 + 2
    chunks = (ctypes.c_int32 * (2 * nch.value))()
    assert lib.cdseg_opt_chunks(sizes, count, chunks, ctypes.byref(nch)) == 0
    chunks_dev = mem.index(torch.tensor(list(chunks), dtype=torch.int32).cuda())
    need = lib.cdseg_opt_ws_bytes(count, nch.value)
    ws, wb = GB.exact_workspace(need)
    P, st = _p, ops._stream()
    assert lib.cdseg_grad_norm(table, count, P(chunks_dev), nch.value, P(scale), OPT_NORM, P(out), P(ws), need, st) == 0
    assert lib.cdseg_adamw_step(table, count, groups, 2, P(chunks_dev), nch.value, P(scale), P(fnd), out.data_ptr() + 4, P(ws), need, st) == 0
    mem.check()
    wb.check()
    return ps, ms, vs, p16, steps, out


@pytest.mark.parametrize("lp", ["bf16", "f16"])
def test_optimizer_step_between_guard_elements(ops, lp):
    """cdseg_grad_norm / cdseg_adamw_step on three tensors of CDSEG_OPT_CHUNK - 1, CDSEG_OPT_CHUNK and CDSEG_OPT_CHUNK + 1 elements
    (the last one spills one element into a second chunk), with a GradScaler scale, the clip by the global norm and the 16-bit
    copies, two steps.  Host checks (check_table / check_work): p, g, m, v, step `& 3`, `(uintptr_t)e.p16 & 1`, the scalars
    `& 3`, ws `& 15` and at least cdseg_opt_ws_bytes - the weak layout is bases at +4 / +8 / +12 bytes and a 16-bit copy at
    +2 bytes (the scalar path).  Every sum runs in an order fixed by the chunk list and the update is element-wise: both
    layouts are bit-equal to FusedAdamW's step on ordinary tensors (test_two_runs_in_different_allocations_give_equal_bits).
    Bound: test_update_against_fp64_is_as_good_as_torch's rule (_judge) against torch.optim.AdamW on clipped, unscaled gradients."""
    from cdsegnet_amd.optim import FusedAdamW
    gen = torch.Generator().manual_seed(5)
    p0 = [torch.randn(n, generator=gen) for n in OPT_SIZES]
    gss = [[torch.randn(n, generator=gen) * 4.0 for n in OPT_SIZES] for _ in range(2)]  # (carrying the scale 4)
    params = [torch.nn.Parameter(t.cuda()) for t in p0]
    opt = FusedAdamW(OPT._groups(params), lr=1.0, betas=OPT.BETAS, eps=OPT.EPS, max_grad_norm=OPT_NORM)
    tparams = [torch.nn.Parameter(t.cuda()) for t in p0]
    topt = torch.optim.AdamW(OPT._groups(tparams), lr=1.0, betas=OPT.BETAS, eps=OPT.EPS, foreach=True)
    ops64 = [t.double().cuda() for t in p0]
    oms, ovs = [torch.zeros_like(t) for t in ops64], [torch.zeros_like(t) for t in ops64]
    norms = []
    for step, grads in enumerate(gss, 1):
        OPT._set_grads(params, grads)
        opt.grad_scale, opt.found_inf = torch.full((), 4.0, device="cuda"), torch.zeros((), device="cuda")
        opt.step()
        norms.append(opt.last_grad_norm.clone())
        OPT._set_grads(tparams, [g / 4.0 for g in grads])
        torch.nn.utils.clip_grad_norm_(tparams, OPT_NORM)
        topt.step()
        g64 = [g.double().cuda() / 4.0 for g in grads]
        coef = min(1.0, OPT_NORM / (float(torch.cat(g64).norm()) + 1e-6))
        for i in range(3):
            grp = OPT.GROUPS[i % 2]
            ops64[i], oms[i], ovs[i] = OPT._oracle_step(ops64[i], g64[i] * coef, oms[i], ovs[i], step, grp["lr"], grp["weight_decay"])
    torch.cuda.synchronize()
    base = OPT._state(opt, params)
    theirs = OPT._state(topt, tparams)
    OPT._judge(f"3 tensors around a chunk, contiguous {lp}", base, theirs, (ops64, oms, ovs))
    for what, aligns in (("aligned", (0, 0, 0, 0, 0)), ("weak", (4, 8, 12, 4, 2))):
        state, cur = None, p0
        for k, grads in enumerate(gss):
            ps, ms, vs, p16, steps, out = _opt_raw(ops, cur, grads, aligns, state=state)
            assert GB.same_bits(out[:1], norms[k].reshape(1)), f"{what}: the clip norm of step {k + 1} differs"
            state, cur = (ms, vs, steps), [p.clone() for p in ps]
        assert all(float(s) == 2.0 for s in steps)
        for name, got, want in zip("pmv", (ps, ms, vs), base):
            for i in range(3):
                assert GB.same_bits(got[i], want[i]), f"{what}: {name}[{i}] differs from FusedAdamW's step"
        for i in range(3):  # test_16_bit_copies_equal_the_library_cast
            assert GB.same_bits(p16[i], ops.cast(ps[i].reshape(1, -1).contiguous(), LP()).reshape(-1)), f"{what}: p16[{i}]"
        OPT._judge(f"3 tensors around a chunk, {what} {lp}", (ps, ms, vs), theirs, (ops64, oms, ovs))
    # a found-inf step: nothing at all may change, the bands included (test_found_inf_leaves_every_buffer_untouched)
    before = [[t.clone() for t in group] for group in (ps, ms, vs, p16, steps)]
    ps2, ms2, vs2, p162, steps2, _ = _opt_raw(ops, [p.clone() for p in ps], gss[0], (4, 8, 12, 4, 2), found=1.0, state=(ms, vs, steps))
    for name, got, want in zip(("p", "m", "v", "step"), (ps2, ms2, vs2, steps2), (before[0], before[1], before[2], before[4])):
        for i in range(3):
            assert GB.same_bits(got[i], want[i]), f"found_inf: {name}[{i}] changed"
    assert all(bool((t == -7.0).all()) for t in p162), "found_inf: a 16-bit copy was written"


def test_optimizer_refuses_tables_it_cannot_take(ops):
    """include/cdseg.h: CDSEG_ERR_ARG for a NULL or not 4-byte aligned p / g / m / v / step, a 16-bit copy at an odd address,
    unknown flags, a group index outside the table, a chunk count that is not the table's, a chunk list or scalar that is not
    4-byte aligned, a workspace that is not 16-byte aligned, a negative max_norm, a bad hyper-parameter; CDSEG_ERR_WORKSPACE for a
    short or NULL workspace.  Every buffer keeps its fill."""
    lib = _lib.load()
    n = 100
    mem = TMem()
    bufs = {k: mem.vout(n, fill=-5.0, name=k) for k in "pgmv"}
    bufs["p16"], bufs["step"] = mem.vout(n, fill=-5.0, dtype=LP(), name="p16"), mem.vout(1, fill=-5.0, name="step")
    out = mem.vout(3, fill=-5.0, name="out")
    chunks = torch.zeros(2, dtype=torch.int32, device="cuda")
    need = lib.cdseg_opt_ws_bytes(1, 1)
    ws, wb = GB.exact_workspace(need)
    P, st, A, W = _p, ops._stream(), "CDSEG_ERR_ARG", "CDSEG_ERR_WORKSPACE"

    def call(which, entry=None, nch=1, ch=chunks, ws=ws, nb=need, max_norm=1.0, scale=None, lr=1e-3, out=out, **kw):
        table = (_lib.OptTensor * 1)()
        e = table[0]
        e.p, e.g, e.m, e.v, e.p16, e.step = (bufs[k].data_ptr() for k in ("p", "g", "m", "v", "p16", "step"))
        e.n, e.group, e.flags = n, 0, 1
        for k, val in (entry or {}).items():
            setattr(e, k, val)
        groups = (_lib.OptGroup * 1)()
        groups[0].lr, groups[0].beta1, groups[0].beta2, groups[0].eps, groups[0].weight_decay = lr, 0.9, 0.999, 1e-8, 0.0
        if which == "norm":
            return _err(lib.cdseg_grad_norm(table, 1, P(ch), nch, P(scale), max_norm, P(out), P(ws), nb, st))
        return _err(lib.cdseg_adamw_step(table, 1, groups, 1, P(ch), nch, P(scale), None, None, P(ws), nb, st))

    for which in ("norm", "step"):
        for k in ("p", "g", "m", "v", "step"):
            assert call(which, {k: bufs[k].data_ptr() + 2}) == A and call(which, {k: None}) == A, (which, k)
        assert call(which, {"p16": bufs["p16"].data_ptr() + 1}) == A and call(which, {"flags": 4}) == A and call(which, {"n": 0}) == A
        assert call(which, nch=2) == A and call(which, ch=chunks.data_ptr() + 2) == A and call(which, ch=None) == A, which
        assert call(which, ws=ws.data_ptr() + 8) == A and call(which, ws=None) == W and call(which, nb=need - 1) == W, which
        assert call(which, scale=out.data_ptr() + 2) == A, which
    assert call("norm", max_norm=-1.0) == A and call("norm", out=None) == A and call("norm", out=out.data_ptr() + 2) == A
    assert call("step", {"group": 1}) == A and call("step", lr=-1.0) == A
    mem.check()
    wb.check()
    assert all(bool((t == -5.0).all()) for t in list(bufs.values()) + [out]) and bool((ws == GB.WorkspaceBand.FILL).all())


# ====================================================================================================== train-time pipeline ops
TT_ALIGN = {torch.float32: 4, torch.int32: 4, torch.float64: 8, torch.int64: 8}


class TTMem(TMem):
    """Flat arrays between guard elements: layout "aligned" = 16-byte aligned bases, "weak" = element-aligned ones."""

    def __init__(self, layout):
        super().__init__()
        self.weak = layout == "weak"

    def _al(self, dtype):
        return TT_ALIGN[dtype] if self.weak else 0

    def arr_in(self, a, name):
        t = torch.as_tensor(np.ascontiguousarray(a)).cuda()
        return self.vin(t.reshape(-1), align=self._al(t.dtype), name=name)

    def arr_io(self, a, name):
        """an array the kernel updates in place: finite guards"""
        t = torch.as_tensor(np.ascontiguousarray(a)).cuda().reshape(-1)
        return self.vout(t.numel(), fill=-777.25, align=self._al(t.dtype), dtype=t.dtype, name=name, pre=t)

    def arr_out(self, numel, dtype, name):
        return self.vout(numel, fill=-777.25 if dtype.is_floating_point else -7, align=self._al(dtype), dtype=dtype, name=name)

    def idx(self, a):
        return self.index(torch.as_tensor(np.ascontiguousarray(a)).cuda())


def _tt_np(t, shape=None):
    a = t.cpu().numpy()
    return a if shape is None else a.reshape(shape)


def _tt_bbox(ops, mem, xk, is64, n):
    """cdseg_tt_bbox into a byte-exact guarded ws12 (12 x 8 bytes: three minima and maxima as ordered keys, then the six
    doubles) -> the (6,) float64 view [min, max], which later calls read as bbox6_dev."""
    ws, band = GB.exact_workspace(96)
    assert _lib.load().cdseg_tt_bbox(_p(xk), is64, n, _p(ws), ops._stream()) == 0
    torch.cuda.synchronize()
    band.check()
    return ws[48:].view(torch.float64)


@pytest.mark.parametrize("layout", ["aligned", "weak"])
@pytest.mark.parametrize("n", [1, 5, 257])
def test_tt_point_kernels_between_guard_elements(ops, n, layout):
    """cdseg_tt_bbox, cdseg_tt_affine (fp64 -> fp64 about the bbox centre, fp32 -> fp64 about a host centre, fp64 -> fp32 centre
    shift), cdseg_tt_jitter (fp64 and fp32 noise), cdseg_tt_color and cdseg_tt_dist_key: one thread per point or element in
    256-thread blocks (one point, five, a block plus one).  Host checks: NULL operands and ranges only.  Reference: the
    restatement of test_bbox_affine_jitter_and_colour_kernels_at_their_edges / test_sphere_crop_..., bit for bit."""
    lib, st, P = _lib.load(), ops._stream(), _p
    rng = np.random.default_rng(n)
    x32 = (rng.standard_normal((n, 3)) * 3 + 1).astype(np.float32)
    x64 = rng.standard_normal((n, 3)) * 3 - 2
    rot = tt.rotation_matrix("y", 0.37)
    r9 = (ctypes.c_double * 9)(*[float(v) for row in rot for v in row])
    c3 = (ctypes.c_double * 3)(0.5, -1.0, 2.0)
    mem = TTMem(layout)
    k32, k64 = mem.arr_in(x32, "xyz32"), mem.arr_in(x64, "xyz64")
    for x, xk, is64 in ((x32, k32, 0), (x64, k64, 1)):
        assert np.array_equal(_tt_np(ops.tt_bbox(torch.as_tensor(x).cuda())), R.bbox(x))
        bb = _tt_bbox(ops, mem, xk, is64, n)
        assert np.array_equal(_tt_np(bb), R.bbox(x))
    # affine (bb: the fp64 cloud's box)
    out = mem.arr_out(3 * n, torch.float64, "affine out")
    assert lib.cdseg_tt_affine(P(k64), 1, n, ops.TT_CENTER_BBOX, None, P(bb), r9, 1, 1.07, 1, 1, 0, P(out), 1, st) == 0
    mem.check()
    assert np.array_equal(TT._bits(_tt_np(out, (n, 3))), TT._bits(R.flip(R.rotate(x64, rot, "bbox") * 1.07, True, False)))
    out = mem.arr_out(3 * n, torch.float64, "affine out")
    assert lib.cdseg_tt_affine(P(k32), 0, n, ops.TT_CENTER_HOST, c3, None, r9, 1, 1.0, 0, 0, 1, P(out), 1, st) == 0
    mem.check()
    assert np.array_equal(TT._bits(_tt_np(out, (n, 3))), TT._bits(R.flip(R.rotate(x32.astype(np.float64), rot, [0.5, -1.0, 2.0]), False, True)))
    for apply_z, mode in ((True, ops.TT_CENTER_SHIFT_Z), (False, ops.TT_CENTER_SHIFT_XY)):
        out = mem.arr_out(3 * n, torch.float32, "affine out32")
        assert lib.cdseg_tt_affine(P(k64), 1, n, mode, None, P(bb), None, 0, 1.0, 0, 0, 0, P(out), 0, st) == 0
        mem.check()
        assert np.array_equal(TT._bits(_tt_np(out, (n, 3))), TT._bits(R.center_shift(x64, apply_z).astype(np.float32)))
    # jitter, in place
    z = rng.standard_normal((n, 3)) * 4
    for zz in (z, z.astype(np.float32)):
        co = mem.arr_io(x64, "coord")
        assert lib.cdseg_tt_jitter(P(co), P(mem.arr_in(zz, "z")), int(zz.dtype == np.float64), 0.005, 0.02, n, st) == 0
        mem.check()
        assert np.array_equal(TT._bits(_tt_np(co, (n, 3))), TT._bits(R.jitter(x64, zz, 0.005, 0.02)))
    # colour chain, in place (a single colour has hi == lo: no contrast stage, as in the existing test)
    col = rng.integers(0, 256, (n, 3)).astype(np.float32)
    tr = (ctypes.c_double * 3)(3.0, -200.0, 250.0)
    if n > 1:
        cd = mem.arr_io(col, "color")
        cbb = _tt_bbox(ops, mem, cd, 0, n)
        assert lib.cdseg_tt_color(P(cd), n, P(cbb), 0.3, 1, tr, P(mem.arr_in(z, "noise")), 1, 0.05 * 255, st) == 0
        mem.check()
        want = R.color_chain(R.color_chain(R.color_chain(col, blend=0.3), tr=[3.0, -200.0, 250.0]), noise=z, noise_mul=0.05 * 255)
        assert np.array_equal(TT._bits(_tt_np(cd, (n, 3))), TT._bits(want))
    cd = mem.arr_io(col, "color")
    assert lib.cdseg_tt_color(P(cd), n, None, 0.0, 0, tr, P(mem.arr_in(z.astype(np.float32), "noise32")), 0, 2.0, st) == 0
    mem.check()
    want = R.color_chain(R.color_chain(col, tr=[3.0, -200.0, 250.0]), noise=z.astype(np.float32), noise_mul=2.0)
    assert np.array_equal(TT._bits(_tt_np(cd, (n, 3))), TT._bits(want))
    # distance keys
    key = mem.arr_out(n, torch.int64, "key")
    assert lib.cdseg_tt_dist_key(P(k64), n, n // 2, P(key), st) == 0
    mem.check()
    assert np.array_equal(_tt_np(key), TT._bits(R.sphere_crop(x64, n // 2, n)[1]))
    assert np.array_equal(_tt_np(ops.tt_dist_key(torch.as_tensor(x64).cuda(), n // 2)), _tt_np(key))


@pytest.mark.parametrize("layout", ["aligned", "weak"])
@pytest.mark.parametrize("n", [1, 5, 257])
def test_tt_elastic_and_blur_between_guard_elements(ops, n, layout):
    """cdseg_tt_blur3 on a (2, 3, 4) grid along each axis (the reference's six passes x, y, z, x, y, z, every pass from one
    guarded buffer into another) and cdseg_tt_elastic on n points with the corners, a point just outside and one on interior
    grid lines.  Reference: R.blur / R.elastic_interp of test_elastic_blur_and_trilinear_apply, bit for bit."""
    lib, st, P = _lib.load(), ops._stream(), _p
    dims = (2, 3, 4)
    rng = np.random.default_rng(n)
    noise = rng.standard_normal(dims + (3,)).astype(np.float32)
    blurred = R.blur(noise)
    assert np.array_equal(TT._bits(_tt_np(ops.tt_blur(torch.as_tensor(noise).cuda()))), TT._bits(blurred))
    mem = TTMem(layout)
    src = mem.arr_in(noise, "noise")
    for k in range(6):
        dst = mem.arr_out(noise.size, torch.float32, f"blur pass {k}")
        assert lib.cdseg_tt_blur3(P(src), *dims, k % 3, P(dst), st) == 0
        mem.check()
        src = dst
    assert np.array_equal(TT._bits(_tt_np(src, dims + (3,))), TT._bits(blurred))
    g = 0.2
    start = np.array([1.0, -2.0, 0.25]) - g
    dim = np.array(dims)
    stop = start + g * (dim - 1)
    step = (stop - start) / (dim - 1)
    pts = start + rng.random((n, 3)) * (stop - start)
    special = [start, stop, stop + [1e-9, 0.0, 0.0], start - [0.0, 0.0, 0.5], start + step * [1, 2, 1]]
    for i, v in enumerate(special[:n]):
        pts[n - 1 - i] = v
    want = R.elastic_interp(pts, blurred, start, step, stop, 1.6)
    co = mem.arr_io(pts, "coord")
    d3 = lambda v: (ctypes.c_double * 3)(*[float(e) for e in v])  # noqa: E731
    assert lib.cdseg_tt_elastic(P(co), n, P(src), (ctypes.c_int * 3)(*dims), d3(start), d3(step), d3(stop), 1.6, st) == 0
    mem.check()
    assert np.array_equal(TT._bits(_tt_np(co, (n, 3))), TT._bits(want))


@pytest.mark.parametrize("layout", ["aligned", "weak"])
@pytest.mark.parametrize("n", [1, 5, 257])
def test_tt_voxel_pick_and_rand_int_between_guard_elements(ops, n, layout):
    """cdseg_tt_voxel_pick on the voxels of n points (idx_sort, seg_start and r between edge copies, the picks between guard
    elements) against R.grid_sample as in test_voxel_pick_...; cdseg_rand_int at n = 1, 5, 257 - none a multiple of the four
    words a thread draws, so the last thread stores 1 word of 4 (`4 * t + i < n`) - raw, modulo a host bound and modulo a
    guarded device bound, against the Philox stream of test_rand_int_is_the_philox_stream_of_randn."""
    lib, st, P = _lib.load(), ops._stream(), _p
    rng = np.random.default_rng(n)
    coord = rng.random((n, 3)) * [0.4, 0.2, 0.1]
    c = torch.as_tensor(coord).cuda()
    grid, key, _ = ops.voxelize_any(c, 0.05)
    key_sorted, idx_sort = ops.sort_pairs(key, None, end_bit=63)
    _, seg_start, count = ops.pool_level(key_sorted, 0)
    m = int(count.item())
    r = rng.integers(0, 50, m)
    want = R.grid_sample(coord, 0.05, r)
    assert m == len(want["count"])
    assert np.array_equal(_tt_np(ops.tt_voxel_pick(idx_sort, seg_start, m, torch.as_tensor(r).cuda())), want["pick"])
    mem = TTMem(layout)
    pick = mem.arr_out(m, torch.int32, "pick")
    assert lib.cdseg_tt_voxel_pick(P(mem.index(idx_sort)), P(mem.index(seg_start[:m + 1].contiguous())), m, P(mem.idx(r)), P(pick), st) == 0
    mem.check()
    assert np.array_equal(_tt_np(pick), want["pick"])
    # rand_int
    seed, offset = 0x1234567811223344, 0x9_0000_0007
    nt = (n + 3) // 4
    t = np.arange(nt, dtype=np.uint64)
    ctr = np.stack([(t & np.uint64(0xFFFFFFFF)).astype(np.uint32), (t >> np.uint64(32)).astype(np.uint32),
                    np.full(nt, offset & 0xFFFFFFFF, dtype=np.uint32), np.full(nt, offset >> 32, dtype=np.uint32)], -1)
    pk = np.stack([np.full(nt, seed & 0xFFFFFFFF, dtype=np.uint32), np.full(nt, seed >> 32, dtype=np.uint32)], -1)
    words = philox.philox4x32_10(ctr, pk).reshape(-1)[:n].astype(np.int64)
    assert n % 4 != 0 and np.array_equal(_tt_np(ops.rand_int(n, seed, offset, "cuda")), words)
    bd = mem.idx(np.array([1000003], dtype=np.int32))
    for bound_dev, bound, wantw in ((None, 0, words), (None, 37, words % 37), (bd, 0, words % 1000003)):
        out = mem.arr_out(n, torch.int64, "out")
        assert lib.cdseg_rand_int(P(out), n, seed, offset, P(bound_dev), bound, st) == 0
        mem.check()
        assert np.array_equal(_tt_np(out), wantw)


def test_tt_entry_points_refuse_what_they_cannot_take(ops):
    """csrc/traintime.hip's host checks, through the return code with the outputs keeping their fill: NULL operands; tt_bbox
    n <= 0; tt_affine a centre mode outside the enum, a host centre or a bbox that the mode needs and is not there; tt_jitter a
    clip that is not positive; tt_blur3 in == out, an axis outside 0 .. 2, an empty grid; tt_elastic a grid side below 2, a step
    that is not positive, stop <= start; tt_color contrast without a bbox; tt_dist_key a centre outside the rows.  (n <= 0 is
    CDSEG_OK with nothing written everywhere but tt_bbox.)"""
    lib, st, P, A = _lib.load(), ops._stream(), _p, "CDSEG_ERR_ARG"
    n = 5
    mem = TTMem("aligned")
    x64, x32 = mem.arr_in(np.ones((n, 3)), "x64"), mem.arr_in(np.ones((n, 3), dtype=np.float32), "x32")
    o64, o32 = mem.arr_out(3 * n, torch.float64, "out64"), mem.arr_out(24 * 3, torch.float32, "out32")
    i64, i32 = mem.arr_out(n, torch.int64, "int64 out"), mem.arr_out(n, torch.int32, "int32 out")
    idx = torch.arange(n + 1, dtype=torch.int32, device="cuda")
    r64 = torch.zeros(n, dtype=torch.int64, device="cuda")
    ws, wb = GB.exact_workspace(96)
    bb = torch.zeros(6, dtype=torch.float64, device="cuda")
    d3 = lambda *v: (ctypes.c_double * 3)(*v)  # noqa: E731
    dims = lambda *v: (ctypes.c_int * 3)(*v)  # noqa: E731
    E = lambda rc: _err(rc)  # noqa: E731
    assert E(lib.cdseg_tt_bbox(P(x64), 1, 0, P(ws), st)) == A and E(lib.cdseg_tt_bbox(None, 1, n, P(ws), st)) == A
    assert E(lib.cdseg_tt_bbox(P(x64), 1, n, None, st)) == A

    def aff(inp=x64, center=0, c3=None, bbox=None, out=o64, n=n):
        return E(lib.cdseg_tt_affine(P(inp), 1, n, center, c3, P(bbox), None, 0, 1.0, 0, 0, 0, P(out), 1, st))

    assert aff(inp=None) == A and aff(out=None) == A and aff(center=5) == A and aff(center=-1) == A
    assert aff(center=ops.TT_CENTER_HOST) == A and aff(center=ops.TT_CENTER_BBOX) == A and aff(center=ops.TT_CENTER_SHIFT_XY) == A
    assert aff(n=0) == 0
    jit = lambda co=o64, z=x64, clip=0.02, n=n: E(lib.cdseg_tt_jitter(P(co), P(z), 1, 0.005, clip, n, st))  # noqa: E731
    assert jit(co=None) == A and jit(z=None) == A and jit(clip=0.0) == A and jit(clip=-1.0) == A and jit(n=0) == 0
    blur = lambda i=x32, o=o32, d=(2, 3, 4), ax=0: E(lib.cdseg_tt_blur3(P(i), *d, ax, P(o), st))  # noqa: E731
    assert blur(i=None) == A and blur(o=None) == A and blur(i=o32) == A and blur(ax=3) == A and blur(ax=-1) == A and blur(d=(0, 3, 4)) == A

    def ela(co=o64, noise=x32, d=dims(2, 2, 2), start=d3(0, 0, 0), step=d3(1, 1, 1), stop=d3(1, 1, 1), n=n):
        return E(lib.cdseg_tt_elastic(P(co), n, P(noise), d, start, step, stop, 1.0, st))

    assert ela(co=None) == A and ela(noise=None) == A and ela(d=None) == A and ela(start=None) == A and ela(step=None) == A
    assert ela(stop=None) == A and ela(d=dims(1, 2, 2)) == A and ela(step=d3(0, 1, 1)) == A and ela(stop=d3(0, 1, 1)) == A and ela(n=0) == 0
    col = lambda c=o32, bbox=None, contrast=0, n=n: E(lib.cdseg_tt_color(P(c), n, P(bbox), 0.3, contrast, None, None, 0, 0.0, st))  # noqa: E731
    assert col(c=None) == A and col(contrast=1) == A and col(n=0) == 0

    def vp(a=idx, s=idx, r=r64, o=i32, m=n):
        return E(lib.cdseg_tt_voxel_pick(P(a), P(s), m, P(r), P(o), st))

    assert vp(a=None) == A and vp(s=None) == A and vp(r=None) == A and vp(o=None) == A and vp(m=0) == 0
    dk = lambda c=x64, center=0, k=i64, n=n: E(lib.cdseg_tt_dist_key(P(c), n, center, P(k), st))  # noqa: E731
    assert dk(c=None) == A and dk(k=None) == A and dk(center=-1) == A and dk(center=n) == A and dk(n=0) == 0
    assert E(lib.cdseg_rand_int(None, n, 1, 2, None, 0, st)) == A and E(lib.cdseg_rand_int(P(i64), 0, 1, 2, None, 0, st)) == 0
    mem.check()
    wb.check()
    assert all(bool((o == -777.25).all()) for o in (o64, o32)) and bool((i64 == -7).all()) and bool((i32 == -7).all())
    assert bool((ws == GB.WorkspaceBand.FILL).all()) and bool((bb == 0).all())
    assert aff(center=ops.TT_CENTER_SHIFT_Z, bbox=bb) == 0 and dk() == 0  # the same operands with nothing wrong run
    mem.check()
    assert _finite(o64) and not bool((i64 == -7).any())
