"""GPU: the CPU emulations of the op layer (tests/emu_*.py) held to the kernels they stand in for.

The CPU half of the suite swaps `cdsegnet_amd.ops` for the emulations, so what it proves about host logic, autograd wiring and
the multi-GPU path holds only as far as an emulation computes what its kernel computes.  Here every public function of the
seven emulation modules has a case (CASES, keyed by op name; `test_every_emulated_op_has_a_case` fails for one without): small
seeded inputs are built once on the CPU, the emulation runs on them, the real op on device copies, and EVERY output is
compared - return values and every caller-owned buffer the op may write, whole buffers from the same non-zero pre-fill, so
that overwrite and accumulate, and the rows no index addresses, can be told apart.

  * integer / index / boolean results: bit-equal (`same`); a region include/cdseg.h leaves undefined is named by the case,
    left out of the comparison, and must hold the emulation's poison (tests/emu_ops.py _POISON);
  * float results: both sides against an fp64 evaluation R of the op on the same (16-bit: rounded) inputs, |hip - R| <= B and
    |emu - R| <= B (`within`), B taken from the GPU test of that op (named next to the case) or derived as
    k * eps * sum |terms| in fp64, k = the roundings of the longer of the two evaluations (derivation next to the case);
    every comparison prints a [measure] line with both errors and |hip - emu|;
  * ops whose contract is bit equality with torch stay bit-equal (cast without saturation, row gathers / scatters, residual);
  * sentinel (-1) entries where the contract gives them a meaning, planted exact ties where it gives a tie rule;
  * steering predicates over the width x dtype (x rows) grid; opaque weight images through the op that consumes them.

profiles/emu_conformance_measured.txt holds the [measure] lines of one run."""
import importlib
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import model as OM
from oracle import serialization as S
from tests.helpers import load_fixture
from tests.test_cpu_emu_signatures import EMU_MODULES, emulated_functions
from tests.test_gpu_ops import LP, _library_variant, ops  # noqa: F401  (fixtures: lp="f16" -> the half build)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24        # unit roundoff of fp32
U64 = 2.0 ** -53      # ... of fp64
LP_DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}

# no tensor result and no tensor side effect: nothing to compare
EXEMPT = {
    "bind_stream": "binds the calling thread's stream; the emulation has none",
    "unbind_stream": "as bind_stream",
    "current_stream_id": "identity of the bound stream",
    "record_event": "returns a stream event",
    "wait_event": "waits for a stream event",
    "is_lp": "a predicate on a dtype (covered with the steering predicates' grid, no device work)",
    "train_block_bytes": "host arithmetic on a device descriptor: the emulation sizes nothing it allocates from it",
}

EMU_OF = {}  # op name -> the emulation function (the module that defines it)
for _m in EMU_MODULES:
    for _name, _fn in emulated_functions(_m).items():
        EMU_OF[_name] = _fn
POISON = importlib.import_module("tests.emu_ops")._POISON

CASES = {}  # op name -> [(case function, takes the 16-bit type)]


def case(*names, lp=False):
    def deco(fn):
        for name in names:
            CASES.setdefault(name, []).append((fn, lp))
        return fn
    return deco


# ------------------------------------------------------------------------------------------ the two sides of a call
def _map(v, f):
    if isinstance(v, torch.Tensor):
        return f(v)
    if isinstance(v, (list, tuple)):
        return type(v)(_map(e, f) for e in v)
    if isinstance(v, dict):
        return {k: _map(e, f) for k, e in v.items()}
    return v


def to_dev(v):
    return _map(v, lambda t: t.detach().clone().cuda())


def to_cpu(v):
    return _map(v, lambda t: t.detach().cpu())


class Res:
    """Both sides of one call: e / h = what the emulation / the kernel returned, ea / ha (ek / hk) = the positional (keyword)
    arguments after the call, the device ones copied back."""

    def __init__(self, e, h, ea, ha, ek, hk):
        self.e, self.h, self.ea, self.ha, self.ek, self.hk = e, h, ea, ha, ek, hk


def hip_call(ops, name, args, kw):
    """The real op on device copies of the arguments -> (result, positional, keyword arguments), all copied back."""
    ha, hk = to_dev(args), to_dev(kw)
    h = getattr(ops, name)(*ha, **hk)
    torch.cuda.synchronize()
    return to_cpu(h), to_cpu(ha), to_cpu(hk)


class K:
    """What a case works with: the two op layers, the 16-bit type of the build under test, the comparisons."""

    def __init__(self, ops, lp, name):
        self.ops, self.lp, self.T, self.name, self.compared = ops, lp, LP_DTYPES[lp], name, 0  # compared: comparisons made so far

    def call(self, name, *args, **kw):
        ea, ek = _map(args, lambda t: t.detach().clone()), _map(kw, lambda t: t.detach().clone())
        e = EMU_OF[name](*ea, **ek)
        h, ha, hk = hip_call(self.ops, name, args, kw)
        return Res(e, h, ea, ha, ek, hk)

    def same(self, what, e, h):
        """Bit equality of two results of any nesting (dtype and shape included)."""
        if isinstance(e, torch.Tensor) or isinstance(h, torch.Tensor):
            assert isinstance(e, torch.Tensor) and isinstance(h, torch.Tensor), (self.name, what, type(e), type(h))
            assert e.dtype == h.dtype and tuple(e.shape) == tuple(h.shape), (self.name, what, e.dtype, h.dtype, e.shape, h.shape)
            ok = torch.equal(e, h) if not e.is_floating_point() else bool(((e == h) | (e.isnan() & h.isnan())).all())
            bad = 0 if ok else int((e != h).sum())
            print(f"[measure] emu-conformance {self.name}[{self.lp}] {what}: bit-equal={int(ok)} of {e.numel()} (differing {bad})")
            assert ok, (self.name, what, f"{bad} of {e.numel()} elements differ")
            self.compared += 1
        elif isinstance(e, (list, tuple)):
            assert isinstance(h, (list, tuple)) and len(e) == len(h), (self.name, what)
            for i, (a, b) in enumerate(zip(e, h)):
                self.same(f"{what}[{i}]", a, b)
        else:
            assert e == h, (self.name, what, e, h)
            self.compared += 1

    def within(self, what, e, h, R, B, src):
        """|hip - R| <= B and |emu - R| <= B, element by element (B a number or a tensor), R in fp64 (or better)."""
        assert e.dtype == h.dtype and tuple(e.shape) == tuple(h.shape) == tuple(R.shape), (self.name, what, e.dtype, h.dtype, e.shape, h.shape, R.shape)
        R = R.double()
        assert bool(torch.isfinite(h.double()).all()) and bool(torch.isfinite(e.double()).all()), (self.name, what)
        eh, ee, d = (h.double() - R).abs(), (e.double() - R).abs(), (h.double() - e.double()).abs()
        Bt = torch.as_tensor(B, dtype=torch.float64).expand(R.shape) if R.numel() else torch.zeros(R.shape, dtype=torch.float64)
        used_h = float((eh / Bt.clamp_min(1e-300)).max()) if R.numel() else 0.0
        used_e = float((ee / Bt.clamp_min(1e-300)).max()) if R.numel() else 0.0
        mx = (lambda t: float(t.max()) if t.numel() else 0.0)
        print(f"[measure] emu-conformance {self.name}[{self.lp}] {what}: |hip-R|={mx(eh):.3e} |emu-R|={mx(ee):.3e} |hip-emu|={mx(d):.3e} "
              f"bound={mx(Bt):.3e} used hip={used_h:.3f} emu={used_e:.3f} ({src})")
        assert used_h <= 1.0, (self.name, what, "hip", mx(eh), mx(Bt), used_h)
        assert used_e <= 1.0, (self.name, what, "emu", mx(ee), mx(Bt), used_e)
        self.compared += 1

    def r16(self, x):
        """fp32 values rounded to the build's 16-bit type (still fp32)."""
        return x.to(self.T).float()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def three_times_torch(t32, R):
    """The rule of tests/test_gpu_train_fp32.py (_assert_vs_torch): max |g - R| <= (3 E_torch + 2^-24) max |R|, E_torch the
    error of torch's fp32 evaluation by the same metric."""
    top = float(R.abs().max())
    return (3.0 * float((t32.double() - R).abs().max()) / top + U) * top


def ulp32(mag):
    """One fp32 unit in the last place at magnitude `mag` (tests/test_gpu_fusion.py / test_gpu_skip.py `_ulp`)."""
    return torch.exp2(torch.floor(torch.log2(mag.double().clamp(min=2.0 ** -126))) - 23.0)


ROWS = (1, 65, 257)


# ------------------------------------------------------------------------------------------ the enumeration
def test_every_emulated_op_has_a_case():
    """Every public function an emulation module defines has a case here, or is one of the named exemptions (no tensor result,
    no tensor side effect)."""
    names = set(EMU_OF)
    assert len(names) >= 100 and set(EXEMPT) <= names
    missing = sorted(names - set(CASES) - set(EXEMPT))
    assert not missing, f"emulated ops without a conformance case: {missing}"
    assert not set(CASES) & set(EXEMPT) and not set(CASES) - names, sorted(set(CASES) - names)


# ------------------------------------------------------------------------------------------ plan state (integer ops)
_CLOUDS = {}
CLOUDS = ("tiny64", "batch2")


def cloud(name):
    """The plan of a golden cloud built ONCE with the emulated ops on the CPU: what every integer case takes its inputs from
    (each op is then run on both sides on the same CPU-built inputs, never on the other side's output)."""
    if name in _CLOUDS:
        return _CLOUDS[name]
    E = types.SimpleNamespace(**EMU_OF)
    fx = load_fixture(f"serialization_{name}.npz")
    grid, batch, offset = (torch.as_tensor(fx[k]) for k in ("grid_coord", "batch", "offset"))
    depth, n, nb = int(fx["depth"]), grid.shape[0], int(offset.numel())
    zc = E.encode(grid, batch, depth, "z")
    zs, perm0 = E.sort_pairs(zc)
    g0, b0 = E.plan_gather_grid(grid, perm0, zs, depth)
    code4 = E.encode4(g0, b0, depth)
    cl1, seg1, cnt1 = E.pool_level(zs, 3)
    m1 = int(cnt1)
    cl2, seg2, cnt2 = E.pool_level(zs, 6)
    m2 = int(cnt2)
    g1, b1, c41 = E.pool_gather(seg1, m1, n, 1, g0, b0, code4)
    pn3 = E.nbr_table(c41[0].contiguous(), g1, b1, depth - 1, 3, True)
    cinfo = E.child_info(zs, seg1, m1)
    offs = torch.cat([torch.zeros(1, dtype=torch.int64), offset]).int()
    end_bit = 3 * depth + max(1, nb.bit_length())
    orders0 = [E.sort_pairs(code4[c].contiguous(), None, end_bit)[1] for c in (1, 2, 3)]
    _CLOUDS[name] = types.SimpleNamespace(grid=grid, batch=batch, offset=offset, depth=depth, n=n, nb=nb, zc=zc, zs=zs, perm0=perm0,
                                          g0=g0, b0=b0, code4=code4, cl1=cl1, seg1=seg1, m1=m1, cl2=cl2, seg2=seg2, m2=m2, g1=g1, b1=b1,
                                          c41=c41, pn3=pn3, cinfo=cinfo, offs=offs, end_bit=end_bit, orders0=orders0)
    return _CLOUDS[name]


@case("grid_max", "offset2batch", "encode", "encode4", "widen")
def case_serialization(k):
    for name in CLOUDS:
        c = cloud(name)
        r = k.call("grid_max", c.grid)
        k.same(f"grid_max {name}", r.e, r.h)
        r = k.call("grid_max", c.grid.int())
        k.same(f"grid_max int32 {name}", r.e, r.h)
        r = k.call("offset2batch", c.offset, c.n)
        k.same(f"offset2batch {name}", r.e, r.h)
        assert torch.equal(r.h.long(), c.batch)
        for o, oname in enumerate(S.ORDERS):
            for g, b in ((c.grid, c.batch), (c.grid.int(), c.batch.int()), (c.grid, None)):
                r = k.call("encode", g, b, c.depth, oname if o % 2 else o)  # (by name and by id)
                k.same(f"encode {name} {oname} {g.dtype} batch={b is not None}", r.e, r.h)
        r = k.call("encode4", c.g0, c.b0, c.depth)
        k.same(f"encode4 {name}", r.e, r.h)
        r = k.call("widen", c.perm0)
        k.same(f"widen {name}", r.e, r.h)


@case("sort_pairs", "sort_curves", "invert_perm")
def case_sorts(k):
    """Stable order: keys with their low bits cut off tie in long runs; the payload keeps the input order inside a run."""
    for name in CLOUDS:
        c = cloud(name)
        r = k.call("sort_pairs", c.zc)
        k.same(f"sort_pairs {name}", r.e, r.h)
        tied = (c.code4[2] % 7).contiguous()  # seven distinct keys: long runs of ties
        vals = torch.randperm(c.n, generator=gen(c.n)).int()
        for kw in (dict(), dict(end_bit=c.end_bit)):
            r = k.call("sort_pairs", tied, vals, **kw)
            k.same(f"sort_pairs ties+payload {name} {kw}", r.e, r.h)
        ks, perm = r.h
        run = ks[1:] == ks[:-1]
        pos = torch.empty(c.n, dtype=torch.long)
        pos[vals.long()] = torch.arange(c.n)
        assert bool((pos[perm.long()][1:][run] > pos[perm.long()][:-1][run]).all()), "a tie is not in input order"
        for rows in ([1, 2, 3], [0], [3, 1], []):
            r = k.call("sort_curves", c.code4, rows, c.end_bit)
            k.same(f"sort_curves {name} rows={rows}", r.e, r.h)
        r = k.call("invert_perm", c.perm0)
        k.same(f"invert_perm {name}", r.e, r.h)


@case("plan_gather_grid", "pool_level", "pool_levels", "pool_gather", "link_derive", "coarse_orders", "child_info")
def case_pooling_structure(k):
    for name in CLOUDS:
        c = cloud(name)
        for g in (c.grid, c.grid.int()):
            r = k.call("plan_gather_grid", g, c.perm0, c.zs, c.depth)
            k.same(f"plan_gather_grid {name} {g.dtype}", r.e, r.h)
        for shift, m in ((3, c.m1), (6, c.m2)):
            # count_out: the caller's counter, pre-filled; seg_start behind count + 1 entries is undefined (include/cdseg.h:
            # "seg_start (count+1 entries)") - compared up to there, and the emulation poisons the rest
            r = k.call("pool_level", c.zs, shift, torch.full((1,), 77, dtype=torch.int32))
            (ecl, eseg, ecnt), (hcl, hseg, hcnt) = r.e, r.h
            assert int(ecnt) == int(hcnt) == m
            k.same(f"pool_level {name} >>{shift} cluster", ecl, hcl)
            k.same(f"pool_level {name} >>{shift} seg_start[:m+1]", eseg[:m + 1], hseg[:m + 1])
            k.same(f"pool_level {name} >>{shift} count / count_out", [ecnt, r.ea[2]], [hcnt, r.ha[2]])
            assert eseg.shape == hseg.shape and bool((eseg[m + 1:] == POISON).all()), "the emulation does not poison seg_start's tail"
        last = (c.offs[1:] - 1).int()
        r = k.call("pool_levels", c.zs, [3, 6], last)
        (ecl, eseg, emeta), (hcl, hseg, hmeta) = r.e, r.h
        k.same(f"pool_levels {name} cluster / meta", [ecl, emeta], [hcl, hmeta])
        for lv, m in enumerate((c.m1, c.m2)):
            k.same(f"pool_levels {name} seg_start[{lv}][:m+1]", eseg[lv, :m + 1], hseg[lv, :m + 1])
            assert bool((eseg[lv, m + 1:] == POISON).all())
        r = k.call("pool_gather", c.seg1, c.m1, c.n, 1, c.g0, c.b0, c.code4)
        k.same(f"pool_gather {name}", r.e, r.h)
        r = k.call("link_derive", c.cl1, c.seg1, c.m1, c.cl2, c.seg2, c.m2)
        k.same(f"link_derive {name}", r.e, r.h)
        r = k.call("coarse_orders", [c.cl1, c.cl2], c.orders0, [c.m1, c.m2])
        k.same(f"coarse_orders {name}", [list(x) for x in r.e], [list(x) for x in r.h])
        r = k.call("child_info", c.zs, c.seg1, c.m1)
        k.same(f"child_info {name}", r.e, r.h)


@case("nbr_table", "nbr_table_from_parent", "nbr_table_from_info")
def case_kernel_maps(k):
    for name in CLOUDS:
        c = cloud(name)
        for ksize in (3, 5):
            for kmajor in (False, True):
                r = k.call("nbr_table", c.zs, c.g0, c.b0, c.depth, ksize, kmajor)
                k.same(f"nbr_table {name} k={ksize} kmajor={kmajor}", r.e, r.h)
                assert bool((r.h < 0).any())  # (the -1 entries every consumer below meets)
                r = k.call("nbr_table_from_parent", c.zs, c.g0, c.cl1, c.pn3, c.seg1, c.m1, c.depth, ksize, kmajor)
                k.same(f"nbr_table_from_parent {name} k={ksize} kmajor={kmajor}", r.e, r.h)
                r = k.call("nbr_table_from_info", c.g0, c.cl1, c.pn3, c.cinfo, c.m1, c.depth, ksize, kmajor)
                k.same(f"nbr_table_from_info {name} k={ksize} kmajor={kmajor}", r.e, r.h)


def _pad(c, patch):
    counts = (c.offs[1:] - c.offs[:-1]).long()
    pc = torch.where(counts > patch, (counts + patch - 1) // patch * patch, counts)
    offs_pad = torch.cat([torch.zeros(1, dtype=torch.long), pc.cumsum(0)]).int()
    return offs_pad, int(offs_pad[-1])


@case("pad_plan", "pad_plan_batch", "slots_select")
def case_slot_plans(k):
    for name in CLOUDS:
        c = cloud(name)
        plans = []
        for patch in (4, 16, 1024):
            offs_pad, n_pad = _pad(c, patch)
            for order in (None, c.orders0[1]):
                r = k.call("pad_plan", order, c.offs, offs_pad, patch, n_pad)
                k.same(f"pad_plan {name} K={patch} order={order is not None}", r.e, r.h)
                plans.append((order, c.offs, offs_pad, patch, n_pad))
                if patch == 16 and name == "batch2":
                    assert bool((r.h[1] < 0).any())  # borrowed duplicates: the -1 write rows attention skips
        r = k.call("pad_plan_batch", plans, c.nb)
        k.same(f"pad_plan_batch {name}", [list(x) for x in r.e], [list(x) for x in r.h])
        offs_pad, n_pad = _pad(c, 16)
        src = [EMU_OF["pad_plan"](o, c.offs, offs_pad, 16, n_pad) for o in (None, c.orders0[0], c.orders0[2])]
        for choice, sources in (([0] * c.nb, src), ([2, 1][:c.nb], src), ([2] * c.nb, [None, None, src[2]])):
            r = k.call("slots_select", sources, offs_pad, choice, n_pad)
            k.same(f"slots_select {name} choice={choice}", r.e, r.h)


# ------------------------------------------------------------------------------------------ row moves, casts (bit-equal)
@case("gather_rows", "scatter_rows", "gather_i32", "gather_pad_cast", "cast", lp=True)
def case_row_moves(k):
    g = gen(5)
    for dtype, c in ((torch.float32, 8), (torch.float32, 3), (k.T, 6)):
        src = torch.randn(257, c, generator=g).to(dtype)
        idx = torch.randint(0, 257, (65,), generator=g).int()
        idx[[0, 7, 64]] = -1
        r = k.call("gather_rows", src, idx)
        k.same(f"gather_rows {dtype} c={c}", r.e, r.h)
        assert bool((r.h[idx < 0] == 0).all()) and bool((r.e[idx < 0] == 0).all())  # idx < 0: a zero row
        # scatter: distinct target rows, -1 = the row is skipped; the other rows of `out` keep the pre-fill
        tgt = torch.randperm(257, generator=g)[:65].int()
        tgt[[3, 30]] = -1
        pre = torch.randn(257, c, generator=g).to(dtype) + 5
        r = k.call("scatter_rows", src[:65].contiguous(), tgt, pre)
        k.same(f"scatter_rows {dtype} c={c} (whole out)", r.ea[2], r.ha[2])
        k.same(f"scatter_rows {dtype} c={c} (result)", r.e, r.h)
        untouched = torch.ones(257, dtype=torch.bool)
        untouched[tgt[tgt >= 0].long()] = False
        assert torch.equal(r.ha[2][untouched], pre[untouched]) and torch.equal(r.ea[2][untouched], pre[untouched])
    src = torch.randint(-5, 1000, (257,), generator=g).int()
    r = k.call("gather_i32", src, torch.randint(0, 257, (65,), generator=g).int())  # (no sentinel: every entry names a row)
    k.same("gather_i32", r.e, r.h)
    feat = torch.randn(100, 6, generator=g)
    for idx in (None, torch.randint(0, 100, (65,), generator=g).int()):
        for dtype in (k.T, torch.float32):
            r = k.call("gather_pad_cast", feat, idx, 8, dtype)
            k.same(f"gather_pad_cast idx={idx is not None} {dtype}", r.e, r.h)
    # cast without saturation: in-range values (the half build's cast clamps beyond +-65504, torch's gives inf)
    x = torch.cat([torch.randn(1000, generator=g) * 100, torch.tensor([0.0, -0.0, 1e-8, 65504.0, -65504.0, 1.0009765625, 3.0e4])]).reshape(-1, 1)
    r = k.call("cast", x, k.T)
    k.same("cast fp32 -> 16 bit", r.e, r.h)
    r = k.call("cast", x.to(k.T), torch.float32)
    k.same("cast 16 bit -> fp32", r.e, r.h)


# ------------------------------------------------------------------------------------------ small element-wise ops (derived bounds)
@case("axpy", "ddim_update", "div_add", "collect_feat")
def case_elementwise(k):
    g = gen(9)
    a, b = torch.randn(257, 7, generator=g), torch.randn(257, 7, generator=g)
    f32 = lambda v: float(np.float32(v))  # noqa: E731  (the ABI takes float scalars)
    al = 0.37
    r = k.call("axpy", a, b, al)
    # a + alpha b: the product and the sum are rounded (a fused multiply-add rounds once): k = 2, terms |a| + |alpha b|
    R = a.double() + f32(al) * b.double()
    k.within("axpy", r.e, r.h, R, 2 * U * (a.double().abs() + abs(f32(al)) * b.double().abs()), "derived: 2 eps (|a| + |alpha b|)")
    c1, c2, c3, c4 = 0.6, 0.8, 0.9, 0.43588989435
    for final in (False, True):
        r = k.call("ddim_update", a, b, c3, c1, c2, c4, final)
        x0 = (a.double() - f32(c1) * b.double()) / f32(c2)
        t0 = (a.double().abs() + abs(f32(c1)) * b.double().abs()) / f32(c2)
        if final:  # product, difference, quotient: k = 3
            R, B = x0, 3 * U * t0
        else:      # ... then two products and a sum: k = 6
            R = f32(c3) * x0 + f32(c4) * b.double()
            B = 6 * U * (f32(c3) * t0 + abs(f32(c4)) * b.double().abs())
        k.within(f"ddim_update final={final}", r.e, r.h, R, B, "derived: k eps sum|terms|, k = 3 (final) / 6")
    color = torch.randint(0, 256, (257, 3), generator=g).float()
    for x in (color, color.to(torch.uint8)):
        r = k.call("div_add", x, 127.5, -1.0)
        # quotient and sum: k = 2, terms |x / div| + |add|
        R = x.double() / 127.5 - 1.0
        k.within(f"div_add {x.dtype}", r.e, r.h, R, 2 * U * (x.double().abs() / 127.5 + 1.0), "derived: 2 eps (|x / div| + |add|)")
    for bd in (torch.float32, torch.float64):
        bb = torch.randn(257, 3, generator=g, dtype=torch.float64).to(bd)
        r = k.call("collect_feat", color, bb)
        # a concatenation; a float64 b is rounded to fp32 once: k = 1 on that part, 0 on the rest
        R = torch.cat([color.double(), bb.double()], 1)
        k.within(f"collect_feat b={bd}", r.e, r.h, R, U * R.abs(), "derived: 1 eps |b| (the fp64 -> fp32 rounding), else exact")


def _ld(t):
    return t.double().numpy().astype(np.longdouble)


@case("center_shift", "tta_apply")
def case_test_time_transforms(k):
    g = gen(11)
    for dtype, eps in ((torch.float32, U), (torch.float64, U64)):
        coord = (torch.randn(257, 3, generator=g, dtype=torch.float64) * 3 + 1).to(dtype)
        for apply_z in (True, False):
            r = k.call("center_shift", coord, apply_z)
            x = _ld(coord)
            mn, mx = x.min(0), x.max(0)
            ctr = np.array([(mn[0] + mx[0]) / 2, (mn[1] + mx[1]) / 2, mn[2] if apply_z else 0.0], dtype=np.longdouble)
            R = torch.from_numpy((x - ctr).astype(np.float64))
            # (min + max) is rounded (the halving is exact), then the difference: k = 2, terms |coord| + |centre|
            B = 2 * eps * torch.from_numpy((np.abs(x) + np.abs(ctr)).astype(np.float64)) + (U64 * R.abs() if dtype == torch.float64 else 0)
            k.within(f"center_shift {dtype} apply_z={apply_z}", r.e, r.h, R, B, "derived: 2 eps (|coord| + |centre|), eps of coord's type")
    xyz = torch.randn(257, 3, generator=g) * 4
    ang = 0.5
    rot = [[math.cos(ang), -math.sin(ang), 0.0], [math.sin(ang), math.cos(ang), 0.0], [0.0, 0.0, 1.0]]
    for scale in (None, 0.95):
        r = k.call("tta_apply", xyz, rot, scale)
        x, rm = _ld(xyz), np.array(rot, dtype=np.longdouble)
        R = x @ rm.T * (np.longdouble(scale) if scale is not None else 1)
        mass = np.abs(x) @ np.abs(rm).T * (abs(scale) if scale is not None else 1)
        # float64: three products, two sums, the scale: k = 6 (+ the rounding of R to fp64 for the comparison)
        k.within(f"tta_apply rot scale={scale}", r.e, r.h, torch.from_numpy(R.astype(np.float64)), 7 * U64 * torch.from_numpy(mass.astype(np.float64)),
                 "derived: 6 eps64 sum|x_i R_ji| |scale| (+1: R held in fp64)")
    r = k.call("tta_apply", xyz, None, None, True)
    k.same("tta_apply flip", r.e, r.h)
    r = k.call("tta_apply", xyz)
    k.same("tta_apply identity", r.e, r.h)


@case("voxelize", "voxelize_any", "max_run", "fragment_select")
def case_gridsample(k):
    for tag in ("room", "neg"):
        fx = load_fixture(f"gridsample_test_{tag}.npz")
        coord, gs = torch.as_tensor(fx["coord"][:600]), float(fx["grid_size"])
        r = k.call("voxelize", coord, gs)
        k.same(f"voxelize {tag}", r.e, r.h)
        r = k.call("voxelize_any", coord, gs)
        k.same(f"voxelize_any fp32 {tag}", r.e, r.h)
        r = k.call("voxelize_any", coord.double() * 1.0009765625, gs)
        k.same(f"voxelize_any fp64 {tag}", r.e, r.h)
        key = r.e[1]
        ks, idx_sort = EMU_OF["sort_pairs"](key)
        flag = torch.ones_like(ks, dtype=torch.bool)
        flag[1:] = ks[1:] != ks[:-1]
        seg = torch.cat([torch.nonzero(flag).flatten(), torch.tensor([ks.numel()])]).int()
        m = seg.numel() - 1
        r = k.call("max_run", seg, m)
        k.same(f"max_run {tag}", r.e, r.h)
        for frag in range(int(r.e) + 1):
            rr = k.call("fragment_select", idx_sort, seg, m, frag)
            k.same(f"fragment_select {tag} frag={frag}", rr.e, rr.h)


@case("softmax_vote", "argmax_rows")
def case_vote(k):
    g = gen(13)
    n, c = 257, 20
    pred0 = torch.rand(n, c, generator=g) + 0.5
    for m in (1, 65):
        logits = torch.randn(m, c, generator=g) * 4
        idx = torch.randperm(n, generator=g)[:m].int()  # (every entry names a row of pred, no row twice: no sentinel, no atomics)
        r = k.call("softmax_vote", logits, idx, pred0)
        p = torch.softmax(logits.double(), -1)
        R = pred0.double().clone()
        R[idx.long()] += p
        # softmax: shift (1), exp (2 ulp), the c-term sum (c - 1), the quotient (1), then the += (1 more on |pred| + p)
        B = U * pred0.double().abs()
        B[idx.long()] = (c + 3) * U * p + U * (pred0.double()[idx.long()].abs() + p)
        B[torch.ones(n, dtype=torch.bool).index_fill(0, idx.long(), False)] = 0.0  # rows no index names: unchanged
        k.within(f"softmax_vote m={m} (whole pred)", r.ea[2], r.ha[2], R, B, "derived: (c + 3) eps p + eps (|pred| + p); other rows exact")
        k.same(f"softmax_vote m={m} returns pred", r.e, r.ea[2])
    x = torch.randint(-3, 4, (65, 200), generator=g).float()  # an integer lattice: every row's maximum is tied many times
    x[3] = -1.0
    x[4, 70] = x[4, 199] = 9.0
    r = k.call("argmax_rows", x)
    k.same("argmax_rows (first maximum)", r.e, r.h)
    assert r.h[3] == 0 and r.h[4] == 70 and torch.equal(r.h.long(), torch.stack([torch.nonzero(row == row.max())[0, 0] for row in x]))


@case("knn1", "iou_counts")
def case_evaluator(k):
    """An integer lattice with half-integer queries: every distance is exact in fp32 and fp64, most minima are tied, the lowest
    index wins (include/cdseg.h).  Two batch elements, the second without a reference point (-1, the reference's 1e10)."""
    rng = np.random.default_rng(17)
    lat = torch.as_tensor(rng.integers(0, 6, size=(400, 3)).astype(np.float32))
    q = torch.as_tensor(rng.integers(0, 6, size=(257, 3)).astype(np.float32) + np.float32(0.5))
    roff, qoff = torch.tensor([400, 400], dtype=torch.int32), torch.tensor([250, 257], dtype=torch.int32)
    r = k.call("knn1", lat, roff, q, qoff, [0.0, 0.0, 0.0], 1.0, True)
    d = ((q[:250, None].double() - lat[None].double()) ** 2).sum(-1)
    want = torch.stack([torch.nonzero(row == row.min())[0, 0] for row in d]).int()
    assert int(((d == d.min(1, keepdim=True).values).sum(1) > 1).sum()) > 100  # tied minima
    k.same("knn1 idx (lowest index on ties)", r.e[0], r.h[0])
    assert torch.equal(r.h[0][:250], want) and bool((r.h[0][250:] == -1).all())
    R = torch.cat([d.min(1).values, torch.full((7,), 1e10, dtype=torch.float64)])
    k.within("knn1 dist2", r.e[1], r.h[1], R, 1e-6 * (1 + R), "test_knn1_vs_bruteforce_oracle (_knn_case): 1e-6 (1 + d2)")
    r = k.call("knn1", lat, roff[:1], q[:250], qoff[:1], [0.0, 0.0, 0.0], 0.5)
    k.same("knn1 idx only", r.e, r.h)
    K_ = 7
    pred = torch.as_tensor(rng.integers(-1, K_ + 1, size=300).astype(np.int32))  # out-of-range predictions count nowhere
    target = torch.as_tensor(rng.integers(-1, K_, size=257).astype(np.int32))
    pidx = torch.as_tensor(rng.integers(0, 300, size=257).astype(np.int32))      # (no sentinel: every entry names a row of pred)
    for ign in (-1, 2):
        r = k.call("iou_counts", pred[:257].contiguous(), target, K_, ign)
        k.same(f"iou_counts ignore={ign}", r.e, r.h)
        r = k.call("iou_counts", pred, target, K_, ign, pidx)
        k.same(f"iou_counts ignore={ign} pred_idx", r.e, r.h)


# ------------------------------------------------------------------------------------------ randn (value-conformant)
def _randn64(n, seed, offset):
    """The device generator's normals in fp64: Philox4x32-10 words (oracle/philox.py), Box-Muller evaluated in double."""
    from oracle import philox as P
    nt = (n + 3) // 4
    t = np.arange(nt, dtype=np.uint64)
    ctr = np.stack([(t & np.uint64(0xFFFFFFFF)).astype(np.uint32), (t >> np.uint64(32)).astype(np.uint32),
                    np.full(nt, offset & 0xFFFFFFFF, dtype=np.uint32), np.full(nt, (offset >> 32) & 0xFFFFFFFF, dtype=np.uint32)], -1)
    key = np.stack([np.full(nt, seed & 0xFFFFFFFF, dtype=np.uint32), np.full(nt, (seed >> 32) & 0xFFFFFFFF, dtype=np.uint32)], -1)
    c = P.philox4x32_10(ctr, key)
    out = np.empty((nt, 4), dtype=np.float64)
    for h in range(2):
        u1 = ((c[:, 2 * h] >> np.uint32(8)).astype(np.float64) + 1.0) / 16777216.0
        u2 = (c[:, 2 * h + 1] >> np.uint32(8)).astype(np.float64) / 16777216.0
        rr = np.sqrt(-2.0 * np.log(u1))
        out[:, 2 * h], out[:, 2 * h + 1] = rr * np.cos(2 * np.pi * u2), rr * np.sin(2 * np.pi * u2)
    return torch.from_numpy(out.reshape(-1)[:n].copy())


@case("randn")
def case_randn(k):
    """Value-conformant: the emulation draws the device generator's stream (oracle/philox.py)."""
    dev = torch.device("cuda")
    src = "test_device_noise_matches_the_philox_oracle: 2e-5"
    for shape, seed, offset in (((1,), 0, 0), ((65, 7), 54421566, 3), ((257,), (1 << 61) + 12345, (1 << 40) + 7)):
        e = EMU_OF["randn"](shape, seed, offset, torch.device("cpu"))
        h = k.ops.randn(shape, seed, offset, dev).cpu()
        n = int(np.prod(shape))
        k.within(f"randn {shape} seed={seed} offset={offset}", e, h, _randn64(n, seed, offset).reshape(shape), 2e-5, src)
    # out: a row slice of a larger, pre-filled buffer is filled in place and returned; the other rows stay
    big = torch.full((9, 16), 7.0)
    eb, hb = big.clone(), big.clone().cuda()
    eo = EMU_OF["randn"]((4, 16), 5, 6, torch.device("cpu"), out=eb[2:6])
    ho = k.ops.randn((4, 16), 5, 6, dev, out=hb[2:6])
    assert eo.data_ptr() == eb[2:6].data_ptr() and ho.data_ptr() == hb[2:6].data_ptr()
    k.within("randn(out=) (whole buffer)", eb, hb.cpu(), torch.cat([big[:2].double(), _randn64(64, 5, 6).reshape(4, 16), big[6:].double()]),
             torch.cat([torch.zeros(2, 16), torch.full((4, 16), 2e-5), torch.zeros(3, 16)]).double(), src + "; other rows exact")
    for side, fn, d in (("emu", EMU_OF["randn"], torch.device("cpu")), ("hip", k.ops.randn, dev)):
        a, b, c = fn((257,), 1, 2, d), fn((257,), 2, 1, d), fn((257,), 1, 2, d)
        assert a.dtype == torch.float32 and tuple(a.shape) == (257,) and torch.equal(a, c), side
        assert float((a == b).float().mean()) < 0.05, f"{side}: (seed, offset) = (1, 2) and (2, 1) give one stream"


# ------------------------------------------------------------------------------------------ dense ops
def _gemm_inputs(k, dtype, M, N, Kd, seed):
    g = gen(seed)
    A, W = torch.randn(M, Kd, generator=g), torch.randn(N, Kd, generator=g) / Kd ** 0.5
    if dtype != torch.float32:
        A, W = k.r16(A), k.r16(W)
    return g, A, W


@case("gemm", lp=True)
def case_gemm(k):
    """Bounds: tests/test_gpu_ops.py - test_gemm_plain (2e-5 sqrt(K) + 1e-5; with GELU + residual 2e-5 sqrt(K) + 1e-4, the 16-bit
    copy 0.02 max + 1e-2), test_gemm_epilogue_bn_gather_add_scatter (5e-4; the pre-add copy 1e-4 / 0.03 of 1 + max),
    test_sparse_conv_gemm_vs_oracle (2e-4), test_gemm_fused_layernorm_epilogue (2e-4 + 2e-5 sqrt(K); h 2e-4 / 0.03 of 1 + max)."""
    O = k.ops
    for dtype in (torch.float32, k.T):
        for M in ROWS:
            N, Kd = 40, 48
            g, A, W = _gemm_inputs(k, dtype, M, N, Kd, 100 + M)
            b, res = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
            Ad, Wd = A.to(dtype), W.to(dtype)
            lin = A.double() @ W.double().t() + b.double()
            r = k.call("gemm", Ad, Wd, torch.full((M, N), 3.0), bias=b)
            k.within(f"gemm plain {dtype} M={M}", r.ea[2], r.ha[2], lin, 2e-5 * Kd ** 0.5 + 1e-5, "test_gemm_plain")
            r = k.call("gemm", Ad, Wd, torch.full((M, N), 3.0), bias=b, act=O.ACT_GELU, res=res, out2=torch.full((M, N), 3.0, dtype=k.T))
            R2 = F.gelu(lin) + res.double()
            k.within(f"gemm gelu+res {dtype} M={M}", r.ea[2], r.ha[2], R2, 2e-5 * Kd ** 0.5 + 1e-4, "test_gemm_plain")
            k.within(f"gemm gelu+res out2 {dtype} M={M}", r.ek["out2"], r.hk["out2"], R2, 0.02 * float(R2.abs().max()) + 1e-2, "test_gemm_plain")
        # BN fold + GELU + gathered add + scattered rows + the pre-add copy; out has 9 rows nothing writes
        M, N, Kd, Mc = 65, 32, 64, 20
        g, A, W = _gemm_inputs(k, dtype, M, N, Kd, 7)
        b, sc, sh = torch.randn(N, generator=g), torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g)
        child = torch.randn(Mc, N, generator=g)
        aidx = torch.randint(0, Mc, (M,), generator=g).int()
        oidx = torch.randperm(M + 9, generator=g)[:M].int()
        oidx[[2, 40]] = -1  # a row that is written nowhere (out, out2); add_idx has no sentinel
        wr = oidx >= 0
        pre = F.gelu((A.double() @ W.double().t() + b.double()) * sc.double() + sh.double())
        R = torch.full((M + 9, N), 3.0, dtype=torch.float64)
        R[oidx[wr].long()] = (pre + child.double()[aidx.long()])[wr]
        B = torch.zeros(M + 9, N, dtype=torch.float64)
        B[oidx[wr].long()] = 5e-4
        r = k.call("gemm", A.to(dtype), W.to(dtype), torch.full((M + 9, N), 3.0), bias=b, scale=sc, shift=sh, act=O.ACT_GELU, add_src=child,
                   add_idx=aidx, out_idx=oidx, out2=torch.full((M, N), 3.0, dtype=dtype), out2_pre_add=True)
        k.within(f"gemm epilogue {dtype} (whole out)", r.ea[2], r.ha[2], R, B, "test_gemm_epilogue_bn_gather_add_scatter; unaddressed rows exact")
        R2 = torch.where(wr[:, None], pre, torch.full_like(pre, 3.0))
        B2 = torch.where(wr[:, None], torch.full_like(pre, (1e-4 if dtype == torch.float32 else 0.03) * (1 + float(pre.abs().max()))), torch.zeros_like(pre))
        k.within(f"gemm epilogue out2 {dtype}", r.ek["out2"], r.hk["out2"], R2, B2, "test_gemm_epilogue_bn_gather_add_scatter; skipped rows exact")
        # the fused LayerNorm epilogues, in place on the residual
        M, N, Kd = 65, 48, 32
        g, A, W = _gemm_inputs(k, dtype, M, N, Kd, 8)
        b, res, cb = torch.randn(N, generator=g), torch.randn(M, N, generator=g), torch.randn(N, generator=g)
        g1, b1, g2, b2 = (torch.randn(N, generator=g) for _ in range(4))
        y = A.double() @ W.double().t() + b.double()
        xR = res.double() + F.layer_norm(y, (N,), g1.double(), b1.double(), 1e-5) + cb.double()
        hR = F.layer_norm(xR, (N,), g2.double(), b2.double(), 1e-5)
        x = res.clone()
        e_x, h_x = x.clone(), x.clone().cuda()
        e_h, h_h = torch.full((M, N), 3.0, dtype=dtype), torch.full((M, N), 3.0, dtype=dtype).cuda()
        EMU_OF["gemm"](A.to(dtype), W.to(dtype), e_x, bias=b, ln_pre=(g1, b1), res=e_x, colbias=cb, ln_post=(g2, b2), ln_out=e_h)
        O.gemm(A.to(dtype).cuda(), W.to(dtype).cuda(), h_x, bias=b.cuda(), ln_pre=(g1.cuda(), b1.cuda()), res=h_x, colbias=cb.cuda(),
               ln_post=(g2.cuda(), b2.cuda()), ln_out=h_h)
        torch.cuda.synchronize()
        k.within(f"gemm ln_pre+ln_post x {dtype}", e_x, h_x.cpu(), xR, 2e-4 + 2e-5 * Kd ** 0.5, "test_gemm_fused_layernorm_epilogue")
        k.within(f"gemm ln_pre+ln_post h {dtype}", e_h, h_h.cpu(), hR, (2e-4 if dtype == torch.float32 else 0.03) * (1 + float(hR.abs().max())),
                 "test_gemm_fused_layernorm_epilogue")
        # the gathered-A (sparse conv) form on a kernel map with -1 entries: no contribution
        c = cloud("tiny64")
        C = 16
        for kmajor in (False, True):
            nbr = EMU_OF["nbr_table"](c.zs, c.g0, c.b0, c.depth, 3, kmajor)
            g = gen(21)
            xx, w = torch.randn(c.n, C, generator=g), torch.randn(C, 27 * C, generator=g) / (27 * C) ** 0.5
            if dtype != torch.float32:
                xx, w = k.r16(xx), k.r16(w)
            bb = torch.randn(C, generator=g)
            nb_ = (nbr.t() if kmajor else nbr).long()
            R = bb.double().expand(c.n, C).clone()
            for o in range(27):
                live = nb_[:, o] >= 0
                R[live] += xx.double()[nb_[live, o]] @ w.double()[:, o * C:(o + 1) * C].t()
            r = k.call("gemm", xx.to(dtype), w.to(dtype), torch.full((c.n, C), 3.0), bias=bb, nbr=nbr, kvol=27, nbr_kmajor=kmajor)
            k.within(f"gemm sparse conv {dtype} kmajor={kmajor}", r.ea[2], r.ha[2], R, 2e-4, "test_sparse_conv_gemm_vs_oracle")


@case("gemv", "layernorm", "segment_max", "segment_mean", lp=True)
def case_small_dense(k):
    O = k.ops
    g = gen(31)
    w, b, x = torch.randn(33, 20, generator=g) / 20 ** 0.5, torch.randn(33, generator=g), torch.randn(20, generator=g)
    for act in (O.ACT_NONE, O.ACT_SWISH, O.ACT_GELU):
        r = k.call("gemv", w, b, x, act)
        v = w.double() @ x.double() + b.double()
        R = {O.ACT_NONE: v, O.ACT_SWISH: v * torch.sigmoid(v), O.ACT_GELU: F.gelu(v)}[act]
        k.within(f"gemv act={act}", r.e, r.h, R, 1e-5, "test_timestep_embedding_chain: 1e-5")
    for M in ROWS:
        C = 48
        x = torch.randn(M, C, generator=g) * 3 + 1
        gm, bt, res, cb = torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(M, C, generator=g), torch.randn(C, generator=g)
        R = F.layer_norm(x.double(), (C,), gm.double(), bt.double(), 1e-5)
        r = k.call("layernorm", x, gm, bt, torch.full((M, C), 3.0))
        k.within(f"layernorm fp32 M={M}", r.ea[3], r.ha[3], R, 2e-5, "test_layernorm: 2e-5")
        R2 = R + res.double() + cb.double()
        r = k.call("layernorm", x, gm, bt, torch.full((M, C), 3.0), res=res, colbias=cb, out2=torch.full((M, C), 3.0, dtype=k.T))
        k.within(f"layernorm res+colbias M={M}", r.ea[3], r.ha[3], R2, 2e-5, "test_layernorm: 2e-5")
        k.within(f"layernorm res+colbias out2 M={M}", r.ek["out2"], r.hk["out2"], R2, 0.02 * (1 + float(R2.abs().max())), "test_layernorm: 0.02 (1 + max)")
        R16 = F.layer_norm(k.r16(x).double(), (C,), gm.double(), bt.double(), 1e-5)
        r = k.call("layernorm", x.to(k.T), gm, bt, torch.full((M, C), 3.0, dtype=k.T))
        k.within(f"layernorm 16 bit M={M}", r.ea[3], r.ha[3], R16, 0.02 * (1 + float(R16.abs().max())), "test_layernorm: 0.02 (1 + max)")
    # pooling maximum: small dyadic values, so every run's maximum is tied (the value does not depend on which row wins)
    m, C = 65, 32
    counts = torch.randint(1, 9, (m,), generator=g)
    seg = torch.cat([torch.zeros(1, dtype=torch.long), counts.cumsum(0)]).int()
    n = int(seg[-1])
    cl = torch.repeat_interleave(torch.arange(m), counts)
    sc, sh = torch.randn(C, generator=g), torch.randn(C, generator=g)  # negative scales too: the maximum comes first
    for dtype in (torch.float32, k.T):
        y = (torch.randint(-4, 5, (n, C), generator=g).float() / 4).to(dtype)
        mx = torch.full((m, C), -math.inf, dtype=torch.float64).scatter_reduce(0, cl[:, None].expand(n, C), y.double(), "amax")
        R = F.gelu(mx * sc.double() + sh.double())
        r = k.call("segment_max", y, seg, m, sc, sh, O.ACT_GELU, torch.full((m, C), 3.0), torch.full((m, C), 3.0, dtype=k.T))
        k.within(f"segment_max {dtype} out", r.ea[6], r.ha[6], R, 1e-5, "test_segment_max_and_mean: 1e-5")
        k.within(f"segment_max {dtype} out2", r.ea[7], r.ha[7], R, 0.01 * (1 + float(R.abs().max())), "test_segment_max_and_mean: 0.01 (1 + max)")
        r = k.call("segment_max", y, seg, m, None, None, O.ACT_NONE, torch.full((m, C), 3.0))
        k.within(f"segment_max {dtype} plain", r.ea[6], r.ha[6], mx, 1e-5, "test_segment_max_and_mean: 1e-5")
    xyz = torch.randn(n, 3, generator=g)
    r = k.call("segment_mean", xyz, seg, m)
    R = torch.zeros(m, 3, dtype=torch.float64).index_add_(0, cl, xyz.double()) / counts.double()[:, None]
    k.within("segment_mean", r.e, r.h, R, 1e-5, "test_segment_max_and_mean: 1e-5")


# ------------------------------------------------------------------------------------------ attention
def _attn_plan(lens, K_, seed):
    """A random serialized order per batch element, its padded slot plan from the emulated pad_plan, the patch table."""
    g = gen(seed)
    offset = np.cumsum(lens)
    n = int(offset[-1])
    starts = np.concatenate([[0], offset[:-1]])
    order = np.concatenate([s + torch.randperm(int(c), generator=g).numpy() for s, c in zip(starts, lens)]).astype(np.int32)
    pad, unpad, cu = S.padding_plan(offset, K_)
    offs = torch.as_tensor(np.concatenate([[0], offset]).astype(np.int32))
    counts = np.diff(offs.numpy())
    pc = np.where(counts > K_, (counts + K_ - 1) // K_ * K_, counts)
    offs_pad = torch.as_tensor(np.concatenate([[0], np.cumsum(pc)]).astype(np.int32))
    gidx, widx = EMU_OF["pad_plan"](torch.as_tensor(order), offs, offs_pad, K_, int(offs_pad[-1]))
    return n, gidx, widx, np.asarray(cu, dtype=np.int32), g


ATTN_SHAPES = (([33, 100], 2, 16), ([10], 1, 4))


@case("attention", lp=True)
def case_attention(k):
    """out rows by widx (-1: the borrowed duplicate writes nothing); three rows behind the n points stay as they were."""
    for lens, H, K_ in ATTN_SHAPES:
        n, gidx, widx, cu, g = _attn_plan(lens, K_, sum(lens) + H)
        C = 16 * H
        assert bool((widx < 0).any())  # a padded last patch borrows rows: their write index is -1
        for dtype, tol, src in ((torch.float32, 2e-5, "test_attention_fp32_vs_oracle: 2e-5 (1 + max)"), (k.T, 0.02, "test_attention_bf16_vs_oracle: 0.02 (1 + max)")):
            qkv = torch.randn(n, 3 * C, generator=g)
            qkv[:, :C] *= 2.0
            if dtype != torch.float32:
                qkv = k.r16(qkv)
            q, kk, v = (qkv[:, i * C:(i + 1) * C].double() for i in range(3))
            scale = 16 ** -0.5
            o = OM._patch_attention(q[gidx.long()], kk[gidx.long()], v[gidx.long()], cu.astype(np.int64), H, scale)
            R = torch.full((n + 3, C), 3.0, dtype=torch.float64)
            live = widx >= 0
            R[widx[live].long()] = o[live]
            B = torch.full((n + 3, C), tol * (1 + float(o.abs().max())), dtype=torch.float64)
            B[n:] = 0.0
            x = qkv.to(dtype)
            e_out, h_out = torch.full((n + 3, C), 3.0, dtype=dtype), torch.full((n + 3, C), 3.0, dtype=dtype).cuda()
            EMU_OF["attention"](x[:, :C], x[:, C:2 * C], x[:, 2 * C:], gidx, gidx, widx, torch.as_tensor(cu), H, int(np.diff(cu).max()), scale, e_out)
            xd = x.cuda()
            k.ops.attention(xd[:, :C], xd[:, C:2 * C], xd[:, 2 * C:], gidx.cuda(), gidx.cuda(), widx.cuda(), torch.as_tensor(cu).cuda(), H,
                            int(np.diff(cu).max()), scale, h_out)
            torch.cuda.synchronize()
            k.within(f"attention {dtype} lens={lens} H={H} K={K_} (whole out)", e_out, h_out.cpu(), R, B, src + "; unaddressed rows exact")


@case("attention_bwd")
def case_attention_bwd(k):
    """dq / dk / dv += from a non-zero pre-fill (fp32 operands).  Bound: tests/test_gpu_train_fp32.py _attn_assert -
    max |g - R| <= (2 E_ref + max_len 2^-24) max |R|, E_ref the error of torch's fp32 autograd (which the emulation is)."""
    for lens, H, K_ in ATTN_SHAPES:
        n, gidx, widx, cu, g = _attn_plan(lens, K_, sum(lens) + 3 * H)
        C = 16 * H
        qkv = torch.randn(n, 3 * C, generator=g)
        dout = torch.randn(n, C, generator=g)
        scale = 16 ** -0.5
        q64, k64, v64 = (qkv[:, i * C:(i + 1) * C].double().clone().requires_grad_(True) for i in range(3))
        o = OM._patch_attention(q64[gidx.long()], k64[gidx.long()], v64[gidx.long()], cu.astype(np.int64), H, scale)
        live = widx >= 0
        (o[live] * dout.double()[widx[live].long()]).sum().backward()
        pre = torch.randn(n, 3 * C, generator=g)
        e_d, h_d = pre.clone(), pre.clone().cuda()
        ps = [int(v) for v in cu]
        EMU_OF["attention_bwd"](qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], gidx, gidx, widx, torch.as_tensor(cu), ps, H, scale, dout,
                                e_d[:, :C], e_d[:, C:2 * C], e_d[:, 2 * C:])
        xd = qkv.cuda()
        k.ops.attention_bwd(xd[:, :C], xd[:, C:2 * C], xd[:, 2 * C:], gidx.cuda(), gidx.cuda(), widx.cuda(), torch.as_tensor(cu).cuda(), ps, H, scale,
                            dout.cuda(), h_d[:, :C], h_d[:, C:2 * C], h_d[:, 2 * C:])
        torch.cuda.synchronize()
        for i, (tn, g64) in enumerate(zip(("dq", "dk", "dv"), (q64.grad, k64.grad, v64.grad))):
            e, h = e_d[:, i * C:(i + 1) * C], h_d.cpu()[:, i * C:(i + 1) * C]
            p = pre[:, i * C:(i + 1) * C]
            top = float(g64.abs().max())
            e_ref = float(((e - p).double() - g64).abs().max()) / top
            k.within(f"attention_bwd lens={lens} H={H} {tn} (pre-fill + gradient)", e, h, p.double() + g64,
                     (2 * e_ref + int(np.diff(cu).max()) * U) * top + U * p.double().abs(),
                     "test_attention_bwd_fp32_at_deep_head_counts (_attn_assert): (2 E_ref + max_len eps) max|R|, + eps |pre-fill| for the +=")


# ------------------------------------------------------------------------------------------ fused Block heads / tails, conv, pooling
def _block_weights(k, C, g):
    rnd = lambda *sh, s=1.0: k.r16(torch.randn(*sh, generator=g) * s)  # noqa: E731
    W = types.SimpleNamespace(wl=rnd(C, C, s=C ** -0.5), wq=rnd(3 * C, C, s=C ** -0.5), wp=rnd(C, C, s=C ** -0.5), w1=rnd(4 * C, C, s=C ** -0.5),
                              w2=rnd(C, 4 * C, s=(4 * C) ** -0.5))
    for name, n_ in (("bl", C), ("bq", 3 * C), ("bp", C), ("b1", 4 * C), ("b2", C), ("g1", C), ("be1", C), ("g2", C), ("be2", C), ("g3", C), ("be3", C), ("cb", C)):
        setattr(W, name, torch.randn(n_, generator=g))
    return W


def _head_R(k, W, y, x0, cb, C):
    t = y.double() @ W.wl.double().t() + W.bl.double()
    xR = x0.double() + F.layer_norm(t, (C,), W.g1.double(), W.be1.double(), 1e-5) + (cb.double() if cb is not None else 0)
    hR = k.r16(F.layer_norm(xR, (C,), W.g2.double(), W.be2.double(), 1e-5).float()).double()
    return xR, hR @ W.wq.double().t() + W.bq.double()


def _tail_R(k, W, o, x0, C):
    xr = x0.double() + o.double() @ W.wp.double().t() + W.bp.double()
    hr = k.r16(F.layer_norm(xr, (C,), W.g3.double(), W.be3.double(), 1e-5).float()).double()
    u = k.r16(F.gelu(hr @ W.w1.double().t() + W.b1.double()).float()).double()
    return xr + u @ W.w2.double().t() + W.b2.double()


@case("cpe_head_fused", "attn_tail_fused", "mlp_fused", "block_rr_pack", "cpe_head_rr", "attn_tail_rr", lp=True)
def case_block_head_tail(k):
    """Bounds: tests/test_gpu_ops.py test_block_rr_head_and_tail_vs_fused_kernels against plain torch with the same 16-bit rounding
    points (x 1e-4, qkv 0.08, the tail 3e-2), test_mlp_fused_vs_two_gemms_and_fp64 (2e-2), the deep widths
    test_deep_head_and_tail_vs_oracle_and_unfused_sequence's.  The 16-bit copy xc is the cast of x on either side.  The
    weight images (block_rr_pack) are opaque: compared through cpe_head_rr / attn_tail_rr."""
    O, T = k.ops, k.T
    for C in (32, 128):
        wide = "test_block_rr_head_and_tail_vs_fused_kernels"
        deep = "test_deep_head_and_tail_vs_oracle_and_unfused_sequence"
        bx, sx = (1e-4, wide + ": 1e-4") if C == 32 else (2e-5 * C ** 0.5, deep + ": 2e-5 sqrt(C)")
        bq, sq = (0.08, wide + ": 0.08") if C == 32 else ((0.08 if k.lp == "bf16" else 0.012), deep + ": 0.08 (bf16) / 0.012 (f16)")
        bt, st = (3e-2, wide + ": 3e-2") if C == 32 else ((3e-2 if k.lp == "bf16" else 5e-3), deep + ": 3e-2 (bf16) / 5e-3 (f16)")
        for M in ROWS:
            g = gen(1000 * C + M)
            W = _block_weights(k, C, g)
            y, o, x0 = k.r16(torch.randn(M, C, generator=g)), k.r16(torch.randn(M, C, generator=g)), torch.randn(M, C, generator=g)
            t16 = lambda t: t.to(T)  # noqa: E731
            pre_q, pre_c = torch.full((M, 3 * C), 3.0, dtype=T), torch.full((M, C), 3.0, dtype=T)
            # ---- the MLP alone (C = 32 / 64 / 128)
            hR = k.r16(torch.randn(M, C, generator=g))
            u = k.r16(F.gelu(hR.double() @ W.w1.double().t() + W.b1.double()).float()).double()
            R = x0.double() + u @ W.w2.double().t() + W.b2.double()
            assert O.mlp_fused_ok(t16(hR).cuda(), 4 * C) and EMU_OF["mlp_fused_ok"](t16(hR), 4 * C)
            r = k.call("mlp_fused", t16(hR), t16(W.w1), W.b1, t16(W.w2), W.b2, x0, pre_c)
            k.within(f"mlp_fused C={C} M={M} x", r.ea[5], r.ha[5], R, 2e-2, "test_mlp_fused_vs_two_gemms_and_fp64: 2e-2")
            assert torch.equal(r.ha[6], r.ha[5].to(T)) and torch.equal(r.ea[6], r.ea[5].to(T))  # xc = cast(x)
            for cb in (None, W.cb):
                xR, qR = _head_R(k, W, y, x0, cb, C)
                calls = []
                if C == 32:
                    assert O.cpe_head_fused_ok(t16(y).cuda()) and EMU_OF["cpe_head_fused_ok"](t16(y))
                    calls.append(("cpe_head_fused", k.call("cpe_head_fused", t16(y), t16(W.wl), W.bl, (W.g1, W.be1), x0, cb, (W.g2, W.be2), t16(W.wq),
                                                            W.bq, pre_q), 4, 9))
                assert O.block_rr_ok(C, T) and EMU_OF["block_rr_ok"](C, T)
                e_img = EMU_OF["block_rr_pack"](C, t16(W.wl), t16(W.wq), t16(W.wp), t16(W.w1), t16(W.w2))
                h_img = O.block_rr_pack(C, *(t16(w).cuda() for w in (W.wl, W.wq, W.wp, W.w1, W.w2)))
                e_x, h_x, e_q, h_q = x0.clone(), x0.clone().cuda(), pre_q.clone(), pre_q.clone().cuda()
                EMU_OF["cpe_head_rr"](t16(y), e_img[0], W.bl, (W.g1, W.be1), e_x, cb, (W.g2, W.be2), W.bq, e_q)
                O.cpe_head_rr(t16(y).cuda(), h_img[0], W.bl.cuda(), (W.g1.cuda(), W.be1.cuda()), h_x, None if cb is None else cb.cuda(),
                              (W.g2.cuda(), W.be2.cuda()), W.bq.cuda(), h_q)
                torch.cuda.synchronize()
                for name, r, ix, iq in calls:
                    k.within(f"{name} C={C} M={M} cb={cb is not None} x", r.ea[ix], r.ha[ix], xR, bx, sx)
                    k.within(f"{name} C={C} M={M} cb={cb is not None} qkv", r.ea[iq], r.ha[iq], qR, bq, sq)
                k.within(f"cpe_head_rr C={C} M={M} cb={cb is not None} x", e_x, h_x.cpu(), xR, bx, sx)
                k.within(f"cpe_head_rr C={C} M={M} cb={cb is not None} qkv", e_q, h_q.cpu(), qR, bq, sq)
            R = _tail_R(k, W, o, x0, C)
            if C == 32:
                assert O.attn_tail_fused_ok(t16(o).cuda(), 4 * C) and EMU_OF["attn_tail_fused_ok"](t16(o), 4 * C)
                r = k.call("attn_tail_fused", t16(o), t16(W.wp), W.bp, W.g3, W.be3, t16(W.w1), W.b1, t16(W.w2), W.b2, x0, pre_c)
                k.within(f"attn_tail_fused C={C} M={M} x", r.ea[9], r.ha[9], R, 3e-2, "test_attn_tail_fused_equals_proj_ln_mlp_sequence: 3e-2")
                assert torch.equal(r.ha[10], r.ha[9].to(T)) and torch.equal(r.ea[10], r.ea[9].to(T))
            e_x, h_x, e_c, h_c = x0.clone(), x0.clone().cuda(), pre_c.clone(), pre_c.clone().cuda()
            EMU_OF["attn_tail_rr"](t16(o), e_img[1], W.bp, W.g3, W.be3, W.b1, W.b2, e_x, e_c)
            O.attn_tail_rr(t16(o).cuda(), h_img[1], W.bp.cuda(), W.g3.cuda(), W.be3.cuda(), W.b1.cuda(), W.b2.cuda(), h_x, h_c)
            torch.cuda.synchronize()
            k.within(f"attn_tail_rr C={C} M={M} x", e_x, h_x.cpu(), R, bt, st)
            assert torch.equal(h_c.cpu(), h_x.cpu().to(T)) and torch.equal(e_c, e_x.to(T))


def _subcloud(name, per):
    """The first `per` points (caller order) of every batch element of a golden cloud, planned with the emulated ops."""
    key = (name, per)
    if key not in _CLOUDS:
        E = types.SimpleNamespace(**EMU_OF)
        fx = load_fixture(f"serialization_{name}.npz")
        ends = [0] + [int(v) for v in fx["offset"]]
        keep = np.concatenate([np.arange(a, min(a + per, b)) for a, b in zip(ends[:-1], ends[1:])])
        grid, batch = torch.as_tensor(fx["grid_coord"][keep]), torch.as_tensor(fx["batch"][keep])
        depth = int(fx["depth"])
        zs, perm0 = E.sort_pairs(E.encode(grid, batch, depth, "z"))
        g0, b0 = E.plan_gather_grid(grid, perm0, zs, depth)
        cl1, seg1, cnt1 = E.pool_level(zs, 3)
        m1 = int(cnt1)
        g1, b1, c41 = E.pool_gather(seg1, m1, len(keep), 1, g0, b0, E.encode4(g0, b0, depth))
        _CLOUDS[key] = types.SimpleNamespace(n=len(keep), depth=depth, zs=zs, perm0=perm0, g0=g0, b0=b0, cl1=cl1, seg1=seg1, m1=m1,
                                             pn3=E.nbr_table(c41[0].contiguous(), g1, b1, depth - 1, 3, True), cinfo=E.child_info(zs, seg1, m1),
                                             nbr3k=E.nbr_table(zs, g0, b0, depth, 3, True), nbr5=E.nbr_table(zs, g0, b0, depth, 5))
    return _CLOUDS[key]


@case("stem5_pack", "stem5", "subm_conv3_pack", "subm_conv3", "conv_wgrad", lp=True)
def case_sparse_convs(k):
    """The k = 5 stem without a kernel map and the weight-stationary k = 3 conv, each through its packed weight image, on tiny64 and
    on 70 points of each element of batch2 (neighbours never cross batch elements); kernel maps with -1 entries throughout."""
    O, T = k.ops, k.T
    for c in (cloud("tiny64"), _subcloud("batch2", 70)):
        if not hasattr(c, "nbr3k"):
            c.nbr3k = EMU_OF["nbr_table"](c.zs, c.g0, c.b0, c.depth, 3, True)
            c.nbr5 = EMU_OF["nbr_table"](c.zs, c.g0, c.b0, c.depth, 5)
        n = c.n
        g = gen(n)
        x8 = torch.zeros(n, 8)
        x8[:, :6] = k.r16(torch.randn(n, 6, generator=g))
        w = torch.zeros(32, 125, 8)
        w[:, :, :6] = k.r16(torch.randn(32, 125, 6, generator=g) / (125 * 6) ** 0.5)
        w = w.reshape(32, 1000)
        sc, sh = torch.rand(32, generator=g) + 0.5, torch.randn(32, generator=g)
        assert bool((c.nbr5 < 0).any())
        conv = torch.zeros(n, 32, dtype=torch.float64)
        for o in range(125):
            live = c.nbr5[:, o] >= 0
            conv[live] += x8.double()[c.nbr5[live, o].long()] @ w.double()[:, o * 8:(o + 1) * 8].t()
        R = F.gelu(conv * sc.double() + sh.double())
        assert O.stem5_ok(32, T) and EMU_OF["stem5_ok"](32, T)
        e_o, e_o2 = torch.full((n, 32), 3.0), torch.full((n, 32), 3.0, dtype=T)
        h_o, h_o2 = e_o.clone().cuda(), e_o2.clone().cuda()
        EMU_OF["stem5"](x8.to(T), EMU_OF["stem5_pack"](w.to(T)), sc, sh, c.g0, c.cl1, c.pn3, c.cinfo, c.depth, e_o, e_o2)
        O.stem5(x8.to(T).cuda(), O.stem5_pack(w.to(T).cuda()), sc.cuda(), sh.cuda(), c.g0.cuda(), c.cl1.cuda(), c.pn3.cuda(), c.cinfo.cuda(), c.depth, h_o, h_o2)
        torch.cuda.synchronize()
        k.within(f"stem5 n={n} out", e_o, h_o.cpu(), R, 1e-4, "test_stem5_map_free_vs_oracle: 1e-4")
        k.within(f"stem5 n={n} out2", e_o2, h_o2.cpu(), R, 0.02 * (1 + float(R.abs().max())), "test_stem5_map_free_vs_oracle: 0.02 (1 + max)")
        C = 32
        x = k.r16(torch.randn(n, C, generator=g))
        w3 = k.r16(torch.randn(C, 27 * C, generator=g) / (27 * C) ** 0.5)
        b = torch.randn(C, generator=g)
        R = b.double().expand(n, C).clone()
        for o in range(27):
            live = c.nbr3k[o] >= 0
            R[live] += x.double()[c.nbr3k[o][live].long()] @ w3.double()[:, o * C:(o + 1) * C].t()
        assert O.subm_conv3_ok(x.to(T).cuda()) and EMU_OF["subm_conv3_ok"](x.to(T))
        e_o, h_o = torch.full((n, C), 3.0, dtype=T), torch.full((n, C), 3.0, dtype=T).cuda()
        EMU_OF["subm_conv3"](x.to(T), EMU_OF["subm_conv3_pack"](w3.to(T)), b, c.nbr3k, e_o)
        O.subm_conv3(x.to(T).cuda(), O.subm_conv3_pack(w3.to(T).cuda()), b.cuda(), c.nbr3k.cuda(), h_o)
        torch.cuda.synchronize()
        k.within(f"subm_conv3 n={n}", e_o, h_o.cpu(), R, 0.01 * (1 + float(R.abs().max())), "test_subm_conv3_weight_stationary_vs_oracle: 0.01 (1 + max)")
        # the conv's weight gradient over all 27 offsets, += into pre-filled dw3 / db; fp32 and 16-bit operands
        for dtype in (torch.float32, T):
            xg = torch.randn(n, 16, generator=g)
            dy = 0.1 * torch.randn(n, 16, generator=g)
            if dtype != torch.float32:
                xg, dy = k.r16(xg), k.r16(dy)
            pre_w, pre_b = torch.randn(16, 27, 16, generator=g), torch.randn(16, generator=g)
            Rw, mass = pre_w.double().clone(), torch.zeros(16, 27, 16, dtype=torch.float64)
            for o in range(27):
                live = (c.nbr3k[o] >= 0)
                xo = xg.double()[c.nbr3k[o].clamp(min=0).long()] * live[:, None]
                Rw[:, o] += dy.double().t() @ xo
                mass[:, o] = dy.double().abs().t() @ xo.abs()
            part = O.wgrad_partition(n, 16, 16, 27, dtype)
            chain = 1.01 * (part.rows_per_split + part.splits) * U
            for det in (False, True):
                r = k.call("conv_wgrad", xg.to(dtype), c.nbr3k, dy.to(dtype), pre_w, pre_b, **({"deterministic": True} if det else {}))
                src = "test_default_conv_wgrad_on_ordinary_values_within_the_derived_bound: 1.01 (R + S) eps mass, + eps |pre-fill| for the +="
                k.within(f"conv_wgrad {dtype} n={n} det={det} dw3 (pre-fill + gradient)", r.ea[3], r.ha[3], Rw, chain * mass + U * Rw.abs(), src)
                k.within(f"conv_wgrad {dtype} n={n} det={det} db", r.ea[4], r.ha[4], pre_b.double() + dy.double().sum(0),
                         chain * dy.double().abs().sum(0) + U * pre_b.double().abs() + U, src)


@case("pool_fused_pack", "pool_fused", lp=True)
def case_pool_fused(k):
    O, T = k.ops, k.T
    for m in ROWS:
        g = gen(40 + m)
        cin, cout = 32, 64
        runs = torch.randint(1, 9, (m,), generator=g)
        seg = torch.cat([torch.zeros(1, dtype=torch.int64), runs.cumsum(0)]).int()
        n = int(seg[-1])
        x, w = k.r16(torch.randn(n, cin, generator=g)), k.r16(torch.randn(cout, cin, generator=g) / cin ** 0.5)
        b, sc, sh = torch.randn(cout, generator=g) * 0.3, torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.2
        sc[::7] *= -1.0
        cl = torch.repeat_interleave(torch.arange(m), runs)
        yt = k.r16((x.double() @ w.double().t() + b.double()).float()).double()
        mx = torch.full((m, cout), -math.inf, dtype=torch.float64).scatter_reduce(0, cl[:, None].expand(-1, cout), yt, "amax")
        R = F.gelu(mx * sc.double() + sh.double())
        assert O.pool_fused_ok(cin, cout, T) and EMU_OF["pool_fused_ok"](cin, cout, T)
        e_o, e_o2 = torch.full((m, cout), 3.0), torch.full((m, cout), 3.0, dtype=T)
        h_o, h_o2 = e_o.clone().cuda(), e_o2.clone().cuda()
        EMU_OF["pool_fused"](x.to(T), EMU_OF["pool_fused_pack"](w.to(T)), b, seg, m, sc, sh, O.ACT_GELU, e_o, e_o2)
        O.pool_fused(x.to(T).cuda(), O.pool_fused_pack(w.to(T).cuda()), b.cuda(), seg.cuda(), m, sc.cuda(), sh.cuda(), O.ACT_GELU, h_o, h_o2)
        torch.cuda.synchronize()
        tol = 2e-2 if k.lp == "bf16" else 3e-3
        k.within(f"pool_fused m={m} out", e_o, h_o.cpu(), R, tol, "test_pool_fused_equals_gemm_then_segment_max: 2e-2 (bf16) / 3e-3 (f16)")
        assert torch.equal(h_o2.cpu(), h_o.cpu().to(T)) and torch.equal(e_o2, e_o.to(T))  # out2 = the 16-bit copy of out


# ------------------------------------------------------------------------------------------ training kernels
@case("linear_wgrad", "layernorm_bwd", "gelu_bwd", lp=True)
def case_training_reductions(k):
    O, T = k.ops, k.T
    for M in ROWS:
        g = gen(50 + M)
        Kd, N = 48, 32
        for dtype in (torch.float32, T):
            x, dy = torch.randn(M + 5, Kd, generator=g), 0.1 * torch.randn(M, N, generator=g)
            if dtype != torch.float32:
                x, dy = k.r16(x), k.r16(dy)
            xidx = torch.randint(0, M + 5, (M,), generator=g).int()
            xidx[::7] = -1  # no row: no contribution
            pre_w, pre_b = torch.randn(N, Kd, generator=g), torch.randn(N, generator=g)
            part = O.wgrad_partition(M, N, Kd, 1, dtype)
            chain = 1.01 * (part.rows_per_split + part.splits) * U
            src = "test_default_wgrad_on_ordinary_values_within_the_derived_bound: 1.01 (R + S) eps mass, + eps |pre-fill| for the +="
            for idx in (None, xidx):
                xs = x[:M] if idx is None else x[idx.clamp(min=0).long()] * (idx >= 0)[:, None]
                Rw = pre_w.double() + dy.double().t() @ xs.double()
                mass = dy.double().abs().t() @ xs.double().abs()
                for det in (False, True):
                    r = k.call("linear_wgrad", (x[:M] if idx is None else x).to(dtype).contiguous(), dy.to(dtype), pre_w, pre_b, idx,
                               **({"deterministic": True} if det else {}))
                    what = f"linear_wgrad {dtype} M={M} xidx={idx is not None} det={det}"
                    k.within(what + " dw (pre-fill + gradient)", r.ea[2], r.ha[2], Rw, chain * mass + U * Rw.abs(), src)
                    k.within(what + " db", r.ea[3], r.ha[3], pre_b.double() + dy.double().sum(0),
                             chain * dy.double().abs().sum(0) + U * pre_b.double().abs() + U, src)
        C = 48
        x, gamma, dy = 0.5 + torch.randn(M, C, generator=g), 1 + 0.3 * torch.randn(C, generator=g), torch.randn(M, C, generator=g)
        pre = dict(dx=torch.randn(M, C, generator=g), dg=torch.randn(C, generator=g), db=torch.randn(C, generator=g))

        def ln_grads(dt_):
            xr, gr = x.to(dt_).clone().requires_grad_(True), gamma.to(dt_).clone().requires_grad_(True)
            br = torch.zeros_like(gr).requires_grad_(True)
            F.layer_norm(xr, (C,), gr, br, 1e-5).backward(dy.to(dt_))
            return xr.grad, gr.grad, br.grad
        g64, g32 = ln_grads(torch.float64), ln_grads(torch.float32)
        src = "test_layernorm_bwd_vs_fp64_within_three_times_torch: (3 E_torch + eps) max|R|"
        for acc in (False, True):
            for det in (False, True):
                r = k.call("layernorm_bwd", x, gamma, dy, pre["dx"], acc, 1e-5, pre["dg"], pre["db"], **({"deterministic": True} if det else {}))
                base = pre["dx"].double() if acc else 0.0
                names = (("dx", 3, g64[0] + base, g32[0] + (pre["dx"] if acc else 0.0)), ("dgamma", 6, pre["dg"].double() + g64[1], pre["dg"] + g32[1]),
                         ("dbeta", 7, pre["db"].double() + g64[2], pre["db"] + g32[2]))
                for tn, i, R, t32 in names:
                    k.within(f"layernorm_bwd M={M} accumulate={acc} det={det} {tn}", r.ea[i], r.ha[i], R, three_times_torch(t32, R), src)
        u, dyu = 2 * torch.randn(M, C, generator=g), torch.randn(M, C, generator=g)
        u64 = u.double()
        R = dyu.double() * (0.5 * torch.special.erfc(-u64 * 0.5 ** 0.5) + u64 * torch.exp(-0.5 * u64 * u64) / (2 * math.pi) ** 0.5)
        ur = u.clone().requires_grad_(True)
        F.gelu(ur).backward(dyu)
        r = k.call("gelu_bwd", u, dyu)
        k.within(f"gelu_bwd M={M}", r.e, r.h, R, three_times_torch(ur.grad, R), "test_gelu_bwd_vs_closed_form_within_three_times_torch: (3 E_torch + eps) max|R|")


@case("residual", "scale_cast", "add_layernorm", "gelu_fwd", "gelu_bwd_cast", lp=True)
def case_block_row_kernels(k):
    """The row kernels of the native training Block: residual and scale_cast are bit-equal to torch (tests/test_gpu_train_block.py
    test_residual_forward_and_backward_are_bit_equal_to_torch, test_cast_without_saturation_is_torchs_cast), x1 of add_layernorm too;
    h, g, du by the three-times-torch rule of that file (_assert_vs_torch)."""
    src = "tests/test_gpu_train_block.py _assert_vs_torch: (3 E_torch + eps) max|R|"
    for M in ROWS:
        g = gen(60 + M)
        C = 32
        x, a = 0.5 + torch.randn(M, C, generator=g), torch.randn(M, C, generator=g)
        mask = (torch.rand(M, generator=g) < 0.7).float() / 0.7
        t_rows = 0.5 * torch.randn(2, C, generator=g)
        offs = torch.tensor([0, M // 2, M], dtype=torch.int32)
        for aa, mm, tt in ((None, None, None), (a, None, None), (a, mask, None), (a, mask, t_rows), (None, None, t_rows)):
            for out in (None, torch.full((M, C), 3.0)):
                r = k.call("residual", x, aa, mm, tt, offs if tt is not None else None, out)
                k.same(f"residual M={M} a={aa is not None} mask={mm is not None} t={tt is not None} out={out is not None}", r.e, r.h)
                if out is not None:
                    k.same("residual out buffer", r.ea[5], r.ha[5])
        gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
        u, dg = 2 * torch.randn(M, 4 * C, generator=g), torch.randn(M, 4 * C, generator=g)
        for variant in (None, k.lp):
            to = (lambda t: t) if variant is None else (lambda t: t.to(k.T))
            for mm in (None, mask):
                r = k.call("scale_cast", a, mm, variant)
                k.same(f"scale_cast M={M} mask={mm is not None} {variant}", r.e, r.h)
                r = k.call("add_layernorm", x, a, mm, gamma, beta, 1e-5, variant)
                k.same(f"add_layernorm x1 M={M} mask={mm is not None} {variant}", r.e[0], r.h[0])
                x1 = x + (a if mm is None else a * mm[:, None])
                R = F.layer_norm(x1.double(), (C,), gamma.double(), beta.double(), 1e-5)
                t32 = to(F.layer_norm(x1, (C,), gamma, beta, 1e-5))
                k.within(f"add_layernorm h M={M} mask={mm is not None} {variant}", r.e[1], r.h[1], R, three_times_torch(t32, R), src)
            u64 = u.double().requires_grad_(True)
            g64 = F.gelu(u64)
            g64.backward(dg.double())
            u32 = u.clone().requires_grad_(True)
            g32 = F.gelu(u32)
            g32.backward(dg)
            r = k.call("gelu_fwd", u, variant)
            k.within(f"gelu_fwd M={M} {variant}", r.e, r.h, g64.detach(), three_times_torch(to(g32.detach()), g64.detach()), src)
            r = k.call("gelu_bwd_cast", u, dg, variant)
            k.within(f"gelu_bwd_cast M={M} {variant}", r.e, r.h, u64.grad, three_times_torch(to(u32.grad), u64.grad), src)


# ------------------------------------------------------------------------------------------ BatchNorm + GELU, pooling arg-max, run sums
@case("bn_stats", "bn_finish", "bn_gelu_fwd", "bn_gelu_bwd")
def case_batchnorm(k):
    """bn_stats / the gsums: fp64 sums of m terms in an order fixed by the shape - derived m eps64 sum|terms| against a long-double
    sum.  bn_finish: fp64 arithmetic on those sums, one rounding to fp32 (k = 2 with the fp64 noise, negligible at these inputs).
    bn_gelu_fwd / dx: the three-times-torch rule of tests/test_gpu_norm.py (_check_kinds: e <= 3 e_t + 2^-24)."""
    src3 = "tests/test_gpu_norm.py _check_kinds: (3 E_torch + eps) max|R|"
    for m in ROWS:
        g = gen(70 + m)
        c = 32
        x, dy = torch.randn(m, c, generator=g) * 2 + 0.5, torch.randn(m, c, generator=g)
        gamma, beta = 1 + 0.3 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
        xl = _ld(x)
        Rs = np.concatenate([xl.sum(0), (xl * xl).sum(0), [np.longdouble(m)]])
        mass = np.concatenate([np.abs(xl).sum(0), (xl * xl).sum(0), [0.0]])
        r = k.call("bn_stats", x)
        k.within(f"bn_stats m={m}", r.e, r.h, torch.from_numpy(Rs.astype(np.float64)), torch.from_numpy(((m + 1) * U64 * mass).astype(np.float64)),
                 "derived: (m + 1) eps64 sum|terms| (m fp64 additions, R held in fp64)")
        stats = r.e
        if m == 1:
            continue  # (one row: the variance is zero and everything behind it is eps alone; bn_stats above is the case)
        rm, rv = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
        r = k.call("bn_finish", stats, 1e-5, 0.1, rm, rv)
        mu = stats[:c] / m
        var = (stats[c:2 * c] / m - mu * mu).clamp(min=0.0)
        Rm, Ri = mu, 1.0 / torch.sqrt(var + 1e-5)
        k.within(f"bn_finish m={m} mean", r.e[0], r.h[0], Rm, 2 * U * Rm.abs() + 1e-12, "derived: 2 eps |v| (fp64, one rounding to fp32)")
        k.within(f"bn_finish m={m} invstd", r.e[1], r.h[1], Ri, 2 * U * Ri.abs(), "derived: 2 eps |v|")
        Rrm = 0.9 * rm.double() + 0.1 * mu
        Rrv = 0.9 * rv.double() + 0.1 * var * (m / (m - 1.0))
        k.within(f"bn_finish m={m} running_mean", r.ea[3], r.ha[3], Rrm, 2 * U * (0.9 * rm.double().abs() + 0.1 * mu.abs()), "derived: 2 eps sum|terms|")
        k.within(f"bn_finish m={m} running_var", r.ea[4], r.ha[4], Rrv, 2 * U * Rrv.abs(), "derived: 2 eps sum|terms|")
        mean, invstd = r.e
        z = lambda dt_: gamma.to(dt_) * ((x.to(dt_) - mean.to(dt_)) * invstd.to(dt_)) + beta.to(dt_)  # noqa: E731
        R = F.gelu(z(torch.float64))
        for out in (None, torch.full((m, c), 3.0)):
            r = k.call("bn_gelu_fwd", x, mean, invstd, gamma, beta, out)
            k.within(f"bn_gelu_fwd m={m} out={out is not None}", r.e, r.h, R, three_times_torch(F.gelu(z(torch.float32)), R), src3)
            if out is not None:
                k.same("bn_gelu_fwd returns out", r.e, r.ea[5])
                k.within(f"bn_gelu_fwd m={m} (out buffer)", r.ea[5], r.ha[5], R, three_times_torch(F.gelu(z(torch.float32)), R), src3)

        def bwd(dt_):
            xh = (x.to(dt_) - mean.to(dt_)) * invstd.to(dt_)
            zz = gamma.to(dt_) * xh + beta.to(dt_)
            gg = dy.to(dt_) * (0.5 * (1.0 + torch.erf(zz * math.sqrt(0.5))) + zz * torch.exp(-0.5 * zz * zz) / math.sqrt(2.0 * math.pi))
            s = torch.cat([gg.double().sum(0), (gg.double() * xh.double()).sum(0)])
            k1, k2 = (s[:c] / m).to(dt_), (s[c:] / m).to(dt_)
            return (gamma.to(dt_) * invstd.to(dt_)) * ((gg - k1) - xh * k2), s, torch.cat([gg.double().abs().sum(0), (gg.double() * xh.double()).abs().sum(0)])
        dx64, s64, smass = bwd(torch.float64)
        dx32 = bwd(torch.float32)[0]
        count = stats[2 * c:].clone()
        r = k.call("bn_gelu_bwd", x, dy, mean, invstd, gamma, beta, count, None, torch.full((m, c), 3.0))
        k.within(f"bn_gelu_bwd m={m} dx", r.e[0], r.h[0], dx64, three_times_torch(dx32, dx64), src3)
        k.within(f"bn_gelu_bwd m={m} (out buffer)", r.ea[8], r.ha[8], dx64, three_times_torch(dx32, dx64), src3)
        # gsums: fp64 sums of fp32-evaluated g (the g of the two sides differ by fp32 rounding: 8 eps32 on every term)
        k.within(f"bn_gelu_bwd m={m} gsums", r.e[1], r.h[1], s64, (8 * U + (m + 1) * U64) * smass + 1e-300,
                 "derived: g and x_hat are fp32 values of ~8 roundings (8 eps32 each term) + m eps64 for the fp64 sum")


@case("segment_max_arg", "segment_max_bwd", "segment_sum")
def case_pool_argmax_and_run_sums(k):
    """Small dyadic values: every run's maximum is tied, the FIRST row that holds it is the arg (include/cdseg.h); the backward
    sends the gradient there and writes every other element as zero.  segment_sum adds a run in ascending row order: bit-equal."""
    for m in ROWS:
        g = gen(80 + m)
        c = 32
        counts = torch.randint(1, 9, (m,), generator=g)
        seg = torch.cat([torch.zeros(1, dtype=torch.long), counts.cumsum(0)]).int()
        n = int(seg[-1])
        cl = torch.repeat_interleave(torch.arange(m), counts).int()
        y = torch.randint(-2, 3, (n, c), generator=g).float() / 2
        r = k.call("segment_max_arg", y, seg, m)
        k.same(f"segment_max_arg m={m}", r.e, r.h)
        out, arg = r.h
        rows = torch.arange(n)[:, None].expand(n, c)
        first = torch.full((m, c), n, dtype=torch.long).scatter_reduce(0, cl.long()[:, None].expand(n, c), torch.where(y == out[cl.long()], rows, n), "amin")
        assert torch.equal(arg.long(), first) and int((y == out[cl.long()]).sum()) > m * c  # ties, and the first row wins
        dout = torch.randn(m, c, generator=g)
        r = k.call("segment_max_bwd", dout, arg, cl)
        k.same(f"segment_max_bwd m={m}", r.e, r.h)
        assert int((r.h != 0).sum()) <= m * c
        src = torch.randn(n, c, generator=g)
        r = k.call("segment_sum", src, seg, m)
        k.same(f"segment_sum m={m}", r.e, r.h)


# ------------------------------------------------------------------------------------------ fusion gate, skip options
@case("fuse_gate_fwd", "fuse_gate_bwd")
def case_fusion_gate(k):
    """Bound: tests/test_gpu_fusion.py `_within` - |mine - R| <= 2 |torch fp32 - R| + ulp(R) element by element; the column sums are
    fp64 sums of fp64 products: derived rows eps64 sum|terms| against a long-double sum."""
    src = "tests/test_gpu_fusion.py _within: 2 E_torch + ulp(R)"
    for rows in ROWS:
        g = gen(90 + rows)
        c = 32
        s, a, dy = (torch.randn(rows, c, generator=g) for _ in range(3))
        alpha, gamma = 1 - torch.rand(c, generator=g), torch.rand(c, generator=g)
        mask = (torch.rand(rows, generator=g) < 0.7).float() / 0.7
        for mm in (None, mask):
            m64 = 1.0 if mm is None else mm.double()[:, None]
            m32 = 1.0 if mm is None else mm[:, None]
            for aa in (a, None):
                if aa is None and mm is not None:  # DropPath factors without the attention operand: an argument error on both sides
                    from cdsegnet_amd._lib import CdsegError
                    for fn, mv in ((EMU_OF["fuse_gate_fwd"], lambda t: t), (k.ops.fuse_gate_fwd, lambda t: t.cuda())):
                        with pytest.raises(CdsegError):
                            fn(mv(s), None, mv(alpha), mv(gamma), mv(mm))
                    continue
                R = alpha.double() * s.double() + (gamma.double() * m64 * aa.double() if aa is not None else 0.0)
                t32 = alpha * s + (gamma * m32 * aa if aa is not None else 0.0)
                for out in (None, torch.full((rows, c), 3.0)):
                    r = k.call("fuse_gate_fwd", s, aa, alpha, gamma, mm, out)
                    k.within(f"fuse_gate_fwd rows={rows} mask={mm is not None} a={aa is not None} out={out is not None}", r.e, r.h, R,
                             2 * (t32.double() - R).abs() + ulp32(R), src)
                    if out is not None:
                        k.same("fuse_gate_fwd returns out", r.e, r.ea[5])
            r = k.call("fuse_gate_bwd", dy, s, a, alpha, gamma, mm)
            dm = dy.double() * m64
            Rds, Rda = alpha.double() * dy.double(), gamma.double() * dm
            k.within(f"fuse_gate_bwd rows={rows} mask={mm is not None} ds", r.e[0], r.h[0], Rds, 2 * ((alpha * dy).double() - Rds).abs() + ulp32(Rds), src)
            k.within(f"fuse_gate_bwd rows={rows} mask={mm is not None} da", r.e[1], r.h[1], Rda, 2 * ((gamma * (dy * m32)).double() - Rda).abs() + ulp32(Rda), src)
            t1, t2 = _ld(dm) * _ld(a), _ld(dy) * _ld(s)
            Rs = np.concatenate([t1.sum(0), t2.sum(0)])
            mass = np.concatenate([np.abs(t1).sum(0), np.abs(t2).sum(0)])
            k.within(f"fuse_gate_bwd rows={rows} mask={mm is not None} sums", r.e[2], r.h[2], torch.from_numpy(Rs.astype(np.float64)),
                     torch.from_numpy(((rows + 3) * U64 * mass).astype(np.float64)) + 1e-300, "derived: (rows + 3) eps64 sum|terms| (products, fp64 additions, R in fp64)")


@case("skip_stats", "skip_fold", "skip_merge", lp=True)
def case_skip(k):
    """Bounds: tests/test_gpu_skip.py - STATS_REL = 1e-12 of sum|x| for the fp64 sums, one fp32 ulp of the largest term for the
    merge (ULPS = 1)."""
    from tests import skip_restatement as SR
    for n in ROWS:
        g = gen(95 + n)
        c = 20
        x = torch.randn(n, c, generator=g) * 3 + 0.5
        mch = max(1, n // 3)
        child, cluster = torch.randn(mch, c, generator=g), torch.randint(0, mch, (n,), generator=g).int()
        ref = torch.randperm(n, generator=g).int()
        for xx in (x, x.to(k.T)):
            for rmap in (None, ref):
                r = k.call("skip_stats", xx, rmap)
                scale = xx.double().abs().sum(0).repeat(3)
                R = SR.stats(xx, rmap)
                k.within(f"skip_stats n={n} {xx.dtype} map={rmap is not None}", r.e, r.h, R, 1e-12 * scale, "test_kernels_vs_the_fp64_restatement: STATS_REL 1e-12 sum|x|")
        for rmap in (None, ref):
            st = SR.stats(x, rmap)
            for s_, f_, with_child, with_stats in ((0.8, 1.0, True, True), (0.9, 1.25, False, True), (1.0, 0.64, True, False)):
                r = k.call("skip_merge", x, st if with_stats else None, s_, f_, rmap, None, child if with_child else None, cluster if with_child else None)
                R = SR.merge(x, st if with_stats else None, s_, f_, rmap, None, child if with_child else None, cluster if with_child else None)
                mag = (abs(f_) * x.double().abs()).clamp(min=1e-30)
                if with_stats:
                    mag = torch.maximum(mag, abs(f_ * SR.k_of(s_, n)) * SR.wave(st, n, rmap).abs())
                if with_child:
                    mag = torch.maximum(mag, child.double()[cluster.long()].abs())
                k.within(f"skip_merge n={n} s={s_} f={f_} child={with_child} stats={with_stats} map={rmap is not None} (x in place)", r.ea[0], r.ha[0],
                         R.double(), ulp32(torch.maximum(mag, R.double().abs())), "test_kernels_vs_the_fp64_restatement: 1 ulp of the largest term")
            w = torch.randn(c, c, generator=g) / c ** 0.5
            r = k.call("skip_fold", w, st)
            Ru = (st.view(3, c) @ w.double().t()).reshape(-1)
            k.within(f"skip_fold n={n} map={rmap is not None}", r.e, r.h, Ru, 1e-12 * (x.double().abs().sum(0).repeat(3).view(3, c) @ w.double().abs().t()).reshape(-1),
                     "test_kernels_vs_the_fp64_restatement: STATS_REL")
            r = k.call("skip_merge", x, Ru, 0.8, 0.75, rmap, folded=True)
            R = SR.merge(x, Ru, 0.8, 0.75, rmap, folded=True)
            mag = torch.maximum(x.double().abs(), abs(0.75 * SR.k_of(0.8, n)) * SR.wave(Ru, n, rmap).abs())
            k.within(f"skip_merge folded n={n} map={rmap is not None}", r.ea[0], r.ha[0], R.double(), ulp32(torch.maximum(mag, R.double().abs())),
                     "test_kernels_vs_the_fp64_restatement: 1 ulp of the largest term")


# ------------------------------------------------------------------------------------------ steering predicates
WIDTHS = (16, 32, 48, 64, 96, 128, 256, 512, 528)
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
PRED_ROWS = (1, 64, 65, 20480, 65536)


def _outcome(fn, *args):
    """What a host-side call gives: its value, or the library's error (raised before any launch)."""
    from cdsegnet_amd._lib import CdsegError
    try:
        return tuple(fn(*args))
    except CdsegError:
        return "CdsegError"


@case("stem5_ok", "subm_conv3_ok", "block_rr_ok", "block_rr_head_on", "cpe_head_fused_ok", "attn_tail_fused_ok", "mlp_fused_ok", "pool_fused_ok", "bn_partition")
def case_predicates(k):
    """What picks the engine's arm: equal on widths x dtypes (x rows where rows are an argument).  Host code on either side; the
    predicates that take a tensor are given an empty-storage view of the shape (no predicate reads data)."""
    E, O = types.SimpleNamespace(**EMU_OF), k.ops
    n = 0
    for c in WIDTHS:
        assert E.block_rr_head_on(c) == O.block_rr_head_on(c), c
        for dt_ in DTYPES:
            assert E.is_lp(dt_) == O.is_lp(dt_)
            assert E.stem5_ok(c, dt_) == O.stem5_ok(c, dt_), (c, dt_)
            assert E.block_rr_ok(c, dt_) == O.block_rr_ok(c, dt_), (c, dt_)
            for cout in (c, 2 * c):
                assert E.pool_fused_ok(c, cout, dt_) == O.pool_fused_ok(c, cout, dt_), (c, cout, dt_)
            for rows in PRED_ROWS:
                t = torch.empty((rows, c), dtype=dt_, device="meta")
                assert E.subm_conv3_ok(t) == O.subm_conv3_ok(t), (rows, c, dt_)
                assert E.cpe_head_fused_ok(t) == O.cpe_head_fused_ok(t), (rows, c, dt_)
                for hidden in (4 * c, 2 * c):
                    assert E.attn_tail_fused_ok(t, hidden) == O.attn_tail_fused_ok(t, hidden), (rows, c, dt_, hidden)
                    assert E.mlp_fused_ok(t, hidden) == O.mlp_fused_ok(t, hidden), (rows, c, dt_, hidden)
                n += 1
        for rows in PRED_ROWS + (0, 255, 256, 257, 65537):
            assert _outcome(E.bn_partition, rows, c) == _outcome(O.bn_partition, rows, c), (rows, c)  # (528: no kernel, both raise)
    assert E.subm_conv3_ok(torch.empty((64, 64), dtype=torch.bfloat16, device="meta")[:, :32]) == \
        O.subm_conv3_ok(torch.empty((64, 64), dtype=torch.bfloat16, device="meta")[:, :32]) is False  # strided rows: the gathered GEMM
    print(f"[measure] emu-conformance predicates: {n} (width, dtype, rows) points, all equal")
    k.compared += 1


# ------------------------------------------------------------------------------------------ the native training Block
def _tb_inputs():
    """One C = 32 case of BLOCK_CASES (tests/test_gpu_train_block.py): 130 + 77 rows in two scenes, a distinct conv input, timestep
    rows."""
    from tests.test_gpu_train_block import BLOCK_CASES, _case
    C, H, rk, distinct, with_t, masks = next(c for c in BLOCK_CASES if c[0] == 32 and c[2] == "130+77" and c[3] and c[4])
    return (C, H, rk, distinct, with_t, masks), _case(C, H, rk, distinct, with_t, masks)


_ROWS_CASE = {}


def _tb_rows_case(cs, C, H):
    """A row level over that case's 207 voxels (engine.RowLevel's layout): the first 40 voxels of either scene hold two rows, every
    other voxel one; a slot plan of patch 64 over the 287 rows in a random order per scene; dropped-row masks.  With it the fp64
    torch-autograd restatement of tests/test_gpu_mix3d_rows.py (`_rows_case`: the CPE on the first row of every voxel, gathered
    to the rows) and the same in fp32, the yardstick of the three-times-torch rule."""
    if _ROWS_CASE:
        return _ROWS_CASE
    plan = cs["plan"]
    V, offs_v, B = plan["n"], plan["lv"].offs_host, plan["B"]
    rng = np.random.default_rng(287)
    counts = np.ones(V, dtype=np.int64)
    for b in range(B):
        counts[offs_v[b]:offs_v[b] + 40] = 2
    row_start = np.concatenate([[0], np.cumsum(counts)])
    n = int(row_start[-1])
    row_vox = np.repeat(np.arange(V), counts)
    offs_r = row_start[np.asarray(offs_v)]
    batch_r = np.repeat(np.arange(B), np.diff(offs_r))
    pad, unpad, cu = S.padding_plan(offs_r[1:], 64)
    perm = np.concatenate([offs_r[b] + rng.permutation(int(offs_r[b + 1] - offs_r[b])) for b in range(B)])
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    order, inverse = perm[pad], unpad[inv]
    widx = np.full(len(order), -1, dtype=np.int32)
    widx[inverse] = np.arange(n, dtype=np.int32)
    x_in, x_conv, dy = (rng.standard_normal((n, C)).astype(np.float32) for _ in range(3))
    t_rows = (0.5 * rng.standard_normal((B, C))).astype(np.float32)
    m1, m2 = ((rng.random(n) < 0.7).astype(np.float32) / np.float32(0.7) for _ in range(2))
    m1[0], m2[n - 1] = 0.0, 0.0
    from tests.test_gpu_train_block import NAMES18

    def grads(dt_):
        P = [torch.as_tensor(p).to(dt_).requires_grad_(True) for p in cs["params"]]
        xi, xc, tr = (torch.as_tensor(v).to(dt_).requires_grad_(True) for v in (x_in, x_conv, t_rows))
        ln = lambda v, i: F.layer_norm(v, (C,), P[i], P[i + 1], 1e-5)  # noqa: E731
        cpe_v = ln(F.linear(OM.subm_conv3d(xc[torch.as_tensor(row_start[:-1])], plan["nbr"], P[0], P[1]), P[2], P[3]), 4)
        x0 = xi + cpe_v[torch.as_tensor(row_vox)] + tr[torch.as_tensor(batch_r)]
        L3 = F.linear(ln(x0, 6), P[8], P[9])[torch.as_tensor(order)].reshape(-1, 3, C)
        feat = OM._patch_attention(L3[:, 0], L3[:, 1], L3[:, 2], np.asarray(cu), H, (C // H) ** -0.5)
        x1 = x0 + F.linear(feat[torch.as_tensor(inverse)], P[10], P[11]) * torch.as_tensor(m1).to(dt_)[:, None]
        y = x1 + F.linear(F.gelu(F.linear(ln(x1, 12), P[14], P[15])), P[16], P[17]) * torch.as_tensor(m2).to(dt_)[:, None]
        (y * torch.as_tensor(dy).to(dt_)).sum().backward()
        out = {"y": y.detach(), "dx_in": xi.grad, "dx_conv": xc.grad, "dt_rows": tr.grad}
        out.update({kk: p.grad for kk, p in zip(NAMES18, P)})
        return out
    _ROWS_CASE.update(n=n, rows=(torch.as_tensor(row_vox.astype(np.int32)), torch.as_tensor(row_start.astype(np.int32))),
                      offs=torch.as_tensor(offs_r.astype(np.int32)), gidx=torch.as_tensor(order.astype(np.int32)), widx=torch.as_tensor(widx),
                      cu=torch.as_tensor(np.asarray(cu, dtype=np.int32)), ins=dict(x_in=torch.as_tensor(x_in), x_conv=torch.as_tensor(x_conv),
                      t_rows=torch.as_tensor(t_rows), m1=torch.as_tensor(m1), m2=torch.as_tensor(m2), dy=torch.as_tensor(dy)),
                      ref=grads(torch.float64), t32=grads(torch.float32))
    assert bool((_ROWS_CASE["widx"] < 0).any())
    return _ROWS_CASE


@case("train_block_prepare", "train_block_forward", "train_block_backward", "train_block_grad_views", lp=True)
def case_train_block(k):
    """The native Block's four calls, emulation against library on one C = 32 case of BLOCK_CASES, in exact fp32 and with 16-bit
    products (the build's type).  The derived-weights buffer is opaque: compared through forward and backward.  Bound:
    test_whole_block_forward_and_backward_vs_fp64_within_three_times_autograd - (3 E_auto + eps) max|R| per tensor, E_auto the
    autograd mode's error on the device, measured here.  Then, in fp32, the same Block on a row level (`rows`): against the fp64
    restatement by the three-times-torch rule of tests/test_gpu_train_fp32.py, torch's fp32 autograd of the restatement the yardstick."""
    from tests.test_gpu_train_block import NAMES18, _run_block
    O = k.ops
    (C, H, rk, distinct, with_t, masks), cs = _tb_inputs()
    plan = cs["plan"]
    lv = plan["lv"]
    src = "test_whole_block_forward_and_backward_vs_fp64_within_three_times_autograd: (3 E_auto + eps) max|R|"
    cpu = lambda v: None if v is None else torch.as_tensor(v)  # noqa: E731
    for tp, variant, with_rows in (("fp32", None, False), ("fp32", None, True), ("bf16-amp" if k.lp == "bf16" else "fp16-amp", k.lp, False)):
        nbr = lv._nbr.cpu()
        if with_rows:
            rc = _tb_rows_case(cs, C, H)
            n, ins, gidx, widx, cu, offs, rows, ref = rc["n"], rc["ins"], rc["gidx"], rc["widx"], rc["cu"], rc["offs"], rc["rows"], rc["ref"]
        else:
            n, rows, ref = plan["n"], None, cs["ref"]
            auto, _ = _run_block(cs, C, H, tp, "autograd")
            ins = dict(x_in=cpu(cs["x_in"]), x_conv=cpu(cs["x_conv"]), t_rows=cpu(cs["t_rows"]), m1=cpu(cs["m1"]), m2=cpu(cs["m2"]), dy=cpu(cs["dy"]))
            gidx, widx, cu = lv._gidx.cpu(), lv._widx.cpu(), torch.as_tensor(lv._cu)
            offs = torch.tensor(lv.offs_host, dtype=torch.int32)
        psh = [int(v) for v in cu]
        rkw = lambda mv: {} if rows is None else dict(rows=tuple(mv(t) for t in rows))  # noqa: E731
        res = {}
        for side, mod, mv in (("emu", types.SimpleNamespace(**EMU_OF, TrainBlock=importlib.import_module("tests.emu_block_ops").TrainBlock), (lambda t: t)),
                              ("hip", O, (lambda t: None if t is None else t.cuda()))):
            params = [mv(torch.as_tensor(p).clone()) for p in cs["params"]]
            tb = mod.TrainBlock(params, H, (C // H) ** -0.5, (1e-5, 1e-5, 1e-5), variant, variant, False)
            mod.train_block_prepare(tb)
            nbytes = O.train_block_bytes(tb, n, psh[-1]) if side == "hip" else EMU_OF["train_block_bytes"](tb, n, psh[-1])
            tape, scratch, slab = (mv(torch.full((b,), 0x5A, dtype=torch.uint8)) for b in (nbytes[0], nbytes[1], nbytes[3]))
            a = [mv(t) for t in (ins["x_in"], ins["x_conv"], ins["t_rows"], offs, ins["m1"], ins["m2"], nbr, gidx, widx, cu)]
            x_out = mv(torch.full((n, C), 3.0))
            y = mod.train_block_forward(tb, n, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], psh, tape, scratch, x_out, **rkw(mv))
            assert y is x_out
            dx_in, dx_conv, dt_rows = mv(torch.full((n, C), 3.0)), mv(torch.full((n, C), 3.0)), mv(torch.full((2, C), 3.0))
            mod.train_block_backward(tb, n, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], psh, tape, scratch, None, mv(ins["dy"]),
                                     dx_in, dx_conv, dt_rows, slab, **rkw(mv))
            if side == "hip":
                torch.cuda.synchronize()
            grads = mod.train_block_grad_views(tb, slab)
            out = {"y": x_out, "dx_in": dx_in, "dx_conv": dx_conv, "dt_rows": dt_rows}
            out.update(dict(zip(NAMES18, grads)))
            res[side] = {kk: v.detach().cpu().clone() for kk, v in out.items()}
        assert set(res["emu"]) == set(res["hip"]) == set(ref)
        for tn, R in ref.items():
            top = float(R.abs().max())
            if with_rows:
                k.within(f"train_block {tp} rows {tn}", res["emu"][tn], res["hip"][tn], R, three_times_torch(rc["t32"][tn], R),
                         "tests/test_gpu_train_fp32.py _assert_vs_torch: (3 E_torch + eps) max|R|")
            else:
                e_auto = float((auto[tn].cpu().double() - R).abs().max()) / top
                k.within(f"train_block {tp} {tn}", res["emu"][tn], res["hip"][tn], R, (3 * e_auto + U) * top, src)


# ------------------------------------------------------------------------------------------ one test per (op group, build)
def _params():
    seen, out = {}, []
    for name in sorted(CASES):
        for fn, lp in CASES[name]:
            if fn not in seen:
                seen[fn] = True
                ops_of = sorted(n for n in CASES if any(f is fn for f, _ in CASES[n]))
                for v in (("bf16", "f16") if lp else ("bf16",)):
                    out.append(pytest.param(fn, v, ops_of, id=f"{fn.__name__[5:]}-{v}"))
    return out


@pytest.mark.parametrize("fn,lp,ops_of", _params())
def test_emulation_conforms_to_the_kernel(ops, fn, lp, ops_of):
    k = K(ops, lp, fn.__name__[5:])  # (ops_of: the emulated functions this case stands for, shown in the test id's report)
    fn(k)
    assert k.compared > 0, "the case compared nothing"
