"""GPU: guard bands and per-operand strides on the inference path (and the fp32x3 wide conv against fp64).

The rest of the suite compares what a kernel writes where it should write, on exact-size contiguous freshly allocated tensors
that all share one row stride.  Here every entry point is called a second time with
  * every output inside a tests/guard_bands.banded buffer (256 guard rows in front and behind, 8 guard columns on both sides),
  * every floating-point input inside a poisoned_input buffer (NaN guard rows and columns),
  * every index operand with guard entries that are valid for the call (-1 where the ABI defines "none", else a copy of the
    first / last entry),
  * a DIFFERENT row stride for every operand.
(a) "strided": strides that are multiples of 8 elements on 16-byte aligned bases - the kernel takes the same code path as the
    contiguous reference call, so the result is BIT-equal to it; all bands intact; inputs unchanged.
(b) the weakest layout the entry point's host checks admit ("ld4": strides % 4 only; "base8": an 8-byte aligned base where the
    host code admits one) - the kernel may take another path (cdseg_gemm leaves the one-store 16-bit epilogue for epilogue4 or
    the scalar epilogue), so the result is compared with the fp64 reference of the existing test of that operation under that
    test's own bound; all bands intact.
Each call is valid under the contract read from the entry point's host code (quoted in the docstrings); refusals are tested
through the return code with the outputs keeping their fill.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cdsegnet_amd import _lib
from oracle import model as OM
from oracle import serialization as S
from tests import guard_bands as GB
from tests.helpers import load_fixture
from tests.test_gpu_ops import LP, LPS, _library_variant, _physical, dev, ops, report  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

NAN = float("nan")
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "f16"])


def _r16(x):
    return x.to(LP()).to(torch.float32)


def _up(n, k):
    return -(-n // k) * k


class Mem:
    """The guarded operands of one call: bands of the outputs, poisoned inputs with their original bits, index guards."""

    def __init__(self):
        self.bands, self.inputs, self.index_checks = [], [], []

    def out(self, shape, dtype, *, ld=None, align=0, fill=NAN, name="out", cols=8):
        inner, band = GB.banded(shape, dtype, ld=ld, align=align, fill=fill, name=name, cols=cols)
        self.bands.append(band)
        return inner

    def inp(self, t, *, ld=None, align=0, name="in", inplace=False, cols=8):
        inner, band = GB.poisoned_input(t, ld=ld, align=align, name=name, cols=cols)
        self.bands.append(band)
        if not inplace:
            self.inputs.append((inner, t.clone(), name))
        return inner

    def index(self, idx, none=None):
        inner, chk = GB.guard_index(idx, none=none)
        self.index_checks.append(chk)
        return inner

    def check(self):
        torch.cuda.synchronize()
        for b in self.bands:
            b.check()
        for inner, orig, name in self.inputs:
            assert GB.same_bits(inner, orig), f"input {name} was written"
        for chk in self.index_checks:
            chk()


def _lds(width, dtype, layout, slot):
    """Row stride of operand number `slot` (every operand of a call gets another one).  strided: multiples of 8 elements;
    ld4: multiples of 4 that are no multiples of 8 (8-byte aligned 16-bit rows, 16-byte aligned fp32 rows)."""
    base = _up(width, 8) + 16 + 8 * slot
    return base if layout == "strided" else base + 4


# ====================================================================================================== cdseg_gemm
# launch_bn (csrc/gemm.hip) picks the kernel; the conditions quoted in the ids and docstrings below are its own.
def _gemm_tensors(M, N, K, dtype, form, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    A, W = r(M, K), r(N, K) / K ** 0.5
    if dtype != torch.float32:
        A, W = A.to(dtype).float(), W.to(dtype).float()
    Mc = max(1, M // 3)
    t = dict(A=A, W=W, bias=r(N), scale=torch.rand(N, generator=g) + 0.5, shift=r(N), add_src=r(Mc, N),
             add_idx=torch.randint(0, Mc, (M,), generator=g).int(), x0=r(M, N), colbias=r(N), g1=r(N), b1=r(N), g2=r(N), b2=r(N))
    perm = torch.randperm(M, generator=g).int()
    if form == "logit-skip":
        perm[torch.rand(M, generator=g) < 0.3] = -1
        perm[0] = -1
    t["out_idx"] = perm
    return t


def _gemm_ref64(t, form, N):
    """fp64 restatement of the epilogue of each engine call site -> dict of expected outputs."""
    y = t["A"].double() @ t["W"].double().t() + t["bias"].double()
    if form == "plain":
        return dict(out=F.gelu((y * t["scale"].double() + t["shift"].double()).float()).double())
    if form == "unpool":
        pre = F.gelu((y * t["scale"].double() + t["shift"].double()).float()).double()
        return dict(out=pre + t["add_src"].double()[t["add_idx"].long()], out2=pre)
    if form == "cat":
        return dict(out=y + t["add_src"].double()[t["add_idx"].long()])
    if form == "cpe":
        x = t["x0"] + F.layer_norm(y.float(), (N,), t["g1"], t["b1"], 1e-5) + t["colbias"]
        return dict(out=x.double(), ln_out=F.layer_norm(x, (N,), t["g2"], t["b2"], 1e-5).double())
    return dict(out=y)  # logit head: rows scattered by out_idx, compared after the scatter


def _gemm_call(ops, t, form, dtype, layout):
    """One cdseg_gemm of `form`; layout None = the reference call: exact-size contiguous operands, as everywhere else in the
    suite (its outputs are contiguous rows between guard rows, so its bands are checked too).  -> (outputs, Mem)."""
    M, K = t["A"].shape
    N = t["W"].shape[0]
    lp_out = dtype  # 16-bit builds write 16-bit second outputs / LayerNorm outputs; the fp32 build fp32 ones
    mem = Mem()
    lay = "strided" if layout == "strided" else "ld4"
    al = 8 if layout == "base8" else 0

    def O(shape, dt, slot, name, fill=NAN):
        if layout is None:
            return mem.out(shape, dt, cols=0, fill=fill, name=name)
        return mem.out(shape, dt, ld=_lds(shape[1], dt, lay, slot), align=al, fill=fill, name=name)

    def I(x, dt, slot, name, inplace=False, align=0):
        x = dev(x, dt)
        if layout is None:
            return x
        # (A: `lda * element size` must be a multiple of 16 bytes, so a 16-bit A keeps strides % 8 in every layout)
        return mem.inp(x, ld=_lds(x.shape[1], dt, "strided" if dt != torch.float32 and name == "A" else lay, slot), align=align, name=name,
                       inplace=inplace)

    def X(idx, none=None):
        return dev(idx) if layout is None else mem.index(dev(idx), none=none)

    A = I(t["A"], dtype, 0, "A")  # (lda * element size must be a multiple of 16: `((long)a->lda * esz) & 15`)
    W = dev(t["W"], dtype)
    vec = lambda k: dev(t[k])  # noqa: E731
    outs = {}
    if form == "plain":
        out = O((M, N), dtype, 1, "out")
        ops.gemm(A, W, out, bias=vec("bias"), scale=vec("scale"), shift=vec("shift"), act=ops.ACT_GELU, cache=False)
        outs["out"] = out
    elif form == "unpool":
        out, out2 = O((M, N), torch.float32, 1, "out"), O((M, N), lp_out, 2, "out2")
        ops.gemm(A, W, out, bias=vec("bias"), scale=vec("scale"), shift=vec("shift"), act=ops.ACT_GELU,
                 add_src=I(t["add_src"], torch.float32, 3, "add_src", align=al), add_idx=X(t["add_idx"]), out2=out2, out2_pre_add=True,
                 cache=False)
        outs.update(out=out, out2=out2)
    elif form == "cat":
        out = O((M, N), torch.float32, 1, "out")
        ops.gemm(A, W, out, bias=vec("bias"), add_src=I(t["add_src"], torch.float32, 3, "add_src", align=al), add_idx=X(t["add_idx"]),
                 cache=False)
        outs["out"] = out
    elif form == "cpe":
        x = I(t["x0"], torch.float32, 1, "x", inplace=True)
        h = O((M, N), lp_out, 4, "ln_out")
        ops.gemm(A, W, x, bias=vec("bias"), ln_pre=(vec("g1"), vec("b1")), res=x, colbias=vec("colbias"),
                 ln_post=(vec("g2"), vec("b2")), ln_out=h, cache=False)
        outs.update(out=x, ln_out=h)
    else:  # logit head
        out = O((M, N), torch.float32, 1, "out", fill=-777.25)
        ops.gemm(A, W, out, bias=vec("bias"), out_idx=X(t["out_idx"], none=-1), cache=False)
        outs["out"] = out
    mem.check()
    return {k: v.clone() for k, v in outs.items()}, mem


def _gemm_bounds(form, dtype, K, ref):
    """The bounds of the existing tests of each product (tests/test_gpu_ops.py), per output."""
    lp_tol = lambda r: (1e-4 if dtype == torch.float32 else 0.03) * (1 + r.abs().max().item())  # noqa: E731
    # fp32 output behind folded BN + GELU: 5e-4 (test_gemm_epilogue_bn_gather_add_scatter, K = 128); for the long reductions
    # of the split-K cases test_gemm_split_k's 2e-5 sqrt(K) + 1e-4 with the product term times the largest |scale| here (1.5;
    # GELU' <= 1.13 is covered by the rounding of 1.5 * 1.13 = 1.7 up to 2)
    f32_tol = max(5e-4, 2 * 2e-5 * K ** 0.5 + 1e-4)
    if form == "plain":
        return dict(out=f32_tol if dtype == torch.float32 else lp_tol(ref["out"]))
    if form == "unpool":
        return dict(out=f32_tol, out2=lp_tol(ref["out2"]))
    if form == "cat":  # test_gemm_plain with a residual
        return dict(out=2e-5 * K ** 0.5 + 1e-4)
    if form == "cpe":  # test_gemm_fused_layernorm_epilogue
        return dict(out=2e-4 + 2e-5 * K ** 0.5, ln_out=(2e-4 if dtype == torch.float32 else 0.03) * (1 + ref["ln_out"].abs().max().item()))
    return dict(out=2e-5 * K ** 0.5 + 1e-5)  # test_gemm_plain


# (id, M, N, K, form): the id names the path for the 16-bit builds and the condition of launch_bn that selects it
GEMM_CASES = [
    ("gemm_kernel-bn32[N<=32]-tile+1", 65, 32, 128, "unpool"),
    ("gemm_kernel-bn32[N<=32]-one-row", 1, 32, 128, "unpool"),
    ("gemm_kernel-bn64[N<=64]-tile+1", 65, 64, 128, "cat"),
    ("gemm_kernel-bn64[N<=64]-one-row", 1, 64, 128, "cat"),
    ("gemm_kernel-bn128[N>64,K%64!=0]-one-store-epilogue-tile+1", 65, 128, 72, "plain"),
    ("gemm_kernel-bn128[N>64,K%64!=0]-one-store-epilogue-one-row", 1, 128, 72, "plain"),
    ("narrow-K[kvol*K<=64]-tile+1", 65, 64, 32, "unpool"),
    ("narrow-K[kvol*K<=64]-one-store-epilogue-one-row", 1, 96, 64, "plain"),
    ("gemm_kernel[M<128]-below-the-dma-row-count", 127, 128, 128, "plain"),
    ("gemm_dma_kernel<64>[16-bit,N>64,K%64==0,M>=128]-one-store-epilogue", 128, 128, 128, "plain"),
    ("gemm_dma_kernel<64>[16-bit,N>64,K%64==0,M>=128]-tile+1-unpool", 129, 128, 128, "unpool"),
    ("gemm_dma_kernel<64>[M<16384]-below-the-128-row-switch", 16383, 128, 128, "plain"),
    ("gemm_dma_kernel<128>[M>=16384]-tile+1", 16385, 128, 128, "plain"),
    ("gemm_dma_kernel<64>[N>=1024,M<2048]", 2047, 1024, 128, "plain"),
    ("gemm_dma_kernel<128>[N>=1024&&M>=2048]-tile+1", 2049, 1024, 128, "unpool"),
    ("split-K[blocks<256,nkc>=16]-splitk_epilogue_kernel-plain", 100, 128, 4096, "plain"),
    ("split-K[blocks<256,nkc>=16]-splitk_epilogue_kernel-unpool", 65, 64, 4096, "unpool"),
    ("layernorm-in-block[N<=128]-bn64-tile+1", 65, 64, 128, "cpe"),
    ("layernorm-in-block[N<=128]-bn128-one-row", 1, 128, 128, "cpe"),
    ("layernorm-row_finish_kernel[N=256]-tile+1", 65, 256, 128, "cpe"),
    ("layernorm-row_finish_kernel[N=512]-one-row", 1, 512, 128, "cpe"),
    ("layernorm-row_finish_kernel[N=512]-dma-rows", 130, 512, 128, "cpe"),
    ("logit-head[N=13:N%4!=0]-scalar-epilogue", 65, 13, 64, "logit"),
    ("logit-head[N=20]-epilogue4-scatter", 65, 20, 64, "logit"),
    ("logit-head[N=13]-skip-rows", 130, 13, 64, "logit-skip"),
    ("logit-head[N=20]-skip-rows", 1, 20, 64, "logit-skip"),
]


@DTYPES
@pytest.mark.parametrize("name,M,N,K,form", GEMM_CASES, ids=[c[0] for c in GEMM_CASES])
def test_gemm_guard_bands_and_per_operand_strides(ops, dtype, name, M, N, K, form):
    """cdseg_gemm's dispatch (launch_bn / launch, csrc/gemm.hip), one case per path, each with the epilogue of an engine call
    site and all of that epilogue's operands present at once, every one on its own stride:
      bm: 64 rows; `tall = GATHER && NCH == 16 && M > 64` 128 rows; the 16-bit LDS-DMA loop when `N > 64 && K % 64 == 0 && M >= 128`
          with `want = (GATHER || M >= 16384 || (N >= 1024 && M >= 2048)) ? 128 : 64`, but `if (ln && N <= 128) want = -1`;
      bn: `N <= 32 ? 32 : (N <= 64 ? 64 : 128)`;  narrow K step: `ktot <= 64` (launch);
      split-K: `can_fix && blocks < 256 && nkc >= 16` -> p.fix = 1 (splitk_epilogue_kernel) or, with a LayerNorm, 2;
      LayerNorm: finished in the block when `gn == 1 && splits == 1` (N <= 128), else `p.fix = 2` (row_finish_kernel, N <= 512);
      epilogue: plain_bf16_out (16-bit output, vec_ok, no second operand, `N % 8 == 0 && ldo % 8 == 0`) -> epilogue8_bf16, one
          16-byte store and the polynomial GELU; else epilogue4 (8-byte stores of 16-bit values, gelu_erf), scalar when !vec_ok
          (`N % 4`, a stride % 4, or a base that is not 16-byte aligned).
    Row counts: one full tile plus one row, one row, and the smallest count on each side of a row threshold.
    strided == the contiguous call bit for bit; ld4 / base8 against fp64 under the existing tests' bounds.  Rows whose out_idx
    is -1 keep their fill (epilogue4: `if (orow < 0) return`)."""
    t = _gemm_tensors(M, N, K, dtype, form, M + 3 * N + 7 * K)
    ref64 = _gemm_ref64(t, form, N)
    bounds = _gemm_bounds(form, dtype, K, ref64)
    base, _ = _gemm_call(ops, t, form, dtype, None)
    layouts = ["strided", "ld4"] + ([] if form == "cpe" else ["base8"])  # (LayerNorm: `!p.vec_ok -> CDSEG_ERR_UNSUPPORTED`)
    idx = t["out_idx"].long()
    for layout in [None] + layouts:
        got = base if layout is None else _gemm_call(ops, t, form, dtype, layout)[0]
        if layout == "strided":
            for k in base:
                assert GB.same_bits(got[k], base[k]), f"{k}: the strided call differs from the contiguous one"
        for k, want in ref64.items():
            g = got[k].double().cpu()
            if form.startswith("logit"):
                live = idx >= 0
                dead = torch.ones(M, dtype=torch.bool)
                dead[idx[live]] = False
                assert bool((g[dead] == -777.25).all()), f"{layout}: a row that no out_idx entry names was written"
                g, want = g[idx[live]], want[live]
            err = (g - want).abs().max().item() if g.numel() else 0.0
            report(f"gemm {name} {dtype} {layout or 'contiguous'} {k}", max_err=err, bound=bounds[k])
            assert err < bounds[k], (layout, k, err)


@DTYPES
@pytest.mark.parametrize("C,n", [(128, 300), (256, 64), (256, 65), (256, 511), (256, 513)])
def test_gathered_gemm_guard_bands_and_minus_one_neighbours_read_no_row(ops, dtype, C, n):
    """The sparse-conv form (nbr, kvol = 27, offset-major map): `tall = GATHER && NCH == 16 && M > 64` (n = 64 / 65), the
    16-bit LDS-DMA loop on 128-row tiles from `M >= 128` with `want = GATHER ? 128`, `deep = tall && 16-bit && N >= 256 &&
    M >= 512` (n = 511 / 513), split-K through ops.gemm's workspace.  A sits between NaN rows: a -1 neighbour that read row -1
    (or any row past the end) would put a NaN into the result.  Reference: fp32 torch gather + matmul per offset on the same
    operands, the bound of test_deep_conv_group_skipping_random_map (fp32 output: 2e-4)."""
    g = torch.Generator().manual_seed(n + C)
    row_on = torch.rand(27, n, generator=g) > 0.5
    row_on[3] = False
    row_on[13] = True
    nbr = torch.where(row_on, torch.randint(0, n, (27, n), generator=g), torch.full((27, n), -1)).int()
    x, w, b = torch.randn(n, C, generator=g), torch.randn(C, 27, C, generator=g) / (13 * C) ** 0.5, torch.randn(C, generator=g)
    if dtype != torch.float32:
        x, w = x.to(dtype).float(), w.to(dtype).float()
    ref = b.double().repeat(n, 1)
    for o in range(27):
        idx = nbr[o].long()
        ref += torch.where((idx >= 0)[:, None], x.double()[idx.clamp(min=0)], torch.zeros((), dtype=torch.float64)) @ w[:, o, :].double().t()
    wd, bd = dev(w.reshape(C, -1), dtype), dev(b)
    base = torch.full((n, C), NAN, device="cuda")
    ops.gemm(dev(x, dtype), wd, base, bias=bd, nbr=dev(nbr), nbr_kmajor=True, kvol=27, cache=False)
    mem = Mem()
    out = mem.out((n, C), torch.float32, ld=C + 24)
    ops.gemm(mem.inp(dev(x, dtype), ld=C + 16, name="A"), wd, out, bias=bd, nbr=mem.index(dev(nbr), none=-1), nbr_kmajor=True, kvol=27,
             cache=False)
    mem.check()
    assert bool(torch.isfinite(out).all()), "a -1 neighbour (or an over-read) reached a guard row of A"
    assert GB.same_bits(out, base)
    err = (out.cpu().double() - ref).abs().max().item()
    assert err < 2e-4, err


# ====================================================================================================== elementwise kernels
def _ln_raw(ops, x, gamma, beta, out, res=None, colbias=None, out2=None):
    return _lib.load().cdseg_layernorm(ops._ptr(x), ops.dt(x), x.stride(0), ops._ptr(gamma), ops._ptr(beta), 1e-5, ops._ptr(res),
                                       res.stride(0) if res is not None else 0, ops._ptr(colbias), ops._ptr(out), ops.dt(out),
                                       out.stride(0), ops._ptr(out2), ops.dt(out2) if out2 is not None else 0,
                                       out2.stride(0) if out2 is not None else 0, x.shape[0], x.shape[1], ops._stream())


@LPS
@pytest.mark.parametrize("xkind", ["x-fp32", "x-16bit"])
@pytest.mark.parametrize("M", [65, 1])
@pytest.mark.parametrize("C", [16, 48, 512, 2048])
def test_layernorm_guard_bands_and_per_operand_strides(ops, lp, C, M, xkind):
    """cdseg_layernorm with res, colbias and out2 together.  TPR = the power of two >= C / 4 (<= 64) lanes share a row, a
    256-thread block holds 4 * 64 / TPR rows (64 rows at C = 16, 4 rows at C >= 256): M = 65 is full blocks plus one row at
    every width, M = 1 one row.  Host checks: `c % 4`, every `ld % 4`, x / out / out2 16-byte aligned as fp32 and 8-byte aligned
    as the 16-bit type.  ld4 + base8: 16-bit x and out2 on 8-byte aligned bases with strides % 4.  fp64 bound: test_layernorm's
    (2e-5 for fp32 x, 0.02 (1 + max) for 16-bit values)."""
    g = torch.Generator().manual_seed(C + M)
    xdt = torch.float32 if xkind == "x-fp32" else LP()
    x = torch.randn(M, C, generator=g) * 3 + 1
    if xdt != torch.float32:
        x = _r16(x)
    gm, bt, res, cb = torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(M, C, generator=g), torch.randn(C, generator=g)
    ref = (F.layer_norm(x.double(), (C,), gm.double(), bt.double(), 1e-5) + res.double() + cb.double())
    base, base2 = torch.full((M, C), NAN, device="cuda"), torch.full((M, C), NAN, dtype=LP(), device="cuda")
    ops.layernorm(dev(x, xdt), dev(gm), dev(bt), base, res=dev(res), colbias=dev(cb), out2=base2)
    for layout in ("strided", "weak"):
        lay = "strided" if layout == "strided" else "ld4"
        al16bit = 0 if layout == "strided" else 8
        mem = Mem()
        xi = mem.inp(dev(x, xdt), ld=_lds(C, xdt, lay, 0), align=al16bit if xdt != torch.float32 else 0, name="x")
        ri = mem.inp(dev(res), ld=_lds(C, torch.float32, lay, 1), name="res")
        out = mem.out((M, C), torch.float32, ld=_lds(C, torch.float32, lay, 2))
        out2 = mem.out((M, C), LP(), ld=_lds(C, LP(), lay, 3), align=al16bit, name="out2")
        ops.layernorm(xi, dev(gm), dev(bt), out, res=ri, colbias=dev(cb), out2=out2)
        mem.check()
        if layout == "strided":
            assert GB.same_bits(out, base) and GB.same_bits(out2, base2)
        err = (out.cpu().double() - ref).abs().max().item()
        err2 = (out2.float().cpu().double() - ref).abs().max().item()
        assert err < 2e-5, (layout, err)
        assert err2 < 0.02 * (1 + ref.abs().max().item()), (layout, err2)
    # in place on the residual (res == out), as the CPE chain calls it
    mem = Mem()
    xr = mem.inp(dev(res), ld=_lds(C, torch.float32, "strided", 1), name="res/out", inplace=True)
    ops.layernorm(mem.inp(dev(x, xdt), ld=_lds(C, xdt, "strided", 0), name="x"), dev(gm), dev(bt), xr, res=xr, colbias=dev(cb))
    mem.check()
    assert GB.same_bits(xr, base)


@LPS
def test_layernorm_and_segment_max_refuse_bases_their_vector_accesses_cannot_take(ops, lp):
    """The preconditions stated in include/cdseg.h, through the return code, with every output keeping its fill: an fp32
    operand that is not 16-byte aligned, a 16-bit operand that is not 8-byte aligned (the kernels load and store groups of
    four elements)."""
    M, C = 5, 16
    x, gm, bt = torch.randn(M, C, device="cuda"), torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    wide = torch.full((M, C + 8), -5.0, device="cuda")
    wide16 = torch.full((M, C + 8), -5.0, dtype=LP(), device="cuda")
    good = wide[:, 4:4 + C]
    for what, kw in (("fp32 out at +4 bytes", dict(out=wide[:, 1:1 + C])), ("fp32 out at +8 bytes", dict(out=wide[:, 2:2 + C])),
                     ("16-bit out2 at +4 bytes", dict(out=good, out2=wide16[:, 2:2 + C])),
                     ("fp32 res at +8 bytes", dict(out=good, res=wide[:, 2:2 + C])),
                     ("gamma at +4 bytes", dict(out=good, gamma=torch.ones(C + 1, device="cuda")[1:]))):
        rc = _ln_raw(ops, x, kw.get("gamma", gm), bt, kw["out"], res=kw.get("res"), out2=kw.get("out2"))
        torch.cuda.synchronize()
        assert _lib.ERRORS.get(rc) == "CDSEG_ERR_ARG", (what, rc)
        assert bool((wide == -5.0).all()) and bool((wide16 == -5.0).all()), what
    x16 = torch.full((M + 1, C), 1.0, dtype=LP(), device="cuda").view(-1)[2:2 + M * C].view(M, C)  # a 16-bit x at +4 bytes
    assert _lib.ERRORS.get(_ln_raw(ops, x16, gm, bt, good)) == "CDSEG_ERR_ARG"
    assert _ln_raw(ops, x, gm, bt, good) == 0  # the aligned call runs
    torch.cuda.synchronize()
    assert bool(torch.isfinite(good).all()) and bool((wide[:, :4] == -5.0).all()) and bool((wide[:, 4 + C:] == -5.0).all())
    # segment_max
    wide.fill_(-5.0)
    seg = torch.tensor([0, 2, 5], dtype=torch.int32, device="cuda")
    lib = _lib.load()

    def smax(y, out, out2=None, scale=None, shift=None):
        rc = lib.cdseg_segment_max(ops._ptr(y), ops.dt(y), y.stride(0), ops._ptr(seg), 2, C, ops._ptr(scale), ops._ptr(shift), 0,
                                   ops._ptr(out), out.stride(0), ops._ptr(out2), ops.dt(out2) if out2 is not None else 0,
                                   out2.stride(0) if out2 is not None else 0, ops._stream())
        torch.cuda.synchronize()
        return _lib.ERRORS.get(rc, rc)

    assert smax(x, wide[:2, 2:2 + C]) == "CDSEG_ERR_ARG" and smax(x, wide[:2, 1:1 + C]) == "CDSEG_ERR_ARG"
    assert smax(x, wide[:2, 4:4 + C], out2=wide16[:2, 2:2 + C]) == "CDSEG_ERR_ARG"
    assert smax(x16, wide[:2, 4:4 + C]) == "CDSEG_ERR_ARG"
    off = torch.ones(C + 1, device="cuda")[1:]
    assert smax(x, wide[:2, 4:4 + C], scale=off, shift=bt) == "CDSEG_ERR_ARG"
    assert bool((wide == -5.0).all()) and bool((wide16 == -5.0).all())
    assert smax(x, wide[:2, 4:4 + C], scale=gm, shift=bt) == 0
    assert torch.equal(wide[:2, 4:4 + C], torch.stack([x[:2].max(0).values, x[2:5].max(0).values]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["y-fp32", "y-bf16", "y-f16"])
@pytest.mark.parametrize("m", [1, 37])
@pytest.mark.parametrize("C", [64, 256, 512])
def test_segment_max_guard_bands_and_per_operand_strides(ops, dtype, C, m):
    """cdseg_segment_max at the widths the deep poolings run it at (one thread per (run, group of 4 columns), grid-stride,
    256-thread blocks: m = 37 is no multiple of a block at any width): runs of 1 to 8 rows and one run of 70, negative scales
    (the maximum comes first), fp32 and 16-bit y, out2 in the build's 16-bit type.  seg_start is an index operand: its guard
    entries repeat the first / last offset.  fp64 bound: test_segment_max_and_mean's (1e-5; 0.01 (1 + max) for out2)."""
    g = torch.Generator().manual_seed(C + m)
    counts = torch.randint(1, 9, (m,), generator=g)
    counts[m // 2] = 70
    seg = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(counts, 0)]).int()
    n = int(seg[-1])
    y = torch.randn(n, C, generator=g)
    if dtype != torch.float32:
        y = _r16(y)
    sc, sh = torch.randn(C, generator=g), torch.randn(C, generator=g)
    cluster = np.repeat(np.arange(m), counts.numpy())
    ref = F.gelu(OM.segment_max(y, cluster, m) * sc + sh)
    base, base2 = torch.full((m, C), NAN, device="cuda"), torch.full((m, C), NAN, dtype=LP(), device="cuda")
    ops.segment_max(dev(y, dtype), dev(seg), m, dev(sc), dev(sh), ops.ACT_GELU, base, base2)
    for layout in ("strided", "weak"):
        lay = "strided" if layout == "strided" else "ld4"
        a16 = 0 if layout == "strided" else 8
        mem = Mem()
        yi = mem.inp(dev(y, dtype), ld=_lds(C, dtype, lay, 0), align=a16 if dtype != torch.float32 else 0, name="y")
        out = mem.out((m, C), torch.float32, ld=_lds(C, torch.float32, lay, 1))
        out2 = mem.out((m, C), LP(), ld=_lds(C, LP(), lay, 2), align=a16, name="out2")
        ops.segment_max(yi, mem.index(dev(seg)), m, dev(sc), dev(sh), ops.ACT_GELU, out, out2)
        mem.check()
        if layout == "strided":
            assert GB.same_bits(out, base) and GB.same_bits(out2, base2)
        assert (out.cpu() - ref).abs().max().item() < 1e-5
        assert (out2.float().cpu() - ref).abs().max().item() < 0.01 * (1 + ref.abs().max().item())


@pytest.mark.parametrize("m", [1, 300])
def test_segment_mean_c3_guard_bands_and_strides(ops, m):
    """cdseg_segment_mean at C = 3 (the pooled coordinates): scalar accesses, no alignment asked of anything; x (n, 3) inside
    5-wide NaN-guarded rows, out (m, 3) inside 7-wide rows.  Bound of test_segment_max_and_mean: 1e-5."""
    g = torch.Generator().manual_seed(m)
    counts = torch.randint(1, 9, (m,), generator=g)
    seg = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(counts, 0)]).int()
    n = int(seg[-1])
    xyz = torch.randn(n, 3, generator=g)
    base = ops.segment_mean(dev(xyz), dev(seg), m)
    mem = Mem()
    xi = mem.inp(dev(xyz), ld=8 + 3 + 8 + 2, name="x")
    out = mem.out((m, 3), torch.float32, ld=8 + 3 + 8 + 4)
    ops.check(_lib.load().cdseg_segment_mean(ops._ptr(xi), xi.stride(0), ops._ptr(mem.index(dev(seg))), m, 3, ops._ptr(out), out.stride(0),
                                             ops._stream()), "segment_mean")
    mem.check()
    assert GB.same_bits(out, base)
    cluster = np.repeat(np.arange(m), counts.numpy())
    assert (out.cpu() - OM.segment_mean(xyz, cluster, m)).abs().max().item() < 1e-5


# ====================================================================================================== row movers
ROWS = pytest.mark.parametrize("n", [1, 333])


@ROWS
def test_gather_rows_and_scatter_rows_against_torch_indexing(ops, n):
    """cdseg_gather_rows (idx < 0 gathers a zero row) and cdseg_scatter_rows (idx < 0 skips the row: `if (d >= 0) dst[d] = src[i]`,
    include/cdseg.h "idx < 0 gathers zeros / skips") bit for bit against torch's index assignment; rows of 4 and of 28 bytes; the
    destinations sit between guard rows (the ABI knows no row stride here: rows are contiguous)."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(n)
    for cols in (1, 7):
        nsrc = 500
        src = torch.randn(nsrc, cols, generator=g).cuda()
        idx = torch.randint(0, nsrc, (n,), generator=g).int()
        idx[::5] = -1
        mem = Mem()
        dst = mem.out((n, cols), torch.float32, cols=0)
        ops.check(lib.cdseg_gather_rows(ops._ptr(src), ops._ptr(mem.index(idx.cuda(), none=-1)), n, 4 * cols, ops._ptr(dst), ops._stream()),
                  "gather_rows")
        mem.check()
        want = torch.where((idx >= 0)[:, None], src.cpu()[idx.clamp(min=0).long()], torch.zeros(()))
        assert GB.same_bits(dst.cpu(), want)
        # scatter: n source rows into a destination of nd rows through a partial permutation
        nd = n + 50
        rows = torch.randn(n, cols, generator=g).cuda()
        perm = torch.randperm(nd, generator=g)[:n].int()
        perm[::3] = -1
        mem = Mem()
        dst = mem.out((nd, cols), torch.float32, cols=0, fill=-777.25)
        got = ops.scatter_rows(rows, mem.index(perm.cuda(), none=-1), dst)
        mem.check()
        want = torch.full((nd, cols), -777.25)
        live = perm >= 0
        want[perm[live].long()] = rows.cpu()[live]
        assert got is dst and GB.same_bits(dst.cpu(), want)


@LPS
@ROWS
def test_gather_pad_cast_and_cast_guard_bands(ops, lp, n):
    """cdseg_gather_pad_cast (src with its own row stride, 6 -> 8 columns, identity and gathered) and cdseg_cast (fp32 -> 16-bit
    and back) write n x cpad / n elements and nothing else; bit-equal to the wrappers' fresh allocations."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(n + 1)
    src = torch.randn(400, 6, generator=g).cuda()
    idx = torch.randint(0, 400, (n,), generator=g).int().cuda()
    for dt in (LP(), torch.float32):
        for ix in (idx, None):
            rows = n if ix is not None else 400
            want = ops.gather_pad_cast(src, ix, 8, dt)
            mem = Mem()
            si = mem.inp(src, ld=8 + 6 + 8 + 3, name="src")
            out = mem.out((rows, 8), dt, cols=0)
            ops.check(lib.cdseg_gather_pad_cast(ops._ptr(si), si.stride(0), ops._ptr(None if ix is None else mem.index(ix)), rows, 6, 8,
                                                ops._ptr(out), ops.dt(out), ops._stream()), "gather_pad_cast")
            mem.check()
            assert GB.same_bits(out, want)
            assert torch.equal(out[:, :6].float(), src[ix.long() if ix is not None else slice(None)].to(dt).float())
    x = torch.randn(n, 7, generator=g).cuda()
    for a, b in ((torch.float32, LP()), (LP(), torch.float32)):
        xa = x.to(a)
        mem = Mem()
        si = mem.inp(xa.view(1, -1), name="src").view(-1)
        out = mem.out((1, n * 7), b)
        ops.check(lib.cdseg_cast(ops._ptr(si), ops.dt(xa), ops._ptr(out), ops.dt(out), n * 7, ops._stream()), "cast")
        mem.check()
        assert GB.same_bits(out.view(n, 7), ops.cast(xa, b)) and GB.same_bits(out.view(n, 7), xa.to(b))


@ROWS
def test_softmax_vote_and_argmax_rows_guard_bands(ops, n):
    """cdseg_softmax_vote (one wave per row, pred[idx[i]] += softmax(logits[i])) and cdseg_argmax_rows, logits / pred with
    their own row strides and c = 13 / 20 / 200 classes.  The vote against fp64 softmax under test_softmax_vote_and_argmax's
    bound (2e-6); the arg-max against torch's on rows without ties."""
    g = torch.Generator().manual_seed(n + 2)
    for c in (13, 20, 200):
        logits = torch.randn(n, c, generator=g) * 4
        npred = n + 17
        idx = torch.randperm(npred, generator=g)[:n].int()
        base = torch.zeros(npred, c, device="cuda")
        ops.softmax_vote(dev(logits), dev(idx), base)
        mem = Mem()
        li = mem.inp(dev(logits), ld=8 + c + 8 + 1, name="logits")
        pred = mem.out((npred, c), torch.float32, ld=8 + c + 8 + 3, name="pred")
        pred.zero_()
        ops.softmax_vote(li, mem.index(dev(idx)), pred)
        mem.check()
        assert GB.same_bits(pred, base)
        want = torch.zeros(npred, c, dtype=torch.float64)
        want[idx.long()] = torch.softmax(logits.double(), 1)
        assert (pred.cpu().double() - want).abs().max().item() < 2e-6
        mem = Mem()
        am = mem.out((1, n), torch.int32, fill=-9, name="argmax")
        ops.check(_lib.load().cdseg_argmax_rows(ops._ptr(li), li.stride(0), n, c, ops._ptr(am), ops._stream()), "argmax_rows")
        mem.check()
        assert torch.equal(am.view(-1).cpu().long(), logits.argmax(1))


# ====================================================================================================== cdseg_split16 (fp32x3)
def _split_restatement(x, T, lo_scale=2048.0):
    """hi = T(x), lo = T((x - hi) * 2048) in torch; T saturates at +-65504 in the half build (pack_bf16x2 there: v_med3 before
    the conversion), and is torch's round-to-nearest-even cast in the bfloat16 build."""
    sat = (lambda v: v.clamp(-65504.0, 65504.0)) if T == torch.float16 else (lambda v: v)
    hi = sat(x).to(T)
    lo = sat((x - hi.float()) * lo_scale).to(T)
    return hi, lo


@LPS
@pytest.mark.parametrize("rows", [1, 333])
def test_split16_equals_its_restatement_bit_for_bit_and_recombines_to_2p_bits(ops, lp, rows):
    """cdseg_split16: bit-equal to the torch restatement on inputs that include values beyond 65504, values below half's normal
    range (down to fp32 values that are subnormal as half and to ones that round to zero), exact 16-bit values (lo == 0) and
    zeros; hi and lo inside guard bands with a stride of their own (`ld16 % 4`, bases 8-byte aligned: the weakest layout),
    x inside NaN guards.

    Bound.  T has p significand bits (11 for half, 8 for bfloat16).  For |x| in T's normal range hi = rn_T(x), so
    |x - hi| <= 2^-p |x| (half an ulp) and x - hi is exact in fp32 (it needs at most 24 - p bits below hi's ulp).  r = (x - hi) *
    2048 is exact (a power of two) and lies in T's normal range or is 0 whenever |x - hi| * 2048 >= T's smallest normal, i.e. for
    half |x - hi| >= 2^-25; then lo = rn_T(r) has |r - lo| <= 2^-p |r| and
        |hi + lo / 2048 - x| = |lo - r| / 2048 <= 2^-p |x - hi| <= 2^-2p |x|.
    If r falls below half's normal range (|r| < 2^-14) lo is rounded to a multiple of 2^-24, an absolute error of at most 2^-25,
    i.e. 2^-36 after the division - below 2^-22 |x| for every |x| >= 2^-14, the smallest normal half.  bfloat16 shares fp32's
    exponent range: no such case above 2^-126 * 2^8."""
    T = LP()
    p = 11 if T == torch.float16 else 8
    g = torch.Generator().manual_seed(rows)
    cols = 64
    x = torch.randn(rows, cols, generator=g)
    x[:, 1::8] *= 1e-3
    x[:, 2::8] = torch.randn(rows, cols // 8, generator=g).to(T).float()        # exact 16-bit values: lo == 0
    x[:, 3::8] *= 1e5                                                           # beyond 65504
    x[:, 4::8] *= 2e-6                                                          # subnormal as half
    x[:, 5::8] *= 1e-9                                                          # rounds to zero as half
    x[:, 6::8] = 0.0
    x[0, 0], x[0, 7] = 65504.0, -70000.0
    want_hi, want_lo = _split_restatement(x, T)
    assert bool((want_lo[:, 2::8] == 0).all())
    base_hi, base_lo = ops.split16(dev(x))
    assert GB.same_bits(base_hi.cpu(), want_hi) and GB.same_bits(base_lo.cpu(), want_lo)
    mem = Mem()
    xi = mem.inp(dev(x), ld=cols + 20, name="x")
    ld16 = cols + 8 + 8 + 4 + 8
    hi = mem.out((rows, cols), T, ld=ld16, align=8, name="hi")
    lo = mem.out((rows, cols), T, ld=ld16, align=8, name="lo")
    ops.check(_lib.load().cdseg_split16(ops._ptr(xi), xi.stride(0), rows, cols, ops._ptr(hi), ops._ptr(lo), ld16, 2048.0, ops._stream()),
              "split16")
    mem.check()
    assert GB.same_bits(hi.cpu(), want_hi) and GB.same_bits(lo.cpu(), want_lo)
    lo_n, hi_n = (2.0 ** -14, 65504.0) if T == torch.float16 else (2.0 ** -118, 3.0e38)
    xd = x.double()
    normal = (xd.abs() >= lo_n) & (xd.abs() <= hi_n)
    rec = hi.cpu().double() + lo.cpu().double() / 2048.0
    rel = ((rec - xd).abs()[normal] / xd.abs()[normal]).max().item()
    report(f"split16 {lp} rows={rows}", max_rel=rel, bound=2.0 ** (-2 * p))
    assert rel <= 2.0 ** (-2 * p)


# ====================================================================================================== wide-stage kernels
def _kernel_map(ops, name, cut=None):
    if name == "random":  # the map of test_subm_conv3_large_random_map, cut to a few thousand rows
        from cdsegnet_amd import synth
        grid = torch.as_tensor(synth.room_scene(2, 120000)["grid_coord"])[:cut].cuda()
        batch = torch.zeros(len(grid), dtype=torch.int64, device="cuda")
        depth = int(ops.grid_max(grid).item()).bit_length()
        zs, perm0 = ops.sort_pairs(ops.encode(grid, batch, depth, "z"))
        g0, b0 = ops.plan_gather_grid(grid, perm0, zs, depth)
    else:
        zs, perm0, g0, b0, depth, p = _physical(ops, load_fixture(f"serialization_{name}.npz"))
    return ops.nbr_table(zs, g0, b0, depth, 3, True)


@pytest.mark.parametrize("lp", ["f16"])  # ("fp32x3" lives in the IEEE-half build: 11 + 11 significant bits per operand)
@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("name", ["room1500", "batch2", "random"])
def test_subm_conv3_f32_as_three_launches_against_fp64(ops, lp, name, C):
    """The fp32x3 sparse conv of the wide stages exactly as Engine._conv3 issues it (IEEE-half build): x and W split by
    cdseg_split16, then cdseg_subm_conv3_f32 three times - x_hi W_hi (+ bias), x_hi W_lo and x_lo W_hi with out_scale = 1 / 2048
    and accumulate - against oracle.model.subm_conv3d in fp64 on fp32 operands that are not representable in 16 bits and carry
    small magnitudes next to O(1) ones (the recipe of test_gemm_fp32x3_is_as_good_as_fp32_on_fp32_operands).  Bound: that
    test's two conditions with K = 27 C; err32 is the error of ops.gemm in exact fp32 on the same operands and map."""
    nbr = _kernel_map(ops, name, cut=4100)
    n = nbr.shape[1]
    g = torch.Generator().manual_seed(C + n)
    x = torch.randn(n, C, generator=g)
    x[:, ::3] *= 1e-4
    w = torch.randn(C, 27 * C, generator=g) / (27 * C) ** 0.5
    b = torch.randn(C, generator=g)
    ref = OM.subm_conv3d(x.double(), nbr.t().cpu().numpy().astype(np.int64), w.double().reshape(C, 3, 3, 3, C), b.double())
    xh, xl = ops.split16(dev(x))
    wh, wl = ops.split16(dev(w))
    assert ops.subm_conv3_ok(xh)
    ih, il = ops.subm_conv3_pack(wh), ops.subm_conv3_pack(wl)
    mem = Mem()
    y = mem.out((n, C), torch.float32, ld=C + 20, fill=NAN)  # accumulate = 0 onto NaN: must overwrite
    ops.subm_conv3_f32(xh, ih, dev(b), nbr, y)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all()), "accumulate = 0 must overwrite the output"
    first = y.clone()
    ops.subm_conv3_f32(xh, il, None, nbr, y, out_scale=1.0 / 2048.0, accumulate=True)
    ops.subm_conv3_f32(xl, ih, None, nbr, y, out_scale=1.0 / 2048.0, accumulate=True)
    mem.check()
    exact = torch.empty(n, C, device="cuda")
    ops.gemm(dev(x), dev(w), exact, bias=dev(b), nbr=nbr, nbr_kmajor=True, kvol=27, cache=False)
    err = (y.cpu().double() - ref).abs().max().item()
    err32 = (exact.cpu().double() - ref).abs().max().item()
    K = 27 * C
    report(f"subm_conv3_f32 x3 {name} C={C} n={n}", max_err=err, exact_fp32_err=err32, bound1=2 * (2e-5 * K ** 0.5 + 1e-5),
           bound2=8 * err32 + 2e-6)
    assert err < 2 * (2e-5 * K ** 0.5 + 1e-5) and err < 8 * err32 + 2e-6
    # accumulate = 1, out_scale = 1 onto a known output: known + the plain call's result, one fp32 rounding per element
    known = torch.randn(n, C, generator=g)
    acc = dev(known)
    ops.subm_conv3_f32(xh, ih, dev(b), nbr, acc, out_scale=1.0, accumulate=True)
    exact_sum = known.double() + first.cpu().double()
    half_ulp = exact_sum.abs() * (2.0 ** -24 * (1 + 2.0 ** -20)) + 2.0 ** -149
    assert bool(((acc.cpu().double() - exact_sum).abs() <= half_ulp).all())


@LPS
@pytest.mark.parametrize("C", [32, 64])
def test_subm_conv3_and_subm_conv3_f32_guard_bands_and_strides(ops, lp, C):
    """Both output forms of csrc/conv.hip on the `batch2` map and on one row.  Host checks: `ldx % 8`, x / y / image 16-byte
    aligned, `(1 << row_shift) == ldx * 2` (feature rows with a power-of-two byte stride only: x is a column window of a 4 C wide
    NaN-filled buffer), `ldy % 8` for the 16-bit output and `ldyf % 4` for the fp32 one.  -1 neighbours read no row: the NaN
    columns and rows around x never reach the output."""
    bf = LP()
    nbr_full = _kernel_map(ops, "batch2")
    for n in (nbr_full.shape[1], 1):
        nbr = nbr_full if n > 1 else torch.full((27, 1), -1, dtype=torch.int32, device="cuda")
        if n == 1:
            nbr[13, 0] = 0
        g = torch.Generator().manual_seed(C + n)
        x = dev(torch.randn(n, C, generator=g), bf)
        img = ops.subm_conv3_pack(dev(torch.randn(C, 27 * C, generator=g) / (27 * C) ** 0.5, bf))
        b = dev(torch.randn(C, generator=g))
        base = torch.full((n, C), NAN, dtype=bf, device="cuda")
        ops.subm_conv3(x, img, b, nbr, base)
        basef = torch.full((n, C), NAN, device="cuda")
        ops.subm_conv3_f32(x, img, b, nbr, basef)
        mem = Mem()
        xi = mem.inp(x, ld=4 * C, name="x")
        y = mem.out((n, C), bf, ld=C + 24)
        yf = mem.out((n, C), torch.float32, ld=C + 20, name="yf")
        nb = mem.index(nbr, none=-1)
        ops.subm_conv3(xi, img, b, nb, y)
        ops.subm_conv3_f32(xi, img, b, nb, yf)
        mem.check()
        assert bool(torch.isfinite(y.float()).all()) and bool(torch.isfinite(yf).all())
        assert GB.same_bits(y, base) and GB.same_bits(yf, basef)


@LPS
@pytest.mark.parametrize("name", ["tiny64", "batch2"])
def test_stem5_guard_bands(ops, lp, name):
    """cdseg_stem5 has no strides: out (n, 32) fp32 and out2 (n, 32) 16-bit are contiguous; both sit between guard rows, the
    8-channel input between NaN rows, every index operand with valid guard entries."""
    zs, perm0, g0, b0, depth, p = _physical(ops, load_fixture(f"serialization_{name}.npz"))
    n = len(p)
    cluster, seg, cnt = ops.pool_level(zs, 3)
    m = int(cnt.item())
    g1, b1, c41 = ops.pool_gather(seg, m, n, 1, g0, b0, ops.encode4(g0, b0, depth))
    pn3 = ops.nbr_table(c41[0].contiguous(), g1, b1, depth - 1, 3, True)
    cinfo = ops.child_info(zs, seg, m)
    g = torch.Generator().manual_seed(n)
    a = dev(torch.randn(n, 8, generator=g), LP())
    a[:, 6:] = 0
    img = ops.stem5_pack(dev(torch.randn(32, 1000, generator=g) / 30, LP()))
    sc, sh = dev(torch.rand(32, generator=g) + 0.5), dev(torch.randn(32, generator=g))
    base, base2 = torch.full((n, 32), NAN, device="cuda"), torch.full((n, 32), NAN, dtype=LP(), device="cuda")
    ops.stem5(a, img, sc, sh, g0, cluster, pn3, cinfo, depth, base, base2)
    mem = Mem()
    ai = mem.inp(a, cols=0, name="x8")
    out, out2 = mem.out((n, 32), torch.float32, cols=0), mem.out((n, 32), LP(), cols=0, name="out2")
    ops.stem5(ai, img, sc, sh, mem.index(g0), mem.index(cluster), mem.index(pn3, none=-1), mem.index(cinfo), depth, out, out2)
    mem.check()
    assert bool(torch.isfinite(out).all()) and GB.same_bits(out, base) and GB.same_bits(out2, base2)


@LPS
@pytest.mark.parametrize("m", [1, 16, 17])
@pytest.mark.parametrize("cin,cout", [(32, 64), (64, 128)])
def test_pool_fused_guard_bands_and_per_operand_strides(ops, lp, cin, cout, m):
    """cdseg_pool_fused, both shapes, m = 1 / 16 / 17 pooled rows (16-row strips: a full one, one more row); runs of 1 to 8 rows
    with one run of 20 that straddles two 16-row strips of x.  Host checks: `ldx % 8`, `ldo % 4`, `ldo2 % 4`, x / image / out
    16-byte aligned, out2 8-byte aligned: out2 runs on an 8-byte aligned base with a stride % 4 in the weak layout.  Bit-equal
    to the contiguous call (which test_pool_fused_equals_gemm_then_segment_max pins to cdseg_gemm + cdseg_segment_max)."""
    bf = LP()
    g = torch.Generator().manual_seed(cin + m)
    runs = torch.randint(1, 9, (m,), generator=g)
    runs[0] = 20 if m == 1 else 10
    if m > 1:
        runs[1] = 20  # rows 10 .. 29: across the strip boundary at row 16
    seg = torch.cat([torch.zeros(1, dtype=torch.int64), runs.cumsum(0)]).int()
    n = int(seg[-1])
    x = dev(torch.randn(n, cin, generator=g), bf)
    img = ops.pool_fused_pack(dev(torch.randn(cout, cin, generator=g) / cin ** 0.5, bf))
    b, sc, sh = dev(torch.randn(cout, generator=g) * 0.3), dev(torch.randn(cout, generator=g)), dev(torch.randn(cout, generator=g) * 0.2)
    base, base2 = torch.full((m, cout), NAN, device="cuda"), torch.full((m, cout), NAN, dtype=bf, device="cuda")
    ops.pool_fused(x, img, b, dev(seg), m, sc, sh, ops.ACT_GELU, base, base2)
    for layout in ("strided", "weak"):
        lay = "strided" if layout == "strided" else "ld4"
        mem = Mem()
        xi = mem.inp(x, ld=_lds(cin, bf, "strided", 0), name="x")
        out = mem.out((m, cout), torch.float32, ld=_lds(cout, torch.float32, lay, 1))
        out2 = mem.out((m, cout), bf, ld=_lds(cout, bf, lay, 2), align=0 if layout == "strided" else 8, name="out2")
        ops.pool_fused(xi, img, b, mem.index(dev(seg)), m, sc, sh, ops.ACT_GELU, out, out2)
        mem.check()
        assert bool(torch.isfinite(out).all()) and GB.same_bits(out, base) and GB.same_bits(out2, base2), layout


# ====================================================================================================== fused Block kernels
def _block_case(M, C, seed):
    from tests.test_gpu_ops import _deep_case
    d, bf = _deep_case(M, C, seed, True)
    return (lambda k, dt=None: None if d[k] is None else dev(d[k], dt)), bf


@LPS
@pytest.mark.parametrize("M,C", [(65, 32), (1, 32), (65, 64), (1, 64), (65, 128), (1, 128), (65535, 128), (65536, 128)])
def test_mlp_fused_guard_bands_and_per_operand_strides(ops, lp, M, C):
    """cdseg_mlp_fused: 64-row tiles; C = 128 switches to 128-row tiles at `n >= 128 * 512` (65535 / 65536).  Host checks:
    `ldh % 8`, `ldx % 4`, `ldxc % 4`, h / x 16-byte aligned, xc 8-byte aligned (weak: xc on an 8-byte aligned base, strides % 4).
    x is updated in place; h stays untouched."""
    D, bf = _block_case(M, C, M + C)
    w1, b1, w2, b2 = D("w1", bf), D("b1"), D("w2", bf), D("b2")
    base, basec = D("x0"), torch.full((M, C), NAN, dtype=bf, device="cuda")
    ops.mlp_fused(D("y", bf), w1, b1, w2, b2, base, basec)
    for layout in ("strided", "weak"):
        lay = "strided" if layout == "strided" else "ld4"
        mem = Mem()
        h = mem.inp(D("y", bf), ld=_lds(C, bf, "strided", 0), name="h")
        x = mem.inp(D("x0"), ld=_lds(C, torch.float32, lay, 1), name="x", inplace=True)
        xc = mem.out((M, C), bf, ld=_lds(C, bf, lay, 2), align=0 if layout == "strided" else 8, name="xc")
        ops.mlp_fused(h, w1, b1, w2, b2, x, xc)
        mem.check()
        assert GB.same_bits(x, base) and GB.same_bits(xc, basec), layout


@LPS
@pytest.mark.parametrize("M,C", [(65, 32), (1, 32), (65, 64), (1, 64)])
def test_attn_tail_fused_and_cpe_head_fused_guard_bands(ops, lp, M, C):
    """cdseg_attn_tail_fused and cdseg_cpe_head_fused below the 65 536-row switch (64-row tiles; the switch itself is
    tests/test_gpu_cpe_head_stream.py's).  Host checks as for cdseg_mlp_fused; qkv `ldqkv % 4` on an 8-byte aligned base."""
    D, bf = _block_case(M, C, 3 * M + C)
    base, basec = D("x0"), torch.full((M, C), NAN, dtype=bf, device="cuda")
    tail = (D("wp", bf), D("bp"), D("g3"), D("e3"), D("w1", bf), D("b1"), D("w2", bf), D("b2"))
    ops.attn_tail_fused(D("o", bf), *tail, base, basec)
    hbase, qbase = D("x0"), torch.full((M, 3 * C), NAN, dtype=bf, device="cuda")
    head = lambda y, x, q: ops.cpe_head_fused(y, D("wl", bf), D("bl"), (D("g1"), D("e1")), x, D("cb"), (D("g2"), D("e2")),  # noqa: E731
                                              D("wq", bf), D("bq"), q)
    head(D("y", bf), hbase, qbase)
    for layout in ("strided", "weak"):
        lay = "strided" if layout == "strided" else "ld4"
        a8 = 0 if layout == "strided" else 8
        mem = Mem()
        o = mem.inp(D("o", bf), ld=_lds(C, bf, "strided", 0), name="o")
        x = mem.inp(D("x0"), ld=_lds(C, torch.float32, lay, 1), name="x", inplace=True)
        xc = mem.out((M, C), bf, ld=_lds(C, bf, lay, 2), align=a8, name="xc")
        ops.attn_tail_fused(o, *tail, x, xc)
        mem.check()
        assert GB.same_bits(x, base) and GB.same_bits(xc, basec), layout
        mem = Mem()
        y = mem.inp(D("y", bf), ld=_lds(C, bf, "strided", 0), name="y")
        x = mem.inp(D("x0"), ld=_lds(C, torch.float32, lay, 1), name="x", inplace=True)
        q = mem.out((M, 3 * C), bf, ld=_lds(3 * C, bf, lay, 2), align=a8, name="qkv")
        head(y, x, q)
        mem.check()
        assert GB.same_bits(x, hbase) and GB.same_bits(q, qbase), layout


@LPS
@pytest.mark.parametrize("M,C", [(257, 32), (1, 32), (257, 64), (1, 64), (129, 128), (1, 128), (129, 256), (33, 256), (1, 256), (65, 512),
                                 (33, 512), (1, 512), (8193, 512)])
def test_block_rr_head_and_tail_guard_bands_and_read_buffers(ops, lp, M, C):
    """cdseg_cpe_head_rr / cdseg_attn_tail_rr at every width (C = 32 / 64: csrc/blockrr.hip; C = 128 / 256 / 512: csrc/deep.hip,
    128- and 32-row workgroups; C = 512 switches to 64-row tiles at DEEP512_ROWS64_MIN = 8193 rows) and, for the deep widths,
    the rr2 forms whose read buffer x must stay untouched.  Host checks: `ldy % 8`, `ldx % 4`, `ldqkv % 8`, `ldxc % 8`, every
    base 16-byte aligned - so the weakest layout differs from the strided one in the fp32 strides only (% 4)."""
    D, bf = _block_case(M, C, 5 * M + C)
    himg, timg = ops.block_rr_pack(C, D("wl", bf), D("wq", bf), D("wp", bf), D("w1", bf), D("w2", bf))
    deep = C in ops.DEEP_CHANNELS
    flags = ops.ATTN_V_BF16 if deep else 0
    hx, hq = D("x0"), torch.full((M, 3 * C), NAN, dtype=bf, device="cuda")
    ops.cpe_head_rr(D("y", bf), himg, D("bl"), (D("g1"), D("e1")), hx, D("cb"), (D("g2"), D("e2")), D("bq"), hq, qkv_flags=flags)
    tx, tc = D("x0"), torch.full((M, C), NAN, dtype=bf, device="cuda")
    ops.attn_tail_rr(D("o", bf), timg, D("bp"), D("g3"), D("e3"), D("b1"), D("b2"), tx, tc)
    for lay in ("strided", "ld4"):
        mem = Mem()
        y = mem.inp(D("y", bf), ld=_lds(C, bf, "strided", 0), name="y")
        x = mem.inp(D("x0"), ld=_lds(C, torch.float32, lay, 1), name="x", inplace=True)
        q = mem.out((M, 3 * C), bf, ld=_lds(3 * C, bf, "strided", 2), name="qkv")
        ops.cpe_head_rr(y, himg, D("bl"), (D("g1"), D("e1")), x, D("cb"), (D("g2"), D("e2")), D("bq"), q, qkv_flags=flags)
        mem.check()
        assert GB.same_bits(x, hx) and GB.same_bits(q, hq), lay
        mem = Mem()
        o = mem.inp(D("o", bf), ld=_lds(C, bf, "strided", 0), name="o")
        x = mem.inp(D("x0"), ld=_lds(C, torch.float32, lay, 1), name="x", inplace=True)
        xc = mem.out((M, C), bf, ld=_lds(C, bf, "strided", 2), name="xc")
        ops.attn_tail_rr(o, timg, D("bp"), D("g3"), D("e3"), D("b1"), D("b2"), x, xc)
        mem.check()
        assert GB.same_bits(x, tx) and GB.same_bits(xc, tc), lay
        if not deep:
            continue
        # rr2: read from x_in, write to x_out; the head is bit-identical to the in-place form, the unsplit tail (no workspace) too
        mem = Mem()
        y = mem.inp(D("y", bf), ld=_lds(C, bf, "strided", 0), name="y")
        x_in = mem.inp(D("x0"), ld=_lds(C, torch.float32, lay, 1), name="x_in")
        x_out = mem.out((M, C), torch.float32, ld=_lds(C, torch.float32, lay, 3), name="x_out")
        q = mem.out((M, 3 * C), bf, ld=_lds(3 * C, bf, "strided", 2), name="qkv")
        ops.cpe_head_rr2(y, himg, D("bl"), (D("g1"), D("e1")), x_in, x_out, D("cb"), (D("g2"), D("e2")), D("bq"), q, qkv_flags=flags)
        mem.check()  # (x_in is a registered input: "the rows read must stay untouched")
        assert GB.same_bits(x_out, hx) and GB.same_bits(q, hq), lay
        mem = Mem()
        o = mem.inp(D("o", bf), ld=_lds(C, bf, "strided", 0), name="o")
        x_in = mem.inp(D("x0"), ld=_lds(C, torch.float32, lay, 1), name="x_in")
        x_out = mem.out((M, C), torch.float32, ld=_lds(C, torch.float32, lay, 3), name="x_out")
        xc = mem.out((M, C), bf, ld=_lds(C, bf, "strided", 2), name="xc")
        ops.attn_tail_rr2(o, timg, D("bp"), D("g3"), D("e3"), D("b1"), D("b2"), x_in, x_out, xc, ws=None)
        mem.check()
        assert GB.same_bits(x_out, tx) and GB.same_bits(xc, tc), lay
        if C == 512 and M < ops.DEEP512_MIN_ROWS:  # the hidden-chunk split through a workspace of exactly 4 M C 4 bytes
            ws, wband = GB.exact_workspace(4 * M * C * 4)
            x_out2 = mem.out((M, C), torch.float32, ld=_lds(C, torch.float32, lay, 4), name="x_out (split)")
            xc2 = mem.out((M, C), bf, ld=_lds(C, bf, "strided", 5), name="xc (split)")
            ops.attn_tail_rr2(o, timg, D("bp"), D("g3"), D("e3"), D("b1"), D("b2"), x_in, x_out2, xc2, ws=ws)
            mem.check()
            wband.check()
            dd = (x_out2 - tx).abs().max().item()
            assert dd < 4e-6 * C ** 0.5 * max(1.0, float(tx.abs().max())), dd  # test_deep_head_and_tail_split_over_workgroups...
            assert torch.equal(xc2, x_out2.to(bf))


# ====================================================================================================== attention
def _attn_inputs(ops, dtype, lens_pts, H, K, seed, cross):
    """The setup of tests/test_gpu_ops.py::_attention_case: inputs, slot plan and the oracle's result."""
    g = torch.Generator().manual_seed(seed)
    C = 16 * H
    offset = np.cumsum(lens_pts)
    n = int(offset[-1])
    qkv = torch.randn(n, 3 * C, generator=g)
    qkv[:, :C] *= 2.0
    if dtype != torch.float32:
        qkv = qkv.to(dtype).float()
    starts = np.concatenate([[0], offset[:-1]])
    order = np.concatenate([s + torch.randperm(int(c), generator=g).numpy() for s, c in zip(starts, lens_pts)]).astype(np.int64)
    order_kv = order if not cross else np.concatenate([s + torch.randperm(int(c), generator=g).numpy() for s, c in zip(starts, lens_pts)])
    inverse = np.empty(n, dtype=np.int64)
    inverse[order] = np.arange(n)
    pad, unpad, cu = S.padding_plan(offset, K)
    q = qkv[:, :C][torch.from_numpy(order[pad])]
    k = qkv[:, C:2 * C][torch.from_numpy(order_kv[pad])]
    v = qkv[:, 2 * C:][torch.from_numpy(order_kv[pad])]
    ref = OM._patch_attention(q, k, v, cu, H, 16 ** -0.5)[torch.from_numpy(unpad[inverse])]
    offs = np.concatenate([[0], offset]).astype(np.int32)
    counts = np.diff(offs)
    pc = np.where(counts > K, (counts + K - 1) // K * K, counts)
    offs_pad = np.concatenate([[0], np.cumsum(pc)]).astype(np.int32)
    n_pad = int(offs_pad[-1])
    gq, wq = ops.pad_plan(dev(order.astype(np.int32)), dev(offs), dev(offs_pad), K, n_pad)
    gkv, _ = ops.pad_plan(dev(order_kv.astype(np.int32)), dev(offs), dev(offs_pad), K, n_pad)
    return dict(qkv=dev(qkv, dtype), gq=gq, gkv=gkv, wq=wq, ps=dev(cu.astype(np.int32)), max_len=int(np.diff(cu).max()), ref=ref, n=n, C=C)


@DTYPES
@pytest.mark.parametrize("cross", [False, True], ids=["self", "cross"])
@pytest.mark.parametrize("H,lens", [(2, [1500, 300]), (32, [991])])
def test_attention_guard_bands_out_stride_and_poisoned_qkv(ops, dtype, H, lens, cross):
    """cdseg_attention_ex: q, k, v each in a NaN-guarded buffer of its own with its own row stride (`ld * esz % 16 == 0`, bases
    16-byte aligned), out in a banded buffer with its own stride; gidx / widx / patch_start with valid guard entries (widx: -1 =
    "no row").  strided: bit-equal to the contiguous call.  16-bit builds also the weakest output layout the host code admits -
    `ldo * esz` and the base 8- but not 16-byte aligned (ATTN_STORE8) - against the oracle under the bounds of
    test_attention_fp32_vs_oracle (2e-5 (1 + max)) / test_attention_bf16_vs_oracle (0.02 (1 + max))."""
    d = _attn_inputs(ops, dtype, lens, H, 1024, sum(lens) + H, cross)
    n, C, qkv = d["n"], d["C"], d["qkv"]
    scale = 16 ** -0.5
    tol = (2e-5 if dtype == torch.float32 else 0.02) * (1 + d["ref"].abs().max().item())
    base = torch.full((n, C), NAN, dtype=dtype, device="cuda")
    ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], d["gq"], d["gkv"], d["wq"], d["ps"], H, d["max_len"], scale, base)
    assert (base.float().cpu() - d["ref"]).abs().max().item() < tol
    for layout in ["strided"] + (["weak"] if dtype != torch.float32 else []):
        mem = Mem()
        q = mem.inp(qkv[:, :C].contiguous(), ld=_lds(C, dtype, "strided", 0), name="q")
        k = mem.inp(qkv[:, C:2 * C].contiguous(), ld=_lds(C, dtype, "strided", 1), name="k")
        v = mem.inp(qkv[:, 2 * C:].contiguous(), ld=_lds(C, dtype, "strided", 2), name="v")
        out = mem.out((n, C), dtype, ld=_lds(C, dtype, "strided" if layout == "strided" else "ld4", 3), align=0 if layout == "strided" else 8)
        ops.attention(q, k, v, mem.index(d["gq"]), mem.index(d["gkv"]), mem.index(d["wq"], none=-1), mem.index(d["ps"]), H,
                      d["max_len"], scale, out)
        mem.check()
        assert bool(torch.isfinite(out.float()).all()), "a guard row of q / k / v reached the output, or a row was never written"
        if layout == "strided":
            assert GB.same_bits(out, base)
        assert (out.float().cpu() - d["ref"]).abs().max().item() < tol
