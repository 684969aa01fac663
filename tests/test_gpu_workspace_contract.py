"""GPU: every workspace, scratch arena and packed image at EXACTLY the size its cdseg_*_bytes function reports.

include/cdseg.h promises an outside caller that the reported size is enough.  Inside this repository nothing ever ran that way:
ops.workspace() grants 25 % + 4 KiB of slack and never shrinks, torch's allocator rounds the training workspaces up to 512
bytes.  Every test here
  1. runs the operation through today's path (the reference result),
  2. runs it again with every workspace / scratch request served by tests/guard_bands.exact_workspace: a 256-byte aligned view
     of exactly the requested bytes inside a buffer of 0xA5 whose bands on both sides are wider than any slack the kernels have
     had (so an overrun lands in memory the test owns),
  3. checks that the request was the size function's figure, that both bands are intact, and that the results are BIT-equal.
A workspace the kernel only partly initialises also shows here: the exact view starts as 0xA5 bytes, not as whatever an earlier
launch left behind.

cdseg_gemm's workspace is sized by cdseg_gemm_ws_bytes like the others, but it also runs with less (fewer split-K slices) and
the size chooses the launch plan: its tests cover the query's three branches through the wrapper (with the recorded route)
and explicit smaller workspaces through the C entry point.

ops.workspace is replaced for the inference wrappers, ops._scratch (the one place the training wrappers, the packed images and
the plan arenas allocate from) for the rest.  The test id names the entry point(s).
"""
import ctypes

import numpy as np
import pytest
import torch

from cdsegnet_amd import _lib
from tests import guard_bands as GB
from tests.helpers import load_fixture
from tests.test_gpu_ops import LP, LPS, _library_variant, _physical, dev, ops  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def _flat(r):
    if isinstance(r, torch.Tensor):
        return [r]
    if isinstance(r, np.ndarray):
        return [torch.as_tensor(r)]
    if isinstance(r, dict):
        return [t for k in sorted(r) for t in _flat(r[k])]
    if isinstance(r, (list, tuple)):
        return [t for x in r for t in _flat(x)]
    return []


def _exact_vs_today(ops, fn, attrs=("workspace",), at_least=1, sizes=None):
    """fn() through today's allocation, then with `attrs` of ops serving exact views: bit-equal results, intact bands.
    sizes: the figures of the size function(s) - every one of them must have been requested, byte for byte."""
    want = _flat(fn())
    torch.cuda.synchronize()
    exact = GB.ExactWorkspaces()
    with pytest.MonkeyPatch.context() as mp:
        for a in attrs:
            mp.setattr(ops, a, exact)
        got = _flat(fn())
        torch.cuda.synchronize()
    exact.check(at_least=at_least)
    served = [b.nbytes for b in exact.served]
    for s in sizes or ():
        assert int(s) in served, f"the size function reports {int(s)} bytes, the wrapper asked for {served}"
    assert len(want) == len(got) and len(want) > 0
    for i, (a, b) in enumerate(zip(want, got)):
        assert GB.same_bits(a, b), f"result {i} differs between the exact-size workspace and today's path"
    return exact


def _cloud(ops, name):
    fx = load_fixture(f"serialization_{name}.npz")
    zs, perm0, g0, b0, depth, p = _physical(ops, fx)
    return zs, g0, b0, depth, len(p)


# ------------------------------------------------------------------ sorting and pooling structure
@pytest.mark.parametrize("n", [1, 255, 4097, 70001])
def test_cdseg_sort_pairs_at_cdseg_sort_ws_bytes(ops, n):
    rng = np.random.default_rng(n)
    keys = dev(rng.integers(0, 2 ** 48, n))
    ex = _exact_vs_today(ops, lambda: ops.sort_pairs(keys, None, end_bit=48), sizes=[_lib.load().cdseg_sort_ws_bytes(n)])
    assert np.array_equal(ops.sort_pairs(keys, None, end_bit=48)[1].cpu().numpy(), np.argsort(keys.cpu().numpy(), kind="stable"))
    assert len(ex.served) == 1


@pytest.mark.parametrize("name", ["room1500", "batch2", "tiny64"])
def test_cdseg_sort_curves_at_cdseg_sort_curves_ws_bytes(ops, name):
    zs, g0, b0, depth, n = _cloud(ops, name)
    code4 = ops.encode4(g0, b0, depth)
    nb = int(b0.max().item()) + 1
    end_bit = 3 * depth + max(1, nb.bit_length())
    for rows in ([1, 2, 3], [2], [0, 1, 2, 3]):
        _exact_vs_today(ops, lambda: ops.sort_curves(code4, rows, end_bit),
                        sizes=[_lib.load().cdseg_sort_curves_ws_bytes(n, len(rows))])


@pytest.mark.parametrize("name", ["room1500", "batch2", "tiny64", "lidar8"])
def test_cdseg_pool_level_and_cdseg_pool_levels_at_their_ws_bytes(ops, name):
    zs, g0, b0, depth, n = _cloud(ops, name)
    lib = _lib.load()

    def one():
        cl, seg, cnt = ops.pool_level(zs, 3)
        m = int(cnt.item())
        return cl, seg[:m + 1], cnt  # (seg_start: the first count + 1 entries are defined)

    _exact_vs_today(ops, one, sizes=[lib.cdseg_sort_ws_bytes(n)])
    shifts = [3 * c for c in (1, 2, 3) if c < depth]
    nbatch = int(b0.max().item()) + 1
    last = torch.as_tensor(np.searchsorted(b0.cpu().numpy(), np.arange(nbatch), side="right") - 1, dtype=torch.int32).cuda()

    def many():
        cl, seg, meta = ops.pool_levels(zs, shifts, last)
        counts = meta.cpu().numpy()[::1 + nbatch][:len(shifts)]
        return [cl, meta] + [seg[i, :int(c) + 1] for i, c in enumerate(counts)]

    _exact_vs_today(ops, many, sizes=[lib.cdseg_pool_levels_ws_bytes(n, len(shifts))])


@pytest.mark.parametrize("name", ["room1500", "batch2", "rand16"])
def test_cdseg_coarse_orders_at_cdseg_coarse_orders_ws_bytes(ops, name):
    zs, g0, b0, depth, n = _cloud(ops, name)
    code0 = ops.encode4(g0, b0, depth)
    orders0 = [ops.sort_pairs(code0[c].contiguous())[1] for c in (1, 2, 3)]
    clusters, sizes = [], []
    for cum in (1, 2, 3):
        if cum >= depth:
            break
        cl, seg, cnt = ops.pool_level(zs, 3 * cum)
        clusters.append(cl)
        sizes.append(int(cnt.item()))
    _exact_vs_today(ops, lambda: ops.coarse_orders(clusters, orders0, sizes),
                    sizes=[_lib.load().cdseg_coarse_orders_ws_bytes(n, len(clusters), 3)])


# ------------------------------------------------------------------ plan builder: the i32 and i64 arenas and the workspace
def _plan_setup(case):
    from cdsegnet_amd import configs, synth
    from cdsegnet_amd.param_init import fill_state_dict
    from cdsegnet_amd.registry import build_model
    import cdsegnet_amd.models  # noqa: F401
    from tests.helpers import tiny_inputs
    model = build_model(configs.cdsegnet_config("scannet"))
    model.load_state_dict(fill_state_dict(model.state_dict(), seed=0))
    model = model.cuda().eval()
    if case == "two_scenes":
        scs = [synth.room_scene(1, 30000), synth.room_scene(2, 1700)]
    elif case == "tiny":
        scs = [synth.room_scene(3, 600)]
    else:
        scs = None
    if scs is None:
        ti = tiny_inputs(case)
        grid = torch.as_tensor(np.asarray(ti["grid_coord"])).cuda()
        offs = [int(v) for v in np.asarray(ti["offset"])]
    else:
        grid = torch.as_tensor(np.concatenate([s["grid_coord"] for s in scs])).cuda()
        offs = list(np.cumsum([len(s["grid_coord"]) for s in scs]).tolist())
    return model, grid, offs


@pytest.mark.parametrize("case", ["tiny", "two_scenes", "seven_and_many"])
def test_cdseg_plan_begin_and_cdseg_plan_finish_arenas_at_their_layout_sizes(ops, case):
    """The three arenas of both calls (i32, i64, ws) at exactly the element counts of cdseg_plan_begin_layout /
    cdseg_plan_finish_layout; every item of the plan bit-equal to the plan built on today's allocations (the cases and the
    item list of test_native_plan_equals_per_op_plan)."""
    from cdsegnet_amd.engine import CURVES
    from tests.test_gpu_e2e import _plan_items
    model, grid, offs = _plan_setup(case)
    offset = torch.tensor(offs, dtype=torch.int64).cuda()
    eng = model.engine()
    eng.prepare(grid.device)
    eng.native_plan = True
    curves = sorted({CURVES.index(o) for o in model.backbone.order})
    ops.bind_stream()
    try:
        eng.build_plan(grid, offset, offs, offs[-1])  # (the first call of an engine takes the exact depth: per-op path)

        def build():
            plan = eng.build_plan(grid, offset, offs, offs[-1])
            assert getattr(plan, "native", None) is not None
            items = _plan_items(plan, eng._pad_keys, curves)
            torch.cuda.synchronize()
            return items

        ex = _exact_vs_today(ops, build, attrs=("workspace", "_scratch"), at_least=5)
    finally:
        ops.unbind_stream()
    assert len(ex.served) >= 5  # b32, b64, ws, f32, f64 (and a second ws when the finish needs more)


# ------------------------------------------------------------------ GEMM: a workspace whose size is the caller's choice
def _gemm_case(M, N, K, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    if dtype != torch.float32:
        A, W = A.to(dtype).float(), W.to(dtype).float()
    b = torch.randn(N, generator=g)
    return A, W, b


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,N,K", [(300, 512, 512), (65, 2048, 512), (100, 128, 4096)])
def test_cdseg_gemm_split_k_through_the_wrapper_at_the_requested_bytes(ops, dtype, M, N, K):
    """ops.gemm asks for cdseg_gemm_ws_bytes(M, N, 0, 0) = min(32 M N 4, 64 MiB): the split-K partial planes (splits, M, N)
    fp32 stay inside exactly that."""
    A, W, b = _gemm_case(M, N, K, dtype, M + N + K)
    Ad, Wd, bd = dev(A, dtype), dev(W, dtype), dev(b)

    def run():
        out = torch.empty(M, N, dtype=torch.float32, device="cuda")
        ops.gemm(Ad, Wd, out, bias=bd, cache=False)
        return out

    size = _lib.load().cdseg_gemm_ws_bytes(M, N, 0, 0)
    assert size == min(32 * M * N * 4, 64 << 20)
    _exact_vs_today(ops, run, sizes=[size])
    err = (run().cpu().double() - (A.double() @ W.double().t() + b.double())).abs().max().item()
    assert err < (2e-5 * K ** 0.5 + 1e-5)  # the bound of test_gemm_split_k / test_gemm_plain


@LPS
def test_cdseg_gemm_deep_conv_through_the_wrapper_at_cdseg_gemm_ws_bytes(ops, lp):
    """The second branch of the size rule: a gathered 16-bit GEMM whose 64 x 128 tiles fill the chip (256 of them) while its
    256 x 256 tiles do not (32).  M = 8192, N = K = 256, 27 offsets on a synthetic kernel map: the wrapper asks for the
    query's 8 M N 4 bytes (= 64 MiB), the launch splits K 256 / 32 = 8 ways and its 8 planes fill exactly that."""
    M, C, bf = 8192, 256, LP()
    g = torch.Generator().manual_seed(M + C)
    nbr = torch.where(torch.rand(27, M, generator=g) > 0.5, torch.randint(0, M, (27, M), generator=g), torch.full((27, M), -1)).int()
    xd = dev(torch.randn(M, C, generator=g), bf)
    wd = dev(torch.randn(C, 27 * C, generator=g) / (13 * C) ** 0.5, bf)
    bd, nd = dev(torch.randn(C, generator=g)), dev(nbr)
    splits = []

    def run():
        out = torch.full((M, C), float("nan"), dtype=torch.float32, device="cuda")
        with ops.record_routes() as rr:
            ops.gemm(xd, wd, out, bias=bd, nbr=nd, nbr_kmajor=True, kvol=27, cache=False)
        splits.append([r.splits for r in rr.routes])
        return out

    size = _lib.load().cdseg_gemm_ws_bytes(M, C, 1, 0)
    assert size == 8 * M * C * 4 and _lib.load().cdseg_gemm_ws_bytes(M, C, 0, 0) == 0
    ex = _exact_vs_today(ops, run, sizes=[size])
    assert [b.nbytes for b in ex.served] == [size]
    assert splits == [[8], [8]], splits  # today's allocation and the exact view: the same plan


def test_cdseg_gemm_fused_layernorm_through_the_wrapper_at_cdseg_gemm_ws_bytes(ops):
    """The third branch: fp32, ln_post over N = 256 (two column tiles), M = 16384 - 512 tiles of 64 x 128, so no split-K: the
    wrapper asks for the query's one plane M N 4 and the row finish runs inside exactly that."""
    M, N, K = 16384, 256, 256
    A, W, b = _gemm_case(M, N, K, torch.float32, M + N + K)
    g = torch.Generator().manual_seed(7)
    Ad, Wd, bd, res = dev(A), dev(W), dev(b), dev(torch.randn(M, N, generator=g))
    g2, b2 = dev(1 + 0.1 * torch.randn(N, generator=g)), dev(0.1 * torch.randn(N, generator=g))
    routes = []

    def run():
        out = torch.full((M, N), float("nan"), dtype=torch.float32, device="cuda")
        h = torch.full((M, N), float("nan"), dtype=torch.float32, device="cuda")
        with ops.record_routes() as rr:
            ops.gemm(Ad, Wd, out, bias=bd, res=res, ln_post=(g2, b2), ln_out=h, cache=False)
        routes.append([(r.splits, r.fix) for r in rr.routes])
        return out, h

    size = _lib.load().cdseg_gemm_ws_bytes(M, N, 0, 1)
    assert size == M * N * 4 and _lib.load().cdseg_gemm_ws_bytes(M, N, 0, 0) == 0
    ex = _exact_vs_today(ops, run, sizes=[size])
    assert [b.nbytes for b in ex.served] == [size]
    assert routes == [[(1, 2)], [(1, 2)]], routes  # unsplit, rows finished from the workspace, on both allocations
    out, h = run()
    x_ref = res.cpu().double() + A.double() @ W.double().t() + b.double()
    assert (out.cpu().double() - x_ref).abs().max().item() < 2e-4 + 2e-5 * K ** 0.5  # test_gemm_fused_layernorm_epilogue's bound
    h_ref = torch.nn.functional.layer_norm(x_ref.float(), (N,), g2.cpu(), b2.cpu())
    assert (h.cpu() - h_ref).abs().max().item() < 2e-4 * (1 + h_ref.abs().max().item())


def _gemm_raw(ops, A, W, out, ws, ws_bytes, bias=None, ln=None, res=None, ln_out=None):
    """cdseg_gemm with an explicit workspace (the wrapper chooses its own): returns the status code."""
    a = _lib.GemmArgs()
    a.A, a.W, a.out, a.bias = A.data_ptr(), W.data_ptr(), out.data_ptr(), None if bias is None else bias.data_ptr()
    a.M, a.N, a.K, a.kvol = A.shape[0], W.shape[0], W.shape[1], 1
    a.lda, a.ldo = A.stride(0), out.stride(0)
    a.compute_dtype = a.a_dtype = ops.dt(A)
    a.out_dtype = ops.dt(out)
    a.act = ops.ACT_NONE
    if res is not None:
        a.res, a.ldres = res.data_ptr(), res.stride(0)
    if ln is not None:
        a.ln_post_g, a.ln_post_b = ln[0].data_ptr(), ln[1].data_ptr()
        a.ln_out, a.ldln, a.ln_out_dtype = ln_out.data_ptr(), ln_out.stride(0), ops.dt(ln_out)
    a.ln_eps = 1e-5
    a.ws, a.ws_bytes = (None, 0) if ws is None else (ws.data_ptr(), int(ws_bytes))
    rc = _lib.load().cdseg_gemm(ctypes.byref(a), ops._stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("short", [0, 16], ids=["exact", "16-bytes-less"])
@pytest.mark.parametrize("s", [2, 3])
def test_cdseg_gemm_with_a_workspace_of_s_planes(ops, dtype, s, short):
    """ws_bytes = s M N 4 (and 16 bytes less: one plane fewer fits, `while (smax * M * N * 4 > ws_bytes) --smax` in launch_bn):
    the bands stay intact, the result meets the bound of test_gemm_split_k, two runs with the same ws_bytes are bit-equal.
    M x N x K = 100 x 128 x 4096: two output tiles, 64 K steps - the launch wants 16 splits and takes what fits."""
    M, N, K = 100, 128, 4096
    A, W, b = _gemm_case(M, N, K, dtype, 17 + s)
    ref = A.double() @ W.double().t() + b.double()
    Ad, Wd, bd = dev(A, dtype), dev(W, dtype), dev(b)
    nbytes = s * M * N * 4 - short
    outs = []
    for _ in range(2):
        ws, band = GB.exact_workspace(nbytes)
        out, oband = GB.banded((M, N), torch.float32, fill=-777.25)
        assert _gemm_raw(ops, Ad, Wd, out, ws, nbytes, bias=bd) == 0
        band.check()
        oband.check()
        outs.append(out.clone())
    assert GB.same_bits(outs[0], outs[1])
    err = (outs[0].cpu().double() - ref).abs().max().item()
    assert err < (2e-5 * K ** 0.5 + 1e-5), err


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_cdseg_gemm_layernorm_refuses_a_workspace_16_bytes_short_and_writes_nothing(ops, dtype):
    """N = 256 with a fused LayerNorm: rows span two column tiles, the second pass (row_finish_kernel) needs M N 4 bytes.
    launch_bn: `if (!can_fix || splits * M * N * 4 > ws_bytes) return CDSEG_ERR_WORKSPACE` - before any launch."""
    M, N, K = 130, 256, 64
    A, W, b = _gemm_case(M, N, K, dtype, 5)
    Ad, Wd, bd = dev(A, dtype), dev(W, dtype), dev(b)
    g2, b2 = dev(torch.ones(N)), dev(torch.zeros(N))
    res = dev(torch.randn(M, N))
    need = M * N * 4
    ws, band = GB.exact_workspace(need - 16)
    out, oband = GB.banded((M, N), torch.float32, fill=-777.25)
    h, hband = GB.banded((M, N), dtype, fill=-3.0)
    rc = _gemm_raw(ops, Ad, Wd, out, ws, need - 16, bias=bd, ln=(g2, b2), res=res, ln_out=h)
    assert _lib.ERRORS.get(rc) == "CDSEG_ERR_WORKSPACE", rc
    band.check(), oband.check(), hband.check()
    assert bool((out == -777.25).all()) and bool((h == -3.0).all()) and bool((ws == 0xA5).all())
    # with exactly M N 4 bytes the same call runs, inside its workspace
    ws, band = GB.exact_workspace(need)
    assert _gemm_raw(ops, Ad, Wd, out, ws, need, bias=bd, ln=(g2, b2), res=res, ln_out=h) == 0
    band.check(), oband.check(), hband.check()
    x_ref = res.cpu().double() + A.double() @ W.double().t() + b.double()
    assert (out.cpu().double() - x_ref).abs().max().item() < 2e-4 + 2e-5 * K ** 0.5  # test_gemm_fused_layernorm_epilogue's bound
    h_ref = torch.nn.functional.layer_norm(x_ref.float(), (N,))
    assert (h.float().cpu() - h_ref).abs().max().item() < (2e-4 if dtype == torch.float32 else 0.03) * (1 + h_ref.abs().max().item())


# ------------------------------------------------------------------ deep tail: the caller's workspace
@LPS
@pytest.mark.parametrize("M", [31, 779])
def test_cdseg_attn_tail_rr2_with_a_workspace_of_s_planes(ops, lp, M):
    """C = 512 below the row threshold of the hidden-chunk split (DEEP512 few-row launches): ws of exactly s M C 4 bytes for
    s = 2, 3, 4 and 16 bytes less than each.  Bands intact, x_in untouched, two runs bit-equal, the result within the bound of
    test_deep_head_and_tail_split_over_workgroups... of the in-place form."""
    from tests.test_gpu_ops import _deep_case
    C = 512
    d, bf = _deep_case(M, C, M * 7 + C, False)
    D = lambda k, dt=None: None if d[k] is None else dev(d[k], dt)  # noqa: E731
    _, timg = ops.block_rr_pack(C, None, None, D("wp", bf), D("w1", bf), D("w2", bf))
    xa = D("x0")
    ops.attn_tail_rr(D("o", bf), timg, D("bp"), D("g3"), D("e3"), D("b1"), D("b2"), xa, None)
    for s in (2, 3, 4):
        for short in (0, 16):
            nbytes = s * M * C * 4 - short
            outs = []
            for _ in range(2):
                ws, band = GB.exact_workspace(nbytes)
                x_in = D("x0")
                xb, xband = GB.banded((M, C), torch.float32, fill=float("nan"))
                xcb, cband = GB.banded((M, C), bf, fill=float("nan"))
                ops.attn_tail_rr2(D("o", bf), timg, D("bp"), D("g3"), D("e3"), D("b1"), D("b2"), x_in, xb, xcb, ws=ws)
                torch.cuda.synchronize()
                band.check(), xband.check(), cband.check()
                assert torch.equal(x_in, D("x0")), "the rows read must stay untouched"
                outs.append((xb.clone(), xcb.clone()))
            assert GB.same_bits(outs[0][0], outs[1][0]) and GB.same_bits(outs[0][1], outs[1][1]), (s, short)
            dd = (outs[0][0] - xa).abs().max().item()
            assert dd < 4e-6 * C ** 0.5 * max(1.0, float(xa.abs().max())), (s, short, dd)
            assert torch.equal(outs[0][1], outs[0][0].to(bf))


# ------------------------------------------------------------------ Block executor scratch
def _native_block(ops, npts, C, seed):
    """One cdseg_block_forward on a synthetic scene's kernel map and padded patch plan (the setup of
    test_native_block_executor_vs_oracle_block without the oracle): returns run(scratch) -> (x, xc_out)."""
    from cdsegnet_amd import synth
    from oracle import model as OM
    from oracle import serialization as S
    rng = np.random.default_rng(seed)
    bf, H = LP(), C // 16
    grid = np.asarray(synth.room_scene(9, npts)["grid_coord"], dtype=np.int64)
    n = len(grid)
    nbr = OM.subm_neighbors(grid, np.zeros(n, dtype=np.int64), 3)
    pad, unpad, cu = S.padding_plan(np.array([n]), 1024)
    perm = rng.permutation(n)
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    order, inverse = perm[pad], unpad[inv]
    w16 = lambda *sh: dev(rng.standard_normal(sh).astype(np.float32) * sh[-1] ** -0.5, bf)  # noqa: E731
    vec = lambda k, one=False: dev((rng.standard_normal(k) * 0.1 + (1.0 if one else 0.0)).astype(np.float32))  # noqa: E731
    t = dict(cpe_conv_w=dev(rng.standard_normal((C, 27 * C)).astype(np.float32) * (13 * C) ** -0.5, bf), cpe_conv_b=vec(C),
             cpe_lin_w=w16(C, C), cpe_lin_b=vec(C), cpe_ln_g=vec(C, True), cpe_ln_b=vec(C), norm1_g=vec(C, True), norm1_b=vec(C),
             qkv_w=w16(3 * C, C), qkv_b=vec(3 * C), proj_w=w16(C, C), proj_b=vec(C), norm2_g=vec(C, True), norm2_b=vec(C),
             fc1_w=w16(4 * C, C), fc1_b=vec(4 * C), fc2_w=w16(C, 4 * C), fc2_b=vec(C))
    if ops.subm_conv3_ok(torch.empty((1, C), dtype=bf, device="meta")):
        t["cpe_conv_wimg"] = ops.subm_conv3_pack(t["cpe_conv_w"])
    himg, t["tail_img"] = ops.block_rr_pack(C, t["cpe_lin_w"], t["qkv_w"], t["proj_w"], t["fc1_w"], t["fc2_w"])
    if ops.block_rr_head_on(C):
        t["head_img"] = himg
    desc = ops.make_block_desc(bf, C, H, 4 * C, 16 ** -0.5, 1e-5, t)
    x_in = torch.as_tensor(rng.standard_normal((n, C)).astype(np.float32)).to(bf).float()
    wi = np.full(len(order), -1, dtype=np.int32)
    wi[inverse] = np.arange(n, dtype=np.int32)
    gidx, widx, nbrd, cud = dev(order.astype(np.int32)), dev(wi), dev(nbr.T.astype(np.int32)), dev(np.asarray(cu, dtype=np.int32))
    tbias = vec(C)

    def run(scratch):
        x, xc_in = dev(x_in), dev(x_in, bf)
        xc_out = torch.full((n, C), float("nan"), dtype=bf, device="cuda")
        ops.bind_stream()
        try:
            ops.block_forward(desc, n, x, xc_in, xc_out, tbias, nbrd, gidx, widx, cud, len(cu) - 1, int(np.diff(cu).max()), scratch)
        finally:
            ops.unbind_stream()
        torch.cuda.synchronize()
        return x, xc_out

    return desc, n, run


@LPS
@pytest.mark.parametrize("npts,C", [(900, 32), (2300, 128), (3200, 512), (790, 512)],
                         ids=["C32", "C128", "C512", "C512-below-the-rr2-row-threshold"])
def test_cdseg_block_forward_scratch_at_cdseg_block_scratch_bytes(ops, lp, npts, C):
    desc, n, run = _native_block(ops, npts, C, npts + C)
    if C == 512 and npts < 1000:
        assert n < ops.DEEP512_MIN_ROWS
    nbytes = ops.block_scratch_bytes(desc, n)
    slack = torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8, device="cuda")  # what the engine hands out today
    x0, xc0 = run(slack)
    ws, band = GB.exact_workspace(nbytes)
    x1, xc1 = run(ws)
    band.check()
    assert bool(torch.isfinite(x1).all()) and GB.same_bits(x0, x1) and GB.same_bits(xc0, xc1)


# ------------------------------------------------------------------ test-time kernels
@pytest.mark.parametrize("m,mixed", [(1, False), (65, True), (1000, True)])
def test_cdseg_fragments_build_at_cdseg_fragments_build_ws_bytes(ops, m, mixed):
    from tests.test_gpu_testpipeline import _layout
    n, nfrag, idx_sort, seg, rng = _layout(m, mixed, 100 * m + mixed)
    grid = dev(rng.integers(0, 1 << 20, (n, 3)).astype(np.int32))
    feat = dev(rng.normal(size=(n, 6)).astype(np.float32))
    for cdt in (torch.float32, torch.float64):
        coord = dev(rng.normal(0, 20, (n, 3)), cdt)
        _exact_vs_today(ops, lambda: ops.fragments_build(idx_sort, seg, m, nfrag, grid, feat, coord, center_shift=True),
                        sizes=[_lib.load().cdseg_fragments_build_ws_bytes(nfrag)])


@pytest.mark.parametrize("nref", [1, 40, 9000])
def test_cdseg_knn1_and_cdseg_knn_at_cdseg_knn1_ws_bytes(ops, nref):
    rng = np.random.default_rng(nref)
    ref = (rng.random((nref, 3)) * np.array([4.0, 3.0, 0.3])).astype(np.float32)
    qry = np.concatenate([(rng.random((3000, 3)) * np.array([4.0, 3.0, 0.3])).astype(np.float32), ref[:50] + np.float32(30.0)])
    r0 = nref // 3
    roff, qoff = dev(np.array([r0, nref], dtype=np.int32)), dev(np.array([300, len(qry)], dtype=np.int32))
    rd, qd = dev(ref), dev(qry)
    size = _lib.load().cdseg_knn1_ws_bytes(nref)
    for cell in (0.05, 4.0):
        _exact_vs_today(ops, lambda: ops.knn1(rd, roff, qd, qoff, ref.min(0).tolist(), cell, want_dist=True), sizes=[size])
        for k in (8, 48):
            _exact_vs_today(ops, lambda: ops.knn(k, rd, roff, qd, qoff, origin=ref.min(0).tolist(), cell=cell), sizes=[size])


# ------------------------------------------------------------------ packed weight images
@LPS
def test_cdseg_subm_conv3_pack_stem5_pack_block_rr_pack_pool_fused_pack_write_inside_their_image_bytes(ops, lp):
    bf, lib = LP(), _lib.load()
    g = torch.Generator(device="cuda").manual_seed(3)
    r = lambda *s: (torch.randn(*s, device="cuda", generator=g) / s[-1] ** 0.5).to(bf)  # noqa: E731
    for C in (32, 64):
        w = r(C, 27 * C)
        _exact_vs_today(ops, lambda: ops.subm_conv3_pack(w), attrs=("_scratch",), sizes=[lib.cdseg_subm_conv3_wimg_bytes(C)])
    w5 = r(32, 1000)
    _exact_vs_today(ops, lambda: ops.stem5_pack(w5), attrs=("_scratch",), sizes=[lib.cdseg_stem5_wimg_bytes()])
    for cin, cout in ((32, 64), (64, 128)):
        wp = r(cout, cin)
        _exact_vs_today(ops, lambda: ops.pool_fused_pack(wp), attrs=("_scratch",), sizes=[lib.cdseg_pool_fused_img_bytes(cin, cout)])
    for C in (32, 64, 128, 256, 512):
        ws_ = [r(C, C), r(3 * C, C), r(C, C), r(4 * C, C), r(C, 4 * C)]
        _exact_vs_today(ops, lambda: ops.block_rr_pack(C, *ws_), attrs=("_scratch",), at_least=2,
                        sizes=[lib.cdseg_block_rr_img_bytes(C, 0), lib.cdseg_block_rr_img_bytes(C, 1)])


# ------------------------------------------------------------------ training kernels (ops._scratch)
@pytest.mark.parametrize("lp", ["fp32", "bf16", "f16"])
def test_cdseg_attention_bwd_at_cdseg_attention_bwd_ws_bytes(ops, lp):
    """The `dups` case of tests/test_gpu_attention_bwd16.py with its padding duplicates redrawn without replacement, as in
    test_attention_bwd_is_bit_repeatable_as_it_is (an element receives at most two atomic adds, which commute)."""
    from tests import test_gpu_attention_bwd16 as A
    _, lens, H, dup, cross, packed, sigma_k = {c[0]: c for c in A.CASES}["dups"]
    lpt = LP()
    rng = np.random.default_rng(sum(lens) + 31 * H + dup)
    launch, (q16, k16, v16, do16) = A._case(lens, H, dup, cross, lpt, rng, sigma_k)
    patches = list(launch.patches)
    gq, gkv, widx = (a.copy() for a in patches[-1])
    own = len(gq) - dup
    pick = rng.choice(own, dup, replace=False)
    gq[own:], gkv[own:] = gq[pick], gkv[pick]
    patches[-1] = (gq, gkv, widx)
    launch = A.Launch(patches)
    dtype = torch.float32 if lp == "fp32" else None
    ex = _exact_vs_today(ops, lambda: list(A._kernel(lpt, q16, k16, v16, do16, launch, H, packed=packed, dtype=dtype)),
                         attrs=("_scratch",))
    assert all(b.nbytes > 0 for b in ex.served)


@pytest.mark.parametrize("m,c", [(200, 16), (5000, 32), (3000, 512)])
def test_cdseg_layernorm_bwd_det_at_cdseg_layernorm_bwd_det_ws_bytes(ops, m, c):
    g = torch.Generator().manual_seed(m + c)
    xd, gd, dyd = (torch.randn(*s, generator=g).cuda() for s in ((m, c), (c,), (m, c)))

    def run():
        dx = torch.empty(m, c, device="cuda")
        dg, db = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda")
        ops.layernorm_bwd(xd, gd, dyd, dx, dgamma=dg, dbeta=db, deterministic=True)
        return dx, dg, db

    _exact_vs_today(ops, run, attrs=("_scratch",), sizes=[max(16, _lib.load().cdseg_layernorm_bwd_det_ws_bytes(m, c))])


@pytest.mark.parametrize("lp", ["fp32", "bf16", "f16"])
def test_cdseg_linear_wgrad_det_and_cdseg_conv_wgrad_det_at_cdseg_wgrad_det_ws_bytes(ops, lp):
    from tests.test_gpu_wgrad16 import _kernel_map
    t = torch.float32 if lp == "fp32" else LP()
    code = _lib.F32 if lp == "fp32" else _lib.BF16
    lib = _lib.load()
    g = torch.Generator().manual_seed(5)
    for M, K, N in ((2100, 32, 96), (5003, 64, 192)):
        assert ops.wgrad_partition(M, N, K, 1, t).splits >= 3
        x, dy = dev(torch.randn(M, K, generator=g), t), dev(0.1 * torch.randn(M, N, generator=g), t)

        def lin():
            dw, db = torch.zeros(N, K, device="cuda"), torch.zeros(N, device="cuda")
            ops.linear_wgrad(x, dy, dw, db, deterministic=True)
            return dw, db

        _exact_vs_today(ops, lin, attrs=("_scratch",), sizes=[max(16, lib.cdseg_wgrad_det_ws_bytes(M, N, K, 1, code))])
    nbr = _kernel_map(ops, "batch2", 3)
    m = nbr.shape[1]
    xc, dyc = dev(torch.randn(m, 32, generator=g), t), dev(torch.randn(m, 32, generator=g), t)

    def conv():
        dw3, db3 = torch.zeros(32, 27, 32, device="cuda"), torch.zeros(32, device="cuda")
        ops.conv_wgrad(xc, nbr, dyc, dw3, db3, deterministic=True)
        return dw3, db3

    _exact_vs_today(ops, conv, attrs=("_scratch",), sizes=[max(16, lib.cdseg_wgrad_det_ws_bytes(m, 32, 32, 27, code))])


@pytest.mark.parametrize("m,c", [(2, 16), (65, 48), (777, 512), (5003, 64)])
def test_cdseg_bn_stats_and_cdseg_bn_gelu_bwd_sums_at_cdseg_bn_ws_bytes(ops, m, c):
    from tests.test_gpu_norm import _data, _fused
    x, dy, gamma, beta, rm, rv = _data(m, c, m + c)

    def run():
        r = _fused(ops, x, dy, gamma, beta, rm, rv)
        return [r[k] for k in ("y", "dx", "stats", "gsums", "mean", "invstd", "rm", "rv")]

    _exact_vs_today(ops, run, attrs=("_scratch",), at_least=2, sizes=[max(16, _lib.load().cdseg_bn_ws_bytes(m, c))])


@LPS
@pytest.mark.parametrize("n,c,variant", [(1, 13, "ignore7"), (65, 16, "half"), (1000, 20, "strided"), (4099, 200, "lone")])
def test_cdseg_seg_loss_fwd_at_cdseg_seg_loss_ws_bytes(ops, lp, n, c, variant):
    from tests.test_gpu_seg_loss import IGNORE, make_case
    t, labels, win = make_case(n, c, variant)
    dev_t, lab = t.cuda(), labels.cuda()
    logits = dev_t if win is None else dev_t[:, win[0]:win[1]]

    def run():
        ce, lv, saved = ops.seg_loss(logits, lab, IGNORE)
        one = torch.tensor(1.0, dtype=torch.float32, device="cuda")
        return ce, lv, ops.seg_loss_bwd(logits, saved, one, None), ops.seg_loss_bwd(logits, saved, None, one)

    _exact_vs_today(ops, run, attrs=("_scratch",), sizes=[max(16, _lib.load().cdseg_seg_loss_ws_bytes(n, c))])


@LPS
@pytest.mark.parametrize("clip", [None, 0.5], ids=["no-clip", "cdseg_grad_norm"])
def test_cdseg_adamw_step_and_cdseg_grad_norm_at_cdseg_opt_ws_bytes(ops, lp, clip):
    from tests.test_gpu_optim import _fused, _inputs, _params, _set_grads, _state
    p0, gs = _inputs(11)

    def run():
        params = _params(p0)
        opt = _fused(params, **({} if clip is None else dict(max_grad_norm=clip)))
        for g in gs:
            _set_grads(params, g)
            opt.step()
        torch.cuda.synchronize()
        p, m, v = _state(opt, params)
        return [*p, *m, *v] + ([opt.last_grad_norm.clone()] if clip is not None else [])

    ex = _exact_vs_today(ops, run, attrs=("_scratch",))
    assert len(ex.served) == 1  # one workspace per optimizer, sized once by cdseg_opt_ws_bytes


# ------------------------------------------------------------------ training Block: tape, scratch, derived buffer, gradient slab
@pytest.mark.parametrize("tp,lp", [("fp32", "bf16"), ("fp16-amp", "f16")])
@pytest.mark.parametrize("C,H", [(32, 2), (512, 32)])
def test_cdseg_train_block_forward_and_backward_buffers_at_cdseg_train_block_bytes(ops, monkeypatch, tp, lp, C, H):
    """Every case of BLOCK_CASES at this width (tests/test_gpu_train_block.py), in the deterministic mode (fixed summation
    order: bit-equal results are the contract there): the tape, both scratch buffers, the derived-weight buffer and the
    gradient slab at exactly the four figures of cdseg_train_block_bytes."""
    from tests import test_gpu_train_block as TB
    graph = TB._graph
    monkeypatch.setattr(TB, "_graph", lambda tp_, mode, training=True, det=False: graph(tp_, mode, training, True))
    for case_key in [c for c in TB.BLOCK_CASES if c[0] == C]:
        case = TB._case(*case_key)

        def run():
            out, _ = TB._run_block(case, C, H, tp, "native")
            return out

        ex = _exact_vs_today(ops, run, attrs=("_scratch",), at_least=5)  # derived, tape, scratch, slab, scratch
        assert all(b.nbytes > 0 for b in ex.served[:2]), case_key
