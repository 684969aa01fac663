"""GPU: every HIP kernel, called through the C ABI (cdsegnet_amd.ops -> libcdseg_hip.so), against
the CPU oracle on the same seeded inputs.  Integer work must be bit-exact; fp32 kernels within
1e-4..1e-3 of the fp32 oracle (tolerances written at each assert); bf16 kernels within bf16
rounding of the fp32 oracle evaluated on bf16-rounded inputs."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import model as OM
from oracle import serialization as S
from tests.helpers import load_fixture

pytestmark = pytest.mark.gpu

CLOUDS = ["tiny64", "room1500", "batch2", "lidar5000", "rand16", "lidar8"]


@pytest.fixture(scope="module")
def ops():
    from cdsegnet_amd import ops as _ops
    assert torch.cuda.is_available()
    return _ops


_CUR = {"lp": torch.bfloat16}


def LP():
    return _CUR["lp"]


@pytest.fixture(autouse=True)
def _library_variant(request):
    """Tests parametrised with dtype=float16 or lp="f16" run against the IEEE-half build of the library."""
    from cdsegnet_amd import _lib
    params = getattr(getattr(request.node, "callspec", None), "params", {})
    variant = "f16" if (params.get("dtype") == torch.float16 or params.get("lp") == "f16") else "bf16"
    _CUR["lp"] = {"bf16": torch.bfloat16, "f16": torch.float16}[variant]
    with _lib.use(variant):
        yield
    _CUR["lp"] = torch.bfloat16


LPS = pytest.mark.parametrize("lp", ["bf16", "f16"])


def dev(x, dtype=None):
    t = torch.as_tensor(x)
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


def report(name, **kw):
    print(f"[measure] {name}: " + ", ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in kw.items()))


# ------------------------------------------------------------------ integer kernels (bit-exact)
@pytest.mark.parametrize("name", CLOUDS)
def test_serialization_bit_exact_vs_reference_golden(ops, name):
    fx = load_fixture(f"serialization_{name}.npz")
    grid, batch = dev(fx["grid_coord"]), dev(fx["batch"])
    assert int(ops.grid_max(grid).item()).bit_length() == int(fx["depth"])
    b32 = ops.offset2batch(dev(fx["offset"]), len(fx["batch"]))
    assert np.array_equal(b32.cpu().numpy(), fx["batch"])
    code, order, inverse, depth = ops.serialization(grid, batch)
    assert depth == int(fx["depth"])
    assert np.array_equal(code.cpu().numpy(), fx["code"])
    assert np.array_equal(order.cpu().numpy(), fx["order"])
    assert np.array_equal(inverse.cpu().numpy(), fx["inverse"])
    # int32 grid / batch inputs take a different kernel instantiation
    for o in range(4):
        c = ops.encode(grid.int(), batch.int(), depth, o)
        assert np.array_equal(c.cpu().numpy(), fx["code"][o])


def test_encode_known_answers_and_empty(ops):
    ka = load_fixture("known_answers.npz")
    g = dev(ka["grid"])
    for o in S.ORDERS:
        assert np.array_equal(ops.encode(g, None, 9, o).cpu().numpy(), ka[o])
    empty = torch.empty((0, 3), dtype=torch.int64, device="cuda")
    assert ops.encode(empty, None, 9, "z").numel() == 0


def test_sort_pairs_large_random(ops):
    rng = np.random.default_rng(0)
    keys = rng.integers(0, 2 ** 48, 300000)
    ks, perm = ops.sort_pairs(dev(keys), None, end_bit=48)
    ref = np.argsort(keys, kind="stable")
    assert np.array_equal(perm.cpu().numpy(), ref)
    assert np.array_equal(ks.cpu().numpy(), keys[ref])
    inv = ops.invert_perm(perm).cpu().numpy()
    assert np.array_equal(inv[ref], np.arange(len(keys)))


def _physical(ops, fx):
    """z-sorted ("physical") view of a fixture cloud, the engine's internal layout."""
    grid, batch = dev(fx["grid_coord"]), dev(fx["batch"])
    depth = int(fx["depth"])
    zc = ops.encode(grid, batch, depth, "z")
    zs, perm0 = ops.sort_pairs(zc)
    g0, b0 = ops.plan_gather_grid(grid, perm0, zs, depth)
    p = perm0.cpu().numpy()
    assert np.array_equal(g0.cpu().numpy(), fx["grid_coord"][p])
    assert np.array_equal(b0.cpu().numpy(), fx["batch"][p])
    return zs, perm0, g0, b0, depth, p


@pytest.mark.parametrize("name", CLOUDS)
@pytest.mark.parametrize("pd", [1, 2])
def test_pooling_structure_vs_reference_golden(ops, name, pd):
    fx = load_fixture(f"serialization_{name}.npz")
    stride = {1: 2, 2: 4}[pd]
    zs, perm0, g0, b0, depth, p = _physical(ops, fx)
    n = len(p)
    code4 = ops.encode4(g0, b0, depth)
    assert np.array_equal(code4.cpu().numpy(), fx["code"][:, p])
    cluster, seg, cnt = ops.pool_level(zs, 3 * pd)
    m = int(cnt.item())
    ref_cluster = fx[f"pool{stride}_cluster"]
    assert m == ref_cluster.max() + 1
    cl = cluster.cpu().numpy()
    # same partition as the reference (cluster ids are numbered by the z curve here, by code[0] = z there)
    assert np.array_equal(cl, ref_cluster[p])
    sg = seg.cpu().numpy()[:m + 1]
    assert sg[0] == 0 and sg[-1] == n and np.all(np.diff(sg) > 0)
    assert np.array_equal(cl[sg[:-1]], np.arange(m)) and np.all(np.diff(cl) >= 0)
    gc, bc, cc = ops.pool_gather(seg, m, n, pd, g0, b0, code4)
    # pooled level is again z-sorted: compare with the reference's pooled arrays sorted by its z code
    rorder = fx[f"pool{stride}_order"][0]
    assert np.array_equal(cc.cpu().numpy(), fx[f"pool{stride}_code"][:, rorder])
    assert np.array_equal(gc.cpu().numpy(), fx[f"pool{stride}_grid"][rorder])
    assert np.array_equal(bc.cpu().numpy(), fx[f"pool{stride}_batch"][rorder])


@pytest.mark.parametrize("name", ["room1500", "batch2", "lidar5000"])
@pytest.mark.parametrize("ksize", [3, 5])
def test_neighbour_table_vs_oracle(ops, name, ksize):
    fx = load_fixture(f"serialization_{name}.npz")
    zs, perm0, g0, b0, depth, p = _physical(ops, fx)
    ref = OM.subm_neighbors(fx["grid_coord"][p], fx["batch"][p], ksize)  # indices already in physical numbering
    nbr = ops.nbr_table(zs, g0, b0, depth, ksize).cpu().numpy()
    assert np.array_equal(nbr, ref)
    nbr_t = ops.nbr_table(zs, g0, b0, depth, ksize, kmajor=True).cpu().numpy()
    assert np.array_equal(nbr_t, ref.T)


@pytest.mark.parametrize("name", CLOUDS)
@pytest.mark.parametrize("K", [4, 16, 1024])
def test_pad_plan_vs_reference_golden(ops, name, K):
    fx = load_fixture(f"serialization_{name}.npz")
    pad, unpad = fx[f"pad_K{K}"], fx[f"unpad_K{K}"]
    n = len(fx["batch"])
    offs = np.concatenate([[0], fx["offset"]]).astype(np.int32)
    counts = np.diff(offs)
    pc = np.where(counts > K, (counts + K - 1) // K * K, counts)
    offs_pad = np.concatenate([[0], np.cumsum(pc)]).astype(np.int32)
    assert offs_pad[-1] == len(pad)
    order = fx["order"][2].astype(np.int32)  # any curve; ranks -> rows
    gidx, widx = ops.pad_plan(dev(order), dev(offs), dev(offs_pad), K, int(offs_pad[-1]))
    gidx, widx = gidx.cpu().numpy(), widx.cpu().numpy()
    assert np.array_equal(gidx, order[pad])  # ptv3.py:259: order = serialized_order[i][pad]
    # ptv3.py:260 inverse = unpad[serialized_inverse]: the kept slot of point j is unpad[rank_j]
    inv = fx["inverse"][2]
    kept = np.full(len(pad), -1, dtype=np.int64)
    kept[unpad[inv]] = np.arange(n)
    assert np.array_equal(widx, kept)
    g2, w2 = ops.pad_plan(None, dev(offs), dev(offs_pad), K, int(offs_pad[-1]))
    assert np.array_equal(g2.cpu().numpy(), pad)


# ------------------------------------------------------------------ GEMM
def _bf16_round(x):
    """Round to the 16-bit type of the library build under test (bfloat16, or IEEE half for the `float16` / lp="f16"
    parametrisations: the same sources compiled with -DCDSEG_LP_F16, cdsegnet_amd/libcdseg_hip_f16.so)."""
    return x.to(LP()).to(torch.float32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,N,K", [(1000, 96, 32), (777, 20, 64), (4096, 128, 128), (300, 512, 512), (65, 2048, 512),
                                   (130, 40, 16), (5000, 64, 2048)])
def test_gemm_plain(ops, dtype, M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g)
    if dtype != torch.float32:
        A, W = _bf16_round(A), _bf16_round(W)
    ref = A.double() @ W.double().t() + b.double()
    out = torch.empty(M, N, dtype=torch.float32, device="cuda")
    ops.gemm(dev(A, dtype), dev(W, dtype), out, bias=dev(b))
    err = (out.cpu().double() - ref).abs().max().item()
    report(f"gemm {dtype} {M}x{N}x{K}", max_err=err)
    assert err < (2e-5 * K ** 0.5 + 1e-5)  # fp32 accumulation of exactly-representable products
    # GELU + residual + second (bf16) copy, asymmetric on purpose (catches transposed C layouts)
    out2 = torch.empty(M, N, dtype=LP(), device="cuda")
    ops.gemm(dev(A, dtype), dev(W, dtype), out, bias=dev(b), act=ops.ACT_GELU, res=dev(res), out2=out2)
    ref2 = F.gelu(ref.float()).double() + res.double()
    err2 = (out.cpu().double() - ref2).abs().max().item()
    assert err2 < (2e-5 * K ** 0.5 + 1e-4), err2
    assert (out2.float().cpu() - ref2.float()).abs().max().item() < 0.02 * ref2.abs().max().item() + 1e-2


@LPS
def test_gemm_16bit_outputs_saturate_in_the_half_build(ops, lp):
    """IEEE half ends at 65504: the half build clamps on conversion (an outlier activation of a trained checkpoint must
    not turn the rest of the forward into inf / NaN); the bfloat16 build has fp32's range and stores the value."""
    M, N, K = 256, 128, 64
    A = torch.full((M, K), 300.0)
    W = torch.full((N, K), 300.0)
    W[::2] *= -1
    out = torch.empty(M, N, dtype=LP(), device="cuda")
    ops.gemm(dev(A, LP()), dev(W, LP()), out)
    got = out.float().cpu()
    assert torch.isfinite(got).all()
    want = 300.0 * 300.0 * K
    if lp == "f16":
        assert torch.equal(got[:, 1::2], torch.full((M, N // 2), 65504.0)) and torch.equal(got[:, ::2], torch.full((M, N // 2), -65504.0))
    else:
        assert (got[:, 1::2] - want).abs().max() <= want * 2 ** -8 and (got[:, ::2] + want).abs().max() <= want * 2 ** -8


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_gemm_epilogue_bn_gather_add_scatter(ops, dtype):
    g = torch.Generator().manual_seed(3)
    M, N, K, Mc = 1500, 64, 128, 400
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    if dtype != torch.float32:
        A, W = _bf16_round(A), _bf16_round(W)
    b, sc, sh = torch.randn(N, generator=g), torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g)
    child = torch.randn(Mc, N, generator=g)
    idx = torch.randint(0, Mc, (M,), generator=g).int()
    perm = torch.randperm(M, generator=g).int()
    pre = F.gelu(((A.double() @ W.double().t() + b.double()) * sc.double() + sh.double()).float())
    ref = pre + child[idx.long()]
    out = torch.zeros(M, N, dtype=torch.float32, device="cuda")
    out2 = torch.zeros(M, N, dtype=dtype, device="cuda")
    ops.gemm(dev(A, dtype), dev(W, dtype), out, bias=dev(b), scale=dev(sc), shift=dev(sh), act=ops.ACT_GELU,
             add_src=dev(child), add_idx=dev(idx), out_idx=dev(perm), out2=out2, out2_pre_add=True)
    got = out.cpu()
    assert (got[perm.long()] - ref).abs().max().item() < 5e-4
    tol2 = 1e-4 if dtype == torch.float32 else 0.03
    assert (out2.float().cpu() - pre).abs().max().item() < tol2 * (1 + pre.abs().max().item())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name,C", [("room1500", 32), ("batch2", 64), ("lidar5000", 16), ("room1500", 128),
                                    ("room1500", 256), ("lidar8", 512)])  # C >= 256: deep-stage widths (the 16-bit builds: 128-row LDS-DMA tiles)
def test_sparse_conv_gemm_vs_oracle(ops, dtype, name, C):
    fx = load_fixture(f"serialization_{name}.npz")
    zs, perm0, g0, b0, depth, p = _physical(ops, fx)
    n = len(p)
    nbr = ops.nbr_table(zs, g0, b0, depth, 3)
    g = torch.Generator().manual_seed(C)
    x = torch.randn(n, C, generator=g)
    w = torch.randn(C, 3, 3, 3, C, generator=g) / (27 * C) ** 0.5
    b = torch.randn(C, generator=g)
    if dtype != torch.float32:
        x, w = _bf16_round(x), _bf16_round(w)
    ref = OM.subm_conv3d(x, nbr.cpu().numpy().astype(np.int64), w, b)
    out = torch.empty(n, C, dtype=torch.float32, device="cuda")
    ops.gemm(dev(x, dtype), dev(w.reshape(C, -1), dtype), out, bias=dev(b), nbr=nbr, kvol=27)
    err = (out.cpu() - ref).abs().max().item()
    report(f"conv {dtype} {name} C={C}", max_err=err)
    assert err < 2e-4


@LPS
@pytest.mark.parametrize("name,C", [("room1500", 32), ("batch2", 64), ("lidar5000", 32), ("lidar8", 64), ("tiny64", 32),
                                    ("rand16", 64)])
def test_subm_conv3_weight_stationary_vs_oracle(ops, lp, name, C):
    """csrc/conv.hip (W resident in LDS, gathered rows straight into MFMA fragments, C = 32 / 64 bf16) against the
    oracle's subm_conv3d on bf16-rounded operands, and against the gathered-A GEMM it replaces (same inputs; different
    summation order only).  Row counts that are not a multiple of the 256-row block, rows with no neighbour but
    themselves (rand16), all 27 offsets (corner offsets of the C = 64 kernel come from L2)."""
    fx = load_fixture(f"serialization_{name}.npz")
    zs, perm0, g0, b0, depth, p = _physical(ops, fx)
    n = len(p)
    nbr = ops.nbr_table(zs, g0, b0, depth, 3, True)
    g = torch.Generator().manual_seed(C + n)
    x = _bf16_round(torch.randn(n, C, generator=g))
    w = _bf16_round(torch.randn(C, 3, 3, 3, C, generator=g) / (27 * C) ** 0.5)
    b = torch.randn(C, generator=g)
    ref = OM.subm_conv3d(x, nbr.t().cpu().numpy().astype(np.int64), w, b)
    xd, wd = dev(x, LP()), dev(w.reshape(C, -1), LP())
    assert ops.subm_conv3_ok(xd)
    img = ops.subm_conv3_pack(wd)
    out = torch.full((n, C), float("nan"), dtype=LP(), device="cuda")
    ops.subm_conv3(xd, img, dev(b), nbr, out)
    old = torch.empty(n, C, dtype=LP(), device="cuda")
    ops.gemm(xd, wd, old, bias=dev(b), nbr=nbr, nbr_kmajor=True, kvol=27)
    err = (out.float().cpu() - ref).abs().max().item()
    err_old = (old.float().cpu() - ref).abs().max().item()
    report(f"subm_conv3 {name} C={C}", max_err=err, gathered_gemm_err=err_old)
    scale = 1 + ref.abs().max().item()
    assert err < 0.01 * scale  # one bf16 rounding of the output (2^-9 relative)
    assert torch.isfinite(out.float()).all()


@LPS
def test_subm_conv3_large_random_map(ops, lp):
    """120k-row scene map, both widths, and bias = None; compares with the gathered-A GEMM on the same bf16 operands
    (fp32 accumulation in both: equal up to summation order, then one bf16 rounding)."""
    from cdsegnet_amd import synth
    sc = synth.room_scene(2, 120000)
    grid = torch.as_tensor(sc["grid_coord"]).cuda()
    batch = torch.zeros(len(grid), dtype=torch.int64, device="cuda")
    depth = int(ops.grid_max(grid).item()).bit_length()
    zs, perm0 = ops.sort_pairs(ops.encode(grid, batch, depth, "z"))
    g0, b0 = ops.plan_gather_grid(grid, perm0, zs, depth)
    nbr = ops.nbr_table(zs, g0, b0, depth, 3, True)
    n = len(grid)
    for C in (32, 64):
        g = torch.Generator().manual_seed(C)
        x = torch.randn(n, C, generator=g).cuda().to(LP())
        w = (torch.randn(C, 27 * C, generator=g) / (27 * C) ** 0.5).cuda().to(LP())
        out = torch.empty(n, C, dtype=LP(), device="cuda")
        ops.subm_conv3(x, ops.subm_conv3_pack(w), None, nbr, out)
        old = torch.empty(n, C, dtype=torch.float32, device="cuda")
        ops.gemm(x, w, old, nbr=nbr, nbr_kmajor=True, kvol=27)
        err = (out.float() - old).abs().max().item()
        report(f"subm_conv3 120k C={C} vs gathered GEMM (fp32 out)", max_err=err)
        assert err < 0.01 * (1 + old.abs().max().item())
        out2 = torch.empty_like(out)
        ops.subm_conv3(x, ops.subm_conv3_pack(w), None, nbr, out2)
        assert torch.equal(out, out2)  # deterministic


@LPS
@pytest.mark.parametrize("C", [32, 64])
def test_subm_conv3_strided_rows(ops, lp, C):
    """Input and output as column slices of wider buffers (row stride 2C: a power-of-two byte stride, as the ABI asks);
    the untouched halves keep their contents."""
    fx = load_fixture("serialization_lidar5000.npz")
    zs, perm0, g0, b0, depth, p = _physical(ops, fx)
    n = len(p)
    nbr = ops.nbr_table(zs, g0, b0, depth, 3, True)
    g = torch.Generator().manual_seed(7 * C)
    xw = torch.randn(n, 2 * C, generator=g).cuda().to(LP())
    w = (torch.randn(C, 27 * C, generator=g) / (27 * C) ** 0.5).cuda().to(LP())
    b = torch.randn(C, generator=g).cuda()
    img = ops.subm_conv3_pack(w)
    dense = torch.empty(n, C, dtype=LP(), device="cuda")
    ops.subm_conv3(xw[:, C:].contiguous(), img, b, nbr, dense)
    yw = torch.full((n, 2 * C), 3.0, dtype=LP(), device="cuda")
    ops.subm_conv3(xw[:, C:], img, b, nbr, yw[:, :C])
    assert torch.equal(yw[:, :C], dense)
    assert torch.equal(yw[:, C:], torch.full((n, C), 3.0, dtype=LP(), device="cuda"))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,N,K", [(1000, 32, 32), (4097, 64, 64), (130, 128, 128), (70, 16, 16), (515, 48, 48),
                                   # rows over several column tiles: finished by the last block of the row tile
                                   (3364, 256, 256), (778, 512, 512), (300, 384, 384), (20000, 256, 256),
                                   # ... combined with split-K (few tiles, long K)
                                   (778, 512, 2048), (3364, 256, 1024), (100, 128, 4096), (70, 64, 2048)])
def test_gemm_fused_layernorm_epilogue(ops, dtype, M, N, K):
    """x = x + LN_a(A W^T + b) + colbias ; h = LN_b(x)   (the CPE + pre-norm chain, ptv3.py:401-413)
    and x = x + (A W^T + b) ; h = LN_b(x)                (attention proj + norm2, ptv3.py:416-421)."""
    g = torch.Generator().manual_seed(M + N)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    if dtype != torch.float32:
        A, W = _bf16_round(A), _bf16_round(W)
    b, res, cb = torch.randn(N, generator=g), torch.randn(M, N, generator=g), torch.randn(N, generator=g)
    g1, b1 = torch.randn(N, generator=g), torch.randn(N, generator=g)
    g2, b2 = torch.randn(N, generator=g), torch.randn(N, generator=g)
    y = (A.double() @ W.double().t() + b.double()).float()
    x_ref = res + F.layer_norm(y, (N,), g1, b1, 1e-5) + cb
    h_ref = F.layer_norm(x_ref, (N,), g2, b2, 1e-5)
    x = dev(res)
    h = torch.empty(M, N, dtype=dtype, device="cuda")
    with ops.record_routes() as rr:
        ops.gemm(dev(A, dtype), dev(W, dtype), x, bias=dev(b), ln_pre=(dev(g1), dev(b1)), res=x, colbias=dev(cb),
                 ln_post=(dev(g2), dev(b2)), ln_out=h)
    routes = list(rr.routes)
    tol_h = 2e-4 if dtype == torch.float32 else 0.03
    assert (x.cpu() - x_ref).abs().max().item() < 2e-4 + 2e-5 * K ** 0.5
    assert (h.float().cpu() - h_ref).abs().max().item() < tol_h * (1 + h_ref.abs().max().item())
    x2_ref = res + y
    h2_ref = F.layer_norm(x2_ref, (N,), g2, b2, 1e-5)
    x2 = dev(res)
    with ops.record_routes() as rr:
        ops.gemm(dev(A, dtype), dev(W, dtype), x2, bias=dev(b), res=x2, ln_post=(dev(g2), dev(b2)), ln_out=h)
    routes += rr.routes
    assert (x2.cpu() - x2_ref).abs().max().item() < 2e-4 + 2e-5 * K ** 0.5
    assert (h.float().cpu() - h2_ref).abs().max().item() < tol_h * (1 + h2_ref.abs().max().item())
    # tile semaphores are left clean: the same call again gives the same bits
    x3 = dev(res)
    h3 = torch.empty_like(h)
    with ops.record_routes() as rr:
        ops.gemm(dev(A, dtype), dev(W, dtype), x3, bias=dev(b), res=x3, ln_post=(dev(g2), dev(b2)), ln_out=h3)
    routes += rr.routes
    assert torch.equal(x3, x2) and torch.equal(h3, h)
    # the launch record: rows of one column tile (N <= 128) are finished in the tile (fix 0), wider rows by the row-finish pass
    # (fix 2), with split-K where the rule gives it: 16 K steps or more (a step is 128 elements in 16 bits, 64 in fp32)
    fix = 0 if N <= 128 and K < 2048 else 2
    split = K >= 2048 or (K == 1024 and dtype == torch.float32)
    assert [(r.fix, r.splits > 1) for r in routes] == [(fix, split)] * 3, routes


@pytest.fixture
def x3(ops):
    """This thread's fp32 products in the split-half "fp32 x3" form (ops.set_f32x3) for the duration of a test."""
    prev = ops.set_f32x3(True)
    yield
    ops.set_f32x3(prev)


@pytest.mark.parametrize("M,N,K", [(1000, 96, 32), (777, 20, 64), (4096, 128, 128), (300, 512, 512), (65, 2048, 512),
                                   (130, 40, 16), (5000, 64, 2048), (448, 512, 2048), (3392, 256, 256)])
def test_gemm_fp32x3_is_as_good_as_fp32_on_fp32_operands(ops, x3, M, N, K):
    """Round 6, CDSEG_F32X3 (csrc/gemm.hip): fp32 A and W, every value split into an IEEE-half pair on its way into LDS
    (x ~= hi + lo' / 2048), three half MFMAs per product, fp32 accumulation.  Against fp64 on operands that are NOT exactly
    representable in 16 bits, incl. tiny magnitudes (the scaled low part keeps them out of half's subnormals) and the
    split-K / GELU / residual / second-output epilogues: the error bound of the exact-fp32 kernel, doubled."""
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g)
    A[:, ::3] *= 1e-4  # small activations next to O(1) ones
    W = torch.randn(N, K, generator=g) / K ** 0.5
    b, res = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    ref = A.double() @ W.double().t() + b.double()
    out = torch.empty(M, N, dtype=torch.float32, device="cuda")
    ops.gemm(dev(A), dev(W), out, bias=dev(b))
    err = (out.cpu().double() - ref).abs().max().item()
    prev = ops.set_f32x3(False)
    exact = torch.empty_like(out)
    ops.gemm(dev(A), dev(W), exact, bias=dev(b))
    ops.set_f32x3(prev)
    err32 = (exact.cpu().double() - ref).abs().max().item()
    report(f"gemm fp32x3 {M}x{N}x{K}", max_err=err, exact_fp32_err=err32)
    assert err < 2 * (2e-5 * K ** 0.5 + 1e-5) and err < 8 * err32 + 2e-6
    out2 = torch.empty(M, N, dtype=torch.float32, device="cuda")
    ops.gemm(dev(A), dev(W), out, bias=dev(b), act=ops.ACT_GELU, res=dev(res), out2=out2)
    ref2 = F.gelu(ref.float()).double() + res.double()
    assert (out.cpu().double() - ref2).abs().max().item() < 2 * (2e-5 * K ** 0.5 + 1e-4)
    assert torch.equal(out2, out)


def test_sparse_conv_and_layernorm_epilogue_fp32x3(ops, x3):
    """The gathered (sparse-conv) form and the LayerNorm-fused epilogue run on the same kernel: fp32x3 vs the oracle conv /
    fp64 LayerNorm."""
    fx = load_fixture("serialization_lidar5000.npz")
    zs, perm0, g0, b0, depth, p = _physical(ops, fx)
    nbr = ops.nbr_table(zs, g0, b0, depth, 3)
    C = 128
    g = torch.Generator().manual_seed(6)
    x = torch.randn(len(p), C, generator=g)
    w = torch.randn(C, 27, C, generator=g) / (27 * C) ** 0.5
    b = torch.randn(C, generator=g)
    ref = OM.subm_conv3d(x, nbr.cpu().numpy().astype(np.int64), w.reshape(C, 3, 3, 3, C), b)
    out = torch.empty(len(p), C, dtype=torch.float32, device="cuda")
    ops.gemm(dev(x), dev(w.reshape(C, -1)), out, bias=dev(b), nbr=nbr, kvol=27)
    err = (out.cpu() - ref).abs().max().item()
    report("conv fp32x3 C=128", max_err=err)
    assert err < 5e-5
    M, N, K = 3000, 256, 256
    A, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
    bias, ga, be, res = (torch.randn(N, generator=g) for _ in range(3)), None, None, None
    bias, ga, be = bias
    res = torch.randn(M, N, generator=g)
    t = A.double() @ W.double().t() + bias.double()
    want = res.double() + F.layer_norm(t, (N,), ga.double(), be.double(), 1e-5)
    xo = dev(res)
    ops.gemm(dev(A), dev(W), xo, bias=dev(bias), ln_pre=(dev(ga), dev(be)), res=xo)
    assert (xo.cpu().double() - want).abs().max().item() < 1e-4


@pytest.mark.parametrize("lens,H,K", [([2500], 2, 1024), ([1024], 4, 1024), ([991], 32, 1024), ([26], 4, 1024),
                                      ([1500, 1100], 2, 1024), ([700, 500, 3000], 1, 1024), ([10], 1, 4),
                                      ([100, 37], 2, 16), ([1025], 8, 1024), ([33], 2, 1024)])
def test_attention_fp32x3_vs_oracle(ops, x3, lens, H, K):
    """attn_x3_kernel: fp32 q / k / v, half pairs for the scores, bfloat16 pairs for P V - against the oracle's fp32 attention
    on the same UNROUNDED inputs; and the cross form."""
    err, mag = _attention_case(ops, torch.float32, lens, H, K, seed=sum(lens) + H)
    report(f"attn fp32x3 lens={lens} H={H} K={K}", max_err=err, ref_max=mag)
    assert err < 4e-5 * (1 + mag)
    err, mag = _attention_case(ops, torch.float32, lens, H, K, seed=sum(lens) + H + 1, cross=True)
    assert err < 4e-5 * (1 + mag)


def test_attention_fp32x3_takes_the_exact_pass_on_scores_outside_fp32_range(ops, x3):
    g = torch.Generator().manual_seed(0)
    n, H = 1024, 2
    C = 16 * H
    qkv = torch.randn(n, 3 * C, generator=g)
    qkv[:, :2 * C] *= 6.0
    order = torch.randperm(n, generator=g).numpy()
    inverse = np.empty(n, dtype=np.int64)
    inverse[order] = np.arange(n)
    t_order = torch.from_numpy(order)
    ref = OM._patch_attention(qkv[:, :C][t_order], qkv[:, C:2 * C][t_order], qkv[:, 2 * C:][t_order],
                              np.array([0, n]), H, 0.25)[torch.from_numpy(inverse)]
    offs = dev(np.array([0, n], dtype=np.int32))
    gq, wq = ops.pad_plan(dev(order.astype(np.int32)), offs, offs, 1024, n)
    d = dev(qkv)
    out = torch.empty(n, C, dtype=torch.float32, device="cuda")
    ops.attention(d[:, :C], d[:, C:2 * C], d[:, 2 * C:], gq, gq, wq, offs, H, n, 0.25, out)
    assert (out.cpu() - ref).abs().max().item() < 2e-4


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,N,K", [(448, 512, 2048), (832, 1536, 512), (100, 256, 4096), (3392, 256, 256)])
def test_gemm_split_k(ops, dtype, M, N, K):
    """Few output tiles + long K -> the split-K path (partials in the workspace, finished by the last block).  The launch record
    shows that only the K = 2048 and K = 4096 shapes split under today's rule (16 K steps or more); (832, 1536, 512) and
    (3392, 256, 256) run unsplit and are kept here as plain few-tile GEMMs with the same epilogue, asserted as such.  The split-K
    routes themselves, kernel by kernel, are held by tests/test_gpu_routes.py."""
    g = torch.Generator().manual_seed(M + N)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    b, res = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    if dtype != torch.float32:
        A, W = _bf16_round(A), _bf16_round(W)
    ref = F.gelu((A.double() @ W.double().t() + b.double()).float()).double() + res.double()
    out = dev(res)
    out2 = torch.empty(M, N, dtype=dtype, device="cuda")
    with ops.record_routes() as rr:
        ops.gemm(dev(A, dtype), dev(W, dtype), out, bias=dev(b), act=ops.ACT_GELU, res=out, out2=out2)
    err = (out.cpu().double() - ref).abs().max().item()
    report(f"split-k gemm {dtype} {M}x{N}x{K}", max_err=err)
    assert err < 2e-5 * K ** 0.5 + 1e-4
    again = dev(res)
    with ops.record_routes() as rr2:
        ops.gemm(dev(A, dtype), dev(W, dtype), again, bias=dev(b), act=ops.ACT_GELU, res=again)
    assert torch.equal(again, out), "split-K must be deterministic"
    # the launch record.  A plain GEMM splits from 16 K steps (128 elements per step in 16 bits, 64 in fp32) and below 256 tiles:
    # K = 2048 and 4096 do, K = 512 and 256 have at most 8 steps and run unsplit in every dtype - two of the four cases no
    # longer reach the path this test is named after; tests/test_gpu_routes.py holds the split-K routes case by case.
    split = K >= 2048
    for r in (rr.routes, rr2.routes):
        assert [(x.fix, x.splits > 1) for x in r] == [(1 if split else 0, split)], r


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_sparse_conv_split_k_deep_stage(ops, dtype):
    """Stage-4-like conv: a few hundred points, C = 512 (K = 27 * 512)."""
    fx = load_fixture("serialization_lidar5000.npz")
    zs, perm0, g0, b0, depth, p = _physical(ops, fx)
    cl, seg, cnt = ops.pool_level(zs, 9)
    m = int(cnt.item())
    gc, bc, cc = ops.pool_gather(seg, m, len(p), 3, g0, b0, ops.encode4(g0, b0, depth))
    nbr = ops.nbr_table(cc[0].contiguous(), gc, bc, depth - 3, 3)
    C = 512
    g = torch.Generator().manual_seed(5)
    x = torch.randn(m, C, generator=g)
    w = torch.randn(C, 27, C, generator=g) / (27 * C) ** 0.5
    b = torch.randn(C, generator=g)
    if dtype != torch.float32:
        x, w = _bf16_round(x), _bf16_round(w)
    ref = OM.subm_conv3d(x, nbr.cpu().numpy().astype(np.int64), w.reshape(C, 3, 3, 3, C), b)
    out = torch.empty(m, C, dtype=torch.float32, device="cuda")
    with ops.record_routes() as rr:
        ops.gemm(dev(x, dtype), dev(w.reshape(C, -1), dtype), out, bias=dev(b), nbr=nbr, kvol=27)
    assert [(r.fix, r.splits > 1, r.gather) for r in rr.routes] == [(1, True, True)], rr.routes  # the launch record: split-K
    err = (out.cpu() - ref).abs().max().item()
    report(f"deep conv {dtype} M={m} C={C}", max_err=err)
    assert err < 5e-4


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name,cin,cout", [("room1500", 6, 32), ("lidar5000", 4, 16), ("batch2", 6, 64)])
def test_stem_as_gathered_gemm_vs_oracle(ops, dtype, name, cin, cout):
    """The engine's stem: input rows gathered/padded to 8 channels, k=5 conv (125 offsets) on the MFMA GEMM,
    folded BN + GELU in the epilogue."""
    fx = load_fixture(f"serialization_{name}.npz")
    zs, perm0, g0, b0, depth, p = _physical(ops, fx)
    n = len(p)
    nbr = ops.nbr_table(zs, g0, b0, depth, 5)
    g = torch.Generator().manual_seed(cin + cout)
    x = torch.randn(n, cin, generator=g)  # caller order
    w = torch.randn(cout, 5, 5, 5, cin, generator=g) / (125 * cin) ** 0.5
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    if dtype != torch.float32:
        x, w = _bf16_round(x), _bf16_round(w)
    xp = x[torch.from_numpy(p)]
    ref = F.gelu(OM.subm_conv3d(xp, nbr.cpu().numpy().astype(np.int64), w, None) * sc + sh)
    a = ops.gather_pad_cast(dev(x), perm0, 8, dtype)
    assert torch.equal(a[:, :cin].float().cpu(), xp) and float(a[:, cin:].abs().max()) == 0.0
    wp = torch.zeros(cout, 125, 8)
    wp[:, :, :cin] = w.reshape(cout, 125, cin)
    out = torch.empty(n, cout, dtype=torch.float32, device="cuda")
    out2 = torch.empty(n, cout, dtype=dtype, device="cuda")
    ops.gemm(a, dev(wp.reshape(cout, -1), dtype), out, scale=dev(sc), shift=dev(sh), act=ops.ACT_GELU, nbr=nbr,
             kvol=125, out2=out2)
    err = (out.cpu() - ref).abs().max().item()
    report(f"stem gemm {dtype} {name}", max_err=err)
    assert err < 1e-4


@LPS
@pytest.mark.parametrize("name,cin", [("room1500", 6), ("lidar5000", 4), ("batch2", 6), ("lidar8", 4), ("rand16", 6), ("tiny64", 6)])
def test_stem5_map_free_vs_oracle(ops, lp, name, cin):
    """csrc/stem.hip: the k = 5 stem WITHOUT a 125-offset kernel map (neighbours enumerated through the parent level's
    3x3x3 map + per-parent octant masks), bf16 operands / fp32 accumulation, folded BN + GELU, against (a) the oracle's
    subm_conv3d on the explicit 5x5x5 map with the same bf16-rounded operands and (b) the gathered-A GEMM path it
    replaces.  Batches of 2 / 3 / 8 clouds: neighbours never cross batch elements (the parent map is per element)."""
    fx = load_fixture(f"serialization_{name}.npz")
    zs, perm0, g0, b0, depth, p = _physical(ops, fx)
    n = len(p)
    cluster, seg, cnt = ops.pool_level(zs, 3)
    m = int(cnt.item())
    code4 = ops.encode4(g0, b0, depth)
    g1, b1, c41 = ops.pool_gather(seg, m, n, 1, g0, b0, code4)
    pn3 = ops.nbr_table(c41[0].contiguous(), g1, b1, depth - 1, 3, True)
    cinfo = ops.child_info(zs, seg, m)
    nbr5 = ops.nbr_table(zs, g0, b0, depth, 5)
    g = torch.Generator().manual_seed(cin + n)
    x = _bf16_round(torch.randn(n, cin, generator=g))  # caller order
    w = _bf16_round(torch.randn(32, 5, 5, 5, cin, generator=g) / (125 * cin) ** 0.5)
    sc, sh = torch.rand(32, generator=g) + 0.5, torch.randn(32, generator=g)
    xp = x[torch.from_numpy(p)]
    ref = F.gelu(OM.subm_conv3d(xp, nbr5.cpu().numpy().astype(np.int64), w, None) * sc + sh)
    a = ops.gather_pad_cast(dev(x), perm0, 8, LP())
    wp = torch.zeros(32, 125, 8)
    wp[:, :, :cin] = w.reshape(32, 125, cin)
    wd = dev(wp.reshape(32, -1), LP())
    out = torch.full((n, 32), float("nan"), dtype=torch.float32, device="cuda")
    out2 = torch.empty(n, 32, dtype=LP(), device="cuda")
    ops.stem5(a, ops.stem5_pack(wd), dev(sc), dev(sh), g0, cluster, pn3, cinfo, depth, out, out2)
    old = torch.empty(n, 32, dtype=torch.float32, device="cuda")
    ops.gemm(a, wd, old, scale=dev(sc), shift=dev(sh), act=ops.ACT_GELU, nbr=nbr5, kvol=125)
    err = (out.cpu() - ref).abs().max().item()
    report(f"stem5 {name}", max_err=err, vs_gathered_gemm=(out - old).abs().max().item())
    assert err < 1e-4
    assert (out2.float() - out).abs().max().item() < 0.02 * (1 + out.abs().max().item())


# ------------------------------------------------------------------ LayerNorm / pooling reduce / small ops
@LPS
@pytest.mark.parametrize("C", [16, 32, 48, 64, 128, 256, 512, 2048])
def test_layernorm(ops, lp, C):
    g = torch.Generator().manual_seed(C)
    M = 1237
    x = torch.randn(M, C, generator=g) * 3 + 1
    gm, bt = torch.randn(C, generator=g), torch.randn(C, generator=g)
    res, cb = torch.randn(M, C, generator=g), torch.randn(C, generator=g)
    ref = F.layer_norm(x, (C,), gm, bt, 1e-5)
    out = torch.empty(M, C, dtype=torch.float32, device="cuda")
    ops.layernorm(dev(x), dev(gm), dev(bt), out)
    assert (out.cpu() - ref).abs().max().item() < 2e-5
    xr = dev(res)
    ops.layernorm(dev(x), dev(gm), dev(bt), xr, res=xr, colbias=dev(cb))  # in place on the residual
    assert (xr.cpu() - (ref + res + cb)).abs().max().item() < 2e-5
    ob = torch.empty(M, C, dtype=LP(), device="cuda")
    ops.layernorm(dev(x, LP()), dev(gm), dev(bt), ob)
    refb = F.layer_norm(_bf16_round(x), (C,), gm, bt, 1e-5)
    assert (ob.float().cpu() - refb).abs().max().item() < 0.02 * (1 + refb.abs().max().item())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_segment_max_and_mean(ops, dtype):
    g = torch.Generator().manual_seed(1)
    m, C = 700, 64
    counts = torch.randint(1, 9, (m,), generator=g)
    seg = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(counts, 0)])
    n = int(seg[-1])
    y = torch.randn(n, C, generator=g)
    if dtype != torch.float32:
        y = _bf16_round(y)
    sc, sh = torch.randn(C, generator=g), torch.randn(C, generator=g)  # negative scales too: max must come first
    cluster = np.repeat(np.arange(m), counts.numpy())
    ref = F.gelu(OM.segment_max(y, cluster, m) * sc + sh)
    out = torch.empty(m, C, dtype=torch.float32, device="cuda")
    out2 = torch.empty(m, C, dtype=LP(), device="cuda")
    ops.segment_max(dev(y, dtype), dev(seg.int()), m, dev(sc), dev(sh), ops.ACT_GELU, out, out2)
    assert (out.cpu() - ref).abs().max().item() < 1e-5
    assert (out2.float().cpu() - ref).abs().max().item() < 0.01 * (1 + ref.abs().max().item())
    xyz = torch.randn(n, 3, generator=g)
    mean = ops.segment_mean(dev(xyz), dev(seg.int()), m)
    assert (mean.cpu() - OM.segment_mean(xyz, cluster, m)).abs().max().item() < 1e-5


def test_timestep_embedding_chain(ops):
    """table row -> fc_t1 -> swish -> fc_t2 -> swish -> t_mlp == the reference's per-point chain (one row)."""
    from cdsegnet_amd.models import calc_t_emb_table
    ka = load_fixture("known_answers.npz")
    table = calc_t_emb_table(1000, 128)
    assert np.array_equal(table[999 + 1].numpy(), ka["t_emb_999_128"][0])  # row index = t + 1 (row 0 is t = -1)
    assert np.array_equal(table[[1, 2, 501, 1000]].numpy(), ka["t_emb_multi_128"])
    g = torch.Generator().manual_seed(0)
    w1, b1 = torch.randn(512, 128, generator=g) / 11, torch.randn(512, generator=g)
    w2, b2 = torch.randn(128, 512, generator=g) / 22, torch.randn(128, generator=g)
    ref = OM.swish(F.linear(OM.swish(F.linear(table[1000], w1, b1)), w2, b2))
    v = ops.gemv(dev(w1), dev(b1), dev(table[1000]), ops.ACT_SWISH)
    v = ops.gemv(dev(w2), dev(b2), v, ops.ACT_SWISH)
    assert (v.cpu() - ref).abs().max().item() < 1e-5


@LPS
def test_randn_cast_axpy_gather(ops, lp):
    z = ops.randn((1 << 20,), 1234, 0, torch.device("cuda")).cpu()
    assert abs(z.mean().item()) < 5e-3 and abs(z.std().item() - 1) < 5e-3
    assert abs((z ** 4).mean().item() - 3) < 0.05
    z2 = ops.randn((1 << 20,), 1234, 1, torch.device("cuda")).cpu()
    assert (z == z2).float().mean().item() < 1e-3
    assert torch.equal(ops.randn((1 << 20,), 1234, 0, torch.device("cuda")).cpu(), z)
    x = torch.randn(1000, 7)
    assert torch.equal(ops.cast(dev(x), LP()).cpu(), x.to(LP()))
    assert torch.allclose(ops.axpy(dev(x), dev(x), 0.5).cpu(), 1.5 * x)
    idx = torch.randint(0, 1000, (333,)).int()
    x8 = torch.randn(1000, 8)
    assert torch.equal(ops.gather_rows(dev(x8), dev(idx)).cpu(), x8[idx.long()])


# ------------------------------------------------------------------ attention
def _attention_case(ops, dtype, lens_pts, H, K, seed, cross=False):
    """lens_pts: points per batch element.  Builds the reference's padded patch structure with the oracle,
    runs the oracle attention on (bf16-rounded) inputs and the HIP kernel through the slot plan."""
    g = torch.Generator().manual_seed(seed)
    C = 16 * H
    offset = np.cumsum(lens_pts)
    n = int(offset[-1])
    qkv = torch.randn(n, 3 * C, generator=g)
    qkv[:, :C] *= 2.0  # sharper softmax
    if dtype != torch.float32:
        qkv = _bf16_round(qkv)
    # a random "serialized order" that keeps batch elements contiguous
    order = np.concatenate([s + torch.randperm(int(c), generator=g).numpy() for s, c in
                            zip(np.concatenate([[0], offset[:-1]]), lens_pts)]).astype(np.int64)
    order_kv = order if not cross else np.concatenate(
        [s + torch.randperm(int(c), generator=g).numpy() for s, c in zip(np.concatenate([[0], offset[:-1]]), lens_pts)])
    inverse = np.empty(n, dtype=np.int64)
    inverse[order] = np.arange(n)
    pad, unpad, cu = S.padding_plan(offset, K)
    q = qkv[:, :C][torch.from_numpy(order[pad])]
    k = qkv[:, C:2 * C][torch.from_numpy(order_kv[pad])]
    v = qkv[:, 2 * C:][torch.from_numpy(order_kv[pad])]
    scale = 16 ** -0.5
    ref = OM._patch_attention(q, k, v, cu, H, scale)[torch.from_numpy(unpad[inverse])]
    # HIP path
    offs = np.concatenate([[0], offset]).astype(np.int32)
    counts = np.diff(offs)
    pc = np.where(counts > K, (counts + K - 1) // K * K, counts)
    offs_pad = np.concatenate([[0], np.cumsum(pc)]).astype(np.int32)
    n_pad = int(offs_pad[-1])
    gq, wq = ops.pad_plan(dev(order.astype(np.int32)), dev(offs), dev(offs_pad), K, n_pad)
    gkv, _ = ops.pad_plan(dev(order_kv.astype(np.int32)), dev(offs), dev(offs_pad), K, n_pad)
    d_qkv = dev(qkv, dtype)
    out = torch.full((n, C), float("nan"), dtype=dtype, device="cuda")
    ops.attention(d_qkv[:, :C], d_qkv[:, C:2 * C], d_qkv[:, 2 * C:], gq, gkv, wq, dev(cu.astype(np.int32)), H,
                  int(np.diff(cu).max()), scale, out)
    got = out.float().cpu()
    assert torch.isfinite(got).all(), "some rows were never written / non-finite"
    return (got - ref).abs().max().item(), ref.abs().max().item()


@pytest.mark.parametrize("lens,H,K", [([2500], 2, 1024), ([1024], 4, 1024), ([991], 32, 1024), ([26], 4, 1024),
                                      ([1500, 1100], 2, 1024), ([700, 500, 3000], 1, 1024), ([10], 1, 4),
                                      ([100, 37], 2, 16), ([1025], 8, 1024), ([33], 2, 1024)])
def test_attention_fp32_vs_oracle(ops, lens, H, K):
    err, mag = _attention_case(ops, torch.float32, lens, H, K, seed=sum(lens) + H)
    report(f"attn fp32 lens={lens} H={H} K={K}", max_err=err, ref_max=mag)
    assert err < 2e-5 * (1 + mag)  # exact-fp32 MFMA; differences = summation order + exp2 vs exp


@LPS
@pytest.mark.parametrize("lens,H,K", [([2500], 2, 1024), ([1024], 4, 1024), ([991], 32, 1024), ([26], 4, 1024),
                                      ([1500, 1100], 2, 1024), ([700, 500, 3000], 1, 1024), ([10], 1, 4),
                                      ([100, 37], 2, 16), ([1025], 8, 1024), ([33], 2, 1024)])
def test_attention_bf16_vs_oracle(ops, lp, lens, H, K):
    err, mag = _attention_case(ops, LP(), lens, H, K, seed=sum(lens) + H)
    report(f"attn bf16 lens={lens} H={H} K={K}", max_err=err, ref_max=mag)
    # inputs are bf16-exact; P is rounded to bf16 (2^-9 relative) and the output to bf16
    assert err < 0.02 * (1 + mag)


@LPS
def test_cross_attention_vs_oracle(ops, lp):
    for dtype, tol in ((torch.float32, 2e-5), (LP(), 0.02)):
        err, mag = _attention_case(ops, dtype, [991], 32, 1024, seed=7, cross=True)
        assert err < tol * (1 + mag)
        err, mag = _attention_case(ops, dtype, [1300, 1200], 4, 1024, seed=8, cross=True)
        assert err < tol * (1 + mag)


@LPS
def test_attention_16bit_output_rows_that_are_only_8_byte_aligned(ops, lp):
    """a 16-bit output with ldo % 8 != 0 (8-byte aligned rows) was a valid call before the one-store epilogue and
    must stay one: the kernel falls back to the two 8-byte pieces a lane holds.  Same values as the aligned call."""
    g = torch.Generator().manual_seed(3)
    n, H = 1500, 2
    C = 16 * H
    qkv = torch.randn(n, 3 * C, generator=g).to(LP()).cuda()
    order = torch.randperm(n, generator=g).numpy()
    offs = dev(np.array([0, n], dtype=np.int32))
    offs_pad = dev(np.array([0, 2048], dtype=np.int32))
    gq, wq = ops.pad_plan(dev(order.astype(np.int32)), offs, offs_pad, 1024, 2048)
    ps = dev(np.array([0, 1024, 2048], dtype=np.int32))
    ref = torch.empty(n, C, dtype=LP(), device="cuda")
    ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], gq, gq, wq, ps, H, 1024, 0.25, ref)
    wide = torch.zeros(n, C + 4, dtype=LP(), device="cuda")  # row stride 36 elements = 72 bytes: 8- but not 16-byte aligned
    out = wide[:, :C]
    ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], gq, gq, wq, ps, H, 1024, 0.25, out)
    torch.cuda.synchronize()
    assert torch.equal(out, ref) and float(wide[:, C:].abs().max()) == 0.0


def test_attention_softmax_is_shift_safe(ops):
    """Large score magnitudes (|s| ~ 60): the two-pass max must keep exp in range (no NaN / inf)."""
    g = torch.Generator().manual_seed(0)
    n, H = 1024, 2
    C = 16 * H
    qkv = torch.randn(n, 3 * C, generator=g)
    qkv[:, :2 * C] *= 6.0
    order = torch.randperm(n, generator=g).numpy()
    inverse = np.empty(n, dtype=np.int64)
    inverse[order] = np.arange(n)
    t_order = torch.from_numpy(order)
    ref = OM._patch_attention(qkv[:, :C][t_order], qkv[:, C:2 * C][t_order], qkv[:, 2 * C:][t_order],
                              np.array([0, n]), H, 0.25)[torch.from_numpy(inverse)]
    offs = dev(np.array([0, n], dtype=np.int32))
    gq, wq = ops.pad_plan(dev(order.astype(np.int32)), offs, offs, 1024, n)
    d = dev(qkv)
    out = torch.empty(n, C, dtype=torch.float32, device="cuda")
    ops.attention(d[:, :C], d[:, C:2 * C], d[:, 2 * C:], gq, gq, wq, offs, H, n, 0.25, out)
    assert (out.cpu() - ref).abs().max().item() < 1e-4


# ---------------------------------------------------------------- test-time pipeline kernels (testtime.hip)
@pytest.mark.parametrize("tag", ["room", "dense", "neg"])
def test_gridsample_device_vs_reference_fixture(ops, tag):
    """voxelize + sort + run segmentation + fragment_select against the reference's GridSample(mode="test")."""
    from cdsegnet_amd import testtime as tt
    from oracle import testtime as OT
    fx = load_fixture(f"gridsample_test_{tag}.npz")
    coord, gsize = fx["coord"], float(fx["grid_size"])
    grid, parts = OT.grid_sample_test(coord, gsize)
    gs = tt.grid_sample_test(dev(coord), gsize)
    assert gs["num_fragments"] == len(parts) == fx["index"].shape[0]
    assert gs["num_voxels"] == len(parts[0])
    assert np.array_equal(gs["grid_coord"].cpu().numpy(), grid)  # bit-exact voxel coordinates
    ref_vox = {tuple(r) for r in fx["grid_coord"][0].tolist()}
    for i, p in enumerate(parts):
        got = tt.fragment(gs, i).cpu().numpy()
        assert np.array_equal(np.sort(got), np.sort(p))  # stable sort on both sides: identical member choice
        assert {tuple(r) for r in grid[got].tolist()} == ref_vox  # one point of every reference voxel


def test_softmax_vote_and_argmax(ops):
    from oracle import testtime as OT
    rng = np.random.default_rng(3)
    n, c = 5000, 20
    parts = [rng.permutation(n)[:3000] for _ in range(3)]
    logits = [(rng.normal(size=(3000, c)) * 4).astype(np.float32) for _ in parts]
    ref_labels, ref_pred = OT.vote(n, c, parts, logits)
    pred = torch.zeros(n, c, device="cuda")
    for p, lg in zip(parts, logits):
        ops.softmax_vote(dev(lg), dev(p.astype(np.int32)), pred)
    assert np.abs(pred.cpu().numpy() - ref_pred).max() < 2e-6
    labels = ops.argmax_rows(pred).cpu().numpy()
    same = labels == ref_labels
    # disagreement only where the two best classes tie to rounding
    top2 = np.sort(ref_pred[~same], 1)[:, -2:]
    assert same.mean() > 0.999 and np.all(top2[:, 1] - top2[:, 0] < 1e-5)
    # tie rule: first maximum; wide rows (200 classes > one wave)
    x = torch.zeros(4, 200, device="cuda")
    x[1, 150] = 1.0
    x[2, 70] = x[2, 199] = 2.0
    x[3] = -1.0
    assert ops.argmax_rows(x).cpu().tolist() == [0, 150, 70, 0]


@pytest.mark.parametrize("name", CLOUDS)
def test_coarse_orders_equal_sorted_orders(ops, name):
    """Pooled-level curve orders derived from the level-0 orders (flag / scan / compact) are bit-identical to
    arg-sorting the shifted codes (what SerializedPooling does, ptv3.py:503-514)."""
    fx = load_fixture(f"serialization_{name}.npz")
    zs, perm0, g0, b0, depth, p = _physical(ops, fx)
    code0 = ops.encode4(g0, b0, depth)
    orders0 = [ops.sort_pairs(code0[c].contiguous())[1] for c in (1, 2, 3)]
    clusters, sizes, sorted_orders = [], [], []
    for cum in (1, 2, 3):
        if cum >= depth:
            break
        cl, seg, cnt = ops.pool_level(zs, 3 * cum)
        m = int(cnt.item())
        gc, bc, cc = ops.pool_gather(seg, m, len(p), cum, g0, b0, code0)
        clusters.append(cl)
        sizes.append(m)
        sorted_orders.append([ops.sort_pairs(cc[c].contiguous())[1] for c in (1, 2, 3)])
    derived = ops.coarse_orders(clusters, orders0, sizes)
    for lvl in range(len(clusters)):
        for c in range(3):
            assert torch.equal(derived[lvl][c], sorted_orders[lvl][c]), (name, lvl, c)


# ---------------------------------------------------------------- evaluator kernels (testtime.hip)
def _knn_case(ops, ref, roff, qry, qoff, cell):
    from oracle import testtime as OT
    want, wd2 = OT.knn1_bruteforce(ref, roff, qry, qoff)
    idx, d2 = ops.knn1(dev(ref), dev(np.asarray(roff, dtype=np.int32)), dev(qry), dev(np.asarray(qoff, dtype=np.int32)),
                       ref.min(0).tolist(), cell, want_dist=True)
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    bad = idx != want
    # any disagreement must be an exact-distance tie broken differently by fp32 contraction, never a farther point
    assert np.all(np.abs(d2[bad] - wd2[bad]) <= 1e-6 * (1 + wd2[bad])), (bad.sum(), d2[bad][:4], wd2[bad][:4])
    assert bad.mean() < 1e-3
    return idx


def test_knn1_vs_bruteforce_oracle(ops):
    rng = np.random.default_rng(1)
    # voxelised scene + its raw points (the evaluator's use): two batch elements
    raw = (rng.random((30000, 3)) * np.array([4.0, 3.0, 0.3])).astype(np.float32)
    keep = rng.random(30000) < 0.35
    ref = raw[keep]
    nr0 = int(keep[:14000].sum())
    _knn_case(ops, ref, [nr0, len(ref)], raw, [14000, 30000], 0.05)
    # queries far outside the reference box (shell limit -> brute-force fallback), tiny and huge cells
    far = np.concatenate([raw[:500], raw[:200] + np.float32(50.0), raw[:100] - np.float32(3.0)])
    _knn_case(ops, ref[:nr0], [nr0], far, [len(far)], 0.05)
    _knn_case(ops, ref[:nr0], [nr0], far[:600], [600], 0.004)
    _knn_case(ops, ref[:nr0], [nr0], far[:600], [600], 5.0)
    # integer lattice: exact ties -> lowest index wins, bit-exact
    lat = rng.integers(0, 12, size=(4000, 3)).astype(np.float32)
    q = rng.integers(0, 12, size=(3000, 3)).astype(np.float32) + np.float32(0.5)
    from oracle import testtime as OT
    want, _ = OT.knn1_bruteforce(lat, [4000], q, [3000])
    got = ops.knn1(dev(lat), dev(np.array([4000], dtype=np.int32)), dev(q), dev(np.array([3000], dtype=np.int32)),
                   [0.0, 0.0, 0.0], 1.0).cpu().numpy()
    assert np.array_equal(got, want)
    # an empty batch element
    got = ops.knn1(dev(lat), dev(np.array([0, 4000], dtype=np.int32)), dev(q), dev(np.array([10, 3000], dtype=np.int32)),
                   [0.0, 0.0, 0.0], 1.0).cpu().numpy()
    assert np.all(got[:10] == -1) and np.all(got[10:] >= 0)


@pytest.mark.parametrize("k", [1, 8, 16, 48, 64])
def test_knn_k_vs_bruteforce_oracle(ops, k):
    """cdseg_knn (round 5: pointops.knn_query for k > 1 - the neighbourhood query of the reference's other backbones,
    libs/pointops/functions/query.py:7-24) against oracle/testtime.py::knn_bruteforce: two batch elements, self-query and
    separate queries, a batch element with fewer than k points (placeholders), queries far outside the box (brute-force
    fallback), an integer lattice with masses of exact ties (bit-exact, index order)."""
    from oracle import testtime as OT
    rng = np.random.default_rng(k)
    raw = (rng.random((9000, 3)) * np.array([4.0, 3.0, 0.3])).astype(np.float32)
    ref = raw[rng.random(9000) < 0.5]
    nr0 = min(len(ref) - 1, 40)  # first batch element: 40 points (< k for the large k: placeholders)
    qry = np.concatenate([raw[:3000], raw[:50] + np.float32(30.0)])
    roff, qoff = [nr0, len(ref)], [300, len(qry)]

    def check(ref, roff, qry, qoff, exact, **kw):
        want, wd2 = OT.knn_bruteforce(k, ref, roff, qry, qoff)
        idx, dist = ops.knn(k, dev(ref), dev(np.asarray(roff, dtype=np.int32)), dev(qry), dev(np.asarray(qoff, dtype=np.int32)), **kw)
        idx, d2 = idx.cpu().numpy().astype(np.int64), dist.cpu().numpy().astype(np.float64) ** 2
        assert idx.shape == (len(qry), k)
        assert np.array_equal(idx < 0, want < 0)          # placeholders exactly where the element runs out of points
        live = want >= 0
        assert np.allclose(d2[live], wd2[live], rtol=2e-5, atol=1e-9)  # the k smallest distances, ascending
        assert np.all(np.diff(d2, axis=1)[live[:, 1:]] >= -1e-12)
        # every returned index realises its distance, lies in the query's batch element and appears once
        bq = np.searchsorted(np.asarray(qoff), np.arange(len(qry)), side="right")
        lo = np.concatenate([[0], roff])[bq][:, None]
        hi = np.asarray(roff)[bq][:, None]
        assert np.all((idx >= lo)[live]) and np.all((idx < hi)[live])
        true = ((qry[:, None, :].astype(np.float32) - ref[np.clip(idx, 0, None)].astype(np.float32)) ** 2).sum(-1)
        assert np.allclose(true[live], d2[live], rtol=2e-5, atol=1e-9)
        srt = np.sort(np.where(live, idx, -1 - np.arange(k)[None, :]), axis=1)
        assert np.all(np.diff(srt, axis=1) != 0)
        if exact:
            assert np.array_equal(idx, want)

    check(ref, roff, qry, qoff, exact=False)
    check(ref, roff, ref, roff, exact=False)                                # self-query (pointops' default)
    check(ref, roff, qry, qoff, exact=False, origin=ref.min(0).tolist(), cell=0.01)   # tiny cells
    check(ref, roff, qry, qoff, exact=False, origin=ref.min(0).tolist(), cell=4.0)    # one cell holds everything
    lat = rng.integers(0, 7, size=(3000, 3)).astype(np.float32)
    q = rng.integers(0, 7, size=(1500, 3)).astype(np.float32) + np.float32(0.5)
    check(lat, [3000], q, [1500], exact=True, origin=[0.0, 0.0, 0.0], cell=1.0)


def test_knn_rejects_k_above_its_limit(ops):
    from cdsegnet_amd import _lib
    x = torch.rand(100, 3, device="cuda")
    off = torch.tensor([100], dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.CdsegError):
        ops.knn(65, x, off)


def test_iou_counts_vs_reference_fixture(ops):
    fx = load_fixture("iou_counts.npz")
    for tag in ("a", "b", "c"):
        k = int(fx[f"{tag}_k"])
        out = ops.iou_counts(dev(fx[f"{tag}_pred"].astype(np.int32)), dev(fx[f"{tag}_target"].astype(np.int32)), k, -1)
        out = out.cpu().numpy()
        assert np.array_equal(out[0], fx[f"{tag}_inter"])
        assert np.array_equal(out[1] + out[2] - out[0], fx[f"{tag}_union"])
        assert np.array_equal(out[2], fx[f"{tag}_tgt"])


def test_evaluate_scene_vs_oracle(ops):
    from cdsegnet_amd import evaluate
    from oracle import testtime as OT
    rng = np.random.default_rng(5)
    raw = (rng.random((20000, 3)) * np.array([3.0, 2.0, 0.2])).astype(np.float32)
    keep = rng.random(20000) < 0.4
    coord = raw[keep]
    k = 13
    logits = rng.normal(size=(len(coord), k)).astype(np.float32)
    seg = rng.integers(-1, k, size=len(raw))
    d = dict(coord=dev(coord), offset=dev(np.array([len(coord)], dtype=np.int64)), origin_coord=dev(raw),
             origin_offset=dev(np.array([len(raw)], dtype=np.int64)), origin_segment=dev(seg))
    counts = evaluate.evaluate_scene(dev(logits), d, k, ignore_index=-1, reduce=False).cpu().numpy()
    idx, _ = OT.knn1_bruteforce(coord, [len(coord)], raw, [len(raw)])
    i, u, t = OT.intersection_and_union(logits.argmax(1)[idx], seg, k, -1)
    assert np.array_equal(counts[0], i) and np.array_equal(counts[1], u) and np.array_equal(counts[2], t)


@pytest.mark.parametrize("name", ["room1500", "batch2", "lidar5000"])
def test_batched_plan_kernels_equal_single_calls(ops, name):
    """pool_levels / link_derive / pad_plan_batch (one launch per scene) against the per-level / per-plan kernels."""
    fx = load_fixture(f"serialization_{name}.npz")
    zs, perm0, g0, b0, depth, p = _physical(ops, fx)
    n = len(p)
    offs_np = np.concatenate([[0], np.cumsum(np.bincount(fx["batch"]))]).astype(np.int32)
    nb = len(offs_np) - 1
    last = dev((offs_np[1:] - 1).astype(np.int32))
    shifts = [3, 6, 9]
    cl, seg, meta = ops.pool_levels(zs, shifts, last)
    meta = meta.cpu().numpy()
    assert meta[-1] == 0  # no duplicate (batch, voxel) codes in the fixture
    meta = meta[:-1].reshape(len(shifts), 1 + nb)
    singles = []
    for l, sh in enumerate(shifts):
        c1, s1, cnt = ops.pool_level(zs, sh)
        m = int(cnt.item())
        singles.append((c1, s1, m))
        assert meta[l, 0] == m
        assert torch.equal(cl[l], c1) and torch.equal(seg[l][:m + 1], s1[:m + 1])
        assert np.array_equal(meta[l, 1:], c1.cpu().numpy()[offs_np[1:] - 1])
    # link between pooled levels 1 and 2 from their links to level 0 == pooling level 1's own codes
    (c0a, s0a, ma), (c0b, s0b, mb) = singles[0], singles[1]
    code0 = ops.encode4(g0, b0, depth)
    ga, ba, ca = ops.pool_gather(s0a, ma, n, 1, g0, b0, code0)
    want_c, want_s, want_m = ops.pool_level(ca[0].contiguous(), 3)
    got_c, got_s = ops.link_derive(c0a, s0a, ma, c0b, s0b, mb)
    assert int(want_m.item()) == mb
    assert torch.equal(got_c, want_c[:ma]) and torch.equal(got_s, want_s[:mb + 1])
    # slot plans
    order = ops.sort_pairs(code0[2].contiguous())[1]
    items = []
    for K in (4, 16, 1024):
        cnt = np.diff(offs_np)
        padc = np.where(cnt > K, (cnt + K - 1) // K * K, cnt)
        offs_pad = np.concatenate([[0], np.cumsum(padc)]).astype(np.int32)
        for od in (None, order):
            items.append((od, dev(offs_np), dev(offs_pad), K, int(offs_pad[-1])))
    got = ops.pad_plan_batch(items, nb)
    for (od, a, b, K, npad), (g, w) in zip(items, got):
        g1, w1 = ops.pad_plan(od, a, b, K, npad)
        assert torch.equal(g, g1) and torch.equal(w, w1)


@LPS
def test_attention_bf16_loose_score_bound_falls_back_to_exact_max(ops, lp):
    """Huge, nearly orthogonal q / k (|q| |k| * scale ~ 900, scores O(10)) on a two-patch launch whose second patch is padded.
    Written for the Cauchy-Schwarz shift of rounds 2 - 5 (m_i = |q_i| max_j |k_j|, loose by 2^60 here); the unshifted
    kernel of round 6 takes no redo on these rows (the denominator stays inside [1e-30, 1e30]), so this now checks large
    operands whose products cancel.  The redo itself is driven by tests/test_gpu_attention_range.py."""
    g = torch.Generator().manual_seed(3)
    n, H = 1500, 2
    C = 16 * H
    q = torch.randn(n, C, generator=g) * 0.05
    k = torch.randn(n, C, generator=g) * 0.05
    v = torch.randn(n, C, generator=g)
    q[:, 0::16] += 60.0   # every head: q mostly along dim 0 ...
    k[:, 1::16] += 60.0   # ... k mostly along dim 1: scores are O(10), |q||k| * scale ~ 900
    q[::7, 1::16] += 1.0  # a few rows with real structure
    q, k, v = _bf16_round(q), _bf16_round(k), _bf16_round(v)
    order = torch.randperm(n, generator=g).numpy()
    inverse = np.empty(n, dtype=np.int64)
    inverse[order] = np.arange(n)
    t_order = torch.from_numpy(order)
    starts = np.array([0, 1024, n])
    ref = torch.cat([OM._patch_attention(q[t_order][a:b], k[t_order][a:b], v[t_order][a:b], np.array([0, b - a]), H, 0.25)
                     for a, b in ((0, 1024), (1024 - (2048 - n), n))])
    # padded second patch borrows the tail of the first (ptv3.py:218-228): use the library's own plan for the layout
    offs = dev(np.array([0, n], dtype=np.int32))
    offs_pad = dev(np.array([0, 2048], dtype=np.int32))
    gq, wq = ops.pad_plan(dev(order.astype(np.int32)), offs, offs_pad, 1024, 2048)
    ps = dev(np.array([0, 1024, 2048], dtype=np.int32))
    out = torch.empty(n, C, dtype=LP(), device="cuda")
    ops.attention(dev(q, LP()), dev(k, LP()), dev(v, LP()), gq, gq, wq, ps, H, 1024, 0.25, out)
    got = out.float().cpu()[t_order]
    want = torch.cat([ref[:1024], ref[1024 + (2048 - n):]])
    assert torch.isfinite(got).all()
    assert (got - want).abs().max().item() < 0.03 * (1 + want.abs().max().item())


@LPS
@pytest.mark.parametrize("lens,H,flags", [([2500], 2, 1), ([2500], 2, 2), ([1500, 1100], 4, 3), ([991], 32, 3), ([26], 4, 3)])
def test_attention_ex_producer_side_flags_vs_oracle(ops, lp, lens, H, flags):
    """cdseg_attention_ex with the preprocessing a producer epilogue does (round 5): q already multiplied by
    softmax scale * log2(e) (CDSEG_ATTN_Q_PRESCALED) and v stored as bfloat16 inside the build's 16-bit buffer
    (CDSEG_ATTN_V_BF16: matters in the IEEE-half build).  Oracle: oracle/model.py's patch attention on the SAME rounded
    operands (the scaled q rounded to the build's type, v rounded to bfloat16)."""
    g = torch.Generator().manual_seed(sum(lens) + H + flags)
    C = 16 * H
    offset = np.cumsum(lens)
    n = int(offset[-1])
    scale = 16 ** -0.5
    c = scale * 1.4426950408889634
    lpt = LP()
    q = torch.randn(n, C, generator=g) * 2.0
    k = torch.randn(n, C, generator=g).to(lpt).float()
    v = torch.randn(n, C, generator=g)
    if flags & ops.ATTN_Q_PRESCALED:
        q_dev = (q * c).to(lpt)                  # what a producer with folded weights writes
        q_ref = q_dev.float() / c                # the oracle applies `scale` itself: exp(scale q k) = 2^(q' k)
    else:
        q_dev = q.to(lpt)
        q_ref = q_dev.float()
    if flags & ops.ATTN_V_BF16:
        v_ref = v.to(torch.bfloat16).float()
        v_dev = v.to(torch.bfloat16).view(torch.int16).view(lpt) if lpt == torch.float16 else v.to(torch.bfloat16)
    else:
        v_ref = v.to(lpt).float()
        v_dev = v.to(lpt)
    order = np.concatenate([s0 + torch.randperm(int(cn), generator=g).numpy() for s0, cn in
                            zip(np.concatenate([[0], offset[:-1]]), lens)]).astype(np.int64)
    inverse = np.empty(n, dtype=np.int64)
    inverse[order] = np.arange(n)
    K = 1024
    pad, unpad, cu = S.padding_plan(offset, K)
    t = torch.from_numpy(order[pad])
    ref = OM._patch_attention(q_ref[t], k[t], v_ref[t], cu, H, scale)[torch.from_numpy(unpad[inverse])]
    offs = np.concatenate([[0], offset]).astype(np.int32)
    counts = np.diff(offs)
    pc = np.where(counts > K, (counts + K - 1) // K * K, counts)
    offs_pad = np.concatenate([[0], np.cumsum(pc)]).astype(np.int32)
    gq, wq = ops.pad_plan(dev(order.astype(np.int32)), dev(offs), dev(offs_pad), K, int(offs_pad[-1]))
    d_qkv = torch.cat([q_dev, k.to(lpt), v_dev], 1).cuda().contiguous()
    out = torch.full((n, C), float("nan"), dtype=lpt, device="cuda")
    ops.attention(d_qkv[:, :C], d_qkv[:, C:2 * C], d_qkv[:, 2 * C:], gq, gq, wq, dev(cu.astype(np.int32)), H,
                  int(np.diff(cu).max()), scale, out, flags=flags)
    got = out.float().cpu()
    assert torch.isfinite(got).all()
    err, mag = (got - ref).abs().max().item(), ref.abs().max().item()
    report(f"attn_ex {lp} lens={lens} H={H} flags={flags}", max_err=err, ref_max=mag)
    assert err < 0.02 * (1 + mag)


def test_attention_ex_rejects_bad_arguments(ops):
    """Unknown flag bits, a v-is-bfloat16 claim on the fp32 path, and misaligned output rows are CDSEG_ERR_ARG, not UB."""
    from cdsegnet_amd import _lib
    n, H = 64, 1
    qkv = torch.zeros(n, 48, dtype=torch.float32, device="cuda")
    out = torch.zeros(n, 16, dtype=torch.float32, device="cuda")
    idx = torch.arange(n, dtype=torch.int32, device="cuda")
    ps = torch.tensor([0, n], dtype=torch.int32, device="cuda")
    for flags in (4, 2):
        with pytest.raises(_lib.CdsegError):
            ops.attention(qkv[:, :16], qkv[:, 16:32], qkv[:, 32:], idx, idx, idx, ps, H, n, 0.25, out, flags=flags)
    wide = torch.zeros(n, 18, dtype=torch.float32, device="cuda")  # 72-byte rows
    with pytest.raises(_lib.CdsegError):
        ops.attention(qkv[:, :16], qkv[:, 16:32], qkv[:, 32:], idx, idx, idx, ps, H, n, 0.25, wide[:, :16])


@LPS
@pytest.mark.parametrize("n,H,scenes", [(420000, 2, 3), (230000, 4, 2), (115000, 8, 2), (150000, 4, 1)])
def test_attention_large_launch_graded_schedule_vs_fp32_kernel(ops, lp, n, H, scenes):
    """A launch with hundreds of (patch, head) units per XCD - where cdseg_attention's graded schedule (lead / tail zones of
    sliced patch-heads, csrc/attention.hip decode_block) is active - against the exact-fp32 kernel, which runs the uniform
    schedule: every output row written exactly once, same values up to the 16-bit rounding of P and O.  Patches are cut
    from the Hilbert order of real (synthetic-room) scenes, ragged last patches included."""
    from cdsegnet_amd import synth
    grids, batches = [], []
    for i in range(scenes):
        sc = synth.room_scene(100 + i, n // scenes)
        grids.append(torch.as_tensor(sc["grid_coord"]))
        batches.append(torch.full((len(sc["grid_coord"]),), i, dtype=torch.int64))
    grid, batch = torch.cat(grids).cuda(), torch.cat(batches).cuda()
    n = grid.shape[0]
    counts = torch.bincount(batch.cpu(), minlength=scenes).numpy()
    depth = int(ops.grid_max(grid).item()).bit_length()
    zs, perm0 = ops.sort_pairs(ops.encode(grid, batch, depth, "z"))
    g0, b0 = ops.plan_gather_grid(grid, perm0, zs, depth)
    code4 = ops.encode4(g0, b0, depth)
    _, order = ops.sort_pairs(code4[2].contiguous())
    K = 1024
    pads = [(c + K - 1) // K * K if c > K else c for c in counts]
    offs = dev(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32))
    offs_pad = dev(np.concatenate([[0], np.cumsum(pads)]).astype(np.int32))
    npad = int(sum(pads))
    gidx, widx = ops.pad_plan(order, offs, offs_pad, K, npad)
    starts = []
    for s0, p in zip(np.concatenate([[0], np.cumsum(pads)])[:-1], pads):
        starts += list(range(int(s0), int(s0 + p), K))
    ps = dev(np.array(starts + [npad], dtype=np.int32))
    C = 16 * H
    g = torch.Generator().manual_seed(n + H)
    qkv = torch.randn(n, 3 * C, generator=g).to(LP())
    d16 = qkv.cuda()
    d32 = qkv.float().cuda()
    o16 = torch.full((n, C), float("nan"), dtype=LP(), device="cuda")
    o32 = torch.full((n, C), float("nan"), dtype=torch.float32, device="cuda")
    ops.attention(d16[:, :C], d16[:, C:2 * C], d16[:, 2 * C:], gidx, gidx, widx, ps, H, K, 0.25, o16)
    ops.attention(d32[:, :C], d32[:, C:2 * C], d32[:, 2 * C:], gidx, gidx, widx, ps, H, K, 0.25, o32)
    assert torch.isfinite(o16.float()).all() and torch.isfinite(o32).all()
    err = (o16.float() - o32).abs().max().item()
    units = (ps.numel() - 1) * H
    # which launches get the tail zones is the library's own statement (host-side diagnostic, csrc/attention.hip)
    from cdsegnet_amd import _lib
    import ctypes
    lib = _lib.load()
    nb = lib.cdseg_attention_schedule(ps.numel() - 1, H, K, _lib.BF16, None, 0)
    tab = np.zeros((nb, 4), dtype=np.int32)
    lib.cdseg_attention_schedule(ps.numel() - 1, H, K, _lib.BF16, tab.ctypes.data_as(ctypes.c_void_p), nb)
    graded = len(set(tab[tab[:, 0] >= 0][:, 3].tolist())) > 1
    assert graded == (units // 8 >= 96), (units, graded)  # the first three shapes are sliced, the last one is not
    report(f"attn large {lp} n={n} H={H}", max_err=err, units=units, graded=int(graded))
    assert err < 0.02 * (1 + o32.abs().max().item())
    # run-to-run bit determinism of the sliced schedule (slices of a patch-head write disjoint rows)
    o16b = torch.full_like(o16, float("nan"))
    ops.attention(d16[:, :C], d16[:, C:2 * C], d16[:, 2 * C:], gidx, gidx, widx, ps, H, K, 0.25, o16b)
    assert torch.equal(o16.view(torch.int16), o16b.view(torch.int16))


@pytest.mark.parametrize("name", ["room1500", "batch2", "lidar5000", "rand16", "lidar8", "tiny64"])
def test_sort_curves_equals_one_sort_per_curve(ops, name):
    """cdseg_sort_curves (all curve orders of a level with one radix sort, the curve slot in the key bits above end_bit)
    == cdseg_sort_pairs per curve; also a subset / permutation of the rows."""
    fx = load_fixture(f"serialization_{name}.npz")
    zs, perm0, g0, b0, depth, p = _physical(ops, fx)
    code4 = ops.encode4(g0, b0, depth)
    nb = int(b0.max().item()) + 1
    end_bit = 3 * depth + max(1, nb.bit_length())
    for rows in ([1, 2, 3], [3, 1], [2], [0, 1, 2, 3]):
        got = ops.sort_curves(code4, rows, end_bit)
        for k, r in enumerate(rows):
            want = ops.sort_pairs(code4[r].contiguous(), None, end_bit=end_bit)[1]
            assert torch.equal(got[k], want), (rows, r)


@pytest.mark.parametrize("name", ["room1500", "batch2", "lidar5000", "rand16", "lidar8", "tiny64"])
def test_kernel_map_from_parent_equals_search(ops, name):
    """cdseg_nbr_table_from_parent (parent level's 3x3x3 map + children runs) and cdseg_nbr_table_from_info (the same with
    the parents' child_info words: first child + popcount of the occupancy) == cdseg_nbr_table (binary search)."""
    fx = load_fixture(f"serialization_{name}.npz")
    zs, perm0, g0, b0, depth, p = _physical(ops, fx)
    code0 = ops.encode4(g0, b0, depth)
    cl, seg, cnt = ops.pool_level(zs, 3)
    m = int(cnt.item())
    gc, bc, cc = ops.pool_gather(seg, m, len(p), 1, g0, b0, code0)
    pn = ops.nbr_table(cc[0].contiguous(), gc, bc, depth - 1, 3, True)
    cinfo = ops.child_info(zs, seg, m)
    for ksize in (3, 5):
        for kmajor in (False, True):
            want = ops.nbr_table(zs, g0, b0, depth, ksize, kmajor)
            got = ops.nbr_table_from_parent(zs, g0, cl, pn, seg, m, depth, ksize, kmajor)
            assert torch.equal(got, want), (ksize, kmajor)
            got = ops.nbr_table_from_info(g0, cl, pn, cinfo, m, depth, ksize, kmajor)
            assert torch.equal(got, want), (ksize, kmajor, "info")


@LPS
@pytest.mark.parametrize("M,C", [(1000, 32), (4097, 64), (64, 32), (70, 64), (120000, 32), (4097, 128), (14293, 128),
                                 (65536 + 77, 128)])  # >= 64 k rows at C = 128: the 128-row workgroups
def test_mlp_fused_vs_two_gemms_and_fp64(ops, lp, M, C):
    """cdseg_mlp_fused (hidden activation kept in LDS) against the two-GEMM form and an fp64 reference that rounds
    the hidden activation to bf16 at the same place (ptv3.py:299-322, :423-427)."""
    g = torch.Generator().manual_seed(M + C)
    h = _bf16_round(torch.randn(M, C, generator=g))
    w1 = _bf16_round(torch.randn(4 * C, C, generator=g) / C ** 0.5)
    w2 = _bf16_round(torch.randn(C, 4 * C, generator=g) / (4 * C) ** 0.5)
    b1, b2 = torch.randn(4 * C, generator=g), torch.randn(C, generator=g)
    x0 = torch.randn(M, C, generator=g)
    u = _bf16_round(F.gelu((h.double() @ w1.double().t() + b1.double()).float()))
    ref = x0.double() + u.double() @ w2.double().t() + b2.double()
    bf = LP()
    x = dev(x0)
    xc = torch.empty(M, C, dtype=bf, device="cuda")
    assert ops.mlp_fused_ok(dev(h, bf), 4 * C)
    with ops.record_routes() as rr:
        ops.mlp_fused(dev(h, bf), dev(w1, bf), dev(b1), dev(w2, bf), dev(b2), x, xc)
    # the launch record: 128-row workgroups at C = 128 from 65 536 rows, 64-row ones everywhere else
    rows = 128 if (C == 128 and M >= 65536) else 64
    assert [(r.kernel, r.aux) for r in rr.routes] == [(f"mlp_fused_kernel<{C},64,mlp,{rows}>", rows)], rr.routes
    err = (x.cpu().double() - ref).abs().max().item()
    report(f"fused mlp M={M} C={C}", max_err=err)
    assert err < 2e-2  # a hidden value on a bf16 rounding boundary may round the other way (fp32 vs fp64 GELU input)
    assert torch.equal(xc, x.to(bf))
    # the unfused launches
    x2 = dev(x0)
    uu = torch.empty(M, 4 * C, dtype=bf, device="cuda")
    ops.gemm(dev(h, bf), dev(w1, bf), uu, bias=dev(b1), act=ops.ACT_GELU)
    ops.gemm(uu, dev(w2, bf), x2, bias=dev(b2), res=x2)
    # same MFMA products; the two kernels may contract the GELU polynomial differently (1 fp32 ulp), which flips a hidden
    # value sitting on a bf16 rounding boundary once in ~2^15 elements: isolated 1e-3 differences, nothing systematic
    d = (x - x2).abs()
    assert d.max().item() < 1e-2 and d.mean().item() < 2e-6


@LPS
@pytest.mark.parametrize("M,C", [(1000, 32), (4097, 64), (64, 64), (120000, 32)])
def test_attn_tail_fused_equals_proj_ln_mlp_sequence(ops, lp, M, C):
    """cdseg_attn_tail_fused == proj GEMM (+ residual, LN2 in its epilogue) followed by the fused MLP, bit for bit:
    same MFMA products, same row-wise LayerNorm arithmetic (ptv3.py:416-427)."""
    g = torch.Generator().manual_seed(M * 3 + C)
    bf = LP()
    o = dev(_bf16_round(torch.randn(M, C, generator=g)), bf)
    wp = dev(_bf16_round(torch.randn(C, C, generator=g) / C ** 0.5), bf)
    w1 = dev(_bf16_round(torch.randn(4 * C, C, generator=g) / C ** 0.5), bf)
    w2 = dev(_bf16_round(torch.randn(C, 4 * C, generator=g) / (4 * C) ** 0.5), bf)
    bp, b1, b2 = dev(torch.randn(C, generator=g)), dev(torch.randn(4 * C, generator=g)), dev(torch.randn(C, generator=g))
    lg, lb = dev(torch.randn(C, generator=g)), dev(torch.randn(C, generator=g))
    x0 = torch.randn(M, C, generator=g)
    xa = dev(x0)
    xca = torch.empty(M, C, dtype=bf, device="cuda")
    assert ops.attn_tail_fused_ok(o, 4 * C)
    ops.attn_tail_fused(o, wp, bp, lg, lb, w1, b1, w2, b2, xa, xca)
    xb = dev(x0)
    h = torch.empty(M, C, dtype=bf, device="cuda")
    ops.gemm(o, wp, xb, bias=bp, res=xb, ln_post=(lg, lb), ln_out=h)
    xcb = torch.empty(M, C, dtype=bf, device="cuda")
    ops.mlp_fused(h, w1, b1, w2, b2, xb, xcb)
    assert torch.equal(xa, xb) and torch.equal(xca, xcb)
    # and against plain torch
    xr = x0 + (o.float().cpu() @ wp.float().cpu().t() + bp.cpu())
    hr = _bf16_round(F.layer_norm(xr, (C,), lg.cpu(), lb.cpu(), 1e-5))
    u = _bf16_round(F.gelu(hr @ w1.float().cpu().t() + b1.cpu()))
    ref = xr + u @ w2.float().cpu().t() + b2.cpu()
    assert (xa.cpu() - ref).abs().max().item() < 3e-2


@LPS
@pytest.mark.parametrize("M,C,tb", [(1000, 32, True), (4097, 64, False), (64, 64, True), (120000, 32, False),
                                    (70001, 64, True)])  # >= 64 k rows: the 128-row workgroups, ragged last tile
def test_cpe_head_fused_equals_linear_ln_qkv_sequence(ops, lp, M, C, tb):
    """cdseg_cpe_head_fused == cpe linear GEMM (LN_cpe + residual + t bias + LN1 in its epilogue) followed by the qkv
    GEMM, bit for bit (ptv3.py:401-414)."""
    g = torch.Generator().manual_seed(M * 5 + C)
    bf = LP()
    y = dev(_bf16_round(torch.randn(M, C, generator=g)), bf)
    wl = dev(_bf16_round(torch.randn(C, C, generator=g) / C ** 0.5), bf)
    wq = dev(_bf16_round(torch.randn(3 * C, C, generator=g) / C ** 0.5), bf)
    bl, bq = dev(torch.randn(C, generator=g)), dev(torch.randn(3 * C, generator=g))
    g1, b1 = dev(torch.randn(C, generator=g)), dev(torch.randn(C, generator=g))
    g2, b2 = dev(torch.randn(C, generator=g)), dev(torch.randn(C, generator=g))
    cb = dev(torch.randn(C, generator=g)) if tb else None
    x0 = torch.randn(M, C, generator=g)
    xa = dev(x0)
    qa = torch.empty(M, 3 * C, dtype=bf, device="cuda")
    assert ops.cpe_head_fused_ok(y)
    ops.cpe_head_fused(y, wl, bl, (g1, b1), xa, cb, (g2, b2), wq, bq, qa)
    xb = dev(x0)
    h = torch.empty(M, C, dtype=bf, device="cuda")
    ops.gemm(y, wl, xb, bias=bl, ln_pre=(g1, b1), res=xb, colbias=cb, ln_post=(g2, b2), ln_out=h)
    qb = torch.empty(M, 3 * C, dtype=bf, device="cuda")
    ops.gemm(h, wq, qb, bias=bq)
    assert torch.equal(xa, xb) and torch.equal(qa, qb)


@LPS
@pytest.mark.parametrize("M,C,tb", [(1000, 32, True), (4097, 64, False), (64, 64, True), (31, 32, False), (120000, 32, False),
                                    (120001, 64, True)])
def test_block_rr_head_and_tail_vs_fused_kernels(ops, lp, M, C, tb):
    """csrc/blockrr.hip (weights resident in LDS, activations in registers, transposed MFMA products, permuted channel
    ownership) against the 64-row-tile fused kernels they replace and against plain torch with the same bf16 rounding
    points (ptv3.py:401-427).  Same products and rounding points; the fp32 summation order inside a dot product differs,
    so the comparison is within a few fp32 ulps of the row norm, plus isolated bf16 boundary flips."""
    g = torch.Generator().manual_seed(M * 7 + C)
    bf = LP()
    rnd = lambda *sh, s=1.0: _bf16_round(torch.randn(*sh, generator=g) * s)  # noqa: E731
    y, o = dev(rnd(M, C), bf), dev(rnd(M, C), bf)
    wl, wq, wp = dev(rnd(C, C, s=C ** -0.5), bf), dev(rnd(3 * C, C, s=C ** -0.5), bf), dev(rnd(C, C, s=C ** -0.5), bf)
    w1, w2 = dev(rnd(4 * C, C, s=C ** -0.5), bf), dev(rnd(C, 4 * C, s=(4 * C) ** -0.5), bf)
    vec = lambda n_: dev(torch.randn(n_, generator=g))  # noqa: E731
    bl, bq, bp, b1, b2 = vec(C), vec(3 * C), vec(C), vec(4 * C), vec(C)
    g1, be1, g2, be2, g3, be3 = vec(C), vec(C), vec(C), vec(C), vec(C), vec(C)
    cb = vec(C) if tb else None
    x0 = torch.randn(M, C, generator=g)
    assert ops.block_rr_ok(C, bf)
    himg, timg = ops.block_rr_pack(C, wl, wq, wp, w1, w2)
    # ---- head
    xa, qa = dev(x0), torch.full((M, 3 * C), float("nan"), dtype=bf, device="cuda")
    ops.cpe_head_rr(y, himg, bl, (g1, be1), xa, cb, (g2, be2), bq, qa)
    xb, qb = dev(x0), torch.empty(M, 3 * C, dtype=bf, device="cuda")
    ops.cpe_head_fused(y, wl, bl, (g1, be1), xb, cb, (g2, be2), wq, bq, qb)
    dx = (xa - xb).abs().max().item()
    dq = (qa.float() - qb.float()).abs()
    report(f"head rr M={M} C={C}", x_max_diff=dx, qkv_max_diff=dq.max().item(), qkv_mean_diff=dq.mean().item())
    assert dx < 2e-5 and dq.max().item() < 0.07 and dq.mean().item() < 2e-4  # x fp32; qkv: bf16 boundary flips only
    t = (y.float().cpu() @ wl.float().cpu().t() + bl.cpu())
    xr = x0 + F.layer_norm(t, (C,), g1.cpu(), be1.cpu(), 1e-5) + (cb.cpu() if tb else 0)
    hr = _bf16_round(F.layer_norm(xr, (C,), g2.cpu(), be2.cpu(), 1e-5))
    qr = hr @ wq.float().cpu().t() + bq.cpu()
    assert (xa.cpu() - xr).abs().max().item() < 1e-4
    assert (qa.float().cpu() - qr).abs().max().item() < 0.08
    # ---- tail
    xa, xca = dev(x0), torch.full((M, C), float("nan"), dtype=bf, device="cuda")
    ops.attn_tail_rr(o, timg, bp, g3, be3, b1, b2, xa, xca)
    xb, xcb = dev(x0), torch.empty(M, C, dtype=bf, device="cuda")
    ops.attn_tail_fused(o, wp, bp, g3, be3, w1, b1, w2, b2, xb, xcb)
    d = (xa - xb).abs()
    report(f"tail rr M={M} C={C}", max_diff=d.max().item(), mean_diff=d.mean().item())
    assert d.max().item() < 2e-2 and d.mean().item() < 5e-5  # isolated hidden values on a bf16 rounding boundary
    assert torch.equal(xca, xa.to(bf))
    xr = x0 + (o.float().cpu() @ wp.float().cpu().t() + bp.cpu())
    hr = _bf16_round(F.layer_norm(xr, (C,), g3.cpu(), be3.cpu(), 1e-5))
    u = _bf16_round(F.gelu(hr @ w1.float().cpu().t() + b1.cpu()))
    ref = xr + u @ w2.float().cpu().t() + b2.cpu()
    assert (xa.cpu() - ref).abs().max().item() < 3e-2


def test_tta_pipeline_device_vs_reference_fixture(ops):
    """SURVEY 8f row 1, complete: raw scan -> CenterShift / NormalizeColor -> the 13 test-time augmentations of
    configs/scannet/CDSegNet.py:278-398 -> GridSample(mode="test") -> per-fragment CenterShift + Collect, all on the device
    (csrc/testtime.hip), against the reference's own transform classes (tests/golden/tta_pipeline.npz): augmented
    coordinates / normals bit-exact incl. their float64 / float32 dtype, per-point voxel coordinates exact, features exact."""
    from cdsegnet_amd import testtime as tt
    fx = load_fixture("tta_pipeline.npz")
    n = len(fx["coord"])
    coord, color, normal = dev(fx["coord"]), dev(fx["color"]), dev(fx["normal"])
    ops.bind_stream()
    c0 = ops.center_shift(coord, apply_z=True)
    assert np.array_equal(c0.cpu().numpy(), fx["coord0"])
    assert np.array_equal(ops.div_add(color, 127.5, -1.0).cpu().numpy(), fx["color0"])
    for a, aug in enumerate(tt.SCANNET_TTA):
        ca, na = tt.apply_aug(c0, normal, aug)
        want_c, want_n = fx[f"aug{a}_coord"], fx[f"aug{a}_normal"]
        assert str(ca.dtype).endswith(str(want_c.dtype)) and np.array_equal(ca.cpu().numpy(), want_c), a
        assert np.array_equal(na.cpu().numpy(), want_n), a
    ops.unbind_stream()
    idxs, dicts = tt.prepare_test_fragments(coord, color, normal, float(fx["grid_size"]))
    pos = 0
    for a in range(13):
        k = len(fx[f"aug{a}_frag_sizes"])
        assert [d["feat"].shape[0] for d in dicts[pos:pos + k]] == fx[f"aug{a}_frag_sizes"].tolist()
        grid = np.full((n, 3), -1, dtype=np.int64)
        feat = np.zeros((n, 6), dtype=np.float32)
        for idx, d in zip(idxs[pos:pos + k], dicts[pos:pos + k]):
            i = idx.cpu().numpy().astype(np.int64)
            grid[i] = d["grid_coord"].cpu().numpy()
            feat[i] = d["feat"].cpu().numpy()
        assert np.array_equal(grid, fx[f"aug{a}_grid"]), a
        assert np.array_equal(feat, fx[f"aug{a}_feat"]), a
        # per-fragment CenterShift(apply_z=False): compare on the reference's own fragment-0 member set
        i0 = fx[f"aug{a}_frag0_index"]
        ops.bind_stream()
        sub = ops.gather_rows((tt.apply_aug(ops.center_shift(coord, True), normal, tt.SCANNET_TTA[a])[0]).contiguous(),
                              dev(i0.astype(np.int32)))
        got = ops.center_shift(sub, apply_z=False).cpu().numpy()
        ops.unbind_stream()
        assert np.array_equal(got.astype(np.float32) if fx[f"aug{a}_frag0_coord"].dtype == np.float32 else got,
                              fx[f"aug{a}_frag0_coord"]), a
        pos += k


# ------------------------------------------------------------------ deep-stage fused head / tail (csrc/deep.hip)
def _deep_case(M, C, seed, with_t):
    g = torch.Generator().manual_seed(seed)
    bf = LP()
    rnd = lambda *sh, s=1.0: _bf16_round(torch.randn(*sh, generator=g) * s)  # noqa: E731
    d = dict(y=rnd(M, C), o=rnd(M, C), wl=rnd(C, C, s=C ** -0.5), wq=rnd(3 * C, C, s=C ** -0.5), wp=rnd(C, C, s=C ** -0.5),
             w1=rnd(4 * C, C, s=C ** -0.5), w2=rnd(C, 4 * C, s=(4 * C) ** -0.5))
    for k, n_ in (("bl", C), ("bq", 3 * C), ("bp", C), ("b1", 4 * C), ("b2", C), ("g1", C), ("e1", C), ("g2", C), ("e2", C),
                  ("g3", C), ("e3", C)):
        d[k] = torch.randn(n_, generator=g) * (0.3 if k[0] == "b" else 1.0)
    d["cb"] = torch.randn(C, generator=g) if with_t else None
    d["x0"] = torch.randn(M, C, generator=g)
    return d, bf


@LPS
@pytest.mark.parametrize("M,C,tb", [(779, 512, True), (31, 512, False), (3364, 256, True), (2561, 512, True), (97, 256, False),
                                    (1000, 128, True)])
def test_deep_head_and_tail_split_over_workgroups_equal_the_in_place_forms(ops, lp, M, C, tb):
    """Round 6 (csrc/deep.hip, cdseg_cpe_head_rr2 / cdseg_attn_tail_rr2): few-row launches cut a tile's weight stream over
    three (head: q / k / v column blocks) or four (tail: MLP hidden chunks + a fixed-order reduce launch) workgroups, with the
    residual rows read from one buffer and written to another.  Head: every output is the same chain of products in the
    same order -> BIT-identical to the in-place launch.  Tail: the partial sums meet in a different order -> fp32 rounding
    of the row only; deterministic (two runs are bit-identical).  C = 128 never splits (same entry points, unsplit path)."""
    d, bf = _deep_case(M, C, M * 7 + C, tb)
    D = lambda k, dt=None: None if d[k] is None else dev(d[k], dt)  # noqa: E731
    himg, timg = ops.block_rr_pack(C, D("wl", bf), D("wq", bf), D("wp", bf), D("w1", bf), D("w2", bf))
    # ---- head
    xa, qa = D("x0"), torch.full((M, 3 * C), float("nan"), dtype=bf, device="cuda")
    ops.cpe_head_rr(D("y", bf), himg, D("bl"), (D("g1"), D("e1")), xa, D("cb"), (D("g2"), D("e2")), D("bq"), qa,
                    qkv_flags=ops.ATTN_V_BF16)
    x_in, x_out = D("x0"), torch.full((M, C), float("nan"), dtype=torch.float32, device="cuda")
    qb = torch.full((M, 3 * C), float("nan"), dtype=bf, device="cuda")
    with ops.record_routes() as rr:
        ops.cpe_head_rr2(D("y", bf), himg, D("bl"), (D("g1"), D("e1")), x_in, x_out, D("cb"), (D("g2"), D("e2")), D("bq"), qb,
                         qkv_flags=ops.ATTN_V_BF16)
    torch.cuda.synchronize()
    # the launch record: workgroups per 32-row tile - the head 3, the tail 4 (or 2) at C = 512 while tiles x split <= 256
    head_split, tail_split = {(779, 512): (3, 4), (31, 512): (3, 4), (2561, 512): (3, 2)}.get((M, C), (1, 1))
    assert [(r.kernel, r.aux) for r in rr.routes] == [(f"deep_head_kernel<{C},32,1>", head_split)], rr.routes
    assert torch.equal(x_in, D("x0")), "the rows read must stay untouched"
    assert torch.equal(x_out, xa) and torch.equal(qb.view(torch.int16), qa.view(torch.int16))
    # ---- tail
    xa, xca = D("x0"), torch.full((M, C), float("nan"), dtype=bf, device="cuda")
    ops.attn_tail_rr(D("o", bf), timg, D("bp"), D("g3"), D("e3"), D("b1"), D("b2"), xa, xca)
    ws = torch.empty(4 * M * C * 4 + 64, dtype=torch.uint8, device="cuda")
    outs = []
    for _ in range(2):
        x_in, xb = D("x0"), torch.full((M, C), float("nan"), dtype=torch.float32, device="cuda")
        xcb = torch.full((M, C), float("nan"), dtype=bf, device="cuda")
        with ops.record_routes() as rr:
            ops.attn_tail_rr2(D("o", bf), timg, D("bp"), D("g3"), D("e3"), D("b1"), D("b2"), x_in, xb, xcb, ws=ws)
        torch.cuda.synchronize()
        assert [(r.kernel, r.aux) for r in rr.routes] == [(f"deep_tail_kernel<{C},32,1>", tail_split)], rr.routes
        assert torch.equal(x_in, D("x0"))
        outs.append((xb, xcb))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1].view(torch.int16), outs[1][1].view(torch.int16))
    xb, xcb = outs[0]
    dd = (xb - xa).abs().max().item()
    report(f"deep tail split vs in place M={M} C={C} {lp}", max_diff=dd, row_norm=float(xa.norm(dim=1).mean()))
    assert dd < 4e-6 * C ** 0.5 * max(1.0, float(xa.abs().max()))
    assert torch.equal(xcb, xb.to(bf))
    # without a workspace the same entry point runs the unsplit tail: bit-identical to the in-place form
    x_in, xc2 = D("x0"), torch.empty(M, C, dtype=torch.float32, device="cuda")
    with ops.record_routes() as rr:
        ops.attn_tail_rr2(D("o", bf), timg, D("bp"), D("g3"), D("e3"), D("b1"), D("b2"), x_in, xc2, None, ws=None)
    assert [(r.kernel, r.aux) for r in rr.routes] == [(f"deep_tail_kernel<{C},32,1>", 1)], rr.routes
    assert torch.equal(xc2, xa)


@LPS
@pytest.mark.parametrize("M,C,tb", [(1000, 128, True), (4097, 256, False), (33, 256, True), (20480, 128, False),
                                    (20481, 256, True), (130000, 128, True), (6200, 512, True), (779, 512, False),
                                    (31, 512, True)])
def test_deep_head_and_tail_vs_oracle_and_unfused_sequence(ops, lp, M, C, tb):
    """csrc/deep.hip (C = 128 / 256: activations of a row tile resident in LDS, weights streamed L2 -> registers, 128- and
    32-row workgroups, ragged last tile) against (i) the oracle's Block pieces in fp64 torch with the kernel's 16-bit
    rounding points (oracle/model.py: cpe / block, ptv3.py:401-427) and (ii) the unfused HIP launches it replaces.  Same
    products and rounding points; the fp32 summation order differs, so: residual stream within fp32 rounding of the row
    norm, 16-bit outputs within isolated rounding-boundary flips."""
    d, bf = _deep_case(M, C, M * 11 + C, tb)
    D = lambda k, dt=None: None if d[k] is None else dev(d[k], dt)  # noqa: E731
    assert ops.block_rr_ok(C, bf) and ops.block_rr_head_on(C)
    himg, timg = ops.block_rr_pack(C, D("wl", bf), D("wq", bf), D("wp", bf), D("w1", bf), D("w2", bf))
    f64 = lambda k: d[k].double()  # noqa: E731
    # ---- head
    xa, qa = D("x0"), torch.full((M, 3 * C), float("nan"), dtype=bf, device="cuda")
    with ops.record_routes() as rr:
        ops.cpe_head_rr(D("y", bf), himg, D("bl"), (D("g1"), D("e1")), xa, D("cb"), (D("g2"), D("e2")), D("bq"), qa)
    # the launch record: 128-row workgroups at C = 128 / 256 from 160 tiles of 128 rows (20 353 rows), else 32-row ones (C = 512:
    # 32 rows below DEEP512_ROWS64_MIN); in place, so one workgroup per tile
    rows = (64 if M >= ops.DEEP512_ROWS64_MIN else 32) if C == 512 else (128 if (M + 127) // 128 >= 160 else 32)
    tile = f"{C},{rows},{2 if rows == 64 else 1}"
    assert [(r.kernel, r.bm, r.aux) for r in rr.routes] == [(f"deep_head_kernel<{tile}>", rows, 1)], rr.routes
    t = f64("y") @ f64("wl").t() + f64("bl")
    xr = f64("x0") + F.layer_norm(t, (C,), f64("g1"), f64("e1"), 1e-5) + (f64("cb") if tb else 0)
    hr = _bf16_round(F.layer_norm(xr, (C,), f64("g2"), f64("e2"), 1e-5).float()).double()
    qr = hr @ f64("wq").t() + f64("bq")
    ex = (xa.cpu().double() - xr).abs().max().item()
    eq = (qa.cpu().double() - qr).abs()
    report(f"deep head M={M} C={C} {lp}", x_err=ex, qkv_max=eq.max().item(), qkv_mean=eq.mean().item())
    assert ex < 2e-5 * C ** 0.5
    assert eq.max().item() < (0.08 if lp == "bf16" else 0.012) and eq.mean().item() < (4e-3 if lp == "bf16" else 6e-4)
    xb, hb, qb = D("x0"), torch.empty(M, C, dtype=bf, device="cuda"), torch.empty(M, 3 * C, dtype=bf, device="cuda")
    ops.gemm(D("y", bf), D("wl", bf), xb, bias=D("bl"), ln_pre=(D("g1"), D("e1")), res=xb, colbias=D("cb"),
             ln_post=(D("g2"), D("e2")), ln_out=hb)
    ops.gemm(hb, D("wq", bf), qb, bias=D("bq"))
    dq = (qa.float() - qb.float()).abs()
    assert (xa - xb).abs().max().item() < 2e-5 * C ** 0.5
    assert dq.max().item() < (0.08 if lp == "bf16" else 0.012) and dq.mean().item() < 2e-4
    # ---- tail
    xa, xca = D("x0"), torch.full((M, C), float("nan"), dtype=bf, device="cuda")
    with ops.record_routes() as rr:
        ops.attn_tail_rr(D("o", bf), timg, D("bp"), D("g3"), D("e3"), D("b1"), D("b2"), xa, xca)
    assert [(r.kernel, r.bm, r.aux) for r in rr.routes] == [(f"deep_tail_kernel<{tile}>", rows, 1)], rr.routes
    x1 = f64("x0") + f64("o") @ f64("wp").t() + f64("bp")
    h2 = _bf16_round(F.layer_norm(x1, (C,), f64("g3"), f64("e3"), 1e-5).float()).double()
    u = _bf16_round(F.gelu(h2 @ f64("w1").t() + f64("b1")).float()).double()
    ref = x1 + u @ f64("w2").t() + f64("b2")
    e = (xa.cpu().double() - ref).abs()
    report(f"deep tail M={M} C={C} {lp}", max_err=e.max().item(), mean_err=e.mean().item())
    assert e.max().item() < (3e-2 if lp == "bf16" else 5e-3) and e.mean().item() < (6e-4 if lp == "bf16" else 3e-4)
    assert torch.equal(xca, xa.to(bf))
    xb, h2b, xcb = D("x0"), torch.empty(M, C, dtype=bf, device="cuda"), torch.empty(M, C, dtype=bf, device="cuda")
    ops.gemm(D("o", bf), D("wp", bf), xb, bias=D("bp"), res=xb, ln_post=(D("g3"), D("e3")), ln_out=h2b)
    ub = torch.empty(M, 4 * C, dtype=bf, device="cuda")
    ops.gemm(h2b, D("w1", bf), ub, bias=D("b1"), act=ops.ACT_GELU)
    ops.gemm(ub, D("w2", bf), xb, bias=D("b2"), res=xb, out2=xcb)
    dd = (xa - xb).abs()
    report(f"deep tail vs unfused M={M} C={C} {lp}", max_diff=dd.max().item(), mean_diff=dd.mean().item())
    # (same GELU polynomial in both; hidden values on a 16-bit rounding boundary flip with the fp32 summation order)
    assert dd.max().item() < (3e-2 if lp == "bf16" else 5e-3) and dd.mean().item() < (4e-4 if lp == "bf16" else 6e-5)


_SQ256, _SQ128, _T128 = ("gemm_dma_kernel<256,gather,256,2,sq>", "gemm_dma_kernel<256,gather,128,2,sq>",
                         "gemm_dma_kernel<128,gather,128,2,ring>")
# (rows, C) -> (kernel, split-K) as recorded.  The 256 x 256 tile needs the split-K workspace, and ops.gemm hands one out only
# while 128 x 256 tiles stay below 256 blocks: (66000, 256) runs 128 x 128 tiles without split-K, not the 256-row tiles this
# table's comment used to claim for it (tests/test_gpu_routes.py holds that tile's no-split case: 8001 / 32767 rows, C = 128).
DEEP_CONV_TILES = {(5000, 256): (_SQ256, True), (2100, 512): (_T128, True), (130, 256): (_T128, True), (40000, 128): (_T128, False),
                   (30000, 256): (_SQ256, True), (6100, 512): (_SQ256, True), (66000, 256): (_T128, False),
                   (12000, 128): (_SQ128, True), (8001, 128): (_SQ128, True)}


@LPS
@pytest.mark.parametrize("n,C", [(5000, 256), (2100, 512), (130, 256), (40000, 128), (30000, 256), (6100, 512),
                                 (66000, 256),   # 516 row tiles of 128: no workspace, no split-K, the tile's own 16-bit epilogue
                                 (12000, 128), (8001, 128)])  # C = 128 on the 8-wave 256 x 128 tile (8000 <= rows < 32768)
def test_deep_conv_group_skipping_random_map(ops, lp, n, C):
    """The deep-stage gathered conv (gemm.hip: 16-row groups without a neighbour at an offset are neither fetched nor
    multiplied; C >= 256 at >= 5000 rows: 256 x 256 tiles on 8 waves with split-K over the live offsets - the (5000, 256),
    (30000, 256) and (6100, 512) cases, ragged last tiles included - else 128 x 128 tiles, split-K when the grid is small) on a random
    offset-major kernel map with whole dead (group, offset) pairs, dead offsets and ragged last tiles, against a plain
    fp32 torch gather + matmul per offset on the same 16-bit operands (ref: spconv.SubMConv3d call sites ptv3.py:356-362)."""
    g = torch.Generator().manual_seed(n + C)
    bf = LP()
    ngrp = (n + 15) // 16
    grp_on = torch.rand(27, ngrp, generator=g) > 0.35
    grp_on[3] = False  # an offset nobody has
    grp_on[:, : max(1, ngrp // 7)] &= torch.rand(27, 1, generator=g) > 0.5  # tiles with few live offsets
    row_on = (torch.rand(27, n, generator=g) > 0.5) & grp_on.repeat_interleave(16, dim=1)[:, :n]
    nbr = torch.where(row_on, torch.randint(0, n, (27, n), generator=g), torch.full((27, n), -1)).int()
    x = _bf16_round(torch.randn(n, C, generator=g))
    w = _bf16_round(torch.randn(C, 27, C, generator=g) / (13 * C) ** 0.5)
    b = torch.randn(C, generator=g)
    xd, wd, nd = dev(x), dev(w), dev(nbr)
    ref = dev(b).repeat(n, 1)
    for o in range(27):
        idx = nd[o].long()
        ref += torch.where((idx >= 0)[:, None], xd[idx.clamp(min=0)], torch.zeros((), device="cuda")) @ wd[:, o, :].t()
    out = torch.full((n, C), float("nan"), dtype=bf, device="cuda")
    with ops.record_routes() as rr:
        ops.gemm(dev(x, bf), dev(w.reshape(C, -1), bf), out, bias=dev(b), nbr=nd, nbr_kmajor=True, kvol=27)
    # the launch record: which tile each case runs on, and split-K or not (DEEP_CONV_TILES)
    assert [(r.kernel, r.splits > 1) for r in rr.routes] == [DEEP_CONV_TILES[(n, C)]], rr.routes
    err = (out.float() - ref).abs().max().item()
    report(f"deep conv random map n={n} C={C} {lp}", max_err=err, ref_max=ref.abs().max().item())
    assert err < (0.04 if lp == "bf16" else 0.006)  # 16-bit rounding of outputs of magnitude ~4
    out32 = torch.empty(n, C, dtype=torch.float32, device="cuda")
    with ops.record_routes() as rr:
        ops.gemm(dev(x, bf), dev(w.reshape(C, -1), bf), out32, bias=dev(b), nbr=nd, nbr_kmajor=True, kvol=27)
    assert [(r.kernel, r.splits > 1) for r in rr.routes] == [DEEP_CONV_TILES[(n, C)]], rr.routes
    assert (out32 - ref).abs().max().item() < 2e-4


@LPS
@pytest.mark.parametrize("cin,cout,m,maxrun,seed", [(32, 64, 1000, 8, 0), (64, 128, 777, 8, 1), (32, 64, 5, 70, 2), (32, 64, 40000, 8, 3),
                                                  (64, 128, 3000, 64, 4), (32, 64, 1, 1, 5)])
def test_pool_fused_equals_gemm_then_segment_max(ops, lp, cin, cout, m, maxrun, seed):
    """cdseg_pool_fused (csrc/pool.hip: SerializedPooling's projection + segment maximum + folded BatchNorm + GELU in one
    launch, ref: ptv3.py:506-515, 548-551) == cdseg_gemm into a 16-bit buffer followed by cdseg_segment_max, BIT FOR BIT
    (rounding to the 16-bit type is monotonic, so it commutes with the maximum), on ragged runs - single children, runs longer
    than a 16-row strip (the c-branch pools 4 x 4 x 4 cells), a last chunk of fewer than 16 pooled rows - and against plain
    torch on the same 16-bit operands."""
    g = torch.Generator().manual_seed(seed)
    bf = LP()
    runs = torch.randint(1, maxrun + 1, (m,), generator=g)
    seg = torch.cat([torch.zeros(1, dtype=torch.int64), runs.cumsum(0)]).int()
    n = int(seg[-1])
    x = _bf16_round(torch.randn(n, cin, generator=g))
    w = _bf16_round(torch.randn(cout, cin, generator=g) / cin ** 0.5)
    b = torch.randn(cout, generator=g) * 0.3
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.2
    sc[::7] *= -1.0  # a folded BatchNorm scale can be negative: the maximum is taken BEFORE it
    xd, wd, segd = dev(x, bf), dev(w, bf), dev(seg)
    assert ops.pool_fused_ok(cin, cout, bf)
    img = ops.pool_fused_pack(wd)
    out = torch.full((m, cout), float("nan"), device="cuda")
    out2 = torch.full((m, cout), float("nan"), dtype=bf, device="cuda")
    ops.pool_fused(xd, img, dev(b), segd, m, dev(sc), dev(sh), ops.ACT_GELU, out, out2)
    y = torch.empty(n, cout, dtype=bf, device="cuda")
    ops.gemm(xd, wd, y, bias=dev(b))
    ref, ref2 = torch.empty(m, cout, device="cuda"), torch.empty(m, cout, dtype=bf, device="cuda")
    ops.segment_max(y, segd, m, dev(sc), dev(sh), ops.ACT_GELU, ref, ref2)
    report(f"pool fused vs two launches {cin}->{cout} m={m} {lp}", fp32_mismatches=int((out != ref).sum()),
           lp_mismatches=int((out2 != ref2).sum()), max_diff=(out - ref).abs().max().item())
    assert torch.equal(out, ref) and torch.equal(out2, ref2)
    cluster = torch.repeat_interleave(torch.arange(m), runs)
    yt = _bf16_round(x @ w.t() + b)
    mx = torch.full((m, cout), -float("inf")).scatter_reduce(0, cluster[:, None].expand(-1, cout), yt, "amax")
    want = F.gelu(mx * sc + sh)
    err = (out.cpu() - want).abs().max().item()
    report(f"pool fused {cin}->{cout} m={m} {lp}", max_err=err)
    assert err < (2e-2 if lp == "bf16" else 3e-3)  # (a projected value on a 16-bit rounding boundary: fp32 summation order)
    # no scale / shift / activation, no 16-bit copy
    out3 = torch.empty(m, cout, device="cuda")
    ops.pool_fused(xd, img, None, segd, m, None, None, ops.ACT_NONE, out3)
    y0 = torch.empty(n, cout, dtype=bf, device="cuda")
    ops.gemm(xd, wd, y0)
    ref3 = torch.empty(m, cout, device="cuda")
    ops.segment_max(y0, segd, m, None, None, ops.ACT_NONE, ref3)
    assert torch.equal(out3, ref3)


# The arms of block_forward_impl (csrc/runtime.hip) that the product constants leave reachable: the consecutive kernel-name prefixes
# an arm must leave in the launch record, and the cases (keys of BLOCK_ROUTES) that run it -
# test_every_block_forward_arm_is_recorded_by_its_cases holds the two tables against each other,
# test_native_block_executor_vs_oracle_block and its siblings hold BLOCK_ROUTES against the record and the result against oracle/
# model.py's Block.  Case keys: (npts, C, variant) - False = the descriptor the engine builds (tail image; head image at deep widths),
# True = a wide-stage head image on top, "f32" = an fp32 descriptor, "none" / "head-only" / "tail-only" = 16-bit descriptors with
# those weight images only.
_CONV_GEMM = ("gemm_dma_kernel<128,gather", "gemm_dma_kernel<256,gather", "gemm_kernel<b16,128,klong,gather", "gemm_kernel<f32,64,klong,gather")
BLOCK_ARMS = {
    "conv: weight-stationary cdseg_subm_conv3 (16-bit, C = 32 / 64, packed image)":
        (["conv_ll_kernel<"], [(900, 32, False), (2300, 64, False), (600, 32, True), (700, 64, "none")]),
    "conv: gathered GEMM that leaves its split-K planes to the deep head (C = 128 / 256, head image)":
        ([_CONV_GEMM, "deep_head_kernel<"], [(2300, 128, False), (5300, 256, False), (40, 256, False), (1000, 128, "head-only")]),
    "conv: gathered GEMM through cdseg_gemm (C = 512; no head image; fp32 descriptors)":
        ([_CONV_GEMM], [(3200, 512, False), (790, 512, False), (900, 64, "f32"), (1000, 128, "tail-only"), (1000, 128, "none"),
                        (600, 256, "none"), (2600, 512, "head-only")]),
    "head: deep_head on the conv's partial planes, residual ping-pong":
        (["deep_head_kernel<"], [(2300, 128, False), (5300, 256, False), (40, 256, False)]),
    "head: deep_head on the conv's partial planes, in place (head image without tail image)":
        (["deep_head_kernel<128,32,1>", "attn_", "gemm_kernel<b16,128,klong,plain,64>"], [(1000, 128, "head-only")]),
    "head: cdseg_cpe_head_rr2, residual ping-pong (deep stages whose conv left no planes)":
        (["gemm_dma_kernel<128,gather", "deep_head_kernel<512,32,1>", "attn_", "deep_tail_kernel<"], [(3200, 512, False), (790, 512, False)]),
    "head: cdseg_cpe_head_rr at C = 32 / 64 (a wide-stage head image)": (["head_rr_kernel<"], [(600, 32, True)]),
    "head: cdseg_cpe_head_rr at deep widths (head image, no ping-pong buffer, conv finished by itself)":
        (["gemm_dma_kernel<128,gather", "deep_head_kernel<512,32,1>", "attn_", "gemm_dma_kernel<64,plain"], [(2600, 512, "head-only")]),
    "head: cdseg_cpe_head_fused (C = 32 / 64 without a head image: what the engine passes)":
        (["cpe_head_fused_kernel<"], [(900, 32, False), (2300, 64, False), (700, 64, "none")]),
    "head: GEMM + fused LayerNorm, then the qkv GEMM (fp32 descriptors; 16-bit deep widths without a head image)":
        ([_CONV_GEMM, ("gemm_kernel<", "gemm_dma_kernel<64,plain"), ("gemm_kernel<", "gemm_dma_kernel<64,plain"), "attn_"],
         [(900, 64, "f32"), (1000, 128, "tail-only"), (1000, 128, "none"), (600, 256, "none")]),
    "head: GEMM + two cdseg_layernorm launches, and proj GEMM + cdseg_layernorm (C > 512: rows wider than a fused LayerNorm finishes)":
        (["gemm_kernel<b16,128,klong,gather,128>", "gemm_kernel<b16,128,klong,plain,64>", "layernorm_kernel<4>", "layernorm_kernel<4>",
          "gemm_kernel<b16,128,klong,plain,64>", "attn_", "gemm_kernel<b16,128,klong,plain,64>", "layernorm_kernel<4>",
          "gemm_kernel<b16,128,klong,plain,64>", "gemm_dma_kernel<64,plain"], [(200, 528, "none")]),
    "tail: cdseg_attn_tail_rr2 (ping-pong)":
        (["attn_", "deep_tail_kernel<"], [(2300, 128, False), (5300, 256, False), (40, 256, False), (3200, 512, False), (790, 512, False)]),
    "tail: cdseg_attn_tail_rr at deep widths (tail image without head image: no ping-pong buffer)":
        (["gemm_dma_kernel<64,plain", "attn_", "deep_tail_kernel<128,32,1>"], [(1000, 128, "tail-only")]),
    "tail: cdseg_attn_tail_rr (C = 32 / 64 with a tail image)":
        (["attn_", "tail_rr_kernel<"], [(900, 32, False), (2300, 64, False), (600, 32, True)]),
    "tail: cdseg_attn_tail_fused (C = 32 / 64 without a tail image)": (["attn_", "mlp_fused_kernel<64,64,proj,64>"], [(700, 64, "none")]),
    "tail: proj GEMM + LayerNorm, then cdseg_mlp_fused (16-bit C = 128 without a tail image)":
        (["attn_", "gemm_kernel<b16,128,klong,plain,64>", "mlp_fused_kernel<128,64,mlp,64>"], [(1000, 128, "none"), (1000, 128, "head-only")]),
    "tail: proj GEMM + LayerNorm, then the two MLP GEMMs (fp32 descriptors; 16-bit C >= 256 without a tail image)":
        (["attn_", ("gemm_kernel<", "gemm_dma_kernel<64,plain"), ("gemm_kernel<", "gemm_dma_kernel<"), ("gemm_kernel<", "gemm_dma_kernel<64,plain")],
         [(900, 64, "f32"), (600, 256, "none"), (2600, 512, "head-only")]),
}
_ATT = dict(kernel="attn_bf16_kernel<")
_G128 = dict(kernel="gemm_kernel<b16,128,klong,plain,64>", split=False)   # a 16-bit GEMM whose LayerNorm is finished in its tile
_D64 = dict(kernel="gemm_dma_kernel<64,plain,128,2,ring>", split=False)
_LN4 = dict(kernel="layernorm_kernel<4>", split=False)                    # a cdseg_layernorm launch on rows of 513 .. 1024 channels
BLOCK_ROUTES = {
    (900, 32, False): [dict(kernel="conv_ll_kernel<32>"), dict(kernel="cpe_head_fused_kernel<32,64>"), _ATT, dict(kernel="tail_rr_kernel<32>")],
    (2300, 64, False): [dict(kernel="conv_ll_kernel<64>"), dict(kernel="cpe_head_fused_kernel<64,64>"), _ATT, dict(kernel="tail_rr_kernel<64>")],
    (600, 32, True): [dict(kernel="conv_ll_kernel<32>"), dict(kernel="head_rr_kernel<32>"), _ATT, dict(kernel="tail_rr_kernel<32>")],
    # no images at C = 64: the fused head and the fused proj + LayerNorm + MLP tail of mlp.hip
    (700, 64, "none"): [dict(kernel="conv_ll_kernel<64>"), dict(kernel="cpe_head_fused_kernel<64,64>"), _ATT,
                        dict(kernel="mlp_fused_kernel<64,64,proj,64>")],
    # an fp32 descriptor: conv on the 128-row gathered loop with split-K, CPE Linear with both LayerNorms in its tile, qkv, the fp32
    # attention kernel, proj with LayerNorm 2 in its tile, fc1 (GELU), fc2 - seven launches, reductions of 64 on the short-K kernels
    (900, 64, "f32"): [dict(kernel="gemm_kernel<f32,64,klong,gather,128>", split=True, partials=False),
                       dict(kernel="gemm_kernel<f32,64,kshort,plain,64>", split=False), dict(kernel="gemm_kernel<f32,128,kshort,plain,64>"),
                       dict(kernel="attn_f32_kernel"), dict(kernel="gemm_kernel<f32,64,kshort,plain,64>", split=False),
                       dict(kernel="gemm_kernel<f32,128,kshort,plain,64>"), dict(kernel="gemm_kernel<f32,64,klong,plain,64>", split=False)],
    # C = 128 with the tail image only: the conv finishes its own split-K, GEMM + LayerNorm head and qkv GEMM, the deep tail in place
    (1000, 128, "tail-only"): [dict(kernel="gemm_dma_kernel<128,gather,128,2,ring>", split=True, partials=False), _G128, _D64, _ATT,
                               dict(kernel="deep_tail_kernel<128,32,1>", nsplit=1)],
    # C = 128 without images: ... proj GEMM + LayerNorm, then the fused MLP
    (1000, 128, "none"): [dict(kernel="gemm_dma_kernel<128,gather,128,2,ring>", split=True, partials=False), _G128, _D64, _ATT, _G128,
                          dict(kernel="mlp_fused_kernel<128,64,mlp,64>")],
    # C = 128 with the head image only: the head sums the conv's planes and updates x in place; GEMM tail
    (1000, 128, "head-only"): [dict(kernel="gemm_dma_kernel<128,gather,128,2,ring>", split=True, partials=True),
                               dict(kernel="deep_head_kernel<128,32,1>", nsplit=1, ysum=True), _ATT, _G128,
                               dict(kernel="mlp_fused_kernel<128,64,mlp,64>")],
    # C = 256 without images: rows of two column tiles, so both LayerNorm GEMMs go through the row-finish pass; two MLP GEMMs
    (600, 256, "none"): [dict(kernel="gemm_dma_kernel<128,gather,128,2,ring>", split=True, partials=False), _D64, _D64, _ATT, _D64, _D64, _D64],
    # C = 512 with the head image only, enough rows for the deep head without the ping-pong buffer: cdseg_cpe_head_rr in place;
    # proj + LayerNorm over four column tiles, fc1 on 128-row tiles (N = 2048, 2600 rows), fc2 with split-K (16 K steps, 164 tiles)
    (2600, 512, "head-only"): [dict(kernel="gemm_dma_kernel<128,gather,128,2,ring>", split=True, partials=False),
                               dict(kernel="deep_head_kernel<512,32,1>", nsplit=1, ysum=False), _ATT, _D64,
                               dict(kernel="gemm_dma_kernel<128,plain,128,2,ring>", split=False),
                               dict(kernel="gemm_dma_kernel<64,plain,128,2,ring>", split=True)],
    # C = 528 (33 heads; K no power of two and no multiple of 64): no LayerNorm is fused - the three cdseg_layernorm launches between
    # the GEMMs are recorded (132 chunks a row on 64 lanes: three of layernorm_kernel<4>'s four passes) -, the conv divides in its
    # gather and splits K, fc2 (K = 2112: 17 K steps) runs the DMA loop with split-K
    (200, 528, "none"): [dict(kernel="gemm_kernel<b16,128,klong,gather,128>", split=True, partials=False), _G128, _LN4, _LN4, _G128, _ATT,
                         _G128, _LN4, _G128, dict(kernel="gemm_dma_kernel<64,plain,128,2,ring>", split=True)],
    (2300, 128, False): [dict(kernel="gemm_dma_kernel<128,gather,128,2,ring>", split=True, partials=True),
                         dict(kernel="deep_head_kernel<128,32,1>", nsplit=1, ysum=True), _ATT,
                         dict(kernel="deep_tail_kernel<128,32,1>", nsplit=1)],
    (5300, 256, False): [dict(kernel="gemm_dma_kernel<256,gather,256,2,sq>", split=True, partials=True),
                         dict(kernel="deep_head_kernel<256,32,1>", nsplit=1, ysum=True), _ATT,
                         dict(kernel="deep_tail_kernel<256,32,1>", nsplit=1)],
    (40, 256, False): [dict(kernel="gemm_kernel<b16,128,klong,gather,64>", split=True, partials=True),
                       dict(kernel="deep_head_kernel<256,32,1>", nsplit=1, ysum=True), _ATT,
                       dict(kernel="deep_tail_kernel<256,32,1>", nsplit=1)],
    # C = 512: the conv finishes its own split-K; 3200 rows (100 tiles) leave the head whole and cut the tail in two, 790 rows
    # (25 tiles) cut the head in three and the tail in four
    (3200, 512, False): [dict(kernel="gemm_dma_kernel<128,gather,128,2,ring>", split=True, partials=False),
                         dict(kernel="deep_head_kernel<512,32,1>", nsplit=1, ysum=False), _ATT,
                         dict(kernel="deep_tail_kernel<512,32,1>", nsplit=2)],
    (790, 512, False): [dict(kernel="gemm_dma_kernel<128,gather,128,2,ring>", split=True, partials=False),
                        dict(kernel="deep_head_kernel<512,32,1>", nsplit=3, ysum=False), _ATT,
                        dict(kernel="deep_tail_kernel<512,32,1>", nsplit=4)],
}


def test_every_block_forward_arm_is_recorded_by_its_cases():
    """Every arm names the run of kernels it must leave in the record; each case credited to it must hold that run in BLOCK_ROUTES
    (which the cases themselves are held to on the GPU), and every case is credited to some arm."""
    credited = set()
    for arm, spec in BLOCK_ARMS.items():
        if isinstance(spec, str):
            assert spec, arm
            continue
        run, cases = spec
        assert run and cases, arm
        for key in cases:
            names = [step["kernel"] for step in BLOCK_ROUTES[key]]
            fits = lambda name, pre: any(name.startswith(q) or q.startswith(name) for q in ((pre,) if isinstance(pre, str) else pre))  # noqa: E731
            assert any(all(fits(n, q) for n, q in zip(names[i:i + len(run)], run)) for i in range(len(names) - len(run) + 1)), (arm, key, names)
            credited.add(key)
    assert credited == set(BLOCK_ROUTES), set(BLOCK_ROUTES) - credited


def test_native_block_executor_with_an_fp32_descriptor_vs_oracle_block(ops):
    """The GEMM + LayerNorm arms of block_forward_impl (head, proj, the two MLP GEMMs, the fp32 attention kernel): what every
    Block of an fp32 engine runs - same oracle, fp32 bound."""
    test_native_block_executor_vs_oracle_block(ops, "bf16", 900, 64, True, False, fp32_desc=True)


@LPS
@pytest.mark.parametrize("npts,C,tb,fold,imgs", [(700, 64, True, False, "none"), (1000, 128, False, True, "tail-only"),
                                                 (1000, 128, True, False, "none"), (1000, 128, True, True, "head-only"),
                                                 (600, 256, False, False, "none"), (2600, 512, True, False, "head-only"),
                                                 (200, 528, True, False, "none")])
def test_native_block_executor_without_some_weight_images_vs_oracle_block(ops, lp, npts, C, tb, fold, imgs):
    """16-bit descriptors the C ABI admits and the engine never builds - no weight images, the head image alone, the tail image
    alone: the arms of block_forward_impl behind `tail_img == NULL` / `head_img == NULL` (cdseg_attn_tail_fused, the deep tail and
    the deep head without the ping-pong buffer, the GEMM + LayerNorm head and tail in 16 bits, cdseg_mlp_fused at C = 128, the two
    MLP GEMMs) with their argument plumbing - same oracle, same bounds as the engine's descriptors."""
    test_native_block_executor_vs_oracle_block(ops, lp, npts, C, tb, fold, imgs=imgs)


@LPS
def test_native_block_executor_with_a_wide_stage_head_image_vs_oracle_block(ops, lp):
    """The cdseg_cpe_head_rr arm of block_forward_impl: a C = 32 descriptor that carries a head image (the register-resident head
    of the wide stages, which the engine leaves off) - same oracle, same bounds as the cases below."""
    test_native_block_executor_vs_oracle_block(ops, lp, 600, 32, True, False, wide_head=True)


@LPS
@pytest.mark.parametrize("npts,C,tb,fold", [(900, 32, True, False), (2300, 64, False, True), (2300, 128, True, False),
                                            (5300, 256, False, True), (40, 256, True, False), (3200, 512, True, True),
                                            (790, 512, False, False)])
def test_native_block_executor_vs_oracle_block(ops, lp, npts, C, tb, fold, wide_head=False, fp32_desc=False, imgs=None):
    """cdseg_block_forward - ONE host call per Block: sparse conv, fused head, attention, fused tail, the kernels the
    timed configuration runs at C = 32 / 64 (conv.hip, mlp.hip, blockrr.hip) and C = 128 / 256 (gemm.hip, deep.hip) -
    against oracle/model.py's Block (ref: ptv3.py:399-428) in fp32 on the SAME 16-bit-rounded weights and input, on the
    real kernel map of a synthetic scene and the real padded patch plan (K = 1024, last patch borrowed), ragged row
    counts.  What differs is the 16-bit rounding of the intermediate activations (conv output, LN output, q k v,
    attention output, hidden units): bounds per build below, measured values in profiles/*_parity_measured.txt.
    Round 5: C = 512 (deep.hip's 16-wave form) and `fold` = the engine's producer-side preprocessing - the q rows of the
    qkv weight / bias handed to the library carry softmax scale * log2(e) and the descriptor says so
    (CDSEG_ATTN_Q_PRESCALED); the oracle keeps the original weights."""
    from cdsegnet_amd import synth
    from oracle import train as OT
    rng = np.random.default_rng(npts + C)
    bf = torch.float32 if fp32_desc else LP()  # fp32_desc: an fp32 descriptor (weights and activations fp32; values still on the 16-bit grid)
    H = C // 16
    sc = synth.room_scene(9, npts)
    grid = np.asarray(sc["grid_coord"], dtype=np.int64)
    n = len(grid)
    nbr = OM.subm_neighbors(grid, np.zeros(n, dtype=np.int64), 3)  # (n, 27)
    pad, unpad, cu = S.padding_plan(np.array([n]), 1024)
    perm = rng.permutation(n)
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    order, inverse = perm[pad], unpad[inv]
    r16 = lambda a: _bf16_round(torch.as_tensor(a, dtype=torch.float32)).numpy()  # noqa: E731 - rounds to the build's 16-bit type
    pre = "blk"
    sd = {}
    for k, shape in ((".cpe.0.weight", (C, 3, 3, 3, C)), (".cpe.0.bias", (C,)), (".cpe.1.weight", (C, C)), (".cpe.1.bias", (C,)),
                     (".cpe.2.weight", (C,)), (".cpe.2.bias", (C,)), (".norm1.0.weight", (C,)), (".norm1.0.bias", (C,)),
                     (".attn.qkv.weight", (3 * C, C)), (".attn.qkv.bias", (3 * C,)), (".attn.proj.weight", (C, C)),
                     (".attn.proj.bias", (C,)), (".norm2.0.weight", (C,)), (".norm2.0.bias", (C,)),
                     (".mlp.0.fc1.weight", (4 * C, C)), (".mlp.0.fc1.bias", (4 * C,)), (".mlp.0.fc2.weight", (C, 4 * C)),
                     (".mlp.0.fc2.bias", (C,))):
        scale = {1: 0.1, 2: shape[-1] ** -0.5, 5: (13 * C) ** -0.5}[len(shape)]
        v = (rng.standard_normal(shape) * scale + (1.0 if k.endswith(".weight") and len(shape) == 1 else 0.0)).astype(np.float32)
        sd[pre + k] = r16(v) if len(shape) > 1 else v
    x_in = r16(rng.standard_normal((n, C)).astype(np.float32))
    tbias = (rng.standard_normal(C) * 0.2).astype(np.float32) if tb else None
    # oracle: the t bias is a constant row added behind the CPE (ptv3.py:407-409) = a shift of cpe.2's bias
    sd_o = dict(sd)
    if tb:
        sd_o[pre + ".cpe.2.bias"] = sd[pre + ".cpe.2.bias"] + tbias
    ry, _, _ = OT.block_full_grads(sd_o, pre, x_in, nbr, order, inverse, cu, H, np.zeros((n, C), dtype=np.float32))

    f32 = lambda k: dev(sd[pre + k])  # noqa: E731
    w16 = lambda k: dev(sd[pre + k].reshape(sd[pre + k].shape[0], -1), bf)  # noqa: E731
    t = dict(cpe_conv_w=w16(".cpe.0.weight"), cpe_conv_b=f32(".cpe.0.bias"), cpe_lin_w=w16(".cpe.1.weight"),
             cpe_lin_b=f32(".cpe.1.bias"), cpe_ln_g=f32(".cpe.2.weight"), cpe_ln_b=f32(".cpe.2.bias"),
             norm1_g=f32(".norm1.0.weight"), norm1_b=f32(".norm1.0.bias"), qkv_w=w16(".attn.qkv.weight"),
             qkv_b=f32(".attn.qkv.bias"), proj_w=w16(".attn.proj.weight"), proj_b=f32(".attn.proj.bias"),
             norm2_g=f32(".norm2.0.weight"), norm2_b=f32(".norm2.0.bias"), fc1_w=w16(".mlp.0.fc1.weight"),
             fc1_b=f32(".mlp.0.fc1.bias"), fc2_w=w16(".mlp.0.fc2.weight"), fc2_b=f32(".mlp.0.fc2.bias"))
    if ops.subm_conv3_ok(torch.empty((1, C), dtype=bf, device="meta")):
        t["cpe_conv_wimg"] = ops.subm_conv3_pack(t["cpe_conv_w"])
    if fold:  # what Engine._prepare does: scale the q rows in fp32, then round to the 16-bit type
        f = 16 ** -0.5 * 1.4426950408889634
        wq = torch.as_tensor(sd[pre + ".attn.qkv.weight"]).clone()
        bq = torch.as_tensor(sd[pre + ".attn.qkv.bias"]).clone()
        wq[:C] *= f
        bq[:C] *= f
        t["qkv_w"], t["qkv_b"] = dev(wq, bf), dev(bq)
    assert ops.block_rr_ok(C, bf) != (fp32_desc or C > 512)
    if not fp32_desc and C <= 512:  # (the weight images are 16-bit, widths up to 512: other Blocks run on the GEMM arms)
        # imgs: which weight images the descriptor carries - None = what the engine packs (the tail image, and the head image at
        # deep widths), or "none" / "head-only" / "tail-only": descriptors the C ABI admits and the engine never builds
        himg, timg = ops.block_rr_pack(C, t["cpe_lin_w"], t["qkv_w"], t["proj_w"], t["fc1_w"], t["fc2_w"])
        if imgs in (None, "tail-only"):
            t["tail_img"] = timg
        if (ops.block_rr_head_on(C) or wide_head) if imgs is None else imgs == "head-only":
            t["head_img"] = himg
    desc = ops.make_block_desc(bf, C, H, 4 * C, 16 ** -0.5, 1e-5, t, attn_flags=ops.ATTN_Q_PRESCALED if fold else 0)
    gidx = dev(order.astype(np.int32))
    wi = np.full(len(order), -1, dtype=np.int32)
    wi[inverse] = np.arange(n, dtype=np.int32)
    x = dev(x_in)
    xc_in, xc_out = dev(x_in, bf), torch.full((n, C), float("nan"), dtype=bf, device="cuda")
    scratch = torch.empty(ops.block_scratch_bytes(desc, n), dtype=torch.uint8, device="cuda")
    ops.bind_stream()
    try:
        with ops.record_routes() as rr:
            ops.block_forward(desc, n, x, xc_in, xc_out, None if tbias is None else dev(tbias), dev(nbr.T.astype(np.int32)), gidx,
                              dev(wi), dev(np.asarray(cu, dtype=np.int32)), len(cu) - 1, int(np.diff(cu).max()), scratch)
    finally:
        ops.unbind_stream()
    torch.cuda.synchronize()
    # which conv, head, attention and tail the executor's callees recorded (csrc/runtime.hip block_forward_impl has no record of
    # its own: the sequence its callees leave IS its route), against BLOCK_ROUTES
    seen = [dict(kernel=r.kernel, split=r.splits > 1, partials=r.partials, nsplit=r.aux & 255, ysum=(r.aux >> 8) > 1) for r in rr.routes]
    want = BLOCK_ROUTES[(npts, C, "f32" if fp32_desc else (imgs or wide_head))]
    assert rr.count == len(want), rr.routes
    for got, exp in zip(seen, want):
        assert got["kernel"].startswith(exp["kernel"]) and all(got[k] == v for k, v in exp.items() if k != "kernel"), (got, exp, rr.routes)
    d = (x.cpu() - ry).abs()
    report(f"native Block vs oracle n={n} C={C} {lp}", max_err=d.max().item(), mean_err=d.mean().item(), ref_max=ry.abs().max().item())
    assert torch.equal(xc_out, x.to(bf))  # the 16-bit copy for the next conv is the rounded fp32 stream
    if fp32_desc:
        # fp32 throughout, against the fp32 oracle on the same values.  Every stored result has magnitude <= 8, so one rounding
        # is at most 4.8e-7; the Block chains about ten such stages (conv, Linear, two LayerNorms with gains up to ~3, qkv,
        # attention, proj, fc1, GELU, fc2) whose reductions both sides add in different orders: 10 x 3 x 4.8e-7 x 2 = 3e-5 worst
        # case, a few 1e-6 on average.  A wrong ln_eps (1e-5 against deviations of ~1 moves y by ~5e-6 |y|, i.e. 4e-5 at |y| = 8)
        # or a dropped residual does not fit under it
        assert d.max().item() < 3e-5 and d.mean().item() < 4e-6
    elif lp == "bf16":  # measured 1.1e-2 .. 1.6e-2 / 2.0e-3 .. 2.2e-3 on outputs of magnitude 6 - 8
        assert d.max().item() < 0.04 and d.mean().item() < 5e-3
    else:             # measured 1.6e-3 .. 2.9e-3 / 2.7e-4 .. 5.4e-4 (P and V of the attention are bfloat16 in this build too)
        assert d.max().item() < 7e-3 and d.mean().item() < 1.2e-3


@pytest.mark.parametrize("n,seed,offset", [(1, 0, 0), (4097, 54421566, 3), (720003, (1 << 61) + 12345, (1 << 40) + 7)])
def test_device_noise_matches_the_philox_oracle(ops, n, seed, offset):
    """cdseg_randn (the benchmark configuration's noise-branch input, `noise_source="device"`) against oracle/philox.py -
    Philox4x32-10, pinned to the Random123 known answers in tests/test_oracle.py - on the same (seed, stream offset):
    the integer stream is the published algorithm's, so what may differ is the last ulp of logf / sincosf."""
    from oracle import philox as P
    got = ops.randn((n,), seed, offset, torch.device("cuda")).cpu().numpy()
    ref = P.randn(n, seed, offset)
    err = float(np.abs(got - ref).max())
    report(f"device noise n={n}", max_abs_err=err)
    assert err < 2e-5
