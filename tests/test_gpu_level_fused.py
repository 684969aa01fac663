"""GPU: the one-launch level kernels of the wide stages (csrc/pool.hip): pooling with both folds, unpooling (further down), and
a forward with them on and off (at the end).

The one-launch pooling (cdseg_pool_fused_n) with BOTH folds of the run maximum
forced in turn - the strip walk of the one-step poolings and the segmented maximum across the 16 child lanes of a step that
the c-branch's two-step pooling takes - and left to the library's own choice, against the two launches they replace
(ops.gemm into a 16-bit buffer + ops.segment_max): `out` (fp32) and `out2` (16-bit) BIT FOR BIT, both builds.

Every case runs in guard bands with non-contiguous row strides (tests/guard_bands.py): x inside NaN rows and columns, out and
out2 inside filled ones.  Pooled rows m = 1, 15, 16, 17, 33 (a wave owns 16 pooled rows: less than one group, a full one, one
row more, two and one row); run patterns: all 1, all 8, mixed 1 .. 40 with one run of 37 children that crosses two 16-child
steps, a run that ends exactly on a step boundary, long runs on both sides of the 16-row group boundary; the fine row count
is no multiple of 16 in the mixed pattern; projected values all negative (a maximum seeded with 0 would win); values beyond
the half build's clamp at 65504."""
import functools

import pytest
import torch

from tests import guard_bands as GB
from tests.test_gpu_ops import LP, LPS, _library_variant, dev, ops, report  # noqa: F401  (fixtures: lp="f16" -> the half build)

pytestmark = pytest.mark.gpu

SHAPES = [(32, 64), (64, 128)]
PATTERNS = ["ones", "eights", "mixed", "step_end", "group_span"]
POOL_ONLY_PATTERNS = ["eights_less_one"]  # every run 8 children but the last, which has 7: one child below the scan's ratio


def make_runs(pattern, m, g):
    """The children per pooled row (every run holds at least one)."""
    if pattern == "ones":
        return torch.ones(m, dtype=torch.int64)
    if pattern == "eights":
        return torch.full((m,), 8, dtype=torch.int64)
    if pattern == "eights_less_one":
        runs = torch.full((m,), 8, dtype=torch.int64)
        runs[-1] = 7
        return runs
    runs = torch.randint(1, 41, (m,), generator=g)
    if pattern == "mixed":
        runs[m // 2] = 37  # longer than 32: in three 16-child steps wherever it starts
        if int(runs.sum()) % 16 == 0:
            runs[-1] += 1
    elif pattern == "step_end":
        runs[0] = 16  # children 0 .. 15: ends with the first step, the next run opens the second one
        if m > 2:
            runs[1], runs[2] = 5, 27  # ... and children 21 .. 47 end with the third
    elif pattern == "group_span":
        runs[min(15, m - 1)] = 21  # the last pooled row of the first wave's group
        if m > 16:
            runs[16] = 19  # the first one of the next group: its steps start at a child that is no multiple of 16
    return runs


@functools.lru_cache(maxsize=None)
def pool_case(lp, cin, cout, m, pattern, values):
    """One problem and the two launches' result on it (computed once per case, read-only afterwards)."""
    from cdsegnet_amd import ops as O
    bf = LP()
    g = torch.Generator().manual_seed(1000 * cin + 10 * m + (PATTERNS + POOL_ONLY_PATTERNS).index(pattern))
    runs = make_runs(pattern, m, g)
    seg = torch.cat([torch.zeros(1, dtype=torch.int64), runs.cumsum(0)]).int()
    n = int(seg[-1])
    x = torch.randn(n, cin, generator=g)
    w = torch.randn(cout, cin, generator=g) / cin ** 0.5
    b = torch.randn(cout, generator=g) * 0.3
    if values == "negative":
        b = b - 60.0  # |W x| stays below 10: every projected value is negative
    elif values == "huge":
        b[::2] += 7.0e4  # projected values of both signs beyond 65504: the half build clamps them, bfloat16 holds them
        b[1::4] -= 7.0e4
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.2
    sc[::7] *= -1.0
    if values == "huge":
        sc = sc * 1e-4
    d = dict(n=n, m=m, seg=dev(seg), x=dev(x, bf), w=dev(w, bf), b=dev(b), sc=dev(sc), sh=dev(sh))
    y = torch.empty(n, cout, dtype=bf, device="cuda")
    O.gemm(d["x"], d["w"], y, bias=d["b"])
    if values == "negative":
        assert float(y.float().max()) < 0.0
    if values == "huge":
        assert float(y.float().abs().max()) >= 65504.0
    d["ref"], d["ref2"] = torch.empty(m, cout, device="cuda"), torch.empty(m, cout, dtype=bf, device="cuda")
    O.segment_max(y, d["seg"], m, d["sc"], d["sh"], O.ACT_GELU, d["ref"], d["ref2"])
    d["img"] = O.pool_fused_pack(d["w"])
    torch.cuda.synchronize()
    return d


CASES = [(m, p, "normal") for p in PATTERNS for m in (1, 15, 16, 17, 33)] + \
        [(m, "mixed", v) for v in ("negative", "huge") for m in (1, 33)] + [(m, "eights_less_one", "normal") for m in (1, 17)]
POOL_SCAN_RATIO = 8  # csrc/pool.hip: left to itself the library scans from n_fine >= 8 m on


def auto_fold(ops, n_fine, m):
    return ops.POOL_FOLD_SCAN if n_fine >= POOL_SCAN_RATIO * m else ops.POOL_FOLD_WALK


def test_the_patterns_reach_both_folds_under_auto_on_either_side_of_the_ratio(ops):
    """What POOL_FOLD_AUTO picks is asserted from the launch record in the test below; this holds its case list to both
    sides of the rule: "eights" sits ON the ratio (n = 8 m: the scan), "eights_less_one" one child below it (the walk)."""
    g = torch.Generator().manual_seed(0)
    auto = {(m, p): auto_fold(ops, int(make_runs(p, m, g).sum()), m) for m, p, v in CASES if p in ("ones", "eights", "eights_less_one")}
    assert {f for (m, p), f in auto.items() if p == "eights"} == {ops.POOL_FOLD_SCAN}
    assert {f for (m, p), f in auto.items() if p == "eights_less_one"} == {ops.POOL_FOLD_WALK}
    assert {f for (m, p), f in auto.items() if p == "ones"} == {ops.POOL_FOLD_WALK}
    assert all(int(make_runs("eights", m, g).sum()) == 8 * m and int(make_runs("eights_less_one", m, g).sum()) == 8 * m - 1
               for m in (1, 17))


@LPS
@pytest.mark.parametrize("m,pattern,values", CASES)
@pytest.mark.parametrize("cin,cout", SHAPES)
def test_pool_fused_both_folds_equal_gemm_then_segment_max(ops, lp, cin, cout, m, pattern, values):
    d = pool_case(lp, cin, cout, m, pattern, values)
    bf = LP()
    if pattern == "mixed":
        assert d["n"] % 16 != 0
    for fold in (ops.POOL_FOLD_WALK, ops.POOL_FOLD_SCAN, ops.POOL_FOLD_AUTO):
        xi, xband = GB.poisoned_input(d["x"], rows=64, name="x")
        out, band = GB.banded((m, cout), torch.float32, rows=64, fill=-7.0, name="out")
        out2, band2 = GB.banded((m, cout), bf, rows=64, fill=-7.0, name="out2")
        assert xi.stride(0) != cin and out.stride(0) != cout and out2.stride(0) != cout
        seg, seg_check = GB.guard_index(d["seg"], rows=64)
        with ops.pool_fused_fold(fold), ops.record_routes() as rr:
            ops.pool_fused(xi, d["img"], d["b"], seg, m, d["sc"], d["sh"], ops.ACT_GELU, out, out2)
        band.check(), band2.check(), seg_check()
        # the launch record: the fold taken - under AUTO the scan from a mean run of POOL_SCAN_RATIO children on
        took = auto_fold(ops, d["n"], m) if fold == ops.POOL_FOLD_AUTO else fold
        name = f"pool_fused_kernel<{cin},{cout},{'scan' if took == ops.POOL_FOLD_SCAN else 'walk'}>"
        assert rr.count == 1 and rr.kernels() == [name], (fold, rr.routes)
        assert (rr.routes[0].fix, rr.routes[0].aux, rr.routes[0].bn) == (took, fold, cout), rr.routes
        bad, bad2 = int((GB.bits(out) != GB.bits(d["ref"])).sum()), int((GB.bits(out2) != GB.bits(d["ref2"])).sum())
        report(f"pool fused fold={fold} {cin}->{cout} m={m} {pattern} {values} {lp}", n=d["n"], fp32_mismatches=bad, lp_mismatches=bad2)
        assert bad == 0 and bad2 == 0, (fold, bad, bad2)


def test_pool_fused_fold_hook_restores_and_rejects(ops):
    lib = ops._lib.load()
    with ops.pool_fused_fold(ops.POOL_FOLD_SCAN):
        with ops.pool_fused_fold(ops.POOL_FOLD_WALK):
            assert lib.cdseg_pool_fused_fold(ops.POOL_FOLD_WALK) == ops.POOL_FOLD_WALK
        assert lib.cdseg_pool_fused_fold(ops.POOL_FOLD_SCAN) == ops.POOL_FOLD_SCAN
    assert lib.cdseg_pool_fused_fold(0) == 0
    assert lib.cdseg_pool_fused_fold(3) < 0 and lib.cdseg_pool_fused_fold(-1) < 0 and lib.cdseg_pool_fused_fold(0) == 0


# ============================================================================================ one-launch unpooling
# ops.unpool_fused (csrc/pool.hip, cdseg_unpool_fused) against the two ops.gemm launches it replaces - the child projection
# into an fp32 buffer, then the skip projection with add_src / add_idx / out2_pre_add=True - x (fp32) and xc (16-bit) BIT FOR
# BIT, both shapes, both builds; fine rows n = 1, 17, 100, 1000 cut into the run patterns of the pooling tests (`cluster` is
# derived from `seg`); every operand in guard bands with non-contiguous row strides.
UNPOOL_SHAPES = [(32, 64, 64), (64, 128, 64)]


def make_unpool_runs(pattern, n, g):
    """Runs of the pattern that cover exactly n fine rows (the last one cut short)."""
    if pattern == "ones":
        return torch.ones(n, dtype=torch.int64)
    runs = make_runs(pattern, n, g)  # n runs hold at least n rows
    if pattern == "mixed":
        runs[min(1, n - 1)] = 37  # (make_runs puts it in the middle of n runs: behind the cut)
    ends = runs.cumsum(0)
    m = int((ends < n).sum()) + 1
    runs = runs[:m].clone()
    runs[-1] -= int(ends[m - 1]) - n
    assert int(runs.sum()) == n and int(runs.min()) >= 1
    return runs


@functools.lru_cache(maxsize=None)
def unpool_case(lp, ks, kp, c, n, pattern):
    from cdsegnet_amd import ops as O
    bf = LP()
    g = torch.Generator().manual_seed(100 * ks + 7 * n + PATTERNS.index(pattern))
    runs = make_unpool_runs(pattern, n, g)
    m = len(runs)
    seg = torch.cat([torch.zeros(1, dtype=torch.int64), runs.cumsum(0)]).int()
    cluster = torch.repeat_interleave(torch.arange(m), runs).int()
    par = lambda: (torch.randn(c, generator=g) * 0.3, torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.2)
    d = dict(n=n, m=m, seg=dev(seg), xs=dev(torch.randn(n, ks, generator=g), bf), xp=dev(torch.randn(m, kp, generator=g), bf),
             ws=dev(torch.randn(c, ks, generator=g) / ks ** 0.5, bf), wp=dev(torch.randn(c, kp, generator=g) / kp ** 0.5, bf),
             ps=[dev(t) for t in par()], pp=[dev(t) for t in par()])
    d["ps"][1][::5] *= -1.0
    child = torch.empty(m, c, device="cuda")
    O.gemm(d["xp"], d["wp"], child, bias=d["pp"][0], scale=d["pp"][1], shift=d["pp"][2], act=O.ACT_GELU)
    d["ref"], d["ref2"] = torch.empty(n, c, device="cuda"), torch.empty(n, c, dtype=bf, device="cuda")
    O.gemm(d["xs"], d["ws"], d["ref"], bias=d["ps"][0], scale=d["ps"][1], shift=d["ps"][2], act=O.ACT_GELU, add_src=child,
           add_idx=dev(cluster), out2=d["ref2"], out2_pre_add=True)
    d["img_s"], d["img_p"] = O.unpool_fused_pack(d["ws"]), O.unpool_fused_pack(d["wp"])
    torch.cuda.synchronize()
    return d


@LPS
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", [1, 17, 100, 1000])
@pytest.mark.parametrize("ks,kp,c", UNPOOL_SHAPES)
def test_unpool_fused_equals_the_two_gemm_launches(ops, lp, ks, kp, c, n, pattern):
    d = unpool_case(lp, ks, kp, c, n, pattern)
    bf, m = LP(), d["m"]
    assert ops.unpool_fused_ok(ks, kp, c, bf, "cuda")
    xs, _ = GB.poisoned_input(d["xs"], rows=64, name="skip_x")
    xp, _ = GB.poisoned_input(d["xp"], rows=64, name="coarse_x")
    out, band = GB.banded((n, c), torch.float32, rows=64, fill=-7.0, name="x")
    out2, band2 = GB.banded((n, c), bf, rows=64, fill=-7.0, name="xc")
    assert xs.stride(0) != ks and xp.stride(0) != kp and out.stride(0) != c and out2.stride(0) != c
    seg, seg_check = GB.guard_index(d["seg"], rows=64)
    with ops.record_routes() as rr:
        ops.unpool_fused(xs, d["img_s"], *d["ps"], xp, d["img_p"], *d["pp"], seg, m, ops.ACT_GELU, out, out2)
    band.check(), band2.check(), seg_check()
    assert rr.count == 1 and rr.kernels() == [f"unpool_fused_kernel<{ks},{kp}>"], rr.routes
    bad, bad2 = int((GB.bits(out) != GB.bits(d["ref"])).sum()), int((GB.bits(out2) != GB.bits(d["ref2"])).sum())
    diff = float((out - d["ref"]).abs().max())
    report(f"unpool fused ({ks},{kp},{c}) n={n} m={m} {pattern} {lp}", fp32_mismatches=bad, lp_mismatches=bad2, max_diff=diff)
    assert bad == 0 and bad2 == 0, (bad, bad2, diff)


# ============================================================================================ end to end
def _count_calls(monkeypatch, ops, names):
    calls = {k: 0 for k in names}
    for k in names:
        real = getattr(ops, k)

        def counted(*a, _real=real, _k=k, **kw):
            calls[_k] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(ops, k, counted)
    return calls


@pytest.mark.parametrize("precision", ["bf16", "fp16+head"])
def test_mini_forward_of_two_collated_scenes_with_the_fused_levels_on_and_off(monkeypatch, precision):
    """The mini config on the two collated fixture scenes: logits with the one-launch level kernels allowed and with both
    predicates answering no (every pooling and unpooling on its two launches), bit for bit.  The mini widths (16 / 32 / 64)
    meet the kernels' shapes in one pooling only (32 -> 64, the walk; no unpooling): what this case holds is that the
    predicates leave a narrow model's forward alone.  The full-width case below runs the new kernels."""
    from cdsegnet_amd import ops as O
    from tests.helpers import fixture_cfg, fixture_draws, fixture_input, fixture_state_dict, load_fixture
    from tests.test_gpu_e2e import build, run
    fx = load_fixture("mini_e2e_batch2.npz")
    cfg, sd = fixture_cfg(fx), fixture_state_dict(fx)
    on = run(build(cfg, sd, precision), fixture_input(fx), fixture_draws(fx))
    monkeypatch.setattr(O, "pool_fused_ok", lambda *a: False)
    monkeypatch.setattr(O, "unpool_fused_ok", lambda *a: False)
    off = run(build(cfg, sd, precision), fixture_input(fx), fixture_draws(fx))
    assert on.shape == off.shape and (on.view("uint32") == off.view("uint32")).all()


@functools.lru_cache(maxsize=None)
def _full_width():
    from cdsegnet_amd import configs
    from cdsegnet_amd.param_init import fill_state_dict
    from cdsegnet_amd.registry import build_model
    cfg = configs.cdsegnet_config("scannet")
    return cfg, fill_state_dict(build_model(cfg).state_dict(), seed=2)


@pytest.mark.parametrize("precision", ["bf16", "fp16+head"])
def test_full_width_forward_takes_the_fused_levels_and_keeps_its_logits(monkeypatch, precision):
    """The mini config is too narrow for the kernels' shapes, so the same comparison at full width: two collated room scenes
    of 3000 points, every pooling of a kernel shape on the scan fold (forced for this forward: at 6000 points the library's
    own choice is not pinned) and both unpool shapes taken (counted), logits bit-equal to the forward on the two-launch paths."""
    import cdsegnet_amd.models  # noqa: F401
    from cdsegnet_amd import _lib, synth
    from cdsegnet_amd import ops as O
    from oracle import model as OM
    from tests.test_gpu_e2e import build, run
    cfg, sd = _full_width()
    both = synth.collate([synth.room_scene(5, 3000), synth.room_scene(6, 3000)])
    inp = {k: both[k] for k in ("coord", "grid_coord", "feat", "offset")}
    draws = OM.draw_rng(1, len(inp["coord"]), cfg["c_in_channels"])
    calls = _count_calls(monkeypatch, O, ["pool_fused", "unpool_fused"])
    # (the engine sends a long-run pooling to the one-launch kernel from 960 k fine rows on, the sizes it was measured at: the
    # limit is lifted for this forward of 6000 points)
    import cdsegnet_amd.engine as E
    monkeypatch.setattr(E, "POOL_LONG_MIN_ROWS", 0)
    with _lib.use("f16" if precision.startswith("fp16") else "bf16"), O.pool_fused_fold(O.POOL_FOLD_SCAN):
        on = run(build(cfg, sd, precision), inp, draws)
    taken = dict(calls)
    assert taken["unpool_fused"] >= 2 and taken["pool_fused"] >= 3, taken  # (n-decoder stages 0 and 1; n- and c-branch poolings)
    monkeypatch.setattr(O, "pool_fused_ok", lambda *a: False)
    monkeypatch.setattr(O, "unpool_fused_ok", lambda *a: False)
    off = run(build(cfg, sd, precision), inp, draws)
    assert calls == taken, (calls, taken)
    assert on.shape == off.shape and (on.view("uint32") == off.view("uint32")).all()
