"""GPU: the attention kernels at the edges of fp32's range, against an fp64 oracle that mirrors the kernels' roundings.

The 16-bit kernel runs its softmax unshifted (P = exp2(s'), csrc/attention.hip attn_bf16_kernel) and redoes a query tile with
the exact row max when a row's denominator leaves [1e-30, 1e30] or one of its outputs is not finite.  These tests build
scores that are EXACT in every kernel: head dim 16, every key has k[0] = 1 and small dyadic entries elsewhere, every query
q' = (M_row, small dyadic entries <= 0), so s'_j = M_row + delta_j with delta_j in about [-7.5, 0] and the shift of each row
is chosen per row.  Without the redo, overflow and underflow rows come out as inf / inf or 0 / 0: "finite and within the
tolerance of the oracle" proves that the redo ran.  Which block shape (8 or 16 waves) a launch gets is computed from the
library's own schedule table and asserted for every case.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import model as OM
from tests.test_gpu_ops import LP, _library_variant, dev, ops, report  # noqa: F401  (fixtures: lp="f16" -> the half build)

pytestmark = pytest.mark.gpu

LPS = pytest.mark.parametrize("lp", ["bf16", "f16"])
SCALE = 0.25
LOG2E = 1.4426950408889634
L30 = float(np.log2(1e30))  # the redo thresholds are den = 1e30 and den = 1e-30: log2 = +-99.66
OVER, UNDER = (130.0, 300.0, 2000.0), (-110.0, -200.0, -2000.0)
# threshold rows: (target log2 den, which side of the threshold it has to land on)
THRESH = ((L30, "in"), (L30, "out"), (-L30, "in"), (-L30, "out"))
# query-tile classes, dealt round-robin over a patch's 32-query tiles
PATTERN = ("over", "ord", "under", "mixed", "ord", "thr", "under", "ord", "thr", "over", "mixed", "ord")
RAGGED = (1, 31, 32, 33, 63, 65)


def _c32(scale=SCALE):
    """The library's softmax factor: fp32(scale) * fp32(log2 e), rounded to fp32 (cdseg_attention_ex)."""
    return float(np.float32(np.float32(scale) * np.float32(LOG2E)))


def _r16(x, lp):
    """Values of the 16-bit type `lp` (round to nearest even; the half build saturates at +-65504), as float64."""
    t = torch.as_tensor(np.asarray(x, dtype=np.float64)).float()
    if lp == torch.float16:
        t = t.clamp(-65504.0, 65504.0)
    return t.to(lp).double().numpy()


def _schedule(num_patches, H, max_len):
    """(blocks, wide16, splits of the live rows) of the 16-bit kernel's launch, from the library's schedule table
    (cdseg_attention_schedule) and the 16-wave predicate of cdseg_attention_ex: at most 256 blocks, one zone, and at least
    16 query tiles per block."""
    from cdsegnet_amd import _lib
    lib = _lib.load()
    nb = lib.cdseg_attention_schedule(num_patches, H, max_len, _lib.BF16, None, 0)
    assert nb > 0
    tab = np.zeros((nb, 4), dtype=np.int32)
    lib.cdseg_attention_schedule(num_patches, H, max_len, _lib.BF16, tab.ctypes.data_as(ctypes.c_void_p), nb)
    live = tab[tab[:, 0] >= 0]
    splits = sorted(set(live[:, 3].tolist()))
    wide16 = nb <= 256 and len(splits) == 1 and ((max_len + 31) // 32) // splits[0] >= 16
    return nb, wide16, splits, tab


# ------------------------------------------------------------------ slot plans and inputs
class Launch:
    """A launch's slot plan: per patch the query row, key / value row and output row (-1: padding duplicate) of each slot."""

    def __init__(self, patches):
        self.patches = patches
        self.ps = np.concatenate([[0], np.cumsum([len(p[0]) for p in patches])]).astype(np.int32)
        self.gq = np.concatenate([p[0] for p in patches]).astype(np.int32)
        self.gkv = np.concatenate([p[1] for p in patches]).astype(np.int32)
        self.widx = np.concatenate([p[2] for p in patches]).astype(np.int32)
        self.max_len = int(np.diff(self.ps).max())

    def device(self):
        return dev(self.gq), dev(self.gkv), dev(self.widx), dev(self.ps)


def _make_patches(lens, row0, rng, dup_last=0, cross=False, kv_rows=None):
    """Patches of the given lengths over the fresh rows row0, row0 + 1, .. (shuffled: a serialized order).  The last patch's
    last `dup_last` slots repeat rows of its other slots and write nothing (the padding of a ragged last patch).
    cross: keys / values come from other rows than the queries (kv_rows: a permutation of all rows)."""
    patches, r = [], row0
    for i, L in enumerate(lens):
        d = dup_last if i == len(lens) - 1 else 0
        own = rng.permutation(np.arange(r, r + L - d))
        r += L - d
        gq = np.concatenate([own, rng.choice(own, d)]) if d else own
        widx = np.concatenate([own, np.full(d, -1)]) if d else own.copy()
        gkv = kv_rows[gq] if cross else gq.copy()
        patches.append((gq, gkv, widx))
    return patches, r


def _base_rows(n, H, rng):
    """q' and k of n rows: k[0] = 1, q'[0] = 0 (the row shift M goes there), small dyadic entries elsewhere (exact in
    bfloat16 and in half; delta = q'[1:] . k[1:] in [-7.5, 0])."""
    qp = np.zeros((n, 16 * H))
    k = np.zeros((n, 16 * H))
    for h in range(H):
        k[:, 16 * h] = 1.0
        k[:, 16 * h + 1:16 * h + 16] = rng.integers(0, 5, (n, 15)) / 4.0
        qp[:, 16 * h + 1:16 * h + 16] = -rng.integers(0, 3, (n, 15)) / 4.0
    v = rng.standard_normal((n, 16 * H))
    return qp, k, v


def _assign_shifts(launch, qp, k, H, lp, classes=PATTERN, last_tail_under=True):
    """Writes each query row's shift M into q'[:, 16 h] by the class of its 32-query tile; returns {class: live slots}.
    Threshold rows get the M of the 16-bit grid that puts log2(den) just inside / just outside +-log2(1e30).  A patch
    whose length is not a multiple of 32 gets underflow rows in its last tile (its key tail must be masked in the redo's
    max pass)."""
    count = {c: 0 for c in ("ord", "over", "under", "thr", "mixed")}
    names = np.array(classes)
    for pi, (gq, gkv, widx) in enumerate(launch.patches):
        L = len(gq)
        s = np.arange(L)
        t = s // 32
        cls = names[(t + 5 * pi) % len(classes)]
        if last_tail_under and L % 32:
            cls[t == t[-1]] = "under"
        live = widx >= 0
        for c in count:
            count[c] += int((live & (cls == c)).sum())
        for h in range(H):
            M = np.zeros(L)
            sel = cls == "over"
            M[sel] = np.array(OVER)[(s[sel] + h) % 3]
            M[(cls == "mixed") & (s % 32 == 7)] = 300.0
            sel = cls == "under"
            M[sel] = np.array(UNDER)[(s[sel] + h) % 3]
            thr = np.nonzero(cls == "thr")[0]
            if len(thr):
                sl = slice(16 * h + 1, 16 * h + 16)
                dl = qp[gq[thr]][:, sl] @ k[gkv][:, sl].T
                t2 = dl.max(1) + np.log2(np.exp2(dl - dl.max(1, keepdims=True)).sum(1))  # log2 sum_j 2^delta_j
                for i, (si, tt) in enumerate(zip(thr, t2)):
                    target, side = THRESH[(si + h) % 4]
                    cand = np.unique(_r16(np.arange(target - tt - 2, target - tt + 2, 1 / 64), lp))
                    tot = cand + tt
                    margin = 0.08
                    if target > 0:
                        M[si] = cand[tot <= target - margin].max() if side == "in" else cand[tot >= target + margin].min()
                    else:
                        M[si] = cand[tot >= target + margin].min() if side == "in" else cand[tot <= target - margin].max()
            qp[gq[live], 16 * h] = M[live]
    return count


def _oracle(qp, k, v, launch, H, patch_ids=None):
    """fp64 attention on the launch's slot plan for the listed patches: s' = q' . k (exp2 units), exp2(s' - max), weighted
    sum.  Returns out (rows x C, NaN where not computed) and log2(den) per (row, head)."""
    n, C = qp.shape
    out = np.full((n, C), np.nan)
    l2d = np.full((n, H), np.nan)
    for pi in (range(len(launch.patches)) if patch_ids is None else patch_ids):
        gq, gkv, widx = launch.patches[pi]
        live = widx >= 0
        for h in range(H):
            sl = slice(16 * h, 16 * h + 16)
            S = qp[gq][:, sl] @ k[gkv][:, sl].T
            m = S.max(1, keepdims=True)
            P = np.exp2(S - m)
            den = P.sum(1)
            out[widx[live], sl] = ((P @ v[gkv][:, sl]) / den[:, None])[live]
            l2d[widx[live], h] = (m[:, 0] + np.log2(den))[live]
    return out, l2d


def _operands(qp, k, v, lp, flags, scale=SCALE):
    """Device q / k / v of the 16-bit kernel for the given producer flags, and the q' / v the kernel computes with:
    q' = round16(fp32(q) * fp32(scale log2 e)) (attention.hip, the one rounding of Q'; ATTN_Q_PRESCALED: q' is q itself);
    v rounded to bfloat16 where the kernel does (the half build, unless the producer passed v as bfloat16)."""
    from cdsegnet_amd import ops as O
    if flags & O.ATTN_Q_PRESCALED:
        q16 = _r16(qp, lp)
        q_eff = q16
    else:
        c = _c32(scale)
        q16 = _r16(qp / c, lp)
        q_eff = _r16((torch.as_tensor(q16).float() * c).double().numpy(), lp)  # fp32 product, then the 16-bit rounding
    k16 = _r16(k, lp)
    if flags & O.ATTN_V_BF16:
        v_eff = _r16(v, torch.bfloat16)
        vt = torch.as_tensor(v).float().to(torch.bfloat16)
        v_dev = vt.view(torch.int16).view(lp) if lp == torch.float16 else vt
    else:
        v16 = _r16(v, lp)
        v_eff = _r16(v16, torch.bfloat16) if lp == torch.float16 else v16
        v_dev = torch.as_tensor(v16).to(lp)
    q_dev = torch.as_tensor(q16).to(lp)
    k_dev = torch.as_tensor(k16).to(lp)
    return q_dev.cuda(), k_dev.cuda(), v_dev.cuda(), q_eff, k16, v_eff


def _run16(launch, q_dev, k_dev, v_dev, H, flags, store8=False, scale=SCALE):
    from cdsegnet_amd import ops as O
    n, C = q_dev.shape
    gq, gkv, widx, ps = launch.device()
    if store8:  # rows of C + 4 elements: 8- but not 16-byte aligned (the ATTN_STORE8 epilogue)
        wide = torch.full((n, C + 4), float("nan"), dtype=q_dev.dtype, device="cuda")
        out = wide[:, :C]
    else:
        out = torch.full((n, C), float("nan"), dtype=q_dev.dtype, device="cuda")
    with O.record_routes() as rr:  # which kernel cdseg_attention_ex picked (include/cdseg.h cdseg_route_*)
        O.attention(q_dev, k_dev, v_dev, gq, gkv, widx, ps, H, launch.max_len, scale, out, flags=flags)
    torch.cuda.synchronize()
    out.routes = rr.routes  # the launch record of this call rides on the tensor it produced
    return out


def _check_rows(got, ref, rows, tol):
    """max |got - ref| over `rows`, after asserting that those rows are finite; tol(mag) is the bound."""
    g, r = got[rows], ref[rows]
    assert np.isfinite(r).all()
    bad = ~np.isfinite(g)
    assert not bad.any(), f"{int(bad.any(1).sum())} of {len(rows)} rows not finite"
    err, mag = float(np.abs(g - r).max()), float(np.abs(r).max())
    assert err < tol(mag), (err, mag)
    return err, mag


def _sample(launch):
    """Patches checked against fp64 in the large launches: every ragged one, the first eight and every 12th."""
    ids = {i for i, p in enumerate(launch.patches) if len(p[0]) != 1024} | set(range(8)) | \
        set(range(0, len(launch.patches), 12))
    return sorted(ids)


def _ragged_lens(num_patches):
    return list(RAGGED) + [1024] * (num_patches - len(RAGGED))


# ------------------------------------------------------------------ C: the 16-bit kernel, both block shapes
CASES16 = [  # (name, lengths, heads, flags, cross, 8-byte-aligned output rows, expected (wide16, split))
    ("3x2", [1024, 1024, 1024], 2, 0, False, False, (False, 4)),
    ("3x2", [1024, 65, 1024], 2, 1, True, True, (False, 4)),
    ("3x2", [1024, 33, 1024], 2, 3, False, False, (False, 4)),
    ("100x2", _ragged_lens(100), 2, 0, False, True, (True, 1)),
    ("100x2", _ragged_lens(100), 2, 1, False, False, (True, 1)),
    ("100x2", _ragged_lens(100), 2, 3, True, False, (True, 1)),
    ("56x2", _ragged_lens(56), 2, 1, False, False, (True, 2)),
    ("56x2", _ragged_lens(56), 2, 0, True, True, (True, 2)),
    ("56x2", _ragged_lens(56), 2, 3, False, False, (True, 2)),
    ("150x2", _ragged_lens(150), 2, 1, False, False, (False, 1)),
]


@LPS
@pytest.mark.parametrize("name,lens,H,flags,cross,store8,shape", CASES16,
                         ids=[f"{c[0]}-f{c[3]}{'-cross' if c[4] else ''}{'-st8' if c[5] else ''}" for c in CASES16])
def test_attention_16bit_redo_rows_vs_fp64(ops, lp, name, lens, H, flags, cross, store8, shape):
    """attn_bf16_kernel<8> and <16>, bfloat16 and half builds: overflow (M = 130, 300, 2000), all-underflow (M = -110,
    -200, -2000), threshold (log2 den just inside / outside +-log2 1e30), mixed (one overflow row in an otherwise ordinary
    tile) and ordinary rows on ragged patches (lengths 1 .. 65, a padded last patch), for the producer flags, the cross
    form and 8-byte-aligned output rows.  Tolerance of test_attention_bf16_vs_oracle: 0.02 (1 + |ref|max)."""
    lpt = LP()
    rng = np.random.default_rng(len(lens) * 100 + flags * 10 + cross + 2 * store8 + (lpt == torch.float16) * 7)
    launch_lens = list(lens)
    dup = 300 if name != "3x2" else 0  # large launches: the last patch is a padded one
    n = sum(launch_lens) - dup
    kv_rows = rng.permutation(n) if cross else None
    patches, _ = _make_patches(launch_lens, 0, rng, dup_last=dup, cross=cross, kv_rows=kv_rows)
    launch = Launch(patches)
    nb, wide16, splits, _ = _schedule(len(patches), H, launch.max_len)
    assert (wide16, splits) == (shape[0], [shape[1]]), (name, nb, wide16, splits)
    qp, k, v = _base_rows(n, H, rng)
    rows = _assign_shifts(launch, qp, k, H, lpt)
    q_dev, k_dev, v_dev, q_eff, k_eff, v_eff = _operands(qp, k, v, lpt, flags)
    out_dev = _run16(launch, q_dev, k_dev, v_dev, H, flags, store8=store8)
    # ... and the kernel the library recorded next to the predicate re-derived from its schedule table
    assert [(r.kernel, r.aux) for r in out_dev.routes] == [("attn_bf16_kernel<16>", 16) if wide16 else ("attn_bf16_kernel<narrow>", 8)], \
        (name, wide16, out_dev.routes)
    out = out_dev.float().cpu().numpy().astype(np.float64)
    ids = _sample(launch) if len(patches) > 8 else None
    ref, l2d = _oracle(q_eff, k_eff, v_eff, launch, H, ids)
    checked = np.nonzero(np.isfinite(ref[:, 0]))[0]
    err, mag = _check_rows(out, ref, checked, lambda m: 0.02 * (1 + m))
    live = l2d[checked]
    n_over, n_under = int((live > L30).sum()), int((live < -L30).sum())
    assert n_over > 0 and n_under > 0, "no redo rows among the checked patches"
    if flags & ops.ATTN_Q_PRESCALED:  # exact q': the threshold rows land on both sides of both thresholds
        near = live[np.abs(np.abs(live) - L30) < 0.7]
        assert ((near > L30).any() and (near < L30).any() and (near > -L30).any() and (near < -L30).any()), near
    # every live row of the launch was written, and nothing else is NaN
    assert np.isfinite(out).all(), "some rows were never written / non-finite"
    report(f"attn16 range {lp} {name} flags={flags} cross={int(cross)} st8={int(store8)}", max_err=err, ref_max=mag,
           waves=16 if wide16 else 8, split=splits[0], blocks=nb, rows_over=n_over, rows_under=n_under,
           patches_checked=len(ids) if ids else len(patches))


# ------------------------------------------------------------------ C: a graded launch, and schedule independence
@LPS
@pytest.mark.parametrize("redo", [False, True], ids=["ordinary", "redo"])
def test_attention_16bit_schedule_independence_and_graded_redo(ops, lp, redo):
    """attention.hip: "results do not depend on the schedule".  The same N = 3 patches (one of length 65) come out
    bit-identical (int16 view) whether they run as the first patches of a 16-wave launch (whole patch-heads), as an
    8-wave launch of just those patches (4 query slices each), or inside a graded launch whose tail zones slice them 2 or 4
    ways; with redo=True they hold overflow / underflow / threshold / mixed rows.  The 8-wave result is checked against
    fp64."""
    lpt = LP()
    H = 2
    rng = np.random.default_rng(11 + redo + 2 * (lpt == torch.float16))
    subj_lens = [1024, 65, 1024]
    n_s = sum(subj_lens)
    fill_n = 1024
    n = n_s + fill_n
    subj, _ = _make_patches(subj_lens, 0, rng)
    filler_rows = rng.permutation(np.arange(n_s, n))
    filler = (filler_rows, filler_rows.copy(), np.full(fill_n, -1))  # reads rows, writes nothing
    qp, k, v = _base_rows(n, H, rng)
    if redo:
        rows = _assign_shifts(Launch(subj), qp, k, H, lpt)
        assert all(rows.values()), rows
    flags = ops.ATTN_Q_PRESCALED
    q_dev, k_dev, v_dev, q_eff, k_eff, v_eff = _operands(qp, k, v, lpt, flags)
    subj_rows = np.concatenate([p[0] for p in subj])

    # 1: the first patches of a 16-wave launch (100 patches x 2 heads: whole patch-heads)
    l1 = Launch(subj + [filler] * 97)
    s1 = _schedule(len(l1.patches), H, l1.max_len)
    assert s1[1] and s1[2] == [1], s1[:3]
    # 2: an 8-wave launch of just those patches (4 slices per patch-head)
    l2 = Launch(subj)
    s2 = _schedule(len(l2.patches), H, l2.max_len)
    assert not s2[1] and s2[2] == [4], s2[:3]
    # 3: a graded launch (lead / tail zones) with the subject patches where its tail zones slice them
    P3 = 400
    nb3, w3, splits3, tab = _schedule(P3, H, 1024)
    assert not w3 and len(splits3) > 1, splits3
    live = tab[tab[:, 0] >= 0]
    psplit = {}
    for p_, h_, _, s_ in live.tolist():
        psplit[p_] = min(psplit.get(p_, 99), s_)
    in2 = [p_ for p_ in sorted(psplit) if psplit[p_] == 2]
    in4 = [p_ for p_ in sorted(psplit) if psplit[p_] == 4]
    assert in2 and in4
    pos = [in2[len(in2) // 2], in4[0], in4[len(in4) // 2]]
    pl3 = [filler] * P3
    for p_, sp in zip(pos, subj):
        pl3[p_] = sp
    l3 = Launch(pl3)

    o1 = _run16(l1, q_dev, k_dev, v_dev, H, flags)[subj_rows]
    o2 = _run16(l2, q_dev, k_dev, v_dev, H, flags)[subj_rows]
    o3 = _run16(l3, q_dev, k_dev, v_dev, H, flags)[subj_rows]
    ref, l2d = _oracle(q_eff, k_eff, v_eff, l2, H)
    err, mag = _check_rows(o2.float().cpu().numpy().astype(np.float64), ref[subj_rows], np.arange(n_s),
                           lambda m: 0.02 * (1 + m))
    same12 = torch.equal(o1.view(torch.int16), o2.view(torch.int16))
    same32 = torch.equal(o3.view(torch.int16), o2.view(torch.int16))
    report(f"attn16 schedule {lp} redo={int(redo)}", max_err=err, ref_max=mag, graded_blocks=nb3,
           graded_splits=str(splits3), rows_redo=int((np.abs(l2d[subj_rows]) > L30).any(1).sum()),
           same_16wave=int(same12), same_graded=int(same32))
    if redo:
        assert (np.abs(l2d[subj_rows]) > L30).any()
    assert same12 and same32


# ------------------------------------------------------------------ D: the fp32 kernels
FP32_LENS = [1024, 1, 31, 32, 33, 63, 65, 1024]


@pytest.mark.parametrize("x3_on", [False, True], ids=["f32", "fp32x3"])
@pytest.mark.parametrize("flags,cross", [(1, False), (1, True), (0, False)], ids=["prescaled", "prescaled-cross", "flags0"])
def test_attention_fp32_kernels_redo_rows_vs_fp64(ops, x3_on, flags, cross):
    """attn_f32_kernel (two-pass max) and attn_x3_kernel (unshifted pass + redo, |q'|, |k| <= 65504) on the same rows and
    ragged patches (the last one padded); tolerances of the existing tests: 2e-5 / 4e-5 (1 + |ref|max).  flags = 0: q is
    given unscaled (q' / c, exact in fp32) and the oracle computes with fp32(q) * c."""
    H = 2
    rng = np.random.default_rng(21 + flags + 2 * cross + 4 * x3_on)
    dup = 300
    n = sum(FP32_LENS) - dup
    kv_rows = rng.permutation(n) if cross else None
    patches, _ = _make_patches(FP32_LENS, 0, rng, dup_last=dup, cross=cross, kv_rows=kv_rows)
    launch = Launch(patches)
    qp, k, v = _base_rows(n, H, rng)
    _assign_shifts(launch, qp, k, H, torch.bfloat16)
    v = v.astype(np.float32).astype(np.float64)
    if flags & ops.ATTN_Q_PRESCALED:
        q_in = qp
        q_eff = qp
    else:
        c = _c32()
        q_in = (qp / c).astype(np.float32).astype(np.float64)
        q_eff = q_in * c
    prev = ops.set_f32x3(x3_on)
    try:
        gq, gkv, widx, ps = launch.device()
        out = torch.full((n, 16 * H), float("nan"), dtype=torch.float32, device="cuda")
        ops.attention(dev(q_in, torch.float32), dev(k, torch.float32), dev(v, torch.float32), gq, gkv, widx, ps, H,
                      launch.max_len, SCALE, out, flags=flags)
        torch.cuda.synchronize()
    finally:
        ops.set_f32x3(prev)
    got = out.cpu().numpy().astype(np.float64)
    ref, l2d = _oracle(q_eff, k, v, launch, H)
    tol = 4e-5 if x3_on else 2e-5
    err, mag = _check_rows(got, ref, np.arange(n), lambda m: tol * (1 + m))
    assert (l2d > L30).any() and (l2d < -L30).any()
    report(f"attn {'fp32x3' if x3_on else 'f32'} range flags={flags} cross={int(cross)}", max_err=err, ref_max=mag)


@pytest.mark.parametrize("lens", [[1, 17, 1024, 45], [1024, 100, 1024, 33]], ids=["L1-17-1024-45", "L1024-100-1024-33"])
def test_attention_bwd_redo_rows_vs_fp64_autograd(ops, lens):
    """ops.attention_bwd (fp32) on overflow, underflow, threshold and mixed rows of ragged patches (L % 16 != 0, a padded
    last patch): dq / dk / dv against fp64 autograd of the same attention (oracle/model.py's patch attention in float64)."""
    H = 2
    rng = np.random.default_rng(sum(lens))
    dup = 24
    n = sum(lens) - dup
    patches, _ = _make_patches(lens, 0, rng, dup_last=dup)
    launch = Launch(patches)
    qp, k, v = _base_rows(n, H, rng)
    rows = _assign_shifts(launch, qp, k, H, torch.bfloat16)
    assert rows["over"] and rows["under"] and rows["mixed"] and rows["thr"], rows
    c = _c32()
    q = (qp / c).astype(np.float32).astype(np.float64)
    v = v.astype(np.float32).astype(np.float64)
    dout = rng.standard_normal((n, 16 * H)).astype(np.float32).astype(np.float64)
    # fp64 autograd of the oracle's attention on the slot plan
    qt, kt, vt = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (q, k, v))
    gq, gkv, widx = (torch.from_numpy(a.astype(np.int64)) for a in (launch.gq, launch.gkv, launch.widx))
    o = OM._patch_attention(qt[gq], kt[gkv], vt[gkv], launch.ps.astype(np.int64), H, SCALE)
    m = widx >= 0
    (o[m] * torch.from_numpy(dout)[widx[m]]).sum().backward()
    dq = torch.zeros(n, 16 * H, dtype=torch.float32, device="cuda")
    dk, dv = torch.zeros_like(dq), torch.zeros_like(dq)
    dgq, dgkv, dwidx, dps = launch.device()
    ops.attention_bwd(dev(q, torch.float32), dev(k, torch.float32), dev(v, torch.float32), dgq, dgkv, dwidx, dps,
                      launch.ps.tolist(), H, SCALE, dev(dout, torch.float32), dq, dk, dv)
    torch.cuda.synchronize()
    # fp32 scores carry an absolute error of about 2^-24 |s'| (exp2 units): a relative error of that order in every P at
    # |s'| = 2000 - hence the score-dependent part of the bound
    tol = 1e-4 + 4 * 2.0 ** -24 * float(np.abs(qp[:, ::16]).max())
    errs = {}
    for name, got, ref in (("dq", dq, qt.grad), ("dk", dk, kt.grad), ("dv", dv, vt.grad)):
        g, r = got.cpu().double(), ref
        assert torch.isfinite(g).all(), name
        err, mag = (g - r).abs().max().item(), r.abs().max().item()
        errs[name] = err
        assert err < tol * (1 + mag), (name, err, mag)
    report(f"attn bwd range lens={lens}", tol=tol, **errs)


# ------------------------------------------------------------------ E: large V on rows that are not redone
@pytest.mark.parametrize("lp,kernel", [("bf16", "bf16"), ("f16", "f16-vbf16"), ("bf16", "fp32x3")],
                         ids=["bf16", "f16-vbf16", "fp32x3"])
def test_attention_large_v_on_rows_below_the_redo_threshold(ops, lp, kernel):
    """|v| ~ 1e10 on rows whose denominator sits just below 1e30 (log2 den in (98, 99], no redo by the denominator): the
    unshifted numerator sum_j 2^s'_j v_j exceeds FLT_MAX although the exact output is about v.  The kernels redo a tile
    whose outputs are not finite (attention.hip); the half build's output saturates at +-65504 like every half store."""
    H = 2
    lpt = LP()
    rng = np.random.default_rng(5)
    lens = [1024, 1024, 65]
    n = sum(lens)
    patches, _ = _make_patches(lens, 0, rng)
    launch = Launch(patches)
    qp, k, v = _base_rows(n, H, rng)
    # every row: log2 den in (98, 99] (below log2 1e30 = 99.66)
    for gq, gkv, widx in launch.patches:
        for h in range(H):
            sl = slice(16 * h, 16 * h + 16)
            dl = qp[gq][:, sl] @ k[gkv][:, sl].T
            t2 = dl.max(1) + np.log2(np.exp2(dl - dl.max(1, keepdims=True)).sum(1))
            qp[gq, 16 * h] = _r16(np.floor(99.0 - t2), lpt)
    # mostly positive, so that the weighted sums are large (about 1e10 x den)
    v = np.where(rng.random(v.shape) < 0.2, -1e10, 1e10) * (1 + rng.integers(0, 8, v.shape) / 8)
    if kernel == "fp32x3":
        prev = ops.set_f32x3(True)
        try:
            gq, gkv, widx, ps = launch.device()
            out = torch.full((n, 16 * H), float("nan"), dtype=torch.float32, device="cuda")
            ops.attention(dev(qp, torch.float32), dev(k, torch.float32), dev(v, torch.float32), gq, gkv, widx, ps, H,
                          launch.max_len, SCALE, out, flags=ops.ATTN_Q_PRESCALED)
            torch.cuda.synchronize()
        finally:
            ops.set_f32x3(prev)
        q_eff, k_eff, v_eff, tol = qp, k, v, 4e-5
    else:
        flags = ops.ATTN_Q_PRESCALED | (ops.ATTN_V_BF16 if lpt == torch.float16 else 0)
        q_dev, k_dev, v_dev, q_eff, k_eff, v_eff = _operands(qp, k, v, lpt, flags)
        out = _run16(launch, q_dev, k_dev, v_dev, H, flags)
        tol = 0.02
    got = out.float().cpu().numpy().astype(np.float64)
    ref, l2d = _oracle(q_eff, k_eff, v_eff, launch, H)
    assert (l2d > 97.9).all() and (l2d < L30 - 0.5).all(), (l2d.min(), l2d.max())
    assert np.isfinite(ref).all() and np.abs(ref).max() > 1e9
    if kernel == "f16-vbf16":
        ref = np.clip(ref, -65504.0, 65504.0)
    err, mag = _check_rows(got, ref, np.arange(n), lambda m: tol * (1 + m))
    report(f"attn large v {kernel}", max_err=err, ref_max=mag, log2den_max=float(l2d.max()))
