"""GPU: the 16-bit attention kernel hands out no query tile behind a patch's last kept slot (csrc/attention.hip).

cdseg_pad_plan fills the tail of every scene's last patch with slots borrowed from the patch before: keys whose rows as
queries are dropped (widx = -1).  attn_bf16_kernel derives, per patch, the highest slot with widx >= 0 and neither claims nor
computes the query tiles behind it.  A query row's result depends on no other query, so the kept rows must come out
BIT-IDENTICAL to a launch in which nothing is dead: the same call with every borrowed slot writing to a scratch row appended
to `out` (every tile computed).  Checked on a real padded plan (ops.pad_plan; scenes with n mod K in {1, 31, 32, 33, 500,
K - 1}) for both block shapes (8 and 16 waves, asserted through the library's schedule table), unsliced, sliced and graded
launches, self and cross attention, both builds.  A launch whose slots are all dead leaves `out` untouched.

attn_f32_kernel and attn_x3_kernel (the parity mode) compute every tile as before; they are not under test here.
"""
import numpy as np
import pytest
import torch

from tests.test_gpu_attention_range import LPS, _schedule
from tests.test_gpu_ops import LP, _library_variant, dev, ops, report  # noqa: F401  (fixtures: lp="f16" -> the half build)

pytestmark = pytest.mark.gpu

K = 1024
REMAINDERS = (1, 31, 32, 33, 500, K - 1)
WHOLE = (1, 2, 1, 3, 1, 2)  # full patches in front of each scene's ragged remainder: 16 patches per set of six scenes
SENTINEL = 7.0


def _plan(ops, copies, rng):
    """The padded slot plan of `copies` x six scenes, by the library's planner: (gidx, widx, patch_start, n, n_pad)."""
    counts = [w * K + r for w, r in zip(WHOLE, REMAINDERS)] * copies
    pads = [(c + K - 1) // K * K for c in counts]
    offs = np.concatenate([[0], np.cumsum(counts)])
    offs_pad = np.concatenate([[0], np.cumsum(pads)])
    n, n_pad = int(offs[-1]), int(offs_pad[-1])
    order = np.concatenate([a + rng.permutation(b - a) for a, b in zip(offs[:-1], offs[1:])])  # a serialized order per scene
    gidx, widx = ops.pad_plan(dev(order, torch.int32), dev(offs, torch.int32), dev(offs_pad, torch.int32), K, n_pad)
    ps = dev(np.arange(0, n_pad + 1, K), torch.int32)
    return gidx, widx, ps, n, n_pad


CASES = [  # (name, copies of the six scenes, heads, cross, expected (16 waves, query slices per patch-head))
    ("16x16", 1, 16, False, (True, [1])),
    ("16x8", 1, 8, False, (True, [2])),
    ("16x8", 1, 8, True, (True, [2])),
    ("16x2", 1, 2, False, (False, [4])),
    ("48x8", 3, 8, False, (False, [1])),
    ("48x8", 3, 8, True, (False, [1])),
    ("400x2", 25, 2, False, (False, None)),  # graded: whole patch-heads, then tail zones of half and quarter slices
]


@LPS
@pytest.mark.parametrize("name,copies,H,cross,shape", CASES, ids=[f"{c[0]}{'-cross' if c[3] else ''}" for c in CASES])
def test_attention_kept_rows_do_not_depend_on_dead_query_tiles(ops, lp, name, copies, H, cross, shape):
    lpt = LP()
    rng = np.random.default_rng(copies * 100 + H + 7 * cross + 3 * (lpt == torch.float16))
    gidx, widx, ps, n, n_pad = _plan(ops, copies, rng)
    num_patches = n_pad // K
    nb, wide16, splits, _ = _schedule(num_patches, H, K)
    if shape[1] is None:
        assert not wide16 and len(splits) > 1, (nb, wide16, splits)
    else:
        assert (wide16, splits) == shape, (nb, wide16, splits)
    w = widx.cpu().numpy()
    dead = w < 0
    n_dead = int(dead.sum())
    # the planner's dead slots are the borrowed ones: K - r per scene, the tail of its last patch; every row is kept once
    assert n_dead == copies * sum(K - r for r in REMAINDERS) and n_dead == n_pad - n
    assert np.array_equal(np.sort(w[~dead]), np.arange(n))
    C = 16 * H
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    q, k, v = (torch.randn(n, C, generator=g).to(lpt).cuda() for _ in range(3))
    kv_gidx = gidx
    if cross:  # keys / values from other rows than the queries (another level's slot plan in the model)
        kv_gidx = dev(rng.permutation(n), torch.int32)[gidx.long()].contiguous()
    # nothing dead: the borrowed slots write to scratch rows behind the n rows of `out`
    w_all = w.copy()
    w_all[dead] = n + np.arange(n_dead)
    widx_all = dev(w_all, torch.int32)
    flags = ops.ATTN_Q_PRESCALED if H == 8 else 0
    out = torch.full((n, C), SENTINEL, dtype=lpt, device="cuda")
    out_all = torch.full((n + n_dead, C), SENTINEL, dtype=lpt, device="cuda")
    ops.attention(q, k, v, gidx, kv_gidx, widx, ps, H, K, 0.25, out, flags=flags)
    ops.attention(q, k, v, gidx, kv_gidx, widx_all, ps, H, K, 0.25, out_all, flags=flags)
    torch.cuda.synchronize()
    same = torch.equal(out.view(torch.int16), out_all[:n].view(torch.int16))
    finite = bool(torch.isfinite(out.float()).all())
    written = bool((out_all[n:].float() != SENTINEL).any(1).all())  # the reference launch did compute the dead queries
    report(f"attn dead queries {lp} {name} cross={int(cross)}", blocks=nb, waves=16 if wide16 else 8, splits=str(splits),
           dead_slots=n_dead, same=int(same), finite=int(finite))
    assert finite and written
    assert same


@LPS
@pytest.mark.parametrize("copies,H", [(1, 16), (1, 2), (3, 8)], ids=["16-wave", "8-wave-sliced", "8-wave"])
def test_attention_units_without_a_kept_query_leave_out_untouched(ops, lp, copies, H):
    """Every slot dead (widx = -1 throughout, a legal plan): every block finds no tile to compute, reaches its barrier and
    returns; `out` keeps its sentinel.  Then one scene's slots alone are kept: its rows are written, all others untouched."""
    lpt = LP()
    rng = np.random.default_rng(copies + H)
    gidx, widx, ps, n, n_pad = _plan(ops, copies, rng)
    C = 16 * H
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(n, C, generator=g).to(lpt).cuda() for _ in range(3))
    out = torch.full((n, C), SENTINEL, dtype=lpt, device="cuda")
    none = torch.full_like(widx, -1)
    ops.attention(q, k, v, gidx, gidx, none, ps, H, K, 0.25, out)
    torch.cuda.synchronize()
    assert bool((out.float() == SENTINEL).all())
    # the second scene only (rows K + 1 .. 3 K + 31): units of the other scenes have no kept query
    lo, hi = K + 1, 3 * K + 32
    w = widx.cpu().numpy()
    one = dev(np.where((w >= lo) & (w < hi), w, -1), torch.int32)
    ref = torch.full((n, C), SENTINEL, dtype=lpt, device="cuda")
    ops.attention(q, k, v, gidx, gidx, widx, ps, H, K, 0.25, ref)
    ops.attention(q, k, v, gidx, gidx, one, ps, H, K, 0.25, out)
    torch.cuda.synchronize()
    o = out.float()
    assert bool((o[:lo] == SENTINEL).all()) and bool((o[hi:] == SENTINEL).all())
    assert torch.equal(out[lo:hi].view(torch.int16), ref[lo:hi].view(torch.int16))
