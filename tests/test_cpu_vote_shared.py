"""CPU: test-time voting on shared geometry - the premise on the reference's recorded output, and the host logic of
Engine.shared_plan / predraw_fragments / Level.slots on curve tuples / TestPipeline.vote(share_plan, fragment_draws) on the
emulated op layer (tests/emu_select_ops.py).  The kernels and the streams are tested on the GPU (tests/test_gpu_vote_shared.py)."""
import copy

import numpy as np
import pytest
import torch

from cdsegnet_amd import testtime as tt
from cdsegnet_amd._lib import CdsegError
from tests import testtime_restatement as R
from tests import vote_shared_common as C
from tests.helpers import load_fixture


# ------------------------------------------------------------------------------------------------ premise
def test_premise_every_fragment_of_a_nuscenes_list_has_the_same_grid_rows():
    """The reference's recorded fragments (tests/golden/testtime_nuscenes.npz): aug_grid[frag_index[f]] is the same array for
    every fragment f of a list - one point per voxel, the same voxels, the same row order."""
    fx = load_fixture("testtime_nuscenes.npz")
    assert int(fx["num_aug"]) == 10
    for a in range(10):
        grid, index = fx[f"aug{a}_grid"], fx[f"aug{a}_frag_index"]
        assert 5 <= len(index) <= 7 and 1321 <= index.shape[1] <= 1429
        first = grid[index[0]]
        assert len(np.unique(first, axis=0)) == len(first)
        for f in range(1, len(index)):
            assert np.array_equal(grid[index[f]], first), (a, f)
            assert not np.array_equal(index[f], index[0])  # different points all the same


def test_premise_holds_for_the_scannet_block_through_the_restatement():
    fx = load_fixture("tta_pipeline.npz")
    cfg = copy.deepcopy(C.blocks()["scannet"])
    cfg["test_cfg"]["voxelize"]["grid_size"] = float(fx["grid_size"])
    out = R.pipeline(cfg, dict(coord=fx["coord"], color=fx["color"], normal=fx["normal"]))
    assert len(out["augs"]) == 13 and max(len(g["index"]) for g in out["augs"]) >= 2
    for a, g in enumerate(out["augs"]):
        for f in range(1, len(g["index"])):
            assert np.array_equal(g["frag_grid"][f], g["frag_grid"][0]), (a, f)


# ------------------------------------------------------------------------------------------------ emulated op layer
@pytest.fixture()
def emu(monkeypatch):
    """The mini LiDAR model in fp32 and a two-list scene (6 and 5 fragments of 1321 / 1429 rows) on the emulated ops."""
    from cdsegnet_amd import engine as engine_mod
    from tests import emu_select_ops
    from tests.test_cpu_testpipeline import EmulatedOps
    monkeypatch.setattr(engine_mod, "ops", emu_select_ops)
    monkeypatch.setattr(tt, "ops", EmulatedOps())
    fx = load_fixture("testtime_nuscenes.npz")
    model, mcfg, sd = C.mini_model()
    tp = tt.TestPipeline(C.block_cut((0, 9)))
    raw = dict(coord=torch.as_tensor(fx["coord"]), strength=torch.as_tensor(fx["strength"]), segment=torch.as_tensor(fx["segment"]))
    scene = tp.prepare(raw, draws={"1.r": fx["1.r"]})
    assert [g["num_fragments"] for g in scene.augs] == [6, 5]
    return dict(model=model, cfg=mcfg, sd=sd, tp=tp, scene=scene, k=mcfg["num_classes"], engine_mod=engine_mod)


def _vote(e, seed=3, **kw):
    eng = e["model"].engine()
    torch.manual_seed(seed)
    before = eng.plans_built
    _, pred = e["tp"].vote(e["model"], e["scene"], e["k"], **kw)
    return pred, eng.plans_built - before, torch.get_rng_state()


def test_share_plan_builds_one_plan_per_augmentation_and_votes_the_same_bits(emu):
    assert emu["model"].engine().plans_built == 0
    base, n_default, _ = _vote(emu)
    assert n_default == 11  # one plan per forward
    pred, n_shared, _ = _vote(emu, share_plan=True)
    assert n_shared == 2  # one per augmentation
    assert torch.equal(pred, base)
    base3, n_default3, _ = _vote(emu, fragment_batch=3)
    assert n_default3 == 4  # groups (3, 3) and (3, 2): one plan per forward
    pred3, n_shared3, _ = _vote(emu, fragment_batch=3, share_plan=True)
    assert n_shared3 == 3 and n_shared3 <= 2 * 2  # (aug 0, 3), (aug 1, 3), (aug 1, 2)
    assert torch.equal(pred3, base3)


def test_vote_arguments_are_checked(emu):
    tp, model, scene, k = emu["tp"], emu["model"], emu["scene"], emu["k"]
    with pytest.raises(ValueError, match="fragment_draws"):
        tp.vote(model, scene, k, fragment_draws="scene")
    with pytest.raises(ValueError, match="share_plan=True"):
        tp.vote(model, scene, k, fragment_batch=3, fragment_draws="fragment")
    scene.augs[1]["shared_geometry"] = False
    with pytest.raises(ValueError, match="augmentation 1"):
        tp.vote(model, scene, k, share_plan=True)


@pytest.mark.parametrize("noise_source", ["torch_cpu", "device"])
def test_fragment_draws_leave_the_generator_where_single_forwards_leave_it(emu, noise_source):
    """predraw_fragments on a batch of k = 3 fragments = 3 predraw calls in fragment order: the same values, the same
    generator state afterwards; with a jitter (noise_level) and with device noise (the stream ids are generator draws)."""
    model, scene = emu["model"], emu["scene"]
    model.noise_source = noise_source
    eng = model.engine()
    d3 = scene.collated(0, 3, 3)
    m = scene.augs[0]["num_voxels"]
    for noise_level in (None, 0.1):
        torch.manual_seed(7)
        singles = [eng.predraw(scene.fragments[3 + j], noise_level) for j in range(3)]
        state = torch.get_rng_state()
        torch.manual_seed(7)
        got = eng.predraw_fragments(d3, noise_level)
        assert torch.equal(torch.get_rng_state(), state)
        # device noise: the stream ids are generator draws; else a counter per engine, which goes on counting
        shift = 0 if noise_source == "device" else got["rng_base"] - singles[0]["rng_base"]
        assert got["rng_bases"] == [s["rng_base"] + shift for s in singles] and got["rng_base"] == got["rng_bases"][0]
        assert len(set(got["rng_bases"])) == 3
        assert len(got["perms"]) == C.N_DRAWS
        for p in range(C.N_DRAWS):
            assert [list(x) for x in got["perms"][p]] == [list(s["perms"][p]) for s in singles]
        for key in ("noise",) + (("feat_noise",) if noise_level is not None else ()):
            if noise_source == "device":
                assert got[key] is None and all(s[key] is None for s in singles)
            else:
                assert got[key].shape[0] == 3 * m and torch.equal(got[key], torch.cat([s[key] for s in singles], 0))
        assert ("feat_noise" in got) == (noise_level is not None)
    with pytest.raises(ValueError, match="share geometry"):
        eng.predraw_fragments({k: v for k, v in d3.items() if k != "shared_geometry"})


def test_reshuffle_curves_applies_each_elements_permutation_to_its_entry(emu):
    """A chain of shuffles (the initial one and three poolings) on a batch of 3 under per-element permutations against the
    three single chains, element by element; one permutation for the whole batch keeps today's form."""
    reshuffle = emu["engine_mod"].reshuffle_curves
    base = [0, 1, 2, 3]
    assert reshuffle(base, None, 3) is base
    assert reshuffle(base, [2, 0, 3, 1], 3) == [2, 0, 3, 1] and reshuffle(base, np.array([2, 0, 3, 1]), 3) == [2, 0, 3, 1]
    batched, singles = base, [base, base, base]
    for p in range(4):
        perms = [C.fragment_perms(f)[p] for f in range(3)]
        batched = reshuffle(batched, perms, 3)
        singles = [reshuffle(s, perm, 1) for s, perm in zip(singles, perms)]
        assert all(isinstance(c, tuple) and len(c) == 3 for c in batched)
        for b in range(3):
            assert [c[b] for c in batched] == singles[b], (p, b)
    # one permutation applied to per-element entries moves the tuples as a whole
    assert reshuffle(batched, [3, 2, 1, 0], 3) == batched[::-1]
    with pytest.raises(ValueError, match="permutations for a batch"):
        reshuffle(base, perms[:2], 3)


def test_a_batch_under_per_fragment_draws_reads_each_fragments_curves_and_computes_its_forward(emu, monkeypatch):
    """One collated forward of fragments 3..5 under group_draws against the three single forwards under fragment_draws: every
    slot-plan request of the batch names, element by element, the curve the single forward asks for at the same place, and
    the fragment's slice of the logits equals the single forward's (the emulated ops compute both the same way)."""
    model, scene, eng_mod = emu["model"], emu["scene"], emu["engine_mod"]
    m, ch = scene.augs[0]["num_voxels"], emu["cfg"]["c_in_channels"]
    asked = []
    real = eng_mod.Level.slots

    depth = [0]

    def spy(self, curve, patch_size, enable_flash):
        if depth[0] == 0:  # (a request on a tuple asks for its sources in turn: those are not requests of the forward)
            asked.append((self.cum, curve, patch_size))
        depth[0] += 1
        try:
            return real(self, curve, patch_size, enable_flash)
        finally:
            depth[0] -= 1
    monkeypatch.setattr(eng_mod.Level, "slots", spy)
    d3 = scene.collated(0, 3, 3)
    plan = model.plan(d3)
    asked.clear()
    out = model.inference(dict(d3), eval=False, draws=C.group_draws(3, 3, m, ch), plan=plan)["seg_logits"]
    batched = list(asked)
    for j in range(3):
        asked.clear()
        single = model.inference(dict(scene.fragments[3 + j]), eval=False, draws=C.fragment_draws(3 + j, m, ch))["seg_logits"]
        assert len(asked) == len(batched)
        for (cum_b, cb, kb), (cum_s, cs, ks) in zip(batched, asked):
            assert cum_b == cum_s and kb == ks
            assert (cb[j] if isinstance(cb, tuple) else cb) == cs
        err = float((out[j * m:(j + 1) * m] - single).abs().max())
        assert err <= 1e-5, (j, err)
    assert sum(isinstance(c, tuple) and len(set(c)) > 1 for _, c, _ in batched) >= 8  # the batch really mixes curves
    # per-fragment draws on a batch that is not marked as sharing geometry
    with pytest.raises(ValueError, match="share geometry"):
        model.inference({k: v for k, v in d3.items() if k != "shared_geometry"}, eval=False, draws=C.group_draws(3, 3, m, ch))


@pytest.mark.parametrize("noise_source", ["torch_cpu", "device"])
def test_faithful_batches_vote_what_single_forwards_vote(emu, noise_source):
    """vote(fragment_batch=3, share_plan=True, fragment_draws="fragment") against fragment_batch=1 under the same seed: the
    same summed votes up to float rounding, the same generator state afterwards - which fragment_draws="batch" does not give."""
    emu["model"].noise_source = noise_source
    base, _, state = _vote(emu, share_plan=True)
    pred, _, state_f = _vote(emu, fragment_batch=3, share_plan=True, fragment_draws="fragment")
    assert torch.equal(state_f, state)
    assert float((pred - base).abs().max()) <= 1e-5
    other, _, state_b = _vote(emu, fragment_batch=3, share_plan=True)
    assert not torch.equal(state_b, state) and float((other - base).abs().max()) > 1e-3


def test_a_plan_of_another_geometry_is_refused(emu):
    model, scene = emu["model"], emu["scene"]
    frag = scene.fragments[0]
    plan = model.plan(frag)
    ok = model.inference(dict(frag), eval=False, draws=C.fragment_draws(0, frag["feat"].shape[0], 4), plan=plan)["seg_logits"]
    assert torch.isfinite(ok).all()
    with pytest.raises(CdsegError, match="points"):
        model.inference(dict(scene.fragments[-1]), eval=False, plan=plan)  # the other list: another row count
    n = frag["feat"].shape[0]
    with pytest.raises(CdsegError, match="offsets"):  # the same rows cut into two scenes
        model.inference(dict(frag, offset=torch.tensor([10, n]), offset_host=[10, n]), eval=False, plan=plan)
    # check mode: one row of the grid differs
    model.check_shared_geometry = True
    model.inference(dict(frag), eval=False, plan=plan)
    moved = dict(frag, grid_coord=frag["grid_coord"].clone())
    moved["grid_coord"][17, 1] += 1
    with pytest.raises(CdsegError, match="check_shared_geometry"):
        model.inference(moved, eval=False, plan=plan)
    model.check_shared_geometry = False
    model.inference(moved, eval=False, plan=plan)  # off by default: nothing is compared


def test_swapping_two_fragments_shuffles_is_visible_to_the_oracle(emu):
    """The faithful-batch GPU test can only catch a wrong curve if one moves the logits by more than its bound: the oracle's
    logits of fragment 3 under fragment 4's shuffles (same noise) differ from its own by more than the fp32 bound 1e-3."""
    from oracle import model as OM
    scene, mcfg, sd = emu["scene"], emu["cfg"], emu["sd"]
    d = scene.fragments[3]
    m = d["feat"].shape[0]
    inp = dict(coord=d["coord"].numpy(), grid_coord=d["grid_coord"].numpy(), feat=d["feat"].numpy(), offset=np.array([m]))
    own = C.fragment_draws(3, m, mcfg["c_in_channels"])
    swapped = dict(own, perms=C.fragment_perms(4))
    a = OM.inference(mcfg["backbone"], sd, inp, own, T=mcfg["T"])
    b = OM.inference(mcfg["backbone"], sd, inp, swapped, T=mcfg["T"])
    moved = float((a - b).abs().max())
    print(f"[measure] swapped shuffles move the oracle's logits by {moved:.3e}")
    assert moved > 1e-3
