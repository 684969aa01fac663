#!/usr/bin/env python3
"""Record the reference's training step on a Mix3D batch: tests/golden/train_step_mix3d.npz.

Run from the repo root:  python tools/make_mix3d_golden.py   (needs the reference checkout, like oracle/make_golden.py)

The recording is oracle/make_golden.py's `gen_train_step` (mini model, MSE + CrossEntropy + Lovasz under GLS, every draw in
consumption order: timesteps, noise, order shuffles, DropPath masks per module; loss and parts, both predictions and their
gradients, the norm of every parameter gradient, the same eight gradients in full, the first AdamW step) on another batch: rooms a (900 points)
and b (700 points) merged into batch element 0 as `point_collate_fn` does with `mix_prob` (both grids start at 0, so voxels
hold a point of each; element 0 spans two 1024-slot patches), room c (500 points) on its own.  40 points of room a are added
once more, jittered inside their voxel, so that some voxels hold three points.

The reference runs with the stand-ins of oracle/refshim: its spconv resolves every tap of a sparse conv, the centre tap
included, to the FIRST row of the addressed voxel - the convention of `model.train_mix3d = "rows"` ("parity
unpinned").  What the tool asserts before it writes anything:
  * a and b share at least 3 % of element 0's rows' voxels, and at least one voxel holds three rows;
  * some shared voxel's first row (caller's order) is not room a's own row of that voxel: the jittered copies stand IN FRONT
    of room a in the caller's order, so "first in the caller's order" is visible in the data;
  * the reference's recorded level-0 orders break ties by ascending caller index (the rule of engine.RowLevel).

Stable sorts while recording.  torch.sort / torch.argsort are not stable by contract, and on the torch build this fixture
was made with they are not stable in fact: left alone, the reference's level-0 orders put the rows of a voxel in either
order, and the stand-in's neighbour table (first hit of a searchsorted over `torch.sort(key)`) resolved a tap to the voxel's
first row in 54 of 105 cases and to its last in 51 - the draw seed has no say in it, the sort is a function of the keys.
Any tie order is a valid result of an unstable sort, so the tool runs the reference with `stable=True` passed to every
torch.sort / torch.argsort call (`StableSorts` below): the recorded step is then the reference's arithmetic under the tie
rule this project documents - first row of a voxel = lowest caller index - and no seed had to be searched.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cdsegnet_amd import configs, synth  # noqa: E402
from oracle.make_golden import OUT, DrawRecorder, load_reference, ref_model, save_fixture  # noqa: E402

FULL = ["backbone._n_head.weight", "backbone._c_head.weight", "backbone._n_embedding.stem.conv.weight",
        "backbone._n_enc.enc2.block0.attn.qkv.weight", "backbone._n_enc.enc1.down.norm.0.weight", "backbone.fc_t1.weight",
        "backbone._tm_dec0.cross_block2.attn.kv.weight", "backbone._n_dec.dec0.up.proj.0.weight"]


class StableSorts:
    """Pass stable=True to every torch.sort / torch.argsort call (functions and Tensor methods) while the reference runs."""
    NAMES = ("sort", "argsort")

    def __enter__(self):
        self.saved = [(obj, name, getattr(obj, name)) for obj in (torch, torch.Tensor) for name in self.NAMES]
        for obj, name, fn in self.saved:
            # (with `stable`, dim and descending are keyword-only)
            setattr(obj, name, (lambda fn: lambda x, *a, **k: fn(x, **dict(zip(("dim", "descending"), a)), **dict(k, stable=True)))(fn))
        return self

    def __exit__(self, *exc):
        for obj, name, fn in self.saved:
            setattr(obj, name, fn)


def mix3d_scene(num_classes):
    a, b, c = synth.room_scene(81, 900), synth.room_scene(82, 700), synth.room_scene(83, 500)
    rng = np.random.default_rng(8)
    # 40 points of room a once more, jittered inside their voxel, placed IN FRONT of room a (caller's order: copies, a, b | c)
    pick = rng.choice(len(a["coord"]), 40, replace=False)
    cat = lambda k: np.concatenate([np.asarray(a[k])[pick], np.asarray(a[k]), np.asarray(b[k]), np.asarray(c[k])])  # noqa: E731
    coord = cat("coord").astype(np.float32)
    coord[:40] += rng.uniform(-0.002, 0.002, (40, 3)).astype(np.float32)
    feat = cat("feat").astype(np.float32)
    feat[:40] += rng.normal(0, 0.05, feat[:40].shape).astype(np.float32)
    grid = cat("grid_coord")
    seg = cat("segment").astype(np.int64) % num_classes
    seg[::17] = -1  # some unlabelled points (ignore_index)
    n0 = 40 + len(a["coord"]) + len(b["coord"])
    return dict(coord=coord, grid_coord=grid, feat=feat, offset=np.array([n0, n0 + len(c["coord"])], dtype=np.int64), segment=seg), 40


def check_batch(scene, copies):
    grid, offset = np.asarray(scene["grid_coord"], dtype=np.int64), scene["offset"]
    n0 = int(offset[0])
    key = (grid[:n0, 0] << 34) | (grid[:n0, 1] << 17) | grid[:n0, 2]
    _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    shared = float((cnt[inv] > 1).mean())
    assert shared >= 0.03, f"only {shared:.3f} of element 0's rows sit in shared voxels"
    assert cnt.max() >= 3, "no voxel holds three rows"
    # a voxel whose first row is one of the jittered copies (rows 0 .. copies - 1) and whose original follows
    first = np.full(len(cnt), n0, dtype=np.int64)
    np.minimum.at(first, inv, np.arange(n0))
    assert ((first < copies) & (cnt > 1)).any()
    key1 = np.asarray(scene["grid_coord"], dtype=np.int64)[n0:]
    assert len(np.unique(key1, axis=0)) == len(key1), "element 1 must have no shared voxel"
    return shared, int(cnt.max())


def main():
    ref = load_reference()
    import pointcept.models.losses  # noqa: F401  (registers the criteria)
    cfg = configs.mini_config()
    cfg["criteria"] = [dict(type="MSELoss", loss_weight=1.0, ignore_index=-1, batch_sample_point=-1),
                       dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1),
                       dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)]
    model, _ = ref_model(ref, cfg, seed=21)
    model.train()
    scene, copies = mix3d_scene(cfg["num_classes"])
    shared, most = check_batch(scene, copies)
    n = len(scene["coord"])
    inp = {k: torch.from_numpy(np.asarray(scene[k])) for k in ("coord", "grid_coord", "feat", "offset", "segment")}
    masks, cur = {}, [None]
    real_bernoulli, real_randint = torch.Tensor.bernoulli_, torch.randint
    for name, mod in model.named_modules():
        if type(mod).__name__ == "DropPath" and mod.drop_prob > 0.0:
            mod.register_forward_pre_hook(lambda m, a, name=name: cur.__setitem__(0, (name, 1.0 - m.drop_prob)))

    def bernoulli_(self, *a, **k):
        r = real_bernoulli(self, *a, **k)
        name, keep = cur[0]
        masks.setdefault(name, []).append((r / keep).clone().numpy())
        return r

    ts_log, orders = [], []

    def randint(*a, **k):
        r = real_randint(*a, **k)
        ts_log.append(r.clone())
        return r

    real_serialization = ref.structure.Point.serialization

    def serialization(self, *a, **k):
        real_serialization(self, *a, **k)
        if self["serialized_order"].shape[1] == n:  # level 0 of a branch: (4, N) in the caller's row order
            orders.append((self["serialized_code"].clone(), self["serialized_order"].clone()))

    caps, parts = {}, []
    torch.manual_seed(123)
    torch.Tensor.bernoulli_, torch.randint, ref.structure.Point.serialization = bernoulli_, randint, serialization
    try:
        with DrawRecorder() as rec, StableSorts():
            hooks = [model.backbone._n_head.register_forward_hook(lambda m, a, o: (o.retain_grad(), caps.__setitem__("n_pred", o))[1]),
                     model.backbone._c_head.register_forward_hook(lambda m, a, o: (o.retain_grad(), caps.__setitem__("c_pred", o))[1])]
            for c in model.criteria.criteria:
                c.register_forward_hook(lambda m, a, o: parts.append(float(o)))
            loss = model(inp)["loss"]
            loss.backward()
            for h in hooks:
                h.remove()
    finally:
        torch.Tensor.bernoulli_, torch.randint, ref.structure.Point.serialization = real_bernoulli, real_randint, real_serialization
    normals = [t for k, t in rec.log if k == "normal"]
    perms = [t for k, t in rec.log if k == "randperm"]
    assert len(ts_log) == 1 and len(normals) == 1 and len(perms) == 8, (len(ts_log), len(normals), len(perms))
    # the tie rule: is every recorded level-0 order the STABLE argsort of its code (ties by ascending caller index)?
    assert len(orders) == 2 and all(o.shape == (4, n) for _, o in orders)
    ties, stable = 0, 0
    for code, order in orders:
        for r in range(4):
            want = torch.sort(code[r], stable=True).indices
            assert torch.equal(code[r][order[r]], code[r][want])  # a permutation that sorts the codes
            stable += int(torch.equal(order[r], want))
            ties += int((code[r][want][1:] == code[r][want][:-1]).sum())
    assert ties > 0
    assert stable == 8, f"only {stable} of the 8 level-0 orders break ties by ascending caller index"
    assert int(scene["offset"][0]) > cfg["backbone"]["n_enc_patch_size"][0]  # element 0 spans two patches
    assert caps["n_pred"].shape[0] == n and normals[0].shape[0] == n
    names = [k for k, _ in model.named_parameters()]
    pd = dict(model.named_parameters())
    gnorm = np.array([float(p.grad.norm()) if p.grad is not None else -1.0 for p in pd.values()], dtype=np.float64)
    fx = dict(coord=scene["coord"], grid_coord=scene["grid_coord"], feat=scene["feat"], offset=scene["offset"], segment=scene["segment"],
              sd_seed=np.int64(21), ts=ts_log[0].numpy(), noise=normals[0].numpy(), perms=np.stack([p.numpy() for p in perms]),
              loss=np.float64(float(loss)), loss_parts=np.array(parts, dtype=np.float64),
              n_pred=caps["n_pred"].detach().numpy(), c_pred=caps["c_pred"].detach().numpy(),
              d_n_pred=caps["n_pred"].grad.numpy(), d_c_pred=caps["c_pred"].grad.numpy(),
              grad_names=np.array(names), grad_norms=gnorm, level0_orders=torch.stack([o for _, o in orders]).numpy().astype(np.int32))
    for k in FULL:
        assert pd[k].grad is not None
        fx["g." + k] = pd[k].grad.numpy().copy()
    # one AdamW step on those gradients, grouped and set like gen_train_step's (lr 2e-3, "block" parameters 2e-4, decay 0.05)
    before = {k: p.detach().clone() for k, p in pd.items()}
    groups = [dict(params=[p for k, p in pd.items() if "block" not in k], lr=0.002),
              dict(params=[p for k, p in pd.items() if "block" in k], lr=0.0002)]
    torch.optim.AdamW(groups, lr=0.002, weight_decay=0.05).step()
    fx["step_norms"] = np.array([float((p.detach() - before[k]).norm()) for k, p in pd.items()], dtype=np.float64)
    for k in ("backbone._n_head.weight", "backbone._n_enc.enc2.block0.attn.qkv.weight"):
        fx["p1." + k] = pd[k].detach().numpy().copy()
    mk = sorted(masks)
    fx["mask_names"] = np.array(mk)
    fx["mask_counts"] = np.array([len(masks[k]) for k in mk], dtype=np.int64)
    for i, k in enumerate(mk):
        for j, m in enumerate(masks[k]):
            fx[f"mask.{i}.{j}"] = m.astype(np.float32)
    path = os.path.join(OUT, "train_step_mix3d.npz")
    save_fixture(path, **fx)
    print(f"train_step_mix3d: loss {float(loss):.6f} parts {parts}; {n} points, {100 * shared:.1f} % of element 0's rows in shared "
          f"voxels, at most {most} rows a voxel, {ties} tied neighbours in the 8 level-0 orders, {stable} of them stable; DropPath modules {len(mk)}; "
          f"params with grad {int((gnorm >= 0).sum())} of {len(gnorm)}; {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
