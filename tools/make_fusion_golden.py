#!/usr/bin/env python3
"""Record the reference's Feature Fusion Module options: learned fusion scales (tm_feat) and bidirectional fusion.

Run from the repo root:  python tools/make_fusion_golden.py   (needs the reference checkout, like oracle/make_golden.py)

Mini model, one batch of two rooms of different size (900 and 600 points), so that each bottleneck holds several rows per
batch element.  Written to tests/golden/:
  state_dict_schema_fusion.json   key order and shapes of tm_bidirectional=True + tm_feat="b_channel_scale", and of
                                  tm_feat="lr_scale" alone
  fusion_infer_<tag>.npz          for each of the four tm_feat modes, and for bidirectional + "channel_scale": single-step
                                  logits and one inference_ddim(step=2, mode="avg"), with all draws
  fusion_train_step.npz           the reference's training step (oracle/make_golden.py's gen_train_step recipe) for
                                  bidirectional + "b_channel_scale": loss and parts, both predictions, the norm of every
                                  parameter gradient, twelve gradients in full (both feat_scales among them), the first AdamW
                                  step, every draw
Every feat_scale is overwritten with seeded normal values before recording (kept in the fixture as "fs.<key>"), so that the
per-channel indexing and the sigmoid are visible, and attn.proj of the cross blocks is enlarged by "gain" (the name-keyed fill
leaves the fusion term at a few hundredths of a logit).  What the tool asserts, with the reference alone, before it writes:
  * the logits of every fixture differ from the default config's logits on the same weights and draws by more than 100 x the
    fp32 test bound (1e-3 single-step, 5e-5 multi-step: tests/test_gpu_e2e.py) - an implementation that ignores the option
    cannot pass;
  * with a hook that restores the n point's feat / sparse_conv_feat behind cross_block1, the bidirectional logits move by more
    than 100 x that bound: "the n point enters cross_block2 normed" is visible at the test's resolution;
  * the recorded DropPath masks of the training step hold a dropped row for each cross block.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cdsegnet_amd import configs, synth  # noqa: E402
from oracle.make_golden import OUT, DrawRecorder, load_reference, ref_model, save_fixture, to_torch_input  # noqa: E402

BOUND_SSI, BOUND_MSI = 1e-3, 5e-5  # the fp32 bounds of tests/test_gpu_e2e.py
INFER = [("lr_scale", "lr_scale", False), ("b_lr_scale", "b_lr_scale", False), ("channel_scale", "channel_scale", False),
         ("b_channel_scale", "b_channel_scale", False), ("bidir_channel_scale", "channel_scale", True)]
FULL = ["backbone._n_head.weight", "backbone._c_head.weight", "backbone._n_embedding.stem.conv.weight",
        "backbone._n_enc.enc2.block0.attn.qkv.weight", "backbone._n_enc.enc1.down.norm.0.weight", "backbone.fc_t1.weight",
        "backbone._tm_dec0.cross_block2.attn.kv.weight", "backbone._n_dec.dec0.up.proj.0.weight",
        "backbone._tm_dec0.cross_block1.feat_scale", "backbone._tm_dec0.cross_block2.feat_scale",
        "backbone._tm_dec0.cross_block1.attn.kv.weight", "backbone._tm_dec0.cross_block1.q_cpe.0.weight"]
CRITERIA = [dict(type="MSELoss", loss_weight=1.0, ignore_index=-1, batch_sample_point=-1),
            dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1),
            dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)]


def fusion_scene():
    return synth.collate([synth.room_scene(91, 900), synth.room_scene(92, 600)])


GAIN = 16.0  # on the cross blocks' attn.proj (weight and bias): the name-keyed fill leaves the fusion term too small to see


def gained(k):
    return "._tm_dec0." in k and ".attn.proj." in k


def fusion_model(ref, cfg, seed):
    """The reference model of `cfg` with name-keyed weights, the cross blocks' attn.proj enlarged by GAIN and every feat_scale
    overwritten by seeded normal values."""
    model, sd = ref_model(ref, cfg, seed=seed)
    g = torch.Generator().manual_seed(1000 + seed)
    fs = {}
    for k in sd:
        if k.endswith("feat_scale"):
            sd[k] = fs[k] = torch.randn(sd[k].shape, generator=g)
        elif gained(k):
            sd[k] = sd[k] * GAIN
    model.load_state_dict(sd, strict=True)
    return model, fs


def run_both(model, cfg, inp, seed):
    """(single-step logits, its draws, multi-step logits, its draws) of the reference under torch.manual_seed(seed)."""
    torch.manual_seed(seed)
    with DrawRecorder() as r1, torch.no_grad():
        ssi = model.inference(dict(inp), eval=False)["seg_logits"].numpy()
    assert [k for k, _ in r1.log] == ["normal"] + ["randperm"] * 8
    torch.manual_seed(seed + 1)
    with DrawRecorder() as r2, torch.no_grad():
        msi = model.inference_ddim(dict(inp), T=cfg["T"], step=2, eval=False, mode="avg")["seg_logits"].numpy()
    assert [k for k, _ in r2.log] == ["normal"] + ["randperm"] * 24
    return ssi, r1.log, msi, r2.log


class RestoreN:
    """Hooks on cross_block1 that put the n point's feat / sparse_conv_feat back to what they were in front of it."""

    def __init__(self, block):
        self.h = [block.register_forward_pre_hook(self.pre), block.register_forward_hook(self.post)]

    def pre(self, mod, args):
        self.feat = args[1].feat.clone()

    def post(self, mod, args, out):
        n = args[1]
        n.feat = self.feat
        n.sparse_conv_feat = n.sparse_conv_feat.replace_feature(self.feat)

    def remove(self):
        for h in self.h:
            h.remove()


def gen_schema(ref):
    out = {}
    for tag, mode, bidir in (("bidir_b_channel_scale", "b_channel_scale", True), ("lr_scale", "lr_scale", False)):
        model, _ = ref_model(ref, configs.mini_config(tm_feat=mode, tm_bidirectional=bidir), seed=0)
        out[tag] = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    with open(os.path.join(OUT, "state_dict_schema_fusion.json"), "w") as f:
        json.dump(out, f, indent=0)
    print("schema", {k: len(v) for k, v in out.items()})


def gen_infer(ref, scene):
    inp = to_torch_input(scene)
    seed, sd_seed = 61, 31
    base, _ = fusion_model(ref, configs.mini_config(), sd_seed)  # (no feat_scale: the same weights, gain included)
    b_ssi, _, b_msi, _ = run_both(base, configs.mini_config(), inp, seed)
    for tag, mode, bidir in INFER:
        cfg = configs.mini_config(tm_feat=mode, tm_bidirectional=bidir)
        model, fs = fusion_model(ref, cfg, sd_seed)
        ssi, d1, msi, d2 = run_both(model, cfg, inp, seed)
        m1, m2 = float(np.abs(ssi - b_ssi).max()), float(np.abs(msi - b_msi).max())
        assert m1 > 100 * BOUND_SSI and m2 > 100 * BOUND_MSI, (tag, m1, m2)
        note = ""
        if bidir:
            hook = RestoreN(model.backbone._tm_dec0.cross_block1)
            r_ssi, _, r_msi, _ = run_both(model, cfg, inp, seed)
            hook.remove()
            q1, q2 = float(np.abs(ssi - r_ssi).max()), float(np.abs(msi - r_msi).max())
            assert q1 > 100 * BOUND_SSI and q2 > 100 * BOUND_MSI, (tag, q1, q2)
            note = f"; n point restored behind cross_block1: logits move {q1:.3f} / {q2:.5f}"
        fx = dict(coord=scene["coord"], grid_coord=scene["grid_coord"], feat=scene["feat"], offset=scene["offset"],
                  sd_seed=np.int64(sd_seed), gain=np.float64(GAIN), cfg_json=np.array(json.dumps(cfg)),
                  logits=ssi, noise=d1[0][1].numpy(), perms=np.stack([v.numpy() for k, v in d1 if k == "randperm"]),
                  ddim_logits=msi, ddim_noise=d2[0][1].numpy(), ddim_perms=np.stack([v.numpy() for k, v in d2 if k == "randperm"]),
                  ddim_step=np.int64(2), ddim_mode=np.array("avg"))
        for k, v in fs.items():
            fx["fs." + k] = v.numpy()
        path = os.path.join(OUT, f"fusion_infer_{tag}.npz")
        save_fixture(path, **fx)
        print(f"fusion_infer_{tag}: differs from the default config by {m1:.3f} (single-step) / {m2:.5f} (multi-step){note}; "
              f"{os.path.getsize(path)} bytes")


def gen_train(ref, scene):
    """oracle/make_golden.py's gen_train_step on the bidirectional + b_channel_scale model."""
    import pointcept.models.losses  # noqa: F401  (registers the criteria)
    cfg = configs.mini_config(tm_feat="b_channel_scale", tm_bidirectional=True)
    cfg["criteria"] = CRITERIA
    sd_seed = 33
    model, fs = fusion_model(ref, cfg, sd_seed)
    model.train()
    seg = np.asarray(scene["segment"]).astype(np.int64) % cfg["num_classes"]
    seg[::17] = -1  # some unlabelled points (ignore_index)
    inp = to_torch_input(scene)
    inp["segment"] = torch.from_numpy(seg)
    masks, order, cur = {}, [], [None]
    real_bernoulli, real_randint = torch.Tensor.bernoulli_, torch.randint
    for name, mod in model.named_modules():
        if type(mod).__name__ == "DropPath" and mod.drop_prob > 0.0:
            mod.register_forward_pre_hook(lambda m, a, name=name: cur.__setitem__(0, (name, 1.0 - m.drop_prob)))

    def bernoulli_(self, *a, **k):
        r = real_bernoulli(self, *a, **k)
        name, keep = cur[0]
        masks.setdefault(name, []).append((r / keep).clone().numpy())
        order.append(name)
        return r

    ts_log = []

    def randint(*a, **k):
        r = real_randint(*a, **k)
        ts_log.append(r.clone())
        return r

    caps, parts = {}, []
    torch.manual_seed(321)
    torch.Tensor.bernoulli_, torch.randint = bernoulli_, randint
    try:
        with DrawRecorder() as rec:
            hooks = [model.backbone._n_head.register_forward_hook(lambda m, a, o: (o.retain_grad(), caps.__setitem__("n_pred", o))[1]),
                     model.backbone._c_head.register_forward_hook(lambda m, a, o: (o.retain_grad(), caps.__setitem__("c_pred", o))[1])]
            for c in model.criteria.criteria:
                c.register_forward_hook(lambda m, a, o: parts.append(float(o)))
            loss = model(inp)["loss"]
            loss.backward()
            for h in hooks:
                h.remove()
    finally:
        torch.Tensor.bernoulli_, torch.randint = real_bernoulli, real_randint
    normals = [t for k, t in rec.log if k == "normal"]
    perms = [t for k, t in rec.log if k == "randperm"]
    assert len(ts_log) == 1 and len(normals) == 1 and len(perms) == 8, (len(ts_log), len(normals), len(perms))
    for blk in ("cross_block1", "cross_block2"):
        name = f"backbone._tm_dec0.{blk}.drop_path.0"
        assert len(masks[name]) == 2 and all((m == 0).any() for m in masks[name]), f"no dropped row in the masks of {blk}"
    x1 = [i for i, k in enumerate(order) if "cross_block1" in k]
    x2 = [i for i, k in enumerate(order) if "cross_block2" in k]
    assert max(x1) < min(x2), "cross_block1 draws its masks in front of cross_block2"
    pd = dict(model.named_parameters())
    names = list(pd)
    gnorm = np.array([float(p.grad.norm()) if p.grad is not None else -1.0 for p in pd.values()], dtype=np.float64)
    fx = dict(coord=scene["coord"], grid_coord=scene["grid_coord"], feat=scene["feat"], offset=scene["offset"], segment=seg,
              sd_seed=np.int64(sd_seed), gain=np.float64(GAIN), ts=ts_log[0].numpy(), noise=normals[0].numpy(), perms=np.stack([p.numpy() for p in perms]),
              loss=np.float64(float(loss)), loss_parts=np.array(parts, dtype=np.float64),
              n_pred=caps["n_pred"].detach().numpy(), c_pred=caps["c_pred"].detach().numpy(),
              grad_names=np.array(names), grad_norms=gnorm, mask_order=np.array(order))
    for k, v in fs.items():
        fx["fs." + k] = v.numpy()
    for k in FULL:
        assert pd[k].grad is not None, k
        fx["g." + k] = pd[k].grad.numpy().copy()
    before = {k: p.detach().clone() for k, p in pd.items()}
    groups = [dict(params=[p for k, p in pd.items() if "block" not in k], lr=0.002),
              dict(params=[p for k, p in pd.items() if "block" in k], lr=0.0002)]
    torch.optim.AdamW(groups, lr=0.002, weight_decay=0.05).step()
    fx["step_norms"] = np.array([float((p.detach() - before[k]).norm()) for k, p in pd.items()], dtype=np.float64)
    for k in ("backbone._n_head.weight", "backbone._tm_dec0.cross_block1.feat_scale", "backbone._tm_dec0.cross_block2.feat_scale"):
        fx["p1." + k] = pd[k].detach().numpy().copy()
    mk = sorted(masks)
    fx["mask_names"] = np.array(mk)
    fx["mask_counts"] = np.array([len(masks[k]) for k in mk], dtype=np.int64)
    for i, k in enumerate(mk):
        for j, m in enumerate(masks[k]):
            fx[f"mask.{i}.{j}"] = m.astype(np.float32)
    path = os.path.join(OUT, "fusion_train_step.npz")
    save_fixture(path, **fx)
    print(f"fusion_train_step: loss {float(loss):.6f} parts {parts}; DropPath modules {len(mk)}; params with grad "
          f"{int((gnorm >= 0).sum())} of {len(gnorm)}; |g feat_scale| {[float(fx['g.' + k].__abs__().max()) for k in FULL[8:10]]}; "
          f"{os.path.getsize(path)} bytes")


def main():
    torch.set_num_threads(8)
    ref = load_reference()
    scene = fusion_scene()
    gen_schema(ref)
    gen_infer(ref, scene)
    gen_train(ref, scene)


if __name__ == "__main__":
    main()
