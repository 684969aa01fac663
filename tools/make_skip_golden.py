#!/usr/bin/env python3
"""Record the reference's skip-connection options: the 'add' mode with a skip scale, ScaleLong's exponential scales and
FreeU's factors (skip_connection_mode, skip_connection_scale, skip_connection_scale_i, b_factor, s_factor).

Run from the repo root:  python tools/make_skip_golden.py   (needs the reference checkout, like oracle/make_golden.py)

Mini models with name-keyed weights.  Written to tests/golden/, each file no larger than the fusion fixtures (which is why the
single rooms hold 1500 points and the collated batch 900 + 600):
  skip_infer_<tag>.npz    single-step logits and one inference_ddim(step=2, mode="avg"), with all draws, for
      add_scale      skip_connection_mode="add", skip_connection_scale=True
      cat_scale_i    "cat", skip_connection_scale_i=True
      cat_all_s      "cat_all", skip_connection_scale_i=True, s_factor=[0.9, 0.8, 1.1, 1.0]
      cat_s_b_batch2 "cat", that s_factor, b_factor=[1.2, 1.0, 1.0, 1.4], on a collated batch of two rooms
      b_only         b_factor=[1.2, 1.2, 1.2, 1.2], s_factor all 1
  skip_train_step.npz     the reference's training step (oracle/make_golden.py's gen_train_step recipe) for "add" +
                          skip_connection_scale_i=True: loss and parts, both predictions, the norm of every parameter
                          gradient, ten gradients in full, every draw
  skip_train_fwd_s.npz    the same model with that s_factor, training-mode FORWARD only (loss, parts, predictions, draws): the
                          reference cannot differentiate through freeU (an in-place write, ptv3.py:96; see gen_train)
What the tool asserts, with the reference alone, before it writes:
  * the logits of every fixture but b_only differ from the default config's logits on the same weights and draws by more than
    50 x the fp32 test bound - an implementation that ignores the option cannot pass (add_scale: "add" changes the c-decoder
    alone, so its single-step logits ARE the default's and its multi-step logits differ by more than 30 x the bound);
  * b_only's logits differ from the default's by no more than FFT rounding (b_factor has no effect of its own: the reference
    reads the channel count behind the channel mean, ptv3.py:81-96).
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
S = [0.9, 0.8, 1.1, 1.0]
INFER = [("add_scale", dict(skip_connection_mode="add", skip_connection_scale=True), False),
         ("cat_scale_i", dict(skip_connection_mode="cat", skip_connection_scale_i=True), False),
         ("cat_all_s", dict(skip_connection_mode="cat_all", skip_connection_scale_i=True, s_factor=S), False),
         ("cat_s_b_batch2", dict(skip_connection_mode="cat", s_factor=S, b_factor=[1.2, 1.0, 1.0, 1.4]), True),
         ("b_only", dict(b_factor=[1.2, 1.2, 1.2, 1.2]), False)]
TRAIN = dict(skip_connection_mode="add", skip_connection_scale_i=True)
TRAIN_S = dict(TRAIN, s_factor=S)
FULL = ["backbone._n_head.weight", "backbone._c_head.weight", "backbone._n_embedding.stem.conv.weight",
        "backbone._n_enc.enc2.block0.attn.qkv.weight", "backbone._n_enc.enc1.down.norm.0.weight", "backbone.fc_t1.weight",
        "backbone._n_dec.dec0.up.proj.0.weight", "backbone._n_dec.dec1.up.proj_skip.0.weight",
        "backbone._c_dec.dec0.up.proj_skip.0.weight", "backbone._n_enc.enc0.block0.mlp.0.fc2.weight"]
CRITERIA = [dict(type="MSELoss", loss_weight=1.0, ignore_index=-1, batch_sample_point=-1),
            dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1),
            dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)]


def scene(batch2):
    if batch2:
        return synth.collate([synth.room_scene(91, 900), synth.room_scene(92, 600)])
    return synth.collate([synth.room_scene(93, 1500)])


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


def gen_infer(ref):
    seed, sd_seed = 71, 41
    for tag, kw, batch2 in INFER:
        sc = scene(batch2)
        inp = to_torch_input(sc)
        cfg = configs.mini_config(**kw)
        model, sd = ref_model(ref, cfg, seed=sd_seed)
        ssi, d1, msi, d2 = run_both(model, cfg, inp, seed)
        # the default config on the same name-keyed weights (the modes differ only in which unpoolings own a proj_cat)
        base, bsd = ref_model(ref, configs.mini_config(), seed=sd_seed)
        assert all(torch.equal(sd[k], bsd[k]) for k in sd if k in bsd)
        b_ssi, _, b_msi, _ = run_both(base, configs.mini_config(), inp, seed)
        m1, m2 = float(np.abs(ssi - b_ssi).max()), float(np.abs(msi - b_msi).max())
        if tag == "b_only":
            assert m1 < BOUND_SSI and m2 < BOUND_MSI, (tag, m1, m2)
        elif tag == "add_scale":
            # "add" changes the c-decoder alone, which a single-step inference never reaches seg_logits through; the second
            # backbone call of the multi-step run reads its noise estimate
            assert m1 == 0.0 and m2 > 30 * BOUND_MSI, (tag, m1, m2)
        else:
            assert m1 > 50 * BOUND_SSI and m2 > 50 * BOUND_MSI, (tag, m1, m2)
        fx = dict(coord=sc["coord"], grid_coord=sc["grid_coord"], feat=sc["feat"], offset=sc["offset"],
                  sd_seed=np.int64(sd_seed), cfg_json=np.array(json.dumps(cfg)),
                  logits=ssi, noise=d1[0][1].numpy(), perms=np.stack([v.numpy() for k, v in d1 if k == "randperm"]),
                  ddim_logits=msi, ddim_noise=d2[0][1].numpy(), ddim_perms=np.stack([v.numpy() for k, v in d2 if k == "randperm"]),
                  ddim_step=np.int64(2), ddim_mode=np.array("avg"), default_delta=np.array([m1, m2]))
        path = os.path.join(OUT, f"skip_infer_{tag}.npz")
        save_fixture(path, **fx)
        print(f"skip_infer_{tag}: differs from the default config by {m1:.3g} (single-step) / {m2:.3g} (multi-step); "
              f"{os.path.getsize(path)} bytes")


def gen_train(ref, kw, fname, backward):
    """oracle/make_golden.py's gen_train_step on the model of `kw`.  backward=False: the training-mode forward alone, under
    torch.no_grad() - the reference's freeU writes `b_feat[:, :C_num]` in place (ptv3.py:96), which autograd refuses, so the
    reference itself cannot take a gradient through a module with b != 1 or s != 1 (FreeU is an inference-time knob)."""
    import pointcept.models.losses  # noqa: F401  (registers the criteria)
    sc = scene(True)
    cfg = configs.mini_config(**kw)
    cfg["criteria"] = CRITERIA
    sd_seed = 43
    model, _ = ref_model(ref, cfg, seed=sd_seed)
    model.train()
    seg = np.asarray(sc["segment"]).astype(np.int64) % cfg["num_classes"]
    seg[::17] = -1  # some unlabelled points (ignore_index)
    inp = to_torch_input(sc)
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
    torch.manual_seed(322)
    torch.Tensor.bernoulli_, torch.randint = bernoulli_, randint
    try:
        with DrawRecorder() as rec:
            hooks = [model.backbone._n_head.register_forward_hook(lambda m, a, o: caps.__setitem__("n_pred", o)),
                     model.backbone._c_head.register_forward_hook(lambda m, a, o: caps.__setitem__("c_pred", o))]
            for c in model.criteria.criteria:
                c.register_forward_hook(lambda m, a, o: parts.append(float(o.detach())))
            with torch.set_grad_enabled(backward):
                loss = model(inp)["loss"]
            if backward:
                loss.backward()
            for h in hooks:
                h.remove()
    finally:
        torch.Tensor.bernoulli_, torch.randint = real_bernoulli, real_randint
    normals = [t for k, t in rec.log if k == "normal"]
    perms = [t for k, t in rec.log if k == "randperm"]
    assert len(ts_log) == 1 and len(normals) == 1 and len(perms) == 8, (len(ts_log), len(normals), len(perms))
    pd = dict(model.named_parameters())
    names = list(pd)
    fx = dict(coord=sc["coord"], grid_coord=sc["grid_coord"], feat=sc["feat"], offset=sc["offset"], segment=seg,
              sd_seed=np.int64(sd_seed), cfg_json=np.array(json.dumps(configs.mini_config(**kw))), ts=ts_log[0].numpy(),
              noise=normals[0].numpy(), perms=np.stack([p.numpy() for p in perms]),
              loss=np.float64(float(loss.detach())), loss_parts=np.array(parts, dtype=np.float64),
              n_pred=caps["n_pred"].detach().numpy(), c_pred=caps["c_pred"].detach().numpy(),
              mask_order=np.array(order))
    if backward:
        gnorm = np.array([float(p.grad.norm()) if p.grad is not None else -1.0 for p in pd.values()], dtype=np.float64)
        fx.update(grad_names=np.array(names), grad_norms=gnorm)
        for k in FULL:
            assert pd[k].grad is not None, k
            fx["g." + k] = pd[k].grad.numpy().copy()
    mk = sorted(masks)
    fx["mask_names"] = np.array(mk)
    fx["mask_counts"] = np.array([len(masks[k]) for k in mk], dtype=np.int64)
    for i, k in enumerate(mk):
        for j, m in enumerate(masks[k]):
            fx[f"mask.{i}.{j}"] = m.astype(np.float32)
    path = os.path.join(OUT, fname)
    save_fixture(path, **fx)
    print(f"{fname}: loss {float(loss):.6f} parts {parts}; DropPath modules {len(mk)}; {os.path.getsize(path)} bytes")


def main():
    torch.set_num_threads(8)
    ref = load_reference()
    gen_infer(ref)
    gen_train(ref, TRAIN, "skip_train_step.npz", True)
    gen_train(ref, TRAIN_S, "skip_train_fwd_s.npz", False)


if __name__ == "__main__":
    main()
