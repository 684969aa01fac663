"""TEST INFRASTRUCTURE shared by tests/test_cpu_fusion.py and tests/test_gpu_fusion.py: the models of the fusion fixtures
(tools/make_fusion_golden.py) rebuilt from their recorded settings."""
import copy
import json

import torch

import cdsegnet_amd.models  # noqa: F401
from cdsegnet_amd.param_init import fill_state_dict
from cdsegnet_amd.registry import build_model

INFER_TAGS = ["lr_scale", "b_lr_scale", "channel_scale", "b_channel_scale", "bidir_channel_scale"]
CRITERIA = [dict(type="MSELoss", loss_weight=1.0, ignore_index=-1, batch_sample_point=-1),
            dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1),
            dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)]


def fusion_state_dict(model, fx):
    """The generator's weights: the name-keyed fill, the cross blocks' attn.proj enlarged by the recorded gain, every
    feat_scale as recorded."""
    sd = fill_state_dict(model.state_dict(), seed=int(fx["sd_seed"]))
    gain = float(fx["gain"])
    for k in sd:
        if k.endswith("feat_scale"):
            sd[k] = torch.as_tensor(fx["fs." + k])
        elif "._tm_dec0." in k and ".attn.proj." in k:
            sd[k] = sd[k] * gain
    return sd


def infer_model(fx, default=False):
    """The model of a fusion_infer fixture (reference's CPU branch: enable_flash=False).  default: the default fusion config
    on the same weights."""
    cfg = copy.deepcopy(json.loads(str(fx["cfg_json"])))
    cfg["backbone"]["enable_flash"] = False
    if default:
        cfg["backbone"].update(tm_feat=1.0, tm_bidirectional=False)
    model = build_model(cfg)
    model.load_state_dict(fusion_state_dict(model, fx), strict=True)
    return model.eval(), cfg


def train_model(fx):
    from cdsegnet_amd import configs
    cfg = configs.mini_config(tm_feat="b_channel_scale", tm_bidirectional=True)
    cfg["backbone"]["enable_flash"] = False
    cfg["criteria"] = copy.deepcopy(CRITERIA)
    model = build_model(cfg)
    sd = fusion_state_dict(model, fx)
    model.load_state_dict(sd, strict=True)
    return model.train(), sd


def train_draws(fx):
    masks = {str(k): [fx[f"mask.{i}.{j}"] for j in range(int(fx["mask_counts"][i]))] for i, k in enumerate(fx["mask_names"])}
    return dict(ts=fx["ts"], noise=fx["noise"], perms=[list(p) for p in fx["perms"]], masks=masks)


def ssi_draws(fx):
    return dict(noise=torch.from_numpy(fx["noise"]), perms=[p for p in fx["perms"]])


def ddim_draws(fx):
    return dict(noise=torch.from_numpy(fx["ddim_noise"]), perms=[p for p in fx["ddim_perms"]])
