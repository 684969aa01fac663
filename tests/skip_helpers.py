"""TEST INFRASTRUCTURE shared by tests/test_cpu_skip.py and tests/test_gpu_skip.py: the models of the skip-option fixtures
(tools/make_skip_golden.py) rebuilt from their recorded settings."""
import copy
import json

import torch

import cdsegnet_amd.models  # noqa: F401
from cdsegnet_amd.param_init import fill_state_dict
from cdsegnet_amd.registry import build_model

S = [0.9, 0.8, 1.1, 1.0]
# the five configurations of the fixtures: tag -> switches
INFER = {"add_scale": dict(skip_connection_mode="add", skip_connection_scale=True),
         "cat_scale_i": dict(skip_connection_mode="cat", skip_connection_scale_i=True),
         "cat_all_s": dict(skip_connection_mode="cat_all", skip_connection_scale_i=True, s_factor=S),
         "cat_s_b_batch2": dict(skip_connection_mode="cat", s_factor=S, b_factor=[1.2, 1.0, 1.0, 1.4]),
         "b_only": dict(b_factor=[1.2, 1.2, 1.2, 1.2])}
CRITERIA = [dict(type="MSELoss", loss_weight=1.0, ignore_index=-1, batch_sample_point=-1),
            dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1),
            dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)]


def fixture_model(fx, train=False, **override):
    """The model of a skip fixture (reference's CPU branch: enable_flash=False) with the generator's name-keyed weights.
    override: backbone settings replaced on the same weights (e.g. b_factor=[1, 1, 1, 1])."""
    cfg = copy.deepcopy(json.loads(str(fx["cfg_json"])))
    cfg["backbone"]["enable_flash"] = False
    cfg["backbone"].update(override)
    if train:
        cfg["criteria"] = copy.deepcopy(CRITERIA)
    model = build_model(cfg)
    model.load_state_dict(fill_state_dict(model.state_dict(), seed=int(fx["sd_seed"])), strict=True)
    return (model.train() if train else model.eval()), cfg


def train_draws(fx):
    masks = {str(k): [fx[f"mask.{i}.{j}"] for j in range(int(fx["mask_counts"][i]))] for i, k in enumerate(fx["mask_names"])}
    return dict(ts=fx["ts"], noise=fx["noise"], perms=[list(p) for p in fx["perms"]], masks=masks)


def ssi_draws(fx):
    return dict(noise=torch.from_numpy(fx["noise"]), perms=[p for p in fx["perms"]])


def ddim_draws(fx):
    return dict(noise=torch.from_numpy(fx["ddim_noise"]), perms=[p for p in fx["ddim_perms"]])
