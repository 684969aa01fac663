"""TEST INFRASTRUCTURE shared by tests/test_cpu_vote_shared.py and tests/test_gpu_vote_shared.py: the mini LiDAR model of
tests/golden/mini_e2e_lidar.npz, the three-list cut of the nuScenes test block (as tests/test_gpu_testpipeline.py builds them:
its fixtures cannot be imported) and the explicitly chosen order shuffles of the faithful-batch tests.  Never imported by the
product."""
import copy
import itertools
import json
import os

import numpy as np
import torch

from tests.helpers import GOLDEN, fixture_cfg, fixture_state_dict, load_fixture

PERMS4 = [np.array(p, dtype=np.int64) for p in itertools.permutations(range(4))]
N_DRAWS = 8  # order shuffles of one conditional forward (2 + 2 c-branch + 4 n-branch poolings)


def blocks():
    with open(os.path.join(GOLDEN, "test_blocks.json")) as f:
        return json.load(f)


def block_cut(names=(0, 2, 9)):
    """The nuScenes test block with the aug_transform lists `names` (scale 0.9; scale 1; scale 1.1 + flip)."""
    cfg = copy.deepcopy(blocks()["nuscenes"])
    lists = cfg["test_cfg"]["aug_transform"]
    cfg["test_cfg"]["aug_transform"] = [lists[i] for i in names]
    return cfg


def mini_model(device=None):
    """(model in eval mode with precision "fp32", its config, its state dict)."""
    import cdsegnet_amd.models  # noqa: F401
    from cdsegnet_amd.registry import build_model
    fx = load_fixture("mini_e2e_lidar.npz")
    cfg = fixture_cfg(fx)
    sd = fixture_state_dict(fx)
    model = build_model(copy.deepcopy(cfg))
    model.load_state_dict(sd, strict=True)
    model = (model if device is None else model.to(device)).eval()
    model.precision = "fp32"
    return model, cfg, sd


def fragment_perms(f):
    """The 8 order shuffles of fragment f (its number in the scene's flat list): at every draw position two consecutive
    fragments differ (5 is no multiple of 24), so in every group of >= 2 consecutive fragments at least two differ."""
    return [PERMS4[(5 * f + 7 * p + 1) % 24] for p in range(N_DRAWS)]


def fragment_noise(f, rows, channels):
    g = torch.Generator().manual_seed(1000 + f)
    return torch.normal(0, 1, size=(rows, channels), dtype=torch.float32, generator=g)


def fragment_draws(f, rows, channels):
    """Injected draws of the single forward of fragment f."""
    return dict(noise=fragment_noise(f, rows, channels), perms=fragment_perms(f))


def group_draws(f0, k, rows, channels):
    """Injected draws of ONE collated forward over fragments f0 .. f0+k-1, every fragment under its own draws: the noise rows
    concatenated, k permutations per draw position."""
    per = [fragment_draws(f0 + j, rows, channels) for j in range(k)]
    return dict(per_fragment=True, noise=torch.cat([d["noise"] for d in per], 0),
                perms=[[d["perms"][p] for d in per] for p in range(N_DRAWS)])
