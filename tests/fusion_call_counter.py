"""TEST INFRASTRUCTURE: counts the library calls (functions of cdsegnet_amd.ops, by name) a default mini model makes during one
`inference` and one training step.  tests/test_gpu_fusion.py compares the counts with the ones recorded on the commit before
the fusion options existed; this module imports nothing that commit lacks, so the same code counted there."""
import collections
import inspect
import threading

import torch

import cdsegnet_amd.models  # noqa: F401
import cdsegnet_amd.ops as O
from cdsegnet_amd import configs
from cdsegnet_amd.param_init import fill_state_dict
from cdsegnet_amd.registry import build_model
from tests.helpers import fixture_cfg, fixture_draws, fixture_input, fixture_state_dict, load_fixture

CRITERIA = [dict(type="MSELoss", loss_weight=1.0, ignore_index=-1, batch_sample_point=-1),
            dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1),
            dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)]


class _CallCounter:
    def __init__(self, setattr_):
        self.counts = collections.Counter()
        self.lock = threading.Lock()  # (autograd runs backward on a thread of its own)
        for name, fn in list(vars(O).items()):
            # (det_kw: a host helper the training graph binds by name at import - seen or not depending on import order)
            if inspect.isfunction(fn) and fn.__module__ == O.__name__ and not name.startswith("_") and name != "det_kw":
                setattr_(O, name, self._wrap(name, fn))

    def _wrap(self, name, fn):
        def call(*a, **k):
            with self.lock:
                self.counts[name] += 1
            return fn(*a, **k)
        return call

    def take(self):
        out = sorted(self.counts.items())
        self.counts.clear()
        return [list(x) for x in out]


def default_model_calls(setattr_):
    """([name, count] of one inference, [name, count] of one training step) of a default mini model."""
    fx = load_fixture("mini_e2e_room.npz")
    model = build_model(fixture_cfg(fx))
    model.load_state_dict(fixture_state_dict(fx), strict=True)
    model = model.cuda().eval()
    inp = {k: torch.as_tensor(v).cuda() for k, v in fixture_input(fx).items()}
    model.inference(dict(inp), eval=False, draws=fixture_draws(fx))  # (prepared weights, allocator warm-up: not counted)
    torch.cuda.synchronize()
    counter = _CallCounter(setattr_)
    model.inference(dict(inp), eval=False, draws=fixture_draws(fx))
    torch.cuda.synchronize()
    infer = counter.take()
    fx = load_fixture("train_step_mini.npz")
    cfg = configs.mini_config()
    cfg["backbone"]["enable_flash"] = False
    cfg["criteria"] = [dict(c) for c in CRITERIA]
    model = build_model(cfg)
    model.load_state_dict(fill_state_dict(model.state_dict(), seed=int(fx["sd_seed"])))
    model = model.cuda().train()
    masks = {str(k): [fx[f"mask.{i}.{j}"] for j in range(int(fx["mask_counts"][i]))] for i, k in enumerate(fx["mask_names"])}
    draws = dict(ts=fx["ts"], noise=fx["noise"], perms=[list(p) for p in fx["perms"]], masks=masks)
    counter.take()
    model({k: torch.as_tensor(fx[k]).cuda() for k in ("coord", "grid_coord", "feat", "offset", "segment")}, draws=draws)["loss"].backward()
    torch.cuda.synchronize()
    return infer, counter.take()
