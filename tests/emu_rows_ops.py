"""TEST INFRASTRUCTURE: what the PyTorch-CPU emulation of the op layer (tests/emu_ops.py) lacks for the row level of a Mix3D
batch (`model.train_mix3d = "rows"`, cdsegnet_amd.engine.RowLevel): the contiguous-run sum behind `_GatherRuns`.  Every
other op is tests/emu_ops.py's.  Tests set ``cdsegnet_amd.train_graph.ops`` and ``engine.ops`` to this module.  Never
imported by the product."""
import torch

from tests import emu_ops


def __getattr__(name):  # every op this file does not define
    return getattr(emu_ops, name)


def segment_sum(src, seg_start, m):
    """out[j] = src[seg_start[j]] + ... + src[seg_start[j + 1] - 1], added in ascending row order."""
    seg = seg_start[:m + 1].long()
    out = torch.zeros((m, src.shape[1]), dtype=torch.float32)
    length = seg[1:] - seg[:-1]
    for k in range(int(length.max()) if m else 0):
        has = length > k
        out[has] = out[has] + src[seg[:-1][has] + k]
    return out
