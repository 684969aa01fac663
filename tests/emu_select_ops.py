"""TEST INFRASTRUCTURE: what the PyTorch-CPU emulation of the op layer (tests/emu_ops.py) lacks for test-time voting on shared
geometry (cdsegnet_amd.engine: Level.slots on a tuple of curves, per-fragment device noise): the element-wise composition of
slot plans behind cdseg_slots_select.  Every other op is tests/emu_ops.py's (`randn` into a row slice among them).  Tests set
``cdsegnet_amd.engine.ops`` to this module.  Never imported by the product."""
import torch

from tests import emu_ops


def __getattr__(name):  # every op this file does not define
    return getattr(emu_ops, name)


def slots_select(sources, offs_pad, choice, n_pad):
    """out[s] = sources[choice[b]][s] for every padded slot s of batch element b (offs_pad[b] <= s < offs_pad[b + 1])."""
    offs_pad = [int(v) for v in offs_pad.tolist()]
    assert len(choice) == len(offs_pad) - 1 and offs_pad[-1] == n_pad
    gidx = torch.empty(n_pad, dtype=torch.int32)
    widx = torch.empty(n_pad, dtype=torch.int32)
    for b, c in enumerate(choice):
        a, e = offs_pad[b], offs_pad[b + 1]
        assert sources[c] is not None, "a chosen source must exist"
        gidx[a:e], widx[a:e] = sources[c][0][a:e], sources[c][1][a:e]
    return gidx, widx
