"""TEST INFRASTRUCTURE: what the PyTorch-CPU emulation of the op layer (tests/emu_ops.py, tests/emu_rows_ops.py) lacks for the
Feature Fusion Module options: the gate of a CrossBlock, forward and backward (cdsegnet_amd.ops.fuse_gate_fwd / _bwd), with the
kernels' arithmetic - fp64 from the fp32 operands, one rounding per output, fp64 column sums.  Every other op is
tests/emu_rows_ops.py's.  Tests set ``cdsegnet_amd.train_graph.ops`` and ``engine.ops`` to this module.  Never imported by the
product."""
import torch

from cdsegnet_amd._lib import CdsegError
from tests import emu_rows_ops


def __getattr__(name):  # every op this file does not define
    return getattr(emu_rows_ops, name)


def fuse_gate_fwd(s, a, alpha, gamma, m=None, out=None):
    if a is None and m is not None:  # (cdseg_fuse_gate_fwd: CDSEG_ERR_ARG before any launch)
        raise CdsegError("fuse_gate_fwd failed: DropPath factors without the attention operand")
    y = alpha.double() * s.double()
    if a is not None:
        mm = 1.0 if m is None else m.double().reshape(-1, 1)
        y = y + gamma.double() * mm * a.double()
    y = y.float()
    if out is not None:
        out.copy_(y)
        return out
    return y


def fuse_gate_bwd(dy, s, a, alpha, gamma, m=None):
    d = dy.double()
    dm = d if m is None else d * m.double().reshape(-1, 1)
    ds = (alpha.double() * d).float()
    da = (gamma.double() * dm).float()
    sums = torch.cat([(dm * a.double()).sum(0), (d * s.double()).sum(0)])
    return ds, da, sums
