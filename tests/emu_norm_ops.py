"""TEST INFRASTRUCTURE: the PyTorch-CPU emulation of the ops of cdsegnet_amd/csrc/norm.hip (train-mode BatchNorm + GELU, the
pooling maximum with its arg-max), same signatures as cdsegnet_amd.ops; everything else is tests/emu_rows_ops.py's (tests/emu_ops.py and the contiguous-run sum
the deterministic training mode needs).  Tests set
``cdsegnet_amd.train_graph.ops`` (and ``engine.ops``) to this module.  Never imported by the product."""
import math

import torch
import torch.nn.functional as F

from cdsegnet_amd._lib import CdsegError
from tests import colsum_rule, emu_rows_ops


def __getattr__(name):  # every op this file does not define
    return getattr(emu_rows_ops, name)


def bn_partition(m, c):
    """The launch rule of csrc/norm.hip restated (tests/colsum_rule.py: at most 256 blocks of at least 256 rows, a multiple of 64
    beyond that); like the library, only for the kernels' widths (multiples of 16 up to 512) and m >= 0."""
    if m < 0 or c < 16 or c > 512 or c % 16:
        raise CdsegError(f"bn_partition failed: no kernel for ({m}, {c})")
    return colsum_rule.partition(m, colsum_rule.MIN_ROWS_BN)


def bn_stats(x):
    xd = x.detach().double()
    return torch.cat([xd.sum(0), (xd * xd).sum(0), torch.tensor([float(x.shape[0])], dtype=torch.float64)])


def bn_finish(stats, eps, momentum, running_mean=None, running_var=None):
    c = (stats.numel() - 1) // 2
    n = stats[2 * c]
    mu = stats[:c] / n
    var = (stats[c:2 * c] / n - mu * mu).clamp(min=0.0)
    if running_mean is not None:
        running_mean.copy_(((1.0 - momentum) * running_mean.double() + momentum * mu).float())
    if running_var is not None:
        unbiased = var * (n / (n - 1.0)) if float(n) > 1.0 else var
        running_var.copy_(((1.0 - momentum) * running_var.double() + momentum * unbiased).float())
    return mu.float(), (1.0 / torch.sqrt(var + eps)).float()


def _z(x, mean, invstd, gamma, beta):
    xh = (x - mean) * invstd
    return xh, gamma.detach() * xh + beta.detach()


def bn_gelu_fwd(x, mean, invstd, gamma, beta, out=None):
    y = F.gelu(_z(x.detach(), mean, invstd, gamma, beta)[1])
    if out is not None:
        out.copy_(y)
        return out
    return y


def bn_gelu_bwd(x, dy, mean, invstd, gamma, beta, count, hook=None, out=None):
    c = x.shape[1]
    xh, z = _z(x.detach(), mean, invstd, gamma, beta)
    g = dy * (0.5 * (1.0 + torch.erf(z * math.sqrt(0.5))) + z * torch.exp(-0.5 * z * z) * (1.0 / math.sqrt(2.0 * math.pi)))
    gsums = torch.cat([g.double().sum(0), (g.double() * xh.double()).sum(0)])
    total = gsums if hook is None else hook(gsums)
    n = count.reshape(-1)[0]
    k1, k2 = (total[:c] / n).float(), (total[c:] / n).float()
    dx = (gamma.detach() * invstd) * ((g - k1) - xh * k2)
    if out is not None:
        out.copy_(dx)
        dx = out
    return dx, gsums


def segment_max_arg(y, seg_start, m):
    seg = seg_start[:m + 1].long()
    cl = torch.repeat_interleave(torch.arange(m), seg[1:] - seg[:-1])
    n, c = y.shape
    out = torch.full((m, c), -math.inf).scatter_reduce(0, cl[:, None].expand(n, c), y, "amax")
    rows = torch.arange(n)[:, None].expand(n, c)
    cand = torch.where(y == out[cl], rows, torch.full_like(rows, n))
    arg = torch.full((m, c), n, dtype=torch.long).scatter_reduce(0, cl[:, None].expand(n, c), cand, "amin")
    arg[arg == n] = -1
    return out, arg.int()


def segment_max_bwd(dout, arg, cluster):
    cl = cluster.long()
    rows = torch.arange(cl.numel(), dtype=torch.int32)[:, None]
    return torch.where(arg[cl] == rows, dout[cl], torch.zeros((), dtype=dout.dtype))
