"""TEST INFRASTRUCTURE: what the PyTorch-CPU emulation of the op layer lacks for the skip-connection options: the three calls
of csrc/skip.hip (cdsegnet_amd.ops.skip_stats / skip_fold / skip_merge) with the kernels' arithmetic - fp64 from the stored
operands, one rounding per output - through tests/skip_restatement.py.  Every other op is tests/emu_fusion_ops.py's.  `calls`
logs (name, details) of every call of the three.  Tests set ``cdsegnet_amd.train_graph.ops`` and ``engine.ops`` to this module.
Never imported by the product."""
import torch

from tests import emu_fusion_ops, skip_restatement as R

calls = []


def __getattr__(name):  # every op this file does not define
    return getattr(emu_fusion_ops, name)


def skip_stats(x, ref_of_row=None, n_total=None):
    calls.append(("skip_stats", dict(n=x.shape[0], c=x.shape[1], dtype=x.dtype, ref=ref_of_row, n_total=n_total)))
    return R.stats(x, ref_of_row, n_total)


def skip_fold(w, stats):
    calls.append(("skip_fold", dict(shape=tuple(w.shape))))
    return (stats.view(3, -1) @ w.double().t()).reshape(-1)


def skip_merge(x, stats=None, s=1.0, f=1.0, ref_of_row=None, n_total=None, child=None, cluster=None, folded=False):
    calls.append(("skip_merge", dict(n=x.shape[0], c=x.shape[1], stats=stats is not None, s=s, f=f, ref=ref_of_row,
                                     n_total=n_total, child=child is not None, folded=folded)))
    assert x.dtype == torch.float32
    x.copy_(R.merge(x, stats, s, f, ref_of_row, n_total, child, cluster, folded).float())
    return x
