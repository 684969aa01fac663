"""TEST INFRASTRUCTURE: what the PyTorch-CPU emulation of the op layer (tests/emu_ops.py) lacks for attention and projection
dropout (`attn_drop`, `proj_drop`): the three dropout ops and `dropout_keep`, with the library's masks as tests/dropout_mask.py
restates them from include/cdseg.h.  Every other op is tests/emu_ops.py's.  Tests set ``cdsegnet_amd.train_graph.ops`` and
``engine.ops`` to this module.  Never imported by the product."""
import numpy as np
import torch

from tests import dropout_mask as DM
from tests import emu_ops


def __getattr__(name):  # every op this file does not define
    return getattr(emu_ops, name)


def dropout_keep(rate):
    return DM.keep_prob(rate)


def _patch_attention_drop(qq, kk, vv, ps, num_heads, scale, rate, seed, offset):
    """softmax over all keys, then (M / keep) o P, per patch and head, on slot-ordered rows (differentiable)."""
    lens = np.diff(ps).tolist()
    masks = DM.attention_mask(seed, offset, rate, lens, num_heads)
    f = float(DM.inv_keep(rate))
    out = []
    for p, L in enumerate(lens):
        a, b = int(ps[p]), int(ps[p + 1])
        heads = []
        for h in range(num_heads):
            sl = slice(16 * h, 16 * h + 16)
            prob = torch.softmax(scale * (qq[a:b, sl] @ kk[a:b, sl].T), dim=1)
            heads.append((prob * (torch.as_tensor(masks[p][h], dtype=prob.dtype) * f)) @ vv[a:b, sl])
        out.append(torch.cat(heads, 1))
    return torch.cat(out, 0)


def attention_drop(q, k, v, q_gidx, kv_gidx, widx, patch_start, num_heads, max_len, scale, out, rate, seed, offset):
    ps = patch_start.numpy().astype(np.int64)
    assert int(np.diff(ps).max()) == max_len
    o = _patch_attention_drop(q.float()[q_gidx.long()], k.float()[kv_gidx.long()], v.float()[kv_gidx.long()], ps, num_heads, scale,
                              rate, seed, offset)
    m = widx >= 0
    out[widx[m].long()] = o[m].to(out.dtype)
    return out


def attention_drop_bwd(q, k, v, q_gidx, kv_gidx, widx, patch_start, patch_start_host, num_heads, scale, dout, dq, dk, dv, rate,
                       seed, offset):
    ps = np.asarray(patch_start_host, dtype=np.int64)
    with torch.enable_grad():
        qq, kk, vv = (t.detach().clone().float().requires_grad_(True) for t in (q, k, v))
        o = _patch_attention_drop(qq[q_gidx.long()], kk[kv_gidx.long()], vv[kv_gidx.long()], ps, num_heads, scale, rate, seed, offset)
        m = widx >= 0
        full = torch.zeros_like(dout).index_put((widx[m].long(),), o[m])
        (full * dout).sum().backward()
    dq += qq.grad
    dk += kk.grad
    dv += vv.grad


def dropout(x, rate, seed, offset, out=None):
    mask = torch.as_tensor(DM.element_mask(seed, offset, rate, x.shape[0], x.shape[1]))
    y = torch.where(mask, x * float(DM.inv_keep(rate)), torch.zeros((), dtype=x.dtype))
    if out is None:
        return y
    out.copy_(y)
    return out
