"""TEST INFRASTRUCTURE: the PyTorch-CPU emulation of the native training Block (cdsegnet_amd/csrc/trainblock.hip), same
signatures as cdsegnet_amd.ops: `TrainBlock`, `train_block_bytes` / `_prepare` / `_forward` / `_backward`, the gradient views
and the row kernels.  The executor's launch sequence is restated on the emulated primitives of tests/emu_ops.py (and
tests/emu_norm_ops.py), so the autograd wiring of `train_graph._NativeBlock` can run without a device.  Tests set
``cdsegnet_amd.train_graph.ops`` (and ``engine.ops``) to this module.  Never imported by the product."""
import torch
import torch.nn.functional as F

from tests import emu_norm_ops as E

TB_PARAMS = 18
TB_MATRICES = (0, 2, 8, 10, 14, 16)
_TAPES = {}  # tape.data_ptr() -> what the emulated forward kept (the tape tensor itself carries no data here)


def __getattr__(name):  # every op this file does not define
    return getattr(E, name)


def _a256(v):
    return (int(v) + 255) // 256 * 256


class TrainBlock:
    def __init__(self, params, heads, attn_scale, eps, mm_variant, attn_variant, deterministic, shadows=None):
        assert len(params) == TB_PARAMS
        self.params, self.heads, self.scale, self.eps = list(params), int(heads), float(attn_scale), tuple(eps)
        self.variant = mm_variant or attn_variant
        self.mm_lp, self.attn_lp, self.deterministic = mm_variant is not None, attn_variant is not None, bool(deterministic)
        self.shadows = [None] * 6 if shadows is None else list(shadows)
        self.channels, self.hidden = params[2].shape[0], params[14].shape[0]
        self.derived = None
        self.prepared = 0
        off, self.grad_offsets = 0, []
        for p in self.params:
            self.grad_offsets.append(off)
            off = _a256(off + 4 * p.numel())
        self.grad_bytes = off

    def t16(self):
        return E.LP_DTYPES[self.variant]


def train_block_bytes(tb, n, slots):
    c, h = tb.channels, tb.hidden
    wide = max(3 * c, h)
    return _a256(4 * n * (7 * c + 2 * h)), _a256(10 * n * wide + 12 * slots * tb.heads), _a256(8 * (27 * c * c + 5 * c * c + 2 * c * h)), tb.grad_bytes


def train_block_grad_views(tb, slab):
    return [slab[off:off + 4 * p.numel()].view(torch.float32).view(p.shape) for p, off in zip(tb.params, tb.grad_offsets)]


def _mm(tb, t):
    return t.to(tb.t16()) if tb.mm_lp else t


def train_block_prepare(tb):
    """Transposed Linear weights, the conv's data-gradient kernel W'[ci][o][co] = W[co][26 - o][ci], and the 16-bit forward
    weights where the optimizer keeps no copy."""
    c = tb.channels
    d = {"w": [], "t": []}
    for j, i in enumerate(TB_MATRICES):
        src = tb.shadows[j] if (tb.mm_lp and tb.shadows[j] is not None) else _mm(tb, tb.params[i].detach())
        if i == 0:
            w3 = src.reshape(c, 27, c)
            d["w"].append(w3.reshape(c, 27 * c))
            d["t"].append(w3.flip(1).permute(2, 1, 0).contiguous().view(c, 27 * c))
        else:
            d["w"].append(src)
            d["t"].append(src.t().contiguous())
    tb.derived = d
    tb.prepared += 1


def _lin(tb, x, j, out_dtype=torch.float32, nbr=None):
    w = tb.derived["w"][j]
    out = torch.empty((x.shape[0], w.shape[0]), dtype=out_dtype)
    kw = dict(nbr=nbr, kvol=27, nbr_kmajor=True) if nbr is not None else {}
    return E.gemm(x, w, out, bias=tb.params[TB_MATRICES[j] + 1].detach(), **kw)


def _dgrad(tb, dy, j, nbr=None):
    wt = tb.derived["t"][j]
    out = torch.empty((dy.shape[0], wt.shape[0]), dtype=torch.float32)
    kw = dict(nbr=nbr, kvol=27, nbr_kmajor=True) if nbr is not None else {}
    return E.gemm(dy, wt, out, **kw)


def residual(x, a=None, mask=None, t_rows=None, scene_offs=None, out=None):
    v = x
    if a is not None:
        v = v + (a if mask is None else a * mask[:, None])
    if t_rows is not None:
        offs = scene_offs.long()
        v = v + t_rows[torch.repeat_interleave(torch.arange(t_rows.shape[0]), offs[1:] - offs[:-1])]
    if out is None:
        return v.clone() if v is x else v
    out.copy_(v)
    return out


def scale_cast(dy, mask=None, variant=None):
    v = dy if mask is None else dy * mask[:, None]
    return v.clone() if variant is None else v.to(E.LP_DTYPES[variant])


def add_layernorm(x, a, mask, gamma, beta, eps=1e-5, variant=None):
    x1 = x + (a if mask is None else a * mask[:, None])
    h = F.layer_norm(x1, (x.shape[1],), gamma, beta, eps)
    return x1, (h if variant is None else E.cast(h, E.LP_DTYPES[variant]))


def gelu_fwd(u, variant=None):
    g = F.gelu(u)
    return g if variant is None else E.cast(g, E.LP_DTYPES[variant])


def gelu_bwd_cast(u, dg, variant=None):
    du = E.gelu_bwd(u, dg)
    return du if variant is None else du.to(E.LP_DTYPES[variant])


def train_block_forward(tb, n, x_in, x_conv, t_rows, scene_offs, mask1, mask2, nbr, gidx, widx, patch_start, patch_start_host,
                        tape, scratch, x_out, rows=None):
    """rows = (row_vox (n), row_start (V + 1)): the row level of a Mix3D batch, as in csrc/trainblock.hip - the CPE (conv, Linear,
    LayerNorm) runs on the first row of every voxel with `nbr` over the V voxels, and every row adds its voxel's term."""
    assert tb.derived is not None, "train_block_prepare has not run"
    P = [p.detach() for p in tb.params]
    c = tb.channels
    mmv = tb.variant if tb.mm_lp else None
    T = {}
    xv = x_conv if rows is None else x_conv[rows[1][:-1].long()]  # gather_first
    T["xc"] = E.cast(xv, tb.t16()) if tb.mm_lp else xv
    T["yc"] = _lin(tb, T["xc"], 0, T["xc"].dtype, nbr=nbr)
    T["z"] = _lin(tb, T["yc"], 1)
    x0 = torch.empty_like(x_in)
    if rows is None:
        E.layernorm(T["z"], P[4], P[5], x0, eps=tb.eps[0], res=x_in)
    else:  # residual_rows: x + LN(z)[row_vox], then the timestep row below
        pe = torch.empty_like(T["z"])
        E.layernorm(T["z"], P[4], P[5], pe, eps=tb.eps[0])
        x0.copy_(x_in + pe[rows[0].long()])
    if t_rows is not None:
        residual(x0, None, None, t_rows, scene_offs, out=x0)
    T["x0"] = x0
    T["h1"] = torch.empty(x0.shape, dtype=T["xc"].dtype)
    E.layernorm(x0, P[6], P[7], T["h1"], eps=tb.eps[1])
    T["qkv"] = _lin(tb, T["h1"], 2, tb.t16() if tb.attn_lp else torch.float32)
    q = T["qkv"]
    o = torch.zeros((n, c), dtype=q.dtype)
    max_len = max(b - a for a, b in zip(patch_start_host[:-1], patch_start_host[1:]))
    E.attention(q[:, :c], q[:, c:2 * c], q[:, 2 * c:], gidx, gidx, widx, patch_start, tb.heads, max_len, tb.scale, o)
    T["o"] = o if tb.attn_lp == tb.mm_lp else (E.cast(o, tb.t16()) if tb.mm_lp else o.float())
    a = _lin(tb, T["o"], 3)
    T["x1"], T["h2"] = add_layernorm(x0, a, mask1, P[12], P[13], tb.eps[2], mmv)
    T["u"] = _lin(tb, T["h2"], 4)
    T["g"] = gelu_fwd(T["u"], mmv)
    hm = _lin(tb, T["g"], 5)
    residual(T["x1"], hm, mask2, out=x_out)
    _TAPES[tape.data_ptr()] = T
    return x_out


def train_block_backward(tb, n, x_in, x_conv, t_rows, scene_offs, mask1, mask2, nbr, gidx, widx, patch_start, patch_start_host,
                         tape, scratch, x_out, dy, dx_in, dx_conv, dt_rows, slab, rows=None):
    T = _TAPES[tape.data_ptr()]
    P = [p.detach() for p in tb.params]
    c = tb.channels
    mmv = tb.variant if tb.mm_lp else None
    slab.zero_()
    det = {"deterministic": True} if tb.deterministic else {}  # the fixed-order reductions, asked for as ops.det_kw does
    G = train_block_grad_views(tb, slab)
    op = (lambda t: t.to(tb.t16())) if tb.mm_lp else (lambda t: t)
    dhm = scale_cast(dy, mask2, mmv)
    E.linear_wgrad(T["g"].float(), dhm.float(), G[16], G[17], **det)
    du = gelu_bwd_cast(T["u"], _dgrad(tb, dhm, 5), mmv)
    E.linear_wgrad(T["h2"].float(), du.float(), G[14], G[15], **det)
    dh2 = _dgrad(tb, du, 4)
    dx_in.copy_(dy)
    E.layernorm_bwd(T["x1"], P[12], dh2, dx_in, accumulate=True, eps=tb.eps[2], dgamma=G[12], dbeta=G[13], **det)
    da = scale_cast(dx_in, mask1, mmv)
    E.linear_wgrad(T["o"].float(), da.float(), G[10], G[11], **det)
    do = _dgrad(tb, da, 3)
    if tb.attn_lp:
        do = do.to(tb.t16())
    dqkv = torch.zeros((n, 3 * c), dtype=torch.float32)
    q = T["qkv"]
    E.attention_bwd(q[:, :c], q[:, c:2 * c], q[:, 2 * c:], gidx, gidx, widx, patch_start, patch_start_host, tb.heads, tb.scale,
                    do.float(), dqkv[:, :c], dqkv[:, c:2 * c], dqkv[:, 2 * c:])
    dq = op(dqkv)
    E.linear_wgrad(T["h1"].float(), dq.float(), G[8], G[9], **det)
    dh1 = _dgrad(tb, dq, 2)
    E.layernorm_bwd(T["x0"], P[6], dh1, dx_in, accumulate=True, eps=tb.eps[1], dgamma=G[6], dbeta=G[7], **det)
    if t_rows is not None:
        offs = [int(v) for v in scene_offs]
        dt_rows.copy_(torch.stack([dx_in[offs[b]:offs[b + 1]].sum(0) for b in range(len(offs) - 1)]))
    dpe = dx_in
    if rows is not None:  # run_sum: a voxel's term collects the gradients of its rows, in ascending row order
        rs = [int(v) for v in rows[1]]
        dpe = torch.zeros((len(rs) - 1, c), dtype=torch.float32)
        for v in range(len(rs) - 1):
            for i in range(rs[v], rs[v + 1]):
                dpe[v] += dx_in[i]
    dz = torch.empty_like(dpe)
    E.layernorm_bwd(T["z"], P[4], dpe, dz, accumulate=False, eps=tb.eps[0], dgamma=G[4], dbeta=G[5], **det)
    dz = op(dz)
    E.linear_wgrad(T["yc"].float(), dz.float(), G[2], G[3], **det)
    dyc = op(_dgrad(tb, dz, 1))
    E.conv_wgrad(T["xc"].float(), nbr, dyc.float(), G[0].view(c, 27, c), G[1], **det)
    dxc = _dgrad(tb, dyc, 0, nbr=nbr)
    if rows is not None:  # scatter_first: the conv read the first row of every voxel only
        first = rows[1][:-1].long()
        if dx_conv is None:
            dx_in[first] += dxc
        else:
            dx_conv.zero_()
            dx_conv[first] = dxc
    elif dx_conv is None:
        dx_in += dxc
    else:
        dx_conv.copy_(dxc)
