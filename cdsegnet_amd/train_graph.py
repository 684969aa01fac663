"""Training forward of the model under torch autograd, on the HIP kernels (training row of SURVEY 8(f4)).

ref: pointcept/models/default.py:424-493 (DefaultSegmentorV2.forward: per-scene timestep, q_sample of the conditioning
target, both branches and BOTH decoders, the criteria) and pointcept/engines/train.py:216-271 (run_step:
`loss = model(input_dict)["loss"]; loss.backward(); optimizer.step()`).  The reference's training step is torch autograd
over torch ops plus three extension ops with hand-written backward passes (spconv.SubMConv3d, flash_attn,
torch_scatter.segment_csr).  The same boundary here: `DefaultSegmentorV2.forward` returns `dict(loss=...)` whose
`.backward()` fills the `.grad` of the model's own nn.Parameters, so `torch.optim.AdamW` and the reference trainer work
unchanged - and underneath, every product that carries the FLOPs runs on this library's kernels behind
`torch.autograd.Function`s:

    sparse conv (k = 3 CPE convs, k = 5 stems)   forward  cdseg_gemm (gathered form)
                                                 backward cdseg_conv_wgrad (all offsets, one launch) + the data gradient as
                                                          the SAME gathered GEMM on the mirrored, transposed kernel
    Linear (qkv, proj, fc1, fc2, CPE, pool / unpool projections)      cdseg_gemm / cdseg_gemm on W^T / cdseg_linear_wgrad
    LayerNorm                                    cdseg_layernorm / cdseg_layernorm_bwd
    serialized (cross) attention                 cdseg_attention / cdseg_attention_bwd (recompute-P, gathered rows)
    segment max of the pooling                   cdseg_segment_max forward; the arg-max mask is recomputed in the backward
                                                 (train_norm "fused": cdseg_segment_max_arg / cdseg_segment_max_bwd)
    train-mode BatchNorm1d -> GELU               torch device ops by default; train_norm "fused": cdseg_bn_stats / _finish /
                                                 cdseg_bn_gelu_fwd, backward cdseg_bn_gelu_bwd_sums / _dx (csrc/norm.hip)

in exact fp32 by default.  The reference never runs its attention core in fp32 on a GPU (`qkv.half()` into flash-attention,
whose backward is half too): `model.train_precision = "fp16-attn"` / `"bf16-attn"` runs the attention core of every Block
and of the cross attention in 16 bits - the inference path's 16-bit forward kernel and the recompute-P backward on the 16-bit
matrix pipe (csrc/train.hip), fp32 dq / dk / dv - and leaves everything else in fp32.
`"fp16-amp"` / `"bf16-amp"` is the reference's AMP setting (`enable_amp = True`: torch.cuda.amp.autocast around the model,
engines/train.py:226-240): the same attention core, and every trunk Linear and sparse conv as `_Linear16` / `_SubMConv16` -
input and weight rounded once to the 16-bit type, forward and data gradient by cdseg_gemm on 16-bit operands, the weight
gradient by cdseg_linear_wgrad16 / cdseg_conv_wgrad16, fp32 accumulation throughout, the 16-bit input saved for the backward,
dy cast without saturation so that a GradScaler sees an overflow.  The residual stream, LayerNorm, GELU, BatchNorm sites,
heads, timestep MLP, criteria, parameters and .grad stay fp32.  ONE difference from torch autocast: autocast also rounds each
Linear's OUTPUT to fp16; here the outputs stay fp32 (operand rounding and fp32 accumulation are the same).  What stays plain torch device ops: the swish timestep MLP on B rows, row masks of
stochastic depth, q_sample, the two (C -> classes) heads, the criteria (cdsegnet_amd.losses) - and, in the default
`train_norm = "torch"`, train-mode BatchNorm1d (3 per pooling stage, batch statistics) with the GELU behind it.  All integer work - serialization, pooling structure,
kernel maps, padded patch plans - is the inference engine's plan (Engine.build_plan), shared with the inference path.

Deterministic mode (`model.train_deterministic`: None = follow torch.are_deterministic_algorithms_enabled(), True / False
override; resolved once per forward).  The forward is a function of the seed either way (timesteps, noise and order shuffles
from torch's CPU generator, stochastic-depth masks from the device generator, the plan is integer work) and is NOT changed by
the mode.  What the mode changes are the backward reductions that otherwise leave through fp32 atomics in arrival order:
    weight gradients of every Linear / sparse conv   ops.linear_wgrad / ops.conv_wgrad(deterministic=True): split partials in a
                                                     workspace, added by ascending split index (ops.wgrad_partition)
    LayerNorm dgamma / dbeta                         ops.layernorm_bwd(deterministic=True): block partials, ascending block index
    unpooling gather child[cluster]                  `_GatherRuns`: backward = ops.segment_sum over the contiguous children
    Mix3D fold point[k][rep]                         `_GatherRuns` after a stable sort of rep
Everything else on the step is already order-fixed: the permutation gathers (perm0, inv0, ref_order) have unique indices;
`_SceneRows` sums contiguous rows and `_SegmentMax` selects one child, neither with atomics; the attention backward adds at most
two values onto a zeroed element (a row sits in at most two slots), which commutes; cdseg_gemm's split-K has no atomics;
train-mode BatchNorm (default `train_norm`) and the criteria are torch ops that are deterministic or raise / warn under torch's
flag; with `train_norm = "fused"` the BatchNorm statistics and backward sums are fp64 sums in an order fixed by the shape.  Limit: the two
(C -> classes) heads and the timestep MLP are torch GEMMs (rocBLAS), which torch pins to atomic-free kernels only under
torch.use_deterministic_algorithms(True); `train_deterministic = True` alone does not reach into them.

Fused loss (`model.train_loss = "fused"`, default "torch"; read at every forward): the cross-entropy and Lovasz terms of the
criteria, forward and backward, on the kernels of csrc/loss.hip (losses.FusedCriteria -> ops.seg_loss / ops.seg_loss_bwd) instead
of torch's per-class sort loop.  Its sums run in a fixed order whatever `train_deterministic` says, and the Lovasz sort breaks
ties by ascending row index, where torch's unstable sort leaves the order (and with it the gradient of tied rows) open.

Fused norm sites (`model.train_norm = "fused"`, default "torch"; read at every forward): every train-mode BatchNorm1d -> GELU
site (stems, SerializedPooling.norm, both projections of SerializedUnpooling: 20 in the conditional model) runs as `_BnGelu` on
the kernels of csrc/norm.hip - per-channel sum x / sum x^2 in fp64 by row blocks whose partials are added by ascending block
index, one normalise + GELU pass, and a backward that recomputes z from x (saved: x, mean, invstd; no BatchNorm output) in two
passes: the fp64 sums of g and g x_hat, then dx.  The pooling maximum keeps its arg-max (`_SegmentMaxArg`: the first maximal
child, torch_scatter's rule) and its backward is one launch.  nn.SyncBatchNorm modules (the reference trainer's
convert_sync_batchnorm under cfg.sync_bn, engines/train.py:275-276) get statistics over all ranks of their process group: one
all_gather of the (2 c + 1) fp64 buffer in the forward and one of the (2 c) sums in the backward, each added in rank order
(`gather_ranks`); dgamma / dbeta stay this rank's sums, averaged with every other gradient by dist.GradSync.  In the default
mode such modules normalise with this rank's rows only, and say so once.  Eval mode, widths that are no multiple of 16 up to
512, momentum = None and modules without affine parameters take the torch path in either mode; a CPU tensor in the fused mode
raises like every other op of the library.  These sites are fp32 in every train_precision.

Dropout (`attn_drop`, `proj_drop` of the backbone; train mode, rate > 0 only - otherwise no node is added): `_AttentionDrop` /
`_AttentionDrop16` in the attention core's place, `_Dropout` behind `proj`, behind the MLP's GELU and behind `fc2`.  A site is (seed,
offset) of the library's mask stream (include/cdseg.h "dropout"): seed = torch.initial_seed(), offset = the next value of a counter on
the TrainGraph that restarts when a forward finds another seed than the forward before; `draws["dropout"] = (seed, first offset)` pins a
forward; `TrainGraph.dropout_sites` lists the sites of the last one.  Under `train_block = "native"` a Block with a rate runs as its
autograd chain (one warning per process).

Native Blocks (`model.train_block = "native"`, default "autograd"; read at every forward): every Block of both branches is ONE
autograd node, `_NativeBlock`, whose forward and backward are one library call each (csrc/trainblock.hip: ops.train_block_forward /
_backward): the same products through the same entry points, the torch glue between them (residual adds, stochastic-depth
multiplies, GELU, the timestep rows, gradient zero fills, weight transposes, the fp32 round trips of the AMP path) as HIP row
kernels, the derived weights of a Block made once per weight version (ops.train_block_prepare).  The CrossBlock, pooling,
unpooling, stems, heads and criteria are what they are in the default mode, which is unchanged bit for bit.

Fusion module options (`tm_feat` a learned scale, `tm_bidirectional`; constructor options of the backbone): a learned gate is ONE
node, `_FuseGate`, over the two kernels of csrc/fusion.hip (`feat_scale` gets its gradient from the backward's two fp64 column sums,
`gate_dp`; fixed summation order in every mode); a bidirectional model runs `cross_block1` (c <- n) in front of `cross_block2`, with
the reference's in-place assignments: the n point enters `cross_block2` holding cross_block1's kv_norm1 output.  A numeric `tm_feat`
without `tm_bidirectional` is the graph it was, bit for bit.  The cross blocks stay autograd nodes under `train_block = "native"`.

Mix3D batches (`model.train_mix3d = "rows"`, default "fold"; read at every forward; no effect on a batch without shared
voxels): a batch element made of two merged scenes has voxels that hold several points.  "fold" runs the network on the first
point of every voxel and copies its prediction to the others.  "rows" keeps every point as a row - serialization, attention,
BatchNorm statistics, stochastic depth, pooling, heads, loss - on an `engine.RowLevel` above the plan of the unique voxels; the
sparse convs (stems, the CPE of the level-0 Blocks, the stale conv input behind the last unpooling) take the voxel as their
unit: conv(x)[i] = conv_V(x[first])[vox(i)] with today's kernel map, first = the voxel's first point in the caller's order
(`_conv`, `_spread`; the native Block does the same inside its two calls).  `TrainGraph.last_shared` = (N, V) of the last forward.
"""
import warnings

import torch
import torch.nn.functional as F

from . import engine as _engine
from . import _lib
from ._lib import DuplicateVoxelsError
from . import ops
from .ops import det_kw as _det_kw  # (by name: tests swap `ops` for the CPU emulation, which has no such helper)
from . import ops as _alloc  # (the allocator of the Block's tape / scratch / gradient slab: never the emulation's; looked up per call)
from .losses import TRAIN_LOSSES, build_criteria
from .optim import shadow16 as _shadow16
from .models import FUSION_MODES as _FUSION_MODES, gate_vectors


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def _f32(shape, like):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


def resolve_deterministic(model):
    """model.train_deterministic: None = torch.are_deterministic_algorithms_enabled(), True / False override."""
    d = getattr(model, "train_deterministic", None)
    if d is None:
        return bool(torch.are_deterministic_algorithms_enabled())
    if not isinstance(d, bool):
        raise ValueError(f"train_deterministic must be None, True or False, not {d!r}")
    return d


# ------------------------------------------------------------------------------------------ autograd functions
class _GatherRuns(torch.autograd.Function):
    """y = x[idx] where the rows that read the same source row form one contiguous run (deterministic mode): seg (m + 1) int32
    are the run starts - directly for the unpooling gather child[cluster] (the children of a pooled row are contiguous in the
    plan's physical order: the seg of `_SegmentMax`), or of the rows taken in the order `perm` (the Mix3D fold: a stable sort
    of rep).  The backward adds a run's rows in ascending order (ops.segment_sum) where torch's index backward uses atomics."""

    @staticmethod
    def forward(ctx, x, idx, seg, perm):
        ctx.save_for_backward(seg, perm) if perm is not None else ctx.save_for_backward(seg)
        ctx.m = x.shape[0]
        return x[idx]

    @staticmethod
    def backward(ctx, dy):
        seg = ctx.saved_tensors[0]
        dy = dy.float()
        if len(ctx.saved_tensors) > 1:
            dy = dy[ctx.saved_tensors[1]]
        return ops.segment_sum(_c(dy), seg, ctx.m), None, None, None


def fold_runs(rep, m):
    """(perm, seg) for `_GatherRuns` of x[rep]: perm = stable sort of rep, seg = run starts of the sorted values (m + 1, int32)."""
    perm = torch.sort(rep, stable=True).indices
    seg = torch.zeros(m + 1, dtype=torch.int32, device=rep.device)
    seg[1:] = torch.bincount(rep, minlength=m).cumsum(0).to(torch.int32)
    return perm, seg


class _SubMConv(torch.autograd.Function):
    """y = bias + sum_o W_o x[nbr[o]] (spconv.SubMConv3d; ref call sites ptv3.py:356, 647, 1106, 1118)."""

    @staticmethod
    def forward(ctx, x, w5, b, nbr, det=False):
        cout, cin = w5.shape[0], w5.shape[-1]
        kvol = nbr.shape[0]
        cp = (cin + 15) // 16 * 16  # the weight-gradient kernel works on 16-channel groups (stems: 6 -> 16)
        w3 = w5.reshape(cout, kvol, cin)
        if cp != cin:
            x = F.pad(x, (0, cp - cin))
            w3 = F.pad(w3, (0, cp - cin))
        x = _c(x)
        w = _c(w3).reshape(cout, kvol * cp)
        y = _f32((x.shape[0], cout), x)
        # (a padded stem weight is a fresh tensor every step: no cache entry may pin it - ADVICE r4)
        ops.gemm(x, w, y, bias=b, nbr=nbr, kvol=kvol, nbr_kmajor=True, cache=cp == cin)
        ctx.save_for_backward(x, w, nbr)
        ctx.meta = (cin, cp, kvol, b is not None, tuple(w5.shape))
        ctx.det = _det_kw(det)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, nbr = ctx.saved_tensors
        cin, cp, kvol, has_b, wshape = ctx.meta
        cout = w.shape[0]
        dy = _c(dy)
        dw3 = torch.zeros((cout, kvol, cp), dtype=torch.float32, device=dy.device)
        db = torch.zeros(cout, dtype=torch.float32, device=dy.device) if has_b else None
        ops.conv_wgrad(x, nbr, dy, dw3, db, **ctx.det)
        dw5 = dw3[:, :, :cin].reshape(wshape)
        dx = None
        if ctx.needs_input_grad[0]:
            # submanifold map: nbr[o][i] = j  <=>  nbr[kvol - 1 - o][j] = i, so dx = conv(dy, W') on the SAME map with
            # W'[ci][o][co] = W[co][kvol - 1 - o][ci]
            wt = _c(w.view(cout, kvol, cp).flip(1).permute(2, 1, 0)).view(cp, kvol * cout)
            dxp = _f32((x.shape[0], cp), dy)
            ops.gemm(dy, wt, dxp, nbr=nbr, kvol=kvol, nbr_kmajor=True, cache=False)  # wt: a per-call temporary
            dx = dxp[:, :cin]
        return dx, dw5, db, None, None


class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, det=False):
        x, w = _c(x), _c(w)
        y = _f32((x.shape[0], w.shape[0]), x)
        ops.gemm(x, w, y, bias=b)
        ctx.save_for_backward(x, w)
        ctx.has_b = b is not None
        ctx.det = _det_kw(det)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = _c(dy)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _f32(x.shape, dy)
            ops.gemm(dy, _c(w.t()), dx, cache=False)  # the transposed copy is a per-call temporary
        dw = torch.zeros_like(w)
        db = torch.zeros(w.shape[0], dtype=torch.float32, device=dy.device) if ctx.has_b else None
        ops.linear_wgrad(x, dy, dw, db, **ctx.det)
        return dx, dw, db, None


class _SubMConv16(torch.autograd.Function):
    """_SubMConv on 16-bit products (the AMP step; ref: spconv's SubMConv3d under torch.cuda.amp.autocast, engines/train.py:
    226-240): x is cast ONCE to the 16-bit type of library build `variant` with the library's cast (saturating in the half
    build, like the inference path), the weight likewise; forward, data gradient and weight gradient are cdseg_gemm /
    cdseg_conv_wgrad16 on 16-bit operands with fp32 accumulation and fp32 outputs.  The 16-bit x is what the backward keeps.
    dy is cast WITHOUT saturation (torch's cast): a scaled gradient beyond half's range must reach the GradScaler as inf.
    The 16-bit weight copy is a per-call temporary (cache=False: no cache entry may pin it), unless an optimizer keeps a current
    copy (optim.shadow16: FusedAdamW(shadow16=...)); then w16 is a view of the optimizer's buffer, saved for the backward like
    the temporary - every such view shares one version counter, which the optimizer's step moves, so a backward that ran
    after the step that rewrote its saved copy is an autograd error, not a silent use of the new weights."""

    @staticmethod
    def forward(ctx, x, w5, b, nbr, variant, det=False):
        t16 = ops.LP_DTYPES[variant]
        cout, cin = w5.shape[0], w5.shape[-1]
        kvol = nbr.shape[0]
        cp = (cin + 15) // 16 * 16
        w3 = w5.reshape(cout, kvol, cin)
        if cp != cin:
            x = F.pad(x, (0, cp - cin))
            w3 = F.pad(w3, (0, cp - cin))
        with _lib.use(variant):
            x16 = ops.cast(_c(x), t16)
            w16 = _shadow16(w5, t16) if cp == cin else None  # the optimizer's current 16-bit copy (optim.FusedAdamW), if any
            w16 = ops.cast(_c(w3).reshape(cout, kvol * cp), t16) if w16 is None else w16.reshape(cout, kvol * cp)
            y = _f32((x.shape[0], cout), x)
            ops.gemm(x16, w16, y, bias=b, nbr=nbr, kvol=kvol, nbr_kmajor=True, cache=False)
        ctx.save_for_backward(x16, w16, nbr)
        ctx.meta = (cin, cp, kvol, b is not None, tuple(w5.shape), variant)
        ctx.det = _det_kw(det)
        return y

    @staticmethod
    def backward(ctx, dy):
        x16, w16, nbr = ctx.saved_tensors
        cin, cp, kvol, has_b, wshape, variant = ctx.meta
        cout = w16.shape[0]
        dy16 = _c(dy).to(x16.dtype)
        dw3 = torch.zeros((cout, kvol, cp), dtype=torch.float32, device=dy.device)
        db = torch.zeros(cout, dtype=torch.float32, device=dy.device) if has_b else None
        dx = None
        with _lib.use(variant):
            ops.conv_wgrad(x16, nbr, dy16, dw3, db, **ctx.det)
            if ctx.needs_input_grad[0]:
                wt = _c(w16.view(cout, kvol, cp).flip(1).permute(2, 1, 0)).view(cp, kvol * cout)
                dxp = _f32((x16.shape[0], cp), dy)
                ops.gemm(dy16, wt, dxp, nbr=nbr, kvol=kvol, nbr_kmajor=True, cache=False)
                dx = dxp[:, :cin]
        return dx, dw3[:, :, :cin].reshape(wshape), db, None, None, None


class _Linear16(torch.autograd.Function):
    """_Linear on 16-bit products (the AMP step): operands rounded once to the 16-bit type of library build `variant`, fp32
    accumulation, fp32 y / dx / dw / db; the saved input is the 16-bit copy.  See _SubMConv16 for the casts."""

    @staticmethod
    def forward(ctx, x, w, b, variant, det=False):
        t16 = ops.LP_DTYPES[variant]
        with _lib.use(variant):
            x16 = ops.cast(_c(x), t16)
            w16 = _shadow16(w, t16)  # the optimizer's current 16-bit copy (optim.FusedAdamW), if any
            if w16 is None:
                w16 = ops.cast(_c(w), t16)
            y = _f32((x.shape[0], w.shape[0]), x)
            ops.gemm(x16, w16, y, bias=b, cache=False)
        ctx.save_for_backward(x16, w16)
        ctx.meta = (b is not None, variant)
        ctx.det = _det_kw(det)
        return y

    @staticmethod
    def backward(ctx, dy):
        x16, w16 = ctx.saved_tensors
        has_b, variant = ctx.meta
        dy16 = _c(dy).to(x16.dtype)
        dx = None
        dw = torch.zeros(w16.shape, dtype=torch.float32, device=dy.device)
        db = torch.zeros(w16.shape[0], dtype=torch.float32, device=dy.device) if has_b else None
        with _lib.use(variant):
            if ctx.needs_input_grad[0]:
                dx = _f32(x16.shape, dy)
                ops.gemm(dy16, _c(w16.t()), dx, cache=False)
            ops.linear_wgrad(x16, dy16, dw, db, **ctx.det)
        return dx, dw, db, None, None


def linear(x, mod, variant=None, det=False):
    """nn.Linear on the library's GEMMs when both widths are multiples of 16 (every Linear of the trunk); the two heads
    (C -> classes / c_in) and the B-row timestep MLP are plain torch.  variant "f16" / "bf16": 16-bit products on that build
    of the library (the AMP step), None: exact fp32.  det: the weight gradient in a fixed summation order."""
    w, b = mod.weight, mod.bias
    if w.shape[0] % 16 or w.shape[1] % 16 or x.shape[0] < 1:
        return F.linear(x, w, b)
    if variant is not None:
        return _Linear16.apply(x, w, b, variant, det)
    return _Linear.apply(x, w, b, det)


def subm_conv(x, w5, b, nbr, variant=None, det=False):
    """Submanifold conv on the offset-major kernel map; variant and det as in `linear`."""
    if variant is not None:
        return _SubMConv16.apply(x, w5, b, nbr, variant, det)
    return _SubMConv.apply(x, w5, b, nbr, det)


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, g, b, eps, det=False):
        x = _c(x)
        y = torch.empty_like(x)
        ops.layernorm(x, g, b, y, eps=eps)
        ctx.save_for_backward(x, g)
        ctx.eps = eps
        ctx.det = _det_kw(det)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, g = ctx.saved_tensors
        dy = _c(dy)
        dx = torch.empty_like(x)
        dg = torch.zeros_like(g)
        db = torch.zeros_like(g)
        ops.layernorm_bwd(x, g, dy, dx, accumulate=False, eps=ctx.eps, dgamma=dg, dbeta=db, **ctx.det)
        return dx, dg, db, None, None


def layernorm(x, mod, det=False):
    return _LayerNorm.apply(x, mod.weight, mod.bias, float(mod.eps), det)


def resolve_train_loss(model):
    """model.train_loss: "torch" (default) or "fused" (losses.FusedCriteria); anything else raises."""
    tl = getattr(model, "train_loss", "torch")
    if tl not in TRAIN_LOSSES:
        raise ValueError(f"train_loss must be one of {sorted(TRAIN_LOSSES)}, not {tl!r}")
    return tl


TRAIN_PRECISIONS = {"fp32": None, "fp16-attn": "f16", "bf16-attn": "bf16",  # train_precision -> library build of the attention core
                    "fp16-amp": "f16", "bf16-amp": "bf16"}                   # (-amp: of the Linears and sparse convs too)


class _Attention(torch.autograd.Function):
    """softmax(q k^T scale) v per padded patch and head on gathered rows (ref: ptv3.py:246-296 / :988-1055).
    q (N, C), kv (N, 2C) (self attention: views of the packed qkv)."""

    @staticmethod
    def forward(ctx, q, k, v, q_gidx, kv_gidx, widx, patch_start, patch_start_host, heads, max_len, scale):
        o = _f32(q.shape, q)
        ops.attention(q, k, v, q_gidx, kv_gidx, widx, patch_start, heads, max_len, scale, o)
        ctx.save_for_backward(q, k, v, q_gidx, kv_gidx, widx, patch_start)
        ctx.meta = (list(patch_start_host), heads, scale)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, q_gidx, kv_gidx, widx, patch_start = ctx.saved_tensors
        psh, heads, scale = ctx.meta
        dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
        ops.attention_bwd(q, k, v, q_gidx, kv_gidx, widx, patch_start, psh, heads, scale, _c(do), dq, dk, dv)
        return dq, dk, dv, None, None, None, None, None, None, None, None


class _Attention16(torch.autograd.Function):
    """_Attention with a 16-bit core (ref: ptv3.py:282-289 `qkv.half()` into flash-attention, :1038-1047): `src` is the packed
    fp32 projection (qkv of a Block; q and kv of the cross attention arrive as two calls' worth: `src2`), cast ONCE to the
    16-bit type of library build `variant`; the forward is the inference path's 16-bit kernel (flags 0) with its 16-bit output
    cast up; the 16-bit copies are what the backward keeps; dout is cast WITHOUT saturation (a scaled gradient beyond half's
    range must reach the GradScaler as inf, the library's own casts would clamp it); dq / dk / dv come back fp32, and the
    cast's backward is the identity.  The build is selected inside forward AND backward from ctx (`_lib.use` is per thread
    and autograd runs backward on a thread of its own)."""

    @staticmethod
    def forward(ctx, src, src2, cq, q_gidx, kv_gidx, widx, patch_start, patch_start_host, heads, max_len, scale, variant):
        t16 = ops.LP_DTYPES[variant]
        with _lib.use(variant):
            a = ops.cast(_c(src), t16)
            b = a if src2 is None else ops.cast(_c(src2), t16)
            q, k, v = (a[:, :cq], a[:, cq:2 * cq], a[:, 2 * cq:]) if src2 is None else (a, b[:, :cq], b[:, cq:])
            o = torch.empty((src.shape[0], cq), dtype=t16, device=src.device)
            ops.attention(q, k, v, q_gidx, kv_gidx, widx, patch_start, heads, max_len, scale, o)
        ctx.save_for_backward(a, b, q_gidx, kv_gidx, widx, patch_start)
        ctx.meta = (list(patch_start_host), heads, scale, variant, cq, src2 is None)
        return o.float()

    @staticmethod
    def backward(ctx, do):
        a, b, q_gidx, kv_gidx, widx, patch_start = ctx.saved_tensors
        psh, heads, scale, variant, cq, packed = ctx.meta
        q, k, v = (a[:, :cq], a[:, cq:2 * cq], a[:, 2 * cq:]) if packed else (a, b[:, :cq], b[:, cq:])
        da = torch.zeros(a.shape, dtype=torch.float32, device=a.device)
        db = da if packed else torch.zeros(b.shape, dtype=torch.float32, device=a.device)
        dq, dk, dv = (da[:, :cq], da[:, cq:2 * cq], da[:, 2 * cq:]) if packed else (da, db[:, :cq], db[:, cq:])
        with _lib.use(variant):
            ops.attention_bwd(q, k, v, q_gidx, kv_gidx, widx, patch_start, psh, heads, scale, _c(do).to(a.dtype), dq, dk, dv)
        return da, (None if packed else db), None, None, None, None, None, None, None, None, None, None


class _AttentionDrop(torch.autograd.Function):
    """_Attention with dropout on the probabilities (ref: ptv3.py:282-288 `dropout_p=self.attn_drop`): drop = (rate, seed,
    offset), the site's mask of include/cdseg.h; the backward regenerates it from the same triple."""

    @staticmethod
    def forward(ctx, q, k, v, q_gidx, kv_gidx, widx, patch_start, patch_start_host, heads, max_len, scale, drop):
        o = _f32(q.shape, q)
        ops.attention_drop(q, k, v, q_gidx, kv_gidx, widx, patch_start, heads, max_len, scale, o, *drop)
        ctx.save_for_backward(q, k, v, q_gidx, kv_gidx, widx, patch_start)
        ctx.meta = (list(patch_start_host), heads, scale, tuple(drop))
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, q_gidx, kv_gidx, widx, patch_start = ctx.saved_tensors
        psh, heads, scale, drop = ctx.meta
        dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
        ops.attention_drop_bwd(q, k, v, q_gidx, kv_gidx, widx, patch_start, psh, heads, scale, _c(do), dq, dk, dv, *drop)
        return dq, dk, dv, None, None, None, None, None, None, None, None, None


class _AttentionDrop16(torch.autograd.Function):
    """_Attention16 with dropout on the probabilities: the same casts (dout WITHOUT saturation), the 16-bit dropout kernels."""

    @staticmethod
    def forward(ctx, src, src2, cq, q_gidx, kv_gidx, widx, patch_start, patch_start_host, heads, max_len, scale, variant, drop):
        t16 = ops.LP_DTYPES[variant]
        with _lib.use(variant):
            a = ops.cast(_c(src), t16)
            b = a if src2 is None else ops.cast(_c(src2), t16)
            q, k, v = (a[:, :cq], a[:, cq:2 * cq], a[:, 2 * cq:]) if src2 is None else (a, b[:, :cq], b[:, cq:])
            o = torch.empty((src.shape[0], cq), dtype=t16, device=src.device)
            ops.attention_drop(q, k, v, q_gidx, kv_gidx, widx, patch_start, heads, max_len, scale, o, *drop)
        ctx.save_for_backward(a, b, q_gidx, kv_gidx, widx, patch_start)
        ctx.meta = (list(patch_start_host), heads, scale, variant, cq, src2 is None, tuple(drop))
        return o.float()

    @staticmethod
    def backward(ctx, do):
        a, b, q_gidx, kv_gidx, widx, patch_start = ctx.saved_tensors
        psh, heads, scale, variant, cq, packed, drop = ctx.meta
        q, k, v = (a[:, :cq], a[:, cq:2 * cq], a[:, 2 * cq:]) if packed else (a, b[:, :cq], b[:, cq:])
        da = torch.zeros(a.shape, dtype=torch.float32, device=a.device)
        db = da if packed else torch.zeros(b.shape, dtype=torch.float32, device=a.device)
        dq, dk, dv = (da[:, :cq], da[:, cq:2 * cq], da[:, 2 * cq:]) if packed else (da, db[:, :cq], db[:, cq:])
        with _lib.use(variant):
            ops.attention_drop_bwd(q, k, v, q_gidx, kv_gidx, widx, patch_start, psh, heads, scale, _c(do).to(a.dtype), dq, dk, dv,
                                   *drop)
        return da, (None if packed else db), None, None, None, None, None, None, None, None, None, None, None


class _Dropout(torch.autograd.Function):
    """Element dropout of an fp32 (rows, C) tensor (ref: proj_drop ptv3.py:293-294, MLP.drop :316-322): y = x o M / keep with
    the site's mask; the backward is the same call on dy."""

    @staticmethod
    def forward(ctx, x, rate, seed, offset):
        ctx.meta = (rate, seed, offset)
        return ops.dropout(_c(x), rate, seed, offset)

    @staticmethod
    def backward(ctx, dy):
        return ops.dropout(_c(dy), *ctx.meta), None, None, None


def attention_core(variant, q_src, kv_src, cq, q_gidx, kv_gidx, widx, patch_start, psh, heads, max_len, scale, drop=None):
    """The attention core of a Block (kv_src None: q_src is the packed (N, 3 cq) qkv) or of the cross attention (q_src (N, cq),
    kv_src (M, 2 cq)); variant None = exact fp32, "f16" / "bf16" = 16-bit core on that build of the library.
    drop: None, or (rate, seed, offset) of the site's attention dropout."""
    if variant is None:
        q, k, v = (q_src[:, :cq], q_src[:, cq:2 * cq], q_src[:, 2 * cq:]) if kv_src is None else (q_src, kv_src[:, :cq], kv_src[:, cq:])
        if drop is not None:
            return _AttentionDrop.apply(q, k, v, q_gidx, kv_gidx, widx, patch_start, psh, heads, max_len, scale, drop)
        return _Attention.apply(q, k, v, q_gidx, kv_gidx, widx, patch_start, psh, heads, max_len, scale)
    if drop is not None:
        return _AttentionDrop16.apply(q_src, kv_src, cq, q_gidx, kv_gidx, widx, patch_start, psh, heads, max_len, scale, variant, drop)
    return _Attention16.apply(q_src, kv_src, cq, q_gidx, kv_gidx, widx, patch_start, psh, heads, max_len, scale, variant)


class _SegmentMax(torch.autograd.Function):
    """Per-channel maximum over the (contiguous) children of every pooled row (torch_scatter.segment_csr(reduce="max"),
    ptv3.py:510-515).  The backward sends a pooled row's gradient to the child that held the maximum (recomputed)."""

    @staticmethod
    def forward(ctx, y, seg, cluster, m):
        y = _c(y)
        c = y.shape[1]
        one = torch.ones(c, dtype=torch.float32, device=y.device)
        out = _f32((m, c), y)
        ops.segment_max(y, seg, m, one, torch.zeros_like(one), ops.ACT_NONE, out)
        ctx.save_for_backward(y, out, seg[:m + 1], cluster)
        return out

    @staticmethod
    def backward(ctx, dout):
        y, out, seg, cluster = ctx.saved_tensors
        cl = cluster.long()
        hit = y == out[cl]
        # exactly ONE child per (pooled row, channel) receives the gradient - the first that holds the maximum, like
        # segment_csr's arg-max (torch_scatter updates its arg only on a strictly larger value); ties are rare but exist
        # (GELU outputs saturate, duplicate points)
        cs = hit.to(torch.int32).cumsum(0)
        before = (cs - hit.to(torch.int32))[seg[:-1].long()]  # hits in front of each segment, per channel
        first = hit & ((cs - before[cl]) == 1)
        return first.to(dout.dtype) * dout[cl], None, None, None


class _SceneRows(torch.autograd.Function):
    """rows[i] = per_scene[batch[i]] for a level in (batch | z) order: the rows of a scene are contiguous, so the backward is
    one column sum per scene (torch's index backward serialises the N duplicates of a row: 234 of a 450 ms step)."""

    @staticmethod
    def forward(ctx, per_scene, batch, offs):
        ctx.offs = offs
        return per_scene[batch]

    @staticmethod
    def backward(ctx, dy):
        o = ctx.offs
        return torch.stack([dy[o[b]:o[b + 1]].sum(0) for b in range(len(o) - 1)]), None, None


TRAIN_MIX3D = ("fold", "rows")


def resolve_train_mix3d(model):
    """model.train_mix3d: "fold" (default) or "rows" (engine.RowLevel: every point of a shared voxel is trained); anything else
    raises."""
    tm = getattr(model, "train_mix3d", "fold")
    if tm not in TRAIN_MIX3D:
        raise ValueError(f"train_mix3d must be one of {sorted(TRAIN_MIX3D)}, not {tm!r}")
    return tm


TRAIN_BLOCKS = ("autograd", "native")


def resolve_train_block(model):
    """model.train_block: "autograd" (default) or "native" (`_NativeBlock`); anything else raises."""
    tb = getattr(model, "train_block", "autograd")
    if tb not in TRAIN_BLOCKS:
        raise ValueError(f"train_block must be one of {sorted(TRAIN_BLOCKS)}, not {tb!r}")
    return tb


def block_parameters(mod):
    """The 18 parameter tensors of a Block in nn.Module order (include/cdseg.h CDSEG_TB_*)."""
    mods = (mod.cpe[0], mod.cpe[1], mod.cpe[2], mod.norm1[0], mod.attn.qkv, mod.attn.proj, mod.norm2[0], mod.mlp[0].fc1, mod.mlp[0].fc2)
    out = []
    for m in mods:
        if m.bias is None:
            raise ValueError("train_block = 'native' needs the bias of every Linear / conv of a Block (qkv_bias = True)")
        out += [m.weight, m.bias]
    return out


class _NativeBlock(torch.autograd.Function):
    """One whole Block (ref: ptv3.py:399-428) as ONE autograd node (`model.train_block = "native"`): the forward is one library
    call that keeps what the backward reads in a tape, the backward is one library call that writes dx_in, dx_conv, dt_rows and
    a gradient slab whose 18 views are returned in parameter order (csrc/trainblock.hip).  The parameters, the optimizer's
    16-bit copies in use, the tape and the index tensors are saved with save_for_backward: a weight that changes in place between
    forward and backward (an optimizer step) is an autograd error, as with the per-op nodes."""

    @staticmethod
    def forward(ctx, tb, idx, x_in, x_conv, t_rows, mask1, mask2, *weights):
        scene_offs, nbr, gidx, widx, patch_start, psh, rows = idx  # rows: None or (row_vox, row_start) of an engine.RowLevel
        x_in = _c(x_in.float())
        xc = x_in if x_conv is None else _c(x_conv.float())
        t_rows = None if t_rows is None else _c(t_rows.float())
        n = x_in.shape[0]
        tape_b, scratch_b, _, grads_b = ops.train_block_bytes(tb, n, psh[-1])
        dev = x_in.device
        tape = _alloc._scratch(tape_b, dev)
        scratch = _alloc._scratch(scratch_b, dev)
        x_out = torch.empty_like(x_in)
        ops.train_block_forward(tb, n, x_in, xc, t_rows, scene_offs, mask1, mask2, nbr, gidx, widx, patch_start, psh, tape, scratch,
                                x_out, **({} if rows is None else dict(rows=rows)))
        opt = [t for t in (None if x_conv is None else xc, t_rows, mask1, mask2) if t is not None]
        opt += [] if rows is None else list(rows)
        ctx.save_for_backward(x_in, tape, scene_offs, nbr, gidx, widx, patch_start, *opt, *weights)
        ctx.has_rows = rows is not None
        ctx.meta = (tb, list(psh), x_conv is not None, t_rows is not None, mask1 is not None, mask2 is not None, scratch_b, grads_b, len(weights))
        return x_out

    @staticmethod
    def backward(ctx, dy):
        tb, psh, has_xc, has_t, has_m1, has_m2, scratch_b, grads_b, nw = ctx.meta
        saved = list(ctx.saved_tensors)
        x_in, tape, scene_offs, nbr, gidx, widx, patch_start = saved[:7]
        rest = iter(saved[7:])
        xc = next(rest) if has_xc else x_in
        t_rows = next(rest) if has_t else None
        mask1 = next(rest) if has_m1 else None
        mask2 = next(rest) if has_m2 else None
        rows = dict(rows=(next(rest), next(rest))) if ctx.has_rows else {}
        n = x_in.shape[0]
        dev = x_in.device
        dy = _c(dy.float())
        dx_in = torch.empty_like(x_in)
        dx_conv = torch.empty_like(x_in) if has_xc else None
        dt_rows = torch.empty_like(t_rows) if has_t else None
        slab = _alloc._scratch(grads_b, dev)
        scratch = _alloc._scratch(scratch_b, dev)
        ops.train_block_backward(tb, n, x_in, xc, t_rows, scene_offs, mask1, mask2, nbr, gidx, widx, patch_start, psh, tape, scratch,
                                 None, dy, dx_in, dx_conv, dt_rows, slab, **rows)
        grads = ops.train_block_grad_views(tb, slab)
        return (None, None, dx_in, dx_conv, dt_rows, None, None, *grads, *([None] * (nw - len(grads))))  # (the 16-bit copies: no gradient)


def gate_dp(mode, p, sums):
    """d loss / d feat_scale (p's shape, fp64) from the two column sums of the gate's backward, sums = [d gamma (c), d alpha (c)]
    = [sum_r dy m a, sum_r dy s]: gamma = p or sigmoid(p), alpha = 1 or 1 - gamma; a scalar p adds over the channels."""
    c = sums.numel() // 2
    d = sums[:c].double()
    if mode.startswith("b_"):
        d = d - sums[c:].double()
    if _FUSION_MODES[mode][0]:
        sg = torch.sigmoid(p.detach().double().reshape(-1))
        return (d * sg * (1 - sg)).reshape(p.shape)
    return d.sum().reshape(p.shape)


class _FuseGate(torch.autograd.Function):
    """The learned gate of a CrossBlock, y = alpha s + gamma m a (`models.gate_vectors`), as one node: forward cdseg_fuse_gate_fwd,
    backward cdseg_fuse_gate_bwd - ds, da and the two fp64 column sums from which `gate_dp` forms feat_scale's gradient.  The
    sums run in a fixed order whatever `train_deterministic` says.  fp32 in every train_precision (the Linear outputs are)."""

    @staticmethod
    def forward(ctx, s, a, m, p, mode):
        s, a = _c(s.float()), _c(a.float())
        m = None if m is None else _c(m.float().reshape(-1))
        alpha, gamma = (_c(v) for v in gate_vectors(mode, p.detach().float(), s.shape[1]))
        y = ops.fuse_gate_fwd(s, a, alpha, gamma, m)
        ctx.save_for_backward(s, a, p, alpha, gamma, *(() if m is None else (m,)))
        ctx.mode = mode
        return y

    @staticmethod
    def backward(ctx, dy):
        s, a, p, alpha, gamma = ctx.saved_tensors[:5]
        m = ctx.saved_tensors[5] if len(ctx.saved_tensors) > 5 else None
        ds, da, sums = ops.fuse_gate_bwd(_c(dy.float()), s, a, alpha, gamma, m)
        return ds, da, None, gate_dp(ctx.mode, p, sums).to(p.dtype), None


def _skip_filter(x, ref_of_row, s):
    y = _c(x.float()).clone()
    n = y.shape[0]
    return ops.skip_merge(y, ops.skip_stats(y, ref_of_row, n), s, 1.0, ref_of_row, n)


class _SkipFilter(torch.autograd.Function):
    """FreeU's Fourier filter of a skip feature (ptv3.py:42-66, :614-620) over the two kernels of csrc/skip.hip:
    y = x + k P x with P symmetric, so the backward is the same pair of calls on the incoming gradient.  The sums run in fp64
    in an order fixed by the shape whatever `train_deterministic` says.  fp32 in every train_precision."""

    @staticmethod
    def forward(ctx, x, ref_of_row, s):
        ctx.ref, ctx.s = ref_of_row, s
        return _skip_filter(x, ref_of_row, s)

    @staticmethod
    def backward(ctx, dy):
        return _skip_filter(dy, ctx.ref, ctx.s), None, None


def _swish(x):  # ptv3.py:30-31
    return x * torch.sigmoid(x)


TRAIN_NORMS = ("torch", "fused")
_NORM_WIDTHS = range(16, 513, 16)  # channel counts of the kernels of csrc/norm.hip


def resolve_train_norm(model):
    """model.train_norm: "torch" (default) or "fused" (`_BnGelu`, `_SegmentMaxArg`); anything else raises."""
    tn = getattr(model, "train_norm", "torch")
    if tn not in TRAIN_NORMS:
        raise ValueError(f"train_norm must be one of {sorted(TRAIN_NORMS)}, not {tn!r}")
    return tn


def merge_shards(parts):
    """Statistics / backward-sum buffers of several row shards -> the buffer of all rows: plain fp64 addition in list order."""
    t = parts[0].clone()
    for p in parts[1:]:
        t += p
    return t


def gather_ranks(buf, group):
    """The cross-rank step of SyncBN: ONE all_gather of this rank's fp64 buffer, added in rank order (`merge_shards`) - the
    same bits on every rank, no all-reduce whose order the backend picks."""
    dist = torch.distributed
    parts = [torch.empty_like(buf) for _ in range(dist.get_world_size(group))]
    dist.all_gather(parts, buf.contiguous(), group=group)
    return merge_shards(parts)


def sync_group(bn):
    """(process group,) when `bn` is an nn.SyncBatchNorm whose group spans more than one rank of an initialised
    torch.distributed (group None = the default group), else None: statistics over this process's rows."""
    if not isinstance(bn, torch.nn.SyncBatchNorm):
        return None
    dist = torch.distributed
    if not (dist.is_available() and dist.is_initialized()):
        return None
    group = getattr(bn, "process_group", None)
    return (group,) if dist.get_world_size(group) > 1 else None


class _BnGelu(torch.autograd.Function):
    """nn.BatchNorm1d (training) -> GELU on the kernels of csrc/norm.hip (`model.train_norm = "fused"`): fp64 statistics in a
    fixed order, one fused normalise + GELU pass; the backward recomputes z from x (saved: x, mean, invstd and the 2 c + 1
    statistics, no BatchNorm output).  group (from `sync_group`): the statistics and the backward sums are gathered over the
    ranks (`gather_ranks`), a rank without rows takes part with zeros.  dgamma / dbeta are THIS rank's sums (averaging them is
    the gradient synchronisation's job, as with torch's SyncBatchNorm).  Running buffers and num_batches_tracked are updated
    like the module would.  No double backward."""

    @staticmethod
    def forward(ctx, x, gamma, beta, bn, group):
        x = _c(x)
        m, c = x.shape
        stats = ops.bn_stats(x)
        if group is not None:
            stats = gather_ranks(stats, group[0])
        elif m <= 1:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
        mean, invstd = ops.bn_finish(stats, bn.eps, bn.momentum, bn.running_mean, bn.running_var)
        if bn.num_batches_tracked is not None:
            bn.num_batches_tracked.add_(1)
        y = ops.bn_gelu_fwd(x, mean, invstd, gamma, beta)
        ctx.save_for_backward(x, mean, invstd, gamma, beta, stats)
        ctx.group = group
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, invstd, gamma, beta, stats = ctx.saved_tensors
        c = x.shape[1]
        group = ctx.group
        hook = None if group is None else (lambda g: gather_ranks(g, group[0]))
        dx, gs = ops.bn_gelu_bwd(x, _c(dy.float()), mean, invstd, gamma, beta, stats[2 * c:], hook=hook)
        return dx, gs[c:].float(), gs[:c].float(), None, None


class _SegmentMaxArg(torch.autograd.Function):
    """`_SegmentMax` with the arg-max kept (`model.train_norm = "fused"`): the forward writes the first maximal child of every
    (pooled row, channel) next to the maximum, the backward is one launch over the fine rows (saved: arg int32 and cluster,
    neither y nor out)."""

    @staticmethod
    def forward(ctx, y, seg, cluster, m):
        out, arg = ops.segment_max_arg(_c(y), seg, m)
        ctx.save_for_backward(arg, cluster)
        return out

    @staticmethod
    def backward(ctx, dout):
        arg, cluster = ctx.saved_tensors
        return ops.segment_max_bwd(_c(dout.float()), arg, _c(cluster)), None, None, None


_warned_local_sync_bn = False
_warned_native_dropout = False


def _bn_gelu(x, bn, norm="torch"):
    """nn.BatchNorm1d -> GELU, in the module's own mode: training = batch statistics, running buffers updated like the
    module would; eval (`model.eval(); model(batch)`, e.g. a validation-loss hook) = running statistics, buffers untouched.
    norm "fused" (model.train_norm): the training form runs as `_BnGelu` where the kernels cover it (width a multiple of 16 up
    to 512, affine, a float momentum) - with statistics over all ranks when `bn` is an nn.SyncBatchNorm (`sync_group`)."""
    if not bn.training:
        return F.gelu(F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, bn.momentum, bn.eps))
    group = sync_group(bn)
    if (norm == "fused" and x.dim() == 2 and x.dtype == torch.float32 and x.shape[1] in _NORM_WIDTHS and bn.weight is not None
            and bn.bias is not None and isinstance(bn.momentum, float)):
        return _BnGelu.apply(x, bn.weight, bn.bias, bn, group)
    if group is not None:
        global _warned_local_sync_bn
        if not _warned_local_sync_bn:
            _warned_local_sync_bn = True
            warnings.warn("nn.SyncBatchNorm under more than one rank: this path normalises with the statistics of THIS rank's "
                          "rows only; model.train_norm = \"fused\" synchronises them (cdsegnet_amd/train_graph.py)")
    if bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    return F.gelu(F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, True, bn.momentum, bn.eps))


def voxel_representatives(grid, offset):
    """Points that share a (batch element, grid_coord) voxel -> (keep, rep, offset_u): `keep` = indices of the first point
    (caller's order) of every voxel, ascending; `rep[i]` = position in `keep` of point i's voxel; `offset_u` = cumulative
    point counts of the kept points per batch element.  torch device ops (training path only)."""
    n, dev = grid.shape[0], grid.device
    ar = torch.arange(n, device=dev)
    batch = torch.bucketize(ar, offset.to(dev), right=True)
    g = grid.long()
    key = ((batch << 17 | g[:, 0]) << 17 | g[:, 1]) << 17 | g[:, 2]  # grid < 2^16 per axis (structure.py:74), batch < 2^12
    _, inverse = torch.unique(key, return_inverse=True)
    first = torch.full((int(inverse.max()) + 1,), n, dtype=torch.long, device=dev).scatter_reduce_(0, inverse, ar, "amin")
    keep = first.sort().values
    pos = torch.empty(n, dtype=torch.long, device=dev)
    pos[keep] = torch.arange(keep.numel(), device=dev)
    rep = pos[first[inverse]]
    offset_u = torch.bincount(batch[keep], minlength=offset.numel()).cumsum(0).to(offset.dtype)
    return keep, rep, offset_u


def feat_is_cuda(input_dict):
    return bool(getattr(input_dict.get("feat"), "is_cuda", False))


class _St:
    """A branch's point set at one level: features in the plan's physical (batch | z) order."""

    def __init__(self, level, x, curves, ref_order, parent=None):
        self.level, self.x, self.curves, self.ref_order, self.parent = level, x, curves, ref_order, parent
        self.conv = None  # stale conv input behind an unpooling (ptv3.py:597-630: sparse_conv_feat is not re-synchronised)


class TrainGraph:
    """Builds the autograd graph of one training forward of `model` (DefaultSegmentorV2 in train mode)."""

    def __init__(self, model):
        self.model = model
        self.attn_variant = None  # library build of the attention core, from model.train_precision at every forward
        self.mm_variant = None    # library build of the Linears and sparse convs ("-amp" modes), None = exact fp32
        self.det = False          # fixed-order gradient reductions, from model.train_deterministic at every forward
        self.eng = _engine.Engine(model, "fp32")  # the plan builder (never prepared: no second copy of the weights)
        self.criteria = build_criteria(model.criteria_cfg, model.loss_type, model.task_num)
        self.fused_criteria = None  # losses.FusedCriteria, built when model.train_loss first says "fused"
        self.train_loss = "torch"   # from model.train_loss at every forward
        self.train_norm = "torch"   # from model.train_norm at every forward
        self.train_block = "autograd"  # from model.train_block at every forward
        self.train_mix3d = "fold"      # from model.train_mix3d at every forward
        self.last_shared = None        # (N points, V voxels) of the last forward
        self._native = {}  # id(Block) -> [Block, static key, weight versions, ops.TrainBlock] (train_block "native")
        # dropout sites (attn_drop / proj_drop): a site is (seed, offset) of the library's mask stream.  seed = torch.initial_seed();
        # every site of a forward takes the next offset of a counter that restarts when a forward finds another seed than the
        # forward before it (the rule of Engine.reserve_rng); draws["dropout"] = (seed, first offset) pins a forward.
        self._drop_seed, self._drop_offset = None, 0
        self._site = None          # [seed, next offset] of the running forward
        self.dropout_sites = []    # (site name, seed, offset) of the last forward, in call order

    # ---------------------------------------------------------------------------------------- pieces
    def _mask(self, st, name, rate, masks):
        """Stochastic-depth row mask of module `name` (already divided by the keep probability), physical order."""
        if masks is not None:
            q = masks.get(name)
            if not q:
                return None
            m = torch.as_tensor(q.pop(0), dtype=torch.float32, device=st.x.device).reshape(-1, 1)
            # recorded masks are in the REFERENCE's row order of the level: the input order at level 0, the sorted order of
            # the curve that was first in the order list when the level was pooled (ptv3.py:489-493) above it;
            # ref_order: reference row -> physical row
            out = torch.empty_like(m)
            out[st.ref_order.long()] = m
            return out
        if rate <= 0.0 or not self.model.training:  # DropPath is the identity in eval mode (timm; ptv3.py:393)
            return None
        keep = 1.0 - rate
        return torch.empty((st.x.shape[0], 1), dtype=torch.float32, device=st.x.device).bernoulli_(keep) / keep

    def _conv(self, lv, x, conv, bias):
        """Sparse conv of a level's rows.  On a row level (Mix3D, `train_mix3d = "rows"`) the voxel is the conv's unit: it reads
        the first row of every voxel and returns ONE row per voxel (`_spread` hands it to the voxel's rows)."""
        if isinstance(lv, _engine.RowLevel):
            x, lv = x[lv.row_start[:-1].long()], lv.voxels
        return subm_conv(x, conv.weight, bias, lv.nbr(conv.kernel_size, True), self.mm_variant, self.det)

    def _spread(self, lv, y):
        """Voxel rows -> the level's rows (the identity below a row level).  The backward adds a voxel's contiguous run in
        ascending row order in either mode: the atomic-free form costs nothing extra here."""
        if isinstance(lv, _engine.RowLevel):
            return _GatherRuns.apply(y, lv.row_vox.long(), lv.row_start, None)
        return y

    def _cpe(self, lv, x, seq):
        y = self._conv(lv, x, seq[0], seq[0].bias)
        return self._spread(lv, self._ln(self._lin(y, seq[1]), seq[2]))

    def _lin(self, x, mod):
        return linear(x, mod, self.mm_variant, self.det)

    def _ln(self, x, mod):
        return layernorm(x, mod, self.det)

    def _begin_sites(self, draws):
        self.dropout_sites = []
        pinned = draws.get("dropout") if draws else None
        if pinned is not None:
            self._site = [int(pinned[0]), int(pinned[1]), True]
            return
        seed = torch.initial_seed()
        if seed != self._drop_seed:
            self._drop_seed, self._drop_offset = seed, 0
        self._site = [seed, self._drop_offset, False]

    def _next_site(self, name):
        """(seed, offset) of dropout site `name`: the next offset of the forward."""
        seed, offset, pinned = self._site
        self._site[1] = offset + 1
        if not pinned:
            self._drop_offset = offset + 1
        self.dropout_sites.append((name, seed, offset))
        return seed, offset

    def _attn_site(self, att, name):
        """None, or (rate, seed, offset) of the attention dropout of `att` in this forward (train mode, rate > 0)."""
        if att.attn_drop <= 0.0 or not self.model.training:
            return None
        return (att.attn_drop,) + self._next_site(name + ".attn.attn_drop")

    def _drop(self, x, rate, name):
        """Element dropout site `name`; the identity in eval mode or at rate 0 (no node)."""
        if rate <= 0.0 or not self.model.training:
            return x
        return _Dropout.apply(x, rate, *self._next_site(name))

    def _mlp(self, h, mlp, rate=0.0, name=""):
        """fc1 - GELU - drop - fc2 - drop (ptv3.py:316-322; rate: the block's proj_drop)."""
        h = self._drop(F.gelu(self._lin(h, mlp.fc1)), rate, name + ".mlp.0.drop.0")
        return self._drop(self._lin(h, mlp.fc2), rate, name + ".mlp.0.drop.1")

    def _native_desc(self, mod):
        """The Block's descriptor for the native executor, with its derived weights current: rebuilt when the mode, a
        parameter's storage or the set of 16-bit optimizer copies changes; `prepare` (one launch) once per weight version."""
        params = block_parameters(mod)
        t16 = ops.LP_DTYPES[self.mm_variant] if self.mm_variant is not None else None
        shadows = [None if t16 is None else _shadow16(params[i], t16) for i in ops.TB_MATRICES]
        shadows = [s if s is not None and s.is_contiguous() and s.data_ptr() % 16 == 0 else None for s in shadows]
        att = mod.attn
        static = (self.mm_variant, self.attn_variant, self.det, att.num_heads, float(att.scale), tuple(p.data_ptr() for p in params),
                  tuple(None if s is None else s.data_ptr() for s in shadows))
        versions = tuple(p._version for p in params)
        ent = self._native.get(id(mod))
        if ent is None or ent[0] is not mod or ent[1] != static:
            eps = (float(mod.cpe[2].eps), float(mod.norm1[0].eps), float(mod.norm2[0].eps))
            tb = ops.TrainBlock([p.detach() for p in params], att.num_heads, att.scale, eps, self.mm_variant, self.attn_variant,
                                self.det, shadows)
            ent = self._native[id(mod)] = [mod, static, None, tb]
        if ent[2] != versions:
            ops.train_block_prepare(ent[3])
            ent[2] = versions
        return ent[3], params, [s for s in shadows if s is not None]

    def _block_native(self, st, mod, name, t_scene, masks):
        """`_block` as one `_NativeBlock` node; the timestep Linear on B rows stays torch (its gradient arrives as dt_rows)."""
        lv = st.level
        x = st.x
        xconv, st.conv = st.conv, None
        t_rows = None
        if t_scene is not None and hasattr(mod, "t_mlp"):
            t_rows = F.linear(t_scene, mod.t_mlp.weight, mod.t_mlp.bias)
        att = mod.attn
        gidx, widx = lv.slots(st.curves[att.order_index], att.patch_size, att.enable_flash)
        pad = lv.pad(att.patch_size, att.enable_flash)
        scene_offs, patch_start = pad[2], pad[4]
        psh = lv.pad_host(att.patch_size, att.enable_flash)[3].tolist()
        m1 = self._mask(st, name + ".drop_path.0", mod.drop_prob, masks)
        m2 = self._mask(st, name + ".drop_path.0", mod.drop_prob, masks)
        m1, m2 = (None if m is None else _c(m.reshape(-1)) for m in (m1, m2))
        tb, params, shadows = self._native_desc(mod)
        rows = isinstance(lv, _engine.RowLevel)
        idx = (scene_offs, (lv.voxels if rows else lv).nbr(mod.cpe[0].kernel_size, True), gidx, widx, patch_start, psh,
               (lv.row_vox, lv.row_start) if rows else None)
        st.x = _NativeBlock.apply(tb, idx, x, xconv, t_rows, m1, m2, *params, *shadows)
        return st

    def _block(self, st, mod, name, t_scene, masks):
        """ref: ptv3.py:399-428."""
        if self.train_block == "native":
            if not self.model.training or (mod.attn_drop <= 0.0 and mod.proj_drop <= 0.0):
                return self._block_native(st, mod, name, t_scene, masks)
            global _warned_native_dropout  # (dropout is not part of the native executor: this Block runs as its autograd chain)
            if not _warned_native_dropout:
                _warned_native_dropout = True
                warnings.warn("train_block = 'native': a Block with attn_drop / proj_drop > 0 runs as its autograd chain (dropout "
                              "is not part of the native Block executor; cdsegnet_amd/train_graph.py)")
        lv = st.level
        x = st.x
        xconv, st.conv = (x if st.conv is None else st.conv), None
        x = x + self._cpe(lv, xconv, mod.cpe)
        if t_scene is not None and hasattr(mod, "t_mlp"):
            x = x + _SceneRows.apply(F.linear(t_scene, mod.t_mlp.weight, mod.t_mlp.bias), lv.batch.long(), list(lv.offs_host))
        att = mod.attn
        c = x.shape[1]
        qkv = self._lin(self._ln(x, mod.norm1[0]), att.qkv)
        gidx, widx = lv.slots(st.curves[att.order_index], att.patch_size, att.enable_flash)
        patch_start, max_len = lv.pad(att.patch_size, att.enable_flash)[4:6]
        psh = lv.pad_host(att.patch_size, att.enable_flash)[3].tolist()
        o = attention_core(self.attn_variant, qkv, None, c, gidx, gidx, widx, patch_start, psh, att.num_heads, max_len, att.scale,
                           self._attn_site(att, name))
        a = self._drop(self._lin(o, att.proj), att.proj_drop, name + ".attn.proj_drop")
        m = self._mask(st, name + ".drop_path.0", mod.drop_prob, masks)
        x = x + (a if m is None else a * m)
        h = self._mlp(self._ln(x, mod.norm2[0]), mod.mlp[0], mod.proj_drop, name)
        m = self._mask(st, name + ".drop_path.0", mod.drop_prob, masks)
        st.x = x + (h if m is None else h * m)
        return st

    def _embedding(self, plan, feat, emb, curves, inv0):
        """ref: ptv3.py:633-663.  inv0: caller row -> physical row (the reference's level-0 order is the caller's)."""
        rows = plan.rows
        lv = plan.levels[0] if rows is None else rows
        x = feat[(plan.perm0 if rows is None else rows.perm_rows).long()]
        y = self._spread(lv, self._conv(lv, x, emb.stem.conv, None))
        return _St(lv, _bn_gelu(y, emb.stem.norm, self.train_norm), curves, inv0)

    def _pooling(self, plan, st, down, cum_to, perm):
        """ref: ptv3.py:464-555."""
        fine, coarse = st.level, plan.levels[cum_to]
        cluster, seg = plan.link_from(fine, cum_to)
        y = self._lin(st.x, down.proj)
        if self.train_norm == "fused" and y.shape[1] in _NORM_WIDTHS:
            y = _SegmentMaxArg.apply(y, seg, cluster, coarse.n)
        else:
            y = _SegmentMax.apply(y, seg, cluster, coarse.n)
        curves = st.curves if perm is None else [st.curves[int(j)] for j in perm]
        order = coarse.order(st.curves[0])  # the reference numbers the pooled points by unique(code[0]) (ptv3.py:489)
        if order is None:
            order = torch.arange(coarse.n, dtype=torch.int32, device=st.x.device)
        return _St(coarse, _bn_gelu(y, down.norm[0], self.train_norm), curves, order, parent=st)

    def _unpooling(self, plan, st, up):
        """ref: ptv3.py:597-630."""
        parent = st.parent
        fine, coarse = parent.level, st.level
        cluster, seg = plan.link_from(fine, coarse.cum)
        child = _bn_gelu(self._lin(st.x, up.proj[0]), up.proj[1], self.train_norm)
        par = _bn_gelu(self._lin(parent.x, up.proj_skip[0]), up.proj_skip[1], self.train_norm)
        out = _St(fine, None, parent.curves, parent.ref_order, parent=parent.parent)
        out.conv = par  # what the next Block's CPE conv reads: the skip feature before scaling and merging
        f = up.skip_scale
        if f != 1.0:
            par = par * f
        if up.skip_filter is not None:  # FreeU: over all rows of the level, in the reference's row order
            if getattr(parent, "ref_of_row", None) is None:  # physical row -> reference row
                parent.ref_of_row = ops.invert_perm(_c(parent.ref_order.to(torch.int32)))
            par = _SkipFilter.apply(par, parent.ref_of_row, up.skip_filter)
        if self.det:  # the index backward would add a pooled row's (up to eight) children with atomics
            gathered = _GatherRuns.apply(child, cluster.long(), seg[:coarse.n + 1], None)
        else:
            gathered = child[cluster.long()]
        if up.skip_connection_mode == "add":
            out.x = par + gathered
        else:
            out.x = self._lin(torch.cat([par, gathered], dim=-1), up.proj_cat[0])
        return out

    def _cross_block(self, qst, kvst, cb, name, masks):
        """ref: ptv3.py:1179-1223 + :988-1055.  CrossBlock `cb` (module path `name`) with `qst` as its q point and `kvst` as its
        kv point: cross_block2 is (n, c), the cross_block1 of a bidirectional model (c, n).  The kv sequence is padded with the q
        level's plan (:1009)."""
        lv, klv = qst.level, kvst.level
        if klv is not lv and list(klv.offs_host) != list(lv.offs_host):
            raise _engine.CdsegError("cross attention needs the same number of c- and n-branch bottleneck points per batch element")
        xq = qst.x + self._cpe(lv, qst.x, cb.q_cpe)
        xkv = kvst.x + self._cpe(klv, kvst.x, cb.kv_cpe)
        hq, hkv = self._ln(xq, cb.q_norm1[0]), self._ln(xkv, cb.kv_norm1[0])
        kvst.x = hkv  # the kv point leaves the block holding its normed feature (modules.py:68-73)
        att = cb.attn
        cq = xq.shape[1]
        q = self._lin(hq, att.q)
        kv = self._lin(hkv, att.kv)
        K = att.q_patch_size
        q_gidx, widx = lv.slots(qst.curves[att.order_index], K, att.enable_flash)
        kv_gidx, _ = klv.slots(kvst.curves[att.order_index], K, att.enable_flash)
        patch_start, max_len = lv.pad(K, att.enable_flash)[4:6]
        psh = lv.pad_host(K, att.enable_flash)[3].tolist()
        o = attention_core(self.attn_variant, q, kv, cq, q_gidx, kv_gidx, widx, patch_start, psh, att.num_heads, max_len, att.scale,
                           self._attn_site(att, name))
        a = self._drop(self._lin(o, att.proj), att.proj_drop, name + ".attn.proj_drop")
        block = name
        name = name + ".drop_path.0"
        m = self._mask(qst, name, cb.drop_prob, masks)
        if isinstance(cb.tm_feat, str):  # a learned gate: one node over the two kernels of csrc/fusion.hip
            x = _FuseGate.apply(xq, a, m, cb.feat_scale, cb.tm_feat)
        else:
            x = xq + cb.tm_feat * (a if m is None else a * m)
        h = self._mlp(self._ln(x, cb.q_norm2[0]), cb.mlp[0], cb.proj_drop, block)
        m = self._mask(qst, name, cb.drop_prob, masks)
        qst.x = x + (h if m is None else h * m)

    def _rows_plan(self, grid, offset_host, keep, rep, offset_u):
        """The plan of a Mix3D batch in `train_mix3d = "rows"`: today's plan of the V unique voxels (kernel maps, pooled
        levels) with an engine.RowLevel of all N points above its level 0."""
        nv = int(keep.numel())
        plan = self.eng.build_plan(grid[keep], offset_u.to(torch.int64), [int(v) for v in offset_u.cpu().tolist()], nv)
        vox_of_kept = torch.empty(nv, dtype=torch.long, device=rep.device)  # kept point -> physical voxel row
        vox_of_kept[plan.perm0.long()] = torch.arange(nv, device=rep.device)
        plan.rows = _engine.RowLevel(plan.levels[0], vox_of_kept[rep], [0] + [int(v) for v in offset_host])
        if not getattr(self, "_warned_rows", False):
            self._warned_rows = True
            seg = plan.rows.row_start.long()
            shared = int((seg[1:] - seg[:-1])[(seg[1:] - seg[:-1]) > 1].sum())
            warnings.warn(f"training batch with {100.0 * shared / rep.numel():.1f} % of its {rep.numel()} points in voxels that "
                          f"hold more than one point (Mix3D): every point is trained as a row of its own, the sparse convs read "
                          f"the first point of a voxel (train_mix3d = 'rows', cdsegnet_amd/train_graph.py)")
        return plan

    # ---------------------------------------------------------------------------------------- the forward
    def forward(self, input_dict, draws=None):
        """input_dict: coord, grid_coord, feat, offset, segment on the model's device.  draws (optional, for replaying a
        recorded step): ts (B, 1), noise (N, c_in), perms (8 x 4), masks {DropPath module name: [row masks]}.
        Returns dict(loss, n_pred, c_pred, c_target).

        The reference trainer calls the model inside `torch.cuda.amp.autocast(enabled=cfg.enable_amp)` and scales the loss
        with a GradScaler (engines/train.py:226-240).  This forward computes what `model.train_precision` says whatever the
        context ("fp32": exact fp32; "fp16-attn" / "bf16-attn": the attention core in 16 bits, the rest fp32; "fp16-amp" /
        "bf16-amp": the Linears and sparse convs on 16-bit products as well, outputs fp32 - see the module docstring): autocast is
        switched off inside it (torch's own ops here - heads, BatchNorm, GELU - would otherwise hand half tensors to fp32
        kernels), so the trainer's AMP branch runs unchanged: the scaler multiplies an fp32 loss, and only a scaled gradient
        that leaves half's range inside the "fp16-attn" core (non-finite dq / dk / dv) or, under "fp16-amp", in the unsaturated
        cast of a Linear's / conv's dy (non-finite dx / dw / db) shows up as an overflow."""
        self.train_mix3d = resolve_train_mix3d(self.model)
        tp = getattr(self.model, "train_precision", "fp32")
        if tp not in TRAIN_PRECISIONS:
            raise ValueError(f"train_precision must be one of {sorted(TRAIN_PRECISIONS)}, not {tp!r}")
        self.attn_variant = TRAIN_PRECISIONS[tp]
        self.mm_variant = TRAIN_PRECISIONS[tp] if tp.endswith("-amp") else None
        self.det = resolve_deterministic(self.model)
        self.train_loss = resolve_train_loss(self.model)
        self.train_norm = resolve_train_norm(self.model)
        self.train_block = resolve_train_block(self.model)
        self._begin_sites(draws)
        if feat_is_cuda(input_dict):
            with torch.autocast(device_type="cuda", enabled=False):
                return self._forward(input_dict, draws)
        return self._forward(input_dict, draws)

    def _forward(self, input_dict, draws=None):
        model, bb = self.model, self.model.backbone
        feat, coord = input_dict["feat"].float(), input_dict["coord"].float()
        dev = feat.device
        n = feat.shape[0]
        offset = input_dict["offset"]
        offset_host = [int(v) for v in offset.cpu().tolist()]
        B = len(offset_host)
        draws = draws or {}
        masks = draws.get("masks")
        if masks is not None:
            masks = {k: list(v) for k, v in masks.items()}
        n_orders = len(bb.order)
        grid = input_dict["grid_coord"]
        rep = None
        try:
            plan = self.eng.build_plan(grid, offset.to(torch.int64), offset_host, n)
        except DuplicateVoxelsError as e:
            # Mix3D (datasets/utils.py:51-54, mix_prob = 0.8 in every shipped CDSegNet training config) merges two scenes into
            # one batch element; both grids start at 0, so some voxels hold a point of each.  spconv tolerates that (its hash
            # keeps one row per voxel as the neighbour, every row is convolved); the kernel maps here need one point per
            # voxel, so the surplus points are FOLDED onto their voxel: the network runs on the first point (caller's order) of
            # every voxel, and every folded point reads its representative's prediction - it still enters the loss with its own
            # label, and its gradient flows into the shared row.
            keep, rep, offset_u = voxel_representatives(grid, offset)
            self.last_shared = (n, int(keep.numel()))
            if self.train_mix3d == "rows":
                # ... unless `model.train_mix3d = "rows"`: every point is a row of its own in serialization, attention,
                # BatchNorm statistics, stochastic depth, pooling and the loss, as in the reference; only the sparse convs
                # take the voxel as their unit (engine.RowLevel: the plan of the unique voxels with a row level above it)
                plan = self._rows_plan(grid, offset_host, keep, rep, offset_u)
                rep = None
            else:
                if any(up.skip_filter is not None for up in _engine.skip_modules(bb)):
                    raise ValueError("a folded Mix3D batch (train_mix3d = 'fold') on a model that filters its skip features "
                                     "(s_factor != 1): the reference filters over all N rows; use train_mix3d = 'rows'")
                if not getattr(self, "_warned_duplicates", False):
                    self._warned_duplicates = True
                    warnings.warn(f"training batch with {e.count} points in already occupied voxels (Mix3D): folded onto the "
                                  f"first point of their voxel (cdsegnet_amd/train_graph.py)")
                feat, coord, grid = feat[keep], coord[keep], grid[keep]
                n, offset_in = feat.shape[0], offset
                offset = offset_u
                offset_host = [int(v) for v in offset.cpu().tolist()]
                if "noise" in draws:
                    draws = dict(draws, noise=torch.as_tensor(draws["noise"], dtype=torch.float32)[keep.cpu()])
                plan = self.eng.build_plan(grid, offset.to(torch.int64), offset_host, n)
        else:
            self.last_shared = (n, n)
        lv0 = plan.levels[0] if plan.rows is None else plan.rows
        perm0 = (plan.perm0 if plan.rows is None else plan.rows.perm_rows).long()  # physical row -> caller row
        inv0 = torch.empty(n, dtype=torch.long, device=dev)
        inv0[perm0] = torch.arange(n, device=dev)
        batch0 = torch.empty(n, dtype=torch.long, device=dev)  # batch index in the CALLER's order
        batch0[perm0] = lv0.batch.long()
        point = {"offset": offset, "loss_mode": "train"}
        base_curves = [_engine.CURVES.index(o) for o in bb.order]

        def shuffled(perm):
            return list(base_curves) if perm is None else [base_curves[int(j)] for j in perm]

        t_scene = None
        if bb.condition:
            x0 = feat if model.c_in_channels == feat.shape[-1] else coord
            c_target = x0
            c_feat = x0
            if model.dm:
                # draws in the reference's order: timesteps, noise, then the backbone's order shuffles (default.py:449-459)
                ts = torch.as_tensor(draws["ts"]) if "ts" in draws else torch.randint(0, model.T, size=(B, 1), dtype=torch.int64)
                ts = ts.to(dev).reshape(B, 1)
                noise = (torch.as_tensor(draws["noise"], dtype=torch.float32) if "noise" in draws
                         else torch.normal(0, 1, size=tuple(x0.shape), dtype=torch.float32)).to(dev)
                if model.T_dim != -1:
                    t_emb = model.t_emb_table.to(dev)[ts[:, 0] + 1]  # rows of calc_t_emb(ts) (comm.py:21-39), one per scene
                    t_scene = _swish(F.linear(_swish(F.linear(t_emb, bb.fc_t1.weight, bb.fc_t1.bias)), bb.fc_t2.weight, bb.fc_t2.bias))
                a = model.Alpha_bar.to(dev)[ts[:, 0]][batch0][:, None]
                c_feat = torch.sqrt(a) * x0 + torch.sqrt(1 - a) * noise  # continuous_q_sample, default.py:216-222
                if model.dm_target == "noise":
                    c_target = noise
                if model.dm_min_snr is not None:
                    raise NotImplementedError("dm_min_snr (SNR loss weights): off in every shipped config")
            point["c_target"] = c_target
        perms = draws.get("perms")
        if perms is None:
            perms = [torch.randperm(n_orders).tolist() if bb.shuffle_orders else None for _ in range(8)]
        pi = iter(perms)
        n_cum, c_cum = plan.n_cum, plan.c_cum

        def enc_stage(st, branch, s, cum, perm, tsc):
            enc = getattr(getattr(bb, f"_{branch}_enc"), f"enc{s}")
            if s > 0:
                st = self._pooling(plan, st, enc.down, cum[s], perm)
            for name, mod in enc._modules.items():
                if name.startswith("block"):
                    self._block(st, mod, f"backbone._{branch}_enc.enc{s}.{name}", tsc, masks)
            return st

        def dec_stage(st, branch, s, tsc):
            dec = getattr(getattr(bb, f"_{branch}_dec"), f"dec{s}")
            st = self._unpooling(plan, st, dec.up)
            for name, mod in dec._modules.items():
                if name.startswith("block"):
                    self._block(st, mod, f"backbone._{branch}_dec.dec{s}.{name}", tsc, masks)
            return st

        if bb.condition:
            # the reference interleaves the encoders c0 n0 c1 n1 n2 c2 n3 n4 (ptv3.py:1781-1794): that fixes which shuffle a
            # stage consumes AND the order in which stochastic-depth masks are drawn; the two encoders are independent
            c_curves = shuffled(next(pi))
            n_curves = shuffled(next(pi))
            p_c1, p_n1, p_n2, p_c2, p_n3, p_n4 = (next(pi) for _ in range(6))
            cst = self._embedding(plan, c_feat, bb._c_embedding, c_curves, inv0)
            nst = self._embedding(plan, feat, bb._n_embedding, n_curves, inv0)
            cst = enc_stage(cst, "c", 0, c_cum, None, t_scene)
            nst = enc_stage(nst, "n", 0, n_cum, None, None)
            cst = enc_stage(cst, "c", 1, c_cum, p_c1, t_scene)
            nst = enc_stage(nst, "n", 1, n_cum, p_n1, None)
            nst = enc_stage(nst, "n", 2, n_cum, p_n2, None)
            cst = enc_stage(cst, "c", 2, c_cum, p_c2, t_scene)
            nst = enc_stage(nst, "n", 3, n_cum, p_n3, None)
            nst = enc_stage(nst, "n", 4, n_cum, p_n4, None)
            # fusion (ptv3.py:1332-1337).  Bidirectional: cross_block1(c <- n) first - the n point leaves it holding
            # kv_norm1(n + kv_cpe(n)), which is what cross_block2 then takes as its q point, and the c point cross_block2 and the
            # c-decoder read is cross_block1's output
            if bb._tm_dec0.tm_bidirectional:
                self._cross_block(cst, nst, bb._tm_dec0.cross_block1, "backbone._tm_dec0.cross_block1", masks)
            self._cross_block(nst, cst, bb._tm_dec0.cross_block2, "backbone._tm_dec0.cross_block2", masks)
            for s in reversed(range(bb.c_num_stages - 1)):
                cst = dec_stage(cst, "c", s, t_scene)
            c_phys = F.linear(cst.x, bb._c_head.weight, bb._c_head.bias) if isinstance(bb._c_head, torch.nn.Linear) else cst.x
            point["c_pred"] = c_phys[inv0]
        else:
            nst = self._embedding(plan, feat, bb._n_embedding, shuffled(next(pi)), inv0)
            for s in range(bb.n_num_stages):
                nst = enc_stage(nst, "n", s, n_cum, next(pi) if s > 0 else None, None)
        for s in reversed(range(bb.n_num_stages - 1)):
            nst = dec_stage(nst, "n", s, None)
        n_phys = F.linear(nst.x, bb._n_head.weight, bb._n_head.bias) if isinstance(bb._n_head, torch.nn.Linear) else nst.x
        point["n_pred"] = n_phys[inv0]
        if rep is not None:  # folded duplicates: back to the caller's N rows (and its offsets, which the criteria sample by)
            point["offset"] = offset_in
            runs = fold_runs(rep, n) if self.det else None
            for k in ("n_pred", "c_pred", "c_target"):
                if point.get(k) is not None:
                    if runs is not None and point[k].requires_grad:
                        point[k] = _GatherRuns.apply(point[k], rep, runs[1], runs[0])
                    else:
                        point[k] = point[k][rep]
        point["n_target"] = input_dict["segment"]
        if self.train_loss == "fused":
            if self.fused_criteria is None:
                self.fused_criteria = build_criteria(self.model.criteria_cfg, self.model.loss_type, self.model.task_num, "fused")
            loss = self.fused_criteria(point)
        else:
            loss = self.criteria(point)
        return dict(loss=loss, n_pred=point["n_pred"], c_pred=point.get("c_pred"), c_target=point.get("c_target"))
