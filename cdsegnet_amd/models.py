"""Model-registry surface of the hot path: ``DefaultSegmentorV2`` + ``"PT-v3m1"``.

Same registry names, constructor kwargs and ``state_dict`` schema as the reference
(ref: pointcept/models/default.py:13-72, pointcept/models/point_transformer_v3/
point_transformer_v3m1_base.py:1340-1755), so released checkpoints load ``strict=True`` and
``tools/test_*.py`` can call ``model.inference(input_dict, eval=False, noise_level=...)``
unchanged.  The ``nn.Module`` tree below only OWNS parameters (names/shapes = the reference's);
the forward pass is executed by ``cdsegnet_amd.engine`` on hand-written HIP kernels.
Options that every shipped CDSegNet config leaves off (RPE, PDNorm, Restormer fusion,
cls_mode) are accepted by the constructors and rejected loudly.  The switches the shipped configs spell out
next to their defaults are built: learned fusion scales (``tm_feat``), bidirectional fusion
(``tm_bidirectional``) and the five skip-connection switches (``skip_connection_mode``,
``skip_connection_scale``, ``skip_connection_scale_i``, ``b_factor``, ``s_factor``).
"""
import math
import numbers
import threading
import warnings

import numpy as np
import torch
import torch.nn as nn

from .registry import MODELS, build_model


class PointSequential(nn.Module):
    """Named container with the reference's ``add`` (ref: pointcept/models/modules.py:19-56)."""

    def __init__(self, *args, **kwargs):
        super().__init__()
        for idx, m in enumerate(args):
            self.add_module(str(idx), m)
        for name, m in kwargs.items():
            if name in self._modules:
                raise ValueError("name exists.")
            self.add_module(name, m)

    def add(self, module, name=None):
        if name is None:
            name = str(len(self._modules))
            if name in self._modules:
                raise KeyError("name exists")
        self.add_module(name, module)

    def __len__(self):
        return len(self._modules)

    def __getitem__(self, idx):
        if not (-len(self) <= idx < len(self)):
            raise IndexError(f"index {idx} is out of range")
        return list(self._modules.values())[idx]


class SubMConv3d(nn.Module):
    """Parameter holder for spconv.SubMConv3d: weight (out, k, k, k, in) [spconv-2.x KRSC], bias (out)."""

    def __init__(self, in_channels, out_channels, kernel_size, bias=True, indice_key=None, padding=0):
        super().__init__()
        k = kernel_size
        self.in_channels, self.out_channels, self.kernel_size, self.indice_key = in_channels, out_channels, k, indice_key
        self.weight = nn.Parameter(torch.empty(out_channels, k, k, k, in_channels))
        fan_in = k * k * k * in_channels
        nn.init.uniform_(self.weight, -1 / math.sqrt(fan_in), 1 / math.sqrt(fan_in))
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels).uniform_(-1 / math.sqrt(fan_in), 1 / math.sqrt(fan_in)))
        else:
            self.register_parameter("bias", None)


class MLP(nn.Module):
    def __init__(self, in_channels, hidden_channels, out_channels):
        super().__init__()
        self.fc1 = nn.Linear(in_channels, hidden_channels)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden_channels, out_channels)


def _reject(**flags):
    for name, (value, allowed) in flags.items():
        if value != allowed:
            raise NotImplementedError(
                f"{name}={value!r}: this option is disabled in every shipped CDSegNet config and is not part of the "
                f"MI355X hot path (supported: {allowed!r})")


def _rate(name, value):
    """A dropout rate: a real number in [0, 1), kept as a plain float (no parameter, no buffer)."""
    if isinstance(value, bool) or not isinstance(value, numbers.Real) or not 0.0 <= float(value) < 1.0:
        raise ValueError(f"{name}={value!r}: a dropout rate is a real number in [0, 1)")
    return float(value)


class SerializedAttention(nn.Module):
    def __init__(self, channels, num_heads, patch_size, qkv_bias=True, qk_scale=None, order_index=0,
                 enable_flash=True, attn_drop=0.0, proj_drop=0.0):
        super().__init__()
        # train mode only (train_graph.py): attn_drop on the attention probabilities (ptv3.py:282-288), proj_drop behind proj
        # (:293-294); the masks are the library's (include/cdseg.h "dropout")
        self.attn_drop, self.proj_drop = _rate("attn_drop", attn_drop), _rate("proj_drop", proj_drop)
        assert channels % num_heads == 0
        if channels // num_heads != 16:
            raise NotImplementedError("the HIP attention kernels are specialised for head dim 16 (C/H == 16)")
        if patch_size > 1024:
            raise NotImplementedError("patch_size > 1024")
        self.channels, self.num_heads, self.patch_size = channels, num_heads, patch_size
        self.scale = qk_scale or (channels // num_heads) ** -0.5
        self.order_index = order_index
        self.enable_flash = enable_flash
        self.qkv = nn.Linear(channels, channels * 3, bias=qkv_bias)
        self.proj = nn.Linear(channels, channels)


class Block(nn.Module):
    """ref: ptv3.py:326-428."""

    def __init__(self, channels, num_heads, patch_size=48, mlp_ratio=4.0, qkv_bias=True, qk_scale=None,
                 order_index=0, cpe_indice_key=None, enable_flash=True, T_dim=-1, pre_norm=True, drop_path=0.0,
                 attn_drop=0.0, proj_drop=0.0):
        super().__init__()
        _reject(pre_norm=(pre_norm, True))
        self.channels, self.T_dim = channels, T_dim
        # proj_drop is also the rate of the two MLP drops, behind the activation and behind fc2 (ptv3.py:316-322, :381)
        self.attn_drop, self.proj_drop = _rate("attn_drop", attn_drop), _rate("proj_drop", proj_drop)
        self.drop_prob = float(drop_path)  # stochastic depth of the training forward (timm DropPath, ptv3.py:392-394): rows
        self.cpe = PointSequential(
            SubMConv3d(channels, channels, 3, bias=True, indice_key=cpe_indice_key),
            nn.Linear(channels, channels),
            nn.LayerNorm(channels),
        )
        self.norm1 = PointSequential(nn.LayerNorm(channels))
        self.attn = SerializedAttention(channels, num_heads, patch_size, qkv_bias, qk_scale, order_index, enable_flash,
                                        attn_drop=self.attn_drop, proj_drop=self.proj_drop)
        self.norm2 = PointSequential(nn.LayerNorm(channels))
        self.mlp = PointSequential(MLP(channels, int(channels * mlp_ratio), channels))
        self.drop_path = PointSequential(nn.Identity())
        if T_dim != -1:
            self.t_mlp = nn.Linear(T_dim, channels)


class SerializedPooling(nn.Module):
    """ref: ptv3.py:431-555."""

    def __init__(self, in_channels, out_channels, stride=2, reduce="max", shuffle_orders=True, T_dim=-1):
        super().__init__()
        assert stride == 2 ** (math.ceil(stride) - 1).bit_length()
        _reject(reduce=(reduce, "max"))
        self.in_channels, self.out_channels, self.stride, self.T_dim = in_channels, out_channels, stride, T_dim
        self.shuffle_orders = shuffle_orders
        self.proj = nn.Linear(in_channels, out_channels)
        self.norm = PointSequential(nn.BatchNorm1d(out_channels, eps=1e-3, momentum=0.01))
        self.act = PointSequential(nn.GELU())


_B_FACTOR_WARNED = False


def _warn_b_factor():
    """Once per process: what a b_factor != 1 does."""
    global _B_FACTOR_WARNED
    if not _B_FACTOR_WARNED:
        _B_FACTOR_WARNED = True
        warnings.warn("b_factor != 1 has the reference's effect, which is none: freeU takes the channel count from the channel "
                      "MEAN (one channel), so C_num = 0 and no backbone channel is scaled "
                      "(point_transformer_v3m1_base.py:81-96).  It only switches the skip filter on, with s_factor as given")


class SerializedUnpooling(nn.Module):
    """ref: ptv3.py:558-630."""

    def __init__(self, in_channels, skip_channels, out_channels, skip_connection_mode="add", b=1.0, s=1.0,
                 skip_connection_scale=False, skip_connection_scale_i=False):
        super().__init__()
        for name, v in (("b", b), ("s", s)):
            if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v):
                raise ValueError(f"SerializedUnpooling({name}={v!r}): a FreeU factor is a finite number")
        # FreeU (ptv3.py:68-100, :614-620).  s: the Fourier filter of the skip feature (csrc/skip.hip).  b has the reference's
        # effect, which is none: freeU reads the channel count AFTER the channel mean has made that dimension 1 (ptv3.py:81-84),
        # so C_num = 0 and `b_feat[:, :0]` scales no channel (:96); b != 1 only switches the filter on with whatever s is
        self.b, self.s = float(b), float(s)
        if self.b != 1.0:
            _warn_b_factor()
        bn = lambda c: nn.BatchNorm1d(c, eps=1e-3, momentum=0.01)  # noqa: E731
        self.proj = PointSequential(nn.Linear(in_channels, out_channels), bn(out_channels), nn.GELU())
        self.proj_skip = PointSequential(nn.Linear(skip_channels, out_channels), bn(out_channels), nn.GELU())
        self.skip_connection_mode = skip_connection_mode
        self.skip_connection_scale = skip_connection_scale
        self.skip_connection_scale_i = skip_connection_scale_i
        if skip_connection_mode == "cat":
            self.proj_cat = PointSequential(nn.Linear(out_channels * 2, out_channels))
        elif skip_connection_mode != "add":
            raise ValueError(f"skip_connection_mode={skip_connection_mode!r}")

    @property
    def skip_scale(self):
        """f of ptv3.py:607-611: 2^-0.5 (skip_connection_scale) times 0.8^(i-1) (skip_connection_scale_i; note that False still
        scales by 0.8^(0-1) = 1.25).  'cat' folds it into proj_cat's weight, 'add' applies it in cdseg_skip_merge."""
        f = 2 ** -0.5 if self.skip_connection_scale else 1.0
        if self.skip_connection_scale_i is not None:
            f *= 0.8 ** (int(self.skip_connection_scale_i) - 1)
        return f

    @property
    def skip_filter(self):
        """The s of the Fourier filter this module runs, or None: the reference filters when b != 1 or s != 1 (ptv3.py:614);
        with s == 1 the filter is the identity (k = 0) and no launch is spent on it."""
        return self.s if float(np.float32(self.s)) != 1.0 else None


class Embedding(nn.Module):
    """ref: ptv3.py:633-663."""

    def __init__(self, in_channels, embed_channels):
        super().__init__()
        self.in_channels, self.embed_channels = in_channels, embed_channels
        self.stem = PointSequential(conv=SubMConv3d(in_channels, embed_channels, 5, bias=False, indice_key="stem",
                                                    padding=1))
        self.stem.add(nn.BatchNorm1d(embed_channels, eps=1e-3, momentum=0.01), name="norm")
        self.stem.add(nn.GELU(), name="act")


class SerializedCrossAttention(nn.Module):
    """ref: ptv3.py:859-1055."""

    def __init__(self, q_channels, kv_channels, num_heads, q_patch_size, kv_patch_size, qkv_bias=True, qk_scale=None,
                 order_index=0, enable_flash=True, attn_drop=0.0, proj_drop=0.0):
        super().__init__()
        assert q_channels % num_heads == 0 and kv_channels % num_heads == 0
        self.attn_drop, self.proj_drop = _rate("attn_drop", attn_drop), _rate("proj_drop", proj_drop)  # (ptv3.py:1038-1053)
        if q_channels // num_heads != 16:
            raise NotImplementedError("the HIP attention kernels are specialised for head dim 16 (C/H == 16)")
        self.q_channels, self.kv_channels, self.num_heads = q_channels, kv_channels, num_heads
        self.q_patch_size, self.kv_patch_size = q_patch_size, kv_patch_size
        self.scale = qk_scale or (q_channels // num_heads) ** -0.5
        self.order_index, self.enable_flash = order_index, enable_flash
        self.q = nn.Linear(q_channels, q_channels, bias=qkv_bias)
        self.kv = nn.Linear(kv_channels, q_channels * 2, bias=qkv_bias)
        self.proj = nn.Linear(q_channels, q_channels)


# tm_feat mode -> (feat_scale per channel (1, C) or scalar (1,), its initial value)   (ptv3.py:1091-1103)
FUSION_MODES = {"channel_scale": (True, 1.0), "b_channel_scale": (True, 0.5), "lr_scale": (False, 1.0), "b_lr_scale": (False, 0.5)}


def gate_vectors(mode, p, c):
    """(alpha, gamma), two (c,) vectors in p's dtype, of the learned fusion gate `mode` with parameter p ((1,) or (1, c)):
    y = alpha * q_shortcut + gamma * attn (ptv3.py:1196-1206).  The sigmoid belongs to the two channel modes only; the two b
    modes blend (alpha = 1 - gamma).  Differentiable in p."""
    g = (torch.sigmoid(p) if FUSION_MODES[mode][0] else p).reshape(-1).expand(c)
    return (1 - g if mode.startswith("b_") else torch.ones_like(g)), g


def fusion_gate(cb, dtype=torch.float32):
    """(alpha, gamma) of CrossBlock `cb`, learned (`gate_vectors` of its feat_scale) or a number f (alpha = 1, gamma = f)."""
    if isinstance(cb.tm_feat, float):
        g = torch.full((cb.q_channels,), cb.tm_feat, dtype=dtype)
        return torch.ones_like(g), g
    return gate_vectors(cb.tm_feat, cb.feat_scale.to(dtype), cb.q_channels)


class CrossBlock(nn.Module):
    """ref: ptv3.py:1058-1223."""

    def __init__(self, q_channels, kv_channels, num_heads, q_patch_size, kv_patch_size, mlp_ratio=4.0, qkv_bias=True,
                 qk_scale=None, order_index=0, q_cpe_indice_key=None, kv_cpe_indice_key=None, enable_flash=True,
                 tm_feat=1.0, drop_path=0.0, attn_drop=0.0, proj_drop=0.0):
        super().__init__()
        self.drop_prob = float(drop_path)
        self.attn_drop, self.proj_drop = _rate("attn_drop", attn_drop), _rate("proj_drop", proj_drop)
        # the fusion gate (ptv3.py:1091-1103): a number f, or one of FUSION_MODES with a learned `feat_scale` - registered
        # FIRST, like the reference's, so that the state_dict keys keep its order
        if isinstance(tm_feat, str):
            if tm_feat not in FUSION_MODES:
                raise NotImplementedError(f"tm_feat={tm_feat!r}: the learned fusion scales are {', '.join(map(repr, FUSION_MODES))}")
            per_channel, init = FUSION_MODES[tm_feat]
            self.tm_feat = tm_feat
            self.feat_scale = nn.Parameter(torch.full((1, q_channels) if per_channel else (1,), init))
        elif isinstance(tm_feat, (int, float)):
            self.tm_feat = float(tm_feat)
        else:
            raise NotImplementedError(f"tm_feat={tm_feat!r}: a number or one of {', '.join(map(repr, FUSION_MODES))}")
        self.q_channels, self.kv_channels = q_channels, kv_channels
        self.q_cpe = PointSequential(SubMConv3d(q_channels, q_channels, 3, bias=True, indice_key=q_cpe_indice_key),
                                     nn.Linear(q_channels, q_channels), nn.LayerNorm(q_channels))
        self.kv_cpe = PointSequential(SubMConv3d(kv_channels, kv_channels, 3, bias=True, indice_key=kv_cpe_indice_key),
                                      nn.Linear(kv_channels, kv_channels), nn.LayerNorm(kv_channels))
        self.q_norm1 = PointSequential(nn.LayerNorm(q_channels))
        self.kv_norm1 = PointSequential(nn.LayerNorm(kv_channels))
        self.attn = SerializedCrossAttention(q_channels, kv_channels, num_heads, q_patch_size, kv_patch_size, qkv_bias,
                                             qk_scale, order_index, enable_flash, attn_drop=self.attn_drop,
                                             proj_drop=self.proj_drop)
        self.q_norm2 = PointSequential(nn.LayerNorm(q_channels))
        self.mlp = PointSequential(MLP(q_channels, int(q_channels * mlp_ratio), q_channels))
        self.drop_path = PointSequential(nn.Identity())


class TransferModule(nn.Module):
    """ref: ptv3.py:1225-1337: cross_block2 (n <- c), and in front of it, with tm_bidirectional, cross_block1 (c <- n) - the
    same block with the roles swapped (:1261-1295), registered first."""

    def __init__(self, tm_bidirectional=False, kv_num_heads=None, kv_drop_path=0.0, **kw):
        super().__init__()
        self.tm_bidirectional = bool(tm_bidirectional)
        self.attn_drop, self.proj_drop = _rate("attn_drop", kw.get("attn_drop", 0.0)), _rate("proj_drop", kw.get("proj_drop", 0.0))
        if self.tm_bidirectional:
            swapped = dict(kw, q_channels=kw["kv_channels"], kv_channels=kw["q_channels"], num_heads=kv_num_heads,
                           q_patch_size=kw["kv_patch_size"], kv_patch_size=kw["q_patch_size"],
                           q_cpe_indice_key=kw.get("kv_cpe_indice_key"), kv_cpe_indice_key=kw.get("q_cpe_indice_key"),
                           drop_path=kv_drop_path)
            self.cross_block1 = CrossBlock(**swapped)
        self.cross_block2 = CrossBlock(**kw)


@MODELS.register_module("PT-v3m1")
class PointTransformerV3(nn.Module):
    """ref: ptv3.py:1340-1755 (constructor) / :1757-1846 (forward, run by engine.backbone_forward)."""

    def __init__(
        self,
        c_in_channels=6, n_in_channels=6, order=("z", "z_trans"),
        c_stride=(4, 4), c_enc_depths=(2, 2, 2), c_enc_channels=(32, 64, 128), c_enc_num_head=(2, 4, 8),
        c_enc_patch_size=(1024, 1024, 1024), c_dec_depths=(2, 2), c_dec_channels=(64, 64), c_dec_num_head=(4, 4),
        c_dec_patch_size=(1024, 1024),
        n_stride=(2, 2, 2, 2), n_enc_depths=(2, 2, 2, 6, 2), n_enc_channels=(32, 64, 128, 256, 512),
        n_enc_num_head=(2, 4, 8, 16, 32), n_enc_patch_size=(48, 48, 48, 48, 48), n_dec_depths=(2, 2, 2, 2),
        n_dec_channels=(64, 64, 128, 256), n_dec_num_head=(4, 4, 8, 16), n_dec_patch_size=(48, 48, 48, 48),
        mlp_ratio=4, qkv_bias=True, qk_scale=None, attn_drop=0.0, proj_drop=0.0, drop_path=0.3, pre_norm=True,
        shuffle_orders=True, enable_rpe=False, enable_flash=True, upcast_attention=True, upcast_softmax=True,
        cls_mode=False, pdnorm_bn=False, pdnorm_ln=False, pdnorm_decouple=True, pdnorm_adaptive=False,
        pdnorm_affine=True, pdnorm_conditions=("ScanNet", "S3DIS", "Structured3D"),
        num_classes=20, T_dim=128, tm_bidirectional=False, tm_feat=1.0, tm_restomer=False, condition=False,
        skip_connection_mode="add", b_factor=(1.0, 1.0, 1.0, 1.0), s_factor=(1.0, 1.0, 1.0, 1.0),
        skip_connection_scale=False, skip_connection_scale_i=False,
    ):
        super().__init__()
        _reject(enable_rpe=(enable_rpe, False), cls_mode=(cls_mode, False), pdnorm_bn=(pdnorm_bn, False),
                pdnorm_ln=(pdnorm_ln, False),
                tm_restomer=(tm_restomer, False), pre_norm=(pre_norm, True))
        self.order = [order] if isinstance(order, str) else list(order)
        for o in self.order:
            if o not in ("z", "z-trans", "hilbert", "hilbert-trans"):
                raise NotImplementedError(f"serialization order {o!r}")
        self.shuffle_orders = shuffle_orders
        self.num_classes, self.T_dim, self.condition = num_classes, T_dim, condition
        self.enable_flash = enable_flash
        self.n_num_stages = len(n_enc_depths)
        self.n_stride, self.c_stride = tuple(n_stride), tuple(c_stride)
        assert self.n_num_stages == len(n_stride) + 1 == len(n_enc_channels) == len(n_enc_num_head) == len(n_enc_patch_size)
        assert self.n_num_stages == len(n_dec_depths) + 1 == len(n_dec_channels) + 1 == len(n_dec_num_head) + 1

        no = len(self.order)
        self.attn_drop, self.proj_drop = _rate("attn_drop", attn_drop), _rate("proj_drop", proj_drop)
        blk = dict(mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, enable_flash=enable_flash,
                   attn_drop=self.attn_drop, proj_drop=self.proj_drop)

        def rates(depths):  # stochastic-depth schedule over the blocks of one coder (ptv3.py:1459-1466)
            return [float(x) for x in torch.linspace(0, drop_path, sum(depths))]

        def stage_rates(all_rates, depths, s, reverse=False):
            r = all_rates[sum(depths[:s]): sum(depths[:s + 1])]
            return r[::-1] if reverse else r  # (decoders: ptv3.py:1515-1518)
        n_enc_dp, n_dec_dp = rates(n_enc_depths), rates(n_dec_depths)
        self._n_embedding = Embedding(n_in_channels, n_enc_channels[0])
        self._n_enc = PointSequential()
        for s in range(self.n_num_stages):
            enc = PointSequential()
            if s > 0:
                enc.add(SerializedPooling(n_enc_channels[s - 1], n_enc_channels[s], stride=n_stride[s - 1]), name="down")
            for i in range(n_enc_depths[s]):
                enc.add(Block(n_enc_channels[s], n_enc_num_head[s], n_enc_patch_size[s], order_index=i % no,
                              cpe_indice_key=f"stage{s}", drop_path=stage_rates(n_enc_dp, n_enc_depths, s)[i], **blk),
                        name=f"block{i}")
            if len(enc) != 0:
                self._n_enc.add(enc, name=f"enc{s}")
        self._n_dec = PointSequential()
        n_dec_channels = list(n_dec_channels) + [n_enc_channels[-1]]
        for s in reversed(range(self.n_num_stages - 1)):
            dec = PointSequential()
            dec.add(SerializedUnpooling(n_dec_channels[s + 1], n_enc_channels[s], n_dec_channels[s],
                                        skip_connection_mode="cat" if skip_connection_mode == "cat_all" else "add",
                                        b=b_factor[s], s=s_factor[s],
                                        skip_connection_scale_i=(s + 1) if skip_connection_scale_i else None),
                    name="up")
            for i in range(n_dec_depths[s]):
                dec.add(Block(n_dec_channels[s], n_dec_num_head[s], n_dec_patch_size[s], order_index=i % no,
                              cpe_indice_key=f"stage{s}", drop_path=stage_rates(n_dec_dp, n_dec_depths, s, True)[i], **blk),
                        name=f"block{i}")
            self._n_dec.add(dec, name=f"dec{s}")
        self._n_head = nn.Linear(n_dec_channels[0], num_classes) if num_classes > 0 else nn.Identity()

        if self.condition:
            self.c_num_stages = len(c_enc_depths)
            assert self.c_num_stages == len(c_stride) + 1 == len(c_enc_channels) == len(c_enc_num_head)
            c_enc_dp, c_dec_dp = rates(c_enc_depths), rates(c_dec_depths)
            self._c_embedding = Embedding(c_in_channels, c_enc_channels[0])
            if T_dim != -1:
                self.fc_t1 = nn.Linear(T_dim, 4 * T_dim)
                self.fc_t2 = nn.Linear(4 * T_dim, T_dim)
            self._c_enc = PointSequential()
            for s in range(self.c_num_stages):
                enc = PointSequential()
                if s > 0:
                    enc.add(SerializedPooling(c_enc_channels[s - 1], c_enc_channels[s], stride=c_stride[s - 1],
                                              T_dim=T_dim), name="down")
                for i in range(c_enc_depths[s]):
                    enc.add(Block(c_enc_channels[s], c_enc_num_head[s], c_enc_patch_size[s], order_index=i % no,
                                  cpe_indice_key=f"stage{s}", T_dim=T_dim,
                                  drop_path=stage_rates(c_enc_dp, c_enc_depths, s)[i], **blk), name=f"block{i}")
                if len(enc) != 0:
                    self._c_enc.add(enc, name=f"enc{s}")
            self._c_dec = PointSequential()
            c_dec_channels = list(c_dec_channels) + [c_enc_channels[-1]]
            for s in reversed(range(self.c_num_stages - 1)):
                dec = PointSequential()
                dec.add(SerializedUnpooling(c_dec_channels[s + 1], c_enc_channels[s], c_dec_channels[s],
                                            skip_connection_mode="add" if skip_connection_mode == "add" else "cat",
                                            skip_connection_scale=skip_connection_scale), name="up")
                for i in range(c_dec_depths[s]):
                    dec.add(Block(c_dec_channels[s], c_dec_num_head[s], c_dec_patch_size[s], order_index=i % no,
                                  cpe_indice_key=f"stage{s}", T_dim=T_dim,
                                  drop_path=stage_rates(c_dec_dp, c_dec_depths, s, True)[i], **blk), name=f"block{i}")
                self._c_dec.add(dec, name=f"dec{s}")
            self._c_head = nn.Linear(n_dec_channels[0], c_in_channels) if num_classes > 0 else nn.Identity()
            self._tm_dec0 = TransferModule(
                q_channels=n_dec_channels[-1], kv_channels=c_dec_channels[-1], num_heads=n_enc_num_head[-1],
                q_patch_size=n_enc_patch_size[-1], kv_patch_size=c_enc_patch_size[-1], mlp_ratio=mlp_ratio,
                qkv_bias=qkv_bias, qk_scale=qk_scale, order_index=0, q_cpe_indice_key="stage2",
                kv_cpe_indice_key="stage2", enable_flash=enable_flash, tm_feat=tm_feat,
                attn_drop=self.attn_drop, proj_drop=self.proj_drop,
                drop_path=c_enc_dp[2] if len(c_enc_dp) > 2 else 0.0,  # (ptv3.py:1735-1736)
                tm_bidirectional=tm_bidirectional, kv_num_heads=c_enc_num_head[-1],
                kv_drop_path=c_enc_dp[2] if len(c_enc_dp) > 2 else 0.0)

    def forward(self, c_point=None, n_point=None):
        raise NotImplementedError(
            "PT-v3m1 on MI355X is driven through DefaultSegmentorV2.inference (cdsegnet_amd.engine); "
            "the training forward is outside the single-step-inference hot path")


def calc_t_emb_table(T, t_emb_dim):
    """Rows t = -1..T-1 (row index t + 1) of the sinusoidal timestep embedding, built once on the host with
    the very ops the reference uses per call (ref: pointcept/utils/comm.py:21-39), so a row is bit-identical
    to ``calc_t_emb(t * ones((N,1)), dim)[0]``."""
    assert t_emb_dim % 2 == 0
    half = t_emb_dim // 2
    c = np.log(10000) / (half - 1)
    f = torch.exp(torch.arange(half) * -c)
    ts = torch.arange(-1, T, dtype=torch.int64)[:, None]  # row 0 is t = -1 (last DDIM step, default.py:224-226)
    e = ts * f
    return torch.cat((torch.sin(e), torch.cos(e)), 1)


def diffusion_betas(kind, start, stop, T):
    """ref: default.py:127-189 (only the schedules the shipped configs use)."""
    if kind == "linear":
        scale = 1000 / T
        return torch.linspace(scale * start, scale * stop, T, dtype=torch.float64)
    if kind == "cosine":
        s = 0.008
        t = torch.linspace(start, stop, T + 1, dtype=torch.float64) / T
        ac = torch.cos((t + s) / (1 + s) * math.pi * 0.5) ** 2
        ac = ac / ac[0]
        return torch.clip(1 - ac[1:] / ac[:-1], 0, 0.999)
    raise NotImplementedError(f"noise_schedule={kind!r}")


def collate_device(dicts):
    """Pointcept's collate_fn for already-resident scenes (datasets/utils.py:34-39): concatenate along the point axis,
    offsets become cumulative.  Host-side sizes ride along in ``offset_host`` (no device sync)."""
    if len(dicts) == 1:
        return dicts[0]
    out = {}
    for k in ("coord", "grid_coord", "feat"):
        out[k] = torch.cat([d[k] for d in dicts], 0)
    ends, base = [], 0
    for d in dicts:
        oh = d["offset_host"] if "offset_host" in d else d["offset"].cpu().tolist()
        ends += [base + int(v) for v in oh]
        base = ends[-1]
    out["offset"] = torch.tensor(ends, dtype=torch.int64, device=dicts[0]["feat"].device)
    out["offset_host"] = ends
    return out


@MODELS.register_module()
class DefaultSegmentorV2(nn.Module):
    """CNF wrapper (ref: default.py:13-494).  ``inference`` is the single-step path (SSI)."""

    def __init__(self, backbone=None, criteria=None, loss_type="EW", task_num=2, num_classes=20, T=1000,
                 beta_start=0.0001, beta_end=0.02, noise_schedule="linear", T_dim=128, dm=False, dm_input="xt",
                 dm_target="noise", dm_min_snr=None, condition=False, c_in_channels=6):
        super().__init__()
        self.backbone = build_model(backbone)
        self.criteria_cfg = criteria  # losses are outside the inference path (tester passes eval=False)
        self.loss_type, self.task_num = loss_type, task_num
        self.num_classes, self.T, self.T_dim = num_classes, T, T_dim
        self.beta_start, self.beta_end, self.noise_schedule = beta_start, beta_end, noise_schedule
        self.condition, self.dm, self.dm_input, self.dm_target = condition, dm, dm_input, dm_target
        self.dm_min_snr, self.c_in_channels = dm_min_snr, c_in_channels
        if self.dm:
            # diffusion tables: plain attributes like the reference's (default.py:57-72); unused by SSI
            beta = diffusion_betas(noise_schedule, beta_start, beta_end, T)
            alpha = 1 - beta
            self.Beta, self.Alpha = beta.float(), alpha.float()
            self.Alpha_bar = torch.cumprod(alpha, 0).float()
        if T_dim != -1:
            self.t_emb_table = calc_t_emb_table(T, T_dim)  # (T, T_dim) host table, uploaded on first use
        # engine knobs (not part of the reference API)
        # "fp16+head" (default) | "fp16" | "bf16+head" | "bf16": 16-bit MFMA operands / activations (IEEE half or bfloat16),
        # fp32 accumulation and residual stream, "+head" = seg heads in exact fp32 | "fp32": exact-fp32 MFMA everywhere
        self.precision = "fp16+head"
        # training forward: "fp32" (default: exact fp32) | "fp16-attn" | "bf16-attn": the attention core (forward and backward,
        # self and cross attention) in IEEE half / bfloat16 like the reference's flash-attention path, everything else fp32;
        # "fp16-amp" | "bf16-amp": the reference's AMP setting (enable_amp = True): that attention core, and every trunk Linear
        # and sparse conv (forward, data gradient, weight gradient) on 16-bit products with fp32 accumulation and fp32 outputs;
        # read at every forward(), anything else raises ValueError there
        self.train_precision = "fp32"
        # training backward with a fixed fp32 summation order (bit-reproducible gradients; cdsegnet_amd/train_graph.py):
        # None (default) = follow torch.are_deterministic_algorithms_enabled() | True | False; read at every forward(),
        # not part of the state_dict
        self.train_deterministic = None
        # the two label terms of the criteria (cross entropy + Lovasz): "torch" (default: cdsegnet_amd/losses.py's torch ops) |
        # "fused": one HIP loss, forward and backward, where the configured pair allows it (losses.FusedCriteria; sort ties by
        # ascending row index); read at every forward() and by the loss of inference(eval=True), anything else raises
        # ValueError there; not part of the state_dict
        self.train_loss = "torch"
        # train-mode BatchNorm1d + GELU sites and the pooling maximum of the training forward: "torch" (default: torch device
        # ops, statistics of this process's rows) | "fused": the kernels of csrc/norm.hip (fp64 statistics in a fixed order;
        # nn.SyncBatchNorm modules - convert_sync_batchnorm, cfg.sync_bn - get statistics over all ranks of their process
        # group); read at every forward(), anything else raises ValueError there; not part of the state_dict
        self.train_norm = "torch"
        # every Block of the training forward: "autograd" (default: ~20 autograd nodes over the library's kernels with torch
        # device ops between them) | "native": ONE autograd node per Block whose forward and backward are one library call
        # each (csrc/trainblock.hip: all launches issued from C++, the torch glue as HIP row kernels); read at every
        # forward(), anything else raises ValueError there; not part of the state_dict
        self.train_block = "autograd"
        # training batches whose voxels hold more than one point (Mix3D, mix_prob = 0.8 in the shipped configs): "fold"
        # (default: the network runs on the first point of every voxel, the other points read its prediction) | "rows": every
        # point is a row of its own everywhere but in the sparse convs, which read the first point of a voxel
        # (engine.RowLevel); no effect on a batch without shared voxels; read at every forward(), anything else raises
        # ValueError there; not part of the state_dict
        self.train_mix3d = "fold"
        self._lanes = {}
        self.noise_source = "torch_cpu"  # "torch_cpu" replays the reference's CPU-generator draws | "device"
        # noise_level jitter: "torch_cpu" = the CPU-run reference's draw order (golden vectors) | "device" = device
        # Philox, leaves the CPU generator alone like a GPU run of the reference does (engine.draw)
        self.feat_noise_source = "torch_cpu"
        # diagnostic (IEEE-half trunk): count clamped activations during `inference` (a few extra launches and one host
        # read per call; off by default) -> engine().saturation_count / .saturation_checked after the call
        self.count_saturation = False
        # a forward that is handed a plan (`plan=`) compares its grid_coord and offset with the ones the plan was built from
        # and raises CdsegError on a difference: one host read per forward, so off by default
        self.check_shared_geometry = False
        self._engine = None

    # -- engine cache management -------------------------------------------------------------
    def _drop_engine(self):
        self._engine = None
        self._train_graph = None

    def load_state_dict(self, *a, **k):
        self._drop_engine()
        return super().load_state_dict(*a, **k)

    def _apply(self, fn, *a, **k):
        self._drop_engine()
        return super()._apply(fn, *a, **k)

    def engine(self):
        from .engine import Engine
        if self._engine is None or self._engine.precision != self.precision:
            self._engine = Engine(self, self.precision)
        self._engine.count_saturation = bool(self.count_saturation)
        return self._engine

    # -- reference API -----------------------------------------------------------------------
    @torch.no_grad()
    def inference(self, input_dict, eval=True, noise_level=None, draws=None, plan=None):
        """ref: default.py:371-422.  Returns dict(seg_logits=(N, num_classes) fp32 on the input's device).
        ``draws`` (optional) injects the random draws: dict(noise=(N,c_in) tensor, perms=[8 x (4,)],
        feat_noise=(N,C) when noise_level is set); by default they are drawn from torch's CPU generator in
        the reference's consumption order, so ``torch.manual_seed`` reproduces the reference bit-for-bit.
        ``plan`` (optional): the result of ``model.plan`` on an input of the same geometry - the forward then builds no
        plan and makes no host read; same logits, bit for bit."""
        logits = self.engine().inference(input_dict, noise_level=noise_level, draws=draws, plan=plan)
        if eval:
            # ref: default.py:414-420 - the criteria in "eval" mode on the n-branch prediction only (the MSE term finds no
            # c_pred and contributes 0.0, losses/misc.py:53-54): cross entropy + Lovasz, summed whatever the loss_type
            from .losses import build_criteria
            point = dict(n_pred=logits, n_target=input_dict["segment"], loss_mode="eval")
            return dict(loss=build_criteria(self.criteria_cfg, self.loss_type, self.task_num, getattr(self, "train_loss", "torch"))(point), seg_logits=logits)
        return dict(seg_logits=logits)

    @torch.no_grad()
    def plan(self, input_dict):
        """The integer side of a forward - curve codes and orders, pooled levels, kernel maps, padding tables, slot plans -
        built once from ``grid_coord``, ``offset`` and ``offset_host`` for every forward over that geometry
        (``inference(..., plan=)``, ``inference_many(..., plans=)``): all fragments of one test-time augmentation hold one
        point per voxel over the same voxels in the same row order.  Keep the plan alive until the streams that consume it
        have been joined.  ``engine().plans_built`` counts the plans built so far."""
        return self.engine().shared_plan(input_dict)

    @torch.no_grad()
    def inference_many(self, input_dicts, lanes=4, noise_level=None, draws=None, threads=False, batch=1, plans=None):
        """Throughput form of ``inference`` for a sequence of INDEPENDENT scenes (the tester's loop over scenes /
        fragments, ref: engines/test.py:197-279): scene i runs on HIP stream ``lane[i % lanes]``, so up to ``lanes``
        scenes are in flight on the GPU.  The deep, latency-bound stages of one scene (a few hundred points, tens of
        workgroups) then overlap the throughput-bound 120k-point stages of another, and a scene's two host syncs
        (serialization depth, pooled sizes) only wait for its own lane.  ``threads=True`` issues every lane from its
        own host thread; measured SLOWER on CPython 3.10 (4.97 vs 4.24 ms per scene: ~500 short library calls per
        scene make the threads convoy on the GIL), so the default is one issuing thread.  Same kernels, same results
        as calling ``inference`` scene by scene: the random draws are taken up front, in scene order.
        ``batch`` > 1 additionally collates every ``batch`` consecutive scenes into ONE forward with cumulative
        ``offset`` s - the reference's own batching (datasets/utils.py:34-39; its nuScenes config tests 8 sweeps per
        GPU): launches and host work per scene drop by ``batch``.  A batched scene gets the logits the reference
        gives it inside that batch (the serialization depth and the order shuffles are per batch), not bit-for-bit
        those of a stand-alone call.
        ``plans`` (optional): one ``model.plan`` result per forward (per collated group when ``batch`` > 1; the same plan
        object may appear many times), built on the caller's current stream.
        Returns the list of output dicts (one per input scene), valid on the caller's current stream."""
        dicts = list(input_dicts)
        if not dicts:
            return []
        if batch > 1:
            groups = [dicts[i:i + batch] for i in range(0, len(dicts), batch)]
            outs = self.inference_many([collate_device(g) for g in groups], lanes=lanes, noise_level=noise_level,
                                       draws=draws, threads=threads, plans=plans)
            res = []
            for g, o in zip(groups, outs):
                pos = 0
                for d in g:
                    n = d["feat"].shape[0]
                    res.append(dict(seg_logits=o["seg_logits"][pos:pos + n]))
                    pos += n
            return res
        dev = dicts[0]["feat"].device
        eng = self.engine()
        if dev.type != "cuda" or lanes <= 1:
            return [self.inference(d, eval=False, noise_level=noise_level, draws=None if draws is None else draws[i],
                                   plan=None if plans is None else plans[i]) for i, d in enumerate(dicts)]
        eng.prepare(dev)
        all_draws = [draws[i] if draws is not None else eng.predraw(d, noise_level) for i, d in enumerate(dicts)]
        cur = torch.cuda.current_stream(dev)
        nl = min(int(lanes), len(dicts))
        streams = self._lanes.setdefault(dev.index, [])  # one pool per device: lanes must not outnumber hardware queues
        while len(streams) < nl:
            streams.append(torch.cuda.Stream(device=dev))
        ready = torch.cuda.Event()
        ready.record(cur)
        outs = [None] * len(dicts)
        errors = []

        def lane(j):
            try:
                torch.cuda.set_device(dev)  # the current device is per thread
                with torch.no_grad(), torch.cuda.stream(streams[j]):
                    streams[j].wait_event(ready)  # inputs produced on the caller's stream
                    for i in range(j, len(dicts), nl):
                        o = eng.inference(dicts[i], noise_level=noise_level, draws=all_draws[i],
                                          plan=None if plans is None else plans[i])
                        o.record_stream(cur)
                        outs[i] = dict(seg_logits=o)
            except BaseException as e:  # noqa: BLE001 - re-raised in the caller
                errors.append(e)

        fork, eng.fork_stage = eng.fork_stage, None  # concurrency comes from the lanes; no intra-scene fork
        try:
            if threads:
                workers = [threading.Thread(target=lane, args=(j,), name=f"cdseg-lane{j}") for j in range(nl)]
                for t in workers:
                    t.start()
                for t in workers:
                    t.join()
            else:  # one host thread, scenes issued round-robin over the lanes
                torch.cuda.set_device(dev)
                for st in streams[:nl]:
                    st.wait_event(ready)
                for i, d in enumerate(dicts):
                    with torch.cuda.stream(streams[i % nl]):
                        o = eng.inference(d, noise_level=noise_level, draws=all_draws[i],
                                          plan=None if plans is None else plans[i])
                    o.record_stream(cur)
                    outs[i] = dict(seg_logits=o)
        finally:
            eng.fork_stage = fork
        if errors:
            raise errors[0]
        for st in streams[:nl]:
            cur.wait_stream(st)
        return outs

    @torch.no_grad()
    def inference_ddim(self, input_dict, T=1000, step=1, report=10, eval=True, mode="avg", noise_level=None, draws=None,
                       plan=None, reuse_encoder=False):
        """Multi-step inference (ref: default.py:278-369): MSAI mode="avg", MSFI mode="final".  The step-invariant
        plan (serialization, kernel maps, slot plans) is built once and reused by all step+1 backbone calls, and the last
        call runs no c-decoder (nobody reads its noise estimate).

        ``reuse_encoder=True``: the n-branch stem and encoder - whose input, ``feat``, is the same in every step and which
        no timestep bias reaches - run ONCE, under the n-branch order shuffles of the first backbone call; every step then
        runs the c-branch, the cross block, the decoders and the heads.  The random draws are consumed exactly as without
        the flag (8 order shuffles per backbone call; the n-branch positions 1, 3, 4, 6, 7 of the later calls are drawn and
        ignored), and the result is bit for bit what the un-hoisted loop computes when those positions repeat the first
        call's draws - one of the outcomes the reference's protocol can draw.  What is given up: MSAI no longer averages
        over n-branch order shuffles (every step's n-encoder sees the first call's orders), only over the c-branch's
        shuffles and the diffusion steps.  No effect on a model with ``condition=False``.
        ``engine().msi_stats`` = dict(backbone_calls=, n_encoders=, c_decoders=) of the last call."""
        if T != self.T:
            raise ValueError("T differs from the model's diffusion length")
        if mode not in ("avg", "final"):
            raise ValueError(mode)
        logits = self.engine().inference_ddim(input_dict, step=step, mode=mode, noise_level=noise_level, draws=draws, plan=plan,
                                              reuse_encoder=reuse_encoder)
        if eval:  # ref: default.py:361-367
            from .losses import build_criteria
            point = dict(n_pred=logits, n_target=input_dict["segment"], loss_mode="eval")
            return dict(loss=build_criteria(self.criteria_cfg, self.loss_type, self.task_num, getattr(self, "train_loss", "torch"))(point), seg_logits=logits)
        return dict(seg_logits=logits)

    @torch.no_grad()
    def inference_ddim_many(self, input_dicts, step=1, mode="avg", lanes=4, noise_level=None, draws=None, plans=None, batch=1,
                            reuse_encoder=False):
        """Throughput form of ``inference_ddim`` for a sequence of independent scenes, the multi-step sibling of
        ``inference_many``: the whole step loop of scene i is issued on HIP stream ``lane[i % lanes]`` from one host thread, the
        random draws are taken up front in scene order (``engine().predraw(d, noise_level, step + 1, always_noise=True)``),
        and the lanes are joined before it returns.  ``batch`` > 1 collates every ``batch`` consecutive scenes into one
        multi-step forward; ``plans``: one ``model.plan`` result per forward.  Same kernels, same results as calling
        ``inference_ddim(d, step=step, mode=mode, eval=False, ...)`` scene by scene under the same draws, bit for bit.
        Returns the list of output dicts (one per input scene), valid on the caller's current stream."""
        if mode not in ("avg", "final"):
            raise ValueError(mode)
        if int(step) < 1:
            raise ValueError(f"step={step!r}: at least 1")
        dicts = list(input_dicts)
        if not dicts:
            return []
        if batch > 1:
            groups = [dicts[i:i + batch] for i in range(0, len(dicts), batch)]
            outs = self.inference_ddim_many([collate_device(g) for g in groups], step=step, mode=mode, lanes=lanes,
                                            noise_level=noise_level, draws=draws, plans=plans, reuse_encoder=reuse_encoder)
            res = []
            for g, o in zip(groups, outs):
                pos = 0
                for d in g:
                    n = d["feat"].shape[0]
                    res.append(dict(seg_logits=o["seg_logits"][pos:pos + n]))
                    pos += n
            return res
        dev = dicts[0]["feat"].device
        eng = self.engine()

        def one(i, d, dr):
            return eng.inference_ddim(d, step=step, mode=mode, noise_level=noise_level, draws=dr,
                                      plan=None if plans is None else plans[i], reuse_encoder=reuse_encoder)

        if dev.type != "cuda" or lanes <= 1:
            return [dict(seg_logits=one(i, d, None if draws is None else draws[i])) for i, d in enumerate(dicts)]
        eng.prepare(dev)
        # a model without the c-branch runs single-step inference whatever `step` says (Engine._inference_ddim)
        n_calls, always = (int(step) + 1, True) if self.backbone.condition else (1, False)
        all_draws = [draws[i] if draws is not None else eng.predraw(d, noise_level, n_calls, always)
                     for i, d in enumerate(dicts)]
        cur = torch.cuda.current_stream(dev)
        nl = min(int(lanes), len(dicts))
        streams = self._lanes.setdefault(dev.index, [])  # one pool per device: lanes must not outnumber hardware queues
        while len(streams) < nl:
            streams.append(torch.cuda.Stream(device=dev))
        ready = torch.cuda.Event()
        ready.record(cur)
        outs = [None] * len(dicts)
        fork, eng.fork_stage = eng.fork_stage, None  # concurrency comes from the lanes; no intra-scene fork
        try:
            torch.cuda.set_device(dev)
            for st in streams[:nl]:
                st.wait_event(ready)  # inputs produced on the caller's stream
            for i, d in enumerate(dicts):
                with torch.cuda.stream(streams[i % nl]):
                    o = one(i, d, all_draws[i])
                o.record_stream(cur)
                outs[i] = dict(seg_logits=o)
        finally:
            eng.fork_stage = fork
            for st in streams[:nl]:
                cur.wait_stream(st)
        return outs

    def forward(self, input_dict, draws=None):
        """Training forward (ref: default.py:424-493): returns dict(loss=...) under torch autograd - `loss.backward()` fills
        the `.grad` of this module's parameters like the reference's does (engines/train.py:216-271).  fp32, with a 16-bit
        attention core, or under AMP (16-bit Linears and sparse convs too; `train_precision`), on the HIP kernels behind torch.autograd.Functions: cdsegnet_amd/train_graph.py.
        `draws` replays recorded random draws."""
        from .train_graph import TrainGraph
        if getattr(self, "_train_graph", None) is None:
            self._train_graph = TrainGraph(self)
        # a training forward is followed by an optimizer step and updates the BatchNorm buffers: the inference engine's
        # prepared weights (16-bit casts, folded BatchNorm, fragment images) are rebuilt at the next inference() call
        self._engine = None
        out = self._train_graph.forward(input_dict, draws)
        return out if draws is not None else dict(loss=out["loss"])
