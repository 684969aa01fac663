"""Model hyper-parameters of the shipped CDSegNet configs, as data.

Values restate configs/{scannet,scannet200,nuscenes}/CDSegNet.py:15-138 of the
reference (the ``model = dict(...)`` block); only the keys the single-step
inference path reads are kept, plus the ones the constructors must accept.
"""
import copy

_BACKBONE = dict(
    type="PT-v3m1",
    c_in_channels=6,
    n_in_channels=6,
    order=("z", "z-trans", "hilbert", "hilbert-trans"),
    c_stride=(4, 4),
    c_enc_depths=(2, 2, 2),
    c_enc_channels=(32, 64, 128),
    c_enc_num_head=(2, 4, 8),
    c_enc_patch_size=(1024, 1024, 1024),
    c_dec_depths=(2, 2),
    c_dec_channels=(64, 64),
    c_dec_num_head=(4, 4),
    c_dec_patch_size=(1024, 1024),
    n_stride=(2, 2, 2, 2),
    n_enc_depths=(2, 2, 2, 6, 6),
    n_enc_channels=(32, 64, 128, 256, 512),
    n_enc_num_head=(2, 4, 8, 16, 32),
    n_enc_patch_size=(1024, 1024, 1024, 1024, 1024),
    n_dec_depths=(2, 2, 2, 2),
    n_dec_channels=(64, 64, 128, 256),
    n_dec_num_head=(4, 4, 8, 16),
    n_dec_patch_size=(1024, 1024, 1024, 1024),
    mlp_ratio=4,
    qkv_bias=True,
    qk_scale=None,
    attn_drop=0.0,
    proj_drop=0.0,
    drop_path=0.3,
    shuffle_orders=True,
    pre_norm=True,
    enable_rpe=False,
    enable_flash=True,
    upcast_attention=False,
    upcast_softmax=False,
    cls_mode=False,
    pdnorm_bn=False,
    pdnorm_ln=False,
    pdnorm_decouple=True,
    pdnorm_adaptive=False,
    pdnorm_affine=True,
    pdnorm_conditions=("ScanNet", "S3DIS", "Structured3D"),
    num_classes=20,
    T_dim=128,
    tm_bidirectional=False,
    tm_feat=1.0,
    tm_restomer=False,
    condition=True,
    skip_connection_mode="cat",
    b_factor=[1.0, 1.0, 1.0, 1.0],
    s_factor=[1.0, 1.0, 1.0, 1.0],
    skip_connection_scale=True,
    skip_connection_scale_i=False,
)

_MODEL = dict(
    type="DefaultSegmentorV2",
    backbone=_BACKBONE,
    criteria=None,
    loss_type="GLS",
    task_num=2,
    num_classes=20,
    T=1000,
    beta_start=0,
    beta_end=1000,
    noise_schedule="cosine",
    T_dim=128,
    dm=True,
    dm_input="xt",
    dm_target="noise",
    dm_min_snr=None,
    condition=True,
    c_in_channels=6,
)


def _fusion(b, tm_feat, tm_bidirectional):
    """The two Feature Fusion Module switches of every shipped config (`tm_feat = 1.0 # "channel_scale", "b_channel_scale",
    "lr_scale", "b_lr_scale", 1.0`, `tm_bidirectional = False`); the defaults leave the dict as it was."""
    b["tm_feat"], b["tm_bidirectional"] = tm_feat, bool(tm_bidirectional)


def _skip(b, skip_connection_mode, skip_connection_scale, skip_connection_scale_i, b_factor, s_factor):
    """The five skip-connection switches of every shipped config (`skip_connection_mode = "cat" # "cat", "add", "cat_all"`,
    `b_factor`, `s_factor`, `skip_connection_scale = True`, `skip_connection_scale_i = False`); None keeps the default."""
    if skip_connection_mode is not None:
        if skip_connection_mode not in ("cat", "add", "cat_all"):
            raise ValueError(f"skip_connection_mode={skip_connection_mode!r}")
        b["skip_connection_mode"] = skip_connection_mode
    if skip_connection_scale is not None:
        b["skip_connection_scale"] = bool(skip_connection_scale)
    if skip_connection_scale_i is not None:
        b["skip_connection_scale_i"] = bool(skip_connection_scale_i)
    for name, v in (("b_factor", b_factor), ("s_factor", s_factor)):
        if v is not None:
            if len(v) != 4:
                raise ValueError(f"{name}: one factor per n-decoder stage (4), got {v!r}")
            b[name] = [float(x) for x in v]


def cdsegnet_config(dataset="scannet", tm_feat=1.0, tm_bidirectional=False, skip_connection_mode=None,
                    skip_connection_scale=None, skip_connection_scale_i=None, b_factor=None, s_factor=None):
    """``model`` dict of configs/<dataset>/CDSegNet.py (criteria dropped: the tester
    calls inference(eval=False), test.py:216).  tm_feat / tm_bidirectional: the fusion ablation switches; skip_connection_* /
    b_factor / s_factor: the skip-connection switches (`_skip`)."""
    m = copy.deepcopy(_MODEL)
    b = m["backbone"]
    _fusion(b, tm_feat, tm_bidirectional)
    _skip(b, skip_connection_mode, skip_connection_scale, skip_connection_scale_i, b_factor, s_factor)
    if dataset == "scannet":
        pass
    elif dataset == "scannet200":
        # configs/scannet200/CDSegNet.py: 200 classes and - unlike scannet - a linear schedule 0.001 .. 0.005 (found by
        # running the reference's own config files: tests/golden/variant_schemas.json)
        m["num_classes"] = b["num_classes"] = 200
        m["beta_start"], m["beta_end"], m["noise_schedule"] = 0.001, 0.005, "linear"
    elif dataset == "nuscenes":
        # configs/nuscenes/CDSegNet.py:25-30,42
        m["num_classes"] = b["num_classes"] = 16
        m["c_in_channels"] = b["c_in_channels"] = 4
        b["n_in_channels"] = 4
        m["beta_start"], m["beta_end"], m["noise_schedule"] = 0.001, 0.005, "linear"
        b["pdnorm_conditions"] = ("nuScenes", "SemanticKITTI", "Waymo")
    else:
        raise KeyError(dataset)
    return m


def model_config(dataset="scannet", variant="CDSegNet"):
    """``model`` dict of configs/<dataset>/<variant>.py for the four model variants the reference ships
    (criteria dropped).  Differences to CDSegNet.py (diffed from the reference's config files):

      PTv3_CNF  n_enc_depths (2,2,2,6,2); linear schedule (scannet 1e-4..5e-4, nuscenes 2e-3..3e-3, scannet200 keeps
                its 1e-3..5e-3)
      PTv3      condition=False, dm=False, skip_connection_mode="add", n_enc_depths (2,2,2,6,2)
      Baseline  dm=False (the c-branch sees the input itself at t = 0)
    """
    m = cdsegnet_config(dataset)
    b = m["backbone"]
    if variant == "CDSegNet":
        return m
    if variant == "Baseline":  # configs/scannet/Baseline.py:18
        m["dm"] = False
        return m
    if variant not in ("PTv3_CNF", "PTv3"):
        raise KeyError(variant)
    b["n_enc_depths"] = (2, 2, 2, 6, 2)  # configs/scannet/PTv3_CNF.py:75
    m["noise_schedule"] = "linear"
    if dataset != "scannet200":
        m["beta_start"], m["beta_end"] = (0.002, 0.003) if dataset == "nuscenes" else (0.0001, 0.0005)
    if variant == "PTv3":  # configs/scannet/PTv3.py:17-18,33,46
        m["condition"] = b["condition"] = False
        m["dm"] = False
        m["loss_type"] = "EW"
        b["skip_connection_mode"] = "add"
    return m


def mini_config(num_classes=13, in_channels=6, T_dim=64, tm_feat=1.0, tm_bidirectional=False, skip_connection_mode=None,
                skip_connection_scale=None, skip_connection_scale_i=None, b_factor=None, s_factor=None):
    """Same architecture, reduced widths/depths (head dim stays 16): the end-to-end
    golden fixture that fits in a few hundred KB.  tm_feat / tm_bidirectional: the fusion ablation switches; skip_connection_* /
    b_factor / s_factor: the skip-connection switches."""
    m = copy.deepcopy(_MODEL)
    b = m["backbone"]
    _fusion(b, tm_feat, tm_bidirectional)
    _skip(b, skip_connection_mode, skip_connection_scale, skip_connection_scale_i, b_factor, s_factor)
    b.update(
        c_in_channels=in_channels, n_in_channels=in_channels,
        c_enc_depths=(1, 2, 1), c_enc_channels=(16, 32, 32), c_enc_num_head=(1, 2, 2),
        c_dec_depths=(1, 1), c_dec_channels=(32, 32), c_dec_num_head=(2, 2),
        n_enc_depths=(1, 1, 2, 1, 5), n_enc_channels=(16, 32, 32, 64, 64), n_enc_num_head=(1, 2, 2, 4, 4),
        n_dec_depths=(1, 1, 1, 2), n_dec_channels=(32, 32, 32, 64), n_dec_num_head=(2, 2, 2, 4),
        num_classes=num_classes, T_dim=T_dim,
    )
    m.update(num_classes=num_classes, T_dim=T_dim, c_in_channels=in_channels)
    return m
