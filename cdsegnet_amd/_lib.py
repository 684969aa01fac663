"""ctypes binding of libcdseg_hip.so (C ABI declared in include/cdseg.h).

The product path has NO fallback: if the HIP library is missing or a call fails, this
module raises.  (`python -m cdsegnet_amd.build` or `__graft_entry__.build()` builds it.)
"""
import ctypes
import os
import threading
from ctypes import POINTER, Structure, c_char_p, c_float, c_int, c_int32, c_int64, c_long, c_size_t, c_uint64, c_void_p

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libcdseg_hip.so")          # 16-bit type = bfloat16
LIB_PATH_F16 = os.path.join(HERE, "libcdseg_hip_f16.so")  # 16-bit type = IEEE half (same sources, -DCDSEG_LP_F16)

F32, BF16 = 0, 1
ACT_NONE, ACT_GELU, ACT_SWISH = 0, 1, 2
ORDER_IDS = {"z": 0, "z-trans": 1, "hilbert": 2, "hilbert-trans": 3}
ERRORS = {-1: "CDSEG_ERR_ARG", -2: "CDSEG_ERR_LAUNCH", -3: "CDSEG_ERR_WORKSPACE", -4: "CDSEG_ERR_UNSUPPORTED"}


class CdsegError(RuntimeError):
    pass


class DuplicateVoxelsError(CdsegError):
    """Several input points share one (batch element, grid_coord) voxel.  `count` = the surplus points."""

    def __init__(self, msg, count):
        super().__init__(msg)
        self.count = int(count)


class GemmArgs(Structure):
    _fields_ = [
        ("A", c_void_p), ("W", c_void_p), ("bias", c_void_p), ("scale", c_void_p), ("shift", c_void_p),
        ("res", c_void_p), ("add_src", c_void_p), ("add_idx", c_void_p), ("nbr", c_void_p), ("out_idx", c_void_p),
        ("out", c_void_p), ("out2", c_void_p),
        ("M", c_long),
        ("N", c_int), ("K", c_int), ("kvol", c_int),
        ("lda", c_int), ("ldo", c_int), ("ldo2", c_int), ("ldres", c_int), ("ldadd", c_int),
        ("a_dtype", c_int), ("compute_dtype", c_int), ("out_dtype", c_int), ("out2_dtype", c_int),
        ("act", c_int), ("out2_pre_add", c_int),
        ("ws", c_void_p), ("ws_bytes", c_size_t),
        ("colbias", c_void_p), ("ln_pre_g", c_void_p), ("ln_pre_b", c_void_p), ("ln_post_g", c_void_p),
        ("ln_post_b", c_void_p), ("ln_out", c_void_p), ("ldln", c_int), ("ln_out_dtype", c_int), ("ln_eps", c_float),
        ("nbr_kmajor", c_int),
    ]


class BlockDesc(Structure):
    _fields_ = [
        ("dtype", c_int), ("channels", c_int), ("heads", c_int), ("hidden", c_int),
        ("attn_scale", c_float), ("ln_eps", c_float),
        ("cpe_conv_w", c_void_p), ("cpe_conv_b", c_void_p), ("cpe_lin_w", c_void_p), ("cpe_lin_b", c_void_p),
        ("cpe_ln_g", c_void_p), ("cpe_ln_b", c_void_p), ("norm1_g", c_void_p), ("norm1_b", c_void_p),
        ("qkv_w", c_void_p), ("qkv_b", c_void_p), ("proj_w", c_void_p), ("proj_b", c_void_p),
        ("norm2_g", c_void_p), ("norm2_b", c_void_p), ("fc1_w", c_void_p), ("fc1_b", c_void_p),
        ("fc2_w", c_void_p), ("fc2_b", c_void_p), ("cpe_conv_wimg", c_void_p),
        ("head_img", c_void_p), ("tail_img", c_void_p),
        ("attn_flags", c_int),
    ]


class BlockIO(Structure):
    _fields_ = [
        ("n", c_long), ("x", c_void_p), ("xc_in", c_void_p), ("xc_out", c_void_p), ("tbias", c_void_p),
        ("nbr", c_void_p), ("gidx", c_void_p), ("widx", c_void_p), ("patch_start", c_void_p),
        ("num_patches", c_int), ("max_len", c_int), ("scratch", c_void_p), ("scratch_bytes", c_size_t),
        ("sat_counter", c_void_p),
        ("flags", c_int), ("logits", c_void_p), ("head_w", c_void_p), ("head_b", c_void_p), ("out_idx", c_void_p),
        ("num_classes", c_int), ("ld_logits", c_int),
    ]


class TrainBlockDesc(Structure):
    _fields_ = [
        ("channels", c_int), ("heads", c_int), ("hidden", c_int),
        ("attn_scale", c_float), ("eps_cpe", c_float), ("eps_norm1", c_float), ("eps_norm2", c_float),
        ("mm_dtype", c_int), ("attn_dtype", c_int), ("deterministic", c_int),
        ("param", c_void_p * 18), ("shadow16", c_void_p * 6),
        ("derived", c_void_p), ("derived_bytes", c_size_t),
    ]


class TrainBlockIO(Structure):
    _fields_ = [
        ("n", c_long), ("x_in", c_void_p), ("x_conv", c_void_p), ("t_rows", c_void_p), ("scene_offs", c_void_p),
        ("num_scenes", c_int), ("mask1", c_void_p), ("mask2", c_void_p),
        ("nbr", c_void_p), ("gidx", c_void_p), ("widx", c_void_p), ("patch_start", c_void_p),
        ("num_patches", c_int), ("max_len", c_int), ("num_slots", c_long),
        ("tape", c_void_p), ("tape_bytes", c_size_t), ("scratch", c_void_p), ("scratch_bytes", c_size_t),
        ("x_out", c_void_p),
        ("n_conv", c_long), ("row_vox", c_void_p), ("row_start", c_void_p),
    ]


class PlanSpec(Structure):
    _fields_ = [
        ("nlev", c_int), ("cum", c_int * 9), ("ncurve", c_int), ("curve_rows", c_int * 3),
        ("nslot_curve", c_int), ("slot_curve", c_int * 4),
        ("nlink", c_int), ("link_a", c_int * 16), ("link_b", c_int * 16),
        ("npad", c_int), ("pad_patch", c_int * 4), ("pad_flash", c_int * 4),
    ]


class PlanBeginIO(Structure):
    _fields_ = [
        ("grid", c_void_p), ("grid_elem_bytes", c_int), ("offset", c_void_p), ("nb", c_int), ("n", c_long),
        ("depth", c_int), ("end_bit", c_int), ("i32", c_void_p), ("i64", c_void_p), ("ws", c_void_p),
        ("ws_bytes", c_size_t), ("gmax_host", c_void_p), ("meta_host", c_void_p),
    ]


class PlanFinishIO(Structure):
    _fields_ = [
        ("n", c_long), ("nb", c_int), ("depth", c_int), ("m_host", POINTER(c_long)), ("offs_host", POINTER(c_int)),
        ("grid0", c_void_p), ("bat0", c_void_p), ("code0", c_void_p), ("cluster", c_void_p), ("seg", c_void_p),
        ("orders0", c_void_p), ("i32", c_void_p), ("i64", c_void_p), ("ws", c_void_p), ("ws_bytes", c_size_t),
        ("pads_host", c_void_p),
    ]


class OptTensor(Structure):
    _fields_ = [("p", c_void_p), ("g", c_void_p), ("m", c_void_p), ("v", c_void_p), ("p16", c_void_p), ("step", c_void_p),
                ("n", c_long), ("group", c_int), ("flags", c_int)]


class OptGroup(Structure):
    _fields_ = [("lr", ctypes.c_double), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double), ("eps", ctypes.c_double),
                ("weight_decay", ctypes.c_double)]


OPT_CLIP, OPT_SKIP = 1, 2  # cdseg_opt_tensor.flags

# name -> (restype, argtypes); every symbol include/cdseg.h declares
SIGNATURES = {
    "cdseg_abi_version": (c_int, []),
    "cdseg_build_info": (c_char_p, []),
    "cdseg_grid_max": (c_int, [c_void_p, c_int, c_long, c_void_p, c_void_p]),
    "cdseg_offset2batch": (c_int, [c_void_p, c_int, c_long, c_void_p, c_void_p]),
    "cdseg_encode": (c_int, [c_void_p, c_int, c_void_p, c_int, c_long, c_int, c_int, c_void_p, c_void_p]),
    "cdseg_encode4": (c_int, [c_void_p, c_void_p, c_long, c_int, c_void_p, c_void_p]),
    "cdseg_sort_ws_bytes": (c_size_t, [c_long]),
    "cdseg_sort_pairs": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_int, c_void_p, c_size_t, c_void_p]),
    "cdseg_sort_curves_ws_bytes": (c_size_t, [c_long, c_int]),
    "cdseg_sort_curves": (c_int, [c_void_p, POINTER(c_int), c_int, c_long, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "cdseg_invert_perm": (c_int, [c_void_p, c_long, c_void_p, c_void_p]),
    "cdseg_widen_i32": (c_int, [c_void_p, c_long, c_void_p, c_void_p]),
    "cdseg_gather_rows": (c_int, [c_void_p, c_void_p, c_long, c_int, c_void_p, c_void_p]),
    "cdseg_scatter_rows": (c_int, [c_void_p, c_void_p, c_long, c_int, c_void_p, c_void_p]),
    "cdseg_gather_i32": (c_int, [c_void_p, c_void_p, c_long, c_void_p, c_void_p]),
    "cdseg_plan_gather_grid": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_long, c_int, c_void_p, c_void_p, c_void_p]),
    "cdseg_pool_level": (c_int, [c_void_p, c_long, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "cdseg_pool_gather": (c_int, [c_void_p, c_long, c_long, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p]),
    "cdseg_pool_levels_ws_bytes": (c_size_t, [c_long, c_int]),
    "cdseg_pool_levels": (c_int, [c_void_p, c_long, POINTER(c_int), c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_size_t, c_void_p]),
    "cdseg_link_derive": (c_int, [c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_void_p]),
    "cdseg_coarse_orders_ws_bytes": (c_size_t, [c_long, c_int, c_int]),
    "cdseg_coarse_orders": (c_int, [POINTER(c_void_p), c_int, POINTER(c_void_p), c_int, c_long, c_void_p, c_void_p,
                                    c_size_t, c_void_p]),
    "cdseg_nbr_table": (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_int, c_int, c_int, c_void_p, c_void_p]),
    "cdseg_nbr_table_from_parent": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_long, c_int, c_int,
                                            c_int, c_void_p, c_void_p]),
    "cdseg_nbr_table_from_info": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_long, c_int, c_int, c_int, c_void_p,
                                          c_void_p]),
    "cdseg_pad_plan": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_long, c_void_p, c_void_p, c_void_p]),
    "cdseg_pad_plan_batch": (c_int, [c_int, POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p), POINTER(c_int),
                                     POINTER(c_long), c_int, c_void_p, c_void_p, c_void_p]),
    "cdseg_slots_select": (c_int, [POINTER(c_void_p), POINTER(c_void_p), c_int, c_void_p, c_int, c_char_p, c_long, c_void_p,
                                   c_void_p, c_void_p]),
    "cdseg_plan_begin_layout": (c_int, [POINTER(PlanSpec), c_long, c_int, POINTER(c_long), POINTER(c_long)]),
    "cdseg_plan_begin": (c_int, [POINTER(PlanSpec), POINTER(PlanBeginIO), c_int, c_void_p]),
    "cdseg_plan_finish_layout": (c_int, [POINTER(PlanSpec), c_long, c_int, POINTER(c_long), POINTER(c_int), POINTER(c_long),
                                         POINTER(c_long)]),
    "cdseg_plan_finish": (c_int, [POINTER(PlanSpec), POINTER(PlanFinishIO), c_void_p]),
    "cdseg_voxelize": (c_int, [c_void_p, ctypes.c_double, c_long, c_void_p, c_void_p, c_void_p, c_void_p]),
    "cdseg_voxelize_f64": (c_int, [c_void_p, ctypes.c_double, c_long, c_void_p, c_void_p, c_void_p, c_void_p]),
    "cdseg_center_shift": (c_int, [c_void_p, c_int, c_long, c_int, c_void_p, c_void_p, c_void_p]),
    "cdseg_tta_apply": (c_int, [c_void_p, c_long, POINTER(ctypes.c_double), ctypes.c_double, c_int, c_int, c_void_p, c_void_p]),
    "cdseg_div_add": (c_int, [c_void_p, c_float, c_float, c_long, c_void_p, c_void_p]),
    "cdseg_collect_feat": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_long, c_void_p, c_void_p]),
    "cdseg_max_run": (c_int, [c_void_p, c_long, c_void_p, c_void_p]),
    "cdseg_fragment_select": (c_int, [c_void_p, c_void_p, c_long, c_int, c_void_p, c_void_p]),
    "cdseg_softmax_vote": (c_int, [c_void_p, c_int, c_void_p, c_long, c_int, c_void_p, c_int, c_void_p]),
    "cdseg_argmax_rows": (c_int, [c_void_p, c_int, c_long, c_int, c_void_p, c_void_p]),
    "cdseg_fragments_build_ws_bytes": (c_size_t, [c_int]),
    "cdseg_fragments_build": (c_int, [c_void_p, c_void_p, c_long, c_int, c_long, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "cdseg_softmax_vote_fragments": (c_int, [c_void_p, c_int, c_void_p, c_long, c_int, c_int, c_void_p, c_int, c_long, c_void_p]),
    "cdseg_voxel_inverse": (c_int, [c_void_p, c_void_p, c_long, c_void_p, c_void_p]),
    "cdseg_tt_bbox": (c_int, [c_void_p, c_int, c_long, c_void_p, c_void_p]),
    "cdseg_tt_affine": (c_int, [c_void_p, c_int, c_long, c_int, POINTER(ctypes.c_double), c_void_p, POINTER(ctypes.c_double), c_int,
                                ctypes.c_double, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    "cdseg_tt_jitter": (c_int, [c_void_p, c_void_p, c_int, ctypes.c_double, ctypes.c_double, c_long, c_void_p]),
    "cdseg_tt_blur3": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "cdseg_tt_elastic": (c_int, [c_void_p, c_long, c_void_p, POINTER(c_int), POINTER(ctypes.c_double), POINTER(ctypes.c_double),
                                 POINTER(ctypes.c_double), ctypes.c_double, c_void_p]),
    "cdseg_tt_color": (c_int, [c_void_p, c_long, c_void_p, ctypes.c_double, c_int, POINTER(ctypes.c_double), c_void_p, c_int,
                               ctypes.c_double, c_void_p]),
    "cdseg_tt_voxel_pick": (c_int, [c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_void_p]),
    "cdseg_tt_dist_key": (c_int, [c_void_p, c_long, c_long, c_void_p, c_void_p]),
    "cdseg_rand_int": (c_int, [c_void_p, c_long, c_uint64, c_uint64, c_void_p, ctypes.c_uint32, c_void_p]),
    "cdseg_knn": (c_int, [c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_long, c_int, c_int, POINTER(c_float), c_float,
                          c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "cdseg_knn1_ws_bytes": (c_size_t, [c_long]),
    "cdseg_knn1": (c_int, [c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_long, c_int, POINTER(c_float), c_float,
                           c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "cdseg_iou_counts": (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_int, c_int, c_void_p, c_void_p]),
    "cdseg_gemm": (c_int, [POINTER(GemmArgs), c_void_p]),
    "cdseg_gemm_ws_bytes": (c_size_t, [c_long, c_int, c_int, c_int]),
    "cdseg_mlp_fused": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int,
                                c_long, c_int, c_int, c_void_p]),
    "cdseg_attn_tail_fused": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_long, c_int, c_int, c_void_p]),
    "cdseg_cpe_head_fused": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                     c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_int, c_long, c_int, c_int,
                                     c_int, c_void_p]),
    "cdseg_subm_conv3_wimg_bytes": (c_size_t, [c_int]),
    "cdseg_subm_conv3_pack": (c_int, [c_void_p, c_int, c_void_p, c_void_p]),
    "cdseg_subm_conv3": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_long, c_int, c_void_p, c_int, c_void_p]),
    "cdseg_child_info": (c_int, [c_void_p, c_void_p, c_long, c_void_p, c_void_p]),
    "cdseg_stem5_wimg_bytes": (c_size_t, []),
    "cdseg_stem5_pack": (c_int, [c_void_p, c_void_p, c_void_p]),
    "cdseg_stem5": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_long,
                            c_int, c_void_p, c_void_p, c_void_p]),
    "cdseg_block_rr_img_bytes": (c_size_t, [c_int, c_int]),
    "cdseg_block_rr_pack": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "cdseg_cpe_head_rr": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                  c_void_p, c_float, c_void_p, c_void_p, c_int, c_long, c_int, c_int, c_void_p]),
    "cdseg_attn_tail_rr": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p,
                                   c_void_p, c_int, c_void_p, c_int, c_long, c_int, c_void_p]),
    "cdseg_attn_tail_rr_ex": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p,
                                      c_void_p, c_int, c_void_p, c_int, c_long, c_int, c_int, c_void_p, c_int, c_void_p,
                                      c_void_p, c_void_p, c_int, c_void_p]),
    "cdseg_cpe_head_rr2": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int,
                                   c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_int, c_long, c_int, c_int, c_void_p]),
    "cdseg_attn_tail_rr2": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p,
                                    c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_long, c_int, c_void_p, c_size_t, c_void_p]),
    "cdseg_block_scratch_bytes": (c_size_t, [POINTER(BlockDesc), c_long]),
    "cdseg_block_forward": (c_int, [POINTER(BlockDesc), POINTER(BlockIO), c_void_p]),
    "cdseg_layernorm": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p, c_int, c_void_p,
                                c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_long, c_int, c_void_p]),
    "cdseg_attention": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_int, c_int, c_void_p]),
    "cdseg_attention_ex": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_int, c_int, c_int, c_void_p]),
    "cdseg_attention_schedule": (c_long, [c_int, c_int, c_int, c_int, c_void_p, c_long]),
    "cdseg_attention_bwd_ws_bytes": (c_size_t, [c_long, c_int]),
    "cdseg_attention_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_int, c_int, c_long, c_int, c_float, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                    c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "cdseg_attention_drop": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_int, c_int, c_int, c_float, c_void_p, c_int, c_int, ctypes.c_double, c_uint64, c_uint64,
                                     c_void_p]),
    "cdseg_attention_drop_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_int, c_int, c_long, c_int, c_float, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                         c_int, c_int, c_int, c_int, c_void_p, c_size_t, ctypes.c_double, c_uint64, c_uint64,
                                         c_void_p]),
    "cdseg_dropout": (c_int, [c_void_p, c_int, c_void_p, c_int, c_long, c_int, ctypes.c_double, c_uint64, c_uint64, c_void_p]),
    "cdseg_layernorm_bwd": (c_int, [c_void_p, c_int, c_void_p, c_float, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p,
                                    c_void_p, c_long, c_int, c_void_p]),
    "cdseg_gelu_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_void_p]),
    "cdseg_conv_wgrad": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_long, c_int, c_int, c_void_p, c_void_p,
                                 c_void_p]),
    "cdseg_linear_wgrad": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_long, c_int, c_int, c_void_p, c_int, c_void_p,
                                   c_void_p]),
    "cdseg_conv_wgrad16": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_long, c_int, c_int, c_void_p, c_void_p,
                                   c_void_p]),
    "cdseg_linear_wgrad16": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_long, c_int, c_int, c_void_p, c_int, c_void_p,
                                     c_void_p]),
    "cdseg_wgrad_partition": (c_int, [c_long, c_int, c_int, c_int, c_int, POINTER(c_long), POINTER(c_int)]),
    "cdseg_wgrad_det_ws_bytes": (c_size_t, [c_long, c_int, c_int, c_int, c_int]),
    "cdseg_linear_wgrad_det": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_long, c_int, c_int, c_void_p, c_int, c_void_p,
                                       c_int, c_void_p, c_size_t, c_void_p]),
    "cdseg_conv_wgrad_det": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_long, c_int, c_int, c_void_p, c_void_p,
                                     c_int, c_void_p, c_size_t, c_void_p]),
    "cdseg_layernorm_bwd_det_ws_bytes": (c_size_t, [c_long, c_int]),
    "cdseg_layernorm_bwd_det": (c_int, [c_void_p, c_int, c_void_p, c_float, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p,
                                        c_void_p, c_long, c_int, c_void_p, c_size_t, c_void_p]),
    "cdseg_segment_sum": (c_int, [c_void_p, c_int, c_void_p, c_long, c_int, c_void_p, c_int, c_void_p]),
    "cdseg_seg_loss_ws_bytes": (c_size_t, [c_long, c_int]),
    "cdseg_seg_loss_fwd": (c_int, [c_void_p, c_int, c_void_p, c_long, c_int, c_long, c_int, c_void_p, POINTER(c_int32), c_void_p,
                                   c_void_p, c_void_p, c_size_t, c_void_p]),
    "cdseg_seg_loss_bwd": (c_int, [c_void_p, c_int, c_void_p, c_long, c_int, c_long, POINTER(c_int32), c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_int, c_void_p]),
    "cdseg_bn_partition": (c_int, [c_long, c_int, POINTER(c_long), POINTER(c_int)]),
    "cdseg_bn_ws_bytes": (c_size_t, [c_long, c_int]),
    "cdseg_bn_stats": (c_int, [c_void_p, c_int, c_long, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "cdseg_bn_finish": (c_int, [c_void_p, c_int, ctypes.c_double, ctypes.c_double, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p]),
    "cdseg_bn_gelu_fwd": (c_int, [c_void_p, c_int, c_long, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                  c_void_p]),
    "cdseg_bn_gelu_bwd_sums": (c_int, [c_void_p, c_int, c_void_p, c_int, c_long, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_size_t, c_void_p]),
    "cdseg_bn_gelu_bwd_dx": (c_int, [c_void_p, c_int, c_void_p, c_int, c_long, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "cdseg_segment_max_arg": (c_int, [c_void_p, c_int, c_void_p, c_long, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p]),
    "cdseg_segment_max_bwd": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_long, c_int, c_void_p, c_int, c_void_p]),
    "cdseg_fuse_gate_ws_bytes": (c_size_t, [c_long, c_int]),
    "cdseg_fuse_gate_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_int, c_void_p]),
    "cdseg_fuse_gate_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_long, c_int, c_void_p, c_size_t, c_void_p]),
    "cdseg_skip_partition": (c_int, [c_long, c_int, POINTER(c_long), POINTER(c_int)]),
    "cdseg_skip_stats_ws_bytes": (c_size_t, [c_long, c_int]),
    "cdseg_skip_stats": (c_int, [c_void_p, c_int, c_int, c_long, c_int, c_void_p, c_long, c_void_p, c_void_p, c_size_t, c_void_p]),
    "cdseg_skip_fold": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "cdseg_skip_merge": (c_int, [c_void_p, c_int, c_long, c_int, c_void_p, c_int, ctypes.c_double, c_long, ctypes.c_double,
                                 c_void_p, c_void_p, c_int, c_void_p, c_long, c_void_p]),
    "cdseg_opt_chunks": (c_int, [POINTER(c_long), c_int, POINTER(c_int32), POINTER(c_long)]),
    "cdseg_opt_ws_bytes": (c_size_t, [c_int, c_long]),
    "cdseg_grad_norm": (c_int, [POINTER(OptTensor), c_int, c_void_p, c_long, c_void_p, c_float, c_void_p, c_void_p, c_size_t,
                                c_void_p]),
    "cdseg_adamw_step": (c_int, [POINTER(OptTensor), c_int, POINTER(OptGroup), c_int, c_void_p, c_long, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_size_t, c_void_p]),
    "cdseg_route_enable": (c_int, [c_int]),
    "cdseg_route_clear": (None, []),
    "cdseg_route_read": (c_int, [POINTER(c_int32), c_int]),
    "cdseg_route_catalog": (c_int, [ctypes.c_char_p, c_size_t]),
    "cdseg_route_note": (c_int, [POINTER(c_int32)]),
    "cdseg_prof_enable": (c_int, [c_int]),
    "cdseg_prof_summary": (c_int, [POINTER(ctypes.c_double), POINTER(c_long)]),
    "cdseg_prof_summary_class": (c_int, [c_int, POINTER(ctypes.c_double), POINTER(c_long)]),
    "cdseg_segment_max": (c_int, [c_void_p, c_int, c_int, c_void_p, c_long, c_int, c_void_p, c_void_p, c_int,
                                  c_void_p, c_int, c_void_p, c_int, c_int, c_void_p]),
    "cdseg_segment_mean": (c_int, [c_void_p, c_int, c_void_p, c_long, c_int, c_void_p, c_int, c_void_p]),
    "cdseg_pool_fused_fold": (c_int, [c_int]),
    "cdseg_pool_fused_n": (c_int, [c_void_p, c_int, c_long, c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_int, c_void_p,
                                   c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    "cdseg_unpool_fused_img_bytes": (c_size_t, [c_int, c_int]),
    "cdseg_unpool_fused_pack": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "cdseg_unpool_fused": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_long, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int,
                                   c_int, c_void_p]),
    "cdseg_pool_fused_img_bytes": (c_size_t, [c_int, c_int]),
    "cdseg_pool_fused_pack": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "cdseg_pool_fused": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_int, c_void_p, c_int,
                                 c_void_p, c_int, c_int, c_int, c_void_p]),
    "cdseg_gemv": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "cdseg_randn": (c_int, [c_void_p, c_long, c_uint64, c_uint64, c_void_p]),
    "cdseg_cast": (c_int, [c_void_p, c_int, c_void_p, c_int, c_long, c_void_p]),
    "cdseg_gather_pad_cast": (c_int, [c_void_p, c_int, c_void_p, c_long, c_int, c_int, c_void_p, c_int, c_void_p]),
    "cdseg_ddim_update": (c_int, [c_void_p, c_void_p, c_float, c_float, c_float, c_float, c_int, c_void_p, c_long,
                                  c_void_p]),
    "cdseg_axpy": (c_int, [c_void_p, c_void_p, c_float, c_void_p, c_long, c_void_p]),
    "cdseg_msi_step": (c_int, [c_void_p, c_void_p, c_long, c_float, c_float, c_float, c_float, c_int, c_void_p, c_void_p, c_long,
                               c_int, c_float, c_void_p]),
    "cdseg_count_saturated": (c_int, [c_void_p, c_long, c_int, c_int, c_void_p, c_void_p]),
    "cdseg_subm_conv3_f32": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_long, c_int, c_void_p, c_int, c_float, c_int,
                                     c_void_p]),
    "cdseg_split16": (c_int, [c_void_p, c_int, c_long, c_int, c_void_p, c_void_p, c_int, c_float, c_void_p]),
    "cdseg_train_block_bytes": (c_int, [POINTER(TrainBlockDesc), c_long, c_long, POINTER(c_size_t), POINTER(c_size_t),
                                        POINTER(c_size_t), POINTER(c_size_t)]),
    "cdseg_train_block_grad_offsets": (c_int, [POINTER(TrainBlockDesc), POINTER(c_size_t)]),
    "cdseg_train_block_prepare": (c_int, [POINTER(TrainBlockDesc), c_void_p]),
    "cdseg_train_block_forward": (c_int, [POINTER(TrainBlockDesc), POINTER(TrainBlockIO), c_void_p]),
    "cdseg_train_block_backward": (c_int, [POINTER(TrainBlockDesc), POINTER(TrainBlockIO), c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_void_p]),
    "cdseg_residual": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_long, c_int, c_void_p]),
    "cdseg_gather_first": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_long, c_int, c_void_p]),
    "cdseg_residual_rows": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_long, c_int, c_void_p]),
    "cdseg_run_sum": (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_int, c_void_p]),
    "cdseg_scatter_first": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_long, c_int, c_void_p]),
    "cdseg_scale_cast": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_long, c_int, c_void_p]),
    "cdseg_add_layernorm": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_int, c_long,
                                    c_int, c_void_p]),
    "cdseg_gelu_fwd": (c_int, [c_void_p, c_void_p, c_int, c_long, c_void_p]),
    "cdseg_gelu_bwd_cast": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_long, c_void_p]),
}

_libs = {}
_tls = threading.local()  # .variant: which build the calling host thread's ops go to ("bf16" default, "f16")
VARIANTS = ("bf16", "f16")


def active():
    return getattr(_tls, "variant", "bf16")


class use:
    """`with _lib.use("f16"):` routes the calling thread's ops to the IEEE-half build of the library."""

    def __init__(self, variant):
        if variant not in VARIANTS:
            raise ValueError(variant)
        self.variant = variant

    def __enter__(self):
        self.prev = active()
        _tls.variant = self.variant
        return self

    def __exit__(self, *exc):
        _tls.variant = self.prev
        return False


def activate(variant):
    """Make `variant` the calling thread's build from here on (a process that runs one precision throughout, e.g. bench.py)."""
    if variant not in VARIANTS:
        raise ValueError(variant)
    _tls.variant = variant


def load(variant=None):
    """Load the HIP library (the calling thread's active build); raises CdsegError (never falls back) if it is absent."""
    v = variant or active()
    lib = _libs.get(v)
    if lib is not None:
        return lib
    path = LIB_PATH if v == "bf16" else LIB_PATH_F16
    if not os.path.exists(path):
        raise CdsegError(
            f"{path} is missing: the MI355X HIP extension was not built. "
            "Run `python -m cdsegnet_amd.build` (hipcc --offload-arch=gfx950). There is no CPU/PyTorch fallback.")
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the ABI lost a symbol
        fn.restype = res
        fn.argtypes = args
    _libs[v] = lib
    return lib


def check(status, what):
    if status != 0:
        raise CdsegError(f"{what} failed: {ERRORS.get(status, status)}")
