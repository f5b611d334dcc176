"""ctypes binding of libyunet_hip.so (the C ABI declared in include/yunet_hip.h).

There is deliberately NO fallback: if the shared library is missing the product path
raises.  Build it with `python __graft_entry__.py` or `make -C libfacedetection.train_amd/csrc`.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# YUNET_HIP_LIB selects another build of the same library (kernel A/B measurements)
LIB_PATH = os.environ.get('YUNET_HIP_LIB') or os.path.join(_HERE, 'libyunet_hip.so')

c_f32p = C.c_void_p
MAX_LEVELS = 5

EINVAL, EOPCODE = -1, -2            # YUNET_EINVAL / YUNET_EOPCODE (include/yunet_hip.h)
FETCH_BAD_RECT, FETCH_BAD_SRC, FETCH_BAD_DST = 1, 2, 4      # YUNET_FETCH_BAD_* (yunet_fetch_windows status bits)
EMA_MAX_SEGMENTS = 3                                        # YUNET_EMA_MAX_SEGMENTS (yunet_ema_update)
HIST_TOTAL, HIST_NOIMG, HIST_SPILLED, HIST_STATUS = 0, 1, 2, 3   # YUNET_HIST_* (yunet_box_size_hist totals[])
HIST_SPILL, HIST_OVERFLOW, HIST_BAD_COUNT = 1, 2, 4             # its status bits
SCORE_BLOCK, SCORE_GT_CHUNK, SCORE_MAX_THRESH = 256, 256, 1024   # YUNET_SCORE_* (csrc/score.hip)
RANK_SEG_CAP, RANK_RADIX_TILE, RANK_CURVE_MAX = 1024, 4096, 1 << 24   # YUNET_RANK_* (csrc/score.hip: ranking and curve)
NORM_BLOCK, NORM_TILE, NORM_MAX_BLOCKS, NORM_SCRATCH_BYTES = 256, 4096, 256, 8 + 8 * 256   # YUNET_NORM_* (csrc/optim.hip)
NORM_INF, NORM_L1, NORM_L2 = 0, 1, 2
ACCUM_SAVE, ACCUM_ADD = 0, 1                      # YUNET_ACCUM_* (yunet_grad_accum)
OPT_ROW, OPT_MAX_GROUPS = 4, 255                                  # YUNET_OPT_* (the group table of csrc/optim.hip)
OPT_FROZEN = 255                                                  # YUNET_OPT_FROZEN: the group-map byte that means no update
T_IDENTITY, T_BNRELU = 0, 1
F32, BF16 = 0, 1
DET_FAST = 1 << 30         # YUNET_DET_FAST: flag in YunetBN.det_rows, above the row count
BOX_EIOU, BOX_DIOU, BOX_IOU_LINEAR, BOX_IOU_SQUARE, BOX_IOU_LOG, BOX_GIOU, BOX_CIOU, BOX_BOUNDED = 0, 1, 2, 3, 4, 5, 6, 7
CLS_BCE, CLS_VARIFOCAL = 0, 1                                     # YUNET_CLS_* (YunetLossTerms.cls_loss / obj_loss)
KPS_SMOOTH_L1, KPS_L1, KPS_MSE, KPS_BALANCED_L1 = 0, 1, 2, 3      # YUNET_KPS_* (YunetLossTerms.kps_loss)
(OP_STEM_FWD, OP_STEM_BWD, OP_DP_FWD, OP_DP_BWD, OP_POOL_FWD, OP_POOL_BWD, OP_UPADD_FWD,
 OP_UPADD_BWD, OP_BN_RUNNING, OP_BN_PARAM_GRAD, OP_REDUCE_PARTIALS, OP_ASSIGN, OP_LOSS_NORM,
 OP_LOSS, OP_LOSS_FINALIZE, OP_SGD, OP_MEMSET, OP_BN_BATCH, OP_REDUCE_BATCH, OP_FORK, OP_JOIN, OP_ADD, OP_BN_FOLD,
 OP_STEM_BWD_DX, OP_IGNORE_MARK) = range(1, 26)
LOSS_IGNORE, LOSS_FLAGS_SLOT = 1, 8  # YUNET_LOSS_IGNORE; YUNET_OP_LOSS carries the flag word in i[8]
IGNORE_MAX_BOXES, IGNORE_MIN_ROWS = 1024, 16      # rows per image of the padded ignore boxes (yunet_ignore_mark: Imax <= 1024)
OP_LANE, MAX_LANES = 10, 2          # YunetOp.i[OP_LANE]: side stream of the op (0 = the caller's stream)
OP_GROUP, DP_GROUP_MAX = 9, 3       # YunetOp.i[OP_GROUP] = g: this DP_FWD op and the g - 1 after it are independent (ABI 10)


class YunetBN(C.Structure):
    _fields_ = [('stats', C.c_void_p), ('bstats', C.c_void_p), ('gamma', C.c_void_p),
                ('beta', C.c_void_p), ('count', C.c_int32), ('eps', C.c_float),
                ('slots', C.c_int32), ('det_rows', C.c_int32)]


class YunetDP(C.Structure):
    _fields_ = [('N', C.c_int32), ('H', C.c_int32), ('W', C.c_int32), ('cin', C.c_int32),
                ('cout', C.c_int32), ('in_transform', C.c_int32), ('out_has_bn', C.c_int32),
                ('accumulate_dx', C.c_int32), ('x_img_stride', C.c_int64),
                ('z_img_stride', C.c_int64), ('x', C.c_void_p), ('in_bn', YunetBN),
                ('w_pw', C.c_void_p), ('b_pw', C.c_void_p), ('w_dw', C.c_void_p),
                ('b_dw', C.c_void_p), ('z', C.c_void_p), ('out_bn', YunetBN),
                ('dy', C.c_void_p), ('dy_scale', C.c_void_p), ('dx', C.c_void_p),
                ('wgrad_partials', C.c_void_p), ('wgrad_blocks', C.c_int32),
                ('prof', C.c_void_p), ('x_dtype', C.c_int32), ('z_dtype', C.c_int32),
                ('pool_out', C.c_void_p), ('pool_idx', C.c_void_p)]


class YunetLevels(C.Structure):
    _fields_ = [('num_levels', C.c_int32), ('h', C.c_int32 * MAX_LEVELS),
                ('w', C.c_int32 * MAX_LEVELS), ('stride', C.c_int32 * MAX_LEVELS)]


SOFTNMS_NAIVE, SOFTNMS_LINEAR, SOFTNMS_GAUSSIAN = 0, 1, 2       # YUNET_SOFTNMS_* (YunetSoftNms.method)


class YunetSoftNms(C.Structure):
    _fields_ = [('method', C.c_int32), ('iou_thr', C.c_float), ('sigma', C.c_float), ('min_score', C.c_float)]


class YunetLossCfg(C.Structure):
    _fields_ = [('box_loss', C.c_int32), ('w_cls', C.c_float), ('w_box', C.c_float),
                ('w_obj', C.c_float), ('w_kps', C.c_float), ('box_eps', C.c_float),
                ('smooth_point', C.c_float), ('kps_beta', C.c_float), ('defer_num_total', C.c_int32)]


class YunetLossTerms(C.Structure):
    """Which loss each term uses (yunet_loss_terms); all-zero = the default selection.  Not a member of YunetOp: an op list
    carries it in YUNET_OP_LOSS's i[4..7] and f[0..5] (op_slots)."""
    _fields_ = [('cls_loss', C.c_int32), ('obj_loss', C.c_int32), ('kps_loss', C.c_int32),
                ('cls_iou_weighted', C.c_int32), ('obj_iou_weighted', C.c_int32),
                ('cls_alpha', C.c_float), ('cls_gamma', C.c_float), ('obj_alpha', C.c_float), ('obj_gamma', C.c_float),
                ('kps_alpha', C.c_float), ('kps_gamma', C.c_float)]

    def op_slots(self):
        """-> (i[4..7], f[0..5]) of a YUNET_OP_LOSS op."""
        return ([self.cls_loss, self.obj_loss, self.kps_loss, (self.cls_iou_weighted & 1) | (self.obj_iou_weighted & 1) << 1],
                [self.cls_alpha, self.cls_gamma, self.obj_alpha, self.obj_gamma, self.kps_alpha, self.kps_gamma])

    def is_default(self):
        return self.cls_loss == CLS_BCE and self.obj_loss == CLS_BCE and self.kps_loss == KPS_SMOOTH_L1


class YunetAssignCfg(C.Structure):
    _fields_ = [('center_radius', C.c_float), ('candidate_topk', C.c_int32), ('iou_weight', C.c_float),
                ('cls_weight', C.c_float)]


class YunetAugCfg(C.Structure):
    _fields_ = [('out_size', C.c_int32), ('n_choice', C.c_int32), ('crop_choice', C.c_double * 8),
                ('flip_ratio', C.c_double), ('pad_value', C.c_float), ('seed', C.c_uint32),
                ('max_attempts', C.c_int32), ('max_retries', C.c_int32), ('gmax', C.c_int32)]


# PhotoMetricDistortion in the pixel pass (YUNET_PHOTO_*): positions, sub-stream salt, per-image table words
PHOTO_NONE, PHOTO_PRE, PHOTO_POST = 0, 1, 2
PHOTO_SALT, PHOTO_WORDS = 0x50484D44, 16
AUG_MAX_EDGE = 8192                  # YUNET_AUG_MAX_EDGE (yunet_aug_decide's scale_hi, yunet_aug_pixels' out_hw)
(PHOTO_BRIGHT, PHOTO_DELTA, PHOTO_MODE, PHOTO_CONTRAST, PHOTO_ALPHA, PHOTO_SAT, PHOTO_SAT_F, PHOTO_HUE, PHOTO_HUE_D,
 PHOTO_SWAP, PHOTO_PERM, PHOTO_DRAWS) = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 13


class YunetPhotoCfg(C.Structure):
    _fields_ = [('brightness_delta', C.c_double), ('contrast_lower', C.c_double), ('contrast_upper', C.c_double),
                ('saturation_lower', C.c_double), ('saturation_upper', C.c_double), ('hue_delta', C.c_double),
                ('position', C.c_int32), ('reserved_', C.c_int32)]


# Mosaic (YUNET_MOSAIC_*): sub-stream salt, geometry table words per image, header words, per-sub-image block
MOSAIC_SALT, MOSAIC_WORDS = 0x4D4F5341, 80
MOSAIC_APPLIED, MOSAIC_CX, MOSAIC_CY, MOSAIC_DRAWS, MOSAIC_KEPT, MOSAIC_STATUS = 0, 1, 2, 3, 4, 5
MOSAIC_QUAD, MOSAIC_QWORDS = 16, 16
(MOSAIC_Q_IDX, MOSAIC_Q_H, MOSAIC_Q_W, MOSAIC_Q_RW, MOSAIC_Q_RH, MOSAIC_Q_PX1, MOSAIC_Q_PY1, MOSAIC_Q_PX2, MOSAIC_Q_PY2,
 MOSAIC_Q_CX1, MOSAIC_Q_CY1) = range(11)
MOSAIC_Q_SX, MOSAIC_Q_SY = 12, 14      # two doubles: the cv2 coordinate scales of the inner resize


class YunetMosaicCfg(C.Structure):
    _fields_ = [('img_scale', C.c_int32), ('gmax', C.c_int32), ('center_lo', C.c_double), ('center_hi', C.c_double),
                ('prob', C.c_double), ('min_bbox_size', C.c_float), ('pad_val', C.c_float), ('seed', C.c_uint32),
                ('bbox_clip_border', C.c_int32), ('skip_filter', C.c_int32), ('reserved_', C.c_int32)]


# CutOut (YUNET_CUTOUT_*): sub-stream salt, hole slots / candidates per configuration, table words per image
CUTOUT_SALT, CUTOUT_MAX_HOLES, CUTOUT_MAX_CANDIDATES = 0x4355544F, 16, 8
CUTOUT_WORDS = 2 + 4 * CUTOUT_MAX_HOLES     # n_holes, draws, then (x1, y1, x2, y2) per slot


class YunetCutoutCfg(C.Structure):
    _fields_ = [('n_lo', C.c_int32), ('n_hi', C.c_int32), ('n_cand', C.c_int32), ('with_ratio', C.c_int32),
                ('cand', (C.c_double * 2) * CUTOUT_MAX_CANDIDATES), ('fill', C.c_float * 3), ('seed', C.c_uint32)]


# RandomAffine (YUNET_AFFINE_*): sub-stream salt, the doubles of a table row and where its parts start
AFFINE_SALT, AFFINE_WORDS, AFFINE_MAX_SHEAR = 0x41464649, 24, 45.0
AFFINE_DRAWS, AFFINE_M, AFFINE_INV, AFFINE_ROWS_IN, AFFINE_ROWS_OUT, AFFINE_EDGE = 0, 6, 15, 21, 22, 23


class YunetAffineCfg(C.Structure):
    _fields_ = [('max_rotate_degree', C.c_double), ('max_translate_ratio', C.c_double), ('scale_lo', C.c_double),
                ('scale_hi', C.c_double), ('max_shear_degree', C.c_double), ('min_bbox_size', C.c_float),
                ('min_area_ratio', C.c_float), ('max_aspect_ratio', C.c_float), ('border_val', C.c_float * 3),
                ('bbox_clip_border', C.c_int32), ('skip_filter', C.c_int32), ('gmax', C.c_int32), ('seed', C.c_uint32)]


# MixUp (YUNET_MIXUP_*): sub-stream salt, the doubles of a table row
MIXUP_SALT, MIXUP_WORDS = 0x4D495855, 18
(MIXUP_PARTNER, MIXUP_APPLIED, MIXUP_INDEX_DRAWS, MIXUP_JIT, MIXUP_FLIP, MIXUP_J, MIXUP_RW, MIXUP_RH, MIXUP_XOFF, MIXUP_YOFF,
 MIXUP_SX, MIXUP_SY, MIXUP_ROWS_IN, MIXUP_ROWS_OUT, MIXUP_STATUS, MIXUP_EDGE, MIXUP_DRAWS, MIXUP_SR) = range(18)


class YunetMixupCfg(C.Structure):
    _fields_ = [('ratio_lo', C.c_double), ('ratio_hi', C.c_double), ('flip_ratio', C.c_double), ('pad_val', C.c_float),
                ('min_bbox_size', C.c_float), ('min_area_ratio', C.c_float), ('max_aspect_ratio', C.c_float),
                ('img_scale', C.c_int32), ('max_iters', C.c_int32), ('bbox_clip_border', C.c_int32),
                ('skip_filter', C.c_int32), ('gmax', C.c_int32), ('seed', C.c_uint32)]


class YunetAugPixels(C.Structure):
    """The pixel pass of yunet_aug_pixels: rect / position / out_hw / geom select the form (include/yunet_hip.h)."""
    _fields_ = [('src', C.c_void_p), ('src_off', C.c_void_p), ('src_hw', C.c_void_p), ('rect', C.c_void_p),
                ('params', C.c_void_p), ('pparams', C.c_void_p), ('geom', C.c_void_p),
                ('mosaic', C.POINTER(YunetMosaicCfg)), ('position', C.c_int32), ('out_hw', C.c_int32)]


MAX_RANKS, IPC_HANDLE_BYTES, COMM_HEADER_BYTES = 8, 64, 20480


class YunetComm(C.Structure):
    _fields_ = [('rank', C.c_int32), ('world', C.c_int32), ('seq', C.c_uint32), ('reserved_', C.c_int32),
                ('slot_bytes', C.c_uint64), ('inbox', C.c_void_p * MAX_RANKS), ('status', C.c_void_p)]


class YunetOp(C.Structure):
    _fields_ = [('opcode', C.c_int32), ('i', C.c_int32 * 12), ('f', C.c_float * 8),
                ('p', C.c_void_p * 12), ('bn', YunetBN * 2), ('dp', YunetDP),
                ('lv', YunetLevels), ('loss', YunetLossCfg)]


_SIGNATURES = {
    'yunet_abi_version': (C.c_int, []),
    'yunet_conv_blocks': (C.c_int, []),
    'yunet_loss_blocks': (C.c_int, [C.c_int, C.c_int]),
    'yunet_stem_fwd': (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 4 + [C.c_void_p]),
    'yunet_stem_fwd_det': (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 5 + [C.c_void_p]),
    'yunet_bn_fold': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    'yunet_stem_bwd': (C.c_int, [C.c_void_p] * 3 + [C.POINTER(YunetBN), C.c_void_p] +
                       [C.c_int] * 5 + [C.c_void_p]),
    'yunet_stem_bwd_rz': (C.c_int, [C.c_void_p] * 4 + [C.POINTER(YunetBN), C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]),
    'yunet_stem_bwd_dx': (C.c_int, [C.c_void_p] * 2 + [C.POINTER(YunetBN)] + [C.c_void_p] * 2 + [C.c_int] * 4 + [C.c_void_p]),
    'yunet_dp_fwd': (C.c_int, [C.POINTER(YunetDP), C.c_void_p]),
    'yunet_dp_bwd': (C.c_int, [C.POINTER(YunetDP), C.c_void_p]),
    'yunet_dp_fwd_group': (C.c_int, [C.POINTER(C.POINTER(YunetDP)), C.c_int, C.c_void_p]),
    'yunet_dp_bwd_blocks': (C.c_int, [C.c_int] * 5),
    'yunet_stem_bwd_blocks': (C.c_int, [C.c_int] * 3),
    'yunet_pool_fwd': (C.c_int, [C.c_void_p, C.POINTER(YunetBN), C.c_void_p] + [C.c_int] * 4 +
                       [C.c_void_p]),
    'yunet_dp_pool_fusion_ok': (C.c_int, [C.c_int] * 5),
    'yunet_dp_bwd_reads_z': (C.c_int, [C.POINTER(YunetDP)]),
    'yunet_dp_fwd_group_one_grid': (C.c_int, [C.POINTER(C.POINTER(YunetDP)), C.c_int]),
    'yunet_dp_route': (C.c_int, [C.POINTER(YunetDP), C.c_int, C.c_char_p, C.c_int]),
    'yunet_pool_bwd': (C.c_int, [C.c_void_p, C.POINTER(YunetBN), C.c_void_p, C.c_void_p] +
                       [C.c_int] * 5 + [C.c_void_p]),
    'yunet_pool_bwd_add': (C.c_int, [C.c_void_p, C.POINTER(YunetBN), C.c_void_p, C.c_void_p, C.c_void_p] +
                           [C.c_int] * 5 + [C.c_void_p]),
    'yunet_upadd_fwd': (C.c_int, [C.c_void_p, C.POINTER(YunetBN), C.c_void_p, C.POINTER(YunetBN),
                                  C.c_void_p] + [C.c_int] * 4 + [C.c_void_p]),
    'yunet_upadd_bwd': (C.c_int, [C.c_void_p, C.POINTER(YunetBN), C.c_void_p, C.POINTER(YunetBN),
                                  C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int] +
                        [C.c_int] * 4 + [C.c_void_p]),
    'yunet_bn_update_running': (C.c_int, [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_float,
                                                             C.c_void_p]),
    'yunet_bn_param_grad': (C.c_int, [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p]),
    'yunet_bn_batch': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                 C.c_void_p, C.c_int, C.c_void_p]),
    'yunet_reduce_partials_batch': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    'yunet_detect': (C.c_int, [C.c_void_p, C.POINTER(YunetLevels), C.c_int, C.c_int, C.c_float, C.c_float,
                              C.c_int] + [C.c_void_p] * 5),
    'yunet_detect_scratch_bytes': (C.c_size_t, [C.c_int, C.c_int]),
    'yunet_nms': (C.c_int, [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_float, C.c_float, C.c_int] + [C.c_void_p] * 5),
    'yunet_detect_soft': (C.c_int, [C.c_void_p, C.POINTER(YunetLevels), C.c_int, C.c_int, C.c_float, C.POINTER(YunetSoftNms),
                                   C.c_int] + [C.c_void_p] * 5),
    'yunet_soft_nms': (C.c_int, [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_float, C.POINTER(YunetSoftNms), C.c_int] +
                       [C.c_void_p] * 5),
    'yunet_aug_decide': (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.POINTER(YunetAugCfg), C.c_int, C.c_int, C.c_int, C.c_uint32,
                                                      C.c_int] + [C.c_void_p] * 5),
    'yunet_aug_ignore': (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p] * 3),
    'yunet_aug_pixels': (C.c_int, [C.POINTER(YunetAugPixels), C.POINTER(YunetAugCfg), C.c_int, C.c_void_p, C.c_void_p]),
    'yunet_aug_photometric': (C.c_int, [C.POINTER(YunetPhotoCfg), C.c_uint32, C.c_uint32, C.c_int, C.c_void_p,
                                        C.c_void_p]),
    'yunet_aug_mosaic_decide': (C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5 +
                                [C.POINTER(YunetMosaicCfg), C.c_uint32] + [C.c_void_p] * 6),
    'yunet_aug_mosaic_canvas': (C.c_int, [C.c_void_p] * 3 + [C.POINTER(YunetMosaicCfg), C.c_int, C.c_void_p, C.c_void_p]),
    'yunet_aug_cutout': (C.c_int, [C.POINTER(YunetCutoutCfg), C.c_uint32, C.c_int, C.c_int] + [C.c_void_p] * 4),
    'yunet_aug_affine_decide': (C.c_int, [C.POINTER(YunetAffineCfg), C.c_uint32, C.c_int, C.c_int] + [C.c_void_p] * 9),
    'yunet_aug_affine_pixels': (C.c_int, [C.c_void_p, C.POINTER(C.c_float * 3), C.c_int, C.c_int] + [C.c_void_p] * 4),
    'yunet_aug_mixup_decide': (C.c_int, [C.POINTER(YunetMixupCfg), C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_int] +
                               [C.c_void_p] * 13),
    'yunet_aug_mixup_pixels': (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_int] +
                               [C.c_void_p] * 5),
    'yunet_test_pixels': (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_void_p, C.c_void_p]),
    'yunet_rescale_dets': (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p]),
    'yunet_score_wider': (C.c_int, [C.c_void_p] * 5 + [C.c_int, C.c_longlong, C.c_longlong, C.c_double, C.c_void_p, C.c_int] +
                          [C.c_void_p] * 7),
    'yunet_score_wider_match': (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_longlong, C.c_longlong, C.c_double] +
                                [C.c_void_p] * 4),
    'yunet_score_map_tpfp': (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_longlong, C.c_longlong, C.c_float] +
                             [C.c_void_p] * 5),
    'yunet_score_rank_scratch_bytes': (C.c_size_t, [C.c_longlong]),
    'yunet_score_rank_images': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p]),
    'yunet_score_rank_global': (C.c_int, [C.c_void_p, C.c_longlong] + [C.c_void_p] * 3),
    'yunet_score_map_curve': (C.c_int, [C.c_void_p] * 3 + [C.c_longlong] + [C.c_void_p] * 6),
    'yunet_aug_gather': (C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_int] +
                         [C.c_void_p] * 6),
    'yunet_aug_window_plan': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'yunet_upload_windows': (C.c_int, [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]),
    'yunet_fetch_windows': (C.c_int, [C.c_void_p, C.c_longlong] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_longlong,
                                                                         C.c_void_p, C.c_void_p]),
    'yunet_ema_update': (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_longlong), C.c_int,
                                   C.c_float, C.c_float, C.c_void_p]),
    'yunet_box_size_hist': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int] +
                            [C.c_void_p] * 4 + [C.c_int, C.c_void_p]),
    'yunet_reduce_partials': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                        C.c_void_p]),
    'yunet_assign': (C.c_int, [C.c_void_p] * 5 + [C.POINTER(YunetLevels)] + [C.c_int] * 3 +
                     [C.c_float] + [C.c_void_p] * 6),
    'yunet_assign_ex': (C.c_int, [C.c_void_p] * 7 + [C.POINTER(YunetLevels)] + [C.c_int] * 3 +
                        [C.c_float] + [C.c_void_p] * 6),
    'yunet_assign_cfg': (C.c_int, [C.c_void_p] * 7 + [C.POINTER(YunetLevels)] + [C.c_int] * 3 +
                         [C.POINTER(YunetAssignCfg)] + [C.c_void_p] * 6),
    'yunet_loss_norm': (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    'yunet_loss': (C.c_int, [C.c_void_p] * 5 + [C.POINTER(YunetLevels), C.POINTER(YunetLossCfg),
                                                C.c_void_p] + [C.c_int] * 3 +
                   [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    'yunet_loss_terms': (C.c_int, [C.c_void_p] * 5 + [C.POINTER(YunetLevels), C.POINTER(YunetLossCfg),
                                                      C.POINTER(YunetLossTerms), C.c_void_p] + [C.c_int] * 3 +
                         [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    'yunet_loss_terms_ex': (C.c_int, [C.c_void_p] * 5 + [C.POINTER(YunetLevels), C.POINTER(YunetLossCfg),
                                                         C.POINTER(YunetLossTerms), C.c_int, C.c_void_p] + [C.c_int] * 3 +
                            [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    'yunet_ignore_mark': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(YunetLevels), C.c_int, C.c_int, C.c_int, C.c_float] +
                          [C.c_void_p] * 3),
    'yunet_loss_finalize': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'yunet_loss_finalize_ex': (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 5),
    'yunet_sgd_step_ex': (C.c_int, [C.c_void_p] * 3 + [C.c_int64, C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_float,
                                    C.c_float, C.c_int, C.c_void_p]),
    'yunet_add': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'yunet_grad_norm': (C.c_int, [C.c_void_p, C.c_int64, C.c_float, C.c_int, C.c_float] + [C.c_void_p] * 3),
    'yunet_sgd_step_grouped': (C.c_int, [C.c_void_p] * 3 + [C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int,
                                         C.c_float, C.c_void_p, C.c_int, C.c_void_p]),
    'yunet_adam_step_grouped': (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int,
                                          C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    'yunet_grad_accum': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    'yunet_sgd_step': (C.c_int, [C.c_void_p] * 3 + [C.c_int64, C.c_void_p, C.c_float, C.c_float,
                                                    C.c_float, C.c_int, C.c_void_p]),
    'yunet_exec': (C.c_int, [C.POINTER(YunetOp), C.c_int, C.c_void_p]),
    'yunet_exec_lanes': (C.c_int, [C.c_int]),
    'yunet_set_option': (C.c_int, [C.c_char_p, C.c_int]),
    'yunet_comm_inbox_bytes': (C.c_size_t, [C.c_int, C.c_size_t]),
    'yunet_comm_alloc': (C.c_int, [C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    'yunet_comm_free': (C.c_int, [C.c_void_p, C.c_void_p]),
    'yunet_comm_export': (C.c_int, [C.c_void_p, C.c_char_p]),
    'yunet_comm_open': (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    'yunet_comm_close': (C.c_int, [C.c_void_p]),
    'yunet_allreduce': (C.c_int, [C.POINTER(YunetComm), C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    'yunet_comm_status': (C.c_int, [C.POINTER(YunetComm)]),
}
for _n in ('yunet_stem_fwd', 'yunet_stem_bwd', 'yunet_stem_bwd_dx', 'yunet_dp_fwd', 'yunet_dp_bwd', 'yunet_dp_fwd_group', 'yunet_pool_fwd', 'yunet_pool_bwd',
           'yunet_pool_bwd_add', 'yunet_upadd_fwd', 'yunet_upadd_bwd'):
    _SIGNATURES[_n + '_bf16'] = _SIGNATURES[_n]      # same arguments, bf16 activation storage

EXPORTED = sorted(_SIGNATURES)

_lib = None


class YunetHipError(RuntimeError):
    pass


def load():
    """dlopen the kernel library (no GPU needed to load it); raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise YunetHipError(
            f'{LIB_PATH} not found: the HIP extension is not built.  Run '
            '`python __graft_entry__.py` (or `make -C libfacedetection.train_amd/csrc`). '
            'There is no CPU fallback.')
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.yunet_abi_version() != 12:
        raise YunetHipError('libyunet_hip.so ABI version mismatch; rebuild it')
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        raise YunetHipError(f'{what} failed with status {rc}')


def set_option(name, value):
    """yunet_set_option(): a measurement switch of the C dispatchers (include/yunet_hip.h); returns the previous value."""
    rc = load().yunet_set_option(name.encode(), int(value))
    if rc < 0:
        raise YunetHipError(f'yunet_set_option({name!r}, {value}) rejected')
    return rc
