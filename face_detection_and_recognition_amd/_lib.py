"""ctypes binding of libfacepath.so (the C ABI declared in include/facepath.h).

There is no CPU fallback: if the shared library is missing or a symbol cannot be
resolved, loading raises.  Build it with ``python -c "import __graft_entry__ as g; g.build()"``
or ``make -C face_detection_and_recognition_amd/csrc``.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfacepath.so")

FP_OK = 0
FP_ERR_INVALID_ARG = -1
ABI_VERSION = 15

# fp_op_kind
OP_CONV, OP_DWCONV, OP_MAXPOOL, OP_UPSAMPLE2X, OP_COPY, OP_L2NORM, OP_BLAZEBLOCK, OP_DWPW, OP_YSTEM = 1, 2, 3, 4, 5, 6, 7, 8, 9
OP_YSTEM_U8, OP_STEM_U8, OP_DWBLOCK, OP_BLAZEPAIR, OP_BLAZECHAIN, OP_SHUFDOWN, OP_SHUFUNIT, OP_YSTEM2 = 10, 11, 12, 13, 14, 15, 16, 17
OP_EMBED_HEAD = 18
OP_POOL_LRN, OP_CLS_HEAD = 19, 20
# fp_act
ACT_NONE, ACT_RELU, ACT_PRELU, ACT_SILU = 0, 1, 2, 3
# fp_res_mode
RES_NONE, RES_ADD_BEFORE_ACT, RES_ADD_AFTER_ACT, RES_POOL2_BEFORE_ACT, RES_SHUFFLE2 = 0, 1, 2, 3, 4
OPF_IN_ROWPAD, OPF_OUT_ROWPAD = 1, 2   # fp_op.flags: row-padded input / output view (include/facepath.h)
OPF_IN_C3 = 4                          # 4-float pixel whose fourth channel meets zero weights
OPF_IN_UP2 = 32                        # CONV (split pointwise): leading input channels = a half-size map upsampled 2x (nearest)
OPF_OUT_DW = 64                        # CONV (Mobile-FaceNet stem): a depthwise 3x3 Conv_block behind the conv, in the same kernel
OPF_SPLIT3 = 8                         # GEMM weights packed as three bf16 planes (bf16x6 split-MFMA kernels)
OPF_OUT_L2 = 128                       # EMBED_HEAD: every output row L2-normalised (F.normalize)


class FpOp(C.Structure):
    """Mirror of struct fp_op (include/facepath.h)."""
    _fields_ = [
        ("kind", C.c_int32), ("act", C.c_int32), ("res_mode", C.c_int32),
        ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
        ("OH", C.c_int32), ("OW", C.c_int32),
        ("Cin", C.c_int32), ("Cout", C.c_int32),
        ("KH", C.c_int32), ("KW", C.c_int32), ("stride", C.c_int32),
        ("pad_t", C.c_int32), ("pad_l", C.c_int32),
        ("in_ld", C.c_int32), ("out_ld", C.c_int32), ("res_ld", C.c_int32),
        ("out_cmul", C.c_int32), ("res_C", C.c_int32),
        ("res_H", C.c_int32), ("res_W", C.c_int32),
        ("in_ns", C.c_int64), ("out_ns", C.c_int64), ("res_ns", C.c_int64),
        ("in_off", C.c_int64), ("out_off", C.c_int64), ("res_off", C.c_int64),
        ("w_off", C.c_int64), ("scale_off", C.c_int64), ("bias_off", C.c_int64), ("slope_off", C.c_int64),
        ("act2", C.c_int32), ("flags", C.c_int32),
        ("Cmid", C.c_int32), ("row_lo", C.c_int16), ("row_end", C.c_int16),
    ]


class FpExt(C.Structure):
    """Mirror of struct fp_ext: an external device buffer of a plan (pointer, readable bytes)."""
    _fields_ = [("ptr", C.c_void_p), ("bytes", C.c_size_t)]


class FpResizeItem(C.Structure):
    """Mirror of struct fp_resize_item."""
    _fields_ = [("src_image", C.c_int32), ("sx", C.c_int32), ("sy", C.c_int32), ("sw", C.c_int32), ("sh", C.c_int32),
                ("dx", C.c_int32), ("dy", C.c_int32), ("dw", C.c_int32), ("dh", C.c_int32)]


class FpFrameDesc(C.Structure):
    """Mirror of struct fp_frame_desc (ABI 14): one frame of a ragged batch (byte offset of pixel (0, 0), size)."""
    _fields_ = [("off", C.c_int64), ("h", C.c_int32), ("w", C.c_int32)]


class FpTtaView(C.Structure):
    """Mirror of struct fp_tta_view: one scaled view of the augmented inference (include/facepath.h)."""
    _fields_ = [("content_h", C.c_int32), ("content_w", C.c_int32), ("padded_h", C.c_int32), ("padded_w", C.c_int32),
                ("flip", C.c_int32), ("reserved", C.c_int32)]


FRAME_MIN_W, FRAME_MAX_W, FRAME_MAX_H = 3, 32767, 65535   # fp_frame_desc sizes the ragged kernels take
RAGGED_U8, RAGGED_F32_LUT = 0, 1                           # fp_resize_ragged output modes
TOPK_MAX = 16                                              # FP_TOPK_MAX: largest k of fp_cosine_topk_x6
COARSE_MAX, QUANT_MAX_D = 64, 1024                         # FP_COARSE_MAX: largest pool of fp_cosine_topk_i8; FP_QUANT_MAX_D
DBSCAN_MAX_MIN_SAMPLES = 64                               # largest min_samples of fp_cosine_dbscan_x6
PAIRHIST_MAX_BINS = 1024                                   # FP_PAIRHIST_MAX_BINS: most bins of fp_pair_histogram_x6
ALIGN_SIZE, ALIGN_DEGENERATE = 112, 1                      # fp_align_warp canvas side, fp_dets_to_crops_aligned flag
DETEVAL_MAX_THRS, DETEVAL_MAX_RECS = 31, 1024              # FP_DETEVAL_MAX_*: IoU / recall thresholds fp_det_match / fp_pr_accumulate take


class FpJpegInfo(C.Structure):
    """Mirror of struct fp_jpeg_info."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("ncomp", C.c_int32), ("restart_interval", C.c_int32),
                ("progressive", C.c_int32), ("reserved", C.c_int32), ("hs", C.c_int32 * 3), ("vs", C.c_int32 * 3),
                ("mcux", C.c_int32), ("mcuy", C.c_int32), ("blocks_w", C.c_int32 * 3), ("blocks_h", C.c_int32 * 3),
                ("comp_w", C.c_int32 * 3), ("comp_h", C.c_int32 * 3), ("coef_off", C.c_int64 * 3), ("n_coefs", C.c_int64),
                ("quant", (C.c_uint16 * 64) * 3)]


class FpJpegHuff(C.Structure):
    """Mirror of struct fp_jpeg_huff."""
    _fields_ = [("look", C.c_uint16 * 512), ("maxcode", C.c_int32 * 18), ("valoff", C.c_int32 * 18), ("vals", C.c_uint8 * 256)]


class FpJpegScan(C.Structure):
    """Mirror of struct fp_jpeg_scan (ABI 12)."""
    _fields_ = [("data_off", C.c_int64), ("data_len", C.c_int64), ("n_coefs", C.c_int64), ("coef_off", C.c_int64 * 3),
                ("blocks_w", C.c_int32 * 3), ("mcux", C.c_int32), ("mcuy", C.c_int32), ("restart_interval", C.c_int32),
                ("blocks_per_mcu", C.c_int32), ("ncomp", C.c_int32), ("slot_comp", C.c_uint8 * 8), ("slot_tab", C.c_uint8 * 8),
                ("slot_dy", C.c_uint8 * 8), ("slot_dx", C.c_uint8 * 8), ("hs", C.c_int32 * 3), ("vs", C.c_int32 * 3),
                ("dc", FpJpegHuff * 3), ("ac", FpJpegHuff * 3)]


class FpJpegEncItem(C.Structure):
    """Mirror of struct fp_jpeg_enc_item (ABI 13)."""
    _fields_ = [("src_off", C.c_int64), ("src_h", C.c_int32), ("src_w", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32),
                ("x1", C.c_int32), ("y1", C.c_int32)]


class FpDrawCmd(C.Structure):
    """Mirror of struct fp_draw_cmd: one 32-byte drawing command (include/facepath.h "Drawing on device frames")."""
    _fields_ = [("frame", C.c_int32), ("kind", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32),
                ("y1", C.c_int32), ("b", C.c_uint8), ("g", C.c_uint8), ("r", C.c_uint8), ("a", C.c_uint8), ("arg", C.c_int32)]


DRAW_RECT, DRAW_FILL, DRAW_RING, DRAW_GLYPH, DRAW_MOSAIC = 1, 2, 3, 4, 5   # fp_draw_kind
DRAW_TILE, DRAW_FONT_BYTES = 64, 760                                       # FP_DRAW_TILE, FP_DRAW_FONT_BYTES
DRAW_MAX_ARG, DRAW_MAX_SCALE, DRAW_MAX_COORD = 4096, 64, 1 << 20           # FP_DRAW_MAX_*
DRAW_MOSAIC_CELLS = (4, 8, 16, 32)
MERGE_CAP = 2048                                                           # FP_MERGE_CAP: candidates fp_merge_views takes per frame
QUALITY_MAX_STEP = 64                                                     # FP_QUALITY_MAX_STEP
QUALITY_EMPTY, QUALITY_BAD_FRAME, QUALITY_NO_LAPLACIAN, QUALITY_TOO_LARGE, QUALITY_POSE_DEGENERATE = 1, 2, 4, 8, 16   # FP_QUALITY_*

TRACK_SLOTS, TRACK_MAX_DETS, TRACK_MAX_DIM, TRACK_MAX_ROWS = 64, 64, 1024, 1 << 30                     # FP_TRACK_*
TRACK_SLOT_INTS, TRACK_SLOT_FLOATS = 5, 10                                # columns of fp_track_state.slot_i / slot_f
TRACK_MOTION_FLOATS = 20                  # FP_TRACK_MOTION_FLOATS: x, v, p00, p01, p11 of cx, cy, w, h per slot of `motion`
TRACK_NEW, TRACK_BEST, TRACK_DEAD_ROW, TRACK_FULL, TRACK_NO_STREAM, TRACK_OVER = 1, 2, 4, 8, 16, 32   # track_flags bits
TRACK_LOST, TRACK_REVIVED = 64, 64        # FP_TRACK_LOST: parked tracks per stream of fp_track_lost; FP_TRACK_REVIVED: a track_flags bit
TRACK_POOL = 128                          # FP_TRACK_POOL: template entries per stream of fp_track_templates
TRACK_TPL_EVICTED, TRACK_TPL_RESTART = 1, 2   # FP_TRACK_TPL_*: track_emb_flags bits
MOT_MAX_ROWS, MOT_STATE_ROWS = 64, 6   # FP_MOT_MAX_ROWS: rows of one frame fp_mot_match takes; int32 rows of its per-id state
HOTA_MAX_ALPHAS = 32                   # FP_HOTA_MAX_ALPHAS: localisation thresholds fp_hota_match takes


class FpTrackState(C.Structure):
    """Mirror of struct fp_track_state: the five state arrays of fp_tracklets_step (include/facepath.h "Tracklets")."""
    _fields_ = [("hdr", C.c_void_p), ("slot_i", C.c_void_p), ("slot_f", C.c_void_p), ("emb", C.c_void_p), ("best_emb", C.c_void_p)]


class FpTrackLost(C.Structure):
    """Mirror of struct fp_track_lost: the five pool arrays of fp_tracklets_step_reid ("Tracklets: re-identification")."""
    _fields_ = [("lost_hdr", C.c_void_p), ("lost_i", C.c_void_p), ("lost_f", C.c_void_p), ("lost_emb", C.c_void_p),
                ("lost_best_emb", C.c_void_p)]


class FpTrackTemplates(C.Structure):
    """Mirror of struct fp_track_templates: the three table arrays of fp_track_pool_step ("Tracklets: templates")."""
    _fields_ = [("tpl_i", C.c_void_p), ("tpl_w", C.c_void_p), ("tpl_sum", C.c_void_p)]


JPEG_DECODE_ON_HOST = 1          # fp_jpeg_entropy_decode_device status: decode this image with fp_jpeg_entropy_decode
JPEG_444, JPEG_422, JPEG_420 = 0, 1, 2   # fp_jpeg_encode_* subsampling (Pillow's numbering)
JPEG_ENC_BYTES_PER_BLOCK = 416   # worst-case scan bytes of one 8 x 8 block, stuffing included
JPEG_ENC_HEADER_BYTES = 623      # what fp_jpeg_encode_headers writes

_P = C.c_void_p
_I = C.c_int
_F = C.c_float
_SZ = C.c_size_t
_I64 = C.c_int64
_D = C.c_double

# the six fp_tracklets_step* entry points: [state(, lost)] + rows (+ reid tail) (+ motion tail) (+ stream on the device path)
_TK_ROWS = [_I, _I, _P, _P, _P, _P, _P, _I, _P, _I, _I, _F, _F, _F, _P, _P, _P, _P]   # n_streams .. track_flags
_TK_MOTION = [_P, _F, _F, _P]                                                         # motion, std_pos, std_vel, track_pred
_TK_REID = [_F, _I]                                                                   # tau_reid, lost_age

# fp_track_pool_step*: [tpl] + n_streams .. track_emb_flags (+ workspace, workspace_bytes, stream on the device path)
_TP_ROWS = [_I, _I, _P, _P, _P, _P, _I, _P, _I, _P, _P, _P, _I, _P, _P, _P]

# name -> (restype, argtypes); every symbol declared in include/facepath.h
SIGNATURES = {
    "fp_abi_version": (_I, []),
    "fp_selftest": (_I, []),
    "fp_debug_reload_env": (None, []),
    "fp_strerror": (C.c_char_p, [_I]),
    "fp_last_hip_error": (C.c_char_p, []),
    "fp_plan_run": (_I, [C.POINTER(FpOp), _I, _P, _SZ, _P, _SZ, _P]),
    "fp_plan_run_ext": (_I, [C.POINTER(FpOp), _I, _P, _SZ, _P, _SZ, C.POINTER(FpExt), _I, _P]),
    "fp_plan_validate": (_I, [C.POINTER(FpOp), _I, _SZ, _SZ]),
    "fp_timer_create": (_I, [_I, C.POINTER(_P)]),
    "fp_timer_destroy": (None, [_P]),
    "fp_plan_run_timed": (_I, [C.POINTER(FpOp), _I, _P, _SZ, _P, _SZ, _P, _P, C.POINTER(C.c_ubyte)]),
    "fp_plan_run_timed_ext": (_I, [C.POINTER(FpOp), _I, _P, _SZ, _P, _SZ, C.POINTER(FpExt), _I, _P, _P,
                                   C.POINTER(C.c_ubyte)]),
    "fp_timer_accumulate": (_I, [_P, C.POINTER(_F), _I]),
    "fp_op_kernel_name": (C.c_char_p, [C.POINTER(FpOp)]),
    "fp_resize_normalize": (_I, [_P, _I, _I, _I, _P, _I, _P, _I, _I, _I, _P, _I, _I, _P]),
    "fp_letterbox_tables": (_I, [_I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "fp_dets_to_crops": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _F, _F, _F, _F, _F, _I, _I, _I, _I, _I, _I, _I,
                                _P, _P, _P, _P]),
    "fp_resize_ragged": (_I, [_P, _SZ, _P, _I, _P, _I, _P, _I, _I, _I, _I, _P, _I, _I, _P]),
    "fp_dets_to_crops_ragged": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _F, _F, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P,
                                       _P]),
    "fp_dets_to_crops_aligned": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _F, _F, _F, _F, _F, _I, _I, _I, _I, _I, _I, _I,
                                        _P, _P, _P, _P, _P, _P, _P]),
    "fp_dets_to_crops_aligned_ragged": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _F, _F, _I, _I, _I, _I, _I, _I, _I, _P,
                                               _P, _P, _P, _P, _P, _P]),
    "fp_dets_to_crops_aligned_emulate": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _F, _F, _I, _I, _I, _I, _I, _I, _I, _P,
                                                _P, _P, _P, _P, _P]),
    "fp_align_warp": (_I, [_P, _I, _I, _I, _P, _P, _P, _P, _I, _P, _P, _I, _P, _P]),
    "fp_align_warp_ragged": (_I, [_P, _SZ, _P, _I, _P, _P, _P, _P, _I, _P, _P, _I, _P, _P]),
    "fp_align_emulate": (_I, [_P, _SZ, _P, _I, _P, _I, _P, _P, _P, _P, _I, _P]),
    "fp_blaze_decode": (_I, [_P, _P, _P, _I, _I, _F, _F, _F, _F, _F, _F, _P, _P, _P]),
    "fp_blaze_weighted_nms": (_I, [_P, _P, _I, _I, _F, _P, _P, _P, _P]),
    "fp_yolo_decode": (_I, [_P, _I, _I, _I, _I, _F, C.POINTER(_F), _P, _I64, _I64, _P]),
    "fp_tta_views": (_I, [_P, _I, _I, _I, C.POINTER(FpTtaView), _P, _P, _F, _P]),
    "fp_yolo_decode_view": (_I, [_P, _I, _I, _I, _I, _F, C.POINTER(_F), _P, _I64, _I64, _F, _I, _I, _I, _P]),
    "fp_yolo_nms": (_I, [_P, _I, _I, _F, _F, _I, _I, _P, _P, _P, _P, _P, _SZ, _P]),
    "fp_yolo_nms_scratch_bytes": (_SZ, [_I, _I]),
    "fp_yolo_w_nms": (_I, [_P, _I, _I, _F, _F, _I, _I, _P, _P, _P, _P, _P, _SZ, _P]),
    "fp_row_inv_norm": (_I, [_P, _I64, _I, _P, _P]),
    "fp_cosine_filter": (_I, [_P, _P, _I64, _P, _P, _I, _I, _F, _P, _P, _P, _P, _P]),
    "fp_split3_bytes": (_SZ, [_I, _I]),
    "fp_split3_rows": (_I, [_P, _I, _I, _P, _P]),
    "fp_cosine_filter_x6": (_I, [_P, _P, _I64, _P, _P, _I, _I, _F, _P, _P, _P, _P, _P]),
    "fp_cosine_filter_x6_tile_rows": (_I, [_I64, _I]),
    "fp_cosine_topk_workspace": (_SZ, [_I64, _I, _I, _I]),
    "fp_cosine_topk_x6": (_I, [_P, _P, _I64, _P, _P, _I, _I, _I, _I, _P, _P, _P, _SZ, _P]),
    "fp_quant_i8_bytes": (_SZ, [_I, _I]),
    "fp_quantize_rows_i8": (_I, [_P, _I, _I, _P, _P, _P]),
    "fp_cosine_topk_i8_workspace": (_SZ, [_I64, _I, _I, _I]),
    "fp_cosine_topk_i8": (_I, [_P, _P, _I64, _P, _P, _I, _I, _I, _I, _P, _P, _P, _SZ, _P]),
    "fp_rerank_topk": (_I, [_P, _P, _I64, _I, _P, _I, _P, _P, _P, _I, _I, _P, _P, _P]),
    "fp_topk_vote": (_I, [_P, _P, _I64, _I, _P, _I, _F, _I, _P, _P, _P, _P]),
    "fp_cosine_dbscan_workspace": (_SZ, [_I64, _I]),
    "fp_cosine_dbscan_x6": (_I, [_P, _P, _P, _I64, _I, _F, _I, _P, _P, _P, _P, _P, _SZ, _P]),
    "fp_cluster_centroids": (_I, [_P, _P, _P, _P, _I, _I, _P, _P, _P]),
    "fp_pair_histogram_workspace": (_SZ, [_I64]),
    "fp_pair_histogram_x6": (_I, [_P, _P, _P, _P, _I64, _I, _F, _F, _I, _P, _P, _P, _SZ, _P]),
    "fp_l2_mean_thres": (_I, [_P, _I, _I, _P, _P, _P]),
    "fp_l2_filter": (_I, [_P, _I64, _I, _P, _P, _P, _P, _P]),
    "fp_resize_standardize": (_I, [_P, _I, _I, _I, _P, _I, _I, _P, _P]),
    "fp_crop_resize_f32": (_I, [_P, _I, _I, _P, _I, _P, _I, _I, _P]),
    "fp_jpeg_parse": (_I, [_P, _SZ, C.POINTER(FpJpegInfo)]),
    "fp_jpeg_entropy_decode": (_I, [_P, _SZ, C.POINTER(FpJpegInfo), _P]),
    "fp_jpeg_workspace_bytes": (_SZ, [C.POINTER(FpJpegInfo)]),
    "fp_jpeg_reconstruct": (_I, [_P, C.POINTER(FpJpegInfo), _P, _SZ, _P, _I, _P]),
    "fp_jpeg_batch_workspace_bytes": (_SZ, [C.POINTER(FpJpegInfo), _I]),
    "fp_jpeg_reconstruct_batch": (_I, [_P, _P, _P, C.POINTER(FpJpegInfo), _I, _P, _SZ, _P, _I, _P]),
    "fp_jpeg_exif_orientation": (_I, [_P, _SZ]),
    "fp_jpeg_scaled_size": (_I, [C.POINTER(FpJpegInfo), _I, _I, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "fp_jpeg_scaled_workspace_bytes": (_SZ, [C.POINTER(FpJpegInfo), _I]),
    "fp_jpeg_reconstruct_scaled": (_I, [_P, C.POINTER(FpJpegInfo), _I, _I, _P, _SZ, _P, _I, _P]),
    "fp_jpeg_reconstruct_scaled_emulate": (_I, [_P, C.POINTER(FpJpegInfo), _I, _I, _P, _SZ, _P, _I]),
    "fp_jpeg_scan_prepare": (_I, [_P, _SZ, C.POINTER(FpJpegInfo), C.POINTER(FpJpegScan)]),
    "fp_jpeg_entropy_workspace_bytes": (_SZ, [C.POINTER(FpJpegScan), _I, _I, _I]),
    "fp_jpeg_entropy_decode_device": (_I, [_P, C.POINTER(FpJpegScan), C.POINTER(_I64), _I, _P, C.POINTER(_I64), _P, _P, _SZ, _I,
                                           _I, _P]),
    "fp_jpeg_entropy_decode_emulate": (_I, [_P, _SZ, C.POINTER(FpJpegScan), _P, _I, _I, C.POINTER(C.c_int32)]),
    "fp_jpeg_encode_workspace_bytes": (_I, [C.POINTER(FpJpegEncItem), _I, _I, C.POINTER(_SZ), C.POINTER(_SZ)]),
    "fp_jpeg_encode_headers": (_I, [_I, _I, _I, _I, _P, _SZ]),
    "fp_jpeg_encode_device": (_I, [_P, C.POINTER(FpJpegEncItem), _I, _I, _I, _I, _P, _SZ, _P, _SZ, _P, _P]),
    "fp_jpeg_encode_emulate": (_I, [_P, C.POINTER(FpJpegEncItem), _I, _I, _I, _I, _P, _SZ, C.POINTER(_I64)]),
    "fp_attr_crop_items": (_I, [_P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "fp_attr_crop_items_emulate": (_I, [_P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _P]),
    "fp_pnet_level_images": (_I, [_P, _SZ, _P, _I, _P, _I, _I, _I, _P, _P]),
    "fp_pnet_threshold": (_I, [_P, _I, _P, _I, _I, _I, _I, _I, _F, _I, _P, _P, _P, _P]),
    "fp_mtcnn_scratch_bytes": (_SZ, [_I, _I]),
    "fp_mtcnn_stage1": (_I, [_P, _P, _I, _I, _P, _I, _P, _P, _P, _P, _P, _SZ, _P]),
    "fp_mtcnn_cut": (_I, [_P, _SZ, _P, _I, _P, _I, _P, _I, _I, _P, _P, _P]),
    "fp_mtcnn_stage2": (_I, [_P, _I, _I, _P, _P, _I, _P, _I, _F, _P, _P, _P, _P, _SZ, _P]),
    "fp_mtcnn_stage3": (_I, [_P, _I, _I, _P, _P, _I, _P, _I, _F, _I, _P, _P, _P, _P, _SZ, _P]),
    "fp_mtcnn_boxes": (_I, [_P, _P, _I, _I, _I, _P, _P, _P]),
    "fp_mtcnn_nms": (_I, [_P, _P, _P, _I, _I, _F, _I, _P, _P, _P, _SZ, _P]),
    "fp_dets_to_crops_px": (_I, [_P, _P, _I, _I, _I, _P, _F, _F, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "fp_tracker_step": (_I, [_P, _P, _P, _I, _I, _P, _P, _I, _I, _F, _F, _P, _P, _P]),
    "fp_det_match_workspace": (_SZ, [_I64, _I]),
    "fp_det_match": (_I, [_P, _P, _P, _P, _P, _I, _I64, _I64, _P, _I, _P, _I, _P, _P, _P, _P, _SZ, _P]),
    "fp_pr_accumulate": (_I, [_P, _P, _P, _P, _I64, _P, _I, _I, _P, _I, _P, _I, _P, _P, _P]),
    "fp_draw": (_I, [_P, _SZ, _P, _I, _P, _P, _I, _P, _I, _P, _P]),
    "fp_draw_check": (_I, [_SZ, _P, _I, _P, _P, _I, _P, _I]),
    "fp_draw_emulate": (_I, [_P, _SZ, _P, _I, _P, _P, _I, _P, _I, _P]),
    "fp_face_quality": (_I, [_P, _SZ, _P, _I, _P, _I, _P, _P, _P]),
    "fp_face_quality_emulate": (_I, [_P, _SZ, _P, _I, _P, _I, _P, _P]),
    "fp_face_pose": (_I, [_P, _I, _I, _P, _P, _P]),
    "fp_face_pose_emulate": (_I, [_P, _I, _I, _P, _P]),
    "fp_merge_views": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _I, _F, _F, _I, _P, _P, _P, _P]),
    "fp_merge_views_emulate": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _I, _F, _F, _I, _P, _P, _P]),
    "fp_gather_tiles": (_I, [_P, _SZ, _P, _I, _P, _I, _I, _I, _P, _P]),
    "fp_tracklets_step": (_I, [C.POINTER(FpTrackState)] + _TK_ROWS + [_P]),
    "fp_tracklets_step_emulate": (_I, [C.POINTER(FpTrackState)] + _TK_ROWS),
    "fp_tracklets_step_motion": (_I, [C.POINTER(FpTrackState)] + _TK_ROWS + _TK_MOTION + [_P]),
    "fp_tracklets_step_motion_emulate": (_I, [C.POINTER(FpTrackState)] + _TK_ROWS + _TK_MOTION),
    "fp_tracklets_step_reid": (_I, [C.POINTER(FpTrackState), C.POINTER(FpTrackLost)] + _TK_ROWS + _TK_REID + _TK_MOTION + [_P]),
    "fp_tracklets_step_reid_emulate": (_I, [C.POINTER(FpTrackState), C.POINTER(FpTrackLost)] + _TK_ROWS + _TK_REID + _TK_MOTION),
    "fp_track_pool_workspace_bytes": (_SZ, [_I]),
    "fp_track_pool_step": (_I, [C.POINTER(FpTrackTemplates)] + _TP_ROWS + [_P, _SZ, _P]),
    "fp_track_pool_step_emulate": (_I, [C.POINTER(FpTrackTemplates)] + _TP_ROWS),
    "fp_mot_match_workspace": (_SZ, [_I64, _I64]),
    "fp_mot_match": (_I, [_P, _P, _P, _I64, _P, _P, _P, _I64, _P, _P, _P, _P, _I, _I64, _I64, _I64, _D, _P, _P, _P, _P, _P, _SZ, _P]),
    "fp_mot_match_emulate": (_I, [_P, _P, _P, _I64, _P, _P, _P, _I64, _P, _P, _P, _P, _I, _I64, _I64, _I64, _D, _P, _P, _P, _P, _P,
                                  _SZ]),
    "fp_hota_match_workspace": (_SZ, [_I64, _I64, _I64]),
    "fp_hota_match": (_I, [_P, _P, _P, _I64, _P, _P, _P, _I64, _P, _P, _P, _P, _I, _I64, _I64, _I64, _I64, _P, _I, _P, _P, _P, _P, _P,
                           _SZ, _P]),
    "fp_hota_match_emulate": (_I, [_P, _P, _P, _I64, _P, _P, _P, _I64, _P, _P, _P, _P, _I, _I64, _I64, _I64, _I64, _P, _I, _P, _P, _P,
                                   _P, _P, _SZ]),
}

_lib = None


class FacepathError(RuntimeError):
    pass


def load():
    """Load libfacepath.so and bind every symbol.  Raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FacepathError(
            f"{LIB_PATH} not found: the HIP extension is not built and there is no CPU fallback. "
            "Run `make -C face_detection_and_recognition_amd/csrc` (hipcc, --offload-arch=gfx950).")
    # torch bundles its own libamdhip64 (same SONAME as /opt/rocm's).  Import torch first so that this
    # library binds to the HIP runtime torch already loaded: one runtime per process, shared streams/memory.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    v = lib.fp_abi_version()
    if v != ABI_VERSION:
        raise FacepathError(f"libfacepath ABI version {v}, expected {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != FP_OK:
        lib = load()
        msg = lib.fp_strerror(rc).decode()
        hip = lib.fp_last_hip_error().decode()
        raise FacepathError(f"{what}: {msg} (status {rc})" + (f" [HIP: {hip}]" if hip else ""))


def ptr(t):
    """Device (or host) pointer of a torch tensor as c_void_p; None -> NULL."""
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())


def current_stream(device):
    """The caller's current torch stream handle (so work is ordered with torch ops and graph-capturable)."""
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
