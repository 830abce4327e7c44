"""Five-point face alignment between detection and embedding (csrc/align.hip, include/facepath.h "Face alignment").

Mobile-FaceNet, like the ArcFace family it belongs to, is trained on faces that a similarity transform has put onto a
fixed five-point template at 112 x 112.  FacePipeline(align=True) fits that transform to each face's landmarks
(fp_dets_to_crops_aligned) and warps the frame with it (fp_align_warp) instead of stretching the box crop.  These are the
thin wrappers; the arithmetic lives in the C library, with host emulators the CPU tests run."""
import ctypes

import numpy as np
import torch

from ... import _lib as L
from ...frames import frame_call_args, frame_descs, ragged_scale_coords_params
from ...frames import uniform_descs  # noqa: F401 (re-export)

SIZE = L.ALIGN_SIZE
DEGENERATE = L.ALIGN_DEGENERATE
# ArcFace 112 x 112 template (x, y): left eye, right eye, nose tip, left mouth corner, right mouth corner
TEMPLATE = np.array([[38.2946, 51.6963], [73.5318, 51.5014], [56.0252, 71.7366], [41.5493, 92.3655], [70.7299, 92.2041]])
# detector landmarks -> template points: YOLOv5-face's five in order; BlazeFace's keypoints 0..3 (eyes, nose tip, mouth
# centre; the ears 4, 5 are unused) -> points 0, 1, 2 and the midpoint of the mouth corners
YOLO_TARGETS = TEMPLATE
BLAZE_TARGETS = np.array([TEMPLATE[0], TEMPLATE[1], TEMPLATE[2], (TEMPLATE[3] + TEMPLATE[4]) * 0.5])


def targets(fmt):
    """Template points the landmarks of detector row format `fmt` (0 BlazeFace, 1 YOLOv5-face) map to."""
    return BLAZE_TARGETS if fmt == 0 else YOLO_TARGETS


def alloc(cap, device):
    """Per-face outputs of fp_dets_to_crops_aligned: dict(lmarks (cap, 10) fp32, M (cap, 6) fp64, flags (cap,) int32)."""
    return dict(lmarks=torch.empty((cap, 10), dtype=torch.float32, device=device),
                M=torch.empty((cap, 6), dtype=torch.float64, device=device),
                flags=torch.empty((cap,), dtype=torch.int32, device=device))


def warp(frames, M, info, flags, items, n, out_u8=None, out_f32=None, lut=None):
    """fp_align_warp / _ragged: the first n faces of a step -> out_u8 (n, 112, 112, 3) uint8 and / or out_f32
    (n, 112, 112, C) float32 (C = 3 or 4, through `lut`), on the frames' device and the current stream."""
    lib = L.load()
    for t in (M, info, flags, items):
        assert t.is_contiguous() and t.shape[0] >= n
    c = 0
    if out_f32 is not None:
        assert out_f32.dtype == torch.float32 and out_f32.is_contiguous() and out_f32.shape[0] >= n and lut is not None
        c = out_f32.shape[3]
    if out_u8 is not None:
        assert out_u8.dtype == torch.uint8 and out_u8.is_contiguous() and out_u8.shape[0] >= n
    ragged, fa = frame_call_args(frames)
    name = "fp_align_warp_ragged" if ragged else "fp_align_warp"
    L.check(getattr(lib, name)(*fa, L.ptr(M), L.ptr(info), L.ptr(flags), L.ptr(items), int(n), L.ptr(out_u8), L.ptr(out_f32), c,
                               L.ptr(lut), L.current_stream(frames.device)), name)


def warp_u8(frames, M, info, flags, items, n):
    """The n aligned faces as a (n, 112, 112, 3) uint8 tensor (BGR, the frames' order) on the frames' device."""
    out = torch.empty((n, SIZE, SIZE, 3), dtype=torch.uint8, device=frames.device)
    if n:
        warp(frames, M, info, flags, items, n, out_u8=out)
    return out


# ---------------------------------------------------------------------------------------------- host emulators (tests)

def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def emulate_estimate(lmarks, fmt):
    """fp_align_emulate's estimate: lmarks (n, 10) float32 -> (M (n, 6) float64, flags (n,) int32)."""
    lm = np.ascontiguousarray(lmarks, np.float32).reshape(-1, 10)
    n = lm.shape[0]
    M = np.zeros((n, 6), np.float64)
    fl = np.zeros((n,), np.int32)
    L.check(L.load().fp_align_emulate(None, 0, None, 0, _p(lm), int(fmt), _p(M), None, _p(fl), None, n, None),
            "fp_align_emulate")
    return M, fl


def emulate_warp(frames, M, info, flags, items):
    """fp_align_emulate's warp over host frames: a (B, H, W, 3) uint8 array or a list of (h, w, 3) arrays; M (n, 6) float64,
    info (n, 7) float32 (column 0 = frame), flags (n,) int32, items (n, 9) int32 -> (n, 112, 112, 3) uint8."""
    if isinstance(frames, np.ndarray) and frames.ndim == 4:
        B, H, W, _ = frames.shape
        data, descs = np.ascontiguousarray(frames).reshape(-1), uniform_descs(B, H, W)
    else:
        frames = [np.ascontiguousarray(f, np.uint8) for f in frames]
        data = np.concatenate([f.reshape(-1) for f in frames])
        offs = np.concatenate([[0], np.cumsum([f.size for f in frames])[:-1]]).astype(np.int64)
        descs = frame_descs(offs, [f.shape[:2] for f in frames])
    M = np.ascontiguousarray(M, np.float64)
    info = np.ascontiguousarray(info, np.float32)
    flags = np.ascontiguousarray(flags, np.int32)
    items = np.ascontiguousarray(items, np.int32)
    n = M.shape[0]
    out = np.zeros((n, SIZE, SIZE, 3), np.uint8)
    L.check(L.load().fp_align_emulate(_p(data), data.size, _p(descs), descs.shape[0], None, 0, _p(M), _p(info), _p(flags),
                                      _p(items), n, _p(out)), "fp_align_emulate")
    return out


def emulate_crops(dets, counts, sizes, in_size, fmt, det_thres, area_thres, offsets=(-6, -1, 4, 5), max_faces=None):
    """fp_dets_to_crops_aligned_emulate on host arrays: dets (B, max_dets, row) float32, counts (B,), sizes [(h, w)] ->
    dict(items, info, lmarks, M, flags) of the n faces found."""
    dets = np.ascontiguousarray(dets, np.float32)
    counts = np.ascontiguousarray(counts, np.int32)
    B, max_dets, row = dets.shape
    cap = max_faces or max(1, B * max_dets)
    descs = frame_descs(0, sizes)
    geom = np.ascontiguousarray(ragged_scale_coords_params(in_size, sizes))
    out = dict(items=np.zeros((cap, 9), np.int32), info=np.zeros((cap, 7), np.float32), lmarks=np.zeros((cap, 10), np.float32),
               M=np.zeros((cap, 6), np.float64), flags=np.zeros((cap,), np.int32))
    nf = np.zeros((1,), np.int32)
    tx, ty, bx, by = offsets
    L.check(L.load().fp_dets_to_crops_aligned_emulate(
        _p(dets), _p(counts), B, max_dets, row, int(fmt), int(in_size[0]), int(in_size[1]), _p(descs), _p(geom),
        float(det_thres), float(area_thres), tx, ty, bx, by, SIZE, SIZE, cap, _p(out["items"]), _p(out["info"]), _p(nf),
        _p(out["lmarks"]), _p(out["M"]), _p(out["flags"])), "fp_dets_to_crops_aligned_emulate")
    n = int(nf[0])
    return {k: v[:n] for k, v in out.items()}
