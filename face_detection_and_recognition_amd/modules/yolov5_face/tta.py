"""Augmented inference of YOLOv5-face (y5/models/yolo.py:156-175; scale_img, y5/utils/torch_utils.py:230-240): the view
geometry on the host, the numpy restatements of csrc/tta.hip's two kernels, and their device wrappers.

The reference runs the network on the input, on the input mirrored left-right and scaled by 0.83, and on the input scaled
by 0.67, maps the box columns of every run back to the input's pixels and hands the concatenated rows to one
non_max_suppression_face.  It does NOT map the landmark columns back: the landmarks of a row of view 2 or 3 stay in that
view's own pixels, unmirrored (a defect of the reference).  ``landmarks="reference"`` reproduces that; ``"mapped"`` maps
them like the boxes, so that columns 5..14 mean the same in every row."""
import math

import numpy as np

from ... import _lib as L

TTA_RATIOS = (1.0, 0.83, 0.67)      # yolo.py:159
TTA_FLIPS = (False, True, False)    # yolo.py:160 (3 = left-right)
TTA_PAD = 0.447                     # torch_utils.py:240
LM_MODES = {"reference": 0, "mapped": 1}
STRIDES = (8, 16, 32)


def tta_views(h, w, gs=32):
    """Per view (ratio, flip, (content_h, content_w), (padded_h, padded_w)), scale_img's host arithmetic in Python doubles."""
    views = []
    for r, f in zip(TTA_RATIOS, TTA_FLIPS):
        if r == 1.0:
            content = padded = (int(h), int(w))
        else:
            content = (int(h * r), int(w * r))
            padded = tuple(math.ceil(x * r / gs) * gs for x in (h, w))
        views.append((r, f, content, padded))
    return views


def view_rows(hw, na=3):
    """Decoded rows of a network input of hw = (h, w): na per cell of the three levels."""
    return sum(na * (hw[0] // s) * (hw[1] // s) for s in STRIDES)


def tta_rows(h, w):
    """Decoded rows of the three views, in order."""
    return [view_rows(v[3]) for v in tta_views(h, w)]


def tta_view_of_rows(keep_idx, h, w):
    """View id (0 / 1 / 2) of every row index into the concatenated z (NMS's keep_idx); numpy in, numpy out, a tensor in, a
    tensor out.  Indices outside the rows (the unused tail of keep_idx) give whatever bucket they fall in."""
    edges = np.cumsum(tta_rows(h, w))[:2]
    if isinstance(keep_idx, np.ndarray) or not hasattr(keep_idx, "device"):
        return np.searchsorted(edges, np.asarray(keep_idx), side="right").astype(np.int64)
    import torch
    return torch.bucketize(keep_idx.long(), torch.as_tensor(edges, device=keep_idx.device), right=True)


# ------------------------------------------------------------------------------------------------- numpy restatements

def _taps(n_in, n_out):
    """upsample_bilinear2d's source taps for align_corners = False, fp32 as the kernel: (i0, i1, weight of i1).  The source
    coordinate is ONE fma, as torch's CPU build and the kernel compute it: the fp64 product of two fp32 numbers and the
    difference are exact here (35 bits), so the cast is the fma's single rounding."""
    scale = np.float32(n_in) / np.float32(n_out)
    d = np.arange(n_out, dtype=np.float32)
    src = (np.float64(scale) * (d + np.float32(0.5)).astype(np.float64) - 0.5).astype(np.float32)
    src = np.maximum(src, np.float32(0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, src - i0.astype(np.float32)


def tta_views_numpy(canvas, pad_value=TTA_PAD):
    """canvas (N, H, W, C) fp32, C = 3 or 4 -> [view 2, view 3] as (N, padded_h, padded_w, C): tta_views_kernel in numpy, same
    order of operations (with C = 4 channel 3 is zero everywhere)."""
    canvas = np.ascontiguousarray(canvas, np.float32)
    N, H, W, C = canvas.shape
    out = []
    for _, flip, (ch, cw), (ph, pw) in tta_views(H, W)[1:]:
        y0, y1, ly = _taps(H, ch)
        x0, x1, lx = _taps(W, cw)
        if flip:
            x0, x1 = W - 1 - x0, W - 1 - x1
        lx, ly = lx[None, None, :, None], ly[None, :, None, None]
        hx, hy = np.float32(1) - lx, np.float32(1) - ly
        top = canvas[:, y0][:, :, x0] * hx + canvas[:, y0][:, :, x1] * lx
        bot = canvas[:, y1][:, :, x0] * hx + canvas[:, y1][:, :, x1] * lx
        v = np.full((N, ph, pw, C), np.float32(pad_value), np.float32)
        v[:, :ch, :cw] = top * hy + bot * ly
        if C == 4:
            v[..., 3] = 0
        out.append(v)
    return out


def unmap_rows_numpy(rows, si, flip, img_w, lm_mode):
    """Decoded rows (..., 16) fp32 of a view -> the rows yolo_decode_view_kernel writes: columns 0..3 / si, cx mirrored, and
    for lm_mode 1 ("mapped") the landmarks divided, mirrored and their left / right points exchanged."""
    q = np.array(rows, np.float32, copy=True)
    si, wf = np.float32(si), np.float32(img_w)
    q[..., :4] = q[..., :4] / si
    if flip:
        q[..., 0] = wf - q[..., 0]
    if LM_MODES.get(lm_mode, lm_mode) == 1:
        q[..., 5:15] = q[..., 5:15] / si
        if flip:
            q[..., 5:15:2] = wf - q[..., 5:15:2]
            q[..., [5, 6, 7, 8, 11, 12, 13, 14]] = q[..., [7, 8, 5, 6, 13, 14, 11, 12]]
    return q


# ------------------------------------------------------------------------------------------------------ device wrappers

def fill_views(canvas, out_a, out_b, pad_value=TTA_PAD):
    """fp_tta_views: canvas (N, H, W, 4) fp32 -> the inputs of views 2 and 3, (N, padded_h, padded_w, 4) each, on the current
    stream."""
    import torch
    N, H, W, C = canvas.shape
    views = tta_views(H, W)[1:]
    for t, v in zip((out_a, out_b), views):
        assert t.shape == (N,) + v[3] + (4,) and t.is_contiguous() and t.dtype == torch.float32, (tuple(t.shape), v)
    assert C == 4 and canvas.is_contiguous() and canvas.dtype == torch.float32
    descs = (L.FpTtaView * 2)(*[L.FpTtaView(v[2][0], v[2][1], v[3][0], v[3][1], int(v[1]), 0) for v in views])
    L.check(L.load().fp_tta_views(L.ptr(canvas), N, H, W, descs, L.ptr(out_a), L.ptr(out_b), float(pad_value),
                                  L.current_stream(canvas.device)), "fp_tta_views")


def decode_view(det, heads, z, row0, si, flip, img_w, lm_mode):
    """fp_yolo_decode_view over the three head tensors (N, ny, nx, na * 16) of one view into z (N, rows, 16) from row row0 on;
    returns the row behind the view's last."""
    lib = L.load()
    ag = det.anchor_grid.view(det.nl, det.na, 2).cpu().numpy()
    row = row0
    for lvl, h in enumerate(heads):
        N, ny, nx, _ = h.shape
        anc = (L.C.c_float * 6)(*[float(v) for v in ag[lvl].reshape(-1)])
        L.check(lib.fp_yolo_decode_view(L.ptr(h), N, ny, nx, det.na, float(det.stride[lvl]), anc, L.ptr(z), z.shape[1] * 16, row,
                                        float(si), int(flip), int(img_w), LM_MODES.get(lm_mode, lm_mode),
                                        L.current_stream(z.device)), "fp_yolo_decode_view")
        row += det.na * ny * nx
    return row
