"""Face crop quality on the device: sharpness, exposure and pose per face, a gate and a best-shot pick (build-defined; DESIGN §7
"Face quality").

The reference's only "is this face usable" signal is the detector's confidence (clean_imdb_wiki's bad_quality test).  Here every
face rectangle -- an fp_resize_item row, the rows the embedder's resize consumes -- is measured at native resolution by
fp_face_quality (csrc/quality.hip): integer luma statistics and the sums of a Laplacian over a block-mean image (definitions:
include/facepath.h "Face crop quality"), and, with the five landmarks of an aligned step, a pose record by fp_face_pose.  Python
derives the readable columns in fp64 from the integers.  None of this is pinned against OpenCV: cv2.Laplacian(...).var() mirrors
the image border, this definition uses interior samples only.

    q = face_quality(frames, items, n, lmarks=al["lmarks"], fmt=det.dets_fmt)     # dict of device tensors, no host sync
    keep = QualityGate(min_side=40, min_sharpness=50.0, max_abs_yaw=0.5).mask(q)  # (n,) bool; thresholds are the caller's
    best = best_per_group(q["sharpness"], labels, n_clusters, mask=keep)          # (n_clusters,) int32 rows, -1 = none

`sharpness` is the variance of the Laplacian of the block-mean image, which is 56 .. 112 samples across for every face above
112 px: it is comparable between face sizes within one decimation step s and JUMPS where s changes (112 -> 113 px, 224 -> 225,
...), because the block means are then taken over more pixels.  The gate ships without default thresholds: good values depend on
the data and none has been measured here.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .frames import batch_len, device_descs, frame_bytes, frame_descs

SIDE = 112                  # most blocks a side of the block-mean image
STAT_FIELDS = ("n_px", "sum_y", "sum_y2", "n_dark", "n_bright", "n_lap", "sum_lap", "sum_lap2")
DERIVED = ("mean", "contrast", "dark_frac", "bright_frac", "sharpness", "side")
POSE_FIELDS = ("iod", "roll", "yaw", "pitch")
DARK_MAX, BRIGHT_MIN = 16, 239
EMPTY, BAD_FRAME, NO_LAPLACIAN, TOO_LARGE, POSE_DEGENERATE = (L.QUALITY_EMPTY, L.QUALITY_BAD_FRAME, L.QUALITY_NO_LAPLACIAN,
                                                              L.QUALITY_TOO_LARGE, L.QUALITY_POSE_DEGENERATE)
UNUSABLE = EMPTY | BAD_FRAME | TOO_LARGE     # a face with one of these fails every gate


# ------------------------------------------------------------------------------------------------ the device entry points

def quality_stats(frames, items, n, stats=None, flags=None):
    """fp_face_quality on the first n rows of items ((>= n, 9) int32 device fp_resize_item rows whose src_image indexes
    `frames`, a (B, H, W, 3) u8 device tensor or a RaggedFrames) -> (stats (n, 8) int64, flags (n,) int32).  One launch on the
    current stream, no host sync.  stats / flags: buffers of the caller's to write rows 0 .. n - 1 of."""
    dev = items.device
    n = int(n)
    assert items.dtype == torch.int32 and items.is_contiguous() and items.shape[0] >= n and items.shape[1] == 9
    stats = torch.empty((n, 8), dtype=torch.int64, device=dev) if stats is None else stats
    flags = torch.empty((n,), dtype=torch.int32, device=dev) if flags is None else flags
    assert stats.dtype == torch.int64 and stats.is_contiguous() and stats.numel() >= 8 * n
    assert flags.dtype == torch.int32 and flags.is_contiguous() and flags.numel() >= n
    if n == 0:                     # (an empty tensor has no pointer to pass)
        return stats, flags
    data = frame_bytes(frames)
    L.check(L.load().fp_face_quality(L.ptr(data), data.numel(), L.ptr(device_descs(frames)), batch_len(frames), L.ptr(items), n,
                                     L.ptr(stats), L.ptr(flags), L.current_stream(dev)), "fp_face_quality")
    return stats, flags


def face_pose(lmarks, fmt, n, flags, out=None):
    """fp_face_pose on the first n rows of lmarks ((>= n, 10) fp32 device, the layout align.alloc's lmarks holds; fmt the
    detector's dets_fmt) -> (n, 4) fp32 iod, roll, yaw, pitch; POSE_DEGENERATE is OR-ed into flags[:n]."""
    n = int(n)
    assert lmarks.dtype == torch.float32 and lmarks.is_contiguous() and lmarks.shape[0] >= n and lmarks.shape[1] == 10
    out = torch.empty((n, 4), dtype=torch.float32, device=lmarks.device) if out is None else out
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= 4 * n
    if n == 0:
        return out
    L.check(L.load().fp_face_pose(L.ptr(lmarks), int(fmt), n, L.ptr(out), L.ptr(flags), L.current_stream(lmarks.device)),
            "fp_face_pose")
    return out


def _frame_hw(frames, src):
    """(h, w) int64 device tensors of the frames the rows' src_image name (0 for an index outside the batch)."""
    d = device_descs(frames).view(torch.int32).view(-1, 4)            # off lo, off hi, h, w
    ok = (src >= 0) & (src < d.shape[0])
    row = d[src.clamp(0, d.shape[0] - 1).long()]
    zero = torch.zeros_like(src, dtype=torch.int64)
    return torch.where(ok, row[:, 2].long(), zero), torch.where(ok, row[:, 3].long(), zero)


def _derive(xp, stats, flags, items, fh, fw):
    """The fp64 columns and the decimation step from the integers; xp = torch or numpy (the same expressions).  items (n, 9),
    fh / fw the rows' frame sizes (int64).  A quotient whose denominator is 0 is NaN."""
    it = items.long() if xp is torch else items.astype(np.int64)
    sx, sy, sw, sh = it[:, 1], it[:, 2], it[:, 3], it[:, 4]
    zero = sx * 0
    cw = xp.minimum(sx + sw, fw) - xp.maximum(sx, zero)
    ch = xp.minimum(sy + sh, fh) - xp.maximum(sy, zero)
    cw, ch = xp.maximum(cw, zero), xp.maximum(ch, zero)
    f = flags.long() if xp is torch else flags.astype(np.int64)
    dead = (f & UNUSABLE) != 0
    side = xp.where(dead, zero, xp.minimum(cw, ch))
    step = xp.where(dead, zero, (xp.maximum(cw, ch) + SIDE - 1) // SIDE)
    st = stats.double() if xp is torch else stats.astype(np.float64)
    nan = st[:, 0] * 0 + float("nan")

    def div(a, b):
        return xp.where(b > 0, a / xp.where(b > 0, b, b + 1), nan)
    n_px, n_lap = st[:, 0], st[:, 5]
    mean = div(st[:, 1], n_px)
    var = div(st[:, 2], n_px) - mean * mean
    lap_mean = div(st[:, 6], n_lap)
    s4 = (step * step * step * step).double() if xp is torch else (step ** 4).astype(np.float64)
    out = dict(step=step.int() if xp is torch else step.astype(np.int32), mean=mean,
               contrast=xp.sqrt(xp.where(var > 0, var, var * 0)),      # NaN stays NaN; a rounding below 0 is 0
               dark_frac=div(st[:, 3], n_px), bright_frac=div(st[:, 4], n_px),
               sharpness=div(div(st[:, 7], n_lap) - lap_mean * lap_mean, s4),
               side=side.double() if xp is torch else side.astype(np.float64))
    return out


def face_quality(frames, items, n, lmarks=None, fmt=None):
    """Quality of the first n face rectangles of items in `frames` -> dict of device tensors, rows in the order of items:
    stats (n, 8) int64 (STAT_FIELDS), flags (n,) int32 (EMPTY | BAD_FRAME | NO_LAPLACIAN | TOO_LARGE | POSE_DEGENERATE), step
    (n,) int32 (the decimation step s; 0 for an unusable face) and, fp64 (n,): mean, contrast, dark_frac, bright_frac,
    sharpness (NaN where their denominator is 0) and side = min(sw, sh) of the clamped rectangle.  With lmarks ((>= n, 10)
    fp32 device) and fmt (the detector's dets_fmt): iod, roll, yaw, pitch, fp32 (n,), 0 for a degenerate landmark set.
    Two launches at most, no host sync."""
    n = int(n)
    stats, flags = quality_stats(frames, items, n)
    pose = None
    if lmarks is not None:
        if fmt is None:
            raise ValueError("face_quality: lmarks need the detector's fmt")
        pose = face_pose(lmarks, fmt, n, flags)
    fh, fw = _frame_hw(frames, items[:n, 0])
    q = dict(stats=stats, flags=flags)
    q.update(_derive(torch, stats, flags, items[:n], fh, fw))
    if pose is not None:
        q.update({k: pose[:, i] for i, k in enumerate(POSE_FIELDS)})
    return q


# ------------------------------------------------------------------------------------------------ the library's host twins

def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _host_batch(frames_list):
    sizes = [f.shape[:2] for f in frames_list]
    offs = np.cumsum([0] + [3 * h * w for h, w in sizes])
    buf = np.concatenate([np.ascontiguousarray(f, np.uint8).reshape(-1) for f in frames_list] + [np.zeros(1, np.uint8)])
    return buf, int(offs[-1]), frame_descs(offs[:-1], sizes), sizes


def _host_hw(sizes, src):
    hw = np.array(list(sizes) + [(0, 0)], np.int64).reshape(-1, 2)
    idx = np.where((src >= 0) & (src < len(sizes)), src, len(sizes))
    return hw[idx, 0], hw[idx, 1]


def face_quality_emulate(frames_list, items, n=None, lmarks=None, fmt=None):
    """face_quality by the library's host twins (fp_face_quality_emulate, fp_face_pose_emulate: the kernels' own code run
    serially, no GPU needed) on host frames (a list of (h, w, 3) u8 numpy arrays) and host items (n, 9) int32 -> the same dict,
    of numpy arrays."""
    items = np.ascontiguousarray(items, np.int32).reshape(-1, 9)
    n = len(items) if n is None else int(n)
    buf, total, descs, sizes = _host_batch(frames_list)
    stats, flags = np.zeros((n, 8), np.int64), np.zeros((n,), np.int32)
    lib = L.load()
    L.check(lib.fp_face_quality_emulate(_p(buf), total, _p(descs), len(sizes), _p(items), n, _p(stats), _p(flags)),
            "fp_face_quality_emulate")
    q = dict(stats=stats, flags=flags)
    if lmarks is not None:
        lm = np.ascontiguousarray(lmarks, np.float32).reshape(-1, 10)
        pose = np.zeros((n, 4), np.float32)
        L.check(lib.fp_face_pose_emulate(_p(lm), int(fmt), n, _p(pose), _p(flags)), "fp_face_pose_emulate")
        q.update({k: pose[:, i].copy() for i, k in enumerate(POSE_FIELDS)})
    with np.errstate(all="ignore"):
        q.update(_derive(np, stats, flags, items[:n], *_host_hw(sizes, items[:n, 0])))
    return q


# ------------------------------------------------------------------------------------------------ the numpy restatement

def luma_numpy(img):
    """(h, w) int64 luma of an (h, w, 3) u8 BGR image."""
    p = img.astype(np.int64)
    return (1868 * p[..., 0] + 9617 * p[..., 1] + 4899 * p[..., 2] + 8192) >> 14


def _numpy_face(frames_list, row):
    """(stats (8,), flags) of one item row, by the definitions of include/facepath.h: whole-array numpy, no library code."""
    src, sx, sy, sw, sh = (int(v) for v in row[:5])
    zero = np.zeros(8, np.int64)
    if not 0 <= src < len(frames_list):
        return zero, BAD_FRAME
    img = frames_list[src]
    h, w = img.shape[:2]
    if not (L.FRAME_MIN_W <= w <= L.FRAME_MAX_W and 1 <= h <= L.FRAME_MAX_H):
        return zero, BAD_FRAME
    x0, y0, x1, y1 = max(sx, 0), max(sy, 0), min(sx + sw, w), min(sy + sh, h)
    if sw <= 0 or sh <= 0 or x0 >= x1 or y0 >= y1:
        return zero, EMPTY
    cw, ch = x1 - x0, y1 - y0
    s = max(1, -(-max(cw, ch) // SIDE))
    if s > L.QUALITY_MAX_STEP:
        return zero, TOO_LARGE
    bw, bh = cw // s, ch // s
    flags = NO_LAPLACIAN if bw < 3 or bh < 3 else 0
    if bw == 0 or bh == 0:
        return zero, flags
    y = luma_numpy(img[y0:y0 + bh * s, x0:x0 + bw * s])
    st = zero.copy()
    st[:5] = y.size, y.sum(), (y * y).sum(), (y <= DARK_MAX).sum(), (y >= BRIGHT_MIN).sum()
    if not flags:
        bk = y.reshape(bh, s, bw, s).sum(axis=(1, 3))
        lap = bk[:-2, 1:-1] + bk[2:, 1:-1] + bk[1:-1, :-2] + bk[1:-1, 2:] - 4 * bk[1:-1, 1:-1]
        st[5:] = lap.size, lap.sum(), (lap * lap).sum()
    return st, flags


def pose_numpy(lmarks, fmt):
    """((n, 4) fp64 iod, roll, yaw, pitch, (n,) int32 POSE_DEGENERATE or 0) of (n, 10) landmarks, in fp64."""
    lm = np.asarray(lmarks, np.float32).reshape(-1, 10).astype(np.float64)
    le, re, nose = lm[:, 0:2], lm[:, 2:4], lm[:, 4:6]
    mouth = lm[:, 6:8] if int(fmt) == 0 else (lm[:, 6:8] + lm[:, 8:10]) / 2
    e = re - le
    iod = np.hypot(e[:, 0], e[:, 1])
    mid = (le + re) / 2
    v = np.stack([-e[:, 1], e[:, 0]], 1)
    den = ((mouth - mid) * v).sum(1)
    bad = ~(iod >= 1) | ~(den > 0)
    with np.errstate(all="ignore"):
        out = np.stack([iod, e[:, 1] / iod, 2 * ((nose - le) * e).sum(1) / (iod * iod) - 1, ((nose - mid) * v).sum(1) / den], 1)
    out[bad] = 0
    return out, np.where(bad, POSE_DEGENERATE, 0).astype(np.int32)


def face_quality_numpy(frames_list, items, n=None, lmarks=None, fmt=None):
    """The restatement the tests compare the kernel and its host twin against: reshape and sum for the blocks, slicing for the
    Laplacian, fp64 for the pose.  Host frames and items as face_quality_emulate; the same dict of numpy arrays (pose fp64)."""
    items = np.asarray(items, np.int32).reshape(-1, 9)
    n = len(items) if n is None else int(n)
    rows = [_numpy_face(frames_list, items[i]) for i in range(n)]
    stats = np.array([r[0] for r in rows], np.int64).reshape(n, 8)
    flags = np.array([r[1] for r in rows], np.int32).reshape(n)
    q = dict(stats=stats, flags=flags)
    if lmarks is not None:
        pose, pf = pose_numpy(np.asarray(lmarks)[:n], fmt)
        flags |= pf
        q.update({k: pose[:, i].copy() for i, k in enumerate(POSE_FIELDS)})
    sizes = [f.shape[:2] for f in frames_list]
    with np.errstate(all="ignore"):
        q.update(_derive(np, stats, flags, items[:n], *_host_hw(sizes, items[:n, 0])))
    return q


# ------------------------------------------------------------------------------------------------ gate and best shot

class QualityGate:
    """Thresholds over a face_quality dict; every one is off (None) by default and NO defaults ship: good values depend on the
    data and none has been measured here.  min_*: the column must be >= the value; max_*: <= it; max_abs_yaw / max_abs_roll:
    |column| <= it; pitch_range: (lo, hi), lo <= pitch <= hi.  A face flagged EMPTY, BAD_FRAME or TOO_LARGE, or with no pixel
    counted, fails every gate (one without thresholds too); NO_LAPLACIAN fails a gate with min_sharpness; POSE_DEGENERATE fails
    a gate with a pose term.  A gate with a pose term needs a dict with the pose columns (ValueError)."""

    TERMS = ("min_side", "min_sharpness", "min_contrast", "max_dark_frac", "max_bright_frac", "max_abs_yaw", "max_abs_roll",
             "pitch_range")

    def __init__(self, min_side=None, min_sharpness=None, min_contrast=None, max_dark_frac=None, max_bright_frac=None,
                 max_abs_yaw=None, max_abs_roll=None, pitch_range=None):
        self.min_side, self.min_sharpness, self.min_contrast = min_side, min_sharpness, min_contrast
        self.max_dark_frac, self.max_bright_frac = max_dark_frac, max_bright_frac
        self.max_abs_yaw, self.max_abs_roll = max_abs_yaw, max_abs_roll
        if pitch_range is not None:
            lo, hi = pitch_range
            pitch_range = (float(lo), float(hi))
        self.pitch_range = pitch_range

    @property
    def uses_pose(self):
        return self.max_abs_yaw is not None or self.max_abs_roll is not None or self.pitch_range is not None

    def __repr__(self):
        on = ", ".join(f"{k}={getattr(self, k)!r}" for k in self.TERMS if getattr(self, k) is not None)
        return f"QualityGate({on})"

    def mask(self, q):
        """(n,) bool tensor (on the dict's device; a dict of numpy arrays gives a CPU tensor): the faces that pass.  A NaN
        column value fails its term."""
        t = {k: torch.as_tensor(v) for k, v in q.items()}
        flags = t["flags"]
        ok = ((flags & UNUSABLE) == 0) & (t["stats"][:, 0] > 0)
        if self.min_side is not None:
            ok = ok & (t["side"] >= self.min_side)
        if self.min_sharpness is not None:
            ok = ok & ((flags & NO_LAPLACIAN) == 0) & (t["sharpness"] >= self.min_sharpness)
        if self.min_contrast is not None:
            ok = ok & (t["contrast"] >= self.min_contrast)
        if self.max_dark_frac is not None:
            ok = ok & (t["dark_frac"] <= self.max_dark_frac)
        if self.max_bright_frac is not None:
            ok = ok & (t["bright_frac"] <= self.max_bright_frac)
        if self.uses_pose:
            if "yaw" not in t:
                raise ValueError("QualityGate: a pose threshold needs face_quality(..., lmarks=, fmt=)")
            ok = ok & ((flags & POSE_DEGENERATE) == 0)
            if self.max_abs_yaw is not None:
                ok = ok & (t["yaw"].abs() <= self.max_abs_yaw)
            if self.max_abs_roll is not None:
                ok = ok & (t["roll"].abs() <= self.max_abs_roll)
            if self.pitch_range is not None:
                ok = ok & (t["pitch"] >= self.pitch_range[0]) & (t["pitch"] <= self.pitch_range[1])
        return ok


def best_per_group(score, groups, n_groups, mask=None):
    """(n_groups,) int32: per group the row with the highest score, the lower row on ties; -1 for a group with no row or none
    passing `mask`.  score (n,) float, groups (n,) integer labels; rows with groups < 0 (or >= n_groups), with a NaN score or
    with mask False are ignored.  Runs on score's device without a host sync; deterministic (two stable sorts and the
    segment heads)."""
    score, groups = torch.as_tensor(score), torch.as_tensor(groups)
    dev, n, n_groups = score.device, score.shape[0], int(n_groups)
    groups = groups.to(dev).long()
    ok = (groups >= 0) & (groups < n_groups) & ~torch.isnan(score)
    if mask is not None:
        ok = ok & torch.as_tensor(mask).to(dev).bool()
    out = torch.full((n_groups + 1,), -1, dtype=torch.int32, device=dev)
    if n == 0:
        return out[:n_groups]
    g = torch.where(ok, groups, torch.full_like(groups, n_groups))
    by_score = torch.sort(score, descending=True, stable=True).indices       # ties: the lower row first
    rows = by_score[torch.sort(g[by_score], stable=True).indices]            # grouped, the order within a group kept
    gs = g[rows]
    head = torch.ones_like(gs, dtype=torch.bool)
    head[1:] = gs[1:] != gs[:-1]
    out[gs[head]] = rows[head].int()
    out[n_groups] = -1
    return out[:n_groups]
