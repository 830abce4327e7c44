"""Tiled ("sliced") detection: find faces that are too small for one letterbox.

Every detector here sees a whole frame through one letterbox: BlazeFace-back takes a 576 x 1024 frame at 256 x 256, a gain of
0.25, so a face 40 px wide reaches the network 10 px wide.  TiledDetector wraps a BlazeFaceModel or YOLOV5FaceModel and runs
it on overlapping tiles of every frame and (full_frame) on the whole frame; each such image is a *view* of its frame.  One
launch of fp_merge_views (csrc/tilemerge.hip) maps every view's rows into the frame's own pixels, drops the boxes a tile
border cut through, removes the duplicates across views and writes one block of fmt-2 rows per frame -- what
fp_dets_to_crops_px, evaluation.dets_to_frame_boxes and annotate take from the MTCNN wrapper, so FacePipeline and the
evaluator take a TiledDetector as they take any detector.

Build-defined: the reference has nothing like it (its users cut frames by hand).  The procedure is written down in
include/facepath.h and DESIGN.md section 7 "Tiled detection"; merge_views_numpy and gather_tiles_numpy restate it in float32
numpy, operation for operation, and are the oracle of the tests.  merge_thr, edge_px, the tile size and the overlap have no
recommended values: no real weights and no annotated data exist offline, so detection accuracy under tiling is unmeasured.
"""
from collections import OrderedDict

import numpy as np
import torch

from . import _lib as L
from .frames import RaggedFrames, as_frames, batch_len, device_descs, frame_bytes, frame_layout, scale_coords_params

PAD_VALUE = 125          # the letterbox pad value: what a tile larger than its frame is filled with
VIEW_DTYPE = np.dtype([("frame", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("vw", "<i4"), ("vh", "<i4"),
                       ("gain", "<f4"), ("pad_x", "<f4"), ("pad_y", "<f4")])      # fp_tile_view, 32 bytes
assert VIEW_DTYPE.itemsize == 32


# ------------------------------------------------------------------------------------------------ the grid

def _axis_starts(size, tile, overlap):
    """Tile starts along one axis: 0, stride, 2 stride, ... while start + tile < size, then the last tile shifted back to
    size - tile (overlap only grows there); a frame no larger than the tile gets the one start 0."""
    if size <= tile:
        return [0]
    stride = tile - overlap
    starts = []
    s = 0
    while s + tile < size:
        starts.append(s)
        s += stride
    starts.append(size - tile)
    return starts


def tile_grid(w, h, tile, overlap):
    """[(x0, y0, vw, vh)] of the tiles of a w x h frame, row-major.  tile = (tw, th), overlap = (ox, oy) with 0 <= ox < tw,
    0 <= oy < th (ValueError otherwise).  vw = min(tw, w), vh = min(th, h): every tile of a frame at least tile-sized has
    the tile's size, a smaller frame gets one tile at 0 that it fills only in part."""
    tw, th = int(tile[0]), int(tile[1])
    ox, oy = int(overlap[0]), int(overlap[1])
    if tw < 1 or th < 1 or not (0 <= ox < tw) or not (0 <= oy < th):
        raise ValueError(f"tile_grid: tile {tile} / overlap {overlap}: need tile >= 1 and 0 <= overlap < tile per axis")
    if w < 1 or h < 1:
        raise ValueError(f"tile_grid: frame {w} x {h}")
    vw, vh = min(tw, w), min(th, h)
    return [(x0, y0, vw, vh) for y0 in _axis_starts(h, th, oy) for x0 in _axis_starts(w, tw, ox)]


def build_views(sizes, tile, overlap, in_size, full_frame=True):
    """The view table of frames of sizes [(h, w)]: per frame its tiles (tile_grid order), then with full_frame the whole
    frame.  -> (views (S,) VIEW_DTYPE, view_start (B + 1,) int32, is_tile (S,) bool).  gain / pad are scale_coords_params of
    the image the detector is given -- the tile's size for a tile, the frame's for the whole frame -- against in_size."""
    tw, th = int(tile[0]), int(tile[1])
    tile_geom = scale_coords_params(in_size, (tw, th))
    rows, start, is_tile = [], [0], []
    for f, (h, w) in enumerate(sizes):
        for x0, y0, vw, vh in tile_grid(w, h, tile, overlap):
            rows.append((f, x0, y0, vw, vh) + tile_geom)
            is_tile.append(True)
        if full_frame:
            rows.append((f, 0, 0, w, h) + scale_coords_params(in_size, (w, h)))
            is_tile.append(False)
        start.append(len(rows))
    return np.array(rows, dtype=VIEW_DTYPE), np.asarray(start, np.int32), np.asarray(is_tile, bool)


# ------------------------------------------------------------------------------------------------ numpy restatements

def gather_tiles_numpy(frames, views, tile):
    """frames: list of (h, w, 3) u8; views: VIEW_DTYPE rows -> (S, th, tw, 3) u8: each view's rectangle at the tile's top
    left, the rest PAD_VALUE (fp_gather_tiles)."""
    tw, th = int(tile[0]), int(tile[1])
    out = np.full((len(views), th, tw, 3), PAD_VALUE, np.uint8)
    for s, v in enumerate(views):
        fr = frames[int(v["frame"])]
        x0, y0 = int(v["x0"]), int(v["y0"])
        cw = max(min(int(v["vw"]), fr.shape[1] - x0, tw), 0)
        ch = max(min(int(v["vh"]), fr.shape[0] - y0, th), 0)
        out[s, :ch, :cw] = fr[y0:y0 + ch, x0:x0 + cw]
    return out


def _f32(x):
    return np.asarray(x, np.float32)


def merge_views_numpy(dets, counts, views, view_start, sizes, in_size, fmt, merge_thr, edge_px, max_out, overflow=None):
    """fp_merge_views in float32 numpy, in the written operation order (include/facepath.h "Tiled detection").
    dets (S, max_dets, row) fp32, counts (S,), views VIEW_DTYPE (S,), view_start (B + 1,), sizes [(h, w)] per frame, in_size
    (w, h) of the detector, fmt 0 / 1.  overflow: (B,) int32 the flags are OR-ed into (default zeros).
    -> (out (B, max_out, 16) fp32, zero behind the counts; counts (B,) int32; overflow (B,) int32)."""
    dets = _f32(dets)
    S, max_dets, _ = dets.shape
    B = len(sizes)
    iw, ih = _f32(in_size[0]), _f32(in_size[1])
    thr, edge = _f32(merge_thr), _f32(edge_px)
    out = np.zeros((B, max_out, 16), np.float32)
    out_counts = np.zeros((B,), np.int32)
    over = np.zeros((B,), np.int32) if overflow is None else np.array(overflow, np.int32)
    old = np.seterr(all="ignore")
    try:
        for f, (H, W) in enumerate(sizes):
            lo = min(max(int(view_start[f]), 0), S)
            hi = min(max(int(view_start[f + 1]), lo), S)
            boxes, scores, rows16, base = [], [], [], 0
            for s in range(lo, hi):
                n = min(max(int(counts[s]), 0), max_dets)
                take = min(n, L.MERGE_CAP - base)
                if n > take:
                    over[f] |= 2
                base += take
                if take <= 0:
                    continue
                v = views[s]
                d = dets[s, :take]
                gain, px, py = _f32(v["gain"]), _f32(v["pad_x"]), _f32(v["pad_y"])
                x0, y0, vw, vh = int(v["x0"]), int(v["y0"]), int(v["vw"]), int(v["vh"])
                if fmt == 0:
                    sc = d[:, 16]
                    x1, y1, x2, y2 = d[:, 1] * iw, d[:, 0] * ih, d[:, 3] * iw, d[:, 2] * ih
                    k = np.array([0, 1, 2, 3, 3])
                    lx, ly = d[:, 4 + 2 * k] * iw, d[:, 5 + 2 * k] * ih
                else:
                    sc = d[:, 4]
                    x1, y1, x2, y2 = d[:, 0], d[:, 1], d[:, 2], d[:, 3]
                    k = np.arange(5)
                    lx, ly = d[:, 5 + 2 * k], d[:, 6 + 2 * k]
                sc = np.where(sc == 0, _f32(0), sc)
                x1, x2, y1, y2 = (x1 - px) / gain, (x2 - px) / gain, (y1 - py) / gain, (y2 - py) / gain
                ok = np.isfinite(x1) & np.isfinite(y1) & np.isfinite(x2) & np.isfinite(y2) & np.isfinite(sc)
                fvw, fvh = _f32(vw), _f32(vh)
                if edge >= 0:
                    if x0 > 0:
                        ok &= ~(x1 <= edge)
                    if x0 + vw < W:
                        ok &= ~(x2 >= fvw - edge)
                    if y0 > 0:
                        ok &= ~(y1 <= edge)
                    if y0 + vh < H:
                        ok &= ~(y2 >= fvh - edge)
                x1, x2 = np.minimum(np.maximum(x1, 0), fvw) + _f32(x0), np.minimum(np.maximum(x2, 0), fvw) + _f32(x0)
                y1, y2 = np.minimum(np.maximum(y1, 0), fvh) + _f32(y0), np.minimum(np.maximum(y2, 0), fvh) + _f32(y0)
                ok &= (x2 > x1) & (y2 > y1)
                row = np.zeros((take, 16), np.float32)
                row[:, 0], row[:, 1], row[:, 2], row[:, 3] = x1, y1, x2, y2
                row[:, 4:14:2] = (lx - px) / gain + _f32(x0)
                row[:, 5:14:2] = (ly - py) / gain + _f32(y0)
                row[:, 14] = sc
                rows16.append(row[ok])
                scores.append(sc[ok])
            if not rows16:
                continue
            rows = np.concatenate(rows16)
            order = np.argsort(-np.concatenate(scores).astype(np.float64), kind="stable")   # candidates are in (view, row) order
            rows = rows[order]
            area = (rows[:, 2] - rows[:, 0]) * (rows[:, 3] - rows[:, 1])
            kept = []
            for i in range(len(rows)):
                if kept:
                    kb, ka = rows[kept], area[kept]
                    iw_ = np.maximum(np.minimum(kb[:, 2], rows[i, 2]) - np.maximum(kb[:, 0], rows[i, 0]), _f32(0))
                    ih_ = np.maximum(np.minimum(kb[:, 3], rows[i, 3]) - np.maximum(kb[:, 1], rows[i, 1]), _f32(0))
                    if np.any(iw_ * ih_ > thr * np.minimum(ka, area[i])):
                        continue
                kept.append(i)
            n_out = min(len(kept), max_out)
            out[f, :n_out] = rows[kept[:n_out]]
            out_counts[f] = n_out
            if len(kept) > max_out:
                over[f] |= 4
    finally:
        np.seterr(**old)
    return out, out_counts, over


# ------------------------------------------------------------------------------------------------ the C entry points

def _descs_host(sizes):
    from .frames import frame_descs
    off = np.concatenate([[0], np.cumsum([h * w * 3 for h, w in sizes])[:-1]]).astype(np.int64)
    return frame_descs(off, sizes)


def merge_views_emulate(dets, counts, views, view_start, sizes, in_size, fmt, merge_thr, edge_px, max_out, overflow=None):
    """fp_merge_views_emulate on host arrays: merge_views_numpy's arguments and results; raises FacepathError on a refusal."""
    lib = L.load()
    dets = np.ascontiguousarray(dets, np.float32)
    counts = np.ascontiguousarray(counts, np.int32)
    views = np.ascontiguousarray(views, VIEW_DTYPE)
    view_start = np.ascontiguousarray(view_start, np.int32)
    descs = _descs_host(sizes)
    B = len(sizes)
    out = np.zeros((B, max_out, 16), np.float32)
    out_counts = np.zeros((B,), np.int32)
    over = np.zeros((B,), np.int32) if overflow is None else np.array(overflow, np.int32)
    p = lambda a: a.ctypes.data          # noqa: E731
    L.check(lib.fp_merge_views_emulate(p(dets), p(counts), dets.shape[0], dets.shape[1], dets.shape[2], int(fmt), int(in_size[0]),
                                       int(in_size[1]), p(views), p(view_start), p(descs), B, float(merge_thr), float(edge_px),
                                       int(max_out), p(out), p(out_counts), p(over)), "fp_merge_views_emulate")
    for f in range(B):
        out[f, out_counts[f]:] = 0
    return out, out_counts, over


def merge_views(dets, counts, views_dev, view_start_dev, descs_dev, B, in_size, fmt, merge_thr, edge_px, max_out, overflow=None):
    """One fp_merge_views launch on the current stream.  dets (S, max_dets, row) fp32 / counts (S,) int32 CUDA tensors in view
    order, views_dev (S, 32) u8, view_start_dev (B + 1,) int32, descs_dev (B, 16) u8.  overflow: (B,) int32 the flags are
    OR-ed into (default zeros).  -> (out (B, max_out, 16), counts (B,), overflow (B,)); rows behind the counts are undefined."""
    lib, dev = L.load(), dets.device
    assert dets.is_contiguous() and dets.dtype == torch.float32 and counts.dtype == torch.int32 and counts.is_contiguous()
    out = torch.empty((B, max_out, 16), dtype=torch.float32, device=dev)
    out_counts = torch.empty((B,), dtype=torch.int32, device=dev)
    over = torch.zeros((B,), dtype=torch.int32, device=dev) if overflow is None else overflow
    L.check(lib.fp_merge_views(L.ptr(dets), L.ptr(counts), dets.shape[0], dets.shape[1], dets.shape[2], int(fmt), int(in_size[0]),
                               int(in_size[1]), L.ptr(views_dev), L.ptr(view_start_dev), L.ptr(descs_dev), int(B), float(merge_thr),
                               float(edge_px), int(max_out), L.ptr(out), L.ptr(out_counts), L.ptr(over), L.current_stream(dev)),
            "fp_merge_views")
    return out, out_counts, over


def gather_tiles(frames, views_dev, n_views, tile):
    """fp_gather_tiles: the rectangles of the first n_views rows of views_dev (device fp_tile_view array) out of a dense
    (B, H, W, 3) batch or a RaggedFrames -> (n_views, th, tw, 3) u8, one launch."""
    lib = L.load()
    tw, th = int(tile[0]), int(tile[1])
    data = frame_bytes(frames)
    out = torch.empty((n_views, th, tw, 3), dtype=torch.uint8, device=data.device)
    L.check(lib.fp_gather_tiles(L.ptr(data), data.numel(), L.ptr(device_descs(frames)), batch_len(frames), L.ptr(views_dev),
                                int(n_views), tw, th, L.ptr(out), L.current_stream(data.device)), "fp_gather_tiles")
    return out


def gather_tiles_torch(frames, views, tile):
    """The same tiles by slicing with torch, one copy per tile (the yardstick of tools/tile_bench.py and of the tests)."""
    tw, th = int(tile[0]), int(tile[1])
    fl = frames.to_list() if isinstance(frames, RaggedFrames) else frames
    out = torch.full((len(views), th, tw, 3), PAD_VALUE, dtype=torch.uint8, device=frames.device)
    for s, v in enumerate(views):
        x0, y0, vw, vh = int(v["x0"]), int(v["y0"]), int(v["vw"]), int(v["vh"])
        out[s, :vh, :vw] = fl[int(v["frame"])][y0:y0 + vh, x0:x0 + vw]
    return out


# ------------------------------------------------------------------------------------------------ the detector

class _ViewTable:
    """The views of one batch shape: host rows and their device copies, with tile views first in the device table used for
    the gather (tile_views_dev) and the positions of tile / whole-frame views in the merge order."""

    def __init__(self, sizes, tile, overlap, in_size, full_frame, dev):
        self.views, self.view_start, is_tile = build_views(sizes, tile, overlap, in_size, full_frame)
        self.n_tiles = int(is_tile.sum())
        to_dev = lambda a: torch.from_numpy(a).to(dev)     # noqa: E731
        self.views_dev = to_dev(self.views.view(np.uint8).reshape(-1, 32))
        self.tile_views = self.views[is_tile]
        self.tile_views_dev = to_dev(np.ascontiguousarray(self.tile_views).view(np.uint8).reshape(-1, 32))
        self.view_start_dev = to_dev(self.view_start)
        self.tile_pos = to_dev(np.nonzero(is_tile)[0].astype(np.int64))
        self.full_pos = to_dev(np.nonzero(~is_tile)[0].astype(np.int64))
        self.view_frame = to_dev(self.views["frame"].astype(np.int64))


class TiledDetector:
    """inner: a BlazeFaceModel or YOLOV5FaceModel (dets_fmt 0 / 1; a dets_fmt 2 detector -- MTCNN, another TiledDetector --
    is refused with ValueError: it has its own pyramid).  tile = (tw, th), overlap = (ox, oy) as tile_grid; merge_thr: the
    intersection-over-smaller-area above which the lower-scored of two boxes goes (NO default: no value has been measured on
    real data; +inf suppresses nothing); edge_px: how close to an interior tile edge a box counts as cut (negative: no cut);
    full_frame: also run inner on the whole frame; max_det: rows per frame of raw_batch.

    The detector interface of FacePipeline and the evaluator: dets_fmt = 2, det_thres / bbox_area_thres / input_size forwarded
    from inner, raw_batch(frames) -> (dets (B, max_det, 16) fp32 fmt-2 rows in each frame's own pixels, counts (B,) int32,
    overflow (B,) int32: bit 1 inner cut a view at its cap, 2 more than FP_MERGE_CAP candidates, 4 more than max_det kept).
    As with the MTCNN wrappers, __call__ sets input_size to the image's (w, h) and returns rows normalised by it; the network
    itself always runs at inner.input_size."""

    accepts_device_frames = True
    returns_opt_labels = False
    dets_fmt = 2
    TABLE_CACHE_SIZE = 8

    def __init__(self, inner, tile, overlap, merge_thr, edge_px=0.0, full_frame=True, max_det=64):
        if getattr(inner, "dets_fmt", None) not in (0, 1):
            raise ValueError(f"TiledDetector wraps a dets_fmt 0 / 1 detector (BlazeFace, YOLOv5-face), got dets_fmt "
                             f"{getattr(inner, 'dets_fmt', None)}: MTCNN has its own pyramid")
        tile_grid(max(int(tile[0]), 1), max(int(tile[1]), 1), tile, overlap)      # ValueError on a bad tile / overlap
        if merge_thr != merge_thr:
            raise ValueError("merge_thr is NaN")
        if not 1 <= int(max_det) <= L.MERGE_CAP:
            raise ValueError(f"max_det must be 1 .. {L.MERGE_CAP}")
        self.inner = inner
        self.tile, self.overlap = (int(tile[0]), int(tile[1])), (int(overlap[0]), int(overlap[1]))
        self.merge_thr, self.edge_px, self.full_frame, self.max_det = float(merge_thr), float(edge_px), bool(full_frame), int(max_det)
        self.input_size = tuple(inner.input_size)
        self._tables = OrderedDict()

    net = property(lambda self: self.inner.net)
    det_thres = property(lambda self: self.inner.det_thres)
    bbox_area_thres = property(lambda self: self.inner.bbox_area_thres)

    def _device(self):
        return self.inner.net._device()

    def view_table(self, frames):
        """The _ViewTable of a batch: on a RaggedFrames through .cached, for a dense batch from a small cache keyed by its shape."""
        key = ("tiled", self.tile, self.overlap, self.full_frame, tuple(self.inner.input_size))
        dev = frames.device

        def make(sizes):
            return _ViewTable(sizes, self.tile, self.overlap, self.inner.input_size, self.full_frame, dev)
        if isinstance(frames, RaggedFrames):
            return frames.cached(key, lambda: make(frames.sizes))
        B, H, W, _ = frames.shape
        key = key + (B, H, W, dev)
        t = self._tables.get(key)
        if t is None:
            t = self._tables[key] = make([(H, W)] * B)
            if len(self._tables) > self.TABLE_CACHE_SIZE:
                self._tables.popitem(last=False)
        return t

    def _inner_raw(self, images, max_det):
        if max_det is None and self.inner.dets_fmt == 1:
            out = self.inner.raw_batch(images, max_det=None)
        else:
            out = self.inner.raw_batch(images)
        return out if len(out) == 3 else (out[0], out[1], None)

    def raw_batch(self, frames, max_det=-1):
        """frames: (B, H, W, 3) u8 BGR (numpy / CUDA tensor) or a RaggedFrames.  max_det: -1 = this wrapper's cap; None =
        uncapped (FacePipeline's re-run after an overflow): inner without its cap, FP_MERGE_CAP rows per frame."""
        frames = as_frames(frames, self._device())
        B, dev = batch_len(frames), frames.device
        t = self.view_table(frames)
        parts = []
        if t.n_tiles:
            tiles = gather_tiles(frames, t.tile_views_dev, t.n_tiles, self.tile)
            parts.append((t.tile_pos,) + self._inner_raw(tiles, max_det))
        if self.full_frame:
            parts.append((t.full_pos,) + self._inner_raw(frames, max_det))
        if len(parts) == 1:                       # one kind of view: inner's rows are in view order as they are
            _, dets, counts, over_v = parts[0]
        else:
            (_, d0, _, _), (_, d1, _, _) = parts
            if d0.shape[1:] != d1.shape[1:]:
                raise L.FacepathError(f"inner detector rows differ between tiles {tuple(d0.shape)} and frames {tuple(d1.shape)}")
            S = len(t.views)
            dets = torch.empty((S,) + tuple(d0.shape[1:]), dtype=torch.float32, device=dev)
            counts = torch.empty((S,), dtype=torch.int32, device=dev)
            over_v = None if all(p[3] is None for p in parts) else torch.zeros((S,), dtype=torch.int32, device=dev)
            for pos, d, c, o in parts:
                dets.index_copy_(0, pos, d)
                counts.index_copy_(0, pos, c.to(torch.int32))
                if o is not None:
                    over_v.index_copy_(0, pos, o.to(torch.int32))
        over = None
        if over_v is not None:                    # a frame is flagged when inner cut any of its views
            hit = torch.zeros((B,), dtype=torch.int32, device=dev).index_add_(0, t.view_frame, (over_v != 0).to(torch.int32))
            over = (hit > 0).to(torch.int32)
        cap = L.MERGE_CAP if max_det is None else (self.max_det if max_det == -1 else int(max_det))
        return merge_views(dets.contiguous(), counts.to(torch.int32).contiguous(), t.views_dev, t.view_start_dev,
                           device_descs(frames), B, self.inner.input_size, self.inner.dets_fmt, self.merge_thr, self.edge_px,
                           cap, over)

    def predict_batch(self, frames):
        """Per frame an (n, 15) array [xmin, ymin, xmax, ymax, (x, y) x 5, conf] normalised by that frame's (w, h)."""
        frames = as_frames(frames, self._device())
        dets, counts, _ = self.raw_batch(frames)
        dets, counts = dets.cpu().numpy(), counts.cpu().numpy()
        out = []
        for i, (_, h, w) in enumerate(frame_layout(frames)):
            rows = dets[i, :counts[i], :15].astype(np.float32)
            rows[:, :14] /= np.asarray([w, h] * 7, np.float32)
            out.append(rows)
        return out

    def __call__(self, cv2_img) -> np.ndarray:
        self.input_size = tuple(int(v) for v in cv2_img.shape[:2][::-1])
        return self.predict_batch(cv2_img[None])[0]


# ------------------------------------------------------------------------------------------------ command-line options

def add_tile_args(parser):
    """--tile / --overlap / --merge_thr / --edge_px / --no_full_frame of the detector entry points.  Every default is
    argparse.SUPPRESS: without the flags the parsed namespace is what it was before they existed."""
    import argparse
    S = argparse.SUPPRESS
    parser.add_argument("--tile", nargs=2, type=int, default=S, metavar=("W", "H"),
                        help="Tiled detection: run the detector on overlapping W x H tiles of every frame (and on the whole frame) "
                             "and merge the detections on the device.  Needs --merge_thr.  (default: off)")
    parser.add_argument("--overlap", nargs=2, type=int, default=S, metavar=("OX", "OY"),
                        help="With --tile: pixels neighbouring tiles share per axis (default: 0 0; no value is recommended yet).")
    parser.add_argument("--merge_thr", type=float, default=S, metavar="T",
                        help="With --tile: drop the lower-scored of two boxes whose intersection exceeds T times the smaller box's "
                             "area.  No default: nothing has been measured on real data.")
    parser.add_argument("--edge_px", type=float, default=S, metavar="E",
                        help="With --tile: drop a box that reaches within E pixels of a tile edge inside the frame (default: 0).")
    parser.add_argument("--no_full_frame", action="store_true", default=S,
                        help="With --tile: do not also run the detector on the whole frame.")
    return parser


def wrap_from_args(det, args, error=None):
    """det itself without --tile, else TiledDetector(det, ...) from the add_tile_args options.  error: parser.error."""
    if getattr(args, "tile", None) is None:
        return det
    if getattr(args, "merge_thr", None) is None:
        msg = "--tile needs --merge_thr (no default: no value has been measured on real data)"
        if error is not None:
            error(msg)
        raise ValueError(msg)
    return TiledDetector(det, tuple(args.tile), tuple(getattr(args, "overlap", (0, 0))), args.merge_thr,
                         edge_px=getattr(args, "edge_px", 0.0), full_frame=not getattr(args, "no_full_frame", False))
