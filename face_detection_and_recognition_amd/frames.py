"""Batches of frames, dense and ragged, and everything that depends on which of the two a batch is.

Every batched entry point of the path takes one (B, H, W, 3) tensor, so all frames of a batch share a size.  The
reference's dataset driver reads folders of photos of any size (fde/face_extraction/extract_faces_from_dataset.py:380-405).
A RaggedFrames holds such a batch the way the ragged kernels read it (include/facepath.h section 2, ABI 14): the u8 BGR
frames packed back to back, one fp_frame_desc (byte offset of pixel (0, 0), h, w) per frame on the device, and the sizes
on the host.  BlazeFaceModel / YOLOV5FaceModel.raw_batch, FacePipeline and the dataset driver accept it wherever they
accept a (B, H, W, 3) tensor.

This module alone knows how the two kinds differ: as_frames makes either from what a caller has, batch_len / frame_layout /
device_descs describe either, and resize_items, dets_to_crops and frame_call_args pick the C entry point of its kind (a dense
batch never goes through a *_ragged form).  The one fork outside is the detectors' choice of plan
(modules/utils/image.py letterbox_plan).
"""
from collections import OrderedDict

import numpy as np
import torch

from . import _lib as L


class RaggedFrames:
    """data: (total_bytes,) u8 CUDA tensor; sizes: host list of (h, w); offsets: host list of byte offsets;
    descs: (B, 16) u8 CUDA tensor, the fp_frame_desc array."""

    def __init__(self, data, sizes, offsets, descs):
        self.data = data
        self.sizes = [(int(h), int(w)) for h, w in sizes]
        self.offsets = [int(o) for o in offsets]
        self.descs = descs
        self._cache = {}

    @classmethod
    def from_list(cls, frames, device):
        """frames: a non-empty list of (h, w, 3) uint8 tensors (any device) or numpy arrays -> one packed batch on `device`
        (one copy per frame).  Raises ValueError on an empty list, a dtype other than uint8, a shape other than (h, w, 3)
        and a size the ragged kernels do not take (w < 3, w > 32767, h < 1, h > 65535)."""
        frames = list(frames)
        if not frames:
            raise ValueError("RaggedFrames: an empty list of frames")
        device = torch.device(device)
        sizes, offsets, off = [], [], 0
        for i, f in enumerate(frames):
            if isinstance(f, np.ndarray):
                if f.dtype != np.uint8:
                    raise ValueError(f"RaggedFrames: frame {i} has dtype {f.dtype}, expected uint8")
            elif isinstance(f, torch.Tensor):
                if f.dtype != torch.uint8:
                    raise ValueError(f"RaggedFrames: frame {i} has dtype {f.dtype}, expected uint8")
            else:
                raise ValueError(f"RaggedFrames: frame {i} is a {type(f).__name__}, expected a tensor or numpy array")
            if f.ndim != 3 or f.shape[2] != 3:
                raise ValueError(f"RaggedFrames: frame {i} has shape {tuple(f.shape)}, expected (h, w, 3)")
            h, w = int(f.shape[0]), int(f.shape[1])
            if not (1 <= h <= L.FRAME_MAX_H and L.FRAME_MIN_W <= w <= L.FRAME_MAX_W):
                raise ValueError(f"RaggedFrames: frame {i} is {h} x {w}; the ragged kernels take 1 <= h <= {L.FRAME_MAX_H}, "
                                 f"{L.FRAME_MIN_W} <= w <= {L.FRAME_MAX_W}")
            sizes.append((h, w))
            offsets.append(off)
            off += h * w * 3
        data = torch.empty((off,), dtype=torch.uint8, device=device)
        for f, o, (h, w) in zip(frames, offsets, sizes):
            src = torch.from_numpy(np.ascontiguousarray(f)) if isinstance(f, np.ndarray) else f
            data[o:o + h * w * 3].view(h, w, 3).copy_(src, non_blocking=True)
        return cls(data, sizes, offsets, torch.from_numpy(frame_descs(offsets, sizes).view(np.uint8)).to(device))

    def __len__(self):
        return len(self.sizes)

    @property
    def device(self):
        return self.data.device

    def frame(self, i):
        """Frame i as an (h, w, 3) view into the packed buffer."""
        h, w = self.sizes[i]
        o = self.offsets[i]
        return self.data[o:o + h * w * 3].view(h, w, 3)

    def to_list(self):
        return [self.frame(i) for i in range(len(self))]

    def record_stream(self, stream):
        """Tensor.record_stream for the device buffers (work on another stream reads them)."""
        self.data.record_stream(stream)
        self.descs.record_stream(stream)

    def cached(self, key, make):
        """A device tensor derived from the batch's sizes alone (letterbox items, scale_coords values), built once."""
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]


# ---------------------------------------------------------------------------------------------- either kind of batch

def frame_descs(offsets, sizes):
    """fp_frame_desc rows (host, (B, 2) int64 = 16 bytes a row) of frames of sizes [(h, w)] at byte offsets `offsets`."""
    d = np.zeros((len(sizes), 2), np.int64)
    d[:, 0] = offsets
    d[:, 1] = [int(h) | (int(w) << 32) for h, w in sizes]     # int32 h, int32 w (little-endian)
    return d


def uniform_descs(B, H, W):
    """frame_descs of B packed H x W frames."""
    return frame_descs(np.arange(B, dtype=np.int64) * (H * W * 3), [(H, W)] * B)


DESCS_CACHE_SIZE = 8
_DESCS = OrderedDict()     # (B, H, W, device) -> device descriptors of a dense batch, oldest first


def device_descs(frames):
    """The (B, 16) u8 device fp_frame_desc array of a batch: a RaggedFrames' own, a dense (B, H, W, 3) tensor's from a small
    cache keyed by its shape and device (built once per shape; the DESCS_CACHE_SIZE latest shapes are kept)."""
    if isinstance(frames, RaggedFrames):
        return frames.descs
    B, H, W, _ = frames.shape
    key = (B, H, W, frames.device)
    d = _DESCS.get(key)
    if d is None:
        d = _DESCS[key] = torch.from_numpy(uniform_descs(B, H, W).view(np.uint8)).to(frames.device)
        if len(_DESCS) > DESCS_CACHE_SIZE:
            _DESCS.popitem(last=False)
    return d


def as_frames(frames, device):
    """What a caller has -> a batch on `device`: a RaggedFrames is returned as it is; a (B, H, W, 3) uint8 numpy array or
    tensor becomes a contiguous device tensor; a list of (h, w, 3) frames is stacked into one if they share a size and packed
    into a RaggedFrames otherwise.  ValueError for another dtype or shape."""
    if isinstance(frames, RaggedFrames):
        return frames
    if isinstance(frames, (list, tuple)):
        if not frames or any(not hasattr(f, "shape") or tuple(f.shape) != tuple(frames[0].shape) for f in frames):
            return RaggedFrames.from_list(frames, device)
        frames = torch.stack([(torch.from_numpy(np.ascontiguousarray(f)) if isinstance(f, np.ndarray) else f).to(device)
                              for f in frames])
    if isinstance(frames, np.ndarray):
        frames = torch.from_numpy(np.ascontiguousarray(frames))
    if frames.dtype != torch.uint8 or frames.ndim != 4 or frames.shape[3] != 3:
        raise ValueError(f"frames: (B, H, W, 3) uint8 expected, got {tuple(frames.shape)} {frames.dtype}")
    return frames.to(device).contiguous()


def batch_len(frames):
    return len(frames) if isinstance(frames, RaggedFrames) else frames.shape[0]


def frame_layout(frames):
    """Host [(byte offset, h, w)] per frame of the batch's buffer."""
    if isinstance(frames, RaggedFrames):
        return [(o, h, w) for o, (h, w) in zip(frames.offsets, frames.sizes)]
    B, H, W, _ = frames.shape
    return [(i * H * W * 3, H, W) for i in range(B)]


def frame_bytes(frames):
    """The batch's buffer as one flat u8 tensor (frame_layout's offsets index it)."""
    return frames.data if isinstance(frames, RaggedFrames) else frames.view(-1)


def frame_call_args(frames):
    """How the C entry points take the frames of each kind: (True, (data, bytes, descs, B)), the arguments a *_ragged form
    starts with, for a RaggedFrames; (False, (frames, B, H, W)), those of the dense form, for a (B, H, W, 3) tensor."""
    if isinstance(frames, RaggedFrames):
        return True, (L.ptr(frames.data), frames.data.numel(), L.ptr(frames.descs), len(frames))
    B, H, W, _ = frames.shape
    return False, (L.ptr(frames), B, H, W)


def resize_items(frames, items, n_items, canvas, lut=None, pad_value=125, swap_rb=False):
    """Resize the rectangles of items (n, 9) int32 device fp_resize_item rows, whose src_image indexes `frames`, into
    canvas[:n_items]: fp_resize_normalize for a dense batch, fp_resize_ragged for a RaggedFrames (bit-identical on the same
    rectangles).  canvas (n, h, w, C) float32 through the LUT (C = 4 for a RaggedFrames); lut None (RaggedFrames only):
    canvas (n, h, w, 3) uint8, the u8 value before any LUT, no R/B swap."""
    lib = L.load()
    ragged, fa = frame_call_args(frames)
    assert canvas.is_contiguous() and canvas.shape[0] >= n_items
    if lut is None:
        assert ragged and canvas.dtype == torch.uint8 and not swap_rb
    else:
        assert canvas.dtype == torch.float32
    shape = (canvas.shape[1], canvas.shape[2], canvas.shape[3])
    tail = (L.ptr(lut), int(pad_value), int(bool(swap_rb)), L.current_stream(frames.device))
    if ragged:
        mode = L.RAGGED_U8 if lut is None else L.RAGGED_F32_LUT
        L.check(lib.fp_resize_ragged(*fa, L.ptr(items), int(n_items), L.ptr(canvas), *shape, mode, *tail), "fp_resize_ragged")
    else:
        L.check(lib.fp_resize_normalize(*fa, L.ptr(items), int(n_items), L.ptr(canvas), *shape, *tail), "fp_resize_normalize")
    return canvas


resize_ragged = resize_items     # the name the ragged callers know


# ---------------------------------------------------------------------------------------------- detections -> crops

def scale_coords_params(in_size, orig_size):
    """gain / pad of scale_coords (modules/utils/image.py:83-87) as fp32 (numpy promotes python floats to the
    float32 array dtype)."""
    iw, ih = in_size
    w, h = orig_size
    gain = min(ih / h, iw / w)
    pad_x, pad_y = (iw - w * gain) / 2, (ih - h * gain) / 2
    return np.float32(gain), np.float32(pad_x), np.float32(pad_y)


def ragged_scale_coords_params(in_size, sizes):
    """(B, 3) float32 host array: scale_coords_params of every (h, w) in sizes, row = (gain, pad_x, pad_y)."""
    return np.array([scale_coords_params(in_size, (w, h)) for h, w in sizes], dtype=np.float32).reshape(-1, 3)


def dets_to_crops(frames, dets, counts, det, dst, cap, offsets, align_out=None):
    """Device-side B7 + crop arithmetic of detector `det`'s rows (dets (B, max_dets, row), counts (B,)) -> (items (cap, 9),
    info (cap, 7), n_faces (1,)), crops resized to dst = (w, h), box offsets (tx, ty, bx, by).  The entry point follows
    det.dets_fmt, the kind of `frames` and align_out (dict(lmarks, M, flags), modules/utils/align.py alloc: also written):
    fmt 2 -> fp_dets_to_crops_px; else fp_dets_to_crops[_aligned] for a dense batch and [_aligned]_ragged for a RaggedFrames
    (each frame's boxes in its own pixels: per-frame scale_coords values, the same fp32 numbers as a frame alone)."""
    lib, dev = L.load(), dets.device
    fmt, row = det.dets_fmt, dets.shape[-1]
    items = torch.empty((cap, 9), dtype=torch.int32, device=dev)
    info = torch.empty((cap, 7), dtype=torch.float32, device=dev)
    nf = torch.empty((1,), dtype=torch.int32, device=dev)
    al = () if align_out is None else (L.ptr(align_out["lmarks"]), L.ptr(align_out["M"]), L.ptr(align_out["flags"]))
    head = (L.ptr(dets), L.ptr(counts), batch_len(frames), dets.shape[1], row)
    thres = (float(det.det_thres), float(det.bbox_area_thres))
    tail = (*offsets, dst[0], dst[1], cap, L.ptr(items), L.ptr(info), L.ptr(nf))
    stream = L.current_stream(dev)
    if fmt == 2:
        # rows already in each frame's own pixels (MTCNN: the detector's "input size" is the frame): no scale_coords values
        name, args = "fp_dets_to_crops_px", (*head, L.ptr(device_descs(frames)), *thres, *tail, *(al or (None,) * 3), stream)
    else:
        if al and fmt == 1 and row < 15:
            raise L.FacepathError(f"align=True needs detector rows with landmarks (got {row} columns)")
        iw, ih = det.input_size
        name = "fp_dets_to_crops_aligned" if al else "fp_dets_to_crops"
        if isinstance(frames, RaggedFrames):
            geom = frames.cached(("scale_coords", iw, ih), lambda: torch.from_numpy(ragged_scale_coords_params(
                (iw, ih), frames.sizes)).to(dev))
            name, args = name + "_ragged", (*head, fmt, iw, ih, L.ptr(frames.descs), L.ptr(geom), *thres, *tail, *al, stream)
        else:
            _, H, W, _ = frames.shape
            gain, px, py = scale_coords_params((iw, ih), (W, H))
            args = (*head, fmt, iw, ih, W, H, *thres, float(gain), float(px), float(py), *tail, *al, stream)
    L.check(getattr(lib, name)(*args), name)
    return items, info, nf
