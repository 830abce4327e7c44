"""Ragged batches: frames of different sizes in one device buffer.

Every batched entry point of the path takes one (B, H, W, 3) tensor, so all frames of a batch share a size.  The
reference's dataset driver reads folders of photos of any size (fde/face_extraction/extract_faces_from_dataset.py:380-405).
A RaggedFrames holds such a batch the way the ragged kernels read it (include/facepath.h section 2, ABI 14): the u8 BGR
frames packed back to back, one fp_frame_desc (byte offset of pixel (0, 0), h, w) per frame on the device, and the sizes
on the host.  BlazeFaceModel / YOLOV5FaceModel.raw_batch, FacePipeline and the dataset driver accept it wherever they
accept a (B, H, W, 3) tensor.
"""
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
        d = np.zeros((len(frames), 2), np.int64)
        d[:, 0] = offsets
        d[:, 1] = [h | (w << 32) for h, w in sizes]     # int32 h, int32 w (little-endian) = fp_frame_desc
        descs = torch.from_numpy(d.view(np.uint8)).to(device)
        return cls(data, sizes, offsets, descs)

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


def resize_ragged(frames, items, n_items, canvas, lut=None, pad_value=125, swap_rb=False):
    """fp_resize_ragged: items (n, 9) int32 CUDA fp_resize_item rows whose src_image indexes `frames` (a RaggedFrames).
    lut None: canvas (n, h, w, 3) uint8 (the u8 value before any LUT, no R/B swap); else canvas (n, h, w, 4) float32
    through the LUT, bit-identical to fp_resize_normalize on the same rectangles."""
    lib = L.load()
    if lut is None:
        mode, c = L.RAGGED_U8, 3
        assert canvas.dtype == torch.uint8 and not swap_rb
    else:
        mode, c = L.RAGGED_F32_LUT, canvas.shape[3]
        assert canvas.dtype == torch.float32
    assert canvas.is_contiguous() and canvas.shape[0] >= n_items
    L.check(lib.fp_resize_ragged(L.ptr(frames.data), frames.data.numel(), L.ptr(frames.descs), len(frames), L.ptr(items),
                                 int(n_items), L.ptr(canvas), canvas.shape[1], canvas.shape[2], c, mode, L.ptr(lut),
                                 int(pad_value), int(bool(swap_rb)), L.current_stream(frames.device)), "fp_resize_ragged")
    return canvas
