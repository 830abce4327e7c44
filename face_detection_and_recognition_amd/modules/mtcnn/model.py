"""MTCNNSlowModel / MTCNNFastModel plugins (face_detection_and_extraction/modules/mtcnn/model.py) on the HIP cascade.

The reference's two wrappers differ in the runtime behind them (the `mtcnn` package / a TensorFlow graph) and in their
parameters; here both run modules/mtcnn/mtcnn.py's MTCNN, with the slow model's defaults (min face 20, factor 0.709,
thresholds 0.6 / 0.7 / 0.7) or the fast model's (40, 0.7, 0.6 / 0.7 / 0.8).  The contract they keep: ``__call__(BGR HWC u8)``
sets ``input_size`` to the image's (w, h) and returns (n, 15) rows [xmin, ymin, xmax, ymax, (x, y) of left_eye, right_eye,
nose, mouth_left, mouth_right, conf] normalised by (w, h); no face gives an array of shape (0, 15).  Equality with the
package's / the graph's numbers is parity-unpinned.
"""
import os
from typing import Tuple

import numpy as np
import torch

from ..models.base import Model
from .mtcnn import MTCNN, check_params

SLOW_DEFAULTS = dict(min_face_size=20, factor=0.709, thresholds=(0.6, 0.7, 0.7))
SLOW_WEIGHTS = "weights/mtcnn/mtcnn_weights.npy"


def load_net(model_path: str, device: str, **kw) -> MTCNN:
    """``.npz`` (our state dict, MTCNN.save_npz), ``.npy`` (the classic port's weight dictionary) or ``.pth`` (a torch
    state dict); anything else -- the reference's ``.pb`` graph included -- is not implemented."""
    _, fext = os.path.splitext(model_path)
    if fext == ".npz":
        net = MTCNN.from_npz(model_path, **kw)
    elif fext == ".npy":
        net = MTCNN.from_keras_npy(model_path, **kw)
    elif fext == ".pth":
        net = MTCNN.from_state_dict(torch.load(model_path, map_location="cpu"), **kw)
    elif fext == ".pb":
        raise NotImplementedError("[ERROR] TensorFlow graphs are out of scope of the HIP build; pass the weights as .npz / .npy")
    else:
        raise NotImplementedError(f"[ERROR] model with extension {fext} not implemented")
    return net.to(device)


class _MTCNNModel(Model):
    """What the two wrappers share.  ``cascade`` is anything with detect_batch (tests pass a stub)."""

    __slots__ = ["net", "max_det"]
    accepts_device_frames = True
    dets_fmt = 2      # raw_batch rows are in each frame's own pixels (fp_dets_to_crops_px), landmarks at 4 .. 13, conf at 14

    def _init(self, det_thres, bbox_area_thres, net, max_det=64):
        Model.__init__(self, (None, None), det_thres, bbox_area_thres)
        self.net = net
        self.max_det = max_det

    def raw_batch(self, frames, max_det=-1):
        """frames: (B, H, W, 3) u8 BGR (numpy / CUDA tensor) or a RaggedFrames -> device (dets (B, max_det, 15) in each
        frame's own pixels, counts (B,), overflow (B,)).  max_det: -1 = this wrapper's default, None = no cap below the cascade's."""
        if max_det is None:          # "uncapped" (FacePipeline's re-run after an overflow): the cascade's own candidate cap
            max_det = getattr(self.net, "cap", self.max_det)
        return self.net.detect_batch(frames, max_det=self.max_det if max_det == -1 else max_det)

    def __call__(self, cv2_img) -> np.ndarray:
        self.input_size = tuple(int(v) for v in cv2_img.shape[:2][::-1])
        iw, ih = self.input_size
        dets, counts, _ = self.raw_batch(cv2_img[None])
        n = int(counts[0])
        if n == 0:
            return np.empty(shape=(0, 15), dtype=np.float32)
        rows = dets[0, :n].detach().cpu().numpy().astype(np.float32)
        rows[:, :14] /= np.asarray([iw, ih] * 7, np.float32)
        return rows


class MTCNNSlowModel(_MTCNNModel):

    def __init__(self, det_thres: float, bbox_area_thres: float, model_path: str = SLOW_WEIGHTS, device: str = "cuda",
                 net=None):
        self._init(det_thres, bbox_area_thres, net if net is not None else load_net(model_path, device, **SLOW_DEFAULTS))


class MTCNNFastModel(_MTCNNModel):

    __slots__ = ["min_size", "factor", "thresholds"]

    def __init__(self, model_path: str, det_thres: float, bbox_area_thres: float, min_size: int = 40, factor: float = 0.7,
                 thresholds: Tuple[float, float, float] = (0.6, 0.7, 0.8), device: str = "cuda", net=None):
        check_params(min_size, factor)
        self.min_size, self.factor, self.thresholds = min_size, factor, tuple(thresholds)
        if net is None:
            net = load_net(model_path, device, min_face_size=min_size, factor=factor, thresholds=thresholds)
        elif hasattr(net, "min_face_size"):      # an already-built cascade runs with THIS wrapper's parameters
            net.min_face_size, net.factor, net.thresholds = min_size, float(factor), tuple(float(t) for t in thresholds)
        self._init(det_thres, bbox_area_thres, net)
