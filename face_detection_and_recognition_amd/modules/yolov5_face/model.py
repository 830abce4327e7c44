"""YOLOV5FaceModel plugin (face_detection_and_extraction/modules/yolov5_face/model.py:8-37) + batched path."""
from typing import Any, Callable, Tuple

import numpy as np

from ...frames import as_frames
from ..models.base import Model
from . import nms_face_device, preprocess_batch
from .general import MAX_DET


class YOLOV5FaceModel(Model):

    __slots__ = ["net", "inf_func", "augment"]
    dets_fmt = 1     # rows are (x1, y1, x2, y2, conf, ...) in model-input pixels (pipeline.py / fp_dets_to_crops)

    def __init__(self, net: Any, det_thres: float, bbox_area_thres: float, inf_func: Callable,
                 input_size: Tuple[int, int], augment: bool = False):
        """augment: augmented inference (the reference's three views behind one NMS, Model.run_views) in __call__ and
        raw_batch."""
        Model.__init__(self, input_size, det_thres, bbox_area_thres)
        self.net = net
        self.inf_func = inf_func
        self.augment = bool(augment)

    def __call__(self, cv2_img: np.ndarray, augment=None) -> np.ndarray:
        """model.py:23-37: (k, 5) [xmin, ymin, xmax, ymax, conf] normalised to [0, 1].  augment: None = the model's own."""
        iw, ih = self.input_size
        if self.augment if augment is None else augment:
            detections = self.inf_func(self.net, cv2_img, self.input_size, augment=True)
        else:
            detections = self.inf_func(self.net, cv2_img, self.input_size)
        if detections is not None and len(detections):
            detections = detections.cpu().numpy()
            detections[:, :4] = detections[:, :4] / np.array([iw, ih, iw, ih])
            detections = detections[:, :5]
        else:
            detections = np.zeros((0, 5), dtype=np.float32)   # the reference returns an uninitialised (0, 5) array
        return detections

    def raw_batch(self, frames, max_det=MAX_DET):
        """frames (B, H, W, 3) u8 BGR or a RaggedFrames -> device dets (B, max_det, 16) in input pixels, counts (B,), overflow (B,).
        overflow[i] != 0: image i had more than max_det survivors and was truncated; the caller re-runs with
        ``max_det=None`` (no cap, as non_max_suppression_face does) -- FacePipeline.step reads the flag in the same
        host transfer as the face count.  With ``augment`` the rows of the three views go through the one NMS, their
        landmarks mapped to the input's pixels ("mapped": crops, alignment, quality and drawing read them); the views are
        built from the fp32 canvas, so the stem that reads u8 frames is not used."""
        plan = preprocess_batch(self.net, as_frames(frames, self.net._device()), self.input_size, fused=not self.augment)
        z = self.net.run_views(plan, "mapped") if self.augment else self.net.run_plan(plan)
        self.net.last_plan = plan     # measurement / tests: the plan (and its decoded head output plan.z) of the last batch
        out, cnt, _, over = nms_face_device(z, conf_thres=0.4, iou_thres=0.5,
                                            max_det=z.shape[1] if max_det is None else max_det)
        return out, cnt, over
