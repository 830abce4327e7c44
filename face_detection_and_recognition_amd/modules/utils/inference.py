"""Inference drivers (face_detection_and_extraction/modules/utils/inference.py).  The GUI loops (cv2.imshow, the webcam's
VideoCapture) are out of scope; ``inference_img`` keeps its signature, returns the post-processed detections and, instead of
showing the drawn frame in a window, saves it when asked to (``save``).  ``inference_vid`` runs a Motion-JPEG video file
(modules/utils/video.py) batch by batch and, instead of showing the frames, writes them annotated to an AVI when asked to."""
import os
from typing import Any, List, Optional, Tuple

import numpy as np

from ..models.base import Model, PostProcessedDetection
from .image import draw_bbox_on_image, scale_coords


def get_dets_bboxes_confs_lmarks_areas(dets: np.ndarray, orig_size: Tuple[int, int], in_size: Tuple[int, int],
                                       det_thres: float, bbox_area_thres: float,
                                       opt_labels: Optional[List[Any]] = None) -> PostProcessedDetection:
    """inference.py:11-58: threshold (strict >), de-normalise to the model input size, area filter
    (100*fraction > thres; the stored value is the fraction), un-letterbox, round."""
    w, h = orig_size
    iw, ih = in_size
    dets = dets[dets[:, -1] > det_thres]
    dets[:, :-1] = dets[:, :-1] * np.array([iw, ih] * ((dets.shape[-1] - 1) // 2))
    bbox_area_perc = ((dets[:, 2] - dets[:, 0]) * (dets[:, 3] - dets[:, 1])) / (iw * ih)
    keep = (100 * bbox_area_perc) > bbox_area_thres
    dets, bbox_area_perc = dets[keep], bbox_area_perc[keep]
    confs = dets[:, -1]
    dets = scale_coords((ih, iw), dets[:, :-1], (h, w)).round()
    return PostProcessedDetection(boxes=dets[:, :4], bbox_confs=confs, bbox_areas=bbox_area_perc,
                                  bbox_lmarks=dets[:, 4:], bbox_labels=opt_labels)


def load_image(path: str, device=None, reduce: int = 1, orientation: bool = True):
    """BGR HWC u8 like cv2.imread (inference.py:68-76), upright by the file's EXIF Orientation tag as cv2.imread returns it
    (orientation=False: IMREAD_IGNORE_ORIENTATION); reduce = 2 / 4 / 8: IMREAD_REDUCED_COLOR_2 / _4 / _8, libjpeg's reduced-size
    decode of a JPEG.  device = a HIP device: the frame is decoded there (baseline JPEGs: host Huffman + device reconstruction,
    modules/utils/jpeg.py, byte-identical to libjpeg-turbo) and returned as a device tensor; device = None: numpy array decoded
    by Pillow on the host (cv2 is not a dependency of this build)."""
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} does not exist")
    from .jpeg import _check_reduce, _pillow_decode, imread
    _check_reduce(reduce)
    if device is not None:
        return imread(path, device, bgr=True, reduce=reduce, orientation=orientation)
    with open(path, "rb") as f:
        return np.ascontiguousarray(_pillow_decode(f.read(), reduce, orientation)[..., ::-1])


def save_annotated(path: str, image, post: PostProcessedDetection, anonymize: int = 0, device=None):
    """The tail of the reference's inference_img with a file in place of the window: draw_bbox_on_image on a device copy of
    `image` (numpy or device tensor; the caller's frame stays as it is), then imwrite (cv2.imwrite's bytes)."""
    import torch
    from .jpeg import imwrite
    if isinstance(image, np.ndarray):
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        frame = torch.from_numpy(np.ascontiguousarray(image)).to(dev)
    else:
        frame = image.contiguous().clone()
    draw_bbox_on_image(frame, post, anonymize=anonymize)
    return imwrite(path, frame)


def inference_img(net: Model, img, waitKey_val: int = 0, save: Optional[str] = None, anonymize: int = 0, reduce: int = 1,
                  orientation: bool = True) -> PostProcessedDetection:
    """inference.py:61-93; the drawing / imshow tail becomes: with `save`, the frame with its detections drawn on (faces
    pixelated first with anonymize = a mosaic cell) is written to that path.  The return value does not depend on it.
    reduce, orientation: how a file is read (load_image)."""
    # a net that takes device frames gets the file decoded ON its device (baseline JPEG: host Huffman + device IDCT / upsampling
    # / colour conversion, byte-identical to cv2.imread's libjpeg-turbo); everything else the host array, as the reference
    dev = net.net._device() if getattr(net, "accepts_device_frames", False) else None
    image = load_image(img, dev if dev is not None and dev.type == "cuda" else None, reduce, orientation) if isinstance(img, str) else img
    h, w = image.shape[:2]
    dets = net(image)
    labels = None
    if net.returns_opt_labels:
        dets, labels = dets
    post = get_dets_bboxes_confs_lmarks_areas(dets, (w, h), net.input_size, net.det_thres, net.bbox_area_thres, labels)
    if save:
        save_annotated(save, image, post, anonymize, dev)
    return post


def _batch_dets(net, frames, w, h):
    """The net's rows for every frame of a decoded batch (device tensor, one size), each what net(frame) gives.  A net with a
    batched path (predict_batch) takes the batch at once; a net whose rows are normalised by the frame (dets_fmt 2: the tiled
    detector) gets its input_size set to the frames' (w, h) first, as its __call__ sets it per image.  Other nets go frame by
    frame: on the device where they take device frames, else on host copies (YOLOV5FaceModel.__call__ takes numpy arrays)."""
    if hasattr(net, "predict_batch"):
        if getattr(net, "dets_fmt", None) == 2:
            net.input_size = (w, h)
        return net.predict_batch(frames)
    if getattr(net, "accepts_device_frames", False):
        return [net(f) for f in frames]
    return [net(f) for f in frames.cpu().numpy()]


def inference_vid(net: Model, vid: str, save: Optional[str] = None, batch: int = 64, anonymize: int = 0, entropy: str = "host",
                  fps=None, reduce: int = 1) -> List[PostProcessedDetection]:
    """inference.py:96-111 for a Motion-JPEG video file (AVI or a raw .mjpeg stream, modules/utils/video.py; every other codec
    raises VideoUnsupported): one PostProcessedDetection per frame, what inference_img returns for that frame.  The file is
    decoded `batch` frames at a time on the net's device (decode_video_batch: one launch sequence per chunk) and goes through
    the net's batched path where it has one (predict_batch), else frame by frame (_batch_dets).  With `save`, the frames with
    their detections drawn on (faces pixelated first with anonymize = a mosaic cell) are written to that path as a Motion-JPEG
    AVI at the source's frame rate (VideoWriter; below 2 GiB).  fps: the rate to write where the source states none (a raw
    stream).  reduce = 2 / 4 / 8: the frames are decoded at that fraction of their size, as load_image reads a file (AVI
    carries no EXIF: there is no orientation to apply)."""
    from .video import VideoReader, VideoWriter
    if not hasattr(getattr(net, "net", None), "_device"):
        raise NotImplementedError("inference_vid decodes the video on the net's device: a net on a HIP device is needed")
    dev = net.net._device()
    posts: List[PostProcessedDetection] = []
    with VideoReader(vid) as reader:
        rate = reader.fps if reader.fps is not None else fps
        if save and rate is None:
            raise ValueError(f"{vid} states no frame rate (a raw MJPEG stream): pass fps= to write {save}")
        writer = VideoWriter(save, rate) if save else None
        try:
            for _, frames in reader.batches(batch, dev, entropy=entropy, reduce=reduce):
                h, w = int(frames.shape[1]), int(frames.shape[2])
                first = len(posts)
                for dets in _batch_dets(net, frames, w, h):
                    labels = None
                    if net.returns_opt_labels:
                        dets, labels = dets
                    posts.append(get_dets_bboxes_confs_lmarks_areas(dets, (w, h), net.input_size, net.det_thres,
                                                                    net.bbox_area_thres, labels))
                if writer is not None:
                    for i in range(frames.shape[0]):            # the decoded batch is this function's own: drawn on in place
                        draw_bbox_on_image(frames[i], posts[first + i], anonymize=anonymize)
                    writer.write(frames)
        finally:
            if writer is not None:
                writer.close()
    return posts
