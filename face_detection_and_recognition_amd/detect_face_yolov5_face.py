"""``python -m face_detection_and_recognition_amd.detect_face_yolov5_face -i img.jpg --md yolov5n-face.pt``
Entry point with the reference's flags (face_detection_and_extraction/detect_face_yolov5_face.py:13-66).  Images and Motion-JPEG
video files (``-i clip.avi`` / ``clip.mjpeg``, modules/utils/video.py: one JSON record per frame, ``-o out.avi`` writes the annotated
video; the webcam GUI loop is out of scope).  ``-o out.jpg`` also
saves the image with the detections drawn on, ``--anonymize CELL`` pixelates the faces in it first (annotate.py).  ``--tile W H
--merge_thr T`` (with ``--overlap``, ``--edge_px``, ``--no_full_frame``) runs the detector on overlapping tiles of the image as well and
merges the detections on the device (tiling.py).  ``--augment`` runs the reference's augmented inference: the image, the image
mirrored and scaled by 0.83, and the image scaled by 0.67, behind one NMS (modules/yolov5_face/tta.py)."""
import argparse
import json
import os
from typing import Tuple

from .modules.utils.files import get_file_type
from .modules.utils.inference import inference_img, inference_vid
from .modules.utils.parser import add_read_args, get_argparse, read_kwargs, torch_device
from .modules.yolov5_face import attempt_load, inference_pytorch_model_yolov5_face
from .modules.yolov5_face.model import YOLOV5FaceModel
from .tiling import add_tile_args, wrap_from_args


def load_model(model_path: str, det_thres: float, bbox_area_thres: float, model_in_size: Tuple[int, int], device: str,
               augment: bool = False):
    """detect_face_yolov5_face.py:13-38: .pt/.pth (state_dict) -> HIP network; .onnx sessions are out of scope."""
    _, fext = os.path.splitext(model_path)
    if fext in {".pt", ".pth"}:
        net = attempt_load(model_path, torch_device(device))
    else:
        raise NotImplementedError(f"[ERROR] model with extension {fext} not implemented")
    return YOLOV5FaceModel(net, det_thres, bbox_area_thres, inference_pytorch_model_yolov5_face, model_in_size, augment=augment)


def build_parser():
    parser = get_argparse(description="YOLOv5-face face detection (MI355X HIP path)", conflict_handler='resolve')
    parser.remove_argument("model")
    parser.add_argument("--md", "--model", dest="model", default="weights/yolov5s/yolov5s-face.pt",
                        help='Path to weight file (.pt/.pth state_dict). (default: %(default)s).')
    parser.add_argument("--is", "--input_size", dest="input_size", nargs=2, default=(640, 640),
                        help='Input images are resized to this size (width, height). (default: %(default)s).')
    parser.add_argument("-o", "--output", dest="output", default=argparse.SUPPRESS,
                        help="Write the image with its detections drawn on (box, landmarks, caption) to this JPEG file; for a video input, the "
                             "annotated frames to this Motion-JPEG AVI file (AVI 1.0: below 2 GiB, OpenDML is out of scope).")
    parser.add_argument("--anonymize", dest="anonymize", type=int, choices=[4, 8, 16, 32], default=argparse.SUPPRESS, metavar="CELL",
                        help="With -o: pixelate every detected face first, mosaic cells of CELL x CELL pixels (4, 8, 16 or 32).")
    parser.add_argument("--augment", action="store_true", default=argparse.SUPPRESS,
                        help="Augmented inference: also run the image mirrored at scale 0.83 and at scale 0.67, one NMS over all rows.")
    return add_read_args(add_tile_args(parser))


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    print("Current Arguments: ", args)
    args.input_size = tuple(map(int, args.input_size))
    net = load_model(args.model, args.det_thres, args.bbox_area_thres, args.input_size, args.device, augment=getattr(args, "augment", False))
    net = wrap_from_args(net, args, parser.error)
    if get_file_type(args.input_src) == "video":
        posts = inference_vid(net, args.input_src, save=getattr(args, "output", None), anonymize=getattr(args, "anonymize", 0),
                              reduce=getattr(args, "reduce", 1))
        for frame, post in enumerate(posts):
            print(json.dumps({"frame": frame, "boxes": post.boxes.tolist(), "confs": post.bbox_confs.tolist(),
                              "areas": post.bbox_areas.tolist()}))
        return posts
    post = inference_img(net, args.input_src, save=getattr(args, "output", None), anonymize=getattr(args, "anonymize", 0),
                         **read_kwargs(args))
    print(json.dumps({"boxes": post.boxes.tolist(), "confs": post.bbox_confs.tolist(), "areas": post.bbox_areas.tolist()}))
    return post


if __name__ == "__main__":
    main()
