"""``python -m face_detection_and_recognition_amd.detect_face_blazeface -i img.jpg --md w.pth --mt back``
Entry point with the reference's flags (face_detection_and_extraction/detect_face_blazeface.py:7-34).  Images
and Motion-JPEG video files (``-i clip.avi`` / ``clip.mjpeg``, modules/utils/video.py: one JSON record per frame, ``-o out.avi`` writes
the annotated video; the webcam GUI loop is out of scope); prints the post-processed detections as JSON.  ``-o out.jpg`` also
saves the image with the detections drawn on, ``--anonymize CELL`` pixelates the faces in it first (annotate.py).  ``--tile W H
--merge_thr T`` (with ``--overlap``, ``--edge_px``, ``--no_full_frame``) runs the detector on overlapping tiles of the image as well and
merges the detections on the device (tiling.py)."""
import argparse
import json

from .modules.blazeface.model import BlazeFaceModel
from .modules.utils.files import get_file_type
from .modules.utils.inference import inference_img, inference_vid
from .modules.utils.parser import add_read_args, get_argparse, read_kwargs, torch_device
from .tiling import add_tile_args, wrap_from_args


def build_parser():
    parser = get_argparse(description="Blazeface face detection (MI355X HIP path)", conflict_handler='resolve')
    parser.add_argument("--md", "--model", dest="model", default="weights/blazeface/blazefaceback.pth",
                        help="Path to weight file (.pth). anchors.npy next to it is used when present, "
                             "otherwise the MediaPipe anchors are generated. (default: %(default)s)")
    parser.add_argument("--mt", "--model_type", dest="model_type", default="back", choices=["back", "front"],
                        help="Model type back or front; must match the weight file. (default: %(default)s)")
    parser.add_argument("-o", "--output", dest="output", default=argparse.SUPPRESS,
                        help="Write the image with its detections drawn on (box, landmarks, caption) to this JPEG file; for a video input, the "
                             "annotated frames to this Motion-JPEG AVI file (AVI 1.0: below 2 GiB, OpenDML is out of scope).")
    parser.add_argument("--anonymize", dest="anonymize", type=int, choices=[4, 8, 16, 32], default=argparse.SUPPRESS, metavar="CELL",
                        help="With -o: pixelate every detected face first, mosaic cells of CELL x CELL pixels (4, 8, 16 or 32).")
    return add_read_args(add_tile_args(parser))


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    print("Current Arguments: ", args)
    net = BlazeFaceModel(args.model, args.det_thres, args.bbox_area_thres, args.model_type,
                         torch_device(args.device))
    net = wrap_from_args(net, args, parser.error)
    if get_file_type(args.input_src) == "video":
        posts = inference_vid(net, args.input_src, save=getattr(args, "output", None), anonymize=getattr(args, "anonymize", 0),
                              reduce=getattr(args, "reduce", 1))
        for frame, post in enumerate(posts):
            print(json.dumps({"frame": frame, "boxes": post.boxes.tolist(), "confs": post.bbox_confs.tolist(),
                              "areas": post.bbox_areas.tolist(), "landmarks": post.bbox_lmarks.tolist()}))
        return posts
    post = inference_img(net, args.input_src, save=getattr(args, "output", None), anonymize=getattr(args, "anonymize", 0),
                         **read_kwargs(args))
    print(json.dumps({"boxes": post.boxes.tolist(), "confs": post.bbox_confs.tolist(),
                      "areas": post.bbox_areas.tolist(), "landmarks": post.bbox_lmarks.tolist()}))
    return post


if __name__ == "__main__":
    main()
