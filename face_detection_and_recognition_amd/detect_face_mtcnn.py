"""``python -m face_detection_and_recognition_amd.detect_face_mtcnn -i img.jpg --mt fast --md weights.npz``
Entry point with the reference's flags (face_detection_and_extraction/detect_face_mtcnn.py).  Images and Motion-JPEG video files
(``-i clip.avi`` / ``clip.mjpeg``, modules/utils/video.py: one JSON record per frame, ``-o out.avi`` writes the annotated video; the
webcam GUI loop is out of scope); for an image it prints the detector's rows (15 numbers each: box, five landmarks, confidence, normalised
by the image size) and the post-processed detections as JSON.  ``-o out.jpg`` also saves the image with the detections drawn
on, ``--anonymize CELL`` pixelates the faces in it first (annotate.py).  ``--md synthetic`` runs seeded random weights calibrated on the image (synth.py)."""
import argparse
import json

from .modules.mtcnn.model import SLOW_DEFAULTS, SLOW_WEIGHTS, MTCNNFastModel, MTCNNSlowModel
from .modules.utils.files import get_file_type
from .modules.utils.inference import get_dets_bboxes_confs_lmarks_areas, inference_vid, load_image, save_annotated
from .modules.utils.parser import add_read_args, get_argparse, read_kwargs, torch_device
from .tiling import add_tile_args


def load_model(model_type, model_path, det_thres, bbox_area_thres, device, image=None):
    net = None
    if model_path == "synthetic":      # seeded random weights, their heads calibrated on the image itself (synth.synth_mtcnn)
        from .modules.mtcnn.mtcnn import MTCNN
        from .synth import synth_mtcnn
        kw = SLOW_DEFAULTS if model_type == "slow" else dict(min_face_size=40, factor=0.7, thresholds=(0.6, 0.7, 0.8))
        net = synth_mtcnn(MTCNN(cap=8192, **kw), 0, shares=(0.005, 0.4, 0.5), frames=None if image is None else image[None]).to(device)
    if model_type == "fast":
        return MTCNNFastModel(model_path, det_thres, bbox_area_thres, device=device, net=net)
    if model_type == "slow":
        return MTCNNSlowModel(det_thres, bbox_area_thres, model_path=model_path, device=device, net=net)
    raise NotImplementedError(f"{model_type} is not supported")


def video_main(args):
    """-i clip.avi: inference_vid over the file; --md synthetic calibrates its heads on the first frame."""
    first = None
    if args.model == "synthetic":
        import io
        import numpy as np
        from PIL import Image
        from .modules.utils.video import VideoReader
        with VideoReader(args.input_src) as reader:
            first = np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(reader.frame_bytes(0))).convert("RGB"))[..., ::-1])
    net = load_model(args.model_type, args.model, args.det_thres, args.bbox_area_thres, torch_device(args.device), first)
    posts = inference_vid(net, args.input_src, save=getattr(args, "output", None), anonymize=getattr(args, "anonymize", 0),
                          reduce=getattr(args, "reduce", 1))
    for frame, post in enumerate(posts):
        print(json.dumps({"frame": frame, "boxes": post.boxes.tolist(), "confs": post.bbox_confs.tolist(),
                          "areas": post.bbox_areas.tolist(), "landmarks": post.bbox_lmarks.tolist()}))
    return posts


def build_parser():
    parser = get_argparse(description="MTCNN face detection (MI355X HIP path)", conflict_handler='resolve')
    parser.add_argument("--md", "--model", dest="model", default=SLOW_WEIGHTS,
                        help="Path to the weights (.npz state dict, .npy port dictionary, .pth) or 'synthetic'. (default: %(default)s)")
    parser.add_argument("--mt", "--model_type", dest="model_type", default="fast", choices=["fast", "slow"],
                        help="MTCNN model type, fast or slow (default: %(default)s).")
    parser.add_argument("-o", "--output", dest="output", default=argparse.SUPPRESS,
                        help="Write the image with its detections drawn on (box, landmarks, caption) to this JPEG file; for a video input, the "
                             "annotated frames to this Motion-JPEG AVI file (AVI 1.0: below 2 GiB, OpenDML is out of scope).")
    parser.add_argument("--anonymize", dest="anonymize", type=int, choices=[4, 8, 16, 32], default=argparse.SUPPRESS, metavar="CELL",
                        help="With -o: pixelate every detected face first, mosaic cells of CELL x CELL pixels (4, 8, 16 or 32).")
    return add_read_args(add_tile_args(parser))      # (tile flags:) accepted so that the three entry points share their flags; MTCNN refuses --tile


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if getattr(args, "tile", None) is not None:
        parser.error("--tile: MTCNN scans its own image pyramid and is not tiled (tiling.TiledDetector refuses it)")
    print("Current Arguments: ", args)
    if get_file_type(args.input_src) == "video":
        return video_main(args)
    image = load_image(args.input_src, **read_kwargs(args))
    net = load_model(args.model_type, args.model, args.det_thres, args.bbox_area_thres, torch_device(args.device), image)
    h, w = image.shape[:2]
    dets = net(image)
    for row in dets:
        print(" ".join(f"{v:.6f}" for v in row))
    post = get_dets_bboxes_confs_lmarks_areas(dets.copy(), (w, h), net.input_size, net.det_thres, net.bbox_area_thres)
    print(json.dumps({"boxes": post.boxes.tolist(), "confs": post.bbox_confs.tolist(),
                      "areas": post.bbox_areas.tolist(), "landmarks": post.bbox_lmarks.tolist()}))
    if getattr(args, "output", None):
        save_annotated(args.output, image, post, getattr(args, "anonymize", 0), torch_device(args.device))
    return dets


if __name__ == "__main__":
    main()
