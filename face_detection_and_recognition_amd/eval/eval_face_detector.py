"""``python -m face_detection_and_recognition_amd.eval.eval_face_detector ann.txt images/ --model_type yolov5_face --model w.pt``

Scores a face detector on WIDER-style annotations with the twelve COCO bbox numbers, like the reference's
face_detection_and_extraction/eval/eval_face_detector.py -- which hands the work to pycocotools; here evaluation.py does it
(the kernels of csrc/deteval.hip on a HIP device, numpy with ``-d cpu``).  ``ann``, ``pics`` and
``--model`` are the reference's; ``--model_type`` takes blazeface, yolov5_face and mtcnn, ``--mt`` the variant (back / front,
fast / slow, or the YOLOv5-face architecture name), ``--is W H`` the input size, ``-d`` the device, ``--batch`` the frames
per detector call.  ``--dets detections.json`` scores an existing COCO-format detection file without running a detector.
``--model synthetic`` runs seeded random weights (synth.py / workload.py).  ``--tile W H --merge_thr T`` (with ``--overlap``,
``--edge_px``, ``--no_full_frame``) scores the detector run on overlapping tiles of every image and on the whole image
(tiling.TiledDetector; blazeface and yolov5_face, MTCNN refuses).  ``--augment`` scores YOLOv5-face with the reference's
augmented inference (three views behind one NMS; yolov5_face only, any other model type is refused).  Writes annotations.json and detections.json in
the reference's formats into ``--out`` (default: the current directory), prints the summary and returns the result.
"""
import argparse
import json
import os

import numpy as np
import torch

from ..evaluation import DetectionEvaluator, clamp_boxes_xywh, coco_eval_bbox, dets_to_frame_boxes
from ..tiling import add_tile_args, wrap_from_args


def parse_wider(path, images_root=""):
    """WIDER ``bbx_gt.txt``: records of a path, a count, then ``count`` lines whose first four integers are x y w h.  A
    count of 0 is followed by one all-zero dummy line, which is consumed.  -> (file names, (n, 4) int64 xywh, (n,) image ids)."""
    with open(path, "rt") as f:
        lines = [line.rstrip("\n") for line in f]
    while lines and not lines[-1].strip():
        lines.pop()
    names, boxes, ids = [], [], []
    i = 0
    while i < len(lines):
        name = lines[i].strip()
        if i + 1 >= len(lines):
            raise ValueError(f"{path}:{i + 1}: image {name!r} without a face count")
        try:
            n = int(lines[i + 1])
        except ValueError:
            raise ValueError(f"{path}:{i + 2}: expected a face count after {name!r}, got {lines[i + 1]!r}") from None
        if n < 0:
            raise ValueError(f"{path}:{i + 2}: negative face count")
        i += 2
        image_id = len(names)
        names.append(os.path.join(images_root, name))
        if n == 0:
            if i < len(lines):                        # the dummy line of the real file; a path never parses as numbers
                try:
                    vals = [int(v) for v in lines[i].split()]
                    if vals and not any(vals):
                        i += 1
                except ValueError:
                    pass
            continue
        if i + n > len(lines):
            raise ValueError(f"{path}: image {name!r} announces {n} faces, the file ends after {len(lines) - i}")
        for k in range(n):
            vals = [int(v) for v in lines[i + k].split()]
            if len(vals) < 4:
                raise ValueError(f"{path}:{i + k + 1}: expected at least four integers")
            boxes.append(vals[:4])
            ids.append(image_id)
        i += n
    return names, np.asarray(boxes, np.int64).reshape(-1, 4), np.asarray(ids, np.int64)


def coco_annotations(names, boxes, ids):
    """The reference's annotations.json (its addImage / addBBox)."""
    return {"images": [{"id": i, "file_name": n} for i, n in enumerate(names)],
            "categories": [{"id": 0, "name": "face"}],
            "annotations": [{"id": k, "image_id": int(ids[k]), "category_id": 0, "bbox": [int(v) for v in boxes[k]],
                             "iscrowd": 0, "area": float(boxes[k][2] * boxes[k][3])} for k in range(len(boxes))]}


def coco_detections(image_ids, boxes, scores):
    """The reference's detections.json (its addDetection)."""
    return [{"image_id": int(i), "category_id": 0, "bbox": [int(v) for v in b], "score": float(s)}
            for i, b, s in zip(image_ids, boxes, scores)]


def load_detections(path):
    with open(path, "rt") as f:
        rows = json.load(f)
    ids = np.asarray([r["image_id"] for r in rows], np.int64)
    boxes = np.asarray([r["bbox"] for r in rows], np.float64).reshape(-1, 4)
    scores = np.asarray([r["score"] for r in rows], np.float64)
    return ids, boxes, scores


def load_detector(args, dev):
    """The detector behind --model_type / --mt / --model, at the thresholds its model exposes."""
    synthetic = args.model == "synthetic"
    if synthetic:
        from ..workload import make_frames
    if args.model_type == "yolov5_face":
        size = tuple(args.input_size) if args.input_size else (640, 640)
        if synthetic:
            from ..workload import build_yolo_detector
            det = build_yolo_detector(dev, make_frames(4, dev), name=args.variant or "yolov5n", input_size=size)
            det.augment = bool(getattr(args, "augment", False))
            return det
        from ..modules.yolov5_face import attempt_load, inference_pytorch_model_yolov5_face
        from ..modules.yolov5_face.model import YOLOV5FaceModel
        net = attempt_load(args.model, dev, cfg=args.variant)
        return YOLOV5FaceModel(net, 0.4, 0.0, inference_pytorch_model_yolov5_face, size, augment=getattr(args, "augment", False))
    if args.input_size:
        raise ValueError("--is applies to yolov5_face only")
    if args.model_type == "blazeface":
        variant = args.variant or "back"
        if synthetic:
            if variant != "back":
                raise ValueError("synthetic BlazeFace weights exist for the back model only")
            from ..workload import build_detector
            return build_detector(dev, make_frames(8, dev, seed=8))
        from ..modules.blazeface.model import BlazeFaceModel
        return BlazeFaceModel(args.model, 0.0, 0.0, variant, str(dev))
    if args.model_type == "mtcnn":
        from ..detect_face_mtcnn import load_model
        image = make_frames(1, dev, h=160, w=224)[0].cpu().numpy() if synthetic else None
        return load_model(args.variant or "fast", args.model, 0.0, 0.0, str(dev), image)
    raise ValueError(f"unknown model type {args.model_type}")


def read_frames(paths, dev):
    """The files as a list of (h, w, 3) u8 BGR device tensors: JPEGs through decode_jpeg_batch, anything else through imread."""
    from ..modules.utils.jpeg import JpegUnsupported, decode_jpeg_batch, imread
    datas = []
    for p in paths:
        with open(p, "rb") as f:
            datas.append(f.read())
    if all(d[:2] == b"\xff\xd8" for d in datas):
        try:
            return decode_jpeg_batch(datas, dev)
        except JpegUnsupported as e:       # a JPEG flavour the device decoder does not take; a damaged file still raises
            print(f"[WARNING] {e}: reading this batch of {len(paths)} files one by one through imread")
    return [imread(p, dev) for p in paths]


def run_detector(det, names, dev, batch, evaluator):
    """Detector over all images, batch by batch; every batch's boxes go to the evaluator without a host synchronisation.
    -> number of frames whose detections were cut at the detector's cap."""
    from ..frames import RaggedFrames
    over = torch.zeros((), dtype=torch.int64, device=dev)
    for b0 in range(0, len(names), batch):
        paths = names[b0:b0 + batch]
        frames = RaggedFrames.from_list(read_frames(paths, dev), dev)
        out = det.raw_batch(frames)
        dets, counts = out[0], out[1]
        if len(out) > 2:
            over += (out[2] != 0).sum()
        boxes, scores, valid = dets_to_frame_boxes(det, dets, counts, frames.sizes)
        wh = torch.tensor([[w, h] for h, w in frames.sizes], dtype=torch.int64, device=dev)[:, None, :]
        xywh = clamp_boxes_xywh(boxes, wh)
        ids = (b0 + torch.arange(len(paths), device=dev))[:, None].expand(valid.shape)
        evaluator.add(ids.reshape(-1), xywh.reshape(-1, 4), scores.reshape(-1), valid.reshape(-1))
    return int(over)


def main(argv=None):
    parser = argparse.ArgumentParser(description="Evaluate face detectors with the COCO bbox metrics (MI355X HIP path)")
    parser.add_argument("ann", help="Text file with WIDER-style ground truth (wider_face_val_bbx_gt.txt).")
    parser.add_argument("pics", help="Images root directory.")
    parser.add_argument("--model_type", default="yolov5_face", choices=["blazeface", "yolov5_face", "mtcnn"],
                        help="Detector family (default: %(default)s).")
    parser.add_argument("--mt", dest="variant", default=None,
                        help="Variant: back / front (blazeface), fast / slow (mtcnn), yolov5n / yolov5n-0.5 / yolov5s (yolov5_face; "
                             "default: from the weight file's name).")
    parser.add_argument("--model", default=None, help="Path to the weights, or 'synthetic'.")
    parser.add_argument("--is", "--input_size", dest="input_size", nargs=2, type=int, default=None, metavar=("W", "H"),
                        help="Model input size, yolov5_face only (default: 640 640).")
    parser.add_argument("-d", "--device", default="hip", help="hip[:N] / cuda[:N]; cpu (numpy path) with --dets, which is also taken when no HIP device "
                                                            "is present (default: %(default)s).")
    parser.add_argument("--batch", type=int, default=32, help="Frames per detector call (default: %(default)s).")
    parser.add_argument("--dets", default=None, help="Score this COCO-format detections.json instead of running a detector.")
    parser.add_argument("--out", default=".", help="Directory for annotations.json (written in --dets mode too) and detections.json "
                                                  "(default: %(default)s).")
    parser.add_argument("--augment", action="store_true",
                        help="yolov5_face only: augmented inference (the image, mirrored at scale 0.83, at scale 0.67; one NMS).")
    add_tile_args(parser)
    args = parser.parse_args(argv)
    if args.batch < 1:
        parser.error("--batch must be positive")
    if args.augment and args.model_type != "yolov5_face":
        parser.error(f"--augment applies to yolov5_face only: {args.model_type} has no augmented inference "
                     "(BlazeFace has a fixed input, MTCNN its own pyramid)")

    names, gt_boxes, gt_ids = parse_wider(args.ann, args.pics)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "annotations.json"), "wt") as f:
        json.dump(coco_annotations(names, gt_boxes, gt_ids), f)
    device = None if args.device == "cpu" else torch.device(args.device.replace("hip", "cuda"))
    if args.dets is not None and device is not None and not torch.cuda.is_available():
        print("[WARNING] no HIP device: scoring the detection file with the numpy path")
        device = None

    if args.dets is not None:
        ids, boxes, scores = load_detections(args.dets)
        result = coco_eval_bbox(gt_boxes, gt_ids, boxes, scores, ids, len(names), device=device)
    else:
        if device is None:
            raise NotImplementedError("the detectors have no CPU path: use -d hip, or --dets with -d cpu")
        if args.model is None:
            parser.error("--model is required unless --dets is given")
        try:
            det = wrap_from_args(load_detector(args, device), args, parser.error)
        except ValueError as e:          # MTCNN under --tile, a bad tile / overlap
            parser.error(str(e))
        evaluator = DetectionEvaluator(len(names), device).set_ground_truth(gt_boxes, gt_ids)
        cut = run_detector(det, names, device, args.batch, evaluator)
        if cut:
            print(f"[WARNING] {cut} images had more detections than the detector's cap; the lowest-scored were dropped")
        ids, boxes, scores = (t.cpu().numpy() for t in evaluator.detections())
        with open(os.path.join(args.out, "detections.json"), "wt") as f:
            json.dump(coco_detections(ids, boxes.astype(np.int64), scores), f)
        result = evaluator.evaluate()
    print(result.summary())
    return result


if __name__ == "__main__":
    main()
