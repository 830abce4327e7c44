"""Augmented inference of YOLOv5-face (Model.run_views) taken apart, on the same run, with synthetic weights and frames:
YOLOv5n-face at 640 x 640, batch 64 and -- if the three arenas fit -- batch 256, frames of 576 x 1024.

Per batch, milliseconds per call (device events, `--iters` calls in a row per round, `--rounds` rounds, augment off and on
alternating within every round; median with min .. max):
  plain_ms         YOLOV5FaceModel(augment=False).raw_batch  -- the u8-fused stem, 25 200 rows per image through NMS
  augment_ms       YOLOV5FaceModel(augment=True).raw_batch   -- fp32 canvas, three plans, 55 755 rows per image through NMS
  ratio            augment_ms / plain_ms, beside the arithmetic ratio of the forward passes (640^2 + 544^2 + 448^2) / 640^2 = 2.21
  views_ms         fp_tta_views alone, with its byte floor (canvas read once + both views written once) at COPY_TBPS
  decode_ms        the nine fp_yolo_decode_view launches of the three views
  nms_plain_ms, nms_augment_ms   nms_face_device on 25 200 / on 55 755 rows per image
  plan_bytes       the arenas of the three plans
No pass / fail threshold.  Prints one JSON line.

  python tools/tta_bench.py [--batches 64 256] [--iters 5] [--rounds 5] [--small]

--small: YOLOv5n-0.5, 128 x 128 input, 2 frames of 96 x 160, 1 iteration, 2 rounds."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_TBPS = 5.3       # the copy rate tools/lab/copy_bw.py measured (profiles/r03_copy_bw2.log), read + write


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    return ap


def views_floor_bytes(n, h, w):
    """What fp_tta_views must move: the 16-byte pixels of the canvas read once and of both views written once."""
    from face_detection_and_recognition_amd.modules.yolov5_face.tta import tta_views
    return n * 16 * sum(v[3][0] * v[3][1] for v in tta_views(h, w))


def forward_ratio(h, w):
    """Pixels of the three network inputs over the pixels of the first."""
    from face_detection_and_recognition_amd.modules.yolov5_face.tta import tta_views
    return sum(v[3][0] * v[3][1] for v in tta_views(h, w)) / (h * w)


def summary(ts):
    return dict(median=round(statistics.median(ts), 4), min=round(min(ts), 4), max=round(max(ts), 4))


def measure(det_plain, det_aug, frames, args, dev):
    import torch
    from face_detection_and_recognition_amd.modules.yolov5_face import nms_face_device, preprocess_batch, tta

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(torch.cuda.current_stream(dev))
        for _ in range(args.iters):
            fn()
        e.record(torch.cuda.current_stream(dev))
        e.synchronize()
        return s.elapsed_time(e) / args.iters

    net = det_aug.net
    B = frames.shape[0]
    iw, ih = det_aug.input_size
    det_aug.raw_batch(frames)
    plans = net.last_view_plans
    z_aug = net.run_views(plans[0], "mapped").clone()
    z_plain = z_aug[:, :plans[0].n_rows].contiguous()
    views = tta.tta_views(ih, iw)
    det = net.model[-1]

    def decodes():
        row = 0
        for p, (ratio, flip, _, _) in zip(plans, views):
            row = tta.decode_view(det, p.heads, net._tta_z[1], row, ratio, flip, iw, "mapped")

    calls = dict(plain_ms=lambda: det_plain.raw_batch(frames), augment_ms=lambda: det_aug.raw_batch(frames),
                 views_ms=lambda: tta.fill_views(plans[0].input, plans[1].input, plans[2].input), decode_ms=decodes,
                 nms_plain_ms=lambda: nms_face_device(z_plain, 0.4, 0.5), nms_augment_ms=lambda: nms_face_device(z_aug, 0.4, 0.5))
    for fn in calls.values():           # warm-up: code objects, plans, the allocator's blocks
        fn()
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in calls}
    for _ in range(args.rounds):        # every round times every call once: plain and augmented alternate
        for k, fn in calls.items():
            ts[k].append(timed(fn))
    rec = dict(batch=B, input=[ih, iw], frame=[int(frames.shape[1]), int(frames.shape[2])], rows=[p.n_rows for p in plans],
               plan_bytes=[int(p.arena.numel() * 4) for p in plans], **{k: summary(v) for k, v in ts.items()})
    med = lambda k: rec[k]["median"]      # noqa: E731
    floor = views_floor_bytes(B, ih, iw)
    out_p, cnt_p, _ = det_plain.raw_batch(frames)
    out_a, cnt_a, over_a = det_aug.raw_batch(frames)
    rec.update(ratio=round(med("augment_ms") / med("plain_ms"), 3), forward_pixel_ratio=round(forward_ratio(ih, iw), 3),
               views_floor_bytes=floor, views_floor_ms=round(floor / (COPY_TBPS * 1e12) * 1e3, 4),
               views_over_floor=round(med("views_ms") / (floor / (COPY_TBPS * 1e12) * 1e3), 2),
               nms_ratio=round(med("nms_augment_ms") / med("nms_plain_ms"), 3),
               kept_plain=int(cnt_p.sum().item()), kept_augment=int(cnt_a.sum().item()), flagged_augment=int((over_a != 0).sum().item()))
    return rec


def main(argv=None):
    args = build_parser().parse_args(argv)
    import torch
    from face_detection_and_recognition_amd import workload as W
    from face_detection_and_recognition_amd.modules.yolov5_face import inference_pytorch_model_yolov5_face
    from face_detection_and_recognition_amd.modules.yolov5_face.model import YOLOV5FaceModel
    dev = torch.device("cuda:0")
    if args.small:
        args.iters, args.rounds, args.batches = 1, 2, [2]
        name, size, fh, fw, cand = "yolov5n-0.5", (128, 128), 96, 160, 20
    else:
        name, size, fh, fw, cand = "yolov5n", (640, 640), 576, 1024, 80
    det_plain = W.build_yolo_detector(dev, W.make_frames(4, dev, seed=6, h=fh, w=fw), name, cand_per_frame=cand, input_size=size)
    det_aug = YOLOV5FaceModel(det_plain.net, det_plain.det_thres, det_plain.bbox_area_thres, inference_pytorch_model_yolov5_face,
                              size, augment=True)
    out = dict(bench="tta", small=bool(args.small), model=name, iters=args.iters, rounds=args.rounds, copy_tbps=COPY_TBPS, batches=[])
    for b in args.batches:
        try:
            out["batches"].append(measure(det_plain, det_aug, W.make_frames(b, dev, seed=7, h=fh, w=fw), args, dev))
        except torch.cuda.OutOfMemoryError as e:            # the three arenas did not fit: say so, do not fall back
            out["batches"].append(dict(batch=b, skipped=f"out of device memory: {str(e).splitlines()[0]}"))
            torch.cuda.empty_cache()
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
