"""``python -m face_detection_and_recognition_amd.eval.eval_face_tracker data/ --tracks hyp/`` or
``... data/ --model synthetic --max_age 30 [--motion STD_POS STD_VEL] [--reid TAU LOST_AGE] [--sweep max_age=5,15,30] [--hota [--alphas a,b,...]]``

Scores a face tracker on labelled video with CLEAR-MOT (MOTA, MOTP, IDSW, Frag, MT / PT / ML) and the identity measures
(IDF1, IDP, IDR): tracking_eval.py, the kernel of csrc/moteval.hip on a HIP device, numpy with ``-d cpu``; DESIGN.md
section 7 "Tracker evaluation".  Build-defined: the reference calls no tracking scorer; parity with TrackEval /
py-motmetrics is unpinned.

``data`` is a folder of sequences, each a folder with ``gt.txt`` (MOTChallenge rows ``frame,id,x,y,w,h,...``, frames 1-based)
and ``frames/*.jpg`` (sorted by name = video order) or, in place of that folder, ``video.avi`` (Motion-JPEG,
modules/utils/video.py).  The hypotheses are either

  * ``--tracks DIR``: ``DIR/<sequence>.txt`` in the same format (a sequence without a file has no hypotheses), or
  * a model plus ``--max_age`` (and ``--tau_near / --tau_far / --iou_min``): FacePipeline(tracker=StreamTracker) runs over the
    frames, one stream per sequence, and every step's rows go to a TrackingEvaluator on the device.

``--motion STD_POS STD_VEL`` turns the tracker's constant-velocity prediction on (tracking.ConstantVelocity; DESIGN section 7
"Tracklets: motion prediction"): no defaults, nothing has been measured; DeepSORT publishes 0.05 and 0.00625.
``--reid TAU LOST_AGE`` turns re-identification on (tracking.LostPool; DESIGN section 7 "Tracklets: re-identification"): an
ended track is remembered for LOST_AGE frames (an integer > max_age) and a returning face whose cosine to its last embedding
exceeds TAU continues it; no defaults, nothing has been measured on real video.
``--sweep key=v1,v2,...`` (key: max_age, tau_near, tau_far, iou_min, with --motion std_pos / std_vel, with --reid tau_reid /
lost_age) repeats the run per
value and prints one combined row each.  Prints the table (one line per sequence and the combined line) and returns the result
(a list of (value, result) under --sweep).  The thresholds' defaults are the reference's numbers restated as cosines; max_age
has no default.

``--hota`` appends HOTA, DetA, AssA, DetRe, DetPr, AssRe, AssPr and LocA (tracking_eval.hota_eval, csrc/hota.hip; DESIGN section 7
"Tracker evaluation: HOTA") to every row, the means over ``--alphas`` (default 0.05 .. 0.95); the result then carries the
HotaResult as ``result.hota``.  Without the flag the output is what it was.
"""
import argparse
import glob
import os

import numpy as np

from ..tracking import IOU_MIN, TAU_FAR, TAU_NEAR
from ..tracking_eval import TrackingEvaluator, hota_eval, mot_eval, read_mot_txt

SWEEP_KEYS = dict(max_age=int, tau_near=float, tau_far=float, iou_min=float, std_pos=float, std_vel=float, tau_reid=float,
                  lost_age=int)


def load_sequences(root):
    """-> list of dict(name, gt (read_mot_txt), frames (sorted .jpg paths, or a VideoReader over video.avi), n_frames) for every
    folder of root with a gt.txt.
    n_frames is the number of .jpg files, or without a frames folder the last labelled frame + 1."""
    seqs = []
    for name in sorted(os.listdir(root)):
        gt_path = os.path.join(root, name, "gt.txt")
        if not os.path.isfile(gt_path):
            continue
        gt = read_mot_txt(gt_path)
        frames = sorted(glob.glob(os.path.join(root, name, "frames", "*.jpg")))
        video = os.path.join(root, name, "video.avi")
        if not frames and os.path.isfile(video):          # a Motion-JPEG file in place of the frames folder
            from ..modules.utils.video import VideoReader
            frames = VideoReader(video)
        n_frames = len(frames) if frames else (int(gt["frame"].max()) + 1 if len(gt["frame"]) else 0)
        if len(gt["frame"]) and (gt["frame"].min() < 0 or gt["frame"].max() >= n_frames):
            raise ValueError(f"{gt_path}: frame numbers outside 1 .. {n_frames}")
        seqs.append(dict(name=name, gt=gt, frames=frames, n_frames=n_frames))
    if not seqs:
        raise ValueError(f"no sequence (a folder with gt.txt) under {root}")
    return seqs


def close_sequences(seqs):
    """Closes the video files load_sequences opened."""
    for s in seqs:
        if hasattr(s["frames"], "close"):
            s["frames"].close()


def stack_rows(per_seq):
    """A list of read_mot_txt dicts (None: no rows), one per sequence -> (seq, frame, id, boxes) arrays."""
    seq, frame, ids, boxes = [], [], [], []
    for s, rows in enumerate(per_seq):
        if rows is None:
            continue
        seq.append(np.full(len(rows["frame"]), s, np.int64))
        frame.append(rows["frame"])
        ids.append(rows["id"])
        boxes.append(rows["boxes"])
    if not seq:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 4))
    return np.concatenate(seq), np.concatenate(frame), np.concatenate(ids), np.concatenate(boxes)


def ground_truth(seqs):
    return stack_rows([s["gt"] for s in seqs]) + (np.array([s["n_frames"] for s in seqs], np.int64),)


def score_tracks(seqs, tracks_dir, thr, device, hota=False, alphas=None):
    hyp = []
    for s in seqs:
        path = os.path.join(tracks_dir, s["name"] + ".txt")
        hyp.append(read_mot_txt(path) if os.path.isfile(path) else None)
        if hyp[-1] is not None and len(hyp[-1]["frame"]) and hyp[-1]["frame"].max() >= s["n_frames"]:
            s["n_frames"] = int(hyp[-1]["frame"].max()) + 1 if not s["frames"] else s["n_frames"]
    gt = ground_truth(seqs)
    rows = stack_rows(hyp)
    result = mot_eval(*gt[:4], *rows, gt[4], thr=thr, device=device)
    if hota:
        result.hota = hota_eval(*gt[:4], *rows, gt[4], alphas=alphas, device=device)
    return result


def build_parts(seqs, args, dev):
    """(detector, embedder) on the synthetic weights, the detector's scores calibrated on the first frames; built once per
    sweep."""
    from .. import workload as W
    from ..modules.utils.video import read_frames
    if args.model != "synthetic":
        raise ValueError("only --model synthetic is wired here; build a FacePipeline(..., tracker=StreamTracker(...)) for real "
                         "weights and feed a TrackingEvaluator from its steps")
    first = next((s["frames"] for s in seqs if s["frames"]), None)
    if first is None:
        raise ValueError("no frames/*.jpg in any sequence: nothing to run the tracker on (use --tracks)")
    return W.build_detector(dev, read_frames(first, 0, 8, dev), cand_per_frame=48), W.build_embedder(dev)


def run_tracker(seqs, args, dev, parts):
    """The pipeline over every sequence's frames, batch by batch, one stream per sequence -> MotResult."""
    import torch
    from ..modules.utils.video import read_frames
    from ..pipeline import FacePipeline
    from ..tracking import ConstantVelocity, LostPool, StreamTracker
    det, emb = parts
    motion = None if args.motion is None else ConstantVelocity(*args.motion)
    tracker = StreamTracker(len(seqs), emb.embedding_size, args.max_age, args.tau_near, args.tau_far, args.iou_min, device=dev,
                            motion=motion, reid=None if args.reid is None else LostPool(*args.reid))
    pipe = FacePipeline(det, emb, None, tracker=tracker)
    ev = TrackingEvaluator(len(seqs), dev, thr=args.thr).set_ground_truth(*ground_truth(seqs))
    for s, seq in enumerate(seqs):
        for lo in range(0, len(seq["frames"]), args.batch_size):
            try:
                frames = read_frames(seq["frames"], lo, lo + args.batch_size, dev)
            except ValueError as e:
                raise ValueError(f"{seq['name']}: {e}") from None
            B = int(frames.shape[0])
            res = pipe.step(frames, streams=[s] * B)
            n, info = res["n_faces"], res["info"]
            ev.add(torch.full((B,), s, dtype=torch.int64), lo, info[:n, 0].to(torch.int32), info[:n, 1:5], res["track_id"][:n])
    result = ev.evaluate()
    if args.hota:
        result.hota = ev.evaluate_hota(args.alphas)
    if ev.dropped:
        print(f"[WARNING] {ev.dropped} face rows carried no track id (FULL, OVER or dead rows) and were not scored")
    return result


def table(result, names):
    """The lines of result.summary(names), each with the HOTA columns behind it when the result carries a HotaResult."""
    lines = result.summary(names).splitlines()
    hota = result.__dict__.get("hota")
    return lines if hota is None else [ln + col for ln, col in zip(lines, hota.columns())]


def parse_alphas(text):
    try:
        return [float(v) for v in text.split(",")]
    except ValueError:
        raise ValueError("--alphas takes a,b,...: ascending thresholds inside (0, 1]") from None


def parse_sweep(text):
    key, _, values = text.partition("=")
    if key not in SWEEP_KEYS or not values:
        raise ValueError(f"--sweep takes key=v1,v2,... with key one of {sorted(SWEEP_KEYS)}")
    return key, [SWEEP_KEYS[key](v) for v in values.split(",")]


def main(argv=None):
    import torch
    parser = argparse.ArgumentParser(description="Evaluate face trackers with CLEAR-MOT and IDF1 (MI355X HIP path)")
    parser.add_argument("data", help="Folder of sequences: <sequence>/gt.txt and <sequence>/frames/*.jpg (or <sequence>/video.avi, Motion-JPEG).")
    parser.add_argument("--tracks", default=None, help="Folder of hypothesis files <sequence>.txt; no tracker is run.")
    parser.add_argument("--model", default=None, help="'synthetic' (seeded random weights); trained weights: use the API.")
    parser.add_argument("--max_age", type=int, default=None, help="Required with --model unless swept: nothing has been measured.")
    parser.add_argument("--tau_near", type=float, default=TAU_NEAR)
    parser.add_argument("--tau_far", type=float, default=TAU_FAR)
    parser.add_argument("--iou_min", type=float, default=IOU_MIN)
    parser.add_argument("--motion", type=float, nargs=2, default=None, metavar=("STD_POS", "STD_VEL"),
                        help="Constant-velocity prediction for the IoU gate: noise as fractions of the box height (no defaults).")
    parser.add_argument("--reid", type=float, nargs=2, default=None, metavar=("TAU", "LOST_AGE"),
                        help="Re-identification of ended tracks: the cosine a returning face must exceed and the frames a track is "
                             "remembered, an integer > max_age (no defaults).")
    parser.add_argument("--sweep", default=None, help="key=v1,v2,...: repeat the run per value of max_age / tau_near / tau_far / iou_min "
                                                      "/ std_pos / std_vel (with --motion) / tau_reid / lost_age (with --reid).")
    parser.add_argument("--thr", type=float, default=0.5, help="IoU threshold of a match (default: %(default)s).")
    parser.add_argument("--hota", action="store_true", help="Append HOTA, DetA, AssA, DetRe, DetPr, AssRe, AssPr, LocA to every row.")
    parser.add_argument("--alphas", default=None, help="a,b,...: HOTA's localisation thresholds, ascending inside (0, 1] "
                                                       "(default: 0.05 .. 0.95); with --hota.")
    parser.add_argument("-b", "--batch_size", type=int, default=256)
    parser.add_argument("-d", "--device", default="hip", help="hip[:N] / cuda[:N]; cpu (numpy path) with --tracks (default: %(default)s).")
    args = parser.parse_args(argv)
    if (args.tracks is None) == (args.model is None):
        parser.error("give either --tracks DIR or --model")
    if args.batch_size < 1:
        parser.error("--batch_size must be positive")
    if args.alphas is not None:
        if not args.hota:
            parser.error("--alphas belongs to --hota")
        try:
            args.alphas = parse_alphas(args.alphas)
        except ValueError as e:
            parser.error(str(e))
    device = None if args.device == "cpu" else torch.device(args.device.replace("hip", "cuda"))
    seqs = load_sequences(args.data)
    try:
        names = [s["name"] for s in seqs]
        if args.tracks is not None:
            if args.sweep:
                parser.error("--sweep needs a tracker to run: use --model")
            if device is not None and not torch.cuda.is_available():
                print("[WARNING] no HIP device: scoring the track files with the numpy path")
                device = None
            result = score_tracks(seqs, args.tracks, args.thr, device, args.hota, args.alphas)
            print("\n".join(table(result, names)))
            return result
        if device is None:
            raise NotImplementedError("the pipeline has no CPU path: use -d hip, or --tracks with -d cpu")
        try:
            key, values = parse_sweep(args.sweep) if args.sweep else (None, [None])
        except ValueError as e:
            parser.error(str(e))
        if args.max_age is None and key != "max_age":
            parser.error("--max_age is required (it has no default: nothing has been measured)")
        if key in ("std_pos", "std_vel") and args.motion is None:
            parser.error(f"--sweep {key}= needs --motion STD_POS STD_VEL for the value that is not swept")
        if key in ("tau_reid", "lost_age") and args.reid is None:
            parser.error(f"--sweep {key}= needs --reid TAU LOST_AGE for the value that is not swept")
        results, parts = [], build_parts(seqs, args, device)
        for v in values:
            if key in ("std_pos", "std_vel"):
                args.motion[("std_pos", "std_vel").index(key)] = v
            elif key in ("tau_reid", "lost_age"):
                args.reid[("tau_reid", "lost_age").index(key)] = v
            elif key is not None:
                setattr(args, key, v)
            result = run_tracker(seqs, args, device, parts)
            results.append((v, result))
            lines = table(result, names)
            if key is None:
                print("\n".join(lines))
            else:
                if len(results) == 1:
                    print(f"{key:<10}" + lines[0])
                print(f"{v!s:<10}" + lines[-1])
        return results[0][1] if key is None else results
    finally:
        close_sequences(seqs)


if __name__ == "__main__":
    main()
