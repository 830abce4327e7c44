"""Detector evaluation (evaluation.coco_eval_bbox) on a synthetic set shaped like WIDER val: 3 226 images, ground-truth
counts per image from a heavy-tailed distribution (most images a handful, a few up to ~1 500), 100 detections per image.

Times the device path with device events -- the torch plumbing (sorts, CSR offsets), fp_det_match, fp_pr_accumulate and
the three together -- after a warm-up, `--rounds` rounds of enough calls to last `--round-s` seconds each, the median
round with its spread; then runs the numpy path ONCE on the same data (wall clock) and checks that both agree.  The
comparison is against this project's own numpy restatement, not against pycocotools, which is not installed and which
nobody here has timed.  Prints one JSON line.

  python tools/deteval_bench.py [--images 3226] [--dets 100] [--rounds 5] [--round-s 0.25] [--no-numpy]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from face_detection_and_recognition_amd import evaluation as E  # noqa: E402


def wider_like(n_images, dets_per_image, seed=0):
    rng = np.random.default_rng(seed)
    n_gt = np.minimum(np.maximum(rng.pareto(1.1, n_images) * 3.0, 1.0), 1500.0).astype(np.int64)   # median 2, tail to 1 500
    n_gt[rng.integers(n_images)] = 1500
    gi = np.repeat(np.arange(n_images), n_gt)
    side = np.exp(rng.uniform(np.log(6.0), np.log(300.0), len(gi)))
    gt = np.stack([rng.uniform(0, 1024 - 6, len(gi)), rng.uniform(0, 768 - 6, len(gi)), side, side * rng.uniform(1.0, 1.4, len(gi))], 1)
    di = np.repeat(np.arange(n_images), dets_per_image)
    dt = np.empty((len(di), 4))
    start = np.concatenate([[0], np.cumsum(n_gt)])
    pick = start[di] + (rng.random(len(di)) * n_gt[di]).astype(np.int64)              # a jittered copy of one of the image's GTs
    dt[:, 2:] = gt[pick, 2:] * rng.uniform(0.85, 1.15, (len(di), 2))
    dt[:, :2] = gt[pick, :2] + gt[pick, 2:] * rng.uniform(-0.1, 0.1, (len(di), 2))
    noise = rng.random(len(di)) < 0.3
    dt[noise, :2] = rng.uniform(0, 900, (int(noise.sum()), 2))
    return gt, gi, dt, rng.random(len(di)), di


def timed(fn, reps, dev):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(torch.cuda.current_stream(dev))
    for _ in range(reps):
        fn()
    e.record(torch.cuda.current_stream(dev))
    e.synchronize()
    return s.elapsed_time(e) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=3226)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--round-s", type=float, default=0.25)
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("deteval_bench.py measures on the GPU; none is available")
    dev = torch.device("cuda:0")
    gt, gi, dt, sc, di = wider_like(a.images, a.dets)
    params = E._params(None, None, E.DEFAULT_MAX_DETS, None)
    t = [torch.from_numpy(x).to(dev) for x in (gt, gi, gt[:, 2] * gt[:, 3], dt, sc, di)]
    ev = E._DeviceEval(*params, a.images, dev)

    def total():
        ev.prepare(*t)
        ev.match()
        ev.accumulate()
    variants = {"plumbing": lambda: ev.prepare(*t), "match": ev.match, "accumulate": ev.accumulate, "total": total}
    total()
    torch.cuda.synchronize()
    reps = {}
    for name, fn in variants.items():
        fn()
        torch.cuda.synchronize()
        reps[name] = max(1, math.ceil(a.round_s * 1e3 / max(timed(fn, 2, dev), 1e-3)))
    times = {name: [] for name in variants}
    for _ in range(a.rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn, reps[name], dev))
    out = dict(bench="deteval", images=a.images, gts=int(len(gi)), max_gts_per_image=int(np.bincount(gi).max()),
               detections=int(len(di)), curves=ev.T * ev.A * ev.M)
    for name, v in times.items():
        out[name] = dict(ms=round(float(np.median(v)), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4),
                         calls_per_round=reps[name])
    res = ev.result()
    out["stats_device"] = [round(float(v), 6) for v in res.stats]
    if not a.no_numpy:
        t0 = time.perf_counter()
        ref = E.coco_eval_bbox(gt, gi, dt, sc, di, a.images)
        out["numpy_once_s"] = round(time.perf_counter() - t0, 2)
        out["numpy_over_device_total"] = round(out["numpy_once_s"] * 1e3 / out["total"]["ms"], 1)
        out["flags_equal"] = bool(np.array_equal(ref.matched, res.matched) and np.array_equal(ref.ignored, res.ignored))
        out["precision_bit_equal"] = bool(np.array_equal(ref.precision.view(np.int64), res.precision.view(np.int64))
                                          and np.array_equal(ref.recall.view(np.int64), res.recall.view(np.int64)))
        out["compared_against"] = "this project's numpy restatement (evaluation.py), not pycocotools"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
