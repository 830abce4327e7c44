"""Drawing the detections on a batch (annotate.draw, fp_draw) on the SURVEY §8(d) workload: `--frames` synthetic frames of
576 x 1024 (workload.make_frames), two faces a frame (seeded boxes with sides of a quarter to a half of the frame height, the
size of the workload's patches, five landmark points each), the reference's layout (annotate.face_draw_list), without and with
anonymize = 16.  Next to it the time of encode_jpeg_batch on the same frames: saving an annotated batch is draw + encode.

Timed with device events: draw `--iters` calls in a row per round (the list is finished and on the device; in-place drawing
costs the same on already drawn frames), the encoder one call per round; `--rounds` rounds, the median is reported with
min .. max.  Prints one JSON line.

  python tools/annotate_bench.py [--frames 256] [--iters 20] [--rounds 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from face_detection_and_recognition_amd import _lib as L  # noqa: E402
from face_detection_and_recognition_amd import annotate as A  # noqa: E402
from face_detection_and_recognition_amd import workload as W  # noqa: E402
from face_detection_and_recognition_amd.modules.utils import jpeg as J  # noqa: E402


def synthetic_faces(B, h, w, per_frame=2, seed=5):
    """(info (n, 7), lmarks (n, 10)) float32 host arrays: per_frame square boxes a frame, five points inside each."""
    rng = np.random.default_rng(seed)
    info, lm = [], []
    for f in range(B):
        for _ in range(per_frame):
            side = int(rng.integers(h // 4, h // 2))
            x, y = int(rng.integers(0, w - side)), int(rng.integers(0, h - side))
            info.append([f, x, y, x + side, y + side, rng.uniform(0.7, 1.0), side * side / (h * w)])
            lm.append((np.array([x, y] * 5) + rng.uniform(0.2, 0.8, 10) * side).round())
    return np.array(info, np.float32), np.array(lm, np.float32)


def timed(fn, reps, dev):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(torch.cuda.current_stream(dev))
    for _ in range(reps):
        fn()
    e.record(torch.cuda.current_stream(dev))
    e.synchronize()
    return s.elapsed_time(e) / reps


def summary(ts):
    return dict(median=round(statistics.median(ts), 3), min=round(min(ts), 3), max=round(max(ts), 3))


def tile_bytes(tiles, h, w):
    """Bytes of the listed tiles (the kernel loads and stores each once)."""
    T = L.DRAW_TILE
    return int(sum(min(T, w - tx * T) * min(T, h - ty * T) * 3 for _, tx, ty in tiles.tolist()))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    B, h, w = args.frames, W.FRAME_H, W.FRAME_W
    frames = W.make_frames(B, dev, seed=99)
    info, lm = synthetic_faces(B, h, w)
    info_d = torch.from_numpy(info).to(dev)
    out = dict(bench="annotate", frames=B, h=h, w=w, faces=len(info), frame_bytes=B * h * w * 3, configs=[])
    for cell in (0, 16):
        t0 = time.perf_counter()
        dl = A.face_draw_list(info_d, len(info), [(h, w)] * B, lmarks=lm, anonymize=cell)
        cmds, _, tiles = dl.host()
        dl.finish(dev)
        build_ms = (time.perf_counter() - t0) * 1e3
        work = frames.clone()
        A.draw(work, dl)                                    # warm-up: code object, font upload
        torch.cuda.synchronize()
        us = [timed(lambda: A.draw(work, dl), args.iters, dev) * 1e3 for _ in range(args.rounds)]
        tb = tile_bytes(tiles, h, w)
        med = statistics.median(us)
        out["configs"].append(dict(anonymize=cell, commands=len(cmds), tiles=len(tiles), tile_bytes=tb,
                                   tile_share_of_frames=round(tb / out["frame_bytes"], 4), list_build_ms=round(build_ms, 2),
                                   draw_us=summary(us), gb_per_s=round(2 * tb / med / 1e3, 1)))
        del work
    imgs = [frames[i] for i in range(B)]
    J.encode_jpeg_batch(imgs)                               # warm-up
    torch.cuda.synchronize()
    enc = []
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        files = J.encode_jpeg_batch(imgs)                   # returns host bytes: the call ends synchronised
        enc.append((time.perf_counter() - t0) * 1e3)
    out["encode_jpeg_batch_ms"] = summary(enc)
    out["jpeg_bytes"] = int(sum(len(f) for f in files))
    for c in out["configs"]:
        c["draw_over_encode"] = round(c["draw_us"]["median"] / 1e3 / out["encode_jpeg_batch_ms"]["median"], 5)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
