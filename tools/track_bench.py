"""The batched tracker (tracking.StreamTracker, fp_tracklets_step) next to the per-frame port of the reference's rule
(face_extraction/face_tracker.py FaceTracker.track, fp_tracker_step), on the same rows in the same run, D = 512:

  a   256 streams x 1 frame, 2 faces each          (256 workgroups, one frame each)
  b   1 stream x 256 frames, 2 faces each          (one workgroup marches 256 frames)
  c   1 stream x 256 frames, 8 faces each, 32 identities taking turns: about 32 live tracks
  d   1 stream x 256 frames, two groups of 4 faces taking turns, max_age 0: every face leaves for max_age + 1 frames and
      returns.  Without a pool every frame opens 4 tracks; with one every frame parks 4 and runs step 3b, which revives 4.

Per layout, milliseconds per step of 256 frames: tracklets_ms (one launch, fp_row_inv_norm included) and per_frame_ms (the
same rows through FaceTracker.track, one call per frame -- layout a: one FaceTracker per stream), and their ratio.  The two
apply different rules (greedy one-to-one with expiry against first match); the comparison is of cost, not of answers.
The motion leg: per layout a second StreamTracker with motion=ConstantVelocity (fp_tracklets_step_motion) on the same rows,
timed in the same process in rounds that alternate with the plain tracker's: motion_off_ms, motion_on_ms and
motion_cost_us_per_frame = their medians' difference over the frames one workgroup marches (1, 256, 256).
The reid leg, likewise: a StreamTracker with reid=LostPool (fp_tracklets_step_reid) on the same rows, alternated with the plain
one: reid_off_ms, reid_on_ms, reid_on_over_off and reid_cost_us_per_frame.  In layouts a to c nothing ever expires: the pool
stays empty and the leg prices the kernel with the pool compiled in; layout d prices parking and step 3b.
The templates leg (--templates only): a StreamTracker with templates=Templates() (fp_track_pool_step behind the tracker's launch)
on the same rows, alternated with the plain one: templates_off_ms, templates_on_ms, templates_cost_ms; and pool_ms, the two
launches of fp_track_pool_step alone on the rows and the ids of a finished step, beside its two yardsticks of the same run:
pool_over_tracklets (against tracklets_ms, the tracker's launch on the same rows) and pool_floor_bytes = 4 * n * D * 4 (emb read,
track_emb written, twice over for the state and the lists' slack) with pool_gbps = those bytes over pool_ms.  With --templates
the pipeline block gains the kind "templates".
Then the pipeline: FacePipeline.step on 256 synthetic frames without tracker=, with it, with a tracker with motion= and with one
with reid=, and
step_overlapped with two_streams (the tracker on the side stream) likewise.  Timed with device events after warm-up, `--iters` calls per round,
`--rounds` rounds; median with min .. max.  Prints one JSON line.  No pass / fail threshold.

  python tools/track_bench.py [--iters 10] [--rounds 5] [--small] [--no-pipeline] [--templates]

--small: 8 frames per layout, 1 iteration, 2 rounds."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from face_detection_and_recognition_amd import workload as W  # noqa: E402
from face_detection_and_recognition_amd.face_extraction.face_tracker import FaceTracker  # noqa: E402
from face_detection_and_recognition_amd.pipeline import FacePipeline  # noqa: E402
from face_detection_and_recognition_amd.tracking import REVIVED, ConstantVelocity, LostPool, StreamTracker, Templates  # noqa: E402

D = 512
REID = LostPool(0.6, 1 << 20)      # sightings of one identity have cosines of about 0.9, two identities of about 0
MOTION = ConstantVelocity(ConstantVelocity.DEEPSORT_STD_POS, ConstantVelocity.DEEPSORT_STD_VEL)   # the cost does not depend on them


def timed(fn, reps, dev):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(torch.cuda.current_stream(dev))
    for _ in range(reps):
        fn()
    e.record(torch.cuda.current_stream(dev))
    e.synchronize()
    return s.elapsed_time(e) / reps


def summary(ts):
    return dict(median=round(statistics.median(ts), 4), min=round(min(ts), 4), max=round(max(ts), 4))


def layout_rows(n_streams, n_frames, faces, n_ident, seed, dev):
    """Rows of one step: frame f of stream s shows `faces` of the stream's n_ident identities, taking turns; every sighting is
    the identity's unit vector plus noise at a cosine of about 0.95, its box the identity's cell."""
    rng = np.random.default_rng(seed)
    B = n_streams * n_frames
    ident = rng.standard_normal((n_streams, n_ident, D))
    ident /= np.linalg.norm(ident, axis=2, keepdims=True)
    frame, boxes, emb = [], [], []
    for f in range(B):
        s, t = f % n_streams, f // n_streams
        for j in range(faces):
            k = (t * faces + j) % n_ident
            noise = rng.standard_normal(D)
            frame.append(f)
            emb.append(ident[s, k] + 0.33 * noise / np.linalg.norm(noise))
            x, y = 100 * (k % 8), 100 * (k // 8)
            boxes.append([x, y, x + 60, y + 60])
    emb = np.asarray(emb, np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    to = lambda a, dt: torch.from_numpy(np.asarray(a, dt)).to(dev)      # noqa: E731
    return dict(frame=to(frame, np.int32), boxes=to(boxes, np.float32), emb=to(emb, np.float32),
                sof=to(np.arange(B) % n_streams, np.int32), B=B, faces=faces, n_streams=n_streams)


def measure_layout(name, rows, max_age, args, dev):
    tr = StreamTracker(rows["n_streams"], D, max_age, device=dev)
    step = lambda: tr.step(rows["frame"], rows["boxes"], rows["emb"], rows["sof"])     # noqa: E731
    olds = [FaceTracker("MOBILE_FACENET", D, dev, max_faces=64) for _ in range(rows["n_streams"])]
    ib = rows["boxes"].to(torch.int32)
    per = [(olds[f % rows["n_streams"]], rows["emb"][f * rows["faces"]:(f + 1) * rows["faces"]],
            ib[f * rows["faces"]:(f + 1) * rows["faces"]]) for f in range(rows["B"])]

    def loop():
        for t, e, b in per:
            t.track(e, b)
    out = step()
    step()
    loop()
    torch.cuda.synchronize()
    live = int((tr.state["slot_i"][:, :, 0] != 0).sum().item())
    rec = dict(name=name, streams=rows["n_streams"], frames=rows["B"], rows=int(rows["frame"].shape[0]), live_tracks=live,
               new_rows_first_step=int((out["track_flags"] & 1).ne(0).sum().item()))
    rec["tracklets_ms"] = summary([timed(step, args.iters, dev) for _ in range(args.rounds)])
    rec["per_frame_ms"] = summary([timed(loop, max(1, args.iters // 5), dev) for _ in range(args.rounds)])
    rec["per_frame_over_tracklets"] = round(rec["per_frame_ms"]["median"] / rec["tracklets_ms"]["median"], 2)
    trm = StreamTracker(rows["n_streams"], D, max_age, device=dev, motion=MOTION)
    mstep = lambda: trm.step(rows["frame"], rows["boxes"], rows["emb"], rows["sof"])   # noqa: E731
    mstep()
    mstep()
    torch.cuda.synchronize()
    off, on = [], []
    for _ in range(args.rounds):            # alternated: both see the same machine
        off.append(timed(step, args.iters, dev))
        on.append(timed(mstep, args.iters, dev))
    rec["motion_off_ms"], rec["motion_on_ms"] = summary(off), summary(on)
    rec["motion_cost_us_per_frame"] = round((rec["motion_on_ms"]["median"] - rec["motion_off_ms"]["median"]) * 1000.0
                                            / (rows["B"] // rows["n_streams"]), 3)
    trr = StreamTracker(rows["n_streams"], D, max_age, device=dev, reid=REID)
    rstep = lambda: trr.step(rows["frame"], rows["boxes"], rows["emb"], rows["sof"])   # noqa: E731
    rstep()
    rout = rstep()
    torch.cuda.synchronize()
    rec["revived_rows_second_step"] = int((rout["track_flags"] & REVIVED).ne(0).sum().item())
    rec["parked_tracks"] = int((trr.state["lost_i"][:, :, 0] != 0).sum().item())
    off, on = [], []
    for _ in range(args.rounds):
        off.append(timed(step, args.iters, dev))
        on.append(timed(rstep, args.iters, dev))
    rec["reid_off_ms"], rec["reid_on_ms"] = summary(off), summary(on)
    rec["reid_on_over_off"] = round(rec["reid_on_ms"]["median"] / rec["reid_off_ms"]["median"], 4)
    rec["reid_cost_us_per_frame"] = round((rec["reid_on_ms"]["median"] - rec["reid_off_ms"]["median"]) * 1000.0
                                          / (rows["B"] // rows["n_streams"]), 3)
    if args.templates:
        measure_templates(rec, rows, max_age, step, args, dev)
    return rec


def measure_templates(rec, rows, max_age, step, args, dev):
    """The templates leg of one layout (module docstring), written into rec."""
    import ctypes as C

    from face_detection_and_recognition_amd import _lib as L
    from face_detection_and_recognition_amd import tracking as T
    trt = StreamTracker(rows["n_streams"], D, max_age, device=dev, templates=Templates())
    tstep = lambda: trt.step(rows["frame"], rows["boxes"], rows["emb"], rows["sof"])   # noqa: E731
    tstep()
    tout = tstep()
    torch.cuda.synchronize()
    rec["template_entries"] = int((trt.state["tpl_i"][:, :, 0] != 0).sum().item())
    rec["template_rows_max"] = int(tout["track_emb_rows"].max().item())
    off, on = [], []
    for _ in range(args.rounds):
        off.append(timed(step, args.iters, dev))
        on.append(timed(tstep, args.iters, dev))
    rec["templates_off_ms"], rec["templates_on_ms"] = summary(off), summary(on)
    rec["templates_cost_ms"] = round(rec["templates_on_ms"]["median"] - rec["templates_off_ms"]["median"], 4)
    # the pool's two launches alone, on the rows and the results of the finished step
    lib, n = L.load(), int(rows["frame"].shape[0])
    xinv = torch.empty((n,), dtype=torch.float32, device=dev)
    L.check(lib.fp_row_inv_norm(L.ptr(rows["emb"]), n, D, L.ptr(xinv), L.current_stream(dev)), "fp_row_inv_norm")
    ws = torch.empty((lib.fp_track_pool_workspace_bytes(n),), dtype=torch.uint8, device=dev)
    outs = [tout[k] for k in T.TEMPLATE_OUT_KEYS]

    def pool():
        L.check(lib.fp_track_pool_step(C.byref(trt._tpl), trt.S, D, L.ptr(rows["frame"]), L.ptr(rows["emb"]), L.ptr(xinv), None, n,
                                       L.ptr(rows["sof"]), rows["B"], L.ptr(tout["track_id"]), L.ptr(tout["track_clock"]),
                                       L.ptr(tout["track_flags"]), trt.keep, *[L.ptr(t) for t in outs], L.ptr(ws), ws.numel(),
                                       L.current_stream(dev)), "fp_track_pool_step")
    pool()
    torch.cuda.synchronize()
    rec["pool_ms"] = summary([timed(pool, args.iters, dev) for _ in range(args.rounds)])
    rec["pool_over_tracklets"] = round(rec["pool_ms"]["median"] / rec["tracklets_ms"]["median"], 4)
    rec["pool_floor_bytes"] = 4 * n * D * 4
    rec["pool_gbps"] = round(rec["pool_floor_bytes"] / (rec["pool_ms"]["median"] * 1e-3) / 1e9, 2)


def measure_pipeline(n_frames, args, dev):
    frames = W.make_frames(n_frames, dev)
    det = W.build_detector(dev, W.make_frames(min(64, n_frames), dev, seed=999))
    emb = W.build_embedder(dev)
    ref = W.make_reference(256, dev)
    rec = dict(frames=n_frames)
    for two in (False, True):
        for kind in ("plain", "tracker", "motion", "reid") + (("templates",) if args.templates else ()):
            tr = None if kind == "plain" else StreamTracker(1, D, 8, device=dev, motion=MOTION if kind == "motion" else None,
                                                            reid=REID if kind == "reid" else None,
                                                            templates=Templates() if kind == "templates" else None)
            pipe = FacePipeline(det, emb, ref, tau=0.0, two_streams=two, tracker=tr)
            if two:
                def fn():
                    pipe.step_overlapped(frames)
            else:
                def fn():
                    pipe.step(frames)
            for _ in range(3):
                fn()
            if two:
                pipe.flush()
            torch.cuda.synchronize()
            ts = [timed(fn, args.iters, dev) for _ in range(args.rounds)]
            if two:
                rec["n_faces"] = pipe.flush()["n_faces"]
            torch.cuda.synchronize()
            rec[("overlapped_" if two else "step_") + kind + "_ms"] = summary(ts)
    for k in ("step", "overlapped"):
        rec[k + "_tracker_cost_ms"] = round(rec[k + "_tracker_ms"]["median"] - rec[k + "_plain_ms"]["median"], 4)
        rec[k + "_motion_cost_ms"] = round(rec[k + "_motion_ms"]["median"] - rec[k + "_tracker_ms"]["median"], 4)
        rec[k + "_reid_cost_ms"] = round(rec[k + "_reid_ms"]["median"] - rec[k + "_tracker_ms"]["median"], 4)
        if args.templates:
            rec[k + "_templates_cost_ms"] = round(rec[k + "_templates_ms"]["median"] - rec[k + "_tracker_ms"]["median"], 4)
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--no-pipeline", dest="pipeline", action="store_false")
    ap.add_argument("--templates", action="store_true", help="add the templates leg (fp_track_pool_step)")
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    if args.small:
        args.iters, args.rounds = 1, 2
    F = 8 if args.small else 256
    out = dict(bench="track", small=bool(args.small), iters=args.iters, rounds=args.rounds, D=D, layouts=[])
    out["layouts"].append(measure_layout("a", layout_rows(F, 1, 2, 2, 1, dev), 8, args, dev))
    out["layouts"].append(measure_layout("b", layout_rows(1, F, 2, 2, 2, dev), 8, args, dev))
    out["layouts"].append(measure_layout("c", layout_rows(1, F, 8, 32, 3, dev), 8, args, dev))
    out["layouts"].append(measure_layout("d", layout_rows(1, F, 4, 8, 4, dev), 0, args, dev))
    if args.pipeline:
        out["pipeline"] = measure_pipeline(F, args, dev)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
