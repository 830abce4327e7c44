"""Tracker evaluation (tracking_eval.mot_eval) on synthetic sequences: targets on random walks, hypotheses = jittered copies
with misses, spurious boxes and id hand-overs, seeded.  Two layouts: many short sequences (one workgroup each: the launch
fills the device) and ONE long sequence (a chain of dependent frames on a single workgroup: latency-bound by construction,
reported as measured).

Times the device path with device events -- the torch plumbing (sorts, CSR offsets, dense ids), the fp_mot_match launch --
after a warm-up, `--rounds` rounds of enough calls to last `--round-s` seconds each, the median round with its spread; the
read-back plus the host id assignment (IDTP) by wall clock; then runs the numpy path ONCE on the same rows (wall clock) and
asserts that the device's integers, per-row outputs and the bits of sum_iou equal numpy's.  The comparison is against this
project's own numpy restatement, not against TrackEval or py-motmetrics, which are not installed and which nobody here has
timed.  Prints one JSON line.

`--hota` times tracking_eval.hota_eval next to it on the same rows in the same process: the fp_hota_match launch alternates with
the fp_mot_match launch round by round (`hota.launch`, `hota.launch_over_mot_launch`), the read-back and the host derivation
of the per-alpha numbers go by wall clock, and the numpy path runs once and must give the same integers and the same bits of
gt_sim, gas and the numerators.

  python tools/moteval_bench.py [--seqs 256] [--frames 64] [--targets 8] [--long-frames 8192] [--rounds 5] [--round-s 0.25]
                                [--no-numpy] [--hota]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from face_detection_and_recognition_amd import tracking_eval as TE  # noqa: E402

INT_KEYS = ("TP", "FN", "FP", "IDSW", "Frag", "MT", "PT", "ML", "IDTP", "IDFN", "IDFP")


def synthetic(n_seqs, n_frames, n_targets, seed=0, p_absent=0.05, p_miss=0.12, p_spur=0.2, p_handover=0.03, field=400.0):
    """-> dict of mot_eval's positional arguments.  Per sequence n_targets targets walk inside a field x field square (sizes
    40 .. 90, steps of sigma 4), each present in a frame with probability 1 - p_absent; a present target is detected with
    probability 1 - p_miss (box jittered by 8 % / 5 % of its size), its hypothesis id replaced by a fresh one with probability
    p_handover per frame; with probability p_spur a frame holds one spurious box with an id of its own.  So a frame has at
    most n_targets ground-truth rows and n_targets + 1 hypothesis rows, rows come in (sequence, frame) order, ground-truth ids
    are 1 .. n_targets and every hypothesis id is positive."""
    if not 1 <= n_targets < TE.MAX_ROWS:
        raise ValueError(f"n_targets must be in 1 .. {TE.MAX_ROWS - 1}")
    rng = np.random.default_rng(seed)
    S, F, T = n_seqs, n_frames, n_targets
    pos = rng.uniform(0.0, field, (S, 1, T, 2)) + np.cumsum(rng.normal(0.0, 4.0, (S, F, T, 2)), axis=1)
    size = np.broadcast_to(rng.uniform(40.0, 90.0, (S, 1, T, 2)), (S, F, T, 2))
    box = np.concatenate([pos, size], -1)
    present = rng.random((S, F, T)) >= p_absent
    generation = np.cumsum(rng.random((S, F, T)) < p_handover, axis=1)
    hyp_id = 1 + np.arange(T)[None, None, :] + T * generation
    detected = present & (rng.random((S, F, T)) >= p_miss)
    jitter = np.concatenate([rng.normal(0.0, 0.08, (S, F, T, 2)), rng.normal(0.0, 0.05, (S, F, T, 2))], -1) * np.concatenate([size, size], -1)
    s, f, t = np.nonzero(present)
    out = dict(gt_seq=s, gt_frame=f, gt_id=t + 1, gt_boxes=box[s, f, t])
    s, f, t = np.nonzero(detected)
    spur = rng.random((S, F)) < p_spur
    ss, sf = np.nonzero(spur)
    sbox = np.concatenate([rng.uniform(0.0, field, (len(ss), 2)), rng.uniform(40.0, 90.0, (len(ss), 2))], 1)
    sid = 1 + T * (int(generation.max()) + 2) + sf
    hs, hf = np.concatenate([s, ss]), np.concatenate([f, sf])
    order = np.argsort(hs * F + hf, kind="stable")
    out.update(hy_seq=hs[order], hy_frame=hf[order], hy_id=np.concatenate([hyp_id[s, f, t], sid])[order],
               hy_boxes=np.concatenate([(box + jitter)[s, f, t], sbox])[order], n_frames=np.full(S, F, np.int64))
    return out


def timed(fn, reps, dev):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(torch.cuda.current_stream(dev))
    for _ in range(reps):
        fn()
    e.record(torch.cuda.current_stream(dev))
    e.synchronize()
    return s.elapsed_time(e) / reps


def same(a, b):
    """Device result a against numpy result b: (integers equal, per-row outputs and pot equal, sum_iou bits equal)."""
    rows = zip(a.sequences + [a.combined], b.sequences + [b.combined])
    ints = all(x[k] == y[k] for x, y in rows for k in INT_KEYS)
    per_row = bool(np.array_equal(a.gt_match, b.gt_match) and np.array_equal(a.gt_switch, b.gt_switch)
                   and all(np.array_equal(p, q) for p, q in zip(a.pot, b.pot)))
    bits = all(np.float64(x["sum_iou"]).tobytes() == np.float64(y["sum_iou"]).tobytes()
               for x, y in zip(a.sequences + [a.combined], b.sequences + [b.combined]))
    return ints, per_row, bits


def same_hota(a, b):
    """Device HotaResult a against numpy's b: (integers equal, per-row outputs equal, fp64 bits equal)."""
    rows = list(zip(a.sequences + [a.combined], b.sequences + [b.combined]))
    ints = all(np.array_equal(x[k], y[k]) for x, y in rows for k in TE.HOTA_INT_KEYS + ("levels", "n_gt", "n_hy"))
    per_row = bool(np.array_equal(a.gt_match, b.gt_match) and np.array_equal(a.levels, b.levels)
                   and all(np.array_equal(p, q) for p, q in zip(a.gtc + a.hyc, b.gtc + b.hyc)))
    bits = bool(a.gt_sim.tobytes() == b.gt_sim.tobytes() and all(p.tobytes() == q.tobytes() for p, q in zip(a.gas, b.gas))
                and all(x[k].tobytes() == y[k].tobytes() for x, y in rows for k in TE.HOTA_SUM_KEYS))
    return ints, per_row, bits


def run_layout(data, dev, rounds, round_s, with_numpy, hota=False):
    keys = ("gt_seq", "gt_frame", "gt_id", "gt_boxes", "hy_seq", "hy_frame", "hy_id", "hy_boxes", "n_frames")
    t = [torch.from_numpy(np.ascontiguousarray(data[k])).to(dev) for k in keys]
    state = {}

    def plumbing():
        state["pb"] = TE._Problem(*t, 0.5, dev)

    def launch():
        state["out"] = TE._match_device(state["pb"])
    variants = {"plumbing": plumbing, "launch": launch}
    if hota:
        state["hpb"] = TE._HotaProblem(*t, None, dev)
        variants["hota_launch"] = lambda: state.update(hout=TE._hota_device(state["hpb"]))
        variants["hota_launch"]()
    plumbing()
    launch()
    torch.cuda.synchronize()
    reps = {}
    for name, fn in variants.items():
        reps[name] = max(1, math.ceil(round_s * 1e3 / max(timed(fn, 2, dev), 1e-3)))
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn, reps[name], dev))
    pb = state["pb"]
    frames, longest = int(pb.total), int(pb.n_frames.max()) if pb.S else 0
    out = dict(sequences=pb.S, frames=frames, frames_longest=longest, gt_rows=pb.Ng, hy_rows=pb.Nh, gt_ids=pb.n_gt_ids,
               pot_cells=pb.n_pot)
    summary = {}
    for name, v in times.items():
        summary[name] = dict(ms=round(float(np.median(v)), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4),
                             calls_per_round=reps[name])
    hota_launch = summary.pop("hota_launch", None)
    out.update(summary)
    out["launch_us_per_frame_of_longest"] = round(out["launch"]["ms"] * 1e3 / max(longest, 1), 3)
    out["launch_us_per_frame_overall"] = round(out["launch"]["ms"] * 1e3 / max(frames, 1), 4)
    t0 = time.perf_counter()
    raw = pb.raw(state["out"])
    t1 = time.perf_counter()
    res = TE._finish(pb, raw)
    out["readback_ms"] = round((t1 - t0) * 1e3, 3)
    out["host_id_assignment_ms"] = round((time.perf_counter() - t1) * 1e3, 3)
    out["combined_device"] = {k: res.combined[k] for k in INT_KEYS}
    out["MOTA"], out["IDF1"] = round(res.MOTA, 6), round(res.IDF1, 6)
    if with_numpy:
        t0 = time.perf_counter()
        ref = TE.mot_eval(*(data[k] for k in keys))
        out["numpy_once_s"] = round(time.perf_counter() - t0, 3)
        device_total = out["plumbing"]["ms"] + out["launch"]["ms"] + out["readback_ms"] + out["host_id_assignment_ms"]
        out["numpy_over_device_total"] = round(out["numpy_once_s"] * 1e3 / device_total, 1)
        out["integers_equal"], out["rows_equal"], out["sum_iou_bit_equal"] = same(res, ref)
        assert out["integers_equal"] and out["rows_equal"] and out["sum_iou_bit_equal"], out
    if hota:
        hpb, h = state["hpb"], dict(launch=hota_launch)
        h["launch_over_mot_launch"] = round(hota_launch["ms"] / out["launch"]["ms"], 3)
        h["launch_us_per_frame_of_longest"] = round(hota_launch["ms"] * 1e3 / max(longest, 1), 3)
        t0 = time.perf_counter()
        raw = hpb.raw(state["hout"])
        t1 = time.perf_counter()
        hres = TE._hota_finish(hpb, raw)
        h["readback_ms"] = round((t1 - t0) * 1e3, 3)
        h["host_derivation_ms"] = round((time.perf_counter() - t1) * 1e3, 3)
        h["alphas"] = int(hpb.A)
        for key in TE.HOTA_KEYS:
            h[key] = round(hres.combined[key], 6)
        if with_numpy:
            t0 = time.perf_counter()
            href = TE.hota_eval(*(data[k] for k in keys))
            h["numpy_once_s"] = round(time.perf_counter() - t0, 3)
            h["integers_equal"], h["rows_equal"], h["fp64_bit_equal"] = same_hota(hres, href)
            assert h["integers_equal"] and h["rows_equal"] and h["fp64_bit_equal"], h
        out["hota"] = h
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=256)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--targets", type=int, default=8)
    ap.add_argument("--long-frames", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--round-s", type=float, default=0.25)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--hota", action="store_true", help="time hota_eval next to mot_eval on the same rows")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("moteval_bench.py measures on the GPU; none is available")
    dev = torch.device("cuda:0")
    out = dict(bench="moteval", targets=a.targets)
    with torch.cuda.device(dev):
        out["many_short"] = run_layout(synthetic(a.seqs, a.frames, a.targets, a.seed), dev, a.rounds, a.round_s, not a.no_numpy,
                                       a.hota)
        out["one_long"] = run_layout(synthetic(1, a.long_frames, a.targets, a.seed + 1), dev, a.rounds, a.round_s, not a.no_numpy, a.hota)
    if not a.no_numpy:
        out["compared_against"] = "this project's numpy restatement (tracking_eval.py), not TrackEval / py-motmetrics"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
