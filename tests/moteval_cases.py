"""Shared inputs of the tracker-evaluation tests (test_moteval_cpu.py: numpy against brute force, scipy and the host emulator;
test_moteval_gpu.py: the device against numpy; test_moteval_bench_tool.py).

A data set is a dict of the positional arguments of tracking_eval.mot_eval: gt_seq, gt_frame, gt_id, gt_boxes, hy_seq,
hy_frame, hy_id, hy_boxes, n_frames.  Boxes are xywh fp64.  Hand cases use B = [0, 0, 100, 100] and thr = 0.5; their expected
values are the ones DESIGN section 7 lists.
"""
import numpy as np

KEYS = ("gt_seq", "gt_frame", "gt_id", "gt_boxes", "hy_seq", "hy_frame", "hy_id", "hy_boxes", "n_frames")
B = [0.0, 0.0, 100.0, 100.0]
INT_KEYS = ("TP", "FN", "FP", "IDSW", "Frag", "MT", "PT", "ML", "IDTP", "IDFN", "IDFP")


def make(gt_rows, hy_rows, n_frames):
    """rows: lists of (seq, frame, id, box)."""
    def cols(rows):
        return (np.array([r[0] for r in rows], np.int64), np.array([r[1] for r in rows], np.int64),
                np.array([r[2] for r in rows], np.int64), np.array([r[3] for r in rows], np.float64).reshape(-1, 4))
    return dict(zip(KEYS, cols(gt_rows) + cols(hy_rows) + (np.asarray(n_frames, np.int64),)))


def shifted(dx):
    return [float(dx), 0.0, 100.0, 100.0]


def hand_cases():
    """name -> (data, expected combined integers, extra)."""
    cases = {}
    # A, hand-over: one target, hypothesis id 1 on frames 0-2, id 2 on frames 3-5, same box
    cases["A"] = (make([(0, f, 7, B) for f in range(6)], [(0, f, 1 if f < 3 else 2, B) for f in range(6)], [6]),
                  dict(TP=6, FN=0, FP=0, IDSW=1, Frag=0, MT=1, IDTP=3, IDFN=3, IDFP=3))
    # B, continuity beats IoU: hypothesis 5 at IoU 0.538 in both frames, hypothesis 6 at IoU 0.960 in frame 1
    cases["B"] = (make([(0, 0, 1, B), (0, 1, 1, B)], [(0, 0, 5, shifted(30)), (0, 1, 6, shifted(2)), (0, 1, 5, shifted(30))], [2]),
                  dict(TP=2, FN=0, FP=1, IDSW=0))
    # C, optimum beats greedy: IoUs [[.818, .538], [.6, .212]]
    cases["C"] = (make([(0, 0, 1, B), (0, 0, 2, shifted(35))], [(0, 0, 1, shifted(10)), (0, 0, 2, shifted(-30))], [1]),
                  dict(TP=2, FN=0, FP=0))
    # D, gap: hypothesis missing in frame 2
    cases["D"] = (make([(0, f, 1, B) for f in range(5)], [(0, f, 1, B) for f in (0, 1, 3, 4)], [5]),
                  dict(TP=4, FN=1, FP=0, IDSW=0, Frag=1, MT=0, PT=1))
    # E, target absent in frame 2
    cases["E"] = (make([(0, f, 1, B) for f in (0, 1, 3, 4)], [(0, f, 9, B) for f in range(5)], [5]),
                  dict(TP=4, FN=0, FP=1, IDSW=0, Frag=1, MT=1))
    # F, swap: the hypothesis ids of two targets exchange at frame 2
    b0, b1 = [0.0, 0.0, 50.0, 50.0], [200.0, 0.0, 50.0, 50.0]
    cases["F"] = (make([(0, f, t, (b0, b1)[t]) for f in range(4) for t in range(2)],
                       [(0, f, (t if f < 2 else 1 - t) + 10, (b0, b1)[t]) for f in range(4) for t in range(2)], [4]),
                  dict(TP=8, FN=0, FP=0, IDSW=2, IDTP=4, IDFN=4, IDFP=4))
    return cases


def seeded_set(seed, n_frames=40, n_targets=6, p_absent=0.06, p_miss=0.13, p_spur=0.2, p_handover=0.05, field=260.0):
    """One sequence: targets on random walks inside a small field (so that they overlap now and then), hypotheses = jittered
    copies with misses, at most one spurious box per frame, and hypothesis ids that are handed over to a fresh id now and
    then.  At most n_targets + 1 hypotheses per frame."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.0, field, (n_targets, 2))
    size = rng.uniform(40.0, 90.0, (n_targets, 2))
    hyp_of = 100 + np.arange(n_targets)
    next_id = 100 + n_targets
    gt_rows, hy_rows = [], []
    for f in range(n_frames):
        pos = pos + rng.normal(0.0, 5.0, pos.shape)
        for t in range(n_targets):
            if rng.random() < p_absent:
                continue
            box = np.concatenate([pos[t], size[t]])
            gt_rows.append((0, f, 7 * t + 3, box))
            if rng.random() < p_handover:
                hyp_of[t], next_id = next_id, next_id + 1
            if rng.random() >= p_miss:
                jit = np.concatenate([rng.normal(0.0, 0.09, 2) * size[t], rng.normal(0.0, 0.06, 2) * size[t]])
                hy_rows.append((0, f, int(hyp_of[t]), box + jit))
        if rng.random() < p_spur:
            hy_rows.append((0, f, next_id, np.concatenate([rng.uniform(0.0, field, 2), rng.uniform(40.0, 90.0, 2)])))
            next_id += 1
    return make(gt_rows, hy_rows, [n_frames])


def dense_frames(n, m, seed, frames=3, pitch=9.0):
    """One sequence of `frames` frames with n targets and m hypotheses each on a tight grid of 50 x 50 boxes: most pairs of
    neighbours are admissible, so the assignment has real work, and hypothesis ids are re-dealt per frame so that
    continuity bonuses pull against IoU."""
    rng = np.random.default_rng(seed)
    gt_rows, hy_rows = [], []
    for f in range(frames):
        hid = rng.permutation(m) if f % 2 else np.arange(m)
        for t in range(n):
            gt_rows.append((0, f, t, [pitch * (t % 8) + rng.normal(0, 1.0), pitch * (t // 8) + rng.normal(0, 1.0), 50.0, 50.0]))
        for j in range(m):
            hy_rows.append((0, f, int(hid[j]) + 500, [pitch * (j % 8) + rng.normal(0, 2.0), pitch * (j // 8) + rng.normal(0, 2.0),
                                                     50.0 + rng.normal(0, 2.0), 50.0 + rng.normal(0, 2.0)]))
    return make(gt_rows, hy_rows, [frames])


def with_empty_frames():
    """Frames without ground truth, without hypotheses and without either, in the middle and at both ends."""
    gt = [(0, f, 1, B) for f in (1, 2, 4, 7)] + [(0, 2, 2, shifted(300))]
    hy = [(0, f, 4, shifted(5)) for f in (1, 3, 4, 7)] + [(0, 5, 8, shifted(300))]
    return make(gt, hy, [10])


def combine(sets, merge_seed=None):
    """Several one-sequence sets as sequences 0, 1, ... of one set.  merge_seed: the rows of the sequences are dealt into one
    another at random, each sequence keeping its own row order."""
    out = {}
    for key in KEYS:
        if key == "n_frames":
            out[key] = np.concatenate([d[key] for d in sets])
        elif key.endswith("_seq"):
            out[key] = np.concatenate([np.full(len(d[key]), s, np.int64) for s, d in enumerate(sets)])
        else:
            out[key] = np.concatenate([d[key] for d in sets])
    if merge_seed is not None:
        rng = np.random.default_rng(merge_seed)
        for side in ("gt", "hy"):
            seqs = out[f"{side}_seq"]                                   # still one sequence after the other
            pool = rng.permutation(seqs)                                # the sequence that supplies position k
            nxt = {int(s): iter(np.nonzero(seqs == s)[0]) for s in np.unique(seqs)}
            rows = np.array([next(nxt[int(s)]) for s in pool], np.int64)
            for key in (f"{side}_seq", f"{side}_frame", f"{side}_id", f"{side}_boxes"):
                out[key] = out[key][rows]
    return out


def permute_within_frames(data, seed):
    """The same rows in another order (any permutation: positions inside the frames change)."""
    rng = np.random.default_rng(seed)
    out = dict(data)
    for side in ("gt", "hy"):
        perm = rng.permutation(len(data[f"{side}_seq"]))
        for key in (f"{side}_seq", f"{side}_frame", f"{side}_id", f"{side}_boxes"):
            out[key] = data[key][perm]
    return out


def many_sequences(k=32, seed=11):
    """k sequences of different lengths (one of them without frames, one without rows) in one set."""
    rng = np.random.default_rng(seed)
    sets = []
    for s in range(k):
        if s == 3:
            sets.append(make([], [], [0]))
        elif s == 5:
            sets.append(make([], [], [4]))
        else:
            sets.append(seeded_set(1000 + s, n_frames=int(rng.integers(1, 14)), n_targets=int(rng.integers(1, 7))))
    return combine(sets)


def emulator_inputs():
    """name -> data: what the emulator and the device are compared on against numpy."""
    cases = {f"seed{s}": seeded_set(s) for s in range(6)}
    cases["3x7"] = dense_frames(3, 7, 21)
    cases["7x3"] = dense_frames(7, 3, 22)
    cases["64x64"] = dense_frames(64, 64, 23)
    cases["40x64"] = dense_frames(40, 64, 24, frames=2)
    cases["empty_frames"] = with_empty_frames()
    cases["no_rows"] = combine([make([], [], [0]), seeded_set(9, n_frames=5), make([], [], [3])])
    cases["gt_only"] = make([(0, 0, 1, B), (0, 1, 1, B)], [], [2])
    cases["hy_only"] = make([], [(0, 0, 1, B), (0, 1, 1, B)], [2])
    for name, (data, _) in hand_cases().items():
        cases[f"hand{name}"] = data
    return cases


def assert_same_result(a, b, what=""):
    """Two MotResults: equal integers per sequence and combined, gt_match / gt_switch, pot, and sum_iou bit for bit."""
    assert len(a.sequences) == len(b.sequences), what
    for s, (x, y) in enumerate(zip(a.sequences + [a.combined], b.sequences + [b.combined])):
        for key in INT_KEYS + ("n_gt_ids", "n_hy_ids"):
            assert x[key] == y[key], (what, s, key, x[key], y[key])
        assert np.float64(x["sum_iou"]).tobytes() == np.float64(y["sum_iou"]).tobytes(), (what, s, x["sum_iou"], y["sum_iou"])
    assert np.array_equal(a.gt_match, b.gt_match), (what, "gt_match", np.nonzero(a.gt_match != b.gt_match)[0][:8])
    assert np.array_equal(a.gt_switch, b.gt_switch), (what, "gt_switch")
    for s, (p, q) in enumerate(zip(a.pot, b.pot)):
        assert p.shape == q.shape and np.array_equal(p, q), (what, "pot", s)
