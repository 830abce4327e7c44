"""Shared case builders of the tracklet tests (test_tracklets_cpu.py: numpy against the host emulator; test_tracklets_gpu.py:
the device against numpy).

Identity decisions hang on an fp32 cosine whose order of additions is the kernel's own business, so every case builds its
embeddings from chosen directions (an identity vector plus a private noise direction at a chosen angle) and must first pass
assert_gap: in float64, every cosine of a live track x live detection pair keeps GAP = 1e-4 from tau_near and from tau_far,
and any two admissible cosines of one frame are GAP apart or equal by construction (the two tracks' stored rows bitwise equal or
the same slot, and the two detections' rows bitwise equal or the same row).  GAP is three times the worst-case error of an fp32
dot product of unit rows at D = 512, D * 2^-24 = 3.1e-5.  Under that condition numpy, emulator and device must agree EXACTLY
on the four per-row outputs and on the final state.

A case is a dict: name, D, S (streams), max_age, steps (a list of dicts frame / boxes / emb / xinv / score / stream_of_frame,
one per call of the tracker), and expect: a function of (outs, state) that asserts the outcome the case was built for.
"""
import numpy as np

from face_detection_and_recognition_amd import tracking as T

GAP = 1e-4
DIMS = (32, 512)
PARAMS = dict(tau_near=T.TAU_NEAR, tau_far=T.TAU_FAR, iou_min=T.IOU_MIN)


# ------------------------------------------------------------------------------------------------ directions and rows

def ortho(D, k, seed):
    """k orthonormal float64 directions of R^D (k <= D)."""
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((D, k)))
    return q.T.copy()


def spread(D, k, seed, max_cos=0.3):
    """k unit float64 directions with pairwise |cos| < max_cos: orthonormal when they fit, else drawn with rejection."""
    if k <= D // 2:
        return ortho(D, k, seed)
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < k:
        v = rng.standard_normal(D)
        v /= np.linalg.norm(v)
        if all(abs(v @ u) < max_cos for u in out):
            out.append(v)
    return np.stack(out)


def toward(a, b, c):
    """The unit vector in span(a, b) whose cosine with the unit vector a is c (b need not be orthogonal to a)."""
    w = b - (b @ a) * a
    w /= np.linalg.norm(w)
    return c * a + np.sqrt(1.0 - c * c) * w


def obs(ident, c, rng, norm=1.0):
    """An observation of the unit vector `ident` at cosine c: a random direction orthogonal to it supplies the rest."""
    return norm * toward(ident, rng.standard_normal(ident.shape[0]), c)


def cell(k, size=40.0, pitch=100.0, per_row=10, dx=0.0):
    """Box k of a grid of disjoint cells."""
    x, y = (k % per_row) * pitch + dx, (k // per_row) * pitch
    return [x, y, x + size, y + size]


class Steps:
    """Collects the rows of one tracker call after the other."""

    def __init__(self, D):
        self.D, self.steps, self._rows, self._scored = D, [], [], False

    def row(self, frame, box, emb, score=None):
        self._rows.append((frame, box, np.asarray(emb, np.float64), score))
        self._scored |= score is not None
        return self

    def end(self, stream_of_frame, xinv=None):
        rows = self._rows
        emb = np.array([r[2] for r in rows], np.float32).reshape(len(rows), self.D)
        step = dict(frame=np.array([r[0] for r in rows], np.int32), boxes=np.array([r[1] for r in rows], np.float32).reshape(-1, 4),
                    emb=emb, xinv=T.row_inv_norm_numpy(emb) if xinv is None else np.asarray(xinv, np.float32),
                    score=np.array([0.0 if r[3] is None else r[3] for r in rows], np.float32) if self._scored else None,
                    stream_of_frame=np.asarray(stream_of_frame, np.int32))
        self.steps.append(step)
        self._rows, self._scored = [], False
        return self


def _case(name, D, steps, expect, S=1, max_age=100):
    return dict(name=f"{name}-D{D}", D=D, S=S, max_age=max_age, steps=steps.steps if isinstance(steps, Steps) else steps,
                expect=expect)


# ------------------------------------------------------------------------------------------------ running a case

def run_case(case, step_fn, state=None):
    """step_fn(state, max_age=, score=, **step inputs, **PARAMS) on a fresh host state -> (outs per step, final state)."""
    state = T.new_state(case["S"], case["D"]) if state is None else state
    outs = [step_fn(state, st["frame"], st["boxes"], st["emb"], st["xinv"], st["stream_of_frame"], case["max_age"],
                    score=st["score"], **PARAMS) for st in case["steps"]]
    return outs, state


def assert_same(got, want, what=""):
    """Two (outs, state) results: equal, not close (NaN boxes compare as their bits)."""
    (outs_a, st_a), (outs_b, st_b) = got, want
    assert len(outs_a) == len(outs_b)
    for k, (a, b) in enumerate(zip(outs_a, outs_b)):
        for key in T.OUT_KEYS:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), (what, "step", k, key, a[key], b[key])
    assert_same_state(st_a, st_b, what)


def assert_same_state(st_a, st_b, what=""):
    """hdr wholly; the fields of the live slots (a freed slot keeps stale fields that carry no meaning, but they too are the
    same on every path, so everything is compared)."""
    for key in T.STATE_KEYS:
        a, b = np.asarray(st_a[key]), np.asarray(st_b[key])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, key)
        assert a.tobytes() == b.tobytes(), (what, key, np.argwhere(a.view(np.int32) != b.view(np.int32))[:5])


def gap_violation(entry, step):
    """None when one frame's log entry of track_step_numpy(cosines=) meets the gap condition of the module docstring, else
    what breaks it."""
    tn, tf, im = float(np.float32(T.TAU_NEAR)), float(np.float32(T.TAU_FAR)), np.float32(T.IOU_MIN)
    f, slots, rows, c, iou, temb = entry
    fin = c[np.isfinite(c)]
    if not ((np.abs(fin - tn) >= GAP).all() and (np.abs(fin - tf) >= GAP).all()):
        return (f, "a cosine at a threshold")
    adm = ((c > tn) & (iou > im)) | (c > tf)
    ti, dj = np.nonzero(adm)
    cv = c[ti, dj]
    close = np.abs(cv[:, None] - cv[None, :]) < GAP
    for a, b in zip(*np.nonzero(np.triu(close, 1))):
        same_t = ti[a] == ti[b] or temb[ti[a]].tobytes() == temb[ti[b]].tobytes()
        same_d = dj[a] == dj[b] or (step["emb"][rows[dj[a]]].tobytes() == step["emb"][rows[dj[b]]].tobytes()
                                    and step["xinv"][rows[dj[a]]] == step["xinv"][rows[dj[b]]])
        if not (same_t and same_d and cv[a] == cv[b]):
            return (f, "two admissible cosines closer than the gap", float(cv[a]), float(cv[b]))
    return None


def assert_gap(case):
    """The gap condition on every frame of the numpy run's float64 cosines.  -> (outs, state) of the numpy run."""
    log = []
    state = T.new_state(case["S"], case["D"])
    outs = []
    for st in case["steps"]:
        before = len(log)
        outs.append(T.track_step_numpy(state, st["frame"], st["boxes"], st["emb"], st["xinv"], st["stream_of_frame"],
                                       case["max_age"], score=st["score"], cosines=log, **PARAMS))
        for entry in log[before:]:
            bad = gap_violation(entry, st)
            assert bad is None, (case["name"],) + bad
    return outs, state


# ------------------------------------------------------------------------------------------------ the crafted cases

def crossing(D):
    """Two tracks whose boxes cross: while they overlap IoU admits both pairings (the cross cosine 0.8 * 0.85 * 0.9 = 0.612 is
    above tau_near) and the cosine decides (0.648 .. 0.714 and 0.7225 for the own pairs, below tau_far: IoU is needed
    throughout).  A's cosine with its identity grows by 0.01 a frame, which keeps the two cross cosines of a frame apart.  Rows
    alternate their order so that row order never decides."""
    dirs = ortho(D, 14, 11)
    a, b, noise = dirs[0], toward(dirs[0], dirs[1], 0.9), dirs[2:]
    s = Steps(D)
    want = []
    for f in range(6):
        xa, xb = 10.0 * f, 50.0 - 10.0 * f           # A walks right, B walks left: they overlap in the middle frames
        ra = (f, [xa, 0, xa + 40, 40], 1.5 * ((0.8 + 0.01 * f) * a + np.sqrt(1 - (0.8 + 0.01 * f) ** 2) * noise[2 * f]))
        rb = (f, [xb, 5, xb + 40, 45], 0.7 * (0.85 * b + np.sqrt(1 - 0.85 ** 2) * noise[2 * f + 1]))
        for r in ((ra, rb) if f % 2 == 0 else (rb, ra)):
            s.row(*r)
        want += [1, 2] if f % 2 == 0 else [2, 1]
    s.end([0] * 6)

    def expect(outs, state):
        assert outs[0]["track_id"].tolist() == want
        assert state["hdr"][0].tolist() == [6, 3]
    return _case("crossing", D, s, expect)


def greedy_rows(D):
    """(a, b, d, boxes): unit rows with a.b = 0.62, d.b = 0.9, d.a = 0.558; d's box sits on a's."""
    a, e, n = ortho(D, 3, 21)
    b = toward(a, e, 0.62)
    d = 0.9 * b + np.sqrt(1 - 0.81) * n
    return a, b, d, ([0, 0, 40, 40], [200, 0, 240, 40], [2, 0, 42, 40])


def greedy_beats_first_match(D):
    """d is admissible to track A marginally (0.558 with IoU) and to track B strongly (0.9): it goes to B.  The reference's
    first-match rule answers A (test_tracklets_cpu.py checks that with the oracle's FaceTrackerRef)."""
    a, b, d, (ba, bb, bd) = greedy_rows(D)
    s = Steps(D).row(0, ba, a).row(0, bb, b).row(1, bd, d).end([0, 0])

    def expect(outs, state):
        assert outs[0]["track_id"].tolist() == [1, 2, 2]
        assert outs[0]["track_flags"].tolist() == [T.NEW | T.BEST, T.NEW | T.BEST, 0]
    return _case("greedy", D, s, expect)


def one_to_one(D):
    """Two detections of one frame both match the only track (0.8 and 0.9, above tau_far): the better one, the LATER row,
    takes it and the other opens a track."""
    a, n1, n2 = ortho(D, 3, 31)
    s = Steps(D).row(0, cell(0), a).row(1, cell(1), 0.8 * a + 0.6 * n1).row(1, cell(2), 0.9 * a + np.sqrt(0.19) * n2).end([0, 0])

    def expect(outs, state):
        assert outs[0]["track_id"].tolist() == [1, 2, 1]
        assert outs[0]["track_hits"].tolist() == [1, 1, 2]
        assert outs[0]["track_flags"].tolist() == [T.NEW | T.BEST, T.NEW | T.BEST, 0]
    return _case("one_to_one", D, s, expect)


def expiry_edge(D):
    """max_age = 3.  A (seen at clocks 1 and 4: unseen for exactly max_age frames) survives; B (seen at 1 and 5: max_age + 1)
    is freed at clock 5 and its slot is reused by the row that would have matched it.  Frames 1, 2 and 5 .. 7 are empty."""
    a, b = ortho(D, 2, 41)
    s = Steps(D).row(0, cell(0), a).row(0, cell(1), b).row(3, cell(0), a).row(4, cell(1), b).end([0] * 8)

    def expect(outs, state):
        assert outs[0]["track_id"].tolist() == [1, 2, 1, 3]
        assert outs[0]["track_clock"].tolist() == [1, 1, 4, 5]
        assert outs[0]["track_flags"].tolist() == [T.NEW | T.BEST, T.NEW | T.BEST, 0, T.NEW | T.BEST]
        assert state["slot_i"][0, :3, T.I_ID].tolist() == [0, 3, 0]     # A too expired by clock 8 (8 - 4 > 3); B's slot reused
        assert state["hdr"][0].tolist() == [8, 4]
    return _case("expiry", D, s, expect, max_age=3)


def empty_frames(D):
    """A step of empty frames alone (n = 0), then a face: the clock has advanced."""
    a = ortho(D, 1, 51)[0]
    s = Steps(D).end([0] * 5).row(2, cell(0), a).end([0, 0, 0])

    def expect(outs, state):
        assert outs[0]["track_id"].shape == (0,)
        assert outs[1]["track_clock"].tolist() == [8] and outs[1]["track_id"].tolist() == [1]
        assert state["hdr"][0].tolist() == [8, 2]
    return _case("empty", D, s, expect)


def _many(D, n_tracks, later, seed, name):
    """n_tracks identities open in frame 0; every later frame shows the identities of later[k] (indices, in that row order).
    Identity k is always seen in the plane of its own two directions, at an angle chosen so that the j-th row of a frame has
    the cosine 0.99 - 0.002 j with the identity's previous sighting: distinct own cosines, all above tau_far."""
    ids = spread(D, n_tracks, seed)
    rng = np.random.default_rng(seed)
    wk = np.stack([toward(v, rng.standard_normal(D), 0.0) for v in ids])     # unit, orthogonal to its identity
    theta = np.zeros((n_tracks,))
    s = Steps(D)
    for k in range(n_tracks):
        s.row(0, cell(k), ids[k], score=0.5)
    for f, shown in enumerate(later, start=1):
        for j, k in enumerate(shown):
            step = np.arccos(0.99 - 0.002 * j)
            theta[k] += step if theta[k] <= 0.5 else -step
            s.row(f, cell(k, dx=3.0), (0.5 + 0.03 * j) * (np.cos(theta[k]) * ids[k] + np.sin(theta[k]) * wk[k]),
                  score=0.5 + 0.001 * ((j * 7) % 11))
    s.end([0] * (1 + len(later)))
    want = list(range(1, n_tracks + 1)) + [k + 1 for shown in later for k in shown]

    def expect(outs, state):
        assert outs[0]["track_id"].tolist() == want
        assert (state["slot_i"][0, :, T.I_ID] != 0).sum() == n_tracks
    return _case(name, D, s, expect)


def pairs_72(D):
    """9 tracks x 8 detections = 72 pairs: more than one wave holds."""
    return _many(D, 9, [[7, 2, 5, 0, 3, 6, 1, 4]], 61, "pairs72")


def pairs_40x40(D):
    """40 x 40 = 1600 pairs (sorted as 2048), then 40 x 33 = 1320 and 40 x 25 = 1000 (sorted as 1024): the sort's power-of-two
    sizes from both sides."""
    p = np.random.default_rng(62).permutation(40)
    return _many(D, 40, [p.tolist(), p[::-1][:33].tolist(), p[5:30].tolist()], 62, "pairs40x40")


def fill_then_full(D):
    """64 faces fill the slots (two frames of 32: every track of frame 0 scored against frame 1's strangers); then a 65th
    identity gets FULL beside a row that matches."""
    rng = np.random.default_rng(63)
    ids = spread(D, 65, 63)
    s = Steps(D)
    for k in range(64):
        s.row(k // 32, cell(k), ids[k])
    s.row(2, cell(64), ids[64]).row(2, cell(3), obs(ids[3], 0.95, rng)).end([0, 0, 0])

    def expect(outs, state):
        o = outs[0]
        assert o["track_id"].tolist() == list(range(1, 65)) + [0, 4]
        assert o["track_flags"][64:].tolist() == [T.FULL, 0] and o["track_hits"][64:].tolist() == [0, 2]
        assert state["hdr"][0].tolist() == [3, 65]
    return _case("full", D, s, expect)


def over_65(D):
    """65 rows in one frame, the 4th dead: positions count dead rows, so 63 tracks open and the 65th row gets OVER."""
    ids = spread(D, 65, 64)
    s = Steps(D)
    for k in range(65):
        s.row(0, cell(k), ids[k] * (0.0 if k == 3 else 1.0))
    s.end([0])

    def expect(outs, state):
        o = outs[0]
        assert o["track_flags"][64] == T.OVER and o["track_flags"][3] == T.DEAD_ROW and o["track_id"][64] == 0
        assert o["track_id"][:64].tolist() == [1, 2, 3, 0] + list(range(4, 64))
        assert state["hdr"][0].tolist() == [1, 64]
    return _case("over", D, s, expect)


def ties(D):
    """Bitwise duplicate detections open duplicate tracks (frame 0); two duplicates again (frame 1): four equal cosines, the
    lower slot takes the lower row; one more (frame 2) goes to the lower slot."""
    a, n = ortho(D, 2, 71)
    d1, d2 = 0.9 * a + np.sqrt(0.19) * n, 0.95 * a + np.sqrt(1 - 0.95 ** 2) * n
    s = Steps(D)
    s.row(0, cell(0), a).row(0, cell(0), a).row(1, cell(0), d1).row(1, cell(0), d1).row(2, cell(0), d2).end([0, 0, 0])

    def expect(outs, state):
        assert outs[0]["track_id"].tolist() == [1, 2, 1, 2, 1]
        assert outs[0]["track_hits"].tolist() == [1, 1, 2, 2, 3]
    return _case("ties", D, s, expect)


def dead_rows(D):
    """Zero, NaN and Inf embeddings (dead rows), a NaN box on a live row (opens a track; matched later through tau_far alone,
    its IoU being 0), a frame of stream -1, a stream index out of range, frame indices out of range."""
    a, b, n = ortho(D, 3, 81)
    nan_row, inf_row = a.copy(), a.copy()
    nan_row[1], inf_row[2] = np.nan, np.inf
    nanbox = [np.nan, 0, 40, 40]
    s = Steps(D)
    s.row(0, cell(0), a).row(0, cell(1), 0 * a).row(0, cell(2), nan_row).row(0, cell(3), inf_row).row(0, nanbox, b)
    s.row(1, cell(0), a).row(2, cell(0), a).row(-1, cell(0), a).row(5, cell(0), a)
    s.row(3, cell(9), 0.9 * b + np.sqrt(0.19) * n).row(3, [0, 0, np.nan, 40], 0.6 * a + 0.8 * n)
    s.end([0, -1, 7, 0])

    def expect(outs, state):
        o = outs[0]
        NB, NS, DR = T.NEW | T.BEST, T.NO_STREAM, T.DEAD_ROW
        assert o["track_flags"].tolist() == [NB, DR, DR, DR, NB, NS, NS, NS, NS, 0, NB]
        assert o["track_id"].tolist() == [1, 0, 0, 0, 2, 0, 0, 0, 0, 2, 3]
        assert o["track_clock"].tolist() == [1, 1, 1, 1, 1, 0, 0, 0, 0, 2, 2]
    return _case("dead", D, s, expect, S=2)


def best_shot(D):
    """BEST moves only on a strictly greater score: scores 0.5 0.5 0.7 0.7 0.6 flag frames 0 and 2 (of equal scores the first
    row wins)."""
    rng = np.random.default_rng(91)
    a = ortho(D, 1, 91)[0]
    s = Steps(D)
    for f, sc in enumerate([0.5, 0.5, 0.7, 0.7, 0.6]):
        s.row(f, cell(0, dx=f), obs(a, 0.97 - 0.01 * f, rng), score=sc)
    s.end([0] * 5)
    third = s.steps[0]["emb"][2].tobytes()

    def expect(outs, state):
        assert outs[0]["track_flags"].tolist() == [T.NEW | T.BEST, 0, T.BEST, 0, 0]
        assert state["slot_i"][0, 0].tolist() == [1, 1, 5, 5, 3]
        assert state["slot_f"][0, 0, T.F_BEST_SCORE] == np.float32(0.7)
        assert state["slot_f"][0, 0, T.F_BEST_BOX:].tolist() == cell(0, dx=2)
        assert state["best_emb"][0, 0].tobytes() == third
    return _case("best", D, s, expect)


CRAFTED = (crossing, greedy_beats_first_match, one_to_one, expiry_edge, empty_frames, pairs_72, pairs_40x40, fill_then_full,
           over_65, ties, dead_rows, best_shot)


def crafted_cases():
    return [fn(D) for fn in CRAFTED for D in DIMS]


# ------------------------------------------------------------------------------------------------ the busy batch of the invariances

def busy(D, seed=5, n_streams=4, n_frames=48, max_age=2):
    """One batch of n_frames frames dealt to n_streams streams (and a few to none), each stream with its own few identities
    that come and go, bursts of empty frames longer than max_age (tracks expire and slots are reused), scores, rows in frame
    order.  -> a one-step case."""
    rng = np.random.default_rng(seed)
    per = 3
    ids = spread(D, n_streams * per, seed + 1)
    sof = rng.integers(-1, n_streams, n_frames)
    sof[1] = sof[n_frames - 2] = -1                  # frames nobody tracks, with rows
    burst = (n_frames // 4, 3 * n_frames // 4)       # empty frames in the middle: about five per stream, tracks expire
    s = Steps(D)
    for f in range(n_frames):
        st = int(sof[f])
        if burst[0] <= f < burst[1]:
            continue
        for j in rng.permutation(per):
            if rng.random() < 0.7 or (st < 0 and j == 0):
                k = max(st, 0) * per + int(j)
                s.row(f, cell(k, dx=float(rng.integers(0, 8))), obs(ids[k], float(rng.choice([0.86, 0.9, 0.94, 0.98])), rng,
                                                                   float(rng.uniform(0.5, 2.0))),
                      score=float(rng.choice([0.2, 0.5, 0.5, 0.8])))
    s.end(sof)
    return _case(f"busy{seed}", D, s, None, S=n_streams, max_age=max_age)


def split_case(case, k):
    """The one-step case cut into two steps: frames [0, k) and [k, B)."""
    (st,) = case["steps"]
    B = len(st["stream_of_frame"])
    parts = []
    for lo, hi in ((0, k), (k, B)):
        m = (st["frame"] >= lo) & (st["frame"] < hi)
        parts.append(dict(frame=st["frame"][m] - lo, boxes=st["boxes"][m], emb=st["emb"][m], xinv=st["xinv"][m],
                          score=None if st["score"] is None else st["score"][m], stream_of_frame=st["stream_of_frame"][lo:hi]))
    return dict(case, steps=parts), [np.nonzero((st["frame"] >= lo) & (st["frame"] < hi))[0] for lo, hi in ((0, k), (k, B))]


def stream_alone(case, s):
    """The one-step case reduced to the frames of stream s, run as stream 0 of a one-stream tracker.  -> (case, rows kept)."""
    (st,) = case["steps"]
    frames = np.nonzero(st["stream_of_frame"] == s)[0]
    new_index = {int(f): i for i, f in enumerate(frames)}
    m = np.isin(st["frame"], frames)
    part = dict(frame=np.array([new_index[int(f)] for f in st["frame"][m]], np.int32), boxes=st["boxes"][m], emb=st["emb"][m],
                xinv=st["xinv"][m], score=None if st["score"] is None else st["score"][m],
                stream_of_frame=np.zeros((len(frames),), np.int32))
    return dict(case, S=1, steps=[part]), np.nonzero(m)[0]


def scattered(case, seed=3):
    """The one-step case with its rows permuted so that no frame's rows stay together, rows of one frame keeping their order.
    -> (case, perm): row i of the new case is row perm[i] of the old."""
    (st,) = case["steps"]
    rng = np.random.default_rng(seed)
    n = len(st["frame"])
    slots = rng.permutation(n)                     # where the rows go ...
    perm = np.empty((n,), np.int64)
    for f in np.unique(st["frame"]):               # ... each frame's rows fill its places in ascending order
        rows = np.nonzero(st["frame"] == f)[0]
        perm[np.sort(slots[rows])] = rows
    part = dict(frame=st["frame"][perm], boxes=st["boxes"][perm], emb=st["emb"][perm], xinv=st["xinv"][perm],
                score=None if st["score"] is None else st["score"][perm], stream_of_frame=st["stream_of_frame"])
    return dict(case, steps=[part]), perm
