"""Shared case builders of the re-identification tests (test_reid_cpu.py: numpy against the host emulator; test_reid_gpu.py: the
device against numpy), on top of track_cases.py and motion_cases.py.

A case is a track_cases case plus `reid` (a LostPool), optionally `lost_init` (a function that writes into the fresh pool before
the first step) and `expect`, a function of (outs, state, lost_state).  Every case must first pass assert_gap: track_cases' gap
condition on the cosines of step 2, and the same condition on step 3b -- in float64 every reid cosine keeps GAP = 1e-4 from
tau_reid, and any two admissible reid cosines of one frame are GAP apart unless the same entry and bitwise equal detection rows
produce them.  Under that condition numpy, emulator and device must agree EXACTLY on the per-row outputs, the five state
arrays, `motion` and the five lost_* arrays.

Embeddings are built from orthonormal directions: two persons are orthogonal, consecutive sightings of one person swing between
its direction and a row at a chosen cosine (motion_cases.swing), a returning face is TC.toward(last row, fresh direction, c).
"""
import numpy as np

import motion_cases as MC
import track_cases as TC
from face_detection_and_recognition_amd import tracking as T

DIMS = TC.DIMS
GAP = TC.GAP


def _case(name, D, steps, expect, reid, S=1, max_age=3, lost_init=None):
    return dict(TC._case(name, D, steps, expect, S=S, max_age=max_age), reid=reid, lost_init=lost_init, motion=MC.CV)


# ------------------------------------------------------------------------------------------------ running a case

def run_case(case, step_fn, reid=True, motion=False, state=None, lost_state=None, motion_state=None):
    """step_fn(state, ..., reid=, lost_state=[, motion=, motion_state=]) over the case's steps on a fresh state ->
    (outs, state, motion_state, lost_state); reid False: the same rows through the tracker without a pool."""
    state = T.new_state(case["S"], case["D"]) if state is None else state
    kw = {}
    if reid:
        if lost_state is None:
            lost_state = T.new_lost_state(case["S"], case["D"])
            if case.get("lost_init"):
                case["lost_init"](lost_state)
        kw.update(reid=case["reid"], lost_state=lost_state)
    if motion:
        motion_state = T.new_motion_state(case["S"]) if motion_state is None else motion_state
        kw.update(motion=case["motion"], motion_state=motion_state)
    outs = [step_fn(state, st["frame"], st["boxes"], st["emb"], st["xinv"], st["stream_of_frame"], case["max_age"],
                    score=st["score"], **TC.PARAMS, **kw) for st in case["steps"]]
    return outs, state, (motion_state if motion else None), (lost_state if reid else None)


def reid_gap_violation(entry, step, tau_reid):
    """None when one frame's entry of track_step_numpy(reid_cosines=) meets the gap condition of the module docstring."""
    f, ents, rows, c = entry
    tr = float(np.float32(tau_reid))
    fin = c[np.isfinite(c)]
    if not (np.abs(fin - tr) >= GAP).all():
        return (f, "a reid cosine at tau_reid")
    ei, dj = np.nonzero(c > tr)
    cv = c[ei, dj]
    close = np.abs(cv[:, None] - cv[None, :]) < GAP
    for a, b in zip(*np.nonzero(np.triu(close, 1))):
        same_d = dj[a] == dj[b] or (step["emb"][rows[dj[a]]].tobytes() == step["emb"][rows[dj[b]]].tobytes()
                                    and step["xinv"][rows[dj[a]]] == step["xinv"][rows[dj[b]]])
        if not (ei[a] == ei[b] and same_d and cv[a] == cv[b]):
            return (f, "two admissible reid cosines closer than the gap", float(cv[a]), float(cv[b]))
    return None


def assert_gap(case, reid=True, motion=False):
    """The numpy run with the gap condition on every frame's float64 cosines, of step 2 and of step 3b.
    -> (outs, state, motion_state, lost_state, reid_log)."""
    log, rlog = [], []

    def step(state, *a, **kw):
        b0, b1 = len(log), len(rlog)
        if reid:
            kw["reid_cosines"] = rlog
        out = T.track_step_numpy(state, *a, cosines=log, **kw)
        st = next(s for s in case["steps"] if s["frame"] is a[0])
        for entry in log[b0:]:
            bad = TC.gap_violation(entry, st)
            assert bad is None, (case["name"],) + bad
        for entry in rlog[b1:]:
            bad = reid_gap_violation(entry, st, case["reid"].tau_reid)
            assert bad is None, (case["name"],) + bad
        return out
    return run_case(case, step, reid, motion) + (rlog,)


def assert_same_lost(l_a, l_b, what=""):
    assert (l_a is None) == (l_b is None), what
    if l_a is not None:
        for key in T.LOST_KEYS:
            a, b = np.asarray(l_a[key]), np.asarray(l_b[key])
            assert a.shape == b.shape and a.dtype == b.dtype, (what, key)
            assert a.tobytes() == b.tobytes(), (what, key, np.argwhere(a.view(np.int32) != b.view(np.int32))[:5])


def assert_same(got, want, what=""):
    """Two (outs, state, motion_state, lost_state) results: equal, not close."""
    MC.assert_same(got[:3], want[:3], what)
    assert_same_lost(got[3], want[3], what)


def flags_of(outs):
    return np.concatenate([np.asarray(o["track_flags"]) for o in outs])


# ------------------------------------------------------------------------------------------------ the crafted cases

def revolving_door(D):
    """max_age 3, tau_reid 0.75, lost_age 100.  B is there in frames 0 .. 21.  A is there in 0 .. 4, away, and back in 17 .. 21
    in another grid cell at cosine 0.85 to its last row; a stranger C enters in frame 17.  Rows of a frame in the order B, C, A.
    With the pool A keeps id 2 (one REVIVED row, hits 6, 7, ...) and next_id ends at 4; without it A comes back as id 4.
    gt: the persons' own rows for mot_eval."""
    a, b, c, wa, wb, wc, n1, wa2 = TC.ortho(D, 8, 201)
    a17 = TC.toward(a, n1, 0.85)                      # frame 4's row of A is `a` itself (an even sighting of the swing)
    s = TC.Steps(D)
    gt = []
    for f in range(22):
        s.row(f, TC.cell(0, dx=float(f % 3)), MC.swing(b, wb, 0.95, f))
        gt.append(1)
        if f >= 17:
            s.row(f, TC.cell(7), MC.swing(c, wc, 0.92, f - 17))
            gt.append(3)
            s.row(f, TC.cell(25), MC.swing(a17, wa2, 0.97, f - 17))
            gt.append(2)
        elif f <= 4:
            s.row(f, TC.cell(3), MC.swing(a, wa, 0.98, f))
            gt.append(2)
    s.end([0] * 22)
    gt = np.array(gt, np.int32)

    def expect(outs, state, lost):
        o = outs[0]
        assert np.array_equal(o["track_id"], gt)
        assert sorted(set(o["track_id"].tolist())) == [1, 2, 3]
        assert (o["track_flags"] & T.REVIVED != 0).sum() == 1 and o["track_flags"][o["track_id"] == 2][5] == T.REVIVED
        assert o["track_hits"][gt == 2].tolist() == list(range(1, 11))
        assert state["hdr"][0].tolist() == [22, 4]
        assert not lost["lost_i"][0, :, T.I_ID].any() and lost["lost_hdr"][0, 0] == 1

    def expect_without(outs, state):
        o = outs[0]
        assert sorted(set(o["track_id"].tolist())) == [1, 2, 3, 4]
        assert o["track_id"][gt == 2].tolist() == [2] * 5 + [4] * 5 and state["hdr"][0].tolist() == [22, 5]
    case = _case("door", D, s, expect, T.LostPool(0.75, 100))
    case["expect_without"] = expect_without
    st = case["steps"][0]
    case["gt"] = (st["frame"], gt, np.concatenate([st["boxes"][:, :2], st["boxes"][:, 2:] - st["boxes"][:, :2]], axis=1))
    return case


def same_frame(D):
    """max_age 3.  A (slot 0) and B (slot 1) open in frame 0; B stays.  A is absent for exactly max_age + 1 frames: in frame 4 it
    expires, is parked and -- its row is there, at cosine 0.85, in a cell that overlaps nothing -- revived in the same frame.
    A new face X stands before it in row order and takes the freed slot 0, so A continues in slot 2."""
    a, b, x, wb, n1 = TC.ortho(D, 5, 211)
    s = TC.Steps(D)
    s.row(0, TC.cell(0), a).row(0, TC.cell(1), b)
    for f in (1, 2, 3):
        s.row(f, TC.cell(1), MC.swing(b, wb, 0.95, f))
    s.row(4, TC.cell(12), x).row(4, TC.cell(30), TC.toward(a, n1, 0.85)).row(4, TC.cell(1), MC.swing(b, wb, 0.95, 4))
    s.end([0] * 5)

    def expect(outs, state, lost):
        o = outs[0]
        assert o["track_id"].tolist() == [1, 2, 2, 2, 2, 3, 1, 2]
        assert o["track_flags"].tolist() == [T.NEW | T.BEST, T.NEW | T.BEST, 0, 0, 0, T.NEW | T.BEST, T.REVIVED, 0]
        assert o["track_hits"].tolist() == [1, 1, 2, 3, 4, 1, 2, 5]
        assert state["slot_i"][0, :3, T.I_ID].tolist() == [3, 2, 1] and state["slot_i"][0, 2].tolist() == [1, 1, 5, 2, 1]
        assert state["hdr"][0].tolist() == [5, 4]
        assert not lost["lost_i"][0, :, T.I_ID].any() and lost["lost_hdr"][0, 0] == 1
    return _case("sameframe", D, s, expect, T.LostPool(0.75, 50))


def crossed_return(D):
    """max_age 2, tau_reid 0.5.  P and Q (orthogonal) are seen in frames 0 .. 2 and parked in frame 5.  In frame 7 two faces
    return, rows in the order y, x: x.P = 0.70, x.Q = 0.60, y.P = 0.65, y.Q = 0.52.  Each face's best parked track is P; the
    greedy walk gives x P (0.70 first) and y Q (0.52, all that is left), although x-Q plus y-P would sum higher."""
    p, q, wp, wq, n1, n2 = TC.ortho(D, 6, 221)
    x = 0.70 * p + 0.60 * q + np.sqrt(1 - 0.49 - 0.36) * n1
    y = 0.65 * p + 0.52 * q + np.sqrt(1 - 0.65 ** 2 - 0.52 ** 2) * n2
    s = TC.Steps(D)
    for f in range(3):
        s.row(f, TC.cell(0), MC.swing(p, wp, 0.98, f)).row(f, TC.cell(1), MC.swing(q, wq, 0.95, f))
    s.row(7, TC.cell(20), y).row(7, TC.cell(21), x).end([0] * 8)

    def expect(outs, state, lost):
        o = outs[0]
        assert o["track_id"].tolist() == [1, 2] * 3 + [2, 1]
        assert o["track_flags"][-2:].tolist() == [T.REVIVED, T.REVIVED] and o["track_hits"][-2:].tolist() == [4, 4]
        assert state["slot_i"][0, :2, T.I_ID].tolist() == [2, 1] and state["hdr"][0].tolist() == [8, 3]
    return _case("crossed", D, s, expect, T.LostPool(0.5, 50), max_age=2)


def stranger(D):
    """P is parked; a face whose best pool cosine is 0.6, below tau_reid = 0.75, opens a new track and the pool keeps P."""
    p, n1 = TC.ortho(D, 2, 231)
    s = TC.Steps(D).row(0, TC.cell(0), p).row(5, TC.cell(9), TC.toward(p, n1, 0.6)).end([0] * 6)

    def expect(outs, state, lost):
        assert outs[0]["track_id"].tolist() == [1, 2] and outs[0]["track_flags"].tolist() == [T.NEW | T.BEST] * 2
        assert lost["lost_i"][0, 0].tolist() == [1, 1, 1, 1, 1] and lost["lost_i"][0, 1:, T.I_ID].any() == 0
        assert lost["lost_emb"][0, 0].tobytes() == np.asarray(p, np.float32).tobytes() and lost["lost_hdr"][0, 0] == 1
        assert state["hdr"][0].tolist() == [6, 3]
    return _case("stranger", D, s, expect, T.LostPool(0.75, 50), max_age=2)


def forgotten(D):
    """max_age 2, lost_age 6.  P is seen at clock 1, Q at clocks 1 and 2; both return at clock 8 at cosine 0.9.  P is
    lost_age + 1 frames past its last sighting: its entry was emptied, it opens id 3.  Q, at exactly lost_age, is revived."""
    p, q, wq, n1, n2 = TC.ortho(D, 5, 241)
    s = TC.Steps(D)
    s.row(0, TC.cell(0), p).row(0, TC.cell(1), q).row(1, TC.cell(1), MC.swing(q, wq, 0.95, 1))
    s.row(7, TC.cell(20), TC.toward(p, n1, 0.9)).row(7, TC.cell(21), TC.toward(MC.swing(q, wq, 0.95, 1), n2, 0.9)).end([0] * 8)

    def expect(outs, state, lost):
        o = outs[0]
        assert o["track_id"].tolist() == [1, 2, 2, 3, 2]
        assert o["track_flags"][-2:].tolist() == [T.NEW | T.BEST, T.REVIVED] and o["track_hits"][-2:].tolist() == [1, 3]
        assert not lost["lost_i"][0, :, T.I_ID].any() and lost["lost_i"][0, 0, T.I_FIRST:].tolist() == [1, 1, 1, 1]
        assert state["hdr"][0].tolist() == [8, 4]
    return _case("forgotten", D, s, expect, T.LostPool(0.75, 6), max_age=2)


def ring(D):
    """max_age 0: every frame parks the face of the frame before.  65 persons, one per frame, fill the ring once round: the 65th
    sits in entry 0 where the first was.  The first returns (frame 66): nothing of it is left, it opens id 66.  The sixth returns
    (frame 67): revived as id 6."""
    ids = TC.spread(D, 65, 251)
    s = TC.Steps(D)
    for k in range(65):
        s.row(k, TC.cell(k), ids[k])
    s.row(66, TC.cell(70), ids[0]).row(67, TC.cell(71), ids[5]).end([0] * 68)

    def expect(outs, state, lost):
        o = outs[0]
        assert o["track_id"].tolist() == list(range(1, 66)) + [66, 6]
        assert o["track_flags"][-2:].tolist() == [T.NEW | T.BEST, T.REVIVED] and o["track_hits"][-1] == 2
        assert lost["lost_i"][0, 0, T.I_ID] == 65 and lost["lost_i"][0, 1, T.I_ID] == 66 and lost["lost_hdr"][0, 0] == 2
        assert lost["lost_i"][0, 5, T.I_ID] == 0 and (lost["lost_i"][0, :, T.I_ID] != 0).sum() == 63
        assert state["hdr"][0].tolist() == [68, 67]
    return _case("ring", D, s, expect, T.LostPool(0.75, 1000), max_age=0)


def full(D):
    """max_age 3.  P (frame 0) is parked in frame 4, where 32 faces open, 32 more in frame 5: 64 live slots.  P's face returns in
    frame 6: step 3b takes its entry, there is no slot, the row gets FULL and id 0 and P stays parked.  In frame 8 the first 32
    expire (and are parked behind P); P's face is there again and is revived into slot 0."""
    rng = np.random.default_rng(261)
    ids = TC.spread(D, 65, 261)
    s = TC.Steps(D)
    s.row(0, TC.cell(64), ids[64])
    for k in range(64):
        s.row(4 + k // 32, TC.cell(k), ids[k])
    s.row(6, TC.cell(80), TC.obs(ids[64], 0.9, rng)).row(8, TC.cell(81), TC.obs(ids[64], 0.92, rng)).end([0] * 9)

    def expect(outs, state, lost):
        o = outs[0]
        assert o["track_id"].tolist() == [1] + list(range(2, 66)) + [0, 1]
        assert o["track_flags"][-2:].tolist() == [T.FULL, T.REVIVED] and o["track_hits"][-2:].tolist() == [0, 2]
        assert state["slot_i"][0, 0, T.I_ID] == 1 and state["hdr"][0].tolist() == [9, 66]
        assert lost["lost_i"][0, 0, T.I_ID] == 0 and lost["lost_i"][0, 1:33, T.I_ID].tolist() == list(range(2, 34))
    return _case("poolfull", D, s, expect, T.LostPool(0.75, 50))


def dead_rows(D):
    """A pool that was handed over with four entries whose stored inverse norm is not live (inf, NaN, 0, -1) and one good entry
    (id 44, 7 hits).  The frame has the four bad entries' own embeddings as faces (cosine 1 if they could pair: each opens a new
    track), a zero, a NaN and an Inf embedding (dead rows) and a face at 0.9 of the good entry (revived: id 44, hits 8)."""
    z = TC.ortho(D, 6, 271)
    bad = [np.inf, np.nan, 0.0, -1.0]

    def lost_init(lost):
        for k, inv in enumerate(bad):
            lost["lost_i"][0, 5 + k] = [40 + k, 1, 0, 3, 1]
            lost["lost_f"][0, 5 + k, T.F_INV] = inv
            lost["lost_emb"][0, 5 + k] = z[k]
        lost["lost_i"][0, 9] = [44, 1, 0, 7, 1]
        lost["lost_f"][0, 9, T.F_INV] = 1.0
        lost["lost_emb"][0, 9] = z[4]
    nan_row, inf_row = z[4].copy(), z[4].copy()
    nan_row[1], inf_row[2] = np.nan, np.inf
    s = TC.Steps(D)
    for k in range(4):
        s.row(0, TC.cell(k), z[k])
    s.row(0, TC.cell(4), 0 * z[4]).row(0, TC.cell(5), nan_row).row(0, TC.cell(6), inf_row)
    s.row(0, TC.cell(7), TC.toward(z[4], z[5], 0.9)).end([0])

    def expect(outs, state, lost):
        o = outs[0]
        NB, DR = T.NEW | T.BEST, T.DEAD_ROW
        assert o["track_flags"].tolist() == [NB, NB, NB, NB, DR, DR, DR, T.REVIVED]
        assert o["track_id"].tolist() == [1, 2, 3, 4, 0, 0, 0, 44] and o["track_hits"][-1] == 8
        assert lost["lost_i"][0, 5:10, T.I_ID].tolist() == [40, 41, 42, 43, 0]
        assert state["hdr"][0].tolist() == [1, 5]
    return _case("deadpool", D, s, expect, T.LostPool(0.75, 50), lost_init=lost_init)


def best_shot(D):
    """max_age 2.  P (scores 0.8, 0.5) and Q (0.4, 0.3) are parked in frame 4.  In frame 5, behind a new face X that takes slot
    0: P returns with score 0.6, below its carried 0.8 -- REVIVED alone, and slot 1 (Q's old one) gets P's parked best embedding;
    Q returns with 0.7, above its 0.4 -- REVIVED | BEST.  In frame 6 P scores 0.9: BEST."""
    p, q, x, wp, wq, n1, n2, n3 = TC.ortho(D, 8, 281)
    p5 = TC.toward(MC.swing(p, wp, 0.98, 1), n1, 0.85)
    s = TC.Steps(D)
    s.row(0, TC.cell(0), p, score=0.8).row(0, TC.cell(1), q, score=0.4)
    s.row(1, TC.cell(0), MC.swing(p, wp, 0.98, 1), score=0.5).row(1, TC.cell(1), MC.swing(q, wq, 0.95, 1), score=0.3)
    s.row(5, TC.cell(9), x, score=0.5).row(5, TC.cell(20), p5, score=0.6)
    s.row(5, TC.cell(21), TC.toward(MC.swing(q, wq, 0.95, 1), n2, 0.88), score=0.7)
    s.row(6, TC.cell(20, dx=2.0), TC.toward(p5, n3, 0.97), score=0.9).end([0] * 7)
    first, sixth = (s.steps[0]["emb"][i].tobytes() for i in (0, 6))

    def expect(outs, state, lost):
        o = outs[0]
        NB = T.NEW | T.BEST
        assert o["track_flags"].tolist() == [NB, NB, 0, 0, NB, T.REVIVED, T.REVIVED | T.BEST, T.BEST]
        assert o["track_id"].tolist() == [1, 2, 1, 2, 3, 1, 2, 1] and o["track_hits"][-3:].tolist() == [3, 3, 4]
        assert state["slot_i"][0, :3, T.I_ID].tolist() == [3, 1, 2]
        assert state["slot_f"][0, 2, T.F_BEST_SCORE] == np.float32(0.7) and state["best_emb"][0, 2].tobytes() == sixth
        assert state["slot_i"][0, 2, T.I_BEST_CLOCK] == 6 and state["slot_i"][0, 1, T.I_BEST_CLOCK] == 7

    def expect_after_frame_5(outs, state, lost):
        assert state["slot_i"][0, 1].tolist() == [1, 1, 6, 3, 1] and state["slot_f"][0, 1, T.F_BEST_SCORE] == np.float32(0.8)
        assert state["best_emb"][0, 1].tobytes() == first and state["slot_f"][0, 1, T.F_BEST_BOX:].tolist() == TC.cell(0)
    case = _case("bestshot", D, s, expect, T.LostPool(0.75, 50), max_age=2)
    case["expect_after_frame_5"] = expect_after_frame_5
    return case


def with_motion(D):
    """A walks through frames 0 .. 3, is away and returns in the last frame (9), B stands throughout.  Run with motion=: the
    revived row's track_pred is zeros and the slot's filter is the one a fresh opening gets from that box."""
    a, b, wa, wb, n1 = TC.ortho(D, 5, 291)
    s = TC.Steps(D)
    for f in range(10):
        s.row(f, TC.cell(1, dx=float(f % 2)), MC.swing(b, wb, 0.95, f))
        if f <= 3:
            s.row(f, MC.box_at(20.0 + 12.0 * f), MC.swing(a, wa, 0.98, f))
    back = [400.0, 300.0, 452.0, 361.0]
    s.row(9, back, TC.toward(MC.swing(a, wa, 0.98, 3), n1, 0.85)).end([0] * 10)

    def expect(outs, state, lost):
        o = outs[0]
        assert o["track_id"][-1] == 2 and o["track_flags"][-1] == T.REVIVED and o["track_hits"][-1] == 5
        assert state["hdr"][0].tolist() == [10, 3]

    def expect_motion(outs, state, motion_state):
        assert outs[0]["track_pred"][-1].tolist() == [0.0] * 4 and (outs[0]["track_pred"][-2] != 0).any()
        slot = int(np.nonzero(state["slot_i"][0, :, T.I_ID] == 2)[0][0])
        fresh = np.zeros((T.MOTION_FLOATS,), np.float32)
        T._motion_init(fresh, np.asarray(back, np.float32), np.float32(MC.CV.std_pos), np.float32(MC.CV.std_vel))
        assert motion_state[0, slot].tobytes() == fresh.tobytes()
    case = _case("revivemotion", D, s, expect, T.LostPool(0.75, 50))
    case["expect_motion"] = expect_motion
    return case


CRAFTED = (revolving_door, same_frame, crossed_return, stranger, forgotten, ring, full, dead_rows, best_shot, with_motion)


def crafted_cases():
    return [fn(D) for fn in CRAFTED for D in DIMS]


def track_cases_in_every_configuration():
    """The crafted cases of track_cases.py (sorts of up to 2048 keys, 64 full slots, 65 rows, ties) made runnable by run_case with
    reid= and motion= on or off: DeepSORT's motion constants and a pool at tau_reid 0.6 that outlives the case's max_age.  The ids
    differ between the configurations (the pool revives where the plain tracker opens), so the cases' own `expect` is not called
    on them: what is compared is one path against another within a configuration."""
    cv = T.ConstantVelocity(T.ConstantVelocity.DEEPSORT_STD_POS, T.ConstantVelocity.DEEPSORT_STD_VEL)
    return [dict(c, reid=T.LostPool(0.6, c["max_age"] + 50), lost_init=None, motion=cv) for c in TC.crafted_cases()]


CONFIGS = [(False, False), (True, False), (False, True), (True, True)]      # (motion, reid)
CONFIG_IDS = ["plain", "motion", "reid", "motion+reid"]


# ------------------------------------------------------------------------------------------------ the batch of the properties

def busy(D, seed=5, n_streams=4, spare_streams=1):
    """track_cases.busy (max_age 2: faces leave for longer than that and return, over n_streams interleaved streams) with a pool:
    sightings of one person have cosines of 0.74 and more, two persons stay below 0.3, tau_reid = 0.55 lies between.
    spare_streams: further streams of the tracker that own no frame.  -> a one-step case."""
    base = TC.busy(D, seed=seed, n_streams=n_streams, max_age=2)
    return dict(base, name=f"reidbusy{seed}-D{D}", S=n_streams + spare_streams, reid=T.LostPool(0.55, 30), lost_init=None,
                motion=MC.CV)
