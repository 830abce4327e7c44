"""Tracklets with re-identification on the host (no GPU): the numpy restatement against fp_tracklets_step_reid_emulate on every case
of reid_cases.py, with and without motion (the per-row outputs, track_pred, the five state arrays, `motion` and the five lost_*
arrays, equal, after the case passed the gap condition of steps 2 and 3b), the outcome each crafted case was built for (and what
mot_eval says of the revolving door), the properties (split anywhere, interleaved, scattered, a stream without frames), the
refusals, header / binding agreement, the state keys of StreamTracker, TrackBook across a revival, and --reid on the drivers."""
import ctypes
import os
import re

import numpy as np
import pytest

import motion_cases as MC
import reid_cases as RC
import track_cases as TC
from face_detection_and_recognition_amd import _lib as L
from face_detection_and_recognition_amd import tracking as T
from face_detection_and_recognition_amd import tracking_eval as TE

CASES = RC.crafted_cases()
BUSY = [RC.busy(D) for D in RC.DIMS]
BY_NAME = {c["name"]: c for c in CASES + BUSY}
TRACK = RC.track_cases_in_every_configuration()
STEP_FNS = pytest.mark.parametrize("step_fn", [T.track_step_numpy, T.track_step_emulate], ids=["numpy", "emulate"])


@pytest.fixture(scope="module")
def numpy_runs():
    """(name, motion) -> (outs, state, motion_state, lost_state, reid log) of the numpy run of every case, made once."""
    return {(c["name"], m): RC.assert_gap(c, motion=m) for c in CASES + BUSY for m in (False, True)}


@pytest.mark.parametrize("motion", [False, True], ids=["plain", "motion"])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_crafted_case_numpy_equals_emulator_and_states_its_outcome(case, motion, numpy_runs):
    want = numpy_runs[case["name"], motion]
    case["expect"](want[0], want[1], want[3])
    got = RC.run_case(case, T.track_step_emulate, motion=motion)
    case["expect"](got[0], got[1], got[3])
    RC.assert_same(got, want, case["name"])
    if motion and "expect_motion" in case:
        case["expect_motion"](*got[:3])
    for o in want[0]:                                     # a revived row is never NEW; without an id no REVIVED
        rev = o["track_flags"] & T.REVIVED != 0
        assert not (o["track_flags"][rev] & T.NEW).any() and (o["track_id"][rev] > 0).all()
        if motion:
            assert (o["track_pred"][rev] == 0).all()


@pytest.mark.parametrize("motion,reid", RC.CONFIGS, ids=RC.CONFIG_IDS)
@pytest.mark.parametrize("case", TRACK, ids=[c["name"] for c in TRACK])
def test_track_case_numpy_equals_emulator_in_every_configuration(case, motion, reid):
    """The crafted cases of track_cases.py through all four kernels' host twin: the one sort, walk and pair scorer at 2048 keys,
    64 full slots, 65 rows and ties, under the gap condition of steps 2 and 3b."""
    want = RC.assert_gap(case, reid=reid, motion=motion)[:4]
    RC.assert_same(RC.run_case(case, T.track_step_emulate, reid=reid, motion=motion), want, case["name"])


@pytest.mark.parametrize("D", RC.DIMS)
def test_revolving_door_keeps_the_id_and_the_scorer_sees_it(D, numpy_runs):
    """Without the pool (track_step_numpy and the emulator as they stand) the returning face is id 4 and costs an identity switch;
    with it, none."""
    case = BY_NAME[f"door-D{D}"]
    gf, gi, gb = case["gt"]
    z = np.zeros_like
    res = {}
    for reid in (True, False):
        outs = numpy_runs[case["name"], False][0] if reid else RC.run_case(case, T.track_step_numpy, reid=False)[0]
        if not reid:
            for fn in (T.track_step_numpy, T.track_step_emulate):
                case["expect_without"](*RC.run_case(case, fn, reid=False)[:2])
        hf, hi, hb = MC.mot_rows(case, outs)
        res[reid] = TE.mot_eval(z(gf), gf, gi, gb, z(hf), hf, hi, hb, [22])
        assert res[reid].TP == 37 and res[reid].FN == 0 and res[reid].FP == 0
    assert res[False].IDSW == 1 and round(res[False].IDF1, 4) == 0.8649
    assert res[True].IDSW == 0 and res[True].IDF1 == 1.0


@pytest.mark.parametrize("D", RC.DIMS)
def test_best_shot_is_carried_across_the_gap(D):
    """After the frame of the revival alone: P sits in Q's old slot with its own carried best score, box, clock and embedding."""
    case = BY_NAME[f"bestshot-D{D}"]
    head, _ = TC.split_case(case, 6)
    for fn in (T.track_step_numpy, T.track_step_emulate):
        outs, state, _, lost = RC.run_case(dict(head, steps=head["steps"][:1]), fn)
        case["expect_after_frame_5"](outs, state, lost)


@pytest.mark.parametrize("motion", [False, True], ids=["plain", "motion"])
@pytest.mark.parametrize("case", BUSY, ids=[c["name"] for c in BUSY])
def test_busy_batch_numpy_equals_emulator(case, motion, numpy_runs):
    want = numpy_runs[case["name"], motion]
    flags = RC.flags_of(want[0])
    assert (flags & T.REVIVED != 0).sum() >= 8 and (flags & T.NEW != 0).sum() >= 8 and len(want[4]) >= 3
    RC.assert_same(RC.run_case(case, T.track_step_emulate, motion=motion), want, case["name"])


@pytest.mark.parametrize("motion", [False, True], ids=["plain", "motion"])
@STEP_FNS
def test_split_anywhere_changes_nothing(step_fn, motion, numpy_runs):
    """One step equals the same frames as two steps cut at ANY frame: the pool is carried by the lost_* arrays alone."""
    case = BUSY[0]
    (whole,), state, mstate, lost, _ = numpy_runs[case["name"], motion]
    B = len(case["steps"][0]["stream_of_frame"])
    for k in range(0, B + 1):
        two, rows = TC.split_case(case, k)
        outs, st, m, lo = RC.run_case(two, step_fn, motion=motion)
        for part, r in zip(outs, rows):
            for key in whole:
                assert np.array_equal(part[key], whole[key][r]), (k, key)
        TC.assert_same_state(st, state, f"split at {k}")
        MC.assert_same_motion(m, mstate, f"split at {k}")
        RC.assert_same_lost(lo, lost, f"split at {k}")


@STEP_FNS
def test_interleaved_streams_equal_each_stream_alone(step_fn, numpy_runs):
    case = BUSY[0]
    (whole,), state, _, lost, _ = numpy_runs[case["name"], False]
    for s in range(4):
        alone, rows = TC.stream_alone(case, s)
        (out,), st, _, lo = RC.run_case(alone, step_fn)
        assert len(rows) > 0
        for key in T.OUT_KEYS:
            assert np.array_equal(out[key], whole[key][rows]), (s, key)
        for key in T.STATE_KEYS:
            assert st[key][0].tobytes() == state[key][s].tobytes(), (s, key)
        for key in T.LOST_KEYS:
            assert lo[key][0].tobytes() == lost[key][s].tobytes(), (s, key)


@STEP_FNS
def test_scattered_rows_equal_contiguous_rows(step_fn, numpy_runs):
    case = BUSY[0]
    (whole,), state, _, lost, _ = numpy_runs[case["name"], False]
    mixed, perm = TC.scattered(case)
    (out,), st, _, lo = RC.run_case(mixed, step_fn)
    for key in T.OUT_KEYS:
        assert np.array_equal(out[key], whole[key][perm]), key
    TC.assert_same_state(st, state, "scattered")
    RC.assert_same_lost(lo, lost, "scattered")


@STEP_FNS
def test_a_stream_without_frames_keeps_its_pool_untouched(step_fn, numpy_runs):
    """The fifth stream owns no frame: whatever its pool rows and its ring head held stays, bit for bit."""
    case = BUSY[0]
    (whole,), state, _, lost, _ = numpy_runs[case["name"], False]
    l0 = T.new_lost_state(case["S"], case["D"])
    l0["lost_hdr"][4] = [77, -3]
    l0["lost_i"][4, 9] = [5, 1, 2, 3, 1]
    l0["lost_f"][4] = (np.arange(T.LOST * L.TRACK_SLOT_FLOATS, dtype=np.float32).reshape(T.LOST, -1) - 100) * np.float32(0.37)
    marks = {k: l0[k][4].copy() for k in T.LOST_KEYS}
    (out,), st, _, lo = RC.run_case(case, step_fn, lost_state=l0)
    for k in T.LOST_KEYS:
        assert lo[k][4].tobytes() == marks[k].tobytes(), k
        assert lo[k][:4].tobytes() == lost[k][:4].tobytes(), k
    for key in T.OUT_KEYS:
        assert np.array_equal(out[key], whole[key]), key


# ------------------------------------------------------------------------------------------------ refusals, ABI, header

def test_refusals(lib):
    p = lambda a: ctypes.c_void_p(a.ctypes.data)                     # noqa: E731
    D, n, B = 32, 2, 2
    st, lo = T.new_state(1, D), T.new_lost_state(1, D)
    r = dict(frame=np.zeros((n,), np.int32), box=np.zeros((n, 4), np.float32), emb=np.ones((n, D), np.float32),
             xinv=np.ones((n,), np.float32), sof=np.zeros((B,), np.int32), motion=T.new_motion_state(1),
             pred=np.zeros((n, 4), np.float32))
    outs = [np.zeros((n,), np.int32) for _ in range(4)]
    struct = L.FpTrackState(*[p(st[k]) for k in T.STATE_KEYS])
    lstruct = L.FpTrackLost(*[p(lo[k]) for k in T.LOST_KEYS])

    def call(fn=lib.fp_tracklets_step_reid_emulate, state=struct, lost=lstruct, S=1, D=32, n=2, B=2, max_age=1, tn=0.5, tf=0.7,
             im=0.1, tr=0.75, la=5, sp=0.05, sv=0.01, tail=(), **ptr):
        a = {k: p(v) for k, v in r.items()}
        a.update(ptr)
        o = [p(x) for x in outs]
        if "out" in ptr:
            o[ptr["out"]] = None
        return fn(None if state is None else ctypes.byref(state), None if lost is None else ctypes.byref(lost), S, D, a["frame"],
                  a["box"], a["emb"], a["xinv"], None, n, a["sof"], B, max_age, tn, tf, im, *o, tr, la, a["motion"], sp, sv,
                  a["pred"], *tail)
    inf, nan = float("inf"), float("nan")
    assert call() == L.FP_OK                                         # with motion
    assert call(motion=None, pred=None, sp=nan, sv=nan) == L.FP_OK   # without: std_pos / std_vel are not looked at
    for base in (dict(), dict(motion=None, pred=None)):
        for kw in (dict(D=30), dict(D=1028), dict(D=0), dict(S=0), dict(n=-1), dict(B=-1), dict(max_age=-1), dict(tn=0.8, tf=0.7),
                   dict(tn=nan), dict(tf=nan), dict(im=nan), dict(state=None), dict(frame=None), dict(box=None), dict(emb=None),
                   dict(xinv=None), dict(sof=None), dict(out=0), dict(out=3),               # what fp_tracklets_step refuses
                   dict(lost=None), dict(la=1), dict(la=0), dict(la=-7), dict(max_age=5), dict(tr=nan), dict(tr=inf),
                   dict(tr=-inf)):
            kw = dict(base, **kw)
            assert call(**kw) == L.FP_ERR_INVALID_ARG, kw
            assert call(fn=lib.fp_tracklets_step_reid, tail=(None,), **kw) == L.FP_ERR_INVALID_ARG, kw   # before any HIP call
    for kw in (dict(pred=None), dict(sp=0.0), dict(sp=nan), dict(sv=-1.0), dict(sv=inf),  # what fp_tracklets_step_motion refuses
               dict(motion=None)):                                                        # track_pred without motion
        assert call(**kw) == L.FP_ERR_INVALID_ARG, kw
    for k in T.STATE_KEYS:                                           # a NULL state array, a NULL pool array
        bad = L.FpTrackState(*[None if j == k else p(st[j]) for j in T.STATE_KEYS])
        assert call(state=bad) == L.FP_ERR_INVALID_ARG, k
    for k in T.LOST_KEYS:
        bad = L.FpTrackLost(*[None if j == k else p(lo[j]) for j in T.LOST_KEYS])
        assert call(lost=bad) == L.FP_ERR_INVALID_ARG, k
        assert call(lost=bad, motion=None, pred=None) == L.FP_ERR_INVALID_ARG, k
    odd = np.ones((2 * 32 + 1,), np.float32)[1:]                     # rows that are not 16-byte aligned
    assert call(emb=ctypes.c_void_p(odd.ctypes.data)) == L.FP_ERR_INVALID_ARG
    oddpool = np.zeros((T.LOST * 32 + 1,), np.float32)[1:]
    for k in ("lost_emb", "lost_best_emb"):
        bad = L.FpTrackLost(*[ctypes.c_void_p(oddpool.ctypes.data) if j == k else p(lo[j]) for j in T.LOST_KEYS])
        assert call(lost=bad, motion=None, pred=None) == L.FP_ERR_INVALID_ARG, k
    assert call(tr=-0.5, motion=None, pred=None) == L.FP_OK          # a cosine: any finite value
    assert call(n=0, frame=None, box=None, emb=None, xinv=None, pred=None, motion=None) == L.FP_OK      # empty frames alone
    assert lib.fp_abi_version() == 15                                # additions only


def test_python_refusals():
    LP = T.LostPool
    for a in ((float("nan"), 10), (float("inf"), 10), (0.7, 2.5), (0.7, "x")):
        with pytest.raises((ValueError, TypeError)):
            LP(*a)
    with pytest.raises(TypeError):
        LP()                                                         # no defaults
    with pytest.raises(TypeError):
        LP(0.7)
    pool = LP(0.7, 4)
    assert (pool.tau_reid, pool.lost_age) == (0.7, 4)
    for max_age in (4, 5):                                           # lost_age must be > max_age
        with pytest.raises(ValueError):
            T.StreamTracker(1, 32, max_age, device="cpu", reid=pool)
    with pytest.raises(TypeError):
        T.StreamTracker(1, 32, 1, device="cpu", reid=(0.7, 4))
    st = T.new_state(1, 32)
    rows = ([0], np.zeros((1, 4)), np.ones((1, 32)), [1.0], [0])
    for fn in (T.track_step_numpy, T.track_step_emulate):
        with pytest.raises(ValueError):
            fn(st, *rows, 1, lost_state=T.new_lost_state(1, 32))     # a pool without the parameters
        with pytest.raises(ValueError):
            fn(st, *rows, 1, reid=pool)                              # the parameters without a pool
        with pytest.raises(ValueError):
            fn(st, *rows, 1, reid=pool, lost_state=T.new_lost_state(2, 32))
        with pytest.raises(ValueError):
            fn(st, *rows, 1, reid=pool, lost_state=T.new_lost_state(1, 64))
        with pytest.raises(ValueError):
            fn(st, *rows, 4, reid=pool, lost_state=T.new_lost_state(1, 32))
    fresh = T.new_lost_state(3, 32)
    assert tuple(fresh) == T.LOST_KEYS and not any(v.any() for v in fresh.values())
    assert fresh["lost_i"].shape == (3, L.TRACK_LOST, L.TRACK_SLOT_INTS) and fresh["lost_best_emb"].shape == (3, 64, 32)


def test_header_and_bindings_agree():
    from conftest import ROOT
    hdr = open(os.path.join(ROOT, "include", "facepath.h")).read()
    assert f"#define FP_TRACK_LOST {L.TRACK_LOST}\n" in hdr and L.TRACK_LOST == 64 == T.LOST
    assert f"#define FP_TRACK_REVIVED {L.TRACK_REVIVED}\n" in hdr and L.TRACK_REVIVED == 64 == T.REVIVED
    assert "#define FP_ABI_VERSION 15\n" in hdr and L.ABI_VERSION == 15
    n_args = {}
    for fn in ("fp_tracklets_step", "fp_tracklets_step_reid", "fp_tracklets_step_reid_emulate"):
        decl = re.search(r"\nint " + fn + r"\(([^;]*)\);", hdr).group(1)
        n_args[fn] = len([a for a in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",") if a.strip()])
        assert n_args[fn] == len(L.SIGNATURES[fn][1]), fn
    assert n_args["fp_tracklets_step_reid"] == n_args["fp_tracklets_step"] + 7 == 27
    assert n_args["fp_tracklets_step_reid_emulate"] == 26
    fields = re.search(r"typedef struct fp_track_lost \{(.*?)\} fp_track_lost;", hdr, re.S).group(1)
    assert re.findall(r"\*\s*(\w+);", fields) == [f[0] for f in L.FpTrackLost._fields_] == list(T.LOST_KEYS)
    fields = re.search(r"typedef struct fp_track_state \{(.*?)\} fp_track_state;", hdr, re.S).group(1)
    assert re.findall(r"\*\s*(\w+);", fields) == list(T.STATE_KEYS) and len(T.STATE_KEYS) == 5
    assert "Tracklets: re-identification" in hdr
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "fp_tracklets_step_reid" in integ and "fp_tracklets_step_reid_emulate" in integ
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Tracklets: re-identification" in design
    assert "Out of scope: re-identification of an expired track" not in design


def test_tracker_state_keys_and_loading():
    """On the CPU device nothing is launched: the state handling alone.  A state saved without reid loads into a tracker with it
    only with the lost_* keys present; the other way round they are ignored."""
    pool = T.LostPool(0.7, 9)
    plain = T.StreamTracker(2, 32, 3, device="cpu")
    both = T.StreamTracker(2, 32, 3, device="cpu", reid=pool, motion=MC.CV)
    with_pool = T.StreamTracker(2, 32, 3, device="cpu", reid=pool)
    assert plain.state_keys == T.STATE_KEYS and with_pool.state_keys == T.STATE_KEYS + T.LOST_KEYS
    assert both.state_keys == T.STATE_KEYS + ("motion",) + T.LOST_KEYS
    saved = plain.state_dict()
    assert set(saved) == set(T.STATE_KEYS) | {"params"}
    with pytest.raises(KeyError):
        with_pool.load_state_dict(saved)
    with_pool.load_state_dict(dict(saved, **{k: v for k, v in T.new_lost_state(2, 32).items()}))
    d = with_pool.state_dict()
    assert d["params"]["tau_reid"] == 0.7 and d["params"]["lost_age"] == 9 and set(T.LOST_KEYS) <= set(d)
    plain.load_state_dict(d)                                         # the pool is ignored
    assert set(plain.host_state()) == set(T.STATE_KEYS)
    with pytest.raises(ValueError):
        T.StreamTracker(1, 32, 3, device="cpu", reid=pool).load_state_dict(d)        # another n_streams
    with pytest.raises(ValueError):
        plain.lost(0)
    lo = T.new_lost_state(2, 32)
    lo["lost_i"][1, 3] = [8, 1, 2, 3, 1]
    lo["lost_f"][1, 3, T.F_BEST_SCORE] = 0.5
    lo["lost_best_emb"][1, 3] = 2.0
    with_pool.load_state_dict(dict(saved, **lo))
    got = with_pool.lost(1)
    assert got["entry"].tolist() == [3] and got["id"].tolist() == [8] and got["hits"].tolist() == [3]
    assert got["last_clock"].tolist() == [2] and got["best_score"].tolist() == [0.5] and (got["best_emb"] == 2.0).all()
    assert len(with_pool.lost(0)["id"]) == 0
    with_pool.reset([1])
    assert len(with_pool.lost(1)["id"]) == 0 and not with_pool.host_state()["lost_best_emb"].any()


@pytest.mark.parametrize("D", RC.DIMS)
def test_trackbook_keeps_one_record_across_the_gap(D, numpy_runs):
    """A REVIVED row is not NEW: the book's record of the id goes on (first clock, best shot), where without the pool the
    returning face starts a second record."""
    case = BY_NAME[f"door-D{D}"]
    st = case["steps"][0]
    for reid in (True, False):
        outs = numpy_runs[case["name"], False][0] if reid else RC.run_case(case, T.track_step_numpy, reid=False)[0]
        book = T.TrackBook()
        book.update(outs[0], st["frame"], st["boxes"], st["stream_of_frame"], emb=st["emb"])
        assert len(book) == (3 if reid else 4)
        rec = book[(0, 2)]
        assert rec["first_clock"] == 1 and rec["best_clock"] == 1 and rec["best_frame"] == 0
        assert (rec["hits"], rec["last_clock"]) == ((10, 22) if reid else (5, 5))


def test_drivers_take_reid_and_sweep_its_parameters():
    from face_detection_and_recognition_amd.eval import eval_face_tracker as ET
    from face_detection_and_recognition_amd.face_extraction import track_faces_in_frames as TF
    assert ET.parse_sweep("tau_reid=0.6,0.7") == ("tau_reid", [0.6, 0.7]) and ET.parse_sweep("lost_age=30,60") == ("lost_age", [30, 60])
    args = TF.get_parsed_args(["--frames", "x", "--max_age", "3", "--reid", "0.7", "30"])
    assert args.reid == [0.7, 30.0] and TF.lost_pool(args).lost_age == 30 and TF.lost_pool(args).tau_reid == 0.7
    plain = TF.get_parsed_args(["--frames", "x", "--max_age", "3"])
    assert plain.reid is None and TF.lost_pool(plain) is None         # opt-in
    with pytest.raises(SystemExit):
        TF.get_parsed_args(["--frames", "x", "--max_age", "3", "--reid", "0.7"])      # both values or none
    with pytest.raises(ValueError):
        TF.lost_pool(TF.get_parsed_args(["--frames", "x", "--max_age", "3", "--reid", "0.7", "30.5"]))
