"""Tracklets with motion prediction on the host (no GPU): the numpy restatement against fp_tracklets_step_motion_emulate on every
case of motion_cases.py (the four per-row outputs, track_pred, the five state arrays and `motion`, equal, after the case passed
the cosine gap condition), the outcome each crafted case was built for with and without motion (and what mot_eval says of the
turning head), the properties (split, interleave, a stream without frames), the refusals, and header / binding agreement."""
import ctypes
import os
import re

import numpy as np
import pytest

import motion_cases as MC
import track_cases as TC
from face_detection_and_recognition_amd import _lib as L
from face_detection_and_recognition_amd import tracking as T
from face_detection_and_recognition_amd import tracking_eval as TE

CASES = MC.crafted_cases()
MOVING = [MC.moving(D) for D in MC.DIMS]
BY_NAME = {c["name"]: c for c in CASES + MOVING}


@pytest.fixture(scope="module")
def numpy_runs():
    """name -> (outs, state, motion_state, log) of the numpy run with motion of every case, made once."""
    return {c["name"]: MC.assert_gap(c) for c in CASES + MOVING}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_crafted_case_numpy_equals_emulator_and_states_its_outcome(case, numpy_runs):
    want = numpy_runs[case["name"]]
    case["expect"](*want[:2])
    got = MC.run_case(case, T.track_step_emulate)
    case["expect"](*got[:2])
    MC.assert_same(got, want, case["name"])
    for o in want[0]:
        matched = (o["track_id"] > 0) & (o["track_flags"] & T.NEW == 0)
        assert o["track_pred"].dtype == np.float32 and (o["track_pred"][~matched] == 0).all()


@pytest.mark.parametrize("name", [f"{n}-D{D}" for n in ("turning", "doorway") for D in MC.DIMS])
def test_motion_changes_the_answer_where_the_last_box_fails(name, numpy_runs):
    """The same rows without motion prediction: numpy and the emulator give the ids the stale box leads to."""
    case = BY_NAME[name]
    without = MC.assert_gap(case, motion=False)
    case["expect_without"](*without[:2])
    assert "track_pred" not in without[0][0]
    got = MC.run_case(case, T.track_step_emulate, motion=False)
    case["expect_without"](*got[:2])
    for log in (numpy_runs[name][3], without[3]):
        MC.assert_decisive_iou_gap(log)


@pytest.mark.parametrize("D", MC.DIMS)
def test_turning_head_keeps_one_identity(D, numpy_runs):
    """Every decisive IoU of the motion run is far above iou_min (frame 2: about 0.88); mot_eval counts no identity switch with
    motion and one per frame without."""
    case = BY_NAME[f"turning-D{D}"]
    outs, _, _, log = numpy_runs[case["name"]]
    decisive = MC.assert_decisive_iou_gap(log)
    assert len(decisive) == 9 and 0.86 < decisive[0] < 0.90 and decisive.min() > 0.5
    gf, gi, gb = case["gt"]
    z = np.zeros_like
    res = {}
    for motion in (True, False):
        o = outs if motion else MC.run_case(case, T.track_step_numpy, motion=False)[0]
        hf, hi, hb = MC.mot_rows(case, o)
        res[motion] = TE.mot_eval(z(gf), gf, gi, gb, z(hf), hf, hi, hb, [11])
        assert res[motion].TP == 11 and res[motion].FN == 0
    assert res[True].IDSW == 0 and res[True].IDF1 == 1.0
    assert res[False].IDSW == 9


@pytest.mark.parametrize("D", MC.DIMS)
def test_static_faces_get_the_same_ids_with_and_without_motion(D, numpy_runs):
    case = BY_NAME[f"static-D{D}"]
    outs, _, motion, _ = numpy_runs[case["name"]]
    without = MC.run_case(case, T.track_step_numpy, motion=False)[0]
    for key in T.OUT_KEYS:
        assert np.array_equal(outs[0][key], without[0][key]), key
    assert (motion[0, :4].reshape(4, 4, T.M_COLS)[:, :, T.M_V] == 0).all()


@pytest.mark.parametrize("case", MOVING, ids=[c["name"] for c in MOVING])
def test_moving_batch_numpy_equals_emulator(case, numpy_runs):
    want = numpy_runs[case["name"]]
    o = want[0][0]
    assert (o["track_id"] > 0).sum() > 200 and (want[1]["hdr"][:, 1] - 1).min() >= 6
    tn, tf = float(np.float32(T.TAU_NEAR)), float(np.float32(T.TAU_FAR))
    band = sum(int(((e[3] > tn) & (e[3] <= tf) & (e[4] > np.float32(T.IOU_MIN))).sum()) for e in want[3])
    assert band > 10                                                           # pairs that only the IoU gate admits
    assert (want[2].reshape(case["S"], T.SLOTS, 4, T.M_COLS)[:, :, :, T.M_V] != 0).any()
    MC.assert_same(MC.run_case(case, T.track_step_emulate), want, case["name"])


@pytest.mark.parametrize("step_fn", [T.track_step_numpy, T.track_step_emulate], ids=["numpy", "emulate"])
def test_split_anywhere_changes_nothing(step_fn, numpy_runs):
    """One step equals the same frames as two steps cut at ANY frame: the filters are carried by `motion` alone."""
    case = MOVING[0]
    (whole,), state, motion, _ = numpy_runs[case["name"]]
    B = len(case["steps"][0]["stream_of_frame"])
    for k in range(0, B + 1):
        two, rows = TC.split_case(case, k)
        outs, st, m = MC.run_case(two, step_fn)
        for part, r in zip(outs, rows):
            for key in MC.OUT_KEYS:
                assert np.array_equal(part[key], whole[key][r]), (k, key)
        TC.assert_same_state(st, state, f"split at {k}")
        MC.assert_same_motion(m, motion, f"split at {k}")


@pytest.mark.parametrize("step_fn", [T.track_step_numpy, T.track_step_emulate], ids=["numpy", "emulate"])
def test_interleaved_streams_equal_each_stream_alone(step_fn, numpy_runs):
    case = MOVING[0]
    (whole,), state, motion, _ = numpy_runs[case["name"]]
    for s in range(case["S"]):
        alone, rows = TC.stream_alone(case, s)
        (out,), st, m = MC.run_case(alone, step_fn)
        assert len(rows) > 0
        for key in MC.OUT_KEYS:
            assert np.array_equal(out[key], whole[key][rows]), (s, key)
        for key in T.STATE_KEYS:
            assert st[key][0].tobytes() == state[key][s].tobytes(), (s, key)
        assert m[0].tobytes() == motion[s].tobytes(), s


@pytest.mark.parametrize("step_fn", [T.track_step_numpy, T.track_step_emulate], ids=["numpy", "emulate"])
def test_a_stream_without_frames_keeps_its_motion_untouched(step_fn, numpy_runs):
    """A fourth stream that owns no frame: whatever its rows of `motion` and of the state held stays, bit for bit; the other
    streams answer as without it."""
    case = MC.moving(32, spare_streams=1)
    (whole,), state, motion, _ = numpy_runs[MOVING[0]["name"]]
    marks = (np.arange(T.SLOTS * T.MOTION_FLOATS, dtype=np.float32).reshape(T.SLOTS, T.MOTION_FLOATS) - 300) * np.float32(0.37)
    m0 = T.new_motion_state(4)
    m0[3] = marks
    st0 = T.new_state(4, 32)
    st0["slot_i"][3, 5] = [9, 1, 2, 3, 1]                     # a live track nobody predicts: the stream has no frame
    st0["hdr"][3] = [2, 10]
    (out,), st, m = MC.run_case(case, step_fn, state=st0, motion_state=m0)
    assert m[3].tobytes() == marks.tobytes() and st["hdr"][3].tolist() == [2, 10] and st["slot_i"][3, 5].tolist() == [9, 1, 2, 3, 1]
    for key in MC.OUT_KEYS:
        assert np.array_equal(out[key], whole[key]), key
    assert m[:3].tobytes() == motion.tobytes()


# ------------------------------------------------------------------------------------------------ refusals, ABI, header

def test_refusals(lib):
    p = lambda a: ctypes.c_void_p(a.ctypes.data)                     # noqa: E731
    D, n, B = 32, 2, 2
    st = T.new_state(1, D)
    r = dict(frame=np.zeros((n,), np.int32), box=np.zeros((n, 4), np.float32), emb=np.ones((n, D), np.float32),
             xinv=np.ones((n,), np.float32), sof=np.zeros((B,), np.int32), motion=T.new_motion_state(1),
             pred=np.zeros((n, 4), np.float32))
    outs = [np.zeros((n,), np.int32) for _ in range(4)]
    struct = L.FpTrackState(*[p(st[k]) for k in T.STATE_KEYS])

    def call(fn=lib.fp_tracklets_step_motion_emulate, state=struct, S=1, D=32, n=2, B=2, max_age=1, tn=0.5, tf=0.7, im=0.1, sp=0.05,
             sv=0.01, tail=(), **ptr):
        a = {k: p(v) for k, v in r.items()}
        a.update(ptr)
        o = [p(x) for x in outs]
        if "out" in ptr:
            o[ptr["out"]] = None
        return fn(None if state is None else ctypes.byref(state), S, D, a["frame"], a["box"], a["emb"], a["xinv"], None, n, a["sof"], B,
                  max_age, tn, tf, im, *o, a["motion"], sp, sv, a["pred"], *tail)
    assert call() == L.FP_OK
    inf, nan = float("inf"), float("nan")
    for kw in (dict(D=30), dict(D=1028), dict(D=0), dict(S=0), dict(n=-1), dict(B=-1), dict(max_age=-1), dict(tn=0.8, tf=0.7),
               dict(tn=nan), dict(tf=nan), dict(im=nan), dict(state=None), dict(frame=None), dict(box=None), dict(emb=None),
               dict(xinv=None), dict(sof=None), dict(out=0), dict(out=3),                   # what fp_tracklets_step refuses
               dict(motion=None), dict(pred=None), dict(sp=0.0), dict(sp=-0.05), dict(sp=nan), dict(sp=inf), dict(sv=0.0),
               dict(sv=-1.0), dict(sv=nan), dict(sv=inf)):
        assert call(**kw) == L.FP_ERR_INVALID_ARG, kw
        assert call(fn=lib.fp_tracklets_step_motion, tail=(None,), **kw) == L.FP_ERR_INVALID_ARG, kw   # before any HIP call
    for k in T.STATE_KEYS:                                           # a NULL state array
        bad = L.FpTrackState(*[None if j == k else p(st[j]) for j in T.STATE_KEYS])
        assert call(state=bad) == L.FP_ERR_INVALID_ARG, k
    odd = np.ones((2 * 32 + 1,), np.float32)[1:]                     # rows that are not 16-byte aligned
    assert call(emb=ctypes.c_void_p(odd.ctypes.data)) == L.FP_ERR_INVALID_ARG
    assert call(n=0, frame=None, box=None, emb=None, xinv=None, pred=None) == L.FP_OK     # empty frames alone need no track_pred
    assert call(n=0, motion=None) == L.FP_ERR_INVALID_ARG
    assert lib.fp_abi_version() == 15                                # additions only


def test_python_refusals():
    CV = T.ConstantVelocity
    for a in ((0, 0.1), (0.1, 0), (-1, 0.1), (float("nan"), 0.1), (0.1, float("inf"))):
        with pytest.raises(ValueError):
            CV(*a)
    with pytest.raises(TypeError):
        CV()                                                         # no defaults
    with pytest.raises(TypeError):
        CV(0.05)
    assert (CV.DEEPSORT_STD_POS, CV.DEEPSORT_STD_VEL) == (1 / 20, 1 / 160)
    cv = CV(CV.DEEPSORT_STD_POS, CV.DEEPSORT_STD_VEL)
    assert (cv.std_pos, cv.std_vel) == (0.05, 0.00625)
    with pytest.raises(TypeError):
        T.StreamTracker(1, 32, 1, device="cpu", motion=(0.05, 0.01))
    st = T.new_state(1, 32)
    rows = ([0], np.zeros((1, 4)), np.ones((1, 32)), [1.0], [0], 1)
    for fn in (T.track_step_numpy, T.track_step_emulate):
        with pytest.raises(ValueError):
            fn(st, *rows, motion_state=T.new_motion_state(1))        # a state without the parameters
        with pytest.raises(ValueError):
            fn(st, *rows, motion=cv)                                 # the parameters without a state
        with pytest.raises(ValueError):
            fn(st, *rows, motion=cv, motion_state=T.new_motion_state(2))
        with pytest.raises(ValueError):
            fn(st, *rows, motion=cv, motion_state=T.new_motion_state(1).astype(np.float64))
    assert T.new_motion_state(3).shape == (3, L.TRACK_SLOTS, L.TRACK_MOTION_FLOATS) and not T.new_motion_state(3).any()


def test_header_and_bindings_agree():
    from conftest import ROOT
    hdr = open(os.path.join(ROOT, "include", "facepath.h")).read()
    assert f"#define FP_TRACK_MOTION_FLOATS {L.TRACK_MOTION_FLOATS}\n" in hdr and L.TRACK_MOTION_FLOATS == 20 == 4 * T.M_COLS
    assert f"#define FP_TRACK_SLOT_FLOATS {L.TRACK_SLOT_FLOATS}\n" in hdr and L.TRACK_SLOT_FLOATS == 10
    n_args = {}
    for fn in ("fp_tracklets_step", "fp_tracklets_step_emulate", "fp_tracklets_step_motion", "fp_tracklets_step_motion_emulate"):
        decl = re.search(r"\nint " + fn + r"\(([^;]*)\);", hdr).group(1)
        n_args[fn] = len([a for a in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",") if a.strip()])
        assert n_args[fn] == len(L.SIGNATURES[fn][1]), fn
    assert n_args["fp_tracklets_step_motion"] == n_args["fp_tracklets_step"] + 4 == 24
    assert n_args["fp_tracklets_step_motion_emulate"] == n_args["fp_tracklets_step_emulate"] + 4 == 23
    fields = re.search(r"typedef struct fp_track_state \{(.*?)\} fp_track_state;", hdr, re.S).group(1)
    assert re.findall(r"\*\s*(\w+);", fields) == list(T.STATE_KEYS) and len(T.STATE_KEYS) == 5
    assert 'Tracklets: motion prediction' in hdr
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "fp_tracklets_step_motion" in integ and "fp_tracklets_step_motion_emulate" in integ


def test_drivers_take_motion_and_sweep_its_parameters():
    from face_detection_and_recognition_amd.eval import eval_face_tracker as ET
    from face_detection_and_recognition_amd.face_extraction import track_faces_in_frames as TF
    assert ET.parse_sweep("std_pos=0.05,0.1") == ("std_pos", [0.05, 0.1]) and ET.parse_sweep("std_vel=0.00625") == ("std_vel", [0.00625])
    args = TF.get_parsed_args(["--frames", "x", "--max_age", "3", "--motion", "0.05", "0.00625"])
    assert args.motion == [0.05, 0.00625] and T.ConstantVelocity(*args.motion).std_vel == 0.00625
    assert TF.get_parsed_args(["--frames", "x", "--max_age", "3"]).motion is None          # opt-in
    with pytest.raises(SystemExit):
        TF.get_parsed_args(["--frames", "x", "--max_age", "3", "--motion", "0.05"])       # both values or none
