"""Tracklets with motion prediction on the device: fp_tracklets_step_motion against the numpy restatement on every case of
motion_cases.py (the four per-row outputs, track_pred, the five state arrays and `motion`, equal, under each case's gap
condition), the turning head scored by mot_eval on the device, the properties on the device (split, interleave, a stream
without frames, two runs bit-identical), the state round trip, tracks(), reset, FacePipeline(tracker=) with motion, and
--motion on the two tracking drivers."""
import numpy as np
import pytest
import torch

import motion_cases as MC
import track_cases as TC
from face_detection_and_recognition_amd import tracking as T
from face_detection_and_recognition_amd import tracking_eval as TE

pytestmark = pytest.mark.gpu

CASES = MC.crafted_cases()
MOVING = [MC.moving(D) for D in MC.DIMS]
BY_NAME = {c["name"]: c for c in CASES + MOVING}


@pytest.fixture(scope="module")
def numpy_runs():
    return {c["name"]: MC.assert_gap(c) for c in CASES + MOVING}


def to_dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def device_step(dev):
    """A step_fn for MC.run_case: a fresh StreamTracker per call, the host state (and `motion`) loaded into it, one launch, the
    state read back (so every step also crosses load_state_dict / host_state)."""
    def step(state, frame, boxes, emb, xinv, stream_of_frame, max_age, score=None, motion=None, motion_state=None, **params):
        tr = T.StreamTracker(state["hdr"].shape[0], state["emb"].shape[2], max_age, device=dev, motion=motion, **params)
        tr.load_state_dict(dict(state, motion=motion_state) if motion is not None else state)
        out = tr.step(to_dev(frame, dev), to_dev(boxes, dev), to_dev(emb, dev), to_dev(stream_of_frame, dev),
                      score=to_dev(score, dev), xinv=to_dev(xinv, dev))
        torch.cuda.synchronize()
        host = tr.host_state()
        for k in T.STATE_KEYS:
            state[k][...] = host[k]
        if motion is not None:
            motion_state[...] = host["motion"]
        return {k: v.cpu().numpy() for k, v in out.items()}
    return step


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_crafted_case_device_equals_numpy(case, numpy_runs, dev):
    got = MC.run_case(case, device_step(dev))
    case["expect"](*got[:2])
    MC.assert_same(got, numpy_runs[case["name"]], case["name"])


@pytest.mark.parametrize("name", [f"{n}-D{D}" for n in ("turning", "doorway") for D in MC.DIMS])
def test_without_motion_the_device_gives_the_stale_box_answer(name, dev):
    case = BY_NAME[name]
    got = MC.run_case(case, device_step(dev), motion=False)
    case["expect_without"](*got[:2])
    assert "track_pred" not in got[0][0]


@pytest.mark.parametrize("D", MC.DIMS)
def test_turning_head_scored_on_the_device(D, dev):
    """mot_eval (the device path) on the device tracker's rows: no identity switch with motion, one per frame without."""
    case = BY_NAME[f"turning-D{D}"]
    gf, gi, gb = case["gt"]
    z = np.zeros_like
    res = {}
    for motion in (True, False):
        hf, hi, hb = MC.mot_rows(case, MC.run_case(case, device_step(dev), motion=motion)[0])
        res[motion] = TE.mot_eval(z(gf), gf, gi, gb, z(hf), hf, hi, hb, [11], device=dev)
        assert res[motion].TP == 11 and res[motion].FN == 0
    assert res[True].IDSW == 0 and res[True].IDF1 == 1.0
    assert res[False].IDSW == 9


@pytest.mark.parametrize("case", MOVING, ids=[c["name"] for c in MOVING])
def test_moving_batch_device_equals_numpy_twice(case, numpy_runs, dev):
    """... and two runs of the kernel are bit-identical, outputs, state and motion."""
    first = MC.run_case(case, device_step(dev))
    MC.assert_same(first, numpy_runs[case["name"]], case["name"])
    MC.assert_same(MC.run_case(case, device_step(dev)), first, "second run")


def test_device_properties_split_interleave_idle_stream(numpy_runs, dev):
    case = MOVING[0]
    (whole,), state, motion, _ = numpy_runs[case["name"]]
    step = device_step(dev)
    B = len(case["steps"][0]["stream_of_frame"])
    for k in (0, 1, B // 3 + 1, B // 2, B - 1, B):
        two, rows = TC.split_case(case, k)
        outs, st, m = MC.run_case(two, step)
        for part, r in zip(outs, rows):
            for key in MC.OUT_KEYS:
                assert np.array_equal(part[key], whole[key][r]), (k, key)
        TC.assert_same_state(st, state, f"split at {k}")
        MC.assert_same_motion(m, motion, f"split at {k}")
    for s in range(case["S"]):
        alone, rows = TC.stream_alone(case, s)
        (out,), st, m = MC.run_case(alone, step)
        for key in MC.OUT_KEYS:
            assert np.array_equal(out[key], whole[key][rows]), (s, key)
        for key in T.STATE_KEYS:
            assert st[key][0].tobytes() == state[key][s].tobytes(), (s, key)
        assert m[0].tobytes() == motion[s].tobytes(), s
    # a fourth stream that owns no frame keeps whatever its motion rows held
    idle = MC.moving(32, spare_streams=1)
    marks = (np.arange(T.SLOTS * T.MOTION_FLOATS, dtype=np.float32).reshape(T.SLOTS, T.MOTION_FLOATS) - 300) * np.float32(0.37)
    m0 = T.new_motion_state(4)
    m0[3] = marks
    st0 = T.new_state(4, 32)
    st0["slot_i"][3, 5] = [9, 1, 2, 3, 1]
    st0["hdr"][3] = [2, 10]
    (out,), st, m = MC.run_case(idle, step, state=st0, motion_state=m0)
    assert m[3].tobytes() == marks.tobytes() and st["hdr"][3].tolist() == [2, 10] and st["slot_i"][3, 5].tolist() == [9, 1, 2, 3, 1]
    for key in MC.OUT_KEYS:
        assert np.array_equal(out[key], whole[key]), key
    assert m[:3].tobytes() == motion.tobytes()


def test_state_round_trip_reset_and_tracks(dev):
    """One tracker across two steps equals state_dict -> load_state_dict into another tracker between them, motion included;
    tracks() reports pred_box and velocity; reset(streams) zeroes those streams' motion only; a tracker without motion= keeps
    today's keys."""
    case = MOVING[0]
    two, _ = TC.split_case(case, 31)
    a, b = two["steps"]
    args = lambda st: (to_dev(st["frame"], dev), to_dev(st["boxes"], dev), to_dev(st["emb"], dev),          # noqa: E731
                       to_dev(st["stream_of_frame"], dev))
    kw = lambda st: dict(score=to_dev(st["score"], dev), xinv=to_dev(st["xinv"], dev))                      # noqa: E731
    make = lambda: T.StreamTracker(case["S"], 32, case["max_age"], device=dev, motion=case["motion"])       # noqa: E731
    one = make()
    first = one.step(*args(a), **kw(a))
    assert first["track_pred"].shape == (len(a["frame"]), 4) and first["track_pred"].dtype == torch.float32
    saved = one.state_dict()
    assert saved["params"]["std_pos"] == case["motion"].std_pos and not saved["motion"].is_cuda
    assert tuple(saved["motion"].shape) == (case["S"], T.SLOTS, T.MOTION_FLOATS)
    want = one.step(*args(b), **kw(b))
    other = make()
    other.load_state_dict(saved)
    got = other.step(*args(b), **kw(b))
    for key in MC.OUT_KEYS:
        assert torch.equal(got[key], want[key]), key
    h_one, h_other = one.host_state(), other.host_state()
    TC.assert_same_state(h_other, h_one, "round trip")
    MC.assert_same_motion(h_other["motion"], h_one["motion"], "round trip")
    with pytest.raises(KeyError):
        make().load_state_dict({k: saved[k] for k in T.STATE_KEYS})        # a state without motion into a tracker with it
    plain = T.StreamTracker(case["S"], 32, case["max_age"], device=dev)
    plain.load_state_dict(saved)                                           # the other way round: motion is ignored
    assert set(plain.host_state()) == set(T.STATE_KEYS) and set(plain.step(*args(b), **kw(b))) == set(T.OUT_KEYS)
    assert "pred_box" not in plain.tracks(0)
    t = one.tracks(1)
    live = np.nonzero(h_one["slot_i"][1, :, T.I_ID])[0]
    m = h_one["motion"][1, live].reshape(len(live), 4, T.M_COLS)
    assert len(live) > 0 and t["pred_box"].shape == (len(live), 4) and t["velocity"].tolist() == m[:, :, T.M_V].tolist()
    assert np.allclose(0.5 * (t["pred_box"][:, 0] + t["pred_box"][:, 2]), m[:, 0, T.M_X], atol=1e-3)
    one.reset([1])
    after = one.host_state()
    assert not after["motion"][1].any() and after["motion"][0].tobytes() == h_one["motion"][0].tobytes()
    one.reset()
    assert not one.host_state()["motion"].any()


def test_pipeline_passes_track_pred_through(dev):
    """FacePipeline(tracker=StreamTracker(motion=)): the step result gains track_pred, zeros on rows without an id and equal to
    the host emulator's on the step's own rows when every id agrees (random embeddings keep no cosine gap: at least three ids
    in four must agree, as test_tracklets_gpu.py accepts); the two-stream path returns the same tensors."""
    from face_detection_and_recognition_amd import workload as W
    from face_detection_and_recognition_amd.pipeline import FacePipeline
    from face_detection_and_recognition_amd.similarity import row_inv_norm
    frames = W.make_frames(8, dev, seed=7)
    det = W.build_detector(dev, W.make_frames(8, dev, seed=8), cand_per_frame=48)
    emb = W.build_embedder(dev)
    cv = T.ConstantVelocity(T.ConstantVelocity.DEEPSORT_STD_POS, T.ConstantVelocity.DEEPSORT_STD_VEL)
    make = lambda: T.StreamTracker(1, emb.embedding_size, 3, device=dev, motion=cv)                         # noqa: E731
    res = FacePipeline(det, emb, None, tracker=make()).step(frames)
    n = res["n_faces"]
    assert n > 0 and res["track_pred"].shape == (n, 4) and res["track_pred"].dtype == torch.float32
    info, e = res["info"][:n].cpu().numpy(), res["emb"][:n].cpu().numpy()
    xinv = row_inv_norm(res["emb"][:n].contiguous()).cpu().numpy()
    want = T.track_step_emulate(T.new_state(1, e.shape[1]), info[:, 0].astype(np.int32), info[:, 1:5], e, xinv,
                                np.zeros((8,), np.int32), 3, score=info[:, 5], motion=cv, motion_state=T.new_motion_state(1))
    ids, pred = res["track_id"].cpu().numpy(), res["track_pred"].cpu().numpy()
    same = ids == want["track_id"]
    assert same.sum() * 4 >= 3 * n
    if same.all():
        assert np.array_equal(pred, want["track_pred"])
    assert (pred[ids == 0] == 0).all() and ((res["track_flags"].cpu().numpy() & T.NEW == 0) & (ids > 0)).any()
    over = FacePipeline(det, emb, None, two_streams=True, tracker=make())
    assert over.step_overlapped(frames) is None
    got = over.flush()
    got["done"].synchronize()
    for key in MC.OUT_KEYS:
        assert torch.equal(got[key], res[key]), key


def test_drivers_with_motion(dev, tmp_path, capsys):
    """track_faces_in_frames --motion writes tracks and a hypothesis file; eval_face_tracker --motion run on the same frames with
    that file as ground truth scores it perfectly (the same tracker twice), a --sweep std_pos= prints one row per value, and a
    swept std_* without --motion is refused."""
    from face_detection_and_recognition_amd import workload as W
    from face_detection_and_recognition_amd.eval import eval_face_tracker as ET
    from face_detection_and_recognition_amd.face_extraction import track_faces_in_frames as TF
    from face_detection_and_recognition_amd.modules.utils.jpeg import encode_jpeg_batch
    seq = tmp_path / "data" / "video"
    (seq / "frames").mkdir(parents=True)
    for i, data in enumerate(encode_jpeg_batch(list(W.make_frames(8, dev, seed=7)))):
        (seq / "frames" / f"frame_{i:04d}.jpg").write_bytes(data)
    motion = ["--motion", "0.05", "0.00625"]
    tracks = TF.main(["--frames", str(seq / "frames"), "--td", str(tmp_path / "out"), "--max_age", "3", "-b", "5", "-d", str(dev),
                      "--mot_out", str(seq / "gt.txt")] + motion)
    rows = TE.read_mot_txt(seq / "gt.txt")
    assert len(tracks) > 0 and len(rows["frame"]) == sum(t["hits"] for t in tracks)
    res = ET.main([str(tmp_path / "data"), "--model", "synthetic", "--max_age", "3", "-b", "5", "-d", str(dev)] + motion)
    assert res.MOTA == res.IDF1 == 1.0 and res.TP == len(rows["frame"])
    capsys.readouterr()
    swept = ET.main([str(tmp_path / "data"), "--model", "synthetic", "--max_age", "3", "--sweep", "std_pos=0.05,0.5", "-b", "5",
                     "-d", str(dev)] + motion)
    assert [v for v, _ in swept] == [0.05, 0.5] and swept[0][1].IDF1 == 1.0
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[-3].split()[:2] == ["std_pos", "sequence"] and [ln.split()[0] for ln in lines[-2:]] == ["0.05", "0.5"]
    with pytest.raises(SystemExit):
        ET.main([str(tmp_path / "data"), "--model", "synthetic", "--max_age", "3", "--sweep", "std_vel=0.01", "-b", "5", "-d", str(dev)])
