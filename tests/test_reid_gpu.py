"""Tracklets with re-identification on the device: fp_tracklets_step_reid against the numpy restatement on every case of
reid_cases.py, with and without motion (the per-row outputs, track_pred, the five state arrays, `motion` and the five lost_*
arrays, equal, under each case's gap condition), two runs bit-identical, the revolving door scored by mot_eval on the device, the
properties on the device (split, interleave, scattered, a stream without frames), a tracker without reid= unchanged, lost() /
reset / state_dict round trip, TrackBook across the gap, FacePipeline(tracker=) with reid, and --reid on the two drivers."""
import numpy as np
import pytest
import torch

import motion_cases as MC
import reid_cases as RC
import track_cases as TC
from face_detection_and_recognition_amd import tracking as T
from face_detection_and_recognition_amd import tracking_eval as TE

pytestmark = pytest.mark.gpu

CASES = RC.crafted_cases()
BUSY = [RC.busy(D) for D in RC.DIMS]
BY_NAME = {c["name"]: c for c in CASES + BUSY}
TRACK = RC.track_cases_in_every_configuration()


@pytest.fixture(scope="module")
def numpy_runs():
    return {(c["name"], m): RC.assert_gap(c, motion=m) for c in CASES + BUSY for m in (False, True)}


def to_dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def device_step(dev):
    """A step_fn for RC.run_case: a fresh StreamTracker per call, the host state (`motion`, the pool) loaded into it, one launch,
    the state read back (so every step also crosses load_state_dict / host_state)."""
    def step(state, frame, boxes, emb, xinv, stream_of_frame, max_age, score=None, motion=None, motion_state=None, reid=None,
             lost_state=None, **params):
        tr = T.StreamTracker(state["hdr"].shape[0], state["emb"].shape[2], max_age, device=dev, motion=motion, reid=reid, **params)
        full = dict(state)
        if motion is not None:
            full["motion"] = motion_state
        if reid is not None:
            full.update(lost_state)
        tr.load_state_dict(full)
        out = tr.step(to_dev(frame, dev), to_dev(boxes, dev), to_dev(emb, dev), to_dev(stream_of_frame, dev),
                      score=to_dev(score, dev), xinv=to_dev(xinv, dev))
        torch.cuda.synchronize()
        host = tr.host_state()
        for k in T.STATE_KEYS:
            state[k][...] = host[k]
        if motion is not None:
            motion_state[...] = host["motion"]
        if reid is not None:
            for k in T.LOST_KEYS:
                lost_state[k][...] = host[k]
        return {k: v.cpu().numpy() for k, v in out.items()}
    return step


@pytest.mark.parametrize("motion", [False, True], ids=["plain", "motion"])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_crafted_case_device_equals_numpy(case, motion, numpy_runs, dev):
    got = RC.run_case(case, device_step(dev), motion=motion)
    case["expect"](got[0], got[1], got[3])
    if motion and "expect_motion" in case:
        case["expect_motion"](*got[:3])
    RC.assert_same(got, numpy_runs[case["name"], motion], case["name"])


@pytest.mark.parametrize("motion,reid", RC.CONFIGS, ids=RC.CONFIG_IDS)
@pytest.mark.parametrize("case", TRACK, ids=[c["name"] for c in TRACK])
def test_track_case_device_equals_emulator_in_every_configuration(case, motion, reid, dev):
    """The crafted cases of track_cases.py through each of the four kernels: all of them sort, walk and score pairs through the
    same functions, and these cases are the ones with 2048 and 1024 keys, 64 full slots, 65 rows and ties.  Device and emulator
    share every bit (outputs, state, motion, pool), so no gap condition is needed here; test_reid_cpu.py holds the emulator to
    numpy on the same matrix."""
    got = RC.run_case(case, device_step(dev), reid=reid, motion=motion)
    RC.assert_same(got, RC.run_case(case, T.track_step_emulate, reid=reid, motion=motion), case["name"])


@pytest.mark.parametrize("D", RC.DIMS)
def test_revolving_door_scored_on_the_device(D, dev):
    """mot_eval (the device path) on the device tracker's rows: one identity switch without the pool (the returning face is id 4),
    none with it; and a tracker without reid= still returns exactly OUT_KEYS and the five STATE_KEYS."""
    case = BY_NAME[f"door-D{D}"]
    gf, gi, gb = case["gt"]
    z = np.zeros_like
    res = {}
    for reid in (True, False):
        outs, state = RC.run_case(case, device_step(dev), reid=reid)[:2]
        if not reid:
            case["expect_without"](outs, state)
            assert set(outs[0]) == set(T.OUT_KEYS)
        hf, hi, hb = MC.mot_rows(case, outs)
        res[reid] = TE.mot_eval(z(gf), gf, gi, gb, z(hf), hf, hi, hb, [22], device=dev)
        assert res[reid].TP == 37 and res[reid].FN == 0
    assert res[False].IDSW == 1 and round(res[False].IDF1, 4) == 0.8649
    assert res[True].IDSW == 0 and res[True].IDF1 == 1.0
    plain = T.StreamTracker(1, D, 3, device=dev)
    assert plain.state_keys == T.STATE_KEYS and set(plain.state) == set(T.STATE_KEYS) == set(plain.host_state())


@pytest.mark.parametrize("motion", [False, True], ids=["plain", "motion"])
@pytest.mark.parametrize("case", BUSY, ids=[c["name"] for c in BUSY])
def test_busy_batch_device_equals_numpy_twice(case, motion, numpy_runs, dev):
    """... and two runs of the kernel are bit-identical: outputs, state, motion and pool."""
    first = RC.run_case(case, device_step(dev), motion=motion)
    RC.assert_same(first, numpy_runs[case["name"], motion], case["name"])
    RC.assert_same(RC.run_case(case, device_step(dev), motion=motion), first, "second run")


def test_device_properties_split_interleave_scattered_idle_stream(numpy_runs, dev):
    case = BUSY[0]
    (whole,), state, _, lost, _ = numpy_runs[case["name"], False]
    step = device_step(dev)
    B = len(case["steps"][0]["stream_of_frame"])
    for k in (0, 1, B // 4, B // 3 + 1, B // 2, 3 * B // 4 + 1, B - 1, B):
        two, rows = TC.split_case(case, k)
        outs, st, _, lo = RC.run_case(two, step)
        for part, r in zip(outs, rows):
            for key in T.OUT_KEYS:
                assert np.array_equal(part[key], whole[key][r]), (k, key)
        TC.assert_same_state(st, state, f"split at {k}")
        RC.assert_same_lost(lo, lost, f"split at {k}")
    for s in range(4):
        alone, rows = TC.stream_alone(case, s)
        (out,), st, _, lo = RC.run_case(alone, step)
        for key in T.OUT_KEYS:
            assert np.array_equal(out[key], whole[key][rows]), (s, key)
        for key in T.STATE_KEYS:
            assert st[key][0].tobytes() == state[key][s].tobytes(), (s, key)
        for key in T.LOST_KEYS:
            assert lo[key][0].tobytes() == lost[key][s].tobytes(), (s, key)
    mixed, perm = TC.scattered(case)
    (out,), st, _, lo = RC.run_case(mixed, step)
    for key in T.OUT_KEYS:
        assert np.array_equal(out[key], whole[key][perm]), key
    TC.assert_same_state(st, state, "scattered")
    RC.assert_same_lost(lo, lost, "scattered")
    # the fifth stream owns no frame: its pool rows and ring head stay, bit for bit
    l0 = T.new_lost_state(case["S"], case["D"])
    l0["lost_hdr"][4] = [77, -3]
    l0["lost_i"][4, 9] = [5, 1, 2, 3, 1]
    l0["lost_f"][4] = (np.arange(T.LOST * 10, dtype=np.float32).reshape(T.LOST, 10) - 100) * np.float32(0.37)
    marks = {k: l0[k][4].copy() for k in T.LOST_KEYS}
    (out,), st, _, lo = RC.run_case(case, step, lost_state=l0)
    for k in T.LOST_KEYS:
        assert lo[k][4].tobytes() == marks[k].tobytes(), k
        assert lo[k][:4].tobytes() == lost[k][:4].tobytes(), k
    for key in T.OUT_KEYS:
        assert np.array_equal(out[key], whole[key]), key


def test_state_round_trip_lost_reset_and_trackbook(dev):
    """One tracker across two steps equals state_dict -> load_state_dict into another tracker between them, the pool included;
    lost() reports the parked tracks; reset(streams) empties those streams' pools only; a state without the pool does not load
    into a tracker with one; TrackBook keeps one record across the gap."""
    case = BY_NAME["door-D32"]
    two, _ = TC.split_case(case, 12)                 # A is parked (frame 8), not yet back (frame 17)
    a, b = two["steps"]
    args = lambda st: (to_dev(st["frame"], dev), to_dev(st["boxes"], dev), to_dev(st["emb"], dev),          # noqa: E731
                       to_dev(st["stream_of_frame"], dev))
    kw = lambda st: dict(score=to_dev(st["score"], dev), xinv=to_dev(st["xinv"], dev))                      # noqa: E731
    make = lambda: T.StreamTracker(2, 32, case["max_age"], device=dev, reid=case["reid"])                   # noqa: E731
    one = make()
    first = one.step(*args(a), **kw(a))
    assert set(first) == set(T.OUT_KEYS)
    parked = one.lost(0)
    assert parked["id"].tolist() == [2] and parked["hits"].tolist() == [5] and parked["last_clock"].tolist() == [5]
    assert parked["first_clock"].tolist() == [1] and parked["best_box"].tolist() == [TC.cell(3)]
    assert parked["best_emb"].tobytes() == a["emb"][1].tobytes() and len(one.lost(1)["id"]) == 0
    saved = one.state_dict()
    assert saved["params"]["tau_reid"] == 0.75 and saved["params"]["lost_age"] == 100 and not saved["lost_emb"].is_cuda
    want = one.step(*args(b), **kw(b))
    other = make()
    other.load_state_dict(saved)
    got = other.step(*args(b), **kw(b))
    for key in T.OUT_KEYS:
        assert torch.equal(got[key], want[key]), key
    assert (want["track_flags"].cpu().numpy() & T.REVIVED != 0).sum() == 1
    h_one, h_other = one.host_state(), other.host_state()
    TC.assert_same_state(h_other, h_one, "round trip")
    RC.assert_same_lost(h_other, h_one, "round trip")
    with pytest.raises(KeyError):
        make().load_state_dict({k: saved[k] for k in T.STATE_KEYS})          # a state without the pool into a tracker with it
    plain = T.StreamTracker(2, 32, case["max_age"], device=dev)
    plain.load_state_dict(saved)                                             # the other way round: the pool is ignored
    out = plain.step(*args(b), **kw(b))
    assert set(out) == set(T.OUT_KEYS) and (out["track_flags"].cpu().numpy() & T.REVIVED == 0).all()
    assert 4 in out["track_id"].cpu().numpy()
    third = make()
    third.load_state_dict(saved)
    third.reset([1])
    assert third.lost(0)["id"].tolist() == [2]
    third.reset([0])
    assert len(third.lost(0)["id"]) == 0 and not any(third.host_state()[k].any() for k in T.LOST_KEYS)
    book = T.TrackBook()
    for st, o in ((a, first), (b, want)):
        book.update(o, st["frame"], st["boxes"], st["stream_of_frame"], emb=st["emb"], frame_base=0 if st is a else 12)
    assert len(book) == 3 and book[(0, 2)]["hits"] == 10 and book[(0, 2)]["first_clock"] == 1 and book[(0, 2)]["last_clock"] == 22


def test_pipeline_carries_revived_through_step_and_step_overlapped(dev):
    """FacePipeline(tracker=StreamTracker(reid=)): eight frames, then the tracker's clock moved on past max_age (empty frames
    through the tracker itself), then the same eight frames in reverse order.  The same crop gives the same embedding, so the
    faces of the last frame meet their own parked tracks' last embeddings at cosine 1: those rows come back REVIVED, never NEW,
    under the ids they had, while every NEW row gets an id above the first pass's.  step_overlapped returns the same tensors."""
    from face_detection_and_recognition_amd import workload as W
    from face_detection_and_recognition_amd.pipeline import FacePipeline
    frames = W.make_frames(8, dev, seed=7)
    det = W.build_detector(dev, W.make_frames(8, dev, seed=8), cand_per_frame=48)
    emb = W.build_embedder(dev)
    make = lambda: T.StreamTracker(1, emb.embedding_size, 3, device=dev, reid=T.LostPool(0.9, 1000))        # noqa: E731

    def away(tr):                                    # five frames without a face: every track expires and is parked
        e = torch.zeros((0, emb.embedding_size), device=dev)
        tr.step(torch.zeros((0,), dtype=torch.int32, device=dev), torch.zeros((0, 4), device=dev), e,
                torch.zeros((5,), dtype=torch.int32, device=dev))
    tr = make()
    pipe = FacePipeline(det, emb, None, tracker=tr)
    first = pipe.step(frames)
    n, last_id = first["n_faces"], int(first["track_id"].max().item())
    assert n > 0 and last_id > 0 and (first["track_flags"].cpu().numpy() & T.REVIVED == 0).all()
    in_last = first["info"][:n, 0].cpu().numpy() == 7
    ids_last = first["track_id"][:n].cpu().numpy()[in_last]
    assert in_last.any() and (ids_last > 0).all()
    away(tr)
    assert set(ids_last.tolist()) <= set(tr.lost(0)["id"].tolist())
    back = frames.flip(0).contiguous()
    res = pipe.step(back)
    assert res["n_faces"] == n
    ids, flags = res["track_id"][:n].cpu().numpy(), res["track_flags"][:n].cpu().numpy()
    rev, new = flags & T.REVIVED != 0, flags & T.NEW != 0
    in_first = res["info"][:n, 0].cpu().numpy() == 0
    assert in_first.sum() == in_last.sum() and rev[in_first].all() and sorted(ids[in_first]) == sorted(ids_last)
    assert not (rev & new).any() and (ids[rev] <= last_id).all() and (ids[new] > last_id).all()
    over_tr = make()
    over = FacePipeline(det, emb, None, two_streams=True, tracker=over_tr)
    assert over.step_overlapped(frames) is None
    over.flush()["done"].synchronize()
    away(over_tr)
    assert over.step_overlapped(back) is None
    got = over.flush()
    got["done"].synchronize()
    for key in T.OUT_KEYS:
        assert torch.equal(got[key][:n], res[key][:n]), key


def test_drivers_with_reid(dev, tmp_path, capsys):
    """track_faces_in_frames --reid writes tracks and a hypothesis file; eval_face_tracker --reid run on the same frames with
    that file as ground truth scores it perfectly (the same tracker twice), a --sweep tau_reid= prints one row per value, and a
    swept lost_age without --reid is refused."""
    from face_detection_and_recognition_amd import workload as W
    from face_detection_and_recognition_amd.eval import eval_face_tracker as ET
    from face_detection_and_recognition_amd.face_extraction import track_faces_in_frames as TF
    from face_detection_and_recognition_amd.modules.utils.jpeg import encode_jpeg_batch
    seq = tmp_path / "data" / "video"
    (seq / "frames").mkdir(parents=True)
    for i, data in enumerate(encode_jpeg_batch(list(W.make_frames(8, dev, seed=7)))):
        (seq / "frames" / f"frame_{i:04d}.jpg").write_bytes(data)
    reid = ["--reid", "0.8", "30"]
    tracks = TF.main(["--frames", str(seq / "frames"), "--td", str(tmp_path / "out"), "--max_age", "3", "-b", "5", "-d", str(dev),
                      "--mot_out", str(seq / "gt.txt")] + reid)
    rows = TE.read_mot_txt(seq / "gt.txt")
    assert len(tracks) > 0 and len(rows["frame"]) == sum(t["hits"] for t in tracks)
    res = ET.main([str(tmp_path / "data"), "--model", "synthetic", "--max_age", "3", "-b", "5", "-d", str(dev)] + reid)
    assert res.MOTA == res.IDF1 == 1.0 and res.TP == len(rows["frame"])
    capsys.readouterr()
    swept = ET.main([str(tmp_path / "data"), "--model", "synthetic", "--max_age", "3", "--sweep", "tau_reid=0.8,0.3", "-b", "5",
                     "-d", str(dev)] + reid)
    assert [v for v, _ in swept] == [0.8, 0.3] and swept[0][1].IDF1 == 1.0
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[-3].split()[:2] == ["tau_reid", "sequence"] and [ln.split()[0] for ln in lines[-2:]] == ["0.8", "0.3"]
    with pytest.raises(SystemExit):
        ET.main([str(tmp_path / "data"), "--model", "synthetic", "--max_age", "3", "--sweep", "lost_age=30", "-b", "5", "-d", str(dev)])
