"""Templates on the device: fp_track_pool_step against track_pool_numpy and track_pool_emulate on every case of template_cases.py
(every bit of the three per-row outputs and the three table arrays), two runs identical, the properties on the device,
StreamTracker(templates=) on the tracker's own cases with reid and motion, the constructed benefit through StreamTracker and
FaceGallery, FacePipeline(identify_tracks=True) on both stream paths, and the driver's flags."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import reid_cases as RC
import template_cases as PC
import track_cases as TC
from face_detection_and_recognition_amd import _lib as L
from face_detection_and_recognition_amd import tracking as T

pytestmark = pytest.mark.gpu

SIZES = PC.width_length_cases()
CRAFTED = PC.crafted_cases()


def to_dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def device_pool(dev):
    """A pool_fn for PC.run_case: the host table copied to the device, fp_track_pool_step, everything read back."""
    def step(table, frame, emb, xinv, stream_of_frame, track_id, track_clock, track_flags, keep, weight=None):
        lib = L.load()
        S, D = table["tpl_sum"].shape[0], table["tpl_sum"].shape[2]
        i32 = lambda a: to_dev(np.asarray(a, np.int32).reshape(-1), dev)           # noqa: E731
        f32 = lambda a: to_dev(np.asarray(a, np.float32), dev)                      # noqa: E731
        frame, sof, ids, clocks, flags = i32(frame), i32(stream_of_frame), i32(track_id), i32(track_clock), i32(track_flags)
        n = frame.shape[0]
        emb, xinv, weight = f32(emb).reshape(n, D), f32(xinv).reshape(n), None if weight is None else f32(weight).reshape(n)
        st = {k: to_dev(table[k], dev) for k in T.TEMPLATE_KEYS}
        out = dict(track_emb=torch.full((n, D), 7.0, device=dev), track_emb_rows=torch.full((n,), -7, dtype=torch.int32, device=dev),
                   track_emb_flags=torch.full((n,), -7, dtype=torch.int32, device=dev))
        ws = torch.empty((lib.fp_track_pool_workspace_bytes(n),), dtype=torch.uint8, device=dev)
        tpl = L.FpTrackTemplates(*[L.ptr(st[k]) for k in T.TEMPLATE_KEYS])
        L.check(lib.fp_track_pool_step(C.byref(tpl), S, D, L.ptr(frame), L.ptr(emb), L.ptr(xinv), L.ptr(weight), n, L.ptr(sof),
                                       sof.shape[0], L.ptr(ids), L.ptr(clocks), L.ptr(flags), int(keep),
                                       *[L.ptr(out[k]) for k in T.TEMPLATE_OUT_KEYS], L.ptr(ws), ws.numel(),
                                       L.current_stream(dev)), "fp_track_pool_step")
        torch.cuda.synchronize()
        for k in T.TEMPLATE_KEYS:
            table[k][...] = st[k].cpu().numpy()
        return {k: v.cpu().numpy() for k, v in out.items()}
    return step


@pytest.fixture(scope="module")
def numpy_runs():
    return {c["name"]: PC.run_case(c, T.track_pool_numpy) for c in SIZES + CRAFTED}


@pytest.mark.parametrize("case", SIZES + CRAFTED, ids=[c["name"] for c in SIZES + CRAFTED])
def test_case_device_equals_numpy_and_emulator(case, numpy_runs, dev):
    got = PC.run_case(case, device_pool(dev))
    if case["expect"]:
        case["expect"](*got)
    PC.assert_same(got, numpy_runs[case["name"]], case["name"] + " numpy")
    PC.assert_same(got, PC.run_case(case, T.track_pool_emulate), case["name"] + " emulator")


@pytest.mark.parametrize("D", PC.CRAFTED_DIMS)
def test_device_properties_twice_split_scattered(D, dev):
    """Two device runs are identical; 18 frames in one call equal 9 + 9 and 3 + 15 (per stream 3 + 3 and 1 + 5) with the table
    carried; scattered rows equal ordered rows."""
    step = device_pool(dev)
    case = PC.busy(D)
    want = PC.run_case(case, T.track_pool_numpy)
    first = PC.run_case(case, step)
    PC.assert_same(first, want, "busy")
    PC.assert_same(PC.run_case(case, step), first, "second run")
    (whole,), table = want
    for k in (9, 3, 0, 18):
        two, rows = PC.split_case(case, k)
        outs, t = PC.run_case(two, step)
        for part, r in zip(outs, rows):
            for key in T.TEMPLATE_OUT_KEYS:
                assert np.array_equal(PC.int_view(part[key]), PC.int_view(whole[key][r])), (k, key)
        PC.assert_same_table(t, table, f"split at {k}")
    case = PC.scattered(D)
    (mixed,), t_mixed = PC.run_case(case, step)
    (ordered,), t_ordered = PC.run_case(case["ordered"], step)
    for key in T.TEMPLATE_OUT_KEYS:
        assert np.array_equal(PC.int_view(mixed[key]), PC.int_view(ordered[key][case["perm"]])), key
    PC.assert_same_table(t_mixed, t_ordered, "scattered")


def tracker_with_templates(case, dev, reid, motion, weighted):
    """The case through ONE StreamTracker(templates=) on the device -> (step outs as numpy, the tracker)."""
    tr = T.StreamTracker(case["S"], case["D"], case["max_age"], device=dev, motion=case["motion"] if motion else None,
                         reid=case["reid"] if reid else None, templates=T.Templates(weighted=weighted), **TC.PARAMS)
    if reid and case.get("lost_init"):
        lost = T.new_lost_state(case["S"], case["D"])
        case["lost_init"](lost)
        tr.load_state_dict(dict(tr.state_dict(), **{k: torch.from_numpy(v) for k, v in lost.items()}))
    outs = []
    for st in case["steps"]:
        o = tr.step(to_dev(st["frame"], dev), to_dev(st["boxes"], dev), to_dev(st["emb"], dev), to_dev(st["stream_of_frame"], dev),
                    score=to_dev(st["score"], dev), xinv=to_dev(st["xinv"], dev))
        outs.append({k: v.cpu().numpy() for k, v in o.items()})
    return outs, tr


TRACKED = RC.track_cases_in_every_configuration()[::2] + RC.crafted_cases()[1::2] + [RC.busy(32)]


@pytest.mark.parametrize("case", TRACKED, ids=[c["name"] for c in TRACKED])
def test_through_the_tracker_device_equals_emulator_and_numpy(case, dev):
    """StreamTracker(templates=, reid=, motion=) on the tracker's own cases: the tracker's results equal the emulator's (as
    test_reid_gpu.py pins), and the three template outputs and the table equal both restatements fed with those results."""
    weighted = all(st["score"] is not None for st in case["steps"])
    outs, tr = tracker_with_templates(case, dev, True, True, weighted)
    want_track = RC.run_case(case, T.track_step_emulate, reid=True, motion=True)[0]
    assert tr.keep == case["reid"].lost_age and set(tr.state_keys) >= set(T.TEMPLATE_KEYS)
    host = tr.host_state()
    for fn in (T.track_pool_numpy, T.track_pool_emulate):
        table = T.new_template_state(case["S"], case["D"])
        for st, o, w in zip(case["steps"], outs, want_track):
            for key in T.OUT_KEYS:
                assert np.array_equal(o[key], w[key]), key
            want = fn(table, st["frame"], st["emb"], st["xinv"], st["stream_of_frame"], o["track_id"], o["track_clock"],
                      o["track_flags"], tr.keep, weight=st["score"] if weighted else None)
            PC.assert_same(([o], table), ([want], table), case["name"])
        PC.assert_same_table(host, table, case["name"])


def test_revived_row_state_round_trip_and_a_plain_tracker(dev):
    """The revolving door through StreamTracker(reid=, templates=): the REVIVED row continues its template (6 rows, no flag);
    templates(stream) reads the table; state_dict -> load_state_dict carries it, reset empties it; TrackBook keeps the latest
    template; a tracker without templates= returns exactly the parent's keys and state."""
    case = next(c for c in RC.crafted_cases() if c["name"] == "door-D32")
    (o,), tr = tracker_with_templates(case, dev, True, False, False)
    a = np.nonzero(o["track_id"] == 2)[0]
    assert o["track_flags"][a[5]] == T.REVIVED and o["track_emb_rows"][a].tolist() == list(range(1, 11))
    assert not o["track_emb_flags"].any()
    t = tr.templates(0)
    assert t["id"].tolist() == [1, 2, 3] and t["rows"].tolist() == [22, 10, 5] and t["wsum"].tolist() == [22.0, 10.0, 5.0]
    assert t["last_clock"].tolist() == [22, 22, 22] and t["sum"][1].tobytes() == o["track_emb"][a[-1]].tobytes()
    st = case["steps"][0]
    book = T.TrackBook()
    book.update(o, st["frame"], st["boxes"], st["stream_of_frame"], track_emb=o["track_emb"], track_emb_rows=o["track_emb_rows"])
    assert book[(0, 2)]["template_rows"] == 10 and book[(0, 2)]["template"].tobytes() == t["sum"][1].tobytes()
    saved = tr.state_dict()
    other = T.StreamTracker(1, 32, case["max_age"], device=dev, reid=case["reid"], templates=T.Templates())
    other.load_state_dict(saved)
    PC.assert_same_table(other.host_state(), tr.host_state(), "round trip")
    with pytest.raises(KeyError):
        other.load_state_dict({k: saved[k] for k in T.STATE_KEYS + T.LOST_KEYS})
    other.reset([0])
    assert len(other.templates(0)["id"]) == 0 and not any(other.host_state()[k].any() for k in T.TEMPLATE_KEYS)
    plain = T.StreamTracker(1, 32, case["max_age"], device=dev, reid=case["reid"])
    plain.load_state_dict(saved)
    assert plain.state_keys == T.STATE_KEYS + T.LOST_KEYS and set(plain.state) == set(plain.state_keys)
    out = plain.step(to_dev(st["frame"], dev), to_dev(st["boxes"], dev), to_dev(st["emb"], dev), to_dev(st["stream_of_frame"], dev))
    assert set(out) == set(T.OUT_KEYS)
    with pytest.raises(ValueError):
        plain.templates(0)
    with pytest.raises(TypeError):
        T.StreamTracker(1, 32, 3, device=dev, templates=True)


def test_constructed_benefit_on_the_device(dev):
    """template_cases.BENEFIT through StreamTracker(templates=) and FaceGallery: the boxes alone tie a track together (tau_near
    -1, tau_far 2: any cosine passes with IoU, none without), the gallery names every row from its own embedding and from its
    track's template.  At least 10 % of the rows are named wrongly one by one; at every track's last row the template's name is
    right."""
    from face_detection_and_recognition_amd.gallery import FaceGallery
    proto, st, truth = PC.benefit_rows()
    K, D = proto.shape
    tr = T.StreamTracker(1, D, 3, tau_near=-1.0, tau_far=2.0, device=dev, templates=T.Templates())
    o = tr.step(to_dev(st["frame"], dev), to_dev(st["boxes"], dev), to_dev(st["emb"], dev), to_dev(st["stream_of_frame"], dev),
                xinv=to_dev(st["xinv"], dev))
    assert o["track_id"].cpu().numpy().tolist() == (truth + 1).tolist()
    assert o["track_emb_rows"].cpu().numpy().tolist() == (st["frame"] + 1).tolist()
    gal = FaceGallery(torch.from_numpy(proto.astype(np.float32)), torch.arange(K, dtype=torch.int32), device=dev)
    per_row = gal.identify(to_dev(st["emb"], dev), k=1, tau=-1.0)["label"].cpu().numpy()
    pooled = gal.identify(o["track_emb"], k=1, tau=-1.0)["label"].cpu().numpy()
    row_rate = float((per_row != truth).mean())
    last = st["frame"] == PC.BENEFIT["FRAMES"] - 1
    print(f"per-row error rate {row_rate} (numpy float64: {PC.ROW_ERROR_RATE}), pooled errors at the last rows "
          f"{int((pooled[last] != truth[last]).sum())}")
    assert row_rate >= 0.10
    assert (pooled[last] == truth[last]).all()


@pytest.fixture(scope="module")
def synthetic(dev):
    from face_detection_and_recognition_amd import workload as W
    from face_detection_and_recognition_amd.gallery import FaceGallery
    frames = W.make_frames(8, dev, seed=7)
    det = W.build_detector(dev, W.make_frames(8, dev, seed=8), cand_per_frame=48)
    emb = W.build_embedder(dev)
    g = torch.Generator().manual_seed(3)
    gal = FaceGallery(torch.randn((24, emb.embedding_size), generator=g), torch.arange(24, dtype=torch.int32) // 2,
                      names={k: f"p{k}" for k in range(12)}, device=dev)
    return frames, det, emb, gal


def test_pipeline_keys_identity_and_two_streams(synthetic, dev):
    from face_detection_and_recognition_amd.annotate import step_labels
    from face_detection_and_recognition_amd.pipeline import FacePipeline
    frames, det, emb, gal = synthetic
    D = emb.embedding_size
    make = lambda **kw: T.StreamTracker(1, D, 3, device=dev, **kw)       # noqa: E731
    for kw in (dict(gallery=gal), dict(tracker=make(templates=T.Templates())), dict(gallery=gal, tracker=make()), dict()):
        with pytest.raises(ValueError):
            FacePipeline(det, emb, None, identify_tracks=True, **kw)
    base = FacePipeline(det, emb, None, gallery=gal, identify_tau=-1.0, tracker=make()).step(frames)
    with_t = FacePipeline(det, emb, None, gallery=gal, identify_tau=-1.0, tracker=make(templates=T.Templates())).step(frames)
    pipe = FacePipeline(det, emb, None, gallery=gal, identify_tau=-1.0, top_k=3, tracker=make(templates=T.Templates()),
                        identify_tracks=True)
    res = pipe.step(frames)
    n = res["n_faces"]
    assert n > 0 and set(with_t) - set(base) == set(T.TEMPLATE_OUT_KEYS)
    assert set(res) - set(with_t) == set(FacePipeline.TRACK_IDENTITY_KEYS)
    assert set(FacePipeline.TRACK_IDENTITY_KEYS) | set(T.TEMPLATE_OUT_KEYS) <= set(FacePipeline.TRACK_RESULT_KEYS)
    for key in T.OUT_KEYS + ("identity", "identity_score"):
        assert torch.equal(res[key], base[key]) and torch.equal(with_t[key], base[key]), key
    assert tuple(res["track_emb"].shape) == (n, D) and tuple(res["track_top_idx"].shape) == (n, 3)
    ids, rows = res["track_id"].cpu().numpy(), res["track_emb_rows"].cpu().numpy()
    assert (rows[ids > 0] >= 1).all() and (rows[ids <= 0] == 0).all() and rows.max() > 1
    lone = torch.from_numpy(rows <= 1).to(dev)
    unit = res["emb"] * torch.rsqrt((res["emb"] ** 2).sum(1, keepdim=True))
    assert torch.equal(res["track_emb"][torch.from_numpy(ids <= 0).to(dev)], res["emb"][torch.from_numpy(ids <= 0).to(dev)])
    assert torch.allclose(res["track_emb"][lone & torch.from_numpy(ids > 0).to(dev)], unit[lone & torch.from_numpy(ids > 0).to(dev)],
                          rtol=1e-5, atol=1e-6)
    want = gal.identify(res["track_emb"], k=3, tau=-1.0, vote="top1")
    assert torch.equal(res["track_identity"], want["label"]) and torch.equal(res["track_identity_score"], want["score"])
    assert torch.equal(res["track_top_scores"], want["top_scores"]) and torch.equal(res["track_top_idx"], want["top_idx"])
    # the caption carries the track's name
    labels = step_labels(res, gal.names)
    who = res["track_identity"].cpu().numpy()
    for i in range(n):
        assert labels[i].startswith(f" p{who[i]}"), (i, labels[i])
    # step_overlapped on two streams returns the same tensors
    over = FacePipeline(det, emb, None, gallery=gal, identify_tau=-1.0, top_k=3, two_streams=True,
                        tracker=make(templates=T.Templates()), identify_tracks=True)
    assert over.step_overlapped(frames) is None
    got = over.flush()
    got["done"].synchronize()
    for key in T.OUT_KEYS + T.TEMPLATE_OUT_KEYS + FacePipeline.TRACK_IDENTITY_KEYS:
        assert torch.equal(got[key][:n], res[key][:n]), key
    # a second step goes on from the first: the same faces again, every template twice as long
    again = pipe.step(frames)
    assert again["track_emb_rows"].max().item() > res["track_emb_rows"].max().item()


def test_driver_flags_write_the_new_fields(synthetic, dev, tmp_path):
    from face_detection_and_recognition_amd.face_extraction import track_faces_in_frames as TF
    from face_detection_and_recognition_amd.modules.utils.jpeg import encode_jpeg_batch
    frames, _, emb, gal = synthetic
    folder = tmp_path / "frames"
    folder.mkdir()
    for i, data in enumerate(encode_jpeg_batch(list(frames))):
        (folder / f"frame_{i:04d}.jpg").write_bytes(data)
    gpath = gal.save(str(tmp_path / "gallery.npz"))
    common = ["--frames", str(folder), "--max_age", "3", "-b", "5", "-d", str(dev)]
    plain = TF.main(common + ["--td", str(tmp_path / "plain")])
    assert plain and all("template_rows" not in t and "identity" not in t for t in plain)
    assert not (tmp_path / "plain" / "tracks.npz").exists()
    tracks = TF.main(common + ["--td", str(tmp_path / "out"), "--templates", "--weighted", "--gallery", gpath, "--identify_tau", "-1"])
    assert [t["id"] for t in tracks] == [t["id"] for t in plain] and [t["hits"] for t in tracks] == [t["hits"] for t in plain]
    written = json.load(open(tmp_path / "out" / "tracks.json"))["tracks"]
    assert written == tracks
    for t in tracks:
        assert 1 <= t["template_rows"] <= t["hits"] and t["identity"] in gal.names.values() and -1.0 <= t["identity_score"] <= 1.0001
    with np.load(tmp_path / "out" / "tracks.npz") as z:
        assert z["ids"].tolist() == [t["id"] for t in tracks] and z["template_rows"].tolist() == [t["template_rows"] for t in tracks]
        assert z["templates"].shape == (len(tracks), emb.embedding_size) and z["templates"].dtype == np.float32
        assert np.isfinite(z["templates"]).all() and (np.abs(z["templates"]).sum(1) > 0).all()
    with pytest.raises(ValueError):
        TF.main(common + ["--td", str(tmp_path / "bad"), "--gallery", gpath])
