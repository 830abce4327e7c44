"""Tracker evaluation on the device: fp_mot_match against the numpy restatement on the inputs of the emulator test (seeded
sets, 3 x 7, 7 x 3, the full 64 x 64 frame, empty frames, sequences without rows) and on 32 sequences of different lengths in
one launch -- integers, gt_match / gt_switch, pot and the bits of sum_iou; two runs bit-identical; the hand cases B and C;
TrackingEvaluator fed from device tensors; StreamTracker scored against the identities its rows were built from."""
import numpy as np
import pytest
import torch

import moteval_cases as MC
import track_cases as TC
from face_detection_and_recognition_amd import tracking as T
from face_detection_and_recognition_amd import tracking_eval as TE

pytestmark = pytest.mark.gpu

EMU = MC.emulator_inputs()
EMU["32seqs"] = MC.many_sequences()
EMU["merged"] = MC.combine([EMU["seed1"], EMU["64x64"], EMU["seed4"]], merge_seed=3)


@pytest.fixture(scope="module")
def numpy_results():
    return {name: TE.mot_eval(**data) for name, data in EMU.items()}


@pytest.mark.parametrize("name", sorted(EMU))
def test_device_equals_numpy(name, numpy_results, dev):
    got = TE.mot_eval(**EMU[name], device=dev)
    MC.assert_same_result(got, numpy_results[name], name)
    for key in TE.DERIVED_KEYS:
        assert got.combined[key] == numpy_results[name].combined[key], key


def test_two_device_runs_are_bit_identical(dev):
    data = {k: torch.from_numpy(v).to(dev) for k, v in EMU["merged"].items()}
    with torch.cuda.device(dev):
        pb = TE._Problem(*(data[k] for k in MC.KEYS), 0.5, dev)
        first, second = TE._match_device(pb), TE._match_device(pb)
    for key in first:
        assert first[key].cpu().numpy().tobytes() == second[key].cpu().numpy().tobytes(), key
    assert int(first["counts"][:, 0].sum()) > 0


@pytest.mark.parametrize("name", ["B", "C"])
def test_hand_case_on_the_device(name, dev):
    data, want = MC.hand_cases()[name]
    res = TE.mot_eval(**data, device=dev)
    assert {k: res.combined[k] for k in want} == want
    assert list(res.gt_match) == ([0, 2] if name == "B" else [1, 0])


def test_evaluator_fed_from_device_tensors_in_three_batches(numpy_results, dev):
    data = MC.seeded_set(31, n_frames=12, n_targets=3)
    for key in ("gt_boxes", "hy_boxes"):
        data[key] = np.round(data[key])                     # integer pixels survive xywh -> xyxy -> xywh
    want = TE.mot_eval(**data)
    ev = TE.TrackingEvaluator(1, dev).set_ground_truth(*(data[k] for k in MC.KEYS[:4]), data["n_frames"])
    edges = [0, 5, 6, 12]
    for lo, hi in zip(edges[:-1], edges[1:]):
        sel = np.nonzero((data["hy_frame"] >= lo) & (data["hy_frame"] < hi))[0]
        b = data["hy_boxes"][sel]
        info = np.concatenate([(data["hy_frame"][sel] - lo)[:, None], b[:, :2], b[:, :2] + b[:, 2:]], 1).astype(np.float32)
        info = np.concatenate([info, [[0, 0, 0, 9, 9]]]).astype(np.float32)            # a row the tracker gave no id
        tid = np.concatenate([data["hy_id"][sel], [0]]).astype(np.int32)
        d_info, d_tid = torch.from_numpy(info).to(dev), torch.from_numpy(tid).to(dev)
        ev.add(torch.zeros(hi - lo, dtype=torch.int32, device=dev), lo, d_info[:, 0].to(torch.int32), d_info[:, 1:5], d_tid)
    got = ev.evaluate()
    assert ev.dropped == 3
    for key in MC.INT_KEYS:
        assert got.combined[key] == want.combined[key], key
    assert got.combined["sum_iou"] == want.combined["sum_iou"]
    assert want.TP > 0 and want.FN + want.FP > 0


def _identity_rows(D=32, K=5, F=12, S=2, seed=3):
    """S streams x F frames x K identities in disjoint cells, identity k of stream s absent in frame 3 + k (one-frame gaps).
    -> batches of (frame, boxes, emb, stream_of_frame, frame numbers, identity of every row)."""
    rng = np.random.default_rng(seed)
    idents = TC.ortho(D, K * S, seed)
    batches = []
    for lo, hi in ((0, 5), (5, F)):
        sof = np.array([s for f in range(lo, hi) for s in range(S)], np.int32)
        number = np.array([f for f in range(lo, hi) for s in range(S)], np.int64)
        frame, boxes, emb, who = [], [], [], []
        for b, (s, f) in enumerate(zip(sof, number)):
            for k in range(K):
                if f == 3 + k:
                    continue
                frame.append(b)
                boxes.append(TC.cell(k))
                emb.append(TC.obs(idents[s * K + k], 0.95, rng))
                who.append(k + 1)
        batches.append((np.array(frame, np.int32), np.array(boxes, np.float32), np.array(emb, np.float32), sof, number,
                        np.array(who, np.int64)))
    return batches, S, F


@pytest.mark.parametrize("max_age", [3, 0])
def test_stream_tracker_scored_against_its_own_identities(max_age, dev):
    batches, S, F = _identity_rows()
    tracker = T.StreamTracker(S, 32, max_age, device=dev)
    ev = TE.TrackingEvaluator(S, dev)
    gt_seq, gt_frame, gt_id, gt_boxes = [], [], [], []
    for frame, boxes, emb, sof, number, who in batches:
        d = [torch.from_numpy(x).to(dev) for x in (frame, boxes, emb, sof)]
        out = tracker.step(*d)
        ev.add(d[3], torch.from_numpy(number).to(dev), d[0], d[1], out["track_id"])
        gt_seq.append(sof[frame].astype(np.int64))
        gt_frame.append(number[frame])
        gt_id.append(who)
        gt_boxes.append(np.concatenate([boxes[:, :2], boxes[:, 2:] - boxes[:, :2]], 1).astype(np.float64))
    ev.set_ground_truth(*(np.concatenate(x) for x in (gt_seq, gt_frame, gt_id, gt_boxes)), [F] * S)
    res = ev.evaluate()
    assert ev.dropped == 0 and res.FN == 0 and res.FP == 0 and res.TP == S * 5 * (F - 1) and res.MOTP == 1.0
    assert res.Frag == S * 5                                 # every identity is absent once: two runs each (case E)
    if max_age == 3:
        assert res.IDSW == 0 and res.IDF1 == 1.0 and res.MOTA == 1.0
    else:                                                    # a track unseen for one frame is freed: the id is reopened
        assert res.IDSW > 0 and res.IDF1 < 1.0
