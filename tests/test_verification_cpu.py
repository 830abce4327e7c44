"""CPU tests of the embedder evaluation (verification.py, similar_face_filtering/evaluate_embedder.py): the report arithmetic on
histograms small enough to work by hand, the numpy restatement against a double loop, the entry points' refusals before any
launch, the CMC counting on a hand-made candidate table, and the program on its numpy path."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import verification_cases as VC
from face_detection_and_recognition_amd import _lib as L
from face_detection_and_recognition_amd import verification as V

P = ctypes.c_void_p(4096)     # a non-null, aligned pointer that is never dereferenced: every call here is refused first

EDGES4 = np.array([0.0, 0.25, 0.5, 0.75, 1.0])
GEN4, IMP4 = [1, 1, 2, 6], [12, 5, 2, 1]
# thresholds b = 0 .. 4:  TA = 10 9 8 6 0,  FA = 20 8 3 1 0,  TAR = 1 .9 .8 .6 0,  FAR = 1 .4 .15 .05 0,  FRR = 0 .1 .2 .4 1


def test_report_by_hand():
    r = V.verification_report(GEN4, IMP4, EDGES4, fars=(0.2, 0.05, 0.01))
    assert (r["n_genuine"], r["n_impostor"]) == (10, 20)
    assert np.allclose(r["tar"], [1, .9, .8, .6, 0], atol=1e-15) and np.allclose(r["far"], [1, .4, .15, .05, 0], atol=1e-15)
    assert np.array_equal(r["thresholds"], EDGES4)
    # trapezoids between consecutive thresholds: .6 * .95 + .25 * .85 + .1 * .7 + .05 * .3
    assert r["auc"] == pytest.approx(0.57 + 0.2125 + 0.07 + 0.015, abs=1e-12)
    # FAR - FRR = 1, .3, -.05, -.35, -1: b* = 2, the zero lies 6/7 of the way from b = 1 to b = 2
    assert r["eer"] == pytest.approx(0.4 - 6 / 7 * 0.25, abs=1e-12) and r["eer"] == pytest.approx(0.1 + 6 / 7 * 0.1, abs=1e-12)
    assert r["eer_threshold"] == pytest.approx(0.25 + 6 / 7 * 0.25, abs=1e-12)
    # accuracy (TA + I - FA) / 30 = 10, 21, 25, 25, 20 thirtieths: the tie goes to the first, b = 2
    assert r["best_accuracy"] == pytest.approx(25 / 30, abs=1e-15) and r["best_threshold"] == 0.5
    assert r["tar_at_far"][0.2] == dict(tar=pytest.approx(0.8), threshold=0.5, far=pytest.approx(0.15))
    assert r["tar_at_far"][0.05] == dict(tar=pytest.approx(0.6), threshold=0.75, far=pytest.approx(0.05))
    assert r["tar_at_far"][0.01] is None                    # 20 impostor pairs resolve no FAR below 1 / 20


def test_report_eer_on_an_exact_crossing():
    """FAR == FRR at a threshold: no interpolation needed, and the value is that threshold's."""
    r = V.verification_report([1, 3], [3, 1], [0.0, 0.5, 1.0])
    # b = 1: TAR = 3/4, FAR = 1/4, FRR = 1/4
    assert r["eer"] == pytest.approx(0.25, abs=1e-15) and r["eer_threshold"] == pytest.approx(0.5, abs=1e-15)
    assert r["auc"] == pytest.approx(0.75 * (1 + 0.75) / 2 + 0.25 * 0.75 / 2, abs=1e-15)


def test_report_accepts_device_style_tensors():
    r = V.verification_report(torch.tensor(GEN4), torch.tensor(IMP4), EDGES4)
    assert r["n_genuine"] == 10 and set(r["tar_at_far"]) == {1e-1, 1e-2, 1e-3, 1e-4}
    assert r["tar_at_far"][1e-1]["threshold"] == 0.75 and r["tar_at_far"][1e-2] is None


@pytest.mark.parametrize("empty", ["genuine", "impostor", "both"])
def test_report_empty_class(empty):
    g = [0, 0, 0, 0] if empty in ("genuine", "both") else GEN4
    i = [0, 0, 0, 0] if empty in ("impostor", "both") else IMP4
    r = V.verification_report(g, i, EDGES4)
    for k in ("auc", "eer", "eer_threshold"):
        assert math.isnan(r[k]), k
    assert np.isnan(r["tar"]).all() == (empty != "impostor") and np.isnan(r["far"]).all() == (empty != "genuine")
    assert all(v is None for v in r["tar_at_far"].values())
    if empty == "both":
        assert math.isnan(r["best_accuracy"])
    else:
        assert r["best_accuracy"] == 1.0                    # reject everything / accept everything
    with pytest.raises(ValueError):
        V.verification_report(GEN4, IMP4[:3], EDGES4)


def brute(X, labels, lo, hi, nbins):
    X = np.asarray(X, np.float64)
    out = np.zeros((2, nbins), np.int64)
    for i in range(len(X)):
        for j in range(i + 1, len(X)):
            if labels[i] < 0 or labels[j] < 0:
                continue
            ni, nj = math.sqrt(float(X[i] @ X[i])), math.sqrt(float(X[j] @ X[j]))
            if not (0 < ni < math.inf and 0 < nj < math.inf):
                continue
            s = float((X[i] / ni) @ (X[j] / nj))
            t = (s - lo) * (nbins / (hi - lo))
            out[0 if labels[i] == labels[j] else 1][0 if t < 0 else min(int(t), nbins - 1)] += 1
    return out


def test_numpy_histogram_against_double_loop():
    X, labels = VC.labelled_faces(7, 40, 16, 4)
    X = X.copy()
    X[3] = 0
    with np.errstate(over="ignore"):
        X[11, 2] = np.inf
    labels[5] = -1
    assert (labels < 0).sum() >= 1
    for lo, hi, nbins in ((-1.0, 1.0, 16), (-0.2, 0.5, 7), (0.0, 1.0, 2)):          # the narrow ranges clamp both ways
        want = brute(X, labels, lo, hi, nbins)
        got = V.pair_histogram_numpy(X, labels, lo, hi, nbins, block=16)
        assert np.array_equal(got["genuine"], want[0]) and np.array_equal(got["impostor"], want[1]), (lo, hi, nbins)
        assert got["genuine"].dtype == np.int64 and got["edges"].shape == (nbins + 1,) and got["edges"][0] == lo and got["edges"][-1] == hi
        live = int(VC.live_mask(X, labels).sum())
        assert want.sum() == live * (live - 1) // 2 and live < 38
    want = brute(X, labels, -0.2, 0.5, 7)
    assert want[1][0] > 0 and want[0][-1] > 0               # scores below lo and above hi were there to clamp
    one = V.pair_histogram_numpy(X, labels, -0.2, 0.5, 7, block=512)
    assert np.array_equal(one["genuine"], want[0]) and np.array_equal(one["impostor"], want[1])


def test_numpy_histogram_equals_the_oracle_of_the_cases():
    X, labels, g, i = VC.case(VC.EXACT[0])
    edges = VC.edges_of(-1.0, 1.0, 64)
    got = V.pair_histogram_numpy(X, labels, -1.0, 1.0, 64)
    # the two restatements (index arithmetic here, edge search there) may part only for a score within rounding of an edge
    assert np.abs(got["genuine"] - VC.oracle_histogram(g, edges)).sum() <= 2
    assert np.abs(got["impostor"] - VC.oracle_histogram(i, edges)).sum() <= 2
    assert VC.sandwich(got["genuine"], g, edges) == [] and VC.sandwich(got["impostor"], i, edges) == []
    bad = got["impostor"].copy()
    bad[30] += 1
    bad[40] -= 1
    assert VC.sandwich(bad, i, edges) != []                 # the sandwich notices one pair moved across ten bins


def test_pair_histogram_argument_errors():
    X, lab = torch.zeros((4, 32)), torch.zeros((4,), dtype=torch.int64)
    for kw in (dict(nbins=1), dict(nbins=L.PAIRHIST_MAX_BINS + 1), dict(lo=0.5, hi=0.5), dict(lo=1.0, hi=-1.0),
               dict(lo=float("nan")), dict(hi=float("inf"))):
        with pytest.raises(ValueError):
            V.pair_histogram(X, lab, **kw)
    with pytest.raises(ValueError):
        V.pair_histogram(np.zeros((4, 32), np.float32), lab)
    with pytest.raises(ValueError):
        V.pair_histogram(X[0], lab)
    for bad in (lab[:3], lab.float(), lab.bool(), [0, 0, 0, 0]):
        with pytest.raises(ValueError, match="labels"):
            V.pair_histogram(X, bad)
    with pytest.raises(ValueError, match="device"):
        V.pair_histogram(X, lab)                            # a host tensor: there is no CPU fallback behind this name
    with pytest.raises(ValueError):
        V.pair_histogram_numpy(np.zeros((4, 8)), np.zeros(4))   # float labels
    assert L.PAIRHIST_MAX_BINS == 1024


def test_entry_point_refusals(lib):
    def call(X=P, xinv=P, X3=P, labels=P, N=100, D=128, lo=-1.0, hi=1.0, nbins=64, gen=P, imp=P, ws=P, ws_bytes=1 << 30):
        return lib.fp_pair_histogram_x6(X, xinv, X3, labels, N, D, lo, hi, nbins, gen, imp, ws, ws_bytes, None)
    for name in ("X", "xinv", "X3", "labels", "gen", "imp", "ws"):
        assert call(**{name: None}) == L.FP_ERR_INVALID_ARG, name
    for kw in (dict(nbins=1), dict(nbins=1025), dict(nbins=0), dict(lo=0.5, hi=0.5), dict(lo=0.5, hi=0.25), dict(lo=float("nan")),
               dict(hi=float("nan")), dict(hi=float("inf")), dict(lo=float("-inf")), dict(D=100), dict(D=0), dict(N=-1)):
        assert call(**kw) == L.FP_ERR_INVALID_ARG, kw
    assert call(N=1 << 31) < 0
    assert call(X=ctypes.c_void_p(4100)) < 0 and call(ws=ctypes.c_void_p(4100)) < 0
    assert lib.fp_pair_histogram_workspace(100) == 128 * 8 and lib.fp_pair_histogram_workspace(129) == 256 * 8
    assert lib.fp_pair_histogram_workspace(0) == 0 and lib.fp_pair_histogram_workspace(1 << 31) == 0
    assert call(ws_bytes=128 * 8 - 1) == L.FP_ERR_INVALID_ARG
    assert lib.fp_abi_version() == 15                       # additions only


def test_header_declares_the_limit():
    from conftest import ROOT
    hdr = open(os.path.join(ROOT, "include", "facepath.h")).read()
    assert f"#define FP_PAIRHIST_MAX_BINS {L.PAIRHIST_MAX_BINS}\n" in hdr


def test_cmc_counts_by_hand():
    g_labels = torch.tensor([0, 0, 1, 2, 2, 7])
    q_labels = torch.tensor([0, 1, 2, 5, -1, 7, 1])
    top_idx = torch.tensor([[0, 2, 3],      # label 0: hit at rank 1
                            [3, 4, 2],      # label 1: gallery row 2 at rank 3
                            [0, 4, 3],      # label 2: rank 2 (and 3)
                            [0, 1, 2],      # label 5 is not enrolled: not mated
                            [0, 1, 2],      # label -1: not mated
                            [5, -1, -1],    # label 7: rank 1, then empty slots
                            [0, 1, -1]],    # label 1: never (an empty slot is no candidate, whatever row -1 would alias)
                           dtype=torch.int32)
    hits, n_mated = V.cmc_counts(top_idx, q_labels, g_labels)
    assert n_mated == 5 and hits.tolist() == [2, 3, 4]
    hits, n_mated = V.cmc_counts(top_idx[:0], q_labels[:0], g_labels)
    assert n_mated == 0 and hits.tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        V.cmc_counts(top_idx, q_labels[:3], g_labels)
    with pytest.raises(ValueError):
        V.identification_rates(torch.zeros((2, 32)), q_labels[:2], torch.zeros((3, 32)), g_labels[:3], k=17)


def test_evaluate_embedder_on_the_numpy_path(tmp_path, capsys):
    from face_detection_and_recognition_amd.similar_face_filtering import evaluate_embedder as E
    X, labels, g, i = VC.case(VC.EXACT[0])
    feats, out = tmp_path / "f.npz", tmp_path / "out"
    np.savez(feats, X=X, labels=labels)
    line = E.main(["--features", str(feats), "-d", "cpu", "--bins", "64", "--far", "0.1", "0.001", "1e-6", "--out", str(out)])
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert printed == json.loads(json.dumps(line)) == json.load(open(out / "report.json"))
    assert line["n_genuine"] == len(g) and line["n_impostor"] == len(i) and line["rows"] == 130 and line["bins"] == 64
    assert 0 < line["eer"] < 0.5 and 0.5 < line["auc"] <= 1 and -1 < line["eer_threshold"] < 1
    assert line["tar_at_far"]["1e-06"] is None and line["tar_at_far"]["0.1"]["far"] <= 0.1
    ref = V.verification_report(*(V.pair_histogram_numpy(X, labels, -1, 1, 64)[k] for k in ("genuine", "impostor", "edges")))
    assert line["eer_threshold"] == ref["eer_threshold"] and line["best_threshold"] == ref["best_threshold"]
    roc = np.load(out / "roc.npz")
    assert roc["thresholds"].shape == roc["tar"].shape == roc["far"].shape == (65,)
    assert (np.diff(roc["tar"]) <= 0).all() and (np.diff(roc["far"]) <= 0).all() and roc["far"][0] == 1 and roc["far"][-1] == 0
    assert int(roc["genuine"].sum()) == len(g) and int(roc["impostor"].sum()) == len(i)
    with pytest.raises(SystemExit):
        E.get_parsed_args([])                               # one of --ld / --features is required
    np.savez(feats, X=X)
    with pytest.raises(ValueError, match="labels"):
        E.main(["--features", str(feats), "-d", "cpu", "--out", str(out)])
