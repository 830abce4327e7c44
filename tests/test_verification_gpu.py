"""The pair histogram on the device (verification.pair_histogram, csrc/pairhist.hip) against the fp64 oracle of
verification_cases.py: EQUAL where every score keeps 2 GAP from every edge, inside the GAP sandwich elsewhere, with exact totals
and bit-identical repeats throughout; then identification_rates and the evaluate_embedder program."""
import json
from math import comb

import numpy as np
import pytest
import torch

import verification_cases as VC

pytestmark = pytest.mark.gpu


def run(X, labels, lo, hi, nbins, dev):
    from face_detection_and_recognition_amd.verification import pair_histogram
    res = pair_histogram(torch.tensor(np.asarray(X)).to(dev), torch.tensor(np.asarray(labels)).to(dev), lo, hi, nbins)
    torch.cuda.synchronize()
    assert res["genuine"].dtype == torch.int64 and res["genuine"].shape == (nbins,) and res["impostor"].shape == (nbins,)
    assert res["edges"].shape == (nbins + 1,) and res["edges"][0] == lo and res["edges"][-1] == hi
    return res["genuine"].cpu().numpy(), res["impostor"].cpu().numpy()


def in_sandwich(X, labels, lo, hi, nbins, dev, max_share=None):
    """Run on the device and hold both classes against the sandwich of the live pairs' fp64 scores -> (genuine, impostor)."""
    g64, i64 = VC.pair_scores(X, labels)
    edges = VC.edges_of(lo, hi, nbins)
    if max_share is not None:
        share = max(VC.ambiguous_share(g64, edges), VC.ambiguous_share(i64, edges))
        print(f"ambiguous share {share:.5f}")
        assert share <= max_share
    g, i = run(X, labels, lo, hi, nbins, dev)
    live = int(VC.live_mask(X, labels).sum())
    assert int(g.sum()) == len(g64) and int(i.sum()) == len(i64) and len(g64) + len(i64) == comb(live, 2)
    assert VC.sandwich(g, g64, edges) == []
    assert VC.sandwich(i, i64, edges) == []
    return g, i


@pytest.mark.parametrize("nbins", (8, 16))
def test_exact(dev, nbins):
    X, labels, g64, i64 = VC.case(VC.EXACT[0])
    lo, hi, margin = VC.exact_range(nbins)
    print(f"margin {margin:.3e} at lo = {lo}")
    assert margin >= 2 * VC.GAP
    edges = VC.edges_of(lo, hi, nbins)
    g, i = run(X, labels, lo, hi, nbins, dev)
    assert np.array_equal(g, VC.oracle_histogram(g64, edges))
    assert np.array_equal(i, VC.oracle_histogram(i64, edges))
    assert g.sum() > 300 and i.sum() > 5000 and (g > 0).sum() >= 3 and (i > 0).sum() >= 3


@pytest.mark.parametrize("nbins", (64, 1024))
@pytest.mark.parametrize("seed", [c[0] for c in VC.CASES])
def test_sandwich(dev, seed, nbins):
    X, labels, g64, i64 = VC.case(seed)
    edges = VC.edges_of(-1.0, 1.0, nbins)
    share = (VC.ambiguous_share(g64, edges) * len(g64) + VC.ambiguous_share(i64, edges) * len(i64)) / (len(g64) + len(i64))
    print(f"ambiguous share {share:.5f}")
    assert share <= 0.02
    g, i = run(X, labels, -1.0, 1.0, nbins, dev)
    assert int(g.sum()) == len(g64) and int(i.sum()) == len(i64)                  # (a)
    assert VC.sandwich(g, g64, edges) == [] and VC.sandwich(i, i64, edges) == []  # (a) (b) (c)
    g2, i2 = run(X, labels, -1.0, 1.0, nbins, dev)
    assert np.array_equal(g, g2) and np.array_equal(i, i2)                        # (d)


@pytest.mark.parametrize("N,D", [(1, 32), (2, 32), (127, 32), (128, 32), (129, 32), (257, 32), (200, 100)])
def test_tile_edges_and_padding(dev, N, D):
    X, labels = VC.labelled_faces(50 + N, N, D, 5)
    labels = np.where(labels < 0, 3, labels)                # every row live: the count is C(N, 2)
    g, i = in_sandwich(X, labels, -1.0, 1.0, 64, dev)
    assert int(g.sum() + i.sum()) == comb(N, 2)
    if N == 1:
        assert not g.any() and not i.any()


def test_no_rows(dev):
    from face_detection_and_recognition_amd.verification import pair_histogram
    res = pair_histogram(torch.zeros((0, 64), device=dev), torch.zeros((0,), dtype=torch.int32, device=dev), nbins=16)
    assert not res["genuine"].any() and not res["impostor"].any() and res["genuine"].shape == (16,)


def test_masks(dev):
    """Zero rows, a row with an inf, label -1 rows -- some of each past the first tile boundary: none is counted."""
    X, labels = VC.labelled_faces(61, 300, 64, 6)
    X, labels = X.copy(), np.where(labels < 0, 2, labels)
    X[[4, 130, 299]] = 0
    X[[17, 200], 3] = np.inf
    X[260, 5] = np.nan
    labels[[0, 9, 129, 256, 298]] = -1
    live = VC.live_mask(X, labels)
    assert int(live.sum()) == 300 - 11
    g, i = in_sandwich(X, labels, -1.0, 1.0, 256, dev, max_share=0.02)
    g2, i2 = in_sandwich(X[live], labels[live], -1.0, 1.0, 256, dev)
    # the live subset alone: a score is a function of its two rows (same operand roles, same order of the features), not of
    # where the rows sit
    assert np.array_equal(g, g2) and np.array_equal(i, i2)
    from face_detection_and_recognition_amd.verification import pair_histogram
    xinv = torch.ones((300,), device=dev)                   # a caller's own inverse norms with dead entries
    xinv[[1, 2, 140]] = torch.tensor([0.0, float("inf"), float("nan")], device=dev)
    Xu = torch.tensor(VC.labelled_faces(61, 300, 64, 6)[0]).to(dev)
    Xu = Xu / Xu.norm(dim=1, keepdim=True)
    res = pair_histogram(Xu, torch.zeros((300,), dtype=torch.int16, device=dev), xinv=xinv)
    assert int(res["genuine"].sum()) == comb(297, 2) and not res["impostor"].any()


def test_label_extremes(dev):
    X, labels = VC.labelled_faces(62, 400, 96, 7)
    one, distinct = np.full(400, 5), np.arange(400)
    g, i = in_sandwich(X, one, -1.0, 1.0, 1024, dev)
    assert not i.any() and int(g.sum()) == comb(400, 2)
    g, i = in_sandwich(X, distinct, -1.0, 1.0, 1024, dev)
    assert not g.any() and int(i.sum()) == comb(400, 2)
    # exact duplicates: a score of about 1.0 is at or above hi = 1 or a hair below -- the last bin either way
    Xd = np.concatenate([X[:150], X[:150]])
    ld = np.concatenate([np.arange(150), np.arange(150)])
    g, i = in_sandwich(Xd, ld, -1.0, 1.0, 1024, dev)
    assert int(g[-1]) == 150 and int(g.sum()) == 150
    # lo = 0: every negative score lands in bin 0
    g64, i64 = VC.pair_scores(X, labels)
    g, i = in_sandwich(X, labels, 0.0, 1.0, 32, dev)
    e1 = 1.0 / 32
    assert (i64 < 0).sum() > 1000
    assert (i64 < e1 - VC.GAP).sum() <= int(i[0]) <= (i64 < e1 + VC.GAP).sum() and int(i[0]) > (i64 < 0).sum()


def test_64_bit_counters_and_one_bin_contention(dev):
    """X[i] = e_(i mod 4), labels = i mod 4: every score is exactly 0 (bin 512 of 1024 over [-1, 1]) or 1 (the last bin).  The
    smallest input whose impostor count passes 2^32, and the case in which every lane of every wave adds to one bin."""
    from face_detection_and_recognition_amd.verification import pair_histogram
    N = 131072
    lab = torch.arange(N, device=dev) % 4
    X = torch.zeros((N, 32), device=dev)
    X[torch.arange(N, device=dev), lab] = 1.0
    res = pair_histogram(X, lab, -1.0, 1.0, 1024)
    g, i = res["genuine"].cpu().numpy(), res["impostor"].cpu().numpy()
    assert int(i[512]) == 6 * 32768 ** 2 == 6442450944 and int(i.sum()) == int(i[512])
    assert int(g[1023]) == 4 * comb(32768, 2) == 2147418112 and int(g.sum()) == int(g[1023])


def test_identification_rates(dev):
    from face_detection_and_recognition_amd.similarity import cosine_topk
    from face_detection_and_recognition_amd.verification import identification_rates
    X, labels = VC.labelled_faces(63, 900, 128, 30)
    G, gl, Q, ql = X[:600], labels[:600].copy(), X[600:], labels[600:].copy()
    keep = (gl >= 0) & (gl != 4) & (gl != 11)               # identities 4 and 11 are not enrolled
    G, gl = G[keep], gl[keep]
    Qd, Gd = torch.tensor(Q).to(dev), torch.tensor(G).to(dev)
    res = identification_rates(Qd, torch.tensor(ql), Gd, torch.tensor(gl), k=5)
    _, idx = cosine_topk(Qd, Gd, 5)
    idx = idx.cpu().numpy()
    mated = (ql >= 0) & np.isin(ql, gl)
    assert (ql < 0).any() and np.isin(ql, (4, 11)).any() and mated.sum() < len(ql)
    assert res["n_mated"] == int(mated.sum())
    want = [int(((gl[idx[:, :r]] == ql[:, None]).any(1) & mated).sum()) for r in range(1, 6)]
    assert res["hits"].tolist() == want
    assert np.array_equal(res["rate"], np.asarray(want) / mated.sum())
    assert (np.diff(res["rate"]) >= 0).all() and 0.5 < res["rate"][0] < res["rate"][-1] <= 1.0
    from face_detection_and_recognition_amd.gallery import FaceGallery
    gal = FaceGallery(Gd, torch.tensor(gl, dtype=torch.int32), device=dev)
    assert identification_rates(Qd, torch.tensor(ql), gal, k=5)["hits"].tolist() == want


def test_evaluate_embedder_program(dev, tmp_path, capsys):
    from face_detection_and_recognition_amd import verification as V
    from face_detection_and_recognition_amd.similar_face_filtering import evaluate_embedder as E
    X, labels, g64, i64 = VC.case(42)                       # look-alike identities, N = 700
    feats, out = tmp_path / "f.npz", tmp_path / "out"
    np.savez(feats, X=X, labels=labels)
    line = E.main(["--features", str(feats), "--out", str(out)])
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert printed == json.load(open(out / "report.json")) == json.loads(json.dumps(line))
    assert line["n_genuine"] == len(g64) and line["n_impostor"] == len(i64) and line["bins"] == 1024
    assert 0 <= line["eer"] <= 1 and 0.5 < line["auc"] <= 1 and 0 < line["best_accuracy"] <= 1
    roc = np.load(out / "roc.npz")
    assert (np.diff(roc["tar"]) <= 0).all() and (np.diff(roc["far"]) <= 0).all()
    assert roc["tar"][0] == 1 and roc["far"][0] == 1 and roc["tar"][-1] == 0 and roc["far"][-1] == 0
    h = V.pair_histogram(torch.tensor(X).to(dev), torch.tensor(labels).to(dev))
    ref = V.verification_report(h["genuine"], h["impostor"], h["edges"])
    assert line["eer_threshold"] == ref["eer_threshold"] and line["eer"] == ref["eer"]
    assert np.array_equal(roc["genuine"], h["genuine"].cpu().numpy())
    far3 = line["tar_at_far"]["0.001"]
    assert far3 is not None and far3["far"] <= 1e-3 and 0 < far3["threshold"] < 1
