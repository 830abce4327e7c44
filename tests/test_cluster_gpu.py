"""Cosine DBSCAN on the device (clustering.dbscan_cosine / cluster_summary, csrc/cluster.hip) against the fp64 oracle of
cluster_cases.py.  Every threshold sits in a gap of the fp64 scores at least 2 GAP wide, so the device's fp32-equivalent
decisions are unambiguous and degree, core and labels must EQUAL the oracle's."""
import os

import numpy as np
import pytest
import torch

import cluster_cases as CC

pytestmark = pytest.mark.gpu


def run(X, tau, ms, dev):
    from face_detection_and_recognition_amd.clustering import dbscan_cosine
    res = dbscan_cosine(torch.tensor(np.asarray(X)).to(dev), tau, ms)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("labels", "core", "degree", "n_clusters"))


def check(res, degree, core, labels):
    assert res["degree"].dtype == np.int32 and res["labels"].dtype == np.int32 and res["core"].dtype == bool
    assert np.array_equal(res["degree"], degree)
    assert np.array_equal(res["core"], core)
    assert np.array_equal(res["labels"], labels)
    assert res["n_clusters"].shape == (1,) and int(res["n_clusters"][0]) == int(labels.max(initial=-1)) + 1


@pytest.mark.parametrize("ms", CC.MIN_SAMPLES)
@pytest.mark.parametrize("seed", [c[0] for c in CC.CASES])
def test_dbscan_against_fp64(dev, seed, ms):
    X, S, tau, A = CC.case(seed)
    assert CC.ambiguous(S, tau) == 0
    res = run(X, tau, ms, dev)
    check(res, *CC.oracle(seed, ms))
    assert same(res, run(X, tau, ms, dev))                  # bit-identical


def test_chain(dev):
    """One component that spans every row tile, with long root paths: X[i] = e_i + e_(i+1), rows permuted."""
    N, D = 300, 320
    X = np.zeros((N, D), np.float32)
    X[np.arange(N), np.arange(N)] = 1
    X[np.arange(N), np.arange(N) + 1] = 1
    perm = np.random.default_rng(45).permutation(N)
    X = X[perm]
    S = CC.cosine64(X)
    assert CC.ambiguous(S, 0.4) == 0
    A = CC.edges(S, 0.4)
    assert A.sum() == 2 * (N - 1)
    for ms in (1, 3, 4):
        res = run(X, 0.4, ms, dev)
        check(res, *CC.restate(A, ms))
        if ms == 1:
            assert int(res["n_clusters"][0]) == 1 and (res["labels"] == 0).all()
        if ms == 3:
            assert int(res["n_clusters"][0]) == 1 and (res["labels"] == 0).all() and int(res["core"].sum()) == N - 2
        if ms == 4:
            assert int(res["n_clusters"][0]) == 0 and (res["labels"] == -1).all() and not res["core"].any()


def test_one_big_identity(dev):
    """Every pair is an edge: 523 776 unions into one root, with exact duplicates among the rows."""
    N, D = 1024, 128
    rng = np.random.default_rng(46)
    c = rng.normal(0, 1, D)
    c /= np.linalg.norm(c)
    X = (c + rng.normal(0, 1, (N, D)) * (0.3 / np.sqrt(D))).astype(np.float32)
    X[100:164] = X[7]
    S = CC.cosine64(X)
    tau = 0.5
    assert CC.ambiguous(S, tau) == 0 and S.min() > tau + CC.GAP
    for ms in (1, 64):
        res = run(X, tau, ms, dev)
        assert (res["labels"] == 0).all() and (res["degree"] == N).all() and res["core"].all()
        assert int(res["n_clusters"][0]) == 1
        assert same(res, run(X, tau, ms, dev))


def test_dead_rows_and_edges(dev):
    X, S, tau, A = CC.case(41)
    X = X.copy()
    dead = [0, 5, 64, 129]
    X[[0, 64, 129]] = 0
    X[5] = np.inf
    live = np.ones(X.shape[0], bool)
    live[dead] = False
    Al = A & live[:, None] & live[None, :]                  # the graph with those rows removed
    for ms in (1, 2, 5):
        res = run(X, tau, ms, dev)
        assert (res["degree"][dead] == 0).all() and not res["core"][dead].any() and (res["labels"][dead] == -1).all()
        check(res, *CC.restate(Al, ms, live))
    one = np.ones((1, 32), np.float32)
    r = run(one, 0.5, 1, dev)
    assert r["labels"].tolist() == [0] and r["core"].tolist() == [True] and r["degree"].tolist() == [1] and r["n_clusters"].tolist() == [1]
    r = run(one, 0.5, 2, dev)
    assert r["labels"].tolist() == [-1] and r["core"].tolist() == [False] and r["degree"].tolist() == [1] and r["n_clusters"].tolist() == [0]
    r = run(np.zeros((0, 32), np.float32), 0.5, 1, dev)
    assert all(r[k].shape == (0,) for k in ("labels", "core", "degree")) and r["n_clusters"].tolist() == [0]
    X, S, _, _ = CC.case(41)
    r = run(X, 1.5, 1, dev)                                 # above every score: N singletons
    assert np.array_equal(r["labels"], np.arange(X.shape[0])) and (r["degree"] == 1).all() and int(r["n_clusters"][0]) == X.shape[0]


def test_cluster_summary(dev):
    from face_detection_and_recognition_amd.clustering import cluster_summary
    for seed in (41, 42):
        X, S, tau, A = CC.case(seed)
        labels = CC.oracle(seed, 5)[2]
        Xd, ld = torch.tensor(X).to(dev), torch.tensor(labels).to(dev)
        out = cluster_summary(Xd, ld)
        again = cluster_summary(Xd, ld)
        torch.cuda.synchronize()
        C = int(labels.max()) + 1
        sizes, cent, med = out["sizes"].cpu().numpy(), out["centroids"].cpu().numpy(), out["medoid"].cpu().numpy()
        assert np.array_equal(sizes, np.bincount(labels[labels >= 0], minlength=C))
        assert cent.shape == (C, X.shape[1]) and med.shape == (C,)
        Xn = X.astype(np.float64)
        Xn /= np.linalg.norm(Xn, axis=1, keepdims=True)
        for c in range(C):
            members = np.nonzero(labels == c)[0]
            ref = Xn[members].sum(0)
            ref /= np.linalg.norm(ref)
            assert np.abs(cent[c] - ref).max() <= 1e-4, (seed, c)
            score = Xn[members] @ ref
            assert med[c] in members
            assert Xn[med[c]] @ ref >= score.max() - CC.GAP, (seed, c)
        for k in ("sizes", "centroids", "medoid"):
            assert torch.equal(out[k], again[k]), k


def test_from_clusters_roundtrip(dev):
    from face_detection_and_recognition_amd.gallery import FaceGallery
    X, S, tau, A = CC.case(42)
    res = run(X, tau, 5, dev)
    labels = res["labels"]
    Xd = torch.tensor(X).to(dev)
    gal = FaceGallery.from_clusters(Xd, torch.as_tensor(labels), device=dev)
    keep = np.nonzero(labels >= 0)[0]
    assert len(gal) == keep.size and gal.name_of(7) == "cluster_0007" and gal.name_of(-1) == "unknown"
    out = gal.identify(Xd[torch.as_tensor(keep).to(dev)], k=1, tau=0.0)
    torch.cuda.synchronize()
    assert np.array_equal(out["label"].cpu().numpy(), labels[keep])
    assert np.array_equal(out["top_idx"].cpu().numpy()[:, 0], np.arange(keep.size))
    assert np.abs(out["score"].cpu().numpy() - 1).max() <= 1e-5
    cg = FaceGallery.from_clusters(Xd, torch.as_tensor(labels), device=dev, centroids_only=True)
    assert len(cg) == int(labels.max()) + 1 and cg.labels.cpu().tolist() == list(range(len(cg)))


def test_cluster_faces_cli(dev, tmp_path):
    """The driver end to end on synthetic weights: copies of one image land in one cluster, every file where dbscan_cosine on
    embed_images of the same files says, and clusters.npz holds what was printed."""
    from PIL import Image
    from face_detection_and_recognition_amd.clustering import dbscan_cosine
    from face_detection_and_recognition_amd.modules.mobile_facenet.mobile_facenet import MobileFaceNet
    from face_detection_and_recognition_amd.similar_face_filtering import cluster_faces as CF
    from face_detection_and_recognition_amd.synth import synth_state_dict
    rng = np.random.default_rng(0)
    net = MobileFaceNet(512)
    net.load_state_dict(synth_state_dict(net.state_dict(), 300))
    wpath = str(tmp_path / "mfn.pth")
    torch.save(net.state_dict(), wpath)
    os.makedirs(tmp_path / "unl" / "nested")
    twins = {}
    for c in ("a", "b"):
        base = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
        Image.fromarray(base).save(tmp_path / "unl" / f"{c}_0.jpg", quality=95)
        for i in (1, 2):                                    # byte copies: cosine 1 with the original
            dst = tmp_path / "unl" / ("nested" if i == 2 else "") / f"{c}_{i}.jpg"
            dst.write_bytes((tmp_path / "unl" / f"{c}_0.jpg").read_bytes())
        twins[c] = [f"{c}_0.jpg", f"{c}_1.jpg", f"nested_{c}_2.jpg"]
    for i in range(4):
        Image.fromarray(rng.integers(0, 256, (48 + 8 * i, 64, 3), dtype=np.uint8)).save(tmp_path / "unl" / f"noise_{i}.jpg", quality=95)
    argv = ["--ud", str(tmp_path / "unl"), "--td", str(tmp_path / "out"), "-m", wpath, "-b", "4", "--tau", "0.999", "--min_samples", "3",
            "-d", "hip:0"]
    groups = CF.main(argv)
    paths = CF.unlabelled_images(str(tmp_path / "unl"))
    assert len(paths) == 10 and sum(g[1] for g in groups) == 10 and groups[-1][0] == "noise"
    landed = {f: d for d, _, _ in groups for f in os.listdir(tmp_path / "out" / d)}
    assert len(landed) == 10
    for c, files in twins.items():
        assert len({landed[f] for f in files}) == 1 and landed[files[0]].startswith("cluster_"), c
    args = CF.get_parsed_args(argv)
    feats = CF.embed_images(CF.load_model(args), paths, 4, preprocess=args.preprocess)
    lab = dbscan_cosine(feats, 0.999, 3)["labels"].cpu().tolist()
    for p, l in zip(paths, lab):
        assert landed[CF.target_name(p, str(tmp_path / "unl"))] == CF.cluster_name(l), p
    with np.load(tmp_path / "out" / "clusters.npz", allow_pickle=False) as z:
        assert z["paths"].tolist() == paths and z["labels"].tolist() == lab
        assert z["centroids"].shape == (max(lab) + 1, 512) and z["medoid"].shape == (max(lab) + 1,)
        for c, m in enumerate(z["medoid"].tolist()):
            assert lab[m] == c
