"""CPU tests of cosine DBSCAN: the fp64 oracle against scikit-learn, the entry points' refusals before any launch, the workspace
size, the driver's file grouping and FaceGallery.from_clusters' argument errors."""
import ctypes
import os

import numpy as np
import pytest

import cluster_cases as CC
from face_detection_and_recognition_amd import _lib as L

P = ctypes.c_void_p(4096)     # a non-null, aligned pointer that is never dereferenced: every call here is refused first


@pytest.mark.parametrize("seed", [c[0] for c in CC.CASES])
def test_threshold_is_unambiguous(seed):
    X, S, tau, A = CC.case(seed)
    _, gap = CC.choose_tau(S)
    assert 0.45 < tau < 0.55 and gap >= 2 * CC.GAP
    assert CC.ambiguous(S, tau) == 0
    s = S[np.triu_indices(S.shape[0], 1)]
    assert ((s >= 0.45) & (s <= 0.55)).sum() > 100          # the threshold cuts through real data


@pytest.mark.parametrize("seed", [c[0] for c in CC.CASES])
def test_oracle_equals_sklearn(seed):
    cluster = pytest.importorskip("sklearn.cluster")
    A = CC.case(seed)[3]
    dist = np.where(A, 0., 1.)
    np.fill_diagonal(dist, 0.)                              # a point is its own neighbour
    for ms in CC.MIN_SAMPLES:
        degree, core, labels = CC.oracle(seed, ms)
        sk = cluster.DBSCAN(eps=0.5, min_samples=ms, metric="precomputed").fit(dist)
        assert np.array_equal(labels, sk.labels_), (seed, ms)
        assert np.array_equal(np.nonzero(core)[0], sk.core_sample_indices_), (seed, ms)
        assert np.array_equal(degree, 1 + A.sum(1))


def test_what_the_cases_contain():
    """The structures the GPU tests rely on are present: clusters, border points contested between clusters, noise."""
    want = {41: (6, 29, 33), 42: (17, 140, 311), 43: (17, 104, 1009), 44: (31, 279, 1239)}
    contested = {}
    for seed, (n_clusters, n_border, n_noise) in want.items():
        A = CC.case(seed)[3]
        degree, core, labels = CC.oracle(seed, 5)
        border = ~core & (labels >= 0)
        assert (labels.max() + 1, int(border.sum()), int((labels < 0).sum())) == (n_clusters, n_border, n_noise), seed
        contested[seed] = sum(len(set(labels[np.nonzero(A[i] & core)[0]])) > 1 for i in np.nonzero(border)[0])
    assert contested[42] > 0 and contested[44] > 0
    assert [int(CC.oracle(s, 1)[2].max()) + 1 for s in want] == [34, 280, 1009, 1151]


def test_dbscan_refusals(lib):
    def call(X=P, xinv=P, X3=P, N=100, D=128, ms=5, degree=P, core=P, labels=P, nc=P, ws=P, ws_bytes=1 << 30):
        return lib.fp_cosine_dbscan_x6(X, xinv, X3, N, D, 0.5, ms, degree, core, labels, nc, ws, ws_bytes, None)
    for name in ("X", "xinv", "X3", "degree", "core", "labels", "nc", "ws"):
        assert call(**{name: None}) == L.FP_ERR_INVALID_ARG, name
    assert call(N=0) == L.FP_ERR_INVALID_ARG and call(N=-1) == L.FP_ERR_INVALID_ARG
    assert call(N=1 << 31) < 0
    assert call(D=100) < 0 and call(D=0) < 0
    assert call(ms=0) == L.FP_ERR_INVALID_ARG and call(ms=65) == L.FP_ERR_INVALID_ARG
    assert call(X=ctypes.c_void_p(4100)) < 0 and call(ws=ctypes.c_void_p(4100)) < 0
    need = lib.fp_cosine_dbscan_workspace(100, 5)
    assert need > 0
    assert call(ws_bytes=need - 1) == L.FP_ERR_INVALID_ARG


def test_centroid_refusals(lib):
    def call(X=P, xinv=P, order=P, offsets=P, C=3, D=128, cent=P, med=P):
        return lib.fp_cluster_centroids(X, xinv, order, offsets, C, D, cent, med, None)
    for name in ("X", "xinv", "order", "offsets", "cent", "med"):
        assert call(**{name: None}) == L.FP_ERR_INVALID_ARG, name
    assert call(C=-1) == L.FP_ERR_INVALID_ARG and call(D=0) == L.FP_ERR_INVALID_ARG
    assert call(D=1 << 20) < 0
    assert call(C=0) == L.FP_OK                              # nothing to do, nothing launched


def test_dbscan_workspace_monotone(lib):
    ws = lib.fp_cosine_dbscan_workspace
    for ms in (1, 2, 3, 12, 64):
        sizes = [ws(N, ms) for N in (1, 100, 128, 129, 5000, 125000, (1 << 31) - 1)]
        assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:])), (ms, sizes)
    for N in (1, 1000, 100000):
        sizes = [ws(N, ms) for ms in range(1, 65)]
        assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:])), (N, sizes)
        assert sizes[-1] > sizes[0]
    assert ws(0, 5) == 0 and ws(100, 0) == 0 and ws(100, 65) == 0 and ws(1 << 31, 5) == 0
    assert L.DBSCAN_MAX_MIN_SAMPLES == 64


def test_group_files_and_npz(tmp_path):
    from face_detection_and_recognition_amd.similar_face_filtering import cluster_faces as CF
    root = tmp_path / "unl"
    os.makedirs(root / "a" / "b")
    rel = ["x0.jpg", "x1.jpg", os.path.join("a", "y0.jpg"), os.path.join("a", "b", "z0.jpg"), "x2.jpg", os.path.join("a", "y1.jpg")]
    paths = []
    for i, r in enumerate(rel):
        (root / r).write_bytes(bytes([i]) * 10)
        paths.append(str(root / r))
    labels = np.array([1, -1, 0, 1, -1, 0], np.int32)
    medoid = np.array([5, 3], np.int32)
    target = tmp_path / "out"
    groups = CF.group_files(paths, labels, medoid, str(root), str(target))
    assert groups == [("cluster_0000", 2, "a_y1.jpg"), ("cluster_0001", 2, "a_b_z0.jpg"), ("noise", 2, None)]
    assert sorted(os.listdir(target)) == ["cluster_0000", "cluster_0001", "noise"]
    assert sorted(os.listdir(target / "cluster_0000")) == ["a_y0.jpg", "a_y1.jpg"]
    assert sorted(os.listdir(target / "cluster_0001")) == ["a_b_z0.jpg", "x0.jpg"]
    assert sorted(os.listdir(target / "noise")) == ["x1.jpg", "x2.jpg"]
    assert (target / "cluster_0001" / "a_b_z0.jpg").read_bytes() == bytes([3]) * 10
    assert CF.cluster_name(7) == "cluster_0007" and CF.cluster_name(-1) == "noise"
    with pytest.raises(ValueError):
        CF.group_files(paths, labels[:-1], medoid, str(root), str(target))
    with pytest.raises(ValueError):
        CF.group_files(paths, labels, medoid[:1], str(root), str(target))
    # everything noise: only the noise folder
    only = CF.group_files(paths[:2], [-1, -1], [], str(root), str(tmp_path / "out2"))
    assert only == [("noise", 2, None)] and os.listdir(tmp_path / "out2") == ["noise"]

    core = labels >= 0
    degree = np.array([3, 1, 2, 3, 1, 2], np.int32)
    cent = np.arange(8, dtype=np.float32).reshape(2, 4)
    npz = CF.save_clusters(str(target / "clusters.npz"), paths, labels, core, degree, cent, medoid)
    with np.load(npz, allow_pickle=False) as z:
        assert sorted(z.files) == ["centroids", "core", "degree", "labels", "medoid", "paths"]
        assert z["paths"].tolist() == paths
        assert np.array_equal(z["labels"], labels) and z["labels"].dtype == np.int32
        assert np.array_equal(z["core"], core) and np.array_equal(z["degree"], degree)
        assert np.array_equal(z["centroids"], cent) and np.array_equal(z["medoid"], medoid)


def test_cluster_faces_arguments():
    from face_detection_and_recognition_amd.similar_face_filtering import cluster_faces as CF
    a = CF.get_parsed_args(["--ud", "u"])
    assert (a.tau, a.min_samples, a.net, a.preprocess, a.batch_size) == (0.5, 2, "mobile_facenet", "mobile_facenet", 32)
    a = CF.get_parsed_args(["--ud", "u", "--td", "t", "--net", "facenet", "--tau", "0.4", "--min_samples", "5", "-b", "8", "-d", "hip:0"])
    assert (a.target_data_path, a.preprocess, a.tau, a.min_samples, a.device) == ("t", "tf_standardize", 0.4, 5, "hip:0")
    assert a.savedmodel_path == "weights/facenet/facenet.pt"


def test_from_clusters_argument_errors():
    import torch
    from face_detection_and_recognition_amd.gallery import FaceGallery
    emb = torch.zeros((4, 8))
    with pytest.raises(ValueError):
        FaceGallery.from_clusters(emb, torch.tensor([0, 1, 0]))                 # one label short
    with pytest.raises(ValueError):
        FaceGallery.from_clusters(emb, torch.tensor([0., 1., 0., 1.]))          # not integers
    with pytest.raises(ValueError):
        FaceGallery.from_clusters(emb, torch.tensor([-1, -1, -1, -1]))          # nothing clustered
    with pytest.raises(ValueError):
        FaceGallery.from_clusters(torch.zeros((4,)), torch.tensor([0, 1, 0, 1]))


def test_python_argument_errors():
    import torch
    from face_detection_and_recognition_amd import clustering as K
    with pytest.raises(ValueError):
        K.dbscan_cosine(np.zeros((4, 8), np.float32), 0.5)
    with pytest.raises(ValueError):
        K.dbscan_cosine(torch.zeros((4, 8)), 0.5)                               # not on the device
    with pytest.raises(ValueError):
        K.dbscan_cosine(torch.zeros((4,)), 0.5)
    with pytest.raises(ValueError):
        K.cluster_summary(torch.zeros((4, 8)), torch.zeros((4,), dtype=torch.int32))
