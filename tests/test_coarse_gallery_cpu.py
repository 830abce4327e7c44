"""CPU tests of the compressed gallery: constants, refusals before any launch, the workspace size, the numpy restatement of
the row quantisation on hand-made rows, the .npz round trip between the two gallery classes and CompressedGallery's argument
checks.  Where a gallery is built here, the three device operators it calls are replaced by host restatements."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from face_detection_and_recognition_amd import _lib as L
from face_detection_and_recognition_amd import similarity as S

FP_ERR_ALIGNMENT = -5
P = ctypes.c_void_p(4096)     # a non-null, aligned pointer that is never dereferenced: every call here is refused first
ODD = ctypes.c_void_p(4100)


def test_coarse_constants_agree(lib):
    from conftest import ROOT
    hdr = open(os.path.join(ROOT, "include", "facepath.h")).read()
    assert int(re.search(r"#define FP_COARSE_MAX (\d+)", hdr).group(1)) == L.COARSE_MAX == 64
    assert int(re.search(r"#define FP_QUANT_MAX_D (\d+)", hdr).group(1)) == L.QUANT_MAX_D == 1024
    assert int(re.search(r"#define FP_ABI_VERSION (\d+)", hdr).group(1)) == 15      # additions only
    assert lib.fp_abi_version() == 15 == L.ABI_VERSION
    for name in ("fp_quant_i8_bytes", "fp_quantize_rows_i8", "fp_cosine_topk_i8_workspace", "fp_cosine_topk_i8", "fp_rerank_topk"):
        assert name in L.SIGNATURES and re.search(r"\b%s\(" % name, hdr), name
    assert 1024 * 127 * 127 < 2 ** 24                    # what FP_QUANT_MAX_D is for: the int32 dot converts to fp32 exactly


def test_quantize_refusals(lib):
    def call(X=P, N=5, D=128, q8=P, scale=P):
        return lib.fp_quantize_rows_i8(X, N, D, q8, scale, None)
    for name in ("X", "q8", "scale"):
        assert call(**{name: None}) == L.FP_ERR_INVALID_ARG, name
    assert call(N=0) == L.FP_ERR_INVALID_ARG and call(D=0) == L.FP_ERR_INVALID_ARG
    assert call(D=1088) == L.FP_ERR_INVALID_ARG          # > 1024
    assert call(D=100) == FP_ERR_ALIGNMENT and call(D=96) == FP_ERR_ALIGNMENT
    assert call(X=ODD) == FP_ERR_ALIGNMENT and call(q8=ODD) == FP_ERR_ALIGNMENT
    assert lib.fp_quant_i8_bytes(1, 64) == 128 * 64
    assert lib.fp_quant_i8_bytes(257, 512) == 384 * 512
    assert lib.fp_quant_i8_bytes(128, 1024) == 128 * 1024
    assert lib.fp_quant_i8_bytes(5, 100) == 0 and lib.fp_quant_i8_bytes(0, 64) == 0


def test_cosine_topk_i8_refusals_and_workspace(lib):
    def call(Q8=P, u=P, M=4, G8=P, w=P, N=100, D=128, pool=16, ns=0, scores=P, idx=P, ws=P, ws_bytes=1 << 30):
        return lib.fp_cosine_topk_i8(Q8, u, M, G8, w, N, D, pool, ns, scores, idx, ws, ws_bytes, None)
    for name in ("Q8", "u", "G8", "w", "scores", "idx", "ws"):
        assert call(**{name: None}) == L.FP_ERR_INVALID_ARG, name
    assert call(pool=0) == L.FP_ERR_INVALID_ARG and call(pool=65) == L.FP_ERR_INVALID_ARG
    assert call(N=0) == L.FP_ERR_INVALID_ARG and call(ns=-1) == L.FP_ERR_INVALID_ARG and call(M=-1) == L.FP_ERR_INVALID_ARG
    assert call(D=1088) == L.FP_ERR_INVALID_ARG
    assert call(D=100) == FP_ERR_ALIGNMENT and call(D=96) == FP_ERR_ALIGNMENT
    for name in ("Q8", "G8", "w"):
        assert call(**{name: ODD}) == FP_ERR_ALIGNMENT, name
    ws = lib.fp_cosine_topk_i8_workspace
    need = ws(4, 100, 16, 1)
    assert need == 4 * 1 * 16 * 8                        # M lists of pool keys
    assert ws(4, 1000, 64, 3) == 4 * 3 * 64 * 8 and ws(4, 100, 64, 3) == 4 * 1 * 64 * 8      # clamped to the chunks
    assert 0 < ws(4, 100, 16, 0) <= 128 * 16 * 8         # one row tile, one 128-column chunk
    assert 0 < ws(4, 100, 64, 0) <= 128 * 64 * 8
    assert ws(4, 100, 0, 1) == 0 and ws(4, 100, 65, 1) == 0 and ws(4, 0, 16, 1) == 0 and ws(0, 100, 16, 1) == 0
    for pool in (1, 16, 32, 33, 64):                     # grows with M across the row-tile sizes
        sizes = [ws(M, 100000, pool, 0) for M in (1, 64, 65, 128, 129, 5000, 125000)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0, (pool, sizes)
    assert call(ns=1, ws_bytes=need - 1) == L.FP_ERR_INVALID_ARG
    assert call(M=0, ws_bytes=0) == L.FP_OK              # nothing to do, nothing launched


def test_rerank_refusals(lib):
    def call(Q=P, qinv=P, M=4, D=128, cand=P, pool=16, G=P, rows=None, ginv=P, N=100, k=5, scores=P, idx=P):
        return lib.fp_rerank_topk(Q, qinv, M, D, cand, pool, G, rows, ginv, N, k, scores, idx, None)
    for name in ("Q", "qinv", "cand", "ginv", "scores", "idx"):
        assert call(**{name: None}) == L.FP_ERR_INVALID_ARG, name
    assert call(G=None, rows=None) == L.FP_ERR_INVALID_ARG       # one of the two addressing modes
    assert call(G=P, rows=P) == L.FP_ERR_INVALID_ARG             # ... and only one
    assert call(pool=0) == L.FP_ERR_INVALID_ARG and call(pool=65) == L.FP_ERR_INVALID_ARG
    assert call(k=0) == L.FP_ERR_INVALID_ARG and call(k=17, pool=32) == L.FP_ERR_INVALID_ARG
    assert call(k=6, pool=5) == L.FP_ERR_INVALID_ARG             # k > pool
    assert call(N=0) == L.FP_ERR_INVALID_ARG and call(M=-1) == L.FP_ERR_INVALID_ARG and call(D=1088) == L.FP_ERR_INVALID_ARG
    assert call(D=100) == FP_ERR_ALIGNMENT
    assert call(Q=ODD) == FP_ERR_ALIGNMENT and call(G=ODD) == FP_ERR_ALIGNMENT
    assert call(G=None, rows=ODD) == FP_ERR_ALIGNMENT
    assert call(M=0) == L.FP_OK and call(M=0, G=None, rows=P) == L.FP_OK


def test_quantize_rows_numpy_hand_made():
    D = 64
    X = np.zeros((6, D), np.float32)
    X[0] = 0.37 * np.where(np.arange(D) % 3 == 0, -1, 1)          # every entry +-amax -> all +-127
    # row 1 stays zero: dead
    X[2] = 1.0
    X[2, 5] = np.nan                                               # a NaN: dead
    X[3] = 1.0
    X[3, 7] = np.inf                                               # an inf: dead
    # amax = 127 makes r = 1: the entries ARE the levels; .5 values lie exactly halfway between two of them
    X[4, :8] = [127, 0.5, 1.5, 2.5, -0.5, -1.5, 63.5, -126.5]
    X[5, :4] = [-3.0, 1.0, 2.999, 0.0118]                          # negative amax entry; 0.0118 * 42.33 = 0.4995 -> 0
    q, scale = S.quantize_rows_i8_numpy(X)
    assert q.dtype == np.int8 and scale.dtype == np.float32 and q.shape == (6, D)
    assert np.array_equal(q[0], np.where(np.arange(D) % 3 == 0, -127, 127))
    assert scale[0] == np.float32(0.37) / np.float32(127)
    for dead in (1, 2, 3):
        assert not q[dead].any() and scale[dead] == 0
    assert q[4, :8].tolist() == [127, 0, 2, 2, 0, -2, 64, -126] and scale[4] == 1.0      # halves go to the even level
    assert q[5, :4].tolist() == [-127, 42, 127, 0] and scale[5] == np.float32(3) / np.float32(127)
    # features are zero-padded to a multiple of 64
    q100, s100 = S.quantize_rows_i8_numpy(np.ones((2, 100), np.float32))
    assert q100.shape == (2, 128) and np.all(q100[:, :100] == 127) and not q100[:, 100:].any()


def test_cosine_topk_i8_numpy_rules():
    qg = np.zeros((6, 64), np.int8)
    qg[:, 0] = [3, 5, 5, 5, 9, -2]
    qq = np.zeros((2, 64), np.int8)
    qq[:, 0] = [2, 1]
    w = np.array([1, 1, 1, 1, 0, 1], np.float32)                   # row 4, the best, is masked
    s, i = S.cosine_topk_i8_numpy(qq, np.array([0.5, 0.0], np.float32), qg, w, 8)
    assert i[0].tolist() == [1, 2, 3, 0, 5, -1, -1, -1]            # ties: the lower index first; tail beyond the live rows
    assert s[0, :5].tolist() == [5.0, 5.0, 5.0, 3.0, -2.0] and np.all(np.isneginf(s[0, 5:]))
    assert np.all(i[1] == -1) and np.all(np.isneginf(s[1]))        # u == 0: a dead query


def _host_operators(monkeypatch):
    """The device operators a gallery's constructor calls, restated on the host (CPU tensors in, CPU tensors out)."""
    monkeypatch.setattr(S, "row_inv_norm", lambda x: 1.0 / x.float().pow(2).sum(1).sqrt())
    monkeypatch.setattr(S, "split3_rows", lambda x: torch.zeros(1, dtype=torch.uint8))

    def quant(x):
        q, s = S.quantize_rows_i8_numpy(x.numpy())
        return S.stage_rows_i8(torch.from_numpy(q)), torch.from_numpy(s)
    monkeypatch.setattr(S, "quantize_rows_i8", quant)


def test_npz_round_trip_between_gallery_classes(monkeypatch, tmp_path):
    from face_detection_and_recognition_amd.gallery import CompressedGallery, FaceGallery
    _host_operators(monkeypatch)
    rng = np.random.default_rng(3)
    emb = rng.normal(0, 1, (9, 100)).astype(np.float32)
    emb[4] = 0                                                     # a dead row
    labels = np.arange(9, dtype=np.int32) % 4
    names = {0: "ann", 1: "bob", 3: "dee"}
    removed = np.zeros(9, bool)
    removed[[2, 4, 7]] = True                                      # removed rows, and the dead one
    a = FaceGallery(emb, labels, names, device="cpu")
    a.remove(torch.tensor([False, False, True, False, False, False, False, True, False]))
    for rows in ("device", "host"):
        if rows == "host":
            monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: self)
        pa = a.save(str(tmp_path / f"a_{rows}.npz"))
        b = CompressedGallery.load(pa, device="cpu", rows=rows)    # FaceGallery's file into the compressed class
        assert len(b) == 9 and b.dim == 100 and b.names == names and b.rows_where == rows
        assert np.array_equal(b.embeddings.numpy(), emb) and np.array_equal(b.labels.numpy(), labels)
        assert np.array_equal((b.ginv == 0).numpy(), removed) and np.array_equal((b.w == 0).numpy(), removed)
        assert b.g8.shape == (2, 128, 64) and b.g8.dtype == torch.int8
        pb = b.save(str(tmp_path / f"b_{rows}.npz"))
        with np.load(pa) as za, np.load(pb) as zb:                 # the same fields, the same content
            assert sorted(za.files) == sorted(zb.files) == ["embeddings", "labels", "name_ids", "name_strs", "removed"]
            for f in za.files:
                assert np.array_equal(za[f], zb[f]), f
        c = FaceGallery.load(pb, device="cpu")                     # ... and back
        assert np.array_equal(c.embeddings.numpy(), emb) and np.array_equal((c.ginv == 0).numpy(), removed) and c.names == names
    d = a.compress(rows=None)
    assert np.array_equal((d.w == 0).numpy(), removed) and d.rows is None
    assert d.device_bytes() <= 128 * (128 + 12) + 9 * 4            # codes + w, ginv, scale per (padded) row, + labels


def test_compressed_gallery_argument_checks(monkeypatch, tmp_path):
    from face_detection_and_recognition_amd.gallery import CompressedGallery
    _host_operators(monkeypatch)
    emb = np.eye(5, 70, dtype=np.float32)
    lab = np.arange(5, dtype=np.int32)
    with pytest.raises(ValueError, match="rows must be"):
        CompressedGallery(emb, lab, device="cpu", rows="disk")
    with pytest.raises(ValueError, match="N > 0"):
        CompressedGallery(np.zeros((0, 64), np.float32), np.zeros((0,), np.int32), device="cpu")
    with pytest.raises(ValueError, match="labels for"):
        CompressedGallery(emb, lab[:4], device="cpu")
    with pytest.raises(ValueError, match="at most 1024"):
        CompressedGallery(np.zeros((2, 1025), np.float32), lab[:2], device="cpu")
    g = CompressedGallery(emb, lab, {1: "one"}, device="cpu")
    assert len(g) == 5 and g.dim == 70 and g.name_of(1) == "one" and g.name_of(-1) == "unknown" and g.name_of(3) == "3"
    Q = torch.zeros((2, 70))
    for k, pool in ((0, None), (17, None), (5, 4), (5, 65), (1, 0)):
        with pytest.raises(ValueError, match="must be"):
            g.search(Q, k, pool)
    with pytest.raises(ValueError, match="features"):
        g.search(torch.zeros((2, 64)), 1)
    with pytest.raises(ValueError, match="mask of"):
        g.remove(np.zeros(4, bool))
    coarse_only = CompressedGallery(emb, lab, device="cpu", rows=None)
    with pytest.raises(ValueError, match="no fp32 rows"):
        coarse_only.save(str(tmp_path / "x.npz"))
    with pytest.raises(ValueError, match="no fp32 rows"):
        coarse_only.add(emb, lab)
    with pytest.raises(ValueError, match="labels for"):
        g.add(emb[:2], lab[:3])


def test_identify_driver_flags():
    from face_detection_and_recognition_amd.similar_face_filtering.identify_faces_using_reference import get_parsed_args
    base = ["--ud", "u", "--rd", "r"]
    a = get_parsed_args(base)
    assert a.coarse is None and a.pool is None and a.rows == "device"           # off by default
    b = get_parsed_args(base + ["--coarse", "int8", "--pool", "32", "--rows", "host"])
    assert b.coarse == "int8" and b.pool == 32 and b.rows == "host"
    with pytest.raises(SystemExit):
        get_parsed_args(base + ["--pool", "32"])
