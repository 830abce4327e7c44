"""CPU tests of the top-k entry points' host side: argument refusals before any launch and the workspace size."""
import ctypes

from face_detection_and_recognition_amd import _lib as L

FP_ERR_ALIGNMENT = -5
P = ctypes.c_void_p(4096)     # a non-null, aligned pointer that is never dereferenced: every call here is refused first


def test_topk_constants_agree():
    import os
    import re
    from conftest import ROOT
    hdr = open(os.path.join(ROOT, "include", "facepath.h")).read()
    assert int(re.search(r"#define FP_TOPK_MAX (\d+)", hdr).group(1)) == L.TOPK_MAX == 16
    assert int(re.search(r"#define FP_ABI_VERSION (\d+)", hdr).group(1)) == 15


def test_cosine_topk_refusals(lib):
    def call(Q=P, qinv=P, M=4, G3=P, ginv=P, N=100, D=128, k=5, ns=0, scores=P, idx=P, ws=P, ws_bytes=1 << 30):
        return lib.fp_cosine_topk_x6(Q, qinv, M, G3, ginv, N, D, k, ns, scores, idx, ws, ws_bytes, None)
    for name in ("Q", "qinv", "G3", "ginv", "scores", "idx", "ws"):
        assert call(**{name: None}) == L.FP_ERR_INVALID_ARG, name
    assert call(k=0) == L.FP_ERR_INVALID_ARG
    assert call(k=17) == L.FP_ERR_INVALID_ARG
    assert call(N=0) == L.FP_ERR_INVALID_ARG
    assert call(ns=-1) == L.FP_ERR_INVALID_ARG
    assert call(M=-1) == L.FP_ERR_INVALID_ARG
    assert call(D=100) == FP_ERR_ALIGNMENT
    assert call(Q=ctypes.c_void_p(4100)) == FP_ERR_ALIGNMENT
    assert call(ginv=ctypes.c_void_p(4100)) == FP_ERR_ALIGNMENT
    need = lib.fp_cosine_topk_workspace(4, 100, 5, 1)
    assert need == 4 * 1 * 5 * 8
    assert 0 < lib.fp_cosine_topk_workspace(4, 100, 5, 0) <= 128 * 1 * 5 * 8      # one row tile, one 128-column chunk
    assert call(ns=1, ws_bytes=need - 1) == L.FP_ERR_INVALID_ARG
    assert call(M=0, ws_bytes=0) == L.FP_OK                 # nothing to do, nothing launched


def test_topk_vote_refusals(lib):
    def call(scores=P, idx=P, M=4, k=5, labels=P, N=10, mode=0, ol=P, os_=P, ov=P):
        return lib.fp_topk_vote(scores, idx, M, k, labels, N, 0.3, mode, ol, os_, ov, None)
    for name in ("scores", "idx", "labels", "ol", "os_", "ov"):
        assert call(**{name: None}) == L.FP_ERR_INVALID_ARG, name
    assert call(k=0) == L.FP_ERR_INVALID_ARG and call(k=17) == L.FP_ERR_INVALID_ARG
    assert call(mode=2) == L.FP_ERR_INVALID_ARG and call(N=0) == L.FP_ERR_INVALID_ARG
    assert call(M=0) == L.FP_OK


def test_topk_workspace_monotone(lib):
    ws = lib.fp_cosine_topk_workspace
    N = 100000
    for ns in (0, 1, 3, 64):
        for k in (1, 5, 16):
            sizes = [ws(M, N, k, ns) for M in (1, 100, 128, 129, 5000, 125000)]
            assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0, (ns, k, sizes)
        for M in (1, 1000):
            sizes = [ws(M, N, k, ns) for k in range(1, 17)]
            assert all(b >= a for a, b in zip(sizes, sizes[1:])), (ns, M, sizes)
    for M in (1, 1000):
        sizes = [ws(M, N, 5, ns) for ns in (1, 2, 3, 8, 100, 782, 5000)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:]))
        assert sizes[-1] == sizes[-2] == M * 782 * 5 * 8          # clamped to the number of 128-column chunks
    assert ws(4, 100, 0, 0) == 0 and ws(4, 100, 17, 0) == 0 and ws(4, 0, 5, 0) == 0
    # the automatic choice depends on M (and k), not on N, until the chunk count clamps it
    assert ws(512, 1000000, 5, 0) == ws(512, 2000000, 5, 0)
