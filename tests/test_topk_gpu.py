"""Top-k cosine search (fp_cosine_topk_x6) against an fp64 oracle, its tie rule and masking, and fp_topk_vote.

The oracle lives here: rows normalised in fp64, S64 = Q^ G^T, stable descending sort (lower index first on equal scores)."""
import numpy as np
import pytest
import torch

SHAPES = [(1, 1, 512, 1), (3, 5, 128, 16), (130, 257, 512, 5), (1000, 77, 128, 16), (257, 3000, 100, 8), (512, 4096, 512, 16)]
SCORE_TOL = 1e-4      # the project's score tolerance
GAP = 1e-5            # an fp64 gap above which the order of two candidates is unambiguous in fp32-equivalent arithmetic

_cache = {}


def _inputs():
    """Q then G of every shape, in order, from ONE generator; the fp64 scores and their stable descending order."""
    if not _cache:
        rng = np.random.default_rng(31)
        for shape in SHAPES:
            M, N, D, k = shape
            Q = rng.normal(0, 1, (M, D)).astype(np.float32)
            G = rng.normal(0, 1, (N, D)).astype(np.float32)
            q64, g64 = Q.astype(np.float64), G.astype(np.float64)
            S64 = (q64 / np.linalg.norm(q64, axis=1, keepdims=True)) @ (g64 / np.linalg.norm(g64, axis=1, keepdims=True)).T
            order = np.argsort(-S64, axis=1, kind="stable")
            _cache[shape] = (Q, G, S64, order)
    return _cache


def _run(dev, Q, G, k, n_splits, **kw):
    from face_detection_and_recognition_amd import similarity as S
    s, i = S.cosine_topk(torch.from_numpy(Q).to(dev), torch.from_numpy(G).to(dev), k, n_splits=n_splits, **kw)
    torch.cuda.synchronize()
    return s.cpu().numpy(), i.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_topk_against_fp64(dev, shape):
    M, N, D, k = shape
    Q, G, S64, order = _inputs()[shape]
    kv = min(k, N)                                       # valid slots
    sorted64 = np.take_along_axis(S64, order, axis=1)
    runs = {}
    for ns in (0, 3):
        sc, ix = _run(dev, Q, G, k, ns)
        runs[ns] = (sc, ix)
        assert sc.shape == (M, k) and ix.shape == (M, k) and sc.dtype == np.float32 and ix.dtype == np.int32
        # 6. slots beyond the valid gallery rows
        assert np.all(np.isneginf(sc[:, kv:])) and np.all(ix[:, kv:] == -1)
        sv, iv = sc[:, :kv], ix[:, :kv]
        # 3. indices in range and distinct within a row
        assert iv.min() >= 0 and iv.max() < N
        assert all(len(set(r)) == kv for r in iv.tolist())
        # 1. every score is the fp64 score at its index
        err = np.abs(sv.astype(np.float64) - np.take_along_axis(S64, iv.astype(np.int64), axis=1)).max()
        print(f"{shape} n_splits={ns}: max |score - S64[idx]| = {err:.3e}")
        assert err < SCORE_TOL
        # 2. non-increasing
        assert np.all(sv[:, 1:] <= sv[:, :-1])
        # 4. completeness, without assuming a tie order
        if N > kv:
            assert np.all(sv[:, kv - 1] >= sorted64[:, kv] - GAP)
        assert np.all(np.take_along_axis(S64, iv.astype(np.int64), axis=1) >= sorted64[:, kv - 1:kv] - GAP)
        # 5. exact positions where fp64 is unambiguous: gaps to both neighbours in the sorted row (the (k+1)-th included)
        head = sorted64[:, :min(kv + 1, N)]
        gaps = head[:, :-1] - head[:, 1:] if head.shape[1] > 1 else np.zeros((M, 0))
        big = gaps > GAP
        above = np.concatenate([np.ones((M, 1), bool), big], axis=1)[:, :kv]
        below = np.concatenate([big, np.ones((M, 1), bool)], axis=1)[:, :kv]      # (N <= k: the last one has no neighbour below)
        sure = above & below
        frac = sure.mean()
        print(f"{shape}: {100 * frac:.2f} % of positions sure")
        assert frac >= 0.98
        assert np.array_equal(iv[sure], order[:, :kv][sure].astype(np.int32))
    # 7. bit-identical: two runs on the same inputs, and n_splits 0 against 3
    sc2, ix2 = _run(dev, Q, G, k, 0)
    assert np.array_equal(sc2.view(np.uint32), runs[0][0].view(np.uint32)) and np.array_equal(ix2, runs[0][1])
    assert np.array_equal(runs[3][0].view(np.uint32), runs[0][0].view(np.uint32)) and np.array_equal(runs[3][1], runs[0][1])


def _tie_inputs():
    rng = np.random.default_rng(32)
    G = rng.normal(0, 1, (700, 128)).astype(np.float32)
    for r in (133, 300, 699):        # duplicates of row 5 in other 128-column chunks and, with n_splits = 3, in other splits
        G[r] = G[5]
    Q = np.concatenate([G[[5]], rng.normal(0, 1, (6, 128)).astype(np.float32)])
    return Q, G


@pytest.mark.gpu
@pytest.mark.parametrize("n_splits", [0, 1, 3, 6])
def test_topk_tie_rule_lower_index_first(dev, n_splits):
    Q, G = _tie_inputs()
    sc, ix = _run(dev, Q, G, 8, n_splits)
    assert ix[0, :4].tolist() == [5, 133, 300, 699]
    assert len(set(sc[0, :4].view(np.uint32).tolist())) == 1 and abs(float(sc[0, 0]) - 1.0) < 1e-6
    assert sc[0, 4] < sc[0, 3]


@pytest.mark.gpu
@pytest.mark.parametrize("n_splits", [0, 1, 3, 6])
def test_topk_masking(dev, n_splits):
    from face_detection_and_recognition_amd import similarity as S
    Q, G = _tie_inputs()
    full_s, full_i = _run(dev, Q, G, 8, n_splits)
    ginv = S.row_inv_norm(torch.from_numpy(G).to(dev))
    ginv[133] = 0
    ginv[699] = 0
    sc, ix = _run(dev, Q, G, 8, n_splits, ginv=ginv)
    assert ix[0, :2].tolist() == [5, 300]
    assert not np.isin(ix, [133, 699]).any()
    # every row: the unmasked result with the masked rows taken out, then the next candidates
    for m in range(Q.shape[0]):
        kept = [i for i in full_i[m].tolist() if i not in (133, 699)]
        assert ix[m, :len(kept)].tolist() == kept
    sc0, ix0 = _run(dev, Q, G, 8, n_splits, ginv=torch.zeros_like(ginv))
    assert np.all(np.isneginf(sc0)) and np.all(ix0 == -1)


def _vote_ref(scores, idx, labels, tau, mode):
    """The vote rules restated: (label, score, votes) of one row."""
    cand = [(s, labels[i]) for s, i in zip(scores, idx) if i >= 0 and s >= tau]
    if mode == 0:
        return (labels[idx[0]], scores[0], 1) if idx[0] >= 0 and scores[0] >= tau else (-1, scores[0], 0)
    if not cand:
        return -1, scores[0], 0
    tally = {}
    for s, lab in cand:
        v, sm, best = tally.get(lab, (0, np.float32(0), -np.inf))
        tally[lab] = (v + 1, np.float32(sm + np.float32(s)), max(best, s))
    lab = min(tally, key=lambda l: (-tally[l][0], -tally[l][1], l))
    return lab, tally[lab][2], tally[lab][0]


@pytest.mark.gpu
def test_topk_vote(dev):
    from face_detection_and_recognition_amd import similarity as S
    ninf = -np.inf
    labels = np.array([0, 0, 1, 1, 2, 2, 7, 3], np.int32)          # gallery row -> identity
    rows = [
        # (scores, idx)                                             what the row covers
        ([0.9, 0.5, 0.4, 0.2], [2, 0, 1, 4]),                      # top-1 above tau; majority: label 0 has two votes, label 1 the best score
        ([0.25, 0.2, 0.1, 0.0], [4, 0, 1, 2]),                     # everything below tau
        ([0.8, 0.7, 0.6, 0.5], [4, 5, 0, 6]),                      # a clear majority (label 2)
        ([0.9, 0.5, 0.7, 0.6], [0, 1, 2, 3]),                      # vote tie 2 : 2, decided by the summed score (0: 1.4, 1: 1.3)
        ([0.5, 0.5, 0.5, 0.5], [6, 7, 2, 4]),                      # a full tie (one vote each, equal sums): the smaller label id (1)
        ([0.6, 0.35, ninf, ninf], [7, 6, -1, -1]),                 # -1 slots
        ([ninf, ninf, ninf, ninf], [-1, -1, -1, -1]),              # nothing at all
        ([0.875, 0.75, 0.5, 0.375], [2, 4, 5, 3]),                 # votes 2 : 2, sums equal (1: 0.875 + 0.375, 2: 0.75 + 0.5) -> label 1
    ]
    rows[3] = (sorted(rows[3][0], reverse=True), [0, 2, 3, 1])     # (descending, as the search returns them)
    sc = np.array([r[0] for r in rows], np.float32)
    ix = np.array([r[1] for r in rows], np.int32)
    tau = 0.3
    for mode, vote in ((0, "top1"), (1, "majority")):
        lab, score, votes = S.topk_vote(torch.from_numpy(sc).to(dev), torch.from_numpy(ix).to(dev),
                                        torch.from_numpy(labels).to(dev), tau, vote)
        torch.cuda.synchronize()
        want = [_vote_ref(sc[m], ix[m], labels, np.float32(tau), mode) for m in range(len(rows))]
        assert lab.cpu().tolist() == [int(w[0]) for w in want], vote
        assert votes.cpu().tolist() == [int(w[2]) for w in want], vote
        assert np.array_equal(score.cpu().numpy(), np.array([w[1] for w in want], np.float32)), vote
    # the hand-worked answers, so that the restatement above cannot be wrong in the same way as the kernel
    lab1 = S.topk_vote(torch.from_numpy(sc).to(dev), torch.from_numpy(ix).to(dev), torch.from_numpy(labels).to(dev), tau, "top1")[0]
    labm, scm, vm = S.topk_vote(torch.from_numpy(sc).to(dev), torch.from_numpy(ix).to(dev), torch.from_numpy(labels).to(dev), tau,
                                "majority")
    assert lab1.cpu().tolist() == [1, -1, 2, 0, 7, 3, -1, 1]
    assert labm.cpu().tolist() == [0, -1, 2, 0, 1, 3, -1, 1]
    assert vm.cpu().tolist() == [2, 0, 2, 2, 1, 1, 0, 2]
    assert scm.cpu().tolist()[0] == 0.5 and scm.cpu().tolist()[1] == 0.25
    with pytest.raises(ValueError):
        S.topk_vote(torch.from_numpy(sc).to(dev), torch.from_numpy(ix).to(dev), torch.from_numpy(labels).to(dev), tau, "nope")
