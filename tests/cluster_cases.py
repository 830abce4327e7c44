"""Shared fixtures of the cosine-DBSCAN tests (test_cluster_cpu.py, test_cluster_gpu.py): synthetic identities, the threshold
choice, and the fp64 oracle.  A plain module; everything expensive is computed once per process."""
import functools

import numpy as np

GAP = 1e-5          # as tests/test_topk_gpu.py: an fp64 margin beyond which an fp32-equivalent decision is unambiguous
CASES = [(41, 130, 128, 8), (42, 700, 100, 24), (43, 1500, 512, 40), (44, 3000, 128, 60)]   # seed, N, D, identities
MIN_SAMPLES = (1, 2, 5, 12)


def faces(seed, N, D, ids):
    rng = np.random.default_rng(seed)
    C = rng.normal(0, 1, (ids, D)); C /= np.linalg.norm(C, axis=1, keepdims=True)
    for a in range(1, ids, 2):                      # every second identity is a look-alike of the one before it
        C[a] = C[a - 1] + 0.9 * C[a]; C[a] /= np.linalg.norm(C[a])
    sig = rng.uniform(0.7, 1.5, ids)                # tight and loose identities
    lab = rng.integers(0, ids, N)
    X = C[lab] + rng.normal(0, 1, (N, D)) * (sig[lab] / np.sqrt(D))[:, None]
    nz = rng.random(N) < 0.1                        # 10 % strangers
    X[nz] = rng.normal(0, 1, (int(nz.sum()), D))
    return X.astype(np.float32)


def cosine64(X):
    """fp64 cosine matrix of the fp32 rows; rows whose norm is zero or not finite give NaN."""
    X = np.asarray(X, np.float64)
    with np.errstate(all="ignore"):
        n = np.sqrt((X * X).sum(1))
        Xn = X / n[:, None]
        return Xn @ Xn.T


def choose_tau(S, lo=0.45, hi=0.55):
    """The midpoint of the widest gap between consecutive upper-triangle scores inside [lo, hi] -> (tau, gap)."""
    s = S[np.triu_indices(S.shape[0], 1)]
    s = np.sort(s[(s >= lo) & (s <= hi)])
    assert s.size >= 2, "the window holds fewer than two scores"
    d = np.diff(s)
    i = int(np.argmax(d))
    return float(0.5 * (s[i] + s[i + 1])), float(d[i])


def ambiguous(S, tau):
    """Pairs whose fp64 score lies within GAP of tau."""
    s = S[np.triu_indices(S.shape[0], 1)]
    return int((np.abs(s - tau) <= GAP).sum())


def edges(S, tau):
    """The boolean edge matrix: symmetric, empty diagonal, NaN compares false."""
    with np.errstate(invalid="ignore"):
        A = S >= tau
    A = A & A.T
    np.fill_diagonal(A, False)
    return A


def restate(A, min_samples, live=None):
    """The semantics of DESIGN §7 on an edge matrix -> (degree, core, labels)."""
    N = A.shape[0]
    live = np.ones(N, bool) if live is None else np.asarray(live, bool)
    degree = np.where(live, 1 + A.sum(1), 0).astype(np.int32)
    core = live & (degree >= min_samples)
    parent = np.arange(N)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    ii, jj = np.nonzero(np.triu(A & core[:, None] & core[None, :], 1))
    for i, j in zip(ii.tolist(), jj.tolist()):
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)               # the smaller root wins
    labels = np.full(N, -1, np.int32)
    roots = [find(i) if core[i] else -1 for i in range(N)]
    rank = {r: c for c, r in enumerate(sorted({r for r in roots if r >= 0}))}
    for i in range(N):
        if core[i]:
            labels[i] = rank[roots[i]]
    for i in np.nonzero(live & ~core)[0]:
        nb = np.nonzero(A[i] & core)[0]
        if nb.size:
            labels[i] = labels[nb].min()
    return degree, core, labels


@functools.lru_cache(maxsize=None)
def case(seed):
    """(X fp32, S fp64, tau, A) of the case with this seed."""
    _, N, D, ids = next(c for c in CASES if c[0] == seed)
    X = faces(seed, N, D, ids)
    S = cosine64(X)
    tau, _ = choose_tau(S)
    for a in (X, S):
        a.setflags(write=False)
    A = edges(S, tau)
    A.setflags(write=False)
    return X, S, tau, A


@functools.lru_cache(maxsize=None)
def oracle(seed, min_samples):
    degree, core, labels = restate(case(seed)[3], min_samples)
    for a in (degree, core, labels):
        a.setflags(write=False)
    return degree, core, labels
