"""Shared fixtures of the embedder-evaluation tests (test_verification_cpu.py, test_verification_gpu.py): labelled synthetic
identities, the fp64 oracle of the pair histogram, and the sandwich a device histogram has to sit in.  A plain module;
everything expensive is computed once per process.

Why GAP bounds the device's disagreement with fp64: the split-MFMA cosine is fp32-equivalent (about 1e-6 on unit rows, the
margin tests/test_topk_gpu.py and cluster_cases.py use), and the bin index adds two fp32 roundings of (s - lo) * scale,
|s - lo| <= 2: at most 2 * 2^-24 * 2 = 2.4e-7 in score units, plus the fp32 rounding of lo and scale, 2^-24 relative each.
Together below 2e-6, a fifth of GAP.  A pair whose fp64 score is farther than GAP from every edge has one possible bin."""
import functools

import numpy as np

GAP = 1e-5          # the project's margin (cluster_cases.GAP, tests/test_topk_gpu.py)
CASES = [(42, 700, 100, 24), (43, 1500, 512, 40), (44, 3000, 128, 60)]   # seed, N, D, identities: the sandwich cases
EXACT = (41, 130, 128, 8)


def labelled_faces(seed, N, D, ids):
    """The recipe of cluster_cases.faces, restated draw for draw (the rows are the same): look-alike identities, tight and
    loose sigma, 10 % strangers -> (X fp32, labels int64).  A row keeps the label of the identity it was drawn from; every
    second stranger gets label -1 (it takes part in no pair), the others an identity of their own (ids + row)."""
    rng = np.random.default_rng(seed)
    C = rng.normal(0, 1, (ids, D)); C /= np.linalg.norm(C, axis=1, keepdims=True)
    for a in range(1, ids, 2):                      # every second identity is a look-alike of the one before it
        C[a] = C[a - 1] + 0.9 * C[a]; C[a] /= np.linalg.norm(C[a])
    sig = rng.uniform(0.7, 1.5, ids)                # tight and loose identities
    lab = rng.integers(0, ids, N)
    X = C[lab] + rng.normal(0, 1, (N, D)) * (sig[lab] / np.sqrt(D))[:, None]
    nz = rng.random(N) < 0.1                        # 10 % strangers
    X[nz] = rng.normal(0, 1, (int(nz.sum()), D))
    labels = lab.astype(np.int64)
    rows = np.nonzero(nz)[0]
    labels[rows[0::2]] = -1
    labels[rows[1::2]] = ids + rows[1::2]
    return X.astype(np.float32), labels


def live_mask(X, labels):
    X = np.asarray(X, np.float64)
    with np.errstate(all="ignore"):
        n = np.sqrt((X * X).sum(1))
    return np.isfinite(n) & (n > 0) & (np.asarray(labels) >= 0)


def pair_scores(X, labels):
    """fp64 cosine of every pair i < j of live rows -> (genuine scores, impostor scores), each sorted ascending."""
    live = live_mask(X, labels)
    Xl = np.asarray(X, np.float64)[live]
    ll = np.asarray(labels)[live]
    Xn = Xl / np.sqrt((Xl * Xl).sum(1))[:, None] if len(Xl) else Xl
    iu = np.triu_indices(Xn.shape[0], 1)
    s = (Xn @ Xn.T)[iu] if len(Xl) else np.zeros(0)
    same = ll[iu[0]] == ll[iu[1]]
    return np.sort(s[same]), np.sort(s[~same])


def edges_of(lo, hi, nbins):
    return lo + (hi - lo) * np.arange(nbins + 1, dtype=np.float64) / nbins


def oracle_histogram(s, edges):
    """The fp64 histogram of sorted scores s with clamping end bins: bin b holds edges[b] <= s < edges[b + 1]."""
    nbins = len(edges) - 1
    cut = np.searchsorted(s, edges[1:-1], side="left")               # scores below each inner edge
    return np.diff(np.concatenate([[0], cut, [len(s)]])).astype(np.int64) if nbins > 1 else np.array([len(s)], np.int64)


def edge_margin(s, edges):
    """The smallest distance of any score to any INNER edge."""
    inner = edges[1:-1]
    if len(s) == 0 or len(inner) == 0:
        return np.inf
    j = np.clip(np.searchsorted(inner, s), 1, len(inner) - 1) if len(inner) > 1 else np.zeros(len(s), np.int64)
    near = np.minimum(np.abs(s - inner[j - 1]), np.abs(s - inner[j])) if len(inner) > 1 else np.abs(s - inner[0])
    return float(near.min())


def ambiguous_share(s, edges):
    """The share of scores within GAP of an inner edge."""
    inner = edges[1:-1]
    amb = np.searchsorted(s, inner + GAP, side="left") - np.searchsorted(s, inner - GAP, side="left")
    return float(amb.sum()) / max(len(s), 1)


def sandwich(dev_hist, s, edges):
    """What a device histogram of the sorted fp64 scores s has to satisfy; returns a list of violations (empty = passes).
      (a) the total is exact;
      (b) per inner edge e:  #(s >= e + GAP) <= sum(dev[b:]) <= #(s >= e - GAP);
      (c) per bin: certain members <= dev[b] <= certain members + the ambiguous scores at its two edges, where a score is
          ambiguous at e when e - GAP <= s < e + GAP and certain for bin b when edges[b] + GAP <= s < edges[b + 1] - GAP (the
          end bins are open: they also take everything below lo / from hi on)."""
    dev_hist = np.asarray(dev_hist, np.int64)
    nbins = len(edges) - 1
    inner = edges[1:-1]
    bad = []
    if int(dev_hist.sum()) != len(s):
        bad.append(f"total {int(dev_hist.sum())} != {len(s)}")
    below_lo = np.searchsorted(s, inner - GAP, side="left")          # scores < e - GAP
    below_hi = np.searchsorted(s, inner + GAP, side="left")          # scores < e + GAP
    cum = np.cumsum(dev_hist[::-1])[::-1][1:]                        # sum(dev[b:]) for b = 1 .. nbins - 1
    lower, upper = len(s) - below_hi, len(s) - below_lo
    for b in np.nonzero((cum < lower) | (cum > upper))[0][:5]:
        bad.append(f"edge {b + 1}: {lower[b]} <= {cum[b]} <= {upper[b]} fails")
    amb = below_hi - below_lo                                        # per inner edge
    start = np.concatenate([[0], below_hi])                          # first certain score of bin b
    stop = np.concatenate([below_lo, [len(s)]])                      # one past its last
    certain = np.maximum(stop - start, 0)
    slack = np.concatenate([[0], amb]) + np.concatenate([amb, [0]])
    for b in np.nonzero((dev_hist < certain) | (dev_hist > certain + slack))[0][:5]:
        bad.append(f"bin {b}: {certain[b]} <= {dev_hist[b]} <= {certain[b] + slack[b]} fails")
    assert len(certain) == nbins
    return bad


@functools.lru_cache(maxsize=None)
def case(seed):
    """(X fp32, labels, sorted fp64 genuine scores, sorted fp64 impostor scores) of the case with this seed; read-only."""
    _, N, D, ids = next(c for c in CASES + [EXACT] if c[0] == seed)
    X, labels = labelled_faces(seed, N, D, ids)
    g, i = pair_scores(X, labels)
    for a in (X, labels, g, i):
        a.setflags(write=False)
    return X, labels, g, i


@functools.lru_cache(maxsize=None)
def exact_range(nbins):
    """The lo of the scan lo = -0.8 - k 1e-4 (k < 2000), hi = lo + 1.6, whose nearest fp64 score of the EXACT case lies
    farthest from any inner edge -> (lo, hi, margin); lo and hi are fp32 values, what the device receives."""
    _, _, g, i = case(EXACT[0])
    s = np.concatenate([g, i])
    best = (None, None, -1.0)
    for k in range(2000):
        lo = float(np.float32(-0.8 - k * 1e-4))
        hi = float(np.float32(lo + 1.6))
        w = (hi - lo) / nbins
        u = (s - lo) / w
        r = np.clip(np.rint(u), 1, nbins - 1)
        m = float((np.abs(u - r) * w).min())
        if m > best[2]:
            best = (lo, hi, m)
    return best
