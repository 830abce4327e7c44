"""Case table, float64 references, bounds and mutants for the gallery search kernels (csrc/sim.hip, csrc/simi8.hip):

  fp_cosine_topk_x6       -> cosine_topk_x6_kernel<2> (128-row tiles, 128-column chunks, n_splits column ranges) + topk_merge_kernel
  fp_rerank_topk          -> rerank_topk_kernel (indexed mode: rows of G; compact mode: the gathered block `rows`)
  fp_topk_vote            -> topk_vote_kernel

tests/test_topk_ops.py runs every case.  The forms are those of tests/similarity_cases.py, whose _rng, _pow2, inv_norm32, TOL and
GUARD are used here.

* A Case names its entry point, its shape -- (M, N, D, k), rerank (M, N, D, pool, k), vote (M, N, k) -- what the data look like,
  and the n_splits values the search runs with.  The inverse norms handed to the kernels are the correctly rounded fp32 values
  of 1 / sqrt(sum of squares in float64): inputs, not results of fp_row_inv_norm.
* topk_reference(Q, G, qinv, ginv, k): float64 from the fp32 data alone.  S = (Q G^T) * qinv * ginv^T; a masked column
  (ginv == 0) and a NaN score (a zero row on either side: 0 * inf; a NaN in a query row) are no candidates; the others in a
  stable descending sort (equal scores: the lower index first); slots beyond the candidates hold -inf / -1.  The rerank is the
  same operation on the row's candidate SET: entries outside 0 .. N-1 are skipped and an index that the list names more than
  once counts once (include/facepath.h); every other column of the row is no candidate.
* The float32 yardstick in both summation orders (similarity_cases' docstring): torch's blocked product over the whole matrix,
  and the plain loop acc = acc + q[d] * g[d] at the returned columns.  bound = 2 * max|ref32 - ref64| + TOL over the k
  returned slots of every row, the larger of the two orders.
* exact slots.  A slot of the float64 ranking is exact -- the kernel must return the reference's index there -- when the float64
  gaps to both neighbours in the sorted row, the (k+1)-th candidate included, exceed 2 * bound ("sure"), or when it lies in a
  run of EQUAL float64 scores that any correct kernel gives equal bits too (copies of one gallery row; scores of exactly 0,
  whose every product has a zero factor) and the run's outer gaps are sure: inside the run the lower index goes first, and a
  run that k cuts returns its lowest indices ("planted").
* Data kinds of the search cases
    normal      rows N(0, 1); scaled: every row times its own power of two from 2^-20 .. 2^20
    ties        TIE_PAIRS: gallery row j0 copied to j0 + 1 (same 4-column group), + 4 (another q lane), + 16 (another
                accumulator), + 128 (the next chunk) and to column N - 2 (another split at every n_splits > 1), a query row
                equal to each; a query row equal to the LAST gallery row alone; k + 2 copies of a query row spread over the
                whole gallery (the k lowest must come back in order); k - 1 distinct better rows and three tied rows in the
                first, the middle and the last chunk (the lowest of the three gets the last slot)
    ascending   the gallery rows permuted so that query row 0's float64 scores rise with the column: every 4-column group
                takes the insertion path and every insert lands at the head
    descending  ... fall with the column: nothing inserts after the first k
    negative    query rows 0 mod 4 score below zero against EVERY column (gallery = minus the perturbed query direction);
                rows 1 mod 4 are zero on the first eight axes, where eight gallery columns are unit axes (score exactly +0,
                pairs of them 1, 4 and 16 columns apart) between three positive columns and the negative rest; row 1 and
                column 1 have norms of exactly 1
    masked_*    ginv == 0 on: scatter 20 % of the columns | chunk 1 | split every chunk behind the first half (whole splits at
                n_splits 2 and 4) | few all but k - 1 columns | all everything.  In each of them gallery row N // 3 is zero and
                keeps its ginv = +inf, query row M // 2 is zero and query row M // 2 + 1 holds a NaN
* MUTANTS / mutant(): float32 evaluations of wrong kernels with the cases that must catch them.

Printed by tests/test_topk_ops.py::test_reference_is_sure_and_the_bound_is_tight: the bound (torch's blocked product differs a
little between hosts) and the share of the slots outside planted ties that are not sure; 0 % where nothing is said:
    x6_1x1x32x1_normal 2.0e-07          x6_3x5x32x16_normal 3.4e-07         x6_3x5x32x16_negative 2.8e-07
    x6_64x127x32x5_normal 5.0e-07       x6_64x128x32x16_normal 4.8e-07      x6_64x129x64x16_normal 4.5e-07
    x6_33x130x32x2_normal 4.5e-07       x6_33x131x32x15_normal 5.8e-07      x6_130x257x96x5_normal 5.1e-07
    x6_130x257x96x5_ties 7.5e-07        ..._masked_scatter 4.9e-07          ..._masked_chunk 5.2e-07       ..._masked_all 2.0e-07
    x6_129x640x128x5_ties 8.9e-07       x6_129x640x128x16_normal 5.3e-07    ..._ascending 4.9e-07          ..._descending 4.9e-07
    x6_129x640x128x16_negative 8.3e-07, 0.28 %
    x6_257x1100x512x16_normal 7.4e-07, 0.22 %   ..._ties 1.5e-06, 0.32 %    ..._masked_scatter 5.1e-07, 0.10 %
    ..._masked_chunk 5.9e-07, 0.15 %    ..._masked_split 5.0e-07, 0.10 %    ..._masked_few 4.5e-07, 0.05 %   ..._masked_all 2.0e-07
    x6_257x1100x512x1_normal 5.9e-07    ..._ties 1.3e-06                    ..._masked_scatter 5.0e-07     ..._masked_chunk 5.6e-07
    ..._masked_split 5.3e-07            ..._masked_all 2.0e-07
    rr_37x500x64x24x5 4.3e-07           ..._scaled 3.9e-07                  ..._dup 6.1e-07                rr_5x300x1024x64x16 8.8e-07
    rr_130x257x128x1x1 3.3e-07          rr_9x40x64x16x16 4.7e-07
and by test_mutants_are_caught: two bf16 pieces move a slot by 2.2e-06 / 1.2e-06 (bounds 4.8e-07 / 5.3e-07), the inverse norm off by
4 ulp by 4.8e-07 (bound 2.8e-07); every other mutant moves a slot by at least 4.8e-04 or changes between 1 and 2473 exact indices.
"""
import functools
from dataclasses import dataclass

import numpy as np
import torch

from face_detection_and_recognition_amd.plan import split3_bf16
from similarity_cases import CHUNK, GUARD, TOL, _pow2, _rng, inv_norm32, planes  # noqa: F401  (GUARD, planes: for the test file)

X6, RERANK, VOTE = "fp_cosine_topk_x6", "fp_rerank_topk", "fp_topk_vote"
TOPK_MAX, COARSE_MAX = 16, 64
WS_GUARD = 4096                  # bytes of sentinels behind the workspace
MULTI = (0, 1, 2, 4, 9, 12)      # n_splits of the multi-chunk shapes; 0: the launcher's choice


@dataclass(frozen=True)
class Case:
    name: str
    entry: str               # X6 | RERANK | VOTE
    shape: tuple             # X6: (M, N, D, k); RERANK: (M, N, D, pool, k); VOTE: (M, N, k)
    kind: str = "normal"     # module docstring
    scaled: bool = False     # every row times its own power of two
    n_splits: tuple = (0,)   # X6: the n_splits values to run
    seed: str = ""           # the name that seeds the data (default: name)

    @property
    def key(self):
        return self.seed or self.name

    @property
    def k(self):
        return self.shape[-1]


def _ro(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ---------------------------------------------------------------------------------------------------------------------------
# the search: data
# ---------------------------------------------------------------------------------------------------------------------------
# (label, j0, j1 - j0): where the two members of a tie meet; None: column N - 2
TIE_PAIRS = (("the same four-column group", 8, 1), ("another q lane", 16, 4), ("another 16-column accumulator", 32, 16),
             ("the next chunk", 3, 128), ("another split", 40, None))
AXIS_COLS = (2, 3, 8, 9, 200, 204, 300, 316)     # negative: the unit-axis columns (those below N), one axis each
PLUS_COLS = (1, 260, 639)                                            # negative: the columns that score above zero against rows 1 mod 4


def _plant_ties(rng, Q, G, k):
    """The ties of the module docstring, written into Q and G -> [(query row, the leading indices it must return, label)]."""
    M, N = Q.shape[0], G.shape[0]
    nchunk = -(-N // CHUNK)
    plan, used = [], set()
    rows = iter([(i * 53 + 5) % M for i in range(16)])

    def take(cols):
        assert not used & set(cols) and all(0 <= j < N for j in cols) and len(set(cols)) == len(cols), (cols, N)
        used.update(cols)
        return list(cols)

    for label, j0, off in TIE_PAIRS:
        j0, j1 = take([j0, N - 2 if off is None else j0 + off])
        G[j1] = G[j0]
        m = next(rows)
        Q[m] = G[j0]
        plan.append((m, (j0, j1)[:k], label))
    last, = take([N - 1])
    m = next(rows)
    Q[m] = G[last]
    plan.append((m, (last,), "the last column alone"))
    step = (N - 4 - 60) // (k + 1)
    cols = take([60 + i * step for i in range(k + 2)])
    assert (cols[-1] // CHUNK - cols[0] // CHUNK >= 2) or nchunk < 4
    G[cols[1:]] = G[cols[0]]
    m = next(rows)
    Q[m] = G[cols[0]]
    plan.append((m, tuple(cols[:k]), "k + 2 copies: the k lowest"))
    better = take([65 + 2 * i for i in range(k - 1)])
    tied = take([101, (nchunk // 2) * CHUNK + 27, N - 3])
    m = next(rows)
    q = Q[m].copy()
    u = rng.standard_normal(q.shape[0], dtype=np.float32)          # one direction: the cosine falls with the step
    for i, j in enumerate(better):
        G[j] = q + np.float32(0.1 * (i + 1)) * u
    G[tied] = q + np.float32(0.1 * k) * u
    plan.append((m, tuple(better + tied[:1]), "k - 1 better rows, then the lowest of three tied"))
    assert len({p[0] for p in plan}) == len(plan)
    return plan


def _negative(rng, Q, G):
    """The negative kind (module docstring).  Axes 0 .. 7, S1 = 8 .. D / 2 - 1, S2 = D / 2 .. D - 1.  c lives on S1 and (positive)
    on the axes, base on S2; both hold four entries of +-1/2 there: a norm of exactly 1 for base."""
    M, D = Q.shape
    N = G.shape[0]
    h = D // 2
    c, base = np.zeros(D, np.float32), np.zeros(D, np.float32)
    c[8:12] = np.where(rng.integers(0, 2, 4) == 1, np.float32(0.5), np.float32(-0.5))
    c[:8] = 0.25
    base[h:h + 4] = np.where(rng.integers(0, 2, 4) == 1, np.float32(0.5), np.float32(-0.5))
    noise = lambda lo, hi: np.concatenate([np.zeros(lo, np.float32), rng.standard_normal(hi - lo, dtype=np.float32),  # noqa: E731
                                           np.zeros(D - hi, np.float32)]) / np.float32(np.sqrt(hi - lo))
    for n in range(N):
        G[n] = -(c + base + np.float32(0.3) * noise(8, D))
    for i, n in enumerate(AXIS_COLS):
        if n < N:
            G[n] = 0.0
            G[n, i] = -1.0
    for i, n in enumerate(PLUS_COLS):
        if n < N:
            G[n] = base - np.float32(0.1 * (i + 1)) * c
    for m in range(M):
        if m % 4 == 0:          # below zero against every column: c-like on S1, positive on the axes
            Q[m] = c + np.float32(0.2) * noise(8, h)
            Q[m, :8] = 0.25 + np.abs(rng.standard_normal(8, dtype=np.float32))
        elif m % 4 == 1:        # base-like on S2, zero elsewhere
            Q[m] = base + (np.float32(0.2) * noise(h, D) if m > 1 else 0)


@functools.lru_cache(maxsize=None)
def x6_inputs(c):
    """{"Q": (M, D), "G": (N, D), "qinv": (M,), "ginv": (N,)} float32, read-only; "plan": _plant_ties() of a ties case."""
    M, N, D, k = c.shape
    rng = _rng(c.key)
    Q = rng.standard_normal((M, D), dtype=np.float32)
    G = rng.standard_normal((N, D), dtype=np.float32)
    d = {"plan": []}
    if c.kind == "negative":
        _negative(rng, Q, G)
    if c.scaled:
        Q *= _pow2(rng, M)
        G *= _pow2(rng, N)
    if c.kind == "ties":
        d["plan"] = _plant_ties(rng, Q, G, k)
    if c.kind in ("ascending", "descending"):
        g64 = G.astype(np.float64)
        s = (g64 @ Q[0].astype(np.float64)) / np.sqrt((g64 * g64).sum(1))
        order = np.argsort(s, kind="stable")
        G = np.ascontiguousarray(G[order if c.kind == "ascending" else order[::-1]])
    masked = c.kind.startswith("masked")
    if masked:
        assert M >= 3 and N >= 3
        G[N // 3] = 0.0
        Q[M // 2] = 0.0
        Q[M // 2 + 1, D // 2] = np.nan
    qinv, ginv = inv_norm32(Q), inv_norm32(G)
    if masked:
        nchunk = -(-N // CHUNK)
        what = c.kind.split("_")[1]
        if what == "scatter":
            ginv[rng.random(N) < 0.2] = 0.0
        elif what == "chunk":
            ginv[CHUNK:2 * CHUNK] = 0.0
        elif what == "split":
            ginv[(nchunk - nchunk // 2) * CHUNK:] = 0.0
        elif what == "few":
            live = [5 + i * ((N - 10) // max(k - 1, 1)) for i in range(k - 1)]
            live = [j + 1 if j == N // 3 else j for j in live]
            keep = ginv[live].copy()
            ginv[:] = 0.0
            ginv[live] = keep
        else:
            assert what == "all"
            ginv[:] = 0.0
        ginv[N // 3] = np.inf
    d.update(Q=Q, G=G, qinv=qinv, ginv=ginv)
    return _ro(d)


# ---------------------------------------------------------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------------------------------------------------------
def score_matrix(Q, G, qinv, ginv, dt):
    """S = ((Q G^T) * qinv) * ginv^T in dtype dt (torch: the float32 product is blocked), as numpy; NaN where it is NaN."""
    with torch.no_grad(), np.errstate(all="ignore"):
        t = lambda x: torch.tensor(np.asarray(x), dtype=dt)  # noqa: E731
        return ((t(Q) @ t(G).T) * t(qinv)[:, None] * t(ginv)[None, :]).numpy()


def plain32(Q, G, qinv, ginv):
    """The same in float32 with every dot product a plain sum over D on its own: identical rows give identical bits."""
    M, N = Q.shape[0], G.shape[0]
    S = np.empty((M, N), np.float32)
    rows = max(1, (32 << 20) // max(N * Q.shape[1] * 4, 1))
    with np.errstate(all="ignore"):
        for lo in range(0, M, rows):
            S[lo:lo + rows] = (Q[lo:lo + rows, None, :] * G[None]).sum(-1, dtype=np.float32)
        return S * qinv[:, None] * ginv[None, :]


def seq32(Q, G, qinv, ginv, rows, cols):
    """float32 scores at (rows[i], cols[i]) with the sum over D taken in sequence, both roundings in fp32 (NaN for cols[i] < 0)."""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    q, g = Q[rows], G[np.maximum(cols, 0)]
    acc = np.zeros(len(rows), np.float32)
    with np.errstate(all="ignore"):
        for d in range(Q.shape[1]):
            acc = acc + q[:, d] * g[:, d]
        s = acc * qinv[rows] * ginv[np.maximum(cols, 0)]
    return np.where(cols < 0, np.float32("nan"), s).astype(np.float32)


def rank(S, live, k, arrival=None):
    """The candidates (live & not NaN) of every row of S in a stable descending sort -> dict(order (M, N) columns, best first;
    sorted (M, N) their scores, -inf behind the candidates; nvalid (M,); sc (M, k), idx (M, k) with -inf / -1).  arrival: a
    permutation of the columns -- equal scores in that order instead of by index."""
    M, N = S.shape
    ok = live & ~np.isnan(S)
    key = np.where(ok, S, -np.inf)
    if arrival is not None:
        order = np.asarray(arrival)[np.argsort(-key[:, arrival], axis=1, kind="stable")]
    else:
        order = np.argsort(-key, axis=1, kind="stable")
    srt = np.take_along_axis(key, order, axis=1)
    nvalid = ok.sum(axis=1)
    sc = np.full((M, k), -np.inf, S.dtype)
    idx = np.full((M, k), -1, np.int32)
    n = min(k, N)
    sc[:, :n], idx[:, :n] = srt[:, :n], order[:, :n]
    idx[np.isneginf(sc)] = -1
    return dict(order=order, sorted=srt, nvalid=nvalid, sc=sc, idx=idx, ok=ok)


def topk_reference(Q, G, qinv, ginv, k, live=None):
    """(scores (M, k) float64, idx (M, k) int32, the rank() dict) of the search in float64 from the fp32 inputs; live (M, N):
    the columns a row may return besides the mask (the rerank's candidate sets)."""
    S = score_matrix(Q, G, qinv, ginv, torch.float64)
    mask = (np.asarray(ginv) != 0)[None, :]
    r = rank(S, mask if live is None else (mask & live), k)
    r["S"] = S
    return r["sc"], r["idx"], r


def _exact_slots(r, G, k, bound):
    """(exact (M, k), planted (M, k)) of a float64 ranking (module docstring)."""
    M = r["S"].shape[0]
    exact, planted = np.zeros((M, k), bool), np.zeros((M, k), bool)
    for m in range(M):
        nv = int(r["nvalid"][m])
        v, cols = r["sorted"][m, :nv], r["order"][m, :nv]
        s = 0
        while s < min(k, nv):
            a = b = s
            while b + 1 < nv and v[b + 1] == v[s]:
                b += 1
            run = cols[a:b + 1]
            same = b == a or v[s] == 0.0 or all(np.array_equal(G[j], G[run[0]]) for j in run[1:])
            clear = (a == 0 or v[a - 1] - v[a] > 2 * bound) and (b + 1 == nv or v[b] - v[b + 1] > 2 * bound)
            exact[m, a:min(b + 1, k)] = same and clear
            planted[m, a:min(b + 1, k)] = same and b > a
            s = b + 1
    return exact, planted


def _bound_and_slots(d, r, k):
    idx = r["idx"]
    M = idx.shape[0]
    valid = idx >= 0
    rows = np.repeat(np.arange(M), k).reshape(M, k)
    b32 = score_matrix(d["Q"], d["G"], d["qinv"], d["ginv"], torch.float32)
    blocked = np.take_along_axis(b32, np.maximum(idx, 0).astype(np.int64), axis=1)
    seq = seq32(d["Q"], d["G"], d["qinv"], d["ginv"], rows.ravel(), idx.ravel()).reshape(M, k)
    e = lambda a: float(np.abs(a[valid].astype(np.float64) - r["sc"][valid]).max()) if valid.any() else 0.0  # noqa: E731
    bound = 2.0 * max(e(blocked), e(seq)) + TOL
    exact, planted = _exact_slots(r, d["G"], k, bound)
    r.update(bound=bound, exact=exact, planted=planted, err_blocked=e(blocked), err_seq=e(seq))
    return _ro(r)


@functools.lru_cache(maxsize=None)
def x6_references(c):
    """The float64 ranking of a search case on its own inputs, with "bound", "exact" and "planted"; read-only, computed once."""
    d = x6_inputs(c)
    _, _, r = topk_reference(d["Q"], d["G"], d["qinv"], d["ginv"], c.k)
    return _bound_and_slots(d, r, c.k)


# ---------------------------------------------------------------------------------------------------------------------------
# the rerank: data and reference
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rerank_inputs(c):
    """{"Q", "G", "qinv", "ginv", "cand" (M, pool) int32, "rows" (M, pool, D): the compact block, NaN where cand names no row}.
    Every list: 10 % holes of -1, one index >= N where the pool allows; 10 % of the gallery masked; row 1 keeps k - 2 entries,
    row 2 none, query row 3 is zero; rows 0 and 4 equal a gallery row j0 whose copy j1 > j0 stands EARLIER in their lists.
    kind dup: row 0 names j0 twice more, row 4 names one index in every place."""
    M, N, D, pool, k = c.shape
    rng = _rng(c.key)
    Q = rng.standard_normal((M, D), dtype=np.float32)
    G = rng.standard_normal((N, D), dtype=np.float32)
    if c.scaled:
        Q *= _pow2(rng, M)
        G *= _pow2(rng, N)
    cand = np.stack([rng.permutation(N)[:pool] for _ in range(M)]).astype(np.int32)
    cand[rng.random((M, pool)) < 0.1] = -1
    masked = rng.random(N) < 0.1
    if pool >= 4:
        cand[:, pool - 1] = N + np.arange(M) % 7
        cand[0, pool - 1] = np.iinfo(np.int32).max
    if M >= 5:
        cand[1, max(k - 2, 0):] = -1
        cand[2] = -1
        Q[3] = 0.0
        if pool >= 4:
            for m, (j0, j1) in ((0, (7, 19)), (4, (11, 12))):
                G[j1] = G[j0]
                masked[[j0, j1]] = False
                Q[m] = G[j0]
                cand[m][np.isin(cand[m], (j0, j1))] = -1
                cand[m, 0], cand[m, 2] = j1, j0
            if c.kind == "dup":
                cand[0, 1], cand[0, 3] = 7, 7
                cand[4] = 11
    qinv, ginv = inv_norm32(Q), inv_norm32(G)
    ginv[masked] = 0.0
    inside = (cand >= 0) & (cand < N)
    rows = np.where(inside[:, :, None], G[np.where(inside, cand, 0)], np.float32("nan")).astype(np.float32)
    live = np.zeros((M, N), bool)
    mm, jj = np.nonzero(inside)
    live[mm, cand[mm, jj]] = True
    return _ro(dict(Q=Q, G=G, qinv=qinv, ginv=ginv, cand=cand, rows=rows, live=live))


@functools.lru_cache(maxsize=None)
def rerank_references(c):
    d = rerank_inputs(c)
    _, _, r = topk_reference(d["Q"], d["G"], d["qinv"], d["ginv"], c.k, d["live"])
    return _bound_and_slots(d, r, c.k)


# ---------------------------------------------------------------------------------------------------------------------------
# the vote: data and reference
# ---------------------------------------------------------------------------------------------------------------------------
VOTE_GRID = (np.arange(32) / 32.0).astype(np.float32)
VOTE_TAU = float(VOTE_GRID[12])


@functools.lru_cache(maxsize=None)
def vote_inputs(c):
    """{"scores" (M, k) fp32 descending from VOTE_GRID, "idx" (M, k) int32, "labels" (N,) int32}: rows of 0 .. k candidates with
    -inf / -1 behind them; 3 % of the indices are >= N; six label ids."""
    M, N, k = c.shape
    rng = _rng(c.key)
    sc = -np.sort(-VOTE_GRID[rng.integers(0, 32, (M, k))], axis=1)
    idx = rng.integers(0, N, (M, k)).astype(np.int32)
    big = rng.random((M, k)) < 0.03
    idx[big] = np.where(rng.random(big.sum()) < 0.5, N, np.iinfo(np.int32).max - 3)
    length = rng.integers(0, k + 1, M)
    length[rng.random(M) < 0.5] = k
    tail = np.arange(k)[None, :] >= length[:, None]
    sc[tail], idx[tail] = -np.inf, -1
    labels = np.array([0, 1, 2, 3, 7, 9], np.int32)[rng.integers(0, 6, N)]
    return _ro(dict(scores=sc, idx=idx, labels=labels))


def vote_reference(scores, idx, labels, tau, mode):
    """(label, score, votes) per row by the rule of similarity.topk_vote / include/facepath.h: a candidate counts when its index is
    in 0 .. N-1 and its score >= tau.  mode 0: the best candidate's label if it counts.  mode 1: the label with the most
    counting candidates, then the larger fp32 sum of their scores (added in slot order), then the smaller label.  score: the
    best among the winner's candidates, the row's first score when nobody wins."""
    M, k = scores.shape
    N = len(labels)
    tau = np.float32(tau)
    out = (np.full(M, -1, np.int32), scores[:, 0].copy(), np.zeros(M, np.int32))
    for m in range(M):
        counts = [j for j in range(1 if mode == 0 else k) if 0 <= idx[m, j] < N and scores[m, j] >= tau]
        tally = {}
        for j in counts:
            v, sm, best = tally.get(int(labels[idx[m, j]]), (0, np.float32(0), None))
            tally[int(labels[idx[m, j]])] = (v + 1, np.float32(sm + scores[m, j]), scores[m, j] if best is None else best)
        if tally:
            lab = min(tally, key=lambda x: (-tally[x][0], -tally[x][1], x))
            out[0][m], out[1][m], out[2][m] = lab, tally[lab][2], tally[lab][0]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# mutants: float32 evaluations of wrong kernels
# ---------------------------------------------------------------------------------------------------------------------------
def _cut2(x):
    """x cut to its first two bf16 pieces."""
    return (split3_bf16(x)[:2].astype(np.uint32) << 16).view(np.float32).astype(np.float64).sum(0).astype(np.float32)


def _ulps(v, n):
    for _ in range(n):
        v = np.nextafter(v, np.float32(np.inf), dtype=np.float32)
    return v


@functools.lru_cache(maxsize=None)
def reference32(c):
    """The float32 reference of a case with plain sums (identical rows: identical bits) -> (S32, live (M, N) | (1, N), rank())."""
    d = x6_inputs(c) if c.entry == X6 else rerank_inputs(c)
    S = plain32(d["Q"], d["G"], d["qinv"], d["ginv"])
    live = (d["ginv"] != 0)[None, :] & d.get("live", True)
    return S, live, rank(S, live, c.k)


def mutant(c, mut):
    """(scores (M, k) float32, idx (M, k)) of the mutated float32 reference of a search case."""
    d = x6_inputs(c)
    M, N, D, k = c.shape
    S, live, base = reference32(c)
    nchunk = -(-N // CHUNK)
    cols = np.arange(N)
    arrival = None
    if mut == "hm":
        S = plain32(_cut2(d["Q"]), _cut2(d["G"]), d["qinv"], d["ginv"])
    elif mut == "kslab":
        S = plain32(d["Q"][:, :D - 32], d["G"][:, :D - 32], d["qinv"], d["ginv"])
    elif mut == "lastchunk":
        live = live & (cols < (nchunk - 1) * CHUNK)[None]
    elif mut == "remchunk":         # n_splits = 2: the first split takes nchunk // 2 + 1 chunks and forgets the one beyond its base
        assert nchunk % 2 == 1 and nchunk >= 3
        live = live & (cols // CHUNK != nchunk // 2)[None]
    elif mut == "ginvtail":
        assert N % 4
        live = live & (cols < N // 4 * 4)[None]
    elif mut == "inv4":             # the query row with the largest score
        m = int(np.argmax(base["sc"][:, 0]))
        S = S.copy()
        S[m] = plain32(d["Q"][m:m + 1], d["G"], _ulps(d["qinv"][m:m + 1], 4), d["ginv"])[0]
    elif mut == "tie_high":
        arrival = cols[::-1]
    elif mut == "gt":               # n_splits = 2, the later split first, and > against the k-th best: equal scores in arrival order
        first = (nchunk - nchunk // 2) * CHUNK
        arrival = np.concatenate([cols[first:], cols[:first]])
    elif mut == "masked":           # a masked column scores acc * qinv * 0 and is returned
        live = np.ones_like(live)
    if mut in ("swap", "dup"):
        sc, idx = base["sc"].copy(), base["idx"].copy()
        ex = x6_references(c)["exact"]
        m = int(np.flatnonzero(ex[:, 0] & ex[:, 1])[0])
        if mut == "swap":
            sc[m, :2], idx[m, :2] = sc[m, 1::-1].copy(), idx[m, 1::-1].copy()
        else:
            sc[m, 1], idx[m, 1] = sc[m, 0], idx[m, 0]
        return sc, idx
    r = rank(S, live, k, arrival)
    return r["sc"], r["idx"]


def mutant_shift(c, mut):
    """(the largest move of a slot's score against the float32 reference -- inf where a slot appears or disappears --, the number
    of exact slots whose index changes)."""
    _, _, base = reference32(c)
    sc, idx = mutant(c, mut)
    both = np.isfinite(sc) & np.isfinite(base["sc"])
    shift = np.inf if (np.isfinite(sc) != np.isfinite(base["sc"])).any() else \
        float(np.abs(sc[both].astype(np.float64) - base["sc"][both]).max()) if both.any() else 0.0
    ex = x6_references(c)["exact"]
    return shift, int((idx[ex] != base["idx"][ex]).sum())


# (label, mutation, names of the cases that must catch it)
MUTANTS = (
    ("operands cut to two bf16 pieces", "hm", ("x6_64x128x32x16_normal", "x6_129x640x128x16_normal")),
    ("the last k-slab dropped", "kslab", ("x6_130x257x96x5_normal", "x6_64x129x64x16_normal")),
    ("the last chunk dropped", "lastchunk", ("x6_64x129x64x16_normal", "x6_130x257x96x5_ties", "x6_257x1100x512x1_ties")),
    ("the remainder chunk of a split dropped", "remchunk", ("x6_257x1100x512x16_ties", "x6_129x640x128x16_normal")),
    ("the scalar ginv tail read as zeros", "ginvtail", ("x6_33x130x32x2_normal", "x6_33x131x32x15_normal", "x6_130x257x96x5_ties")),
    ("an inverse norm off by 4 ulp", "inv4", ("x6_3x5x32x16_negative",)),
    ("the higher index of a boundary tie", "tie_high", ("x6_257x1100x512x16_ties", "x6_257x1100x512x1_ties", "x6_129x640x128x5_ties")),
    ("> for >= against the k-th best across splits", "gt", ("x6_257x1100x512x16_ties", "x6_257x1100x512x1_ties")),
    ("two neighbouring slots swapped", "swap", ("x6_33x130x32x2_normal", "x6_129x640x128x16_descending")),
    ("a masked column returned", "masked", ("x6_257x1100x512x16_masked_few", "x6_257x1100x512x1_masked_all", "x6_130x257x96x5_masked_all")),
    ("a duplicate index in a row", "dup", ("x6_129x640x128x16_ascending", "x6_257x1100x512x16_masked_scatter")),
)


# ---------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------
_MASKS = ("masked_scatter", "masked_chunk", "masked_split", "masked_few", "masked_all")
# (M, N, D, k), kinds, scaled rows, n_splits
_X6_SHAPES = (
    ((1, 1, 32, 1), ("normal",), False, (0, 1)),                             # the smallest problem
    ((3, 5, 32, 16), ("normal", "negative"), False, (0, 1, 2)),              # N < k
    ((64, 127, 32, 5), ("normal",), False, (0, 1, 2)),                       # one ragged chunk
    ((64, 128, 32, 16), ("normal",), True, (0, 1, 2)),                       # one full chunk
    ((64, 129, 64, 16), ("normal",), False, (0, 1, 2, 4)),                   # the second chunk holds one column
    ((33, 130, 32, 2), ("normal",), False, (0, 1, 2)),                       # N % 4 = 2: the scalar ginv tail
    ((33, 131, 32, 15), ("normal",), True, (0, 1, 2)),                       # N % 4 = 3
    ((130, 257, 96, 5), ("normal", "ties", "masked_scatter", "masked_chunk", "masked_all"), True, MULTI),    # three k-slabs, N % 4 = 1, a ragged row tile, waves wholly past M
    ((129, 640, 128, 5), ("ties",), False, MULTI),                           # k = 5 with k + 2 copies over five chunks
    ((129, 640, 128, 16), ("normal", "ascending", "descending", "negative"), True, MULTI),      # 5 chunks
    ((257, 1100, 512, 16), ("normal", "ties") + _MASKS, True, MULTI),        # 9 chunks, three row tiles; the LDS above 64 KiB
    ((257, 1100, 512, 1), ("normal", "ties", "masked_scatter", "masked_chunk", "masked_split", "masked_all"), False, MULTI),
)
_RERANK = (((37, 500, 64, 24, 5), "normal", False), ((37, 500, 64, 24, 5), "normal", True), ((37, 500, 64, 24, 5), "dup", False),
           ((5, 300, 1024, 64, 16), "normal", False),                        # all four f32x4 of a lane
           ((130, 257, 128, 1, 1), "normal", False), ((9, 40, 64, 16, 16), "normal", False))


# seeds that were changed until a condition of the CPU tests held (never a bound or a cap): the default seed of (33, 130, 32, 2) puts
# neither of the two tail columns into a sure slot of its 66
_SEEDS = {"x6_33x130x32x2_normal": "x6_33x130x32x2_normal/3"}


def _cases():
    out = []
    for shape, kinds, scaled, ns in _X6_SHAPES:
        for kind in kinds:
            sc = scaled and kind in ("normal", "negative")
            name = "x6_" + "x".join(map(str, shape)) + "_" + kind
            out.append(Case(name, X6, shape, kind, scaled=sc, n_splits=ns, seed=_SEEDS.get(name, "")))
    for shape, kind, scaled in _RERANK:
        out.append(Case("rr_" + "x".join(map(str, shape)) + ("_dup" if kind == "dup" else "") + ("_scaled" if scaled else ""),
                        RERANK, shape, kind, scaled=scaled))
    out += [Case(f"vote_1000x50x{k}", VOTE, (1000, 50, k)) for k in (1, 5, 16)]
    assert len({c.name for c in out}) == len(out)
    return out


CASES = _cases()
X6_CASES = [c for c in CASES if c.entry == X6]
RERANK_CASES = [c for c in CASES if c.entry == RERANK]
VOTE_CASES = [c for c in CASES if c.entry == VOTE]
BY_NAME = {c.name: c for c in CASES}
