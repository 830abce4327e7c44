"""The gallery search kernels (csrc/sim.hip: cosine_topk_x6_kernel<2>, topk_merge_kernel, topk_vote_kernel; csrc/simi8.hip:
rerank_topk_kernel) against float64 references at every slot, with write footprints, the tie rule and the masks.  Every case of
tests/topk_cases.py.

CPU (wherever the library is built): every case passes its entry point's argument checks with M = 0, and k = 0, k = 17, k > pool,
D % 32 (search) and D % 64 (rerank), a misaligned ginv and G / rows both given or both missing are refused; the fp64 bound
2 * max|ref32 - ref64| + 2e-7 (the float32 reference in both summation orders, over the k returned slots of every row) is below
1e-5 on every case, at most 1 % of the slots that are not planted are unsure, every planted tie is exact and comes back lowest index
first, and the float32 reference agrees with the float64 one at every exact slot; the eleven mutants of topk_cases.MUTANTS each
move a slot by more than the bound or change an index at an exact slot on the cases named for them; and the protocol itself, run
on the host against a stand-in that answers with a float32 evaluation, passes -- and fails once the stand-in nudges one score
by three bounds, swaps two sure slots, returns the higher index of a boundary tie, repeats an index, returns a masked column,
leaves one slot unwritten, writes one guard element or puts anything but -inf / -1 behind the valid slots.

GPU, fp_cosine_topk_x6 (called through _lib on the test's own buffers; every case at every n_splits of the case): scores and idx
carry 64 guard elements behind M * k and start as sentinels, the workspace is exactly fp_cosine_topk_workspace(M, N, k, n_splits)
bytes followed by 4 KiB of sentinels; after the call all guards are unchanged and every slot below M * k is written.  Per row and
slot: |score - S64[m, idx]| within the bound; scores non-increasing; indices in range, live (not masked, not a NaN score) and
distinct; the k-th returned fp64 score >= the (k+1)-th reference score - 2 * bound; the index is the reference's at every exact
slot (sure gaps to both neighbours, or a planted tie: lowest index first, the lowest indices of a tie that k cuts); -inf / -1
behind the valid slots, in every slot of a zero query row, a NaN query row and a fully masked gallery.  All n_splits values and a
second run give the same bits; so do planes that fp_split3_rows wrote into a buffer of 0xFF and planes whose padding rows hold
random bits; slot 0 equals fp_cosine_filter_x6's best / arg bit for bit on every unmasked case (scaled and negative included).
GPU, fp_rerank_topk: the same guards and checks against its bound in indexed mode; compact mode and a second run give the same
bits; an index that a list names more than once comes back once.
GPU, fp_topk_vote: label, score and votes guarded, all three equal to the rule of similarity.topk_vote exactly in both modes, at
tau on a score value (>= holds) and one ulp above (it does not).

Largest error / bound measured on the MI355X: fp_cosine_topk_x6 0.36 (x6_257x1100x512x16_masked_scatter: 1.8e-7 of 5.1e-7; the ties
cases, with scores of 1, reach 4.0e-7 of 1.5e-6), fp_rerank_topk 0.24 (rr_37x500x64x24x5_scaled: 9.4e-8 of 3.9e-7); fp_topk_vote is
compared by equality.  The one defect the cases found: rerank_topk_kernel ranked equal keys by list position, so a gallery row
that a candidate list named twice came back twice (rr_37x500x64x24x5_dup); a list is now a set of rows (include/facepath.h).
"""
import ctypes

import numpy as np
import pytest
import torch

import topk_cases as C
from face_detection_and_recognition_amd import _lib as L

SENT_SCORE, SENT_IDX, SENT_BYTE = 0x7FC0BEEF, -7, 0xA5
I32 = torch.int32
FP_ERR_ALIGNMENT = -5
X6_IDS, RR_IDS, VOTE_IDS = ([c.name for c in cs] for cs in (C.X6_CASES, C.RERANK_CASES, C.VOTE_CASES))


def _refs(c):
    return C.x6_references(c) if c.entry == C.X6 else C.rerank_references(c)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the argument checks, the table, the bound, the mutants
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", X6_IDS + RR_IDS + VOTE_IDS)
def test_case_passes_the_argument_checks(lib, name):
    """The shape of every case is accepted (the checks run before the M == 0 return, so no device is needed)."""
    c = C.BY_NAME[name]
    buf = torch.zeros(64)
    assert buf.data_ptr() % 16 == 0
    p = L.ptr(buf)
    if c.entry == C.X6:
        M, N, D, k = c.shape
        for ns in c.n_splits:
            assert lib.fp_cosine_topk_x6(p, p, 0, p, p, N, D, k, ns, p, p, p, 0, None) == L.FP_OK
        assert max(M, N, D) <= 1200 and M <= 300 and D <= 512
    elif c.entry == C.RERANK:
        M, N, D, pool, k = c.shape
        assert lib.fp_rerank_topk(p, p, 0, D, p, pool, p, None, p, N, k, p, p, None) == L.FP_OK
        assert lib.fp_rerank_topk(p, p, 0, D, p, pool, None, p, p, N, k, p, p, None) == L.FP_OK
    else:
        M, N, k = c.shape
        for mode in (0, 1):
            assert lib.fp_topk_vote(p, p, 0, k, p, N, ctypes.c_float(C.VOTE_TAU), mode, p, p, p, None) == L.FP_OK


def test_refusals(lib):
    buf = torch.zeros(64)
    p, off = L.ptr(buf), ctypes.c_void_p(buf.data_ptr() + 4)
    x6 = lambda D=64, k=5, ginv=p, ns=0: lib.fp_cosine_topk_x6(p, p, 0, p, ginv, 100, D, k, ns, p, p, p, 0, None)  # noqa: E731
    assert x6() == L.FP_OK
    assert x6(k=0) == x6(k=17) == x6(ns=-1) == L.FP_ERR_INVALID_ARG
    assert x6(D=48) == x6(ginv=off) == FP_ERR_ALIGNMENT
    assert lib.fp_cosine_topk_workspace(10, 100, 0, 1) == lib.fp_cosine_topk_workspace(10, 100, 17, 1) == 0
    assert lib.fp_cosine_topk_workspace(10, 300, 16, 12) == lib.fp_cosine_topk_workspace(10, 300, 16, 3) == 10 * 3 * 16 * 8
    rr = lambda D=64, pool=8, k=5, G=p, rows=None: lib.fp_rerank_topk(p, p, 0, D, p, pool, G, rows, p, 100, k, p, p, None)  # noqa: E731
    assert rr() == rr(G=None, rows=p) == rr(pool=64, k=16) == L.FP_OK
    assert rr(k=0) == rr(pool=32, k=17) == rr(pool=4, k=5) == rr(pool=65) == L.FP_ERR_INVALID_ARG
    assert rr(rows=p) == rr(G=None) == L.FP_ERR_INVALID_ARG
    assert rr(D=96) == rr(D=32) == FP_ERR_ALIGNMENT
    vote = lambda k=5, mode=1: lib.fp_topk_vote(p, p, 0, k, p, 10, ctypes.c_float(0.5), mode, p, p, p, None)  # noqa: E731
    assert vote() == L.FP_OK and vote(k=0) == vote(k=17) == vote(mode=2) == L.FP_ERR_INVALID_ARG


def test_the_table_holds_what_the_pin_names():
    x6 = {c.name: c for c in C.X6_CASES}
    shapes = {c.shape for c in C.X6_CASES}
    assert {(1, 1, 32, 1), (3, 5, 32, 16), (64, 127, 32, 5), (64, 128, 32, 16), (64, 129, 64, 16), (33, 130, 32, 2), (33, 131, 32, 15),
            (130, 257, 96, 5), (129, 640, 128, 16), (257, 1100, 512, 16), (257, 1100, 512, 1)} <= shapes
    for c in C.X6_CASES:
        if c.shape[1] > 2 * C.CHUNK:
            assert c.n_splits == (0, 1, 2, 4, 9, 12), c.name
    multi16 = {c.kind.split("_")[0] for c in C.X6_CASES if c.shape[1] >= 640 and c.k == 16}
    assert multi16 == {"normal", "ties", "ascending", "descending", "negative", "masked"}
    for k in (1, 5):
        assert {"ties", "masked"} <= {c.kind.split("_")[0] for c in C.X6_CASES if c.k == k}
    assert {c.kind for c in C.X6_CASES if c.shape == (257, 1100, 512, 16)} >= set(C._MASKS)
    assert any(c.scaled for c in x6.values()) and x6["x6_129x640x128x16_negative"].scaled
    assert {c.shape for c in C.RERANK_CASES} == {(37, 500, 64, 24, 5), (5, 300, 1024, 64, 16), (130, 257, 128, 1, 1), (9, 40, 64, 16, 16)}
    assert {c.shape[2] for c in C.VOTE_CASES} == {1, 5, 16} and all(c.shape[0] == 1000 for c in C.VOTE_CASES)


@pytest.mark.parametrize("name", X6_IDS + RR_IDS)
def test_reference_is_sure_and_the_bound_is_tight(name):
    """The bound is below 1e-5; at most 1 % of the slots that are not planted are unsure; the float32 reference (plain sums) has
    the float64 index at every exact slot and lies within the bound; the planted ties are exact, lowest index first."""
    c = C.BY_NAME[name]
    r = _refs(c)
    d = C.x6_inputs(c) if c.entry == C.X6 else C.rerank_inputs(c)
    valid = r["idx"] >= 0
    free = valid & ~r["planted"]
    unsure = float((free & ~r["exact"]).sum()) / max(int(free.sum()), 1)
    print(f"{name}: bound {r['bound']:.3e} (blocked {r['err_blocked']:.2e}, sequential {r['err_seq']:.2e}), unsure {100 * unsure:.2f} % "
          f"of {int(free.sum())} slots, {int(r['planted'].sum())} planted")
    assert C.TOL <= r["bound"] < 1e-5
    assert unsure <= 0.01
    assert r["exact"][r["planted"]].all(), f"{name}: a planted tie whose outer gaps are not sure"
    _, _, r32 = C.reference32(c)
    ex = r["exact"]
    np.testing.assert_array_equal(r32["idx"][ex], r["idx"][ex])
    np.testing.assert_array_equal(r32["idx"] >= 0, valid)
    assert np.abs(r32["sc"][valid].astype(np.float64) - r["sc"][valid]).max(initial=0.0) <= r["bound"]
    for m, cols, label in d.get("plan", []):
        n = len(cols)
        assert r["idx"][m, :n].tolist() == list(cols) and r["exact"][m, :n].all(), (name, m, cols, label)
        if n > 1 and not label.startswith("k - 1"):
            assert r["planted"][m, :n].all() and abs(r["sc"][m, 0] - 1.0) < 1e-6
    M, N = r["S"].shape
    k = c.k
    if c.kind == "ties":
        assert {p[2] for p in d["plan"]} >= {t[0] for t in C.TIE_PAIRS}
        cut = [m for m in range(M) if r["nvalid"][m] > k and r["sorted"][m, k - 1] == r["sorted"][m, k]]
        assert len(cut) >= 2, "no tie at the k-th slot"
    if c.kind in ("ascending", "descending"):
        s = r["S"][0]
        assert (np.diff(s) > 0).all() if c.kind == "ascending" else (np.diff(s) < 0).all()
    if c.kind == "negative":
        S = r["S"]
        assert (S[0::4] < 0).all()
        row = r["sc"][1] if M < 5 else r["sc"][5]
        assert (row > 0).any() and (row == 0).sum() >= 2 and ((row < 0).any() or N < k)
        assert c.scaled or d["qinv"][1] == 1.0
    if c.kind.startswith("masked"):
        assert r["nvalid"][M // 2] == 0 and r["nvalid"][M // 2 + 1] == 0 and np.isinf(d["ginv"][N // 3])
        assert not (r["idx"] == N // 3).any() and not np.isin(r["idx"], np.flatnonzero(d["ginv"] == 0)).any()
        what = c.kind.split("_")[1]
        live = int((d["ginv"] != 0).sum()) - 1
        assert {"all": live == 0, "few": live == k - 1, "chunk": (d["ginv"][128:256] == 0).all() and live == N - 129,
                "split": (d["ginv"][640:] == 0).all() and live == 639, "scatter": 0.7 * N < live < 0.9 * N}[what]
    if c.entry == C.RERANK and M >= 5:
        assert r["nvalid"][2] == 0 and r["nvalid"][3] == 0 and r["nvalid"][1] < max(k, 2) and (r["nvalid"] < k).sum() >= 3
        if c.shape[3] >= 4:
            assert r["idx"][0, :2].tolist() == [7, 19] and r["idx"][4, :2].tolist()[0] == 11 and r["planted"][0, :2].all()
            cand = d["cand"]
            assert (cand >= N).any() and (cand == -1).any() and (d["ginv"][cand[(cand >= 0) & (cand < N)]] == 0).any()
        if c.kind == "dup":
            assert (d["cand"][0] == 7).sum() == 3 and (d["cand"][4] == 11).all() and r["nvalid"][4] == 1


@pytest.mark.parametrize("label,mut,name", [(lab, mut, n) for lab, mut, names in C.MUTANTS for n in names],
                         ids=[f"{mut}-{n}" for _, mut, names in C.MUTANTS for n in names])
def test_mutants_are_caught(label, mut, name):
    c = C.BY_NAME[name]
    shift, moved = C.mutant_shift(c, mut)
    bound = C.x6_references(c)["bound"]
    print(f"{name}: {label}: moves a slot by {shift:.3e} (bound {bound:.3e}), changes {moved} exact indices")
    assert shift > bound or moved > 0, f"{name}: {label} is not caught: shift {shift:.3e}, bound {bound:.3e}, {moved} indices"
    if mut in ("hm", "kslab", "inv4"):
        assert shift > bound
    if mut in ("tie_high", "gt", "swap", "dup", "lastchunk", "remchunk", "ginvtail"):
        assert moved > 0


def test_vote_cases_hold_what_the_pin_names():
    for c in C.VOTE_CASES:
        d = C.vote_inputs(c)
        M, N, k = c.shape
        sc, ix = d["scores"], d["idx"]
        assert (sc[:, 1:] <= sc[:, :-1]).all() and np.isin(sc[np.isfinite(sc)], C.VOTE_GRID).all()
        assert (ix >= N).any() and ((ix == -1) == np.isneginf(sc)).all() and (ix[:, 0] == -1).any() and (sc == np.float32(C.VOTE_TAU)).any()
        lab, score, votes = C.vote_reference(sc, ix, d["labels"], C.VOTE_TAU, 1)
        up = C.vote_reference(sc, ix, d["labels"], np.nextafter(np.float32(C.VOTE_TAU), np.float32(1)), 1)
        assert (up[2] < votes).any() and (lab == -1).any() and votes.max() == min(k, votes.max())
        if k > 1:
            top1 = C.vote_reference(sc, ix, d["labels"], C.VOTE_TAU, 0)[0]
            assert (top1 != lab).any() and votes.max() >= 3
    # the hand-worked rows of tests/test_topk_gpu.py through this reference
    labels = np.array([0, 0, 1, 1, 2, 2, 7, 3], np.int32)
    sc = np.array([[0.9, 0.5, 0.4, 0.2], [0.9, 0.7, 0.6, 0.5], [0.5, 0.5, 0.5, 0.5], [0.875, 0.75, 0.5, 0.375]], np.float32)
    ix = np.array([[2, 0, 1, 4], [0, 2, 3, 1], [6, 7, 2, 4], [2, 4, 5, 3]], np.int32)
    lab, score, votes = C.vote_reference(sc, ix, labels, 0.3, 1)
    assert lab.tolist() == [0, 0, 1, 1] and votes.tolist() == [2, 2, 1, 2] and score.tolist() == np.array([0.5, 0.9, 0.5, 0.875], np.float32).tolist()


# ---------------------------------------------------------------------------------------------------------------------------
# the protocol (GPU tests; on the host against a stand-in)
# ---------------------------------------------------------------------------------------------------------------------------
class _Device:
    """The entry points of libfacepath on device tensors."""

    def __init__(self, dev):
        self.dev, self.lib = dev, L.load()

    def ws_bytes(self, c, ns):
        M, N, D, k = c.shape
        return self.lib.fp_cosine_topk_workspace(M, N, k, ns)

    def x6(self, c, T, ns, ws, ws_bytes):
        M, N, D, k = c.shape
        L.check(self.lib.fp_cosine_topk_x6(L.ptr(T["Q"]), L.ptr(T["qinv"]), M, L.ptr(T["g3"]), L.ptr(T["ginv"]), N, D, k, ns,
                                           L.ptr(T["scores"]), L.ptr(T["idx"]), L.ptr(ws), ws_bytes, L.current_stream(self.dev)), c.name)
        torch.cuda.synchronize()

    def rerank(self, c, T, compact):
        M, N, D, pool, k = c.shape
        L.check(self.lib.fp_rerank_topk(L.ptr(T["Q"]), L.ptr(T["qinv"]), M, D, L.ptr(T["cand"]), pool, None if compact else L.ptr(T["G"]),
                                        L.ptr(T["rows"]) if compact else None, L.ptr(T["ginv"]), N, k, L.ptr(T["scores"]),
                                        L.ptr(T["idx"]), L.current_stream(self.dev)), c.name)
        torch.cuda.synchronize()


class _Host:
    """A stand-in for the entry points on the host: topk_cases.reference32 (float32, every score a plain sum over D, the first
    index wins) -- with one planted defect, if any."""

    def __init__(self, fault=None):
        self.dev, self.fault = torch.device("cpu"), fault

    def ws_bytes(self, c, ns):
        M, N, D, k = c.shape
        return M * max(1, min(ns, -(-N // C.CHUNK))) * k * 8

    def _answer(self, c, T, ws=None):
        M, k = c.shape[0], c.k
        r, d = _refs(c), (C.x6_inputs(c) if c.entry == C.X6 else C.rerank_inputs(c))
        base = C.reference32(c)[2]
        sc, idx = base["sc"].copy(), base["idx"].copy()
        both = np.flatnonzero(r["exact"][:, :2].all(axis=1)) if k > 1 else []
        f = self.fault
        if f == "nudge":
            m = int(np.flatnonzero(idx[:, 0] >= 0)[-1])
            sc[m, 0] += np.float32(3.0 * r["bound"])
        elif f == "swap":
            m = int(both[0])
            sc[m, :2], idx[m, :2] = sc[m, 1::-1].copy(), idx[m, 1::-1].copy()
        elif f == "tie_high":
            m, cols, _ = next(p for p in d["plan"] if p[2].startswith("k + 2"))
            idx[m, k - 1] = int(np.flatnonzero((d["G"] == d["G"][cols[0]]).all(axis=1))[k])
        elif f == "dup":
            m = int(both[-1])
            sc[m, 1], idx[m, 1] = sc[m, 0], idx[m, 0]
        elif f == "masked":
            m = int(np.flatnonzero(idx[:, 0] >= 0)[0])
            idx[m, 0] = int(np.flatnonzero(d["ginv"] == 0)[0])
        elif f == "tail":
            m = int(np.flatnonzero(idx[:, k - 1] < 0)[0])
            sc[m, k - 1] = 0.0
        flat = np.arange(M * k)
        if f == "hole":
            flat = np.delete(flat, (M // 2) * k + k - 1)
        at = torch.from_numpy(flat)
        T["scores"][at] = torch.from_numpy(sc.reshape(-1))[at]
        T["idx"][at] = torch.from_numpy(idx.reshape(-1))[at]
        if f == "guard":
            T["idx"][M * k + 1] = 3
        if f == "ws_guard" and ws is not None:
            ws[-C.WS_GUARD] = 0

    def x6(self, c, T, ns, ws, ws_bytes):
        self._answer(c, T, ws)

    def rerank(self, c, T, compact):
        self._answer(c, T)


def _outputs(c, be, T):
    n = c.shape[0] * c.k + C.GUARD
    T["scores"] = torch.empty(n, dtype=torch.float32, device=be.dev)
    T["idx"] = torch.empty(n, dtype=I32, device=be.dev)
    return T


def _call(c, T, fn):
    """Sentinels into scores and idx, one call; the guards (everything behind M * k) unchanged, every slot below written ->
    (scores (M, k) float32, idx (M, k) int32) as numpy."""
    M, k = c.shape[0], c.k
    T["scores"].view(I32).fill_(SENT_SCORE)
    T["idx"].fill_(SENT_IDX)
    fn()
    out = []
    for key, sent in (("scores", SENT_SCORE), ("idx", SENT_IDX)):
        v = T[key].view(I32).cpu().numpy()
        stray = np.flatnonzero(v[M * k:] != sent)
        assert stray.size == 0, f"{c.name}: {stray.size} guard elements of {key} written, first at {M * k + stray[:8]}"
        holes = np.flatnonzero(v[:M * k] == sent)
        assert holes.size == 0, f"{c.name}: {holes.size} slots of {key} not written, first at {holes[:8]}"
        out.append(v[:M * k].copy().reshape(M, k))
    return out[0].view(np.float32), out[1]


def _call_x6(c, be, T, ns):
    """One search with a workspace of exactly the bytes the library asks for and WS_GUARD bytes of sentinels behind it."""
    nbytes = be.ws_bytes(c, ns)
    assert nbytes > 0 and nbytes % 8 == 0
    ws = torch.full((nbytes + C.WS_GUARD,), SENT_BYTE, dtype=torch.uint8, device=be.dev)
    assert ws.data_ptr() % 8 == 0
    got = _call(c, T, lambda: be.x6(c, T, ns, ws, nbytes))
    stray = np.flatnonzero(ws[nbytes:].cpu().numpy() != SENT_BYTE)
    assert stray.size == 0, f"{c.name} n_splits={ns}: {stray.size} guard bytes behind the workspace written, first at {nbytes + stray[:8]}"
    return got


def _check(c, sc, idx, what=""):
    """Every row and slot of one result against the float64 reference (module docstring) -> largest error / bound."""
    r = _refs(c)
    M, k = sc.shape
    N, bound = r["S"].shape[1], r["bound"]
    name = f"{c.name} {what}".strip()
    kv = np.minimum(r["nvalid"], k)
    slot = np.arange(k)[None, :]
    valid = slot < kv[:, None]
    bad = np.argwhere(~valid & ~(np.isneginf(sc) & (idx == -1)))
    assert bad.size == 0, f"{name}: not -inf / -1 behind the valid slots at (row, slot) {bad[:4].tolist()}"
    rows, slots = np.nonzero(valid)
    iv = idx[valid].astype(np.int64)
    bad = np.flatnonzero((iv < 0) | (iv >= N))
    assert bad.size == 0, f"{name}: an index outside [0, N) at (row, slot) {[(int(rows[i]), int(slots[i])) for i in bad[:4]]}"
    bad = np.flatnonzero(~r["ok"][rows, iv])
    assert bad.size == 0, (f"{name}: a column that is not live (masked, a NaN score, no candidate) returned at (row, slot, index) "
                           f"{[(int(rows[i]), int(slots[i]), int(iv[i])) for i in bad[:4]]}")
    srt = np.sort(np.where(valid, idx, -1 - slot), axis=1)
    bad = np.flatnonzero((srt[:, 1:] == srt[:, :-1]).any(axis=1))
    assert bad.size == 0, f"{name}: the indices of a row are not distinct in rows {bad[:8]}"
    s64 = r["S"][rows, iv]
    err = np.abs(sc[valid].astype(np.float64) - s64)
    worst = float(err.max(initial=0.0))
    ratio = worst / bound
    print(f"{name}: max |score - S64[m, idx]| {worst:.3e}, bound {bound:.3e}, ratio {ratio:.3f}")
    w = int(np.argmax(err)) if err.size else 0
    assert not err.size or worst <= bound, f"{name}: |score - S64[m, idx]| = {worst:.3e} above the bound {bound:.3e} at (row, slot) {(int(rows[w]), int(slots[w]))}"
    with np.errstate(invalid="ignore"):
        bad = np.argwhere(valid[:, 1:] & ~(sc[:, 1:] <= sc[:, :-1]))
    assert bad.size == 0, f"{name}: scores increase at (row, slot) {bad[:4].tolist()}"
    more = np.flatnonzero(r["nvalid"] > k)
    if more.size:
        kth = r["S"][more, idx[more, k - 1]]
        bad = more[kth < r["sorted"][more, k] - 2 * bound]
        assert bad.size == 0, f"{name}: the k-th returned score lies below the (k+1)-th candidate in rows {bad[:8]}"
    ex = r["exact"]
    bad = np.argwhere(ex & (idx != r["idx"]))
    assert bad.size == 0, (f"{name}: not the reference's index at {len(bad)} exact slots (row, slot, got, want) "
                           f"{[(int(m), int(s), int(idx[m, s]), int(r['idx'][m, s])) for m, s in bad[:6]]}")
    return ratio


def _same(c, a, b, what):
    for key, x, y in (("scores", a[0].view(np.int32), b[0].view(np.int32)), ("idx", a[1], b[1])):
        bad = np.argwhere(x != y)
        assert bad.size == 0, f"{c.name}: {what}: {key} differs at {len(bad)} slots, first (row, slot) {bad[:4].tolist()}"


def _x6_tensors(c, be):
    d = C.x6_inputs(c)
    T = {key: torch.from_numpy(d[key].copy()).to(be.dev) for key in ("Q", "qinv", "ginv")}
    T["g3"] = torch.from_numpy(C.planes(d["G"]).view(np.int16)).to(be.dev)
    assert T["ginv"].data_ptr() % 16 == 0
    return _outputs(c, be, T)


def _run_x6_case(c, be):
    """The protocol of one search case on a backend -> (tensors, first result, error / bound)."""
    T = _x6_tensors(c, be)
    first = ratio = None
    for ns in c.n_splits:
        got = _call_x6(c, be, T, ns)
        if first is None:
            first, ratio = got, _check(c, *got, what=f"n_splits={ns}")
        else:
            _same(c, got, first, f"n_splits = {ns} against {c.n_splits[0]}")
    _same(c, _call_x6(c, be, T, c.n_splits[-1]), first, "the second run")
    return T, first, ratio


def _rerank_tensors(c, be):
    d = C.rerank_inputs(c)
    T = {key: torch.from_numpy(d[key].copy()).to(be.dev) for key in ("Q", "G", "qinv", "ginv", "cand", "rows")}
    return _outputs(c, be, T)


def _run_rerank_case(c, be):
    T = _rerank_tensors(c, be)
    first = _call(c, T, lambda: be.rerank(c, T, False))
    ratio = _check(c, *first, what="indexed")
    _same(c, _call(c, T, lambda: be.rerank(c, T, True)), first, "compact mode against indexed mode")
    _same(c, _call(c, T, lambda: be.rerank(c, T, False)), first, "the second run")
    return first, ratio


HOST = ["x6_3x5x32x16_negative", "x6_33x131x32x15_normal", "x6_130x257x96x5_ties", "x6_130x257x96x5_masked_scatter",
        "x6_129x640x128x16_negative", "x6_257x1100x512x16_ties", "x6_257x1100x512x16_masked_few", "rr_37x500x64x24x5_dup",
        "rr_9x40x64x16x16"]
FAULTS = [("x6_130x257x96x5_ties", "nudge", "above the bound"), ("rr_37x500x64x24x5_dup", "nudge", "above the bound"),
          ("x6_33x131x32x15_normal", "swap", "scores increase"), ("x6_129x640x128x16_negative", "swap", "scores increase"),
          ("x6_130x257x96x5_ties", "tie_high", "not the reference's index"), ("x6_257x1100x512x16_ties", "tie_high", "not the reference's index"),
          ("x6_33x131x32x15_normal", "dup", "not distinct"), ("rr_37x500x64x24x5_dup", "dup", "not distinct"),
          ("x6_130x257x96x5_masked_scatter", "masked", "not live"), ("x6_257x1100x512x16_masked_few", "masked", "not live"),
          ("x6_130x257x96x5_ties", "hole", "not written"), ("rr_9x40x64x16x16", "hole", "not written"),
          ("x6_33x131x32x15_normal", "guard", "guard elements of idx written"), ("x6_130x257x96x5_ties", "ws_guard", "behind the workspace written"),
          ("x6_3x5x32x16_negative", "tail", "behind the valid slots"), ("x6_257x1100x512x16_masked_few", "tail", "behind the valid slots")]


def _run(c, be):
    return _run_x6_case(c, be) if c.entry == C.X6 else _run_rerank_case(c, be)


@pytest.mark.parametrize("name", HOST)
def test_protocol_passes_the_float32_stand_in_on_the_host(name):
    _run(C.BY_NAME[name], _Host())


@pytest.mark.parametrize("name,fault,message", FAULTS, ids=[f"{n}-{f}" for n, f, _ in FAULTS])
def test_protocol_catches_a_fault_on_the_host(name, fault, message):
    with pytest.raises(AssertionError, match=message):
        _run(C.BY_NAME[name], _Host(fault))


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", X6_IDS)
def test_topk_x6_vs_fp64(dev, name):
    """The protocol of the module docstring on one case, then the planes and, on an unmasked case, the filter's best."""
    c = C.BY_NAME[name]
    M, N, D, k = c.shape
    be = _Device(dev)
    T, first, _ = _run_x6_case(c, be)
    d = C.x6_inputs(c)
    ns = c.n_splits[-1]
    # planes written by fp_split3_rows into a buffer of 0xFF; then random bits in the padding rows
    nbytes = be.lib.fp_split3_bytes(N, D)
    assert nbytes == T["g3"].numel() * 2
    Gd = torch.from_numpy(d["G"].copy()).to(dev)
    host3 = T["g3"]
    T["g3"] = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
    L.check(be.lib.fp_split3_rows(L.ptr(Gd), N, D, L.ptr(T["g3"]), L.current_stream(dev)), "fp_split3_rows")
    _same(c, _call_x6(c, be, T, ns), first, "planes from fp_split3_rows over 0xFF")
    if N % C.CHUNK:
        T["g3"] = host3.clone()
        pad = T["g3"][:, :, N:]
        T["g3"][:, :, N:] = torch.from_numpy(C._rng(name, 7).integers(-32768, 32768, tuple(pad.shape)).astype(np.int16)).to(dev)
        _same(c, _call_x6(c, be, T, ns), first, "random bits in the padding rows of the planes")
    T["g3"] = host3
    if not c.kind.startswith("masked"):
        best = torch.full((M,), SENT_SCORE, dtype=I32, device=dev)
        arg = torch.full((M,), SENT_IDX, dtype=I32, device=dev)
        keep = torch.empty((M,), dtype=torch.uint8, device=dev)
        packed = torch.empty((M,), dtype=torch.int64, device=dev)
        L.check(be.lib.fp_cosine_filter_x6(L.ptr(T["Q"]), L.ptr(T["qinv"]), M, L.ptr(T["g3"]), L.ptr(T["ginv"]), N, D, ctypes.c_float(0.0),
                                           L.ptr(best), L.ptr(arg), L.ptr(keep), L.ptr(packed), L.current_stream(dev)), "fp_cosine_filter_x6")
        torch.cuda.synchronize()
        bad = np.flatnonzero((best.cpu().numpy() != first[0][:, 0].view(np.int32)) | (arg.cpu().numpy() != first[1][:, 0]))
        assert bad.size == 0, f"{name}: slot 0 differs from fp_cosine_filter_x6's best / arg in rows {bad[:8]}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", RR_IDS)
def test_rerank_vs_fp64(dev, name):
    _run_rerank_case(C.BY_NAME[name], _Device(dev))


@pytest.mark.gpu
@pytest.mark.parametrize("name", VOTE_IDS)
def test_vote_equals_the_rule(dev, name):
    c = C.BY_NAME[name]
    M, N, k = c.shape
    d = C.vote_inputs(c)
    lib = L.load()
    T = {key: torch.from_numpy(d[key].copy()).to(dev) for key in ("scores", "idx", "labels")}
    tau = np.float32(C.VOTE_TAU)
    for t in (tau, np.nextafter(tau, np.float32(1))):
        for mode in (0, 1):
            lab = torch.full((M + C.GUARD,), SENT_IDX, dtype=I32, device=dev)
            score = torch.full((M + C.GUARD,), SENT_SCORE, dtype=I32, device=dev)
            votes = torch.full((M + C.GUARD,), SENT_IDX, dtype=I32, device=dev)
            L.check(lib.fp_topk_vote(L.ptr(T["scores"]), L.ptr(T["idx"]), M, k, L.ptr(T["labels"]), N, ctypes.c_float(float(t)), mode,
                                     L.ptr(lab), L.ptr(score), L.ptr(votes), L.current_stream(dev)), "fp_topk_vote")
            torch.cuda.synchronize()
            want = C.vote_reference(d["scores"], d["idx"], d["labels"], t, mode)
            for key, got, w, sent in (("label", lab, want[0], SENT_IDX), ("score", score, want[1].view(np.int32), SENT_SCORE),
                                      ("votes", votes, want[2], SENT_IDX)):
                h = got.cpu().numpy()
                assert (h[M:] == sent).all(), f"{name}: guard elements of {key} written"
                assert not (h[:M] == sent).any(), f"{name}: rows of {key} not written"
                bad = np.flatnonzero(h[:M] != w)
                assert bad.size == 0, f"{name} mode {mode} tau {t!r}: {key} differs from the rule in {bad.size} rows, first {bad[:8]}"
