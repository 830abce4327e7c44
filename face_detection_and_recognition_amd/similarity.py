"""Similarity-filter operators on device tensors (csrc/sim.hip).

  l2_mean_thres / l2_filter  — the reference's filter arithmetic
      (similar_face_filtering/filter_faces_using_reference.py:85-99, 186-189)
  cosine_filter              — batched cosine filter (cosine of
      face_detection_and_extraction/face_extraction/extract_and_label_faces_from_dataset.py:106)
  cosine_topk / topk_vote    — the k best gallery rows of every query and the identity they vote for (build-defined)
"""
import numpy as np
import torch

from . import _lib as L


def _f32c(t):
    assert t.is_cuda and t.dtype == torch.float32
    return t.contiguous()


def row_inv_norm(x):
    x = _f32c(x)
    out = torch.empty((x.shape[0],), dtype=torch.float32, device=x.device)
    L.check(L.load().fp_row_inv_norm(L.ptr(x), x.shape[0], x.shape[1], L.ptr(out), L.current_stream(x.device)),
            "fp_row_inv_norm")
    return out


def split3_rows(R):
    """The reference rows as three bf16 planes for cosine_filter's split-MFMA kernel (csrc/split.h: exact three-way split of
    every fp32 value; layout [D / 32][3][round_up(Nr, 128)][32]).  Done once per reference set."""
    R = _f32c(R)
    Nr, D = R.shape
    lib = L.load()
    out = torch.empty((lib.fp_split3_bytes(Nr, D),), dtype=torch.uint8, device=R.device)
    L.check(lib.fp_split3_rows(L.ptr(R), Nr, D, L.ptr(out), L.current_stream(R.device)), "fp_split3_rows")
    return out


def cosine_filter(G, R, tau, ginv=None, rinv=None, r3=None, x6=None):
    """G (M, D) gallery, R (Nr, D) reference -> best (M,), arg (M,) int32, keep (M,) bool.
    The M x Nr score matrix is never materialised.  x6 (default: PlanBuilder.X6 and D a multiple of 32): S = G R^T on the
    bf16 matrix cores with fp32-equivalent split arithmetic (r3 = split3_rows(R), computed here when not passed in).
    score = <G[m], R[j]> * ginv[m] * rinv[j]; on equal scores the lowest j.  Zero rows and masks (pinned by
    tests/test_similarity_ops.py): an all-zero gallery row has ginv = inf, every score of it is NaN and it gives best = NaN,
    arg = -1, keep = False; an all-zero reference row has rinv = inf, its scores are NaN and it never wins.  An explicitly
    passed rinv of 0 is NOT a mask here, unlike ginv in cosine_topk: that column scores exactly 0 (+0 or -0) in every row and
    wins wherever the other scores are negative.  To exclude a reference row, leave it out of R."""
    from .plan import PlanBuilder
    G, R = _f32c(G), _f32c(R)
    M, D = G.shape
    Nr = R.shape[0]
    assert R.shape[1] == D
    ginv = row_inv_norm(G) if ginv is None else ginv
    rinv = row_inv_norm(R) if rinv is None else rinv
    dev = G.device
    best = torch.empty((M,), dtype=torch.float32, device=dev)
    arg = torch.empty((M,), dtype=torch.int32, device=dev)
    keep = torch.empty((M,), dtype=torch.uint8, device=dev)
    packed = torch.empty((M,), dtype=torch.int64, device=dev)
    if x6 is None:
        x6 = PlanBuilder.X6 and D % 32 == 0
    if x6:
        r3 = split3_rows(R) if r3 is None else r3
        L.check(L.load().fp_cosine_filter_x6(L.ptr(G), L.ptr(ginv), M, L.ptr(r3), L.ptr(rinv), Nr, D, float(tau),
                                             L.ptr(best), L.ptr(arg), L.ptr(keep), L.ptr(packed), L.current_stream(dev)),
                "fp_cosine_filter_x6")
    else:
        L.check(L.load().fp_cosine_filter(L.ptr(G), L.ptr(ginv), M, L.ptr(R), L.ptr(rinv), Nr, D, float(tau),
                                          L.ptr(best), L.ptr(arg), L.ptr(keep), L.ptr(packed), L.current_stream(dev)),
                "fp_cosine_filter")
    return best, arg, keep.bool()


def pad_features(x):
    """x (M, D) with D zero-padded to the next multiple of 32 (what the split-MFMA kernels take).  Zeros change neither
    the dot products nor the norms.  Returns x itself when D already is one."""
    D = x.shape[1]
    return x if D % 32 == 0 else torch.nn.functional.pad(x, (0, 32 - D % 32)).contiguous()


def cosine_topk(Q, G, k, qinv=None, ginv=None, g3=None, n_splits=0):
    """Q (M, D) queries, G (N, D) gallery -> scores (M, k) fp32 descending, idx (M, k) int32 gallery rows; on equal scores the
    lower index first.  A gallery row whose ginv is 0 is excluded; slots beyond the valid rows hold -inf / -1.  The M x N
    score matrix is never materialised, the result is deterministic and does not depend on n_splits (0 = chosen from M and
    the device; a positive value is clamped to the number of 128-column chunks).  One kernel (bf16 split arithmetic as
    cosine_filter's x6 form): when D is not a multiple of 32 both operands are zero-padded first.  g3 = split3_rows of the
    (padded) gallery, computed here when not passed in; G may then be None if ginv is given with it."""
    Q = pad_features(_f32c(Q))
    M, D = Q.shape
    k = int(k)
    if g3 is None or ginv is None:
        G = pad_features(_f32c(G))
        assert G.shape[1] == D
        ginv = row_inv_norm(G) if ginv is None else ginv
        g3 = split3_rows(G) if g3 is None else g3
    N = ginv.shape[0]
    qinv = row_inv_norm(Q) if qinv is None else qinv
    assert ginv.dtype == torch.float32 and ginv.is_contiguous() and qinv.dtype == torch.float32 and qinv.is_contiguous()
    dev = Q.device
    lib = L.load()
    scores = torch.empty((M, k), dtype=torch.float32, device=dev)
    idx = torch.empty((M, k), dtype=torch.int32, device=dev)
    ws_bytes = lib.fp_cosine_topk_workspace(M, N, k, int(n_splits))
    ws = torch.empty((max(ws_bytes, 8) // 8,), dtype=torch.int64, device=dev)
    L.check(lib.fp_cosine_topk_x6(L.ptr(Q), L.ptr(qinv), M, L.ptr(g3), L.ptr(ginv), N, D, k, int(n_splits), L.ptr(scores),
                                  L.ptr(idx), L.ptr(ws), ws.numel() * 8, L.current_stream(dev)), "fp_cosine_topk_x6")
    return scores, idx


# ---- the compressed gallery: int8 coarse search + exact rerank (csrc/simi8.hip, DESIGN S7 "Compressed gallery") -------------
def pad_features64(x):
    """x (M, D) with D zero-padded to the next multiple of 64 (one k-slab of the i8 MFMA).  x itself when D already is one."""
    D = x.shape[1]
    return x if D % 64 == 0 else torch.nn.functional.pad(x, (0, 64 - D % 64)).contiguous()


def quantize_rows_i8(X):
    """X (N, D) fp32 on the device -> q8 (D64 / 64, round_up(N, 128), 64) int8, the staged layout of the coarse search with zero
    rows in the padding, and scale (N,) fp32.  Per row q = rint(x * (127 / amax)), scale = amax / 127; a row that is all zero
    or holds a non-finite value is dead (q = 0, scale = 0).  Equal to quantize_rows_i8_numpy byte for byte, bit for bit."""
    X = pad_features64(_f32c(X))
    N, D = X.shape
    if D > L.QUANT_MAX_D:
        raise ValueError(f"{D} features: the int8 search takes at most {L.QUANT_MAX_D} (the int32 dot must convert to fp32 exactly)")
    lib = L.load()
    q8 = torch.empty((D // 64, lib.fp_quant_i8_bytes(N, D) // D, 64), dtype=torch.int8, device=X.device)
    scale = torch.empty((N,), dtype=torch.float32, device=X.device)
    L.check(lib.fp_quantize_rows_i8(L.ptr(X), N, D, L.ptr(q8), L.ptr(scale), L.current_stream(X.device)), "fp_quantize_rows_i8")
    return q8, scale


def stage_rows_i8(q):
    """q (N, D) int8 codes, D a multiple of 64 -> the staged layout of quantize_rows_i8 (plain tensor moves; for tests and tools
    that bring their own codes)."""
    N, D = q.shape
    assert q.dtype == torch.int8 and D % 64 == 0
    out = torch.zeros((D // 64, (N + 127) // 128 * 128, 64), dtype=torch.int8, device=q.device)
    out[:, :N] = q.reshape(N, D // 64, 64).permute(1, 0, 2)
    return out


def unstage_rows_i8(q8, N):
    """The inverse of stage_rows_i8: (N, D) int8."""
    return q8[:, :N].permute(1, 0, 2).reshape(N, -1).contiguous()


def quantize_rows_i8_numpy(X):
    """The restatement of quantize_rows_i8 in numpy fp32: X (N, D) -> q (N, D64) int8 row-major, scale (N,) fp32."""
    X = np.asarray(X, np.float32)
    if X.shape[1] % 64:
        X = np.pad(X, ((0, 0), (0, 64 - X.shape[1] % 64)))
    with np.errstate(all="ignore"):
        amax = np.abs(X).max(axis=1)
        dead = ~np.isfinite(X).all(axis=1) | (amax == 0)
        safe = np.where(dead, np.float32(1), amax).astype(np.float32)
        r = (np.float32(127) / safe).astype(np.float32)
        y = np.rint((X * r[:, None]).astype(np.float32))
        y = np.clip(np.where(np.isnan(y), np.float32(0), y), -127, 127)
        q = y.astype(np.int8)
        q[dead] = 0
        scale = np.where(dead, np.float32(0), (safe / np.float32(127)).astype(np.float32)).astype(np.float32)
    return q, scale


def cosine_topk_i8(qq, u, g8, w, N, pool, n_splits=0):
    """The coarse search.  qq / g8: staged int8 codes of the M = len(u) queries and the N gallery rows (quantize_rows_i8),
    u (M,) fp32 positive per-query factors, w (N,) fp32 per-row weights, ANY values: c = fp32(float(int32 dot) * w[n]) orders
    the rows (higher first, then the LOWER index), the score returned is fp32(c * u[m]).  w == 0 masks a gallery row; a query
    whose u is not positive and finite is dead.  -> scores (M, pool) fp32 non-increasing, idx (M, pool) int32, -inf / -1 for
    dead queries and beyond the live rows.  Exactly cosine_topk_i8_numpy, for every n_splits."""
    assert qq.dtype == torch.int8 and g8.dtype == torch.int8 and qq.is_contiguous() and g8.is_contiguous()
    assert qq.shape[0] == g8.shape[0], "queries and gallery differ in (padded) features"
    u, w = _f32c(u), _f32c(w)
    M, pool, N = u.shape[0], int(pool), int(N)
    assert w.shape[0] == N and qq.shape[1] == (M + 127) // 128 * 128 and g8.shape[1] == (N + 127) // 128 * 128 and qq.shape[2] == 64
    D = qq.shape[0] * 64
    dev = g8.device
    lib = L.load()
    scores = torch.empty((M, pool), dtype=torch.float32, device=dev)
    idx = torch.empty((M, pool), dtype=torch.int32, device=dev)
    ws_bytes = lib.fp_cosine_topk_i8_workspace(M, N, pool, int(n_splits))
    ws = torch.empty((max(ws_bytes, 8) // 8,), dtype=torch.int64, device=dev)
    L.check(lib.fp_cosine_topk_i8(L.ptr(qq), L.ptr(u), M, L.ptr(g8), L.ptr(w), N, D, pool, int(n_splits), L.ptr(scores),
                                  L.ptr(idx), L.ptr(ws), ws.numel() * 8, L.current_stream(dev)), "fp_cosine_topk_i8")
    return scores, idx


def cosine_topk_i8_numpy(qq, u, qg, w, pool):
    """The restatement of cosine_topk_i8: qq (M, D) / qg (N, D) int8 ROW-MAJOR codes, u (M,), w (N,) fp32."""
    qq, qg = np.asarray(qq), np.asarray(qg)
    u, w = np.asarray(u, np.float32), np.asarray(w, np.float32)
    M, N = qq.shape[0], qg.shape[0]
    dots = qq.astype(np.float64) @ qg.astype(np.float64).T             # integers below 2^53: exact
    with np.errstate(all="ignore"):
        c = (dots.astype(np.float32) * w[None, :]).astype(np.float32)
        live_q = (u > 0) & np.isfinite(u)
        out = ~live_q[:, None] | (w == 0)[None, :] | np.isnan(c)
        c = np.where(out, -np.inf, c).astype(np.float32)
        order = np.argsort(-c, axis=1, kind="stable")[:, :pool]         # stable: the lower index first on equal scores
        cs = np.take_along_axis(c, order, 1)
        gone = np.take_along_axis(out, order, 1)
        scores = np.where(gone, -np.inf, (cs * u[:, None]).astype(np.float32)).astype(np.float32)
        idx = np.where(gone, -1, order).astype(np.int32)
    if N < pool:
        scores = np.pad(scores, ((0, 0), (0, pool - N)), constant_values=-np.inf)
        idx = np.pad(idx, ((0, 0), (0, pool - N)), constant_values=-1)
    return scores, idx


def rerank_topk(Q, cand, k, G=None, ginv=None, qinv=None, rows=None):
    """The exact scores of a candidate list.  Q (M, D) fp32, cand (M, pool) int32 gallery rows (-1 and rows whose ginv is 0 are
    skipped, a row named more than once counts once), ginv (N,) -> scores (M, k) descending, idx (M, k) int32 gallery rows, -inf / -1 behind the valid ones.  The fp32
    rows come from G (N, D64) on the device, or from rows (M, pool, D64): the candidates' rows gathered in the order of cand
    (a gallery whose rows live on the host).  score = <Q, row> * qinv * ginv in fp32 with a fixed summation order: both
    modes and every run give the same bits.  D64: the features zero-padded to a multiple of 64 (pad_features64)."""
    Q = pad_features64(_f32c(Q))
    M, D = Q.shape
    cand = cand.contiguous()
    assert cand.dtype == torch.int32 and cand.shape[0] == M and (G is None) != (rows is None) and ginv is not None
    pool, k = cand.shape[1], int(k)
    src = _f32c(G if rows is None else rows)
    assert src.shape[-1] == D and (rows is None or tuple(src.shape) == (M, pool, D))
    ginv = _f32c(ginv)
    assert rows is not None or src.shape[0] == ginv.shape[0]
    qinv = row_inv_norm(Q) if qinv is None else _f32c(qinv)
    dev = Q.device
    scores = torch.empty((M, k), dtype=torch.float32, device=dev)
    idx = torch.empty((M, k), dtype=torch.int32, device=dev)
    L.check(L.load().fp_rerank_topk(L.ptr(Q), L.ptr(qinv), M, D, L.ptr(cand), pool, L.ptr(src) if rows is None else None,
                                    None if rows is None else L.ptr(src), L.ptr(ginv), ginv.shape[0], k, L.ptr(scores),
                                    L.ptr(idx), L.current_stream(dev)), "fp_rerank_topk")
    return scores, idx


VOTE_MODES = {"top1": 0, "majority": 1}


def topk_vote(scores, idx, labels, tau, vote="top1"):
    """scores / idx (M, k) of cosine_topk, labels (N,) int32 per gallery row -> label (M,) int32 (-1: nobody), score (M,),
    votes (M,) int32.  top1: the best candidate's label if its score >= tau.  majority: the label with the most candidates
    >= tau; ties to the larger summed score, then the smaller label."""
    if vote not in VOTE_MODES:
        raise ValueError(f"vote must be one of {sorted(VOTE_MODES)}, got {vote!r}")
    scores, idx, labels = scores.contiguous(), idx.contiguous(), labels.contiguous()
    assert scores.dtype == torch.float32 and idx.dtype == torch.int32 and labels.dtype == torch.int32
    M, k = scores.shape
    dev = scores.device
    label = torch.empty((M,), dtype=torch.int32, device=dev)
    score = torch.empty((M,), dtype=torch.float32, device=dev)
    votes = torch.empty((M,), dtype=torch.int32, device=dev)
    L.check(L.load().fp_topk_vote(L.ptr(scores), L.ptr(idx), M, k, L.ptr(labels), labels.shape[0], float(tau),
                                  VOTE_MODES[vote], L.ptr(label), L.ptr(score), L.ptr(votes), L.current_stream(dev)),
            "fp_topk_vote")
    return label, score, votes


def l2_mean_thres(ref):
    """ref (R, D) -> mean (D,), thres (1,) on device (filter_faces_using_reference.py:85-99)."""
    ref = _f32c(ref)
    R, D = ref.shape
    mean = torch.empty((D,), dtype=torch.float32, device=ref.device)
    thres = torch.empty((1,), dtype=torch.float32, device=ref.device)
    L.check(L.load().fp_l2_mean_thres(L.ptr(ref), R, D, L.ptr(mean), L.ptr(thres), L.current_stream(ref.device)),
            "fp_l2_mean_thres")
    return mean, thres


def l2_filter(E, mean, thres):
    """E (M, D), mean (D,), thres (1,) -> dist (M,), keep (M,) bool (filter_faces_using_reference.py:186-189)."""
    E, mean = _f32c(E), _f32c(mean)
    M, D = E.shape
    dist = torch.empty((M,), dtype=torch.float32, device=E.device)
    keep = torch.empty((M,), dtype=torch.uint8, device=E.device)
    L.check(L.load().fp_l2_filter(L.ptr(E), M, D, L.ptr(mean), L.ptr(thres), L.ptr(dist), L.ptr(keep),
                                  L.current_stream(E.device)), "fp_l2_filter")
    return dist, keep.bool()
