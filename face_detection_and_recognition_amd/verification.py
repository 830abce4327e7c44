"""Score an embedder on labelled faces: verification over ALL pairs, and closed-set identification (csrc/pairhist.hip).

  pair_histogram        — genuine / impostor histograms of the cosine scores of all pairs of live rows, on the device
  pair_histogram_numpy  — the same in fp64 on the host: the yardstick, and the path without a GPU
  verification_report   — ROC, AUC, EER, best accuracy and TAR at FAR from the 2 x nbins integers (host, fp64)
  identification_rates  — closed-set rank-1 .. rank-k identification rates (CMC) on top of similarity.cosine_topk

Build-defined: the reference has no counterpart.  A row is live when its norm is finite and non-zero and its label
is >= 0; bin b of nbins over [lo, hi) takes t = (s - lo) * (nbins / (hi - lo)), b = 0 for t < 0, else min(int(t), nbins - 1).
"""
import numpy as np
import torch

from . import _lib as L
from . import similarity as S
from .clustering import _features, _sanitised_inv


def _bins(lo, hi, nbins):
    lo, hi, nbins = float(lo), float(hi), int(nbins)
    if not 2 <= nbins <= L.PAIRHIST_MAX_BINS:
        raise ValueError(f"nbins must be in 2 .. {L.PAIRHIST_MAX_BINS}, got {nbins}")
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise ValueError(f"lo < hi, both finite, got lo = {lo}, hi = {hi}")
    return lo, hi, nbins


def bin_edges(lo, hi, nbins):
    """The nbins + 1 edges in fp64: edge b = lo + (hi - lo) b / nbins, the last one hi itself."""
    lo, hi, nbins = _bins(lo, hi, nbins)
    e = lo + (hi - lo) * np.arange(nbins + 1, dtype=np.float64) / nbins
    e[-1] = hi
    return e


def _labels(labels, N):
    if not isinstance(labels, torch.Tensor) or labels.shape != (N,) or labels.is_floating_point() or labels.dtype == torch.bool:
        raise ValueError(f"labels must be {N} integers, one per row of X")
    return labels


def pair_histogram(X, labels, lo=-1.0, hi=1.0, nbins=1024, xinv=None, x3=None):
    """X (N, D) fp32 on the device, labels (N,) integers -> dict(genuine, impostor: (nbins,) int64 device tensors, edges:
    (nbins + 1,) float64 numpy).  Every pair i < j of live rows is scored once (split bf16 arithmetic of cosine_topk and
    dbscan_cosine) and counted into genuine (same label) or impostor; scores below lo / at or above hi land in the end bins,
    so the counts total the live pairs.  Rows whose norm is zero or not finite, and rows with a label < 0, take part in no
    pair.  Deterministic.  xinv / x3: the inverse row norms and split3_rows of the (padded) rows, computed here when not
    passed in."""
    lo, hi, nbins = _bins(lo, hi, nbins)
    if not isinstance(X, torch.Tensor) or X.dim() != 2:
        raise ValueError(f"X must be an (N, D) tensor, got {type(X).__name__} {tuple(getattr(X, 'shape', ()))}")
    labels = _labels(labels, X.shape[0])
    X = _features(X)
    N, dev = X.shape[0], X.device
    if N and (int(labels.max().item()) >= 2 ** 31 or int(labels.min().item()) < -2 ** 31):
        raise ValueError("labels must fit in int32")
    labels = labels.to(dev, torch.int32).contiguous()
    genuine = torch.empty((nbins,), dtype=torch.int64, device=dev)
    impostor = torch.empty((nbins,), dtype=torch.int64, device=dev)
    lib = L.load()
    if N:
        X = S.pad_features(X)
        xinv = _sanitised_inv(X, xinv)
        x3 = S.split3_rows(X) if x3 is None else x3
    ws_bytes = lib.fp_pair_histogram_workspace(N)
    ws = torch.empty((max(ws_bytes, 16) + 15) // 16 * 2, dtype=torch.int64, device=dev)
    L.check(lib.fp_pair_histogram_x6(L.ptr(X) if N else None, L.ptr(xinv) if N else None, L.ptr(x3) if N else None,
                                     L.ptr(labels) if N else None, N, X.shape[1] if N else 32, lo, hi, nbins, L.ptr(genuine),
                                     L.ptr(impostor), L.ptr(ws), ws.numel() * 8, L.current_stream(dev)), "fp_pair_histogram_x6")
    return dict(genuine=genuine, impostor=impostor, edges=bin_edges(lo, hi, nbins))


def live_rows(X, labels):
    """numpy: the rows pair_histogram counts -- norm (fp64 of the fp32 rows) finite and non-zero, label >= 0."""
    X = np.asarray(X, np.float64)
    with np.errstate(all="ignore"):
        n = np.sqrt((X * X).sum(1))
    return np.isfinite(n) & (n > 0) & (np.asarray(labels) >= 0)


def pair_histogram_numpy(X, labels, lo=-1.0, hi=1.0, nbins=1024, block=512):
    """The restatement in fp64 on the host: X (N, D) array, labels (N,) integers -> dict(genuine, impostor (nbins,) int64
    numpy, edges).  Same liveness and bin rule as pair_histogram, scores in fp64; row blocks of `block` rows."""
    lo, hi, nbins = _bins(lo, hi, nbins)
    X = np.asarray(X, np.float64)
    labels = np.asarray(labels)
    if X.ndim != 2 or labels.shape != (X.shape[0],) or labels.dtype.kind not in "iu":
        raise ValueError(f"X must be (N, D) and labels N integers, got {X.shape} and {labels.dtype} {labels.shape}")
    live = live_rows(X, labels)
    Xl, ll = X[live], labels[live].astype(np.int64)
    Xn = Xl / np.sqrt((Xl * Xl).sum(1))[:, None] if len(Xl) else Xl
    n = Xn.shape[0]
    scale = nbins / (hi - lo)
    out = np.zeros((2, nbins), np.int64)
    for r0 in range(0, n, block):
        r1 = min(n, r0 + block)
        s = Xn[r0:r1] @ Xn[r0:].T                                   # columns r0 .. n
        up = np.arange(r0, n)[None, :] > np.arange(r0, r1)[:, None]
        with np.errstate(invalid="ignore"):
            t = (s - lo) * scale
            b = np.where(t < 0, 0, np.minimum(np.nan_to_num(t, nan=0.0, posinf=nbins, neginf=0.0), nbins - 1)).astype(np.int64)
        ok = up & ~np.isnan(s)
        same = ll[r0:r1, None] == ll[None, r0:]
        out[0] += np.bincount(b[ok & same], minlength=nbins)
        out[1] += np.bincount(b[ok & ~same], minlength=nbins)
    return dict(genuine=out[0], impostor=out[1], edges=bin_edges(lo, hi, nbins))


def _host(a):
    return (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).astype(np.int64)


def verification_report(genuine, impostor, edges, fars=(1e-1, 1e-2, 1e-3, 1e-4)):
    """The two histograms and their nbins + 1 edges -> the verification figures, in numpy fp64.  At threshold e_b (accept a
    pair when its score >= e_b; b = 0 .. nbins) TA_b = sum genuine[b:], FA_b = sum impostor[b:], TAR = TA / G, FAR = FA / I,
    FRR = 1 - TAR.  Returns dict(
      n_genuine, n_impostor, thresholds, tar, far (nbins + 1 each),
      auc            trapezoid over the (FAR, TAR) points,
      eer, eer_threshold   b* = the smallest b with FAR_b <= FRR_b, linear interpolation of FAR - FRR between b* - 1 and b*,
      best_accuracy, best_threshold   the first b maximising (TA_b + I - FA_b) / (G + I),
      tar_at_far     {f: dict(tar, threshold, far) at the smallest b with FAR_b <= f, or None when f < 1 / I}).
    With an empty class the rates that need it are NaN; nothing raises."""
    g, i = _host(genuine), _host(impostor)
    edges = np.asarray(edges, np.float64)
    if g.ndim != 1 or g.shape != i.shape or edges.shape != (g.shape[0] + 1,):
        raise ValueError(f"genuine and impostor must be (nbins,) and edges (nbins + 1,), got {g.shape}, {i.shape}, {edges.shape}")
    G, I = int(g.sum()), int(i.sum())
    ta = np.concatenate([np.cumsum(g[::-1])[::-1], [0]]).astype(np.float64)
    fa = np.concatenate([np.cumsum(i[::-1])[::-1], [0]]).astype(np.float64)
    nan = float("nan")
    tar = ta / G if G else np.full_like(ta, nan)
    far = fa / I if I else np.full_like(fa, nan)
    out = dict(n_genuine=G, n_impostor=I, thresholds=edges, tar=tar, far=far, auc=nan, eer=nan, eer_threshold=nan,
               best_accuracy=nan, best_threshold=nan, tar_at_far={float(f): None for f in fars})
    if G + I:
        acc = (ta + I - fa) / (G + I)
        b = int(np.argmax(acc))                                      # the first maximum
        out["best_accuracy"], out["best_threshold"] = float(acc[b]), float(edges[b])
    if not (G and I):
        return out
    out["auc"] = float(np.sum((far[:-1] - far[1:]) * (tar[:-1] + tar[1:]) * 0.5))     # FAR falls with b
    frr = 1.0 - tar
    d = far - frr                                                    # non-increasing, d[0] = 1, d[nbins] = -1
    bs = int(np.argmax(d <= 0))
    if bs == 0 or d[bs - 1] == d[bs]:
        w = 1.0
    else:
        w = d[bs - 1] / (d[bs - 1] - d[bs])                          # the zero of d between b* - 1 and b*
    a = max(bs - 1, 0)
    out["eer"] = float(far[a] + w * (far[bs] - far[a]))
    out["eer_threshold"] = float(edges[a] + w * (edges[bs] - edges[a]))
    for f in fars:
        f = float(f)
        if f < 1.0 / I:
            continue
        b = int(np.argmax(far <= f))
        out["tar_at_far"][f] = dict(tar=float(tar[b]), threshold=float(edges[b]), far=float(far[b]))
    return out


def cmc_counts(top_idx, q_labels, g_labels):
    """The counting half of identification_rates, on tensors of any device: top_idx (M, k) gallery rows (-1 = no candidate),
    q_labels (M,), g_labels (N,) integers -> (hits (k,) int64: mated probes whose first r candidates hold a gallery row of
    their label, n_mated).  A probe is mated when its label is >= 0 and some gallery row carries it."""
    top_idx, q_labels, g_labels = top_idx.to(torch.int64), q_labels.to(torch.int64), g_labels.to(torch.int64)
    M, k = top_idx.shape
    if q_labels.shape != (M,) or g_labels.dim() != 1:
        raise ValueError(f"q_labels must be {M} integers and g_labels one per gallery row")
    if M == 0 or g_labels.numel() == 0:
        return torch.zeros((k,), dtype=torch.int64, device=top_idx.device), 0
    mated = (q_labels >= 0) & torch.isin(q_labels, g_labels)
    cand = g_labels[top_idx.clamp(min=0)]
    hit = (cand == q_labels[:, None]) & (top_idx >= 0) & mated[:, None]
    within = torch.cummax(hit.to(torch.int64), dim=1).values         # 1 from the first hit on
    return within.sum(0), int(mated.sum().item())


def identification_rates(Q, q_labels, G_or_gallery, g_labels=None, k=5):
    """Closed-set identification: Q (M, D) probes and their labels against a gallery -- a (N, D) tensor with g_labels, or a
    FaceGallery (its own labels) -> dict(rate (k,) float64 numpy, hits (k,) int64, n_mated).  rate[r - 1] is the share of
    mated probes whose first r candidates of cosine_topk contain a gallery row of their label (CMC); 1 <= k <= 16.  NaN rates
    when no probe is mated."""
    k = int(k)
    if not 1 <= k <= L.TOPK_MAX:
        raise ValueError(f"k must be in 1 .. {L.TOPK_MAX}, got {k}")
    Q = _features(Q)
    if hasattr(G_or_gallery, "search"):
        gal = G_or_gallery
        _, idx = gal.search(Q, k)
        g_labels = gal.labels if g_labels is None else g_labels
    else:
        G = _features(G_or_gallery)
        if g_labels is None:
            raise ValueError("g_labels is required with a gallery tensor")
        _, idx = S.cosine_topk(Q, G, k)
    q_labels = _labels(q_labels, Q.shape[0]).to(Q.device)
    g_labels = g_labels.to(Q.device)
    hits, n_mated = cmc_counts(idx, q_labels, g_labels)
    hits = hits.cpu().numpy()
    rate = hits / n_mated if n_mated else np.full((k,), np.nan)
    return dict(rate=np.asarray(rate, np.float64), hits=hits, n_mated=n_mated)
