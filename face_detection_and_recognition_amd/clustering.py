"""Group unlabelled face embeddings by identity: cosine DBSCAN on the device (csrc/cluster.hip).

  dbscan_cosine    — labels, core flags and degrees of the threshold graph  <x_i, x_j> / (|x_i| |x_j|) >= tau
  cluster_summary  — size, centroid and medoid of every cluster

Build-defined: the reference has no counterpart.  On the same edge set the labels equal scikit-learn's
DBSCAN(metric="precomputed").labels_.
"""
import torch

from . import _lib as L
from . import similarity as S


def _features(X):
    if not isinstance(X, torch.Tensor) or X.dim() != 2:
        raise ValueError(f"X must be an (N, D) tensor, got {type(X).__name__} {tuple(getattr(X, 'shape', ()))}")
    if not X.is_cuda or X.dtype != torch.float32:
        raise ValueError(f"X must be a float32 tensor on the device, got {X.dtype} on {X.device}")
    if X.shape[1] == 0:
        raise ValueError("X has no features")
    return X.contiguous()


def _sanitised_inv(X, xinv):
    xinv = S.row_inv_norm(X) if xinv is None else xinv
    if xinv.dtype != torch.float32 or xinv.shape != (X.shape[0],) or xinv.device != X.device:
        raise ValueError(f"xinv must be {X.shape[0]} float32 values on {X.device}")
    return torch.where(torch.isfinite(xinv), xinv, torch.zeros_like(xinv)).contiguous()


def dbscan_cosine(X, tau, min_samples=1, xinv=None, x3=None):
    """X (N, D) fp32 on the device -> dict(labels (N,) int32, core (N,) bool, degree (N,) int32, n_clusters (1,) int32), all
    device tensors.  i ~ j iff the cosine of rows i and j is >= tau (split bf16 arithmetic of cosine_topk; every pair is
    decided once); degree counts the point itself; core = degree >= min_samples (1 .. 64); clusters are the components of the
    core points, numbered by their smallest row; a non-core point with a core neighbour takes the smallest cluster number
    among its core neighbours; everything else, and every row whose norm is zero or not finite, is noise (-1).  The result is
    deterministic.  min_samples = 1: the connected components of the threshold graph.  xinv / x3: the inverse row norms and
    split3_rows of the (padded) rows, computed here when not passed in."""
    X = _features(X)
    min_samples = int(min_samples)
    if not 1 <= min_samples <= L.DBSCAN_MAX_MIN_SAMPLES:
        raise ValueError(f"min_samples must be in 1 .. {L.DBSCAN_MAX_MIN_SAMPLES}, got {min_samples}")
    tau = float(tau)
    N, dev = X.shape[0], X.device
    degree = torch.empty((N,), dtype=torch.int32, device=dev)
    core = torch.empty((N,), dtype=torch.uint8, device=dev)
    labels = torch.empty((N,), dtype=torch.int32, device=dev)
    n_clusters = torch.zeros((1,), dtype=torch.int32, device=dev)
    if N == 0:
        return dict(labels=labels, core=core.bool(), degree=degree, n_clusters=n_clusters)
    X = S.pad_features(X)
    xinv = _sanitised_inv(X, xinv)
    x3 = S.split3_rows(X) if x3 is None else x3
    lib = L.load()
    ws_bytes = lib.fp_cosine_dbscan_workspace(N, min_samples)
    ws = torch.empty((max(ws_bytes, 16) + 15) // 16 * 2, dtype=torch.int64, device=dev)
    L.check(lib.fp_cosine_dbscan_x6(L.ptr(X), L.ptr(xinv), L.ptr(x3), N, X.shape[1], tau, min_samples, L.ptr(degree), L.ptr(core),
                                    L.ptr(labels), L.ptr(n_clusters), L.ptr(ws), ws.numel() * 8, L.current_stream(dev)),
            "fp_cosine_dbscan_x6")
    return dict(labels=labels, core=core.bool(), degree=degree, n_clusters=n_clusters)


def cluster_summary(X, labels):
    """X (N, D) fp32, labels (N,) integer (-1 = noise) -> dict(sizes (C,) int64, centroids (C, D) fp32, medoid (C,) int32)
    with C = labels.max() + 1.  A centroid is the renormalised sum of its members' normalised rows, in row order; the medoid
    is the member closest to it (cosine; the lower row on equal scores).  Deterministic."""
    X = _features(X)
    N, D = X.shape
    dev = X.device
    if not isinstance(labels, torch.Tensor) or labels.shape != (N,) or labels.is_floating_point():
        raise ValueError(f"labels must be {N} integers, one per row of X")
    labels = labels.to(dev, torch.int64)
    C = int(labels.max().item()) + 1 if N else 0
    C = max(C, 0)
    if N and int(labels.min().item()) < -1:
        raise ValueError("labels must be >= -1")
    centroids = torch.zeros((C, D), dtype=torch.float32, device=dev)
    medoid = torch.full((C,), -1, dtype=torch.int32, device=dev)
    sizes = torch.bincount(labels[labels >= 0], minlength=C) if C else torch.zeros((0,), dtype=torch.int64, device=dev)
    if C == 0:
        return dict(sizes=sizes, centroids=centroids, medoid=medoid)
    # members sorted by (label, row): a stable sort of the labels keeps the rows of one label ascending; noise first
    _, order = torch.sort(labels, stable=True)
    order = order[N - int(sizes.sum().item()):].to(torch.int32).contiguous()
    offsets = torch.zeros((C + 1,), dtype=torch.int32, device=dev)
    offsets[1:] = torch.cumsum(sizes, 0).to(torch.int32)
    xinv = _sanitised_inv(X, None)
    L.check(L.load().fp_cluster_centroids(L.ptr(X), L.ptr(xinv), L.ptr(order), L.ptr(offsets), C, D, L.ptr(centroids),
                                          L.ptr(medoid), L.current_stream(dev)), "fp_cluster_centroids")
    return dict(sizes=sizes, centroids=centroids, medoid=medoid)
