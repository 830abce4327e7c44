"""An enrolled gallery of face embeddings and the recognition question asked of it: who is this, out of everyone enrolled,
with the runner-up candidates (similarity.cosine_topk + similarity.topk_vote, csrc/sim.hip).

Build-defined: the reference stops at the single best cosine score per face; nothing in it searches a gallery.
FaceGallery.from_clusters enrols what clustering.dbscan_cosine found in unlabelled embeddings.
"""
import glob
import os

import numpy as np
import torch

from . import similarity as S


class FaceGallery:
    """embeddings (N, D) fp32, labels: one int32 identity id per row, names: {id: str} (optional), device: a HIP device.

    Everything the search needs is computed once, here: the inverse row norms, the copy zero-padded to a multiple of 32
    features and its three bf16 planes (similarity.split3_rows).  A row whose norm is zero or not finite can never be
    returned (its inverse norm is stored as 0, the library's mask for padding and removed rows)."""

    def __init__(self, embeddings, labels, names=None, device=None):
        if device is None:
            device = embeddings.device if isinstance(embeddings, torch.Tensor) and embeddings.is_cuda else "cuda"
        self.device = torch.device(str(device).replace("hip", "cuda"))
        self.names = {int(k): str(v) for k, v in (names or {}).items()}
        self._set(torch.as_tensor(embeddings), torch.as_tensor(labels))

    def _set(self, emb, labels):
        emb = emb.to(self.device, torch.float32).contiguous()
        labels = labels.to(self.device, torch.int32).contiguous().reshape(-1)
        if emb.dim() != 2 or emb.shape[0] == 0:
            raise ValueError(f"a gallery needs (N, D) embeddings with N > 0, got {tuple(emb.shape)}")
        if labels.shape[0] != emb.shape[0]:
            raise ValueError(f"{labels.shape[0]} labels for {emb.shape[0]} embeddings")
        self.embeddings, self.labels = emb, labels
        padded = S.pad_features(emb)
        ginv = S.row_inv_norm(padded)
        self.ginv = torch.where(torch.isfinite(ginv), ginv, torch.zeros_like(ginv))
        self.g3 = S.split3_rows(padded)

    def __len__(self):
        return self.embeddings.shape[0]

    @property
    def dim(self):
        return self.embeddings.shape[1]

    # -- search --------------------------------------------------------------------------------------
    def search(self, Q, k, n_splits=0):
        """Q (M, D) -> scores (M, k) descending, idx (M, k) int32 gallery rows (similarity.cosine_topk): lower row first on
        equal scores, removed rows never, -inf / -1 beyond the live rows."""
        if Q.shape[1] != self.dim:
            raise ValueError(f"queries have {Q.shape[1]} features, the gallery {self.dim}")
        return S.cosine_topk(Q.to(self.device), None, k, ginv=self.ginv, g3=self.g3, n_splits=n_splits)

    def identify(self, Q, k=5, tau=0.3, vote="top1"):
        """Who is each row of Q?  dict(label (M,) int32, -1 = nobody enrolled scores >= tau; score (M,); votes (M,) int32;
        top_scores (M, k); top_idx (M, k)), all device tensors (similarity.topk_vote for the vote rules)."""
        top_scores, top_idx = self.search(Q, k)
        label, score, votes = S.topk_vote(top_scores, top_idx, self.labels, tau, vote)
        return dict(label=label, score=score, votes=votes, top_scores=top_scores, top_idx=top_idx)

    def name_of(self, label):
        label = int(label)
        return "unknown" if label < 0 else self.names.get(label, str(label))

    # -- enrolment -----------------------------------------------------------------------------------
    def add(self, embeddings, labels, names=None):
        """Append rows.  The bf16 plane layout is NOT appendable (planes are [D / 32][3][round_up(N, 128)][32]: a new row
        moves every plane), so this rebuilds norms, padded copy and planes of the whole gallery; enrol in batches.  Rows
        removed before stay removed."""
        dead = self.ginv == 0
        emb = torch.cat([self.embeddings, torch.as_tensor(embeddings).to(self.device, torch.float32).reshape(-1, self.dim)])
        lab = torch.cat([self.labels, torch.as_tensor(labels).to(self.device, torch.int32).reshape(-1)])
        self.names.update({int(k): str(v) for k, v in (names or {}).items()})
        self._set(emb, lab)
        self.ginv[:dead.shape[0]][dead] = 0

    def remove(self, mask):
        """mask (N,) bool: those rows are never returned again (their inverse norm becomes 0; nothing is moved)."""
        mask = torch.as_tensor(mask).to(self.device, torch.bool).reshape(-1)
        if mask.shape[0] != len(self):
            raise ValueError(f"mask of {mask.shape[0]} for {len(self)} rows")
        self.ginv[mask] = 0

    # -- files ---------------------------------------------------------------------------------------
    def save(self, path):
        """One .npz: embeddings (fp32), labels (int32), the names as two arrays (ids, strings), and the removed-row mask."""
        ids = np.array(sorted(self.names), dtype=np.int32)
        np.savez(path, embeddings=self.embeddings.cpu().numpy(), labels=self.labels.cpu().numpy(), name_ids=ids,
                 name_strs=np.array([self.names[int(i)] for i in ids], dtype=np.str_),
                 removed=(self.ginv == 0).cpu().numpy())
        return path

    @classmethod
    def load(cls, path, device="cuda"):
        with np.load(path, allow_pickle=False) as z:
            g = cls(z["embeddings"], z["labels"], dict(zip(z["name_ids"].tolist(), z["name_strs"].tolist())), device)
            if "removed" in z.files:
                g.remove(z["removed"])
        return g

    def compress(self, rows="device"):
        """The same rows, labels, names and removed rows as a CompressedGallery (rows: where its fp32 rows live)."""
        g = CompressedGallery(self.embeddings, self.labels, self.names, self.device, rows=rows)
        g.remove(self.ginv == 0)
        return g

    @classmethod
    def from_clusters(cls, embeddings, labels, names=None, device=None, centroids_only=False):
        """Enrol the outcome of clustering.dbscan_cosine: every row whose label is >= 0 under its cluster number (noise, -1,
        is left out), names `cluster_0007` unless given.  centroids_only: one row per cluster instead, its centroid
        (clustering.cluster_summary)."""
        emb, lab = torch.as_tensor(embeddings), torch.as_tensor(labels).reshape(-1)
        if emb.dim() != 2 or lab.shape[0] != emb.shape[0]:
            raise ValueError(f"{lab.shape[0]} labels for embeddings of shape {tuple(emb.shape)}")
        if lab.is_floating_point() or lab.dtype == torch.bool:
            raise ValueError(f"cluster labels must be integers, got {lab.dtype}")
        keep = lab >= 0
        if not bool(keep.any()):
            raise ValueError("no clustered rows: every label is noise (-1)")
        n_clusters = int(lab.max()) + 1
        if names is None:
            names = {c: f"cluster_{c:04d}" for c in range(n_clusters)}
        if not centroids_only:
            return cls(emb[keep.to(emb.device)], lab[keep], names, device)
        from .clustering import cluster_summary
        if device is None:
            device = emb.device if emb.is_cuda else "cuda"
        device = torch.device(str(device).replace("hip", "cuda"))
        summ = cluster_summary(emb.to(device, torch.float32), lab.to(device))
        present = summ["sizes"] > 0
        return cls(summ["centroids"][present], torch.arange(n_clusters, device=device)[present], names, device)

    @classmethod
    def from_feature_files(cls, paths_or_dir, feature_size, device="cuda"):
        """Enrol from the .npy annotation dicts face_extraction.save_extracted_faces writes: `feature` reshaped to rows of
        feature_size (all-zero rows are its padding and are dropped), every row under the file's `label`, names from
        `class_name`.  paths_or_dir: a directory (searched recursively for .npy) or a list of files."""
        if isinstance(paths_or_dir, (str, os.PathLike)):
            paths = sorted(glob.glob(os.path.join(str(paths_or_dir), "**", "*.npy"), recursive=True))
        else:
            paths = [str(p) for p in paths_or_dir]
        feats, labels, names = [], [], {}
        for p in paths:
            annot = np.load(p, allow_pickle=True).item()
            f = np.asarray(annot["feature"], np.float32).reshape(-1, int(feature_size))
            f = f[np.any(f != 0, axis=1)]
            feats.append(f)
            labels.append(np.full((f.shape[0],), int(annot["label"]), np.int32))
            names[int(annot["label"])] = str(annot["class_name"])
        if not feats or sum(len(f) for f in feats) == 0:
            raise ValueError(f"no face features under {paths_or_dir!r}")
        return cls(np.concatenate(feats), np.concatenate(labels), names, device)


class CompressedGallery:
    """The gallery for row counts that do not fit as FaceGallery keeps them (10 bytes per feature): per enrolled row one int8
    code per feature (zero-padded to a multiple of 64, at most 1024), and 12 bytes of weight, inverse norm and scale
    (similarity.quantize_rows_i8).  search is two stages: a coarse pass over every row on the i8 matrix cores that keeps `pool`
    candidates per query (similarity.cosine_topk_i8), then the exact fp32 cosine of those candidates and the k best of them
    (similarity.rerank_topk).  Same interface as FaceGallery; FacePipeline(gallery=) takes either.

    rows: where the fp32 rows of the rerank live.
      "device"  on the device beside the codes (4 more bytes per feature).
      "host"    in pinned host memory: search reads the candidate indices back, gathers M x pool rows on the host, uploads
                them and reranks that compact block.  THIS SYNCHRONISES the stream, once per search.
      None      nowhere: search returns the best k of the coarse list with the COARSE scores, which are approximate (int8
                codes on both sides); such a gallery cannot add rows or be saved.
    Building uploads all fp32 rows once, whatever `rows` says; they are dropped or moved afterwards."""

    ROWS = ("device", "host", None)

    def __init__(self, embeddings, labels, names=None, device=None, rows="device"):
        if rows not in self.ROWS:
            raise ValueError(f"rows must be one of {self.ROWS}, got {rows!r}")
        if device is None:
            device = embeddings.device if isinstance(embeddings, torch.Tensor) and embeddings.is_cuda else "cuda"
        self.device = torch.device(str(device).replace("hip", "cuda"))
        self.rows_where = rows
        self.names = {int(k): str(v) for k, v in (names or {}).items()}
        emb, labels = torch.as_tensor(embeddings), torch.as_tensor(labels).reshape(-1)
        if emb.dim() != 2 or emb.shape[0] == 0:
            raise ValueError(f"a gallery needs (N, D) embeddings with N > 0, got {tuple(emb.shape)}")
        if labels.shape[0] != emb.shape[0]:
            raise ValueError(f"{labels.shape[0]} labels for {emb.shape[0]} embeddings")
        if (emb.shape[1] + 63) // 64 * 64 > S.L.QUANT_MAX_D:
            raise ValueError(f"{emb.shape[1]} features: a compressed gallery takes at most {S.L.QUANT_MAX_D}")
        self._set(emb, labels)

    def _set(self, emb, labels):
        self._dim = emb.shape[1]
        padded = S.pad_features64(emb.to(self.device, torch.float32).contiguous())
        self.labels = labels.to(self.device, torch.int32).contiguous()
        ginv = S.row_inv_norm(padded)
        self.g8, self.scale = S.quantize_rows_i8(padded)
        live = torch.isfinite(ginv) & (self.scale > 0)
        self.ginv = torch.where(live, ginv, torch.zeros_like(ginv))
        self.w = self.scale * self.ginv                   # one rounding; 0 for dead rows
        if self.rows_where == "device":
            self.rows = padded
        elif self.rows_where == "host":
            self.rows = padded.cpu().pin_memory()
        else:
            self.rows = None

    def __len__(self):
        return self.labels.shape[0]

    @property
    def dim(self):
        return self._dim

    @property
    def embeddings(self):
        """The fp32 rows (N, D), where they live; a coarse-only gallery has none."""
        if self.rows is None:
            raise ValueError("a coarse-only gallery (rows=None) holds no fp32 rows")
        return self.rows[:, :self._dim]

    def device_bytes(self):
        """Bytes this gallery holds on the device: codes, weight, inverse norm, scale, labels, and the fp32 rows if they are there."""
        held = [self.g8, self.w, self.ginv, self.scale, self.labels] + ([self.rows] if self.rows_where == "device" else [])
        return sum(t.numel() * t.element_size() for t in held)

    # -- search --------------------------------------------------------------------------------------
    def coarse(self, Q, pool, n_splits=0):
        """The first stage alone: padded queries, their inverse norms, coarse scores (M, pool) and candidate rows (M, pool)."""
        if Q.shape[1] != self.dim:
            raise ValueError(f"queries have {Q.shape[1]} features, the gallery {self.dim}")
        Qp = S.pad_features64(Q.to(self.device, torch.float32).contiguous())
        qinv = S.row_inv_norm(Qp)
        qinv = torch.where(torch.isfinite(qinv), qinv, torch.zeros_like(qinv))
        qq, sq = S.quantize_rows_i8(Qp)
        cs, ci = S.cosine_topk_i8(qq, sq * qinv, self.g8, self.w, len(self), pool, n_splits)
        return Qp, qinv, cs, ci

    def search(self, Q, k, pool=None, n_splits=0):
        """Q (M, D) -> scores (M, k) descending, idx (M, k) int32 gallery rows, as FaceGallery.search: exact fp32 scores of
        the best k among the `pool` coarse candidates (default min(64, 4 k); k <= pool <= 64), lower row first on equal
        scores, removed rows never, -inf / -1 beyond the live rows.  A true neighbour the coarse pass ranks below `pool` is
        missed: pool is the recall knob.  rows="host": synchronises (class docstring).  rows=None: coarse scores, approximate."""
        k = int(k)
        pool = min(S.L.COARSE_MAX, 4 * k) if pool is None else int(pool)
        if not 1 <= k <= S.L.TOPK_MAX:
            raise ValueError(f"k must be 1 .. {S.L.TOPK_MAX}, got {k}")
        if not k <= pool <= S.L.COARSE_MAX:
            raise ValueError(f"pool must be k .. {S.L.COARSE_MAX}, got {pool} at k = {k}")
        Qp, qinv, cs, ci = self.coarse(Q, pool, n_splits)
        if self.rows_where is None:
            return cs[:, :k].contiguous(), ci[:, :k].contiguous()
        if self.rows_where == "device":
            return S.rerank_topk(Qp, ci, k, G=self.rows, ginv=self.ginv, qinv=qinv)
        cand = ci.cpu().to(torch.int64).clamp_(min=0).reshape(-1)      # the synchronisation; -1 gathers row 0, which the kernel skips
        block = torch.empty((cand.shape[0], self.rows.shape[1]), dtype=torch.float32).pin_memory()
        torch.index_select(self.rows, 0, cand, out=block)
        block = block.to(self.device, non_blocking=True).reshape(ci.shape[0], pool, -1)
        return S.rerank_topk(Qp, ci, k, rows=block, ginv=self.ginv, qinv=qinv)

    def identify(self, Q, k=5, tau=0.3, vote="top1", pool=None):
        """As FaceGallery.identify, on search(Q, k, pool)."""
        top_scores, top_idx = self.search(Q, k, pool)
        label, score, votes = S.topk_vote(top_scores, top_idx, self.labels, tau, vote)
        return dict(label=label, score=score, votes=votes, top_scores=top_scores, top_idx=top_idx)

    def name_of(self, label):
        label = int(label)
        return "unknown" if label < 0 else self.names.get(label, str(label))

    # -- enrolment -----------------------------------------------------------------------------------
    def add(self, embeddings, labels, names=None):
        """Append rows.  The staged code layout is no more appendable than FaceGallery's planes: this rebuilds codes, norms
        and weights of the whole gallery from the fp32 rows (not possible with rows=None).  Rows removed before stay removed."""
        old = self.embeddings
        dead = self.ginv == 0
        new = torch.as_tensor(embeddings).to(old.device, torch.float32).reshape(-1, self.dim)
        lab = torch.cat([self.labels, torch.as_tensor(labels).to(self.device, torch.int32).reshape(-1)])
        if lab.shape[0] != old.shape[0] + new.shape[0]:
            raise ValueError(f"{lab.shape[0] - old.shape[0]} labels for {new.shape[0]} embeddings")
        self.names.update({int(k): str(v) for k, v in (names or {}).items()})
        self._set(torch.cat([old, new]), lab)
        self.ginv[:dead.shape[0]][dead] = 0
        self.w[:dead.shape[0]][dead] = 0

    def remove(self, mask):
        """mask (N,) bool: those rows are never returned again (their weight and inverse norm become 0; nothing is moved)."""
        mask = torch.as_tensor(mask).to(self.device, torch.bool).reshape(-1)
        if mask.shape[0] != len(self):
            raise ValueError(f"mask of {mask.shape[0]} for {len(self)} rows")
        self.ginv[mask] = 0
        self.w[mask] = 0

    # -- files ---------------------------------------------------------------------------------------
    def save(self, path):
        """The .npz of FaceGallery.save, field for field: either class loads the other's file (not possible with rows=None)."""
        ids = np.array(sorted(self.names), dtype=np.int32)
        np.savez(path, embeddings=self.embeddings.cpu().numpy(), labels=self.labels.cpu().numpy(), name_ids=ids,
                 name_strs=np.array([self.names[int(i)] for i in ids], dtype=np.str_),
                 removed=(self.ginv == 0).cpu().numpy())
        return path

    @classmethod
    def load(cls, path, device="cuda", rows="device"):
        with np.load(path, allow_pickle=False) as z:
            g = cls(z["embeddings"], z["labels"], dict(zip(z["name_ids"].tolist(), z["name_strs"].tolist())), device, rows=rows)
            if "removed" in z.files:
                g.remove(z["removed"])
        return g
