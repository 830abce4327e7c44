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
