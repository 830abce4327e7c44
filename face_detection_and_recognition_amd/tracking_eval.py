"""Score a tracker against ground truth: CLEAR-MOT (MOTA, MOTP, identity switches, fragmentations, MT / PT / ML) and the
identity measures (IDF1, IDP, IDR), for one class without ignore regions.

The reference calls no tracking scorer, so this is build-defined in the standing of evaluation.py: the published procedure
restated (DESIGN.md section 7 "Tracker evaluation" and include/facepath.h are the specification; parity with TrackEval /
py-motmetrics is unpinned, neither is installed) three times:

  * ``device=None`` / ``"cpu"``: plain numpy, fp64, a Python loop over the frames, the assignment vectorised over columns
    only -- the oracle, and the path for a machine without a GPU;
  * a HIP device: fp_mot_match (csrc/moteval.hip), one launch, one workgroup per sequence marching its frames.  The stable
    sort by (sequence, frame), the CSR offsets and the dense ids are torch plumbing;
  * fp_mot_match_emulate: the kernel's decision code serially on host memory (the tests' third witness).

All three give the same integers, the same per-row outputs and a bit-equal sum_iou.  The id assignment behind IDTP runs on
the host (_idtp).  A single long sequence is a chain of dependent frames on one workgroup and is latency-bound; many
sequences fill the device the way many streams fill fp_tracklets_step.

hota_eval scores the same rows with HOTA (DetA, AssA, LocA over a family of localisation thresholds; DESIGN.md section 7
"Tracker evaluation: HOTA"): the same three paths, fp_hota_match (csrc/hota.hip) on the device, everything per threshold
derived on the host.

Thresholds and max_age of tracking.py remain unmeasured on real video until somebody runs this on labelled footage.
"""
import numpy as np
import torch

from . import _lib as L
from .evaluation import _boxes, _iou_matrix

MAX_ROWS = L.MOT_MAX_ROWS
BONUS = 1000.0                       # what the previous frame's partner adds to an admissible pair's score
COUNT_KEYS = ("TP", "FN", "FP", "IDSW", "Frag", "MT", "PT", "ML", "IDTP", "IDFN", "IDFP", "n_gt_ids", "n_hy_ids")
DERIVED_KEYS = ("MOTA", "MOTP", "IDF1", "IDP", "IDR", "precision", "recall")


# ---- the assignment ----------------------------------------------------------------------------------------------------

def _hungarian(cost):
    """Shortest-augmenting-path Hungarian method on an (n, m) fp64 cost matrix with n <= m (the frames' matrices are square),
    exactly as DESIGN section 7 writes it: rows inserted in ascending order, potentials u / v, per step one scan over the
    unused columns (vectorised here), strict comparisons so that the lowest column wins a tie.  -> p (m + 1,): p[j] = the
    row (1-based) assigned to column j (1-based), 0 for none."""
    n, m = cost.shape
    u, v = np.zeros(n + 1), np.zeros(m + 1)
    p, way = np.zeros(m + 1, np.int64), np.zeros(m + 1, np.int64)
    for i in range(1, n + 1):
        p[0] = i
        j0 = 0
        minv = np.full(m + 1, np.inf)
        used = np.zeros(m + 1, bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            free = ~used[1:]
            cur = cost[i0 - 1] - u[i0] - v[1:]
            upd = free & (cur < minv[1:])
            minv[1:][upd] = cur[upd]
            way[1:][upd] = j0
            cand = np.where(free, minv[1:], np.inf)
            j1 = int(np.argmin(cand)) + 1                  # the first minimum: the lowest column
            delta = cand[j1 - 1]
            u[p[used]] += delta
            v[used] -= delta
            minv[~used] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    return p


def assign_max(score):
    """One-to-one assignment of the rows to the columns of an (n, m) fp64 score matrix with the largest total: the matrix
    padded with zeros to N x N, N = max(n, m), C = -score, _hungarian.  -> col (n,): the column of every row, -1 where the
    row went to a padding column."""
    n, m = score.shape
    N = max(n, m)
    col = -np.ones(n, np.int64)
    if n == 0 or m == 0:
        return col
    padded = np.zeros((N, N))
    padded[:n, :m] = score
    p = _hungarian(-padded)
    for j in range(1, m + 1):
        if 1 <= p[j] <= n:
            col[p[j] - 1] = j - 1
    return col


def _components(pot):
    """Connected components of the non-zero pattern of pot (G, H): list of (rows, cols) index arrays."""
    gi, hi = np.nonzero(pot)
    G = pot.shape[0]
    parent = list(range(G + pot.shape[1]))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for g, h in zip(gi.tolist(), hi.tolist()):
        a, b = find(g), find(G + h)
        if a != b:
            parent[b] = a
    groups = {}
    for node in sorted(set(gi.tolist()) | {G + h for h in hi.tolist()}):
        groups.setdefault(find(node), []).append(node)
    return [(np.array([x for x in nodes if x < G], np.int64), np.array([x - G for x in nodes if x >= G], np.int64))
            for nodes in groups.values()]


def _idtp(pot):
    """max over one-to-one assignments of ground-truth ids to hypothesis ids of sum pot[g][h].  pot is split into the
    connected components of its non-zero pattern and each is solved with _hungarian (integers below 2^53 are exact in
    fp64), the smaller side as rows.  Worst case: one component holding every id, O(min(G, H)^2 max(G, H)) operations as
    O(min(G, H)^2) numpy calls of length max(G, H); a tracker that mostly keeps its identities gives components of a handful
    of ids."""
    total = 0
    for rows, cols in _components(pot):
        sub = pot[np.ix_(rows, cols)].astype(np.float64)
        sub = sub.T if sub.shape[0] > sub.shape[1] else sub
        p = _hungarian(-sub)
        j = np.nonzero(p[1:])[0]
        total += int(round(float(sub[p[1:][j] - 1, j].sum())))
    return total


# ---- arguments and plumbing ----------------------------------------------------------------------------------------------

def _ints(x, n, what, dev):
    if isinstance(x, torch.Tensor):
        if x.dtype.is_floating_point or x.dtype == torch.bool:
            raise ValueError(f"{what}: expected integers, got {x.dtype}")
        t = x.detach().to(device=dev, dtype=torch.int64)
    else:
        a = np.asarray(x)
        if a.size == 0:
            a = a.astype(np.int64)
        if a.dtype.kind not in "iu":
            raise ValueError(f"{what}: expected integers, got {a.dtype}")
        t = torch.as_tensor(a.astype(np.int64), device=dev)
    if t.ndim != 1 or (n is not None and t.shape[0] != n):
        raise ValueError(f"{what}: expected shape ({'n' if n is None else n},), got {tuple(t.shape)}")
    return t.contiguous()


def _exclusive(counts):
    off = torch.zeros(counts.shape[0] + 1, dtype=torch.int64, device=counts.device)
    off[1:] = torch.cumsum(counts, 0)
    return off


class _Rows:
    """One row set sorted by (sequence, frame), stable: order (indices into the caller's arrays), boxes (n, 4) fp64, dense
    (n,) int32 ids 0 .. ids_s - 1 inside the row's sequence, off (frames + 1,) int32 CSR over the global frame index,
    n_ids (S,) int64, id_base (S + 1,) int64, ids (sum n_ids,) the caller's ids in (sequence, id) order."""


def _prepare(seq, frame, ids, boxes, n_frames, base, what, dev):
    b = _boxes(boxes, f"{what}_boxes", dev)
    n, S, total = int(b.shape[0]), int(n_frames.shape[0]), int(base[-1])
    s, f, i = _ints(seq, n, f"{what}_seq", dev), _ints(frame, n, f"{what}_frame", dev), _ints(ids, n, f"{what}_id", dev)
    r = _Rows()
    if n == 0:
        r.order = torch.zeros(0, dtype=torch.int64, device=dev)
        r.boxes, r.dense = b, torch.zeros(0, dtype=torch.int32, device=dev)
        r.off = torch.zeros(total + 1, dtype=torch.int32, device=dev)
        r.n_ids, r.ids = torch.zeros(S, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int64, device=dev)
        r.id_base = _exclusive(r.n_ids)
        return r
    if int(s.min()) < 0 or int(s.max()) >= S:
        raise ValueError(f"{what}_seq: sequence outside [0, {S})")
    if int(f.min()) < 0 or bool((f >= n_frames[s]).any()):
        raise ValueError(f"{what}_frame: frame outside [0, n_frames[seq])")
    gf = base[s] + f
    r.order = torch.sort(gf, stable=True).indices
    cnt = torch.bincount(gf, minlength=total)
    if int(cnt.max()) > MAX_ROWS:
        raise ValueError(f"{what}: more than {MAX_ROWS} rows in one frame of one sequence")
    r.off = _exclusive(cnt).to(torch.int32)
    uniq, inv = torch.unique(torch.stack([s, i], 1), dim=0, return_inverse=True)
    r.n_ids = torch.bincount(uniq[:, 0], minlength=S)
    r.id_base, r.ids = _exclusive(r.n_ids), uniq[:, 1].contiguous()
    if int(torch.unique(gf * int(uniq.shape[0]) + inv).shape[0]) != n:
        raise ValueError(f"{what}_id: an id occurs twice in one frame of one sequence")
    r.boxes = b[r.order].contiguous()
    r.dense = (inv - r.id_base[s])[r.order].to(torch.int32).contiguous()
    return r


class _Problem:
    """The validated, sorted inputs of one evaluation and the raw outputs every path fills: counts (S, 4) int64 = TP, FN, FP,
    IDSW; sum_iou (S,) fp64; gt_match / gt_switch in sorted ground-truth order (gt_match: sorted hypothesis row); state
    (6, sum G_s) int32 = last + 1, cur, stamp, seen, hit, runs; pot (sum G_s * H_s,) int32."""

    def __init__(self, gt_seq, gt_frame, gt_id, gt_boxes, hy_seq, hy_frame, hy_id, hy_boxes, n_frames, thr, dev):
        self.dev, self.thr = dev, float(thr)
        if not np.isfinite(self.thr):
            raise ValueError("thr: not finite")
        nf = _ints(n_frames, None, "n_frames", dev)
        if nf.shape[0] and int(nf.min()) < 0:
            raise ValueError("n_frames: negative")
        self.n_frames, self.S = nf, int(nf.shape[0])
        self.base = _exclusive(nf)
        self.total = int(self.base[-1])
        if self.total >= 2 ** 31 - 2:
            raise ValueError("more than 2^31 - 3 frames")
        self.gt = _prepare(gt_seq, gt_frame, gt_id, gt_boxes, nf, self.base, "gt", dev)
        self.hy = _prepare(hy_seq, hy_frame, hy_id, hy_boxes, nf, self.base, "hy", dev)
        self.Ng, self.Nh = int(self.gt.boxes.shape[0]), int(self.hy.boxes.shape[0])
        self.pot_base = _exclusive(self.gt.n_ids * self.hy.n_ids)
        self.n_gt_ids, self.n_pot = int(self.gt.id_base[-1]), int(self.pot_base[-1])
        self.frame_base32 = self.base.to(torch.int32)
        self.gt_id_base32 = self.gt.id_base.to(torch.int32)
        self.hy_count32 = self.hy.n_ids.to(torch.int32)
        self.ws_ints = max(L.MOT_STATE_ROWS * self.n_gt_ids + self.n_pot, 1)

    def outputs(self, dev):
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)   # noqa: E731
        return dict(counts=z((self.S, 4), torch.int64), sum_iou=z((self.S,), torch.float64), gt_match=z((self.Ng,), torch.int32),
                    gt_switch=z((self.Ng,), torch.uint8), ws=z((self.ws_ints,), torch.int32))

    def call_args(self, out):
        gt, hy = self.gt, self.hy
        return ([L.ptr(gt.boxes), L.ptr(gt.dense), L.ptr(gt.off), self.Ng, L.ptr(hy.boxes), L.ptr(hy.dense), L.ptr(hy.off), self.Nh,
                 L.ptr(self.frame_base32), L.ptr(self.gt_id_base32), L.ptr(self.hy_count32), L.ptr(self.pot_base), self.S,
                 self.total, self.n_gt_ids, self.n_pot, self.thr] +
                [L.ptr(out[k]) for k in ("counts", "sum_iou", "gt_match", "gt_switch", "ws")] + [self.ws_ints * 4])

    def raw(self, out):
        ws = out["ws"].cpu().numpy()
        k = L.MOT_STATE_ROWS * self.n_gt_ids
        return dict(counts=out["counts"].cpu().numpy(), sum_iou=out["sum_iou"].cpu().numpy(),
                    gt_match=out["gt_match"].cpu().numpy(), gt_switch=out["gt_switch"].cpu().numpy(),
                    state=ws[:k].reshape(L.MOT_STATE_ROWS, self.n_gt_ids).copy(), pot=ws[k:k + self.n_pot].copy())


def _match_device(pb):
    """One launch on the current stream of pb.dev; nothing is read back here."""
    out = pb.outputs(pb.dev)
    L.check(L.load().fp_mot_match(*pb.call_args(out), L.current_stream(pb.dev)), "fp_mot_match")
    return out


def _match_emulate(pb):
    out = pb.outputs(torch.device("cpu"))
    L.check(L.load().fp_mot_match_emulate(*pb.call_args(out)), "fp_mot_match_emulate")
    return out


def _match_numpy(pb):
    """The procedure of DESIGN section 7, frame after frame."""
    gt, hy = pb.gt, pb.hy
    gb, gd, goff = gt.boxes.numpy(), gt.dense.numpy(), gt.off.numpy()
    hb, hd, hoff = hy.boxes.numpy(), hy.dense.numpy(), hy.off.numpy()
    base, idb, potb = pb.base.numpy(), gt.id_base.numpy(), pb.pot_base.numpy()
    n_hy_ids = hy.n_ids.numpy()
    counts, sum_iou = np.zeros((pb.S, 4), np.int64), np.zeros(pb.S)
    gt_match, gt_switch = -np.ones(pb.Ng, np.int32), np.zeros(pb.Ng, np.uint8)
    state, pot_all = np.zeros((L.MOT_STATE_ROWS, pb.n_gt_ids), np.int32), np.zeros(pb.n_pot, np.int32)
    for s in range(pb.S):
        G, H = int(idb[s + 1] - idb[s]), int(n_hy_ids[s])
        last, cur = -np.ones(G, np.int64), -np.ones(G, np.int64)
        seen, hit, runs = (state[k, idb[s]:idb[s + 1]] for k in (3, 4, 5))
        pot = pot_all[potb[s]:potb[s + 1]].reshape(G, H)
        TP = FN = FP = IDSW = 0
        acc = np.float64(0.0)
        for gf in range(base[s], base[s + 1]):
            g0, g1, h0, h1 = goff[gf], goff[gf + 1], hoff[gf], hoff[gf + 1]
            n, m = g1 - g0, h1 - h0
            g, h = gd[g0:g1].astype(np.int64), hd[h0:h1].astype(np.int64)
            k = 0
            new_cur = -np.ones(G, np.int64)
            if n and m:
                sim = _iou_matrix(gb[g0:g1], hb[h0:h1])
                adm = sim >= pb.thr
                np.add.at(pot, (g[:, None].repeat(m, 1)[adm], h[None, :].repeat(n, 0)[adm]), 1)
                score = np.where(adm, sim + np.where(cur[g][:, None] == h[None, :], BONUS, 0.0), 0.0)
                col = assign_max(score)
                for i in range(n):
                    j = col[i]
                    if j < 0 or not score[i, j] > 0:
                        continue
                    gi, hj = g[i], h[j]
                    sw = last[gi] >= 0 and last[gi] != hj
                    IDSW += int(sw)
                    hit[gi] += 1
                    runs[gi] += int(cur[gi] < 0)
                    acc = acc + sim[i, j]
                    gt_match[g0 + i], gt_switch[g0 + i] = h0 + j, sw
                    last[gi] = new_cur[gi] = hj
                    k += 1
            seen[g] += 1
            cur = new_cur
            TP, FN, FP = TP + k, FN + n - k, FP + m - k
        counts[s] = (TP, FN, FP, IDSW)
        sum_iou[s] = acc
    return dict(counts=counts, sum_iou=sum_iou, gt_match=gt_match, gt_switch=gt_switch, state=state, pot=pot_all)


# ---- results ---------------------------------------------------------------------------------------------------------------

def _ratio(a, b):
    return float(a) / float(b) if b else -1.0


def derive(c):
    """The derived numbers of a dict of counters (fp64 from integers and sum_iou); -1 where a denominator is 0."""
    TP, FN, FP = c["TP"], c["FN"], c["FP"]
    return dict(MOTA=_ratio(TP - FP - c["IDSW"], TP + FN), MOTP=_ratio(c["sum_iou"], TP) if TP else -1.0,
                IDF1=_ratio(c["IDTP"], c["IDTP"] + (c["IDFN"] + c["IDFP"]) / 2), IDP=_ratio(c["IDTP"], c["IDTP"] + c["IDFP"]),
                IDR=_ratio(c["IDTP"], c["IDTP"] + c["IDFN"]), precision=_ratio(TP, TP + FP), recall=_ratio(TP, TP + FN))


class MotResult:
    """sequences: one dict per sequence with the counters (COUNT_KEYS; n_gt_ids / n_hy_ids = distinct ids), sum_iou and the
    derived numbers (DERIVED_KEYS); combined: the same keys from the integers and sum_iou summed in sequence order, as
    MOTChallenge's combined row.  gt_match (Ng,) int32: the caller's index of the hypothesis row matched to every ground-truth
    row, -1 without one; gt_switch (Ng,) uint8: the match was an identity switch.  pot: per sequence the (G_s, H_s) int32
    counts of admissible pairs, rows / columns in ascending order of the caller's ids (gt_ids[s], hy_ids[s]).  Attribute
    access reaches the combined numbers: res.MOTA, res.IDSW, ..."""

    def __init__(self, sequences, combined, gt_match, gt_switch, pot, gt_ids, hy_ids, thr):
        self.sequences, self.combined = sequences, combined
        self.gt_match, self.gt_switch, self.pot, self.gt_ids, self.hy_ids, self.thr = gt_match, gt_switch, pot, gt_ids, hy_ids, thr

    def __getattr__(self, name):
        combined = self.__dict__.get("combined")
        if combined is not None and name in combined:
            return combined[name]
        raise AttributeError(name)

    _COLS = ("MOTA", "MOTP", "IDF1", "IDP", "IDR", "recall", "precision", "TP", "FN", "FP", "IDSW", "Frag", "MT", "PT", "ML")

    def summary(self, names=None):
        """A header, one line per sequence and the combined line."""
        fmt = lambda v: f"{v:9.4f}" if isinstance(v, float) else f"{v:9d}"   # noqa: E731
        lines = [f"{'sequence':<16}" + "".join(f"{c:>10}" for c in self._COLS)]
        for k, row in enumerate(self.sequences + [self.combined]):
            name = "COMBINED" if k == len(self.sequences) else (str(names[k]) if names is not None else f"seq{k}")
            lines.append(f"{name:<16}" + "".join(" " + fmt(row[c]) for c in self._COLS))
        return "\n".join(lines)


def _finish(pb, raw):
    gt, hy = pb.gt, pb.hy
    gorder, horder = gt.order.cpu().numpy(), hy.order.cpu().numpy()
    gm = raw["gt_match"].astype(np.int64)
    gt_match, gt_switch = -np.ones(pb.Ng, np.int32), np.zeros(pb.Ng, np.uint8)
    if pb.Ng:
        gt_match[gorder] = np.where(gm >= 0, horder[np.clip(gm, 0, max(pb.Nh - 1, 0))] if pb.Nh else -1, -1)
        gt_switch[gorder] = raw["gt_switch"]
    idb, potb = gt.id_base.cpu().numpy(), pb.pot_base.cpu().numpy()
    hidb, n_hy_ids = hy.id_base.cpu().numpy(), hy.n_ids.cpu().numpy()
    gids, hids = gt.ids.cpu().numpy(), hy.ids.cpu().numpy()
    sequences, pots, gt_ids, hy_ids = [], [], [], []
    for s in range(pb.S):
        G, H = int(idb[s + 1] - idb[s]), int(n_hy_ids[s])
        seen, hit, runs = (raw["state"][k, idb[s]:idb[s + 1]].astype(np.int64) for k in (3, 4, 5))
        pot = raw["pot"][potb[s]:potb[s + 1]].reshape(G, H)
        TP, FN, FP, IDSW = (int(v) for v in raw["counts"][s])
        live = seen > 0
        frac = hit[live] / seen[live]
        mt = frac > 0.8
        pt = (frac >= 0.2) & ~mt
        idtp = _idtp(pot)
        c = dict(TP=TP, FN=FN, FP=FP, IDSW=IDSW, Frag=int(np.maximum(runs - 1, 0).sum()), MT=int(mt.sum()), PT=int(pt.sum()),
                 ML=int((~mt & ~pt).sum()), IDTP=idtp, IDFN=TP + FN - idtp, IDFP=TP + FP - idtp, n_gt_ids=G, n_hy_ids=H,
                 sum_iou=float(raw["sum_iou"][s]))
        sequences.append(c)
        pots.append(pot)
        gt_ids.append(gids[idb[s]:idb[s + 1]])
        hy_ids.append(hids[hidb[s]:hidb[s + 1]])
    combined = {k: sum(c[k] for c in sequences) for k in COUNT_KEYS}
    total = 0.0
    for c in sequences:                                       # sequence order
        total = total + c["sum_iou"]
    combined["sum_iou"] = total
    for c in sequences + [combined]:
        c.update(derive(c))
    return MotResult(sequences, combined, gt_match, gt_switch, pots, gt_ids, hy_ids, pb.thr)


_PATHS = {"numpy": _match_numpy, "emulate": lambda pb: pb.raw(_match_emulate(pb))}


def mot_eval(gt_seq, gt_frame, gt_id, gt_boxes, hy_seq, hy_frame, hy_id, hy_boxes, n_frames, *, thr=0.5, device=None,
             _path=None) -> MotResult:
    """CLEAR-MOT and identity measures of hypothesis rows against ground-truth rows.  Per row: the sequence (0 ..
    len(n_frames) - 1), the frame inside it (0-based, below n_frames[seq]), an integer id (arbitrary values, compared inside
    a sequence) and an xywh box; arrays or tensors.  device None / "cpu": the numpy path; a HIP device: the kernel.
    ValueError: shape mismatches, non-integer ids, sequences or frames out of range, non-finite boxes, negative widths or
    heights, an id twice in one frame of one sequence, more than 64 rows of either kind in one frame of one sequence."""
    dev = torch.device("cpu" if device is None else device)
    if dev.type == "cpu":
        pb = _Problem(gt_seq, gt_frame, gt_id, gt_boxes, hy_seq, hy_frame, hy_id, hy_boxes, n_frames, thr, dev)
        return _finish(pb, _PATHS[_path or "numpy"](pb))
    with torch.cuda.device(dev):
        pb = _Problem(gt_seq, gt_frame, gt_id, gt_boxes, hy_seq, hy_frame, hy_id, hy_boxes, n_frames, thr, dev)
        return _finish(pb, pb.raw(_match_device(pb)))


def mot_eval_emulate(*args, **kw) -> MotResult:
    """mot_eval through fp_mot_match_emulate: the kernel's decision code on host memory (no GPU needed)."""
    return mot_eval(*args, device="cpu", _path="emulate", **kw)


# ---- HOTA ----------------------------------------------------------------------------------------------------------------
# DESIGN section 7 "Tracker evaluation: HOTA" and include/facepath.h are the specification.  The same three paths as above:
# numpy, fp_hota_match (csrc/hota.hip) and fp_hota_match_emulate give the same integers and the same bits of gt_sim and gas;
# everything per alpha is derived here, on the host, from their per-row outputs.

MAX_ALPHAS = L.HOTA_MAX_ALPHAS
DEFAULT_ALPHAS = np.arange(1, 20) / 20.0                 # 0.05 .. 0.95, computed once: every path compares against these bits
HOTA_INT_KEYS = ("TP", "FN", "FP")
HOTA_SUM_KEYS = ("loc_sum", "ass_num", "re_num", "pr_num")
HOTA_KEYS = ("HOTA", "DetA", "AssA", "DetRe", "DetPr", "AssRe", "AssPr", "LocA")


def _alphas(alphas):
    a = DEFAULT_ALPHAS.copy() if alphas is None else np.array(alphas, dtype=np.float64).reshape(-1)
    if alphas is not None and np.ndim(alphas) != 1:
        raise ValueError("alphas: expected a one-dimensional array")
    if not 1 <= a.shape[0] <= MAX_ALPHAS:
        raise ValueError(f"alphas: expected 1 .. {MAX_ALPHAS} values, got {a.shape[0]}")
    if not bool(np.all((a > 0.0) & (a <= 1.0))):
        raise ValueError("alphas: every value must lie in (0, 1]")
    if not bool(np.all(a[1:] > a[:-1])):
        raise ValueError("alphas: not strictly ascending")
    return np.ascontiguousarray(a)


def _seq_sum(x):
    """The sum of x in ascending index order, one fp64 addition each (np.sum adds pairwise)."""
    x = np.asarray(x, np.float64)
    return float(np.add.accumulate(x)[-1]) if x.shape[0] else 0.0


class _HotaProblem(_Problem):
    """_Problem with the localisation thresholds in place of thr, and the raw outputs of the HOTA paths: gt_match (sorted
    hypothesis row) and gt_sim in sorted ground-truth order, levels (S, A + 1) int64, counts (S, 2) int64 = n_gt, n_hy; the
    workspace = gas (sum G_s * H_s) fp64, then gtc (sum G_s) and hyc (sum H_s) int32."""

    def __init__(self, gt_seq, gt_frame, gt_id, gt_boxes, hy_seq, hy_frame, hy_id, hy_boxes, n_frames, alphas, dev):
        self.alphas = _alphas(alphas)
        super().__init__(gt_seq, gt_frame, gt_id, gt_boxes, hy_seq, hy_frame, hy_id, hy_boxes, n_frames, 0.0, dev)
        self.A = int(self.alphas.shape[0])
        self.n_hy_ids = int(self.hy.id_base[-1])
        self.hy_id_base32 = self.hy.id_base.to(torch.int32)
        self.ws_ints = max(2 * self.n_pot + self.n_gt_ids + self.n_hy_ids, 2)

    def outputs(self, dev):
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)   # noqa: E731
        return dict(gt_match=z((self.Ng,), torch.int32), gt_sim=z((self.Ng,), torch.float64),
                    levels=z((self.S, self.A + 1), torch.int64), counts=z((self.S, 2), torch.int64), ws=z((self.ws_ints,), torch.int32))

    def call_args(self, out):
        gt, hy = self.gt, self.hy
        return ([L.ptr(gt.boxes), L.ptr(gt.dense), L.ptr(gt.off), self.Ng, L.ptr(hy.boxes), L.ptr(hy.dense), L.ptr(hy.off), self.Nh,
                 L.ptr(self.frame_base32), L.ptr(self.gt_id_base32), L.ptr(self.hy_id_base32), L.ptr(self.pot_base), self.S,
                 self.total, self.n_gt_ids, self.n_hy_ids, self.n_pot, self.alphas.ctypes.data, self.A] +
                [L.ptr(out[k]) for k in ("gt_match", "gt_sim", "levels", "counts", "ws")] + [self.ws_ints * 4])

    def raw(self, out):
        ws = out["ws"].cpu().numpy()
        k = 2 * self.n_pot
        return dict(gt_match=out["gt_match"].cpu().numpy(), gt_sim=out["gt_sim"].cpu().numpy(), levels=out["levels"].cpu().numpy(),
                    counts=out["counts"].cpu().numpy(), gas=ws[:k].view(np.float64).copy(),
                    gtc=ws[k:k + self.n_gt_ids].copy(), hyc=ws[k + self.n_gt_ids:k + self.n_gt_ids + self.n_hy_ids].copy())


def _hota_device(pb):
    """One launch on the current stream of pb.dev; nothing is read back here."""
    out = pb.outputs(pb.dev)
    L.check(L.load().fp_hota_match(*pb.call_args(out), L.current_stream(pb.dev)), "fp_hota_match")
    return out


def _hota_emulate(pb):
    out = pb.outputs(torch.device("cpu"))
    L.check(L.load().fp_hota_match_emulate(*pb.call_args(out)), "fp_hota_match_emulate")
    return out


def _hota_numpy(pb):
    """The procedure of DESIGN section 7 "Tracker evaluation: HOTA": the alignment march, the sweep, the matching march."""
    gt, hy = pb.gt, pb.hy
    gb, gd, goff = gt.boxes.numpy(), gt.dense.numpy(), gt.off.numpy()
    hb, hd, hoff = hy.boxes.numpy(), hy.dense.numpy(), hy.off.numpy()
    base, gidb, hidb, potb = pb.base.numpy(), gt.id_base.numpy(), hy.id_base.numpy(), pb.pot_base.numpy()
    gt_match, gt_sim = -np.ones(pb.Ng, np.int32), np.zeros(pb.Ng)
    levels, counts = np.zeros((pb.S, pb.A + 1), np.int64), np.zeros((pb.S, 2), np.int64)
    gas_all, gtc_all, hyc_all = np.zeros(pb.n_pot), np.zeros(pb.n_gt_ids, np.int32), np.zeros(pb.n_hy_ids, np.int32)
    for s in range(pb.S):
        G, H = int(gidb[s + 1] - gidb[s]), int(hidb[s + 1] - hidb[s])
        gtc, hyc = gtc_all[gidb[s]:gidb[s + 1]], hyc_all[hidb[s]:hidb[s + 1]]
        pmc = np.zeros((G, H))
        frames = []
        for gf in range(base[s], base[s + 1]):
            g0, g1, h0, h1 = goff[gf], goff[gf + 1], hoff[gf], hoff[gf + 1]
            g, h = gd[g0:g1].astype(np.int64), hd[h0:h1].astype(np.int64)
            sim = _iou_matrix(gb[g0:g1], hb[h0:h1]) if len(g) and len(h) else np.zeros((len(g), len(h)))
            frames.append((g0, h0, g, h, sim))
            gtc[g] += 1
            hyc[h] += 1
            if sim.size:
                row = np.add.accumulate(sim, axis=1)[:, -1]           # ascending j, one addition each
                col = np.add.accumulate(sim, axis=0)[-1, :]           # ascending i
                den = (row[:, None] + col[None, :]) - sim
                pos = sim > 0.0
                pmc[np.ix_(g, h)] += np.divide(sim, den, out=np.zeros_like(sim), where=pos)
        pos = pmc > 0.0
        gas = np.divide(pmc, (gtc[:, None].astype(np.float64) + hyc[None, :].astype(np.float64)) - pmc, out=np.zeros_like(pmc),
                        where=pos)
        gas_all[potb[s]:potb[s + 1]] = gas.reshape(-1)
        for g0, h0, g, h, sim in frames:
            counts[s] += (len(g), len(h))
            if not sim.size:
                continue
            score = gas[np.ix_(g, h)] * sim
            col = assign_max(score)
            for i in range(len(g)):
                j = col[i]
                if j < 0 or not score[i, j] > 0:
                    continue
                gt_match[g0 + i], gt_sim[g0 + i] = h0 + j, sim[i, j]
                levels[s, int(np.count_nonzero(sim[i, j] >= pb.alphas))] += 1
    return dict(gt_match=gt_match, gt_sim=gt_sim, levels=levels, counts=counts, gas=gas_all, gtc=gtc_all, hyc=hyc_all)


def _mean(x):
    return _seq_sum(x) / len(x) if len(x) else -1.0


def derive_hota(c):
    """The per-alpha arrays and headline means of a dict of TP / FN / FP (int64 arrays) and loc_sum / ass_num / re_num / pr_num
    (fp64 arrays).  -1 where a Det* denominator is 0 (HOTA too); AssA = AssRe = AssPr = 0 and LocA = -1 where TP is 0 (TrackEval
    reports 1 there).  The headline numbers are the means over the alphas, LocA over the alphas with TP > 0 (-1 without one)."""
    TP, FN, FP = (c[k].astype(np.float64) for k in HOTA_INT_KEYS)
    some = TP > 0

    def ratio(num, den, empty):
        return np.divide(num, den, out=np.full(TP.shape, float(empty)), where=den > 0)
    pa = dict(DetA=ratio(TP, TP + FN + FP, -1), DetRe=ratio(TP, TP + FN, -1), DetPr=ratio(TP, TP + FP, -1),
              AssA=ratio(c["ass_num"], TP, 0), AssRe=ratio(c["re_num"], TP, 0), AssPr=ratio(c["pr_num"], TP, 0),
              LocA=ratio(c["loc_sum"], TP, -1))
    pa["HOTA"] = np.where(pa["DetA"] >= 0, np.sqrt(np.maximum(pa["DetA"], 0.0) * pa["AssA"]), -1.0)
    out = {k: _mean(pa[k]) for k in HOTA_KEYS if k != "LocA"}
    out["LocA"] = _mean(pa["LocA"][some]) if some.any() else -1.0
    out["per_alpha"] = pa
    return out


class HotaResult:
    """alphas (A,) fp64.  sequences: one dict per sequence with TP / FN / FP (A,) int64, loc_sum / ass_num / re_num / pr_num
    (A,) fp64, n_gt / n_hy, levels (A + 1,) int64, the headline means (HOTA_KEYS) and per_alpha: the same names as (A,) fp64
    arrays; combined: the same keys from the integers and numerators summed in sequence order, then derived (so AssA combines
    TP-weighted, as TrackEval's combined row).  gt_match (Ng,) int32: the caller's index of the hypothesis row matched to every
    ground-truth row, -1 without one; gt_sim (Ng,) fp64: the IoU of that pair, 0 without one; levels (S, A + 1) int64: matched
    pairs by the number of alphas their IoU reaches.  gas: per sequence the (G_s, H_s) fp64 global alignment scores, gtc / hyc
    the frames every id occurs in, rows / columns in ascending order of the caller's ids (gt_ids[s], hy_ids[s]).  Attribute
    access reaches the combined headline numbers: res.HOTA, res.DetA, ..."""

    def __init__(self, alphas, sequences, combined, gt_match, gt_sim, levels, gas, gtc, hyc, gt_ids, hy_ids):
        self.alphas, self.sequences, self.combined = alphas, sequences, combined
        self.gt_match, self.gt_sim, self.levels, self.gas, self.gtc, self.hyc = gt_match, gt_sim, levels, gas, gtc, hyc
        self.gt_ids, self.hy_ids = gt_ids, hy_ids

    def __getattr__(self, name):
        combined = self.__dict__.get("combined")
        if combined is not None and name in combined:
            return combined[name]
        raise AttributeError(name)

    def columns(self):
        """The header and one string per sequence and for the combined row: HOTA_KEYS in summary()'s column format."""
        return ["".join(f"{c:>10}" for c in HOTA_KEYS)] + ["".join(f" {row[c]:9.4f}" for c in HOTA_KEYS)
                                                           for row in self.sequences + [self.combined]]

    def summary(self, names=None):
        """A header, one line per sequence and the combined line."""
        cols = self.columns()
        lines = [f"{'sequence':<16}" + cols[0]]
        for k in range(len(self.sequences) + 1):
            name = "COMBINED" if k == len(self.sequences) else (str(names[k]) if names is not None else f"seq{k}")
            lines.append(f"{name:<16}" + cols[k + 1])
        return "\n".join(lines)


def _hota_finish(pb, raw):
    gt, hy = pb.gt, pb.hy
    A, alphas = pb.A, pb.alphas
    gorder, horder = gt.order.cpu().numpy(), hy.order.cpu().numpy()
    gm = raw["gt_match"].astype(np.int64)
    gt_match, gt_sim = -np.ones(pb.Ng, np.int32), np.zeros(pb.Ng)
    if pb.Ng:
        gt_match[gorder] = np.where(gm >= 0, horder[np.clip(gm, 0, max(pb.Nh - 1, 0))] if pb.Nh else -1, -1)
        gt_sim[gorder] = raw["gt_sim"]
    gidb, hidb, potb = gt.id_base.cpu().numpy(), hy.id_base.cpu().numpy(), pb.pot_base.cpu().numpy()
    gids, hids = gt.ids.cpu().numpy(), hy.ids.cpu().numpy()
    gdense, hdense = gt.dense.cpu().numpy().astype(np.int64), hy.dense.cpu().numpy().astype(np.int64)
    goff, base = gt.off.cpu().numpy(), pb.base.cpu().numpy()
    sequences, gas_list, gtc_list, hyc_list, gt_ids, hy_ids = [], [], [], [], [], []
    for s in range(pb.S):
        G, H = int(gidb[s + 1] - gidb[s]), int(hidb[s + 1] - hidb[s])
        gtc, hyc = raw["gtc"][gidb[s]:gidb[s + 1]].astype(np.int64), raw["hyc"][hidb[s]:hidb[s + 1]].astype(np.int64)
        r0, r1 = int(goff[base[s]]), int(goff[base[s + 1]])               # the sequence's rows in sorted order
        rows = np.arange(r0, r1)[gm[r0:r1] >= 0]
        rows = rows[np.argsort(gorder[rows], kind="stable")]              # ascending caller row order
        sim = raw["gt_sim"][rows]
        key = gdense[rows] * H + hdense[np.clip(gm[rows], 0, max(pb.Nh - 1, 0))] if len(rows) else np.zeros(0, np.int64)
        n_gt, n_hy = (int(v) for v in raw["counts"][s])
        c = dict(TP=np.zeros(A, np.int64), loc_sum=np.zeros(A), ass_num=np.zeros(A), re_num=np.zeros(A), pr_num=np.zeros(A),
                 n_gt=n_gt, n_hy=n_hy, levels=raw["levels"][s].astype(np.int64), n_gt_ids=G, n_hy_ids=H)
        for a in range(A):
            sel = sim >= alphas[a]
            c["TP"][a] = int(sel.sum())
            c["loc_sum"][a] = _seq_sum(sim[sel])
            pair, mc = np.unique(key[sel], return_counts=True)            # the id pairs that occur, ascending (g, h)
            g, h = pair // max(H, 1), pair % max(H, 1)
            mcf = mc.astype(np.float64)
            c["ass_num"][a] = _seq_sum(mcf * (mcf / np.maximum(1, gtc[g] + hyc[h] - mc)))
            c["re_num"][a] = _seq_sum(mcf * (mcf / np.maximum(1, gtc[g])))
            c["pr_num"][a] = _seq_sum(mcf * (mcf / np.maximum(1, hyc[h])))
        c["FN"], c["FP"] = n_gt - c["TP"], n_hy - c["TP"]
        sequences.append(c)
        gas_list.append(raw["gas"][potb[s]:potb[s + 1]].reshape(G, H))
        gtc_list.append(gtc)
        hyc_list.append(hyc)
        gt_ids.append(gids[gidb[s]:gidb[s + 1]])
        hy_ids.append(hids[hidb[s]:hidb[s + 1]])
    combined = {k: np.zeros(A, np.int64) for k in HOTA_INT_KEYS}
    combined.update({k: np.zeros(A) for k in HOTA_SUM_KEYS})
    combined.update(n_gt=0, n_hy=0, levels=np.zeros(A + 1, np.int64), n_gt_ids=0, n_hy_ids=0)
    for c in sequences:                                                   # sequence order
        for k in HOTA_INT_KEYS + HOTA_SUM_KEYS + ("n_gt", "n_hy", "levels", "n_gt_ids", "n_hy_ids"):
            combined[k] = combined[k] + c[k]
    for c in sequences + [combined]:
        c.update(derive_hota(c))
    return HotaResult(alphas, sequences, combined, gt_match, gt_sim, raw["levels"].astype(np.int64), gas_list, gtc_list, hyc_list,
                      gt_ids, hy_ids)


_HOTA_PATHS = {"numpy": _hota_numpy, "emulate": lambda pb: pb.raw(_hota_emulate(pb))}


def hota_eval(gt_seq, gt_frame, gt_id, gt_boxes, hy_seq, hy_frame, hy_id, hy_boxes, n_frames, *, alphas=None, device=None,
              _path=None) -> HotaResult:
    """HOTA (DetA, AssA, LocA and their recalls / precisions) of hypothesis rows against ground-truth rows: the arguments and
    ValueErrors of mot_eval, with alphas -- strictly ascending localisation thresholds inside (0, 1], at most 32, default
    0.05 .. 0.95 -- in place of thr.  device None / "cpu": the numpy path; a HIP device: the kernel."""
    dev = torch.device("cpu" if device is None else device)
    if dev.type == "cpu":
        pb = _HotaProblem(gt_seq, gt_frame, gt_id, gt_boxes, hy_seq, hy_frame, hy_id, hy_boxes, n_frames, alphas, dev)
        return _hota_finish(pb, _HOTA_PATHS[_path or "numpy"](pb))
    with torch.cuda.device(dev):
        pb = _HotaProblem(gt_seq, gt_frame, gt_id, gt_boxes, hy_seq, hy_frame, hy_id, hy_boxes, n_frames, alphas, dev)
        return _hota_finish(pb, pb.raw(_hota_device(pb)))


def hota_eval_emulate(*args, **kw) -> HotaResult:
    """hota_eval through fp_hota_match_emulate: the kernel's decision code on host memory (no GPU needed)."""
    return hota_eval(*args, device="cpu", _path="emulate", **kw)


class TrackingEvaluator:
    """Collects a tracker's rows step by step on the device (add() never synchronises with the host) and scores them against
    the ground truth given to set_ground_truth()."""

    def __init__(self, n_seqs, device, thr=0.5):
        self.n_seqs, self.device, self.thr = int(n_seqs), torch.device(device), float(thr)
        self._seq, self._frame, self._id, self._boxes, self._keep = [], [], [], [], []
        self._gt = None

    def set_ground_truth(self, gt_seq, gt_frame, gt_id, gt_boxes, n_frames):
        if len(n_frames) != self.n_seqs:
            raise ValueError(f"n_frames: expected {self.n_seqs} sequences, got {len(n_frames)}")
        self._gt = (gt_seq, gt_frame, gt_id, gt_boxes, n_frames)
        return self

    def add(self, seq_of_frame, frame_base, frame, boxes_xyxy, track_id, valid=None):
        """One step of the pipeline.  seq_of_frame (B,) integers: the sequence of every frame of the batch, -1 for a frame
        that is not scored (the tracker's stream_of_frame when stream = sequence); frame_base: the frame number inside its
        sequence of every batch frame, (B,) integers, or one integer for the batch's first frame when the batch holds
        consecutive frames of one video; frame (n,): the batch index of every row (info[:, 0]); boxes_xyxy (n, 4)
        (info[:, 1:5]); track_id (n,) the tracker's ids; valid (n,) bool or None.  Tensors on any device.  Rows with
        track_id <= 0 (FULL, NO_STREAM, OVER, dead rows) and rows of unscored frames are dropped, in evaluate(), and counted
        (self.dropped)."""
        n = int(track_id.shape[0])
        if tuple(boxes_xyxy.shape) != (n, 4) or tuple(frame.shape) != (n,) or seq_of_frame.ndim != 1 or (
                valid is not None and tuple(valid.shape) != (n,)):
            raise ValueError(f"add(): frame {tuple(frame.shape)}, boxes {tuple(boxes_xyxy.shape)}, track_id {tuple(track_id.shape)} "
                             "do not describe n rows")
        for name, t in (("seq_of_frame", seq_of_frame), ("frame", frame), ("track_id", track_id)):
            if t.dtype.is_floating_point or t.dtype == torch.bool:
                raise ValueError(f"add(): {name} must be integers, got {t.dtype}")
        dev, B = self.device, int(seq_of_frame.shape[0])
        sof = seq_of_frame.to(dev, torch.int64, non_blocking=True)
        if isinstance(frame_base, torch.Tensor) or np.ndim(frame_base) == 1:
            number = torch.as_tensor(frame_base).to(dev, torch.int64, non_blocking=True)
            if tuple(number.shape) != (B,):
                raise ValueError(f"add(): frame_base {tuple(number.shape)} for {B} frames")
        else:
            number = int(frame_base) + torch.arange(B, dtype=torch.int64, device=dev)
        fr = frame.to(dev, torch.int64, non_blocking=True)
        tid = track_id.to(dev, torch.int64, non_blocking=True)
        box = boxes_xyxy.to(dev, torch.float64, non_blocking=True)
        inside = (fr >= 0) & (fr < B)
        fc = fr.clamp(0, max(B - 1, 0))
        seq = sof[fc] if B else torch.full_like(fr, -1)
        keep = inside & (seq >= 0) & (tid > 0)
        if valid is not None:
            keep = keep & valid.to(dev, torch.bool, non_blocking=True)
        self._seq.append(seq)
        self._frame.append(number[fc] if B else fr)
        self._id.append(tid)
        self._boxes.append(torch.cat([box[:, :2], box[:, 2:] - box[:, :2]], 1))
        self._keep.append(keep)

    def rows(self):
        """(seq, frame, id, xywh boxes) of everything kept so far, on the device."""
        if not self._seq:
            z = torch.zeros(0, dtype=torch.int64, device=self.device)
            return z, z, z, torch.zeros((0, 4), dtype=torch.float64, device=self.device)
        keep = torch.cat(self._keep)
        return torch.cat(self._seq)[keep], torch.cat(self._frame)[keep], torch.cat(self._id)[keep], torch.cat(self._boxes)[keep]

    @property
    def dropped(self):
        return int(sum(int(k.numel()) for k in self._keep) - sum(int(k.sum()) for k in self._keep))

    def evaluate(self) -> MotResult:
        if self._gt is None:
            raise ValueError("evaluate(): no ground truth; call set_ground_truth() first")
        gt_seq, gt_frame, gt_id, gt_boxes, n_frames = self._gt
        return mot_eval(gt_seq, gt_frame, gt_id, gt_boxes, *self.rows(), n_frames, thr=self.thr, device=self.device)

    def evaluate_hota(self, alphas=None) -> HotaResult:
        """hota_eval on the rows collected so far; evaluate() and its thr are not involved."""
        if self._gt is None:
            raise ValueError("evaluate_hota(): no ground truth; call set_ground_truth() first")
        gt_seq, gt_frame, gt_id, gt_boxes, n_frames = self._gt
        return hota_eval(gt_seq, gt_frame, gt_id, gt_boxes, *self.rows(), n_frames, alphas=alphas, device=self.device)


# ---- MOTChallenge text rows ----------------------------------------------------------------------------------------------

def write_mot_txt(path, frame, ids, boxes_xywh, conf=None):
    """Rows `frame,id,x,y,w,h,conf,-1,-1,-1`, the frame numbers 1-based in the file (0-based here), floats in their shortest
    form that reads back to the same fp64."""
    frame, ids = np.asarray(frame, np.int64), np.asarray(ids, np.int64)
    boxes = np.asarray(boxes_xywh, np.float64).reshape(-1, 4)
    conf = np.ones(len(frame)) if conf is None else np.asarray(conf, np.float64)
    if not (len(frame) == len(ids) == len(boxes) == len(conf)):
        raise ValueError("write_mot_txt: frame, ids, boxes and conf differ in length")
    with open(path, "w") as fh:
        for f, i, b, c in zip(frame.tolist(), ids.tolist(), boxes.tolist(), conf.tolist()):
            fh.write(",".join([str(f + 1), str(i)] + [repr(v) for v in b] + [repr(c), "-1", "-1", "-1"]) + "\n")


def read_mot_txt(path):
    """-> dict(frame (n,) int64 0-based, id (n,) int64, boxes (n, 4) fp64 xywh, conf (n,) fp64).  Rows need at least six
    fields; a missing confidence reads as 1."""
    frame, ids, boxes, conf = [], [], [], []
    with open(path) as fh:
        for ln, line in enumerate(fh, 1):
            line = line.strip()
            if not line:
                continue
            parts = line.replace(" ", ",").split(",")
            parts = [p for p in parts if p != ""]
            if len(parts) < 6:
                raise ValueError(f"{path}:{ln}: expected frame,id,x,y,w,h[,conf,...]")
            frame.append(int(float(parts[0])) - 1)
            ids.append(int(float(parts[1])))
            boxes.append([float(v) for v in parts[2:6]])
            conf.append(float(parts[6]) if len(parts) > 6 else 1.0)
    return dict(frame=np.array(frame, np.int64), id=np.array(ids, np.int64), boxes=np.array(boxes, np.float64).reshape(-1, 4),
                conf=np.array(conf, np.float64))
