"""Score a detector against ground truth: COCO-style bbox AP / AR for one category without crowd boxes.

The reference's eval/eval_face_detector.py hands its annotations and detections to pycocotools, which is not part of the
reference tree.  This module restates the published procedure (DESIGN.md section 7 is the specification; parity with
pycocotools is unpinned) twice:

  * ``device=None`` / ``"cpu"``: plain numpy, fp64, detections walked one after the other -- the oracle, and the path for a
    machine without a GPU;
  * a HIP device: fp_det_match (one workgroup per image and area range, all IoU thresholds) and fp_pr_accumulate (one
    workgroup per precision / recall curve), csrc/deteval.hip.  Sorting and the CSR offsets are torch plumbing.

Both give the same match decisions, the same integer counts and, from them, bit-identical precision and recall arrays.
"""
import numpy as np
import torch

from . import _lib as L

DEFAULT_IOU_THRS = np.linspace(.5, .95, 10)
DEFAULT_REC_THRS = np.linspace(.0, 1.00, 101)
DEFAULT_MAX_DETS = (1, 10, 100)
DEFAULT_AREA_RNGS = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))
AREA_LABELS = ("all", "small", "medium", "large")


class CocoBBoxResult:
    """precision (T, R, A, M) and recall (T, A, M) fp64, -1 where an area range has no ground truth; stats: the twelve COCO
    numbers (None unless there are four area ranges and three maxDets); matched / ignored (A, T, Nd) uint8 for the Nd
    detections that survive the per-image cut, in (image id, rank) order; dt_order (Nd,): their indices in the caller's
    arrays; dt_rank (Nd,): their per-image ranks; npig (A,): ground-truth boxes not ignored per area range."""

    def __init__(self, precision, recall, npig, matched, ignored, dt_order, dt_rank, iou_thrs, rec_thrs, max_dets, area_rngs):
        self.precision, self.recall, self.npig = precision, recall, npig
        self._lazy = {"matched": matched, "ignored": ignored, "dt_order": dt_order, "dt_rank": dt_rank}
        self.iou_thrs, self.rec_thrs, self.max_dets, self.area_rngs = iou_thrs, rec_thrs, max_dets, area_rngs
        self.stats = self._stats() if len(area_rngs) == 4 and len(max_dets) == 3 else None
        self.dt_gt = None        # numpy path only: (A, T, Nd) index of the matched ground-truth box, -1 without one

    def _get(self, name):
        v = self._lazy[name]
        if isinstance(v, torch.Tensor):          # the device path leaves the flags on the device until somebody asks
            v = self._lazy[name] = v.cpu().numpy()
        return v

    matched = property(lambda self: self._get("matched"))
    ignored = property(lambda self: self._get("ignored"))
    dt_order = property(lambda self: self._get("dt_order"))
    dt_rank = property(lambda self: self._get("dt_rank"))

    def _select(self, ap, iou_thr, a, m):
        s = self.precision[:, :, a, m] if ap else self.recall[:, a, m]
        if iou_thr is not None:
            s = s[np.where(iou_thr == self.iou_thrs)[0]]
        s = s[s > -1]
        return float(np.mean(s)) if s.size else -1.0

    _ROWS = ((1, None, 0, 2), (1, .5, 0, 2), (1, .75, 0, 2), (1, None, 1, 2), (1, None, 2, 2), (1, None, 3, 2),
             (0, None, 0, 0), (0, None, 0, 1), (0, None, 0, 2), (0, None, 1, 2), (0, None, 2, 2), (0, None, 3, 2))

    def _stats(self):
        return np.array([self._select(*row) for row in self._ROWS], np.float64)

    def summary(self):
        """The familiar twelve lines."""
        if self.stats is None:
            raise ValueError("summary() needs the COCO layout: four area ranges (all, small, medium, large) and three maxDets")
        lines = []
        for (ap, thr, a, m), v in zip(self._ROWS, self.stats):
            iou = "{:0.2f}:{:0.2f}".format(self.iou_thrs[0], self.iou_thrs[-1]) if thr is None else "{:0.2f}".format(thr)
            lines.append(" {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}".format(
                "Average Precision" if ap else "Average Recall", "(AP)" if ap else "(AR)", iou, AREA_LABELS[a],
                int(self.max_dets[m]), v))
        return "\n".join(lines)


# ---- arguments -------------------------------------------------------------------------------------------------------

def _tensor(x, dtype, device):
    if isinstance(x, torch.Tensor):
        return x.detach().to(device=device, dtype=dtype)
    return torch.as_tensor(np.asarray(x), dtype=dtype, device=device)


def _ids(x, n, what, n_images, device):
    if isinstance(x, torch.Tensor):
        if x.dtype.is_floating_point or x.dtype == torch.bool:
            raise ValueError(f"{what}: image ids must be integers, got {x.dtype}")
    else:
        x = np.asarray(x)
        if x.size == 0:
            x = x.astype(np.int64)
        if x.dtype.kind not in "iu":
            raise ValueError(f"{what}: image ids must be integers, got {x.dtype}")
    t = _tensor(x, torch.int64, device)
    if t.ndim != 1 or t.shape[0] != n:
        raise ValueError(f"{what}: expected shape ({n},), got {tuple(t.shape)}")
    if n and (int(t.min()) < 0 or int(t.max()) >= n_images):
        raise ValueError(f"{what}: image ids outside [0, {n_images})")
    return t


def _boxes(x, what, device):
    t = _tensor(x, torch.float64, device)
    if t.numel() == 0 and t.ndim == 1:
        t = t.reshape(0, 4)
    if t.ndim != 2 or t.shape[1] != 4:
        raise ValueError(f"{what}: expected shape (n, 4) xywh, got {tuple(t.shape)}")
    if t.numel():
        if not bool(torch.isfinite(t).all()):
            raise ValueError(f"{what}: non-finite box")
        if bool((t[:, 2:] < 0).any()):
            raise ValueError(f"{what}: negative width or height")
    return t.contiguous()


def _vector(x, n, what, device):
    t = _tensor(x, torch.float64, device)
    if t.ndim != 1 or t.shape[0] != n:
        raise ValueError(f"{what}: expected shape ({n},), got {tuple(t.shape)}")
    if n and not bool(torch.isfinite(t).all()):
        raise ValueError(f"{what}: non-finite value")
    return t.contiguous()


def _params(iou_thrs, rec_thrs, max_dets, area_rngs):
    iou_thrs = np.array(DEFAULT_IOU_THRS if iou_thrs is None else iou_thrs, np.float64)
    rec_thrs = np.array(DEFAULT_REC_THRS if rec_thrs is None else rec_thrs, np.float64)
    area_rngs = np.array(DEFAULT_AREA_RNGS if area_rngs is None else area_rngs, np.float64)
    md = np.asarray(max_dets)
    if iou_thrs.ndim != 1 or not 1 <= iou_thrs.size <= L.DETEVAL_MAX_THRS or not np.isfinite(iou_thrs).all():
        raise ValueError(f"iou_thrs: 1 to {L.DETEVAL_MAX_THRS} finite thresholds")
    if rec_thrs.ndim != 1 or not 1 <= rec_thrs.size <= L.DETEVAL_MAX_RECS or not np.isfinite(rec_thrs).all():
        raise ValueError(f"rec_thrs: 1 to {L.DETEVAL_MAX_RECS} finite thresholds")
    if area_rngs.ndim != 2 or area_rngs.shape[1] != 2 or area_rngs.shape[0] < 1 or np.isnan(area_rngs).any():
        raise ValueError("area_rngs: expected shape (A, 2)")
    if md.ndim != 1 or md.size < 1 or md.dtype.kind not in "iu" or (md < 1).any() or (np.diff(md) < 0).any():
        raise ValueError("max_dets: positive integers in ascending order")
    return iou_thrs, rec_thrs, md.astype(np.int64), area_rngs


# ---- numpy path ------------------------------------------------------------------------------------------------------

def _iou_matrix(d, g):
    """(D, 4) x (G, 4) xywh -> (D, G), the operations in the order DESIGN section 7 writes them."""
    dx, dy, dw, dh = (d[:, i, None] for i in range(4))
    gx, gy, gw, gh = (g[None, :, i] for i in range(4))
    iw = np.minimum(dx + dw, gx + gw) - np.maximum(dx, gx)
    ih = np.minimum(dy + dh, gy + gh) - np.maximum(dy, gy)
    i = iw * ih
    u = dw * dh + gw * gh - i
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = i / u
    return np.where((iw <= 0) | (ih <= 0), 0.0, iou)


def _last_argmax(cand, row):
    """Per threshold row of cand (T, G): the candidate with the largest IoU, on equal IoU the last one; -1 without one."""
    G = row.shape[0]
    vals = np.where(cand, row[None, :], -1.0)
    j = G - 1 - np.argmax(vals[:, ::-1], axis=1)
    return np.where(cand.any(axis=1), j, -1)


def _match_image(d, g, garea, thr, area_rngs, matched, ignored, dt_gt, npig):
    """Greedy matching of one image; matched / ignored / dt_gt (position of the matched GT in the image) are (A, T, D) views
    that are filled."""
    D, G, T = d.shape[0], g.shape[0], thr.shape[0]
    ious = _iou_matrix(d, g) if D and G else np.zeros((D, G))
    darea = d[:, 2] * d[:, 3]
    for a, (lo, hi) in enumerate(area_rngs):
        gig = (garea < lo) | (garea > hi)
        npig[a] += int((~gig).sum())
        dout = (darea < lo) | (darea > hi)
        gtm = np.zeros((T, G), bool)
        for k in range(D):
            if G:
                ok = (ious[k][None, :] >= thr[:, None]) & ~gtm
                pn = _last_argmax(ok & ~gig[None, :], ious[k])
                pi = _last_argmax(ok & gig[None, :], ious[k])
            else:
                pn = pi = np.full(T, -1)
            pick = np.where(pn >= 0, pn, pi)
            hit = pick >= 0
            gtm[np.nonzero(hit)[0], pick[hit]] = True
            matched[a, :, k] = hit
            dt_gt[a, :, k] = pick
            ignored[a, :, k] = np.where(hit, pn < 0, dout[k])


def _eval_numpy(gtb, gti, gta, dtb, dts, dti, n_images, iou_thrs, rec_thrs, max_dets, area_rngs):
    T, R, A, M = len(iou_thrs), len(rec_thrs), len(area_rngs), len(max_dets)
    o1 = np.argsort(-dts, kind="stable")
    perm = o1[np.argsort(dti[o1], kind="stable")]
    dt_start = np.concatenate([[0], np.cumsum(np.bincount(dti, minlength=n_images))])
    rank = np.arange(len(perm)) - dt_start[dti[perm]]
    keep = rank < max_dets[-1]
    dt_order, rank = perm[keep], rank[keep]
    img = dti[dt_order]
    dt_off = np.concatenate([[0], np.cumsum(np.bincount(img, minlength=n_images))])
    gperm = np.argsort(gti, kind="stable")
    gt_off = np.concatenate([[0], np.cumsum(np.bincount(gti, minlength=n_images))])
    boxes, scores = dtb[dt_order], dts[dt_order]
    gboxes, gareas = gtb[gperm], gta[gperm]
    Nd = len(dt_order)
    thr = np.minimum(iou_thrs, 1 - 1e-10)
    matched = np.zeros((A, T, Nd), np.uint8)
    ignored = np.zeros((A, T, Nd), np.uint8)
    dt_gt = -np.ones((A, T, Nd), np.int64)
    npig = np.zeros(A, np.int64)
    for i in range(n_images):
        d0, d1, g0, g1 = dt_off[i], dt_off[i + 1], gt_off[i], gt_off[i + 1]
        _match_image(boxes[d0:d1], gboxes[g0:g1], gareas[g0:g1], thr, area_rngs, matched[:, :, d0:d1], ignored[:, :, d0:d1],
                     dt_gt[:, :, d0:d1], npig)
        hit = dt_gt[:, :, d0:d1] >= 0                      # -> the GT's index in the caller's arrays
        dt_gt[:, :, d0:d1][hit] = gperm[g0 + dt_gt[:, :, d0:d1][hit]]

    precision = -np.ones((T, R, A, M))
    recall = -np.ones((T, A, M))
    for mi, m in enumerate(max_dets):
        sel = rank < m
        inds = np.argsort(-scores[sel], kind="mergesort")
        for a in range(A):
            if npig[a] == 0:
                continue
            for t in range(T):
                dtm = matched[a, t][sel][inds].astype(bool)
                dig = ignored[a, t][sel][inds].astype(bool)
                dtm = dtm[~dig]
                tp = np.cumsum(dtm, dtype=np.int64)
                fp = np.cumsum(~dtm, dtype=np.int64)
                rc = tp / int(npig[a])
                pr = tp / (fp + tp + np.spacing(1))
                recall[t, a, mi] = rc[-1] if len(tp) else 0
                pr = np.maximum.accumulate(pr[::-1])[::-1]
                idx = np.searchsorted(rc, rec_thrs, side="left")
                q = np.zeros(R)
                ok = idx < len(tp)
                q[ok] = pr[idx[ok]]
                precision[t, :, a, mi] = q
    res = CocoBBoxResult(precision, recall, npig, matched, ignored, dt_order, rank, iou_thrs, rec_thrs, max_dets, area_rngs)
    res.dt_gt = dt_gt
    return res


# ---- device path -----------------------------------------------------------------------------------------------------

def _csr(ids, n_images, cap=None):
    c = torch.bincount(ids, minlength=n_images)
    if cap is not None:
        c = c.clamp(max=cap)
    off = torch.zeros(n_images + 1, dtype=torch.int64, device=ids.device)
    off[1:] = torch.cumsum(c, 0)
    return off


class _DeviceEval:
    """The device path in its three steps (tools/deteval_bench.py times them one by one): prepare() is torch plumbing --
    per-image stable score order, the cut to the largest maxDet, CSR offsets, the global score order; match() and
    accumulate() are one kernel launch each."""

    def __init__(self, iou_thrs, rec_thrs, max_dets, area_rngs, n_images, dev):
        self.lib, self.dev, self.n_images = L.load(), dev, n_images
        self.params = (iou_thrs, rec_thrs, max_dets, area_rngs)
        self.T, self.R, self.A, self.M = len(iou_thrs), len(rec_thrs), len(area_rngs), len(max_dets)
        self.d_thr = torch.from_numpy(iou_thrs).to(dev)
        self.d_rec = torch.from_numpy(rec_thrs).to(dev)
        self.d_rng = torch.from_numpy(np.ascontiguousarray(area_rngs)).to(dev)
        self.d_md = torch.from_numpy(max_dets.astype(np.int32)).to(dev)

    def prepare(self, gtb, gti, gta, dtb, dts, dti):
        n_images, dev, cap = self.n_images, self.dev, int(self.params[2][-1])
        o1 = torch.sort(-dts, stable=True).indices
        perm = o1[torch.sort(dti[o1], stable=True).indices]
        start = _csr(dti, n_images)
        rank = torch.arange(perm.shape[0], device=dev) - start[dti[perm]]
        keep = rank < cap
        self.dt_order, self.rank = perm[keep], rank[keep].to(torch.int32)
        self.dt_off = _csr(dti, n_images, cap).to(torch.int32)
        gperm = torch.sort(gti, stable=True).indices
        self.gt_off = _csr(gti, n_images).to(torch.int32)
        self.boxes, scores = dtb[self.dt_order].contiguous(), dts[self.dt_order].contiguous()
        self.gboxes, self.gareas = gtb[gperm].contiguous(), gta[gperm].contiguous()
        self.Nd, self.Ng = int(self.boxes.shape[0]), int(self.gboxes.shape[0])
        if self.Nd >= 2 ** 31 or self.Ng >= 2 ** 31:
            raise ValueError("more than 2^31 - 1 boxes")
        self.order = torch.sort(-scores, stable=True).indices
        self.rank_sorted = self.rank[self.order].contiguous()
        A, T, R, M, Nd = self.A, self.T, self.R, self.M, self.Nd
        self.matched = torch.empty((A, T, Nd), dtype=torch.uint8, device=dev)
        self.ignored = torch.empty((A, T, Nd), dtype=torch.uint8, device=dev)
        self.npig = torch.empty((A,), dtype=torch.int32, device=dev)
        self.ws_bytes = self.lib.fp_det_match_workspace(self.Ng, A)
        self.ws = torch.empty((self.ws_bytes // 4,), dtype=torch.int32, device=dev)
        self.precision = torch.empty((T, R, A, M), dtype=torch.float64, device=dev)
        self.recall = torch.empty((T, A, M), dtype=torch.float64, device=dev)
        return self

    def match(self):
        L.check(self.lib.fp_det_match(L.ptr(self.gboxes), L.ptr(self.gareas), L.ptr(self.gt_off), L.ptr(self.boxes),
                                      L.ptr(self.dt_off), self.n_images, self.Ng, self.Nd, L.ptr(self.d_thr), self.T,
                                      L.ptr(self.d_rng), self.A, L.ptr(self.matched), L.ptr(self.ignored), L.ptr(self.npig),
                                      L.ptr(self.ws), self.ws_bytes, L.current_stream(self.dev)), "fp_det_match")

    def accumulate(self):
        L.check(self.lib.fp_pr_accumulate(L.ptr(self.matched), L.ptr(self.ignored), L.ptr(self.order), L.ptr(self.rank_sorted),
                                          self.Nd, L.ptr(self.npig), self.T, self.A, L.ptr(self.d_md), self.M, L.ptr(self.d_rec),
                                          self.R, L.ptr(self.precision), L.ptr(self.recall), L.current_stream(self.dev)),
                "fp_pr_accumulate")

    def result(self):
        return CocoBBoxResult(self.precision.cpu().numpy(), self.recall.cpu().numpy(), self.npig.cpu().numpy().astype(np.int64),
                              self.matched, self.ignored, self.dt_order, self.rank, *self.params)


def _eval_device(gtb, gti, gta, dtb, dts, dti, n_images, iou_thrs, rec_thrs, max_dets, area_rngs, dev):
    ev = _DeviceEval(iou_thrs, rec_thrs, max_dets, area_rngs, n_images, dev).prepare(gtb, gti, gta, dtb, dts, dti)
    ev.match()
    ev.accumulate()
    return ev.result()


def coco_eval_bbox(gt_boxes, gt_image, dt_boxes, dt_scores, dt_image, n_images, *, gt_area=None, iou_thrs=None,
                   rec_thrs=None, max_dets=DEFAULT_MAX_DETS, area_rngs=None, device=None) -> CocoBBoxResult:
    """COCO bbox evaluation of detections (xywh boxes, scores, image ids) against ground truth (xywh boxes, image ids, areas
    defaulting to w * h) over images 0 .. n_images - 1.  Arrays or tensors.  device None / "cpu": the numpy path; a HIP
    device: the kernels.  ValueError on shape mismatches, image ids outside [0, n_images), non-finite boxes, scores or areas
    and negative widths or heights."""
    dev = torch.device("cpu" if device is None else device)
    n_images = int(n_images)
    if n_images < 0:
        raise ValueError("n_images < 0")
    iou_thrs, rec_thrs, max_dets, area_rngs = _params(iou_thrs, rec_thrs, max_dets, area_rngs)
    gtb = _boxes(gt_boxes, "gt_boxes", dev)
    dtb = _boxes(dt_boxes, "dt_boxes", dev)
    gti = _ids(gt_image, gtb.shape[0], "gt_image", n_images, dev)
    dti = _ids(dt_image, dtb.shape[0], "dt_image", n_images, dev)
    dts = _vector(dt_scores, dtb.shape[0], "dt_scores", dev)
    gta = gtb[:, 2] * gtb[:, 3] if gt_area is None else _vector(gt_area, gtb.shape[0], "gt_area", dev)
    if dev.type == "cpu":
        return _eval_numpy(gtb.numpy(), gti.numpy(), gta.numpy(), dtb.numpy(), dts.numpy(), dti.numpy(), n_images, iou_thrs,
                           rec_thrs, max_dets, area_rngs)
    with torch.cuda.device(dev):
        return _eval_device(gtb, gti, gta, dtb, dts, dti, n_images, iou_thrs, rec_thrs, max_dets, area_rngs, dev)


class DetectionEvaluator:
    """Collects detections batch by batch on the device (add() never synchronises with the host) and scores them against
    the ground truth given to set_ground_truth()."""

    def __init__(self, n_images, device, **params):
        self.n_images, self.device, self.params = int(n_images), torch.device(device), params
        self._ids, self._boxes, self._scores, self._valid = [], [], [], []
        self._gt = None

    def set_ground_truth(self, gt_boxes, gt_image, gt_area=None):
        self._gt = (gt_boxes, gt_image, gt_area)
        return self

    def add(self, image_ids, boxes_xywh, scores, valid=None):
        """image_ids (n,) integer, boxes_xywh (n, 4), scores (n,), valid (n,) bool or None (padding rows of a detector's
        fixed-size output are dropped in evaluate(), not here): tensors, any device.  Values are checked in evaluate()."""
        n = int(scores.shape[0])
        if (tuple(boxes_xywh.shape) != (n, 4) or tuple(image_ids.shape) != (n,) or scores.ndim != 1
                or (valid is not None and tuple(valid.shape) != (n,))):
            raise ValueError(f"add(): image_ids {tuple(image_ids.shape)}, boxes {tuple(boxes_xywh.shape)}, scores "
                             f"{tuple(scores.shape)} do not describe n boxes")
        if image_ids.dtype.is_floating_point or image_ids.dtype == torch.bool:
            raise ValueError(f"add(): image ids must be integers, got {image_ids.dtype}")
        self._ids.append(image_ids.to(self.device, torch.int64, non_blocking=True))
        self._boxes.append(boxes_xywh.to(self.device, torch.float64, non_blocking=True))
        self._scores.append(scores.to(self.device, torch.float64, non_blocking=True))
        self._valid.append(torch.ones(n, dtype=torch.bool, device=self.device) if valid is None
                           else valid.to(self.device, torch.bool, non_blocking=True))

    def detections(self):
        """(image ids, xywh boxes, scores) of everything added so far, on the device."""
        if not self._ids:
            return (torch.zeros(0, dtype=torch.int64, device=self.device), torch.zeros((0, 4), dtype=torch.float64, device=self.device),
                    torch.zeros(0, dtype=torch.float64, device=self.device))
        keep = torch.cat(self._valid)
        return torch.cat(self._ids)[keep], torch.cat(self._boxes)[keep], torch.cat(self._scores)[keep]

    def evaluate(self) -> CocoBBoxResult:
        if self._gt is None:
            raise ValueError("evaluate(): no ground truth; call set_ground_truth() first")
        ids, boxes, scores = self.detections()
        gt_boxes, gt_image, gt_area = self._gt
        return coco_eval_bbox(gt_boxes, gt_image, boxes, scores, ids, self.n_images, gt_area=gt_area, device=self.device,
                              **self.params)


# ---- detector rows -> boxes in frame pixels ----------------------------------------------------------------------------

def dets_to_frame_boxes(detector, dets, counts, frame_sizes):
    """Raw rows of detector.raw_batch -> (boxes (B, K, 4) fp64 xyxy in each frame's own pixels, scores (B, K) fp64, valid
    (B, K) bool = row < counts[frame]), all on the rows' device and without a host synchronisation.  frame_sizes: host list
    of (h, w) per frame.  dets_fmt 0 (BlazeFace: normalised (ymin, xmin, ymax, xmax), confidence last) and 1 (YOLOv5-face:
    input pixels, confidence in column 4) are taken back through the letterbox with the arithmetic of
    modules/utils/image.py scale_coords (subtract the pad, divide by the gain, clip to the frame); dets_fmt 2 (MTCNN) is
    already in frame pixels: gain 1, no pad."""
    fmt = detector.dets_fmt
    B, K = int(dets.shape[0]), int(dets.shape[1])
    if len(frame_sizes) != B or tuple(counts.shape) != (B,):
        raise ValueError(f"dets_to_frame_boxes: {B} frames of rows, {len(frame_sizes)} sizes, counts {tuple(counts.shape)}")
    dev = dets.device
    rows = dets.to(torch.float64)
    if fmt == 0:
        iw, ih = detector.input_size
        scores = rows[:, :, -1]
        boxes = rows[:, :, [1, 0, 3, 2]] * torch.tensor([iw, ih, iw, ih], dtype=torch.float64, device=dev)
    elif fmt == 1:
        iw, ih = detector.input_size
        scores = rows[:, :, 4]
        boxes = rows[:, :, :4].clone()
    elif fmt == 2:
        scores = rows[:, :, 14]
        boxes = rows[:, :, :4].clone()
    else:
        raise ValueError(f"dets_to_frame_boxes: unknown dets_fmt {fmt}")
    geom = np.empty((B, 6), np.float64)                    # pad x, pad y, gain, width, height
    for i, (h, w) in enumerate(frame_sizes):
        if fmt == 2:
            gain, px, py = 1.0, 0.0, 0.0
        else:                                              # scale_coords((ih, iw), ., (h, w))
            gain = min(ih / h, iw / w)
            px, py = (iw - w * gain) / 2, (ih - h * gain) / 2
        geom[i] = (px, py, gain, w, h, 0.0)
    g = torch.from_numpy(geom).to(dev, non_blocking=True)[:, None, :]
    pad = torch.stack([g[..., 0], g[..., 1], g[..., 0], g[..., 1]], -1)
    lim = torch.stack([g[..., 3], g[..., 4], g[..., 3], g[..., 4]], -1)
    boxes = (boxes - pad) / g[..., 2:3]
    boxes = torch.minimum(boxes.clamp(min=0.0), lim)
    valid = torch.arange(K, device=dev)[None, :] < counts.to(dev)[:, None]
    return boxes, scores, valid


def clamp_boxes_xywh(boxes_xyxy, frame_wh):
    """The box arithmetic of the reference's eval script on the device: truncate toward zero, x = clamp(left, 0, W - 1),
    w = max(0, min(right - x + 1, W - x)), likewise y / h.  boxes (..., 4) xyxy, frame_wh (..., 2) broadcastable -> int64 xywh."""
    b = torch.trunc(boxes_xyxy.to(torch.float64)).to(torch.int64)
    W, H = frame_wh[..., 0].to(torch.int64), frame_wh[..., 1].to(torch.int64)
    x = torch.minimum(b[..., 0].clamp(min=0), W - 1)
    y = torch.minimum(b[..., 1].clamp(min=0), H - 1)
    w = torch.minimum(b[..., 2] - x + 1, W - x).clamp(min=0)
    h = torch.minimum(b[..., 3] - y + 1, H - y).clamp(min=0)
    return torch.stack([x, y, w, h], -1)
