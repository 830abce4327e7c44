"""Seeded synthetic sets for the detector-evaluation tests, and a literal restatement of the matching rule of DESIGN
section 7 (one Python loop per ground-truth box, as the published sequential scan) that the numpy path is checked against."""
import numpy as np

SCORES16 = np.arange(1, 17) / 16.0        # 16 distinct score values: ties within and across images


def _image(rng, n_gt, n_dt, span):
    """Integer xywh boxes on a coarse grid: duplicates and exact IoU ties occur; detections are jittered copies of GTs or noise."""
    sizes = np.array([8, 16, 24, 32, 48, 64, 96, 128])
    g = np.zeros((n_gt, 4))
    if n_gt:
        g[:, 2] = rng.choice(sizes, n_gt)
        g[:, 3] = rng.choice(sizes, n_gt)
        g[:, 0] = rng.integers(0, span // 8, n_gt) * 8
        g[:, 1] = rng.integers(0, span // 8, n_gt) * 8
    d = np.zeros((n_dt, 4))
    for k in range(n_dt):
        if n_gt and rng.random() < 0.75:
            d[k] = g[rng.integers(n_gt)]
            d[k, :2] += rng.choice([-8, 0, 0, 8], 2)
            d[k, 2:] = np.maximum(d[k, 2:] + rng.choice([-8, 0, 0, 0, 8], 2), 0)     # a zero-sized detection now and then
        else:
            d[k] = (rng.integers(0, span // 8) * 8, rng.integers(0, span // 8) * 8, rng.choice(sizes), rng.choice(sizes))
    return g, d


def synthetic_set(seed=0, n_images=40, big=True):
    """-> dict(gt_boxes, gt_image, gt_area, dt_boxes, dt_scores, dt_image, n_images).  With big: image 3 has 300 GTs, image 4
    has 1 100, image 5 has 130 detections; images 0 / 1 / 2 have no GT / no detection / neither; image 6 holds the exact-area
    and exact-IoU constructions.  About 4 000 detections in total."""
    rng = np.random.default_rng(seed)
    gb, gi, ga, db, di = [], [], [], [], []
    for i in range(n_images):
        n_gt, n_dt, span = int(rng.integers(1, 30)), int(rng.integers(70, 140)), 512
        if i == 0:
            n_gt = 0
        elif i == 1:
            n_dt = 0
        elif i == 2:
            n_gt = n_dt = 0
        elif big and i == 3:
            n_gt, n_dt, span = 300, 110, 1024
        elif big and i == 4:
            n_gt, n_dt, span = 1100, 120, 2048
        elif big and i == 5:
            n_dt = 130
        g, d = _image(rng, n_gt, n_dt, span)
        area = g[:, 2] * g[:, 3]
        if i == 6:
            # areas exactly on the range borders (inside both neighbours), IoU exactly 0.5 and exactly 0.75
            g = np.array([[0, 0, 32, 32], [600, 0, 96, 96], [0, 600, 10, 20], [300, 600, 40, 40], [700, 700, 16, 64]], float)
            area = g[:, 2] * g[:, 3]
            d = np.concatenate([d, [[0, 600, 10, 10], [300, 600, 30, 40], [0, 0, 32, 32], [600, 0, 96, 96], [700, 700, 64, 16]]])
        if i == 7 and n_gt:
            area = area.copy()
            area[0] = 5000.0                 # an annotation whose area is not w * h
        gb.append(g), ga.append(area), gi.append(np.full(len(g), i)), db.append(d), di.append(np.full(len(d), i))
    dt_boxes = np.concatenate(db)
    return dict(gt_boxes=np.concatenate(gb), gt_image=np.concatenate(gi).astype(np.int64), gt_area=np.concatenate(ga),
                dt_boxes=dt_boxes, dt_scores=rng.choice(SCORES16, len(dt_boxes)), dt_image=np.concatenate(di).astype(np.int64),
                n_images=n_images)


def literal_match(gt_boxes, gt_area, dt_boxes, thr, lo, hi):
    """One image, one area range, one threshold; dt_boxes in score order.  The sequential scan: GTs sorted not-ignored first
    (stable), `if iou < best: continue`, stop at the first ignored GT once a not-ignored one is held.  -> (matched, ignored, gt index)."""
    def iou(d, g):
        iw = min(d[0] + d[2], g[0] + g[2]) - max(d[0], g[0])
        ih = min(d[1] + d[3], g[1] + g[3]) - max(d[1], g[1])
        if iw <= 0 or ih <= 0:
            return 0.0
        i = iw * ih
        return i / (d[2] * d[3] + g[2] * g[3] - i)
    gig = [bool(a < lo or a > hi) for a in gt_area]
    order = sorted(range(len(gt_boxes)), key=lambda j: gig[j])
    taken = [False] * len(gt_boxes)
    out = []
    for d in dt_boxes:
        best, m = min(thr, 1 - 1e-10), -1
        for j in order:
            if taken[j]:
                continue
            if m > -1 and not gig[m] and gig[j]:
                break
            v = iou(d, gt_boxes[j])
            if v < best:
                continue
            best, m = v, j
        if m > -1:
            taken[m] = True
            out.append((1, int(gig[m]), m))
        else:
            a = d[2] * d[3]
            out.append((0, int(a < lo or a > hi), -1))
    return out
