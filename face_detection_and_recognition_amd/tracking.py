"""Tracklets: faces tracked across the frames of many streams, one launch per step (csrc/tracklets.hip, fp_tracklets_step).

FacePipeline.step treats every face row alone; a video's unit of work is a track: a person is identified once per sighting,
the best shot is chosen per track (quality.best_per_group takes track_id as its group), a caption carries a stable number.
StreamTracker keeps, per stream, up to L.TRACK_SLOTS live tracks on the device and assigns every face row of a step -- 256
consecutive frames of one video, one frame of each of 256 cameras, or any mix -- a track id in ONE launch that reads nothing
back.  face_extraction/face_tracker.py (fp_tracker_step) stays the port of the reference's per-frame first-match rule.

Build-defined: the reference has nothing batched.  The procedure is written down in include/facepath.h "Tracklets" and
DESIGN.md section 7 "Tracklets"; track_step_numpy restates it (IoU float32 in the written order, cosine float64) and is the
oracle of the tests, track_step_emulate runs the kernel's own decision code on the host.  The three agree exactly wherever no
decisive cosine lies within D * 2^-24 of a threshold or of another one.  tau_near = 0.5, tau_far = 0.7408 and iou_min = 0.1
restate the reference's thresholds for unit vectors (L2 distance < 1.0 with IoU > 0.1, or < 0.72 alone; cos = 1 - d^2 / 2):
they are the reference's numbers, unmeasured on real video.  max_age has no reference counterpart and no default.

Motion prediction is opt-in: motion=ConstantVelocity(std_pos, std_vel) gives every slot four two-state constant-velocity Kalman
filters (centre, width, height), the IoU gate then takes the box the track is PREDICTED at in the frame instead of its last box,
and every matched row also reports that box (track_pred).  fp_tracklets_step_motion, include/facepath.h "Tracklets: motion
prediction"; the filter is float32 in the written order on all three paths, so it adds nothing to the agreement condition.
Without motion= nothing changes.  Rows for coasting tracks, Mahalanobis gating and camera-motion compensation are not part of
this, and no value of std_pos / std_vel has been measured.

Re-identification is opt-in too: reid=LostPool(tau_reid, lost_age) parks a track that expires in a ring of L.TRACK_LOST entries
per stream instead of dropping it, and a face that no live track takes is compared (cosine alone, against the parked track's LAST
embedding) with the parked tracks before it opens a new one; above tau_reid it continues the old track -- id, hits, first clock,
best shot -- and its row carries REVIVED instead of NEW.  fp_tracklets_step_reid, include/facepath.h "Tracklets:
re-identification"; the state gains the five lost_* arrays.  Without reid= nothing changes.  Neither parameter has a default and
neither has been measured on real video; re-identification across streams, pools beyond 64 tracks and a best-shot descriptor are
not part of this.

Templates are opt-in as well: templates=Templates(weighted=False) keeps, per stream, a table of L.TRACK_POOL entries with the
weighted sum of the normalised embeddings of every row of a track (fp_track_pool_step, csrc/trackpool.hip, two launches after
the tracker's, nothing read back; include/facepath.h "Tracklets: templates"), and step() also returns track_emb (n, D): the
sum of the row's track after the row, the row's own embedding where it has no track.  A gallery search on track_emb answers "who
is this track" (FacePipeline(identify_tracks=True)).  The state gains tpl_i, tpl_w, tpl_sum.  track_pool_numpy restates the
procedure in numpy float32, track_pool_emulate runs the kernel's own arithmetic on the host; there is no reduction, so the
three agree on every bit without a gap condition.  weighted=True weighs a row by the step's score; keep is lost_age with reid=,
else max_age.  Neither choice, nor any gain on real video, has been measured here.  Without templates= nothing changes.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L

SLOTS, MAX_DETS = L.TRACK_SLOTS, L.TRACK_MAX_DETS
NEW, BEST, DEAD_ROW, FULL, NO_STREAM, OVER = (L.TRACK_NEW, L.TRACK_BEST, L.TRACK_DEAD_ROW, L.TRACK_FULL, L.TRACK_NO_STREAM,
                                              L.TRACK_OVER)
REVIVED, LOST = L.TRACK_REVIVED, L.TRACK_LOST
LOST_KEYS = ("lost_hdr", "lost_i", "lost_f", "lost_emb", "lost_best_emb")
TAU_NEAR, TAU_FAR, IOU_MIN = 0.5, 0.7408, 0.1        # the reference's 1.0 / 0.72 L2 thresholds as cosines, and its IoU gate
I_ID, I_FIRST, I_LAST, I_HITS, I_BEST_CLOCK = range(5)      # slot_i columns
F_BOX, F_INV, F_BEST_SCORE, F_BEST_BOX = 0, 4, 5, 6         # slot_f columns
STATE_KEYS = ("hdr", "slot_i", "slot_f", "emb", "best_emb")
OUT_KEYS = ("track_id", "track_hits", "track_clock", "track_flags")
MOTION_FLOATS = L.TRACK_MOTION_FLOATS
POOL, TPL_EVICTED, TPL_RESTART = L.TRACK_POOL, L.TRACK_TPL_EVICTED, L.TRACK_TPL_RESTART
TEMPLATE_KEYS = ("tpl_i", "tpl_w", "tpl_sum")
TEMPLATE_OUT_KEYS = ("track_emb", "track_emb_rows", "track_emb_flags")
P_ID, P_LAST, P_ROWS = range(3)                             # tpl_i columns
M_X, M_V, M_P00, M_P01, M_P11, M_COLS = 0, 1, 2, 3, 4, 5    # columns of one coordinate (cx, cy, w, h) of a slot of `motion`


class ConstantVelocity:
    """The parameters of the tracker's motion prediction: noise as a fraction of the box height, both finite and > 0
    (ValueError otherwise).  No defaults, as max_age has none: nothing has been measured here.  DEEPSORT_STD_POS and
    DEEPSORT_STD_VEL are the constants DeepSORT's Kalman filter publishes (1/20 and 1/160), named for convenience and
    unmeasured on this tracker."""
    DEEPSORT_STD_POS = 1 / 20
    DEEPSORT_STD_VEL = 1 / 160

    def __init__(self, std_pos, std_vel):
        self.std_pos, self.std_vel = float(std_pos), float(std_vel)
        for name, v in (("std_pos", self.std_pos), ("std_vel", self.std_vel)):
            if not (v > 0 and np.isfinite(np.float32(v))):
                raise ValueError(f"{name} must be finite and > 0, got {v}")

    def __repr__(self):
        return f"ConstantVelocity(std_pos={self.std_pos}, std_vel={self.std_vel})"


class LostPool:
    """The parameters of the tracker's re-identification: tau_reid, the cosine a returning face must exceed against a parked
    track's last embedding (finite, ValueError otherwise), and lost_age, the frames after its last sighting for which an expired
    track stays parked (an int; the tracker wants lost_age > max_age).  No defaults: nothing has been measured here."""

    def __init__(self, tau_reid, lost_age):
        self.tau_reid = float(tau_reid)
        if not np.isfinite(np.float32(self.tau_reid)):
            raise ValueError(f"tau_reid must be finite, got {tau_reid}")
        if isinstance(lost_age, bool) or int(lost_age) != lost_age:
            raise ValueError(f"lost_age must be an int, got {lost_age!r}")
        self.lost_age = int(lost_age)

    def check(self, max_age):
        if not self.lost_age > int(max_age):
            raise ValueError(f"lost_age must be > max_age, got lost_age {self.lost_age}, max_age {max_age}")

    def __repr__(self):
        return f"LostPool(tau_reid={self.tau_reid}, lost_age={self.lost_age})"


def new_lost_state(n_streams, feat_dim):
    """A fresh pool: dict of zero numpy arrays in the layout of fp_track_lost (every entry empty, every ring head 0)."""
    S, D = int(n_streams), int(feat_dim)
    return dict(lost_hdr=np.zeros((S, 2), np.int32), lost_i=np.zeros((S, LOST, L.TRACK_SLOT_INTS), np.int32),
                lost_f=np.zeros((S, LOST, L.TRACK_SLOT_FLOATS), np.float32), lost_emb=np.zeros((S, LOST, D), np.float32),
                lost_best_emb=np.zeros((S, LOST, D), np.float32))


def _reid_args(reid, lost_state, S, D, max_age):
    """None without reid; else the checked pool dict."""
    if reid is None:
        if lost_state is not None:
            raise ValueError("lost_state without reid=")
        return None
    if not isinstance(reid, LostPool):
        raise TypeError(f"reid must be None or a LostPool, got {type(reid).__name__}")
    reid.check(max_age)
    fresh = new_lost_state(1, D)
    ok = isinstance(lost_state, dict) and all(
        isinstance(lost_state.get(k), np.ndarray) and lost_state[k].dtype == fresh[k].dtype
        and lost_state[k].shape == (S,) + fresh[k].shape[1:] and lost_state[k].flags.c_contiguous and lost_state[k].flags.writeable
        for k in LOST_KEYS)
    if not ok:
        raise ValueError(f"lost_state must be a dict of the writable C-contiguous arrays of new_lost_state({S}, {D})")
    return lost_state


class Templates:
    """The tracker keeps a template per track (module docstring).  weighted: a row's weight is the step's score (a row whose
    score is not finite and > 0 adds nothing), else every row weighs 1.  Which of the two serves real video is unmeasured."""

    def __init__(self, weighted=False):
        self.weighted = bool(weighted)

    def __repr__(self):
        return f"Templates(weighted={self.weighted})"


def new_template_state(n_streams, feat_dim):
    """A fresh template table: dict of zero numpy arrays in the layout of fp_track_templates (every entry free)."""
    S, D = int(n_streams), int(feat_dim)
    return dict(tpl_i=np.zeros((S, POOL, 3), np.int32), tpl_w=np.zeros((S, POOL), np.float32),
                tpl_sum=np.zeros((S, POOL, D), np.float32))


def _template_args(tstate, frame, emb, xinv, stream_of_frame, track_id, track_clock, track_flags, keep, weight):
    """The checked, contiguous host arguments of track_pool_numpy / track_pool_emulate."""
    fresh = new_template_state(1, 4)
    ok = isinstance(tstate, dict) and all(
        isinstance(tstate.get(k), np.ndarray) and tstate[k].dtype == fresh[k].dtype and tstate[k].ndim == fresh[k].ndim
        and tstate[k].flags.c_contiguous and tstate[k].flags.writeable for k in TEMPLATE_KEYS)
    if ok:
        S, D = tstate["tpl_sum"].shape[0], tstate["tpl_sum"].shape[2]
        ok = tstate["tpl_i"].shape == (S, POOL, 3) and tstate["tpl_w"].shape == (S, POOL) and tstate["tpl_sum"].shape[1] == POOL
    if not ok:
        raise ValueError("the template state must be a dict of the writable C-contiguous arrays of new_template_state")
    if S < 1 or D < 4 or D % 4 or D > L.TRACK_MAX_DIM:
        raise ValueError(f"need n_streams >= 1 and feat_dim a multiple of 4 in 4 .. {L.TRACK_MAX_DIM}, got {S}, {D}")
    if isinstance(keep, bool) or int(keep) != keep or int(keep) < 0:
        raise ValueError(f"keep must be an int >= 0, got {keep!r}")
    frame = np.ascontiguousarray(frame, np.int32).reshape(-1)
    n = frame.shape[0]
    emb = np.ascontiguousarray(emb, np.float32).reshape(n, D)
    xinv = np.ascontiguousarray(xinv, np.float32).reshape(n)
    sof = np.ascontiguousarray(stream_of_frame, np.int32).reshape(-1)
    ids, clocks, flags = (np.ascontiguousarray(a, np.int32).reshape(n) for a in (track_id, track_clock, track_flags))
    weight = None if weight is None else np.ascontiguousarray(weight, np.float32).reshape(n)
    return S, D, n, frame, emb, xinv, sof, ids, clocks, flags, weight


def track_pool_numpy(tstate, frame, emb, xinv, stream_of_frame, track_id, track_clock, track_flags, keep, weight=None):
    """fp_track_pool_step in numpy float32 on a host table (new_template_state; updated IN PLACE): include/facepath.h
    "Tracklets: templates", step by step.  track_id / track_clock / track_flags: a tracker step's per-row results, or crafted.
    -> dict(track_emb (n, D) float32, track_emb_rows (n,) int32, track_emb_flags (n,) int32)."""
    S, D, n, frame, emb, xinv, sof, ids, clocks, flags, weight = _template_args(
        tstate, frame, emb, xinv, stream_of_frame, track_id, track_clock, track_flags, keep, weight)
    B, keep = sof.shape[0], int(keep)
    out = dict(track_emb=emb.copy(), track_emb_rows=np.zeros((n,), np.int32), track_emb_flags=np.zeros((n,), np.int32))
    with np.errstate(all="ignore"):
        for f in range(B):
            s = int(sof[f])
            if s < 0 or s >= S:
                continue
            ti, tw, ts = tstate["tpl_i"][s], tstate["tpl_w"][s], tstate["tpl_sum"][s]
            for i in np.nonzero(frame == f)[0]:
                tid, c = int(ids[i]), int(clocks[i])
                if tid <= 0:
                    continue
                is_new, oflags = bool(flags[i] & NEW), 0
                found = np.nonzero(ti[:, P_ID] == tid)[0]
                take = bool(len(found)) and is_new
                if len(found):
                    e = int(found[0])
                else:
                    cand = np.nonzero((ti[:, P_ID] == 0) | (c - ti[:, P_LAST].astype(np.int64) > keep))[0]
                    if len(cand):
                        e = int(cand[0])
                    else:
                        e = int(np.argmin(ti[:, P_LAST]))       # the first of the smallest
                        oflags |= TPL_EVICTED
                    take = True
                    if not is_new:
                        oflags |= TPL_RESTART
                if take:
                    ts[e], tw[e] = 0, 0
                    ti[e, P_ID], ti[e, P_ROWS] = tid, 0
                w = np.float32(1) if weight is None else weight[i]
                if np.isfinite(w) and w > 0:
                    ts[e] = ts[e] + ((emb[i] * xinv[i]) * w)
                    tw[e] = tw[e] + w
                    ti[e, P_ROWS] += 1
                ti[e, P_LAST] = c
                out["track_emb_flags"][i] = oflags
                if ti[e, P_ROWS] > 0:
                    out["track_emb"][i], out["track_emb_rows"][i] = ts[e], ti[e, P_ROWS]
    return out


def _aligned_like(a):
    """a, or a 16-byte aligned copy of it (numpy aligns what it allocates; a view may start anywhere)."""
    if a.ctypes.data % 16 == 0:
        return a
    buf = np.empty((a.size + 4,), a.dtype)
    off = (-buf.ctypes.data % 16) // 4
    out = buf[off:off + a.size].reshape(a.shape)
    out[...] = a
    return out


def track_pool_emulate(tstate, frame, emb, xinv, stream_of_frame, track_id, track_clock, track_flags, keep, weight=None):
    """fp_track_pool_step_emulate on a host table (updated IN PLACE): track_pool_numpy's arguments and results.  Raises
    FacepathError on a refusal.  Needs no GPU."""
    lib = L.load()
    S, D, n, frame, emb, xinv, sof, ids, clocks, flags, weight = _template_args(
        tstate, frame, emb, xinv, stream_of_frame, track_id, track_clock, track_flags, keep, weight)
    if tstate["tpl_sum"].ctypes.data % 16:
        raise ValueError("tpl_sum must be 16-byte aligned")
    emb = _aligned_like(emb)
    out = dict(track_emb=_aligned_like(np.zeros((n, D), np.float32)), track_emb_rows=np.zeros((n,), np.int32),
               track_emb_flags=np.zeros((n,), np.int32))
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)          # noqa: E731
    st = L.FpTrackTemplates(*[p(tstate[k]) for k in TEMPLATE_KEYS])
    L.check(lib.fp_track_pool_step_emulate(C.byref(st), S, D, p(frame), p(emb), p(xinv), p(weight), n, p(sof), sof.shape[0],
                                           p(ids), p(clocks), p(flags), int(keep), *[p(out[k]) for k in TEMPLATE_OUT_KEYS]),
            "fp_track_pool_step_emulate")
    return out


def new_motion_state(n_streams):
    """A fresh `motion` array: zeros (n_streams, SLOTS, MOTION_FLOATS) float32."""
    return np.zeros((int(n_streams), SLOTS, MOTION_FLOATS), np.float32)


def check_params(n_streams, feat_dim, max_age, tau_near, tau_far, iou_min):
    """ValueError for what fp_tracklets_step would refuse."""
    if int(n_streams) < 1:
        raise ValueError(f"n_streams must be >= 1, got {n_streams}")
    if int(feat_dim) < 4 or int(feat_dim) % 4 or int(feat_dim) > L.TRACK_MAX_DIM:
        raise ValueError(f"feat_dim must be a multiple of 4 in 4 .. {L.TRACK_MAX_DIM}, got {feat_dim}")
    if int(max_age) < 0:
        raise ValueError(f"max_age must be >= 0, got {max_age}")
    if not (float(tau_far) >= float(tau_near)) or iou_min != iou_min:
        raise ValueError(f"need tau_far >= tau_near and no NaN, got tau_near {tau_near}, tau_far {tau_far}, iou_min {iou_min}")


def new_state(n_streams, feat_dim):
    """A fresh host state: dict of numpy arrays in the layout of fp_track_state (every clock 0, every next_id 1)."""
    S, D = int(n_streams), int(feat_dim)
    st = dict(hdr=np.zeros((S, 2), np.int32), slot_i=np.zeros((S, SLOTS, L.TRACK_SLOT_INTS), np.int32),
              slot_f=np.zeros((S, SLOTS, L.TRACK_SLOT_FLOATS), np.float32), emb=np.zeros((S, SLOTS, D), np.float32),
              best_emb=np.zeros((S, SLOTS, D), np.float32))
    st["hdr"][:, 1] = 1
    return st


def copy_state(state):
    return {k: np.array(state[k]) for k in STATE_KEYS}


def _row_inputs(frame, boxes, emb, xinv, score, stream_of_frame):
    frame = np.ascontiguousarray(frame, np.int32).reshape(-1)
    n = frame.shape[0]
    emb = np.ascontiguousarray(emb, np.float32)
    emb = emb.reshape(n, emb.shape[-1] if emb.ndim == 2 else 0)
    boxes = np.ascontiguousarray(boxes, np.float32).reshape(n, 4)
    xinv = np.ascontiguousarray(xinv, np.float32).reshape(n)
    score = None if score is None else np.ascontiguousarray(score, np.float32).reshape(n)
    sof = np.ascontiguousarray(stream_of_frame, np.int32).reshape(-1)
    return frame, boxes, emb, xinv, score, sof


def row_inv_norm_numpy(emb):
    """1 / |row| in float32 from a float64 sum (a zero row: inf, a dead row like any non-finite value)."""
    emb = np.asarray(emb, np.float32)
    with np.errstate(all="ignore"):
        return (1.0 / np.sqrt((emb.astype(np.float64) ** 2).sum(axis=1))).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the numpy restatement

_F = np.float32


def _hs(t):
    return t if t > _F(1) else _F(1)


def _measure(b):
    """include/facepath.h "Tracklets: motion prediction": z of a float32 box."""
    return (_F(0.5) * (b[0] + b[2]), _F(0.5) * (b[1] + b[3]), b[2] - b[0], b[3] - b[1])


def _motion_init(m, box, sp, sv):
    z = _measure(box)
    H = _hs(z[3])
    a, b = (_F(2) * sp) * H, (_F(10) * sv) * H
    for c in range(4):
        m[c * M_COLS:(c + 1) * M_COLS] = (z[c], _F(0), a * a, _F(0), b * b)


def _motion_predict(m, sp, sv):
    """One live slot one frame on (m: its (MOTION_FLOATS,) float32 row, IN PLACE) -> the predicted box (4,) float32."""
    H = _hs(m[3 * M_COLS + M_X])
    q0, q1 = (sp * H) * (sp * H), (sv * H) * (sv * H)
    for c in range(4):
        x, v, p00, p01, p11 = m[c * M_COLS:(c + 1) * M_COLS]
        a = p01 + p11
        m[c * M_COLS:(c + 1) * M_COLS] = (x + v, v, ((p00 + p01) + a) + q0, a, p11 + q1)
    cx, cy, w, h = (m[c * M_COLS + M_X] for c in range(4))
    pw, ph = (w if w > 0 else _F(0)), (h if h > 0 else _F(0))
    return np.array([cx - _F(0.5) * pw, cy - _F(0.5) * ph, cx + _F(0.5) * pw, cy + _F(0.5) * ph], np.float32)


def _motion_update(m, box, sp, sv):
    z = _measure(box)
    H = _hs(m[3 * M_COLS + M_X])
    r = (sp * H) * (sp * H)
    ok = True
    for c in range(4):
        x, v, p00, p01, p11 = m[c * M_COLS:(c + 1) * M_COLS]
        s = p00 + r
        k0, k1, y = p00 / s, p01 / s, z[c] - x
        x, v = x + k0 * y, v + k1 * y
        m[c * M_COLS:(c + 1) * M_COLS] = (x, v, p00 - k0 * p00, p01 - k1 * p00, p11 - k1 * p01)
        ok = ok and x - x == 0 and v - v == 0
    if not ok:
        _motion_init(m, box, sp, sv)


def _motion_args(motion, motion_state, S):
    """(None, None, None) without motion; else (std_pos, std_vel as float32, the checked state array)."""
    if motion is None:
        if motion_state is not None:
            raise ValueError("motion_state without motion=")
        return None, None, None
    ms = motion_state
    if not (isinstance(ms, np.ndarray) and ms.dtype == np.float32 and ms.shape == (S, SLOTS, MOTION_FLOATS)
            and ms.flags.c_contiguous and ms.flags.writeable):
        raise ValueError(f"motion_state must be a writable C-contiguous float32 array ({S}, {SLOTS}, {MOTION_FLOATS}) "
                         "(new_motion_state)")
    return np.float32(motion.std_pos), np.float32(motion.std_vel), ms

def _iou_f32(t, d):
    """include/facepath.h "Tracklets" step 2: float32, written order; t the track's box, d (k, 4) the detections'."""
    f = np.float32
    ix1, iy1 = np.where(t[0] > d[:, 0], t[0], d[:, 0]), np.where(t[1] > d[:, 1], t[1], d[:, 1])
    ix2, iy2 = np.where(t[2] < d[:, 2], t[2], d[:, 2]), np.where(t[3] < d[:, 3], t[3], d[:, 3])
    iw, ih = (ix2 - ix1).astype(f), (iy2 - iy1).astype(f)
    inter = (iw * ih).astype(f)
    area_t = f(f(t[2] - t[0]) * f(t[3] - t[1]))
    area_d = ((d[:, 2] - d[:, 0]).astype(f) * (d[:, 3] - d[:, 1]).astype(f)).astype(f)
    iou = (inter / ((area_t + area_d).astype(f) - inter).astype(f)).astype(f)
    return np.where((iw > 0) & (ih > 0), iou, f(0))


def track_step_numpy(state, frame, boxes, emb, xinv, stream_of_frame, max_age, tau_near=TAU_NEAR, tau_far=TAU_FAR,
                     iou_min=IOU_MIN, score=None, cosines=None, motion=None, motion_state=None, reid=None, lost_state=None,
                     reid_cosines=None):
    """fp_tracklets_step in numpy on a host state (new_state; updated IN PLACE).  IoU in float32 in the written order, the
    cosine in float64: (dot * inv_t) * inv_d with float64 products of the float32 values.  -> dict of the four per-row int32
    arrays.  cosines: a list that receives, per frame with live tracks and live detections, (frame, slots, rows, c (T, K)
    float64, iou (T, K) float32, the tracks' stored rows (T, D)) -- what the tests' gap condition looks at.
    motion: a ConstantVelocity, with motion_state = the streams' `motion` array (new_motion_state; updated IN PLACE): the filter
    of "Tracklets: motion prediction" in np.float32 scalars, the IoU taken with the predicted boxes, and the result also
    carries track_pred (n, 4) float32.
    reid: a LostPool, with lost_state = the streams' pool (new_lost_state; updated IN PLACE): steps 1a, 1 (parking), 3b and 4 of
    "Tracklets: re-identification", the reid cosine in float64 like step 2's.  reid_cosines: a list that receives, per frame
    with unmatched live detections and parked tracks, (frame, entries, rows, c (E, K) float64)."""
    frame, boxes, emb, xinv, score, sof = _row_inputs(frame, boxes, emb, xinv, score, stream_of_frame)
    n, B = frame.shape[0], sof.shape[0]
    S, D = state["hdr"].shape[0], state["emb"].shape[2]
    check_params(S, D, max_age, tau_near, tau_far, iou_min)
    f32 = np.float32
    tn, tf, im = float(f32(tau_near)), float(f32(tau_far)), f32(iou_min)
    sp, sv, mstate = _motion_args(motion, motion_state, S)
    pool = _reid_args(reid, lost_state, S, D, max_age)
    tr = None if pool is None else float(f32(reid.tau_reid))
    out = {k: np.zeros((n,), np.int32) for k in OUT_KEYS}
    if motion is not None:
        out["track_pred"] = np.zeros((n, 4), np.float32)
    live_row = np.isfinite(xinv) & (xinv > 0)
    ok_frame = (frame >= 0) & (frame < B)
    srow = np.full((n,), -1, np.int64)
    srow[ok_frame] = sof[frame[ok_frame]]
    untracked = (srow < 0) | (srow >= S)
    out["track_flags"][untracked] = NO_STREAM
    old = np.seterr(all="ignore")
    try:
        for f in range(B):
            s = int(sof[f])
            if s < 0 or s >= S:
                continue
            hdr, si, sf = state["hdr"][s], state["slot_i"][s], state["slot_f"][s]
            hdr[0] += 1
            clock = int(hdr[0])
            expiring = (si[:, I_ID] != 0) & (clock - si[:, I_LAST] > max_age)
            if pool is not None:
                lh, li, lf = pool["lost_hdr"][s], pool["lost_i"][s], pool["lost_f"][s]
                li[(li[:, I_ID] != 0) & (clock - li[:, I_LAST] > reid.lost_age), I_ID] = 0          # step 1a
                for t in np.nonzero(expiring)[0]:                                                    # step 1: parked, then freed
                    e = int(lh[0]) & (LOST - 1)
                    li[e], lf[e] = si[t], sf[t]
                    pool["lost_emb"][s][e], pool["lost_best_emb"][s][e] = state["emb"][s][t], state["best_emb"][s][t]
                    lh[0] = (e + 1) & (LOST - 1)
            si[expiring, I_ID] = 0
            if motion is not None:                          # step 1b: every live slot, rows or not
                pbox = {int(t): _motion_predict(mstate[s, t], sp, sv) for t in np.nonzero(si[:, I_ID] != 0)[0]}
            rows = np.nonzero(frame == f)[0]
            for i in rows[MAX_DETS:]:
                out["track_clock"][i], out["track_flags"][i] = clock, OVER
            rows = rows[:MAX_DETS]
            for i in rows[~live_row[rows]]:
                out["track_clock"][i], out["track_flags"][i] = clock, DEAD_ROW
            dets = rows[live_row[rows]]                     # ascending: position order
            slots = np.nonzero(si[:, I_ID] != 0)[0]
            taken = {}                                      # detection row -> slot
            if len(slots) and len(dets):
                te, de = state["emb"][s][slots].astype(np.float64), emb[dets].astype(np.float64)
                dot = (te[:, None, :] * de[None, :, :]).sum(axis=2)       # row by row: equal rows give equal sums
                c = (dot * sf[slots, F_INV].astype(np.float64)[:, None]) * xinv[dets].astype(np.float64)[None, :]
                iou = np.stack([_iou_f32(sf[t, F_BOX:F_BOX + 4] if motion is None else pbox[int(t)], boxes[dets]) for t in slots])
                if cosines is not None:
                    cosines.append((f, slots.copy(), dets.copy(), c.copy(), iou.copy(), state["emb"][s][slots].copy()))
                adm = ((c > tn) & (iou > im)) | (c > tf)
                ti, dj = np.nonzero(adm)
                order = np.lexsort((dj, ti, -c[ti, dj]))    # c descending, then slot, then row
                t_used, d_used = set(), set()
                for q in order:
                    t, d = int(ti[q]), int(dj[q])
                    if t in t_used or d in d_used:
                        continue
                    t_used.add(t)
                    d_used.add(d)
                    taken[int(dets[d])] = int(slots[t])
            revived = {}                                    # detection row -> pool entry (step 3b)
            if pool is not None:
                un = np.array([i for i in dets if int(i) not in taken], np.int64)
                with np.errstate(all="ignore"):
                    ents = np.nonzero((li[:, I_ID] != 0) & np.isfinite(lf[:, F_INV]) & (lf[:, F_INV] > 0))[0]
                if len(un) and len(ents):
                    le, de = pool["lost_emb"][s][ents].astype(np.float64), emb[un].astype(np.float64)
                    dot = (le[:, None, :] * de[None, :, :]).sum(axis=2)
                    c = (dot * lf[ents, F_INV].astype(np.float64)[:, None]) * xinv[un].astype(np.float64)[None, :]
                    if reid_cosines is not None:
                        reid_cosines.append((f, ents.copy(), un.copy(), c.copy()))
                    ei, dj = np.nonzero(c > tr)
                    order = np.lexsort((dj, ei, -c[ei, dj]))   # c descending, then entry, then row
                    e_used, d_used = set(), set()
                    for q in order:
                        e, d = int(ei[q]), int(dj[q])
                        if e in e_used or d in d_used:
                            continue
                        e_used.add(e)
                        d_used.add(d)
                        revived[int(un[d])] = int(ents[e])
            for i in dets:
                i = int(i)
                slot, is_new, ent = taken.get(i), False, None
                if slot is None:
                    free = np.nonzero(si[:, I_ID] == 0)[0]
                    if not len(free):                       # a revived detection too: its entry stays parked
                        out["track_clock"][i], out["track_flags"][i] = clock, FULL
                        continue
                    slot, ent = int(free[0]), revived.get(i)
                    if ent is None:
                        is_new = True
                        si[slot, I_ID], si[slot, I_FIRST], si[slot, I_HITS] = hdr[1], clock, 0
                        hdr[1] += 1
                    else:                                   # the slot continues the parked track
                        si[slot], sf[slot] = li[ent], lf[ent]
                        li[ent, I_ID] = 0
                if motion is not None and (is_new or ent is not None):
                    _motion_init(mstate[s, slot], boxes[i], sp, sv)
                elif motion is not None:
                    out["track_pred"][i] = pbox[slot]
                    _motion_update(mstate[s, slot], boxes[i], sp, sv)
                sc = f32(0) if score is None else score[i]
                si[slot, I_HITS] += 1
                si[slot, I_LAST] = clock
                sf[slot, F_BOX:F_BOX + 4], sf[slot, F_INV] = boxes[i], xinv[i]
                flags = NEW if is_new else (0 if ent is None else REVIVED)
                if is_new or sc > sf[slot, F_BEST_SCORE]:
                    sf[slot, F_BEST_SCORE], si[slot, I_BEST_CLOCK] = sc, clock
                    sf[slot, F_BEST_BOX:F_BEST_BOX + 4] = boxes[i]
                    flags |= BEST
                elif ent is not None:                       # the carried best shot keeps its embedding
                    state["best_emb"][s][slot] = pool["lost_best_emb"][s][ent]
                out["track_id"][i], out["track_hits"][i] = si[slot, I_ID], si[slot, I_HITS]
                out["track_clock"][i], out["track_flags"][i] = clock, flags
            for i in dets:                                  # after the frame's pairs were scored against the old embeddings
                i = int(i)
                if out["track_id"][i] > 0:
                    slot = int(np.nonzero(si[:, I_ID] == out["track_id"][i])[0][0])
                    state["emb"][s][slot] = emb[i]
                    if out["track_flags"][i] & BEST:
                        state["best_emb"][s][slot] = emb[i]
    finally:
        np.seterr(**old)
    return out


# ------------------------------------------------------------------------------------------------ the C entry points

def _state_struct(arrays, pointer):
    return L.FpTrackState(*[pointer(arrays[k]) for k in STATE_KEYS])


def _lost_struct(arrays, pointer):
    return L.FpTrackLost(*[pointer(arrays[k]) for k in LOST_KEYS])


def _step_call(st, lost, rows, motion_tail, reid, emulate, stream):
    """The one call of a tracker step: picks among the six fp_tracklets_step* entry points and lays out their arguments.
    st: FpTrackState; lost: FpTrackLost or None; rows: n_streams .. track_flags; motion_tail: (motion, std_pos, std_vel,
    track_pred) or None; reid: a LostPool or None (with lost); emulate: the host twin, which takes no stream."""
    name = "fp_tracklets_step" + ("_reid" if reid is not None else "_motion" if motion_tail is not None else "")
    args = (C.byref(st),) + rows
    if reid is not None:
        args = (args[0], C.byref(lost)) + rows + (reid.tau_reid, reid.lost_age) + (motion_tail or (None, 0.0, 0.0, None))
    elif motion_tail is not None:
        args += motion_tail
    if emulate:
        name += "_emulate"
    else:
        args += (stream,)
    L.check(getattr(L.load(), name)(*args), name)


def track_step_emulate(state, frame, boxes, emb, xinv, stream_of_frame, max_age, tau_near=TAU_NEAR, tau_far=TAU_FAR,
                       iou_min=IOU_MIN, score=None, motion=None, motion_state=None, reid=None, lost_state=None):
    """fp_tracklets_step_emulate on a host state (new_state; updated IN PLACE): track_step_numpy's arguments and results; with
    motion= and motion_state=, fp_tracklets_step_motion_emulate; with reid= and lost_state= (with or without motion),
    fp_tracklets_step_reid_emulate.  Raises FacepathError on a refusal.  Needs no GPU."""
    L.load()                                                 # a library that is not built is what is reported first
    frame, boxes, emb, xinv, score, sof = _row_inputs(frame, boxes, emb, xinv, score, stream_of_frame)
    n, B = frame.shape[0], sof.shape[0]
    S, D = state["hdr"].shape[0], state["emb"].shape[2]
    for k in STATE_KEYS:
        a = state[k]
        if not (isinstance(a, np.ndarray) and a.flags.c_contiguous and a.flags.writeable
                and a.dtype == (np.int32 if k in ("hdr", "slot_i") else np.float32)):
            raise ValueError(f"state[{k!r}] must be a writable C-contiguous numpy array of the state's dtype")
    if emb.ctypes.data % 16:                                 # numpy gives 16-byte alignment; a slice may not have it
        buf = np.empty((emb.size + 4,), np.float32)
        off = (-buf.ctypes.data % 16) // 4
        aligned = buf[off:off + emb.size].reshape(emb.shape)
        aligned[...] = emb
        emb = aligned
    sp, sv, mstate = _motion_args(motion, motion_state, S)
    pool = _reid_args(reid, lost_state, S, D, max_age)
    out = {k: np.zeros((n,), np.int32) for k in OUT_KEYS}
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)          # noqa: E731
    rows = (S, D, p(frame), p(boxes), p(emb), p(xinv), p(score), n, p(sof), B, int(max_age), float(tau_near), float(tau_far),
            float(iou_min), *[p(out[k]) for k in OUT_KEYS])
    tail = None
    if motion is not None:
        out["track_pred"] = np.zeros((n, 4), np.float32)
        tail = (p(mstate), float(sp), float(sv), p(out["track_pred"]))
    _step_call(_state_struct(state, p), None if pool is None else _lost_struct(pool, p), rows, tail, reid, True, None)
    return out


class StreamTracker:
    """n_streams independent streams, each with up to L.TRACK_SLOTS live tracks of feat_dim-float embeddings, on `device`.
    max_age: a track unseen for more than max_age frames of its stream is freed (required: nothing to restate).  The
    thresholds default to the reference's numbers as cosines (module docstring); tau_far < tau_near is a ValueError.
    motion: None, or a ConstantVelocity: the IoU gate takes the predicted box (fp_tracklets_step_motion), the state gains
    "motion" (n_streams, SLOTS, MOTION_FLOATS) and step() also returns track_pred.
    reid: None, or a LostPool with lost_age > max_age (ValueError otherwise): expired tracks are parked and a returning face
    takes its old id back (fp_tracklets_step_reid; its row carries REVIVED); the state gains the five LOST_KEYS arrays.
    templates: None, or a Templates: a template per track (fp_track_pool_step after the tracker's launch); the state gains the
    three TEMPLATE_KEYS arrays and step() also returns track_emb, track_emb_rows and track_emb_flags."""

    def __init__(self, n_streams, feat_dim, max_age, tau_near=TAU_NEAR, tau_far=TAU_FAR, iou_min=IOU_MIN, device="cuda:0",
                 motion=None, reid=None, templates=None):
        check_params(n_streams, feat_dim, max_age, tau_near, tau_far, iou_min)
        if motion is not None and not isinstance(motion, ConstantVelocity):
            raise TypeError(f"motion must be None or a ConstantVelocity, got {type(motion).__name__}")
        if reid is not None and not isinstance(reid, LostPool):
            raise TypeError(f"reid must be None or a LostPool, got {type(reid).__name__}")
        if reid is not None:
            reid.check(max_age)
        if templates is not None and not isinstance(templates, Templates):
            raise TypeError(f"templates must be None or a Templates, got {type(templates).__name__}")
        self.motion, self.reid, self.templates_opt = motion, reid, templates
        self.S, self.D, self.max_age = int(n_streams), int(feat_dim), int(max_age)
        self.tau_near, self.tau_far, self.iou_min = float(tau_near), float(tau_far), float(iou_min)
        self.dev = torch.device(device)
        self.state = {k: torch.from_numpy(v).to(self.dev) for k, v in new_state(self.S, self.D).items()}
        self._struct = _state_struct(self.state, L.ptr)
        if motion is not None:
            self.state["motion"] = torch.from_numpy(new_motion_state(self.S)).to(self.dev)
        if reid is not None:
            self.state.update({k: torch.from_numpy(v).to(self.dev) for k, v in new_lost_state(self.S, self.D).items()})
            self._lost = _lost_struct(self.state, L.ptr)
        if templates is not None:
            self.state.update({k: torch.from_numpy(v).to(self.dev) for k, v in new_template_state(self.S, self.D).items()})
            self._tpl = L.FpTrackTemplates(*[L.ptr(self.state[k]) for k in TEMPLATE_KEYS])
            self._tpl_ws = None

    @property
    def keep(self):
        """The clocks a template outlives its track's last row: lost_age with reid=, else max_age."""
        return self.reid.lost_age if self.reid is not None else self.max_age

    @property
    def state_keys(self):
        return (STATE_KEYS + (("motion",) if self.motion is not None else ()) + (LOST_KEYS if self.reid is not None else ())
                + (TEMPLATE_KEYS if self.templates_opt is not None else ()))

    def step(self, frame, boxes, emb, stream_of_frame, score=None, n=None, xinv=None):
        """One launch on the current stream.  frame (n,) int32 batch index of every face row, boxes (n, 4) fp32 (the
        info[:, 1:5] columns), emb (n, D) fp32, stream_of_frame (B,) int32 (-1: the frame is not tracked), score (n,) fp32
        or None; n: use the first n rows only (default: all); xinv: (n,) fp32 inverse norms of the rows of emb when the caller
        has them (default: fp_row_inv_norm here).  Device tensors; a frames / boxes tensor with a row stride (a
        column slice of info) is made contiguous.  -> dict(track_id, track_hits, track_clock, track_flags), (n,) int32 each;
        with motion= also track_pred (n, 4) fp32: the box a matched row's track was predicted at, zeros for every other row.
        With reid= a row that continues a parked track carries REVIVED in track_flags (never NEW) and the track's old id.
        With templates= also track_emb (n, D) fp32, track_emb_rows and track_emb_flags (n,) int32: the template of the row's
        track after the row (the row's own embedding and 0 rows where it has no track), two more launches."""
        n = int(emb.shape[0] if n is None else n)
        f32c = lambda t: t[:n].to(self.dev, torch.float32).contiguous()      # noqa: E731
        frame = frame[:n].to(self.dev, torch.int32).contiguous()
        boxes, emb = f32c(boxes), f32c(emb)
        sof = stream_of_frame.to(self.dev, torch.int32).contiguous()
        if tuple(emb.shape) != (n, self.D) or tuple(boxes.shape) != (n, 4) or frame.shape[0] != n or sof.dim() != 1:
            raise ValueError(f"expected {n} rows of frame, boxes (n, 4) and emb (n, {self.D}) and a 1-D stream_of_frame, got "
                             f"{tuple(frame.shape)} {tuple(boxes.shape)} {tuple(emb.shape)} {tuple(sof.shape)}")
        for name, t in (("score", score), ("xinv", xinv)):
            if t is not None and (t.dim() != 1 or t.shape[0] < n):
                raise ValueError(f"{name} must be a 1-D tensor of at least {n} rows, got {tuple(t.shape)}")
        score = None if score is None else f32c(score)
        out = {k: torch.empty((n,), dtype=torch.int32, device=self.dev) for k in OUT_KEYS}
        lib = L.load()
        if xinv is not None:
            xinv = f32c(xinv)
        elif n:
            xinv = torch.empty((n,), dtype=torch.float32, device=self.dev)
            L.check(lib.fp_row_inv_norm(L.ptr(emb), n, self.D, L.ptr(xinv), L.current_stream(self.dev)), "fp_row_inv_norm")
        rows = (self.S, self.D, L.ptr(frame), L.ptr(boxes), L.ptr(emb), L.ptr(xinv), L.ptr(score), n, L.ptr(sof), sof.shape[0],
                self.max_age, self.tau_near, self.tau_far, self.iou_min, *[L.ptr(out[k]) for k in OUT_KEYS])
        tail = None
        if self.motion is not None:
            out["track_pred"] = torch.empty((n, 4), dtype=torch.float32, device=self.dev)
            tail = (L.ptr(self.state["motion"]), self.motion.std_pos, self.motion.std_vel, L.ptr(out["track_pred"]))
        _step_call(self._struct, self._lost if self.reid is not None else None, rows, tail, self.reid, False,
                   L.current_stream(self.dev))
        if self.templates_opt is not None:
            out["track_emb"] = torch.empty((n, self.D), dtype=torch.float32, device=self.dev)
            out["track_emb_rows"] = torch.empty((n,), dtype=torch.int32, device=self.dev)
            out["track_emb_flags"] = torch.empty((n,), dtype=torch.int32, device=self.dev)
            need = lib.fp_track_pool_workspace_bytes(n)
            if self._tpl_ws is None or self._tpl_ws.numel() < need:
                self._tpl_ws = torch.empty((need,), dtype=torch.uint8, device=self.dev)
            weight = score if self.templates_opt.weighted else None
            if self.templates_opt.weighted and score is None:
                raise ValueError("Templates(weighted=True) needs the step's score")
            L.check(lib.fp_track_pool_step(C.byref(self._tpl), self.S, self.D, L.ptr(frame), L.ptr(emb), L.ptr(xinv), L.ptr(weight),
                                           n, L.ptr(sof), sof.shape[0], L.ptr(out["track_id"]), L.ptr(out["track_clock"]),
                                           L.ptr(out["track_flags"]), self.keep, *[L.ptr(out[k]) for k in TEMPLATE_OUT_KEYS],
                                           L.ptr(self._tpl_ws), self._tpl_ws.numel(), L.current_stream(self.dev)),
                    "fp_track_pool_step")
        return out

    def templates(self, stream):
        """The templates of one stream (a host read; ValueError without templates=): dict of numpy arrays entry, id, rows, wsum,
        last_clock and sum (k, D), in entry order."""
        if self.templates_opt is None:
            raise ValueError("this tracker keeps no templates (templates=)")
        s = int(stream)
        if not 0 <= s < self.S:
            raise ValueError(f"stream {stream} outside 0 .. {self.S - 1}")
        ti, tw, ts = (self.state[k][s].cpu().numpy() for k in TEMPLATE_KEYS)
        e = np.nonzero(ti[:, P_ID] != 0)[0]
        return dict(entry=e, id=ti[e, P_ID], rows=ti[e, P_ROWS], wsum=tw[e], last_clock=ti[e, P_LAST], sum=ts[e])

    def tracks(self, stream):
        """The live slots of one stream (a host read): dict of numpy arrays slot, id, first_clock, last_clock, hits, box,
        best_score, best_clock, best_box, best_emb, in slot order, and clock / next_id; with motion= also pred_box (the box the
        filter holds now: the prediction of the stream's last frame, or the update of a track matched in it) and velocity (the
        filter's v of cx, cy, w, h, per frame)."""
        s = int(stream)
        if not 0 <= s < self.S:
            raise ValueError(f"stream {stream} outside 0 .. {self.S - 1}")
        hdr, si, sf = (self.state[k][s].cpu().numpy() for k in ("hdr", "slot_i", "slot_f"))
        live = np.nonzero(si[:, I_ID] != 0)[0]
        t = dict(slot=live, id=si[live, I_ID], first_clock=si[live, I_FIRST], last_clock=si[live, I_LAST],
                 hits=si[live, I_HITS], box=sf[live, F_BOX:F_BOX + 4], best_score=sf[live, F_BEST_SCORE],
                 best_clock=si[live, I_BEST_CLOCK], best_box=sf[live, F_BEST_BOX:F_BEST_BOX + 4],
                 best_emb=self.state["best_emb"][s].cpu().numpy()[live], clock=int(hdr[0]), next_id=int(hdr[1]))
        if self.motion is not None:
            m = self.state["motion"][s].cpu().numpy()[live].reshape(len(live), 4, M_COLS)
            cx, cy, w, h = (m[:, c, M_X] for c in range(4))
            w, h = np.maximum(w, 0), np.maximum(h, 0)
            t["pred_box"] = np.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], axis=1).astype(np.float32)
            t["velocity"] = m[:, :, M_V].copy()
        return t

    def lost(self, stream):
        """The parked tracks of one stream (a host read; ValueError without reid=): dict of numpy arrays entry, id, first_clock,
        last_clock, hits, best_score, best_box, best_emb, in entry order."""
        if self.reid is None:
            raise ValueError("this tracker has no lost-track pool (reid=)")
        s = int(stream)
        if not 0 <= s < self.S:
            raise ValueError(f"stream {stream} outside 0 .. {self.S - 1}")
        li, lf = (self.state[k][s].cpu().numpy() for k in ("lost_i", "lost_f"))
        e = np.nonzero(li[:, I_ID] != 0)[0]
        return dict(entry=e, id=li[e, I_ID], first_clock=li[e, I_FIRST], last_clock=li[e, I_LAST], hits=li[e, I_HITS],
                    best_score=lf[e, F_BEST_SCORE], best_box=lf[e, F_BEST_BOX:F_BEST_BOX + 4],
                    best_emb=self.state["lost_best_emb"][s].cpu().numpy()[e])

    def reset(self, streams=None):
        """Forget the tracks, clocks and ids of `streams` (an iterable of stream indices; None: all)."""
        fresh = new_state(1, self.D)
        idx = slice(None) if streams is None else torch.as_tensor(list(streams), dtype=torch.long, device=self.dev)
        for k in STATE_KEYS:
            self.state[k][idx] = torch.from_numpy(fresh[k][0]).to(self.dev)
        if self.motion is not None:
            self.state["motion"][idx] = 0
        if self.reid is not None:
            for k in LOST_KEYS:
                self.state[k][idx] = 0
        if self.templates_opt is not None:
            for k in TEMPLATE_KEYS:
                self.state[k][idx] = 0

    def state_dict(self):
        """A copy of the device state and the parameters (host tensors)."""
        d = {k: v.detach().cpu().clone() for k, v in self.state.items()}
        d["params"] = dict(n_streams=self.S, feat_dim=self.D, max_age=self.max_age, tau_near=self.tau_near,
                           tau_far=self.tau_far, iou_min=self.iou_min)
        if self.motion is not None:
            d["params"].update(std_pos=self.motion.std_pos, std_vel=self.motion.std_vel)
        if self.reid is not None:
            d["params"].update(tau_reid=self.reid.tau_reid, lost_age=self.reid.lost_age)
        return d

    def load_state_dict(self, d):
        """The arrays of a state_dict of a tracker with the same n_streams and feat_dim (ValueError otherwise), copied into
        this tracker's own buffers; the parameters stay this tracker's.  A tracker with motion= needs the "motion" array too
        (KeyError without it); one without ignores it.  The same holds for the five LOST_KEYS arrays and reid=, and for the
        three TEMPLATE_KEYS arrays and templates=."""
        for k in self.state_keys:
            if tuple(d[k].shape) != tuple(self.state[k].shape):
                raise ValueError(f"state_dict[{k!r}] has shape {tuple(d[k].shape)}, this tracker {tuple(self.state[k].shape)}")
        for k in self.state_keys:
            self.state[k].copy_(torch.as_tensor(d[k]).to(self.state[k].dtype))

    def host_state(self):
        """The state as a dict of numpy arrays (new_state's layout, plus "motion" with motion= and the LOST_KEYS arrays with
        reid= and the TEMPLATE_KEYS arrays with templates=): what track_step_numpy / track_step_emulate and track_pool_numpy /
        track_pool_emulate continue from."""
        return {k: self.state[k].detach().cpu().numpy().copy() for k in self.state_keys}


class TrackBook:
    """A host-side record per (stream, id): first and last clock, hits, best score, best embedding and the frame and box of
    the best row.  Fed one step at a time from the NEW and BEST rows; sits outside the timed path (it reads the step's
    tensors back).  frame_base: what to add to a step's frame indices to number frames across steps."""

    def __init__(self):
        self.records = {}

    def update(self, out, frame, boxes, stream_of_frame, emb=None, score=None, frame_base=0, track_emb=None, track_emb_rows=None):
        """out: a step's four per-row arrays (dict; tensors or numpy); frame / boxes / emb / score / stream_of_frame: the
        step's inputs.  track_emb / track_emb_rows: the step's templates (a tracker with templates=); a record then keeps the
        latest of its track as `template` (D,) float32 and `template_rows`.  -> the keys (stream, id) the step touched."""
        host = lambda t: None if t is None else (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t))  # noqa: E731
        ids, hits, clocks, flags = (host(out[k]) for k in OUT_KEYS)
        frame, boxes, emb, score, sof = host(frame), host(boxes), host(emb), host(score), host(stream_of_frame)
        track_emb, track_emb_rows = host(track_emb), host(track_emb_rows)
        touched = []
        for i in range(len(ids)):
            if ids[i] <= 0:
                continue
            key = (int(sof[frame[i]]), int(ids[i]))
            rec = self.records.get(key)
            if rec is None or flags[i] & NEW:
                rec = self.records[key] = dict(stream=key[0], id=key[1], first_clock=int(clocks[i]), best_score=None,
                                               best_frame=None, best_box=None, best_emb=None, best_clock=None)
            rec["last_clock"], rec["hits"] = int(clocks[i]), int(hits[i])
            if flags[i] & BEST:
                rec["best_score"] = 0.0 if score is None else float(score[i])
                rec["best_frame"], rec["best_clock"] = int(frame_base) + int(frame[i]), int(clocks[i])
                rec["best_box"] = [float(v) for v in boxes[i]]
                rec["best_emb"] = None if emb is None else np.array(emb[i], np.float32)
            if track_emb is not None:
                rec["template"] = np.array(track_emb[i], np.float32)
                rec["template_rows"] = 0 if track_emb_rows is None else int(track_emb_rows[i])
            touched.append(key)
        return touched

    def __len__(self):
        return len(self.records)

    def __getitem__(self, key):
        return self.records[key]

    def rows(self):
        """The records in (stream, id) order."""
        return [self.records[k] for k in sorted(self.records)]
