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
they are the reference's numbers, unmeasured on real video.  max_age has no reference counterpart and no default.  Motion
prediction (Kalman, constant velocity) is not part of this.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L

SLOTS, MAX_DETS = L.TRACK_SLOTS, L.TRACK_MAX_DETS
NEW, BEST, DEAD_ROW, FULL, NO_STREAM, OVER = (L.TRACK_NEW, L.TRACK_BEST, L.TRACK_DEAD_ROW, L.TRACK_FULL, L.TRACK_NO_STREAM,
                                              L.TRACK_OVER)
TAU_NEAR, TAU_FAR, IOU_MIN = 0.5, 0.7408, 0.1        # the reference's 1.0 / 0.72 L2 thresholds as cosines, and its IoU gate
I_ID, I_FIRST, I_LAST, I_HITS, I_BEST_CLOCK = range(5)      # slot_i columns
F_BOX, F_INV, F_BEST_SCORE, F_BEST_BOX = 0, 4, 5, 6         # slot_f columns
STATE_KEYS = ("hdr", "slot_i", "slot_f", "emb", "best_emb")
OUT_KEYS = ("track_id", "track_hits", "track_clock", "track_flags")


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
                     iou_min=IOU_MIN, score=None, cosines=None):
    """fp_tracklets_step in numpy on a host state (new_state; updated IN PLACE).  IoU in float32 in the written order, the
    cosine in float64: (dot * inv_t) * inv_d with float64 products of the float32 values.  -> dict of the four per-row int32
    arrays.  cosines: a list that receives, per frame with live tracks and live detections, (frame, slots, rows, c (T, K)
    float64, iou (T, K) float32, the tracks' stored rows (T, D)) -- what the tests' gap condition looks at."""
    frame, boxes, emb, xinv, score, sof = _row_inputs(frame, boxes, emb, xinv, score, stream_of_frame)
    n, B = frame.shape[0], sof.shape[0]
    S, D = state["hdr"].shape[0], state["emb"].shape[2]
    check_params(S, D, max_age, tau_near, tau_far, iou_min)
    f32 = np.float32
    tn, tf, im = float(f32(tau_near)), float(f32(tau_far)), f32(iou_min)
    out = {k: np.zeros((n,), np.int32) for k in OUT_KEYS}
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
            si[(si[:, I_ID] != 0) & (clock - si[:, I_LAST] > max_age), I_ID] = 0
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
                iou = np.stack([_iou_f32(sf[t, F_BOX:F_BOX + 4], boxes[dets]) for t in slots])
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
            for i in dets:
                i = int(i)
                slot, is_new = taken.get(i), False
                if slot is None:
                    free = np.nonzero(si[:, I_ID] == 0)[0]
                    if not len(free):
                        out["track_clock"][i], out["track_flags"][i] = clock, FULL
                        continue
                    slot, is_new = int(free[0]), True
                    si[slot, I_ID], si[slot, I_FIRST], si[slot, I_HITS] = hdr[1], clock, 0
                    hdr[1] += 1
                sc = f32(0) if score is None else score[i]
                si[slot, I_HITS] += 1
                si[slot, I_LAST] = clock
                sf[slot, F_BOX:F_BOX + 4], sf[slot, F_INV] = boxes[i], xinv[i]
                flags = NEW if is_new else 0
                if is_new or sc > sf[slot, F_BEST_SCORE]:
                    sf[slot, F_BEST_SCORE], si[slot, I_BEST_CLOCK] = sc, clock
                    sf[slot, F_BEST_BOX:F_BEST_BOX + 4] = boxes[i]
                    flags |= BEST
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


def track_step_emulate(state, frame, boxes, emb, xinv, stream_of_frame, max_age, tau_near=TAU_NEAR, tau_far=TAU_FAR,
                       iou_min=IOU_MIN, score=None):
    """fp_tracklets_step_emulate on a host state (new_state; updated IN PLACE): track_step_numpy's arguments and results.
    Raises FacepathError on a refusal.  Needs no GPU."""
    lib = L.load()
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
    out = {k: np.zeros((n,), np.int32) for k in OUT_KEYS}
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)          # noqa: E731
    st = _state_struct(state, p)
    L.check(lib.fp_tracklets_step_emulate(C.byref(st), S, D, p(frame), p(boxes), p(emb), p(xinv), p(score), n, p(sof), B,
                                          int(max_age), float(tau_near), float(tau_far), float(iou_min),
                                          *[p(out[k]) for k in OUT_KEYS]), "fp_tracklets_step_emulate")
    return out


class StreamTracker:
    """n_streams independent streams, each with up to L.TRACK_SLOTS live tracks of feat_dim-float embeddings, on `device`.
    max_age: a track unseen for more than max_age frames of its stream is freed (required: nothing to restate).  The
    thresholds default to the reference's numbers as cosines (module docstring); tau_far < tau_near is a ValueError."""

    def __init__(self, n_streams, feat_dim, max_age, tau_near=TAU_NEAR, tau_far=TAU_FAR, iou_min=IOU_MIN, device="cuda:0"):
        check_params(n_streams, feat_dim, max_age, tau_near, tau_far, iou_min)
        self.S, self.D, self.max_age = int(n_streams), int(feat_dim), int(max_age)
        self.tau_near, self.tau_far, self.iou_min = float(tau_near), float(tau_far), float(iou_min)
        self.dev = torch.device(device)
        self.state = {k: torch.from_numpy(v).to(self.dev) for k, v in new_state(self.S, self.D).items()}
        self._struct = _state_struct(self.state, L.ptr)

    def step(self, frame, boxes, emb, stream_of_frame, score=None, n=None, xinv=None):
        """One launch on the current stream.  frame (n,) int32 batch index of every face row, boxes (n, 4) fp32 (the
        info[:, 1:5] columns), emb (n, D) fp32, stream_of_frame (B,) int32 (-1: the frame is not tracked), score (n,) fp32
        or None; n: use the first n rows only (default: all); xinv: (n,) fp32 inverse norms of the rows of emb when the caller
        has them (default: fp_row_inv_norm here).  Device tensors; a frames / boxes tensor with a row stride (a
        column slice of info) is made contiguous.  -> dict(track_id, track_hits, track_clock, track_flags), (n,) int32 each."""
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
        L.check(lib.fp_tracklets_step(C.byref(self._struct), self.S, self.D, L.ptr(frame), L.ptr(boxes), L.ptr(emb), L.ptr(xinv),
                                      L.ptr(score), n, L.ptr(sof), sof.shape[0], self.max_age, self.tau_near, self.tau_far,
                                      self.iou_min, *[L.ptr(out[k]) for k in OUT_KEYS], L.current_stream(self.dev)),
                "fp_tracklets_step")
        return out

    def tracks(self, stream):
        """The live slots of one stream (a host read): dict of numpy arrays slot, id, first_clock, last_clock, hits, box,
        best_score, best_clock, best_box, best_emb, in slot order, and clock / next_id."""
        s = int(stream)
        if not 0 <= s < self.S:
            raise ValueError(f"stream {stream} outside 0 .. {self.S - 1}")
        hdr, si, sf = (self.state[k][s].cpu().numpy() for k in ("hdr", "slot_i", "slot_f"))
        live = np.nonzero(si[:, I_ID] != 0)[0]
        return dict(slot=live, id=si[live, I_ID], first_clock=si[live, I_FIRST], last_clock=si[live, I_LAST],
                    hits=si[live, I_HITS], box=sf[live, F_BOX:F_BOX + 4], best_score=sf[live, F_BEST_SCORE],
                    best_clock=si[live, I_BEST_CLOCK], best_box=sf[live, F_BEST_BOX:F_BEST_BOX + 4],
                    best_emb=self.state["best_emb"][s].cpu().numpy()[live], clock=int(hdr[0]), next_id=int(hdr[1]))

    def reset(self, streams=None):
        """Forget the tracks, clocks and ids of `streams` (an iterable of stream indices; None: all)."""
        fresh = new_state(1, self.D)
        idx = slice(None) if streams is None else torch.as_tensor(list(streams), dtype=torch.long, device=self.dev)
        for k in STATE_KEYS:
            self.state[k][idx] = torch.from_numpy(fresh[k][0]).to(self.dev)

    def state_dict(self):
        """A copy of the device state and the parameters (host tensors)."""
        d = {k: v.detach().cpu().clone() for k, v in self.state.items()}
        d["params"] = dict(n_streams=self.S, feat_dim=self.D, max_age=self.max_age, tau_near=self.tau_near,
                           tau_far=self.tau_far, iou_min=self.iou_min)
        return d

    def load_state_dict(self, d):
        """The arrays of a state_dict of a tracker with the same n_streams and feat_dim (ValueError otherwise), copied into
        this tracker's own buffers; the parameters stay this tracker's."""
        for k in STATE_KEYS:
            if tuple(d[k].shape) != tuple(self.state[k].shape):
                raise ValueError(f"state_dict[{k!r}] has shape {tuple(d[k].shape)}, this tracker {tuple(self.state[k].shape)}")
        for k in STATE_KEYS:
            self.state[k].copy_(torch.as_tensor(d[k]).to(self.state[k].dtype))

    def host_state(self):
        """The state as a dict of numpy arrays (new_state's layout): what track_step_numpy / track_step_emulate continue from."""
        return {k: self.state[k].detach().cpu().numpy().copy() for k in STATE_KEYS}


class TrackBook:
    """A host-side record per (stream, id): first and last clock, hits, best score, best embedding and the frame and box of
    the best row.  Fed one step at a time from the NEW and BEST rows; sits outside the timed path (it reads the step's
    tensors back).  frame_base: what to add to a step's frame indices to number frames across steps."""

    def __init__(self):
        self.records = {}

    def update(self, out, frame, boxes, stream_of_frame, emb=None, score=None, frame_base=0):
        """out: a step's four per-row arrays (dict; tensors or numpy); frame / boxes / emb / score / stream_of_frame: the
        step's inputs.  -> the keys (stream, id) the step touched."""
        host = lambda t: None if t is None else (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t))  # noqa: E731
        ids, hits, clocks, flags = (host(out[k]) for k in OUT_KEYS)
        frame, boxes, emb, score, sof = host(frame), host(boxes), host(emb), host(score), host(stream_of_frame)
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
            touched.append(key)
        return touched

    def __len__(self):
        return len(self.records)

    def __getitem__(self, key):
        return self.records[key]

    def rows(self):
        """The records in (stream, id) order."""
        return [self.records[k] for k in sorted(self.records)]
