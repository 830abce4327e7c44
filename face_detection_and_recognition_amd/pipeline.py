"""Batched detect -> crop -> embed -> similarity-filter pipeline, resident on one GPU.

This is the reference's own composition (face_extraction/extract_faces_from_dataset.py:270-307:
``net.inf_func`` -> ``bbox_conf_area_func`` -> crop with offsets -> ``get_face_features``) followed by the
similarity filter, run for a whole batch of frames at once: every stage is a HIP kernel launched on the
caller's stream and the only host round trip is reading the number of faces found (it sizes the embedder batch).
"""
import torch

from . import _lib as L
from . import quality as Q
from . import similarity as S
from .frames import batch_len, dets_to_crops
from .frames import ragged_scale_coords_params, scale_coords_params  # noqa: F401 (re-exports)
from .modules.mobile_facenet.utils import crops_to_input
from .modules.age_gender import age_gender_net as AG
from .modules.utils import align as A

FACE_OFFSETS = (-6, -1, 4, 5)   # tx, ty, bx, by  (extract_faces_from_dataset.py:285-287)


class FacePipeline:
    """detector: a BlazeFaceModel or YOLOV5FaceModel (HIP); embedder: a HIP MobileFaceNet or InceptionResnetV1 (FaceNet):
    the crops are resized to its ``input_size``, in its channel order (``swap_rb``), through its ``input_lut``;
    reference: (Nr, E) CUDA tensor of reference embeddings for the cosine filter (or None).
    align: feed the embedder each face warped onto the five-point template (modules/utils/align.py) instead of its
    stretched box crop; step results then also carry lmarks, align_M and align_flags.
    attributes: an AgeGenderNet (modules/age_gender): step results then also carry age_probs (n, 8) and gender_probs (n, 2),
    one row per face in the order of emb, from the reference's age / gender crops (fp_attr_crop_items); a face whose crop
    is empty gets NaN rows.  Under two_streams they run on the embedder's side stream.
    gallery: a FaceGallery (gallery.py): step results then also carry top_scores (n, top_k), top_idx (n, top_k) int32 gallery
    rows, identity (n,) int32 (-1: nobody enrolled reaches identify_tau; default tau) and identity_score (n,), one row per
    face in the order of emb, voted by `vote` ("top1" | "majority"); side stream as the attributes.
    quality: True or a QualityGate (quality.py): step results then also carry quality, the face_quality dict of the step's items
    (with align, the pose columns from its landmarks), rows in the order of emb, and, with a gate, quality_keep (n,) bool: its
    mask, which compacts nothing (as the cosine filter's keep); side stream as the attributes.
    tracker: a StreamTracker (tracking.py) whose feat_dim is the embedder's: step results then also carry track_id, track_hits,
    track_clock and track_flags (n,) int32, rows in the order of emb, from one fp_tracklets_step launch behind the embedder (side
    stream as the attributes); a tracker built with motion= adds track_pred (n, 4) fp32, the predicted box of every matched row; one built with reid= (a
    tracking.LostPool) gives a returning face its old id back, and that row's track_flags carry tracking.REVIVED (64) where an
    opening row carries NEW: the flags pass through unchanged.  step / step_overlapped take streams = the stream of every frame ((B,) ints, -1: not tracked;
    None: the batch is consecutive frames of stream 0).  The score of the best shot is the conf column of info, or
    quality["sharpness"] with quality on.  Steps must reach the tracker in order: it carries state from step to step.  A tracker
    built with templates= adds track_emb (n, D) fp32, track_emb_rows and track_emb_flags (n,) int32: the template of every row's
    track after the row (tracking.py; the row's own embedding where it has no track).
    identify_tracks: needs a gallery and a tracker with templates= (ValueError otherwise): step results then also carry
    track_identity, track_identity_score, track_top_scores and track_top_idx, the gallery's answer for track_emb (same top_k,
    identify_tau and vote), searched behind the tracker: who the TRACK is, which one turned or blurred frame does not change,
    beside the per-row identity keys, which stay.  What that gains on real video has not been measured."""

    # embed(): a batch a little above a multiple of ROUND_CROPS crops is run as that multiple + the remainder on a side stream
    ROUND_CROPS = 512     # crops whose tiles fill whole rounds of workgroups in every Depth_Wise kernel (2 / 4 / 7 tiles per crop, 512 slots)
    TAIL_MAX = 96         # largest remainder worth splitting off (measured: tools/lab/embed_split_probe.py)
    TAIL_CAP = 128        # capacity of the remainder's plan

    def __init__(self, detector, embedder, reference=None, tau=0.3, max_faces_per_frame=8, bucket=8, two_streams=False,
                 split_tail=True, align=False, attributes=None, gallery=None, top_k=5, identify_tau=None, vote="top1",
                 quality=None, tracker=None, identify_tracks=False):
        self.det = detector
        if tracker is not None and tracker.D != embedder.embedding_size:
            raise ValueError(f"tracker feat_dim {tracker.D} is not the embedder's {embedder.embedding_size}")
        self.tracker = tracker
        self.identify_tracks = bool(identify_tracks)
        if self.identify_tracks and (gallery is None or tracker is None or getattr(tracker, "templates_opt", None) is None):
            raise ValueError("identify_tracks needs gallery= and a tracker built with templates=")
        if not (quality is None or quality is True or isinstance(quality, Q.QualityGate)):
            raise ValueError(f"quality must be None, True or a QualityGate, got {quality!r}")
        self.quality = quality
        self.gallery, self.top_k, self.vote = gallery, int(top_k), vote
        self.identify_tau = float(tau if identify_tau is None else identify_tau)
        if gallery is not None and vote not in S.VOTE_MODES:
            raise ValueError(f"vote must be one of {sorted(S.VOTE_MODES)}, got {vote!r}")
        self.attr = attributes
        self.align = bool(align)
        self.emb = embedder
        self.tau = float(tau)
        self.max_faces_per_frame = int(max_faces_per_frame)
        self.bucket = int(bucket)
        self.dev = embedder._device()
        self.in_w, self.in_h = embedder.input_size
        self.swap_rb = bool(embedder.swap_rb)
        self.lut = embedder.input_lut(self.dev)
        if self.align and (self.in_w, self.in_h) != (L.ALIGN_SIZE, L.ALIGN_SIZE):
            raise ValueError(f"align=True warps faces onto the {L.ALIGN_SIZE} x {L.ALIGN_SIZE} template; the embedder takes "
                             f"{self.in_w} x {self.in_h}")
        # step_overlapped with two_streams: embed + filter of batch k run on a SIDE stream beside the detector of batch
        # k + 1 (the split-MFMA embedder kernels are matrix-core bound, the BlazeFace kernels vector-ALU / HBM bound, and
        # every kernel's last, partly empty round of workgroups is filled by the other stream's work)
        self.emb_stream = torch.cuda.Stream(device=self.dev) if two_streams else None
        self.split_tail = bool(split_tail)
        self.tail_stream = torch.cuda.Stream(device=self.dev) if split_tail else None
        net = getattr(detector, "net", None)
        self._co_net = net if hasattr(net, "co_scheduled") else None     # BlazeFace: no whole-CU ops beside the embedder's kernels
        self.set_reference(reference)

    def set_reference(self, reference):
        self.reference = None if reference is None else reference.to(self.dev, torch.float32).contiguous()
        self.rinv = None if reference is None else S.row_inv_norm(self.reference)
        # the reference set split once into bf16 planes for the split-MFMA cosine kernel (similarity.split3_rows)
        self.ref3 = None if reference is None or self.reference.shape[1] % 32 else S.split3_rows(self.reference)

    # -- stages ----------------------------------------------------------------------------------
    def detect(self, frames, max_det=-1, beside=False):
        """frames (B, H, W, 3) u8 BGR on device or a RaggedFrames -> (dets, counts, overflow or None).  max_det: -1 = the detector's
        default cap, None = uncapped (the exact re-run after an overflow).  beside: the detector's kernels will run
        beside the embedder's on the other stream (step_overlapped with two_streams)."""
        if self._co_net is not None:      # selects the plan (blazeface.py plan_for): several pipelines may share one detector
            self._co_net.co_scheduled = bool(beside)
        out = self.det.raw_batch(frames) if max_det == -1 else self.det.raw_batch(frames, max_det=max_det)
        return out if len(out) == 3 else (out[0], out[1], None)

    def crops(self, frames, dets, counts):
        """Device-side B7 + crop arithmetic -> (items, info, n_faces tensor).  frames: (B, H, W, 3) or a RaggedFrames
        (each frame's boxes in its own pixels: per-frame scale_coords values, the same fp32 numbers as a frame alone).
        With align: (items, info, n_faces, al), al = dict(lmarks, M, flags) of fp_dets_to_crops_aligned."""
        out = self._crops(frames, dets, counts)
        return out if self.align else out[:3]

    def _crops(self, frames, dets, counts):
        cap = batch_len(frames) * self.max_faces_per_frame
        al = A.alloc(cap, self.dev) if self.align else None
        dst = (L.ALIGN_SIZE, L.ALIGN_SIZE) if self.align else (self.in_w, self.in_h)
        return dets_to_crops(frames, dets, counts, self.det, dst, cap, FACE_OFFSETS, al) + (al,)

    def _to_input(self, frames, items, n, canvas, al, info, start=0):
        """The embedder input of faces start .. start + n: the box crops (crops_to_input), or with al the aligned faces."""
        if al is None:
            crops_to_input(frames, items[start:] if start else items, n, canvas, self.lut, swap_rb=self.swap_rb)
        else:
            A.warp(frames, al["M"][start:], info[start:], al["flags"][start:], items[start:], n, out_f32=canvas, lut=self.lut)

    def embed(self, frames, items, n_faces, al=None, info=None):
        """Crop + resize + normalise into the embedder's input, run the embedder.  -> (n_faces, E), a view into the
        embedder plan's arena.  ONE plan (arena sized for the largest batch seen, in steps of 256 crops) serves every
        face count: it runs on the first n_pad = n_faces rounded up to `bucket` images (8 keeps the 14x14 layers'
        row count a multiple of the 32-row MFMA tiles the streaming 1x1 kernels need), so at most bucket - 1 crops of
        work are padding and a varying face count neither builds new plans nor pins new arenas.
        al / info: the aligned crops' outputs (crops() with align): the input is the aligned faces (fp_align_warp)."""
        if n_faces == 0:
            return torch.zeros((0, self.emb.embedding_size), device=self.dev)
        n_pad = (n_faces + self.bucket - 1) // self.bucket * self.bucket
        cap = max(getattr(self, "_emb_cap", 0), (n_pad + 255) // 256 * 256)
        self._emb_cap = cap
        plan = self.emb.plan_for(cap, n_run=n_pad)
        self.emb_key, self.emb_n_pad = (cap, n_pad), n_pad     # the plan itself stays owned by the embedder's LRU cache
        main = n_pad // self.ROUND_CROPS * self.ROUND_CROPS
        if self.split_tail and main and 0 < n_pad - main <= self.TAIL_MAX and main < n_faces:
            return self._embed_split(frames, items, n_faces, n_pad, main, plan, al, info)
        self._to_input(frames, items, n_faces, plan.input, al, info)
        if n_pad > n_faces:
            plan.input[n_faces:n_pad].zero_()    # padding crops: defined inputs (every op is per-image, their rows are dropped)
        plan.run(n=n_pad)
        return plan.out[:n_faces]

    def _embed_split(self, frames, items, n_faces, n_pad, main, plan, al=None, info=None):
        """~528 crops are 1056 band tiles of a 14 x 14 Depth_Wise kernel on 512 workgroup slots: two full rounds and a third
        with 32 tiles, in EVERY launch (28 x 28: 2112 tiles, 56 x 56: 3696) -- the last 16 crops cost 0.25 ms of a 2.3 ms
        forward.  The first `main` crops (whole rounds in every kernel) run on the current stream, the remainder as its own
        small forward on a side stream beside them (its own plan / arena): 2.30 -> 2.16 ms alone on the GPU.  Every op is
        per-image and kernels do not depend on the batch, so the rows are bit-identical to the one-run form
        (tests: test_embedder_split_tail_is_bit_identical).  Returns a new (n_faces, E) tensor."""
        rem, rem_pad = n_faces - main, n_pad - main
        tail = self.emb.plan_for(self.TAIL_CAP, n_run=rem_pad)
        cur = torch.cuda.current_stream(self.dev)
        ready = torch.cuda.Event()
        ready.record(cur)
        with torch.cuda.stream(self.tail_stream):
            self.tail_stream.wait_event(ready)           # items / frames are complete (and the tail plan's previous consumer is done)
            frames.record_stream(self.tail_stream)
            items.record_stream(self.tail_stream)
            if al is not None:
                for t in (info, al["M"], al["flags"]):
                    t.record_stream(self.tail_stream)
            self._to_input(frames, items, rem, tail.input, al, info, start=main)
            if rem_pad > rem:
                tail.input[rem:rem_pad].zero_()
            tail.run(n=rem_pad)
            done = torch.cuda.Event()
            done.record(self.tail_stream)
        self._to_input(frames, items, main, plan.input, al, info)
        plan.run(n=main)
        cur.wait_event(done)
        return torch.cat([plan.out[:main], tail.out[:rem]])

    @property
    def emb_plan(self):
        """The embedder plan of the last step (looked up in the embedder's plan cache; not held by the pipeline)."""
        cap, n_pad = self.emb_key
        return self.emb.plan_for(cap, n_run=n_pad)

    # -- software-pipelined form ----------------------------------------------------------------------
    def step_overlapped(self, frames, streams=None):
        """step() with the host round trip taken off the GPU's critical path: this call ENQUEUES the detector stages of
        `frames` and then finishes the PREVIOUS call's batch (embed + filter), whose face count -- produced a whole
        detector pass ago -- is already on the host when it is read (pinned buffer + event).  The GPU queue never drains
        while the host waits.  Returns the previous batch's result dict (None on the first call); flush() returns the
        last one.  Same kernels, same numbers as step(); a detector overflow (more survivors than the cap in some frame)
        falls back to the exact un-capped re-run for that batch."""
        dets, counts, over = self.detect(frames, beside=self.emb_stream is not None)
        items, info, nf, al = self._crops(frames, dets, counts)
        # two pinned count buffers, used alternately: at most one batch is pending while the previous one's is read
        if getattr(self, "_host_counts", None) is None:
            self._host_counts, self._host_k = [torch.empty((2,), dtype=torch.int32).pin_memory() for _ in range(2)], 0
        host = self._host_counts[self._host_k & 1]
        self._host_k += 1
        self._counts_to_host(nf, over, host)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.dev))
        prev, self._pending = getattr(self, "_pending", None), (frames, (items, info, nf, al), host, ev, streams)
        return None if prev is None else self._finish(prev)

    def flush(self):
        """Finish the batch a previous step_overlapped() call left pending (None if there is none)."""
        prev, self._pending = getattr(self, "_pending", None), None
        return None if prev is None else self._finish(prev)

    @staticmethod
    def _counts_to_host(nf, over, host=None):
        """[faces found, frames whose detections overflowed the detector's cap (0 for a detector without one)] in one host
        transfer: enqueued into the pinned (2,) `host`, or (host None) read now -- the one host sync of step()."""
        both = nf if over is None else torch.stack([nf[0], over.sum().to(torch.int32)])
        if host is None:
            return (both.tolist() + [0])[:2]
        host[1] = 0
        host[:both.numel()].copy_(both, non_blocking=True)

    def _result(self, frames, crops, n, n_over, side=None, streams=None):
        """The step's result dict from the crop stage's outputs and the two host counts: the exact re-run after a detector
        overflow, the cap check, embed, filter, attributes, identity, alignment records.  side = (stream, event the crops are
        complete at): embed and everything after it run there and the dict carries the event `done` (_finish)."""
        items, info, _, al = crops
        if n_over:                              # > MAX_DET survivors in some frame: exact re-run without a cap
            dets, counts, _ = self.detect(frames, max_det=None)
            items, info, nf, al = self._crops(frames, dets, counts)
            n = int(nf.item())
        cap = items.shape[0]
        if n > cap:
            raise L.FacepathError(f"{n} faces in the batch exceed max_faces_per_frame*B = {cap}")

        def tail():
            emb = self.embed(frames, items, n, al, info)
            res = self.filter(emb)
            out = dict(n_faces=n, info=info[:n], emb=emb.clone(), items=items[:n])
            self._add_attributes(out, frames, info, n)
            self._add_identity(out)
            if self.quality is not None:
                self._add_quality(out, frames, items, al, n)
            if self.tracker is not None:
                self._add_tracks(out, batch_len(frames), streams)
            return out, res
        if side is None:
            out, res = tail()
        else:
            out, res = self._on_side_stream(tail, side, (frames, items, info) + (() if al is None else tuple(al.values())))
        self._add_align(out, al, n)
        if res is not None:
            out.update(best=res[0], arg=res[1], keep=res[2])
        return out

    def _on_side_stream(self, tail, side, inputs):
        """tail() on the side stream, ordered after the crops' event and before the caller's next use of the main stream."""
        stream, ev = side
        main = torch.cuda.current_stream(self.dev)
        stream.wait_event(ev)                          # the crops of this batch (detector stream)
        if getattr(self, "_emb_done", None) is not None:
            main.wait_event(self._emb_done)            # (results of the batch before are complete for the caller)
        with torch.cuda.stream(stream):
            for t in inputs:
                t.record_stream(stream)
            out, res = tail()
            # allocated on the side stream, consumed by the caller on the main stream (after `done`): tell the caching
            # allocator, or it hands the blocks to the next embed / filter while main-stream reads are still queued
            attrs = tuple(out[k] for k in ("age_probs", "gender_probs") + self.IDENTITY_KEYS if k in out)
            if self.quality is not None:
                attrs += tuple(out["quality"].values()) + ((out["quality_keep"],) if "quality_keep" in out else ())
            attrs += tuple(out[k] for k in self.TRACK_RESULT_KEYS if k in out)
            for t in (out["emb"],) + attrs + (tuple(res) if res is not None else ()):
                t.record_stream(main)
            self._emb_done = torch.cuda.Event()
            self._emb_done.record(stream)
        out["done"] = self._emb_done                   # the caller waits for this event before it reads the results
        return out, res

    def _finish(self, pending):
        frames, crops, host, ev, streams = pending
        ev.synchronize()
        return self._result(frames, crops, int(host[0]), int(host[1]), None if self.emb_stream is None else (self.emb_stream, ev),
                            streams)

    ATTR_CAP_STEP = 64    # the attribute plan's capacity grows in steps of this many crops (about 3.8 MB of arena each)

    def attributes_of(self, frames, info, n):
        """(age_probs (n, 8), gender_probs (n, 2)) of the first n face rows of info: the reference's age / gender crops, both
        nets in one plan run on the first n rounded up to `bucket` crops.  New tensors; NaN rows for empty crops."""
        net = self.attr
        if n == 0:
            return (torch.zeros((0, net.n_age), device=self.dev), torch.zeros((0, net.n_gender), device=self.dev))
        items = AG.attr_crop_items(info, n, frames, dst=net.input_size)
        n_pad = (n + self.bucket - 1) // self.bucket * self.bucket
        cap = max(getattr(self, "_attr_cap", 0), (n_pad + self.ATTR_CAP_STEP - 1) // self.ATTR_CAP_STEP * self.ATTR_CAP_STEP)
        self._attr_cap = cap
        age, gender = AG.run_on_items(net, frames, items, n, n_pad, net.plan_for(cap))
        return AG.nan_empty(age, items), AG.nan_empty(gender, items)

    def _add_attributes(self, out, frames, info, n):
        if self.attr is not None:
            out["age_probs"], out["gender_probs"] = self.attributes_of(frames, info, n)

    IDENTITY_KEYS = ("top_scores", "top_idx", "identity", "identity_score")

    def _add_identity(self, out):
        """The gallery's answer for the step's embeddings (rows in the order of emb); nothing without a gallery."""
        if self.gallery is None:
            return
        k = self.top_k
        if out["n_faces"] == 0:
            out.update(top_scores=torch.zeros((0, k), device=self.dev), top_idx=torch.zeros((0, k), dtype=torch.int32, device=self.dev),
                       identity=torch.zeros((0,), dtype=torch.int32, device=self.dev), identity_score=torch.zeros((0,), device=self.dev))
            return
        r = self.gallery.identify(out["emb"], k=k, tau=self.identify_tau, vote=self.vote)
        out.update(top_scores=r["top_scores"], top_idx=r["top_idx"], identity=r["label"], identity_score=r["score"])

    def _add_quality(self, out, frames, items, al, n):
        """The face_quality dict of the step's items (with align: the pose columns from its landmarks) and the gate's mask."""
        lm = None if al is None else al["lmarks"]
        out["quality"] = Q.face_quality(frames, items, n, lmarks=lm, fmt=None if al is None else self.det.dets_fmt)
        if self.quality is not True:
            out["quality_keep"] = self.quality.mask(out["quality"])

    TRACK_KEYS = ("track_id", "track_hits", "track_clock", "track_flags")
    TRACK_IDENTITY_KEYS = ("track_top_scores", "track_top_idx", "track_identity", "track_identity_score")
    # track_pred: only from a tracker with motion=; track_emb*: with templates=; the last four: with identify_tracks
    TRACK_RESULT_KEYS = TRACK_KEYS + ("track_pred", "track_emb", "track_emb_rows", "track_emb_flags") + TRACK_IDENTITY_KEYS

    def _stream_of_frame(self, B, streams):
        """(B,) int32 on the device: zeros for None (small cache by B), else the caller's streams."""
        if streams is None:
            cache = self.__dict__.setdefault("_stream0", {})
            if B not in cache:
                cache[B] = torch.zeros((B,), dtype=torch.int32, device=self.dev)
            return cache[B]
        sof = torch.as_tensor(streams, dtype=torch.int32).reshape(-1)
        if sof.shape[0] != B:
            raise ValueError(f"streams has {sof.shape[0]} entries for a batch of {B} frames")
        return sof.to(self.dev, non_blocking=True)

    def _add_tracks(self, out, B, streams):
        """One tracker launch over the step's rows (info's frame and box columns, emb, the score)."""
        n, info = out["n_faces"], out["info"]
        score = out["quality"]["sharpness"] if self.quality is not None else info[:, 5]
        out.update(self.tracker.step(info[:, 0], info[:, 1:5], out["emb"], self._stream_of_frame(B, streams), score=score, n=n))
        if self.identify_tracks:
            k = self.top_k
            if n == 0:
                out.update(track_top_scores=torch.zeros((0, k), device=self.dev),
                           track_top_idx=torch.zeros((0, k), dtype=torch.int32, device=self.dev),
                           track_identity=torch.zeros((0,), dtype=torch.int32, device=self.dev),
                           track_identity_score=torch.zeros((0,), device=self.dev))
                return
            r = self.gallery.identify(out["track_emb"], k=k, tau=self.identify_tau, vote=self.vote)
            out.update(track_top_scores=r["top_scores"], track_top_idx=r["top_idx"], track_identity=r["label"],
                       track_identity_score=r["score"])

    @staticmethod
    def _add_align(out, al, n):
        if al is not None:
            out.update(lmarks=al["lmarks"][:n], align_M=al["M"][:n], align_flags=al["flags"][:n])

    def filter(self, emb):
        if self.reference is None or emb.shape[0] == 0:
            return None
        return S.cosine_filter(emb, self.reference, self.tau, rinv=self.rinv, r3=self.ref3)

    def annotate(self, frames, result, **kw):
        """The frames of a finished step with its result drawn on: annotate.annotate_step(frames, result, **kw) (names,
        anonymize, inplace); names default to the gallery's.  A call of the user's, outside the timed path."""
        from .annotate import annotate_step
        if self.gallery is not None:
            kw.setdefault("names", self.gallery.names)
        return annotate_step(frames, result, **kw)

    # -- whole step ------------------------------------------------------------------------------
    def step(self, frames, beside=False, streams=None):
        """One pass over a batch of frames ((B, H, W, 3) u8 BGR on device, or a RaggedFrames of different sizes).
        Returns dict(n_faces, info, emb, best, arg, keep).
        ``emb`` is a copy (the embedder's output lives in its plan arena and the next step overwrites it).
        beside: use the detector plan of the two-stream steps (measurement: bench.py's per-op probe pass)."""
        dets, counts, over = self.detect(frames, beside=beside)
        crops = self._crops(frames, dets, counts)
        n, n_over = self._counts_to_host(crops[2], over)     # (the face count sizes the embedder batch)
        return self._result(frames, crops, n, n_over, streams=streams)
