"""Batched detect -> crop -> embed for media items, with the reference's on-disk feature format
(face_detection_and_extraction/face_extraction/extract_faces_from_dataset.py:270-365).

  extract_face_feat_conf_area_list(pipe, frames)  :270-307  (here: a whole batch of frames per call, on device)
  extract_faces_from_images(pipe, paths)          :400-407  (image media items of any size, batch by batch)
  save_extracted_faces(...)                       :311-363  (same annot dict, zero-padded feature vector, np.save)

Face crops as JPEG files (:346-349, cv2.imwrite): extract_face_feat_conf_area_list(..., save_face=True) encodes every crop of the
batch on the device in one call (modules/utils/jpeg.py encode_crops, byte-identical to cv2.imwrite's libjpeg-turbo output at
quality 95) and keeps each frame's files in FrameFacesObj.face_jpegs; save_extracted_faces(..., save_face=True,
faces_save_dir=...) writes them under the reference's file names.  The reference saves faces unless --noface is given; here
save_face defaults to False, so a caller that does not ask for crops gets exactly the feature files as before.  The
directory follows the reference's driver (:395-409): <target>/faces/<class_name> for images, .../<media_root> for videos.

The reference walks a dataset one frame at a time through a Net wrapper; this module is the SURVEY 8(f) rank-1
"next" row: the same composition driven by pipeline.FacePipeline, so detection, cropping and embedding of all frames
of a media item are three device-resident stages.  Directory walking / video decoding stay with the caller (a Motion-JPEG
file's frames come batch by batch from modules/utils/video.py's VideoReader.batches)."""
import os
from dataclasses import dataclass, field
from typing import List

import numpy as np

from ..frames import as_frames

MAX_N_FACES_PER_FRAME = 3      # extract_faces_from_dataset.py:38
MAX_N_FRAME_FROM_VID = 15      # :40


@dataclass
class FrameFacesObj:
    """One frame's faces (the reference's FrameFacesObj record)."""
    frame_num: int
    time_sec: float
    confs: List[float]
    areas: List[float]
    boxes: np.ndarray
    feats: List[np.ndarray] = field(default_factory=list)
    face_jpegs: List[bytes] = field(default_factory=list)   # save_face=True: each face's JPEG file (None: an empty crop)
    track_ids: List[int] = field(default_factory=list)      # tracker=...: each face's track id (0: none); else empty


def extract_face_feat_conf_area_list(pipe, frames, frame_nums=None, times_sec=None, save_face=False,
                                     quality=95, align=False, quality_gate=None, tiled=None, tracker=None,
                                     streams=None, augment=None) -> List[FrameFacesObj]:
    """frames: (B, H, W, 3) u8 BGR (numpy or CUDA tensor), a RaggedFrames, or a list of (h, w, 3) frames.  One FacePipeline
    step (no similarity filter needed); returns per-frame records with boxes (each frame's own pixels, rounded), confs,
    area fractions and embeddings.  A list whose frames share one size is stacked and takes the uniform path; otherwise it
    is packed into a RaggedFrames.  save_face: also encode every face crop (the reference's image[y:yh, x:xw]) to a JPEG
    file of that quality, in one device call.  align: embed each face warped onto the five-point template
    (FacePipeline(align=True) for this call, modules/utils/align.py); with save_face the files are then the 112 x 112
    aligned faces the embedder saw (as u8), under the same names.  quality_gate: a quality.QualityGate; every face is measured
    (quality.face_quality on the step's items, with its landmarks when the step is aligned) and the faces that fail the gate
    are left out of the records -- before save_extracted_faces applies the per-frame face cap, so a frame's
    MAX_N_FACES_PER_FRAME slots go to usable faces.  A gate with a pose term needs align (ValueError otherwise).
    tiled: dict(tile=(w, h), overlap=(ox, oy), merge_thr=t[, edge_px, full_frame, max_det]): for this call the pipeline's
    detector runs on overlapping tiles of every frame as well (tiling.TiledDetector over pipe.det; merge_thr has no default).
    tracker: a tracking.StreamTracker: for this call the step also tracks its faces (streams: the stream of every frame, None =
    consecutive frames of stream 0) and every record carries track_ids, one per face; calls must come in video order.
    augment: True / False: for this call the pipeline's YOLOv5-face detector runs with / without augmented inference (the
    reference's three views behind one NMS; ValueError for a detector without it); None leaves the detector as it is."""
    if isinstance(frames, (list, tuple)) and not frames:
        return []
    frames = as_frames(frames, pipe.dev)
    B = len(frames)
    was = (pipe.det, pipe.align, pipe.tracker)
    base_det, was_augment = pipe.det, getattr(pipe.det, "augment", None)
    if augment is not None and was_augment is None:
        raise ValueError(f"augment= needs a YOLOv5-face detector; {type(pipe.det).__name__} has no augmented inference")
    if tiled is not None:
        from ..tiling import TiledDetector
        key = tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in tiled.items()))
        cache = pipe.__dict__.setdefault("_tiled_dets", {})          # one wrapper (and its view tables) per option set
        if (id(pipe.det), key) not in cache:
            cache[(id(pipe.det), key)] = TiledDetector(pipe.det, **tiled)
        pipe.det = cache[(id(pipe.det), key)]
    pipe.align = pipe.align or bool(align)
    if tracker is not None:
        pipe.tracker = tracker
    try:
        if augment is not None:
            base_det.augment = bool(augment)
        res = pipe.step(frames, streams=streams)   # detect -> crops -> embed (+ the exact re-run on a detector overflow)
    finally:
        pipe.det, pipe.align, pipe.tracker = was
        if augment is not None:
            base_det.augment = was_augment
    n = res["n_faces"]
    emb = res["emb"].cpu().numpy()
    info = res["info"].cpu().numpy()
    track_ids = res["track_id"].cpu().numpy() if "track_id" in res else None
    keep = None
    if quality_gate is not None:
        from ..quality import face_quality
        lm = res.get("lmarks")
        fmt = 2 if tiled is not None else pipe.det.dets_fmt      # a tiled step's landmarks are fmt-2 rows
        q = face_quality(frames, res["items"], n, lmarks=lm, fmt=None if lm is None else fmt)
        keep = quality_gate.mask(q).cpu().numpy()
    jpegs = None
    if save_face:
        from ..modules.utils.jpeg import encode_crops, encode_jpeg_batch
        if "align_M" in res:
            from ..modules.utils.align import warp_u8
            faces = warp_u8(frames, res["align_M"], res["info"], res["align_flags"], res["items"], n)
            jpegs = encode_jpeg_batch(list(faces), quality=quality)
        else:
            jpegs = encode_crops(frames, res["items"], n, quality=quality)
    out = [FrameFacesObj(frame_nums[i] if frame_nums is not None else i,
                         times_sec[i] if times_sec is not None else 0.0, [], [], np.zeros((0, 4), np.float32))
           for i in range(B)]
    boxes = [[] for _ in range(B)]
    for k in range(n):
        if keep is not None and not keep[k]:
            continue
        f = int(info[k, 0])
        x1, y1, x2, y2, conf, area = info[k, 1:7]
        boxes[f].append([x1, y1, x2, y2])
        out[f].confs.append(float(conf))
        out[f].areas.append(float(area))     # BlazeFace: fraction (inference.py:40-46); YOLO: percent (onnx_utils.py:331)
        out[f].feats.append(emb[k])
        if jpegs is not None:
            out[f].face_jpegs.append(jpegs[k])
        if track_ids is not None:
            out[f].track_ids.append(int(track_ids[k]))
    for f in range(B):
        if boxes[f]:
            out[f].boxes = np.asarray(boxes[f], dtype=np.float32)
    return out


def extract_faces_from_images(pipe, paths, batch_size=256, entropy="host", save_face=False, quality=95,
                              align=False, quality_gate=None, tiled=None, augment=None, reduce=1,
                              orientation=True) -> List[FrameFacesObj]:
    """The reference's image media items (:400-407: one photo per item, any size, recorded as FrameFacesObj(1, 1, ...)) for a
    whole list of files: decode batch_size files at a time (modules/utils/jpeg.py imread_batch; entropy as there), then one
    pipeline step per batch -- frames of different sizes as one RaggedFrames.  Returns one record per path, in order; pass
    each to save_extracted_faces under its file's media_root.  align, quality_gate, tiled, augment: as extract_face_feat_conf_area_list.
    reduce = 2 / 4 / 8: the JPEGs are decoded at 1/2, 1/4, 1/8 size (cv2's IMREAD_REDUCED_COLOR_*: frames of a quarter, a sixteenth,
    a sixty-fourth of the bytes; boxes and crops are then in the reduced frame's pixels); orientation=False: the EXIF Orientation
    tag is not applied (imread_batch)."""
    from ..modules.utils.jpeg import imread_batch
    out = []
    for i in range(0, len(paths), int(batch_size)):
        chunk = paths[i:i + int(batch_size)]
        # (B, H, W, 3) when the sizes agree, else a list
        frames = imread_batch(chunk, pipe.dev, entropy=entropy, reduce=reduce, orientation=orientation)
        recs = extract_face_feat_conf_area_list(pipe, frames, save_face=save_face, quality=quality, align=align,
                                                quality_gate=quality_gate, tiled=tiled, augment=augment)
        for r in recs:
            r.frame_num, r.time_sec = 1, 1
        out.extend(recs)
    return out


def save_extracted_faces(frames_faces_obj_list, media_root, class_name, feats_save_dir, face_feature_size,
                         class2label_dict, save_feat=True, save_face=False, faces_save_dir=None):
    """:311-363: annot dict {media_id, frames_info, class_name, label, feature} with the feature vector zero-padded to
    MAX_N_FRAME_FROM_VID * MAX_N_FACES_PER_FRAME * face_feature_size.  save_face: also write each frame's face_jpegs
    (extract_face_feat_conf_area_list(..., save_face=True)) into faces_save_dir as
    frame_{frame_num}_sec_{time_sec}_conf_{round(conf, 3), '.' -> '_'}_area_{area}.jpg, the reference's names (a later
    face with the same name overwrites an earlier one, as there).  An empty crop, which the reference cannot write, is
    skipped."""
    if save_face:
        if faces_save_dir is None:
            raise ValueError("save_face=True needs faces_save_dir")
        os.makedirs(faces_save_dir, exist_ok=True)
    annot = {"media_id": media_root, "frames_info": []}
    feats_list, total = [], 0
    for fr in frames_faces_obj_list:
        if save_feat:
            feats = list(fr.feats[:MAX_N_FACES_PER_FRAME])
            feats.extend([np.zeros(face_feature_size)] * (MAX_N_FACES_PER_FRAME - len(feats)))
            feats_list.extend(feats)
        annot["frames_info"].append({"frame_num": fr.frame_num, "time_sec": fr.time_sec, "confs": fr.confs,
                                     "areas": fr.areas})
        if save_face:
            if len(fr.face_jpegs) != len(fr.confs):
                raise ValueError(f"frame {fr.frame_num}: no JPEG crops (extract with save_face=True)")
            for data, conf, area in zip(fr.face_jpegs, fr.confs, fr.areas):
                if data is None:
                    continue
                conf = str(round(conf, 3)).replace('.', '_')
                with open(f"{faces_save_dir}/frame_{fr.frame_num}_sec_{fr.time_sec}_conf_{conf}_area_{area}.jpg", "wb") as f:
                    f.write(data)
        total += len(fr.confs)
    os.makedirs(feats_save_dir, exist_ok=True)
    annot["class_name"] = class_name
    annot["label"] = class2label_dict[class_name]
    if save_feat:
        if len(frames_faces_obj_list) < MAX_N_FRAME_FROM_VID:
            pad = MAX_N_FRAME_FROM_VID - len(frames_faces_obj_list)
            feats_list.extend([np.zeros(face_feature_size)] * (MAX_N_FACES_PER_FRAME * pad))
        annot["feature"] = np.concatenate(feats_list, axis=0).astype(np.float32)
    np.save(os.path.join(feats_save_dir, media_root + ".npy"), annot)
    return total
