"""track_faces_in_frames: the faces of one video, given as a folder of its frames or as a Motion-JPEG file, grouped into tracks.

Every .jpg of --frames (sorted by name = video order), or every frame of --video (a Motion-JPEG AVI or raw .mjpeg stream,
modules/utils/video.py; exactly one of the two is given; tracks.json then names frames frame_000000.jpg ...), goes through FacePipeline (BlazeFace-back + Mobile-FaceNet) batch by
batch with a tracking.StreamTracker behind the embedder: one fp_tracklets_step launch per batch assigns every face a track id
(DESIGN section 7 "Tracklets").  A TrackBook collects, per track, its first and last frame, its hits and its best row (the
highest detector confidence, or with --quality the sharpest crop); at the end <td>/tracks.json lists the tracks and
<td>/track_XXXX/best.jpg is each track's best face crop, encoded on the device (modules/utils/jpeg.py encode_crops).

`--model synthetic` (the default: no trained weights ship with the project) runs the seeded random weights of workload.py.
The thresholds default to the reference's numbers restated as cosines, unmeasured on real video; --max_age has no default.
--motion STD_POS STD_VEL turns the tracker's constant-velocity prediction on (tracking.ConstantVelocity: the IoU gate takes the
box a track is predicted at; no defaults, nothing has been measured).
--reid TAU LOST_AGE turns re-identification on (tracking.LostPool: a track that ends is remembered for LOST_AGE frames and a
returning face whose cosine to its last embedding exceeds TAU continues it -- one track_XXXX/ folder and one id instead of
two; no defaults, nothing has been measured on real video).
--templates [--weighted] keeps a template per track on the device (tracking.Templates: the sum of the track's normalised
embeddings, with --weighted each weighed by its score): tracks.json gains template_rows and <td>/tracks.npz holds the templates
(ids, templates, template_rows).  --gallery FILE [--identify_tau T] (a FaceGallery.save file; needs --templates) names every
track from its template (FacePipeline(identify_tracks=True)): tracks.json gains identity (the gallery's name, null for nobody)
and identity_score, and the captions of --video_out carry the track's name.  What either gains on real video is unmeasured.
Build-defined: the reference labels faces frame by frame (face_tracker.py is that port).

--video_out FILE writes every frame with its tracked faces' boxes and ` #<id>` captions (FacePipeline.annotate) to a
Motion-JPEG AVI at the source's frame rate (25 where a folder or raw stream states none; below 2 GiB: OpenDML is out of scope).

--mot_out FILE also writes every tracked face as a MOTChallenge row `frame,id,x,y,w,h,conf,-1,-1,-1` (frames 1-based in video
order): a hypothesis file for eval/eval_face_tracker.py --tracks.  Nothing changes without it.
"""
import argparse
import glob
import json
import os

import numpy as np

from ..tracking import BEST, IOU_MIN, TAU_FAR, TAU_NEAR, ConstantVelocity, LostPool, StreamTracker, Templates, TrackBook


def get_parsed_args(argv=None):
    parser = argparse.ArgumentParser()
    source = parser.add_mutually_exclusive_group(required=True)
    source.add_argument('--frames', dest="frames_path", type=str, default=None, help="a folder of one video's frames as .jpg")
    source.add_argument('--video', dest="video_path", type=str, default=None,
                        help="a Motion-JPEG video file (AVI 1.0 or a raw .mjpeg stream) in place of --frames")
    parser.add_argument('--video_out', type=str, default=None,
                        help="write the frames with the tracked faces' boxes and ' #<id>' captions to this Motion-JPEG AVI "
                             "(AVI 1.0: below 2 GiB, OpenDML is out of scope)")
    parser.add_argument('--td', '--target_data_path', dest="target_data_path", type=str, default="data/tracks")
    parser.add_argument('--model', default="synthetic", help="'synthetic' (seeded random weights); trained weights: use the API")
    parser.add_argument('--max_age', type=int, required=True,
                        help='a track unseen for more than this many frames ends (no default: nothing has been measured)')
    parser.add_argument('--tau_near', type=float, default=TAU_NEAR)
    parser.add_argument('--tau_far', type=float, default=TAU_FAR)
    parser.add_argument('--iou_min', type=float, default=IOU_MIN)
    parser.add_argument('--motion', type=float, nargs=2, default=None, metavar=("STD_POS", "STD_VEL"),
                        help="constant-velocity prediction for the IoU gate: noise as fractions of the box height (no defaults)")
    parser.add_argument('--reid', type=float, nargs=2, default=None, metavar=("TAU", "LOST_AGE"),
                        help="re-identification of ended tracks: the cosine a returning face must exceed and the frames a track "
                             "is remembered, an integer > max_age (no defaults)")
    parser.add_argument('--templates', action="store_true",
                        help="keep a template per track (the sum of its normalised embeddings) and write them to tracks.npz")
    parser.add_argument('--weighted', action="store_true", help="with --templates: weigh every row by its score")
    parser.add_argument('--gallery', type=str, default=None,
                        help="a FaceGallery.save file: name every track from its template (needs --templates)")
    parser.add_argument('--identify_tau', type=float, default=None, help="with --gallery: the cosine a name needs (default 0.3)")
    parser.add_argument('--quality', action="store_true", help="best shot by crop sharpness instead of detector confidence")
    parser.add_argument('-b', '--batch_size', type=int, default=256)
    parser.add_argument('--jpeg_quality', type=int, default=95)
    parser.add_argument('-d', '--device', default="cuda:0")
    parser.add_argument('--mot_out', type=str, default=None, help="also write the tracked rows as MOTChallenge text to this file")
    return parser.parse_args(argv)


def lost_pool(args):
    """--reid as a tracking.LostPool, or None (ValueError for a LOST_AGE that is no integer)."""
    return None if args.reid is None else LostPool(args.reid[0], args.reid[1])


def frame_files(folder):
    return sorted(glob.glob(os.path.join(folder, "*.jpg")))


def build_pipeline(args, dev, first_frames):
    """(pipeline, tracker) on the synthetic weights, the detector's scores calibrated on the first frames."""
    from .. import workload as W
    from ..pipeline import FacePipeline
    if args.model != "synthetic":
        raise ValueError("only --model synthetic is wired here; build a FacePipeline(..., tracker=StreamTracker(...)) for real weights")
    det = W.build_detector(dev, first_frames, cand_per_frame=48)
    emb = W.build_embedder(dev)
    motion = None if args.motion is None else ConstantVelocity(*args.motion)
    if (args.weighted or args.gallery) and not args.templates:
        raise ValueError("--weighted and --gallery need --templates")
    tracker = StreamTracker(1, emb.embedding_size, args.max_age, args.tau_near, args.tau_far, args.iou_min, device=dev, motion=motion,
                            reid=lost_pool(args), templates=Templates(args.weighted) if args.templates else None)
    kw = {}
    if args.gallery:
        from ..gallery import FaceGallery
        kw = dict(gallery=FaceGallery.load(args.gallery, device=dev), identify_tau=args.identify_tau, identify_tracks=True)
    return FacePipeline(det, emb, None, quality=True if args.quality else None, tracker=tracker, **kw), tracker


def track_frames(pipe, paths, batch_size, jpeg_quality=95, mot_rows=None, writer=None):
    """-> (TrackBook, {(stream, id): JPEG bytes of the best row's crop}).  Frames of one size (a video's).  paths: the sorted
    .jpg files, or a VideoReader.  mot_rows: a list that receives, per batch, (frame numbers, ids, xywh boxes, confidences) of
    the rows with a track id (numpy).  writer: a VideoWriter that receives every batch annotated (FacePipeline.annotate).
    With a tracker that keeps templates the book's records carry template / template_rows, and with identify_tracks also
    identity / identity_score: the track's latest."""
    import torch
    from ..modules.utils.jpeg import encode_crops
    from ..modules.utils.video import read_frames
    book, shots = TrackBook(), {}
    for lo in range(0, len(paths), int(batch_size)):
        frames = read_frames(paths, lo, lo + int(batch_size), pipe.dev)
        res = pipe.step(frames)
        if writer is not None:
            writer.write(pipe.annotate(frames, res))
        n, info = res["n_faces"], res["info"]
        score = res["quality"]["sharpness"] if "quality" in res else info[:, 5]
        sof = np.zeros((frames.shape[0],), np.int32)
        out = {k: res[k] for k in pipe.TRACK_KEYS}
        book.update(out, info[:n, 0].to(torch.int32), info[:n, 1:5], sof, emb=res["emb"], score=score[:n], frame_base=lo,
                    track_emb=res.get("track_emb"), track_emb_rows=res.get("track_emb_rows"))
        flags, ids = res["track_flags"].cpu().numpy(), res["track_id"].cpu().numpy()
        if "track_identity" in res:
            who, how = res["track_identity"].cpu().numpy(), res["track_identity_score"].cpu().numpy()
            for i in range(n):
                if ids[i] > 0:
                    book[(0, int(ids[i]))].update(identity=int(who[i]), identity_score=float(how[i]))
        if mot_rows is not None:
            rows = info[:n].cpu().numpy().astype(np.float64)
            keep = ids[:n] > 0
            xywh = np.concatenate([rows[:, 1:3], rows[:, 3:5] - rows[:, 1:3]], 1)
            mot_rows.append((lo + rows[keep, 0].astype(np.int64), ids[:n][keep].astype(np.int64), xywh[keep], rows[keep, 5]))
        best_rows = [i for i in range(n) if flags[i] & BEST and ids[i] > 0]
        if best_rows:                              # the crops of this batch's BEST rows, one device call; a later BEST replaces
            idx = torch.as_tensor(best_rows, device=pipe.dev)
            files = encode_crops(frames, res["items"][idx].contiguous(), len(best_rows), quality=jpeg_quality)
            for i, data in zip(best_rows, files):
                shots[(0, int(ids[i]))] = data
    return book, shots


def save_tracks(target, book, shots, paths, names=None):
    """<target>/tracks.json and <target>/track_XXXX/best.jpg; with templates in the book also <target>/tracks.npz (ids,
    templates, template_rows, in the order of tracks.json).  names: the gallery's {label: name}.  -> the list written to
    tracks.json."""
    os.makedirs(target, exist_ok=True)
    tracks, templates = [], []
    for r in book.rows():
        name = f"track_{r['id']:04d}"
        rec = dict(id=r["id"], first_frame=os.path.basename(paths[r["first_clock"] - 1]),
                   last_frame=os.path.basename(paths[r["last_clock"] - 1]), hits=r["hits"], best_score=r["best_score"],
                   best_file=os.path.basename(paths[r["best_frame"]]), best_box=r["best_box"], best_jpg=None)
        data = shots.get((r["stream"], r["id"]))
        if data is not None:
            os.makedirs(os.path.join(target, name), exist_ok=True)
            with open(os.path.join(target, name, "best.jpg"), "wb") as f:
                f.write(data)
            rec["best_jpg"] = f"{name}/best.jpg"
        if "template" in r:
            rec["template_rows"] = r["template_rows"]
            templates.append(r["template"])
        if "identity" in r:
            k = r["identity"]
            rec["identity"] = None if k < 0 else str((names or {}).get(k, k))
            rec["identity_score"] = r["identity_score"]
        tracks.append(rec)
    if templates:
        np.savez(os.path.join(target, "tracks.npz"), ids=np.array([t["id"] for t in tracks], np.int32),
                 templates=np.stack(templates).astype(np.float32),
                 template_rows=np.array([t["template_rows"] for t in tracks], np.int32))
    with open(os.path.join(target, "tracks.json"), "w") as f:
        json.dump(dict(frames=len(paths), tracks=tracks), f, indent=1)
    return tracks


def write_mot_rows(path, mot_rows):
    """The batches collected by track_frames(mot_rows=) as one MOTChallenge text file."""
    from ..tracking_eval import write_mot_txt
    cols = [np.concatenate([r[k] for r in mot_rows]) if mot_rows else np.zeros((0, 4) if k == 2 else 0) for k in range(4)]
    write_mot_txt(path, cols[0].astype(np.int64), cols[1].astype(np.int64), cols[2], cols[3])


def main(argv=None):
    import torch
    from ..modules.utils.video import VideoReader, VideoWriter, read_frames
    args = get_parsed_args(argv)
    print(args)
    fps = None
    if args.video_path is not None:
        source = VideoReader(args.video_path)
        if not len(source):
            raise Exception(f"no frames in {args.video_path}")
        paths, fps = [f"frame_{i:06d}.jpg" for i in range(len(source))], source.fps
    else:
        source = paths = frame_files(args.frames_path)
        if not paths:
            raise Exception(f"no .jpg under {args.frames_path}")
    dev = torch.device(args.device)
    pipe, _ = build_pipeline(args, dev, read_frames(source, 0, 8, dev))
    mot_rows = [] if args.mot_out else None
    writer = VideoWriter(args.video_out, fps if fps is not None else 25) if args.video_out else None
    try:
        book, shots = track_frames(pipe, source, args.batch_size, args.jpeg_quality, mot_rows=mot_rows, writer=writer)
    finally:
        if writer is not None:
            writer.close()
        if isinstance(source, VideoReader):
            source.close()
    tracks = save_tracks(args.target_data_path, book, shots, paths, names=pipe.gallery.names if pipe.gallery is not None else None)
    if args.mot_out:
        write_mot_rows(args.mot_out, mot_rows)
    print(f"{len(tracks)} tracks in {len(paths)} frames -> {os.path.join(args.target_data_path, 'tracks.json')}")
    return tracks


if __name__ == "__main__":
    main()
