"""cluster_faces: sort unlabelled face images by identity without any reference (the third sibling of
filter_faces_using_reference.py and identify_faces_using_reference.py).

Every .jpg under --ud (flat or nested) is embedded with the --net network, the embeddings are grouped by cosine DBSCAN on the
device (clustering.dbscan_cosine, csrc/cluster.hip) and every image is copied to <td>/cluster_0000/ ... or <td>/noise/.
<td>/clusters.npz keeps paths, labels, core, degree, centroids and medoid.  Same networks, weights and argument conventions as
the identify script (embed_images, load_model).  Build-defined: the reference has no counterpart.
"""
import argparse
import os
import shutil

import numpy as np

from ..clustering import cluster_summary, dbscan_cosine
from .filter_faces_using_reference import embed_images, load_model
from .identify_faces_using_reference import target_name, unlabelled_images

NOISE = "noise"


def get_parsed_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--ud', '--unlabelled_data_path', dest="unlabelled_data_path", type=str, required=True,
                        help='a flat or nested folder of unlabelled .jpg faces')
    parser.add_argument('--td', '--target_data_path', dest="target_data_path", type=str, default="data/faces_clustered")
    parser.add_argument('--net', choices=["mobile_facenet", "facenet"], default="mobile_facenet")
    parser.add_argument('-m', '--savedmodel_path', type=str, default=None,
                        help='state_dict (.pth / .pt) of the --net network. (default: weights/mobile_facenet/mobile_facenet.pth, '
                             'weights/facenet/facenet.pt)')
    parser.add_argument('-b', '--batch_size', type=int, default=32)
    parser.add_argument('--tau', type=float, default=0.5, help='two faces are neighbours when their cosine score is >= tau')
    parser.add_argument('--min_samples', type=int, default=2,
                        help='a face with this many neighbours, itself included, is a core face (1 .. 64)')
    parser.add_argument('--preprocess', choices=["mobile_facenet", "tf_standardize"], default=None,
                        help='(default: mobile_facenet with --net mobile_facenet, tf_standardize with facenet)')
    parser.add_argument('--best-shot', dest="best_shot", action="store_true",
                        help='measure every image (quality.face_quality over the whole image), keep the columns in clusters.npz '
                             'and copy each cluster\'s sharpest usable image to cluster_XXXX/best.jpg')
    parser.add_argument('-d', '--device', default="cuda")
    parser.add_argument('--reduce', type=int, choices=[1, 2, 4, 8], default=1,
                        help='decode the JPEGs at 1/2, 1/4 or 1/8 size out of smaller inverse DCTs (cv2\'s IMREAD_REDUCED_COLOR_*)')
    parser.add_argument('--ignore_orientation', action="store_true",
                        help='do not turn the images upright by their EXIF Orientation tag (the default applies it, as cv2.imread)')
    args = parser.parse_args(argv)
    if args.preprocess is None:
        args.preprocess = "tf_standardize" if args.net == "facenet" else "mobile_facenet"
    if args.savedmodel_path is None:
        args.savedmodel_path = "weights/facenet/facenet.pt" if args.net == "facenet" else "weights/mobile_facenet/mobile_facenet.pth"
    return args


def cluster_name(label):
    label = int(label)
    return NOISE if label < 0 else f"cluster_{label:04d}"


def group_files(paths, labels, medoid, root, target):
    """Copy every path to <target>/cluster_XXXX/ or <target>/noise/ under target_name(path, root).  medoid: one row index per
    cluster.  Returns [(folder, size, target_name of the medoid's file)] per cluster, then the noise folder (medoid None)."""
    labels = [int(l) for l in labels]
    medoid = [int(m) for m in medoid]
    if len(labels) != len(paths):
        raise ValueError(f"{len(labels)} labels for {len(paths)} paths")
    n_clusters = max(labels, default=-1) + 1
    if len(medoid) != n_clusters:
        raise ValueError(f"{len(medoid)} medoids for {n_clusters} clusters")
    folders = [cluster_name(c) for c in range(n_clusters)] + [NOISE]
    for f in folders:
        os.makedirs(os.path.join(target, f), exist_ok=True)
    sizes = [0] * (n_clusters + 1)
    for pth, lab in zip(paths, labels):
        shutil.copy(pth, os.path.join(target, cluster_name(lab), target_name(pth, root)))
        sizes[lab if lab >= 0 else n_clusters] += 1
    rep = [target_name(paths[m], root) if 0 <= m < len(paths) else None for m in medoid] + [None]
    return list(zip(folders, sizes, rep))


def save_clusters(path, paths, labels, core, degree, centroids, medoid, quality=None):
    """<td>/clusters.npz: plain arrays, readable without pickle.  quality: further arrays (--best-shot: quality_<column> per
    image and best_shot per cluster)."""
    np.savez(path, paths=np.array([str(p) for p in paths], dtype=np.str_), labels=np.asarray(labels, np.int32),
             core=np.asarray(core, bool), degree=np.asarray(degree, np.int32), centroids=np.asarray(centroids, np.float32),
             medoid=np.asarray(medoid, np.int32), **(quality or {}))
    return path


QUALITY_COLUMNS = ("flags", "step", "mean", "contrast", "dark_frac", "bright_frac", "sharpness", "side")


def image_quality(paths, device, batch_size=32, entropy="host", reduce=1, orientation=True):
    """quality.face_quality of every image as ONE whole-image rectangle (these images are face crops already) -> dict of
    host arrays, one row per path: stats (n, 8) and QUALITY_COLUMNS.  Decoded batch by batch as embed_images decodes them."""
    import torch
    from ..frames import as_frames, frame_layout
    from ..modules.utils.jpeg import imread_batch
    from ..quality import face_quality
    cols = {k: [] for k in ("stats",) + QUALITY_COLUMNS}
    for i in range(0, len(paths), int(batch_size)):
        decoded = imread_batch(paths[i:i + int(batch_size)], device, entropy=entropy, reduce=reduce, orientation=orientation)
        frames = as_frames(list(decoded) if isinstance(decoded, (list, tuple)) else decoded, device)
        rows = [[k, 0, 0, w, h, 0, 0, 0, 0] for k, (_, h, w) in enumerate(frame_layout(frames))]
        items = torch.tensor(rows, dtype=torch.int32, device=device)
        q = face_quality(frames, items, len(rows))
        for k in cols:
            cols[k].append(q[k].cpu().numpy())
    return {k: np.concatenate(v) for k, v in cols.items()}


def best_shots(q, labels, n_clusters):
    """(n_clusters,) int32 rows: per cluster its image with the highest sharpness among the usable ones (an open QualityGate's
    mask, and a Laplacian to speak of); -1 when a cluster has none."""
    from ..quality import NO_LAPLACIAN, QualityGate, best_per_group
    usable = QualityGate().mask(q).numpy() & ((q["flags"] & NO_LAPLACIAN) == 0)
    return best_per_group(q["sharpness"], np.asarray(labels, np.int64), n_clusters, usable).numpy()


def copy_best_shots(paths, best, target):
    """Copy image best[c] to <target>/cluster_XXXX/best.jpg for every cluster c that has one.  Returns the files written."""
    out = []
    for c, row in enumerate(best):
        if row >= 0:
            out.append(shutil.copy(paths[int(row)], os.path.join(target, cluster_name(c), "best.jpg")))
    return out


def main(argv=None):
    args = get_parsed_args(argv)
    print(args)
    model = load_model(args)
    paths = unlabelled_images(args.unlabelled_data_path)
    if not paths:
        raise Exception(f"no .jpg under {args.unlabelled_data_path}")
    read = dict(reduce=args.reduce, orientation=not args.ignore_orientation)
    feats = embed_images(model, paths, args.batch_size, preprocess=args.preprocess, **read)
    res = dbscan_cosine(feats, args.tau, args.min_samples)
    summ = cluster_summary(feats, res["labels"])
    labels, medoid = res["labels"].cpu().numpy(), summ["medoid"].cpu().numpy()
    groups = group_files(paths, labels, medoid, args.unlabelled_data_path, args.target_data_path)
    quality = None
    if args.best_shot:
        q = image_quality(paths, model._device(), args.batch_size, **read)
        best = best_shots(q, labels, len(medoid))
        copy_best_shots(paths, best, args.target_data_path)
        quality = {f"quality_{k}": v for k, v in q.items()}
        quality["best_shot"] = best.astype(np.int32)
    save_clusters(os.path.join(args.target_data_path, "clusters.npz"), paths, labels, res["core"].cpu().numpy(),
                  res["degree"].cpu().numpy(), summ["centroids"].cpu().numpy(), medoid, quality)
    for k, (folder, size, rep) in enumerate(groups):
        shot = ""
        if quality is not None and k < len(medoid) and quality["best_shot"][k] >= 0:
            shot = f", best shot {target_name(paths[int(quality['best_shot'][k])], args.unlabelled_data_path)}"
        print(f"{folder}: {size} of {len(paths)}" + (f", medoid {rep}" if rep is not None else "") + shot)
    return groups


if __name__ == "__main__":
    main()
