"""identify_faces_using_reference: sort unlabelled face images by who they show (the sibling of filter_faces_using_reference.py).

The filter script checks a folder of faces against the ONE class whose name the folder carries; this one asks the recognition
question.  Every class folder under --rd is enrolled into a FaceGallery (gallery.py; up to -r images per class), every .jpg
under --ud (flat or nested) is embedded with the same network and preprocess, identified against the gallery (top-k cosine
search + vote, csrc/sim.hip; with --coarse int8 the two-stage search of a CompressedGallery, csrc/simi8.hip) and copied to <td>/<class name>/ or <td>/unknown/.  Same networks, weights and argument
conventions as the filter (embed_images, load_model).  Build-defined: the reference has no counterpart.
"""
import argparse
import glob
import os
import shutil

import torch

from ..gallery import FaceGallery
from .filter_faces_using_reference import embed_images, get_class_name_list, load_model

UNKNOWN = "unknown"


def get_parsed_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--ud', '--unlabelled_data_path', dest="unlabelled_data_path", type=str, required=True,
                        help='a flat or nested folder of unlabelled .jpg faces')
    parser.add_argument('--rd', '--reference_data_path', dest="reference_data_path", type=str, required=True,
                        help='reference root: one folder of .jpg faces per class')
    parser.add_argument('--td', '--target_data_path', dest="target_data_path", type=str, default="data/faces_identified")
    parser.add_argument('--net', choices=["mobile_facenet", "facenet"], default="mobile_facenet")
    parser.add_argument('-m', '--savedmodel_path', type=str, default=None,
                        help='state_dict (.pth / .pt) of the --net network. (default: weights/mobile_facenet/mobile_facenet.pth, '
                             'weights/facenet/facenet.pt)')
    parser.add_argument('-b', '--batch_size', type=int, default=32)
    parser.add_argument('-r', '--ref_img_per_class', type=int, default=32)
    parser.add_argument('-k', '--top_k', type=int, default=5, help='candidates per face (1 .. 16)')
    parser.add_argument('--tau', type=float, default=0.3, help='a candidate counts when its cosine score is >= tau')
    parser.add_argument('--vote', choices=["top1", "majority"], default="top1")
    parser.add_argument('--preprocess', choices=["mobile_facenet", "tf_standardize"], default=None,
                        help='(default: mobile_facenet with --net mobile_facenet, tf_standardize with facenet)')
    parser.add_argument('--coarse', choices=["int8"], default=None,
                        help='search a CompressedGallery: an int8 coarse pass over every row, then an exact rerank of --pool '
                             'candidates (default: off, the exact FaceGallery search)')
    parser.add_argument('--pool', type=int, default=None, help='candidates the coarse pass keeps per face (default: min(64, 4k))')
    parser.add_argument('--rows', choices=["device", "host", "none"], default="device",
                        help='with --coarse: where the fp32 rows of the rerank live; none = coarse scores only (approximate)')
    parser.add_argument('-d', '--device', default="cuda")
    args = parser.parse_args(argv)
    if args.coarse is None and (args.pool is not None or args.rows != "device"):
        parser.error("--pool and --rows need --coarse int8")
    if args.preprocess is None:
        args.preprocess = "tf_standardize" if args.net == "facenet" else "mobile_facenet"
    if args.savedmodel_path is None:
        args.savedmodel_path = "weights/facenet/facenet.pt" if args.net == "facenet" else "weights/mobile_facenet/mobile_facenet.pth"
    return args


def reference_images(reference_root, ref_img_per_class):
    """[(class name, sorted first <= ref_img_per_class .jpg paths)] of every class folder, in class-name order."""
    return [(c, sorted(glob.glob(os.path.join(reference_root, c, "*.jpg")))[:ref_img_per_class])
            for c in get_class_name_list(reference_root)]


def unlabelled_images(root):
    """Every .jpg under root, at any depth, sorted."""
    return sorted(glob.glob(os.path.join(root, "**", "*.jpg"), recursive=True))


def enrol_reference(model, reference_root, args):
    """The gallery of the reference root: label = position of the class in get_class_name_list."""
    feats, labels, names = [], [], {}
    for label, (name, paths) in enumerate(reference_images(reference_root, args.ref_img_per_class)):
        names[label] = name
        if paths:
            feats.append(embed_images(model, paths, args.batch_size, preprocess=args.preprocess))
            labels += [label] * len(paths)
    if not feats:
        raise Exception(f"no reference .jpg under {reference_root}")
    gallery = FaceGallery(torch.cat(feats), torch.tensor(labels, dtype=torch.int32), names, device=feats[0].device)
    if getattr(args, "coarse", None) == "int8":
        gallery = gallery.compress(rows=None if args.rows == "none" else args.rows)
    return gallery


def identify_images(model, gallery, paths, args):
    """[class name or "unknown"] for every path."""
    if not paths:
        return []
    feats = embed_images(model, paths, args.batch_size, preprocess=args.preprocess)
    kw = dict(pool=args.pool) if getattr(args, "coarse", None) == "int8" else {}
    res = gallery.identify(feats, k=min(args.top_k, 16), tau=args.tau, vote=args.vote, **kw)
    return [gallery.name_of(l) for l in res["label"].cpu().tolist()]


def target_name(path, root):
    """File name under the class folder: the path below root with the folders folded in (a flat root: the file name)."""
    return os.path.relpath(path, root).replace(os.sep, "_")


def main(argv=None):
    args = get_parsed_args(argv)
    print(args)
    model = load_model(args)
    gallery = enrol_reference(model, args.reference_data_path, args)
    paths = unlabelled_images(args.unlabelled_data_path)
    who = identify_images(model, gallery, paths, args)
    counts = {name: 0 for name in list(gallery.names.values()) + [UNKNOWN]}
    for name in counts:
        os.makedirs(os.path.join(args.target_data_path, name), exist_ok=True)
    for pth, name in zip(paths, who):
        shutil.copy(pth, os.path.join(args.target_data_path, name, target_name(pth, args.unlabelled_data_path)))
        counts[name] += 1
    for name, c in counts.items():
        print(f"{name}: {c} of {len(paths)}")
    return counts


if __name__ == "__main__":
    main()
