"""evaluate_embedder: score an embedder (and its preprocess) on labelled faces, and read off the cosine threshold the other
tools take (filter / identify / cluster_faces --tau, FaceGallery.identify).

Input: --ld, class sub-folders of .jpg faces (read as the identify script reads its reference directory; class = label), or
--features file.npz holding X (N, D) and labels (N,).  ALL pairs of the labelled rows are scored on the device
(verification.pair_histogram, csrc/pairhist.hip) into a genuine and an impostor histogram; ROC, AUC, EER, the best-accuracy
threshold and TAR at the requested FARs follow on the host (verification.verification_report).  Writes <out>/report.json and
<out>/roc.npz (thresholds, tar, far, genuine, impostor) and prints one JSON line.  With -d cpu and --features the histogram
is the fp64 numpy restatement.  Build-defined: the reference has no counterpart.
"""
import argparse
import json
import os

import numpy as np
import torch

from .. import verification as V

SCALARS = ("n_genuine", "n_impostor", "eer", "eer_threshold", "auc", "best_accuracy", "best_threshold")


def get_parsed_args(argv=None):
    parser = argparse.ArgumentParser()
    src = parser.add_mutually_exclusive_group(required=True)
    src.add_argument('--ld', '--labelled_data_path', dest="labelled_data_path", type=str, default=None,
                     help='a folder of class sub-folders of .jpg faces')
    src.add_argument('--features', type=str, default=None, help='an .npz holding X (N, D) float and labels (N,) integers')
    parser.add_argument('--net', choices=["mobile_facenet", "facenet"], default="mobile_facenet")
    parser.add_argument('-m', '--savedmodel_path', type=str, default=None,
                        help='state_dict (.pth / .pt) of the --net network. (default: weights/mobile_facenet/mobile_facenet.pth, '
                             'weights/facenet/facenet.pt)')
    parser.add_argument('-b', '--batch_size', type=int, default=32)
    parser.add_argument('--preprocess', choices=["mobile_facenet", "tf_standardize"], default=None,
                        help='(default: mobile_facenet with --net mobile_facenet, tf_standardize with facenet)')
    parser.add_argument('-d', '--device', default="cuda")
    parser.add_argument('--bins', type=int, default=1024)
    parser.add_argument('--range', type=float, nargs=2, default=[-1.0, 1.0], metavar=("LO", "HI"))
    parser.add_argument('--far', type=float, nargs="+", default=[1e-1, 1e-2, 1e-3, 1e-4])
    parser.add_argument('--out', type=str, default="data/embedder_eval")
    args = parser.parse_args(argv)
    if args.preprocess is None:
        args.preprocess = "tf_standardize" if args.net == "facenet" else "mobile_facenet"
    if args.savedmodel_path is None:
        args.savedmodel_path = "weights/facenet/facenet.pt" if args.net == "facenet" else "weights/mobile_facenet/mobile_facenet.pth"
    return args


def load_features(path):
    """(X (N, D) float32, labels (N,) int64) of an .npz."""
    with np.load(path) as z:
        if "X" not in z or "labels" not in z:
            raise ValueError(f"{path} must hold X and labels, it holds {sorted(z.files)}")
        X, labels = np.asarray(z["X"], np.float32), np.asarray(z["labels"])
    if X.ndim != 2 or labels.shape != (X.shape[0],) or labels.dtype.kind not in "iu":
        raise ValueError(f"X must be (N, D) and labels N integers, got {X.shape} and {labels.dtype} {labels.shape}")
    return X, labels.astype(np.int64)


def embed_labelled(args):
    """Embed every .jpg of every class folder -> (features on the device, labels int32 tensor, class names)."""
    from .filter_faces_using_reference import embed_images, load_model
    from .identify_faces_using_reference import reference_images
    model = load_model(args)
    feats, labels, names = [], [], []
    for label, (name, paths) in enumerate(reference_images(args.labelled_data_path, None)):
        names.append(name)
        if paths:
            feats.append(embed_images(model, paths, args.batch_size, preprocess=args.preprocess))
            labels += [label] * len(paths)
    if not feats:
        raise Exception(f"no .jpg under the class folders of {args.labelled_data_path}")
    return torch.cat(feats), torch.tensor(labels, dtype=torch.int32), names


def histograms(args):
    """-> (genuine, impostor int64 numpy, edges, number of rows)."""
    lo, hi = args.range
    if args.features is not None:
        X, labels = load_features(args.features)
        if args.device == "cpu":
            h = V.pair_histogram_numpy(X, labels, lo, hi, args.bins)
            return h["genuine"], h["impostor"], h["edges"], len(labels)
        dev = torch.device(args.device.replace("hip", "cuda"))
        X, labels = torch.from_numpy(X).to(dev), torch.from_numpy(labels).to(dev)
    else:
        if args.device == "cpu":
            raise SystemExit("embedding images needs the GPU; -d cpu goes with --features")
        X, labels, _ = embed_labelled(args)
    h = V.pair_histogram(X, labels, lo, hi, args.bins)
    return h["genuine"].cpu().numpy(), h["impostor"].cpu().numpy(), h["edges"], int(labels.shape[0])


def summary_of(report, n_rows, args):
    """The printed line: plain JSON types, NaN as null."""
    def num(v):
        return None if isinstance(v, float) and v != v else v
    line = {k: num(report[k]) for k in SCALARS}
    line["tar_at_far"] = {repr(f): (None if v is None else {k: num(x) for k, x in v.items()})
                          for f, v in report["tar_at_far"].items()}
    line.update(rows=n_rows, bins=args.bins, range=list(args.range))
    return line


def write_report(out_dir, line, report, genuine, impostor):
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "report.json"), "w") as f:
        json.dump(line, f, indent=1)
    np.savez(os.path.join(out_dir, "roc.npz"), thresholds=report["thresholds"], tar=report["tar"], far=report["far"],
             genuine=np.asarray(genuine, np.int64), impostor=np.asarray(impostor, np.int64))


def main(argv=None):
    args = get_parsed_args(argv)
    genuine, impostor, edges, n_rows = histograms(args)
    report = V.verification_report(genuine, impostor, edges, fars=args.far)
    line = summary_of(report, n_rows, args)
    write_report(args.out, line, report, genuine, impostor)
    print(json.dumps(line))
    return line


if __name__ == "__main__":
    main()
