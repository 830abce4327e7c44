"""The pair histogram (verification.pair_histogram, fp_pair_histogram_x6) at N = 10 000 and 100 000 rows of D = 512 and 128, on
the operands of tools/cluster_bench.py and one more:

  iid      seeded normal rows, labels i mod 1000: impostor scores in a narrow band around 0
  faces    identities with a long-tailed size distribution (the largest holds N / 10 rows), unit centres plus noise, 10 %
           strangers (each an identity of its own): genuine scores high, impostor scores around 0
  one      the iid rows under ONE label: every pair is genuine

and, on the SAME operand in the same process, the yardstick: the single edge-free walk of the DBSCAN kernel,
clustering.dbscan_cosine(X, tau = 2.0, min_samples = 2) -- the same work list, staging and MFMAs, an epilogue that leaves a
32 x 128 block after one ballot.  Variants timed:

  walk       dbscan_cosine(tau = 2.0, min_samples = 2): one walk + the small launches
  hist1024   pair_histogram over [-1, 1] with 1024 bins: 56 KiB of LDS, two workgroups per CU
  hist512    the same with 512 bins: 52 KiB, three workgroups per CU as in the walk

Norms and the bf16 planes are computed once, outside the timed region.  All variants of an operand are warmed up, then timed
alternately with device events: `--rounds` rounds per variant, each of enough calls to last `--round-s` seconds; the median round
is reported with min .. max.  TFLOP/s are fp32-equivalent, counted on N^2 D (the half square's FLOPs).  Prints one JSON line.

  python tools/verify_bench.py [--n 10000 100000] [--d 512 128] [--operands iid faces one] [--rounds 5] [--round-s 0.25]"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from face_detection_and_recognition_amd import clustering as K  # noqa: E402
from face_detection_and_recognition_amd import similarity as S  # noqa: E402
from face_detection_and_recognition_amd import verification as V  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cluster_bench import iid_rows, timed  # noqa: E402


def face_rows(N, D, dev, sigma=0.7):
    """cluster_bench.face_rows draw for draw (the rows are the same), with the labels: the identity of every row, and for a
    stranger an identity of its own."""
    gen = torch.Generator(device=dev).manual_seed(3000 + N % 997)
    sizes, left, rank = [], N, 1
    while left > 0:
        s = min(left, max(1, N // (10 * rank)))
        sizes.append(s)
        left -= s
        rank += 1
    ids = torch.repeat_interleave(torch.arange(len(sizes), device=dev), torch.tensor(sizes, device=dev))
    C = torch.randn((len(sizes), D), generator=gen, device=dev)
    C /= C.norm(dim=1, keepdim=True)
    X = C[ids] + torch.randn((N, D), generator=gen, device=dev) * (sigma / math.sqrt(D))
    stranger = torch.rand((N,), generator=gen, device=dev) < 0.1
    X[stranger] = torch.randn((int(stranger.sum()), D), generator=gen, device=dev)
    labels = torch.where(stranger, len(sizes) + torch.arange(N, device=dev), ids)
    perm = torch.randperm(N, generator=gen, device=dev)
    return X[perm].contiguous(), labels[perm].to(torch.int32).contiguous(), len(sizes), max(sizes)


def run_operand(name, X, labels, rounds, round_s, dev, extra):
    N, D = X.shape
    xinv, x3 = S.row_inv_norm(X), S.split3_rows(X)
    variants = {
        "walk": lambda: K.dbscan_cosine(X, 2.0, 2, xinv=xinv, x3=x3),
        "hist1024": lambda: V.pair_histogram(X, labels, -1.0, 1.0, 1024, xinv=xinv, x3=x3),
        "hist512": lambda: V.pair_histogram(X, labels, -1.0, 1.0, 512, xinv=xinv, x3=x3),
    }
    reps = {}
    for vn, fn in variants.items():             # warm-up, and the number of calls that fill a round
        fn()
        torch.cuda.synchronize()
        reps[vn] = max(1, math.ceil(round_s * 1e3 / max(timed(fn, 2, dev), 1e-3)))
    times = {vn: [] for vn in variants}
    for _ in range(rounds):
        for vn, fn in variants.items():
            times[vn].append(timed(fn, reps[vn], dev))
    out = dict(operand=name, N=N, D=D, **extra)
    half = 1.0 * N * N * D                      # FLOPs of the half square: 2 * (N^2 / 2) * D
    for vn, t in times.items():
        ms = float(np.median(t))
        out[vn] = dict(ms=round(ms, 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4), calls_per_round=reps[vn],
                       tflops_fp32_equiv=round(half / ms / 1e9, 1))
    for vn in ("hist1024", "hist512"):
        out[vn + "_over_walk"] = round(out[vn]["ms"] / out["walk"]["ms"], 3)
    res, res512 = variants["hist1024"](), variants["hist512"]()
    torch.cuda.synchronize()
    out["n_genuine"], out["n_impostor"] = int(res["genuine"].sum().item()), int(res["impostor"].sum().item())
    out["bins_hit_impostor"] = int((res["impostor"] > 0).sum().item())
    out["bins_hit_genuine"] = int((res["genuine"] > 0).sum().item())
    # 512 bins are pairs of the 1024: the same scores, the same class, counted at another occupancy
    out["hist512_is_hist1024_folded"] = bool(torch.equal(res["genuine"].view(512, 2).sum(1), res512["genuine"])
                                             and torch.equal(res["impostor"].view(512, 2).sum(1), res512["impostor"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[10000, 100000])
    ap.add_argument("--d", type=int, nargs="+", default=[512, 128])
    ap.add_argument("--operands", nargs="+", choices=["iid", "faces", "one"], default=["iid", "faces", "one"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--round-s", type=float, default=0.25)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("verify_bench.py measures on the GPU; none is available")
    dev = torch.device("cuda:0")
    res = []
    for D in a.d:
        for N in a.n:
            for op in a.operands:
                if op == "faces":
                    X, labels, n_ids, biggest = face_rows(N, D, dev)
                    extra = dict(identities=n_ids, largest_identity=biggest)
                else:
                    X, extra = iid_rows(N, D, dev), {}
                    labels = (torch.arange(N, device=dev) % 1000).to(torch.int32) if op == "iid" else \
                        torch.zeros((N,), dtype=torch.int32, device=dev)
                res.append(run_operand(op, X, labels, a.rounds, a.round_s, dev, extra))
                del X
                torch.cuda.empty_cache()
    print(json.dumps(dict(bench="pair_histogram", configs=res)))


if __name__ == "__main__":
    main()
