"""Cosine DBSCAN (clustering.dbscan_cosine, fp_cosine_dbscan_x6) at N = 10 000 and 100 000 rows of D = 512, on two operands:

  iid      seeded normal rows, tau = 0.5: no edges, the pure triangular walk
  faces    identities with a long-tailed size distribution (the largest holds N / 10 rows: 10 000 at N = 100 000), unit centres
           plus noise, 10 % strangers: prices the degree atomics and the contention of the union-find

and, on the SAME operand in the same process, the yardstick the project already has: similarity.cosine_topk(X, X, k = 1), which
walks the full square with the same instruction mix.  Variants timed:

  walk1    min_samples = 1: ONE walk (degree and union folded) + the five small launches
  walk2    min_samples = 3: the degree walk + the union walk + the small launches; per_pass_ms = walk2 / 2 bounds each pass
           from above (the small launches are inside)
  summary  cluster_summary on the labels of walk1 (faces operand only)

Norms and the bf16 planes are computed once, outside the timed region.  All variants of an operand are warmed up, then timed
alternately with device events: `--rounds` rounds per variant, each of enough calls to last `--round-s` seconds; the median round
is reported with min .. max.  TFLOP/s are fp32-equivalent, counted on N^2 D per walk (the half square's FLOPs).  Prints one
JSON line.  Kernel times per pass: `rocprofv3 --kernel-trace --stats -- python tools/cluster_bench.py --rounds 1 --round-s 0.05`.

  python tools/cluster_bench.py [--n 10000 100000] [--d 512] [--rounds 5] [--round-s 0.25]"""
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


def timed(fn, reps, dev):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(torch.cuda.current_stream(dev))
    for _ in range(reps):
        fn()
    e.record(torch.cuda.current_stream(dev))
    e.synchronize()
    return s.elapsed_time(e) / reps


def iid_rows(N, D, dev):
    gen = torch.Generator(device=dev).manual_seed(2000 + N % 997)
    return torch.randn((N, D), generator=gen, device=dev)


def face_rows(N, D, dev, sigma=0.7):
    """Identity sizes ~ 1 / rank, the largest N / 10 rows; unit centres + sigma / sqrt(D) noise per feature; 10 % strangers;
    rows shuffled."""
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
    return X[torch.randperm(N, generator=gen, device=dev)].contiguous(), len(sizes), max(sizes)


def run_operand(name, X, tau, rounds, round_s, dev, extra):
    N, D = X.shape
    xinv, x3 = S.row_inv_norm(X), S.split3_rows(X)
    variants = {
        "topk_k1_full_square": lambda: S.cosine_topk(X, None, 1, qinv=xinv, ginv=xinv, g3=x3),
        "walk1": lambda: K.dbscan_cosine(X, tau, 1, xinv=xinv, x3=x3),
        "walk2": lambda: K.dbscan_cosine(X, tau, 3, xinv=xinv, x3=x3),
    }
    res1 = variants["walk1"]()
    if name == "faces":
        variants["summary"] = lambda: K.cluster_summary(X, res1["labels"])
    reps = {}
    for vn, fn in variants.items():             # warm-up, and the number of calls that fill a round
        fn()
        torch.cuda.synchronize()
        reps[vn] = max(1, math.ceil(round_s * 1e3 / max(timed(fn, 2, dev), 1e-3)))
    times = {vn: [] for vn in variants}
    for _ in range(rounds):
        for vn, fn in variants.items():
            times[vn].append(timed(fn, reps[vn], dev))
    out = dict(operand=name, N=N, D=D, tau=tau, **extra)
    half = 1.0 * N * N * D                      # FLOPs of the half square: 2 * (N^2 / 2) * D
    walks = {"topk_k1_full_square": 2, "walk1": 1, "walk2": 2}
    for vn, t in times.items():
        ms = float(np.median(t))
        out[vn] = dict(ms=round(ms, 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4), calls_per_round=reps[vn])
        if vn in walks:
            out[vn]["tflops_fp32_equiv"] = round(walks[vn] * half / ms / 1e9, 1)
    out["walk2"]["per_pass_ms"] = round(out["walk2"]["ms"] / 2, 4)
    yard = out["topk_k1_full_square"]["ms"]
    out["walk1_over_yardstick"] = round(out["walk1"]["ms"] / yard, 3)
    out["per_pass_over_yardstick"] = round(out["walk2"]["per_pass_ms"] / yard, 3)
    res3 = variants["walk2"]()
    torch.cuda.synchronize()
    deg = res1["degree"].to(torch.int64)
    out["edges"] = int((deg.sum() - (deg > 0).sum()).item() // 2)
    out["clusters_min_samples_1"] = int(res1["n_clusters"].item())
    out["clusters_min_samples_3"] = int(res3["n_clusters"].item())
    out["noise_min_samples_3"] = int((res3["labels"] < 0).sum().item())
    out["largest_cluster_min_samples_3"] = int(torch.bincount(res3["labels"][res3["labels"] >= 0].to(torch.int64)).max().item()) \
        if out["clusters_min_samples_3"] else 0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[10000, 100000])
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--operands", nargs="+", choices=["iid", "faces"], default=["iid", "faces"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--round-s", type=float, default=0.25)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cluster_bench.py measures on the GPU; none is available")
    dev = torch.device("cuda:0")
    res = []
    for N in a.n:
        for op in a.operands:
            if op == "iid":
                X, extra = iid_rows(N, a.d, dev), {}
            else:
                X, n_ids, biggest = face_rows(N, a.d, dev)
                extra = dict(identities=n_ids, largest_identity=biggest)
            res.append(run_operand(op, X, 0.5, a.rounds, a.round_s, dev, extra))
            del X
            torch.cuda.empty_cache()
    print(json.dumps(dict(bench="cluster_dbscan", configs=res)))


if __name__ == "__main__":
    main()
