"""Top-k cosine search (similarity.cosine_topk, fp_cosine_topk_x6) at the two shapes a user runs it at:

  125 000 x 10 000 x 512   the shape the cosine filter is quoted at; here also cosine_filter (top-1, x6) on the SAME operands,
                           the feature's only comparable baseline, and the ratio top-k / top-1
  512 x 1 000 000 x 512    one step's faces against a large gallery; here also the least time the hardware could take: the
                           larger of FLOPs over the bf16 x 6 peak and the split planes' bytes over the HBM bandwidth

each at k = 1, 5 and 16.  Operands are seeded normal rows made on the device; norms and the gallery's bf16 planes are
computed once, outside the timed region (as FaceGallery does).  All variants of a shape are warmed up, then timed
alternately in one process with device events: `--rounds` rounds per variant, each of enough calls to last `--round-s`
seconds (so every variant's timed window is rounds x round-s >= 1 s); the median round is reported with the spread
(min .. max) over rounds.  TFLOP/s are fp32-equivalent: 2 M N D over the time.  --splits: also time forced n_splits values
at k = 5 (how the launcher's automatic choice compares).  Prints one JSON line.
Kernel times: `rocprofv3 --kernel-trace --stats -- python tools/identify_bench.py --rounds 1 --round-s 0.05`.

  python tools/identify_bench.py [--shapes 125000x10000x512 512x1000000x512] [--k 1 5 16] [--rounds 5] [--round-s 0.25]"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from face_detection_and_recognition_amd import similarity as S  # noqa: E402

BF16_PEAK_TFLOPS = 2500.0 / 6      # dense bf16 MFMA peak over the six products of one fp32-equivalent product
HBM_TBS = 6.29                     # measured streaming bandwidth (8.0 spec)


def timed(fn, reps, dev):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(torch.cuda.current_stream(dev))
    for _ in range(reps):
        fn()
    e.record(torch.cuda.current_stream(dev))
    e.synchronize()
    return s.elapsed_time(e) / reps


def run_shape(M, N, D, ks, splits, rounds, round_s, dev, with_filter):
    gen = torch.Generator(device=dev).manual_seed(1000 + M % 997)
    Q = torch.randn((M, D), generator=gen, device=dev)
    G = torch.randn((N, D), generator=gen, device=dev)
    qinv, ginv, g3 = S.row_inv_norm(Q), S.row_inv_norm(G), S.split3_rows(G)
    variants = {}
    if with_filter:
        variants["filter_top1_x6"] = lambda: S.cosine_filter(Q, G, 0.3, ginv=qinv, rinv=ginv, r3=g3, x6=True)
    else:
        del G                                   # the planes are all the search reads
        G = None
    for k in ks:
        variants[f"topk_k{k}"] = lambda k=k: S.cosine_topk(Q, None, k, qinv=qinv, ginv=ginv, g3=g3)
    for ns in splits:
        variants[f"topk_k5_splits{ns}"] = lambda ns=ns: S.cosine_topk(Q, None, 5, qinv=qinv, ginv=ginv, g3=g3, n_splits=ns)
    reps = {}
    for name, fn in variants.items():           # warm-up, and the number of calls that fill a round
        fn()
        torch.cuda.synchronize()
        reps[name] = max(1, math.ceil(round_s * 1e3 / max(timed(fn, 2, dev), 1e-3)))
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn, reps[name], dev))
    flop = 2.0 * M * N * D
    out = dict(M=M, N=N, D=D, gflop=round(flop / 1e9, 1))
    for name, t in times.items():
        ms = float(np.median(t))
        out[name] = dict(ms=round(ms, 4), tflops_fp32_equiv=round(flop / ms / 1e9, 1), min_ms=round(min(t), 4),
                         max_ms=round(max(t), 4), calls_per_round=reps[name], window_s=round(sum(t) * reps[name] / 1e3, 2))
    if with_filter:
        for k in ks:
            out[f"topk_k{k}"]["ratio_to_filter_top1"] = round(out[f"topk_k{k}"]["ms"] / out["filter_top1_x6"]["ms"], 3)
        # the two agree on the best candidate
        best, arg, _ = variants["filter_top1_x6"]()
        sc, ix = variants[f"topk_k{ks[0]}"]()
        out["top1_index_agreement"] = float((ix[:, 0] == arg).float().mean())
        out["top1_max_score_diff"] = float((sc[:, 0] - best).abs().max())
    plane_bytes = g3.numel()
    t_flop, t_mem = flop / (BF16_PEAK_TFLOPS * 1e9), plane_bytes / (HBM_TBS * 1e9)          # ms
    out["floor"] = dict(flops_over_bf16x6_peak_ms=round(t_flop, 4), plane_bytes_over_hbm_ms=round(t_mem, 4),
                        plane_gbytes=round(plane_bytes / 1e9, 3), bound="flops" if t_flop >= t_mem else "hbm")
    for k in ks:
        out[f"topk_k{k}"]["share_of_floor"] = round(max(t_flop, t_mem) / out[f"topk_k{k}"]["ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["125000x10000x512", "512x1000000x512"])
    ap.add_argument("--k", type=int, nargs="+", default=[1, 5, 16])
    ap.add_argument("--splits", type=int, nargs="*", default=[])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--round-s", type=float, default=0.25)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("identify_bench.py measures on the GPU; none is available")
    dev = torch.device("cuda:0")
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes]
    res = []
    for i, (M, N, D) in enumerate(shapes):
        res.append(run_shape(M, N, D, a.k, a.splits, a.rounds, a.round_s, dev, with_filter=M * N <= 125000 * 10000 and i == 0))
        torch.cuda.empty_cache()
    print(json.dumps(dict(bench="identify_topk", shapes=res)))


if __name__ == "__main__":
    main()
