"""The compressed gallery (gallery.CompressedGallery: int8 coarse search + exact rerank, csrc/simi8.hip) beside the exact
search (gallery.FaceGallery, fp_cosine_topk_x6) in ONE process, at the identify shapes of the README:

  512 x 1 000 000 x 512    one step's faces against a large gallery, k = 1 / 5 / 16 with pool = min(64, 4 k)
  125 000 x 10 000 x 512   many faces against a small gallery, k = 5

Per (shape, k): exact = FaceGallery.search; quantize_q = the queries' codes; coarse = the coarse kernel alone on prepared
codes; rerank = the rerank alone on the coarse candidates; two_stage_device / two_stage_host = CompressedGallery.search with
the fp32 rows on the device / in pinned host memory (the host form synchronises and moves M x pool rows: it is left out when
that block exceeds --host-limit-mb).  Rows are synthetic unit vectors: the gallery is seeded normal rows, query i is gallery
row p(i) plus normal noise of --noise times its length, so every query has ONE planted neighbour above a crowd of chance
neighbours -- the hardest case for recall beyond the first place.  recall_coarse@k / recall_two_stage@k: the share of the
exact search's top-k rows found in the coarse list / in the two-stage result; @1 likewise for the first place.
All variants are warmed up, then timed alternately with device events: --rounds rounds per variant, each of enough calls to
last --round-s seconds; the median round and the spread (min .. max) are reported.  --splits: also the coarse pass at forced
n_splits values (how the launcher's automatic choice compares).  Prints one JSON line.

  python tools/coarse_bench.py [--shapes 512x1000000x512 125000x10000x512] [--k 1 5 16] [--rounds 5] [--round-s 0.25]"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from face_detection_and_recognition_amd import similarity as S  # noqa: E402
from face_detection_and_recognition_amd.gallery import CompressedGallery, FaceGallery  # noqa: E402


def timed(fn, reps, dev):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(torch.cuda.current_stream(dev))
    for _ in range(reps):
        fn()
    e.record(torch.cuda.current_stream(dev))
    e.synchronize()
    return s.elapsed_time(e) / reps


def recall(found, truth):
    """Share of truth's rows (M, k) present in found (M, p), over the valid entries of truth."""
    hit = (truth[:, :, None] == found[:, None, :]).any(dim=2) & (truth >= 0)
    return float(hit.sum()) / max(1, int((truth >= 0).sum()))


def run_shape(M, N, D, ks, rounds, round_s, noise, host_limit_mb, dev, splits=()):
    gen = torch.Generator(device=dev).manual_seed(1000 + M % 997)
    G = torch.nn.functional.normalize(torch.randn((N, D), generator=gen, device=dev))
    pick = torch.randint(0, N, (M,), generator=gen, device=dev)
    Q = torch.nn.functional.normalize(G[pick] + noise / math.sqrt(D) * torch.randn((M, D), generator=gen, device=dev))
    labels = torch.zeros((N,), dtype=torch.int32, device=dev)
    exact = FaceGallery(G, labels, device=dev)
    on_dev = CompressedGallery(G, labels, device=dev, rows="device")
    on_host = CompressedGallery(G, labels, device=dev, rows="host")
    out = dict(M=M, N=N, D=D, noise=noise, device_bytes=dict(
        face_gallery=int(sum(t.numel() * t.element_size() for t in (exact.embeddings, exact.g3, exact.ginv, exact.labels))),
        compressed_rows_device=on_dev.device_bytes(), compressed_rows_host_or_none=on_host.device_bytes()), k={})
    del G
    for k in ks:
        pool = min(S.L.COARSE_MAX, 4 * k)
        Qp, qinv, cs, ci = on_dev.coarse(Q, pool)
        qq, sq = S.quantize_rows_i8(Qp)
        u = sq * qinv
        variants = {
            "exact": lambda: exact.search(Q, k),
            "quantize_q": lambda: S.quantize_rows_i8(Qp),
            "coarse": lambda: S.cosine_topk_i8(qq, u, on_dev.g8, on_dev.w, N, pool),
            "rerank": lambda: S.rerank_topk(Qp, ci, k, G=on_dev.rows, ginv=on_dev.ginv, qinv=qinv),
            "two_stage_device": lambda: on_dev.search(Q, k, pool),
        }
        for ns in splits:
            variants[f"coarse_splits{ns}"] = lambda ns=ns: S.cosine_topk_i8(qq, u, on_dev.g8, on_dev.w, N, pool, ns)
        host_mb = M * pool * D * 4 / 2 ** 20
        if host_mb <= host_limit_mb:
            variants["two_stage_host"] = lambda: on_host.search(Q, k, pool)
        reps = {}
        for name, fn in variants.items():           # warm-up, and the number of calls that fill a round
            fn()
            torch.cuda.synchronize()
            reps[name] = max(1, math.ceil(round_s * 1e3 / max(timed(fn, 2, dev), 1e-3)))
        times = {name: [] for name in variants}
        for _ in range(rounds):
            for name, fn in variants.items():
                times[name].append(timed(fn, reps[name], dev))
        r = dict(pool=pool)
        for name, t in times.items():
            r[name] = dict(ms=round(float(np.median(t)), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4),
                           calls_per_round=reps[name])
        if "two_stage_host" not in variants:
            r["two_stage_host"] = f"left out: {host_mb:.0f} MB of gathered rows per search"
        r["two_stage_device_over_exact"] = round(r["two_stage_device"]["ms"] / r["exact"]["ms"], 3)
        r["coarse_over_exact"] = round(r["coarse"]["ms"] / r["exact"]["ms"], 3)
        es, ei = exact.search(Q, k)
        ts, ti = on_dev.search(Q, k, pool)
        r["recall_coarse_at_k"], r["recall_two_stage_at_k"] = round(recall(ci, ei), 4), round(recall(ti, ei), 4)
        r["recall_coarse_at_1"], r["recall_two_stage_at_1"] = round(recall(ci, ei[:, :1]), 4), round(recall(ti[:, :1], ei[:, :1]), 4)
        r["planted_found_at_1"] = float((ti[:, 0] == pick).float().mean())
        same = ti == ei
        r["max_score_diff_where_same_row"] = float((ts - es)[same].abs().max()) if bool(same.any()) else None
        if "two_stage_host" in variants:
            hs, hi = on_host.search(Q, k, pool)
            r["host_equals_device"] = bool(torch.equal(hi, ti) and torch.equal(hs, ts))
        out["k"][str(k)] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["512x1000000x512", "125000x10000x512"])
    ap.add_argument("--k", type=int, nargs="+", default=[1, 5, 16])
    ap.add_argument("--small-k", type=int, nargs="+", default=[5], help="the k values of shapes with more queries than gallery rows")
    ap.add_argument("--splits", type=int, nargs="*", default=[], help="also time the coarse pass at these forced n_splits")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--round-s", type=float, default=0.25)
    ap.add_argument("--noise", type=float, default=0.5)
    ap.add_argument("--host-limit-mb", type=float, default=1024)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("coarse_bench.py measures on the GPU; none is available")
    dev = torch.device("cuda:0")
    res = []
    for s in a.shapes:
        M, N, D = (int(v) for v in s.split("x"))
        res.append(run_shape(M, N, D, a.k if M <= N else a.small_k, a.rounds, a.round_s, a.noise, a.host_limit_mb, dev, a.splits))
        torch.cuda.empty_cache()
    print(json.dumps(dict(bench="coarse_gallery", shapes=res)))


if __name__ == "__main__":
    main()
