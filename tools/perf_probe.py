"""Stage-by-stage timing of the pipeline on one GPU (development aid, not the benchmark)."""
import sys
import time

import torch

import os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from face_detection_and_recognition_amd import workload as W  # noqa: E402
from face_detection_and_recognition_amd.pipeline import FacePipeline  # noqa: E402


def timeit(fn, n=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    dev = torch.device("cuda:0")
    frames = W.make_frames(B, dev)
    det = W.build_detector(dev, frames[:64])
    emb = W.build_embedder(dev)
    ref = W.make_reference(10000, dev)
    pipe = FacePipeline(det, emb, ref, tau=0.3)
    out = pipe.step(frames)
    print("faces", out["n_faces"], "per frame", out["n_faces"] / B, "keep", int(out["keep"].sum()))
    dets, counts, _ = pipe.detect(frames)
    cand, ccount = det.net._last_candidates
    print("candidates/frame", float(ccount.float().mean()), "dets/frame", float(counts.float().mean()))

    net = det.net
    plan = net.plan_for(B)
    from face_detection_and_recognition_amd.modules.utils.image import letterbox_batch
    t_lb = timeit(lambda: letterbox_batch(frames, det.input_size, net._preprocess_lut(), plan.input, 125, True))
    t_fwd = timeit(lambda: plan.run())
    t_post = timeit(lambda: net.postprocess(plan.r, plan.c))
    items, info, nf = pipe.crops(frames, dets, counts)
    n = int(nf.item())
    t_crop = timeit(lambda: pipe.crops(frames, dets, counts))
    t_emb = timeit(lambda: pipe.embed(frames, items, n))
    e = pipe.embed(frames, items, n)
    t_sim = timeit(lambda: pipe.filter(e))
    t_all = timeit(lambda: pipe.step(frames), n=5)
    print(f"B={B} letterbox {t_lb:.3f} ms | blazeface fwd {t_fwd:.3f} ms ({B / t_fwd * 1e3:.0f} fps) | post {t_post:.3f} ms | "
          f"crops {t_crop:.3f} ms | embed[{n}] {t_emb:.3f} ms ({n / t_emb * 1e3:.0f} crops/s) | cosine {t_sim:.3f} ms | "
          f"step {t_all:.3f} ms -> {n / t_all * 1e3:.0f} faces/s")


if __name__ == "__main__":
    main()
