"""FaceNet (Inception-ResNet-v1, modules/facenet) forward throughput: the split-MFMA plan (PlanBuilder.X6, every conv on
csrc/pwx6.hip) against the fp32-MFMA plan (X6 off, conv_igemm_kernel), at one batch (default 1024 crops of 160 x 160).

Both plans are built up front on the same seeded weights and inputs, warmed up, then timed alternately in one process with
device events (`--rounds` rounds of `--reps` forwards each, the median round reported).  FLOPs are the reference's count
(2 x the multiply-accumulates of the convs and the Linear, from the op shapes: CompiledPlan.flops).  Prints one JSON line.
Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/facenet_bench.py` (a run of its own).

  python tools/facenet_bench.py [--crops 1024] [--dim 512] [--reps 10] [--rounds 5]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from face_detection_and_recognition_amd.modules.facenet.inception_resnet_v1 import InceptionResnetV1  # noqa: E402
from face_detection_and_recognition_amd.plan import PlanBuilder  # noqa: E402
from face_detection_and_recognition_amd.synth import synth_state_dict  # noqa: E402


def build(net, n, x6):
    saved = PlanBuilder.X6
    PlanBuilder.X6 = x6
    try:
        return net._build(n)
    finally:
        PlanBuilder.X6 = saved


def timed(plan, reps, dev):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(torch.cuda.current_stream(dev))
    for _ in range(reps):
        plan.run()
    e.record(torch.cuda.current_stream(dev))
    e.synchronize()
    return s.elapsed_time(e) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crops", type=int, default=1024)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    net = InceptionResnetV1(a.dim, normalize=a.dim == 512)
    net.load_state_dict(synth_state_dict(net.state_dict(), 7))
    net = net.to(dev)
    x = torch.from_numpy(np.random.default_rng(3).normal(0, 1, (a.crops, 160, 160, 3)).astype(np.float32)).to(dev)
    plans = {"x6": build(net, a.crops, True), "fp32_mfma": build(net, a.crops, False)}
    for p in plans.values():
        p.input[..., :3].copy_(x)
        p.input[..., 3:].zero_()
        for _ in range(3):
            p.run()
    torch.cuda.synchronize()
    flops = sum(plans["x6"].flops(i) for i in range(plans["x6"].n_ops))
    times = {k: [] for k in plans}
    for _ in range(a.rounds):
        for k, p in plans.items():
            times[k].append(timed(p, a.reps, dev))
    out = dict(net="inception_resnet_v1", crops=a.crops, dim=a.dim, gflop_per_crop=round(flops / a.crops / 1e9, 4))
    for k, t in times.items():
        ms = float(np.median(t))
        out[k] = dict(ms_per_forward=round(ms, 3), crops_per_s=round(a.crops / ms * 1e3, 1),
                      tflops_fp32_equiv=round(flops / ms / 1e9, 2), rounds_ms=[round(v, 3) for v in t],
                      n_ops=plans[k].n_ops)
    out["x6_speedup"] = round(out["fp32_mfma"]["ms_per_forward"] / out["x6"]["ms_per_forward"], 3)
    d = (plans["x6"].out.float() - plans["fp32_mfma"].out.float()).abs().max().item()
    out["max_abs_diff_x6_vs_fp32"] = d
    print(json.dumps(out))


if __name__ == "__main__":
    main()
