"""Decode rate of the JPEG front end (modules/utils/jpeg.py) against Pillow on the host: 256 synthetic 576 x 1024 4:2:0 frames,
then the host and the device Huffman stage (entropy="host" / "device") alternated on the frames and on 1024 small crops.
    python tools/jpeg_bench.py [n_frames] [threads] [repeats]
With --reduce and / or --orientation the reduced-size / oriented reconstruction (csrc/jpegscale.hip) is measured instead, the
parent path (fp_jpeg_reconstruct) and the new one alternating in this one process:
    python tools/jpeg_bench.py [n_frames] [threads] [repeats] --reduce 1,2,4,8 --orientation 1,6 [--size 576x1024]"""
import io
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from face_detection_and_recognition_amd.modules.utils import jpeg as J  # noqa: E402
from PIL import Image  # noqa: E402

SCALED = {}
for flag in ("--reduce", "--orientation", "--size"):
    if flag in sys.argv:
        k = sys.argv.index(flag)
        SCALED[flag] = sys.argv[k + 1]
        del sys.argv[k:k + 2]
FH, FW = (int(v) for v in SCALED.get("--size", "576x1024").split("x"))
n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
threads = int(sys.argv[2]) if len(sys.argv) > 2 else 16
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
dev = torch.device("cuda:0")
rng = np.random.default_rng(0)
datas = []
for i in range(8):
    img = np.clip(np.cumsum(np.cumsum(rng.normal(0, 2.5, (FH, FW, 3)), 0), 1) * 0.2 + rng.normal(128, 20, (FH, FW, 3)), 0, 255).astype(np.uint8)
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=90, subsampling=2)
    datas.append(b.getvalue())
datas = [datas[i % 8] for i in range(n)]
print(f"{n} frames {FH}x{FW} 4:2:0 q90, {sum(len(d) for d in datas) / n / 1024:.0f} KiB each, {threads} host threads")


def scaled_leg():
    """The device half at reduce r, tag t against the parent's fp_jpeg_reconstruct, alternated round by round (each round: `iters`
    calls of one path on one frame's coefficients, already on the device, ending in a synchronise); tag 6 at reduce 1 also against
    the parent followed by torch.rot90(...).contiguous(); then whole batches through decode_jpeg_batch (host Huffman) at
    reduce 1 and r, alternated.  Prints medians over the rounds and each path's byte model."""
    reduces = [int(v) for v in SCALED.get("--reduce", "1").split(",")]
    tags = [int(v) for v in SCALED.get("--orientation", "1").split(",")]
    info, coefs = J.entropy_decode(datas[0], pinned=True)
    cd = coefs.to(dev)
    iters, rounds = (200 if FH * FW <= (1 << 20) else 40), max(5, repeats)
    coef_bytes = 2 * int(info.n_coefs)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e6

    parent_out = J.reconstruct(info, cd, dev)
    paths = {"parent fp_jpeg_reconstruct": lambda: J.reconstruct(info, cd, dev, out=parent_out),
             "parent + torch.rot90().contiguous()": lambda: torch.rot90(J.reconstruct(info, cd, dev, out=parent_out), -1, (0, 1)).contiguous()}
    lib, C = J.L.load(), J.C
    pws = torch.empty((int(lib.fp_jpeg_workspace_bytes(info)),), dtype=torch.uint8, device=dev)
    # (a): the same two launches without the Python layer in front of them (what a difference to the line above would show)
    paths["parent fp_jpeg_reconstruct, bare C call"] = lambda: lib.fp_jpeg_reconstruct(
        J.L.ptr(cd), C.byref(info), J.L.ptr(pws), pws.numel(), J.L.ptr(parent_out), 1, J.L.current_stream(dev))
    model = {"parent fp_jpeg_reconstruct": (coef_bytes, 2 * int(J.L.load().fp_jpeg_workspace_bytes(info)), 3 * FH * FW)}
    for r in reduces:
        for t in tags:
            if (r, t) == (1, 1):
                continue                  # the Python layer routes this to the parent's kernels: nothing new to time
            oh, ow = J.scaled_size(info, r, t)
            out = torch.empty((oh, ow, 3), dtype=torch.uint8, device=dev)
            name = f"scaled reduce={r} tag={t}"
            paths[name] = (lambda r=r, t=t, out=out: J.reconstruct(info, cd, dev, out=out, reduce=r, orientation=t))
            model[name] = (coef_bytes, 2 * int(J.L.load().fp_jpeg_scaled_workspace_bytes(info, r)), 3 * oh * ow)
    if 6 in tags and 1 in reduces:        # the fused kernel must give what the parent and a rotation give
        assert torch.equal(J.reconstruct(info, cd, dev, reduce=1, orientation=6), torch.rot90(parent_out, -1, (0, 1)))
    else:
        del paths["parent + torch.rot90().contiguous()"]
    for fn in paths.values():
        for _ in range(3):
            fn()
    times = {k: [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            times[k].append(timed(fn))
    print(f"device half on one {FH}x{FW} frame, {rounds} rounds of {iters} calls, alternating; us per frame: median (min - max)")
    print("  byte model: coefficient read (does not shrink with reduce: the kernel touches every block's DC line) + plane write and read + frame write")
    for k, v in times.items():
        extra = ""
        if k in model:
            c, p, o = model[k]
            extra = f"   bytes: coefs {c / 1e6:.2f} MB + planes {p / 1e6:.2f} MB + frame {o / 1e6:.2f} MB -> {(c + p + o) / np.median(v) / 1e3:.0f} GB/s"
        print(f"  {k}: {np.median(v):.1f} ({min(v):.1f} - {max(v):.1f}){extra}")
    # end to end: host Huffman on `threads` threads + upload + reconstruction
    e2e = {f"reduce={r}": (lambda r=r: J.decode_jpeg_batch(datas, dev, threads=threads, reduce=r, orientation=False)) for r in sorted(set([1] + reduces))}
    for fn in e2e.values():
        fn()
    rates = {k: [] for k in e2e}
    for _ in range(repeats):
        for k, fn in e2e.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            rates[k].append(n / (time.perf_counter() - t0))
    for k, v in rates.items():
        print(f"  decode_jpeg_batch of {n} files, host Huffman on {threads} threads, {k}: {' '.join(f'{x:.0f}' for x in v)} frames/s (median {np.median(v):.0f})")


if SCALED:
    scaled_leg()
    sys.exit(0)


def pil_one(d):
    return np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))


for name, fn in (("Pillow decode on the host + upload", lambda: torch.from_numpy(np.stack(list(ThreadPoolExecutor(threads).map(pil_one, datas)))).to(dev)),
                 ("host Huffman + device reconstruction", lambda: torch.stack(J.decode_jpeg_batch(datas, dev, threads=threads)))):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"{name}: {dt * 1e3:.1f} ms = {n / dt:.0f} frames/s  ({tuple(out.shape)})")
# the device half alone
info, coefs = J.entropy_decode(datas[0], pinned=True)
cd = coefs.to(dev)
out = J.reconstruct(info, cd, dev)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(200):
    J.reconstruct(info, cd, dev, out=out)
torch.cuda.synchronize()
print(f"device half alone: {(time.perf_counter() - t0) / 200 * 1e6:.1f} us per frame")
t0 = time.perf_counter()
for _ in range(20):
    J.entropy_decode(datas[0])
print(f"host half alone (one thread): {(time.perf_counter() - t0) / 20 * 1e3:.2f} ms per frame")


def alternate(label, files, repeats):
    """entropy="host" and entropy="device" decode_jpeg_batch, alternated, `repeats` times each (after one warm-up of each)."""
    fns = (("host Huffman", lambda: J.decode_jpeg_batch(files, dev, threads=threads)),
           ("device Huffman", lambda: J.decode_jpeg_batch(files, dev, threads=threads, entropy="device")))
    for _, fn in fns:
        fn()
    torch.cuda.synchronize()
    rates = {name: [] for name, _ in fns}
    for _ in range(repeats):
        for name, fn in fns:
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            rates[name].append(len(files) / (time.perf_counter() - t0))
    for name, r in rates.items():
        print(f"{label}, {name} + device reconstruction: {' '.join(f'{x:.0f}' for x in r)} frames/s (median {np.median(r):.0f})")


alternate(f"{n} frames", datas, repeats)
res = J.device_entropy_decode(datas, dev)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(5):
    res = J.device_entropy_decode(datas, dev)
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / 5
print(f"device Huffman stage alone ({n} frames, prepare + pack + copy + decode + status read-back): {dt * 1e3:.1f} ms = "
      f"{n / dt:.0f} frames/s, {sum(r is None for r in res)} left to the host")
crops = []
for i in range(16):
    h, w = 120 + 8 * i, 104 + 4 * i
    img = np.clip(np.cumsum(np.cumsum(rng.normal(0, 2.5, (h, w, 3)), 0), 1) * 0.2 + rng.normal(128, 20, (h, w, 3)), 0, 255).astype(np.uint8)
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=90, subsampling=2)
    crops.append(b.getvalue())
crops = [crops[i % 16] for i in range(1024)]
print(f"1024 crops {min(len(c) for c in crops) / 1024:.1f}-{max(len(c) for c in crops) / 1024:.1f} KiB")
alternate("1024 crops", crops, repeats)
