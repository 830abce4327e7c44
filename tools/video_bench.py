"""Decode rate of a Motion-JPEG video (modules/utils/jpeg.py decode_video_batch, modules/utils/video.py) against the per-frame
path it replaces, in one process, the paths alternating pass by pass, medians over the passes:
    python tools/video_bench.py [n_frames] [threads] [passes] [--size 576x1024] [--ws_mb MiB]
  (a) the parent's path: decode_jpeg_batch (per frame: workspace, two launches) followed by torch.stack
  (b) decode_video_batch, entropy="host"      (c) decode_video_batch, entropy="device"
  (d) the device half alone on coefficients already on the device, HIP events around it: the per-frame fp_jpeg_reconstruct loop
      plus torch.stack, and fp_jpeg_reconstruct_batch in the chunks decode_video_batch cuts (VIDEO_WS_BYTES)
  (e) VideoReader.read from a file and VideoWriter.write of the same frames
The frames are synth.py's synthetic frames (16 distinct ones, cycled), encoded once at quality 90, 4:2:0."""
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from face_detection_and_recognition_amd.modules.utils import jpeg as J  # noqa: E402
from face_detection_and_recognition_amd.modules.utils.video import VideoReader, VideoWriter  # noqa: E402
from face_detection_and_recognition_amd.synth import synth_frames  # noqa: E402

size, ws_mb = "576x1024", None
for flag in ("--size", "--ws_mb"):
    if flag in sys.argv:
        k = sys.argv.index(flag)
        if flag == "--size":
            size = sys.argv[k + 1]
        else:
            ws_mb = float(sys.argv[k + 1])
        del sys.argv[k:k + 2]
if ws_mb is not None:                                  # another workspace cap than the shipped one, to compare
    J.VIDEO_WS_BYTES = int(ws_mb * (1 << 20))
FH, FW = (int(v) for v in size.split("x"))
n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
threads = int(sys.argv[2]) if len(sys.argv) > 2 else 16
passes = int(sys.argv[3]) if len(sys.argv) > 3 else 5
dev = torch.device("cuda:0")


def spread(v):
    return f"median {np.median(v):.4g} (min {min(v):.4g}, max {max(v):.4g})"


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3, out


distinct = torch.from_numpy(synth_frames(16, FH, FW, seed=5)).to(dev)
files = J.encode_jpeg_batch(list(distinct), quality=90, subsampling="4:2:0")
datas = [files[i % len(files)] for i in range(n)]
print(f"workspace cap {J.VIDEO_WS_BYTES / (1 << 20):.0f} MiB")
print(f"{n} frames {FH}x{FW} 4:2:0 q90 ({len(files)} distinct), {sum(len(d) for d in datas) / n / 1024:.0f} KiB each, "
      f"{threads} host threads, {passes} passes, alternating")

# ---- (a) (b) (c): end to end -------------------------------------------------------------------------------------------
paths = {
    "(a) decode_jpeg_batch + torch.stack": lambda: torch.stack(J.decode_jpeg_batch(datas, dev, threads=threads, orientation=False)),
    "(a') the same, entropy=device": lambda: torch.stack(J.decode_jpeg_batch(datas, dev, threads=threads, entropy="device", orientation=False)),
    "(b) decode_video_batch entropy=host": lambda: J.decode_video_batch(datas, dev, threads=threads),
    "(c) decode_video_batch entropy=device": lambda: J.decode_video_batch(datas, dev, threads=threads, entropy="device"),
}
ref = None
for name, fn in paths.items():                        # warm-up, and the three paths give the same tensor
    out = fn()
    ref = out if ref is None else ref
    assert torch.equal(out, ref), name
rates = {k: [] for k in paths}
for _ in range(passes):
    for name, fn in paths.items():
        rates[name].append(n / wall(fn)[0])
print("end to end, frames/s:")
for name, v in rates.items():
    print(f"  {name}: {spread(v)}")

# ---- (d): the device half alone ----------------------------------------------------------------------------------------
parsed = [J.parse(d) for d in datas]
info = parsed[0][0]
nc = int(info.n_coefs)
arena = torch.empty((n * nc,), dtype=torch.int16)
for i, d in enumerate(datas[:len(files)]):
    arena[i * nc:(i + 1) * nc] = J.entropy_decode(d)[1]
for i in range(len(files), n):
    arena[i * nc:(i + 1) * nc] = arena[(i % len(files)) * nc:(i % len(files) + 1) * nc]
arena = arena.to(dev)
views = [arena[i * nc:(i + 1) * nc] for i in range(n)]
infos = [p[0] for p in parsed]
quant = J._quant_rows(infos)
per = int(J.L.load().fp_jpeg_workspace_bytes(info))
step = max(1, J.VIDEO_WS_BYTES // per)
out = torch.empty((n, FH, FW, 3), dtype=torch.uint8, device=dev)


def loop():
    return torch.stack([J.reconstruct(infos[i], views[i], dev, orientation=1) for i in range(n)])


def batched():
    for s in range(0, n, step):
        e = min(n, s + step)
        J.reconstruct_batch(info, arena, np.arange(s, e, dtype=np.int64) * nc, quant[s:e], dev, out[s:e])
    return out


assert torch.equal(loop(), ref) and torch.equal(batched(), ref)
half = {"(d) per-frame fp_jpeg_reconstruct loop + torch.stack": loop, f"(d) fp_jpeg_reconstruct_batch, {-(-n // step)} calls of <= {step} frames": batched}
ms = {k: [] for k in half}
for _ in range(max(passes, 7)):
    for name, fn in half.items():
        ms[name].append(events(fn)[0] * 1e3)
print(f"device half alone on {n} frames' coefficients (on the device), HIP events, ms per batch:")
for name, v in ms.items():
    print(f"  {name}: {spread(v)}  = {np.median(v) / n * 1e3:.1f} us per frame")
a, b = (np.median(v) for v in ms.values())
la = list(ms.values())[0]
print(f"  batched / loop = {b / a:.3f} (the loop's own spread between its passes: {min(la) / np.median(la):.3f} .. {max(la) / np.median(la):.3f})")

# ---- (e): file to frames, frames to file -------------------------------------------------------------------------------
with tempfile.TemporaryDirectory() as tmp:
    path = os.path.join(tmp, "bench.avi")
    wr, rd = [], []
    for _ in range(passes):
        def write():
            with VideoWriter(path, 25, quality=90) as w:
                for s in range(0, n, 64):
                    w.write(ref[s:s + 64])
        wr.append(n / wall(write)[0])

        def read():
            with VideoReader(path) as r:
                return r.read(0, None, dev, threads=threads)
        dt, got = wall(read)
        rd.append(n / dt)
    mb = os.path.getsize(path) / 1e6
    print(f"file ({mb:.1f} MB AVI in the page cache; read throughput from a disk is not measured), frames/s:")
    print(f"  (e) VideoWriter.write, 64 frames a call (encode on the device + file): {spread(wr)}")
    print(f"  (e) VideoReader.read (mmap + decode_video_batch entropy=host): {spread(rd)}")
