#!/usr/bin/env python3
"""Headline benchmark: faces/sec end-to-end (detect -> embed -> cosine-filter) on synthetic 576x1024 frames,
batch 256 per GPU (BASELINE.json configs[1]: BlazeFace back-camera 256^2 -> Mobile-FaceNet 112^2 -> cosine filter).

  python bench.py                         # 1 GPU, 200 timed steps after 10 warm-ups
  python bench.py --gpus 1 --steps 20 --warmup 5
  python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs DIR   # + the last timed step's outputs as DIR/<name>.npy
  python bench.py --gpus N --steps K --warmup W        # N > 1: starts N ranks ITSELF (launch_ranks below), one per GPU
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W         # ... or runs as one rank of an external launcher (WORLD_SIZE set)

One step = one pass of the hot path over one batch of 256 frames already resident in HBM: letterbox+normalise ->
BlazeFace-back forward -> anchor decode -> weighted NMS -> detections-to-crops -> crop/resize/normalise ->
Mobile-FaceNet -> cosine filter against a 10k-row reference set.  Workload as SURVEY 8(d) defines it: ~64 candidates
per frame before NMS, ~2 faces per frame after it (two textured patches per frame); the step rotates through
N_BATCHES different frame batches (seed + batch index), so no step re-reads the previous step's frames.
N > 1: frames shard by image, every rank processes its own 256 frames per step (weak scaling, no data-path
collective) and the similarity stage's exchange runs as north_star names it: RCCL all_gather of the step's embedding
matrix (fixed-capacity blocks + device-side counts, no host round trip), then every rank matches its faces against the
faces of all other ranks with the same HIP cosine kernel (face_detection_and_recognition_amd/distributed.py).
Rank 0 prints ONE JSON line (contract in the task statement) including `roofline` (dominant kernel family, HIP events
recorded on the launch stream during the timed steps) and `cpu_baseline` (the oracle timed on the host cores).

  --workload c5: BASELINE configs[4], the sharded similarity filter alone: 125 k gallery rows per rank x 10 k reference
  rows (10 k / N produced per rank, one all_gather of equal blocks), fused row-max cosine kernel.
"""
import argparse
import contextlib
import ctypes
import glob
import json
import os
import sys
import time



def cpu_budget():
    """Host cores this process may actually use: the scheduler affinity, capped by the cgroup CPU quota.  (A gpurun box shows
    256 cores in its affinity mask and has a quota of 16: a thread pool sized by the mask -- torch's default there is 128
    threads -- spends its time being throttled.)"""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    for path, parse in (("/sys/fs/cgroup/cpu.max", lambda t: t.split()),
                        ("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", lambda t: (t.strip(), open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read().strip()))):
        try:
            quota, period = parse(open(path).read())
            if quota != "max" and int(quota) > 0:
                n = min(n, max(1, int(quota) // int(period)))
            break
        except (OSError, ValueError):
            continue
    return max(1, n)


def launch_ranks(n, argv):
    """`bench.py --gpus N` without an external launcher: start N fresh rank processes of this script (RANK / LOCAL_RANK /
    WORLD_SIZE / MASTER_* set, rendezvous on 127.0.0.1), relay rank 0's single JSON line
    to this process's stdout and return non-zero if any rank fails or the line does not report n_gpus == N.  The parent
    imports neither torch nor the HIP library and makes NO GPU call (a process that has touched the GPU must not be
    replaced or forked from); children are started with subprocess (fork + exec of a fresh interpreter) and stopped, if
    one of them dies, by their exact PIDs."""
    import socket
    import subprocess
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cores = cpu_budget()
    procs = []
    for r in range(n):
        env = dict(os.environ)
        env.update(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), BENCH_LAUNCHED_BY="bench.py")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        env.setdefault("OMP_NUM_THREADS", str(max(1, cores // n)))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env,
                                      stdout=subprocess.PIPE if r == 0 else sys.stderr.fileno()))
    import threading
    chunks = []                               # rank 0's stdout is drained while it runs (a full pipe would block it)
    reader = threading.Thread(target=lambda: chunks.append(procs[0].stdout.read()), daemon=True)
    reader.start()
    deadline = time.time() + float(os.environ.get("BENCH_LAUNCH_TIMEOUT", "1500"))
    failed = None
    while failed is None and any(p.poll() is None for p in procs):
        for r, p in enumerate(procs):
            if p.poll() not in (None, 0):
                failed = (r, p.returncode)
        if time.time() > deadline:
            failed = (-1, 124)
        time.sleep(0.05)
    if failed is None:
        for r, p in enumerate(procs):
            if p.returncode != 0:
                failed = (r, p.returncode)
    if failed is not None:
        for p in procs:                       # the exact processes started above, nothing else
            if p.poll() is None:
                p.terminate()
        t_kill = time.time() + 10
        for p in procs:
            while p.poll() is None and time.time() < t_kill:
                time.sleep(0.05)
            if p.poll() is None:
                p.kill()
        reader.join(timeout=5)
        sys.stderr.write(f"bench.py launcher: rank {failed[0]} failed (exit code {failed[1]}); all ranks stopped\n"
                         if failed[0] >= 0 else "bench.py launcher: timed out; all ranks stopped\n")
        return failed[1] if 0 < failed[1] < 256 else 1
    reader.join(timeout=30)
    out = b"".join(chunks).decode()
    lines = [ln for ln in out.splitlines() if ln.strip()]
    try:
        rec = json.loads(lines[-1])
    except Exception:
        sys.stderr.write(f"bench.py launcher: rank 0 printed no JSON line (stdout: {out[-300:]!r})\n")
        return 1
    if len(lines) != 1 or rec.get("n_gpus") != n or (rec.get("launch") or {}).get("world_size") != n:
        sys.stderr.write(f"bench.py launcher: asked for {n} ranks, the line reports n_gpus = {rec.get('n_gpus')}, "
                         f"world_size = {(rec.get('launch') or {}).get('world_size')} ({len(lines)} line(s))\n")
        return 1
    sys.stdout.write(lines[-1] + "\n")
    sys.stdout.flush()
    return 0


def _requested_gpus(argv):
    for i, a in enumerate(argv):
        if a == "--gpus" and i + 1 < len(argv):
            return int(argv[i + 1])
        if a.startswith("--gpus="):
            return int(a.split("=", 1)[1])
    return 1


if __name__ == "__main__" and "WORLD_SIZE" not in os.environ and _requested_gpus(sys.argv[1:]) > 1:
    sys.exit(launch_ranks(_requested_gpus(sys.argv[1:]), sys.argv[1:]))      # before torch / HIP are even imported
os.environ.setdefault("OMP_NUM_THREADS", str(cpu_budget()))     # (read when torch's thread pools come up)

# how this process came to be (before init_dist fills in defaults): started by launch_ranks, by an external launcher, or alone
LAUNCH_MODE = ("self-launched (bench.py started the ranks)" if os.environ.get("BENCH_LAUNCHED_BY") == "bench.py" else
               "external launcher (WORLD_SIZE in the environment)" if "WORLD_SIZE" in os.environ else "in-process, one rank")

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from face_detection_and_recognition_amd import similarity as S  # noqa: E402
from face_detection_and_recognition_amd import workload as W  # noqa: E402
from face_detection_and_recognition_amd.pipeline import FacePipeline  # noqa: E402

DTYPE_LABEL = "f32 (bf16x6 split GEMMs)"   # fp32 operands and accumulation; the GEMM products as six bf16 MFMA products (csrc/split.h)
HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E 8.0 TB/s (spec)
FP32_MFMA_PEAK_TF = 157.3  # MI355X_MICROARCH.md: dense fp32 matrix peak (= the fp32 vector rate); SURVEY 8(d)'s fp32 roofline
BF16_MFMA_PEAK_TF = 2500.0 # MI355X_MICROARCH.md: dense bf16 matrix peak
X6_PEAK_TF = BF16_MFMA_PEAK_TF / 6.0   # fp32 products as six bf16 MFMA products each (csrc/split.h): 416.7 TFLOP/s fp32-equivalent
MFMA_F32_PEAK_TFS = 157.3  # MI355X_MICROARCH.md: fp32 MFMA = fp32 vector peak
B_FRAMES = 256
N_BATCHES = 4              # distinct frame batches the timed steps rotate through
N_REF = 10000
EMB_CAP_ROWS = 1024        # STARTING all_gather block rows per rank (~512 faces per step at 2 faces / frame); StepExchange grows it
FRAME_BYTES = 576 * 1024 * 3
LETTERBOX_OUT_BYTES = 256 * 256 * 3 * 4


def host_cores():
    """Threads for the CPU baseline: the box's CPU share (16 per GPU on the pool), never more than the affinity / cgroup quota."""
    return max(1, min(16, cpu_budget()))


def cpu_baseline(det_model, emb_model, ref, frames_cpu, tau, budget_s=25.0):
    """The oracle (CPU restatement of the reference, torch-CPU fp32 + numpy) on a bounded sample of the same
    workload, all host cores.  Baseline only: it is never the thing shipped or the target."""
    import numpy as np
    from oracle import blazeface_ref, image_ref, mobilefacenet_ref, similarity_ref
    torch.set_num_threads(host_cores())
    sd_det = {k: v.detach().cpu() for k, v in det_model.net.state_dict().items()}
    sd_emb = {k: v.detach().cpu() for k, v in emb_model.state_dict().items()}
    anchors = det_model.net.anchors.cpu()
    refn = ref.cpu().numpy()
    frames = frames_cpu.numpy()
    iw, ih = det_model.input_size
    t0 = time.perf_counter()
    n_faces = n_frames = 0
    embs = []
    with torch.no_grad():
        for f in frames:                                            # the reference runs one frame per call
            if time.perf_counter() - t0 > budget_s:
                break
            n_frames += 1
            lb = image_ref.pad_resize_image(f, (iw, ih))[..., ::-1].copy()
            x = torch.from_numpy(lb).permute(2, 0, 1).unsqueeze(0)
            faces, _ = blazeface_ref.predict_on_batch(sd_det, x, anchors, True)
            d = faces[0].numpy()
            if len(d) == 0:
                continue
            d = d[:, [1, 0, 3, 2] + list(range(4, 17))]
            post = image_ref.dets_to_boxes(d.copy(), (f.shape[1], f.shape[0]), (iw, ih), det_model.det_thres,
                                           det_model.bbox_area_thres)
            for box in post["boxes"]:
                crop, _ = image_ref.crop_face(f, box)
                if crop.size == 0:
                    continue
                face = image_ref.mfn_lut()[image_ref.resize_bilinear_u8(crop, (112, 112))]
                xin = torch.from_numpy(np.ascontiguousarray(face.transpose(2, 0, 1))).unsqueeze(0)
                embs.append(mobilefacenet_ref.forward(sd_emb, xin)[0].numpy())
                n_faces += 1
        if embs:
            similarity_ref.cosine_filter(np.stack(embs), refn, tau)
    dt = time.perf_counter() - t0
    return n_faces / dt, n_faces, n_frames, dt


def latest_pmc_traffic():
    """(file name, {kernel family: hbm bytes per launch}) of the newest committed PMC summary, or (None, {}).
    The figures come from separate `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` passes of this same command
    (gfx950: FETCH_SIZE doubled, MI355X_MICROARCH.md), summarised by tools/profile_summary.py -- they are NOT measured
    in this run, which is why the JSON line names the file."""
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_bench_pmc_traffic.json"))) or \
        sorted(glob.glob(os.path.join(ROOT, "profiles", "r??_pmc_traffic.json")))
    if not files:
        return None, {}
    try:
        return os.path.relpath(files[-1], ROOT), json.load(open(files[-1]))
    except Exception:
        return None, {}


def init_dist():
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    # test hooks (single-GPU rehearsal of the multi-rank path): BENCH_DIST_BACKEND=gloo BENCH_SAME_DEVICE=1
    backend = os.environ.get("BENCH_DIST_BACKEND", "nccl")
    if os.environ.get("BENCH_SAME_DEVICE") == "1":
        local_rank = 0
    # BENCH_FORCE_DIST=1: initialise the process group and run the exchange even with one rank (exercises RCCL itself
    # on a one-GPU box; the timing of such a run is not a benchmark result)
    if world > 1 or os.environ.get("BENCH_FORCE_DIST") == "1":
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        torch.cuda.set_device(local_rank)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)
    if os.environ.get("BENCH_MAIN_PRIO"):      # lab (tools/lab/stream_prio_ab.sh): the detector's stream at another priority
        torch.cuda.set_stream(torch.cuda.Stream(dev, priority=int(os.environ["BENCH_MAIN_PRIO"])))
    return world, rank, dev, dist, backend


def check_world(args, world):
    """`--gpus` must be the number of ranks that actually run: a line that says n_gpus = 1 for a `--gpus 8` command (or the
    reverse) would be a scaling point measured on the wrong job.  Fails on every rank, before any work."""
    if args.gpus != world and not os.environ.get("BENCH_FORCE_DIST"):
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE = {world}: run `python bench.py --gpus {args.gpus}` "
                         f"(it starts the ranks itself) or launch exactly --gpus ranks")


def launch_record(args, world, rank, dev, dist, backend, count):
    """What the result line says about the job's shape: the world size the process group itself reports, the collective
    library, every rank's device and every rank's share of the processed units (all gathered through the group)."""
    rec = {"mode": LAUNCH_MODE, "requested_gpus": args.gpus, "world_size": world, "backend": None, "units_per_rank": [count], "devices": None}
    if dist is None:
        return rec
    mine = {"rank": rank, "units": int(count), "device": str(dev)}
    if dev is not None and dev.type == "cuda":
        props = torch.cuda.get_device_properties(dev)
        mine["device"] = f"{dev} {props.name}" + (f" {props.uuid}" if hasattr(props, "uuid") else "")
    got = [None] * dist.get_world_size()
    dist.all_gather_object(got, mine)
    rec["world_size"] = dist.get_world_size()
    rec["units_per_rank"] = [g["units"] for g in got]
    rec["devices"] = [g["device"] for g in got]
    if backend == "nccl":
        rec["backend"] = "nccl = RCCL " + ".".join(str(v) for v in torch.cuda.nccl.version())
    else:
        rec["backend"] = backend + " (CPU rehearsal)"
    return rec


def run_stub(args):
    """BENCH_STUB_STEP=1 (tests, no GPU): the launcher, the rendezvous, the reductions and the result line with a stub in
    place of the step -- every rank 'finds' 100 + rank faces per step in a gloo group on the CPU."""
    import torch.distributed as dist
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    check_world(args, world)
    if os.environ.get("BENCH_STUB_FAIL_RANK") == str(rank):
        raise SystemExit(3)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", "1")
    dist.init_process_group("gloo")

    def barrier():      # not dist.barrier(): it asks torch for the accelerator, which opens the GPU, and the stub must not
        dist.all_reduce(torch.zeros(1))
    barrier()
    t0 = time.perf_counter()
    faces = 0
    for _ in range(args.steps):
        time.sleep(0.001)
        faces += 100 + rank
    barrier()
    elapsed, faces_all = reduce_time_and_count(time.perf_counter() - t0, faces, max(world, 2), dist, None, "gloo")
    launch = launch_record(args, world, rank, torch.device("cpu"), dist, "gloo", faces)
    if rank == 0:
        emit_line({"metric": "faces/sec end-to-end (detect->embed->cosine-filter), 576x1024 batch=256", "stub": True,
                   "value": round(faces_all / elapsed, 1), "unit": "faces/s", "n_gpus": world, "steps": args.steps,
                   "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True,
                   "scaling": "weak", "vs_baseline": None, "dtype": DTYPE_LABEL, "data": "synthetic",
                   "config": {"workload": "STUB step (launcher test, no GPU work)"}, "launch": launch,
                   "roofline": None, "cpu_baseline": None})
    dist.destroy_process_group()


def reduce_time_and_count(elapsed, count, world, dist, dev, backend):
    """MAX of the elapsed time and SUM of the processed units over ranks."""
    if world == 1 or dist is None:
        return elapsed, float(count)
    rdev = dev if backend == "nccl" else torch.device("cpu")
    tmax = torch.tensor([elapsed], dtype=torch.float64, device=rdev)
    fsum = torch.tensor([float(count)], dtype=torch.float64, device=rdev)
    dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dist.all_reduce(fsum, op=dist.ReduceOp.SUM)
    return float(tmax), float(fsum)


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(path, arrays):
    """--dump-outputs: every array as `path/<name>.npy`, floating point as float32 (float64 stays float64), integers and
    booleans as float64 (exact).  Past DUMP_LIMIT_BYTES in all, every array keeps the same fixed, seeded sample of its rows,
    so that two builds run with the same arguments compare output for output."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    host = {}
    for name, a in arrays.items():
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        host[name] = a.astype(np.float32 if np.issubdtype(a.dtype, np.floating) and a.dtype != np.float64 else np.float64)
    total = sum(a.nbytes for a in host.values())
    if total > DUMP_LIMIT_BYTES:
        for name, a in host.items():
            if a.ndim and a.shape[0] > 1:
                rows = np.random.default_rng(0).choice(a.shape[0], max(1, a.shape[0] * DUMP_LIMIT_BYTES // total), replace=False)
                host[name] = a[np.sort(rows)]
    for name, a in host.items():
        np.save(os.path.join(path, name + ".npy"), a)


# ---------------------------------------------------------------------------------------------------------------
def run_pipeline(args):
    check_world(args, int(os.environ.get("WORLD_SIZE", "1")))
    world, rank, dev, dist, backend = init_dist()
    from face_detection_and_recognition_amd.modules.mobile_facenet.mobile_facenet import Depth_Wise
    Depth_Wise.X6 = args.mfma == "bf16x6"

    # ---- workload (off the clock) ----
    batches = [W.make_frames(B_FRAMES, dev, seed=1234 + 97 * rank + b) for b in range(N_BATCHES)]
    det = W.build_detector(dev, W.make_frames(64, dev, seed=999), box_px=args.box_px)   # same calibration on every rank
    emb = W.build_embedder(dev)
    ref = W.make_reference(N_REF, dev)
    pipe = FacePipeline(det, emb, ref, tau=0.3, two_streams=args.overlap == 2)
    exchange = None
    multi = dist is not None
    if multi:
        # The step's exchange (all_gather of the embedding blocks + counts, cross-rank cosine match) runs on a side stream
        # BESIDE the next step's detector and is consumed one step late (distributed.StepExchange): ranks meet inside a
        # collective only when one of them is a whole step ahead, instead of in every step.
        from face_detection_and_recognition_amd import distributed as D
        if backend == "nccl":               # RCCL over xGMI + the HIP cosine kernel on the gathered matrix
            exchange = D.StepExchange(EMB_CAP_ROWS, emb.embedding_size, dev, pipe.tau,
                                      lambda G, R, tau, rinv: S.cosine_filter(G, R, tau, rinv=rinv), S.row_inv_norm)
        else:                               # gloo rehearsal: collectives on host copies, kernel on the device
            exchange = D.StepExchange(EMB_CAP_ROWS, emb.embedding_size, dev, pipe.tau,
                                      lambda G, R, tau, rinv: S.cosine_filter(G.to(dev), R.to(dev), tau, rinv=rinv.to(dev)),
                                      lambda R: S.row_inv_norm(R.to(dev)).cpu(), comm=lambda t: t.cpu())

    matched = [0]
    last_out = [None]                           # the result dict of the most recent step (--dump-outputs)

    def finish(out):
        last_out[0] = out
        n = out["n_faces"]
        if multi:
            # two-stream step: the embeddings come from the embedder's stream, and the exchange is queued THERE (its copy into
            # the gather block, the wait for the slot's previous exchange), so the detector stream never waits for an embedder
            ctx = torch.cuda.stream(pipe.emb_stream) if "done" in out else contextlib.nullcontext()
            with ctx:
                prev = exchange.submit(out["emb"], n)   # result of the previous step's exchange (None on the first)
            if prev is not None:
                matched[0] += 1
        return n

    def step(k):
        """One whole step: the detector stages of batch k, the host read of its face count, embedder, filter."""
        return finish(pipe.step(batches[k % N_BATCHES]))

    def run_steps(k0, count):
        """`count` steps starting at batch index k0 -> faces per step.  --overlap: software-pipelined
        (FacePipeline.step_overlapped: the detector of batch k + 1 is enqueued before the host reads batch k's face
        count, so the GPU queue never drains during the round trip); every batch is finished inside the call."""
        if not args.overlap:
            return [step(k0 + i) for i in range(count)]
        ns = []
        for i in range(count):
            out = pipe.step_overlapped(batches[(k0 + i) % N_BATCHES])
            if out is not None:
                ns.append(finish(out))
        ns.append(finish(pipe.flush()))
        return ns

    # off the clock, before the W warm-up steps: one pass over the batches builds every plan (detector, embedder, the embedder's
    # remainder plan) and loads every kernel; the probe pass below needs the plans.  The W warm-up steps themselves run LAST,
    # directly in front of the timed region, so that it starts from the clocks and caches of a running pipeline and not from a
    # GPU that idled through the probe's bookkeeping (with K = 20 timed steps that ramp was 2 % of the line).
    old_order = os.environ.get("BENCH_OLD_ORDER") == "1"      # lab: round 3's order (warm-up first), for the A/B
    run_steps(0, max(args.warmup, N_BATCHES) if old_order else N_BATCHES)
    torch.cuda.synchronize()

    # ---- per-op timers for the roofline figures ----
    # HIP events around an op cost a little, so: one un-timed probe pass over the batches with events on every op
    # finds the dominant kernel family; the timed steps then carry events only on that family's launches.
    det_plan = det.net.last_plan
    emb_plan = pipe.emb_plan                   # one plan (arena capacity >= every step's face count), run on n_pad crops
    plans = [det_plan, emb_plan]
    fam_steps = {}
    split_tail, pipe.split_tail = pipe.split_tail, False      # exclusive figures: nothing beside the op that is timed
    for k in range(N_BATCHES):
        probe = [p.new_timer() for p in plans]
        for p, t in zip(plans, probe):
            p._timing = (t, bytes([1] * p.n_ops))
        finish(pipe.step(batches[k % N_BATCHES], beside=args.overlap == 2))   # the plans of the timed steps, alone on the GPU
        torch.cuda.synchronize()
        step_ms = {}
        for p, t in zip(plans, probe):
            p._timing = None
            ms0 = (ctypes.c_float * p.n_ops)()
            p.accumulate(t, ms0)
            p.destroy_timer(t)
            for i in range(p.n_ops):
                step_ms[p.kernel_name(i)] = step_ms.get(p.kernel_name(i), 0.0) + ms0[i]
            if os.environ.get("BENCH_DEBUG_PROBE"):
                sys.stderr.write(f"probe step {k} plan N={p.N} n_run={p.n_run}: " +
                                 " ".join(f"{p.kernel_name(i).split('<')[0]}:{ms0[i] * 1e3:.0f}" for i in range(p.n_ops)) + "\n")
        for name, v in step_ms.items():
            fam_steps.setdefault(name, []).append(v)
    pipe.split_tail = split_tail
    # per family: the MEDIAN probe step x the number of probe steps (one disturbed launch must not pick the family)
    fam_ms = {name: sorted(v)[len(v) // 2] * len(v) for name, v in fam_steps.items()}
    dom = max(fam_ms, key=fam_ms.get)
    probe_share = fam_ms[dom] / sum(fam_ms.values())
    probe_launches = sum(1 for p in plans for i in range(p.n_ops) if p.kernel_name(i) == dom) * N_BATCHES
    excl_us = fam_ms[dom] * 1e3 / max(probe_launches, 1)   # the family's launch time when nothing else shares the GPU
    masks = [bytes([1 if p.kernel_name(i) == dom else 0 for i in range(p.n_ops)]) for p in plans]
    timers = [[p.new_timer() for p in plans] for _ in range(args.steps)]

    def family_exclusive(name):
        """A family's figures from the probe pass alone (each launch alone on the GPU): launches per step, average launch time,
        compulsory bytes and reference FLOPs per launch, the roofline fraction of its own bound."""
        ops = [(p, i) for p in plans for i in range(p.n_ops) if p.kernel_name(i) == name]
        if not ops:
            return None
        us = fam_ms[name] * 1e3 / (len(ops) * N_BATCHES)
        n_emb = pipe.emb_n_pad
        byt = sum(p.compulsory_bytes(i, p.N if p is det_plan else n_emb) for p, i in ops) / len(ops)
        flp = sum(p.flops(i, p.N if p is det_plan else n_emb) for p, i in ops) / len(ops)
        bound = ops[0][0].bound(ops[0][1])
        rec = {"kernel": name, "bound": bound, "launches_per_step": len(ops), "exclusive_avg_launch_us": round(us, 2),
               "share_of_network_kernel_time": round(fam_ms[name] / sum(fam_ms.values()), 3)}
        if bound == "mfma":
            tf = flp / (us * 1e-6) / 1e12
            rec.update({"exclusive_TFLOPs": round(tf, 1), "exclusive_frac": round(tf / X6_PEAK_TF, 4), "peak": round(X6_PEAK_TF, 1)})
        else:
            gb = byt / (us * 1e-6) / 1e9
            rec.update({"exclusive_GBps": round(gb, 1), "exclusive_frac": round(gb / HBM_PEAK_GBS, 4), "peak": HBM_PEAK_GBS})
        return rec
    ranked = sorted(fam_ms, key=fam_ms.get, reverse=True)
    runners_up = [family_exclusive(nm) for nm in ranked[1:4]]

    if not old_order and args.warmup > 0:
        run_steps(0, args.warmup)              # the W untimed warm-up steps (same form as the timed ones)
    if multi:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if args.overlap:
        # the dominant family's HIP events ride along on the first plan runs of the region (a timer per plan run)
        run_idx = [0, 0]

        def arm(which):
            def hook(plan_run):
                def wrapped(*a, **kw):
                    k = run_idx[which]
                    run_idx[which] += 1
                    plans[which]._timing = (timers[k][which], masks[which]) if k < args.steps else None
                    return plan_run(*a, **kw)
                return wrapped
            return hook
        for which, p in enumerate(plans):
            p.run = arm(which)(type(p).run.__get__(p))
        faces_per_step = run_steps(0, args.steps)
        for p in plans:
            del p.run
    else:
        faces_per_step = []
        for k in range(args.steps):
            for p, t, m in zip(plans, timers[k], masks):
                p._timing = (t, m)
            faces_per_step.append(step(k))
    faces = sum(faces_per_step)
    if multi:
        with (torch.cuda.stream(pipe.emb_stream) if pipe.emb_stream is not None else contextlib.nullcontext()):
            exchange.drain()                             # the last step's exchange belongs to the timed region
    torch.cuda.synchronize()
    if multi:
        dist.barrier()
    t1 = time.perf_counter()
    for p in plans:
        p._timing = None
    if args.dump_outputs and rank == 0:
        # what the last timed step handed its caller (FacePipeline.step): face count, crop records, embeddings, filter result
        dump_outputs(args.dump_outputs, {k: v for k, v in last_out[0].items() if k != "done"})

    elapsed, faces_all = reduce_time_and_count(t1 - t0, faces, world if not multi else max(world, 2), dist, dev, backend)
    launch = launch_record(args, world, rank, dev, dist, backend, faces)

    # ---- roofline of the dominant kernel family (rank 0) ----
    roof = None
    if rank == 0:
        # Two byte models.  PHYSICAL (`achieved`, `frac`): what the launch must move -- its input tensor(s) once + its
        # output once (plan.compulsory_bytes; a fused op is not charged for tensors that never exist) -- so frac <= 1 by
        # construction.  OP-GRANULAR (`op_granular_*`): SURVEY 8(d)'s model, every conv of the reference reads its input
        # and writes its output; a fused kernel beats it by design (values > 1 there measure fusion, not bandwidth).
        ms_tot, launches, alg_tot, phys_tot, pipe_alg, pipe_phys, flop_tot, dom_bound = 0.0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, "hbm"
        for k in range(args.steps):
            n_k = faces_per_step[k]
            n_pad = (n_k + pipe.bucket - 1) // pipe.bucket * pipe.bucket
            for p, t, m in zip(plans, timers[k], masks):
                ms = (ctypes.c_float * p.n_ops)()
                p.accumulate(t, ms)
                p.destroy_timer(t)
                # Mobile-FaceNet's plan is emitted for its arena capacity and run on the step's crops (padded to a
                # multiple of 8): op-granular bytes count the REAL faces of the step, physical bytes the crops it ran on
                real = 1.0 if p is det_plan else n_k / float(p.N)
                n_run = p.N if p is det_plan else n_pad
                for i in range(p.n_ops):
                    pipe_alg += p.algorithmic_bytes(i) * real
                    pipe_phys += p.compulsory_bytes(i, n_run)
                    if m[i]:
                        ms_tot += ms[i]
                        launches += 1
                        alg_tot += p.algorithmic_bytes(i) * real
                        phys_tot += p.compulsory_bytes(i, n_run)
                        flop_tot += p.flops(i, n_run)
                        dom_bound = p.bound(i)
        pipe_alg = pipe_alg / args.steps + B_FRAMES * (FRAME_BYTES + LETTERBOX_OUT_BYTES)
        pipe_phys = pipe_phys / args.steps
        achieved = phys_tot / (ms_tot * 1e-3) / 1e9 if ms_tot > 0 else 0.0
        op_gran = alg_tot / (ms_tot * 1e-3) / 1e9 if ms_tot > 0 else 0.0
        avg_us = ms_tot * 1e3 / max(launches, 1)
        src, table = latest_pmc_traffic()
        traffic = table.get(dom, {}).get("hbm_bytes_per_launch")
        step_s = elapsed / args.steps
        roof = {"bound": "hbm", "kernel": dom, "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic,
                "traffic_source": (f"{src} (committed rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command; "
                                   "not measured in this run)") if traffic is not None else None,
                "hbm_frac_from_traffic": round(traffic / (avg_us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)
                if traffic else None,
                "avg_launch_us": round(avg_us, 2), "launches_per_step": round(launches / args.steps, 2),
                "bytes_per_launch": int(phys_tot / max(launches, 1)),
                "op_granular_GBps": round(op_gran, 1), "op_granular_frac": round(op_gran / HBM_PEAK_GBS, 4),
                "op_granular_bytes_per_launch": int(alg_tot / max(launches, 1)),
                "share_of_network_kernel_time": round(probe_share, 3),
                "exclusive_avg_launch_us": round(excl_us, 2),
                "exclusive_frac": round(phys_tot / max(launches, 1) / (excl_us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4) if excl_us > 0 else None,
                "streams": 2 if args.overlap == 2 else 1,
                "runners_up": runners_up,
                "pipeline_GBps": round(pipe_phys / step_s / 1e9, 1),
                "pipeline_frac": round(pipe_phys / step_s / 1e9 / HBM_PEAK_GBS, 4),
                "pipeline_op_granular_GBps": round(pipe_alg / step_s / 1e9, 1),
                "pipeline_op_granular_frac": round(pipe_alg / step_s / 1e9 / HBM_PEAK_GBS, 4),
                "model": ("streams = 2: the timed steps run the detector of batch k + 1 and embed + filter of batch k on two "
                          "streams, so a launch shares the CUs with the other network's kernels and achieved / frac (HIP events "
                          "in the timed region) are LOWER BOUNDS of the kernel's own rate; exclusive_* = the same launches in "
                          "the un-timed single-stream probe pass.  " if args.overlap == 2 else "") +
                         "achieved / frac / pipeline_frac: bytes the launch must move (every input tensor once + every "
                         "output once; tensors inside a fused op are not counted) / HIP-event time / 8 TB/s; op_granular_*: "
                         "SURVEY 8(d)'s model (every reference conv reads its input and writes its output), which a fused "
                         "kernel beats by design; hbm_frac_from_traffic: PMC bytes of the committed profile / launch time"}
        if dom_bound == "mfma":
            # the dominant family is a split-MFMA block: bound by matrix-core issue, not by HBM.  achieved = the reference's
            # conv FLOPs of the launch / HIP-event time; peak = the fp32 matrix peak SURVEY 8(d) prices fp32 GEMMs at;
            # matrix_pipe_frac = the bf16 MFMA work actually issued (six products per fp32 product) / the bf16 peak
            tf = flop_tot / (ms_tot * 1e-3) / 1e12 if ms_tot > 0 else 0.0
            roof.update({"bound": "mfma", "achieved": round(tf, 1), "peak": round(X6_PEAK_TF, 1), "unit": "TFLOP/s",
                         "frac": round(tf / X6_PEAK_TF, 4),
                         "vs_fp32_mfma_peak": round(tf / FP32_MFMA_PEAK_TF, 4),
                         "hbm_GBps": round(achieved, 1), "hbm_frac": round(achieved / HBM_PEAK_GBS, 4),
                         "flops_per_launch": int(flop_tot / max(launches, 1)),
                         "exclusive_frac": round(flop_tot / max(launches, 1) / (excl_us * 1e-6) / 1e12 / X6_PEAK_TF, 4)
                         if excl_us > 0 else None})
            roof["model"] = ("bound mfma: achieved = reference conv FLOPs of the launch (fp32 semantics) / HIP-event time; the kernel "
                             "computes every fp32 product as six bf16 MFMA products, so peak = 2.5 PF dense bf16 / 6 = 416.7 TF/s "
                             "fp32-equivalent and frac is the matrix-pipe utilisation; vs_fp32_mfma_peak = achieved / 157.3 TF/s, "
                             "the fp32 MFMA peak SURVEY 8(d) prices fp32 GEMMs at; hbm_*: "
                             "compulsory bytes / time; " + roof["model"])

    # ---- the same step with every GEMM on the fp32 MFMA (outside the timed region; rank 0, N = 1) ----
    arith = None
    if rank == 0:
        arith = {"mobilefacenet_depth_wise": args.mfma,
                 "note": "bf16x6: fp32 operands split EXACTLY into three bf16 pieces by round-to-nearest cuts (w == h + m + l, "
                         "|m| <= 2^-8 |w|, |l| <= 2^-16 |w|), six of the nine products on v_mfma_f32_16x16x32_bf16, fp32 "
                         "accumulation; the three dropped products are < 2^-22.99 of a product (one fp32 rounding unit) and carry "
                         "either sign; measured against fp64 on adversarial operands (all-ones mantissas, rounding ties, "
                         "all-positive rows, K up to 1152: tests/test_gpu_parity.py test_split_gemms_adversarial_vs_fp64) the "
                         "error is below the k-ordered fp32 fmaf chain's, or 2^-23 of sum |a b| where that chain is exact; "
                         "everything else fp32 throughout"}
        if world == 1 and args.mfma == "bf16x6" and not args.no_fp32_leg:
            # (both legs: single stream, every step self-contained -- FacePipeline.step -- so that they compare with each other)
            for k in range(2):
                step(k)
            torch.cuda.synchronize()
            tq = time.perf_counter()
            nq = sum(step(k) for k in range(20))
            torch.cuda.synchronize()
            dq = time.perf_counter() - tq
            arith["split_mfma_single_stream"] = {"ms_per_step": round(dq / 20 * 1e3, 3), "faces_per_s": round(nq / dq, 1), "steps": 20}
            Depth_Wise.X6 = False
            try:
                for k in range(3):
                    step(k)
                torch.cuda.synchronize()
                tq = time.perf_counter()
                nq = sum(step(k) for k in range(20))
                torch.cuda.synchronize()
                dq = time.perf_counter() - tq
                arith["fp32_mfma_only"] = {"ms_per_step": round(dq / 20 * 1e3, 3), "faces_per_s": round(nq / dq, 1), "steps": 20}
            finally:
                Depth_Wise.X6 = True

    cpu = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        v, n_cpu, nfr, dt = cpu_baseline(det, emb, ref, batches[0][:args.cpu_frames].cpu(), pipe.tau)
        cpu = {"value": round(v, 2), "unit": "faces/s", "cores": host_cores(), "kind": "port",
               "sample": f"first {nfr} frames of batch 0 (time-boxed), one frame per call like the reference: "
                         f"{n_cpu} faces in {dt:.1f} s, torch-CPU fp32 oracle"}

    # ---- the other BASELINE configs, short legs after the timed region (rank 0, N = 1): driver-visible, not the headline ----
    others = None
    if rank == 0 and world == 1 and not args.no_other_configs:
        from tools.config_bench import other_configs
        others = other_configs(dev)

    if rank == 0:
        line = {
            "metric": "faces/sec end-to-end (detect->embed->cosine-filter), 576x1024 batch=256",
            "value": round(faces_all / elapsed, 1), "unit": "faces/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": DTYPE_LABEL if args.mfma == "bf16x6" else "f32", "data": "synthetic",
            "launch": launch,
            "config": {"workload": "BlazeFace back-camera 256x256, batch 256 synthetic 576x1024 frames per GPU -> "
                                   "weighted NMS -> Mobile-FaceNet 112x112 -> cosine filter vs 10k x 512 reference",
                       "frames_per_step_per_gpu": B_FRAMES, "frame_batches_rotated": N_BATCHES,
                       "faces_per_frame": round(faces_all / world / args.steps / B_FRAMES, 3),
                       "frames_per_s": round(B_FRAMES * world * args.steps / elapsed, 1), "n_ref": N_REF,
                       "weights": "seeded synthetic (no weights ship with the reference)",
                       "parallelism": f"frames sharded by image, {world} rank(s), 1 per GPU" +
                                      (f", all_gather of the step's embeddings over "
                                       f"{'RCCL' if backend == 'nccl' else backend + ' (CPU rehearsal)'} + cross-rank cosine match, "
                                       f"overlapped with the next step's detector (side stream, consumed one step late)"
                                       if world > 1 else "")},
            "roofline": roof, "cpu_baseline": cpu, "arithmetic": arith, "other_configs": others,
        }
        emit_line(line)
    if multi:
        dist.destroy_process_group()


# ---------------------------------------------------------------------------------------------------------------
def run_c5(args):
    """BASELINE configs[4]: gallery rows sharded 125 k per rank, 10 k reference rows produced sharded (10 k / N per
    rank), one all_gather of the equal reference blocks, then the fused row-max cosine kernel on every rank's shard."""
    check_world(args, int(os.environ.get("WORLD_SIZE", "1")))
    world, rank, dev, dist, backend = init_dist()
    M, D = args.gallery_rows, 512
    nr_local = N_REF // world
    g = torch.Generator(device=dev).manual_seed(42 + rank)
    G = torch.randn((M, D), device=dev, generator=g)
    Rl = torch.randn((nr_local, D), device=dev, generator=g)
    ginv = S.row_inv_norm(G)

    def step():
        if dist is not None:
            from face_detection_and_recognition_amd import distributed as Dm
            if backend == "nccl":
                return Dm.sharded_cosine_filter(G, Rl, 0.3, lambda a, b, tau: S.cosine_filter(a, b, tau, ginv=ginv),
                                                equal_blocks=True)
            return Dm.sharded_cosine_filter(G.cpu(), Rl.cpu(), 0.3,
                                            lambda a, b, tau: S.cosine_filter(G, b.to(dev), tau, ginv=ginv),
                                            equal_blocks=True)
        return S.cosine_filter(G, Rl, 0.3, ginv=ginv)

    for _ in range(max(args.warmup, 1)):
        step()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    t0 = time.perf_counter()
    for k in range(args.steps):
        ev[k][0].record()
        best, arg, keep = step()
        ev[k][1].record()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    t1 = time.perf_counter()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"best": best, "arg": arg, "keep": keep})
    nr = nr_local * world
    elapsed, rows_all = reduce_time_and_count(t1 - t0, M * args.steps, world, dist, dev, backend)
    launch = launch_record(args, world, rank, dev, dist, backend, M * args.steps)
    if rank == 0:
        ms = sum(a.elapsed_time(b) for a, b in ev) / args.steps
        tf = 2.0 * M * nr * D / (ms * 1e-3) / 1e12
        line = {"metric": "pair-scores/sec, cosine filter gallery x reference x 512-d (fused row max, matrix never written)",
                "value": round(rows_all * nr / elapsed, 1), "unit": "pair-scores/s", "n_gpus": world, "steps": args.steps,
                "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True,
                "scaling": "weak", "vs_baseline": None, "dtype": DTYPE_LABEL, "data": "synthetic", "launch": launch,
                "config": {"workload": f"filter_faces_using_reference cosine mode: {M} gallery rows per GPU x {nr} reference "
                                       f"rows x {D}-d, reference produced sharded ({nr_local} rows per rank)",
                           "parallelism": f"gallery row-sharded over {world} rank(s)" +
                                          (f", one all_gather of the equal reference blocks over "
                                           f"{'RCCL' if backend == 'nccl' else backend + ' (CPU rehearsal)'}" if world > 1 else "")},
                "roofline": {"bound": "mfma", "kernel": "cosine_x6_kernel<4>", "achieved": round(tf, 1),
                             "peak": round(X6_PEAK_TF, 1), "unit": "TFLOP/s", "frac": round(tf / X6_PEAK_TF, 4),
                             "vs_fp32_mfma_peak": round(tf / MFMA_F32_PEAK_TFS, 4),
                             "traffic": None, "note": "step = (all_gather +) split of the gathered reference rows into bf16 planes + "
                                                      "cosine kernel (fp32 products as six bf16 MFMA products, csrc/split.h: peak = "
                                                      "2.5 PF / 6) + row-max finalisation, events on torch's current stream (the "
                                                      "launch stream); the fp32-MFMA kernel (cosine_tile_kernel) ran 117 TF/s"},
                "cpu_baseline": None}
        emit_line(line)
    if dist is not None:
        dist.destroy_process_group()


_LINE_FD = None


def emit_line(line):
    """The ONE JSON line of the run, written to the process's original stdout."""
    data = (json.dumps(line) + "\n").encode()
    if _LINE_FD is None:
        sys.stdout.write(data.decode())
        sys.stdout.flush()
    else:
        os.write(_LINE_FD, data)


def main():
    # Libraries write to stdout too (RCCL prints a version banner there when the process group comes up): everything but
    # the result line goes to stderr, so that stdout carries exactly one line.
    global _LINE_FD
    sys.stdout.flush()
    _LINE_FD = os.dup(1)
    os.dup2(2, 1)
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # defaults: 200 timed steps (~1.3 s of GPU time: long enough for a utilisation sampler to see it) after 10 warm-ups
    # (the c5 workload's step is ~60-90 ms: 20 / 3 there)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--workload", choices=["pipeline", "c5"], default="pipeline")
    ap.add_argument("--cpu-frames", type=int, default=256, help="frames in the bounded CPU-baseline sample")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--mfma", choices=["bf16x6", "fp32"], default="bf16x6",
                    help="matrix arithmetic of the Mobile-FaceNet Depth_Wise blocks: bf16x6 = fp32 operands split exactly into "
                         "three bf16 pieces (round-to-nearest cuts), six products, fp32 accumulation (csrc/split.h); "
                         "fp32 = every GEMM on the fp32 MFMA (rounds 1-3)")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="skip the short legs of BASELINE configs[2], [3], the batch-1024 embedder and the configs[4] shard that "
                         "fill `other_configs` (1 GPU only)")
    ap.add_argument("--no-fp32-leg", action="store_true", help="skip the short un-timed-region leg that re-measures the step "
                                                               "with --mfma fp32 for the `arithmetic` object")
    ap.add_argument("--overlap", type=int, nargs="?", const=1, default=2,
                    help="2 (default): software-pipelined steps on TWO streams (FacePipeline.step_overlapped, two_streams: the "
                         "detector of batch k + 1 runs beside embed + filter of batch k; every batch is finished inside the timed "
                         "region): 4.05 against 4.52 ms per step on one MI355X.  1: the same pipelining on one stream (4.51 ms: "
                         "the host round trip is already hidden).  0: every step self-contained")
    ap.add_argument("--box-px", type=float, default=W.BOX_PX,
                    help="synthetic detector's box size (model-input pixels); sets how candidates cluster in the NMS")
    ap.add_argument("--gallery-rows", type=int, default=125_000, help="c5: gallery rows per rank")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned (rank 0) as DIR/<name>.npy, float32 "
                         "or float64, at most 64 MB in all; the inputs are seeded, so runs with the same arguments compare")
    args = ap.parse_args()
    if args.steps is None:
        args.steps = 20 if args.workload == "c5" else 200
    if args.warmup is None:
        args.warmup = 3 if args.workload == "c5" else 10
    if os.environ.get("BENCH_STUB_STEP") == "1":
        run_stub(args)
    elif args.workload == "c5":
        run_c5(args)
    else:
        run_pipeline(args)


if __name__ == "__main__":
    main()
