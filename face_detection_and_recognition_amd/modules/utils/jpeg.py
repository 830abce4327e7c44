"""JPEG decode in front of the path: host Huffman + device reconstruction (csrc/jpeg.hip), byte-identical to what the
reference's cv2.imread returns (libjpeg-turbo's default decompressor; fde/modules/utils/inference.py:68-76,
fde/face_extraction/extract_faces_from_dataset.py:393-420).

    decode_jpeg(data, device)                 one frame  -> (H, W, 3) u8 BGR tensor on `device`
    decode_jpeg_batch(datas, device)          many frames: Huffman decoding on a thread pool (the C function drops the GIL),
                                              coefficient upload and the device kernels on the caller's stream
    entropy="device" (decode_jpeg / decode_jpeg_batch / imread_batch): the Huffman stage of sequential files runs on the
                                              device too (csrc/jpegdec.hip), one launch sequence per batch; files it does not take or
                                              leaves undecided go through the host path, bit-identical either way
    imread(path, device)                      cv2.imread for the device: JPEGs (sequential and progressive) through the above;
                                              what the decoder does not take (CMYK / arithmetic-coded JPEGs, PNG, ...) is
                                              decoded by Pillow on the host -- file I/O, not the hot path -- and uploaded

JpegUnsupported is raised by the first two for files outside csrc/jpeg.hip's scope (arithmetic-coded, lossless, 12-bit,
CMYK, sampling layouts other than 4:4:4 / 4:2:2 / 4:2:0).  All 1048 JPEG files of the reference's tree are inside it."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from ... import _lib as L

FP_ERR_UNSUPPORTED = -3
FP_ERR_INVALID_ARG = -1
DEVICE_SUB_BITS = 1024        # entropy="device": bits per subsequence (one lane each)
DEVICE_MAX_ROUNDS = 8         # entropy="device": synchronisation rounds before an image is left to the host path


class JpegUnsupported(L.FacepathError):
    pass


def parse(data):
    """JPEG bytes -> fp_jpeg_info (host only)."""
    info = L.FpJpegInfo()
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    rc = L.load().fp_jpeg_parse(buf, len(data), C.byref(info))
    if rc == FP_ERR_UNSUPPORTED:
        raise JpegUnsupported("a JPEG this decoder does not take (arithmetic-coded / lossless / 12-bit / CMYK / unusual sampling)")
    L.check(rc, "fp_jpeg_parse")
    return info, buf


def entropy_decode(data, pinned=False):
    """JPEG bytes -> (fp_jpeg_info, int16 coefficient tensor in host memory): the host half of the decode."""
    info, buf = parse(data)
    # (page-locking a buffer costs about a millisecond: only worth it for frames, not for face crops of a few KB)
    coefs = torch.empty((int(info.n_coefs),), dtype=torch.int16, pin_memory=pinned and info.n_coefs >= (1 << 19))
    L.check(L.load().fp_jpeg_entropy_decode(buf, len(data), C.byref(info), C.c_void_p(coefs.data_ptr())),
            "fp_jpeg_entropy_decode")
    return info, coefs


def reconstruct(info, coefs_dev, device, bgr=True, out=None):
    """The device half: coefficients (int16, on `device`) -> (H, W, 3) u8."""
    lib = L.load()
    ws_bytes = int(lib.fp_jpeg_workspace_bytes(C.byref(info)))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=device)
    if out is None:
        out = torch.empty((info.height, info.width, 3), dtype=torch.uint8, device=device)
    assert out.is_contiguous() and tuple(out.shape) == (info.height, info.width, 3) and out.dtype == torch.uint8
    L.check(lib.fp_jpeg_reconstruct(L.ptr(coefs_dev), C.byref(info), L.ptr(ws), ws_bytes, L.ptr(out), 1 if bgr else 0,
                                    L.current_stream(device)), "fp_jpeg_reconstruct")
    return out


def _check_entropy(entropy):
    if entropy not in ("host", "device"):
        raise ValueError(f"entropy must be 'host' or 'device', not {entropy!r}")


def device_entropy_decode(datas, device, sub_bits=None, max_rounds=None):
    """The Huffman stage of a batch on the device (fp_jpeg_entropy_decode_device).  Per file: (info, int16 device coefficients)
    when the device decoded it, FP_ERR_INVALID_ARG when it proved the file damaged (fp_jpeg_entropy_decode's status), None for
    the host path (not a sequential file the device takes, or left undecided by the device)."""
    lib = L.load()
    sub_bits = DEVICE_SUB_BITS if sub_bits is None else sub_bits
    max_rounds = DEVICE_MAX_ROUNDS if max_rounds is None else max_rounds
    out = [None] * len(datas)
    idx, infos, scans = [], [], []
    for i, d in enumerate(datas):
        info, scan = L.FpJpegInfo(), L.FpJpegScan()
        buf = (C.c_uint8 * max(1, len(d))).from_buffer_copy(d) if len(d) else (C.c_uint8 * 1)()
        if lib.fp_jpeg_scan_prepare(buf, len(d), C.byref(info), C.byref(scan)) == 0:
            idx.append(i)
            infos.append(info)
            scans.append(scan)
    if not idx:
        return out
    n = len(idx)
    file_off, coef_off, fo, co = (C.c_int64 * n)(), (C.c_int64 * n)(), 0, 0
    for j, i in enumerate(idx):
        file_off[j], coef_off[j] = fo, co
        fo += (len(datas[i]) + 15) // 16 * 16
        co += (int(scans[j].n_coefs) + 7) // 8 * 8
    files = torch.zeros((fo,), dtype=torch.uint8, pin_memory=True)
    fnp = files.numpy()
    for j, i in enumerate(idx):
        fnp[file_off[j]:file_off[j] + len(datas[i])] = np.frombuffer(datas[i], np.uint8)
    scan_arr = (L.FpJpegScan * n)(*scans)
    ws_bytes = int(lib.fp_jpeg_entropy_workspace_bytes(scan_arr, n, sub_bits, max_rounds))
    if ws_bytes == 0:
        raise L.FacepathError("fp_jpeg_entropy_workspace_bytes: invalid batch")
    files_dev = files.to(device, non_blocking=True)
    coefs = torch.empty((co,), dtype=torch.int16, device=device)
    status = torch.empty((n,), dtype=torch.int32, device=device)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=device)
    L.check(lib.fp_jpeg_entropy_decode_device(L.ptr(files_dev), scan_arr, file_off, n, L.ptr(coefs), coef_off, L.ptr(status),
                                              L.ptr(ws), ws_bytes, sub_bits, max_rounds, L.current_stream(device)),
            "fp_jpeg_entropy_decode_device")
    st = status.cpu().tolist()                  # (synchronises: the buffers above stay alive until the decode is done)
    for j, i in enumerate(idx):
        if st[j] == 0:
            out[i] = (infos[j], coefs[coef_off[j]:coef_off[j] + int(scans[j].n_coefs)])
        elif st[j] == FP_ERR_INVALID_ARG:
            out[i] = FP_ERR_INVALID_ARG
    return out


def decode_jpeg(data, device, bgr=True, entropy="host"):
    device = torch.device(device)
    _check_entropy(entropy)
    if device.type != "cuda":
        raise L.FacepathError("decode_jpeg reconstructs on a HIP device; there is no CPU path")
    if entropy == "device":
        return decode_jpeg_batch([data], device, bgr, entropy="device")[0]
    info, coefs = entropy_decode(data, pinned=True)
    return reconstruct(info, coefs.to(device, non_blocking=True), device, bgr)


def _host_entropy(d):
    try:
        return entropy_decode(d, pinned=True)
    except L.FacepathError as e:
        return e


def _device_batch(datas, device, bgr, threads, missing):
    """entropy="device" for a batch: per file a frame, or missing(i, exception) for a file the host path raises on."""
    dev = device_entropy_decode(datas, device)
    rest = [i for i, r in enumerate(dev) if r is None]
    host = {}
    if rest:
        with ThreadPoolExecutor(max_workers=max(1, min(threads, len(rest)))) as pool:
            host = dict(zip(rest, pool.map(lambda i: _host_entropy(datas[i]), rest)))
    frames = []
    for i, r in enumerate(dev):
        if r is None:
            r = host[i]
            if isinstance(r, Exception):
                frames.append(missing(i, r))
                continue
            frames.append(reconstruct(r[0], r[1].to(device, non_blocking=True), device, bgr))
        elif isinstance(r, int):
            try:
                L.check(r, "fp_jpeg_entropy_decode")          # what the host path raises for this file
            except L.FacepathError as e:
                frames.append(missing(i, e))
        else:
            frames.append(reconstruct(r[0], r[1], device, bgr))
    return frames


def _raise(i, e):
    raise e


def _unsupported_to_imread(i, e):
    if isinstance(e, JpegUnsupported):
        return None                              # imread_batch decodes it through imread's host fallback
    raise e


def decode_jpeg_batch(datas, device, bgr=True, threads=8, entropy="host"):
    """List of JPEG byte strings -> list of (H, W, 3) u8 tensors on `device` (sizes may differ).  entropy="device": the Huffman
    stage on the device for the sequential files it takes (one batch), the others through the host path; the first damaged or
    unsupported file in order raises what the host path raises."""
    device = torch.device(device)
    _check_entropy(entropy)
    if device.type != "cuda":
        raise L.FacepathError("decode_jpeg_batch reconstructs on a HIP device; there is no CPU path")
    if entropy == "device":
        return _device_batch(datas, device, bgr, threads, _raise)
    with ThreadPoolExecutor(max_workers=max(1, min(threads, len(datas)))) as pool:
        # in order, as each frame's Huffman decode finishes: its copy and reconstruction run under the decodes still going
        return [reconstruct(info, coefs.to(device, non_blocking=True), device, bgr)
                for info, coefs in pool.map(lambda d: entropy_decode(d, pinned=True), datas)]


def imread(path, device, bgr=True):
    """cv2.imread(path) as a device tensor: (H, W, 3) u8, BGR by default."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:2] == b"\xff\xd8":
        try:
            return decode_jpeg(data, device, bgr)
        except JpegUnsupported:
            pass
    import io
    from PIL import Image
    rgb = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    arr = np.ascontiguousarray(rgb[..., ::-1] if bgr else rgb)
    return torch.from_numpy(arr).to(device)


def imread_batch(paths, device, bgr=True, threads=8, entropy="host"):
    """cv2.imread over a list of files (the dataset driver reads its media this way,
    fde/face_extraction/extract_faces_from_dataset.py:393-420) -> (B, H, W, 3) u8 on `device` when every frame has the same size,
    else a list of (H, W, 3) tensors.  Baseline JPEGs: Huffman decoding on a thread pool, everything else of the decode on the
    device; other files through imread's host fallback."""
    device = torch.device(device)
    _check_entropy(entropy)
    datas = []
    for p in paths:
        with open(p, "rb") as f:
            datas.append(f.read())
    if entropy == "device":
        jpg = [i for i, d in enumerate(datas) if d[:2] == b"\xff\xd8"]
        frames = [None] * len(datas)
        dec = _device_batch([datas[i] for i in jpg], device, bgr, threads, _unsupported_to_imread)
        for i, f in zip(jpg, dec):
            frames[i] = f
        frames = [f if f is not None else imread(p, device, bgr) for f, p in zip(frames, paths)]
        if frames and all(f.shape == frames[0].shape for f in frames):
            return torch.stack(frames)
        return frames

    def host(d):
        if d[:2] == b"\xff\xd8":
            try:
                return entropy_decode(d, pinned=True)
            except JpegUnsupported:
                pass
        return None
    with ThreadPoolExecutor(max_workers=max(1, min(threads, len(datas)))) as pool:
        frames = [reconstruct(h[0], h[1].to(device, non_blocking=True), device, bgr) if h is not None else imread(p, device, bgr)
                  for h, p in zip(pool.map(host, datas), paths)]
    if frames and all(f.shape == frames[0].shape for f in frames):
        return torch.stack(frames)
    return frames
