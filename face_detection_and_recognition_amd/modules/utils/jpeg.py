"""JPEG decode in front of the path: host Huffman + device reconstruction (csrc/jpeg.hip), byte-identical to what the
reference's cv2.imread returns (libjpeg-turbo's default decompressor; fde/modules/utils/inference.py:68-76,
fde/face_extraction/extract_faces_from_dataset.py:393-420).

    decode_jpeg(data, device)                 one frame  -> (H, W, 3) u8 BGR tensor on `device`
    decode_jpeg_batch(datas, device)          many frames: Huffman decoding on a thread pool (the C function drops the GIL),
                                              coefficient upload and the device kernels on the caller's stream
    entropy="device" (decode_jpeg / decode_jpeg_batch / imread_batch): the Huffman stage of sequential files runs on the
                                              device too (csrc/jpegdec.hip), one launch sequence per batch; files it does not take or
                                              leaves undecided go through the host path, bit-identical either way
    decode_video_batch(datas, device)         the frames of a video (one size, one sampling) -> ONE (B, H, W, 3) tensor: the
                                              device half in one launch sequence per chunk of frames (csrc/jpegbatch.hip), no
                                              stacking copy; modules/utils/video.py reads and writes the Motion-JPEG containers.
                                              Sequential files without Huffman tables (MJPEG frames) decode with the Annex K.3
                                              tables, as libjpeg-turbo decodes them (all of the above)
    imread(path, device)                      cv2.imread for the device: JPEGs (sequential and progressive) through the above;
                                              what the decoder does not take (CMYK / arithmetic-coded JPEGs, PNG, ...) is
                                              decoded by Pillow on the host -- file I/O, not the hot path -- and uploaded
    orientation=True (all of the above)       the frame is turned upright by the file's EXIF Orientation tag (0x0112, read by
                                              fp_jpeg_exif_orientation on the host), as cv2.imread does: tags 2 .. 8 are applied in
                                              the colour kernel's addressing (csrc/jpegscale.hip), tags 5 .. 8 give a (W, H, 3)
                                              frame.  cv2 parity of this is pinned through Pillow's ImageOps.exif_transpose, which
                                              the host fallback applies too.  orientation=False: cv2's IMREAD_IGNORE_ORIENTATION
    reduce=2 / 4 / 8 (all of the above)       cv2's IMREAD_REDUCED_COLOR_2 / _4 / _8 = libjpeg's scale_denom: the frame comes out
                                              of 4 x 4 / 2 x 2 / 1 x 1 inverse DCTs at ceil(H / reduce) x ceil(W / reduce), no
                                              resize; byte-identical to Pillow's draft() decode.  The orientation is applied after
                                              scaling.  JPEGs only: a reduced PNG is a resize in cv2, which is not pinned here
                                              (ValueError).  reduce=1 on a file without a tag (or with tag 1) is the unchanged
                                              fp_jpeg_reconstruct call

    encode_jpeg_batch(images, ...)            JPEG ENCODE (csrc/jpegenc.hip): a list of (h, w, 3) u8 device images -> list of JPEG
                                              files (bytes), byte-identical to libjpeg-turbo's default compressor -- cv2.imwrite /
                                              Pillow's save(quality=q, subsampling=s) -- in one device call per batch
    encode_crops(frames, items, n, ...)       the same for the pipeline's crop records over its device frames, without cutting the
                                              crops out first
    imwrite(path, image, quality=95)          cv2.imwrite for one device image

JpegUnsupported is raised by the first two for files outside csrc/jpeg.hip's scope (arithmetic-coded, lossless, 12-bit,
CMYK, sampling layouts other than 4:4:4 / 4:2:2 / 4:2:0).  All 1048 JPEG files of the reference's tree are inside it."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from ... import _lib as L

FP_ERR_UNSUPPORTED = -3
FP_ERR_INVALID_ARG = -1
REDUCE = (1, 2, 4, 8)         # libjpeg's scale_denom values (cv2: IMREAD_REDUCED_COLOR_2 / _4 / _8)
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


def _check_reduce(reduce):
    if isinstance(reduce, bool) or reduce not in REDUCE:
        raise ValueError(f"reduce must be 1, 2, 4 or 8 (libjpeg's scale_denom), not {reduce!r}")


def exif_orientation(data):
    """The EXIF Orientation tag (1 .. 8) of a JPEG file's bytes (fp_jpeg_exif_orientation, host only); 1 for no tag, a value
    outside 1 .. 8 or a damaged segment."""
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data) if len(data) else (C.c_uint8 * 1)()
    return int(L.load().fp_jpeg_exif_orientation(buf, len(data)))


def scaled_size(info, reduce=1, orientation=1):
    """(rows, columns) of the frame reconstruct(info, ..., reduce, orientation) writes."""
    _check_reduce(reduce)
    h, w = C.c_int(), C.c_int()
    L.check(L.load().fp_jpeg_scaled_size(C.byref(info), reduce, int(orientation), C.byref(h), C.byref(w)), "fp_jpeg_scaled_size")
    return h.value, w.value


def reconstruct(info, coefs_dev, device, bgr=True, out=None, reduce=1, orientation=True):
    """The device half: coefficients (int16, on `device`) -> (H, W, 3) u8.  reduce = 2 / 4 / 8: libjpeg's scale_denom, a
    (ceil(H / reduce), ceil(W / reduce), 3) frame out of the reduced inverse DCTs.  orientation: there is no file here, so this
    function takes the TAG ITSELF, 1 .. 8 (True counts as 1, as does False); the frame is turned upright by it after scaling,
    tags 5 .. 8 give a (W', H', 3) frame.  reduce = 1 with tag 1 is fp_jpeg_reconstruct as before; everything else goes
    through fp_jpeg_reconstruct_scaled (csrc/jpegscale.hip)."""
    lib = L.load()
    _check_reduce(reduce)
    tag = int(orientation) or 1
    if not 1 <= tag <= 8:
        raise ValueError(f"orientation tag {orientation!r}: 1 .. 8")
    if reduce != 1 or tag != 1:
        oh, ow = scaled_size(info, reduce, tag)
        ws_bytes = int(lib.fp_jpeg_scaled_workspace_bytes(C.byref(info), reduce))
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=device)
        if out is None:
            out = torch.empty((oh, ow, 3), dtype=torch.uint8, device=device)
        assert out.is_contiguous() and tuple(out.shape) == (oh, ow, 3) and out.dtype == torch.uint8
        L.check(lib.fp_jpeg_reconstruct_scaled(L.ptr(coefs_dev), C.byref(info), reduce, tag, L.ptr(ws), ws_bytes, L.ptr(out),
                                               1 if bgr else 0, L.current_stream(device)), "fp_jpeg_reconstruct_scaled")
        return out
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
    the host path (not a sequential file the device takes, or left undecided by the device -- a file with 0xff fill bytes in
    front of a restart marker among them: the host decoder skips the fill bytes as libjpeg does)."""
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


def _tag(data, orientation):
    return exif_orientation(data) if orientation else 1


def decode_jpeg(data, device, bgr=True, entropy="host", reduce=1, orientation=True):
    """One JPEG file's bytes -> (H, W, 3) u8 on `device`.  reduce = 2 / 4 / 8: cv2's IMREAD_REDUCED_COLOR_2 / _4 / _8 (libjpeg's
    scale_denom).  orientation=True turns the frame upright by the file's EXIF Orientation tag, as cv2.imread does; False is
    cv2's IMREAD_IGNORE_ORIENTATION."""
    device = torch.device(device)
    _check_entropy(entropy)
    _check_reduce(reduce)
    if device.type != "cuda":
        raise L.FacepathError("decode_jpeg reconstructs on a HIP device; there is no CPU path")
    if entropy == "device":
        return decode_jpeg_batch([data], device, bgr, entropy="device", reduce=reduce, orientation=orientation)[0]
    info, coefs = entropy_decode(data, pinned=True)
    return reconstruct(info, coefs.to(device, non_blocking=True), device, bgr, reduce=reduce, orientation=_tag(data, orientation))


def _host_entropy(d):
    try:
        return entropy_decode(d, pinned=True)
    except L.FacepathError as e:
        return e


def _device_batch(datas, device, bgr, threads, missing, reduce=1, orientation=True):
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
            frames.append(reconstruct(r[0], r[1].to(device, non_blocking=True), device, bgr, reduce=reduce,
                                      orientation=_tag(datas[i], orientation)))
        elif isinstance(r, int):
            try:
                L.check(r, "fp_jpeg_entropy_decode")          # what the host path raises for this file
            except L.FacepathError as e:
                frames.append(missing(i, e))
        else:
            frames.append(reconstruct(r[0], r[1], device, bgr, reduce=reduce, orientation=_tag(datas[i], orientation)))
    return frames


def _raise(i, e):
    raise e


def _unsupported_to_imread(i, e):
    if isinstance(e, JpegUnsupported):
        return None                              # imread_batch decodes it through imread's host fallback
    raise e


def decode_jpeg_batch(datas, device, bgr=True, threads=8, entropy="host", reduce=1, orientation=True):
    """List of JPEG byte strings -> list of (H, W, 3) u8 tensors on `device` (sizes may differ).  entropy="device": the Huffman
    stage on the device for the sequential files it takes (one batch), the others through the host path; the first damaged or
    unsupported file in order raises what the host path raises.  reduce, orientation: as decode_jpeg, per file."""
    device = torch.device(device)
    _check_entropy(entropy)
    _check_reduce(reduce)
    if device.type != "cuda":
        raise L.FacepathError("decode_jpeg_batch reconstructs on a HIP device; there is no CPU path")
    if entropy == "device":
        return _device_batch(datas, device, bgr, threads, _raise, reduce, orientation)
    with ThreadPoolExecutor(max_workers=max(1, min(threads, len(datas)))) as pool:
        # in order, as each frame's Huffman decode finishes: its copy and reconstruction run under the decodes still going
        return [reconstruct(info, coefs.to(device, non_blocking=True), device, bgr, reduce=reduce, orientation=_tag(d, orientation))
                for d, (info, coefs) in zip(datas, pool.map(lambda d: entropy_decode(d, pinned=True), datas))]


def _pillow_decode(data, reduce, orientation):
    """imread's host fallback (CMYK / arithmetic-coded JPEGs, other formats) -> (H, W, 3) u8 RGB array.  reduce > 1: libjpeg's
    own scaled decode through draft() for a JPEG; cv2 RESIZES other formats, which cannot be pinned here: ValueError."""
    import io
    from PIL import Image, ImageOps
    im = Image.open(io.BytesIO(data))
    if reduce > 1:
        if im.format != "JPEG":
            raise ValueError(f"reduce={reduce} on a {im.format} file: only JPEGs are decoded at a reduced size")
        w, h = im.size
        im.draft(None, (max(1, w // reduce), max(1, h // reduce)))
    if orientation:
        im = ImageOps.exif_transpose(im)
    return np.asarray(im.convert("RGB"))


def imread(path, device, bgr=True, reduce=1, orientation=True):
    """cv2.imread(path) as a device tensor: (H, W, 3) u8, BGR by default, upright by the EXIF Orientation tag unless
    orientation=False (cv2's IMREAD_IGNORE_ORIENTATION); reduce = 2 / 4 / 8: IMREAD_REDUCED_COLOR_2 / _4 / _8 (JPEGs only)."""
    _check_reduce(reduce)
    with open(path, "rb") as f:
        data = f.read()
    if data[:2] == b"\xff\xd8":
        try:
            return decode_jpeg(data, device, bgr, reduce=reduce, orientation=orientation)
        except JpegUnsupported:
            pass
    rgb = _pillow_decode(data, reduce, orientation)
    arr = np.ascontiguousarray(rgb[..., ::-1] if bgr else rgb)
    return torch.from_numpy(arr).to(device)


def imread_batch(paths, device, bgr=True, threads=8, entropy="host", reduce=1, orientation=True):
    """cv2.imread over a list of files (the dataset driver reads its media this way,
    fde/face_extraction/extract_faces_from_dataset.py:393-420) -> (B, H, W, 3) u8 on `device` when every frame has the same size,
    else a list of (H, W, 3) tensors.  Baseline JPEGs: Huffman decoding on a thread pool, everything else of the decode on the
    device; other files through imread's host fallback.  reduce, orientation: as imread, per file; the frames are stacked when
    their OUTPUT shapes agree (a portrait file with tag 6 among landscape ones gives a list)."""
    device = torch.device(device)
    _check_entropy(entropy)
    _check_reduce(reduce)
    datas = []
    for p in paths:
        with open(p, "rb") as f:
            datas.append(f.read())
    if entropy == "device":
        jpg = [i for i, d in enumerate(datas) if d[:2] == b"\xff\xd8"]
        frames = [None] * len(datas)
        dec = _device_batch([datas[i] for i in jpg], device, bgr, threads, _unsupported_to_imread, reduce, orientation)
        for i, f in zip(jpg, dec):
            frames[i] = f
        frames = [f if f is not None else imread(p, device, bgr, reduce, orientation) for f, p in zip(frames, paths)]
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
        frames = [reconstruct(h[0], h[1].to(device, non_blocking=True), device, bgr, reduce=reduce, orientation=_tag(d, orientation))
                  if h is not None else imread(p, device, bgr, reduce, orientation)
                  for h, p, d in zip(pool.map(host, datas), paths, datas)]
    if frames and all(f.shape == frames[0].shape for f in frames):
        return torch.stack(frames)
    return frames


# ---- frames of one geometry: a video ---------------------------------------------------------------------------------

VIDEO_WS_BYTES = 64 << 20     # decode_video_batch: cap of one fp_jpeg_reconstruct_batch call's workspace (the sample planes of its
                              # frames: 0.88 MB each at 576 x 1024 4:2:0, so 75 frames a call); a larger batch goes in chunks
SAME_SIZE = "the frames of a video share one size"


def _geometry(info):
    return (info.width, info.height, info.ncomp, tuple(info.hs), tuple(info.vs))


def reconstruct_batch(info, coefs_dev, coef_off, quant, device, out, bgr=True):
    """The device half for len(coef_off) frames of info's geometry: fp_jpeg_reconstruct_batch.  coefs_dev: int16 on `device`;
    coef_off: int64 elements into it, one per frame; quant: (n, 3, 64) uint16 -- both host numpy arrays, uploaded together in
    one small copy.  out: contiguous (n, H, W, 3) u8 on `device`, written in place."""
    lib = L.load()
    n = len(coef_off)
    assert out.is_contiguous() and tuple(out.shape) == (n, info.height, info.width, 3) and out.dtype == torch.uint8
    # (pinned and asynchronous: a pageable copy would make the host wait for the coefficient copy queued in front of it, and
    # with it the Huffman decoding of the next chunk)
    side_host = torch.empty((n * 8 + n * 384,), dtype=torch.uint8, pin_memory=True)
    side = side_host.numpy()
    side[:n * 8] = np.ascontiguousarray(coef_off, dtype=np.int64).view(np.uint8)
    side[n * 8:] = np.ascontiguousarray(quant, dtype=np.uint16).reshape(-1).view(np.uint8)
    side_dev = side_host.to(device, non_blocking=True)
    ws_bytes = int(lib.fp_jpeg_batch_workspace_bytes(C.byref(info), n))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=device)
    L.check(lib.fp_jpeg_reconstruct_batch(L.ptr(coefs_dev), side_dev.data_ptr(), side_dev.data_ptr() + n * 8, C.byref(info), n,
                                          L.ptr(ws), ws_bytes, L.ptr(out), 1 if bgr else 0, L.current_stream(device)),
            "fp_jpeg_reconstruct_batch")
    return out


def _quant_rows(infos):
    return np.stack([np.frombuffer(i, dtype=np.uint16, count=192, offset=L.FpJpegInfo.quant.offset) for i in infos]).reshape(-1, 3, 64)


def _host_submit(datas, info0, pool):
    """Queues a chunk on the pool: every frame's headers are parsed and its scans Huffman-decoded into its slice of ONE pinned
    arena.  The file's bytes go to the C functions as they are (no copy).  -> (arena, futures of (status, function, info))."""
    lib = L.load()
    nc, geo = int(info0.n_coefs), _geometry(info0)
    arena = torch.empty((len(datas) * nc,), dtype=torch.int16, pin_memory=True)

    def one(j):
        base = arena.data_ptr()                       # (the closure holds the arena: it lives as long as a task may write to it)
        d = datas[j]
        info = L.FpJpegInfo()
        rc = lib.fp_jpeg_parse(d, len(d), C.byref(info))
        if rc:
            return rc, "fp_jpeg_parse", None
        if _geometry(info) != geo:
            return None, None, None
        return lib.fp_jpeg_entropy_decode(d, len(d), C.byref(info), C.c_void_p(base + 2 * j * nc)), "fp_jpeg_entropy_decode", info
    return arena, [pool.submit(one, j) for j in range(len(datas))]


def _host_finish(job, device):
    """Waits for a chunk queued by _host_submit -- in order: the first frame that is damaged, unsupported or of another
    geometry raises, as decode_jpeg_batch would --, then one host-to-device copy -> (device arena, the frames' infos)."""
    arena, futures = job
    infos = []
    for f in futures:
        rc, what, info = f.result()
        if rc is None:
            raise ValueError(SAME_SIZE)
        if rc == FP_ERR_UNSUPPORTED and what == "fp_jpeg_parse":
            raise JpegUnsupported("a JPEG this decoder does not take (arithmetic-coded / lossless / 12-bit / CMYK / unusual sampling)")
        L.check(rc, what)
        infos.append(info)
    return arena.to(device, non_blocking=True), infos


def _spans(n, step):
    return [(s, min(n, s + step)) for s in range(0, n, step)]


def _video_host(datas, info0, device, bgr, out, step, pool):
    """entropy="host": chunk after chunk; the pool stays busy, because the next two chunks are queued before this one is
    waited for: their Huffman decoding runs under this chunk's copy and kernels, which are asynchronous."""
    nc = int(info0.n_coefs)
    spans, jobs = _spans(len(datas), step), {}
    for k, (s, e) in enumerate(spans):
        for a in range(k, min(len(spans), k + 3)):
            if a not in jobs:
                jobs[a] = _host_submit(datas[spans[a][0]:spans[a][1]], info0, pool)
        coefs, infos = _host_finish(jobs.pop(k), device)
        reconstruct_batch(info0, coefs, np.arange(e - s, dtype=np.int64) * nc, _quant_rows(infos), device, out[s:e], bgr)


def _video_device(datas, info0, device, bgr, out, step, pool):
    """entropy="device": device_entropy_decode over the whole batch, as decode_jpeg_batch runs it (its fixed costs and its
    synchronisation once); the frames it leaves undecided are Huffman-decoded on the host into a second arena.  Reconstruction
    in chunks under the workspace cap; a chunk whose frames lie in both arenas is cut where the arena changes, so that every
    fp_jpeg_reconstruct_batch call addresses one allocation."""
    dev = device_entropy_decode(datas, device)
    rest = [j for j, r in enumerate(dev) if r is None]
    job = _host_submit([datas[j] for j in rest], info0, pool) if rest else None
    geo, nc = _geometry(info0), int(info0.n_coefs)
    bases = {}                                        # "device": the decoder's arena, "host": the second one
    arena, offs, infos = [None] * len(datas), np.zeros(len(datas), np.int64), [None] * len(datas)
    for j, r in enumerate(dev):                       # in order, with the host's frames: the first bad frame raises
        if isinstance(r, int):
            L.check(r, "fp_jpeg_entropy_decode")      # what the host path raises for this file
        elif r is not None:
            if _geometry(r[0]) != geo:
                raise ValueError(SAME_SIZE)
            bases.setdefault("device", r[1]._base if r[1]._base is not None else r[1])     # r[1] is a view of the arena
            infos[j], arena[j], offs[j] = r[0], "device", r[1].storage_offset()
        elif job is not None:                         # the host's frames are waited for at the first of them
            host, host_infos = _host_finish(job, device)
            job = None
            bases["host"] = host
            for k, i in enumerate(rest):
                infos[i], arena[i], offs[i] = host_infos[k], "host", k * nc
    quant = _quant_rows(infos)
    for s, e in _spans(len(datas), step):
        a = s
        while a < e:
            b = a + 1
            while b < e and arena[b] == arena[a]:
                b += 1
            reconstruct_batch(info0, bases[arena[a]], offs[a:b], quant[a:b], device, out[a:b], bgr)
            a = b


def decode_video_batch(datas, device, bgr=True, threads=8, entropy="host", reduce=1, out=None, max_ws_bytes=None):
    """The frames of a video -- JPEG byte strings that share width, height, components and sampling -> ONE (B, H, W, 3) u8 tensor
    on `device`, reconstructed by fp_jpeg_reconstruct_batch (csrc/jpegbatch.hip): one launch sequence per chunk of frames and no
    stacking copy, byte-identical to decode_jpeg(d, orientation=False) of each frame.  The headers are parsed on the thread pool
    (the first frame's in front of it: it sizes the arena); a frame that disagrees with the first raises
    ValueError("the frames of a video share one size").  entropy="host": chunk by chunk, the Huffman decoding on the pool into
    one pinned arena per chunk, one copy to the device each.  entropy="device": device_entropy_decode over the batch, the frames
    it leaves undecided through the host path.  The reconstruction is cut into chunks whose workspace stays under max_ws_bytes
    (VIDEO_WS_BYTES = 64 MiB by default; a single frame over the cap goes alone).  The first damaged or unsupported frame in
    order raises what decode_jpeg_batch raises for it.  reduce = 2 / 4 / 8: frame by frame through decode_jpeg_batch, stacked
    (there is no batched kernel for the reduced sizes).  No EXIF orientation: a video's frames are taken as stored.  out: a
    (B, H', W', 3) u8 tensor to fill."""
    device = torch.device(device)
    _check_entropy(entropy)
    _check_reduce(reduce)
    if device.type != "cuda":
        raise L.FacepathError("decode_video_batch reconstructs on a HIP device; there is no CPU path")
    datas = [d if isinstance(d, bytes) else bytes(d) for d in datas]
    if not datas:
        raise ValueError("decode_video_batch: no frames")
    cap = VIDEO_WS_BYTES if max_ws_bytes is None else int(max_ws_bytes)
    if cap < 1:
        raise ValueError(f"max_ws_bytes must be positive, not {max_ws_bytes!r}")
    info0 = parse(datas[0])[0]
    oh, ow = scaled_size(info0, reduce, 1)
    if out is None:
        out = torch.empty((len(datas), oh, ow, 3), dtype=torch.uint8, device=device)
    if not (out.is_contiguous() and tuple(out.shape) == (len(datas), oh, ow, 3) and out.dtype == torch.uint8 and out.device == device):
        raise ValueError(f"out must be a contiguous ({len(datas)}, {oh}, {ow}, 3) uint8 tensor on {device}")
    if reduce != 1:
        frames = decode_jpeg_batch(datas, device, bgr, threads, entropy, reduce, orientation=False)
        if any(f.shape != out.shape[1:] for f in frames):
            raise ValueError(SAME_SIZE)
        for i, f in enumerate(frames):
            out[i].copy_(f)
        return out
    step = max(1, cap // max(1, int(L.load().fp_jpeg_workspace_bytes(C.byref(info0)))))
    with ThreadPoolExecutor(max_workers=max(1, min(threads, len(datas)))) as pool:
        (_video_host if entropy == "host" else _video_device)(datas, info0, device, bgr, out, step, pool)
    return out


# ---- encode ----------------------------------------------------------------------------------------------------------

_SUBSAMPLING = {"4:4:4": L.JPEG_444, "4:2:2": L.JPEG_422, "4:2:0": L.JPEG_420,
                L.JPEG_444: L.JPEG_444, L.JPEG_422: L.JPEG_422, L.JPEG_420: L.JPEG_420}
_headers = {}


def _subsampling(s):
    if s not in _SUBSAMPLING:
        raise JpegUnsupported(f"subsampling {s!r}: the encoder takes '4:4:4', '4:2:2' or '4:2:0' (or Pillow's 0, 1, 2)")
    return _SUBSAMPLING[s]


def encode_headers(w, h, quality=95, subsampling="4:2:0"):
    """The headers of a w x h file (SOI .. SOS, fp_jpeg_encode_headers): they depend on nothing else."""
    key = (w, h, quality, _subsampling(subsampling))
    hdr = _headers.get(key)
    if hdr is None:
        buf = (C.c_uint8 * L.JPEG_ENC_HEADER_BYTES)()
        rc = L.load().fp_jpeg_encode_headers(w, h, quality, key[3], buf, len(buf))
        if rc < 0:
            L.check(rc, "fp_jpeg_encode_headers")
        hdr = bytes(buf[:rc])
        if len(_headers) < 4096:
            _headers[key] = hdr
    return hdr


def _encode_items(src, items, quality, subsampling, bgr, emulate=False):
    """fp_jpeg_enc_item list over the u8 buffer `src` (a device tensor; a host numpy array for emulate=True) -> files."""
    lib = L.load()
    sub = _subsampling(subsampling)
    n = len(items)
    if n == 0:
        return []
    if not isinstance(quality, int) or not 1 <= quality <= 100:
        raise L.FacepathError(f"quality {quality!r}: must be an int in 1 .. 100")
    arr = (L.FpJpegEncItem * n)(*items)
    ws_bytes, out_bytes = C.c_size_t(), C.c_size_t()
    rc = lib.fp_jpeg_encode_workspace_bytes(arr, n, sub, C.byref(ws_bytes), C.byref(out_bytes))
    if rc == FP_ERR_UNSUPPORTED:
        raise JpegUnsupported("a crop the encoder does not take (a side over 65535, or too many blocks in the batch)")
    L.check(rc, "fp_jpeg_encode_workspace_bytes")
    if emulate:
        out = np.empty((out_bytes.value,), np.uint8)
        offs = (C.c_int64 * (n + 1))()
        L.check(lib.fp_jpeg_encode_emulate(src.ctypes.data, arr, n, quality, sub, 1 if bgr else 0, out.ctypes.data,
                                           out_bytes.value, offs), "fp_jpeg_encode_emulate")
        offs = list(offs)
        data = out[:offs[n]].tobytes()
    else:
        device = src.device
        ws = torch.empty((ws_bytes.value,), dtype=torch.uint8, device=device)
        out = torch.empty((out_bytes.value,), dtype=torch.uint8, device=device)
        offs_dev = torch.empty((n + 1,), dtype=torch.int64, device=device)
        L.check(lib.fp_jpeg_encode_device(L.ptr(src), arr, n, quality, sub, 1 if bgr else 0, L.ptr(ws), ws_bytes.value,
                                          L.ptr(out), out_bytes.value, L.ptr(offs_dev), L.current_stream(device)),
                "fp_jpeg_encode_device")
        offs = offs_dev.cpu().tolist()                      # (synchronises)
        data = out[:offs[n]].cpu().numpy().tobytes()        # one copy of the batch's compressed bytes
    files = []
    for i, it in enumerate(items):
        w = min(it.x1, it.src_w) - max(it.x0, 0)
        h = min(it.y1, it.src_h) - max(it.y0, 0)
        files.append(encode_headers(w, h, quality, sub) + data[offs[i]:offs[i + 1]] + b"\xff\xd9")
    return files


def encode_jpeg_batch(images, quality=95, subsampling="4:2:0", bgr=True):
    """List of (h, w, 3) u8 tensors on one HIP device (BGR, cv2's order, unless bgr=False) -> list of JPEG files (bytes), one
    device call for the batch.  Each file equals cv2.imwrite's (libjpeg-turbo, quality 95, 4:2:0 by default) byte for byte."""
    if not images:
        return []
    device = images[0].device
    if device.type != "cuda":
        raise L.FacepathError("encode_jpeg_batch encodes on a HIP device; there is no CPU path")
    items, flat, off = [], [], 0
    for im in images:
        if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or im.device != device:
            raise L.FacepathError("encode_jpeg_batch takes (h, w, 3) uint8 tensors on one device")
        h, w = int(im.shape[0]), int(im.shape[1])
        if h < 1 or w < 1:
            raise L.FacepathError(f"encode_jpeg_batch: an empty image ({h} x {w})")
        items.append(L.FpJpegEncItem(off, h, w, 0, 0, w, h))
        flat.append(im.reshape(-1))
        off += h * w * 3
    src = torch.cat(flat) if len(flat) > 1 else flat[0].contiguous()
    return _encode_items(src, items, quality, subsampling, bgr)


def crop_items(frames, items, n):
    """The pipeline's crop records (fp_resize_item rows from fp_dets_to_crops, items[:n]) over frames (B, H, W, 3) or a
    RaggedFrames -> fp_jpeg_enc_item list; None for a crop that is empty after the clamp (the reference's slice of it is
    empty)."""
    from ...frames import frame_layout
    geo = frame_layout(frames)
    rows = items[:n].cpu().tolist() if n else []
    out = []
    for src_image, sx, sy, sw, sh, *_ in rows:
        if not 0 <= src_image < len(geo):
            raise L.FacepathError(f"crop record of frame {src_image} outside the batch of {len(geo)}")
        off, H, W = geo[src_image]
        it = L.FpJpegEncItem(off, H, W, sx, sy, sx + sw, sy + sh)
        empty = min(it.x1, W) <= max(it.x0, 0) or min(it.y1, H) <= max(it.y0, 0)
        out.append(None if empty else it)
    return out


def encode_crops(frames, items, n, quality=95, subsampling="4:2:0", bgr=True):
    """The first n crop records of a FacePipeline step (res["items"]) over its device frames (B, H, W, 3) u8 or RaggedFrames
    -> one JPEG file per face (bytes; None for a crop that is empty after the clamp), encoded straight from the frames in one
    device call (a ragged batch: the items address its packed buffer through the frames' descriptors)."""
    from ...frames import frame_bytes
    if isinstance(frames, torch.Tensor) and (frames.device.type != "cuda" or frames.dtype != torch.uint8 or frames.dim() != 4
                                             or not frames.is_contiguous()):
        raise L.FacepathError("encode_crops takes contiguous (B, H, W, 3) uint8 frames on a HIP device")
    recs = crop_items(frames, items, n)
    take = [it for it in recs if it is not None]
    files = iter(_encode_items(frame_bytes(frames), take, quality, subsampling, bgr))
    return [None if it is None else next(files) for it in recs]


def imwrite(path, image, quality=95, bgr=True):
    """cv2.imwrite(path, image) with cv2's default JPEG settings (quality 95, 4:2:0) for one (h, w, 3) u8 device image
    (a numpy array is uploaded to the current HIP device).  Returns True, as cv2.imwrite does."""
    if isinstance(image, np.ndarray):
        image = torch.from_numpy(np.ascontiguousarray(image)).to(torch.device("cuda", torch.cuda.current_device()))
    data = encode_jpeg_batch([image], quality=quality, bgr=bgr)[0]
    with open(path, "wb") as f:
        f.write(data)
    return True


def encode_jpeg_batch_emulate(images, quality=95, subsampling="4:2:0", bgr=True):
    """encode_jpeg_batch on host numpy images through fp_jpeg_encode_emulate: the device's phases run serially on the CPU
    (tests and debugging; the same bytes)."""
    items, flat, off = [], [], 0
    for im in images:
        im = np.ascontiguousarray(im, dtype=np.uint8)
        if im.ndim != 3 or im.shape[2] != 3:
            raise L.FacepathError("encode_jpeg_batch_emulate takes (h, w, 3) uint8 arrays")
        h, w = im.shape[:2]
        items.append(L.FpJpegEncItem(off, h, w, 0, 0, w, h))
        flat.append(im.reshape(-1))
        off += im.size
    if not items:
        return []
    return _encode_items(np.concatenate(flat), items, quality, subsampling, bgr, emulate=True)
