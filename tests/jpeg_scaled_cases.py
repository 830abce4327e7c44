"""Cases and a numpy restatement for the reduced-size, orientation-aware JPEG decode (csrc/jpegscale.hip).  TEST SUPPORT ONLY.

`scaled_ycc` / `scaled_rgb` restate what libjpeg-turbo does after the entropy decoder at scale_denom = s (m = 8 / s), from the
library's published procedure -- jdmaster.c (output size, per-component DCT_scaled_size: chroma is scaled up in the IDCT rather
than by upsampling where the sampling factors allow), jidctred.c (4 x 4, 2 x 2, 1 x 1 transforms; CONST_BITS 13, PASS1_BITS 2),
jdsample.c (fancy upsampling only for min_DCT_scaled_size > 1 and a plane more than 2 samples wide), jdcolor.c -- in numpy,
from the product's host-half coefficients.  The tests compare it, and the product, with Pillow's draft() decode: Pillow is the
judge, this text is not."""
import ctypes
import io

import numpy as np

from face_detection_and_recognition_amd import _lib as L
from oracle import jpeg_ref

SCALES = (2, 4, 8)
SIZES = ((8, 8), (16, 16), (17, 9), (67, 45), (2, 5), (4, 3), (40, 24), (250, 131))     # (w, h)


def _smooth(rng, w, h):
    return np.clip(np.cumsum(np.cumsum(rng.normal(0, 3, (h, w, 3)), 0), 1) + 128, 0, 255).astype(np.uint8)


def _noise(rng, w, h):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def encode(img, gray=False, exif=None, **kw):
    from PIL import Image
    b = io.BytesIO()
    if exif is not None:
        kw["exif"] = exif
    Image.fromarray(img[..., 0] if gray else img).save(b, "JPEG", **kw)
    return b.getvalue()


def case_list():
    """[(name, w, h, jpeg bytes)]: smooth images at quality 30 and 92, uniform noise at quality 100 (every coefficient position,
    the clamp); subsampling 0 / 1 / 2 and grayscale; sequential and progressive coding; the sizes of SIZES.  Built once (seeded)."""
    global _CASES
    if _CASES is None:
        rng = np.random.default_rng(20)
        out = []
        for (w, h) in SIZES:
            for sub in (0, 1, 2, "gray"):
                for q, prog, make in ((30, False, _smooth), (92, True, _smooth), (100, False, _noise), (100, True, _noise)):
                    if (q, prog) == (100, True) and (w, h) not in ((17, 9), (40, 24)):
                        continue                                  # progressive noise: two sizes are enough
                    kw = dict(quality=q, progressive=prog)
                    if sub == "gray":
                        data = encode(make(rng, w, h), gray=True, **kw)
                    else:
                        data = encode(make(rng, w, h), subsampling=sub, **kw)
                    out.append((f"{w}x{h}-sub{sub}-q{q}-{'prog' if prog else 'seq'}", w, h, data))
        _CASES = out
    return _CASES


_CASES = None


def host_decode(data):
    """JPEG bytes -> (fp_jpeg_info, int16 coefficients) through the product's host half."""
    lib = L.load()
    info = L.FpJpegInfo()
    buf = (ctypes.c_uint8 * len(data)).from_buffer_copy(data)
    assert lib.fp_jpeg_parse(buf, len(data), ctypes.byref(info)) == 0
    coefs = np.zeros(int(info.n_coefs), np.int16)
    assert lib.fp_jpeg_entropy_decode(buf, len(data), ctypes.byref(info), coefs.ctypes.data_as(ctypes.c_void_p)) == 0
    return info, coefs


def exif_orientation(data):
    buf = (ctypes.c_uint8 * max(1, len(data))).from_buffer_copy(data) if len(data) else (ctypes.c_uint8 * 1)()
    return L.load().fp_jpeg_exif_orientation(buf, len(data))


def emulate(info, coefs, s, tag=1, bgr=False):
    """fp_jpeg_reconstruct_scaled_emulate -> (H', W', 3) u8 (transposed sizes for tags 5 .. 8)."""
    lib = L.load()
    h, w = ctypes.c_int(), ctypes.c_int()
    assert lib.fp_jpeg_scaled_size(ctypes.byref(info), s, tag, ctypes.byref(h), ctypes.byref(w)) == 0
    nws = int(lib.fp_jpeg_scaled_workspace_bytes(ctypes.byref(info), s))
    assert nws > 0
    ws = np.zeros(nws, np.uint8)
    out = np.zeros((h.value, w.value, 3), np.uint8)
    rc = lib.fp_jpeg_reconstruct_scaled_emulate(coefs.ctypes.data_as(ctypes.c_void_p), ctypes.byref(info), s, tag,
                                                ws.ctypes.data_as(ctypes.c_void_p), nws, out.ctypes.data_as(ctypes.c_void_p), 1 if bgr else 0)
    assert rc == 0, rc
    return out


# ---- numpy restatement -----------------------------------------------------------------------------------------------

def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _idct4(v, shift):
    """jidctred.c jpeg_idct_4x4, one pass along the last axis of v (int64 [..., 8]) -> [..., 4]."""
    i0, i1, i2, i3, i5, i6, i7 = (v[..., k] for k in (0, 1, 2, 3, 5, 6, 7))
    t0 = i0 << 14
    t2 = i2 * 15137 - i6 * 6270
    a, b = t0 + t2, t0 - t2
    o0 = -i7 * 1730 + i5 * 11893 - i3 * 17799 + i1 * 8697
    o2 = -i7 * 4176 - i5 * 4926 + i3 * 7373 + i1 * 20995
    return _descale(np.stack([a + o2, b + o0, b - o0, a - o2], -1), shift)


def _idct2(v, shift):
    """jidctred.c jpeg_idct_2x2, one pass along the last axis -> [..., 2]."""
    i0, i1, i3, i5, i7 = (v[..., k] for k in (0, 1, 3, 5, 7))
    t = i0 << 15
    o = -i7 * 5906 + i5 * 6967 - i3 * 10426 + i1 * 29692
    return _descale(np.stack([t + o, t - o], -1), shift)


def _plane(info, coefs, c, ss):
    """Component c at ss x ss samples per block -> u8 plane, padded to whole blocks."""
    bw, bh = info.blocks_w[c], info.blocks_h[c]
    q = np.array(info.quant[c][:], np.int64).reshape(8, 8)
    blk = coefs[info.coef_off[c]: info.coef_off[c] + bw * bh * 64].astype(np.int64).reshape(bh, bw, 8, 8) * q
    if ss == 8:
        px = jpeg_ref._idct8(jpeg_ref._idct8(blk.swapaxes(-1, -2), 11).swapaxes(-1, -2), 18)
    elif ss == 4:
        px = _idct4(_idct4(blk.swapaxes(-1, -2), 12).swapaxes(-1, -2), 19)           # columns (per column: 4 rows out), then rows
    elif ss == 2:
        px = _idct2(_idct2(blk.swapaxes(-1, -2), 13).swapaxes(-1, -2), 20)
    else:
        px = ((blk[..., :1, :1] + 4) >> 3)
    px = np.clip(px + 128, 0, 255).astype(np.uint8)
    return px.transpose(0, 2, 1, 3).reshape(bh * ss, bw * ss)


def scaled_ycc(info, coefs, s):
    """-> (H', W', ncomp) u8: the Y (Cb, Cr) samples libjpeg-turbo hands to its colour converter at scale_denom = s."""
    m = 8 // s
    W, H = info.width, info.height
    ow, oh = -(-W // s), -(-H // s)
    nc = info.ncomp
    hmax, vmax = (info.hs[0], info.vs[0]) if nc == 3 else (1, 1)
    planes = []
    for c in range(nc):
        hc, vc = (info.hs[c], info.vs[c]) if nc == 3 else (1, 1)
        ss = m
        while ss < 8 and (hmax * m) % (hc * ss * 2) == 0 and (vmax * m) % (vc * ss * 2) == 0:
            ss *= 2
        pw, ph = -(-W * hc * ss // (hmax * 8)), -(-H * vc * ss // (vmax * 8))
        p = _plane(info, coefs, c, ss)[:ph, :pw]
        hx, vx = (hmax * m) // (hc * ss), (vmax * m) // (vc * ss)
        if hx == 2:
            if m > 1 and pw > 2:
                p = jpeg_ref._h2v2_fancy(p) if vx == 2 else jpeg_ref._h2v1_fancy(p)
            else:
                p = np.repeat(np.repeat(p, vx, axis=0), 2, axis=1)
        else:
            assert hx == 1 and vx == 1
        planes.append(np.asarray(p)[:oh, :ow].astype(np.uint8))
    return np.stack(planes, axis=2)


def ycc_to_rgb(ycc):
    y = ycc[..., 0].astype(np.int32)
    if ycc.shape[2] == 1:
        return np.repeat(y[..., None], 3, axis=2).astype(np.uint8)
    cb, cr = ycc[..., 1].astype(np.int32) - 128, ycc[..., 2].astype(np.int32) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def scaled_rgb(info, coefs, s):
    return ycc_to_rgb(scaled_ycc(info, coefs, s))


def orient(a, tag):
    """The orientation table of the decoder on an (H', W', C) array: out[y][x] = in[...]."""
    if tag in (2, 3, 7, 8):
        a = a[:, ::-1]                 # columns W' - 1 - c
    if tag in (3, 4, 6, 7):
        a = a[::-1]                    # rows H' - 1 - r
    if tag >= 5:
        a = a.transpose(1, 0, 2)       # out[y][x] = in'[x][y]
    return np.ascontiguousarray(a)


def pil_draft(data, s, mode="RGB"):
    """Pillow / libjpeg-turbo at scale 1 / s: draft(mode, (w // s, h // s)), then the decode.  Returns (array, im.size)."""
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    w, h = im.size
    im.draft("L" if im.mode == "L" else mode, (w // s, h // s))       # (a gray file stays gray: one plane)
    size = im.size
    a = np.asarray(im, dtype=np.uint8)
    if a.ndim == 2:
        a = a[..., None]
    return a, size


def exif_bytes(tag, big_endian=False):
    """A minimal Exif APP1 payload (what Pillow's save(exif=...) takes) with the Orientation tag alone."""
    from PIL import Image
    ex = Image.Exif()
    ex[0x0112] = tag
    b = ex.tobytes()
    assert b[:6] == b"Exif\x00\x00" and b[6:8] in (b"II", b"MM")
    if (b[6:8] == b"MM") != big_endian:
        b = tiff_swap_order(b)
    return b


def with_exif(data, tag, big_endian=False):
    """The same JPEG file with an Exif APP1 segment (Orientation = tag) spliced in behind SOI: same scans, same coefficients."""
    import struct
    ex = exif_bytes(tag, big_endian)
    assert data[:2] == b"\xff\xd8"
    return data[:2] + b"\xff\xe1" + struct.pack(">H", len(ex) + 2) + ex + data[2:]


def pil_oriented(data, s=1):
    """Pillow's decode of the file at scale 1 / s (draft), turned by ImageOps.exif_transpose -> (H, W, 3) u8 RGB."""
    from PIL import Image, ImageOps
    im = Image.open(io.BytesIO(data))
    w, h = im.size
    if s > 1:
        im.draft("L" if im.mode == "L" else "RGB", (w // s, h // s))
        assert im.size == (-(-w // s), -(-h // s)), (im.size, s)
    return np.asarray(ImageOps.exif_transpose(im).convert("RGB"), dtype=np.uint8)


def tiff_swap_order(b):
    """Rewrite the single-IFD Exif block Pillow emits (SHORT / LONG values held in the entries) in the other byte order."""
    import struct
    t = bytearray(b[6:])
    src, dst = ("<", ">") if t[:2] == b"II" else (">", "<")
    off, = struct.unpack_from(src + "I", t, 4)
    n, = struct.unpack_from(src + "H", t, off)
    out = bytearray(t)
    out[0:4] = b"MM\x00\x2a" if dst == ">" else b"II\x2a\x00"
    struct.pack_into(dst + "I", out, 4, off)
    struct.pack_into(dst + "H", out, off, n)
    for i in range(n):
        e = off + 2 + 12 * i
        tag, typ, cnt = struct.unpack_from(src + "HHI", t, e)
        struct.pack_into(dst + "HHI", out, e, tag, typ, cnt)
        assert typ in (3, 4) and cnt == 1
        if typ == 3:
            struct.pack_into(dst + "H", out, e + 8, struct.unpack_from(src + "H", t, e + 8)[0])
        else:
            struct.pack_into(dst + "I", out, e + 8, struct.unpack_from(src + "I", t, e + 8)[0])
    nxt, = struct.unpack_from(src + "I", t, off + 2 + 12 * n)
    struct.pack_into(dst + "I", out, off + 2 + 12 * n, nxt)
    return b[:6] + bytes(out)
