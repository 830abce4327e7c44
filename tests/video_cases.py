"""Inputs for the Motion-JPEG video tests (modules/utils/video.py, decode_video_batch, the default Huffman tables of
csrc/jpeg.hip).  TEST SUPPORT ONLY.  Everything is made in memory with Pillow and struct.

`strip_dht` cuts DHT segments out of a file Pillow wrote without `optimize`, i.e. with the standard tables of ITU T.81
Annex K.3: libjpeg-turbo (Pillow) decodes such a file with the tables it presets (std_huff_tables), which is what the tests
pin the product to.  Pillow cannot write a PROGRESSIVE file with the standard tables (libjpeg forces optimised tables in
progressive mode), so `progressive_std` re-codes a sequential file's coefficients as a progressive one -- one interleaved DC
scan, one full-band AC scan per component, no successive approximation, every block closed by EOB0 because the standard AC
tables hold no EOBn run symbols -- with the standard tables taken from the source file's own DHT segments.  The tests check it
against Pillow before they use it: Pillow must decode it, with and without its DHT segments, to the sequential file's pixels."""
import io
import struct

import numpy as np

ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35,
          42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)


def smooth(rng, w, h):
    return np.clip(np.cumsum(np.cumsum(rng.normal(0, 3, (h, w, 3)), 0), 1) + 128, 0, 255).astype(np.uint8)


def noise(rng, w, h):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def encode(img, gray=False, **kw):
    """RGB array -> JPEG bytes by Pillow (non-optimised: the standard Huffman tables, four DHT segments; two for gray)."""
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img[..., 0] if gray else img).save(b, "JPEG", **kw)
    return b.getvalue()


def pil_rgb(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"), dtype=np.uint8)


def segments(data):
    """[(marker, offset of the ff, length with the two marker bytes)] of the segments up to and including the first SOS."""
    assert data[:2] == b"\xff\xd8"
    pos, out = 2, []
    while True:
        assert data[pos] == 0xff
        m, ln = data[pos + 1], struct.unpack_from(">H", data, pos + 2)[0]
        out.append((m, pos, 2 + ln))
        if m == 0xda:
            return out
        pos += 2 + ln


def dht_tables(data):
    """{(class, slot): (bits[1..16], values)} of every table the file's DHT segments (in front of the first scan) define."""
    tabs = {}
    for m, pos, ln in segments(data):
        if m != 0xc4:
            continue
        s, e = pos + 4, pos + ln
        while s < e:
            bits = list(data[s + 1:s + 17])
            n = sum(bits)
            tabs[(data[s] >> 4, data[s] & 15)] = (bits, list(data[s + 17:s + 17 + n]))
            s += 17 + n
    return tabs


def strip_dht(data, keep=lambda tc, th: False):
    """The file without its DHT segments in front of the first scan; keep(class, slot) -> True keeps that segment (Pillow
    writes one table per segment).  -> (bytes, number of segments cut)."""
    out, cut, last = bytearray(data[:2]), 0, 2
    for m, pos, ln in segments(data):
        if m == 0xc4 and not keep(data[pos + 4] >> 4, data[pos + 4] & 15):
            cut += 1
        else:
            out += data[pos:pos + ln]
        last = pos + ln
    return bytes(out + data[last:]), cut


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, size):
        self.acc = (self.acc << size) | code
        self.n += size
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xff
            self.out.append(b)
            if b == 0xff:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)
        return bytes(self.out)


def _codes(bits, vals):
    code, k, out = 0, 0, {}
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def _value(v):
    s = int(abs(v)).bit_length()
    return s, (v if v >= 0 else v + (1 << s) - 1)


def progressive_std(data, info, coefs):
    """A sequential Pillow file (standard tables) and its quantised coefficients (info: the product's fp_jpeg_info, coefs: int16
    numpy in its layout) -> a progressive file (SOF2) of the same coefficients coded with the same standard tables."""
    segs = segments(data)
    tabs = {k: _codes(*v) for k, v in dht_tables(data).items()}
    nc = info.ncomp
    head = bytearray(b"\xff\xd8")
    ids = []
    for m, pos, ln in segs:
        if m == 0xc0:
            head += b"\xff\xc2" + data[pos + 2:pos + ln]
            ids = [data[pos + 10 + 3 * c] for c in range(nc)]
        elif m != 0xda:
            head += data[pos:pos + ln]
    slot = [0 if c == 0 else 1 for c in range(nc)]

    def block(c, by, bx):
        o = info.coef_off[c] + (by * info.blocks_w[c] + bx) * 64
        return coefs[o:o + 64]

    out = bytes(head)
    # DC scan, interleaved over every component (a gray file: its one component, block by block)
    w = _Bits()
    pred = [0] * nc
    sos = bytes([nc]) + b"".join(bytes([ids[c], slot[c] << 4]) for c in range(nc)) + bytes([0, 0, 0])
    if nc == 1:
        order = [(0, by, bx) for by in range((info.comp_h[0] + 7) // 8) for bx in range((info.comp_w[0] + 7) // 8)]
    else:
        order = [(c, my * info.vs[c] + v, mx * info.hs[c] + h) for my in range(info.mcuy) for mx in range(info.mcux)
                 for c in range(nc) for v in range(info.vs[c]) for h in range(info.hs[c])]
    for c, by, bx in order:
        dc = int(block(c, by, bx)[0])
        s, bits = _value(dc - pred[c])
        pred[c] = dc
        w.put(*tabs[(0, slot[c])][s])
        if s:
            w.put(bits, s)
    out += b"\xff\xda" + struct.pack(">H", 2 + len(sos)) + sos + w.flush()
    # one AC scan per component: the whole band 1 .. 63, every block closed by EOB0 unless its last coefficient is coded
    for c in range(nc):
        w = _Bits()
        ac = tabs[(1, slot[c])]
        for by in range((info.comp_h[c] + 7) // 8):
            for bx in range((info.comp_w[c] + 7) // 8):
                blk = block(c, by, bx)
                run = 0
                for k in range(1, 64):
                    v = int(blk[ZIGZAG[k]])
                    if v == 0:
                        run += 1
                        continue
                    while run > 15:
                        w.put(*ac[0xf0])
                        run -= 16
                    s, bits = _value(v)
                    w.put(*ac[(run << 4) | s])
                    w.put(bits, s)
                    run = 0
                if run:
                    w.put(*ac[0x00])
        sos = bytes([1, ids[c], slot[c], 1, 63, 0])
        out += b"\xff\xda" + struct.pack(">H", 2 + len(sos)) + sos + w.flush()
    return out + b"\xff\xd9"


# ---- containers, assembled by hand (independent of VideoWriter) ------------------------------------------------------

def chunk(cid, body):
    return cid + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def riff_list(kind, body):
    return b"LIST" + struct.pack("<I", 4 + len(body)) + kind + body


def avi_headers(w, h, n, rate=30000, scale=1001, fourcc=b"MJPG", audio_first=False):
    """LIST hdrl: avih + a video strl (and, with audio_first, an audio strl in front of it: the video stream is then number 1)."""
    avih = struct.pack("<14I", 33367, 0, 0, 0x10, n, 0, 2 if audio_first else 1, 0, w, h, 0, 0, 0, 0)
    strh = struct.pack("<4s4sIHHIIIIIIIi4H", b"vids", fourcc, 0, 0, 0, 0, scale, rate, 0, n, 0, 0xffffffff, 0, 0, 0, w, h)
    strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, fourcc, w * h * 3, 0, 0, 0, 0)
    strl = riff_list(b"strl", chunk(b"strh", strh) + chunk(b"strf", strf))
    if audio_first:
        astrh = struct.pack("<4s4sIHHIIIIIIIi4H", b"auds", b"\0\0\0\0", 0, 0, 0, 0, 1, 8000, 0, 0, 0, 0, 1, 0, 0, 0, 0)
        strl = riff_list(b"strl", chunk(b"strh", astrh) + chunk(b"strf", struct.pack("<HHIIHH", 1, 1, 8000, 8000, 1, 8))) + strl
    return riff_list(b"hdrl", chunk(b"avih", avih) + strl)


def riff_avi(body):
    return b"RIFF" + struct.pack("<I", 4 + len(body)) + b"AVI " + body
