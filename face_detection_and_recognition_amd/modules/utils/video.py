"""Motion-JPEG video: AVI and raw .mjpeg streams in, AVI out -- the container around the JPEG codec of modules/utils/jpeg.py.
The reference opens its videos with cv2.VideoCapture (fde/modules/utils/inference.py:96-111 and the "video" branch of every
driver's filter_faces_from_data); this build has no video library, and Motion-JPEG -- what webcams and IP cameras emit and what
cv2.VideoWriter(fourcc="MJPG") writes -- is the one codec it decodes and encodes itself: every frame is a baseline JPEG.

    VideoReader(path)      AVI 1.0 (RIFF 'AVI ': hdrl/avih, the first video strl, movi, idx1) with an MJPG / mjpg / jpeg / JPEG
                           stream, or a raw stream of concatenated JPEGs (.mjpeg / .mjpg / a file that begins ff d8).  The file is
                           memory-mapped; frame_bytes(i) slices it; read(start, stop, device) decodes the frames with
                           decode_video_batch into one (B, H, W, 3) u8 tensor; batches(batch, device) walks the file
    VideoWriter(path, fps) AVI 1.0 with one MJPG stream: write(frames) encodes a (B, H, W, 3) u8 device tensor (or a list of
                           frames) with encode_jpeg_batch, one device call per batch, and appends 00dc chunks; close() writes
                           idx1 and the sizes

Pure Python on the host: parsing is struct.unpack_from over the mapping and find(); the walk of a raw stream takes one
Python step per segment and per 0xff byte of the entropy-coded data, never one per byte.
**Out of scope** (VideoUnsupported names what was found): every codec but Motion-JPEG, audio (other streams' chunks are
skipped), OpenDML (AVIX segments / indx: files over 2 GiB), field-interlaced MJPEG (two images per chunk), capture devices,
seeking by time (frames are addressed by index).  What cv2.VideoWriter writes is not pinned (cv2 is absent): the layout is the
published AVI 1.0 one, build-defined where the documents leave a choice ("Video")."""
import mmap
import os
import struct
from fractions import Fraction

from ... import _lib as L

MJPEG_FOURCCS = (b"MJPG", b"mjpg", b"jpeg", b"JPEG")
RAW_EXTENSIONS = (".mjpeg", ".mjpg")
AVI_MAX_BYTES = (1 << 31) - 1       # AVI 1.0: one RIFF chunk, signed 32-bit offsets in common readers; beyond it is OpenDML
AVIF_HASINDEX = 0x10
AVIIF_KEYFRAME = 0x10
FPS_MAX_DENOMINATOR = 100000        # VideoWriter: dwRate / dwScale = Fraction(fps).limit_denominator(this)
_HEADER_BYTES = 224                 # RIFF .. the first byte behind the 'movi' fourcc, as VideoWriter lays it out
_MOVI_FOURCC_AT = 220


class VideoUnsupported(L.FacepathError):
    """A video outside this build's scope; the message names what was found (the codec's fourcc, AVIX, ...)."""


def _fourcc(b):
    return bytes(b).decode("latin-1")


def jpeg_end(buf, pos, end):
    """The offset behind the EOI of the JPEG image that starts (ff d8) at pos, by a marker-aware walk: segment lengths up to
    SOS, then the entropy-coded data up to the next marker that is not a stuffed zero, RSTn or a fill byte.  ff d9 inside an
    APPn segment is stepped over with its segment.  None: the image is cut off before its EOI."""
    pos += 2
    while pos + 2 <= end:
        if buf[pos] != 0xff:
            return None
        m = buf[pos + 1]
        if m == 0xff:                                   # fill byte
            pos += 1
            continue
        if m == 0xd9:
            return pos + 2
        if m == 0x01 or 0xd0 <= m <= 0xd8:              # markers without a length
            pos += 2
            continue
        if pos + 4 > end:
            return None
        pos += 2 + struct.unpack_from(">H", buf, pos + 2)[0]
        if m != 0xda:
            continue
        while True:                                     # the scan's entropy-coded data
            j = buf.find(b"\xff", pos, end)
            if j < 0 or j + 1 >= end:
                return None
            n = buf[j + 1]
            if n == 0 or 0xd0 <= n <= 0xd7:
                pos = j + 2
            elif n == 0xff:
                pos = j + 1
            else:
                pos = j
                break
    return None


def jpeg_size(buf, pos, end):
    """(width, height) from the frame header (SOFn) of the JPEG image at pos; None when there is none in front of the scan."""
    pos += 2
    while pos + 4 <= end and buf[pos] == 0xff:
        m = buf[pos + 1]
        if m == 0xff:
            pos += 1
            continue
        if m == 0x01 or 0xd0 <= m <= 0xd8:
            pos += 2
            continue
        if m in (0xd9, 0xda):
            return None
        if 0xc0 <= m <= 0xcf and m not in (0xc4, 0xc8, 0xcc):
            if pos + 9 > end:
                return None
            h, w = struct.unpack_from(">HH", buf, pos + 5)
            return w, h
        pos += 2 + struct.unpack_from(">H", buf, pos + 2)[0]
    return None


class VideoReader:
    """A Motion-JPEG AVI or raw MJPEG stream, memory-mapped.  width, height, fps (a fractions.Fraction: dwRate / dwScale of the
    stream header, avih.dwMicroSecPerFrame only where the scale is 0; None for a raw stream), n_frames, codec (the fourcc as
    str; "MJPG" for a raw stream), len(), frame_bytes(i), read(start, stop, device), batches(batch, device).  Frames are
    addressed by index only.  A zero-length video chunk is a dropped frame and repeats the frame before it.  A file cut off in
    the middle of a chunk gives the frames in front of the cut.  The codec is Motion-JPEG where strf.biCompression or
    strh.fccHandler says so.  The check for a second image in a chunk (field-interlaced MJPEG) looks at the first frame only: a
    stream that turns interlaced later is opened, and its chunks decode to their first field."""

    def __init__(self, path):
        self.path = path
        self._file = open(path, "rb")
        try:
            if os.fstat(self._file.fileno()).st_size == 0:
                raise L.FacepathError(f"{path}: an empty file")
            self._mm = mmap.mmap(self._file.fileno(), 0, access=mmap.ACCESS_READ)
        except Exception:
            self._file.close()
            raise
        self.width = self.height = 0
        self.fps = None
        self.codec = "MJPG"
        self._frames = []                 # (offset, length) of each frame's JPEG bytes in the mapping
        try:
            buf = self._mm
            if buf[:4] == b"RIFF" and buf[8:12] == b"AVI ":
                self._parse_avi()
            elif buf[:2] == b"\xff\xd8" or path.lower().endswith(RAW_EXTENSIONS):
                self._parse_raw()
            else:
                raise VideoUnsupported(f"{path}: neither a RIFF AVI file nor a raw MJPEG stream (it begins {bytes(buf[:12])!r})")
        except Exception:
            self.close()
            raise
        self.n_frames = len(self._frames)

    # ---- containers ------------------------------------------------------------------------------------------------

    def _parse_raw(self):
        buf, n, pos = self._mm, len(self._mm), 0
        while True:
            pos = buf.find(b"\xff\xd8", pos)
            if pos < 0:
                break
            e = jpeg_end(buf, pos, n)
            if e is None:                 # cut off: the frames in front of the cut
                break
            self._frames.append((pos, e - pos))
            pos = e
        if self._frames:
            size = jpeg_size(buf, self._frames[0][0], self._frames[0][0] + self._frames[0][1])
            if size:
                self.width, self.height = size

    def _parse_avi(self):
        buf, n = self._mm, len(self._mm)
        riff_end = min(n, 8 + struct.unpack_from("<I", buf, 4)[0])
        if riff_end + 12 <= n and buf[riff_end:riff_end + 4] == b"RIFF" and buf[riff_end + 8:riff_end + 12] == b"AVIX":
            raise VideoUnsupported(f"{self.path}: an OpenDML AVI (AVIX segment); files over 2 GiB are out of scope")
        avih = movi = idx1 = None
        stream = None                     # (stream number, strh, strf) of the first video stream
        n_strl = 0
        pos = 12
        while pos + 8 <= riff_end:
            cid, size = struct.unpack_from("<4sI", buf, pos)
            body, end = pos + 8, min(riff_end, pos + 8 + size)
            if cid == b"LIST" and body + 4 <= end:
                kind = buf[body:body + 4]
                if kind == b"hdrl":
                    p = body + 4
                    while p + 8 <= end:
                        c2, s2 = struct.unpack_from("<4sI", buf, p)
                        b2, e2 = p + 8, min(end, p + 8 + s2)
                        if c2 == b"avih":
                            avih = (b2, e2)
                        elif c2 == b"LIST" and buf[b2:b2 + 4] == b"strl":
                            strh = strf = None
                            q = b2 + 4
                            while q + 8 <= e2:
                                c3, s3 = struct.unpack_from("<4sI", buf, q)
                                if c3 == b"strh":
                                    strh = (q + 8, min(e2, q + 8 + s3))
                                elif c3 == b"strf":
                                    strf = (q + 8, min(e2, q + 8 + s3))
                                elif c3 == b"indx":
                                    raise VideoUnsupported(f"{self.path}: an OpenDML AVI (indx chunk); out of scope")
                                q += 8 + s3 + (s3 & 1)
                            if stream is None and strh and strh[1] - strh[0] >= 36 and buf[strh[0]:strh[0] + 4] == b"vids":
                                stream = (n_strl, strh, strf)
                            n_strl += 1
                        p += 8 + s2 + (s2 & 1)
                elif kind == b"movi" and movi is None:
                    movi = (body, end)    # body: the 'movi' fourcc, which idx1's relative offsets count from
            elif cid == b"idx1":
                idx1 = (body, end)
            pos += 8 + size + (size & 1)
        if stream is None:
            raise VideoUnsupported(f"{self.path}: an AVI without a video stream")
        if movi is None:
            raise L.FacepathError(f"{self.path}: an AVI without a movi list")
        number, strh, strf = stream
        handler = bytes(buf[strh[0] + 4:strh[0] + 8])
        compression = bytes(buf[strf[0] + 16:strf[0] + 20]) if strf and strf[1] - strf[0] >= 20 else b""
        if compression in MJPEG_FOURCCS:              # either field may name the codec
            self.codec = _fourcc(compression)
        elif handler in MJPEG_FOURCCS:
            self.codec = _fourcc(handler)
        else:
            found = compression if compression.strip(b"\0") else handler
            raise VideoUnsupported(f"{self.path}: codec {_fourcc(found)!r} ({found!r}); only Motion-JPEG "
                                   "(MJPG / mjpg / jpeg / JPEG) is decoded")
        scale, rate = struct.unpack_from("<II", buf, strh[0] + 20)
        if scale and rate:
            self.fps = Fraction(rate, scale)
        elif avih and avih[1] - avih[0] >= 4 and struct.unpack_from("<I", buf, avih[0])[0]:
            self.fps = Fraction(1000000, struct.unpack_from("<I", buf, avih[0])[0])
        if strf and strf[1] - strf[0] >= 12:
            w, h = struct.unpack_from("<ii", buf, strf[0] + 4)
            self.width, self.height = w, abs(h)
        elif avih and avih[1] - avih[0] >= 40:
            self.width, self.height = struct.unpack_from("<II", buf, avih[0] + 32)
        ids = (b"%02ddc" % number, b"%02ddb" % number)
        chunks = self._index_chunks(idx1, movi, ids) if idx1 else None
        if chunks is None:
            chunks = self._walk_movi(movi, ids)
        for off, size in chunks:
            if size == 0:                 # a dropped frame: the one before it again
                if not self._frames:
                    raise L.FacepathError(f"{self.path}: the first video chunk is empty (a dropped frame with none before it)")
                self._frames.append(self._frames[-1])
            else:
                self._frames.append((off, size))
        if self._frames:                  # field-interlaced MJPEG: a second image behind the first one's EOI (first frame only)
            off, size = self._frames[0]
            e = jpeg_end(buf, off, off + size)
            if e is not None and buf.find(b"\xff\xd8", e, off + size) >= 0:
                raise VideoUnsupported(f"{self.path}: two JPEG images in one chunk (field-interlaced Motion-JPEG); out of scope")

    def _walk_movi(self, movi, ids):
        buf, n = self._mm, len(self._mm)
        chunks = []
        pos, end = movi[0] + 4, movi[1]
        while pos + 8 <= end:
            cid, size = struct.unpack_from("<4sI", buf, pos)
            if cid == b"LIST":            # 'rec ' groups: their chunks follow the 12-byte header
                pos += 12
                continue
            if pos + 8 + size > n:        # cut off in the middle of this chunk
                break
            if cid in ids:
                chunks.append((pos + 8, size))
            pos += 8 + size + (size & 1)
        return chunks

    def _index_chunks(self, idx1, movi, ids):
        """The video chunks by idx1, or None for an index that does not point at them (the caller walks movi then).  The
        offsets count from the 'movi' fourcc or from the start of the file: the first entry tells which."""
        buf, n = self._mm, len(self._mm)
        count = (idx1[1] - idx1[0]) // 16
        if count == 0:
            return None
        entries = struct.iter_unpack("<4sIII", buf[idx1[0]:idx1[0] + 16 * count])
        base = None
        chunks = []
        for cid, _flags, off, size in entries:
            if base is None:
                if movi[0] + off + 4 <= n and buf[movi[0] + off:movi[0] + off + 4] == cid:
                    base = movi[0]
                elif off + 4 <= n and buf[off:off + 4] == cid:
                    base = 0
                else:
                    return None
            if cid not in ids:
                continue
            at = base + off
            if at + 8 + size > n or struct.unpack_from("<4sI", buf, at) != (cid, size):
                return None
            chunks.append((at + 8, size))
        return chunks

    # ---- frames ----------------------------------------------------------------------------------------------------

    def __len__(self):
        return self.n_frames

    def frame_bytes(self, i):
        """The JPEG file of frame i (bytes)."""
        if not -self.n_frames <= i < self.n_frames:
            raise IndexError(f"frame {i} of {self.n_frames}")
        off, size = self._frames[i]
        return self._mm[off:off + size]

    def read(self, start, stop, device, bgr=True, entropy="host", reduce=1, **kw):
        """Frames start .. stop - 1 -> (B, H, W, 3) u8 on `device` (decode_video_batch: one launch sequence per chunk)."""
        from .jpeg import decode_video_batch
        start, stop, _ = slice(start, stop).indices(self.n_frames)
        if stop <= start:
            raise IndexError(f"frames {start} .. {stop} of {self.n_frames}: nothing to read")
        return decode_video_batch([self.frame_bytes(i) for i in range(start, stop)], device, bgr=bgr, entropy=entropy,
                                  reduce=reduce, **kw)

    def batches(self, batch, device, **kw):
        """Yields (first_index, frames) over the whole file, `batch` frames at a time (the last batch may be shorter)."""
        if batch < 1:
            raise ValueError(f"batch must be positive, not {batch!r}")
        for s in range(0, self.n_frames, batch):
            yield s, self.read(s, min(self.n_frames, s + batch), device, **kw)

    def close(self):
        if getattr(self, "_mm", None) is not None:
            self._mm.close()
            self._mm = None
        self._file.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def read_frames(source, lo, hi, device):
    """Frames lo .. hi - 1 of a driver's frame source -- a VideoReader, or a sorted list of image paths (imread_batch) -- as
    one (B, H, W, 3) u8 tensor on `device`; ValueError where a folder's frames differ in size."""
    import torch
    if isinstance(source, VideoReader):
        return source.read(lo, min(hi, len(source)), device)
    from .jpeg import imread_batch
    frames = imread_batch(source[lo:hi], device)
    if not isinstance(frames, torch.Tensor):
        raise ValueError("the frames of a video share one size")
    return frames


class VideoWriter:
    """An AVI 1.0 file with one Motion-JPEG stream: RIFF 'AVI ' / LIST hdrl (avih, LIST strl (strh, strf)) / LIST movi (00dc
    chunks, padded to even length) / idx1 (offsets relative to the 'movi' fourcc, every entry AVIIF_KEYFRAME).  dwRate / dwScale
    = Fraction(fps).limit_denominator(100000); dwSuggestedBufferSize = the largest chunk; fccHandler = biCompression = 'MJPG'.
    The frames keep their Huffman tables (DHT segments), so that every reader decodes them.  write(frames): a (B, H, W, 3) u8
    device tensor or a list of (H, W, 3) frames, BGR unless bgr=False, all of one size; one encode call per write.  encode: the
    batch encoder, encode_jpeg_batch by default (encode_jpeg_batch_emulate takes host arrays: tests without a device).
    **Files stay below 2^31 - 1 bytes: a write that would pass it raises VideoUnsupported (OpenDML is out of scope).**
    close() writes the index and patches the sizes; the writer is a context manager."""

    def __init__(self, path, fps, quality=95, subsampling="4:2:0", encode=None, bgr=True):
        frac = Fraction(fps).limit_denominator(FPS_MAX_DENOMINATOR)
        if frac <= 0 or frac.numerator >= 1 << 32:
            raise ValueError(f"fps {fps!r}: a positive rate")
        if encode is None:
            from .jpeg import encode_jpeg_batch as encode
        self.path, self.fps, self.quality, self.subsampling, self.bgr = path, frac, quality, subsampling, bgr
        self._encode = encode
        self.width = self.height = 0
        self._index = []                  # (offset of the chunk header from the 'movi' fourcc, length)
        self._file = open(path, "wb")
        self._file.write(bytes(_HEADER_BYTES))
        self._pos = _HEADER_BYTES

    @property
    def n_frames(self):
        return len(self._index)

    def write(self, frames):
        if self._file is None:
            raise L.FacepathError(f"{self.path}: write() after close()")
        frames = list(frames)             # a (B, H, W, 3) tensor or array gives its B frames
        if not frames:
            return
        for f in frames:
            h, w = int(f.shape[0]), int(f.shape[1])
            if not self.width:
                self.width, self.height = w, h
            if len(f.shape) != 3 or (w, h) != (self.width, self.height):
                raise ValueError("the frames of a video share one size")
        files = self._encode(frames, quality=self.quality, subsampling=self.subsampling, bgr=self.bgr)
        for data in files:
            size = len(data)
            after = self._pos + 8 + size + (size & 1)
            if after + 8 + 16 * (len(self._index) + 1) > AVI_MAX_BYTES:
                raise VideoUnsupported(f"{self.path}: the file would pass 2^31 - 1 bytes; AVI 1.0 ends there (OpenDML is out of "
                                       "scope): start another file")
            self._file.write(b"00dc" + struct.pack("<I", size) + data + (b"\0" if size & 1 else b""))
            self._index.append((self._pos - _MOVI_FOURCC_AT, size))
            self._pos = after

    def close(self):
        if self._file is None:
            return
        f, n = self._file, len(self._index)
        f.write(b"idx1" + struct.pack("<I", 16 * n) + b"".join(struct.pack("<4sIII", b"00dc", AVIIF_KEYFRAME, off, size)
                                                                for off, size in self._index))
        total = self._pos + 8 + 16 * n
        largest = max((size for _, size in self._index), default=0)
        rate, scale = self.fps.numerator, self.fps.denominator
        w, h = self.width, self.height
        avih = struct.pack("<14I", int(round(1000000 / self.fps)), 0, 0, AVIF_HASINDEX, n, 0, 1, largest, w, h, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIIi4H", b"vids", b"MJPG", 0, 0, 0, 0, scale, rate, 0, n, largest, 0xffffffff, 0, 0, 0, w, h)
        strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", w * h * 3, 0, 0, 0, 0)
        strl = b"LIST" + struct.pack("<I", 4 + 8 + len(strh) + 8 + len(strf)) + b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh \
            + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"LIST" + struct.pack("<I", 4 + 8 + len(avih) + len(strl)) + b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + strl
        head = b"RIFF" + struct.pack("<I", total - 8) + b"AVI " + hdrl + b"LIST" + struct.pack("<I", self._pos - _MOVI_FOURCC_AT) + b"movi"
        assert len(head) == _HEADER_BYTES
        f.seek(0)
        f.write(head)
        f.close()
        self._file = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
