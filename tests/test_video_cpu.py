"""Motion-JPEG video on the host: the default Huffman tables of csrc/jpeg.hip (files without DHT segments decode as
libjpeg-turbo decodes them), VideoReader on hand-assembled AVI and raw streams, VideoWriter's layout, the drivers' video
branch.  No GPU."""
import ctypes
import struct
from fractions import Fraction

import numpy as np
import pytest

import video_cases as V
from face_detection_and_recognition_amd import _lib as L
from face_detection_and_recognition_amd.modules.utils import jpeg as J
from face_detection_and_recognition_amd.modules.utils.files import get_file_type
from face_detection_and_recognition_amd.modules.utils.video import VideoReader, VideoUnsupported, VideoWriter

GEOMETRY = ("width", "height", "ncomp", "progressive", "restart_interval", "mcux", "mcuy", "n_coefs")
GEOMETRY_ARRAYS = ("hs", "vs", "blocks_w", "blocks_h", "comp_w", "comp_h", "coef_off")


def _same_decode(a, b):
    ia, ca = J.entropy_decode(a)
    ib, cb = J.entropy_decode(b)
    for k in GEOMETRY:
        assert getattr(ia, k) == getattr(ib, k), k
    for k in GEOMETRY_ARRAYS:
        assert list(getattr(ia, k)) == list(getattr(ib, k)), k
    assert np.array_equal(np.ctypeslib.as_array(ia.quant), np.ctypeslib.as_array(ib.quant))
    assert ca.dtype == cb.dtype and np.array_equal(ca.numpy(), cb.numpy())
    return ia, ca


def _files():
    rng = np.random.default_rng(5)
    out = {}
    for name, kw in (("444", dict(subsampling=0)), ("422", dict(subsampling=1)), ("420", dict(subsampling=2)), ("gray", dict(gray=True))):
        out[name] = V.encode(V.smooth(rng, 50, 38), quality=80, **kw)
    out["420-noise"] = V.encode(V.noise(rng, 37, 21), quality=100, subsampling=2)     # every code of the tables, long codes too
    return out


FILES = _files()


# ---- files without Huffman tables ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(FILES))
def test_dht_less_file_decodes_as_libjpeg_turbo(name):
    full = FILES[name]
    stripped, cut = V.strip_dht(full)
    assert cut == (2 if name == "gray" else 4) and b"\xff\xc4" not in stripped[:600]
    assert np.array_equal(V.pil_rgb(stripped), V.pil_rgb(full))            # the oracle itself: Pillow takes the stripped file
    _same_decode(stripped, full)
    scan = L.FpJpegScan()                                                  # the device entropy decoder's preparation too
    info = L.FpJpegInfo()
    buf = (ctypes.c_uint8 * len(stripped)).from_buffer_copy(stripped)
    assert L.load().fp_jpeg_scan_prepare(buf, len(stripped), ctypes.byref(info), ctypes.byref(scan)) == 0
    full_scan = L.FpJpegScan()
    fbuf = (ctypes.c_uint8 * len(full)).from_buffer_copy(full)
    assert L.load().fp_jpeg_scan_prepare(fbuf, len(full), ctypes.byref(info), ctypes.byref(full_scan)) == 0
    for i in range(info.ncomp):
        for a, b in ((scan.dc[i], full_scan.dc[i]), (scan.ac[i], full_scan.ac[i])):
            assert bytes(a) == bytes(b)


@pytest.mark.parametrize("name", ["420", "444", "gray"])
def test_progressive_file_gets_no_default_tables(name):
    """libjpeg-turbo presets the standard tables in its SEQUENTIAL Huffman decoder only (jdhuff.c jinit_huff_decoder); its
    progressive decoder (jdphuff.c) refuses a scan whose table no DHT defined.  Pillow is the judge of that as well: it decodes
    the hand-coded progressive file with its tables and raises without them, and so does the product."""
    seq = FILES[name]
    info, coefs = J.entropy_decode(seq)
    prog = V.progressive_std(seq, info, coefs.numpy())
    assert b"\xff\xc2" in prog[:600] and len(V.dht_tables(prog)) == (2 if name == "gray" else 4)
    assert np.array_equal(V.pil_rgb(prog), V.pil_rgb(seq))                 # the hand-coded file is a valid progressive file
    pinfo, pcoefs = J.entropy_decode(prog)
    assert pinfo.progressive == 1 and np.array_equal(pcoefs.numpy(), coefs.numpy())
    cuts = [V.strip_dht(prog)[0]]
    if name != "gray":
        cuts.append(V.strip_dht(prog, keep=lambda tc, th: th == 0)[0])      # the chroma tables alone missing
    for stripped in cuts:
        with pytest.raises(OSError):
            V.pil_rgb(stripped)
        sinfo, buf = J.parse(stripped)
        out = np.zeros(int(sinfo.n_coefs), np.int16)
        rc = L.load().fp_jpeg_entropy_decode(buf, len(stripped), ctypes.byref(sinfo), out.ctypes.data_as(ctypes.c_void_p))
        assert rc == J.FP_ERR_INVALID_ARG


def test_chroma_tables_alone_missing():
    full = FILES["420"]
    stripped, cut = V.strip_dht(full, keep=lambda tc, th: th == 0)
    assert cut == 2 and len(V.dht_tables(stripped)) == 2
    assert np.array_equal(V.pil_rgb(stripped), V.pil_rgb(full))
    _same_decode(stripped, full)


def test_slot_two_stays_absent():
    stripped, _ = V.strip_dht(FILES["420"])
    m, pos, ln = V.segments(stripped)[-1]
    assert m == 0xda and stripped[pos + 4] == 3
    bad = bytearray(stripped)
    bad[pos + 8] = 0x22                                                    # the second component: DC and AC table 2
    info, buf = J.parse(bytes(bad))
    coefs = np.zeros(int(info.n_coefs), np.int16)
    rc = L.load().fp_jpeg_entropy_decode(buf, len(bad), ctypes.byref(info), coefs.ctypes.data_as(ctypes.c_void_p))
    assert rc == J.FP_ERR_INVALID_ARG
    scan = L.FpJpegScan()
    assert L.load().fp_jpeg_scan_prepare(buf, len(bad), ctypes.byref(info), ctypes.byref(scan)) == J.FP_ERR_INVALID_ARG


# ---- the reader on hand-assembled containers ---------------------------------------------------------------------------

W, H = 48, 40


def _frames():
    rng = np.random.default_rng(9)
    fr = [V.encode(V.smooth(rng, W, H), quality=q, subsampling=2) for q in (70, 75, 80, 85)]
    if not len(fr[0]) & 1:                                                 # an odd chunk: a five-byte COM segment turns the parity
        fr[0] = fr[0][:2] + b"\xff\xfe\x00\x03x" + fr[0][2:]
    assert len(fr[0]) & 1
    return fr


FRAMES = _frames()
EXPECT = [FRAMES[0], FRAMES[1], FRAMES[1], FRAMES[2], FRAMES[3]]           # the third chunk is empty: a dropped frame


def _movi():
    """-> (LIST movi bytes, [(chunk id, offset of the chunk header from the 'movi' fourcc, length)])."""
    body, index = b"movi", []

    def add(cid, data, into):
        index.append((cid, len(body) + len(into), len(data)))
        return into + V.chunk(cid, data)
    body = add(b"00dc", FRAMES[0], body)
    body = add(b"01wb", b"\x80" * 33, body)
    start = len(body)                                                      # a LIST rec group: a video and an audio chunk
    inner = b""
    index.append((b"00dc", start + 12, len(FRAMES[1])))
    inner += V.chunk(b"00dc", FRAMES[1])
    index.append((b"01wb", start + 12 + len(inner), 7))
    inner += V.chunk(b"01wb", b"\x80" * 7)
    body += V.riff_list(b"rec ", inner)
    body = add(b"00dc", b"", body)
    body = add(b"00dc", FRAMES[2], body)
    body = add(b"00dc", FRAMES[3], body)
    return b"LIST" + struct.pack("<I", len(body)) + body, index


def _avi(index_base=None, fourcc=b"MJPG"):
    hdrl = V.avi_headers(W, H, 5, fourcc=fourcc)
    movi, index = _movi()
    movi_fourcc_at = 12 + len(hdrl) + 8
    body = hdrl + movi + V.chunk(b"JUNK", b"\0" * 10)
    if index_base is not None:
        base = 0 if index_base == "movi" else movi_fourcc_at
        body += V.chunk(b"idx1", b"".join(struct.pack("<4sIII", cid, 0x10, base + off, size) for cid, off, size in index))
    data = V.riff_avi(body)
    assert data[movi_fourcc_at:movi_fourcc_at + 4] == b"movi"
    return data


def _open(tmp_path, data, name="clip.avi"):
    p = tmp_path / name
    p.write_bytes(data)
    return VideoReader(str(p))


@pytest.mark.parametrize("index_base", [None, "movi", "file"])
def test_reader_walks_movi_and_both_kinds_of_idx1(tmp_path, index_base):
    data = _avi(index_base)
    assert all(i % 2 == 0 for i in (data.find(f) - 8 for f in FRAMES))     # chunks at even offsets: the pad byte is there
    with _open(tmp_path, data) as r:
        assert (r.width, r.height, r.n_frames, len(r), r.codec) == (W, H, 5, 5, "MJPG")
        assert r.fps == Fraction(30000, 1001) and isinstance(r.fps, Fraction)
        got = [r.frame_bytes(i) for i in range(5)]
        assert got == EXPECT and all(isinstance(g, bytes) for g in got)
        with pytest.raises(IndexError):
            r.frame_bytes(5)


def test_reader_unusable_index_falls_back_to_movi(tmp_path):
    data = bytearray(_avi("movi"))
    at = data.rfind(b"idx1") + 8
    struct.pack_into("<I", data, at + 8, 0x7fff0000)                       # the first entry points nowhere
    with _open(tmp_path, bytes(data)) as r:
        assert [r.frame_bytes(i) for i in range(5)] == EXPECT


def test_reader_takes_the_video_stream_behind_an_audio_stream(tmp_path):
    body = V.avi_headers(W, H, 2, audio_first=True) + V.riff_list(b"movi", V.chunk(b"00wb", b"\x80" * 9) + V.chunk(b"01dc", FRAMES[0])
                                                                  + V.chunk(b"01db", FRAMES[1]))
    with _open(tmp_path, V.riff_avi(body)) as r:
        assert [r.frame_bytes(i) for i in range(len(r))] == FRAMES[:2]


def test_reader_scale_zero_takes_avih_period(tmp_path):
    body = V.avi_headers(W, H, 1, rate=0, scale=0) + V.riff_list(b"movi", V.chunk(b"00dc", FRAMES[0]))
    with _open(tmp_path, V.riff_avi(body)) as r:
        assert r.fps == Fraction(1000000, 33367)


def test_reader_takes_the_codec_from_either_field(tmp_path):
    data = _avi()
    at = data.find(b"strf") + 8 + 16                                       # biCompression
    assert data[at:at + 4] == b"MJPG"
    with _open(tmp_path, data[:at] + b"\0\0\0\0" + data[at + 4:]) as r:    # the handler alone names the codec
        assert r.codec == "MJPG" and [r.frame_bytes(i) for i in range(5)] == EXPECT
    at = data.find(b"vids") + 4                                            # fccHandler
    with _open(tmp_path, data[:at] + b"\0\0\0\0" + data[at + 4:]) as r:    # biCompression alone
        assert r.codec == "MJPG" and len(r) == 5


def test_reader_refuses_what_is_out_of_scope(tmp_path):
    with pytest.raises(VideoUnsupported, match="H264"):
        _open(tmp_path, _avi(fourcc=b"H264"))
    avix = _avi() + b"RIFF" + struct.pack("<I", 16) + b"AVIX" + V.riff_list(b"movi", b"")
    with pytest.raises(VideoUnsupported, match="AVIX"):
        _open(tmp_path, avix)
    body = V.avi_headers(W, H, 2) + V.riff_list(b"movi", V.chunk(b"00dc", b"") + V.chunk(b"00dc", FRAMES[0]))
    with pytest.raises(L.FacepathError, match="first"):
        _open(tmp_path, V.riff_avi(body))
    body = V.avi_headers(W, H, 1) + V.riff_list(b"movi", V.chunk(b"00dc", FRAMES[0] + FRAMES[1]))
    with pytest.raises(VideoUnsupported, match="interlaced"):
        _open(tmp_path, V.riff_avi(body))
    with pytest.raises(VideoUnsupported):
        _open(tmp_path, b"\x89PNG\r\n\x1a\n" + b"\0" * 32, "clip.bin")
    assert issubclass(VideoUnsupported, L.FacepathError)


def test_reader_truncated_file_gives_the_frames_before_the_cut(tmp_path):
    data = _avi()
    cut = data.find(FRAMES[2]) + len(FRAMES[2]) // 2
    with _open(tmp_path, data[:cut]) as r:
        assert [r.frame_bytes(i) for i in range(len(r))] == EXPECT[:3]


def test_raw_stream_is_split_by_markers_not_by_ff_d9(tmp_path):
    app1 = b"\xff\xe1" + struct.pack(">H", 2 + 8) + b"ab\xff\xd9cd\xff\xd8"           # an APP1 holding ff d9 and ff d8
    three = [FRAMES[0], FRAMES[1][:2] + app1 + FRAMES[1][2:], FRAMES[2]]
    assert V.pil_rgb(three[1]).shape == (H, W, 3)
    with _open(tmp_path, b"".join(three), "cam.mjpeg") as r:
        assert r.fps is None and (r.width, r.height, r.codec) == (W, H, "MJPG")
        assert [r.frame_bytes(i) for i in range(len(r))] == three
    with _open(tmp_path, b"".join(three)[:-10], "cut.mjpg") as r:          # the last frame cut off
        assert [r.frame_bytes(i) for i in range(len(r))] == three[:2]
    restart = V.encode(V.noise(np.random.default_rng(2), W, H), quality=95, subsampling=2, restart_marker_blocks=2)
    assert b"\xff\xd0" in restart and b"\xff\x00" in restart               # RSTn and stuffed bytes inside the scan
    with _open(tmp_path, restart + FRAMES[0], "noext") as r:               # recognised by ff d8
        assert [r.frame_bytes(i) for i in range(len(r))] == [restart, FRAMES[0]]


# ---- the writer's layout, by a RIFF walker of this test's own ------------------------------------------------------------

def _walk(data, pos, end, path, found):
    """Every chunk of data[pos:end] -> found[(path..., id)] = [(offset of the body, size)]; sizes and padding checked."""
    while pos < end:
        assert pos % 2 == 0 and pos + 8 <= end, (path, pos)
        cid, size = struct.unpack_from("<4sI", data, pos)
        assert pos + 8 + size <= end, (path, cid, size)
        if cid in (b"RIFF", b"LIST"):
            kind = data[pos + 8:pos + 12]
            found.setdefault(path + (kind,), []).append((pos + 8, size))
            _walk(data, pos + 12, pos + 8 + size, path + (kind,), found)
        else:
            found.setdefault(path + (cid,), []).append((pos + 8, size))
        pos += 8 + size + (size & 1)
    assert pos == end or pos == end + 1, (path, pos, end)
    return found


@pytest.mark.parametrize("fps", [Fraction(30000, 1001), 25, 12.5])
def test_writer_layout(tmp_path, fps):
    rng = np.random.default_rng(3)
    frames = [V.smooth(rng, 36, 28) for _ in range(5)]
    path = str(tmp_path / "out.avi")
    want = J.encode_jpeg_batch_emulate(frames, quality=90, subsampling="4:2:2")
    with VideoWriter(path, fps, quality=90, subsampling="4:2:2", encode=J.encode_jpeg_batch_emulate) as w:
        w.write(frames[:2])
        w.write(np.stack(frames[2:]))                                      # a (B, H, W, 3) array as well as a list
        assert w.n_frames == 5
        with pytest.raises(ValueError, match="the frames of a video share one size"):
            w.write([frames[0][:, :-1]])
    data = open(path, "rb").read()
    assert any(len(f) & 1 for f in want) and any(not len(f) & 1 for f in want)
    found = _walk(data, 0, len(data), (), {})
    A = (b"AVI ",)
    assert found[A] == [(8, len(data) - 8)]                                # one RIFF chunk spanning the file
    assert sorted(k for k in found if len(k) == 2) == [A + (b"hdrl",), A + (b"idx1",), A + (b"movi",)]
    (avih_at, avih_n), = found[A + (b"hdrl", b"avih")]
    (strh_at, strh_n), = found[A + (b"hdrl", b"strl", b"strh")]
    (strf_at, strf_n), = found[A + (b"hdrl", b"strl", b"strf")]
    assert (avih_n, strh_n, strf_n) == (56, 56, 40)
    avih = struct.unpack_from("<14I", data, avih_at)
    strh = struct.unpack_from("<4s4sIHHIIIIIIIi4H", data, strh_at)
    strf = struct.unpack_from("<IiiHH4sIiiII", data, strf_at)
    chunks = found[A + (b"movi", b"00dc")]
    assert len(found[A + (b"movi",)]) == 1 and set(k[-1] for k in found if k[:2] == A + (b"movi",) and len(k) == 3) == {b"00dc"}
    assert avih[4] == strh[9] == len(chunks) == 5                          # dwTotalFrames == dwLength == the 00dc chunks
    assert [data[at:at + n] for at, n in chunks] == want
    assert avih[3] & 0x10 and avih[6] == 1 and (avih[8], avih[9]) == (36, 28)
    assert strh[0] == b"vids" and strh[1] == b"MJPG" and strf[5] == b"MJPG" and (strf[0], strf[1], strf[2]) == (40, 36, 28)
    assert Fraction(strh[7], strh[6]) == Fraction(fps)                     # dwRate / dwScale
    assert avih[0] == round(1000000 / Fraction(fps))
    assert avih[7] == strh[10] == max(len(f) for f in want)                # dwSuggestedBufferSize: the largest chunk
    (idx_at, idx_n), = found[A + (b"idx1",)]
    movi_fourcc_at = found[A + (b"movi",)][0][0]
    entries = list(struct.iter_unpack("<4sIII", data[idx_at:idx_at + idx_n]))
    assert len(entries) == 5
    for (cid, flags, off, size), (at, n) in zip(entries, chunks):
        assert cid == b"00dc" and flags & 0x10 and size == n
        assert movi_fourcc_at + off == at - 8 and data[at - 8:at - 4] == b"00dc"
    with VideoReader(path) as r:
        assert (r.width, r.height, r.fps, r.n_frames) == (36, 28, Fraction(fps), 5)
        assert [r.frame_bytes(i) for i in range(5)] == want
    for f in want:                                                         # the frames keep their Huffman tables
        assert len(V.dht_tables(f)) == 4


def test_writer_refuses_to_pass_two_gib(tmp_path, monkeypatch):
    from face_detection_and_recognition_amd.modules.utils import video as VID
    w = VideoWriter(str(tmp_path / "big.avi"), 25, encode=lambda frames, **kw: [b"\xff\xd8\xff\xd9"] * len(frames))
    w.write([np.zeros((8, 8, 3), np.uint8)])
    monkeypatch.setattr(VID, "AVI_MAX_BYTES", w._pos + 8 + 16 * 2 + 11)     # no room for one more 12-byte chunk and its index entry
    with pytest.raises(VideoUnsupported, match="2\\^31"):
        w.write([np.zeros((8, 8, 3), np.uint8)])
    w.close()
    with VideoReader(str(tmp_path / "big.avi")) as r:
        assert len(r) == 1


def test_empty_writer_gives_a_readable_file(tmp_path):
    VideoWriter(str(tmp_path / "none.avi"), 30, encode=J.encode_jpeg_batch_emulate).close()
    with VideoReader(str(tmp_path / "none.avi")) as r:
        assert len(r) == 0 and r.fps == 30


# ---- drivers -----------------------------------------------------------------------------------------------------------

def test_get_file_type():
    assert get_file_type("clip.avi") == "video" and get_file_type("cam.mjpeg") == "video" and get_file_type("CAM.MJPG") == "video"
    assert get_file_type("a/b/face.jpg") == "image" and get_file_type("0") == "camera" and get_file_type("notes.txt") is None


class _StubNet:
    accepts_device_frames = True

    def __init__(self, *a, **kw):
        self.args = a


@pytest.mark.parametrize("module", ["detect_face_blazeface", "detect_face_yolov5_face", "detect_face_mtcnn"])
def test_detect_scripts_send_a_video_to_inference_vid(module, monkeypatch, capsys):
    import importlib
    from face_detection_and_recognition_amd.modules.models.base import PostProcessedDetection
    mod = importlib.import_module("face_detection_and_recognition_amd." + module)
    calls = []

    def vid(net, path, save=None, anonymize=0, **kw):
        calls.append((type(net), path, save, anonymize))
        z = np.zeros((1, 4))
        return [PostProcessedDetection(z + k, np.ones(1), np.ones(1), np.zeros((1, 10))) for k in range(3)]

    def img(*a, **kw):
        raise AssertionError("a video went down the image path")
    monkeypatch.setattr(mod, "inference_vid", vid)
    for name in ("inference_img", "load_image"):
        if hasattr(mod, name):
            monkeypatch.setattr(mod, name, img)
    for name in ("BlazeFaceModel", "load_model"):
        if hasattr(mod, name):
            monkeypatch.setattr(mod, name, _StubNet)
    posts = mod.main(["-i", "x.avi", "-o", "y.avi", "--anonymize", "8", "--md", "weights.pth", "-d", "hip:0"])
    assert len(posts) == 3 and calls == [(_StubNet, "x.avi", "y.avi", 8)]
    import json
    lines = [json.loads(line) for line in capsys.readouterr().out.splitlines() if line.startswith("{")]
    assert [r["frame"] for r in lines] == [0, 1, 2] and lines[2]["boxes"] == [[2.0] * 4]


def test_tracker_driver_takes_exactly_one_source():
    from face_detection_and_recognition_amd.face_extraction import track_faces_in_frames as T
    a = T.get_parsed_args(["--frames", "dir", "--max_age", "5"])
    assert (a.frames_path, a.video_path, a.video_out) == ("dir", None, None)
    a = T.get_parsed_args(["--video", "clip.avi", "--max_age", "5", "--video_out", "o.avi"])
    assert (a.frames_path, a.video_path, a.video_out) == (None, "clip.avi", "o.avi")
    for argv in (["--max_age", "5"], ["--frames", "d", "--video", "v.avi", "--max_age", "5"]):
        with pytest.raises(SystemExit):
            T.get_parsed_args(argv)


def test_eval_driver_takes_video_avi_in_place_of_frames(tmp_path):
    from face_detection_and_recognition_amd.eval.eval_face_tracker import load_sequences
    seq = tmp_path / "seq1"
    seq.mkdir()
    (seq / "gt.txt").write_text("1,1,2,3,10,10,1,-1,-1,-1\n5,1,2,3,10,10,1,-1,-1,-1\n")
    (seq / "video.avi").write_bytes(_avi())
    s, = load_sequences(str(tmp_path))
    assert s["n_frames"] == 5 and isinstance(s["frames"], VideoReader) and s["frames"].frame_bytes(4) == FRAMES[3]
    from face_detection_and_recognition_amd.eval.eval_face_tracker import close_sequences
    close_sequences([s])
    with pytest.raises(Exception):
        s["frames"].frame_bytes(0)                                         # the mapping is closed
