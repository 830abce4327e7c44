"""Reduced-size JPEG decode and EXIF orientation, the parts that need no GPU (csrc/jpegscale.hip's host emulator,
fp_jpeg_exif_orientation, modules/utils/jpeg.py's keywords).

Pin: libjpeg-turbo through Pillow -- Image.draft(mode, (w // s, h // s)) makes the library decode at scale 1 / s, the same
scale_denom cv2.imread's IMREAD_REDUCED_COLOR_2 / _4 / _8 hand it; ImageOps.exif_transpose is the orientation cv2.imread applies.
tests/jpeg_scaled_cases.py holds the case list and a numpy restatement of the library's procedure."""
import ctypes
import io
import struct

import numpy as np
import pytest

import jpeg_scaled_cases as J
from oracle import jpeg_ref


def _rgb3(a):
    return np.repeat(a, 3, axis=2) if a.shape[2] == 1 else a


@pytest.mark.parametrize("size", J.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_scaled_decode_equals_pillow_draft(lib, size):
    """For every case of this size and s in 2, 4, 8 with min(w, h) >= s: Pillow takes the scale (asserted through its output
    size, ceil(w / s) x ceil(h / s)), and the numpy restatement and the host emulator (fp_jpeg_reconstruct_scaled_emulate: the
    device's own __host__ __device__ arithmetic, run serially) each equal its RGB decode byte for byte; the restatement's Y / Cb / Cr
    samples equal Pillow's draft("YCbCr") decode, which is returned unconverted.  For min(w, h) < s Pillow cannot be steered to
    the scale (its rule is min(w // rw, h // rh)): there the emulator is compared with the numpy restatement only, and parity with
    libjpeg is NOT pinned for those sizes.  At s = 1 the emulator equals Pillow's plain decode (the 8 x 8 path of the new kernels)."""
    n_pinned = 0
    for name, w, h, data in J.case_list():
        if (w, h) != size:
            continue
        info, coefs = J.host_decode(data)
        np.testing.assert_array_equal(J.emulate(info, coefs, 1), jpeg_ref.decode_pil(data), err_msg=name)
        for s in J.SCALES:
            ycc = J.scaled_ycc(info, coefs, s)
            rgb = J.ycc_to_rgb(ycc)
            em = J.emulate(info, coefs, s)
            assert em.shape == (-(-h // s), -(-w // s), 3), (name, s)
            np.testing.assert_array_equal(em, rgb, err_msg=f"{name} s={s}: emulator vs restatement")
            if min(w, h) < s:
                continue
            pil, took = J.pil_draft(data, s, "RGB")
            assert took == (-(-w // s), -(-h // s)), (name, s, took)          # Pillow decoded at 1 / s, nothing else
            np.testing.assert_array_equal(rgb, _rgb3(pil), err_msg=f"{name} s={s}: restatement vs Pillow")
            np.testing.assert_array_equal(em, _rgb3(pil), err_msg=f"{name} s={s}: emulator vs Pillow")
            pycc, took = J.pil_draft(data, s, "YCbCr")
            assert took == (-(-w // s), -(-h // s))
            np.testing.assert_array_equal(ycc, pycc, err_msg=f"{name} s={s}: Y / Cb / Cr vs Pillow")
            n_pinned += 1
    assert n_pinned or min(size) < 2


def test_emulator_bgr_and_argument_checks(lib):
    """bgr swaps the first and third byte; scale_denom outside 1 / 2 / 4 / 8 and tags outside 1 .. 8 are refused
    (FP_ERR_INVALID_ARG), a short workspace with FP_ERR_BOUNDS; the ABI number is unchanged."""
    assert lib.fp_abi_version() == 15
    _, w, h, data = next(c for c in J.case_list() if c[0].startswith("67x45-sub2-q92"))
    info, coefs = J.host_decode(data)
    np.testing.assert_array_equal(J.emulate(info, coefs, 4, 6, bgr=True), J.emulate(info, coefs, 4, 6)[..., ::-1])
    oh, ow = ctypes.c_int(), ctypes.c_int()
    for s, tag in ((3, 1), (0, 1), (16, 1), (2, 0), (2, 9)):
        assert lib.fp_jpeg_scaled_size(ctypes.byref(info), s, tag, ctypes.byref(oh), ctypes.byref(ow)) == -1
    assert lib.fp_jpeg_scaled_workspace_bytes(ctypes.byref(info), 3) == 0
    assert lib.fp_jpeg_scaled_size(ctypes.byref(info), 8, 6, ctypes.byref(oh), ctypes.byref(ow)) == 0
    assert (oh.value, ow.value) == (9, 6)                                      # ceil(67 / 8) rows, ceil(45 / 8) columns
    nws = int(lib.fp_jpeg_scaled_workspace_bytes(ctypes.byref(info), 2))
    ws, out = np.zeros(nws, np.uint8), np.zeros((23, 34, 3), np.uint8)
    args = (coefs.ctypes.data_as(ctypes.c_void_p), ctypes.byref(info), 2, 1, ws.ctypes.data_as(ctypes.c_void_p))
    assert lib.fp_jpeg_reconstruct_scaled_emulate(*args, nws, out.ctypes.data_as(ctypes.c_void_p), 0) == 0
    assert lib.fp_jpeg_reconstruct_scaled_emulate(*args, 64, out.ctypes.data_as(ctypes.c_void_p), 0) == -2      # FP_ERR_BOUNDS


# ---- the orientation tag ---------------------------------------------------------------------------------------------

def _tagged(tag, big_endian=False, w=67, h=45, seed=3):
    rng = np.random.default_rng(seed)
    return J.encode(J._smooth(rng, w, h), quality=90, subsampling=2, exif=J.exif_bytes(tag, big_endian))


def _app1(data):
    """(offset of the APP1 marker, offset behind the segment) of the file's Exif segment."""
    p = 2
    while data[p + 1] != 0xe1:
        p += 2 + struct.unpack_from(">H", data, p + 2)[0]
    return p, p + 2 + struct.unpack_from(">H", data, p + 2)[0]


@pytest.mark.parametrize("big_endian", [False, True], ids=["II", "MM"])
def test_exif_orientation_reads_the_tag(lib, big_endian):
    """All eight tags in both byte orders, in files Pillow wrote with save(exif=...): fp_jpeg_exif_orientation returns what
    Pillow's getexif() reads.  No Exif segment, and tag values 0 and 9: 1."""
    from PIL import Image
    for tag in range(1, 9):
        data = _tagged(tag, big_endian)
        assert Image.open(io.BytesIO(data)).getexif().get(0x0112) == tag
        assert J.exif_orientation(data) == tag
    for tag in (0, 9, 0xffff):
        assert J.exif_orientation(_tagged(tag, big_endian)) == 1
    plain = J.encode(J._smooth(np.random.default_rng(3), 67, 45), quality=90)
    assert J.exif_orientation(plain) == 1
    assert J.exif_orientation(b"") == 1 and J.exif_orientation(b"\xff\xd8") == 1 and J.exif_orientation(b"\x89PNG\r\n\x1a\n" + bytes(32)) == 1


@pytest.mark.parametrize("big_endian", [False, True], ids=["II", "MM"])
def test_exif_orientation_on_damaged_segments(lib, big_endian):
    """Damaged input returns 1 and is read inside its bounds; every input here sits in an exact-size heap block (a ctypes copy), as
    the sanitizer harness under tools/fuzz holds it.  The file cut at every length up to the end of the APP1 segment; the segment
    itself shortened to every length (its length field rewritten, the rest of the file behind it): 1 until the tag's IFD entry lies
    wholly inside; an IFD offset past the end; an entry count that overruns the segment; a wrong type; a count other than 1."""
    data = _tagged(6, big_endian)
    a, e = _app1(data)
    assert J.exif_orientation(data) == 6
    for cut in range(0, e):
        assert J.exif_orientation(data[:cut]) == 1, cut
    assert J.exif_orientation(data[:e]) == 6                         # the whole segment is there
    body = data[a + 4:e]                                             # "Exif\0\0" + TIFF
    entry_end = 6 + 8 + 2 + 12
    for n in range(0, len(body)):
        short = data[:a + 2] + struct.pack(">H", n + 2) + body[:n] + data[e:]
        got = J.exif_orientation(short)
        assert got == (6 if n >= entry_end else 1), n
    o = "<" if not big_endian else ">"
    t = a + 10                                                       # the TIFF header's offset in the file

    def patched(off, fmt, v):
        b = bytearray(data)
        struct.pack_into(o + fmt, b, t + off, v)
        return bytes(b)
    ifd, = struct.unpack_from(o + "I", data, t + 4)
    assert ifd == 8 and struct.unpack_from(o + "H", data, t + ifd)[0] == 1
    tn = e - t
    for bad in (tn - 1, tn, tn + 1, 0x7fffffff, 0xffffffff, 0xfffffff0):
        assert J.exif_orientation(patched(4, "I", bad)) == 1, bad   # IFD offset at / past the end
    for cnt in (2, 3, 1000, 0xffff):
        assert J.exif_orientation(patched(ifd, "H", cnt)) == 1, cnt  # the entries would run past the segment
    assert J.exif_orientation(patched(ifd, "H", 0)) == 1
    assert J.exif_orientation(patched(ifd + 2 + 2, "H", 4)) == 1     # type LONG
    assert J.exif_orientation(patched(ifd + 2 + 4, "I", 2)) == 1     # two values
    assert J.exif_orientation(patched(0, "H", 0x4949 if big_endian else 0x4d4d)) == 1   # byte-order mark against the magic


@pytest.mark.parametrize("wh", [(67, 45), (1, 1), (1, 7), (7, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_emulator_orientation_equals_exif_transpose(lib, wh):
    """The emulator's output for the file's own tag equals ImageOps.exif_transpose of Pillow's decode, for all eight tags; at
    67 x 45 also at 1 / 2 and 1 / 4 size (orientation after scaling).  The decoder's table, restated in numpy, agrees too."""
    from PIL import Image, ImageOps
    w, h = wh
    for tag in range(1, 9):
        data = _tagged(tag, tag & 1 == 0, w, h)
        info, coefs = J.host_decode(data)
        assert J.exif_orientation(data) == tag
        for s in (1, 2, 4) if wh == (67, 45) else (1,):
            im = Image.open(io.BytesIO(data))
            if s > 1:
                im.draft("RGB", (w // s, h // s))
                assert im.size == (-(-w // s), -(-h // s))
            want = np.asarray(ImageOps.exif_transpose(im).convert("RGB"))
            got = J.emulate(info, coefs, s, tag)
            np.testing.assert_array_equal(got, want, err_msg=f"tag {tag} s={s}")
            np.testing.assert_array_equal(got, J.orient(J.emulate(info, coefs, s, 1), tag))


# ---- the Python surface ----------------------------------------------------------------------------------------------

def _png(path, w, h, tag=None, seed=0):
    from PIL import Image
    img = J._smooth(np.random.default_rng(seed), w, h)
    kw = {} if tag is None else {"exif": J.exif_bytes(tag)}
    Image.fromarray(img).save(path, "PNG", **kw)
    return img


def test_reduce_and_orientation_keywords_on_the_host_paths(lib, tmp_path):
    """A reduce outside 1, 2, 4, 8 raises ValueError from every entry point (before any device work); a non-JPEG file with
    reduce > 1 raises ValueError (cv2 resizes those); the Pillow fallback applies exif_transpose when orientation is on and
    draft() for a JPEG the decoder does not take (CMYK); load_image's host path does the same; imread_batch stacks by the OUTPUT
    shapes."""
    import torch
    from PIL import Image, ImageOps
    from face_detection_and_recognition_amd.modules.utils import jpeg as JP
    from face_detection_and_recognition_amd.modules.utils.inference import load_image
    data = _tagged(6)
    jp = str(tmp_path / "a.jpg")
    open(jp, "wb").write(data)
    info, coefs = J.host_decode(data)
    for bad in (0, 3, 16, -2, True, 2.5, "2"):
        for call in (lambda: JP.decode_jpeg(data, "cuda", reduce=bad), lambda: JP.decode_jpeg_batch([data], "cuda", reduce=bad),
                     lambda: JP.imread(jp, "cuda", reduce=bad), lambda: JP.imread_batch([jp], "cuda", reduce=bad),
                     lambda: JP.reconstruct(info, None, "cuda", reduce=bad), lambda: load_image(jp, None, reduce=bad),
                     lambda: JP.scaled_size(info, bad)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        JP.reconstruct(info, None, "cuda", orientation=9)
    assert JP.exif_orientation(data) == 6 and JP.scaled_size(info, 4, 6) == (17, 12) and JP.scaled_size(info, 4) == (12, 17)
    # non-JPEG files: the fallback, with the tag applied or not
    p6, p1 = str(tmp_path / "six.png"), str(tmp_path / "one.png")
    img6, img1 = _png(p6, 9, 5, 6, seed=1), _png(p1, 9, 5, None, seed=2)
    up = JP.imread(p6, "cpu", bgr=False)
    assert tuple(up.shape) == (9, 5, 3)
    np.testing.assert_array_equal(up.numpy(), np.asarray(ImageOps.exif_transpose(Image.open(p6)).convert("RGB")))
    np.testing.assert_array_equal(up.numpy(), J.orient(img6, 6))
    np.testing.assert_array_equal(JP.imread(p6, "cpu", bgr=True, orientation=False).numpy(), img6[..., ::-1])
    np.testing.assert_array_equal(load_image(p6), J.orient(img6, 6)[..., ::-1])
    np.testing.assert_array_equal(load_image(p6, orientation=False), img6[..., ::-1])
    for call in (lambda: JP.imread(p6, "cpu", reduce=2), lambda: load_image(p1, None, reduce=4), lambda: JP.imread_batch([p1, p6], "cpu", reduce=8)):
        with pytest.raises(ValueError):
            call()
    # stacking by output shape: tags 1 and 6 of one 9 x 5 size give 5 x 9 and 9 x 5 frames
    mixed = JP.imread_batch([p1, p6], "cpu", bgr=False)
    assert isinstance(mixed, list) and [tuple(f.shape) for f in mixed] == [(5, 9, 3), (9, 5, 3)]
    np.testing.assert_array_equal(mixed[0].numpy(), img1)
    np.testing.assert_array_equal(mixed[1].numpy(), J.orient(img6, 6))
    flat = JP.imread_batch([p1, p6], "cpu", bgr=False, orientation=False)
    assert isinstance(flat, torch.Tensor) and tuple(flat.shape) == (2, 5, 9, 3)
    np.testing.assert_array_equal(flat[1].numpy(), img6)
    # the host path of load_image on a JPEG: libjpeg's own reduced decode, then the tag
    im = Image.open(jp)
    im.draft("RGB", (67 // 2, 45 // 2))
    want = np.asarray(ImageOps.exif_transpose(im).convert("RGB"))
    assert want.shape == (34, 23, 3)
    np.testing.assert_array_equal(load_image(jp, None, reduce=2), want[..., ::-1])
    np.testing.assert_array_equal(load_image(jp, None, reduce=2)[..., ::-1], J.emulate(info, coefs, 2, 6))
    # a JPEG outside the decoder's scope (CMYK) through the fallback, reduced and turned
    b = io.BytesIO()
    Image.new("CMYK", (32, 16), (10, 200, 30, 40)).save(b, "JPEG", exif=J.exif_bytes(8))
    got = JP._pillow_decode(b.getvalue(), 4, True)
    assert got.shape == (8, 4, 3)
    assert JP._pillow_decode(b.getvalue(), 4, False).shape == (4, 8, 3)


def test_entry_points_take_reduce_and_ignore_orientation():
    """--reduce {1, 2, 4, 8} and --ignore_orientation on the three detector entry points and cluster_faces; the default applies
    the tag at full size; extract_faces_from_images, embed_images and inference_img take the keywords."""
    import inspect
    from face_detection_and_recognition_amd import detect_face_blazeface, detect_face_mtcnn, detect_face_yolov5_face
    from face_detection_and_recognition_amd.face_extraction import extract_faces_from_dataset as X
    from face_detection_and_recognition_amd.modules.utils import inference
    from face_detection_and_recognition_amd.modules.utils.parser import read_kwargs
    from face_detection_and_recognition_amd.similar_face_filtering import cluster_faces, filter_faces_using_reference
    for mod in (detect_face_blazeface, detect_face_mtcnn, detect_face_yolov5_face):
        p = mod.build_parser()
        assert read_kwargs(p.parse_args(["-i", "x.jpg"])) == dict(reduce=1, orientation=True)
        assert read_kwargs(p.parse_args(["-i", "x.jpg", "--reduce", "4", "--ignore_orientation"])) == dict(reduce=4, orientation=False)
        with pytest.raises(SystemExit):
            p.parse_args(["-i", "x.jpg", "--reduce", "3"])
    a = cluster_faces.get_parsed_args(["--ud", "x", "--reduce", "8"])
    assert a.reduce == 8 and a.ignore_orientation is False
    assert cluster_faces.get_parsed_args(["--ud", "x", "--ignore_orientation"]).reduce == 1
    for fn in (X.extract_faces_from_images, filter_faces_using_reference.embed_images, cluster_faces.image_quality,
               inference.inference_img, inference.load_image):
        sig = inspect.signature(fn).parameters
        assert sig["reduce"].default == 1 and sig["orientation"].default is True, fn
