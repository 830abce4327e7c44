"""Huffman decoding of sequential JPEG scans on the device (csrc/jpegdec.hip, ABI 12; modules/utils/jpeg.py entropy="device").

Pin: the host decoder fp_jpeg_entropy_decode (csrc/jpeg.hip), itself byte-identical to libjpeg-turbo (tests/test_jpeg.py).
  CPU:  fp_jpeg_scan_prepare's scope; the fp_jpeg_scan layout against a C compiler; the SOS over-read reproducer; the device
        algorithm run serially on the CPU (fp_jpeg_entropy_decode_emulate) against the host decoder, status and every coefficient,
        on clean and damaged files at three subsequence lengths; a slice of the sanitizer fuzzer of the same comparison.
  GPU:  fp_jpeg_entropy_decode_device against the host decoder on mixed batches and damaged files; the host fallback; pixels
        and embeddings through entropy="device" against entropy="host" and Pillow."""
import ctypes
import io
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from face_detection_and_recognition_amd import _lib as L
from oracle import jpeg_ref
from test_jpeg import BASELINE, JDIR, SYNTH, _host_decode, _synthetic

SEQUENTIAL = BASELINE[:3]
ON_HOST = L.JPEG_DECODE_ON_HOST


def _buf(data):
    return (ctypes.c_uint8 * max(1, len(data))).from_buffer_copy(data) if data else (ctypes.c_uint8 * 1)()


def _prepare(lib, data):
    info, scan = L.FpJpegInfo(), L.FpJpegScan()
    rc = lib.fp_jpeg_scan_prepare(_buf(data), len(data), ctypes.byref(info), ctypes.byref(scan))
    return rc, info, scan


def _emulate(lib, data, sub_bits, max_rounds=8):
    rc, info, scan = _prepare(lib, data)
    if rc:
        return rc, None, 0
    coefs = np.zeros(int(scan.n_coefs), np.int16)
    rounds = ctypes.c_int32()
    rc = lib.fp_jpeg_entropy_decode_emulate(_buf(data), len(data), ctypes.byref(scan), coefs.ctypes.data_as(ctypes.c_void_p),
                                            sub_bits, max_rounds, ctypes.byref(rounds))
    return rc, coefs, rounds.value


def _fixture(name):
    return open(os.path.join(JDIR, name), "rb").read()


def _sos(data):
    p = 2
    while not (data[p] == 0xFF and data[p + 1] == 0xDA):
        p += 2 + (data[p + 2] << 8 | data[p + 3])
    return p


def _second_scan(data):
    """A sequential file with a second (one-component) scan spliced in behind its first, in front of EOI."""
    assert data[-2:] == b"\xff\xd9"
    cid = data[_sos(data) + 5]
    return data[:-2] + bytes([0xFF, 0xDA, 0, 8, 1, cid, 0, 0, 63, 0]) + bytes(40) + b"\xff\xd9"


def _damaged(good, rng):
    """test_jpeg_refusals_and_damaged_input's recipes on a sequential file: cuts, noise in the scan, a third of the file."""
    out = [good[:len(good) // 2], good[:len(good) - 3], good[:700], good[:len(good) // 3]]
    for _ in range(4):
        noisy = bytearray(good)
        for i in rng.integers(700, len(good) - 2, 40):
            noisy[int(i)] = int(rng.integers(0, 256))
        out.append(bytes(noisy))
    return out


def _corpus(rng, frames=True):
    """Sequential files of every layout the device path takes: the fixtures, SYNTH's sequential entries, 576 x 1024 q90 4:2:0
    frames, q100, a flat image (long EOB runs), restart intervals of 1 and 3 MCUs, gray, 1 x 1."""
    files = [_fixture(n) for n in SEQUENTIAL]
    files += [_synthetic(rng, w, h, **dict(kw)) for w, h, kw in SYNTH if not kw.get("progressive")]
    from PIL import Image
    b = io.BytesIO()
    Image.new("RGB", (200, 120), (90, 140, 200)).save(b, "JPEG", quality=85)
    files.append(b.getvalue())                                                   # flat
    files += [_synthetic(rng, 160, 96, quality=100, subsampling=2), _synthetic(rng, 160, 96, quality=100, subsampling=0),
              _synthetic(rng, 120, 72, quality=90, restart_marker_blocks=1), _synthetic(rng, 120, 72, quality=90, subsampling=1,
                                                                                        restart_marker_blocks=3),
              _synthetic(rng, 90, 50, quality=80, gray=True, restart_marker_blocks=1), _synthetic(rng, 1, 1, quality=90, gray=True)]
    if frames:
        files += [_synthetic(rng, 1024, 576, quality=90, subsampling=2) for _ in range(2)]
    return files


# ---------------------------------------------------------------------------------------------------------------------- CPU


def test_scan_prepare_takes_sequential_interleaved_scans_only(lib):
    """fp_jpeg_scan_prepare takes the three sequential fixtures and fills the descriptor like fp_jpeg_parse; it refuses the
    progressive fixture, CMYK and a first scan that names one of three components with FP_ERR_UNSUPPORTED.  A second scan
    spliced in behind the first passes prepare (it does not read the scan data): the emulator leaves that file to the host."""
    for name in SEQUENTIAL:
        data = _fixture(name)
        rc, info, scan = _prepare(lib, data)
        assert rc == 0, name
        ref = L.FpJpegInfo()
        assert lib.fp_jpeg_parse(_buf(data), len(data), ctypes.byref(ref)) == 0
        assert bytes(info) == bytes(ref)
        assert scan.data_off == _sos(data) + 2 + (data[_sos(data) + 2] << 8 | data[_sos(data) + 3])
        assert scan.data_len == len(data) - scan.data_off and scan.n_coefs == info.n_coefs
        assert (scan.mcux, scan.mcuy, scan.blocks_per_mcu, scan.ncomp) == (info.mcux, info.mcuy, 6, 3)
        assert list(scan.slot_comp[:6]) == [0, 0, 0, 0, 1, 2] and list(scan.slot_dy[:4]) == [0, 0, 1, 1]
    assert _prepare(lib, _fixture(BASELINE[3]))[0] == -3
    from PIL import Image
    b = io.BytesIO()
    Image.new("CMYK", (32, 32)).save(b, "JPEG")
    assert _prepare(lib, b.getvalue())[0] == -3
    good = _fixture(SEQUENTIAL[2])
    p = _sos(good)
    one = good[:p + 2] + bytes([0, 8, 1]) + good[p + 5:p + 7] + bytes([0, 63, 0]) + good[p + 12:]   # first scan: component 1 only
    assert _host_decode(lib, one)[0] in (0, -1)
    assert _prepare(lib, one)[0] == -3
    two = _second_scan(good)
    assert _prepare(lib, two)[0] == 0
    assert _host_decode(lib, two)[0] == 0
    for sub_bits in (32, 1024):
        assert _emulate(lib, two, sub_bits)[0] == ON_HOST


def test_scan_descriptor_layout_matches_a_c_compiler(tmp_path):
    """The ctypes mirror of fp_jpeg_scan / fp_jpeg_huff agrees with a C99 compiler on the size and every field offset."""
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/lib/llvm/bin/clang") if shutil.which(c)), None)
    if cc is None:
        pytest.skip("no C compiler")
    fields = [f for f, _ in L.FpJpegScan._fields_]
    hfields = [f for f, _ in L.FpJpegHuff._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "facepath.h"', "int main(void) {",
           '  printf("%zu %zu\\n", sizeof(fp_jpeg_scan), sizeof(fp_jpeg_huff));']
    src += [f'  printf("%zu\\n", offsetof(fp_jpeg_scan, {f}));' for f in fields]
    src += [f'  printf("%zu\\n", offsetof(fp_jpeg_huff, {f}));' for f in hfields]
    src += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.run([cc, "-std=c99", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")],
                   check=True)
    out = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()
    sizes, offs = [int(v) for v in out[:2]], [int(v) for v in out[2:]]
    assert sizes == [ctypes.sizeof(L.FpJpegScan), ctypes.sizeof(L.FpJpegHuff)]
    assert offs == [getattr(L.FpJpegScan, f).offset for f in fields] + [getattr(L.FpJpegHuff, f).offset for f in hfields]


def test_sos_header_cut_after_its_length_is_refused_by_both_host_entries(lib):
    """ADVICE r4's reproducer: a fixture cut at its SOS + ff da 00 02 (an SOS segment with an empty body).  read_sos checks the
    length before it reads the component count: FP_ERR_INVALID_ARG from fp_jpeg_entropy_decode and fp_jpeg_scan_prepare (the
    sanitizer fuzzer runs the same file in an exact-size block)."""
    good = _fixture(SEQUENTIAL[0])
    bad = good[:_sos(good)] + b"\xff\xda\x00\x02"
    assert _host_decode(lib, bad)[0] == -1
    assert _prepare(lib, bad)[0] == -1


def test_emulator_equals_host_decoder(lib):
    """fp_jpeg_entropy_decode_emulate (the device phases run serially on the CPU, same per-lane source) == fp_jpeg_entropy_decode:
    status and every coefficient, at subsequence lengths of 32, 64 and 1024 bits, on clean files of every layout and on damaged
    ones.  At 1024 bits every file is decided (no host fallback); short subsequences may leave a large frame to the host."""
    rng = np.random.default_rng(11)
    files = _corpus(rng)
    damaged = [d for f in files[:3] + files[-2:-1] for d in _damaged(f, rng)]
    decided = 0
    for sub_bits in (32, 64, 1024):
        for i, data in enumerate(files + damaged):
            big = len(data) > 50_000
            if big and sub_bits == 32 and i >= len(files):
                continue                                       # (time: the damaged frames run at 64 and 1024 bits)
            rh, _, ch = _host_decode(lib, data)
            re, ce, _ = _emulate(lib, data, sub_bits, 16)
            if re == ON_HOST:
                assert sub_bits < 1024 or i >= len(files), (sub_bits, i)
                continue
            decided += 1
            assert re == rh, (sub_bits, i, re, rh)
            if rh == 0 or ch is not None:
                np.testing.assert_array_equal(ce, ch, err_msg=str((sub_bits, i)))
    assert decided > 2 * (len(files) + len(damaged))
    # a cap of one round: what the speculative pass did not get right goes to the host
    frame = files[-1]
    assert _emulate(lib, frame, 1024, 1)[0] == ON_HOST
    rc, ce, rounds = _emulate(lib, frame, 1024, 8)
    assert rc == 0 and 2 <= rounds <= 8
    np.testing.assert_array_equal(ce, _host_decode(lib, frame)[2])


def test_device_decoder_mutation_fuzz_under_asan_ubsan(tmp_path):
    """tools/fuzz/run_jpeg_device_fuzz.sh: the emulator against the host decoder on truncated / bit-flipped / marker-spliced
    variants of 38 small files (4:4:4 / 4:2:2 / 4:2:0 / gray, restart intervals of 1-3 MCUs) at 32-bit subsequences (every file
    crosses many subsequence boundaries), built with AddressSanitizer + UndefinedBehaviorSanitizer, plus the SOS over-read
    reproducer as a fixed seed and every seed with restart markers again with 0xff fill bytes in front of each RSTn (the host
    decodes it to the same coefficients, the emulator hands it to the host or agrees): no difference, no sanitizer report."""
    if not (os.path.exists("/opt/rocm/bin/hipcc") and os.path.exists("/opt/rocm/lib/llvm/bin/clang++") and shutil.which("nm")):
        pytest.skip("needs hipcc + clang++ + nm")
    env = dict(os.environ, FUZZ_BUILD_DIR=str(tmp_path))
    r = subprocess.run([os.path.join(ROOT, "tools", "fuzz", "run_jpeg_device_fuzz.sh"), "1000", "3", "32", "64"], capture_output=True,
                       text=True, timeout=900, env=env)
    report = "Sanitizer" in r.stderr or "runtime error" in r.stderr or "MISMATCH" in r.stderr or "fixed" in r.stderr
    if r.returncode != 0 and not report and "fuzz.o" not in r.stderr:
        pytest.skip("the sanitizer build of the fuzzer did not come up here: " + r.stderr[-300:])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    words = r.stdout.strip().splitlines()[-1].split()
    n, taken, host, equal = int(words[0]), int(words[2]), int(words[8]), int(words[13])
    assert n >= 38_000 and taken > n // 2 and host < taken // 4 and equal == n - host, r.stdout


# ---------------------------------------------------------------------------------------------------------------------- GPU


def _device_vs_host(lib, dev, files, sub_bits=1024, max_rounds=8):
    from face_detection_and_recognition_amd.modules.utils import jpeg as J
    res = J.device_entropy_decode(files, dev, sub_bits, max_rounds)
    host = 0
    for i, (data, r) in enumerate(zip(files, res)):
        rh, _, ch = _host_decode(lib, data)
        if r is None:
            host += 1
            continue
        if isinstance(r, int):
            assert rh == r == -1, (i, rh, r)
            continue
        assert rh == 0, (i, rh)
        np.testing.assert_array_equal(r[1].cpu().numpy(), ch, err_msg=str(i))
    return res, host


@pytest.mark.gpu
def test_device_entropy_decode_equals_host_on_mixed_batches(dev, lib):
    """fp_jpeg_entropy_decode_device == fp_jpeg_entropy_decode, status and every coefficient: the corpus of every layout in one
    batch of mixed sizes (every file decided on the device), 256 frames of 576 x 1024 q90 4:2:0, 1024 small crops."""
    rng = np.random.default_rng(12)
    files = _corpus(rng)
    res, host = _device_vs_host(lib, dev, files)
    assert host == 0 and all(isinstance(r, tuple) for r in res)
    frames = [_synthetic(rng, 1024, 576, quality=90, subsampling=2) for _ in range(8)] * 32
    res, host = _device_vs_host(lib, dev, frames)
    assert host == 0
    crops = [_synthetic(rng, int(w), int(h), quality=90, subsampling=2) for w, h in rng.integers(24, 140, (64, 2))] * 16
    res, host = _device_vs_host(lib, dev, crops)
    assert host == 0


@pytest.mark.gpu
def test_device_entropy_decode_damaged_files(dev, lib):
    """The damaged-file recipes (cuts, noise in the scan, a third of the file) of three files: the device's status equals the
    host decoder's for every file it decides, coefficients included, at 1024- and 64-bit subsequences."""
    rng = np.random.default_rng(13)
    files = [d for f in [_fixture(n) for n in SEQUENTIAL] + [_synthetic(rng, 300, 200, quality=90, restart_marker_blocks=2)]
             for d in _damaged(f, rng)]
    for sub_bits in (1024, 64):
        res, host = _device_vs_host(lib, dev, files, sub_bits, 16)
        assert host < len(files) // 2
        assert any(r == -1 for r in res)


@pytest.mark.gpu
def test_device_entropy_forced_fallback(dev, monkeypatch):
    """A round cap of 1 leaves the large frames to the host: decode_jpeg_batch(entropy="device") still returns Pillow's frames."""
    from face_detection_and_recognition_amd.modules.utils import jpeg as J
    rng = np.random.default_rng(14)
    files = [_synthetic(rng, 1024, 576, quality=90, subsampling=2) for _ in range(3)] + [_fixture(SEQUENTIAL[0])]
    assert any(r is None for r in J.device_entropy_decode(files, dev, 1024, 1))
    monkeypatch.setattr(J, "DEVICE_MAX_ROUNDS", 1)
    outs = J.decode_jpeg_batch(files, dev, bgr=False, entropy="device")
    for data, o in zip(files, outs):
        np.testing.assert_array_equal(o.cpu().numpy(), jpeg_ref.decode_pil(data))


@pytest.mark.gpu
def test_device_entropy_pixels_and_fallbacks(dev, tmp_path):
    """decode_jpeg_batch / decode_jpeg / imread_batch with entropy="device" == entropy="host" == Pillow: sequential fixtures and
    synthetic files, progressive files and a spliced second scan in the same batch (host path), progressive and PNG files in an
    imread_batch list; CMYK raises JpegUnsupported from decode_jpeg_batch as before; a damaged file raises what the host raises."""
    from PIL import Image

    from face_detection_and_recognition_amd import _lib
    from face_detection_and_recognition_amd.modules.utils import jpeg as J
    from face_detection_and_recognition_amd.modules.utils.inference import load_image
    rng = np.random.default_rng(15)
    files = [_fixture(n) for n in BASELINE] + [_synthetic(rng, w, h, **dict(kw)) for w, h, kw in SYNTH[::3]]
    files.append(_second_scan(_fixture(SEQUENTIAL[1])))
    got = J.decode_jpeg_batch(files, dev, bgr=False, entropy="device")
    ref = J.decode_jpeg_batch(files, dev, bgr=False)
    for i, (data, a, b) in enumerate(zip(files, got, ref)):
        np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy(), err_msg=str(i))
        if i < len(files) - 1:                           # (libjpeg-turbo refuses the spliced scan: host path only)
            np.testing.assert_array_equal(a.cpu().numpy(), jpeg_ref.decode_pil(data), err_msg=str(i))
    np.testing.assert_array_equal(J.decode_jpeg(files[0], dev, entropy="device").cpu().numpy(),
                                  J.decode_jpeg(files[0], dev).cpu().numpy())
    cmyk = io.BytesIO()
    Image.new("CMYK", (32, 32)).save(cmyk, "JPEG")
    with pytest.raises(J.JpegUnsupported):
        J.decode_jpeg_batch([files[0], cmyk.getvalue()], dev, entropy="device")
    cut = files[0][:len(files[0]) // 3]
    rc = _host_decode(L.load(), cut)[0]
    if rc:
        with pytest.raises(_lib.FacepathError):
            J.decode_jpeg_batch([files[1], cut], dev, entropy="device")
    paths = []
    for i, data in enumerate(files[:6]):
        paths.append(str(tmp_path / f"f{i}.jpg"))
        open(paths[-1], "wb").write(data)
    png = str(tmp_path / "x.png")
    Image.fromarray(np.arange(24 * 16 * 3, dtype=np.uint8).reshape(24, 16, 3)).save(png)
    cm = str(tmp_path / "cmyk.jpg")
    open(cm, "wb").write(cmyk.getvalue())
    paths += [png, cm]
    got = J.imread_batch(paths, dev, entropy="device")
    ref = J.imread_batch(paths, dev)
    assert isinstance(got, list) and len(got) == len(paths)
    for p, a, b in zip(paths, got, ref):
        np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy(), err_msg=p)
        np.testing.assert_array_equal(a.cpu().numpy(), load_image(p), err_msg=p)
    same = [paths[0]] * 3
    stacked = J.imread_batch(same, dev, entropy="device")
    assert isinstance(stacked, torch.Tensor) and torch.equal(stacked, J.imread_batch(same, dev))


@pytest.mark.gpu
def test_embed_images_device_entropy_is_bitwise_equal(dev, tmp_path):
    """similar_face_filtering embed_images(entropy="device") == entropy="host", bit for bit (same decoded pixels)."""
    from PIL import Image

    from face_detection_and_recognition_amd.modules.mobile_facenet.mobile_facenet import MobileFaceNet
    from face_detection_and_recognition_amd.similar_face_filtering import filter_faces_using_reference as F
    from face_detection_and_recognition_amd.synth import synth_state_dict
    net = MobileFaceNet(512)
    net.load_state_dict(synth_state_dict(net.state_dict(), 300))
    net = net.to(dev)
    rng = np.random.default_rng(16)
    paths = []
    for i in range(6):
        img = np.clip(np.cumsum(rng.normal(0, 6, (80 + 8 * i, 72, 3)), 0) + 128, 0, 255).astype(np.uint8)
        paths.append(str(tmp_path / f"c{i}.jpg"))
        Image.fromarray(img).save(paths[-1], quality=90)
    a = F.embed_images(net, paths, 4, entropy="device").cpu().numpy()
    b = F.embed_images(net, paths, 4).cpu().numpy()
    np.testing.assert_array_equal(a, b)
