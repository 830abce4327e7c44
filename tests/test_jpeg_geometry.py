"""JPEG decode at the geometries and stream structures where a decoder goes wrong unnoticed (csrc/jpeg.hip, csrc/jpegdec.hip,
oracle/jpeg_ref.py): narrow images and fill bytes.

Pin: libjpeg-turbo through Pillow on the bytes under test (oracle/jpeg_ref.decode_pil).  Everything is byte-for-byte equality.
  * jdsample.c jinit_upsampler takes the fancy (triangle) chroma filters only for downsampled_width > 2: a chroma plane 1 or 2
    samples wide is replicated, across and down.  tests/test_jpeg.py's sizes never had such a plane on the h2v2 path.
  * JPEG B.1.1.2: any marker may be preceded by any number of 0xff fill bytes -- in front of an RSTn inside a scan too.
  CPU:  the host half (fp_jpeg_parse / fp_jpeg_entropy_decode) + the oracle restatement against Pillow over a grid of sizes,
        subsamplings, modes and contents; the oracle's upsampler choice; structural variants (fill bytes, optimised tables,
        restart rows, custom 8- and 16-bit quantisation tables, quality 1 / 100, garbage behind EOI); the device Huffman
        emulator on the narrow and fill-byte files; committed narrow fixtures with recorded hashes (tests/golden/jpeg/narrow,
        tools/gen_golden.py jpeg_narrow: Pillow output of synthetic arrays).
  GPU:  decode_jpeg_batch over the grid and the fixtures; entropy="device" over its sequential files and the fill-byte files."""
import functools
import hashlib
import io
import json
import os

import numpy as np
import pytest

from conftest import ROOT
from face_detection_and_recognition_amd import _lib as L
from oracle import jpeg_ref
from test_jpeg import _host_decode, _synthetic
from test_jpeg_device_entropy import _emulate

NDIR = os.path.join(ROOT, "tests", "golden", "jpeg", "narrow")
NARROW = json.load(open(os.path.join(NDIR, "expected.json")))
ON_HOST = L.JPEG_DECODE_ON_HOST

WIDTHS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 33)
HEIGHTS = (1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 33)
GPU_WIDTHS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17)
GPU_HEIGHTS = (1, 2, 3, 8, 9, 17)
SUBS = (0, 1, 2, "gray")                 # Pillow's numbering: 4:4:4, 4:2:2, 4:2:0; a one-component file
MODES = ("seq", "prog", "rst1")          # sequential, progressive, sequential with a restart interval of 1 MCU
CONTENTS = ("smooth", "noise")           # noise makes neighbouring chroma samples differ: a smooth image can hide a wrong filter


def _encode(img, sub, **kw):
    from PIL import Image
    b = io.BytesIO()
    if sub == "gray":
        Image.fromarray(np.ascontiguousarray(img[..., 0])).save(b, "JPEG", **kw)
    else:
        Image.fromarray(img).save(b, "JPEG", subsampling=sub, **kw)
    return b.getvalue()


def _noise(rng, w, h):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _grid_file(w, h, sub, mode, content):
    """One file of the grid (the same bytes for every test that asks: the generator is seeded by the case)."""
    rng = np.random.default_rng([w, h, SUBS.index(sub), MODES.index(mode), CONTENTS.index(content)])
    kw = dict(quality=90, progressive=mode == "prog")
    if mode == "rst1":
        kw["restart_marker_blocks"] = 1
    if content == "noise":
        return _encode(_noise(rng, w, h), sub, **kw)
    if sub == "gray":
        return _synthetic(rng, w, h, gray=True, **kw)
    return _synthetic(rng, w, h, subsampling=sub, **kw)


@functools.lru_cache(maxsize=None)
def _pil(data):
    a = jpeg_ref.decode_pil(data)
    a.setflags(write=False)
    return a


def _grid(widths=WIDTHS, heights=HEIGHTS, modes=MODES, contents=CONTENTS):
    return [(w, h, sub, mode, content) for w in widths for h in heights for sub in SUBS for mode in modes for content in contents]


def _report(bad, total):
    """The failing cases, short enough to read: how many, at which widths, the first few."""
    return f"{len(bad)} of {total} differ; widths {sorted({b[0][0] for b in bad})}; first: {bad[:12]}"


# ---- stream surgery ------------------------------------------------------------------------------------------------------


def _markers(data):
    """(offset of the 0xff, code) of every marker of a well-formed file, RSTn inside the scans included."""
    out, p = [(0, 0xD8)], 2
    while p + 1 < len(data):
        assert data[p] == 0xFF, p
        m = data[p + 1]
        out.append((p, m))
        if m == 0xD9:
            break
        p += 2 + (data[p + 2] << 8 | data[p + 3])
        if m == 0xDA:                                  # entropy-coded data: up to the next marker that is not an RSTn
            while True:
                p = data.index(b"\xff", p)
                m = data[p + 1]
                if m == 0:
                    p += 2
                elif 0xD0 <= m <= 0xD7:
                    out.append((p, m))
                    p += 2
                else:
                    break
    return out


def _with_fill(data, n, codes):
    """n 0xff fill bytes in front of every marker whose code is in `codes`; returns the file and how many markers got them."""
    out, last, hits = [], 0, 0
    for p, m in _markers(data):
        if m in codes:
            out.append(data[last:p] + b"\xff" * n)
            last = p
            hits += 1
    return b"".join(out) + data[last:], hits


RST = tuple(range(0xD0, 0xD8))


@functools.lru_cache(maxsize=None)
def _fill_rst_files():
    """Fill bytes (1, 2 and 7) in front of every RSTn: 4:4:4 / 4:2:0 / gray, restart intervals of 1 and 3 MCUs, sequential and
    progressive, 45 x 37 noise.  [(case, file)]."""
    out = []
    for sub in (0, 2, "gray"):
        for interval in (1, 3):
            for prog in (False, True):
                rng = np.random.default_rng([7, SUBS.index(sub), interval, int(prog)])
                clean = _encode(_noise(rng, 45, 37), sub, quality=90, progressive=prog, restart_marker_blocks=interval)
                for n in (1, 2, 7):
                    data, hits = _with_fill(clean, n, RST)
                    assert hits >= 2 and len(data) == len(clean) + n * hits
                    assert _pil(data).tobytes() == _pil(clean).tobytes()       # fill bytes change nothing for libjpeg
                    out.append(((sub, interval, prog, n), data))
    return out


def _check_vs_pillow(lib, data):
    rc, info, coefs = _host_decode(lib, data)
    if rc:
        return f"rc {rc}"
    got = jpeg_ref.reconstruct(info, coefs)
    ref = _pil(data)
    if got.shape != ref.shape:
        return f"shape {got.shape} vs {ref.shape}"
    if not np.array_equal(got, ref):
        return f"max |diff| {int(np.abs(got.astype(int) - ref.astype(int)).max())}"
    return None


# ---- CPU -----------------------------------------------------------------------------------------------------------------


def test_geometry_sweep_host_half_and_oracle_vs_pillow(lib):
    """Widths 1-9, 15, 16, 17, 33 x heights 1-4, 7, 8, 9, 15, 16, 17, 33 x 4:4:4 / 4:2:2 / 4:2:0 / gray x sequential /
    progressive / restart interval 1 x smooth / noise content, quality 90 (3432 files, every one compared):
    oracle reconstruct(fp_jpeg_entropy_decode) == Pillow's decode of the same bytes.  With the fancy upsampler applied to chroma
    planes 1 or 2 samples wide (the decoder and oracle before jinit_upsampler's rule went in) 4:2:2 differed at widths 3 and 4,
    4:2:0 at widths 1-4, by up to 97 grey levels; widths >= 5, 4:4:4 and gray were exact (this grid: 331 of 3432 differed)."""
    cases = _grid()
    bad = []
    for case in cases:
        why = _check_vs_pillow(lib, _grid_file(*case))
        if why:
            bad.append((case, why))
    assert len(cases) == len(WIDTHS) * len(HEIGHTS) * 4 * 3 * 2
    assert not bad, _report(bad, len(cases))


def test_oracle_takes_the_librarys_upsampler_choice(lib):
    """jinit_upsampler: fancy only for downsampled_width > 2.  Chroma widths 1, 2 (replication) and 3 (fancy), h2v1 and h2v2,
    noise at heights 1, 2 and 16, each against Pillow; and the branch itself: _upsample replicates at chroma widths 1 and 2 and
    does not at 3.  On the oracle that special-cased only cw == 1 on the h2v1 path this failed at chroma width 2 for h2v1
    (image widths 3, 4) and at chroma widths 1 and 2 for h2v2 (image widths 1-4, every height but 1 and 2 at widths 1 and 2);
    chroma width 3 passed (28 of the 72 files differed, image widths 1-4)."""
    bad, n = [], 0
    for cw in (1, 2, 3):
        for w in (2 * cw - 1, 2 * cw):
            for sub in (1, 2):
                for h in (1, 2, 16):
                    for mode in ("seq", "prog"):
                        why = _check_vs_pillow(lib, _grid_file(w, h, sub, mode, "noise"))
                        n += 1
                        if why:
                            bad.append(((w, h, sub, mode), why))
    assert not bad, _report(bad, n)
    rng = np.random.default_rng(3)
    for v2 in (False, True):
        for cw in (1, 2, 3):
            p = rng.integers(0, 256, (5, cw), dtype=np.uint8)
            up = jpeg_ref._upsample(p, v2)
            rep = np.repeat(np.repeat(p, 2 if v2 else 1, axis=0), 2, axis=1)
            assert up.shape == rep.shape
            assert np.array_equal(up, rep) == (cw <= 2), (v2, cw)


def _variants():
    """(name, file): the structural variants next to the RSTn fill bytes."""
    rng = np.random.default_rng(21)
    img = _noise(rng, 45, 37)
    out = []
    for sub in (0, 2, "gray"):
        for prog in (False, True):
            clean = _encode(img, sub, quality=85, progressive=prog)
            for name, codes in (("SOS", (0xDA,)), ("DHT", (0xC4,)), ("EOI", (0xD9,))):
                data, hits = _with_fill(clean, 3, codes)
                assert hits >= 1
                out.append((f"fill before {name} {sub} prog={prog}", data))
            out.append((f"optimize {sub} prog={prog}", _encode(img, sub, quality=85, progressive=prog, optimize=True)))
    for sub in (0, 1, 2, "gray"):
        out.append((f"restart rows {sub}", _encode(img, sub, quality=85, restart_marker_rows=1)))
    q8 = [[int(v) for v in rng.integers(1, 256, 64)] for _ in range(2)]
    q16 = [[int(v) for v in rng.integers(1, 1024, 64)] for _ in range(2)]
    q16[0][5] = q16[1][9] = 1000                                    # (certainly a 16-bit table)
    for sub in (0, 2):
        out.append((f"qtables 8-bit {sub}", _encode(img, sub, qtables=q8)))
        d = _encode(img, sub, qtables=q16)
        dqt = [p for p, m in _markers(d) if m == 0xDB]
        assert any(d[p + 4] >> 4 == 1 for p in dqt), "Pillow wrote no 16-bit table"
        out.append((f"qtables 16-bit {sub}", d))
    out.append(("quality 1", _encode(img, 0, quality=1)))
    out.append(("quality 100", _encode(img, 0, quality=100)))
    out.append(("garbage behind EOI", _encode(img, 2, quality=85) + bytes(int(v) for v in rng.integers(0, 256, 256))))
    return out


def test_structural_variants_vs_pillow(lib):
    """Files libjpeg decodes and nothing pinned: 1, 2 and 7 fill bytes in front of every RSTn (4:4:4 / 4:2:0 / gray, restart
    intervals 1 and 3, sequential and progressive); fill bytes in front of SOS, DHT and EOI; optimised Huffman tables;
    restart_marker_rows=1; custom 8-bit and 16-bit quantisation tables; quality 1 and 100 at 4:4:4; 256 bytes of garbage behind
    EOI.  Each: rc 0 and oracle reconstruct(host decode) == Pillow.  (The RSTn fill-byte files returned FP_ERR_INVALID_ARG while
    BitReader::fill took ff ff dn for the marker 0xff; the others were equal to Pillow before too.)"""
    files = [(f"fill before RSTn {c}", d) for c, d in _fill_rst_files()] + _variants()
    bad = [(name, why) for name, why in ((name, _check_vs_pillow(lib, d)) for name, d in files) if why]
    assert not bad, f"{len(bad)} of {len(files)}: {bad[:12]}"


def test_emulator_on_narrow_and_fill_byte_files(lib):
    """fp_jpeg_entropy_decode_emulate (the device Huffman phases, serially) at 32- and 1024-bit subsequences on the sequential
    files of the sweep with width <= 9 and on the sequential RSTn fill-byte files: status 0 and the host decoder's exact
    coefficients, or FP_JPEG_DECODE_ON_HOST.  The narrow files have no fill bytes: every one is decided.  The fill-byte files are
    handed to the host (jd_unstuff ends the device attempt at 0xff 0xff: kTermHost), never refused and never decoded differently."""
    narrow = [c for c in _grid(widths=tuple(w for w in WIDTHS if w <= 9), modes=("seq", "rst1"))]
    fills = [d for (sub, interval, prog, n), d in _fill_rst_files() if not prog]
    assert len(narrow) == 9 * len(HEIGHTS) * 4 * 2 * 2 and len(fills) == 18
    for sub_bits in (32, 1024):
        for case in narrow:
            data = _grid_file(*case)
            rh, _, ch = _host_decode(lib, data)
            re, ce, _ = _emulate(lib, data, sub_bits, 64)
            assert rh == 0 and re == 0, (sub_bits, case, rh, re)
            np.testing.assert_array_equal(ce, ch, err_msg=str((sub_bits, case)))
        for i, data in enumerate(fills):
            rh, _, ch = _host_decode(lib, data)
            re, ce, _ = _emulate(lib, data, sub_bits, 64)
            assert rh == 0 and re in (0, ON_HOST), (sub_bits, i, rh, re)
            if re == 0:
                np.testing.assert_array_equal(ce, ch, err_msg=str((sub_bits, i)))


def _narrow(name):
    return open(os.path.join(NDIR, name), "rb").read()


def test_pillow_still_decodes_the_narrow_fixtures_as_recorded():
    """The pin, independent of the Pillow of the box: widths 1-5 at 4:2:2 and 4:2:0, a progressive, a gray and a fill-byte file
    (Pillow output of synthetic arrays) decode to the recorded bytes.  If this fails the library under the oracle changed."""
    assert len(NARROW) >= 13
    for name, exp in NARROW.items():
        a = jpeg_ref.decode_pil(_narrow(name))
        assert list(a.shape) == exp["shape"] and hashlib.sha256(a.tobytes()).hexdigest() == exp["sha256_rgb"], name


def test_host_half_and_oracle_on_the_narrow_fixtures(lib):
    """oracle reconstruct(fp_jpeg_entropy_decode) of every narrow fixture has the recorded hash."""
    for name, exp in NARROW.items():
        rc, info, coefs = _host_decode(lib, _narrow(name))
        assert rc == 0, (name, rc)
        got = jpeg_ref.reconstruct(info, coefs)
        assert list(got.shape) == exp["shape"] and hashlib.sha256(got.tobytes()).hexdigest() == exp["sha256_rgb"], name


# ---- GPU -----------------------------------------------------------------------------------------------------------------


def _gpu_grid(modes=MODES):
    return _grid(widths=GPU_WIDTHS, heights=GPU_HEIGHTS, modes=modes, contents=("noise",))


@pytest.mark.gpu
def test_device_reconstruction_over_the_geometry_grid(dev, lib):
    """decode_jpeg_batch (host Huffman, device IDCT + upsampling + colour) over widths 1-9, 16, 17 x heights 1, 2, 3, 8, 9, 17 x
    every subsampling and mode, noise content (792 files, in batches of 128): every frame == Pillow == the oracle restatement;
    BGR on every seventh file; the committed narrow fixtures against their recorded hashes."""
    from face_detection_and_recognition_amd.modules.utils import jpeg as J
    cases = _gpu_grid()
    assert len(cases) == len(GPU_WIDTHS) * len(GPU_HEIGHTS) * 4 * 3
    files = [_grid_file(*c) for c in cases]
    bad = []
    for b0 in range(0, len(files), 128):
        outs = [o.cpu().numpy() for o in J.decode_jpeg_batch(files[b0:b0 + 128], dev, bgr=False)]
        for case, data, got in zip(cases[b0:], files[b0:b0 + 128], outs):
            rc, info, coefs = _host_decode(lib, data)
            assert rc == 0, case
            ref = _pil(data)
            if got.shape != ref.shape or not np.array_equal(got, ref) or not np.array_equal(got, jpeg_ref.reconstruct(info, coefs)):
                bad.append((case, "differs"))
    assert not bad, _report(bad, len(cases))
    sub = files[::7]
    for data, o in zip(sub, J.decode_jpeg_batch(sub, dev, bgr=True)):
        np.testing.assert_array_equal(o.cpu().numpy()[..., ::-1], _pil(data))
    names = sorted(NARROW)
    for name, o in zip(names, J.decode_jpeg_batch([_narrow(n) for n in names], dev, bgr=False)):
        a = o.cpu().numpy()
        assert list(a.shape) == NARROW[name]["shape"] and hashlib.sha256(a.tobytes()).hexdigest() == NARROW[name]["sha256_rgb"], name


@pytest.mark.gpu
def test_device_entropy_on_narrow_and_fill_byte_files(dev, lib, tmp_path):
    """entropy="device" on the sequential files of the GPU grid, the sequential RSTn fill-byte files and the fill-byte fixture,
    in ONE batch with a 64 x 48 and a 576 x 1024 file, through decode_jpeg_batch and imread_batch: every frame == the
    host-entropy result == Pillow.  device_entropy_decode gives a tuple or None for the fill-byte files (None: the device hands
    a scan with 0xff 0xff in it to the host), never FP_ERR_INVALID_ARG; a tuple's coefficients are the host decoder's."""
    from face_detection_and_recognition_amd.modules.utils import jpeg as J
    rng = np.random.default_rng(31)
    fills = [d for (sub, interval, prog, n), d in _fill_rst_files() if not prog]
    fills += [_narrow(n) for n in sorted(NARROW) if "fill" in n]
    assert len(fills) == 19
    files = [_grid_file(*c) for c in _gpu_grid(("seq", "rst1"))]
    files += fills + [_synthetic(rng, 64, 48, quality=85, subsampling=2), _synthetic(rng, 1024, 576, quality=90, subsampling=2)]
    res = J.device_entropy_decode(fills, dev)
    for i, (data, r) in enumerate(zip(fills, res)):
        assert r is None or isinstance(r, tuple), (i, r)
        if r is not None:
            rh, _, ch = _host_decode(lib, data)
            assert rh == 0
            np.testing.assert_array_equal(r[1].cpu().numpy(), ch, err_msg=str(i))
    got = J.decode_jpeg_batch(files, dev, bgr=False, entropy="device")
    ref = J.decode_jpeg_batch(files, dev, bgr=False)
    paths = []
    for i, data in enumerate(files):
        paths.append(str(tmp_path / f"f{i:04d}.jpg"))
        with open(paths[-1], "wb") as f:
            f.write(data)
    read = J.imread_batch(paths, dev, bgr=False, entropy="device")
    assert len(got) == len(ref) == len(read) == len(files)
    for i, (data, a, b, c) in enumerate(zip(files, got, ref, read)):
        a = a.cpu().numpy()
        np.testing.assert_array_equal(a, b.cpu().numpy(), err_msg=str(i))
        np.testing.assert_array_equal(a, c.cpu().numpy(), err_msg=str(i))
        np.testing.assert_array_equal(a, _pil(data), err_msg=str(i))
