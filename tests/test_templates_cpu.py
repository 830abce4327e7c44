"""Templates on the host: track_pool_numpy (numpy float32) against track_pool_emulate (fp_track_pool_step_emulate, the kernel's
own tests and arithmetic on host memory) on every case of template_cases.py -- every bit of the three per-row outputs and the
three table arrays --, each case's own expectation, the properties (a step split anywhere, scattered rows), the tracker's cases
with a template table behind them, the constructed benefit, the refusals of both entry points, and header against binding.
No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import reid_cases as RC
import template_cases as PC
import track_cases as TC
from face_detection_and_recognition_amd import _lib as L
from face_detection_and_recognition_amd import tracking as T

SIZES = PC.width_length_cases()
CRAFTED = PC.crafted_cases()


@pytest.mark.parametrize("case", SIZES + CRAFTED, ids=[c["name"] for c in SIZES + CRAFTED])
def test_case_numpy_equals_emulator(case, lib):
    want = PC.run_case(case, T.track_pool_numpy)
    if case["expect"]:
        case["expect"](*want)
    PC.assert_same(PC.run_case(case, T.track_pool_emulate), want, case["name"])


@pytest.mark.parametrize("D", PC.CRAFTED_DIMS)
def test_scattered_equals_ordered(D, lib):
    case = PC.scattered(D)
    for fn in (T.track_pool_numpy, T.track_pool_emulate):
        (mixed,), t_mixed = PC.run_case(case, fn)
        (ordered,), t_ordered = PC.run_case(case["ordered"], fn)
        for key in T.TEMPLATE_OUT_KEYS:
            assert np.array_equal(PC.int_view(mixed[key]), PC.int_view(ordered[key][case["perm"]])), key
        PC.assert_same_table(t_mixed, t_ordered, "scattered")


@pytest.mark.parametrize("D", PC.CRAFTED_DIMS)
def test_a_step_equals_its_parts(D, lib):
    """18 frames (6 of each of three streams) in one call, as 9 + 9 (3 + 3 per stream) and as 3 + 15 (1 + 5), state carried."""
    case = PC.busy(D)
    (whole,), table = PC.run_case(case, T.track_pool_numpy)
    assert (whole["track_emb_flags"] & T.TPL_RESTART).any() and (whole["track_emb_rows"] > 1).any()
    for fn in (T.track_pool_numpy, T.track_pool_emulate):
        for k in (9, 3, 0, 18):
            two, rows = PC.split_case(case, k)
            outs, t = PC.run_case(two, fn)
            for part, r in zip(outs, rows):
                for key in T.TEMPLATE_OUT_KEYS:
                    assert np.array_equal(PC.int_view(part[key]), PC.int_view(whole[key][r])), (k, key)
            PC.assert_same_table(t, table, f"split at {k}")


def pool_behind(case, track_fn, pool_fn, reid, motion, weighted):
    """The case through track_fn (RC.run_case), each step's results through pool_fn on one table -> (pool outs, table, track
    outs)."""
    table = T.new_template_state(case["S"], case["D"])
    keep = case["reid"].lost_age if reid else case["max_age"]
    touts = RC.run_case(case, track_fn, reid=reid, motion=motion)[0]
    outs = [pool_fn(table, st["frame"], st["emb"], st["xinv"], st["stream_of_frame"], o["track_id"], o["track_clock"],
                    o["track_flags"], keep, weight=st["score"] if weighted else None) for st, o in zip(case["steps"], touts)]
    return outs, table, touts


TRACKED = RC.track_cases_in_every_configuration() + RC.crafted_cases() + [RC.busy(D) for D in RC.DIMS]


@pytest.mark.parametrize("case", TRACKED, ids=[c["name"] for c in TRACKED])
def test_behind_the_tracker_numpy_equals_emulator(case, lib):
    """The tracker's own cases (track_cases.py, reid_cases.py) with reid and motion on, the emulator's per-row results handed to
    both restatements of the pool, unweighted and weighted by the score."""
    for weighted in (False, True):
        if weighted and case["steps"][0]["score"] is None:
            continue
        a = pool_behind(case, T.track_step_emulate, T.track_pool_numpy, True, True, weighted)
        b = pool_behind(case, T.track_step_emulate, T.track_pool_emulate, True, True, weighted)
        PC.assert_same(b[:2], a[:2], case["name"])


def test_a_revived_row_continues_its_template(lib):
    """The revolving door: A's sixth row is REVIVED under its old id, 12 frames after its fifth; keep = lost_age, so its template
    is still there and goes on (6 rows, no RESTART).  Without the pool the face comes back as a NEW id and a new template."""
    case = next(c for c in RC.crafted_cases() if c["name"] == "door-D32")
    (out,), table, (tout,) = pool_behind(case, T.track_step_emulate, T.track_pool_numpy, True, False, False)
    a = np.nonzero(tout["track_id"] == 2)[0]
    assert tout["track_flags"][a[5]] == T.REVIVED
    assert out["track_emb_rows"][a].tolist() == list(range(1, 11)) and not out["track_emb_flags"].any()
    (out,), table, (tout,) = pool_behind(case, T.track_step_emulate, T.track_pool_numpy, False, False, False)
    a4 = np.nonzero(tout["track_id"] == 4)[0]
    assert out["track_emb_rows"][a4].tolist() == list(range(1, 6)) and not out["track_emb_flags"].any()


def test_constructed_benefit():
    """The figures written into template_cases.py: at least 10 % of the rows are named wrongly one by one, no track from its
    pooled sum."""
    row_rate, track_rate = PC.benefit_rates()
    assert (row_rate, track_rate) == (PC.ROW_ERROR_RATE, PC.TRACK_ERROR_RATE)
    assert row_rate >= 0.10 and track_rate == 0.0


def test_python_argument_checks():
    t = T.new_template_state(1, 8)
    z = np.zeros((0,), np.int32)
    args = (z, np.zeros((0, 8), np.float32), np.zeros((0,), np.float32), z, z, z, z)
    for fn in (T.track_pool_numpy, T.track_pool_emulate):
        assert fn(t, *args, 3)["track_emb"].shape == (0, 8)
        for keep in (-1, 1.5, True):
            with pytest.raises(ValueError):
                fn(t, *args, keep)
        with pytest.raises(ValueError):
            fn(dict(t, tpl_w=t["tpl_w"].astype(np.float64)), *args, 3)
        with pytest.raises(ValueError):
            fn(dict(t, tpl_i=t["tpl_i"][:, :64]), *args, 3)
    assert repr(T.Templates(weighted=True)) == "Templates(weighted=True)" and T.Templates().weighted is False
    assert T.POOL == T.SLOTS + T.LOST == 128
    book = T.TrackBook()
    out = dict(track_id=np.array([3, 0, 3]), track_hits=np.array([1, 0, 2]), track_clock=np.array([1, 1, 2]),
               track_flags=np.array([T.NEW | T.BEST, T.DEAD_ROW, 0]))
    temb = np.arange(12, dtype=np.float32).reshape(3, 4)
    book.update(out, np.array([0, 0, 1]), np.zeros((3, 4), np.float32), np.zeros((2,), np.int32), track_emb=temb,
                track_emb_rows=np.array([1, 0, 2]))
    assert book[(0, 3)]["template"].tolist() == temb[2].tolist() and book[(0, 3)]["template_rows"] == 2
    plain = T.TrackBook()
    plain.update(out, np.array([0, 0, 1]), np.zeros((3, 4), np.float32), np.zeros((2,), np.int32))
    assert "template" not in plain[(0, 3)]


def test_header_and_binding_agree(lib):
    from conftest import ROOT
    hdr = open(os.path.join(ROOT, "include", "facepath.h")).read()
    assert f"#define FP_TRACK_POOL {L.TRACK_POOL}\n" in hdr and L.TRACK_POOL == 128 == L.TRACK_SLOTS + L.TRACK_LOST
    assert f"#define FP_TRACK_TPL_EVICTED {L.TRACK_TPL_EVICTED}\n" in hdr and L.TRACK_TPL_EVICTED == 1 == T.TPL_EVICTED
    assert f"#define FP_TRACK_TPL_RESTART {L.TRACK_TPL_RESTART}\n" in hdr and L.TRACK_TPL_RESTART == 2 == T.TPL_RESTART
    assert "#define FP_ABI_VERSION 15\n" in hdr and L.ABI_VERSION == 15 == lib.fp_abi_version()
    n_args = {}
    for fn in ("fp_track_pool_step", "fp_track_pool_step_emulate", "fp_track_pool_workspace_bytes"):
        decl = re.search(r"\n(?:int|size_t) " + fn + r"\(([^;]*)\);", hdr).group(1)
        n_args[fn] = len([a for a in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",") if a.strip()])
        assert n_args[fn] == len(L.SIGNATURES[fn][1]), fn
    assert n_args["fp_track_pool_step"] == n_args["fp_track_pool_step_emulate"] + 3 == 20
    fields = re.search(r"typedef struct fp_track_templates \{(.*?)\} fp_track_templates;", hdr, re.S).group(1)
    assert re.findall(r"\*\s*(\w+);", fields) == [f[0] for f in L.FpTrackTemplates._fields_] == list(T.TEMPLATE_KEYS)
    assert "Tracklets: templates" in hdr
    for doc in ("INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "fp_track_pool_step" in text and "Tracklets: templates" in text, doc
    assert lib.fp_track_pool_workspace_bytes(0) == 16 and lib.fp_track_pool_workspace_bytes(-1) == 0
    assert lib.fp_track_pool_workspace_bytes(1000) >= 1000 * 44


def test_refusals_before_any_launch(lib):
    """Both entry points refuse every invalid argument with FP_ERR_INVALID_ARG before they touch a pointer (the device entry
    point before any HIP call: this runs without a GPU); n == 0 is FP_OK on both, B == 0 with rows passes every row through."""
    P = ctypes.c_void_p(4096)          # 16-byte aligned, never dereferenced: every call that uses it is refused first
    odd = ctypes.c_void_p(4096 + 4)

    def call(device, tpl="ok", S=2, D=8, frame=P, emb=P, xinv=P, weight=None, n=5, sof=P, B=3, ids=P, clocks=P, flags=P, keep=2,
             temb=P, trows=P, tflags=P, ws=P, ws_bytes=1 << 20, tsum=P, ti=P, tw=P):
        st = None if tpl is None else ctypes.byref(L.FpTrackTemplates(ti, tw, tsum))
        args = (st, S, D, frame, emb, xinv, weight, n, sof, B, ids, clocks, flags, keep, temb, trows, tflags)
        if device:
            return lib.fp_track_pool_step(*args, ws, ws_bytes, None)
        return lib.fp_track_pool_step_emulate(*args)

    bad = [dict(tpl=None), dict(ti=None), dict(tw=None), dict(tsum=None), dict(S=0), dict(D=6), dict(D=0), dict(D=2),
           dict(D=L.TRACK_MAX_DIM + 4), dict(keep=-1), dict(n=-1), dict(B=-1), dict(sof=None), dict(frame=None), dict(emb=None),
           dict(xinv=None), dict(ids=None), dict(clocks=None), dict(flags=None), dict(temb=None), dict(trows=None),
           dict(tflags=None), dict(emb=odd), dict(tsum=odd), dict(temb=odd)]
    for device in (False, True):
        for kw in bad:
            assert call(device, **kw) == L.FP_ERR_INVALID_ARG, (device, kw)
        assert call(device, n=0) == L.FP_OK and call(device, n=0, B=0, sof=None) == L.FP_OK
        assert call(device, n=0, frame=None, emb=None, xinv=None, ids=None, clocks=None, flags=None, temb=None, trows=None,
                    tflags=None, ws=None, ws_bytes=0) == L.FP_OK
    for kw in (dict(ws=None), dict(ws_bytes=5 * 44), dict(ws=ctypes.c_void_p(4097))):
        assert call(True, **kw) == L.FP_ERR_INVALID_ARG, kw
    # B == 0 with rows: nothing has a stream
    t = T.new_template_state(1, 8)
    emb = np.arange(24, dtype=np.float32).reshape(3, 8)
    out = T.track_pool_emulate(t, [0, 1, 2], emb, [1, 1, 1], [], [1, 2, 3], [1, 1, 1], [T.NEW] * 3, 2)
    assert out["track_emb"].tobytes() == emb.tobytes() and not out["track_emb_rows"].any() and not t["tpl_i"].any()
