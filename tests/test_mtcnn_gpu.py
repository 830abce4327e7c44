"""MTCNN on the GPU against the float64 restatement (tests/mtcnn_restatement.py): the nets alone, the resize / cut, the NMS,
every stage teacher-forced (nets, NMS and box arithmetic apart, then each stage kernel as a whole), determinism and the
whole cascade."""
import functools

import numpy as np
import pytest
import torch

import mtcnn_cases as C
import mtcnn_restatement as R
from conftest import rel_err
from face_detection_and_recognition_amd import synth
from face_detection_and_recognition_amd.frames import RaggedFrames
from face_detection_and_recognition_amd.modules.mtcnn.mtcnn import MTCNN, pnet_out
from face_detection_and_recognition_amd.plan import PlanBuilder

pytestmark = pytest.mark.gpu

# The project's bars for a net against float64 (tests/test_age_gender.py): logits and regressions 1e-4 relative,
# probabilities 1e-5 absolute.
REL, PROB_ABS = 1e-4, 1e-5
DEV_SCORE, DEV_COORD, FP32_UNMATCHED_SHARE = C.DEV_SCORE, C.DEV_COORD, C.FP32_UNMATCHED_SHARE


def gpu(net):
    import copy
    return copy.deepcopy(net).to("cuda")


def decode_cands(cand, n):
    """(n, 6) float32 records -> level, cell, score, reg."""
    c = cand[:n].cpu().numpy()
    key = c[:, 5].copy().view(np.uint32)
    return (key >> 24).astype(np.int64), (key & 0xFFFFFF).astype(np.int64), c[:, 4].astype(np.float64), c[:, :4].astype(np.float64)


@pytest.mark.parametrize("hw", [(37, 53), (64, 41), (90, 121)])
def test_pnet_maps_through_the_proposal_kernel(hw):
    """t1 = 0 emits every cell of every level: the probability and regression maps of P-Net on the kernel's own level
    images (area resize included), odd sizes included."""
    h, w = hw
    net = gpu(synth.synth_mtcnn(MTCNN(min_face_size=12, factor=0.709, cap=8192), 5, frame_hw=(64, 64)))
    frame = synth.synth_frames(1, h, w, 21)
    data, descs, sizes = net._as_ragged(frame, net._device())
    cand, counts, over = net.propose(data, descs, sizes, t1=0.0)
    n = int(counts[0])
    assert int(over[0]) == 0
    lvl, cell, score, reg = decode_cands(cand[0], n)
    sd = net.state_dict()
    pyr = R.pyramid(h, w, 12, 0.709)
    assert n == sum(pnet_out(lh) * pnet_out(lw) for _, lh, lw in pyr)
    for li, (s, lh, lw) in enumerate(pyr):
        p, r, _ = R.pnet(sd, R.normalise(R.resize_u8(frame[0], lh, lw))[None])
        sel = np.nonzero(lvl == li)[0]
        order = sel[np.argsort(cell[sel])]
        assert np.array_equal(cell[order], np.arange(p[0].size))
        err_p = np.abs(score[order] - p[0].ravel()).max()
        err_r = rel_err(reg[order], r[0].reshape(-1, 4))
        print(f"P-Net {hw} level {li} ({lh} x {lw}): prob abs {err_p:.2e}, reg rel {err_r:.2e}")
        assert err_p <= PROB_ABS and err_r <= REL


@pytest.mark.parametrize("x6", [True, False])
@pytest.mark.parametrize("name", ["rnet", "onet"])
def test_refine_nets(name, x6):
    saved = PlanBuilder.X6
    PlanBuilder.X6 = x6
    try:
        net = gpu(C.case("wide")[1])
        size = getattr(net, name).size
        x = np.random.default_rng(3).integers(0, 256, (48, size, size, 3), dtype=np.uint8)
        prob, logit, reg = net.run_net(name, torch.from_numpy(x))
        p, r, z = (R.rnet if name == "rnet" else R.onet)(net.state_dict(), R.normalise(x))
        errs = (np.abs(prob[:, 1].cpu().numpy() - p).max(), rel_err(logit[:, :2].cpu().numpy(), z),
                rel_err(reg[:, :r.shape[1]].cpu().numpy(), r))
        print(f"{name} x6={x6}: prob abs {errs[0]:.2e}, logits rel {errs[1]:.2e}, reg rel {errs[2]:.2e}")
        assert errs[0] <= PROB_ABS and errs[1] <= REL and errs[2] <= REL
    finally:
        PlanBuilder.X6 = saved


@pytest.mark.parametrize("size", [24, 48])
def test_cut_and_resize(size):
    """Area shrink, area-mode enlargement, mixed axes and boxes hanging over every edge: u8 identical to the restatement
    (both sides compute the mean in exact integer arithmetic, so a rounding tie is a tie on both)."""
    frames, net, _ = C.case("wide")
    net = gpu(net)
    h, w = frames.shape[1:3]
    boxes = [[10, 10, 100, 100], [-20, -15, 60, 70], [150, 100, 260, 200], [30, 40, 45, 52], [5, 5, 30, 90], [60, 20, 140, 35],
             [-5, 130, 40, 175], [200, 1, 223, 24], [1, 1, w, h], [100, 100, 100 + size - 1, 100 + size - 1], [-50, -50, -10, -10]]
    data, descs, sizes = net._as_ragged(frames[:2], net._device())
    bt = torch.zeros((2, 16, 4), dtype=torch.int32)
    bt[0, :len(boxes)] = torch.tensor(boxes, dtype=torch.int32)
    bt[1, :3] = torch.tensor(boxes[:3], dtype=torch.int32)
    bt = bt.cuda()
    offs = torch.tensor([0, len(boxes), len(boxes) + 3], dtype=torch.int32).cuda()
    n = len(boxes) + 3
    out = torch.empty((n, size, size, 4), dtype=torch.float32, device="cuda")
    out8 = torch.empty((n, size, size, 3), dtype=torch.uint8, device="cuda")
    net.cut(data, descs, 2, bt, offs, n, size, out, out8)
    got, gotf = out8.cpu().numpy(), out.cpu().numpy()
    todo = [(0, b) for b in boxes] + [(1, b) for b in boxes[:3]]
    for i, (f, b) in enumerate(todo):
        want = R.resize_u8(R.cut(frames[f], b), size, size)
        assert np.array_equal(got[i], want), (f, b, int((got[i] != want).sum()))
        assert np.array_equal(gotf[i, ..., :3], ((got[i].astype(np.float32) - 127.5) * 0.0078125)) and not gotf[i, ..., 3].any()


# ---- teacher forcing: every stage gets the restatement's candidates, and nets, NMS and box arithmetic are compared apart ----
# A decision is exempt only if the restatement's OWN float64 margin of that decision is below 8 x the fp32-vs-fp64 deviation
# of that quantity (tests/mtcnn_cases.py); everything else must be identical, and the exempt ones are counted against 5 % of
# the stage's candidates.
@functools.lru_cache(maxsize=None)
def _traces(name):
    frames, net, kw = C.case(name)
    sd = net.state_dict()
    out = []
    for frame in frames:
        tr = {}
        R.detect(frame, sd, trace=tr, **kw)
        out.append(tr)
    return out


def _f32(a):
    return np.asarray(a, np.float32)


@pytest.mark.parametrize("name", list(C.SETS))
def test_stage1_nets_on_the_test_sets(name):
    """(i) for stage 1: the level images + P-Net plans + threshold on the test frames, every cell (t1 = 0): probabilities and
    regressions meet the bars on every level, and p >= t1 agrees with the restatement cell by cell."""
    frames, net, kw = C.case(name)
    g = gpu(net)
    g.cap = 8192
    t1 = kw["thresholds"][0]
    data, descs, sizes = g._as_ragged(frames, g._device())
    cand, counts, over = g.propose(data, descs, sizes, t1=0.0)
    assert not over.any()
    sd = net.state_dict()
    exempt = passing = 0
    for f, frame in enumerate(frames):
        lvl, cell, score, reg = decode_cands(cand[f], int(counts[f]))
        for li, (s, lh, lw) in enumerate(R.pyramid(frame.shape[0], frame.shape[1], kw["min_face_size"], kw["factor"])):
            p, r, _ = R.pnet(sd, R.normalise(R.resize_u8(frame, lh, lw))[None])
            p, r = p[0].ravel(), r[0].reshape(-1, 4)
            sel = np.nonzero(lvl == li)[0]
            order = sel[np.argsort(cell[sel])]
            assert np.array_equal(cell[order], np.arange(p.size))
            assert np.abs(score[order] - p).max() <= PROB_ABS and rel_err(reg[order], r) <= REL, (name, f, li)
            differ = (score[order] >= np.float32(t1)) != (p >= t1)
            coin = np.abs(p - t1) < 8 * DEV_SCORE
            assert not (differ & ~coin).any(), (name, f, li)
            exempt += int((differ & coin).sum())
            passing += int((p >= t1).sum())
    assert exempt <= 0.05 * passing


@pytest.mark.parametrize("stage", [2, 3])
@pytest.mark.parametrize("name", list(C.SETS))
def test_refine_nets_on_the_restatements_candidates(name, stage):
    """(i) for stages 2 and 3: the restatement's candidates (frame, integer box) through the device's cut + resize and R-Net /
    O-Net: scores, regressions and landmarks meet the bars, and p >= t agrees candidate by candidate."""
    frames, net, kw = C.case(name)
    g = gpu(net)
    traces = _traces(name)
    src, dst, netname = ("s1", "s2", "rnet") if stage == 2 else ("s2", "s3", "onet")
    t = kw["thresholds"][stage - 1]
    B = len(frames)
    counts = np.asarray([len(tr[src]["boxes"]) for tr in traces], np.int32)
    boxes = np.zeros((B, int(counts.max()), 4), np.int32)
    for f, tr in enumerate(traces):
        boxes[f, :counts[f]] = tr[src]["boxes"]
    data, descs, sizes = g._as_ragged(frames, g._device())
    offs, plan = g._refine(netname, data, descs, B, torch.from_numpy(boxes).cuda(), counts, torch.from_numpy(counts).cuda())
    n = int(counts.sum())
    prob, reg = plan.prob[:n, 1].cpu().numpy(), plan.reg[:n].cpu().numpy()
    p = np.concatenate([tr[dst]["prob"] for tr in traces])
    r = np.concatenate([tr[dst]["reg"] for tr in traces])
    errs = np.abs(prob - p).max(), rel_err(reg[:, :4], r[:, :4]), (rel_err(reg[:, 4:14], r[:, 4:14]) if stage == 3 else 0.0)
    print(f"{name} {netname} on {n} candidates: prob abs {errs[0]:.2e}, reg rel {errs[1]:.2e}, landmarks rel {errs[2]:.2e}")
    assert errs[0] <= PROB_ABS and errs[1] <= REL and errs[2] <= REL
    differ = (prob >= np.float32(t)) != (p >= t)
    coin = np.abs(p - t) < 8 * DEV_SCORE
    assert not (differ & ~coin).any()
    assert (differ & coin).sum() <= 0.05 * n


@pytest.mark.parametrize("name", list(C.SETS))
def test_nms_of_every_stage_bit_exact(name):
    """(ii): the device NMS fed the restatement's own boxes and scores of each stage, rounded to fp32 -- per level (0.5, union),
    per frame (0.7, union), behind R-Net (0.7, union, integer boxes), behind O-Net (0.7, min, regressed float boxes) -- returns
    the identical keep list in the identical order (the expectation: the plain greedy loop in float64 on the same fp32 values)."""
    frames, net, kw = C.case(name)
    g = gpu(net)
    t2, t3 = kw["thresholds"][1:]
    jobs = {"level": ([], [], [0], 0.5, "union"), "frame": ([], [], [0], 0.7, "union"), "rnet": ([], [], [0], 0.7, "union"),
            "onet": ([], [], [0], 0.7, "min")}

    def add(kind, b, sc):
        bx, ss, seg = jobs[kind][:3]
        bx.append(_f32(b).reshape(-1, 4)); ss.append(_f32(sc)); seg.append(seg[-1] + len(sc))

    for tr in _traces(name):
        s1, s2, s3 = tr["s1"], tr["s2"], tr["s3"]
        for li in np.unique(s1["level"]):
            m = s1["level"] == li
            add("level", s1["q"][m], s1["score"][m])
        add("frame", s1["q"][s1["keep_level"]], s1["score"][s1["keep_level"]])
        add("rnet", s1["boxes"][s2["passed"]], s2["prob"][s2["passed"]])
        add("onet", s3["regressed"], s3["prob"][s3["passed"]])
    for kind, (bx, ss, seg, thr, mode) in jobs.items():
        q, sc, seg = np.concatenate(bx), np.concatenate(ss), np.asarray(seg, np.int32)
        keep, cnt = g.nms(torch.from_numpy(q).cuda(), torch.from_numpy(sc).cuda(), torch.from_numpy(seg).cuda(), thr, mode)
        keep, cnt = keep.cpu().numpy(), cnt.cpu().numpy()
        dropped = 0
        for s in range(len(seg) - 1):
            a, b = int(seg[s]), int(seg[s + 1])
            assert len(np.unique(sc[a:b])) == b - a
            want = a + R.nms(q[a:b].astype(np.float64), sc[a:b].astype(np.float64), thr, mode)
            assert cnt[s] == len(want) and np.array_equal(keep[a:a + cnt[s]], want), (kind, s)
            dropped += (b - a) - len(want)
        assert dropped > 0 or (kind == "frame" and name == "wide"), kind      # (factor 0.709: levels overlap by 0.5 at most)


@pytest.mark.parametrize("name", list(C.SETS))
def test_box_arithmetic_alone(name):
    """(iii): regress / square / truncate of stages 1 and 2 and regress + landmark mapping of stage 3 (fp_mtcnn_boxes: the
    device functions the stage kernels call), fed the restatement's KEPT boxes and regressions rounded to fp32, no NMS in front:
    identical integers -- a box is exempt only if one of its own coordinates lies within 8 x DEV_COORD of an integer before the
    truncation -- and floats within 1e-6 of each value's own magnitude."""
    frames, net, kw = C.case(name)
    g = gpu(net)
    exempt = total = 0
    for tr in _traces(name):
        s1, s2, s3 = tr["s1"], tr["s2"], tr["s3"]
        for mode, boxes, reg in ((1, s1["q"][s1["keep_frame"]], s1["reg"][s1["keep_frame"]]),
                                 (2, s1["boxes"][s2["keep"]], s2["reg"][s2["keep"]])):
            b32, r32 = _f32(boxes), _f32(reg)
            got = g.box_arithmetic(torch.from_numpy(b32).cuda(), torch.from_numpy(r32).cuda(), mode).cpu().numpy()
            pre = R.square(R.regress(b32.astype(np.float64), r32.astype(np.float64), 0.0 if mode == 1 else 1.0))
            bad = (got != np.trunc(pre)).any(1)
            coin = np.abs(pre - np.rint(pre)).min(1) < 8 * DEV_COORD
            assert not (bad & ~coin).any(), (name, mode)
            exempt += int((bad & coin).sum())
            total += len(pre)
        b32, r32 = _f32(s2["boxes"][s3["keep"]]), _f32(s3["reg"][s3["keep"]])
        got = g.box_arithmetic(torch.from_numpy(b32).cuda(), torch.from_numpy(r32).cuda(), 3).cpu().numpy().astype(np.float64)
        want = R.stage3_rows(b32.astype(np.float64), r32.astype(np.float64))
        assert (np.abs(got - want) <= 1e-6 * np.abs(want)).all(), name
    assert exempt <= 0.05 * total


def _exempt_boxes(got, n_got, pre, ok):
    """Device boxes of one frame against the restatement's kept boxes `pre` (before truncation; `ok`: the positive-side rule):
    the number of boxes that differ and are coin tosses by their own margin; any other difference fails."""
    want = np.trunc(pre)[ok].astype(np.int32)
    assert n_got == len(want)
    bad = (got[:n_got] != want).any(1)
    coin = (np.abs(pre - np.rint(pre)).min(1) < 8 * DEV_COORD)[ok]
    assert not (bad & ~coin).any()
    return int((bad & coin).sum())


@pytest.mark.parametrize("name", list(C.SETS))
def test_stage1_teacher_forced(name):
    """fp_mtcnn_stage1 as a whole, fed the restatement's candidates (scores and regressions rounded to fp32, records shuffled:
    the order of the atomics must not matter): the restatement's integer boxes in its order, box by box."""
    frames, net, kw = C.case(name)
    g = gpu(net)
    traces = _traces(name)
    rng = np.random.default_rng(1)
    B, cap = len(frames), g.cap
    cand = np.zeros((B, cap, 6), np.float32)
    counts = np.zeros(B, np.int32)
    for f, tr in enumerate(traces):
        s1 = tr["s1"]
        n = len(s1["score"])
        perm = rng.permutation(n)
        cand[f, :n, :4] = s1["reg"][perm]
        cand[f, :n, 4] = s1["score"][perm]
        cand[f, :n, 5] = ((s1["level"][perm] << 24) | s1["cell"][perm]).astype(np.uint32).view(np.float32)
        counts[f] = n
    sizes = [tuple(int(v) for v in frames.shape[1:3])] * B
    boxes, scores, oc = g.stage1(torch.from_numpy(cand).cuda(), torch.from_numpy(counts).cuda(), sizes)
    boxes, oc = boxes.cpu().numpy(), oc.cpu().numpy()
    exempt = sum(_exempt_boxes(boxes[f], int(oc[f]), tr["s1"]["pre"], tr["s1"]["ok"]) for f, tr in enumerate(traces))
    assert exempt <= 0.05 * sum(len(tr["s1"]["pre"]) for tr in traces)


def _forced_inputs(name, key):
    """The restatement's stage-`key` boxes of every frame on the device, and its net outputs on them rounded to fp32; a
    candidate whose score lies within 8 x DEV_SCORE of the threshold is a coin toss of `p >= t` and is left out (and counted)."""
    frames, net, kw = C.case(name)
    nxt = "s2" if key == "s1" else "s3"
    t = kw["thresholds"][1 if key == "s1" else 2]
    traces = _traces(name)
    B = len(frames)
    per, coins = [], 0
    for tr in traces:
        p, r, b = tr[nxt]["prob"], tr[nxt]["reg"], tr[key]["boxes"]
        sure = np.abs(p - t) >= 8 * DEV_SCORE
        coins += int((~sure).sum())
        per.append((b[sure], _f32(p[sure]), _f32(r[sure])))
    cap = max(len(b) for b, _, _ in per)
    boxes = np.zeros((B, cap, 4), np.int32)
    offs = np.zeros(B + 1, np.int32)
    for f, (b, _, _) in enumerate(per):
        boxes[f, :len(b)] = b
        offs[f + 1] = offs[f] + len(b)
    prob = np.zeros((offs[-1], 4), np.float32)
    prob[:, 1] = np.concatenate([p for _, p, _ in per])
    reg = np.zeros((offs[-1], 16), np.float32)
    r = np.concatenate([r for _, _, r in per])
    reg[:, :r.shape[1]] = r
    total = sum(len(tr[nxt]["prob"]) for tr in traces)
    assert coins <= 0.05 * total
    return net, t, per, torch.from_numpy(boxes).cuda(), torch.from_numpy(offs).cuda(), torch.from_numpy(prob).cuda(), torch.from_numpy(reg).cuda()


@pytest.mark.parametrize("name", list(C.SETS))
def test_stage2_teacher_forced(name):
    """fp_mtcnn_stage2 as a whole, fed the restatement's stage-1 boxes and its R-Net outputs rounded to fp32: threshold, NMS,
    regress / square / truncate give the boxes the restatement computes from those same fp32 values, box by box."""
    net, t, per, boxes, offs, prob, reg = _forced_inputs(name, "s1")
    ob, osc, oc = gpu(net).stage2(boxes, offs, prob, reg, t2=t)
    ob, oc = ob.cpu().numpy(), oc.cpu().numpy()
    exempt = total = 0
    for f, (b, p, r) in enumerate(per):
        want = R.stage2_from(b, p, r, t)
        exempt += _exempt_boxes(ob[f], int(oc[f]), want["pre"], want["ok"])
        total += len(b)
    assert exempt <= 0.05 * total


@pytest.mark.parametrize("name", list(C.SETS))
def test_stage3_teacher_forced(name):
    """fp_mtcnn_stage3 as a whole, fed the restatement's stage-2 boxes and its O-Net outputs rounded to fp32: the final rows
    (threshold, regressed boxes, landmark mapping, the "min" NMS, the order) equal what the restatement computes from those same
    fp32 values: every box and landmark value within 1e-6 of its own magnitude, scores the fp32 values themselves."""
    net, t, per, boxes, offs, prob, reg = _forced_inputs(name, "s2")
    dets, counts, over = gpu(net).stage3(boxes, offs, prob, reg, 64, t3=t)
    dets, counts = dets.cpu().numpy().astype(np.float64), counts.cpu().numpy()
    assert not over.any()
    for f, (b, p, r) in enumerate(per):
        want = R.stage3_from(b, p, r, t)["dets"]
        assert counts[f] == len(want), (name, f)
        got = dets[f, :counts[f]]
        assert (np.abs(got[:, :14] - want[:, :14]) <= 1e-6 * np.abs(want[:, :14])).all(), (name, f)
        assert np.array_equal(got[:, 14], want[:, 14]), (name, f)


@pytest.mark.parametrize("name", list(C.SETS))
def test_determinism_and_batch_independence(name):
    frames, net, kw = C.case(name)
    g = gpu(net)
    d1, c1, o1 = g.detect_batch(frames)
    d2, c2, o2 = g.detect_batch(frames)
    assert torch.equal(c1, c2) and not o1.any() and not o2.any()
    for b in range(len(frames)):
        n = int(c1[b])
        assert n >= 3
        assert torch.equal(d1[b, :n], d2[b, :n])
        ds, cs, _ = g.detect_batch(frames[b:b + 1])
        assert int(cs[0]) == n and torch.equal(ds[0, :n], d1[b, :n]), b


def test_end_to_end_against_restatement():
    """Final faces of the GPU and of the restatement matched one-to-one at IoU >= 0.9 over both sets (16 frames, two shapes):
    the share left unmatched on either side stays within twice the restatement's own fp32-vs-fp64 share, plus one face;
    matched faces agree to 1e-3 of the box side in boxes and landmarks, 1e-4 in score."""
    unmatched = total = 0
    for name in C.SETS:
        frames, net, kw = C.case(name)
        dets, counts, over = gpu(net).detect_batch(frames)
        assert not over.any()
        dets, counts = dets.cpu().numpy().astype(np.float64), counts.cpu().numpy()
        sd = net.state_dict()
        for f, frame in enumerate(frames):
            ref = R.detect(frame, sd, **kw)
            got = dets[f, :counts[f]]
            pairs, ua, ub = R.match(got, ref)
            unmatched += len(ua) + len(ub)
            total += len(ref)
            for i, j in pairs:
                side = max(ref[j, 2] - ref[j, 0], ref[j, 3] - ref[j, 1])
                assert np.abs(got[i, :14] - ref[j, :14]).max() <= 1e-3 * side, (name, f, i, j)
                assert abs(got[i, 14] - ref[j, 14]) <= 1e-4
    print(f"end to end: {unmatched} faces unmatched of {total}")
    assert total >= 16 * 3
    assert unmatched <= 2 * FP32_UNMATCHED_SHARE * total + 1


def test_ragged_batch_equals_frames_alone():
    fr, net, kw = C.ragged_mix()
    g = gpu(net)
    rf = RaggedFrames.from_list(fr, "cuda")
    d, c, o = g.detect_batch(rf)
    for b, f in enumerate(fr):
        ds, cs, _ = g.detect_batch(f[None])
        n = int(c[b])
        assert n == int(cs[0]) and torch.equal(d[b, :n], ds[0, :n])


def test_candidate_cap_raises():
    from face_detection_and_recognition_amd import _lib as L
    frames, net, kw = C.case("wide")
    g = gpu(net)
    g.cap = 16
    with pytest.raises(L.FacepathError, match="cap"):
        g.detect_batch(frames[:2])
