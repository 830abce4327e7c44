"""Age and gender nets (Levi & Hassner, the reference's modules/opencv2_dnn/model.py): the Caffe weight reader, the plans,
the attribute crop geometry, the label format (CPU), and the new ops and both whole nets against float64 torch
restatements (GPU)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from face_detection_and_recognition_amd import _lib as L
from face_detection_and_recognition_amd.modules.age_gender import age_gender_net as AG
from face_detection_and_recognition_amd.modules.age_gender.age_gender_net import AgeGenderNet
from face_detection_and_recognition_amd.modules.utils.caffemodel import (CaffeModelError, encode_net, read_caffemodel,
                                                                          read_caffemodel_blobs)
from face_detection_and_recognition_amd.plan import CompiledPlan, PlanBuilder, validate_on_host
from face_detection_and_recognition_amd.synth import synth_age_gender

MEAN = torch.tensor(AG.MEAN_BGR, dtype=torch.float64).view(1, 3, 1, 1)


def _net_layers(sub):
    return [(name, [getattr(sub, name).weight.numpy(), getattr(sub, name).bias.numpy()]) for name in AG.LAYERS]


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the caffemodel reader
@pytest.mark.parametrize("v1,legacy,packed", [(False, False, True), (True, True, True), (True, False, False),
                                              (False, True, False)])
def test_caffemodel_round_trip(v1, legacy, packed):
    rng = np.random.default_rng(3)
    layers = [("conv1", [rng.normal(size=(4, 3, 2, 2)).astype(np.float32), rng.normal(size=4).astype(np.float32)]),
              ("relu1", []),
              ("fc8", [rng.normal(size=(2, 6)).astype(np.float32), rng.normal(size=2).astype(np.float32)])]
    buf = encode_net(layers, v1=v1, legacy_shape=legacy, packed=packed)
    got = read_caffemodel(buf)
    assert sorted(got) == ["conv1", "fc8"]           # a layer without blobs is not listed
    for name, blobs in layers:
        for b, g in zip(blobs, got.get(name, [])):
            assert np.array_equal(g.reshape(b.shape), b)
            if not legacy:
                assert g.shape == b.shape
    pairs = read_caffemodel_blobs(buf, {"conv1": ((4, 3, 2, 2), (4,)), "fc8": ((2, 6), (2,))})
    assert pairs["fc8"][0].shape == (2, 6) and np.array_equal(pairs["fc8"][1], layers[2][1][1])


def test_caffemodel_whole_net_round_trip(tmp_path):
    src = synth_age_gender(AgeGenderNet(), 11)
    paths = []
    for sub, v1 in ((src.age, True), (src.gender, False)):
        p = tmp_path / f"{'age' if v1 else 'gender'}.caffemodel"
        p.write_bytes(encode_net(_net_layers(sub), v1=v1, legacy_shape=v1))
        paths.append(str(p))
    net = AgeGenderNet.from_caffemodels(*paths)
    for k, v in src.state_dict().items():
        assert torch.equal(net.state_dict()[k], v), k


def test_caffemodel_refuses_bad_files():
    rng = np.random.default_rng(4)
    good = [("conv1", [rng.normal(size=(4, 3, 2, 2)).astype(np.float32), np.zeros(4, np.float32)])]
    buf = encode_net(good)
    with pytest.raises(CaffeModelError, match="not found"):
        read_caffemodel_blobs(buf, {"conv2": ((4, 3, 2, 2), (4,))})
    with pytest.raises(CaffeModelError, match="shape"):
        read_caffemodel_blobs(buf, {"conv1": ((4, 3, 3, 3), (4,))})
    with pytest.raises(CaffeModelError, match="blob"):
        read_caffemodel_blobs(encode_net([("conv1", good[0][1][:1])]), {"conv1": ((4, 3, 2, 2), (4,))})
    with pytest.raises(CaffeModelError):
        read_caffemodel(buf[:-3])                       # truncated
    with pytest.raises(CaffeModelError):
        read_caffemodel(b"\x07\x01")                    # field 0
    with pytest.raises(CaffeModelError):
        AgeGenderNet.from_caffemodels(buf, buf)          # a net without conv2 .. fc8


# ---------------------------------------------------------------------------------------------------------------------
# CPU: plans
@pytest.mark.parametrize("x6", [True, False])
def test_plans_validate(lib, x6):
    net = synth_age_gender(AgeGenderNet(), 1)
    saved = PlanBuilder.X6
    PlanBuilder.X6 = x6
    try:
        pb, *_ = net._emit(6)
        assert validate_on_host(pb) == 0
        names = [lib.fp_op_kernel_name(ctypes.byref(op)).decode() for op in pb.ops]
    finally:
        PlanBuilder.X6 = saved
    assert "?" not in names
    convs = [(op, n) for op, n in zip(pb.ops, names) if op.kind == L.OP_CONV]
    assert len(convs) == 9            # conv1 (both nets) + conv2 .. fc7 of each net
    for op, n in convs:
        if x6:
            assert op.flags & L.OPF_SPLIT3 and n.startswith(("convx6_kernel", "pwx6_kernel")), n
        else:
            assert not op.flags & L.OPF_SPLIT3 and n.startswith("conv_igemm_kernel"), n
    assert convs[0][0].stride == 4 and convs[0][0].Cout == 192 and convs[0][0].KH == 7
    kinds = [op.kind for op in pb.ops]
    assert kinds.count(L.OP_POOL_LRN) == 2 and kinds.count(L.OP_CLS_HEAD) == 2 and kinds.count(L.OP_MAXPOOL) == 1
    lrn = [op for op in pb.ops if op.kind == L.OP_POOL_LRN]
    assert [(op.Cin, op.Cmid, op.res_C, op.OH) for op in lrn] == [(192, 96, 5, 28), (512, 256, 5, 14)]


def test_plan_refuses_cpu_device():
    with pytest.raises(L.FacepathError):
        AgeGenderNet().plan_for(2)


def test_new_ops_refuse_bad_shapes(lib):
    pb = PlanBuilder(2)
    x, o = pb.new_buf(9, 9, 16), pb.new_buf(4, 4, 16)
    pb.pool_lrn(x.view(), o.view(), 3, 2, group=8)
    op = pb.ops[0]
    assert lib.fp_op_kernel_name(ctypes.byref(op)).decode() == "pool_lrn_kernel"
    for field, v in (("Cmid", 6), ("res_C", 4), ("Cout", 12), ("KH", 8)):
        bad = L.FpOp.from_buffer_copy(op)
        setattr(bad, field, v)
        assert lib.fp_op_kernel_name(ctypes.byref(bad)).decode() == "?", field
    pb = PlanBuilder(2)
    x, o = pb.new_buf(1, 1, 64), pb.new_buf(1, 1, 80)
    pb.cls_head(x.view(), np.zeros((80, 64), np.float32), None, o.view(0, 80))
    assert lib.fp_op_kernel_name(ctypes.byref(pb.ops[0])).decode() == "?"       # at most 64 classes


# ---------------------------------------------------------------------------------------------------------------------
# CPU: crop geometry and labels
def ref_attr_items(info, sizes, pad=5, dst=227):
    """The reference's rule (OpenCVFaceDetAgeGenderModel.__call__) restated in numpy, as fp_resize_item rows."""
    out = []
    for row in np.asarray(info, np.float32):
        h, w = sizes[int(row[0])]
        b = list(map(int, np.round(row[1:5].astype(np.float64))))
        img = np.zeros((h, w), np.uint8)
        face = img[max(0, b[1] - pad):min(b[3] + pad, h - 1), max(0, b[0] - pad):min(b[2] + pad, w - 1)]
        x0, y0 = max(0, b[0] - pad), max(0, b[1] - pad)
        if face.shape[0] == 0 or face.shape[1] == 0:
            out.append([int(row[0]), 0, 0, 0, 0, 0, 0, 0, 0])
        else:
            out.append([int(row[0]), x0, y0, face.shape[1], face.shape[0], 0, 0, dst, dst])
    return np.array(out, np.int32).reshape(-1, 9)


ATTR_SIZES = [(120, 160), (97, 61), (20, 30)]
ATTR_INFO = np.array([
    [0, 10.5, 11.5, 40.5, 60.5],      # .5 ties both ways (10, 12, 40, 60)
    [0, 0, 0, 160, 120],              # the whole frame: clamp to W - 1, H - 1
    [0, 3, 2, 9, 8],                  # near the top-left corner
    [0, 150, 110, 160, 120],          # touching the bottom-right corner
    [1, 0, 40, 61, 97],               # left, right and bottom edges
    [1, 58.5, 3.5, 61, 10],           # a sliver at the right edge
    [1, 61, 97, 61, 97],              # a point in the corner: the padding keeps 4 x 4 of it
    [1, 40, 40, 20, 60],              # x2 < x1 - 10: empty
    [1, 70, 20, 80, 30],              # beyond the frame: empty
    [2, 2.5, 3.5, 2.5, 3.5],          # zero-size box: 5 px around it
    [2, 25, 15, 30, 20],              # x0 = 20, x_end = 29
    [2, 29.5, 19.5, 30, 20],          # x0 = 25 ... (the rounding of 29.5 is 30)
], np.float32)


def test_attr_crop_items_match_reference_rule(lib):
    info = np.concatenate([ATTR_INFO, np.zeros((len(ATTR_INFO), 2), np.float32)], axis=1)     # 7-float info rows
    got = AG.attr_crop_items_host(info, ATTR_SIZES)
    want = ref_attr_items(ATTR_INFO, ATTR_SIZES)
    assert np.array_equal(got, want), (got, want)
    empty = want[:, 3] == 0
    assert empty.sum() == 2 and (got[empty, 7:] == 0).all()


def test_attr_crop_items_dense_and_refusals(lib):
    info = ATTR_INFO[ATTR_INFO[:, 0] == 0]
    descs = (L.FpFrameDesc * 1)()
    items = np.zeros((len(info), 9), np.int32)
    assert lib.fp_attr_crop_items_emulate(info.ctypes.data, len(info), 5, None, 1, 160, 120, 5, 227, 227,
                                          items.ctypes.data) == 0
    assert np.array_equal(items, ref_attr_items(info, ATTR_SIZES))
    for n, nf, pad, d in ((-1, 5, 5, 227), (1, 4, 5, 227), (1, 5, -1, 227), (1, 5, 5, 0)):
        assert lib.fp_attr_crop_items_emulate(info.ctypes.data, n, nf, descs, 1, 160, 120, pad, d, d,
                                              items.ctypes.data) == L.FP_ERR_INVALID_ARG


def test_labels_match_reference_format():
    age = np.array([[0.1, 0.05, 0.05, 0.5, 0.1, 0.1, 0.05, 0.05], [1 / 8] * 8, [0] * 7 + [1.0]], np.float32)
    gender = np.array([[0.3, 0.7], [0.5, 0.5], [0.996, 0.004]], np.float32)
    got = AG.labels(age, gender)
    want = []
    for a, g in zip(age, gender):      # OpenCVFaceDetAgeGenderModel.__call__
        want.append(f"{AG.GENDER_LIST[g.argmax()]}:{g.max():.2f}," + f"{AG.AGE_LIST[a.argmax()]}:{a.max():.2f}")
    assert got == want == ["Female:0.70,(15-20):0.50", "Male:0.50,(0-2):0.12", "Male:1.00,(60-100):1.00"]
    assert AG.labels(np.full((1, 8), np.nan), np.full((1, 2), np.nan)) == ["?:nan,?:nan"]
    assert AG.AGE_LIST == ['(0-2)', '(4-6)', '(8-12)', '(15-20)', '(25-32)', '(38-43)', '(48-53)', '(60-100)']
    assert AG.GENDER_LIST == ['Male', 'Female']


def test_opencv_models_interface():
    from face_detection_and_recognition_amd.modules.opencv2_dnn.model import (OpenCVFaceAgeModel,
                                                                              OpenCVFaceDetAgeGenderModel,
                                                                              OpenCVFaceGenderModel)
    net = AgeGenderNet()
    a = OpenCVFaceAgeModel(net, 0.5, 0.1)
    g = OpenCVFaceGenderModel(net, 0.5, 0.1)
    assert a.input_size == g.input_size == (227, 227) and not a.returns_opt_labels
    with pytest.raises(ValueError):
        OpenCVFaceAgeModel(net, 0.5, 0.1, AGE_MEAN_VALUES=(104.0, 117.0, 123.0))

    class Det:
        input_size, det_thres, bbox_area_thres = (128, 128), 0.7, 0.1
    m = OpenCVFaceDetAgeGenderModel(Det(), net)
    assert m.returns_opt_labels and m.det_thres == 0.7 and m.age_list == AG.AGE_LIST and m.gender_list == AG.GENDER_LIST


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the new ops against float64
def oracle_pool_lrn(x, group, lrn=True, size=5, alpha=1e-4, beta=0.75, k=1.0):
    """x (N, C, H, W) float64: max_pool2d(3, 2, ceil) then local_response_norm per channel group."""
    y = F.max_pool2d(x, 3, 2, ceil_mode=True)
    if not lrn:
        return y
    return torch.cat([F.local_response_norm(t, size, alpha, beta, k) for t in y.split(group, dim=1)], dim=1)


@pytest.mark.gpu
@pytest.mark.parametrize("N,C,G,H,W", [(3, 192, 96, 56, 56), (2, 512, 256, 28, 28), (5, 24, 8, 13, 10), (1, 4092, 1364, 7, 6),
                                       (4, 40, 40, 6, 9)])
def test_pool_lrn_vs_fp64(dev, N, C, G, H, W):
    rng = np.random.default_rng(C + G + H)
    x = rng.normal(0, 60, (N, C, H, W)).astype(np.float32)
    OH, OW = AG.pool_out(H), AG.pool_out(W)
    pb = PlanBuilder(N)
    xb, ob = pb.new_buf(H, W, C + 8), pb.new_buf(OH, OW, C + 4)
    pb.pool_lrn(xb.view(4, C), ob.view(0, C), 3, 2, group=G)
    plan = CompiledPlan(pb, dev)
    assert plan.kernel_name(0) == "pool_lrn_kernel"
    xt = torch.full((N, H, W, C + 8), float("nan"), device=dev)
    xt[..., 4:4 + C] = torch.from_numpy(x).to(dev).permute(0, 2, 3, 1)
    plan.buf_tensor(xb, N).copy_(xt)
    out = plan.buf_tensor(ob, N)
    out.fill_(-7.0)
    plan.run()
    torch.cuda.synchronize()
    full = out.permute(0, 3, 1, 2).cpu().numpy()
    assert (full[:, C:] == -7.0).all()                       # channels beyond the view untouched
    want = oracle_pool_lrn(torch.from_numpy(x).double(), G).numpy()
    assert rel_err(full[:, :C], want) < 1e-5
    # and the group matters: one LRN over all channels differs at the boundaries
    if G < C:
        assert rel_err(oracle_pool_lrn(torch.from_numpy(x).double(), C).numpy(), want) > 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("stride4_cout", [192, 96])
def test_stride4_conv_vs_fp64(dev, stride4_cout):
    N, H, W, cout = 3, 227, 227, stride4_cout
    rng = np.random.default_rng(cout)
    x = rng.uniform(0, 255, (N, 3, H, W)).astype(np.float32)
    w = rng.normal(0, (2 / 147) ** 0.5, (cout, 3, 7, 7)).astype(np.float32)
    b = rng.normal(0, 5, cout).astype(np.float32)
    outs = {}
    for x6 in (True, False):
        saved = PlanBuilder.X6
        PlanBuilder.X6 = x6
        try:
            pb = PlanBuilder(N)
            pb.x6_all = True
            xb, ob = pb.new_buf(H, W, 3), pb.new_buf(56, 56, cout)
            pb.conv(xb.view(), w, ob.view(), stride=4, bias=b, act=L.ACT_RELU)
            plan = CompiledPlan(pb, dev)
        finally:
            PlanBuilder.X6 = saved
        assert plan.kernel_name(0).startswith("convx6_kernel" if x6 else "conv_igemm_kernel"), plan.kernel_name(0)
        xt = torch.zeros((N, H, W, 4), device=dev)
        xt[..., :3] = torch.from_numpy(x).to(dev).permute(0, 2, 3, 1)
        plan.buf_tensor(xb, N).copy_(xt)
        plan.run()
        torch.cuda.synchronize()
        outs[x6] = plan.buf_tensor(ob, N).permute(0, 3, 1, 2).cpu().numpy()
    want = torch.relu(F.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(),
                               stride=4)).numpy()
    assert rel_err(outs[True], want) < 1e-5
    assert rel_err(outs[False], want) < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("N,C,D", [(7, 512, 8), (5, 512, 2), (3, 100, 64), (1, 4096, 33)])
def test_cls_head_vs_fp64(dev, N, C, D):
    rng = np.random.default_rng(N * D)
    x = rng.normal(0, 1, (N, C)).astype(np.float32)
    w = rng.normal(0, 2 / C ** 0.5, (D, C)).astype(np.float32)
    b = rng.normal(0, 0.5, D).astype(np.float32)
    pb = PlanBuilder(N)
    xb, ob, zb = pb.new_buf(1, 1, C), pb.new_buf(1, 1, D), pb.new_buf(1, 1, D)
    pb.cls_head(xb.view(), w, b, ob.view(0, D), zb.view(0, D))
    plan = CompiledPlan(pb, dev)
    xt = torch.zeros((N, 1, 1, xb.C), device=dev)
    xt[..., :C] = torch.from_numpy(x).to(dev).view(N, 1, 1, C)
    plan.buf_tensor(xb, N).copy_(xt)
    plan.run()
    torch.cuda.synchronize()
    p = plan.buf_tensor(ob, N).reshape(N, -1)[:, :D].cpu().numpy()
    z = plan.buf_tensor(zb, N).reshape(N, -1)[:, :D].cpu().numpy()
    zw = torch.from_numpy(x).double() @ torch.from_numpy(w).double().T + torch.from_numpy(b).double()
    assert rel_err(z, zw.numpy()) < 1e-5
    assert np.abs(p - torch.softmax(zw, 1).numpy()).max() < 1e-6
    assert np.abs(p.sum(1) - 1).max() < 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# GPU: both whole nets against a float64 oracle
def oracle_forward(net, x):
    """x (N, 3, 227, 227) float64 BGR pixel values -> [(age logits, age probs), (gender logits, gender probs)]."""
    out = []
    for sub in (net.age, net.gender):
        p = {k: (getattr(sub, k).weight.double(), getattr(sub, k).bias.double()) for k in AG.LAYERS}
        y = torch.relu(F.conv2d(x - MEAN, *p["conv1"], stride=4))
        y = F.local_response_norm(F.max_pool2d(y, 3, 2, ceil_mode=True), 5, 1e-4, 0.75, 1.0)
        y = torch.relu(F.conv2d(y, *p["conv2"], padding=2))
        y = F.local_response_norm(F.max_pool2d(y, 3, 2, ceil_mode=True), 5, 1e-4, 0.75, 1.0)
        y = torch.relu(F.conv2d(y, *p["conv3"], padding=1))
        y = F.max_pool2d(y, 3, 2, ceil_mode=True).flatten(1)       # Caffe's (c, y, x) order
        y = torch.relu(F.linear(y, *p["fc6"]))
        y = torch.relu(F.linear(y, *p["fc7"]))
        z = F.linear(y, *p["fc8"])
        out.append((z, torch.softmax(z, 1)))
    return out


@pytest.fixture(scope="module")
def agnet(dev):
    return synth_age_gender(AgeGenderNet(), 2024).to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("x6", [True, False])
def test_whole_nets_vs_fp64_oracle(dev, agnet, x6):
    N = 3
    rng = np.random.default_rng(77)
    x = rng.integers(0, 256, (N, 3, 227, 227)).astype(np.float32)
    saved = PlanBuilder.X6
    PlanBuilder.X6 = x6
    try:
        age, gender, za, zg = agnet(torch.from_numpy(x), return_logits=True)
    finally:
        PlanBuilder.X6 = saved
    torch.cuda.synchronize()
    assert age.shape == (N, 8) and gender.shape == (N, 2)
    cpu = synth_age_gender(AgeGenderNet(), 2024)
    (wza, wa), (wzg, wg) = oracle_forward(cpu, torch.from_numpy(x).double())
    assert rel_err(za.cpu().numpy(), wza.numpy()) < 1e-4
    assert rel_err(zg.cpu().numpy(), wzg.numpy()) < 1e-4
    assert np.abs(age.cpu().numpy() - wa.numpy()).max() < 1e-5
    assert np.abs(gender.cpu().numpy() - wg.numpy()).max() < 1e-5
    # the two nets really differ: a swapped branch or a leaking LRN group could not pass the bounds above
    assert not torch.allclose(cpu.age.conv1.weight, cpu.gender.conv1.weight)
    assert wa.max() < 0.999 and wg.max() < 0.999                    # the softmax is not saturated


@pytest.mark.gpu
def test_opencv_models_on_gpu(dev, agnet):
    from face_detection_and_recognition_amd.modules.opencv2_dnn.model import OpenCVFaceAgeModel, OpenCVFaceGenderModel
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, (90, 70, 3)).astype(np.uint8)
    pa = OpenCVFaceAgeModel(agnet, 0.5, 0.1)(img)
    pg = OpenCVFaceGenderModel(agnet, 0.5, 0.1)(img)
    assert pa.shape == (8,) and pg.shape == (2,)
    # the same crop resized by the resize kernel and run through forward()
    from face_detection_and_recognition_amd.modules.mobile_facenet.utils import crops_to_input
    frames = torch.from_numpy(img).to(dev).unsqueeze(0)
    items = torch.tensor([[0, 0, 0, 70, 90, 0, 0, 227, 227]], dtype=torch.int32, device=dev)
    canvas = torch.zeros((1, 227, 227, 4), device=dev)
    crops_to_input(frames, items, 1, canvas, agnet.input_lut(dev))
    a, g = agnet(canvas[..., :3].permute(0, 3, 1, 2))
    assert np.array_equal(a[0].cpu().numpy(), pa) and np.array_equal(g[0].cpu().numpy(), pg)
    assert abs(pa.sum() - 1) < 1e-5 and abs(pg.sum() - 1) < 1e-5
