"""CPU checks of the plan builder's packing helpers (plan.py) and of the networks' plan-cache mixin (modules/params.py) -- no GPU.

The two split-bf16 plane packers are compared, element by element, with a plain-loop restatement of the layout their docstrings
(and include/facepath.h) give; the parameter-row helpers with pack_dw_weight / pad_vec called directly."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from face_detection_and_recognition_amd.modules.blazeface.blazeface import BlazeFace
from face_detection_and_recognition_amd.modules.mtcnn.mtcnn import MTCNN
from face_detection_and_recognition_amd.plan import (affine_rows, dw_rows, pack_dw_weight, pack_kslab_x6, pack_rowblock_x6, pad_vec,
                                                     split3_bf16)
from face_detection_and_recognition_amd.synth import synth_state_dict


def _adversarial(rng, shape):
    """An fp32 matrix of bit patterns whose split pieces are as large as they get (all-ones mantissas, mantissas next to the
    rounding ties of both cuts) or all non-zero (random mantissas with low bits set), random signs and exponents: a dropped or
    repeated plane cannot sum to the input."""
    n = int(np.prod(shape))
    mant = rng.choice(np.array([0x7FFFFF, 0x007FFF, 0x00807F, 0x7F7F7F, 0x35A5C3], np.uint32), n)
    mant[n // 2:] = rng.integers(1 << 8, 1 << 23, n - n // 2) | 0x101
    expo = rng.integers(100, 150, n).astype(np.uint32)
    sign = rng.integers(0, 2, n).astype(np.uint32)
    return ((sign << 31) | (expo << 23) | mant.astype(np.uint32)).view(np.float32).reshape(shape)


def _bf16(blob, shape):
    """The packed blob (fp32-viewed, two bf16 per float) as fp32 values of its bf16 elements, in `shape`."""
    assert blob.dtype == np.float32 and blob.ndim == 1 and blob.size * 2 == int(np.prod(shape))
    return (blob.view(np.uint16).astype(np.uint32) << 16).view(np.float32).reshape(shape)


def _pieces(m):
    return (split3_bf16(m).astype(np.uint32) << 16).view(np.float32)         # [3][rows][columns]


@pytest.mark.parametrize("shape", [(48, 64), (96, 32), (32, 96)])
def test_kslab_layout(shape):
    m = _adversarial(np.random.default_rng(shape[0]), shape)
    n, K = shape
    got = _bf16(pack_kslab_x6(m), (K // 32, 3, n, 32))
    piece = _pieces(m)
    for slab in range(K // 32):
        for plane in range(3):
            for row in range(n):
                for k in range(32):
                    assert got[slab, plane, row, k] == piece[plane, row, 32 * slab + k], (slab, plane, row, k)
    total = got[:, 0] + got[:, 1] + got[:, 2]                                # [slab][n][32], summed high piece first
    np.testing.assert_array_equal(total.transpose(1, 0, 2).reshape(n, K), m)


@pytest.mark.parametrize("shape", [(64, 64), (96, 32), (32, 96)])
def test_rowblock_layout(shape):
    m = _adversarial(np.random.default_rng(shape[1]), shape)
    g, k = shape
    got = _bf16(pack_rowblock_x6(m), (g // 32, 3, k // 32, 32, 32))
    piece = _pieces(m)
    for R in range(g // 32):
        for plane in range(3):
            for ks in range(k // 32):
                for gi in range(32):
                    for ki in range(32):
                        assert got[R, plane, ks, gi, ki] == piece[plane, 32 * R + gi, 32 * ks + ki], (R, plane, ks, gi, ki)
    total = got[:, 0] + got[:, 1] + got[:, 2]                                # [R][ks][g'][k']
    np.testing.assert_array_equal(total.transpose(0, 2, 1, 3).reshape(g, k), m)


def test_packers_refuse_partial_slabs():
    z = np.zeros
    with pytest.raises(AssertionError):
        pack_kslab_x6(z((32, 48), np.float32))
    pack_kslab_x6(z((5, 32), np.float32))              # the row count of a k-slab matrix is free
    with pytest.raises(AssertionError):
        pack_rowblock_x6(z((48, 64), np.float32))
    with pytest.raises(AssertionError):
        pack_rowblock_x6(z((64, 48), np.float32))


@pytest.mark.parametrize("with_slope", [True, False])
def test_dw_rows(with_slope):
    rng = np.random.default_rng(3)
    c, C = 6, 8                                        # six logical channels in eight physical ones
    w = rng.normal(size=(c, 1, 3, 3)).astype(np.float32)
    scale, bias, slope = (rng.normal(size=c).astype(np.float32) for _ in range(3))
    got = dw_rows(w, (scale, bias), slope if with_slope else None, C)
    want = np.concatenate([pack_dw_weight(w, C), pad_vec(scale, C), pad_vec(bias, C),
                           pad_vec(slope, C) if with_slope else np.zeros(C, np.float32)])
    assert got.dtype == np.float32 and got.shape == (12 * C,)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(affine_rows((scale, bias), C), want[9 * C:11 * C])


def _state_dict_keys(name):
    with open(os.path.join(GOLDEN, "state_dict_keys.json")) as f:
        return json.load(f)[name]


def _fill(net):
    """One entry in everything the network derives from its parameters."""
    net._plans.get("key", lambda cache: object())
    assert len(net._plans) == 1


@pytest.mark.parametrize("back", [False, True])
def test_blazeface_drops_its_plans(back):
    net = BlazeFace(back)
    assert list(net.state_dict().keys()) == _state_dict_keys("blazeface_back" if back else "blazeface_front")
    anchors = np.arange(896 * 4, dtype=np.float32).reshape(896, 4)
    net.set_anchors(anchors)
    _fill(net)
    net.load_state_dict(synth_state_dict(net.state_dict(), 1))
    assert len(net._plans) == 0
    _fill(net)
    assert net.to("cpu") is net and len(net._plans) == 0
    assert isinstance(net.anchors, torch.Tensor) and np.array_equal(net.anchors.numpy(), anchors)     # _apply still moves them
    assert list(net.state_dict().keys()) == _state_dict_keys("blazeface_back" if back else "blazeface_front")


def test_mtcnn_drops_its_plans_and_tables():
    net = MTCNN()
    assert list(net.state_dict().keys()) == _state_dict_keys("mtcnn")

    def fill():
        _fill(net)
        net._tables["key"] = object()
        net._pnet_plans["key"] = object()

    def empty():
        return len(net._plans) == 0 and net._tables == {} and net._pnet_plans == {}

    fill()
    net.load_state_dict(synth_state_dict(net.state_dict(), 2))
    assert empty()
    fill()
    assert net.to("cpu") is net and empty()
    assert list(net.state_dict().keys()) == _state_dict_keys("mtcnn")
