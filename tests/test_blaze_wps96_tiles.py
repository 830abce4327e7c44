"""blazeblock_wps_kernel<96> (csrc/blazewp.hip) runs eight waves per workgroup, one 32-pixel tile per wave and launch up to
2048 tiles: the shapes at which that mapping can go wrong, each as a one-op plan (96 -> 96, stride 1, row-padded input) with
dense and with row-padded output.

The protocol, the seeded parameters and data, the float64 reference and its bound (2 * max|ref32 - ref64| + 2e-7 * max|ref64|)
and the footprint check are those of tests/test_blaze_ops.py and tests/blaze_op_cases.py, imported: a sentinel-filled arena,
NaN wherever the op must not read and in its footprint, nothing written outside the output view (pad pixels and pad rows of
a row-padded output included), a second run that repeats the first bit for bit.

  16 x 16, N = 1     8 tiles: one workgroup, eight waves, one tile each
  16 x 16, N = 3     24 tiles: several workgroups, XCD order
  4 x 16,  N = 3     2 tiles per image, 6 tiles: waves 6 and 7 of the only workgroup have no tile
  4 x 16,  N = 5     10 tiles: the second workgroup partly empty
  8 x 32,  N = 2     W = 32 addressing (wshift = 5)
  16 x 16, N = 257   2056 tiles > 256 CUs x 8 waves: two tiles per wave, so the second tile and its rolled window prefetch,
                     with the last runs short

Images past the third hold the data of image i % 3 and must equal it bit for bit; image i of the N = 3 run equals the N = 1
run on that image bit for bit: which wave computes a tile does not matter.
"""
import numpy as np
import pytest
import torch

import blaze_op_cases as S
import test_blaze_ops as T
from face_detection_and_recognition_amd.plan import CompiledPlan, validate_on_host

KERNEL = "blazeblock_wps_kernel<96>"
WAVES, SLOTS = 8, 256 * 8          # waves per workgroup; waves of a full grid (one workgroup per CU)
SHAPES = [(16, 16, 1), (16, 16, 3), (4, 16, 3), (4, 16, 5), (8, 32, 2), (16, 16, 257)]


def _case(H, W, N, out_rp):
    return S.Case(f"wps96_tiles_{H}x{W}_n{N}_{'rp' if out_rp else 'dense'}", "block", KERNEL, N, H, W, 96, 96, in_rp=True,
                  out_rp=out_rp, large=N > 3)


CASES = [_case(H, W, N, rp) for H, W, N in SHAPES for rp in (False, True)]
IDS = [c.name for c in CASES]


def _grid(c):
    """(tiles, tiles per wave, workgroups) as launch_blazeblock_wps<96> has them."""
    ntiles = c.N * c.H * c.W // 32
    per_wave = -(-ntiles // SLOTS)
    return ntiles, per_wave, -(-ntiles // (WAVES * per_wave))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_lands_on_the_kernel(lib, case):
    """Every case validates, reaches blazeblock_wps_kernel<96> and keeps a bound below 1e-5 of scale."""
    pb, _ = S.build(case)
    assert validate_on_host(pb) == 0
    assert S.kernel_name(pb.ops[0]) == KERNEL
    r64, r32 = S.reference(case), S.reference(case, dtype=torch.float32)
    scale = np.abs(r64).max()
    assert 2.0 * np.abs(r32 - r64).max() + S.tolerance(case) * scale < 1e-5 * scale


def test_shapes_are_what_the_table_says():
    g = {(c.H, c.W, c.N): _grid(c) for c in CASES}
    assert g[16, 16, 1] == (8, 1, 1)                    # one workgroup, every wave one tile
    assert g[16, 16, 3] == (24, 1, 3)
    assert g[4, 16, 3] == (6, 1, 1)                     # waves 6 and 7 empty
    assert g[4, 16, 5] == (10, 1, 2)                    # second workgroup: two tiles, six empty waves
    assert g[8, 32, 2] == (16, 1, 2)
    assert g[16, 16, 257] == (2056, 2, 129)             # two tiles per wave; 2056 = 128 * 16 + 8: the last workgroup's waves 4 .. 7 empty


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wps96_tiles_vs_fp64(dev, case):
    """The protocol of tests/test_blaze_ops.py on every shape: fp64 bound, footprint, second run, image i == image i % 3."""
    T._result(case, dev)


def _single(case1, image, dev):
    """The N = 1 plan of case1 on one image [H, W, 96] -> its output [H, W, 96]."""
    pb, bufs = S.build(case1)
    plan = CompiledPlan(pb, dev)
    assert plan.kernel_name(0) == KERNEL
    host = np.zeros(plan.arena_floats, np.float32)
    T._in_view(host, bufs["x"], 1, 96)[0] = image
    plan.arena.copy_(torch.from_numpy(host).to(dev))
    plan.run(1)
    torch.cuda.synchronize()
    return T._out_view(plan.arena.cpu().numpy(), plan.ops[0], 1)[0].copy()


@pytest.mark.gpu
@pytest.mark.parametrize("out_rp", [False, True], ids=["dense", "rp"])
def test_wave_position_does_not_matter(dev, out_rp):
    """Image i of the N = 3 run (tiles 8 i .. 8 i + 7: another workgroup, another XCD) equals the N = 1 run on that image,
    where the same tiles belong to the waves of workgroup 0."""
    c3, c1 = _case(16, 16, 3, out_rp), _case(16, 16, 1, out_rp)
    got3 = T._result(c3, dev)[3]
    x = S.inputs(c3)
    for i in range(3):
        one = _single(c1, x[i], dev)
        assert np.array_equal(one.view(np.int32), got3[i].view(np.int32)), f"image {i}"
