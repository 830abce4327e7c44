"""Plan builder: turns a network description into the flat ``fp_op`` array that
``fp_plan_run`` (include/facepath.h) executes, plus the packed weight blob and
the activation-arena layout.

The host side mirrors the reference's module graph (modules/blazeface.py,
modules/mobile_facenet.py, modules/yolov5_face.py emit ops in the order the
reference's ``forward`` runs them); all arithmetic happens in the HIP kernels.
Activations are NHWC fp32 inside one arena tensor; channel counts are padded
to multiples of 4 (16-byte accesses) with zero weights in the padding.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib as L


def round_up(a, b):
    return (a + b - 1) // b * b


def cpad(c):
    """Internal channel count for a logical channel count (16-byte alignment)."""
    return round_up(int(c), 4)


@dataclass
class Buf:
    """An NHWC activation tensor inside the arena (offset in floats)."""
    H: int
    W: int
    C: int       # physical channels = pixel stride
    off: int
    size: int    # floats, whole batch
    ns_: int = -1   # per-image stride override (e.g. a head writing into a [B, 896, 16] tensor)
    rowpad: bool = False   # row-padded layout (include/facepath.h): off = pixel (0, 0) of image 0, row pitch (W+1)*C
    dedicated: bool = False   # the output of ONE row-windowed op: never recycled (rows outside the window keep their values)

    @property
    def ld(self):
        return self.C

    @property
    def ns(self):
        return self.H * self.W * self.C if self.ns_ < 0 else self.ns_

    def view(self, coff=0, C=None, cmul=1):
        return View(self, coff, self.C - coff if C is None else C, cmul)


@dataclass
class View:
    """Channel slice [coff, coff + C*cmul) of a Buf; cmul > 1 interleaves (channel_shuffle)."""
    buf: Buf
    coff: int
    C: int
    cmul: int = 1
    up: object = None   # a View of a half-size map: channels [0, up.C) of THIS view are its nearest-neighbour 2x upsampling and
                        # have NOT been written (PlanBuilder.conv folds them into the operand addressing, FP_OPF_IN_UP2, or
                        # materialises them first: PlanBuilder.materialise_up)

    @property
    def H(self):
        return self.buf.H

    @property
    def W(self):
        return self.buf.W


class Arena:
    """First-fit free-list allocator over a float arena (offsets are multiples of 64 floats)."""

    def __init__(self):
        self.free = []   # sorted list of (off, size)
        self.top = 0

    def place(self, size):
        """(offset, size) of the block alloc(size) returns next; nothing is allocated."""
        size = round_up(size, 64)
        return next(((off, size) for off, sz in self.free if sz >= size), (self.top, size))

    def alloc(self, size):
        off, size = self.place(size)
        for i, (o, sz) in enumerate(self.free):
            if o == off:
                if sz == size:
                    self.free.pop(i)
                else:
                    self.free[i] = (off + size, sz - size)
                return off, size
        self.top += size
        return off, size

    def release(self, off, size):
        self.free.append((off, size))
        self.free.sort()
        merged = []
        for o, s in self.free:
            if merged and merged[-1][0] + merged[-1][1] == o:
                merged[-1] = (merged[-1][0], merged[-1][1] + s)
            else:
                merged.append((o, s))
        # a free block that ends at the top lowers the top
        if merged and merged[-1][0] + merged[-1][1] == self.top:
            self.top = merged[-1][0]
            merged.pop()
        self.free = merged


def pack_conv_weight(w, cin_phys, cout_phys):
    """[Cout, Cin, KH, KW] (torch OIHW) -> Wp[Kpad/4][Npad][4], k = (ky*KW + kx)*cin_phys + ci."""
    w = np.asarray(w, dtype=np.float32)
    cout, cin, kh, kw = w.shape
    assert cin <= cin_phys and cout <= cout_phys
    K = kh * kw * cin_phys
    kpad = round_up(K, 8)
    npad = round_up(cout_phys, 32)
    full = np.zeros((kh, kw, cin_phys, npad), dtype=np.float32)
    full[:, :, :cin, :cout] = np.transpose(w, (2, 3, 1, 0))
    flat = np.zeros((kpad, npad), dtype=np.float32)
    flat[:K] = full.reshape(K, npad)
    return np.ascontiguousarray(flat.reshape(kpad // 4, 4, npad).transpose(0, 2, 1)).reshape(-1)


def pack_dw_weight(w, c_phys):
    """[C, 1, KH, KW] -> Wd[KH*KW][c_phys]."""
    w = np.asarray(w, dtype=np.float32)
    c, one, kh, kw = w.shape
    assert one == 1 and c <= c_phys
    out = np.zeros((kh * kw, c_phys), dtype=np.float32)
    out[:, :c] = w.reshape(c, kh * kw).T
    return out.reshape(-1)


def _bf16_rn_bits(x):
    """fp32 array -> uint32 bit patterns of bf16(x) << 16 (round to nearest even; no NaN / inf handling -- weights are finite)."""
    u = x.view(np.uint32)
    return (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)


def split3_bf16(w):
    """The exact three-way bf16 split of fp32 values (csrc/split.h): h = bf16(w), m = bf16(w - h), l = bf16(w - h - m), every
    conversion round-to-nearest-even, every subtraction exact, w == h + m + l.  Returns uint16 [3, ...] (the bf16 bit
    patterns of the three pieces)."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    h = _bf16_rn_bits(w)
    r = w - h.view(np.float32)
    m = _bf16_rn_bits(r)
    r2 = r - m.view(np.float32)
    l = _bf16_rn_bits(r2)
    assert np.array_equal(l.view(np.float32), r2), "third piece is not exact"
    assert np.array_equal(h.view(np.float32) + m.view(np.float32) + l.view(np.float32), w)
    return np.stack([h >> 16, m >> 16, l >> 16]).astype(np.uint16)


def _f32_blob(planes):
    """bf16 bit patterns (uint16) in their final order -> the flat fp32-viewed blob the weight array carries (2 per float)."""
    return np.ascontiguousarray(planes, dtype=np.uint16).reshape(-1).view(np.float32)


def _mat(w):
    """The fp32 matrix [O, I] of a 1x1 conv weight ([O, I, 1, 1]) or a linear weight ([O, I])."""
    w = np.asarray(w, dtype=np.float32)
    assert w.shape[2:] in ((), (1, 1)), w.shape
    return w.reshape(w.shape[:2])


def pack_kslab_x6(m):
    """"k-slab" split-bf16 planes of an fp32 matrix m[n, K], K a multiple of 32: [K / 32][3 planes][n][32], element
    [slab][plane][n][k'] = piece `plane` of m[n, 32 * slab + k'] (split3_bf16).  The B operand of every split GEMM
    (include/facepath.h, "FP_OPF_SPLIT3" and the BLAZECHAIN / DWBLOCK / SHUFDOWN / SHUFUNIT / YSTEM2 parameter blocks)."""
    m = np.asarray(m, dtype=np.float32)
    n, K = m.shape
    assert K % 32 == 0, (n, K)
    return _f32_blob(split3_bf16(m).reshape(3, n, K // 32, 32).transpose(2, 0, 1, 3))


def pack_rowblock_x6(m):
    """"row-block" split-bf16 planes of an fp32 matrix m[g, k], both multiples of 32: [g / 32][3 planes][k / 32][32][32],
    element [R][plane][ks][g'][k'] = piece `plane` of m[32 * R + g', 32 * ks + k'] (split3_bf16).  The expand matrices,
    in the fragment order of the whole-block kernels (include/facepath.h, "DWBLOCK", "SHUFDOWN", "SHUFUNIT")."""
    m = np.asarray(m, dtype=np.float32)
    g, k = m.shape
    assert g % 32 == 0 and k % 32 == 0, (g, k)
    return _f32_blob(split3_bf16(m).reshape(3, g // 32, 32, k // 32, 32).transpose(1, 0, 3, 2, 4))


def pad_vec(v, n, fill=0.0):
    v = np.asarray(v, dtype=np.float32).reshape(-1)
    out = np.full((n,), fill, dtype=np.float32)
    out[:v.shape[0]] = v
    return out


def affine_rows(aff, c):
    """(scale, bias) -> the rows [2][c], zero padded."""
    return np.concatenate([pad_vec(aff[0], c), pad_vec(aff[1], c)])


def dw_rows(w, aff, slope, c):
    """The parameter block [12][c] of a depthwise 3x3 Conv_block: nine taps (pack_dw_weight), BN scale, BN bias, PReLU
    slope (zeros where there is no PReLU: slope = None)."""
    return np.concatenate([pack_dw_weight(w, c), affine_rows(aff, c),
                           np.zeros(c, np.float32) if slope is None else pad_vec(slope, c)])


def bn_affine(gamma, beta, mean, var, eps):
    """Eval-mode BatchNorm as y = x*s + b (mobile_facenet.py:48-49, common.py:50)."""
    gamma, beta, mean, var = (np.asarray(t, dtype=np.float32) for t in (gamma, beta, mean, var))
    s = gamma / np.sqrt(var + np.float32(eps))
    return s.astype(np.float32), (beta - mean * s).astype(np.float32)


class PlanBuilder:
    def __init__(self, N, dwblock_shapes=None):
        self.N = int(N)
        self.dwblock_shapes = dwblock_shapes   # Mobile-FaceNet: map sizes whose Depth_Wise blocks may take the fp32 whole-block
                                               # kernel (None: Depth_Wise.block_policy(N))
        self.ops = []
        self.wchunks = []
        self.w_floats = 0
        self.arena = Arena()
        self.peak = 0
        self.alg_bytes = []   # op-granular algorithmic bytes per op, from LOGICAL channel counts
        self.rowpad_free = {}   # (H, W, C) -> row-padded buffers released by free()
        self.rowpad_bufs = []   # every row-padded buffer (offsets relative to the row-padded region until finish())
        self.rowpad_top = 0
        self.rowpad_end = 0
        self.has_rowpad = False
        self._placed = False
        self.windows = []       # [(op index, row_lo, row_end)]: the row windows of window() (applied by CompiledPlan)
        self.x6_all = False     # True: every conv the split-MFMA kernels accept runs there, whatever the size policy says
                                # (x6_policy; set by the network that emits the plan: Inception-ResNet-v1)

    # ---- memory ----
    def new_buf(self, H, W, C, peek=False):
        """peek: the buffer the next new_buf(H, W, C) returns, not allocated (the output of an op that is only probed:
        take() allocates it)."""
        C = cpad(C)
        if peek:
            return Buf(H, W, C, *self.arena.place(self.N * H * W * C))
        off, size = self.arena.alloc(self.N * H * W * C)
        self.peak = max(self.peak, self.arena.top)
        return Buf(H, W, C, off, size)

    def take(self, peeked):
        """Allocate the buffer a peek named (nothing may have been allocated since the peek)."""
        if peeked.rowpad:
            buf = self.new_buf_rowpad(peeked.H, peeked.W, peeked.C, peeked.dedicated)
        else:
            buf = self.new_buf(peeked.H, peeked.W, peeked.C)
        assert buf == peeked, (buf, peeked)
        return buf

    def new_buf_rowpad(self, H, W, C, dedicated=False, peek=False):
        """A buffer in the row-padded layout of include/facepath.h (one zero pixel after every row, a zero row above and
        below every image): 3x3 windows read it without bounds checks.  The pads must stay zero for the life of the
        plan, so these buffers live in a region of their own behind the recycled arena (no op ever writes there except
        through a row-padded view: a recycled block would carry another tensor's data into the pads), free() keeps
        them for the next row-padded buffer of the same shape, and the arena of such a plan starts zeroed.  Offsets are
        relative to that region until finish() places it.  dedicated: a buffer of its own that free() never hands out
        again (the output of a row-windowed op, window()).  peek: as new_buf's."""
        assert not self._placed, "plan already finished"
        C = cpad(C)
        pool = self.rowpad_free.get((H, W, C))
        if pool and not dedicated:
            return pool[-1] if peek else pool.pop()
        ns = ((H + 2) * (W + 1) + 1) * C
        base = self.rowpad_top
        buf = Buf(H, W, C, base + (W + 2) * C, self.N * ns, ns_=ns, rowpad=True, dedicated=dedicated)
        if peek:
            return buf
        self.rowpad_end = base + self.N * ns           # exact end of the region (the arena size is exact too)
        self.rowpad_top += round_up(self.N * ns, 64)
        self.has_rowpad = True
        self.rowpad_bufs.append(buf)
        return buf

    def new_raw(self, floats_per_image):
        """An untyped per-image region (heads / decoded tensors); returns (offset, size) in floats."""
        off, size = self.arena.alloc(self.N * floats_per_image)
        self.peak = max(self.peak, self.arena.top)
        return off, size

    @staticmethod
    def new_shape(H, W):
        """A shape-only stand-in for an input that is not an arena buffer (u8 frames read by a *_U8 op)."""
        return Buf(H, W, 0, 0, 0)

    def free(self, buf):
        if buf.dedicated:
            return
        if buf.rowpad:
            self.rowpad_free.setdefault((buf.H, buf.W, buf.C), []).append(buf)
        else:
            self.arena.release(buf.off, buf.size)

    def add_weight(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.float32).reshape(-1)
        off = self.w_floats
        self.wchunks.append(arr)
        pad = round_up(arr.size, 4) - arr.size   # keep every chunk 16-byte aligned
        if pad:
            self.wchunks.append(np.zeros(pad, dtype=np.float32))
        self.w_floats += arr.size + pad
        return off

    def window(self, lo, end):
        """Give the last emitted op the output row window [lo, end) (include/facepath.h "Row windows").  Its output must be a
        dedicated buffer: the rows outside the window are left as the plan's unrestricted runs wrote them."""
        op = self.ops[-1]
        assert 0 <= lo < end <= op.OH and (lo, end) != (0, op.OH)
        self.windows.append((len(self.ops) - 1, int(lo), int(end)))

    # ---- op emission ----
    @staticmethod
    def probe(op):
        """The kernel the op's launcher picks for it (its dry run, fp_op_kernel_name), or None if the launcher refuses it.
        The launchers alone decide which ops a kernel takes: an emitter fills in every field of a fused or split op, with
        weight offsets that are multiples of 4 until the weights are packed (add_weight keeps every chunk 16-byte aligned),
        asks, and emits that form only if the answer is a kernel."""
        name = L.load().fp_op_kernel_name(C.byref(op)).decode()
        return None if name == "?" else name

    @staticmethod
    def _offsets(op, *present):
        """Provisional weight offsets (0, a multiple of 4) for the weight / scale / bias / slope blocks that are present,
        -1 for the others."""
        op.w_off, op.scale_off, op.bias_off, op.slope_off = (0 if p else -1 for p in present)

    def _base(self, kind, x, out, OH, OW):
        if x.up is not None and kind != L.OP_CONV:      # only conv() knows how to read a folded upsample
            self.materialise_up(x)
        op = L.FpOp()
        op.kind = kind
        op.N = self.N
        op.H, op.W = x.H, x.W
        op.OH, op.OW = OH, OW
        op.Cin = x.C
        op.in_ld = x.buf.ld
        op.in_ns = x.buf.ns
        op.in_off = x.buf.off + x.coff
        op.out_ld = out.buf.ld
        op.out_ns = out.buf.ns
        op.out_off = out.buf.off + out.coff
        op.out_cmul = out.cmul
        op.KH = op.KW = 1
        op.stride = 1
        op.w_off = op.scale_off = op.bias_off = op.slope_off = -1
        assert x.cmul == 1, "inputs must be dense channel slices"
        assert out.H == OH and out.W == OW, (out.H, out.W, OH, OW)
        for v, bit in ((x, L.OPF_IN_ROWPAD), (out, L.OPF_OUT_ROWPAD)):
            if v.buf.rowpad:
                assert v.coff == 0 and v.C == v.buf.C and v.cmul == 1, "row-padded buffers are used whole"
                op.flags |= bit
        return op

    def _base_u8(self, kind, u8, out, OH, OW):
        """_base for an op that reads u8 frames itself: u8 = (H, W, frame_h, frame_w, ext_index), the H x W letterbox canvas is
        never materialised (external buffers ext_index .. ext_index + 2 = frames, tap tables, LUT; fp_plan_run_ext)."""
        H, W, fh, fw, ext_index = u8
        op = L.FpOp()
        op.kind, op.N, op.H, op.W, op.OH, op.OW = kind, self.N, H, W, OH, OW
        op.Cin, op.in_ld, op.in_ns, op.in_off = 3, 3, fh * fw * 3, ext_index
        op.out_ld, op.out_ns, op.out_off, op.out_cmul = out.buf.ld, out.buf.ns, out.buf.off + out.coff, 1
        if out.buf.rowpad:
            op.flags |= L.OPF_OUT_ROWPAD
        op.w_off = op.scale_off = op.bias_off = op.slope_off = -1
        return op

    @staticmethod
    def _set_window(op, k, stride, pad):
        """The op's window: k = KH = KW or (KH, KW), pad = pad_t = pad_l or (pad_t, pad_l)."""
        op.KH, op.KW = (k, k) if np.isscalar(k) else k
        op.stride = stride
        op.pad_t, op.pad_l = (pad, pad) if np.isscalar(pad) else pad

    @staticmethod
    def _set_res(op, v, C=None):
        """The op's second tensor (residual, shortcut, pooled or half-size map) = the View v, C (default: all) of its channels."""
        op.res_ld, op.res_ns, op.res_off = v.buf.ld, v.buf.ns, v.buf.off + v.coff
        op.res_C, op.res_H, op.res_W = v.C if C is None else C, v.H, v.W

    def _epilogue(self, op, c, scale=None, bias=None, slope=None):
        """Append the optional scale / bias / slope vectors (c channels) of a plain epilogue and set the op's three offsets."""
        for field, v in (("scale_off", scale), ("bias_off", bias), ("slope_off", slope)):
            if v is not None:
                setattr(op, field, self.add_weight(pad_vec(v, c)))

    # ---- split-MFMA policy: which convs the split kernels (csrc/pwx6.hip) should run when they take them ----
    # Master switch of the bf16x6 split-MFMA kernels (csrc/split.h): False = every GEMM on the fp32 MFMA (the fmaf-chain
    # kernels of rounds 1-3).  Mobile-FaceNet's Depth_Wise.X6 is this attribute.
    X6 = True
    # Pointwise convs with K >= PW_X6_MIN_K input channels on the split kernel.
    # (YOLOv5n-face forward at batch 256: 18.2 ms with 128, 17.0 ms with 64, 17.5 ms with 32.)
    PW_X6_MIN_K = 64
    # Dense 3x3 convs (pad 1, stride 1 / 2) with at least this many input channels on the split kernel as well,
    # and those on 8 / 16 / 24 input channels, with K flattened over (tap, channel) (YOLOv5n-face's stem_2b, 16 -> 32
    # stride 2 at 320x320: 945 us on conv_igemm_kernel)
    CONV3_X6_MIN_K = 32
    X6_SMALL_K_MIN_PIXELS = 400   # below 128 input channels only on maps of at least 20 x 20 (measured on YOLOv5-face; the
                                  # small-map 1x1 convs of BlazeFace stay on the fp32-MFMA kernels)
    X6_MIN_COUT = 48              # from 32 input channels on, at least 48 outputs (32: a third of the three-tile chunk would
                                  # be padding)
    UP2_FOLD = True               # nn.Upsample + Concat in front of a pointwise conv as operand addressing

    def x6_policy(self, x, out, kh, kw, stride, pad):
        """True if the size policy above sends this conv to the split kernels (where the launcher takes it).  The policy
        covers the 1x1 and 3x3-pad-1 shapes; every other window, and every conv of an x6_all plan, goes wherever the
        launcher takes it."""
        if not self.X6:
            return False
        k1 = (kh, kw, stride, *pad) == (1, 1, 1, 0, 0)
        k3 = (kh, kw, *pad) == (3, 3, 1, 1)
        if self.x6_all or not (k1 or k3):
            return True
        if k1 and x.C < self.PW_X6_MIN_K:
            return False
        if k3 and x.C < self.CONV3_X6_MIN_K and x.C not in (8, 16, 24):
            return False
        if x.C < 128 and out.H * out.W < self.X6_SMALL_K_MIN_PIXELS:
            return False
        return x.C < 32 or out.C >= self.X6_MIN_COUT

    @staticmethod
    def x6_tiles(cout):
        """(16-column tiles per chunk, padded width) of the split conv's weight planes: general_tiles (csrc/pwx6.hip)."""
        nt = (cout + 15) // 16
        if nt <= 2:
            per = 2
        elif nt <= 3:
            per = 3
        elif nt <= 4:
            per = 4
        elif nt <= 6:
            per = 6
        else:
            p6, p4 = (nt + 5) // 6 * 6, (nt + 3) // 4 * 4
            per = 6 if p6 <= p4 else 4
        return per, (nt + per - 1) // per * per * 16

    def materialise_up(self, x):
        """Write the upsampled slice of a view that still carries `up` (a consumer that cannot fold it)."""
        if x.up is not None:
            u, x.up = x.up, None
            self.upsample2x(u, View(x.buf, x.coff, u.C))

    @classmethod
    def conv_weights(cls, w, cin_phys, cout_phys, flags):
        """The packed weights (at w_off) of a conv op with these flags: OIHW w for cin_phys input and cout_phys output channels."""
        cout, cin, kh, kw = w.shape
        if not flags & L.OPF_SPLIT3:
            return pack_conv_weight(w, cin_phys, cout_phys)
        taps = np.asarray(w, np.float32).reshape(cout, cin, kh * kw).transpose(0, 2, 1)        # [cout][tap][channel]
        if flags & L.OPF_OUT_DW:
            # csrc/stemdw.hip: k = tap * 3 + channel in ONE 32-k slab, planes [channel tile of 16][plane][16][32]
            flat = np.zeros((cout, 32), np.float32)
            flat[:, :kh * kw * cin] = taps.reshape(cout, -1)
            return _f32_blob(split3_bf16(flat).reshape(3, cout // 16, 16, 32).transpose(1, 0, 2, 3))
        # FP_OPF_SPLIT3 on FP_OP_CONV (include/facepath.h): k = tap * pitch + channel with pitch = Cin_phys below 32 channels
        # (flat) and Cin padded to whole 32-channel slabs from there on (per tap: [tap][slab][3][Npad][32] is the k-slab
        # layout of that k); zeros behind the last k and in the padding of Cout to whole chunks
        pitch = cin_phys if cin_phys < 32 else round_up(cin_phys, 32)
        wt = np.zeros((cout, kh * kw, pitch), np.float32)
        wt[:, :, :cin] = taps
        full = np.zeros((cls.x6_tiles(cout_phys)[1], round_up(kh * kw * pitch, 32)), np.float32)
        full[:cout, :kh * kw * pitch] = wt.reshape(cout, -1)
        return pack_kslab_x6(full)

    def conv(self, x, w, out, stride=1, pad=(0, 0), scale=None, bias=None, slope=None,
             act=L.ACT_NONE, res=None, res_mode=L.RES_NONE, n_convs=1, out_dw=None):
        """Dense conv (OIHW weight); out is a View whose C >= Cout (extra channels get zeros).  On the split kernels
        (FP_OPF_SPLIT3) when x6_policy says so and the launcher takes the op, reading a folded upsample of x (FP_OPF_IN_UP2)
        if the launcher takes that too; else on the fp32 kernels.
        out_dw = (weights [C,1,3,3], (scale, bias), PReLU slope) of a depthwise 3x3 stride-1 pad-1 Conv_block computed behind
        the conv in the same kernel (FP_OPF_OUT_DW: Mobile-FaceNet's conv1 + conv2_dw); `out` then receives ITS output.  Returns
        None (nothing emitted) if the launcher refuses that op."""
        cout, cin, kh, kw = w.shape
        assert cin <= x.C, (cin, x.C)
        if res_mode == L.RES_SHUFFLE2:   # out is the dense view of the conv's own Cout channels; 2*Cout are written
            assert out.cmul == 1 and out.coff + 2 * out.C <= out.buf.ld and res is not None and res.C >= out.C
        if res_mode != L.RES_NONE:
            assert res is not None and res.cmul == 1

        def make(flags):
            op = self._base(L.OP_CONV, x, out, out.H, out.W)
            op.flags |= flags
            op.Cout = out.C
            self._set_window(op, (kh, kw), stride, pad)
            op.act, op.res_mode = act, res_mode
            if cin == 3 and x.C == 4 and x.buf.ld == 4:   # 3-channel image padded to 16-byte pixels: the pad channel's weights are zero
                op.flags |= L.OPF_IN_C3
            self._offsets(op, True, scale is not None, bias is not None, slope is not None)
            if flags & L.OPF_IN_UP2:
                assert x.up.cmul == 1 and not x.up.buf.rowpad, "the op reads the half-size map as a dense slice"
                self._set_res(op, x.up)
            elif res_mode != L.RES_NONE:
                self._set_res(op, res, min(res.C, out.C))
            return op

        flags = 0
        if out_dw is not None:
            flags = L.OPF_OUT_DW | (L.OPF_SPLIT3 if self.X6 else 0)
            if self.probe(make(flags)) is None:
                return None
        elif self.x6_policy(x, out, kh, kw, stride, pad):
            if (x.up is not None and self.UP2_FOLD and res_mode == L.RES_NONE and
                    self.probe(make(L.OPF_SPLIT3 | L.OPF_IN_UP2)) is not None):
                flags = L.OPF_SPLIT3 | L.OPF_IN_UP2
            elif self.probe(make(L.OPF_SPLIT3)) is not None:
                flags = L.OPF_SPLIT3
        if not flags & L.OPF_IN_UP2:
            self.materialise_up(x)
        op = make(flags)
        op.w_off = self.add_weight(self.conv_weights(w, x.C, out.C, op.flags))
        self._epilogue(op, out.C, scale, bias, slope if out_dw is None else None)
        if out_dw is not None:     # the conv's slopes followed by the depthwise block
            assert tuple(out_dw[0].shape) == (out.C, 1, 3, 3)
            op.slope_off = self.add_weight(np.concatenate([pad_vec(slope, out.C), dw_rows(*out_dw, out.C)]))
        self.ops.append(op)
        # n_convs > 1: several reference convs on the same input merged into one op (their outputs concatenated): the
        # op-granular model counts the input once per conv
        # (FP_OPF_OUT_DW: + the depthwise conv's input and output, SURVEY 8d counts every conv)
        self.alg_bytes.append(4 * self.N * (n_convs * x.H * x.W * cin + out.H * out.W * cout +
                                            (2 * out.H * out.W * cout if out_dw is not None else 0)))
        return out

    def dwconv(self, x, w, out, stride=1, pad=(0, 0), scale=None, bias=None, slope=None, act=L.ACT_NONE):
        c, _, kh, kw = w.shape
        assert c <= x.C and out.C == x.C and out.cmul == 1
        op = self._base(L.OP_DWCONV, x, out, out.H, out.W)
        op.Cout = x.C
        self._set_window(op, (kh, kw), stride, pad)
        op.act = act
        op.w_off = self.add_weight(pack_dw_weight(w, x.C))
        self._epilogue(op, x.C, scale, bias, slope)
        self.ops.append(op)
        self.alg_bytes.append(4 * self.N * (x.H * x.W * c + out.H * out.W * c))
        return out

    def blazeblock_op(self, x, out, cin, stride):
        """The FP_OP_BLAZEBLOCK op of a cin -> out.C block on view x, weights not yet packed (blazeblock(); probe())."""
        op = self._base(L.OP_BLAZEBLOCK, x, out, out.H, out.W)
        op.Cout = out.C
        self._set_window(op, 3, stride, 1 if stride == 1 else 0)
        op.res_C = min(cin, x.C)
        self._offsets(op, True, True, True, True)
        return op

    def blazeblock(self, x, wd, bd, wp, bp, out, stride):
        """Fused BlazeBlock (blazeface.py:12-47): dw3x3(stride) -> 1x1 -> + shortcut -> ReLU in one kernel."""
        cin = wd.shape[0]
        cout = wp.shape[0]
        assert out.cmul == 1 and out.coff == 0 and out.buf.ld == out.C
        op = self.blazeblock_op(x, out, cin, stride)
        op.w_off = self.add_weight(pack_dw_weight(wd, x.C))
        op.scale_off = self.add_weight(pad_vec(bd, x.C, 0.0))
        op.slope_off = self.add_weight(pack_conv_weight(wp, x.C, out.C))
        op.bias_off = self.add_weight(pad_vec(bp, out.C, 0.0))
        self.ops.append(op)
        opix = out.H * out.W
        self.alg_bytes.append(4 * self.N * (x.H * x.W * cin + opix * cin + opix * cin + opix * cout))
        return out

    def blazepair_op(self, x, out, stride):
        """The FP_OP_BLAZEPAIR op of two BlazeBlocks on the row-padded view x, the second of stride `stride`, weights not yet
        packed (blazepair(), blazepair_s2(); probe())."""
        op = self._base(L.OP_BLAZEPAIR, x, out, out.H, out.W)
        op.Cout = out.C
        self._set_window(op, 3, stride, 1 if stride == 1 else 0)
        op.act = L.ACT_RELU
        op.res_mode = L.RES_ADD_BEFORE_ACT if stride == 1 else L.RES_POOL2_BEFORE_ACT
        self._set_res(op, x, 24)      # the shortcut view IS the input view
        self._offsets(op, True, True, True, True)
        return op

    def _blazepair(self, x, blocks, out, stride, alg_bytes):
        """blazepair() / blazepair_s2(): the second block has this stride and wp2.shape[0] outputs (24 at stride 1)."""
        (wd1, bd1, wp1, bp1), (wd2, bd2, wp2, bp2) = blocks
        cout2 = wp2.shape[0]
        assert wd1.shape == (24, 1, 3, 3) and wp1.shape[:2] == (24, 24) and wd2.shape == (24, 1, 3, 3) and wp2.shape[1] == 24
        assert cout2 == 24 if stride == 1 else out.C == cout2
        op = self.blazepair_op(x, out, stride)
        if self.probe(op) is None:
            return None
        op.w_off = self.add_weight(np.concatenate([pack_dw_weight(wd1, 24), pack_dw_weight(wd2, 24)]))
        op.scale_off = self.add_weight(np.concatenate([pad_vec(bd1, 24), pad_vec(bd2, 24)]))
        op.slope_off = self.add_weight(np.concatenate([pack_conv_weight(wp1, 24, 24), pack_conv_weight(wp2, 24, cout2)]))
        op.bias_off = self.add_weight(np.concatenate([pad_vec(bp1, 24), pad_vec(bp2, cout2)]))
        self.ops.append(op)
        self.alg_bytes.append(alg_bytes)
        return out

    def blazepair(self, x, blocks, out):
        """Two consecutive stride-1 24 -> 24 BlazeBlocks (blazeface.py:12-47) as ONE op (FP_OP_BLAZEPAIR): blocks =
        ((dw_w, dw_b, pw_w, pw_b), (dw_w, dw_b, pw_w, pw_b)); the tensor between them never reaches HBM.  None (nothing
        emitted) if the launcher refuses the op (csrc/blazepair.hip: a row-padded map 128 or 64 pixels wide)."""
        pix = out.H * out.W
        return self._blazepair(x, blocks, out, 1, 2 * 4 * self.N * pix * 24 * 4)      # two blocks, four tensor passes each

    def blazepair_s2(self, x, blocks, out):
        """A stride-1 24 -> 24 BlazeBlock and the STRIDE-2 BlazeBlock behind it (blazeface.py:12-47) as ONE op (FP_OP_BLAZEPAIR
        with stride = 2): blocks = ((dw_w, dw_b, pw_w, pw_b) of the stride-1 block, the same of the stride-2 block); the
        full-size tensor between them never reaches HBM, `out` is the half-size map (dense or row-padded, ld = its channels).
        None (nothing emitted) if the launcher refuses the op (csrc/blazepair.hip)."""
        pix, opix, cout2 = x.H * x.W, out.H * out.W, blocks[1][2].shape[0]
        # the stride-1 block's four tensor passes + the stride-2 block's (input, dw output, 1x1 input, output)
        return self._blazepair(x, blocks, out, 2, 4 * self.N * (pix * 24 * 4 + pix * 24 + opix * 24 + opix * 24 + opix * cout2))

    def blazechain(self, x, blocks, out):
        """A run of stride-1 96 -> 96 BlazeBlocks on the 16 x 16 map (blazeface.py:12-47,146-152) as ONE op
        (FP_OP_BLAZECHAIN): blocks = ((dw_w, dw_b, pw_w, pw_b), ...); the tensors between them never reach HBM.  The 1x1
        weights go in as k-slab planes (pack_kslab_x6): include/facepath.h BLAZECHAIN.
        None (nothing emitted) if the launcher refuses the op (csrc/blazechain.hip)."""
        for wd, bd, wp, bp in blocks:
            assert wd.shape == (96, 1, 3, 3) and wp.shape[:2] == (96, 96)
        op = self._base(L.OP_BLAZECHAIN, x, out, out.H, out.W)
        op.Cout = out.C
        self._set_window(op, 3, 1, 1)
        op.act, op.res_mode = L.ACT_RELU, L.RES_ADD_BEFORE_ACT
        self._set_res(op, x, 96)
        op.Cmid = len(blocks)
        op.flags |= L.OPF_SPLIT3
        self._offsets(op, True, False, False, False)
        if self.probe(op) is None:
            return None
        chunks = []
        for wd, bd, wp, bp in blocks:
            par = np.zeros(1280, np.float32)
            par[:864] = pack_dw_weight(wd, 96)
            par[864:960] = pad_vec(bd, 96)
            par[960:1056] = pad_vec(bp, 96)
            chunks += [par, pack_kslab_x6(_mat(wp))]
        op.w_off = self.add_weight(np.concatenate(chunks))
        self.ops.append(op)
        self.alg_bytes.append(len(blocks) * 4 * self.N * 256 * 96 * 4)     # four tensor passes per block
        return out

    # The dw -> 1x1 op with its 1x1 on the split MFMA (csrc/dwpwx6.hip) for 128 outputs only: measured on YOLOv5n-face (256 images): 128 -> 128 at 40x40 278 -> 246 us, 80x80 stride 2
    # 367 / 298 -> 345 / 248; 64 -> 64 at 80x80 420 -> 440 (the depthwise phase, not the 1x1, bounds the narrow form)
    DWPW_X6_COUT = 128

    def dwpw(self, x, dw_w, dw_scale, dw_bias, dw_slope, pw_w, pw_scale, pw_bias, out, stride, res=None,
             out_slope=None, out_act=L.ACT_NONE, shuffle=False):
        """Fused Depth_Wise tail (mobile_facenet.py:72-85): dw3x3 stride s (+BN affine, +PReLU) -> 1x1 (+BN affine)
        [+ res], or -- with out_slope -- a depthwise Conv_block followed by a 1x1 Conv_block (BN + PReLU on both:
        conv2_dw -> conv_23.conv, mobile_facenet.py:117-118,70).  x has G (multiple of 64) channels.  The 1x1 runs on the
        split MFMA (FP_OPF_SPLIT3, its weights as k-slab planes: csrc/dwpwx6.hip) when X6 and DWPW_X6_COUT allow it and
        the launcher takes the op."""
        G = dw_w.shape[0]
        cout, cin = pw_w.shape[0], pw_w.shape[1]
        assert cin == G == x.C and G % 64 == 0 and out.cmul == 1
        # out_act = ACT_SILU: SiLU on the 1x1 output; shuffle: `out` is the dense view of the conv's own Cout channels
        # inside a buffer that receives 2*Cout (out[2n] = res[n], out[2n+1] = y[n]: ShuffleV2Block's cat + shuffle)
        if shuffle:
            assert res is not None and res.C >= out.C and out.coff + 2 * out.C <= out.buf.ld
        else:
            assert out.coff == 0 and out.buf.ld == out.C or out_act != L.ACT_NONE
        assert res is None or (res.cmul == 1 and out_slope is None)

        def make(flags):
            op = self._base(L.OP_DWPW, x, out, out.H, out.W)
            op.flags |= flags
            op.act2 = out_act
            op.Cout = out.C
            self._set_window(op, 3, stride, 1)
            op.act = L.ACT_PRELU if dw_slope is not None else L.ACT_NONE
            op.w_off, op.slope_off, op.bias_off = 0, 0, 0 if out_slope is not None else -1
            if res is not None:
                op.res_mode = L.RES_SHUFFLE2 if shuffle else L.RES_ADD_AFTER_ACT
                self._set_res(op, res, min(res.C, out.C))
            return op

        split = self.X6 and out.C == self.DWPW_X6_COUT and self.probe(make(L.OPF_SPLIT3)) is not None
        op = make(L.OPF_SPLIT3 if split else 0)
        op.w_off = self.add_weight(dw_rows(dw_w, (dw_scale, dw_bias), dw_slope, G))
        if split:
            full = np.zeros((out.C, G), np.float32)
            full[:cout] = _mat(pw_w)
            wp = pack_kslab_x6(full)
        else:
            wp = pack_conv_weight(pw_w, G, out.C)
        c4 = round_up(out.C, 4)
        op.slope_off = self.add_weight(np.concatenate([wp, affine_rows((pw_scale, pw_bias), c4)]))
        if out_slope is not None:
            op.bias_off = self.add_weight(pad_vec(out_slope, c4))
        self.ops.append(op)
        opix = out.H * out.W
        self.alg_bytes.append(4 * self.N * (x.H * x.W * G + opix * G + opix * G + opix * cout))
        return out

    def dwblock(self, x, e_w, e_aff, e_slope, dw_w, dw_aff, dw_slope, pw_w, pw_aff, out, residual, stride=1, fp32=True):
        """A whole Depth_Wise block (mobile_facenet.py:67-88) as ONE op (FP_OP_DWBLOCK): 1x1 expand + BN + PReLU -> dw3x3
        (stride) + BN + PReLU -> 1x1 project + BN [+ x]; the expanded tensor stays in LDS.  *_aff = (scale, bias) of the
        eval-mode BatchNorm.  The split form (FP_OPF_SPLIT3, csrc/dwblockx6.hip) when X6 is on and the launcher takes it,
        else the fp32 form (csrc/dwblock.hip) if the caller's policy allows it (`fp32`) and the launcher takes it, else None
        (nothing emitted)."""
        cmid, cin = e_w.shape[0], e_w.shape[1]
        cout = pw_w.shape[0]
        assert dw_w.shape == (cmid, 1, 3, 3) and pw_w.shape[1] == cmid
        assert out.coff == 0 and out.C == cout

        def make(flags):
            op = self._base(L.OP_DWBLOCK, x, out, out.H, out.W)
            op.flags |= flags
            op.Cout, op.Cmid = cout, cmid
            self._set_window(op, 3, stride, 1)
            op.act = L.ACT_PRELU
            self._offsets(op, True, True, False, True)
            if residual:
                op.res_mode = L.RES_ADD_AFTER_ACT
                self._set_res(op, x, cin)
            return op

        forms = ([L.OPF_SPLIT3] if self.X6 else []) + ([0] if fp32 else [])
        split = next((f for f in forms if self.probe(make(f)) is not None), None)
        if split is None:
            return None
        op = make(split)
        if split:      # include/facepath.h, DWBLOCK: the expand matrix in row blocks, the projection in k-slabs
            op.w_off = self.add_weight(pack_rowblock_x6(_mat(e_w)))
            wp = pack_kslab_x6(_mat(pw_w))
        else:
            op.w_off = self.add_weight(pack_conv_weight(e_w, cin, cmid))
            wp = pack_conv_weight(pw_w, cmid, cout)
        op.scale_off = self.add_weight(np.concatenate([affine_rows(e_aff, cmid), pad_vec(e_slope, cmid),
                                                       dw_rows(dw_w, dw_aff, dw_slope, cmid)]))
        op.slope_off = self.add_weight(np.concatenate([wp, affine_rows(pw_aff, cout)]))
        pix, opix = x.H * x.W, out.H * out.W
        self.ops.append(op)
        # the three convs of the block, each input once + output once
        self.alg_bytes.append(4 * self.N * (pix * (cin + cmid) + (pix + opix) * cmid + opix * (cmid + cout)))
        return out

    def _shuf_op(self, kind, x, out, cb, stride):
        """The FP_OP_SHUFDOWN / FP_OP_SHUFUNIT op with branch width cb, weights not yet packed; None if X6 is off or the
        launcher refuses it."""
        op = self._base(kind, x, out, out.H, out.W)
        op.Cout, op.Cmid = 2 * cb, cb
        self._set_window(op, 3, stride, 1)
        op.act = op.act2 = L.ACT_SILU
        op.flags |= L.OPF_SPLIT3
        self._offsets(op, True, False, False, False)
        return op if self.X6 and self.probe(op) is not None else None

    @staticmethod
    def _shuf_branch2(pw1, pw1_aff, dw2, dw2_aff, pw2, pw2_aff):
        """Branch 2 of a ShuffleV2Block in its parameter block (facepath.h "SHUFUNIT"; the tail of "SHUFDOWN"): the first 1x1
        in row blocks + affine, the depthwise taps + affine, the second 1x1 in k-slabs + affine."""
        cb = pw1.shape[0]
        return [pack_rowblock_x6(_mat(pw1)), affine_rows(pw1_aff, cb), pack_dw_weight(dw2, cb), affine_rows(dw2_aff, cb),
                pack_kslab_x6(_mat(pw2)), affine_rows(pw2_aff, cb)]

    def shufdown(self, x, b1_dw, b1_dw_aff, b1_pw, b1_pw_aff, pw1, pw1_aff, dw2, dw2_aff, pw2, pw2_aff, out):
        """A whole stride-2 ShuffleV2Block (y5/models/common.py:127-176) as ONE op (FP_OP_SHUFDOWN, csrc/shufdown.hip):
        branch1 = dw3x3 s2 + BN -> 1x1 + BN + SiLU, branch2 = 1x1 + BN + SiLU -> dw3x3 s2 + BN -> 1x1 + BN + SiLU,
        out[2c] = branch1[c], out[2c + 1] = branch2[c].  *_aff = (scale, bias) of the eval-mode BatchNorm.  The parameter block's
        layout is facepath.h "SHUFDOWN".  None (nothing emitted) if X6 is off or the launcher refuses the op."""
        cin, cb = x.C, pw1.shape[0]
        assert b1_dw.shape == (cin, 1, 3, 3) and b1_pw.shape[:2] == (cb, cin) and pw1.shape[:2] == (cb, cin)
        assert dw2.shape == (cb, 1, 3, 3) and pw2.shape[:2] == (cb, cb) and out.C == 2 * cb
        op = self._shuf_op(L.OP_SHUFDOWN, x, out, cb, 2)
        if op is None:
            return None
        blob = [pack_dw_weight(b1_dw, cin), affine_rows(b1_dw_aff, cin), pack_kslab_x6(_mat(b1_pw)), affine_rows(b1_pw_aff, cb)]
        op.w_off = self.add_weight(np.concatenate(blob + self._shuf_branch2(pw1, pw1_aff, dw2, dw2_aff, pw2, pw2_aff)))
        self.ops.append(op)
        pix, opix = x.H * x.W, out.H * out.W
        # the five convs of the block, each input once + output once
        self.alg_bytes.append(4 * self.N * ((pix + opix) * cin + opix * (cin + cb) + pix * (cin + cb) + (pix + opix) * cb + opix * 2 * cb))
        return out

    def shufunit(self, x, pw1, pw1_aff, dw2, dw2_aff, pw2, pw2_aff, out):
        """A whole stride-1 ShuffleV2Block (y5/models/common.py:127-176) as ONE op (FP_OP_SHUFUNIT, csrc/shufdown.hip):
        x1, x2 = x.chunk(2); branch2(x2) = 1x1 + BN + SiLU -> dw3x3 + BN -> 1x1 + BN + SiLU; out[2c] = x1[c], out[2c + 1] = branch2[c].
        The parameter block's layout is facepath.h "SHUFUNIT".  None (nothing emitted) if X6 is off or the launcher refuses
        the op."""
        cb = pw1.shape[0]
        assert pw1.shape[:2] == (cb, cb) and dw2.shape == (cb, 1, 3, 3) and pw2.shape[:2] == (cb, cb) and out.C == 2 * cb
        op = self._shuf_op(L.OP_SHUFUNIT, x, out, cb, 1)
        if op is None:
            return None
        op.w_off = self.add_weight(np.concatenate(self._shuf_branch2(pw1, pw1_aff, dw2, dw2_aff, pw2, pw2_aff)))
        self.ops.append(op)
        pix = x.H * x.W
        self.alg_bytes.append(4 * self.N * pix * 6 * cb)     # three convs of cb channels, input once + output once each
        return out

    @staticmethod
    def pack_stem5_x6(w):
        """[24, 3, 5, 5] -> the three bf16 planes of stem5_u8_x6_kernel (csrc/stem.hip): [3 slabs][2 channel tiles][3 planes][16][32]
        with k = 16 (ky - 2 slab) + 3 kx + c inside a slab (every ky padded to 16, the sixth ky and channels 24 .. 31 zero)."""
        w = np.asarray(w, dtype=np.float32)
        assert w.shape == (24, 3, 5, 5)
        full = np.zeros((3, 2, 16, 32), dtype=np.float32)               # [slab][nt][channel][k]
        for ky in range(5):
            for kx in range(5):
                for c in range(3):
                    k = 16 * (ky % 2) + 3 * kx + c
                    for co in range(24):
                        full[ky // 2, co // 16, co % 16, k] = w[co, c, ky, kx]
        return _f32_blob(split3_bf16(full).transpose(1, 2, 0, 3, 4))    # [3 planes][slab][nt][16][32] -> [slab][nt][plane][16][32]

    def stem_u8(self, u8, w, out, pad=(0, 0), scale=None, bias=None, slope=None, act=L.ACT_NONE, split=False):
        """First conv of a network reading u8 frames itself (FP_OP_STEM_U8): KxK (3 or 5) stride 2, Cout <= 64, dense
        output buffer.  u8 = (H, W, frame_h, frame_w, ext_index): the H x W letterbox canvas is resampled from the
        frames while the conv's input tile is staged (_base_u8).
        w is the [Cout, 3, K, K] weight; it is packed for a 4-channel pixel like the fp32-canvas form."""
        H, W = u8[:2]
        cout, cin, kh, kw = w.shape
        assert cin == 3 and kh == kw and kh in (3, 5) and out.cmul == 1 and out.coff == 0 and out.buf.ld == out.C
        assert out.C <= 64 and H + W <= 2048
        op = self._base_u8(L.OP_STEM_U8, u8, out, out.H, out.W)
        op.Cout = out.C
        self._set_window(op, kh, 2, pad)
        op.act = act
        op.res_H, op.res_W = u8[2:4]
        if split:
            # BlazeFace's 5x5 stem on the bf16 matrix cores (FP_OPF_SPLIT3, stem5_u8_x6_kernel): the band form's shape only
            assert (kh, H, W, out.H, out.W, cout) == (5, 256, 256, 128, 128, 24) and pad == (1, 1) and scale is None
            assert bias is not None and act == L.ACT_RELU and self.N >= 16
            op.flags |= L.OPF_SPLIT3
            op.w_off = self.add_weight(self.pack_stem5_x6(w))
        else:
            op.w_off = self.add_weight(pack_conv_weight(w, 4, out.C))
        self._epilogue(op, out.C, scale, bias, slope)
        self.ops.append(op)
        self.alg_bytes.append(4 * self.N * (H * W * 3 + out.H * out.W * cout))
        return out

    def ystem(self, x, w1, scale1, bias1, w2, scale2, bias2, a_out, pool_out, u8=None):
        """Head of YOLOv5-face's StemBlock (common.py:58-73) as ONE op: stem_1 (3x3 s2 p1, SiLU) stays in LDS,
        stem_2a (1x1, SiLU) -> a_out, maxpool2x2(stem_1) -> pool_out (a channel slice of stem_3's concat buffer).
        scale1 / scale2 = None when the BatchNorm is folded into the conv (Model.fuse()).
        u8 = (H, W, frame_h, frame_w, ext_index): the op reads the u8 frames itself (FP_OP_YSTEM_U8, _base_u8) and x is None."""
        c1, c2 = w1.shape[0], w2.shape[0]
        assert w1.shape[2:] == (3, 3) and w2.shape[1] == c1 and w2.shape[2:] == (1, 1)
        assert c1 <= 32 and a_out.C <= 32 and pool_out.C >= c1 and pool_out.cmul == 1 and a_out.cmul == 1
        if u8 is None:
            assert x.C == 4 and x.buf.ld == 4 and x.coff == 0
            H, W = x.H, x.W
            op = self._base(L.OP_YSTEM, x, a_out, H // 2, W // 2)
            if w1.shape[1] == 3:   # 3-channel image in 16-byte pixels: the pad channel's weights are zero
                op.flags |= L.OPF_IN_C3
        else:
            assert x is None
            H, W = u8[:2]
            op = self._base_u8(L.OP_YSTEM_U8, u8, a_out, H // 2, W // 2)
        H1, W1 = H // 2, W // 2
        assert H % 4 == 0 and W % 4 == 0 and (a_out.H, a_out.W) == (H1, W1) and (pool_out.H, pool_out.W) == (H1 // 2, W1 // 2)
        op.Cout = a_out.C
        self._set_window(op, 3, 2, 1)
        op.act = L.ACT_SILU
        self._set_res(op, pool_out, cpad(c1))
        if u8 is not None:
            op.res_H, op.res_W = u8[2:4]      # the frames' size
        op.w_off = self.add_weight(pack_conv_weight(w1, 4, cpad(c1)))
        self._epilogue(op, 32, scale1, bias1)
        nb2 = (a_out.C + 15) // 16
        wq = np.zeros((32, nb2 * 16), np.float32)                       # [k][n], zero padded
        wq[:c1, :c2] = np.asarray(w2, np.float32).reshape(c2, c1).T
        blob = [np.ascontiguousarray(wq.reshape(2, 4, 4, nb2 * 16).transpose(0, 1, 3, 2)).reshape(-1),  # [j][g][n][e]
                affine_rows((scale2 if scale2 is not None else np.ones(c2, np.float32), bias2), nb2 * 16)]
        op.slope_off = self.add_weight(np.concatenate(blob))
        self.ops.append(op)
        self.alg_bytes.append(4 * self.N * (H * W * 3 + H1 * W1 * c1 + H1 * W1 * c1 + H1 * W1 * c2))
        return a_out

    def ystem2(self, a, pool, w2b, aff2b, w3, aff3, out):
        """The tail of YOLOv5-face's StemBlock (y5/models/common.py:58-73) as ONE op (FP_OP_YSTEM2, csrc/ystem2.hip):
        out = stem_3(cat(stem_2b(a), pool)), both convs + (BN) + SiLU.  *_aff = (scale or None, bias).  Layout: facepath.h "YSTEM2".
        None (nothing emitted) if X6 is off or the launcher refuses the op."""
        assert w2b.shape == (32, 16, 3, 3) and w3.shape[:2] == (32, 64) and pool.cmul == 1
        op = self._base(L.OP_YSTEM2, a, out, out.H, out.W)
        op.Cout = out.C
        self._set_window(op, 3, 2, 1)
        op.act = op.act2 = L.ACT_SILU
        op.flags |= L.OPF_SPLIT3
        self._set_res(op, pool)
        self._offsets(op, True, False, False, False)
        if not self.X6 or self.probe(op) is None:
            return None

        def aff(sb):
            return affine_rows((np.ones(32, np.float32) if sb[0] is None else sb[0], sb[1]), 32)
        k2 = np.zeros((32, 160), np.float32)                                    # k = (ky*3 + kx)*16 + c, padded to five slabs
        k2[:, :144] = np.asarray(w2b, np.float32).transpose(0, 2, 3, 1).reshape(32, 144)
        op.w_off = self.add_weight(np.concatenate([pack_kslab_x6(k2), aff(aff2b), pack_kslab_x6(_mat(w3)), aff(aff3)]))
        self.ops.append(op)
        pix, opix = a.H * a.W, out.H * out.W
        self.alg_bytes.append(4 * self.N * (pix * 16 + opix * 32 + opix * 64 + opix * 32))   # the two convs
        return out

    def maxpool(self, x, out, k, stride, pad):
        assert out.C == x.C
        op = self._base(L.OP_MAXPOOL, x, out, out.H, out.W)
        op.Cout = x.C
        self._set_window(op, k, stride, pad)
        self.ops.append(op)
        self.alg_bytes.append(0)
        return out

    def upsample2x(self, x, out):
        assert out.C == x.C and out.H == 2 * x.H and out.W == 2 * x.W
        op = self._base(L.OP_UPSAMPLE2X, x, out, out.H, out.W)
        op.Cout = x.C
        self.ops.append(op)
        self.alg_bytes.append(0)
        return out

    def copy(self, x, out):
        assert out.C == x.C and out.H == x.H and out.W == x.W
        op = self._base(L.OP_COPY, x, out, out.H, out.W)
        op.Cout = x.C
        self.ops.append(op)
        self.alg_bytes.append(0)
        return out

    def l2norm(self, x, out):
        op = self._base(L.OP_L2NORM, x, out, out.H, out.W)
        op.Cout = x.C
        self.ops.append(op)
        self.alg_bytes.append(0)
        return out

    def embed_head(self, x, w, out, scale=None, bias=None, normalize=False):
        """Embedding head as ONE op (FP_OP_EMBED_HEAD, csrc/embedhead.hip): mean over x's H x W pixels -> Linear (w: [D, C], no
        bias) -> x*scale + bias (BatchNorm1d) -> with normalize, F.normalize.  out: a View of a 1 x 1 buffer, D channels."""
        d, c = w.shape
        assert c <= x.C and out.C >= d and (out.H, out.W) == (1, 1) and out.cmul == 1 and x.up is None
        op = self._base(L.OP_EMBED_HEAD, x, out, 1, 1)
        op.Cout = d
        wp = np.zeros((d, x.C), np.float32)
        wp[:, :c] = np.asarray(w, np.float32)
        op.w_off = self.add_weight(wp)
        self._epilogue(op, d, scale, bias)
        if normalize:
            op.flags |= L.OPF_OUT_L2
        self.ops.append(op)
        self.alg_bytes.append(4 * self.N * (x.H * x.W * c + d))
        return out

    def pool_lrn(self, x, out, k, stride, pad=0, group=0, size=5, alpha=1e-4, beta=0.75, lrn_k=1.0):
        """k x k max pool (-inf padding; out.H / out.W as the caller computed them, Caffe's ceil mode included) followed by
        Caffe's cross-channel LRN within groups of `group` channels (0: no LRN) as ONE op (FP_OP_POOL_LRN, csrc/lrn.hip)."""
        assert out.C == x.C and out.cmul == 1 and x.up is None
        op = self._base(L.OP_POOL_LRN, x, out, out.H, out.W)
        op.Cout = x.C
        self._set_window(op, k, stride, pad)
        if group:
            op.Cmid, op.res_C = group, size
            op.w_off = self.add_weight(np.array([alpha, beta, lrn_k, 0.0], np.float32))
        self.ops.append(op)
        self.alg_bytes.append(0)
        return out

    def cls_head(self, x, w, bias, out, logits=None):
        """Linear (w: [D, C], + bias) -> softmax on the row at pixel 0 of every image of x as ONE op (FP_OP_CLS_HEAD,
        csrc/clshead.hip).  out: a View of a 1 x 1 buffer (D channels) for the probabilities; logits: one for the logits."""
        d, c = w.shape
        assert c <= x.C and out.C >= d and (out.H, out.W) == (1, 1) and out.cmul == 1 and x.up is None
        op = self._base(L.OP_CLS_HEAD, x, out, 1, 1)
        op.H = op.W = 1
        op.Cout = d
        wp = np.zeros((d, x.C), np.float32)
        wp[:, :c] = np.asarray(w, np.float32)
        op.w_off = self.add_weight(wp)
        if bias is not None:
            op.bias_off = self.add_weight(pad_vec(bias, d))
        op.res_off = -1
        if logits is not None:
            assert logits.cmul == 1 and logits.C >= d
            op.res_off, op.res_ns, op.res_ld = logits.buf.off + logits.coff, logits.buf.ns, logits.buf.ld
        self.ops.append(op)
        self.alg_bytes.append(4 * self.N * (c + d))
        return out

    def finish(self):
        if not self._placed:   # the row-padded region goes behind the recycled arena: relocate its views once
            self._placed = True
            if self.rowpad_top:
                shift = round_up(self.peak, 64)
                for op in self.ops:
                    if op.flags & L.OPF_IN_ROWPAD:
                        if op.kind == L.OP_BLAZEPAIR:
                            op.res_off += shift      # its shortcut view IS its input view
                        op.in_off += shift
                    if op.flags & L.OPF_OUT_ROWPAD:
                        op.out_off += shift
                for buf in self.rowpad_bufs:
                    buf.off += shift
                self.peak = shift + self.rowpad_end
        weights = np.concatenate(self.wchunks) if self.wchunks else np.zeros(4, np.float32)
        return self.ops, weights, self.peak


def switch_key(*classes):
    """Every class-wide switch of the given classes (their own UPPER_CASE attributes holding a bool / int / float / str /
    tuple / None: FUSE, ROWPAD, PAIR, CHAIN, FOLD_UPSAMPLE, PlanBuilder.X6, ...) as one hashable tuple.  It is part of
    every plan-cache key: a plan records the kernels the switches selected when it was emitted, so flipping one after a
    plan exists must build another plan, not reuse that one."""
    key = []
    for cls in classes:
        for name, v in sorted(vars(cls).items()):
            if name.isupper() and isinstance(v, (bool, int, float, str, tuple, type(None))):
                key.append((cls.__name__, name, v))
    return tuple(key)


class PlanCache:
    """Per-network cache of compiled plans, keyed by batch shape + the emit switches (switch_key).

    * LRU-bounded (``max_plans``): a plan owns an activation arena of several GB at batch >= 1024, so a caller whose
      batch size varies (FacePipeline's 64-row buckets) must not pin one arena per size it has ever seen.
    * The packed weight blob does not depend on the batch size: every plan of one network shares ONE device copy
      (compared by content on the host, so a plan emitted with different fusion switches gets its own).
    ``clear()`` is what load_state_dict / .to() / fuse() call."""

    def __init__(self, max_plans=4):
        self.max_plans = int(max_plans)
        self._plans = {}          # insertion-ordered: oldest first
        self._weights = []        # [(host ndarray, device tensor)]

    def clear(self):
        self._plans = {}
        self._weights = []

    def __len__(self):
        return len(self._plans)

    def __contains__(self, key):
        return key in self._plans

    def get(self, key, build):
        plan = self._plans.pop(key, None)
        if plan is None:
            while len(self._plans) >= self.max_plans:
                self._plans.pop(next(iter(self._plans)))
            plan = build(self)
        self._plans[key] = plan   # most recently used last
        return plan

    def device_weights(self, host, device):
        import torch
        for h, d in self._weights:
            if d.device == device and h.shape == host.shape and np.array_equal(h.view(np.uint32), host.view(np.uint32)):
                return d
        d = torch.from_numpy(host).to(device)
        self._weights.append((host, d))
        return d


class CompiledPlan:
    """Ops + device weights + arena, ready to run on a stream.

    Every tensor a plan exposes (``input``, ``out``, ``r``, ``c``, ``z`` ...) is a VIEW into its arena: the next
    ``run()`` of the same plan overwrites it.  The public forward APIs of the networks return clones; the
    ``*_resident`` variants hand out the views (zero-copy, for callers that consume them before the next run)."""

    def __init__(self, builder, device, cache=None):
        import torch
        ops, weights, arena_floats = builder.finish()
        self.n_ops = len(ops)
        self.N = builder.N            # batch capacity: the arena holds N images; run(n=...) may process fewer
        self.n_run = builder.N
        self.alg_bytes = list(builder.alg_bytes)
        assert len(self.alg_bytes) == self.n_ops
        self.ops = (L.FpOp * max(self.n_ops, 1))(*ops)
        self.device = torch.device(device)
        self.weights = cache.device_weights(weights, self.device) if cache is not None else \
            torch.from_numpy(weights).to(self.device)
        self.arena_floats = int(arena_floats)
        # row-padded buffers rely on pads that nobody ever writes: start from zeros
        alloc = torch.zeros if builder.has_rowpad else torch.empty
        self.arena = alloc(self.arena_floats, dtype=torch.float32, device=self.device)
        self.lib = L.load()
        L.check(self.lib.fp_plan_validate(self.ops, self.n_ops, self.weights.numel(), self.arena_floats),
                "fp_plan_validate")
        # Row windows (PlanBuilder.window): a windowed op writes only its window, so the rows outside it must already hold
        # what an unrestricted run writes there.  They do not depend on the frames, but they do depend on the kernels that
        # wrote them (the stem's kernel follows the batch) and on the pad colour / LUT behind the tap tables.  So a run is
        # windowed only if an unrestricted run of at least as many images, with the same kernels and external tables, came
        # before it; any other run is unrestricted and becomes the new record.  `prime_runs` counts those.
        self.windows = list(builder.windows)
        self.prime_runs = 0
        self._primed = None         # (n, key) of the last unrestricted run
        self._win_key = {}          # n -> (windowed kernels, windows valid at n)
        self._win_on = True
        self._set_windows(False)

    def _set_windows(self, on):
        if on != self._win_on:
            for i, lo, end in self.windows:
                self.ops[i].row_lo, self.ops[i].row_end = (lo, end) if on else (0, 0)
            self._win_on = on

    def _window_choice(self, n):
        """(names of the kernels the windowed ops launch at batch n, whether the library accepts the windows at n)"""
        if n not in self._win_key:
            self._set_windows(True)
            ok = self.lib.fp_plan_validate(self.ops, self.n_ops, self.weights.numel(), self.arena_floats) == 0
            self._win_key[n] = (tuple(self.kernel_name(i) for i, _, _ in self.windows), ok)
        return self._win_key[n]

    def invalidate_windows(self):
        """The next run is unrestricted (the caller changed something the rows outside the windows depend on)."""
        self._primed = None

    def _prepare_windows(self):
        n = self.n_run
        names, ok = self._window_choice(n)
        key = (names, tuple(t.data_ptr() for t in self._ext_keep[1:]))    # kernels; tap tables + LUT (external buffer 0 = the frames)
        on = ok and self._primed is not None and self._primed[1] == key and n <= self._primed[0]
        self._set_windows(on)
        if not on:
            self._primed = (n, key)
            self.prime_runs += 1

    def buf_tensor(self, buf, N):
        """A torch view [N, H, W, C] of an arena buffer (no copy)."""
        if buf.rowpad:
            return self.arena.as_strided((N, buf.H, buf.W, buf.C), (buf.ns, (buf.W + 1) * buf.C, buf.C, 1), buf.off)
        return self.arena[buf.off: buf.off + N * buf.ns].view(N, buf.H, buf.W, buf.C)

    _timing = None   # (timer, mask) set by bench.py around a timed step; None = plain fp_plan_run
    _ext = None      # ctypes array of fp_ext (external buffers of *_U8 ops), set by set_ext()
    _ext_keep = ()   # the tensors behind it, kept alive

    def set_ext(self, tensors):
        """External device buffers of the plan (e.g. [frames u8, tap tables, LUT] for a *_U8 stem op), in the order the
        ops index them.  The tensors are held until the next set_ext."""
        self._ext_keep = tuple(tensors)
        self._ext = (L.FpExt * max(len(tensors), 1))(*[L.FpExt(t.data_ptr(), t.numel() * t.element_size())
                                                      for t in tensors])

    def set_batch(self, n):
        """Process only the first n <= N images on the following runs.  Every per-image stride of an op is independent
        of the batch size, so this only rewrites the ops' N field; kernel selection (persistent / streaming / per-tile)
        follows the actual n at launch time."""
        n = int(n)
        if not 0 < n <= self.N:
            raise ValueError(f"batch {n} outside the plan's capacity 1..{self.N}")
        if n != self.n_run:
            for i in range(self.n_ops):
                self.ops[i].N = n
            self.n_run = n

    def run(self, n=None):
        if n is not None:
            self.set_batch(n)
        if self.windows:
            self._prepare_windows()
        if self._timing is not None:
            return self.run_timed(*self._timing)
        rc = self.lib.fp_plan_run_ext(self.ops, self.n_ops, L.ptr(self.weights), self.weights.numel(),
                                      L.ptr(self.arena), self.arena_floats, self._ext, len(self._ext_keep),
                                      L.current_stream(self.device))
        L.check(rc, "fp_plan_run")

    # ---- measurement support (bench.py) ----
    def new_timer(self):
        t = C.c_void_p()
        L.check(self.lib.fp_timer_create(max(self.n_ops, 1), C.byref(t)), "fp_timer_create")
        return t

    def run_timed(self, timer, mask):
        """Like run(), with HIP events recorded on the stream around the ops selected by mask (bytes, n_ops)."""
        m = (C.c_ubyte * self.n_ops)(*mask)
        rc = self.lib.fp_plan_run_timed_ext(self.ops, self.n_ops, L.ptr(self.weights), self.weights.numel(),
                                            L.ptr(self.arena), self.arena_floats, self._ext, len(self._ext_keep),
                                            L.current_stream(self.device), timer, m)
        L.check(rc, "fp_plan_run_timed")

    def accumulate(self, timer, ms):
        """ms: ctypes float array of n_ops; adds the last timed run's per-op milliseconds."""
        L.check(self.lib.fp_timer_accumulate(timer, ms, self.n_ops), "fp_timer_accumulate")

    def destroy_timer(self, timer):
        self.lib.fp_timer_destroy(timer)

    def kernel_name(self, i):
        """The HIP kernel family op i launches (matches the rocprofv3 kernel-trace names)."""
        return self.lib.fp_op_kernel_name(C.byref(self.ops[i])).decode()

    def compulsory_bytes(self, i, n=None):
        """Bytes op i MUST move for a batch of n images (default: the batch the plan last ran on): every tensor it reads
        once + every tensor it writes once, physical channel counts, weights not counted (they are re-read from L2).
        A fused op is charged for its inputs and outputs only -- the tensors between the reference ops it replaces never
        exist -- so this is the denominator of a physical roofline fraction (bench.py `roofline.frac`); the SURVEY 8(d)
        op-granular figure is algorithmic_bytes()."""
        op = self.ops[i]
        n = self.n_run if n is None else n
        k = op.kind
        if k in (L.OP_STEM_U8, L.OP_YSTEM_U8):
            b_in = op.res_H * op.res_W * 3                       # u8 frame
        else:
            b_in = op.H * op.W * op.Cin * 4
            if op.flags & L.OPF_IN_UP2:                          # the leading res_C channels come from the half-size map
                b_in = op.H * op.W * (op.Cin - op.res_C) * 4 + op.res_H * op.res_W * op.res_C * 4
        cout = op.Cout if k in (L.OP_CONV, L.OP_BLAZEBLOCK, L.OP_DWPW, L.OP_DWBLOCK, L.OP_BLAZEPAIR, L.OP_BLAZECHAIN, L.OP_YSTEM, L.OP_YSTEM_U8,
                                L.OP_STEM_U8, L.OP_SHUFDOWN, L.OP_SHUFUNIT, L.OP_YSTEM2, L.OP_EMBED_HEAD) else op.Cin
        oh, ow = (op.H, op.W) if k in (L.OP_COPY, L.OP_L2NORM) else (op.OH, op.OW)
        b_out = oh * ow * cout * 4 * (2 if op.res_mode == L.RES_SHUFFLE2 else 1)
        b_res = 0
        if k in (L.OP_YSTEM, L.OP_YSTEM_U8):
            b_res = (op.OH // 2) * (op.OW // 2) * op.res_C * 4   # the pooled stem_1 map it also writes
        elif k == L.OP_YSTEM2:
            b_res = op.OH * op.OW * op.res_C * 4                 # the pooled map it reads
        elif (k in (L.OP_CONV, L.OP_DWPW) and op.res_off != op.in_off and
              op.res_mode in (L.RES_ADD_BEFORE_ACT, L.RES_ADD_AFTER_ACT, L.RES_SHUFFLE2)):
            b_res = oh * ow * op.res_C * 4                       # a residual that is not the op's own input (the block
                                                                 # ops' shortcut is their input: read once)
        if op.row_end > 0:      # a row window (the last run's): its rows are written, and the input rows they reach are read
            if k == L.OP_BLAZEPAIR:
                lo, end = (op.row_lo - 2, op.row_end + 2) if op.stride == 1 else (2 * op.row_lo - 1, 2 * op.row_end + 2)
                b_in = b_in * (min(op.H, end) - max(0, lo)) // op.H
            b_out = b_out * (op.row_end - op.row_lo) // oh
        return n * (b_in + b_out + b_res)

    def flops(self, i, n=None):
        """Arithmetic of op i as the REFERENCE counts it (2 x multiply-accumulates of its convolutions, logical shapes) for a
        batch of n images -- whatever instructions the kernel uses for them."""
        op = self.ops[i]
        n = self.n_run if n is None else n
        k, opix = op.kind, op.OH * op.OW
        if k in (L.OP_CONV, L.OP_STEM_U8):
            f = opix * op.KH * op.KW * op.Cin * op.Cout + (opix * 9 * op.Cout if op.flags & L.OPF_OUT_DW else 0)
        elif k == L.OP_DWCONV:
            f = opix * op.KH * op.KW * op.Cin
        elif k in (L.OP_BLAZEBLOCK, L.OP_DWPW):
            f = opix * (9 * op.Cin + op.Cin * op.Cout)
        elif k == L.OP_BLAZEPAIR and op.stride == 2:
            f = op.H * op.W * (9 * op.Cin + op.Cin * op.Cin) + opix * (9 * op.Cin + op.Cin * op.Cout)
        elif k == L.OP_BLAZEPAIR:
            f = 2 * opix * (9 * op.Cin + op.Cin * op.Cout)
        elif k == L.OP_BLAZECHAIN:
            f = op.Cmid * opix * (9 * op.Cin + op.Cin * op.Cout)
        elif k == L.OP_DWBLOCK:
            f = op.H * op.W * op.Cin * op.Cmid + opix * (9 * op.Cmid + op.Cmid * op.Cout)
        elif k == L.OP_SHUFUNIT:
            f = opix * (2 * op.Cmid * op.Cmid + 9 * op.Cmid)
        elif k == L.OP_YSTEM2:
            f = opix * (9 * op.Cin * op.Cout + 2 * op.Cout * op.Cout)
        elif k in (L.OP_EMBED_HEAD, L.OP_CLS_HEAD):  # the Linear (the mean, the affine, the softmax are epilogue-class)
            f = op.Cin * op.Cout
        elif k == L.OP_SHUFDOWN:   # branch1: dw + 1x1; branch2: 1x1 at full resolution, dw, 1x1
            f = opix * (9 * op.Cin + op.Cin * op.Cmid) + op.H * op.W * op.Cin * op.Cmid + opix * (9 * op.Cmid + op.Cmid * op.Cmid)
        else:
            f = 0
        return 2.0 * n * f

    def bound(self, i):
        """"mfma" for the ops whose kernels run on the matrix cores near their issue limit (the split-MFMA blocks), else "hbm"."""
        return "mfma" if self.ops[i].flags & L.OPF_SPLIT3 else "hbm"

    def algorithmic_bytes(self, i):
        """Op-granular fp32 activation bytes of op i: a conv / linear reads its input once and
        writes its output once (logical channel counts); epilogue-class ops (bias, BN, activation, residual,
        pad, concat, pool, shuffle, upsample, l2norm) are free; a fused op counts the convs it contains."""
        return self.alg_bytes[i]


def validate_on_host(builder):
    """Host-only validation (no GPU): runs fp_plan_validate on the built ops."""
    ops, weights, arena_floats = builder.finish()
    arr = (L.FpOp * max(len(ops), 1))(*ops)
    lib = L.load()
    return lib.fp_plan_validate(arr, len(ops), int(weights.size), int(arena_floats))
