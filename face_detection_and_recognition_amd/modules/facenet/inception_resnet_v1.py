"""FaceNet (Inception-ResNet-v1, Szegedy et al. 2016) on MI355X: the network the reference's similarity filter and its
FACENET_TRT / FACENET_OV dataset options embed faces with, with facenet-pytorch's ``state_dict`` keys and the forward pass
compiled to a HIP plan.

* 160 x 160 RGB input in 4-float pixels (like the other stems); 128-d (Keras / TensorRT ``Bottleneck_BatchNorm``) or 512-d
  (Sandberg's 20180408-102900) embeddings, L2-normalised or not (``normalize``).
* Every BasicConv (conv without bias -> BatchNorm eps 1e-3 -> ReLU) is one FP_OP_CONV with the BatchNorm as its affine
  epilogue.  With PlanBuilder.X6 every conv runs on the split-MFMA kernels (csrc/pwx6.hip: fp32-equivalent arithmetic on
  the bf16 matrix cores), the unpadded 3x3 and the 1x7 / 7x1 / 1x3 / 3x1 windows included.
* No copies: the 1x1 branch convs that read a block's input are ONE op; every branch writes its channel slice of the
  buffer the up-projection reads (max-pool branches included); a block's scale rides in the up-projection's epilogue
  (scale = s, bias = s * b, + x, ReLU or none).  The head (mean, last_linear, last_bn, F.normalize) is one
  FP_OP_EMBED_HEAD (csrc/embedhead.hip).
"""
import numpy as np
import torch
import torch.nn as nn

from ... import _lib as L
from ...plan import CompiledPlan, PlanBuilder, PlanCache, switch_key
from ..params import BNParams, ConvParams, LinearParams, PlanCacheMixin, _NoCompute, bn_sb, npy


class _RectConv(_NoCompute):
    """Keys: ``weight`` [O, I, kh, kw] like nn.Conv2d(bias=False) with a rectangular kernel."""

    def __init__(self, cin, cout, kh, kw):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin, kh, kw), requires_grad=False)
        nn.init.normal_(self.weight, 0.0, float(np.sqrt(2.0 / (cin * kh * kw))))


class BasicConv2d(_NoCompute):
    """conv (no bias) -> BatchNorm2d(eps 1e-3) -> ReLU; stride-2 convs unpadded, the others 'same'."""

    def __init__(self, cin, cout, kernel, stride=1, padding=0):
        super().__init__()
        self.kh, self.kw = (kernel, kernel) if isinstance(kernel, int) else kernel
        self.pad = (padding, padding) if isinstance(padding, int) else tuple(padding)
        self.stride, self.cin, self.cout = stride, cin, cout
        self.conv = _RectConv(cin, cout, self.kh, self.kw)
        self.bn = BNParams(cout, eps=1e-3)

    def out_hw(self, H, W):
        return ((H + 2 * self.pad[0] - self.kh) // self.stride + 1, (W + 2 * self.pad[1] - self.kw) // self.stride + 1)

    def emit(self, pb, x, out):
        """x: input View; out: the View (a channel slice, possibly) the ReLU output goes to."""
        s, b = bn_sb(self.bn)
        pb.conv(x, npy(self.conv.weight), out, stride=self.stride, pad=self.pad, scale=s, bias=b, act=L.ACT_RELU)
        return out

    def emit_new(self, pb, x):
        H, W = self.out_hw(x.H, x.W)
        y = pb.new_buf(H, W, self.cout)
        self.emit(pb, x, y.view())
        return y


def _merged_1x1(pb, x, convs, out):
    """Several 1x1 BasicConvs on the same input as ONE op (their outputs side by side in `out`)."""
    w = np.concatenate([npy(c.conv.weight) for c in convs])
    aff = [bn_sb(c.bn) for c in convs]
    pb.conv(x, w, out, scale=np.concatenate([a[0] for a in aff]), bias=np.concatenate([a[1] for a in aff]),
            act=L.ACT_RELU, n_convs=len(convs))


class _Block(_NoCompute):
    """The residual blocks: branch0 = 1x1 c; branch1 = 1x1 c -> the convs of `chain`; [branch2 = 1x1 c -> 3x3 -> 3x3
    (Block35)]; concat -> conv2d 1x1 (+ bias) -> x + scale * up -> ReLU (unless no_relu)."""

    def _up(self, pb, x, cat, out):
        s = np.float32(self.scale)
        w = npy(self.conv2d.weight)
        pb.conv(cat, w, out.view(), scale=np.full(w.shape[0], s, np.float32), bias=s * npy(self.conv2d.bias),
                act=L.ACT_NONE if self.no_relu else L.ACT_RELU, res=x, res_mode=L.RES_ADD_BEFORE_ACT)

    def emit(self, pb, xbuf):
        """Buffer layout Z (one pixel): [first convs of the chains | branch0 | chain outputs]; the merged 1x1 op writes the first
        two parts, each chain its last part, and the up-projection reads [branch0 | chain outputs] -- the concat -- in place."""
        x = xbuf.view()
        c = self.c
        heads = [ch[0] for ch in self.chains]
        nch = len(self.chains)
        Z = pb.new_buf(x.H, x.W, (2 * nch + 1) * c)
        _merged_1x1(pb, x, heads + [self.branch0], Z.view(0, (nch + 1) * c))
        for i, ch in enumerate(self.chains):
            v = Z.view(i * c, c)
            tmp = []
            for j, conv in enumerate(ch[1:]):
                last = j == len(ch) - 2
                dst = Z.view((nch + 1 + i) * c, c) if last else pb.new_buf(x.H, x.W, c).view()
                conv.emit(pb, v, dst)
                if not last:
                    tmp.append(dst.buf)
                v = dst
            for t in tmp:
                pb.free(t)
        y = pb.new_buf(x.H, x.W, x.C)
        self._up(pb, x, Z.view(nch * c, (nch + 1) * c), y)
        pb.free(Z)
        return y


class Block35(_Block):
    def __init__(self, scale=1.0):
        super().__init__()
        self.scale, self.no_relu, self.c = scale, False, 32
        self.branch0 = BasicConv2d(256, 32, 1)
        self.branch1 = nn.Sequential(BasicConv2d(256, 32, 1), BasicConv2d(32, 32, 3, padding=1))
        self.branch2 = nn.Sequential(BasicConv2d(256, 32, 1), BasicConv2d(32, 32, 3, padding=1), BasicConv2d(32, 32, 3, padding=1))
        self.conv2d = ConvParams(96, 256, 1, bias=True)

    @property
    def chains(self):
        return [list(self.branch1), list(self.branch2)]


class Block17(_Block):
    def __init__(self, scale=1.0):
        super().__init__()
        self.scale, self.no_relu, self.c = scale, False, 128
        self.branch0 = BasicConv2d(896, 128, 1)
        self.branch1 = nn.Sequential(BasicConv2d(896, 128, 1), BasicConv2d(128, 128, (1, 7), padding=(0, 3)),
                                     BasicConv2d(128, 128, (7, 1), padding=(3, 0)))
        self.conv2d = ConvParams(256, 896, 1, bias=True)

    @property
    def chains(self):
        return [list(self.branch1)]


class Block8(_Block):
    def __init__(self, scale=1.0, noReLU=False):
        super().__init__()
        self.scale, self.no_relu, self.c = scale, noReLU, 192
        self.branch0 = BasicConv2d(1792, 192, 1)
        self.branch1 = nn.Sequential(BasicConv2d(1792, 192, 1), BasicConv2d(192, 192, (1, 3), padding=(0, 1)),
                                     BasicConv2d(192, 192, (3, 1), padding=(1, 0)))
        self.conv2d = ConvParams(384, 1792, 1, bias=True)

    @property
    def chains(self):
        return [list(self.branch1)]


class Mixed_6a(_NoCompute):
    def __init__(self):
        super().__init__()
        self.branch0 = BasicConv2d(256, 384, 3, stride=2)
        self.branch1 = nn.Sequential(BasicConv2d(256, 192, 1), BasicConv2d(192, 192, 3, padding=1),
                                     BasicConv2d(192, 256, 3, stride=2))

    def emit(self, pb, xbuf):
        x = xbuf.view()
        OH, OW = (x.H - 3) // 2 + 1, (x.W - 3) // 2 + 1
        out = pb.new_buf(OH, OW, 896)
        self.branch0.emit(pb, x, out.view(0, 384))
        a = self.branch1[0].emit_new(pb, x)
        b = self.branch1[1].emit_new(pb, a.view())
        pb.free(a)
        self.branch1[2].emit(pb, b.view(), out.view(384, 256))
        pb.free(b)
        pb.maxpool(x, out.view(640, 256), 3, 2, 0)
        return out


class Mixed_7a(_NoCompute):
    def __init__(self):
        super().__init__()
        self.branch0 = nn.Sequential(BasicConv2d(896, 256, 1), BasicConv2d(256, 384, 3, stride=2))
        self.branch1 = nn.Sequential(BasicConv2d(896, 256, 1), BasicConv2d(256, 256, 3, stride=2))
        self.branch2 = nn.Sequential(BasicConv2d(896, 256, 1), BasicConv2d(256, 256, 3, padding=1),
                                     BasicConv2d(256, 256, 3, stride=2))

    def emit(self, pb, xbuf):
        x = xbuf.view()
        OH, OW = (x.H - 3) // 2 + 1, (x.W - 3) // 2 + 1
        out = pb.new_buf(OH, OW, 1792)
        m = pb.new_buf(x.H, x.W, 768)
        _merged_1x1(pb, x, [self.branch0[0], self.branch1[0], self.branch2[0]], m.view())
        self.branch0[1].emit(pb, m.view(0, 256), out.view(0, 384))
        self.branch1[1].emit(pb, m.view(256, 256), out.view(384, 256))
        t = self.branch2[1].emit_new(pb, m.view(512, 256))
        pb.free(m)
        self.branch2[2].emit(pb, t.view(), out.view(640, 256))
        pb.free(t)
        pb.maxpool(x, out.view(896, 896), 3, 2, 0)
        return out


class InceptionResnetV1(PlanCacheMixin, nn.Module):
    """Inception-ResNet-v1 (facenet-pytorch's layout and ``state_dict`` keys; ``logits.*`` is not part of it).
    ``forward(x)``: (b, 3, 160, 160) float, RGB, already standardised -> (b, embedding_size), unit rows if ``normalize``."""

    input_size = (160, 160)

    def __init__(self, embedding_size=512, normalize=True):
        super().__init__()
        self.embedding_size = int(embedding_size)
        self.normalize = bool(normalize)
        self.conv2d_1a = BasicConv2d(3, 32, 3, stride=2)
        self.conv2d_2a = BasicConv2d(32, 32, 3)
        self.conv2d_2b = BasicConv2d(32, 64, 3, padding=1)
        self.conv2d_3b = BasicConv2d(64, 80, 1)
        self.conv2d_4a = BasicConv2d(80, 192, 3)
        self.conv2d_4b = BasicConv2d(192, 256, 3, stride=2)
        self.repeat_1 = nn.Sequential(*[Block35(scale=0.17) for _ in range(5)])
        self.mixed_6a = Mixed_6a()
        self.repeat_2 = nn.Sequential(*[Block17(scale=0.10) for _ in range(10)])
        self.mixed_7a = Mixed_7a()
        self.repeat_3 = nn.Sequential(*[Block8(scale=0.20) for _ in range(5)])
        self.block8 = Block8(noReLU=True)
        self.last_linear = LinearParams(1792, self.embedding_size, bias=False)
        self.last_bn = BNParams(self.embedding_size, eps=1e-3)
        self._plans = PlanCache()

    def _device(self):
        return self.last_linear.weight.device

    def load_state_dict(self, state_dict, strict=True):
        """facenet-pytorch / converted-Keras state dicts: ``logits.*`` and ``num_batches_tracked`` are ignored; any other
        missing, unexpected or mis-shaped key raises."""
        own = super().state_dict()
        sd = {k: v for k, v in state_dict.items() if not k.startswith("logits.") and not k.endswith("num_batches_tracked")}
        for k, v in own.items():
            if k.endswith("num_batches_tracked"):
                sd[k] = v
        return super().load_state_dict(sd, strict=True)      # PlanCacheMixin: + _invalidate()

    def _emit(self, N):
        """Emit the op list for batch N (host only, no GPU needed)."""
        pb = PlanBuilder(N)
        pb.x6_all = True
        H, W = self.input_size
        inp = pb.new_buf(H, W, 3)
        x = inp
        for m in (self.conv2d_1a, self.conv2d_2a, self.conv2d_2b):
            y = m.emit_new(pb, x.view())
            if x is not inp:
                pb.free(x)
            x = y
        y = pb.new_buf((x.H - 3) // 2 + 1, (x.W - 3) // 2 + 1, x.C)          # maxpool_3a
        pb.maxpool(x.view(), y.view(), 3, 2, 0)
        pb.free(x)
        x = y
        for m in (self.conv2d_3b, self.conv2d_4a, self.conv2d_4b):
            y = m.emit_new(pb, x.view())
            pb.free(x)
            x = y
        for m in list(self.repeat_1) + [self.mixed_6a] + list(self.repeat_2) + [self.mixed_7a] + list(self.repeat_3) + [self.block8]:
            y = m.emit(pb, x)
            pb.free(x)
            x = y
        D = self.embedding_size
        o = pb.new_buf(1, 1, D)
        s, b = bn_sb(self.last_bn)
        pb.embed_head(x.view(), npy(self.last_linear.weight), o.view(0, D), scale=s, bias=b, normalize=self.normalize)
        return pb, inp, o

    def _build(self, N, cache=None):
        D = self.embedding_size
        pb, inp, o = self._emit(N)
        plan = CompiledPlan(pb, self._device(), cache)
        plan.input = plan.buf_tensor(inp, N)
        plan.out = plan.buf_tensor(o, N).view(N, -1)[:, :D]
        return plan

    def plan_for(self, N, n_run=None):
        """The plan with batch capacity N (n_run: accepted for the embedder interface; the op list does not depend on it)."""
        if self._device().type != "cuda":
            raise L.FacepathError("InceptionResnetV1 runs only on a HIP device (model.to('cuda')); there is no CPU path")
        key = (N, self.normalize, switch_key(PlanBuilder))
        return self._plans.get(key, lambda cache: self._build(N, cache))

    def forward(self, x):
        b = x.shape[0]
        plan = self.plan_for(b)
        plan.input[..., :3].copy_(x.to(self._device(), torch.float32).permute(0, 2, 3, 1))
        plan.input[..., 3:].zero_()
        plan.run()
        return plan.out.clone()                      # plan.out is an arena view the next call overwrites

    def embed_resident(self, n):
        """Run the plan on whatever was written into plan_for(n).input; returns (n, D), a view into the plan arena valid
        until the next run at this batch size."""
        plan = self.plan_for(n)
        plan.run()
        return plan.out

    # ---- what FacePipeline asks an embedder ----
    swap_rb = True       # crops in RGB

    def input_lut(self, device):
        """Per-value input LUT of the pipeline's crops: (x - 127.5) / 128 (the 512-d FaceNet weights' convention)."""
        return ((torch.arange(256, dtype=torch.float32) - 127.5) / 128.0).to(device)
