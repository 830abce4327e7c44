"""Parameter containers with the reference's ``state_dict`` key names.

They hold weights only; calling them raises.  All arithmetic of the hot path
runs in the HIP plan built from these parameters (plan.py), never in torch.
"""
import math

import torch
import torch.nn as nn

from ..plan import bn_affine


class _NoCompute(nn.Module):
    def forward(self, *a, **k):
        raise RuntimeError(f"{type(self).__name__} is a parameter container; the network runs as a HIP plan "
                           "(libfacepath.so), not through torch modules")


class ConvParams(_NoCompute):
    """Keys: ``weight`` [O, I/g, k, k] (+ ``bias``) like nn.Conv2d."""

    def __init__(self, cin, cout, k, stride=1, padding=0, groups=1, bias=True):
        super().__init__()
        self.in_channels, self.out_channels = cin, cout
        self.kernel_size, self.stride, self.padding, self.groups = k, stride, padding, groups
        self.weight = nn.Parameter(torch.empty(cout, cin // groups, k, k), requires_grad=False)
        fan_in = (cin // groups) * k * k
        nn.init.normal_(self.weight, 0.0, math.sqrt(2.0 / fan_in))
        if bias:
            self.bias = nn.Parameter(torch.zeros(cout), requires_grad=False)
        else:
            self.register_parameter("bias", None)


class BNParams(_NoCompute):
    """Keys: weight, bias, running_mean, running_var, num_batches_tracked like nn.BatchNorm{1,2}d (eval mode)."""

    def __init__(self, c, eps=1e-5):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(c), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(c), requires_grad=False)
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))


class PReLUParams(_NoCompute):
    def __init__(self, c):
        super().__init__()
        self.weight = nn.Parameter(torch.full((c,), 0.25), requires_grad=False)


class LinearParams(_NoCompute):
    def __init__(self, cin, cout, bias=False):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin), requires_grad=False)
        nn.init.normal_(self.weight, 0.0, math.sqrt(1.0 / cin))
        if bias:
            self.bias = nn.Parameter(torch.zeros(cout), requires_grad=False)
        else:
            self.register_parameter("bias", None)


def npy(t):
    return t.detach().cpu().numpy()


def bn_sb(bn):
    """(scale, bias) of an eval-mode BatchNorm (BNParams) as the epilogue affine y = x * scale + bias."""
    return bn_affine(npy(bn.weight), npy(bn.bias), npy(bn.running_mean), npy(bn.running_var), bn.eps)


class PlanCacheMixin:
    """For a network (in front of nn.Module in its bases) that keeps its compiled plans in ``self._plans`` (plan.PlanCache):
    the plans hold packed copies of the weights, so whatever replaces or moves the parameters -- load_state_dict, .to() /
    .cuda() through _apply -- drops them.  A network with more derived state overrides _invalidate().  The mixin holds no
    parameter, buffer or submodule."""

    def _invalidate(self):
        self._plans.clear()

    def load_state_dict(self, *a, **k):
        out = super().load_state_dict(*a, **k)
        self._invalidate()
        return out

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self._invalidate()
        return out
