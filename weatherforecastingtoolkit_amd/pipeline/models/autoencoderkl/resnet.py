"""Convolutional building blocks of the frozen AutoencoderKL (reference pipeline/models/autoencoderkl/resnet.py:
`ResnetBlock2D`, `Downsample2D`, `Upsample2D`) on csrc/aekl.hip; after `AutoencoderKL.unfreeze()` with a graph, whose
backward runs on csrc/aekl_bwd.hip.

The torch classes are parameter containers: created in the reference's order with torch's default initialisation, so
state_dict keys / order / shapes and the seeded initial values are the reference's.  A block runs as
    GroupNorm statistics -> 3x3 conv with the GroupNorm + SiLU prologue -> statistics -> 3x3 conv with the prologue and
    the residual (+ 1x1 shortcut) / scale epilogue:
the normalised tensors, the padded tensor of `Downsample2D` and the upsampled tensor of `Upsample2D` are never written.
"""
from __future__ import annotations

import torch
import torch.nn as tnn

from .... import functional as Fn
from .... import ops
from ...._lib import WfaeError

GN_EPS = 1e-6


def trains(p):
    """whether a layer with parameter p builds a graph: the parameter was unfrozen and autograd is recording"""
    return p.requires_grad and torch.is_grad_enabled()


class Conv3x3(tnn.Conv2d):
    """nn.Conv2d(cin, cout, 3) of the provider.  The weights are packed (and split into bf16 planes) once per arithmetic
    mode, orientation and device, again only when the parameter is written (load_state_dict, an optimiser step) or moved."""

    def __init__(self, cin, cout, stride=1, padding=1):
        super().__init__(cin, cout, kernel_size=3, stride=stride, padding=padding)
        self._packed = {}

    def _pack(self, mode, transposed):
        w = self.weight
        key = (mode, w.device, w.data_ptr(), w._version)
        slot = (mode, transposed)
        hit = self._packed.get(slot)
        if hit is None or hit[0] != key:
            src = w.detach().flip(2, 3).transpose(0, 1) if transposed else w.detach()
            hit = (key, ops.aekl_conv3_pack(src.contiguous(), mode))
            self._packed[slot] = hit
        return hit[1]

    def packed(self, mode):
        return self._pack(mode, False)

    def packed_t(self, mode):
        """the weights rotated 180 degrees with in / out transposed: the operand of the data gradient"""
        return self._pack(mode, True)

    def forward(self, x, norm=None, res=None, kind=0, out_mul=1.0):
        """conv3x3(x), or conv3x3(SiLU(norm(x))) with `norm` an nn.GroupNorm; (+ bias + res) * out_mul"""
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise WfaeError(f"Conv3x3: expected (N, {self.in_channels}, H, W), got {tuple(x.shape)}")
        mode = ops.aekl_mode()
        if trains(self.weight):
            return Fn.aekl_conv3x3_train(x, self, norm, res, kind, out_mul, mode)
        gn = None if norm is None else group_norm_affine(norm, x)
        return Fn.aekl_conv3x3(x, self.packed(mode), self.out_channels, self.bias, gn, res, kind, out_mul, mode)


def group_norm_affine(norm, x):
    """folded (scale, shift) per (sample, channel) of `norm` = nn.GroupNorm on x"""
    return Fn.aekl_group_norm_stats(x, norm.weight, norm.bias, norm.num_groups, norm.eps)[2:]


def conv1x1(conv, x):
    """nn.Conv2d(cin, cout, 1) on the 1x1 kernels; with `conv.row_invariant` (`AutoencoderKL.pass_invariant()`, frozen only) on
    the form whose result for a sample does not depend on the batch"""
    if trains(conv.weight):
        return Fn.conv1x1(x, conv.weight, conv.bias)
    if getattr(conv, "row_invariant", False):
        return Fn.aekl_conv1x1_rowinv(x, conv.weight, conv.bias)
    return ops.conv1x1_fwd(x, conv.weight.detach().view(conv.out_channels, conv.in_channels), conv.bias.detach())


class Downsample2D(tnn.Module):
    """conv 3x3 stride 2 with `padding`; the reference pads (0, 1, 0, 1) in front of a padding-0 convolution, which is
    the only form its encoder builds"""

    def __init__(self, channels, use_conv=True, out_channels=None, padding=0, name="op"):
        super().__init__()
        if not use_conv or padding != 0:
            raise WfaeError("Downsample2D: only the convolutional form with padding=0 (pad (0, 1, 0, 1), stride 2) is built")
        self.channels, self.out_channels, self.padding = channels, out_channels or channels, padding
        self.conv = Conv3x3(channels, self.out_channels, stride=2, padding=0)

    def forward(self, x):
        return self.conv(x, kind=ops.AEKL_KINDS["down"])


class Upsample2D(tnn.Module):
    """nearest x2 upsample + conv 3x3; the convolution reads its input through the upsample"""

    def __init__(self, channels, use_conv=True, out_channels=None):
        super().__init__()
        if not use_conv:
            raise WfaeError("Upsample2D: only the convolutional form is built")
        self.channels, self.out_channels = channels, out_channels or channels
        self.conv = Conv3x3(channels, self.out_channels)

    def forward(self, x):
        return self.conv(x, kind=ops.AEKL_KINDS["up"])


class ResnetBlock2D(tnn.Module):
    """norm1 -> SiLU -> conv1 -> norm2 -> SiLU -> conv2, + input (through a 1x1 `conv_shortcut` when the channel count
    changes), / output_scale_factor.  No time embedding, dropout 0 (the autoencoder's configuration)."""

    def __init__(self, *, in_channels, out_channels=None, groups=32, eps=GN_EPS, output_scale_factor=1.0):
        super().__init__()
        out_channels = in_channels if out_channels is None else out_channels
        self.in_channels, self.out_channels = in_channels, out_channels
        self.output_scale_factor = output_scale_factor
        self.norm1 = tnn.GroupNorm(num_groups=groups, num_channels=in_channels, eps=eps, affine=True)
        self.conv1 = Conv3x3(in_channels, out_channels)
        self.norm2 = tnn.GroupNorm(num_groups=groups, num_channels=out_channels, eps=eps, affine=True)
        self.conv2 = Conv3x3(out_channels, out_channels)
        self.conv_shortcut = None
        if in_channels != out_channels:
            self.conv_shortcut = tnn.Conv2d(in_channels, out_channels, kernel_size=1, stride=1, padding=0)

    def forward(self, x, temb=None):
        if temb is not None:
            raise WfaeError("ResnetBlock2D: the autoencoder has no time embedding")
        h = self.conv1(x, norm=self.norm1)
        if self.conv_shortcut is not None:
            x = conv1x1(self.conv_shortcut, x)
        return self.conv2(h, norm=self.norm2, res=x, out_mul=1.0 / self.output_scale_factor)
