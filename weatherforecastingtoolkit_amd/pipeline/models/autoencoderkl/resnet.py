"""Convolutional building blocks of the frozen AutoencoderKL (reference pipeline/models/autoencoderkl/resnet.py:
`ResnetBlock2D`, `Downsample2D`, `Upsample2D`), forward only, on csrc/aekl.hip.

The torch classes are parameter containers: created in the reference's order with torch's default initialisation, so
state_dict keys / order / shapes and the seeded initial values are the reference's.  A block runs as
    GroupNorm statistics -> 3x3 conv with the GroupNorm + SiLU prologue -> statistics -> 3x3 conv with the prologue and
    the residual (+ 1x1 shortcut) / scale epilogue:
the normalised tensors, the padded tensor of `Downsample2D` and the upsampled tensor of `Upsample2D` are never written.
"""
from __future__ import annotations

import torch.nn as tnn

from .... import functional as Fn
from .... import ops
from ...._lib import WfaeError

GN_EPS = 1e-6


class Conv3x3(tnn.Conv2d):
    """nn.Conv2d(cin, cout, 3) of the provider.  The weights are frozen: they are packed (and split into bf16 planes)
    once per arithmetic mode and device, again only when the parameter is written (load_state_dict) or moved."""

    def __init__(self, cin, cout, stride=1, padding=1):
        super().__init__(cin, cout, kernel_size=3, stride=stride, padding=padding)
        self._packed = {}

    def packed(self, mode):
        w = self.weight
        key = (mode, w.device, w.data_ptr(), w._version)
        hit = self._packed.get(mode)
        if hit is None or hit[0] != key:
            hit = (key, ops.aekl_conv3_pack(w.detach().contiguous(), mode))
            self._packed[mode] = hit
        return hit[1]

    def forward(self, x, gn=None, res=None, kind=0, out_mul=1.0):
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise WfaeError(f"Conv3x3: expected (N, {self.in_channels}, H, W), got {tuple(x.shape)}")
        mode = ops.aekl_mode()
        return Fn.aekl_conv3x3(x, self.packed(mode), self.out_channels, self.bias, gn, res, kind, out_mul, mode)


def group_norm_affine(norm, x):
    """folded (scale, shift) per (sample, channel) of `norm` = nn.GroupNorm on x"""
    return Fn.aekl_group_norm_stats(x, norm.weight, norm.bias, norm.num_groups, norm.eps)[2:]


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
        h = self.conv1(x, gn=group_norm_affine(self.norm1, x))
        gn2 = group_norm_affine(self.norm2, h)
        if self.conv_shortcut is not None:
            sc = self.conv_shortcut
            x = ops.conv1x1_fwd(x, sc.weight.detach().view(self.out_channels, self.in_channels), sc.bias.detach())
        return self.conv2(h, gn=gn2, res=x, out_mul=1.0 / self.output_scale_factor)
