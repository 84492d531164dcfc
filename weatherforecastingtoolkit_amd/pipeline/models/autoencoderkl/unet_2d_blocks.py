"""Blocks of the frozen AutoencoderKL (reference pipeline/models/autoencoderkl/unet_2d_blocks.py): `DownEncoderBlock2D`,
`UpDecoderBlock2D`, `UNetMidBlock2D` and the two factories.  Submodules are created in the reference's order."""
from __future__ import annotations

import torch.nn as tnn

from ...._lib import WfaeError
from .attention import AttentionBlock
from .resnet import Downsample2D, ResnetBlock2D, Upsample2D


def get_down_block(down_block_type, num_layers, in_channels, out_channels, add_downsample, resnet_eps, resnet_groups,
                   downsample_padding):
    if down_block_type != "DownEncoderBlock2D":
        raise WfaeError(f"down block type {down_block_type!r}: only 'DownEncoderBlock2D' is built")
    return DownEncoderBlock2D(in_channels, out_channels, num_layers=num_layers, resnet_eps=resnet_eps,
                              resnet_groups=resnet_groups, add_downsample=add_downsample,
                              downsample_padding=downsample_padding)


def get_up_block(up_block_type, num_layers, in_channels, out_channels, add_upsample, resnet_eps, resnet_groups):
    if up_block_type != "UpDecoderBlock2D":
        raise WfaeError(f"up block type {up_block_type!r}: only 'UpDecoderBlock2D' is built")
    return UpDecoderBlock2D(in_channels, out_channels, num_layers=num_layers, resnet_eps=resnet_eps,
                            resnet_groups=resnet_groups, add_upsample=add_upsample)


class UNetMidBlock2D(tnn.Module):
    """resnet, attention, resnet; state_dict order `attentions` then `resnets`, creation order resnet, attention, resnet"""

    def __init__(self, in_channels, resnet_eps=1e-6, resnet_groups=32, output_scale_factor=1.0):
        super().__init__()
        def resnet():
            return ResnetBlock2D(in_channels=in_channels, out_channels=in_channels, eps=resnet_eps, groups=resnet_groups,
                                 output_scale_factor=output_scale_factor)
        first = resnet()
        attn = AttentionBlock(in_channels, num_head_channels=None, rescale_output_factor=output_scale_factor,
                              eps=resnet_eps, norm_num_groups=resnet_groups)
        second = resnet()
        self.attentions = tnn.ModuleList([attn])
        self.resnets = tnn.ModuleList([first, second])

    def forward(self, x):
        x = self.resnets[0](x)
        for attn, resnet in zip(self.attentions, self.resnets[1:]):
            x = resnet(attn(x))
        return x


class DownEncoderBlock2D(tnn.Module):
    def __init__(self, in_channels, out_channels, num_layers=1, resnet_eps=1e-6, resnet_groups=32, output_scale_factor=1.0,
                 add_downsample=True, downsample_padding=1):
        super().__init__()
        self.resnets = tnn.ModuleList([
            ResnetBlock2D(in_channels=in_channels if i == 0 else out_channels, out_channels=out_channels, eps=resnet_eps,
                          groups=resnet_groups, output_scale_factor=output_scale_factor) for i in range(num_layers)])
        self.downsamplers = None
        if add_downsample:
            self.downsamplers = tnn.ModuleList([Downsample2D(out_channels, use_conv=True, out_channels=out_channels,
                                                             padding=downsample_padding, name="op")])

    def forward(self, x):
        for resnet in self.resnets:
            x = resnet(x)
        for down in self.downsamplers or ():
            x = down(x)
        return x


class UpDecoderBlock2D(tnn.Module):
    def __init__(self, in_channels, out_channels, num_layers=1, resnet_eps=1e-6, resnet_groups=32, output_scale_factor=1.0,
                 add_upsample=True):
        super().__init__()
        self.resnets = tnn.ModuleList([
            ResnetBlock2D(in_channels=in_channels if i == 0 else out_channels, out_channels=out_channels, eps=resnet_eps,
                          groups=resnet_groups, output_scale_factor=output_scale_factor) for i in range(num_layers)])
        self.upsamplers = None
        if add_upsample:
            self.upsamplers = tnn.ModuleList([Upsample2D(out_channels, use_conv=True, out_channels=out_channels)])

    def forward(self, x):
        for resnet in self.resnets:
            x = resnet(x)
        for up in self.upsamplers or ():
            x = up(x)
        return x
