"""`Encoder` and `Decoder` of the frozen AutoencoderKL (reference pipeline/models/autoencoderkl/vae.py)."""
from __future__ import annotations

import torch.nn as tnn

from ...._lib import WfaeError
from .resnet import GN_EPS, Conv3x3
from .unet_2d_blocks import UNetMidBlock2D, get_down_block, get_up_block


def _check_act(act_fn):
    if act_fn != "silu":
        raise WfaeError(f"act_fn {act_fn!r}: only 'silu' is built")


class Encoder(tnn.Module):
    def __init__(self, in_channels=3, out_channels=3, down_block_types=("DownEncoderBlock2D",), block_out_channels=(64,),
                 layers_per_block=2, norm_num_groups=32, act_fn="silu", double_z=True):
        super().__init__()
        _check_act(act_fn)
        if len(down_block_types) != len(block_out_channels):
            raise WfaeError("Encoder: down_block_types and block_out_channels differ in length")
        self.layers_per_block = layers_per_block
        self.conv_in = Conv3x3(in_channels, block_out_channels[0])
        self.mid_block = None
        self.down_blocks = tnn.ModuleList([])
        out_c = block_out_channels[0]
        for i, kind in enumerate(down_block_types):
            in_c, out_c = out_c, block_out_channels[i]
            self.down_blocks.append(get_down_block(kind, num_layers=layers_per_block, in_channels=in_c, out_channels=out_c,
                                                   add_downsample=i != len(block_out_channels) - 1, resnet_eps=GN_EPS,
                                                   resnet_groups=norm_num_groups, downsample_padding=0))
        self.mid_block = UNetMidBlock2D(block_out_channels[-1], resnet_eps=GN_EPS, resnet_groups=norm_num_groups,
                                        output_scale_factor=1)
        self.conv_norm_out = tnn.GroupNorm(num_channels=block_out_channels[-1], num_groups=norm_num_groups, eps=GN_EPS)
        self.conv_act = tnn.SiLU()
        self.conv_out = Conv3x3(block_out_channels[-1], 2 * out_channels if double_z else out_channels)

    def forward(self, x):
        x = self.conv_in(x)
        for block in self.down_blocks:
            x = block(x)
        x = self.mid_block(x)
        return self.conv_out(x, norm=self.conv_norm_out)


class Decoder(tnn.Module):
    def __init__(self, in_channels=3, out_channels=3, up_block_types=("UpDecoderBlock2D",), block_out_channels=(64,),
                 layers_per_block=2, norm_num_groups=32, act_fn="silu"):
        super().__init__()
        _check_act(act_fn)
        if len(up_block_types) != len(block_out_channels):
            raise WfaeError("Decoder: up_block_types and block_out_channels differ in length")
        self.layers_per_block = layers_per_block
        self.conv_in = Conv3x3(in_channels, block_out_channels[-1])
        self.mid_block = None
        self.up_blocks = tnn.ModuleList([])   # registered in front of mid_block, created after it
        self.mid_block = UNetMidBlock2D(block_out_channels[-1], resnet_eps=GN_EPS, resnet_groups=norm_num_groups,
                                        output_scale_factor=1)
        rev = list(reversed(block_out_channels))
        out_c = rev[0]
        for i, kind in enumerate(up_block_types):
            in_c, out_c = out_c, rev[i]
            self.up_blocks.append(get_up_block(kind, num_layers=layers_per_block + 1, in_channels=in_c, out_channels=out_c,
                                               add_upsample=i != len(block_out_channels) - 1, resnet_eps=GN_EPS,
                                               resnet_groups=norm_num_groups))
        self.conv_norm_out = tnn.GroupNorm(num_channels=block_out_channels[0], num_groups=norm_num_groups, eps=GN_EPS)
        self.conv_act = tnn.SiLU()
        self.conv_out = Conv3x3(block_out_channels[0], out_channels)

    def forward(self, z):
        x = self.mid_block(self.conv_in(z))
        for block in self.up_blocks:
            x = block(x)
        return self.conv_out(x, norm=self.conv_norm_out)
