"""Plain-torch functional restatement of the frozen AutoencoderKL (state dict -> outputs), the CPU oracle of
tests/test_aekl_*.py and the eager baseline of tools/aekl_bench.py.  Written from the architecture:

  encoder: conv_in 3x3 -> per level [resnet x layers_per_block, then (all but the last level) pad (0, 1, 0, 1) + conv 3x3
           stride 2] -> mid (resnet, attention, resnet) -> GroupNorm -> SiLU -> conv_out 3x3 (2 x latent channels)
  moments = quant_conv 1x1; mean, logvar = halves; logvar clamped to [-30, 20]; std = exp(logvar / 2)
  decoder: post_quant_conv 1x1 -> conv_in 3x3 -> mid -> per level [resnet x (layers_per_block + 1), then (all but the
           last) nearest x2 + conv 3x3] -> GroupNorm -> SiLU -> conv_out 3x3
  resnet:  x + conv2(silu(gn2(conv1(silu(gn1(x)))))), x through a 1x1 conv_shortcut when the channel count changes
  attention: one head over the h*w tokens of gn(x): softmax(q k^T / sqrt(C)) v, projected, + x
  GroupNorm eps 1e-6 everywhere.

It runs in the dtype / on the device of the state dict it is given (fp32 or fp64).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

EPS = 1e-6

CONFIGS = {
    # (a) of tests/golden/g14_aekl.npz: small, stored in full
    "small": dict(in_channels=1, out_channels=1, down_block_types=("DownEncoderBlock2D",) * 3,
                  up_block_types=("UpDecoderBlock2D",) * 3, block_out_channels=(32, 64, 64), layers_per_block=1,
                  act_fn="silu", latent_channels=4, norm_num_groups=8),
    # (b) the reference configuration of the v1 experiments with 64 latent channels
    "ref64": dict(in_channels=1, out_channels=1, down_block_types=("DownEncoderBlock2D",) * 4,
                  up_block_types=("UpDecoderBlock2D",) * 4, block_out_channels=(128, 256, 512, 512), layers_per_block=2,
                  act_fn="silu", latent_channels=64, norm_num_groups=32),
    # (c) the same with the 4 latent channels of pretrained_ae_convae_sevir
    "ref4": dict(in_channels=1, out_channels=1, down_block_types=("DownEncoderBlock2D",) * 4,
                 up_block_types=("UpDecoderBlock2D",) * 4, block_out_channels=(128, 256, 512, 512), layers_per_block=2,
                 act_fn="silu", latent_channels=4, norm_num_groups=32),
}


def _gn(sd, p, x, groups):
    return F.group_norm(x, groups, sd[p + ".weight"], sd[p + ".bias"], EPS)


def _conv(sd, p, x, **kw):
    return F.conv2d(x, sd[p + ".weight"], sd[p + ".bias"], **kw)


def resnet(sd, p, x, groups):
    h = _conv(sd, p + ".conv1", F.silu(_gn(sd, p + ".norm1", x, groups)), padding=1)
    h = _conv(sd, p + ".conv2", F.silu(_gn(sd, p + ".norm2", h, groups)), padding=1)
    if p + ".conv_shortcut.weight" in sd:
        x = _conv(sd, p + ".conv_shortcut", x)
    return x + h


def attention(sd, p, x, groups):
    n, c, h, w = x.shape
    t = _gn(sd, p + ".group_norm", x, groups).reshape(n, c, h * w).transpose(1, 2)
    q = F.linear(t, sd[p + ".query.weight"], sd[p + ".query.bias"])
    k = F.linear(t, sd[p + ".key.weight"], sd[p + ".key.bias"])
    v = F.linear(t, sd[p + ".value.weight"], sd[p + ".value.bias"])
    a = torch.softmax(q @ k.transpose(1, 2) * (1.0 / c ** 0.5), dim=-1)
    o = F.linear(a @ v, sd[p + ".proj_attn.weight"], sd[p + ".proj_attn.bias"])
    return o.transpose(1, 2).reshape(n, c, h, w) + x


def mid(sd, p, x, groups):
    x = resnet(sd, p + ".resnets.0", x, groups)
    x = attention(sd, p + ".attentions.0", x, groups)
    return resnet(sd, p + ".resnets.1", x, groups)


def encoder(sd, x, cfg):
    g, levels = cfg["norm_num_groups"], len(cfg["block_out_channels"])
    x = _conv(sd, "encoder.conv_in", x, padding=1)
    for i in range(levels):
        for j in range(cfg["layers_per_block"]):
            x = resnet(sd, f"encoder.down_blocks.{i}.resnets.{j}", x, g)
        if i != levels - 1:
            x = _conv(sd, f"encoder.down_blocks.{i}.downsamplers.0.conv", F.pad(x, (0, 1, 0, 1)), stride=2)
    x = mid(sd, "encoder.mid_block", x, g)
    return _conv(sd, "encoder.conv_out", F.silu(_gn(sd, "encoder.conv_norm_out", x, g)), padding=1)


def decoder(sd, z, cfg):
    g, levels = cfg["norm_num_groups"], len(cfg["block_out_channels"])
    x = mid(sd, "decoder.mid_block", _conv(sd, "decoder.conv_in", z, padding=1), g)
    for i in range(levels):
        for j in range(cfg["layers_per_block"] + 1):
            x = resnet(sd, f"decoder.up_blocks.{i}.resnets.{j}", x, g)
        if i != levels - 1:
            x = _conv(sd, f"decoder.up_blocks.{i}.upsamplers.0.conv", F.interpolate(x, scale_factor=2.0, mode="nearest"),
                      padding=1)
    return _conv(sd, "decoder.conv_out", F.silu(_gn(sd, "decoder.conv_norm_out", x, g)), padding=1)


def encode(sd, x, cfg, noise=None):
    """-> dict(mean, logvar, std, mode, sample (with noise))"""
    m = _conv(sd, "quant_conv", encoder(sd, x, cfg))
    mean, logvar = torch.chunk(m, 2, dim=1)
    logvar = torch.clamp(logvar, -30.0, 20.0)
    std = torch.exp(0.5 * logvar)
    out = dict(mean=mean, logvar=logvar, std=std, mode=mean)
    if noise is not None:
        out["sample"] = mean + std * noise
    return out


def decode(sd, z, cfg):
    return decoder(sd, _conv(sd, "post_quant_conv", z), cfg)


def cast(sd, dtype=None, device=None):
    return {k: v.to(dtype=dtype, device=device) for k, v in sd.items()}


def rel_err(got, want):
    """max |got - want| / max |want| (the measure of tests/test_convae_gpu.py)"""
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))
