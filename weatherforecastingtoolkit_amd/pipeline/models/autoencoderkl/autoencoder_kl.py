"""`AutoencoderKL` of the v1 experiments on MI355X (reference pipeline/models/autoencoderkl/autoencoder_kl.py): the
reference's constructor keywords, state_dict keys / order / shapes and seeded initial values;
`encode(x) -> DiagonalGaussianDistribution`, `decode(z)`, `forward(...)`.  By default it is the frozen latent provider,
forward only: the parameters are frozen and an input that asks for a gradient is refused (WfaeError) rather than answered
without a graph.  `unfreeze()` opts into training: the parameters require gradients and the three calls build a graph
whose backward runs on csrc/aekl_bwd.hip; `freeze()` goes back.  A reference checkpoint loads with `load_state_dict`."""
from __future__ import annotations

import torch
import torch.nn as tnn

from ...._lib import WfaeError
from .distributions import DiagonalGaussianDistribution
from .resnet import conv1x1
from .vae import Decoder, Encoder


class AutoencoderKL(tnn.Module):
    def __init__(self, in_channels=3, out_channels=3, down_block_types=("DownEncoderBlock2D",),
                 up_block_types=("UpDecoderBlock2D",), block_out_channels=(64,), layers_per_block=1, act_fn="silu",
                 latent_channels=4, norm_num_groups=32, sample_size=32, scaling_factor=0.18215):
        super().__init__()
        block_out_channels = tuple(int(c) for c in block_out_channels)
        for c in block_out_channels:
            if c % norm_num_groups:
                raise WfaeError(f"AutoencoderKL: {c} channels are not divisible into {norm_num_groups} groups")
        self.latent_channels, self.scaling_factor, self.sample_size = latent_channels, scaling_factor, sample_size
        self.downscale = 2 ** (len(block_out_channels) - 1)
        self.encoder = Encoder(in_channels=in_channels, out_channels=latent_channels,
                               down_block_types=tuple(down_block_types), block_out_channels=block_out_channels,
                               layers_per_block=layers_per_block, act_fn=act_fn, norm_num_groups=norm_num_groups,
                               double_z=True)
        self.decoder = Decoder(in_channels=latent_channels, out_channels=out_channels, up_block_types=tuple(up_block_types),
                               block_out_channels=block_out_channels, layers_per_block=layers_per_block,
                               norm_num_groups=norm_num_groups, act_fn=act_fn)
        self.quant_conv = tnn.Conv2d(2 * latent_channels, 2 * latent_channels, 1)
        self.post_quant_conv = tnn.Conv2d(latent_channels, latent_channels, 1)
        self.use_slicing = False
        self.invariant = False
        self.freeze()

    def freeze(self):
        """the latent provider (the default): eval mode, no parameter asks for a gradient, no call builds a graph"""
        self.trainable = False
        super().train(False)
        for p in self.parameters():
            p.requires_grad_(False)
        return self

    def unfreeze(self):
        """opt into training: parameters require gradients, `train(mode)` behaves as for any module, and `encode` /
        `decode` / `forward` build a graph when autograd is recording"""
        if self.invariant:
            raise WfaeError("AutoencoderKL.unfreeze: the model is in pass-invariant mode, which belongs to the frozen provider "
                            "(the training path has no row-invariant kernels): call pass_invariant(False) first")
        self.trainable = True
        for p in self.parameters():
            p.requires_grad_(True)
        return self

    def pass_invariant(self, flag=True):
        """frozen provider only: make the result for a sample the same bits whatever else shares its `encode` / `decode`
        call.  Two things depend on the pass size: the summation order of the four projections of every `AttentionBlock`
        (their GEMM rows are samples x tokens), and the instruction of the 1x1 convolutions with 128 or more input channels
        (the ResNet shortcuts, `quant_conv`, `post_quant_conv`: gemm.hip picks the split or the fp32 form by the column
        count).  With the flag both run on ops.linear_fwd_rowinv (functional.aekl_attention(row_invariant=True),
        functional.aekl_conv1x1_rowinv).  The values differ from the default mode's in the last bits, and so do not
        replace it silently.  -> self"""
        if self.trainable:
            raise WfaeError("AutoencoderKL.pass_invariant: the model is unfrozen; pass-invariant mode belongs to the frozen "
                            "provider (freeze() first)")
        from .attention import AttentionBlock
        self.invariant = bool(flag)
        for m in self.modules():
            if isinstance(m, AttentionBlock) or (isinstance(m, tnn.Conv2d) and tuple(m.kernel_size) == (1, 1)):
                m.row_invariant = self.invariant
        return self

    def train(self, mode=True):
        return super().train(mode if self.trainable else False)   # frozen: there is no training-mode behaviour

    def _check(self, what, x, channels):
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != channels:
            raise WfaeError(f"AutoencoderKL.{what}: expected (N, {channels}, H, W), got "
                            f"{tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
        if self.trainable:
            return x.contiguous()
        if torch.is_grad_enabled() and x.requires_grad:
            raise WfaeError(f"AutoencoderKL.{what} is forward only (frozen provider): call it under torch.no_grad() or "
                            "detach the input, or opt into training with unfreeze()")
        return x.detach().contiguous()

    def _graph(self):
        return torch.set_grad_enabled(self.trainable and torch.is_grad_enabled())

    def _encode(self, x):
        d = self.downscale
        if x.shape[2] % d or x.shape[3] % d:
            raise WfaeError(f"AutoencoderKL.encode: the plane {tuple(x.shape[2:])} is not divisible by {d}")
        with self._graph():
            return conv1x1(self.quant_conv, self.encoder(x))

    def moments(self, x):
        """the quant_conv output (N, 2 * latent channels, h, w) that `encode` wraps into the distribution"""
        return self._encode(self._check("encode", x, self.encoder.conv_in.in_channels))

    def encode(self, x):
        moments = self.moments(x)
        with self._graph():
            return DiagonalGaussianDistribution(moments)

    def _decode(self, z):
        with self._graph():
            return self.decoder(conv1x1(self.post_quant_conv, z))

    def enable_slicing(self):
        self.use_slicing = True

    def disable_slicing(self):
        self.use_slicing = False

    def decode(self, z):
        z = self._check("decode", z, self.latent_channels)
        if self.use_slicing and z.shape[0] > 1:
            return torch.cat([self._decode(s.contiguous()) for s in z.split(1)])
        return self._decode(z)

    def forward(self, sample, sample_posterior=False, return_posterior=False, generator=None):
        posterior = self.encode(sample)
        z = posterior.sample(generator=generator) if sample_posterior else posterior.mode()
        dec = self.decode(z)
        return (dec, posterior) if return_posterior else dec
