"""Mid-block attention of the frozen AutoencoderKL (reference pipeline/models/autoencoderkl/attention.py
`AttentionBlock`): GroupNorm, one head over the h*w tokens, projection, residual; with a graph after `AutoencoderKL.unfreeze()`."""
from __future__ import annotations

import torch.nn as tnn

from .... import functional as Fn
from ...._lib import WfaeError
from .resnet import group_norm_affine, trains


class AttentionBlock(tnn.Module):
    def __init__(self, channels, num_head_channels=None, norm_num_groups=32, rescale_output_factor=1.0, eps=1e-5):
        super().__init__()
        if num_head_channels is not None and num_head_channels != channels:
            raise WfaeError("AttentionBlock: only the single-head form (num_head_channels=None) is built")
        self.channels = channels
        self.num_heads = 1
        self.group_norm = tnn.GroupNorm(num_channels=channels, num_groups=norm_num_groups, eps=eps, affine=True)
        self.query = tnn.Linear(channels, channels)
        self.key = tnn.Linear(channels, channels)
        self.value = tnn.Linear(channels, channels)
        self.rescale_output_factor = rescale_output_factor
        self.proj_attn = tnn.Linear(channels, channels, bias=True)
        self.row_invariant = False      # `AutoencoderKL.pass_invariant()`: the projections on linear_fwd_rowinv (frozen only)

    def forward(self, x):
        if x.dim() != 4 or x.shape[1] != self.channels:
            raise WfaeError(f"AttentionBlock: expected (N, {self.channels}, H, W), got {tuple(x.shape)}")
        s = x.shape[2] * x.shape[3]
        if s % 32 or self.channels % 32:
            raise WfaeError(f"AttentionBlock: tokens S = H*W and channels must be multiples of 32 (got S={s}, "
                            f"C={self.channels})")
        q, k, v, o = self.query, self.key, self.value, self.proj_attn
        if trains(q.weight):
            if self.row_invariant:
                raise WfaeError("AttentionBlock: row_invariant belongs to the frozen provider, the training path has no such form")
            return Fn.aekl_attention_train(x, self.group_norm, q, k, v, o, self.rescale_output_factor)
        return Fn.aekl_attention(x, group_norm_affine(self.group_norm, x), q.weight, q.bias, k.weight, k.bias, v.weight,
                                 v.bias, o.weight, o.bias, self.rescale_output_factor, row_invariant=self.row_invariant)
