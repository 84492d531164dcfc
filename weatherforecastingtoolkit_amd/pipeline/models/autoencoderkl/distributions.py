"""`DiagonalGaussianDistribution` of the AutoencoderKL (reference pipeline/models/autoencoderkl/distributions.py): mean,
clamped logvar, std and samples come from one kernel (csrc/aekl.hip posterior).  On moments that carry a graph (an unfrozen
AutoencoderKL), `sample()`, `mode()` and `kl()` are differentiable (csrc/aekl_bwd.hip posterior_bwd); the read-outs
`mean`, `logvar`, `std` stay plain tensors."""
from __future__ import annotations

import torch

from .... import functional as Fn


class DiagonalGaussianDistribution:
    def __init__(self, parameters, deterministic=False):
        self.parameters = parameters
        self.deterministic = deterministic
        self.graph = torch.is_grad_enabled() and parameters.requires_grad
        self.mean, self.logvar, self.std, _ = Fn.aekl_posterior(parameters.detach())
        if deterministic:
            self.std = torch.zeros_like(self.mean)

    @property
    def var(self):
        return self.std * self.std

    def mode(self):
        if self.graph:
            return Fn.AeklPosteriorSampleFn.apply(self.parameters, None)
        return self.mean

    def sample(self, generator=None, noise=None):
        """mean + std * noise; `noise` (keyword extension) replaces the draw torch.randn(mean.shape, generator=...)"""
        if noise is None:
            noise = torch.randn(self.mean.shape, generator=generator, device=self.parameters.device,
                                dtype=self.parameters.dtype)
        if self.deterministic:
            return self.mode()
        if self.graph:
            return Fn.AeklPosteriorSampleFn.apply(self.parameters, noise)
        return Fn.aekl_posterior(self.parameters, noise)[3]

    def kl(self, other=None):
        """0.5 sum(mean^2 + var - 1 - logvar) per sample (against `other` when given); a scalar-sized read-out, not a
        hot path: torch reductions over the kernel's mean / logvar / std"""
        if self.deterministic:
            return torch.Tensor([0.])
        if other is None and self.graph:
            return Fn.AeklPosteriorKlFn.apply(self.parameters)
        if other is None:
            return 0.5 * torch.sum(self.mean * self.mean + self.var - 1.0 - self.logvar, dim=[1, 2, 3])
        d = self.mean - other.mean
        return 0.5 * torch.sum(d * d / other.var + self.var / other.var - 1.0 - self.logvar + other.logvar, dim=[1, 2, 3])
