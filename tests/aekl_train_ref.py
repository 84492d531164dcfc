"""The AutoencoderKL training loss and its gradients by torch autograd over tests/aekl_ref.py, in the dtype / on the device of
the state dict: the CPU oracle of tests/test_aekl_train_*.py and the eager baseline of tools/aekl_train_bench.py.

    loss = mean |decode(z) - x| + kl_weight * sum_n KL_n / B,   KL_n = 0.5 sum(mean^2 + var - 1 - logvar)
    z = mean + std * noise  (`noise` given)  or  the mean (`noise` None: `posterior.mode()`)
"""
from __future__ import annotations

import torch

from tests import aekl_ref as A

KL_WEIGHT = 1e-2
NSAMPLE = 512       # a gradient of more than BIG elements is recorded as NSAMPLE of them + its L2 norm
BIG = 2048


def sample_index(numel):
    return torch.arange(NSAMPLE) * (numel // NSAMPLE)


def kl_per_sample(post):
    return 0.5 * torch.sum(post["mean"] ** 2 + post["std"] ** 2 - 1.0 - post["logvar"], dim=[1, 2, 3])


def loss_of(sd, x, cfg, noise=None, kl_weight=KL_WEIGHT):
    x = x.to(next(iter(sd.values())).dtype)
    post = A.encode(sd, x, cfg, None if noise is None else noise.to(x.dtype))
    dec = A.decode(sd, post["sample"] if noise is not None else post["mode"], cfg)
    loss = (dec - x).abs().mean()
    if kl_weight:
        loss = loss + kl_weight * kl_per_sample(post).sum() / x.shape[0]
    return loss, dec


def loss_and_grads(sd, x, cfg, noise=None, kl_weight=KL_WEIGHT):
    """-> (loss, {key: gradient}); a parameter the loss does not reach (the logvar rows without noise and KL) gets zeros"""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    loss, _ = loss_of(leaves, x, cfg, noise, kl_weight)
    grads = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
    return loss.detach(), {k: (torch.zeros_like(v) if g is None else g) for (k, v), g in zip(leaves.items(), grads)}

