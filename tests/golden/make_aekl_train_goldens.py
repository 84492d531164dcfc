"""Generate tests/golden/g20_aekl_train.npz from the reference's own AutoencoderKL (CPU).

    python tests/golden/make_aekl_train_goldens.py <reference checkout root>

One case: tests/aekl_ref.py CONFIGS["small"], torch.manual_seed(SEED); AutoencoderKL(**config) (the weights are pinned by
`init_sha`, not stored), B = 2 frames 1 x 32 x 32 from Generator().manual_seed(X_SEED) (stored as `x`), `noise` =
torch.randn(latent shape) from Generator().manual_seed(NOISE_SEED): the draw the reference's
`forward(x, sample_posterior=True, generator=...)` makes in fp32.

    loss = mean |forward(x, sample_posterior=True) - x| + 1e-2 * sum(posterior.kl()) / B          -> `loss`, `grad.<key>`
    the same with posterior.mode() and no KL term                                                  -> `mode_loss`, `mode_grad.<key>`

The backward is run in fp64 and in fp32.  Recorded per parameter, as fp64: the fp64 gradient — whole when it has at most
aekl_train_ref.BIG elements or (first loss only) is one of FULL (the first stride-2 layer), else NSAMPLE elements
at aekl_train_ref.sample_index plus `<name>_norm` (L2) and `<name>_max` (max |g|) — and `<name>_spread` =
max|g32 - g64| / max|g64| over the whole tensor.

Which fp64.  The reference's attention casts its scores to fp32 for the softmax whatever the model's dtype, so the backward
of its fp64 copy carries about 1e-8 of fp32 noise.  The recorded fp64 values are those of tests/aekl_train_ref.py (the
plain-torch restatement, fp64 throughout) on the reference model's weights; the reference module's own fp64 backward and
loss are asserted here to agree with them to 2e-7 (the bound make_aekl_goldens.py uses for the forward), and the fp32
side of every spread is the reference module's own fp32 backward.
"""
from __future__ import annotations

import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import aekl_ref as A  # noqa: E402
from tests import aekl_train_ref as T  # noqa: E402
from tests import convae_ref as R  # noqa: E402

SEED, X_SEED, NOISE_SEED = 1234, 3020, 4020
SHAPE = (2, 1, 32, 32)
FULL = ("encoder.down_blocks.0.downsamplers.0.conv.weight",)


def module_loss(model, x, noise_seed, kl_weight):
    """the loss through the reference module's own forward"""
    if kl_weight:
        dec, post = model(x, sample_posterior=True, return_posterior=True, generator=torch.Generator().manual_seed(noise_seed))
        return (dec - x).abs().mean() + kl_weight * post.kl().sum() / x.shape[0]
    return (model(x) - x).abs().mean()


def module_grads(model, x, noise, kl_weight):
    model.zero_grad()
    if kl_weight and x.dtype == torch.float64:
        # the fp64 module would draw another noise (randn in fp64): sample by hand with the stored draw
        post = model.encode(x)
        dec = model.decode(post.mean + post.std * noise.double())
        loss = (dec - x).abs().mean() + kl_weight * post.kl().sum() / x.shape[0]
    else:
        loss = module_loss(model, x, NOISE_SEED, kl_weight)
    loss.backward()
    return loss.detach(), {k: (torch.zeros_like(p) if p.grad is None else p.grad.detach().clone())
                           for k, p in model.named_parameters()}


def main(argv):
    root = argv[1] if len(argv) > 1 else os.environ.get("WFAE_REFERENCE_ROOT")
    if not root:
        raise SystemExit(__doc__)
    sys.path.insert(0, root)
    from pipeline.models.autoencoderkl.autoencoder_kl import AutoencoderKL
    cfg = A.CONFIGS["small"]
    torch.manual_seed(SEED)
    m32 = AutoencoderKL(**cfg).train()
    m64 = copy.deepcopy(m32).double()
    sd0 = {k: v.detach().clone() for k, v in m32.state_dict().items()}
    x = torch.rand(*SHAPE, generator=torch.Generator().manual_seed(X_SEED))
    with torch.no_grad():
        lat = m32.encode(x).mean.shape
    noise = torch.randn(lat, generator=torch.Generator().manual_seed(NOISE_SEED))
    out = {"seed": np.int64(SEED), "config": np.array("small"), "init_sha": np.array(R.values_digest(sd0)),
           "keys": np.array(list(sd0)), "x": x.numpy(), "noise": noise.numpy(), "kl_weight": np.float64(T.KL_WEIGHT)}
    sd64 = A.cast(sd0, torch.float64)
    for prefix, kw, nz in (("", T.KL_WEIGHT, noise), ("mode_", 0.0, None)):
        l32, g32 = module_grads(m32, x, noise, kw)
        l64m, g64m = module_grads(m64, x.double(), noise, kw)
        l64, g64 = T.loss_and_grads(sd64, x.double(), cfg, nz, kw)
        assert abs(float(l64m) - float(l64)) <= 2e-7 * abs(float(l64)), (float(l64m), float(l64))
        out[prefix + "loss"] = np.float64(l64.item())
        out[prefix + "loss_spread"] = np.float64(abs(float(l32) - float(l64)) / abs(float(l64)))
        print(f"{prefix}loss {float(l64):.12f} spread {float(out[prefix + 'loss_spread']):.3e}")
        worst, gmax = 0.0, max(float(g.abs().max()) for g in g64.values())
        for k, g in g64.items():
            if float(g.abs().max()) == 0.0:
                assert float(g64m[k].abs().max()) == 0.0 and float(g32[k].abs().max()) == 0.0, k
            elif float(g.abs().max()) < 1e-9 * gmax:
                # mathematically zero (the key bias: a softmax row does not see a shift of its scores); both backward
                # passes leave rounding residue there, and the recorded spread of such a tensor is of order 1 or more
                print(f"{k}: max |g| {float(g.abs().max()):.3e} is rounding residue")
            else:
                worst = max(worst, A.rel_err(g64m[k], g))
            name = f"{prefix}grad.{k}"
            out[name + "_spread"] = np.float64(R.spread(g32[k], g) if float(g.abs().max()) else 0.0)
            if g.numel() > T.BIG and (prefix or k not in FULL):
                out[name + "_sample"] = g.flatten()[T.sample_index(g.numel())].numpy()
                out[name + "_norm"] = np.float64(g.norm().item())
                out[name + "_max"] = np.float64(g.abs().max().item())
            else:
                out[name] = g.numpy()
        print(f"{prefix}: the reference module's fp64 backward against the restatement: {worst:.3e}")
        assert worst < 2e-7, worst
        sp = [float(out[f"{prefix}grad.{k}_spread"]) for k in g64]
        print(f"{prefix}spreads: min {min(sp):.3e} median {sorted(sp)[len(sp) // 2]:.3e} max {max(sp):.3e}")
    path = os.path.join(HERE, "g20_aekl_train.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    if size > 1_000_000:
        raise SystemExit(f"{path}: {size} bytes exceeds the 1 000 000 byte limit for a committed fixture")


if __name__ == "__main__":
    main(sys.argv)
