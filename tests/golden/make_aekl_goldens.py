"""Generate tests/golden/g14_aekl.npz from the reference's own AutoencoderKL (CPU).

    python tests/golden/make_aekl_goldens.py <reference checkout root>

The reference package pipeline.models.autoencoderkl imports with torch alone.  Nothing from the reference is copied; the
fixture holds inputs and recorded results only, in the conventions of g13_convae.npz.

Three cases, names prefixed `a_`, `b_`, `c_` (configurations: tests/aekl_ref.py CONFIGS):
  a  "small": block_out_channels [32, 64, 64], 4 latent channels, 2 x 1 x 64 x 64 frames (256 attention tokens); every
     tensor stored in full
  b  "ref64": the reference configuration with 64 latent channels, 1 x 1 x 128 x 128
  c  "ref4":  the reference configuration with 4 latent channels, 1 x 1 x 384 x 384 (2304 attention tokens)
Weights: torch.manual_seed(SEED); AutoencoderKL(**config).  They are not stored — `<p>_keys`, `<p>_shapes`, `<p>_keys_sha`,
`<p>_init_sha` (fp32 bytes of the seeded initial state dict) and `<p>_nparams` pin them.  Frames: torch.rand from
Generator().manual_seed(`<p>_x_seed`), stored as `<p>_x` for a and b and pinned by `<p>_x_sha` (sha256 of the fp32 bytes)
for c.  `<p>_noise` = torch.randn(latent shape) from Generator().manual_seed(`<p>_noise_seed`): the draw the reference's
`posterior.sample(generator)` makes.
Recorded per case: `mean`, `logvar`, `mode`, `draw` (sample(): mean + std * noise) and `decode` (decode(mode)).  Every result is
computed by the fp32 model and by an fp64 copy of it; the fp64 value rounded to fp32 is stored, with `<name>_spread` =
max|a32 - a64| / max|a64| over the whole tensor.  For b and c tensors of more than 4096 elements are stored as
`<name>_sample` (2048 elements at arange(2048) * (numel // 2048)) and `<name>_norm` (fp64 L2 norm).
"""
from __future__ import annotations

import copy
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import aekl_ref as A  # noqa: E402
from tests import convae_ref as R  # noqa: E402

SEED = 1234
CASES = [("a", "small", (2, 1, 64, 64), True), ("b", "ref64", (1, 1, 128, 128), False), ("c", "ref4", (1, 1, 384, 384), False)]


def x_digest(x):
    return hashlib.sha256(x.detach().to(torch.float32).contiguous().numpy().tobytes()).hexdigest()


def put(out, name, a32, a64, full):
    out[f"{name}_spread"] = np.float64(R.spread(a32, a64))
    a64 = a64.detach().double()
    if a64.numel() > R.BIG and not full:
        out[f"{name}_sample"] = a64.flatten()[R.sample_index(a64.numel())].float().numpy()
        out[f"{name}_norm"] = np.float64(a64.norm().item())
    else:
        out[name] = a64.float().numpy()
    print(f"{name}: spread {float(out[f'{name}_spread']):.3e}")


def main(argv):
    root = argv[1] if len(argv) > 1 else os.environ.get("WFAE_REFERENCE_ROOT")
    if not root:
        raise SystemExit(__doc__)
    sys.path.insert(0, root)
    from pipeline.models.autoencoderkl.autoencoder_kl import AutoencoderKL
    out = {"seed": np.int64(SEED)}
    for i, (p, name, shape, full) in enumerate(CASES):
        cfg = A.CONFIGS[name]
        torch.manual_seed(SEED)
        m32 = AutoencoderKL(**cfg).eval()
        m64 = copy.deepcopy(m32).double()
        sd0 = {k: v.detach().clone() for k, v in m32.state_dict().items()}
        items = [(k, tuple(v.shape)) for k, v in sd0.items()]
        out[f"{p}_config"] = np.array(name)
        out[f"{p}_keys"] = np.array([k for k, _ in items])
        out[f"{p}_shapes"] = np.array([" ".join(str(d) for d in s) for _, s in items])
        out[f"{p}_keys_sha"] = np.array(R.keys_digest(items))
        out[f"{p}_init_sha"] = np.array(R.values_digest(sd0))
        out[f"{p}_nparams"] = np.int64(sum(v.numel() for v in sd0.values()))
        print(p, name, len(items), "entries", int(out[f"{p}_nparams"]), "parameters")
        xs, ns = 3000 + i, 4000 + i
        x = torch.rand(*shape, generator=torch.Generator().manual_seed(xs))
        out[f"{p}_x_seed"], out[f"{p}_noise_seed"] = np.int64(xs), np.int64(ns)
        out[f"{p}_x_shape"] = np.array(shape, dtype=np.int64)
        out[f"{p}_x_sha"] = np.array(x_digest(x))
        if p != "c":
            out[f"{p}_x"] = x.numpy()
        with torch.no_grad():
            p32, p64 = m32.encode(x), m64.encode(x.double())
            noise = torch.randn(p32.mean.shape, generator=torch.Generator().manual_seed(ns))
            s32 = p32.sample(generator=torch.Generator().manual_seed(ns))
            assert torch.equal(s32, p32.mean + p32.std * noise), "the stored noise is not the reference's draw"
            s64 = p64.mean + p64.std * noise.double()
            d32, d64 = m32.decode(p32.mode()), m64.decode(p64.mode())
            # the restatement must be the same function: fp64 against fp64.  Not to fp64 rounding: the reference's
            # attention casts its scores to fp32 for the softmax whatever the model's dtype, which leaves about 1e-8
            sd64 = A.cast(sd0, torch.float64)
            e = A.encode(sd64, x.double(), cfg, noise.double())
            assert A.rel_err(e["mean"], p64.mean) < 2e-7 and A.rel_err(e["logvar"], p64.logvar) < 2e-7
            assert A.rel_err(A.decode(sd64, p64.mode(), cfg), d64) < 2e-7
        out[f"{p}_noise"] = noise.numpy()
        put(out, f"{p}_mean", p32.mean, p64.mean, full)
        put(out, f"{p}_logvar", p32.logvar, p64.logvar, full)
        put(out, f"{p}_mode", p32.mode(), p64.mode(), full)
        put(out, f"{p}_draw", s32, s64, full)
        put(out, f"{p}_decode", d32, d64, full)
    path = os.path.join(HERE, "g14_aekl.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    if size > 1_000_000:
        raise SystemExit(f"{path}: {size} bytes exceeds the 1 000 000 byte limit for a committed fixture")


if __name__ == "__main__":
    main(sys.argv)
