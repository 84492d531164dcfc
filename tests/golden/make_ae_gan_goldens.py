"""Generate tests/golden/g21_ae_gan.npz from the reference's own classes (CPU).

    python tests/golden/make_ae_gan_goldens.py <reference checkout root>

The reference's experiments/v1_experiments/ae_gan/train.py imports pytorch_lightning, omegaconf and wandb at module level,
so it is not imported: the `ResidualBlock`, `UpsampleBlock`, `ConvAutoencoder` and `ConvAutoencoderBIG` class definitions
are taken out of the file with `ast` at run time and executed against torch.  Its pipeline/metrics.py is loaded by path
with a stub in place of torchmetrics (SSIM / PSNR are then NaN and are not recorded as values).  Nothing from the reference
is copied; the fixture holds inputs and recorded results only.

Recipe (tests/ae_gan_ref.py `golden_state` rebuilds the model from it):
  1. torch.manual_seed(1234); ConvAutoencoderBIG().
  2. every BatchNorm: gamma ~ U(0.75, 1.25), beta ~ 0.05 randn, from Generator().manual_seed(1237), in state_dict order.
  3. calibration: CALIB train-mode forward passes of the reference on rand(8, 1, 128, 128) from Generator().manual_seed(1236)
     (momentum 0.1 moves the running statistics towards the batch's).  At the raw initialisation (running_mean 0,
     running_var 1) the signal dies on the way through 14 blocks and `recon` is the bias of `final_conv`; the script
     prints each block's output scale after calibration and refuses a fixture in which one leaves [1e-2, 10].
  4. eval().
Stored: `bn_weight`, `bn_bias`, `bn_running_mean`, `bn_running_var` (the BatchNorm layers concatenated in state_dict
order; everything else is rebuilt from the seed); `keys`, `shapes`, `keys_sha`, `init_sha`, `nparams` of the seeded
ConvAutoencoderBIG and, with the suffix `_small`, of torch.manual_seed(1234); ConvAutoencoder().  For x =
rand(2, 1, 128, 128) from Generator().manual_seed(1235) (`ae_gan_ref.golden_input`): `z`, `recon`, `enc1`..`enc7`,
`dec1`..`dec7` — the fp64 run rounded to fp32, tensors above 4096 elements as `<name>_sample` (2048 elements at
arange(2048) * (numel // 2048) of the flattened tensor) + `<name>_norm` (fp64 L2 norm) — each with `<name>_spread` =
max|a32 - a64| / max|a64| between the reference's fp32 and fp64 runs; `rec_loss` = mean |recon - x| (+ spread);
`metric_keys` (the `test_` keys of log_metrics(recon.unsqueeze(2), x.unsqueeze(2))) and `metric_values` of the fp32 run.
"""
from __future__ import annotations

import ast
import copy
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import ae_gan_ref as R  # noqa: E402

CLASSES = ["ResidualBlock", "UpsampleBlock", "ConvAutoencoder", "ConvAutoencoderBIG"]
CALIB = 3


def load_classes(root):
    path = os.path.join(root, "experiments", "v1_experiments", "ae_gan", "train.py")
    tree = ast.parse(open(path).read(), path)
    keep = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in CLASSES]
    assert [n.name for n in keep] == CLASSES, path
    ns = {"torch": torch, "nn": nn, "F": F}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns


def load_metrics(root):
    tm, tmi = types.ModuleType("torchmetrics"), types.ModuleType("torchmetrics.image")
    tmi.StructuralSimilarityIndexMeasure = tmi.PeakSignalNoiseRatio = None
    tm.image = tmi
    sys.modules.setdefault("torchmetrics", tm)
    sys.modules.setdefault("torchmetrics.image", tmi)
    spec = importlib.util.spec_from_file_location("ref_metrics", os.path.join(root, "pipeline", "metrics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.ssim = mod.psnr = lambda p, t: float("nan")
    return mod


def put(out, name, a32, a64):
    out[f"{name}_spread"] = np.float64(R.spread(a32, a64))
    a64 = a64.detach().double()
    if a64.numel() > R.BIG:
        out[f"{name}_sample"] = a64.flatten()[R.sample_index(a64.numel())].float().numpy()
        out[f"{name}_norm"] = np.float64(a64.norm().item())
    else:
        out[name] = a64.float().numpy()


def describe(out, sfx, model):
    sd = model.state_dict()
    items = [(k, tuple(v.shape)) for k, v in sd.items()]
    assert items == R.key_list(big=not sfx), "tests/ae_gan_ref.py key_list() does not match the reference"
    out["keys" + sfx] = np.array([k for k, _ in items])
    out["shapes" + sfx] = np.array([" ".join(str(d) for d in s) for _, s in items])
    out["keys_sha" + sfx] = np.array(R.keys_digest(items))
    out["init_sha" + sfx] = np.array(R.values_digest(sd))
    out["nparams" + sfx] = np.int64(sum(p.numel() for p in model.parameters()))


def stages_of(model, x):
    """the reference module's own forward, with every block's output recorded by hooks"""
    st, hooks = {}, []
    for name in [f"enc{i}" for i in range(1, 8)] + [f"dec{i}" for i in range(1, 8)]:
        hooks.append(getattr(model, name).register_forward_hook(lambda m, i, o, name=name: st.__setitem__(name, o.detach())))
    with torch.no_grad():
        recon, z = model(x)
    for h in hooks:
        h.remove()
    return recon, z, st


def main(argv):
    root = argv[1] if len(argv) > 1 else os.environ.get("WFAE_REFERENCE_ROOT")
    if not root:
        raise SystemExit(__doc__)
    ns = load_classes(root)
    out = {"seed": np.int64(R.SEED), "calib": np.int64(CALIB)}
    torch.manual_seed(R.SEED)
    describe(out, "_small", ns["ConvAutoencoder"]())
    torch.manual_seed(R.SEED)
    m32 = ns["ConvAutoencoderBIG"]()
    describe(out, "", m32)

    g = torch.Generator().manual_seed(R.SEED + 3)
    bns = [m for m in m32.modules() if isinstance(m, nn.BatchNorm2d)]
    with torch.no_grad():
        for bn in bns:
            bn.weight.copy_(0.75 + 0.5 * torch.rand(bn.num_features, generator=g))
            bn.bias.copy_(0.05 * torch.randn(bn.num_features, generator=g))
    xc = torch.rand(8, 1, 128, 128, generator=torch.Generator().manual_seed(R.SEED + 2))
    m32.train()
    with torch.no_grad():
        for _ in range(CALIB):
            m32(xc)
    m32.eval()
    sd = m32.state_dict()
    for name in ("weight", "bias", "running_mean", "running_var"):
        out["bn_" + name] = torch.cat([sd[f"{p}.{name}"] for p in R.bn_prefixes(list(sd))]).numpy()
    assert out["bn_weight"].shape == (24416,)

    x = R.golden_input()
    m64 = copy.deepcopy(m32).double()
    r32, z32, s32 = stages_of(m32, x)
    r64, z64, s64 = stages_of(m64, x.double())
    # the restatement of tests/ae_gan_ref.py computes what the reference module computes
    rr, zr = R.forward(R.cast(sd, torch.float64), x.double())
    assert R.spread(rr, r64) < 1e-12 and R.spread(zr, z64) < 1e-12
    for name in s64:
        scale = float(s64[name].abs().max())
        print(f"{name}: max |out| = {scale:.3e}, spread {R.spread(s32[name], s64[name]):.2e}")
        if not 1e-2 <= scale <= 10:
            raise SystemExit(f"{name}: output scale {scale:.3e} outside [1e-2, 10]: the calibration does not hold")
        put(out, name, s32[name], s64[name])
    put(out, "z", z32, z64)
    put(out, "recon", r32, r64)
    print(f"z spread {out['z_spread']:.2e}, recon spread {out['recon_spread']:.2e}, max |recon| = {float(r64.abs().max()):.3e}, "
          f"final_conv.bias = {float(sd['final_conv.bias']):.3e}")
    l32, l64 = F.l1_loss(r32, x), F.l1_loss(r64, x.double())
    out["rec_loss"] = np.float64(l64)
    out["rec_loss_spread"] = np.float64(abs(float(l32) - float(l64)) / abs(float(l64)))
    metrics = load_metrics(root).calc_metrics(r32.unsqueeze(2), x.unsqueeze(2))
    out["metric_keys"] = np.array(["test_" + k for k in metrics])
    out["metric_values"] = np.array([float(v) for v in metrics.values()], dtype=np.float64)
    path = os.path.join(HERE, "g21_ae_gan.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    if size > 1_000_000:
        raise SystemExit(f"{path}: {size} bytes exceeds the 1 000 000 byte limit for a committed fixture")


if __name__ == "__main__":
    main(sys.argv)
