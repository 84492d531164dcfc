"""Generate tests/golden/g17_conv_disc.npz from the reference's own classes (CPU).

    python tests/golden/make_conv_disc_goldens.py <reference checkout root>

The reference's experiments/v1_experiments/pretrained_ae_conv_disc/train.py imports pytorch_lightning, omegaconf and wandb
at module level, so it is not imported: the `Encoder`, `Decoder` and `ConvModel` class definitions are taken out of the
file with `ast` at run time and executed against torch.  `NLayerDiscriminator` and `weights_init` come from the reference's
importable pipeline/models/autoencoderkl/losses/model.py.  The reference's `Loss` is never instantiated (its constructor
fetches LPIPS weights from the network): its arithmetic (:52-100) is restated in `nll` / `gan_step` below.  Nothing from the
reference is copied; the fixture holds inputs and recorded results only.

Weights: torch.manual_seed(1234); ConvModel(); then NLayerDiscriminator(input_nc=64, n_layers=3).apply(weights_init).
The predictor's are not stored — `keys`, `shapes`, `keys_sha`, `init_sha` and `nparams` pin them, and `disc_init_sha` the
discriminator's.  Input: x = randn(2, 64, 16, 16) from Generator().manual_seed(S), S the first seed from 2000 up whose L1
margin holds: `l1_min_abs` = min |recon - x| of the fp64 run >= 4 `l1_diff`, the largest fp32-vs-fp64 absolute difference
of recon (the L1 derivative jumps at recon = x).  Every result is computed twice, by the fp32 model and by an fp64 copy of
it; the fp64 value rounded to fp32 is stored as the expected value, and per tensor `<name>_spread` =
max|a32 - a64| / max|a64|.  Names: `z`, `rec`, `loss` (the pre-disc_start loss, logvar 0), `grad_<key>`, `post_<key>`
(parameters after 3 steps of torch.optim.AdamW(lr 1e-3, weight_decay 1e-2) with clip_grad_norm_(1.0)).  From disc_start:
`g_loss`, `d_weight`, `gen_loss`, `gen_gradnorm` (L2 norm over all 24 gradients of the generator loss),
`gen_grad_<key>_norm`, `d_loss`, `disc_gradnorm`, `disc_grad_<key>_norm` — the discriminator's LeakyReLU and hinge kinks
are not margin-checked, so these gradients are recorded and compared by norm only.  Tensors of more than 4096 elements are
stored as `<name>_sample` (the 2048 elements at arange(2048) * (numel // 2048) of the flattened tensor) and `<name>_norm`
(fp64 L2 norm).
"""
from __future__ import annotations

import ast
import copy
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import conv_disc_ref as R  # noqa: E402

SEED = 1234
CLASSES = ["Encoder", "Decoder", "ConvModel"]


def load_classes(root):
    path = os.path.join(root, "experiments", "v1_experiments", "pretrained_ae_conv_disc", "train.py")
    tree = ast.parse(open(path).read(), path)
    keep = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in CLASSES]
    assert [n.name for n in keep] == CLASSES, path
    ns = {"torch": torch, "nn": nn, "F": F}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    spec = importlib.util.spec_from_file_location(
        "_ref_disc_model", os.path.join(root, "pipeline", "models", "autoencoderkl", "losses", "model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ns["NLayerDiscriminator"], ns["weights_init"] = mod.NLayerDiscriminator, mod.weights_init
    return ns


def put(out, name, a32, a64):
    out[f"{name}_spread"] = np.float64(R.spread(a32, a64))
    a64 = a64.detach().double()
    if a64.numel() > R.BIG:
        out[f"{name}_sample"] = a64.flatten()[R.sample_index(a64.numel())].float().numpy()
        out[f"{name}_norm"] = np.float64(a64.norm().item())
    else:
        out[name] = a64.float().numpy()


def put_scalar(out, name, a32, a64):
    a32, a64 = float(a32), float(a64)
    out[name] = np.float64(a64)
    out[f"{name}_spread"] = np.float64(abs(a32 - a64) / max(abs(a64), 1e-300))


def nll(recon, x, logvar=0.0):
    """Loss.forward :54,62-63 with perceptual_weight 0"""
    rec = F.l1_loss(recon, x, reduction="mean")
    lv = torch.as_tensor(logvar, dtype=recon.dtype)
    return torch.sum(rec / torch.exp(lv) + lv) / x.size(0)


def gan_step(model, disc, x):
    """Loss.forward :74-100 from disc_start on, disc_weight 1 -> scalars and gradient dicts"""
    _, recon = model(x)
    n = nll(recon, x)
    g_loss = -torch.mean(disc(recon))
    last = model.decoder.conv_out.weight
    ng = torch.autograd.grad(n, last, retain_graph=True)[0]
    gg = torch.autograd.grad(g_loss, last, retain_graph=True)[0]
    d_weight = torch.clamp(torch.norm(ng) / (torch.norm(gg) + 1e-4), 0.0, 1e4).detach()
    loss = n + d_weight * g_loss
    names = [k for k, _ in model.named_parameters()]
    g_grads = dict(zip(names, torch.autograd.grad(loss, list(model.parameters()))))
    real, fake = disc(x.detach()), disc(recon.detach())
    d_loss = 0.5 * (torch.mean(F.relu(1.0 - real)) + torch.mean(F.relu(1.0 + fake)))
    dnames = [k for k, _ in disc.named_parameters()]
    d_grads = dict(zip(dnames, torch.autograd.grad(d_loss, list(disc.parameters()))))
    return {"g_loss": g_loss.detach(), "d_weight": d_weight, "gen_loss": loss.detach(), "d_loss": d_loss.detach()}, \
        g_grads, d_grads


def main(argv):
    root = argv[1] if len(argv) > 1 else os.environ.get("WFAE_REFERENCE_ROOT")
    if not root:
        raise SystemExit(__doc__)
    ns = load_classes(root)
    torch.manual_seed(SEED)
    m32 = ns["ConvModel"]()
    d32 = ns["NLayerDiscriminator"](input_nc=64, n_layers=3).apply(ns["weights_init"])
    m64, d64 = copy.deepcopy(m32).double(), copy.deepcopy(d32).double()
    sd0 = {k: v.detach().clone() for k, v in m32.state_dict().items()}
    items = [(k, tuple(v.shape)) for k, v in sd0.items()]
    assert items == R.key_list(), "tests/conv_disc_ref.py key_list() does not match the reference"
    out = {"seed": np.int64(SEED), "keys": np.array([k for k, _ in items]),
           "shapes": np.array([" ".join(str(d) for d in s) for _, s in items]),
           "keys_sha": np.array(R.keys_digest(items)), "init_sha": np.array(R.values_digest(sd0)),
           "nparams": np.int64(sum(v.numel() for v in sd0.values())),
           "disc_keys": np.array(list(d32.state_dict())),
           "disc_init_sha": np.array(R.values_digest({k: v for k, v in d32.state_dict().items() if v.is_floating_point()}))}

    for S in range(2000, 2032):
        x = torch.randn(2, 64, 16, 16, generator=torch.Generator().manual_seed(S))
        z32, r32 = m32(x)
        z64, r64 = m64(x.double())
        amin, diff = R.l1_margin(r64.detach(), r32.detach(), x)
        print(f"input seed {S}: min |recon - x| = {amin:.3e}, fp32-vs-fp64 difference of recon = {diff:.3e}")
        if amin >= 4 * diff:
            break
    else:
        raise SystemExit("no input seed in 2000..2031 keeps recon - x clear of the L1 kink")
    out["input_seed"], out["x"] = np.int64(S), x.numpy()
    out["l1_min_abs"], out["l1_diff"] = np.float64(amin), np.float64(diff)
    l32, l64 = nll(r32, x), nll(r64, x.double())
    l32.backward()
    l64.backward()
    put(out, "z", z32.detach(), z64.detach())
    put(out, "rec", r32.detach(), r64.detach())
    put(out, "loss", l32.detach(), l64.detach())
    g32 = dict(m32.named_parameters())
    for k, p in m64.named_parameters():
        put(out, f"grad_{k}", g32[k].grad, p.grad)
    m32.zero_grad(set_to_none=True)
    m64.zero_grad(set_to_none=True)

    # from disc_start on, on the initial weights (BatchNorm in training mode: batch statistics)
    s32, gg32, dg32 = gan_step(m32, d32.train(), x)
    s64, gg64, dg64 = gan_step(m64, d64.train(), x.double())
    for k in s64:
        put_scalar(out, k, s32[k], s64[k])
    put_scalar(out, "gen_gradnorm", R.grad_norm(gg32), R.grad_norm(gg64))
    put_scalar(out, "disc_gradnorm", R.grad_norm(dg32), R.grad_norm(dg64))
    for k in gg64:
        put_scalar(out, f"gen_grad_{k}_norm", gg32[k].double().norm(), gg64[k].norm())
    for k in dg64:
        put_scalar(out, f"disc_grad_{k}_norm", dg32[k].double().norm(), dg64[k].norm())

    for model, inp in ((m32, x), (m64, x.double())):
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-2)
        model.zero_grad(set_to_none=True)
        for _ in range(3):
            _, recon = model(inp)
            nll(recon, inp).backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
            opt.step()
            opt.zero_grad(set_to_none=True)
    p32 = dict(m32.named_parameters())
    for k, p in m64.named_parameters():
        put(out, f"post_{k}", p32[k].detach(), p.detach())
    path = os.path.join(HERE, "g17_conv_disc.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    if size > 1_000_000:
        raise SystemExit(f"{path}: {size} bytes exceeds the 1 000 000 byte limit for a committed fixture")


if __name__ == "__main__":
    main(sys.argv)
