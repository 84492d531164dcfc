"""Generate tests/golden/g18_convattn.npz from the reference's own class (CPU).

    python tests/golden/make_convattn_goldens.py <reference checkout root>

The reference's experiments/v1_experiments/pretrained_ae_convattn_ae_sevir/train.py imports pytorch_lightning, omegaconf
and wandb at module level, so it is not imported: the `ConvAttnModel` class definition is taken out of the file with `ast`
at run time and executed against torch.  Nothing from the reference is copied; the fixture holds inputs and recorded results
only.

Weights: torch.manual_seed(1234); ConvAttnModel().  They are not stored — `keys`, `shapes`, `keys_sha`, `init_sha` and
`nparams` pin them.  Input: x = randn(2, 4, 48, 48) from Generator().manual_seed(2000).  The model is in EVAL mode (no
dropout).  Every result is computed twice, by the fp32 model and by an fp64 copy of it; the fp64 value rounded to fp32 is
stored as the expected value, and per item `<name>_spread` = max|a32 - a64| / max|a64|.  Names: `z`, `rec`, `loss`
(nn.HuberLoss between rec and x), `gradnorm` (L2 norm over the live gradients), `grad_<key>`, `post_<key>` (parameters after 3
steps of torch.optim.AdamW(lr 1e-3, weight_decay 1e-2) with clip_grad_norm_(1.0)).

DEAD parameters (`dead_keys`, `dead_lo`, `dead_hi`; -1: the whole tensor, else rows lo:hi), tests/convattn_ref.py
dead_list(): (a) the decoder's cross-attention has one key, so its softmax is identically 1 and norm2 and the q / k rows of
multihead_attn.in_proj_{weight,bias} cannot reach the output; (b) the key bias of every softmax attention shifts all scores of
a row alike and cancels (rows E:2E of every in_proj_bias).  Torch returns rounding noise for their gradients
(`dead_grad_max_32`, `dead_grad_max_64`: the largest magnitude seen, next to `live_grad_max`), which AdamW normalises into a
random walk of +-lr per step, so nothing of them is recorded but their names: the product gives them exact zeros, and
their "post" values are the initial ones times (1 - lr wd)^3.  The recorded steps zero those gradients before clipping
(their share of the norm is below 1e-16), so that the fixture holds that trajectory.  For a tensor with a dead slice, `grad_` /
`post_` hold the live rows only, those below the slice first.

Tensors of more than 128 elements are stored as `<name>_sample` (the 128 elements at arange(128) * step of the flattened
tensor, step the largest integer <= numel // 128 coprime with numel: tests/convattn_ref.py g18_index(), which therefore visits
many columns of a weight matrix and many taps of a kernel), `<name>_norm` (fp64 L2 norm) and `<name>_amax` (max |a64| over the WHOLE tensor: the denominator of the
spread, so that an error on the sample is measured in the spread's own unit).
"""
from __future__ import annotations

import ast
import copy
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import convattn_ref as R  # noqa: E402

SEED, INPUT_SEED, LR, WD, STEPS = 1234, 2000, 1e-3, 1e-2, 3


def load_class(root):
    path = os.path.join(root, "experiments", "v1_experiments", "pretrained_ae_convattn_ae_sevir", "train.py")
    tree = ast.parse(open(path).read(), path)
    keep = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "ConvAttnModel"]
    assert len(keep) == 1, path
    ns = {"torch": torch, "nn": nn, "F": F}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns["ConvAttnModel"]


def put(out, name, a32, a64):
    out[f"{name}_spread"] = np.float64(R.spread(a32, a64))
    a64 = a64.detach().double()
    if a64.numel() > R.G18_SAMPLE:
        out[f"{name}_sample"] = a64.flatten()[R.g18_index(a64.numel())].float().numpy()
        out[f"{name}_norm"] = np.float64(a64.norm().item())
        out[f"{name}_amax"] = np.float64(a64.abs().max().item())
    else:
        out[name] = a64.float().numpy()


def put_scalar(out, name, a32, a64):
    a32, a64 = float(a32), float(a64)
    out[name] = np.float64(a64)
    out[f"{name}_spread"] = np.float64(abs(a32 - a64) / max(abs(a64), 1e-300))


def main(argv):
    root = argv[1] if len(argv) > 1 else os.environ.get("WFAE_REFERENCE_ROOT")
    if not root:
        raise SystemExit(__doc__)
    cls = load_class(root)
    torch.manual_seed(SEED)
    m32 = cls().eval()
    m64 = copy.deepcopy(m32).double().eval()
    sd0 = {k: v.detach().clone() for k, v in m32.state_dict().items()}
    items = [(k, tuple(v.shape)) for k, v in sd0.items()]
    assert items == R.key_list(), "tests/convattn_ref.py key_list() does not match the reference"
    dead = R.dead_list()
    out = {"seed": np.int64(SEED), "input_seed": np.int64(INPUT_SEED), "keys": np.array([k for k, _ in items]),
           "shapes": np.array([" ".join(str(d) for d in s) for _, s in items]),
           "keys_sha": np.array(R.keys_digest(items)), "init_sha": np.array(R.values_digest(sd0)),
           "nparams": np.int64(sum(v.numel() for v in sd0.values())),
           "dead_keys": np.array([k for k, _, _ in dead]), "dead_lo": np.array([lo for _, lo, _ in dead], dtype=np.int64),
           "dead_hi": np.array([hi for _, _, hi in dead], dtype=np.int64),
           "lr": np.float64(LR), "wd": np.float64(WD), "steps": np.int64(STEPS)}
    x = torch.randn(2, 4, 48, 48, generator=torch.Generator().manual_seed(INPUT_SEED))
    out["x"] = x.numpy()

    z32, r32 = m32(x)
    z64, r64 = m64(x.double())
    l32, l64 = F.huber_loss(r32, x), F.huber_loss(r64, x.double())
    l32.backward()
    l64.backward()
    put(out, "z", z32.detach(), z64.detach())
    put(out, "rec", r32.detach(), r64.detach())
    put_scalar(out, "loss", l32.detach(), l64.detach())
    out["huber_quadratic_fraction"] = np.float64(((r64.detach() - x.double()).abs() <= 1.0).double().mean().item())
    g32 = {k: p.grad for k, p in m32.named_parameters()}
    g64 = {k: p.grad for k, p in m64.named_parameters()}
    live32, live64, dmax32, dmax64, lmax = {}, {}, 0.0, 0.0, 0.0
    for k in g64:
        d32, d64 = R.dead_part(k, g32[k], dead), R.dead_part(k, g64[k], dead)
        if d64 is not None:
            dmax32, dmax64 = max(dmax32, float(d32.abs().max())), max(dmax64, float(d64.abs().max()))
        a32, a64 = R.live_part(k, g32[k], dead), R.live_part(k, g64[k], dead)
        if a64 is None:
            continue
        live32[k], live64[k] = a32, a64
        lmax = max(lmax, float(a64.abs().max()))
        put(out, f"grad_{k}", a32, a64)
    put_scalar(out, "gradnorm", R.grad_norm(live32), R.grad_norm(live64))
    out["dead_grad_max_32"], out["dead_grad_max_64"], out["live_grad_max"] = np.float64(dmax32), np.float64(dmax64), np.float64(lmax)
    print(f"loss {float(l64.detach()):.6f}  gradnorm {float(out['gradnorm']):.4f}  dead |grad| max fp32 {dmax32:.2e} fp64 {dmax64:.2e}"
          f"  live max {lmax:.2e}")

    for model, inp in ((m32, x), (m64, x.double())):
        opt = torch.optim.AdamW(model.parameters(), lr=LR, weight_decay=WD)
        model.zero_grad(set_to_none=True)
        prm = dict(model.named_parameters())
        for _ in range(STEPS):
            _, recon = model(inp)
            F.huber_loss(recon, inp).backward()
            for k, lo, hi in dead:
                (prm[k].grad if lo < 0 else prm[k].grad[lo:hi]).zero_()
            torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
            opt.step()
            opt.zero_grad(set_to_none=True)
    p32 = dict(m32.named_parameters())
    for k, p in m64.named_parameters():
        a32, a64 = R.live_part(k, p32[k].detach(), dead), R.live_part(k, p.detach(), dead)
        if a64 is not None:
            put(out, f"post_{k}", a32, a64)
        d64 = R.dead_part(k, p.detach(), dead)
        if d64 is not None:       # decay alone: the claim the product is held to
            want = R.dead_part(k, sd0[k].double(), dead) * (1.0 - LR * WD) ** STEPS
            assert float((d64 - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1.0), k
    worst = sorted(((float(out[n]), n) for n in out if n.endswith("_spread")), reverse=True)[:6]
    print("largest spreads:", ", ".join(f"{n} {v:.2e}" for v, n in worst))
    path = os.path.join(HERE, "g18_convattn.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    if size > 1_000_000:
        raise SystemExit(f"{path}: {size} bytes exceeds the 1 000 000 byte limit for a committed fixture")


if __name__ == "__main__":
    main(sys.argv)
