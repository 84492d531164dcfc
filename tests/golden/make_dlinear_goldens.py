"""Generate tests/golden/g12_dlinear.npz from the reference's own DLinear classes (CPU, fp32).

    python tests/golden/make_dlinear_goldens.py <reference checkout root>

The reference train.py files import pytorch_lightning, omegaconf and wandb at module level, so they are not
imported: the `moving_avg`, `series_decomp` and `DLinear` class definitions are taken out of each file with `ast` at
run time and executed against torch.  Nothing from the reference is copied; the fixture holds inputs and recorded
results only.

Per variant `<v>` (sevir, ind, indc_indp) at a small size: `<v>_shape` (B, C, h, w), `<v>_v` the latents
(B, 25, C, h, w), the seeded initial state dict stacked per map (`<v>_init_<Map>_w` / `_b`), `<v>_pred`, `<v>_loss`,
the gradients (`<v>_grad_<Map>_w` / `_b`) and the parameters after 3 steps of torch.optim.AdamW (lr 1e-3, wd 1e-2)
with clip_grad_norm_(1.0) (`<v>_post_<Map>_w` / `_b`).  At the reference size (4 x 48 x 48 latents): `<v>_ref_nkeys`,
`<v>_ref_keys_sha` (ordered key + shape list), `<v>_ref_head` (first keys) and `<v>_ref_init_sha` (fp32 bytes of the
seeded initial state dict).
"""
from __future__ import annotations

import ast
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import dlinear_ref as R  # noqa: E402

SEED = 1234
SMALL = {"sevir": (2, 4, 5, 5), "ind": (2, 3, 4, 4), "indc_indp": (2, 4, 2, 2)}


def load_classes(root, variant):
    path = os.path.join(root, "experiments", "v1_experiments", f"pretrained_ae_dlinear_{variant}", "train.py")
    tree = ast.parse(open(path).read(), path)
    keep = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in ("moving_avg", "series_decomp", "DLinear")]
    assert [n.name for n in keep] == ["moving_avg", "series_decomp", "DLinear"], path
    ns = {"torch": torch, "nn": nn, "F": F}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns


def make(variant, root, out):
    individual, K, cf, _ = R.VARIANTS[variant]
    ns = load_classes(root, variant)
    B, C, h, w = SMALL[variant]
    M = C * h * w // cf
    cfg = types.SimpleNamespace(seq_len=R.TIN, pred_len=R.TOUT, individual=individual, enc_in=M, kernel_size=K)
    torch.manual_seed(SEED)
    model = ns["DLinear"](cfg)
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for n, (wt, bi) in R.stacked_from_state_dict(sd0, individual, M).items():
        out[f"{variant}_init_{n}_w"], out[f"{variant}_init_{n}_b"] = wt.numpy(), bi.numpy()
    g = torch.Generator().manual_seed(SEED + 1)
    v = torch.randn(B, R.TIN + R.TOUT, C, h, w, generator=g)
    out[f"{variant}_shape"] = np.array([B, C, h, w])
    out[f"{variant}_v"] = v.numpy()

    def step_loss():
        b, t, c, hh, ww = v.shape
        inp, tgt = v[:, :R.TIN], v[:, R.TIN:]
        inp_t = inp[:, -1].unsqueeze(1)
        inp, tgt = inp - inp_t, tgt - inp_t
        if cf == 1:
            pred = model(inp.reshape(b, R.TIN, c * hh * ww)).reshape(b, R.TOUT, c, hh, ww)
        else:
            pred = model(inp.reshape(b, R.TIN * c, hh * ww)).reshape(b, R.TOUT, c, hh, ww)
        return F.mse_loss(pred, tgt), pred

    loss, pred = step_loss()
    loss.backward()
    out[f"{variant}_pred"] = pred.detach().numpy()
    out[f"{variant}_loss"] = np.float32(loss.item())
    grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    for n, (wt, bi) in R.stacked_from_state_dict(grads, individual, M).items():
        if n != "Linear_Decoder":
            out[f"{variant}_grad_{n}_w"], out[f"{variant}_grad_{n}_b"] = wt.numpy(), bi.numpy()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-2)
    model.zero_grad(set_to_none=True)
    for _ in range(3):
        loss, _ = step_loss()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
        opt.step()
        opt.zero_grad(set_to_none=True)
    sd = {k: p.detach().clone() for k, p in model.state_dict().items()}
    for n, (wt, bi) in R.stacked_from_state_dict(sd, individual, M).items():
        out[f"{variant}_post_{n}_w"], out[f"{variant}_post_{n}_b"] = wt.numpy(), bi.numpy()

    # reference size: key list and seeded initial values, as digests
    C0, h0, w0 = R.REF_LATENT
    Mref = C0 * h0 * w0 // cf
    cfg = types.SimpleNamespace(seq_len=R.TIN, pred_len=R.TOUT, individual=individual, enc_in=Mref, kernel_size=K)
    torch.manual_seed(SEED)
    big = ns["DLinear"](cfg).state_dict()
    items = [(k, tuple(t.shape)) for k, t in big.items()]
    out[f"{variant}_ref_nkeys"] = np.int64(len(items))
    out[f"{variant}_ref_keys_sha"] = np.array(R.keys_digest(items))
    out[f"{variant}_ref_head"] = np.array([k for k, _ in items[:8]])
    out[f"{variant}_ref_init_sha"] = np.array(R.values_digest(big))


def main(argv):
    root = argv[1] if len(argv) > 1 else os.environ.get("WFAE_REFERENCE_ROOT")
    if not root:
        raise SystemExit(__doc__)
    out = {"seed": np.int64(SEED)}
    for variant in R.VARIANTS:
        make(variant, root, out)
    path = os.path.join(HERE, "g12_dlinear.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv)
