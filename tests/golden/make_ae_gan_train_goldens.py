"""Generate tests/golden/g22_ae_gan_train.npz from the reference's own classes (CPU): one training-mode forward and
backward of ConvAutoencoderBIG, and five optimiser steps on one batch.

    python tests/golden/make_ae_gan_train_goldens.py <reference checkout root>

The classes are taken out of the reference's experiments/v1_experiments/ae_gan/train.py with `ast` at run time, as
make_ae_gan_goldens.py does; nothing is copied, the fixture holds recorded results only.

Recipe:
  1. torch.manual_seed(1234); ConvAutoencoderBIG(); G21's calibrated state (tests/ae_gan_ref.py `golden_state` on
     g21_ae_gan.npz); train().
  2. (x, G) = tests/ae_gan_train_ref.py `golden_batch()`: x = rand(8, 1, 128, 128), G = randn of the same shape.  B = 8 is
     the experiment's batch: at B = 2 the BatchNorms of the 1x1 planes see two values and the gradient is degenerate.
  3. loss = mean(recon * G): smooth, so no L1 near-tie sign differs between fp32 and fp64.  backward().
Stored, each as the fp64 run rounded to fp32 with `<name>_spread` = max|a32 - a64| / max|a64| between the reference's own
fp32 and fp64 runs: `loss`; `z`, `recon` (sample + norm above 4096 elements); per parameter, in state_dict order,
`grad_norm` (fp64 L2 norms), `grad_max` (max |g|, what a spread is relative to), `grad_samples` (256 elements at
`ae_gan_train_ref.grad_index`, or all of a smaller one, concatenated; `grad_offsets`), `grad_spread`; the updated
`running_mean` / `running_var` of all BatchNorms concatenated (sample + norm).
  4. The step: from the same state, STEPS = 5 times on x: loss = l1_loss(recon, x); backward; clip_grad_norm_(1.0);
     torch.optim.AdamW(lr 1e-3, weight_decay 1e-5) under SequentialLR(LinearLR(0.1, 1 step), CosineAnnealingLR(9 steps,
     eta_min 1e-4)) — the shipped config at trainer.total_train_steps = 10.  Stored: `step_loss` (fp64), `step_loss_spread`
     per step, `step_grad_norm` of step 1 before clipping and its spread.
The script refuses a fixture in which any recorded spread exceeds 1e-3: the state is then too ill-conditioned to test
against, and another seed should be tried.
"""
from __future__ import annotations

import copy
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from tests import ae_gan_ref as R  # noqa: E402
from tests import ae_gan_train_ref as T  # noqa: E402
from make_ae_gan_goldens import load_classes, put  # noqa: E402

LIMIT = 1e-3
TOTAL = 10       # trainer.total_train_steps of the step test


def grads_of(model, x, G):
    model.zero_grad(set_to_none=True)
    recon, z = model(x)
    loss = (recon * G).mean()
    loss.backward()
    return loss.detach(), z.detach(), recon.detach()


def bn_cat(model, name):
    sd = model.state_dict()
    return torch.cat([sd[f"{p}.{name}"] for p in R.bn_prefixes(list(sd))])


def steps_of(model, x):
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-5)
    warm = torch.optim.lr_scheduler.LinearLR(opt, start_factor=0.1, total_iters=1)
    cos = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=TOTAL - 1, eta_min=1e-4)
    sch = torch.optim.lr_scheduler.SequentialLR(opt, [warm, cos], milestones=[1])
    losses, norms = [], []
    for _ in range(T.STEPS):
        loss = F.l1_loss(model(x)[0], x)
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)))
        opt.step()
        sch.step()
        opt.zero_grad(set_to_none=True)
        losses.append(float(loss))
    return losses, norms


def main(argv):
    root = argv[1] if len(argv) > 1 else os.environ.get("WFAE_REFERENCE_ROOT")
    if not root:
        raise SystemExit(__doc__)
    ns = load_classes(root)
    g21 = np.load(os.path.join(HERE, "g21_ae_gan.npz"))
    torch.manual_seed(R.SEED)
    m32 = ns["ConvAutoencoderBIG"]()
    m32.load_state_dict(R.golden_state(m32, g21))
    m32.train()
    m64 = copy.deepcopy(m32).double()
    s32, s64 = copy.deepcopy(m32), copy.deepcopy(m64)      # the step test starts from the same state
    x, G = T.golden_batch()

    out, worst = {}, {}
    l32, z32, r32 = grads_of(m32, x, G)
    l64, z64, r64 = grads_of(m64, x.double(), G.double())
    out["loss"] = np.float64(l64)
    out["loss_spread"] = np.float64(abs(float(l32) - float(l64)) / abs(float(l64)))
    put(out, "z", z32, z64)
    put(out, "recon", r32, r64)
    norms, maxes, samples, offsets, spreads, off = [], [], [], [0], [], 0
    for (k, p32), (_, p64) in zip(m32.named_parameters(), m64.named_parameters()):
        g64 = p64.grad.flatten()
        idx = T.grad_index(g64.numel())
        norms.append(float(g64.norm()))
        maxes.append(float(g64.abs().max()))
        samples.append(g64[idx].float().numpy())
        spreads.append(R.spread(p32.grad, p64.grad))
        off += idx.numel()
        offsets.append(off)
        if spreads[-1] > 1e-4:
            print(f"grad {k}: spread {spreads[-1]:.2e}, norm {norms[-1]:.3e}")
    out["grad_keys"] = np.array([k for k, _ in m64.named_parameters()])
    out["grad_norm"], out["grad_max"], out["grad_spread"] = np.array(norms), np.array(maxes), np.array(spreads)
    out["grad_samples"], out["grad_offsets"] = np.concatenate(samples), np.array(offsets, dtype=np.int64)
    for name in ("running_mean", "running_var"):
        put(out, name, bn_cat(m32, name), bn_cat(m64, name))
    worst.update({"loss": out["loss_spread"], "z": out["z_spread"], "recon": out["recon_spread"], "grad": max(spreads),
                  "running_mean": out["running_mean_spread"], "running_var": out["running_var_spread"]})

    sl32, sn32 = steps_of(s32, x)
    sl64, sn64 = steps_of(s64, x.double())
    out["step_loss"] = np.array(sl64)
    out["step_loss_spread"] = np.array([abs(a - b) / abs(b) for a, b in zip(sl32, sl64)])
    out["step_grad_norm"] = np.float64(sn64[0])
    out["step_grad_norm_spread"] = np.float64(abs(sn32[0] - sn64[0]) / abs(sn64[0]))
    worst.update({"step_loss": float(out["step_loss_spread"].max()), "step_grad_norm": out["step_grad_norm_spread"]})
    print("loss", float(l64), "step losses", sl64, "fp32", sl32, "grad norm", sn64[0])
    for k, v in worst.items():
        print(f"spread {k}: {float(v):.3e}")
    bad = {k: float(v) for k, v in worst.items() if float(v) > LIMIT}
    if bad:
        raise SystemExit(f"spreads above {LIMIT}: {bad}: the state is too ill-conditioned to test against; try another seed")
    path = os.path.join(HERE, "g22_ae_gan_train.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    if size > 1_000_000:
        raise SystemExit(f"{path}: {size} bytes exceeds the 1 000 000 byte limit for a committed fixture")


if __name__ == "__main__":
    main(sys.argv)
