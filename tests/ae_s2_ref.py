"""Torch restatement of the `ae_s2` step (reference experiments/ae_s2/train.py:29-53, 154-192) on a state dict of the
AutoencoderKL (tests/aekl_ref.py) and the stacked DLinear parameters (tests/dlinear_ref.py).  It runs in the dtype / on the
device of what it is given: fp32 against the fp32 values of tests/golden/g24_ae_s2.npz on the CPU, fp64 as the yardstick
of the GPU tests.

    encode:   per frame t, z[:, t] = mean + std * noise[t]            (noise (T, B, C, h, w): draw t belongs to frame t)
    step:     inp, tgt = z[:, :L] - z[:, L-1:L], z[:, L:] - z[:, L-1:L];  pred = DLinear(inp);  loss = mse(pred, tgt)
    validate: decode(pred + z[:, L-1:L]) against decode(tgt + z[:, L-1:L]), each frame on its own
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests import aekl_ref as A
from tests import dlinear_ref as D

TIN, TOUT, K = 7, 6, 3              # dataset.input_frames / pred_frames, dlinear.kernel_size of ae_s2/config.yaml
AE_CONFIG = "small"                 # tests/aekl_ref.py CONFIGS: the smallest one tests/test_aekl_gpu.py runs
FRAME = 32                          # 4 x 8 x 8 latents: enc_in = 256
BETAS, LR, WD, CLIP = (0.8, 0.95), 1e-2, 1e-2, 1.0      # the optimiser of the recorded steps
COLUMNS = (0, 101, 255)             # latent scalars whose forecast and gradients the fixture stores


def encode(sd, frames, cfg, noise):
    """frames (B, T, 1, H, W), noise (T, B, C, h, w) -> z (B, T, C, h, w), one frame index at a time"""
    # .contiguous(): a convolution's output can be channels-last, and torch.stack would carry that order into z, where the
    # decoder's convolutions then add up in another order than on the reference's torch.cat result
    return torch.stack([A.encode(sd, frames[:, t], cfg, noise[t])["sample"] for t in range(frames.shape[1])], dim=1).contiguous()


def decode(sd, z, cfg):
    """z (B, T, C, h, w) -> frames (B, T, 1, H, W), one frame index at a time"""
    return torch.stack([A.decode(sd, z[:, t], cfg) for t in range(z.shape[1])], dim=1).contiguous()


def step(z, params, L=TIN, P=TOUT, kernel=K):
    """params = (seasonal w (M, P, L), seasonal b (M, P), trend w, trend b) -> (loss, pred (B, P, M))"""
    r = D.rows(z, 1)
    pred = D.apply(D.diff_inputs(r, L, 1), *params, kernel, True)
    return F.mse_loss(pred, D.target(r, L, P, 1)), pred


def forecast_and_target(z, pred, L=TIN):
    """the latents the reference decodes (:181-182): pred + inp_t and (tgt - inp_t) + inp_t, both (B, P, C, h, w)"""
    b, _, c, h, w = z.shape
    inp_t = z[:, L - 1:L]
    return pred.reshape(b, -1, c, h, w) + inp_t, (z[:, L:] - inp_t) + inp_t


def step_per_column(z, leaves, L=TIN, P=TOUT, kernel=K):
    """`step`'s loss on per-column leaves [seasonal (w, b) of column 0, 1, ..., then trend]: one F.linear per latent scalar,
    the order of operations of nn.Linear modules in a loop"""
    r = D.rows(z, 1)
    m = r.shape[2]
    s, t = (x.permute(0, 2, 1) for x in D.decomp(D.diff_inputs(r, L, 1), kernel))
    so, to = torch.zeros(r.shape[0], m, P, dtype=r.dtype), torch.zeros(r.shape[0], m, P, dtype=r.dtype)
    for i in range(m):
        so[:, i] = F.linear(s[:, i], leaves[2 * i], leaves[2 * i + 1])
        to[:, i] = F.linear(t[:, i], leaves[2 * m + 2 * i], leaves[2 * m + 2 * i + 1])
    return F.mse_loss((so + to).permute(0, 2, 1), D.target(r, L, P, 1))


def fit(z_of_step, params, steps, betas=BETAS, lr=LR, wd=WD, clip=CLIP):
    """`steps` steps of clip_grad_norm_(clip) + torch.optim.AdamW from `params` (the four stacked tensors of `step`);
    z_of_step(i) -> the latents of step i.  -> the losses.  The steps run on per-column leaf tensors: clip_grad_norm_ adds
    up per-tensor norms in tensor order, and an fp32 loss near 1.5 resolves 8e-8, the size of the recorded spread, so the
    tensors are cut the way a ModuleList of nn.Linear cuts them"""
    ws, bs, wt, bt = params
    leaves = [t.detach().clone().requires_grad_(True) for w, b in ((ws, bs), (wt, bt)) for i in range(w.shape[0])
              for t in (w[i], b[i])]
    opt = torch.optim.AdamW(leaves, lr=lr, weight_decay=wd, betas=betas)
    losses = []
    for i in range(steps):
        loss = step_per_column(z_of_step(i), leaves)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(leaves, clip)
        opt.step()
        opt.zero_grad(set_to_none=True)
        losses.append(float(loss.detach()))
    return losses


def spread(a32, a64):
    """max |a32 - a64| / max |a64|: the measure of the fixtures' `_spread` entries"""
    a32, a64 = torch.as_tensor(a32).double(), torch.as_tensor(a64).double()
    return float((a32 - a64).abs().max() / a64.abs().max().clamp_min(1e-300))


def flat_keys(tree, prefix=""):
    """dotted keys of a nested mapping, in file order: the key surface of a config"""
    out = []
    for k, v in tree.items():
        out.append(prefix + str(k))
        if isinstance(v, dict):
            out += flat_keys(v, prefix + str(k) + ".")
    return out
