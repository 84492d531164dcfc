"""Torch restatement of the DLinear forecasters of the reference's v1 experiments
(experiments/v1_experiments/pretrained_ae_dlinear_{sevir,ind,indc_indp}/train.py:22-100, 151-162) on the stacked
parameter layout: weights (M, P, L) when individual, else (P, L).  Any device / dtype; used against
tests/golden/g12_dlinear.npz on the CPU and as the fp64 yardstick of the GPU tests."""
import hashlib

import torch
import torch.nn.functional as F

# name -> (individual, K, features per step, has Linear_Decoder); reference sizes below
VARIANTS = {
    "sevir": (False, 3, 1, True),
    "ind": (True, 3, 1, True),
    "indc_indp": (True, 5, 4, False),
}
TIN, TOUT = 13, 12
REF_LATENT = (4, 48, 48)
NAMES = ("Linear_Seasonal", "Linear_Trend", "Linear_Decoder")


def decomp(x, K):
    """x (B, L, M) -> (seasonal, trend): replicate padding of (K-1)//2 rows, AvgPool1d(K, stride 1)"""
    h = (K - 1) // 2
    xp = torch.cat([x[:, :1].repeat(1, h, 1), x, x[:, -1:].repeat(1, h, 1)], dim=1)
    t = F.avg_pool1d(xp.permute(0, 2, 1), K, 1).permute(0, 2, 1)
    return x - t, t


def apply(x, ws, bs, wt, bt, K, individual):
    """x (B, L, M) -> (B, P, M)"""
    s, t = decomp(x, K)
    if individual:
        return (torch.einsum("mpl,blm->bpm", ws, s) + bs.t()[None] + torch.einsum("mpl,blm->bpm", wt, t)
                + bt.t()[None])
    return torch.einsum("pl,blm->bpm", ws, s) + bs[None, :, None] + torch.einsum("pl,blm->bpm", wt, t) + bt[None, :, None]


def rows(v, cf):
    """latents (B, T, C, h, w) -> (B, T*cf, M)"""
    b, t, c, h, w = v.shape
    return v.reshape(b, t * cf, c * h * w // cf)


def diff_inputs(r, L, cf):
    """row l minus row L - cf + l % cf, rows [0, L)"""
    return r[:, :L] - r[:, L - cf:L].repeat(1, L // cf, 1)


def target(r, L, P, cf):
    return r[:, L:L + P] - r[:, L - cf:L].repeat(1, P // cf, 1)


def loss_and_pred(v, params, K, individual, cf):
    r = rows(v, cf)
    L, P = TIN * cf, TOUT * cf
    pred = apply(diff_inputs(r, L, cf), *params, K, individual)
    return F.mse_loss(pred, target(r, L, P, cf)), pred


def stacked_from_state_dict(sd, individual, M):
    """reference-layout state dict -> {name: (weight, bias)} stacked"""
    out = {}
    for n in NAMES:
        if individual:
            if f"{n}.0.weight" not in sd:
                continue
            out[n] = (torch.stack([sd[f"{n}.{i}.weight"] for i in range(M)]),
                      torch.stack([sd[f"{n}.{i}.bias"] for i in range(M)]))
        elif f"{n}.weight" in sd:
            out[n] = (sd[f"{n}.weight"], sd[f"{n}.bias"])
    return out


def keys_digest(items):
    """sha256 of the ordered (key, shape) list"""
    h = hashlib.sha256()
    for k, shape in items:
        h.update(f"{k} {tuple(int(s) for s in shape)}\n".encode())
    return h.hexdigest()


def values_digest(sd):
    """sha256 of the fp32 bytes of every tensor, in key order"""
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(v.detach().to(torch.float32).contiguous().cpu().numpy().tobytes())
    return h.hexdigest()
