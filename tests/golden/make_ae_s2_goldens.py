"""Generate tests/golden/g24_ae_s2.npz from the reference's own `ae_s2` classes (CPU).

    python tests/golden/make_ae_s2_goldens.py <reference checkout root>

experiments/ae_s2/train.py imports pytorch_lightning, omegaconf and wandb at module level, so it is not imported: its
`Autoencoder`, `moving_avg`, `series_decomp`, `DLinear` and `Model` class definitions are taken out of the file with `ast`
at run time and executed against torch, with `pl.LightningModule` standing in as `nn.Module` and the two logging helpers
as recorders.  The constructors of `Autoencoder` and `Model` (a hard-coded checkpoint path, `save_hyperparameters`) are
not run; the objects are assembled from the reference's AutoencoderKL and DLinear, and then the reference's own
`Autoencoder.encode` / `decode` loops and `Model.training_step` / `validation_step` do the arithmetic.  Nothing from the
reference is copied; the fixture holds inputs and recorded results only.

Geometry (tests/ae_s2_ref.py): AutoencoderKL "small" (tests/aekl_ref.py), B = 2, T = 13 = 7 in + 6 out, 32 x 32 frames ->
latents 4 x 8 x 8, enc_in = 256.  Seeds: `seed` (AutoencoderKL weights), `seed` + 1 (DLinear), `seed` + 2 (frames, k / 255
like SEVIR's), `noise_seed`: torch.manual_seed before the first encode — the reference samples from the global generator.
`noise` (4, T, B, C, h, w): draw [i] is what the i-th encode of the run consumed (T calls of randn((B, C, h, w))); encode 0
is the recorded step, encodes 1 .. 3 the optimiser steps.

Every result is computed in fp32 by the reference and again by an fp64 copy of it on the same noise: `<name>` is the fp64
value (tensors rounded to fp32 for storage), `<name>_32` the fp32 one, `<name>_spread` = max|a32 - a64| / max|a64|.
  z (B, T, C, h, w), loss, pred (B, P, 3) and grad_seasonal_w / grad_seasonal_b / grad_trend_w / grad_trend_b of the
  latent scalars `columns`; `grad_norm` of all gradients; val_loss, decoded_pred, decoded_tgt (B, 6, 1, H, W) of
  validation_step; step_loss (3): clip_grad_norm_(1.0) + torch.optim.AdamW(lr, weight_decay, betas) as `lr`, `wd`, `betas`.
`dlinear_init_sha`: the seeded initial DLinear state dict.  `config_keys`: the dotted keys of the reference's config.yaml.
At the reference size (enc_in 16384): `ref_nkeys`, `ref_keys_sha`, `ref_head`, `ref_init_sha`.
"""
from __future__ import annotations

import ast
import copy
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import ae_s2_ref as S  # noqa: E402
from tests import aekl_ref as A  # noqa: E402
from tests import dlinear_ref as D  # noqa: E402

SEED, NOISE_SEED = 1234, 4321
B = 2
NAMES = ("z", "loss", "pred", "grad_seasonal_w", "grad_seasonal_b", "grad_trend_w", "grad_trend_b", "grad_norm", "val_loss",
         "decoded_pred", "decoded_tgt", "step_loss")


def load_classes(root, AutoencoderKL, seen):
    path = os.path.join(root, "experiments", "ae_s2", "train.py")
    tree = ast.parse(open(path).read(), path)
    want = ["Autoencoder", "moving_avg", "series_decomp", "DLinear", "Model"]
    keep = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in want]
    assert [n.name for n in keep] == want, path
    ns = {"torch": torch, "nn": nn, "F": F, "pl": types.SimpleNamespace(LightningModule=nn.Module),
          "AutoencoderKL": AutoencoderKL,
          "log_metrics": lambda pred, tgt, tag, model: seen.update(decoded_pred=pred, decoded_tgt=tgt),
          "log_wandb_images": lambda *a, **k: None}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns


def assemble(ns, vae, predictor, encode=None):
    """the reference's Model around `vae` and `predictor` without its constructors; `encode`: replaces the sampling encode
    (the fp64 copy reuses the fp32 run's noise)"""
    ae = ns["Autoencoder"].__new__(ns["Autoencoder"])
    nn.Module.__init__(ae)
    ae.autoencoder = vae
    if encode is not None:
        ae.encode = encode
    m = ns["Model"].__new__(ns["Model"])
    nn.Module.__init__(m)
    m.autoencoder, m.predictor = ae, predictor
    m.input_frames, m.pred_frames = S.TIN, S.TOUT
    m.cfg = types.SimpleNamespace(logging=types.SimpleNamespace(log_train_plots_n=1.0),
                                  trainer=types.SimpleNamespace(total_val_steps=1))
    m.current_epoch = 0
    m.log = lambda *a, **k: None
    return m


def columns(t, dim=-1):
    """the recorded latent scalars: the last dimension of pred (B, P, M), the first of the stacked gradients (M, ...)"""
    return t.index_select(dim, torch.tensor(S.COLUMNS))


def record(model, frames, seen):
    """one training_step with gradients, one validation_step, three optimiser steps -> {name: value}; every call of the
    model's encode consumes noise in order"""
    out = {}
    batch = {"vil": frames}
    loss = model.training_step(batch, 0)
    loss.backward()
    sd = {k: p.grad for k, p in model.predictor.named_parameters() if p.grad is not None}
    g = D.stacked_from_state_dict(sd, True, model.predictor.channels)
    out["loss"] = loss.detach()
    out["grad_seasonal_w"], out["grad_seasonal_b"] = (columns(t, 0) for t in g["Linear_Seasonal"])
    out["grad_trend_w"], out["grad_trend_b"] = (columns(t, 0) for t in g["Linear_Trend"])
    out["grad_norm"] = torch.sqrt(sum((t.double() ** 2).sum() for t in sd.values()))
    model.predictor.zero_grad(set_to_none=True)
    opt = torch.optim.AdamW(model.predictor.parameters(), lr=S.LR, weight_decay=S.WD, betas=S.BETAS)
    losses = []
    for _ in range(3):
        loss = model.training_step(batch, 0)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.predictor.parameters(), S.CLIP)
        opt.step()
        opt.zero_grad(set_to_none=True)
        losses.append(loss.detach())
    out["step_loss"] = torch.stack(losses)
    return out


def main(argv):
    root = argv[1] if len(argv) > 1 else os.environ.get("WFAE_REFERENCE_ROOT")
    if not root:
        raise SystemExit(__doc__)
    sys.path.insert(0, root)
    from pipeline.models.autoencoderkl.autoencoder_kl import AutoencoderKL
    seen = {}
    ns = load_classes(root, AutoencoderKL, seen)
    cfg = A.CONFIGS[S.AE_CONFIG]
    torch.manual_seed(SEED)
    vae32 = AutoencoderKL(**cfg).eval().requires_grad_(False)
    vae64 = copy.deepcopy(vae32).double()
    c, hw = cfg["latent_channels"], S.FRAME // 2 ** (len(cfg["block_out_channels"]) - 1)
    M = c * hw * hw
    dcfg = types.SimpleNamespace(seq_len=S.TIN, pred_len=S.TOUT, individual=True, enc_in=M, kernel_size=S.K)
    torch.manual_seed(SEED + 1)
    pred32 = ns["DLinear"](dcfg)
    init = {k: v.detach().clone() for k, v in pred32.state_dict().items()}
    pred64 = copy.deepcopy(pred32).double()
    T = S.TIN + S.TOUT
    u8 = torch.randint(0, 256, (B, T, 1, S.FRAME, S.FRAME), generator=torch.Generator().manual_seed(SEED + 2), dtype=torch.uint8)
    frames = u8.float() / 255

    # the noise the fp32 run will consume: 4 encodes of T draws each, from the global generator
    torch.manual_seed(NOISE_SEED)
    noise = torch.stack([torch.stack([torch.randn((B, c, hw, hw)) for _ in range(T)]) for _ in range(4)])

    m32 = assemble(ns, vae32, pred32)
    ref_encode = ns["Autoencoder"].encode
    z_seen = []

    def encode32(x):                                   # the reference's sampling loop, recorded
        z_seen.append(ref_encode(m32.autoencoder, x))
        return z_seen[-1]

    m32.autoencoder.encode = encode32
    torch.manual_seed(NOISE_SEED)
    r32 = record(m32, frames, seen)
    # the draw itself, exactly: mean + std * noise of the reference's own posterior, frame by frame, for all four encodes
    assert len(z_seen) == 4
    with torch.no_grad():
        for t in range(T):
            p = vae32.encode(frames[:, t])
            for i in range(4):
                assert torch.equal(z_seen[i][:, t], p.mean + p.std * noise[i, t]), "the stored noise is not the reference's draw"

    # fp64: the same noise through the reference's posterior, then the reference's steps
    calls = [0]

    def encode64(x):
        i = calls[0]
        calls[0] += 1
        with torch.no_grad():
            out = []
            for t in range(T):
                p = vae64.encode(x[:, t])
                out.append((p.mean + p.std * noise[i, t].double()).unsqueeze(1))
            return torch.cat(out, dim=1)

    m64 = assemble(ns, vae64, pred64, encode=encode64)
    r64 = record(m64, frames.double(), seen)
    calls[0] = 0
    r32["z"], r64["z"] = z_seen[0], encode64(frames.double())

    # pred of the recorded step and validation_step, on the initial parameters and encode 0's noise
    for r, m, vae, fr, dt in ((r32, m32, vae32, frames, torch.float32), (r64, m64, vae64, frames.double(), torch.float64)):
        fresh = ns["DLinear"](dcfg).to(dt)
        fresh.load_state_dict({k: v.to(dt) for k, v in init.items()})
        z0 = r["z"]
        v = assemble(ns, vae, fresh, encode=lambda x, z0=z0: z0)
        with torch.no_grad():
            b = z0.shape[0]
            inp = z0[:, :S.TIN] - z0[:, S.TIN - 1:S.TIN]
            r["pred"] = columns(v(inp.reshape(b, S.TIN, M)))
            r["val_loss"] = v.validation_step({"vil": fr}, 0)
        r["decoded_pred"], r["decoded_tgt"] = seen["decoded_pred"], seen["decoded_tgt"]
        assert r["decoded_pred"].shape == (B, S.TOUT, 1, S.FRAME, S.FRAME)
        assert abs(float(r["val_loss"]) - float(r["loss"])) <= 1e-6 * abs(float(r["loss"]))

    # the restatement is the same function: fp64 against fp64 (to the fp32 softmax of the reference's attention, 1e-8)
    sd64 = A.cast(dict(vae64.state_dict()), torch.float64)
    zr = S.encode(sd64, frames.double(), cfg, noise[0].double())
    assert S.spread(zr, r64["z"]) < 2e-7
    st = D.stacked_from_state_dict({k: v.double() for k, v in init.items()}, True, M)
    params = (*st["Linear_Seasonal"], *st["Linear_Trend"])
    loss_r, pred_r = S.step(r64["z"], params)
    assert abs(float(loss_r) - float(r64["loss"])) < 1e-12 and S.spread(columns(pred_r), r64["pred"]) < 1e-12
    fc, tg = S.forecast_and_target(r64["z"], pred_r)
    assert S.spread(S.decode(sd64, fc, cfg), r64["decoded_pred"]) < 2e-7
    assert S.spread(S.decode(sd64, tg, cfg), r64["decoded_tgt"]) < 2e-7

    out = {"seed": np.int64(SEED), "noise_seed": np.int64(NOISE_SEED), "frames_u8": u8.numpy(), "noise": noise.numpy(),
           "columns": np.array(S.COLUMNS), "lr": np.float64(S.LR), "wd": np.float64(S.WD), "betas": np.array(S.BETAS),
           "dlinear_init_sha": np.array(D.values_digest(init))}
    for name in NAMES:
        a32, a64 = r32[name].detach(), r64[name].detach()
        out[name + "_spread"] = np.float64(S.spread(a32, a64))
        scalar = a64.numel() <= 3
        out[name] = a64.double().numpy() if scalar else a64.float().numpy()
        out[name + "_32"] = a32.double().numpy() if scalar else a32.float().numpy()
        print(f"{name}: spread {float(out[name + '_spread']):.3e}")

    with open(os.path.join(root, "experiments", "ae_s2", "config.yaml")) as f:
        out["config_keys"] = np.array(S.flat_keys(yaml.safe_load(f)))

    # reference size: key list and seeded initial values, as digests
    big_cfg = types.SimpleNamespace(seq_len=S.TIN, pred_len=S.TOUT, individual=True, enc_in=16384, kernel_size=S.K)
    torch.manual_seed(SEED)
    big = ns["DLinear"](big_cfg).state_dict()
    items = [("predictor." + k, tuple(t.shape)) for k, t in big.items()]
    out["ref_nkeys"] = np.int64(len(items))
    out["ref_keys_sha"] = np.array(D.keys_digest(items))
    out["ref_head"] = np.array([k for k, _ in items[:8]])
    out["ref_init_sha"] = np.array(D.values_digest(big))

    path = os.path.join(HERE, "g24_ae_s2.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    if size > 1_000_000:
        raise SystemExit(f"{path}: {size} bytes exceeds the 1 000 000 byte limit for a committed fixture")


if __name__ == "__main__":
    main(sys.argv)
