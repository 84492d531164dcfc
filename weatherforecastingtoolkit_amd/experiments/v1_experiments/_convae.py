"""Conv latent autoencoder of the reference's v1 experiments:
experiments/v1_experiments/pretrained_ae_convae_sevir/train.py without Lightning / W&B.

Reference (:58-143): the latents (B, T, 4, 48, 48) go frame by frame through `conv0` [Conv2d 3x3 + LayerNorm([8, 48, 48])
+ LeakyReLU(0.01)], three `down` units [Conv2d 4x4 stride 2 + LayerNorm + LeakyReLU], Linear 288 -> 512 (`z`),
Linear 512 -> 288, three `up` units [ConvTranspose2d 4x4 stride 2 + LayerNorm + LeakyReLU] and `conv_out` (Conv2d 3x3);
the step (:161-167) takes nn.HuberLoss between that reconstruction and the latents themselves.

Each of the seven units is ONE gfx950 launch forward (csrc/convae.hip: one workgroup holds a sample's convolution
output in LDS from the convolution to the activation) and one entry point backward.  The torch module classes are kept
as parameter containers, built and initialised in the reference's order, so state_dict keys / order / shapes and the
seeded initial values are the reference's.
"""
from __future__ import annotations

import argparse
import json
import os
import time

import torch
import torch.nn as tnn

from ... import config as C
from ... import functional as Fn
from ... import nn as wnn
from ... import ops, parallel, synth
from ..._lib import WfaeError
from ...pipeline import helpers
from ...pipeline.datasets.sevire.sevir import SEVIRFrameLoader
from ._dlinear import Autoencoder  # noqa: F401  (the frozen latent provider; it already decodes)

CLN_MAX_CIN, CLN_MAX_COUT, CLN_MAX_ELEMS = 64, 16, 18432   # served range of the fused unit (include/wfae.h)


def _check_geometry(what, cin, cout, size):
    if size < 8 or size % 8 != 0:
        raise WfaeError(f"{what}: size must be a positive multiple of 8 (three stride-2 stages), got {size}")
    if cin > CLN_MAX_CIN:
        raise WfaeError(f"{what}: {cin} input channels, the fused conv + LayerNorm unit serves Cin <= {CLN_MAX_CIN}")
    if cout > CLN_MAX_COUT:
        raise WfaeError(f"{what}: {cout} unit channels, the fused conv + LayerNorm unit serves Cout <= {CLN_MAX_COUT}")
    if cout * size * size > CLN_MAX_ELEMS:
        raise WfaeError(f"{what}: a sample of {cout}x{size}x{size} = {cout * size * size} elements, the fused conv + "
                        f"LayerNorm unit serves <= {CLN_MAX_ELEMS} (it is held in LDS)")


class _Unit(tnn.Sequential):
    """Sequential(conv, LayerNorm([C, s, s]), LeakyReLU()) of the reference, run as one fused launch"""

    def __init__(self, conv, channels, plane):
        super().__init__(conv, tnn.LayerNorm([channels, plane, plane]), tnn.LeakyReLU())
        if isinstance(conv, tnn.ConvTranspose2d):
            self.kind = ops.CLN_KINDS["up4"]
        else:
            self.kind = ops.CLN_KINDS["conv3" if conv.kernel_size == (3, 3) else "down4"]

    def forward(self, x):
        conv, ln, act = self[0], self[1], self[2]
        want = conv.in_channels
        if x.dim() != 4 or x.shape[1] != want:
            raise WfaeError(f"conv unit: expected (N, {want}, H, W), got {tuple(x.shape)}")
        return Fn.conv_layernorm_act(x, conv.weight, conv.bias, ln.weight, ln.bias, self.kind, act.negative_slope)


class ConvEncoder(tnn.Module):
    """reference :58-88; `size` (keyword only) is the latent plane, 48 in the reference"""

    def __init__(self, in_channels=4, bottleneck_channels=8, *, size=48):
        super().__init__()
        c = bottleneck_channels
        _check_geometry("ConvEncoder", in_channels, c, size)
        self.conv0 = _Unit(tnn.Conv2d(in_channels, c, kernel_size=3, padding=1), c, size)
        self.down1 = _Unit(tnn.Conv2d(c, c, kernel_size=4, stride=2, padding=1), c, size // 2)
        self.down2 = _Unit(tnn.Conv2d(c, c, kernel_size=4, stride=2, padding=1), c, size // 4)
        self.down3 = _Unit(tnn.Conv2d(c, c, kernel_size=4, stride=2, padding=1), c, size // 8)

    def forward(self, x):
        return self.down3(self.down2(self.down1(self.conv0(x))))


class ConvDecoder(tnn.Module):
    """reference :91-116"""

    def __init__(self, bottleneck_channels=8, out_channels=4, *, size=48):
        super().__init__()
        c = bottleneck_channels
        _check_geometry("ConvDecoder", c, c, size)
        self.up1 = _Unit(tnn.ConvTranspose2d(c, c, kernel_size=4, stride=2, padding=1), c, size // 4)
        self.up2 = _Unit(tnn.ConvTranspose2d(c, c, kernel_size=4, stride=2, padding=1), c, size // 2)
        self.up3 = _Unit(tnn.ConvTranspose2d(c, c, kernel_size=4, stride=2, padding=1), c, size)
        self.conv_out = wnn.Conv2d(c, out_channels, kernel_size=3, padding=1)

    def forward(self, x):
        return self.conv_out(self.up3(self.up2(self.up1(x))))


class ConvModel(tnn.Module):
    """reference :118-143.  Keyword-only extensions with the reference's values as defaults: `in_channels` and `size`
    of the latents (the project's own providers give 64 x 24 x 24 and 64 x 8 x 8)."""

    def __init__(self, latent_dim=512, *, in_channels=4, size=48):
        super().__init__()
        self.in_channels, self.size, self.bottleneck = in_channels, size, 8
        self.encoder = ConvEncoder(in_channels, self.bottleneck, size=size)
        self.decoder = ConvDecoder(self.bottleneck, in_channels, size=size)
        self.flat = self.bottleneck * (size // 8) ** 2
        self.to_latent = wnn.Linear(self.flat, latent_dim)
        self.to_reconstruction = wnn.Linear(latent_dim, self.flat)
        self.apply(self.init_weights)

    def init_weights(self, m):
        if isinstance(m, (tnn.Linear, tnn.Conv2d, tnn.ConvTranspose2d)):
            tnn.init.kaiming_normal_(m.weight, nonlinearity="leaky_relu")
            if m.bias is not None:
                tnn.init.zeros_(m.bias)

    def forward(self, x):
        """x (B, T, C, H, W) -> (z (B*T, latent_dim), reconstruction (B, T, C, H, W))"""
        if x.dim() != 5 or tuple(x.shape[2:]) != (self.in_channels, self.size, self.size):
            raise WfaeError(f"ConvModel: expected latents (B, T, {self.in_channels}, {self.size}, {self.size}), got "
                            f"{tuple(x.shape)}")
        b, t, c, h, w = x.shape
        s = self.size // 8
        y = self.encoder(x.reshape(b * t, c, h, w))
        z = self.to_latent(y.reshape(b * t, self.flat))
        y = self.to_reconstruction(z).reshape(b * t, self.bottleneck, s, s)
        return z, self.decoder(y).reshape(b, t, c, h, w)


class Model(tnn.Module):
    """reference Model (:145-207): `predictor`, `forward`, the training / validation / test steps and the optimiser"""

    def __init__(self, cfg, autoencoder=None):
        super().__init__()
        self.cfg = cfg
        self.autoencoder = autoencoder
        self.input_frames, self.pred_frames = cfg.dataset.input_frames, cfg.dataset.pred_frames
        self.total_steps = cfg.trainer.total_train_steps
        cv = cfg.convae
        self.predictor = ConvModel(latent_dim=int(cv.latent_dim), in_channels=int(cv.in_channels), size=int(cv.size))
        self.delta = 1.0   # nn.HuberLoss()

    def forward(self, x):
        return self.predictor(x)[1]

    def latent_loss(self, v):
        """latents (B, T, C, h, w) -> (loss, reconstruction): Huber(predictor(v), v), reference :166-167"""
        v = v.contiguous()
        pred = self(v)
        return Fn.huber_loss(pred, v, self.delta), pred

    def _frames_latents(self, batch):
        """-> (frames (B, T, 1, H, W) or None, latents (B, T, C, h, w))"""
        if isinstance(batch, dict):
            batch = batch["vil"]
        if batch.dim() == 4:
            if self.autoencoder is None:
                raise WfaeError("a batch of frames (B, T, H, W) needs the frozen autoencoder; pass latents "
                                "(B, T, C, h, w) or construct Model(cfg, autoencoder=...)")
            frames = batch.unsqueeze(2)
            return frames, self.autoencoder.encode(frames)
        return None, batch

    def _metric_interval(self, split):
        """the reference's metric cadence: every int(logging.log_<split>_all_metrics_n * total steps) batches"""
        lg = self.cfg.get("logging") or {}
        n = lg.get(f"log_{'train' if split == 'train' else 'val'}_all_metrics_n", 0) or 0
        return max(1, int(n * max(self.total_steps, 1)))

    def configure_optimizers(self):
        o, sp = self.cfg.optim, self.cfg.cosine_warmup
        self.opt = helpers.adamw_optimizer(self.predictor, o.lr, o.weight_decay, exact_complements=True)
        self.sch = helpers.cosine_warmup_scheduler(self.opt, sp.start_lr, sp.final_lr, sp.peak_lr, self.total_steps,
                                                   sp.warmup_ratio * self.total_steps)
        self._dp = parallel.DataParallelTrainer(self.predictor, self.opt)
        return self.opt

    def training_step(self, batch, batch_idx=0):
        """batch: frames (B, T, H, W) fp32 in [0, 1] ('NTHW') or latents (B, T, C, h, w); AdamW + cosine warmup, the
        gradient norm clipped at optim.gradient_clip_val.  -> (loss, gradient norm before clipping)"""
        _, v = self._frames_latents(batch)
        loss, _ = self.latent_loss(v)
        loss.backward()
        self._dp.reduce_gradients()
        gn = self.opt.clip_grad_norm_(self.cfg.optim.gradient_clip_val)
        self.opt.step()
        self.sch.step()
        self.opt.zero_grad(set_to_none=True)
        return loss.detach(), gn

    @torch.no_grad()
    def validation_step(self, batch, batch_idx=0, split="val"):
        """-> (loss, logs): logs holds `{split}_loss` and, for a batch of frames with a provider that decodes, the
        `{split}_` calc_metrics keys of the decoded reconstruction against the input frames (reference :189-192)"""
        frames, v = self._frames_latents(batch)
        loss, pred = self.latent_loss(v)
        logs = {f"{split}_loss": loss}
        ae = self.autoencoder
        if frames is not None and batch_idx % self._metric_interval(split) == 0 \
                and getattr(ae, "can_decode", lambda: False)():
            logs.update(helpers.log_metrics(ae.decode(pred), frames, split))
        return loss, logs

    def test_step(self, batch, batch_idx=0):
        return self.validation_step(batch, 0, split="test")


def main(here, default_mode, argv=None):
    """`--mode fit` trains (AdamW, cosine warmup, clip) and writes `last.ckpt` with `predictor.`-prefixed keys in the
    reference's layout; `--mode test` runs test_step over the loader"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=os.path.join(here, "config.yaml"))
    ap.add_argument("--max-steps", type=int, default=-1)
    ap.add_argument("--mode", choices=("fit", "test"), default=default_mode)
    args, unknown = ap.parse_known_args(argv)
    cfg = C.load(args.config)
    cli = C.from_dotlist(unknown)
    helpers.check_yaml(cfg, cli)
    cfg = C.merge(cfg, cli)
    rank, world, local = parallel.init_from_env()
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    size, frames = (384, 49) if cfg.dataset.name == "sevir" else (128, 25)
    events = synth.blob_events(max(2, cfg.dataset.batch_size * 2 * world), size, frames, seed=1234)
    loader = SEVIRFrameLoader(events, cfg.dataset.batch_size, cfg.dataset.seq_len, cfg.dataset.stride, "NTHW",
                              shuffle=args.mode == "fit", device=dev, num_shard=world, rank=rank)
    total = max(1, int(len(loader) * cfg.trainer.max_epochs / cfg.trainer.accumulate_grad_batches))
    if args.mode == "test":
        total = len(loader)
    if 0 < args.max_steps < total:
        total = args.max_steps
    cfg.trainer.total_train_steps = total
    torch.manual_seed(0)
    model = Model(cfg, autoencoder=Autoencoder(size, cfg.autoencoder.kind, cfg.autoencoder)).to(dev).train()
    model.autoencoder.eval()
    step, t0 = 0, time.time()
    if args.mode == "test":
        model.eval()
        for batch in loader:
            if step >= total:
                break
            loss, logs = model.test_step(batch["vil"], step)
            step += 1
            if rank == 0:
                print(json.dumps({"step": step, **{k: float(v) for k, v in logs.items()}}), flush=True)
        if rank == 0:
            print("done")
        return 0
    model.configure_optimizers()
    while step < total:
        for batch in loader:
            if step >= total:
                break
            loss, gn = model.training_step(batch["vil"])
            step += 1
            if rank == 0 and step % max(1, cfg.trainer.log_every_n_steps) == 0:
                print(json.dumps({"step": step, "train_loss": float(loss), "grad_norm": float(gn),
                                  "lr": model.opt.param_groups[0]["lr"],
                                  "frames_per_s": step * cfg.dataset.batch_size * cfg.dataset.seq_len * world
                                  / (time.time() - t0)}), flush=True)
    if rank == 0:
        out = os.path.join(cfg.experiment_path, "outputs", cfg.experiment_name, "checkpoints")
        os.makedirs(out, exist_ok=True)
        torch.save({"state_dict": {"predictor." + k: v.detach().cpu().clone()
                                   for k, v in model.predictor.state_dict().items()},
                    "global_step": step}, os.path.join(out, "last.ckpt"))
        print("done")
    return 0
