"""Conv latent autoencoder of the reference's v1 experiments:
experiments/v1_experiments/pretrained_ae_convae_sevir/train.py without Lightning / W&B.

Reference (:58-143): the latents (B, T, 4, 48, 48) go frame by frame through `conv0` [Conv2d 3x3 + LayerNorm([8, 48, 48])
+ LeakyReLU(0.01)], three `down` units [Conv2d 4x4 stride 2 + LayerNorm + LeakyReLU], Linear 288 -> 512 (`z`),
Linear 512 -> 288, three `up` units [ConvTranspose2d 4x4 stride 2 + LayerNorm + LeakyReLU] and `conv_out` (Conv2d 3x3);
the step (:161-167) takes nn.HuberLoss between that reconstruction and the latents themselves.

Each of the seven units is ONE gfx950 launch forward (csrc/convae.hip: one workgroup holds a sample's convolution
output in LDS from the convolution to the activation) and one entry point backward.  The torch module classes are kept
as parameter containers, built and initialised in the reference's order, so state_dict keys / order / shapes and the
seeded initial values are the reference's.  The frozen latent provider is ./_latents.py; the optimiser step and the
driver are the v1 experiments' shared ones (./_runner.py).
"""
from __future__ import annotations

import torch
import torch.nn as tnn

from ... import functional as Fn
from ... import nn as wnn
from ... import ops
from ..._lib import WfaeError
from ...pipeline import helpers
from ._latents import Autoencoder  # noqa: F401  (the frozen latent provider)
from ._runner import Step

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


class Model(Step, tnn.Module):
    """reference Model (:145-207): `predictor`, `forward`, the training / validation / test steps; the optimiser is
    `Step`'s, with the exact complements of FusedAdamW"""

    exact_complements = True

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

    def _metric_interval(self, split):
        """the reference's metric cadence: every int(logging.log_<split>_all_metrics_n * total steps) batches"""
        lg = self.cfg.get("logging") or {}
        n = lg.get(f"log_{'train' if split == 'train' else 'val'}_all_metrics_n", 0) or 0
        return max(1, int(n * max(self.total_steps, 1)))

    def training_step(self, batch, batch_idx=0):
        """batch: frames (B, T, H, W) fp32 in [0, 1] ('NTHW') or latents (B, T, C, h, w); AdamW + cosine warmup, the
        gradient norm clipped at optim.gradient_clip_val.  -> (loss, gradient norm before clipping)"""
        _, v = self.frames_latents(batch)
        loss, _ = self.latent_loss(v)
        return self.optimizer_step(loss)

    @torch.no_grad()
    def validation_step(self, batch, batch_idx=0, split="val", plot_idx=None):
        """-> (loss, logs): logs holds `{split}_loss` and, for a batch of frames with a provider that decodes, the
        `{split}_` calc_metrics keys of the decoded reconstruction against the input frames (reference :189-192)"""
        frames, v = self.frames_latents(batch)
        loss, pred = self.latent_loss(v)
        logs = {f"{split}_loss": loss}
        ae = self.autoencoder
        if frames is not None and batch_idx % self._metric_interval(split) == 0 \
                and getattr(ae, "can_decode", lambda: False)():
            decoded_pred = ae.decode(pred)
            logs.update(helpers.log_metrics(decoded_pred, frames, split))
            if self.panels is not None:
                # reference :194-196; it has no test step: the port's takes the validation label with `_test` appended
                i = batch_idx if plot_idx is None else plot_idx
                label = f"Reconstruction vs Original_epoch_{self.panels.epoch}_batch_{i}"
                helpers.plot_panels(self, decoded_pred, frames, label + ("_test" if split == "test" else ""), i,
                                    helpers.plot_fraction(self.cfg, "log_val_plots_n", 0.05), self.panels.total("val"))
        return loss, logs

    def test_step(self, batch, batch_idx=0):
        return self.validation_step(batch, 0, split="test", plot_idx=batch_idx)
