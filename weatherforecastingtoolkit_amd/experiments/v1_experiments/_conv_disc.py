"""Conv + GAN latent model of the reference's v1 experiments:
experiments/v1_experiments/pretrained_ae_conv_disc/train.py without Lightning / W&B.

Reference (:140-206): the latents (B, 64, 16, 16) of the frozen AutoencoderKL go through four [Conv2d 3x3 stride 2 + SiLU]
stages (64 -> 128 -> 256 -> 512 -> 1024 channels, 16 -> 1 pixels), a 1x1 convolution and Linear 1024 -> 512 (`z`), then
Linear 512 -> 1024, four [ConvTranspose2d 3x3 stride 2 output_padding 1 + SiLU] stages (1024 -> 1024 -> 512 -> 256 -> 128)
and a 1x1 convolution 128 -> 64.  The loss (:26-100) is L1 as a negative log-likelihood, `rec / exp(logvar) + logvar`
divided by the batch size, plus — from `disc_start` on — the adaptive-weight generator term of a PatchGAN on the latents,
and the hinge loss for that discriminator; the step (:240-274) is manual optimisation, generator first.

Each conv + SiLU stage is ONE entry point forward, one for the data gradient and one for the weight and bias gradients
(csrc/c3s2.hip).  The 1x1 convolution on the 1x1 plane is a Linear and runs as one; the last 1x1 goes through the
library's conv1x1 (its weight is the `last_layer` of the adaptive weight).  The torch module classes are kept as
parameter containers, built and initialised in the reference's order, so state_dict keys / order / shapes and the seeded
initial values are the reference's.

Two things in the reference are broken; this module decides them:
  1. `configure_optimizers` (:300) hands the FROZEN latent provider to the generator's AdamW, so as written the predictor
     never changes.  Built here is the evident intent: the generator optimiser owns `predictor` (`Step.trained`), as in the
     other v1 models.  There is no switch for the bug.
  2. `perceptual_weight > 0` (:56-60) repeats the 64-channel latent to 192 channels and feeds it to a VGG16 that takes 3:
     it cannot run, and the shipped config has 0.0.  `Loss` refuses a positive value.  `kl_weight` is read and never used
     by the reference; the key is kept and ignored.
One smaller difference: `loss.logvar` is created with requires_grad=False.  The reference's is a plain nn.Parameter
(requires_grad=True) that no optimiser owns, so it never moves there either; value and state-dict key are the same, and here
no backward pass forms a gradient nobody reads.
"""
from __future__ import annotations

import math

import torch
import torch.nn as tnn

from ... import functional as Fn
from ... import parallel
from ..._lib import WfaeError
from ...pipeline import helpers
from .. import _gan
from .._gan import GanLoss
from ._latents import Autoencoder  # noqa: F401  (the frozen latent provider)
from ._runner import Step

LATENT_SHAPE = (64, 16, 16)   # what the model takes: the AutoencoderKL's latent at 128 x 128


def _as_matrix(w):
    """(Cout, Cin, 1, 1) -> (Cout, Cin): the same memory, and the same slot of the optimiser's gradient arena"""
    m = w.view(w.shape[0], w.shape[1])
    gv = getattr(w, "_wfae_grad_view", None)
    if gv is not None:
        m._wfae_grad_view = gv.view(m.shape)
    return m


def _units(seq, x, transposed):
    """walk Sequential(conv, SiLU, conv, SiLU, ...): each pair is one fused launch family"""
    mods = list(seq)
    for conv, act in zip(mods[0::2], mods[1::2]):
        if not isinstance(act, tnn.SiLU):
            raise WfaeError(f"conv unit: expected SiLU after the convolution, got {type(act).__name__}")
        want = conv.in_channels
        if x.dim() != 4 or x.shape[1] != want:
            raise WfaeError(f"conv unit: expected (N, {want}, H, W), got {tuple(x.shape)}")
        op = conv.output_padding if transposed else 0
        x = Fn.conv3x3s2_act(x, conv.weight, conv.bias, transposed, True, op)
    return x


class Encoder(tnn.Module):
    """reference :140-162"""

    def __init__(self, latent_dim):
        super().__init__()
        self.conv = tnn.Sequential(
            tnn.Conv2d(64, 128, 3, stride=2, padding=1), tnn.SiLU(inplace=True),
            tnn.Conv2d(128, 256, 3, stride=2, padding=1), tnn.SiLU(inplace=True),
            tnn.Conv2d(256, 512, 3, stride=2, padding=1), tnn.SiLU(inplace=True),
            tnn.Conv2d(512, 1024, 3, stride=2, padding=1), tnn.SiLU(inplace=True),
        )
        self.conv_out = tnn.Conv2d(1024, 1024, 1, 1, 0)
        self.fc = tnn.Linear(1024, latent_dim)

    def forward(self, x):
        x = _units(self.conv, x, False)
        if tuple(x.shape[2:]) != (1, 1):
            raise WfaeError(f"Encoder: the four stride-2 stages must end on a 1x1 plane, got {tuple(x.shape)}")
        x = x.view(x.size(0), -1)
        x = Fn.LinearFn.apply(x, _as_matrix(self.conv_out.weight), self.conv_out.bias)   # a 1x1 conv on a 1x1 plane
        return Fn.LinearFn.apply(x, self.fc.weight, self.fc.bias)


class Decoder(tnn.Module):
    """reference :164-188"""

    def __init__(self, latent_dim):
        super().__init__()
        self.fc = tnn.Linear(latent_dim, 1024)
        self.deconv = tnn.Sequential(
            tnn.ConvTranspose2d(1024, 1024, 3, stride=2, padding=1, output_padding=1), tnn.SiLU(inplace=True),
            tnn.ConvTranspose2d(1024, 512, 3, stride=2, padding=1, output_padding=1), tnn.SiLU(inplace=True),
            tnn.ConvTranspose2d(512, 256, 3, stride=2, padding=1, output_padding=1), tnn.SiLU(inplace=True),
            tnn.ConvTranspose2d(256, 128, 3, stride=2, padding=1, output_padding=1), tnn.SiLU(inplace=True),
        )
        self.conv_out = tnn.Conv2d(128, 64, 1, 1, 0)

    def forward(self, z):
        x = Fn.LinearFn.apply(z, self.fc.weight, self.fc.bias)
        x = _units(self.deconv, x.view(x.size(0), 1024, 1, 1), True)
        return Fn.conv1x1(x, self.conv_out.weight, self.conv_out.bias)


class ConvModel(tnn.Module):
    """reference :190-206"""

    def __init__(self, latent_dim=512):
        super().__init__()
        self.encoder = Encoder(latent_dim)
        self.decoder = Decoder(latent_dim)
        self.apply(self._init_weights)

    def _init_weights(self, m):
        if isinstance(m, (tnn.Conv2d, tnn.ConvTranspose2d, tnn.Linear)):
            tnn.init.kaiming_normal_(m.weight, nonlinearity="relu")
            if m.bias is not None:
                tnn.init.zeros_(m.bias)

    def forward(self, x):
        """x (B, 64, 16, 16) -> (z (B, latent_dim), recon (B, 64, 16, 16))"""
        if x.dim() != 4 or tuple(x.shape[1:]) != LATENT_SHAPE:
            raise WfaeError(f"ConvModel: expected latents (B, {', '.join(map(str, LATENT_SHAPE))}) — the AutoencoderKL's "
                            f"latent of a 128 x 128 frame (autoencoder.kind: autoencoder_kl, latent_channels: 64) — got "
                            f"{tuple(x.shape)}; the project's own conv provider gives 64 x 8 x 8, which four stride-2 "
                            "stages cannot take to 1 x 1 and back to the same plane")
        z = self.encoder(x)
        return z, self.decoder(z)


class Loss(GanLoss):
    """reference :26-100 (`Loss`): L1 as a negative log-likelihood over the batch size, and the GAN half"""

    def __init__(self, disc_start, disc_num_layers=3, disc_in_channels=64, disc_weight=1.0, use_actnorm=False,
                 perceptual_weight=1.0, kl_weight=1.0, logvar_init=0.0):
        if perceptual_weight > 0:
            raise WfaeError(f"Loss: perceptual_weight = {perceptual_weight} > 0: the reference repeats the 64-channel latent "
                            "to 192 channels and feeds it to a VGG16 that takes 3 (train.py:56-60), which cannot run; the "
                            "shipped config sets lpips.perceptual_weight: 0.0")
        super().__init__(disc_start, disc_num_layers, disc_in_channels, disc_weight, use_actnorm)
        self.perceptual_weight = perceptual_weight
        self.kl_weight = kl_weight                     # read and never used by the reference either
        # a scalar Parameter that no optimiser owns (reference :41): it stays at logvar_init, and is part of the state dict
        self.logvar = tnn.Parameter(torch.ones(size=()) * logvar_init, requires_grad=False)
        self._lv = (None, 0.0)                         # (version of logvar, its host value)
        self._consts = {}

    def _logvar_value(self):
        v = self.logvar._version
        if self._lv[0] != (v, self.logvar.data_ptr()):
            self._lv = ((v, self.logvar.data_ptr()), float(self.logvar))
        return self._lv[1]

    def _const(self, value, device):
        key = (value, device)
        if key not in self._consts:
            self._consts[key] = torch.full((), value, dtype=torch.float32, device=device)
        return self._consts[key]

    def nll(self, inputs, reconstructions):
        """-> (nll, rec): rec = mean |recon - x|; nll = sum(rec / exp(logvar) + logvar) / batch size (:54,62-63)"""
        rec = Fn.l1_loss(reconstructions, inputs)
        lv, b = self._logvar_value(), inputs.size(0)
        nll = Fn.ScaleByFn.apply(rec, self._const(math.exp(-lv) / b, rec.device))
        if lv != 0.0:
            nll = Fn.AddFn.apply(nll, self._const(lv / b, rec.device))
        return nll, rec

    def forward(self, inputs, reconstructions, posteriors, optimizer_idx, last_layer, split, global_step, split_terms=False):
        """the reference's signature; `posteriors` (it is handed `z`) is unused there too.  -> (loss, log dict); with
        split_terms the discriminator's loss comes as its two terms (real, fake), whose sum it is"""
        inputs = inputs.detach()
        if global_step < self.disc_start or optimizer_idx == 0:
            nll, rec = self.nll(inputs, reconstructions)
            if global_step < self.disc_start:
                return nll, {f"{split}/total_loss": nll.detach(), f"{split}/rec_loss": rec.detach(),
                             f"{split}/nll_loss": nll.detach(), f"{split}/g_loss": 0.0, f"{split}/d_weight": 0.0}
            loss, g_loss, d_weight = self.generator_loss(nll, reconstructions, last_layer)
            return loss, {f"{split}/total_loss": loss.detach(), f"{split}/nll_loss": nll.detach(),
                          f"{split}/rec_loss": rec.detach(), f"{split}/g_loss": g_loss.detach(),
                          f"{split}/d_weight": d_weight}
        if optimizer_idx != 1:
            raise WfaeError(f"Loss: optimizer_idx {optimizer_idx!r}, expected 0 (generator) or 1 (discriminator)")
        if split_terms:
            # the two halves of the hinge loss on their own, for a caller that takes their gradients one after the other
            logits_real = self.discriminator(inputs)
            logits_fake = self.discriminator(reconstructions.detach())
            real = Fn.MeanFn.apply(logits_real, True, -1.0, 0.5)
            fake = Fn.MeanFn.apply(logits_fake, True, 1.0, 0.5)
            d_loss = Fn.AddFn.apply(real.detach(), fake.detach())
            return (real, fake), {f"{split}/disc_loss": d_loss, f"{split}/logits_real": logits_real.detach().mean(),
                                  f"{split}/logits_fake": logits_fake.detach().mean()}
        d_loss, logits_real, logits_fake = self.discriminator_loss(inputs, reconstructions)
        return d_loss, {f"{split}/disc_loss": d_loss.detach(), f"{split}/logits_real": logits_real.detach().mean(),
                        f"{split}/logits_fake": logits_fake.detach().mean()}


class Model(Step, tnn.Module):
    """reference Model (:208-314): `predictor`, `loss`, `forward`, the two-optimiser training step, validation / test"""

    exact_complements = True

    def __init__(self, cfg, autoencoder=None):
        super().__init__()
        self.cfg = cfg
        self.autoencoder = autoencoder
        lp = cfg.lpips
        self.loss = Loss(lp.disc_start, disc_num_layers=lp.disc_num_layers, disc_in_channels=lp.disc_in_channels,
                         disc_weight=lp.disc_weight, use_actnorm=lp.use_actnorm, perceptual_weight=lp.perceptual_weight,
                         kl_weight=lp.kl_weight, logvar_init=lp.logvar_init)
        self.predictor = ConvModel(latent_dim=int(cfg.predictor.latent_dim))
        self.input_frames, self.pred_frames = cfg.dataset.input_frames, cfg.dataset.pred_frames
        self.total_steps = cfg.trainer.total_train_steps
        self.accumulate_grad_batches = cfg.trainer.accumulate_grad_batches
        if self.accumulate_grad_batches != 1:
            raise WfaeError("Model: trainer.accumulate_grad_batches must be 1 (the shipped value)")
        self.global_step = 0
        self.logs = {}

    def forward(self, x):
        z, out = self.predictor(x)
        return out, z

    def get_last_layer(self):
        return self.predictor.decoder.conv_out.weight

    def configure_optimizers(self):
        """generator: AdamW(optim.*) on `predictor` + cosine_warmup.*; discriminator: AdamW(lpips.disc_*, the same weight
        decay) + the lpips.disc_* schedule (reference :299-314, with `predictor` where it names the frozen provider)"""
        o, sp, lp = self.cfg.optim, self.cfg.cosine_warmup, self.cfg.lpips
        super().configure_optimizers()
        for g in self.opt.param_groups:
            g["betas"] = (float(o.get("beta1", 0.9)), float(o.get("beta2", 0.999)))
        self.d_opt = helpers.adamw_optimizer(self.loss.discriminator, lp.disc_peak_lr, o.weight_decay,
                                             beta1=lp.disc_beta1, beta2=lp.disc_beta2,
                                             exact_complements=self.exact_complements)
        self.d_sch = helpers.cosine_warmup_scheduler(self.d_opt, lp.disc_start_lr, lp.disc_final_lr, lp.disc_peak_lr,
                                                     self.total_steps, lp.disc_warmup_ratio * self.total_steps)
        self._dp_d = parallel.DataParallelTrainer(self.loss.discriminator, self.d_opt)
        return self.opt, self.d_opt

    def optimizers(self):
        return [(self.opt, self.sch), (self.d_opt, self.d_sch)]

    def latents(self, batch):
        """-> (frames (B, T, 1, H, W) or None, latents (B * T, 64, 16, 16))"""
        frames, v = self.frames_latents(batch)
        if v.dim() != 5 or tuple(v.shape[2:]) != LATENT_SHAPE:
            raise WfaeError(f"Model: latents {tuple(v.shape)}, expected (B, T, {', '.join(map(str, LATENT_SHAPE))}): this "
                            "model needs autoencoder.kind: autoencoder_kl with 64 latent channels on 128 x 128 frames")
        return frames, v.reshape(-1, *LATENT_SHAPE).contiguous()

    def training_step(self, batch, batch_idx=0):
        """reference :240-274: G loss -> backward (discriminator frozen) -> clip -> AdamW -> schedule; from disc_start on
        the same for D on the detached reconstruction.  -> (generator loss, generator gradient norm before clipping);
        every logged value of the step is in `self.logs`"""
        _, v = self.latents(batch)
        pred, z = self(v)
        clip = self.cfg.optim.gradient_clip_val
        with _gan.frozen(self.loss.discriminator.parameters()):
            aeloss, logs = self.loss(v, pred, z, 0, self.get_last_layer(), "train", self.global_step)
            logs = dict(logs)
            _, gn = self.optimizer_step(aeloss)
        logs["train/g_grad_norm"] = gn
        if self.global_step >= self.loss.disc_start:
            # the hinge loss is a sum of a term on D(x) and one on D(recon): backward of one, then of the other.  The first
            # writes every gradient into the optimiser's flat buffer and the second is added to it there, so clip and AdamW
            # are one launch each; one backward through both would leave autograd's sums in 13 separate tensors
            (real, fake), log_d = self.loss(v, pred, z, 1, self.get_last_layer(), "train", self.global_step,
                                            split_terms=True)
            logs.update(log_d)
            real.backward()
            fake.backward()
            self._dp_d.reduce_gradients()
            logs["train/d_grad_norm"] = self.d_opt.clip_grad_norm_(clip)
            self.d_opt.step()
            self.d_sch.step()
            self.d_opt.zero_grad(set_to_none=True)
        self.global_step += 1
        self.logs = logs
        return aeloss.detach(), gn

    @torch.no_grad()
    def validation_step(self, batch, batch_idx=0, split="val"):
        """reference :282-297: both loss calls (no gradients: d_weight is 0, as the reference's RuntimeError branch makes
        it) and, for a batch of frames with a provider that decodes, the calc_metrics keys of the decoded prediction
        against the frames.  -> (generator loss, logs)"""
        frames, v = self.latents(batch)
        pred, z = self(v)
        aeloss, logs = self.loss(v, pred, z, 0, self.get_last_layer(), split, self.global_step)
        logs = dict(logs)
        _, log_d = self.loss(v, pred, z, 1, self.get_last_layer(), split, self.global_step)
        logs.update(log_d)
        ae = self.autoencoder
        if frames is not None and getattr(ae, "can_decode", lambda: False)():
            decoded_pred = ae.decode(pred.view(frames.shape[0], frames.shape[1], *LATENT_SHAPE))
            logs.update(helpers.log_metrics(decoded_pred, frames, split))
            if self.panels is not None:
                # reference :295-297 (the train fraction and total, as it has them); it has no test step: the port's takes
                # the validation label with `_test` appended
                label = f"Reconstruction vs Original_epoch_{self.panels.epoch}_batch_{batch_idx}"
                helpers.plot_panels(self, decoded_pred, frames, label + ("_test" if split == "test" else ""), batch_idx,
                                    helpers.plot_fraction(self.cfg, "log_train_plots_n", 0.001), self.panels.total("train"))
        return aeloss, logs

    def test_step(self, batch, batch_idx=0):
        return self.validation_step(batch, batch_idx, split="test")


def model_state(model):
    """what `last.ckpt` holds, in Lightning's spelling: `predictor.*`, `loss.discriminator.*` and `loss.logvar`"""
    state = {"predictor." + k: v for k, v in model.predictor.state_dict().items()}
    state.update({"loss." + k: v for k, v in model.loss.state_dict().items()})
    return state
