"""KL autoencoder with a GAN loss, the reference's experiments/v1_experiments/ae_gan_kl/train.py without Lightning / W&B:
the `AutoencoderKL` itself is trained on SEVIR frames.

Reference (:27-110 `Loss`, :113-260 `Model`): rec = recon_weight * L1 (+ perceptual_weight * (1 - SSIM) when
perceptual_weight > 0: its LPIPS call is commented out, and `repeat(1, 3, 1, 1)` leaves the SSIM of a one-channel image
unchanged); nll = (rec / exp(logvar) + logvar) / B + kl_weight * sum(posterior.kl()) / B.  Below `disc_start` that is the
loss; from it on the generator adds d_weight * (-mean D(recon)) with the adaptive weight on `decoder.conv_out.weight`, and the
PatchGAN takes its hinge step with its own optimiser and schedule (`_gan.GanLoss`).  The step (:163-200) is manual
optimisation, generator first.  The model runs on csrc/aekl.hip + csrc/aekl_bwd.hip through `AutoencoderKL.unfreeze()`.

Three things in the reference do not run as written; this module decides them:
  1. It imports `custom_akl.AutoencoderKL` and calls it with `return_posterior=True`, which `custom_akl.forward` does not
     accept, and `custom_akl.decode` reshapes to (64, 8, 8) against latent_channels=512.  Built here is the
     `autoencoder_kl.AutoencoderKL` with the script's constructor arguments and its
     `forward(x, sample_posterior=True, return_posterior=True)`.  The arguments are the `autoencoder:` block of the config
     (the script hard-codes them).
  2. `loss.perceptual_loss` (an LPIPS whose weights the script downloads and never uses) is neither built nor emitted;
     its keys are skipped when a reference checkpoint is loaded (`load_model_state`).
  3. `loss.logvar` is an nn.Parameter that no optimiser of the reference owns, so there it gets a gradient and never
     moves.  Here the generator's optimiser owns it next to `autoencoder`: the evident intent of a learned log-variance.
"""
from __future__ import annotations

import torch
import torch.nn as tnn

from ... import functional as Fn
from ... import parallel
from ..._lib import WfaeError
from ...pipeline import helpers
from ...pipeline.models.autoencoderkl import AutoencoderKL
from .. import _gan
from .._gan import GanLoss
from ._runner import Step

# the constructor arguments of the script (train.py:118-131); `autoencoder:` in the config overrides them key by key
AUTOENCODER = dict(in_channels=1, out_channels=1, latent_channels=512, block_out_channels=(64, 128, 256, 512, 512),
                   sample_size=128, down_block_types=("DownEncoderBlock2D",) * 5, up_block_types=("UpDecoderBlock2D",) * 5)
SKIPPED_PREFIX = "loss.perceptual_loss."


class Loss(GanLoss):
    """reference :27-110"""

    def __init__(self, disc_start, disc_num_layers=3, disc_in_channels=1, disc_weight=1.0, use_actnorm=False,
                 perceptual_weight=1.0, kl_weight=1.0, logvar_init=0.0, recon_weight=1.0):
        super().__init__(disc_start, disc_num_layers, disc_in_channels, disc_weight, use_actnorm)
        self.perceptual_weight, self.kl_weight, self.recon_weight = perceptual_weight, kl_weight, recon_weight
        self.logvar = tnn.Parameter(torch.ones(size=()) * logvar_init)

    def nll(self, inputs, reconstructions, posteriors):
        """-> (nll, rec, kl): the scalar arithmetic around the loss kernels is torch's, on 0-dim tensors"""
        b = inputs.size(0)
        rec = self.recon_weight * Fn.l1_loss(reconstructions, inputs)
        if self.perceptual_weight > 0:
            rec = rec + self.perceptual_weight * (1.0 - Fn.ssim(inputs, reconstructions))
        kl = torch.sum(posteriors.kl()) / b
        nll = (rec / torch.exp(self.logvar) + self.logvar) / b + kl * self.kl_weight
        return nll, rec, kl

    def forward(self, inputs, reconstructions, posteriors, optimizer_idx, last_layer, split, global_step):
        inputs = inputs.detach()
        if global_step < self.disc_start or optimizer_idx == 0:
            nll, rec, kl = self.nll(inputs, reconstructions, posteriors)
            logs = {f"{split}/rec_loss": rec.detach(), f"{split}/kl_loss": kl.detach(), f"{split}/nll_loss": nll.detach()}
            if global_step < self.disc_start:
                return nll, dict(logs, **{f"{split}/total_loss": nll.detach(), f"{split}/g_loss": 0.0, f"{split}/d_weight": 0.0})
            loss, g_loss, d_weight = self.generator_loss(nll, reconstructions, last_layer)
            return loss, dict(logs, **{f"{split}/total_loss": loss.detach(), f"{split}/g_loss": g_loss.detach(),
                                       f"{split}/d_weight": d_weight})
        if optimizer_idx != 1:
            raise WfaeError(f"Loss: optimizer_idx {optimizer_idx!r}, expected 0 (generator) or 1 (discriminator)")
        d_loss, logits_real, logits_fake = self.discriminator_loss(inputs, reconstructions)
        return d_loss, {f"{split}/disc_loss": d_loss.detach(), f"{split}/logits_real": logits_real.detach().mean(),
                        f"{split}/logits_fake": logits_fake.detach().mean()}


class Generator(tnn.Module):
    """what the generator's optimiser owns: the autoencoder and the loss's log-variance (not part of any state dict)"""

    def __init__(self, autoencoder, logvar):
        super().__init__()
        self.autoencoder, self.logvar = autoencoder, logvar


class Model(Step, tnn.Module):
    """reference Model (:113-260): `autoencoder`, `loss`, the two-optimiser training step, validation / test"""

    exact_complements = True

    def __init__(self, cfg, autoencoder=None):
        super().__init__()
        if autoencoder is not None:
            raise WfaeError("ae_gan_kl trains its own AutoencoderKL: it takes no latent provider")
        self.cfg = cfg
        kw = dict(AUTOENCODER)
        kw.update({k: v for k, v in dict(cfg.get("autoencoder") or {}).items() if v is not None})
        for k in ("block_out_channels", "down_block_types", "up_block_types"):
            kw[k] = tuple(kw[k])
        self.autoencoder = AutoencoderKL(**kw).unfreeze()       # the reference's construction order: autoencoder, loss
        lp = cfg.lpips
        self.loss = Loss(lp.disc_start, disc_num_layers=lp.disc_num_layers, disc_in_channels=lp.disc_in_channels,
                         disc_weight=lp.disc_weight, use_actnorm=lp.use_actnorm, perceptual_weight=lp.perceptual_weight,
                         kl_weight=lp.kl_weight, logvar_init=lp.logvar_init, recon_weight=lp.recon_weight)
        self.total_steps = cfg.trainer.total_train_steps
        if cfg.trainer.accumulate_grad_batches != 1:
            raise WfaeError("Model: trainer.accumulate_grad_batches must be 1 (the shipped value)")
        self.global_step = 0
        self.logs = {}

    def forward(self, x, generator=None):
        return self.autoencoder(x, sample_posterior=True, return_posterior=True, generator=generator)

    def get_last_layer(self):
        return self.autoencoder.decoder.conv_out.weight

    def configure_optimizers(self):
        """generator: AdamW(optim.*) on the autoencoder and loss.logvar + cosine_warmup.*; discriminator: AdamW(lpips.disc_*,
        the same weight decay) + the lpips.disc_* schedule (reference :240-257)"""
        o, sp, lp = self.cfg.optim, self.cfg.cosine_warmup, self.cfg.lpips
        net = Generator(self.autoencoder, self.loss.logvar)
        self.opt = helpers.adamw_optimizer(net, o.lr, o.weight_decay, beta1=o.beta1, beta2=o.beta2,
                                           exact_complements=self.exact_complements)
        self.sch = helpers.cosine_warmup_scheduler(self.opt, sp.start_lr, sp.final_lr, sp.peak_lr, self.total_steps,
                                                   sp.warmup_ratio * self.total_steps)
        self._dp = parallel.DataParallelTrainer(net, self.opt)
        self.d_opt = helpers.adamw_optimizer(self.loss.discriminator, lp.disc_peak_lr, o.weight_decay, beta1=lp.disc_beta1,
                                             beta2=lp.disc_beta2, exact_complements=self.exact_complements)
        self.d_sch = helpers.cosine_warmup_scheduler(self.d_opt, lp.disc_start_lr, lp.disc_final_lr, lp.disc_peak_lr,
                                                     self.total_steps, lp.disc_warmup_ratio * self.total_steps)
        self._dp_d = parallel.DataParallelTrainer(self.loss.discriminator, self.d_opt)
        return self.opt, self.d_opt

    def optimizers(self):
        return [(self.opt, self.sch), (self.d_opt, self.d_sch)]

    @staticmethod
    def frames(batch):
        """the loader's batch (a tensor or its dict; (B, T, H, W) or (B, 1, H, W) frames) -> (B * T, 1, H, W)"""
        if isinstance(batch, dict):
            batch = batch["vil"]
        if batch.dim() != 4:
            raise WfaeError(f"Model: expected frames (B, T, H, W), got {tuple(batch.shape)}")
        return batch.reshape(-1, 1, batch.shape[2], batch.shape[3]).contiguous()

    def training_step(self, batch, batch_idx=0):
        """reference :163-200: G loss -> backward (discriminator frozen) -> clip -> AdamW -> schedule; from disc_start on the
        same for D on the detached reconstruction.  -> (generator loss, generator gradient norm before clipping)"""
        x = self.frames(batch)
        pred, post = self(x)
        clip = self.cfg.optim.gradient_clip_val
        with _gan.frozen(self.loss.discriminator.parameters()):
            aeloss, logs = self.loss(x, pred, post, 0, self.get_last_layer(), "train", self.global_step)
            logs = dict(logs)
            _, gn = self.optimizer_step(aeloss)
        logs["train/g_grad_norm"] = gn
        if self.global_step >= self.loss.disc_start:
            d_loss, log_d = self.loss(x, pred, post, 1, self.get_last_layer(), "train", self.global_step)
            logs.update(log_d)
            d_loss.backward()
            self._dp_d.reduce_gradients()
            logs["train/d_grad_norm"] = self.d_opt.clip_grad_norm_(clip)
            self.d_opt.step()
            self.d_sch.step()
            self.d_opt.zero_grad(set_to_none=True)
        self.global_step += 1
        self.logs = logs
        if self.panels is not None:
            self._plot(pred, x, "train", self.panels.batch_idx)
        return aeloss.detach(), gn

    def _plot(self, pred, inp, split, batch_idx):
        """the figures of reference :196-198, :211-213, :226-228: the batch index against int(fraction * total), the train fraction and total in
        the training step, the validation ones in the validation AND the test step"""
        if self.panels is None:
            return
        e, tr = self.panels.epoch, split == "train"
        label = {"train": "Train Reconstruction", "val": "Val_Reconstruction", "test": "Test_Reconstruction"}[split] \
            + f" vs Original_epoch_{e}_batch_{batch_idx}" + ("_test" if split == "test" else "")
        helpers.plot_panels(self, pred, inp, label, batch_idx,
                            helpers.plot_fraction(self.cfg, "log_train_plots_n" if tr else "log_val_plots_n", 0.1),
                            self.panels.total("train" if tr else "val"))

    @torch.no_grad()
    def validation_step(self, batch, batch_idx=0, split="val"):
        """reference :202-230: both loss calls (no gradients: d_weight is 0, as the reference's RuntimeError branch makes it)
        and the calc_metrics keys of the reconstruction.  -> (generator loss, logs)"""
        x = self.frames(batch)
        pred, post = self(x)
        aeloss, logs = self.loss(x, pred, post, 0, self.get_last_layer(), split, self.global_step)
        logs = dict(logs)
        logs.update(self.loss(x, pred, post, 1, self.get_last_layer(), split, self.global_step)[1])
        logs.update(helpers.log_metrics(pred.unsqueeze(2), x.unsqueeze(2), split))
        self._plot(pred, x, split, batch_idx)
        return aeloss, logs

    def test_step(self, batch, batch_idx=0):
        return self.validation_step(batch, batch_idx, split="test")


def model_state(model):
    """what `last.ckpt` holds, in Lightning's spelling: `autoencoder.*`, `loss.logvar`, `loss.discriminator.*`"""
    state = {"autoencoder." + k: v for k, v in model.autoencoder.state_dict().items()}
    state.update({"loss." + k: v for k, v in model.loss.state_dict().items()})
    return state


def load_model_state(model, state):
    """load `model_state` (or a reference checkpoint's state dict) strictly, but for the reference's unused
    `loss.perceptual_loss.*`, which is skipped"""
    state = {k: v for k, v in state.items() if not k.startswith(SKIPPED_PREFIX)}
    model.autoencoder.load_state_dict({k[len("autoencoder."):]: v for k, v in state.items() if k.startswith("autoencoder.")})
    model.loss.load_state_dict({k[len("loss."):]: v for k, v in state.items() if k.startswith("loss.")})
    other = [k for k in state if not k.startswith(("autoencoder.", "loss."))]
    if other:
        raise WfaeError(f"load_model_state: keys of neither the autoencoder nor the loss: {other[:4]}")
    return model
