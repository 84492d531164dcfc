"""Conv + GAN latent model `pretrained_ae_conv_disc` on MI355X: the reference's
experiments/v1_experiments/pretrained_ae_conv_disc/train.py without Lightning / W&B — latents (64, 16, 16) of the frozen
AutoencoderKL are auto-encoded by a stride-2 conv / transposed-conv network with SiLU under an L1 negative
log-likelihood, joined from `lpips.disc_start` (a fraction of the total steps) by a PatchGAN on the latents.

    python -m weatherforecastingtoolkit_amd.experiments.v1_experiments.pretrained_ae_conv_disc.train key=value ...

The classes live in ../_conv_disc.py, the driver in ../_runner.py.  `last.ckpt` holds `predictor.*`,
`loss.discriminator.*` and `loss.logvar`.
"""
from __future__ import annotations

import os
import sys

from .._conv_disc import Autoencoder, ConvModel, Decoder, Encoder, Loss, Model, model_state  # noqa: F401
from .._runner import run, with_provider

HERE = os.path.dirname(os.path.abspath(__file__))


def build(cfg, size):
    """the model with its frozen provider; lpips.disc_start turns from a fraction into a step count (reference :370)"""
    cfg.lpips.disc_start = int(cfg.lpips.disc_start * cfg.trainer.total_train_steps)
    return with_provider(Model)(cfg, size)


def main(argv=None):
    return run(HERE, argv, build, rate="frames_per_s", state=model_state)


if __name__ == "__main__":
    sys.exit(main())
