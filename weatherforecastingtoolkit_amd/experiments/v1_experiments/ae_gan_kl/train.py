"""KL autoencoder with a GAN loss `ae_gan_kl` on MI355X: the reference's experiments/v1_experiments/ae_gan_kl/train.py
without Lightning / W&B — the AutoencoderKL itself is trained on 128 x 128 SEVIR frames under L1 / SSIM as a negative
log-likelihood plus the KL term, joined from `lpips.disc_start` (a fraction of the total steps) by a PatchGAN.

    python -m weatherforecastingtoolkit_amd.experiments.v1_experiments.ae_gan_kl.train key=value ...

The classes live in ../_ae_gan_kl.py, the driver in ../_runner.py.  `last.ckpt` holds `autoencoder.*`,
`loss.discriminator.*` and `loss.logvar`.
"""
from __future__ import annotations

import os
import sys

from .._ae_gan_kl import Loss, Model, load_model_state, model_state  # noqa: F401
from .._runner import run

HERE = os.path.dirname(os.path.abspath(__file__))


def build(cfg, size):
    """lpips.disc_start turns from a fraction into a step count (reference :279)"""
    cfg.lpips.disc_start = int(cfg.lpips.disc_start * cfg.trainer.total_train_steps)
    return Model(cfg)


def main(argv=None):
    return run(HERE, argv, build, rate="frames_per_s", state=model_state)


if __name__ == "__main__":
    sys.exit(main())
