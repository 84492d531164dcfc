"""Residual autoencoder `ae_gan` on MI355X, evaluation only: the reference's experiments/v1_experiments/ae_gan/train.py
without Lightning / W&B — `ConvAutoencoderBIG` on 128 x 128 SEVIR frames, scored with the test step of its `Model` (L1
reconstruction loss and the calc_metrics keys).

    python -m weatherforecastingtoolkit_amd.experiments.v1_experiments.ae_gan.train [--mode test] key=value ...

`model.checkpoint` names a state dict or a Lightning checkpoint of the reference's run (`autoencoder.*` is loaded,
`loss.discriminator.*` / `loss.perceptual_loss.*` ignored); without it the seeded initialisation is evaluated.  The
classes live in ../_ae_gan.py, the driver in ../_runner.py.  This entry point is forward-only: `--mode fit` is refused
here, training is ./fit.py.
"""
from __future__ import annotations

import os
import sys

from ...._lib import WfaeError
from .._ae_gan import FOLLOW_UP, ConvAutoencoder, ConvAutoencoderBIG, Model, ResidualBlock, UpsampleBlock  # noqa: F401
from .._runner import run

HERE = os.path.dirname(os.path.abspath(__file__))


def build(cfg, size):
    """lpips.disc_start turns from a fraction into a step count (reference :568)"""
    cfg.lpips.disc_start = int(cfg.lpips.disc_start * cfg.trainer.total_train_steps)
    return Model(cfg)


def mode_of(argv):
    """the value of --mode on the command line, "test" without one"""
    argv = list(sys.argv[1:] if argv is None else argv)
    for i, a in enumerate(argv):
        if a == "--mode" and i + 1 < len(argv):
            return argv[i + 1]
        if a.startswith("--mode="):
            return a.split("=", 1)[1]
    return "test"


def main(argv=None):
    if mode_of(argv) == "fit":      # before the driver opens the device
        raise WfaeError("ae_gan.train --mode fit: this entry point is forward-only; train with "
                        "`python -m weatherforecastingtoolkit_amd.experiments.v1_experiments.ae_gan.fit`")
    return run(HERE, argv, build, default_mode="test", rate="frames_per_s")


if __name__ == "__main__":
    try:
        sys.exit(main())
    except WfaeError as e:
        print(f"error: {e}", file=sys.stderr)
        sys.exit(2)
