"""Training the residual autoencoder `ae_gan` on MI355X: the reference's experiments/v1_experiments/ae_gan/train.py without
Lightning / W&B, below `lpips.disc_start` — the run its shipped config does (disc_start 1.0 of the total steps, disc_weight
0, perceptual_weight 0): L1 on `ConvAutoencoderBIG` with AdamW, cosine warmup and gradient clipping.

    python -m weatherforecastingtoolkit_amd.experiments.v1_experiments.ae_gan.fit [--max-steps N] key=value ...

Prints a JSON line every trainer.log_every_n_steps steps and writes `last.ckpt` with `autoencoder.*` keys, which
`model.checkpoint=` of ./train.py reads back.  The discriminator branch (a `disc_start` below 1) is refused.  The classes
live in ../_ae_gan.py, the driver in ../_runner.py.
"""
from __future__ import annotations

import os
import sys

from ...._lib import WfaeError
from .._ae_gan import Model, model_state
from .._runner import run

HERE = os.path.dirname(os.path.abspath(__file__))


def build(cfg, size):
    """lpips.disc_start turns from a fraction into a step count (reference :568); a run that would reach it is refused
    before anything is trained"""
    total = cfg.trainer.total_train_steps
    cfg.lpips.disc_start = int(cfg.lpips.disc_start * total)
    if cfg.lpips.disc_start < total:
        raise WfaeError(f"ae_gan fit: lpips.disc_start = step {cfg.lpips.disc_start} of {total}: the discriminator branch of "
                        "the loss is not built; the shipped config (disc_start: 1.0) never reaches it")
    return Model(cfg, trainable=True)


def check_args(argv):
    """--mode belongs to ./train.py (evaluation): refused here, before the driver opens the device"""
    argv = list(sys.argv[1:] if argv is None else argv)
    if any(a == "--mode" or a.startswith("--mode=") for a in argv):
        raise WfaeError("ae_gan.fit takes no --mode: it trains; evaluation is `python -m ...ae_gan.train --mode test`")
    return argv


def main(argv=None):
    return run(HERE, check_args(argv), build, rate="frames_per_s", state=model_state)


if __name__ == "__main__":
    try:
        sys.exit(main())
    except WfaeError as e:
        print(f"error: {e}", file=sys.stderr)
        sys.exit(2)
