"""Conv latent autoencoder `pretrained_ae_convae_sevir` on MI355X: the predictor step of the reference's
experiments/v1_experiments/pretrained_ae_convae_sevir/train.py without Lightning / W&B — frozen-autoencoder latents are
auto-encoded by a small conv network (conv + LayerNorm over the sample + LeakyReLU units) under a Huber loss.

    python -m weatherforecastingtoolkit_amd.experiments.v1_experiments.pretrained_ae_convae_sevir.train [--mode fit|test] key=value ...

The default mode is `fit`, as the reference's `__main__` calls `trainer.fit`.  The classes live in ../_convae.py, the
driver in ../_runner.py.
"""
from __future__ import annotations

import os
import sys

from .._convae import Autoencoder, ConvDecoder, ConvEncoder, ConvModel, Model  # noqa: F401
from .._runner import run, with_provider

HERE = os.path.dirname(os.path.abspath(__file__))


def main(argv=None):
    return run(HERE, argv, with_provider(Model), default_mode="fit", rate="frames_per_s")


if __name__ == "__main__":
    sys.exit(main())
