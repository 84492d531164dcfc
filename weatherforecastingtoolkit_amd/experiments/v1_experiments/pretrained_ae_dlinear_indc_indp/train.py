"""DLinear latent forecaster `pretrained_ae_dlinear_indc_indp` on MI355X: the predictor step of the
reference's experiments/v1_experiments/pretrained_ae_dlinear_indc_indp/train.py without Lightning / W&B — a separate Linear(13*C -> 12*C) pair for each latent pixel.

    python -m weatherforecastingtoolkit_amd.experiments.v1_experiments.pretrained_ae_dlinear_indc_indp.train [--mode fit|test] key=value ...

The default mode is `fit`, as the reference's `__main__` calls `trainer.fit`.  Model, DLinear, moving_avg and
series_decomp are shared by the three DLinear experiments (../_dlinear.py); the driver is ../_runner.py.
"""
from __future__ import annotations

import functools
import os
import sys

from .._dlinear import Autoencoder, DLinear, Model, moving_avg, series_decomp  # noqa: F401
from .._runner import run, with_provider

HERE = os.path.dirname(os.path.abspath(__file__))


def main(argv=None):
    return run(HERE, argv, with_provider(functools.partial(Model, plots="indc_indp")), default_mode="fit")


if __name__ == "__main__":
    sys.exit(main())
