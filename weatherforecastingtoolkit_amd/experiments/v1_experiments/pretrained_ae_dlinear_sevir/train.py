"""DLinear latent forecaster `pretrained_ae_dlinear_sevir` on MI355X: the predictor step of the
reference's experiments/v1_experiments/pretrained_ae_dlinear_sevir/train.py without Lightning / W&B — one shared Linear(13 -> 12) over time for seasonal and one for trend.

    python -m weatherforecastingtoolkit_amd.experiments.v1_experiments.pretrained_ae_dlinear_sevir.train [--mode fit|test] key=value ...

The default mode is `test`, as the reference's `__main__` calls `trainer.test`.  Model, DLinear, moving_avg and
series_decomp are shared by the three DLinear experiments (../_dlinear.py); the driver is ../_runner.py.
"""
from __future__ import annotations

import os
import sys

from .._dlinear import Autoencoder, DLinear, Model, moving_avg, series_decomp  # noqa: F401
from .._runner import run, with_provider

HERE = os.path.dirname(os.path.abspath(__file__))


def main(argv=None):
    return run(HERE, argv, with_provider(Model), default_mode="test")


if __name__ == "__main__":
    sys.exit(main())
