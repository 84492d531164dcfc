"""Intensity-statistics MLP forecaster `prediff_mlp_sevir` on MI355X: the step of the reference's
experiments/v1_experiments/prediff_mlp_sevir/train.py without Lightning / W&B — per-frame mean intensities of 5 input
frames -> Linear(5, 128)-ReLU-Linear(128, 128)-ReLU-Linear(128, 8) -> mean and std of 4 runs of 5 target frames.

    python -m weatherforecastingtoolkit_amd.experiments.v1_experiments.prediff_mlp_sevir.train [--max-steps N] key=value ...

MLP and Model live in ../_prediff_mlp.py, the driver in ../_runner.py.
"""
from __future__ import annotations

import os
import sys

from .._prediff_mlp import MLP, Model  # noqa: F401
from .._runner import run

HERE = os.path.dirname(os.path.abspath(__file__))


def main(argv=None):
    return run(HERE, argv, lambda cfg, size: Model(cfg), layout=lambda cfg: cfg.dataset.layout,
               state=lambda model: model.state_dict())


if __name__ == "__main__":
    sys.exit(main())
