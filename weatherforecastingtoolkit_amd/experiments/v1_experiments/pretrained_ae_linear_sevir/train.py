"""Path-B linear latent forecaster on MI355X: the predictor step of the reference's
experiments/v1_experiments/pretrained_ae_linear_sevir/train.py without Lightning / W&B.

    python -m weatherforecastingtoolkit_amd.experiments.v1_experiments.pretrained_ae_linear_sevir.train key=value ...

Reference step (:73-83): latents v (B,T,C,h,w) of a frozen autoencoder; inp = v[:, :Tin] - v[:, Tin-1],
tgt = v[:, Tin:] - v[:, Tin-1]; pred = Linear(Tin*C -> Tout*C) applied per latent pixel on the
(b,h,w,Tin*C) layout; loss = mse(pred, tgt); AdamW + cosine-warmup on the predictor only, clip 1.0 (:189).
Here: one differencing/layout kernel, one MFMA GEMM (+ its weight-gradient GEMM), one MSE kernel.
The frozen AutoencoderKL of the reference (pretrained checkpoint, not available) is replaced by a pluggable
latent provider (../_latents.py); by default the frozen `enc` stack of the ae_v2 conv autoencoder.  The optimiser step
and the driver are the v1 experiments' shared ones (../_runner.py).
"""
from __future__ import annotations

import os
import sys

import torch
import torch.nn as tnn

from .... import functional as Fn
from .... import nn as wnn
from .... import ops
from .._latents import Autoencoder  # noqa: F401  (the frozen latent provider)
from .._runner import Step, run, with_provider

HERE = os.path.dirname(os.path.abspath(__file__))


class Model(Step, tnn.Module):
    """reference Model (:58-134): `predictor`, `forward` and the training step; the optimiser is `Step`'s"""

    def __init__(self, cfg, latent_channels=None, autoencoder=None):
        super().__init__()
        self.cfg = cfg
        self.autoencoder = autoencoder
        self.input_frames, self.pred_frames = cfg.dataset.input_frames, cfg.dataset.pred_frames
        c = latent_channels if latent_channels is not None else cfg.autoencoder.latent_channels
        self.latent_channels = c
        self.predictor = wnn.Linear(self.input_frames * c, self.pred_frames * c)
        self.total_steps = cfg.trainer.total_train_steps

    def forward(self, x):
        return self.predictor(x)

    def latent_loss(self, v):
        """v (B,T,C,h,w) latents -> (loss, pred (B*h*w, Tout*C)) — reference :75-82"""
        X, Y = ops.latent_diff_pack(v.contiguous(), self.input_frames)
        pred = self(X)
        return Fn.mse_loss(pred, Y), pred

    def predict_latents(self, v):
        """forecast latents (B,Tout,C,h,w) = pred + last input frame (reference :86-87)"""
        X, _ = ops.latent_diff_pack(v.contiguous(), self.input_frames)
        with torch.no_grad():
            return ops.latent_unpack_add(self(X).contiguous(), v.contiguous(), self.input_frames)

    def training_step(self, batch, batch_idx=0):
        """batch: frames (B,T,H,W) fp32 in [0,1] ('NTHW') or latents (B,T,C,h,w)"""
        _, v = self.frames_latents(batch)
        loss, _ = self.latent_loss(v)
        return self.optimizer_step(loss)


def main(argv=None):
    return run(HERE, argv, with_provider(Model))


if __name__ == "__main__":
    sys.exit(main())
