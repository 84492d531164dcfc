"""Intensity-statistics MLP forecaster of the reference's v1 experiments:
experiments/v1_experiments/prediff_mlp_sevir/train.py without Lightning / W&B / torch.compile.

Reference (:20-38, :56-70): from a raw 'NHWT' batch (B, H, W, 25) the mean intensity of each of the 5 input frames is
the MLP input (B, 5); the 20 target frames, cut into 4 runs of 5, give the target (B, 8) — the 4 run means, then the 4
unbiased run standard deviations; Linear(5, 128)-ReLU-Linear(128, 128)-ReLU-Linear(128, 8), MSE, AdamW, cosine warmup,
clip 1.0.

Here a training step is: one read of the batch for all 13 statistics (two launches of csrc/prediff.hip, in the memory
order the loader delivers, no copy), one launch for the MLP forward + loss + all six gradients, then scale, clip and
AdamW over the flat arenas.  `torch.compile` only renames the reference's checkpoint keys (`model._orig_mod.mlp.N.*`):
state_dict() writes that spelling, load_state_dict() takes it and the plain `model.mlp.N.*`.  The optimiser step and
the driver are the v1 experiments' shared ones (./_runner.py).
"""
from __future__ import annotations

from collections import OrderedDict

import torch
import torch.nn as tnn

from ... import functional as Fn
from ... import nn as wnn
from ... import ops
from ..._lib import WfaeError
from ._runner import Step

GROUPS = 4   # the reference's `reshape(b, 4, t // 4, -1)`
_COMPILED = "model._orig_mod."


class MLP(tnn.Module):
    """reference :20-38: B, 5 -> B, 8.  The submodules are built by the same constructors in the same order as the
    reference's nn.Sequential, so after the same torch.manual_seed every initial value is bit-identical and the
    state_dict keys are `mlp.{0,2,4}.{weight,bias}`; forward is one launch, not five modules."""

    def __init__(self, inp_seq_len=5, out_var_len=8, hidden_dim=128):
        super().__init__()
        self.inp_seq_len, self.out_var_len, self.hidden_dim = inp_seq_len, out_var_len, hidden_dim
        self.mlp = tnn.Sequential(
            wnn.Linear(inp_seq_len, hidden_dim),
            tnn.ReLU(),
            wnn.Linear(hidden_dim, hidden_dim),
            tnn.ReLU(),
            wnn.Linear(hidden_dim, out_var_len),
        )

    def parameters_in_order(self):
        m = self.mlp
        return (m[0].weight, m[0].bias, m[2].weight, m[2].bias, m[4].weight, m[4].bias)

    def _check(self, x):
        if x.dim() != 2 or x.shape[1] != self.inp_seq_len:
            raise WfaeError(f"MLP: expected (batch, {self.inp_seq_len}), got {tuple(x.shape)}")

    def forward(self, x):
        self._check(x)
        return Fn.mlp3(x, *self.parameters_in_order())

    def loss(self, x, target):
        """-> (F.mse_loss(self(x), target), pred), with the parameter gradients attached to the loss"""
        self._check(x)
        return Fn.mlp3_mse_loss(x, target, *self.parameters_in_order())


class Model(Step, tnn.Module):
    """reference Model (:40-95): `model` (the MLP), forward, the training / validation steps; the optimiser is `Step`'s,
    on `model`"""

    trained = "model"

    def __init__(self, cfg, mlp=None):
        super().__init__()
        self.cfg = cfg
        self.model = mlp if mlp is not None else MLP()
        self.input_frames, self.pred_frames = int(cfg.dataset.input_frames), int(cfg.dataset.pred_frames)
        self.total_steps = cfg.trainer.total_train_steps
        if self.input_frames != self.model.inp_seq_len:
            raise WfaeError(f"dataset.input_frames = {self.input_frames} must equal the MLP's input width "
                            f"{self.model.inp_seq_len} (one mean intensity per input frame)")
        if int(cfg.dataset.seq_len) != self.input_frames + self.pred_frames:
            raise WfaeError(f"dataset.seq_len = {cfg.dataset.seq_len} must equal input_frames + pred_frames = "
                            f"{self.input_frames} + {self.pred_frames}")
        if self.pred_frames <= 0 or self.pred_frames % GROUPS:
            raise WfaeError(f"dataset.pred_frames = {self.pred_frames} must be a positive multiple of {GROUPS}: the "
                            f"target is the mean and std of {GROUPS} runs of whole frames")
        if self.model.out_var_len != 2 * GROUPS:
            raise WfaeError(f"the MLP's output width {self.model.out_var_len} must be {2 * GROUPS} "
                            f"({GROUPS} means and {GROUPS} stds)")

    # -- checkpoint spelling of the reference (`self.model = torch.compile(self.model)`) ---------------------------
    def state_dict(self, *args, **kwargs):
        sd = super().state_dict(*args, **kwargs)
        prefix = kwargs.get("prefix", args[1] if len(args) > 1 else "")
        out = OrderedDict()
        for k, v in sd.items():
            head = prefix + "model."
            out[prefix + _COMPILED + k[len(head):] if k.startswith(head) else k] = v
        if hasattr(sd, "_metadata"):
            out._metadata = sd._metadata
        return out

    def load_state_dict(self, state_dict, strict=True, **kwargs):
        plain = OrderedDict((("model." + k[len(_COMPILED):]) if k.startswith(_COMPILED) else k, v)
                            for k, v in state_dict.items())
        return super().load_state_dict(plain, strict=strict, **kwargs)

    def forward(self, x):
        return self.model(x)

    def statistics(self, batch):
        """'NHWT' batch (B, H, W, T) -> (input intensities (B, input_frames), target (B, 8))"""
        if isinstance(batch, dict):
            batch = batch["vil"]
        if batch.dim() != 4 or batch.shape[3] != self.input_frames + self.pred_frames:
            raise WfaeError(f"expected an 'NHWT' batch (B, H, W, {self.input_frames + self.pred_frames}), got "
                            f"{tuple(batch.shape)}")
        return ops.seq_intensity_stats(batch, self.input_frames, GROUPS)

    def training_step(self, batch, batch_idx=0):
        """batch: 'NHWT' frames (B, H, W, T) fp32 in [0, 1]; AdamW + cosine warmup, clip 1.0 -> (loss, grad norm)"""
        x, target = self.statistics(batch)
        loss, _ = self.model.loss(x, target)
        return self.optimizer_step(loss)

    @torch.no_grad()
    def validation_step(self, batch, batch_idx=0):
        """-> val_loss (reference :72-84)"""
        x, target = self.statistics(batch)
        return ops.mlp3_mse(x, target, *[p.detach() for p in self.model.parameters_in_order()])[1]
