"""Intensity-statistics MLP forecaster of the reference's v1 experiments:
experiments/v1_experiments/prediff_mlp_sevir/train.py without Lightning / W&B / torch.compile.

Reference (:20-38, :56-70): from a raw 'NHWT' batch (B, H, W, 25) the mean intensity of each of the 5 input frames is
the MLP input (B, 5); the 20 target frames, cut into 4 runs of 5, give the target (B, 8) — the 4 run means, then the 4
unbiased run standard deviations; Linear(5, 128)-ReLU-Linear(128, 128)-ReLU-Linear(128, 8), MSE, AdamW, cosine warmup,
clip 1.0.

Here a training step is: one read of the batch for all 13 statistics (two launches of csrc/prediff.hip, in the memory
order the loader delivers, no copy), one launch for the MLP forward + loss + all six gradients, then scale, clip and
AdamW over the flat arenas.  `torch.compile` only renames the reference's checkpoint keys (`model._orig_mod.mlp.N.*`):
state_dict() writes that spelling, load_state_dict() takes it and the plain `model.mlp.N.*`.
"""
from __future__ import annotations

import argparse
import json
import os
import time
from collections import OrderedDict

import torch
import torch.nn as tnn

from ... import config as C
from ... import functional as Fn
from ... import nn as wnn
from ... import ops, parallel, synth
from ..._lib import WfaeError
from ...pipeline import helpers
from ...pipeline.datasets.sevire.sevir import SEVIRFrameLoader

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


class Model(tnn.Module):
    """reference Model (:40-95): `model` (the MLP), forward, the training / validation steps and the optimiser"""

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

    def configure_optimizers(self):
        o, sp = self.cfg.optim, self.cfg.cosine_warmup
        self.opt = helpers.adamw_optimizer(self.model, o.lr, o.weight_decay)
        self.sch = helpers.cosine_warmup_scheduler(self.opt, sp.start_lr, sp.final_lr, sp.peak_lr, self.total_steps,
                                                   sp.warmup_ratio * self.total_steps)
        self._dp = parallel.DataParallelTrainer(self.model, self.opt)
        return self.opt

    def training_step(self, batch, batch_idx=0):
        """batch: 'NHWT' frames (B, H, W, T) fp32 in [0, 1]; AdamW + cosine warmup, clip 1.0 -> (loss, grad norm)"""
        x, target = self.statistics(batch)
        loss, _ = self.model.loss(x, target)
        loss.backward()
        self._dp.reduce_gradients()
        gn = self.opt.clip_grad_norm_(self.cfg.optim.gradient_clip_val)
        self.opt.step()
        self.sch.step()
        self.opt.zero_grad(set_to_none=True)
        return loss.detach(), gn

    @torch.no_grad()
    def validation_step(self, batch, batch_idx=0):
        """-> val_loss (reference :72-84)"""
        x, target = self.statistics(batch)
        return ops.mlp3_mse(x, target, *[p.detach() for p in self.model.parameters_in_order()])[1]


def main(here, argv=None):
    """`fit` of the reference's `__main__`: trains on synthetic blob events through the 'NHWT' loader and writes
    `last.ckpt` in the reference's key layout"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=os.path.join(here, "config.yaml"))
    ap.add_argument("--max-steps", type=int, default=-1)
    args, unknown = ap.parse_known_args(argv)
    cfg = C.load(args.config)
    cli = C.from_dotlist(unknown)
    helpers.check_yaml(cfg, cli)
    cfg = C.merge(cfg, cli)
    rank, world, local = parallel.init_from_env()
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    size, frames = (384, 49) if cfg.dataset.name == "sevir" else (128, 25)
    events = synth.blob_events(max(2, cfg.dataset.batch_size * 2 * world), size, frames, seed=1234)
    loader = SEVIRFrameLoader(events, cfg.dataset.batch_size, cfg.dataset.seq_len, cfg.dataset.stride,
                              cfg.dataset.layout, shuffle=True, device=dev, num_shard=world, rank=rank)
    total = max(1, int(len(loader) * cfg.trainer.max_epochs / cfg.trainer.accumulate_grad_batches))
    if 0 < args.max_steps < total:
        total = args.max_steps
    cfg.trainer.total_train_steps = total
    torch.manual_seed(0)
    model = Model(cfg).to(dev).train()
    model.configure_optimizers()
    step, t0 = 0, time.time()
    while step < total:
        for batch in loader:
            if step >= total:
                break
            loss, gn = model.training_step(batch["vil"])
            step += 1
            if rank == 0 and step % max(1, cfg.trainer.log_every_n_steps) == 0:
                print(json.dumps({"step": step, "train_loss": float(loss), "grad_norm": float(gn),
                                  "lr": model.opt.param_groups[0]["lr"],
                                  "sequences_per_s": step * cfg.dataset.batch_size * world / (time.time() - t0)}),
                      flush=True)
    if rank == 0:
        out = os.path.join(cfg.experiment_path, "outputs", cfg.experiment_name, "checkpoints")
        os.makedirs(out, exist_ok=True)
        torch.save({"state_dict": {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
                    "global_step": step}, os.path.join(out, "last.ckpt"))
        print("done")
    return 0
