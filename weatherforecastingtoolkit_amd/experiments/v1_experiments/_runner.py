"""What the v1 latent experiments (linear, DLinear, conv autoencoder, statistics MLP) share on the host: the optimiser
side of a `Model` (`Step`) and the command-line driver of every `*/train.py` (`run`).  The experiments keep what differs:
their networks, losses, validation / test steps and checkpoint spelling.
"""
from __future__ import annotations

import argparse
import json
import os
import time

import torch

from ... import config as C
from ... import parallel, synth
from ..._lib import WfaeError
from ...pipeline import helpers
from ...pipeline.datasets.sevire.sevir import SEVIRFrameLoader
from ._latents import Autoencoder


class Step:
    """mix-in of the four `Model` classes (next to nn.Module): AdamW + cosine warmup on the sub-module named by
    `trained`, the optimiser tail of `training_step`, and the batch preamble.  Uses `cfg`, `total_steps` and, for the
    preamble, `autoencoder` of the class it is mixed into."""

    trained = "predictor"        # the attribute that holds the trained sub-module
    exact_complements = False    # see optim.FusedAdamW

    def configure_optimizers(self):
        o, sp = self.cfg.optim, self.cfg.cosine_warmup
        net = getattr(self, self.trained)
        self.opt = helpers.adamw_optimizer(net, o.lr, o.weight_decay, exact_complements=self.exact_complements)
        self.sch = helpers.cosine_warmup_scheduler(self.opt, sp.start_lr, sp.final_lr, sp.peak_lr, self.total_steps,
                                                   sp.warmup_ratio * self.total_steps)
        self._dp = parallel.DataParallelTrainer(net, self.opt)
        return self.opt

    def optimizer_step(self, loss):
        """backward, gradient all-reduce, clip at optim.gradient_clip_val, AdamW, schedule
        -> (loss, gradient norm before clipping)"""
        loss.backward()
        self._dp.reduce_gradients()
        gn = self.opt.clip_grad_norm_(self.cfg.optim.gradient_clip_val)
        self.opt.step()
        self.sch.step()
        self.opt.zero_grad(set_to_none=True)
        return loss.detach(), gn

    def frames_latents(self, batch):
        """batch (a tensor, or the loader's dict): frames (B, T, H, W) fp32 in [0, 1] ('NTHW') or latents (B, T, C, h, w)
        -> (frames (B, T, 1, H, W) or None, latents (B, T, C, h, w))"""
        if isinstance(batch, dict):
            batch = batch["vil"]
        if batch.dim() == 4:
            if self.autoencoder is None:
                raise WfaeError("a batch of frames (B, T, H, W) needs the frozen autoencoder; pass latents "
                                "(B, T, C, h, w) or construct Model(cfg, autoencoder=...)")
            frames = batch.unsqueeze(2)
            return frames, self.autoencoder.encode(frames)
        return None, batch


def total_steps(n_batches, max_epochs, accumulate_grad_batches, max_steps=-1, mode="fit"):
    """steps of a run over a loader of `n_batches`: the reference's optimiser-step count when fitting, one pass when
    testing; `--max-steps` shortens it, and never lengthens it"""
    total = n_batches if mode == "test" else max(1, int(n_batches * max_epochs / accumulate_grad_batches))
    return max_steps if 0 < max_steps < total else total


def checkpoint(state, step):
    """the dictionary `last.ckpt` holds: host copies of `state` (key -> tensor) that share no memory with the model"""
    return {"state_dict": {k: v.detach().cpu().clone() for k, v in state.items()}, "global_step": step}


def predictor_state(model):
    """`predictor.`-prefixed state of the predictor, the reference's Lightning key layout"""
    return {"predictor." + k: v for k, v in model.predictor.state_dict().items()}


def with_provider(model_cls):
    """-> build(cfg, size): the model with the frozen latent provider its `autoencoder:` block describes"""
    return lambda cfg, size: model_cls(cfg, autoencoder=Autoencoder(size, cfg.autoencoder.kind, cfg.autoencoder))


# samples per step and rank behind the rate field of a log line
RATES = {"sequences_per_s": lambda d: d.batch_size, "frames_per_s": lambda d: d.batch_size * d.seq_len}


def run(here, argv, build, *, default_mode=None, layout=lambda cfg: "NTHW", rate="sequences_per_s",
        state=predictor_state):
    """driver of an experiment in directory `here` on synthetic blob events: `fit` trains `build(cfg, size)` (AdamW,
    cosine warmup, clip), prints a JSON line every trainer.log_every_n_steps steps and writes `last.ckpt` with
    `state(model)`; `--mode test` — offered only where `default_mode` is given — runs test_step over the loader"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=os.path.join(here, "config.yaml"))
    ap.add_argument("--max-steps", type=int, default=-1)
    if default_mode is not None:
        ap.add_argument("--mode", choices=("fit", "test"), default=default_mode)
    args, unknown = ap.parse_known_args(argv)
    mode = getattr(args, "mode", "fit")
    cfg = C.load(args.config)
    cli = C.from_dotlist(unknown)
    helpers.check_yaml(cfg, cli)
    cfg = C.merge(cfg, cli)
    rank, world, local = parallel.init_from_env()
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    size, frames = (384, 49) if cfg.dataset.name == "sevir" else (128, 25)
    events = synth.blob_events(max(2, cfg.dataset.batch_size * 2 * world), size, frames, seed=1234)
    loader = SEVIRFrameLoader(events, cfg.dataset.batch_size, cfg.dataset.seq_len, cfg.dataset.stride, layout(cfg),
                              shuffle=mode == "fit", device=dev, num_shard=world, rank=rank)
    total = total_steps(len(loader), cfg.trainer.max_epochs, cfg.trainer.accumulate_grad_batches, args.max_steps, mode)
    cfg.trainer.total_train_steps = total
    torch.manual_seed(0)
    model = build(cfg, size).to(dev).train()
    if getattr(model, "autoencoder", None) is not None:
        model.autoencoder.eval()
    step = 0
    if mode == "test":
        model.eval()
        for batch in loader:
            if step >= total:
                break
            loss, logs = model.test_step(batch["vil"], step)
            step += 1
            if rank == 0:
                print(json.dumps({"step": step, **{k: float(v) for k, v in logs.items()}}), flush=True)
        if rank == 0:
            print("done")
        return 0
    model.configure_optimizers()
    per_step = RATES[rate](cfg.dataset) * world
    t0 = time.time()
    while step < total:
        for batch in loader:
            if step >= total:
                break
            loss, gn = model.training_step(batch["vil"])
            step += 1
            if rank == 0 and step % max(1, cfg.trainer.log_every_n_steps) == 0:
                print(json.dumps({"step": step, "train_loss": float(loss), "grad_norm": float(gn),
                                  "lr": model.opt.param_groups[0]["lr"],
                                  rate: step * per_step / (time.time() - t0)}), flush=True)
    if rank == 0:
        out = os.path.join(cfg.experiment_path, "outputs", cfg.experiment_name, "checkpoints")
        os.makedirs(out, exist_ok=True)
        torch.save(checkpoint(state(model), step), os.path.join(out, "last.ckpt"))
        print("done")
    return 0
