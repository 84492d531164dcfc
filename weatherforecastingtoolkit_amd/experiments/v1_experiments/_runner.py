"""What the v1 latent experiments (linear, DLinear, conv autoencoder, statistics MLP) share on the host: the optimiser
side of a `Model` (`Step`) and the command-line driver of every `*/train.py` (`run`).  The experiments keep what differs:
their networks, losses, validation / test steps and checkpoint spelling.

Opt-in by flag, the driver also runs on real SEVIR (`--data-dir`), validates (`--validate`, or with `--data-dir`), tests
after the fit (`--test`), checkpoints during the run and resumes (`--resume`, `--stop-after`).  Which loader an experiment
reads real data through is decided by what its reference `train.py` imports (`loader_path`).
"""
from __future__ import annotations

import argparse
import datetime
import json
import os
import sys
import time

import torch

from ... import config as C
from ... import functional as Fn
from ... import ops, parallel, synth
from ..._lib import WfaeError
from ...pipeline import helpers
from ...pipeline.datasets.sevir.sevir import SEVIRLightningDataModule
from ...pipeline.datasets.sevire.sevir import SEVIRFrameLoader, parse_presample, presample_line, resolve_presample
from ..ae_v2.train import _mean_logs
from ._latents import Autoencoder


class Step:
    """mix-in of the four `Model` classes (next to nn.Module): AdamW + cosine warmup on the sub-module named by
    `trained`, the optimiser tail of `training_step`, and the batch preamble.  Uses `cfg`, `total_steps` and, for the
    preamble, `autoencoder` of the class it is mixed into."""

    trained = "predictor"        # the attribute that holds the trained sub-module
    panels = None                # helpers.PanelSink with `--plots DIR` on rank 0: the steps that plot draw into it
    verification = None          # metrics.LeadVerification with `--verify`: the validation / test steps add to it
    exact_complements = False    # see optim.FusedAdamW
    batch_ids = None             # with `--latent-cache`: (split, frame ids) of the loader batch the driver hands to a step

    def configure_optimizers(self):
        o, sp = self.cfg.optim, self.cfg.cosine_warmup
        net = getattr(self, self.trained)
        # optim.beta1 / beta2: ae_s2's config names them (reference ae_s2/train.py:220-221); the defaults are AdamW's
        self.opt = helpers.adamw_optimizer(net, o.lr, o.weight_decay, beta1=o.get("beta1", 0.9), beta2=o.get("beta2", 0.999),
                                           exact_complements=self.exact_complements)
        self.sch = helpers.cosine_warmup_scheduler(self.opt, sp.start_lr, sp.final_lr, sp.peak_lr, self.total_steps,
                                                   sp.warmup_ratio * self.total_steps)
        self._dp = parallel.DataParallelTrainer(net, self.opt)
        return self.opt

    def optimizers(self):
        """[(optimiser, schedule), ...] in the order a checkpoint lists them; the two-optimiser models add their
        discriminator's pair"""
        return [(self.opt, self.sch)]

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
            if self.batch_ids is not None:
                return frames, self.autoencoder.encode(frames, ids=self.batch_ids)
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


def resume_state(model, epoch):
    """what `last.ckpt` holds next to `checkpoint()`'s two keys so that `--resume` continues the run: the state of every
    (optimiser, schedule) pair of `model.optimizers()` in its order, the epoch, the generators and the dropout counter,
    and the model's own `global_step` where it keeps one"""
    pairs = model.optimizers()
    out = {"optimizer_states": [o.state_dict() for o, _ in pairs], "lr_schedulers": [s.state_dict() for _, s in pairs],
           "epoch": int(epoch),
           "rng": {"torch_state": torch.get_rng_state(),
                   "cuda_state": torch.cuda.get_rng_state() if torch.cuda.is_available() else None,
                   "dropout_counter": Fn._seed_counter[0]}}
    if hasattr(model, "global_step"):
        out["model_global_step"] = int(model.global_step)
    return out


def load_resume_state(model, ck):
    """the inverse of `resume_state` on a loaded checkpoint -> epoch.  A checkpoint without optimiser state (written
    before the driver kept it) restarts the moments: the first schedule continues at `global_step`, any further pair
    restarts with its moments"""
    pairs, step = model.optimizers(), int(ck.get("global_step", 0))
    if ck.get("optimizer_states"):
        if len(ck["optimizer_states"]) != len(pairs) or len(ck.get("lr_schedulers") or ()) != len(pairs):
            raise ValueError(f"checkpoint holds {len(ck['optimizer_states'])} optimiser states and "
                             f"{len(ck.get('lr_schedulers') or ())} schedules, the model has {len(pairs)} of each")
        for (opt, sch), o, s in zip(pairs, ck["optimizer_states"], ck["lr_schedulers"]):
            opt.load_state_dict(o)
            sch.load_state_dict(s)
    else:
        print("checkpoint holds no optimiser state: AdamW moments restart from zero", file=sys.stderr)
        pairs[0][1].load_state_dict({"last_epoch": step})
    rng = ck.get("rng")
    if rng:
        torch.set_rng_state(rng["torch_state"])
        if rng.get("cuda_state") is not None and torch.cuda.is_available():
            torch.cuda.set_rng_state(rng["cuda_state"])
        Fn._seed_counter[0] = rng["dropout_counter"]
    if hasattr(model, "global_step"):
        model.global_step = int(ck.get("model_global_step", step))
    return int(ck.get("epoch", 0))


def load_state(live, saved):
    """copy `saved` (key -> tensor, a checkpoint's state_dict) into `live`, the experiment's `state(model)`: its tensors
    are views of the parameters and buffers, so the copy lands in the model and in the optimiser's arena; the key sets
    must agree"""
    missing, extra = [k for k in live if k not in saved], [k for k in saved if k not in live]
    if missing or extra:
        raise ValueError(f"checkpoint state_dict does not fit the model: missing {missing[:4]}, unexpected {extra[:4]}")
    with torch.no_grad():
        for k, v in live.items():
            if tuple(v.shape) != tuple(saved[k].shape):
                raise ValueError(f"checkpoint state_dict: {k} has shape {tuple(saved[k].shape)}, the model {tuple(v.shape)}")
            v.copy_(saved[k])


def save_checkpoint(path, model, state, step, epoch):
    """`last.ckpt`: `checkpoint()`'s keys first, then `resume_state`'s; written to a temporary file and moved in place"""
    ck = checkpoint(state(model), step)
    ck.update(resume_state(model, epoch))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    torch.save(ck, path + ".tmp")
    os.replace(path + ".tmp", path)


def resume(path, model, state):
    """load `last.ckpt` at `path` into the model, its optimisers, schedules and generators -> the step the run continues
    from; without a file the run starts from scratch, at step 0"""
    if not os.path.exists(path):
        return 0
    ck = torch.load(path, map_location="cpu", weights_only=False)
    load_state(state(model), ck["state_dict"])
    load_resume_state(model, ck)
    return int(ck["global_step"])


def predictor_state(model):
    """`predictor.`-prefixed state of the predictor, the reference's Lightning key layout"""
    return {"predictor." + k: v for k, v in model.predictor.state_dict().items()}


def with_provider(model_cls):
    """-> build(cfg, size): the model with the frozen latent provider its `autoencoder:` block describes"""
    return lambda cfg, size: model_cls(cfg, autoencoder=Autoencoder(size, cfg.autoencoder.kind, cfg.autoencoder))


# samples per step and rank behind the rate field of a log line
RATES = {"sequences_per_s": lambda d: d.batch_size, "frames_per_s": lambda d: d.batch_size * d.seq_len}


def run(here, argv, build, *, default_mode=None, layout=lambda cfg: "NTHW", rate="sequences_per_s",
        state=predictor_state, test_after_fit=False):
    """driver of an experiment in directory `here`, on synthetic blob events or with `--data-dir` on a SEVIR store: `fit`
    trains `build(cfg, size)` (AdamW, cosine warmup, clip), prints a JSON line every trainer.log_every_n_steps steps and
    writes `last.ckpt` with `state(model)` and the resume state; `--mode test` — offered only where `default_mode` is
    given — runs test_step over the loader (the test split of a store).  With `--data-dir` or `--validate` a validation
    pass follows every training epoch and the last step; `--test` adds a test pass after the fit; with any of the new
    flags `last.ckpt` is also written every int(total steps * trainer.save_every_n_steps) steps, and `--resume`
    continues from it (`--stop-after N` is the interruption).  `test_after_fit`: the default of `--test` (ae_s2's
    `__main__` calls trainer.test after trainer.fit; `--no-test` leaves it out).  `--latent-cache FRAMES` keeps the frozen
    AutoencoderKL's latents on the device (`enable_latent_cache`): the training, validation and test-after-fit steps get
    their batch's frame ids in `model.batch_ids`, and one `latent_cache` line is printed in front of `done`; with
    `--mode test` the flag is refused.  `--invariant-encode` puts that provider into pass-invariant mode
    (`enable_invariant_encode`), with or without the cache.  `--verify` (`enable_verification`) gives the DLinear
    forecasters a `metrics.LeadVerification`: every validation / test pass, `--mode test` included, starts with empty
    tables and ends with one `verification` line after its own (`report_verification`); no other line changes"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=os.path.join(here, "config.yaml"))
    ap.add_argument("--max-steps", type=int, default=-1)
    if default_mode is not None:
        ap.add_argument("--mode", choices=("fit", "test"), default=default_mode)
    ap.add_argument("--data-dir", default=None, help="SEVIR root (CATALOG.csv + data/); default: synthetic events")
    ap.add_argument("--data-format", choices=("npy", "h5"), default="npy")
    ap.add_argument("--presample", type=parse_presample, default="auto", metavar="auto|none|T,H,W",
                    help="with --data-dir: pool the events on the device as the loader converts them.  auto = (2, 3, 3) "
                         "when the config names sevir_lr and the store holds raw 384x384x49 events, else none")
    ap.add_argument("--validate", action="store_true",
                    help="run the validation pass on synthetic events too (with --data-dir it always runs)")
    ap.add_argument("--test", action=argparse.BooleanOptionalAction, default=test_after_fit,
                    help="run the test loop after the fit")
    ap.add_argument("--matmul-precision", default="high", choices=["highest", "high", "medium"],
                    help="reference: torch.set_float32_matmul_precision('high').  'medium' = bf16 operands with fp32 "
                         "accumulation in the matrix-core kernels")
    ap.add_argument("--resume", action="store_true", help="continue from last.ckpt if there is one")
    ap.add_argument("--plots", default=None, metavar="DIR",
                    help="write target / prediction / difference panels of the steps that plot in the reference into "
                         "DIR as PNG files, with one line per figure in DIR/index.jsonl (rank 0)")
    ap.add_argument("--latent-cache", type=int, default=0, metavar="FRAMES",
                    help="keep the frozen AutoencoderKL's latents of up to FRAMES frames on the device, so that a frame is "
                         "encoded once per run and not once per epoch (each rank caches its own shard; a resumed run "
                         "refills it).  The run's numbers are bit for bit those without the flag: missing frames are "
                         "encoded in passes of the size the uncached encode uses, and a batch of another pass size (a "
                         "short last batch) goes around the cache; with --invariant-encode exactly the missing frames "
                         "are encoded and no batch goes around.  Fit only.  0 = off")
    ap.add_argument("--invariant-encode", action="store_true",
                    help="frozen AutoencoderKL providers: make a frame's latent the same bits whatever shares its encoder "
                         "pass (the attention projections run on the row-invariant linear kernel).  The latents differ "
                         "from the default mode's in the last bits.  With --latent-cache the cache then encodes exactly "
                         "the frames it misses, and serves short batches and tail chunks too")
    ap.add_argument("--verify", action="store_true",
                    help="DLinear forecasters: score the decoded forecast, persistence (the last input frame) and the "
                         "decoded target against the observed frames per lead time in every validation / test pass, and "
                         "print one `verification` line per pass: MSE, MAE, CSI, HSS per lead and field, the MSE skill "
                         "against persistence and the leads at which the forecast beats it")
    ap.add_argument("--stop-after", type=int, default=-1,
                    help="stop (and checkpoint) after this many optimiser steps without changing the schedule: an "
                         "interrupted run that --resume continues")
    args, unknown = ap.parse_known_args(argv)
    mode = getattr(args, "mode", "fit")
    if args.latent_cache and mode == "test":        # before the device is opened
        raise WfaeError("--latent-cache with --mode test: a test run is a single pass over the loader, no frame is met twice; "
                        "the flag belongs to a fit (its validation and test-after-fit passes included)")
    cfg = C.load(args.config)
    cli = C.from_dotlist(unknown)
    helpers.check_yaml(cfg, cli)
    cfg = C.merge(cfg, cli)
    ops.set_float32_matmul_precision(args.matmul_precision)
    rank, world, local = parallel.init_from_env()
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    if args.data_dir:
        train, val, test, size, line = open_data(cfg, layout(cfg), loader_path(here), args.data_dir, args.data_format,
                                                 args.presample, device=dev, rank=rank, world=world,
                                                 test=args.test or mode == "test")
        if line and rank == 0:
            print(line, flush=True)
        loader = test if mode == "test" else train
    else:
        loader, val, test, size = synthetic_data(cfg, layout(cfg), mode, args.validate, args.test, dev, rank, world)
    total = total_steps(len(loader), cfg.trainer.max_epochs, cfg.trainer.accumulate_grad_batches, args.max_steps, mode)
    cfg.trainer.total_train_steps = total
    torch.manual_seed(0)
    model = build(cfg, size).to(dev).train()
    if getattr(model, "autoencoder", None) is not None:
        model.autoencoder.eval()
    if args.invariant_encode:
        enable_invariant_encode(model)
    cache = enable_latent_cache(model, loader, args.latent_cache) if args.latent_cache else None
    if args.verify:
        enable_verification(model)
    # the figures' sink: rank 0's, and only with --plots; a model's steps draw nothing while `panels` is None
    model.panels = helpers.make_sink(args.plots, rank, cfg.trainer, total, len(loader) if mode == "test" else len(val),
                                     len(loader) if mode == "test" else len(test))
    step = 0
    if mode == "test":
        model.eval()
        if getattr(model, "verification", None) is not None:
            model.verification.reset()
        for i in range(min(total, len(loader))):
            if model.panels is not None:
                model.panels.global_step = step
            loss, logs = model.test_step(_frames(loader[i]), step)
            step += 1
            if rank == 0:
                print(json.dumps({"step": step, **{k: float(v) for k, v in logs.items()}}), flush=True)
        report_verification(model, "test", step, rank, world)
        if rank == 0:
            print("done")
        return 0
    nb = len(loader)
    if nb == 0:
        raise ValueError(f"the training loader holds no batch of {cfg.dataset.batch_size} sequences per rank")
    Fn._seed_counter[0] = 0          # the counter-based dropout stream restarts with the run (restored on --resume)
    model.configure_optimizers()
    last = os.path.join(cfg.experiment_path, "outputs", cfg.experiment_name, "checkpoints", "last.ckpt")
    if args.resume:
        step = resume(last, model, state)
        for opt, _ in model.optimizers():               # every rank continues from rank 0's parameters
            for a in opt.arenas:
                model._dp.sync.broadcast_(a.flat_p, 0)
    validating = bool(args.data_dir or args.validate)
    if validating and not hasattr(model, "validation_step"):
        validating = False
        if rank == 0:
            print(f"{type(model).__module__}.Model has no validation_step: training without the validation pass", flush=True)
    # checkpoints during the run come with the new flags; a run without them writes last.ckpt once, at its end
    during = bool(args.data_dir or args.validate or args.test or args.resume or args.stop_after >= 0)
    save_every = max(1, int(total * cfg.trainer.save_every_n_steps)) if during else 0
    stop_at = total if args.stop_after < 0 else min(total, args.stop_after)
    per_step = RATES[rate](cfg.dataset) * world
    t0, start = time.time(), step
    while step < stop_at:
        first = step % nb                               # a resumed run skips the batches its epoch has done
        loader.set_epoch(step // nb)
        for i in range(first, nb):
            if step >= stop_at:
                break
            if model.panels is not None:
                model.panels.global_step, model.panels.epoch, model.panels.batch_idx = step, step // nb, i
            with batch_ids(model, loader, i, "train", cache):
                loss, gn = model.training_step(_frames(loader[i]))
            step += 1
            if rank == 0 and step % max(1, cfg.trainer.log_every_n_steps) == 0:
                print(json.dumps({"step": step, "train_loss": float(loss), "grad_norm": float(gn),
                                  "lr": model.opt.param_groups[0]["lr"],
                                  rate: (step - start) * per_step / (time.time() - t0)}), flush=True)
            if save_every and step % save_every == 0 and step < stop_at and rank == 0:
                save_checkpoint(last, model, state, step, step // nb)
        if validating and step % nb == 0 and step < total:
            # the validation loop at the end of every training epoch; the one after the last step follows the checkpoint
            report(evaluate(model, val, "val", cfg.trainer.limit_val_batches, world, step, nb), rank, step=step,
                   epoch=(step - 1) // nb)
            report_verification(model, "val", step, rank, world)
    if rank == 0:
        save_checkpoint(last, model, state, step, step // nb)
    if validating and step >= total:
        report(evaluate(model, val, "val", cfg.trainer.limit_val_batches, world, step, nb), rank, step=step,
               epoch=(step - 1) // nb)
        report_verification(model, "val", step, rank, world)
    if args.test:
        report(evaluate(model, test, "test", cfg.trainer.limit_test_batches, world, step, nb), rank)
        report_verification(model, "test", step, rank, world)
    if rank == 0:
        if cache is not None:
            print(json.dumps({"latent_cache": cache.stats()}), flush=True)
        print("done")
    return 0


def enable_latent_cache(model, loader, frames):
    """`--latent-cache FRAMES`: the cache of the model's frozen provider, or the reason the run cannot have one"""
    if frames < 0:
        raise WfaeError(f"--latent-cache {frames}: a count of frames, 0 = off")
    ae = getattr(model, "autoencoder", None)
    if not isinstance(ae, Autoencoder):
        raise WfaeError(f"--latent-cache: {type(model).__module__}.Model has no frozen latent provider (_latents.Autoencoder) "
                        "whose latents could be kept: it trains on frames or on its own encoder")
    if not isinstance(model, Step):
        raise WfaeError(f"--latent-cache: {type(model).__module__}.Model does not take the driver's frame ids")
    cache = ae.enable_cache(frames)                 # refuses every kind but autoencoder_kl
    aug = str(getattr(getattr(loader, "loader", loader), "aug_mode", "0"))
    if aug != "0":
        ae.cache = None
        raise WfaeError(f"--latent-cache: the training loader augments (dataset.aug_mode {aug!r}), so a frame differs from "
                        "epoch to epoch and its latent cannot be kept; the flag needs aug_mode \"0\"")
    return cache


def enable_verification(model):
    """`--verify`: a LeadVerification in `model.verification`, or the reason the run cannot have one"""
    from ...pipeline import metrics
    what = f"{type(model).__module__}.Model"
    if not isinstance(model, Step) or not hasattr(model, "validate_latents"):
        raise WfaeError(f"--verify: {what} has no validation step that decodes its forecast (validate_latents); the flag "
                        "belongs to the DLinear forecasters (pretrained_ae_dlinear_*, ae_s2)")
    ae = getattr(model, "autoencoder", None)
    if ae is None:
        raise WfaeError(f"--verify: {what} has no latent provider: without frames and a decoder there is no forecast in "
                        "frame space to hold against persistence")
    if not getattr(ae, "can_decode", lambda: False)():
        raise WfaeError(f"--verify: the latent provider of kind {getattr(ae, 'kind', type(ae).__name__)!r} cannot decode, "
                        "so the forecast never reaches frame space")
    model.verification = metrics.LeadVerification(("forecast", "persistence", "reconstruction"), model.pred_frames)
    return model.verification


def report_verification(model, split, step, rank, world):
    """the `verification` line of a pass that ended (rank 0); every rank takes part in the sum over ranks"""
    v = getattr(model, "verification", None)
    if v is None:
        return
    v.merge(world)
    res = v.result()
    if rank == 0:
        print(json.dumps({"verification": res if "skipped" in res else dict(split=split, step=step, **res)}), flush=True)


def enable_invariant_encode(model):
    """`--invariant-encode`: the model's frozen provider in pass-invariant mode, or the reason the run cannot have it"""
    ae = getattr(model, "autoencoder", None)
    if not isinstance(ae, Autoencoder):
        raise WfaeError(f"--invariant-encode: {type(model).__module__}.Model has no frozen latent provider "
                        "(_latents.Autoencoder) to put into pass-invariant mode: it trains on frames or on its own encoder")
    if ae.kind != "autoencoder_kl":
        raise WfaeError(f"--invariant-encode: the provider is of kind {ae.kind!r}; only the frozen AutoencoderKL "
                        "(autoencoder.kind autoencoder_kl) has a pass-invariant form")
    return ae.set_pass_invariant()


class batch_ids:
    """around a step on `loader[i]`: `model.batch_ids` = (split, the batch's frame ids in (b, t) order), None again
    afterwards.  Without a cache it does nothing"""

    def __init__(self, model, loader, i, split, cache):
        self.model, self.ids = model, None if cache is None else (split, loader.frame_ids(i).reshape(-1))

    def __enter__(self):
        if self.ids is not None:
            self.model.batch_ids = self.ids

    def __exit__(self, *exc):
        if self.ids is not None:
            self.model.batch_ids = None


def _frames(batch):
    """the frame loader yields {"vil": tensor}, the DataModule's loaders a bare tensor"""
    return batch["vil"] if isinstance(batch, dict) else batch


# experiments whose reference train.py imports pipeline.datasets.sevire (one loader per split of the catalog by date);
# every other one imports pipeline.datasets.sevir and builds SEVIRLightningDataModule(cfg.dataset)
DATE_SPLIT = ("ae_gan", "ae_gan_kl", "pretrained_ae_conv_disc")
VAL_DATE, TEST_DATE = datetime.datetime(2019, 1, 1), datetime.datetime(2019, 6, 1)


def loader_path(here):
    """"date" or "datamodule" for the experiment in directory `here`"""
    return "date" if os.path.basename(os.path.normpath(here)) in DATE_SPLIT else "datamodule"


class RankShard:
    """every world-th batch of a DataModule loader for this rank; a remainder is left out (ae_v2_2/train_data2.py)"""

    def __init__(self, loader, world, rank):
        self.loader, self.world, self.rank = loader, int(world), int(rank)

    def __len__(self):
        return len(self.loader) // self.world

    def __getitem__(self, i):
        if i >= len(self):
            raise IndexError(i)
        return self.loader[i * self.world + self.rank]

    def set_epoch(self, epoch):
        self.loader.set_epoch(epoch)

    def frame_ids(self, i):
        if i >= len(self):
            raise IndexError(i)
        return self.loader.frame_ids(i * self.world + self.rank)


def open_data(cfg, layout, path, data_dir, data_format="npy", presample="auto", *, device=None, rank=0, world=1,
              test=True):
    """the loaders of a run on `<data_dir>/CATALOG.csv` + `<data_dir>/data/` -> (train, val, test, size, presample line or
    None); an empty validation or test split (or `test=False`) gives `()`, whose loop is skipped.
    path "date": train < 2019-01-01 <= val < 2019-06-01 <= test, one SEVIRFrameLoader per split sharded by rank, the
    catalog arguments of ae_v2/train.py.  path "datamodule": SEVIRLightningDataModule over the events before 2019-06-01
    (random_split by dataset.val_ratio and dataset.seed, a permutation per epoch, dataset.aug_mode) and the events after
    it for the test loader, as ae_v2_2/train_data2.py builds it; every rank takes each world-th batch"""
    from ...pipeline.datasets.sevire.catalog import CatalogEventStore, H5EventSource, NpyEventSource, SEVIRCatalog
    cat_path = os.path.join(data_dir, "CATALOG.csv")
    source = (H5EventSource if data_format == "h5" else NpyEventSource)(os.path.join(data_dir, "data"))
    d = cfg.dataset

    def store(**kw):
        cat = SEVIRCatalog(cat_path, **kw)
        return CatalogEventStore(cat, source) if len(cat) else None

    split = VAL_DATE if path == "date" else TEST_DATE
    ev_train = store(end_date=split, shuffle=True, shuffle_seed=1)
    if ev_train is None:
        raise ValueError(f"{cat_path}: no training events before {split:%Y-%m-%d}")
    ev_test = store(start_date=TEST_DATE) if test else None
    factors, pooled = resolve_presample(presample, d.name, ev_train.event_shape)
    line = None if factors is None else presample_line(factors, ev_train.event_shape, pooled)
    if path == "date":
        def mk(ev, shuffle):
            if ev is None:
                return ()
            return SEVIRFrameLoader(ev, d.batch_size, d.seq_len, d.stride, layout, shuffle=shuffle, device=device,
                                    num_shard=world, rank=rank, presample=factors)
        return mk(ev_train, True), mk(store(start_date=VAL_DATE, end_date=TEST_DATE), False), mk(ev_test, False), pooled[0], line
    dm = SEVIRLightningDataModule(ev_train, ev_test, dataset_name="sevirlr" if d.name == "sevir_lr" else d.name,
                                  num_workers=d.num_workers, batch_size=d.batch_size, seq_len=d.seq_len, stride=d.stride,
                                  layout=layout, aug_mode=str(d.get("aug_mode", "0")), val_ratio=d.get("val_ratio", 0.1),
                                  seed=d.get("seed", 0),
                                  ret_contiguous=False, device=device, presample=factors)
    dm.prepare_data()
    dm.setup()
    out = [dm.train_dataloader(), dm.val_dataloader(), dm.test_dataloader() if ev_test is not None else ()]
    if world > 1:
        out = [RankShard(ld, world, rank) if len(ld) else () for ld in out]
    return out[0], out[1] if len(out[1]) else (), out[2], pooled[0], line


def synthetic_data(cfg, layout, mode, validate, test, device, rank, world):
    """-> (loader, val, test, size) on synthetic blob events: the loader of the run, and with `validate` / `test` a second
    and third set of events with seeds of their own, as ae_v2/train.py draws them"""
    d = cfg.dataset
    size, frames = (384, 49) if d.name == "sevir" else (128, 25)

    def mk(events, shuffle):
        return SEVIRFrameLoader(events, d.batch_size, d.seq_len, d.stride, layout, shuffle=shuffle, device=device,
                                num_shard=world, rank=rank)

    def extra(seed):
        nspe = 1 + (frames - d.seq_len) // d.stride
        return mk(synth.blob_events(max(1, (d.batch_size * 2 * world) // nspe + 1), size, frames, seed=seed), False)

    loader = mk(synth.blob_events(max(2, d.batch_size * 2 * world), size, frames, seed=1234), mode == "fit")
    return loader, extra(4321) if validate else (), extra(9876) if test else (), size


def evaluate(model, loader, split, limit, world, step=None, nb_train=1):
    """one pass over `limit` (a fraction, Lightning's limit_*_batches; None = all) of `loader` in evaluation mode ->
    {key: epoch mean of the step's logs (`_mean_logs`), "batches": n}, or {"skipped": reason} where the model has no
    step for `split` or refuses it now.  Every module gets its own train / eval state back, so a frozen provider stays
    in evaluation mode; the generators and the dropout counter are left where they were, so a pass does not move the run.
    `step`, `nb_train`: the run's optimiser step and batches per epoch, for the sink of `--plots` (index lines, labels)"""
    name = "test_step" if split == "test" else "validation_step"
    if getattr(model, "verification", None) is not None:
        model.verification.reset()                      # the tables of `--verify` hold one pass
    if not hasattr(model, name):
        return {"skipped": f"{type(model).__module__}.Model has no {name}"}
    refused = getattr(model, "validation_refused", lambda: None)()
    if refused:
        return {"skipped": refused}
    if hasattr(model, "_dp"):
        model._dp.sync_buffers(model)                   # rank 0's BatchNorm statistics everywhere; a collective
    n = len(loader)
    n = n if limit is None else max(1, int(n * limit)) if n else 0
    modes = [(m, m.training) for m in model.modules()]
    counter = Fn._seed_counter[0]
    if getattr(model, "panels", None) is not None and step is not None:
        model.panels.global_step, model.panels.epoch = step, max(0, step - 1) // max(1, nb_train)
    model.eval()
    rows = []
    with torch.random.fork_rng(devices=[torch.cuda.current_device()] if torch.cuda.is_available() else []):
        for i in range(n):
            with batch_ids(model, loader, i, split, getattr(getattr(model, "autoencoder", None), "cache", None)):
                res = getattr(model, name)(_frames(loader[i]), i)
            rows.append(res[1] if isinstance(res, tuple) else {f"{split}_loss": res})
    Fn._seed_counter[0] = counter
    for m, training in modes:
        m.training = training
    out = _mean_logs(rows, world)
    out["batches"] = n
    return out


def report(logs, rank, **more):
    """print the line of a validation / test pass (rank 0); nothing for a split without batches"""
    if rank != 0:
        return
    if "skipped" in logs:
        print(f"pass skipped: {logs['skipped']}", flush=True)
    elif logs.get("batches"):
        print(json.dumps(dict(logs, **more)), flush=True)
