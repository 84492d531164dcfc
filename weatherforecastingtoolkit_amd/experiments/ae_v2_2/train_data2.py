"""experiments/ae_v2_2 on the SECOND SEVIR loader — the mirror of the reference's experiments/ae_v2_2/train_data2.py:
the same `Model` and `Loss` as train.py (imported, not copied), driven through `SEVIRLightningDataModule`
(pipeline/datasets/sevir/sevir.py) with layout 'NTHW', `aug_mode=str(cfg.dataset.aug_mode)`, val_ratio 0.1 and
ret_contiguous False, as the reference builds it (:243-253).  A batch is a bare tensor (:130).

    python -m weatherforecastingtoolkit_amd.experiments.ae_v2_2.train_data2 [--config F] [--max-steps N] key=value ...

What differs from train.py is the data path only: single sequences split into train / val by random_split, a fresh
train permutation per epoch, and the flips + rotation of `aug_mode` applied inside the uint8 -> fp32 conversion kernel.
Without --data-dir the events are synthetic (`synth.blob_events`); with it, --presample (default auto) pools raw
384 x 384 x 49 events to the 128 x 128 x 25 of the `sevirlr` config on the device.  Checkpoints are written like
train.py's; resuming is train.py's feature and not repeated here.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

from ... import config as C
from ... import functional as Fn
from ... import ops
from ... import parallel, synth
from ...nn import flush_bn_counters
from ...pipeline import helpers
from ...pipeline.datasets.sevir.sevir import SEVIRLightningDataModule
from ...pipeline.datasets.sevire.sevir import parse_presample, presample_line, resolve_presample
from .train import CARRIED_KEYS, HERE, Model, add_lpips_arguments, lpips_from_arguments


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=os.path.join(HERE, "config.yaml"))
    ap.add_argument("--max-steps", type=int, default=-1, help="shorten the run (smoke runs): total_train_steps = this")
    ap.add_argument("--matmul-precision", default="high", choices=["highest", "high", "medium"])
    ap.add_argument("--data-dir", default=None, help="SEVIR root (CATALOG.csv + data/); default: synthetic events")
    ap.add_argument("--data-format", choices=("npy", "h5"), default="npy")
    ap.add_argument("--presample", type=parse_presample, default="auto", metavar="auto|none|T,H,W",
                    help="with --data-dir: pool the events on the device as the loader converts them.  auto = (2, 3, 3) "
                         "when the config names sevirlr and the store holds raw 384x384x49 events, else none")
    ap.add_argument("--plots", default=None, metavar="DIR",
                    help="write target / prediction / difference panels of the training step, at the reference's cadence, "
                         "into DIR as PNG files with one line each in DIR/index.jsonl (rank 0)")
    add_lpips_arguments(ap)
    args, unknown = ap.parse_known_args(argv)
    cfg = C.load(args.config, CARRIED_KEYS)
    cli = C.from_dotlist(unknown)
    helpers.check_yaml(cfg, cli)
    cfg = C.merge(cfg, cli)

    rank, world, local = parallel.init_from_env()
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    ops.set_float32_matmul_precision(args.matmul_precision)

    size, frames = (384, 49) if cfg.dataset.name == "sevir" else (128, 25)
    B = cfg.dataset.batch_size
    presample = None
    if args.data_dir:
        # train + val before the reference's train_test_split_date, test after it (sevir/sevir.py:1087, 1175, 1197)
        import datetime
        from ...pipeline.datasets.sevire.catalog import CatalogEventStore, H5EventSource, NpyEventSource, SEVIRCatalog
        cat_path = os.path.join(args.data_dir, "CATALOG.csv")
        source = (H5EventSource if args.data_format == "h5" else NpyEventSource)(os.path.join(args.data_dir, "data"))
        split = datetime.datetime(2019, 6, 1)
        cat_train = SEVIRCatalog(cat_path, end_date=split, shuffle=True, shuffle_seed=1)
        cat_test = SEVIRCatalog(cat_path, start_date=split)
        if not len(cat_train):
            raise ValueError(f"{cat_path}: no events before {split:%Y-%m-%d}")
        ev_train = CatalogEventStore(cat_train, source)
        ev_test = CatalogEventStore(cat_test, source) if len(cat_test) else None
        presample, pooled = resolve_presample(args.presample, cfg.dataset.name, ev_train.event_shape)
        size = pooled[0]
        if presample is not None and rank == 0:
            print(presample_line(presample, ev_train.event_shape, pooled), flush=True)
    else:
        nspe = 1 + (frames - cfg.dataset.seq_len) // cfg.dataset.stride
        ev_train = synth.blob_events(max(2, (B * 10 * world) // nspe + 1), size, frames, seed=1234)
        ev_test = synth.blob_events(max(1, (B * 2 * world) // nspe + 1), size, frames, seed=9876)

    dm = SEVIRLightningDataModule(ev_train, ev_test, dataset_name=cfg.dataset.name, num_workers=cfg.dataset.num_workers,
                                  batch_size=B, seq_len=cfg.dataset.seq_len, stride=cfg.dataset.stride, layout="NTHW",
                                  aug_mode=str(cfg.dataset.aug_mode), val_ratio=0.1, ret_contiguous=False, device=dev,
                                  presample=presample)
    dm.prepare_data()
    dm.setup()
    loader = dm.train_dataloader()
    if rank == 0:
        for ld in (loader, dm.val_dataloader()) + ((dm.test_dataloader(),) if ev_test is not None else ()):
            print(f"Number of batches in dataloader: {len(ld)}")                  # reference :257-261
            print(f"Data shape: {tuple(ld[0].shape)}", flush=True)

    per_epoch = len(loader) // world         # every rank takes each world-th batch; a remainder is left out
    accum = cfg.trainer.accumulate_grad_batches
    total = (per_epoch * cfg.trainer.max_epochs) / accum                          # reference :263
    if cfg.trainer.limit_train_batches is not None:
        total = total * cfg.trainer.limit_train_batches                           # reference :269-270
    total = max(1, int(total))
    if 0 < args.max_steps < total:
        total = args.max_steps
    cfg.trainer.total_train_steps = total
    cfg.lpips.disc_start = int(cfg.lpips.disc_start * total)                      # reference :275

    torch.manual_seed(0)
    Fn._seed_counter[0] = 0
    model = Model(cfg, img_size=size, lpips=lpips_from_arguments(args)).to(dev).train()
    Fn.set_wgrad_overlap(True)
    model.configure_optimizers()
    model.panels = helpers.make_sink(args.plots, rank, cfg.trainer, total, 0, 0)      # this driver has no other loop

    t0, done, epoch = time.time(), 0, 0
    pending = []   # per-step scalars are read one step late (no stall of the launch queue)

    def flush_logs():
        while pending:
            step_, logs_, lr_, n_ = pending.pop(0)
            rec = {k: float(v) for k, v in logs_.items()}
            rec.update(step=step_, lr=lr_, frames_per_s=n_ * B * world / (time.time() - t0))
            print(json.dumps(rec), flush=True)

    while model.global_step < total:
        loader.set_epoch(epoch)              # this epoch's permutation and this epoch's transforms
        if model.panels is not None:
            model.panels.epoch = epoch
        for k in range(per_epoch):
            if model.global_step >= total:
                break
            _, logs = model.training_step(loader[k * world + rank], k)
            done += 1
            if rank == 0 and done % max(1, cfg.trainer.log_every_n_steps) == 0:
                flush_logs()
                pending.append((model.global_step, logs, model.g_opt.param_groups[0]["lr"], done))
        epoch += 1
    flush_logs()
    for dp in model._dp:
        dp.sync_buffers()
    if rank == 0:
        flush_bn_counters(model)
        ckpt_dir = os.path.join(cfg.experiment_path, "outputs", cfg.experiment_name, "checkpoints")
        os.makedirs(ckpt_dir, exist_ok=True)
        last = os.path.join(ckpt_dir, "last.ckpt")
        sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
        torch.save({"state_dict": sd, "global_step": model.global_step,
                    "optimizer_states": [model.g_opt.state_dict(), model.d_opt.state_dict()],
                    "lr_schedulers": [model.g_sch.state_dict(), model.d_sch.state_dict()]}, last + ".tmp")
        os.replace(last + ".tmp", last)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print("done")
    return 0


if __name__ == "__main__":
    sys.exit(main())
