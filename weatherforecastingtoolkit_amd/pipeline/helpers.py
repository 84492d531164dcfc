"""Host-side mirror of the reference's pipeline/helpers.py for the AE train step:
optimiser / scheduler factories with the reference signatures, the YAML
override check, the gradient-norm tracker and `log_images`, the reference's
`log_wandb_images` as PNG files (`--plots DIR`).  (W&B / Lightning glue of the
reference file is orchestration and out of scope — SURVEY.md §2 row 8.)"""
from __future__ import annotations

import json
import math
import os
import struct
import sys
import zlib

import torch

from .. import ops
from ..optim import CosineWarmupLR, FusedAdamW


def adamw_optimizer(model, lr, weight_decay, beta1=0.9, beta2=0.999, exact_complements=False):
    """reference pipeline/helpers.py:63-74 -> torch.optim.AdamW(model.parameters(), ...);
    here one fused kernel over a flat parameter arena with identical arithmetic (`exact_complements`: see FusedAdamW)."""
    return FusedAdamW(model.parameters(), lr=lr, weight_decay=weight_decay, betas=(beta1, beta2),
                      exact_complements=exact_complements)


def cosine_warmup_scheduler(opt, start_lr, final_lr, peak_lr, total_steps, warmup_steps):
    """reference pipeline/helpers.py:76-107 (same positional order). The optimiser's lr is
    overridden by peak_lr like the reference does (:86-89)."""
    for g in opt.param_groups:
        if g["lr"] != peak_lr:
            print(f"lr is not peak lr, it is {g['lr']} changing to {peak_lr}")
            g["lr"] = peak_lr
    return CosineWarmupLR(opt, start_lr, final_lr, peak_lr, total_steps, warmup_steps)


def one_cycle_scheduler(opt, start_lr, peak_lr, final_lr, total_steps, rampup_steps):
    """reference pipeline/helpers.py:109-140 (same positional order): OneCycleLR with pct_start = rampup/total,
    div_factor = peak/start, final_div_factor = start/final, cosine annealing."""
    from ..optim import OneCycleLR
    if rampup_steps / total_steps < 0.2:
        print(f"rampup steps should be higher than 20% of total steps, it is {rampup_steps / total_steps}")
    return OneCycleLR(opt, max_lr=peak_lr, total_steps=total_steps, pct_start=rampup_steps / total_steps,
                      div_factor=peak_lr / start_lr, final_div_factor=start_lr / final_lr)


def check_yaml(cfg, cli_cfg, path=""):
    """reference pipeline/helpers.py:260-266: reject override keys absent from the base file."""
    for k in cli_cfg:
        full_key = f"{path}.{k}" if path else k
        if k not in cfg:
            raise KeyError(f"Invalid override key: '{full_key}' not found in base config")
        if isinstance(cli_cfg[k], dict) and isinstance(cfg[k], dict):
            check_yaml(cfg[k], cli_cfg[k], full_key)


def grad_norm(optimizer_or_params, norm_type=2):
    """TrackGradNormCallback arithmetic (reference :250-256) without 323 host syncs: one
    sum-of-squares kernel per gradient arena (or per tensor), one .item()."""
    assert norm_type == 2
    from ..functional import join_side_stream
    join_side_stream()
    total = 0.0
    arenas = getattr(optimizer_or_params, "arenas", None)
    if arenas:
        for a in arenas:
            if a.grads_in_arena():
                total += float(ops.sumsq(a.flat_g).item())
            else:
                total += sum(float(ops.sumsq(p.grad.contiguous().view(-1)).item()) for p in a.params if p.grad is not None)
        return math.sqrt(total)
    for p in optimizer_or_params:
        if p.grad is not None:
            total += float(ops.sumsq(p.grad.contiguous().view(-1)).item())
    return math.sqrt(total)


def log_metrics(pred, target, tag, log_fn=None):
    """reference :142-153: calc_metrics -> {tag_key: value}."""
    from .metrics import calc_metrics
    out = {f"{tag}_{k}": v for k, v in calc_metrics(pred, target).items()}
    if log_fn is not None:
        log_fn(out)
    return out


# ---- prediction / target / difference panels (reference :155-225 `log_wandb_images`), without matplotlib and W&B:
# csrc/panels.hip draws the first samples of the batch where it lies, the host compresses and frames the PNG
PANEL_GAP = 2            # white pixels between neighbouring panels and row blocks
PANEL_ROWS = ("target", "prediction", "abs_difference")   # the fixed row order of a figure, top to bottom
# zlib level of the figures: compression is all but the whole cost of a due call (tools/panels_bench.py), and level 1 takes
# about a third of level 6's time for files about a third larger
PNG_LEVEL = 1

# matplotlib's `Reds` as `imshow(u8, cmap='Reds', vmin=0, vmax=255)` paints it (reference :212): 256 x RGB, table index =
# byte value.  Carried as data (tests/golden/make_panel_goldens.py prints it): interpolating the nine ColorBrewer anchors
# in fp64 is off by one level in places, and the package does not import matplotlib.
_REDS_HEX = (
    "fff5f0fef4effef3eefef3edfef2ecfef1ebfef1eafef0e9feefe8feefe7feeee6feede5feede4feece3feebe2feebe1"
    "feeae0fee9e0fee9dffee8defee7ddfee7dcfee6dbfee5dafee5d9fee4d8fee3d7fee3d6fee2d5fee1d4fee1d3fee0d2"
    "fddfd1fdded0fdddcefddccdfddbcbfddacafdd8c8fdd7c7fdd6c5fdd5c3fdd4c2fdd3c0fdd1bffdd0bdfdcfbcfdceba"
    "fccdb9fcccb7fccab6fcc9b4fcc8b3fcc7b1fcc6affcc5aefcc3acfcc2abfcc1a9fcc0a8fcbfa6fcbea5fcbda3fcbba2"
    "fcbaa0fcb99ffcb89dfcb69cfcb59afcb499fcb297fcb196fcb094fcaf93fcad91fcac90fcab8efca98dfca88bfca78a"
    "fca689fca487fca386fca284fca083fc9f81fc9e80fc9d7efc9b7dfc9a7bfc997afc9778fc9677fc9575fc9474fc9272"
    "fb9171fb9070fb8f6ffb8d6dfb8c6cfb8b6bfb8a6afb8868fb8767fb8666fb8464fb8363fb8262fb8161fb7f5ffb7e5e"
    "fb7d5dfb7c5cfb7a5afb7959fb7858fb7757fb7555fb7454fb7353fb7252fb7050fb6f4ffb6e4efb6d4dfb6b4bfb6a4a"
    "fa6949fa6748fa6647f96446f96345f86144f86043f85e42f75d42f75b41f75a40f6593ff6573ef5563df5543cf5533b"
    "f4513af45039f44e38f34d37f34b36f24a35f24834f24733f14532f14432f14231f04130f03f2fef3e2eef3d2def3b2c"
    "ee3a2bed392bec382aea372ae93529e83429e73328e63228e53127e43027e32f27e12e26e02d26df2c25de2a25dd2924"
    "dc2824db2723d92623d82522d72422d62321d52221d42120d31f20d21e1fd01d1fcf1c1fce1b1ecd1a1ecc191dcb181d"
    "ca171cc8171cc7171cc6161cc5161bc4161bc2161bc1151bc0151abf151abe141abc141abb1419ba1419b91319b81319"
    "b71318b51218b41218b31218b21217b11117af1117ae1117ad1116ac1016ab1016a91016a80f15a70f15a60f15a50f15"
    "a30e14a10e149f0d149d0d149b0c13990c13970b13950b13930a12910a128f09128d09128b08118a0811880811860711"
    "8407108206108006107e05107c050f7a040f78040f76030f74030e72020e70020e6e010e6c010d6a000d68000d67000c")


def reds_lut():
    """uint8 (256, 3): the colours of the difference row"""
    return torch.frombuffer(bytearray(bytes.fromhex(_REDS_HEX)), dtype=torch.uint8).view(256, 3).clone()


_luts = {}


def _device_luts(device):
    """(vil, reds) on `device`, uploaded once"""
    key = str(device)
    if key not in _luts:
        from .datasets.sevir.sevir import vil_lut
        _luts[key] = (vil_lut().to(device), reds_lut().to(device))
    return _luts[key]


class PanelSink:
    """Where the figures of a run go: the directory of `--plots DIR`, the global step the index lines carry, and what
    the steps' cadence reads from a Lightning module and its config in the reference: the current epoch and the
    `trainer.total_{train,val,test}_steps` of the run.  The drivers keep it up to date; it lives as `model.panels`
    (None without the flag), on rank 0 only."""

    def __init__(self, directory, global_step=0, epoch=0, totals=None):
        self.dir = str(directory)
        self.global_step, self.epoch = int(global_step), int(epoch)
        self.batch_idx = 0           # the training batch in flight, for the training steps that take no index
        self.totals = dict(totals or {})
        os.makedirs(self.dir, exist_ok=True)

    def total(self, split):
        return self.totals.get(split, 0)


def make_sink(directory, rank, trainer, n_train_steps, n_val_batches, n_test_batches):
    """the sink of `--plots directory` for rank 0, None for every other rank and without the flag.  The totals are the
    reference's (`ae_v2/train.py:306-317`): batches * max_epochs / accumulate_grad_batches, as an int, or times
    limit_*_batches where that is set; the train total is the run's own number of optimiser steps"""
    if not directory or rank != 0:
        return None

    def total(n, limit):
        t = n * trainer.max_epochs / trainer.accumulate_grad_batches
        return t * limit if limit is not None else int(t)

    return PanelSink(directory, totals={"train": n_train_steps,
                                        "val": total(n_val_batches, trainer.get("limit_val_batches")),
                                        "test": total(n_test_batches, trainer.get("limit_test_batches"))})


def plot_fraction(cfg, key, default):
    """logging.<key> of the run's config, or `default` (the value of the reference's config.yaml) where the file has
    no such key; a null fraction (prediff_mlp_sevir) stays None"""
    lg = cfg.get("logging") or {}
    return lg[key] if key in lg else default


def plot_due(counter, fraction, total):
    """the reference's cadence (e.g. ae_v2/train.py:220-221): interval = int(fraction * total), due iff
    counter % interval == 0.  The one deviation: where the reference divides by zero (a short run, interval == 0) the
    interval is 1.  A null fraction never plots (the reference would raise on None * total)."""
    if fraction is None:
        return False
    interval = int(fraction * total)
    return counter % (interval if interval > 0 else 1) == 0


def sanitise_label(label):
    """a label as a file name: every character outside [A-Za-z0-9._-] becomes '_', leading dots go, at most 200
    characters; an empty result is 'panel'"""
    out = "".join(c if (c.isascii() and c.isalnum()) or c in "._-" else "_" for c in str(label)).lstrip(".")[:200]
    return out or "panel"


_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"


def _png_chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_png(path, data, width, height, level=6):
    """8-bit RGB, non-interlaced PNG of `width` x `height` from `data` (bytes-like): either the scanline stream an IDAT
    chunk holds before compression — `height` rows of a filter byte 0 and 3 * width colour bytes, what
    ops.panel_render leaves — or plain RGB rows of 3 * width bytes, which get their filter bytes here.  Standard
    library only; written to a temporary name, then moved in place."""
    data = bytes(data)
    width, height = int(width), int(height)
    if width < 1 or height < 1:
        raise ValueError(f"write_png: {width} x {height}")
    if len(data) == height * 3 * width:
        row = 3 * width
        data = b"".join(b"\x00" + data[y * row:(y + 1) * row] for y in range(height))
    elif len(data) != height * (1 + 3 * width):
        raise ValueError(f"write_png: {len(data)} bytes for {width} x {height} RGB")
    png = (_PNG_MAGIC + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, 2, 0, 0, 0))
           + _png_chunk(b"IDAT", zlib.compress(data, level)) + _png_chunk(b"IEND", b""))
    tmp = f"{path}.tmp{os.getpid()}"
    with open(tmp, "wb") as f:
        f.write(png)
    os.replace(tmp, path)


def log_images(predicted, target, label, sink, batch_idxs=4):
    """reference :155-225.  predicted, target: device fp32 (B, T, H, W) or (B, T, 1, H, W), values in [0, 1].  Draws
    the first min(batch_idxs, B) samples (ops.panel_render: rows target / prediction / absolute difference, one column
    per frame, the VIL colours and `Reds`), copies only those figures to the host and writes
    `<sink.dir>/<sanitised label>_b<b>.png` plus one line per figure in `<sink.dir>/index.jsonl`.  Prints the
    reference's warning (to stderr: stdout stays JSON lines) when fewer than 90 % of the WHOLE target lies in [0, 1].
    No titles, axes or colour bars: there is no font rasteriser here; the index line names the row order.
    Touches no generator and no module state.  -> the written paths"""
    predicted, target = predicted.detach(), target.detach()
    if predicted.dim() == 5:
        if predicted.shape[2] != 1:
            raise ValueError(f"Predicted must be (B,T,1,H,W), got {tuple(predicted.shape)}")
        predicted = predicted.squeeze(2)
    if target.dim() == 5:
        if target.shape[2] != 1:
            raise ValueError(f"Target must be (B,T,1,H,W), got {tuple(target.shape)}")
        target = target.squeeze(2)
    if predicted.dim() != 4 or predicted.shape != target.shape:
        raise ValueError(f"log_images: predicted {tuple(predicted.shape)} and target {tuple(target.shape)} must be one "
                         "(B, T, H, W) or (B, T, 1, H, W) shape")
    predicted, target = predicted.contiguous(), target.contiguous()
    b, t, h, w = target.shape
    nb = min(int(batch_idxs), b)
    ratio = int(ops.range_count(target).item()) / target.numel()
    if ratio < 0.9:
        print(f"\033[91mtarget data not in [0,1] range: {ratio:.2%}\033[0m", file=sys.stderr, flush=True)
    if nb < 1:
        return []
    vil, reds = _device_luts(target.device)
    figs = ops.panel_render(predicted, target, vil, reds, nb, PANEL_GAP).cpu().numpy()
    hfig, wfig = figs.shape[1], (figs.shape[2] - 1) // 3
    stem = sanitise_label(label)
    paths, lines = [], []
    for i in range(nb):
        name = f"{stem}_b{i}.png"
        write_png(os.path.join(sink.dir, name), figs[i].tobytes(), wfig, hfig, PNG_LEVEL)
        paths.append(os.path.join(sink.dir, name))
        lines.append(json.dumps({"label": str(label), "file": name, "sample": i, "global_step": int(sink.global_step),
                                 "T": t, "H": h, "W": w, "gap": PANEL_GAP, "rows": list(PANEL_ROWS),
                                 "in_range": ratio}))
    with open(os.path.join(sink.dir, "index.jsonl"), "a") as f:
        f.write("".join(line + "\n" for line in lines))
    return paths


def plot_panels(module, predicted, target, label, counter, fraction, total):
    """what a step calls next to `log_metrics`: `log_images` on the same pair when the module has a sink
    (`module.panels`, set by `--plots`) and `plot_due(counter, fraction, total)`"""
    sink = getattr(module, "panels", None)
    if sink is not None and plot_due(counter, fraction, total):
        log_images(predicted, target, label, sink)
