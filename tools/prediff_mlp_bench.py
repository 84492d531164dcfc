"""Intensity-statistics MLP forecaster (prediff_mlp_sevir) at the config's size — B = 8 sequences of 25 frames of
384 x 384 fp32, 118 MB — on the gfx950 kernels.  Prints one JSON line:

  stats_<order>_*   the statistics entry point (both of its launches) in the two memory orders: `frames` (the loader's
                    permuted view of a contiguous (B, T, H, W) tensor) and `tinner` (contiguous (B, H, W, T)), timed with
                    device events.  `hot`: back-to-back calls on the same batch, which fits the 256 MiB Infinity Cache;
                    `cold`: each call after a read pass over a 1 GiB buffer that evicts it (a read, so that
                    no dirty lines are left to be written back under the timed call).  GB/s = batch bytes / time.
  step_*            the whole training step (statistics, fused MLP + loss + gradients, scale, clip 1.0, AdamW,
                    scheduler) in microseconds of wall clock per step, its entry-point calls and kernel launches;
  eager_*           the reference's training_step written with torch-ROCm eager ops (strided views, reshape copies,
                    nn.Sequential, F.mse_loss, clip_grad_norm_, torch.optim.AdamW) on the same GPU and batch.

    python tools/prediff_mlp_bench.py [--steps 200] [--batch 8] [--size 384]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn as tnn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from weatherforecastingtoolkit_amd import config as C  # noqa: E402
from weatherforecastingtoolkit_amd import ops  # noqa: E402
from weatherforecastingtoolkit_amd.experiments.v1_experiments import _prediff_mlp as M  # noqa: E402

# kernel launches behind one call of an entry point (csrc/prediff.hip, loss.hip, api.hip)
LAUNCHES = {"wfae_seq_intensity_stats": 2, "wfae_sumsq": 2}


def events_us(fn, reps, between=None):
    """per-call device time of fn in microseconds: [reps] samples when `between` runs in front of every call, else one
    figure from a window of reps back-to-back calls"""
    if between is None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return [e0.elapsed_time(e1) * 1e3 / reps]
    out = []
    for _ in range(reps):
        between()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return out


def wall_us(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def eager_launches(fn):
    """device kernels of one call, from torch's profiler; None where the build has no device tracing"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=384)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prediff_mlp_bench needs a GPU: nothing here is measured on a CPU")
    dev = torch.device("cuda:0")
    B, S, T = a.batch, a.size, 25
    g = torch.Generator().manual_seed(1)
    nthw = torch.rand(B, T, S, S, generator=g).to(dev)
    batches = {"frames": nthw.permute(0, 2, 3, 1), "tinner": nthw.permute(0, 2, 3, 1).contiguous()}
    nbytes = 4 * nthw.numel()
    evict = torch.empty(1 << 28, dtype=torch.float32, device=dev)   # 1 GiB
    out = {"B": B, "size": S, "frames": T, "batch_MB": round(nbytes / 1e6, 1)}
    for order, batch in batches.items():
        fn = lambda: ops.seq_intensity_stats(batch, 5)   # noqa: E731
        for _ in range(a.warmup):
            fn()
        hot = events_us(fn, a.steps)[0]
        cold = events_us(fn, 20, between=lambda: evict.sum())
        out[f"stats_{order}_hot_us"] = round(hot, 2)
        out[f"stats_{order}_hot_GBps"] = round(nbytes / hot / 1e3, 1)
        out[f"stats_{order}_cold_us_median"] = round(statistics.median(cold), 2)
        out[f"stats_{order}_cold_us_min"] = round(min(cold), 2)
        out[f"stats_{order}_cold_GBps"] = round(nbytes / statistics.median(cold) / 1e3, 1)

    cfg = C.load(os.path.join(os.path.dirname(M.__file__), "prediff_mlp_sevir", "config.yaml"))
    cfg.trainer.total_train_steps = 10 ** 6
    for order, batch in batches.items():
        torch.manual_seed(0)
        model = M.Model(cfg).to(dev).train()
        model.configure_optimizers()
        out[f"step_{order}_us"] = round(wall_us(lambda: model.training_step(batch), a.warmup, a.steps), 1)
    ops.profile_start()
    model.training_step(batch)
    prof = ops.profile_stop()
    out["step_entry_point_calls"] = {k: v[0] for k, v in sorted(prof.items())}
    out["step_launches"] = sum(v[0] * LAUNCHES.get(k, 1) for k, v in prof.items())
    x, target = ops.seq_intensity_stats(batch, 5)
    out["mlp_fused_us"] = round(events_us(lambda: model.model.loss(x, target), a.steps)[0], 2)

    # the reference's step in torch eager ops on the same GPU (the reference's `ret_contiguous: true` batch)
    torch.manual_seed(0)
    net = tnn.Sequential(tnn.Linear(5, 128), tnn.ReLU(), tnn.Linear(128, 128), tnn.ReLU(), tnn.Linear(128, 8)).to(dev)
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3, weight_decay=1e-2)
    nhwt = batches["tinner"]

    def eager_stats():
        seq = nhwt.permute(0, 3, 1, 2).unsqueeze(2)
        inp, tgt = seq[:, :5], seq[:, 5:]
        b, t = inp.shape[:2]
        xi = inp.reshape(b, t, -1).mean(dim=2)
        runs = tgt.reshape(b, t, -1).reshape(b, 4, t // 4, -1)
        return xi, torch.cat([runs.mean(dim=[2, 3]), runs.std(dim=[2, 3])], dim=-1)

    def eager_step():
        xi, tg = eager_stats()
        loss = F.mse_loss(net(xi), tg)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), 1.0)
        opt.step()

    out["eager_step_us"] = round(wall_us(eager_step, 5, max(10, a.steps // 4)), 1)
    out["eager_stats_us"] = round(events_us(eager_stats, max(10, a.steps // 4))[0], 1)
    out["eager_step_launches"] = eager_launches(eager_step)
    out["speedup_step"] = round(out["eager_step_us"] / out["step_tinner_us"], 1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
