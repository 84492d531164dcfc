"""What `--latent-cache` is worth: one training step with the frozen AutoencoderKL's latents recomputed (the path without the
flag), with the cache on and every frame missing, and with every frame hitting, at two shipped geometries —

  ae_s2     experiments/ae_s2/config.yaml: B = 8 sequences of 13 frames of 128 x 128, sampled latents 64 x 16 x 16
            (a row is the moments, 2 x 16384 fp32 = 128 KiB: 8192 frames are 1 GiB), DLinear predictor
  convae    experiments/v1_experiments/pretrained_ae_convae_sevir/config_autoencoder_kl.yaml: B = 8 frames of 384 x 384,
            latents 4 x 48 x 48 (a row is the mode, 9216 fp32 = 36 KiB), conv autoencoder predictor

    python tools/latent_cache_bench.py [--steps 5] [--rounds 5] [--precisions highest,medium] [--capacity 8192]
                                       [--out profiles/latent_cache_bench.jsonl]

Synthetic frames (seeded uniform noise), nothing outside the tree is read.  Per geometry and precision one JSON line is
appended to --out.  The three variants alternate inside one process, `rounds` rounds of `steps` steps each between a pair of
device events, one untimed step of each first:
  (a) uncached    model.batch_ids = None: `Autoencoder.encode(frames)`, the code path of a run without the flag
  (b) all_miss    the cache forgets its frames in front of every step (a host dict): plan, encode, scatter, gather
  (c) all_hit     every frame is in the table: plan, gather; the encoder is not called
The line holds the median of each, every round's triple, (b) - (a) next to the spread (min .. max) of the (a) rounds, the
misses and hits counted in the (b) and (c) windows, whether the cached latents are the uncached bits at this geometry (all
miss, all hit, and partial misses: the cached batch with its last 1, 5 and 13 frames replaced by unseen ones), the
table's size, the same three variants with the provider in pass-invariant mode (`--invariant-encode`; both modes alternate
inside every round, its uncached step is held against the default uncached step of the same run and the spread of both),
a step with 1, 5 and 13 of the batch's frames missing in both modes (`partial_miss_step_ms`: the default mode encodes whole
passes for them, the pass-invariant mode the missing frames), and the gather kernel on its own: the call a step makes (B*T frames; launch-bound at this size) and one over
the whole table, whose bytes (row + noise read, latent written) over device time is the figure to hold against the
6.1 - 6.2 TB/s of the project's other streaming kernels.  There are no thresholds: the tool measures.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import weatherforecastingtoolkit_amd as pkg  # noqa: E402
from weatherforecastingtoolkit_amd import config as C  # noqa: E402
from weatherforecastingtoolkit_amd import _lib, ops  # noqa: E402
from weatherforecastingtoolkit_amd.experiments.ae_s2 import train as S2  # noqa: E402
from weatherforecastingtoolkit_amd.experiments.v1_experiments import _runner  # noqa: E402
from weatherforecastingtoolkit_amd.experiments.v1_experiments.pretrained_ae_convae_sevir import train as CV  # noqa: E402


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def ae_s2_case(dev):
    cfg = C.load(os.path.join(S2.HERE, "config.yaml"))
    cfg.trainer.total_train_steps = 1000
    torch.manual_seed(0)
    model = S2.Model(cfg)
    d = cfg.dataset
    frames = torch.rand(d.batch_size, d.seq_len, 1, d.image_width, d.image_width, generator=torch.Generator().manual_seed(1))
    return "ae_s2", model, frames.to(dev), (d.batch_size, d.seq_len)


def convae_case(dev):
    cfg = C.load(os.path.join(CV.HERE, "config_autoencoder_kl.yaml"))
    cfg.trainer.total_train_steps = 1000
    torch.manual_seed(0)
    model = _runner.with_provider(CV.Model)(cfg, 384)
    d = cfg.dataset
    frames = torch.rand(d.batch_size, d.seq_len, 384, 384, generator=torch.Generator().manual_seed(1))      # 'NTHW'
    return "convae_autoencoder_kl", model, frames.to(dev), (d.batch_size, d.seq_len)


def gather_alone(table, latent_shape, sample, bt, calls, dev):
    """the gather over `bt` frames that all hit -> {frames, MB moved, kernel_ms and TB_per_s of the entry point launched
    back to back on a prepared index and output, ops_call_ms of ops.latent_gather as a step calls it (index check, its
    copy to the device and the output's allocation included)}"""
    b, t = bt
    n, l = b * t, table.shape[1]
    index = np.arange(n) % table.shape[0]
    noise = torch.randn(t, b, latent_shape[0] // 2, *latent_shape[1:], device=dev) if sample else None
    lout = l // 2 if sample else l
    nbytes = 4 * n * (l + lout + (lout if sample else 0))
    out = ops.latent_gather(table, None, index, bt, noise)
    call_ms = timed(lambda: ops.latent_gather(table, None, index, bt, noise), calls)
    index_dev = torch.from_numpy(index.astype(np.int32)).to(dev)
    args = (table.data_ptr(), None, index_dev.data_ptr(), None if noise is None else noise.data_ptr(), out.data_ptr(), b, t, l,
            1 if sample else 0, table.shape[0], 0, torch.cuda.current_stream().cuda_stream)
    ms = timed(lambda: _lib.call("wfae_latent_gather", *args), calls)
    return {"frames": n, "MB": round(nbytes / 1e6, 2), "kernel_ms": round(ms, 4), "TB_per_s": round(nbytes / ms / 1e9, 3),
            "ops_call_ms": round(call_ms, 4)}


def bits_check(ae, cache, x, ids, n, bt, dev):
    """the cached latents against the uncached ones of the provider's present mode, on one noise where the provider samples:
    all miss, all hit, and partial misses — the cached batch with its last 1, 5 and 13 frames replaced by unseen ones (other
    pixels, new ids); a partial miss counts as equal only if exactly k frames were counted as missed"""
    with torch.no_grad():
        plain = ae.encode(x)
        shape = tuple(plain.shape[2:])
        noise = ae.draw_noise(bt[0], bt[1], shape, dev) if ae.sample else None
        plain = ae.encode(x, noise=noise)
        cache.clear()
        missed = ae.encode(x, noise=noise, ids=ids)
        hit = ae.encode(x, noise=noise, ids=ids)
        partial = {}
        for k in (1, 5, 13):
            if k >= n:
                continue
            flat = x.reshape(n, *x.shape[2:]).clone()
            flat[n - k:] = 1.0 - flat[n - k:]
            x2 = flat.view_as(x)
            ids2 = ids[1].copy()
            ids2[n - k:] = n + 100 * k + np.arange(k)
            m0 = cache.misses
            got = ae.encode(x2, noise=noise, ids=("train", ids2))
            partial[str(k)] = bool(torch.equal(got, ae.encode(x2, noise=noise))) and cache.misses - m0 == k
    return {"miss": bool(torch.equal(plain, missed)), "hit": bool(torch.equal(plain, hit)), "partial_miss_of_k_frames": partial}


def measure(name, model, frames, bt, prec, a, dev):
    ae = model.autoencoder
    cache = ae.enable_cache(a.capacity)
    n = bt[0] * bt[1]
    ids = ("train", np.arange(n, dtype=np.int64))
    ks = [k for k in (1, 5, 13) if k < n]
    unseen = [1 << 20]              # ids of the frames a partial-miss step has not met: a new one for every missing frame

    def uncached():
        model.batch_ids = None
        model.training_step(frames)

    def all_miss():
        cache.clear()
        model.batch_ids = ids
        model.training_step(frames)

    def all_hit():
        model.batch_ids = ids
        model.training_step(frames)

    def partial(k):
        def step():                 # the batch that hits, its last k frames under ids the table has not seen
            ids2 = ids[1].copy()
            ids2[n - k:] = unseen[0] + np.arange(k)
            unseen[0] += k
            model.batch_ids = ("train", ids2)
            model.training_step(frames)
        step.__name__ = f"partial_{k}"
        return step

    # one mode after the other inside every round; all_miss refills the table that the change of mode emptied, all_hit and
    # the partial misses follow it
    variants = [uncached, all_miss, all_hit, *(partial(k) for k in ks)]
    modes = ("default", "pass_invariant")
    for mode in modes:
        ae.set_pass_invariant(mode == "pass_invariant")
        for fn in variants:
            timed(fn, 1)
    rounds = {mode: [] for mode in modes}
    counts = {mode: {fn.__name__: [0, 0] for fn in variants[1:]} for mode in modes}
    for _ in range(a.rounds):
        for mode in modes:
            ae.set_pass_invariant(mode == "pass_invariant")
            row = []
            for fn in variants:
                h, m = cache.hits, cache.misses
                row.append(timed(fn, a.steps))
                if fn is not uncached:
                    counts[mode][fn.__name__][0] += cache.misses - m
                    counts[mode][fn.__name__][1] += cache.hits - h
            rounds[mode].append(row)
    model.batch_ids = None
    med = {mode: [statistics.median(r[i] for r in rounds[mode]) for i in range(len(variants))] for mode in modes}
    spread = {mode: [round(min(r[0] for r in rounds[mode]), 3), round(max(r[0] for r in rounds[mode]), 3)] for mode in modes}
    ta, tb, tc = med["default"][:3]
    ia, ib, ic = med["pass_invariant"][:3]

    x = frames if frames.dim() == 5 else frames.unsqueeze(2)
    ae.set_pass_invariant(False)
    bits = bits_check(ae, cache, x, ids, n, bt, dev)
    pass_frames, bypassed = cache.pass_frames.get("train"), cache.bypassed
    ae.set_pass_invariant(True)
    bits_inv = bits_check(ae, cache, x, ids, n, bt, dev)
    bypassed_inv = cache.bypassed - bypassed
    ae.set_pass_invariant(False)
    shape = cache.latent_shape
    big = (max(1, min(a.capacity, 8192) // 16), 16)
    cache.table.normal_()           # the big gather reads every row: give the rows nobody wrote a value
    names = [fn.__name__ for fn in variants]
    line = {"case": name, "frames": list(frames.shape), "precision": prec, "latent": list(shape), "sample": bool(ae.sample),
            "row_KiB": cache.table.shape[1] * 4 / 1024, "capacity_frames": cache.capacity, "table_MiB": cache.bytes / 2 ** 20,
            "train_step_ms": {"uncached": round(ta, 3), "all_miss": round(tb, 3), "all_hit": round(tc, 3),
                              "uncached_over_all_hit": round(ta / tc, 2)},
            "miss_overhead_ms": {"all_miss_minus_uncached": round(tb - ta, 3), "uncached_spread": spread["default"]},
            "rounds_uncached_miss_hit": [[round(v, 3) for v in r[:3]] for r in rounds["default"]],
            "counted": {k: {"misses": v[0], "hits": v[1]} for k, v in counts["default"].items()},
            "cached_bits_equal_uncached": bits,
            "pass_frames": pass_frames, "bypassed": bypassed,
            # the same step with the provider in pass-invariant mode (--invariant-encode), alternated with the above
            "pass_invariant": {
                "train_step_ms": {"uncached": round(ia, 3), "all_miss": round(ib, 3), "all_hit": round(ic, 3)},
                "uncached_minus_default_uncached_ms": round(ia - ta, 3),
                "uncached_spread": spread["pass_invariant"], "default_uncached_spread": spread["default"],
                "rounds_uncached_miss_hit": [[round(v, 3) for v in r[:3]] for r in rounds["pass_invariant"]],
                "counted": {k: {"misses": v[0], "hits": v[1]} for k, v in counts["pass_invariant"].items()},
                "cached_bits_equal_uncached": bits_inv, "bypassed": bypassed_inv},
            # a step with k of the batch's frames missing: the default mode encodes whole passes, the other mode k frames
            "partial_miss_step_ms": {mode: {names[i][len("partial_"):]: round(med[mode][i], 3) for i in range(3, len(variants))}
                                     for mode in modes},
            "gather_step": gather_alone(cache.table, shape, ae.sample, bt, 200, dev),
            "gather_table": gather_alone(cache.table, shape, ae.sample, big, 20, dev)}
    ae.cache = None
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--precisions", default="highest,medium")
    ap.add_argument("--capacity", type=int, default=8192, help="frames the table holds")
    ap.add_argument("--cases", default="ae_s2,convae")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "latent_cache_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("latent_cache_bench measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    makers = {"ae_s2": ae_s2_case, "convae": convae_case}
    for case in a.cases.split(","):
        name, model, frames, bt = makers[case](dev)
        model = model.to(dev).train()
        model.autoencoder.eval()
        model.configure_optimizers()
        for prec in a.precisions.split(","):
            pkg.set_float32_matmul_precision(prec)
            try:
                line = measure(name, model, frames, bt, prec, a, dev)
            finally:
                pkg.set_float32_matmul_precision("highest")
            print(json.dumps(line), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        del model, frames
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
