"""The loader's augmenting conversion kernel (wfae_vil_augment_u8_to_f32) against the plain conversion kernel
(wfae_vil_u8_to_f32) on the same uint8 batch, in the same process.  Both read 1 byte and write 4 per pixel, so the plain
kernel is the yardstick.  Shapes: the two the experiments run (B = 32, T = 1, 384 x 384 and B = 8, T = 1, 128 x 128);
transforms: identity, a quarter turn, a generic 33.3 degrees (whose gather walks slanted lines through the source).

Timing: a launch of either kernel lasts a few microseconds, less than it takes the host to enqueue one, so a window of
`--window` launches into one preallocated output is captured in a HIP graph per variant and device events bracket its
replay: the kernels then run back to back.  The variants take turns, round after round, so that drift of the clock or of
a shared host hits all of them alike; per variant the median over `--rounds` windows, and the spread of the windows
((p90 - p10) / median) — the plain kernel's spread is what a ratio has to exceed to mean anything.  The batches fit the
256 MiB Infinity Cache, like the loader's batch that the copy engine has just written.
Appends one JSON line per shape to profiles/augment_bench.jsonl (or --out).

    python tools/augment_bench.py [--rounds 40] [--window 200] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from weatherforecastingtoolkit_amd import _lib, ops  # noqa: E402
from weatherforecastingtoolkit_amd.pipeline.datasets.sevire.sevir import transform_rows  # noqa: E402

SHAPES = [(32, 384, 384, 1), (8, 128, 128, 1)]
TRANSFORMS = {"identity": 0.0, "turn_90": 90.0, "generic_33.3": 33.3}


def capture(launch, reps):
    """a graph of `reps` launches on the capturing stream"""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            launch()
    return g


def window_us(graph, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    graph.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def spread(xs):
    q = statistics.quantiles(xs, n=10)
    return (q[-1] - q[0]) / statistics.median(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--window", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench needs a GPU: nothing here is measured on a CPU")
    dev = torch.device("cuda:0")
    for B, H, W, T in SHAPES:
        u8 = torch.randint(0, 256, (B, H, W, T), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to(dev)
        fns = {"plain": lambda: ops.vil_u8_to_f32(u8)}
        for name, angle in TRANSFORMS.items():
            rows = transform_rows([(False, False, angle)] * B).to(dev)
            fns[name] = lambda rows=rows: ops.vil_augment_u8_to_f32(u8, rows)     # also loads both kernels
        assert torch.equal(fns["identity"](), fns["plain"]())
        assert torch.equal(fns["turn_90"](), torch.rot90(fns["plain"](), 1, (2, 3)))
        dst = torch.empty((B, T, H, W), dtype=torch.float32, device=dev)
        scale = 1.0 / 255.0
        cur = lambda: torch.cuda.current_stream().cuda_stream      # noqa: E731  (the capturing stream inside capture())
        launches = {"plain": lambda: _lib.call("wfae_vil_u8_to_f32", u8.data_ptr(), dst.data_ptr(), B, H, W, T, scale,
                                               cur())}
        for name, angle in TRANSFORMS.items():
            rows = transform_rows([(False, False, angle)] * B).to(dev)
            launches[name] = lambda rows=rows: _lib.call("wfae_vil_augment_u8_to_f32", u8.data_ptr(), rows.data_ptr(),
                                                         dst.data_ptr(), B, H, W, T, scale, cur())
        torch.cuda.synchronize()
        graphs = {k: capture(fn, a.window) for k, fn in launches.items()}
        for g in graphs.values():
            for _ in range(max(1, a.warmup // 10)):
                g.replay()
        torch.cuda.synchronize()
        times = {k: [] for k in graphs}
        for _ in range(a.rounds):
            for k, g in graphs.items():
                times[k].append(window_us(g, a.window))
        nbytes = 5 * B * H * W * T
        plain = statistics.median(times["plain"])
        rec = {"B": B, "H": H, "W": W, "T": T, "bytes": nbytes, "rounds": a.rounds, "window": a.window,
               "device": torch.cuda.get_device_name(0)}
        for k, ts in times.items():
            med = statistics.median(ts)
            rec[k] = {"us": round(med, 3), "GBps": round(nbytes / med / 1e3, 1), "spread": round(spread(ts), 4),
                      "vs_plain": round(med / plain, 4)}
        print(json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
