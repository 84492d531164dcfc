"""The loader's pooling conversion kernel (wfae_vil_pool_u8_to_f32, mode max) against what the package could do with the
same bytes before it existed: the plain conversion kernel (wfae_vil_u8_to_f32) on the selected frames, then
torch.nn.functional.max_pool2d on the device.  Shapes: the AE batch (32, 384, 384, 1) at factors (1, 3, 3) and the
forecaster batch (8, 384, 384, 49) at (2, 3, 3) — raw SEVIR pooled to sevir_lr.

Variants (all produce bit-equal output, asserted before anything is timed):
    fused            the kernel as the library dispatches it (T == 1: row reads; T > 1: LDS-staged row segments)
    fused_direct     T > 1 only: the direct gather (WFAE_VIL_POOL_STAGED=0) — the other read path, timed to choose
    composed         plain kernel + max_pool2d; the frames [::ft] were selected beforehand and are not timed — the yardstick
    composed_select  the same with the device-side frame selection (u8[..., ::ft].contiguous()) inside the window

Timing as in tools/augment_bench.py: a window of `--window` launches is captured in a HIP graph per variant and device
events bracket its replay; the variants take turns, round after round; per variant the median over `--rounds` windows and
the spread of the windows ((p90 - p10) / median).  `fused` has to beat `composed` by more than composed's own spread for
the ratio to mean anything.  Appends one JSON line per shape to profiles/vil_pool_bench.jsonl (or --out).

    python tools/vil_pool_bench.py [--rounds 40] [--window 100] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from weatherforecastingtoolkit_amd import _lib, ops  # noqa: E402

CASES = [((32, 384, 384, 1), (1, 3, 3)), ((8, 384, 384, 49), (2, 3, 3))]
SWITCH = "WFAE_VIL_POOL_STAGED"


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
    ap.add_argument("--window", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3, help="untimed replays of every graph")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vil_pool_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vil_pool_bench needs a GPU: nothing here is measured on a CPU")
    dev = torch.device("cuda:0")
    os.environ.pop(SWITCH, None)
    scale = 1.0 / 255.0
    for (B, H, W, T), (ft, fh, fw) in CASES:
        u8 = torch.randint(0, 256, (B, H, W, T), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to(dev)
        sel = u8[..., ::ft].contiguous()
        To, Ho, Wo = sel.shape[3], -(-H // fh), -(-W // fw)
        dst = torch.empty((B, To, Ho, Wo), dtype=torch.float32, device=dev)
        cur = lambda: torch.cuda.current_stream().cuda_stream      # noqa: E731  (the capturing stream inside capture())

        def fused():
            _lib.call("wfae_vil_pool_u8_to_f32", u8.data_ptr(), None, dst.data_ptr(), B, H, W, T, ft, fh, fw, 0, scale, 0.0,
                      cur())

        def composed():
            return F.max_pool2d(ops.vil_u8_to_f32(sel), (fh, fw), ceil_mode=True)

        def composed_select():
            return F.max_pool2d(ops.vil_u8_to_f32(u8[..., ::ft].contiguous()), (fh, fw), ceil_mode=True)

        launches = {"fused": (fused, None), "composed": (composed, None), "composed_select": (composed_select, None)}
        if T > 1:
            launches["fused_direct"] = (fused, "0")
        want = composed()                                          # also loads the kernels outside any capture
        assert torch.equal(composed_select(), want)
        graphs = {}
        for k, (fn, switch) in launches.items():
            if switch is not None:
                os.environ[SWITCH] = switch                        # read by the library on every call
            try:
                if fn is fused:
                    dst.fill_(-1.0)
                    fn()
                    torch.cuda.synchronize()
                    assert torch.equal(dst, want), k
                torch.cuda.synchronize()
                graphs[k] = capture(fn, a.window)
            finally:
                os.environ.pop(SWITCH, None)
        for g in graphs.values():
            for _ in range(max(1, a.warmup)):
                g.replay()
        torch.cuda.synchronize()
        times = {k: [] for k in graphs}
        for _ in range(a.rounds):
            for k, g in graphs.items():
                times[k].append(window_us(g, a.window))
        yard = statistics.median(times["composed"])
        rec = {"B": B, "H": H, "W": W, "T": T, "factors": [ft, fh, fw], "bytes_in": u8.numel(), "bytes_out": 4 * dst.numel(),
               "rounds": a.rounds, "window": a.window, "device": torch.cuda.get_device_name(0)}
        for k, ts in times.items():
            med = statistics.median(ts)
            rec[k] = {"us": round(med, 3), "spread": round(spread(ts), 4), "vs_composed": round(med / yard, 4)}
        rec["fused_beats_composed_by_more_than_its_spread"] = bool(
            rec["fused"]["us"] < yard * (1.0 - rec["composed"]["spread"]))
        print(json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
        del graphs


if __name__ == "__main__":
    main()
