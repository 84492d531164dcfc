"""Evaluation forward of the ae_gan residual autoencoder (ConvAutoencoderBIG) on csrc/resae.hip.

    python tools/resae_bench.py [--steps 50] [--rounds 5] [--out profiles/resae_bench.jsonl]

Two kinds of JSON lines are appended to --out, all from one process:
  {"layer": ...}  for every launch of ConvAutoencoderBIG on 128 x 128 frames whose output plane has at most 16 pixels (the
      set the small-plane route serves), at B = 8 and B = 32: the time of the small-plane route and of the tile route forced
      on the same input (alternated, median of `rounds` windows of `steps` launches between a pair of device events), the
      live weight bytes (4 bytes x Cout x Cin x live taps) over the small route's time, and that rate as a fraction of the
      HBM roof (8 TB/s, MI355X).  Weights of a layer above the 256 MiB last-level cache are streamed from HBM on every launch;
      smaller ones may be served from the cache in this loop, which the line says (`weights_fit_llc`).
  {"model": ...}  the whole evaluation forward at B = 8 (the experiment's batch) against the same architecture written
      with torch.nn modules inside this file and run by torch in eval mode on the same GPU, alternated the same way, plus the
      per-label kernel times of one product forward.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as tnn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from weatherforecastingtoolkit_amd import ops  # noqa: E402
from weatherforecastingtoolkit_amd.experiments.v1_experiments import _ae_gan as M  # noqa: E402

ENC = [(1, 64), (64, 128), (128, 256), (256, 512), (512, 1024), (1024, 2048), (2048, 2048)]
DEC = [(2048, 1024), (1024, 512), (512, 256), (256, 128), (128, 64), (64, 64), (64, 32)]
LLC_BYTES = 256 << 20


class EagerBlock(tnn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1, self.bn1 = tnn.Conv2d(cin, cout, 3, stride, 1, bias=False), tnn.BatchNorm2d(cout)
        self.conv2, self.bn2 = tnn.Conv2d(cout, cout, 3, 1, 1, bias=False), tnn.BatchNorm2d(cout)
        self.shortcut = tnn.Sequential()
        if stride != 1 or cin != cout:
            self.shortcut = tnn.Sequential(tnn.Conv2d(cin, cout, 1, stride, bias=False), tnn.BatchNorm2d(cout))
        self.act = tnn.GELU()

    def forward(self, x):
        return self.act(self.bn2(self.conv2(self.act(self.bn1(self.conv1(x))))) + self.shortcut(x))


class EagerBig(tnn.Module):
    """ConvAutoencoderBIG written with torch.nn modules (same layers, same order)"""

    def __init__(self):
        super().__init__()
        self.enc = tnn.Sequential(*[EagerBlock(ci, co, 2) for ci, co in ENC])
        self.fc_enc, self.fc_dec = tnn.Linear(2048, 2048), tnn.Linear(2048, 2048)
        self.dec = tnn.Sequential(*[tnn.Sequential(tnn.Upsample(scale_factor=2, mode="nearest"), EagerBlock(ci, co, 1))
                                    for ci, co in DEC])
        self.final_conv = tnn.Conv2d(32, 1, 3, 1, 1)

    def forward(self, x):
        z = self.fc_enc(self.enc(x).flatten(1))
        return self.final_conv(self.dec(self.fc_dec(z)[:, :, None, None])), z


def small_layers():
    """(name, kind, Cin, Cout, H, W) of the launches of ConvAutoencoderBIG that resae_route sends to the small-plane route"""
    out, s = [], 128
    for i, (ci, co) in enumerate(ENC, 1):
        out += [(f"enc{i}.shortcut", 4, ci, co, s, s), (f"enc{i}.conv1", 1, ci, co, s, s), (f"enc{i}.conv2", 0, co, co, s // 2, s // 2)]
        s //= 2
    for i, (ci, co) in enumerate(DEC, 1):
        if ci != co:
            out.append((f"dec{i}.shortcut", 3, ci, co, s, s))
        out += [(f"dec{i}.conv1", 2, ci, co, s, s), (f"dec{i}.conv2", 0, co, co, 2 * s, 2 * s)]
        s *= 2
    return [l for l in out if ops.resae_route(l[1], 8, *l[2:]) == "small"]


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def alternate(fa, fb, steps, rounds, warmup):
    timed(fa, warmup)
    timed(fb, warmup)
    a, b = [], []
    for _ in range(rounds):
        a.append(timed(fa, steps))
        b.append(timed(fb, steps))
    return a, b


def ms(v):
    return {"ms": round(statistics.median(v), 5), "ms_range": [round(min(v), 5), round(max(v), 5)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "resae_bench.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    lines = []
    mode = ops.aekl_mode()
    for name, kind, cin, cout, h, w in small_layers():
        k = 1 if kind >= 3 else 3
        wt = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5).to(dev)
        scale, shift = torch.rand(cout, generator=g).to(dev) + 0.5, torch.randn(cout, generator=g).to(dev)
        ps, pt = ops.resae_pack(wt, kind, "small", mode), ops.resae_pack(wt, kind, "tile", mode)
        taps = sum(map(sum, ops.resae_live_taps(kind, h, w)))
        live_bytes = 4 * cout * cin * taps
        for n in (8, 32):
            x = torch.randn(n, cin, h, w, generator=g).to(dev)
            small, tile = alternate(lambda: ops.resae_conv(x, ps, scale, shift, act=True, route="small"),
                                    lambda: ops.resae_conv(x, pt, scale, shift, act=True, route="tile"), a.steps, a.rounds, a.warmup)
            gbs = live_bytes / (statistics.median(small) * 1e-3) / 1e9
            lines.append({"layer": name, "kind": kind, "cin": cin, "cout": cout, "plane_in": [h, w], "batch": n, "tile_mode": mode,
                          "live_taps": taps, "live_weight_bytes": live_bytes, "weights_fit_llc": live_bytes <= LLC_BYTES,
                          "small": ms(small), "tile": ms(tile),
                          "tile_over_small": round(statistics.median(tile) / statistics.median(small), 2),
                          "small_slowest_below_tile_fastest": max(small) < min(tile),
                          "small_live_gb_per_s": round(gbs, 1), "small_fraction_of_hbm_roof": round(gbs * 1e9 / ops.PEAK_HBM, 4)})
            print(json.dumps(lines[-1]), flush=True)
        del wt, ps, pt

    torch.manual_seed(0)
    model = M.ConvAutoencoderBIG().to(dev)
    eager = EagerBig().to(dev).eval()
    x = torch.rand(8, 1, 128, 128, generator=g).to(dev)

    def run_eager():
        with torch.no_grad():
            eager(x)
    steps = max(1, a.steps // 2)
    prod, eag = alternate(lambda: model(x), run_eager, steps, a.rounds, a.warmup)
    ops.profile_start()
    model(x)
    prof = ops.profile_stop()
    lines.append({"model": "ConvAutoencoderBIG eval forward", "batch": 8, "steps": steps, "rounds": a.rounds, "tile_mode": mode,
                  "product": ms(prod), "eager": ms(eag),
                  "eager_over_product": round(statistics.median(eag) / statistics.median(prod), 2),
                  "product_slowest_below_eager_fastest": max(prod) < min(eag),
                  "entry_point_calls": sum(v[0] for v in prof.values()),
                  "ms_by_label": {k: round(v[1], 4) for k, v in sorted(prof.items(), key=lambda kv: -kv[1][1])}})
    print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for l in lines:
            f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
