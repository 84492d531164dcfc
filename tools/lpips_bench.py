"""LPIPS perceptual loss (csrc/lpips.hip) on the MI355X: forward, and forward + backward to the first image.

    python tools/lpips_bench.py [--steps 5] [--rounds 3] [--cases 32x384,8x128] [--out profiles/lpips_bench.jsonl]

Cases: (32, 1, 384, 384) — the AE+GAN step's batch — and (8, 1, 128, 128), at 'highest' (conv mode 3: three exact bf16
planes, six matrix instructions per product) and 'medium' (mode 1: one plane).  Per case and precision one JSON line is
appended to --out: median ms of `rounds` rounds of `steps` calls between a pair of device events, the convolution FLOPs of
the call (two VGG16 forwards per sample; forward + backward adds one backward-data pass over the first image), the
achieved fp32-equivalent TFLOP/s and the implied fraction of the dense bf16 MFMA peak (mode 3 issues six bf16 products per
fp32 product), and the time per entry point of one forward + backward (ops.profile_start / profile_stop).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import weatherforecastingtoolkit_amd as pkg  # noqa: E402
from weatherforecastingtoolkit_amd import ops  # noqa: E402
from weatherforecastingtoolkit_amd.pipeline.models.autoencoderkl.losses import LPIPS  # noqa: E402
from weatherforecastingtoolkit_amd.pipeline.models.autoencoderkl.losses.lpips import VGG16_CONVS, VGG16_POOLS  # noqa: E402

CASES = {"32x384": (32, 384), "8x128": (8, 128)}


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def vgg_flops(size):
    """FLOPs of the 13 convolutions of one VGG16-features pass over one size x size image (backward-data has the forward's
    FLOPs layer by layer)"""
    total, s = 0, size
    for idx in range(30):
        if idx in VGG16_POOLS:
            s //= 2
        elif idx in VGG16_CONVS:
            ci, co = VGG16_CONVS[idx]
            total += 2 * 9 * s * s * ci * co
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", default="32x384,8x128")
    ap.add_argument("--precisions", default="highest,medium")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_bench.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    model = LPIPS().to(dev)
    for key in a.cases.split(","):
        n, size = CASES[key]
        g = torch.Generator().manual_seed(1)
        t = torch.rand(n, 1, size, size, generator=g)
        x = (t + 0.2 * torch.randn(n, 1, size, size, generator=g)).clamp(0, 1).to(dev).requires_grad_(True)
        t = t.to(dev)
        per_pass = n * vgg_flops(size)
        torch.cuda.reset_peak_memory_stats()
        for prec in a.precisions.split(","):
            pkg.set_float32_matmul_precision(prec)
            try:
                mode = ops.aekl_mode()

                def fwd():
                    with torch.no_grad():
                        return model(x, t)

                def fwd_bwd():
                    x.grad = None
                    model(x, t).mean().backward()

                res = {}
                for what, fn, passes in (("forward", fwd, 2), ("forward_backward", fwd_bwd, 3)):
                    timed(fn, 1)
                    ms = statistics.median(timed(fn, a.steps) for _ in range(a.rounds))
                    tf = passes * per_pass / ms / 1e9
                    res[what] = {"ms": round(ms, 3), "ms_per_sample": round(ms / n, 4), "conv_gflop": round(passes * per_pass / 1e9, 1),
                                 "tflops_fp32_equivalent": round(tf, 1),
                                 "fraction_of_bf16_mfma_peak": round(tf * 1e12 * (6 if mode == 3 else 1) / ops.PEAK_BF16_MFMA, 4)}
                ops.profile_start()
                fwd_bwd()
                prof = ops.profile_stop()
                by_entry = {}
                for k, v in prof.items():
                    by_entry[k.split(" ", 1)[0]] = round(by_entry.get(k.split(" ", 1)[0], 0.0) + v[1], 3)
                layers = {k.split("wfae_lpips_", 1)[1]: {"ms": round(v[1], 3), "tflops": round(v[2] / v[1] / 1e9, 1)}
                          for k, v in sorted(prof.items()) if k.startswith("wfae_lpips_conv3")}
                line = {"case": f"{n}x1x{size}x{size}", "precision": prec, "conv3_mode": mode,
                        "gflop_per_image_per_pass": round(vgg_flops(size) / 1e9, 2), **res, "entry_points_ms": by_entry,
                        "conv3_layers": layers, "peak_memory_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
                print(json.dumps(line), flush=True)
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(json.dumps(line) + "\n")
            finally:
                pkg.set_float32_matmul_precision("highest")
        del x, t
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
