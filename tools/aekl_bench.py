"""Frozen AutoencoderKL latent provider on the gfx950 kernels against the same network run eagerly by torch on the same
GPU (tests/aekl_ref.py, the plain-torch restatement).

    python tools/aekl_bench.py [--steps 5] [--rounds 3] [--cases 128,384] [--layer-only]

Cases: 8 frames of 128 x 128 with 64 latent channels, and 4 frames of 384 x 384 with 4 latent channels (the reference
configuration of the v1 experiments).  Per case and per precision ('highest', 'medium') one JSON line: ms per frame of
encode (mode) and decode for the product and for eager torch (alternated inside one process, `rounds` rounds of `steps`
calls between a pair of device events, medians), the FLOPs per frame counted by torch's FLOP counter on the eager
network, and the achieved TFLOP/s of the 3x3 kernel per layer shape (ops.profile_start / profile_stop labels).
First line: the 128-channel 128 x 128 layer (stride 1, prologue on) in the three operand forms of the 3x3 kernel — three
exact bf16 planes, fp32 MFMA, one bf16 plane — the measurement behind the choice of the 'highest' form.
Second line: the FLOP counter at the configuration of the figures quoted in DESIGN.md, one 384 x 384 frame at 64 latent
channels, against them (622 GFLOP encode, 1407 GFLOP decode).
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
from tests import aekl_ref as A  # noqa: E402
from weatherforecastingtoolkit_amd import ops  # noqa: E402
from weatherforecastingtoolkit_amd.pipeline.models.autoencoderkl import AutoencoderKL  # noqa: E402

CASES = {"128": ("ref64", 8, 128), "384": ("ref4", 4, 384)}


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def layer_comparison(dev, steps, rounds):
    """Cin = Cout = 128 at 128 x 128, 8 frames, GroupNorm + SiLU prologue and residual: ms and TFLOP/s per operand form"""
    n, c, s = 8, 128, 128
    g = torch.Generator().manual_seed(0)
    x = torch.randn(n, c, s, s, generator=g).to(dev)
    w = (torch.randn(c, c, 3, 3, generator=g) * (9 * c) ** -0.5).to(dev)
    b = torch.zeros(c, device=dev)
    gn = (torch.ones(n, c, device=dev), torch.zeros(n, c, device=dev))
    flops = 2 * 9 * n * s * s * c * c
    out = {"layer": f"{c}->{c} {s}x{s} n{n}", "gflop": round(flops / 1e9, 2)}
    for name, mode in ops.AEKL_MODES.items():
        packed = ops.aekl_conv3_pack(w, mode)
        fn = lambda: ops.aekl_conv3_fwd(x, packed, c, b, gn, x, 0, mode)  # noqa: E731
        timed(fn, 3)
        ms = statistics.median(timed(fn, steps) for _ in range(rounds))
        out[name] = {"ms": round(ms, 4), "tflops": round(flops / ms / 1e9, 1)}
    y = torch.nn.functional
    xin = y.silu(x)
    fn = lambda: y.conv2d(xin, w, b, padding=1)  # noqa: E731
    timed(fn, 3)
    ms = statistics.median(timed(fn, steps) for _ in range(rounds))
    out["torch_conv2d_fp32"] = {"ms": round(ms, 4), "tflops": round(flops / ms / 1e9, 1)}
    print(json.dumps(out), flush=True)


def count_flops(sd, cfg, x, z):
    from torch.utils.flop_counter import FlopCounterMode
    with torch.no_grad():
        with FlopCounterMode(display=False) as fe:
            A.encode(sd, x[:1], cfg)
        with FlopCounterMode(display=False) as fd:
            A.decode(sd, z[:1], cfg)
    return fe.get_total_flops(), fd.get_total_flops()


def flop_cross_check(dev):
    """the configuration of the quoted figures — 64 latent channels, one 384 x 384 frame: 622 GFLOP encode, 1407 decode"""
    cfg = A.CONFIGS["ref64"]
    torch.manual_seed(0)
    sd = {k: v.detach().to(dev) for k, v in AutoencoderKL(**cfg).state_dict().items()}
    x = torch.rand(1, 1, 384, 384, device=dev)
    with torch.no_grad():
        z = A.encode(sd, x, cfg)["mode"]
    fe, fd = count_flops(sd, cfg, x, z)
    print(json.dumps({"flop_cross_check": "ref64 1x384x384", "encode_gflop": round(fe / 1e9, 1),
                      "decode_gflop": round(fd / 1e9, 1), "expected": [622, 1407],
                      "agrees": abs(fe / 622e9 - 1) < 5e-3 and abs(fd / 1407e9 - 1) < 5e-3}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", default="128,384")
    ap.add_argument("--precisions", default="highest,medium")
    ap.add_argument("--layer-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    layer_comparison(dev, max(a.steps, 10), a.rounds)
    if a.layer_only:
        return
    torch.backends.cuda.matmul.allow_tf32 = False
    flop_cross_check(dev)
    for key in a.cases.split(","):
        name, n, size = CASES[key]
        cfg = A.CONFIGS[name]
        torch.manual_seed(0)
        model = AutoencoderKL(**cfg).to(dev)
        sd = {k: v.detach() for k, v in model.state_dict().items()}
        x = torch.rand(n, 1, size, size, generator=torch.Generator().manual_seed(1)).to(dev)
        for prec in a.precisions.split(","):
            pkg.set_float32_matmul_precision(prec)
            torch.set_float32_matmul_precision(prec)
            try:
                z = model.encode(x).mode()
                fe, fd = count_flops(sd, cfg, x, z)
                with torch.no_grad():
                    ze = A.encode(sd, x, cfg)["mode"]
                    parity = {"z": A.rel_err(z, ze), "decode": A.rel_err(model.decode(z), A.decode(sd, z, cfg))}
                fns = {"encode": lambda: model.encode(x).mode(), "decode": lambda: model.decode(z)}
                with torch.no_grad():
                    efn = {"encode": lambda: A.encode(sd, x, cfg)["mode"], "decode": lambda: A.decode(sd, z, cfg)}
                    res = {}
                    for what in ("encode", "decode"):
                        timed(fns[what], 1)
                        timed(efn[what], 1)
                        prod, eag = [], []
                        for _ in range(a.rounds):
                            prod.append(timed(fns[what], a.steps) / n)
                            eag.append(timed(efn[what], a.steps) / n)
                        res[what] = {"product_ms_per_frame": round(statistics.median(prod), 3),
                                     "eager_ms_per_frame": round(statistics.median(eag), 3),
                                     "eager_over_product": round(statistics.median(eag) / statistics.median(prod), 2)}
                ops.profile_start()
                model.decode(model.encode(x).mode())
                prof = ops.profile_stop()
                layers = {k.split(" ", 1)[1]: {"calls": v[0], "ms": round(v[1], 3), "tflops": round(v[2] / v[1] / 1e9, 1)}
                          for k, v in sorted(prof.items()) if k.startswith("wfae_aekl_conv3_fwd ")}
                conv_ms = sum(v[1] for k, v in prof.items() if k.startswith("wfae_aekl_conv3_fwd "))
                other = {k: round(v[1], 3) for k, v in sorted(prof.items()) if not k.startswith("wfae_aekl_conv3_fwd ")}
                print(json.dumps({"case": f"{n}x{size}x{size} latent {cfg['latent_channels']}", "precision": prec,
                                  "conv3_mode": ops.aekl_mode(), **res,
                                  "gflop_per_frame": {"encode": round(fe / 1e9, 1), "decode": round(fd / 1e9, 1)},
                                  "parity_vs_eager": parity, "conv3_ms_total": round(conv_ms, 3), "conv3_layers": layers,
                                  "other_entry_points_ms": other}), flush=True)
            finally:
                pkg.set_float32_matmul_precision("highest")
                torch.set_float32_matmul_precision("highest")
        del model, sd
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
