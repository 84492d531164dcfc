"""Training the AutoencoderKL on the gfx950 kernels (csrc/aekl.hip + csrc/aekl_bwd.hip) against the same loss run eagerly by
torch on the same GPU (tests/aekl_train_ref.py over tests/aekl_ref.py).

    python tools/aekl_train_bench.py [--steps 3] [--rounds 3] [--cases ae_gan_kl,ref64] [--out profiles/aekl_train_bench.jsonl]

Cases: "ae_gan_kl" — the five-level autoencoder of experiments/v1_experiments/ae_gan_kl ((64, 128, 256, 512, 512), 512 latent
channels, one layer per block), 8 frames of 1 x 128 x 128 — and "ref64" (tests/aekl_ref.py), 8 frames of 1 x 128 x 128.
Per case and precision ('highest', 'medium') one JSON line: ms per step of forward + backward of L1 + 1e-2 KL / B + an
AdamW step for the product (FusedAdamW) and for eager torch (torch.optim.AdamW), alternated inside one process, `rounds`
rounds of `steps` steps between a pair of device events, medians; and per 3x3 layer shape of the step the ms of the
weight-gradient, data-gradient and forward kernels of that shape (ops.profile_start / profile_stop labels, summed over the
layers of the shape), the weight gradient's achieved TFLOP/s and its time over the forward's.  They do the same arithmetic.
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
from tests import aekl_train_ref as T  # noqa: E402
from weatherforecastingtoolkit_amd import functional as Fn  # noqa: E402
from weatherforecastingtoolkit_amd import ops  # noqa: E402
from weatherforecastingtoolkit_amd.optim import FusedAdamW  # noqa: E402
from weatherforecastingtoolkit_amd.pipeline.models.autoencoderkl import AutoencoderKL  # noqa: E402

AE_GAN_KL = dict(in_channels=1, out_channels=1, down_block_types=("DownEncoderBlock2D",) * 5,
                 up_block_types=("UpDecoderBlock2D",) * 5, block_out_channels=(64, 128, 256, 512, 512), layers_per_block=1,
                 act_fn="silu", latent_channels=512, norm_num_groups=32)
CASES = {"ae_gan_kl": (AE_GAN_KL, 8, 128), "ref64": (A.CONFIGS["ref64"], 8, 128)}


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def product_step(model, opt, x, noise):
    post = model.encode(x)
    loss = Fn.l1_loss(model.decode(post.sample(noise=noise)), x) + T.KL_WEIGHT * post.kl().sum() / x.shape[0]
    loss.backward()
    opt.step()
    opt.zero_grad(set_to_none=True)
    return loss


def eager_step(leaves, opt, x, noise, cfg):
    loss, _ = T.loss_of(leaves, x, cfg, noise)
    loss.backward()
    opt.step()
    opt.zero_grad(set_to_none=True)
    return loss


def per_shape(prof):
    """{"k<kind> Cin->Cout HxW": {fwd_ms, wgrad_ms, dgrad_ms, layers, wgrad_tflops, wgrad_over_fwd}}"""
    shapes = {}
    for label, v in prof.items():
        name, _, shape = label.partition(" ")
        key = {"wfae_aekl_conv3_fwd": "fwd", "wfae_aekl_conv3_bwd_weight": "wgrad", "wfae_aekl_conv3_bwd_data": "dgrad"}.get(name)
        if key is None or not shape:
            continue
        if key == "dgrad":      # labelled Cout->Cin: turn it round
            k, io, hw = shape.split(" ")
            o, i = io.split("->")
            shape = f"{k} {i}->{o} {hw}"
        d = shapes.setdefault(shape, {})
        d[key + "_ms"] = round(v[1], 4)
        if key == "wgrad":
            d["layers"], d["wgrad_tflops"] = v[0], round(v[2] / v[1] / 1e9, 1)
    for d in shapes.values():
        if "fwd_ms" in d and "wgrad_ms" in d:
            d["wgrad_over_fwd"] = round(d["wgrad_ms"] / d["fwd_ms"], 2)
    return shapes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", default="ae_gan_kl,ref64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aekl_train_bench.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for case in args.cases.split(","):
        cfg, n, size = CASES[case]
        for precision in ("highest", "medium"):
            pkg.set_float32_matmul_precision(precision)
            torch.manual_seed(0)
            model = AutoencoderKL(**cfg).to(dev).unfreeze().train()
            opt = FusedAdamW(model.parameters(), lr=1e-5, weight_decay=1e-4)
            x = torch.rand(n, 1, size, size, generator=torch.Generator().manual_seed(1)).to(dev)
            lat = size // model.downscale
            noise = torch.randn(n, cfg["latent_channels"], lat, lat, generator=torch.Generator().manual_seed(2)).to(dev)
            leaves = {k: v.detach().clone().requires_grad_(True) for k, v in model.state_dict().items()}
            eopt = torch.optim.AdamW(list(leaves.values()), lr=1e-5, weight_decay=1e-4)
            prod = lambda: product_step(model, opt, x, noise)  # noqa: E731
            eager = lambda: eager_step(leaves, eopt, x, noise, cfg)  # noqa: E731
            lp, le = float(prod()), float(eager())      # warm-up, and the two losses of the first step side by side
            prod(), eager()
            pm, em = [], []
            for _ in range(args.rounds):
                pm.append(timed(prod, args.steps))
                em.append(timed(eager, args.steps))
            ops.profile_start()
            prod()
            prof = ops.profile_stop()
            pkg.set_float32_matmul_precision("highest")
            p, e = statistics.median(pm), statistics.median(em)
            line = {"case": f"{case} {n}x1x{size}x{size}", "precision": precision, "conv3_mode": ops.AEKL_MODES["bf16" if precision == "medium" else "split3"],
                    "first_loss": {"product": round(lp, 6), "eager": round(le, 6)},
                    "step_ms": {"product": round(p, 3), "eager": round(e, 3), "eager_over_product": round(e / p, 2)},
                    "kernel_ms_in_one_step": {k.split(" ")[0]: 0 for k in prof}, "conv3_shapes": per_shape(prof)}
            for k, v in prof.items():
                line["kernel_ms_in_one_step"][k.split(" ")[0]] = round(line["kernel_ms_in_one_step"][k.split(" ")[0]] + v[1], 3)
            print(json.dumps(line), flush=True)
            lines.append(line)
            del model, opt, leaves, eopt
            torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
