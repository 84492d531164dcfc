"""Conv + GAN latent model step of pretrained_ae_conv_disc on the gfx950 kernels, before and after `disc_start`, against
the same network and loss built from torch.nn modules and run eagerly on the same GPU.

    python tools/conv_disc_bench.py [--steps 100] [--rounds 5] [--sizes 8,200] [--out profiles/conv_disc_bench.jsonl]

Sizes: 8 latents of 64 x 16 x 16 (the reference config's batch) and 200.  After a warm-up of all four, the product and
the eager step are alternated inside one process, `rounds` times, each round timing `steps` steps between a pair of device
events; per size one JSON line (appended to --out) with the median and the range of the per-round ms per step of each,
the entry-point calls of one product forward + loss + backward, and — for the forward of decoder.deconv.0 and
encoder.conv.6 at that size — the achieved bytes/s over the LIVE weight bytes (4 of 9 taps), event-timed over `--launches`
launches: `hot` on one weight tensor (it stays in the 256 MiB Infinity Cache), `rotating` over copies that together exceed
the cache, so that every launch streams from HBM.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as tnn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from weatherforecastingtoolkit_amd import config as C  # noqa: E402
from weatherforecastingtoolkit_amd import ops  # noqa: E402
from weatherforecastingtoolkit_amd.experiments.v1_experiments import _conv_disc as M  # noqa: E402


def eager_predictor():
    """the reference's ConvModel written with torch.nn modules (same layers, same order)"""
    def down(a, b):
        return [tnn.Conv2d(a, b, 3, stride=2, padding=1), tnn.SiLU()]

    def up(a, b):
        return [tnn.ConvTranspose2d(a, b, 3, stride=2, padding=1, output_padding=1), tnn.SiLU()]
    enc = tnn.Sequential(*down(64, 128), *down(128, 256), *down(256, 512), *down(512, 1024), tnn.Conv2d(1024, 1024, 1),
                         tnn.Flatten(), tnn.Linear(1024, 512))
    dec = tnn.Sequential(tnn.Linear(512, 1024), tnn.Unflatten(1, (1024, 1, 1)), *up(1024, 1024), *up(1024, 512),
                         *up(512, 256), *up(256, 128), tnn.Conv2d(128, 64, 1))
    return tnn.Sequential(enc, dec)


def eager_discriminator():
    def unit(a, b, s):
        return [tnn.Conv2d(a, b, 4, s, 1, bias=False), tnn.BatchNorm2d(b), tnn.LeakyReLU(0.2)]
    return tnn.Sequential(tnn.Conv2d(64, 64, 4, 2, 1), tnn.LeakyReLU(0.2), *unit(64, 128, 2), *unit(128, 256, 2),
                          *unit(256, 512, 1), tnn.Conv2d(512, 1, 1, 1, 1))


class EagerStep:
    def __init__(self, dev, gan):
        self.net, self.disc, self.gan = eager_predictor().to(dev).train(), eager_discriminator().to(dev).train(), gan
        self.g_opt = torch.optim.AdamW(self.net.parameters(), lr=5e-4, weight_decay=1e-3)
        self.d_opt = torch.optim.AdamW(self.disc.parameters(), lr=5e-6, weight_decay=1e-3, betas=(0.5, 0.999))

    def __call__(self, x):
        recon = self.net(x)
        loss = F.l1_loss(recon, x) / x.size(0)
        if self.gan:
            self.disc.requires_grad_(False)
            g_loss = -self.disc(recon).mean()
            last = self.net[1][-1].weight
            ng = torch.autograd.grad(loss, last, retain_graph=True)[0]
            gg = torch.autograd.grad(g_loss, last, retain_graph=True)[0]
            loss = loss + torch.clamp(ng.norm() / (gg.norm() + 1e-4), 0.0, 1e4).detach() * g_loss
        self.g_opt.zero_grad(set_to_none=True)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(self.net.parameters(), 1.0)
        self.g_opt.step()
        if self.gan:
            self.disc.requires_grad_(True)
            d_loss = 0.5 * (F.relu(1.0 - self.disc(x)).mean() + F.relu(1.0 + self.disc(recon.detach())).mean())
            self.d_opt.zero_grad(set_to_none=True)
            d_loss.backward()
            torch.nn.utils.clip_grad_norm_(self.disc.parameters(), 1.0)
            self.d_opt.step()


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def stream_rate(dev, n, chi, clo, transposed, launches):
    """forward of one 2x2 <-> 1x1 layer: live weight bytes / time per launch, hot and rotating"""
    live = clo * chi * 4 * 4
    copies = (300 << 20) // (clo * chi * 9 * 4) + 1
    ws = [torch.randn(clo, chi, 3, 3, device=dev) * 0.01 for _ in range(copies)]
    x = torch.randn(n, clo, 1, 1, device=dev) if transposed else torch.randn(n, chi, 2, 2, device=dev)
    b = torch.zeros(chi if transposed else clo, device=dev)
    out = {"live_weight_bytes": live}
    for name, pick in (("hot", lambda i: ws[0]), ("rotating", lambda i: ws[i % copies])):
        for i in range(copies):
            ops.c3s2_fwd(x, pick(i), b, transposed, True, 1, save_t=True)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(launches):
            ops.c3s2_fwd(x, pick(i), b, transposed, True, 1, save_t=True)
        e1.record()
        torch.cuda.synchronize()
        us = 1e3 * e0.elapsed_time(e1) / launches
        out[name] = {"us_per_call": round(us, 2), "live_TB_per_s": round(live / us / 1e6, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--sizes", default="8,200")
    ap.add_argument("--out", default=os.path.join("profiles", "conv_disc_bench.jsonl"))
    a = ap.parse_args()
    if a.launches < 50:
        raise SystemExit("--launches: at least 50")
    dev = torch.device("cuda:0")
    cfg = C.load(os.path.join(os.path.dirname(M.__file__), "pretrained_ae_conv_disc", "config.yaml"))
    cfg.trainer.total_train_steps = 10 ** 6
    for n in (int(s) for s in a.sizes.split(",")):
        x = torch.randn(n, 1, 64, 16, 16, generator=torch.Generator().manual_seed(1)).to(dev)
        xe = x.view(n, 64, 16, 16)
        rec = {"samples": n, "steps": a.steps, "rounds": a.rounds}
        for phase, start in (("pre_start", 10 ** 9), ("post_start", 0)):
            torch.manual_seed(0)
            cfg.lpips.disc_start = start
            model = M.Model(cfg).to(dev).train()
            model.configure_optimizers()
            eager = EagerStep(dev, start == 0)
            timed(lambda: model.training_step(x), a.warmup)
            timed(lambda: eager(xe), a.warmup)
            prod, eag = [], []
            for _ in range(a.rounds):
                prod.append(timed(lambda: model.training_step(x), a.steps))
                eag.append(timed(lambda: eager(xe), a.steps))
            ops.profile_start()
            model.training_step(x)
            prof = ops.profile_stop()
            rec[phase] = {"product_ms": round(statistics.median(prod), 4),
                          "product_ms_range": [round(min(prod), 4), round(max(prod), 4)],
                          "eager_ms": round(statistics.median(eag), 4),
                          "eager_ms_range": [round(min(eag), 4), round(max(eag), 4)],
                          "eager_over_product": round(statistics.median(eag) / statistics.median(prod), 2),
                          "entry_point_calls_step": sum(v[0] for v in prof.values()),
                          "calls": {k: v[0] for k, v in sorted(prof.items())}}
            del model, eager
            torch.cuda.empty_cache()
        rec["fwd_decoder_deconv_0"] = stream_rate(dev, n, 1024, 1024, True, a.launches)
        rec["fwd_encoder_conv_6"] = stream_rate(dev, n, 512, 1024, False, a.launches)
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
