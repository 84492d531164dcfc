"""Conv latent autoencoder step (forward, Huber, backward, clip 1.0, AdamW) of pretrained_ae_convae_sevir on the gfx950
kernels, against the same network built from torch.nn modules and run eagerly on the same GPU.

    python tools/convae_bench.py [--steps 200] [--rounds 5] [--sizes 8,200]

Sizes: 8 samples of 4 x 48 x 48 (the reference config's batch) and 200 (8 SEVIR-LR sequences of 25 frames).  After a
warm-up of both, the two are alternated inside one process, `rounds` times, each round timing `steps` steps between a
pair of device events; per size one JSON line with the median and the range of the per-round ms per step of each, and the
entry-point calls of one product forward + loss + backward (ops.profile_start / profile_stop).
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as tnn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from weatherforecastingtoolkit_amd import config as C  # noqa: E402
from weatherforecastingtoolkit_amd import ops  # noqa: E402
from weatherforecastingtoolkit_amd.experiments.v1_experiments import _convae as M  # noqa: E402


class EagerConvModel(tnn.Module):
    """the reference's ConvModel written with torch.nn modules (same layers, same order)"""

    def __init__(self, latent_dim=512, c=8, cin=4, size=48):
        super().__init__()

        def unit(conv, plane):
            return tnn.Sequential(conv, tnn.LayerNorm([c, plane, plane]), tnn.LeakyReLU())

        s = size
        self.encoder = tnn.Sequential(unit(tnn.Conv2d(cin, c, 3, padding=1), s),
                                      unit(tnn.Conv2d(c, c, 4, 2, 1), s // 2), unit(tnn.Conv2d(c, c, 4, 2, 1), s // 4),
                                      unit(tnn.Conv2d(c, c, 4, 2, 1), s // 8))
        self.decoder = tnn.Sequential(unit(tnn.ConvTranspose2d(c, c, 4, 2, 1), s // 4),
                                      unit(tnn.ConvTranspose2d(c, c, 4, 2, 1), s // 2),
                                      unit(tnn.ConvTranspose2d(c, c, 4, 2, 1), s), tnn.Conv2d(c, cin, 3, padding=1))
        self.flat, self.c, self.s8 = c * (s // 8) ** 2, c, s // 8
        self.to_latent = tnn.Linear(self.flat, latent_dim)
        self.to_reconstruction = tnn.Linear(latent_dim, self.flat)

    def forward(self, x):
        b, t, c, h, w = x.shape
        y = self.encoder(x.reshape(b * t, c, h, w)).reshape(b * t, self.flat)
        y = self.to_reconstruction(self.to_latent(y)).reshape(b * t, self.c, self.s8, self.s8)
        return self.decoder(y).reshape(b, t, c, h, w)


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="8,200")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = C.load(os.path.join(os.path.dirname(M.__file__), "pretrained_ae_convae_sevir", "config.yaml"))
    cfg.convae.in_channels, cfg.convae.size = 4, 48
    cfg.trainer.total_train_steps = 10 ** 6
    for n in (int(s) for s in a.sizes.split(",")):
        torch.manual_seed(0)
        model = M.Model(cfg).to(dev).train()
        model.configure_optimizers()
        eager = EagerConvModel().to(dev).train()
        opt = torch.optim.AdamW(eager.parameters(), lr=1e-4, weight_decay=1e-2)
        crit = tnn.HuberLoss()
        x = torch.randn(n, 1, 4, 48, 48, generator=torch.Generator().manual_seed(1)).to(dev)

        def product_step():
            model.training_step(x)

        def eager_step():
            loss = crit(eager(x), x)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(eager.parameters(), 1.0)
            opt.step()

        timed(product_step, a.warmup)
        timed(eager_step, a.warmup)
        prod, eag = [], []
        for _ in range(a.rounds):
            prod.append(timed(product_step, a.steps))
            eag.append(timed(eager_step, a.steps))
        ops.profile_start()
        loss, _ = model.latent_loss(x)
        loss.backward()
        prof = ops.profile_stop()
        model.zero_grad(set_to_none=True)
        print(json.dumps({"samples": n, "steps": a.steps, "rounds": a.rounds,
                          "product_ms": round(statistics.median(prod), 4),
                          "product_ms_range": [round(min(prod), 4), round(max(prod), 4)],
                          "eager_ms": round(statistics.median(eag), 4),
                          "eager_ms_range": [round(min(eag), 4), round(max(eag), 4)],
                          "eager_over_product": round(statistics.median(eag) / statistics.median(prod), 2),
                          "entry_point_calls_fwd_loss_bwd": sum(v[0] for v in prof.values()),
                          "calls": {k: v[0] for k, v in sorted(prof.items())}}), flush=True)
        del model, eager, opt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
