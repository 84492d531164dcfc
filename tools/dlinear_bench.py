"""DLinear predictor step (target, forward, MSE, backward, clip 1.0, AdamW) of the three v1 DLinear experiments at the
reference size — B = 8, 25 latent frames of 4 x 48 x 48 — on the gfx950 kernels, against a torch-eager restatement of
the reference's per-column module loop (train.py:83-100 with `individual: true`; one nn.Linear pair per column) on the
same GPU.  Prints one JSON line per variant.

    python tools/dlinear_bench.py [--steps 20] [--eager-steps 3]

Kernel time is also reported against a bytes / HBM-roof estimate: per step the weights are read by the forward,
their gradients written by the backward, read twice and written once by the clip, and AdamW reads p, g, m, v and
writes p, m, v; activations (latents, prediction, target, dy) add a few MB.
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn as tnn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from weatherforecastingtoolkit_amd import config as C  # noqa: E402
from weatherforecastingtoolkit_amd.experiments.v1_experiments import _dlinear as D  # noqa: E402

HBM_PEAK = 8.0e12    # MI355X HBM3E peak, bytes/s
VARIANTS = {"sevir": (False, 3, 1), "ind": (True, 3, 1), "indc_indp": (True, 5, 4)}
B, TIN, TOUT, LAT = 8, 13, 12, (4, 48, 48)


class EagerDLinear(tnn.Module):
    """the reference's DLinear forward, written out with the same module structure (per-column loop when individual)"""

    def __init__(self, L, P, M, K, individual):
        super().__init__()
        self.K, self.individual, self.M = K, individual, M
        n = M if individual else 1
        self.S = tnn.ModuleList(tnn.Linear(L, P) for _ in range(n))
        self.T = tnn.ModuleList(tnn.Linear(L, P) for _ in range(n))
        self.P = P

    def forward(self, x):
        h = (self.K - 1) // 2
        xp = torch.cat([x[:, :1].repeat(1, h, 1), x, x[:, -1:].repeat(1, h, 1)], 1)
        t = F.avg_pool1d(xp.permute(0, 2, 1), self.K, 1).permute(0, 2, 1)
        s = (x - t).permute(0, 2, 1)
        t = t.permute(0, 2, 1)
        if self.individual:
            so = torch.zeros(s.size(0), s.size(1), self.P, device=s.device)
            to = torch.zeros_like(so)
            for i in range(self.M):
                so[:, i, :] = self.S[i](s[:, i, :])
                to[:, i, :] = self.T[i](t[:, i, :])
        else:
            so, to = self.S[0](s), self.T[0](t)
        return (so + to).permute(0, 2, 1)


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--eager-steps", type=int, default=3)
    ap.add_argument("--variants", default=",".join(VARIANTS))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    c, h, w = LAT
    for name in a.variants.split(","):
        individual, K, cf = VARIANTS[name]
        M, L, P = c * h * w // cf, TIN * cf, TOUT * cf
        cfg = C.load(os.path.join(os.path.dirname(D.__file__), f"pretrained_ae_dlinear_{name}", "config.yaml"))
        cfg.dlinear.enc_in, cfg.dlinear.features_per_step = M, cf
        cfg.trainer.total_train_steps = 10 ** 6
        torch.manual_seed(0)
        model = D.Model(cfg).to(dev).train()
        model.configure_optimizers()
        g = torch.Generator().manual_seed(1)
        v = torch.randn(B, TIN + TOUT, c, h, w, generator=g).to(dev)
        ms = timed(lambda: model.training_step(v), a.warmup, a.steps)

        wbytes = 4 * sum(p.numel() for p in (model.predictor.seasonal_weight, model.predictor.seasonal_bias,
                                             model.predictor.trend_weight, model.predictor.trend_bias))
        act = 4 * B * M * (L + P) + 4 * 3 * B * P * M    # latents read twice-ish, pred / target / dy
        nbytes = wbytes * (1 + 1 + 3 + 7) + 2 * act
        roof_ms = nbytes / HBM_PEAK * 1e3

        eager = EagerDLinear(L, P, M, K, individual).to(dev)
        opt = torch.optim.AdamW(eager.parameters(), lr=1e-4, weight_decay=1e-2)
        rows = v.reshape(B, (TIN + TOUT) * cf, M)

        def eager_step():
            inp = rows[:, :L] - rows[:, L - cf:L].repeat(1, TIN, 1)
            tgt = rows[:, L:] - rows[:, L - cf:L].repeat(1, TOUT, 1)
            loss = F.mse_loss(eager(inp), tgt)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(eager.parameters(), 1.0)
            opt.step()

        ems = timed(eager_step, 1, a.eager_steps)
        print(json.dumps({"variant": name, "M": M, "L": L, "P": P, "K": K, "individual": individual,
                          "kernel_step_ms": round(ms, 4), "eager_step_ms": round(ems, 2),
                          "speedup": round(ems / ms, 1), "weight_MB": round(wbytes / 1e6, 2),
                          "step_bytes_MB": round(nbytes / 1e6, 1), "hbm_roof_ms": round(roof_ms, 4),
                          "fraction_of_roof": round(roof_ms / ms, 3)}), flush=True)
        del model, eager, opt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
