"""Conv + attention latent autoencoder step of pretrained_ae_convattn_ae_sevir on the gfx950 kernels against the same
network built from torch.nn modules and run eagerly on the same GPU.

    python tools/convattn_bench.py [--steps 100] [--rounds 5] [--batch 8] [--out profiles/convattn_bench.jsonl]

Batch 8 on 4 x 48 x 48 latents (the reference config's batch), training mode (dropout 0.1); no latent provider is in the
timing.  Both sides do forward, Huber loss, backward, clip at 1.0 and AdamW.  After a warm-up of both, the product and the
eager step are alternated inside one process, `rounds` times, each round timing `steps` steps between a pair of device
events; one JSON line (appended to --out) holds the median and the range of the per-round ms per step of each and the
entry-point calls of one product step.
"""
import argparse
import json
import os
import statistics
import sys
import warnings

import torch
import torch.nn as tnn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from weatherforecastingtoolkit_amd import config as C  # noqa: E402
from weatherforecastingtoolkit_amd import ops  # noqa: E402
from weatherforecastingtoolkit_amd.experiments.v1_experiments import _convattn as M  # noqa: E402


class EagerConvAttn(tnn.Module):
    """the reference's ConvAttnModel written with torch.nn modules (same layers, same order)"""

    def __init__(self, c=4, e=128, h=8, layers=4, latent=512):
        super().__init__()
        self.e = e
        self.encoder_cnn = tnn.Sequential(tnn.Conv2d(c, 64, 3, 2, 1), tnn.GroupNorm(8, 64), tnn.GELU(),
                                          tnn.Conv2d(64, e, 3, 2, 1), tnn.GroupNorm(8, e), tnn.GELU())
        self.encoder_pos_embedding = tnn.Parameter(torch.randn(1, 144, e))
        kw = dict(d_model=e, nhead=h, dim_feedforward=4 * e, activation="gelu", batch_first=True, norm_first=True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            self.encoder_tf = tnn.TransformerEncoder(tnn.TransformerEncoderLayer(**kw), num_layers=layers)
        self.pooling_query = tnn.Parameter(torch.randn(1, 1, e))
        self.attention_pool = tnn.MultiheadAttention(e, h, batch_first=True)
        self.encoder_head = tnn.Sequential(tnn.LayerNorm(e), tnn.Linear(e, latent))
        self.decoder_head = tnn.Linear(latent, e)
        self.decoder_queries = tnn.Parameter(torch.randn(1, 144, e))
        self.decoder_pos_embedding = tnn.Parameter(torch.randn(1, 144, e))
        self.decoder_tf = tnn.TransformerDecoder(tnn.TransformerDecoderLayer(**kw), num_layers=layers)
        self.decoder_cnn = tnn.Sequential(tnn.ConvTranspose2d(e, 64, 4, 2, 1), tnn.GroupNorm(8, 64), tnn.GELU(),
                                          tnn.ConvTranspose2d(64, c, 4, 2, 1))

    def forward(self, x):
        b = x.shape[0]
        t = self.encoder_cnn(x).flatten(2).transpose(1, 2) + self.encoder_pos_embedding
        t = self.encoder_tf(t)
        pooled, _ = self.attention_pool(self.pooling_query.expand(b, -1, -1), t, t)
        z = self.encoder_head(pooled).squeeze(1)
        q = self.decoder_queries.expand(b, -1, -1) + self.decoder_pos_embedding
        t = self.decoder_tf(q, self.decoder_head(z).unsqueeze(1))
        return self.decoder_cnn(t.transpose(1, 2).reshape(b, self.e, 12, 12))


class EagerStep:
    def __init__(self, dev):
        self.net = EagerConvAttn().to(dev).train()
        self.opt = torch.optim.AdamW(self.net.parameters(), lr=1e-4, weight_decay=1e-2)

    def __call__(self, x):
        loss = F.huber_loss(self.net(x), x)
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(self.net.parameters(), 1.0)
        self.opt.step()


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
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=os.path.join("profiles", "convattn_bench.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = C.load(os.path.join(os.path.dirname(M.__file__), "pretrained_ae_convattn_ae_sevir", "config.yaml"))
    cfg.trainer.total_train_steps = 10 ** 6
    n = a.batch
    x = torch.randn(n, 1, 4, 48, 48, generator=torch.Generator().manual_seed(1)).to(dev)
    xe = x.view(n, 4, 48, 48)
    torch.manual_seed(0)
    model = M.Model(cfg).to(dev).train()
    model.configure_optimizers()
    eager = EagerStep(dev)
    timed(lambda: model.training_step(x), a.warmup)
    timed(lambda: eager(xe), a.warmup)
    prod, eag = [], []
    for _ in range(a.rounds):
        prod.append(timed(lambda: model.training_step(x), a.steps))
        eag.append(timed(lambda: eager(xe), a.steps))
    ops.profile_start()
    model.training_step(x)
    prof = ops.profile_stop()
    rec = {"samples": n, "steps": a.steps, "rounds": a.rounds,
           "product_ms": round(statistics.median(prod), 4), "product_ms_range": [round(min(prod), 4), round(max(prod), 4)],
           "eager_ms": round(statistics.median(eag), 4), "eager_ms_range": [round(min(eag), 4), round(max(eag), 4)],
           "eager_over_product": round(statistics.median(eag) / statistics.median(prod), 2),
           "product_slowest_below_eager_fastest": max(prod) < min(eag),
           "entry_point_calls_step": sum(v[0] for v in prof.values()),
           "calls": {k: v[0] for k, v in sorted(prof.items())},
           "ms_by_entry_point": {k: round(v[1], 4) for k, v in sorted(prof.items(), key=lambda kv: -kv[1][1])[:12]}}
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
