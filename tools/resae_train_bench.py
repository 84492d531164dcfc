"""Training the ae_gan residual autoencoder (ConvAutoencoderBIG) on csrc/resae.hip + csrc/resae_bwd.hip.

    python tools/resae_train_bench.py [--steps 20] [--rounds 5] [--out profiles/resae_train_bench.jsonl]

Two kinds of JSON lines are appended to --out, all from one process:
  {"layer": ...}  for every layer of ConvAutoencoderBIG on 128 x 128 frames whose output plane has at most 16 pixels, at
      B = 8 and B = 32: the data and the weight gradient on the small-plane route and on the tile route forced on the same
      input (alternated, median of `rounds` windows of `steps` launches between a pair of device events), and for the
      weight gradient the bytes of dw (4 x Cout x Cin x k x k) over the small route's time as a fraction of the HBM roof
      (8 TB/s, MI355X).
  {"model": ...}  one full train step at B = 8 (forward, L1, backward, clip, AdamW, schedule) against the same
      architecture written with torch.nn modules (tools/resae_bench.py `EagerBig`) under torch.optim.AdamW and
      clip_grad_norm_ on the same GPU, alternated the same way, plus the kernel times by label of one product step.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from resae_bench import EagerBig, alternate, ms, small_layers  # noqa: E402
from weatherforecastingtoolkit_amd import config as C  # noqa: E402
from weatherforecastingtoolkit_amd import ops  # noqa: E402
from weatherforecastingtoolkit_amd.experiments.v1_experiments import _ae_gan as M  # noqa: E402
from weatherforecastingtoolkit_amd.experiments.v1_experiments.ae_gan import fit as FIT  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "resae_train_bench.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    lines = []
    for name, kind, cin, cout, h, w in small_layers():
        k = 1 if kind >= 3 else 3
        wt = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5).to(dev)
        pt = ops.resae_bwd_pack(wt, kind)
        dw = torch.empty_like(wt)
        ho, wo = ops.resae_out_plane(kind, h, w)
        taps = sum(map(sum, ops.resae_live_taps(kind, h, w)))
        for n in (8, 32):
            x = torch.randn(n, cin, h, w, generator=g).to(dev)
            dy = torch.randn(n, cout, ho, wo, generator=g).to(dev)
            ds, dt = alternate(lambda: ops.resae_bwd_data(dy, pt, x.shape, route="small"),
                               lambda: ops.resae_bwd_data(dy, pt, x.shape, route="tile"), a.steps, a.rounds, a.warmup)
            ws, wtile = alternate(lambda: ops.resae_bwd_weight(dy, x, dw, kind, route="small"),
                                  lambda: ops.resae_bwd_weight(dy, x, dw, kind, route="tile"), a.steps, a.rounds, a.warmup)
            gbs = 4 * dw.numel() / (statistics.median(ws) * 1e-3) / 1e9
            lines.append({"layer": name, "kind": kind, "cin": cin, "cout": cout, "plane_in": [h, w], "batch": n, "live_taps": taps,
                          "dw_bytes": 4 * dw.numel(),
                          "data_small": ms(ds), "data_tile": ms(dt),
                          "data_tile_over_small": round(statistics.median(dt) / statistics.median(ds), 2),
                          "weight_small": ms(ws), "weight_tile": ms(wtile),
                          "weight_tile_over_small": round(statistics.median(wtile) / statistics.median(ws), 2),
                          "weight_small_dw_gb_per_s": round(gbs, 1),
                          "weight_small_fraction_of_hbm_roof": round(gbs * 1e9 / ops.PEAK_HBM, 4)})
            print(json.dumps(lines[-1]), flush=True)
        del wt, pt, dw

    cfg = C.load(os.path.join(FIT.HERE, "config.yaml"))
    cfg.trainer.total_train_steps = 1000
    torch.manual_seed(0)
    model = FIT.build(cfg, 128).to(dev).train()
    model.configure_optimizers()
    eager = EagerBig().to(dev).train()
    opt = torch.optim.AdamW(eager.parameters(), lr=1e-3, weight_decay=1e-5)
    x = torch.rand(8, 1, 128, 128, generator=g).to(dev)

    def eager_step():
        loss = F.l1_loss(eager(x)[0], x)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(eager.parameters(), 1.0)
        opt.step()
        opt.zero_grad(set_to_none=True)

    steps = max(1, a.steps // 2)
    prod, eag = alternate(lambda: model.training_step(x), eager_step, steps, a.rounds, a.warmup)
    ops.profile_start()
    model.training_step(x)
    prof = ops.profile_stop()
    by_label = {}
    for k_, v in prof.items():      # the per-layer labels of the resae entry points, folded to entry point + route
        key = " ".join(k_.split()[:2]) if k_.startswith("wfae_resae") else k_
        by_label[key] = by_label.get(key, 0.0) + v[1]
    lines.append({"model": "ConvAutoencoderBIG train step", "batch": 8, "steps": steps, "rounds": a.rounds,
                  "tile_mode": ops.aekl_mode(), "product": ms(prod), "eager": ms(eag),
                  "eager_over_product": round(statistics.median(eag) / statistics.median(prod), 2),
                  "entry_point_calls": sum(v[0] for v in prof.values()),
                  "kernel_ms_total": round(sum(v[1] for v in prof.values()), 3),
                  "ms_by_label": {k_: round(v, 4) for k_, v in sorted(by_label.items(), key=lambda kv: -kv[1])}})
    print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for l in lines:
            f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
