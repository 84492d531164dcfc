"""What one due `log_images` call costs (pipeline/helpers.py, `--plots DIR`), stage by stage, at the two shapes the
experiments hand over: B = 8, T = 13, 128 x 128 (a forecaster's decoded sequence) and B = 8, T = 1, 384 x 384 (the
autoencoders on full-size SEVIR).  Four of the eight samples are drawn, as in a run.  Two kinds of content, because
zlib's time depends on it: `blobs`, the synthetic VIL-like events of synth.blob_events with the next frame plus a little
noise as the prediction (smooth fields, about half zeros, like real VIL), and `noise`, uniform values, which no
compressor shrinks: the worst case.

    count      wfae_range_count over the whole target + the read of its integer   device events around launch and .item()
    render     wfae_panel_render of the four figures                              device events
    copy       the figures to the host                                            device events around .cpu()
    compress   zlib at helpers.PNG_LEVEL (1, what log_images uses) of the four scanline buffers   host clock
    compress6  the same at zlib's default level 6, for comparison                 host clock
    write      chunk framing, CRCs, the four files and the index lines            host clock (= write_png - compress)
    call       the whole helpers.log_images call                                  host clock, device synchronised

and, for the 384 x 384 shape, the train step of the autoencoder at the same batch (PosAwareAE_TF, forward + L1 +
backward + AdamW, as __graft_entry__.smoke runs it) so that the cost has something to stand next to.  Medians over
`--rounds` calls after `--warmup` untimed ones, with the spread of the calls ((p90 - p10) / median).  Appends one JSON
line per shape to profiles/panels_bench.jsonl (or --out).  No acceptance bar hangs on these numbers.

    python tools/panels_bench.py [--rounds 20] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from weatherforecastingtoolkit_amd import ops, synth  # noqa: E402
from weatherforecastingtoolkit_amd.pipeline import helpers  # noqa: E402

CASES = [(8, 13, 128, 128), (8, 1, 384, 384)]
KINDS = ("blobs", "noise")


def content(kind, b, t, h, w, dev):
    """-> (pred, target) fp32 (b, t, h, w) on the device"""
    g = torch.Generator().manual_seed(b * t + h)
    if kind == "noise":
        target = torch.rand((b, t, h, w), generator=g)
        return (target + 0.1 * torch.randn((b, t, h, w), generator=g)).to(dev), target.to(dev)
    ev = synth.blob_events(b, h, t + 1, seed=99).astype(np.float32) / np.float32(255)       # (b, h, w, t + 1)
    frames = torch.from_numpy(ev).permute(0, 3, 1, 2)
    target = frames[:, :t].contiguous()
    pred = (frames[:, 1:] + 0.02 * torch.randn((b, t, h, w), generator=g)).contiguous()
    return pred.to(dev), target.to(dev)


def spread(xs):
    q = statistics.quantiles(xs, n=10)
    return (q[-1] - q[0]) / statistics.median(xs)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def ae_step_ms(b, size, rounds, warmup, dev):
    from weatherforecastingtoolkit_amd import functional as Fn
    from weatherforecastingtoolkit_amd.optim import FusedAdamW
    from weatherforecastingtoolkit_amd.pipeline.models.ae_64x8x8_lin import PosAwareAE_TF
    torch.manual_seed(0)
    net = PosAwareAE_TF(img_size=size).to(dev).train()
    opt = FusedAdamW(net.parameters(), lr=5e-5, weight_decay=1e-4)
    x = torch.rand(b, 1, size, size, device=dev)
    ts = []
    for i in range(warmup + rounds):
        def step():
            recon, _ = net(x)
            Fn.l1_loss(recon, x).backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
        ms, _ = event_ms(step)
        if i >= warmup:
            ts.append(ms)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panels_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("panels_bench needs a GPU: nothing here is measured on a CPU")
    dev = torch.device("cuda:0")
    vil, reds = helpers._device_luts(dev)
    for (b, t, h, w), kind in [(c, k) for c in CASES for k in KINDS]:
        pred, target = content(kind, b, t, h, w, dev)
        nb = min(4, b)
        stages = {k: [] for k in ("count", "render", "copy", "compress", "compress6", "write", "call")}
        png_bytes = 0
        with tempfile.TemporaryDirectory() as tmp:
            sink = helpers.PanelSink(tmp)
            for i in range(a.warmup + a.rounds):
                c_ms, _ = event_ms(lambda: int(ops.range_count(target).item()))
                r_ms, figs = event_ms(lambda: ops.panel_render(pred, target, vil, reds, nb, helpers.PANEL_GAP))
                d_ms, host = event_ms(lambda: figs.cpu().numpy())
                t0 = time.perf_counter()
                comp = [zlib.compress(host[k].tobytes(), helpers.PNG_LEVEL) for k in range(nb)]
                z_ms = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                comp1 = [zlib.compress(host[k].tobytes(), 6) for k in range(nb)]
                z1_ms = (time.perf_counter() - t0) * 1e3
                hfig, wfig = host.shape[1], (host.shape[2] - 1) // 3
                t0 = time.perf_counter()
                for k in range(nb):
                    helpers.write_png(os.path.join(tmp, f"bench_b{k}.png"), host[k].tobytes(), wfig, hfig, helpers.PNG_LEVEL)
                w_ms = (time.perf_counter() - t0) * 1e3 - z_ms
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                helpers.log_images(pred, target, "bench call", sink)
                torch.cuda.synchronize()
                all_ms = (time.perf_counter() - t0) * 1e3
                if i >= a.warmup:
                    for k, v in zip(stages, (c_ms, r_ms, d_ms, z_ms, z1_ms, w_ms, all_ms)):
                        stages[k].append(v)
                    png_bytes, png1_bytes = sum(len(c) for c in comp), sum(len(c) for c in comp1)
        rec = {"B": b, "T": t, "H": h, "W": w, "content": kind, "drawn": nb, "gap": helpers.PANEL_GAP,
               "figure_bytes": ops.panel_bytes(t, h, w, helpers.PANEL_GAP), "idat_bytes_drawn": png_bytes,
               "idat_bytes_drawn_level6": png1_bytes, "level": helpers.PNG_LEVEL,
               "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
        for k, ts in stages.items():
            rec[k] = {"ms": round(statistics.median(ts), 4), "spread": round(spread(ts), 4)}
        if t == 1 and kind == KINDS[0]:
            ts = ae_step_ms(b, h, a.rounds, a.warmup, dev)
            rec["ae_train_step"] = {"ms": round(statistics.median(ts), 4), "spread": round(spread(ts), 4)}
        print(json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
