"""The `ae_s2` step at its shipped geometry — B = 8 sequences of 13 frames of 128 x 128, AutoencoderKL with 64 latent
channels (latents 64 x 16 x 16, enc_in 16384) — on the gfx950 kernels against an eager-torch restatement of the same step
on the same GPU (tests/ae_s2_ref.py: the reference's per-frame encode / decode loops on tests/aekl_ref.py; the DLinear as
two einsums over stacked weights, which is far kinder to eager torch than the reference's Python loop over 16384 module
pairs; torch.optim.AdamW on the four stacked tensors).

    python tools/ae_s2_bench.py [--steps 10] [--rounds 3] [--precisions highest,medium] [--out profiles/ae_s2_bench.jsonl]

Per precision one JSON line is appended to --out: ms of one training step (sampled encode of 104 frames, predictor
forward / loss / backward / clip / AdamW) and of one validation step (encode, loss, decode of the 48 forecast and the 48
target frames, calc_metrics) for the product and for eager torch, alternated inside one process, `rounds` rounds of
`steps` calls between a pair of device events, medians; the product's encode / predictor / decode parts timed on their
own and as shares of their step; and the encode in ms per frame with all 104 frames in one pass against chunks of 8 — and,
for eager torch, the reference's loop over T (13 calls of 8 frames, what the eager steps above run) against one call of 104.
There are no thresholds: the tool measures.
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
from tests import ae_s2_ref as S  # noqa: E402
from tests import aekl_ref as A  # noqa: E402
from tests import dlinear_ref as D  # noqa: E402
from weatherforecastingtoolkit_amd import config as C  # noqa: E402
from weatherforecastingtoolkit_amd.experiments.ae_s2 import train as T  # noqa: E402


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def median_pair(prod, eager, steps, rounds):
    """-> (product ms, eager ms, every round's pair): medians of `rounds` alternated rounds, one untimed call of each first"""
    timed(prod, 1)
    timed(eager, 1)
    p, e = [], []
    for _ in range(rounds):
        p.append(timed(prod, steps))
        e.append(timed(eager, steps))
    return statistics.median(p), statistics.median(e), [[round(x, 2), round(y, 2)] for x, y in zip(p, e)]


def median_of(fn, steps, rounds):
    timed(fn, 1)
    return statistics.median(timed(fn, steps) for _ in range(rounds))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--precisions", default="highest,medium")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ae_s2_bench.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.backends.cuda.matmul.allow_tf32 = False
    cfg = C.load(os.path.join(T.HERE, "config.yaml"))
    cfg.trainer.total_train_steps = 1000
    d = cfg.dataset
    b, t, size = d.batch_size, d.seq_len, d.image_width
    torch.manual_seed(0)
    model = T.Model(cfg).to(dev).train()
    model.autoencoder.eval()
    model.configure_optimizers()
    ae = model.autoencoder
    frames = torch.rand(b, t, 1, size, size, generator=torch.Generator().manual_seed(1)).to(dev)
    ae_cfg = {k: cfg.ae_kl[k] for k in ae.AEKL_KEYS if cfg.ae_kl.get(k) is not None}
    sd = {k: v.detach() for k, v in ae.autoencoder.state_dict().items()}

    # the eager step: its own copy of the predictor's parameters, stacked
    st = D.stacked_from_state_dict({k: v.detach().clone() for k, v in model.predictor.state_dict().items()}, True,
                                   cfg.dlinear.enc_in)
    params = [p.clone().requires_grad_(True) for p in (*st["Linear_Seasonal"], *st["Linear_Trend"])]
    del st
    opt = torch.optim.AdamW(params, lr=cfg.optim.lr, weight_decay=cfg.optim.weight_decay,
                            betas=(cfg.optim.beta1, cfg.optim.beta2))
    latent = (cfg.ae_kl.latent_channels, size // ae.autoencoder.downscale, size // ae.autoencoder.downscale)

    def eager_encode():
        with torch.no_grad():
            return S.encode(sd, frames, ae_cfg, ae.draw_noise(b, t, latent, dev))

    def eager_train():
        loss, _ = S.step(eager_encode(), params)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, cfg.optim.gradient_clip_val)
        opt.step()
        opt.zero_grad(set_to_none=True)

    def eager_val():
        from weatherforecastingtoolkit_amd.pipeline import helpers
        with torch.no_grad():
            z = eager_encode()
            _, pred = S.step(z, params)
            fc, tg = S.forecast_and_target(z, pred)
            # the metrics are the product's kernels on both sides: the reference's calc_metrics is not restated here
            helpers.log_metrics(S.decode(sd, fc, ae_cfg), S.decode(sd, tg, ae_cfg), "val")

    for prec in a.precisions.split(","):
        pkg.set_float32_matmul_precision(prec)
        torch.set_float32_matmul_precision(prec)
        try:
            z = ae.encode(frames)
            half = z[:, :d.pred_frames].contiguous()
            train_p, train_e, train_r = median_pair(lambda: model.training_step(frames), eager_train, a.steps, a.rounds)
            val_p, val_e, val_r = median_pair(lambda: model.validation_step(frames), eager_val, a.steps, a.rounds)
            flat = frames.view(b * t, 1, size, size)
            with torch.no_grad():
                eager_loop = median_of(lambda: [A.encode(sd, frames[:, i], ae_cfg)["mean"] for i in range(t)], a.steps, a.rounds)
                eager_one = median_of(lambda: A.encode(sd, flat, ae_cfg)["mean"], a.steps, a.rounds)
            ae.chunk_frames = 0
            enc_one = median_of(lambda: ae.encode(frames), a.steps, a.rounds)
            ae.chunk_frames = 8
            enc_chunks = median_of(lambda: ae.encode(frames), a.steps, a.rounds)
            ae.chunk_frames = 0
            predictor = median_of(lambda: model.train_latents(z), a.steps, a.rounds)
            decode = median_of(lambda: (ae.decode(half), ae.decode(half)), a.steps, a.rounds)
            with torch.no_grad():
                noise = ae.draw_noise(b, t, latent, dev)
                whole = ae.encode(frames, noise=noise)
                parity = S.spread(whole, S.encode(sd, frames, ae_cfg, noise))
                ae.chunk_frames = 8
                same_bits = bool(torch.equal(whole, ae.encode(frames, noise=noise)))
                ae.chunk_frames = 0
            n = b * t
            line = {"case": f"{b}x{t}x{size}x{size} latent {latent[0]}x{latent[1]}x{latent[2]} enc_in {cfg.dlinear.enc_in}",
                    "precision": prec,
                    "train_step_ms": {"product": round(train_p, 2), "eager": round(train_e, 2),
                                      "eager_over_product": round(train_e / train_p, 2), "rounds": train_r},
                    "val_step_ms": {"product": round(val_p, 2), "eager": round(val_e, 2),
                                    "eager_over_product": round(val_e / val_p, 2), "rounds": val_r},
                    "product_parts_ms": {"encode": round(enc_one, 2), "predictor_step": round(predictor, 2),
                                         "decode_2x48": round(decode, 2)},
                    "train_shares": {"encode": round(enc_one / train_p, 3), "predictor": round(predictor / train_p, 3)},
                    "val_shares": {"encode": round(enc_one / val_p, 3), "decode": round(decode / val_p, 3)},
                    "encode_ms_per_frame": {"one_pass_104": round(enc_one / n, 3), "chunks_of_8": round(enc_chunks / n, 3),
                                            "eager_loop_over_T": round(eager_loop / n, 3), "eager_one_pass_104": round(eager_one / n, 3)},
                    "z_vs_eager": parity, "one_pass_bit_equal_to_chunks_of_8": same_bits}
            print(json.dumps(line), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        finally:
            pkg.set_float32_matmul_precision("highest")
            torch.set_float32_matmul_precision("highest")


if __name__ == "__main__":
    main()
