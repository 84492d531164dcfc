"""`ae_s2` on MI355X: the reference's experiments/ae_s2/train.py without Lightning / W&B — a frozen AutoencoderKL whose
latents are SAMPLED (`encode(frame).sample()` per frame, :29-38, fresh noise every step), and on them the per-scalar
DLinear of `pretrained_ae_dlinear_ind` (16384 Linear(7 -> 6) pairs): differencing against the last input frame, MSE,
AdamW with `optim.beta1` / `beta2`, cosine warmup.

    python -m weatherforecastingtoolkit_amd.experiments.ae_s2.train [--mode fit|test] [--no-test] key=value ...

The default is `fit` followed by the test pass, as the reference's `__main__` calls trainer.fit and trainer.test.  Its
`fast_dev_run=True` (one batch per split) is not reproduced: `--max-steps 1` gives that.  DLinear, moving_avg and
series_decomp are the v1 experiments' (../v1_experiments/_dlinear.py), the provider is ../v1_experiments/_latents.py with
`sample: true`, the driver ../v1_experiments/_runner.py.

A loader batch is frames (B, T, 1, H, W) ('NTCHW', :260), so `Model` encodes every 5-D batch; latents go in through
`train_latents` / `validate_latents`, by name.
"""
from __future__ import annotations

import os
import sys

from ..._lib import WfaeError
from ..v1_experiments import _dlinear
from ..v1_experiments import _latents
from ..v1_experiments._dlinear import DLinear, moving_avg, series_decomp  # noqa: F401
from ..v1_experiments._runner import run

HERE = os.path.dirname(os.path.abspath(__file__))


class Autoencoder(_latents.Autoencoder):
    """reference :19-53: `Autoencoder(cfg.ae_kl)`, encode (B, T, 1, H, W) -> sampled latents (B, T, C, h, w), decode back;
    `self.autoencoder` is the AutoencoderKL, as there.  One pass over the B*T frames (`chunk_frames`, default 0) instead
    of a loop over T; the noise is drawn as the loop draws it.  `encode(x, generator=None, noise=None)`: the keyword
    arguments are the provider's extensions."""

    def __init__(self, config):
        cfg = dict(config)
        cfg.setdefault("chunk_frames", 0)
        cfg["sample"] = True
        if not cfg.get("checkpoint"):
            print(f"ae_kl.checkpoint is null: the AutoencoderKL is the seeded initialisation (ae_kl.seed = "
                  f"{int(cfg.get('seed') or 0)}), not a pretrained one", flush=True)
        super().__init__(kind="autoencoder_kl", cfg=cfg)


class Model(_dlinear.Model):
    """reference Model (:135-226): the steps of `pretrained_ae_dlinear_ind` (both splits' figures timed by
    epoch * total_val_steps + batch_idx against logging.log_train_plots_n) on the provider of `cfg.ae_kl`.
    `generator`: where the latent noise is drawn from (None: the device's global generator)."""

    generator = None

    def __init__(self, cfg, autoencoder=None):
        super().__init__(cfg, autoencoder=autoencoder if autoencoder is not None else Autoencoder(cfg.ae_kl), plots="ind")

    def frames_latents(self, batch):
        """batch (a tensor, or the loader's dict): frames (B, T, 1, H, W) or (B, T, H, W) -> (frames (B, T, 1, H, W),
        sampled latents (B, T, C, h, w)).  Never latents: those go to `train_latents` / `validate_latents`"""
        if isinstance(batch, dict):
            batch = batch["vil"]
        if batch.dim() == 4:
            batch = batch.unsqueeze(2)
        if batch.dim() != 5 or batch.shape[2] != 1:
            raise WfaeError(f"expected frames (B, T, 1, H, W), got {tuple(batch.shape)}; latents go to train_latents / "
                            "validate_latents")
        if self.batch_ids is not None:
            return batch, self.autoencoder.encode(batch.contiguous(), generator=self.generator, ids=self.batch_ids)
        return batch, self.autoencoder.encode(batch.contiguous(), generator=self.generator)


def build(cfg, size):
    # reference :282; nothing else reads the lpips block
    cfg.lpips.disc_start = int(cfg.lpips.disc_start * cfg.trainer.total_train_steps)
    return Model(cfg)


def main(argv=None):
    return run(HERE, argv, build, default_mode="fit", layout=lambda cfg: "NTCHW", test_after_fit=True)


if __name__ == "__main__":
    sys.exit(main())
