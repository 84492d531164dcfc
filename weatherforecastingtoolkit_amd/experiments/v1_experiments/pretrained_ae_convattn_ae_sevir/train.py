"""Conv + attention latent autoencoder `pretrained_ae_convattn_ae_sevir` on MI355X: the predictor step of the reference's
experiments/v1_experiments/pretrained_ae_convattn_ae_sevir/train.py without Lightning / W&B — latents (4, 48, 48) of the
frozen AutoencoderKL are auto-encoded through two conv + GroupNorm + GELU units, four pre-norm transformer encoder layers
over the 144 tokens, an attention pool to a 512-vector, and back through four transformer decoder layers and two
transposed convolutions, under a Huber loss.

    python -m weatherforecastingtoolkit_amd.experiments.v1_experiments.pretrained_ae_convattn_ae_sevir.train [--mode fit|test] key=value ...

The default mode is `fit`, as the reference's `__main__` calls `trainer.fit`.  The classes live in ../_convattn.py, the
driver in ../_runner.py.  `last.ckpt` holds `predictor._orig_mod.<key>` (the reference wraps the predictor in
torch.compile); `load_predictor_state` accepts the keys with or without `_orig_mod.`.
"""
from __future__ import annotations

import os
import sys

from .._convattn import Autoencoder, ConvAttnModel, Model, load_predictor_state, predictor_state  # noqa: F401
from .._runner import run, with_provider

HERE = os.path.dirname(os.path.abspath(__file__))


def main(argv=None):
    return run(HERE, argv, with_provider(Model), default_mode="fit", rate="frames_per_s", state=predictor_state)


if __name__ == "__main__":
    sys.exit(main())
