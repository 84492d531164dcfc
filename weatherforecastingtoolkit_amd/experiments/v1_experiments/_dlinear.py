"""DLinear latent forecasters of the reference's v1 experiments:
experiments/v1_experiments/pretrained_ae_dlinear_{sevir,ind,indc_indp}/train.py without Lightning / W&B.

Reference (:22-100): the latent sequence is split into a replicate-padded moving-average trend and a seasonal
remainder (`series_decomp`), each goes through a linear map over time (one shared `nn.Linear`, or one per latent
scalar / latent pixel when `individual`), and the two results are added.  The step (:151-162) differences inputs and
targets against the last input frame and takes the MSE.

Here the latent sequence v (B, T, C, h, w) is viewed as rows (B, T*cf, M): cf = 1, M = C*h*w for `dlinear_sevir` /
`dlinear_ind`; cf = C, M = h*w for `dlinear_indc_indp` (the reference hardcodes its 4 latent channels as `* 4`).
The whole predictor step is a handful of gfx950 kernels (csrc/dlinear.hip): target, fused differencing +
decomposition + both linear maps, MSE, the weight gradients, clip and AdamW — instead of the reference's Python loop
over 9216 (or 2304) module pairs.  Parameters are stacked (M, P, L) tensors; state_dict() / load_state_dict() speak
the reference's per-module keys.  The frozen latent provider is ./_latents.py; the optimiser step and the driver are
the v1 experiments' shared ones (./_runner.py).
"""
from __future__ import annotations

import math

import torch
import torch.nn as tnn

from ... import functional as Fn
from ... import ops
from ..._lib import WfaeError
from ...pipeline import helpers
from ._latents import Autoencoder  # noqa: F401  (the frozen latent provider)
from ._runner import Step


def _check_kernel_size(kernel_size):
    if kernel_size < 1 or kernel_size % 2 == 0:
        raise WfaeError(f"DLinear: kernel_size must be odd and >= 1, got {kernel_size} (an even window changes the "
                        "sequence length and breaks the reference's seasonal = x - trend)")


class moving_avg(tnn.Module):
    """reference :21-36: trend of x (B, L, M) along L, replicate padding of (K-1)/2 rows, AvgPool1d(K, stride 1)"""

    def __init__(self, kernel_size, stride):
        super().__init__()
        _check_kernel_size(kernel_size)
        if stride != 1:
            raise WfaeError("moving_avg: only stride 1 (what series_decomp uses) is implemented")
        self.kernel_size = kernel_size

    def forward(self, x):
        return Fn.series_decomp(x, self.kernel_size)[1]


class series_decomp(tnn.Module):
    """reference :38-48: x (B, L, M) -> (x - trend, trend)"""

    def __init__(self, kernel_size):
        super().__init__()
        self.moving_avg = moving_avg(kernel_size, stride=1)

    def forward(self, x):
        return Fn.series_decomp(x, self.moving_avg.kernel_size)


class DLinear(tnn.Module):
    """reference :50-100 with the constructor surface `configs.{seq_len, pred_len, kernel_size, individual, enc_in}`
    and `configs.features_per_step` (default 1; `dlinear_indc_indp` uses its latent channel count, the reference's
    `* 4`): the maps are Linear(seq_len * f -> pred_len * f), and there is no `Linear_Decoder` when f > 1.

    forward(x (B, L, M)) -> (B, P, M) as the reference's; forward_rows(v (B, R, M)) also differences rows [0, L)
    against the last input frame first (the training step's `inp - inp_t`).

    Initialisation consumes torch's global generator exactly as the reference's constructor does (default nn.Linear
    init of Seasonal, Trend and, when present, Decoder for each column in turn, then the Seasonal / Trend weights
    overwritten with 1 / (f * seq_len)), so after the same torch.manual_seed every value is bit-identical."""

    def __init__(self, configs):
        super().__init__()
        get = configs.get if hasattr(configs, "get") else (lambda k, d=None: getattr(configs, k, d))
        self.seq_len, self.pred_len = int(get("seq_len")), int(get("pred_len"))
        self.kernel_size = int(get("kernel_size"))
        _check_kernel_size(self.kernel_size)
        self.individual = bool(get("individual"))
        self.channels = int(get("enc_in"))
        self.features = int(get("features_per_step", 1) or 1)
        self.decompsition = series_decomp(self.kernel_size)
        f = self.features
        L, P = self.seq_len * f, self.pred_len * f
        self.in_rows, self.out_rows = L, P
        self.has_decoder = f == 1
        names = ["Linear_Seasonal", "Linear_Trend"] + (["Linear_Decoder"] if self.has_decoder else [])
        n = self.channels if self.individual else 1
        wshape = (n, P, L) if self.individual else (P, L)
        bshape = (n, P) if self.individual else (P,)
        # the reference's RNG stream: per column, per module, kaiming_uniform_(weight) then uniform_(bias); one flat
        # draw consumes the generator identically (one 32-bit draw per fp32 element), drawn once per bound
        width = P * L + P
        bound_b = 1 / math.sqrt(L) if L > 0 else 0
        gain = tnn.init.calculate_gain("leaky_relu", math.sqrt(5))
        bound_w = math.sqrt(3.0) * (gain / math.sqrt(L))
        state = torch.get_rng_state()
        draws_w = torch.empty(n, len(names), width).uniform_(-bound_w, bound_w)
        torch.set_rng_state(state)
        draws_b = torch.empty(n, len(names), width).uniform_(-bound_b, bound_b)
        fill = 1 / self.seq_len if f == 1 else 1 / (f * self.seq_len)
        self._names = names
        self.seasonal_weight = tnn.Parameter(torch.full(wshape, fill))
        self.seasonal_bias = tnn.Parameter(draws_b[:, 0, P * L:].reshape(bshape).clone())
        self.trend_weight = tnn.Parameter(torch.full(wshape, fill))
        self.trend_bias = tnn.Parameter(draws_b[:, 1, P * L:].reshape(bshape).clone())
        if self.has_decoder:
            # built like the reference's and never used: it gets no gradient, AdamW skips it
            self.decoder_weight = tnn.Parameter(draws_w[:, 2, :P * L].reshape(wshape).clone())
            self.decoder_bias = tnn.Parameter(draws_b[:, 2, P * L:].reshape(bshape).clone())

    def _maps(self):
        out = [("Linear_Seasonal", self.seasonal_weight, self.seasonal_bias),
               ("Linear_Trend", self.trend_weight, self.trend_bias)]
        if self.has_decoder:
            out.append(("Linear_Decoder", self.decoder_weight, self.decoder_bias))
        return out

    def reference_keys(self, prefix=""):
        """[(key, shape)] of the reference module's state_dict, in its order"""
        keys = []
        P, L = self.out_rows, self.in_rows
        for name, _, _ in self._maps():
            if self.individual:
                for i in range(self.channels):
                    keys += [(f"{prefix}{name}.{i}.weight", (P, L)), (f"{prefix}{name}.{i}.bias", (P,))]
            else:
                keys += [(f"{prefix}{name}.weight", (P, L)), (f"{prefix}{name}.bias", (P,))]
        return keys

    # -- reference checkpoint layout: per-column keys are views of the stacked tensors -----------------------------
    def _save_to_state_dict(self, destination, prefix, keep_vars):
        for name, w, b in self._maps():
            w = w if keep_vars else w.detach()
            b = b if keep_vars else b.detach()
            if self.individual:
                for i in range(self.channels):
                    destination[f"{prefix}{name}.{i}.weight"] = w[i]
                    destination[f"{prefix}{name}.{i}.bias"] = b[i]
            else:
                destination[f"{prefix}{name}.weight"] = w
                destination[f"{prefix}{name}.bias"] = b

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        expected = set()
        for name, w, b in self._maps():
            for tgt, suffix in ((w, "weight"), (b, "bias")):
                if self.individual:
                    keys = [f"{prefix}{name}.{i}.{suffix}" for i in range(self.channels)]
                else:
                    keys = [f"{prefix}{name}.{suffix}"]
                expected.update(keys)
                present = [k for k in keys if k in state_dict]
                missing_keys.extend(k for k in keys if k not in state_dict)
                if len(present) != len(keys):
                    continue
                want = tuple(tgt.shape[1:]) if self.individual else tuple(tgt.shape)
                bad = [k for k in keys if tuple(state_dict[k].shape) != want]
                if bad:
                    error_msgs.append(f"size mismatch for {bad[0]}: copying a param with shape "
                                      f"{tuple(state_dict[bad[0]].shape)}, the model has {want}")
                    continue
                with torch.no_grad():
                    if self.individual:
                        tgt.copy_(torch.stack([state_dict[k].to(torch.float32) for k in keys]))
                    else:
                        tgt.copy_(state_dict[keys[0]])
        if strict:
            child = tuple(f"{prefix}{c}." for c in self._modules)
            unexpected_keys.extend(k for k in state_dict
                                   if k.startswith(prefix) and k not in expected and not k.startswith(child))

    def _apply_rows(self, v, diff):
        if v.dim() != 3:
            raise WfaeError(f"DLinear: expected (batch, length, channels), got {tuple(v.shape)}")
        if self.individual and v.shape[2] != self.channels:
            raise WfaeError(f"DLinear: enc_in = {self.channels} but the input has {v.shape[2]} channels")
        return Fn.dlinear(v, self.seasonal_weight, self.seasonal_bias, self.trend_weight, self.trend_bias,
                          self.in_rows, self.kernel_size, self.individual, diff, self.features)

    def forward(self, x):
        """x (B, L, M) -> (B, P, M) (reference forward, :83-100)"""
        if x.shape[1] != self.in_rows:
            raise WfaeError(f"DLinear: input length {x.shape[1]}, expected {self.in_rows}")
        return self._apply_rows(x, False)

    def forward_rows(self, v):
        """v (B, R >= L, M): rows [0, L) differenced against the last input frame, then forward"""
        return self._apply_rows(v, True)


class Model(Step, tnn.Module):
    """reference Model (:137-239): `predictor`, `forward`, the training / validation / test steps; the optimiser is
    `Step`'s"""

    # how each reference script words and times its validation / test figures (`log_wandb_images`):
    # style -> (counts epochs into the counter, config key of the fraction, test label prefix, test label suffix)
    PLOT_STYLES = {"ind": (True, "log_train_plots_n", "", "_test"),            # pretrained_ae_dlinear_ind :201-203, :226-228
                   "sevir": (False, "log_val_plots_n", "", "_test"),           # pretrained_ae_dlinear_sevir :200-202, :225-227
                   "indc_indp": (False, "log_val_plots_n", "Test_", "")}       # ..._indc_indp :200-202, :226-228

    def __init__(self, cfg, autoencoder=None, plots="sevir"):
        super().__init__()
        self.cfg = cfg
        self.autoencoder = autoencoder
        self.plot_style = self.PLOT_STYLES[plots]
        self.input_frames, self.pred_frames = cfg.dataset.input_frames, cfg.dataset.pred_frames
        self.total_steps = cfg.trainer.total_train_steps
        self.predictor = DLinear(cfg.dlinear)
        if self.predictor.seq_len != self.input_frames or self.predictor.pred_len != self.pred_frames:
            raise WfaeError(f"dlinear.seq_len / pred_len ({self.predictor.seq_len}, {self.predictor.pred_len}) must "
                            f"equal dataset.input_frames / pred_frames ({self.input_frames}, {self.pred_frames})")

    def forward(self, x):
        return self.predictor(x)

    def _rows(self, v):
        """latents (B, T, C, h, w) -> the predictor's row view (B, T*cf, M)"""
        if v.dim() != 5:
            raise WfaeError(f"expected latents (B, T, C, h, w), got {tuple(v.shape)}")
        b, t, c, h, w = v.shape
        if t != self.input_frames + self.pred_frames:
            raise WfaeError(f"latent sequence has {t} frames, expected {self.input_frames + self.pred_frames}")
        f = self.predictor.features
        if f != 1 and f != c:
            raise WfaeError(f"dlinear.features_per_step = {f} must be 1 or the latent channel count {c}")
        m = c * h * w // f
        if m != self.predictor.channels:
            what = "C*h*w" if f == 1 else "h*w"
            raise WfaeError(f"dlinear.enc_in = {self.predictor.channels} does not match the latent provider: latents "
                            f"{c}x{h}x{w} need enc_in = {m} ({what})")
        return v.contiguous().view(b, t * f, m)

    def latent_loss(self, v):
        """-> (loss, pred (B, P, M), rows)"""
        rows = self._rows(v)
        L, P, f = self.predictor.in_rows, self.predictor.out_rows, self.predictor.features
        pred = self.predictor.forward_rows(rows)
        tgt = ops.dlinear_target(rows, L, P, f)
        return Fn.mse_loss(pred, tgt), pred, rows

    @torch.no_grad()
    def predict_latents(self, v):
        """forecast latents (B, Tout, C, h, w) = pred + last input frame (reference :197)"""
        rows = self._rows(v)
        pred = self.predictor.forward_rows(rows)
        b, _, c, h, w = v.shape
        return ops.dlinear_forecast(pred, rows, self.predictor.in_rows, self.predictor.features).view(
            b, self.pred_frames, c, h, w)

    def training_step(self, batch, batch_idx=0):
        """batch: frames (B,T,H,W) fp32 in [0,1] ('NTHW') or latents (B,T,C,h,w); AdamW + cosine warmup, clip 1.0"""
        _, v = self.frames_latents(batch)
        return self.train_latents(v)

    def train_latents(self, v):
        """training_step on latents (B, T, C, h, w)"""
        loss, _, _ = self.latent_loss(v)
        return self.optimizer_step(loss)

    @torch.no_grad()
    def validation_step(self, batch, batch_idx=0, split="val"):
        """-> (loss, logs): logs holds `{split}_loss` and, when the provider decodes, the `{split}_` calc_metrics keys
        of the decoded forecast against the decoded target (reference :180-203)"""
        frames, v = self.frames_latents(batch)
        return self.validate_latents(v, batch_idx, split, frames=frames)

    @torch.no_grad()
    def validate_latents(self, v, batch_idx=0, split="val", frames=None):
        """validation_step on latents (B, T, C, h, w).  `frames` (B, T, 1, H, W): the observed frames behind `v`; with
        `verification` set they score the decoded forecast, persistence (the last input frame, lead stride 0) and the
        decoded target (the autoencoder's floor) per lead in one launch pair, from views of the batch"""
        loss, pred, rows = self.latent_loss(v)
        logs = {f"{split}_loss": loss}
        ae = self.autoencoder
        if ae is not None and getattr(ae, "can_decode", lambda: False)():
            L, P, f = self.predictor.in_rows, self.predictor.out_rows, self.predictor.features
            b, _, c, h, w = v.shape
            shape = (b, self.pred_frames, c, h, w)
            fc = ops.dlinear_forecast(pred, rows, L, f).view(shape)
            tgt = ops.dlinear_forecast(ops.dlinear_target(rows, L, P, f), rows, L, f).view(shape)
            decoded_pred, decoded_tgt = ae.decode(fc), ae.decode(tgt)
            logs.update(helpers.log_metrics(decoded_pred, decoded_tgt, split))
            if self.verification is not None and frames is not None:
                n = self.input_frames
                self.verification.add({"forecast": decoded_pred, "persistence": frames[:, n - 1],
                                       "reconstruction": decoded_tgt}, frames[:, n:])
            if self.panels is not None:
                epochs, key, prefix, suffix = self.plot_style
                e, tv = self.panels.epoch, self.panels.total("val")     # every script times both splits by total_val_steps
                if split != "test":
                    prefix = suffix = ""
                helpers.plot_panels(self, decoded_pred, decoded_tgt,
                                    f"{prefix}Reconstruction vs Original_epoch_{e}_batch_{batch_idx}{suffix}",
                                    e * tv + batch_idx if epochs else batch_idx,
                                    helpers.plot_fraction(self.cfg, key, 0.05), tv)
        return loss, logs

    def test_step(self, batch, batch_idx=0):
        return self.validation_step(batch, batch_idx, split="test")

