"""Conv + attention latent autoencoder of the reference's v1 experiments:
experiments/v1_experiments/pretrained_ae_convattn_ae_sevir/train.py without Lightning / W&B.

Reference `ConvAttnModel` (:58-161).  Encode: the latents (B, 4, 48, 48) go through two [Conv2d 3x3 stride 2 + GroupNorm(8)
+ GELU] units to (B, 128, 12, 12), become 144 tokens of 128 with a learned positional embedding, pass four pre-norm
nn.TransformerEncoderLayer (8 heads of 16, feed-forward 512, GELU, dropout 0.1), are pooled by an nn.MultiheadAttention
with one learned query, and LayerNorm + Linear give `z` (B, 512).  Decode: Linear 512 -> 128 gives a ONE-token memory; the
144 learned queries + positional embedding pass four pre-norm nn.TransformerDecoderLayer (self-attention over the 144
tokens, cross-attention to the memory, feed-forward), are laid out as (B, 128, 12, 12) and go through
[ConvTranspose2d 4x4 stride 2 + GroupNorm(8) + GELU] and ConvTranspose2d 4x4 stride 2.  The step (:186-203) takes
nn.HuberLoss between the reconstruction and the latents themselves.

torch's own module classes are kept as parameter containers, built in the reference's order with its `init_weights`, so
state_dict keys / order / shapes and the seeded initial values are the reference's.  forward / encode / decode run on
libwfae kernels only (csrc/convattn.hip for attention, GroupNorm + GELU, the last bias and the cross-attention; csrc/c3s2.hip
and the 4x4 stride-2 family for the convolutions; the latent transformer's LayerNorm, Linear, GELU and dropout kernels).

Pre-norm layers (`encoder_layer`, `decoder_layer`).  Dropout seeds are drawn through Fn.next_seed() in this order, and only
in training with p > 0:
  encoder layer: 1 attention probabilities (N, H, S, S)   2 dropout1 (N*S, E)   3 feed-forward dropout (N*S, FF)
                 4 dropout2 (N*S, E)
  decoder layer: 1 self-attention probabilities (N, H, S, S)   2 dropout1 (N*S, E)   3 cross-attention probabilities
                 (N, H, S, 1)   4 dropout2 (N*S, E)   5 feed-forward dropout (N*S, FF)   6 dropout3 (N*S, E)
Masks index the contiguous tensors of those shapes (tests/convattn_ref.py regenerates them).

The decoder's cross-attention has ONE key, so its softmax is identically 1 and the layer reduces to
out_proj(dropout_heads(v_proj(memory))) broadcast over the queries: `norm2`, the q projection and the k projection do not
reach the output, and are not launched.  Their gradients — `norm2.{weight,bias}` and rows 0:2E of
`multihead_attn.in_proj_{weight,bias}` of every decoder layer, the DEAD parameters — are mathematically zero (torch returns
rounding noise there, which AdamW would normalise into a random walk) and are written as exact zeros: the optimiser applies
its weight decay to them and nothing else.  The same holds for the KEY BIAS of every softmax attention (rows E:2E of each
`in_proj_bias`): it shifts all scores of a row alike, the softmax cancels it, and its gradient is a sum of rounding errors.
`dead_parameters` lists them all.
"""
from __future__ import annotations

import warnings

import torch
import torch.nn as tnn

from ... import functional as Fn
from ... import ops
from ..._lib import WfaeError
from ...pipeline import helpers
from ._latents import Autoencoder  # noqa: F401  (the frozen latent provider)
from ._runner import Step

HEAD_DIM = ops.ATTN_D
MAX_TOKENS = ops.ATTN_MAX_S


class ToTokensFn(torch.autograd.Function):
    """(B, C, H, W) -> token rows (B*H*W, C) (`.flatten(2).transpose(1, 2)`) and back: the patch permutation at P = 1"""

    @staticmethod
    def forward(ctx, x):
        ctx.shape = x.shape
        return ops.patchify(Fn._c(x), 1)

    @staticmethod
    def backward(ctx, dy):
        b, c, h, w = ctx.shape
        return ops.unpatchify(Fn._c(dy), None, b, c, h, w, 1)


class FromTokensFn(torch.autograd.Function):
    """token rows (B*H*W, C) -> (B, C, H, W) (`.transpose(1, 2).reshape(B, C, H, W)`)"""

    @staticmethod
    def forward(ctx, rows, b, c, h, w):
        return ops.unpatchify(Fn._c(rows), None, b, c, h, w, 1)

    @staticmethod
    def backward(ctx, dy):
        return ops.patchify(Fn._c(dy), 1), None, None, None, None


def _norm(x, ln):
    return Fn.AddLayerNormFn.apply(x, None, ln.weight, ln.bias, ln.eps)


def _lin(x, m):
    return Fn.LinearFn.apply(x, m.weight, m.bias)


def _check_attn(what, at, e):
    if not at._qkv_same_embed_dim or at.bias_k is not None or at.in_proj_bias is None or at.add_zero_attn:
        raise WfaeError(f"{what}: only the packed in-projection with bias is built")
    if at.embed_dim != e or at.head_dim != HEAD_DIM:
        raise WfaeError(f"{what}: embed_dim {at.embed_dim} with {at.num_heads} heads gives heads of {at.head_dim}; "
                        f"heads of {HEAD_DIM} are built")


def _self_attention(h, at, n, s, training):
    """h (n*s, E) normalised rows -> out_proj(attention) (n*s, E); one seed when the probabilities are dropped"""
    p = float(at.dropout) if training else 0.0
    qkv = Fn.InProjFn.apply(h, at.in_proj_weight, at.in_proj_bias, at.embed_dim)
    a = Fn.AttnFn.apply(qkv, None, n, s, s, at.num_heads, p, Fn.next_seed() if p > 0 else 0)
    return _lin(a, at.out_proj)


def _feed_forward(h, layer, drop, training):
    f = Fn.dropout(Fn.GeluFn.apply(_lin(h, layer.linear1)), layer.dropout.p, training)
    return Fn.dropout(_lin(f, layer.linear2), drop.p, training)


def _check_layer(what, layer, e):
    if not layer.norm_first:
        raise WfaeError(f"{what}: the pre-norm (norm_first) configuration is built here")
    if layer.activation is not torch.nn.functional.gelu:
        raise WfaeError(f"{what}: only GELU is built")
    _check_attn(what, layer.self_attn, e)


def encoder_layer(layer, x, n, s):
    """pre-norm nn.TransformerEncoderLayer on token rows x (n*s, E):
    x + dropout1(self_attn(norm1 x)), then + dropout2(linear2(dropout(gelu(linear1(norm2 .)))))"""
    _check_layer("encoder_layer", layer, x.shape[1])
    tr = layer.training
    a = Fn.dropout(_self_attention(_norm(x, layer.norm1), layer.self_attn, n, s, tr), layer.dropout1.p, tr)
    x = Fn.AddFn.apply(x, a)
    return Fn.AddFn.apply(x, _feed_forward(_norm(x, layer.norm2), layer, layer.dropout2, tr))


def decoder_layer(layer, x, memory, n, s):
    """pre-norm nn.TransformerDecoderLayer on token rows x (n*s, E) with a ONE-token memory (n, E): self-attention,
    the closed form of the one-key cross-attention (module docstring), feed-forward"""
    e = x.shape[1]
    _check_layer("decoder_layer", layer, e)
    _check_attn("decoder_layer", layer.multihead_attn, e)
    if memory.dim() != 2 or tuple(memory.shape) != (n, e):
        raise WfaeError(f"decoder_layer: the memory is one token per sample, ({n}, {e}); got {tuple(memory.shape)}")
    tr = layer.training
    a = Fn.dropout(_self_attention(_norm(x, layer.norm1), layer.self_attn, n, s, tr), layer.dropout1.p, tr)
    x = Fn.AddFn.apply(x, a)
    ca = layer.multihead_attn
    p = float(ca.dropout) if tr else 0.0
    v = Fn.LinearRowsFn.apply(memory, ca.in_proj_weight, ca.in_proj_bias, 2 * e, 3 * e, layer.norm2.weight,
                              layer.norm2.bias)
    c = Fn.HeadDropoutBcastFn.apply(v, s, ca.num_heads, p, Fn.next_seed() if p > 0 else 0)
    x = Fn.AddFn.apply(x, Fn.dropout(_lin(c, ca.out_proj), layer.dropout2.p, tr))
    return Fn.AddFn.apply(x, _feed_forward(_norm(x, layer.norm3), layer, layer.dropout3, tr))


def dead_parameters(model):
    """[(state_dict key, row slice or None for the whole tensor)] of the parameters that cannot influence the output
    (module docstring): their gradients are exact zeros"""
    e = model.transformer_embed_dim
    out = [(f"encoder_tf.layers.{i}.self_attn.in_proj_bias", slice(e, 2 * e)) for i in range(len(model.encoder_tf.layers))]
    out.append(("attention_pool.in_proj_bias", slice(e, 2 * e)))
    for i in range(len(model.decoder_tf.layers)):
        pre = f"decoder_tf.layers.{i}."
        out += [(pre + "self_attn.in_proj_bias", slice(e, 2 * e)),
                (pre + "multihead_attn.in_proj_weight", slice(0, 2 * e)), (pre + "multihead_attn.in_proj_bias", slice(0, 2 * e)),
                (pre + "norm2.weight", None), (pre + "norm2.bias", None)]
    return out


class ConvAttnModel(tnn.Module):
    """reference :58-161.  Keyword-only extensions with the reference's values as defaults: `size`, the latent plane
    (a multiple of 4; (size / 4)^2 tokens, at most 256), next to the reference's `in_channels`."""

    def __init__(self, in_channels=4, transformer_embed_dim=128, nhead=8, num_tf_layers=4, latent_dim=512, *, size=48):
        super().__init__()
        if size < 4 or size % 4 != 0:
            raise WfaeError(f"ConvAttnModel: size must be a positive multiple of 4 (two stride-2 stages), got {size}")
        self.tokens = (size // 4) ** 2
        if self.tokens > MAX_TOKENS:
            raise WfaeError(f"ConvAttnModel: size {size} gives {self.tokens} tokens, the attention kernels serve <= {MAX_TOKENS}")
        if transformer_embed_dim != nhead * HEAD_DIM:
            raise WfaeError(f"ConvAttnModel: {transformer_embed_dim} / {nhead} heads: heads of {HEAD_DIM} are built")
        e = self.transformer_embed_dim = transformer_embed_dim
        self.in_channels, self.size, self.plane = in_channels, size, size // 4
        self.encoder_cnn = tnn.Sequential(
            tnn.Conv2d(in_channels, 64, kernel_size=3, stride=2, padding=1), tnn.GroupNorm(8, 64), tnn.GELU(),
            tnn.Conv2d(64, e, kernel_size=3, stride=2, padding=1), tnn.GroupNorm(8, e), tnn.GELU())
        self.encoder_pos_embedding = tnn.Parameter(torch.randn(1, self.tokens, e))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")      # torch notes that a pre-norm layer disables its nested-tensor path
            self.encoder_tf = tnn.TransformerEncoder(
                tnn.TransformerEncoderLayer(d_model=e, nhead=nhead, dim_feedforward=e * 4, activation="gelu",
                                            batch_first=True, norm_first=True), num_layers=num_tf_layers)
        self.pooling_query = tnn.Parameter(torch.randn(1, 1, e))
        self.attention_pool = tnn.MultiheadAttention(embed_dim=e, num_heads=nhead, batch_first=True)
        self.encoder_head = tnn.Sequential(tnn.LayerNorm(e), tnn.Linear(e, latent_dim))
        self.decoder_head = tnn.Linear(latent_dim, e)
        self.decoder_queries = tnn.Parameter(torch.randn(1, self.tokens, e))
        self.decoder_pos_embedding = tnn.Parameter(torch.randn(1, self.tokens, e))
        self.decoder_tf = tnn.TransformerDecoder(
            tnn.TransformerDecoderLayer(d_model=e, nhead=nhead, dim_feedforward=e * 4, activation="gelu", batch_first=True,
                                        norm_first=True), num_layers=num_tf_layers)
        self.decoder_cnn = tnn.Sequential(
            tnn.ConvTranspose2d(e, 64, kernel_size=4, stride=2, padding=1), tnn.GroupNorm(8, 64), tnn.GELU(),
            tnn.ConvTranspose2d(64, in_channels, kernel_size=4, stride=2, padding=1))
        self.apply(self.init_weights)

    def init_weights(self, m):
        if isinstance(m, (tnn.Linear, tnn.Conv2d, tnn.ConvTranspose2d)):
            tnn.init.kaiming_normal_(m.weight, nonlinearity="relu")
            if m.bias is not None:
                tnn.init.zeros_(m.bias)
        elif isinstance(m, (tnn.LayerNorm, tnn.GroupNorm)):
            tnn.init.ones_(m.weight)
            tnn.init.zeros_(m.bias)

    @staticmethod
    def _conv_gn_gelu(x, conv, gn):
        y = Fn.conv3x3s2_act(x, conv.weight, conv.bias, transposed=False, act=False)
        return Fn.GroupNormActFn.apply(y, gn.weight, gn.bias, None, gn.num_groups, gn.eps, 1)

    def encode(self, x):
        """x (B, C, size, size) -> z (B, latent_dim)"""
        if x.dim() != 4 or tuple(x.shape[1:]) != (self.in_channels, self.size, self.size):
            raise WfaeError(f"ConvAttnModel.encode: expected (B, {self.in_channels}, {self.size}, {self.size}), got "
                            f"{tuple(x.shape)}")
        b, s, e = x.shape[0], self.tokens, self.transformer_embed_dim
        cnn = self.encoder_cnn
        y = self._conv_gn_gelu(self._conv_gn_gelu(x, cnn[0], cnn[1]), cnn[3], cnn[4])
        t = Fn.AddBcastFn.apply(ToTokensFn.apply(y).view(b, s * e), self.encoder_pos_embedding).view(b * s, e)
        for layer in self.encoder_tf.layers:
            t = encoder_layer(layer, t, b, s)
        at = self.attention_pool
        _check_attn("attention_pool", at, e)
        q, kv = Fn.SplitInProjFn.apply(Fn.ExpandRowsFn.apply(self.pooling_query, b), t, at.in_proj_weight, at.in_proj_bias, e)
        p = float(at.dropout) if self.training else 0.0
        pooled = _lin(Fn.AttnFn.apply(q, kv, b, 1, s, at.num_heads, p, Fn.next_seed() if p > 0 else 0), at.out_proj)
        return _lin(_norm(pooled, self.encoder_head[0]), self.encoder_head[1])

    def decode(self, z):
        """z (B, latent_dim) -> reconstruction (B, C, size, size)"""
        if z.dim() != 2 or z.shape[1] != self.decoder_head.in_features:
            raise WfaeError(f"ConvAttnModel.decode: expected (B, {self.decoder_head.in_features}), got {tuple(z.shape)}")
        b, s, e = z.shape[0], self.tokens, self.transformer_embed_dim
        memory = _lin(z, self.decoder_head)
        t = Fn.AddBcastFn.apply(Fn.ExpandRowsFn.apply(self.decoder_queries, b), self.decoder_pos_embedding).view(b * s, e)
        for layer in self.decoder_tf.layers:
            t = decoder_layer(layer, t, memory, b, s)
        cnn = self.decoder_cnn
        y = Fn.ConvT4x4UpFn.apply(FromTokensFn.apply(t, b, e, self.plane, self.plane), cnn[0].weight)
        y = Fn.GroupNormActFn.apply(y, cnn[1].weight, cnn[1].bias, cnn[0].bias, cnn[1].num_groups, cnn[1].eps, 1)
        return Fn.ChannelBiasFn.apply(Fn.ConvT4x4UpFn.apply(y, cnn[3].weight), cnn[3].bias)

    def forward(self, x):
        """x (B, C, size, size) -> (z (B, latent_dim), reconstruction (B, C, size, size))"""
        z = self.encode(x)
        return z, self.decode(z)


def predictor_state(model):
    """the reference wraps the predictor in torch.compile, so its Lightning keys are `predictor._orig_mod.<key>`"""
    return {"predictor._orig_mod." + k: v for k, v in model.predictor.state_dict().items()}


def load_predictor_state(model, state_dict):
    """load `predictor.[_orig_mod.]<key>` entries of a checkpoint's state_dict into model.predictor (strict)"""
    sd = {}
    for k, v in state_dict.items():
        if k.startswith("predictor."):
            k = k[len("predictor."):]
            sd[k[len("_orig_mod."):] if k.startswith("_orig_mod.") else k] = v
    model.predictor.load_state_dict(sd, strict=True)


class Model(Step, tnn.Module):
    """reference Model (:163-229): `predictor`, `forward` on one-frame latents (B, 1, C, h, w), the training /
    validation / test steps; the optimiser is `Step`'s, with the exact complements of FusedAdamW"""

    exact_complements = True

    def __init__(self, cfg, autoencoder=None):
        super().__init__()
        self.cfg = cfg
        self.autoencoder = autoencoder
        self.input_frames, self.pred_frames = cfg.dataset.input_frames, cfg.dataset.pred_frames
        self.total_steps = cfg.trainer.total_train_steps
        cv = cfg.convattn
        self.predictor = ConvAttnModel(in_channels=int(cv.in_channels), transformer_embed_dim=int(cv.transformer_embed_dim),
                                       nhead=int(cv.nhead), num_tf_layers=int(cv.num_tf_layers),
                                       latent_dim=int(cv.latent_dim), size=int(cv.size))
        self.delta = 1.0   # nn.HuberLoss()

    def forward(self, x):
        """latents (B, T, C, h, w), frame by frame (the reference asserts T == 1) -> reconstruction of the same shape"""
        if x.dim() != 5:
            raise WfaeError(f"Model: expected latents (B, T, C, h, w), got {tuple(x.shape)}")
        b, t = x.shape[:2]
        return self.predictor(x.reshape(b * t, *x.shape[2:]))[1].view(x.shape)

    def latent_loss(self, v):
        """latents (B, T, C, h, w) -> (loss, reconstruction): Huber(predictor(v), v), reference :191-192"""
        v = v.contiguous()
        pred = self(v)
        return Fn.huber_loss(pred, v, self.delta), pred

    def _metric_interval(self, split):
        """the reference's metric cadence: every int(logging.log_<split>_all_metrics_n * total steps) batches"""
        lg = self.cfg.get("logging") or {}
        n = lg.get(f"log_{'train' if split == 'train' else 'val'}_all_metrics_n", 0) or 0
        return max(1, int(n * max(self.total_steps, 1)))

    def training_step(self, batch, batch_idx=0):
        """batch: frames (B, T, H, W) fp32 in [0, 1] ('NTHW') or latents (B, T, C, h, w); AdamW + cosine warmup, the
        gradient norm clipped at optim.gradient_clip_val.  -> (loss, gradient norm before clipping)"""
        _, v = self.frames_latents(batch)
        loss, _ = self.latent_loss(v)
        return self.optimizer_step(loss)

    @torch.no_grad()
    def validation_step(self, batch, batch_idx=0, split="val", plot_idx=None):
        """-> (loss, logs): logs holds `{split}_loss` and, for a batch of frames with a provider that decodes, the
        `{split}_` calc_metrics keys of the decoded reconstruction against the input frames (reference :214-217)"""
        frames, v = self.frames_latents(batch)
        loss, pred = self.latent_loss(v)
        logs = {f"{split}_loss": loss}
        ae = self.autoencoder
        if frames is not None and batch_idx % self._metric_interval(split) == 0 \
                and getattr(ae, "can_decode", lambda: False)():
            decoded_pred = ae.decode(pred)
            logs.update(helpers.log_metrics(decoded_pred, frames, split))
            if self.panels is not None:
                # reference :219-221; it has no test step: the port's takes the validation label with `_test` appended
                i = batch_idx if plot_idx is None else plot_idx
                label = f"Val_Reconstruction vs Original_epoch_{self.panels.epoch}_batch_{i}"
                helpers.plot_panels(self, decoded_pred, frames, label + ("_test" if split == "test" else ""), i,
                                    helpers.plot_fraction(self.cfg, "log_val_plots_n", 0.05), self.panels.total("val"))
        return loss, logs

    def test_step(self, batch, batch_idx=0):
        return self.validation_step(batch, 0, split="test", plot_idx=batch_idx)
