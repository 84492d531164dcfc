"""Plain-torch restatement (any dtype, no library import) of the conv + attention latent autoencoder of the reference's
experiments/v1_experiments/pretrained_ae_convattn_ae_sevir/train.py and of what csrc/convattn.hip computes: attention with
separate query / key lengths and a dropout mask on the probabilities, GroupNorm (+ pre-bias) + exact GELU, the one-key
cross-attention in closed form, the pre-norm encoder / decoder layers with their dropout sites and given masks, the whole
model on a state dict with torch's keys, and the Huber step.  Run in float64 it is the reference of
tests/test_convattn_gpu.py; run in float32 on the same inputs it is the yardstick that sets the tolerance there.  Backward
passes come from torch autograd (the masks are constants).  tests/test_convattn_cpu.py checks the restatement itself against
torch's own layers and against tests/golden/g18_convattn.npz.  The generator and LayerNorm are tests/transformer_ref.py's."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import transformer_ref as T
from tests.convae_ref import BIG, NSAMPLE, keys_digest, sample_index, spread, values_digest  # noqa: F401

E, H, FF, LAYERS, LATENT, GROUPS, GN_EPS = 128, 8, 512, 4, 512, 8, 1e-5
G18_SAMPLE = 128     # the fixture holds 148 tensors three times: tensors above this many elements are stored as a sample


def g18_index(numel):
    """the elements of a flattened tensor that tests/golden/g18_convattn.npz stores for it: 128 of them, evenly spread, at
    the largest stride <= numel / 128 that shares no factor with numel.  The stride is then coprime with every row length
    (and tap count) of the tensor, so the sample walks through the columns of a weight matrix instead of sitting in one."""
    step = numel // G18_SAMPLE
    while math.gcd(step, numel) != 1:
        step -= 1
    return torch.arange(G18_SAMPLE) * step


# ------------------------------------------------------------------------------------------------ kernels, restated
def attn_mask(seed, N, Hh, Sq, Skv, p):
    """keep mask (N, H, Sq, Skv) of wfae_attn_fwd: index ((n H + h) Sq + i) Skv + j"""
    return T.keep_mask(seed, (N, Hh, Sq, Skv), p)


def _drop(t, mask, p):
    return t if mask is None else t * T._mask_scale(mask, p, t).view(t.shape)


def attention(q, k, v, N, Sq, Skv, Hh, mask=None, p=0.0, dtype=None):
    """q (N*Sq, E), k, v (N*Skv, E), batch-first rows -> (out (N*Sq, E), probabilities before dropout (N, H, Sq, Skv))"""
    q, k, v = T._cast(dtype, q, k, v)
    D = q.shape[1] // Hh
    qh = q.reshape(N, Sq, Hh, D).transpose(1, 2)
    kh = k.reshape(N, Skv, Hh, D).transpose(1, 2)
    vh = v.reshape(N, Skv, Hh, D).transpose(1, 2)
    probs = ((qh * D ** -0.5) @ kh.transpose(-2, -1)).softmax(-1)
    o = _drop(probs, mask, p) @ vh
    return o.transpose(1, 2).reshape(N * Sq, Hh * D), probs


def head_dropout_bcast(v, Sq, Hh, mask=None, p=0.0, dtype=None):
    """v (N, E) -> (N*Sq, E): attention over one key; mask (N, H, Sq) (or (N, H, Sq, 1)) on the probability 1"""
    (v,) = T._cast(dtype, v)
    N, Ee = v.shape
    out = v.view(N, 1, Hh, Ee // Hh).expand(N, Sq, Hh, Ee // Hh)
    if mask is not None:
        m = T._mask_scale(mask, p, v).reshape(N, Hh, Sq).transpose(1, 2).unsqueeze(-1)
        out = out * m
    return out.reshape(N * Sq, Ee)


def group_norm_act(x, gamma, beta, groups, eps=GN_EPS, act=True, bias=None, dtype=None):
    """act(GroupNorm(x + bias[c])), two-pass statistics -> (y, mean (N, G), rstd (N, G))"""
    x, gamma, beta, bias = T._cast(dtype, x, gamma, beta, bias)
    N, C = x.shape[:2]
    if bias is not None:
        x = x + bias.view(1, C, *([1] * (x.dim() - 2)))
    g = x.reshape(N, groups, -1)
    mu = g.mean(-1, keepdim=True)
    d = g - mu
    rstd = ((d * d).mean(-1, keepdim=True) + eps).rsqrt()
    shape = (1, C) + (1,) * (x.dim() - 2)
    z = (d * rstd).reshape(x.shape) * gamma.view(shape) + beta.view(shape)
    return (F.gelu(z) if act else z), mu.reshape(N, groups), rstd.reshape(N, groups)


def gn_inputs(N, C, Hh, W, groups, kind, seed):
    """seeded fp32 inputs of one GroupNorm unit: x, pre-bias, gamma, beta, dy.  kind as tests/bn_ref.py mixes them:
    'benign'; 'offset': group 1 of every sample sits 100 sigma from zero; 'constant': group 0 of sample 0 is one value;
    'spike': one element of the last group is 1000 sigma"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, Hh, W, generator=g)
    cpg = C // groups
    if kind == "offset":
        x[:, cpg * (1 % groups):cpg * (1 % groups) + cpg] += 100.0
    elif kind == "constant":
        x[0, :cpg] = 0.75
    elif kind == "spike":
        x[-1, -1, -1, -1] = 1000.0
    elif kind != "benign":
        raise ValueError(kind)
    return {"x": x, "bias": 0.5 * torch.randn(C, generator=g), "gamma": 1.0 + 0.3 * torch.randn(C, generator=g),
            "beta": 0.3 * torch.randn(C, generator=g), "dy": torch.randn(N, C, Hh, W, generator=g)}


def gn_oracle(inp, groups, act, with_bias, dtype):
    """forward + backward of one unit in `dtype` -> dict y, mean, rstd, dx, dgamma, dbeta, dbias"""
    t = {k: v.detach().to(dtype).clone() for k, v in inp.items()}
    for k in ("x", "bias", "gamma", "beta"):
        t[k].requires_grad_(True)
    y, mean, rstd = group_norm_act(t["x"], t["gamma"], t["beta"], groups, GN_EPS, act, t["bias"] if with_bias else None)
    y.backward(t["dy"])
    return {"y": y.detach(), "mean": mean.detach(), "rstd": rstd.detach(), "dx": t["x"].grad, "dgamma": t["gamma"].grad,
            "dbeta": t["beta"].grad, "dbias": t["bias"].grad if with_bias else None}


# ------------------------------------------------------------------------------------------------ layers
def encoder_mask_shapes(N, S, Ee=E, Hh=H, ff=FF):
    """shapes of the four dropout masks of encoder_layer, in the order the seeds are drawn"""
    return [(N, Hh, S, S), (N * S, Ee), (N * S, ff), (N * S, Ee)]


def decoder_mask_shapes(N, S, Ee=E, Hh=H, ff=FF):
    """shapes of the six dropout masks of decoder_layer, in the order the seeds are drawn"""
    return [(N, Hh, S, S), (N * S, Ee), (N, Hh, S, 1), (N * S, Ee), (N * S, ff), (N * S, Ee)]


def _self_attn(sd, pre, h, N, S, Hh, mask, p):
    Ee = h.shape[1]
    qkv = F.linear(h, sd[pre + "in_proj_weight"], sd[pre + "in_proj_bias"])
    a, _ = attention(qkv[:, :Ee], qkv[:, Ee:2 * Ee], qkv[:, 2 * Ee:], N, S, S, Hh, mask, p)
    return F.linear(a, sd[pre + "out_proj.weight"], sd[pre + "out_proj.bias"])


def _ff(sd, h, m_act, m_out, p):
    f = _drop(F.gelu(F.linear(h, sd["linear1.weight"], sd["linear1.bias"])), m_act, p)
    return _drop(F.linear(f, sd["linear2.weight"], sd["linear2.bias"]), m_out, p)


def _ln(sd, name, x):
    return T.layernorm(x, None, sd[name + ".weight"], sd[name + ".bias"])[0]


def encoder_layer(sd, x, nhead=H, masks=None, p=0.0, dtype=None):
    """pre-norm nn.TransformerEncoderLayer (GELU, batch-first) on x (N, S, E) with the layer's own keys.  Dropout sites
    in seed order: attention probabilities, dropout1, feed-forward dropout, dropout2"""
    (x,) = T._cast(dtype, x)
    sd = dict(zip(sd.keys(), T._cast(dtype, *sd.values())))
    N, S, Ee = x.shape
    m = [None] * 4 if masks is None else list(masks)
    h = x.reshape(N * S, Ee)
    h = h + _drop(_self_attn(sd, "self_attn.", _ln(sd, "norm1", h), N, S, nhead, m[0], p), m[1], p)
    h = h + _ff(sd, _ln(sd, "norm2", h), m[2], m[3], p)
    return h.view(N, S, Ee)


def decoder_layer(sd, x, memory, nhead=H, masks=None, p=0.0, dtype=None, full_cross=False):
    """pre-norm nn.TransformerDecoderLayer (GELU, batch-first) on x (N, S, E) with a one-token memory (N, E).  Dropout
    sites in seed order: self-attention probabilities, dropout1, cross-attention probabilities, dropout2, feed-forward
    dropout, dropout3.  The cross-attention is the closed form out_proj(mask * v_proj(memory)); full_cross forms it as
    torch does — norm2, q and k projections, softmax over the one key — so that the dead gradients can be looked at."""
    x, memory = T._cast(dtype, x, memory)
    sd = dict(zip(sd.keys(), T._cast(dtype, *sd.values())))
    N, S, Ee = x.shape
    m = [None] * 6 if masks is None else list(masks)
    h = x.reshape(N * S, Ee)
    h = h + _drop(_self_attn(sd, "self_attn.", _ln(sd, "norm1", h), N, S, nhead, m[0], p), m[1], p)
    w, b = sd["multihead_attn.in_proj_weight"], sd["multihead_attn.in_proj_bias"]
    if full_cross:
        q = F.linear(_ln(sd, "norm2", h), w[:Ee], b[:Ee])
        kv = F.linear(memory, w[Ee:], b[Ee:])
        c, _ = attention(q, kv[:, :Ee], kv[:, Ee:], N, S, 1, nhead, m[2], p)
    else:
        c = head_dropout_bcast(F.linear(memory, w[2 * Ee:], b[2 * Ee:]), S, nhead, m[2], p)
    h = h + _drop(F.linear(c, sd["multihead_attn.out_proj.weight"], sd["multihead_attn.out_proj.bias"]), m[3], p)
    h = h + _ff(sd, _ln(sd, "norm3", h), m[4], m[5], p)
    return h.view(N, S, Ee)


def sub(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


# ------------------------------------------------------------------------------------------------ the model
def _layer_keys(pre, decoder, e=E, ff=FF):
    out = [(pre + "self_attn.in_proj_weight", (3 * e, e)), (pre + "self_attn.in_proj_bias", (3 * e,)),
           (pre + "self_attn.out_proj.weight", (e, e)), (pre + "self_attn.out_proj.bias", (e,))]
    if decoder:
        out += [(pre + "multihead_attn.in_proj_weight", (3 * e, e)), (pre + "multihead_attn.in_proj_bias", (3 * e,)),
                (pre + "multihead_attn.out_proj.weight", (e, e)), (pre + "multihead_attn.out_proj.bias", (e,))]
    out += [(pre + "linear1.weight", (ff, e)), (pre + "linear1.bias", (ff,)), (pre + "linear2.weight", (e, ff)),
            (pre + "linear2.bias", (e,))]
    for n in ("norm1", "norm2") + (("norm3",) if decoder else ()):
        out += [(pre + n + ".weight", (e,)), (pre + n + ".bias", (e,))]
    return out


def key_list(in_channels=4, size=48, e=E, layers=LAYERS, latent=LATENT):
    """[(key, shape)] of the reference ConvAttnModel's state_dict, in its order"""
    s = (size // 4) ** 2
    out = [("encoder_pos_embedding", (1, s, e)), ("pooling_query", (1, 1, e)), ("decoder_queries", (1, s, e)),
           ("decoder_pos_embedding", (1, s, e)),
           ("encoder_cnn.0.weight", (64, in_channels, 3, 3)), ("encoder_cnn.0.bias", (64,)),
           ("encoder_cnn.1.weight", (64,)), ("encoder_cnn.1.bias", (64,)),
           ("encoder_cnn.3.weight", (e, 64, 3, 3)), ("encoder_cnn.3.bias", (e,)),
           ("encoder_cnn.4.weight", (e,)), ("encoder_cnn.4.bias", (e,))]
    for i in range(layers):
        out += _layer_keys(f"encoder_tf.layers.{i}.", False, e, 4 * e)
    out += [("attention_pool.in_proj_weight", (3 * e, e)), ("attention_pool.in_proj_bias", (3 * e,)),
            ("attention_pool.out_proj.weight", (e, e)), ("attention_pool.out_proj.bias", (e,)),
            ("encoder_head.0.weight", (e,)), ("encoder_head.0.bias", (e,)),
            ("encoder_head.1.weight", (latent, e)), ("encoder_head.1.bias", (latent,)),
            ("decoder_head.weight", (e, latent)), ("decoder_head.bias", (e,))]
    for i in range(layers):
        out += _layer_keys(f"decoder_tf.layers.{i}.", True, e, 4 * e)
    out += [("decoder_cnn.0.weight", (e, 64, 4, 4)), ("decoder_cnn.0.bias", (64,)),
            ("decoder_cnn.1.weight", (64,)), ("decoder_cnn.1.bias", (64,)),
            ("decoder_cnn.3.weight", (64, in_channels, 4, 4)), ("decoder_cnn.3.bias", (in_channels,))]
    return out


def dead_list(layers=LAYERS, e=E):
    """[(key, lo, hi)] of the parameters (rows lo:hi; -1, -1: the whole tensor) whose gradient is mathematically zero.
    (a) With one key the decoder's cross-attention has a softmax of 1, so norm2 and the q / k rows of its in-projection
    cannot reach the output.  (b) In every softmax attention the key bias adds the same q . b_k to all scores of a row,
    which the softmax cancels: rows e:2e of every in_proj_bias."""
    out = []
    for i in range(layers):
        out.append((f"encoder_tf.layers.{i}.self_attn.in_proj_bias", e, 2 * e))
    out.append(("attention_pool.in_proj_bias", e, 2 * e))
    for i in range(layers):
        pre = f"decoder_tf.layers.{i}."
        out += [(pre + "self_attn.in_proj_bias", e, 2 * e),
                (pre + "multihead_attn.in_proj_weight", 0, 2 * e), (pre + "multihead_attn.in_proj_bias", 0, 2 * e),
                (pre + "norm2.weight", -1, -1), (pre + "norm2.bias", -1, -1)]
    return out


def live_part(key, t, dead=None):
    """the part of tensor `t` of parameter `key` that is live: None for a dead tensor, the rows outside a dead slice, else t"""
    for k, lo, hi in (dead_list() if dead is None else dead):
        if k == key:
            return None if lo < 0 else torch.cat([t[:lo], t[hi:]])
    return t


def dead_part(key, t, dead=None):
    """the dead rows of `t` (the whole tensor for a dead one), None for a live parameter"""
    for k, lo, hi in (dead_list() if dead is None else dead):
        if k == key:
            return t if lo < 0 else t[lo:hi]
    return None


def n_layers(sd, prefix):
    return 1 + max(int(k[len(prefix):].split(".")[0]) for k in sd if k.startswith(prefix))


def mask_shapes(N, S, layers=LAYERS, Ee=E, Hh=H):
    """every dropout mask of one training forward, in the order the model draws its seeds (the attention pool's dropout is 0)"""
    out = []
    for _ in range(layers):
        out += encoder_mask_shapes(N, S, Ee, Hh, 4 * Ee)
    for _ in range(layers):
        out += decoder_mask_shapes(N, S, Ee, Hh, 4 * Ee)
    return out


def encode(sd, x, masks=None, p=0.0, nhead=H):
    N = x.shape[0]
    y = F.conv2d(x, sd["encoder_cnn.0.weight"], sd["encoder_cnn.0.bias"], stride=2, padding=1)
    y = group_norm_act(y, sd["encoder_cnn.1.weight"], sd["encoder_cnn.1.bias"], GROUPS)[0]
    y = F.conv2d(y, sd["encoder_cnn.3.weight"], sd["encoder_cnn.3.bias"], stride=2, padding=1)
    y = group_norm_act(y, sd["encoder_cnn.4.weight"], sd["encoder_cnn.4.bias"], GROUPS)[0]
    t = y.flatten(2).transpose(1, 2) + sd["encoder_pos_embedding"]
    S, Ee = t.shape[1], t.shape[2]
    L = n_layers(sd, "encoder_tf.layers.")
    for i in range(L):
        t = encoder_layer(sub(sd, f"encoder_tf.layers.{i}."), t, nhead, None if masks is None else masks[4 * i:4 * i + 4], p)
    w, b = sd["attention_pool.in_proj_weight"], sd["attention_pool.in_proj_bias"]
    q = F.linear(sd["pooling_query"].reshape(1, Ee).expand(N, Ee), w[:Ee], b[:Ee])
    kv = F.linear(t.reshape(N * S, Ee), w[Ee:], b[Ee:])
    pooled, _ = attention(q, kv[:, :Ee], kv[:, Ee:], N, 1, S, nhead)
    pooled = F.linear(pooled, sd["attention_pool.out_proj.weight"], sd["attention_pool.out_proj.bias"])
    return F.linear(_ln(sd, "encoder_head.0", pooled), sd["encoder_head.1.weight"], sd["encoder_head.1.bias"])


def decode(sd, z, masks=None, p=0.0, nhead=H, full_cross=False):
    N = z.shape[0]
    memory = F.linear(z, sd["decoder_head.weight"], sd["decoder_head.bias"])
    t = (sd["decoder_queries"] + sd["decoder_pos_embedding"]).expand(N, -1, -1)
    S, Ee = t.shape[1], t.shape[2]
    L = n_layers(sd, "decoder_tf.layers.")
    for i in range(L):
        t = decoder_layer(sub(sd, f"decoder_tf.layers.{i}."), t, memory, nhead,
                          None if masks is None else masks[6 * i:6 * i + 6], p, full_cross=full_cross)
    side = int(round(S ** 0.5))
    y = t.transpose(1, 2).reshape(N, Ee, side, side)
    y = F.conv_transpose2d(y, sd["decoder_cnn.0.weight"], None, stride=2, padding=1)
    y = group_norm_act(y, sd["decoder_cnn.1.weight"], sd["decoder_cnn.1.bias"], GROUPS, bias=sd["decoder_cnn.0.bias"])[0]
    return F.conv_transpose2d(y, sd["decoder_cnn.3.weight"], sd["decoder_cnn.3.bias"], stride=2, padding=1)


def forward(sd, x, masks=None, p=0.0, nhead=H, full_cross=False):
    """x (B, C, size, size) -> (z, recon).  masks: mask_shapes(...) keep masks (training), else eval"""
    L = n_layers(sd, "encoder_tf.layers.")
    z = encode(sd, x, None if masks is None else masks[:4 * L], p, nhead)
    return z, decode(sd, z, None if masks is None else masks[4 * L:], p, nhead, full_cross)


def run(sd, x, dtype, masks=None, p=0.0, full_cross=False):
    """one forward + backward of the Huber step in `dtype` on detached copies -> (loss, z, recon, {key: grad}); a parameter
    that does not enter the graph (the dead ones in the closed form) gets a zero gradient"""
    prm = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    x = x.to(dtype)
    z, recon = forward(prm, x, masks, p, full_cross=full_cross)
    loss = F.huber_loss(recon, x, delta=1.0)
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in prm.items()}
    return loss.detach(), z.detach(), recon.detach(), grads


def grad_norm(grads):
    return float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values())))


def seeded_masks(seeds, shapes, p):
    return [T.keep_mask(s, shape, p) for s, shape in zip(seeds, shapes)]
