"""Plain restatement (numpy for the RNG, torch for the maths; any dtype, no library import) of what
csrc/transformer.hip and csrc/vit.hip compute: the counter-based dropout RNG, LayerNorm(x + res), multi-head attention
in both row layouts with dropout on the probabilities, single-query attention, and the post-norm
nn.TransformerEncoderLayer with its four dropout sites.  Run in float64 it is the reference of
tests/test_transformer_gpu.py; run in float32 on the same inputs it is the yardstick that sets the tolerance there.
Backward passes come from torch autograd on these functions (the masks are constants).
tests/test_transformer_ref_cpu.py checks the restatement itself against torch."""
import numpy as np
import torch
import torch.nn.functional as F

_G = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def rng01(seed, idx):
    """uniform [0, 1) from (seed, index): the splitmix64 finaliser of csrc/transformer.hip in wrapping uint64
    arithmetic; the top 24 bits times 2**-24, as float32 (exact)"""
    idx = np.atleast_1d(np.asarray(idx, dtype=np.uint64))           # arrays wrap silently, scalars would warn
    s = np.full(1, int(seed) & 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    z = s + idx * _G + _G
    z = (z ^ (z >> np.uint64(30))) * _M1
    z = (z ^ (z >> np.uint64(27))) * _M2
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)


def keep_mask(seed, n_or_shape, p):
    """bool mask (True = kept) of the elements 0..n-1 of a contiguous tensor.  p reaches the kernels as a C `float`,
    so the comparison is against float32(p), not the Python double"""
    shape = (int(n_or_shape),) if np.isscalar(n_or_shape) else tuple(int(v) for v in n_or_shape)
    n = int(np.prod(shape, dtype=np.int64))
    return (rng01(seed, np.arange(n, dtype=np.uint64)) >= np.float32(p)).reshape(shape)


def _cast(dtype, *ts):
    return [None if t is None else (t if dtype is None else t.to(dtype)) for t in ts]


def _mask_scale(mask, p, like):
    """mask / (1 - p) as a constant of like's dtype"""
    if not isinstance(mask, torch.Tensor):
        mask = torch.from_numpy(np.ascontiguousarray(mask))
    return mask.to(like.dtype) / (1.0 - p)


def layernorm(x, res, g, b, eps=1e-5, dtype=None):
    """two-pass LayerNorm over the last axis of h = x + res (res may be None) -> (y, mean, rstd)"""
    x, res, g, b = _cast(dtype, x, res, g, b)
    h = x if res is None else x + res
    mu = h.mean(-1, keepdim=True)
    d = h - mu
    rstd = ((d * d).mean(-1, keepdim=True) + eps).rsqrt()
    return d * rstd * g + b, mu.squeeze(-1), rstd.squeeze(-1)


def layernorm_bwd(x, res, g, b, dy, eps=1e-5, dtype=None):
    """(dh, dgamma, dbeta) of sum(y * dy) by autograd; dh is the gradient w.r.t. h = x + res (that of x and of res)"""
    x, res, g, b, dy = [None if t is None else t.detach() for t in _cast(dtype, x, res, g, b, dy)]
    x, g, b = x.clone().requires_grad_(True), g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y, _, _ = layernorm(x, res, g, b, eps)
    return torch.autograd.grad(y, (x, g, b), dy)


def mha(qkv, S, N, H, D, batch_first, mask=None, p=0.0, dtype=None):
    """qkv (S*N, 3*H*D), columns [q | k | v]; row = s*N + n (seq-first) or n*S + s (batch-first); attention over s
    for each (n, h), scale D**-0.5.  mask (N, H, S, S), indexed (n, h, query i, key j), multiplies the probabilities
    as P * mask / (1 - p).  Returns out (S*N, H*D) in the row order of qkv and the pre-dropout probabilities
    (N, H, S, S)."""
    (qkv,) = _cast(dtype, qkv)
    E = H * D
    x = qkv.view(N, S, 3, H, D).transpose(0, 1) if batch_first else qkv.view(S, N, 3, H, D)
    q, k, v = [x[:, :, c].permute(1, 2, 0, 3) for c in range(3)]          # (N, H, S, D)
    probs = ((q * D ** -0.5) @ k.transpose(-2, -1)).softmax(-1)
    pd = probs if mask is None else probs * _mask_scale(mask, p, probs)
    o = (pd @ v).permute(2, 0, 1, 3)                                       # (S, N, H, D)
    if batch_first:
        o = o.transpose(0, 1)
    return o.reshape(S * N, E), probs


def sq_attn(q, kv, B, L, H, D, dtype=None):
    """one query per batch element: q (B, H*D), kv (B*L, 2*H*D) with row = b*L + l and columns [k | v]
    -> out (B, H*D), probs (B, H, L)"""
    q, kv = _cast(dtype, q, kv)
    x = kv.view(B, L, 2, H, D)
    k, v = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2)          # (B, H, L, D)
    probs = ((q.view(B, H, 1, D) * D ** -0.5) @ k.transpose(-2, -1)).softmax(-1)   # (B, H, 1, L)
    return (probs @ v).reshape(B, H * D), probs.squeeze(2)


def layer_mask_shapes(S, N, H, E, FF):
    """shapes of the four dropout masks of encoder_layer, in the order the seeds are drawn"""
    return [(N, H, S, S), (S * N, E), (S * N, FF), (S * N, E)]


def encoder_layer(sd, x, nhead, batch_first, act, masks=None, p=0.0, dtype=None):
    """post-norm nn.TransformerEncoderLayer.forward on a state dict with torch's keys; x (S, N, E) or, batch-first,
    (N, S, E); act "relu" or "gelu" (erf).  Four dropout sites, in this order: attention probabilities, dropout1
    (after out_proj), dropout (after the activation), dropout2 (after linear2).  masks: four keep masks in that order,
    the last three over the elements of the contiguous (rows, features) tensors in x's own row order."""
    (x,) = _cast(dtype, x)
    sd = dict(zip(sd.keys(), _cast(dtype, *sd.values())))
    if batch_first:
        N, S, E = x.shape
    else:
        S, N, E = x.shape
    m = [None] * 4 if masks is None else list(masks)

    def drop(t, mk):
        return t if mk is None else t * _mask_scale(mk, p, t).view(t.shape)

    h0 = x.reshape(S * N, E)
    qkv = F.linear(h0, sd["self_attn.in_proj_weight"], sd["self_attn.in_proj_bias"])
    a, _ = mha(qkv, S, N, nhead, E // nhead, batch_first, m[0], p)
    a = drop(F.linear(a, sd["self_attn.out_proj.weight"], sd["self_attn.out_proj.bias"]), m[1])
    x1, _, _ = layernorm(h0, a, sd["norm1.weight"], sd["norm1.bias"])
    f = F.linear(x1, sd["linear1.weight"], sd["linear1.bias"])
    f = drop(F.relu(f) if act == "relu" else F.gelu(f), m[2])
    f = drop(F.linear(f, sd["linear2.weight"], sd["linear2.bias"]), m[3])
    x2, _, _ = layernorm(x1, f, sd["norm2.weight"], sd["norm2.bias"])
    return x2.view(x.shape)
