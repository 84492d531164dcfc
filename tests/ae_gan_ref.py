"""Torch restatement of the ae_gan residual autoencoders in EVALUATION mode (reference
experiments/v1_experiments/ae_gan/train.py `ResidualBlock`, `UpsampleBlock`, `ConvAutoencoder`, `ConvAutoencoderBIG`),
functional over a state dict, runnable in fp32 and fp64 on the CPU; and of the fused unit of csrc/resae.hip,
    y = act(conv(x, w) * scale + shift + res).
Also: `spread` / `sample_index` of the fixtures, the live-tap and the route predicate, each restated here independently of
weatherforecastingtoolkit_amd/ops.py; `key_list` and the recipe of tests/golden/g21_ae_gan.npz (`golden_state`).
"""
from __future__ import annotations

import hashlib

import torch
import torch.nn.functional as F

BIG = 4096          # tensors above this many elements are stored as a 2048-element sample + their L2 norm
NSAMPLE = 2048
BN_EPS = 1e-5
SEED = 1234
KINDS = {"conv": 0, "down": 1, "up": 2, "short": 3, "short_down": 4}

# (name, cin, cout) of the blocks; every encoder block has stride 2, every decoder block upsamples by 2
ENC_BIG = [(1, 64), (64, 128), (128, 256), (256, 512), (512, 1024), (1024, 2048), (2048, 2048)]
DEC_BIG = [(2048, 1024), (1024, 512), (512, 256), (256, 128), (128, 64), (64, 64), (64, 32)]
ENC_SMALL = [(1, 64), (64, 128), (128, 256), (256, 512), (512, 1024), (1024, 1024), (1024, 1024)]
DEC_SMALL = [(1024, 512), (512, 256), (256, 128), (128, 64), (64, 64), (64, 64), (64, 64)]


def spread(a32, a64):
    a32, a64 = a32.detach().double(), a64.detach().double()
    return float((a32 - a64).abs().max() / a64.abs().max().clamp_min(1e-300))


def bound(s):
    """the project's tolerance: max |a - a64| / max |a64| <= max(4 x spread, 2e-6)"""
    return max(4.0 * float(s), 2e-6)


def sample_index(numel):
    return torch.arange(NSAMPLE) * (numel // NSAMPLE)


def keys_digest(items):
    h = hashlib.sha256()
    for k, shape in items:
        h.update(f"{k} {tuple(int(s) for s in shape)}\n".encode())
    return h.hexdigest()


def values_digest(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(v.detach().to(torch.float32).contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------- geometry predicates
def out_plane(kind, h, w):
    if kind == 2:
        return 2 * h, 2 * w
    if kind in (1, 4):
        return (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1       # Conv2d(3, stride 2, padding 1); the 1x1 stride 2 agrees
    return h, w


def live_taps(kind, h, w):
    """by enumeration: tap (ky, kx) is live iff some output position reads a real input pixel through it -> 9-bit mask,
    bit ky * 3 + kx"""
    if kind in (3, 4):
        return 1 << 4
    ho, wo = out_plane(kind, h, w)

    def reads(o, k, size):
        if kind == 2:
            return 0 <= o + k - 1 < 2 * size
        return 0 <= (2 if kind == 1 else 1) * o + k - 1 < size
    mask = 0
    for ky in range(3):
        for kx in range(3):
            if any(reads(oy, ky, h) for oy in range(ho)) and any(reads(ox, kx, w) for ox in range(wo)):
                mask |= 1 << (ky * 3 + kx)
    return mask


def route(kind, n, cin, cout, h, w):
    ho, wo = out_plane(kind, h, w)
    return "small" if ho * wo <= 16 else "tile"


def layers(enc, dec, init_conv=False, n=1):
    """every resae_conv launch of a model on 128 x 128 frames: (kind, N, Cin, Cout, H, W)"""
    out, s = [], 128
    for cin, cout in enc:
        out += [(4, n, cin, cout, s, s), (1, n, cin, cout, s, s), (0, n, cout, cout, s // 2, s // 2)]
        s //= 2
    if init_conv:
        out += [(0, n, enc[-1][1], enc[-1][1], 1, 1)] * 2
    for cin, cout in dec:
        if cin != cout:
            out.append((3, n, cin, cout, s, s))
        out += [(2, n, cin, cout, s, s), (0, n, cout, cout, 2 * s, 2 * s)]
        s *= 2
    out.append((0, n, dec[-1][1], 1, s, s))
    return out


# ------------------------------------------------------------------------------------------------------- the fused unit
def gelu(x):
    return F.gelu(x)    # the exact (erf) form, nn.GELU()'s default


def unit(x, w, kind, scale=None, shift=None, res=None, res_up=False, act=False):
    """the unit in x's dtype, from the RAW weights"""
    if kind == 2:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    k = w.shape[-1]
    y = F.conv2d(x, w, None, stride=2 if kind in (1, 4) else 1, padding=k // 2)
    if scale is not None:
        y = y * scale.view(1, -1, 1, 1)
    if shift is not None:
        y = y + shift.view(1, -1, 1, 1)
    if res is not None:
        y = y + (F.interpolate(res, scale_factor=2, mode="nearest") if res_up else res)
    return gelu(y) if act else y


def unit_inputs(kind, n, cin, cout, h, w, seed, res_up=False):
    """seeded fp32 CPU inputs of one unit: x, w, scale, shift, res"""
    g = torch.Generator().manual_seed(seed)
    k = 1 if kind >= 3 else 3
    ho, wo = out_plane(kind, h, w)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    scale = 0.75 + 0.5 * torch.rand(cout, generator=g)
    shift = 0.2 * torch.randn(cout, generator=g)
    res = torch.randn((n, cout, ho // 2, wo // 2) if res_up else (n, cout, ho, wo), generator=g)
    return x, wt, scale, shift, res


# ------------------------------------------------------------------------------------------- blocks and models (eval)
def _k(p, name):
    return f"{p}.{name}" if p else name


def bn_eval(sd, p, x):
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, BN_EPS)


def residual_block(sd, p, x, stride):
    """reference ResidualBlock.forward in evaluation mode; p: the block's key prefix ("" for a bare block)"""
    short = x
    if _k(p, "shortcut.0.weight") in sd:
        short = bn_eval(sd, _k(p, "shortcut.1"), F.conv2d(x, sd[_k(p, "shortcut.0.weight")], None, stride=stride))
    out = gelu(bn_eval(sd, _k(p, "bn1"), F.conv2d(x, sd[_k(p, "conv1.weight")], None, stride=stride, padding=1)))
    out = bn_eval(sd, _k(p, "bn2"), F.conv2d(out, sd[_k(p, "conv2.weight")], None, stride=1, padding=1))
    return gelu(out + short)


def upsample_block(sd, p, x):
    return residual_block(sd, _k(p, "resblock"), F.interpolate(x, scale_factor=2, mode="nearest"), 1)


def encode(sd, x, stages=None):
    for i in range(1, 8):
        x = residual_block(sd, f"enc{i}", x, 2)
        if stages is not None:
            stages[f"enc{i}"] = x
    return F.linear(x.flatten(1), sd["fc_enc.weight"], sd["fc_enc.bias"])


def decode(sd, z, stages=None):
    x = F.linear(z, sd["fc_dec.weight"], sd["fc_dec.bias"])[:, :, None, None]
    if "dec_init_conv.conv1.weight" in sd:
        x = residual_block(sd, "dec_init_conv", x, 1)
    for i in range(1, 8):
        x = upsample_block(sd, f"dec{i}", x)
        if stages is not None:
            stages[f"dec{i}"] = x
    return F.conv2d(x, sd["final_conv.weight"], sd["final_conv.bias"], padding=1)


def forward(sd, x, stages=None):
    z = encode(sd, x, stages)
    return decode(sd, z, stages), z


def cast(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def block_state(prefix, cin, cout, stride, g):
    """seeded fp32 state of one ResidualBlock under `prefix`: weights, random affine and running statistics"""
    sd = {}

    def bn(p):
        sd[p + ".weight"] = 0.75 + 0.5 * torch.rand(cout, generator=g)
        sd[p + ".bias"] = 0.1 * torch.randn(cout, generator=g)
        sd[p + ".running_mean"] = 0.2 * torch.randn(cout, generator=g)
        sd[p + ".running_var"] = 0.5 + torch.rand(cout, generator=g)
        sd[p + ".num_batches_tracked"] = torch.tensor(3)
    sd[prefix + "conv1.weight"] = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
    bn(prefix + "bn1")
    sd[prefix + "conv2.weight"] = torch.randn(cout, cout, 3, 3, generator=g) / (9 * cout) ** 0.5
    bn(prefix + "bn2")
    if stride != 1 or cin != cout:
        sd[prefix + "shortcut.0.weight"] = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
        bn(prefix + "shortcut.1")
    return sd


# ---------------------------------------------------------------------------------------------------- keys and recipe
def key_list(big=True, in_ch=1, latent_dim=None):
    """[(key, shape)] of the reference module's state_dict, in its order"""
    enc, dec = (ENC_BIG, DEC_BIG) if big else (ENC_SMALL, DEC_SMALL)
    latent_dim = (2048 if big else 1024) if latent_dim is None else latent_dim
    out = []

    def bn(p, c):
        out.extend([(p + ".weight", (c,)), (p + ".bias", (c,)), (p + ".running_mean", (c,)), (p + ".running_var", (c,)),
                    (p + ".num_batches_tracked", ())])

    def block(p, cin, cout, stride):
        out.append((p + ".conv1.weight", (cout, cin, 3, 3)))
        bn(p + ".bn1", cout)
        out.append((p + ".conv2.weight", (cout, cout, 3, 3)))
        bn(p + ".bn2", cout)
        if stride != 1 or cin != cout:
            out.append((p + ".shortcut.0.weight", (cout, cin, 1, 1)))
            bn(p + ".shortcut.1", cout)
    for i, (cin, cout) in enumerate(enc):
        block(f"enc{i + 1}", in_ch if i == 0 else cin, cout, 2)
    top = enc[-1][1]
    out += [("fc_enc.weight", (latent_dim, top)), ("fc_enc.bias", (latent_dim,)),
            ("fc_dec.weight", (top, latent_dim)), ("fc_dec.bias", (top,))]
    if not big:
        block("dec_init_conv", top, top, 1)
    for i, (cin, cout) in enumerate(dec):
        block(f"dec{i + 1}.resblock", cin, cout, 1)
    out += [("final_conv.weight", (in_ch, dec[-1][1], 3, 3)), ("final_conv.bias", (in_ch,))]
    return out


def bn_prefixes(keys):
    return [k[:-len(".running_mean")] for k in keys if k.endswith(".running_mean")]


def golden_input():
    return torch.rand(2, 1, 128, 128, generator=torch.Generator().manual_seed(SEED + 1))


def golden_state(model, g):
    """G21's recipe on a freshly seeded ConvAutoencoderBIG-shaped module `model` (any class with the reference's keys):
    the seeded weights stay, the BatchNorm affine and running statistics come from the fixture `g` -> state dict"""
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    off = 0
    for p in bn_prefixes(list(sd)):
        c = sd[p + ".weight"].numel()
        for name in ("weight", "bias", "running_mean", "running_var"):
            sd[f"{p}.{name}"] = torch.from_numpy(g["bn_" + name][off:off + c].copy())
        off += c
    assert off == g["bn_weight"].shape[0]
    return sd
