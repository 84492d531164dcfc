"""Torch restatement (functional, any dtype / device) of the conv latent autoencoder of the reference's
experiments/v1_experiments/pretrained_ae_convae_sevir/train.py:58-143 (`ConvEncoder`, `ConvDecoder`, `ConvModel`) and
its Huber loss (:155), on a state dict with the reference's keys.  Used against tests/golden/g13_convae.npz on the CPU
and as the fp64 yardstick of the GPU tests at sizes the fixture does not hold."""
import hashlib

import torch
import torch.nn.functional as F

SLOPE = 0.01
BIG = 4096          # tensors above this many elements are stored as a 2048-element sample + their L2 norm
NSAMPLE = 2048
UNITS = [("encoder.conv0", 0), ("encoder.down1", 1), ("encoder.down2", 1), ("encoder.down3", 1),
         ("decoder.up1", 2), ("decoder.up2", 2), ("decoder.up3", 2)]


def key_list(in_channels=4, size=48, latent_dim=512, c=8):
    """[(key, shape)] of the reference module's state_dict, in its order"""
    s = [size, size // 2, size // 4, size // 8]
    out = []

    def unit(name, wshape, plane):
        out.extend([(f"{name}.0.weight", wshape), (f"{name}.0.bias", (c,)),
                    (f"{name}.1.weight", (c, plane, plane)), (f"{name}.1.bias", (c, plane, plane))])

    unit("encoder.conv0", (c, in_channels, 3, 3), s[0])
    for i in (1, 2, 3):
        unit(f"encoder.down{i}", (c, c, 4, 4), s[i])
    for i in (1, 2, 3):
        unit(f"decoder.up{i}", (c, c, 4, 4), s[3 - i])
    flat = c * s[3] * s[3]
    out += [("decoder.conv_out.weight", (in_channels, c, 3, 3)), ("decoder.conv_out.bias", (in_channels,)),
            ("to_latent.weight", (latent_dim, flat)), ("to_latent.bias", (latent_dim,)),
            ("to_reconstruction.weight", (flat, latent_dim)), ("to_reconstruction.bias", (flat,))]
    return out


def conv(x, w, b, kind):
    if kind == 0:
        return F.conv2d(x, w, b, padding=1)
    if kind == 1:
        return F.conv2d(x, w, b, stride=2, padding=1)
    return F.conv_transpose2d(x, w, b, stride=2, padding=1)


def unit(x, w, b, gamma, beta, kind, slope=SLOPE, pre=None):
    """LeakyReLU_slope(LayerNorm([C, H, W])(conv(x) + b)); the pre-activation is appended to `pre`"""
    u = conv(x, w, b, kind)
    a = F.layer_norm(u, tuple(gamma.shape), gamma, beta, 1e-5)
    if pre is not None:
        pre.append(a)
    return F.leaky_relu(a, slope)


def forward(sd, x, pre=None):
    """x (B, T, C, H, W) -> (z (B*T, latent), reconstruction (B, T, C, H, W))"""
    b, t, c, h, w = x.shape
    y = x.reshape(b * t, c, h, w)
    for name, kind in UNITS[:4]:
        y = unit(y, sd[f"{name}.0.weight"], sd[f"{name}.0.bias"], sd[f"{name}.1.weight"], sd[f"{name}.1.bias"], kind,
                 pre=pre)
    shape = y.shape
    z = F.linear(y.reshape(b * t, -1), sd["to_latent.weight"], sd["to_latent.bias"])
    y = F.linear(z, sd["to_reconstruction.weight"], sd["to_reconstruction.bias"]).reshape(shape)
    for name, kind in UNITS[4:]:
        y = unit(y, sd[f"{name}.0.weight"], sd[f"{name}.0.bias"], sd[f"{name}.1.weight"], sd[f"{name}.1.bias"], kind,
                 pre=pre)
    y = F.conv2d(y, sd["decoder.conv_out.weight"], sd["decoder.conv_out.bias"], padding=1)
    return z, y.reshape(b, t, c, h, w)


def loss_of(sd, x, pre=None, delta=1.0):
    z, rec = forward(sd, x, pre)
    return F.huber_loss(rec, x, delta=delta), z, rec


def run(sd, x, dtype):
    """one forward + backward in `dtype` on detached copies -> (loss, z, rec, {key: grad}, pre-activations)"""
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    pre = []
    loss, z, rec = loss_of(p, x.to(dtype), pre)
    loss.backward()
    return loss.detach(), z.detach(), rec.detach(), {k: v.grad for k, v in p.items()}, [a.detach() for a in pre]


def kink_margin(pre64, pre32):
    """(min |a| of the fp64 pre-activations, largest fp32-vs-fp64 absolute difference of them)"""
    return (min(float(a.abs().min()) for a in pre64),
            max(float((a.double() - b.double()).abs().max()) for a, b in zip(pre64, pre32)))


def spread(a32, a64):
    a32, a64 = a32.detach().double(), a64.detach().double()
    return float((a32 - a64).abs().max() / a64.abs().max().clamp_min(1e-300))


def sample_index(numel):
    return torch.arange(NSAMPLE) * (numel // NSAMPLE)


def keys_digest(items):
    """sha256 of the ordered (key, shape) list"""
    h = hashlib.sha256()
    for k, shape in items:
        h.update(f"{k} {tuple(int(s) for s in shape)}\n".encode())
    return h.hexdigest()


def values_digest(sd):
    """sha256 of the fp32 bytes of every tensor, in key order"""
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(v.detach().to(torch.float32).contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def unit_inputs(kind, n, cin, cout, h, w, seed):
    """seeded fp32 CPU inputs of one fused unit: x, w, b, gamma, beta (random, not ones / zeros) and dy"""
    g = torch.Generator().manual_seed(seed)
    k = 3 if kind == 0 else 4
    ho, wo = (h, w) if kind == 0 else (h // 2, w // 2) if kind == 1 else (2 * h, 2 * w)
    fan = cin * k * k // (4 if kind == 2 else 1)
    wshape = (cin, cout, k, k) if kind == 2 else (cout, cin, k, k)
    return {"x": torch.randn(n, cin, h, w, generator=g),
            "w": torch.randn(*wshape, generator=g) / fan ** 0.5,
            "b": 0.5 * torch.randn(cout, generator=g),
            "gamma": 1.0 + 0.5 * torch.randn(cout, ho, wo, generator=g),
            "beta": 0.5 * torch.randn(cout, ho, wo, generator=g),
            "dy": torch.randn(n, cout, ho, wo, generator=g)}


def unit_oracle(inp, kind, slope, dtype):
    """-> {y, a, dx, dw, db, dgamma, dbeta} of one unit in `dtype`, for the output gradient inp['dy']"""
    t = {k: v.detach().to(dtype).clone().requires_grad_(k != "dy") for k, v in inp.items()}
    pre = []
    y = unit(t["x"], t["w"], t["b"], t["gamma"], t["beta"], kind, slope, pre)
    y.backward(t["dy"])
    return {"y": y.detach(), "a": pre[0].detach(), "dx": t["x"].grad, "dw": t["w"].grad, "db": t["b"].grad,
            "dgamma": t["gamma"].grad, "dbeta": t["beta"].grad}
