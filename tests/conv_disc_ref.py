"""Torch restatement (functional, any dtype / device) of the conv + GAN latent model of the reference's
experiments/v1_experiments/pretrained_ae_conv_disc/train.py: `Encoder`, `Decoder`, `ConvModel` (:140-206), the arithmetic of
`Loss.forward` (:52-100) with the PatchGAN of pipeline/models/autoencoderkl/losses/model.py in training mode, and one
conv + SiLU unit, on state dicts with the reference's keys.  Used against tests/golden/g17_conv_disc.npz on the CPU and
as the fp64 yardstick of the GPU tests at sizes the fixture does not hold."""
import torch
import torch.nn.functional as F

from tests.convae_ref import BIG, NSAMPLE, keys_digest, sample_index, spread, values_digest  # noqa: F401

ENC = [(64, 128), (128, 256), (256, 512), (512, 1024)]         # encoder.conv.{0,2,4,6}: Conv2d(cin -> cout)
DEC = [(1024, 1024), (1024, 512), (512, 256), (256, 128)]      # decoder.deconv.{0,2,4,6}: ConvTranspose2d(cin -> cout)
DISC_BN = (3, 6, 9)                                            # main.{3,6,9}: the BatchNorm layers of NLayerDiscriminator(64)


def key_list(latent_dim=512):
    """[(key, shape)] of the reference ConvModel's state_dict, in its order"""
    out = []
    for i, (cin, cout) in enumerate(ENC):
        out += [(f"encoder.conv.{2 * i}.weight", (cout, cin, 3, 3)), (f"encoder.conv.{2 * i}.bias", (cout,))]
    out += [("encoder.conv_out.weight", (1024, 1024, 1, 1)), ("encoder.conv_out.bias", (1024,)),
            ("encoder.fc.weight", (latent_dim, 1024)), ("encoder.fc.bias", (latent_dim,)),
            ("decoder.fc.weight", (1024, latent_dim)), ("decoder.fc.bias", (1024,))]
    for i, (cin, cout) in enumerate(DEC):
        out += [(f"decoder.deconv.{2 * i}.weight", (cin, cout, 3, 3)), (f"decoder.deconv.{2 * i}.bias", (cout,))]
    out += [("decoder.conv_out.weight", (64, 128, 1, 1)), ("decoder.conv_out.bias", (64,))]
    return out


def forward(sd, x):
    """x (B, 64, 16, 16) -> (z (B, latent), recon (B, 64, 16, 16))"""
    y = x
    for i in (0, 2, 4, 6):
        y = F.silu(F.conv2d(y, sd[f"encoder.conv.{i}.weight"], sd[f"encoder.conv.{i}.bias"], stride=2, padding=1))
    y = F.conv2d(y, sd["encoder.conv_out.weight"], sd["encoder.conv_out.bias"])
    z = F.linear(y.view(y.size(0), -1), sd["encoder.fc.weight"], sd["encoder.fc.bias"])
    y = F.linear(z, sd["decoder.fc.weight"], sd["decoder.fc.bias"]).view(-1, 1024, 1, 1)
    for i in (0, 2, 4, 6):
        y = F.silu(F.conv_transpose2d(y, sd[f"decoder.deconv.{i}.weight"], sd[f"decoder.deconv.{i}.bias"], stride=2,
                                      padding=1, output_padding=1))
    return z, F.conv2d(y, sd["decoder.conv_out.weight"], sd["decoder.conv_out.bias"])


def nll_of(recon, x, logvar=0.0):
    """reference :54,62-63: mean |recon - x| / exp(logvar) + logvar, summed (a scalar) and divided by the batch size"""
    rec = F.l1_loss(recon, x)
    lv = torch.as_tensor(logvar, dtype=recon.dtype, device=recon.device)
    return (rec / torch.exp(lv) + lv) / x.size(0), rec


def disc(dsd, x, pre=None):
    """NLayerDiscriminator(input_nc=64, n_layers=3) in training mode (batch statistics); LeakyReLU inputs go to `pre`"""
    def leaky(h):
        if pre is not None:
            pre.append(h)
        return F.leaky_relu(h, 0.2)
    h = leaky(F.conv2d(x, dsd["main.0.weight"], dsd["main.0.bias"], stride=2, padding=1))
    for i, s in ((2, 2), (5, 2), (8, 1)):
        h = F.conv2d(h, dsd[f"main.{i}.weight"], None, stride=s, padding=1)
        h = leaky(F.batch_norm(h, None, None, dsd[f"main.{i + 1}.weight"], dsd[f"main.{i + 1}.bias"], True, 0.1, 1e-5))
    return F.conv2d(h, dsd["main.11.weight"], dsd["main.11.bias"], padding=1)


def disc_params(dsd, dtype):
    return {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in dsd.items()
            if v.is_floating_point() and "running" not in k}


def run(sd, x, dtype, logvar=0.0):
    """one forward + backward of the pre-disc_start loss in `dtype` on detached copies
    -> (loss, z, recon, {key: grad})"""
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    x = x.to(dtype)
    z, recon = forward(p, x)
    loss, _ = nll_of(recon, x, logvar)
    loss.backward()
    return loss.detach(), z.detach(), recon.detach(), {k: v.grad for k, v in p.items()}


def l1_margin(recon64, recon32, x):
    """(min |recon - x| of the fp64 run, largest fp32-vs-fp64 absolute difference of recon): the L1 derivative jumps at 0"""
    return (float((recon64.double() - x.double()).abs().min()),
            float((recon64.double() - recon32.double()).abs().max()))


def gan(sd, dsd, x, dtype, logvar=0.0, disc_weight=1.0):
    """the step from disc_start on (reference :74-100), in `dtype`
    -> dict: g_loss, d_weight, loss (generator), nll, g_grads {key: grad of the generator loss}, d_loss, d_grads, and the
    LeakyReLU / hinge inputs of the three discriminator passes (`pre_g`, `pre_d`, `logits_real`, `logits_fake`)"""
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    dp = disc_params(dsd, dtype)
    x = x.to(dtype)
    _, recon = forward(p, x)
    nll, _ = nll_of(recon, x, logvar)
    pre_g = []
    g_loss = -disc(dp, recon, pre_g).mean()
    last = p["decoder.conv_out.weight"]
    ng = torch.autograd.grad(nll, last, retain_graph=True)[0]
    gg = torch.autograd.grad(g_loss, last, retain_graph=True)[0]
    d_weight = torch.clamp(disc_weight * ng.norm() / (gg.norm() + 1e-4), 0.0, 1e4).detach()
    loss = nll + d_weight * g_loss
    g_grads = dict(zip(p, torch.autograd.grad(loss, list(p.values()))))
    pre_d = []
    real, fake = disc(dp, x, pre_d), disc(dp, recon.detach(), pre_d)
    d_loss = 0.5 * (F.relu(1.0 - real).mean() + F.relu(1.0 + fake).mean())
    d_grads = dict(zip(dp, torch.autograd.grad(d_loss, list(dp.values()))))
    return {"g_loss": g_loss.detach(), "d_weight": d_weight, "loss": loss.detach(), "nll": nll.detach(), "g_grads": g_grads,
            "d_loss": d_loss.detach(), "d_grads": d_grads, "pre_g": [a.detach() for a in pre_g],
            "pre_d": [a.detach() for a in pre_d], "logits_real": real.detach(), "logits_fake": fake.detach()}


def grad_norm(grads):
    return float(torch.sqrt(sum(g.double().pow(2).sum() for g in grads.values())))


# ---- one conv + SiLU unit.  w is (Clo, Chi, 3, 3) for both module types
def unit_shapes(n, chi, clo, hhi, whi, transposed):
    hlo, wlo = (hhi - 1) // 2 + 1, (whi - 1) // 2 + 1
    hi, lo = (n, chi, hhi, whi), (n, clo, hlo, wlo)
    return (lo, hi) if transposed else (hi, lo)      # (input, output)


def unit_inputs(n, chi, clo, hhi, whi, transposed, seed):
    """seeded fp32 CPU inputs of one unit: x, w, b and the output gradient dy"""
    g = torch.Generator().manual_seed(seed)
    xin, yout = unit_shapes(n, chi, clo, hhi, whi, transposed)
    fan = (clo if transposed else chi) * 9
    return {"x": torch.randn(*xin, generator=g), "w": torch.randn(clo, chi, 3, 3, generator=g) / fan ** 0.5,
            "b": 0.5 * torch.randn(yout[1], generator=g), "dy": torch.randn(*yout, generator=g)}


def unit(x, w, b, transposed, act, out_hw=None):
    if transposed:
        op = (out_hw[0] - (2 * x.shape[2] - 1), out_hw[1] - (2 * x.shape[3] - 1))
        t = F.conv_transpose2d(x, w, b, stride=2, padding=1, output_padding=op)
    else:
        t = F.conv2d(x, w, b, stride=2, padding=1)
    return F.silu(t) if act else t


def unit_oracle(inp, transposed, act, dtype, w=None):
    """-> {y, dx, dw, db} of one unit in `dtype` for the output gradient inp['dy'] (w: another weight tensor to use)"""
    t = {k: v.detach().to(dtype).clone().requires_grad_(k != "dy") for k, v in inp.items()}
    if w is not None:
        t["w"] = w.detach().to(dtype).clone().requires_grad_(True)
    y = unit(t["x"], t["w"], t["b"], transposed, act, tuple(inp["dy"].shape[2:]))
    y.backward(t["dy"])
    return {"y": y.detach(), "dx": t["x"].grad, "dw": t["w"].grad, "db": t["b"].grad}
