"""GPU: training the AutoencoderKL (csrc/aekl_bwd.hip, `AutoencoderKL.unfreeze()`): the 3x3 weight and data gradients in
their three kinds, GroupNorm / softmax / attention / posterior backward against torch autograd on the CPU; the whole model
against the reference's recorded fp64 gradients (tests/golden/g20_aekl_train.npz); repeatability, a second backward, the
launch budget.

Tolerances: the rule of tests/test_aekl_gpu.py.  Every comparison is against fp64 in the measure max|a - b| / max|b|; the
bound is max(4 x spread, 2e-6), spread = the same measure between torch fp32 and torch fp64 on the CPU, measured in the
test or read from the fixture."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import aekl_ref as A
from tests import aekl_train_ref as T
from tests import convae_ref as R
from tests.test_aekl_gpu import (CONV3_CASES, CONV3_IDS, conv3_inputs, conv3_oracle, medium, rel, rnd, tol,  # noqa: F401
                                 x_for_bf16_safe_prologue)
from weatherforecastingtoolkit_amd import functional as Fn
from weatherforecastingtoolkit_amd import ops
from weatherforecastingtoolkit_amd._lib import WfaeError
from weatherforecastingtoolkit_amd.pipeline.models.autoencoderkl import AutoencoderKL
from weatherforecastingtoolkit_amd.pipeline.models.autoencoderkl.attention import AttentionBlock

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G20 = os.path.join(HERE, "golden", "g20_aekl_train.npz")

# one more case per kind whose output pixels span at least three reduction slabs of the weight gradient (a slab is 8 tiles
# of 8 x 16 output pixels, 4 x 16 for kind 1): 25 tiles, 18 tiles, 25 tiles
SLAB_CASES = [(0, 2, 32, 32, 40, 72), (1, 1, 32, 32, 48, 80), (2, 1, 32, 32, 20, 36)]
BWD_CASES = CONV3_CASES + SLAB_CASES
BWD_IDS = CONV3_IDS + ["slabs-k%d-n%d-%dto%d-%dx%d" % c for c in SLAB_CASES]


def check(name, got, w64, w32):
    bound, err = tol(R.spread(w32, w64)), rel(got, w64)
    print(f"{name}: err {err:.3e} tol {bound:.3e}")
    assert got.shape == w64.shape, name
    assert err <= bound, name


# ------------------------------------------------------------------------------------------------ the 3x3 gradients
def conv3_grad_oracle(t, kind, pro, dtype, a=None):
    """fp autograd of conv3_oracle on the operand a = silu(u), u = x * scale + shift (`pro`) or a = u = x:
    -> du, dw, dbias under dy = t["dy"]; `a`: the operand given outright (du is then the gradient of a)"""
    w, b = t["w"].to(dtype).requires_grad_(True), t["b"].to(dtype).requires_grad_(True)
    if a is not None:
        u = a.to(dtype).requires_grad_(True)
        act = u
    else:
        u = t["x"].to(dtype)
        if pro:
            u = u * t["scale"].to(dtype)[:, :, None, None] + t["shift"].to(dtype)[:, :, None, None]
        u = u.detach().requires_grad_(True)
        act = F.silu(u) if pro else u
    y = conv3_oracle(act, w, b, None, None, None, kind, 1.0, dtype)
    return torch.autograd.grad(y, (u, w, b), t["dy"].to(dtype))


def bwd_inputs(case, seed=7):
    t = conv3_inputs(*case, seed)
    t["dy"] = rnd(t["res"].shape, seed + 6)
    return t


@functools.lru_cache(maxsize=None)
def bwd_reference(case, pro):
    """computed once per (case, variant), shared by the weight- and the data-gradient test"""
    t = bwd_inputs(case)
    return t, conv3_grad_oracle(t, case[0], pro, torch.float64), conv3_grad_oracle(t, case[0], pro, torch.float32)


@pytest.mark.parametrize("variant", ["plain", "pro"])
@pytest.mark.parametrize("case", BWD_CASES, ids=BWD_IDS)
def test_conv3_weight_gradient_against_fp64(dev, case, variant):
    pro = variant == "pro"
    t, o64, o32 = bwd_reference(case, pro)
    d = {k: v.to(dev) for k, v in t.items()}
    dw, db = torch.empty_like(d["w"]), torch.empty_like(d["b"])
    ops.aekl_conv3_bwd_weight(d["dy"], d["x"], dw, db, (d["scale"], d["shift"]) if pro else None, case[0])
    check("dw", dw, o64[1], o32[1])
    check("dbias", db, o64[2], o32[2])


@pytest.mark.parametrize("variant", ["plain", "pro"])
@pytest.mark.parametrize("case", BWD_CASES, ids=BWD_IDS)
def test_conv3_data_gradient_against_fp64(dev, case, variant):
    pro = variant == "pro"
    t, o64, o32 = bwd_reference(case, pro)
    d = {k: v.to(dev) for k, v in t.items()}
    packed_t = ops.aekl_conv3_pack(d["w"].flip(2, 3).transpose(0, 1).contiguous())
    du = ops.aekl_conv3_bwd_data(d["dy"], packed_t, d["x"], (d["scale"], d["shift"]) if pro else None, case[0])
    check("du", du, o64[0], o32[0])


@pytest.mark.parametrize("case", [(0, 1, 128, 128, 48, 48), (1, 1, 64, 128, 14, 22), (2, 2, 256, 256, 6, 10)],
                         ids=lambda c: "k%d-n%d-%dto%d-%dx%d" % c)
def test_conv3_data_gradient_fp32_mfma_variant(dev, case):
    """mode 4 of the data gradient (the forward's comparison form); the weight gradient refuses it"""
    t, o64, o32 = bwd_reference(case, True)
    d = {k: v.to(dev) for k, v in t.items()}
    mode = ops.AEKL_MODES["fp32"]
    packed_t = ops.aekl_conv3_pack(d["w"].flip(2, 3).transpose(0, 1).contiguous(), mode)
    du = ops.aekl_conv3_bwd_data(d["dy"], packed_t, d["x"], (d["scale"], d["shift"]), case[0], mode)
    check("du", du, o64[0], o32[0])
    with pytest.raises(WfaeError, match="mode 4"):
        ops.aekl_conv3_bwd_weight(d["dy"], d["x"], torch.empty_like(d["w"]), None, None, case[0], mode)


@pytest.mark.parametrize("case", [(0, 1, 128, 128, 48, 48), (1, 1, 64, 128, 14, 22), (2, 2, 256, 256, 6, 10)],
                         ids=lambda c: "k%d-n%d-%dto%d-%dx%d" % c)
def test_conv3_gradients_medium_round_the_operand_after_the_prologue(dev, medium, case):
    """'medium' (mode 1): the weight gradient's operands are bf16(silu(x * scale + shift)) — rounded after the prologue —
    and bf16(dy); the data gradient's are bf16(dy) and the bf16-rounded weights.  Oracle: fp autograd on those rounded
    operands, to fp32 accumulation error.  An oracle that leaves the prologue's result unrounded misses the same bound."""
    assert ops.aekl_mode() == ops.AEKL_MODES["bf16"]
    kind = case[0]
    t = bwd_inputs(case)
    t["x"] = x_for_bf16_safe_prologue(t)       # also leaves t["a"]: the bf16 values the prologue rounds to
    d = {k: v.to(dev) for k, v in t.items()}
    gn = (d["scale"], d["shift"])
    dw = torch.empty_like(d["w"])
    ops.aekl_conv3_bwd_weight(d["dy"], d["x"], dw, None, gn, kind)
    du = ops.aekl_conv3_bwd_data(d["dy"], ops.aekl_conv3_pack(d["w"].flip(2, 3).transpose(0, 1).contiguous()), d["x"], gn, kind)
    r = dict(t, dy=t["dy"].bfloat16().float(), w=t["w"].bfloat16().float())
    o64, o32 = conv3_grad_oracle(r, kind, True, torch.float64, a=t["a"]), conv3_grad_oracle(r, kind, True, torch.float32, a=t["a"])
    bound, err = tol(R.spread(o32[1], o64[1])), rel(dw, o64[1])
    unrounded = rel(conv3_grad_oracle(r, kind, True, torch.float64)[1], o64[1])
    print(f"dw err {err:.3e} tol {bound:.3e}; unrounded prologue {unrounded:.3e}")
    assert unrounded > 10 * bound
    assert err <= bound
    # the data gradient: conv of the rounded dy and weights (the gradient of the operand a), times silu'(u) in fp32
    u = t["x"].double() * t["scale"].double()[:, :, None, None] + t["shift"].double()[:, :, None, None]
    s = torch.sigmoid(u)
    f64 = s * (1 + u * (1 - s))
    check("du", du, o64[0] * f64, o32[0] * f64.float())
    exact = conv3_grad_oracle(dict(t), kind, True, torch.float64)[0]
    assert rel(du, exact) > 10 * tol(R.spread(o32[0] * f64.float(), o64[0] * f64))


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_conv3_gradients_at_the_padded_rim(dev, kind):
    """silu(gn(0)) != 0: with a shift of 3 a padding tap that went through the prologue would add silu(3) = 2.86 times the
    sum of dy along the rim to the weight gradient.  dW, and the rim of du on its own, against fp64."""
    case = (kind, 2, 64, 64, 10, 14)
    t = bwd_inputs(case, 21)
    t["shift"] = torch.full_like(t["shift"], 3.0)
    d = {k: v.to(dev) for k, v in t.items()}
    gn = (d["scale"], d["shift"])
    dw = torch.empty_like(d["w"])
    ops.aekl_conv3_bwd_weight(d["dy"], d["x"], dw, None, gn, kind)
    du = ops.aekl_conv3_bwd_data(d["dy"], ops.aekl_conv3_pack(d["w"].flip(2, 3).transpose(0, 1).contiguous()), d["x"], gn, kind)
    o64, o32 = conv3_grad_oracle(t, kind, True, torch.float64), conv3_grad_oracle(t, kind, True, torch.float32)
    check("dw", dw, o64[1], o32[1])

    def border(a):
        return torch.cat([a[:, :, 0].flatten(), a[:, :, -1].flatten(), a[:, :, :, 0].flatten(), a[:, :, :, -1].flatten()])
    check("du rim", border(du), border(o64[0]), border(o32[0]))
    if kind == 0:      # the trap itself: padding before the prologue gives another weight gradient
        xp = F.silu(F.pad(t["x"].double(), (1, 1, 1, 1)) * t["scale"].double()[:, :, None, None] + 3.0)
        w = t["w"].double().requires_grad_(True)
        wrong, = torch.autograd.grad(F.conv2d(xp, w), w, t["dy"].double())
        assert rel(wrong, o64[1]) > 100 * tol(R.spread(o32[1], o64[1]))


def test_conv3_gradients_are_bitwise_repeatable_and_refuse(dev):
    case = (0, 2, 32, 64, 40, 72)
    t = bwd_inputs(case)
    d = {k: v.to(dev) for k, v in t.items()}
    gn = (d["scale"], d["shift"])
    a, b = torch.empty_like(d["w"]), torch.empty_like(d["w"])
    ops.aekl_conv3_bwd_weight(d["dy"], d["x"], a, None, gn, 0)
    ops.aekl_conv3_bwd_weight(d["dy"], d["x"], b, None, gn, 0)
    pt = ops.aekl_conv3_pack(d["w"].flip(2, 3).transpose(0, 1).contiguous())
    u, v = ops.aekl_conv3_bwd_data(d["dy"], pt, d["x"], gn, 0), ops.aekl_conv3_bwd_data(d["dy"], pt, d["x"], gn, 0)
    assert torch.equal(a, b) and torch.equal(u, v)
    with pytest.raises(WfaeError, match="kind"):
        ops.aekl_conv3_bwd_weight(d["dy"], d["x"], a, None, gn, 3)
    with pytest.raises(WfaeError, match="does not belong"):
        ops.aekl_conv3_bwd_data(d["dy"][:, :, :8], pt, d["x"], gn, 0)
    with pytest.raises(WfaeError, match="packed weights"):
        ops.aekl_conv3_bwd_data(d["dy"], ops.aekl_conv3_pack(d["w"]), d["x"][:, :16].contiguous(), None, 0)


# ------------------------------------------------------------------------------------------------ GroupNorm backward
@pytest.mark.parametrize("n,c,h,w,groups", [(2, 64, 16, 16, 8), (1, 128, 48, 48, 32), (3, 32, 6, 10, 32), (1, 512, 24, 24, 32),
                                            (1, 128, 128, 128, 8)])
@pytest.mark.parametrize("offset", [0.0, 100.0])
def test_group_norm_backward(dev, n, c, h, w, groups, offset):
    g = torch.Generator().manual_seed(c + h)
    x = torch.randn(n, c, h, w, generator=g) + offset
    du, skip = torch.randn(n, c, h, w, generator=g), torch.randn(n, c, h, w, generator=g)
    gamma, beta = rnd((c,), 1, 0.5, 1.5), rnd((c,), 2)

    def oracle(dtype):
        xx, gm, bt = (v.to(dtype).requires_grad_(True) for v in (x, gamma, beta))
        dx, dg, db = torch.autograd.grad(F.group_norm(xx, groups, gm, bt, 1e-6), (xx, gm, bt), du.to(dtype))
        return dx + skip.to(dtype), dg, db
    o64, o32 = oracle(torch.float64), oracle(torch.float32)
    xd, gd = x.to(dev), gamma.to(dev)
    mean, rstd = ops.aekl_gn_stats(xd, gd, beta.to(dev), groups)[:2]
    got = ops.aekl_gn_bwd(du.to(dev), xd, gd, mean, rstd, skip.to(dev))
    for name, a, b64, b32 in zip(("dx", "dgamma", "dbeta"), got, o64, o32):
        check(name, a, b64, b32)
    again = ops.aekl_gn_bwd(du.to(dev), xd, gd, mean, rstd, skip.to(dev))
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    plain = ops.aekl_gn_bwd(du.to(dev), xd, gd, mean, rstd)[0]
    check("dx without skip", plain, o64[0] - skip.double(), o32[0] - skip)


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("rows,cols", [(256, 256), (7, 33)])
def test_row_softmax_backward(dev, rows, cols):
    x, dp = rnd((rows, cols), rows, -30, 30), rnd((rows, cols), rows + 1)

    def oracle(dtype):
        xx = x.to(dtype).requires_grad_(True)
        p = torch.softmax(xx * 0.37, -1)
        return torch.autograd.grad(p, xx, dp.to(dtype))[0]
    p = ops.aekl_softmax(x.to(dev), 0.37)
    check("ds", ops.aekl_softmax_bwd(p, dp.to(dev), 0.37), oracle(torch.float64), oracle(torch.float32))


@pytest.mark.parametrize("n,c,h,w,groups", [(2, 64, 16, 16, 8), (1, 512, 16, 16, 32)], ids=["S256-C64", "S256-C512"])
def test_attention_block_backward(dev, n, c, h, w, groups):
    g = torch.Generator().manual_seed(c + h)
    p = "a"
    sd = {f"{p}.group_norm.weight": rnd((c,), 1, 0.5, 1.5), f"{p}.group_norm.bias": rnd((c,), 2)}
    for i, nm in enumerate(("query", "key", "value", "proj_attn")):
        sd[f"{p}.{nm}.weight"] = torch.randn(c, c, generator=g) * c ** -0.5 * (2.0 if i < 2 else 1.0)
        sd[f"{p}.{nm}.bias"] = rnd((c,), 10 + i)
    x, dy = torch.randn(n, c, h, w, generator=g), torch.randn(n, c, h, w, generator=g)

    def oracle(dtype):
        leaves = {k: v.to(dtype).requires_grad_(True) for k, v in sd.items()}
        xx = x.to(dtype).requires_grad_(True)
        grads = torch.autograd.grad(A.attention(leaves, p, xx, groups), [xx] + list(leaves.values()), dy.to(dtype))
        return dict(zip(["x"] + [k[2:] for k in leaves], grads))
    o64, o32 = oracle(torch.float64), oracle(torch.float32)
    block = AttentionBlock(c, norm_num_groups=groups, eps=A.EPS)
    block.load_state_dict({k[2:]: v for k, v in sd.items()})
    block.to(dev)
    xd = x.to(dev).requires_grad_(True)
    y = block(xd)
    assert y.requires_grad
    grads = torch.autograd.grad(y, [xd] + list(block.parameters()), dy.to(dev), retain_graph=True)
    got = dict(zip(["x"] + [k for k, _ in block.named_parameters()], grads))
    for k in o64:
        check(k, got[k], o64[k], o32[k])
    again = torch.autograd.grad(y, [xd] + list(block.parameters()), dy.to(dev))
    assert all(torch.equal(a, b) for a, b in zip(grads, again))


# ------------------------------------------------------------------------------------------------ posterior
def test_posterior_backward(dev):
    g = torch.Generator().manual_seed(5)
    m = torch.randn(3, 8, 6, 10, generator=g) * 4
    m[0, 4, 0, :6] = torch.tensor([-31.0, -30.0, 20.0, 25.0, -30.000002, 20.000002])   # logvar at and beyond both clamps
    noise, dz, gkl = torch.randn(3, 4, 6, 10, generator=g), torch.randn(3, 4, 6, 10, generator=g), rnd((3,), 9)

    def oracle(dtype, with_noise, with_kl):
        mm = m.to(dtype).requires_grad_(True)
        mean, logvar = torch.chunk(mm, 2, dim=1)
        logvar = torch.clamp(logvar, -30.0, 20.0)
        std = torch.exp(0.5 * logvar)
        out = ((mean + std * noise.to(dtype) if with_noise else mean) * dz.to(dtype)).sum()
        if with_kl:
            out = out + (0.5 * torch.sum(mean ** 2 + std ** 2 - 1.0 - logvar, dim=[1, 2, 3]) * gkl.to(dtype)).sum()
        return torch.autograd.grad(out, mm)[0]
    md = m.to(dev)
    both = ops.aekl_posterior_bwd(md, dz.to(dev), noise.to(dev), gkl.to(dev))
    check("sample + kl", both, oracle(torch.float64, True, True), oracle(torch.float32, True, True))
    # inclusive boundaries, as torch.clamp's gradient: a gradient at exactly -30 and 20, none beyond
    lv = both[0, 4, 0, :6].cpu()
    assert lv[1] != 0 and lv[2] != 0 and lv[0] == 0 and lv[3] == 0 and lv[4] == 0 and lv[5] == 0
    check("sample", ops.aekl_posterior_bwd(md, dz.to(dev), noise.to(dev)), oracle(torch.float64, True, False),
          oracle(torch.float32, True, False))
    check("kl", ops.aekl_posterior_bwd(md, gkl=gkl.to(dev)), oracle(torch.float64, False, True),
          oracle(torch.float32, False, True))
    mode = ops.aekl_posterior_bwd(md, dz.to(dev))
    assert torch.equal(mode[:, :4].cpu(), dz) and not mode[:, 4:].any()      # mode() and no KL: exact zeros


# ------------------------------------------------------------------------------------------------ the whole model
@pytest.fixture(scope="module")
def g20():
    return np.load(G20, allow_pickle=False)


def golden_model(g20, dev):
    torch.manual_seed(int(g20["seed"]))
    model = AutoencoderKL(**A.CONFIGS[str(g20["config"])])
    assert R.values_digest(model.state_dict()) == str(g20["init_sha"])
    return model.to(dev).unfreeze().train()


def model_loss(model, x, noise, kl_weight):
    post = model.encode(x)
    dec = model.decode(post.sample(noise=noise) if noise is not None else post.mode())
    loss = Fn.l1_loss(dec, x)
    if kl_weight:
        loss = loss + kl_weight * post.kl().sum() / x.shape[0]
    return loss


def check_g20(g20, prefix, model, loss):
    bad = []
    t = tol(g20[prefix + "loss_spread"])
    err = abs(float(loss.detach()) - float(g20[prefix + "loss"])) / abs(float(g20[prefix + "loss"]))
    print(f"{prefix}loss: err {err:.3e} tol {t:.3e}")
    if not err <= t:
        bad.append((prefix + "loss", err, t))
    for k, p in model.named_parameters():
        name = f"{prefix}grad.{k}"
        t = tol(g20[name + "_spread"])
        assert p.grad is not None, k
        got = p.grad.detach().double().cpu()
        if name in g20.files:
            want = torch.from_numpy(g20[name])
            assert want.shape == got.shape, k
            if not want.any():
                err = nerr = float(got.abs().max())       # an exact zero is recorded: an exact zero is asked for
                t = 0.0
            else:
                err = nerr = rel(got, want)
        else:
            want = torch.from_numpy(g20[name + "_sample"])
            err = float((got.flatten()[T.sample_index(got.numel())] - want).abs().max() / float(g20[name + "_max"]))
            nerr = abs(float(got.norm()) - float(g20[name + "_norm"])) / float(g20[name + "_norm"])
        print(f"{name}: err {err:.3e} norm err {nerr:.3e} tol {t:.3e}")
        if not (err <= t and nerr <= t):
            bad.append((name, err, nerr, t))
    return bad


def test_golden_loss_and_gradients(dev, g20):
    """L1 + 1e-2 KL / B on forward(sample_posterior) with the stored noise: the loss and every parameter's gradient"""
    model = golden_model(g20, dev)
    x, noise = torch.from_numpy(g20["x"]).to(dev), torch.from_numpy(g20["noise"]).to(dev)
    loss = model_loss(model, x, noise, float(g20["kl_weight"]))
    loss.backward()
    bad = check_g20(g20, "", model, loss)
    assert not bad, bad


def test_golden_mode_without_kl(dev, g20):
    """posterior.mode() and no KL term: the logvar half of the moments gets no gradient, so the logvar rows of quant_conv
    (weight and bias) are exact zeros, here as in the fixture (check_g20 asks for an exact zero wherever one is recorded).
    encoder.conv_out feeds quant_conv, which mixes all of its channels into the mean rows: its logvar rows are not zero in
    the reference's gradients either, and are held to the fixture like every other tensor."""
    model = golden_model(g20, dev)
    x = torch.from_numpy(g20["x"]).to(dev)
    loss = model_loss(model, x, None, 0.0)
    loss.backward()
    bad = check_g20(g20, "mode_", model, loss)
    assert not bad, bad
    lc = model.latent_channels
    assert not g20["mode_grad.quant_conv.weight"][lc:].any() and g20["mode_grad.encoder.conv_out.bias"][lc:].any()
    assert not model.quant_conv.weight.grad[lc:].any() and not model.quant_conv.bias.grad[lc:].any()
    assert model.quant_conv.weight.grad[:lc].any()


def test_forward_call_matches_the_pieces_and_the_switch(dev, g20):
    model = golden_model(g20, dev)
    x = torch.from_numpy(g20["x"]).to(dev)
    dec, post = model(x, sample_posterior=True, return_posterior=True, generator=torch.Generator(device=dev).manual_seed(3))
    assert dec.requires_grad and post.kl().requires_grad and post.sample(noise=torch.zeros_like(post.mean)).requires_grad
    assert not post.mean.requires_grad
    with torch.no_grad():
        assert not model(x).requires_grad
    model.freeze()
    assert not model.training and all(not p.requires_grad for p in model.parameters())
    with pytest.raises(WfaeError, match="forward only"):
        model.encode(x.clone().requires_grad_(True))
    assert not model(x).requires_grad
    assert model.train().training is False and model.unfreeze().train().training is True


def grads_of(model, x, noise, kl_weight):
    model.zero_grad(set_to_none=True)
    model_loss(model, x, noise, kl_weight).backward()
    return [p.grad.clone() for p in model.parameters()]


def test_two_backward_passes_are_bitwise_identical(dev, g20):
    model = golden_model(g20, dev)
    x, noise = torch.from_numpy(g20["x"]).to(dev), torch.from_numpy(g20["noise"]).to(dev)
    a, b = grads_of(model, x, noise, 1e-2), grads_of(model, x, noise, 1e-2)
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_second_grad_under_retain_graph_equals_the_first(dev, g20):
    """the adaptive weight of the KL-GAN loss differentiates the graph twice before backward"""
    model = golden_model(g20, dev)
    x, noise = torch.from_numpy(g20["x"]).to(dev), torch.from_numpy(g20["noise"]).to(dev)
    loss = model_loss(model, x, noise, 1e-2)
    last = model.decoder.conv_out.weight
    first = torch.autograd.grad(loss, last, retain_graph=True)[0].clone()
    second = torch.autograd.grad(loss, last, retain_graph=True)[0].clone()
    loss.backward()
    assert torch.equal(first, second) and torch.equal(first, last.grad)
    assert all(p.grad is not None for p in model.parameters())


def test_train_launch_budget(dev):
    """entry-point calls (ops.profile_start / profile_stop) of one forward + backward of L1 + 1e-2 KL / B at the reference
    configuration "ref64" (1 x 1 x 128 x 128; 58 3x3 convolutions, 50 of them behind a GroupNorm + SiLU prologue).
    Designed for 390:
    forward 146 = the encode 64 + decode 79 of tests/test_aekl_gpu.py::test_launch_budget, the posterior kernel twice more
    (read-out, sample, KL instead of the read-out alone) and the L1 loss 1;
    backward 244 = 58 weight gradients (with the bias) + 57 data gradients (the first layer's input asks for none) + 50
    GroupNorm backward + 2 attention blocks x 29 (to_tokens of dy, 4 Linear x (weight, bias, data), 7 operand splits, 2
    transposes, 4 products, softmax backward, from_tokens, GroupNorm backward) + 6 1x1 convolutions x 3 (4 shortcuts,
    quant_conv, post_quant_conv: weight, data, bias) + posterior backward 2 + L1 backward 1.
    Bound: 1.5 x 390 = 585.  A step that follows an unchanged weight packs nothing; after an update each 3x3 weight is
    packed once per orientation (the first layer's rotated form is never asked for)."""
    torch.manual_seed(0)
    model = AutoencoderKL(**A.CONFIGS["ref64"]).to(dev).unfreeze().train()
    x = torch.rand(1, 1, 128, 128, generator=torch.Generator().manual_seed(1)).to(dev)
    noise = torch.randn(1, 64, 16, 16, generator=torch.Generator().manual_seed(2)).to(dev)
    n3 = sum(1 for m in model.modules() if type(m).__name__ == "Conv3x3")
    assert n3 == 58

    def count():
        model.zero_grad(set_to_none=True)
        ops.profile_start()
        model_loss(model, x, noise, 1e-2).backward()
        calls = {}
        for k, v in ops.profile_stop().items():
            calls[k.split(" ")[0]] = calls.get(k.split(" ")[0], 0) + v[0]
        return calls
    count()      # warm-up: weight packing, workspace
    step = count()
    total = sum(step.values())
    print("step", total, step)
    assert "wfae_aekl_conv3_pack" not in step
    assert total <= 585
    with torch.no_grad():
        for p in model.parameters():
            p.add_(p.grad, alpha=-1e-4)
    packs = count().get("wfae_aekl_conv3_pack", 0)
    print("packs after an update", packs)
    assert packs == 2 * n3 - 1


def test_the_fused_optimiser_step_reaches_the_packed_weights(dev, g20):
    """FusedAdamW writes the parameters through raw pointers.  The packed 3x3 weights must follow: after a step the model
    computes what a fresh model with the same state dict computes, and each orientation is packed once for the stepped weights"""
    from weatherforecastingtoolkit_amd.optim import FusedAdamW
    model = golden_model(g20, dev)
    opt = FusedAdamW(model.parameters(), lr=1e-2, weight_decay=0.0)
    x, noise = torch.from_numpy(g20["x"]).to(dev), torch.from_numpy(g20["noise"]).to(dev)
    before = model.decoder.conv_out.weight.detach().clone()
    for _ in range(2):
        model_loss(model, x, noise, 1e-2).backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
    assert not torch.equal(before, model.decoder.conv_out.weight)
    fresh = AutoencoderKL(**A.CONFIGS[str(g20["config"])]).to(dev)
    fresh.load_state_dict(model.state_dict())
    with torch.no_grad():
        assert torch.equal(model.decode(model.encode(x).mode()), fresh.decode(fresh.encode(x).mode()))
    ops.profile_start()
    model_loss(model, x, noise, 1e-2).backward()
    packs = sum(v[0] for k, v in ops.profile_stop().items() if k.startswith("wfae_aekl_conv3_pack"))
    n3 = sum(1 for m in model.modules() if type(m).__name__ == "Conv3x3")
    # the evaluation above re-packed the forward orientation of the stepped weights; this backward packs the rotated one
    # (of every layer but the first, whose data gradient is never taken)
    assert packs == n3 - 1
