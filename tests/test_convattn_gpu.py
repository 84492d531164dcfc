"""GPU: the conv + attention latent autoencoder (csrc/convattn.hip, experiments/v1_experiments/_convattn.py) — the attention
kernels with two lengths, GroupNorm + GELU forward and backward, the channel bias and the one-key cross-attention against
fp64, the pre-norm encoder / decoder layers in eval and in training with regenerated masks, the whole model against the
reference's recorded step (tests/golden/g18_convattn.npz) and, at 16 tokens, against the restatement
tests/convattn_ref.py, the dead parameters, bitwise repeatability, the launch budget and the experiment.

Tolerances.  Every comparison is against fp64 values in the measure max|a - b| / max|b|.  Per tensor the bound is
max(4 x spread, 2e-6), spread = the same measure between an fp32 and an fp64 run of the restatement on the CPU (recorded in
the fixture, or measured inside the test), and never looser than the project's standing bars (outputs 1e-4, loss 1e-5,
gradients 5e-4) — the rule of tests/test_conv_disc_gpu.py.  GELU and Huber (delta 1) have continuous first derivatives, so
no gradient comparison needs a margin from a kink.  Error and bound of every comparison are printed."""
import os

import numpy as np
import pytest
import torch

from tests import convattn_ref as R
from weatherforecastingtoolkit_amd import config as C
from weatherforecastingtoolkit_amd import functional as Fn
from weatherforecastingtoolkit_amd import ops
from weatherforecastingtoolkit_amd._lib import WfaeError
from weatherforecastingtoolkit_amd.experiments.v1_experiments import _convattn as M
from weatherforecastingtoolkit_amd.optim import FusedAdamW

pytestmark = pytest.mark.gpu

G18 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g18_convattn.npz")
EXP = os.path.join(os.path.dirname(M.__file__), "pretrained_ae_convattn_ae_sevir")
BAR_OUT, BAR_LOSS, BAR_GRAD = 1e-4, 1e-5, 5e-4
FLOOR = 2e-6
H, D, E = 8, 16, 128
P_DROP = 0.1


@pytest.fixture(scope="module")
def g18():
    return np.load(G18, allow_pickle=False)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def tol(spread, bar=None):
    t = max(4.0 * float(spread), FLOOR)
    return min(t, bar) if bar is not None else t


def check(name, got, o64, o32, bar, bad):
    """`got` against the fp64 oracle, bounded by the fp32 oracle's own distance from it"""
    err, bound = rel(got, o64), tol(R.spread(o32, o64), bar)
    print(f"{name}: err {err:.3e} bound {bound:.3e}")
    if not err <= bound:
        bad.append((name, err, bound))


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------ wfae_attn_*
def attn_inputs(N, Sq, Skv, seed, special=False):
    g = gen(seed)
    q, k, v = torch.randn(N * Sq, E, generator=g), torch.randn(N * Skv, E, generator=g), torch.randn(N * Skv, E, generator=g)
    if special:
        # row 1 of sample 0: every score carries + 80 (k has a constant first component per head, q a matching one);
        # row 2: all scores equal (q = 0): uniform probabilities
        k.view(N * Skv, H, D)[:, :, 0] = 2.0
        q.view(N * Sq, H, D)[:, :, 0] = 0.0
        q.view(N * Sq, H, D)[1, :, 0] = 80.0 * D ** 0.5 / 2.0
        q[2] = 0.0
    return q, k, v, torch.randn(N * Sq, E, generator=g)


def attn_oracle(q, k, v, dout, N, Sq, Skv, mask, p, dtype):
    q, k, v = (t.detach().to(dtype).clone().requires_grad_(True) for t in (q, k, v))
    out, probs = R.attention(q, k, v, N, Sq, Skv, H, mask, p)
    out.backward(dout.to(dtype))
    return {"out": out.detach(), "probs": probs.detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad}


def attn_device(dev, q, k, v, dout, N, Sq, Skv, layout, p, seed):
    """ops.attn_fwd / attn_bwd through the packed [q | k | v] or the separate-q + [k | v] layout"""
    if layout == "packed":
        buf = torch.cat([q, k, v], 1).to(dev)
        dbuf = torch.full_like(buf, float("nan"))
        views = (buf[:, :E], buf[:, E:2 * E], buf[:, 2 * E:])
        dviews = (dbuf[:, :E], dbuf[:, E:2 * E], dbuf[:, 2 * E:])
    else:
        qd, kv = q.to(dev), torch.cat([k, v], 1).to(dev)
        dq, dkv = torch.full_like(qd, float("nan")), torch.full_like(kv, float("nan"))
        views, dviews = (qd, kv[:, :E], kv[:, E:]), (dq, dkv[:, :E], dkv[:, E:])
    out, probs = ops.attn_fwd(*views, N, Sq, Skv, H, D, p, seed)
    ops.attn_bwd(*views, probs, dout.to(dev), *dviews, N, Sq, Skv, H, D, p, seed)
    return {"out": out, "probs": probs, "dq": dviews[0].clone(), "dk": dviews[1].clone(), "dv": dviews[2].clone()}


ATTN_SHAPES = [(144, 144), (65, 65), (64, 64), (1, 144), (144, 1), (3, 5)]
ATTN_CASES = [(sq, skv, p, lay) for sq, skv in ATTN_SHAPES for p in (0.0, P_DROP)
              for lay in (("packed", "separate") if sq == skv else ("separate",))]


@pytest.mark.parametrize("case", ATTN_CASES, ids=lambda c: "%dx%d-p%g-%s" % c)
def test_attention_against_fp64(dev, case):
    Sq, Skv, p, layout = case
    N, seed = 2, 77 + Sq
    q, k, v, dout = attn_inputs(N, Sq, Skv, 1000 + 3 * Sq + Skv)
    mask = R.attn_mask(seed, N, H, Sq, Skv, p) if p > 0 else None
    if mask is not None:
        assert 0 < int(mask.sum()) < mask.size
    o64 = attn_oracle(q, k, v, dout, N, Sq, Skv, mask, p, torch.float64)
    o32 = attn_oracle(q, k, v, dout, N, Sq, Skv, mask, p, torch.float32)
    got = attn_device(dev, q, k, v, dout, N, Sq, Skv, layout, p, seed)
    bad = []
    for name in ("out", "probs"):
        check(name, got[name], o64[name], o32[name], BAR_OUT, bad)
    for name in ("dq", "dk", "dv"):
        if Skv == 1 and name in ("dq", "dk"):
            continue
        check(name, got[name], o64[name], o32[name], BAR_GRAD, bad)
    assert not bad, bad
    if Skv == 1:        # one key: the softmax is identically 1, nothing flows to q and k
        assert bool((got["probs"] == 1).all()) and bool((got["dq"] == 0).all()) and bool((got["dk"] == 0).all())
    again = attn_device(dev, q, k, v, dout, N, Sq, Skv, layout, p, seed)
    assert all(torch.equal(got[n], again[n]) for n in got)        # bitwise repeatable


def test_attention_offset_row_and_uniform_row(dev):
    N, S = 2, 65
    q, k, v, dout = attn_inputs(N, S, S, 4242, special=True)
    o64 = attn_oracle(q, k, v, dout, N, S, S, None, 0.0, torch.float64)
    o32 = attn_oracle(q, k, v, dout, N, S, S, None, 0.0, torch.float32)
    scores = (q.double().view(N, S, H, D).transpose(1, 2) @ k.double().view(N, S, H, D).transpose(1, 2).transpose(-2, -1)) / 4
    assert float(scores[0, :, 1].min()) > 60 and float(scores[0, :, 2].abs().max()) == 0.0
    assert float((o64["probs"][0, :, 2] - 1.0 / S).abs().max()) <= 1e-15
    bad = []
    for layout in ("packed", "separate"):
        got = attn_device(dev, q, k, v, dout, N, S, S, layout, 0.0, 0)
        for name, bar in (("out", BAR_OUT), ("probs", BAR_OUT), ("dq", BAR_GRAD), ("dk", BAR_GRAD), ("dv", BAR_GRAD)):
            check(f"{layout} {name}", got[name], o64[name], o32[name], bar, bad)
        assert bool(torch.isfinite(got["probs"]).all())
        assert float((got["probs"][0, :, 2].cpu() - 1.0 / S).abs().max()) <= 1e-8      # uniform row
    assert not bad, bad


def test_attention_agrees_with_mha_at_64(dev):
    N, S = 2, 64
    q, k, v, dout = attn_inputs(N, S, S, 64064)
    o64 = attn_oracle(q, k, v, dout, N, S, S, None, 0.0, torch.float64)
    o32 = attn_oracle(q, k, v, dout, N, S, S, None, 0.0, torch.float32)
    got = attn_device(dev, q, k, v, dout, N, S, S, "packed", 0.0, 0)
    qkv = torch.cat([q, k, v], 1).to(dev)
    out, probs = ops.mha_fwd(qkv, S, N, H, D, 0.0, 0, True)
    for name, a, b in (("out", got["out"], out), ("probs", got["probs"], probs)):
        err, bound = rel(a, b), tol(R.spread(o32[name], o64[name]), BAR_OUT)
        print(f"attn vs mha {name}: err {err:.3e} bound {bound:.3e}")
        assert err <= bound
    # the same masks at p > 0: wfae_mha_fwd's batch-first mask index is wfae_attn_fwd's at Sq = Skv
    a, _ = ops.attn_fwd(qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:], N, S, S, H, D, P_DROP, 5)
    b, _ = ops.mha_fwd(qkv, S, N, H, D, P_DROP, 5, True)
    assert rel(a, b) <= tol(R.spread(o32["out"], o64["out"]), BAR_OUT)


def test_attention_function_and_refusals(dev):
    """AttnFn in both forms gives the gradients of the packed buffers; unsupported shapes are refused"""
    N, S = 2, 5
    q, k, v, dout = attn_inputs(N, S, S, 9)
    o64 = attn_oracle(q, k, v, dout, N, S, S, None, 0.0, torch.float64)
    o32 = attn_oracle(q, k, v, dout, N, S, S, None, 0.0, torch.float32)
    qkv = torch.cat([q, k, v], 1).to(dev).requires_grad_(True)
    Fn.AttnFn.apply(qkv, None, N, S, S, H, 0.0, 0).backward(dout.to(dev))
    qd, kv = q.to(dev).requires_grad_(True), torch.cat([k, v], 1).to(dev).requires_grad_(True)
    Fn.AttnFn.apply(qd, kv, N, S, S, H, 0.0, 0).backward(dout.to(dev))
    bad = []
    want64, want32 = (torch.cat([o["dq"], o["dk"], o["dv"]], 1) for o in (o64, o32))
    check("dqkv", qkv.grad, want64, want32, BAR_GRAD, bad)
    check("dq", qd.grad, o64["dq"], o32["dq"], BAR_GRAD, bad)
    check("dkv", kv.grad, want64[:, E:], want32[:, E:], BAR_GRAD, bad)
    assert not bad, bad
    z = torch.zeros(N * 257, E, device=dev)
    with pytest.raises(WfaeError, match="256"):
        ops.attn_fwd(z, z, z, N, 257, 257, H, D)
    z = torch.zeros(N * S, 64, device=dev)
    with pytest.raises(WfaeError, match="head dim"):
        ops.attn_fwd(z, z, z, N, S, S, 8, 8)
    with pytest.raises(WfaeError, match="unit column stride|expected"):
        ops.attn_fwd(qkv.detach()[:, ::3], qkv.detach()[:, :E], qkv.detach()[:, :E], N, S, S, H, D)
    qd, dd = q.to(dev), dout.to(dev)
    out, probs = ops.attn_fwd(qd, qd, qd, N, S, S, H, D)
    for pr, do in ((probs[:, :, :, :S - 1].contiguous(), dd), (probs, dd[:-1])):     # refused, not read out of bounds
        with pytest.raises(WfaeError, match="attn_bwd: probs"):
            ops.attn_bwd(qd, qd, qd, pr, do, *(torch.empty_like(qd) for _ in range(3)), N, S, S, H, D)


# ------------------------------------------------------------------------------------------------ wfae_gn_act_*
GN_SHAPES = [(2, 64, 24, 24, 8), (2, 128, 12, 12, 8), (1, 16, 3, 5, 8), (3, 8, 1, 1, 8)]
GN_KINDS = ["benign", "offset", "constant", "spike"]
_gn_cache = {}


def gn_case(shape, kind, act, with_bias):
    """inputs and both oracles of one case, computed once and left unchanged"""
    key = (shape, kind, act, with_bias)
    if key not in _gn_cache:
        N, Cc, Hh, W, G = shape
        inp = R.gn_inputs(N, Cc, Hh, W, G, kind, 31 * Cc + 7 * Hh + GN_KINDS.index(kind))
        _gn_cache[key] = (inp, R.gn_oracle(inp, G, act, with_bias, torch.float64), R.gn_oracle(inp, G, act, with_bias, torch.float32))
    return _gn_cache[key]


GN_BARS = {"y": BAR_OUT, "mean": BAR_OUT, "rstd": BAR_OUT, "dx": BAR_GRAD, "dgamma": BAR_GRAD, "dbeta": BAR_GRAD,
           "dbias": BAR_GRAD}


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "prebias"])
@pytest.mark.parametrize("act", [0, 1], ids=["bare", "gelu"])
@pytest.mark.parametrize("kind", GN_KINDS)
@pytest.mark.parametrize("shape", GN_SHAPES, ids=lambda s: "n%d-c%d-%dx%d-g%d" % s)
def test_group_norm_act_against_fp64(dev, shape, kind, act, with_bias):
    gn_check(dev, shape, kind, act, with_bias)


# Groups above the workload's: 16 x 576 (36 KiB of LDS forward, 72 KiB backward: past the 64 KiB a launch gets unasked) and
# exactly WFAE_GN_MAX_GROUP, as one channel of 128 x 128 and as 16 channels of 32 x 32 (64 KiB forward, 128 KiB backward)
# (the gradient of a pre-bias on a group of one channel is a sum that cancels to zero: nothing to compare relatively)
GN_LARGE = [((1, 128, 24, 24, 8), 0, False), ((1, 128, 24, 24, 8), 1, True), ((2, 8, 128, 128, 8), 1, False),
            ((1, 32, 32, 32, 2), 0, False), ((1, 32, 32, 32, 2), 1, True)]


@pytest.mark.parametrize("shape,act,with_bias", GN_LARGE,
                         ids=lambda v: "n%d-c%d-%dx%d-g%d" % v if isinstance(v, tuple) else str(int(v)))
def test_group_norm_act_large_groups_against_fp64(dev, shape, act, with_bias):
    assert shape[1] // shape[4] * shape[2] * shape[3] in (16 * 576, ops.GN_MAX_GROUP)
    gn_check(dev, shape, "benign", act, with_bias)


def gn_check(dev, shape, kind, act, with_bias):
    """forward and backward of one case by the per-tensor rule, repeatability, accumulate"""
    G = shape[4]
    inp, o64, o32 = gn_case(shape, kind, act, with_bias)
    names = [n for n in GN_BARS if o64[n] is not None]
    for n in names:     # first, on the CPU: the fp32 restatement itself stays within the bars on these inputs
        assert R.spread(o32[n], o64[n]) <= GN_BARS[n], (n, R.spread(o32[n], o64[n]))
    t = {k: v.to(dev) for k, v in inp.items()}
    bias = t["bias"] if with_bias else None

    def run(accumulate=False, preset=None):
        y, mean, rstd = ops.gn_act_fwd(t["x"], t["gamma"], t["beta"], G, R.GN_EPS, act, bias)
        bufs = preset if preset is not None else [torch.full_like(t["gamma"], float("nan")) for _ in range(3)]
        dx = ops.gn_act_bwd(t["dy"], t["x"], t["gamma"], t["beta"], mean, rstd, bufs[0], bufs[1], G, act, bias,
                            bufs[2] if with_bias else None, accumulate)
        return {"y": y, "mean": mean, "rstd": rstd, "dx": dx, "dgamma": bufs[0], "dbeta": bufs[1],
                "dbias": bufs[2] if with_bias else None}

    got = run()
    bad = []
    for n in names:
        check(n, got[n], o64[n], o32[n], GN_BARS[n], bad)
    assert not bad, bad
    again = run()
    assert all(torch.equal(got[n], again[n]) for n in names)                                     # bitwise repeatable
    preset = [torch.full_like(t["gamma"], 0.5 * (i + 1)) for i in range(3)]
    acc = run(True, [p.clone() for p in preset])
    for i, n in enumerate(("dgamma", "dbeta", "dbias")):
        if got[n] is not None:
            assert torch.equal(acc[n], preset[i] + got[n]), n                                    # accumulate adds


def test_group_norm_function_and_refusals(dev):
    shape = (2, 128, 12, 12, 8)
    inp, o64, o32 = gn_case(shape, "benign", 1, True)
    t = {k: v.to(dev).requires_grad_(k != "dy") for k, v in inp.items()}
    Fn.GroupNormActFn.apply(t["x"], t["gamma"], t["beta"], t["bias"], 8, R.GN_EPS, 1).backward(t["dy"])
    bad = []
    for n, k in (("dx", "x"), ("dgamma", "gamma"), ("dbeta", "beta"), ("dbias", "bias")):
        check(n, t[k].grad, o64[n], o32[n], BAR_GRAD, bad)
    assert not bad, bad
    x = torch.zeros(1, 60, 4, 4, device=dev)
    with pytest.raises(WfaeError, match="divisible"):
        ops.gn_act_fwd(x, torch.ones(60, device=dev), torch.zeros(60, device=dev), 8)
    x = torch.zeros(1, 8, 129, 128, device=dev)
    with pytest.raises(WfaeError, match="16384"):
        ops.gn_act_fwd(x, torch.ones(8, device=dev), torch.zeros(8, device=dev), 8)
    g, st = torch.ones(8, device=dev), torch.zeros(1, 8, device=dev)
    with pytest.raises(WfaeError, match="16384"):
        ops.gn_act_bwd(x, x, g, g, st, st, g.clone(), g.clone(), 8)
    x = torch.zeros(2, 8, 4, 4, device=dev)          # mis-shaped gradients and statistics are refused, not read past
    st = torch.zeros(2, 8, device=dev)
    with pytest.raises(WfaeError, match="dbeta"):
        ops.gn_act_bwd(x, x, g, g, st, st, g.clone(), torch.zeros(4, device=dev), 8)
    with pytest.raises(WfaeError, match="statistics"):
        ops.gn_act_bwd(x, x, g, g, st[:1].contiguous(), st, g.clone(), g.clone(), 8)


# ------------------------------------------------------------------------------------------------ bias, one-key attention
@pytest.mark.parametrize("shape", [(2, 4, 48, 48), (3, 5, 7, 3)], ids=str)
def test_channel_bias(dev, shape):
    g = gen(17)
    x, b, dy = torch.randn(*shape, generator=g), torch.randn(shape[1], generator=g), torch.randn(*shape, generator=g)
    xd, bd = x.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    y = Fn.ChannelBiasFn.apply(xd, bd)
    y.backward(dy.to(dev))
    assert torch.equal(y.detach().cpu(), x + b.view(1, -1, 1, 1))          # one fp32 addition: exact
    assert torch.equal(xd.grad.cpu(), dy)
    want64, want32 = dy.double().sum((0, 2, 3)), dy.sum((0, 2, 3))
    bad = []
    check("dbias", bd.grad, want64, want32, BAR_GRAD, bad)
    assert not bad, bad


@pytest.mark.parametrize("p", [0.0, P_DROP], ids=["p0", "p0.1"])
@pytest.mark.parametrize("sq", [144, 5])
def test_head_dropout_bcast(dev, sq, p):
    N, seed = 3, 99
    g = gen(sq)
    v, dout = torch.randn(N, E, generator=g), torch.randn(N * sq, E, generator=g)
    mask = R.attn_mask(seed, N, H, sq, 1, p) if p > 0 else None

    def oracle(dtype):
        vv = v.to(dtype).clone().requires_grad_(True)
        out = R.head_dropout_bcast(vv, sq, H, mask, p)
        out.backward(dout.to(dtype))
        return out.detach(), vv.grad

    (o64, g64), (o32, g32) = oracle(torch.float64), oracle(torch.float32)
    vd = v.to(dev).requires_grad_(True)
    out = Fn.HeadDropoutBcastFn.apply(vd, sq, H, p, seed)
    out.backward(dout.to(dev))
    bad = []
    check("out", out, o64, o32, BAR_OUT, bad)
    check("dv", vd.grad, g64, g32, BAR_GRAD, bad)
    # the whole of a one-key attention: wfae_attn_fwd at Skv = 1 with the same seed
    q = torch.randn(N * sq, E, generator=g).to(dev)
    a, probs = ops.attn_fwd(q, vd.detach(), vd.detach(), N, sq, 1, H, D, p, seed)
    err, bound = rel(out, a), tol(R.spread(o32, o64), BAR_OUT)
    print(f"closed form vs attn at Skv = 1: err {err:.3e} bound {bound:.3e}")
    assert err <= bound and not bad, bad
    if p == 0:
        assert torch.equal(out.detach(), Fn.RepeatRowsFn.apply(vd.detach(), sq))
    else:
        assert np.array_equal((out.detach().view(N, sq, H, D)[..., 0] != 0).cpu().numpy().transpose(0, 2, 1), mask[..., 0])


# ------------------------------------------------------------------------------------------------ pre-norm layers
@pytest.fixture
def seed_log(monkeypatch):
    """records every seed functional.next_seed() hands out"""
    log = []
    real = Fn.next_seed

    def recording():
        s = real()
        log.append(s)
        return s

    monkeypatch.setattr(Fn, "next_seed", recording)
    return log


def make_layer(decoder, seed):
    torch.manual_seed(seed)
    kw = dict(d_model=E, nhead=H, dim_feedforward=4 * E, activation="gelu", batch_first=True, norm_first=True)
    layer = (torch.nn.TransformerDecoderLayer if decoder else torch.nn.TransformerEncoderLayer)(**kw)
    with torch.no_grad():
        for prm in layer.parameters():          # biases and norms away from their 0 / 1 initial values
            prm.add_(0.05 * torch.randn_like(prm))
    return layer


def layer_oracle(decoder, sd, x, mem, dy, masks, p, dtype):
    prm = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    xx = x.to(dtype).clone().requires_grad_(True)
    mm = mem.to(dtype).clone().requires_grad_(True)
    y = R.decoder_layer(prm, xx, mm, H, masks, p) if decoder else R.encoder_layer(prm, xx, H, masks, p)
    y.backward(dy.to(dtype))
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in prm.items()}
    return y.detach(), xx.grad, mm.grad if decoder else None, grads


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("decoder", [False, True], ids=["encoder", "decoder"])
def test_prenorm_layer_against_fp64(dev, seed_log, decoder, train):
    N, S = 2, 144
    layer = make_layer(decoder, 21 + decoder)
    sd = {k: v.detach().clone() for k, v in layer.state_dict().items()}
    g = gen(5 + decoder)
    x, mem, dy = torch.randn(N, S, E, generator=g), torch.randn(N, E, generator=g), torch.randn(N, S, E, generator=g)
    layer = layer.to(dev).train(train)
    xd, md = x.view(N * S, E).to(dev).requires_grad_(True), mem.to(dev).requires_grad_(True)
    y = M.decoder_layer(layer, xd, md, N, S) if decoder else M.encoder_layer(layer, xd, N, S)
    y.backward(dy.view(N * S, E).to(dev))
    shapes = R.decoder_mask_shapes(N, S) if decoder else R.encoder_mask_shapes(N, S)
    assert len(seed_log) == (len(shapes) if train else 0)
    masks = R.seeded_masks(seed_log, shapes, P_DROP) if train else None
    p = P_DROP if train else 0.0
    y64, dx64, dm64, g64 = layer_oracle(decoder, sd, x, mem, dy, masks, p, torch.float64)
    y32, dx32, dm32, g32 = layer_oracle(decoder, sd, x, mem, dy, masks, p, torch.float32)
    bad = []
    check("y", y.view(N, S, E), y64, y32, BAR_OUT, bad)
    check("dx", xd.grad.view(N, S, E), dx64, dx32, BAR_GRAD, bad)
    if decoder:
        check("dmemory", md.grad, dm64, dm32, BAR_GRAD, bad)
    pre = "decoder_tf.layers.0." if decoder else "encoder_tf.layers.0."
    dead = [d for d in R.dead_list(1) if d[0].startswith(pre)]
    assert len(dead) == (5 if decoder else 1)
    for k, prm in layer.named_parameters():
        assert prm.grad is not None, k
        dpart = R.dead_part(pre + k, prm.grad, dead)
        if dpart is not None:
            assert int(torch.count_nonzero(dpart)) == 0, k                   # exact zeros
        lg, l64, l32 = (R.live_part(pre + k, t, dead) for t in (prm.grad, g64[k], g32[k]))
        if l64 is not None:
            check(f"grad {k}", lg, l64, l32, BAR_GRAD, bad)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the whole model
def check_fixture(g, name, got, bar, report):
    """`got` against the recorded fp64 value `name`: whole, or on the stored sample (in units of the whole tensor's largest
    magnitude, like the spread) and the L2 norm"""
    t = tol(g[f"{name}_spread"], bar)
    got = got.detach().double().cpu()
    if name in g.files:
        want = torch.from_numpy(np.asarray(g[name])).double().reshape(got.shape)
        err = rel(got, want)
        print(f"{name}: err {err:.3e} bound {t:.3e}")
        if not err <= t:
            report.append((name, err, t))
        return
    want = torch.from_numpy(g[f"{name}_sample"]).double()
    err = float((got.flatten()[R.g18_index(got.numel())] - want).abs().max() / float(g[f"{name}_amax"]))   # the spread's unit
    wn = float(g[f"{name}_norm"])
    nerr = abs(float(got.norm()) - wn) / wn
    print(f"{name}: sample err {err:.3e} norm err {nerr:.3e} bound {t:.3e}")
    if not (err <= t and nerr <= t):
        report.append((name, err, nerr, t))


def seeded_model(dev, g):
    torch.manual_seed(int(g["seed"]))
    m = M.ConvAttnModel()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return m.to(dev).eval(), sd


def step(model, x):
    z, rec = model(x)
    return Fn.huber_loss(rec, x, 1.0), z, rec


def test_golden_parity(dev, g18):
    model, sd = seeded_model(dev, g18)
    assert R.values_digest(sd) == str(g18["init_sha"])        # the recorded initial weights, rebuilt from the seed
    dead = [(str(k), int(lo), int(hi)) for k, lo, hi in zip(g18["dead_keys"], g18["dead_lo"], g18["dead_hi"])]
    assert dead == R.dead_list()
    x = torch.from_numpy(g18["x"]).to(dev)
    bad = []
    loss, z, rec = step(model, x)
    check_fixture(g18, "z", z, BAR_OUT, bad)
    check_fixture(g18, "rec", rec, BAR_OUT, bad)
    err, bound = abs(float(loss) - float(g18["loss"])) / float(g18["loss"]), tol(g18["loss_spread"], BAR_LOSS)
    print(f"loss: err {err:.3e} bound {bound:.3e}")
    assert err <= bound
    loss.backward()
    params = dict(model.named_parameters())
    assert len(params) == 148
    live = {}
    for k, prm in params.items():
        assert prm.grad is not None, k
        dpart = R.dead_part(k, prm.grad, dead)
        if dpart is not None:
            assert int(torch.count_nonzero(dpart)) == 0, k
        part = R.live_part(k, prm.grad, dead)
        if part is not None:
            live[k] = part
            check_fixture(g18, f"grad_{k}", part, BAR_GRAD, bad)
    gn = R.grad_norm({k: v.cpu() for k, v in live.items()})
    err, bound = abs(gn - float(g18["gradnorm"])) / float(g18["gradnorm"]), tol(g18["gradnorm_spread"], BAR_GRAD)
    print(f"gradnorm: {gn:.6f} err {err:.3e} bound {bound:.3e}")
    assert err <= bound and gn > 1.0                     # the clip at 1.0 is active from the first step
    assert not bad, bad


def test_golden_parity_three_steps(dev, g18):
    """the live parameters after three steps of FusedAdamW (lr 1e-3, wd 1e-2, 1 - beta formed in double like torch) with
    clip_grad_norm_(1.0), as recorded, by the per-tensor rule max(4 x spread, 2e-6); the dead parameters equal to weight decay
    alone.  The biases start at zero, so their value IS the three Adam updates m / (sqrt(v) + eps), which turn the element-wise
    relative error of the smaller gradient entries into parameter error: this is the test that caught the softmax row sums
    (forward: the denominator, backward: sum_j P dP) accumulated in an fp32 chain — a rounding error shared by a whole row —
    with four biases of decoder layer 0 at 1.05 to 1.62 x their bound; they are summed in fp64 now."""
    model, sd = seeded_model(dev, g18)
    dead = R.dead_list()
    x = torch.from_numpy(g18["x"]).to(dev)
    params = dict(model.named_parameters())
    bad = []
    lr, wd, steps = float(g18["lr"]), float(g18["wd"]), int(g18["steps"])
    opt = FusedAdamW(model.parameters(), lr=lr, weight_decay=wd, exact_complements=True)
    for i in range(steps):
        loss, _, _ = step(model, x)
        loss.backward()
        total = opt.clip_grad_norm_(1.0)
        if i == 0:
            err, bound = abs(float(total) - float(g18["gradnorm"])) / float(g18["gradnorm"]), tol(g18["gradnorm_spread"], BAR_GRAD)
            assert err <= bound
        opt.step()
        opt.zero_grad(set_to_none=True)
    decay = (1.0 - lr * wd) ** steps
    for k, prm in params.items():
        part = R.live_part(k, prm.detach(), dead)
        if part is not None:
            check_fixture(g18, f"post_{k}", part, None, bad)
        dpart = R.dead_part(k, prm.detach(), dead)
        if dpart is not None:      # decay alone; three fp32 roundings of the product
            want = R.dead_part(k, sd[k], dead).double() * decay
            assert bool(((dpart.double().cpu() - want).abs() <= 4e-7 * want.abs()).all()), k
    assert not bad, bad


def test_model_at_16_tokens_against_restatement(dev, seed_log):
    """size = 16, three input channels, batch 3: eval, then training with every mask regenerated from the issued seeds"""
    torch.manual_seed(8)
    m = M.ConvAttnModel(in_channels=3, size=16)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x = torch.randn(3, 3, 16, 16, generator=gen(81))
    m = m.to(dev)
    bad = []
    for train in (False, True):
        m.train(train).zero_grad(set_to_none=True)
        del seed_log[:]
        loss, z, rec = step(m, x.to(dev))
        loss.backward()
        shapes = R.mask_shapes(3, 16)
        assert len(seed_log) == (len(shapes) if train else 0) == (40 if train else 0)
        masks = R.seeded_masks(seed_log, shapes, P_DROP) if train else None
        p = P_DROP if train else 0.0
        l64, z64, r64, g64 = R.run(sd, x, torch.float64, masks, p)
        l32, z32, r32, g32 = R.run(sd, x, torch.float32, masks, p)
        tag = "train" if train else "eval"
        check(f"{tag} z", z, z64, z32, BAR_OUT, bad)
        check(f"{tag} rec", rec, r64, r32, BAR_OUT, bad)
        check(f"{tag} loss", loss, l64, l32, BAR_LOSS, bad)
        for k, prm in m.named_parameters():
            dpart = R.dead_part(k, prm.grad)
            if dpart is not None:
                assert int(torch.count_nonzero(dpart)) == 0, k
            lg, a64, a32 = (R.live_part(k, t) for t in (prm.grad, g64[k], g32[k]))
            if a64 is not None:
                check(f"{tag} grad {k}", lg, a64, a32, BAR_GRAD, bad)
    assert not bad, bad


def test_loss_and_gradients_bitwise_repeatable(dev, g18):
    model, _ = seeded_model(dev, g18)
    x = torch.randn(8, 4, 48, 48, generator=gen(4)).to(dev)
    runs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        loss, _, _ = step(model, x)
        loss.backward()
        runs.append([loss.detach().clone()] + [prm.grad.clone() for prm in model.parameters()])
    torch.cuda.synchronize()
    assert len(runs[0]) == 149
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# Entry-point calls of one training forward + loss + backward, derived from the composition ("Launch
# census").  L = 45 Linears: 4 per encoder layer, 6 per decoder layer (in / out projection, the cross-attention's v rows and
# out projection, the feed-forward's two), 3 in the attention pool, the head and the memory projection.
LAUNCHES = {
    "wfae_c3s2_fwd": 2, "wfae_c3s2_bwd_weight": 2, "wfae_c3s2_bwd_data": 1,     # the input needs no gradient
    "wfae_gn_act_fwd": 3, "wfae_gn_act_bwd": 3,
    "wfae_patchify": 2, "wfae_unpatchify": 2,                                    # planes <-> tokens, each with its backward
    "wfae_add_bcast": 2, "wfae_copy_rows": 2,                                    # position embeddings, learned queries
    "wfae_layernorm_fwd": 17, "wfae_layernorm_bwd": 17,                          # 2 per layer (norm2 of a decoder layer: none) + 1
    "wfae_linear_fwd": 45, "linear_bwd_weight": 45, "linear_bwd_data": 45,
    "wfae_reduce_sum": 50,                                                       # 45 Linear biases, 4 learned tensors, the last bias
    "wfae_attn_fwd": 9, "wfae_attn_bwd": 9,                                      # 4 + 4 self-attentions and the pool
    "wfae_head_dropout_bcast_fwd": 4, "wfae_head_dropout_bcast_bwd": 4,
    "wfae_gelu_fwd": 8, "wfae_gelu_bwd": 8,
    "wfae_dropout": 2 * (4 * 3 + 4 * 4),                                         # 3 / 4 element-wise sites per layer
    "wfae_add": 20,                                                              # 2 / 3 residuals per layer
    "wfae_channel_bias_fwd": 1, "wfae_huber_fwd": 1, "wfae_huber_bwd": 1,
}
TCONV_BUDGET = 14       # measured, not derived: the 4x4 stride-2 family's plans for 128 -> 64 (Winograd) and 64 -> 4 (gather)


def test_launch_budget(dev, g18):
    """one forward + loss + backward of a training step (dropout on) at B = 8: every entry point outside the transposed
    convolutions is called exactly as often as the composition says (359 calls; a Linear's two gradients may each take the
    split-K entry point), and the transposed convolutions stay within the 14 calls measured for their plans: 373 in all."""
    model, _ = seeded_model(dev, g18)
    model.train()
    x = torch.randn(8, 4, 48, 48, generator=gen(4)).to(dev)
    step(model, x)[0].backward()      # warm-up: workspace allocation
    model.zero_grad(set_to_none=True)
    ops.profile_start()
    step(model, x)[0].backward()
    prof = ops.profile_stop()
    n = {k: v[0] for k, v in prof.items()}
    print(n, sum(n.values()))
    tconv = sum(v for k, v in n.items() if k.startswith(("wfae_wino_", "wfae_conv4x4s2_")))
    rest = {}
    for k, v in n.items():
        if not k.startswith(("wfae_wino_", "wfae_conv4x4s2_")):
            k = k[len("wfae_"):-len("_splitk")] if k.endswith("_splitk") else k
            k = k[len("wfae_"):] if k in ("wfae_linear_bwd_weight", "wfae_linear_bwd_data") else k
            rest[k] = rest.get(k, 0) + v
    assert rest == LAUNCHES, {k: (rest.get(k), LAUNCHES.get(k)) for k in set(rest) | set(LAUNCHES) if rest.get(k) != LAUNCHES.get(k)}
    assert sum(LAUNCHES.values()) == 359 and 0 < tconv <= TCONV_BUDGET, n


def test_experiment_fits_and_tests(dev, tmp_path, capsys, g18):
    """three training steps of the Model on latents, then the documented commands: a fit of 3 steps and one --mode test pass"""
    cfg = C.load(os.path.join(EXP, "config.yaml"))
    cfg.trainer.total_train_steps = 10
    torch.manual_seed(0)
    model = M.Model(cfg).to(dev).train()
    model.configure_optimizers()
    latents = torch.randn(4, 1, 4, 48, 48, generator=gen(2)).to(dev)
    before = {k: v.detach().clone() for k, v in model.predictor.state_dict().items()}
    losses = []
    for _ in range(3):
        loss, gn = model.training_step(latents)
        losses.append(float(loss))
        assert np.isfinite(float(loss)) and float(gn) > 1.0
    Fn.join_side_stream()
    print("losses", losses)
    after = model.predictor.state_dict()
    moved = {k: not torch.equal(before[k], after[k]) for k in before}
    dead_whole = {k for k, s in M.dead_parameters(model.predictor) if s is None}
    assert all(v for k, v in moved.items() if k not in dead_whole and not k.endswith("in_proj_bias")), moved
    for k, s in M.dead_parameters(model.predictor):     # weight decay alone: zeros stay zeros, norm2.weight shrinks from 1
        a, b = (before[k], after[k]) if s is None else (before[k][s], after[k][s])
        assert bool(((b - a).abs() <= 1e-3 * a.abs()).all()) and float((b.abs() - a.abs()).max()) <= 0, k
    model.eval()
    vloss, logs = model.validation_step(latents)
    assert list(logs) == ["val_loss"] and np.isfinite(float(vloss))
    _, tlogs = model.test_step(latents)
    assert list(tlogs) == ["test_loss"]
    with pytest.raises(WfaeError, match="4, 48, 48"):
        model.training_step(torch.zeros(2, 1, 4, 24, 24, device=dev))

    from weatherforecastingtoolkit_amd.experiments.v1_experiments.pretrained_ae_convattn_ae_sevir import train
    capsys.readouterr()
    assert train.main(["--max-steps", "3", "dataset.batch_size=2", f"experiment_path={tmp_path}"]) == 0
    out = capsys.readouterr().out
    assert out.strip().endswith("done") and out.count('"train_loss"') == 3
    ck = torch.load(tmp_path / "outputs" / "pretrained_ae_convattn_ae_sevir" / "checkpoints" / "last.ckpt", map_location="cpu")
    assert ck["global_step"] == 3
    assert list(ck["state_dict"]) == ["predictor._orig_mod." + str(k) for k in g18["keys"]]
    M.load_predictor_state(model, ck["state_dict"])
    assert train.main(["--mode", "test", "--max-steps", "1", "dataset.batch_size=2", f"experiment_path={tmp_path}"]) == 0
    out = capsys.readouterr().out
    assert out.strip().endswith("done") and '"test_loss"' in out and '"test_' in out.replace('"test_loss"', "")
