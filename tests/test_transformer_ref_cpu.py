"""tests/transformer_ref.py earns its trust on the CPU: the restatement of the encoder layer, of both attention
layouts and of single-query attention against torch in float64, and the statistics of the RNG replica that
tests/test_transformer_gpu.py uses to predict the dropout masks of csrc/transformer.hip bit for bit."""
import math

import numpy as np
import pytest
import torch
import torch.nn as tnn
import torch.nn.functional as F

from tests import transformer_ref as tr
from tests._util import relerr

SEEDS = [0, 1, 12345037042, 2 ** 63 - 1]
N_STAT = 1 << 20


def test_rng01_matches_integer_arithmetic():
    """the vectorised uint64 replica against the same finaliser in Python integers reduced mod 2**64"""
    m = (1 << 64) - 1

    def one(seed, idx):
        z = (seed + idx * 0x9E3779B97F4A7C15 + 0x9E3779B97F4A7C15) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        z ^= z >> 31
        return (z >> 40) / 16777216.0

    idx = [0, 1, 2, 63, 4095, 2 ** 31 - 1, 2 ** 31, 2 ** 40 + 17]
    for seed in SEEDS + [2 ** 63]:
        got = tr.rng01(seed, idx)
        assert got.dtype == np.float32
        assert [float(v) for v in got] == [one(seed, i) for i in idx]
        assert float(got.min()) >= 0.0 and float(got.max()) < 1.0


def test_keep_mask_shape_and_float_threshold():
    a = tr.keep_mask(7, 1000, 0.1)
    b = tr.keep_mask(7, (10, 4, 25), 0.1)
    assert a.dtype == np.bool_ and b.shape == (10, 4, 25) and np.array_equal(a, b.reshape(-1))
    # float32(0.1) > 0.1: a draw equal to k * 2**-24 between the two would flip under a double comparison
    r = tr.rng01(7, np.arange(1000))
    assert np.array_equal(a, r >= np.float32(0.1))
    assert tr.keep_mask(7, 1000, 0.0).all()


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("seed", SEEDS)
def test_keep_rate_and_independence(seed, p):
    """keep rate within 4 sigma of 1 - p; the masks of consecutive seeds (what next_seed() hands out) and a mask and
    itself shifted by one index agree at a rate within 4 sigma of (1-p)^2 + p^2.  sigma = sqrt(p (1-p) / n) for the
    rate and sqrt(a (1-a) / n) for an agreement rate a.  Fixed seeds: nothing here is random."""
    n = N_STAT
    m0 = tr.keep_mask(seed, n, p)
    m1 = tr.keep_mask(seed + 1, n, p)
    sig = math.sqrt(p * (1 - p) / n)
    z_rate = (m0.mean() - (1 - p)) / sig
    agree = (1 - p) ** 2 + p ** 2
    sig_a = math.sqrt(agree * (1 - agree) / n)
    z_seed = ((m0 == m1).mean() - agree) / sig_a
    z_shift = ((m0[1:] == m0[:-1]).mean() - agree) / sig_a
    print(f"seed {seed} p {p}: keep {z_rate:+.2f} sigma, seed+1 {z_seed:+.2f} sigma, shift {z_shift:+.2f} sigma")
    assert abs(z_rate) <= 4 and abs(z_seed) <= 4 and abs(z_shift) <= 4


def _sdpa_rows(qkv, S, N, H, D, batch_first):
    E = H * D
    x = qkv.view(N, S, 3, H, D) if batch_first else qkv.view(S, N, 3, H, D).transpose(0, 1)
    q, k, v = [x[:, :, c].transpose(1, 2) for c in range(3)]                # (N, H, S, D)
    o = F.scaled_dot_product_attention(q, k, v).transpose(1, 2)             # (N, S, H, D)
    return (o if batch_first else o.transpose(0, 1)).reshape(S * N, E)


@pytest.mark.parametrize("batch_first", [False, True])
def test_mha_restatement_vs_sdpa(batch_first):
    torch.manual_seed(2)
    for S, N, H, D in [(5, 3, 2, 8), (1, 4, 1, 16), (7, 2, 3, 64)]:
        qkv = torch.randn(S * N, 3 * H * D, dtype=torch.float64, requires_grad=True)
        dout = torch.randn(S * N, H * D, dtype=torch.float64)
        out, probs = tr.mha(qkv, S, N, H, D, batch_first)
        (g,) = torch.autograd.grad(out, qkv, dout)
        ref = _sdpa_rows(qkv, S, N, H, D, batch_first)
        (gr,) = torch.autograd.grad(ref, qkv, dout)
        assert relerr(out, ref) <= 1e-12 and relerr(g, gr) <= 1e-12
        assert tuple(probs.shape) == (N, H, S, S)
        assert relerr(probs.sum(-1), torch.ones(N, H, S, dtype=torch.float64)) <= 1e-12
        # an all-ones mask with p = 0 is the identity; a mask scales single probabilities
        out1, _ = tr.mha(qkv, S, N, H, D, batch_first, np.ones((N, H, S, S), bool), 0.0)
        assert torch.equal(out1, out)
        if S > 1:
            mk = np.ones((N, H, S, S), bool)
            mk[0, 0, 0, 1] = False
            out2, _ = tr.mha(qkv, S, N, H, D, batch_first, mk, 0.5)
            x = qkv.detach().view(N, S, 3, H, D) if batch_first else qkv.detach().view(S, N, 3, H, D).transpose(0, 1)
            v = x[0, :, 2, 0]                                               # (S, D) values of (n 0, h 0)
            pr = probs.detach()[0, 0, 0].clone()
            pr[1] = 0
            assert relerr(out2.detach()[0, :D], 2 * (pr @ v)) <= 1e-12      # row 0 is (s 0, n 0) in both layouts


def test_sq_attn_restatement_vs_sdpa():
    torch.manual_seed(3)
    for B, L, H, D in [(2, 5, 3, 8), (3, 1, 2, 16), (2, 64, 2, 40)]:
        q = torch.randn(B, H * D, dtype=torch.float64, requires_grad=True)
        kv = torch.randn(B * L, 2 * H * D, dtype=torch.float64, requires_grad=True)
        dout = torch.randn(B, H * D, dtype=torch.float64)
        out, probs = tr.sq_attn(q, kv, B, L, H, D)
        g = torch.autograd.grad(out, (q, kv), dout)
        x = kv.view(B, L, 2, H, D)
        ref = F.scaled_dot_product_attention(q.view(B, H, 1, D), x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2))
        ref = ref.reshape(B, H * D)
        gr = torch.autograd.grad(ref, (q, kv), dout)
        assert tuple(probs.shape) == (B, H, L)
        assert relerr(out, ref) <= 1e-12
        for a, b in zip(g, gr):
            if L == 1 and float(a.abs().max()) == 0.0:       # softmax over one key: dq = dk = 0, torch leaves rounding
                assert float(b.abs().max()) <= 1e-12
            else:
                assert relerr(a, b) <= 1e-12


def test_layernorm_restatement_vs_torch():
    torch.manual_seed(4)
    x, res = torch.randn(9, 63, dtype=torch.float64), torch.randn(9, 63, dtype=torch.float64)
    g, b, dy = [torch.randn(*s, dtype=torch.float64) for s in [(63,), (63,), (9, 63)]]
    for r in (res, None):
        h = (x if r is None else x + r).clone().requires_grad_(True)
        gg, bb = g.clone().requires_grad_(True), b.clone().requires_grad_(True)
        ref = F.layer_norm(h, (63,), gg, bb, 1e-5)
        gr = torch.autograd.grad(ref, (h, gg, bb), dy)
        y, mean, rstd = tr.layernorm(x, r, g, b)
        assert relerr(y, ref) <= 1e-12
        assert relerr(mean, h.detach().mean(-1)) <= 1e-12
        assert relerr(rstd, (h.detach().var(-1, unbiased=False) + 1e-5).rsqrt()) <= 1e-12
        for a, c in zip(tr.layernorm_bwd(x, r, g, b, dy), gr):
            assert relerr(a, c) <= 1e-12


@pytest.mark.parametrize("cfg", [dict(d=64, h=8, ff=256, act="relu", bf=False, shape=(5, 6, 64)),
                                 dict(d=128, h=2, ff=128, act="gelu", bf=True, shape=(3, 16, 128))],
                         ids=["seqfirst_relu", "batchfirst_gelu"])
def test_encoder_layer_restatement_vs_torch(cfg):
    """float64, p = 0, against nn.TransformerEncoderLayer in train mode with dropout 0: output, input gradient and
    every parameter gradient to 1e-12 relative"""
    torch.manual_seed(5)
    ref = tnn.TransformerEncoderLayer(cfg["d"], cfg["h"], cfg["ff"], dropout=0.0, activation=cfg["act"],
                                      batch_first=cfg["bf"]).double().train()
    with torch.no_grad():
        for n, p in ref.named_parameters():                                  # norms start at (1, 0), biases at 0
            if p.dim() == 1:
                p.copy_(torch.randn_like(p) * 0.5 + (1.0 if "norm" in n and "weight" in n else 0.0))
    x = torch.randn(*cfg["shape"], dtype=torch.float64)
    gy = torch.randn_like(x)
    xr = x.clone().requires_grad_(True)
    ref(xr).backward(gy)
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in ref.state_dict().items()}
    xm = x.clone().requires_grad_(True)
    y = tr.encoder_layer(sd, xm, cfg["h"], cfg["bf"], cfg["act"])
    y.backward(gy)
    assert relerr(y, ref(x)) <= 1e-12
    assert relerr(xm.grad, xr.grad) <= 1e-12
    names = [n for n, _ in ref.named_parameters()]
    assert sorted(names) == sorted(sd)
    for n, p in ref.named_parameters():
        assert relerr(sd[n].grad, p.grad) <= 1e-12, n
    # the float32 evaluation (the yardstick of the GPU tests) is the same function to float32 accuracy
    y32 = tr.encoder_layer({k: v.detach() for k, v in sd.items()}, x, cfg["h"], cfg["bf"], cfg["act"],
                           dtype=torch.float32)
    assert y32.dtype == torch.float32 and relerr(y32, y) < 1e-5


def test_encoder_layer_masks_reach_their_sites():
    """each of the four masks changes the output, and a mask of ones with p = 0 does not"""
    torch.manual_seed(6)
    S, N, E, H, FF = 4, 3, 16, 2, 24
    ref = tnn.TransformerEncoderLayer(E, H, FF, dropout=0.0).double()
    sd = {k: v.detach() for k, v in ref.state_dict().items()}
    x = torch.randn(S, N, E, dtype=torch.float64)
    shapes = tr.layer_mask_shapes(S, N, H, E, FF)
    ones = [np.ones(s, bool) for s in shapes]
    base = tr.encoder_layer(sd, x, H, False, "relu")
    assert torch.equal(tr.encoder_layer(sd, x, H, False, "relu", ones, 0.0), base)
    outs = []
    for site in range(4):
        mk = [np.ones(s, bool) for s in shapes]
        mk[site] = tr.keep_mask(11 + site, shapes[site], 0.5)
        outs.append(tr.encoder_layer(sd, x, H, False, "relu", mk, 0.5))
        assert relerr(outs[-1], base) > 1e-3, site
    for i in range(4):
        for j in range(i):
            assert relerr(outs[i], outs[j]) > 1e-3, (i, j)
