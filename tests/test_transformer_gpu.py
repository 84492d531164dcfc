"""Kernel-level parity of csrc/transformer.hip and csrc/vit.hip (LayerNorm, multi-head attention with dropout,
dropout / ReLU, single-query attention, patch folding, the row-copy helpers) against tests/transformer_ref.py.

Inputs are seeded fp32 tensors; the reference is the restatement in float64 on the same fp32 values.  The tolerance
is measured, not guessed: the yardstick of a case is the error of the SAME restatement evaluated in float32 on the CPU
against float64, and a kernel passes when its own error is at most 4x that (the convention of
tests/golden/tf_sensitivity.py: two differently ordered fp32 sums sit about sqrt(2)-2x apart), with a floor of 16 fp32
epsilons relative to max |ref| (fewer than 16 roundings lie between an input and an output element of these ops).  The
yardstick never looks at the kernel's output.  Data movement and the dropout masks are exact: the RNG is counter-based,
so transformer_ref.keep_mask predicts every mask bit for bit from the seed."""
import numpy as np
import pytest
import torch
import torch.nn as tnn

from tests import transformer_ref as tr
from tests._util import relerr

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23
FLOOR = 16 * EPS32
SEEDS = [0, 1, 12345037042, 2 ** 63 - 1]
F64, F32 = torch.float64, torch.float32


def _check(family, label, got, ref, yard):
    """got: the kernel's fp32 result; ref: float64 restatement; yard: float32 restatement, same inputs"""
    err, y = relerr(got, ref), relerr(yard, ref)
    bar = max(4 * y, FLOOR)
    print(f"PARITY {family} {label}: kernel {err:.2e} yardstick {y:.2e} bar {bar:.2e}")
    assert np.isfinite(err) and err <= bar, (family, label, err, y, bar)


def _randn(gen, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen) * scale


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _keep(p):
    """1 / (1 - p) as the kernels form it: p is a C float and both operations round to float32"""
    return np.float32(1) / (np.float32(1) - np.float32(p))


# ----------------------------------------------------------------------------------------------------------- dropout
@pytest.mark.parametrize("n", [1, 255, 1025, 3 * 2 ** 20 + 7])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_mask_and_scale_exact(dev, n, p):
    """the zero pattern is ~keep_mask exactly and kept values are x * float32(1 / (1 - p)) bit for bit (the factor formed
    in float32 as the kernel forms it, which gives the same float for these p); the largest n
    exceeds 2048 blocks x 1024, so the kernel's grid-stride loop runs more than once"""
    from weatherforecastingtoolkit_amd import ops
    x = _randn(_gen(n), n)
    x[x == 0] = 1.0                                   # a zero input would hide a mask bit
    xd = x.to(dev)
    keep = _keep(p)
    for seed in SEEDS:
        y = ops.dropout(xd, p, seed).cpu().numpy()
        mask = tr.keep_mask(seed, n, p)
        assert np.array_equal(y != 0, mask), (seed, int((mask != (y != 0)).sum()))
        want = np.where(mask, x.numpy() * keep, np.float32(0))
        assert want.dtype == np.float32 and np.array_equal(y.view(np.uint32), want.view(np.uint32)), seed


def test_dropout_p0_is_identity(dev):
    from weatherforecastingtoolkit_amd import ops
    x = _randn(_gen(0), 1025)
    for seed in SEEDS:
        assert torch.equal(ops.dropout(x.to(dev), 0.0, seed).cpu(), x)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_fn_backward_uses_forward_mask(dev, p):
    from weatherforecastingtoolkit_amd import functional as Fn
    g = _gen(1)
    shape = (37, 100)
    x, dy = _randn(g, *shape), _randn(g, *shape)
    keep = _keep(p)
    for seed in SEEDS:
        xd = x.to(dev).requires_grad_(True)
        y = Fn.DropoutFn.apply(xd, p, seed)
        y.backward(dy.to(dev))
        mask = tr.keep_mask(seed, shape, p)
        assert np.array_equal(y.detach().cpu().numpy(), np.where(mask, x.numpy() * keep, np.float32(0)))
        assert np.array_equal(xd.grad.cpu().numpy(), np.where(mask, dy.numpy() * keep, np.float32(0)))


# --------------------------------------------------------------------------------------------------------- LayerNorm
LN_SHAPES = [(1, 1), (3, 5), (9, 63), (7, 65), (37, 100), (64, 64), (5, 2048), (8200, 8)]


def _ln_case(dev, rows, E, with_res, offset=0.0, seed=0):
    """forward and backward of one geometry against the restatement; returns the device tensors for further checks"""
    from weatherforecastingtoolkit_amd import ops
    g = _gen(1000 * rows + E + seed)
    x = _randn(g, rows, E) + offset
    res = _randn(g, rows, E) if with_res else None
    gamma, beta, dy = _randn(g, E) * 0.5 + 1.0, _randn(g, E), _randn(g, rows, E)
    label = f"({rows},{E}) res={with_res} offset={offset:g}"
    ref = tr.layernorm(x, res, gamma, beta, dtype=F64)
    yard = tr.layernorm(x, res, gamma, beta, dtype=F32)
    d = [None if t is None else t.to(dev) for t in (x, res, gamma, beta, dy)]
    y, mean, rstd = ops.layernorm_fwd(d[0], d[1], d[2], d[3])
    for name, got, r, yd in zip(("y", "mean", "rstd"), (y, mean, rstd), ref, yard):
        _check("layernorm_fwd", f"{label} {name}", got, r, yd)
    bref = tr.layernorm_bwd(x, res, gamma, beta, dy, dtype=F64)
    byard = tr.layernorm_bwd(x, res, gamma, beta, dy, dtype=F32)
    dg, db = torch.full((E,), 7.0, device=dev), torch.full((E,), -7.0, device=dev)     # must be overwritten
    dx = ops.layernorm_bwd(d[4], d[0], d[1], d[2], mean, rstd, dg, db)
    for name, got, r, yd in zip(("dx", "dgamma", "dbeta"), (dx, dg, db), bref, byard):
        _check("layernorm_bwd", f"{label} {name}", got, r, yd)
    return d, (mean, rstd), (dx, dg, db), bref, byard


@pytest.mark.parametrize("with_res", [True, False], ids=["res", "nores"])
@pytest.mark.parametrize("rows,E", LN_SHAPES)
def test_layernorm_fwd_bwd(dev, rows, E, with_res):
    """E % 64 != 0, rows % 4 != 0, more than 8 rows per block (8200 rows), E = 2048 (64 KiB of dynamic LDS)"""
    _ln_case(dev, rows, E, with_res)


@pytest.mark.parametrize("with_res", [True, False], ids=["res", "nores"])
def test_layernorm_large_common_offset(dev, with_res):
    """rows of 1000 + randn: only a two-pass variance is right (E[h^2] - mu^2 loses every digit of a variance of 1 next
    to a mean square of 1e6 and misses this bar by three orders)"""
    _ln_case(dev, 37, 100, with_res, offset=1000.0)


@pytest.mark.parametrize("rows,E", [(37, 100), (8200, 8)])
def test_layernorm_bwd_accumulate_and_repeatable(dev, rows, E):
    from weatherforecastingtoolkit_amd import ops
    d, (mean, rstd), (dx, dg, db), bref, byard = _ln_case(dev, rows, E, True, seed=5)
    g = _gen(9)
    g0, b0 = _randn(g, E, scale=3.0), _randn(g, E, scale=3.0)
    dg2, db2 = g0.to(dev), b0.to(dev)
    dx2 = ops.layernorm_bwd(d[4], d[0], d[1], d[2], mean, rstd, dg2, db2, accumulate=True)
    assert torch.equal(dx2, dx)
    _check("layernorm_bwd", f"({rows},{E}) accumulate dgamma", dg2, g0.double() + bref[1], g0 + byard[1])
    _check("layernorm_bwd", f"({rows},{E}) accumulate dbeta", db2, b0.double() + bref[2], b0 + byard[2])
    # two identical calls: bit-identical parameter gradients (fixed reduction order, no atomics)
    dg3, db3 = torch.empty_like(dg), torch.empty_like(db)
    dx3 = ops.layernorm_bwd(d[4], d[0], d[1], d[2], mean, rstd, dg3, db3)
    assert torch.equal(dg3, dg) and torch.equal(db3, db) and torch.equal(dx3, dx)


def test_layernorm_bwd_refuses_e_above_2048(dev):
    from weatherforecastingtoolkit_amd import ops
    from weatherforecastingtoolkit_amd._lib import WfaeError
    g = _gen(2049)
    xc, gc, bc = _randn(g, 2, 2049), _randn(g, 2049) * 0.5 + 1.0, _randn(g, 2049)
    x, gamma, beta = xc.to(dev), gc.to(dev), bc.to(dev)
    y, mean, rstd = ops.layernorm_fwd(x, None, gamma, beta)            # the forward has no such limit
    _check("layernorm_fwd", "(2,2049) y", y, tr.layernorm(xc, None, gc, bc, dtype=F64)[0],
           tr.layernorm(xc, None, gc, bc, dtype=F32)[0])
    with pytest.raises(WfaeError):
        ops.layernorm_bwd(torch.ones_like(x), x, None, gamma, mean, rstd, torch.empty_like(gamma), torch.empty_like(beta))


# --------------------------------------------------------------------------------------------------------- attention
def _mha_case(dev, S, N, H, D, batch_first, p, seed, scale=0.5, gen_seed=0):
    from weatherforecastingtoolkit_amd import ops
    E = H * D
    g = _gen(gen_seed + 7 * S + 131 * N + 17 * H + D)
    qkv, dout = _randn(g, S * N, 3 * E, scale=scale), _randn(g, S * N, E)
    mask = tr.keep_mask(seed, (N, H, S, S), p) if p > 0 else None
    label = f"{'bf' if batch_first else 'sf'} S={S} N={N} H={H} D={D} p={p} scale={scale:g}"
    res = {}
    for dt in (F64, F32):
        q = qkv.to(dt, copy=True).requires_grad_(True)
        out, probs = tr.mha(q, S, N, H, D, batch_first, mask, p)
        (dq,) = torch.autograd.grad(out, q, dout.to(dt))
        res[dt] = (out.detach(), probs.detach(), dq)
    qd = qkv.to(dev)
    out, probs = ops.mha_fwd(qd, S, N, H, D, p, seed, batch_first)
    dqkv = ops.mha_bwd(qd, probs, dout.to(dev), S, N, H, D, p, seed, batch_first)
    for name, got, r, yd in zip(("out", "probs", "dqkv"), (out, probs, dqkv), res[F64], res[F32]):
        _check("mha_bwd" if name == "dqkv" else "mha_fwd", f"{label} {name}", got, r, yd)


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("D", [8, 16, 64])
@pytest.mark.parametrize("batch_first", [False, True], ids=["seqfirst", "batchfirst"])
def test_mha_fwd_bwd(dev, batch_first, D, p):
    """S in {1, 2, 5, 63, 64} x (N, H) in {(3,1), (5,3)} and, at D = 8, (64,8); the mask is the replica's, indexed
    (n, h, i, j), and the backward must regenerate the forward's"""
    shapes = [(3, 1), (5, 3)] + ([(64, 8)] if D == 8 else [])
    for si, S in enumerate([1, 2, 5, 63, 64]):
        for N, H in shapes:
            _mha_case(dev, S, N, H, D, batch_first, p, SEEDS[(si + N) % 4])


@pytest.mark.parametrize("batch_first", [False, True], ids=["seqfirst", "batchfirst"])
def test_mha_large_logits(dev, batch_first):
    """qkv x8 at D = 64: logits in the hundreds, finite only because the row maximum is subtracted before expf"""
    for p in (0.0, 0.1):
        _mha_case(dev, 63, 3, 2, 64, batch_first, p, SEEDS[2], scale=8.0)


def test_mha_refuses_unbuilt_geometry(dev):
    from weatherforecastingtoolkit_amd import ops
    from weatherforecastingtoolkit_amd._lib import WfaeError
    for S, D in [(65, 8), (5, 32)]:
        N, H = 2, 2
        g = _gen(S + D)
        qkv = _randn(g, S * N, 3 * H * D).to(dev)
        with pytest.raises(WfaeError):
            ops.mha_fwd(qkv, S, N, H, D)
        probs = torch.full((N, H, S, S), 1.0 / S, device=dev)
        with pytest.raises(WfaeError):
            ops.mha_bwd(qkv, probs, _randn(g, S * N, H * D).to(dev), S, N, H, D)


@pytest.mark.parametrize("B,L,H,D", [(4, 64, 8, 256), (3, 1, 2, 64), (2, 3, 3, 40), (5, 63, 1, 100), (2, 17, 4, 8)])
def test_sq_attn_fwd_bwd(dev, B, L, H, D):
    """L < 64 (lanes >= L must drop out of the wave reductions), D % 64 != 0, D < 64"""
    from weatherforecastingtoolkit_amd import ops
    g = _gen(L + D)
    q, kv, dout = _randn(g, B, H * D, scale=0.5), _randn(g, B * L, 2 * H * D, scale=0.5), _randn(g, B, H * D)
    res = {}
    for dt in (F64, F32):
        qq, kk = q.to(dt, copy=True).requires_grad_(True), kv.to(dt, copy=True).requires_grad_(True)
        out, probs = tr.sq_attn(qq, kk, B, L, H, D)
        dq, dkv = torch.autograd.grad(out, (qq, kk), dout.to(dt))
        res[dt] = (out.detach(), probs.detach(), dq, dkv)
    out, probs = ops.sq_attn_fwd(q.to(dev), kv.to(dev), B, L, H, D)
    dq, dkv = ops.sq_attn_bwd(q.to(dev), kv.to(dev), probs, dout.to(dev), B, L, H, D)
    label = f"B={B} L={L} H={H} D={D}"
    for name, got, r, yd in zip(("out", "probs", "dq", "dkv"), (out, probs, dq, dkv), res[F64], res[F32]):
        _check("sq_attn_bwd" if name[0] == "d" else "sq_attn_fwd", f"{label} {name}", got, r, yd)


# ---------------------------------------------------------------------------------------------------- layout helpers
def test_copy_rows_four_addressing_modes(dev):
    from weatherforecastingtoolkit_amd import ops
    g = _gen(3)
    # (1, F) parameter expanded to B rows: src_ld = 0
    p = _randn(g, 77)
    assert torch.equal(ops.copy_rows(p.to(dev), 5, 77, 0).cpu(), p.expand(5, 77))
    # column slice [a, b) of a (rows, ld) tensor
    x = _randn(g, 9, 70)
    assert torch.equal(ops.copy_rows(x.to(dev), 9, 33, 70, src_off=13).cpu(), x[:, 13:46])
    # the slice's gradient: dy placed at dst_off inside zeroed rows, dst_off > 0 and dst_off + cols < dst_ld
    dy = _randn(g, 9, 33)
    want = torch.zeros(9, 70)
    want[:, 13:46] = dy
    got = ops.copy_rows(dy.to(dev), 9, 33, 33, dst_ld=70, dst_off=13, zero_fill=True).cpu()
    assert torch.equal(got, want)
    # every row repeated l times
    x = _randn(g, 7, 65)
    assert torch.equal(ops.copy_rows(x.to(dev), 7 * 3, 65, 65, row_div=3).cpu(), x.repeat_interleave(3, dim=0))
    # more elements than one pass of the grid (16384 blocks x 256): the grid-stride loop
    x = _randn(g, 2, 2049)
    n_rows = 2 * 2100
    assert torch.equal(ops.copy_rows(x.to(dev), n_rows, 2049, 2049, row_div=2100).cpu(),
                       x.repeat_interleave(2100, dim=0))


def test_sum_mid_and_add_bcast(dev):
    from weatherforecastingtoolkit_amd import ops
    g = _gen(4)
    for a, m, bn in [(1, 1, 1), (3, 5, 7), (2, 64, 65), (5, 17, 300)]:
        x = _randn(g, a, m, bn)
        _check("sum_mid", f"({a},{m},{bn})", ops.sum_mid(x.to(dev).view(a * m, bn), a, m, bn), x.double().sum(1), x.sum(1))
    for outer, inner in [((1,), (1,)), ((3,), (5, 7)), ((6,), (64, 33))]:
        x, p = _randn(g, *outer, *inner), _randn(g, *inner)
        assert torch.equal(ops.add_bcast(x.to(dev), p.to(dev)).cpu(), x + p)


def test_relu_fwd_bwd_exact(dev):
    """including +-0 and, for the backward, a negative saved output (dx = dy where y > 0, else 0)"""
    from weatherforecastingtoolkit_amd import ops
    g = _gen(5)
    x = _randn(g, 1031)
    x[:6] = torch.tensor([0.0, -0.0, 1e-45, -1e-45, float("inf"), -float("inf")])
    y = ops.relu_fwd(x.to(dev)).cpu()
    assert torch.equal(y, torch.relu(x)) and not bool((y < 0).any())
    ysaved = _randn(g, 1031)                            # negative entries on purpose
    ysaved[:4] = torch.tensor([0.0, -0.0, 1e-45, -3.0])
    dy = _randn(g, 1031)
    dx = ops.relu_bwd(dy.to(dev), ysaved.to(dev)).cpu()
    assert torch.equal(dx, torch.where(ysaved > 0, dy, torch.zeros(())))


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("P", [2, 16])
def test_patchify_unpatchify_bias(dev, P, C):
    from weatherforecastingtoolkit_amd import ops
    B, Hp, Wp = 2, 3, 5
    g = _gen(P + C)
    img, bias = _randn(g, B, C, Hp * P, Wp * P), _randn(g, C)
    want = img.view(B, C, Hp, P, Wp, P).permute(0, 2, 4, 1, 3, 5).reshape(B * Hp * Wp, C * P * P)
    rows = ops.patchify(img.to(dev), P)
    assert torch.equal(rows.cpu(), want)
    assert torch.equal(ops.unpatchify(rows, None, B, C, Hp, Wp, P).cpu(), img)
    assert torch.equal(ops.unpatchify(rows, bias.to(dev), B, C, Hp, Wp, P).cpu(), img + bias.view(1, C, 1, 1))


# ------------------------------------------------------------------------------------------- the training-mode layer
@pytest.fixture
def seed_log(monkeypatch):
    """records every seed functional.next_seed() hands out (nn.py and functional.dropout both call it through the
    module)"""
    from weatherforecastingtoolkit_amd import functional as Fn
    log = []
    real = Fn.next_seed

    def recording():
        s = real()
        log.append(s)
        return s

    monkeypatch.setattr(Fn, "next_seed", recording)
    return log


LAYERS = {
    "seqfirst_relu": dict(d=64, h=8, ff=256, act="relu", bf=False, shape=(5, 64, 64)),
    "batchfirst_gelu": dict(d=128, h=2, ff=128, act="gelu", bf=True, shape=(3, 16, 128)),
    "headdim16": dict(d=64, h=4, ff=96, act="relu", bf=False, shape=(7, 5, 64)),
}


@pytest.mark.parametrize("name", list(LAYERS))
def test_encoder_layer_train_mode_dropout(dev, seed_log, name):
    """nn.TransformerEncoderLayer in train mode with dropout 0.1 against the float64 restatement with the masks of
    the seeds actually issued: output, input gradient, every parameter gradient; a second forward draws four new seeds
    and matches its own restatement, not the first"""
    from weatherforecastingtoolkit_amd import nn as wnn
    cfg = LAYERS[name]
    p = 0.1
    torch.manual_seed(11)
    init = tnn.TransformerEncoderLayer(cfg["d"], cfg["h"], cfg["ff"], dropout=p, activation=cfg["act"],
                                       batch_first=cfg["bf"])
    with torch.no_grad():
        for n, q in init.named_parameters():
            if q.dim() == 1:
                q.copy_(torch.randn_like(q) * 0.3 + (1.0 if "norm" in n and "weight" in n else 0.0))
    mine = wnn.TransformerEncoderLayer(cfg["d"], cfg["h"], cfg["ff"], dropout=p, activation=cfg["act"],
                                       batch_first=cfg["bf"])
    mine.load_state_dict(init.state_dict())
    mine = mine.to(dev).train()
    sd = {k: v.detach().clone() for k, v in init.state_dict().items()}
    x, gy = torch.randn(*cfg["shape"]), torch.randn(*cfg["shape"])
    if cfg["bf"]:
        N, S, E = cfg["shape"]
    else:
        S, N, E = cfg["shape"]
    shapes = tr.layer_mask_shapes(S, N, cfg["h"], E, cfg["ff"])

    def restate(seeds, dt):
        masks = [tr.keep_mask(s, shp, p) for s, shp in zip(seeds, shapes)]
        w = {k: v.to(dt, copy=True).requires_grad_(True) for k, v in sd.items()}     # leaves of their own
        xi = x.to(dt, copy=True).requires_grad_(True)
        y = tr.encoder_layer(w, xi, cfg["h"], cfg["bf"], cfg["act"], masks, p)
        y.backward(gy.to(dt))
        return y.detach(), xi.grad, {k: v.grad for k, v in w.items()}

    outs = []
    for rnd in range(2):
        for q in mine.parameters():
            q.grad = None
        xd = x.to(dev).requires_grad_(True)
        yd = mine(xd)
        yd.backward(gy.to(dev))
        assert len(seed_log) == 4 * (rnd + 1), seed_log
        seeds = seed_log[-4:]
        ref, yard = restate(seeds, F64), restate(seeds, F32)
        _check("encoder_layer", f"{name} pass {rnd} out", yd, ref[0], yard[0])
        _check("encoder_layer", f"{name} pass {rnd} dx", xd.grad, ref[1], yard[1])
        for n, q in mine.named_parameters():
            _check("encoder_layer", f"{name} pass {rnd} d{n}", q.grad, ref[2][n], yard[2][n])
        outs.append((yd.detach(), ref[0]))
    assert len(set(seed_log)) == 8, seed_log
    assert relerr(outs[1][0], outs[0][1]) > 1e-2            # new masks: the second output is not the first's


def test_layer_eval_mode_draws_no_seed(dev, seed_log):
    from weatherforecastingtoolkit_amd import nn as wnn
    torch.manual_seed(12)
    mine = wnn.TransformerEncoderLayer(64, 8, 256, dropout=0.1).to(dev).eval()
    x = torch.randn(5, 6, 64).to(dev)
    with torch.no_grad():
        y = mine(x)
    assert seed_log == []
    sd = {k: v.detach().cpu() for k, v in mine.state_dict().items()}
    _check("encoder_layer", "eval out", y, tr.encoder_layer(sd, x.cpu(), 8, False, "relu", dtype=F64),
           tr.encoder_layer(sd, x.cpu(), 8, False, "relu", dtype=F32))


def test_tf_model_seed_stream(dev, seed_log):
    """PosAwareAE_TF at 128x128, B = 2: 8 layers x 4 dropout sites draw 32 seeds per train-mode forward, all distinct
    across two forwards (no site shares a seed, no step repeats its masks); eval mode draws none"""
    from weatherforecastingtoolkit_amd.pipeline.models.ae_64x8x8_tf import PosAwareAE_TF
    torch.manual_seed(0)
    net = PosAwareAE_TF().to(dev).train()
    x = torch.rand(2, 1, 128, 128).to(dev)
    with torch.no_grad():
        r0, _ = net(x)
        assert len(seed_log) == 32
        r1, _ = net(x)
    assert len(seed_log) == 64 and len(set(seed_log)) == 64
    assert bool(torch.isfinite(r0).all()) and not torch.equal(r0, r1)
    net.eval()
    with torch.no_grad():
        net(x)
    assert len(seed_log) == 64
