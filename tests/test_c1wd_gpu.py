"""csrc/c1wd.hip — the last 1x1 weight gradient dW3 = dy . gelu(bn3(t2))^T and the data gradient dA3 = W3^T dy of a C <= 256
Bottleneck's backward pass in ONE pass over dy, against the pair of launches it replaces: ops.conv1x1_bwd_weight_bnact on
csrc/c1w.hip and the c1r data gradient.  The fused kernel repeats both kernels' operations per output element (the same MFMA
instruction, the same position of every contraction index, the same order of the six plane products, the same split-K slabs),
so both results must keep their bits; a tile fetched, transposed or stored wrongly cannot hide in a tolerance.

The wrapper ops.conv1x1_bwd_wd is called directly: the pixel threshold of ops.conv1x1_wd_route is not in the way."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

# (C, NB, H, W): ten K-steps and no multiple of 128 pixels; C = 256; HW = 832 is the smallest pixel count (a multiple of 64) at
# which c1w's chunking gives an image more than one chunk with a short last one (3 chunks of 288, 288, 256 pixels)
SHAPES = [(128, 3, 16, 20), (256, 2, 24, 24), (128, 1, 26, 32)]


@pytest.fixture(scope="module")
def ops(dev):
    from weatherforecastingtoolkit_amd import ops as o
    assert o.c1wd_enabled()
    return o


def normal(shape, seed, dev, offset=0):
    """seeded normal values with a per-channel offset and scale; `offset` floats into a larger buffer (storage offset)"""
    g = torch.Generator().manual_seed(seed)
    c = shape[1]
    v = torch.randn(shape, generator=g) * (0.5 + torch.rand((1, c, 1, 1), generator=g)) + torch.randn((1, c, 1, 1), generator=g)
    buf = torch.empty(v.numel() + offset, device=dev)
    out = buf[offset:].view(shape)
    out.copy_(v)
    return out


def stats(ops, dev, m, seed):
    g = torch.Generator().manual_seed(seed)
    st = ops.BnStats(m, dev)
    st.scale.copy_(torch.rand(m, generator=g) + 0.5)
    st.shift.copy_(torch.rand(m, generator=g) - 0.5)
    return st


def activated64(x, scale, shift):
    """float64 GELU of the fp32 value u = fma(x, scale, shift) the kernels evaluate"""
    u = (x.double() * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)).float().double()
    return 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))


def pair(ops, dy, t2, st, w3, dw=None, accumulate=False):
    dw = torch.empty_like(w3) if dw is None else dw
    ops.conv1x1_bwd_weight_bnact(dy, t2, st, dw, accumulate)
    return dw, ops._c1_launch("c1r", w3, True, dy)[0]


def fused(ops, dy, t2, st, w3, dw=None, accumulate=False):
    dw = torch.empty_like(w3) if dw is None else dw
    da = ops.conv1x1_bwd_wd(dy, t2, st, w3, dw, accumulate)
    assert da is not None, "not served"
    return dw, da


_cases = {}


def case(ops, dev, c, nb, h, w, offset=0):
    key = (c, nb, h, w, offset)
    if key not in _cases:
        mid = c // 4
        dy, t2 = normal((nb, c, h, w), 1, dev, offset), normal((nb, mid, h, w), 2, dev, offset)
        w3 = (torch.randn((c, mid, 1, 1), generator=torch.Generator().manual_seed(3)) * 0.2).to(dev)
        st = stats(ops, dev, mid, 4)
        _cases[key] = dict(dy=dy, t2=t2, w3=w3, st=st, pair=pair(ops, dy, t2, st, w3), fused=fused(ops, dy, t2, st, w3))
    return _cases[key]


@pytest.mark.parametrize("c,nb,h,w", SHAPES)
def test_c1wd_keeps_the_bits_of_the_pair(ops, dev, c, nb, h, w):
    k = case(ops, dev, c, nb, h, w)
    (dw_p, da_p), (dw_f, da_f) = k["pair"], k["fused"]
    assert torch.equal(dw_f, dw_p), "dW3: %g" % float((dw_f - dw_p).abs().max())
    assert torch.equal(da_f, da_p), "dA3: %g" % float((da_f - da_p).abs().max())
    # accumulating into a gradient that is already there
    base = torch.full_like(k["w3"], 0.75)
    dw_pa, _ = pair(ops, k["dy"], k["t2"], k["st"], k["w3"], base.clone(), True)
    dw_fa, _ = fused(ops, k["dy"], k["t2"], k["st"], k["w3"], base.clone(), True)
    assert torch.equal(dw_fa, dw_pa) and not torch.equal(dw_fa, dw_p)


@pytest.mark.parametrize("c,nb,h,w", SHAPES[:2])
def test_c1wd_at_a_storage_offset(ops, dev, c, nb, h, w):
    """tensors 16-byte but not 256-byte aligned"""
    k = case(ops, dev, c, nb, h, w, offset=4)
    assert k["dy"].data_ptr() % 256 != 0 and k["dy"].data_ptr() % 16 == 0 and k["t2"].data_ptr() % 256 != 0
    assert torch.equal(k["fused"][0], k["pair"][0]) and torch.equal(k["fused"][1], k["pair"][1])
    k0 = case(ops, dev, c, nb, h, w)
    assert torch.equal(k["fused"][0], k0["fused"][0]) and torch.equal(k["fused"][1], k0["fused"][1]), "the same values at either place"


def worst(y, ref64, mag64):
    """largest error of an element relative to the sum of |a| |b| over its contraction"""
    return float(((y.double() - ref64).abs() / mag64).max())


@pytest.mark.parametrize("c,nb,h,w", SHAPES)
def test_c1wd_values_match_float64_like_the_pair(ops, dev, c, nb, h, w):
    k = case(ops, dev, c, nb, h, w)
    mid, hw = c // 4, h * w
    dy64 = k["dy"].double().view(nb, c, hw)
    a64 = activated64(k["t2"], k["st"].scale, k["st"].shift).view(nb, mid, hw)
    w64 = k["w3"].double().view(c, mid)
    ref_w = torch.einsum("ncp,nmp->cm", dy64, a64).view(c, mid, 1, 1)
    mag_w = torch.einsum("ncp,nmp->cm", dy64.abs(), a64.abs()).view(c, mid, 1, 1)
    ref_a = torch.einsum("cm,ncp->nmp", w64, dy64).view(nb, mid, h, w)
    mag_a = torch.einsum("cm,ncp->nmp", w64.abs(), dy64.abs()).view(nb, mid, h, w)
    for name, i, ref, mag in (("dW3", 0, ref_w, mag_w), ("dA3", 1, ref_a, mag_a)):
        e_f, e_p = worst(k["fused"][i], ref, mag), worst(k["pair"][i], ref, mag)
        print("c1wd %s C %d %dx%dx%d error / sum |a||b|: fused %.3e, pair %.3e" % (name, c, nb, h, w, e_f, e_p))
        assert e_f <= 1.5 * e_p + 1e-7, (name, e_f, e_p)


def test_c1wd_repeat_launches_are_bit_identical(ops, dev):
    for c, nb, h, w in SHAPES[:2]:
        k = case(ops, dev, c, nb, h, w)
        dw, da = fused(ops, k["dy"], k["t2"], k["st"], k["w3"])
        assert torch.equal(dw, k["fused"][0]) and torch.equal(da, k["fused"][1])


def test_c1wd_refuses_what_it_does_not_serve(ops, dev):
    """'not served' = None and nothing launched; the route then names the pair"""
    k = case(ops, dev, 128, 3, 16, 20)
    dy, t2, st, w3 = k["dy"], k["t2"], k["st"], k["w3"]
    dw = torch.full_like(w3, 7.0)
    assert ops.conv1x1_bwd_wd(dy, t2, None, w3, dw) is None, "a3 materialised: no prologue to rebuild"
    bf = torch.bfloat16
    assert ops.conv1x1_bwd_wd(dy.to(bf), t2.to(bf), st, w3, dw) is None, "bf16 storage"
    dy5, t5 = torch.zeros((1, 512, 8, 16), device=dev), torch.zeros((1, 128, 8, 16), device=dev)
    w5 = torch.zeros((512, 128, 1, 1), device=dev)
    assert ops.conv1x1_bwd_wd(dy5, t5, stats(ops, dev, 128, 5), w5, torch.empty_like(w5)) is None, "C = 512"
    big = 1 << 16
    assert ops.conv1x1_wd_route(512, 128, big) == "pair" and ops.conv1x1_wd_route(128, 32, big, "bf16") == "pair"
    assert ops.conv1x1_wd_route(128, 32, big) == "c1wd" and ops.conv1x1_wd_route(256, 64, big) == "c1wd"
    assert ops.C1WD_MIN_HW > 192 and ops.conv1x1_wd_route(128, 32, 192) == "pair"
    try:
        ops.set_c1wd(False)
        assert not ops.c1wd_enabled()
        assert ops.conv1x1_bwd_wd(dy, t2, st, w3, dw) is None and ops.conv1x1_wd_route(128, 32, big) == "pair"
    finally:
        ops.set_c1wd(True)
    torch.cuda.synchronize()
    assert bool((dw == 7.0).all()), "a refused call writes nothing"
    assert ops.conv1x1_bwd_wd(dy, t2, st, w3, dw) is not None


def test_c1wd_in_the_bottleneck_backward(ops, dev):
    """one Bottleneck(128) at the smallest routed pixel count, forward + backward with the switch on and off: every gradient with
    the same bits; the fused launch once with the switch on, the pair with it off"""
    from weatherforecastingtoolkit_amd import functional as Fn
    from weatherforecastingtoolkit_amd.pipeline.models.ae_64x8x8_lin import Bottleneck
    hw = ops.C1WD_MIN_HW
    h = 64
    assert hw % h == 0 and ops.conv1x1_wd_route(128, 32, hw) == "c1wd" and ops.conv1x1_wd_route(128, 32, hw - 64) == "pair"
    torch.manual_seed(0)
    blk = Bottleneck(128).to(dev).train()
    x0, gy = normal((2, 128, h, hw // h), 11, dev), normal((2, 128, h, hw // h), 12, dev)
    out = {}
    try:
        for on in (True, False):
            ops.set_c1wd(on)
            blk.zero_grad(set_to_none=True)
            x = x0.clone().requires_grad_(True)
            ops.profile_start()
            blk(x).backward(gy)
            Fn.join_side_stream()
            calls = {name: v[0] for name, v in ops.profile_stop().items()}
            out[on] = ([x.grad.clone()] + [p.grad.clone() for p in blk.parameters()], calls)
    finally:
        ops.set_c1wd(True)
    assert out[True][1].get("wfae_c1wd_bwd", 0) == 1 and "wfae_c1wd_bwd" not in out[False][1]
    assert out[False][1].get("wfae_conv1x1_bwd_weight_bnact", 0) == out[True][1].get("wfae_conv1x1_bwd_weight_bnact", 0) + 1
    assert out[False][1].get("wfae_conv1x1_bwd_data", 0) == out[True][1].get("wfae_conv1x1_bwd_data", 0) + 1
    assert len(out[True][0]) == len(out[False][0]) == 1 + len(list(blk.parameters()))
    for a, b in zip(out[True][0], out[False][0]):
        assert torch.equal(a, b)
