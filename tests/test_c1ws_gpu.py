"""csrc/c1ws.hip — the first 1x1 weight gradient dW1 = dT1 . gelu(bn1(x))^T and the sums of the first BatchNorm's backward
(sum dU, sum dU xhat with dU = (W1^T dT1) gelu'(bn1(x))) of a C <= 256 Bottleneck in ONE pass over x, against the pair of launches
it replaces: ops.conv1x1_bwd_weight_bnact on csrc/c1w.hip and the sums-alone ops.c1r_bnred(store=False).  The fused kernel repeats
c1w's operations per element of dW1 (the same MFMA instruction, the same position of every contraction index, the same order of the
six plane products, the same split-K slabs): dW1 keeps its bits.  Its sums add the SAME fp32 sums of four pixels (a bit-identical
dA1, bn_act_bwd_reduce_kernel's quad()) in fp64 in another order: the two totals differ by what two fp64 summations of the same n
terms can differ by, 2 (n - 1) 2^-53 sum |term| — a mis-addressed pixel misses that by ten orders of magnitude.

The wrapper ops.conv1x1_bwd_ws is called directly: the pixel threshold of ops.conv1x1_ws_route is not in the way."""
import math

import pytest
import torch

from tests._util import relerr

pytestmark = pytest.mark.gpu

# (C, NB, H, W): ten K-steps, five 64-pixel tiles and no multiple of 128 pixels; C = 256; HW = 832 is the smallest pixel count (a
# multiple of 64) at which c1w's chunking gives an image several chunks with a short last one; 40 images = 40 partial rows
SHAPES = [(128, 3, 16, 20), (256, 2, 24, 24), (128, 1, 26, 32), (128, 40, 16, 16)]


@pytest.fixture(scope="module")
def ops(dev):
    from weatherforecastingtoolkit_amd import ops as o
    assert o.c1ws_enabled()
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


def pair(ops, k, dw=None, accumulate=False):
    dw = torch.empty_like(k["w1"]) if dw is None else dw
    ops.conv1x1_bwd_weight_bnact(k["dt1"], k["x"], k["st"], dw, accumulate)
    none, sr = ops.c1r_bnred(k["w1"], k["dt1"], k["x"], k["st"], store=False)
    assert none is None
    return dw, sr


def fused(ops, k, dw=None, accumulate=False):
    dw = torch.empty_like(k["w1"]) if dw is None else dw
    sr = ops.conv1x1_bwd_ws(k["dt1"], k["x"], k["st"], k["w1"], dw, accumulate)
    assert sr is not None, "not served"
    return dw, sr


_cases = {}


def case(ops, dev, c, nb, h, w, offset=0):
    key = (c, nb, h, w, offset)
    if key not in _cases:
        mid = c // 4
        g = torch.Generator().manual_seed(5)
        k = dict(x=normal((nb, c, h, w), 1, dev, offset), dt1=normal((nb, mid, h, w), 2, dev, offset),
                 w1=(torch.randn((mid, c, 1, 1), generator=torch.Generator().manual_seed(3)) * 0.2).to(dev),
                 gamma=(torch.rand(c, generator=g) + 0.5).to(dev), beta=(torch.rand(c, generator=g) - 0.5).to(dev))
        # the statistics of x itself: mean and invstd belong to the tensor, u = gamma xhat + beta takes both signs
        k["st"] = ops.bn_stats_train(k["x"], k["gamma"], k["beta"], torch.zeros(c, device=dev), torch.ones(c, device=dev))
        k["pair"], k["fused"] = pair(ops, k), fused(ops, k)
        _cases[key] = k
    return _cases[key]


def totals(sr, c):
    """the partial rows added in fp64 on the host -> (sum dU [C], sum dU xhat [C])"""
    p = sr.part.cpu().view(2, sr.rows, c)
    return p[0].sum(0), p[1].sum(0)


def finish(ops, dev, sr, c):
    dg, db = torch.empty(c, device=dev), torch.empty(c, device=dev)
    ops.bn_act_bwd_from_rows(sr, c, dg, db)
    return dg, db


def restated64(k):
    """float64 restatement of the two sums and of the magnitudes their summation error scales with: dA1 in fp64 from the fp32
    operands, GELU' in fp64 of the fp32 value u, xhat the fp32 value -> (sum dU, sum dU xhat, sum |dU|, sum |dU xhat|), [C] each"""
    if "ref" not in k:
        x, st = k["x"].double(), k["st"]
        nb, c, h, w = x.shape
        v = lambda t: t.double().view(1, -1, 1, 1)
        u = (x * v(st.scale) + v(st.shift)).float().double()
        grad = 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
        xhat = ((k["x"] - st.mean.view(1, -1, 1, 1)) * st.invstd.view(1, -1, 1, 1)).double()
        da = torch.einsum("mc,nmp->ncp", k["w1"].double().view(c // 4, c), k["dt1"].double().view(nb, c // 4, h * w)).view(nb, c, h, w)
        du = da * grad
        red = lambda t: t.sum((0, 2, 3)).cpu()
        k["ref"] = (red(du), red(du * xhat), red(du.abs()), red((du * xhat).abs()))
    return k["ref"]


@pytest.mark.parametrize("c,nb,h,w", SHAPES)
def test_c1ws_dw1_keeps_the_bits_of_c1w(ops, dev, c, nb, h, w):
    k = case(ops, dev, c, nb, h, w)
    dw_p, dw_f = k["pair"][0], k["fused"][0]
    assert torch.equal(dw_f, dw_p), "dW1: %g" % float((dw_f - dw_p).abs().max())
    # accumulating into a gradient that is already there
    base = torch.full_like(k["w1"], 0.75)
    dw_pa, _ = pair(ops, k, base.clone(), True)
    dw_fa, _ = fused(ops, k, base.clone(), True)
    assert torch.equal(dw_fa, dw_pa) and not torch.equal(dw_fa, dw_p)


@pytest.mark.parametrize("c,nb,h,w", SHAPES)
def test_c1ws_sums_are_the_sums_of_the_pair(ops, dev, c, nb, h, w):
    k = case(ops, dev, c, nb, h, w)
    sr_p, sr_f = k["pair"][1], k["fused"][1]
    assert sr_f.part.numel() == 2 * sr_f.rows * c
    (dg_p, db_p), (dg_f, db_f) = finish(ops, dev, sr_p, c), finish(ops, dev, sr_f, c)
    e_g, e_b = relerr(dg_f, dg_p), relerr(db_f, db_p)
    print("c1ws C %d %dx%dx%d dgamma relerr %.3e, dbeta relerr %.3e" % (c, nb, h, w, e_g, e_b))
    assert e_g < 1e-6 and e_b < 1e-6
    # both forms are fp64 summations of the same n fp32 quads per channel
    n = nb * h * w // 4
    ref1, ref2, mag1, mag2 = restated64(k)
    for name, t_f, t_p, ref, mag in zip(("sum dU", "sum dU xhat"), totals(sr_f, c), totals(sr_p, c), (ref1, ref2), (mag1, mag2)):
        bound = 2.0 * (n - 1) * 2.0 ** -53 * mag
        d = (t_f - t_p).abs()
        e_f, e_p = (t_f - ref).abs(), (t_p - ref).abs()
        print("c1ws %s C %d %dx%dx%d: |fused - pair| / bound %.3e; error to float64 / sum |term|: fused %.3e, pair %.3e"
              % (name, c, nb, h, w, float((d / bound).max()), float((e_f / mag).max()), float((e_p / mag).max())))
        assert bool((d <= bound).all()), (name, float((d / bound).max()))
        assert bool((e_f <= e_p + bound).all()), (name, float(((e_f - e_p) / bound).max()))


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("c,nb,h,w", SHAPES)
def test_c1ws_dx_through_the_whole_sequence(ops, dev, c, nb, h, w, skip):
    """fused -> from_rows -> c1r_bndx against today's c1r_bnred(store=False) -> from_rows -> c1r_bndx on the same tensors"""
    k = case(ops, dev, c, nb, h, w)
    res = normal((nb, c, h, w), 7, dev) if skip else None
    out = []
    for sr in (k["pair"][1], k["fused"][1]):
        dg, db = finish(ops, dev, sr, c)     # the coefficients at the head of the workspace, read by c1r_bndx next
        out.append(ops.c1r_bndx(k["w1"], k["dt1"], k["x"], k["gamma"], k["st"], res, True))
    e = relerr(out[1], out[0])
    print("c1ws dx C %d %dx%dx%d skip %d relerr %.3e" % (c, nb, h, w, skip, e))
    assert e < 1e-6


@pytest.mark.parametrize("c,nb,h,w", SHAPES[:2])
def test_c1ws_at_a_storage_offset(ops, dev, c, nb, h, w):
    """tensors 16-byte but not 256-byte aligned"""
    k = case(ops, dev, c, nb, h, w, offset=4)
    assert k["x"].data_ptr() % 256 != 0 and k["x"].data_ptr() % 16 == 0 and k["dt1"].data_ptr() % 256 != 0
    assert torch.equal(k["fused"][0], k["pair"][0])
    k0 = case(ops, dev, c, nb, h, w)
    assert torch.equal(k["fused"][0], k0["fused"][0]), "the same values at either place"
    assert k["fused"][1].rows == k0["fused"][1].rows and torch.equal(k["fused"][1].part, k0["fused"][1].part)
    for t_f, t_p, mag in zip(totals(k["fused"][1], c), totals(k["pair"][1], c), restated64(k)[2:]):
        assert bool(((t_f - t_p).abs() <= 2.0 * (nb * h * w // 4 - 1) * 2.0 ** -53 * mag).all())


def test_c1ws_repeat_launches_are_bit_identical(ops, dev):
    for c, nb, h, w in SHAPES[:2]:
        k = case(ops, dev, c, nb, h, w)
        dw, sr = fused(ops, k)
        assert torch.equal(dw, k["fused"][0]) and sr.rows == k["fused"][1].rows and torch.equal(sr.part, k["fused"][1].part)


def test_c1ws_refuses_what_it_does_not_serve(ops, dev):
    """'not served' = None and nothing launched; the route then names the pair"""
    k = case(ops, dev, 128, 3, 16, 20)
    dt1, x, st, w1 = k["dt1"], k["x"], k["st"], k["w1"]
    dw = torch.full_like(w1, 7.0)
    z = lambda *s: torch.zeros(s, device=dev)
    assert ops.conv1x1_bwd_ws(dt1, x, None, w1, dw) is None, "a1 materialised: no prologue to rebuild"
    assert ops.conv1x1_bwd_ws(z(1, 64, 8, 16), z(1, 128, 8, 16), st, z(64, 128, 1, 1), z(64, 128, 1, 1)) is None, "mid != C / 4"
    assert ops.conv1x1_bwd_ws(z(1, 128, 8, 16), z(1, 512, 8, 16), ops.BnStats(512, dev), z(128, 512, 1, 1), z(128, 512, 1, 1)) is None, "C = 512"
    assert ops.conv1x1_bwd_ws(z(1, 32, 8, 12), z(1, 128, 8, 12), st, w1, dw) is None, "HW % 64 != 0"
    bf = torch.bfloat16
    assert ops.conv1x1_bwd_ws(dt1.to(bf), x.to(bf), st, w1, dw) is None, "bf16 storage"
    big = 1 << 16
    assert ops.conv1x1_ws_route(128, 32, big) == "c1ws" and ops.conv1x1_ws_route(256, 64, big) == "c1ws"
    assert ops.conv1x1_ws_route(128, 64, big) == "pair" and ops.conv1x1_ws_route(512, 128, big) == "pair"
    assert ops.conv1x1_ws_route(128, 32, big + 32) == "pair" and ops.conv1x1_ws_route(128, 32, big, "bf16") == "pair"
    assert ops.C1WD_MIN_HW == 512 and ops.conv1x1_ws_route(128, 32, 512) == "c1ws"
    assert ops.conv1x1_ws_route(128, 32, 448) == "pair" and ops.conv1x1_ws_route(128, 32, 192) == "pair"
    try:
        ops.set_c1ws(False)
        assert not ops.c1ws_enabled()
        assert ops.conv1x1_bwd_ws(dt1, x, st, w1, dw) is None and ops.conv1x1_ws_route(128, 32, big) == "pair"
    finally:
        ops.set_c1ws(True)
    torch.cuda.synchronize()
    assert bool((dw == 7.0).all()), "a refused call writes nothing"
    assert ops.conv1x1_bwd_ws(dt1, x, st, w1, dw) is not None


def test_c1ws_in_the_bottleneck_backward(ops, dev):
    """one Bottleneck(128) at the smallest routed pixel count, forward + backward with the switch on and off: dW1 with the same
    bits, every other gradient to the rounding of the two sums; the fused launch once with the switch on, the pair with it off"""
    from weatherforecastingtoolkit_amd import functional as Fn
    from weatherforecastingtoolkit_amd.pipeline.models.ae_64x8x8_lin import Bottleneck
    hw = ops.C1WD_MIN_HW
    h = 64
    assert hw % h == 0 and ops.conv1x1_ws_route(128, 32, hw) == "c1ws" and ops.conv1x1_ws_route(128, 32, hw - 64) == "pair"
    torch.manual_seed(0)
    blk = Bottleneck(128).to(dev).train()
    x0, gy = normal((2, 128, h, hw // h), 11, dev), normal((2, 128, h, hw // h), 12, dev)
    w1 = blk.f[2].weight
    assert tuple(w1.shape[:2]) == (32, 128)
    out = {}
    try:
        for on in (True, False):
            ops.set_c1ws(on)
            blk.zero_grad(set_to_none=True)
            x = x0.clone().requires_grad_(True)
            ops.profile_start()
            blk(x).backward(gy)
            Fn.join_side_stream()
            calls = {name: v[0] for name, v in ops.profile_stop().items()}
            out[on] = (w1.grad.clone(), [x.grad.clone()] + [p.grad.clone() for p in blk.parameters()], calls)
    finally:
        ops.set_c1ws(True)
    assert out[True][2].get("wfae_c1ws_bwd", 0) == 1 and "wfae_c1ws_bwd" not in out[False][2]
    assert out[False][2].get("wfae_conv1x1_bwd_weight_bnact", 0) == out[True][2].get("wfae_conv1x1_bwd_weight_bnact", 0) + 1
    assert out[False][2].get("wfae_conv1x1_bwd_data", 0) == out[True][2].get("wfae_conv1x1_bwd_data", 0) + 1   # the sums alone
    assert torch.equal(out[True][0], out[False][0]), "dW1"
    assert len(out[True][1]) == len(out[False][1]) == 1 + len(list(blk.parameters()))
    for a, b in zip(out[True][1], out[False][1]):
        assert relerr(a, b) < 1e-6
