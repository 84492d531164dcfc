"""csrc/c1n.hip — the narrowing 1x1 products of the C >= 512 Bottleneck stages ((M, K) = (128, 512) and (256, 1024): the C -> C/4
forward behind the BatchNorm + GELU prologue, and the C -> C/4 data gradient with the weight read transposed), routed inside
the library from wfae_conv1x1_fwd_bnact / wfae_conv1x1_bwd_data.  Both operands are split into their bf16 planes once, on
their way into LDS; `ops.set_c1n(False)` keeps the shapes on gemm.hip's in-register split, the kernel they ran on before.

The multiply side repeats the old kernel's operations per output element, so at the step's sizes the results keep their bits.

Against float64 on the same fp32 inputs, under the bar of tests/test_split_gemm_gpu.py (the error of the new kernel within
1.5x of the old one's plus 1e-7 of the result's rms), on grids with an edge tile in every image, on the persistent launch,
with the BatchNorm sums of the epilogue under the float64 bounds of tests/test_bn_chain_gpu.py."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests._util import relerr
from tests.test_bn_chain_gpu import Affine, check_stats, conv_input, conv_weight, ratios

pytestmark = pytest.mark.gpu

MK = [(128, 512), (256, 1024)]           # the routed shapes: 128 rows x 256 columns and 256 rows x 128 columns per block
COLS = {128: 256, 256: 128}
# an edge tile in every image (576 = 4.5 tiles of 128 = 2.25 of 256); exactly one tile of 128 (half a tile of 256)
GRIDS = [(3, 24, 24), (2, 8, 16)]


@pytest.fixture(scope="module")
def ops(dev):
    from weatherforecastingtoolkit_amd import ops as o
    assert o.c1n_enabled()
    return o


def rnd(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * (hi - lo) + lo).float()


def activated64(x, scale, shift):
    """float64 GELU of the fp32 value u = fma(x, scale, shift) the kernels evaluate (the fp64 product of two fp32 values is
    exact, so the fp64 sum rounded to fp32 is the fma)"""
    u = (x.double() * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)).float().double()
    return 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))


def old_and_new(ops, fn):
    ops.set_c1n(False)
    try:
        old = fn()
    finally:
        ops.set_c1n(True)
    return old, fn()


def err_rms(y, ref64):
    return float((y.double() - ref64).abs().max()) / float(ref64.pow(2).mean().sqrt())


def under_the_bar(new, old, ref64, what, differs=True):
    e_new, e_old = err_rms(new, ref64), err_rms(old, ref64)
    print("c1n %-40s error / rms: new %.3e, gemm.hip %.3e" % (what, e_new, e_old))
    assert e_new <= 1.5 * e_old + 1e-7, (what, e_new, e_old)
    if differs:
        assert not torch.equal(new, old), "c1n did not run (same bits as gemm.hip): %s" % (what,)


def prologue_stats(ops, dev, k, seed):
    st = ops.BnStats(k, dev)
    st.scale.copy_(rnd((k,), seed, 0.5, 1.5))
    st.shift.copy_(rnd((k,), seed + 1, -0.5, 0.5))
    return st


_cases = {}


def case(ops, dev, m, k, nb, h, w):
    """inputs, both launches on both kernels and the float64 references of one shape, computed once for the tests that share them"""
    key = (m, k, nb, h, w)
    if key not in _cases:
        x = rnd((nb, k, h, w), 1, -2.0, 2.0).to(dev)
        wt = rnd((m, k, 1, 1), 2, -0.3, 0.3).to(dev)            # forward weight (Cout = m, Cin = k), read row-major
        wt_t = rnd((k, m, 1, 1), 3, -0.3, 0.3).to(dev)          # (Cout = k, Cin = m): its data gradient reads it transposed
        st = prologue_stats(ops, dev, k, 4)
        ref_f = F.conv2d(activated64(x.cpu(), st.scale.cpu(), st.shift.cpu()), wt.double().cpu()).to(dev)
        ref_d = F.conv_transpose2d(x.double().cpu(), wt_t.double().cpu()).to(dev)
        fwd = old_and_new(ops, lambda: ops.conv1x1_fwd_bnact(x, st, wt, stats=True))
        dgr = old_and_new(ops, lambda: ops.conv1x1_bwd_data(x, wt_t))
        _cases[key] = dict(x=x, wt=wt, wt_t=wt_t, st=st, ref_f=ref_f, ref_d=ref_d, fwd=fwd, dgr=dgr)
    return _cases[key]


@pytest.mark.parametrize("nb,h,w", GRIDS)
@pytest.mark.parametrize("m,k", MK)
def test_c1n_values_match_fp64_like_the_in_register_split(ops, dev, m, k, nb, h, w):
    c = case(ops, dev, m, k, nb, h, w)
    (y_old, _), (y_new, sr) = c["fwd"]
    assert sr is not None and sr.rows == nb * -(-(h * w) // COLS[m]), "one partial row per block"
    under_the_bar(y_new, y_old, c["ref_f"], "forward + prologue (%d, %d) %dx%dx%d" % (m, k, nb, h, w))
    under_the_bar(c["dgr"][1], c["dgr"][0], c["ref_d"], "data gradient (%d, %d) %dx%dx%d" % (m, k, nb, h, w))
    # the forms without sums / without prologue run the same arithmetic
    assert torch.equal(ops.conv1x1_fwd_bnact(c["x"], c["st"], c["wt"]), y_new)
    a = ops.bn_act_fwd(c["x"], c["st"], 1)
    assert torch.equal(ops.conv1x1_fwd(a, c["wt"]), y_new), "the prologue is bn_act_fwd's arithmetic, bit for bit"


@pytest.mark.parametrize("m,k", MK)
def test_c1n_persistent_launch(ops, dev, m, k):
    """just more items than the chip has CUs (rounded up to the 8 XCDs), HW no multiple of the column tile: workgroups walk
    several items, the loader fetches a workgroup's next tile under the last K-steps of the current one.  On grids of this size
    gemm.hip runs its in-register split, whose operations c1n repeats product for product (the same MFMA instruction, k
    placement, order of the six plane products and of the 16-deep slabs): every element must come out with the same bits —
    a tile fetched or stored wrongly cannot hide in a tolerance.  (The small grids of the value test run gemm.hip's fp32-MFMA
    kernel with the switch off: there the results differ, which is what shows that c1n ran.)"""
    cus = (torch.cuda.get_device_properties(dev).multi_processor_count + 7) // 8 * 8
    h, w = (120, 112) if COLS[m] == 256 else (56, 72)       # 52.5 tiles of 256; 31.5 tiles of 128
    tpi = -(-(h * w) // COLS[m])
    nb = cus // tpi + 1
    assert nb * tpi > cus and (h * w) % COLS[m] != 0 and (nb - 1) * tpi <= cus
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.rand((nb, k, h, w), generator=g, device=dev) * 4.0 - 2.0
    wt = rnd((m, k, 1, 1), 6, -0.3, 0.3).to(dev)
    wt_t = rnd((k, m, 1, 1), 7, -0.3, 0.3).to(dev)
    st = prologue_stats(ops, dev, k, 8)
    (y_old, sr_old), (y_new, sr) = old_and_new(ops, lambda: ops.conv1x1_fwd_bnact(x, st, wt, stats=True))
    assert sr is not None and sr.rows == cus, "one workgroup per CU, one partial row each"
    a64 = activated64(x, st.scale, st.shift).view(nb, k, h * w)
    under_the_bar(y_new, y_old, (wt.double().view(m, k) @ a64).view(nb, m, h, w), "persistent forward + prologue (%d, %d)" % (m, k), differs=False)
    assert torch.equal(y_new, y_old), "every element, the edge tile of every image included"
    del a64
    # the rows of a grid in which every workgroup accumulates several items (and, with fewer items than 8 ceil(items / 8),
    # some none at all), under the same float64 bounds
    aff = Affine(m, dev)
    check_stats(y_new, ops.bn_stats_from_rows(sr, tuple(y_new.shape), *aff.args), aff, None, True)
    d_old, d_new = old_and_new(ops, lambda: ops.conv1x1_bwd_data(x, wt_t))
    ref_d = (wt_t.double().view(k, m).t() @ x.double().view(nb, k, h * w)).view(nb, m, h, w)
    under_the_bar(d_new, d_old, ref_d, "persistent data gradient (%d, %d)" % (m, k), differs=False)
    assert torch.equal(d_new, d_old)


@pytest.mark.parametrize("nb,h,w", GRIDS)
@pytest.mark.parametrize("m,k", MK)
def test_c1n_batchnorm_sums_match_float64(ops, dev, m, k, nb, h, w):
    """the finished statistics of the epilogue's rows under the float64 bounds every other producer of BatchNorm sums meets,
    evaluated on the tensor the kernel stored; 576 pixels: the columns the loader clamped at each image's edge stay out.
    Inputs and weights of tests/test_bn_chain_gpu.py: output channels far from zero in units of their spread"""
    x, st_in = conv_input((nb, k, h, w), 33, True, dev, ops)
    x = x.to(dev)
    wt = conv_weight(m, k, 34).to(dev)
    (y_old, _), (y, sr) = old_and_new(ops, lambda: ops.conv1x1_fwd_bnact(x, st_in, wt, stats=True))
    assert sr is not None and not torch.equal(y, y_old), "c1n did not run"
    print("c1n sums (%d, %d) %dx%dx%d: largest |mean| / sigma %.1f" % (m, k, nb, h, w, max(ratios(y))))
    aff = Affine(m, dev)
    check_stats(y, ops.bn_stats_from_rows(sr, tuple(y.shape), *aff.args), aff, None, True)
    # the epilogue takes its fp32 sums over the same quads of adjacent pixels as the statistics pass: the two agree to rounding
    a2 = Affine(m, dev)
    s_sep = ops.bn_stats_train(y, *a2.args)
    s_epi = ops.bn_stats_from_rows(sr, tuple(y.shape), *Affine(m, dev).args)
    for name in ("mean", "invstd", "scale", "shift"):
        assert relerr(getattr(s_epi, name), getattr(s_sep, name)) < 2e-7, name
    # and on the uniform inputs of the value test
    c = case(ops, dev, m, k, nb, h, w)
    y, sr = c["fwd"][1]
    aff = Affine(m, dev)
    check_stats(y, ops.bn_stats_from_rows(sr, tuple(y.shape), *aff.args), aff, None, True)


def test_c1n_refuses_what_it_does_not_serve(ops, dev):
    """outside the routing condition the switch changes nothing: the same bits on and off"""
    m, k, nb = 128, 512, 2
    x = rnd((nb, k, 8, 16), 11, -2.0, 2.0).to(dev)
    wt = rnd((m, k, 1, 1), 12, -0.3, 0.3).to(dev)
    st = prologue_stats(ops, dev, k, 13)
    bias, res = rnd((m,), 14).to(dev), rnd((nb, m, 8, 16), 15).to(dev)
    x6 = rnd((nb, k, 6, 6), 16, -2.0, 2.0).to(dev)              # HW = 36: a multiple of 4, not of 8
    xs = rnd((nb, 256, 8, 16), 17, -2.0, 2.0).to(dev)           # (M, K) = (64, 256)
    ws, sts = rnd((64, 256, 1, 1), 18, -0.3, 0.3).to(dev), prologue_stats(ops, dev, 256, 19)
    ws_t = rnd((256, 64, 1, 1), 20, -0.3, 0.3).to(dev)
    wt_t = rnd((k, m, 1, 1), 21, -0.3, 0.3).to(dev)
    forms = {"bias": lambda: ops.conv1x1_fwd_bnact(x, st, wt, bias, None),
             "residual": lambda: ops.conv1x1_fwd_bnact(x, st, wt, None, res),
             "HW % 8, forward": lambda: ops.conv1x1_fwd_bnact(x6, st, wt),
             "HW % 8, data gradient": lambda: ops.conv1x1_bwd_data(x6, wt_t),
             "(64, 256), forward": lambda: ops.conv1x1_fwd_bnact(xs, sts, ws),
             "(64, 256), data gradient": lambda: ops.conv1x1_bwd_data(xs, ws_t)}
    for name, fn in forms.items():
        old, new = old_and_new(ops, fn)
        assert torch.equal(old, new), name
    # and the served form of the same tensors does change kernels
    old, new = old_and_new(ops, lambda: ops.conv1x1_fwd_bnact(x, st, wt))
    assert not torch.equal(old, new)


def test_c1n_repeat_launches_are_bit_identical(ops, dev):
    """20 identical launches of the prologue form with sums: fixed item -> workgroup assignment, no atomics, and the GELU's
    branch-free select (common.h) — one run, the same bits every time"""
    c = case(ops, dev, 256, 1024, 3, 24, 24)
    y0, sr0 = c["fwd"][1]
    for _ in range(20):
        y, sr = ops.conv1x1_fwd_bnact(c["x"], c["st"], c["wt"], stats=True)
        assert torch.equal(y, y0) and torch.equal(sr.part[:2 * sr.rows * 256], sr0.part[:2 * sr0.rows * 256])
