"""GPU: the fp32 glue kernels of csrc/norm_act.hip called through the C ABI (element-wise helpers, wfae_scale, wfae_pad2d,
wfae_reduce_sum, the fp32 <-> bf16 converters) at odd sizes, from misaligned views, past the block caps of their grids and
in place: bitwise against the fp32 formula where there is one, per element within the bounds of tests/optim_ref.py
otherwise.  Prints `optim_fp64 <kernel> <case> <largest error as a fraction of its bound>` lines like
tests/test_optim_gpu.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import optim_ref as R
from tests.optim_ref import bits, report, worst

pytestmark = pytest.mark.gpu

f32 = np.float32
SENTINEL = 123.0
EW_SIZES = [1, 2, 3, 5, 1027, 4194304 + 1027]   # the last: past the 4096-block cap of launch_ew, grid-stride path
LEAKY = f32(0.2)


@pytest.fixture(scope="module")
def ops(dev):
    from weatherforecastingtoolkit_amd import ops as o
    return o


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def placed(arr, dev, offset):
    """the array on the device inside a sentinel-filled buffer, starting `offset` elements in (offset 0: 16-byte aligned,
    offset 1: not)"""
    n = len(arr)
    buf = torch.full((n + offset + 3,), SENTINEL, device=dev)
    view = buf[offset:offset + n]
    view.copy_(torch.from_numpy(np.ascontiguousarray(arr)))
    assert (view.data_ptr() % 16 == 0) == (offset % 4 == 0)
    return buf, view


def launch_ew(name, a, b, out):
    from weatherforecastingtoolkit_amd import _lib
    st = torch.cuda.current_stream().cuda_stream
    if b is None:
        _lib.call("wfae_" + name, a.data_ptr(), out.data_ptr(), a.numel(), st)
    else:
        _lib.call("wfae_" + name, a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), st)


def ew_inputs(name, n, seed):
    r = np.random.default_rng(seed)
    if name == "sigmoid_fwd":
        x = r.uniform(-30, 30, n).astype(f32)
        if n >= 16:
            x[3:9] = [88.0, -88.0, 104.0, -104.0, 0.0, -0.0]
        return x, None
    if name == "gelu_fwd":
        return r.uniform(-9, 9, n).astype(f32), None
    if name == "gelu_bwd":
        return r.uniform(-2, 2, n).astype(f32), r.uniform(-9, 9, n).astype(f32)
    if name == "sigmoid_bwd":
        return r.standard_normal(n).astype(f32), r.uniform(0, 1, n).astype(f32)
    a, b = r.standard_normal(n).astype(f32), r.standard_normal(n).astype(f32)
    if n >= 16:   # the branch of the leaky kernels at both zeros
        a[2:4] = [0.0, -0.0]
        b[4:6] = [0.0, -0.0]
    return a, (None if name == "leaky_relu_fwd" else b)


def ew_check(name, a, b, got):
    """bitwise kernels: True / False; the others: the largest error as a fraction of its bound"""
    if name == "add":
        return same_bits(got, a + b)
    if name == "leaky_relu_fwd":
        return same_bits(got, np.where(a > 0, a, LEAKY * a))
    if name == "leaky_relu_bwd":
        return same_bits(got, np.where(b > 0, a, LEAKY * a))
    if name == "sigmoid_bwd":
        return same_bits(got, a * b * (f32(1.0) - b))
    if name == "sigmoid_fwd":
        return worst(got, *R.sigmoid_bound(a))
    if name == "gelu_fwd":
        return worst(got, *R.gelu_bounds(a))
    return worst(got, *R.gelu_bwd_bounds(a, b))


@pytest.mark.parametrize("name", ["gelu_fwd", "gelu_bwd", "sigmoid_fwd", "sigmoid_bwd", "leaky_relu_fwd", "leaky_relu_bwd", "add"])
def test_elementwise_sizes_and_alignments(ops, dev, name):
    """every size from aligned buffers (vector path) and with a, b and out in turn one element off (scalar path): the same
    bits each time, nothing written outside the n elements, and the aligned result against the reference"""
    for n in EW_SIZES:
        a, b = ew_inputs(name, n, n % 1000)
        variants = [(0, 0, 0), (1, 0, 0), (0, 0, 1)] + ([(0, 1, 0)] if b is not None else [])
        first = None
        for oa, ob, oo in variants:
            _, av = placed(a, dev, oa)
            bv = None if b is None else placed(b, dev, ob)[1]
            obuf, ov = placed(np.full(n, SENTINEL, f32), dev, oo)
            launch_ew(name, av, bv, ov)
            torch.cuda.synchronize()
            got = ov.cpu().numpy()
            assert bool((obuf[:oo] == SENTINEL).all()) and bool((obuf[oo + n:] == SENTINEL).all()), (n, oa, ob, oo)
            assert same_bits(av.cpu().numpy(), a) and (b is None or same_bits(bv.cpu().numpy(), b))
            if first is None:
                first = got
                res = ew_check(name, a, b, got)
                if res is True or res is False:
                    assert res, (name, n, "differs from the fp32 formula")
                else:
                    report(name, f"n={n}", res)
                    assert res <= 1.0, (name, n, res)
            else:
                assert same_bits(got, first), (name, n, (oa, ob, oo), "scalar path differs from the vector path")
        # in place: out is a
        _, av = placed(a, dev, 0)
        bv = None if b is None else placed(b, dev, 0)[1]
        launch_ew(name, av, bv, av)
        assert same_bits(av.cpu().numpy(), first), (name, n, "in place")


def test_sigmoid_propagates_nan(ops, dev):
    x = torch.tensor([0.5, float("nan"), -1.0, float("nan"), 2.0], device=dev)
    for xv in (x, placed(x.cpu().numpy(), dev, 1)[1]):
        y = ops.sigmoid_fwd(xv).cpu().numpy()
        assert np.array_equal(np.isnan(y), [False, True, False, True, False])


@pytest.mark.parametrize("n", [1, 3, 1027, 4194304 + 1027])
def test_scale_bitwise(ops, dev, n):
    r = np.random.default_rng(n)
    x = r.standard_normal(n).astype(f32)
    sd = f32(0.3)
    xd, sdev = torch.from_numpy(x).to(dev), torch.tensor([float(sd), SENTINEL], device=dev)
    for s, dev_factor, f in ((0.7, None, f32(0.7)), (0.7, sdev[0:1], sd * f32(0.7)), (1.0, sdev[0:1], sd)):
        want = x * f
        out = ops.scale(xd, s, dev_factor)
        assert same_bits(out.cpu().numpy(), want), (n, s)
        for offset in (0, 1):   # in place, also from a view that is not 16-byte aligned
            buf, v = placed(x, dev, offset)
            ops.scale(v, s, dev_factor, out=v)
            assert same_bits(v.cpu().numpy(), want) and bool((buf[:offset] == SENTINEL).all()) and bool((buf[offset + n:] == SENTINEL).all())
    assert same_bits(xd.cpu().numpy(), x)


@pytest.mark.parametrize("shape,pad", [((2, 3, 7, 9), 0), ((2, 3, 7, 9), 1), ((2, 3, 7, 9), 2), ((2, 3, 7, 9), 5),
                                       ((1, 5, 500, 440), 2)])
def test_pad_and_crop_bitwise(ops, dev, shape, pad):
    """(1, 5, 500, 440) has more than 1 048 576 elements with and without the border: grid_1d(total, 1) is capped and
    the loop strides"""
    g = torch.Generator().manual_seed(pad)
    x = torch.randn(shape, generator=g)
    x.view(-1)[:3] = torch.tensor([float("nan"), -0.0, float("inf")])
    xd = x.to(dev)
    y = ops.pad2d(xd, pad)
    want = F.pad(x, (pad, pad, pad, pad))
    assert y.shape == want.shape and same_bits(y.cpu().numpy(), want.numpy())
    back = ops.crop2d(y, pad)
    assert back.shape == x.shape and same_bits(back.cpu().numpy(), x.numpy())
    if pad:   # a crop of something that is not zero outside
        z = torch.randn(want.shape, generator=g)
        assert same_bits(ops.crop2d(z.to(dev), pad).cpu().numpy(), z[:, :, pad:-pad, pad:-pad].contiguous().numpy())


# ------------------------------------------------------------- reduce_sum ---
@pytest.mark.parametrize("outer", [1, 63, 64, 65, 1000, 65600])
def test_reduce_sum_columns(ops, dev, outer):
    """inner == 1: colsum_kernel with one split, a partial last split, several, and past its cap of 1024 (65 600 rows);
    column blocks of 64 with C below, at and above one and two blocks.  Data 1e3 + noise: an fp32 accumulator would show."""
    r = np.random.default_rng(outer)
    for c in (1, 63, 64, 65, 130):
        x = (1e3 + r.standard_normal((outer, c))).astype(f32)
        base = r.standard_normal(c).astype(f32) * f32(100.0)
        xd = torch.from_numpy(x).to(dev)
        for accumulate in (False, True):
            out = torch.from_numpy(base).to(dev) if accumulate else torch.full((c,), float("nan"), device=dev)
            ops.reduce_sum(xd, outer, c, 1, out, accumulate=accumulate)
            S, b = R.reduce_sum_bound(x, 0, vector=False, accumulate_onto=base if accumulate else None)
            ratio = worst(out.cpu().numpy(), S, b)
            report("reduce_sum inner=1", f"outer={outer} C={c} accumulate={int(accumulate)}", ratio)
            assert ratio <= 1.0, (outer, c, accumulate, ratio)


@pytest.mark.parametrize("inner,offset", [(1155, 0), (1156, 0), (1156, 1)], ids=["scalar", "vector", "vector_size_misaligned"])
def test_reduce_sum_channels(ops, dev, inner, offset):
    outer, c = 3, 7
    r = np.random.default_rng(inner + offset)
    x = (1e3 + r.standard_normal((outer, c, inner))).astype(f32)
    _, xv = placed(x.ravel(), dev, offset)
    vector = inner % 4 == 0 and offset == 0
    base = r.standard_normal(c).astype(f32) * f32(100.0)
    for accumulate in (False, True):
        out = torch.from_numpy(base).to(dev) if accumulate else torch.full((c,), float("nan"), device=dev)
        ops.reduce_sum(xv, outer, c, inner, out, accumulate=accumulate)
        S, b = R.reduce_sum_bound(x, (0, 2), vector=vector, accumulate_onto=base if accumulate else None)
        ratio = worst(out.cpu().numpy(), S, b)
        report("reduce_sum channels", f"inner={inner} offset={offset} accumulate={int(accumulate)}", ratio)
        assert ratio <= 1.0, (inner, offset, accumulate, ratio)


# -------------------------------------------------------------- converters ---
SPECIAL_BITS = np.array([
    0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001,   # +-0, +-inf, NaNs
    0x00000001, 0x807FFFFF, 0x00008000, 0x00018000, 0x00400000,                          # subnormals (two of them ties)
    0x7F7FFFFF, 0xFF7FFFFF,                                                              # largest finite: rounds to inf
    0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,                                      # ties: even / odd upper half
    0x3F808001, 0x3F807FFF, 0x3F80FFFF, 0x00800000, 0x007F8000,                          # either side of a tie, carries
], dtype=np.uint32)


def bf16_rne_bits(u):
    """round-to-nearest-even of fp32 bit patterns to bf16 in integer arithmetic; NaN positions are returned apart"""
    u = u.astype(np.uint64)
    nan = ((u & 0x7F800000) == 0x7F800000) & ((u & 0x007FFFFF) != 0)
    out = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return out, nan


@pytest.mark.parametrize("n", [4096, 1027, 2055], ids=["n%8=0", "n%8=3", "n%8=7"])
def test_converters_bit_patterns(ops, dev, n):
    r = np.random.default_rng(n)
    u = r.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    u[:len(SPECIAL_BITS)] = SPECIAL_BITS
    u[-len(SPECIAL_BITS):] = SPECIAL_BITS[::-1]          # the specials in the scalar tail too
    x = torch.from_numpy(u.view(f32).copy()).to(dev)
    got = ops.to_bf16(x).view(torch.int16).cpu().numpy().view(np.uint16)
    want, nan = bf16_rne_bits(u)
    assert np.array_equal(got[~nan], want[~nan]), np.flatnonzero((got != want) & ~nan)[:8]
    gn = got[nan]
    assert bool(((gn & 0x7F80) == 0x7F80).all() and ((gn & 0x007F) != 0).all()), "a NaN must stay a NaN"
    assert np.array_equal(gn >> 15, (u[nan] >> 31).astype(np.uint16))
    # and back: exact, NaN payloads included
    h = r.integers(0, 2 ** 16, n, dtype=np.uint64).astype(np.uint16)
    h[:len(SPECIAL_BITS)] = (SPECIAL_BITS >> 16).astype(np.uint16)
    hb = torch.from_numpy(h.view(np.int16).copy()).to(dev).view(torch.bfloat16)
    back = ops.to_f32(hb).cpu().numpy().view(np.uint32)
    assert np.array_equal(back, h.astype(np.uint32) << 16)
