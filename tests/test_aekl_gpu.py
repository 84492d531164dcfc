"""GPU: the frozen AutoencoderKL latent provider (csrc/aekl.hip, pipeline/models/autoencoderkl) — the 3x3 matrix-core
convolution in its three forms, GroupNorm statistics, the attention pieces and the posterior kernel against torch on the
CPU; the whole model against the reference's recorded fp64 values (tests/golden/g14_aekl.npz); bitwise repeatability,
chunking, the launch budget and the experiment.

Tolerances.  Every comparison is against fp64 values in the measure max|a - b| / max|b|, the measure of
tests/test_convae_gpu.py.  The bound of a tensor is max(4 x spread, 2e-6), spread = the same measure between an fp32 and
an fp64 run of torch on the CPU (recorded in the fixture with the reference module, or measured inside the test): the
reference's own arithmetic noise, times the project's factor of 4 for a different summation order."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import aekl_ref as A
from tests import convae_ref as R
from weatherforecastingtoolkit_amd import config as C
from weatherforecastingtoolkit_amd import functional as Fn
from weatherforecastingtoolkit_amd import ops
from weatherforecastingtoolkit_amd._lib import WfaeError
from weatherforecastingtoolkit_amd.pipeline.models.autoencoderkl import AutoencoderKL

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G14 = os.path.join(HERE, "golden", "g14_aekl.npz")
FLOOR = 2e-6


@pytest.fixture(scope="module")
def g14():
    return np.load(G14, allow_pickle=False)


@pytest.fixture()
def medium(dev):
    import weatherforecastingtoolkit_amd as pkg
    pkg.set_float32_matmul_precision("medium")
    try:
        yield
    finally:
        pkg.set_float32_matmul_precision("highest")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def tol(spread):
    return max(4.0 * float(spread), FLOOR)


def rnd(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * (hi - lo) + lo).float()


# ------------------------------------------------------------------------------------------------ the 3x3 kernel
def conv3_oracle(x, w, b, scale, shift, res, kind, out_mul, dtype):
    """torch on the CPU in `dtype`: prologue silu(x * scale + shift), then the convolution of `kind`, + res, * out_mul"""
    x, w, b = x.to(dtype), w.to(dtype), b.to(dtype)
    if scale is not None:
        x = F.silu(x * scale.to(dtype)[:, :, None, None] + shift.to(dtype)[:, :, None, None])
    if kind == 0:
        y = F.conv2d(x, w, b, padding=1)
    elif kind == 1:
        y = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride=2)
    else:
        y = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, b, padding=1)
    if res is not None:
        y = y + res.to(dtype)
    return y * out_mul


def conv3_inputs(kind, n, cin, cout, h, w, seed):
    ho, wo = (h, w) if kind == 0 else ((h - 2) // 2 + 1, (w - 2) // 2 + 1) if kind == 1 else (2 * h, 2 * w)
    return dict(x=rnd((n, cin, h, w), seed, -2, 2), w=rnd((cout, cin, 3, 3), seed + 1) * (9 * cin) ** -0.5,
                b=rnd((cout,), seed + 2), scale=rnd((n, cin), seed + 3, 0.5, 1.5), shift=rnd((n, cin), seed + 4),
                res=rnd((n, cout, ho, wo), seed + 5))


# (kind, N, Cin, Cout, H, W): channel pairs from {32, 64, 128, 256, 512}; 16x16 and 48x48; planes that are odd multiples
# of 2 and non-square (tile tails in both directions); then the model's narrow layers (1 -> C, C -> 1, 4 -> C, C -> 8)
CONV3_CASES = [
    (0, 2, 32, 64, 16, 16), (0, 1, 128, 128, 48, 48), (0, 1, 512, 512, 16, 16), (0, 2, 64, 32, 6, 10),
    (0, 1, 256, 512, 14, 22), (0, 1, 512, 256, 10, 6),
    (1, 1, 128, 128, 48, 48), (1, 2, 32, 32, 6, 10), (1, 1, 256, 256, 16, 16), (1, 1, 64, 128, 14, 22),
    (2, 1, 512, 512, 16, 16), (2, 2, 256, 256, 6, 10), (2, 1, 128, 128, 24, 24), (2, 1, 64, 32, 7, 11),
    (0, 2, 1, 32, 18, 22), (0, 1, 128, 1, 48, 48), (0, 2, 4, 512, 16, 16), (0, 1, 512, 8, 16, 16),
]
CONV3_IDS = ["k%d-n%d-%dto%d-%dx%d" % c for c in CONV3_CASES]


def run_conv3(dev, case, variant, mode=None, seed=7, x=None):
    kind = case[0]
    t = conv3_inputs(*case, seed)
    if x is not None:
        t["x"] = x(t)
    pro, res, mul = "pro" in variant, "res" in variant, 0.5 if "scale" in variant else 1.0
    args = (t["x"], t["w"], t["b"], t["scale"] if pro else None, t["shift"] if pro else None, t["res"] if res else None,
            kind, mul)
    d = {k: v.to(dev) for k, v in t.items()}
    mode = ops.aekl_mode() if mode is None else mode
    packed = ops.aekl_conv3_pack(d["w"], mode)
    y = ops.aekl_conv3_fwd(d["x"], packed, case[3], d["b"], (d["scale"], d["shift"]) if pro else None,
                           d["res"] if res else None, kind, mode, mul)
    return y, args


@pytest.mark.parametrize("variant", ["plain", "pro", "res+scale", "pro+res+scale"])
@pytest.mark.parametrize("case", CONV3_CASES, ids=CONV3_IDS)
def test_conv3_against_fp64(dev, case, variant):
    y, args = run_conv3(dev, case, variant)
    o64, o32 = conv3_oracle(*args, torch.float64), conv3_oracle(*args, torch.float32)
    assert y.shape == o64.shape
    bound, err = tol(R.spread(o32, o64)), rel(y, o64)
    print(f"err {err:.3e} tol {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("case", [(0, 1, 128, 128, 48, 48), (1, 1, 64, 128, 14, 22), (2, 2, 256, 256, 6, 10)],
                         ids=lambda c: "k%d-n%d-%dto%d-%dx%d" % c)
def test_conv3_fp32_mfma_variant_against_fp64(dev, case):
    """the v_mfma_f32_16x16x4_f32 form: no precision setting selects it (the split form is faster); it is
    reached by an explicit `mode` alone and kept correct for the comparison tools/aekl_bench.py prints"""
    y, args = run_conv3(dev, case, "pro+res+scale", ops.AEKL_MODES["fp32"])
    o64, o32 = conv3_oracle(*args, torch.float64), conv3_oracle(*args, torch.float32)
    bound, err = tol(R.spread(o32, o64)), rel(y, o64)
    print(f"err {err:.3e} tol {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_conv3_border_is_zero_padded_after_the_prologue(dev, kind):
    """silu(gn(0)) != 0: with a shift of 3 a padding tap that went through the prologue would contribute silu(3) = 2.86 per
    weight.  The border outputs are compared on their own, and the wrong padding is shown to miss the bound."""
    case = (kind, 2, 64, 64, 10, 14)
    t = conv3_inputs(*case, 21)
    t["shift"] = torch.full_like(t["shift"], 3.0)
    d = {k: v.to(dev) for k, v in t.items()}
    y = ops.aekl_conv3_fwd(d["x"], ops.aekl_conv3_pack(d["w"]), 64, d["b"], (d["scale"], d["shift"]), None, kind).cpu()
    args = (t["x"], t["w"], t["b"], t["scale"], t["shift"], None, kind, 1.0)
    o64, o32 = conv3_oracle(*args, torch.float64), conv3_oracle(*args, torch.float32)

    def border(a):
        return torch.cat([a[:, :, 0].flatten(), a[:, :, -1].flatten(), a[:, :, :, 0].flatten(), a[:, :, :, -1].flatten()])
    bound = tol(R.spread(border(o32), border(o64)))
    err = rel(border(y), border(o64))
    print(f"border err {err:.3e} tol {bound:.3e}")
    assert err <= bound
    # the trap itself: padding before the prologue gives another border
    xp = F.silu(F.pad(t["x"].double(), (1, 1, 1, 1)) * t["scale"].double()[:, :, None, None] + 3.0)
    if kind == 0:
        wrong = F.conv2d(xp, t["w"].double(), t["b"].double())
        assert rel(border(wrong), border(o64)) > 100 * bound


@pytest.mark.parametrize("case", [(0, 1, 128, 128, 48, 48), (0, 2, 512, 256, 10, 6), (1, 1, 256, 256, 16, 16),
                                  (2, 1, 64, 32, 7, 11)], ids=lambda c: "k%d-n%d-%dto%d-%dx%d" % c)
def test_conv3_medium_is_fp32_on_bf16_rounded_operands(dev, medium, case):
    """'medium': only the h plane — torch fp32 on bf16-rounded activations and weights, to fp32 accumulation error"""
    assert ops.aekl_mode() == ops.AEKL_MODES["bf16"]
    y, args = run_conv3(dev, case, "res+scale")
    x, w = args[0].bfloat16().float(), args[1].bfloat16().float()
    args = (x, w) + args[2:]
    o64, o32 = conv3_oracle(*args, torch.float64), conv3_oracle(*args, torch.float32)
    bound, err = tol(R.spread(o32, o64)), rel(y, o64)
    print(f"err {err:.3e} tol {bound:.3e}")
    assert err <= bound


def x_for_bf16_safe_prologue(t):
    """x such that silu(x * scale + shift) = a * (1 + d): a is a bf16 value in [0.25, 4), |d| <= 2^-10.  The nearest bf16
    neighbours of a are at relative distance >= 2^-8, the rounding boundaries at >= 2^-9, so every fp32 evaluation of the
    prologue (errors of a few 2^-24) rounds to a, whatever its exp and whether or not it fuses the multiply-add: the
    oracle's operands after the prologue are the kernel's, bit for bit, and the fp32-accumulation bound applies."""
    shape = t["x"].shape
    a = rnd(shape, 31, 0.25, 4.0).bfloat16().double()
    want = a * (1.0 + rnd(shape, 32).double() * 2.0 ** -10)
    lo, hi = torch.zeros_like(want), torch.full_like(want, 8.0)       # silu is increasing on [0, 8], silu(8) > 4
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        below = mid * torch.sigmoid(mid) < want
        lo, hi = torch.where(below, mid, lo), torch.where(below, hi, mid)
    sc, sh = t["scale"].double()[:, :, None, None], t["shift"].double()[:, :, None, None]
    x = ((0.5 * (lo + hi) - sh) / sc).float()
    got = F.silu(x.double() * sc + sh)
    assert float((got / a - 1).abs().max()) <= 2.0 ** -10 * 1.01          # fp32 x moved the value by ~1e-7
    t["a"] = a.float()
    return x


@pytest.mark.parametrize("case", [(0, 1, 128, 128, 48, 48), (1, 1, 64, 128, 14, 22), (2, 2, 256, 256, 6, 10)],
                         ids=lambda c: "k%d-n%d-%dto%d-%dx%d" % c)
def test_conv3_medium_rounds_the_operand_after_the_prologue(dev, medium, case):
    """'medium' with the GroupNorm + SiLU prologue on, as the model runs it: the operand is bf16(silu(x * scale + shift)),
    rounded after the prologue.  Oracle: the convolution of those bf16 values and the bf16-rounded weights, to fp32
    accumulation error.  An oracle that leaves the prologue's result unrounded is shown to miss the same bound."""
    kept = {}

    def make_x(t):
        kept["x"] = x_for_bf16_safe_prologue(t)
        kept["a"] = t["a"]
        return kept["x"]
    y, args = run_conv3(dev, case, "pro+res", x=make_x)
    w = args[1].bfloat16().float()
    plain = (kept["a"], w, args[2], None, None) + args[5:]
    o64, o32 = conv3_oracle(*plain, torch.float64), conv3_oracle(*plain, torch.float32)
    bound, err = tol(R.spread(o32, o64)), rel(y, o64)
    unrounded = rel(conv3_oracle(*((args[0], w) + args[2:]), torch.float64), o64)
    print(f"err {err:.3e} tol {bound:.3e}; unrounded prologue {unrounded:.3e}")
    assert unrounded > 10 * bound
    assert err <= bound


def test_conv3_refuses_what_it_does_not_serve(dev):
    z = lambda *s: torch.zeros(*s, device=dev)
    w = ops.aekl_conv3_pack(z(32, 32, 3, 3))
    with pytest.raises(WfaeError, match="kind"):
        ops.aekl_conv3_fwd(z(1, 32, 8, 8), w, 32, kind=3)
    with pytest.raises(WfaeError, match="packed weights"):
        ops.aekl_conv3_fwd(z(1, 64, 8, 8), w, 32)
    with pytest.raises(WfaeError, match="mode"):
        _lib_call_bad_mode(z, w)
    with pytest.raises(WfaeError, match="2x2"):
        ops.aekl_conv3_fwd(z(1, 32, 1, 8), w, 32, kind=1)
    with pytest.raises(WfaeError, match="expected"):
        ops.aekl_conv3_pack(z(32, 32, 4, 4))
    with pytest.raises(WfaeError, match="fp32"):
        ops.aekl_conv3_fwd(z(1, 32, 8, 8).double(), w, 32)


def _lib_call_bad_mode(z, w):
    from weatherforecastingtoolkit_amd import _lib
    x, y = z(1, 32, 8, 8), z(1, 32, 8, 8)
    _lib.call("wfae_aekl_conv3_fwd", x.data_ptr(), w.data_ptr(), None, None, None, None, y.data_ptr(), 0, 2, 1, 32, 32, 8, 8,
              1.0, torch.cuda.current_stream().cuda_stream)


# -------------------------------------------------------------------------------------- GroupNorm statistics
@pytest.mark.parametrize("n,c,h,w,groups", [(2, 64, 16, 16, 8), (1, 128, 48, 48, 32), (3, 32, 6, 10, 32), (1, 512, 24, 24, 32),
                                            (1, 128, 128, 128, 8)])
@pytest.mark.parametrize("offset", [0.0, 100.0])
def test_group_norm_statistics(dev, n, c, h, w, groups, offset):
    """mean, rstd and the folded affine against fp64, also with |mean| = 100 std, where E[x^2] - E[x]^2 in fp32 has no
    digits left.  Bound: torch's own fp32 statistics against fp64 on the same values, times 4."""
    g = torch.Generator().manual_seed(c + h)
    x = torch.randn(n, c, h, w, generator=g) + offset
    gamma, beta = rnd((c,), 1, 0.5, 1.5), rnd((c,), 2)
    mean, rstd, scale, shift = (t.cpu() for t in ops.aekl_gn_stats(x.to(dev), gamma.to(dev), beta.to(dev), groups))
    xg = x.reshape(n, groups, -1)
    v64, m64 = torch.var_mean(xg.double(), dim=2, unbiased=False)
    v32, m32 = torch.var_mean(xg, dim=2, unbiased=False)
    r64, r32 = (v64 + 1e-6).rsqrt(), (v32 + 1e-6).rsqrt()
    bm, br = tol(R.spread(m32, m64)), tol(R.spread(r32, r64))
    em, er = rel(mean, m64), rel(rstd, r64)
    print(f"mean err {em:.3e} tol {bm:.3e}; rstd err {er:.3e} tol {br:.3e}")
    assert em <= bm and er <= br
    cg = c // groups
    s64 = gamma.double() * r64.repeat_interleave(cg, 1)
    h64 = beta.double() - m64.repeat_interleave(cg, 1) * s64
    assert rel(scale, s64) <= br
    # the shift carries mean * scale: its error is measured against that magnitude
    assert float((shift.double() - h64).abs().max()) <= max(bm, br) * float((m64.abs().max() * s64.abs().max()).clamp_min(1.0))
    if offset:
        naive = (xg * xg).mean(2) - xg.mean(2) ** 2          # what the kernel must not do
        assert rel((naive.clamp_min(0) + 1e-6).rsqrt(), r64) > 10 * br


def test_group_norm_statistics_repeatable(dev):
    x = (torch.randn(2, 128, 96, 96, generator=torch.Generator().manual_seed(3)) + 7).to(dev)
    gamma, beta = torch.ones(128, device=dev), torch.zeros(128, device=dev)
    a, b = ops.aekl_gn_stats(x, gamma, beta, 32), ops.aekl_gn_stats(x, gamma, beta, 32)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("rows,cols", [(256, 256), (2304, 2304), (7, 33)])
def test_row_softmax(dev, rows, cols):
    x = rnd((rows, cols), rows, -30, 30)
    y = ops.aekl_softmax(x.to(dev), 0.37)
    o64, o32 = torch.softmax(x.double() * 0.37, -1), torch.softmax(x * 0.37, -1)
    assert rel(y, o64) <= tol(R.spread(o32, o64))
    assert float((y.double().sum(-1) - 1).abs().max()) < 1e-5


@pytest.mark.parametrize("n,c,h,w,groups", [(2, 64, 16, 16, 8), (1, 512, 16, 16, 32), (1, 512, 48, 48, 32)],
                         ids=["S256-C64", "S256-C512", "S2304-C512"])
def test_attention_block(dev, n, c, h, w, groups):
    g = torch.Generator().manual_seed(c + h)
    p = "a"
    sd = {f"{p}.group_norm.weight": rnd((c,), 1, 0.5, 1.5), f"{p}.group_norm.bias": rnd((c,), 2)}
    for i, nm in enumerate(("query", "key", "value", "proj_attn")):
        sd[f"{p}.{nm}.weight"] = torch.randn(c, c, generator=g) * c ** -0.5 * (2.0 if i < 2 else 1.0)
        sd[f"{p}.{nm}.bias"] = rnd((c,), 10 + i)
    x = torch.randn(n, c, h, w, generator=g)
    d = {k: v.to(dev) for k, v in sd.items()}
    xd = x.to(dev)
    gn = ops.aekl_gn_stats(xd, d[f"{p}.group_norm.weight"], d[f"{p}.group_norm.bias"], groups)[2:]
    y = Fn.aekl_attention(xd, gn, *(d[f"{p}.{nm}.{wb}"] for nm in ("query", "key", "value", "proj_attn")
                                    for wb in ("weight", "bias")))
    o64 = A.attention(A.cast(sd, torch.float64), p, x.double(), groups)
    o32 = A.attention(sd, p, x, groups)
    bound, err = tol(R.spread(o32, o64)), rel(y, o64)
    print(f"err {err:.3e} tol {bound:.3e}")
    assert err <= bound


def test_attention_refuses_token_counts_off_the_grid(dev):
    with pytest.raises(WfaeError, match="multiples of 32"):
        ops.aekl_to_tokens(torch.zeros(1, 64, 6, 6, device=dev))
    with pytest.raises(WfaeError, match="multiples of 32"):
        ops.aekl_to_tokens(torch.zeros(1, 48, 8, 8, device=dev))


# ------------------------------------------------------------------------------------------------ posterior
def test_posterior_kernel(dev):
    g = torch.Generator().manual_seed(5)
    m = torch.randn(3, 8, 6, 10, generator=g) * 4
    m[0, 4, 0, :4] = torch.tensor([-31.0, -30.0, 20.0, 25.0])      # logvar at and beyond both clamps
    noise = torch.randn(3, 4, 6, 10, generator=g)
    mean, logvar, std, sample = ops.aekl_posterior(m.to(dev), noise.to(dev))
    m64 = m.double()
    lv = m64[:, 4:].clamp(-30.0, 20.0)
    assert torch.equal(mean.cpu(), m[:, :4]) and torch.equal(logvar.cpu(), m[:, 4:].clamp(-30.0, 20.0))
    sd = torch.exp(0.5 * lv)
    assert float(((std.double().cpu() - sd) / sd).abs().max()) <= FLOOR
    want = m64[:, :4] + sd * noise.double()
    assert rel(sample, want) <= FLOOR
    none = ops.aekl_posterior(m.to(dev))
    assert none[3] is None and torch.equal(none[2], std)


# ------------------------------------------------------------------------------------------------ the whole model
def golden_model(g14, p, dev):
    torch.manual_seed(int(g14["seed"]))
    model = AutoencoderKL(**A.CONFIGS[str(g14[f"{p}_config"])])
    assert R.values_digest(model.state_dict()) == str(g14[f"{p}_init_sha"])
    return model.to(dev)


def golden_input(g14, p):
    shape = tuple(int(v) for v in g14[f"{p}_x_shape"])
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(int(g14[f"{p}_x_seed"])))
    if f"{p}_x" in g14.files:
        assert torch.equal(x, torch.from_numpy(g14[f"{p}_x"]))
    import hashlib
    assert hashlib.sha256(x.numpy().tobytes()).hexdigest() == str(g14[f"{p}_x_sha"])
    return x


def check_fixture(g14, name, got, report):
    """`got` against the recorded fp64 value `name`: every stored element — the whole tensor, or the stored sample and the
    L2 norm"""
    t = tol(g14[f"{name}_spread"])
    got = got.detach().double().cpu()
    if name in g14.files:
        want = torch.from_numpy(g14[name]).double()
        assert want.shape == got.shape, name
        err = rel(got, want)
        print(f"{name}: err {err:.3e} tol {t:.3e}")
        if not err <= t:
            report.append((name, err, t))
        return
    want = torch.from_numpy(g14[f"{name}_sample"]).double()
    wn = float(g14[f"{name}_norm"])
    # max |fp64| of the whole tensor is not stored: the sample's maximum stands in for it (it is no larger, so the
    # measure is no more lenient)
    err = float((got.flatten()[R.sample_index(got.numel())] - want).abs().max() / want.abs().max())
    nerr = abs(float(got.norm()) - wn) / wn
    print(f"{name}: sample err {err:.3e} norm err {nerr:.3e} tol {t:.3e}")
    if not (err <= t and nerr <= t):
        report.append((name, err, nerr, t))


@pytest.mark.parametrize("p", ["a", "b", "c"])
def test_golden_parity(dev, g14, p):
    """mean, logvar, mode(), sample() for the stored noise and decode(mode) of the three recorded cases"""
    model = golden_model(g14, p, dev)
    x = golden_input(g14, p).to(dev)
    noise = torch.from_numpy(g14[f"{p}_noise"]).to(dev)
    post = model.encode(x)
    bad = []
    check_fixture(g14, f"{p}_mean", post.mean, bad)
    check_fixture(g14, f"{p}_logvar", post.logvar, bad)
    check_fixture(g14, f"{p}_mode", post.mode(), bad)
    check_fixture(g14, f"{p}_draw", post.sample(noise=noise), bad)
    check_fixture(g14, f"{p}_decode", model.decode(post.mode()), bad)
    assert not bad, bad


def test_sample_draws_like_torch(dev, g14):
    """sample(generator) = mean + std * torch.randn(mean.shape, generator=generator, device=...)"""
    model = golden_model(g14, "a", dev)
    post = model.encode(golden_input(g14, "a").to(dev))
    noise = torch.randn(post.mean.shape, generator=torch.Generator(device=dev).manual_seed(11), device=dev)
    got = post.sample(generator=torch.Generator(device=dev).manual_seed(11))
    assert torch.equal(got, post.sample(noise=noise))
    assert rel(got, post.mean.double() + post.std.double() * noise.double()) <= FLOOR
    kl = post.kl()
    want = 0.5 * (post.mean.double() ** 2 + post.std.double() ** 2 - 1 - post.logvar.double()).sum(dim=[1, 2, 3])
    assert kl.shape == (2,) and rel(kl, want) <= 1e-5
    dec, post2 = model(golden_input(g14, "a").to(dev), return_posterior=True)
    assert torch.equal(dec, model.decode(post.mode())) and torch.equal(post2.mean, post.mean)


def test_medium_follows_the_precision_switch(dev, g14, medium):
    """at 'medium' the model runs on bf16-rounded operands: close to, and different from, the fp32 result"""
    model = golden_model(g14, "a", dev)
    x = golden_input(g14, "a").to(dev)
    z = model.encode(x).mode()
    want = torch.from_numpy(g14["a_mode"]).double()
    err = rel(z, want)
    print(f"medium z err {err:.3e}")
    assert 1e-5 < err < 0.1


def test_forward_only(dev, g14):
    model = golden_model(g14, "a", dev)
    assert all(not q.requires_grad for q in model.parameters())
    x = golden_input(g14, "a").to(dev).requires_grad_(True)
    with pytest.raises(WfaeError, match="forward only"):
        model.encode(x)
    with pytest.raises(WfaeError, match="forward only"):
        model.decode(torch.zeros(1, 4, 16, 16, device=dev, requires_grad=True))
    with torch.no_grad():
        assert not model.encode(x).mode().requires_grad
    with pytest.raises(WfaeError, match="expected"):
        model.encode(torch.zeros(1, 3, 64, 64, device=dev))
    with pytest.raises(WfaeError, match="divisible"):
        model.encode(torch.zeros(1, 1, 66, 64, device=dev))


def test_bitwise_repeatable(dev, g14):
    model = golden_model(g14, "b", dev)
    x = golden_input(g14, "b").to(dev)
    z = [model.encode(x).mode().clone() for _ in range(2)]
    d = [model.decode(z[0]).clone() for _ in range(2)]
    torch.cuda.synchronize()
    assert torch.equal(z[0], z[1]) and torch.equal(d[0], d[1])


# ------------------------------------------------------------------------------------------------ provider, experiment
def _exp_dir():
    from weatherforecastingtoolkit_amd.experiments.v1_experiments import _convae as M
    return os.path.join(os.path.dirname(M.__file__), "pretrained_ae_convae_sevir")


def small_provider(dev, chunk):
    from weatherforecastingtoolkit_amd.experiments.v1_experiments._dlinear import Autoencoder
    cfg = C.Cfg(dict(A.CONFIGS["small"], kind="autoencoder_kl", checkpoint=None, chunk_frames=chunk, seed=0))
    return Autoencoder(64, "autoencoder_kl", cfg).to(dev)


def test_provider_chunking_is_bitwise_neutral(dev):
    frames = torch.rand(2, 5, 1, 64, 64, generator=torch.Generator().manual_seed(1)).to(dev)
    whole, chunked = small_provider(dev, 64), small_provider(dev, 3)
    a, b = whole.encode(frames), chunked.encode(frames)
    assert a.shape == (2, 5, 4, 16, 16) and torch.equal(a, b)
    assert whole.can_decode()
    da, db = whole.decode(a), chunked.decode(a)
    assert da.shape == (2, 5, 1, 64, 64) and torch.equal(da, db)
    # the provider returns the mode of the posterior
    model = whole.autoencoder
    assert torch.equal(a.view(10, 4, 16, 16), model.encode(frames.view(10, 1, 64, 64)).mode())


def test_provider_loads_a_checkpoint(dev, tmp_path):
    from weatherforecastingtoolkit_amd.experiments.v1_experiments._dlinear import Autoencoder
    torch.manual_seed(5)
    src = AutoencoderKL(**A.CONFIGS["small"])
    path = tmp_path / "vae.pt"
    torch.save({k: v.clone() for k, v in src.state_dict().items()}, path)
    cfg = C.Cfg(dict(A.CONFIGS["small"], kind="autoencoder_kl", checkpoint=str(path), chunk_frames=8))
    prov = Autoencoder(64, "autoencoder_kl", cfg).to(dev)
    for (k, a), (_, b) in zip(src.state_dict().items(), prov.autoencoder.state_dict().items()):
        assert torch.equal(a, b.cpu()), k


def test_launch_budget(dev, g14):
    """entry-point calls (ops.profile_start / profile_stop, as tests/test_convae_gpu.py counts them) of one encode and one
    decode at the reference configuration (64 latent channels, 1 x 128 x 128).  Designed for:
    encode 64 = conv_in 1 + 8 resnets x 4 (two statistics calls, two 3x3) + 2 shortcuts + 3 downsamplers + mid block 22
    (2 resnets x 4 + attention 14: statistics, to_tokens, 4 Linear, 4 splits, 2 products, softmax, from_tokens) +
    conv_norm_out / conv_out 2 + quant_conv 1 + posterior 1;
    decode 79 = post_quant_conv 1 + conv_in 1 + mid block 22 + 12 resnets x 4 + 2 shortcuts + 3 upsamplers + 2.
    Bounds: 1.5 x, i.e. 96 and 118.  Counted on an MI355X: 64 and 79."""
    model = golden_model(g14, "b", dev)
    x = golden_input(g14, "b").to(dev)
    z = model.encode(x).mode()      # warm-up: weight packing, workspace
    model.decode(z)
    ops.profile_start()
    z = model.encode(x).mode()
    enc = ops.profile_stop()
    ops.profile_start()
    model.decode(z)
    dec = ops.profile_stop()
    ne, nd = sum(v[0] for v in enc.values()), sum(v[0] for v in dec.values())
    print("encode", ne, {k: v[0] for k, v in enc.items()})
    print("decode", nd, {k: v[0] for k, v in dec.items()})
    assert "wfae_aekl_conv3_pack" not in enc and "wfae_aekl_conv3_pack" not in dec      # packed once per module
    assert ne <= 96 and nd <= 118


def test_experiment_runs_on_the_reference_geometry(dev, tmp_path):
    """pretrained_ae_convae_sevir with config_autoencoder_kl.yaml: 384 x 384 frames -> 4 x 48 x 48 latents; three training
    steps and a test_step with the 56 calc_metrics keys; the DLinear Model accepts the same provider"""
    from weatherforecastingtoolkit_amd.experiments.v1_experiments import _convae as M
    from weatherforecastingtoolkit_amd.experiments.v1_experiments import _dlinear as D
    from weatherforecastingtoolkit_amd.pipeline import metrics
    cfg = C.load(os.path.join(_exp_dir(), "config_autoencoder_kl.yaml"))
    assert cfg.autoencoder.kind == "autoencoder_kl" and cfg.autoencoder.latent_channels == 4
    assert cfg.convae.in_channels == 4 and cfg.convae.size == 48 and cfg.dataset.name == "sevir"
    cfg.trainer.total_train_steps = 3
    torch.manual_seed(0)
    prov = M.Autoencoder(384, cfg.autoencoder.kind, cfg.autoencoder)
    model = M.Model(cfg, autoencoder=prov).to(dev).train()
    model.autoencoder.eval()
    assert len(prov.autoencoder.state_dict()) == 248
    frames = torch.rand(2, 1, 384, 384, generator=torch.Generator().manual_seed(1)).to(dev)
    latents = prov.encode(frames.unsqueeze(2))
    assert latents.shape == (2, 1, 4, 48, 48)
    model.configure_optimizers()
    losses = [float(model.training_step(frames)[0]) for _ in range(3)]
    assert all(np.isfinite(losses))
    model.eval()
    loss, logs = model.test_step(frames)
    ref_keys = list(metrics.calc_metrics(torch.rand(1, 2, 1, 64, 64, device=dev), torch.rand(1, 2, 1, 64, 64, device=dev)))
    keys = [k for k in logs if k != "test_loss"]
    assert len(keys) == 56 and keys == [f"test_{k}" for k in ref_keys] and torch.isfinite(loss)

    from weatherforecastingtoolkit_amd.experiments.v1_experiments.pretrained_ae_convae_sevir import train
    assert train.main(["--config", os.path.join(_exp_dir(), "config_autoencoder_kl.yaml"), "--max-steps", "3",
                       "dataset.batch_size=2", f"experiment_path={tmp_path}"]) == 0

    # the DLinear forecaster on the same kind of provider (small configuration, 64 x 64 frames)
    dl = os.path.join(os.path.dirname(_exp_dir()), "pretrained_ae_dlinear_sevir", "config.yaml")
    dcfg = C.load(dl)
    dcfg.autoencoder = C.Cfg(dict(A.CONFIGS["small"], kind="autoencoder_kl", checkpoint=None, chunk_frames=4))
    dcfg.trainer.total_train_steps = 2
    dcfg.dlinear.enc_in = 4 * 16 * 16      # 64 x 64 frames -> 4 x 16 x 16 latents
    torch.manual_seed(0)
    dprov = D.Autoencoder(64, "autoencoder_kl", dcfg.autoencoder)
    t = dcfg.dataset.input_frames + dcfg.dataset.pred_frames
    dmodel = D.Model(dcfg, autoencoder=dprov).to(dev).train()
    dmodel.autoencoder.eval()
    dmodel.configure_optimizers()
    seq = torch.rand(1, t, 64, 64, generator=torch.Generator().manual_seed(2)).to(dev)
    out = dmodel.training_step(seq)
    assert np.isfinite(float(out[0]))
