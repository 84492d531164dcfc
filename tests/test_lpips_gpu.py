"""GPU: the LPIPS perceptual loss (csrc/lpips.hip, pipeline/models/autoencoderkl/losses/lpips.py) — every kernel against
torch on the CPU, the whole loss and its input gradient against the fp64 restatement tests/lpips_ref.py, repeatability,
the retained graph, 'medium', and one AE+GAN step with the perceptual term.

Tolerances, as in tests/test_aekl_gpu.py: every comparison is against fp64 in the measure max|a - b| / max|b|; the bound is
max(4 x spread, 2e-6), spread = the same measure between an fp32 and an fp64 run of torch on the CPU of the same
arithmetic, measured inside the test.  The kernel tests share their inputs (activations, masks) with the oracle, so no
ReLU or max-pool decision can fall differently; the end-to-end gradient is compared with the restatement's `acts=` mode fed
the product's own activations, for the same reason.

Measured on the MI355X (err / bound): see DESIGN.md "LPIPS perceptual loss"."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import lpips_ref as L
from weatherforecastingtoolkit_amd import ops
from weatherforecastingtoolkit_amd.pipeline.models.autoencoderkl.losses import LPIPS

pytestmark = pytest.mark.gpu

FLOOR = 2e-6


def rel(a, b):
    return L.spread(a.detach().cpu(), b.detach().cpu())


def tol(spread):
    return max(4.0 * float(spread), FLOOR)


def check(what, got, o32, o64):
    bound, err = tol(L.spread(o32, o64)), rel(got, o64)
    msg = f"{what}: err {err:.3e} bound {bound:.3e}"
    print(msg)
    assert got.shape == o64.shape and err <= bound, msg
    return err, bound


def rnd(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * (hi - lo) + lo).float()


@pytest.fixture()
def medium(dev):
    import weatherforecastingtoolkit_amd as pkg
    pkg.set_float32_matmul_precision("medium")
    try:
        yield
    finally:
        pkg.set_float32_matmul_precision("highest")


# ------------------------------------------------------------------------------------------------ conv3 + ReLU / mask
CONV_CASES = [(2, 3, 64, 9, 17), (1, 64, 128, 6, 10), (1, 256, 512, 3, 2), (1, 512, 512, 1, 1), (2, 128, 64, 14, 22)]
CONV_IDS = ["n%d-%dto%d-%dx%d" % c for c in CONV_CASES]


def conv_inputs(case, seed=11):
    n, cin, cout, h, w = case
    return dict(x=rnd((n, cin, h, w), seed, -2, 2), w=rnd((cout, cin, 3, 3), seed + 1) * (9 * cin) ** -0.5,
                b=rnd((cout,), seed + 2), dy=rnd((n, cout, h, w), seed + 3), a_prev=rnd((n, cin, h, w), seed + 4).clamp_min(0))


def conv_fwd_oracle(t, dtype, rounded=False):
    x, w = (t["x"].bfloat16().float(), t["w"].bfloat16().float()) if rounded else (t["x"], t["w"])
    return F.relu(F.conv2d(x.to(dtype), w.to(dtype), t["b"].to(dtype), padding=1))


def conv_bwd_oracle(t, dtype, rounded=False, mask=True):
    """the data gradient of conv2d(., w, padding=1) as torch states it (conv_transpose2d), times (a_prev > 0)"""
    dy, w = (t["dy"].bfloat16().float(), t["w"].bfloat16().float()) if rounded else (t["dy"], t["w"])
    dx = F.conv_transpose2d(dy.to(dtype), w.to(dtype), padding=1)
    return dx * (t["a_prev"] > 0).to(dtype) if mask else dx


def run_conv(dev, t, mode, mask=True):
    d = {k: v.to(dev) for k, v in t.items()}
    cin = t["x"].shape[1]
    y = ops.lpips_conv3_fwd(d["x"], ops.aekl_conv3_pack(d["w"], mode), d["b"], mode)
    wt = d["w"].flip(2, 3).transpose(0, 1).contiguous()
    dx = ops.lpips_conv3_bwd_data(d["dy"], ops.aekl_conv3_pack(wt, mode), cin, d["a_prev"] if mask else None, mode)
    return y, dx


@pytest.mark.parametrize("mode", [3, 4])
@pytest.mark.parametrize("case", CONV_CASES, ids=CONV_IDS)
def test_conv3_relu_forward_and_masked_backward_data(dev, case, mode):
    t = conv_inputs(case)
    y, dx = run_conv(dev, t, mode)
    check("fwd", y, conv_fwd_oracle(t, torch.float32), conv_fwd_oracle(t, torch.float64))
    check("bwd", dx, conv_bwd_oracle(t, torch.float32), conv_bwd_oracle(t, torch.float64))
    assert float(y.min()) == 0.0 and bool((dx.cpu()[t["a_prev"] <= 0] == 0).all())
    if case == CONV_CASES[0]:       # the first layer: no mask
        _, dx = run_conv(dev, t, mode, mask=False)
        check("bwd unmasked", dx, conv_bwd_oracle(t, torch.float32, mask=False), conv_bwd_oracle(t, torch.float64, mask=False))


@pytest.mark.parametrize("case", CONV_CASES, ids=CONV_IDS)
def test_conv3_mode_1_is_fp32_on_bf16_rounded_operands(dev, case):
    t = conv_inputs(case, seed=23)
    y, dx = run_conv(dev, t, 1)
    check("fwd bf16", y, conv_fwd_oracle(t, torch.float32, True), conv_fwd_oracle(t, torch.float64, True))
    check("bwd bf16", dx, conv_bwd_oracle(t, torch.float32, True), conv_bwd_oracle(t, torch.float64, True))


# ------------------------------------------------------------------------------------------------ max-pool
def pool_bwd_oracle(a, dy, add):
    ar = a.clone().requires_grad_(True)
    F.max_pool2d(ar, 2).backward(dy)
    return (ar.grad + add) * (a > 0).float() if add is not None else ar.grad * (a > 0).float()


def planted_ties():
    a = rnd((1, 64, 6, 5), 31, -1, 1).clamp_min(0)      # about half the elements are exact zeros (post-ReLU)
    a[0, 0:8, 0:2, 0:2] = 1.25                           # whole window tied at its maximum (the other values are <= 1)
    a[0, 8:16, 2, 2], a[0, 8:16, 3, 3] = 1.5, 1.5        # diagonal tie
    a[0, 16:24, 4, 1], a[0, 16:24, 5, 0] = 1.75, 1.75    # anti-diagonal tie
    a[0, 24:32, 0, 3], a[0, 24:32, 1, 3] = 2.0, 2.0      # vertical tie
    a[0, 32:40, 2:4, 0:2] = 0.0                          # all-zero windows
    a[0, 40:48] = 0.0
    return a


@pytest.mark.parametrize("shape", [(2, 64, 5, 7), (1, 128, 2, 2), (1, 64, 6, 5)], ids=lambda s: "x".join(map(str, s)))
def test_pool_forward_and_fused_backward_bit_exact(dev, shape):
    a = planted_ties() if shape == (1, 64, 6, 5) else rnd(shape, 29, -1, 1).clamp_min(0)
    n, c, h, w = shape
    dy, add = rnd((n, c, h // 2, w // 2), 30), rnd(shape, 32)
    y = ops.lpips_pool_fwd(a.to(dev))
    assert torch.equal(y.cpu(), F.max_pool2d(a, 2))
    for ad in (add, None):
        got = ops.lpips_pool_bwd(a.to(dev), dy.to(dev), None if ad is None else ad.to(dev)).cpu()
        want = pool_bwd_oracle(a, dy, ad)
        assert torch.equal(got, want), f"{int((got != want).sum())} of {got.numel()} differ"
    if h % 2 or w % 2:      # the last odd row / column belongs to no window: add, masked
        got = ops.lpips_pool_bwd(a.to(dev), dy.to(dev), add.to(dev)).cpu()
        edge = (slice(None), slice(None), slice(2 * (h // 2), None)) if h % 2 else (slice(None), slice(None), slice(None), slice(2 * (w // 2), None))
        assert torch.equal(got[edge], (add * (a > 0))[edge])


# ------------------------------------------------------------------------------------------------ distance
def dist_oracle(a0, a1, lin, g, dtype):
    x = a0.to(dtype).clone().requires_grad_(True)
    d = (L.normalize(x) - L.normalize(a1.to(dtype))) ** 2
    val = F.conv2d(d, lin.to(dtype).view(1, -1, 1, 1)).mean([2, 3]).flatten()
    (dx,) = torch.autograd.grad((val * g.to(dtype)).sum(), x)
    return val.detach(), dx


def dist_inputs(n, c, h, w, seed=41):
    return (rnd((n, c, h, w), seed, -1, 1).clamp_min(0), rnd((n, c, h, w), seed + 1, -1, 1).clamp_min(0), rnd((c,), seed + 2, 0, 1),
            rnd((n,), seed + 3, 0.5, 1.5))


@pytest.mark.parametrize("shape", [(1, 64, 5, 7), (1, 512, 1, 1), (2, 256, 2, 3)], ids=lambda s: "x".join(map(str, s)))
def test_dist_forward_and_backward(dev, shape):
    a0, a1, lin, g = dist_inputs(*shape)
    n = shape[0]
    v32, d32 = dist_oracle(a0, a1, lin, g, torch.float32)
    v64, d64 = dist_oracle(a0, a1, lin, g, torch.float64)
    out = torch.full((n,), 0.25, device=dev)
    ops.lpips_dist_fwd(a0.to(dev), a1.to(dev), lin.to(dev), out)          # accumulates into out
    check("value", out, v32 + 0.25, v64 + 0.25)
    da = ops.lpips_dist_bwd(a0.to(dev), a1.to(dev), lin.to(dev), g.to(dev))
    check("grad", da, d32, d64)
    dm = ops.lpips_dist_bwd(a0.to(dev), a1.to(dev), lin.to(dev), g.to(dev), relu=True)
    assert torch.equal(dm, da * (a0.to(dev) > 0))


def test_dist_backward_is_finite_at_an_all_zero_pixel(dev):
    """the documented deviation: the reference's autograd gives NaN where a0 is zero in every channel; the kernel drops
    the projection term there: da0 = u / 1e-10 with u = 2 g / HW lin (0 - f1).  Every other pixel is untouched."""
    a0, a1, lin, g = dist_inputs(1, 64, 5, 7)
    a0[0, :, 2, 3] = 0.0
    _, d64 = dist_oracle(a0, a1, lin, g, torch.float64)
    _, d32 = dist_oracle(a0, a1, lin, g, torch.float32)
    assert bool(d64[0, :, 2, 3].isnan().all())                  # the reference arithmetic
    da = ops.lpips_dist_bwd(a0.to(dev), a1.to(dev), lin.to(dev), g.to(dev)).cpu()
    assert bool(da.isfinite().all())
    keep = torch.ones(5, 7, dtype=torch.bool)
    keep[2, 3] = False
    check("other pixels", da[0][:, keep], d32[0][:, keep], d64[0][:, keep])
    f1 = L.normalize(a1.double())[0, :, 2, 3]
    eps32 = float(torch.tensor(1e-10, dtype=torch.float32))
    want = 2.0 * float(g[0]) / 35.0 * lin.double() * (0.0 - f1) / eps32
    assert L.spread(da[0, :, 2, 3], want) <= FLOOR


# ------------------------------------------------------------------------------------------------ scaling layer
@pytest.mark.parametrize("cx", [1, 3])
def test_prep_forward_and_backward(dev, cx):
    model = LPIPS()
    x, dy = rnd((2, cx, 5, 7), 51, 0, 1), rnd((2, 3, 5, 7), 52)
    sd = model.state_dict()
    shift, scale = sd["scaling_layer.shift"], sd["scaling_layer.scale"]
    y = ops.lpips_prep_fwd(x.to(dev), shift.to(dev), scale.to(dev))
    check("fwd", y, L.scaling(sd, x, torch.float32), L.scaling(sd, x, torch.float64))

    def bwd(dtype):
        xr = x.to(dtype).clone().requires_grad_(True)
        L.scaling(sd, xr, dtype).backward(dy.to(dtype))
        return xr.grad
    dx = ops.lpips_prep_bwd(dy.to(dev), scale.to(dev), cx)
    check("bwd", dx, bwd(torch.float32), bwd(torch.float64))
    # writing into one half of a 2N buffer
    z = torch.zeros((4, 3, 5, 7), device=dev)
    ops.lpips_prep_fwd(x.to(dev), shift.to(dev), scale.to(dev), z[2:])
    assert torch.equal(z[2:], y) and float(z[:2].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ end to end
E2E = {"a": ((2, 1, 48, 40), 0), "b": ((1, 3, 16, 16), 1)}
_e2e_cache = {}


def seeded(dev, seed):
    model = LPIPS()
    model.load_state_dict(L.weights(seed), strict=True)
    return model.to(dev)


def e2e(dev, name):
    """the product's value, activations and gradient, and the restatement's, once per case; nothing here is modified"""
    if name in _e2e_cache:
        return _e2e_cache[name]
    import weatherforecastingtoolkit_amd as pkg
    prev = ops.get_float32_matmul_precision()
    pkg.set_float32_matmul_precision("highest")
    try:
        _e2e_cache[name] = _e2e(dev, name)
    finally:
        pkg.set_float32_matmul_precision(prev)
    return _e2e_cache[name]


def _e2e(dev, name):
    shape, seed = E2E[name]
    sd = L.weights(seed)
    x, t = L.inputs(shape, seed)
    g = rnd((shape[0],), 61, 0.5, 1.5)
    model = seeded(dev, seed)
    xd = x.to(dev).requires_grad_(True)
    val, acts = model(xd, t.to(dev), return_activations=True)
    (dx,) = torch.autograd.grad((val.flatten() * g.to(dev)).sum(), xd)
    acts_cpu = [a.detach().cpu() for a in acts]
    r = dict(sd=sd, x=x, t=t, g=g, model=model, val=val.detach().cpu(), dx=dx.cpu(), acts=acts_cpu)
    r["v64"], r["dx64_own"], r["acts64"], r["taps64_t"] = L.value_and_grad(sd, x, t, torch.float64, None, g)
    r["v32"], _, r["acts32"], _ = L.value_and_grad(sd, x, t, torch.float32, None, g)
    _, r["dx64"], _, _ = L.value_and_grad(sd, x, t, torch.float64, acts_cpu, g)
    _, r["dx32"], _, _ = L.value_and_grad(sd, x, t, torch.float32, acts_cpu, g)
    return r


@pytest.mark.parametrize("name", list(E2E))
def test_value_against_the_fp64_restatement(dev, name):
    r = e2e(dev, name)
    assert tuple(r["val"].shape) == (E2E[name][0][0], 1, 1, 1) and len(r["acts"]) == 13
    check("value", r["val"], r["v32"], r["v64"])


@pytest.mark.parametrize("name", list(E2E))
def test_conditions_no_zero_pixel_and_relu_signs(dev, name):
    r = e2e(dev, name)
    taps = [r["acts64"][i] for i in (1, 3, 6, 9, 12)]
    norms = [float(a.pow(2).sum(1).sqrt().min()) for a in taps] + [float(a.pow(2).sum(1).sqrt().min()) for a in r["taps64_t"]]
    print("min channel norm", min(norms))
    assert min(norms) > 0.0                                       # the restatement has no all-zero feature pixel
    units = sum(a.numel() for a in r["acts64"])
    flips = sum(int(((a > 0) != (b > 0)).sum()) for a, b in zip(r["acts"], r["acts64"]))
    flips32 = sum(int(((a > 0) != (b > 0)).sum()) for a, b in zip(r["acts32"], r["acts64"]))
    msg = f"ReLU sign flips against fp64: product {flips}, torch fp32 {flips32}, of {units}"
    print(msg)
    assert flips <= 1e-5 * units, msg


@pytest.mark.parametrize("name", list(E2E))
def test_input_gradient_against_the_restatement_on_the_products_branch(dev, name):
    r = e2e(dev, name)
    assert r["dx"].shape == r["x"].shape and float(r["dx64"].abs().max()) > 0
    check("gradient", r["dx"], r["dx32"], r["dx64"])


def test_two_runs_give_the_same_bits(dev):
    r = e2e(dev, "a")
    xd = r["x"].to(dev).requires_grad_(True)
    val, acts = r["model"](xd, r["t"].to(dev), return_activations=True)
    (dx,) = torch.autograd.grad((val.flatten() * r["g"].to(dev)).sum(), xd)
    assert torch.equal(val.cpu(), r["val"]) and torch.equal(dx.cpu(), r["dx"])
    assert all(torch.equal(a.cpu(), b) for a, b in zip(acts, r["acts"]))


def test_backward_twice_through_a_retained_graph(dev):
    """calculate_adaptive_weight calls autograd.grad(..., retain_graph=True) before the real backward"""
    r = e2e(dev, "b")
    xd = r["x"].to(dev).requires_grad_(True)
    loss = r["model"](xd, r["t"].to(dev)).mean()
    (first,) = torch.autograd.grad(loss, xd, retain_graph=True)
    keep = first.clone()
    loss.backward()
    assert torch.equal(xd.grad, keep) and torch.equal(first, keep) and float(keep.abs().max()) > 0
    # without a gradient to take nothing is kept, and the value is the same
    with torch.no_grad():
        assert torch.equal(r["model"](xd, r["t"].to(dev)).mean(), loss.detach())


def test_medium_is_the_bf16_operand_arithmetic(dev, medium):
    r = e2e(dev, "a")          # the cached results are computed at 'highest' whatever the current setting
    assert ops.aekl_mode() == 1
    with torch.no_grad():
        vm = r["model"](r["x"].to(dev), r["t"].to(dev)).cpu()
        vb, _, _ = L.lpips(r["sd"], r["x"], r["t"], torch.float64, None, bf16_ops=True)
    err, bound = L.spread(vm, r["v64"]), 4.0 * L.spread(vb, r["v64"])
    msg = f"medium: |v - v64| {err:.3e}, 4 x |v64 on bf16 operands - v64| {bound:.3e}"
    print(msg)
    assert err <= bound, msg
    assert not torch.equal(vm, r["val"])                           # and it really is another arithmetic


def test_load_state_dict_repacks_the_weights(dev):
    r = e2e(dev, "b")
    model = seeded(dev, 1)
    x, t = r["x"].to(dev), r["t"].to(dev)
    with torch.no_grad():
        assert torch.equal(model(x, t).cpu(), r["val"])
        model.load_state_dict(L.weights(5), strict=True)
        other = model(x, t).cpu()
        assert not torch.equal(other, r["val"])
        model.load_state_dict(L.weights(1), strict=True)
        assert torch.equal(model(x, t).cpu(), r["val"])


# ------------------------------------------------------------------------------------------------ one AE+GAN step
def test_one_loss_step_with_the_perceptual_term(dev):
    """built as tests/test_gan_gpu.py builds its 128^2 B = 2 step, with perceptual_weight 0.5, disc_start 0"""
    from tests.test_gan_gpu import _cfg
    from weatherforecastingtoolkit_amd import functional as Fn
    from weatherforecastingtoolkit_amd import synth
    from weatherforecastingtoolkit_amd.experiments.ae_v2_2.train import Model
    cfg = _cfg(40, 0)
    cfg.lpips.perceptual_weight = 0.5
    sd = L.weights(2)
    lp = LPIPS()
    lp.load_state_dict(sd, strict=True)
    model = Model(cfg, img_size=128, lpips=lp)
    ae_sd = synth.synth_state_dict(synth.ae_state_dict_spec(128), seed=0)
    d_sd = synth.synth_state_dict(synth.disc_state_dict_spec(1, 64, 3), seed=5)
    model.autoencoder.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in ae_sd.items()}, strict=True)
    model.loss.discriminator.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in d_sd.items()}, strict=True)
    model = model.to(dev).train()
    model.configure_optimizers()
    x = torch.from_numpy(synth.uniform_frames(2, 128, seed=1234))
    before = [p.detach().clone() for p in model.autoencoder.parameters()]
    pred, logs = model.training_step({"vil": x.to(dev)}, 0)
    Fn.join_side_stream()
    pred = pred.detach().cpu()
    with torch.no_grad():
        want = {}
        for dtype in (torch.float32, torch.float64):
            v, _, _ = L.lpips(sd, pred, x, dtype)
            want[dtype] = (pred.to(dtype) - x.to(dtype)).abs().mean() + 0.5 * v.mean()
    got = float(logs["train/rec_loss"])
    err = abs(got - float(want[torch.float64])) / abs(float(want[torch.float64]))
    bound = tol(abs(float(want[torch.float32]) - float(want[torch.float64])) / abs(float(want[torch.float64])))
    msg = f"rec_loss {got:.8f}, L1 + 0.5 mean(LPIPS) in fp64 {float(want[torch.float64]):.8f}: err {err:.3e} bound {bound:.3e}"
    print(msg)
    assert err <= bound, msg
    dw = float(logs["train/d_weight"])
    assert np.isfinite(dw) and dw > 0.0 and np.isfinite(float(logs["train/total_loss"])) and "train/disc_loss" in logs
    assert model.global_step == 1 and np.isfinite(float(logs["train/g_grad_norm"]))
    assert any(not torch.equal(p.detach(), b) for p, b in zip(model.autoencoder.parameters(), before))
    assert all(p.grad is None for p in model.parameters())
