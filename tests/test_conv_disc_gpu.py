"""GPU: the conv + GAN latent model (csrc/c3s2.hip, experiments/v1_experiments/pretrained_ae_conv_disc) — parity with the
reference's recorded step (tests/golden/g17_conv_disc.npz), the 3x3 stride-2 unit in its three forms and both module
directions against fp64, dead taps, the discriminator's layers at (64, 16, 16), the whole model at the reference size
against the fp64 restatement tests/conv_disc_ref.py, bitwise repeatability, the launch budget and the experiment.

Tolerances.  Every comparison is against fp64 values in the measure max|a - b| / max|b|.  Per tensor the bound is
max(4 x spread, 2e-6), spread = the same measure between an fp32 and an fp64 run of the oracle on the CPU (recorded in the
fixture, or measured inside the test), and never looser than the project's standing bars (outputs 1e-4, loss 1e-5,
gradients 5e-4) — the rule of tests/test_convae_gpu.py.  SiLU is smooth; the one kink of the predictor's step is L1's at
recon = x, so every per-tensor comparison of gradients first asserts, on the oracle alone, that min |recon - x| is at least
4 x the fp32-vs-fp64 difference of recon.  The discriminator's LeakyReLU / hinge kinks carry no such precondition: its
gradients, and the generator's gradients through it, are compared by norm: the total norm, and the per-tensor norms as one
vector in the same measure."""
import os

import numpy as np
import pytest
import torch

from tests import conv_disc_ref as R
from weatherforecastingtoolkit_amd import config as C
from weatherforecastingtoolkit_amd import functional as Fn
from weatherforecastingtoolkit_amd import ops
from weatherforecastingtoolkit_amd._lib import WfaeError
from weatherforecastingtoolkit_amd.experiments import _gan
from weatherforecastingtoolkit_amd.experiments.v1_experiments import _conv_disc as M
from weatherforecastingtoolkit_amd.optim import FusedAdamW
from weatherforecastingtoolkit_amd.pipeline.models.autoencoderkl.losses import NLayerDiscriminator, weights_init

pytestmark = pytest.mark.gpu

G17 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g17_conv_disc.npz")
EXP = os.path.join(os.path.dirname(M.__file__), "pretrained_ae_conv_disc")
BAR_REC, BAR_LOSS, BAR_GRAD = 1e-4, 1e-5, 5e-4
FLOOR = 2e-6


@pytest.fixture(scope="module")
def g17():
    return np.load(G17, allow_pickle=False)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def tol(spread, bar=None):
    t = max(4.0 * float(spread), FLOOR)
    return min(t, bar) if bar is not None else t


def model_cfg(disc_start=10, total=20):
    cfg = C.load(os.path.join(EXP, "config.yaml"))
    cfg.trainer.total_train_steps = total
    cfg.lpips.disc_start = disc_start
    return cfg


def seeded_model(dev, seed=1234, disc_start=10):
    """Model whose predictor and discriminator are the fixture's: ConvModel, then the discriminator, from one seed"""
    torch.manual_seed(seed)
    pred = M.ConvModel()
    disc = NLayerDiscriminator(input_nc=64, n_layers=3).apply(weights_init)
    sd = {k: v.detach().clone() for k, v in pred.state_dict().items()}
    dsd = {k: v.detach().clone() for k, v in disc.state_dict().items()}
    model = M.Model(model_cfg(disc_start))
    model.predictor.load_state_dict(sd)
    model.loss.discriminator.load_state_dict(dsd)
    return model.to(dev).train(), sd, dsd


def check_fixture(g, name, got, bar, report):
    """`got` against the recorded fp64 value `name`: whole, or on the stored sample and the L2 norm"""
    t = tol(g[f"{name}_spread"], bar)
    got = got.detach().double().cpu()
    if name in g.files:
        want = torch.from_numpy(np.asarray(g[name])).double().reshape(got.shape)
        err = rel(got, want)
        print(f"{name}: err {err:.3e} tol {t:.3e}")
        if err > t:
            report.append((name, err, t))
        return
    want = torch.from_numpy(g[f"{name}_sample"]).double()
    err = float((got.flatten()[R.sample_index(got.numel())] - want).abs().max() / want.abs().max())
    wn = float(g[f"{name}_norm"])
    nerr = abs(float(got.norm()) - wn) / wn
    print(f"{name}: sample err {err:.3e} norm err {nerr:.3e} tol {t:.3e}")
    if err > t or nerr > t:
        report.append((name, err, nerr, t))


def pre_start_loss(model, x):
    pred, z = model(x)
    loss, _ = model.loss(x, pred, z, 0, model.get_last_layer(), "train", 0)
    return loss, z, pred


def test_golden_parity(dev, g17):
    model, sd, _ = seeded_model(dev, int(g17["seed"]))
    assert R.values_digest(sd) == str(g17["init_sha"])     # the recorded initial weights, rebuilt from the seed
    assert float(g17["l1_min_abs"]) >= 4 * float(g17["l1_diff"])
    x = torch.from_numpy(g17["x"]).to(dev)
    bad = []
    loss, z, rec = pre_start_loss(model, x)
    check_fixture(g17, "z", z, BAR_REC, bad)
    check_fixture(g17, "rec", rec, BAR_REC, bad)
    check_fixture(g17, "loss", loss, BAR_LOSS, bad)
    loss.backward()
    params = dict(model.predictor.named_parameters())
    assert len(params) == 24
    for k, p in params.items():
        check_fixture(g17, f"grad_{k}", p.grad, BAR_GRAD, bad)
    # three steps of AdamW (lr 1e-3, wd 1e-2) + clip_grad_norm_(1.0), as recorded; 1 - beta formed in double like torch
    opt = FusedAdamW(model.predictor.parameters(), lr=1e-3, weight_decay=1e-2, exact_complements=True)
    opt.zero_grad(set_to_none=True)
    for _ in range(3):
        loss, _, _ = pre_start_loss(model, x)
        loss.backward()
        opt.clip_grad_norm_(1.0)
        opt.step()
        opt.zero_grad(set_to_none=True)
    for k, p in params.items():
        check_fixture(g17, f"post_{k}", p, None, bad)
    assert not bad, bad


def test_golden_parity_gan(dev, g17):
    """from disc_start on: g_loss, d_weight, the generator loss and the norms of its 24 gradients (the discriminator
    frozen), the hinge loss and the norms of the discriminator's gradients — BatchNorm on batch statistics, as recorded"""
    model, sd, dsd = seeded_model(dev, int(g17["seed"]), disc_start=0)
    assert R.values_digest({k: v for k, v in dsd.items() if v.is_floating_point()}) == str(g17["disc_init_sha"])
    x = torch.from_numpy(g17["x"]).to(dev)
    bad = []

    def scalar(name, got, bar):
        t, want = tol(g17[f"{name}_spread"], bar), float(g17[name])
        err = abs(float(got) - want) / abs(want)
        print(f"{name}: got {float(got):.9e} want {want:.9e} err {err:.3e} tol {t:.3e}")
        if err > t:
            bad.append((name, err, t))

    def norms(prefix, grads):
        """the per-tensor L2 norms as ONE vector in the suite's measure, max|a - b| / max|b| (a recorded norm can be exactly
        0 — the hinge gradient of main.9.bias and main.11.bias is, in fp64 — so a per-entry ratio is not defined there; the
        generator's entries, none of which is zero, are also checked one by one below);
        the vector's spread is rebuilt from the per-entry ones the fixture holds.  Measured on an MI355X: generator 2.6e-6
        against 1.1e-5, discriminator 4.0e-5 against 2.5e-4; each entry's error relative to itself is printed — the
        generator's bias norms are 1.7e-6 to 7.6e-6 off, three of them (3.4e-6, 5.4e-6, 4.5e-6) above what 4 x their own
        fp32 spread would allow (2.0e-6 to 2.2e-6); d_weight, which scales the discriminator's share of them, is 4.1e-5 off"""
        want = np.array([float(g17[f"{prefix}_{k}_norm"]) for k in grads])
        dev32 = np.array([float(g17[f"{prefix}_{k}_norm_spread"]) * w if w > 0 else 0.0 for k, w in zip(grads, want)])
        got = np.array([float(g.double().norm()) for g in grads.values()])
        t = tol(dev32.max() / want.max(), BAR_GRAD)
        for k, a, b in zip(grads, got, want):
            print(f"{prefix}_{k}_norm: got {a:.9e} want {b:.9e} own-relative {abs(a - b) / max(b, 1e-300):.3e}")
        err = float(np.abs(got - want).max() / want.max())
        print(f"{prefix} norms: err {err:.3e} tol {t:.3e}")
        if err > t:
            bad.append((prefix, err, t))

    pred, z = model(x)
    with _gan.frozen(model.loss.discriminator.parameters()):
        loss, logs = model.loss(x, pred, z, 0, model.get_last_layer(), "train", 0)
        assert list(logs) == ["train/total_loss", "train/nll_loss", "train/rec_loss", "train/g_loss", "train/d_weight"]
        loss.backward()
    assert all(p.grad is None for p in model.loss.discriminator.parameters())
    scalar("g_loss", logs["train/g_loss"], BAR_LOSS)
    scalar("d_weight", logs["train/d_weight"], BAR_GRAD)
    scalar("gen_loss", loss, BAR_LOSS)
    grads = {k: p.grad for k, p in model.predictor.named_parameters()}
    scalar("gen_gradnorm", R.grad_norm(grads), BAR_GRAD)
    norms("gen_grad", grads)
    # entry by entry.  The generator's gradient of tensor k is A_k + w B_k: A the gradient of the nll (recorded before
    # disc_start), B that of g_loss, w = d_weight.  An error dw in the weight moves |A_k + w B_k| by at most |dw| |B_k|, and
    # |w B_k| <= |g_k| + |A_k|, so next to the entry's own max(4 x spread, 2e-6) it may be off by the relative error allowed
    # to d_weight (4 x its recorded fp32 spread) times (|g_k| + |A_k|) / |g_k|; never looser than the 5e-4 bar
    w_tol = 4.0 * float(g17["d_weight_spread"])
    for k, g in grads.items():
        want = float(g17[f"gen_grad_{k}_norm"])
        a_k = float(g17[f"grad_{k}_norm"]) if f"grad_{k}_norm" in g17.files else float(np.linalg.norm(g17[f"grad_{k}"].astype(np.float64)))
        t = min(tol(g17[f"gen_grad_{k}_norm_spread"]) + w_tol * (want + a_k) / want, BAR_GRAD)
        err = abs(float(g.double().norm()) - want) / want
        print(f"gen_grad_{k}_norm entry: err {err:.3e} tol {t:.3e}")
        if err > t:
            bad.append((k, err, t))
    d_loss, dlogs = model.loss(x, pred, z, 1, model.get_last_layer(), "train", 0)
    assert list(dlogs) == ["train/disc_loss", "train/logits_real", "train/logits_fake"]
    d_loss.backward()
    Fn.join_side_stream()
    scalar("d_loss", d_loss, BAR_LOSS)
    dgrads = {k: p.grad for k, p in model.loss.discriminator.named_parameters()}
    scalar("disc_gradnorm", R.grad_norm(dgrads), BAR_GRAD)
    norms("disc_grad", dgrads)
    assert not bad, bad


# (N, Chi, Clo, Hhi, Whi); w is (Clo, Chi, 3, 3).  The eight model shapes at N = 2 — encoder.conv.{0,2,4,6} in the first row,
# decoder.deconv.{0,2,4,6} (Clo -> Chi: 1024 -> 1024, 1024 -> 512, 512 -> 256, 256 -> 128) in the second; every case runs as
# Conv2d Chi -> Clo and as ConvTranspose2d Clo -> Chi, with and without SiLU —, N = 1 and N = 9, odd
# channel counts, odd and non-square planes (output_padding 0 on the way back), 1x1 -> 1x1 (only the centre tap is live),
# 2x2 -> 1x1 and 1x2 -> 1x1 (output_padding (0, 1)), Chi = 7 (9 Chi is no multiple of the 4-float access) next to Chi = 8,
# Clo = 33 (one row past a 32-row workgroup tile), and 40 x 64 = 2560 rows (more than one row range in the weight gradient)
UNIT_CASES = [
    (2, 64, 128, 16, 16), (2, 128, 256, 8, 8), (2, 256, 512, 4, 4), (2, 512, 1024, 2, 2),
    (2, 1024, 1024, 2, 2), (2, 512, 1024, 4, 4), (2, 256, 512, 8, 8), (2, 128, 256, 16, 16),
    (1, 64, 128, 16, 16), (9, 128, 256, 8, 8), (1, 512, 1024, 2, 2), (9, 512, 1024, 2, 2),
    (2, 3, 5, 6, 6), (2, 5, 3, 6, 6), (2, 3, 5, 5, 7), (2, 5, 3, 7, 5),
    (3, 6, 8, 1, 1), (3, 8, 6, 2, 2), (3, 8, 6, 1, 2), (2, 7, 33, 4, 4), (2, 8, 33, 4, 4), (40, 16, 24, 16, 16),
]
UNIT_SEED = 0    # SiLU has no kink; with this seed the fp32 oracle is within every bound for every case above


def run_unit(dev, inp, transposed, act, w=None):
    t = {k: v.to(dev).requires_grad_(k != "dy") for k, v in inp.items()}
    if w is not None:
        t["w"] = w.to(dev).requires_grad_(True)
    hi_hw = tuple(inp["dy"].shape[2:]) if transposed else tuple(inp["x"].shape[2:])
    lo_hw = tuple(inp["x"].shape[2:]) if transposed else tuple(inp["dy"].shape[2:])
    op = (hi_hw[0] - (2 * lo_hw[0] - 1), hi_hw[1] - (2 * lo_hw[1] - 1))
    y = Fn.conv3x3s2_act(t["x"], t["w"], t["b"], transposed, act, op)
    y.backward(t["dy"])
    return {"y": y.detach(), "dx": t["x"].grad, "dw": t["w"].grad, "db": t["b"].grad}


@pytest.mark.parametrize("act", [True, False], ids=["silu", "bare"])
@pytest.mark.parametrize("transposed", [False, True], ids=["conv", "convT"])
@pytest.mark.parametrize("case", UNIT_CASES, ids=lambda c: "n%d-hi%d-lo%d-%dx%d" % c)
def test_unit_against_fp64(dev, case, transposed, act):
    inp = R.unit_inputs(*case, transposed, UNIT_SEED)
    o64 = R.unit_oracle(inp, transposed, act, torch.float64)
    o32 = R.unit_oracle(inp, transposed, act, torch.float32)
    got = run_unit(dev, inp, transposed, act)
    bad = []
    for name, g in got.items():
        assert g is not None and g.shape == o64[name].shape, name
        bound = tol(R.spread(o32[name], o64[name]), BAR_REC if name == "y" else BAR_GRAD)
        err = rel(g, o64[name])
        print(f"{name}: err {err:.3e} tol {bound:.3e}")
        if err > bound:
            bad.append((name, err, bound))
    assert not bad, bad


def dead_mask(hhi, whi):
    return ~torch.tensor(ops.c3s2_live_taps(hhi, whi))


@pytest.mark.parametrize("chi", [5, 12], ids=["scalar-access", "vector-access"])
@pytest.mark.parametrize("transposed", [False, True], ids=["2x2to1x1", "1x1to2x2"])
def test_dead_taps_are_never_read_and_get_exact_zeros(dev, transposed, chi):
    inp = R.unit_inputs(3, chi, 9, 2, 2, transposed, 3)
    dead = dead_mask(2, 2)
    assert int(dead.sum()) == 5
    w_nan, w_zero = inp["w"].clone(), inp["w"].clone()
    w_nan[:, :, dead], w_zero[:, :, dead] = float("nan"), 0.0
    o64 = R.unit_oracle(inp, transposed, True, torch.float64, w=w_zero)
    o32 = R.unit_oracle(inp, transposed, True, torch.float32, w=w_zero)
    got = run_unit(dev, inp, transposed, True, w=w_nan)
    for name in ("y", "dx", "db"):
        assert bool(torch.isfinite(got[name]).all()), name
        bound, err = tol(R.spread(o32[name], o64[name]), BAR_REC if name == "y" else BAR_GRAD), rel(got[name], o64[name])
        print(f"{name}: err {err:.3e} tol {bound:.3e}")
        assert err <= bound, name
    dw = got["dw"].cpu()
    assert bool((dw[:, :, dead] == 0.0).all()) and not bool(torch.signbit(dw[:, :, dead]).any())
    live_err = float((dw[:, :, ~dead].double() - o64["dw"][:, :, ~dead]).abs().max() / o64["dw"].abs().max())
    assert live_err <= tol(R.spread(o32["dw"], o64["dw"]), BAR_GRAD)

    # accumulate: a prefilled gradient keeps its dead-tap values bit for bit, live taps and the bias get the sum
    t = {k: v.to(dev) for k, v in inp.items()}
    _, pre = ops.c3s2_fwd(t["x"], w_nan.to(dev), t["b"], transposed, True, 1)
    fill = torch.randn(inp["w"].shape, generator=torch.Generator().manual_seed(4))
    fill[0, 0, 0, 0], fill[1, 0, 0, 1], fill[2, 0, 0, 2] = -0.0, float("nan"), float("inf")
    dwa, dba = fill.to(dev), torch.ones_like(t["b"])
    ops.c3s2_bwd_weight(t["dy"], pre, t["x"], dwa, dba, transposed, True, accumulate=True)
    dwa = dwa.cpu()
    assert torch.equal(dwa[:, :, dead].view(torch.int32), fill[:, :, dead].view(torch.int32))
    # the sums: the prefill is exact in both precisions, so the spread of the sum is that of the gradient's own fp32 error
    want = fill[:, :, ~dead].double() + o64["dw"][:, :, ~dead]
    sp = float((o32["dw"][:, :, ~dead].double() - o64["dw"][:, :, ~dead]).abs().max() / want.abs().max())
    err, bound = float((dwa[:, :, ~dead].double() - want).abs().max() / want.abs().max()), tol(sp, BAR_GRAD)
    print(f"accumulated dw (live): err {err:.3e} tol {bound:.3e}")
    assert err <= bound
    err, bound = rel(dba, 1.0 + o64["db"]), tol(R.spread(1.0 + o32["db"].double(), 1.0 + o64["db"]), BAR_GRAD)
    print(f"accumulated db: err {err:.3e} tol {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("transposed", [False, True], ids=["4x4to2x2", "2x2to4x4"])
def test_live_taps_propagate_nan(dev, transposed):
    """at 4x4 -> 2x2 all nine taps are live: a NaN weight in any of them must reach the output"""
    assert not bool(dead_mask(4, 4).any())
    inp = R.unit_inputs(2, 4, 6, 4, 4, transposed, 5)
    t = {k: v.to(dev) for k, v in inp.items()}
    for ky in range(3):
        for kx in range(3):
            w = inp["w"].clone()
            w[:, :, ky, kx] = float("nan")
            y, _ = ops.c3s2_fwd(t["x"], w.to(dev), t["b"], transposed, True, 1)
            assert bool(torch.isnan(y).any()), (ky, kx)


def test_unit_skips_the_data_gradient_when_not_asked(dev):
    """the first encoder layer: its input, the frozen provider's latent, needs no gradient"""
    inp = R.unit_inputs(2, 64, 128, 16, 16, False, 1)
    t = {k: v.to(dev) for k, v in inp.items()}
    t["w"].requires_grad_(True)
    t["b"].requires_grad_(True)
    ops.profile_start()
    y = Fn.conv3x3s2_act(t["x"], t["w"], t["b"])
    y.backward(t["dy"])
    prof = ops.profile_stop()
    assert t["x"].grad is None and t["w"].grad is not None and t["b"].grad is not None
    assert {k: v[0] for k, v in prof.items()} == {"wfae_c3s2_fwd": 1, "wfae_c3s2_bwd_weight": 1}
    o64, o32 = R.unit_oracle(inp, False, True, torch.float64), R.unit_oracle(inp, False, True, torch.float32)
    for name, got in (("dw", t["w"].grad), ("db", t["b"].grad)):
        err, bound = rel(got, o64[name]), tol(R.spread(o32[name], o64[name]), BAR_GRAD)
        print(f"{name}: err {err:.3e} tol {bound:.3e}")
        assert err <= bound, name


def test_unit_refusals_on_device(dev):
    z = lambda *s: torch.zeros(*s, device=dev)
    with pytest.raises(WfaeError, match="weight"):
        ops.c3s2_fwd(z(1, 5, 4, 4), z(8, 4, 3, 3))
    with pytest.raises(WfaeError, match="belong together"):
        ops.c3s2_bwd_data(z(1, 8, 3, 3), z(1, 8, 3, 3), z(8, 4, 3, 3), (1, 4, 4, 4))
    with pytest.raises(WfaeError, match="belong together"):
        ops.c3s2_bwd_weight(z(1, 8, 2, 2), z(1, 8, 2, 2), z(1, 4, 6, 6), z(8, 4, 3, 3))


# the discriminator NLayerDiscriminator(64) on a 16 x 16 plane, layer by layer: (Cin, Cout, stride, bias, plane in)
DISC_LAYERS = [(64, 64, 2, True, 16), (64, 128, 2, False, 8), (128, 256, 2, False, 4), (256, 512, 1, False, 2)]


@pytest.mark.parametrize("layer", DISC_LAYERS, ids=lambda c: "%dto%d-s%d-b%d-%dx%d" % (c + (c[4],)))
def test_discriminator_layers_at_64x16x16_against_fp64(dev, layer):
    """the 4x4 convolutions of the PatchGAN at 64 input channels on 16 x 16: forward, data and weight gradient"""
    cin, cout, stride, bias, plane = layer
    g = torch.Generator().manual_seed(cin + plane)
    x = torch.randn(4, cin, plane, plane, generator=g)
    w = torch.randn(cout, cin, 4, 4, generator=g) / (cin * 16) ** 0.5
    b = 0.5 * torch.randn(cout, generator=g) if bias else None
    outs = {}
    for dt in (torch.float64, torch.float32):
        xr, wr = x.to(dt).requires_grad_(True), w.to(dt).requires_grad_(True)
        br = b.to(dt).requires_grad_(True) if bias else None
        y = torch.nn.functional.conv2d(xr, wr, br, stride=stride, padding=1)
        dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(7))
        y.backward(dy.to(dt))
        outs[dt] = {"y": y.detach(), "dx": xr.grad, "dw": wr.grad, "db": br.grad if bias else None}
    xd, wd = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
    bd = b.to(dev).requires_grad_(True) if bias else None
    y = Fn.Conv4Fn.apply(xd, wd, bd, stride)
    y.backward(dy.to(dev))
    Fn.join_side_stream()
    got = {"y": y.detach(), "dx": xd.grad, "dw": wd.grad, "db": bd.grad if bias else None}
    bad = []
    for name, gt in got.items():
        if gt is None:
            continue
        bound = tol(R.spread(outs[torch.float32][name], outs[torch.float64][name]), BAR_REC if name == "y" else BAR_GRAD)
        err = rel(gt, outs[torch.float64][name])
        print(f"{name}: err {err:.3e} tol {bound:.3e}")
        if err > bound:
            bad.append((name, err, bound))
    assert not bad, bad


B8_SEED = 2002   # chosen on the CPU: the L1 precondition holds at B = 8 with this seed (it does not with 2001)


def whole_step(model, x):
    loss, z, rec = pre_start_loss(model, x)
    loss.backward()
    return loss, z, rec, {k: p.grad for k, p in model.predictor.named_parameters()}


def test_reference_size_b8_against_fp64(dev):
    """the config's batch of 8 against the fp64 restatement.  The L1 precondition holds for the chosen seed (asserted), so
    the forward, the loss and all 24 gradients are compared per tensor"""
    model, sd, _ = seeded_model(dev)
    x = torch.randn(8, 64, 16, 16, generator=torch.Generator().manual_seed(B8_SEED))
    l64, z64, r64, g64 = R.run(sd, x, torch.float64)
    l32, z32, r32, g32 = R.run(sd, x, torch.float32)
    amin, diff = R.l1_margin(r64, r32, x)
    assert amin >= 4 * diff, f"oracle precondition: min |recon - x| = {amin:.3e}, fp32-vs-fp64 difference {diff:.3e}"
    loss, z, rec, grads = whole_step(model, x.to(dev))
    bad = []
    for name, got, w32, w64, bar in [("z", z, z32, z64, BAR_REC), ("rec", rec, r32, r64, BAR_REC),
                                     ("loss", loss, l32, l64, BAR_LOSS)] + \
                                    [(f"grad_{k}", grads[k], g32[k], g64[k], BAR_GRAD) for k in g64]:
        bound, err = tol(R.spread(w32, w64), bar), rel(got, w64)
        print(f"{name}: err {err:.3e} tol {bound:.3e}")
        if err > bound:
            bad.append((name, err, bound))
    assert not bad, bad


def test_loss_and_gradients_bitwise_repeatable(dev):
    """the reductions split over workgroups (K chunks, channel ranges, row ranges) are finished in a fixed order"""
    model, _, _ = seeded_model(dev)
    x = torch.randn(8, 64, 16, 16, generator=torch.Generator().manual_seed(B8_SEED)).to(dev)
    runs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        loss, _, _, grads = whole_step(model, x)
        runs.append([loss.detach().clone()] + [g.clone() for g in grads.values()])
    torch.cuda.synchronize()
    assert len(runs[0]) == 25
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_launch_budget(dev):
    """one forward + loss + backward of the pre-disc_start step at B = 8: at most 49 entry-point calls.  The 8 conv + SiLU
    units are one forward, one data-gradient and one weight-gradient call each, the first without a data gradient: 23.
    Three Linears (encoder.conv_out on its 1x1 plane, encoder.fc, decoder.fc) at 4 each (forward, weight gradient, data
    gradient, bias sum): 12.  decoder.conv_out through conv1x1: 4.  L1 forward + backward: 2.  The scale by
    exp(-logvar) / B forward + backward: 2.  23 + 12 + 4 + 2 + 2 = 43, plus 6."""
    model, _, _ = seeded_model(dev)
    x = torch.randn(8, 64, 16, 16, generator=torch.Generator().manual_seed(B8_SEED)).to(dev)
    whole_step(model, x)      # warm-up: workspace allocation
    model.zero_grad(set_to_none=True)
    ops.profile_start()
    whole_step(model, x)
    prof = ops.profile_stop()
    calls = sum(v[0] for v in prof.values())
    print({k: v[0] for k, v in prof.items()}, calls)
    assert prof["wfae_c3s2_fwd"][0] == 8 and prof["wfae_c3s2_bwd_weight"][0] == 8 and prof["wfae_c3s2_bwd_data"][0] == 7
    assert not [k for k in prof if "silu" in k or "gelu" in k or "sigmoid" in k]       # no standalone activation launch
    assert calls <= 49, prof


def test_gradients_land_in_the_optimiser_arena(dev):
    """every predictor gradient, encoder.conv_out's (a 1x1 convolution run as a Linear) included, is written by its kernel
    into the flat gradient buffer: one AdamW launch for the 24 tensors"""
    model, _, _ = seeded_model(dev)
    model.configure_optimizers()
    x = torch.randn(2, 64, 16, 16, generator=torch.Generator().manual_seed(1)).to(dev)
    whole_step(model, x)
    Fn.join_side_stream()
    assert model.opt.arenas[0].grads_in_arena()


def test_discriminator_step_is_one_optimiser_launch(dev):
    """from disc_start on: the two hinge terms are taken backward one after the other, so the discriminator's gradients sit
    in its flat buffer like the generator's and each optimiser is one AdamW launch; a bias-only unit still gets its gradient"""
    model, _, _ = seeded_model(dev, disc_start=0)
    model.configure_optimizers()
    x = torch.randn(2, 1, 64, 16, 16, generator=torch.Generator().manual_seed(1)).to(dev)
    model.training_step(x)      # warm-up
    d_before = [p.detach().clone() for p in model.loss.discriminator.parameters()]
    ops.profile_start()
    model.training_step(x)
    prof = ops.profile_stop()
    print({k: v[0] for k, v in prof.items()})
    assert prof["wfae_adamw"][0] == 2, prof["wfae_adamw"]
    assert all(np.isfinite(float(v)) for v in model.logs.values())
    assert not torch.equal(d_before[0], next(model.loss.discriminator.parameters()))
    inp = R.unit_inputs(2, 6, 8, 4, 4, False, 2)
    t = {k: v.to(dev) for k, v in inp.items()}
    t["b"].requires_grad_(True)
    Fn.conv3x3s2_act(t["x"], t["w"], t["b"]).backward(t["dy"])
    o64, o32 = R.unit_oracle(inp, False, True, torch.float64), R.unit_oracle(inp, False, True, torch.float32)
    err, bound = rel(t["b"].grad, o64["db"]), tol(R.spread(o32["db"], o64["db"]), BAR_GRAD)
    print(f"db (frozen weight): err {err:.3e} tol {bound:.3e}")
    assert t["w"].grad is None and err <= bound


def test_experiment_trains_validates_and_saves(dev, tmp_path, g17):
    from weatherforecastingtoolkit_amd.pipeline import metrics
    cfg = model_cfg(disc_start=10, total=20)
    cfg.dataset.batch_size = 4
    torch.manual_seed(0)
    model = M.Model(cfg, autoencoder=M.Autoencoder(128, cfg.autoencoder.kind, cfg.autoencoder)).to(dev).train()
    model.autoencoder.eval()
    frames = torch.rand(4, 1, 128, 128, generator=torch.Generator().manual_seed(1)).to(dev)
    latents = model.autoencoder.encode(frames.unsqueeze(2))
    assert latents.shape == (4, 1, 64, 16, 16)
    model.configure_optimizers()
    assert all(p.requires_grad is False for p in model.autoencoder.parameters())
    assert {id(p) for g in model.opt.param_groups for p in g["params"]} == {id(p) for p in model.predictor.parameters()}
    assert model.d_opt.param_groups[0]["betas"] == (0.5, 0.999) and model.opt.param_groups[0]["betas"] == (0.9, 0.999)
    d0 = [p.detach().clone() for p in model.loss.discriminator.parameters()]
    p0 = [p.detach().clone() for p in model.predictor.parameters()]
    losses = []
    for step in range(20):
        loss, gn = model.training_step(frames)
        logs = {k: float(v) for k, v in model.logs.items()}
        losses.append(float(loss))
        assert all(np.isfinite(v) for v in logs.values()), (step, logs)
        if step < 10:
            assert logs["train/g_loss"] == 0.0 and logs["train/d_weight"] == 0.0 and "train/disc_loss" not in logs
            assert logs["train/total_loss"] == logs["train/nll_loss"] == float(loss)
            assert abs(logs["train/rec_loss"] - 4 * logs["train/nll_loss"]) <= 1e-6 * logs["train/rec_loss"]   # logvar 0, B 4
        else:
            assert {"train/disc_loss", "train/logits_real", "train/logits_fake", "train/d_grad_norm"} <= set(logs)
            assert logs["train/d_weight"] > 0.0
        if step == 9:
            assert all(torch.equal(a, b) for a, b in zip(d0, model.loss.discriminator.parameters()))
    print("losses", losses)
    assert losses[9] < losses[0]
    # after the start every discriminator weight has moved (a bias whose gradient is exactly zero may stand still: the
    # output bias sees the real and the fake hinge terms cancel while every logit is inside (-1, 1))
    moved = {k: not torch.equal(a, p) for a, (k, p) in zip(d0, model.loss.discriminator.named_parameters())}
    assert all(v for k, v in moved.items() if k.endswith("weight")), moved
    assert not any(torch.equal(a, b) for a, b in zip(p0, model.predictor.parameters()))
    assert model.global_step == 20
    model.eval()
    loss, logs = model.validation_step(frames)
    ref_keys = list(metrics.calc_metrics(torch.rand(1, 1, 1, 64, 64, device=dev), torch.rand(1, 1, 1, 64, 64, device=dev)))
    loss_keys = ["val/total_loss", "val/nll_loss", "val/rec_loss", "val/g_loss", "val/d_weight", "val/disc_loss",
                 "val/logits_real", "val/logits_fake"]
    assert list(logs)[:8] == loss_keys and float(logs["val/d_weight"]) == 0.0
    keys = list(logs)[8:]
    assert len(keys) == 56 and keys == [f"val_{k}" for k in ref_keys]
    assert all(np.isfinite(float(v)) for v in logs.values())
    _, tlogs = model.test_step(frames)
    assert sorted(tlogs) == sorted([k.replace("val/", "test/") for k in loss_keys] + [f"test_{k}" for k in ref_keys])
    _, llogs = model.validation_step(latents)       # latents carry no frames to score against
    assert list(llogs) == loss_keys

    from weatherforecastingtoolkit_amd.experiments.v1_experiments.pretrained_ae_conv_disc import train
    assert train.main(["--max-steps", "3", f"experiment_path={tmp_path}"]) == 0
    ck = torch.load(tmp_path / "outputs" / "pretrained_ae_conv_disc" / "checkpoints" / "last.ckpt", map_location="cpu")
    assert ck["global_step"] == 3
    keys = list(ck["state_dict"])
    assert [(k, tuple(ck["state_dict"][k].shape)) for k in keys[:24]] == [("predictor." + k, s) for k, s in R.key_list()]
    assert keys[24] == "loss.logvar" and ck["state_dict"]["loss.logvar"].shape == ()
    assert keys[25:] == ["loss.discriminator." + str(k) for k in g17["disc_keys"]]
