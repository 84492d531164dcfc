"""GPU: the DLinear kernels (csrc/dlinear.hip) and the three DLinear experiments — parity with the reference's
recorded step (tests/golden/g12_dlinear.npz), with the fp64 restatement tests/dlinear_ref.py at the reference size and
at edge shapes, the input gradient, bitwise repeatability, validation metrics and the experiment scripts."""
import os

import numpy as np
import pytest
import torch

from tests import dlinear_ref as R
from weatherforecastingtoolkit_amd import config as C
from weatherforecastingtoolkit_amd import functional as Fn
from weatherforecastingtoolkit_amd import ops
from weatherforecastingtoolkit_amd.experiments.v1_experiments import _dlinear as D
from weatherforecastingtoolkit_amd.optim import FusedAdamW

pytestmark = pytest.mark.gpu

G12 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g12_dlinear.npz")
EXP = os.path.dirname(D.__file__)
MAPS = ("Linear_Seasonal", "Linear_Trend")


@pytest.fixture(scope="module")
def g12():
    return np.load(G12, allow_pickle=False)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def model_cfg(variant, M, cf):
    cfg = C.load(os.path.join(EXP, f"pretrained_ae_dlinear_{variant}", "config.yaml"))
    cfg.dlinear.enc_in, cfg.dlinear.features_per_step = M, cf
    return cfg


def params_of(m):
    return [m.seasonal_weight, m.seasonal_bias, m.trend_weight, m.trend_bias]


@pytest.mark.parametrize("variant", list(R.VARIANTS))
def test_golden_parity(dev, g12, variant):
    individual, K, cf, _ = R.VARIANTS[variant]
    v = torch.from_numpy(g12[f"{variant}_v"]).to(dev)
    b, _, c, h, w = v.shape
    model = D.Model(model_cfg(variant, c * h * w // cf, cf)).to(dev)
    for p, (n, s) in zip(params_of(model.predictor), [(n, s) for n in MAPS for s in ("w", "b")]):
        p.data.copy_(torch.from_numpy(g12[f"{variant}_init_{n}_{s}"]))
    loss, pred, _ = model.latent_loss(v)
    assert rel(pred.view(b, R.TOUT, c, h, w), torch.from_numpy(g12[f"{variant}_pred"])) <= 1e-5
    assert abs(loss.item() - float(g12[f"{variant}_loss"])) <= 1e-6 * abs(float(g12[f"{variant}_loss"]))
    loss.backward()
    for p, (n, s) in zip(params_of(model.predictor), [(n, s) for n in MAPS for s in ("w", "b")]):
        assert rel(p.grad, torch.from_numpy(g12[f"{variant}_grad_{n}_{s}"])) <= 1e-5, (n, s)
    if model.predictor.has_decoder:
        assert model.predictor.decoder_weight.grad is None
    # three steps of AdamW (lr 1e-3, wd 1e-2) + clip_grad_norm_(1.0), as recorded
    opt = FusedAdamW(model.predictor.parameters(), lr=1e-3, weight_decay=1e-2)
    opt.zero_grad(set_to_none=True)
    for _ in range(3):
        loss, _, _ = model.latent_loss(v)
        loss.backward()
        opt.clip_grad_norm_(1.0)
        opt.step()
        opt.zero_grad(set_to_none=True)
    for p, (n, s) in zip(params_of(model.predictor), [(n, s) for n in MAPS for s in ("w", "b")]):
        assert rel(p, torch.from_numpy(g12[f"{variant}_post_{n}_{s}"])) <= 1e-5, (n, s)


def _random_params(M, P, L, individual, dev, seed):
    g = torch.Generator().manual_seed(seed)
    ws = (M, P, L) if individual else (P, L)
    bs = (M, P) if individual else (P,)
    return [(torch.randn(*shape, generator=g) / (L ** 0.5 if len(shape) > 1 + individual else 1)).to(dev)
            for shape in (ws, bs, ws, bs)]


def _check_against_fp64(dev, B, M, Tin, Tout, cf, K, individual, seed=0, need_dx=True):
    L, P = Tin * cf, Tout * cf
    g = torch.Generator().manual_seed(seed + 7)
    v = torch.randn(B, (Tin + Tout) * cf, M, generator=g).to(dev)
    params = [p.requires_grad_(True) for p in _random_params(M, P, L, individual, dev, seed)]
    vg = v.clone().requires_grad_(need_dx)
    y = Fn.dlinear(vg, *params, L, K, individual, diff=True, cf=cf)
    tgt = ops.dlinear_target(v, L, P, cf)
    loss = Fn.mse_loss(y, tgt)
    loss.backward()
    # fp64 restatement
    v64 = v.double().requires_grad_(True)
    p64 = [p.detach().double().requires_grad_(True) for p in params]
    y64 = R.apply(R.diff_inputs(v64, L, cf), *p64, K, individual)
    t64 = R.target(v64.detach(), L, P, cf)
    l64 = torch.nn.functional.mse_loss(y64, t64)
    l64.backward()
    assert rel(y, y64) <= 1e-5
    assert rel(tgt, t64) <= 1e-6
    assert abs(loss.item() - l64.item()) <= 1e-6 * abs(l64.item())
    for p, q in zip(params, p64):
        assert rel(p.grad, q.grad) <= 1e-5
    if need_dx:
        assert rel(vg.grad, v64.grad) <= 1e-5
    return params


@pytest.mark.parametrize("variant", list(R.VARIANTS))
def test_reference_size_against_fp64(dev, variant):
    individual, K, cf, _ = R.VARIANTS[variant]
    c, h, w = R.REF_LATENT
    _check_against_fp64(dev, 8, c * h * w // cf, R.TIN, R.TOUT, cf, K, individual, need_dx=False)


@pytest.mark.parametrize("individual", [False, True])
@pytest.mark.parametrize("cf", [1, 4])
def test_input_gradient(dev, individual, cf):
    _check_against_fp64(dev, 3, 70, R.TIN, R.TOUT, cf, 5 if cf > 1 else 3, individual)


@pytest.mark.parametrize("K", [1, 31, 53])
@pytest.mark.parametrize("individual", [False, True])
def test_edge_kernel_sizes(dev, K, individual):
    # K = 1 (trend = x), K > L (every row reaches both padded ends)
    _check_against_fp64(dev, 2, 100, R.TIN, R.TOUT, 1, K, individual)


@pytest.mark.parametrize("individual", [False, True])
@pytest.mark.parametrize("B,M", [(1, 100), (1, 257), (11, 65), (9, 9216)])
def test_edge_shapes(dev, B, M, individual):
    # M not a multiple of 64, B = 1, B above the 8-row register chunk
    _check_against_fp64(dev, B, M, R.TIN, R.TOUT, 1, 3, individual, need_dx=B < 9)


def test_series_decomp_modules(dev):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4, 13, 130, generator=g).to(dev).requires_grad_(True)
    s, t = D.series_decomp(5)(x)
    x64 = x.detach().double().requires_grad_(True)
    s64, t64 = R.decomp(x64, 5)
    assert rel(s, s64) <= 1e-6 and rel(t, t64) <= 1e-6
    assert rel(D.moving_avg(5, 1)(x), t64) <= 1e-6
    gs, gt = torch.randn_like(s), torch.randn_like(t)
    (s * gs + t * gt).sum().backward()
    (s64 * gs.double() + t64 * gt.double()).sum().backward()
    assert rel(x.grad, x64.grad) <= 1e-6


@pytest.mark.parametrize("individual", [False, True])
def test_gradients_bitwise_repeatable(dev, individual):
    M, L, P = 9216, R.TIN, R.TOUT
    g = torch.Generator().manual_seed(11)
    v = torch.randn(8, 25, M, generator=g).to(dev)
    params = _random_params(M, P, L, individual, dev, 5)
    dy = torch.randn(8, P, M, generator=g).to(dev)
    outs = []
    for _ in range(2):
        grads = [torch.empty_like(p) for p in params]
        ops.dlinear_bwd_weight(v, dy, grads[0], grads[1], grads[2], grads[3], L, P, 3, individual, True, 1)
        dv = ops.dlinear_bwd_data(dy, params[0], params[2], 25, L, 3, individual, True, 1)
        outs.append(grads + [dv])
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_forecast_layout(dev):
    g = torch.Generator().manual_seed(2)
    v = torch.randn(2, 25, 4, 3, 3, generator=g).to(dev)
    cfg = model_cfg("indc_indp", 9, 4)
    torch.manual_seed(0)
    model = D.Model(cfg).to(dev)
    fc = model.predict_latents(v)
    loss, pred, rows = model.latent_loss(v)
    want = pred.detach().view(2, 12, 4, 3, 3) + v[:, 12:13]
    assert fc.shape == (2, 12, 4, 3, 3) and rel(fc, want) <= 1e-6


def test_validation_step_metrics(dev):
    from weatherforecastingtoolkit_amd.pipeline import metrics
    cfg = model_cfg("sevir", 4096, 1)
    torch.manual_seed(0)
    model = D.Model(cfg, autoencoder=D.Autoencoder(128)).to(dev).eval()
    frames = torch.rand(1, 25, 128, 128, device=dev)
    loss, logs = model.validation_step(frames)
    keys = [k for k in logs if k != "val_loss"]
    assert len(keys) == 56 and all(k.startswith("val_") for k in keys)
    ref_keys = list(metrics.calc_metrics(torch.rand(1, 2, 1, 64, 64, device=dev),
                                         torch.rand(1, 2, 1, 64, 64, device=dev)))
    assert keys == [f"val_{k}" for k in ref_keys]
    assert torch.isfinite(loss) and logs["val_loss"] is loss
    tloss, tlogs = model.test_step(frames)
    assert sorted(tlogs) == sorted(["test_loss"] + [f"test_{k}" for k in ref_keys])


@pytest.mark.parametrize("variant,extra", [
    ("sevir", ["dlinear.enc_in=4096"]),
    ("ind", ["dlinear.enc_in=4096"]),
    ("indc_indp", ["dlinear.enc_in=64", "dlinear.features_per_step=64"]),
])
def test_experiment_scripts_run(dev, tmp_path, variant, extra):
    mod = __import__(f"weatherforecastingtoolkit_amd.experiments.v1_experiments.pretrained_ae_dlinear_{variant}.train",
                     fromlist=["main"])
    rc = mod.main(["--max-steps", "2", f"experiment_path={tmp_path}", "dataset.batch_size=1", *extra])
    assert rc == 0
    if variant != "sevir":   # dlinear_sevir defaults to the test pass, like the reference
        ck = torch.load(tmp_path / "outputs" / f"pretrained_ae_dlinear_{variant}" / "checkpoints" / "last.ckpt",
                        map_location="cpu")
        assert ck["global_step"] == 2 and "predictor.Linear_Seasonal.0.weight" in ck["state_dict"]
    rc = mod.main(["--max-steps", "1", "--mode", "fit" if variant == "sevir" else "test", f"experiment_path={tmp_path}",
                   "dataset.batch_size=1", *extra])
    assert rc == 0
