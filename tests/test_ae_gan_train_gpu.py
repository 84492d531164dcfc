"""GPU tests of training the ae_gan residual autoencoders: the backward kernels of csrc/resae_bwd.hip per element against
fp64 on both routes, the dead-tap and same-bits properties, the join, the blocks and the whole ConvAutoencoderBIG against
tests/ae_gan_train_ref.py and tests/golden/g22_ae_gan_train.npz, the caches, the step and the fit entry point.

Tolerance, per element:  max |a - a64| <= max(4 x spread, FLOOR) x max |a64|,  spread = torch's own fp32 against fp64 on
the same inputs (the project's convention, tests/test_ae_gan_gpu.py).  FLOOR = 2e-6 is 32 ulp of fp32 (2^-24 = 6e-8 per
rounding; the longest fp32 accumulation chain of these cases, ~10^3 terms in two levels, gives sqrt(10^3) x 6e-8 = 1.9e-6):
it only matters where torch's fp32 happens to be exact.  Measured on the MI355X: the kernel and join cases reach at most
0.25 of their bound (errors 2e-8 .. 5e-7, so the floor is what binds there), the blocks and the whole model against G22 at
most 0.32 of max(4 x recorded spread, FLOOR), the five losses of the step test 0.09 .. 0.74 of 4 x the recorded spread
("Training the residual autoencoders").
"""
from __future__ import annotations

import pytest
import torch

from tests import ae_gan_ref as R
from tests import ae_gan_train_ref as T

pytestmark = pytest.mark.gpu

FLOOR = 2e-6

# (kind, N, Cin, Cout, H, W) of the forward layer.  Channel counts cross 16 / 32 / 64; planes 1x1, 2x2, 3x3, 4x4, 5x5 (odd,
# stride 2), 8x8 -> 4x4; N = 5 at 4x4 is 80 columns: a second column group that starts inside a sample.
SMALL = [
    (0, 3, 5, 7, 1, 1), (0, 2, 24, 20, 2, 2), (0, 2, 40, 72, 3, 3), (0, 5, 24, 20, 4, 4), (0, 5, 40, 72, 4, 4),
    (1, 3, 24, 72, 2, 2), (1, 2, 5, 20, 5, 5), (1, 2, 40, 7, 8, 8), (1, 5, 24, 40, 8, 8),
    (2, 2, 24, 7, 1, 1), (2, 3, 5, 72, 2, 2), (2, 5, 40, 20, 2, 2),
    (3, 3, 5, 7, 1, 1), (3, 2, 40, 20, 4, 4), (3, 5, 24, 72, 4, 4),
    (4, 2, 24, 72, 5, 5), (4, 2, 40, 7, 8, 8), (4, 3, 5, 20, 2, 2),
]
# the tile route: the same small planes (it serves any shape) and planes that cross the 8 x 8 tile in both directions, odd
TILE = [
    (0, 2, 5, 7, 1, 1), (0, 2, 40, 72, 3, 3), (0, 2, 24, 20, 11, 19),
    (1, 2, 5, 20, 5, 5), (1, 2, 24, 72, 21, 37), (1, 2, 40, 7, 16, 18),
    (2, 2, 24, 7, 1, 1), (2, 2, 40, 20, 9, 11), (2, 2, 5, 72, 5, 4),
    (3, 2, 40, 20, 4, 4), (3, 2, 24, 72, 11, 19),
    (4, 2, 24, 72, 5, 5), (4, 2, 40, 7, 21, 35),
]
CASES = [("small",) + c for c in SMALL] + [("tile",) + c for c in TILE]
IDS = [f"{c[0]}-k{c[1]}-n{c[2]}-{c[3]}to{c[4]}-{c[5]}x{c[6]}" for c in CASES]


def _inputs(kind, n, cin, cout, h, w, seed=7):
    x, wt, _, _, _ = R.unit_inputs(kind, n, cin, cout, h, w, seed)
    ho, wo = R.out_plane(kind, h, w)
    g = torch.Generator().manual_seed(seed + 1)
    dy = torch.randn(n, cout, ho, wo, generator=g)
    add = torch.randn(n, cin, h, w, generator=g)
    return x, wt, dy, add


def _close(what, got, ref64, ref32):
    got = got.detach().double().cpu()
    bound = max(4.0 * R.spread(ref32, ref64), FLOOR)
    err = float((got - ref64).abs().max() / ref64.abs().max().clamp_min(1e-300))
    print(f"{what}: err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
    assert err <= bound, (what, err, bound)


@pytest.mark.parametrize("route,kind,n,cin,cout,h,w", CASES, ids=IDS)
def test_data_gradient_per_element(dev, route, kind, n, cin, cout, h, w):
    from weatherforecastingtoolkit_amd import ops
    x, wt, dy, add = _inputs(kind, n, cin, cout, h, w)
    dx64, _, _ = T.unit_grads(x.double(), wt.double(), kind, dy.double())
    dx32, _, _ = T.unit_grads(x, wt, kind, dy)
    pt = ops.resae_bwd_pack(wt.to(dev), kind)
    dyd = dy.to(dev)
    got = ops.resae_bwd_data(dyd, pt, x.shape, route=route)
    _close("dx", got, dx64, dx32)
    again = ops.resae_bwd_data(dyd, pt, x.shape, route=route)
    assert torch.equal(got, again)                       # two launches, the same bits
    with_add = ops.resae_bwd_data(dyd, pt, x.shape, add=add.to(dev), route=route)
    _close("dx + add", with_add, dx64 + add.double(), dx32 + add)
    if kind == 4:                                        # exact zeros at the positions no output reads
        assert float(got[:, :, 1::2, :].abs().max() if h > 1 else 0.0) == 0.0
        assert float(got[:, :, :, 1::2].abs().max() if w > 1 else 0.0) == 0.0


@pytest.mark.parametrize("route,kind,n,cin,cout,h,w", CASES, ids=IDS)
def test_weight_gradient_per_element(dev, route, kind, n, cin, cout, h, w):
    from weatherforecastingtoolkit_amd import ops
    x, wt, dy, _ = _inputs(kind, n, cin, cout, h, w)
    _, dw64, db64 = T.unit_grads(x.double(), wt.double(), kind, dy.double(), bias=True)
    _, dw32, db32 = T.unit_grads(x, wt, kind, dy, bias=True)
    xd, dyd = x.to(dev), dy.to(dev)
    dw = torch.full_like(wt, 7.0, device=dev)            # written, not accumulated
    ops.resae_bwd_weight(dyd, xd, dw, kind, route=route)
    _close("dw", dw, dw64, dw32)
    for ky, kx in T.dead_taps(kind, h, w):               # exact zeros, not small numbers
        assert float(dw[:, :, ky, kx].abs().max()) == 0.0
    dw2, db = torch.full_like(dw, -3.0), torch.full((cout,), 5.0, device=dev)
    ops.resae_bwd_weight(dyd, xd, dw2, kind, dbias=db, route=route)
    assert torch.equal(dw, dw2)                          # two launches, the same bits; dbias changes nothing
    _close("dbias", db, db64, db32)


@pytest.mark.parametrize("kind,n,cin,cout,h,w", [c for c in SMALL if c[0] < 3 and T.dead_taps(c[0], c[4], c[5])],
                         ids=lambda v: str(v))
def test_dead_taps_never_reach_the_data_gradient(dev, kind, n, cin, cout, h, w):
    from weatherforecastingtoolkit_amd import ops
    x, wt, dy, _ = _inputs(kind, n, cin, cout, h, w)
    dyd = dy.to(dev)
    clean = ops.resae_bwd_data(dyd, ops.resae_bwd_pack(wt.to(dev), kind), x.shape, route="small")
    for ky, kx in T.dead_taps(kind, h, w):
        wt[:, :, ky, kx] = 1e30
    dirty = ops.resae_bwd_data(dyd, ops.resae_bwd_pack(wt.to(dev), kind), x.shape, route="small")
    assert torch.equal(clean, dirty)


def test_data_gradient_finishing_launch_above_2_20_outputs(dev):
    """K split in two (Cout = 40 is two chunks, 275 column groups x one slab ask for two splits) and 64 x 1100 x 16 =
    1 126 400 elements of dx: the finishing launch indexes past 2^20"""
    from weatherforecastingtoolkit_amd import ops
    kind, n, cin, cout, h, w = 0, 1100, 64, 40, 4, 4
    assert n * cin * h * w > 1 << 20
    x, wt, dy, add = _inputs(kind, n, cin, cout, h, w)
    dx64, _, _ = T.unit_grads(x.double(), wt.double(), kind, dy.double())
    dx32, _, _ = T.unit_grads(x, wt, kind, dy)
    got = ops.resae_bwd_data(dy.to(dev), ops.resae_bwd_pack(wt.to(dev), kind), x.shape, add=add.to(dev), route="small")
    _close("dx + add", got, dx64 + add.double(), dx32 + add)


JOIN = [(False, False, 3, 7, 5, 3), (True, False, 2, 21, 4, 6), (False, True, 3, 7, 6, 2), (True, True, 2, 33, 4, 10)]


@pytest.mark.parametrize("affine,res_up,n,c,h,w", JOIN, ids=lambda v: str(v))
def test_join_forward_and_backward(dev, affine, res_up, n, c, h, w):
    from weatherforecastingtoolkit_amd import ops
    g = torch.Generator().manual_seed(11)
    c2, dy = torch.randn(n, c, h, w, generator=g), torch.randn(n, c, h, w, generator=g)
    r = torch.randn((n, c, h // 2, w // 2) if res_up else (n, c, h, w), generator=g)
    s2, ss = (0.75 + 0.5 * torch.rand(c, generator=g) for _ in range(2))
    h2, hs = (0.2 * torch.randn(c, generator=g) for _ in range(2))
    aff = (ss, hs) if affine else (None, None)
    d = lambda t: None if t is None else t.to(dev)
    f64 = lambda t: None if t is None else t.double()
    args32, args64 = (c2, s2, h2, r) + aff, tuple(f64(t) for t in (c2, s2, h2, r) + aff)
    y = ops.resae_join_fwd(*(d(t) for t in args32), res_up=res_up)
    _close("y", y, T.join(*args64, res_up=res_up), T.join(*args32, res_up=res_up))
    dpre, dres = ops.resae_join_bwd(d(dy), *(d(t) for t in args32), res_up=res_up)
    p64, r64 = T.join_grads(dy.double(), *args64, res_up=res_up)
    p32, r32 = T.join_grads(dy, *args32, res_up=res_up)
    _close("dpre", dpre, p64, p32)
    _close("dres", dres, r64, r32)
    dpre2, dres2 = ops.resae_join_bwd(d(dy), *(d(t) for t in args32), res_up=res_up)
    assert torch.equal(dpre, dpre2) and torch.equal(dres, dres2)


# ------------------------------------------------------------------------------------------------------------ blocks
# (Cin, Cout, stride, up, N, H, W): with and without a shortcut convolution, on both routes
BLOCKS = [(5, 7, 1, False, 3, 6, 5), (6, 6, 1, False, 3, 3, 3), (5, 9, 2, False, 2, 7, 7), (5, 9, 2, False, 2, 12, 10),
          (6, 6, 1, True, 2, 2, 2), (5, 7, 1, True, 2, 5, 6), (8, 4, 1, True, 3, 1, 1)]


@pytest.mark.parametrize("cin,cout,stride,up,n,h,w", BLOCKS, ids=lambda v: str(v))
def test_block_training_against_the_restatement(dev, cin, cout, stride, up, n, h, w):
    from weatherforecastingtoolkit_amd.experiments.v1_experiments import _ae_gan as M
    g = torch.Generator().manual_seed(5)
    sd = R.block_state("", cin, cout, stride, g)
    x = torch.randn(n, cin, h, w, generator=g)
    ho, wo = (2 * h, 2 * w) if up else R.out_plane(1 if stride == 2 else 0, h, w)
    dy = torch.randn(n, cout, ho, wo, generator=g)
    y64, g64, dx64, new64 = T.block_train(sd, x, dy, stride, up, torch.float64)
    y32, g32, dx32, new32 = T.block_train(sd, x, dy, stride, up, torch.float32)

    mod = M.UpsampleBlock(cin, cout) if up else M.ResidualBlock(cin, cout, stride)
    blk = mod.resblock if up else mod
    blk.load_state_dict(sd)
    mod.unfreeze().to(dev).train()
    assert all(p.requires_grad for p in mod.parameters())
    xd = x.to(dev).requires_grad_(True)
    y = mod(xd)
    y.backward(dy.to(dev))
    _close("y", y, y64, y32)
    _close("dx", xd.grad, dx64, dx32)
    params = dict(blk.named_parameters())
    for k in g64:
        _close("d " + k, params[k].grad, g64[k], g32[k])
    out = blk.state_dict()
    for k in new64:
        if k.endswith("num_batches_tracked"):
            assert int(out[k]) == int(new64[k]) == 4
        else:
            _close(k, out[k], new64[k], new32[k])
    # evaluation mode of the unfrozen block: the folded path on the UPDATED running statistics (the cache follows them)
    mod.eval()
    ref_eval = (R.upsample_block({"resblock." + k: v for k, v in R.cast(out, torch.float64).items()}, "", x.double().to(dev))
                if up else R.residual_block(R.cast(out, torch.float64), "", x.double().to(dev), stride)).cpu()
    got = mod(x.to(dev))
    assert not got.requires_grad
    assert float((got.double().cpu() - ref_eval).abs().max() / ref_eval.abs().max()) <= 1e-5


def test_single_value_per_channel_raises(dev):
    from weatherforecastingtoolkit_amd.experiments.v1_experiments import _ae_gan as M
    blk = M.ResidualBlock(4, 4).unfreeze().to(dev).train()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        blk(torch.zeros(1, 4, 1, 1, device=dev))


# ------------------------------------------------------------------------------------------- the whole model against G22
@pytest.fixture(scope="module")
def g22():
    from tests._util import golden
    return golden("g22_ae_gan_train")


def _big(dev):
    from tests._util import golden
    from weatherforecastingtoolkit_amd.experiments.v1_experiments import _ae_gan as M
    torch.manual_seed(R.SEED)
    big = M.ConvAutoencoderBIG()
    big.load_state_dict(R.golden_state(big, golden("g21_ae_gan")))
    return big.unfreeze().to(dev).train()


def _rel(what, got, ref, spread, scale=None):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double()
    bound = max(4.0 * float(spread), FLOOR)
    err = float((got - ref).abs().max() / (scale if scale is not None else ref.abs().max()))
    print(f"{what}: err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
    return err / bound


def test_big_forward_backward_against_g22(dev, g22):
    big = _big(dev)
    x, G = (t.to(dev) for t in T.golden_batch())
    recon, z = big(x)
    assert recon.requires_grad and z.requires_grad
    loss = (recon * G).mean()
    loss.backward()
    worst = {"loss": _rel("loss", loss.detach(), g22["loss"], g22["loss_spread"])}
    for name, t in (("z", z), ("recon", recon)):
        t = t.detach().flatten()
        if name + "_sample" in g22:
            worst[name] = _rel(name, t[R.sample_index(t.numel()).to(dev)], g22[name + "_sample"], g22[name + "_spread"])
            worst[name + " norm"] = _rel(name + " norm", t.double().norm(), g22[name + "_norm"], g22[name + "_spread"])
        else:
            worst[name] = _rel(name, t, g22[name].flatten(), g22[name + "_spread"])
    params = dict(big.named_parameters())
    off = g22["grad_offsets"]
    for i, k in enumerate(g22["grad_keys"]):
        gr = params[str(k)].grad.flatten()
        ref = g22["grad_samples"][off[i]:off[i + 1]]
        sp = g22["grad_spread"][i]
        worst["d " + str(k)] = max(_rel("d " + str(k), gr[T.grad_index(gr.numel()).to(dev)], ref, sp, scale=float(g22["grad_max"][i])),
                                   _rel("|d " + str(k) + "|", gr.double().norm(), g22["grad_norm"][i], sp))
    sd = big.state_dict()
    for name in ("running_mean", "running_var"):
        cat = torch.cat([sd[f"{p}.{name}"] for p in R.bn_prefixes(list(sd))])
        worst[name] = _rel(name, cat[R.sample_index(cat.numel()).to(dev)], g22[name + "_sample"], g22[name + "_spread"])
    bad = {k: v for k, v in worst.items() if v > 1.0}
    print("worst ratio", max(worst.values()), max(worst, key=worst.get))
    assert not bad, bad


# ---------------------------------------------------------------------------------------- the model: caches, step, fit
def _config(**over):
    import os
    from weatherforecastingtoolkit_amd import config as C
    from weatherforecastingtoolkit_amd.experiments.v1_experiments.ae_gan import train as TR
    cfg = C.load(os.path.join(TR.HERE, "config.yaml"))
    cfg.trainer.total_train_steps = 10
    cfg = C.merge(cfg, C.from_dotlist([f"{k}={v}" for k, v in over.items()]))
    cfg.lpips.disc_start = int(cfg.lpips.disc_start * cfg.trainer.total_train_steps)
    return cfg


def _model(dev):
    from tests._util import golden
    from weatherforecastingtoolkit_amd.experiments.v1_experiments import _ae_gan as M
    torch.manual_seed(R.SEED)
    model = M.Model(_config(), trainable=True)
    model.autoencoder.load_state_dict(R.golden_state(model.autoencoder, golden("g21_ae_gan")))
    model.to(dev).train()
    model.configure_optimizers()
    return M, model


def test_five_steps_against_g22_and_the_caches(dev, g22):
    M, model = _model(dev)
    x = T.golden_batch()[0].to(dev)
    probe = R.golden_input().to(dev)
    model.eval()
    before = model(probe)                     # fills the packed-weight and folded-statistics caches
    model.train()
    losses, ratios = [], []
    for i in range(T.STEPS):
        loss, gn = model.training_step(x)
        losses.append(float(loss))
        if i == 0:
            gn0 = float(gn)
            assert set(model.logs) >= {"train/total_loss", "train/rec_loss", "train/g_loss", "train/d_weight"}
            assert model.logs["train/g_loss"] == 0.0 and model.logs["train/d_weight"] == 0.0
            # caches: an evaluation forward after the step equals that of a fresh model loaded from the trained state
            model.eval()
            after = model(probe)
            fresh = M.Model(_config()).to(dev).eval()
            fresh.autoencoder.load_state_dict(model.autoencoder.state_dict())
            assert torch.equal(after, fresh(probe)) and not torch.equal(after, before)
            del fresh
            model.train()
    for i, (got, ref, sp) in enumerate(zip(losses, g22["step_loss"], g22["step_loss_spread"])):
        err = abs(got - ref) / abs(ref)
        print(f"step {i + 1}: loss {got:.8f} reference {ref:.8f} err {err:.3e} bound {4 * sp:.3e} ratio {err / (4 * sp):.3f}")
        ratios.append(err / (4 * sp))
    gerr = abs(gn0 - g22["step_grad_norm"]) / g22["step_grad_norm"]
    print(f"grad norm {gn0:.6f} reference {float(g22['step_grad_norm']):.6f} err {gerr:.3e} bound {4 * g22['step_grad_norm_spread']:.3e}")
    assert losses[-1] < losses[0]
    assert max(ratios) <= 1.0, ratios
    assert gerr <= 4 * g22["step_grad_norm_spread"]
    assert model.global_step == T.STEPS


def test_fit_entry_point_trains_two_steps_and_writes_a_checkpoint(dev, tmp_path):
    import json
    import os
    import subprocess
    import sys
    from weatherforecastingtoolkit_amd.experiments.v1_experiments import _ae_gan as M
    from tests._util import ROOT
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "weatherforecastingtoolkit_amd.experiments.v1_experiments.ae_gan.fit",
           "--max-steps", "2", f"experiment_path={tmp_path}"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 2 and r.stdout.strip().endswith("done")
    rec = [json.loads(ln) for ln in lines]
    assert [d["step"] for d in rec] == [1, 2] and all(d["train_loss"] > 0 and d["grad_norm"] > 0 for d in rec)
    ckpt = os.path.join(str(tmp_path), "outputs", "ae_conv_1024", "checkpoints", "last.ckpt")
    big = M.load_checkpoint(M.ConvAutoencoderBIG(), ckpt)
    assert int(big.enc1.bn1.num_batches_tracked) == 2
