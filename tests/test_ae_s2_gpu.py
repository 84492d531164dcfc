"""GPU: the `ae_s2` experiment — the sequence posterior kernel (csrc/aekl.hip `aekl_posterior_seq_kernel`) against the
four-output posterior kernel bit for bit and against fp64, the sampled one-pass encode, the training and validation steps
against the reference's recorded values (tests/golden/g24_ae_s2.npz) and train.py end to end with an interrupted run.

Tolerance, per element:  max |a - a64| <= max(4 x spread, FLOOR) x max |a64|,  spread = the reference's own fp32 against
fp64 on the same inputs, recorded in the fixture; FLOOR = 2e-6 with the derivation of tests/test_ae_gan_train_gpu.py (32 ulp
of fp32: 2^-24 = 6e-8 per rounding, sqrt(10^3) x 6e-8 = 1.9e-6 for the longest accumulation chains of these cases).  The
kernel itself is held to the bound tests/test_aekl_gpu.py applies to the posterior: FLOOR in the same measure.

Measured on the MI355X, err / bound: the kernel against fp64 0.003 .. 0.048; z 0.19, for the one pass and for the per-frame
loop, which are bit-equal at this geometry (at the shipped one they are not: DESIGN.md names the K-split GEMM of the
attention's Linear layers); loss 0.011, forecast 0.12, the four gradients 0.13 .. 0.17, gradient norm 0.009; the three
optimiser steps 0.004 .. 0.022; val_loss 0.011, decoded forecast 0.15, decoded target 0.14; the metrics against the restated
frames at most 2.2e-7 of the 1e-3 they are allowed.
"""
from __future__ import annotations

import json
import os

import numpy as np
import pytest
import torch

from tests import ae_s2_ref as S
from tests.test_ae_s2_cpu import G24, frames_of, small_cfg
from weatherforecastingtoolkit_amd import ops
from weatherforecastingtoolkit_amd._lib import WfaeError
from weatherforecastingtoolkit_amd.experiments.ae_s2 import train as T
from weatherforecastingtoolkit_amd.pipeline import helpers, metrics

pytestmark = pytest.mark.gpu

FLOOR = 2e-6


@pytest.fixture(scope="module")
def g24():
    return np.load(G24, allow_pickle=False)


def ratio(what, got, ref64, spread_, scale=None):
    """err / bound of `got` against the recorded fp64 value, in the per-element measure of the module docstring"""
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref64).double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bound = max(4.0 * float(spread_), FLOOR)
    err = float((got - ref).abs().max() / (scale if scale is not None else ref.abs().max()))
    print(f"{what}: err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
    return err / bound


# ------------------------------------------------------------------------------------------------ the kernel
# (B, T, C, h, w, element offset of the three buffers).  h*w = 25: the scalar path, B != T so a transposed index shows, 450
# elements = two blocks; h*w = 16: the 16-byte path inside one block; 3072 elements: three blocks of 16-byte accesses; the
# same off 16-byte alignment: the scalar path although h*w % 4 == 0; the last two run past the grid's 2048 blocks, so the
# grid-stride loop takes a second turn (scalar: > 524288 elements, 16-byte: > 2097152)
SEQ_CASES = [(2, 3, 3, 5, 5, 0), (3, 2, 4, 4, 4, 0), (2, 3, 8, 8, 8, 0), (2, 3, 8, 8, 8, 1), (2, 3, 4, 211, 209, 0),
             (2, 3, 16, 152, 152, 0)]


def _offset(t, off, dev):
    """`t` on the device in a buffer that starts `off` elements past an allocation: contiguous, and off 16-byte alignment"""
    buf = torch.empty(t.numel() + off, dtype=torch.float32, device=dev)
    view = buf[off:].view(t.shape)
    view.copy_(t)
    return view


@pytest.mark.parametrize("case", SEQ_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_posterior_seq_kernel(dev, case):
    b, t, c, h, w, off = case
    g = torch.Generator().manual_seed(b * 1000 + h)
    mom = torch.randn(b * t, 2 * c, h, w, generator=g) * 4
    mom[0, c, 0, :4] = torch.tensor([-40.0, -30.0, 20.0, 40.0])          # logvar at and beyond both clamps
    mom[-1, 2 * c - 1, -1, -2:] = torch.tensor([40.0, -40.0])
    noise = torch.randn(t, b, c, h, w, generator=g)
    md, nd = _offset(mom, off, dev), _offset(noise, off, dev)
    assert (md.data_ptr() % 16 == 0) == (off == 0)
    z = ops.aekl_posterior_seq(md, nd)
    again = ops.aekl_posterior_seq(md, nd)
    assert z.shape == (b, t, c, h, w)
    # the four-output kernel on the noise permuted to frame order: the same bits
    permuted = noise.permute(1, 0, 2, 3, 4).reshape(b * t, c, h, w).contiguous().to(dev)
    four = ops.aekl_posterior(mom.to(dev), permuted)[3]
    assert torch.equal(z.view(b * t, c, h, w), four)
    assert torch.equal(z, again)
    m64 = mom.double().view(b, t, 2 * c, h, w)
    want = m64[:, :, :c] + torch.exp(0.5 * m64[:, :, c:].clamp(-30.0, 20.0)) * noise.double().transpose(0, 1)
    err = float((z.double().cpu() - want).abs().max() / want.abs().max())
    print(f"posterior_seq {case}: err {err:.3e} bound {FLOOR:.1e} ratio {err / FLOOR:.3f}")
    assert err <= FLOOR


def test_posterior_seq_refuses_bad_arguments(dev):
    mom, noise = torch.zeros(6, 8, 4, 4, device=dev), torch.zeros(3, 2, 4, 4, 4, device=dev)
    with pytest.raises(WfaeError, match="does not fit"):
        ops.aekl_posterior_seq(mom, noise[:2].contiguous())
    with pytest.raises(WfaeError, match="expected moments"):
        ops.aekl_posterior_seq(mom, noise.view(6, 4, 4, 4))
    with pytest.raises(WfaeError, match="device tensors"):
        ops.aekl_posterior_seq(mom.cpu(), noise.cpu())


# ------------------------------------------------------------------------------------------------ the sampled encode
@pytest.fixture(scope="module")
def model(dev, g24):
    """the experiment's Model at the fixture's geometry, on the fixture's weights: the provider's seeded initialisation and
    the predictor after the fixture's DLinear seed"""
    torch.manual_seed(int(g24["seed"]) + 1)
    m = T.Model(small_cfg(seed=int(g24["seed"]))).to(dev)
    m.autoencoder.eval()
    return m


@pytest.fixture(scope="module")
def latents(dev, g24, model):
    """z of the four recorded encodes, one pass each with the recorded noise"""
    frames, noise = frames_of(g24).to(dev), torch.from_numpy(g24["noise"]).to(dev)
    return [model.autoencoder.encode(frames, noise=noise[i]) for i in range(4)]


def test_sampled_encode_against_the_reference(dev, g24, model, latents):
    """one pass over the B*T = 26 frames (chunk_frames: 0) and the reference's loop over T, both against the recorded z"""
    ae = model.autoencoder
    assert ae.sample and ae.chunk_frames == 0
    frames, noise = frames_of(g24).to(dev), torch.from_numpy(g24["noise"]).to(dev)
    loop = torch.stack([ae.autoencoder.encode(frames[:, t].contiguous()).sample(noise=noise[0, t]) for t in range(frames.shape[1])], 1)
    worst = {"one pass": ratio("z, one pass", latents[0], g24["z"], g24["z_spread"]),
             "per-frame loop": ratio("z, per-frame loop", loop, g24["z"], g24["z_spread"])}
    same = torch.equal(latents[0], loop)
    diff = float((latents[0] - loop).abs().max())
    print(f"one pass and per-frame loop bit-equal: {same} (max |difference| {diff:.3e})")
    assert max(worst.values()) <= 1.0, worst
    # the default draw: T calls of randn((B, C, h, w)) from the device generator, in frame order
    gen = torch.Generator(device=dev).manual_seed(5)
    drawn = ae.encode(frames, generator=gen)
    ref = torch.Generator(device=dev).manual_seed(5)
    want = torch.stack([torch.randn((2, 4, 8, 8), generator=ref, device=dev) for _ in range(frames.shape[1])])
    assert torch.equal(drawn, ae.encode(frames, noise=want))
    torch.manual_seed(9)
    a = ae.encode(frames)
    torch.manual_seed(9)
    assert torch.equal(a, ae.encode(frames)) and not torch.equal(a, drawn)


# ------------------------------------------------------------------------------------------------ the steps
def test_training_step_against_the_reference(dev, g24, model, latents):
    """loss, forecast and predictor gradients of one step on the recorded noise"""
    cols = torch.from_numpy(g24["columns"]).to(dev)
    p = model.predictor
    loss, pred, _ = model.latent_loss(latents[0])
    loss.backward()
    grads = {"grad_seasonal_w": p.seasonal_weight.grad, "grad_seasonal_b": p.seasonal_bias.grad,
             "grad_trend_w": p.trend_weight.grad, "grad_trend_b": p.trend_bias.grad}
    worst = {"loss": ratio("loss", loss.detach(), g24["loss"], g24["loss_spread"]),
             "pred": ratio("pred", pred.detach()[..., cols], g24["pred"], g24["pred_spread"])}
    for name, gr in grads.items():
        worst[name] = ratio(name, gr[cols], g24[name], g24[name + "_spread"])
    gn = torch.sqrt(sum((gr.double() ** 2).sum() for gr in grads.values()))
    worst["grad_norm"] = ratio("grad_norm", gn, g24["grad_norm"], g24["grad_norm_spread"])
    assert p.decoder_weight.grad is None
    p.zero_grad(set_to_none=True)
    print("worst ratio", max(worst.values()), max(worst, key=worst.get))
    assert max(worst.values()) <= 1.0, worst


def test_three_optimiser_steps_against_the_reference(dev, g24, latents):
    """clip + AdamW with betas (0.8, 0.95) at a constant learning rate, on the noise of the recorded encodes 1 .. 3"""
    torch.manual_seed(int(g24["seed"]) + 1)
    model = T.Model(small_cfg(seed=int(g24["seed"]))).to(dev).train()
    model.configure_optimizers()
    assert tuple(model.opt.param_groups[0]["betas"]) == tuple(float(v) for v in g24["betas"])
    losses = [float(model.train_latents(latents[i])[0]) for i in (1, 2, 3)]
    worst = [ratio(f"step {i + 1} loss", torch.tensor(got), torch.tensor(g24["step_loss"][i]), g24["step_loss_spread"])
             for i, got in enumerate(losses)]
    assert max(worst) <= 1.0, worst


def test_validation_step_against_the_reference(dev, g24, model, latents):
    """val_loss, the decoded forecast and target, calc_metrics' keys, and its values against the same metrics of the
    recorded fp64 frames.  The metrics' bound: the two pairs of images differ per element by at most the decoded bound,
    d = 1.1e-5 of the largest value; CRPS, SSIM and PSNR are averages over 12288 pixels whose terms move by a few d, so
    1e-3 relative leaves a factor of ten; CSI and HSS move only if a pixel lies within d of a threshold, and by one count"""
    z = latents[0]
    loss, logs = model.validate_latents(z, 0, "val")
    keys = metrics.metric_keys()
    assert list(logs) == ["val_loss"] + ["val_" + k for k in keys]
    fc = model.predict_latents(z)
    tgt = z[:, S.TIN:]
    dp, dt = model.autoencoder.decode(fc), model.autoencoder.decode((tgt - z[:, S.TIN - 1:S.TIN]) + z[:, S.TIN - 1:S.TIN])
    assert dp.shape == dt.shape == (2, S.TOUT, 1, S.FRAME, S.FRAME)
    worst = {"val_loss": ratio("val_loss", loss, g24["val_loss"], g24["val_loss_spread"]),
             "decoded_pred": ratio("decoded_pred", dp, g24["decoded_pred"], g24["decoded_pred_spread"]),
             "decoded_tgt": ratio("decoded_tgt", dt, g24["decoded_tgt"], g24["decoded_tgt_spread"])}
    assert max(worst.values()) <= 1.0, worst
    want = helpers.log_metrics(torch.from_numpy(g24["decoded_pred"]).to(dev), torch.from_numpy(g24["decoded_tgt"]).to(dev), "val")
    bad = {}
    for k, v in want.items():
        err = abs(float(logs[k]) - float(v)) / max(1.0, abs(float(v)))
        print(f"{k}: {float(logs[k]):.6g} restated {float(v):.6g} err {err:.2e}")
        if not err <= 1e-3:
            bad[k] = (float(logs[k]), float(v))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ train.py
OVER = ["ae_kl.block_out_channels=[32,64,64]", "ae_kl.down_block_types=[DownEncoderBlock2D,DownEncoderBlock2D,DownEncoderBlock2D]",
        "ae_kl.up_block_types=[UpDecoderBlock2D,UpDecoderBlock2D,UpDecoderBlock2D]", "ae_kl.layers_per_block=1",
        "ae_kl.latent_channels=4", "ae_kl.norm_num_groups=8", "dlinear.enc_in=4096", "dataset.batch_size=2",
        "trainer.log_every_n_steps=1", "trainer.save_every_n_steps=1.0"]


def run_main(capsys, argv):
    capsys.readouterr()
    assert T.main(argv) == 0
    out = capsys.readouterr().out.splitlines()
    print("\n".join(out))
    assert out and out[-1] == "done"
    return [json.loads(line) for line in out if line.startswith("{")], out


def last_ckpt(path):
    return torch.load(os.path.join(str(path), "outputs", "ae_s2_dlinear", "checkpoints", "last.ckpt"), map_location="cpu",
                      weights_only=False)


def test_train_end_to_end(dev, tmp_path, capsys):
    """two training steps on synthetic events, then the validation pass and — by default, as the reference's __main__ —
    the test pass; last.ckpt holds the reference's predictor keys"""
    logs, out = run_main(capsys, ["--max-steps", "2", "--validate", *OVER, f"experiment_path={tmp_path}"])
    assert any("seeded initialisation" in line for line in out)
    assert [log.get("step") for log in logs[:3]] == [1, 2, 2] and len(logs) == 4
    assert {"train_loss", "grad_norm", "lr", "sequences_per_s"} <= set(logs[0])
    val, test = logs[2], logs[3]
    assert "val_loss" in val and "val_SSIM" in val and val["batches"] >= 1
    assert "test_loss" in test and "test_SSIM" in test and test["batches"] >= 1
    assert all(np.isfinite(v) for log in logs for v in log.values())
    ck = last_ckpt(tmp_path)
    keys = list(ck["state_dict"])
    assert ck["global_step"] == 2 and len(keys) == 3 * 4096 * 2
    assert keys[0] == "predictor.Linear_Seasonal.0.weight" and keys[-1] == "predictor.Linear_Decoder.4095.bias"


def test_train_on_a_sevir_store(dev, tmp_path, capsys):
    """--data-dir: the `sevir_lr` store through SEVIRLightningDataModule in the reference's 'NTCHW' layout (the config has
    no aug_mode / val_ratio / seed: the DataModule's defaults) — one step, the validation pass, the test pass"""
    from tests.test_v1_run_cpu import STAMPS, write_store
    store = str(tmp_path / "sevir")
    write_store(store, STAMPS)
    logs, out = run_main(capsys, ["--max-steps", "1", "--data-dir", store, *OVER, f"experiment_path={tmp_path}"])
    assert len(logs) == 3 and logs[0]["step"] == 1 and "train_loss" in logs[0]
    assert "val_loss" in logs[1] and logs[1]["batches"] >= 1 and "test_loss" in logs[2] and logs[2]["batches"] >= 1
    assert all(np.isfinite(v) for log in logs for v in log.values())


def test_resume_is_bit_exact(dev, tmp_path, capsys):
    """A: two steps.  B: the same run stopped after one, then resumed.  The latent noise comes from the device generator,
    seeded by the driver and carried by the checkpoint: losses and parameters are equal bit for bit"""
    common = ["--max-steps", "2", "--no-test", *OVER]
    a, _ = run_main(capsys, [*common, f"experiment_path={tmp_path / 'a'}"])
    b1, _ = run_main(capsys, [*common, "--stop-after", "1", f"experiment_path={tmp_path / 'b'}"])
    assert last_ckpt(tmp_path / "b")["global_step"] == 1
    b2, _ = run_main(capsys, [*common, "--resume", f"experiment_path={tmp_path / 'b'}"])
    assert [log["step"] for log in a] == [1, 2] and [log["step"] for log in b1 + b2] == [1, 2]
    for x, y in zip(a, b1 + b2):
        assert x["train_loss"] == y["train_loss"] and x["lr"] == y["lr"], (x, y)
    assert a[0]["train_loss"] != a[1]["train_loss"]
    ca, cb = last_ckpt(tmp_path / "a"), last_ckpt(tmp_path / "b")
    assert ca["global_step"] == cb["global_step"] == 2 and list(ca["state_dict"]) == list(cb["state_dict"])
    for k, v in ca["state_dict"].items():
        assert torch.equal(v, cb["state_dict"][k]), k
