"""GPU: forecast-skill scores (csrc/skill.hip) against tests/golden/g11_skill.npz, recorded from the reference's own
pipeline/metrics.py: contingency counts exactly (exact threshold ties and a 5-member ensemble included), CRPS to 1e-5,
CSI / HSS, the standalone crps / csi / hss, calc_metrics' 56 keys; at 32 x 384^2 against the torch restatement
tests/skill_ref.py; launch-to-launch repeatability; the ae_v2 validation step's logged keys."""
import os

import numpy as np
import pytest
import torch

from tests import skill_ref
from weatherforecastingtoolkit_amd import ops, synth
from weatherforecastingtoolkit_amd.pipeline import metrics as M

pytestmark = pytest.mark.gpu

G11 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g11_skill.npz")
IMAGE_KEYS = ("SSIM", "PSNR", "paper_SSIM", "paper_PSNR")


@pytest.fixture(scope="module")
def g11():
    return np.load(G11, allow_pickle=False)


@pytest.mark.parametrize("case", skill_ref.CASES)
def test_skill_scores_match_g11(dev, g11, case):
    pred, target, pools, clamp = skill_ref.load_case(g11, case)
    thr = g11["thresholds"]
    packed = ops.skill_scores(pred.to(dev), target.to(dev), thr, [(("none", "avg", "max")[t], s) for t, s in pools],
                              clamp01=clamp).cpu().numpy()
    counts, sums, cells = skill_ref.unpack(packed, len(thr))
    want = g11[f"{case}_counts"]
    np.testing.assert_array_equal(counts, want[..., :3])
    np.testing.assert_array_equal(cells[:, None] - counts.sum(-1), want[..., 3])
    np.testing.assert_allclose(sums / cells, g11[f"{case}_crps"], rtol=1e-5)
    for p in range(len(pools)):
        for t in range(len(thr)):
            c, h = M.scores_from_counts(*counts[p, t], cells[p])
            assert abs(c - g11[f"{case}_csi"][p, t]) <= 1e-6 and abs(h - g11[f"{case}_hss"][p, t]) <= 1e-6


@pytest.mark.parametrize("case", ["u8", "wide", "max", "ens"])
def test_standalone_functions_match_g11(dev, g11, case):
    """metrics.crps / csi / hss with the reference's signatures (they do not clamp: clamped cases get clamped input)"""
    pred, target, pools, clamp = skill_ref.load_case(g11, case)
    if clamp:
        pred, target = pred.clamp(0, 1), target.clamp(0, 1)
    pd, td = pred.to(dev), target.to(dev)
    single = ops.ensemble_mean(pd) if pd.dim() == 6 else pd
    for p, (t, s) in enumerate(pools):
        name = ("none", "avg", "max")[t]
        assert abs(M.crps(pd, td, name, s) - g11[f"{case}_crps"][p]) <= 1e-5 * g11[f"{case}_crps"][p]
        for i, th in enumerate(g11["thresholds"]):
            assert abs(M.csi(single, td, float(th), name, s) - g11[f"{case}_csi"][p, i]) <= 1e-6
            assert abs(M.hss(single, td, float(th), name, s) - g11[f"{case}_hss"][p, i]) <= 1e-6


@pytest.mark.parametrize("case", skill_ref.CALC_CASES)
def test_calc_metrics_match_g11(dev, g11, case):
    pred, target, _, _ = skill_ref.load_case(g11, case)
    d = M.calc_metrics(pred.to(dev), target.to(dev))
    keys = [str(k) for k in g11["keys"]]
    assert list(d) == keys
    want = dict(zip(keys, g11[f"{case}_metrics"]))
    for k in keys:
        if k in IMAGE_KEYS:
            continue
        tol = 1e-5 * abs(want[k]) if "CRPS" in k else 1e-6
        assert abs(d[k] - want[k]) <= tol, (k, d[k], want[k])
    # SSIM / PSNR: the existing kernels on the same clamped tensors (the ensemble mean of the clamped members for 6-D)
    pc, tc = pred.clamp(0, 1), target.clamp(0, 1)
    single = pc.mean(dim=1) if pc.dim() == 6 else pc
    p, g = M._flat(single.to(dev)), M._flat(tc.to(dev))
    assert d["SSIM"] == d["paper_SSIM"] == ops.ssim_fwd(g, p, clamp01=True).item()
    assert d["PSNR"] == d["paper_PSNR"] == ops.psnr(p, g, clamp01=True).item()


def test_ensemble_mean_is_torch_order(dev, g11):
    pred, _, _, _ = skill_ref.load_case(g11, "ens")
    assert torch.equal(ops.ensemble_mean(pred.to(dev)).cpu(), pred.mean(dim=1))
    assert torch.equal(ops.ensemble_mean((pred * 1.5 - 0.25).to(dev), clamp01=True).cpu(),
                       (pred * 1.5 - 0.25).clamp(0, 1).mean(dim=1))


def _blob_frames(seed):
    ev = synth.blob_events(32, 384, 1, seed=seed)                     # (32, 384, 384, 1) uint8
    return torch.from_numpy(ev.transpose(0, 3, 1, 2)[:, :, None].astype(np.float32) / np.float32(255))


@pytest.fixture(scope="module")
def blobs():
    return _blob_frames(21), _blob_frames(22)


def test_full_size_blobs_match_restatement(dev, blobs):
    """B = 32, T = 1, 384^2 VIL-like frames: every count exact, CRPS within 1e-5, for calc_metrics' pools and the
    max pools"""
    pred, target = blobs
    for pools in (M.POOLS, [("max", 4), ("max", 16), ("avg", 3)]):
        packed = ops.skill_scores(pred.to(dev), target.to(dev), M.THRESHOLDS, pools, clamp01=True).cpu().numpy()
        counts, sums, cells = skill_ref.unpack(packed, len(M.THRESHOLDS))
        rc, rs, rn = skill_ref.skill_scores(pred, target, M.THRESHOLDS, pools, True)
        np.testing.assert_array_equal(counts, rc)
        np.testing.assert_array_equal(cells, rn)
        np.testing.assert_allclose(sums / cells, rs / rn, rtol=1e-5)


def test_two_launches_bitwise_identical(dev, blobs):
    pred, target = (t.to(dev) for t in blobs)
    ens = torch.stack([pred, target.flip(-1), pred.flip(-2)], dim=1)
    for p in (pred, ens):
        a = ops.skill_scores(p, target, M.THRESHOLDS, M.POOLS, clamp01=True)
        b = ops.skill_scores(p, target, M.THRESHOLDS, M.POOLS, clamp01=True)
        assert torch.equal(a, b)


def test_validation_step_logs_every_metric_key(dev):
    from weatherforecastingtoolkit_amd import config as C
    from weatherforecastingtoolkit_amd.experiments.ae_v2 import train
    cfg = C.load(os.path.join(os.path.dirname(train.__file__), "config.yaml"), train.CARRIED_KEYS)
    cfg.trainer.total_train_steps = 10
    cfg.lpips.disc_start = 10
    torch.manual_seed(0)
    model = train.Model(cfg, img_size=128, variant="lin").to(dev).eval()
    x = torch.from_numpy(synth.uniform_frames(2, 128, seed=7)).to(dev)
    _, logs = model.validation_step({"vil": x}, 0)
    for k in M.metric_keys():
        assert f"val_{k}" in logs, k
        assert np.isfinite(logs[f"val_{k}"]), k
