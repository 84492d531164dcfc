"""CPU: forecast-skill scores (CRPS / CSI / HSS of pipeline/metrics.py) — the torch restatement tests/skill_ref.py and
the host half of calc_metrics against tests/golden/g11_skill.npz (recorded from the reference's own metrics.py), and
the host-side argument checks of wfae_skill_scores."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import skill_ref
from weatherforecastingtoolkit_amd import _lib
from weatherforecastingtoolkit_amd.pipeline import metrics as M

G11 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g11_skill.npz")


@pytest.fixture(scope="module")
def g11():
    return np.load(G11, allow_pickle=False)


@pytest.mark.parametrize("case", skill_ref.CASES)
def test_restatement_reproduces_g11(g11, case):
    pred, target, pools, clamp = skill_ref.load_case(g11, case)
    counts, sums, cells = skill_ref.skill_scores(pred, target, g11["thresholds"], pools, clamp)
    want = g11[f"{case}_counts"]
    np.testing.assert_array_equal(counts, want[..., :3])
    np.testing.assert_array_equal(cells[:, None] - counts.sum(-1), want[..., 3])
    np.testing.assert_allclose(sums / cells, g11[f"{case}_crps"], rtol=1e-5)


def test_fixture_has_exact_ties(g11):
    assert int(g11["u8_ties"]) > 0


@pytest.mark.parametrize("case", skill_ref.CASES)
def test_scores_from_counts_reproduce_g11(g11, case):
    counts = g11[f"{case}_counts"]
    for p in range(counts.shape[0]):
        for t in range(counts.shape[1]):
            tp, fn, fp, tn = (int(v) for v in counts[p, t])
            c, h = M.scores_from_counts(tp, fn, fp, tp + fn + fp + tn)
            assert c == g11[f"{case}_csi"][p, t], (p, t)
            assert h == g11[f"{case}_hss"][p, t], (p, t)


def _packed(counts, sums, cells):
    n_pools, n_thr = counts.shape[:2]
    out = np.zeros((n_pools, 3 * n_thr + 2), dtype=np.int64)
    out[:, :3 * n_thr] = counts.reshape(n_pools, -1)
    out[:, 3 * n_thr] = sums.astype(np.float64).view(np.int64)
    out[:, 3 * n_thr + 1] = cells
    return out


def test_metric_keys_are_the_reference_keys_in_order(g11):
    keys = [str(k) for k in g11["keys"]]
    assert len(keys) == 56
    assert M.metric_keys() == keys
    d = M.assemble_metrics(np.zeros((3, 20), dtype=np.int64) + np.array([0] * 18 + [0, 1]), 0.5, 20.0)
    assert list(d) == keys


@pytest.mark.parametrize("case", skill_ref.CALC_CASES)
def test_assembled_metrics_match_g11(g11, case):
    """calc_metrics' host half (assemble_metrics) on the restatement's counts: every key except SSIM / PSNR equals the
    reference's value (CRPS to 1e-5 relative); the four image-metric keys carry the values handed in"""
    pred, target, _, _ = skill_ref.load_case(g11, case)
    counts, sums, cells = skill_ref.skill_scores(pred, target, M.THRESHOLDS, M.POOLS, True)
    d = M.assemble_metrics(_packed(counts, sums, cells), 0.25, 30.0)
    want = dict(zip([str(k) for k in g11["keys"]], g11[f"{case}_metrics"]))
    for k, v in d.items():
        if k in ("SSIM", "PSNR", "paper_SSIM", "paper_PSNR"):
            assert v == (0.25 if "SSIM" in k else 30.0)
        elif "CRPS" in k:
            assert abs(v - want[k]) <= 1e-5 * abs(want[k]), k
        else:
            assert v == want[k], (k, v, want[k])


def _arr(ct, vals):
    return (ct * len(vals))(*vals)


def test_skill_scores_rejects_bad_arguments_without_gpu():
    """Null pointers, pool / threshold counts, pool types and scales, and short workspaces are rejected on the host
    before any launch (fake device addresses are never dereferenced)."""
    lib = _lib.load()
    P, Q, R, WS = 0x7F0000000000, 0x7F1000000000, 0x7F2000000000, 0x7F3000000000
    thr = _arr(ctypes.c_float, [0.1] * 9)
    ty, sc = _arr(ctypes.c_int, [0, 1, 1, 1]), _arr(ctypes.c_int, [1, 4, 16, 2])
    a = ctypes.addressof

    def call(pred=P, tgt=Q, out=R, B=2, N=1, TC=1, H=64, W=64, thr_p=a(thr), n_thr=6, types=a(ty), scales=a(sc),
             n_pools=3, ws=WS, ws_bytes=1 << 20):
        return lib.wfae_skill_scores(pred, tgt, out, B, N, TC, H, W, thr_p, n_thr, types, scales, n_pools, 1, ws,
                                     ws_bytes, None)

    assert call(pred=None) == -2 and b"null" in lib.wfae_last_error_string()
    assert call(tgt=None) == -2
    assert call(out=None) == -2
    assert call(n_pools=4) == -1
    assert call(n_pools=0) == -1
    assert call(n_thr=9) == -1
    assert call(thr_p=None) == -1
    assert call(types=None) == -1
    assert call(B=0) == -1
    assert call(N=0) == -1
    assert call(H=15) == -1 and b"scale" in lib.wfae_last_error_string()
    bad_type = _arr(ctypes.c_int, [0, 3, 1])
    assert call(types=a(bad_type)) == -1
    zero_scale = _arr(ctypes.c_int, [1, 0, 16])
    assert call(scales=a(zero_scale)) == -1
    assert call(ws=None) == -3
    assert call(ws_bytes=64) == -3
    assert lib.wfae_ensemble_mean(None, R, 2, 5, 4096, 1, None) == -2
    assert lib.wfae_ensemble_mean(P, R, 2, 0, 4096, 1, None) == -1


def test_skill_ops_have_no_cpu_fallback():
    from weatherforecastingtoolkit_amd import ops
    x = torch.zeros(1, 1, 1, 16, 16)
    with pytest.raises(_lib.WfaeError):
        ops.skill_scores(x, x, M.THRESHOLDS, M.POOLS)
    with pytest.raises(_lib.WfaeError):
        ops.ensemble_mean(torch.zeros(1, 2, 1, 1, 16, 16))
