"""The reference's pipeline/metrics.py on gfx950 kernels: SSIM / PSNR (:71-84) and the forecast-skill scores CRPS /
CSI / HSS (:9-68), assembled by calc_metrics (:86-133) into the reference's 56 keys in the reference's order.

Inputs are (b, t, c, h, w) — pred may be an ensemble (b, n, t, c, h, w) — in [0, 1] like the reference's
calc_metrics; SSIM is torchmetrics' StructuralSimilarityIndexMeasure(data_range=1.0) (11-tap Gaussian, sigma 1.5 —
numerically the valid-window form), PSNR is per-sample PeakSignalNoiseRatio() with
data_range = max(target) - min(target).  The contingency counts and CRPS sums of every pool come from one
csrc/skill.hip pass (ops.skill_scores); the counts equal the reference's bit for bit, and CSI / HSS are formed from
them on the host in fp32 with the reference's expressions (scores_from_counts).  calc_metrics launches SSIM, PSNR and
the skill pass on the stream and copies everything to the host once.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import ops

_eps = 1e-8
THRESHOLDS = [16 / 255, 74 / 255, 133 / 255, 160 / 255, 181 / 255, 219 / 255]
POOLS = [("none", 1), ("avg", 4), ("avg", 16)]          # calc_metrics' three poolings
_SUFFIX = ["", "_4", "_16"]
_PAPER_POOLS = [("POOL1", ""), ("POOL4", "_4"), ("POOL16", "_16")]


def _flat(x):
    b, t, c, h, w = x.shape
    return x.reshape(b * t * c, 1, h, w).contiguous()


def _pool(pool_type, scale):
    # the reference pools only for 'avg' / 'max'; any other pool_type means no pooling
    return (pool_type, int(scale)) if pool_type in ("avg", "max") else ("none", 1)


def _dense(x):
    return x.detach().contiguous()


def scores_from_counts(tp, fn, fp, cells):
    """(CSI, HSS) of one (pool, threshold) from its counts: reference :51 and :64-66 in fp32 arithmetic, as torch
    evaluates them on the fp32 sums of _hit_miss_fa_cn (tn = cells - tp - fn - fp).  Host only.  The fp32 conversion
    of a count is exact below 2^24 cells, where torch's sum is exact too."""
    f = np.float32
    tn = f(int(cells) - int(tp) - int(fn) - int(fp))
    tp, fn, fp, eps = f(tp), f(fn), f(fp), f(_eps)
    csi = tp / (tp + fn + fp + eps)
    num = f(2) * (tp * tn - fn * fp)
    den = (tp + fn) * (fn + tn) + (tp + fp) * (fp + tn) + eps
    return float(csi), float(num / den)


def metric_keys():
    """calc_metrics' keys in the reference's order (:97-131)."""
    keys = ["CRPS", "CRPS_4", "CRPS_16", "SSIM", "PSNR"]
    for i in range(len(THRESHOLDS)):
        keys += [f"CSI_{i}", f"CSI_{i}_4", f"CSI_{i}_16", f"HSS_{i}", f"HSS_{i}_4", f"HSS_{i}_16"]
    keys += ["paper_SSIM", "paper_PSNR", "paper_CRPS"]
    for name, _ in _PAPER_POOLS:
        keys += [f"paper_CSI_M_{name}", f"paper_CSI_181_{name}", f"paper_CSI_219_{name}", f"paper_HSS_{name}"]
    return keys


def assemble_metrics(skill, ssim_value, psnr_value):
    """calc_metrics' dict from the host copy of ops.skill_scores(pred, target, THRESHOLDS, POOLS, clamp01=True)
    (int64 (3, 20)) and the two image metrics.  Host only; the aggregates follow :120-131."""
    skill = np.asarray(skill, dtype=np.int64)
    nt = len(THRESHOLDS)
    r = {}
    crps = [float(skill[p, 3 * nt:3 * nt + 1].view(np.float64)[0] / skill[p, 3 * nt + 1]) for p in range(len(POOLS))]
    r["CRPS"], r["CRPS_4"], r["CRPS_16"] = crps
    r["SSIM"] = float(ssim_value)
    r["PSNR"] = float(psnr_value)
    for i in range(nt):
        csi, hss = [], []
        for p in range(len(POOLS)):
            c, h = scores_from_counts(*skill[p, 3 * i:3 * i + 3], skill[p, 3 * nt + 1])
            csi.append(c)
            hss.append(h)
        for p, sfx in enumerate(_SUFFIX):
            r[f"CSI_{i}{sfx}"] = csi[p]
        for p, sfx in enumerate(_SUFFIX):
            r[f"HSS_{i}{sfx}"] = hss[p]
    r["paper_SSIM"] = r["SSIM"]
    r["paper_PSNR"] = r["PSNR"]
    r["paper_CRPS"] = r["CRPS"]
    for name, sfx in _PAPER_POOLS:
        r[f"paper_CSI_M_{name}"] = float(np.mean([r[f"CSI_{i}{sfx}"] for i in range(nt)]))
        r[f"paper_CSI_181_{name}"] = r[f"CSI_4{sfx}"]
        r[f"paper_CSI_219_{name}"] = r[f"CSI_5{sfx}"]
        r[f"paper_HSS_{name}"] = float(np.mean([r[f"HSS_{i}{sfx}"] for i in range(nt)]))
    return r


def crps(pred, target, pool_type="none", scale=1):
    """reference pipeline/metrics.py:18-41 (pred (b, t, c, h, w) or an ensemble (b, n, t, c, h, w))"""
    s = ops.skill_scores(_dense(pred), _dense(target), [], [_pool(pool_type, scale)]).cpu().numpy()
    return float(s[0, 0:1].view(np.float64)[0] / s[0, 1])


def _counts(pred, target, threshold, pool_type, scale):
    if pred.dim() != 5:
        raise ValueError(f"csi / hss take a (b, t, c, h, w) forecast, got {tuple(pred.shape)}")
    return ops.skill_scores(_dense(pred), _dense(target), [threshold], [_pool(pool_type, scale)]).cpu().numpy()[0]


def csi(pred, target, threshold, pool_type="none", scale=1):
    """reference pipeline/metrics.py:43-52"""
    s = _counts(pred, target, threshold, pool_type, scale)
    return scores_from_counts(s[0], s[1], s[2], s[4])[0]


def hss(pred, target, threshold, pool_type="none", scale=1):
    """reference pipeline/metrics.py:54-67"""
    s = _counts(pred, target, threshold, pool_type, scale)
    return scores_from_counts(s[0], s[1], s[2], s[4])[1]


def ssim(pred, target):
    """reference pipeline/metrics.py:71-75"""
    return float(ops.ssim_fwd(_flat(target.detach()), _flat(pred.detach()), clamp01=False).item())


def psnr(pred, target):
    """reference pipeline/metrics.py:77-84"""
    return float(ops.psnr(_flat(pred.detach()), _flat(target.detach()), clamp01=False).item())


def calc_metrics(pred, target):
    """reference pipeline/metrics.py:86-133: clamp to [0,1] (:92-93, fused into the kernels), the ensemble mean
    `single` for 6-D pred (:94), SSIM / PSNR of `single`, CRPS / CSI / HSS of the three poolings; one device-to-host
    copy for the whole dict."""
    pred, target = _dense(pred), _dense(target)
    single = ops.ensemble_mean(pred, clamp01=True) if pred.dim() == 6 else pred
    p, g = _flat(single), _flat(target)
    s = ops.ssim_fwd(g, p, clamp01=True)
    q = ops.psnr(p, g, clamp01=True)
    k = ops.skill_scores(pred, target, THRESHOLDS, POOLS, clamp01=True)
    host = torch.cat([s.double().reshape(1), q.double().reshape(1), k.view(torch.float64).reshape(-1)]).cpu().numpy()
    return assemble_metrics(host[2:].view(np.int64).reshape(k.shape), host[0], host[1])
