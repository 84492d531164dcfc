"""Torch-CPU restatement of the forecast-skill counts and CRPS sums (csrc/skill.hip, ops.skill_scores): the
semantics of the reference's pipeline/metrics.py:9-68, written from torch ops.  Pinned to tests/golden/g11_skill.npz
by tests/test_skill_cpu.py; the GPU tests use it at sizes too large for a fixture."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

PTYPE = {"none": 0, "avg": 1, "max": 2}


def _pool(x, ptype, s):
    """x (..., H, W) -> pooled like F.*_pool2d(s, stride=s) on the flattened planes"""
    if ptype == 0:
        return x
    h, w = x.shape[-2:]
    y = x.reshape(-1, 1, h, w)
    y = F.avg_pool2d(y, s, stride=s) if ptype == 1 else F.max_pool2d(y, s, stride=s)
    return y.reshape(x.shape[:-2] + y.shape[-2:])


def skill_scores(pred, target, thresholds, pools, clamp01):
    """pred (B, T, C, H, W) or (B, N, T, C, H, W), target (B, T, C, H, W) CPU fp32; pools [(type, scale)] with type a
    name or 0/1/2 -> (counts int64 (pools, thresholds, 3) = tp, fn, fp on the pooled ensemble mean; CRPS sums fp64
    (pools,); pooled cell counts int64 (pools,))"""
    if clamp01:
        pred, target = pred.clamp(0, 1), target.clamp(0, 1)
    ens = pred if pred.dim() == 6 else pred.unsqueeze(1)
    n = ens.shape[1]
    single = ens.mean(dim=1)
    thr = torch.tensor(np.asarray(thresholds, dtype=np.float32))
    counts, sums, cells = [], [], []
    for pt, s in pools:
        pt = PTYPE.get(pt, pt)
        s = 1 if pt == 0 else int(s)
        sp, tg = _pool(single, pt, s), _pool(target, pt, s)
        row = []
        for th in thr:
            p, t = sp >= th, tg >= th
            row.append([int((p & t).sum()), int((~p & t).sum()), int((p & ~t).sum())])
        counts.append(row)
        members = _pool(ens, pt, s)
        mean = members.mean(dim=1)
        std = members.std(dim=1) if n > 1 else torch.zeros_like(mean)
        eps = 1e-10
        normed = (mean - tg + eps) / (std + eps)
        cdf = 0.5 * (1 + torch.erf(normed / math.sqrt(2)))
        pdf = torch.exp(-(normed ** 2) / 2 - math.log(math.sqrt(2 * math.pi)))
        val = (std + eps) * (normed * (2 * cdf - 1) + 2 * pdf - 1 / math.sqrt(math.pi))
        sums.append(float(val.double().sum()))
        cells.append(val.numel())
    return (np.array(counts, dtype=np.int64).reshape(len(pools), len(thresholds), 3), np.array(sums),
            np.array(cells, dtype=np.int64))


def unpack(packed, n_thr):
    """host copy of ops.skill_scores -> the (counts, crps sums, cells) triple skill_scores returns"""
    packed = np.ascontiguousarray(packed, dtype=np.int64)
    counts = packed[:, :3 * n_thr].reshape(len(packed), n_thr, 3)
    sums = packed[:, 3 * n_thr].copy().view(np.float64)
    return counts, sums, packed[:, 3 * n_thr + 1].copy()


CASES = ["cont", "u8", "wide", "odd", "max", "ens"]
CALC_CASES = ["cont", "u8", "wide", "odd", "ens"]


def load_case(z, name):
    """one case of g11_skill.npz -> (pred, target, pools, clamp01); the quantised case is stored as uint8 (value / 255)"""
    pred, target = z[f"{name}_pred"], z[f"{name}_target"]
    if pred.dtype == np.uint8:
        pred, target = pred.astype(np.float32) / np.float32(255), target.astype(np.float32) / np.float32(255)
    pools = [(int(t), int(s)) for t, s in zip(z[f"{name}_ptype"], z[f"{name}_pscale"])]
    return torch.from_numpy(pred), torch.from_numpy(target), pools, bool(z[f"{name}_clamp"])
