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


class LeadVerification:
    """Scores per lead time of named fields ("forecast", "persistence", "reconstruction", ...) against the observed
    frames, kept over a pass in two device tables: `counts` int64 (P, F, 3 n_thr + 1) and `sums` float64 (P, F, 2), the
    layout of ops.verify_leads.  `add` is one launch pair without a host synchronisation, `merge` one all_reduce per table
    (two tensors, so that a plain sum is right for the integers and for the doubles), `result` one device-to-host copy.
    Totals over the leads are formed from the summed tables, never from the per-lead scores."""

    def __init__(self, names, pred_frames, thresholds=THRESHOLDS, device=None):
        self.names, self.pred_frames = tuple(names), int(pred_frames)
        self.thresholds = [float(t) for t in thresholds]
        if not 1 <= len(self.names) <= 4 or len(set(self.names)) != len(self.names):
            raise ValueError(f"LeadVerification: 1 to 4 distinct field names, got {self.names}")
        self.counts = self.sums = None
        if device is not None:
            self._allocate(device)

    def _allocate(self, device):
        p, f, nt = self.pred_frames, len(self.names), len(self.thresholds)
        self.counts = torch.zeros((p, f, 3 * nt + 1), dtype=torch.int64, device=device)
        self.sums = torch.zeros((p, f, 2), dtype=torch.float64, device=device)

    def reset(self):
        if self.counts is not None:
            self.counts.zero_()
            self.sums.zero_()

    def add(self, fields, target):
        """fields: {name: tensor} for every name (or the tensors in the order of `names`), target (B, P, ...): views as
        ops.verify_leads takes them; both sides are clamped to [0, 1] like calc_metrics' inputs"""
        if isinstance(fields, dict):
            if set(fields) != set(self.names):
                raise ValueError(f"LeadVerification.add: fields {sorted(fields)} are not {sorted(self.names)}")
            fields = [fields[n] for n in self.names]
        if len(fields) != len(self.names) or target.shape[1] != self.pred_frames:
            raise ValueError(f"LeadVerification.add: {len(fields)} fields against a target {tuple(target.shape)}, expected "
                             f"{len(self.names)} fields and {self.pred_frames} leads")
        if self.counts is None:
            self._allocate(target.device)
        ops.verify_leads(fields, target, self.thresholds, clamp01=True, out=(self.counts, self.sums))

    def merge(self, world):
        """sum the tables over the ranks; every rank calls it, also one whose pass held no batch"""
        if world > 1:
            import torch.distributed as dist
            if self.counts is None:
                self._allocate(torch.device("cuda", torch.cuda.current_device()))
            dist.all_reduce(self.counts)
            dist.all_reduce(self.sums)

    def _scores(self, counts, sums):
        """one field's dict from its count row (3 n_thr + 1) and its two sums"""
        nt, cells = len(self.thresholds), int(counts[-1])
        r = {"mse": float(sums[0]) / cells, "mae": float(sums[1]) / cells}
        pairs = [scores_from_counts(*counts[3 * i:3 * i + 3], cells) for i in range(nt)]
        for i, (c, h) in enumerate(pairs):
            r[f"csi_{i}"], r[f"hss_{i}"] = c, h
        if nt:
            r["csi_m"] = float(np.mean([c for c, _ in pairs]))
            r["hss_m"] = float(np.mean([h for _, h in pairs]))
        return r

    def _entry(self, counts, sums):
        """{name: scores} of one lead (or of the summed tables) and the MSE skill of every other field against
        persistence: "skill" for the first field, "skill_<name>" for the others; None where persistence has no error"""
        e = {n: self._scores(counts[f], sums[f]) for f, n in enumerate(self.names)}
        if "persistence" in self.names:
            base = e["persistence"]["mse"]
            others = [n for n in self.names if n != "persistence"]
            for n in others:
                e["skill" if n == others[0] else f"skill_{n}"] = None if base == 0 else 1.0 - e[n]["mse"] / base
        return e

    def result(self):
        """-> {"cells_per_lead", "leads": [{"lead": 1 .. P, <name>: {mse, mae, csi_i, hss_i, csi_m, hss_m}, "skill", ...}],
        "total": the same entry from the tables summed over the leads, "beats_persistence": the leads with skill > 0}, or
        {"skipped": reason} when the tables hold no cell"""
        if self.counts is None:
            return {"skipped": "no frames were verified (the pass held no batch of frames)"}
        nc = self.counts.numel()
        host = torch.cat([self.counts.reshape(-1).view(torch.float64), self.sums.reshape(-1)]).cpu().numpy()
        counts = host[:nc].view(np.int64).reshape(tuple(self.counts.shape))
        sums = host[nc:].reshape(tuple(self.sums.shape))
        if int(counts[:, :, -1].min()) == 0:
            return {"skipped": "no frames were verified (the pass held no batch of frames)"}
        leads = [dict(lead=p + 1, **self._entry(counts[p], sums[p])) for p in range(self.pred_frames)]
        out = {"cells_per_lead": int(counts[0, 0, -1]), "leads": leads, "total": self._entry(counts.sum(0), sums.sum(0))}
        if "persistence" in self.names and len(self.names) > 1:
            out["beats_persistence"] = [e["lead"] for e in leads if e["skill"] is not None and e["skill"] > 0]
        return out


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
