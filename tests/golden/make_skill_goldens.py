"""Generate tests/golden/g11_skill.npz from the reference's own pipeline/metrics.py (CPU, fp32).

    python tests/golden/make_skill_goldens.py <reference checkout root>

The reference file imports torchmetrics at module level for SSIM / PSNR only; a stub module stands in for it so
the file loads by path, and its crps / csi / hss / _hit_miss_fa_cn / calc_metrics run unchanged.  For calc_metrics
the module's ssim / psnr are replaced with NaN stubs: the ordered key list and every other value come from the
reference.  Nothing from the reference is copied; the fixture holds inputs and recorded results only.

Per case `<c>`: `<c>_pred`, `<c>_target` (fp32, or uint8 for the quantised case: value = u8 / 255 in fp32),
`<c>_clamp`, `<c>_ptype` / `<c>_pscale` (0 none, 1 avg, 2 max), `<c>_thr` (fp64), `<c>_counts`
(pools x thresholds x [tp, fn, fp, tn], the tensors _hit_miss_fa_cn returned inside csi), `<c>_crps`, `<c>_csi`,
`<c>_hss` (the reference's float results) and, for calc_metrics cases, `<c>_metrics` (values in `keys` order).
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
THRESHOLDS = [16 / 255, 74 / 255, 133 / 255, 160 / 255, 181 / 255, 219 / 255]
CALC_POOLS = [("none", 1), ("avg", 4), ("avg", 16)]
PTYPE = {"none": 0, "avg": 1, "max": 2}


def load_reference(root):
    tm = types.ModuleType("torchmetrics")
    tmi = types.ModuleType("torchmetrics.image")
    tmi.StructuralSimilarityIndexMeasure = tmi.PeakSignalNoiseRatio = None
    tm.image = tmi
    sys.modules.setdefault("torchmetrics", tm)
    sys.modules.setdefault("torchmetrics.image", tmi)
    spec = importlib.util.spec_from_file_location("ref_metrics", os.path.join(root, "pipeline", "metrics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Recorder:
    """wraps the module's _hit_miss_fa_cn and keeps what it returned"""

    def __init__(self, ref):
        self.ref, self.orig, self.calls = ref, ref._hit_miss_fa_cn, []
        ref._hit_miss_fa_cn = self

    def __call__(self, pred, target, threshold):
        r = self.orig(pred, target, threshold)
        self.calls.append([float(v) for v in r])
        return r

    def take(self):
        c, self.calls = self.calls, []
        assert len(c) == 1
        return c[0]


def standalone(ref, rec, pred, target, pools, clamp):
    """counts / crps / csi / hss of the standalone functions (no clamp inside them: clamp here like :92-93)"""
    if clamp:
        pred, target = pred.clamp(0, 1), target.clamp(0, 1)
    single = pred.mean(dim=1) if pred.ndim == 6 else pred
    counts, crps, csi, hss = [], [], [], []
    for pt, s in pools:
        crps.append(ref.crps(pred, target, pt, s))
        cr, ci, hr = [], [], []
        for th in THRESHOLDS:
            ci.append(ref.csi(single, target, th, pt, s))
            c = rec.take()
            hr.append(ref.hss(single, target, th, pt, s))
            assert rec.take() == c
            cr.append(c)
        counts.append(cr)
        csi.append(ci)
        hss.append(hr)
    return (np.array(counts, dtype=np.float64), np.array(crps), np.array(csi), np.array(hss))


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = load_reference(sys.argv[1])
    rec = Recorder(ref)
    nan = float("nan")
    ref.ssim = lambda p, t: nan
    ref.psnr = lambda p, t: nan
    g = torch.Generator().manual_seed(11)
    out = {"thresholds": np.array(THRESHOLDS)}

    def rand(*shape, lo=0.0, hi=1.0):
        return torch.rand(shape, generator=g) * (hi - lo) + lo

    def u8(*shape):
        return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)

    pu, tu = u8(4, 1, 1, 128, 128), u8(4, 1, 1, 128, 128)
    cases = {
        # name: (pred, target, stored pred, stored target, pools, clamp, run calc_metrics)
        "cont": (rand(2, 2, 1, 64, 64), rand(2, 2, 1, 64, 64), None, None, CALC_POOLS, True, True),
        "u8": (pu.float() / 255, tu.float() / 255, pu, tu, CALC_POOLS, True, True),
        "wide": (rand(2, 1, 1, 48, 48, lo=-0.5, hi=1.5), rand(2, 1, 1, 48, 48, lo=-0.5, hi=1.5), None, None,
                 CALC_POOLS, False, True),
        "odd": (rand(2, 1, 1, 72, 88), rand(2, 1, 1, 72, 88), None, None, CALC_POOLS, True, True),
        "max": (rand(2, 1, 1, 72, 88), rand(2, 1, 1, 72, 88), None, None, [("max", 3), ("max", 4), ("max", 16)],
                False, False),
        "ens": (rand(2, 5, 1, 1, 64, 64), rand(2, 1, 1, 64, 64), None, None, CALC_POOLS, True, True),
    }
    keys = None
    for name, (pred, target, sp, st, pools, clamp, calc) in cases.items():
        counts, crps, csi, hss = standalone(ref, rec, pred, target, pools, clamp)
        out[f"{name}_pred"] = (sp if sp is not None else pred).numpy()
        out[f"{name}_target"] = (st if st is not None else target).numpy()
        out[f"{name}_clamp"] = np.array(clamp)
        out[f"{name}_ptype"] = np.array([PTYPE[p] for p, _ in pools], dtype=np.int32)
        out[f"{name}_pscale"] = np.array([s for _, s in pools], dtype=np.int32)
        out[f"{name}_counts"] = counts.astype(np.int64)
        assert np.array_equal(out[f"{name}_counts"], counts)
        out[f"{name}_crps"], out[f"{name}_csi"], out[f"{name}_hss"] = crps, csi, hss
        if calc:
            m = ref.calc_metrics(pred, target)
            rec.calls.clear()
            keys = list(m) if keys is None else keys
            assert list(m) == keys
            out[f"{name}_metrics"] = np.array([m[k] for k in keys], dtype=np.float64)
            if clamp:   # calc_metrics clamps: its pooled counts are the ones recorded above
                for i, (pt, s) in enumerate(pools):
                    for j in range(len(THRESHOLDS)):
                        sfx = "" if s == 1 else f"_{s}"
                        assert m[f"CSI_{j}{sfx}"] == csi[i, j] and m[f"HSS_{j}{sfx}"] == hss[i, j]
        print(name, {k: v.shape for k, v in out.items() if k.startswith(name + "_")})
    # the quantised case must exercise pooled values that equal a threshold exactly
    p = out["u8_pred"].astype(np.float32) / np.float32(255)
    pooled = torch.nn.functional.avg_pool2d(torch.from_numpy(p).reshape(-1, 1, 128, 128), 4, stride=4)
    ties = sum(int((pooled == np.float32(th)).sum()) for th in THRESHOLDS)
    assert ties > 0, ties
    out["u8_ties"] = np.array(ties)
    out["keys"] = np.array(keys)
    assert out["keys"].dtype.kind == "U" and len(keys) == 56
    path = os.path.join(HERE, "g11_skill.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", ties, "exact ties in u8 pooled pred")


if __name__ == "__main__":
    main()
