"""Generate tests/golden/g25_verify.npz from the reference's own pipeline/metrics.py (CPU, fp32).

    python tests/golden/make_verify_goldens.py <reference checkout root>

One seeded case quantised to k / 255, so that target, persistence and forecast values tie exactly with the six
thresholds: frames (B = 2, T = 5, 1 x 24 x 20) with L = 2 input and P = 3 predicted frames, and a forecast field
(2, 3, 1, 24, 20).  Per lead and for the two fields (forecast, persistence = frames[:, L - 1]) against frames[:, L:] the
fixture records the reference's `csi` / `hss` called on that lead's slice, and torch fp64 `mse` / `mae`.  The reference
module is loaded as make_skill_goldens.py loads it; nothing from it is copied, the fixture holds inputs and recorded
results only.

Keys: `frames_u8` (2, 5, 24, 20), `forecast_u8` (2, 3, 24, 20) (value = u8 / 255 in fp32), `input_frames`, `thresholds`
(fp64), `csi`, `hss` (P, 2, 6), `mse`, `mae` (P, 2) (field 0 forecast, field 1 persistence), `ties`.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_skill_goldens import THRESHOLDS, load_reference  # noqa: E402

B, T, L, H, W = 2, 5, 2, 24, 20


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = load_reference(sys.argv[1])
    g = torch.Generator().manual_seed(25)
    frames_u8 = torch.randint(0, 256, (B, T, H, W), generator=g, dtype=torch.uint8)
    forecast_u8 = torch.randint(0, 256, (B, T - L, H, W), generator=g, dtype=torch.uint8)
    frames = (frames_u8.float() / 255).unsqueeze(2)             # (B, T, 1, H, W)
    forecast = (forecast_u8.float() / 255).unsqueeze(2)         # (B, P, 1, H, W)
    target = frames[:, L:]
    fields = [forecast, frames[:, L - 1:L].expand(B, T - L, 1, H, W)]
    P = T - L
    csi, hss = np.zeros((P, 2, len(THRESHOLDS))), np.zeros((P, 2, len(THRESHOLDS)))
    mse, mae = np.zeros((P, 2)), np.zeros((P, 2))
    for p in range(P):
        t = target[:, p:p + 1].contiguous()
        for i, f in enumerate(fields):
            v = f[:, p:p + 1].contiguous()
            for k, th in enumerate(THRESHOLDS):
                csi[p, i, k] = ref.csi(v, t, th)
                hss[p, i, k] = ref.hss(v, t, th)
            e = v.double() - t.double()
            mse[p, i], mae[p, i] = float((e * e).mean()), float(e.abs().mean())
    ties = sum(int((x == np.float32(th)).sum()) for th in THRESHOLDS for x in (target.numpy(), forecast.numpy(),
                                                                               frames[:, L - 1].numpy()))
    assert ties > 0
    out = {"frames_u8": frames_u8.numpy(), "forecast_u8": forecast_u8.numpy(), "input_frames": np.array(L),
           "thresholds": np.array(THRESHOLDS), "csi": csi, "hss": hss, "mse": mse, "mae": mae, "ties": np.array(ties)}
    path = os.path.join(HERE, "g25_verify.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", ties, "values equal to a threshold")


if __name__ == "__main__":
    main()
