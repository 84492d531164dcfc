"""Plain-torch CPU reference of SSIM and PSNR (csrc/ssim.hip; ops.ssim_fwd / ssim_bwd / psnr), the seeded input families
and the bounds of tests/test_ssim_psnr_gpu.py.  Pinned by tests/test_ssim_ref_cpu.py to oracle.ssim / oracle.psnr, to
tests/golden/g7_metrics.npz and to a non-separable 11 x 11 window sum.

SSIM: 11-tap Gaussian sigma 1.5 normalised in the dtype given (oracle/ae_oracle.py::_gauss_1d), valid window, C1 = 1e-4,
C2 = 9e-4; `ssim_map` is the per-pixel map, `ssim` its mean, `ssim_grad` d(g * ssim)/dy from autograd.  PSNR:
per-sample 10 log10(range^2 / mse), range = max(target) - min(target) of that sample; the metric is the mean.

Bounds (torch's own fp32 against fp64 on the same inputs, times 4, the project's convention):

  SSIM value      |got - s64| / |s64|            <= 4 mean|map32 - map64| / |s64|
                  The scalar spread |s32 - s64| is not usable: the per-pixel errors cancel in the mean, by luck down to
                  1e-9, while a correct fp32 kernel with the other filter order is 6e-8 off.  The mean absolute per-pixel
                  spread bounds the error of the mean (triangle inequality) and does not cancel.  It needs a few pixels to
                  be a stable estimate: every shape has at least MIN_MAP_PIXELS map pixels in total.
  SSIM gradient   max|got - g64| / max|g64|      <= 4 max|g32 - g64| / max|g64|          (no floor)
  PSNR            |got - r64| / |r64|            <= max(4 |r32 - r64| / |r64|, PSNR_FLOOR)

PSNR_FLOOR = 4 x 2^-24.  The kernel accumulates (p - g)^2 and the mean over samples in fp64 and rounds once to fp32, so
against fp64 on the same fp32 tensors it owes two things: the final rounding, at most 2^-24 relative; and the fp32
subtraction p - g, at most 2^-24 relative per difference, so at most 2^-23 relative on a sample's mse, which is 10 log10(1 +
2^-23) = 5.2e-7 dB, 0.43 x 2^-24 of a 20 dB value.  Together under 1.5 x 2^-24 for values of 20 dB and more (2.7 x 2^-24 at
5 dB); 4 x 2^-24 is the next power of two.  The test inputs lie between 12 and 36 dB.  The floor binds where torch's fp32
mean happens to round to the fp64 one.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

WIN, SIGMA = 11, 1.5
C1, C2 = 0.01 ** 2, 0.03 ** 2
MIN_MAP_PIXELS = 8
PSNR_FLOOR = 4.0 * 2.0 ** -24


# ------------------------------------------------------------------ reference ---
def gauss_1d(dtype):
    c = torch.arange(WIN, dtype=dtype) - WIN // 2
    g = torch.exp(-(c ** 2) / (2 * SIGMA ** 2))
    return g / g.sum()


def ssim_map(x, y, horizontal_first=False):
    """(N, C, H, W) x 2 -> (N, C, H - 10, W - 10) in x.dtype.  The filter runs down the columns first like
    pytorch_msssim; `horizontal_first` is the order csrc/ssim.hip uses (the same value, another rounding)."""
    ch = x.shape[1]
    g = gauss_1d(x.dtype)
    wv = g.view(1, 1, -1, 1).repeat(ch, 1, 1, 1)
    wh = g.view(1, 1, 1, -1).repeat(ch, 1, 1, 1)
    first, second = (wh, wv) if horizontal_first else (wv, wh)

    def filt(t):
        return F.conv2d(F.conv2d(t, first, groups=ch), second, groups=ch)

    mu1, mu2 = filt(x), filt(y)
    s11 = filt(x * x) - mu1 * mu1
    s22 = filt(y * y) - mu2 * mu2
    s12 = filt(x * y) - mu1 * mu2
    cs = (2 * s12 + C2) / (s11 + s22 + C2)
    return ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs


def ssim(x, y, horizontal_first=False):
    return ssim_map(x, y, horizontal_first).mean()


def ssim_grad(x, y, g, horizontal_first=False):
    """d(g * ssim(x, y)) / dy by autograd, in x.dtype"""
    y = y.detach().clone().requires_grad_(True)
    (g * ssim(x, y, horizontal_first)).backward()
    return y.grad


def psnr_samples(pred, target):
    """(NB, ...) x 2 -> (NB,) in pred.dtype; +inf, -inf and nan where the expression gives them"""
    p, t = pred.flatten(1), target.flatten(1)
    mse = ((p - t) ** 2).mean(dim=1)
    r = t.max(dim=1).values - t.min(dim=1).values
    return 10.0 * torch.log10(r * r / mse)


def psnr(pred, target):
    return psnr_samples(pred, target).mean()


# --------------------------------------------------------------------- bounds ---
def ssim_value_ref(a, p):
    """fp32 target a and prediction p -> (s64, relative bound)"""
    m64 = ssim_map(a.double(), p.double())
    s64 = float(m64.mean())
    spread = float((ssim_map(a, p).double() - m64).abs().mean())
    return s64, 4.0 * spread / abs(s64)


def ssim_grad_ref(a, p, g):
    """-> (g64, bound relative to max|g64|)"""
    g64 = ssim_grad(a.double(), p.double(), g)
    g32 = ssim_grad(a, p, g)
    return g64, 4.0 * float((g32.double() - g64).abs().max() / g64.abs().max())


def psnr_ref(pred, target):
    """-> (r64, relative bound); r64 may be non-finite, the bound is then meaningless"""
    r64 = float(psnr(pred.double(), target.double()))
    r32 = float(psnr(pred, target))
    if not math.isfinite(r64):
        return r64, 0.0
    return r64, max(4.0 * abs(r32 - r64) / abs(r64), PSNR_FLOOR)


# --------------------------------------------------------------------- inputs ---
FAMILIES = ["noise", "storm", "bright", "anti", "same"]
GRAD_FAMILIES = ["noise", "storm", "bright", "anti"]          # the exact gradient of `same` is zero

# (N, C, H, W): one window per image; 1 x 2 windows; one row of windows, 17 wide (a one-pixel second tile); exactly one
# 16 x 16 tile of the map under 2 x 2 tiles of the backward gather (which tiles H x W, not the map); a 17 x 33 map (a
# one-pixel tile both ways); a 27 x 43 map (2 x 3 tiles) under 3 x 4 backward tiles; a 2 x 54 map
SHAPES = [(8, 1, 11, 11), (4, 2, 11, 12), (2, 1, 11, 27), (1, 2, 26, 26), (2, 3, 27, 43), (1, 1, 37, 53), (3, 1, 12, 64)]


def map_pixels(shape):
    n, c, h, w = shape
    return n * c * (h - WIN + 1) * (w - WIN + 1)


def case_seed(family, shape):
    return 1000 * FAMILIES.index(family) + SHAPES.index(tuple(shape))


def make(family, shape, seed):
    """-> (target a, prediction p), fp32 CPU, from torch.Generator(seed)"""
    gen = torch.Generator().manual_seed(int(seed))
    n, c, h, w = shape

    def uni():
        return torch.rand(shape, generator=gen, dtype=torch.float64)

    def nrm():
        return torch.randn(shape, generator=gen, dtype=torch.float64)

    if family in ("noise", "same"):
        a = uni()
        p = a + (uni() * 0.4 - 0.2) if family == "noise" else a.clone()
    elif family == "storm":
        # one blob per image and channel on the unit square, centre anywhere in [0.25, 0.75]^2
        cy = 0.25 + 0.5 * torch.rand((n, c, 1, 1), generator=gen, dtype=torch.float64)
        cx = 0.25 + 0.5 * torch.rand((n, c, 1, 1), generator=gen, dtype=torch.float64)
        v = ((torch.arange(h, dtype=torch.float64) + 0.5) / h).view(1, 1, h, 1)
        u = ((torch.arange(w, dtype=torch.float64) + 0.5) / w).view(1, 1, 1, w)
        r2 = (v - cy) ** 2 + (u - cx) ** 2
        a = 1.6 * torch.exp(-r2 / 0.08) - 0.1
        p = a + 0.05 * nrm()
    elif family == "bright":
        a = 0.97 + 0.002 * nrm()
        p = a + 0.002 * nrm()
    elif family == "anti":
        a = uni()
        p = 1.0 - a + 0.05 * nrm()
    else:
        raise ValueError(family)
    return a.float(), p.float()


# (NB, HW): under one wavefront; under one block; exactly one chunk; a second chunk of one element; more samples than the
# finalize kernel has threads (256), with and without a remainder of 1; the 64-chunk cap with 17 strides per thread, the last
# one of 4099 elements
PSNR_CASES = [(3, 7), (2, 255), (2, 4096), (2, 4097), (300, 50), (257, 16), (2, 64 * 4096 + 4099)]


def psnr_inputs(nb, hw, seed):
    """-> (pred, target) (nb, 1, hw) fp32.  Sample i has its own target interval [lo_i, lo_i + range_i] (range 0.3 .. 0.9,
    every third sample starting at -0.1, so that clamping changes range and error) and a noise whose RMS is set so that the
    samples' unclamped values step from 15 to 35 dB in nb equal steps, in an order that follows neither i nor range_i."""
    gen = torch.Generator().manual_seed(int(seed))
    i = torch.arange(nb, dtype=torch.float64)
    rng = 0.3 + 0.6 * ((i * 7) % nb) / nb
    lo = torch.where(i % 3 == 1, torch.full_like(i, -0.1), 0.02 + 0.2 * ((i * 3) % nb) / nb)
    db = 15.0 + 20.0 * ((i * 11) % nb) / nb
    sigma = rng / 10.0 ** (db / 20.0)
    u = torch.rand((nb, hw), generator=gen, dtype=torch.float64)
    u = (u - u.min(dim=1, keepdim=True).values) / (u.max(dim=1, keepdim=True).values - u.min(dim=1, keepdim=True).values)
    target = lo[:, None] + rng[:, None] * u
    e = torch.randn((nb, hw), generator=gen, dtype=torch.float64)
    e = e * (sigma[:, None] / e.pow(2).mean(dim=1, keepdim=True).sqrt())
    return (target + e).float().view(nb, 1, hw), target.float().view(nb, 1, hw)


def psnr_extreme_inputs(hw, pos_lo, pos_hi, seed):
    """-> (pred, target) (2, 1, hw): targets uniform in [0.3, 0.6] except one 0.05 and one 0.95, at pos_lo / pos_hi in sample 0
    and the other way round in sample 1; prediction = target + 0.02 randn"""
    gen = torch.Generator().manual_seed(int(seed))
    target = 0.3 + 0.3 * torch.rand((2, hw), generator=gen, dtype=torch.float64)
    target[0, pos_lo], target[0, pos_hi] = 0.05, 0.95
    target[1, pos_hi], target[1, pos_lo] = 0.05, 0.95
    pred = target + 0.02 * torch.randn((2, hw), generator=gen, dtype=torch.float64)
    return pred.float().view(2, 1, hw), target.float().view(2, 1, hw)


_BIG = 64 * 4096 + 4099
_STRIDE = 64 * 256                       # elements per grid stride once the chunk count is capped at 64
# (HW, pos_lo, pos_hi): first and last element; the last thread of block 0 and the first of block 1 (255 / 256); the two sides
# of 4096 (one chunk's worth of elements); the first and the last element of the last (17th, partial) grid stride, and the last
# element of the last full one
PSNR_EXTREMES = [(7, 0, 6), (255, 0, 254), (4097, 0, 4096), (4097, 255, 256), (8197, 4095, 4096),
                 (_BIG, 0, _BIG - 1), (_BIG, 16 * _STRIDE, _BIG - 1), (_BIG, 4095, 16 * _STRIDE - 1)]


def psnr_nonfinite_cases():
    """name -> (pred, target, clamp01, class): what the reference expression gives on empty and on perfectly predicted
    frames.  (3, 1, 40) fp32; `class` is 'inf', '-inf' or 'nan', the value of the MEAN over the samples."""
    gen = torch.Generator().manual_seed(77)
    t = 0.2 + 0.5 * torch.rand((3, 1, 40), generator=gen)
    e = 0.03 * torch.randn((3, 1, 40), generator=gen)
    zero, flat = torch.zeros_like(t), torch.full_like(t, 0.25)
    one_empty = t.clone()
    one_empty[1] = 0.0
    one_exact = t + e
    one_exact[2] = t[2]
    one_nan = t.clone()
    one_nan[0] = 0.25
    p_nan = t + e
    p_nan[0] = 0.25
    both = t.clone()                      # sample 0 predicted exactly (+inf), sample 1 empty with an error (-inf)
    both[1] = 0.0
    p_both = both + e
    p_both[0] = both[0]
    below = torch.full_like(t, -0.05)     # empty only after the clamp
    return {
        "pred_equals_target": (t.clone(), t, False, "inf"),
        "constant_target": (flat + e, flat, False, "-inf"),
        "zero_target": (e.abs() + 0.01, zero, False, "-inf"),
        "both_constant_equal": (flat.clone(), flat, False, "nan"),
        "both_zero": (zero.clone(), zero, False, "nan"),
        "one_exact_among_finite": (one_exact, t, False, "inf"),
        "one_empty_among_finite": (one_empty + e, one_empty, False, "-inf"),
        "one_nan_among_finite": (p_nan, one_nan, False, "nan"),
        "inf_and_minus_inf": (p_both, both, False, "nan"),
        "empty_after_clamp": (below + e.abs() + 0.1, below, True, "-inf"),
        "both_empty_after_clamp": (below - e.abs(), below, True, "nan"),
    }


def value_class(v):
    v = float(v)
    return "nan" if math.isnan(v) else ("inf" if v == math.inf else ("-inf" if v == -math.inf else "finite"))
