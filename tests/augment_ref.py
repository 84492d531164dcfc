"""Float64 restatement (numpy only) of the loader's train-time augmentation: h-flip, v-flip, then a nearest-neighbour
rotation about the image centre with zero fill (torchvision.transforms.functional.rotate with its defaults), applied to a
uint8 'NHWT' batch and followed by the loader's `scale * (u8 + 0)` conversion to fp32 'NTHW'.

For output pixel (i, j), theta counter-clockwise, x_o = j + 0.5 - W/2, y_o = i + 0.5 - H/2:
    x_s = cos(theta) x_o - sin(theta) y_o + W/2 - 0.5
    y_s = sin(theta) x_o + cos(theta) y_o + H/2 - 0.5
    (ys, xs) = round-half-to-even(y_s, x_s);  outside the image -> 0;  else flipped[ys, xs]
    flipped[ys, xs] = img[H-1-ys if vflip else ys, W-1-xs if hflip else xs]

An fp32 evaluation of the same coordinates may round to the other neighbour where x_s or y_s lies within TIE_EPS of a
half-integer; `tie_mask` marks those pixels.  Coordinates reach 272 in magnitude at 384x384, one fp32 ulp there is 3e-5,
a few fused operations stay under 1e-4, and 1e-3 is ten times that.
"""
import math

import numpy as np

TIE_EPS = 1e-3
SCALE = np.float32(1 / 255)


def cos_sin(angle_degrees):
    """exact 0 / +-1 at whole multiples of 90 degrees (a quarter turn is then an exact permutation), else fp64"""
    q = angle_degrees / 90.0
    if q == int(q):
        return ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(q) % 4]
    th = math.radians(angle_degrees)
    return math.cos(th), math.sin(th)


def source_coords(H, W, angle_degrees):
    """fp64 (x_s, y_s), each (H, W)"""
    c, s = cos_sin(angle_degrees)
    xo, yo = np.meshgrid(np.arange(W) + 0.5 - W / 2, np.arange(H) + 0.5 - H / 2)
    return c * xo - s * yo + W / 2 - 0.5, s * xo + c * yo + H / 2 - 0.5


def tie_mask(H, W, angle_degrees, eps=TIE_EPS):
    xs, ys = source_coords(H, W, angle_degrees)
    fx = np.abs(xs - np.floor(xs) - 0.5)
    fy = np.abs(ys - np.floor(ys) - 0.5)
    return (fx < eps) | (fy < eps)


def augment_one(img_hwt, hflip, vflip, angle_degrees, scale=SCALE):
    """uint8 (H, W, T) -> (fp32 (T, H, W), bool (H, W) tie mask)"""
    H, W, T = img_hwt.shape
    xs, ys = source_coords(H, W, angle_degrees)
    xi, yi = np.rint(xs).astype(np.int64), np.rint(ys).astype(np.int64)     # np.rint: half to even
    ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
    xf = np.where(hflip, W - 1 - xi, xi)
    yf = np.where(vflip, H - 1 - yi, yi)
    out = np.zeros((T, H, W), np.float32)
    picked = img_hwt[yf[ok], xf[ok], :].astype(np.float32)                  # (n_ok, T)
    out[:, ok] = (np.float32(scale) * (picked + np.float32(0))).T
    return out, tie_mask(H, W, angle_degrees)


def augment_batch(u8_nhwt, params, scale=SCALE):
    """uint8 (N, H, W, T), [(hflip, vflip, angle)] -> (fp32 (N, T, H, W), bool (N, H, W))"""
    outs, ties = zip(*[augment_one(u8_nhwt[n], *params[n], scale=scale) for n in range(u8_nhwt.shape[0])])
    return np.stack(outs), np.stack(ties)


def neighbour_values(img_hwt, hflip, vflip, angle_degrees, scale=SCALE):
    """fp32 (5, T, H, W): what a pixel may legitimately hold when its rounding is in doubt — 0, or scale * src of one of
    the four pixels around (y_s, x_s) (0 where that neighbour is outside)"""
    H, W, T = img_hwt.shape
    xs, ys = source_coords(H, W, angle_degrees)
    cands = [np.zeros((T, H, W), np.float32)]
    for yi in (np.floor(ys), np.floor(ys) + 1):
        for xi in (np.floor(xs), np.floor(xs) + 1):
            xi_, yi_ = xi.astype(np.int64), yi.astype(np.int64)
            ok = (xi_ >= 0) & (xi_ < W) & (yi_ >= 0) & (yi_ < H)
            xf = np.where(hflip, W - 1 - xi_, xi_)
            yf = np.where(vflip, H - 1 - yi_, yi_)
            v = np.zeros((T, H, W), np.float32)
            v[:, ok] = (np.float32(scale) * (img_hwt[yf[ok], xf[ok], :].astype(np.float32) + np.float32(0))).T
            cands.append(v)
    return np.stack(cands)
