"""numpy restatement of the panels (include/wfae.h "panels in the SEVIR VIL colours"; reference
pipeline/helpers.py:155-225): quantisation, difference, the two table look-ups and the mosaic, plus the PNG decoder the
tests read the written files with.  Integers throughout: every comparison against it is exact equality."""
import os
import struct
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g23_panel_luts.npz")


def luts():
    """(vil, reds) uint8 (256, 3) as matplotlib evaluates them (tests/golden/make_panel_goldens.py)"""
    g = np.load(GOLDEN)
    return g["vil"], g["reds"]


def quantise(x):
    """u = (uint8)(min(max(x, 0), 1) * 255.0f): one fp32 multiply, truncation toward zero; NaN -> 0"""
    x = np.asarray(x, dtype=np.float32)
    c = np.where(x > 0, np.where(x < 1, x, np.float32(1)), np.float32(0)).astype(np.float32)   # NaN fails x > 0
    return (c * np.float32(255.0)).astype(np.float32).astype(np.int64).astype(np.uint8)


def range_count(x):
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return int(((x >= 0) & (x <= 1)).sum())


def figure_shape(t, h, w, gap):
    return 3 * h + 2 * gap, t * w + (t - 1) * gap


def render(pred, target, nb, gap, vil=None, reds=None):
    """pred, target (B, T, H, W) -> uint8 (nb, Hfig, Wfig, 3): rows target / prediction / |difference|, white gaps"""
    if vil is None:
        vil, reds = luts()
    pred, target = np.asarray(pred, dtype=np.float32)[:nb], np.asarray(target, dtype=np.float32)[:nb]
    _, t, h, w = target.shape
    ut, up = quantise(target), quantise(pred)
    d = np.abs(ut.astype(np.int64) - up.astype(np.int64)).astype(np.uint8)
    hfig, wfig = figure_shape(t, h, w, gap)
    out = np.full((nb, hfig, wfig, 3), 255, dtype=np.uint8)
    for r, img in enumerate((vil[ut], vil[up], reds[d])):            # (nb, T, H, W, 3)
        for k in range(t):
            y0, x0 = r * (h + gap), k * (w + gap)
            out[:, y0:y0 + h, x0:x0 + w] = img[:, k]
    return out


def scanlines(rgb):
    """(n, Hfig, Wfig, 3) -> (n, Hfig, 1 + 3 Wfig): what a PNG IDAT holds before compression, filter byte 0"""
    n, hfig, wfig, _ = rgb.shape
    out = np.zeros((n, hfig, 1 + 3 * wfig), dtype=np.uint8)
    out[:, :, 1:] = rgb.reshape(n, hfig, 3 * wfig)
    return out


def decode_png(path):
    """-> uint8 (H, W, 3) of an 8-bit RGB non-interlaced PNG whose scanlines all carry filter type 0; every chunk's CRC
    is checked"""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n", data[:8]
    pos, chunks = 8, []
    while pos < len(data):
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == (zlib.crc32(tag + body) & 0xFFFFFFFF), tag
        chunks.append((tag, body))
        pos += 12 + n
    assert pos == len(data)
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"] and chunks[2][1] == b""
    w, h, depth, colour, comp, filt, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, interlace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), dtype=np.uint8)
    assert raw.size == h * (1 + 3 * w), (raw.size, h, w)
    raw = raw.reshape(h, 1 + 3 * w)
    assert not raw[:, 0].any(), "filter bytes must be 0"
    return raw[:, 1:].reshape(h, w, 3).copy()


def edge_values():
    """fp32: for every k in 0..255 the value k/255 and its two fp32 neighbours (every table boundary and truncation
    edge), then negatives, values above 1, NaN and +-inf"""
    k = (np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float32)
    lo, hi = np.nextafter(k, np.float32(-np.inf)), np.nextafter(k, np.float32(np.inf))
    special = np.array([-0.0, -1e-30, -0.5, -3.0, 1.0000001, 1.5, 255.0, 1e30, np.nan, -np.nan, np.inf, -np.inf],
                       dtype=np.float32)
    return np.concatenate([k, lo, hi, special]).astype(np.float32)


def edge_tensor(shape, seed, within=None, offset=0):
    """an fp32 tensor of `shape`, uniform in [-0.2, 1.2], with the edge values (rotated by `offset`, as many as fit)
    scattered over its first `within` elements (default: all), e.g. the samples that are drawn"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    within = n if within is None else min(int(within), n)
    ev = np.roll(edge_values(), -offset)
    x = rng.uniform(-0.2, 1.2, size=n).astype(np.float32)
    m = min(within, ev.size)
    x[:m] = ev[:m]
    x[:within] = x[:within][rng.permutation(within)]
    return x.reshape(shape)


def holds_all_edges(x):
    """every edge value occurs in x, bit for bit (NaN by its payload-free test)"""
    have = set(np.asarray(x, dtype=np.float32).view(np.uint32).ravel().tolist())
    ev = edge_values()
    return all(int(b) in have for b in ev[~np.isnan(ev)].view(np.uint32)) and bool(np.isnan(x).any())
