"""GPU: csrc/ssim.hip (ops.ssim_fwd, ops.ssim_bwd, ops.psnr, Fn.ssim, calc_metrics' SSIM / PSNR) against the fp64 reference
tests/ssim_ref.py, which tests/test_ssim_ref_cpu.py pins to the oracle, to G7 and to a direct window sum.

SSIM on five input families (in-range noise that its prediction leaves, VIL-like blobs with flat plateaus below 0 and above
1, bright nearly constant frames, anti-correlated pairs, identical pairs) x seven plane shapes (H != W, one window, one row
of windows, exactly one 16 x 16 map tile, one-pixel second tiles, several channels): value with and without the clamp,
gradient with upstream -0.7 and through autograd, clamp01=True against pre-clamped input bit for bit, two launches bit for
bit.  PSNR at the launch geometries of psnr_part_kernel / psnr_finalize_kernel (under a wavefront, a second chunk of one
element, more samples than finalize threads, the 64-chunk cap), with the target's extremes planted at the positions a
strided loop can miss, and on empty / exactly predicted frames, where the reference gives -inf, +inf or nan.  Argument checks.

Bounds (derived in tests/ssim_ref.py, always from the reference): value 4 x mean |map32 - map64| / |s64|; gradient per element
4 x max |g32 - g64| / max |g64|; PSNR max(4 x |r32 - r64| / |r64|, 4 x 2^-24).  Every test prints err, bound and ratio.

Measured on the MI355X, worst err / bound per group ("SSIM and PSNR against fp64"):
  ssim_fwd          noise 0.21, storm 0.17, bright 0.05, anti 0.27, same 0 (the kernel returns exactly 1, as torch's fp32 does)
  ssim_bwd          noise 0.31, storm 0.41, bright 0.42, anti 0.36; through Fn.ssim 0.42
  psnr              launch geometries 0.16, planted extremes 0.24 (the floor 4 x 2^-24 binds in 26 of 30)
  calc_metrics      SSIM 0.21, PSNR 0.20
The clamp and repeat properties hold bit for bit and the eleven non-finite PSNR cases return the reference's class.
Mutants of csrc/ssim.hip built on a scratch copy, each run once: the backward gather tiled by Wo instead of W fails the
gradient, autograd and repeat tests at 26 x 26 and 37 x 53 (the two shapes where cdiv(W - 10, 16) != cdiv(W, 16)) and passes
every older test; `valid` tested with <= fails 103 cases here (none at 26 x 26, whose map is exactly one tile) and two
older ones (test_ssim_psnr_golden, test_ssim_finalize_bits); the finalize loop without its stride fails only test_psnr_launch_geometry[300-50] and [257-16].
"""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest
import torch

from tests import skill_ref
from tests import ssim_ref as R
from weatherforecastingtoolkit_amd import _lib, functional as Fn, ops
from weatherforecastingtoolkit_amd.pipeline import metrics as M

pytestmark = pytest.mark.gpu

G = float(torch.tensor(-0.7, dtype=torch.float32))          # the upstream gradient as the kernel reads it
W = float(torch.tensor(0.4, dtype=torch.float32))           # the weight of the SSIM term in the autograd test
SSIM_CASES = [(f, s) for f in R.FAMILIES for s in R.SHAPES]
GRAD_CASES = [(f, s) for f in R.GRAD_FAMILIES for s in R.SHAPES]
_id = lambda c: f"{c[0]}-{'x'.join(map(str, c[1]))}"
G11 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g11_skill.npz")


@functools.lru_cache(maxsize=None)
def _inputs(family, shape):
    return R.make(family, shape, R.case_seed(family, shape))


@functools.lru_cache(maxsize=None)
def _value_ref(family, shape, clamp):
    a, p = _inputs(family, shape)
    return R.ssim_value_ref(a.clamp(0, 1), p.clamp(0, 1)) if clamp else R.ssim_value_ref(a, p)


@functools.lru_cache(maxsize=None)
def _grad_ref(family, shape):
    return R.ssim_grad_ref(*_inputs(family, shape), G)


def _report(what, err, bound):
    ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
    print(f"{what}: err {err:.3e} bound {bound:.3e} ratio {ratio:.3f}")
    assert err <= bound, (what, err, bound)


# ----------------------------------------------------------------------- SSIM ---
@pytest.mark.parametrize("family,shape", SSIM_CASES, ids=[_id(c) for c in SSIM_CASES])
def test_ssim_value(dev, family, shape):
    a, p = _inputs(family, shape)
    ad, pd = a.to(dev), p.to(dev)
    for clamp in (False, True):
        s64, bound = _value_ref(family, shape, clamp)
        if family == "same":
            assert s64 == 1.0
        got = float(ops.ssim_fwd(ad, pd, clamp01=clamp).item())
        _report(f"ssim_fwd {family} {shape} clamp={int(clamp)} s64 {s64:+.6f}", abs(got - s64) / abs(s64), bound)


def _grad_err(got, g64):
    return float((got.double().cpu() - g64).abs().max() / g64.abs().max())


@pytest.mark.parametrize("family,shape", GRAD_CASES, ids=[_id(c) for c in GRAD_CASES])
def test_ssim_gradient(dev, family, shape):
    a, p = _inputs(family, shape)
    g64, bound = _grad_ref(family, shape)
    got = ops.ssim_bwd(a.to(dev), p.to(dev), torch.tensor(G, device=dev))
    assert got.shape == p.shape
    _report(f"ssim_bwd {family} {shape}", _grad_err(got, g64), bound)


@pytest.mark.parametrize("family,shape", GRAD_CASES, ids=[_id(c) for c in GRAD_CASES])
def test_ssim_gradient_through_autograd(dev, family, shape):
    """loss = 0.4 * ssim(a, p) + sum(q^2) / 2: p gets 0.4 x the SSIM gradient, q gets q, the target a gets nothing"""
    a, p = _inputs(family, shape)
    g64, bound = _grad_ref(family, shape)
    ad = a.to(dev).requires_grad_(True)
    pd = p.to(dev).requires_grad_(True)
    q = torch.linspace(-1, 1, 7, device=dev).requires_grad_(True)
    loss = W * Fn.ssim(ad, pd) + 0.5 * (q * q).sum()
    loss.backward()
    assert ad.grad is None and torch.equal(q.grad, q.detach())
    _report(f"Fn.ssim backward {family} {shape}", _grad_err(pd.grad, g64 * (W / G)), bound)


@pytest.mark.parametrize("family,shape", SSIM_CASES, ids=[_id(c) for c in SSIM_CASES])
def test_ssim_clamp_flag_is_a_clamp_and_launches_repeat(dev, family, shape):
    """clamp01=True on the raw tensors and clamp01=False on clamp(0, 1) tensors: the same bits (clamping an in-range fp32
    value is the identity); a second launch of forward and backward: the same bits"""
    a, p = _inputs(family, shape)
    ad, pd = a.to(dev), p.to(dev)
    ac, pc = a.clamp(0, 1).to(dev), p.clamp(0, 1).to(dev)
    if family in ("noise", "storm"):
        assert not torch.equal(pc, pd)
    on = ops.ssim_fwd(ad, pd, clamp01=True)
    assert torch.equal(on, ops.ssim_fwd(ac, pc, clamp01=False))
    assert torch.equal(on, ops.ssim_fwd(ac, pc, clamp01=True))
    assert torch.equal(on, ops.ssim_fwd(ad, pd, clamp01=True))
    off = ops.ssim_fwd(ad, pd, clamp01=False)
    assert torch.equal(off, ops.ssim_fwd(ad, pd, clamp01=False))
    g = torch.tensor(G, device=dev)
    assert torch.equal(ops.ssim_bwd(ad, pd, g), ops.ssim_bwd(ad, pd, g))


# ----------------------------------------------------------------------- PSNR ---
def _psnr_check(what, dev, pred, target):
    for clamp in (False, True):
        pc, tc = (pred.clamp(0, 1), target.clamp(0, 1)) if clamp else (pred, target)
        r64, bound = R.psnr_ref(pc, tc)
        got = ops.psnr(pred.to(dev), target.to(dev), clamp01=clamp)
        _report(f"psnr {what} clamp={int(clamp)} r64 {r64:.5f}", abs(float(got.item()) - r64) / abs(r64), bound)
        if clamp:
            assert torch.equal(got, ops.psnr(pc.to(dev), tc.to(dev), clamp01=False))
        assert torch.equal(got, ops.psnr(pred.to(dev), target.to(dev), clamp01=clamp))


@pytest.mark.parametrize("nb,hw", R.PSNR_CASES)
def test_psnr_launch_geometry(dev, nb, hw):
    pred, target = R.psnr_inputs(nb, hw, seed=nb * 31 + hw)
    _psnr_check(f"({nb}, {hw})", dev, pred, target)


@pytest.mark.parametrize("hw,pos_lo,pos_hi", R.PSNR_EXTREMES)
def test_psnr_sees_the_extremes(dev, hw, pos_lo, pos_hi):
    """the target's minimum and maximum sit at pos_lo / pos_hi (and the other way round in the second sample); missing either
    moves the value by more than 1000 x the bound (tests/test_ssim_ref_cpu.py)"""
    pred, target = R.psnr_extreme_inputs(hw, pos_lo, pos_hi, seed=hw + pos_lo)
    _psnr_check(f"extremes ({hw}, {pos_lo}, {pos_hi})", dev, pred, target)


@pytest.mark.parametrize("name", list(R.psnr_nonfinite_cases()))
def test_psnr_nonfinite_classes(dev, name):
    """empty target frames (range 0) and exact predictions (mse 0): the kernel returns what the fp64 expression returns"""
    pred, target, clamp, cls = R.psnr_nonfinite_cases()[name]
    pc, tc = (pred.clamp(0, 1), target.clamp(0, 1)) if clamp else (pred, target)
    want = R.value_class(R.psnr(pc.double(), tc.double()))
    assert want == cls
    got = ops.psnr(pred.to(dev), target.to(dev), clamp01=clamp).item()
    print(f"psnr {name}: kernel {got} reference {cls}")
    assert R.value_class(got) == want


# --------------------------------------------------------------- calc_metrics ---
@pytest.mark.parametrize("case", skill_ref.CALC_CASES)
def test_calc_metrics_ssim_psnr_against_fp64(dev, case):
    """calc_metrics goes through clamp01=True; the reference is fp64 on the clamped tensors (for the 6-D ensemble: on the
    fp32 mean over members of the clamped members, which ops.ensemble_mean reproduces bit for bit, test_skill_gpu.py).
    PSNR here is 4.7 .. 10 dB: the floor's derivation gives 2.9 x 2^-24 at 4.65 dB, still under 4 x 2^-24."""
    pred, target, _, _ = skill_ref.load_case(np.load(G11, allow_pickle=False), case)
    d = M.calc_metrics(pred.to(dev), target.to(dev))
    pc, tc = pred.clamp(0, 1), target.clamp(0, 1)
    single = pc.mean(dim=1) if pc.dim() == 6 else pc
    h, w = single.shape[-2:]
    p, g = single.reshape(-1, 1, h, w), tc.reshape(-1, 1, h, w)
    s64, bound = R.ssim_value_ref(g, p)
    assert R.map_pixels(p.shape) >= R.MIN_MAP_PIXELS
    _report(f"calc_metrics {case} SSIM s64 {s64:+.6f}", abs(d["SSIM"] - s64) / abs(s64), bound)
    r64, bound = R.psnr_ref(p, g)
    _report(f"calc_metrics {case} PSNR r64 {r64:.5f}", abs(d["PSNR"] - r64) / abs(r64), bound)
    assert d["paper_SSIM"] == d["SSIM"] and d["paper_PSNR"] == d["PSNR"]


# ------------------------------------------------------------ argument checks ---
def test_shape_mismatch_raises(dev):
    """nothing is launched: every call is refused on the host"""
    x = torch.zeros((2, 1, 12, 16), device=dev)
    g = torch.ones((), device=dev)
    for other in (torch.zeros((2, 1, 12, 15), device=dev), torch.zeros((1, 1, 12, 16), device=dev),
                  torch.zeros((2, 1, 16, 12), device=dev), torch.zeros((2, 12, 16), device=dev)):
        for call in (lambda: ops.ssim_fwd(x, other), lambda: ops.ssim_fwd(other, x), lambda: ops.ssim_bwd(x, other, g),
                     lambda: ops.ssim_bwd(other, x, g), lambda: ops.psnr(x, other), lambda: ops.psnr(other, x)):
            with pytest.raises(_lib.WfaeError, match="differ"):
                call()
    flat = torch.zeros((24, 16), device=dev)
    for call in (lambda: ops.ssim_fwd(flat, flat), lambda: ops.ssim_bwd(flat, flat, g), lambda: ops.psnr(flat, flat)):
        with pytest.raises(_lib.WfaeError, match="expected"):
            call()


def test_plane_smaller_than_the_window_raises(dev):
    g = torch.ones((), device=dev)
    for shape in ((2, 1, 10, 11), (2, 1, 11, 10)):
        x = torch.zeros(shape, device=dev)
        with pytest.raises(_lib.WfaeError):
            ops.ssim_fwd(x, x)
        with pytest.raises(_lib.WfaeError):
            ops.ssim_bwd(x, x, g)
