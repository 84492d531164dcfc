"""CPU: tests/ssim_ref.py (the fp64 reference, the input families and the bounds of tests/test_ssim_psnr_gpu.py) against
oracle.ssim / oracle.psnr, tests/golden/g7_metrics.npz and a non-separable 11 x 11 window sum; the families do what they
claim; a correct fp32 SSIM with the kernel's filter order stays under both SSIM bounds on every case of the GPU test, and
a map that loses its last column does not; the PSNR inputs keep their samples apart."""
import math

import pytest
import torch

from oracle import ae_oracle as orc
from tests import ssim_ref as R
from tests._util import golden

G = -0.7                                  # the upstream gradient the GPU test uses
SSIM_CASES = [(f, s) for f in R.FAMILIES for s in R.SHAPES]
IDS = [f"{f}-{'x'.join(map(str, s))}" for f, s in SSIM_CASES]


@pytest.fixture(scope="module")
def g7():
    return golden("g7_metrics")


def _g7_pair(g7, i):
    return torch.from_numpy(g7[f"{i}/pred"]), torch.from_numpy(g7[f"{i}/target"])


@pytest.mark.parametrize("i", range(4))
def test_reference_matches_oracle_and_g7(g7, i):
    p, t = _g7_pair(g7, i)
    s = float(R.ssim(t.double(), p.double()))
    assert abs(s - float(orc.ssim(t.double(), p.double()))) <= 1e-7
    assert abs(s - float(g7[f"{i}/ssim"])) <= 1e-7 and abs(s - float(g7[f"{i}/ssim_form2"])) <= 1e-7
    r = float(R.psnr(p.double(), t.double()))
    assert abs(r - orc.psnr(p.double(), t.double())) <= 1e-9 * r
    assert abs(r - float(g7[f"{i}/psnr"])) <= 1e-9 * r and abs(r - float(g7[f"{i}/psnr_form2"])) <= 1e-7 * r


@pytest.mark.parametrize("i", range(4))
def test_gradient_matches_g7(g7, i):
    """G7 holds torch's fp32 autograd gradient of 1 - ssim: the fp64 one differs by fp32 rounding (measured 6e-7 .. 1.3e-6
    of the largest element; 2^-24 = 6e-8 per rounding over the 2 x 121-term window sums and the quotient)"""
    p, t = _g7_pair(g7, i)
    g64 = R.ssim_grad(t.double(), p.double(), -1.0)
    want = torch.from_numpy(g7[f"{i}/ssim_loss_grad"]).double()
    err = float((g64 - want).abs().max() / want.abs().max())
    print(f"g7/{i}: fp64 autograd against the recorded fp32 gradient {err:.2e}")
    assert err <= 4e-6


def _window_sum_map(x, y):
    """the SSIM map from direct 11 x 11 window sums (outer product of the taps, no separable pass), fp64"""
    g = R.gauss_1d(torch.float64)
    w2 = torch.outer(g, g)

    def win(t):
        return (t.unfold(2, R.WIN, 1).unfold(3, R.WIN, 1) * w2).sum(dim=(-1, -2))

    mx, my = win(x), win(y)
    sxx, syy, sxy = win(x * x) - mx * mx, win(y * y) - my * my, win(x * y) - mx * my
    return (2 * mx * my + R.C1) * (2 * sxy + R.C2) / ((mx * mx + my * my + R.C1) * (sxx + syy + R.C2))


@pytest.mark.parametrize("family,shape", [("noise", (4, 2, 11, 12)), ("storm", (2, 3, 27, 43)), ("anti", (3, 1, 12, 64)),
                                          ("bright", (1, 1, 37, 53))])
def test_reference_matches_window_sum(family, shape):
    a, p = R.make(family, shape, R.case_seed(family, shape))
    a, p = a.double(), p.double()
    m = R.ssim_map(a, p)
    assert m.shape == (shape[0], shape[1], shape[2] - 10, shape[3] - 10)
    # `bright` divides by variances of 4e-6 that come from a difference of numbers near 0.94: 1e-16 / 4e-6 per pixel
    tol = 1e-9 if family == "bright" else 1e-12
    assert float((m - _window_sum_map(a, p)).abs().max()) <= tol
    assert float((m - R.ssim_map(a, p, horizontal_first=True)).abs().max()) <= tol


def test_every_shape_has_enough_map_pixels():
    for s in R.SHAPES:
        assert R.map_pixels(s) >= R.MIN_MAP_PIXELS, s
    assert R.map_pixels(R.SHAPES[0]) == 8 and (R.SHAPES[3][2] - 10, R.SHAPES[4][3] - 10) == (16, 33)


def test_families_do_what_they_claim():
    def windows(t):
        return t.unfold(2, R.WIN, 1).unfold(3, R.WIN, 1).flatten(-2)

    # storm: plateaus of exact 0 and exact 1 after the clamp, with windows wholly inside each and windows across the edge
    shape = (1, 1, 37, 53)
    a, p = R.make("storm", shape, R.case_seed("storm", shape))
    assert float(a.min()) < 0 and float(a.max()) > 1 and float(p.min()) < 0 and float(p.max()) > 1
    w = windows(a.clamp(0, 1))
    lo, hi = w.min(-1).values, w.max(-1).values
    assert bool((hi == 0).any()) and bool((lo == 1).any()) and bool(((lo == 0) & (hi == 1)).any())
    wp = windows(p.clamp(0, 1))
    assert bool(((wp == 0).float().mean(-1) > 0.9).any()) and bool(((wp == 1).float().mean(-1) > 0.9).any())
    for s in R.SHAPES:
        a, p = R.make("storm", s, R.case_seed("storm", s))
        assert bool((a.clamp(0, 1) == 0).any()) and float(a.max()) > 0.5, s
    for s in R.SHAPES:
        a, p = R.make("anti", s, R.case_seed("anti", s))
        assert float(R.ssim(a.double(), p.double())) < -0.9, s
        a, p = R.make("noise", s, R.case_seed("noise", s))
        assert float(p.min()) < 0 and float(p.max()) > 1, s
        noise_spread = float((R.ssim_map(a, p).double() - R.ssim_map(a.double(), p.double())).abs().mean())
        # bright: E[x^2] - mu^2 = 0.94 - 0.94 leaves 2^-24 x 0.94 of absolute error on a variance of 4e-6
        a, p = R.make("bright", s, R.case_seed("bright", s))
        spread = float((R.ssim_map(a, p).double() - R.ssim_map(a.double(), p.double())).abs().mean())
        print(f"{s}: mean per-pixel fp32 spread bright {spread:.2e} noise {noise_spread:.2e}")
        assert spread > 1e-5 and noise_spread < 1e-6, s
        a, p = R.make("same", s, R.case_seed("same", s))
        assert torch.equal(a, p)


@pytest.mark.parametrize("family,shape", SSIM_CASES, ids=IDS)
def test_correct_fp32_variant_is_under_the_bounds(family, shape):
    """the reference's own formula in fp32 with the filter order swapped (rows first, as csrc/ssim.hip does) is a correct
    fp32 SSIM: it must pass both bounds, so that they are passable before anyone runs a GPU"""
    a, p = R.make(family, shape, R.case_seed(family, shape))
    for clamp in (False, True):
        ac, pc = (a.clamp(0, 1), p.clamp(0, 1)) if clamp else (a, p)
        s64, bound = R.ssim_value_ref(ac, pc)
        err = abs(float(R.ssim(ac, pc, horizontal_first=True)) - s64) / abs(s64)
        print(f"value clamp={int(clamp)}: s64 {s64:+.6f} err {err:.3e} bound {bound:.3e} ratio {err / bound if bound else 0:.3f}")
        assert err <= bound
        if family == "same":
            assert s64 == 1.0
    if family in R.GRAD_FAMILIES:
        g64, bound = R.ssim_grad_ref(a, p, G)
        got = R.ssim_grad(a, p, G, horizontal_first=True)
        err = float((got.double() - g64).abs().max() / g64.abs().max())
        print(f"gradient: err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
        assert err <= bound


@pytest.mark.parametrize("family,shape", [(f, s) for f in ("noise", "storm", "anti") for s in R.SHAPES if s[3] > 11],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_value_bound_rejects_a_map_without_its_last_column(family, shape):
    """the bounds bite: a mean over a map that misses its last column (`ox < Wo - 1`) is 18 to 4055 times over the bound on
    these cases; a gradient written one column off 1e4 to 5e5 times"""
    a, p = R.make(family, shape, R.case_seed(family, shape))
    for clamp in (False, True):
        ac, pc = (a.clamp(0, 1), p.clamp(0, 1)) if clamp else (a, p)
        s64, bound = R.ssim_value_ref(ac, pc)
        short = float(R.ssim_map(ac.double(), pc.double())[..., :-1].mean())
        over = abs(short - s64) / abs(s64) / bound
        print(f"clamp={int(clamp)}: without the last column {over:.0f} x the bound")
        assert over > 10
    g64, bound = R.ssim_grad_ref(a, p, G)
    over = float((g64.roll(1, -1) - g64).abs().max() / g64.abs().max()) / bound
    print(f"gradient one column off: {over:.0f} x the bound")
    assert over > 10


@pytest.mark.parametrize("nb,hw", R.PSNR_CASES)
def test_psnr_inputs_keep_their_samples_apart(nb, hw):
    """replacing one sample's value by any other sample's moves the mean by more than the bound; the clamp moves the mean by
    far more than the bound; the values lie where PSNR_FLOOR was derived"""
    pred, target = R.psnr_inputs(nb, hw, seed=nb * 31 + hw)
    v = R.psnr_samples(pred.double(), target.double())
    r64, bound = R.psnr_ref(pred, target)
    assert abs(r64 - float(v.mean())) <= 1e-12 * r64
    gap = float(v.sort().values.diff().min())
    print(f"({nb}, {hw}): mean {r64:.4f} dB, smallest gap {gap:.3e} dB, bound {bound * r64:.3e} dB")
    assert gap / nb > 4 * bound * r64
    vc = R.psnr_samples(pred.clamp(0, 1).double(), target.clamp(0, 1).double())
    c64, cbound = R.psnr_ref(pred.clamp(0, 1), target.clamp(0, 1))
    assert abs(c64 - r64) > 1000 * max(bound * r64, cbound * c64)
    for x in (v, vc):
        assert bool(torch.isfinite(x).all()) and 12.0 < float(x.min()) and float(x.max()) < 36.0


@pytest.mark.parametrize("hw,pos_lo,pos_hi", R.PSNR_EXTREMES)
def test_psnr_extremes_decide_the_range(hw, pos_lo, pos_hi):
    pred, target = R.psnr_extreme_inputs(hw, pos_lo, pos_hi, seed=hw + pos_lo)
    assert float(target[0, 0, pos_lo]) == pytest.approx(0.05) and float(target[1, 0, pos_lo]) == pytest.approx(0.95)
    r64, bound = R.psnr_ref(pred, target)
    for pos in (pos_lo, pos_hi):
        blind = target.clone()
        blind[:, 0, pos] = 0.45                                     # a kernel that never sees this element
        mse = ((pred.double() - target.double()) ** 2).flatten(1).mean(1)
        rng = (blind.flatten(1).max(1).values - blind.flatten(1).min(1).values).double()
        missed = float((10 * torch.log10(rng * rng / mse)).mean())
        assert abs(missed - r64) / r64 > 1000 * bound


def test_psnr_nonfinite_classes():
    """the reference expression on empty frames and exact predictions, in fp64 and in fp32, gives the class each case names"""
    for name, (pred, target, clamp, cls) in R.psnr_nonfinite_cases().items():
        pc, tc = (pred.clamp(0, 1), target.clamp(0, 1)) if clamp else (pred, target)
        assert R.value_class(R.psnr(pc.double(), tc.double())) == cls, name
        assert R.value_class(R.psnr(pc, tc)) == cls, name
        assert R.value_class(orc.psnr(pc.double(), tc.double())) == cls, name
    assert math.isinf(R.psnr_ref(*R.psnr_nonfinite_cases()["pred_equals_target"][:2])[0])
