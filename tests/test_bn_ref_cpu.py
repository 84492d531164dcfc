"""tests/bn_ref.py on the CPU: the float64 restatement of the BatchNorm chain against torch's float64 autograd, the numpy
emulation of the kernels' sums-of-four arithmetic inside the derived mean / variance bounds on every channel class and
shape of tests/test_bn_chain_gpu.py (the condition that the reference alone meets the bounds), and the conditioning table of
DESIGN.md ("BatchNorm chain against float64") regenerated and asserted for its ordering."""
import pytest
import torch
import torch.nn.functional as F

from tests import bn_ref as R

GENERIC_SHAPES, BF16_SHAPES = R.GENERIC_SHAPES, R.BF16_SHAPES       # the shapes of tests/test_bn_chain_gpu.py
TOL64 = 1e-12


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("act", [1, 2])
@pytest.mark.parametrize("classes", [("benign",), ("offset10",), ("benign", "offset10")])
def test_restatement_matches_torch_float64_autograd(classes, act, training):
    """F.batch_norm -> GELU / LeakyReLU(0.2) -> a random cotangent, in float64: forward, saved and running statistics, dx,
    dgamma and dbeta of bn_ref agree with torch to 1e-12, in training and eval mode"""
    shape = (3, 6, 5, 7)
    x32, _ = R.mixed(shape, 11, classes)
    x = x32.double().requires_grad_(True)
    g = torch.Generator().manual_seed(3)
    gamma = (torch.rand(6, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = torch.randn(6, generator=g, dtype=torch.float64).requires_grad_(True)
    rm0, rv0 = torch.randn(6, generator=g, dtype=torch.float64), torch.rand(6, generator=g, dtype=torch.float64) + 0.5
    dy = R.grad(shape, "uniform", 5).double()
    rm, rv = rm0.clone(), rv0.clone()
    u = F.batch_norm(x, rm, rv, gamma, beta, training, 0.1, 1e-5)
    y = F.gelu(u) if act == 1 else F.leaky_relu(u, 0.2)
    y.backward(dy)
    if training:
        s = R.stats64(x32, gamma, beta, 1e-5, rm0, rv0, 0.1)
        mean, invstd, scale, shift = s.mean, s.invstd, s.scale, s.shift
        assert rel(s.running_mean, rm) < TOL64 and rel(s.running_var, rv) < TOL64
        # torch's own saved statistics
        _, sm, si = torch.native_batch_norm(x.detach(), gamma.detach(), beta.detach(), rm0.clone(), rv0.clone(), True, 0.1, 1e-5)
        assert rel(mean, sm) < TOL64 and rel(invstd, si) < TOL64
    else:
        mean, invstd, scale, shift = R.fold_eval64(gamma, beta, rm0, rv0)
        assert torch.equal(rm, rm0) and torch.equal(rv, rv0)
    assert rel(R.apply64(x32, scale, shift, act), y.detach()) < TOL64
    s1, s2 = R.bwd_sums64(dy, x32, scale, shift, mean, invstd, act)
    assert rel(s1, beta.grad) < TOL64 and rel(s2, gamma.grad) < TOL64
    dx = R.bwd_dx64(dy, x32, gamma, scale, shift, mean, invstd, act, training)
    assert rel(dx, x.grad) < TOL64
    res = R.grad(shape, "uniform", 6)
    dx_r = R.bwd_dx64(dy, x32, gamma, scale, shift, mean, invstd, act, training, coef=(s1, s2), res=res)
    assert rel(dx_r, x.grad + res.double()) < TOL64


def test_gradient_classes_are_what_they_claim():
    shape = (3, 5, 7, 9)
    c = R.grad(shape, "cancelling", 1).double()
    assert float(c.sum(dim=(0, 2, 3)).abs().max()) == 0.0 and float(c.abs().max()) > 0.5
    assert float(c.flip(0, 2, 3).sum(dim=(0, 2, 3)).abs().max()) == 0.0          # in another order too
    l1 = R.grad(shape, "l1like", 2)
    assert set(l1.abs().unique().tolist()) == {float(torch.tensor(1.0 / l1.numel(), dtype=torch.float32))}
    x, names = R.mixed((2, 16, 4, 4), 3)
    assert names[:9] == list(R.X_CLASSES) and float(x[:, 3].abs().max()) == 0.0
    assert float((x[:, 5] == 0).float().mean()) > 0.7 and float(x[:, 6].max()) == 1e3
    # a constant cotangent on a channel: the float64 dx of training mode is exactly 0 on a const channel, and 0 to
    # float64 rounding elsewhere
    s = R.stats64(x)
    dy = torch.full((2, 16, 4, 4), 0.25)
    dx = R.bwd_dx64(dy, x, torch.ones(16), s.scale, s.shift, s.mean, s.invstd, 0, True)
    assert float(dx[:, 4].abs().max()) == 0.0 and float(dx[:, 0].abs().max()) < 1e-14


def test_offset_rows_place_output_channels():
    """bn_ref.offset_rows: a 1x1 and a padded 4x4 stride-2 convolution of x = m + s N(0, 1) put the chosen output channels
    at |mean| / sigma near 10 and near 100"""
    g = torch.Generator().manual_seed(1)
    x = (2.5 + 0.1 * torch.randn(2, 32, 16, 16, generator=g)).double()
    w = R.offset_rows(torch.rand(8, 32, 1, 1, generator=g) - 0.5, {0: 10.0, 1: 100.0}, 25.0).double()
    s = R.stats64(F.conv2d(x, w))
    r = (s.mean.abs() * s.invstd).tolist()
    assert 5 < r[0] < 20 and 50 < r[1] < 200, r
    inner = torch.zeros(4, 4, dtype=torch.bool)
    inner[1:3, 1:3] = True
    w4 = R.offset_rows(torch.rand(8, 32, 4, 4, generator=g) - 0.5, {0: 10.0, 1: 100.0}, 25.0, inner).double()
    s = R.stats64(F.conv2d(x, w4, stride=2, padding=1))
    r = (s.mean.abs() * s.invstd).tolist()
    assert 5 < r[0] < 20 and 50 < r[1] < 200, r
    # transposed: a pixel sees 4 of the 16 taps, one of them interior -> half the planned ratio; m / s = 100
    lo = (2.5 + 0.025 * torch.randn(2, 16, 8, 12, generator=g)).double()
    wu = R.offset_rows(torch.rand(8, 16, 4, 4, generator=g) - 0.5, {0: 20.0, 1: 200.0}, 100.0, inner).double()
    s = R.stats64(F.conv_transpose2d(lo, wu.transpose(0, 1), stride=2, padding=1))
    r = (s.mean.abs() * s.invstd).tolist()
    assert 5 < r[0] < 20 and 50 < r[1] < 200, r


@pytest.mark.parametrize("shape", sorted(set(GENERIC_SHAPES + BF16_SHAPES)))
@pytest.mark.parametrize("bf16", [False, True])
def test_emulated_sums_of_four_stay_inside_the_derived_bounds(shape, bf16):
    """the arithmetic of chan_reduce_kernel and bn_finalize_kernel, emulated in numpy, against float64 on every channel
    class: mean and variance inside bn_ref's bounds.  No class may use more than half of a bound (measured: 0.319 of the
    variance bound, (5, 64, 16, 8) as bf16 values, and 0.239 of the mean bound, (2, 16, 10, 12), both on the channel with one
    value of 1e3; the test prints them) — above that the rounding count would be wrong"""
    x, names = R.mixed(shape, 7, R.classes_for(shape[1]))
    if bf16:
        x = x.bfloat16().float()
    s = R.stats64(x)
    width = 8 if bf16 else 4        # values per 16-byte access: the vector path needs HW % width == 0
    mean, var, _ = R.emulate_stats(x, width=width)
    k_sum, k_sq = R.sum_counts(x, (shape[2] * shape[3]) % width == 0)
    exact = dict(zip(names, R.fp32_exact_channels(x).tolist()))
    assert exact["grid"] and exact.get("const0", True) and not exact["spike" if "spike" in exact else "benign"], exact
    assert bf16 or not (exact.get("const", False) or exact["offset100"]), exact      # (bf16 values near 100 lie on a grid of 1/2)
    use_m = (mean - s.mean).abs() / R.mean_bound(s, k_sum).clamp_min(1e-300)
    use_v = (var - s.var).abs() / R.var_bound(s, k_sum, k_sq).clamp_min(1e-300)
    print(shape, bf16, "largest use of the mean bound %.3f (%s), of the variance bound %.3f (%s)" % (
        float(use_m.max()), names[int(use_m.argmax())], float(use_v.max()), names[int(use_v.argmax())]))
    assert float(use_m.max()) <= 0.5, (float(use_m.max()), names[int(use_m.argmax())])
    assert float(use_v.max()) <= 0.5, (float(use_v.max()), names[int(use_v.argmax())])


def conditioning_table():
    """per channel class: relative error of invstd and max error of y = xhat (gamma 1, beta 0) of the emulated kernel
    arithmetic and of torch's fp32 CPU batch norm, against float64, worst of 8 channels of 960 and of 36864 values"""
    rows = {}
    for cls in ("benign", "offset10", "offset100", "sparse"):
        e_inv, t_inv, e_y, t_y = 0.0, 0.0, 0.0, 0.0
        for shape in ((15, 8, 8, 8), (4, 8, 96, 96)):
            x, _ = R.mixed(shape, 21, (cls,))
            s = R.stats64(x)
            mean, _, invstd = R.emulate_stats(x)
            invstd = invstd.float().double()                            # save_invstd is an fp32 value, like torch's
            e_inv = max(e_inv, float(((invstd - s.invstd).abs() / s.invstd).max()))
            sc = invstd.float()                                         # the kernel's fp32 scale / shift and its fma
            sh = (-(mean.float() * sc)).float()
            y_e = torch.addcmul(sh.view(1, -1, 1, 1), x, sc.view(1, -1, 1, 1))
            y_t, m_t, i_t = torch.native_batch_norm(x, None, None, None, None, True, 0.1, 1e-5)
            y64 = R.apply64(x, s.scale, s.shift, 0)
            t_inv = max(t_inv, float(((i_t.double() - s.invstd).abs() / s.invstd).max()))
            e_y = max(e_y, float((y_e.double() - y64).abs().max()))
            t_y = max(t_y, float((y_t.double() - y64).abs().max()))
        rows[cls] = (e_inv, t_inv, e_y, t_y)
    return rows


def test_conditioning_table_keeps_its_ordering():
    """DESIGN.md's claim, kept true to the code: on the model's own kind of activations (mean / sigma of order 1, zero-heavy
    frames) S2 / n - mean^2 on fp64 accumulators is no worse than 4 x torch's fp32 CPU BatchNorm; at a mean of 100 sigma it is
    worse than 4 x torch — in save_invstd (rounded to fp32 on both sides) and in y.  Only the ordering is asserted; the figures
    are printed"""
    rows = conditioning_table()
    for cls, (e_inv, t_inv, e_y, t_y) in rows.items():
        print("%-10s invstd: emulation %.1e torch fp32 %.1e   y: emulation %.1e torch fp32 %.1e" % (cls, e_inv, t_inv, e_y, t_y))
    for cls in ("benign", "sparse"):
        assert rows[cls][0] <= 4 * rows[cls][1] and rows[cls][2] <= 4 * rows[cls][3], (cls, rows[cls])
    assert rows["offset100"][0] > 4 * rows["offset100"][1] and rows["offset100"][2] > 4 * rows["offset100"][3], rows["offset100"]
