"""Float64 restatement of the optimiser step and the fp32 glue kernels of csrc/norm_act.hip (wfae_adamw / wfae_adamw_c,
wfae_sumsq -> wfae_clip_coef -> wfae_scale, wfae_adaptive_weight, wfae_reduce_sum, sigmoid / GELU), with per-element error
bounds derived from the kernels' operation sequences, and the table of AdamW cases that tests/test_optim_ref_cpu.py and
tests/test_optim_gpu.py and tests/test_glue_kernels_gpu.py share.  numpy (torch only for erf in float64).

Convention: U = 2^-24, the largest relative error of one fp32 operation rounded to nearest (+, -, *, /, sqrt and a
conversion from fp64; the device's fp32 division and square root are correctly rounded).  Bounds are first-order
propagations of one U per operation through the kernel's expression, times SLACK = 1 + 2^-10 for the second-order
terms (each is below 16 U of a first-order one).  A fused multiply-add has one rounding where the bound counts two, so
the bounds hold for either contraction of an expression.  No case here enters the subnormal range.

AdamW (adamw_kernel / adamw_c_kernel), per element, from fp32 state p, g, m, v and the fp32 scalars the kernel receives
(lr, b2, 1-b1, 1-b2, eps, d = fl(1 - lr wd), step = fl(lr / bc1), q = sqrtf(bc2), s = grad_scale):

    G = g s                                   |dG| <= U |G|
    M = m + (G - m)(1 - b1)                   |dM| <= U [(1 - b1)(|G| + 2 |G - m|) + |M|]
            fl(G - m) carries dG and U |G - m|; the product adds U (1 - b1)|G - m|; the sum U |M|.  Where m nearly
            cancels, |M| is far below |G| and |m| and the RELATIVE error of M is large: the bound stays absolute.
    V = b2 v + (1 - b2) G G                   |dV| <= U [4 (1 - b2) G^2 + b2 v + V]
            ((1 - b2) G) G: two products on a G that is U off twice -> 4 U; b2 v: U; the sum: U V.
    D = sqrt(V) / q + eps                     |dR| <= dV / (2 sqrt V) + U sqrt V    (R = sqrt V; 0 where V = 0)
                                              |dD| <= dR / q + U R / q + U D
    W = step (M / D)                          |dW| <= step (dM / D + |M| dD / D^2) + 2 U |W|
    P = p d - W                               |dP| <= dW + ulp(max(|p|, |P|))
            the two roundings of p, fl(p d) and the final difference, are each at most half an ulp of their result, and
            |p d| <= |p|: together one ulp of the larger of old and new p.

`adamw_step` returns P, M, V and these three bounds.  It also carries errors that enter with the state (dp, dm, dv, dg:
the bounds of an earlier step, or of a gradient that a clip scaled) and, with scalar_err=True, the distance to the same
step taken with UNROUNDED scalars (torch.optim.AdamW in float64): one U on each of lr, b2, 1-b1, 1-b2, eps, three on
step (lr, bc1, the division), one and a half on q (bc2, sqrtf), and U (1 + 2 lr wd) on d.  `adamw_iterate` chains steps
that way: the tolerance of FusedAdamW.step over several steps against torch in float64.

Clip (clip_coef_kernel): the parts are fp64 sums of fp64 squares (wfae_sumsq), so total = fl(fl(sqrt S) pre_scale) is
2 U off and coef = fl(max_norm / fl(total + 1e-6)) two more, plus U on each of max_norm and pre_scale as they are
handed over: CLIP_REL = 6 U on the coefficient, NORM_REL = 3 U on the norm.  min(1, .) as torch.clamp(max=1) has it: a
NaN norm gives NaN, an infinite one 0.

reduce_sum: chan_reduce_kernel's vector path adds fp32 sums of four, (a + b) + (c + d): each value passes two fp32
additions (2 U) and the quad is converted once (U): 3 U sum|x|, then fp64.  Its scalar path and colsum_kernel convert each
value to fp64 first.  The fp64 additions are below 2^-53 (n + 2) sum|x| in any order (counted twice: the float64 sum here has them too).  All of them round the
result to fp32 once: half an ulp of it; with accumulate the sum fl(out + fl(S)) rounds twice.
"""
from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
CLIP_REL = 6.0 * U
NORM_REL = 3.0 * U
f32 = np.float32


def ulp32(x):
    """spacing of fp32 at |x| (float64 in, float64 out)"""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(f32)).astype(np.float64)


def worst(got, ref, bound):
    """largest |got - ref| / bound over the elements; 0 / 0 counts as 0, an error where the bound is 0 as inf"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    return float(np.max(r))


def report(kernel, case, *ratios):
    """the line profiles/optim_glue_fp64_errors.txt keeps: largest error as a fraction of its bound"""
    print(f"optim_fp64 {kernel:<24} {case:<44} " + " ".join(f"{r:6.3f}" for r in ratios))


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


# ------------------------------------------------------------------ AdamW ---
# lr, betas, eps, wd, t, grad_scale, |g|, |p|; zero: g = m = v = 0
CASES = [
    dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, wd=1e-2, t=1, grad_scale=1.0, g=1.0, p=1.0),
    dict(lr=1e-2, betas=(0.95, 0.999), eps=1e-8, wd=0.1, t=7, grad_scale=0.5, g=1e-3, p=1e-3),
    dict(lr=5e-5, betas=(0.85, 0.999), eps=1e-8, wd=1e-4, t=10000, grad_scale=1.0 / 3.0, g=1e-9, p=1.0),
    dict(lr=1e-3, betas=(0.5, 0.9), eps=1e-3, wd=0.0, t=2, grad_scale=1.0, g=1e-4, p=1.0),
    dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, wd=1e-2, t=3, grad_scale=1.0, g=0.0, p=1.0, zero=True),
    dict(lr=0.1, betas=(0.9, 0.999), eps=1e-8, wd=0.5, t=1, grad_scale=1.0, g=1.0, p=1.0),
]
SIZES = [1, 3, 255, 256, 257, 4099, 4194304 + 1027]   # the last: past the 4096-block cap of grid_1d, grid-stride path


def case_args(case):
    """(lr, b1, b2, eps, wd, bc1, bc2, grad_scale) as FusedAdamW.step forms them at step t"""
    b1, b2 = case["betas"]
    t = case["t"]
    return (case["lr"], b1, b2, case["eps"], case["wd"], 1.0 - b1 ** t, 1.0 - b2 ** t, case["grad_scale"])


def case_state(case, n, seed):
    """fp32 p, g, m, v of n elements.  At t > 1 the moments are those of a history of gradients of the same size: m of
    either sign (so that m + (G - m)(1 - b1) cancels on some elements), v around G^2."""
    r = np.random.default_rng(seed)
    p = (case["p"] * r.standard_normal(n)).astype(f32)
    if case.get("zero"):
        z = np.zeros(n, f32)
        return p, z.copy(), z.copy(), z.copy()
    g = (case["g"] * r.standard_normal(n)).astype(f32)
    if case["t"] == 1:
        return p, g, np.zeros(n, f32), np.zeros(n, f32)
    gs = case["g"] * case["grad_scale"]
    m = (0.5 * gs * r.standard_normal(n)).astype(f32)
    v = (gs * gs * r.uniform(0.1, 2.0, n)).astype(f32)
    return p, g, m, v


def decay_factors(lr, wd):
    """fl(1 - lr wd) with the product rounded first, and as one fused operation: the compiler may pick either"""
    lr32, wd32 = f32(lr), f32(wd)
    return float(f32(1.0) - lr32 * wd32), float(f32(1.0 - float(lr32) * float(wd32)))


def kernel_scalars(lr, b1, b2, eps, wd, bc1, bc2, grad_scale, exact_complements, round_scalars=True):
    """the scalars of the kernel's loop, as float64 values"""
    if not round_scalars:
        return dict(lr=lr, b2=b2, omb1=1.0 - b1, omb2=1.0 - b2, eps=eps, wd=wd, d=1.0 - lr * wd, step=lr / bc1,
                    q=math.sqrt(bc2), s=grad_scale)
    lr32, b132, b232 = f32(lr), f32(b1), f32(b2)
    if exact_complements:
        omb1, omb2 = f32(1.0 - b1), f32(1.0 - b2)
    else:
        omb1, omb2 = f32(1.0) - b132, f32(1.0) - b232
    return dict(lr=float(lr32), b2=float(b232), omb1=float(omb1), omb2=float(omb2), eps=float(f32(eps)), wd=float(f32(wd)),
                d=decay_factors(lr, wd)[1], step=float(lr32 / f32(bc1)), q=float(np.sqrt(f32(bc2))), s=float(f32(grad_scale)))


def adamw_step(p, g, m, v, lr, b1, b2, eps, wd, bc1, bc2, grad_scale, exact_complements, *, round_scalars=True,
               dp=None, dm=None, dv=None, dg=None, scalar_err=False):
    """-> P, M, V (float64) and the bounds bP, bM, bV of one kernel step from this state (module docstring)"""
    k = kernel_scalars(lr, b1, b2, eps, wd, bc1, bc2, grad_scale, exact_complements, round_scalars)
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    zero = np.zeros_like(p)
    dp, dm, dv, dg = (zero if a is None else np.asarray(a, dtype=np.float64) for a in (dp, dm, dv, dg))
    se = 1.0 if scalar_err else 0.0
    s, omb1, omb2, b2k, d, step, q = k["s"], k["omb1"], k["omb2"], k["b2"], k["d"], k["step"], k["q"]

    G = g * s
    dG = U * np.abs(G) + s * dg + se * U * np.abs(G)   # its own rounding, what came with g, the rounding of s
    M = m + (G - m) * omb1
    # dM / dG = omb1 and dM / dm = 1 - omb1 carry what came in; fl(G - m) and the product: 2 U omb1 |G - m|; the sum: U |M|
    bM = omb1 * dG + (1.0 - omb1) * dm + 2.0 * U * omb1 * np.abs(G - m) + U * np.abs(M) + se * U * omb1 * np.abs(G - m)
    V = b2k * v + omb2 * G * G
    # dV / dG = 2 omb2 G (with dG = U |G|: 2 U omb2 G^2); the two products of (omb2 G) G: 2 U omb2 G^2; b2 v: U; the sum: U V
    bV = (2.0 * omb2 * np.abs(G) * dG + U * (2.0 * omb2 * G * G + b2k * v + V) + b2k * dv
          + se * U * (omb2 * G * G + b2k * v))
    R = np.sqrt(V)
    with np.errstate(divide="ignore", invalid="ignore"):
        bR = np.where(V > 0.0, bV / (2.0 * R), np.sqrt(bV)) + U * R
    D = R / q + k["eps"]
    bD = bR / q + U * R / q + U * D + se * (1.5 * U * R / q + U * k["eps"])
    W = step * (M / D)
    bW = step * (bM / D + np.abs(M) * bD / (D * D)) + 2.0 * U * np.abs(W) + se * 3.0 * U * np.abs(W)
    P = p * d - W
    bP = SLACK * (bW + d * dp + se * U * (1.0 + 2.0 * k["lr"] * k["wd"]) * np.abs(p)) + ulp32(np.maximum(np.abs(p), np.abs(P)))
    return P, M, V, bP, SLACK * bM, SLACK * bV


def adamw_iterate(p, grads, lr, betas, eps, wd, grad_scale, exact_complements, dgs=None):
    """`len(grads)` steps from zero moments, t = 1, 2, ...: P, M, V of the rounded-scalar recursion and the bounds on the
    distance of an fp32 run of the kernel to torch.optim.AdamW in float64 with unrounded scalars (scalar_err).  dgs: per
    step, how far the gradient the kernel reads may be from grads[t]"""
    P = np.asarray(p, dtype=np.float64)
    M, V = np.zeros_like(P), np.zeros_like(P)
    bP, bM, bV = np.zeros_like(P), np.zeros_like(P), np.zeros_like(P)
    b1, b2 = betas
    for t, g in enumerate(grads, 1):
        P, M, V, bP, bM, bV = adamw_step(P, g, M, V, lr, b1, b2, eps, wd, 1.0 - b1 ** t, 1.0 - b2 ** t, grad_scale,
                                         exact_complements, dp=bP, dm=bM, dv=bV, dg=None if dgs is None else dgs[t - 1],
                                         scalar_err=True)
    return P, M, V, bP, bM, bV


# ------------------------------------------------------------------- clip ---
def clip(chunks, max_norm, pre_scale=1.0):
    """torch.nn.utils.clip_grad_norm_ on pre_scale * chunks -> (coef, total norm), float64: min(1, max_norm / (norm +
    1e-6)) as torch.clamp(max=1) computes it: NaN stays NaN, an infinite norm gives 0"""
    ss = 0.0
    for c in chunks:
        c = np.asarray(c, dtype=np.float64).ravel()
        ss += float(np.sum(c * c))
    total = math.sqrt(ss) * float(pre_scale)
    if math.isnan(total):
        return float("nan"), float("nan")
    coef = float(max_norm) / (total + 1e-6)
    return (1.0 if coef > 1.0 else coef), total


def adaptive_weight(ss_rec, ss_disc, disc_weight=1.0):
    """Loss.calculate_adaptive_weight from the two sums of squares: clamp(disc_weight |rec| / (|disc| + 1e-4), 0, 1e4);
    torch.clamp keeps a NaN"""
    w = float(disc_weight) * (math.sqrt(ss_rec) / (math.sqrt(ss_disc) + 1e-4))
    if math.isnan(w):
        return float("nan")
    return min(max(w, 0.0), 1e4)


# the two square roots converted to fp32, the constant 1e-4f, the sum, the quotient, the product, disc_weight as handed over
ADAPTIVE_REL = 7.0 * U


# -------------------------------------------------------------- reductions ---
def reduce_sum_bound(x, axes, vector, accumulate_onto=None):
    """x: the float64 view of the fp32 data with the reduced axes `axes` -> (sum, bound) per remaining element"""
    x = np.asarray(x, dtype=np.float64)
    S, A = x.sum(axis=axes), np.abs(x).sum(axis=axes)
    n = x.size // max(S.size, 1)
    b = (3.0 * U if vector else 0.0) * A + 2.0 ** -52 * (n + 2) * A   # the fp64 additions, in any order: the kernel's and this sum's
    if accumulate_onto is None:
        return S, SLACK * b + 0.5 * ulp32(S)
    T = np.asarray(accumulate_onto, dtype=np.float64) + S
    return T, SLACK * b + 0.5 * ulp32(S) + 0.5 * ulp32(T)


# ------------------------------------------------------------ element-wise ---
EXP_ULPS = 2.0


def sigmoid_bound(x):
    """1 / (1 + expf(-x)): (sigmoid in float64, bound).  expf is within EXP_ULPS ulp (the device library states 1; 2 are
    counted), e = exp(-x): y = 1 / (1 + e) moves by y (1 - y) times the relative error of e; the sum and the quotient add
    U y each.  Where expf overflows (x < -88.7) the result is 1 / inf = 0 against a true value below 2^-126; where e
    underflows the result is exactly 1.  The absolute floor is 2^-126, the smallest normal number: below it the format
    promises no relative precision, and a denormal quotient may be flushed."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore"):
        y = 1.0 / (1.0 + np.exp(-x))
    b = SLACK * (y * (1.0 - y) * EXP_ULPS * 2.0 * U + 2.0 * U * y) + 2.0 ** -126
    return y, b


def gelu_exact(u):
    u = np.asarray(u, dtype=np.float64)
    return 0.5 * u * (1.0 + _erf(u / math.sqrt(2.0)))


def gelu_grad_exact(u):
    u = np.asarray(u, dtype=np.float64)
    return 0.5 * (1.0 + _erf(u / math.sqrt(2.0))) + u * np.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


def _erf(z):
    import torch   # numpy has no erf; torch's float64 erf is what test_gelu_tracks_exact_erf_form uses
    return torch.erf(torch.from_numpy(np.ascontiguousarray(z, dtype=np.float64))).numpy()


# the figures csrc/common.h states for its tail form of GELU, as tests/test_kernels_gpu.py::test_gelu_tracks_exact_erf_form
# holds them on its grid: relative 8e-7 for u > 0, 1e-5 for -3 < u < 0, absolute 1e-6 everywhere; derivative absolute 4e-7
GELU_REL_POS, GELU_REL_NEG, GELU_ABS, GELU_GRAD_ABS = 8e-7, 1e-5, 1e-6, 4e-7


def gelu_bounds(u):
    """-> (exact, bound): the tightest of the stated figures that applies to each element"""
    y = gelu_exact(u)
    u = np.asarray(u, dtype=np.float64)
    b = np.full(u.shape, GELU_ABS)
    b = np.where(u > 0, np.minimum(b, GELU_REL_POS * np.abs(y)), b)
    b = np.where((u < 0) & (u > -3), np.minimum(b, GELU_REL_NEG * np.abs(y)), b)
    return y, b


def gelu_bwd_bounds(dy, u):
    """dy * gelu'(u): the derivative's absolute figure scaled by |dy|, and the rounding of the product"""
    dy = np.asarray(dy, dtype=np.float64)
    e = dy * gelu_grad_exact(u)
    return e, np.abs(dy) * GELU_GRAD_ABS + U * np.abs(e)
