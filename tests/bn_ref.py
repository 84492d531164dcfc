"""Plain float64 restatement (torch on the CPU, no library import) of the BatchNorm2d chain of csrc/norm_act.hip and of every
kernel that produces its sums: batch statistics with the folded scale / shift and the running-statistics update, the
apply pass with its three activations, the two backward sums and dx in training and eval form — together with the error
bounds the fp32 kernels are held to and the seeded inputs on which they are held.

Stage isolation: every function takes the statistics it depends on as arguments, so a test can hand in the GPU's own fp32
scale / shift / save_mean / save_invstd / coef and judge a kernel on its own arithmetic, not on the error it inherits.

Bounds: each one is a function of the inputs and of a count of fp32 roundings (U = 2^-24 each) read from the kernel's
code; the counts are the K_* constants below, each with the line it was counted from.  tests/test_bn_ref_cpu.py holds the
restatement to torch's float64 autograd and the bounds to a numpy emulation of the kernels' arithmetic."""
import math

import numpy as np
import torch

U = 2.0 ** -24          # unit roundoff of fp32 (round to nearest)
U64 = 2.0 ** -53        # of fp64: the accumulators behind the fp32 sums of four
TINY = 2.0 ** -126      # smallest normal fp32: a result below it may be flushed to zero
FP64_SLACK = 2.0 ** -40 # references and bounds are themselves evaluated in fp64: a correctly rounded fp32 result may sit at 1.0 of its bound
LEAKY = 0.2             # nn.LeakyReLU(0.2), act 2
ACTS = (0, 1, 2)        # identity, exact-erf GELU, LeakyReLU(0.2)

# ---- rounding counts (norm_act.hip; every producer epilogue restates the same two expressions: gemm.hip E_BATCHED vector
# epilogue, c1r.hip store_pass STATS, c1b.hip / c1rb.hip epilogues, wino.hip wino_out_kernel / wino_in_t_kernel STATS)
# chan_reduce_kernel, vector path: `(v[q] + v[q+1]) + (v[q+2] + v[q+3])` — a value passes through 2 fp32 additions before
# the fp64 accumulator (the scalar path adds in fp64: 0)
K_SUM = 2
# chan_reduce_kernel, vector path: `fmaf(v, v, v1 * v1) + fmaf(...)` — a square passes through at most 3 roundings (the
# product v1 * v1, the fma, the addition of the two halves); the scalar path squares in fp64: 0
K_SQ = 3
# bn_finalize_kernel: `save_invstd = (float)(1.0 / sqrt(var + eps))` — the (float), and one for the fp64 root and quotient
K_INVSTD = 2
# bn_finalize_kernel: `a = gamma[c] * invstd` — 1 rounding
K_SCALE = 1
# bn_finalize_kernel: `shift = beta[c] - meanf * a` — product and difference (one fma under -ffp-contract=on): at most 2
K_SHIFT = 2
# bn_finalize_kernel: `(1.f - momentum) * running + momentum * stat` — the complement and its product (2) on the first term,
# the second product (1, the (float) of the unbiased variance makes it 2 for running_var), the sum (1): at most 3 of
# |first term| + |second term|
K_RUNNING = 3
# bn_act_fwd_kernel: `act_f(fmaf(v, a, b))` — 1 rounding in front of the activation
K_APPLY = 1
# bn_act_bwd_reduce_kernel quad(): `dv * act_grad_f(fmaf(xv, a, b))` — the fma in front of act' (1, scaled by the Lipschitz
# constant of act') and the product (1)
K_DU = 1
# quad(): `(xv - mu) * is` — 2 roundings
K_XHAT = 2
# bn_bwd_finalize_kernel: `(float)s1` — 1 rounding of the total (accumulate: one more addition)
K_FINAL = 1
# bn_act_bwd_dx_kernel one(): `gi * (du - k1 - xh * k2) + rv` with gi = gamma * is (1), k1, k2 = coef * inv_count with
# inv_count = 1.0f / (float)n (2 each), xh (2), the product xh * k2 (1), two subtractions (2), the product with gi (1) and
# the final addition (1): 2 |k1| + 5 |xh k2| + 2 T + 2 T + T <= 10 T with T = |dU| + |k1| + |xh k2|
K_DX = 10

GELU_LIP = 1.13         # max |gelu'|
GELU_GRAD_LIP = 0.8     # max |gelu''| = 2 phi(0)
# the activation's own error: the bars of tests/test_kernels_gpu.py::test_gelu_tracks_exact_erf_form
GELU_ABS = 1e-6         # |gelu_f(u) - gelu(u)|, every u
GELU_REL_POS = 8e-7     # relative, u > 0
GELU_REL_NEG = 1e-5     # relative, -3 < u < 0
GELU_GRAD_ABS = 4e-7    # |gelu_grad_f(u) - gelu'(u)|


def _d(t):
    return None if t is None else torch.as_tensor(t).detach().to("cpu", torch.float64)


def _pc(v):
    """per-channel vector -> (1, C, 1, 1)"""
    return _d(v).view(1, -1, 1, 1)


def act64(u, act):
    if act == 1:     # erfc, not 1 + erf: the left tail (u Phi(u) = -8e-17 at u = -8.5) survives in float64
        return 0.5 * u * torch.special.erfc(-u / math.sqrt(2.0))
    if act == 2:
        return torch.where(u > 0, u, LEAKY * u)
    return u


def act_grad64(u, act):
    if act == 1:
        return 0.5 * torch.special.erfc(-u / math.sqrt(2.0)) + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
    if act == 2:
        return torch.where(u > 0, torch.ones_like(u), torch.full_like(u, LEAKY))
    return torch.ones_like(u)


class Stats64:
    __slots__ = ("n", "mean", "var", "invstd", "scale", "shift", "running_mean", "running_var", "abs_mean", "sq_mean")


def stats64(x, gamma=None, beta=None, eps=1e-5, running_mean=None, running_var=None, momentum=0.1):
    """batch statistics of x (N, C, H, W): mean, biased variance (two-pass), invstd, folded scale = gamma invstd and
    shift = beta - mean scale, and the running-statistics update with the unbiased variance; E|x| and E[x^2] for the bounds"""
    x = _d(x)
    s = Stats64()
    s.n = x.shape[0] * x.shape[2] * x.shape[3]
    s.mean = x.mean(dim=(0, 2, 3))
    s.var = ((x - s.mean.view(1, -1, 1, 1)) ** 2).mean(dim=(0, 2, 3))
    s.invstd = 1.0 / torch.sqrt(s.var + eps)
    g = torch.ones_like(s.mean) if gamma is None else _d(gamma)
    b = torch.zeros_like(s.mean) if beta is None else _d(beta)
    s.scale = g * s.invstd
    s.shift = b - s.mean * s.scale
    s.running_mean = s.running_var = None
    if running_mean is not None:
        unb = s.var * (s.n / (s.n - 1.0)) if s.n > 1 else s.var
        s.running_mean = (1.0 - momentum) * _d(running_mean) + momentum * s.mean
        s.running_var = (1.0 - momentum) * _d(running_var) + momentum * unb
    s.abs_mean = x.abs().mean(dim=(0, 2, 3))
    s.sq_mean = (x * x).mean(dim=(0, 2, 3))
    return s


def fold_eval64(gamma, beta, running_mean, running_var, eps=1e-5):
    """(mean, invstd, scale, shift) of eval mode"""
    invstd = 1.0 / torch.sqrt(_d(running_var) + eps)
    scale = _d(gamma) * invstd
    return _d(running_mean), invstd, scale, _d(beta) - _d(running_mean) * scale


def apply64(x, scale, shift, act):
    return act64(_d(x) * _pc(scale) + _pc(shift), act)


def bwd_terms64(dy, x, scale, shift, mean, invstd, act):
    """(u, dU, xhat): the pre-activation, dU = dy act'(u) and xhat = (x - mean) invstd"""
    x = _d(x)
    u = x * _pc(scale) + _pc(shift)
    return u, _d(dy) * act_grad64(u, act), (x - _pc(mean)) * _pc(invstd)


def bwd_sums64(dy, x, scale, shift, mean, invstd, act):
    """per channel (sum dU, sum dU xhat) = (dbeta, dgamma)"""
    _, du, xh = bwd_terms64(dy, x, scale, shift, mean, invstd, act)
    return du.sum(dim=(0, 2, 3)), (du * xh).sum(dim=(0, 2, 3))


def bwd_dx64(dy, x, gamma, scale, shift, mean, invstd, act, training=True, coef=None, res=None):
    """dx = gamma invstd (dU - sum dU / n - xhat sum dU xhat / n) (+ res); eval mode drops both sums.  coef = (sum dU,
    sum dU xhat): the GPU's own fp32 sums when given, else the float64 sums of this restatement"""
    _, du, xh = bwd_terms64(dy, x, scale, shift, mean, invstd, act)
    gi = _pc(gamma) * _pc(invstd)
    if training:
        n = du.shape[0] * du.shape[2] * du.shape[3]
        s1, s2 = (du.sum(dim=(0, 2, 3)), (du * xh).sum(dim=(0, 2, 3))) if coef is None else (_d(coef[0]), _d(coef[1]))
        dx = gi * (du - _pc(s1) / n - xh * (_pc(s2) / n))
    else:
        dx = gi * du
    return dx if res is None else dx + _d(res)


# ------------------------------------------------------------------------------------------------------------ bounds
def fp32_exact_channels(x):
    """per channel: True where no fp32 sum of four values or of four squares can round — every value is a multiple of one
    power of two q with 4 max(x / q)^2 < 2^24 (zeros, the 1/8 grid of the `grid` class).  There the count of fp32 roundings
    is 0 and the kernels owe the float64 result"""
    x = _d(x)
    a = x.abs().permute(1, 0, 2, 3).reshape(x.shape[1], -1)
    top = a.max(dim=1).values
    # the finest grid the magnitude allows: the largest k with 4 (max 2^k)^2 < 2^24; a channel on a coarser grid is on this one
    k = torch.floor(torch.log2(2047.0 / top.clamp_min(2.0 ** -1000)))
    v = a * torch.exp2(k).view(-1, 1)
    return (top == 0) | ((v == v.floor()).all(dim=1) & (4.0 * v.max(dim=1).values ** 2 < 2.0 ** 24))


def sum_counts(x, vector=True):
    """(k_sum, k_sq) per channel for a kernel that takes the sums of x: K_SUM / K_SQ on the vector path, 0 on the scalar path
    (chan_reduce_kernel adds `v` and `(double)v * v` in fp64 there) and on channels where the fp32 stage cannot round"""
    live = (~fp32_exact_channels(x)).double() * (1.0 if vector else 0.0)
    return K_SUM * live, K_SQ * live


def mean_bound(s, k=K_SUM):
    """|mean - mean64| <= k U E|x| + U |mean64|  (the sums of four, the final (float)); n U64 E|x| for the fp64 accumulators"""
    return k * U * s.abs_mean + U * s.mean.abs() + s.n * U64 * s.abs_mean


def var_bound(s, k_sum=K_SUM, k_sq=K_SQ):
    """|var - var64| for var = S2 / n - mean^2 formed in fp64 from sums whose terms carry k_sq / k_sum fp32 roundings:
    k_sq U E[x^2] from S2, and 2 |mean| (k_sum U E|x|) + (k_sum U E|x|)^2 from the square of the fp64 mean; as |mean| <=
    E|x| <= sqrt(E[x^2]) this is at most (k_sq + 2 k_sum) U E[x^2] = 7 U E[x^2].  (3 n + 4) U64 E[x^2] covers the fp64
    accumulation of both sums and the finalize arithmetic"""
    dm = k_sum * U * s.abs_mean
    return k_sq * U * s.sq_mean + 2.0 * s.mean.abs() * dm + dm * dm + (3 * s.n + 4) * U64 * s.sq_mean


def invstd_rel_bound(s, eps=1e-5, dvar=None):
    """relative: (1/2) |dvar| / (var64 + eps) + K_INVSTD U"""
    dvar = var_bound(s) if dvar is None else dvar
    return 0.5 * dvar / (s.var + eps) + K_INVSTD * U


def running_bound(momentum, running, stat, dstat):
    """K_RUNNING U (|(1 - m) running| + |m stat|) + m dstat  (dstat: the error the statistic itself is allowed)"""
    return K_RUNNING * U * ((1.0 - momentum) * _d(running).abs() + momentum * _d(stat).abs()) + momentum * dstat


def act_error(u64, y64, act):
    """the activation's own error at y64 = act(u64) (0 for the two piecewise-linear ones): for GELU the three bars of
    test_gelu_tracks_exact_erf_form — relative for u > 0 (the absolute one cannot hold above 1.25: half an ulp of 30 is
    1e-6), the smaller of the relative and the absolute one on -3 < u < 0, the absolute one below"""
    if act != 1:
        return torch.zeros_like(y64)
    mid = torch.minimum(torch.full_like(y64, GELU_ABS), GELU_REL_NEG * y64.abs())
    return torch.where(u64 > 0, GELU_REL_POS * y64.abs(), torch.where(u64 > -3.0, mid, torch.full_like(y64, GELU_ABS)))


def apply_bound(x, scale, shift, act):
    """per element |y - y64|: K_APPLY U |u| through the activation's Lipschitz constant, plus the activation's own error"""
    u = _d(x) * _pc(scale) + _pc(shift)
    lip = GELU_LIP if act == 1 else 1.0
    return lip * K_APPLY * U * u.abs() + act_error(u, act64(u, act), act) + TINY


def du_bound(dy, u, du, act):
    """per element |dU - dU64|: the fma in front of act' (U |u| times the Lipschitz constant of act'), act's own error, the
    product"""
    dy = _d(dy).abs()
    if act == 1:
        return dy * (GELU_GRAD_ABS + GELU_GRAD_LIP * U * u.abs()) + K_DU * U * du.abs()
    return K_DU * U * du.abs()      # act' is piecewise constant and the sign of a rounded fma is that of the exact value


def bwd_sums_bound(dy, x, scale, shift, mean, invstd, act, accumulate_into=None, finals=K_FINAL):
    """(|S1 - S1_64|, |S2 - S2_64|) per channel, relative to the sums of magnitudes: K_SUM U sum |dU| and K_SQ U sum |dU xhat|
    for the sums of four, the fp32 error of forming dU and xhat per element, and the final rounding(s) to fp32 (finals=0: the
    fp64 totals of a producer's partial rows, not yet rounded)"""
    u, du, xh = bwd_terms64(dy, x, scale, shift, mean, invstd, act)
    ddu = du_bound(dy, u, du, act)
    dxh = K_XHAT * U * xh.abs()
    red = (0, 2, 3)
    s1, s2 = du.sum(dim=red), (du * xh).sum(dim=red)
    b1 = ddu.sum(dim=red) + K_SUM * U * du.abs().sum(dim=red) + finals * U * s1.abs()
    b2 = (ddu * xh.abs() + du.abs() * dxh).sum(dim=red) + K_SQ * U * (du * xh).abs().sum(dim=red) + finals * U * s2.abs()
    if accumulate_into is not None:      # `dbeta[c] + (float)s1`: one more addition
        b1 = b1 + U * (_d(accumulate_into[1]) + s1).abs()
        b2 = b2 + U * (_d(accumulate_into[0]) + s2).abs()
    return b1, b2


def dx_bound(dy, x, gamma, scale, shift, mean, invstd, act, training=True, coef=None, res=None):
    """per element |dx - dx64|: |gi| (d(dU) + K_DX U (|dU| + |k1| + |xhat k2|)) + U |res|"""
    u, du, xh = bwd_terms64(dy, x, scale, shift, mean, invstd, act)
    gi = (_pc(gamma) * _pc(invstd)).abs()
    t = du.abs()
    if training:
        n = du.shape[0] * du.shape[2] * du.shape[3]
        t = t + _pc(coef[0]).abs() / n + (xh * (_pc(coef[1]) / n)).abs()
    b = gi * (du_bound(dy, u, du, act) + K_DX * U * t)
    return b if res is None else b + U * _d(res).abs()


def bf16_round(t64):
    """float64 -> the bf16 value nearest to it, as float64"""
    return t64.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def bf16_mismatch(got_bf16, ref64, bound):
    """number of elements of a bf16 result that are not the correctly rounded bf16 of ref64, allowing the neighbouring bf16
    value only where ref64 lies within `bound` (the fp32 bound) of a rounding boundary: got must lie between the roundings
    of ref64 - bound and ref64 + bound (rounding is monotone), and within one bf16 ulp (2^-7 relative covers it) of ref's"""
    return len(bf16_offenders(got_bf16, ref64, bound, limit=None))


def bf16_offenders(got_bf16, ref64, bound, limit=5):
    """[(flat index, got, ref64, bound)] of the elements bf16_mismatch counts (TINY: flush to zero at the underflow threshold)"""
    got = got_bf16.detach().to("cpu", torch.float64)
    lo, hi, mid = bf16_round(ref64 - bound), bf16_round(ref64 + bound), bf16_round(ref64)
    ok = (got >= lo - TINY) & (got <= hi + TINY) & ((got - mid).abs() <= 2.0 ** -7 * mid.abs() + TINY)
    idx = (~ok).flatten().nonzero().flatten().tolist()
    return [(i, float(got.flatten()[i]), float(ref64.flatten()[i]), float(bound.flatten()[i])) for i in idx[:limit]]


# ------------------------------------------------------------------------------------------------------ input generators
X_CLASSES = ("benign", "offset10", "offset100", "const0", "const", "sparse", "spike", "tiny", "grid")
DY_CLASSES = ("uniform", "l1like", "cancelling")
# the shapes the tests run on: the scalar path of norm_act.hip (HW % 4 != 0), its vector path, several splits per channel
# with a partial last one, a wide tensor
GENERIC_SHAPES = [(3, 5, 7, 9), (3, 8, 12, 12), (2, 3, 96, 96), (5, 64, 16, 8)]
# bf16 storage moves 8 values per 16-byte access: two shapes on the vector path (144 and 120 = 8 * 15 values per plane) and
# one on the scalar path (110: HW % 8 != 0); (3, 5, 7, 9) of the list above is a second scalar one
BF16_SHAPES = [(3, 8, 12, 12), (2, 16, 10, 12), (2, 16, 10, 11)]
# fewer than nine channels cannot hold every class: the ones that bite at the sizes of the tests
CLASSES_OF = {3: ("offset100", "grid", "spike"), 5: ("benign", "offset100", "const", "sparse", "grid"),
              8: ("benign", "offset10", "offset100", "const0", "const", "sparse", "spike", "grid")}


def classes_for(c):
    return CLASSES_OF.get(c, X_CLASSES)

CONST_VALUE = float(np.float32(3.7))      # representable, and neither it nor its square is a short binary fraction


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def channel(cls, count, seed):
    """`count` fp32 values of one channel class"""
    g = _gen(seed)
    if cls == "benign":
        v = 0.5 + 2.0 * torch.randn(count, generator=g)
    elif cls == "offset10":
        v = 10.0 + torch.randn(count, generator=g)
    elif cls == "offset100":
        v = 100.0 + torch.randn(count, generator=g)
    elif cls == "const0":
        v = torch.zeros(count)
    elif cls == "const":
        v = torch.full((count,), CONST_VALUE)
    elif cls == "sparse":
        v = torch.rand(count, generator=g) * (torch.rand(count, generator=g) < 0.1)
    elif cls == "spike":
        v = torch.randn(count, generator=g)
        v[int(torch.randint(count, (1,), generator=g))] = 1e3
    elif cls == "tiny":
        v = 1e-4 * torch.randn(count, generator=g)
    elif cls == "grid":     # 100 +- 4 on a grid of 1/8: no fp32 sum of four values or squares rounds (fp32_exact_channels)
        v = 100.0 + torch.randint(-32, 33, (count,), generator=g).float() / 8.0
    else:
        raise ValueError(cls)
    return v.float()


def mixed(shape, seed, classes=X_CLASSES):
    """fp32 tensor (N, C, H, W) whose channel c is of class classes[c % len(classes)] -> (x, [class of each channel]); the
    vector body and the scalar tail of a launch meet every class"""
    nb, c, h, w = shape
    names = [classes[i % len(classes)] for i in range(c)]
    x = torch.empty(shape, dtype=torch.float32)
    for i, cls in enumerate(names):
        x[:, i] = channel(cls, nb * h * w, seed * 1000 + i).view(nb, h, w)
    return x, names


def grad(shape, kind, seed):
    """the cotangent classes: 'uniform' U(-1, 1); 'l1like' +-1/N (what the L1 loss sends down); 'cancelling': every channel
    sums to exactly 0 (values on a 2^-10 grid, each with its negative: any summation order gives 0 in fp64; an odd count
    leaves one 0)"""
    nb, c, h, w = shape
    g = _gen(seed)
    if kind == "uniform":
        return (torch.rand(shape, generator=g) * 2 - 1).float()
    if kind == "l1like":
        return ((torch.randint(0, 2, shape, generator=g) * 2 - 1).float() / float(nb * c * h * w)).float()
    if kind == "cancelling":
        n = nb * h * w
        out = torch.zeros((c, n), dtype=torch.float32)
        for i in range(c):
            half = torch.randint(-1024, 1025, (n // 2,), generator=g).float() / 1024.0
            v = torch.cat([half, -half, torch.zeros(n - 2 * (n // 2))])
            out[i] = v[torch.randperm(n, generator=g)]
        return out.view(c, nb, h, w).permute(1, 0, 2, 3).contiguous()
    raise ValueError(kind)


def offset_rows(weight, rows_ratio, m_over_s, taps=None):
    """make output channels of a convolution fed with x = m + s N(0, 1) land at chosen |mean| / sigma: row r of `weight`
    (Cout, K) or (Cout, K, kh, kw) gets zero sum over the taps that carry the mean plus a constant d on them, so that
    mean = m d T and sigma = s ||w||, with d solved from ratio = (m / s) T d / sqrt(||r||^2 + T d^2).  `taps`: boolean mask
    (kh, kw) of the taps every output pixel sees (the interior taps of a padded 4x4 stride-2 convolution); None = all"""
    w = weight.clone().double()
    co = w.shape[0]
    flat = w.view(co, w.shape[1], -1)
    mask = torch.ones(flat.shape[2], dtype=torch.bool) if taps is None else taps.reshape(-1)
    for r, ratio in rows_ratio.items():
        row = flat[r]
        row -= row.mean(dim=0, keepdim=True)                    # every tap: zero sum over the input channels
        t = float(mask.sum()) * row.shape[0]
        q = ratio / m_over_s
        assert q * q < t, "ratio out of reach for this fan-in"
        d = math.sqrt(q * q * float((row * row).sum()) / (t * t - q * q * t))
        row[:, mask] += d
    return w.float()


def emulate_sums(x, width=4):
    """numpy emulation of chan_reduce_kernel's arithmetic on x (N, C, H, W) fp32 -> fp64 (S1, S2) per channel: with
    HW % 4 == 0 fp32 sums of four consecutive values and of their squares (product, fma, addition) enter fp64 accumulators;
    otherwise every value and its exact square are added in fp64"""
    a = np.ascontiguousarray(x.detach().cpu().numpy().astype(np.float32))
    nb, c, h, w = a.shape
    if (h * w) % width:
        d = a.astype(np.float64)
        return d.sum(axis=(0, 2, 3)), (d * d).sum(axis=(0, 2, 3))
    q = a.reshape(nb, c, h * w // 4, 4)
    v0, v1, v2, v3 = (q[..., i] for i in range(4))
    s1 = ((v0 + v1) + (v2 + v3)).astype(np.float64)

    def fma(p, r):      # float32(p * p + r): p * p is exact in fp64
        return (p.astype(np.float64) * p.astype(np.float64) + r.astype(np.float64)).astype(np.float32)
    s2 = (fma(v0, v1 * v1) + fma(v2, v3 * v3)).astype(np.float64)
    return s1.sum(axis=(0, 2)), s2.sum(axis=(0, 2))


def emulate_stats(x, eps=1e-5, width=4):
    """(mean, var, invstd) in fp64 as bn_finalize_kernel forms them from emulate_sums (before the rounding to fp32)"""
    s1, s2 = emulate_sums(x, width)
    n = x.shape[0] * x.shape[2] * x.shape[3]
    mean = s1 / n
    var = np.maximum(s2 / n - mean * mean, 0.0)
    return torch.from_numpy(mean), torch.from_numpy(var), torch.from_numpy(1.0 / np.sqrt(var + eps))
