"""The BatchNorm2d chain of csrc/norm_act.hip — statistics, apply, backward — and every kernel that produces its sums, against
the float64 restatement of tests/bn_ref.py, through the C ABI.

Every bound is derived (bn_ref: a function of the inputs and of a count of fp32 roundings read from the kernel's code), every
kernel is fed the GPU's own fp32 statistics so that it is judged on its own arithmetic, and the inputs mix well and badly
conditioned channels (bn_ref.X_CLASSES) in one launch.  A later fusion that produces BatchNorm sums adds one line to
PRODUCERS; one that restates the backward hands its results to `check_backward`.

`_use` prints the largest fraction of its bound every check used (pytest -s); DESIGN.md ("BatchNorm chain against float64")
records them."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bn_ref as R

pytestmark = pytest.mark.gpu

U = R.U
EPS = float(np.float32(1e-5))       # eps and momentum reach the kernels as C floats
MOM = float(np.float32(0.1))
BF = torch.bfloat16
GENERIC_SHAPES, BF16_SHAPES = R.GENERIC_SHAPES, R.BF16_SHAPES


@pytest.fixture(scope="module")
def ops(dev):
    from weatherforecastingtoolkit_amd import ops as o
    return o


def _use(what, err, bound, names=None):
    """assert err <= bound element-wise; print the largest fraction of the bound in use"""
    err, bound = err.detach().double().cpu(), bound.detach().double().cpu().expand_as(err)
    frac = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = int(frac.argmax())
    where = np.unravel_index(worst, tuple(frac.shape)) if frac.dim() else ()
    tag = "" if names is None or frac.dim() == 0 else " " + names[where[1] if frac.dim() == 4 else where[0]]
    print("use %-28s %.3f%s" % (what, float(frac.max()), tag))
    assert float(frac.max()) <= 1.0 + R.FP64_SLACK, (what, float(frac.max()), where, tag, float(err.flatten()[worst]), float(bound.flatten()[worst]))
    return float(frac.max())


class Affine:
    """gamma, beta and non-trivial running statistics of C channels: CPU originals and device copies the kernels update"""

    def __init__(self, c, dev, seed=17):
        g = torch.Generator().manual_seed(seed)
        self.gamma = (torch.rand(c, generator=g) + 0.5).float()
        self.beta = torch.randn(c, generator=g).float()
        self.rm0 = torch.randn(c, generator=g).float()
        self.rv0 = (torch.rand(c, generator=g) + 0.5).float()
        self.g, self.b, self.rm, self.rv = (t.clone().to(dev) for t in (self.gamma, self.beta, self.rm0, self.rv0))

    @property
    def args(self):
        return self.g, self.b, self.rm, self.rv, EPS, MOM


def check_stats(y, st, aff, names=None, vector=True):
    """a BnStats and the updated running statistics against stats64 of the tensor actually stored; vector: the producer
    combines values in fp32 before fp64 (every one does, except the scalar paths of norm_act.hip)"""
    s = R.stats64(y.float(), aff.gamma, aff.beta, EPS, aff.rm0, aff.rv0, MOM)
    mean, invstd, scale, shift = (t.double().cpu() for t in (st.mean, st.invstd, st.scale, st.shift))
    k_sum, k_sq = R.sum_counts(y.float(), vector)
    dvar = R.var_bound(s, k_sum, k_sq)
    _use("mean", (mean - s.mean).abs(), R.mean_bound(s, k_sum), names)
    _use("invstd", (invstd / s.invstd - 1.0).abs(), R.invstd_rel_bound(s, EPS, dvar), names)
    # folded scale / shift on the GPU's own mean and invstd
    g, b = aff.gamma.double(), aff.beta.double()
    _use("scale", (scale - g * invstd).abs(), R.K_SCALE * U * (g * invstd).abs(), names)
    _use("shift", (shift - (b - mean * scale)).abs(), R.K_SHIFT * U * (b.abs() + (mean * scale).abs()), names)
    # running statistics: the mean from the GPU's own save_mean; the variance is not an output, so from var64 with its bound
    rm64 = (1.0 - MOM) * aff.rm0.double() + MOM * mean
    _use("running_mean", (aff.rm.double().cpu() - rm64).abs(), R.running_bound(MOM, aff.rm0, mean, torch.zeros_like(mean)), names)
    k = s.n / (s.n - 1.0)
    _use("running_var", (aff.rv.double().cpu() - s.running_var).abs(), R.running_bound(MOM, aff.rv0, s.var * k, dvar * k), names)
    return s


def ratios(y):
    s = R.stats64(y.float())
    return (s.mean.abs() / torch.sqrt(s.var).clamp_min(1e-300)).tolist()


def assert_offset_channels(y):
    """the tensor a convolution produced has a channel near 10 sigma and one near 100 sigma (measured in fp64)"""
    r = ratios(y)
    assert any(5 <= v <= 20 for v in r) and any(50 <= v <= 200 for v in r), sorted(r)[-6:]


# ------------------------------------------------------------------------------------------ 1. statistics: the producers
M_OVER_S = 25.0
ROW_RATIOS = (0.25, 10.0, 100.0, 1.0, None)        # per output channel, cyclically; None: a zero row (y = res or 0)
INNER_TAPS = torch.zeros(4, 4, dtype=torch.bool)
INNER_TAPS[1:3, 1:3] = True                         # the taps of a padded 4x4 stride-2 convolution every output pixel sees


def conv_weight(cout, cin, seed, taps=None, gain=1.0, ksize=1, m_over_s=M_OVER_S):
    """weights that put output channels of x = m + s N(0, 1) at the ROW_RATIOS (bn_ref.offset_rows)"""
    g = torch.Generator().manual_seed(seed)
    w = (torch.rand((cout, cin, ksize, ksize), generator=g) - 0.5) * 0.6
    plan = {r: ROW_RATIOS[r % len(ROW_RATIOS)] for r in range(cout)}
    w = R.offset_rows(w, {r: v * gain for r, v in plan.items() if v is not None}, m_over_s, taps)
    for r, v in plan.items():
        if v is None:
            w[r] = 0.0
    return w


def conv_input(shape, seed, prologue, dev, ops):
    """x = 2.5 + 0.1 N(0, 1); behind a BatchNorm + GELU prologue the same through scale 0.1 / shift 2.5 on N(0, 1), where
    gelu(u) is u to 1 %"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(shape, generator=g)
    if not prologue:
        return (2.5 + 0.1 * z).float(), None
    st = ops.BnStats(shape[1], dev)
    st.scale.fill_(0.1)
    st.shift.fill_(2.5)
    return z.float(), st


def residual(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.05 + 0.02 * torch.randn(shape, generator=g)).float()


def on_vector_path(x):
    """norm_act.hip takes 16-byte accesses (4 fp32 or 8 bf16 values, summed in fp32 four at a time) when HW allows"""
    return (x.shape[2] * x.shape[3]) % (8 if x.dtype == BF else 4) == 0


def p_stats_train(ops, dev, case):
    shape, dtype = case
    x, names = R.mixed(shape, 31, R.classes_for(shape[1]))
    x = x.to(dtype).to(dev)
    aff = Affine(shape[1], dev)
    return x, ops.bn_stats_train(x, *aff.args), aff, names, on_vector_path(x)


def p_act_fwd_stats(ops, dev, case):
    """wfae_bn_act_fwd_stats(_bf16) + wfae_bn_stats_from_parts: identity scale / shift keep the channel classes through the
    pass (GELU and LeakyReLU bend the benign ones)"""
    shape, dtype, act = case
    x, names = R.mixed(shape, 32, R.classes_for(shape[1]))
    x = x.to(dtype).to(dev)
    st_in = ops.BnStats(shape[1], dev)
    st_in.scale.fill_(1.0)
    st_in.shift.fill_(0.0)
    y, sp = ops.bn_act_fwd_stats(x, st_in, act)
    assert torch.equal(y, ops.bn_act_fwd(x, st_in, act))
    aff = Affine(shape[1], dev)
    return y, ops.bn_stats_from_parts(sp, shape, *aff.args), aff, names, on_vector_path(x)


def _conv1x1(ops, dev, nb, cin, cout, h, w, res, prologue, c1r, served=True):
    x, st_in = conv_input((nb, cin, h, w), 33, prologue, dev, ops)
    x = x.to(dev)
    wt = conv_weight(cout, cin, 34).to(dev)
    r = residual((nb, cout, h, w), 35).to(dev) if res else None
    fn = (lambda: ops.conv1x1_fwd_bnact(x, st_in, wt, None, r, stats=True)) if prologue else (lambda: ops.conv1x1_fwd_stats(x, wt, None, r))
    ops.set_c1r(False)
    try:
        y_gemm, sr_gemm = fn()
    finally:
        ops.set_c1r(True)
    if c1r:     # the route, as tests/test_c1r_gpu.py asserts it
        assert ops.c1r_supported(cout, cin, h * w)
        y, sr = fn()
        assert not torch.equal(y, y_gemm), "c1r did not run (same bits as gemm.hip)"
    else:
        y, sr = y_gemm, sr_gemm
    assert (sr is not None) == served, "the epilogue serves this shape: %s" % served
    assert_offset_channels(y)
    aff = Affine(cout, dev)
    if sr is None:      # the contract of conv1x1_fwd_stats: no rows, y complete, the caller runs the statistics pass
        return y, ops.bn_stats_train(y, *aff.args), aff, None, on_vector_path(y)
    return y, ops.bn_stats_from_rows(sr, tuple(y.shape), *aff.args), aff, None, True


def p_conv1x1_gemm(ops, dev, case):
    return _conv1x1(ops, dev, *case[:7], c1r=False, served=case[7])


def p_conv1x1_c1r(ops, dev, case):
    return _conv1x1(ops, dev, *case, c1r=True)


def p_wino(ops, dev, case):
    """wino_down(stats=True) = wfae_wino_out_stats / _bf16 and wino_up(stats=True) = wfae_wino_in_t_stats / _bf16, with the
    sum-reducing kernels on whatever the tile count"""
    mode, up, nb, chi, clo, hlo, wlo, dtype = case
    keep, ops.WINO_STATS_MIN_TILES = ops.WINO_STATS_MIN_TILES, 0
    ops.set_winograd(mode)
    try:
        pl = ops.wino_plan(nb, chi, clo, hlo, wlo)
        assert pl is not None and pl.variant == (1 if mode == "f42" else 0)
        g = torch.Generator().manual_seed(36)
        if up:      # ConvTranspose2d: output channels are dim 1 of the weight; a pixel sees 4 of the 16 taps, one of them interior:
            # half the planned ratio, and a fan-in of 4 Clo that reaches 100 sigma only from a narrower input (m / s = 100)
            wt = conv_weight(chi, clo, 37, INNER_TAPS, gain=2.0, ksize=4, m_over_s=100.0).transpose(0, 1).contiguous().to(dev)
            lo = (2.5 + 0.025 * torch.randn((nb, clo, hlo, wlo), generator=g)).float().to(dev)
            y, sp = ops.wino_up(ops.wino_weights(wt, pl), ops.wino_out_t(lo, pl), pl, stats=True, out_dtype=dtype)
        else:
            wt = conv_weight(clo, chi, 37, INNER_TAPS, ksize=4).to(dev)
            hi = (2.5 + 0.1 * torch.randn((nb, chi, 2 * hlo, 2 * wlo), generator=g)).float().to(dev)
            y, sp = ops.wino_down(ops.wino_weights(wt, pl), ops.wino_in(hi, pl), pl, stats=True, out_dtype=dtype)
    finally:
        ops.set_winograd("auto")
        ops.WINO_STATS_MIN_TILES = keep
    assert sp is not None and y.dtype == dtype
    assert_offset_channels(y)
    aff = Affine(y.shape[1], dev)
    return y, ops.bn_stats_from_parts(sp, tuple(y.shape), *aff.args), aff, None, True


def p_medium(ops, dev, case):
    """the bf16-storage 1x1 forms at 'medium' precision: csrc/c1b.hip, csrc/c1rb.hip and gemm.hip's element-typed kernel
    behind wfae_conv1x1_fwd_bf16; precision and storage restored whatever happens"""
    import weatherforecastingtoolkit_amd as pkg
    kind, nb, cin, cout, h, w, res, prologue = case
    pkg.set_float32_matmul_precision("medium")
    try:
        x, st_in = conv_input((nb, cin, h, w), 38, prologue, dev, ops)
        x = x.bfloat16().to(dev)
        wt = conv_weight(cout, cin, 39).to(dev)
        r = residual((nb, cout, h, w), 40).bfloat16().to(dev) if res else None
        if kind == "c1b":
            assert ops.c1b_supported(cout, cin, h * w)
            y, sr = ops.c1b_fwd(ops.c1b_weights(wt)[0], x, st_in, r, True)
        elif kind == "c1rb":
            assert ops.c1rb_supported(cout, cin, h * w)
            y, sr = ops.c1rb_fwd(wt, False, x, st_in, r, True)
        elif prologue:
            y, sr = ops.conv1x1_fwd_bnact(x, st_in, wt, None, r, stats=True)
        else:
            y, sr = ops.conv1x1_fwd_stats(x, wt, None, r)
        assert sr is not None and y.dtype == BF
        aff = Affine(cout, dev)
        st = ops.bn_stats_from_rows(sr, tuple(y.shape), *aff.args)
    finally:
        pkg.set_float32_matmul_precision("highest")
        ops.set_activation_storage(torch.float32)
    assert_offset_channels(y)
    return y, st, aff, None, True


class Producer:
    def __init__(self, name, fn, cases):
        self.name, self.fn, self.cases = name, fn, cases


F32 = torch.float32
C1R_MK = [(128, 32), (32, 128), (256, 64), (512, 128)]
PRODUCERS = [
    Producer("bn_stats_train", p_stats_train, [(s, F32) for s in GENERIC_SHAPES]),
    Producer("bn_stats_train_bf16", p_stats_train, [(s, BF) for s in BF16_SHAPES]),
    Producer("bn_act_fwd_stats", p_act_fwd_stats, [(s, dt, act) for s in GENERIC_SHAPES for dt in (F32, BF) for act in R.ACTS]),
    # (nb, cin, cout, h, w, res, prologue, served): wfae_conv1x1_fwd_stats and wfae_conv1x1_fwd_bnact(stats) on gemm.hip.  Its
    # epilogue takes the sums only in the kernels with two wave columns (conv1x1_fwd_impl: pick_bm(M, tiles) != 32, i.e.
    # cdiv(Cout, 64) * cdiv(NB * HW, 128) >= 512): the three small shapes report no rows and fall back to the statistics pass,
    # the three large ones are the smallest that reach the 64-row kernel (twice) and the 128-row kernel
    Producer("conv1x1_gemm", p_conv1x1_gemm, [(nb, ci, co, h, w, res, pro, served)
                                              for nb, ci, co, h, w, served in ((2, 32, 128, 16, 16, False), (3, 64, 256, 12, 12, False),
                                                                               (5, 128, 32, 16, 8, False), (4, 32, 1024, 32, 32, True),
                                                                               (4, 64, 256, 64, 64, True), (4, 64, 512, 64, 64, True))
                                              for res in (False, True) for pro in (False, True)]),
    # the same two on csrc/c1r.hip (wfae_c1r_fwd); the residual belongs to the widening products
    Producer("conv1x1_c1r", p_conv1x1_c1r, [(nb, k, m, h, w, res, pro) for m, k in C1R_MK for nb, h, w in ((1, 8, 8), (3, 16, 20))
                                            for res in ((False, True) if m > k else (False,)) for pro in (False, True)]),
    # (mode, up, nb, chi, clo, hlo, wlo, dtype): square and Hlo != Wlo, fewer and more than 256 tiles per image
    Producer("wino", p_wino, [(mode, up, *geo, dt) for mode, geos in (("f22", ((2, 16, 16, 8, 12), (1, 16, 16, 36, 36))),
                                                                      ("f42", ((2, 16, 16, 8, 8), (1, 16, 16, 64, 72))))
                              for geo in geos for up in (False, True) for dt in (F32, BF)]),
    # (kind, nb, cin, cout, h, w, res, prologue): the smallest shapes these kernels serve
    Producer("medium", p_medium, [("c1b", 5, 32, 64, 4, 6, True, False), ("c1b", 5, 32, 64, 4, 6, False, True),
                                  ("c1rb", 1, 32, 128, 8, 16, True, False), ("c1rb", 1, 32, 128, 8, 16, True, True),
                                  ("gemm", 4, 64, 256, 64, 64, True, False), ("gemm", 4, 64, 256, 64, 64, False, True)]),
]


def _case_id(v):
    if isinstance(v, torch.dtype):
        return "bf16" if v == BF else "f32"
    if isinstance(v, tuple):
        return "x".join(_case_id(e) for e in v)
    return str(v)


@pytest.mark.parametrize("producer,case", [pytest.param(p, c, id=p.name + "-" + _case_id(c)) for p in PRODUCERS for c in p.cases])
def test_batchnorm_sums_of_every_producer_match_float64(ops, dev, producer, case):
    y, st, aff, names, vector = producer.fn(ops, dev, case)
    check_stats(y, st, aff, names, vector)


# ------------------------------------------------------------------------------------------------------------- 2. apply
K_FOLD = 3      # bn_fold_eval_kernel: `1.0f / sqrtf(rv[c] + eps)` — the sum, the root, the quotient


def eval_stats(ops, dev, aff):
    st = ops.bn_fold_eval(aff.g, aff.b, aff.rm, aff.rv, EPS)
    mean, invstd, scale, shift = R.fold_eval64(aff.gamma, aff.beta, aff.rm0, aff.rv0, EPS)
    assert torch.equal(st.mean.cpu(), aff.rm0)
    _use("fold invstd", (st.invstd.double().cpu() / invstd - 1.0).abs(), torch.full_like(invstd, K_FOLD * U))
    gi = aff.gamma.double() * st.invstd.double().cpu()
    _use("fold scale", (st.scale.double().cpu() - gi).abs(), R.K_SCALE * U * gi.abs())
    sh = aff.beta.double() - aff.rm0.double() * st.scale.double().cpu()
    _use("fold shift", (st.shift.double().cpu() - sh).abs(), R.K_SHIFT * U * (aff.beta.double().abs() + (aff.rm0.double() * st.scale.double().cpu()).abs()))
    return st


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("shape,dtype", [(s, F32) for s in GENERIC_SHAPES] + [(s, BF) for s in sorted(set(GENERIC_SHAPES + BF16_SHAPES))])
def test_apply_matches_float64_on_the_gpus_own_scale_and_shift(ops, dev, shape, dtype, training):
    """wfae_bn_act_fwd(_bf16), act 0 / 1 / 2, on training and wfae_bn_fold_eval statistics: per element within one fma rounding
    through the activation plus the activation's own error; bf16 results are the correctly rounded float64 value"""
    x, names = R.mixed(shape, 41, R.classes_for(shape[1]))
    x = x.to(dtype).to(dev)
    aff = Affine(shape[1], dev)
    st = ops.bn_stats_train(x, *aff.args) if training else eval_stats(ops, dev, aff)
    for act in R.ACTS:
        y = ops.bn_act_fwd(x, st, act)
        assert y.dtype == dtype
        ref = R.apply64(x.float(), st.scale, st.shift, act)
        bound = R.apply_bound(x.float(), st.scale, st.shift, act)
        if dtype == BF:
            assert R.bf16_mismatch(y, ref, bound) == 0, (act, R.bf16_offenders(y, ref, bound))
        else:
            _use("y act %d" % act, (y.double().cpu() - ref).abs(), bound, names)


# ---------------------------------------------------------------------------------------------------------- 3. backward
def coef_of(ops, c):
    """the two fp32 sums per channel at the head of this stream's workspace, where the dx pass reads them"""
    return ops.workspace()[:8 * c].view(torch.float32).view(c, 2).clone().t().contiguous().cpu()


def check_backward(what, dy, x, res, aff, st, act, training, got, dg0=None, names=None, sums=None):
    """got = (dx, dgamma, dbeta, coef (2, C)); references on the GPU's own statistics and coefficients; sums: fp64 totals of a
    producer's partial rows, checked without the final rounding"""
    dx, dg, db, coef = got
    stat = (st.scale, st.shift, st.mean, st.invstd)
    f = [t.float() for t in (dy, x)]
    s1, s2 = R.bwd_sums64(*f, *stat, act)
    b1, b2 = R.bwd_sums_bound(*f, *stat, act)
    if sums is not None:
        p1, p2 = R.bwd_sums_bound(*f, *stat, act, finals=0)
        _use(what + " rows dU", (sums[0].double().cpu() - s1).abs(), p1, names)
        _use(what + " rows dU xhat", (sums[1].double().cpu() - s2).abs(), p2, names)
    _use(what + " coef dU", (coef[0].double() - s1).abs(), b1, names)
    _use(what + " coef dU xhat", (coef[1].double() - s2).abs(), b2, names)
    if dg0 is None:
        _use(what + " dbeta", (db.double().cpu() - s1).abs(), b1, names)
        _use(what + " dgamma", (dg.double().cpu() - s2).abs(), b2, names)
    else:
        a1, a2 = R.bwd_sums_bound(*f, *stat, act, accumulate_into=dg0)
        _use(what + " dbeta+=", (db.double().cpu() - (dg0[1].double() + s1)).abs(), a1, names)
        _use(what + " dgamma+=", (dg.double().cpu() - (dg0[0].double() + s2)).abs(), a2, names)
    r = None if res is None else res.float()
    ref = R.bwd_dx64(*f, aff.gamma, *stat, act, training, coef=coef, res=r)
    bound = R.dx_bound(*f, aff.gamma, *stat, act, training, coef=coef, res=r)
    if dx.dtype == BF:
        assert R.bf16_mismatch(dx, ref, bound) == 0, (what, R.bf16_offenders(dx, ref, bound))
    else:
        _use(what + " dx", (dx.double().cpu() - ref).abs(), bound, names)
    return ref, bound


def run_bn_act_bwd(ops, dev, dy, x, res, aff, st, act, training, accumulate):
    c = x.shape[1]
    g = torch.Generator().manual_seed(43)
    dg0 = (torch.randn(c, generator=g).float(), torch.randn(c, generator=g).float()) if accumulate else None
    dg, db = (dg0[0].clone().to(dev), dg0[1].clone().to(dev)) if accumulate else (torch.empty(c, device=dev), torch.empty(c, device=dev))
    dx = ops.bn_act_bwd(dy, x, aff.g, st, dg, db, res, act, training, accumulate)
    return (dx, dg, db, coef_of(ops, c)), dg0


@pytest.mark.parametrize("act", [1, 2])
@pytest.mark.parametrize("kind", R.DY_CLASSES)
@pytest.mark.parametrize("shape,dtype", [(s, F32) for s in GENERIC_SHAPES] + [(s, BF) for s in BF16_SHAPES])
def test_backward_sums_and_dx_match_float64(ops, dev, shape, dtype, kind, act):
    """wfae_bn_act_bwd(_bf16) in one call (phases 3) and as phase 1 + phase 2, training and eval, with and without `res`, with
    dgamma / dbeta accumulated into non-zero buffers: the sums (coef), dgamma / dbeta and dx.  Every cotangent class meets every
    channel class; among them the cancelling gradient on the 100-sigma channel and the constant channel, whose xhat is 0"""
    x, names = R.mixed(shape, 44, R.classes_for(shape[1]))
    x = x.to(dtype).to(dev)
    dy = R.grad(shape, kind, 45).to(dtype).to(dev)
    res = R.grad(shape, "uniform", 46).to(dtype).to(dev)
    aff = Affine(shape[1], dev)
    for training in (True, False):
        st = ops.bn_stats_train(x, *aff.args) if training else ops.bn_fold_eval(aff.g, aff.b, aff.rm, aff.rv, EPS)
        for r, accumulate in ((None, False), (res, True)):
            what = "%s%s" % ("train" if training else "eval", "+res" if r is not None else "")
            got, dg0 = run_bn_act_bwd(ops, dev, dy, x, r, aff, st, act, training, accumulate)
            check_backward(what, dy, x, r, aff, st, act, training, got, dg0, names)
            if dtype == F32:        # phase 1, then phase 2 alone: the same bits
                dg, db = torch.empty(shape[1], device=dev), torch.empty(shape[1], device=dev)
                assert ops.bn_act_bwd(dy, x, aff.g, st, dg, db, r, act, training, need_dx=False) is None
                assert torch.equal(coef_of(ops, shape[1]), got[3])
                assert torch.equal(ops.bn_act_bwd_dx(dy, x, aff.g, st, r, act, training), got[0])
                if not accumulate:
                    assert torch.equal(dg, got[1]) and torch.equal(db, got[2])


@pytest.mark.parametrize("shape", GENERIC_SHAPES)
def test_constant_gradient_gives_zero_dx_in_training_mode(ops, dev, shape):
    """a channel whose dU is exactly constant (LeakyReLU with every pre-activation positive, a constant cotangent): the float64
    dx of training mode is 0, and |dx| of the kernel must lie within the per-element bound evaluated at those inputs — an
    absolute bound, there is nothing to be relative to.  The kernel works on its own fp32 statistics and sums, so the bound
    on |dx| is that of the dx expression plus what those inputs are allowed: the two sums may be off by bwd_sums_bound, and
    the saved mean by mean_bound, which leaves sum dU xhat = c n (mean64 - mean) invstd instead of 0"""
    x, names = R.mixed(shape, 47, R.classes_for(shape[1]))
    c = shape[1]
    aff = Affine(c, dev)
    aff.beta = torch.full((c,), 8.0)
    aff.b = aff.beta.to(dev)
    dy = (torch.arange(1, c + 1).float() * 0.3).view(1, c, 1, 1).expand(shape).contiguous()
    x, dy = x.to(dev), dy.to(dev)
    st = ops.bn_stats_train(x, *aff.args)
    u, du, _ = R.bwd_terms64(dy, x, st.scale, st.shift, st.mean, st.invstd, 2)
    assert float(u.min()) > 0 and torch.equal(du, dy.double().cpu())
    s = R.stats64(x, aff.gamma, aff.beta, EPS)
    exact = R.bwd_dx64(dy, x, aff.gamma, s.scale, s.shift, s.mean, s.invstd, 2, True)
    assert float(exact.abs().max()) <= R.FP64_SLACK * float(dy.max())      # 0 to the rounding of float64
    got, _ = run_bn_act_bwd(ops, dev, dy, x, None, aff, st, 2, True, False)
    ref, bound = check_backward("constant", dy, x, None, aff, st, 2, True, got, None, names)
    n = x.numel() // c
    stat = (st.scale, st.shift, st.mean, st.invstd)
    b1, b2 = R.bwd_sums_bound(dy, x, *stat, 2)
    _, _, xh = R.bwd_terms64(dy, x, *stat, 2)
    pc = lambda v: v.double().cpu().view(1, -1, 1, 1)
    gi = (pc(aff.gamma) * pc(st.invstd)).abs()
    dmean = R.mean_bound(s, R.sum_counts(x, on_vector_path(x))[0])
    slack = gi * (pc(b1) / n + xh.abs() * (pc(b2) / n + pc(dy[0, :, 0, 0]) * pc(dmean) * pc(st.invstd)))
    _use("constant |dx|", got[0].double().cpu().abs(), bound + slack, names)


@pytest.mark.parametrize("m,k", [(128, 32), (256, 64)])
@pytest.mark.parametrize("nb,h,w", [(2, 8, 8), (5, 16, 24)])
@pytest.mark.parametrize("kind", R.DY_CLASSES)
def test_fused_backward_forms_match_float64(ops, dev, m, k, nb, h, w, kind):
    """wfae_c1r_bnred (store and no-store) + wfae_bn_act_bwd_from_rows + phase 2, and wfae_c1r_bndx: the cotangent dA of the
    BatchNorm is the data gradient the kernels form themselves; the stored one (bit-identical to wfae_conv1x1_bwd_data) is
    what the float64 references are evaluated on"""
    assert ops.c1r_bnred_supported(m, k, h * w)
    shape = (nb, m, h, w)
    x, names = R.mixed(shape, 48)
    x = x.to(dev)
    # dA = W^T dT: an identity block in W hands the chosen cotangent class through to the first k channels of dA
    dt = R.grad((nb, k, h, w), kind, 49).to(dev)
    g = torch.Generator().manual_seed(50)
    wt = ((torch.rand((k, m, 1, 1), generator=g) - 0.5) * 0.6).float()
    wt[:, :k] = torch.eye(k).view(k, k, 1, 1)
    wt = wt.to(dev)
    res = R.grad(shape, "uniform", 51).to(dev)
    aff = Affine(m, dev)
    for training in (True, False):
        st = ops.bn_stats_train(x, *aff.args) if training else ops.bn_fold_eval(aff.g, aff.b, aff.rm, aff.rv, EPS)
        da, sr = ops.c1r_bnred(wt, dt, x, st)
        assert torch.equal(da, ops.conv1x1_bwd_data(dt, wt))
        none, sr2 = ops.c1r_bnred(wt, dt, x, st, store=False)
        assert none is None and sr2.rows == sr.rows and torch.equal(sr2.part, sr.part)
        sums = sr.part.view(2, sr.rows, m).sum(dim=1)
        for r, accumulate in ((None, False), (res, True)):
            gq = torch.Generator().manual_seed(52)
            dg0 = (torch.randn(m, generator=gq).float(), torch.randn(m, generator=gq).float()) if accumulate else None
            dg, db = (dg0[0].clone().to(dev), dg0[1].clone().to(dev)) if accumulate else (torch.empty(m, device=dev), torch.empty(m, device=dev))
            ops.bn_act_bwd_from_rows(sr2, m, dg, db, accumulate)
            coef = coef_of(ops, m)
            what = "%s%s" % ("train" if training else "eval", "+res" if r is not None else "")
            dx = ops.bn_act_bwd_dx(da, x, aff.g, st, r, 1, training)
            check_backward("rows " + what, da, x, r, aff, st, 1, training, (dx, dg, db, coef), dg0, names, sums)
            assert torch.equal(coef_of(ops, m), coef)
            dx2 = ops.c1r_bndx(wt, dt, x, aff.g, st, r, training)
            check_backward("bndx " + what, da, x, r, aff, st, 1, training, (dx2, dg, db, coef), dg0, names)


# -------------------------------------------------------------------------------------------------------- 4. end to end
def chain_errors(ops, dev, x, dy, aff, act):
    """errors against torch float64 autograd of (a) the kernels' chain bn_stats_train -> bn_act_fwd -> bn_act_bwd and (b)
    torch's fp32 CPU BatchNorm chain on the same tensors: {quantity: (kernel, torch fp32, max |ref|)}"""
    def torch_chain(dt):
        xx = x.detach().clone().to(dt).requires_grad_(True)
        g, b = aff.gamma.to(dt).requires_grad_(True), aff.beta.to(dt).requires_grad_(True)
        rm, rv = aff.rm0.to(dt).clone(), aff.rv0.to(dt).clone()
        u = F.batch_norm(xx, rm, rv, g, b, True, MOM, EPS)
        y = F.gelu(u) if act == 1 else F.leaky_relu(u, 0.2) if act == 2 else u
        y.backward(dy.to(dt))
        _, _, invstd = torch.native_batch_norm(x.to(dt), None, None, None, None, True, MOM, EPS)
        return {"y": y.detach(), "dx": xx.grad, "dgamma": g.grad, "dbeta": b.grad, "invstd": invstd}
    ref, t32 = torch_chain(torch.float64), torch_chain(torch.float32)
    xd, dyd = x.to(dev), dy.to(dev)
    st = ops.bn_stats_train(xd, *aff.args)
    dg, db = torch.empty(x.shape[1], device=dev), torch.empty(x.shape[1], device=dev)
    got = {"y": ops.bn_act_fwd(xd, st, act), "dx": ops.bn_act_bwd(dyd, xd, aff.g, st, dg, db, None, act, True), "dgamma": dg, "dbeta": db,
           "invstd": st.invstd}
    return {q: (float((got[q].double().cpu() - ref[q]).abs().max()), float((t32[q].double() - ref[q]).abs().max()),
                float(ref[q].abs().max())) for q in ref}


def assert_within_4x_torch_fp32(errs, quantities, what):
    """error <= 4 x the error of torch's fp32 CPU BatchNorm on the same tensors against the same float64 (two fp32 evaluations
    that differ in summation order), floor 4 U max |ref|.  torch fp32 is the measure, never the kernel under test"""
    bad = []
    for q in quantities:
        e, t, m = errs[q]
        print("e2e %-20s %-7s kernel %.2e torch fp32 %.2e ratio %.2f bar %.2e" % (what, q, e, t, e / max(t, 1e-300), 4 * t + 4 * U * m))
        if e > 4 * t + 4 * U * m:
            bad.append((q, e, t))
    assert not bad, (what, bad)


@pytest.mark.parametrize("act", [1, 2])
@pytest.mark.parametrize("shape", GENERIC_SHAPES)
def test_chain_tracks_float64_like_torch_fp32(ops, dev, shape, act):
    x, _ = R.mixed(shape, 53, ("benign", "sparse"))
    aff = Affine(shape[1], dev)
    errs = chain_errors(ops, dev, x, R.grad(shape, "uniform", 54), aff, act)
    assert_within_4x_torch_fp32(errs, ("y", "dx", "dgamma", "dbeta"), "%s act %d" % (shape, act))


# ------------------------------------------------------------------------------------------------ 5. the known limit
@pytest.mark.xfail(strict=True, raises=AssertionError, reason="var = S2 / n - mean^2 in bn_finalize_kernel and bn_finalize_parts_kernel: the squares are rounded to "
                   "fp32 before they are summed, and at a mean of 100 sigma the subtraction leaves 1e-4 of their rounding in the variance")
@pytest.mark.parametrize("shape", [(3, 8, 12, 12), (2, 3, 96, 96)])
def test_batchnorm_statistics_under_a_100_sigma_offset_match_fp32_reference(ops, dev, shape):
    """the known limit (open item "BatchNorm variance by cancellation"): bn_stats_train + bn_act_fwd on a tensor whose
    every channel sits at 100 sigma, held to the bar of the end-to-end test.  Measured on an MI355X: invstd off by 4.1e-5 and
    6.4e-6 relative (torch fp32: 5.2e-8 and 3.1e-8), y by 1.9e-4 and 2.6e-5 (torch fp32: 7.1e-6 and 9.1e-6).  A variance from
    sums of deviations from a per-channel pivot has to reach every producer epilogue of PRODUCERS; when it does, this test passes
    and the mark has to go"""
    x, _ = R.mixed(shape, 55, ("offset100",))
    aff = Affine(shape[1], dev)
    errs = chain_errors(ops, dev, x, R.grad(shape, "uniform", 56), aff, 0)
    assert_within_4x_torch_fp32(errs, ("invstd", "y"), "offset100 %s" % (shape,))
