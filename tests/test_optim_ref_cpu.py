"""tests/optim_ref.py pinned on the CPU: the float64 restatements against torch itself, a numpy fp32 emulation of the
kernels' operation sequences inside the derived bounds on every case of the shared table, and a list of mutations of that
emulation, each of which must leave a bound by a factor of 10 or more on some case: a bound no mutation can break would
check nothing."""
import math

import numpy as np
import pytest
import torch

from tests import optim_ref as R
from tests.optim_ref import worst

f32 = np.float32
N = 4099
MODES = (False, True)
MUTATIONS = ("decay_after_update", "bc2_without_sqrt", "eps_inside_sqrt", "grad_scale_dropped", "b1_for_complement",
             "bc1_omitted", "wd_for_lr_wd")


def emulate(p, g, m, v, lr, b1, b2, eps, wd, bc1, bc2, gs, exact, mutation=None):
    """adamw_kernel / adamw_c_kernel op by op in numpy fp32 (no contraction), with one of MUTATIONS applied"""
    lr, b2f, eps, wd, bc1f, gs = f32(lr), f32(b2), f32(eps), f32(wd), f32(bc1), f32(gs)
    one = f32(1.0)
    omb1, omb2 = (f32(1.0 - b1), f32(1.0 - b2)) if exact else (one - f32(b1), one - b2f)
    if mutation == "b1_for_complement":
        omb1 = f32(b1)
    q = np.sqrt(f32(bc2))
    if mutation == "bc2_without_sqrt":
        q = f32(bc2)
    step = lr if mutation == "bc1_omitted" else lr / bc1f
    d = one - (wd if mutation == "wd_for_lr_wd" else lr * wd)
    gv = g if mutation == "grad_scale_dropped" else g * gs
    pv = p if mutation == "decay_after_update" else p * d
    mv = m + (gv - m) * omb1
    vv = b2f * v + omb2 * gv * gv
    if mutation == "eps_inside_sqrt":
        denom = np.sqrt(vv + eps) / q
    else:
        denom = np.sqrt(vv) / q + eps
    pn = pv - step * (mv / denom)
    if mutation == "decay_after_update":
        pn = pn * d
    for a in (pn, mv, vv):
        assert a.dtype == f32
    return pn, mv, vv


# --------------------------------------------------- restatement vs torch ---
@pytest.mark.parametrize("ci", range(len(R.CASES)))
def test_adamw_step_is_torch_adamw_in_float64(ci):
    case = R.CASES[ci]
    r = np.random.default_rng(ci)
    p0 = case["p"] * r.standard_normal(257)
    grads = [case["g"] * r.standard_normal(257) for _ in range(5)]
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.AdamW([tp], lr=case["lr"], betas=case["betas"], eps=case["eps"], weight_decay=case["wd"])
    P, M, V = p0.copy(), np.zeros(257), np.zeros(257)
    b1, b2 = case["betas"]
    s = case["grad_scale"]
    for t, g in enumerate(grads, 1):
        tp.grad = torch.from_numpy(g * s)
        opt.step()
        P, M, V, *_ = R.adamw_step(P, g, M, V, case["lr"], b1, b2, case["eps"], case["wd"], 1 - b1 ** t, 1 - b2 ** t, s, True,
                                   round_scalars=False)
        st = opt.state[tp]
        assert np.max(np.abs(P - tp.detach().numpy())) <= 1e-13 * max(case["p"], case["lr"]) * 8
        assert np.max(np.abs(M - st["exp_avg"].numpy())) <= 1e-13 * case["g"] * 8
        assert np.max(np.abs(V - st["exp_avg_sq"].numpy())) <= 1e-13 * case["g"] ** 2 * 32


def _torch_clip(chunks, max_norm):
    ps = [torch.nn.Parameter(torch.zeros(len(c), dtype=torch.float64)) for c in chunks]
    for q, c in zip(ps, chunks):
        q.grad = torch.from_numpy(np.asarray(c, dtype=np.float64).copy())
    norm = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    return float(norm), [q.grad.numpy() for q in ps]


@pytest.mark.parametrize("name", ["above", "below", "equal", "zero", "inf", "nan"])
def test_clip_is_torch_clip_grad_norm(name):
    r = np.random.default_rng(3)
    chunks = [r.standard_normal(n) for n in (7, 130, 2)]
    max_norm = 1.0
    if name == "below":
        chunks = [1e-3 * c for c in chunks]
    elif name == "equal":
        chunks = [np.zeros(7), np.zeros(130), np.zeros(2)]
        chunks[0][3] = chunks[1][0] = chunks[1][129] = chunks[2][1] = 0.5
    elif name == "zero":
        chunks = [np.zeros_like(c) for c in chunks]
    elif name == "inf":
        chunks[1][5] = np.inf
    elif name == "nan":
        chunks[1][5] = np.nan
    coef, total = R.clip(chunks, max_norm)
    tnorm, tg = _torch_clip(chunks, max_norm)
    if name == "nan":
        assert math.isnan(coef) and math.isnan(total) and math.isnan(tnorm)
        assert all(np.all(np.isnan(g)) for g in tg)             # torch: every gradient turns NaN
        return
    if name == "inf":
        assert coef == 0.0 and total == np.inf and tnorm == np.inf
    else:
        assert abs(total - tnorm) <= 1e-15 * max(tnorm, 1.0)
    if name == "equal":
        assert total == 1.0 and coef == 1.0 / (1.0 + 1e-6)
    if name in ("below", "zero"):
        assert coef == 1.0
    if name == "zero":
        assert total == 0.0
    for c, g in zip(chunks, tg):
        with np.errstate(invalid="ignore"):
            want = c * coef
        assert np.allclose(want, g, rtol=1e-14, atol=0.0, equal_nan=True)
    # pre_scale multiplies the norm only
    c2, t2 = R.clip(chunks, max_norm, 0.25)
    assert (t2 == 0.25 * total) or name == "inf"


def test_adaptive_weight_is_the_reference_formula():
    for ss_rec, ss_disc, dw in [(4.0, 9.0, 0.5), (4.0, 0.0, 1.0), (1e12, 1e-12, 1.0), (0.0, 3.0, 0.7), (float("nan"), 1.0, 1.0),
                                (1.0, float("nan"), 1.0)]:
        want = torch.clamp(dw * (torch.tensor(ss_rec, dtype=torch.float64).sqrt()
                                 / (torch.tensor(ss_disc, dtype=torch.float64).sqrt() + 1e-4)), 0.0, 1e4)
        got = R.adaptive_weight(ss_rec, ss_disc, dw)
        if math.isnan(float(want)):
            assert math.isnan(got)
        else:
            assert got == pytest.approx(float(want), rel=1e-15)
    assert R.adaptive_weight(1e12, 1e-12, 1.0) == 1e4 and R.adaptive_weight(0.0, 3.0, 0.7) == 0.0


# ------------------------------------------- fp32 emulation vs the bounds ---
@pytest.mark.parametrize("exact", MODES)
@pytest.mark.parametrize("ci", range(len(R.CASES)))
def test_fp32_emulation_stays_inside_the_bounds(ci, exact):
    case = R.CASES[ci]
    args = R.case_args(case)
    for seed in range(3):
        p, g, m, v = R.case_state(case, N, 100 * ci + seed)
        P, M, V, bP, bM, bV = R.adamw_step(p, g, m, v, *args, exact)
        pn, mv, vv = emulate(p, g, m, v, *args, exact)
        rp, rm, rv = worst(pn, P, bP), worst(mv, M, bM), worst(vv, V, bV)
        print(f"optim_ref emu row {ci + 1} exact={int(exact)} seed {seed}: p {rp:.3f} m {rm:.3f} v {rv:.3f} of the bound")
        assert rp <= 1.0 and rm <= 1.0 and rv <= 1.0


def test_zero_gradient_row_is_the_decay_alone():
    case = R.CASES[4]
    assert case.get("zero")
    for c in R.CASES:   # the two ways the compiler may form 1 - lr wd agree on every row: the bitwise claim is unambiguous
        a, b = R.decay_factors(c["lr"], c["wd"])
        assert a == b
    p, g, m, v = R.case_state(case, N, 7)
    for exact in MODES:
        P, M, V, bP, bM, bV = R.adamw_step(p, g, m, v, *R.case_args(case), exact)
        want = p * f32(R.decay_factors(case["lr"], case["wd"])[0])
        assert want.dtype == f32
        assert np.array_equal(P.astype(f32), want) and not M.any() and not V.any() and not bM.any() and not bV.any()
        pn, mv, vv = emulate(p, g, m, v, *R.case_args(case), exact)
        assert np.array_equal(pn, want) and not mv.any() and not vv.any()


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_every_mutation_leaves_the_bound_by_a_factor_of_ten(mutation):
    best = 0.0
    for ci, case in enumerate(R.CASES):
        args = R.case_args(case)
        for exact in MODES:
            p, g, m, v = R.case_state(case, N, 100 * ci)
            P, M, V, bP, bM, bV = R.adamw_step(p, g, m, v, *args, exact)
            pn, mv, vv = emulate(p, g, m, v, *args, exact, mutation)
            best = max(best, worst(pn, P, bP), worst(mv, M, bM), worst(vv, V, bV))
    print(f"optim_ref mutation {mutation}: {best:.3g} of the bound")
    assert best >= 10.0


def test_flat_relative_bound_would_fail_where_m_cancels():
    """why the bound on p is not '1 ulp + k U |update|': on row 2 the fp32 emulation is off by far more than that on the
    elements where m + (G - m)(1 - b1) nearly cancels"""
    case = R.CASES[1]
    p, g, m, v = R.case_state(case, 1 << 16, 5)
    P, M, V, bP, *_ = R.adamw_step(p, g, m, v, *R.case_args(case), False)
    pn, *_ = emulate(p, g, m, v, *R.case_args(case), False)
    upd = np.abs(P - p.astype(np.float64) * R.kernel_scalars(*R.case_args(case), False)["d"])
    excess = np.abs(pn - P) - R.ulp32(np.maximum(np.abs(p), np.abs(P)))
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.max(np.where(excess > 0, excess / (R.U * upd), 0.0))
    assert k > 16.0, k
    assert worst(pn, P, bP) <= 1.0


@pytest.mark.parametrize("exact", MODES)
def test_iterated_bound_holds_fp32_steps_against_torch_float64(exact):
    case = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, wd=1e-2)
    r = np.random.default_rng(11)
    n = 2048
    p0 = r.standard_normal(n).astype(f32)
    grads = [r.standard_normal(n).astype(f32) for _ in range(3)]
    grads[1][:64] = 0.0
    s = 0.25
    tp = torch.nn.Parameter(torch.from_numpy(p0.astype(np.float64)))
    opt = torch.optim.AdamW([tp], lr=case["lr"], betas=case["betas"], eps=case["eps"], weight_decay=case["wd"])
    p, m, v = p0.copy(), np.zeros(n, f32), np.zeros(n, f32)
    b1, b2 = case["betas"]
    for t, g in enumerate(grads, 1):
        tp.grad = torch.from_numpy(g.astype(np.float64) * s)
        opt.step()
        p, m, v = emulate(p, g, m, v, case["lr"], b1, b2, case["eps"], case["wd"], 1 - b1 ** t, 1 - b2 ** t, s, exact)
    P, M, V, bP, bM, bV = R.adamw_iterate(p0, grads, case["lr"], case["betas"], case["eps"], case["wd"], s, exact)
    st = opt.state[tp]
    if exact:   # only then are the kernel's complements the rounded true ones, which scalar_err counts
        assert worst(p, tp.detach().numpy(), bP) <= 1.0
        assert worst(m, st["exp_avg"].numpy(), bM) <= 1.0
        assert worst(v, st["exp_avg_sq"].numpy(), bV) <= 1.0
    assert worst(p, P, bP) <= 1.0 and worst(m, M, bM) <= 1.0 and worst(v, V, bV) <= 1.0
    assert float(np.max(bP)) < 64 * R.U * 4.0   # three steps stay at rounding level


# ------------------------------------------------------------- reductions ---
def test_reduce_sum_bound_holds_quads_and_rejects_an_fp32_accumulator():
    r = np.random.default_rng(2)
    x = (1e3 + r.standard_normal((3, 7, 1156))).astype(f32)
    S, b = R.reduce_sum_bound(x.astype(np.float64), (0, 2), vector=True)
    q = x.reshape(3, 7, -1, 4)
    quads = ((q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3]))
    assert quads.dtype == f32
    got = quads.astype(np.float64).sum(axis=(0, 2)).astype(f32)
    assert worst(got, S, b) <= 1.0
    Ss, bs = R.reduce_sum_bound(x.astype(np.float64), (0, 2), vector=False)
    assert worst(x.astype(np.float64).sum(axis=(0, 2)).astype(f32), Ss, bs) <= 1.0
    assert np.all(bs <= 0.5 * R.ulp32(Ss) * 1.01)
    # the mutation: one sequential fp32 accumulator per channel, on a reduction long enough for it to drift
    x = (1e3 + r.standard_normal((24, 7, 1156))).astype(f32)
    S, b = R.reduce_sum_bound(x.astype(np.float64), (0, 2), vector=True)
    acc = np.cumsum(x.transpose(1, 0, 2).reshape(7, -1), axis=1, dtype=f32)[:, -1]
    print("reduce_sum fp32 sequential accumulator:", worst(acc, S, b), "of the vector bound")
    assert worst(acc, S, b) >= 10.0


def test_sigmoid_and_gelu_bounds_hold_the_fp32_formulas():
    x = np.concatenate([np.linspace(-30, 30, 20001), [88.0, -88.0, 104.0, -104.0, 0.0, -0.0]]).astype(f32)
    y, b = R.sigmoid_bound(x)
    with np.errstate(over="ignore"):
        got = f32(1.0) / (f32(1.0) + np.exp(-x))
        wrong = f32(1.0) / (f32(1.0) + np.exp(-x * f32(1.0 + 2e-6)))      # an exponent that is 17 U off
    assert got.dtype == f32 and worst(got, y, b) <= 1.0
    assert worst(wrong, y, b) >= 10.0
    u = np.linspace(-9, 9, 20001).astype(f32)
    ye, be = R.gelu_bounds(u)
    t = torch.nn.functional.gelu(torch.from_numpy(u).double()).numpy()
    assert np.max(np.abs(ye - t)) < 1e-14
    ue = torch.from_numpy(u).double().requires_grad_(True)
    torch.nn.functional.gelu(ue).backward(torch.full_like(ue, 0.7))
    ge, bg = R.gelu_bwd_bounds(np.full(u.shape, 0.7), u)
    assert np.max(np.abs(ge - ue.grad.numpy())) < 1e-14
    assert np.all(be <= R.GELU_ABS) and np.all(bg <= 0.7 * R.GELU_GRAD_ABS + R.U * 0.8)
