"""GPU: the optimiser step (wfae_adamw / wfae_adamw_c, FusedAdamW.step over a mixed arena), the clipping chain
(wfae_sumsq -> wfae_clip_coef -> wfae_scale through FusedAdamW.clip_grad_norm_) and wfae_adaptive_weight against the float64
restatements of tests/optim_ref.py, per element, within its derived bounds.  Every case prints
`optim_fp64 <kernel> <case> <largest error as a fraction of its bound>` (profiles/optim_glue_fp64_errors.txt is that
output)."""
import math

import numpy as np
import pytest
import torch

from tests import optim_ref as R
from tests.optim_ref import bits, report, worst

pytestmark = pytest.mark.gpu

f32 = np.float32
SENTINEL = 123.0


@pytest.fixture(scope="module")
def ops(dev):
    from weatherforecastingtoolkit_amd import ops as o
    return o


def placed(arr, dev, offset):
    """the array on the device inside a buffer with a sentinel on either side: the view starts `offset` elements in"""
    n = len(arr)
    buf = torch.full((n + offset + 1,), SENTINEL, device=dev)
    view = buf[offset:offset + n]
    view.copy_(torch.from_numpy(arr))
    return buf, view


def untouched_outside(buf, offset, n):
    return bool((buf[:offset] == SENTINEL).all()) and bool((buf[offset + n:] == SENTINEL).all())


# ------------------------------------------------ the two AdamW kernels ---
@pytest.mark.parametrize("exact", [False, True], ids=["fp32_complements", "exact_complements"])
@pytest.mark.parametrize("ci", range(len(R.CASES)), ids=[f"row{i + 1}" for i in range(len(R.CASES))])
def test_adamw_kernels_per_element(ops, dev, ci, exact):
    """one step from identical fp32 state: p, m and v of the kernel inside the bounds of optim_ref.adamw_step at every
    size (one element, around one block, several blocks, past the 4096-block cap) and from views that start one element
    into their buffers; the zero-gradient row gives the bits of fl(p fl(1 - lr wd))"""
    case = R.CASES[ci]
    args = R.case_args(case)
    for n in R.SIZES:
        p, g, m, v = R.case_state(case, n, 1000 * ci + n % 997)
        P, M, V, bP, bM, bV = R.adamw_step(p, g, m, v, *args, exact)
        for offset in (0, 1):
            bufs, views = zip(*(placed(a, dev, offset) for a in (p, g, m, v)))
            ops.adamw_(*views, *args, exact)
            torch.cuda.synchronize()
            pn, gn, mn, vn = (t.cpu().numpy() for t in views)
            assert all(untouched_outside(b, offset, n) for b in bufs), "a write outside the n elements"
            assert np.array_equal(bits(gn), bits(g)), "the gradient was written"
            if case.get("zero"):
                assert np.array_equal(bits(pn), bits(P.astype(f32))) and not mn.any() and not vn.any()
                ratios = (0.0, 0.0, 0.0)
            else:
                ratios = (worst(pn, P, bP), worst(mn, M, bM), worst(vn, V, bV))
            report("adamw_c" if exact else "adamw", f"row{ci + 1} n={n} offset={offset}  p m v", *ratios)
            assert max(ratios) <= 1.0, (n, offset, ratios)


# --------------------------------------------------------- mixed arena ---
SHAPES = [(7,), (1,), (64, 33), (5,), (3, 3, 3, 5), (130,), (2,)]
NONE_IDX, STRAY_IDX, COLUMN_IDX = 1, 3, 6   # no gradient; stray contiguous; stray (contiguous, or a strided column)
HYPER = dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.1)


def make_arena(dev, seed, **kw):
    from weatherforecastingtoolkit_amd.optim import FusedAdamW
    g = torch.Generator().manual_seed(seed)
    init = [torch.randn(s, generator=g) for s in SHAPES]
    ps = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    opt = FusedAdamW(ps, exact_complements=True, **HYPER, **kw)
    return init, ps, opt


def set_grads(ps, grads, dev, strided_column):
    """gradient states, in order: in-arena, none, in-arena, stray contiguous, in-arena, in-arena, stray (a column of a
    2 x 2 matrix, stride 2, when strided_column)"""
    for i, (p, g) in enumerate(zip(ps, grads)):
        if i == NONE_IDX:
            p.grad = None
        elif i == STRAY_IDX:
            p.grad = g.clone().to(dev)
        elif i == COLUMN_IDX:
            if strided_column:
                sq = torch.zeros(2, 2, device=dev)
                sq[:, 0] = g.to(dev)
                p.grad = sq[:, 0]
                assert not p.grad.is_contiguous()
            else:
                p.grad = g.clone().to(dev)
        else:
            p._wfae_grad_view.copy_(g.to(dev))
            p.grad = p._wfae_grad_view


def padding_mask(arena):
    mask = torch.ones(arena.numel, dtype=torch.bool)
    for p, o in zip(arena.params, arena.offsets):
        mask[o:o + p.numel()] = False
    return mask


def test_fused_adamw_mixed_arena(ops, dev):
    """FusedAdamW.step over in-arena, missing and stray gradients (one of them strided) for 3 steps against
    torch.optim.AdamW in float64 on the same gradients, within optim_ref.adamw_iterate; the parameter without a gradient is
    not touched (no decay, as in torch), the arena's padding stays zero, and a step is one launch per run and per stray"""
    init, ps, opt = make_arena(dev, 0)
    opt.grad_scale = 0.5
    arena = opt.arenas[0]
    gen = torch.Generator().manual_seed(1)
    steps = [[torch.randn(s, generator=gen) * (0.3 + k) for s in SHAPES] for k in range(3)]
    ref = [torch.nn.Parameter(t.double().clone()) for t in init]
    ropt = torch.optim.AdamW(ref, **HYPER)
    for k, grads in enumerate(steps):
        set_grads(ps, grads, dev, strided_column=True)
        runs, stray = arena.runs()
        o = arena.offsets
        assert runs == [(o[0], o[0] + 7), (o[2], o[2] + 64 * 33), (o[4], o[5] + 130)] and stray == [STRAY_IDX, COLUMN_IDX]
        for i, (q, g) in enumerate(zip(ref, grads)):
            q.grad = None if i == NONE_IDX else g.double() * 0.5
        ropt.step()
        ops.profile_start()
        opt.step()
        prof = ops.profile_stop()
        assert prof["wfae_adamw"][0] == len(runs) + len(stray) == 5, prof
    pad = padding_mask(arena)
    for name, flat in (("p", arena.flat_p), ("m", arena.m), ("v", arena.v)):
        assert not flat.cpu()[pad].any(), f"padding of {name} moved"
    for i, (p, q, t0) in enumerate(zip(ps, ref, init)):
        o, n = arena.offsets[i], p.numel()
        got = [p.detach().cpu().numpy().ravel(), arena.m[o:o + n].cpu().numpy(), arena.v[o:o + n].cpu().numpy()]
        if i == NONE_IDX:
            assert np.array_equal(bits(got[0]), bits(t0.numpy().ravel())) and not got[1].any() and not got[2].any()
            assert torch.equal(q.detach(), t0.double())
            continue
        P, M, V, bP, bM, bV = R.adamw_iterate(t0.numpy().ravel(), [s[i].numpy().ravel() for s in steps], HYPER["lr"],
                                              HYPER["betas"], HYPER["eps"], HYPER["weight_decay"], 0.5, True)
        st = ropt.state[q]
        ratios = (worst(got[0], q.detach().numpy().ravel(), bP), worst(got[1], st["exp_avg"].numpy().ravel(), bM),
                  worst(got[2], st["exp_avg_sq"].numpy().ravel(), bV))
        report("FusedAdamW.step x3", f"param {i} {tuple(SHAPES[i])} vs torch fp64  p m v", *ratios)
        assert max(ratios) <= 1.0, (i, ratios)


# ------------------------------------------------------- clip_grad_norm_ ---
def clip_grads(kind, grad_scale):
    gen = torch.Generator().manual_seed(5)
    grads = [torch.randn(s, generator=gen) for s in SHAPES]
    if kind == "below":
        grads = [g * 1e-3 for g in grads]
    elif kind in ("equal", "zero"):
        grads = [torch.zeros(s) for s in SHAPES]
        if kind == "equal":   # four elements of 0.5 / grad_scale: the scaled norm is exactly 1
            for i, j in ((0, 3), (3, 4), (5, 129), (6, 1)):
                grads[i].view(-1)[j] = 0.5 / grad_scale
    elif kind == "inf":
        grads[2].view(-1)[77] = float("inf")
    elif kind == "nan":
        grads[4].view(-1)[11] = float("nan")
    return grads


@pytest.mark.parametrize("grad_scale", [1.0, 0.25])
@pytest.mark.parametrize("kind", ["above", "below", "equal", "zero", "inf", "nan"])
def test_clip_grad_norm_mixed_arena(ops, dev, kind, grad_scale):
    """clip_grad_norm_(1.0) over runs and strays against torch.nn.utils.clip_grad_norm_ in float64 on grad_scale * g, then
    (finite cases) one step() against torch AdamW on the clipped, scaled gradients"""
    init, ps, opt = make_arena(dev, 2)
    opt.grad_scale = grad_scale
    arena = opt.arenas[0]
    grads = clip_grads(kind, grad_scale)
    set_grads(ps, grads, dev, strided_column=False)
    live = [i for i in range(len(SHAPES)) if i != NONE_IDX]
    ref = [torch.nn.Parameter(t.double().clone()) for t in init]
    for i in live:
        ref[i].grad = grads[i].double() * grad_scale
    tnorm = float(torch.nn.utils.clip_grad_norm_([ref[i] for i in live], 1.0))
    coef, total = R.clip([grads[i].numpy() for i in live], 1.0, grad_scale)
    norm = opt.clip_grad_norm_(1.0).item()
    got = {i: ps[i].grad.detach().cpu().numpy().ravel() for i in live}
    assert ps[NONE_IDX].grad is None
    if kind == "nan":
        assert math.isnan(norm) and math.isnan(tnorm) and math.isnan(coef)
        assert all(np.isnan(got[i]).all() for i in live), "a NaN norm must reach every gradient, as in torch"
        return
    if kind == "inf":
        assert norm == tnorm == total == float("inf") and coef == 0.0
        for i in live:
            want = ref[i].grad.numpy().ravel()            # 0 everywhere, NaN where the inf was
            assert np.array_equal(np.isnan(got[i]), np.isnan(want)) and not np.nan_to_num(got[i]).any()
        return
    assert abs(total - tnorm) <= 1e-14 * max(tnorm, 1.0)
    assert abs(norm - tnorm) <= R.SLACK * R.NORM_REL * tnorm, (norm, tnorm)
    if kind == "zero":
        assert norm == 0.0
    if kind == "equal":
        assert norm == 1.0 and coef == 1.0 / (1.0 + 1e-6)
    rel = R.SLACK * (R.CLIP_REL + R.U)     # the coefficient, and the one product of wfae_scale
    dgs = {}
    for i in live:
        want = ref[i].grad.numpy().ravel()
        if kind in ("below", "zero"):
            assert np.array_equal(bits(got[i]), bits(grads[i].numpy().ravel())), "coefficient 1 must not move a bit"
        dgs[i] = rel * np.abs(want) / grad_scale
        ratio = worst(got[i].astype(np.float64) * grad_scale, want, rel * np.abs(want))
        report("clip_grad_norm_", f"{kind} grad_scale={grad_scale} param {i}", ratio)
        assert ratio <= 1.0, (i, ratio)
    # one step on what the clip left, against torch on its own clipped gradients
    ropt = torch.optim.AdamW(ref, **HYPER)
    ropt.step()
    opt.step()
    for i in live:
        o, n = arena.offsets[i], ps[i].numel()
        P, M, V, bP, bM, bV = R.adamw_iterate(init[i].numpy().ravel(), [ref[i].grad.numpy().ravel() / grad_scale], HYPER["lr"],
                                              HYPER["betas"], HYPER["eps"], HYPER["weight_decay"], grad_scale, True, dgs=[dgs[i]])
        st = ropt.state[ref[i]]
        ratios = (worst(ps[i].detach().cpu().numpy().ravel(), ref[i].detach().numpy().ravel(), bP),
                  worst(arena.m[o:o + n].cpu().numpy(), st["exp_avg"].numpy().ravel(), bM),
                  worst(arena.v[o:o + n].cpu().numpy(), st["exp_avg_sq"].numpy().ravel(), bV))
        report("clip + step", f"{kind} grad_scale={grad_scale} param {i}  p m v", *ratios)
        assert max(ratios) <= 1.0, (i, ratios)
    assert torch.equal(ps[NONE_IDX].detach().cpu(), init[NONE_IDX])


def test_clip_grad_norm_raises_on_a_strided_stray_gradient(ops, dev):
    init, ps, opt = make_arena(dev, 3)
    grads = clip_grads("above", 1.0)
    set_grads(ps, grads, dev, strided_column=True)
    before_flat = bits(opt.arenas[0].flat_g.cpu().numpy()).copy()
    with pytest.raises(RuntimeError, match="non-contiguous"):
        opt.clip_grad_norm_(1.0)
    torch.cuda.synchronize()
    assert np.array_equal(bits(opt.arenas[0].flat_g.cpu().numpy()), before_flat)
    for i, p in enumerate(ps):
        if i != NONE_IDX:
            assert np.array_equal(bits(p.grad.cpu().numpy().ravel()), bits(grads[i].numpy().ravel())), i


# ------------------------------------------------------ the two scalars ---
@pytest.mark.parametrize("nparts", [1, 7, 300])
def test_clip_coef_alone(ops, dev, nparts):
    r = np.random.default_rng(nparts)
    parts = r.uniform(0.5, 2.0, nparts)
    S = float(np.sum(parts))
    for max_norm, pre in ((0.37, 1.0), (0.37, 0.25), (1e3, 0.5)):
        out = ops.clip_coef(torch.from_numpy(parts).to(dev), max_norm, pre).cpu().numpy().astype(np.float64)
        total = math.sqrt(S) * pre
        coef = min(1.0, max_norm / (total + 1e-6))
        rc = 0.0 if coef == 1.0 else abs(out[0] - coef) / (R.SLACK * R.CLIP_REL * coef)
        rn = abs(out[1] - total) / (R.SLACK * R.NORM_REL * total)
        report("clip_coef", f"parts={nparts} max_norm={max_norm} pre_scale={pre}  coef norm", rc, rn)
        assert rc <= 1.0 and rn <= 1.0
        if coef == 1.0:
            assert out[0] == 1.0
    for bad, want_coef in ((float("nan"), float("nan")), (float("inf"), 0.0)):
        q = parts.copy()
        q[nparts // 2] = bad
        out = ops.clip_coef(torch.from_numpy(q).to(dev), 1.0, 1.0).cpu().numpy()
        assert (math.isnan(out[0]) and math.isnan(out[1])) if math.isnan(bad) else (out[0] == want_coef and np.isinf(out[1]))


@pytest.mark.parametrize("ss_rec,ss_disc,dw", [(4.0, 9.0, 0.5), (123.456, 0.789, 0.8), (4.0, 0.0, 1.0), (1e12, 1e-12, 1.0),
                                               (0.0, 3.0, 0.7), (float("nan"), 1.0, 1.0), (1.0, float("nan"), 1.0)])
def test_adaptive_weight_alone(ops, dev, ss_rec, ss_disc, dw):
    a = torch.tensor(ss_rec, dtype=torch.float64, device=dev)
    b = torch.tensor(ss_disc, dtype=torch.float64, device=dev)
    got = float(ops.adaptive_weight(a, b, dw).item())
    want = R.adaptive_weight(ss_rec, ss_disc, dw)
    if math.isnan(want):
        assert math.isnan(got), "torch.clamp keeps a NaN"
        return
    if want in (0.0, 1e4):
        assert got == float(f32(want))
        return
    ratio = abs(got - want) / (R.SLACK * R.ADAPTIVE_REL * want)
    report("adaptive_weight", f"ss_rec={ss_rec} ss_disc={ss_disc} w={dw}", ratio)
    assert ratio <= 1.0
