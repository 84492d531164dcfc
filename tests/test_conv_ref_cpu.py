"""CPU: tests/conv_ref.py against torch's float64 autograd on every case shape; the case table against the dispatch
predicates (every route has an exact and a real-valued case, every case lands on its route, the multi-trip cases take the
trips they are there for); and the two checks against the corruptions they are meant to catch — with the old bar
(whole-tensor relerr < 2e-5 against torch fp32) shown to let the first of them through."""
import pytest
import torch

from tests import conv_ref as R


def _geoms():
    """one (x, w, dy, ks, stride, pad, groups) per distinct geometry of the table: the three operations share it"""
    seen = {}
    for c in R.CASES:
        g = R.geometry(c.ep, c.shape)
        seen.setdefault((g.x, g.w, g.dy, g.ks, g.stride, g.pad, g.groups), g)
    return list(seen.values())


@pytest.mark.parametrize("g", _geoms(), ids=lambda g: "x".join(map(str, g.x)) + "-w" + "x".join(map(str, g.w)) + "-s%dp%d" % (g.stride, g.pad))
def test_reference_matches_torch_float64_autograd(g):
    t = R.inputs(g._replace(bias=True), "real", 7)
    y, dx, dw = R.torch_conv(t["x"], t["w"], t["bias"], t["dy"], g.stride, g.pad, g.groups, torch.float64)
    for got, want, op in ((R.conv64(t["x"], t["w"], t["bias"], g.stride, g.pad, g.groups), y, "fwd"),
                          (R.dgrad64(t["dy"], t["w"], g.stride, g.pad, g.groups, in_hw=g.x[2:]), dx, "dgrad"),
                          (R.wgrad64(t["dy"], t["x"], g.ks, g.stride, g.pad, g.groups), dw, "wgrad")):
        assert got.shape == want.shape, op
        # two float64 orders of one sum: a few 2^-53 of the sum of magnitudes; 1e-12 of the largest value is 10^3 times that
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), op


def _max_s_bound(case):
    """an upper bound of max S of an exact case: every term is at most 3 x 3 (the bias, the accumulated-onto dw: 3)"""
    g = R.geometry(case.ep, case.shape)
    if g.op == "fwd":
        return 9 * g.w[1] * g.ks * g.ks + 3
    if g.op == "dgrad":
        return 9 * (g.w[0] // g.groups) * g.ks * g.ks
    return 9 * g.dy[0] * g.dy[2] * g.dy[3] + 3


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_case_lands_on_its_route_and_stays_exact(case):
    assert case.route in R.ROUTES
    assert R.routes_of(R.ctx(case)) == [case.route]
    assert _max_s_bound(case) < R.EXACT_LIMIT
    g = R.geometry(case.ep, case.shape)
    if g.x[0] * g.x[1] * g.x[2] * g.x[3] <= 1 << 18:      # the bound is one: S itself, where it is cheap
        t = R.inputs(g, "exact", 3)
        s = R.reference(g, t, absolute=True)
        assert float(s.max()) <= _max_s_bound(case) and float(s.max()) < R.EXACT_LIMIT
        assert torch.equal(R.reference(g, t), R.reference(g, t).round()), "integers in, integers out"


def test_every_route_has_an_exact_and_a_real_valued_case():
    for label in R.ROUTES:
        mine = [c for c in R.CASES if c.route == label]
        assert mine, label
        assert any("real" in R.kinds_of(c) and "offset" in R.kinds_of(c) for c in mine), label
        assert all("exact" in R.kinds_of(c) for c in mine), label
    for c in R.CASES:   # real-valued weight gradients stay where a lost plane stands above the summation noise
        g = R.geometry(c.ep, c.shape)
        if g.op == "wgrad" and "real" in R.kinds_of(c):
            assert g.dy[0] * g.dy[2] * g.dy[3] <= R.WGRAD_REAL_PIXELS
    groups = {c.shape[4] for c in R.CASES if c.ep.startswith("g3_")}
    assert {6, 8, 32} <= groups


@pytest.mark.parametrize("cus", [256, 304, 64, 8])
def test_gconv3p_multitrip_cases_take_three_trips(cus):
    cases = R.multitrip_cases(cus)
    assert [c.route for c in cases] == ["gconv3p<4>", "gconv3p<8>"]
    for c in cases:
        x = R.ctx(c, cus=cus)
        items, cap = R.gconv3p_items_cap(x)
        assert R.routes_of(x) == [c.route]
        assert items >= 2 * cap + 1 and R.gconv3p_trips(x) >= 3
        assert c.shape[2:4] == (17, 68), "2 x 2 partial tiles per image"
    if cus == 256:
        assert all(R.gconv3p_trips(R.ctx(c)) == 3 for c in cases)
        assert [c.shape for c in cases] == [(9, 128, 17, 68, 32), (25, 256, 17, 68, 32)]
        assert all(c in R.CASES for c in cases)


def test_short_workspace_cases_walk_their_tiles():
    short = [c for c in R.CASES if c.ws is not None]
    assert {c.route for c in short} >= {"gconv3_wgrad_mfma<4>", "gconv3_wgrad_mfma<8>", "gconv3_wgrad_mfma<16>", "gconv3_wgrad_mfma<32>",
                                        "gconv3_wgrad_valu<4,2>", "gconv3_wgrad_valu<8,2>", "dconv_wgrad<3,1,4>", "dconv_wgrad<3,1,1>",
                                        "dconv_wgrad<4,2,4>", "dconv_wgrad<4,1,1>", "B_WGRAD3"}
    for c in short:
        total, parts = R.wgrad_trips(c)
        assert parts == c.ws[1], (c, total, parts)                # the --parts branch: the workspace, not the grid, set the count
        full = R.wgrad_trips(c._replace(ws=None))[1]
        assert full > parts, (c, full)
        if c.route == "B_WGRAD3":
            continue
        assert total >= 7 and -(-total // parts) >= 4, (c, total, parts)
        if parts == 3:
            assert total % 3 != 0, (c, total)
    # c1_wgrad_mfma: an odd tile count on one block
    for c in R.CASES:
        if "three tiles on one block" in c.note:
            assert R.wgrad_trips(c) == (3, 1), c
    # the two fallbacks of dconv.hip:414-421 on a short workspace
    a, b = [c for c in short if c.route == "dconv_wgrad<3,1,1>"]
    assert R.routes_of(R.ctx(a._replace(ws=None))) == ["c1conv3_wgrad"]
    assert R.routes_of(R.ctx(b._replace(ws=None))) == ["c1_wgrad_mfma<flip1>"]
    assert R.routes_of(R.ctx(b._replace(ws=("slabs", 2)))) == ["c1conv3_wgrad"]


# ---------------------------------------------------------------------------------------------------- the checkers bite
def _hm(v):
    """the h + m bf16 planes of an fp32 tensor: 16 significant bits, the third plane lost"""
    h = v.bfloat16().float()
    return (h + (v - h).bfloat16().float()).double()


G3 = lambda shape: R.geometry("g3_fwd", shape + (8,))


@pytest.mark.parametrize("shape", [(2, 32, 16, 16), (2, 64, 24, 40), (2, 256, 16, 32), (3, 128, 40, 200)])
def test_a_lost_operand_plane_passes_the_old_bar_and_is_rejected(shape):
    g = G3(shape)
    t = R.inputs(g, "real", 11)
    ref, s, y32 = R.reference(g, t), R.reference(g, t, absolute=True), R.torch32(g, t)
    lost = R.conv64(_hm(t["x"]), _hm(t["w"]), None, 1, 1, 8).float()
    e_lost, e_32 = R.elem_err(lost, ref, s), R.elem_err(y32, ref, s)
    print("lost l plane %s: relerr %.2e, e %.1f U, torch fp32 %.1f U" % (shape, R.old_relerr(lost, y32), e_lost / R.U, e_32 / R.U))
    assert R.old_relerr(lost, y32) < R.OLD_TOL, "the gap: the whole-tensor bar lets it through"
    assert e_lost > R.real_bar(e_32), (e_lost / R.U, e_32 / R.U)
    assert e_32 <= R.real_bar(e_32)
    # on exact inputs nothing is lost (integers fit one plane): this corruption is the real-valued check's to catch
    te = R.inputs(g, "exact", 11)
    assert R.bits_equal(R.conv64(_hm(te["x"]), _hm(te["w"]), None, 1, 1, 8).float(), R.reference(g, te))


@pytest.mark.parametrize("kind", ["exact", "real", "offset"])
def test_a_shifted_tile_and_a_zeroed_halo_column_are_rejected(kind):
    """one 16 x 64 tile of gconv3p stored one column off; one tile computed with its right halo column read as zero: what a
    wrong second trip of the persistent loop would leave.  The whole-tensor relerr sees both too (printed) — but only in a
    test whose grid takes that trip, which the kernel tests' did not"""
    g = G3((2, 32, 17, 132))
    t = R.inputs(g, kind, 13)
    ref, s = R.reference(g, t), R.reference(g, t, absolute=True)
    good = R.torch32(g, t) if kind != "exact" else ref.float()
    bar = R.real_bar(R.elem_err(good, ref, s))
    assert R.elem_err(good, ref, s) <= bar and (kind != "exact" or R.bits_equal(good, ref))
    shifted = good.clone()
    shifted[1, 4:8, 0:16, 64:128] = good[1, 4:8, 0:16, 65:129]
    x0 = t["x"].clone()
    x0[1, 4:8, :, 128] = 0.0                                   # the halo column right of tile (0, 1) of group 1
    halo = good.clone()
    halo[1, 4:8, 0:16, 127] = R.conv64(x0, t["w"], None, 1, 1, 8).float()[1, 4:8, 0:16, 127]
    for name, bad in (("shifted tile", shifted), ("zeroed halo column", halo)):
        e = R.elem_err(bad, ref, s)
        print("%s (%s): e %.3g U against a bar of %.1f U; relerr %.2e" % (name, kind, e / R.U, bar / R.U, R.old_relerr(bad, good)))
        assert e > bar, name
        if kind == "exact":
            assert not R.bits_equal(bad, ref), name
            assert R.first_mismatches(bad, ref)[0] > 0


@pytest.mark.parametrize("kind", ["exact", "real"])
def test_a_weight_gradient_missing_one_tile_is_rejected(kind):
    """28 tiles of 8 x 16 pixels, one of them never added: the exact check, and at 2000 pixels the real-valued one"""
    g = R.geometry("g3_wgrad", (2, 32, 50, 20, 8))
    t = R.inputs(g, kind, 17)
    t["dw0"] = None
    ref, s = R.reference(g, t), R.reference(g, t, absolute=True)
    good = R.torch32(g, t) if kind == "real" else ref.float()
    dy = t["dy"].clone()
    dy[1, :, 48:50, 16:20] = 0.0                               # the last, partial tile: 2 x 4 pixels of 2000
    bad = R.wgrad64(dy, t["x"], 3, 1, 1, 8).float()
    bar = R.real_bar(R.elem_err(good, ref, s))
    assert R.elem_err(good, ref, s) <= bar
    assert R.elem_err(bad, ref, s) > bar
    if kind == "exact":
        assert R.bits_equal(good, ref) and not R.bits_equal(bad, ref)


def test_bf16_results_are_held_to_the_rounding_of_the_reference():
    g = G3((1, 32, 16, 33))
    t = R.inputs(g, "real", 19, bf16=True)
    ref, s = R.reference(g, t), R.reference(g, t, absolute=True)
    y32 = R.torch32(g, t)
    bound = R.real_bar(R.elem_err(y32, ref, s)) * s
    assert R.bf16_within(y32.bfloat16(), ref, bound)
    lost = R.conv64(_hm(t["x"]) * (1 + 2.0 ** -9), t["w"], None, 1, 1, 8).float()     # half a bf16 ulp off: 2^-9 relative
    assert not R.bf16_within(lost.bfloat16(), ref, bound)
    te = R.inputs(g, "exact", 19)
    assert R.bits_equal(R.reference(g, te).to(torch.bfloat16), R.reference(g, te), bf16=True)
    assert not R.bits_equal(R.reference(g, te).float(), R.reference(g, te), bf16=True)
