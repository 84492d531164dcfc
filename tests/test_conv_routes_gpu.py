"""GPU: the spatial convolution kernels (csrc/dconv.hip, csrc/c1conv.hip, csrc/g3b.hip, the grouped-3x3 weight-gradient
dispatcher, the direct 4x4 stride-2 GEMMs and the flat-shift 4x4 stride-1 GEMMs of csrc/gemm.hip) against the float64
restatement of tests/conv_ref.py, per element, on every route of their dispatch (conv_ref.CASES).

exact:  integer inputs — the result holds the bits of the float64 result: at 'highest' with the split switch on and off, at
        'medium', the g3b fp32 routes also beside set_g3b(False); weight gradients again accumulating onto an integer dw.
real / offset:  e = max |got - ref64| / S under 3 e_torch32 + 2 U (conv_ref.real_bar); a bf16-stored result between the bf16
        roundings of ref64 -+ that bound.  Every case prints `conv_fp64 <case> <kind> e_gpu / U  e_torch32 / U`
        (profiles/r06_conv_fp64_errors.txt is that output)."""
import pytest
import torch

from tests import conv_ref as R

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
G3B_DIRECT = {"g3b_fwd_f32": "wfae_g3b_fwd", "g3b_fwd_bf16": "wfae_g3b_fwd_bf16", "g3b_bwd_weight_f32": "wfae_g3b_bwd_weight",
              "g3b_bwd_weight_bf16": "wfae_g3b_bwd_weight_bf16"}


@pytest.fixture(scope="module")
def ops(dev):
    from weatherforecastingtoolkit_amd import ops as o
    return o


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _stream():
    return torch.cuda.current_stream().cuda_stream


def run(ops, dev, case, label, t, accumulate=False):
    """one launch of the case's entry point -> the result.  g3b routes and short workspaces go to the entry point itself
    (a route that is not served there is an error, not another kernel); everything else through ops, as the model does"""
    from weatherforecastingtoolkit_amd import _lib
    g, bf = R.geometry(case.ep, case.shape), case.storage == "bf16"
    act = (lambda v: v.to(dev).bfloat16()) if bf else (lambda v: v.to(dev))
    w = t["w"].to(dev)
    fam, op = case.ep.split("_")
    dw = None
    if g.op == "wgrad":
        dw = t["dw0"].to(dev).clone() if accumulate else torch.full(g.w, float("nan"), device=dev)
    ws = ops.workspace()
    wsb = R.ws_bytes(case) or ws.numel()
    if fam == "g3":
        nb, c, h, wd, groups = case.shape
        if g.op != "wgrad":
            src = act(t["x"] if g.op == "fwd" else t["dy"])
            if label in G3B_DIRECT:
                y = torch.empty_like(src)
                _lib.call(G3B_DIRECT[label], src.data_ptr(), w.data_ptr(), y.data_ptr(), nb, c, h, wd, groups, int(g.op == "dgrad"),
                          ws.data_ptr(), ws.numel(), _stream())
                return y
            return ops.gconv3x3_fwd(src, w, groups, g.op == "dgrad")
        dy, x = act(t["dy"]), act(t["x"])
        if label in G3B_DIRECT or case.ws is not None:
            name = G3B_DIRECT.get(label, "wfae_gconv3x3_bwd_weight")
            _lib.call(name, dy.data_ptr(), x.data_ptr(), dw.data_ptr(), nb, c, h, wd, groups, int(accumulate), ws.data_ptr(), wsb, _stream())
            return dw
        return ops.gconv3x3_bwd_weight(dy, x, dw, groups, accumulate)
    if fam == "d":
        nb, cin, cout, h, wd, ks, stride, pad, groups = case.shape
        if g.op == "fwd":
            bias = t["bias"].to(dev)
            if bf and cin == 1:
                return ops.dconv_fwd(t["x"].to(dev), w, bias, ks, stride, pad, groups, out_dtype=BF)
            return ops.dconv_fwd(act(t["x"]), w, bias, ks, stride, pad, groups)
        if g.op == "dgrad":
            return ops.dconv_bwd_data(t["dy"].to(dev), w, cin, ks, pad, groups, out_dtype=BF if bf else torch.float32)
        dy = t["dy"].to(dev).bfloat16() if bf and cin == 1 else t["dy"].to(dev)
        x = t["x"].to(dev).bfloat16() if bf and cin != 1 else t["x"].to(dev)
        if case.ws is not None:
            _lib.call("wfae_dconv_bwd_weight", dy.data_ptr(), x.data_ptr(), dw.data_ptr(), nb, cin, cout, h, wd, ks, stride, pad, groups,
                      int(accumulate), ws.data_ptr(), wsb, _stream())
            return dw
        return ops.dconv_bwd_weight(dy, x, dw, ks, stride, pad, groups, accumulate)
    if fam == "s2":
        if g.op == "fwd":
            return ops.conv4x4s2_down(t["x"].to(dev), w)
        if g.op == "dgrad":
            return ops.conv4x4s2_up(t["dy"].to(dev), w)
        return ops.conv4x4s2_wgrad(t["dy"].to(dev), t["x"].to(dev), dw, accumulate)
    pad = case.shape[5]
    if g.op == "fwd":
        return ops.conv4x4s1_fwd(t["x"].to(dev), w, pad, False)
    if g.op == "dgrad":
        return ops.conv4x4s1_fwd(t["dy"].to(dev), w, pad, True)
    return ops.conv4x4s1_bwd_weight(t["dy"].to(dev), t["x"].to(dev), dw, pad, accumulate)


class Config:
    """precision / split / g3b / Winograd switches around a block, restored on the way out"""

    def __init__(self, ops, precision="highest", split=True, g3b=True):
        self.ops, self.precision, self.split, self.g3b = ops, precision, split, g3b

    def __enter__(self):
        self.ops.set_float32_matmul_precision(self.precision)
        self.ops.set_split_gemm(self.split)
        self.ops.set_g3b(self.g3b)
        self.ops.set_winograd(False)
        return self

    def __exit__(self, *exc):
        self.ops.set_float32_matmul_precision("highest")
        self.ops.set_split_gemm(True)
        self.ops.set_g3b(True)
        self.ops.set_winograd("auto")
        return False


def configs(case):
    if case.storage == "bf16":
        return [dict(precision="medium")]
    out = [dict(), dict(split=False), dict(precision="medium")]
    if case.route in ("g3b_fwd_f32", "g3b_bwd_weight_f32"):
        out.append(dict(g3b=False))
    return out


def resolve(case):
    """the multi-trip cases take their batch from this chip's CU count"""
    if case.note != "three trips":
        return case
    case = case._replace(shape=R.gconv3p_multitrip_shape(case.shape[1] // case.shape[4], _cus()))
    x = R.ctx(case, cus=_cus())
    items, cap = R.gconv3p_items_cap(x)
    assert items >= 2 * cap + 1 and R.gconv3p_trips(x) >= 3, (items, cap)
    return case


def _params():
    return [pytest.param(c, k, id=R.case_id(c) + "-" + k) for c in R.CASES for k in R.kinds_of(c)]


@pytest.mark.parametrize("case,kind", _params())
def test_route_against_float64(ops, dev, case, kind):
    case = resolve(case)
    g, bf = R.geometry(case.ep, case.shape), case.storage == "bf16"
    t = R.inputs(g, kind, 1 + len(case.shape) + sum(case.shape), bf16=bf)
    plain = dict(t, dw0=None)
    ref = R.reference(g, plain)
    for n, cfg in enumerate(configs(case) if kind == "exact" else configs(case)[:1]):
        x = R.Ctx(case.ep, case.shape, case.storage, cus=_cus(), ws=R.ws_bytes(case), **cfg)
        labels = R.routes_of(x)
        assert len(labels) == 1 and (n > 0 or labels == [case.route]), (labels, cfg)
        with Config(ops, **cfg):
            got = run(ops, dev, case, labels[0], t)
            acc = run(ops, dev, case, labels[0], t, accumulate=True) if g.op == "wgrad" else None
        out_bf = got.dtype == BF
        if kind == "exact":
            assert R.bits_equal(got, ref, bf16=out_bf), (labels[0], cfg, R.first_mismatches(got, ref))
            if acc is not None:
                ref_acc = R.reference(g, t)
                assert R.bits_equal(acc, ref_acc), ("accumulate", labels[0], cfg, R.first_mismatches(acc, ref_acc))
            continue
        s = R.reference(g, plain, absolute=True)
        e_gpu, e_t32 = R.elem_err(got, ref, s), R.elem_err(R.torch32(g, plain), ref, s)
        print("conv_fp64 %-62s %-6s e_gpu %8.2f U   e_torch32 %6.2f U%s" % (R.case_id(case), kind, e_gpu / R.U, e_t32 / R.U,
                                                                         "   (bf16 result)" if out_bf else ""))
        if out_bf:
            assert R.bf16_within(got, ref, R.real_bar(e_t32) * s), (labels[0], e_t32 / R.U)
        else:
            assert e_gpu <= R.real_bar(e_t32), (labels[0], e_gpu / R.U, e_t32 / R.U)
        if acc is not None:
            ref_acc, s_acc = R.reference(g, t), R.reference(g, t, absolute=True)
            e_acc, e_t32a = R.elem_err(acc, ref_acc, s_acc), R.elem_err(R.torch32(g, t), ref_acc, s_acc)
            print("conv_fp64 %-62s %-6s e_gpu %8.2f U   e_torch32 %6.2f U   (accumulate)" % (R.case_id(case), kind, e_acc / R.U, e_t32a / R.U))
            assert e_acc <= R.real_bar(e_t32a), ("accumulate", labels[0], e_acc / R.U, e_t32a / R.U)


def test_every_route_label_is_exercised():
    assert {c.route for c in R.CASES} == set(R.ROUTES)
