"""Plain float64 restatement (torch on the CPU, no library import) of the spatial convolutions of csrc/dconv.hip,
csrc/c1conv.hip, csrc/g3b.hip and of the gather / flat-shift GEMMs of csrc/gemm.hip (grouped 3x3, 4x4 stride 2, 4x4 stride 1,
the one-channel first and last layers): forward, data gradient and weight gradient as sums over taps of shifted slices,
never torch's own convolution — together with the inputs on which the kernels are held to it, the dispatch of the library
restated as predicates, and the table of cases that walks every route of that dispatch.

Two checks per case.
  exact:  integer-valued inputs in [-3, 3].  Such values are exact in fp32, in one bf16 plane and in all three split planes,
          every partial sum of every summation order is an integer below S = conv(|x|, |w|), so while max S < 2^24 a correct
          kernel owes THE BITS of the float64 result, in fp32 mode, split mode and 'medium' mode; a bf16-stored result owes
          ref64.to(bfloat16).  No tolerance: one lost tile, halo column or slab shows.
  real:   the suite's uniform data (and a second flavour with a per-channel offset, x = 1.5 + u, like post-GELU
          activations): e = max_elem |got - ref64| / S_elem, S the same sum over magnitudes, must stay under
          3 e_torch32 + 2 U, e_torch32 being torch's own fp32 CPU convolution / autograd on the same inputs.  3 is the spread
          between two correct fp32 orders of one sum (tests/test_split_gemm_gpu.py, grouped wgrad: measured 0.5 - 2x), 2 U
          the final rounding and one slab addition.  A kernel that drops the third bf16 plane of its operands sits at
          25 - 74 U on this scale (tests/test_conv_ref_cpu.py) and passes the whole-tensor relerr < 2e-5 by a factor of 6.

tests/test_conv_ref_cpu.py holds this file to torch's float64 autograd and shows that both checks reject the corruptions
they are meant for; tests/test_conv_routes_gpu.py runs the table on the GPU."""
import collections

import torch
import torch.nn.functional as F

U = 2.0 ** -24            # unit roundoff of fp32
EXACT_LIMIT = 2.0 ** 24   # integers below it are fp32 values, and so is every partial sum of an exact case
REAL_FACTOR, REAL_SLACK = 3.0, 2.0 * U
WGRAD_REAL_PIXELS = 2048  # real-valued wgrad cases: N * Ho * Wo at most this (beyond it a lost plane sinks below the summation noise)


def _d(t):
    return None if t is None else torch.as_tensor(t).detach().to("cpu", torch.float64)


# ---------------------------------------------------------------------------------------------------- reference functions
def _out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def _padded(x, pad):
    nb, c, h, w = x.shape
    xp = torch.zeros((nb, c, h + 2 * pad, w + 2 * pad), dtype=x.dtype)
    xp[:, :, pad:pad + h, pad:pad + w] = x
    return xp


def _taps(kh, kw, ho, wo, stride):
    """(ky, kx, row slice, column slice) of the padded input that tap (ky, kx) multiplies into the ho x wo outputs"""
    for ky in range(kh):
        for kx in range(kw):
            yield ky, kx, slice(ky, ky + stride * (ho - 1) + 1, stride), slice(kx, kx + stride * (wo - 1) + 1, stride)


def conv64(x, w, bias=None, stride=1, pad=0, groups=1):
    """y[n, o, p] = bias[o] + sum_{i, tap} w[o, i, tap] x[n, i, stride p + tap - pad]; x (N, Cin, H, W), w (Cout, Cin / groups, KH, KW)"""
    x, w = _d(x), _d(w)
    nb, cin, h, wd = x.shape
    cout, ig, kh, kw = w.shape
    og = cout // groups
    ho, wo = _out_size(h, kh, stride, pad), _out_size(wd, kw, stride, pad)
    xg = _padded(x, pad).view(nb, groups, ig, h + 2 * pad, wd + 2 * pad)
    wg = w.view(groups, og, ig, kh, kw)
    y = torch.zeros((nb, groups, og, ho, wo), dtype=torch.float64)
    for ky, kx, ys, xs in _taps(kh, kw, ho, wo, stride):
        y += torch.einsum("ngihw,goi->ngohw", xg[:, :, :, ys, xs], wg[:, :, :, ky, kx])
    y = y.view(nb, cout, ho, wo)
    return y if bias is None else y + _d(bias).view(1, -1, 1, 1)


def dgrad64(dy, w, stride=1, pad=0, groups=1, in_hw=None):
    """dx[n, i, q] = sum over (o, tap, p) with stride p + tap - pad = q of w[o, i, tap] dy[n, o, p]; in_hw: the input plane,
    (Ho - 1) stride + K - 2 pad when not given"""
    dy, w = _d(dy), _d(w)
    nb, cout, ho, wo = dy.shape
    _, ig, kh, kw = w.shape
    og = cout // groups
    h, wd = in_hw if in_hw is not None else ((ho - 1) * stride + kh - 2 * pad, (wo - 1) * stride + kw - 2 * pad)
    dyg = dy.view(nb, groups, og, ho, wo)
    wg = w.view(groups, og, ig, kh, kw)
    dxp = torch.zeros((nb, groups, ig, h + 2 * pad, wd + 2 * pad), dtype=torch.float64)
    for ky, kx, ys, xs in _taps(kh, kw, ho, wo, stride):
        dxp[:, :, :, ys, xs] += torch.einsum("ngohw,goi->ngihw", dyg, wg[:, :, :, ky, kx])
    return dxp[:, :, :, pad:pad + h, pad:pad + wd].reshape(nb, groups * ig, h, wd)


def wgrad64(dy, x, ksize, stride=1, pad=0, groups=1):
    """dw[o, i, tap] = sum_{n, p} dy[n, o, p] x[n, i, stride p + tap - pad]"""
    dy, x = _d(dy), _d(x)
    nb, cout, ho, wo = dy.shape
    cin, h, wd = x.shape[1:]
    og, ig = cout // groups, cin // groups
    dyg = dy.view(nb, groups, og, ho, wo)
    xg = _padded(x, pad).view(nb, groups, ig, h + 2 * pad, wd + 2 * pad)
    dw = torch.zeros((groups, og, ig, ksize, ksize), dtype=torch.float64)
    for ky, kx, ys, xs in _taps(ksize, ksize, ho, wo, stride):
        dw[:, :, :, ky, kx] = torch.einsum("ngohw,ngihw->goi", dyg, xg[:, :, :, ys, xs])
    return dw.view(cout, ig, ksize, ksize)


def torch_conv(x, w, bias, dy, stride, pad, groups, dtype):
    """torch's OWN convolution and autograd in `dtype` -> (y, dx, dw): float64 is what the restatement above is held to,
    float32 the comparator of the real-valued bar"""
    xr = x.detach().to(dtype).requires_grad_(True)
    wr = w.detach().to(dtype).requires_grad_(True)
    y = F.conv2d(xr, wr, None if bias is None else bias.to(dtype), stride=stride, padding=pad, groups=groups)
    y.backward(dy.to(dtype))
    return y.detach(), xr.grad, wr.grad


# ----------------------------------------------------------------------------------------------------------------- inputs
def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def exact_inputs(shape, seed):
    """integer-valued fp32 tensor in [-3, 3]"""
    return torch.randint(-3, 4, tuple(shape), generator=_gen(seed)).float()


def real_inputs(shape, seed, lo=-1.0, hi=1.0, offset=0.0, bf16=False):
    """the suite's uniform data (tests/test_kernels_gpu.py rnd); offset: x = offset + u; bf16: rounded to bf16 values (what a
    bf16-stored tensor holds — the reference then multiplies the very same values)"""
    v = (torch.rand(tuple(shape), generator=_gen(seed)) * (hi - lo) + lo).float() + offset
    return v.bfloat16().float() if bf16 else v


# --------------------------------------------------------------------------------------------------------------- geometry
# entry points (ep) and their shape tuples:
#   g3_fwd, g3_dgrad, g3_wgrad   (N, C, H, W, groups)                          ops.gconv3x3_fwd / gconv3x3_bwd_weight
#   d_fwd, d_dgrad, d_wgrad      (N, Cin, Cout, H, W, ks, stride, pad, groups)  ops.dconv_fwd / dconv_bwd_data / dconv_bwd_weight
#   s2_down, s2_up, s2_wgrad     (N, Chi, Clo, Hlo, Wlo)                       ops.conv4x4s2_* with Winograd off
#   s1_fwd, s1_dgrad, s1_wgrad   (N, Cin, Cout, H, W, pad)                     ops.conv4x4s1_fwd / conv4x4s1_bwd_weight
Geom = collections.namedtuple("Geom", "op x w dy ks stride pad groups bias")


def geometry(ep, shape):
    """-> Geom: the operation (fwd / dgrad / wgrad), the shapes of x, w and dy, and the convolution's parameters"""
    fam, op = ep.split("_")
    op = {"down": "fwd", "up": "dgrad"}.get(op, op)
    if fam == "g3":
        nb, c, h, w, groups = shape
        return Geom(op, (nb, c, h, w), (c, c // groups, 3, 3), (nb, c, h, w), 3, 1, 1, groups, False)
    if fam == "d":
        nb, cin, cout, h, w, ks, stride, pad, groups = shape
        ho, wo = _out_size(h, ks, stride, pad), _out_size(w, ks, stride, pad)
        return Geom(op, (nb, cin, h, w), (cout, cin // groups, ks, ks), (nb, cout, ho, wo), ks, stride, pad, groups, op == "fwd")
    if fam == "s2":
        nb, chi, clo, hlo, wlo = shape
        return Geom(op, (nb, chi, 2 * hlo, 2 * wlo), (clo, chi, 4, 4), (nb, clo, hlo, wlo), 4, 2, 1, 1, False)
    if fam == "s1":
        nb, cin, cout, h, w, pad = shape
        return Geom(op, (nb, cin, h, w), (cout, cin, 4, 4), (nb, cout, h + 2 * pad - 3, w + 2 * pad - 3), 4, 1, pad, 1, False)
    raise ValueError(ep)


def out_shape(g):
    return {"fwd": g.dy, "dgrad": g.x, "wgrad": g.w}[g.op]


def reference(g, t, absolute=False):
    """float64 result of Geom g on the tensors t = dict(x, w, dy, bias, dw0); absolute: the same sums over magnitudes, the
    per-element scale S.  dw0: what an accumulating weight gradient adds onto"""
    f = (lambda v: None if v is None else _d(v).abs()) if absolute else _d
    if g.op == "fwd":
        return conv64(f(t["x"]), f(t["w"]), f(t.get("bias")), g.stride, g.pad, g.groups)
    if g.op == "dgrad":
        return dgrad64(f(t["dy"]), f(t["w"]), g.stride, g.pad, g.groups, in_hw=g.x[2:])
    dw = wgrad64(f(t["dy"]), f(t["x"]), g.ks, g.stride, g.pad, g.groups)
    return dw if t.get("dw0") is None else dw + f(t["dw0"])


def torch32(g, t):
    """the same result from torch's fp32 CPU convolution / autograd: the comparator of the real-valued bar"""
    bias = t.get("bias")
    x = t["x"] if g.op != "dgrad" else torch.zeros(g.x)
    dy = t["dy"] if g.op != "fwd" else torch.zeros(g.dy)
    w = t["w"] if g.op != "wgrad" else torch.zeros(g.w)
    y, dx, dw = torch_conv(x, w, bias, dy, g.stride, g.pad, g.groups, torch.float32)
    if g.op == "fwd":
        return y
    if g.op == "dgrad":
        return dx
    return dw if t.get("dw0") is None else dw + t["dw0"]


KINDS = ("exact", "real", "offset")


def inputs(g, kind, seed, bf16=False):
    """the tensors of one case.  exact: integers; real: uniform in (-1, 1), weights scaled like the suite's; offset: x (and
    the cotangent of a data gradient) carry +1.5.  bf16: activations AND weights hold bf16 values (g3b.hip multiplies the
    weights' bf16 rounding, dconv.hip the fp32 weights: on bf16-valued weights both owe the same sums)"""
    t = {}
    if kind == "exact":
        t["x"], t["w"], t["dy"] = exact_inputs(g.x, seed), exact_inputs(g.w, seed + 1), exact_inputs(g.dy, seed + 2)
        t["bias"] = exact_inputs((g.w[0],), seed + 3) if g.bias else None
        t["dw0"] = exact_inputs(g.w, seed + 4)
    else:
        off = 1.5 if kind == "offset" else 0.0
        t["x"] = real_inputs(g.x, seed, offset=off, bf16=bf16)
        t["w"] = real_inputs(g.w, seed + 1, -0.3, 0.3, bf16=bf16)
        t["dy"] = real_inputs(g.dy, seed + 2, offset=off if g.op == "dgrad" else 0.0, bf16=bf16)
        t["bias"] = real_inputs((g.w[0],), seed + 3) if g.bias else None
        t["dw0"] = real_inputs(g.w, seed + 4)
    return t


# ---------------------------------------------------------------------------------------------------------------- checkers
def bits_equal(got, ref64, bf16=False):
    """the exact check: got holds the float64 result's bits (a bf16-stored result: its rounding)"""
    want = ref64.to(torch.bfloat16) if bf16 else ref64.to(torch.float32)
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(got.cpu(), want)


def first_mismatches(got, ref64, limit=4):
    """[(index, got, want)] for the assertion message of a failed exact check"""
    bad = (got.detach().cpu().double() != ref64).nonzero()
    return int(bad.shape[0]), [(tuple(i.tolist()), float(got.cpu().double()[tuple(i)]), float(ref64[tuple(i)])) for i in bad[:limit]]


def elem_err(got, ref64, s64):
    """e = max over elements of |got - ref64| / S; an element with S = 0 (every term zero) owes exactly 0"""
    d = (got.detach().cpu().double() - ref64).abs()
    return float(torch.where(s64 > 0, d / s64.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), d)).max())


def real_bar(e_torch32):
    return REAL_FACTOR * e_torch32 + REAL_SLACK


def bf16_within(got_bf16, ref64, bound):
    """a bf16-stored result under the real-valued bar: rounding is monotone, so a value whose fp32 form lies within `bound` of
    ref64 rounds to a bf16 value between the roundings of ref64 - bound and ref64 + bound"""
    got = got_bf16.detach().cpu().double()
    lo = (ref64 - bound).to(torch.bfloat16).double()
    hi = (ref64 + bound).to(torch.bfloat16).double()
    return bool(((got >= lo) & (got <= hi)).all())


def old_relerr(got, ref32):
    """the bar these kernels rested on (tests/_util.py relerr against torch fp32, < 2e-5)"""
    return float((got.double() - ref32.double()).abs().max() / ref32.double().abs().max())


OLD_TOL = 2e-5


# ------------------------------------------------------------------------------------------------------------------ routes
class Ctx:
    """what the dispatch of one call depends on: entry point, shape, storage of the activations ('f32' | 'bf16'), matmul
    precision, the split switch, the g3b switch, the CU count and the workspace the call is given (None: the 512 MiB default).
    Tensors are 16-byte aligned (torch allocations): misaligned base pointers are out of scope"""

    def __init__(self, ep, shape, storage="f32", precision=None, split=True, g3b=True, cus=256, ws=None):
        self.ep, self.shape, self.storage = ep, tuple(shape), storage
        self.precision = precision or ("medium" if storage == "bf16" else "highest")
        self.split, self.g3b, self.cus = split, g3b, cus
        self.ws = (512 << 20) if ws is None else ws
        self.g = geometry(ep, shape)


def cdiv(a, b):
    return -(-a // b)


def g3b_strip(cpg, h, w):
    """g3b.hip:352 — rows per strip, 0 when the (channels per group, W) pair or H is not served"""
    ri = {(4, 384): 1, (8, 192): 2, (16, 96): 4, (32, 48): 8, (32, 24): 12}.get((cpg, w), 0)
    if not ri:
        return 0
    for rh in range(24, ri - 1, -ri):
        if rh % ri == 0 and h % rh == 0:
            return rh
    return 0


def _g3(c):
    nb, ch, h, w, groups = c.shape
    return nb, ch, h, w, groups, ch // groups


def g3b_supported(c):
    """g3b.hip:591"""
    nb, ch, h, w, groups, cpg = _g3(c)
    v = 32 if cpg == 32 else 16
    return ch % v == 0 and ch // v <= 65535 and g3b_strip(cpg, h, w) > 0


def g3b_f32_supported(c, wgrad):
    """g3b.hip:644 — fp32 tensors at fp32 precision with the split switch on; wgrad W <= 96, forward (16, 96) only"""
    nb, ch, h, w, groups, cpg = _g3(c)
    if not (g3b_supported(c) and c.precision == "highest" and c.split):
        return False
    return w <= 96 if wgrad else (cpg == 16 and w == 96)


def r_g3b_fwd_f32(c):
    """ops.gconv3x3_fwd (fp32 branch) -> g3b.hip:656 g3b_launch<16, 6, 96, 3, 3, float>"""
    return c.ep in ("g3_fwd", "g3_dgrad") and c.storage == "f32" and c.g3b and g3b_f32_supported(c, False)


def r_g3b_fwd_bf16(c):
    """ops.gconv3x3_fwd (bf16 branch; ops.g3b_supported: the switch, 'medium', g3b.hip:591) -> g3b.hip:598"""
    return c.ep in ("g3_fwd", "g3_dgrad") and c.storage == "bf16" and c.g3b and c.precision == "medium" and g3b_supported(c)


def _g3_dconv_fwd(c):
    return c.ep in ("g3_fwd", "g3_dgrad") and not r_g3b_fwd_f32(c) and not r_g3b_fwd_bf16(c) and _g3(c)[5] in (4, 8, 16, 32)


def r_gconv3_mfma(cpg, storage):
    def pred(c):
        """dconv.hip:1028 — cpg >= 16 and cpg H W < 2^28"""
        if not c.ep.startswith("g3_"):
            return False
        nb, ch, h, w, groups, k = _g3(c)
        return _g3_dconv_fwd(c) and c.storage == storage and k >= 16 and k * h * w < (1 << 28) and (cpg is None or k == cpg)
    return pred


def gconv3p_taken(c):
    """dconv.hip:1034-1035 — fp32 tensors, cpg <= 8, W % 4 == 0, items < 2^31, cpg H W < 2^24"""
    nb, ch, h, w, groups, k = _g3(c)
    return (c.storage == "f32" and k <= 8 and w % 4 == 0 and cdiv(w, 64) * cdiv(h, 16) * groups * nb < (1 << 31)
            and k * h * w < (1 << 24))


def r_gconv3p(cpg):
    def pred(c):
        return _g3_dconv_fwd(c) and _g3(c)[5] == cpg and gconv3p_taken(c)
    return pred


def r_gconv3(cpg, storage):
    def pred(c):
        """dconv.hip:1040 — what neither the MFMA form nor gconv3p takes: tiles 16 x 32"""
        if not c.ep.startswith("g3_"):
            return False
        k = _g3(c)[5]
        return (_g3_dconv_fwd(c) and c.storage == storage and k < 16 and not gconv3p_taken(c) and (cpg is None or k == cpg))
    return pred


def gconv3p_items_cap(c):
    """dconv.hip:1000-1004 — (items, grid cap): 16 x 64 tiles per (image, group); (CUs / 8) * 8 * (2 | 6) blocks"""
    nb, ch, h, w, groups, k = _g3(c)
    return cdiv(w, 64) * cdiv(h, 16) * groups * nb, c.cus // 8 * 8 * (2 if k == 4 else 6)


def gconv3p_trips(c):
    """the most trips a block of gconv3p_kernel takes (dconv.hip:700-701, 754: block b starts at item (b & 7) pb + (b >> 3)
    and steps by the grid)"""
    items, cap = gconv3p_items_cap(c)
    blocks = min(cdiv(items, 8) * 8, cap)
    return cdiv(items, blocks)


def gconv3p_multitrip_shape(cpg, cus):
    """(N, C, 17, 68, 32 groups) with N the smallest batch at which items >= 2 cap + 1: 2 x 2 partial tiles per image, and
    some blocks take three trips — first, middle, last.  At 256 CUs: (9, 128, ...) and (25, 256, ...)"""
    cap = cus // 8 * 8 * (2 if cpg == 4 else 6)
    nb = cdiv(2 * cap + 1, 4 * 32)
    return (nb, 32 * cpg, 17, 68, 32)


def _wgrad_mfma_taken(c):
    """dconv.hip:1435-1438 — cpg in 4 / 8 / 16 / 32, W % 4 == 0, C a multiple of the MFMA tile's 16 (32) channels"""
    nb, ch, h, w, groups, k = _g3(c)
    v = 32 if k == 32 else 16
    return k in (4, 8, 16, 32) and w % 4 == 0 and ch % v == 0 and ch // v <= 65535


def _wgrad_valu_taken(c):
    """dconv.hip:1475-1483 — cpg 4 / 8, (groups * cpg / 2) % 4 == 0, and groups % 4 == 0 at 4 channels per group"""
    nb, ch, h, w, groups, k = _g3(c)
    return k in (4, 8) and (groups * (k // 2)) % 4 == 0 and (k != 4 or groups % 4 == 0)


def r_g3b_wgrad_f32(c):
    """ops.gconv3x3_bwd_weight (fp32 branch) -> g3b.hip:671"""
    return c.ep == "g3_wgrad" and c.storage == "f32" and c.g3b and g3b_f32_supported(c, True)


def r_g3b_wgrad_bf16(c):
    """ops.gconv3x3_bwd_weight (bf16 branch, g3b) -> g3b.hip:619"""
    return c.ep == "g3_wgrad" and c.storage == "bf16" and c.g3b and c.precision == "medium" and g3b_supported(c)


def r_gconv3_wgrad_bf16(c):
    """ops.gconv3x3_bwd_weight (bf16 branch, g3b not taken) -> gemm.hip:1796: the MFMA kernel on bf16 tensors, no fallback"""
    return c.ep == "g3_wgrad" and c.storage == "bf16" and not r_g3b_wgrad_bf16(c) and _wgrad_mfma_taken(c)


def r_gconv3_wgrad_mfma(cpg):
    def pred(c):
        """gemm.hip:1817 -> dconv.hip:1432"""
        return (c.ep == "g3_wgrad" and c.storage == "f32" and not r_g3b_wgrad_f32(c) and _g3(c)[5] == cpg and _wgrad_mfma_taken(c))
    return pred


def r_gconv3_wgrad_valu(cpg):
    def pred(c):
        """gemm.hip:1822 -> dconv.hip:1472"""
        return (c.ep == "g3_wgrad" and c.storage == "f32" and not r_g3b_wgrad_f32(c) and _g3(c)[5] == cpg
                and not _wgrad_mfma_taken(c) and _wgrad_valu_taken(c))
    return pred


def r_b_wgrad3(c):
    """gemm.hip:1825-1846 — launch_gemm<A_KCONTIG, B_WGRAD3, E_SLAB>: cpg <= 32 and neither dedicated kernel took the shape"""
    return (c.ep == "g3_wgrad" and c.storage == "f32" and not r_g3b_wgrad_f32(c) and _g3(c)[5] <= 32
            and not _wgrad_mfma_taken(c) and not _wgrad_valu_taken(c))


def _dshape(c):
    nb, cin, cout, h, w, ks, stride, pad, groups = c.shape
    return nb, cin, cout, h, w, ks, stride, pad, groups


def r_c1in_conv42(c):
    """dconv.hip:363 + :194 — Conv2d(1, C, 4, 2, 1) on even planes with Wo % 4 == 0"""
    if c.ep != "d_fwd" or c.storage != "f32":
        return False
    nb, cin, cout, h, w, ks, stride, pad, groups = _dshape(c)
    return cin == 1 and groups == 1 and (ks, stride, pad) == (4, 2, 1) and h % 2 == 0 and w % 2 == 0 and (w // 2) % 4 == 0


def r_dconv_fwd(ks, stride, ocb):
    def pred(c):
        """dconv.hip:374-376 + :212-217 — the generic kernel, OCB output channels per thread by Cout / groups % 8, % 4"""
        if c.ep != "d_fwd" or c.storage != "f32" or r_c1in_conv42(c):
            return False
        nb, cin, cout, h, w, k, s, pad, groups = _dshape(c)
        og = cout // groups
        return (k, s) == (ks, stride) and (8 if og % 8 == 0 else 4 if og % 4 == 0 else 1) == ocb
    return pred


def r_c1in_conv31_flip(c):
    """dconv.hip:389 + :194 — the data gradient of Conv2d(C, 1, 3, 1, 1): W % 4 == 0"""
    if c.ep != "d_dgrad" or c.storage != "f32":
        return False
    nb, cin, cout, h, w, ks, stride, pad, groups = _dshape(c)
    return cout == 1 and groups == 1 and (ks, pad) == (3, 1) and w % 4 == 0


def r_dconv_dgrad(ks, ocb):
    def pred(c):
        """dconv.hip:403-404 — the generic kernel with transposed, flipped weights; OCB by Cin / groups"""
        if c.ep != "d_dgrad" or c.storage != "f32" or r_c1in_conv31_flip(c):
            return False
        nb, cin, cout, h, w, k, s, pad, groups = _dshape(c)
        ig = cin // groups
        return s == 1 and k == ks and (8 if ig % 8 == 0 else 4 if ig % 4 == 0 else 1) == ocb
    return pred


def c1_wgrad_mfma_parts(flip, nb, ch, h, w):
    """dconv.hip:1398-1406 — (tiles, parts), None where the kernel declines the shape: C % 64, Wb % 4, odd planes"""
    hb, wb = (h, w) if flip else (h // 2, w // 2)
    if (not flip and (h % 2 or w % 2)) or ch % 64 or wb % 4 or ch // 64 > 65535:
        return None
    total = nb * cdiv(wb, 32) * cdiv(hb, 4)
    parts = cdiv(1024, ch // 64)
    if parts > total // 2:
        parts = max(total // 2, 1)
    return total, parts


def _c1_flip1_shape(c):
    nb, cin, cout, h, w, ks, stride, pad, groups = _dshape(c)
    return (ks, stride, pad, groups, cout) == (3, 1, 1, 1, 1)


def _c1_flip0_shape(c):
    nb, cin, cout, h, w, ks, stride, pad, groups = _dshape(c)
    return (ks, stride, pad, groups, cin) == (4, 2, 1, 1, 1)


def r_c1_wgrad_mfma(flip):
    def pred(c):
        """dconv.hip:414 (flip 1) / :422 (flip 0) + :1399-1408 — declines a workspace short of parts slabs"""
        if c.ep != "d_wgrad" or c.storage != "f32" or not (_c1_flip1_shape(c) if flip else _c1_flip0_shape(c)):
            return False
        nb, cin, cout, h, w, ks, stride, pad, groups = _dshape(c)
        ch = cin if flip else cout
        tp = c1_wgrad_mfma_parts(flip, nb, ch, h, w)
        return tp is not None and tp[1] * ch * ks * ks * 4 <= c.ws
    return pred


def r_c1conv3_wgrad(c):
    """dconv.hip:418 + c1conv.hip:85-88 — Cin >= 16, one slab per 16 x 64 tile must fit the workspace"""
    if c.ep != "d_wgrad" or c.storage != "f32" or not _c1_flip1_shape(c) or r_c1_wgrad_mfma(1)(c):
        return False
    nb, cin, cout, h, w, ks, stride, pad, groups = _dshape(c)
    return cin >= 16 and nb <= 65535 and nb * cdiv(w, 64) * cdiv(h, 16) * cin * 9 * 4 <= c.ws


def dconv_wgrad_parts(c):
    """dconv.hip:426-459 — (tiles, parts) of the generic weight-gradient kernel under the call's workspace"""
    nb, cin, cout, h, w, ks, stride, pad, groups = _dshape(c)
    ig, og = cin // groups, cout // groups
    ob = 4 if og % 4 == 0 else 1
    igc, ogc = min(ig, 32), min(og, 64)
    if ob == 1 and ogc > 16:
        ogc = 16
    units = (ogc // ob) * igc
    gb = max(1, min(groups, 32 // igc, 64 // ogc, 256 // units))
    gy = cdiv(groups, gb) * cdiv(og, ogc) * cdiv(ig, igc)
    total = nb * cdiv(_out_size(w, ks, stride, pad), 32) * cdiv(_out_size(h, ks, stride, pad), 8)
    parts = min(max(1024 // gy, 1), total)
    while parts > 1 and parts * cout * ig * ks * ks * 4 > c.ws:
        parts -= 1
    return total, parts


def r_dconv_wgrad(ks, stride, ob):
    def pred(c):
        """dconv.hip:426-487 — what the three one-channel kernels leave; OB = 4 when Cout / groups % 4 == 0, else 1"""
        if c.ep != "d_wgrad" or c.storage != "f32" or r_c1_wgrad_mfma(1)(c) or r_c1conv3_wgrad(c) or r_c1_wgrad_mfma(0)(c):
            return False
        nb, cin, cout, h, w, k, s, pad, groups = _dshape(c)
        return (k, s) == (ks, stride) and (4 if (cout // groups) % 4 == 0 else 1) == ob
    return pred


def r_dconv_bf16(ep, first=False):
    def pred(c):
        """ops.dconv_fwd, ops.dconv_bwd_data, ops.dconv_bwd_weight -> dconv.hip:496-531: the first layer (fp32 frame -> bf16), the output
        convolution (bf16 -> fp32), its data gradient (-> bf16) and their weight gradients (the big tensor bf16)"""
        if c.ep != ep or c.storage != "bf16":
            return False
        nb, cin, cout, h, w, ks, stride, pad, groups = _dshape(c)
        if ep == "d_fwd" and first:           # bf16out: c1in_conv<4, 2, bf16>
            return cin == 1 and groups == 1 and (ks, stride, pad) == (4, 2, 1) and h % 2 == 0 and w % 2 == 0 and (w // 2) % 4 == 0
        if ep == "d_fwd":                     # bf16in: dconv_fwd_kernel<3, 1, ., bf16, float>
            return cin > 1 and groups == 1 and (ks, stride, pad) == (3, 1, 1)
        if ep == "d_dgrad":                   # bf16out: c1in_conv<3, 1, flip, bf16>
            return cout == 1 and groups == 1 and (ks, pad) == (3, 1) and w % 4 == 0
        flip = 0 if cin == 1 else 1
        if not (_c1_flip1_shape(c) if flip else _c1_flip0_shape(c)):
            return False
        tp = c1_wgrad_mfma_parts(flip, nb, cin if flip else cout, h, w)
        return tp is not None
    return pred


def r_simple(ep):
    def pred(c):
        """gemm.hip:1730 / :1748 / :1771 (Winograd off: ops.conv4x4s2_down / _up / _wgrad fall through to the gather GEMMs) and gemm.hip:1868 /
        :1907 (the flat-shift 4x4 stride-1 GEMMs: the channels read must be a multiple of 16, gemm.hip:1875)"""
        if c.ep != ep or c.storage != "f32":
            return False
        if ep == "s1_fwd":
            return c.shape[1] % 16 == 0
        if ep == "s1_dgrad":
            return c.shape[2] % 16 == 0
        return True
    return pred


ROUTES = collections.OrderedDict([
    ("gconv3p<4>", r_gconv3p(4)), ("gconv3p<8>", r_gconv3p(8)),
    ("gconv3<4,1>", r_gconv3(4, "f32")), ("gconv3<8,1>", r_gconv3(8, "f32")),
    ("gconv3_mfma<16>", r_gconv3_mfma(16, "f32")), ("gconv3_mfma<32>", r_gconv3_mfma(32, "f32")),
    ("g3b_fwd_f32", r_g3b_fwd_f32),
    ("gconv3<.,1,bf16>", r_gconv3(None, "bf16")), ("gconv3_mfma<.,bf16>", r_gconv3_mfma(None, "bf16")),
    ("g3b_fwd_bf16", r_g3b_fwd_bf16),
    ("gconv3_wgrad_mfma<4>", r_gconv3_wgrad_mfma(4)), ("gconv3_wgrad_mfma<8>", r_gconv3_wgrad_mfma(8)),
    ("gconv3_wgrad_mfma<16>", r_gconv3_wgrad_mfma(16)), ("gconv3_wgrad_mfma<32>", r_gconv3_wgrad_mfma(32)),
    ("gconv3_wgrad_valu<4,2>", r_gconv3_wgrad_valu(4)), ("gconv3_wgrad_valu<8,2>", r_gconv3_wgrad_valu(8)),
    ("B_WGRAD3", r_b_wgrad3),
    ("g3b_bwd_weight_f32", r_g3b_wgrad_f32), ("g3b_bwd_weight_bf16", r_g3b_wgrad_bf16),
    ("gconv3x3_bwd_weight_bf16", r_gconv3_wgrad_bf16),
    ("c1in_conv<4,2>", r_c1in_conv42),
    ("dconv_fwd<4,2,8>", r_dconv_fwd(4, 2, 8)), ("dconv_fwd<4,2,4>", r_dconv_fwd(4, 2, 4)),
    ("dconv_fwd<3,1,1>", r_dconv_fwd(3, 1, 1)), ("dconv_fwd<3,1,4>", r_dconv_fwd(3, 1, 4)), ("dconv_fwd<3,1,8>", r_dconv_fwd(3, 1, 8)),
    ("dconv_fwd<4,1,1>", r_dconv_fwd(4, 1, 1)),
    ("c1in_conv<3,1,flip>", r_c1in_conv31_flip),
    ("dconv_dgrad<3,8>", r_dconv_dgrad(3, 8)), ("dconv_dgrad<3,4>", r_dconv_dgrad(3, 4)), ("dconv_dgrad<4,1>", r_dconv_dgrad(4, 1)),
    ("c1_wgrad_mfma<flip0>", r_c1_wgrad_mfma(0)), ("c1_wgrad_mfma<flip1>", r_c1_wgrad_mfma(1)),
    ("c1conv3_wgrad", r_c1conv3_wgrad),
    ("dconv_wgrad<3,1,4>", r_dconv_wgrad(3, 1, 4)), ("dconv_wgrad<3,1,1>", r_dconv_wgrad(3, 1, 1)),
    ("dconv_wgrad<4,2,4>", r_dconv_wgrad(4, 2, 4)), ("dconv_wgrad<4,2,1>", r_dconv_wgrad(4, 2, 1)),
    ("dconv_wgrad<4,1,4>", r_dconv_wgrad(4, 1, 4)), ("dconv_wgrad<4,1,1>", r_dconv_wgrad(4, 1, 1)),
    ("dconv_fwd_bf16out", r_dconv_bf16("d_fwd", True)), ("dconv_fwd_bf16in", r_dconv_bf16("d_fwd")),
    ("dconv_bwd_data_bf16out", r_dconv_bf16("d_dgrad")), ("c1_wgrad_bf16", r_dconv_bf16("d_wgrad")),
    ("conv4x4s2_down", r_simple("s2_down")), ("conv4x4s2_up", r_simple("s2_up")), ("conv4x4s2_wgrad", r_simple("s2_wgrad")),
    ("conv4x4s1_fwd", r_simple("s1_fwd")), ("conv4x4s1_dgrad", r_simple("s1_dgrad")), ("conv4x4s1_bwd_weight", r_simple("s1_wgrad")),
])


def routes_of(c):
    """every label whose predicate holds for the call: exactly one for a call the library serves"""
    return [k for k, p in ROUTES.items() if p(c)]


# ------------------------------------------------------------------------------------------------------------------- cases
# ws: None (the default workspace), or ("slabs", p): room for p copies of the weight gradient, handed to the entry point itself
Case = collections.namedtuple("Case", "route ep shape storage ws note")


def _c(route, ep, shape, storage="f32", ws=None, note=""):
    return Case(route, ep, tuple(shape), storage, ws, note)


def ws_bytes(case):
    if case.ws is None:
        return None
    g = geometry(case.ep, case.shape)
    return case.ws[1] * g.w[0] * g.w[1] * g.w[2] * g.w[3] * 4


def ctx(case, cus=256, **kw):
    return Ctx(case.ep, case.shape, case.storage, cus=cus, ws=ws_bytes(case), **kw)


def wgrad_trips(case):
    """(tiles, parts) of a split-K weight-gradient case under its workspace: every block walks tiles b, b + parts, ..."""
    c = ctx(case._replace(storage="f32"))      # the bf16 forms run the same kernels on the same grids
    budget = c.ws
    if case.ep == "d_wgrad":
        for flip in (1, 0):
            if r_c1_wgrad_mfma(flip)(c):
                nb, cin, cout, h, w = case.shape[:5]
                return c1_wgrad_mfma_parts(flip, nb, cin if flip else cout, h, w)
        return dconv_wgrad_parts(c)
    nb, ch, h, w, groups, k = _g3(c)
    slab = ch * k * 9 * 4
    if r_b_wgrad3(c):                                          # gemm.hip:1836-1842: (K stages of 16 pixels, splits)
        stages = cdiv(nb * h * w, 16)
        want = min(cdiv(1024, groups * cdiv(k * 9, 128)), stages)
        while want > 1 and want * slab > budget:
            want -= 1
        return stages, cdiv(nb * h * w, cdiv(stages, want) * 16)
    if _wgrad_mfma_taken(c):                                   # dconv.hip:1440-1445
        total = nb * cdiv(w, 16) * cdiv(h, 8)
        parts = cdiv(1536, ch // (32 if k == 32 else 16))
        if parts > total // 2:
            parts = max(total // 2, 1)
    else:                                                      # dconv.hip:1484-1491
        total = nb * cdiv(w, 64) * cdiv(h, 8)
        parts = min(max(768 // (groups * (k // 2) // 4), 1), total)
    while parts > 1 and parts * slab > budget:
        parts -= 1
    return total, parts


def multitrip_cases(cus):
    return [_c("gconv3p<4>", "g3_fwd", gconv3p_multitrip_shape(4, cus), note="three trips"),
            _c("gconv3p<8>", "g3_dgrad", gconv3p_multitrip_shape(8, cus), note="three trips")]


def cases(cus=256):
    f, d, wg = "g3_fwd", "g3_dgrad", "g3_wgrad"
    t = []
    # ---- grouped 3x3 forward / data gradient, fp32 (dconv.hip gconv3x3_fwd_impl)
    for r, k in (("gconv3p<4>", 4), ("gconv3p<8>", 8)):
        t += [_c(r, f, (1, 8 * k, 16, 64, 8), note="one exact 16 x 64 tile"),
              _c(r, d, (2, 6 * k, 17, 68, 6), note="one tile + one row + one 16-byte piece, 6 groups"),
              _c(r, f, (1, 8 * k, 1, 4, 8), note="a single row, one piece"),
              _c(r, d, (3, 32 * k, 5, 132, 32), note="three tiles across, 32 groups")]
    t += multitrip_cases(cus)
    for r, k in (("gconv3<4,1>", 4), ("gconv3<8,1>", 8)):
        t += [_c(r, f, (1, 8 * k, 16, 33, 8), note="one 16 x 32 tile + one column"),
              _c(r, d, (2, 6 * k, 17, 31, 6), note="a partial tile, one row below"),
              _c(r, f, (2, 32 * k, 1, 67, 32), note="a single row")]
    for r, k in (("gconv3_mfma<16>", 16), ("gconv3_mfma<32>", 32)):
        t += [_c(r, f, (1, 8 * k, 16, 16, 8), note="one exact 16 x 16 tile"),
              _c(r, d, (2, 6 * k, 17, 17, 6), note="2 x 2 partial tiles"),
              _c(r, f, (1, 8 * k, 1, 35, 8), note="a single row")]
    t += [_c("g3b_fwd_f32", f, (2, 128, 4, 96, 8), note="one strip"), _c("g3b_fwd_f32", d, (1, 96, 28, 96, 6), note="seven strips"),
          _c("g3b_fwd_f32", d, (1, 512, 24, 96, 32), note="32 groups")]
    # ---- bf16 storage
    t += [_c("gconv3<.,1,bf16>", f, (2, 32, 17, 33, 8), "bf16"), _c("gconv3<.,1,bf16>", d, (1, 48, 16, 68, 6), "bf16"),
          _c("gconv3_mfma<.,bf16>", f, (2, 128, 17, 17, 8), "bf16"), _c("gconv3_mfma<.,bf16>", d, (1, 192, 9, 20, 6), "bf16")]
    for shape in ((1, 32, 5, 384, 8), (2, 48, 2, 192, 6), (1, 128, 4, 96, 8), (2, 128, 28, 96, 8), (1, 256, 8, 48, 8),
                  (1, 192, 40, 48, 6), (2, 256, 12, 24, 8), (1, 1024, 36, 24, 32)):
        t += [_c("g3b_fwd_bf16", f if shape[2] % 8 else d, shape, "bf16")]
    # ---- grouped 3x3 weight gradient
    for k in (4, 8, 16, 32):
        r = "gconv3_wgrad_mfma<%d>" % k
        t += [_c(r, wg, (1, 8 * k, 8, 16, 8), note="one exact 8 x 16 tile"),
              _c(r, wg, (2, 8 * k, 9, 20, 8), note="one tile + one row + one piece"),
              _c(r, wg, (1, 32 * k, 3, 36, 32), note="32 groups"),
              _c(r, wg, (2, 8 * k, 50, 20, 8), ws=("slabs", 1), note="28 tiles on one block"),
              _c(r, wg, (2, 8 * k, 50, 20, 8), ws=("slabs", 3), note="28 tiles on three blocks: 10, 9, 9")]
    t += [_c("gconv3_wgrad_mfma<8>", wg, (2, 96, 9, 20, 12), note="12 groups")]
    for k in (4, 8):
        r = "gconv3_wgrad_valu<%d,2>" % k
        t += [_c(r, wg, (1, 8 * k, 8, 63, 8), note="one 8 x 64 tile less a column"),
              _c(r, wg, (2, 8 * k, 9, 70, 8), note="2 x 2 partial tiles"),
              _c(r, wg, (2, 8 * k, 50, 37, 8), ws=("slabs", 1), note="14 tiles on one block"),
              _c(r, wg, (2, 8 * k, 50, 37, 8), ws=("slabs", 3), note="14 tiles on three blocks: 5, 5, 4")]
    t += [_c("gconv3_wgrad_valu<4,2>", wg, (1, 128, 9, 33, 32), note="32 groups"),
          _c("gconv3_wgrad_valu<8,2>", wg, (2, 40, 9, 36, 5), note="C % 16 != 0 keeps W % 4 == 0 off the MFMA kernel")]
    t += [_c("B_WGRAD3", wg, (2, 128, 9, 17, 8), note="16 per group, W % 4 != 0"),
          _c("B_WGRAD3", wg, (1, 192, 17, 33, 6), note="32 per group, 6 groups"),
          _c("B_WGRAD3", wg, (2, 24, 16, 21, 6), note="4 per group, groups % 4 != 0"),
          _c("B_WGRAD3", wg, (2, 24, 12, 20, 6), note="4 per group, 6 groups: C % 16 != 0 although W % 4 == 0"),
          _c("B_WGRAD3", wg, (2, 24, 12, 24, 6), note="W % 8 == 0: the loader's row runs of eight pixels (gemm.hip:772)"),
          _c("B_WGRAD3", wg, (1, 512, 5, 18, 32), note="32 groups"),
          _c("B_WGRAD3", wg, (2, 128, 30, 33, 8), ws=("slabs", 2), note="1980 pixels over two splits")]
    t += [_c("g3b_bwd_weight_f32", wg, (2, 128, 4, 96, 8), note="one strip"), _c("g3b_bwd_weight_f32", wg, (1, 96, 28, 96, 6)),
          _c("g3b_bwd_weight_f32", wg, (1, 256, 8, 48, 8)), _c("g3b_bwd_weight_f32", wg, (1, 192, 40, 48, 6)),
          _c("g3b_bwd_weight_f32", wg, (2, 256, 12, 24, 8)), _c("g3b_bwd_weight_f32", wg, (1, 1024, 36, 24, 32))]
    for shape in ((1, 32, 5, 384, 8), (2, 48, 2, 192, 6), (1, 128, 20, 96, 8), (1, 256, 40, 48, 8), (2, 192, 12, 24, 6)):
        t += [_c("g3b_bwd_weight_bf16", wg, shape, "bf16")]
    t += [_c("gconv3x3_bwd_weight_bf16", wg, (2, 32, 9, 20, 8), "bf16"), _c("gconv3x3_bwd_weight_bf16", wg, (1, 64, 17, 36, 8), "bf16"),
          _c("gconv3x3_bwd_weight_bf16", wg, (2, 96, 8, 16, 6), "bf16"), _c("gconv3x3_bwd_weight_bf16", wg, (1, 256, 9, 12, 8), "bf16")]
    # ---- wfae_dconv_*: (N, Cin, Cout, H, W, ks, stride, pad, groups)
    t += [_c("c1in_conv<4,2>", "d_fwd", (2, 1, 16, 10, 24, 4, 2, 1, 1)), _c("c1in_conv<4,2>", "d_fwd", (1, 1, 5, 2, 8, 4, 2, 1, 1)),
          _c("dconv_fwd<4,2,8>", "d_fwd", (2, 1, 16, 10, 22, 4, 2, 1, 1), note="Wo % 4 != 0: the generic first layer"),
          _c("dconv_fwd<4,2,4>", "d_fwd", (1, 3, 4, 18, 66, 4, 2, 1, 1)),
          _c("dconv_fwd<3,1,1>", "d_fwd", (2, 24, 1, 9, 33, 3, 1, 1, 1), note="Cout = 1"),
          _c("dconv_fwd<3,1,1>", "d_fwd", (1, 6, 3, 8, 32, 3, 1, 1, 3), note="3 groups of 2 -> 1"),
          _c("dconv_fwd<3,1,4>", "d_fwd", (2, 4, 8, 17, 40, 3, 1, 1, 2)), _c("dconv_fwd<3,1,8>", "d_fwd", (1, 5, 8, 5, 70, 3, 1, 1, 1)),
          _c("dconv_fwd<4,1,1>", "d_fwd", (2, 8, 1, 9, 12, 4, 1, 1, 1), note="the PatchGAN head")]
    t += [_c("c1in_conv<3,1,flip>", "d_dgrad", (2, 24, 1, 9, 36, 3, 1, 1, 1)), _c("c1in_conv<3,1,flip>", "d_dgrad", (1, 64, 1, 1, 4, 3, 1, 1, 1)),
          _c("dconv_dgrad<3,8>", "d_dgrad", (2, 24, 1, 9, 33, 3, 1, 1, 1), note="W % 4 != 0: the generic data gradient"),
          _c("dconv_dgrad<3,4>", "d_dgrad", (1, 8, 6, 17, 40, 3, 1, 1, 2)),
          _c("dconv_dgrad<4,1>", "d_dgrad", (2, 3, 8, 10, 13, 4, 1, 1, 1))]
    t += [_c("c1_wgrad_mfma<flip1>", "d_wgrad", (1, 64, 1, 12, 32, 3, 1, 1, 1), note="three tiles on one block"),
          _c("c1_wgrad_mfma<flip1>", "d_wgrad", (1, 128, 1, 27, 36, 3, 1, 1, 1), note="14 tiles on 7 blocks, partial tiles"),
          _c("c1_wgrad_mfma<flip0>", "d_wgrad", (1, 1, 64, 24, 64, 4, 2, 1, 1), note="three tiles on one block"),
          _c("c1_wgrad_mfma<flip0>", "d_wgrad", (3, 1, 64, 10, 72, 4, 2, 1, 1), note="12 tiles, partial"),
          _c("c1conv3_wgrad", "d_wgrad", (2, 24, 1, 17, 66, 3, 1, 1, 1), note="C % 64 != 0"),
          _c("c1conv3_wgrad", "d_wgrad", (1, 64, 1, 16, 63, 3, 1, 1, 1), note="W % 4 != 0"),
          _c("dconv_wgrad<3,1,1>", "d_wgrad", (2, 24, 1, 17, 66, 3, 1, 1, 1), ws=("slabs", 1),
             note="c1conv3_wgrad's partials do not fit: dconv.hip:420"),
          _c("dconv_wgrad<3,1,1>", "d_wgrad", (2, 64, 1, 16, 64, 3, 1, 1, 1), ws=("slabs", 1),
             note="c1_wgrad_mfma declines a short workspace, then c1conv3_wgrad does"),
          _c("dconv_wgrad<3,1,1>", "d_wgrad", (2, 8, 1, 9, 33, 3, 1, 1, 1), note="Cin < 16"),
          _c("dconv_wgrad<3,1,4>", "d_wgrad", (2, 6, 8, 50, 20, 3, 1, 1, 2), ws=("slabs", 1), note="14 tiles on one block"),
          _c("dconv_wgrad<3,1,4>", "d_wgrad", (2, 6, 8, 50, 20, 3, 1, 1, 2), ws=("slabs", 3), note="14 tiles on three blocks"),
          _c("dconv_wgrad<3,1,4>", "d_wgrad", (1, 80, 8, 9, 33, 3, 1, 1, 1), note="three input-channel chunks"),
          _c("dconv_wgrad<4,2,4>", "d_wgrad", (2, 1, 16, 10, 22, 4, 2, 1, 1), note="the first layer on odd Wo"),
          _c("dconv_wgrad<4,2,4>", "d_wgrad", (2, 3, 4, 100, 40, 4, 2, 1, 1), ws=("slabs", 3), note="14 tiles on three blocks"),
          _c("dconv_wgrad<4,2,1>", "d_wgrad", (2, 3, 2, 18, 66, 4, 2, 1, 1)),
          _c("dconv_wgrad<4,1,4>", "d_wgrad", (2, 3, 8, 10, 13, 4, 1, 1, 1)),
          _c("dconv_wgrad<4,1,1>", "d_wgrad", (2, 8, 1, 9, 35, 4, 1, 1, 1), note="the PatchGAN head"),
          _c("dconv_wgrad<4,1,1>", "d_wgrad", (2, 8, 1, 51, 21, 4, 1, 1, 1), ws=("slabs", 3), note="14 tiles on three blocks")]
    t += [_c("dconv_fwd_bf16out", "d_fwd", (2, 1, 16, 10, 24, 4, 2, 1, 1), "bf16"),
          _c("dconv_fwd_bf16in", "d_fwd", (2, 24, 1, 9, 33, 3, 1, 1, 1), "bf16"),
          _c("dconv_bwd_data_bf16out", "d_dgrad", (2, 24, 1, 9, 36, 3, 1, 1, 1), "bf16"),
          _c("c1_wgrad_bf16", "d_wgrad", (1, 64, 1, 12, 32, 3, 1, 1, 1), "bf16", note="flip 1, three tiles on one block"),
          _c("c1_wgrad_bf16", "d_wgrad", (3, 1, 64, 10, 72, 4, 2, 1, 1), "bf16", note="flip 0")]
    # ---- gather GEMMs (N, Chi, Clo, Hlo, Wlo) and flat-shift GEMMs (N, Cin, Cout, H, W, pad)
    for ep in ("s2_down", "s2_up", "s2_wgrad"):
        r = "conv4x4" + ep
        t += [_c(r, ep, (2, 16, 32, 8, 8)), _c(r, ep, (1, 3, 8, 5, 7), note="odd planes, 3 channels"),
              _c(r, ep, (3, 24, 40, 4, 12)), _c(r, ep, (1, 64, 130, 9, 8), note="M = 130: a partial row tile")]
    for ep, r in (("s1_fwd", "conv4x4s1_fwd"), ("s1_dgrad", "conv4x4s1_dgrad"), ("s1_wgrad", "conv4x4s1_bwd_weight")):
        t += [_c(r, ep, (2, 16, 16, 8, 8, 1)), _c(r, ep, (1, 32, 16, 7, 9, 1), note="odd planes"),
              _c(r, ep, (2, 64, 80, 6, 11, 2), note="pad 2, K = 1024: the in-register split")]
    return t


CASES = cases(256)


def kinds_of(case):
    """exact always; the real-valued flavours unless a weight gradient sums more than WGRAD_REAL_PIXELS pixels, or the case is a
    multi-trip grid (judged by the exact check)"""
    g = geometry(case.ep, case.shape)
    if case.note == "three trips":
        return ("exact",)
    if g.op == "wgrad" and g.dy[0] * g.dy[2] * g.dy[3] > WGRAD_REAL_PIXELS:
        return ("exact",)
    return KINDS


def case_id(case):
    return "%s-%s-%s%s%s" % (case.route, case.ep, "x".join(str(v) for v in case.shape), "-bf16" if case.storage == "bf16" else "",
                             "" if case.ws is None else "-ws%d" % case.ws[1])


if __name__ == "__main__":      # python -m tests.conv_ref: the table, route by route (profiles/r06_conv_route_cases.txt)
    for label in ROUTES:
        print(label)
        for c in CASES:
            if c.route == label:
                print("    %-9s %-34s %-5s %-8s %-20s %s" % (c.ep, "x".join(str(v) for v in c.shape), c.storage,
                                                             "" if c.ws is None else "ws=%d" % c.ws[1], "+".join(kinds_of(c)), c.note))
