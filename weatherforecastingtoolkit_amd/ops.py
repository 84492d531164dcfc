"""Tensor-level launch wrappers over the libwfae.so C ABI (no autograd here).

torch is used for device memory, the current HIP stream and nothing else:
every arithmetic operation below is a hand-written gfx950 kernel reached
through ctypes.  All tensors must be CUDA(HIP) fp32 and contiguous (NCHW).
"""
from __future__ import annotations

import ctypes
import math
import os

import numpy as np
import torch

from . import _lib

_WS_DEFAULT = int(os.environ.get("WFAE_WORKSPACE_MB", "512")) << 20
_ws = {}


def _stream():
    return torch.cuda.current_stream().cuda_stream


# Optional per-launch timing with events on the launch stream (bench.py's
# roofline read-out): name -> [(start_evt, end_evt, algorithmic flops, algorithmic bytes)]
_prof = None


def profile_start():
    global _prof
    _prof = {}


PEAK_HBM = 8.0e12          # MI355X_MICROARCH.md
PEAK_FP32_MFMA = 157.3e12  # v_mfma_f32_32x32x2_f32 = the fp32 vector rate
PEAK_BF16_MFMA = 2500.0e12 # dense bf16


def profile_stop():
    """-> {name: (calls, total_ms, flops, bytes, ideal_ms, mfma_ms, hbm_ms)}; synchronises the device.  ideal_ms = sum over
    the launches of max(algorithmic bytes / HBM peak, algorithmic FLOPs / peak of the matrix instruction that launch runs on);
    mfma_ms / hbm_ms: the two terms summed on their own (which roof binds the label's launches as a whole)"""
    global _prof
    rec, _prof = _prof, None
    torch.cuda.synchronize()
    out = {}
    for k, lst in (rec or {}).items():
        ms = sum(a.elapsed_time(b) for a, b, _, _, _ in lst)
        out[k] = (len(lst), ms, sum(f for _, _, f, _, _ in lst), sum(b for _, _, _, b, _ in lst),
                  1e3 * sum(max(b / PEAK_HBM, f / pk) for _, _, f, b, pk in lst),
                  1e3 * sum(f / pk for _, _, f, _, pk in lst), 1e3 * sum(b / PEAK_HBM for _, _, _, b, _ in lst))
    return out


def _default_peak():
    return PEAK_BF16_MFMA if _lib.load().wfae_get_matmul_precision() == 1 else PEAK_FP32_MFMA


def _gemm_peak(m, k):
    """FLOP/s ceiling of the instruction a plain GEMM-family launch (1x1 / linear) runs on: bf16 operands at 'medium'; at
    fp32 precision the exact three-plane split (six bf16 products per fp32 product) for K >= 128, M >= 64 (gemm.hip
    launch_gemm_v), else v_mfma_f32_32x32x2_f32.  Work is counted in fp32-equivalent FLOPs."""
    if _lib.load().wfae_get_matmul_precision() == 1:
        return PEAK_BF16_MFMA
    if _SPLIT_GEMM and k >= 128 and m >= 64:
        return PEAK_BF16_MFMA / 6
    return PEAK_FP32_MFMA


def _call(name, flops, nbytes, *args, label=None, peak=None):
    if _prof is None:
        return _lib.call(name, *args)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _lib.call(name, *args)
    e1.record()
    if peak is None:
        fn = _PEAK_OF.get(name)
        peak = fn(args) if fn is not None else PEAK_FP32_MFMA
    _prof.setdefault(label or name, []).append((e0, e1, flops, nbytes, peak))


def _planes_peak(planes):
    return PEAK_BF16_MFMA / 6 if planes == 3 else PEAK_BF16_MFMA


def _peak_table():
    """matrix-instruction ceiling per GEMM-family entry point from its C arguments, found by the NAMES include/wfae.h gives
    them: a name the header does not have raises here, at import, not at the first profiled launch"""
    decls = _lib.parse_header()

    def at(entry, name):
        if name not in decls[entry][2]:
            raise _lib.WfaeError(f"include/wfae.h: {entry} has no argument named {name}")
        return decls[entry][2].index(name)

    t = {}
    for mk, entries in ((("Cout", "Cin"), "conv1x1_fwd conv1x1_fwd_stats conv1x1_fwd_bnact"), (("Cin", "Cout"), "conv1x1_bwd_data"),
                        (("Out", "In"), "linear_fwd"), (("In", "Out"), "linear_bwd_data linear_bwd_data_splitk"),
                        (("Out", "B"), "linear_bwd_weight linear_bwd_weight_splitk")):
        for e in entries.split():
            t["wfae_" + e] = lambda a, i=at("wfae_" + e, mk[0]), j=at("wfae_" + e, mk[1]): _gemm_peak(a[i], a[j])
    # weight gradients: M = Cout, or Cin when the roles are swapped (Cin < Cout and Cin < 128); K = the pixels
    for e in ("wfae_conv1x1_bwd_weight", "wfae_conv1x1_bwd_weight_bnact"):
        t[e] = lambda a, i=at(e, "Cin"), j=at(e, "Cout"): _gemm_peak(a[i] if (a[i] < a[j] and a[i] < 128) else a[j], 1 << 20)
    for e in ("wfae_wino_gemm_down_split", "wfae_wino_gemm_up_split", "wfae_wino_gemm_wgrad_split", "wfae_split_gemm"):
        t[e] = lambda a, i=at(e, "planes"): _planes_peak(a[i])
    for e in "wino_gemm_down wino_gemm_up wino_gemm_wgrad conv4x4s2_down conv4x4s2_up conv4x4s2_wgrad".split():
        t["wfae_" + e] = lambda a: _default_peak()
    for e in ("wfae_conv1x1_fwd_bf16", "wfae_conv1x1_bwd_data_bf16", "wfae_conv1x1_bwd_weight_bf16"):
        t[e] = lambda a: PEAK_BF16_MFMA
    t["wfae_conv4x4s1_fwd"] = lambda a, i=at("wfae_conv4x4s1_fwd", "Cout"), j=at("wfae_conv4x4s1_fwd", "Cin"): _gemm_peak(a[i], 16 * a[j])
    t["wfae_conv4x4s1_bwd_weight"] = lambda a, i=at("wfae_conv4x4s1_bwd_weight", "Cout"): _gemm_peak(a[i], 1 << 20)
    return t


_PEAK_OF = _peak_table()


def workspace(min_bytes: int = 0):
    """Per-(device, stream) scratch buffer handed to kernels that need one."""
    dev = torch.cuda.current_device()
    key = (dev, _stream())
    need = max(_WS_DEFAULT, int(min_bytes))
    buf = _ws.get(key)
    if buf is None or buf.numel() < need:
        buf = torch.empty(need, dtype=torch.uint8, device=f"cuda:{dev}")
        _ws[key] = buf
    return buf


def _chk(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.WfaeError("wfae kernels need device tensors (the HIP path has no CPU fallback)")
        if t.dtype != torch.float32:
            raise _lib.WfaeError(f"wfae kernels are fp32, got {t.dtype}")
        if not t.is_contiguous():
            raise _lib.WfaeError("wfae kernels need contiguous NCHW tensors")


BF16 = torch.bfloat16


def _chka(*ts):
    """like _chk for ACTIVATION tensors, which may be bf16 in the bf16-storage mode; all of them must agree -> the
    entry-point suffix ("" or "_bf16") and the element size"""
    dt = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.WfaeError("wfae kernels need device tensors (the HIP path has no CPU fallback)")
        if t.dtype not in (torch.float32, BF16):
            raise _lib.WfaeError(f"wfae activation tensors are fp32 or bf16, got {t.dtype}")
        if dt is not None and t.dtype != dt:
            raise _lib.WfaeError(f"activation tensors of one call must share a storage type ({dt} vs {t.dtype})")
        dt = t.dtype
        if not t.is_contiguous():
            raise _lib.WfaeError("wfae kernels need contiguous NCHW tensors")
    return ("_bf16", 2) if dt == BF16 else ("", 4)


# Activation storage (include/wfae.h "bf16 ACTIVATION STORAGE"): the dtype in which the convolution stacks keep their
# activations and activation gradients in HBM.  fp32 always at 'highest' / 'high' precision; at 'medium' bf16 unless
# WFAE_BF16_STORAGE=0 (then only the matrix-core operands are rounded, as in round 2).
_ACT_DTYPE = torch.float32


def activation_dtype():
    return _ACT_DTYPE


def set_activation_storage(dtype):
    """torch.float32 | torch.bfloat16 (bf16 needs 'medium' matmul precision)"""
    global _ACT_DTYPE
    if dtype not in (torch.float32, BF16):
        raise ValueError("activation storage is torch.float32 or torch.bfloat16")
    if dtype == BF16 and _lib.load().wfae_get_matmul_precision() != 1:
        raise _lib.WfaeError("bf16 activation storage needs set_float32_matmul_precision('medium')")
    _ACT_DTYPE = dtype


def to_f32(x):
    """bf16-stored tensor -> fp32 (the boundaries of the bf16-storage mode)"""
    if x.dtype == torch.float32:
        return x
    _chka(x)
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    _call("wfae_convert_bf16_to_f32", 0, 6 * x.numel(), _p(x), _p(y), x.numel(), _stream())
    return y


def to_bf16(x):
    if x.dtype == BF16:
        return x
    _chk(x)
    y = torch.empty(x.shape, dtype=BF16, device=x.device)
    _call("wfae_convert_f32_to_bf16", 0, 6 * x.numel(), _p(x), _p(y), x.numel(), _stream())
    return y


def to_dtype(x, dtype):
    return to_bf16(x) if dtype == BF16 else to_f32(x)


def _p(t):
    return None if t is None else t.data_ptr()


class StatRows:
    """partial BatchNorm sums written by a GEMM epilogue: `part` (float64) = sum[rows][C] ++ sumsq[rows][C]"""
    __slots__ = ("part", "rows")

    def __init__(self, part, rows):
        self.part, self.rows = part, rows


class StatParts:
    """fp64 partial BatchNorm sums left by a producer kernel: `part` = [splits][C][2] doubles (sum, sum of squares)"""
    __slots__ = ("part", "splits")

    def __init__(self, part, splits):
        self.part, self.splits = part, splits


def _rows_out(n, device):
    """an fp64 partial buffer of n doubles and the int a launcher writes its row / split count to (a HOST pointer) ->
    (part, count, the three C arguments (part, capacity, &count)); read count.value after the call"""
    part = torch.empty(n, dtype=torch.float64, device=device)
    count = ctypes.c_int(0)
    return part, count, (part.data_ptr(), n, ctypes.cast(ctypes.pointer(count), ctypes.c_void_p))


_NO_ROWS = (None, 0, None)


# ------------------------------------------------------------- 1x1 products
# y[n, M, p] = sum_k A[M, k] f(x[n, k, p]) (+ bias) (+ res): the forward convolution (A = w), its data gradient (A = w^T) and
# its weight gradient, on six kernel families.  conv1x1_route names the family of a product, _c1_launch / _c1_wgrad launch it.
#   c1r   csrc/c1r.hip   fp32 tensors, register-direct (activation HBM -> registers -> bf16 matrix core with exact three-plane
#                        operands, no LDS staging): the Bottleneck shapes with HW % 64 == 0, fp32 precision, split GEMMs on
#   c1rb  csrc/c1rb.hip  the same on bf16-stored tensors ('medium'), HW % 128 == 0; reads the fp32 weight
#   c1b   csrc/c1b.hip   bf16-stored tensors, LDS-tiled, takes the bf16 weight planes of c1b_weights
#   c1w   csrc/c1w.hip   weight gradients, both operands as K-contiguous rows (no LDS transpose)
#   gemm  csrc/gemm.hip  everything else; the library itself hands the narrowing products of the C >= 512 stages on fp32
#                        tensors to csrc/c1n.hip (set_c1n), see conv1x1_route
_C1R = _C1R_BNRED = _C1R_BNDX = _C1RB = _C1B = _C1W = True   # A/B switches, through the set_* functions below


def set_c1r(on):
    """A/B switch: the fp32 1x1 forward / data gradient of the C <= 256 stages on csrc/c1r.hip or on gemm.hip"""
    global _C1R
    _C1R = bool(on)


def set_c1r_bnred(on):
    """A/B switch: the reductions of the first BatchNorm's backward pass in the epilogue of the c1r data gradient (C <= 256)"""
    global _C1R_BNRED
    _C1R_BNRED = bool(on)


def set_c1r_bndx(on):
    """A/B switch: the second pass of the first BatchNorm's backward in the epilogue of a recomputed data gradient (c1r_bndx)
    or as bn_act_bwd_dx over the stored one"""
    global _C1R_BNDX
    _C1R_BNDX = bool(on)


def set_c1n(on):
    """A/B switch: the fp32 narrowing products of C >= 512 on csrc/c1n.hip (operands split once on their way into LDS) or on
    gemm.hip's in-register split"""
    _lib.call("wfae_set_c1n", int(bool(on)))


def set_c1wd(on):
    """A/B switch: the last 1x1 weight gradient and the data gradient in front of the third BatchNorm of a C <= 256 Bottleneck in
    one pass over dy (csrc/c1wd.hip) or as the pair c1w + c1r"""
    _lib.call("wfae_set_c1wd", int(bool(on)))


def set_c1ws(on):
    """A/B switch: the first 1x1 weight gradient and the sums of the first BatchNorm's backward of a C <= 256 Bottleneck in one
    pass over x (csrc/c1ws.hip) or as the pair c1r_bnred(store=False) + c1w"""
    _lib.call("wfae_set_c1ws", int(bool(on)))


def set_c1rb(on):
    """A/B switch: the bf16 1x1 forward / data gradient on csrc/c1rb.hip (register-direct) or on csrc/c1b.hip (LDS-tiled)"""
    global _C1RB
    _C1RB = bool(on)


def set_c1b(on):
    """A/B switch: bf16 1x1 forward / data gradient on csrc/c1b.hip or on the element-typed generic GEMM kernel"""
    global _C1B
    _C1B = bool(on)


def set_c1w(on):
    """A/B switch: the 1x1 weight gradients on csrc/c1w.hip or on gemm.hip"""
    global _C1W
    _C1W = bool(on)


def c1r_bndx_on():
    return _C1R_BNDX


def c1n_enabled():
    return bool(_lib.load().wfae_get_c1n())


def c1wd_enabled():
    return bool(_lib.load().wfae_get_c1wd())


def c1ws_enabled():
    return bool(_lib.load().wfae_get_c1ws())


def _precision():
    return _lib.load().wfae_get_matmul_precision()


def c1r_supported(m, k, hw):
    return _C1R and _SPLIT_GEMM and _precision() == 0 and bool(_lib.load().wfae_c1r_supported(int(m), int(k), int(hw)))


def c1r_bnred_supported(m, k, hw):
    return (_C1R and _C1R_BNRED and _SPLIT_GEMM and _precision() == 0
            and bool(_lib.load().wfae_c1r_bnred_supported(int(m), int(k), int(hw))))


def c1rb_supported(m, k, hw):
    return _C1RB and _precision() == 1 and bool(_lib.load().wfae_c1rb_supported(int(m), int(k), int(hw)))


def c1b_supported(m, k, hw):
    return _C1B and _precision() == 1 and bool(_lib.load().wfae_c1b_supported(int(m), int(k), int(hw)))


def conv1x1_bnact_supported(x, cout):
    """geometries wfae_conv1x1_fwd_bnact / wfae_conv1x1_bwd_weight_bnact serve (the library re-checks and refuses the rest); x: the
    operand or its (N, Cin, H, W) shape"""
    nb, cin, h, wd = getattr(x, "shape", x)
    swapped = cin < cout and cin < 128          # the weight gradient then computes dW^T (N = Cout columns)
    return (h * wd) % 4 == 0 and h * wd >= 16 and cin % 4 == 0 and (cout % 4 == 0 or not swapped)


def conv1x1_route(op, m, k, hw, storage="f32", prologue=False, bias=False, residual="none"):
    """The kernel family that serves one 1x1 product — the whole decision, from the switches, the matmul precision and the
    library's wfae_*_supported predicates; no tensor is touched.  -> 'c1r' | 'c1rb' | 'c1b' | 'c1w' | 'gemm'.

    op 'fwd' | 'dgrad' | 'wgrad'; (m, k): y[m] = A[m, k] x[k] — forward (Cout, Cin), data gradient (Cin, Cout), weight
    gradient (Cout, Cin) of the convolution it belongs to; hw pixels per image; storage 'f32' | 'bf16' of the activations;
    prologue: BatchNorm + GELU in the operand loader; bias; residual 'none' | 'ordinary' | 'broadcast'.

    'gemm' covers the library's own hand-off to csrc/c1n.hip: inside wfae_conv1x1_fwd / _fwd_stats / _fwd_bnact (no bias,
    no residual) and wfae_conv1x1_bwd_data, fp32 tensors at fp32 precision with the split GEMMs on, (M, K) = (128, 512) and
    (256, 1024), unless set_c1n(False).

    Weight gradients: c1w wherever wfae_c1w_supported — fp32 tensors at fp32 precision with the split GEMMs on, bf16-stored
    tensors at 'medium'.

    A bias, a broadcast residual or a residual on a product that does not widen (m <= k; the register-direct kernels add
    one to widening products only) stay on gemm.hip.

    fp32 tensors: c1r for every shape it serves (profiles/r04_kbench_c1r_variants.txt, r04_kbench_c1r_knobs.txt): at
    C = 256 gemm.hip's kernels are bound by the fp32 MFMA instruction and c1r wins all four products (0.346 -> 0.31, 0.445 ->
    0.30, 0.685 -> 0.49, 0.500 -> 0.40 - 0.45 ms); at C = 128 both are HBM-bound: c1r wins the forward launches, which carry a
    BatchNorm + GELU prologue and / or a residual + BatchNorm-sum epilogue in the step (0.72 -> 0.65, 1.14 -> 1.02 ms), and
    ties the two plain data gradients (0.54 - 0.59 vs 0.57 - 0.59 ms) — one kernel family per stage, and every form of a
    shape on the same kernel keeps fused and unfused forms bit-identical.  The M-sliced shapes of the C >= 512 stages serve the
    widening products in both directions (profiles/r04_kbench_c1r_sliced.txt).

    bf16-stored tensors (profiles/r04_kbench_c1rb_vs_c1b.txt): c1rb wins or ties every form except the narrowing products of
    C >= 256 with the BatchNorm + GELU prologue, which run on c1b: the M-sliced ones (C >= 512) evaluate the activation of the
    whole operand again in every slice (0.163 -> 0.462 ms), and the prologue forms run one wave per SIMD (csrc/c1rb.hip,
    wfae_c1rb_fwd: with two, repeat launches differed), where C = 256 takes 0.327 ms against c1b's 0.284 (C = 128: 0.477
    against 0.536, kept).  That exception holds whatever set_c1b says: the switch is the A/B of the shapes c1rb does not serve.
    The bf16 forms of conv1x1_fwd* / conv1x1_bwd_data are gemm.hip's own (c1b needs the planes of c1b_weights, which they do
    not have); functional.py follows this route."""
    if op == "wgrad":
        ok = _C1W and _lib.load().wfae_c1w_supported(int(k), int(m), int(hw))
        return "c1w" if ok and (_precision() == 1 if storage == "bf16" else (_precision() == 0 and _SPLIT_GEMM)) else "gemm"
    if bias or residual == "broadcast" or (residual == "ordinary" and m <= k):
        return "gemm"
    if storage == "f32":
        return "c1r" if c1r_supported(m, k, hw) else "gemm"
    rb = c1rb_supported(m, k, hw)
    if rb and not (prologue and m < k and k >= 256):
        return "c1rb"
    return "c1b" if (rb or c1b_supported(m, k, hw)) else "gemm"


def conv1x1_dgrad_bn_route(m, k, hw, storage="f32"):
    """How the data gradient (m, k) in front of a BatchNorm + GELU backward takes that backward along (C <= 256 widening
    gradients on c1r): 'bndx' — c1r_bnred(store=False) for the sums, then c1r_bndx, which computes the product again and
    applies the second pass in its epilogue, so dA is never stored; 'bnred' — c1r_bnred stores dA, bn_act_bwd_dx reads it;
    None — the product of conv1x1_route('dgrad', ...) followed by bn_act_bwd."""
    if storage == "f32" and c1r_bnred_supported(m, k, hw):
        return "bndx" if _C1R_BNDX else "bnred"
    return None


_C1_PEAK = {"c1r": PEAK_BF16_MFMA / 6, "c1rb": PEAK_BF16_MFMA, "c1b": PEAK_BF16_MFMA, "gemm": None}   # None: _PEAK_OF


def _c1_launch(fam, w, transposed, x, st=None, bias=None, res=None, res_broadcast=False, stats=False, label=None):
    """y = A f(x) (+ bias) (+ res) on family `fam`: A = w (Cout, Cin) or, transposed, w^T (the data gradient) — for c1b the bf16
    (M, K) plane of c1b_weights that is already A; f = the BatchNorm + GELU of `st` or nothing; stats: the epilogue also
    reduces the BatchNorm sums of y.  -> (y, StatRows | None); gemm.hip reports no rows for shapes whose epilogue has no
    sums (run bn_stats_train on y)."""
    sfx, es = _chka(x, res)
    nb, k, h, wd = x.shape
    hw, n = h * wd, nb * h * wd
    if fam == "c1b":
        if not sfx or w.dtype != BF16 or not w.is_contiguous() or w.shape[1] != k:
            raise _lib.WfaeError("c1b_fwd: bf16 activations and the contiguous (M, K) bf16 weight plane of c1b_weights")
        m = w.shape[0]
    else:
        _chk(w, bias)
        if fam != "gemm" and (fam == "c1rb") != bool(sfx):
            raise _lib.WfaeError(f"{fam}: {'bf16-stored' if fam == 'c1rb' else 'fp32'} activations")
        m = w.shape[1] if transposed else w.shape[0]
    y = torch.empty((nb, m, h, wd), dtype=x.dtype, device=x.device)
    by = es * n * (k + m) + w.element_size() * k * m + (0 if res is None else es * n * m)
    ps, ph = (None, None) if st is None else (_p(st.scale), _p(st.shift))
    label = label or ("wfae_conv1x1_bwd_data" if transposed else "wfae_conv1x1_fwd_bnact" if st is not None else "wfae_conv1x1_fwd")
    part, rows, out = None, None, _NO_ROWS
    if stats:     # the register-direct capacity is sized for the widest user of the shape
        cap = 4 * ((n + 127) // 128) * m if fam == "gemm" else 2 * int(getattr(_lib.load(), f"wfae_{fam}_stat_rows")(m, k, nb, hw)) * m
        part, rows, out = _rows_out(cap, x.device)
    if fam in ("c1r", "c1rb"):
        name, args = f"wfae_{fam}_fwd", (_p(w), *((1, m) if transposed else (k, 1)), _p(x), ps, ph, _p(res), _p(y), nb, k, m, hw, *out)
    elif fam == "c1b":
        name, args = "wfae_c1b_fwd", (_p(w), _p(x), ps, ph, _p(res), _p(y), nb, k, m, hw, *out)
    elif transposed:
        name, args = "wfae_conv1x1_bwd_data" + sfx, (_p(x), _p(w), _p(y), nb, m, k, hw)
    else:
        tail = (_p(w), _p(bias), _p(res), 0 if res_broadcast else m * hw, _p(y), nb, k, m, hw)
        if sfx or st is not None:
            name, args = "wfae_conv1x1_fwd" + (sfx or "_bnact"), (_p(x), ps, ph, *tail, *out)
        else:
            name, args = ("wfae_conv1x1_fwd_stats", (_p(x), *tail, *out)) if stats else ("wfae_conv1x1_fwd", (_p(x), *tail))
    _call(name, 2 * n * k * m, by, *args, _stream(), label=label, peak=_C1_PEAK[fam])
    if not stats:
        return y, None
    if fam == "gemm":
        return y, (StatRows(part, rows.value) if rows.value > 0 else None)
    return y, StatRows(part if fam == "c1b" else part[:2 * rows.value * m], rows.value)


# the private names tests/ reach into, as questions to the route and calls onto the launch path
def _c1r_take(m, k, hw, dgrad):
    return conv1x1_route("dgrad" if dgrad else "fwd", m, k, hw) == "c1r"


def _c1w_route(dy, x, sfx):
    return conv1x1_route("wgrad", dy.shape[1], x.shape[1], dy.shape[2] * dy.shape[3], "bf16" if sfx else "f32") == "c1w"


def _c1r(w, transposed, x, st, res, stats, label):
    r = _c1_launch("c1r", w, transposed, x, st, None, res, False, stats, label)
    return r if stats else r[0]


def _c1_fwd(x, st, w, bias, res, res_broadcast, stats):
    nb, cin, h, wd = x.shape
    residual = "broadcast" if res_broadcast else "none" if res is None else "ordinary"
    fam = "gemm" if x.dtype == BF16 else conv1x1_route("fwd", w.shape[0], cin, h * wd, "f32", st is not None, bias is not None, residual)
    return _c1_launch(fam, w, False, x, st, bias, res, res_broadcast, stats)


def conv1x1_fwd(x, w, bias=None, res=None, res_broadcast=False):
    if res_broadcast and x.dtype == BF16:
        raise _lib.WfaeError("conv1x1_fwd: the broadcast residual (pos_emb) belongs to an fp32 layer")
    return _c1_fwd(x, None, w, bias, res, res_broadcast, False)[0]


def conv1x1_fwd_stats(x, w, bias=None, res=None):
    """conv1x1_fwd whose epilogue also reduces the per-channel sum / sum of squares of y (for the BatchNorm that
    follows).  -> (y, StatRows | None); None = this shape is not served, run bn_stats_train on y."""
    return _c1_fwd(x, None, w, bias, res, False, True)


def conv1x1_fwd_bnact(x, st, w, bias=None, res=None, stats=False):
    """conv1x1_fwd(bn_act_fwd(x, st, GELU), w): the activated tensor is rebuilt in the GEMM's operand loader and never
    written (reference chain BN -> GELU -> Conv2d 1x1, pipeline/models/ae_64x8x8_lin.py:14-15).  stats=True: the
    epilogue also reduces the BatchNorm sums of y -> (y, StatRows | None)"""
    r = _c1_fwd(x, st, w, bias, res, False, stats)
    return r if stats else r[0]


def conv1x1_bwd_data(dy, w):
    nb, cout, h, wd = dy.shape
    fam = "gemm" if dy.dtype == BF16 else conv1x1_route("dgrad", w.shape[1], cout, h * wd)
    return _c1_launch(fam, w, True, dy)[0]


def c1rb_fwd(w, transposed, x, st=None, res=None, stats=False, label="wfae_c1b_fwd"):
    """_c1_launch on csrc/c1rb.hip (y bf16; the fp32 weight itself is passed, the kernel rounds it into its LDS image)
    -> y | (y, StatRows)"""
    r = _c1_launch("c1rb", w, transposed, x, st, None, res, False, stats, label)
    return r if stats else r[0]


def c1b_weights(w):
    """w (Cout, Cin[,1,1]) fp32 -> (Wb (Cout, Cin), Wtb (Cin, Cout)) bf16"""
    _chk(w)
    cout, cin = w.shape[0], w.shape[1]
    Wb = torch.empty((cout, cin), dtype=BF16, device=w.device)
    Wtb = torch.empty((cin, cout), dtype=BF16, device=w.device)
    _call("wfae_c1b_weights", 0, 8 * w.numel(), _p(w), _p(Wb), _p(Wtb), cout, cin, _stream())
    return Wb, Wtb


def c1b_fwd(Wb, x, st=None, res=None, stats=False, label="wfae_c1b_fwd"):
    """_c1_launch on csrc/c1b.hip; Wb (M, K) from c1b_weights -> y | (y, StatRows of y)"""
    r = _c1_launch("c1b", Wb, False, x, st, None, res, False, stats, label)
    return r if stats else r[0]


def _c1_wgrad(dy, x, st, dw, accumulate):
    """dw (Cout, Cin) (+)= dy . f(x)^T, f = the BatchNorm + GELU of `st` rebuilt in the loader, or nothing"""
    sfx, es = _chka(dy, x)
    _chk(dw)
    nb, cout, h, wd = dy.shape
    cin, n = x.shape[1], nb * h * wd
    pro = (None, None) if st is None else (_p(st.scale), _p(st.shift))
    peak = None
    if conv1x1_route("wgrad", cout, cin, h * wd, "bf16" if sfx else "f32", st is not None) == "c1w":
        name, peak = "wfae_c1w_bwd_weight" + sfx, PEAK_BF16_MFMA / (1 if sfx else 6)
    elif sfx:
        name = "wfae_conv1x1_bwd_weight_bf16"
    else:
        name, pro = ("wfae_conv1x1_bwd_weight", ()) if st is None else ("wfae_conv1x1_bwd_weight_bnact", pro)
    ws = workspace()
    _call(name, 2 * n * cin * cout, es * n * (cin + cout) + 4 * cin * cout, _p(dy), _p(x), *pro, _p(dw), nb, cin, cout, h * wd,
          int(accumulate), ws.data_ptr(), ws.numel(), _stream(), peak=peak,
          label="wfae_conv1x1_bwd_weight" if st is None else "wfae_conv1x1_bwd_weight_bnact")
    return dw


def conv1x1_bwd_weight(dy, x, dw, accumulate=False):
    return _c1_wgrad(dy, x, None, dw, accumulate)


def conv1x1_bwd_weight_bnact(dy, x, st, dw, accumulate=False):
    """conv1x1_bwd_weight(dy, bn_act_fwd(x, st, GELU), dw) without the activated tensor in HBM"""
    return _c1_wgrad(dy, x, st, dw, accumulate)


# Pixels per image from which the Bottleneck backward takes the fused form.  No crossover was found: tools/kbench.py --only c1wd
# (profiles/r08_c1wd_kbench_vs_pair.txt, B = 32) has the fused launch ahead at every size measured, down to 512 pixels, the
# smallest — 0.036 -> 0.027 ms at C = 128, 0.053 -> 0.041 ms at C = 256, where it is one kernel + reduce against two kernels +
# reduce.  Nothing below 512 was measured, and the launch traces recorded at 128 and 192 pixels
# (tests/golden/g19_c1_launches.json) hold the pair.
C1WD_MIN_HW = 512


def conv1x1_wd_supported(c, mid, hw, storage="f32"):
    """csrc/c1wd.hip serves the shape AND the two launches it replaces are today's pair (c1w weight gradient with the BatchNorm +
    GELU prologue, c1r data gradient), whose results it reproduces bit for bit: C in (128, 256), mid = C / 4, hw % 64 == 0, fp32
    tensors at fp32 precision with the split GEMMs on, set_c1wd / set_c1w / set_c1r on"""
    return (storage == "f32" and _SPLIT_GEMM and _precision() == 0 and bool(_lib.load().wfae_c1wd_supported(int(c), int(mid), int(hw)))
            and conv1x1_route("wgrad", c, mid, hw, "f32", True) == "c1w" and conv1x1_route("dgrad", mid, c, hw) == "c1r")


def conv1x1_wd_route(c, mid, hw, storage="f32"):
    """How a Bottleneck's backward computes dW3 and dA3 from dy when a3 was not materialised: 'c1wd' — one launch that reads dy
    once (conv1x1_bwd_wd) — or 'pair' — conv1x1_bwd_weight_bnact + the data gradient of conv1x1_route.  Below C1WD_MIN_HW
    pixels both forms are launch-bound and there is no dy traffic to save."""
    return "c1wd" if hw >= C1WD_MIN_HW and conv1x1_wd_supported(c, mid, hw, storage) else "pair"


def conv1x1_bwd_wd(dy, t2, st, w3, dw3, accumulate=False):
    """dw3 (+)= dy . gelu(bn(t2))^T as conv1x1_bwd_weight_bnact(dy, t2, st, dw3) and da3 = w3^T dy as the c1r data gradient, both
    bit for bit, in one pass over dy (csrc/c1wd.hip) -> da3; None: not served (nothing launched, the caller runs the pair) —
    st None (the activated tensor was materialised), bf16-stored tensors, other shapes, set_c1wd(False)"""
    if st is None or dy.dtype != torch.float32 or t2.dtype != torch.float32:
        return None
    nb, c, h, wd = dy.shape
    mid, hw = t2.shape[1], h * wd
    if not conv1x1_wd_supported(c, mid, hw):
        return None
    _chk(dy, t2, w3, dw3)
    if tuple(t2.shape) != (nb, mid, h, wd) or w3.numel() != c * mid or dw3.numel() != c * mid:
        raise _lib.WfaeError("conv1x1_bwd_wd: dy (N, C, H, W), t2 (N, C/4, H, W), w3 and dw3 (C, C/4)")
    if (dy.data_ptr() | t2.data_ptr()) & 15:
        return None
    da = torch.empty_like(t2)
    n = nb * hw
    ws = workspace()
    _call("wfae_c1wd_bwd", 4 * n * c * mid, 4 * n * (c + 2 * mid) + 8 * c * mid, _p(dy), _p(t2), _p(st.scale), _p(st.shift), _p(w3),
          _p(dw3), _p(da), nb, c, mid, hw, int(accumulate), ws.data_ptr(), ws.numel(), _stream(), peak=PEAK_BF16_MFMA / 6,
          label="wfae_c1wd_bwd")
    return da


def conv1x1_ws_supported(c, mid, hw, storage="f32"):
    """csrc/c1ws.hip serves the shape AND the two launches it replaces are today's pair (c1w weight gradient with the BatchNorm +
    GELU prologue, whose bits it keeps, and the sums-alone c1r_bnred in front of c1r_bndx, whose fp32 quads it adds up in fp64):
    C in (128, 256), mid = C / 4, hw % 64 == 0, fp32 tensors at fp32 precision with the split GEMMs on, set_c1ws / set_c1w /
    set_c1r / set_c1r_bnred / set_c1r_bndx on"""
    return (storage == "f32" and _SPLIT_GEMM and _precision() == 0 and bool(_lib.load().wfae_c1ws_supported(int(c), int(mid), int(hw)))
            and conv1x1_route("wgrad", mid, c, hw, "f32", True) == "c1w" and conv1x1_dgrad_bn_route(c, mid, hw, storage) == "bndx")


def conv1x1_ws_route(c, mid, hw, storage="f32"):
    """How a Bottleneck's backward computes dW1 and the sums of the first BatchNorm's backward from x and dT1 when a1 was not
    materialised: 'c1ws' — one launch that reads x once (conv1x1_bwd_ws) — or 'pair' — conv1x1_bwd_weight_bnact + the sums-alone
    c1r_bnred.  Below C1WD_MIN_HW pixels both forms are launch-bound (nothing below was measured; the launch traces recorded
    at 128 and 192 pixels, tests/golden/g19_c1_launches.json, hold the pair)."""
    return "c1ws" if hw >= C1WD_MIN_HW and conv1x1_ws_supported(c, mid, hw, storage) else "pair"


def conv1x1_bwd_ws(dt1, x, st, w1, dw1, accumulate=False):
    """dw1 (+)= dt1 . gelu(bn(x))^T as conv1x1_bwd_weight_bnact(dt1, x, st, dw1), bit for bit, and the partial rows of
    c1r_bnred(w1, dt1, x, st, store=False) (the same fp32 sums of four pixels, added in fp64 in another order), in one pass over x
    (csrc/c1ws.hip) -> StatRows, to be finished by bn_act_bwd_from_rows; None: not served (nothing launched, the caller runs
    the pair) — st None (the activated tensor was materialised), bf16-stored tensors, other shapes, set_c1ws(False)"""
    if st is None or dt1.dtype != torch.float32 or x.dtype != torch.float32:
        return None
    nb, c, h, wd = x.shape
    mid, hw = dt1.shape[1], h * wd
    if not conv1x1_ws_supported(c, mid, hw):
        return None
    _chk(dt1, x, w1, dw1)
    if tuple(dt1.shape) != (nb, mid, h, wd) or w1.numel() != c * mid or dw1.numel() != c * mid:
        raise _lib.WfaeError("conv1x1_bwd_ws: x (N, C, H, W), dt1 (N, C/4, H, W), w1 and dw1 (C/4, C)")
    if (dt1.data_ptr() | x.data_ptr()) & 15:
        return None
    n = nb * hw
    ws = workspace()
    cap = 2 * int(_lib.load().wfae_c1ws_stat_rows(c, mid, nb, hw, ws.numel())) * c
    if cap <= 0:
        return None
    part, rows, out = _rows_out(cap, x.device)
    _call("wfae_c1ws_bwd", 4 * n * c * mid, 4 * n * (c + mid) + 8 * c * mid, _p(x), _p(dt1), _p(st.scale), _p(st.shift), _p(st.mean),
          _p(st.invstd), _p(w1), _p(dw1), *out, nb, c, mid, hw, int(accumulate), ws.data_ptr(), ws.numel(), _stream(),
          peak=PEAK_BF16_MFMA / 6, label="wfae_c1ws_bwd")
    return StatRows(part[:2 * rows.value * c], rows.value)


def c1r_bnred(w, dt, x, st, store=True):
    """da = conv1x1_bwd_data(dt, w) on c1r with phase 1 of bn_act_bwd(da, x, ...) taken in the epilogue -> (da, StatRows of
    (sum dU, sum dU xhat)); finish with bn_act_bwd_from_rows, then bn_act_bwd_dx — or, with store=False (da is None: the sums
    alone), with c1r_bndx, which rebuilds da in its own registers"""
    _chk(w, dt, x)
    nb, k, h, wd = dt.shape
    m, n = w.shape[1], nb * h * wd
    da = torch.empty((nb, m, h, wd), dtype=torch.float32, device=dt.device) if store else None
    part, rows, out = _rows_out(2 * int(_lib.load().wfae_c1r_stat_rows(m, k, nb, h * wd)) * m, dt.device)
    _call("wfae_c1r_bnred", 2 * n * k * m, 4 * (n * (k + (2 if store else 1) * m) + k * m), _p(w), 1, m, _p(dt), _p(x), _p(st.scale),
          _p(st.shift), _p(st.mean), _p(st.invstd), _p(da), nb, k, m, h * wd, *out, _stream(), label="wfae_conv1x1_bwd_data",
          peak=_C1_PEAK["c1r"])
    return da, StatRows(part[:2 * rows.value * m], rows.value)


def bn_act_bwd_from_rows(sr, c, dgamma, dbeta, accumulate=False):
    """phase 1 of bn_act_bwd from the partial rows of c1r_bnred: dgamma / dbeta + the coefficients at the head of this stream's
    workspace, where bn_act_bwd_dx (phase 2) reads them (no other workspace user in between)"""
    _chk(dgamma, dbeta)
    ws = workspace()
    _call("wfae_bn_act_bwd_from_rows", 0, 8 * sr.part.numel(), sr.part.data_ptr(), sr.rows, c, _p(dgamma), _p(dbeta), int(accumulate),
          ws.data_ptr(), ws.numel(), _stream(), label="wfae_bn_act_bwd[reduce]")
    return ws


def bn_act_bwd_dx(dy, x, gamma, st, res=None, act=1, training=True):
    """phase 2 of bn_act_bwd alone (after bn_act_bwd_from_rows on the same stream; fp32 storage)"""
    _chk(dy, x, gamma, res)
    nb, c, h, wd = x.shape
    dx = torch.empty_like(x)
    ws = workspace()
    _call("wfae_bn_act_bwd", 0, 4 * x.numel() * (4 if res is not None else 3), _p(dy), _p(x), _p(gamma), _p(st.scale), _p(st.shift),
          _p(st.mean), _p(st.invstd), _p(res), _p(dx), None, None, nb, c, h * wd, act, int(training), 0, 2, ws.data_ptr(),
          ws.numel(), _stream(), label="wfae_bn_act_bwd[dx]")
    return dx


def c1r_bndx(w, dt, x, gamma, st, res=None, training=True):
    """dx of  conv1x1(gelu(bn(x)), w)  given dt, second pass: da = conv1x1_bwd_data(dt, w) rebuilt in registers and
    bn_act_bwd_dx(da, x, ...) + res applied in the epilogue (after c1r_bnred(store=False) + bn_act_bwd_from_rows on this stream)"""
    _chk(w, dt, x, gamma, res)
    nb, k, h, wd = dt.shape
    m, n = w.shape[1], nb * h * wd
    dx = torch.empty((nb, m, h, wd), dtype=torch.float32, device=dt.device)
    ws = workspace()
    _call("wfae_c1r_bndx", 2 * n * k * m, 4 * (n * (k + (3 if res is not None else 2) * m) + k * m), _p(w), 1, m, _p(dt), _p(x), _p(gamma),
          _p(st.scale), _p(st.shift), _p(st.mean), _p(st.invstd), ws.data_ptr(), _p(res), _p(dx), nb, k, m, h * wd, int(training),
          _stream(), label="wfae_c1r_bndx", peak=_C1_PEAK["c1r"])
    return dx


# ------------------------------------------------------------------- linear
def linear_fwd(x, w, bias=None):
    _chk(x, w, bias)
    b, inf = x.shape
    out = w.shape[0]
    y = torch.empty((b, out), dtype=x.dtype, device=x.device)
    ws = workspace()
    _call("wfae_linear_fwd", 2 * b * inf * out, 4 * (inf * out + b * (inf + out)), _p(x), _p(w), _p(bias), _p(y), b, inf, out, ws.data_ptr(), ws.numel(), _stream())
    return y


def linear_fwd_rowinv(x, w, bias=None):
    """x (B, In) @ w (Out, In)^T + bias like linear_fwd, with the bits of a result row a function of that row of x, of w,
    bias and the matmul precision alone: not of B, of the row's place, of the other rows, nor of the pointers' alignment
    (include/wfae.h "row-invariant nn.Linear forward"; csrc/linear_rowinv.hip).  In and Out: multiples of 32 up to 4096"""
    _chk(x, w, bias)
    if x.dim() != 2 or w.dim() != 2 or w.shape[1] != x.shape[1] or (bias is not None and tuple(bias.shape) != (w.shape[0],)):
        raise _lib.WfaeError(f"linear_fwd_rowinv: expected x (B, In), w (Out, In) and bias (Out), got {tuple(x.shape)}, "
                             f"{tuple(w.shape)} and {None if bias is None else tuple(bias.shape)}")
    b, inf = x.shape
    out = w.shape[0]
    y = torch.empty((b, out), dtype=x.dtype, device=x.device)
    _call("wfae_linear_fwd_rowinv", 2 * b * inf * out, 4 * (inf * out + b * (inf + out)), _p(x), _p(w), _p(bias), _p(y), b, inf,
          out, _stream(), peak=_default_peak())
    return y


def linear_bwd_data(dy, w):
    _chk(dy, w)
    b, out = dy.shape
    inf = w.shape[1]
    dx = torch.empty((b, inf), dtype=dy.dtype, device=dy.device)
    tiles = ((b + 127) // 128) * ((inf + 127) // 128)
    if tiles < 256 and out >= 512:    # few output tiles, long reduction: split it
        ws = workspace(b * inf * 4 * 2)
        _call("wfae_linear_bwd_data_splitk", 2 * b * inf * out, 4 * (inf * out + b * (inf + out)), _p(dy), _p(w), _p(dx), b, inf,
              out, ws.data_ptr(), ws.numel(), _stream())
        return dx
    _call("wfae_linear_bwd_data", 2 * b * inf * out, 4 * (inf * out + b * (inf + out)), _p(dy), _p(w), _p(dx), b, inf, out, _stream())
    return dx


def linear_bwd_weight(dy, x, dw, accumulate=False):
    _chk(dy, x, dw)
    b, out = dy.shape
    inf = x.shape[1]
    tiles = ((out + 127) // 128) * ((inf + 127) // 128)
    if tiles < 256 and b >= 256:      # few output tiles, long batch dimension: split it (transformer layers)
        ws = workspace(out * inf * 4 * 2)
        _call("wfae_linear_bwd_weight_splitk", 2 * b * inf * out, 4 * (inf * out + b * (inf + out)), _p(dy), _p(x), _p(dw), b, inf,
              out, int(accumulate), ws.data_ptr(), ws.numel(), _stream())
        return dw
    _call("wfae_linear_bwd_weight", 2 * b * inf * out, 4 * (inf * out + b * (inf + out)), _p(dy), _p(x), _p(dw), b, inf, out, int(accumulate), _stream())
    return dw


# ------------------------------------------------------ 4x4 stride-2 family
# Winograd forms of the 4x4 stride-2 operations (csrc/wino.hip, include/wfae.h): F(2x2,2x2) (9/16 of the
# multiplies) or F(4x4,2x2) (25/64), paid for with streaming transforms of the operands.
# WFAE_WINO = 0: never; f22 / f42: that variant whenever the geometry allows; unset / auto: F(4x4,2x2) when Hlo, Wlo
# are multiples of 4, else F(2x2,2x2), for layers with both channel counts >= 16 (measured, tools/kbench.py: every
# GEMM-class layer of the model gains).
_WINO_MODE = os.environ.get("WFAE_WINO", "auto")
_plans = {}


def set_winograd(mode):
    """'auto' | 'f22' | 'f42' | True (= auto without the channel threshold) | False — overrides WFAE_WINO"""
    global _WINO_MODE
    _WINO_MODE = mode if isinstance(mode, str) else ("1" if mode else "0")


_PRECISIONS = {"highest": 0, "high": 0, "medium": 1}


def set_float32_matmul_precision(precision):
    """Counterpart of torch.set_float32_matmul_precision, which the reference calls once at start-up
    (experiments/ae_v2/train.py:270, 'high' = TF32 on its CUDA machines).  'highest' (default) and 'high': fp32
    MFMA (gfx950 has no TF32/xf32 matrix instruction; fp32 is the next precision up).  'medium': every GEMM-family
    kernel rounds its operands to bf16 on the way into the matrix core and accumulates in fp32, tensors stay fp32
    (BASELINE config 5).  In 'medium' the automatic Winograd choice is F(2x2,2x2): the F(4x4,2x2) transforms
    amplify operand rounding ~10x, which fp32 absorbs and bf16 does not."""
    global _ACT_DTYPE
    if precision not in _PRECISIONS:
        raise ValueError(f"precision must be one of {sorted(_PRECISIONS)}, got {precision!r}")
    _lib.call("wfae_set_matmul_precision", _PRECISIONS[precision])
    _ACT_DTYPE = BF16 if (_PRECISIONS[precision] == 1 and os.environ.get("WFAE_BF16_STORAGE", "1") != "0") else torch.float32


def get_float32_matmul_precision():
    return "medium" if _lib.load().wfae_get_matmul_precision() == 1 else "highest"


class WinoPlan:
    __slots__ = ("variant", "nb", "chi", "clo", "hlo", "wlo", "T", "nU", "nV", "nM", "split", "planes")

    @property
    def dims(self):
        return (self.nb, self.chi, self.clo, self.hlo, self.wlo)

    @property
    def gemm_flops(self):
        per = 12.5 if self.variant else 18.0
        return per * self.nb * self.hlo * self.wlo * self.clo * self.chi


def _query_plan(variant, key):
    out = (ctypes.c_int64 * 4)()
    rc = _lib.load().wfae_wino_sizes(variant, *key, ctypes.cast(out, ctypes.c_void_p))
    if rc != 0:
        return None
    pl = WinoPlan()
    pl.variant = variant
    pl.nb, pl.chi, pl.clo, pl.hlo, pl.wlo = key
    pl.T, pl.nU, pl.nV, pl.nM = (int(v) for v in out)
    pl.split = False
    pl.planes = 3
    return pl


# Winograd-domain GEMMs on the bf16 matrix pipe with fp32-exact three-plane operands (include/wfae.h, "split"): the
# default at fp32 precision wherever the geometry allows; WFAE_SPLIT_GEMM=0 keeps v_mfma_f32_32x32x2_f32
_SPLIT_GEMM = os.environ.get("WFAE_SPLIT_GEMM", "1") != "0"


def set_split_gemm(on):
    """switch the split-operand GEMMs (Winograd-domain products and the in-register split of the generic GEMM kernel)
    on / off (plans are cached per setting)"""
    global _SPLIT_GEMM
    _SPLIT_GEMM = bool(on)
    _lib.call("wfae_set_split_gemm", int(_SPLIT_GEMM))


def split_gemm_enabled():
    return _SPLIT_GEMM


def wino_plan(nb, chi, clo, hlo, wlo):
    """WinoPlan when a Winograd form should run for this layer geometry, else None"""
    mode = _WINO_MODE
    if mode == "0":
        return None
    if mode == "auto" and min(chi, clo) < 16:
        return None
    if mode not in ("f22", "f42") and _lib.load().wfae_get_matmul_precision() == 1:
        mode = os.environ.get("WFAE_WINO_BF16", "f22")
        if mode == "0":
            return None
    key = (nb, chi, clo, hlo, wlo)
    # split operands: three exact planes at fp32 precision, the bf16 h plane alone at 'medium' precision
    prec = _lib.load().wfae_get_matmul_precision()
    split = _SPLIT_GEMM
    ck = (mode if mode in ("f22", "f42") else "a", split, prec, key)
    pl = _plans.get(ck, False)
    if pl is False:
        if mode == "f22":
            pl = _query_plan(0, key)
        elif mode == "f42":
            pl = _query_plan(1, key)
        else:
            pl = _query_plan(1, key) or _query_plan(0, key)
        if pl is not None and split:
            pl.split = bool(_lib.load().wfae_wino_split_supported(pl.variant, *key))
            pl.planes = 3 if prec == 0 else 1
        _plans[ck] = pl
    return pl


def _buf(n, like):
    return torch.empty(n, dtype=torch.float32, device=like.device)


def _buf3(n, like, planes=3):
    """a split operand: `planes` planes of bf16 bit patterns, n elements each"""
    return torch.empty(planes * n, dtype=torch.int16, device=like.device)


def split_bf16x3(x, planes=3):
    """fp32 tensor -> its three bf16 planes (int16 bit patterns, shape (3,) + x.shape): x == h + m + l exactly;
    planes=1: the h plane alone (x rounded to bf16)"""
    _chk(x)
    out = torch.empty((planes,) + tuple(x.shape), dtype=torch.int16, device=x.device)
    _call("wfae_split_bf16x3", 0, (4 + 2 * planes) * x.numel(), _p(x), out.data_ptr(), x.numel(), planes, _stream())
    return out


def split_gemm(a3, b3, b_kind=0):
    """C[y] = A[y] B[y] from split operands: a3 (P, Y, M, K); b3 (P, Y, K, N) for b_kind 0, (P, Y, N, K) for b_kind 1;
    P = 3 planes (exact fp32 product) or 1 (bf16-rounded operands)"""
    planes, y, m, k = a3.shape
    n = b3.shape[3] if b_kind == 0 else b3.shape[2]
    if a3.dtype != torch.int16 or b3.dtype != torch.int16 or not (a3.is_contiguous() and b3.is_contiguous()):
        raise _lib.WfaeError("split_gemm: contiguous int16 plane tensors from split_bf16x3")
    c = torch.empty((y, m, n), dtype=torch.float32, device=a3.device)
    if b3.shape[0] != planes:
        raise _lib.WfaeError("split_gemm: operands with different plane counts")
    _call("wfae_split_gemm", 2 * y * m * n * k, 2 * planes * y * k * (m + n) + 4 * y * m * n, b_kind, planes, a3.data_ptr(),
          b3.data_ptr(), _p(c), m, n, k, y, _stream())
    return c


def wino_weights(w, pl):
    _chk(w)
    if pl.split:
        U = _buf3(2 * pl.nU, w, pl.planes)   # U3 then Ut3
        _call("wfae_wino_weights_split", 0, 4 * w.numel() + 4 * pl.planes * pl.nU, pl.variant, _p(w), U.data_ptr(),
              U.data_ptr() + 2 * pl.planes * pl.nU, pl.planes, pl.chi, pl.clo, _stream(), label="wfae_wino_weights")
        return U
    U = _buf(pl.nU, w)
    _call("wfae_wino_weights", 0, 4 * (w.numel() + pl.nU), pl.variant, _p(w), _p(U), pl.chi, pl.clo, _stream())
    return U


def wino_in(hi, pl):
    """hi-side tensor (N,Chi,2Hlo,2Wlo) -> V[xi][4Chi][T]"""
    if not pl.split:
        hi = to_f32(hi)      # the fp32-operand transforms read fp32 tensors
    sfx, es = _chka(hi)
    if pl.split:
        V = _buf3(pl.nV, hi, pl.planes)
        _call("wfae_wino_in_split" + sfx, 0, es * hi.numel() + 2 * pl.planes * pl.nV, pl.variant, _p(hi), V.data_ptr(), pl.planes,
              pl.nb, pl.chi, pl.hlo, pl.wlo, _stream(), label="wfae_wino_in")
        return V
    V = _buf(pl.nV, hi)
    _call("wfae_wino_in", 0, 4 * (hi.numel() + pl.nV), pl.variant, _p(hi), _p(V), pl.nb, pl.chi, pl.hlo, pl.wlo, _stream())
    return V


def wino_out_t(lo, pl):
    """lo-side tensor (N,Clo,Hlo,Wlo) -> Mt[xi][Clo][T]"""
    if not pl.split:
        lo = to_f32(lo)
    sfx, es = _chka(lo)
    if pl.split:
        Mt = _buf3(pl.nM, lo, pl.planes)
        _call("wfae_wino_out_t_split" + sfx, 0, es * lo.numel() + 2 * pl.planes * pl.nM, pl.variant, _p(lo), Mt.data_ptr(), pl.planes,
              pl.nb, pl.clo, pl.hlo, pl.wlo, _stream(), label="wfae_wino_out_t")
        return Mt
    Mt = _buf(pl.nM, lo)
    _call("wfae_wino_out_t", 0, 4 * (lo.numel() + pl.nM), pl.variant, _p(lo), _p(Mt), pl.nb, pl.clo, pl.hlo, pl.wlo, _stream())
    return Mt


# tiles per image below which the Winograd output / adjoint input transforms leave the BatchNorm sums to the ordinary
# statistics pass (the sum-reducing kernels need one block per (channel, image); tests set 0 to exercise them on small shapes)
WINO_STATS_MIN_TILES = 256


def wino_down(U, V, pl, stats=False, out_dtype=torch.float32):
    """lo = Out(U * V) stored as `out_dtype`; stats=True: -> (lo, StatParts of lo) — the output transform also reduces the
    BatchNorm sums"""
    M = _buf(pl.nM, V)
    lo = torch.empty((pl.nb, pl.clo, pl.hlo, pl.wlo), dtype=out_dtype, device=V.device)
    es = lo.element_size()
    if pl.split:
        _call("wfae_wino_gemm_down_split", pl.gemm_flops, 2 * pl.planes * (pl.nU + pl.nV) + 4 * pl.nM, pl.variant, U.data_ptr(),
              V.data_ptr(), _p(M), pl.planes, *pl.dims, _stream(), label="wfae_wino_gemm_down")
    else:
        _call("wfae_wino_gemm_down", pl.gemm_flops, 4 * (pl.nU + pl.nV + pl.nM), pl.variant, _p(U), _p(V), _p(M), *pl.dims, _stream())
    m = 4 if pl.variant else 2
    # images of fewer than 256 tiles: the transform runs one thread per (channel, image, tile) (full waves, whole cache
    # lines of M) and the sums of the small result are taken by the ordinary statistics pass
    small = (pl.hlo // m) * (pl.wlo // m) < WINO_STATS_MIN_TILES
    if not stats or small:
        if out_dtype == BF16:
            _call("wfae_wino_out_bf16", 0, 4 * pl.nM + es * lo.numel(), pl.variant, _p(M), _p(lo), pl.nb, pl.clo, pl.hlo, pl.wlo,
                  None, 0, None, _stream(), label="wfae_wino_out")
        else:
            _call("wfae_wino_out", 0, 4 * (pl.nM + lo.numel()), pl.variant, _p(M), _p(lo), pl.nb, pl.clo, pl.hlo, pl.wlo, _stream())
        return (lo, None) if stats else lo
    part, splits, out = _rows_out(2 * pl.clo * pl.nb * (((pl.hlo // m) * (pl.wlo // m) + 255) // 256), V.device)
    _call("wfae_wino_out_bf16" if out_dtype == BF16 else "wfae_wino_out_stats", 0, 4 * pl.nM + es * lo.numel(), pl.variant, _p(M),
          _p(lo), pl.nb, pl.clo, pl.hlo, pl.wlo, *out, _stream(), label="wfae_wino_out")
    return lo, StatParts(part, splits.value)


def wino_up(U, Mt, pl, stats=False, out_dtype=torch.float32):
    """hi = In^T(U^T * Mt) stored as `out_dtype`; stats=True: -> (hi, StatParts of hi)"""
    dV = _buf(pl.nV, Mt)
    hi = torch.empty((pl.nb, pl.chi, 2 * pl.hlo, 2 * pl.wlo), dtype=out_dtype, device=Mt.device)
    es = hi.element_size()
    if pl.split:
        _call("wfae_wino_gemm_up_split", pl.gemm_flops, 2 * pl.planes * (pl.nU + pl.nM) + 4 * pl.nV, pl.variant,
              U.data_ptr() + 2 * pl.planes * pl.nU, Mt.data_ptr(), _p(dV), pl.planes, *pl.dims, _stream(), label="wfae_wino_gemm_up")
    else:
        _call("wfae_wino_gemm_up", pl.gemm_flops, 4 * (pl.nU + pl.nV + pl.nM), pl.variant, _p(U), _p(Mt), _p(dV), *pl.dims, _stream())
    m = 4 if pl.variant else 2
    small = (pl.hlo // m) * (pl.wlo // m) < WINO_STATS_MIN_TILES
    if not stats or small:
        if out_dtype == BF16:
            _call("wfae_wino_in_t_bf16", 0, 4 * pl.nV + es * hi.numel(), pl.variant, _p(dV), _p(hi), pl.nb, pl.chi, pl.hlo, pl.wlo,
                  None, 0, None, _stream(), label="wfae_wino_in_t")
        else:
            _call("wfae_wino_in_t", 0, 4 * (pl.nV + hi.numel()), pl.variant, _p(dV), _p(hi), pl.nb, pl.chi, pl.hlo, pl.wlo, _stream())
        return (hi, None) if stats else hi
    part, splits, out = _rows_out(2 * pl.chi * pl.nb * (((pl.hlo // m) * (pl.wlo // m) + 255) // 256), Mt.device)
    _call("wfae_wino_in_t_bf16" if out_dtype == BF16 else "wfae_wino_in_t_stats", 0, 4 * pl.nV + es * hi.numel(), pl.variant, _p(dV),
          _p(hi), pl.nb, pl.chi, pl.hlo, pl.wlo, *out, _stream(), label="wfae_wino_in_t")
    return hi, StatParts(part, splits.value)


def wino_wgrad(Mt, V, dw, pl, accumulate=False):
    """dw (Clo,Chi,4,4) (+)= G^T (Mt * V^T) G"""
    _chk(dw)
    if pl.split:
        ws = workspace(min(pl.nU * 4 * 13, max(pl.nU * 4 * 6, 1 << 30)))
        _call("wfae_wino_gemm_wgrad_split", pl.gemm_flops, 2 * pl.planes * (pl.nV + pl.nM) + 4 * pl.nU, pl.variant, Mt.data_ptr(),
              V.data_ptr(), _p(dw), pl.planes, *pl.dims, int(accumulate), ws.data_ptr(), ws.numel(), _stream(),
              label="wfae_wino_gemm_wgrad")
        return dw
    ws = workspace(pl.nU * 4 * 6)
    _call("wfae_wino_gemm_wgrad", pl.gemm_flops, 4 * (pl.nU + pl.nV + pl.nM), pl.variant, _p(Mt), _p(V), _p(dw), *pl.dims,
          int(accumulate), ws.data_ptr(), ws.numel(), _stream())
    return dw


def conv4x4s2_down(hi, w):
    """hi (N,Chi,2H,2W), w (Clo,Chi,4,4) -> lo (N,Clo,H,W)"""
    _chka(hi)
    _chk(w)
    nb, chi, h2, w2 = hi.shape
    clo = w.shape[0]
    hlo, wlo = h2 // 2, w2 // 2
    pl = wino_plan(nb, chi, clo, hlo, wlo)
    if pl is not None:
        return wino_down(wino_weights(w, pl), wino_in(hi, pl), pl, out_dtype=hi.dtype)
    if hi.dtype == BF16:      # shapes without a Winograd form run the fp32 gather GEMM
        return to_bf16(conv4x4s2_down(to_f32(hi), w))
    lo = torch.empty((nb, clo, hlo, wlo), dtype=hi.dtype, device=hi.device)
    _call("wfae_conv4x4s2_down", 32 * nb * hlo * wlo * clo * chi, 4 * (nb * hlo * wlo * (clo + 4 * chi) + 16 * clo * chi), _p(hi), _p(w), _p(lo), nb, chi, clo, hlo, wlo, _stream())
    return lo


def conv4x4s2_up(lo, w):
    """lo (N,Clo,H,W), w (Clo,Chi,4,4) -> hi (N,Chi,2H,2W)"""
    _chka(lo)
    _chk(w)
    nb, clo, hlo, wlo = lo.shape
    chi = w.shape[1]
    pl = wino_plan(nb, chi, clo, hlo, wlo)
    if pl is not None:
        return wino_up(wino_weights(w, pl), wino_out_t(lo, pl), pl, out_dtype=lo.dtype)
    if lo.dtype == BF16:
        return to_bf16(conv4x4s2_up(to_f32(lo), w))
    hi = torch.empty((nb, chi, 2 * hlo, 2 * wlo), dtype=lo.dtype, device=lo.device)
    ws = workspace(w.numel() * 4)
    _call("wfae_conv4x4s2_up", 32 * nb * hlo * wlo * clo * chi, 4 * (nb * hlo * wlo * (clo + 4 * chi) + 16 * clo * chi), _p(lo), _p(w), _p(hi), nb, chi, clo, hlo, wlo, ws.data_ptr(), ws.numel(), _stream())
    return hi


def conv4x4s2_wgrad(lo, hi, dw, accumulate=False):
    _chk(dw)
    if wino_plan(lo.shape[0], hi.shape[1], lo.shape[1], lo.shape[2], lo.shape[3]) is None:
        lo, hi = to_f32(lo), to_f32(hi)
        _chk(lo, hi)
    nb, clo, hlo, wlo = lo.shape
    chi = hi.shape[1]
    pl = wino_plan(nb, chi, clo, hlo, wlo)
    if pl is not None:
        return wino_wgrad(wino_out_t(lo, pl), wino_in(hi, pl), dw, pl, accumulate)
    ws = workspace(dw.numel() * 4 * 2)
    _call("wfae_conv4x4s2_wgrad", 32 * nb * hlo * wlo * clo * chi, 4 * (nb * hlo * wlo * (clo + 4 * chi) + 16 * clo * chi), _p(lo), _p(hi), _p(dw), nb, chi, clo, hlo, wlo, int(accumulate),
              ws.data_ptr(), ws.numel(), _stream())
    return dw


# ------------------------------------------------------------- direct convs
def dconv_fwd(x, w, bias, ks, stride, pad, groups, out_dtype=torch.float32):
    """direct convolution; bf16 storage serves the two full-resolution layers with one channel on one side: the first layer
    (x fp32, one channel -> out_dtype bf16) and the output convolution (x bf16 -> fp32)"""
    _chk(w, bias)
    nb, cin, h, wd = x.shape
    cout = w.shape[0]
    ho = (h + 2 * pad - ks) // stride + 1
    wo = (wd + 2 * pad - ks) // stride + 1
    fl, n_in, n_out = 2 * nb * ho * wo * cout * (cin // groups) * ks * ks, x.numel(), nb * cout * ho * wo
    if x.dtype == BF16:
        _chka(x)
        if not (ks == 3 and stride == 1 and pad == 1 and groups == 1 and out_dtype == torch.float32):
            raise _lib.WfaeError("dconv_fwd: a bf16-stored input is served for the 3x3 stride-1 output convolution only")
        y = torch.empty((nb, cout, ho, wo), dtype=torch.float32, device=x.device)
        _call("wfae_dconv_fwd_bf16in", fl, 2 * n_in + 4 * n_out + 4 * w.numel(), _p(x), _p(w), _p(bias), _p(y), nb, cin, cout, h, wd,
              _stream(), label="wfae_dconv_fwd")
        return y
    _chk(x)
    if out_dtype == BF16:
        if not (cin == 1 and groups == 1 and ks == 4 and stride == 2 and pad == 1):
            raise _lib.WfaeError("dconv_fwd: a bf16-stored result is served for the one-channel 4x4 stride-2 first layer only")
        y = torch.empty((nb, cout, ho, wo), dtype=BF16, device=x.device)
        _call("wfae_dconv_fwd_bf16out", fl, 4 * n_in + 2 * n_out + 4 * w.numel(), _p(x), _p(w), _p(bias), _p(y), nb, cout, h, wd,
              _stream(), label="wfae_dconv_fwd")
        return y
    y = torch.empty((nb, cout, ho, wo), dtype=x.dtype, device=x.device)
    _call("wfae_dconv_fwd", 2 * nb * ho * wo * cout * (cin // groups) * ks * ks, 4 * (nb * (cin * h * wd + cout * ho * wo) + w.numel()), _p(x), _p(w), _p(bias), _p(y), nb, cin, cout, h, wd, ks, stride, pad, groups, _stream())
    return y


def dconv_bwd_data(dy, w, cin, ks, pad, groups, out_dtype=torch.float32):
    """data gradient of a stride-1 convolution; the input plane is (Ho + ks - 1 - 2 pad)^2.  out_dtype bf16: the output
    convolution's data gradient (dy fp32, one channel)"""
    _chk(dy, w)
    nb, cout, ho, wo = dy.shape
    h, wd = ho + ks - 1 - 2 * pad, wo + ks - 1 - 2 * pad
    if out_dtype == BF16:
        if not (cout == 1 and groups == 1 and ks == 3 and pad == 1):
            raise _lib.WfaeError("dconv_bwd_data: a bf16-stored result is served for the one-channel output convolution only")
        dx = torch.empty((nb, cin, h, wd), dtype=BF16, device=dy.device)
        _call("wfae_dconv_bwd_data_bf16out", 2 * nb * h * wd * cin * 9, 4 * dy.numel() + 2 * dx.numel(), _p(dy), _p(w), _p(dx), nb,
              cin, h, wd, _stream(), label="wfae_dconv_bwd_data")
        return dx
    dx = torch.empty((nb, cin, h, wd), dtype=dy.dtype, device=dy.device)
    _call("wfae_dconv_bwd_data", 2 * nb * h * wd * cout * (cin // groups) * ks * ks, 4 * (nb * h * wd * (cin + cout) + w.numel()), _p(dy), _p(w), _p(dx), nb, cin, cout, h, wd, ks, pad, groups, _stream())
    return dx


def dconv_bwd_weight(dy, x, dw, ks, stride, pad, groups, accumulate=False):
    _chk(dw)
    nb, cin, h, wd = x.shape
    cout = dy.shape[1]
    ws = workspace()
    if dy.dtype == BF16 or x.dtype == BF16:
        # the two layers with one channel on one side: the big tensor is bf16, the one-channel tensor fp32
        first = dy.dtype == BF16 and x.dtype == torch.float32 and cin == 1 and ks == 4 and stride == 2 and pad == 1
        last = x.dtype == BF16 and dy.dtype == torch.float32 and cout == 1 and ks == 3 and stride == 1 and pad == 1
        if not ((first or last) and groups == 1):
            raise _lib.WfaeError("dconv_bwd_weight: bf16 storage serves the first layer and the output convolution only")
        big, small, c = (dy, x, cout) if first else (x, dy, cin)
        _chka(big)
        _chk(small)
        _call("wfae_c1_wgrad_bf16", 2 * dy.numel() * cin * ks * ks, 2 * big.numel() + 4 * small.numel(), 0 if first else 1, _p(big),
              _p(small), _p(dw), nb, c, h, wd, int(accumulate), ws.data_ptr(), ws.numel(), _stream(), label="wfae_dconv_bwd_weight")
        return dw
    _chk(dy, x)
    _call("wfae_dconv_bwd_weight", 2 * dy.numel() * (cin // groups) * ks * ks, 4 * (x.numel() + dy.numel() + dw.numel()), _p(dy), _p(x), _p(dw), nb, cin, cout, h, wd, ks, stride, pad, groups,
              int(accumulate), ws.data_ptr(), ws.numel(), _stream())
    return dw


def conv4x4s1_supported(c_read):
    """MFMA path of the stride-1 4x4 convolution: the channel count of the operand that is read must be a
    multiple of 16 (smaller layers go through the direct kernels)"""
    return c_read % 16 == 0


def conv4x4s1_fwd(x, w, pad=1, transposed=False):
    """4x4 stride-1 convolution on the GEMM kernel; transposed=True: x is dy, the result is the data gradient"""
    _chk(x, w)
    nb, c, h, wd = x.shape
    cout, cin = w.shape[0], w.shape[1]
    pe = 3 - pad if transposed else pad
    m = cin if transposed else cout
    ho, wo = h + 2 * pe - 3, wd + 2 * pe - 3
    y = torch.empty((nb, m, ho, wo), dtype=x.dtype, device=x.device)
    ws = workspace()
    _call("wfae_conv4x4s1_fwd", 32 * nb * ho * wo * cin * cout, 4 * (x.numel() + y.numel() + w.numel()), _p(x), _p(w), _p(y),
          nb, cin, cout, h, wd, pad, int(transposed), ws.data_ptr(), ws.numel(), _stream())
    return y


def conv4x4s1_bwd_weight(dy, x, dw, pad=1, accumulate=False):
    _chk(dy, x, dw)
    nb, cin, h, wd = x.shape
    cout = dy.shape[1]
    ws = workspace()
    _call("wfae_conv4x4s1_bwd_weight", 32 * dy.numel() * cin, 4 * (x.numel() + dy.numel() + dw.numel()), _p(dy), _p(x), _p(dw),
          nb, cin, cout, h, wd, pad, int(accumulate), ws.data_ptr(), ws.numel(), _stream())
    return dw


def gconv3x3_supported(c, groups):
    return c % groups == 0 and (c // groups) in (4, 8, 16, 32)


_G3B = True   # A/B through set_g3b()


def set_g3b(on):
    """A/B switch: bf16 grouped 3x3 convolutions on the implicit-GEMM kernel (csrc/g3b.hip) or on the dconv.hip kernels"""
    global _G3B
    _G3B = bool(on)


def g3b_supported(c, h, wd, groups):
    return _G3B and _lib.load().wfae_get_matmul_precision() == 1 and bool(
        _lib.load().wfae_g3b_supported(int(c), int(h), int(wd), int(groups)))


def gconv3x3_fwd(x, w, groups, transposed=False):
    """grouped 3x3 'same' conv with Cin == Cout (Bottleneck middle conv); transposed=True gives the data gradient."""
    sfx, es = _chka(x)
    _chk(w)
    nb, c, h, wd = x.shape
    y = torch.empty_like(x)
    ws = workspace()
    cpg = c // groups
    if sfx == "" and _G3B and _lib.load().wfae_g3b_f32_supported(int(c), int(h), int(wd), int(groups), 0):
        _call("wfae_g3b_fwd", 2 * x.numel() * cpg * 9, 2 * es * x.numel(), _p(x), _p(w), _p(y), nb, c, h, wd, groups,
              int(transposed), ws.data_ptr(), ws.numel(), _stream(), label="wfae_gconv3x3_fwd", peak=PEAK_BF16_MFMA / 6)
        return y
    if sfx == "_bf16" and g3b_supported(c, h, wd, groups):
        _call("wfae_g3b_fwd_bf16", 2 * x.numel() * cpg * 9, 2 * es * x.numel(), _p(x), _p(w), _p(y), nb, c, h, wd, groups,
              int(transposed), ws.data_ptr(), ws.numel(), _stream(), label="wfae_gconv3x3_fwd", peak=PEAK_BF16_MFMA)
        return y
    _call("wfae_gconv3x3_fwd" + sfx, 2 * x.numel() * cpg * 9, 2 * es * x.numel(), _p(x), _p(w), _p(y), nb, c, h, wd, groups,
          int(transposed), ws.data_ptr(), ws.numel(), _stream(), label="wfae_gconv3x3_fwd")
    return y


def gconv3x3_bwd_weight(dy, x, dw, groups, accumulate=False):
    sfx, es = _chka(dy, x)
    _chk(dw)
    nb, c, h, wd = x.shape
    ws = workspace()
    if sfx == "" and _G3B and _lib.load().wfae_g3b_f32_supported(int(c), int(h), int(wd), int(groups), 1):
        _call("wfae_g3b_bwd_weight", 2 * x.numel() * (c // groups) * 9, 2 * es * x.numel(), _p(dy), _p(x), _p(dw), nb, c, h, wd,
              groups, int(accumulate), ws.data_ptr(), ws.numel(), _stream(), label="wfae_gconv3x3_bwd_weight", peak=PEAK_BF16_MFMA / 6)
        return dw
    if sfx == "_bf16" and g3b_supported(c, h, wd, groups):
        _call("wfae_g3b_bwd_weight_bf16", 2 * x.numel() * (c // groups) * 9, 2 * es * x.numel(), _p(dy), _p(x), _p(dw), nb, c, h, wd,
              groups, int(accumulate), ws.data_ptr(), ws.numel(), _stream(), label="wfae_gconv3x3_bwd_weight", peak=PEAK_BF16_MFMA)
        return dw
    _call("wfae_gconv3x3_bwd_weight" + sfx, 2 * x.numel() * (c // groups) * 9, 2 * es * x.numel(), _p(dy), _p(x), _p(dw), nb, c,
          h, wd, groups, int(accumulate), ws.data_ptr(), ws.numel(), _stream(), label="wfae_gconv3x3_bwd_weight")
    return dw


# ---------------------------------------------------------------- BatchNorm
class BnStats:
    """per-channel vectors produced by the statistics kernels"""
    __slots__ = ("mean", "invstd", "scale", "shift")

    def __init__(self, c, device):
        buf = torch.empty((4, c), dtype=torch.float32, device=device)
        self.mean, self.invstd, self.scale, self.shift = buf[0], buf[1], buf[2], buf[3]


def bn_stats_train(x, gamma, beta, running_mean, running_var, eps=1e-5, momentum=0.1):
    sfx, es = _chka(x)
    _chk(gamma, beta, running_mean, running_var)
    nb, c, h, wd = x.shape
    st = BnStats(c, x.device)
    ws = workspace()
    _call("wfae_bn_stats_train" + sfx, 0, es * x.numel(), _p(x), nb, c, h * wd, _p(gamma), _p(beta), eps, momentum, _p(running_mean),
              _p(running_var), _p(st.mean), _p(st.invstd), _p(st.scale), _p(st.shift), ws.data_ptr(), ws.numel(),
              _stream(), label="wfae_bn_stats_train")
    return st


def bn_stats_from_rows(sr, shape, gamma, beta, running_mean, running_var, eps=1e-5, momentum=0.1):
    """bn_stats_train of a tensor of `shape` (N, C, H, W) whose partial sums a producer epilogue left in `sr`"""
    _chk(gamma, beta, running_mean, running_var)
    nb, c, h, wd = shape
    st = BnStats(c, gamma.device)
    ws = workspace()
    _call("wfae_bn_stats_from_rows", 0, 8 * sr.part.numel(), sr.part.data_ptr(), sr.rows, nb, c, h * wd, _p(gamma), _p(beta), eps,
          momentum, _p(running_mean), _p(running_var), _p(st.mean), _p(st.invstd), _p(st.scale), _p(st.shift),
          ws.data_ptr(), ws.numel(), _stream(), label="wfae_bn_stats_train")
    return st


def bn_stats_from_parts(sp, shape, gamma, beta, running_mean, running_var, eps=1e-5, momentum=0.1):
    """bn_stats_train of a tensor of `shape` (N, C, H, W) whose fp64 partial sums a producer kernel left in `sp`"""
    _chk(gamma, beta, running_mean, running_var)
    nb, c, h, wd = shape
    st = BnStats(c, gamma.device)
    _call("wfae_bn_stats_from_parts", 0, 8 * sp.part.numel(), sp.part.data_ptr(), sp.splits, nb, c, h * wd, _p(gamma), _p(beta),
          eps, momentum, _p(running_mean), _p(running_var), _p(st.mean), _p(st.invstd), _p(st.scale), _p(st.shift), _stream(),
          label="wfae_bn_stats_train")
    return st


def bn_act_fwd_stats(x, st, act=1):
    """bn_act_fwd that also reduces the BatchNorm sums of its OUTPUT -> (y, StatParts)"""
    sfx, es = _chka(x)
    nb, c, h, wd = x.shape
    y = torch.empty_like(x)
    # capacity for the library's LARGEST split count per (image, channel) — its scalar path, cdiv(HW, 1024) clamped to
    # 1..1024 (the 16-byte path, taken by pointer alignment as well as by shape, needs fewer); `splits` comes back from the call
    part, splits, out = _rows_out(2 * c * nb * max(1, min(1024, (h * wd + 1023) // 1024)), x.device)
    _call("wfae_bn_act_fwd_stats" + sfx, 0, 2 * es * x.numel(), _p(x), _p(st.scale), _p(st.shift), _p(y), nb, c, h * wd, act,
          *out, _stream(), label="wfae_bn_act_fwd")
    return y, StatParts(part, splits.value)


def bn_fold_eval(gamma, beta, running_mean, running_var, eps=1e-5):
    _chk(gamma, beta, running_mean, running_var)
    c = gamma.shape[0]
    st = BnStats(c, gamma.device)
    _call("wfae_bn_fold_eval", 0, 0, _p(gamma), _p(beta), _p(running_mean), _p(running_var), eps, _p(st.mean),
              _p(st.invstd), _p(st.scale), _p(st.shift), c, _stream())
    return st


def bn_act_fwd(x, st, act=1):
    sfx, es = _chka(x)
    nb, c, h, wd = x.shape
    y = torch.empty_like(x)
    _call("wfae_bn_act_fwd" + sfx, 0, 2 * es * x.numel(), _p(x), _p(st.scale), _p(st.shift), _p(y), nb, c, h * wd, act, _stream(),
          label="wfae_bn_act_fwd")
    return y


def bn_act_bwd(dy, x, gamma, st, dgamma, dbeta, res=None, act=1, training=True, accumulate=False, need_dx=True):
    sfx, es = _chka(dy, x, res)
    _chk(gamma, dgamma, dbeta)
    nb, c, h, wd = x.shape
    dx = torch.empty_like(x) if need_dx else None
    ws = workspace()
    args = (_p(dy), _p(x), _p(gamma), _p(st.scale), _p(st.shift), _p(st.mean), _p(st.invstd), _p(res), _p(dx), _p(dgamma),
            _p(dbeta), nb, c, h * wd, act, int(training), int(accumulate))
    tail = (ws.data_ptr(), ws.numel(), _stream())
    n = x.numel()
    if _prof is None or not need_dx:
        _call("wfae_bn_act_bwd" + sfx, 0, es * n * (6 if res is not None else 5), *args, 3 if need_dx else 1, *tail,
              label="wfae_bn_act_bwd")
    else:
        # kernel-granular timing for the roofline read-out: the two kernels of this entry point separately
        _call("wfae_bn_act_bwd" + sfx, 0, 2 * es * n, *args, 1, *tail, label="wfae_bn_act_bwd[reduce]")
        _call("wfae_bn_act_bwd" + sfx, 0, es * n * (4 if res is not None else 3), *args, 2, *tail, label="wfae_bn_act_bwd[dx]")
    return dx


# ------------------------------------------------------------- element-wise
def _ew(name, a, b=None):
    _chk(a, b)
    out = torch.empty_like(a)
    if b is None:
        _call(name, 0, 8 * a.numel(), _p(a), _p(out), a.numel(), _stream())
    else:
        _call(name, 0, 12 * a.numel(), _p(a), _p(b), _p(out), a.numel(), _stream())
    return out


def gelu_fwd(x):
    return _ew("wfae_gelu_fwd", x)


def gelu_bwd(dy, x):
    return _ew("wfae_gelu_bwd", dy, x)


def sigmoid_fwd(x):
    return _ew("wfae_sigmoid_fwd", x)


def sigmoid_bwd(dy, y):
    return _ew("wfae_sigmoid_bwd", dy, y)


def add(a, b):
    return _ew("wfae_add", a, b)


def leaky_relu_fwd(x):
    return _ew("wfae_leaky_relu_fwd", x)


def leaky_relu_bwd(dy, x):
    return _ew("wfae_leaky_relu_bwd", dy, x)


def pad2d(x, pad):
    _chk(x)
    nb, c, h, wd = x.shape
    y = torch.empty((nb, c, h + 2 * pad, wd + 2 * pad), dtype=x.dtype, device=x.device)
    _call("wfae_pad2d", 0, 4 * (x.numel() + y.numel()), _p(x), _p(y), nb * c, h, wd, pad, 0, _stream())
    return y


def crop2d(xp, pad):
    _chk(xp)
    nb, c, hp, wp = xp.shape
    y = torch.empty((nb, c, hp - 2 * pad, wp - 2 * pad), dtype=xp.dtype, device=xp.device)
    _call("wfae_pad2d", 0, 4 * (xp.numel() + y.numel()), _p(xp), _p(y), nb * c, hp - 2 * pad, wp - 2 * pad, pad, 1, _stream())
    return y


def mean_fwd(x, hinge=False, sign=1.0, weight=1.0):
    """weight * mean(x)  or  weight * mean(relu(1 + sign*x))"""
    _chk(x)
    out = torch.empty((), dtype=torch.float32, device=x.device)
    ws = workspace()
    _call("wfae_mean_fwd", 0, 4 * x.numel(), _p(x), _p(out), x.numel(), int(hinge), sign, weight, ws.data_ptr(), ws.numel(), _stream())
    return out


def mean_bwd(x, gout, hinge=False, sign=1.0, weight=1.0):
    _chk(x, gout)
    dx = torch.empty_like(x)
    _call("wfae_mean_bwd", 0, 8 * x.numel(), _p(x), _p(gout), _p(dx), x.numel(), int(hinge), sign, weight, _stream())
    return dx


def scale(x, s=1.0, s_dev=None, out=None):
    """x * s * (s_dev[0] if given); out may alias x"""
    _chk(x, s_dev)
    y = torch.empty_like(x) if out is None else out
    _call("wfae_scale", 0, 8 * x.numel(), _p(x), _p(s_dev), float(s), _p(y), x.numel(), _stream())
    return y


def reduce_sum(x, outer, c, inner, out, accumulate=False):
    _chk(x, out)
    ws = workspace()
    _call("wfae_reduce_sum", 0, 4 * x.numel(), _p(x), outer, c, inner, _p(out), int(accumulate), ws.data_ptr(), ws.numel(), _stream())
    return out


# --------------------------------------------------------------------- loss
def sigmoid_l1_fwd(h, x, weight=1.0):
    _chk(h, x)
    recon = torch.empty_like(h)
    loss = torch.empty((), dtype=torch.float32, device=h.device)
    ws = workspace()
    _call("wfae_sigmoid_l1_fwd", 0, 12 * h.numel(), _p(h), _p(x), _p(recon), _p(loss), weight, h.numel(), ws.data_ptr(), ws.numel(),
              _stream())
    return recon, loss


def sigmoid_l1_bwd(recon, x, gloss, weight=1.0):
    _chk(recon, x, gloss)
    dh = torch.empty_like(recon)
    _call("wfae_sigmoid_l1_bwd", 0, 12 * recon.numel(), _p(recon), _p(x), _p(gloss), weight, _p(dh), recon.numel(), _stream())
    return dh


def l1_fwd(recon, x, weight=1.0):
    _chk(recon, x)
    loss = torch.empty((), dtype=torch.float32, device=recon.device)
    ws = workspace()
    _call("wfae_l1_fwd", 0, 8 * recon.numel(), _p(recon), _p(x), _p(loss), weight, recon.numel(), ws.data_ptr(), ws.numel(), _stream())
    return loss


def l1_bwd(recon, x, gloss, weight=1.0):
    _chk(recon, x, gloss)
    d = torch.empty_like(recon)
    _call("wfae_l1_bwd", 0, 12 * recon.numel(), _p(recon), _p(x), _p(gloss), weight, _p(d), recon.numel(), _stream())
    return d


# ------------------------------------------------- Path-B latent forecaster
def latent_diff_pack(v, tin):
    """v (B,T,C,H,W) -> X (B*H*W, tin*C), Y (B*H*W, (T-tin)*C), both differenced against frame tin-1"""
    _chk(v)
    b, t, c, h, w = v.shape
    X = torch.empty((b * h * w, tin * c), dtype=torch.float32, device=v.device)
    Y = torch.empty((b * h * w, (t - tin) * c), dtype=torch.float32, device=v.device)
    _call("wfae_latent_diff_pack", 0, 8 * v.numel(), _p(v), _p(X), _p(Y), b, t, tin, c, h * w, _stream())
    return X, Y


def latent_unpack_add(pred, v, tin):
    """pred (B*H*W, Tout*C) + last input frame of v (B,T,C,H,W) -> (B,Tout,C,H,W)"""
    _chk(pred, v)
    b, t, c, h, w = v.shape
    out = torch.empty((b, t - tin, c, h, w), dtype=torch.float32, device=v.device)
    _call("wfae_latent_unpack_add", 0, 8 * out.numel(), _p(pred), _p(v), _p(out), b, t, tin, c, h * w, _stream())
    return out


def mse_fwd(pred, target):
    _chk(pred, target)
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    ws = workspace()
    _call("wfae_mse_fwd", 0, 8 * pred.numel(), _p(pred), _p(target), _p(loss), pred.numel(), ws.data_ptr(), ws.numel(), _stream())
    return loss


def mse_bwd(pred, target, gloss):
    _chk(pred, target, gloss)
    d = torch.empty_like(pred)
    _call("wfae_mse_bwd", 0, 12 * pred.numel(), _p(pred), _p(target), _p(gloss), _p(d), pred.numel(), _stream())
    return d


# ---- DLinear (include/wfae.h "DLinear latent forecasters"): v (B, R, M), the predictor reads rows [0, L) ----------
def _dl_dims(v, L, P, K, individual, w):
    b, r, m = v.shape
    if K < 1 or K % 2 == 0:
        raise _lib.WfaeError(f"dlinear: kernel_size must be odd and >= 1, got {K}")
    want = (m, P, L) if individual else (P, L)
    if tuple(w.shape) != want:
        raise _lib.WfaeError(f"dlinear: weight shape {tuple(w.shape)}, expected {want}")
    return b, r, m


def dlinear_fwd(v, ws, bs, wt, bt, L, P, K, individual, diff=False, cf=1):
    """-> y (B, P, M) = Ws seasonal + bs + Wt trend + bt of rows [0, L) of v (differenced against the last input
    frame when diff)"""
    _chk(v, ws, bs, wt, bt)
    b, r, m = _dl_dims(v, L, P, K, individual, ws)
    y = torch.empty((b, P, m), dtype=torch.float32, device=v.device)
    nbytes = 4 * (b * L * m + b * P * m + 2 * ws.numel() + 2 * bs.numel())
    _call("wfae_dlinear_fwd", 4 * b * m * P * L, nbytes, _p(v), _p(ws), _p(bs), _p(wt), _p(bt), _p(y), b, r, m, L, P,
          K, int(individual), int(diff), cf, _stream())
    return y


def dlinear_bwd_weight(v, dy, dws, dbs, dwt, dbt, L, P, K, individual, diff=False, cf=1):
    """dWs, dbs, dWt, dbt (overwritten) of dlinear_fwd for the output gradient dy (B, P, M)"""
    _chk(v, dy, dws, dbs, dwt, dbt)
    b, r, m = _dl_dims(v, L, P, K, individual, dws)
    ws = workspace(4 * ((m + 63) // 64) * (2 * P * L + P))
    nbytes = 4 * (b * L * m + b * P * m + 2 * dws.numel() + 2 * dbs.numel())
    _call("wfae_dlinear_bwd_weight", 4 * b * m * P * L, nbytes, _p(v), _p(dy), _p(dws), _p(dbs), _p(dwt), _p(dbt),
          b, r, m, L, P, K, int(individual), int(diff), cf, ws.data_ptr(), ws.numel(), _stream())


def dlinear_bwd_data(dy, ws_, wt, R, L, K, individual, diff=False, cf=1):
    """-> dv (B, R, M): the input gradient of dlinear_fwd (rows >= L are zero)"""
    _chk(dy, ws_, wt)
    b, P, m = dy.shape
    if tuple(ws_.shape) != ((m, P, L) if individual else (P, L)):
        raise _lib.WfaeError(f"dlinear_bwd_data: weight shape {tuple(ws_.shape)} does not match dy {tuple(dy.shape)}")
    dv = torch.empty((b, R, m), dtype=torch.float32, device=dy.device)
    w = workspace(8 * b * L * m)
    _call("wfae_dlinear_bwd_data", 4 * b * m * P * L, 4 * (b * P * m + 2 * ws_.numel() + b * R * m), _p(dy), _p(ws_),
          _p(wt), _p(dv), b, R, m, L, P, K, int(individual), int(diff), cf, w.data_ptr(), w.numel(), _stream())
    return dv


def series_decomp_fwd(x, K):
    """x (B, L, M) -> (seasonal, trend) along L"""
    _chk(x)
    b, L, m = x.shape
    s, t = torch.empty_like(x), torch.empty_like(x)
    _call("wfae_series_decomp_fwd", 0, 12 * x.numel(), _p(x), _p(s), _p(t), b, L, m, K, _stream())
    return s, t


def series_decomp_bwd(ds, dt, K):
    _chk(ds, dt)
    b, L, m = ds.shape
    dx = torch.empty_like(ds)
    _call("wfae_series_decomp_bwd", 0, 12 * ds.numel(), _p(ds), _p(dt), _p(dx), b, L, m, K, _stream())
    return dx


def dlinear_target(v, L, P, cf=1):
    """v (B, R, M) -> (B, P, M) = v[:, L + p] - v[:, L - cf + p % cf]"""
    _chk(v)
    b, r, m = v.shape
    out = torch.empty((b, P, m), dtype=torch.float32, device=v.device)
    _call("wfae_dlinear_frames", 0, 12 * out.numel(), None, _p(v), _p(out), b, r, m, L, P, cf, 0, _stream())
    return out


def dlinear_forecast(pred, v, L, cf=1):
    """pred (B, P, M) + the last input frame of v (B, R, M) -> (B, P, M)"""
    _chk(pred, v)
    b, P, m = pred.shape
    out = torch.empty_like(pred)
    _call("wfae_dlinear_frames", 0, 12 * out.numel(), _p(pred), _p(v), _p(out), b, v.shape[1], m, L, P, cf, 1,
          _stream())
    return out


# ---- intensity-statistics MLP forecaster (include/wfae.h "intensity-statistics MLP forecaster") ---------------------
def _chk_dev_f32(*ts):
    """_chk without the contiguity rule, for entry points that take the memory order as an argument"""
    for t in ts:
        if not t.is_cuda:
            raise _lib.WfaeError("wfae kernels need device tensors (the HIP path has no CPU fallback)")
        if t.dtype != torch.float32:
            raise _lib.WfaeError(f"wfae kernels are fp32, got {t.dtype}")


def seq_intensity_stats(batch, t_in, groups=4):
    """batch: 'NHWT' sequences (B, H, W, T) fp32 -> (x (B, t_in), target (B, 2 * groups)): the mean of each of the
    first t_in frames; mean, then unbiased std, of `groups` equal runs of the remaining frames (reference
    v1_experiments/prediff_mlp_sevir/train.py:56-64).  The batch is read once, in the memory order it has — the
    frame-contiguous storage under the loader's permuted view, or a contiguous T-innermost tensor — never copied."""
    _chk_dev_f32(batch)
    if batch.dim() != 4:
        raise _lib.WfaeError(f"seq_intensity_stats: expected an 'NHWT' batch (B, H, W, T), got {tuple(batch.shape)}")
    b, h, w, t = batch.shape
    if batch.is_contiguous():
        t_innermost = 1
    elif batch.permute(0, 3, 1, 2).is_contiguous():
        t_innermost = 0
    else:
        raise _lib.WfaeError(f"seq_intensity_stats: strides {batch.stride()} of an 'NHWT' batch {tuple(batch.shape)} "
                             "are neither T-innermost contiguous nor a permuted view of a contiguous (B, T, H, W) "
                             "tensor; the kernel does not copy")
    if not 0 < t_in < t or groups < 1 or (t - t_in) % groups:
        raise _lib.WfaeError(f"seq_intensity_stats: pred_frames = {t - t_in} (of {t} frames, {t_in} input frames) must "
                             f"be a positive multiple of groups = {groups}: a group is a run of whole frames")
    x = torch.empty((b, t_in), dtype=torch.float32, device=batch.device)
    target = torch.empty((b, 2 * groups), dtype=torch.float32, device=batch.device)
    ws = workspace(_lib.load().wfae_seq_intensity_stats_ws_bytes(b, t, h * w, t_innermost))
    _call("wfae_seq_intensity_stats", 0, 4 * batch.numel(), _p(batch), _p(x), _p(target), b, t, h * w, t_in, groups,
          t_innermost, ws.data_ptr(), ws.numel(), _stream())
    return x, target


def _mlp3_dims(x, w1, b1, w2, b2, w3, b3):
    if x.dim() != 2:
        raise _lib.WfaeError(f"mlp3: expected x (B, in), got {tuple(x.shape)}")
    b, i = x.shape
    h, o = w1.shape[0], w3.shape[0]
    want = [(h, i), (h,), (h, h), (h,), (o, h), (o,)]
    got = [tuple(t.shape) for t in (w1, b1, w2, b2, w3, b3)]
    if got != want:
        raise _lib.WfaeError(f"mlp3: parameter shapes {got}, expected {want} for x {tuple(x.shape)}")
    return b, i, h, o


def mlp3_mse(x, target, w1, b1, w2, b2, w3, b3, grads=None):
    """Linear-ReLU-Linear-ReLU-Linear + F.mse_loss in one launch -> (pred (B, out), loss).  grads: six tensors shaped
    like the parameters, overwritten with d loss / d parameter; None: forward only.  target None (forward only):
    pred alone, loss is None."""
    _chk(x, target, w1, b1, w2, b2, w3, b3, *(grads or ()))
    b, i, h, o = _mlp3_dims(x, w1, b1, w2, b2, w3, b3)
    if target is not None and tuple(target.shape) != (b, o):
        raise _lib.WfaeError(f"mlp3_mse: target shape {tuple(target.shape)}, expected {(b, o)}")
    if grads is not None:
        if target is None:
            raise _lib.WfaeError("mlp3_mse: gradients need a target")
        if [tuple(g.shape) for g in grads] != [tuple(p.shape) for p in (w1, b1, w2, b2, w3, b3)]:
            raise _lib.WfaeError("mlp3_mse: gradient buffers must be shaped like the six parameters")
    pred = torch.empty((b, o), dtype=torch.float32, device=x.device)
    loss = None if target is None else torch.empty((), dtype=torch.float32, device=x.device)
    ws = workspace(4 * (4 * b * h + b * o))
    g = [_p(t) for t in grads] if grads is not None else [None] * 6
    macs = b * (i * h + h * h + h * o)
    _call("wfae_mlp3_mse", 2 * macs * (1 if grads is None else 3), 4 * (i * h + h * h + h * o) * (1 if grads is None else 2),
          _p(x), _p(target), _p(w1), _p(b1), _p(w2), _p(b2), _p(w3), _p(b3), _p(pred), _p(loss), *g, b, i, h, o,
          int(grads is None), ws.data_ptr(), ws.numel(), _stream())
    return pred, loss


# ---- conv latent autoencoder (include/wfae.h "conv latent autoencoder"): the fused conv + LayerNorm + LeakyReLU unit
CLN_KINDS = {"conv3": 0, "down4": 1, "up4": 2}


def _cln_dims(x, w, kind):
    if kind not in (0, 1, 2):
        raise _lib.WfaeError(f"cln: kind {kind!r}, expected 0 (3x3 s1), 1 (4x4 s2) or 2 (transposed 4x4 s2)")
    n, cin, h, wd = x.shape
    k = 3 if kind == 0 else 4
    cout = w.shape[1] if kind == 2 else w.shape[0]
    want = (cin, cout, k, k) if kind == 2 else (cout, cin, k, k)
    if tuple(w.shape) != want:
        raise _lib.WfaeError(f"cln: weight shape {tuple(w.shape)}, expected {want} for input {tuple(x.shape)}")
    if kind == 1 and (h % 2 or wd % 2):
        raise _lib.WfaeError(f"cln: the 4x4 stride-2 convolution needs an even input plane, got {h}x{wd}")
    ho, wo = (h, wd) if kind == 0 else (h // 2, wd // 2) if kind == 1 else (2 * h, 2 * wd)
    return n, cin, cout, h, wd, ho, wo, k


def cln_fwd(x, w, bias, gamma, beta, kind, slope=0.01):
    """-> y, xhat (N, Cout, Ho, Wo), mean, rstd (N): LeakyReLU_slope(LayerNorm([Cout, Ho, Wo])(conv(x) + bias))"""
    _chk(x, w, bias, gamma, beta)
    n, cin, cout, h, wd, ho, wo, k = _cln_dims(x, w, kind)
    if tuple(gamma.shape) != (cout, ho, wo) or tuple(beta.shape) != (cout, ho, wo):
        raise _lib.WfaeError(f"cln_fwd: LayerNorm affine {tuple(gamma.shape)}, expected {(cout, ho, wo)}")
    y = torch.empty((n, cout, ho, wo), dtype=torch.float32, device=x.device)
    xhat = torch.empty_like(y)
    mean = torch.empty((n,), dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    e = cout * ho * wo
    flops = 2 * n * e * cin * k * k // (4 if kind == 2 else 1) + 10 * n * e
    _call("wfae_cln_fwd", flops, 4 * (x.numel() + w.numel() + 2 * e + 2 * n * e), _p(x), _p(w), _p(bias), _p(gamma),
          _p(beta), _p(y), _p(xhat), _p(mean), _p(rstd), kind, n, cin, cout, h, wd, float(slope), _stream())
    return y, xhat, mean, rstd


def cln_bwd(dy, xhat, rstd, gamma, beta, x, w, dw, dbias, dgamma, dbeta, kind, slope=0.01, need_dx=True):
    """dw, dbias, dgamma, dbeta are overwritten; -> dx (N, Cin, H, W) or None"""
    _chk(dy, xhat, rstd, gamma, beta, x, w, dw, dbias, dgamma, dbeta)
    n, cin, cout, h, wd, ho, wo, k = _cln_dims(x, w, kind)
    if tuple(dy.shape) != (n, cout, ho, wo) or dy.shape != xhat.shape:
        raise _lib.WfaeError(f"cln_bwd: dy {tuple(dy.shape)} / xhat {tuple(xhat.shape)}, expected {(n, cout, ho, wo)}")
    dx = torch.empty_like(x) if need_dx else None
    ws = workspace(4 * n * (w.numel() + cout))
    e = cout * ho * wo
    per = 2 * n * e * cin * k * k // (4 if kind == 2 else 1)
    _call("wfae_cln_bwd", per * (2 if need_dx else 1) + 20 * n * e,
          4 * (3 * n * e + 2 * x.numel() + 2 * w.numel() + 4 * e + 2 * n * w.numel()), _p(dy), _p(xhat), _p(rstd),
          _p(gamma), _p(beta), _p(x), _p(w), _p(dx), _p(dw), _p(dbias), _p(dgamma), _p(dbeta), kind, n, cin, cout, h, wd,
          float(slope), ws.data_ptr(), ws.numel(), _stream())
    return dx


def huber_fwd(pred, target, delta=1.0):
    _chk(pred, target)
    if pred.shape != target.shape:
        raise _lib.WfaeError(f"huber_fwd: shapes {tuple(pred.shape)} and {tuple(target.shape)} differ")
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    ws = workspace()
    _call("wfae_huber_fwd", 0, 8 * pred.numel(), _p(pred), _p(target), _p(loss), pred.numel(), float(delta), ws.data_ptr(),
          ws.numel(), _stream())
    return loss


def huber_bwd(pred, target, gloss, delta=1.0):
    _chk(pred, target, gloss)
    d = torch.empty_like(pred)
    _call("wfae_huber_bwd", 0, 12 * pred.numel(), _p(pred), _p(target), _p(gloss), _p(d), pred.numel(), float(delta),
          _stream())
    return d


# ---- 3x3 stride-2 padding-1 convolution family of the conv + GAN latent model (include/wfae.h "3x3 stride-2"; csrc/c3s2.hip)
# w (Clo, Chi, 3, 3) is Conv2d(Chi -> Clo).weight and ConvTranspose2d(Clo -> Chi).weight; transposed names the module type.
def c3s2_live_taps(hhi, whi, hlo=None, wlo=None):
    """-> the 3 x 3 nested list of booleans: tap (ky, kx) is live iff some lo position (oy, ox) reads a real hi pixel
    through it, 0 <= 2 oy - 1 + ky < Hhi and likewise in x.  Pure host arithmetic (the library's rule is
    wfae_c3s2_live_taps)."""
    hlo = (hhi - 1) // 2 + 1 if hlo is None else hlo
    wlo = (whi - 1) // 2 + 1 if wlo is None else wlo

    def axis(k, hi, lo):
        # o = 0 reaches k = 1, 2 (source k - 1); o = 1 reaches k = 0 (source 1)
        return (k >= 1 and k - 1 < hi) or (k == 0 and lo >= 2 and hi >= 2)
    return [[axis(ky, hhi, hlo) and axis(kx, whi, wlo) for kx in range(3)] for ky in range(3)]


def _c3s2_geo(what, w, transposed, x_shape, output_padding=1):
    """-> (N, Chi, Clo, Hhi, Whi, Hlo, Wlo) from the module input's shape"""
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
        raise _lib.WfaeError(f"{what}: weight shape {tuple(w.shape)}, expected (Clo, Chi, 3, 3)")
    clo, chi = w.shape[0], w.shape[1]
    if len(x_shape) != 4 or x_shape[1] != (clo if transposed else chi):
        raise _lib.WfaeError(f"{what}: input {tuple(x_shape)} against {'ConvTranspose2d' if transposed else 'Conv2d'} "
                             f"weight {tuple(w.shape)}")
    n, _, h, wd = x_shape
    if transposed:
        oph, opw = output_padding if isinstance(output_padding, (tuple, list)) else (output_padding, output_padding)
        if oph not in (0, 1) or opw not in (0, 1):
            raise _lib.WfaeError(f"{what}: output_padding {output_padding!r}, a stride-2 transpose takes 0 or 1 (per axis)")
        return n, chi, clo, 2 * h - 1 + oph, 2 * wd - 1 + opw, h, wd
    return n, chi, clo, h, wd, (h - 1) // 2 + 1, (wd - 1) // 2 + 1


def _c3s2_ws(op, transposed, geo):
    return workspace(_lib.load().wfae_c3s2_workspace_bytes(op, int(transposed), *geo))


def c3s2_fwd(x, w, bias=None, transposed=False, act=True, output_padding=1, save_t=True):
    """-> (y, t): t = conv(x) + bias (pre-activation, None unless save_t), y = SiLU(t) if act else t.  Conv2d 3x3 s2 p1, or
    with transposed ConvTranspose2d 3x3 s2 p1 with output_padding (an int, or one per axis)"""
    geo = _c3s2_geo("c3s2_fwd", w, transposed, tuple(x.shape), output_padding)
    _chk(x, w, bias)
    n, chi, clo, hhi, whi, hlo, wlo = geo
    y = torch.empty((n, chi, hhi, whi) if transposed else (n, clo, hlo, wlo), dtype=torch.float32, device=x.device)
    t = torch.empty_like(y) if save_t else None
    ws = _c3s2_ws(0, transposed, geo)
    live = sum(map(sum, c3s2_live_taps(hhi, whi, hlo, wlo)))
    _call("wfae_c3s2_fwd", 2 * n * hlo * wlo * clo * chi * 9, 4 * (w.numel() * live // 9 + x.numel() + 2 * y.numel()),
          _p(x), _p(w), _p(bias), _p(y), _p(t), int(transposed), int(act), *geo, ws.data_ptr(), ws.numel(), _stream())
    return y, t


def _c3s2_geo_pair(what, w, hi_shape, lo_shape):
    """geometry from the shapes of the hi and the lo tensor; the library checks that the planes belong together"""
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
        raise _lib.WfaeError(f"{what}: weight shape {tuple(w.shape)}, expected (Clo, Chi, 3, 3)")
    clo, chi = w.shape[0], w.shape[1]
    if len(hi_shape) != 4 or len(lo_shape) != 4 or hi_shape[0] != lo_shape[0] or hi_shape[1] != chi or lo_shape[1] != clo:
        raise _lib.WfaeError(f"{what}: tensors {tuple(hi_shape)} (hi) / {tuple(lo_shape)} (lo) against weight {tuple(w.shape)}")
    return hi_shape[0], chi, clo, hi_shape[2], hi_shape[3], lo_shape[2], lo_shape[3]


def c3s2_bwd_data(da, t, w, x_shape, transposed=False, act=True):
    """-> dx of shape x_shape (the module input's): the data gradient for dt = da SiLU'(t) (da itself without act)"""
    _chk(da, t, w)
    x_shape = tuple(x_shape)
    geo = _c3s2_geo_pair("c3s2_bwd_data", w, da.shape if transposed else x_shape, x_shape if transposed else da.shape)
    n, chi, clo, hhi, whi, hlo, wlo = geo
    dx = torch.empty(x_shape, dtype=torch.float32, device=da.device)
    ws = _c3s2_ws(1, transposed, geo)
    live = sum(map(sum, c3s2_live_taps(hhi, whi, hlo, wlo)))
    _call("wfae_c3s2_bwd_data", 2 * n * hlo * wlo * clo * chi * 9, 4 * (w.numel() * live // 9 + 2 * da.numel() + dx.numel()),
          _p(da), _p(t), _p(w), _p(dx), int(transposed), int(act), *geo, ws.data_ptr(), ws.numel(), _stream())
    return dx


def c3s2_bwd_weight(da, t, x, dw, dbias=None, transposed=False, act=True, accumulate=False):
    """dw (Clo, Chi, 3, 3) and dbias of dt = da SiLU'(t) against the module input x, one call; dead taps of dw become exact
    zeros, or stay as they are when accumulating"""
    _chk(da, t, x, dw, dbias)
    hi, lo = (da, x) if transposed else (x, da)
    geo = _c3s2_geo_pair("c3s2_bwd_weight", dw, hi.shape, lo.shape)
    n, chi, clo, hhi, whi, hlo, wlo = geo
    ws = _c3s2_ws(2, transposed, geo)
    live = sum(map(sum, c3s2_live_taps(hhi, whi, hlo, wlo)))
    _call("wfae_c3s2_bwd_weight", 2 * n * hlo * wlo * clo * chi * 9, 4 * (dw.numel() * live // 9 + 2 * da.numel() + x.numel()),
          _p(da), _p(t), _p(x), _p(dw), _p(dbias), int(transposed), int(act), int(accumulate), *geo, ws.data_ptr(),
          ws.numel(), _stream())
    return dw


# ---- frozen AutoencoderKL latent provider (include/wfae.h "frozen AutoencoderKL"; csrc/aekl.hip), forward only
AEKL_KINDS = {"conv": 0, "down": 1, "up": 2}
AEKL_MODES = {"bf16": 1, "split3": 3, "fp32": 4}
# 'highest' / 'high' run "split3": measured 0.354 ms against 0.511 ms for "fp32" on the 128-channel 128 x 128 layer
# (DESIGN.md).  "fp32" is reachable only through an explicit `mode=` (tools/aekl_bench.py's comparison, one test).


def aekl_mode():
    """operand form of the 3x3 kernel under the current matmul precision"""
    return AEKL_MODES["bf16" if _lib.load().wfae_get_matmul_precision() == 1 else "split3"]


def _aekl_peak(mode):
    return PEAK_FP32_MFMA if mode == 4 else _planes_peak(mode)


def aekl_conv3_pack(w, mode=None):
    """(Cout, Cin, 3, 3) -> the packed (and split) operand of aekl_conv3_fwd for `mode`; done once per frozen layer"""
    _chk(w)
    mode = aekl_mode() if mode is None else mode
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
        raise _lib.WfaeError(f"aekl_conv3_pack: weight shape {tuple(w.shape)}, expected (Cout, Cin, 3, 3)")
    cout, cin = w.shape[:2]
    nbytes = _lib.load().wfae_aekl_conv3_pack_bytes(cout, cin, mode)
    if nbytes == 0:
        raise _lib.WfaeError(f"aekl_conv3_pack: unsupported Cout={cout} Cin={cin} mode={mode}")
    packed = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    _call("wfae_aekl_conv3_pack", 0, 4 * w.numel() + nbytes, _p(w), packed.data_ptr(), cout, cin, mode, _stream())
    return packed


def aekl_conv3_fwd(x, packed, cout, bias=None, gn=None, res=None, kind=0, mode=None, out_mul=1.0):
    """3x3 convolution on the matrix cores.  kind 0: stride 1 pad 1; 1: stride 2 over the (0, 1, 0, 1)-padded input;
    2: over the nearest x2 upsample.  gn = (scale, shift) (N, Cin): operand SiLU(x * scale + shift), zero padding after
    it.  y = (conv + bias + res) * out_mul."""
    mode = aekl_mode() if mode is None else mode
    scale, shift = gn if gn is not None else (None, None)
    _chk(x, bias, scale, shift, res)
    if x.dim() != 4:
        raise _lib.WfaeError(f"aekl_conv3_fwd: expected (N, C, H, W), got {tuple(x.shape)}")
    if kind not in (0, 1, 2):
        raise _lib.WfaeError(f"aekl_conv3_fwd: kind {kind!r}, expected 0 (stride 1), 1 (stride 2) or 2 (x2 upsample)")
    n, cin, h, wd = x.shape
    want = _lib.load().wfae_aekl_conv3_pack_bytes(cout, cin, mode)
    if want == 0 or packed.dtype != torch.uint8 or packed.numel() != want or not packed.is_cuda:
        raise _lib.WfaeError(f"aekl_conv3_fwd: packed weights do not belong to Cout={cout} Cin={cin} mode={mode}")
    if kind == 1 and (h < 2 or wd < 2):
        raise _lib.WfaeError(f"aekl_conv3_fwd: the stride-2 form needs a plane of at least 2x2, got {h}x{wd}")
    ho, wo = (h, wd) if kind == 0 else ((h - 2) // 2 + 1, (wd - 2) // 2 + 1) if kind == 1 else (2 * h, 2 * wd)
    if gn is not None and (tuple(scale.shape) != (n, cin) or tuple(shift.shape) != (n, cin)):
        raise _lib.WfaeError(f"aekl_conv3_fwd: prologue scale / shift {tuple(scale.shape)}, expected {(n, cin)}")
    if bias is not None and tuple(bias.shape) != (cout,):
        raise _lib.WfaeError(f"aekl_conv3_fwd: bias {tuple(bias.shape)}, expected {(cout,)}")
    if res is not None and tuple(res.shape) != (n, cout, ho, wo):
        raise _lib.WfaeError(f"aekl_conv3_fwd: residual {tuple(res.shape)}, expected {(n, cout, ho, wo)}")
    y = torch.empty((n, cout, ho, wo), dtype=torch.float32, device=x.device)
    _call("wfae_aekl_conv3_fwd", 2 * 9 * n * ho * wo * cin * cout,
          4 * (x.numel() + y.numel() * (2 if res is not None else 1)) + want, _p(x), packed.data_ptr(), _p(bias), _p(scale),
          _p(shift), _p(res), _p(y), kind, mode, n, cin, cout, h, wd, float(out_mul), _stream(),
          label=f"wfae_aekl_conv3_fwd k{kind} {cin}->{cout} {ho}x{wo}", peak=_aekl_peak(mode))
    return y


def aekl_gn_stats(x, gamma, beta, groups, eps=1e-6):
    """GroupNorm statistics of x (N, C, ...) -> mean, rstd (N, groups), scale = gamma rstd, shift = beta - mean rstd gamma
    (N, C): the folded per-(sample, channel) affine its consumers apply"""
    _chk(x, gamma, beta)
    n, c = x.shape[:2]
    hw = x.numel() // max(1, n * c)
    if groups <= 0 or c % groups or tuple(gamma.shape) != (c,) or tuple(beta.shape) != (c,):
        raise _lib.WfaeError(f"aekl_gn_stats: {c} channels, {groups} groups, affine {tuple(gamma.shape)}")
    mean = torch.empty((n, groups), dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    scale = torch.empty((n, c), dtype=torch.float32, device=x.device)
    shift = torch.empty_like(scale)
    ws = workspace(_lib.load().wfae_aekl_gn_ws_bytes(n, c, hw, groups))
    _call("wfae_aekl_gn_stats", 0, 8 * x.numel(), _p(x), _p(gamma), _p(beta), _p(mean), _p(rstd), _p(scale), _p(shift), n, c,
          hw, groups, float(eps), ws.data_ptr(), ws.numel(), _stream())
    return mean, rstd, scale, shift


def aekl_to_tokens(x, gn=None):
    """x (N, C, H, W) -> tokens (N, H*W, C), optionally through the folded GroupNorm affine gn = (scale, shift)"""
    scale, shift = gn if gn is not None else (None, None)
    _chk(x, scale, shift)
    n, c = x.shape[:2]
    s = x.numel() // (n * c)
    if c % 32 or s % 32:
        raise _lib.WfaeError(f"aekl_to_tokens: C and S = H*W must be multiples of 32 (got C={c} S={s})")
    tok = torch.empty((n, s, c), dtype=torch.float32, device=x.device)
    _call("wfae_aekl_to_tokens", 0, 8 * x.numel(), _p(x), _p(scale), _p(shift), _p(tok), n, c, s, _stream())
    return tok


def aekl_from_tokens(tok, shape, res=None, mul=1.0):
    """tokens (N, S, C) -> (tokens^T + res) * mul in the NCHW `shape`"""
    _chk(tok, res)
    n, s, c = tok.shape
    if c % 32 or s % 32:
        raise _lib.WfaeError(f"aekl_from_tokens: C and S must be multiples of 32 (got C={c} S={s})")
    y = torch.empty(tuple(shape), dtype=torch.float32, device=tok.device)
    if y.numel() != tok.numel() or (res is not None and res.shape != y.shape) or shape[0] != n or shape[1] != c:
        raise _lib.WfaeError(f"aekl_from_tokens: tokens {tuple(tok.shape)} do not fill {tuple(shape)}")
    _call("wfae_aekl_from_tokens", 0, 12 * tok.numel(), _p(tok), _p(res), _p(y), n, c, s, float(mul), _stream())
    return y


def aekl_softmax(x, scale=1.0):
    """softmax(scale * x) over the last dimension"""
    _chk(x)
    cols = x.shape[-1]
    y = torch.empty_like(x)
    _call("wfae_aekl_softmax", 0, 8 * x.numel(), _p(x), _p(y), x.numel() // cols, cols, float(scale), _stream())
    return y


def aekl_posterior(moments, noise=None):
    """moments (N, 2C, H, W) -> mean, logvar (clamped to [-30, 20]), std, sample = mean + std * noise (None without noise)"""
    _chk(moments, noise)
    n, c2, h, wd = moments.shape
    if c2 % 2:
        raise _lib.WfaeError(f"aekl_posterior: {c2} moment channels, expected an even count")
    shp = (n, c2 // 2, h, wd)
    if noise is not None and tuple(noise.shape) != shp:
        raise _lib.WfaeError(f"aekl_posterior: noise {tuple(noise.shape)}, expected {shp}")
    mean, logvar, std = (torch.empty(shp, dtype=torch.float32, device=moments.device) for _ in range(3))
    sample = torch.empty_like(mean) if noise is not None else None
    _call("wfae_aekl_posterior", 0, 4 * moments.numel() * 3, _p(moments), _p(noise), _p(mean), _p(logvar), _p(std),
          _p(sample), n, c2 // 2, h * wd, _stream())
    return mean, logvar, std, sample


def aekl_posterior_seq(moments, noise):
    """moments (B*T, 2C, h, w) of the frames f = b*T + t, noise (T, B, C, h, w) -> z (B, T, C, h, w) = mean + std * noise:
    the sample of aekl_posterior, bit for bit, without its other three outputs and without a permuted copy of the noise"""
    _chk(moments, noise)
    if moments.dim() != 4 or noise.dim() != 5 or moments.shape[1] % 2:
        raise _lib.WfaeError(f"aekl_posterior_seq: expected moments (B*T, 2C, h, w) and noise (T, B, C, h, w), got "
                             f"{tuple(moments.shape)} and {tuple(noise.shape)}")
    t, b = noise.shape[:2]
    n, c2, h, wd = moments.shape
    if (t * b, c2 // 2, h, wd) != (n, *noise.shape[2:]):
        raise _lib.WfaeError(f"aekl_posterior_seq: noise {tuple(noise.shape)} does not fit moments {tuple(moments.shape)}")
    z = torch.empty((b, t, c2 // 2, h, wd), dtype=torch.float32, device=moments.device)
    _call("wfae_aekl_posterior_seq", 0, 4 * moments.numel() * 2, _p(moments), _p(noise), _p(z), b, t, c2 // 2, h * wd, _stream())
    return z


# ---- latent cache (include/wfae.h "latent cache"; csrc/latent_cache.hip)
def _host_i32(name, what, v, lo, hi, device):
    """a HOST list / array / tensor of integers in [lo, hi) -> (the int64 numpy copy that was checked, the int32 device
    tensor built from it).  The kernels trust these values, so they are checked here, where they were made.  The copy goes
    through pinned memory and does not block: a pageable one would make the host wait for the stream, and with it for the
    encoder launches queued in front"""
    if isinstance(v, torch.Tensor):
        if v.is_cuda:
            raise _lib.WfaeError(f"{name}: {what} is checked on the host, pass the host copy (a list, an array or a CPU tensor)")
        v = v.numpy()
    a = np.asarray(v)
    if a.ndim != 1 or a.size == 0 or a.dtype.kind not in "iu":
        raise _lib.WfaeError(f"{name}: {what} must be a non-empty 1-D integer array, got shape {a.shape} of {a.dtype}")
    a = a.astype(np.int64)
    if int(a.min()) < lo or int(a.max()) >= hi:
        raise _lib.WfaeError(f"{name}: {what} in [{int(a.min())}, {int(a.max())}], outside [{lo}, {hi})")
    return a, torch.from_numpy(a.astype(np.int32)).pin_memory().to(device, non_blocking=True)


def latent_scatter(src, slots, table):
    """table[slots[m], :] = src[m, :] for the rows with slots[m] >= 0; slots[m] == -1 skips row m.  src (M, L), table
    (capacity, L) fp32 on the device; `slots`: M host integers in [-1, capacity), no slot twice (rows are written without
    atomics).  Writes into `table`, returns it"""
    _chk(src, table)
    if src.dim() != 2 or table.dim() != 2 or src.shape[1] != table.shape[1] or src.device != table.device:
        raise _lib.WfaeError(f"latent_scatter: expected src (M, L) and table (capacity, L) on one device, got "
                             f"{tuple(src.shape)} and {tuple(table.shape)}")
    m, l = src.shape
    cap = table.shape[0]
    host, dev = _host_i32("latent_scatter", "slots", slots, -1, cap, src.device)
    if host.size != m:
        raise _lib.WfaeError(f"latent_scatter: {host.size} slots for {m} rows")
    used = host[host >= 0]
    if np.unique(used).size != used.size:
        raise _lib.WfaeError("latent_scatter: two rows share a slot")
    _call("wfae_latent_scatter", 0, 8 * used.size * l, _p(src), dev.data_ptr(), _p(table), m, l, cap, _stream())
    return table


def latent_gather(table, fresh, index, shape_bt, noise=None):
    """output frame f = b*T + t reads table[index[f]] if index[f] >= 0, else fresh[-1 - index[f]].  table (capacity, L),
    fresh (M, L) or None (no negative index), `index`: B*T host integers in [-M, capacity), shape_bt = (B, T).
    noise None -> (B, T, L), a copy of the rows.  noise (T, B, C, h, w) with L = 2 C h w: the rows are moments and the result
    is (B, T, C h w) = mean + std * noise, the bits of aekl_posterior_seq on the same moments"""
    _chk(table, fresh, noise)
    b, t = (int(v) for v in shape_bt)
    if table.dim() != 2 or (fresh is not None and (fresh.dim() != 2 or fresh.shape[1] != table.shape[1] or fresh.shape[0] < 1
                                                   or fresh.device != table.device)):
        raise _lib.WfaeError(f"latent_gather: expected table (capacity, L) and fresh (M, L) on one device, got "
                             f"{tuple(table.shape)} and {None if fresh is None else tuple(fresh.shape)}")
    cap, l = table.shape
    m = 0 if fresh is None else fresh.shape[0]
    if b < 1 or t < 1:
        raise _lib.WfaeError(f"latent_gather: shape_bt {(b, t)}")
    host, dev = _host_i32("latent_gather", "index", index, -m, cap, table.device)
    if host.size != b * t:
        raise _lib.WfaeError(f"latent_gather: {host.size} indices for {b} x {t} frames")
    lout = l
    if noise is not None:
        lout = l // 2
        if l % 2 or noise.dim() < 3 or tuple(noise.shape[:2]) != (t, b) or noise.numel() != t * b * lout or noise.device != table.device:
            raise _lib.WfaeError(f"latent_gather: noise {tuple(noise.shape)} does not fit {(t, b)} draws of rows of {l} moments")
    out = torch.empty((b, t, lout), dtype=torch.float32, device=table.device)
    _call("wfae_latent_gather", 0, 4 * b * t * (l + lout + (lout if noise is not None else 0)), _p(table), _p(fresh),
          dev.data_ptr(), _p(noise), _p(out), b, t, l, 0 if noise is None else 1, cap, m, _stream())
    return out


# ---- AutoencoderKL backward (include/wfae.h "AutoencoderKL backward"; csrc/aekl_bwd.hip)
def _aekl_out_plane(kind, h, wd):
    return (h, wd) if kind == 0 else ((h - 2) // 2 + 1, (wd - 2) // 2 + 1) if kind == 1 else (2 * h, 2 * wd)


def _aekl_bwd_args(what, dy, x_shape, kind, gn):
    scale, shift = gn if gn is not None else (None, None)
    if dy.dim() != 4 or len(x_shape) != 4 or kind not in (0, 1, 2):
        raise _lib.WfaeError(f"{what}: expected dy (N, Cout, Ho, Wo), the shape of x (N, Cin, H, W) and kind 0, 1 or 2")
    n, cin, h, wd = x_shape
    if kind == 1 and (h < 2 or wd < 2):
        raise _lib.WfaeError(f"{what}: the stride-2 form needs a plane of at least 2x2, got {h}x{wd}")
    ho, wo = _aekl_out_plane(kind, h, wd)
    if dy.shape[0] != n or tuple(dy.shape[2:]) != (ho, wo):
        raise _lib.WfaeError(f"{what}: dy {tuple(dy.shape)} does not belong to x {tuple(x_shape)} and kind {kind}")
    if gn is not None and (tuple(scale.shape) != (n, cin) or tuple(shift.shape) != (n, cin)):
        raise _lib.WfaeError(f"{what}: prologue scale / shift {tuple(scale.shape)}, expected {(n, cin)}")
    return scale, shift, n, cin, dy.shape[1], h, wd, ho, wo


def aekl_conv3_bwd_data(dy, packed_t, x, gn=None, kind=0, mode=None, x_shape=None):
    """du (x's shape) = conv(dy, rotated / transposed weights) * silu'(x * scale + shift) for gn = (scale, shift), the
    gradient of the forward prologue's pre-activation; gn None: the plain data gradient (x may be None, give x_shape).
    packed_t = aekl_conv3_pack(w.flip(2, 3).transpose(0, 1), mode)"""
    mode = aekl_mode() if mode is None else mode
    x_shape = tuple(x.shape) if x is not None else tuple(x_shape)
    scale, shift, n, cin, cout, h, wd, ho, wo = _aekl_bwd_args("aekl_conv3_bwd_data", dy, x_shape, kind, gn)
    _chk(dy, x, scale, shift)
    if gn is not None and x is None:
        raise _lib.WfaeError("aekl_conv3_bwd_data: the prologue factor needs x")
    want = _lib.load().wfae_aekl_conv3_pack_bytes(cin, cout, mode)
    if want == 0 or packed_t.dtype != torch.uint8 or packed_t.numel() != want or not packed_t.is_cuda:
        raise _lib.WfaeError(f"aekl_conv3_bwd_data: packed weights do not belong to (Cin={cin}, Cout={cout}, 3, 3) mode={mode}")
    du = torch.empty(x_shape, dtype=torch.float32, device=dy.device)
    hg, wg = (2 * h, 2 * wd) if kind == 2 else (h, wd)
    _call("wfae_aekl_conv3_bwd_data", 2 * 9 * n * hg * wg * cin * cout, 4 * (dy.numel() + du.numel() * (2 if gn else 1)) + want,
          _p(dy), packed_t.data_ptr(), _p(x), _p(scale), _p(shift), _p(du), kind, mode, n, cin, cout, h, wd, _stream(),
          label=f"wfae_aekl_conv3_bwd_data k{kind} {cout}->{cin} {ho}x{wo}", peak=_aekl_peak(mode))
    return du


def aekl_conv3_bwd_weight(dy, x, dw, dbias=None, gn=None, kind=0, mode=None):
    """dw (Cout, Cin, 3, 3) = the weight gradient of aekl_conv3_fwd(x, ., gn=gn, kind=kind) under dy, the operand
    SiLU(x * scale + shift) recomputed on the load; dbias (Cout) = sum of dy.  Both written, not accumulated."""
    mode = aekl_mode() if mode is None else mode
    scale, shift, n, cin, cout, h, wd, ho, wo = _aekl_bwd_args("aekl_conv3_bwd_weight", dy, tuple(x.shape), kind, gn)
    _chk(dy, x, scale, shift, dw, dbias)
    if tuple(dw.shape) != (cout, cin, 3, 3) or (dbias is not None and tuple(dbias.shape) != (cout,)):
        raise _lib.WfaeError(f"aekl_conv3_bwd_weight: dw {tuple(dw.shape)}, expected {(cout, cin, 3, 3)} (dbias {(cout,)})")
    need = _lib.load().wfae_aekl_conv3_wgrad_ws_bytes(kind, n, cin, cout, h, wd)
    if need == 0:
        raise _lib.WfaeError(f"aekl_conv3_bwd_weight: unsupported shape N={n} Cin={cin} Cout={cout} {h}x{wd} kind={kind}")
    ws = workspace(need)
    _call("wfae_aekl_conv3_bwd_weight", 2 * 9 * n * ho * wo * cin * cout, 4 * (dy.numel() + x.numel() + dw.numel()) + 2 * need,
          _p(dy), _p(x), _p(scale), _p(shift), _p(dw), _p(dbias), kind, mode, n, cin, cout, h, wd, ws.data_ptr(), ws.numel(),
          _stream(), label=f"wfae_aekl_conv3_bwd_weight k{kind} {cin}->{cout} {ho}x{wo}", peak=_aekl_peak(mode))
    return dw


def aekl_gn_bwd(du, x, gamma, mean, rstd, skip=None):
    """GroupNorm backward: du = gradient of gamma xhat + beta -> (dx (+ skip), dgamma, dbeta)"""
    _chk(du, x, gamma, mean, rstd, skip)
    n, c = x.shape[:2]
    hw = x.numel() // max(1, n * c)
    groups = mean.shape[1]
    if du.shape != x.shape or tuple(gamma.shape) != (c,) or tuple(mean.shape) != (n, groups) or rstd.shape != mean.shape \
            or c % groups or (skip is not None and skip.shape != x.shape):
        raise _lib.WfaeError(f"aekl_gn_bwd: du {tuple(du.shape)}, x {tuple(x.shape)}, gamma {tuple(gamma.shape)}, "
                             f"mean {tuple(mean.shape)}")
    dx = torch.empty_like(x)
    dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
    ws = workspace(_lib.load().wfae_aekl_gn_bwd_ws_bytes(n, c, groups))
    _call("wfae_aekl_gn_bwd", 0, 4 * x.numel() * (6 if skip is not None else 5), _p(du), _p(x), _p(gamma), _p(mean), _p(rstd),
          _p(skip), _p(dx), _p(dgamma), _p(dbeta), n, c, hw, groups, ws.data_ptr(), ws.numel(), _stream())
    return dx, dgamma, dbeta


def aekl_softmax_bwd(p, dp, scale=1.0):
    """ds = p (dp - sum_j p_j dp_j) scale for p = softmax(scale * s) over the last dimension"""
    _chk(p, dp)
    if p.shape != dp.shape:
        raise _lib.WfaeError(f"aekl_softmax_bwd: p {tuple(p.shape)} and dp {tuple(dp.shape)} differ")
    cols = p.shape[-1]
    ds = torch.empty_like(p)
    _call("wfae_aekl_softmax_bwd", 0, 12 * p.numel(), _p(p), _p(dp), _p(ds), p.numel() // cols, cols, float(scale), _stream())
    return ds


def aekl_posterior_bwd(moments, dz=None, noise=None, gkl=None):
    """dmoments (N, 2C, H, W) of sample = mean + std * noise (noise None: the mean) under dz and of the per-sample KL under
    gkl (N)"""
    _chk(moments, dz, noise, gkl)
    n, c2, h, wd = moments.shape
    shp = (n, c2 // 2, h, wd)
    if c2 % 2 or any(t is not None and tuple(t.shape) != shp for t in (dz, noise)) or (noise is not None and dz is None) \
            or (gkl is not None and gkl.numel() != n):
        raise _lib.WfaeError(f"aekl_posterior_bwd: moments {tuple(moments.shape)} need dz / noise {shp} and gkl ({n},)")
    dmom = torch.empty_like(moments)
    _call("wfae_aekl_posterior_bwd", 0, 4 * moments.numel() * 3, _p(dz), _p(noise), _p(moments), _p(gkl), _p(dmom), n, c2 // 2,
          h * wd, _stream())
    return dmom


# ---- LPIPS perceptual loss (include/wfae.h "LPIPS perceptual loss"; csrc/lpips.hip).  The conv shares the packed weights
# and the modes of the AutoencoderKL 3x3 kernel: pack with aekl_conv3_pack.
def _lpips_packed(what, packed, cout, cin, mode):
    want = _lib.load().wfae_aekl_conv3_pack_bytes(cout, cin, mode)
    if want == 0 or packed.dtype != torch.uint8 or packed.numel() != want or not packed.is_cuda:
        raise _lib.WfaeError(f"{what}: packed weights do not belong to Cout={cout} Cin={cin} mode={mode}")
    return want


def lpips_conv3_fwd(x, packed, bias, mode=None):
    """relu(conv3x3(x, stride 1, pad 1) + bias); packed = aekl_conv3_pack(w (Cout, Cin, 3, 3), mode)"""
    mode = aekl_mode() if mode is None else mode
    _chk(x, bias)
    if x.dim() != 4 or bias is None or bias.dim() != 1:
        raise _lib.WfaeError("lpips_conv3_fwd: expected x (N, C, H, W) and bias (Cout,)")
    n, cin, h, wd = x.shape
    cout = bias.shape[0]
    want = _lpips_packed("lpips_conv3_fwd", packed, cout, cin, mode)
    y = torch.empty((n, cout, h, wd), dtype=torch.float32, device=x.device)
    _call("wfae_lpips_conv3_fwd", 2 * 9 * n * h * wd * cin * cout, 4 * (x.numel() + y.numel()) + want, _p(x),
          packed.data_ptr(), _p(bias), _p(y), mode, n, cin, cout, h, wd, _stream(),
          label=f"wfae_lpips_conv3_fwd {cin}->{cout} {h}x{wd}", peak=_aekl_peak(mode))
    return y


def lpips_conv3_bwd_data(dy, packed_t, cin, a_prev=None, mode=None):
    """dx (N, cin, H, W) = conv3x3(dy, rotated / transposed weights) * (a_prev > 0);
    packed_t = aekl_conv3_pack(w.flip(2, 3).transpose(0, 1), mode)"""
    mode = aekl_mode() if mode is None else mode
    _chk(dy, a_prev)
    if dy.dim() != 4:
        raise _lib.WfaeError(f"lpips_conv3_bwd_data: expected dy (N, C, H, W), got {tuple(dy.shape)}")
    n, cout, h, wd = dy.shape
    want = _lpips_packed("lpips_conv3_bwd_data", packed_t, cin, cout, mode)
    if a_prev is not None and tuple(a_prev.shape) != (n, cin, h, wd):
        raise _lib.WfaeError(f"lpips_conv3_bwd_data: a_prev {tuple(a_prev.shape)}, expected {(n, cin, h, wd)}")
    dx = torch.empty((n, cin, h, wd), dtype=torch.float32, device=dy.device)
    _call("wfae_lpips_conv3_bwd_data", 2 * 9 * n * h * wd * cin * cout,
          4 * (dy.numel() + dx.numel() * (2 if a_prev is not None else 1)) + want, _p(dy), packed_t.data_ptr(), _p(a_prev),
          _p(dx), mode, n, cin, cout, h, wd, _stream(), label=f"wfae_lpips_conv3_bwd_data {cout}->{cin} {h}x{wd}",
          peak=_aekl_peak(mode))
    return dx


def lpips_pool_fwd(x):
    """2 x 2 stride-2 max-pool, floor on odd sizes"""
    _chk(x)
    if x.dim() != 4 or x.shape[2] < 2 or x.shape[3] < 2:
        raise _lib.WfaeError(f"lpips_pool_fwd: expected (N, C, H >= 2, W >= 2), got {tuple(x.shape)}")
    n, c, h, wd = x.shape
    y = torch.empty((n, c, h // 2, wd // 2), dtype=torch.float32, device=x.device)
    _call("wfae_lpips_pool_fwd", 0, 4 * (x.numel() + y.numel()), _p(x), _p(y), n, c, h, wd, _stream())
    return y


def lpips_pool_bwd(a, dy, add=None):
    """gradient of the pre-activation of the pool's input a (post-ReLU): torch's max-pool routing of dy, + add, * (a > 0)"""
    _chk(a, dy, add)
    if a.dim() != 4 or a.shape[2] < 2 or a.shape[3] < 2:
        raise _lib.WfaeError(f"lpips_pool_bwd: expected a (N, C, H >= 2, W >= 2), got {tuple(a.shape)}")
    n, c, h, wd = a.shape
    if tuple(dy.shape) != (n, c, h // 2, wd // 2) or (add is not None and add.shape != a.shape):
        raise _lib.WfaeError(f"lpips_pool_bwd: dy {tuple(dy.shape)} / add do not belong to a {tuple(a.shape)}")
    dpre = torch.empty_like(a)
    _call("wfae_lpips_pool_bwd", 0, 4 * (a.numel() * (3 if add is not None else 2) + dy.numel()), _p(a), _p(dy), _p(add),
          _p(dpre), n, c, h, wd, _stream())
    return dpre


def _lpips_dist_args(what, a0, a1, lin):
    _chk(a0, a1, lin)
    if a0.dim() != 4 or a1.shape != a0.shape or lin.numel() != a0.shape[1]:
        raise _lib.WfaeError(f"{what}: a0 {tuple(a0.shape)}, a1 {tuple(a1.shape)}, lin {tuple(lin.shape)}")
    if a0.shape[1] not in (64, 128, 256, 512):
        raise _lib.WfaeError(f"{what}: {a0.shape[1]} channels, served are 64, 128, 256 and 512")
    return a0.shape[0], a0.shape[1], a0.shape[2] * a0.shape[3]


def lpips_dist_fwd(a0, a1, lin, out):
    """out (N) += mean over pixels of sum_c lin[c] (a0 / (||a0|| + 1e-10) - a1 / (||a1|| + 1e-10))^2, in place"""
    n, c, hw = _lpips_dist_args("lpips_dist_fwd", a0, a1, lin)
    _chk(out)
    if out.numel() != n:
        raise _lib.WfaeError(f"lpips_dist_fwd: out {tuple(out.shape)}, expected {n} values")
    ws = workspace(_lib.load().wfae_lpips_dist_ws_bytes(n, hw))
    _call("wfae_lpips_dist_fwd", 0, 8 * a0.numel(), _p(a0), _p(a1), _p(lin), _p(out), n, c, hw, ws.data_ptr(), ws.numel(),
          _stream())
    return out


def lpips_dist_bwd(a0, a1, lin, g, relu=False):
    """g[n] * d(the layer's term of sample n) / d a0; relu: times (a0 > 0).  Finite at an all-zero pixel of a0 (wfae.h)."""
    n, c, hw = _lpips_dist_args("lpips_dist_bwd", a0, a1, lin)
    _chk(g)
    if g.numel() != n:
        raise _lib.WfaeError(f"lpips_dist_bwd: g {tuple(g.shape)}, expected {n} values")
    da0 = torch.empty(a0.shape, dtype=torch.float32, device=a0.device)
    _call("wfae_lpips_dist_bwd", 0, 12 * a0.numel(), _p(a0), _p(a1), _p(lin), _p(g), _p(da0), n, c, hw, int(bool(relu)),
          _stream())
    return da0


def lpips_prep_fwd(x, shift, scale, out=None):
    """(x - shift[c]) / scale[c] into 3 channels from a 1- or 3-channel x (N, Cx, H, W); `out`: where to write (N, 3, H, W)"""
    _chk(x, shift, scale, out)
    if x.dim() != 4 or x.shape[1] not in (1, 3) or shift.numel() != 3 or scale.numel() != 3:
        raise _lib.WfaeError(f"lpips_prep_fwd: expected x (N, 1 or 3, H, W) and 3 shifts / scales, got {tuple(x.shape)}")
    n, cx, h, wd = x.shape
    if out is None:
        out = torch.empty((n, 3, h, wd), dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (n, 3, h, wd):
        raise _lib.WfaeError(f"lpips_prep_fwd: out {tuple(out.shape)}, expected {(n, 3, h, wd)}")
    _call("wfae_lpips_prep_fwd", 0, 4 * (x.numel() + out.numel()), _p(x), _p(shift), _p(scale), _p(out), n, cx, h * wd, _stream())
    return out


def lpips_prep_bwd(dy, scale, cx):
    """dx (N, cx, H, W) of lpips_prep_fwd"""
    _chk(dy, scale)
    if dy.dim() != 4 or dy.shape[1] != 3 or cx not in (1, 3) or scale.numel() != 3:
        raise _lib.WfaeError(f"lpips_prep_bwd: expected dy (N, 3, H, W), cx 1 or 3, got {tuple(dy.shape)}, cx={cx}")
    n, _, h, wd = dy.shape
    dx = torch.empty((n, cx, h, wd), dtype=torch.float32, device=dy.device)
    _call("wfae_lpips_prep_bwd", 0, 4 * (dy.numel() + dx.numel()), _p(dy), _p(scale), _p(dx), n, cx, h * wd, _stream())
    return dx


def _chk_planes(what, a, b):
    """the two images of an image metric: one shape, (N, ..., H, W)"""
    if a.shape != b.shape:
        raise _lib.WfaeError(f"{what}: shapes {tuple(a.shape)} and {tuple(b.shape)} differ")
    if a.dim() < 3:
        raise _lib.WfaeError(f"{what}: expected (N, ..., H, W), got {tuple(a.shape)}")


def ssim_fwd(x, y, clamp01=False):
    _chk(x, y)
    _chk_planes("ssim_fwd", x, y)
    h, wd = x.shape[-2:]
    nb = math.prod(x.shape[:-2])
    out = torch.empty((), dtype=torch.float32, device=x.device)
    ws = workspace()
    _call("wfae_ssim_fwd", 0, 8 * x.numel(), _p(x), _p(y), _p(out), nb, h, wd, int(clamp01), ws.data_ptr(), ws.numel(), _stream())
    return out


def ssim_bwd(x, y, gout):
    _chk(x, y, gout)
    _chk_planes("ssim_bwd", x, y)
    h, wd = x.shape[-2:]
    nb = math.prod(x.shape[:-2])
    dy = torch.empty_like(y)
    ws = workspace(3 * nb * (h - 10) * (wd - 10) * 4)
    _call("wfae_ssim_bwd", 0, 12 * x.numel(), _p(x), _p(y), _p(gout), _p(dy), nb, h, wd, ws.data_ptr(), ws.numel(), _stream())
    return dy


def psnr(pred, target, clamp01=False):
    _chk(pred, target)
    _chk_planes("psnr", pred, target)
    nb = pred.shape[0]
    hw = pred.numel() // nb
    out = torch.empty((), dtype=torch.float32, device=pred.device)
    ws = workspace()
    _call("wfae_psnr", 0, 8 * pred.numel(), _p(pred), _p(target), _p(out), nb, hw, int(clamp01), ws.data_ptr(), ws.numel(), _stream())
    return out


# ------------------------------------------------------- forecast-skill scores (csrc/skill.hip)
POOL_TYPES = {"none": 0, "avg": 1, "max": 2}


def skill_scores(pred, target, thresholds, pools, clamp01=False):
    """Contingency counts and CRPS sums of pipeline/metrics.py:9-68 in one pass.

    pred (B, T, C, H, W) or an ensemble (B, N, T, C, H, W), target (B, T, C, H, W), both fp32; thresholds: up to 8
    floats (compared in fp32, like `tensor >= python_float`); pools: up to 3 (type, scale) pairs, type in
    'none' / 'avg' / 'max'.  -> int64 device tensor (len(pools), 3 * len(thresholds) + 2): per pool [tp, fn, fp] per
    threshold (on the ensemble mean), the CRPS sum over pooled cells as the bits of a float64, the pooled cell count."""
    _chk(pred, target)
    if pred.dim() == 5:
        b, t, c, h, w = pred.shape
        n = 1
    elif pred.dim() == 6:
        b, n, t, c, h, w = pred.shape
    else:
        raise _lib.WfaeError(f"skill_scores: pred must be 5-D or 6-D, got {tuple(pred.shape)}")
    if tuple(target.shape) != (b, t, c, h, w):
        raise _lib.WfaeError(f"skill_scores: target {tuple(target.shape)} does not match pred {tuple(pred.shape)}")
    if pred.dtype != torch.float32 or target.dtype != torch.float32:
        raise _lib.WfaeError("skill_scores: fp32 tensors only")
    if not (pred.is_contiguous() and target.is_contiguous()):
        raise _lib.WfaeError("skill_scores: contiguous tensors only")
    thr = (ctypes.c_float * max(1, len(thresholds)))(*[float(x) for x in thresholds])
    types = (ctypes.c_int * max(1, len(pools)))(*[POOL_TYPES[p] for p, _ in pools])
    scales = (ctypes.c_int * max(1, len(pools)))(*[int(s) for _, s in pools])
    out = torch.empty((len(pools), 3 * len(thresholds) + 2), dtype=torch.int64, device=pred.device)
    ws = workspace()
    _call("wfae_skill_scores", 0, 4 * (pred.numel() + target.numel()), _p(pred), _p(target), _p(out), b, n, t * c, h,
          w, ctypes.addressof(thr), len(thresholds), ctypes.addressof(types), ctypes.addressof(scales), len(pools),
          int(clamp01), ws.data_ptr(), ws.numel(), _stream())
    return out


def ensemble_mean(pred, clamp01=False):
    """pred (B, N, ...) -> (B, ...): pred.mean(dim=1) in torch's order (sequential sum over N, then / N); clamp01
    clamps every member to [0, 1] first."""
    _chk(pred)
    if pred.dtype != torch.float32 or not pred.is_contiguous() or pred.dim() < 2:
        raise _lib.WfaeError("ensemble_mean: contiguous fp32 tensor (B, N, ...) only")
    b, n = pred.shape[:2]
    out = torch.empty((b,) + tuple(pred.shape[2:]), dtype=torch.float32, device=pred.device)
    inner = out.numel() // b
    _call("wfae_ensemble_mean", 0, 4 * (pred.numel() + out.numel()), _p(pred), _p(out), b, n, inner, int(clamp01),
          _stream())
    return out


# ------------------------------------------------------- verification per lead time (csrc/verify.hip)
def _frame_strides(name, t, lead_dims, b, p, s):
    """(sample stride, lead stride) in elements of the view `t`, whose first `lead_dims` axes are (B,) or (B, P or 1) and
    whose other axes are one frame of `s` contiguous pixels"""
    want = 1
    for size, stride in zip(reversed(t.shape[lead_dims:]), reversed(t.stride()[lead_dims:])):
        if size > 1 and stride != want:
            raise _lib.WfaeError(f"verify_leads: {name}: a frame must be contiguous, got shape {tuple(t.shape)} with "
                                 f"strides {t.stride()}")
        want *= size
    bs = t.stride(0) if b > 1 else 0
    ls = t.stride(1) if lead_dims == 2 and t.shape[1] > 1 else 0
    return bs, ls


def verify_leads(fields, target, thresholds, clamp01=True, out=None):
    """Scores per lead time of up to 4 fields against one target in one launch pair, from views (nothing is copied).

    target (B, P, ...): P leads of frames with S = prod(...) contiguous pixels each, e.g. `frames[:, L:]` of a loader
    batch.  Every field has the same B and S per frame and is (B, P, ...), or (B, 1, ...) / (B, ...) for one frame held
    against every lead (lead stride 0: persistence, `frames[:, L - 1]`); the frame axes may be spelled differently
    ((H, W) against (1, H, W)).  thresholds: up to 8 floats, events are `value >= threshold` in fp32; clamp01 clamps both
    sides to [0, 1] first.  -> (counts int64 (P, F, 3 * len(thresholds) + 1): [tp, fn, fp] per threshold, then the cells of
    the lead; sums float64 (P, F, 2): sum of e^2 and of |e|, e = field - target in fp64).  out=(counts, sums): the call
    adds to these tables and returns them.  No host synchronisation; the same inputs give the same bits."""
    fields = list(fields)
    if not 1 <= len(fields) <= 4:
        raise _lib.WfaeError(f"verify_leads: 1 to 4 fields, got {len(fields)}")
    if len(thresholds) > 8:
        raise _lib.WfaeError(f"verify_leads: at most 8 thresholds, got {len(thresholds)}")
    for name, t in [("target", target)] + [(f"field {i}", f) for i, f in enumerate(fields)]:
        if not t.is_cuda:
            raise _lib.WfaeError("wfae kernels need device tensors (the HIP path has no CPU fallback)")
        if t.dtype != torch.float32:
            raise _lib.WfaeError(f"verify_leads: {name} must be fp32, got {t.dtype}")
        if t.device != target.device:
            raise _lib.WfaeError(f"verify_leads: {name} is on {t.device}, the target on {target.device}")
    if target.dim() < 3:
        raise _lib.WfaeError(f"verify_leads: target must be (B, P, ...), got {tuple(target.shape)}")
    b, p = target.shape[:2]
    s = math.prod(target.shape[2:])
    if b < 1 or p < 1 or s < 1:
        raise _lib.WfaeError(f"verify_leads: empty target {tuple(target.shape)}")
    tb, tl = _frame_strides("target", target, 2, b, p, s)
    ptrs, bstr, lstr, moved = [], [], [], target.numel()
    for i, f in enumerate(fields):
        shape = tuple(f.shape)
        if f.dim() >= 3 and shape[0] == b and shape[1] in (p, 1) and math.prod(shape[2:]) == s:
            lead_dims = 2
        elif f.dim() >= 2 and shape[0] == b and math.prod(shape[1:]) == s:
            lead_dims = 1
        else:
            raise _lib.WfaeError(f"verify_leads: field {i} {shape} does not match the target {tuple(target.shape)}: "
                                 f"expected ({b}, {p}, ...), ({b}, 1, ...) or ({b}, ...) with {s} pixels per frame")
        bs, ls = _frame_strides(f"field {i}", f, lead_dims, b, p, s)
        ptrs.append(f.data_ptr())
        bstr.append(bs)
        lstr.append(ls)
        moved += b * s * (p if ls else 1)
    nf, nt = len(fields), len(thresholds)
    if out is None:
        counts = torch.empty((p, nf, 3 * nt + 1), dtype=torch.int64, device=target.device)
        sums = torch.empty((p, nf, 2), dtype=torch.float64, device=target.device)
    else:
        counts, sums = out
        for t, dt, shape in ((counts, torch.int64, (p, nf, 3 * nt + 1)), (sums, torch.float64, (p, nf, 2))):
            if t.dtype != dt or tuple(t.shape) != shape or t.device != target.device or not t.is_contiguous():
                raise _lib.WfaeError(f"verify_leads: out must hold a contiguous {dt} tensor of shape {shape} on "
                                     f"{target.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    fp = (ctypes.c_void_p * nf)(*ptrs)
    fb = (ctypes.c_int64 * nf)(*bstr)
    fl = (ctypes.c_int64 * nf)(*lstr)
    thr = (ctypes.c_float * max(1, nt))(*[float(x) for x in thresholds])
    ws = workspace(p * min(256, -(-b * s // 1024)) * nf * (3 * nt + 2) * 8)
    _call("wfae_verify_leads", 0, 4 * moved, ctypes.addressof(fp), ctypes.addressof(fb), ctypes.addressof(fl),
          target.data_ptr(), tb, tl, nf, b, p, s, ctypes.addressof(thr), nt, int(clamp01), int(out is not None),
          counts.data_ptr(), sums.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    return counts, sums


# ------------------------------------------------------- latent transformer
def layernorm_fwd(x, res, gamma, beta, eps=1e-5):
    _chk(x, res, gamma, beta)
    rows, e = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    _call("wfae_layernorm_fwd", 0, 12 * x.numel(), _p(x), _p(res), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), rows,
          e, eps, _stream())
    return y, mean, rstd


def layernorm_bwd(dy, x, res, gamma, mean, rstd, dgamma, dbeta, accumulate=False):
    _chk(dy, x, res, gamma, mean, rstd, dgamma, dbeta)
    rows, e = x.shape
    dx = torch.empty_like(x)
    ws = workspace()
    _call("wfae_layernorm_bwd", 0, 16 * x.numel(), _p(dy), _p(x), _p(res), _p(gamma), _p(mean), _p(rstd), _p(dx),
          _p(dgamma), _p(dbeta), rows, e, int(accumulate), ws.data_ptr(), ws.numel(), _stream())
    return dx


def mha_fwd(qkv, s, n, h, d, p_drop=0.0, seed=0, batch_first=False):
    """attention over the s axis for each of n sequences; rows of qkv: s*n+… (seq-first) or n*s+… (batch-first)"""
    _chk(qkv)
    out = torch.empty((s * n, h * d), dtype=torch.float32, device=qkv.device)
    probs = torch.empty((n, h, s, s), dtype=torch.float32, device=qkv.device)
    _call("wfae_mha_fwd", 4 * n * h * s * s * d, 4 * (qkv.numel() + out.numel()), _p(qkv), _p(out), _p(probs),
          s, n, h, d, int(batch_first), p_drop, seed, _stream())
    return out, probs


def mha_bwd(qkv, probs, dout, s, n, h, d, p_drop=0.0, seed=0, batch_first=False):
    _chk(qkv, probs, dout)
    dqkv = torch.empty_like(qkv)
    _call("wfae_mha_bwd", 8 * n * h * s * s * d, 8 * qkv.numel(), _p(qkv), _p(probs), _p(dout), _p(dqkv), s, n,
          h, d, int(batch_first), p_drop, seed, _stream())
    return dqkv


# --------------------------------------------------- AE_ViT_2048 (Path-B)
def patchify(img, patch):
    """(B,C,H,W) -> (B*Hp*Wp, C*P*P)"""
    _chk(img)
    b, c, h, w = img.shape
    hp, wp = h // patch, w // patch
    rows = torch.empty((b * hp * wp, c * patch * patch), dtype=torch.float32, device=img.device)
    _call("wfae_patchify", 0, 8 * img.numel(), _p(img), _p(rows), b, c, hp, wp, patch, _stream())
    return rows


def unpatchify(rows, bias, b, c, hp, wp, patch):
    """(B*Hp*Wp, C*P*P) (+ bias[c]) -> (B,C,Hp*P,Wp*P)"""
    _chk(rows, bias)
    img = torch.empty((b, c, hp * patch, wp * patch), dtype=torch.float32, device=rows.device)
    _call("wfae_unpatchify", 0, 8 * img.numel(), _p(rows), _p(bias), _p(img), b, c, hp, wp, patch, _stream())
    return img


def add_bcast(x, p):
    """x (outer, *inner) + p (*inner)"""
    _chk(x, p)
    out = torch.empty_like(x)
    inner = p.numel()
    _call("wfae_add_bcast", 0, 8 * x.numel(), _p(x), _p(p), _p(out), x.numel() // inner, inner, _stream())
    return out


def copy_rows(src, rows, cols, src_ld, src_off=0, row_div=1, dst_ld=None, dst_off=0, zero_fill=False):
    """dst (rows, dst_ld): dst[r][dst_off + c] = src[(r // row_div) * src_ld + src_off + c] (see wfae_copy_rows)"""
    _chk(src)
    dst_ld = cols if dst_ld is None else dst_ld
    dst = torch.empty((rows, dst_ld), dtype=torch.float32, device=src.device)
    _call("wfae_copy_rows", 0, 4 * rows * (cols + dst_ld), _p(src), _p(dst), rows, cols, src_ld, src_off, row_div, dst_ld,
          dst_off, int(zero_fill), _stream())
    return dst


def sum_mid(x, a, m, bn):
    """x viewed as (a, m, bn) -> (a, bn)"""
    _chk(x)
    out = torch.empty((a, bn), dtype=torch.float32, device=x.device)
    _call("wfae_sum_mid", 0, 4 * x.numel(), _p(x), _p(out), a, m, bn, _stream())
    return out


def sq_attn_fwd(q, kv, b, l, h, d):
    _chk(q, kv)
    out = torch.empty((b, h * d), dtype=torch.float32, device=q.device)
    probs = torch.empty((b, h, l), dtype=torch.float32, device=q.device)
    _call("wfae_sq_attn_fwd", 4 * b * h * l * d, 4 * (kv.numel() + q.numel()), _p(q), _p(kv), _p(out), _p(probs), b, l, h, d, _stream())
    return out, probs


def sq_attn_bwd(q, kv, probs, dout, b, l, h, d):
    _chk(q, kv, probs, dout)
    dq, dkv = torch.empty_like(q), torch.empty_like(kv)
    _call("wfae_sq_attn_bwd", 8 * b * h * l * d, 8 * kv.numel(), _p(q), _p(kv), _p(probs), _p(dout), _p(dq), _p(dkv), b, l, h, d, _stream())
    return dq, dkv


def relu_fwd(x):
    _chk(x)
    y = torch.empty_like(x)
    _call("wfae_relu_fwd", 0, 8 * x.numel(), _p(x), _p(y), x.numel(), _stream())
    return y


def relu_bwd(dy, y):
    _chk(dy, y)
    dx = torch.empty_like(dy)
    _call("wfae_relu_bwd", 0, 12 * y.numel(), _p(dy), _p(y), _p(dx), y.numel(), _stream())
    return dx


def dropout(x, p_drop, seed):
    _chk(x)
    y = torch.empty_like(x)
    _call("wfae_dropout", 0, 8 * x.numel(), _p(x), _p(y), x.numel(), p_drop, seed, _stream())
    return y


# ---------------------------------------------------------------- optimiser
def adamw_(p, g, m, v, lr, beta1, beta2, eps, wd, bc1, bc2, grad_scale=1.0, exact_complements=False):
    """exact_complements: 1 - beta formed from the Python doubles and rounded once, as torch does (wfae_adamw_c); the
    default forms them in fp32 from the rounded betas (1.f - 0.999f is 1.3e-5 short of 0.001)"""
    _chk(p, g, m, v)
    if exact_complements:
        _call("wfae_adamw_c", 0, 28 * p.numel(), _p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, 1.0 - beta1,
              1.0 - beta2, eps, wd, bc1, bc2, grad_scale, _stream(), label="wfae_adamw")
        return
    _call("wfae_adamw", 0, 28 * p.numel(), _p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, wd, bc1, bc2, grad_scale,
              _stream())


def sumsq(x):
    _chk(x)
    out = torch.empty((), dtype=torch.float64, device=x.device)
    ws = workspace()
    _call("wfae_sumsq", 0, 4 * x.numel(), _p(x), x.numel(), _p(out), ws.data_ptr(), ws.numel(), _stream())
    return out


def sumsq_into(x, out_slot):
    """sum of squares of x written into a 0-dim fp64 view (one slot of a parts vector)"""
    _chk(x)
    ws = workspace()
    _call("wfae_sumsq", 0, 4 * x.numel(), _p(x), x.numel(), _p(out_slot), ws.data_ptr(), ws.numel(), _stream())


def clip_coef(parts, max_norm, pre_scale=1.0):
    """(coef, total_norm) device pair from fp64 partial sums of squares"""
    out = torch.empty(2, dtype=torch.float32, device=parts.device)
    _call("wfae_clip_coef", 0, 0, _p(parts), parts.numel(), float(max_norm), float(pre_scale), _p(out), _stream())
    return out


def adaptive_weight(ss_rec, ss_disc, disc_weight=1.0):
    out = torch.empty((), dtype=torch.float32, device=ss_rec.device)
    _call("wfae_adaptive_weight", 0, 0, _p(ss_rec), _p(ss_disc), float(disc_weight), _p(out), _stream())
    return out


def vil_u8_to_f32(src_nhwt, scale=1.0 / 255.0):
    """uint8 (N,H,W,T) -> fp32 (N,T,H,W) * scale: the loader contract on device."""
    if src_nhwt.dtype != torch.uint8 or not src_nhwt.is_cuda or not src_nhwt.is_contiguous():
        raise _lib.WfaeError("vil_u8_to_f32 needs a contiguous uint8 device tensor")
    n, h, w, t = src_nhwt.shape
    dst = torch.empty((n, t, h, w), dtype=torch.float32, device=src_nhwt.device)
    _call("wfae_vil_u8_to_f32", 0, 5 * dst.numel(), src_nhwt.data_ptr(), _p(dst), n, h, w, t, scale, _stream())
    return dst


def vil_augment_u8_to_f32(src_nhwt, xf, scale=1.0 / 255.0):
    """uint8 (N,H,W,T) -> fp32 (N,T,H,W) * scale with one flip + nearest-neighbour rotation per sample in the same
    pass; xf: fp32 (N,4) device rows (cos, sin, hflip, vflip) — include/wfae.h states the formula."""
    if src_nhwt.dtype != torch.uint8 or not src_nhwt.is_cuda or not src_nhwt.is_contiguous() or src_nhwt.dim() != 4:
        raise _lib.WfaeError("vil_augment_u8_to_f32 needs a contiguous uint8 (N,H,W,T) device tensor")
    n, h, w, t = src_nhwt.shape
    if (xf.dtype != torch.float32 or not xf.is_contiguous() or tuple(xf.shape) != (n, 4)
            or xf.device != src_nhwt.device):
        raise _lib.WfaeError(f"vil_augment_u8_to_f32 needs contiguous fp32 transform rows of shape ({n}, 4) on "
                             f"{src_nhwt.device}")
    dst = torch.empty((n, t, h, w), dtype=torch.float32, device=src_nhwt.device)
    _call("wfae_vil_augment_u8_to_f32", 0, 5 * dst.numel(), src_nhwt.data_ptr(), xf.data_ptr(), _p(dst), n, h, w, t,
          scale, _stream())
    return dst


_POOL_MODES = {"max": 0, "mean": 1}


def vil_pool_u8_to_f32(src_nhwt, factors, mode="max", xf=None, scale=1.0 / 255.0, offset=0.0):
    """uint8 (N,H,W,T) -> fp32 (N,To,Ho,Wo) = scale * (u8 + offset) of every ft-th frame, pooled over fh x fw blocks:
    mode "max" (ceil sizes; factors (2, 3, 3) make sevir_lr from raw SEVIR) or "mean" (floor sizes, avg_pool2d).  xf: None,
    or the fp32 (N,4) rows of vil_augment_u8_to_f32, applied on the pooled grid — include/wfae.h states the arithmetic."""
    if src_nhwt.dtype != torch.uint8 or not src_nhwt.is_cuda or not src_nhwt.is_contiguous() or src_nhwt.dim() != 4:
        raise _lib.WfaeError("vil_pool_u8_to_f32 needs a contiguous uint8 (N,H,W,T) device tensor")
    if mode not in _POOL_MODES:
        raise _lib.WfaeError(f"vil_pool_u8_to_f32: mode {mode!r}, not one of {sorted(_POOL_MODES)}")
    try:
        ft, fh, fw = (int(f) for f in factors)
    except (TypeError, ValueError):
        raise _lib.WfaeError(f"vil_pool_u8_to_f32 needs three integer factors (t, h, w), got {factors!r}") from None
    n, h, w, t = src_nhwt.shape
    if min(ft, fh, fw) < 1 or (mode == "mean" and (fh > h or fw > w)):
        raise _lib.WfaeError(f"vil_pool_u8_to_f32: factors {(ft, fh, fw)} on frames of {h} x {w}, mode {mode}")
    if xf is not None and (xf.dtype != torch.float32 or not xf.is_contiguous() or tuple(xf.shape) != (n, 4)
                           or xf.device != src_nhwt.device):
        raise _lib.WfaeError(f"vil_pool_u8_to_f32 needs contiguous fp32 transform rows of shape ({n}, 4) on "
                             f"{src_nhwt.device}")
    to = -(-t // ft)
    ho, wo = (-(-h // fh), -(-w // fw)) if mode == "max" else (h // fh, w // fw)
    dst = torch.empty((n, to, ho, wo), dtype=torch.float32, device=src_nhwt.device)
    if dst.numel() == 0:
        return dst
    _call("wfae_vil_pool_u8_to_f32", 0, src_nhwt.numel() + 4 * dst.numel(), src_nhwt.data_ptr(),
          None if xf is None else xf.data_ptr(), _p(dst), n, h, w, t, ft, fh, fw, _POOL_MODES[mode], scale, offset,
          _stream())
    return dst


# ---- conv + attention latent autoencoder (include/wfae.h "conv + attention latent autoencoder"; csrc/convattn.hip)
ATTN_MAX_S, ATTN_D, GN_MAX_GROUP = 256, 16, 16384


def _attn_views(what, q, k, v, n, sq, skv, h, d):
    """row-sliced column views of one projection buffer: 2-D, fp32, unit column stride, (n * s) rows of h * d columns"""
    e = h * d
    for name, t, s in (("q", q, sq), ("k", k, skv), ("v", v, skv)):
        if not t.is_cuda:
            raise _lib.WfaeError("wfae kernels need device tensors (the HIP path has no CPU fallback)")
        if t.dtype != torch.float32:
            raise _lib.WfaeError(f"wfae kernels are fp32, got {t.dtype}")
        if t.dim() != 2 or tuple(t.shape) != (n * s, e) or t.stride(1) != 1 or t.stride(0) < e:
            raise _lib.WfaeError(f"{what}: {name} of shape {tuple(t.shape)} / strides {tuple(t.stride())}, expected "
                                 f"({n * s}, {e}) rows with unit column stride")


def attn_fwd(q, k, v, n, sq, skv, h, d, p_drop=0.0, seed=0):
    """q (n*sq, h*d), k, v (n*skv, h*d): contiguous tensors or column slices of a packed projection (row stride = the packed
    width) -> (out (n*sq, h*d), probs (n, h, sq, skv) before dropout)"""
    _attn_views("attn_fwd", q, k, v, n, sq, skv, h, d)
    out = torch.empty((n * sq, h * d), dtype=torch.float32, device=q.device)
    probs = torch.empty((n, h, sq, skv), dtype=torch.float32, device=q.device)
    _call("wfae_attn_fwd", 4 * n * h * sq * skv * d, 4 * (q.numel() + k.numel() + v.numel() + out.numel() + 2 * probs.numel()),
          _p(q), _p(k), _p(v), _p(out), _p(probs), n, sq, skv, h, d, q.stride(0), k.stride(0), v.stride(0), p_drop, seed,
          _stream())
    return out, probs


def attn_bwd(q, k, v, probs, dout, dq, dk, dv, n, sq, skv, h, d, p_drop=0.0, seed=0):
    """dq, dk, dv: views with the row strides of q, k, v (the gradient of a packed projection lands in one buffer)"""
    _attn_views("attn_bwd", q, k, v, n, sq, skv, h, d)
    _attn_views("attn_bwd", dq, dk, dv, n, sq, skv, h, d)
    if (dq.stride(0), dk.stride(0), dv.stride(0)) != (q.stride(0), k.stride(0), v.stride(0)):
        raise _lib.WfaeError("attn_bwd: dq, dk, dv must have the row strides of q, k, v")
    _chk(probs, dout)
    if tuple(probs.shape) != (n, h, sq, skv) or tuple(dout.shape) != (n * sq, h * d):
        raise _lib.WfaeError(f"attn_bwd: probs {tuple(probs.shape)} / dout {tuple(dout.shape)}, expected "
                             f"({n}, {h}, {sq}, {skv}) and ({n * sq}, {h * d})")
    _call("wfae_attn_bwd", 10 * n * h * sq * skv * d, 4 * (2 * (q.numel() + k.numel() + v.numel()) + dout.numel() + 3 * probs.numel()),
          _p(q), _p(k), _p(v), _p(probs), _p(dout), _p(dq), _p(dk), _p(dv), n, sq, skv, h, d, q.stride(0), k.stride(0),
          v.stride(0), p_drop, seed, _stream())


def _gn_dims(what, x, gamma, beta, bias, d=""):
    """(N, C, HW) of x; the per-channel vectors (with d = "d": their gradients) are checked against C"""
    if x.dim() < 3:
        raise _lib.WfaeError(f"{what}: expected (N, C, ...), got {tuple(x.shape)}")
    n, c = x.shape[0], x.shape[1]
    hw = x.numel() // max(n * c, 1)
    for name, t in (("gamma", gamma), ("beta", beta), ("bias", bias)):
        if t is not None and tuple(t.shape) != (c,):
            raise _lib.WfaeError(f"{what}: {d}{name} of shape {tuple(t.shape)} against {c} channels")
    return n, c, hw


def gn_act_fwd(x, gamma, beta, groups, eps=1e-5, act=0, bias=None):
    """-> (y, mean (N, G), rstd (N, G)): y = act(GroupNorm(x + bias[c])), act 0 none / 1 exact GELU"""
    _chk(x, gamma, beta, bias)
    n, c, hw = _gn_dims("gn_act_fwd", x, gamma, beta, bias)
    y = torch.empty_like(x)
    mean = torch.empty((n, groups), dtype=torch.float32, device=x.device)
    rstd = torch.empty((n, groups), dtype=torch.float32, device=x.device)
    _call("wfae_gn_act_fwd", 0, 8 * x.numel(), _p(x), _p(bias), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), n, c, hw,
          int(groups), float(eps), int(act), _stream())
    return y, mean, rstd


def gn_act_bwd(dy, x, gamma, beta, mean, rstd, dgamma, dbeta, groups, act=0, bias=None, dbias=None, accumulate=False):
    """-> dx; dgamma, dbeta (and dbias when a bias was given) are written, or added to with accumulate"""
    _chk(dy, x, gamma, beta, mean, rstd, dgamma, dbeta, bias, dbias)
    n, c, hw = _gn_dims("gn_act_bwd", x, gamma, beta, bias)
    _gn_dims("gn_act_bwd", x, dgamma, dbeta, dbias, "d")
    if dy.shape != x.shape or tuple(mean.shape) != (n, groups) or tuple(rstd.shape) != (n, groups):
        raise _lib.WfaeError(f"gn_act_bwd: dy {tuple(dy.shape)} / statistics {tuple(mean.shape)} against x {tuple(x.shape)}")
    dx = torch.empty_like(x)
    ws = workspace(_lib.load().wfae_gn_act_bwd_workspace_bytes(n, c))
    _call("wfae_gn_act_bwd", 0, 12 * x.numel(), _p(dy), _p(x), _p(bias), _p(gamma), _p(beta), _p(mean), _p(rstd), _p(dx),
          _p(dgamma), _p(dbeta), _p(dbias), n, c, hw, int(groups), int(act), int(accumulate), ws.data_ptr(), ws.numel(),
          _stream())
    return dx


def channel_bias_fwd(x, b):
    """x (N, C, ...) + b (C)"""
    _chk(x, b)
    if x.dim() < 2 or tuple(b.shape) != (x.shape[1],):
        raise _lib.WfaeError(f"channel_bias_fwd: x {tuple(x.shape)} against a bias of shape {tuple(b.shape)}")
    n, c = x.shape[0], x.shape[1]
    y = torch.empty_like(x)
    _call("wfae_channel_bias_fwd", 0, 8 * x.numel(), _p(x), _p(b), _p(y), n, c, x.numel() // (n * c), _stream())
    return y


def head_dropout_bcast_fwd(v, sq, h, p_drop=0.0, seed=0):
    """v (N, E) -> (N * sq, E): attention over one key, the value row under the head-wise dropout mask of its probabilities"""
    _chk(v)
    if v.dim() != 2 or v.shape[1] % h != 0:
        raise _lib.WfaeError(f"head_dropout_bcast_fwd: v {tuple(v.shape)} against {h} heads")
    n, e = v.shape
    out = torch.empty((n * sq, e), dtype=torch.float32, device=v.device)
    _call("wfae_head_dropout_bcast_fwd", 0, 4 * (v.numel() + out.numel()), _p(v), _p(out), n, sq, h, e // h, p_drop, seed,
          _stream())
    return out


def head_dropout_bcast_bwd(dout, n, sq, h, p_drop=0.0, seed=0):
    _chk(dout)
    if dout.dim() != 2 or dout.shape[0] != n * sq or dout.shape[1] % h != 0:
        raise _lib.WfaeError(f"head_dropout_bcast_bwd: dout {tuple(dout.shape)} against N = {n}, Sq = {sq}, {h} heads")
    e = dout.shape[1]
    dv = torch.empty((n, e), dtype=torch.float32, device=dout.device)
    _call("wfae_head_dropout_bcast_bwd", 0, 4 * (dv.numel() + dout.numel()), _p(dout), _p(dv), n, sq, h, e // h, p_drop, seed,
          _stream())
    return dv


# ---- residual autoencoder: the ae_gan models in evaluation mode (include/wfae.h "residual autoencoders of ae_gan";
# csrc/resae.hip).  One unit, y = act(conv(x, w) * scale + shift + res), on two routes; `resae_route` alone decides.
RESAE_KINDS = {"conv": 0, "down": 1, "up": 2, "short": 3, "short_down": 4}
RESAE_ROUTES = {"tile": 0, "small": 1}
RESAE_SMALL_PLANE = 16     # output pixels up to which the small-plane route serves a layer


def resae_out_plane(kind, h, wd):
    """output plane of `kind` on an h x wd input"""
    if kind == 2:
        return 2 * h, 2 * wd
    if kind in (1, 4):
        return (h - 1) // 2 + 1, (wd - 1) // 2 + 1
    return h, wd


def resae_live_taps(kind, h, wd):
    """-> the 3 x 3 nested list of booleans: tap (ky, kx) is live iff some output position reads a real input pixel through
    it; the library's rule (wfae_resae_live_taps, bit ky * 3 + kx), which is the one the kernels use"""
    mask = _lib.load().wfae_resae_live_taps(int(kind), int(h), int(wd))
    if mask < 0:
        raise _lib.WfaeError(f"resae_live_taps: kind {kind!r} on a {h}x{wd} plane")
    return [[bool(mask >> (ky * 3 + kx) & 1) for kx in range(3)] for ky in range(3)]


def resae_route(kind, N, Cin, Cout, H, W):
    """-> "small" | "tile": the small-plane route wherever it serves the layer (an output plane of at most 16 pixels).
    Measured faster there on every such layer of ConvAutoencoderBIG (256 to 2048 channels) at B = 8 and B = 32
    (profiles/resae_bench.jsonl); for other channel counts and batch sizes, ConvAutoencoder's
    1024-channel layers among them, the rule is extrapolated from those rows, not measured."""
    ho, wo = resae_out_plane(kind, H, W)
    return "small" if ho * wo <= RESAE_SMALL_PLANE else "tile"


class ResaePacked:
    """packed weights of one layer for one (route, kind, mode)"""
    __slots__ = ("data", "route", "kind", "mode", "cout", "cin")

    def __init__(self, data, route, kind, mode, cout, cin):
        self.data, self.route, self.kind, self.mode, self.cout, self.cin = data, route, kind, mode, cout, cin


def _resae_kind(what, kind):
    kind = RESAE_KINDS.get(kind, kind)
    if kind not in RESAE_KINDS.values():
        raise _lib.WfaeError(f"{what}: kind {kind!r}, expected one of {sorted(RESAE_KINDS)} (0..4)")
    return kind


def resae_pack(w, kind, route, mode=None):
    """raw weights (Cout, Cin, 3, 3), or (Cout, Cin, 1, 1) for the shortcut kinds, -> ResaePacked for `route`"""
    _chk(w)
    kind = _resae_kind("resae_pack", kind)
    if route not in RESAE_ROUTES:
        raise _lib.WfaeError(f"resae_pack: route {route!r}, expected 'small' or 'tile'")
    mode = aekl_mode() if mode is None else mode
    k = 1 if kind >= 3 else 3
    if w.dim() != 4 or tuple(w.shape[2:]) != (k, k):
        raise _lib.WfaeError(f"resae_pack: weight shape {tuple(w.shape)}, expected (Cout, Cin, {k}, {k}) for kind {kind}")
    cout, cin = w.shape[:2]
    nbytes = _lib.load().wfae_resae_pack_bytes(RESAE_ROUTES[route], kind, mode, cout, cin)
    if nbytes == 0:
        raise _lib.WfaeError(f"resae_pack: unsupported Cout={cout} Cin={cin} mode={mode}")
    data = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    _call("wfae_resae_pack", 0, 4 * w.numel() + nbytes, _p(w), data.data_ptr(), RESAE_ROUTES[route], kind, mode, cout, cin,
          _stream())
    return ResaePacked(data, route, kind, mode, cout, cin)


def resae_fold(gamma, beta, running_mean, running_var, eps=1e-5):
    """BatchNorm's running statistics folded per channel, in fp64 on the host, stored as fp32 on the parameters' device:
    -> (scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale)"""
    g, b, m, v = (t.detach().to("cpu", torch.float64) for t in (gamma, beta, running_mean, running_var))
    scale = g / torch.sqrt(v + eps)
    shift = b - m * scale
    return scale.to(gamma.device, torch.float32), shift.to(gamma.device, torch.float32)


def resae_conv(x, packed, scale=None, shift=None, res=None, res_up=False, act=False, route=None):
    """y = act(conv(x) * scale + shift + res): the one launch of the residual autoencoders.  packed: resae_pack's, for the
    route `resae_route` gives this shape (or the `route=` override of the tests and the bench); res (N, Cout, Ho, Wo), or
    with res_up (N, Cout, Ho / 2, Wo / 2) read through a x2 nearest upsample; act: exact GELU"""
    _chk(x, scale, shift, res)
    if x.dim() != 4 or x.shape[1] != packed.cin:
        raise _lib.WfaeError(f"resae_conv: expected (N, {packed.cin}, H, W), got {tuple(x.shape)}")
    n, cin, h, wd = x.shape
    kind, cout = packed.kind, packed.cout
    want = resae_route(kind, n, cin, cout, h, wd) if route is None else route
    if want != packed.route or packed.data.device != x.device:
        raise _lib.WfaeError(f"resae_conv: weights packed for route {packed.route!r} on {packed.data.device}, the launch is "
                             f"route {want!r} on {x.device}")
    ho, wo = resae_out_plane(kind, h, wd)
    for name, v in (("scale", scale), ("shift", shift)):
        if v is not None and tuple(v.shape) != (cout,):
            raise _lib.WfaeError(f"resae_conv: {name} {tuple(v.shape)}, expected {(cout,)}")
    rshape = (n, cout, ho // 2, wo // 2) if res_up else (n, cout, ho, wo)
    if res is not None and (tuple(res.shape) != rshape or (res_up and (ho % 2 or wo % 2))):
        raise _lib.WfaeError(f"resae_conv: residual {tuple(res.shape)}, expected {rshape}")
    y = torch.empty((n, cout, ho, wo), dtype=torch.float32, device=x.device)
    ws_bytes = _lib.load().wfae_resae_workspace_bytes(kind, n, cin, cout, h, wd) if want == "small" else 0
    ws = workspace(ws_bytes) if ws_bytes else None
    taps = sum(map(sum, resae_live_taps(kind, h, wd)))
    wbytes = 4 * cout * cin * taps if want == "small" else packed.data.numel()
    _call("wfae_resae_conv", 2 * taps * n * ho * wo * cin * cout,
          wbytes + 4 * (x.numel() + y.numel() + (res.numel() if res is not None else 0)), _p(x), packed.data.data_ptr(),
          _p(scale), _p(shift), _p(res), _p(y), RESAE_ROUTES[want], kind, packed.mode, (2 if res_up else 1) if res is not None else 0,
          int(bool(act)), n, cin, cout, h, wd, None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel(), _stream(),
          label=f"wfae_resae_conv {want} k{kind} {cin}->{cout} {ho}x{wo}",
          peak=PEAK_FP32_MFMA if want == "small" else _aekl_peak(packed.mode))
    return y


# ---- residual autoencoder, backward (include/wfae.h "residual autoencoders of ae_gan, backward"; csrc/resae_bwd.hip): the
# data and the weight gradient of the five kinds on two routes, `resae_bwd_route` alone decides; the join of a train-mode
# block forward and backward.
def resae_bwd_route(what, kind, N, Cin, Cout, H, W):
    """-> "small" | "tile" for what = "data" | "weight" of the layer (kind, N, Cin, Cout, H, W: the forward's).  The
    small-plane route wherever it serves the layer: an output plane of at most 16 pixels, the forward's rule (`resae_route`).
    Both gradients follow it; DESIGN.md "Training the residual autoencoders" has the rows it rests on."""
    if what not in ("data", "weight"):
        raise _lib.WfaeError(f"resae_bwd_route: what {what!r}, expected 'data' or 'weight'")
    ho, wo = resae_out_plane(kind, H, W)
    return "small" if ho * wo <= RESAE_SMALL_PLANE else "tile"


class ResaePackedT:
    """the data gradient's operand of one layer: the weight with in and out channels transposed (both routes)"""
    __slots__ = ("data", "kind", "cout", "cin")

    def __init__(self, data, kind, cout, cin):
        self.data, self.kind, self.cout, self.cin = data, kind, cout, cin


def resae_bwd_pack(w, kind):
    """raw weights (Cout, Cin, k, k) -> ResaePackedT"""
    _chk(w)
    kind = _resae_kind("resae_bwd_pack", kind)
    k = 1 if kind >= 3 else 3
    if w.dim() != 4 or tuple(w.shape[2:]) != (k, k):
        raise _lib.WfaeError(f"resae_bwd_pack: weight shape {tuple(w.shape)}, expected (Cout, Cin, {k}, {k}) for kind {kind}")
    cout, cin = w.shape[:2]
    nbytes = _lib.load().wfae_resae_bwd_pack_bytes(kind, cout, cin)
    if nbytes == 0:
        raise _lib.WfaeError(f"resae_bwd_pack: unsupported Cout={cout} Cin={cin}")
    data = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    _call("wfae_resae_bwd_pack", 0, 4 * w.numel() + nbytes, _p(w), data.data_ptr(), kind, cout, cin, _stream())
    return ResaePackedT(data, kind, cout, cin)


def _resae_bwd_shapes(what, kind, dy, cin, cout, x_shape):
    """checks dy (N, Cout, Ho, Wo) against the forward input shape (N, Cin, H, W) -> (n, h, wd, ho, wo)"""
    if len(x_shape) != 4 or x_shape[1] != cin:
        raise _lib.WfaeError(f"{what}: input shape {tuple(x_shape)}, expected (N, {cin}, H, W)")
    n, _, h, wd = x_shape
    ho, wo = resae_out_plane(kind, h, wd)
    if tuple(dy.shape) != (n, cout, ho, wo):
        raise _lib.WfaeError(f"{what}: dy {tuple(dy.shape)}, expected {(n, cout, ho, wo)} for kind {kind} on {tuple(x_shape)}")
    return n, h, wd, ho, wo


def _resae_bwd_route_arg(what, which, route, kind, n, cin, cout, h, wd):
    route = resae_bwd_route(which, kind, n, cin, cout, h, wd) if route is None else route
    if route not in RESAE_ROUTES:
        raise _lib.WfaeError(f"{what}: route {route!r}, expected 'small' or 'tile'")
    return route


def resae_bwd_data(dy, packed_t, x_shape, add=None, route=None):
    """dx = dgrad(dy) + add for the layer whose forward input had `x_shape`; packed_t: resae_bwd_pack's; add: dx's shape"""
    _chk(dy, add)
    kind, cin, cout = packed_t.kind, packed_t.cin, packed_t.cout
    n, h, wd, ho, wo = _resae_bwd_shapes("resae_bwd_data", kind, dy, cin, cout, tuple(x_shape))
    if add is not None and tuple(add.shape) != (n, cin, h, wd):
        raise _lib.WfaeError(f"resae_bwd_data: add {tuple(add.shape)}, expected {(n, cin, h, wd)}")
    if packed_t.data.device != dy.device:
        raise _lib.WfaeError(f"resae_bwd_data: weights packed on {packed_t.data.device}, dy on {dy.device}")
    route = _resae_bwd_route_arg("resae_bwd_data", "data", route, kind, n, cin, cout, h, wd)
    dx = torch.empty((n, cin, h, wd), dtype=torch.float32, device=dy.device)
    ws_bytes = _lib.load().wfae_resae_bwd_data_workspace_bytes(RESAE_ROUTES[route], kind, n, cin, cout, h, wd)
    ws = workspace(ws_bytes) if ws_bytes else None
    taps = sum(map(sum, resae_live_taps(kind, h, wd)))
    _call("wfae_resae_bwd_data", 2 * taps * n * ho * wo * cin * cout,
          4 * (cout * cin * taps + dy.numel() + dx.numel() * (2 if add is not None else 1)), _p(dy), packed_t.data.data_ptr(),
          _p(add), _p(dx), RESAE_ROUTES[route], kind, n, cin, cout, h, wd, None if ws is None else ws.data_ptr(),
          0 if ws is None else ws.numel(), _stream(), label=f"wfae_resae_bwd_data {route} k{kind} {cin}<-{cout} {ho}x{wo}",
          peak=PEAK_FP32_MFMA)
    return dx


def resae_bwd_weight(dy, x, dw, kind, dbias=None, route=None):
    """dw (Cout, Cin, k, k) = wgrad(dy, x), written (exact zeros in dead taps); dbias (Cout) = the sum of dy, optional"""
    _chk(dy, x, dw, dbias)
    kind = _resae_kind("resae_bwd_weight", kind)
    k = 1 if kind >= 3 else 3
    if dw.dim() != 4 or tuple(dw.shape[2:]) != (k, k):
        raise _lib.WfaeError(f"resae_bwd_weight: dw shape {tuple(dw.shape)}, expected (Cout, Cin, {k}, {k}) for kind {kind}")
    cout, cin = dw.shape[:2]
    n, h, wd, ho, wo = _resae_bwd_shapes("resae_bwd_weight", kind, dy, cin, cout, tuple(x.shape))
    if dbias is not None and tuple(dbias.shape) != (cout,):
        raise _lib.WfaeError(f"resae_bwd_weight: dbias {tuple(dbias.shape)}, expected {(cout,)}")
    route = _resae_bwd_route_arg("resae_bwd_weight", "weight", route, kind, n, cin, cout, h, wd)
    ws_bytes = _lib.load().wfae_resae_bwd_weight_workspace_bytes(RESAE_ROUTES[route], kind, n, cin, cout, h, wd)
    ws = workspace(ws_bytes) if ws_bytes else None
    taps = sum(map(sum, resae_live_taps(kind, h, wd)))
    _call("wfae_resae_bwd_weight", 2 * taps * n * ho * wo * cin * cout, 4 * (dw.numel() + dy.numel() + x.numel()), _p(dy), _p(x),
          _p(dw), _p(dbias), RESAE_ROUTES[route], kind, n, cin, cout, h, wd, None if ws is None else ws.data_ptr(),
          0 if ws is None else ws.numel(), _stream(), label=f"wfae_resae_bwd_weight {route} k{kind} {cin}->{cout} {ho}x{wo}",
          peak=PEAK_FP32_MFMA)
    return dw


def _resae_join_args(what, c2, s2, h2, r, ss, hs, res_up):
    _chk(c2, s2, h2, r, ss, hs)
    if c2.dim() != 4:
        raise _lib.WfaeError(f"{what}: expected c2 (N, C, H, W), got {tuple(c2.shape)}")
    n, c, h, wd = c2.shape
    rshape = (n, c, h // 2, wd // 2) if res_up else (n, c, h, wd)
    if tuple(r.shape) != rshape or (res_up and (h % 2 or wd % 2)):
        raise _lib.WfaeError(f"{what}: residual {tuple(r.shape)}, expected {rshape}")
    if (ss is None) != (hs is None):
        raise _lib.WfaeError(f"{what}: ss and hs go together")
    for name, v in (("s2", s2), ("h2", h2), ("ss", ss), ("hs", hs)):
        if v is not None and tuple(v.shape) != (c,):
            raise _lib.WfaeError(f"{what}: {name} {tuple(v.shape)}, expected {(c,)}")
    return n, c, h, wd


def resae_join_fwd(c2, s2, h2, r, ss=None, hs=None, res_up=False):
    """y = gelu(c2 s2[c] + h2[c] + r'), r' = r ss[c] + hs[c] or r itself; res_up: r at half resolution"""
    n, c, h, wd = _resae_join_args("resae_join_fwd", c2, s2, h2, r, ss, hs, res_up)
    y = torch.empty_like(c2)
    _call("wfae_resae_join_fwd", 0, 4 * (2 * c2.numel() + r.numel()), _p(c2), _p(s2), _p(h2), _p(r), _p(ss), _p(hs), _p(y),
          2 if res_up else 1, n, c, h, wd, _stream())
    return y


def resae_join_bwd(dy, c2, s2, h2, r, ss=None, hs=None, res_up=False):
    """-> (dpre = dy gelu'(pre), dres): dres is dpre itself at the same resolution, its 2 x 2 block sums with res_up"""
    n, c, h, wd = _resae_join_args("resae_join_bwd", c2, s2, h2, r, ss, hs, res_up)
    _chk(dy)
    if dy.shape != c2.shape:
        raise _lib.WfaeError(f"resae_join_bwd: dy {tuple(dy.shape)}, expected {tuple(c2.shape)}")
    dpre = torch.empty_like(c2)
    dres = torch.empty_like(r) if res_up else None
    _call("wfae_resae_join_bwd", 0, 4 * (3 * c2.numel() + 2 * r.numel()), _p(dy), _p(c2), _p(s2), _p(h2), _p(r), _p(ss), _p(hs),
          _p(dpre), _p(dres), 2 if res_up else 1, n, c, h, wd, _stream())
    return dpre, (dres if res_up else dpre)


def resae_bn_stats_train(x, gamma, beta, running_mean, running_var, eps=1e-5, momentum=0.1, replicas=1):
    """bn_stats_train for a block of the residual autoencoders.  replicas = 4: x is what the reference's BatchNorm sees
    through the x2 upsample (the shortcut of an UpsampleBlock, kept at the source resolution): the batch statistics are
    x's, the unbiased factor of the running variance counts every value four times.  A single value per channel raises
    ValueError, as nn.BatchNorm2d does in training mode."""
    nb, c, h, wd = x.shape
    if nb * h * wd * replicas <= 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
    if replicas == 1:
        return bn_stats_train(x, gamma, beta, running_mean, running_var, eps, momentum)
    _chk(running_mean, running_var)
    st = bn_stats_train(x, gamma, beta, None, None, eps, momentum)
    _call("wfae_resae_bn_running", 0, 16 * c, _p(st.mean), _p(st.invstd), _p(running_mean), _p(running_var), c, eps, momentum,
          nb * h * wd * replicas, _stream())
    return st


# ---- prediction / target / difference panels (include/wfae.h "panels in the SEVIR VIL colours"; csrc/panels.hip)
def panel_bytes(t, h, w, gap=0):
    """bytes of one figure of `t` frames of h x w with `gap` white pixels between panels: (3h + 2 gap) scanlines of a
    filter byte and 3 (t w + (t - 1) gap) colour bytes; 0 where panel_render refuses the arguments"""
    return int(_lib.load().wfae_panel_bytes(int(t), int(h), int(w), int(gap)))


def panel_render(pred, target, lut_vil, lut_diff, nb, gap=0):
    """pred, target fp32 (B, T, H, W); lut_vil, lut_diff uint8 (256, 3) on the same device -> uint8 (nb, Hfig, 1 + 3 Wfig):
    the first nb samples as target / prediction / difference rows, each figure the uncompressed scanlines of a PNG"""
    _chk(pred, target)
    if pred.dim() != 4 or pred.shape != target.shape:
        raise _lib.WfaeError(f"panel_render: pred {tuple(pred.shape)} and target {tuple(target.shape)} must be one "
                             "(B, T, H, W) shape")
    for name, lut in (("lut_vil", lut_vil), ("lut_diff", lut_diff)):
        if (lut.dtype != torch.uint8 or tuple(lut.shape) != (256, 3) or not lut.is_contiguous()
                or lut.device != pred.device):
            raise _lib.WfaeError(f"panel_render: {name} must be a contiguous uint8 (256, 3) tensor on {pred.device}")
    b, t, h, w = pred.shape
    nb, gap = int(nb), int(gap)
    fig = panel_bytes(t, h, w, gap) if min(b, t, h, w) > 0 else 0
    if not 1 <= nb <= b or gap < 0 or fig == 0:
        raise _lib.WfaeError(f"panel_render: {nb} samples of a batch of shape {tuple(pred.shape)} with gap {gap}")
    hfig, wfig = 3 * h + 2 * gap, t * w + (t - 1) * gap
    out = torch.empty((nb, hfig, 1 + 3 * wfig), dtype=torch.uint8, device=pred.device)
    _call("wfae_panel_render", 0, nb * (fig + 8 * t * h * w), _p(pred), _p(target), lut_vil.data_ptr(), lut_diff.data_ptr(),
          out.data_ptr(), b, nb, t, h, w, gap, _stream())
    return out


def range_count(x):
    """the number of elements of the fp32 tensor x in [0, 1] (NaN, +-inf outside) -> int64 device scalar"""
    _chk(x)
    if x.numel() < 1:
        raise _lib.WfaeError("range_count: empty tensor")
    out = torch.empty((), dtype=torch.int64, device=x.device)
    ws = workspace()
    _call("wfae_range_count", 0, 4 * x.numel(), _p(x), x.numel(), out.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    return out
