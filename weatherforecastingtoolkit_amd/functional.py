"""autograd glue: torch.autograd.Function wrappers whose forward AND backward are
sequences of libwfae.so kernel launches (ops.py).  Granularity follows the
reference's building blocks so that the fan-out of the residual stream stays
inside one Function (no ATen gradient-accumulation kernels on the hot path):

  DownUnitFn     Conv2d(4,2,1) -> BN -> GELU            EncBlock.down  (ae_64x8x8_lin.py:30-33)
  UpUnitFn       ConvTranspose2d(4,2,1) -> BN -> GELU   DecBlock.up    (:41-44)
  BottleneckFn   x + f(x)                               Bottleneck     (:7-22)
  Conv1x1Fn      1x1 conv (+bias) (+broadcast pos_emb)  enc[4], dec[0] (:69,79,91)
  LinearFn       to_latent / from_latent                (:74-75)
  DConvFn        3x3 'same' conv, any groups            dec[5]         (:84)
  SigmoidFn, L1LossFn, SsimFn                           (:86; experiments/ae_v2/train.py:55,62)

Parameter gradients are written by the kernels straight into the tensor that
`grad_buffer(p)` returns — a view of a flat gradient arena when an optimiser /
data-parallel wrapper registered one (so AdamW and the RCCL all-reduce see one
contiguous buffer), otherwise a fresh tensor — and handed back to autograd,
which adopts it as `p.grad` without a copy.
"""
from __future__ import annotations

import os

import torch
from torch.autograd import Function

from . import ops

BN_EPS = 1e-5


# ---------------------------------------------------------------------------------------------
# Weight-gradient kernels do not feed the backward chain (dgrad -> BN bwd -> dgrad ...), so they
# can run on a second HIP stream: the MFMA-bound wgrad GEMMs then overlap the HBM-bound
# BatchNorm / element-wise backward kernels of the critical path.  Opt-in (bench / train script):
# whoever reads .grad afterwards must call join_side_stream() first (FusedAdamW.step,
# DataParallelTrainer.reduce_gradients and helpers.grad_norm do).
# ---------------------------------------------------------------------------------------------
_overlap = False
_side = {}


# BatchNorm statistics of 1x1-convolution outputs reduced in the GEMM epilogue instead of by a pass over the tensor.
# Round 1 built this with fp32 partial sums (four DPP adds per 64-column wave row) and left it off: the fp32 partials
# are as accurate as the separate pass but not ROUNDED like it, and a 1-ulp difference of a channel mean was enough to
# push a near-tie pixel of the L1 loss across its kink.  The partials are now reduced in fp64 from
# fp32 sums of four — the arithmetic of the separate pass (chan_reduce_kernel) — so the statistics are reproduced to
# fp64 rounding (2e-7 asserted in test_conv1x1_fwd_stats_epilogue).  WFAE_STAT_FUSION=0: separate passes.
STAT_FUSION = os.environ.get("WFAE_STAT_FUSION", "1") == "1"


# BatchNorm-apply + GELU of a Bottleneck's FIRST BatchNorm (the C-channel residual stream: 70 % of the BN/GELU bytes)
# inside the operand loaders of the two GEMMs that consume it (forward C -> C/4 convolution, its weight gradient):
# a1 = gelu(bn1(x)) is never written, saved or re-read (ops.conv1x1_fwd_bnact).  Bit-identical results.
# Measured (B = 32, 384x384, fp32, profiles/r02_v2_*): forward GEMMs + apply passes 21.6 -> 14.8 ms per step, weight
# gradients 12.7 -> 15.0 ms (they evaluate the GELU a second time), step 256.0 -> 249.7 ms, peak memory 106.9 -> 86.4 GiB.
# WFAE_FUSE_A1=0 restores the materialised form, WFAE_FUSE_A1_MAXC limits the fused form to that many input channels (A/B:
# 256 -> 250.1 ms, 512 -> 249.6 ms, all -> 249.7 ms).
FUSE_A1 = os.environ.get("WFAE_FUSE_A1", "1") == "1"
FUSE_A1_MAXC = 1 << 30
# The same for the THIRD BatchNorm of a Bottleneck (C/4 channels -> the C/4 -> C convolution and its weight gradient; the
# roles of that weight gradient are swapped when C/4 < 128, so the prologue sits on its A operand there).  The forward
# GEMM re-loads (and re-activates) every element once per M tile, 1 - 8 times: measured for the whole step, fusing it
# at every width costs 3 ms (247.4 -> 250.5 ms), at C <= 256 0.5 ms, at C <= 128 nothing — so it is limited to
# WFAE_FUSE_A3_MAXC = 128 output channels (one M tile; -1.1 GiB; 256 where csrc/c1r.hip serves the product, below).  WFAE_FUSE_A3=0: off.
FUSE_A3 = os.environ.get("WFAE_FUSE_A3", "1") == "1"
FUSE_A3_MAXC = int(os.environ.get("WFAE_FUSE_A3_MAXC", "128"))
# fp32 tensors on csrc/c1r.hip (round 4): its prologue form of the C/4 -> C product at C = 256 costs 0.519 against 0.507 ms + the
# 0.123 ms apply pass, the weight gradient's prologue sits on the 64-channel operand: the step is unchanged (185.1 / 185.3 against
# 184.9 / 185.4 ms, same box) and a3 is not kept: - 2.25 GiB.  Above that the M-sliced kernels activate the operand once per slice.
# bf16 storage on csrc/c1rb.hip: 93.25 / 92.9 -> 92.68 / 92.71 ms, - 1.1 GiB.
FUSE_A3_MAXC_C1R = max(FUSE_A3_MAXC, 256)


# BatchNorm sums produced by the kernel that WRITES the tensor when that kernel is a streaming one (the Winograd output
# transform in front of a unit's BatchNorm; the unit's BatchNorm+GELU pass in front of the first Bottleneck): fp64
# accumulation like the separate statistics pass, so its results are reproduced to fp64 rounding.  WFAE_PRODUCER_STATS=0: off.
PRODUCER_STATS = os.environ.get("WFAE_PRODUCER_STATS", "1") == "1"


def set_wgrad_overlap(flag: bool):
    global _overlap
    _overlap = bool(flag)


def _side_stream():
    dev = torch.cuda.current_device()
    s = _side.get(dev)
    if s is None:
        s = _side[dev] = torch.cuda.Stream(device=dev)
    return s


# Tensors read by side-stream kernels are kept alive (Python references) until the main stream has
# waited for the side stream; only then may the caching allocator hand their memory to later
# main-stream kernels.  (tensor.record_stream() would also be correct but makes the allocator poll
# per-block events and, with the host running several steps ahead, fall back to fresh hipMallocs.)
_keep = []
_keep_bytes = [0]
_KEEP_LIMIT = 24 << 30


def join_side_stream():
    if _side:
        dev = torch.cuda.current_device()
        if dev in _side:
            torch.cuda.current_stream().wait_stream(_side[dev])
    _keep.clear()
    _keep_bytes[0] = 0


def _wgrad(fn, *tensors):
    """run fn() (a weight-gradient launch reading `tensors`) on the side stream when overlap is on"""
    if not _overlap:
        return fn()
    if _force_main[0]:
        # the gradient buffer handed out last will be summed with an earlier contribution by autograd on the
        # main stream: wait for the side stream (the earlier contribution may still be in flight there) and
        # stay on the main stream
        _force_main[0] = False
        join_side_stream()
        return fn()
    side = _side_stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    _keep.extend(tensors)
    _keep_bytes[0] += sum(t.numel() * t.element_size() for t in tensors)
    if _keep_bytes[0] > _KEEP_LIMIT:
        join_side_stream()


def _on_main(fn):
    """run fn() (a launch that writes a gradient buffer) on the main stream — behind the side stream when grad_buffer handed
    out a buffer autograd will add to an earlier contribution (see _wgrad)"""
    if _force_main[0]:
        _force_main[0] = False
        if _overlap:
            join_side_stream()
    return fn()


_arena_grads = [True]


class detached_grads:
    """Context in which parameter gradients are written to fresh buffers instead of the optimiser's
    gradient arena — for torch.autograd.grad(...) probes whose results must survive later backward
    passes (the adaptive GAN weight, experiments/ae_v2_2/train.py:46-52)."""

    def __enter__(self):
        self.prev = _arena_grads[0]
        _arena_grads[0] = False

    def __exit__(self, *exc):
        _arena_grads[0] = self.prev


_force_main = [False]


def grad_buffer(p):
    """Where a backward kernel writes the gradient of parameter p: p's slot in the optimiser's gradient
    arena when this is the only contribution autograd will see for p in this pass.  When the gradient is
    going to be ADDED to another one — p already has a .grad (gradient accumulation), or p is used more
    than once in the graph (the discriminator on real and fake batches, ae_v2_2/train.py:88-89; the engine
    sums both before AccumulateGrad runs) — it gets a fresh buffer, and the launch that fills it is kept
    on the main stream behind the side stream (`_wgrad`), because autograd performs that addition on the
    main stream."""
    task = torch._C._current_graph_task_id()
    again = task >= 0 and getattr(p, "_wfae_lent_task", None) == task
    p._wfae_lent_task = task
    if p.grad is not None or again:
        _force_main[0] = True
        return torch.empty_like(p)
    v = getattr(p, "_wfae_grad_view", None)
    if v is not None and _arena_grads[0]:
        # a fresh alias: autograd adopts the tensor as p.grad without a copy only
        # when nobody else references the same TensorImpl
        return v.view(v.shape)
    return torch.empty_like(p)


def _bn_stats(x, bn, training):
    """training: batch statistics + running-stat update; eval: fold running stats."""
    if training:
        st = ops.bn_stats_train(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, bn.momentum)
        bn._nbt_pending += 1
        return st
    return ops.bn_fold_eval(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)


def _bn_stats_rows(sr, x, bn, training):
    """_bn_stats of x when a producer kernel may already have reduced its per-channel sums (ops.StatRows: fp32 rows of
    a GEMM epilogue; ops.StatParts: fp64 partials of a streaming producer)"""
    if training and isinstance(sr, ops.StatParts):
        st = ops.bn_stats_from_parts(sr, tuple(x.shape), bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps,
                                     bn.momentum)
        bn._nbt_pending += 1
        return st
    if training and sr is not None:
        st = ops.bn_stats_from_rows(sr, tuple(x.shape), bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps,
                                    bn.momentum)
        bn._nbt_pending += 1
        return st
    return _bn_stats(x, bn, training)


def _use_batch_stats(bn):
    return bn.training or bn.running_mean is None


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


# ----------------------------------------------------------- 4x4 s2 units --
def _down_fwd(x, w, unit=False):
    if w.shape[1] < 16:
        # the one-channel first layer of the MODEL's stack (unit=True: DownUnitFn) reads the fp32 frame and writes the stack's
        # activation storage type; the generic Conv2d(.., 4, 2, 1) layer (Conv4x4DownFn) keeps the dtype of its input
        out = ops.activation_dtype() if (unit and x.dtype == torch.float32 and w.shape[1] == 1) else torch.float32
        return ops.dconv_fwd(x, w, None, 4, 2, 1, 1, out_dtype=out)
    return ops.conv4x4s2_down(x, w)


def _down_wgrad(dlo, hi, dw):
    if hi.shape[1] < 16:
        return ops.dconv_bwd_weight(dlo, hi, dw, 4, 2, 1, 1)
    return ops.conv4x4s2_wgrad(dlo, hi, dw)


# Winograd form of the 4x4 stride-2 GEMMs (ops.wino_*): every tensor is transformed ONCE per step.
# The forward keeps the transformed input (V = In(hi) for a Conv2d, Mt = Out^T(lo) for a ConvTranspose2d) and the
# transformed weights U; the backward transforms the incoming gradient once and feeds it to both the data-
# gradient GEMM and the weight-gradient GEMM.
def _down_plan(x, w):
    """plan for Conv2d(Chi -> Clo, 4, s2, p1) on x (N,Chi,2Hlo,2Wlo); None: direct kernels"""
    if w.shape[1] < 16 or (x.shape[2] & 1) or (x.shape[3] & 1):
        return None
    return ops.wino_plan(x.shape[0], w.shape[1], w.shape[0], x.shape[2] // 2, x.shape[3] // 2)


def _down_forward(x, w, stats=False):
    """-> (t, pl, U, V[, StatParts of t]): 4x4 s2 convolution of x; U, V are None on the direct path"""
    pl = _down_plan(x, w)
    if pl is None:
        return (_down_fwd(x, w, unit=True), None, None, None) + ((None,) if stats else ())
    U, V = ops.wino_weights(w, pl), ops.wino_in(x, pl)
    if stats:
        t, sp = ops.wino_down(U, V, pl, stats=True, out_dtype=x.dtype)
        return t, pl, U, V, sp
    return ops.wino_down(U, V, pl, out_dtype=x.dtype), pl, U, V


def _down_backward(dt, x, w, pl, U, V, need_dx, need_dw):
    """gradients of the 4x4 s2 convolution: (dx or None, dw or None); the weight gradient goes to the side stream"""
    dw = dx = None
    if pl is None:
        if need_dw:
            dw = grad_buffer(w)
            _wgrad(lambda: _down_wgrad(dt, x, dw), dt, x)
        if need_dx:
            dx = ops.conv4x4s2_up(dt, w)
        return dx, dw
    Mt = ops.wino_out_t(dt, pl)
    if need_dw:
        dw = grad_buffer(w)
        _wgrad(lambda: ops.wino_wgrad(Mt, V, dw, pl), Mt, V)
    if need_dx:
        dx = ops.wino_up(U, Mt, pl, out_dtype=x.dtype)
    return dx, dw


def _opt(t):
    """placeholder for an absent cached tensor in save_for_backward"""
    return t if t is not None else torch.empty(0)


class DownUnitFn(Function):
    @staticmethod
    def forward(ctx, x, w, gamma, beta, bn):
        x = _c(x)
        training = _use_batch_stats(bn)
        prod = training and PRODUCER_STATS
        t, pl, U, V, sp = _down_forward(x, w, stats=True) if prod else _down_forward(x, w) + (None,)
        st = _bn_stats_rows(sp, t, bn, training)
        if prod:    # the sums of `a` ride along for the BatchNorm of the first Bottleneck (EncBlock.forward hands them on)
            a, bn._out_stats = ops.bn_act_fwd_stats(t, st, 1)
        else:
            a, bn._out_stats = ops.bn_act_fwd(t, st, 1), None
        ctx.save_for_backward(x, w, gamma, t, st.mean, st.invstd, st.scale, st.shift, _opt(U), _opt(V))
        ctx.training, ctx.beta, ctx.pl = training, beta, pl
        return a

    @staticmethod
    def backward(ctx, da):
        x, w, gamma, t, mean, invstd, scale, shift, U, V = ctx.saved_tensors
        st = _mk_stats(mean, invstd, scale, shift)
        dg, db = grad_buffer(gamma), grad_buffer(ctx.beta)
        dt = ops.bn_act_bwd(_c(da), t, gamma, st, dg, db, None, 1, ctx.training)
        dx, dw = _down_backward(dt, x, w, ctx.pl, U, V, ctx.needs_input_grad[0], True)
        return dx, dw, dg, db, None


class UpUnitFn(Function):
    @staticmethod
    def forward(ctx, x, w, gamma, beta, bn):
        x = _c(x)
        training = _use_batch_stats(bn)
        pl = ops.wino_plan(x.shape[0], w.shape[1], w.shape[0], x.shape[2], x.shape[3])
        U = Mt = None
        sp = None
        act_dt = ops.activation_dtype() if x.dtype == torch.float32 else x.dtype   # dec[1] reads the fp32 latent projection
        if pl is not None:
            U, Mt = ops.wino_weights(w, pl), ops.wino_out_t(x, pl)
            if training and PRODUCER_STATS:
                t, sp = ops.wino_up(U, Mt, pl, stats=True, out_dtype=act_dt)
            else:
                t = ops.wino_up(U, Mt, pl, out_dtype=act_dt)
        else:
            t = ops.to_dtype(ops.conv4x4s2_up(x, w), act_dt)
        st = _bn_stats_rows(sp, t, bn, training)
        if training and PRODUCER_STATS:
            a, bn._out_stats = ops.bn_act_fwd_stats(t, st, 1)
        else:
            a, bn._out_stats = ops.bn_act_fwd(t, st, 1), None
        ctx.save_for_backward(x, w, gamma, t, st.mean, st.invstd, st.scale, st.shift, _opt(U), _opt(Mt))
        ctx.training, ctx.beta, ctx.pl = training, beta, pl
        return a

    @staticmethod
    def backward(ctx, da):
        x, w, gamma, t, mean, invstd, scale, shift, U, Mt = ctx.saved_tensors
        st = _mk_stats(mean, invstd, scale, shift)
        dg, db = grad_buffer(gamma), grad_buffer(ctx.beta)
        dt = ops.bn_act_bwd(_c(da), t, gamma, st, dg, db, None, 1, ctx.training)
        dw = grad_buffer(w)
        pl = ctx.pl
        if pl is not None:
            V = ops.wino_in(dt, pl)                                  # the hi-side tensor of this layer is dt
            _wgrad(lambda: ops.wino_wgrad(Mt, V, dw, pl), Mt, V)     # lo = x (Mt kept from forward), hi = dt
            dx = ops.wino_down(U, V, pl, out_dtype=x.dtype) if ctx.needs_input_grad[0] else None
        else:
            _wgrad(lambda: ops.conv4x4s2_wgrad(x, dt, dw), x, dt)    # lo = x, hi = dt
            dx = ops.to_dtype(ops.conv4x4s2_down(dt, w), x.dtype) if ctx.needs_input_grad[0] else None
        return dx, dw, dg, db, None


# ------------------------------------------------- PatchGAN discriminator --
# (pipeline/models/autoencoderkl/losses/model.py:100-150).  Parameters that do not require grad (the
# discriminator during the generator step, Lightning's toggle_optimizer in ae_v2_2/train.py:133) get no
# weight-gradient launches at all.
def _maybe_buffer(p, needed):
    return grad_buffer(p) if needed else torch.empty_like(p)


def _conv4_fwd(x, w, bias, stride):
    if stride == 1:
        if bias is None and ops.conv4x4s1_supported(w.shape[1]):
            return ops.conv4x4s1_fwd(x, w, 1, False)
        return ops.dconv_fwd(x, w, bias, 4, 1, 1, 1)
    if bias is not None or w.shape[1] < 16:
        return ops.dconv_fwd(x, w, bias, 4, 2, 1, 1)
    return ops.conv4x4s2_down(x, w)


def _conv4_wgrad(dy, x, dw, stride):
    if stride == 1:
        if ops.conv4x4s1_supported(x.shape[1]):
            return ops.conv4x4s1_bwd_weight(dy, x, dw, 1)
        return ops.dconv_bwd_weight(dy, x, dw, 4, 1, 1, 1)
    return _down_wgrad(dy, x, dw)


def _conv4_dgrad(dy, w, stride):
    if stride == 1:
        if ops.conv4x4s1_supported(w.shape[0]):
            return ops.conv4x4s1_fwd(dy, w, 1, True)
        return ops.dconv_bwd_data(dy, w, w.shape[1], 4, 1, 1)
    return ops.conv4x4s2_up(dy, w)


class DiscUnitFn(Function):
    """Conv2d(4x4, stride s, pad 1, bias=False) -> BatchNorm2d -> LeakyReLU(0.2)  (model.py:129-141)"""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, bn, stride):
        x = _c(x)
        training = _use_batch_stats(bn)
        pl = U = V = None
        if stride == 2:
            t, pl, U, V = _down_forward(x, w)
        else:
            t = _conv4_fwd(x, w, None, stride)
        st = _bn_stats(t, bn, training)
        a = ops.bn_act_fwd(t, st, 2)
        ctx.save_for_backward(x, w, gamma, t, st.mean, st.invstd, st.scale, st.shift, _opt(U), _opt(V))
        ctx.training, ctx.beta, ctx.stride, ctx.pl = training, beta, stride, pl
        return a

    @staticmethod
    def backward(ctx, da):
        x, w, gamma, t, mean, invstd, scale, shift, U, V = ctx.saved_tensors
        st = _mk_stats(mean, invstd, scale, shift)
        need_w, need_g = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        dg, db = _maybe_buffer(gamma, need_g), _maybe_buffer(ctx.beta, need_g)
        dt = ops.bn_act_bwd(_c(da), t, gamma, st, dg, db, None, 2, ctx.training)
        if ctx.stride == 2:
            dx, dw = _down_backward(dt, x, w, ctx.pl, U, V, ctx.needs_input_grad[0], need_w)
        else:
            dw = None
            if need_w:
                dw = grad_buffer(w)
                _wgrad(lambda: _conv4_wgrad(dt, x, dw, 1), dt, x)
            dx = _conv4_dgrad(dt, w, 1) if ctx.needs_input_grad[0] else None
        return dx, dw, dg if need_g else None, db if need_g else None, None, None


class Conv4LeakyFn(Function):
    """Conv2d(4x4, stride 2, pad 1, bias) -> LeakyReLU(0.2)  (model.py:125)"""

    @staticmethod
    def forward(ctx, x, w, bias):
        x = _c(x)
        t = _conv4_fwd(x, w, bias, 2)
        ctx.save_for_backward(x, w, t)
        ctx.bias = bias
        return ops.leaky_relu_fwd(t)

    @staticmethod
    def backward(ctx, dy):
        x, w, t = ctx.saved_tensors
        dt = ops.leaky_relu_bwd(_c(dy), t)
        dw = dbias = None
        if ctx.needs_input_grad[1]:
            dw = grad_buffer(w)
            _conv4_wgrad(dt, x, dw, 2)
        if ctx.bias is not None and ctx.needs_input_grad[2]:
            nb, cout, h, wd = dt.shape
            dbias = grad_buffer(ctx.bias)
            ops.reduce_sum(dt, nb, cout, h * wd, dbias)
        dx = ops.conv4x4s2_up(dt, w) if ctx.needs_input_grad[0] else None
        return dx, dw, dbias


class Conv4Fn(Function):
    """Conv2d(4x4, stride 1|2, pad 1, optional bias) as a standalone layer"""

    @staticmethod
    def forward(ctx, x, w, bias, stride):
        x = _c(x)
        ctx.save_for_backward(x, w)
        ctx.bias, ctx.stride = bias, stride
        return _conv4_fwd(x, w, bias, stride)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = _c(dy)
        dw = dbias = None
        if ctx.needs_input_grad[1]:
            dw = grad_buffer(w)
            _conv4_wgrad(dy, x, dw, ctx.stride)
        if ctx.bias is not None and ctx.needs_input_grad[2]:
            nb, cout, h, wd = dy.shape
            dbias = grad_buffer(ctx.bias)
            ops.reduce_sum(dy, nb, cout, h * wd, dbias)
        dx = _conv4_dgrad(dy, w, ctx.stride) if ctx.needs_input_grad[0] else None
        return dx, dw, dbias, None


class Pad2dFn(Function):
    """zero padding of the spatial dims (the `padding=1` of the reference's final 1x1 conv, model.py:145)"""

    @staticmethod
    def forward(ctx, x, pad):
        ctx.pad = pad
        return ops.pad2d(_c(x), pad)

    @staticmethod
    def backward(ctx, dy):
        return ops.crop2d(_c(dy), ctx.pad), None


class LeakyReluFn(Function):
    @staticmethod
    def forward(ctx, x):
        x = _c(x)
        ctx.save_for_backward(x)
        return ops.leaky_relu_fwd(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return ops.leaky_relu_bwd(_c(dy), x)


class MeanFn(Function):
    """weight * mean(x)  or  weight * mean(relu(1 + sign * x))  (hinge terms, contperceptual.py:19-23)"""

    @staticmethod
    def forward(ctx, x, hinge, sign, weight):
        x = _c(x)
        ctx.save_for_backward(x)
        ctx.cfg = (hinge, sign, weight)
        return ops.mean_fwd(x, hinge, sign, weight)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        hinge, sign, weight = ctx.cfg
        return ops.mean_bwd(x, _c(g), hinge, sign, weight), None, None, None


class ScaleByFn(Function):
    """y = x * s with s a detached device scalar (the adaptive weight, ae_v2/train.py:46-52,84)"""

    @staticmethod
    def forward(ctx, x, s):
        ctx.save_for_backward(s)
        return ops.scale(_c(x), 1.0, s)

    @staticmethod
    def backward(ctx, g):
        (s,) = ctx.saved_tensors
        return ops.scale(_c(g), 1.0, s), None


def hinge_d_loss(logits_real, logits_fake):
    """0.5 * (mean(relu(1 - real)) + mean(relu(1 + fake)))  (contperceptual.py:19-23)"""
    return AddFn.apply(MeanFn.apply(logits_real, True, -1.0, 0.5), MeanFn.apply(logits_fake, True, 1.0, 0.5))


def neg_mean(x):
    """generator term -mean(D(x_hat))  (ae_v2/train.py:78)"""
    return MeanFn.apply(x, False, 1.0, -1.0)


# grouped 3x3 conv of the Bottleneck: register-blocked kernels when channels/group is 4/8/16/32
def _g3_fwd(x, w, groups):
    if ops.gconv3x3_supported(x.shape[1], groups) and w.shape[0] == x.shape[1]:
        return ops.gconv3x3_fwd(x, w, groups, False)
    return ops.dconv_fwd(x, w, None, 3, 1, 1, groups)


def _g3_dgrad(dy, w, cin, groups):
    if ops.gconv3x3_supported(cin, groups) and w.shape[0] == cin:
        return ops.gconv3x3_fwd(dy, w, groups, True)
    return ops.dconv_bwd_data(dy, w, cin, 3, 1, groups)


def _g3_wgrad(dy, x, dw, groups):
    c = x.shape[1]
    # measured (tools/kbench.py): pixel-parallel VALU kernel wins at 4 and 8 channels/group, the per-group
    # MFMA implicit GEMM at 16 and 32 (the library picks between the two)
    if c % groups == 0 and c // groups in (4, 8, 16, 32) and dw.shape[0] == c and groups > 1:
        return ops.gconv3x3_bwd_weight(dy, x, dw, groups)
    return ops.dconv_bwd_weight(dy, x, dw, 3, 1, 1, groups)


# -------------------------------------------------------------- Bottleneck --
def _mk_stats(mean, invstd, scale, shift):
    st = ops.BnStats.__new__(ops.BnStats)
    st.mean, st.invstd, st.scale, st.shift = mean, invstd, scale, shift
    return st


def _storage(t):
    return "bf16" if t.dtype == ops.BF16 else "f32"


def _c1(w, plane, transposed, x, st=None, res=None, stats=False, fam=None):
    """a Bottleneck 1x1 product y = A f(x) (+ res), A = w or, transposed, w^T (the data gradient), on the kernel family
    ops.conv1x1_route names for it (`fam`: the caller has asked already) -> (y, StatRows | None).  `plane`: the bf16 plane of
    ops.c1b_weights that is A, which csrc/c1b.hip takes (a caller without one gets gemm.hip)"""
    if fam is None:
        fam = ops.conv1x1_route("dgrad" if transposed else "fwd", w.shape[1] if transposed else w.shape[0], x.shape[1],
                                x.shape[2] * x.shape[3], _storage(x), st is not None, False, "none" if res is None else "ordinary")
    if fam == "c1b" and (plane is None or plane.numel() == 0):
        fam = "gemm"
    label = None if fam in ("c1r", "gemm") else "wfae_c1b_dgrad" if transposed else "wfae_c1b_fwd"
    return ops._c1_launch(fam, plane if fam == "c1b" else w, transposed, x, st, None, res, False, stats, label)


_b16 = _c1      # (the name tests/ reach it by: it served the bf16-stored tensors only)


def _dgrad_bn(dt, w, Wt, x, gamma, st, dgamma, dbeta, res, training, rows=None):
    """dx of  conv1x1(gelu(bn(x)), w)  given dt = dL/d(conv output): the data gradient dA = W^T dT followed by the
    BatchNorm + GELU backward at x (+ res, the residual-branch gradient); Wt: the bf16 plane of w^T for csrc/c1b.hip, or empty;
    rows: the StatRows of sum dU / sum dU xhat when ops.conv1x1_bwd_ws has taken them already (the 'bndx' route)"""
    if rows is not None:
        # the sums came with the weight gradient: straight to the finish and the second pass.  from_rows writes the coefficients
        # at the head of the workspace whose slabs the fused launch's slab_reduce has read — same stream, in this order
        ops.bn_act_bwd_from_rows(rows, x.shape[1], dgamma, dbeta)
        return ops.c1r_bndx(w, dt, x, gamma, st, res, training)
    how = ops.conv1x1_dgrad_bn_route(w.shape[1], dt.shape[1], dt.shape[2] * dt.shape[3], _storage(dt))
    if how is not None:
        # the C <= 256 widening data gradients on csrc/c1r.hip: sum dU / sum dU xhat of the BatchNorm in front ride in the epilogue
        # (x travels through the kernel's residual ring), the reduce pass over (dA, x) disappears — and with 'bndx' so does dA
        # itself: the second pass runs in the epilogue of the same product computed again
        da, sr = ops.c1r_bnred(w, dt, x, st, store=how == "bnred")
        ops.bn_act_bwd_from_rows(sr, x.shape[1], dgamma, dbeta)
        if how == "bndx":
            return ops.c1r_bndx(w, dt, x, gamma, st, res, training)
        return ops.bn_act_bwd_dx(da, x, gamma, st, res, 1, training)
    return ops.bn_act_bwd(_c1(w, Wt, True, dt)[0], x, gamma, st, dgamma, dbeta, res, 1, training)


class BottleneckFn(Function):
    @staticmethod
    def forward(ctx, x, g1, b1, w1, g2, b2, wg, g3, b3, w3, mod, x_stats=None):
        """`x_stats`: the BatchNorm sums of x if the kernel that produced x already reduced them (the previous
        Bottleneck's last 1x1 convolution); `mod._out_stats` receives those of y when `mod.emit_stats` is set.  In
        training mode the statistics of the two 1x1 outputs (t1 here, y for the next block) ride in the GEMM
        epilogues (fp64 partial sums, STAT_FUSION) instead of costing a pass over the tensor each; the first and — for
        C <= 128 — the third BatchNorm + GELU are applied inside the loaders of the GEMMs that consume them
        (FUSE_A1 / FUSE_A3), so a1 / a3 are neither written nor saved."""
        xc = _c(x)
        if xc is not x:
            x_stats = None
        x = xc
        bn1, bn2, bn3 = mod.f[0], mod.f[3], mod.f[6]
        groups = mod.f[5].groups
        training = _use_batch_stats(bn1)
        fuse = training and STAT_FUSION
        emit = fuse and getattr(mod, "emit_stats", False)
        C, mid, hw = x.shape[1], w1.shape[0], x.shape[2] * x.shape[3]
        sto = _storage(x)

        def route(op, m, k, pro=False, res="none"):
            return ops.conv1x1_route(op, m, k, hw, sto, pro, False, res)
        # the routes of the 1x1 products, each asked once (host time per block shows in the step) — (M = mid, K = C): the
        # C -> C/4 forward r1 and the C/4 -> C data gradient d3; (M = C, K = mid): the C/4 -> C forward r3 and the C -> C/4 data
        # gradient d1
        fused1 = FUSE_A1 and C <= FUSE_A1_MAXC and ops.conv1x1_bnact_supported(x, mid)
        r1, r3 = route("fwd", mid, C, fused1), route("fwd", C, mid, True, "ordinary")
        fused3 = (FUSE_A3 and C <= (FUSE_A3_MAXC_C1R if r3 in ("c1r", "c1rb") else FUSE_A3_MAXC)     # register-direct: see above
                  and ops.conv1x1_bnact_supported((x.shape[0], mid) + x.shape[2:], C))
        if not fused3:
            r3 = route("fwd", C, mid, False, "ordinary")
        # csrc/c1b.hip takes a bf16 weight plane each way (they exist for bf16-stored tensors only): both pairs are written once
        # here when a product of the block routes to it, and a transposed plane is kept for the data gradient that does
        d1, d3 = (route("dgrad", C, mid), route("dgrad", mid, C)) if sto == "bf16" else (None, None)
        W1p, W3p = (ops.c1b_weights(w1), ops.c1b_weights(w3)) if "c1b" in (r1, r3, d1, d3) else ((None, None), (None, None))
        st1 = _bn_stats_rows(x_stats if (fuse or isinstance(x_stats, ops.StatParts)) else None, x, bn1, training)
        a1 = None if fused1 else ops.bn_act_fwd(x, st1, 1)
        t1, sr2 = _c1(w1, W1p[0], False, *((x, st1) if fused1 else (a1, None)), None, fuse, r1)
        st2 = _bn_stats_rows(sr2, t1, bn2, training)
        a2 = ops.bn_act_fwd(t1, st2, 1)
        t2 = _g3_fwd(a2, wg, groups)
        st3 = _bn_stats(t2, bn3, training)
        a3 = None if fused3 else ops.bn_act_fwd(t2, st3, 1)
        y, mod._out_stats = _c1(w3, W3p[0], False, *((t2, st3) if fused3 else (a3, None)), x, emit, r3)
        ctx.save_for_backward(x, _opt(a1), t1, a2, t2, _opt(a3), g1, w1, g2, wg, g3, w3,
                              st1.mean, st1.invstd, st1.scale, st1.shift,
                              st2.mean, st2.invstd, st2.scale, st2.shift,
                              st3.mean, st3.invstd, st3.scale, st3.shift,
                              _opt(W1p[1] if d1 == "c1b" else None), _opt(W3p[1] if d3 == "c1b" else None))
        ctx.training = training
        ctx.groups = groups
        ctx.betas = (b1, b2, b3)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x, a1, t1, a2, t2, a3, g1, w1, g2, wg, g3, w3, *s) = ctx.saved_tensors
        st1, st2, st3 = _mk_stats(*s[0:4]), _mk_stats(*s[4:8]), _mk_stats(*s[8:12])
        W1t, W3t = s[12], s[13]     # bf16 planes of w1^T (M = C, K = mid) and w3^T (M = mid, K = C); empty: fp32 storage
        tr = ctx.training
        dy = _c(dy)
        mid = w1.shape[0]
        dw3 = grad_buffer(w3)
        da3 = None
        if a3.numel() == 0:     # a3 = gelu(bn3(t2)) was never materialised: rebuilt in the weight gradient's loader
            if ops.conv1x1_wd_route(dy.shape[1], mid, dy.shape[2] * dy.shape[3], _storage(dy)) == "c1wd":
                # dW3 and dA3 = W3^T dy in one pass over dy, on the main stream (the side stream only fills launch tails)
                da3 = _on_main(lambda: ops.conv1x1_bwd_wd(dy, t2, st3, w3, dw3))
            if da3 is None:
                _wgrad(lambda: ops.conv1x1_bwd_weight_bnact(dy, t2, st3, dw3), dy, t2, st3.scale, st3.shift)
        else:
            _wgrad(lambda: ops.conv1x1_bwd_weight(dy, a3, dw3), dy, a3)
        dg3, db3 = grad_buffer(g3), grad_buffer(ctx.betas[2])
        if da3 is not None:
            dt2 = ops.bn_act_bwd(da3, t2, g3, st3, dg3, db3, None, 1, tr)
        else:
            dt2 = _dgrad_bn(dy, w3, W3t, t2, g3, st3, dg3, db3, None, tr)
        del da3
        dwg = grad_buffer(wg)
        _wgrad(lambda: _g3_wgrad(dt2, a2, dwg, ctx.groups), dt2, a2)
        da2 = _g3_dgrad(dt2, wg, mid, ctx.groups)
        del dt2
        dg2, db2 = grad_buffer(g2), grad_buffer(ctx.betas[1])
        dt1 = ops.bn_act_bwd(da2, t1, g2, st2, dg2, db2, None, 1, tr)
        del da2
        dw1 = grad_buffer(w1)
        rows1 = None
        if a1.numel() == 0:     # a1 was never materialised: the weight gradient rebuilds it from x in its loader
            if ops.conv1x1_ws_route(x.shape[1], mid, x.shape[2] * x.shape[3], _storage(x)) == "c1ws":
                # dW1 and the sums of the first BatchNorm's backward in one pass over x, on the main stream: it writes a gradient
                # buffer and its rows are needed there at once
                rows1 = _on_main(lambda: ops.conv1x1_bwd_ws(dt1, x, st1, w1, dw1))
            if rows1 is None:
                _wgrad(lambda: ops.conv1x1_bwd_weight_bnact(dt1, x, st1, dw1), dt1, x, st1.scale, st1.shift)
        else:
            _wgrad(lambda: ops.conv1x1_bwd_weight(dt1, a1, dw1), dt1, a1)
        dg1, db1 = grad_buffer(g1), grad_buffer(ctx.betas[0])
        dx = _dgrad_bn(dt1, w1, W1t, x, g1, st1, dg1, db1, dy, tr, rows1)
        return dx, dg1, db1, dw1, dg2, db2, dwg, dg3, db3, dw3, None, None


# ------------------------------------------------------------ leaf layers --
class Conv1x1Fn(Function):
    """y = conv1x1(x, w) + bias (+ pos broadcast over the batch)."""

    @staticmethod
    def forward(ctx, x, w, bias, pos):
        # the latent projections (enc[4], dec[0]) are fp32 layers: in the bf16-storage mode the (small) neighbouring
        # activation is converted at this boundary, the result is fp32
        ctx.x_dtype = x.dtype
        x = ops.to_f32(_c(x))
        y = ops.conv1x1_fwd(x, w, bias, None if pos is None else _c(pos), pos is not None)
        ctx.save_for_backward(x, w)
        ctx.bias, ctx.pos = bias, pos
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = ops.to_f32(_c(dy))
        nb, cout, h, wd = dy.shape
        dw = grad_buffer(w)
        ops.conv1x1_bwd_weight(dy, x, dw)
        dx = ops.to_dtype(ops.conv1x1_bwd_data(dy, w), ctx.x_dtype) if ctx.needs_input_grad[0] else None
        dbias = dpos = None
        if ctx.bias is not None:
            dbias = grad_buffer(ctx.bias)
            ops.reduce_sum(dy, nb, cout, h * wd, dbias)
        if ctx.pos is not None:
            dpos = grad_buffer(ctx.pos)
            ops.reduce_sum(dy, nb, cout * h * wd, 1, dpos)
        return dx, dw, dbias, dpos


def conv1x1(x, w, bias=None, pos=None):
    return Conv1x1Fn.apply(x, w, bias, pos)


class LinearFn(Function):
    @staticmethod
    def forward(ctx, x, w, bias):
        x = _c(x)
        y = ops.linear_fwd(x, w, bias)
        ctx.save_for_backward(x, w)
        ctx.bias = bias
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = _c(dy)
        dw = grad_buffer(w)
        ops.linear_bwd_weight(dy, x, dw)
        dx = ops.linear_bwd_data(dy, w) if ctx.needs_input_grad[0] else None
        dbias = None
        if ctx.bias is not None:
            dbias = grad_buffer(ctx.bias)
            ops.reduce_sum(dy, dy.shape[0], w.shape[0], 1, dbias)
        return dx, dw, dbias


class DConvFn(Function):
    """3x3 'same' stride-1 convolution with any group count (direct kernels)."""

    @staticmethod
    def forward(ctx, x, w, bias, groups):
        x = _c(x)
        y = ops.dconv_fwd(x, w, bias, 3, 1, 1, groups)
        ctx.save_for_backward(x, w)
        ctx.groups = groups
        ctx.bias = bias
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = _c(dy)
        dw = grad_buffer(w)
        ops.dconv_bwd_weight(dy, x, dw, 3, 1, 1, ctx.groups)
        dx = ops.dconv_bwd_data(dy, w, x.shape[1], 3, 1, ctx.groups, out_dtype=x.dtype) if ctx.needs_input_grad[0] else None
        dbias = None
        if ctx.bias is not None:
            nb, cout, h, wd = dy.shape
            dbias = grad_buffer(ctx.bias)
            ops.reduce_sum(dy, nb, cout, h * wd, dbias)
        return dx, dw, dbias, None


class Conv4x4DownFn(Function):
    @staticmethod
    def forward(ctx, x, w):
        x = _c(x)
        ctx.save_for_backward(x, w)
        return _down_fwd(x, w)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = _c(dy)
        dw = grad_buffer(w)
        _down_wgrad(dy, x, dw)
        dx = ops.conv4x4s2_up(dy, w) if ctx.needs_input_grad[0] else None
        return dx, dw


class ConvT4x4UpFn(Function):
    @staticmethod
    def forward(ctx, x, w):
        x = _c(x)
        ctx.save_for_backward(x, w)
        return ops.conv4x4s2_up(x, w)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = _c(dy)
        dw = grad_buffer(w)
        ops.conv4x4s2_wgrad(x, dy, dw)
        dx = ops.conv4x4s2_down(dy, w) if ctx.needs_input_grad[0] else None
        return dx, dw


class BatchNormActFn(Function):
    """BatchNorm2d (+ optional fused GELU) as a standalone layer."""

    @staticmethod
    def forward(ctx, x, gamma, beta, bn, act):
        x = _c(x)
        training = _use_batch_stats(bn)
        st = _bn_stats(x, bn, training)
        y = ops.bn_act_fwd(x, st, act)
        ctx.save_for_backward(x, gamma, st.mean, st.invstd, st.scale, st.shift)
        ctx.training, ctx.act, ctx.beta = training, act, beta
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, *s = ctx.saved_tensors
        st = _mk_stats(*s)
        dg, db = grad_buffer(gamma), grad_buffer(ctx.beta)
        dx = ops.bn_act_bwd(_c(dy), x, gamma, st, dg, db, None, ctx.act, ctx.training,
                            need_dx=ctx.needs_input_grad[0])
        return dx, dg, db, None, None


class GeluFn(Function):
    @staticmethod
    def forward(ctx, x):
        x = _c(x)
        ctx.save_for_backward(x)
        return ops.gelu_fwd(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return ops.gelu_bwd(_c(dy), x)


class SigmoidFn(Function):
    @staticmethod
    def forward(ctx, x):
        y = ops.sigmoid_fwd(_c(x))
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return ops.sigmoid_bwd(_c(dy), y)


class AddFn(Function):
    @staticmethod
    def forward(ctx, a, b):
        return ops.add(_c(a), _c(b))

    @staticmethod
    def backward(ctx, dy):
        return dy, dy


# ------------------------------------------------------- latent transformer --
class AddLayerNormFn(Function):
    """LayerNorm(x + res): the post-norm residual of nn.TransformerEncoderLayer.  res None: LayerNorm(x), the norm of a
    pre-norm layer."""

    @staticmethod
    def forward(ctx, x, res, gamma, beta, eps):
        x, res = _c(x), None if res is None else _c(res)
        y, mean, rstd = ops.layernorm_fwd(x, res, gamma, beta, eps)
        ctx.save_for_backward(x, res, gamma, mean, rstd)
        ctx.beta = beta
        return y

    @staticmethod
    def backward(ctx, dy):
        x, res, gamma, mean, rstd = ctx.saved_tensors
        dg, db = grad_buffer(gamma), grad_buffer(ctx.beta)
        dh = ops.layernorm_bwd(_c(dy), x, res, gamma, mean, rstd, dg, db)
        return dh, None if res is None else dh, dg, db, None


class MhaSeqFirstFn(Function):
    @staticmethod
    def forward(ctx, qkv, s, n, h, p_drop, seed, batch_first=False):
        qkv = _c(qkv)
        d = qkv.shape[1] // (3 * h)
        out, probs = ops.mha_fwd(qkv, s, n, h, d, p_drop, seed, batch_first)
        ctx.save_for_backward(qkv, probs)
        ctx.cfg = (s, n, h, d, p_drop, seed, batch_first)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, probs = ctx.saved_tensors
        return ops.mha_bwd(qkv, probs, _c(dout), *ctx.cfg), None, None, None, None, None, None


class SingleQueryAttnFn(Function):
    """attention of one (projected) query per batch element over L projected key/value tokens
    (GlobalCrossEncode, pipeline/models/ae_vit.py:22-42)"""

    @staticmethod
    def forward(ctx, q, kv, l, h):
        q, kv = _c(q), _c(kv)
        b = q.shape[0]
        d = q.shape[1] // h
        out, probs = ops.sq_attn_fwd(q, kv, b, l, h, d)
        ctx.save_for_backward(q, kv, probs)
        ctx.cfg = (b, l, h, d)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, kv, probs = ctx.saved_tensors
        dq, dkv = ops.sq_attn_bwd(q, kv, probs, _c(dout), *ctx.cfg)
        return dq, dkv, None, None


class AddBcastFn(Function):
    """x (B, ...) + p (...) with p a parameter broadcast over the leading dimension (positional tokens)"""

    @staticmethod
    def forward(ctx, x, p):
        ctx.p = p
        return ops.add_bcast(_c(x), _c(p))

    @staticmethod
    def backward(ctx, dy):
        dy = _c(dy)
        dp = None
        if ctx.needs_input_grad[1]:
            dp = grad_buffer(ctx.p)
            ops.reduce_sum(dy, dy.numel() // dp.numel(), dp.numel(), 1, dp)
        return dy, dp


class ExpandRowsFn(Function):
    """(1, F) parameter -> (B, F) rows (query_vec.expand, dec_queries.expand in AE_ViT_2048.forward): wfae_copy_rows"""

    @staticmethod
    def forward(ctx, p, b):
        ctx.p = p
        return ops.copy_rows(_c(p.detach()).view(-1), b, p.numel(), 0)   # every row = the parameter (src_ld = 0)

    @staticmethod
    def backward(ctx, dy):
        dp = grad_buffer(ctx.p)
        dy = _c(dy)
        ops.reduce_sum(dy, dy.shape[0], dp.numel(), 1, dp)
        return dp, None


class SliceColsFn(Function):
    """columns [a, b) of a 2-D tensor (a copy; the gradient is zero outside the slice)"""

    @staticmethod
    def forward(ctx, x, a, b):
        x = _c(x)
        ctx.cfg = (x.shape, a, b)
        return ops.copy_rows(x, x.shape[0], b - a, x.shape[1], src_off=a)

    @staticmethod
    def backward(ctx, dy):
        shape, a, b = ctx.cfg
        return ops.copy_rows(_c(dy), shape[0], b - a, b - a, dst_ld=shape[1], dst_off=a, zero_fill=True), None, None


class RepeatRowsFn(Function):
    """(B, F) -> (B*l, F), every row repeated l times (one latent-derived token copied to all positions)"""

    @staticmethod
    def forward(ctx, x, l):
        ctx.l = l
        x = _c(x)
        b, f = x.shape
        return ops.copy_rows(x, b * l, f, f, row_div=l)

    @staticmethod
    def backward(ctx, dy):
        l = ctx.l
        dy = _c(dy)
        return ops.sum_mid(dy, dy.shape[0] // l, l, dy.shape[1]), None


class PatchEmbedFn(Function):
    """Conv2d(C, E, kernel_size=P, stride=P) as patch folding + one GEMM (ae_vit.py:99,138-139): returns the
    token rows (B*Hp*Wp, E), i.e. already `.flatten(2).transpose(1, 2)`"""

    @staticmethod
    def forward(ctx, x, w, bias):
        p = w.shape[2]
        rows = ops.patchify(_c(x), p)
        ctx.save_for_backward(rows, w)
        ctx.bias = bias
        return ops.linear_fwd(rows, w.view(w.shape[0], -1), bias)

    @staticmethod
    def backward(ctx, dy):
        rows, w = ctx.saved_tensors
        dy = _c(dy)
        dw = grad_buffer(w)
        ops.linear_bwd_weight(dy, rows, dw.view(w.shape[0], -1))
        dbias = None
        if ctx.bias is not None:
            dbias = grad_buffer(ctx.bias)
            ops.reduce_sum(dy, dy.shape[0], dy.shape[1], 1, dbias)
        return None, dw, dbias


class UnpatchFn(Function):
    """ConvTranspose2d(E, C, kernel_size=P, stride=P) on token rows (B*Hp*Wp, E) -> image (B,C,Hp*P,Wp*P)
    (ae_vit.py:128,165-166): one GEMM + patch unfolding"""

    @staticmethod
    def forward(ctx, tok, w, bias, b, hp, wp):
        tok = _c(tok)
        e, c, p = w.shape[0], w.shape[1], w.shape[2]
        rows = ops.linear_bwd_data(tok, w.view(e, -1))          # (rows, E) x (E, C*P*P)
        ctx.save_for_backward(tok, w)
        ctx.cfg, ctx.bias = (b, c, hp, wp, p), bias
        return ops.unpatchify(rows, bias, b, c, hp, wp, p)

    @staticmethod
    def backward(ctx, dimg):
        tok, w = ctx.saved_tensors
        b, c, hp, wp, p = ctx.cfg
        drows = ops.patchify(_c(dimg), p)
        e = w.shape[0]
        dw = grad_buffer(w)
        ops.linear_bwd_weight(tok, drows, dw.view(e, -1))        # dw[e][j] = sum_rows tok[row][e] drows[row][j]
        dtok = ops.linear_fwd(drows, w.view(e, -1), None) if ctx.needs_input_grad[0] else None
        dbias = None
        if ctx.bias is not None:
            dbias = grad_buffer(ctx.bias)
            ops.reduce_sum(_c(dimg), b, c, hp * p * wp * p, dbias)
        return dtok, dw, dbias, None, None, None


class ReluFn(Function):
    @staticmethod
    def forward(ctx, x):
        y = ops.relu_fwd(_c(x))
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return ops.relu_bwd(_c(dy), y)


class DropoutFn(Function):
    """y = x * mask / (1-p); the mask is a pure function of (seed, element index), so backward
    applies the same kernel to dy."""

    @staticmethod
    def forward(ctx, x, p_drop, seed):
        ctx.cfg = (p_drop, seed)
        return ops.dropout(_c(x), p_drop, seed)

    @staticmethod
    def backward(ctx, dy):
        return ops.dropout(_c(dy), *ctx.cfg), None, None


_seed_counter = [0]


def next_seed():
    _seed_counter[0] += 1
    return (torch.initial_seed() * 1000003 + _seed_counter[0]) & 0x7FFFFFFFFFFFFFFF


def dropout(x, p, training):
    if not training or p <= 0.0:
        return x
    return DropoutFn.apply(x, float(p), next_seed())


# ------------------------------------------------------------------- losses --
class L1LossFn(Function):
    """weight * mean |recon - x|  (F.l1_loss, experiments/ae_v2/train.py:55)."""

    @staticmethod
    def forward(ctx, recon, x, weight):
        recon, x = _c(recon), _c(x)
        ctx.save_for_backward(recon, x)
        ctx.weight = float(weight)
        return ops.l1_fwd(recon, x, ctx.weight)

    @staticmethod
    def backward(ctx, g):
        recon, x = ctx.saved_tensors
        return ops.l1_bwd(recon, x, _c(g), ctx.weight), None, None


class SsimFn(Function):
    """pytorch_msssim.ssim(X, Y, data_range=1): gradient flows to Y (train.py:62)."""

    @staticmethod
    def forward(ctx, x, y):
        x, y = _c(x), _c(y)
        ctx.save_for_backward(x, y)
        return ops.ssim_fwd(x, y, False)

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        return None, ops.ssim_bwd(x, y, _c(g))


class MseLossFn(Function):
    """F.mse_loss(pred, target) (reference v1_experiments/pretrained_ae_linear_sevir/train.py:82)"""

    @staticmethod
    def forward(ctx, pred, target):
        pred, target = _c(pred), _c(target)
        ctx.save_for_backward(pred, target)
        return ops.mse_fwd(pred, target)

    @staticmethod
    def backward(ctx, g):
        pred, target = ctx.saved_tensors
        return ops.mse_bwd(pred, target, _c(g)), None


def mse_loss(pred, target):
    return MseLossFn.apply(pred, target)


def l1_loss(recon, x, weight=1.0):
    return L1LossFn.apply(recon, x, weight)


def ssim(x, y):
    return SsimFn.apply(x, y)


class DLinearFn(Function):
    """DLinear of the reference's v1 experiments (pretrained_ae_dlinear_*/train.py:50-100) on the column layout:
    v (B, R, M) -> y (B, P, M) = Ws seasonal + bs + Wt trend + bt of rows [0, L) of v, seasonal / trend the
    replicate-padded moving-average decomposition with window K.  Weights are stacked (M, P, L) when individual,
    else shared (P, L).  diff: the rows are first differenced against the last input frame (L - cf + r % cf), the
    reference's `inp - inp_t`.  The input gradient is formed only when v requires one."""

    @staticmethod
    def forward(ctx, v, ws, bs, wt, bt, L, K, individual, diff, cf):
        v = _c(v)
        P = bs.shape[-1]
        y = ops.dlinear_fwd(v, ws, bs, wt, bt, L, P, K, individual, diff, cf)
        ctx.save_for_backward(v, ws, wt)
        ctx.cfg = (L, P, K, individual, diff, cf)
        ctx.biases = (bs, bt)
        return y

    @staticmethod
    def backward(ctx, dy):
        v, ws, wt = ctx.saved_tensors
        L, P, K, individual, diff, cf = ctx.cfg
        bs, bt = ctx.biases
        dy = _c(dy)
        dws, dwt, dbs, dbt = grad_buffer(ws), grad_buffer(wt), grad_buffer(bs), grad_buffer(bt)
        ops.dlinear_bwd_weight(v, dy, dws, dbs, dwt, dbt, L, P, K, individual, diff, cf)
        dv = None
        if ctx.needs_input_grad[0]:
            dv = ops.dlinear_bwd_data(dy, ws, wt, v.shape[1], L, K, individual, diff, cf)
        return dv, dws, dbs, dwt, dbt, None, None, None, None, None


def dlinear(v, ws, bs, wt, bt, L, K, individual, diff=False, cf=1):
    return DLinearFn.apply(v, ws, bs, wt, bt, L, K, bool(individual), bool(diff), int(cf))


class SeriesDecompFn(Function):
    """series_decomp (pretrained_ae_dlinear_*/train.py:38-48): x (B, L, M) -> (x - trend, trend), trend the
    replicate-padded AvgPool1d(K, stride 1) along L"""

    @staticmethod
    def forward(ctx, x, K):
        ctx.K = K
        return ops.series_decomp_fwd(_c(x), K)

    @staticmethod
    def backward(ctx, ds, dt):
        ds = _c(ds) if ds is not None else None
        dt = _c(dt) if dt is not None else None
        if ds is None:
            ds = torch.zeros_like(dt)
        if dt is None:
            dt = torch.zeros_like(ds)
        return ops.series_decomp_bwd(ds, dt, ctx.K), None


def series_decomp(x, K):
    if K < 1 or K % 2 == 0:
        raise ops._lib.WfaeError(f"series_decomp: kernel_size must be odd and >= 1, got {K}")
    return SeriesDecompFn.apply(x, K)


class Mlp3MseFn(Function):
    """Linear-ReLU-Linear-ReLU-Linear + F.mse_loss of the intensity-statistics forecaster (reference
    v1_experiments/prediff_mlp_sevir/train.py:20-38, :65-66) -> (loss, pred) from ONE launch (csrc/prediff.hip) that
    also leaves the six parameter gradients of the loss; backward scales them by the upstream gradient into the
    parameters' gradient buffers — one launch when the six buffers are consecutive in the gradient arena, else one
    each.  x and target are data: they get no gradient, and asking for one is an error."""

    @staticmethod
    def forward(ctx, x, target, w1, b1, w2, b2, w3, b3):
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            raise ops._lib.WfaeError("mlp3_mse_loss: no gradient with respect to x or target is implemented")
        params = (w1, b1, w2, b2, w3, b3)
        sizes = [(p.numel() + 3) // 4 * 4 for p in params]   # the arena's 16-byte slots
        # padding floats between slots travel into the arena with the one-launch scale: they must stay zero there
        padded = any(n != p.numel() for p, n in zip(params[:-1], sizes[:-1]))
        flat = (torch.zeros if padded else torch.empty)(sum(sizes), dtype=torch.float32, device=x.device)
        grads, off = [], 0
        for p, n in zip(params, sizes):
            grads.append(flat[off:off + p.numel()].view_as(p))
            off += n
        pred, loss = ops.mlp3_mse(_c(x), _c(target), *params, grads=grads)
        ctx.params, ctx.flat, ctx.grads = params, flat, grads
        ctx.mark_non_differentiable(pred)
        return loss, pred

    @staticmethod
    def backward(ctx, g, _gpred):
        g = _c(g).view(1)
        bufs = [grad_buffer(p) for p in ctx.params]
        step = [(p.numel() + 3) // 4 * 4 * 4 for p in ctx.params]
        if all(bufs[i + 1].data_ptr() == bufs[i].data_ptr() + step[i] for i in range(5)) and \
                all(b._base is not None and b._base is bufs[0]._base for b in bufs):
            # consecutive slots of one arena: the padding floats between them are scaled along (they are never read)
            n = ctx.flat.numel() - (step[5] // 4 - ctx.params[5].numel())
            dst = bufs[0]._base.as_strided((n,), (1,), bufs[0].storage_offset())
            ops.scale(ctx.flat[:n], 1.0, g, out=dst)
        else:
            for src, dst in zip(ctx.grads, bufs):
                ops.scale(src, 1.0, g, out=dst)
        return (None, None, *bufs)


def mlp3_mse_loss(x, target, w1, b1, w2, b2, w3, b3):
    """-> (loss, pred)"""
    return Mlp3MseFn.apply(x, target, w1, b1, w2, b2, w3, b3)


def mlp3(x, w1, b1, w2, b2, w3, b3):
    """forward only: pred (B, out), no graph"""
    return ops.mlp3_mse(_c(x.detach()), None, w1.detach(), b1.detach(), w2.detach(), b2.detach(), w3.detach(),
                        b3.detach())[0]


class ConvLayerNormActFn(Function):
    """one unit of the conv latent autoencoder (reference v1_experiments/pretrained_ae_convae_sevir/train.py:62-108):
    LeakyReLU_slope(LayerNorm([C, H, W])(conv(x) + bias)) in one launch per sample batch (csrc/convae.hip); kind 0 =
    Conv2d 3x3 pad 1, 1 = Conv2d 4x4 stride 2 pad 1, 2 = ConvTranspose2d 4x4 stride 2 pad 1.  Saved for backward: x,
    x_hat and rstd (the pre-norm convolution output is never stored).  The data gradient is formed only when x
    requires one."""

    @staticmethod
    def forward(ctx, x, w, bias, gamma, beta, kind, slope):
        x = _c(x)
        y, xhat, _, rstd = ops.cln_fwd(x, w, bias, gamma, beta, kind, slope)
        ctx.save_for_backward(x, w, gamma, beta, xhat, rstd)
        ctx.bias, ctx.kind, ctx.slope = bias, kind, slope
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, gamma, beta, xhat, rstd = ctx.saved_tensors
        dw, db, dg, dbt = grad_buffer(w), grad_buffer(ctx.bias), grad_buffer(gamma), grad_buffer(beta)
        dx = ops.cln_bwd(_c(dy), xhat, rstd, gamma, beta, x, w, dw, db, dg, dbt, ctx.kind, ctx.slope,
                         need_dx=ctx.needs_input_grad[0])
        return dx, dw, db, dg, dbt, None, None


def conv_layernorm_act(x, w, bias, gamma, beta, kind, slope=0.01):
    return ConvLayerNormActFn.apply(x, w, bias, gamma, beta, int(kind), float(slope))


class Conv3x3s2ActFn(Function):
    """one unit of the conv + GAN latent model (reference v1_experiments/pretrained_ae_conv_disc/train.py:144-180):
    Conv2d(3x3, stride 2, padding 1) or, transposed, ConvTranspose2d(3x3, stride 2, padding 1, output_padding), with bias
    and, with act, SiLU — one entry point forward, one for the data gradient, one for the weight and bias gradients
    (csrc/c3s2.hip).  w is (Clo, Chi, 3, 3) for both module types.  Saved for backward: x and the pre-activation t, which
    is a few KiB next to the MiB of weights a recomputation would stream again; SiLU'(t) is applied inside the backward
    kernels.  The data gradient is formed only when x requires one."""

    @staticmethod
    def forward(ctx, x, w, bias, transposed, act, output_padding):
        x = _c(x)
        y, t = ops.c3s2_fwd(x, w, bias, transposed, act, output_padding, save_t=act)
        ctx.save_for_backward(x, w, t)
        ctx.bias, ctx.transposed, ctx.act = bias, transposed, act
        return y

    @staticmethod
    def backward(ctx, da):
        x, w, t = ctx.saved_tensors
        da = _c(da)
        dw = db = dx = None
        need_w, need_b = ctx.needs_input_grad[1], ctx.bias is not None and ctx.needs_input_grad[2]
        if need_w or need_b:
            # one launch gives both; a frozen weight next to a trainable bias gets a throw-away buffer
            dw = grad_buffer(w) if need_w else torch.empty_like(w)
            db = grad_buffer(ctx.bias) if need_b else None
            ops.c3s2_bwd_weight(da, t, x, dw, db, ctx.transposed, ctx.act)
            if not need_w:
                dw = None
        if ctx.needs_input_grad[0]:
            dx = ops.c3s2_bwd_data(da, t, w, x.shape, ctx.transposed, ctx.act)
        return dx, dw, db, None, None, None


def conv3x3s2_act(x, w, bias=None, transposed=False, act=True, output_padding=1):
    return Conv3x3s2ActFn.apply(x, w, bias, bool(transposed), bool(act), output_padding)


class HuberLossFn(Function):
    """nn.HuberLoss(delta) with mean reduction (reference pretrained_ae_convae_sevir/train.py:155)"""

    @staticmethod
    def forward(ctx, pred, target, delta):
        pred, target = _c(pred), _c(target)
        ctx.save_for_backward(pred, target)
        ctx.delta = delta
        return ops.huber_fwd(pred, target, delta)

    @staticmethod
    def backward(ctx, g):
        pred, target = ctx.saved_tensors
        return ops.huber_bwd(pred, target, _c(g), ctx.delta), None, None


def huber_loss(pred, target, delta=1.0):
    return HuberLossFn.apply(pred, target, float(delta))


# ---- frozen AutoencoderKL latent provider: forward-only building blocks (csrc/aekl.hip).  No autograd Function: the
# provider is frozen, and a tensor that asks for a gradient is refused instead of being answered without a graph.
def _aekl_no_grad(what, *ts):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts):
        raise ops._lib.WfaeError(f"{what} is forward only (the AutoencoderKL provider is frozen): call it under "
                                 "torch.no_grad() or detach its input")


def aekl_group_norm_stats(x, gamma, beta, groups, eps=1e-6):
    """-> (mean, rstd, scale, shift) of nn.GroupNorm(groups, C, eps): ops.aekl_gn_stats"""
    _aekl_no_grad("aekl_group_norm_stats", x)
    return ops.aekl_gn_stats(_c(x.detach()), gamma.detach(), beta.detach(), int(groups), float(eps))


def aekl_conv3x3(x, packed, cout, bias=None, gn=None, res=None, kind=0, out_mul=1.0, mode=None):
    """3x3 convolution of the provider on the matrix cores, with the GroupNorm + SiLU prologue `gn` and the
    bias / residual / scale epilogue: ops.aekl_conv3_fwd"""
    _aekl_no_grad("aekl_conv3x3", x, res)
    return ops.aekl_conv3_fwd(_c(x.detach()), packed, int(cout), None if bias is None else bias.detach(), gn,
                              None if res is None else _c(res.detach()), int(kind), mode, float(out_mul))


def aekl_attention(x, gn, wq, bq, wk, bk, wv, bv, wo, bo, rescale=1.0, row_invariant=False):
    """single-head AttentionBlock on x (N, C, H, W) with the folded GroupNorm affine gn = (scale, shift):
    (proj(softmax(q k^T / sqrt C) v) + x) / rescale.  The four products run on linear_fwd / split_gemm; with
    `row_invariant` on linear_fwd_rowinv, whose result for a token does not depend on how many samples share the call."""
    _aekl_no_grad("aekl_attention", x)
    x = _c(x.detach())
    n, c, h, w = x.shape
    s = h * w
    planes = 1 if ops.get_float32_matmul_precision() == "medium" else 3
    linear = ops.linear_fwd_rowinv if row_invariant else ops.linear_fwd
    tok = ops.aekl_to_tokens(x, gn).view(n * s, c)
    q = linear(tok, wq.detach(), bq.detach()).view(n, s, c)
    k = linear(tok, wk.detach(), bk.detach()).view(n, s, c)
    v = linear(tok, wv.detach(), bv.detach()).view(n, s, c)
    scores = ops.split_gemm(ops.split_bf16x3(q, planes), ops.split_bf16x3(k, planes), b_kind=1)   # (n, s, s)
    probs = ops.aekl_softmax(scores, 1.0 / float(c) ** 0.5)
    ctxv = ops.split_gemm(ops.split_bf16x3(probs, planes), ops.split_bf16x3(v, planes), b_kind=0)   # (n, s, c)
    out = linear(ctxv.view(n * s, c), wo.detach(), bo.detach()).view(n, s, c)
    return ops.aekl_from_tokens(out, x.shape, x, 1.0 / float(rescale))


def aekl_conv1x1_rowinv(x, w, bias=None):
    """1x1 convolution of the frozen provider, x (N, Cin, H, W), w (Cout, Cin[, 1, 1]), whose result for a sample does not
    depend on the batch size.  ops.conv1x1_fwd with a bias runs on gemm.hip, which from Cin >= 128 and Cout >= 64 on chooses
    between the three-plane split and the fp32 matrix instruction by the column count N H W (`launch_gemm_v`, `pick_bm`).
    So: channel counts and H W that are multiples of 32 go through tokens — to_tokens, linear_fwd_rowinv, from_tokens, the
    two layout kernels being copies; below Cin = 128 the default kernel has one instruction and one k-order for every batch
    size and is kept; anything else is refused."""
    _aekl_no_grad("aekl_conv1x1_rowinv", x)
    x = _c(x.detach())
    n, c, h, wd = x.shape
    cout = w.shape[0]
    w2 = w.detach().reshape(cout, c)
    b = None if bias is None else bias.detach()
    if c % 32 == 0 and cout % 32 == 0 and (h * wd) % 32 == 0 and max(c, cout) <= 4096:
        tok = ops.aekl_to_tokens(x).view(n * h * wd, c)
        out = ops.linear_fwd_rowinv(tok, w2, b).view(n, h * wd, cout)
        return ops.aekl_from_tokens(out, (n, cout, h, wd))
    if c >= 128:
        raise ops._lib.WfaeError(f"aekl_conv1x1_rowinv: Cin={c}, Cout={cout}, H*W={h * wd}: from Cin = 128 on the pass-invariant "
                                 "form needs channel counts and H*W that are multiples of 32 (channels up to 4096)")
    return ops.conv1x1_fwd(x, w2, b)


def aekl_posterior(moments, noise=None):
    """-> (mean, logvar, std, sample): ops.aekl_posterior"""
    _aekl_no_grad("aekl_posterior", moments)
    return ops.aekl_posterior(_c(moments.detach()), None if noise is None else _c(noise))


# ---- AutoencoderKL training (csrc/aekl_bwd.hip): the autograd Functions behind `AutoencoderKL.unfreeze()`.  They save
# inputs and statistics, never an activated tensor, keep nothing that a backward consumes, and so run a second backward
# under retain_graph (the adaptive weight of the KL-GAN loss differentiates twice before backward).
class AeklConv3Fn(Function):
    """(conv3x3(SiLU(GroupNorm(x))) + bias + res) * out_mul on ops.aekl_conv3_fwd; `norm` None: the plain convolution.
    `conv` is the pipeline's Conv3x3: it owns the packed weights of both orientations."""

    @staticmethod
    def forward(ctx, x, w, bias, gamma, beta, res, conv, norm, kind, out_mul, mode):
        x = _c(x)
        gn = mean = rstd = None
        if norm is not None:
            mean, rstd, scale, shift = ops.aekl_gn_stats(x, gamma, beta, norm.num_groups, norm.eps)
            gn = (scale, shift)
        y = ops.aekl_conv3_fwd(x, conv.packed(mode), w.shape[0], bias, gn, None if res is None else _c(res), kind, mode, out_mul)
        ctx.save_for_backward(x, w, gamma, mean, rstd, *(gn or ()))
        ctx.conv, ctx.bias, ctx.has_res, ctx.kind, ctx.out_mul, ctx.mode = conv, bias, res is not None, kind, out_mul, mode
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, gamma, mean, rstd, *gn = ctx.saved_tensors
        gn = tuple(gn) if gn else None
        dy = _c(dy)
        if ctx.out_mul != 1.0:
            dy = dy * ctx.out_mul
        dw, dbias = grad_buffer(w), None if ctx.bias is None else grad_buffer(ctx.bias)
        ops.aekl_conv3_bwd_weight(dy, x, dw, dbias, gn, ctx.kind, ctx.mode)
        dx = dgamma = dbeta = None
        if gn is not None or ctx.needs_input_grad[0]:
            dx = ops.aekl_conv3_bwd_data(dy, ctx.conv.packed_t(ctx.mode), x, gn, ctx.kind, ctx.mode)
        if gn is not None:
            dx, dgamma, dbeta = ops.aekl_gn_bwd(dx, x, gamma, mean, rstd)
        return dx, dw, dbias, dgamma, dbeta, (dy if ctx.has_res else None), None, None, None, None, None


def aekl_conv3x3_train(x, conv, norm=None, res=None, kind=0, out_mul=1.0, mode=None):
    mode = ops.aekl_mode() if mode is None else mode
    gamma, beta = (norm.weight, norm.bias) if norm is not None else (None, None)
    return AeklConv3Fn.apply(x, conv.weight, conv.bias, gamma, beta, res, conv, norm, int(kind), float(out_mul), mode)


class AeklAttentionFn(Function):
    """the single-head AttentionBlock of aekl_attention with its GroupNorm, differentiable: the five products of the backward
    run on linear_bwd_data / linear_bwd_weight / split_gemm, the transposes on the token kernels"""

    @staticmethod
    def forward(ctx, x, gamma, beta, wq, bq, wk, bk, wv, bv, wo, bo, groups, eps, rescale):
        x = _c(x)
        n, c, h, w = x.shape
        s = h * w
        planes = 1 if ops.get_float32_matmul_precision() == "medium" else 3
        mean, rstd, scale, shift = ops.aekl_gn_stats(x, gamma, beta, groups, eps)
        tok = ops.aekl_to_tokens(x, (scale, shift)).view(n * s, c)
        q = ops.linear_fwd(tok, wq, bq).view(n, s, c)
        k = ops.linear_fwd(tok, wk, bk).view(n, s, c)
        v = ops.linear_fwd(tok, wv, bv).view(n, s, c)
        scores = ops.split_gemm(ops.split_bf16x3(q, planes), ops.split_bf16x3(k, planes), b_kind=1)
        probs = ops.aekl_softmax(scores, 1.0 / float(c) ** 0.5)
        ctxv = ops.split_gemm(ops.split_bf16x3(probs, planes), ops.split_bf16x3(v, planes), b_kind=0)
        out = ops.linear_fwd(ctxv.view(n * s, c), wo, bo).view(n, s, c)
        ctx.save_for_backward(x, gamma, mean, rstd, tok, q, k, v, probs, ctxv, wq, wk, wv, wo)
        ctx.biases, ctx.rescale, ctx.planes = (bq, bk, bv, bo), rescale, planes
        return ops.aekl_from_tokens(out, x.shape, x, 1.0 / float(rescale))

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mean, rstd, tok, q, k, v, probs, ctxv, wq, wk, wv, wo = ctx.saved_tensors
        n, c, h, w = x.shape
        s, planes = h * w, ctx.planes
        dy = _c(dy)
        if ctx.rescale != 1.0:
            dy = dy * (1.0 / float(ctx.rescale))
        sp = lambda t: ops.split_bf16x3(_c(t), planes)

        def lin_bwd(d, inp, wt, b):
            dwt = grad_buffer(wt)
            ops.linear_bwd_weight(d, inp, dwt)
            db = grad_buffer(b)
            ops.reduce_sum(d, d.shape[0], wt.shape[0], 1, db)
            return ops.linear_bwd_data(d, wt), dwt, db

        dout = ops.aekl_to_tokens(dy).view(n * s, c)
        dctx, dwo, dbo = lin_bwd(dout, ctxv.view(n * s, c), wo, ctx.biases[3])
        dctx3 = sp(dctx.view(n, s, c))
        dprobs = ops.split_gemm(dctx3, sp(v), b_kind=1)                                # (n, s_q, s_k)
        dv = ops.split_gemm(sp(ops.aekl_to_tokens(probs)), dctx3, b_kind=0)            # probs^T dctx
        ds = ops.aekl_softmax_bwd(probs, dprobs, 1.0 / float(c) ** 0.5)
        dq = ops.split_gemm(sp(ds), sp(k), b_kind=0)
        dk = ops.split_gemm(sp(ops.aekl_to_tokens(ds)), sp(q), b_kind=0)               # ds^T q
        dtq, dwq, dbq = lin_bwd(dq.view(n * s, c), tok, wq, ctx.biases[0])
        dtk, dwk, dbk = lin_bwd(dk.view(n * s, c), tok, wk, ctx.biases[1])
        dtv, dwv, dbv = lin_bwd(dv.view(n * s, c), tok, wv, ctx.biases[2])
        dtok = (dtq + dtk + dtv).view(n, s, c)
        du = ops.aekl_from_tokens(dtok, x.shape)
        dx, dgamma, dbeta = ops.aekl_gn_bwd(du, x, gamma, mean, rstd, skip=dy)         # skip: the residual path
        return dx, dgamma, dbeta, dwq, dbq, dwk, dbk, dwv, dbv, dwo, dbo, None, None, None


def aekl_attention_train(x, norm, q, k, v, o, rescale=1.0):
    return AeklAttentionFn.apply(x, norm.weight, norm.bias, q.weight, q.bias, k.weight, k.bias, v.weight, v.bias, o.weight,
                                 o.bias, int(norm.num_groups), float(norm.eps), float(rescale))


class AeklPosteriorSampleFn(Function):
    """z = mean + std * noise of the moments (noise None: the mean, `mode()`)"""

    @staticmethod
    def forward(ctx, moments, noise):
        moments = _c(moments)
        noise = None if noise is None else _c(noise)
        mean, _, _, sample = ops.aekl_posterior(moments, noise)
        ctx.save_for_backward(moments, *(() if noise is None else (noise,)))
        return mean if noise is None else sample

    @staticmethod
    def backward(ctx, dz):
        moments, *noise = ctx.saved_tensors
        return ops.aekl_posterior_bwd(moments, _c(dz), noise[0] if noise else None), None


class AeklPosteriorKlFn(Function):
    """kl (N) = 0.5 sum(mean^2 + var - 1 - logvar) per sample"""

    @staticmethod
    def forward(ctx, moments):
        moments = _c(moments)
        mean, logvar, std, _ = ops.aekl_posterior(moments)
        ctx.save_for_backward(moments)
        return 0.5 * torch.sum(mean * mean + std * std - 1.0 - logvar, dim=[1, 2, 3])

    @staticmethod
    def backward(ctx, gkl):
        moments, = ctx.saved_tensors
        return ops.aekl_posterior_bwd(moments, gkl=_c(gkl))


# ---- LPIPS perceptual loss (csrc/lpips.hip; reference pipeline/models/autoencoderkl/losses/lpips.py:47-60,107-129)
LPIPS_SLICES = (2, 2, 3, 3, 3)   # 3x3 conv + ReLU layers per VGG16 slice; a 2 x 2 max-pool opens slices 2..5; a tap closes each


class LpipsFn(Function):
    """(N, 1, 1, 1) LPIPS distance of x to target, gradient to x only.  `st` (losses/lpips.py `LPIPS._state`) carries the
    frozen operands: shift, scale, 13 packed forward weights `fwd`, 13 packed rotated / transposed weights `bwd`, biases,
    input channel counts `cin`, 5 `lin` vectors and the conv `mode`.  x and target go through the VGG as one 2N batch.
    Saved for backward: the five tap activations whole (the target half is the distance's second operand) and a copy of
    the recon half of the other eight.  backward only reads them and allocates its results, so it may run any number
    of times (autograd.grad(..., retain_graph=True) for the adaptive weight, then the real backward).  `sink`: a list
    that receives the recon half of the 13 activations, or None."""

    @staticmethod
    def forward(ctx, x, target, st, sink):
        x, target = _c(x), _c(target)
        n, _, h, w = x.shape
        z = torch.empty((2 * n, 3, h, w), dtype=torch.float32, device=x.device)
        ops.lpips_prep_fwd(x, st.shift, st.scale, z[:n])
        ops.lpips_prep_fwd(target, st.shift, st.scale, z[n:])
        keep = ctx.needs_input_grad[0]
        out = torch.zeros((n, 1, 1, 1), dtype=torch.float32, device=x.device)
        saved, li, hcur = [], 0, z
        for s, nconv in enumerate(LPIPS_SLICES):
            if s:
                hcur = ops.lpips_pool_fwd(hcur)
            for j in range(nconv):
                hcur = ops.lpips_conv3_fwd(hcur, st.fwd[li], st.bias[li], st.mode)
                li += 1
                tap = j == nconv - 1
                if tap:
                    ops.lpips_dist_fwd(hcur[:n], hcur[n:], st.lin[s], out)
                if keep or sink is not None:
                    saved.append(hcur if tap else hcur[:n].clone())
        if sink is not None:
            sink.extend(a[:n] for a in saved)
        if keep:
            ctx.save_for_backward(*saved)
            ctx.st, ctx.cx = st, x.shape[1]
        return out

    @staticmethod
    def backward(ctx, g):
        saved, st = ctx.saved_tensors, ctx.st
        g = _c(g).view(-1)
        n = g.numel()
        li, d = len(saved) - 1, None
        for s in reversed(range(len(LPIPS_SLICES))):
            a0, a1 = saved[li][:n], saved[li][n:]
            if d is None:      # relu5_3: no pool follows, the distance gradient takes the ReLU mask itself
                d = ops.lpips_dist_bwd(a0, a1, st.lin[s], g, relu=True)
            else:
                d = ops.lpips_pool_bwd(a0, d, ops.lpips_dist_bwd(a0, a1, st.lin[s], g))
            for j in reversed(range(LPIPS_SLICES[s])):
                # d: gradient of layer li's pre-activation -> of the pre-activation of the layer that feeds it (the first
                # layer of a slice is fed by the pool / the scaling layer: no mask)
                d = ops.lpips_conv3_bwd_data(d, st.bwd[li], st.cin[li], saved[li - 1][:n] if j else None, st.mode)
                li -= 1
        return ops.lpips_prep_bwd(d, st.scale, ctx.cx), None, None, None


# ---- conv + attention latent autoencoder (csrc/convattn.hip; experiments/v1_experiments/_convattn.py) --------------------
class AttnFn(Function):
    """multi-head attention (heads of 16) with separate query / key lengths up to 256 and dropout on the probabilities.
    kv None: `q` is the packed (n*sq, 3E) projection [q | k | v] of a self-attention (sq == skv); otherwise q is (n*sq, E)
    and kv the packed (n*skv, 2E) projection [k | v].  Saved: the projections and the probabilities before dropout; the
    mask is regenerated from `seed`.  The gradient of a packed projection is one buffer."""

    @staticmethod
    def forward(ctx, q, kv, n, sq, skv, h, p_drop, seed):
        q = _c(q)
        kv = None if kv is None else _c(kv)
        e = q.shape[1] // 3 if kv is None else q.shape[1]
        d = e // h
        qv, kk, vv = AttnFn._views(q, kv, e)
        out, probs = ops.attn_fwd(qv, kk, vv, n, sq, skv, h, d, p_drop, seed)
        ctx.save_for_backward(q, kv, probs)
        ctx.cfg = (n, sq, skv, h, d, p_drop, seed)
        ctx.e = e
        return out

    @staticmethod
    def _views(q, kv, e):
        if kv is None:
            return q[:, :e], q[:, e:2 * e], q[:, 2 * e:]
        return q, kv[:, :e], kv[:, e:]

    @staticmethod
    def backward(ctx, dout):
        q, kv, probs = ctx.saved_tensors
        dq = torch.empty_like(q)
        dkv = None if kv is None else torch.empty_like(kv)
        ops.attn_bwd(*AttnFn._views(q, kv, ctx.e), probs, _c(dout), *AttnFn._views(dq, dkv, ctx.e), *ctx.cfg)
        return dq, dkv, None, None, None, None, None, None


class GroupNormActFn(Function):
    """GroupNorm(groups, C) (+ exact GELU with act) of x + bias[c] in training form: one launch forward, the backward
    entry point gives dx, dgamma, dbeta and the bias gradient.  Saved: x and the (N, G) statistics; the activation is
    recomputed."""

    @staticmethod
    def forward(ctx, x, gamma, beta, bias, groups, eps, act):
        x = _c(x)
        y, mean, rstd = ops.gn_act_fwd(x, gamma, beta, groups, eps, act, bias)
        ctx.save_for_backward(x, gamma, beta, mean, rstd)
        ctx.bias, ctx.cfg = bias, (groups, act)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, beta, mean, rstd = ctx.saved_tensors
        groups, act = ctx.cfg
        dg, db = grad_buffer(gamma), grad_buffer(beta)
        dbias = grad_buffer(ctx.bias) if ctx.bias is not None else None
        dx = ops.gn_act_bwd(_c(dy), x, gamma, beta, mean, rstd, dg, db, groups, act, ctx.bias, dbias)
        return dx, dg, db, dbias, None, None, None


class ChannelBiasFn(Function):
    """x (N, C, ...) + b (C): the bias of a convolution whose kernel takes none"""

    @staticmethod
    def forward(ctx, x, b):
        ctx.b = b
        return ops.channel_bias_fwd(_c(x), b)

    @staticmethod
    def backward(ctx, dy):
        dy = _c(dy)
        db = grad_buffer(ctx.b)
        n, c = dy.shape[0], dy.shape[1]
        ops.reduce_sum(dy, n, c, dy.numel() // (n * c), db)
        return dy, db


class HeadDropoutBcastFn(Function):
    """attention over ONE key in training: v (N, E) -> (N*sq, E), every query position the value row under the head-wise
    dropout mask of its (identically 1) probability.  At p = 0 this is RepeatRowsFn."""

    @staticmethod
    def forward(ctx, v, sq, h, p_drop, seed):
        v = _c(v)
        ctx.cfg = (v.shape[0], sq, h, p_drop, seed)
        return ops.head_dropout_bcast_fwd(v, sq, h, p_drop, seed)

    @staticmethod
    def backward(ctx, dout):
        return ops.head_dropout_bcast_bwd(_c(dout), *ctx.cfg), None, None, None, None


class LinearRowsFn(Function):
    """y = x w[r0:r1]^T + b[r0:r1]: the part of a packed projection that is live.  The other rows of w and b take no part
    in the output, and neither does any parameter in `dead` (a norm in front of a projection that is never formed): their
    gradients are mathematically zero and are written as exact zeros, so the optimiser applies its weight decay and
    nothing else to them."""

    @staticmethod
    def forward(ctx, x, w, b, r0, r1, *dead):
        x = _c(x)
        ctx.save_for_backward(x, w)
        ctx.b, ctx.rows, ctx.dead = b, (r0, r1), dead
        return ops.linear_fwd(x, w[r0:r1], b[r0:r1])

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        r0, r1 = ctx.rows
        dy = _c(dy)
        dw, db = grad_buffer(w).zero_(), grad_buffer(ctx.b).zero_()
        ops.linear_bwd_weight(dy, x, dw[r0:r1])
        ops.reduce_sum(dy, dy.shape[0], r1 - r0, 1, db[r0:r1])
        dx = ops.linear_bwd_data(dy, w[r0:r1]) if ctx.needs_input_grad[0] else None
        return (dx, dw, db, None, None) + tuple(grad_buffer(p).zero_() for p in ctx.dead)


class InProjFn(Function):
    """the packed in-projection [q | k | v] = x w^T + b of a self-attention.  LinearFn, but for the key bias b[e:2e]: it
    adds the same q . b_k to every score of a row, which the softmax cancels, so its gradient is mathematically zero (a sum
    of rounding errors that AdamW would normalise into steps of +-lr) and is written as exact zeros."""

    @staticmethod
    def forward(ctx, x, w, b, e):
        x = _c(x)
        ctx.save_for_backward(x, w)
        ctx.b, ctx.e = b, e
        return ops.linear_fwd(x, w, b)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = _c(dy)
        dw, db = grad_buffer(w), grad_buffer(ctx.b)
        ops.linear_bwd_weight(dy, x, dw)
        ops.reduce_sum(dy, dy.shape[0], w.shape[0], 1, db)
        db[ctx.e:2 * ctx.e].zero_()
        dx = ops.linear_bwd_data(dy, w) if ctx.needs_input_grad[0] else None
        return dx, dw, db, None


class SplitInProjFn(Function):
    """the packed in-projection of an attention whose queries and keys come from different tensors:
    q = xq w[:e]^T + b[:e], kv = xkv w[e:]^T + b[e:] -> (q, kv); the gradient of w (and of b) is one buffer, the key
    bias's exact zeros (InProjFn)"""

    @staticmethod
    def forward(ctx, xq, xkv, w, b, e):
        xq, xkv = _c(xq), _c(xkv)
        ctx.save_for_backward(xq, xkv, w)
        ctx.b, ctx.e = b, e
        return ops.linear_fwd(xq, w[:e], b[:e]), ops.linear_fwd(xkv, w[e:], b[e:])

    @staticmethod
    def backward(ctx, dq, dkv):
        xq, xkv, w = ctx.saved_tensors
        e = ctx.e
        dq, dkv = _c(dq), _c(dkv)
        dw, db = grad_buffer(w), grad_buffer(ctx.b)
        ops.linear_bwd_weight(dq, xq, dw[:e])
        ops.linear_bwd_weight(dkv, xkv, dw[e:])
        ops.reduce_sum(dq, dq.shape[0], e, 1, db[:e])
        ops.reduce_sum(dkv, dkv.shape[0], dkv.shape[1], 1, db[e:])
        db[e:2 * e].zero_()
        dxq = ops.linear_bwd_data(dq, w[:e]) if ctx.needs_input_grad[0] else None
        dxkv = ops.linear_bwd_data(dkv, w[e:]) if ctx.needs_input_grad[1] else None
        return dxq, dxkv, dw, db, None


# ---- training the ae_gan residual autoencoders (csrc/resae_bwd.hip): the autograd Functions behind `unfreeze()` of
# experiments/v1_experiments/_ae_gan.py.  One Function per block; the upsampled tensor is never written and never saved.
def _resae_bn(x, bn, replicas=1):
    """train-mode statistics of `bn` on x, the running-statistics update included; the kernels write the buffers through
    raw pointers, so their version counters are bumped here for the caches keyed on them (FoldedBatchNorm.folded)"""
    st = ops.resae_bn_stats_train(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, bn.momentum, replicas)
    bn._nbt_pending += 1
    torch.autograd.graph.increment_version([bn.running_mean, bn.running_var])
    return st


def _st4(st):
    return st.mean, st.invstd, st.scale, st.shift


class ResaeBlockFn(Function):
    """ResidualBlock in training mode, also read through the x2 upsample (UpsampleBlock):
        c1 = conv1(x)           stride 1, stride 2, or over the upsample
        h  = gelu(bn1(c1))
        c2 = conv2(h)
        cs = shortcut conv(x)   at the block INPUT's resolution (or none: the identity shortcut)
        y  = gelu(bn2(c2) + bn_s(cs) or x)                       ops.resae_join_fwd
    with batch statistics.  `blk` is the module: it owns the packed weights and the BatchNorm buffers."""

    @staticmethod
    def forward(ctx, x, w1, g1, b1, w2, g2, b2, ws, gs, bs, blk, up, route):
        x = _c(x)
        k1 = "up" if up else "down" if blk.stride == 2 else "conv"
        c1 = blk.conv1(x, k1, route=route)
        st1 = _resae_bn(c1, blk.bn1)
        h = ops.bn_act_fwd(c1, st1, 1)
        c2 = blk.conv2(h, "conv", route=route)
        st2 = _resae_bn(c2, blk.bn2)
        cs, sts = None, None
        if ws is not None:
            cs = blk.shortcut[0](x, "short_down" if blk.stride == 2 else "short", route=route)
            sts = _resae_bn(cs, blk.shortcut[1], 4 if up else 1)
        y = ops.resae_join_fwd(c2, st2.scale, st2.shift, x if cs is None else cs, None if sts is None else sts.scale,
                               None if sts is None else sts.shift, res_up=up)
        ctx.save_for_backward(x, w1, g1, w2, g2, ws, gs, c1, h, c2, cs, *_st4(st1), *_st4(st2), *(_st4(sts) if sts else ()))
        ctx.blk, ctx.up, ctx.route, ctx.k1 = blk, up, route, k1
        ctx.betas = (b1, b2, bs)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w1, g1, w2, g2, ws, gs, c1, h, c2, cs, *s = ctx.saved_tensors
        blk, up, route = ctx.blk, ctx.up, ctx.route
        b1, b2, bs = ctx.betas
        st1, st2 = _mk_stats(*s[0:4]), _mk_stats(*s[4:8])
        sts = _mk_stats(*s[8:12]) if cs is not None else None
        dpre, dres = ops.resae_join_bwd(_c(dy), c2, st2.scale, st2.shift, x if cs is None else cs,
                                        None if sts is None else sts.scale, None if sts is None else sts.shift, res_up=up)
        dg2, db2 = grad_buffer(g2), grad_buffer(b2)
        dc2 = ops.bn_act_bwd(dpre, c2, g2, st2, dg2, db2, None, 0, True)
        dw2 = grad_buffer(w2)
        ops.resae_bwd_weight(dc2, h, dw2, "conv", route=route)
        dh = ops.resae_bwd_data(dc2, blk.conv2.packed_t("conv"), h.shape, route=route)
        dg1, db1 = grad_buffer(g1), grad_buffer(b1)
        dc1 = ops.bn_act_bwd(dh, c1, g1, st1, dg1, db1, None, 1, True)
        dw1 = grad_buffer(w1)
        ops.resae_bwd_weight(dc1, x, dw1, ctx.k1, route=route)
        need_dx = ctx.needs_input_grad[0]
        dws = dgs = dbs = None
        side = dres                       # the identity shortcut: the join's gradient at r is x's
        if cs is not None:
            ks = "short_down" if blk.stride == 2 else "short"
            dgs, dbs = grad_buffer(gs), grad_buffer(bs)
            dcs = ops.bn_act_bwd(dres, cs, gs, sts, dgs, dbs, None, 0, True)
            dws = grad_buffer(ws)
            ops.resae_bwd_weight(dcs, x, dws, ks, route=route)
            side = ops.resae_bwd_data(dcs, blk.shortcut[0].packed_t(ks), x.shape, route=route) if need_dx else None
        dx = ops.resae_bwd_data(dc1, blk.conv1.packed_t(ctx.k1), x.shape, add=side, route=route) if need_dx else None
        return dx, dw1, dg1, db1, dw2, dg2, db2, dws, dgs, dbs, None, None, None


def resae_block_train(blk, x, up=False, route=None):
    sc = blk.shortcut
    ws, gs, bs = (sc[0].weight, sc[1].weight, sc[1].bias) if len(sc) else (None, None, None)
    return ResaeBlockFn.apply(x, blk.conv1.weight, blk.bn1.weight, blk.bn1.bias, blk.conv2.weight, blk.bn2.weight, blk.bn2.bias,
                              ws, gs, bs, blk, bool(up), route)


class ResaeConvFn(Function):
    """a plain convolution of the residual autoencoders with a bias (`final_conv`): ops.resae_conv and its two gradients"""

    @staticmethod
    def forward(ctx, x, w, bias, conv, kind, route):
        x = _c(x)
        ctx.save_for_backward(x, w)
        ctx.conv, ctx.bias, ctx.kind, ctx.route = conv, bias, kind, route
        return conv(x, kind, shift=bias, route=route)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = _c(dy)
        dw, dbias = grad_buffer(w), None if ctx.bias is None else grad_buffer(ctx.bias)
        ops.resae_bwd_weight(dy, x, dw, ctx.kind, dbias=dbias, route=ctx.route)
        dx = ops.resae_bwd_data(dy, ctx.conv.packed_t(ctx.kind), x.shape, route=ctx.route) if ctx.needs_input_grad[0] else None
        return dx, dw, dbias, None, None, None


def resae_conv_train(conv, x, kind="conv", route=None):
    return ResaeConvFn.apply(x, conv.weight, conv.bias, conv, kind, route)
