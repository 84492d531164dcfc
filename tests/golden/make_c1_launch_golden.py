"""Launch traces of the 1x1 products: which C entry points the package calls, in which order, with which arguments.

    python tests/golden/make_c1_launch_golden.py            # on an MI355X: writes tests/golden/g19_c1_launches.json

Only public names of weatherforecastingtoolkit_amd.ops / .functional and the model's Bottleneck module are used, so this file
records any revision of the package unmodified; tests/test_c1_dispatch_gpu.py replays the same cases on the tree under test
and tests/test_c1_route_cpu.py checks ops.conv1x1_route against the recorded entry points without a device.

A case is recorded with _lib.call replaced (ops._call reaches it through the module attribute).  One canonical line per
launch: the entry point, every integer / float argument by value, every pointer argument as null / ptr (the header's argument
types tell which is which), nothing for the stream.  The golden holds, per case, the entry-point names and the SHA-256 of the
lines.

A single-product case is one (configuration, switch, M, K, HW) and issues every FORM of that product, one launch each, in a
fixed order.  (M, K) names the product y[M] = A[M, K] x[K] whatever the operation: the forward weight is (M, K), the data
gradient takes dy with K channels and the (K, M) weight of the convolution it differentiates, the weight gradient is that
of a convolution K -> M.  Tensors stored as bf16 reach the c1rb / c1b wrappers the way the Bottleneck reaches them, by the
rule written out in _bf16_family below (deliberately not taken from the package, so that the golden does not follow an edit
of the package's own rule)."""
from __future__ import annotations

import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "g19_c1_launches.json")

NB = 2
SHAPES = [(c // 4, c) for c in (128, 256, 512, 1024)] + [(c, c // 4) for c in (128, 256, 512, 1024)] + [(24, 96)]
PIXELS = [(8, 16), (8, 24), (4, 5)]
# name -> (matmul precision, split GEMMs, bf16 activation storage)
CONFIGS = {"highest_split": ("highest", True, False), "highest_nosplit": ("highest", False, False),
           "medium_bf16": ("medium", True, True), "medium_f32": ("medium", True, False)}
# each A/B switch off, at the one configuration where it decides something
SWITCHES = {"set_c1r": "highest_split", "set_c1r_bnred": "highest_split", "set_c1r_bndx": "highest_split", "set_c1n": "highest_split",
            "set_c1rb": "medium_bf16", "set_c1b": "medium_bf16", "set_c1w": "highest_split"}
BLOCK_C = (128, 256, 512, 1024)
BLOCK_SWITCHES = ("set_c1r_bnred", "set_c1r_bndx")     # these two decide inside the block's backward only

# Arguments left out of the lines: capacities only, never a shape, a flag or a null-ness.
#   ws_bytes: the size of the per-stream workspace, which grows with the largest request the PROCESS has made so far
EXCLUDED_ARGS = {"ws_bytes"}


# ------------------------------------------------------------------ recorder
class Recorder:
    """with Recorder() as lines: ...   # _lib.call is replaced inside the block; the launches still run"""

    def __enter__(self):
        from weatherforecastingtoolkit_amd import _lib
        self._lib, self._real, self.lines = _lib, _lib.call, []
        _lib.load()
        decls = _lib.parse_header()

        def call(name, *args):
            _, argtypes, argnames = decls[name]
            assert len(args) == len(argtypes), (name, len(args), len(argtypes))
            out = [name]
            for a, t, n in zip(args, argtypes, argnames):
                if n == "stream" or n in EXCLUDED_ARGS:
                    continue
                if t.__name__ == "c_void_p":
                    v = getattr(a, "value", a)
                    out.append(f"{n}={'null' if not v else 'ptr'}")
                elif t.__name__ == "c_float":
                    out.append(f"{n}={float(a)!r}")
                else:
                    out.append(f"{n}={int(a)}")
            self.lines.append(" ".join(out))
            return self._real(name, *args)

        _lib.call = call
        return self.lines

    def __exit__(self, *exc):
        self._lib.call = self._real


def digest(lines):
    return {"names": [ln.split(" ", 1)[0] for ln in lines], "sha256": hashlib.sha256("\n".join(lines).encode()).hexdigest()}


def family_of(entry):
    """kernel family of a recorded entry point (None: not a 1x1 product)"""
    for prefix, fam in (("wfae_c1rb_fwd", "c1rb"), ("wfae_c1r_", "c1r"), ("wfae_c1b_fwd", "c1b"), ("wfae_c1w_", "c1w"),
                        ("wfae_conv1x1_", "gemm")):
        if entry.startswith(prefix):
            return fam
    return None


class configured:
    """the package in configuration `cfg` with `switch` (a set_* name or None) off; the defaults afterwards"""

    def __init__(self, cfg, switch=None):
        self.cfg, self.switch = CONFIGS[cfg], switch

    def __enter__(self):
        import torch
        from weatherforecastingtoolkit_amd import ops
        prec, split, bf16 = self.cfg
        ops.set_float32_matmul_precision(prec)
        ops.set_split_gemm(split)
        ops.set_activation_storage(torch.bfloat16 if bf16 else torch.float32)
        if self.switch:
            getattr(ops, self.switch)(False)

    def __exit__(self, *exc):
        from weatherforecastingtoolkit_amd import ops
        if self.switch:
            getattr(ops, self.switch)(True)
        ops.set_float32_matmul_precision("highest")
        ops.set_split_gemm(True)


# -------------------------------------------------------------- single products
FORMS_F32 = ["plain", "stats", "pro", "pro_stats", "res", "bias", "bres", "dgrad",
             "wgrad", "wgrad_acc", "wgrad_pro", "wgrad_pro_acc", "bnred", "bnred_nostore", "bndx"]
FORMS_BF16 = ["c1b_weights", "plain", "stats", "pro", "pro_stats", "res", "bias", "dgrad",
              "wgrad", "wgrad_acc", "wgrad_pro", "wgrad_pro_acc"]


def route_query(form, m, k, hw, bf16):
    """the product a form is, in the vocabulary of ops.conv1x1_route -> keyword arguments (None: the form is no routed product)"""
    if form == "c1b_weights":
        return None
    op = "wgrad" if form.startswith("wgrad") else "dgrad" if form in ("dgrad", "bnred", "bnred_nostore", "bndx") else "fwd"
    return dict(op=op, m=m, k=k, hw=hw, storage="bf16" if bf16 else "f32", prologue="pro" in form, bias=form == "bias",
                residual={"res": "ordinary", "bres": "broadcast"}.get(form, "none"))


def _bf16_family(ops, m, k, hw, form):
    """the family that serves a forward / data-gradient product on bf16-stored tensors: c1rb wherever it serves the shape,
    except the narrowing products of K >= 256 with the prologue; those, and what c1rb does not serve, on c1b; else gemm.hip.
    Neither has a bias, and c1rb adds a residual to widening products only."""
    if form == "bias" or (form == "res" and m <= k):
        return "gemm"
    rb = ops.c1rb_supported(m, k, hw)
    if rb and not ("pro" in form and m < k and k >= 256):
        return "c1rb"
    return "c1b" if (rb or ops.c1b_supported(m, k, hw)) else "gemm"


def single_case_ids():
    for cfg in CONFIGS:
        for m, k in SHAPES:
            for h, w in PIXELS:
                yield f"single/{cfg}/-/M{m}K{k}/hw{h * w}", cfg, None, m, k, h, w
    for switch, cfg in SWITCHES.items():
        for m, k in SHAPES:
            for h, w in PIXELS:
                yield f"single/{cfg}/{switch}/M{m}K{k}/hw{h * w}", cfg, switch, m, k, h, w


def run_single(dev, cfg, switch, m, k, h, w):
    """-> ([form names], [canonical lines]): one launch per form"""
    import torch
    from weatherforecastingtoolkit_amd import ops
    bf16 = CONFIGS[cfg][2]
    dt = torch.bfloat16 if bf16 else torch.float32
    hw = h * w

    def t(*shape, dtype=torch.float32):
        return torch.full(shape, 0.25, dtype=dtype, device=dev)

    forms, lines = [], []
    with configured(cfg, switch):
        x, ym = t(NB, k, h, w, dtype=dt), t(NB, m, h, w, dtype=dt)       # K-channel operand, M-channel residual / dy of the wgrad
        wf, wd = t(m, k, 1, 1), t(k, m, 1, 1)                           # forward weight; the (Cout = K, Cin = M) weight of the dgrad
        bias, dw = t(m), t(m, k, 1, 1)
        st = ops.BnStats(k, dev)                                        # prologue on the K-channel operand
        stm = ops.BnStats(m, dev)                                       # BatchNorm in front of the convolution M -> K (bnred / bndx)
        for s in (st, stm):
            s.scale.fill_(1.0), s.shift.zero_(), s.mean.zero_(), s.invstd.fill_(1.0)
        todo = {}
        if not bf16:
            todo = {"plain": lambda: ops.conv1x1_fwd(x, wf), "stats": lambda: ops.conv1x1_fwd_stats(x, wf),
                    "pro": lambda: ops.conv1x1_fwd_bnact(x, st, wf), "pro_stats": lambda: ops.conv1x1_fwd_bnact(x, st, wf, stats=True),
                    "res": lambda: ops.conv1x1_fwd(x, wf, None, ym), "bias": lambda: ops.conv1x1_fwd(x, wf, bias),
                    "bres": lambda: ops.conv1x1_fwd(x, wf, None, ym[0], True), "dgrad": lambda: ops.conv1x1_bwd_data(x, wd)}
            if ops.c1r_bnred_supported(m, k, hw):
                xm, gamma = t(NB, m, h, w), t(m)
                ws_rows = {}

                def bnred_nostore():
                    ws_rows["sr"] = ops.c1r_bnred(wd, x, xm, stm, store=False)[1]

                def bndx():       # (the coefficients at the head of the workspace come from bn_act_bwd_from_rows, not recorded)
                    ops.bn_act_bwd_from_rows(ws_rows["sr"], m, t(m), t(m))
                    with Recorder() as ln:
                        ops.c1r_bndx(wd, x, xm, gamma, stm, ym, True)
                    return ln
                todo.update({"bnred": lambda: ops.c1r_bnred(wd, x, xm, stm), "bnred_nostore": bnred_nostore, "bndx": bndx})
        else:
            planes = {}

            def fwd(form, pro, res, stats):
                fam = _bf16_family(ops, m, k, hw, form)
                if fam == "c1rb":
                    return ops.c1rb_fwd(wf, False, x, pro, res, stats)
                if fam == "c1b":
                    return ops.c1b_fwd(planes["f"][0], x, pro, res, stats)
                if pro is not None:
                    return ops.conv1x1_fwd_bnact(x, pro, wf, None, res, stats)
                return ops.conv1x1_fwd_stats(x, wf, None, res) if stats else ops.conv1x1_fwd(x, wf, bias if form == "bias" else None, res)

            def dgrad():
                fam = _bf16_family(ops, m, k, hw, "dgrad")
                if fam == "c1rb":
                    return ops.c1rb_fwd(wd, True, x, label="wfae_c1b_dgrad")
                if fam == "c1b":
                    return ops.c1b_fwd(ops.c1b_weights(wd)[1], x, label="wfae_c1b_dgrad")
                return ops.conv1x1_bwd_data(x, wd)

            def c1b_weights():
                planes["f"] = ops.c1b_weights(wf)
            todo = {"c1b_weights": c1b_weights, "plain": lambda: fwd("plain", None, None, False),
                    "stats": lambda: fwd("stats", None, None, True), "pro": lambda: fwd("pro", st, None, False),
                    "pro_stats": lambda: fwd("pro_stats", st, None, True), "res": lambda: fwd("res", None, ym, False),
                    "bias": lambda: fwd("bias", None, None, False), "dgrad": dgrad}
        todo.update({"wgrad": lambda: ops.conv1x1_bwd_weight(ym, x, dw), "wgrad_acc": lambda: ops.conv1x1_bwd_weight(ym, x, dw, True),
                     "wgrad_pro": lambda: ops.conv1x1_bwd_weight_bnact(ym, x, st, dw),
                     "wgrad_pro_acc": lambda: ops.conv1x1_bwd_weight_bnact(ym, x, st, dw, True)})
        for form in (FORMS_BF16 if bf16 else FORMS_F32):
            if form not in todo:
                continue
            with Recorder() as ln:
                inner = todo[form]()
            ln = inner if form == "bndx" else ln
            if form == "dgrad" and bf16:
                ln = [l for l in ln if not l.startswith("wfae_c1b_weights")]     # (its plane is made on the spot)
            assert len(ln) == 1, (form, ln)
            forms.append(form)
            lines += ln
        torch.cuda.synchronize()
    return forms, lines


# ----------------------------------------------------------------- whole blocks
def block_case_ids():
    for cfg in CONFIGS:
        for c in BLOCK_C:
            for train in (True, False):
                for emit in (False, True):
                    yield f"block/{cfg}/-/C{c}/{'train' if train else 'eval'}/{'emit' if emit else 'noemit'}", cfg, None, c, train, emit
    for switch in BLOCK_SWITCHES:
        for c in (128, 256):
            yield f"block/highest_split/{switch}/C{c}/train/noemit", "highest_split", switch, c, True, False


def run_block(dev, cfg, switch, c, train, emit):
    """BottleneckFn forward + backward on the model's Bottleneck module -> [canonical lines] of every launch it makes"""
    import torch
    from weatherforecastingtoolkit_amd import functional as Fn, ops
    from weatherforecastingtoolkit_amd.pipeline.models.ae_64x8x8_lin import Bottleneck
    torch.manual_seed(0)
    blk = Bottleneck(c).to(dev)
    blk.train(train)
    blk.emit_stats = emit
    with configured(cfg, switch):
        x = torch.full((NB, c, 8, 16), 0.25, device=dev)
        x = ops.to_dtype(x, ops.activation_dtype()).requires_grad_(True)
        with Recorder() as lines:
            y = blk(x)
            y.backward(torch.full_like(y, 0.5))
            Fn.join_side_stream()
        torch.cuda.synchronize()
    return lines


def record_all(dev):
    out = {"single": {}, "block": {}}
    for cid, cfg, switch, m, k, h, w in single_case_ids():
        forms, lines = run_single(dev, cfg, switch, m, k, h, w)
        out["single"][cid] = dict(forms=forms, **digest(lines))
    for cid, *args in block_case_ids():
        out["block"][cid] = digest(run_block(dev, *args))
    return out


if __name__ == "__main__":
    import torch
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    rec = record_all(torch.device("cuda:0"))
    with open(path, "w") as f:      # one case per line
        kinds = [f'"{kind}": {{\n' + ",\n".join(f"{json.dumps(cid)}: {json.dumps(rec[kind][cid], sort_keys=True)}" for cid in sorted(rec[kind]))
                 + "\n}" for kind in sorted(rec)]
        f.write("{\n" + ",\n".join(kinds) + "\n}\n")
    print(f"{len(rec['single'])} single-product cases, {len(rec['block'])} block cases -> {path}")
