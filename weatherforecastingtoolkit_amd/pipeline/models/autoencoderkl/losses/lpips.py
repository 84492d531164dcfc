"""LPIPS perceptual loss (reference pipeline/models/autoencoderkl/losses/lpips.py) on csrc/lpips.hip.

The torch classes are parameter containers with the reference's names, constructor signatures and state_dict keys
(`scaling_layer.shift/scale`, `net.slice1.0.weight` ... `net.slice5.28.bias`, `lin0.model.1.weight` ...
`lin4.model.1.weight`), so a saved reference `LPIPS` state dict loads with strict=True.  What differs:
  * nothing is fetched and torchvision is not needed: `LPIPS()` builds seeded-random parameters, `LPIPS.from_files`
    loads a torchvision VGG16 state dict and the `vgg.pth` linear layers from two files the user supplies;
  * everything is frozen, and the module stays in eval mode (`train()` does not switch it): the reference's `Loss` builds
    `LPIPS().eval()`, and the Dropout in front of the linear layers is not built;
  * forward + backward are one autograd Function (functional.LpipsFn); the gradient flows to `input` only;
  * at a pixel whose features are zero in every channel the reference's gradient is NaN, here it is finite (include/wfae.h).
"""
from __future__ import annotations

from collections import namedtuple
from types import SimpleNamespace

import torch
import torch.nn as tnn

from ..... import functional as Fn
from ..... import ops
from ....._lib import WfaeError

# torchvision vgg16().features: index -> (Cin, Cout) of the 3x3 convolutions; ReLU follows each; 'M' at 4, 9, 16, 23
VGG16_CONVS = {0: (3, 64), 2: (64, 64), 5: (64, 128), 7: (128, 128), 10: (128, 256), 12: (256, 256), 14: (256, 256),
               17: (256, 512), 19: (512, 512), 21: (512, 512), 24: (512, 512), 26: (512, 512), 28: (512, 512)}
VGG16_POOLS = (4, 9, 16, 23)
SLICE_RANGES = ((0, 4), (4, 9), (9, 16), (16, 23), (23, 30))
VggOutputs = namedtuple("VggOutputs", ["relu1_2", "relu2_2", "relu3_3", "relu4_3", "relu5_3"])


def _forward_only(what, *ts):
    if torch.is_grad_enabled() and any(t.requires_grad for t in ts):
        raise WfaeError(f"{what} is forward only: gradients come from LPIPS.forward (functional.LpipsFn)")


class ScalingLayer(tnn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.Tensor([-.030, -.088, -.188])[None, :, None, None])
        self.register_buffer("scale", torch.Tensor([.458, .448, .450])[None, :, None, None])

    def forward(self, inp):
        """(inp - shift) / scale; a 1-channel image is read as its repeat(1, 3, 1, 1)"""
        _forward_only("ScalingLayer", inp)
        return ops.lpips_prep_fwd(Fn._c(inp.detach()), self.shift, self.scale)


class NetLinLayer(tnn.Module):
    """ A single linear layer which does a 1x1 conv """

    def __init__(self, chn_in, chn_out=1, use_dropout=False):
        super().__init__()
        if chn_out != 1:
            raise WfaeError("NetLinLayer: chn_out = 1 is built (the LPIPS distance)")
        layers = [tnn.Dropout(), ] if use_dropout else []
        layers += [tnn.Conv2d(chn_in, chn_out, 1, stride=1, padding=0, bias=False), ]
        self.model = _Container(*layers)


class _Container(tnn.Sequential):
    """keeps the reference's module tree (and with it the state_dict keys); the arithmetic runs in the HIP kernels"""

    def forward(self, *a, **k):
        raise WfaeError("this container holds parameters only: run vgg16 / LPIPS")


class vgg16(tnn.Module):
    """VGG16 features in the reference's five slices.  weights: None (torch's default initialisation; LPIPS overwrites
    it with its seeded values) — nothing is fetched."""

    def __init__(self, requires_grad=False, weights=None):
        super().__init__()
        if weights is not None:
            raise WfaeError("vgg16: pretrained weights are not fetched; load them with LPIPS.from_files / load_state_dict")
        if requires_grad:
            raise WfaeError("vgg16: the network is frozen (there are no weight-gradient kernels)")
        self.N_slices = 5
        for k, (lo, hi) in enumerate(SLICE_RANGES):
            sl = _Container()
            for x in range(lo, hi):
                if x in VGG16_CONVS:
                    m = tnn.Conv2d(*VGG16_CONVS[x], kernel_size=3, padding=1)
                elif x in VGG16_POOLS:
                    m = tnn.MaxPool2d(kernel_size=2, stride=2)
                else:
                    m = tnn.ReLU(inplace=True)
                sl.add_module(str(x), m)
            setattr(self, f"slice{k + 1}", sl)
        for param in self.parameters():
            param.requires_grad = False

    def convs(self):
        """the 13 convolutions in order"""
        return [m for k in range(5) for m in getattr(self, f"slice{k + 1}") if isinstance(m, tnn.Conv2d)]

    def forward(self, X):
        """the five tap activations of X (N, 3, H, W), forward only"""
        _forward_only("vgg16", X)
        h, mode, outs, convs = Fn._c(X.detach()), ops.aekl_mode(), [], iter(self.convs())
        for s, nconv in enumerate(Fn.LPIPS_SLICES):
            if s:
                h = ops.lpips_pool_fwd(h)
            for _ in range(nconv):
                c = next(convs)
                h = ops.lpips_conv3_fwd(h, ops.aekl_conv3_pack(c.weight.detach().contiguous(), mode), c.bias.detach(), mode)
            outs.append(h)
        return VggOutputs(*outs)


class LPIPS(tnn.Module):
    # Learned perceptual metric
    def __init__(self, use_dropout=True, *, weights=None, seed=0):
        super().__init__()
        if weights is not None:
            raise WfaeError("LPIPS: pretrained weights are not fetched; use LPIPS.from_files(vgg_features, lin)")
        self.scaling_layer = ScalingLayer()
        self.chns = [64, 128, 256, 512, 512]  # vg16 features
        with torch.random.fork_rng(devices=[]):   # torch's default initialisation draws from the global generator
            self.net = vgg16(requires_grad=False, weights=None)
            for k, c in enumerate(self.chns):
                setattr(self, f"lin{k}", NetLinLayer(c, use_dropout=use_dropout))
        # seeded-random parameters from a generator of their own (the caller's stays untouched): He-normal convolutions,
        # small biases, non-negative linear layers like the trained ones
        g = torch.Generator().manual_seed(int(seed))
        with torch.no_grad():
            for c in self.net.convs():
                c.weight.copy_(torch.randn(c.weight.shape, generator=g) * (2.0 / (9 * c.in_channels)) ** 0.5)
                c.bias.copy_(torch.randn(c.bias.shape, generator=g) * 0.1)
            for lin in self.lins():
                lin.weight.copy_(torch.rand(lin.weight.shape, generator=g))
        for param in self.parameters():
            param.requires_grad = False
        self._cache = None
        super().train(False)

    def lins(self):
        return [getattr(self, f"lin{k}").model[-1] for k in range(5)]

    def train(self, mode=True):
        """stays in eval mode (the reference's `LPIPS().eval()`; the Dropout of the linear layers is not built)"""
        return super().train(False)

    @classmethod
    def from_files(cls, vgg_features, lin, use_dropout=True):
        """vgg_features: a torchvision VGG16 state dict file (`features.N.weight / bias`; classifier keys are ignored; the
        bare `N.weight` keys of `vgg16().features.state_dict()` are accepted too).  lin: the LPIPS `vgg.pth` file
        (`linK.model.1.weight`)."""
        model = cls(use_dropout=use_dropout)
        vsd = torch.load(vgg_features, map_location="cpu", weights_only=True)
        lsd = torch.load(lin, map_location="cpu", weights_only=True)
        sd = {k: v for k, v in model.state_dict().items() if k.startswith("scaling_layer.")}
        sd.update(map_vgg_features(vsd))
        for k, v in lsd.items():
            if k.startswith("lin"):
                sd[k] = v
        model.load_state_dict(sd, strict=True)
        return model

    def _state(self):
        """the frozen operands of functional.LpipsFn: packed once, again when a parameter is written (load_state_dict),
        moved, or the matmul precision changes the conv mode"""
        mode, convs, lins = ops.aekl_mode(), self.net.convs(), self.lins()
        sc = self.scaling_layer
        key = (mode,) + tuple((p.device, p.data_ptr(), p._version) for p in
                              [c.weight for c in convs] + [c.bias for c in convs] + [m.weight for m in lins] + [sc.shift, sc.scale])
        if self._cache is None or self._cache[0] != key:
            ws = [c.weight.detach().contiguous() for c in convs]
            st = SimpleNamespace(
                mode=mode, shift=sc.shift.detach().reshape(3).contiguous(), scale=sc.scale.detach().reshape(3).contiguous(),
                fwd=[ops.aekl_conv3_pack(w, mode) for w in ws],
                bwd=[ops.aekl_conv3_pack(w.flip(2, 3).transpose(0, 1).contiguous(), mode) for w in ws],
                bias=[c.bias.detach().contiguous() for c in convs], cin=[c.in_channels for c in convs],
                lin=[m.weight.detach().reshape(-1).contiguous() for m in lins])
            self._cache = (key, st)
        return self._cache[1]

    def forward(self, input, target, *, return_activations=False):
        """-> (N, 1, 1, 1); with return_activations also the recon half's 13 post-ReLU activations (what backward reads)"""
        if target.requires_grad:
            raise WfaeError("LPIPS: the gradient flows to `input` only; detach the target")
        if input.dim() != 4 or input.shape != target.shape or input.shape[1] not in (1, 3):
            raise WfaeError(f"LPIPS: expected two (N, 1 or 3, H, W) images, got {tuple(input.shape)} and {tuple(target.shape)}")
        if min(input.shape[2:]) < 16:
            raise WfaeError(f"LPIPS: images of at least 16 x 16 (four 2 x 2 pools), got {tuple(input.shape[2:])}")
        sink = [] if return_activations else None
        val = Fn.LpipsFn.apply(input, target, self._state(), sink)
        return (val, sink) if return_activations else val


def map_vgg_features(vsd):
    """torchvision `features.N.*` (or bare `N.*`) -> `net.sliceK.N.*`; other keys (the classifier) are dropped"""
    out = {}
    for k, v in vsd.items():
        parts = k.split(".")
        if parts[0] == "features":
            parts = parts[1:]
        if len(parts) != 2 or not parts[0].isdigit() or int(parts[0]) not in VGG16_CONVS:
            continue
        idx = int(parts[0])
        sl = next(i for i, (lo, hi) in enumerate(SLICE_RANGES) if lo <= idx < hi)
        out[f"net.slice{sl + 1}.{idx}.{parts[1]}"] = v
    return out
