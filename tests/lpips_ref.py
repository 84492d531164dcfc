"""Plain-torch restatement of the reference's LPIPS (pipeline/models/autoencoderkl/losses/lpips.py) for the tests: runs on
the CPU in fp64 or fp32, from a state dict with the reference's keys.

    lpips.py:63-70    ScalingLayer            -> scaling()
    lpips.py:107-120  vgg16.forward           -> features()   (torchvision vgg16().features[0:30]: conv3x3 + ReLU, 'M')
    lpips.py:123-125  normalize_tensor        -> normalize()
    lpips.py:128-129  spatial_average         -> .mean([2, 3], keepdim=True)
    lpips.py:47-60    LPIPS.forward           -> lpips()
    experiments/ae_v2_2/train.py:57-58        -> a 1-channel image is repeat(1, 3, 1, 1)

`acts=`: the 13 post-ReLU activations of the FIRST image as another implementation computed them.  The forward values
are still the restatement's own; the two non-smooth derivatives — ReLU'(pre) and the max-pool's routing — are taken
from the supplied activations ((a > 0), first maximum of a window in the order (0,0), (0,1), (1,0), (1,1)), so that two
implementations whose pre-activations differ by rounding are compared on the same branch of every kink."""
import torch
import torch.nn.functional as F

CONVS = [(0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256),
         (17, 256, 512), (19, 512, 512), (21, 512, 512), (24, 512, 512), (26, 512, 512), (28, 512, 512)]
SLICES = (2, 2, 3, 3, 3)
SLICE_OF = [1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5]
CHNS = [64, 128, 256, 512, 512]


def conv_keys():
    return [f"net.slice{s}.{i}" for (i, _, _), s in zip(CONVS, SLICE_OF)]


def state_dict_items():
    """(key, shape) of the reference's LPIPS().state_dict(), in its order"""
    items = [("scaling_layer.shift", (1, 3, 1, 1)), ("scaling_layer.scale", (1, 3, 1, 1))]
    for k, (_, ci, co) in zip(conv_keys(), CONVS):
        items += [(k + ".weight", (co, ci, 3, 3)), (k + ".bias", (co,))]
    items += [(f"lin{k}.model.1.weight", (1, c, 1, 1)) for k, c in enumerate(CHNS)]
    return items


def weights(seed):
    """seeded fp32 state dict: He-normal convolutions, 0.1-normal biases, uniform linear layers (drawn in fp64)"""
    g = torch.Generator().manual_seed(seed)
    sd = {"scaling_layer.shift": torch.tensor([-.030, -.088, -.188])[None, :, None, None],
          "scaling_layer.scale": torch.tensor([.458, .448, .450])[None, :, None, None]}
    for k, (_, ci, co) in zip(conv_keys(), CONVS):
        sd[k + ".weight"] = (torch.randn(co, ci, 3, 3, generator=g, dtype=torch.float64) * (2.0 / (9 * ci)) ** 0.5).float()
        sd[k + ".bias"] = (torch.randn(co, generator=g, dtype=torch.float64) * 0.1).float()
    for k, c in enumerate(CHNS):
        sd[f"lin{k}.model.1.weight"] = torch.rand(c, generator=g, dtype=torch.float64).float().view(1, c, 1, 1)
    return sd


def inputs(shape, seed):
    """(x, target) fp32 in [0, 1]: a target and a noisy copy of it"""
    g = torch.Generator().manual_seed(100 + seed)
    t = torch.rand(shape, generator=g, dtype=torch.float64)
    x = (t + 0.2 * torch.randn(shape, generator=g, dtype=torch.float64)).clamp(0, 1)
    return x.float(), t.float()


class _ReluAs(torch.autograd.Function):
    """relu(pre) with the derivative (a > 0) of a supplied activation"""

    @staticmethod
    def forward(ctx, pre, a):
        ctx.save_for_backward(a > 0)
        return pre.clamp_min(0)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0].to(g.dtype), None


def first_max_onehot(a):
    """(N, C, Ho, Wo, 4) one-hot of the first maximum of every 2 x 2 window of a, window order (0,0), (0,1), (1,0), (1,1)"""
    n, c, h, w = a.shape
    ho, wo = h // 2, w // 2
    win = a[:, :, :2 * ho, :2 * wo].reshape(n, c, ho, 2, wo, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, ho, wo, 4)
    return F.one_hot(win.argmax(-1), 4)      # argmax returns the first of several maxima


class _PoolAs(torch.autograd.Function):
    """max_pool2d(x, 2) with the gradient routed to the first maximum of a supplied activation's windows"""

    @staticmethod
    def forward(ctx, x, a):
        ctx.save_for_backward(first_max_onehot(a))
        ctx.shape = x.shape
        return F.max_pool2d(x, 2)

    @staticmethod
    def backward(ctx, g):
        n, c, h, w = ctx.shape
        ho, wo = h // 2, w // 2
        r = g[..., None] * ctx.saved_tensors[0].to(g.dtype)                     # (n, c, ho, wo, 4)
        r = r.reshape(n, c, ho, wo, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, 2 * ho, 2 * wo)
        return F.pad(r, (0, w - 2 * wo, 0, h - 2 * ho)), None


def scaling(sd, x, dtype):
    """lpips.py:63-70 (after train.py:57-58 for a 1-channel image)"""
    x = x.to(dtype)
    if x.shape[1] == 1:
        x = x.repeat(1, 3, 1, 1)
    return (x - sd["scaling_layer.shift"].to(dtype)) / sd["scaling_layer.scale"].to(dtype)


def _bf16(t):
    return t.float().bfloat16().to(t.dtype)


def features(sd, h, dtype, acts=None, bf16_ops=False):
    """lpips.py:107-120 -> (five taps, the 13 post-ReLU activations)"""
    taps, all_acts, li = [], [], 0
    for s, nconv in enumerate(SLICES):
        if s:
            h = F.max_pool2d(h, 2) if acts is None else _PoolAs.apply(h, acts[li - 1].to(dtype))
        for _ in range(nconv):
            k = conv_keys()[li]
            w, b = sd[k + ".weight"].to(dtype), sd[k + ".bias"].to(dtype)
            pre = F.conv2d(_bf16(h), _bf16(w), b, padding=1) if bf16_ops else F.conv2d(h, w, b, padding=1)
            h = F.relu(pre) if acts is None else _ReluAs.apply(pre, acts[li].to(dtype))
            all_acts.append(h)
            li += 1
        taps.append(h)
    return taps, all_acts


def normalize(x, eps=1e-10):
    """lpips.py:123-125"""
    return x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + eps)


def lpips(sd, x, target, dtype=torch.float64, acts=None, bf16_ops=False):
    """lpips.py:47-60 -> (value (N, 1, 1, 1), the 13 activations of x, the five taps of the target)"""
    t0, a0 = features(sd, scaling(sd, x, dtype), dtype, acts, bf16_ops)
    with torch.no_grad():
        t1, _ = features(sd, scaling(sd, target, dtype), dtype, None, bf16_ops)
    val = None
    for kk in range(5):
        diff = (normalize(t0[kk]) - normalize(t1[kk])) ** 2
        res = F.conv2d(diff, sd[f"lin{kk}.model.1.weight"].to(dtype)).mean([2, 3], keepdim=True)
        val = res if val is None else val + res
    return val, a0, t1


def value_and_grad(sd, x, target, dtype=torch.float64, acts=None, g=None):
    """-> (value, d sum(g * value) / d x, activations of x, taps of the target), all detached"""
    xr = x.to(dtype).clone().requires_grad_(True)
    val, a0, t1 = lpips(sd, xr, target, dtype, acts)
    g = torch.ones_like(val) if g is None else g.to(dtype).view_as(val)
    (dx,) = torch.autograd.grad((val * g).sum(), xr)
    return val.detach(), dx, [a.detach() for a in a0], t1


def spread(a32, a64):
    """max |a32 - a64| / max |a64|: the measure of every bound"""
    a32, a64 = a32.double(), a64.double()
    return float((a32 - a64).abs().max() / a64.abs().max().clamp_min(1e-300))
