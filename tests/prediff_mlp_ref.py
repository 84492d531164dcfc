"""Torch restatement of the intensity-statistics MLP forecaster of the reference's v1 experiments
(experiments/v1_experiments/prediff_mlp_sevir/train.py:20-38, 56-70), written from the formulas.  Any device / dtype;
used against tests/golden/g16_prediff_mlp.npz on the CPU and as the fp64 yardstick of the GPU tests.

Batch: 'NHWT' (B, H, W, T).  Input: the mean of each of the first t_in frames.  Target: the remaining P = T - t_in
frames, frame-major, cut into `groups` runs of P H W / groups consecutive elements; the run means, then the run
standard deviations with the n - 1 divisor."""
import torch

KEYS = ("mlp.0.weight", "mlp.0.bias", "mlp.2.weight", "mlp.2.bias", "mlp.4.weight", "mlp.4.bias")
T_IN, GROUPS = 5, 4


def statistics(batch, t_in=T_IN, groups=GROUPS):
    """-> (x (B, t_in), target (B, 2 groups)) in batch's dtype"""
    b, h, w, t = batch.shape
    frames = batch.permute(0, 3, 1, 2).reshape(b, t, h * w)
    x = frames[:, :t_in].sum(dim=2) / (h * w)
    runs = frames[:, t_in:].reshape(b, groups, -1)
    n = runs.shape[2]
    mean = runs.sum(dim=2) / n
    dev = runs - mean[:, :, None]
    std = ((dev * dev).sum(dim=2) / (n - 1)).sqrt()
    return x, torch.cat([mean, std], dim=1)


def mlp(x, params):
    w1, b1, w2, b2, w3, b3 = params
    h1 = (x @ w1.t() + b1).clamp_min(0)
    h2 = (h1 @ w2.t() + b2).clamp_min(0)
    return h2 @ w3.t() + b3


def loss_and_pred(x, target, params):
    pred = mlp(x, params)
    d = pred - target
    return (d * d).sum() / d.numel(), pred


def step_loss(batch, params, t_in=T_IN, groups=GROUPS):
    """-> (loss, pred, x, target): the whole training-step forward"""
    x, target = statistics(batch, t_in, groups)
    loss, pred = loss_and_pred(x, target, params)
    return loss, pred, x, target


def rel_err(got, want):
    """largest |got - want| / |want| over the elements (the statistics' bar)"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float(((got - want).abs() / want.abs().clamp_min(1e-300)).max())
