"""GPU: the kernels of the intensity-statistics MLP forecaster (csrc/prediff.hip) and the prediff_mlp_sevir experiment.

Statistics: every case runs in both memory orders the loader can deliver — `frames` (a permuted view of a contiguous
(B, T, H, W) tensor) and `tinner` (a contiguous (B, H, W, T) tensor) — and is compared with the fp64 restatement
tests/prediff_mlp_ref.py on the same fp32 input: relative error <= 1e-5 on every mean and every std.  (The reference's
fp32 CPU result sits at 1e-7 / 5e-8 on these inputs, a chunked Chan / two-pass algorithm around 1e-6, E[x^2] - E[x]^2
in fp32 at 1.0 on the offset case.)  Measured maxima over all cases: see DESIGN.md "Intensity-statistics MLP".

Fused MLP: the project's standing parity bars against tests/golden/g16_prediff_mlp.npz — pred <= 1e-4, loss <= 1e-5,
each gradient <= 5e-4 of its norm, post-step parameters <= 5e-4."""
import os

import numpy as np
import pytest
import torch

from tests import prediff_mlp_ref as R
from weatherforecastingtoolkit_amd import config as C
from weatherforecastingtoolkit_amd import functional as Fn
from weatherforecastingtoolkit_amd import ops
from weatherforecastingtoolkit_amd.experiments.v1_experiments import _prediff_mlp as M
from weatherforecastingtoolkit_amd.pipeline.datasets.sevire.sevir import change_layout_torch

pytestmark = pytest.mark.gpu

G16 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g16_prediff_mlp.npz")
CONFIG = os.path.join(os.path.dirname(M.__file__), "prediff_mlp_sevir", "config.yaml")
STAT_BAR = 1e-5
ORDERS = ("frames", "tinner")


@pytest.fixture(scope="module")
def g16():
    return np.load(G16, allow_pickle=False)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def rel_norm(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def deliver(nhwt_cpu, order, dev, offset=0):
    """the 'NHWT' batch on the device in one of the two memory orders; offset: floats the storage starts past a
    16-byte boundary"""
    src = nhwt_cpu.permute(0, 3, 1, 2).contiguous() if order == "frames" else nhwt_cpu.contiguous()
    flat = torch.empty(src.numel() + 4, dtype=torch.float32, device=dev)
    assert flat.data_ptr() % 16 == 0
    store = flat[offset:offset + src.numel()].view(src.shape)
    store.copy_(src)
    out = store.permute(0, 2, 3, 1) if order == "frames" else store
    assert out.shape == nhwt_cpu.shape and out.is_contiguous() == (order == "tinner")
    return out


def check_stats(nhwt_cpu, dev, what, t_in=5, groups=4, offset=0):
    x64, t64 = R.statistics(nhwt_cpu.double(), t_in, groups)
    worst = 0.0
    for order in ORDERS:
        batch = deliver(nhwt_cpu, order, dev, offset)
        x, target = ops.seq_intensity_stats(batch, t_in, groups)
        assert x.shape == x64.shape and target.shape == t64.shape
        g = groups
        ex, em, es = R.rel_err(x, x64), R.rel_err(target[:, :g], t64[:, :g]), R.rel_err(target[:, g:], t64[:, g:])
        print(f"{what} [{order}, offset {offset}]: rel err frame means {ex:.2e}, group means {em:.2e}, group stds {es:.2e}")
        assert ex <= STAT_BAR and em <= STAT_BAR and es <= STAT_BAR, (what, order, ex, em, es)
        worst = max(worst, ex, em, es)
    return worst


def uniform(shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


def test_stats_golden(dev, g16):
    batch = torch.from_numpy(g16["batch"])
    check_stats(batch, dev, "golden")
    for order in ORDERS:
        x, target = ops.seq_intensity_stats(deliver(batch, order, dev), 5)
        assert R.rel_err(x, torch.from_numpy(g16["x"])) <= STAT_BAR
        assert R.rel_err(target, torch.from_numpy(g16["target"])) <= STAT_BAR


@pytest.mark.parametrize("offset", [0, 1, 3])
def test_stats_unaligned_frames(dev, offset):
    # H W = 399: no frame but the first starts on a 16-byte boundary, every frame ends inside a quad
    check_stats(uniform((3, 21, 19, 25), 1), dev, "unaligned 21x19", offset=offset)


def test_stats_multi_chunk(dev):
    # frames order: a workgroup reduces one 8192-float window of a frame; H W = 160 * 157 = 25120 = 3 * 8192 + 544, so
    # every frame spans three whole windows plus a ragged tail (four or five partials, frames start mid-window).
    # tinner order: a workgroup reduces 16 rows of 1024 floats, 25 workgroups share a tile of 409600 floats; a sample
    # (628000 floats) is one whole tile plus a ragged one, 50 partials per frame.
    check_stats(uniform((2, 160, 157, 25), 2), dev, "multi-chunk 160x157", offset=2)


def test_stats_full_size(dev):
    check_stats(uniform((1, 384, 384, 25), 3), dev, "full size 384x384")


def test_stats_offset_field(dev):
    # cancellation: E[x^2] - E[x]^2 in fp32 loses every digit of this std
    check_stats(0.9 + 1e-3 * uniform((2, 96, 100, 25), 4), dev, "offset 0.9 + 1e-3 U")
    check_stats(0.9 + 1e-3 * uniform((1, 384, 384, 25), 5), dev, "offset, full size")


def test_stats_sparse_field(dev):
    v = uniform((2, 96, 100, 25), 6)
    v = torch.where(uniform((2, 96, 100, 25), 7) < 0.7, torch.zeros(()), v)
    assert float((v == 0).float().mean()) > 0.65
    check_stats(v, dev, "sparse 70 % zeros")


def test_stats_other_splits(dev):
    # 7 input frames, 16 target frames in 4 and in 2 groups; groups of one frame
    check_stats(uniform((2, 33, 31, 23), 8), dev, "t_in 7 of 23", t_in=7, groups=4)
    check_stats(uniform((2, 33, 31, 23), 8), dev, "t_in 7 of 23, 2 groups", t_in=7, groups=2)
    check_stats(uniform((1, 8, 9, 9), 9), dev, "t_in 1 of 9, 8 groups", t_in=1, groups=8)


def test_stats_refusals(dev):
    batch = torch.rand(2, 16, 16, 23, device=dev)
    with pytest.raises(ops._lib.WfaeError, match="pred_frames = 18"):
        ops.seq_intensity_stats(batch, 5)
    with pytest.raises(ops._lib.WfaeError, match="does not copy"):
        ops.seq_intensity_stats(torch.rand(2, 16, 25, 16, device=dev).permute(0, 1, 3, 2), 5)
    with pytest.raises(ops._lib.WfaeError, match="fp32"):
        ops.seq_intensity_stats(torch.rand(2, 16, 16, 25, device=dev).half(), 5)


def test_stats_bitwise_repeatable(dev):
    v = uniform((2, 160, 157, 25), 10)
    for order in ORDERS:
        batch = deliver(v, order, dev, offset=1)
        a = ops.seq_intensity_stats(batch, 5)
        b = ops.seq_intensity_stats(batch, 5)
        torch.cuda.synchronize()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def golden_mlp(g16, dev):
    m = M.MLP().to(dev)
    for i, p in enumerate(m.parameters_in_order()):
        p.data.copy_(torch.from_numpy(g16[f"init_{i}"]))
    return m


def test_mlp_golden_parity(dev, g16):
    m = golden_mlp(g16, dev)
    x, target = torch.from_numpy(g16["x"]).to(dev), torch.from_numpy(g16["target"]).to(dev)
    loss, pred = m.loss(x, target)
    e_pred, e_loss = rel(pred, torch.from_numpy(g16["pred"])), abs(loss.item() - float(g16["loss"])) / float(g16["loss"])
    print(f"mlp golden: pred {e_pred:.2e} loss {e_loss:.2e}")
    assert e_pred <= 1e-4 and e_loss <= 1e-5
    assert not pred.requires_grad
    loss.backward()
    for i, p in enumerate(m.parameters_in_order()):
        e = rel_norm(p.grad, torch.from_numpy(g16[f"grad_{i}"]))
        print(f"mlp golden: grad {R.KEYS[i]} {e:.2e}")
        assert e <= 5e-4, (R.KEYS[i], e)
    # the forward-only flag: the same pred bits, through the module and through validation's pred + loss form
    assert torch.equal(m(x), pred)
    p2, l2 = ops.mlp3_mse(x, target, *[p.detach() for p in m.parameters_in_order()])
    assert torch.equal(p2, pred) and torch.equal(l2, loss.detach())
    # an upstream factor scales every gradient
    m.zero_grad(set_to_none=True)
    (3.0 * m.loss(x, target)[0]).backward()
    for i, p in enumerate(m.parameters_in_order()):
        assert rel_norm(p.grad, 3.0 * torch.from_numpy(g16[f"grad_{i}"])) <= 5e-4


@pytest.mark.parametrize("B,dims", [(1, (5, 8, 128)), (64, (5, 8, 128)), (5, (7, 6, 96)), (64, (32, 32, 256))])
def test_mlp_against_fp64(dev, B, dims):
    torch.manual_seed(B + dims[2])
    m = M.MLP(*dims).to(dev)
    g = torch.Generator().manual_seed(17 + B)
    x, target = torch.rand(B, dims[0], generator=g).to(dev), torch.rand(B, dims[1], generator=g).to(dev)
    loss, pred = m.loss(x, target)
    loss.backward()
    p64 = [p.detach().double().cpu().requires_grad_(True) for p in m.parameters_in_order()]
    l64, pr64 = R.loss_and_pred(x.double().cpu(), target.double().cpu(), p64)
    l64.backward()
    assert rel(pred, pr64) <= 1e-4
    assert abs(loss.item() - l64.item()) <= 1e-5 * abs(l64.item())
    for p, q, k in zip(m.parameters_in_order(), p64, R.KEYS):
        assert rel_norm(p.grad, q.grad) <= 5e-4, k
    assert torch.equal(m(x), pred)


def test_mlp_bitwise_repeatable_and_limits(dev):
    torch.manual_seed(0)
    m = M.MLP().to(dev)
    x, target = torch.rand(64, 5, device=dev), torch.rand(64, 8, device=dev)
    params = [p.detach() for p in m.parameters_in_order()]
    outs = []
    for _ in range(2):
        grads = [torch.empty_like(p) for p in params]
        pred, loss = ops.mlp3_mse(x, target, *params, grads=grads)
        outs.append([pred, loss] + grads)
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    with pytest.raises(ops._lib.WfaeError, match="hidden=512"):
        M.MLP(5, 8, 512).to(dev)(x)
    with pytest.raises(ops._lib.WfaeError, match="B=65"):
        m(torch.rand(65, 5, device=dev))
    with pytest.raises(ops._lib.WfaeError, match="no gradient with respect to x"):
        m.loss(x.clone().requires_grad_(True), target)


def train_cfg(steps=3):
    cfg = C.load(CONFIG)
    cfg.trainer.total_train_steps = steps
    cfg.cosine_warmup.update(start_lr=1e-3, peak_lr=1e-3, final_lr=1e-3)   # the recorded steps use a constant 1e-3
    return cfg


def golden_model(g16, dev):
    model = M.Model(train_cfg()).to(dev).train()
    model.load_state_dict({"model." + str(k): torch.from_numpy(g16[f"init_{i}"]) for i, k in enumerate(g16["keys"])})
    return model


def test_training_steps_land_on_golden(dev, g16):
    model = golden_model(g16, dev)
    model.configure_optimizers()
    nthw = torch.from_numpy(g16["batch"]).permute(0, 3, 1, 2).contiguous().to(dev)
    batch = change_layout_torch(nthw, "NTHW", "NHWT")
    assert not batch.is_contiguous() and batch.shape == (2, 16, 16, 25)
    for s in range(3):
        assert model.opt.param_groups[0]["lr"] == pytest.approx(1e-3, rel=1e-9)
        loss, gn = model.training_step(batch, s)
        if s == 0:
            assert abs(loss.item() - float(g16["loss"])) <= 1e-5 * float(g16["loss"])
        assert abs(gn.item() - float(g16["gnorm"][s])) <= 5e-4 * float(g16["gnorm"][s]), (s, gn.item())
    for i, p in enumerate(model.model.parameters_in_order()):
        e = rel(p, torch.from_numpy(g16[f"post_{i}"]))
        print(f"post-step {R.KEYS[i]}: {e:.2e}")
        assert e <= 5e-4, (R.KEYS[i], e)
    # the T-innermost delivery (the reference's ret_contiguous: true) trains to the same place
    other = golden_model(g16, dev)
    other.configure_optimizers()
    for s in range(3):
        other.training_step(change_layout_torch(nthw, "NTHW", "NHWT", ret_contiguous=True), s)
    for p, q in zip(model.model.parameters_in_order(), other.model.parameters_in_order()):
        assert rel(q, p) <= 1e-5


def test_validation_step(dev, g16):
    model = golden_model(g16, dev)
    model.configure_optimizers()
    batch = torch.from_numpy(g16["batch"]).to(dev)
    before = [p.detach().clone() for p in model.parameters()]
    val = model.validation_step(batch)
    for p, q in zip(model.parameters(), before):
        assert torch.equal(p, q) and p.grad is None
    assert not val.requires_grad
    loss, _ = model.training_step(batch)
    assert torch.equal(val, loss)
    assert abs(val.item() - float(g16["loss"])) <= 1e-5 * float(g16["loss"])


def test_experiment_script_runs(dev, tmp_path):
    from weatherforecastingtoolkit_amd.experiments.v1_experiments.prediff_mlp_sevir import train
    assert train.main(["--max-steps", "3", "dataset.batch_size=2", f"experiment_path={tmp_path}"]) == 0
    ck = torch.load(tmp_path / "outputs" / "mlp_sevir" / "checkpoints" / "last.ckpt", map_location="cpu")
    assert ck["global_step"] == 3
    assert list(ck["state_dict"]) == ["model._orig_mod." + k for k in R.KEYS]
    model = M.Model(C.load(CONFIG))
    model.load_state_dict(ck["state_dict"], strict=True)
    for p, k in zip(model.model.parameters_in_order(), R.KEYS):
        assert torch.equal(p.detach(), ck["state_dict"]["model._orig_mod." + k])
    with pytest.raises(KeyError, match="Invalid override key"):
        train.main(["--max-steps", "1", "dataset.batchsize=2"])
