"""CPU: training the ae_gan residual autoencoders — the fp64 restatement tests/ae_gan_train_ref.py against
tests/golden/g22_ae_gan_train.npz (recorded from the reference's own classes) and its index-level gradient formulas
against autograd, `unfreeze()` / `freeze()` and the refusals that stay, the backward route rule against its restatement,
the argument checks of the new entry points of csrc/resae_bwd.hip (they answer without a device), the host logic of the
training step, and the arguments of ae_gan/fit.py."""
import os

import numpy as np
import pytest
import torch

from tests import ae_gan_ref as R
from tests import ae_gan_train_ref as T
from weatherforecastingtoolkit_amd import _lib, ops
from weatherforecastingtoolkit_amd import config as C
from weatherforecastingtoolkit_amd._lib import WfaeError
from weatherforecastingtoolkit_amd.experiments.v1_experiments import _ae_gan as M
from weatherforecastingtoolkit_amd.experiments.v1_experiments._runner import Step
from weatherforecastingtoolkit_amd.experiments.v1_experiments.ae_gan import fit as FIT

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EXP = os.path.join(os.path.dirname(M.__file__), "ae_gan")
ENTRY_POINTS = ["wfae_resae_bwd_pack_bytes", "wfae_resae_bwd_pack", "wfae_resae_bwd_data_workspace_bytes", "wfae_resae_bwd_data",
                "wfae_resae_bwd_weight_workspace_bytes", "wfae_resae_bwd_weight", "wfae_resae_join_fwd", "wfae_resae_join_bwd",
                "wfae_resae_bn_running"]
SHAPE, NULL, WORKSPACE, UNSUPPORTED = -1, -2, -3, -5                       # include/wfae.h


def test_restatement_reproduces_g22():
    """tests/ae_gan_train_ref.py computes, in fp64, what the reference's train-mode module computed: loss, z, recon, every
    parameter gradient and the updated running statistics"""
    g21 = np.load(os.path.join(GOLDEN, "g21_ae_gan.npz"), allow_pickle=False)
    g22 = np.load(os.path.join(GOLDEN, "g22_ae_gan_train.npz"), allow_pickle=False)
    torch.manual_seed(R.SEED)
    sd = T.with_grad(R.golden_state(M.ConvAutoencoderBIG(), g21), torch.float64)
    x, G = (t.double() for t in T.golden_batch())
    new = {}
    recon, z = T.forward(sd, x, new)
    loss = (recon * G).mean()
    loss.backward()
    tol = 2e-7                                                              # the fixture stores the fp64 run rounded to fp32
    assert abs(float(loss.detach()) - float(g22["loss"])) <= 1e-12 * abs(float(g22["loss"]))
    for name, t in (("z", z), ("recon", recon)):
        t = t.detach().flatten()
        assert R.spread(t[R.sample_index(t.numel())], torch.from_numpy(g22[name + "_sample"])) <= tol
        assert abs(float(t.norm()) - float(g22[name + "_norm"])) <= 1e-12 * float(g22[name + "_norm"])
    keys, off = [str(k) for k in g22["grad_keys"]], g22["grad_offsets"]
    assert keys == T.param_keys(sd) and len(keys) == 129          # 252 state entries less 41 BatchNorms x 3 buffers
    for i, k in enumerate(keys):
        gr = sd[k].grad.flatten()
        assert abs(float(gr.norm()) - g22["grad_norm"][i]) <= 1e-10 * g22["grad_norm"][i], k
        ref = torch.from_numpy(g22["grad_samples"][off[i]:off[i + 1]]).double()
        assert float((gr[T.grad_index(gr.numel())] - ref).abs().max()) <= tol * g22["grad_max"][i], k
    for name in ("running_mean", "running_var"):
        cat = torch.cat([new[f"{p}.{name}"] for p in R.bn_prefixes(list(sd))])
        assert R.spread(cat[R.sample_index(cat.numel())], torch.from_numpy(g22[name + "_sample"])) <= tol
    assert all(float(g22[k]) <= 1e-3 for k in ("loss_spread", "z_spread", "recon_spread", "step_grad_norm_spread"))
    assert float(g22["grad_spread"].max()) <= 1e-3 and float(g22["step_loss_spread"].max()) <= 1e-3
    assert len(g22["step_loss"]) == T.STEPS and g22["step_loss"][-1] < g22["step_loss"][0]


CASES = [(0, 2, 3, 4, 1, 1), (0, 2, 3, 4, 3, 4), (1, 2, 3, 4, 5, 5), (1, 2, 3, 4, 8, 6), (1, 1, 2, 2, 2, 2), (2, 2, 3, 4, 1, 1),
         (2, 2, 3, 4, 2, 3), (3, 2, 3, 4, 3, 3), (4, 2, 3, 4, 5, 4), (4, 2, 3, 4, 1, 1)]


@pytest.mark.parametrize("kind,n,cin,cout,h,w", CASES, ids=lambda v: str(v))
def test_index_formulas_match_autograd(kind, n, cin, cout, h, w):
    """the formulas the kernels of csrc/resae_bwd.hip implement, and the dead-tap rule for gradients"""
    x, wt, _, _, _ = R.unit_inputs(kind, n, cin, cout, h, w, 3)
    x, wt = x.double(), wt.double()
    dy = torch.randn(n, cout, *R.out_plane(kind, h, w), generator=torch.Generator().manual_seed(4)).double()
    dx, dw, _ = T.unit_grads(x, wt, kind, dy)
    assert float((T.dgrad_index(dy, wt, kind, x.shape) - dx).abs().max()) <= 1e-13
    assert float((T.wgrad_index(dy, x, kind) - dw).abs().max()) <= 1e-13
    dead = T.dead_taps(kind, h, w)
    assert len(dead) == 9 - bin(R.live_taps(kind, h, w)).count("1") if kind < 3 else not dead
    poisoned = wt.clone()
    for ky, kx in dead:
        assert float(dw[:, :, ky, kx].abs().max()) == 0.0                  # autograd agrees: exactly zero
        poisoned[:, :, ky, kx] = 1e30
    assert torch.equal(T.dgrad_index(dy, poisoned, kind, x.shape), T.dgrad_index(dy, wt, kind, x.shape))


def test_unfreeze_and_freeze():
    blk, up = M.ResidualBlock(4, 6, 2), M.UpsampleBlock(4, 4)
    x = torch.zeros(2, 4, 2, 2)
    for m in (blk, up):
        assert not m.training and not any(p.requires_grad for p in m.parameters())
        assert m.unfreeze() is m and all(p.requires_grad for p in m.parameters())
        assert not m.training                                               # unfreeze() does not change the mode
        m.train()
        assert m.training and all(s.training for s in m.modules())
        with pytest.raises(WfaeError, match="device tensors"):              # trainable now: it reaches the kernels
            m(x)
        m.eval()
        assert not any(s.training for s in m.modules())
        assert m.freeze() is m and not m.training and not any(p.requires_grad for p in m.parameters())
        m.train()
        with pytest.raises(WfaeError, match="follow-up"):                   # frozen again: refused as before
            m(x)
    with pytest.raises(WfaeError, match="follow-up"):
        blk.unfreeze().bn1(x)                                               # a BatchNorm is still not a layer of its own
    with pytest.raises(WfaeError, match="expected"):
        blk.train()(torch.zeros(2, 5, 2, 2))


def test_unfreeze_reaches_every_block_of_a_model():
    ae = M.ConvAutoencoder()
    assert not any(m._trainable for m in ae.modules() if isinstance(m, M._Trainable))
    ae.unfreeze()
    assert all(m._trainable for m in ae.modules() if isinstance(m, M._Trainable)) and all(p.requires_grad for p in ae.parameters())
    assert sum(isinstance(m, M._Trainable) for m in ae.modules()) == 1 + 15 + 7     # the model, 15 blocks, 7 upsample wrappers
    ae.train()
    with pytest.raises(WfaeError, match="device tensors"):
        ae.encode(torch.zeros(1, 1, 128, 128))
    ae.freeze()
    assert not ae.training and not any(p.requires_grad for p in ae.parameters())
    # num_batches_tracked is counted on the host and written when the state is read
    bn = ae.enc1.bn1
    bn._nbt_pending = 3
    assert int(ae.state_dict()["enc1.bn1.num_batches_tracked"]) == 3 and bn._nbt_pending == 0


def test_backward_route_matches_restatement():
    seen = set()
    for n in (1, 8, 32):
        for layer in R.layers(R.ENC_BIG, R.DEC_BIG, n=n) + R.layers(R.ENC_SMALL, R.DEC_SMALL, init_conv=True, n=n):
            for what in ("data", "weight"):
                got = ops.resae_bwd_route(what, *layer)
                assert got == T.bwd_route(what, *layer), (what, layer)
                seen.add(got)
    assert seen == {"small", "tile"}
    assert ops.resae_bwd_route("weight", 0, 8, 2048, 2048, 1, 1) == "small" and ops.resae_bwd_route("data", 1, 8, 512, 1024, 8, 8) == "small"
    assert ops.resae_bwd_route("data", 2, 8, 512, 256, 4, 4) == "tile"
    with pytest.raises(WfaeError, match="what"):
        ops.resae_bwd_route("bias", 0, 1, 1, 1, 1, 1)


def test_entry_points_declared_exported_and_sized():
    decls, lib = _lib.parse_header(), _lib.load()
    for name in ENTRY_POINTS:
        assert name in decls and hasattr(lib, name), name
    assert lib.wfae_version() == 103
    assert lib.wfae_resae_bwd_pack_bytes(0, 72, 40) == 9 * 3 * 6 * 256 * 4     # [9][3 x 16 ci][6 x 16 co (3 chunks of 32)] fp32
    assert lib.wfae_resae_bwd_pack_bytes(4, 72, 40) == 3 * 6 * 256 * 4
    for bad in ((5, 8, 8), (0, 0, 8), (0, 8, 4097)):
        assert lib.wfae_resae_bwd_pack_bytes(*bad) == 0, bad
    # data gradient: K = Cout is split on the small route when the columns do not fill the chip; kind 2 always finishes
    assert lib.wfae_resae_bwd_data_workspace_bytes(1, 0, 8, 2048, 2048, 1, 1) > 0
    assert lib.wfae_resae_bwd_data_workspace_bytes(1, 0, 8, 64, 32, 1, 1) == 0
    assert lib.wfae_resae_bwd_data_workspace_bytes(1, 2, 8, 64, 32, 1, 1) == 64 * 32 * 4        # [64 ci][8 x 2 x 2 pixels] fp32
    assert lib.wfae_resae_bwd_data_workspace_bytes(0, 2, 8, 64, 32, 64, 64) == 0                  # tile route: in registers
    # weight gradient: one slab per SPLIT of the columns, never per sample
    assert lib.wfae_resae_bwd_weight_workspace_bytes(1, 0, 8, 2048, 2048, 1, 1) == 0              # 2048 tiles fill the chip
    slab = 64 * 32 * 9 * 4
    ws = lib.wfae_resae_bwd_weight_workspace_bytes(0, 0, 8, 32, 64, 128, 128)
    assert ws % slab == 0 and 1 < ws // slab <= 8 * 16 * 16
    assert lib.wfae_resae_bwd_weight_workspace_bytes(1, 0, 8, 64, 64, 8, 8) == 0                  # refused: not a small plane


def test_launch_refusals_before_any_launch():
    """the argument checks come before any launch: they answer on a machine without a GPU (the buffer is host memory)"""
    lib, buf = _lib.load(), torch.zeros(64)
    p = buf.data_ptr()
    data = dict(dy=p, packed_t=p, add=None, dx=p, route=0, kind=0, N=1, Cin=1, Cout=1, H=2, W=2, ws=None, ws_bytes=0, stream=None)
    weight = dict(dy=p, x=p, dw=p, dbias=None, route=0, kind=0, N=1, Cin=1, Cout=1, H=2, W=2, ws=None, ws_bytes=0, stream=None)

    def rd(**kw):
        return lib.wfae_resae_bwd_data(*dict(data, **kw).values())

    def rw(**kw):
        return lib.wfae_resae_bwd_weight(*dict(weight, **kw).values())
    assert rd(dy=None) == rd(packed_t=None) == rd(dx=None) == NULL
    assert rw(dy=None) == rw(x=None) == rw(dw=None) == NULL
    for r in (rd, rw):
        assert r(route=2) == r(kind=5) == r(kind=-1) == r(N=0) == r(H=0) == r(W=8193) == SHAPE
        assert r(Cin=4097) == r(Cout=0) == UNSUPPORTED
        assert r(route=1, H=5, W=5) == UNSUPPORTED                          # 25 output pixels: not a small plane
        assert r(route=1, kind=1, H=9, W=8) == UNSUPPORTED                  # 5 x 4 = 20 output pixels
        assert r(Cin=4096, H=1024, W=1024) == SHAPE                         # a sample of 2^32 elements
    assert rd(packed_t=p + 4) == SHAPE                                      # misaligned operand
    assert rd(route=1, Cout=64, H=1, W=1) == WORKSPACE                      # K split in two without a workspace
    assert "workspace" in lib.wfae_last_error_string().decode()
    assert rd(route=1, kind=2, H=1, W=1) == WORKSPACE                       # kind 2 on the small route finishes from ws
    assert rw(N=4, H=16, W=16) == WORKSPACE                                 # 16 column groups split over workgroups
    assert lib.wfae_resae_bwd_pack(None, p, 0, 1, 1, None) == lib.wfae_resae_bwd_pack(p, None, 0, 1, 1, None) == NULL
    assert lib.wfae_resae_bwd_pack(p, p, 5, 1, 1, None) == SHAPE and lib.wfae_resae_bwd_pack(p, p, 0, 1, 4097, None) == UNSUPPORTED

    join = dict(c2=p, s2=p, h2=p, r=p, ss=None, hs=None, y=p, res_mode=1, N=1, C=1, H=2, W=2, stream=None)
    jb = dict(dy=p, c2=p, s2=p, h2=p, r=p, ss=None, hs=None, dpre=p, dres=None, res_mode=1, N=1, C=1, H=2, W=2, stream=None)

    def jf(**kw):
        return lib.wfae_resae_join_fwd(*dict(join, **kw).values())

    def jw(**kw):
        return lib.wfae_resae_join_bwd(*dict(jb, **kw).values())
    assert jf(c2=None) == jf(s2=None) == jf(h2=None) == jf(r=None) == jf(y=None) == NULL
    assert jw(dy=None) == jw(dpre=None) == jw(r=None) == NULL
    for j in (jf, jw):
        assert j(res_mode=0) == j(res_mode=3) == j(ss=p) == j(hs=p) == j(N=0) == j(C=0) == j(H=0) == SHAPE
    assert jf(res_mode=2, H=3) == jw(res_mode=2, H=3, dres=p) == SHAPE      # odd plane behind an upsampled residual
    assert jw(dres=p) == jw(res_mode=2) == SHAPE                            # dres goes with res_mode 2 exactly
    run = lib.wfae_resae_bn_running
    assert run(None, p, p, p, 1, 1e-5, 0.1, 8, None) == run(p, p, p, None, 1, 1e-5, 0.1, 8, None) == NULL
    assert run(p, p, p, p, 0, 1e-5, 0.1, 8, None) == run(p, p, p, p, 1, 1e-5, 0.1, 0, None) == SHAPE


def config(**over):
    cfg = C.load(os.path.join(EXP, "config.yaml"))
    cfg.trainer.total_train_steps = 10
    return C.merge(cfg, C.from_dotlist([f"{k}={v}" for k, v in over.items()]))


def test_training_step_host_logic(monkeypatch):
    monkeypatch.setattr(M, "ConvAutoencoderBIG", lambda latent_dim: M.ResidualBlock(1, 2, 2))   # the logic needs no 207 M parameters
    frozen = M.Model(config())
    assert not frozen.trainable and not any(p.requires_grad for p in frozen.parameters())
    trainable = FIT.build(config(), 128)
    assert isinstance(trainable, Step) and trainable.trained == "autoencoder" and trainable.trainable
    assert trainable.disc_start == 10 and trainable.total_steps == 10
    assert all(p.requires_grad for p in trainable.autoencoder.parameters())
    trainable.train()
    assert trainable.autoencoder.training                                   # train(mode) as for any module
    trainable.eval()
    assert not trainable.autoencoder.training
    with pytest.raises(WfaeError, match="configure_optimizers"):
        trainable.training_step(torch.zeros(1, 1, 128, 128))
    trainable.global_step = 10
    with pytest.raises(WfaeError, match="disc_start"):
        trainable.training_step(torch.zeros(1, 1, 128, 128))
    with pytest.raises(WfaeError, match="perceptual_weight"):
        M.Model(config(**{"lpips.perceptual_weight": 0.5}), trainable=True)
    with pytest.raises(WfaeError, match="accumulate_grad_batches"):
        M.Model(config(**{"trainer.accumulate_grad_batches": 2}), trainable=True)
    with pytest.raises(WfaeError, match="disc_start"):                      # a run that would reach the discriminator
        FIT.build(config(**{"lpips.disc_start": 0.5}), 128)

    # the step itself, with the device work replaced: the loss is L1 x recon_weight, the logs are the reference's keys
    calls = []
    monkeypatch.setattr(M.Fn, "l1_loss", lambda pred, inp, w: calls.append(("l1", w)) or torch.tensor(0.25))
    monkeypatch.setattr(M.Model, "forward", lambda self, x: x)
    monkeypatch.setattr(M.Model, "optimizer_step", lambda self, loss: (calls.append(("opt", float(loss))) or loss, torch.tensor(2.0)))
    trainable.global_step, trainable.opt = 0, object()
    loss, gn = trainable.training_step(torch.zeros(2, 3, 4, 4))
    assert calls == [("l1", 1.0), ("opt", 0.25)] and float(loss) == 0.25 and float(gn) == 2.0
    assert trainable.autoencoder.training and trainable.global_step == 1
    logs = trainable.logs
    assert set(logs) == {"train/total_loss", "train/rec_loss", "train/g_loss", "train/d_weight", "train/g_grad_norm"}
    assert float(logs["train/total_loss"]) == float(logs["train/rec_loss"]) == 0.25
    assert logs["train/g_loss"] == 0.0 and logs["train/d_weight"] == 0.0
    state = M.model_state(trainable)
    assert state and all(k.startswith("autoencoder.") for k in state)
    assert set(M.autoencoder_state(state)) == set(trainable.autoencoder.state_dict())


def test_fit_arguments():
    assert FIT.check_args(["--max-steps", "2", "optim.lr=1e-4"]) == ["--max-steps", "2", "optim.lr=1e-4"]
    for argv in (["--mode", "fit"], ["--mode=test"]):
        with pytest.raises(WfaeError, match="--mode"):
            FIT.check_args(argv)
    with pytest.raises(WfaeError, match="--mode"):
        FIT.main(["--mode", "test"])                                        # before the driver opens the device
