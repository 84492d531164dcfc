"""CPU: the ae_gan residual autoencoders (forward only) — state-dict layout and seeded initialisation of the product
classes against tests/golden/g21_ae_gan.npz (recorded from the reference's own classes), the torch restatement
tests/ae_gan_ref.py against the same fixture, the checkpoint prefix filter, the live-tap and route rules of csrc/resae.hip
against their restatements, and every refusal."""
import os

import numpy as np
import pytest
import torch

from tests import ae_gan_ref as R
from weatherforecastingtoolkit_amd import _lib, ops
from weatherforecastingtoolkit_amd import config as C
from weatherforecastingtoolkit_amd._lib import WfaeError
from weatherforecastingtoolkit_amd.experiments.v1_experiments import _ae_gan as M
from weatherforecastingtoolkit_amd.experiments.v1_experiments._latents import Autoencoder
from weatherforecastingtoolkit_amd.experiments.v1_experiments.ae_gan import train as T

G21 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g21_ae_gan.npz")
EXP = os.path.join(os.path.dirname(M.__file__), "ae_gan")
ENTRY_POINTS = ["wfae_resae_live_taps", "wfae_resae_pack_bytes", "wfae_resae_pack", "wfae_resae_workspace_bytes",
                "wfae_resae_conv"]


@pytest.fixture(scope="module")
def g21():
    return np.load(G21, allow_pickle=False)


@pytest.fixture(scope="module")
def big(g21):
    torch.manual_seed(int(g21["seed"]))
    return M.ConvAutoencoderBIG()


def fixture_keys(g, sfx=""):
    return [(str(k), tuple(int(d) for d in str(s).split())) for k, s in zip(g["keys" + sfx], g["shapes" + sfx])]


def test_state_dict_layout_and_seeded_init(g21, big):
    """keys, shapes, order and the seeded initial values of both models are the reference's"""
    torch.manual_seed(int(g21["seed"]))
    small = M.ConvAutoencoder()
    for model, sfx, kl in ((big, "", R.key_list(True)), (small, "_small", R.key_list(False))):
        sd = model.state_dict()
        items = [(k, tuple(v.shape)) for k, v in sd.items()]
        assert len(items) == 252
        assert items == fixture_keys(g21, sfx) == kl
        assert R.keys_digest(items) == str(g21["keys_sha" + sfx])
        assert R.values_digest(sd) == str(g21["init_sha" + sfx])
        assert sum(p.numel() for p in model.parameters()) == int(g21["nparams" + sfx])
        assert not model.training and not any(p.requires_grad for p in model.parameters())
    assert int(g21["nparams"]) == 206_997_089 and int(g21["nparams_small"]) == 90_707_137
    assert M.reference_keys(big)[:7] == ["enc1.conv1.weight", "enc1.bn1.weight", "enc1.bn1.bias", "enc1.bn1.running_mean",
                                         "enc1.bn1.running_var", "enc1.bn1.num_batches_tracked", "enc1.conv2.weight"]
    assert M.reference_keys(big)[-2:] == ["final_conv.weight", "final_conv.bias"]


def test_reference_keys_round_trip():
    """state_dict -> load_state_dict (strict) on a second, differently seeded model reproduces every tensor"""
    torch.manual_seed(1)
    a = M.ResidualBlock(3, 5, 2)
    torch.manual_seed(2)
    b = M.ResidualBlock(3, 5, 2)
    a.bn1.running_mean.normal_()
    assert M.reference_keys(a) == M.reference_keys(b) == list(a.state_dict()) and len(M.reference_keys(a)) == 18
    b.load_state_dict(a.state_dict(), strict=True)
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)
    with pytest.raises(RuntimeError):
        b.load_state_dict({k: v for k, v in a.state_dict().items() if k != "bn2.bias"}, strict=True)


def test_checkpoint_prefix_filter(tmp_path):
    torch.manual_seed(3)
    a = M.ResidualBlock(2, 2, 1)
    sd = a.state_dict()
    lightning = {"state_dict": dict({"autoencoder." + k: v for k, v in sd.items()},
                                    **{"loss.discriminator.main.0.weight": torch.zeros(2),
                                       "loss.perceptual_loss.lin0.model.1.weight": torch.zeros(2)}), "global_step": 7}
    kept = M.autoencoder_state(lightning)
    assert list(kept) == list(sd) and all(torch.equal(kept[k], sd[k]) for k in sd)
    assert list(M.autoencoder_state(sd)) == list(sd)                       # a bare state dict passes through
    assert list(M.autoencoder_state({"state_dict": sd})) == list(sd)
    with pytest.raises(WfaeError, match="neither"):
        M.autoencoder_state({"autoencoder.conv1.weight": sd["conv1.weight"], "predictor.w": torch.zeros(1)})
    torch.manual_seed(4)
    b = M.ResidualBlock(2, 2, 1)
    path = str(tmp_path / "last.ckpt")
    torch.save(lightning, path)
    M.load_checkpoint(b, path)
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in sd.items())
    del lightning["state_dict"]["autoencoder.bn1.weight"]                   # strict on what is kept
    torch.save(lightning, path)
    with pytest.raises(RuntimeError, match="bn1.weight"):
        M.load_checkpoint(b, path)


def test_entry_points_declared_and_exported():
    decls = _lib.parse_header()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert name in decls and hasattr(lib, name), name
    for name in ("wfae_resae_pack", "wfae_resae_conv"):
        assert decls[name][2][-1] == "stream"


def test_live_taps_match_restatement():
    lib = _lib.load()
    for kind in range(5):
        for h in range(1, 6):
            for w in range(1, 6):
                want = R.live_taps(kind, h, w)
                assert lib.wfae_resae_live_taps(kind, h, w) == want, (kind, h, w)
                nested = ops.resae_live_taps(kind, h, w)
                assert sum(int(nested[ky][kx]) << (ky * 3 + kx) for ky in range(3) for kx in range(3)) == want, (kind, h, w)
    assert R.live_taps(0, 1, 1) == 1 << 4                                   # enc7.conv2: the centre tap only
    assert R.live_taps(1, 2, 2) == (1 << 4) | (1 << 5) | (1 << 7) | (1 << 8)  # enc7.conv1: 4 of 9
    assert R.live_taps(1, 3, 3) == R.live_taps(0, 2, 2) == R.live_taps(2, 1, 1) == 0x1ff
    # the stride-2 rule is the one of the 3x3 stride-2 family
    for h in range(1, 6):
        for w in range(1, 6):
            assert lib.wfae_resae_live_taps(1, h, w) == lib.wfae_c3s2_live_taps(h, w, (h - 1) // 2 + 1, (w - 1) // 2 + 1)
    assert lib.wfae_resae_live_taps(5, 2, 2) == lib.wfae_resae_live_taps(-1, 2, 2) == lib.wfae_resae_live_taps(0, 0, 2) == -1   # WFAE_ERR_BAD_SHAPE


def test_route_matches_restatement():
    seen = set()
    for big_ in (True, False):
        for n in (1, 8, 64):
            enc, dec = (R.ENC_BIG, R.DEC_BIG) if big_ else (R.ENC_SMALL, R.DEC_SMALL)
            for layer in R.layers(enc, dec, init_conv=not big_, n=n):
                got = ops.resae_route(*layer)
                assert got == R.route(*layer), layer
                seen.add(got)
    assert seen == {"small", "tile"}
    assert ops.resae_route(0, 8, 2048, 2048, 1, 1) == "small" and ops.resae_route(1, 8, 512, 1024, 8, 8) == "small"
    assert ops.resae_route(1, 8, 256, 512, 16, 16) == "tile" and ops.resae_route(2, 8, 512, 256, 4, 4) == "tile"


def test_pack_bytes_and_workspace_refusals():
    lib = _lib.load()
    assert lib.wfae_resae_pack_bytes(1, 0, 3, 72, 40) == 9 * 5 * 4 * 256 * 4      # [9][5 x 16 co][4 x 16 ci] fp32
    assert lib.wfae_resae_pack_bytes(1, 4, 3, 72, 40) == 5 * 4 * 256 * 4          # one tap
    assert lib.wfae_resae_pack_bytes(0, 0, 3, 72, 40) == lib.wfae_aekl_conv3_pack_bytes(72, 40, 3)
    assert lib.wfae_resae_pack_bytes(0, 0, 4, 72, 40) == lib.wfae_aekl_conv3_pack_bytes(72, 40, 4)
    assert lib.wfae_resae_pack_bytes(0, 3, 4, 72, 40) * 9 == lib.wfae_aekl_conv3_pack_bytes(72, 40, 4)
    for bad in ((2, 0, 3, 8, 8), (0, 5, 3, 8, 8), (0, 0, 2, 8, 8), (0, 0, 3, 0, 8), (0, 0, 3, 8, 4097)):
        assert lib.wfae_resae_pack_bytes(*bad) == 0, bad
    assert lib.wfae_resae_workspace_bytes(0, 8, 2048, 2048, 1, 1) > 0             # K is split
    assert lib.wfae_resae_workspace_bytes(0, 8, 32, 64, 1, 1) == 0                # one chunk: nothing to split
    assert lib.wfae_resae_workspace_bytes(0, 8, 64, 64, 8, 8) == 0                # not a small plane


def test_launch_refusals_before_any_launch():
    """argument checks of the library come before any launch: they answer on a machine without a GPU"""
    lib, buf = _lib.load(), torch.zeros(64)
    p = buf.data_ptr()
    base = dict(x=p, packed=p, scale=None, shift=None, res=None, y=p, route=0, kind=0, mode=3, res_mode=0, act=0, N=1, Cin=1,
                Cout=1, H=2, W=2, ws=None, ws_bytes=0, stream=None)

    def rc(**kw):
        return lib.wfae_resae_conv(*dict(base, **kw).values())
    SHAPE, NULL, WORKSPACE, UNSUPPORTED = -1, -2, -3, -5                   # include/wfae.h
    # every call below is refused BEFORE a launch (the buffer is host memory: a call that passed the checks would launch on it)
    assert rc(x=None) == rc(y=None) == rc(packed=None) == NULL
    assert rc(route=2) == rc(kind=5) == rc(mode=2) == rc(act=2) == SHAPE
    assert rc(res_mode=1) == rc(res=p) == rc(res_mode=3, res=p) == SHAPE
    assert rc(kind=3, res=p, res_mode=2, H=3, W=3) == SHAPE                # odd output plane behind an upsampled residual
    assert rc(N=0) == rc(H=0) == SHAPE and rc(Cin=4097) == UNSUPPORTED
    assert rc(route=1, H=5, W=5) == UNSUPPORTED                            # 25 output pixels: not a small plane
    assert rc(route=1, Cin=64, N=1) == WORKSPACE                           # K split of 2 without a workspace
    assert "workspace" in lib.wfae_last_error_string().decode()
    assert lib.wfae_resae_pack(None, p, 0, 0, 3, 1, 1, None) == NULL and lib.wfae_resae_pack(p, p, 0, 0, 2, 1, 1, None) == SHAPE


def test_block_and_model_refusals(big):
    with pytest.raises(WfaeError, match="stride"):
        M.ResidualBlock(4, 4, stride=4)
    with pytest.raises(WfaeError, match="scale_factor"):
        M.UpsampleBlock(4, 4, scale_factor=4)
    blk, up = M.ResidualBlock(4, 4), M.UpsampleBlock(4, 4)
    x = torch.zeros(1, 4, 2, 2)
    for m in (blk, up):
        assert not m.training
        m.train()
        with pytest.raises(WfaeError, match="follow-up"):
            m(x)
        m.eval()
    with pytest.raises(WfaeError, match="device tensors"):
        blk(x)                                                             # no CPU fall-back
    big.train()
    with pytest.raises(WfaeError, match="follow-up"):
        big.encode(torch.zeros(1, 1, 128, 128))
    big.eval()
    with pytest.raises(WfaeError, match="expected"):
        big.encode(torch.zeros(1, 1, 64, 64))
    with pytest.raises(WfaeError, match="expected"):
        big.decode(torch.zeros(1, 1024))
    with pytest.raises(WfaeError, match="follow-up"):
        blk.bn1(x)


def config(**over):
    cfg = C.load(os.path.join(EXP, "config.yaml"))
    cfg.trainer.total_train_steps = 10
    return C.merge(cfg, C.from_dotlist([f"{k}={v}" for k, v in over.items()]))


def test_config_has_the_reference_keys():
    cfg = C.load(os.path.join(EXP, "config.yaml"))
    assert cfg.model.name == "convautoencoder" and cfg.model.checkpoint is None
    assert cfg.ConvAutoencoder.latent_dim == 2048 and cfg.lpips.disc_start == 1.0 and cfg.lpips.perceptual_weight == 0.0
    assert cfg.lpips.recon_weight == 1 and cfg.dataset.batch_size == 8 and cfg.dataset.image_width == 128
    for k in ("project_name", "experiment_name", "experiment_path", "ConvAutoencoder2", "AttentionChargedAutoencoder", "optim",
              "cosine_warmup", "one_cycle", "lr_range_test", "trainer", "logging"):
        assert k in cfg, k


def test_model_refusals(monkeypatch):
    for name in ("convautoencoder2", "attentionchargedautoencoder"):
        with pytest.raises(WfaeError, match="not built"):
            M.Model(config(**{"model.name": name}))
    with pytest.raises(ValueError, match="Unknown model type"):
        M.Model(config(**{"model.name": "other"}))
    monkeypatch.setattr(M, "ConvAutoencoderBIG", lambda latent_dim: M.ResidualBlock(1, 2, 2))   # the refusals need no 207 M parameters
    with pytest.raises(WfaeError, match="perceptual_weight"):
        M.Model(config(**{"lpips.perceptual_weight": 0.5}))
    with pytest.raises(WfaeError, match="no latent provider"):
        M.Model(config(), autoencoder=object())
    cfg = config()
    model = T.build(cfg, 128)
    assert cfg.lpips.disc_start == 10 and model.disc_start == 10
    model.train()
    assert model.training and not model.autoencoder.training                # the autoencoder stays in eval
    model.global_step = 10
    with pytest.raises(WfaeError, match="disc_start"):
        model.test_step(torch.zeros(1, 1, 128, 128))
    for call in (lambda: model.training_step(None), model.configure_optimizers):
        with pytest.raises(WfaeError, match="follow-up"):
            call()
    with pytest.raises(WfaeError, match="frames"):
        model.frames(torch.zeros(2, 3))
    assert model.get_last_layer is not None


def test_fit_mode_is_refused_before_the_device():
    assert T.mode_of(["--mode", "fit"]) == T.mode_of(["--mode=fit", "a=b"]) == "fit"
    assert T.mode_of([]) == T.mode_of(["--max-steps", "2"]) == "test"
    with pytest.raises(WfaeError, match="forward-only"):
        T.main(["--mode", "fit"])


def test_provider_kind_is_known():
    with pytest.raises(ValueError, match="autoencoder.kind"):
        Autoencoder(128, "ae_gan.other", {})
    assert "ae_gan.convautoencoder" in Autoencoder.__doc__


def expected(g, name, full):
    full = full.detach().double().cpu()
    if name in g.files:
        return full, torch.from_numpy(g[name]).double().reshape(full.shape), None, None
    idx = R.sample_index(full.numel())
    return full.flatten()[idx], torch.from_numpy(g[f"{name}_sample"]).double(), float(full.norm()), float(g[f"{name}_norm"])


def test_restatement_reproduces_fixture(g21, big):
    """tests/ae_gan_ref.py is held to the reference: its fp64 run of G21's recipe gives the recorded fp64 tensors (to the
    fixture's rounding to fp32), its fp32 run stays within the bound the GPU path is held to"""
    sd = R.golden_state(big, g21)
    x = R.golden_input()
    for dtype, tol in ((torch.float64, lambda s: 2e-7), (torch.float32, R.bound)):
        st = {}
        recon, z = R.forward(R.cast(sd, dtype), x.to(dtype), st)
        st.update(z=z, recon=recon)
        assert sorted(st) == sorted(["z", "recon"] + [f"enc{i}" for i in range(1, 8)] + [f"dec{i}" for i in range(1, 8)])
        for name, full in st.items():
            got, want, norm, wnorm = expected(g21, name, full)
            err = float((got - want).abs().max() / want.abs().max())
            assert err <= tol(g21[f"{name}_spread"]), (name, str(dtype), err)
            if norm is not None:
                assert abs(norm - wnorm) <= tol(g21[f"{name}_spread"]) * wnorm, (name, norm, wnorm)
        loss = float((recon.double() - x.double()).abs().mean())
        assert abs(loss - float(g21["rec_loss"])) <= max(4 * float(g21["rec_loss_spread"]), 2e-6) * float(g21["rec_loss"])
    assert len(g21["metric_keys"]) == 56 and all(str(k).startswith("test_") for k in g21["metric_keys"])
