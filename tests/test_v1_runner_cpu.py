"""CPU: what the v1 latent experiments share on the host (experiments/v1_experiments/_runner.py, _latents.py) — the
step count of a run, the dictionary written to last.ckpt, the batch preamble's refusal, and the one latent provider
behind every import path."""
import os

import pytest
import torch

from tests import aekl_ref as A
from tests import prediff_mlp_ref as R
from weatherforecastingtoolkit_amd import config as C
from weatherforecastingtoolkit_amd._lib import WfaeError
from weatherforecastingtoolkit_amd.experiments.v1_experiments import _convae, _dlinear, _latents, _prediff_mlp, _runner
from weatherforecastingtoolkit_amd.experiments.v1_experiments.pretrained_ae_linear_sevir import train as linear

EXP = os.path.dirname(_runner.__file__)


@pytest.mark.parametrize("n_batches,max_epochs,accumulate,max_steps,mode,want", [
    (10, 2, 1, -1, "fit", 20),      # int(10 * 2 / 1)
    (10, 2, 1, 0, "fit", 20),       # 0 is no limit
    (10, 2, 1, 5, "fit", 5),        # below the total: clamps
    (10, 2, 1, 20, "fit", 20),      # equal
    (10, 2, 1, 25, "fit", 20),      # above: never lengthens
    (10, 3, 4, -1, "fit", 7),       # int(30 / 4) = int(7.5)
    (10, 3, 4, 7, "fit", 7),
    (10, 3, 4, 6, "fit", 6),
    (1, 1, 4, -1, "fit", 1),        # int(0.25) = 0: the floor of one step
    (1, 1, 4, 1, "fit", 1),
    (1, 1, 4, 3, "fit", 1),
    (10, 2, 4, -1, "test", 10),     # one pass over the loader, whatever the epochs
    (10, 2, 4, 0, "test", 10),
    (10, 2, 4, 3, "test", 3),
    (10, 2, 4, 10, "test", 10),
    (10, 2, 4, 11, "test", 10),
])
def test_total_steps(n_batches, max_epochs, accumulate, max_steps, mode, want):
    got = _runner.total_steps(n_batches, max_epochs, accumulate, max_steps, mode)
    assert got == want and isinstance(got, int)


def test_total_steps_defaults_to_an_unlimited_fit():
    assert _runner.total_steps(6, 1, 1) == 6


def dlinear_model():
    cfg = C.load(os.path.join(EXP, "pretrained_ae_dlinear_ind", "config.yaml"))
    cfg.dlinear.update(enc_in=3)
    return _dlinear.Model(cfg)


def check_copies(ck, params):
    """the stored tensors are detached host copies: changing a parameter in place does not reach them"""
    before = {k: v.clone() for k, v in ck["state_dict"].items()}
    ptrs = {p.data_ptr() for p in params}
    for v in ck["state_dict"].values():
        assert v.device.type == "cpu" and not v.requires_grad and v.grad_fn is None
        assert v.is_contiguous() and v.data_ptr() not in ptrs and v._base is None
    with torch.no_grad():
        for p in params:
            p.add_(1.0)
    for k, v in ck["state_dict"].items():
        assert torch.equal(v, before[k])


def test_checkpoint_predictor_keys():
    model = dlinear_model()
    ck = _runner.checkpoint(_runner.predictor_state(model), 7)
    assert list(ck) == ["state_dict", "global_step"] and ck["global_step"] == 7
    sd = model.predictor.state_dict()
    assert list(ck["state_dict"]) == ["predictor." + k for k in sd]
    assert [(k, tuple(v.shape)) for k, v in ck["state_dict"].items()] == model.predictor.reference_keys("predictor.")
    assert list(ck["state_dict"])[:2] == ["predictor.Linear_Seasonal.0.weight", "predictor.Linear_Seasonal.0.bias"]
    for k, v in sd.items():
        assert torch.equal(ck["state_dict"]["predictor." + k], v)
    check_copies(ck, list(model.predictor.parameters()))


def test_checkpoint_compiled_mlp_keys():
    model = _prediff_mlp.Model(C.load(os.path.join(EXP, "prediff_mlp_sevir", "config.yaml")))
    ck = _runner.checkpoint(model.state_dict(), 3)
    assert ck["global_step"] == 3
    assert list(ck["state_dict"]) == ["model._orig_mod." + k for k in R.KEYS] == list(model.state_dict())
    for p, k in zip(model.model.parameters_in_order(), R.KEYS):
        assert torch.equal(p.detach(), ck["state_dict"]["model._orig_mod." + k])
    check_copies(ck, list(model.parameters()))


def linear_model():
    return linear.Model(C.load(os.path.join(EXP, "pretrained_ae_linear_sevir", "config.yaml")), latent_channels=2)


@pytest.mark.parametrize("make", [linear_model, dlinear_model])
def test_frames_without_a_provider_are_refused(make):
    model = make()
    with pytest.raises(WfaeError, match="needs the frozen autoencoder"):
        model.frames_latents(torch.zeros(1, 25, 16, 16))
    with pytest.raises(WfaeError, match="needs the frozen autoencoder"):
        model.training_step({"vil": torch.zeros(1, 25, 16, 16)})
    v = torch.zeros(1, 25, 2, 4, 4)
    frames, got = model.frames_latents({"vil": v})
    assert frames is None and got is v
    assert model.frames_latents(v)[1] is v


def test_one_provider_class():
    A_ = _latents.Autoencoder
    assert _dlinear.Autoencoder is A_ and linear.Autoencoder is A_ and _convae.Autoencoder is A_
    from weatherforecastingtoolkit_amd.experiments.v1_experiments._dlinear import Autoencoder as a
    from weatherforecastingtoolkit_amd.experiments.v1_experiments.pretrained_ae_linear_sevir.train import (
        Autoencoder as b, Model)
    assert a is b is A_ and Model is linear.Model
    for name in ("pretrained_ae_dlinear_sevir", "pretrained_ae_dlinear_ind", "pretrained_ae_dlinear_indc_indp",
                 "pretrained_ae_convae_sevir"):
        mod = __import__(f"weatherforecastingtoolkit_amd.experiments.v1_experiments.{name}.train",
                         fromlist=["Autoencoder"])
        assert mod.Autoencoder is A_ and callable(mod.main) and os.path.isdir(mod.HERE)
    assert _dlinear.Model is not _convae.Model and issubclass(_dlinear.Model, _runner.Step)


def test_provider_kinds():
    kl = C.Cfg(dict(A.CONFIGS["small"], kind="autoencoder_kl", checkpoint=None, chunk_frames=3, seed=1234))
    want = {"ae_64x8x8_lin.enc": True, "autoencoder_kl": True, "ae_vit.tokens": False}
    for kind, decodes in want.items():
        prov = _latents.Autoencoder(64, kind, kl if kind == "autoencoder_kl" else None)
        assert prov.kind == kind and prov.can_decode() is decodes
        assert not any(p.requires_grad for p in prov.parameters())
    with pytest.raises(WfaeError, match="no decoder"):
        prov.decode(torch.zeros(1, 1, 512, 8, 8))
    with pytest.raises(ValueError, match="nonsense"):
        _latents.Autoencoder(64, "nonsense")
    assert len(_latents.Autoencoder.AEKL_KEYS) == 11
