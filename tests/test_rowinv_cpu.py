"""CPU: the host side of the pass-invariant frozen AutoencoderKL — the C ABI of wfae_linear_fwd_rowinv up to the launch,
the wrapper's refusals, `AutoencoderKL.pass_invariant` against `unfreeze`, the provider's `pass_invariant` key, the
refusals of `--invariant-encode`, and the compact plan of `Autoencoder._encode_cached` as host logic: the encoder and the
two cache kernels are replaced by host stand-ins that record what they were asked for."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch
import torch.nn as tnn

from tests import aekl_ref as A
from weatherforecastingtoolkit_amd import _lib, ops
from weatherforecastingtoolkit_amd import config as C
from weatherforecastingtoolkit_amd._lib import WfaeError
from weatherforecastingtoolkit_amd.experiments.v1_experiments import _runner
from weatherforecastingtoolkit_amd.experiments.v1_experiments._latents import Autoencoder
from weatherforecastingtoolkit_amd.pipeline.models.autoencoderkl import AutoencoderKL
from weatherforecastingtoolkit_amd.pipeline.models.autoencoderkl.attention import AttentionBlock


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_symbol_and_argument_validation():
    decls = _lib.parse_header()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert len(decls) == 230
    name = "wfae_linear_fwd_rowinv"
    assert name in decls and hasattr(raw, name)
    assert decls[name][2] == ["x", "w", "bias", "y", "B", "In", "Out", "stream"]      # no workspace
    lib = _lib.load()
    assert lib.wfae_version() == 103
    p = 0x7F0000000000                 # never dereferenced: every call below is refused before a launch
    f = lib.wfae_linear_fwd_rowinv
    for args in [(None, p, p, p), (p, None, p, p), (p, p, p, None), (None, None, None, None)]:
        assert f(*args, 64, 512, 512, None) == -2 and b"null" in lib.wfae_last_error_string()
    for sizes in [(0, 512, 512), (64, 0, 512), (64, 512, 0), (-1, 512, 512), (64, -32, 512)]:
        assert f(p, p, None, p, *sizes, None) == -1 and b"bad shape" in lib.wfae_last_error_string()
    for sizes in [(64, 48, 512), (64, 512, 48), (64, 4128, 512), (64, 512, 4128), (1, 1, 1), (64, 500, 512)]:
        assert f(p, p, None, p, *sizes, None) == -5 and b"multiples of 32" in lib.wfae_last_error_string()
    # a null pointer is reported before a bad size, a bad size before an unsupported one
    assert f(None, p, None, p, 0, 48, 512, None) == -2
    assert f(p, p, None, p, 0, 48, 512, None) == -1


def test_ops_refuse_host_tensors_and_bad_rows():
    with pytest.raises(WfaeError, match="device tensors"):
        ops.linear_fwd_rowinv(torch.zeros(2, 32), torch.zeros(32, 32))
    with pytest.raises(WfaeError, match="device tensors"):
        ops.linear_fwd_rowinv(torch.zeros(2, 32), torch.zeros(32, 32), torch.zeros(32))


# ------------------------------------------------------------------------------------------------ the model
def test_pass_invariant_belongs_to_the_frozen_model():
    model = AutoencoderKL(**A.CONFIGS["small"])
    blocks = [m for m in model.modules() if isinstance(m, AttentionBlock)]
    assert len(blocks) == 2                                   # the encoder's and the decoder's mid block
    assert not model.invariant and not any(b.row_invariant for b in blocks)
    assert model.pass_invariant() is model
    assert model.invariant and all(b.row_invariant for b in blocks)
    ones = [m for m in model.modules() if isinstance(m, tnn.Conv2d) and tuple(m.kernel_size) == (1, 1)]
    assert model.quant_conv in ones and model.post_quant_conv in ones and all(m.row_invariant for m in ones)
    assert not any(getattr(m, "row_invariant", False) for m in model.modules() if isinstance(m, tnn.Conv2d) and m not in ones)
    keys = list(model.state_dict())
    assert keys == list(AutoencoderKL(**A.CONFIGS["small"]).state_dict())       # the mode is no part of the state
    with pytest.raises(WfaeError, match="pass-invariant"):
        model.unfreeze()
    assert not model.trainable and not any(p.requires_grad for p in model.parameters())
    assert model.pass_invariant(False) is model and not any(b.row_invariant for b in blocks)
    model.unfreeze()
    with pytest.raises(WfaeError, match="unfrozen"):
        model.pass_invariant()
    assert not model.invariant and not any(b.row_invariant for b in blocks)
    model.freeze().pass_invariant()
    assert all(b.row_invariant for b in blocks)


def kl_provider(chunk=4, sample=False, **extra):
    cfg = C.Cfg(dict(A.CONFIGS["small"], kind="autoencoder_kl", checkpoint=None, chunk_frames=chunk, seed=0, sample=sample,
                     **extra))
    return Autoencoder(32, "autoencoder_kl", cfg)


def test_provider_key():
    assert not kl_provider().pass_invariant and not kl_provider().autoencoder.invariant
    assert not kl_provider(pass_invariant=False).autoencoder.invariant
    prov = kl_provider(pass_invariant=True)
    assert prov.pass_invariant and prov.autoencoder.invariant
    assert all(m.row_invariant for m in prov.autoencoder.modules() if isinstance(m, AttentionBlock))


@pytest.mark.parametrize("kind", ["ae_64x8x8_lin.enc", "ae_vit.tokens", "ae_gan.convautoencoder"])
def test_the_key_and_the_flag_are_refused_for_every_kind_but_autoencoder_kl(kind):
    for value in (True, False):
        with pytest.raises(WfaeError, match="autoencoder_kl") as e:
            Autoencoder(128, kind, {"latent_dim": 64, "pass_invariant": value})
        assert kind in str(e.value)
    prov = Autoencoder(128, kind, {"latent_dim": 64})
    with pytest.raises(WfaeError, match="autoencoder_kl"):
        prov.set_pass_invariant()
    with pytest.raises(WfaeError, match="--invariant-encode.*only the frozen AutoencoderKL") as e:
        _runner.enable_invariant_encode(Tiny(prov))
    assert kind in str(e.value) and not prov.pass_invariant


class Tiny(_runner.Step, tnn.Module):
    def __init__(self, autoencoder):
        super().__init__()
        self.autoencoder = autoencoder


def test_the_flag_without_a_provider_and_with_one(monkeypatch):
    with pytest.raises(WfaeError, match="--invariant-encode.*no frozen latent provider"):
        _runner.enable_invariant_encode(Tiny(None))
    from tests.test_ae_gan_cpu import config
    from weatherforecastingtoolkit_amd.experiments.v1_experiments import _ae_gan as M
    monkeypatch.setattr(M, "ConvAutoencoderBIG", lambda latent_dim: M.ResidualBlock(1, 2, 2))   # no 207 M parameters
    with pytest.raises(WfaeError, match="--invariant-encode.*no frozen latent provider"):
        _runner.enable_invariant_encode(M.Model(config()))
    prov = kl_provider()
    assert _runner.enable_invariant_encode(Tiny(prov)) is prov
    assert prov.pass_invariant and prov.autoencoder.invariant
    # with the cache, in either order
    from tests.test_latent_cache_cpu import events
    from weatherforecastingtoolkit_amd.pipeline.datasets.sevire.sevir import SEVIRFrameLoader
    cache = _runner.enable_latent_cache(Tiny(prov), SEVIRFrameLoader(events(2, 7), 1), 16)
    assert cache is prov.cache and prov.pass_invariant


def test_a_cache_filled_in_the_other_mode_is_emptied():
    prov = kl_provider()
    cache = prov.enable_cache(4)
    cache.plan([("train", 1)])
    cache.serves("train", 4, 4)
    prov.set_pass_invariant(False)
    assert cache.frames_cached == 1                           # no change of mode
    prov.set_pass_invariant()
    assert cache.frames_cached == 0 and cache.pass_frames == {}


# ------------------------------------------------------------------------------------------------ the compact plan
class Host:
    """stand-ins on the host: the encoder gives frame f (a constant plane of value v) the row [v, v + 0.5], and records the
    frames of every pass; scatter and gather are torch indexing"""

    def __init__(self, prov, monkeypatch):
        self.passes = []
        monkeypatch.setattr(prov.autoencoder, "encode", self.encode, raising=False)
        monkeypatch.setattr(prov.autoencoder, "moments", self.moments, raising=False)
        monkeypatch.setattr(ops, "latent_scatter", self.scatter)
        monkeypatch.setattr(ops, "latent_gather", self.gather)

    def moments(self, frames):
        self.passes.append([int(v) for v in frames[:, 0, 0, 0]])
        v = frames[:, 0, 0, 0]
        return torch.stack([v, v + 0.5], 1).view(-1, 2, 1, 1)

    def encode(self, frames):
        class Posterior:
            def __init__(self, m):
                self.m = m

            def mode(self):
                return self.m
        return Posterior(self.moments(frames))

    @staticmethod
    def scatter(src, slots, table):
        for m, s in enumerate(slots):
            if s >= 0:
                table[s] = src[m]
        return table

    @staticmethod
    def gather(table, fresh, index, shape_bt, noise=None):
        assert noise is None
        return torch.stack([table[i] if i >= 0 else fresh[-1 - i] for i in index]).view(*shape_bt, -1)


def frames_of(ids, b):
    """(b, len(ids) / b, 1, 2, 2): frame i is a constant plane of value ids[i]"""
    return torch.tensor(ids, dtype=torch.float32).view(b, -1, 1, 1, 1).expand(b, len(ids) // b, 1, 2, 2).contiguous()


def encode(prov, ids, b=1, split="train"):
    z = prov.encode(frames_of(ids, b), ids=(split, np.asarray(ids)))
    assert z.shape == (b, len(ids) // b, 2, 1, 1)
    assert z[..., 0, 0, 0].flatten().tolist() == [float(i) for i in ids]
    assert z[..., 1, 0, 0].flatten().tolist() == [i + 0.5 for i in ids]
    return z


def test_compact_plan_encodes_the_unique_misses_in_short_passes(monkeypatch):
    prov = kl_provider(chunk=4, pass_invariant=True)
    host, cache = Host(prov, monkeypatch), prov.enable_cache(16)
    encode(prov, [0, 1, 2, 0, 4, 5, 6, 2], b=2)
    assert host.passes == [[0, 1, 2, 4], [5, 6]]              # six distinct frames: a pass of 4, a pass of 2, no repeats
    encode(prov, [9, 3, 0])                                   # a short batch, a tail chunk: served like any other
    assert host.passes[2:] == [[9, 3]]
    encode(prov, [9, 3, 0])
    assert host.passes[3:] == []                              # and it hits the second time
    encode(prov, [1, 7, 2, 5, 0], split="val")                # another split: other frames, same table
    assert host.passes[3:] == [[1, 7, 2, 5], [0]]
    assert cache.stats() == {"hits": 2 + 1 + 3, "misses": 6 + 2 + 5, "frames_cached": 13, "capacity": 16,
                             "MiB": round(16 * 2 * 4 / 2 ** 20, 3), "bypassed": 0}
    assert cache.pass_frames == {}


def test_compact_plan_in_one_pass_and_past_the_capacity(monkeypatch):
    prov = kl_provider(chunk=0, pass_invariant=True)
    host, cache = Host(prov, monkeypatch), prov.enable_cache(8)
    encode(prov, list(range(8)), b=2)
    assert host.passes == [list(range(8))] and cache.frames_cached == 8            # the table is full
    encode(prov, [0, 1, 2, 30, 4, 5, 6, 7], b=2)
    assert host.passes[1:] == [[30]]                          # one missing frame of eight costs itself
    for _ in range(2):                                        # frames past the capacity cost only themselves, every time
        encode(prov, [31, 1, 30, 3, 30], b=1)
    assert host.passes[2:] == [[31, 30], [31, 30]]
    assert (cache.hits, cache.misses, cache.frames_cached, cache.bypassed) == (7 + 3 + 3, 8 + 1 + 2 + 2, 8, 0)


def test_the_default_mode_still_fills_whole_passes_and_goes_around(monkeypatch):
    prov = kl_provider(chunk=4)
    host, cache = Host(prov, monkeypatch), prov.enable_cache(16)
    encode(prov, [0, 1, 2, 0, 4, 5, 6, 2], b=2)
    assert host.passes == [[0, 1, 2, 4], [5, 6, 6, 6]]        # whole passes, filled up with repeats of the last frame
    assert prov._encode_cached(frames_of([9, 3, 0], 1), ("train", np.asarray([9, 3, 0])), None, None) is None
    assert cache.bypassed == 3
