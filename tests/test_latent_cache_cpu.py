"""CPU: the host side of the latent cache of the frozen AutoencoderKL provider — the loaders' frame ids against
hand-written expectations and against the frames `batch_u8` slices, `LatentCache.plan` (slot order, duplicates, a full
table, no eviction, counters), the refusals of `enable_cache` / `--latent-cache` / `encode(ids=...)`, and the C ABI of
wfae_latent_scatter / wfae_latent_gather up to the launch."""
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
from weatherforecastingtoolkit_amd.experiments.v1_experiments._latents import Autoencoder, LatentCache
from weatherforecastingtoolkit_amd.pipeline.datasets.sevir.sevir import SequenceBatchLoader
from weatherforecastingtoolkit_amd.pipeline.datasets.sevire.sevir import SEVIRFrameLoader


def events(n, t, hw=4):
    """uint8 (n, hw, hw, t) events whose every pixel of frame t of event e is e * t_total + t: a frame names itself"""
    ev = np.zeros((n, hw, hw, t), dtype=np.uint8)
    ev += (np.arange(n)[:, None] * t + np.arange(t)[None, :]).astype(np.uint8)[:, None, None, :]
    return ev


# ------------------------------------------------------------------------------------------------ frame ids
def test_frame_loader_ids_two_shards_and_an_event_boundary():
    """3 events x 10 frames, sequences of 4 every 3 frames: 3 per event (starts 0, 3, 6), 9 in all; batches of 2 over 2
    shards: rank r takes the global batches r, 2 + r.  Global batch 1 = sequences 2, 3 = (event 0, start 6) and (event 1,
    start 0): it crosses the event boundary"""
    ev = events(3, 10)
    r0 = SEVIRFrameLoader(ev, 2, seq_len=4, stride=3, num_shard=2, rank=0)
    r1 = SEVIRFrameLoader(ev, 2, seq_len=4, stride=3, num_shard=2, rank=1)
    assert len(r0) == len(r1) == 2
    assert r0.frame_ids(0).tolist() == [[0, 1, 2, 3], [3, 4, 5, 6]]
    assert r0.frame_ids(1).tolist() == [[13, 14, 15, 16], [16, 17, 18, 19]]
    assert r1.frame_ids(0).tolist() == [[6, 7, 8, 9], [10, 11, 12, 13]]
    assert r1.frame_ids(1).tolist() == [[20, 21, 22, 23], [23, 24, 25, 26]]
    ids = r1.frame_ids(0)
    assert ids.dtype == np.int64 and ids.shape == (2, 4)
    # the ids name the frames the loader slices: pixel value = event * 10 + frame = id
    for ld in (r0, r1):
        for i in range(len(ld)):
            assert np.array_equal(ld.batch_u8(i)[:, 0, 0, :], ld.frame_ids(i))


def test_frame_loader_ids_with_presample():
    """2 events x 10 raw frames pooled by 2 in time: 5 frames an event (raw 0, 2, 4, 6, 8), the id space counts those.
    Sequences of 2 every frame: 4 per event.  Batch 1 of 3 = (event 0, start 3), (event 1, start 0), (event 1, start 1)"""
    ld = SEVIRFrameLoader(events(2, 10), 3, seq_len=2, stride=1, presample=(2, 1, 1))
    assert ld.raw_seq_len == 5 and ld.num_seq_per_event == 4 and len(ld) == 2
    assert ld.frame_ids(0).tolist() == [[0, 1], [1, 2], [2, 3]]
    assert ld.frame_ids(1).tolist() == [[3, 4], [5, 6], [6, 7]]
    # batch_u8 is the raw span under the sequence, 2 * (2 - 1) + 1 = 3 raw frames: pooled frame k starts at raw frame 2k
    for i in range(2):
        u8, ids = ld.batch_u8(i), ld.frame_ids(i)
        assert u8.shape[-1] == 3
        event, pooled = np.divmod(ids, 5)
        assert np.array_equal(u8[:, 0, 0, ::2], event * 10 + 2 * pooled)


def test_sequence_batch_loader_ids_follow_the_epoch_order():
    """2 events x 7 frames, sequences of 3 every 2 frames: 3 per event (starts 0, 2, 4); global sequence 4 = (event 1,
    start 2) = frames 7 + 2 .. 7 + 4"""
    ev = events(2, 7)
    fixed = SequenceBatchLoader(ev, [4, 0, 5, 1, 2], 2, 3, 2, "NTHW")
    assert len(fixed) == 3
    assert fixed.frame_ids(0).tolist() == [[9, 10, 11], [0, 1, 2]]
    assert fixed.frame_ids(1).tolist() == [[11, 12, 13], [2, 3, 4]]
    assert fixed.frame_ids(2).tolist() == [[4, 5, 6]]              # the short last batch
    for i in range(3):
        assert np.array_equal(fixed.batch_u8(i)[:, 0, 0, :], fixed.frame_ids(i))
    # a fresh permutation per epoch: the ids are those of the epoch's own order, and the frames batch_u8 slices
    ld = SequenceBatchLoader(ev, [4, 0, 5, 1, 2, 3], 2, 3, 2, "NTHW", shuffle_order=True, seed=3)
    seen = []
    for epoch in (0, 1):
        ld.set_epoch(epoch)
        rows = []
        for i in range(len(ld)):
            want = [[(s // 3) * 7 + (s % 3) * 2 + k for k in range(3)] for s in ld.order[2 * i:2 * i + 2]]
            assert ld.frame_ids(i).tolist() == want
            assert np.array_equal(ld.batch_u8(i)[:, 0, 0, :], ld.frame_ids(i))
            rows += want
        seen.append(rows)
    assert seen[0] != seen[1] and sorted(seen[0]) == sorted(seen[1])


def test_rank_shard_forwards_frame_ids():
    ld = SequenceBatchLoader(events(2, 7), [4, 0, 5, 1, 2, 3], 1, 3, 2, "NTHW")
    shard = _runner.RankShard(ld, 2, 1)
    assert len(shard) == 3
    assert shard.frame_ids(0).tolist() == [[0, 1, 2]]               # global batch 1: sequence 0
    assert shard.frame_ids(1).tolist() == [[2, 3, 4]]               # global batch 3: sequence 1
    assert shard.frame_ids(2).tolist() == [[7, 8, 9]]               # global batch 5: sequence 3 = (event 1, start 0)
    with pytest.raises(IndexError):
        shard.frame_ids(3)


# ------------------------------------------------------------------------------------------------ the plan
def k(*ids, split="train"):
    return [(split, i) for i in ids]


def test_plan_hands_out_slots_in_first_seen_order_and_plans_a_duplicate_once():
    c = LatentCache(8)
    assert (c.hits, c.misses, c.frames_cached, c.bytes) == (0, 0, 0, 0)
    missing, slots, index = c.plan(k(30, 10, 30, 20, 10))
    assert missing == k(30, 10, 20)
    assert slots.tolist() == [0, 1, 2] and slots.dtype == np.int64
    # frames encoded this step are read from `fresh`, the repeats too
    assert index.tolist() == [-1, -2, -1, -3, -2] and index.dtype == np.int64
    assert (c.hits, c.misses, c.frames_cached) == (2, 3, 3)
    missing, slots, index = c.plan(k(20, 40, 30, 40))
    assert missing == k(40) and slots.tolist() == [3]
    assert index.tolist() == [2, -1, 0, -1]
    assert (c.hits, c.misses, c.frames_cached) == (5, 4, 4)
    # the split is part of the key
    missing, slots, index = c.plan(k(30, split="val") + k(30))
    assert missing == k(30, split="val") and slots.tolist() == [4] and index.tolist() == [-1, 0]
    # all hit: nothing to encode
    missing, slots, index = c.plan(k(10, 20, 30, 40))
    assert missing == [] and slots.shape == (0,) and index.tolist() == [1, 2, 0, 3]
    assert c.stats() == {"hits": 10, "misses": 5, "frames_cached": 5, "capacity": 8, "MiB": 0.0, "bypassed": 0}


def test_plan_at_capacity_keeps_what_it_has_and_never_evicts():
    c = LatentCache(3)
    missing, slots, index = c.plan(k(1, 2, 3, 4, 5, 4))             # full after the third frame, in the middle of the batch
    assert missing == k(1, 2, 3, 4, 5) and slots.tolist() == [0, 1, 2, -1, -1]
    assert index.tolist() == [-1, -2, -3, -4, -5, -4]
    assert (c.hits, c.misses, c.frames_cached) == (1, 5, 3)
    for _ in range(2):                                              # 4 and 5 stay fresh on every later step; 1 .. 3 stay cached
        missing, slots, index = c.plan(k(5, 1, 4, 3, 2))
        assert missing == k(5, 4) and slots.tolist() == [-1, -1]
        assert index.tolist() == [-1, 0, -2, 2, 1]
    assert (c.hits, c.misses, c.frames_cached) == (7, 9, 3)
    assert c.slot == {("train", 1): 0, ("train", 2): 1, ("train", 3): 2}
    with pytest.raises(ValueError):
        LatentCache(0)


def test_only_batches_of_the_splits_pass_size_are_served():
    """the encoder's GEMM routes follow the number of frames in a pass, so a row belongs to one pass size"""
    c = LatentCache(8)
    assert c.serves("train", 104, 0) == 104 and c.serves("train", 104, 0) == 104        # one pass of all frames
    assert c.serves("train", 52, 0) == 0 and c.bypassed == 52                            # the short last batch
    assert c.serves("val", 52, 0) == 52                                                  # a split has its own size
    c = LatentCache(8)
    assert c.serves("train", 104, 8) == 8 and c.serves("train", 16, 8) == 8              # whole chunks, any batch size
    assert c.serves("train", 20, 8) == 0 and c.serves("train", 5, 8) == 0                # a tail chunk of 4, of 5
    assert c.serves("val", 6, 4) == 0 and c.pass_frames == {"train": 8} and c.bypassed == 31
    assert c.serves("val", 8, 4) == 4 and c.serves("val", 8, 8) == 0


# ------------------------------------------------------------------------------------------------ refusals
def kl_provider(sample=False):
    cfg = C.Cfg(dict(A.CONFIGS["small"], kind="autoencoder_kl", checkpoint=None, chunk_frames=4, seed=0, sample=sample))
    return Autoencoder(32, "autoencoder_kl", cfg)


class Tiny(_runner.Step, tnn.Module):
    def __init__(self, autoencoder):
        super().__init__()
        self.autoencoder = autoencoder


@pytest.mark.parametrize("kind", ["ae_64x8x8_lin.enc", "ae_vit.tokens", "ae_gan.convautoencoder"])
def test_enable_cache_refuses_every_kind_but_autoencoder_kl(kind):
    prov = Autoencoder(128, kind, {"latent_dim": 64})
    with pytest.raises(WfaeError, match="batch size") as e:
        prov.enable_cache(16)
    assert kind in str(e.value) and "autoencoder_kl" in str(e.value)
    assert prov.cache is None
    with pytest.raises(WfaeError, match="batch size"):
        _runner.enable_latent_cache(Tiny(prov), SEVIRFrameLoader(events(2, 7), 1), 16)


def test_the_flag_is_refused_with_augmentation_and_without_a_provider(monkeypatch):
    prov = kl_provider()
    assert prov.cache is None
    ev = events(2, 7)
    with pytest.raises(WfaeError, match="aug_mode"):
        _runner.enable_latent_cache(Tiny(prov), SEVIRFrameLoader(ev, 1, aug_mode="1"), 16)
    assert prov.cache is None
    sharded = _runner.RankShard(SequenceBatchLoader(ev, None, 1, 3, 2, "NTHW", aug_mode="2"), 2, 0)
    with pytest.raises(WfaeError, match="aug_mode"):
        _runner.enable_latent_cache(Tiny(prov), sharded, 16)
    cache = _runner.enable_latent_cache(Tiny(prov), SEVIRFrameLoader(ev, 1), 16)
    assert cache is prov.cache and cache.capacity == 16 and cache.table is None
    # ae_gan trains its own autoencoder: there is no frozen provider whose latents could be kept
    from tests.test_ae_gan_cpu import config
    from weatherforecastingtoolkit_amd.experiments.v1_experiments import _ae_gan as M
    monkeypatch.setattr(M, "ConvAutoencoderBIG", lambda latent_dim: M.ResidualBlock(1, 2, 2))   # no 207 M parameters
    with pytest.raises(WfaeError, match="no frozen latent provider"):
        _runner.enable_latent_cache(M.Model(config()), SEVIRFrameLoader(ev, 1), 16)
    with pytest.raises(WfaeError, match="no frozen latent provider"):
        _runner.enable_latent_cache(Tiny(None), SEVIRFrameLoader(ev, 1), 16)


def test_the_flag_is_refused_for_a_test_run():
    from weatherforecastingtoolkit_amd.experiments.v1_experiments.pretrained_ae_convae_sevir import train
    with pytest.raises(WfaeError, match="--mode test"):
        train.main(["--mode", "test", "--latent-cache", "8"])


def test_encode_refuses_ids_of_the_wrong_count():
    prov = kl_provider()
    prov.enable_cache(4)
    x = torch.zeros(1, 2, 1, 32, 32)
    with pytest.raises(WfaeError, match="3 frame ids for a batch of 1 x 2"):
        prov.encode(x, ids=("train", np.arange(3)))
    assert prov.cache.frames_cached == 0 and prov.cache.misses == 0


def test_ops_refuse_host_tensors():
    with pytest.raises(WfaeError, match="device tensors"):
        ops.latent_scatter(torch.zeros(2, 4), [0, 1], torch.zeros(2, 4))
    with pytest.raises(WfaeError, match="device tensors"):
        ops.latent_gather(torch.zeros(2, 4), None, [0, 1], (1, 2))


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_symbols_and_argument_validation():
    decls = _lib.parse_header()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("wfae_latent_scatter", "wfae_latent_gather"):
        assert name in decls and hasattr(raw, name)
        assert decls[name][2][-1] == "stream"
    assert decls["wfae_latent_scatter"][2] == ["src", "slots", "table", "M", "L", "capacity", "stream"]
    assert decls["wfae_latent_gather"][2] == ["table", "fresh", "index", "noise", "out", "B", "T", "L", "mode", "capacity",
                                             "M", "stream"]
    lib = _lib.load()
    assert lib.wfae_version() == 103
    p = 0x7F0000000000                 # never dereferenced: every call below is refused before a launch
    sc, ga = lib.wfae_latent_scatter, lib.wfae_latent_gather
    for args in [(None, p, p), (p, None, p), (p, p, None)]:
        assert sc(*args, 2, 4, 3, None) == -2 and b"null" in lib.wfae_last_error_string()
    for sizes in [(0, 4, 3), (2, 0, 3), (2, 4, 0), (-1, 4, 3)]:
        assert sc(p, p, p, *sizes, None) == -1 and b"bad shape" in lib.wfae_last_error_string()
    assert sc(p, p, p, 1 << 20, 1 << 19, 1, None) == -1 and b"too large" in lib.wfae_last_error_string()
    for args in [(None, p, p, None, p), (p, p, None, None, p), (p, p, p, None, None)]:
        assert ga(*args, 2, 3, 4, 0, 5, 1, None) == -2 and b"null" in lib.wfae_last_error_string()
    assert ga(p, None, p, None, p, 2, 3, 4, 0, 5, 1, None) == -2          # M fresh rows without fresh
    assert ga(p, p, p, None, p, 2, 3, 4, 1, 5, 1, None) == -2             # mode 1 without noise
    assert ga(p, p, p, p, p, 2, 3, 4, 0, 5, 1, None) == -2                # noise without mode 1
    for sizes in [(0, 3, 4, 0, 5, 1), (2, 0, 4, 0, 5, 1), (2, 3, 0, 0, 5, 1), (2, 3, 4, 0, 0, 1), (2, 3, 4, 0, 5, -1)]:
        assert ga(p, p, p, None, p, *sizes, None) == -1 and b"bad shape" in lib.wfae_last_error_string()
    for mode in (-1, 2):
        assert ga(p, p, p, p, p, 2, 3, 4, mode, 5, 1, None) == -1 and b"mode" in lib.wfae_last_error_string()
    assert ga(p, p, p, p, p, 2, 3, 5, 1, 5, 1, None) == -1 and b"odd" in lib.wfae_last_error_string()
    assert ga(p, None, p, None, p, 1 << 20, 1 << 10, 1 << 10, 0, 1, 0, None) == -1 and b"too large" in lib.wfae_last_error_string()
