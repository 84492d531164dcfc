"""GPU: the latent cache of the frozen AutoencoderKL provider (csrc/latent_cache.hip, `_latents.LatentCache`,
`--latent-cache`).  Everything here is held to bit equality: the kernels are copies (and, in mode 1, the expression of
`aekl_posterior_seq_kernel` on the copied operands), and a cached run computes on the bits an uncached run computes on,
because the missing frames are encoded in passes of exactly as many frames as the uncached encode uses: the encoder's GEMM
routes (K-split, tile size) are chosen from the row count of a pass, not from which frames are in it.  No tolerance appears
below.

The provider is tests/aekl_ref.CONFIGS["small"] on 32 x 32 frames: 8 x 8 = 64 tokens at the mid block, latents 4 x 8 x 8, so a
row is L = 256 values (the mode) or 512 (the moments).  Its mid block is 64 wide, where the K-split of the attention's
projections is the same for every pass size; `WIDE` below (mid block 512 wide on 128 x 128 frames: 256 tokens, the ae_s2
mid block) is where the split count follows the pass size: 2 splits for 104 frames, 3 for 13, 6 for 6, 32 for one.
"""
from __future__ import annotations

import json
import os

import numpy as np
import pytest
import torch

from tests import aekl_ref as A
from tests.test_ae_s2_gpu import OVER as S2_OVER
from tests.test_ae_s2_gpu import _offset, last_ckpt
from weatherforecastingtoolkit_amd import config as C
from weatherforecastingtoolkit_amd import ops
from weatherforecastingtoolkit_amd._lib import WfaeError
from weatherforecastingtoolkit_amd.experiments.ae_s2 import train as ae_s2
from weatherforecastingtoolkit_amd.experiments.v1_experiments._latents import Autoencoder

pytestmark = pytest.mark.gpu

SENTINEL = -7.5

# (L, element offset of the float buffers).  1 and 6: the scalar path, a row of 6 is 24 bytes, so rows are not 16-byte aligned;
# 256: the 16-byte path inside one block; 4100: the 16-byte path over 17 blocks with rows of 16400 bytes; 4100 off 16-byte
# alignment: the scalar path over 65 blocks although L % 4 == 0
ROWS = [(1, 0), (6, 0), (256, 0), (4100, 0), (4100, 1)]
# capacity -> (scatter slots, gather index over table and fresh (3 rows) with a repeated row, gather index when all hit)
CASES = {1: ([-1, 0, -1], [0, -2, 0, -1, -3, 0], [0, 0, 0, 0, 0, 0]),
         5: ([3, -1, 0, 4], [2, -1, 2, -3, 4, 0], [4, 4, 1, 0, 3, 2])}


def rand(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("capacity", [1, 5])
@pytest.mark.parametrize("row", ROWS, ids=lambda r: f"L{r[0]}off{r[1]}")
def test_scatter_against_torch_indexing(dev, row, capacity):
    l, off = row
    slots = CASES[capacity][0]
    src = rand((len(slots), l), 1 + l)
    table = _offset(torch.full((capacity, l), SENTINEL), off, dev)
    want = torch.full((capacity, l), SENTINEL)
    for m, s in enumerate(slots):
        if s >= 0:
            want[s] = src[m]
    out = ops.latent_scatter(_offset(src, off, dev), slots, table)
    assert out is table and torch.equal(table.cpu(), want)
    untouched = [s for s in range(capacity) if s not in slots]
    assert all(bool((table[s] == SENTINEL).all()) for s in untouched) and (capacity == 1 or untouched)
    # the slots may come as an array or a host tensor; the rows land in the same place
    again = torch.full((capacity, l), SENTINEL, device=dev)
    ops.latent_scatter(src.to(dev), np.asarray(slots), again)
    ops.latent_scatter(src.to(dev), torch.tensor(slots), again)
    assert torch.equal(again.cpu(), want)


@pytest.mark.parametrize("capacity", [1, 5])
@pytest.mark.parametrize("row", ROWS, ids=lambda r: f"L{r[0]}off{r[1]}")
def test_gather_against_torch_indexing(dev, row, capacity):
    l, off = row
    _, mixed, hits = CASES[capacity]
    table, fresh = rand((capacity, l), 2 + l), rand((3, l), 3 + l)
    td, fd = _offset(table, off, dev), _offset(fresh, off, dev)
    want = torch.stack([table[i] if i >= 0 else fresh[-1 - i] for i in mixed]).view(2, 3, l)
    out = ops.latent_gather(td, fd, mixed, (2, 3))
    assert out.shape == (2, 3, l) and torch.equal(out.cpu(), want)
    # every frame in the table: no fresh rows at all
    out = ops.latent_gather(td, None, np.asarray(hits), (2, 3))
    assert torch.equal(out.cpu(), table[hits].view(2, 3, l))
    out = ops.latent_gather(td, None, hits, (3, 2))
    assert out.shape == (3, 2, l) and torch.equal(out.cpu(), table[hits].view(3, 2, l))


# (C, h, w): C h w = 256 and 6 as the 16-byte and the scalar case; 36 = 4 x 9: 16-byte here, scalar in aekl_posterior_seq
# (h w % 4 != 0), the same bits all the same
@pytest.mark.parametrize("capacity", [1, 5])
@pytest.mark.parametrize("chw", [(4, 8, 8), (3, 1, 2), (4, 3, 3)], ids=lambda s: "x".join(map(str, s)))
def test_gather_sample_is_the_sequence_posterior_bit_for_bit(dev, chw, capacity):
    c, h, w = chw
    n = c * h * w
    b, t = 2, 3
    _, mixed, hits = CASES[capacity]
    table, fresh = rand((capacity, 2 * n), 5 + n) * 4, rand((3, 2 * n), 6 + n) * 4
    for rows in (table, fresh):                  # log-variances at and beyond both clamps, first and last element
        rows[0, n:n + 4] = torch.tensor([-40.0, -30.0, 20.0, 40.0])
        rows[-1, -2:] = torch.tensor([40.0, -40.0])
    noise = rand((t, b, c, h, w), 7 + n).to(dev)
    td, fd = table.to(dev), fresh.to(dev)
    for index, fr in ((mixed, fd), (hits, None)):
        moments = torch.stack([table[i] if i >= 0 else fresh[-1 - i] for i in index]).view(b * t, 2 * c, h, w).to(dev)
        want = ops.aekl_posterior_seq(moments, noise)
        out = ops.latent_gather(td, fr, index, (b, t), noise)
        assert out.shape == (b, t, n) and torch.equal(out.view(b, t, c, h, w), want)
    assert bool(torch.isfinite(want).all())


def test_ops_refuse_bad_arguments(dev):
    src, table = torch.zeros(3, 8, device=dev), torch.zeros(4, 8, device=dev)
    with pytest.raises(WfaeError, match="outside"):
        ops.latent_scatter(src, [0, 4, 1], table)
    with pytest.raises(WfaeError, match="outside"):
        ops.latent_scatter(src, [0, -2, 1], table)
    with pytest.raises(WfaeError, match="share a slot"):
        ops.latent_scatter(src, [2, -1, 2], table)
    with pytest.raises(WfaeError, match="2 slots for 3 rows"):
        ops.latent_scatter(src, [0, 1], table)
    with pytest.raises(WfaeError, match="host copy"):
        ops.latent_scatter(src, torch.tensor([0, 1, 2], device=dev), table)
    with pytest.raises(WfaeError, match="expected src"):
        ops.latent_scatter(torch.zeros(3, 4, device=dev), [0, 1, 2], table)
    with pytest.raises(WfaeError, match="outside"):
        ops.latent_gather(table, src, [0, 4], (1, 2))
    with pytest.raises(WfaeError, match="outside"):
        ops.latent_gather(table, src, [0, -4], (1, 2))
    with pytest.raises(WfaeError, match="outside"):
        ops.latent_gather(table, None, [0, -1], (1, 2))
    with pytest.raises(WfaeError, match="3 indices for 1 x 2"):
        ops.latent_gather(table, None, [0, 1, 2], (1, 2))
    with pytest.raises(WfaeError, match="does not fit"):
        ops.latent_gather(table, None, [0, 1], (1, 2), torch.zeros(1, 2, 4, device=dev))
    with pytest.raises(WfaeError, match="fp32"):
        ops.latent_gather(table.double(), None, [0, 1], (1, 2))
    assert ops.latent_gather(table, None, [0, 1], (1, 2), torch.zeros(2, 1, 4, device=dev)).shape == (1, 2, 4)


# ------------------------------------------------------------------------------------------------ the provider
def provider(dev, sample=False, chunk=4):
    cfg = C.Cfg(dict(A.CONFIGS["small"], kind="autoencoder_kl", checkpoint=None, chunk_frames=chunk, seed=0, sample=sample))
    return Autoencoder(32, "autoencoder_kl", cfg).to(dev).eval()


@pytest.fixture(scope="module")
def pool(dev):
    """12 frames, frame i is the frame with id i"""
    return torch.rand(12, 1, 32, 32, generator=torch.Generator().manual_seed(11)).to(dev)


def batch(pool, ids):
    return pool[torch.as_tensor(ids, device=pool.device)].view(2, len(ids) // 2, 1, 32, 32).contiguous()


def refuse(*a, **k):
    raise AssertionError("the encoder ran on a batch whose every frame is cached")


def test_mode_provider_is_bit_equal_and_skips_the_encoder_on_hits(dev, pool, monkeypatch):
    plain, cached = provider(dev), provider(dev)
    cache = cached.enable_cache(16)
    first = list(range(8))
    want = plain.encode(batch(pool, first))
    assert want.shape == (2, 4, 4, 8, 8)
    got = cached.encode(batch(pool, first), ids=("train", np.asarray(first)))
    assert torch.equal(got, want)
    assert (cache.hits, cache.misses, cache.frames_cached, cache.bytes) == (0, 8, 8, 16 * 256 * 4)
    with monkeypatch.context() as m:
        m.setattr(cached.autoencoder, "encode", refuse)
        m.setattr(cached.autoencoder, "moments", refuse)
        assert torch.equal(cached.encode(batch(pool, first), ids=("train", np.asarray(first))), want)
    assert (cache.hits, cache.misses) == (8, 8)
    third = [9, 3, 0, 10, 7, 1, 11, 8]                      # seen and unseen frames, in another order
    got = cached.encode(batch(pool, third), ids=("train", np.asarray(third)))
    assert torch.equal(got, plain.encode(batch(pool, third)))
    assert (cache.hits, cache.misses, cache.frames_cached) == (12, 12, 12)
    # the same ids under another split are other frames; without ids the cache is not touched
    other = [i + 4 for i in first]
    got = cached.encode(batch(pool, other), ids=("val", np.asarray(first)))
    assert torch.equal(got, plain.encode(batch(pool, other))) and cache.misses == 20
    assert torch.equal(cached.encode(batch(pool, first)), want) and (cache.hits, cache.misses) == (12, 20)
    # a provider without a cache does not read ids
    assert torch.equal(plain.encode(batch(pool, first), ids=("train", np.arange(3))), want)


def test_a_full_table_stays_equal(dev, pool):
    plain, cached = provider(dev), provider(dev)
    cache = cached.enable_cache(3)
    ids = [5, 2, 8, 1, 0, 3, 9, 4]
    want = plain.encode(batch(pool, ids))
    for call in range(2):
        assert torch.equal(cached.encode(batch(pool, ids), ids=("train", np.asarray(ids))), want)
    assert (cache.frames_cached, cache.misses, cache.hits) == (3, 8 + 5, 3)
    assert cache.slot == {("train", 5): 0, ("train", 2): 1, ("train", 8): 2}


def test_a_frame_twice_in_one_batch_is_encoded_once(dev, pool):
    plain, cached = provider(dev), provider(dev)
    cached.enable_cache(16)
    ids = [0, 1, 2, 0, 4, 5, 6, 2]
    encoded = []
    inner = cached.autoencoder.encode
    cached.autoencoder.encode = lambda f: (encoded.append(f.shape[0]), inner(f))[1]
    try:
        got = cached.encode(batch(pool, ids), ids=("train", np.asarray(ids)))
    finally:
        del cached.autoencoder.encode
    assert encoded == [4, 4]            # six distinct frames in whole passes of chunk_frames = 4, the last one twice over
    want = plain.encode(batch(pool, ids))
    assert torch.equal(got, want) and torch.equal(got[0, 0], got[0, 3]) and torch.equal(got[0, 2], got[1, 3])


def test_batches_of_another_pass_size_go_around_the_cache(dev, pool):
    """chunk_frames 3 on 8 frames: passes of 3, 3, 2 frames — not one size, so nothing is cached; chunk_frames 0: the first
    batch sets the pass to 8 frames, a batch of 6 is a pass of another size"""
    plain, cached = provider(dev, chunk=3), provider(dev, chunk=3)
    cache = cached.enable_cache(16)
    ids = list(range(8))
    for _ in range(2):
        assert torch.equal(cached.encode(batch(pool, ids), ids=("train", np.asarray(ids))), plain.encode(batch(pool, ids)))
    assert (cache.bypassed, cache.misses, cache.hits, cache.frames_cached) == (16, 0, 0, 0)
    plain, cached = provider(dev, chunk=0), provider(dev, chunk=0)
    cache = cached.enable_cache(16)
    assert torch.equal(cached.encode(batch(pool, ids), ids=("train", np.asarray(ids))), plain.encode(batch(pool, ids)))
    short = [2, 9, 4, 10, 0, 11]
    assert torch.equal(cached.encode(batch(pool, short), ids=("train", np.asarray(short))), plain.encode(batch(pool, short)))
    assert (cache.bypassed, cache.misses, cache.frames_cached, cache.pass_frames) == (6, 8, 8, {"train": 8})
    # another split has its own pass size
    assert torch.equal(cached.encode(batch(pool, short), ids=("val", np.asarray(short))), plain.encode(batch(pool, short)))
    assert (cache.bypassed, cache.misses, cache.pass_frames) == (6, 14, {"train": 8, "val": 6})


# the ae_s2 mid block (512 wide, 256 tokens on 128 x 128 frames) behind narrow outer blocks
WIDE = dict(A.CONFIGS["small"], down_block_types=("DownEncoderBlock2D",) * 4, up_block_types=("UpDecoderBlock2D",) * 4,
            block_out_channels=(32, 32, 64, 512))


@pytest.fixture(scope="module")
def wide_pool(dev):
    """123 frames of 128 x 128, frame i is the frame with id i"""
    return torch.rand(123, 1, 128, 128, generator=torch.Generator().manual_seed(12)).to(dev)


@pytest.mark.parametrize("sample,chunk", [(True, 0), (False, 8)], ids=["sampled-one-pass", "mode-chunks-of-8"])
def test_partial_misses_where_the_gemm_split_follows_the_pass_size(dev, wide_pool, sample, chunk):
    """B T = 104 frames as in ae_s2.  After a batch that fills the cache, batches of the same 104 slots with 13, 5 and 1
    frames replaced by unseen ones — partial misses — and the table (110 rows) running full in the middle of the first of
    them.  Every batch equals the uncached encode of the same frames bit for bit, and stays equal when it hits."""
    def make():
        cfg = C.Cfg(dict(WIDE, kind="autoencoder_kl", checkpoint=None, chunk_frames=chunk, seed=0, sample=sample))
        return Autoencoder(128, "autoencoder_kl", cfg).to(dev).eval()
    plain, cached = make(), make()
    cache = cached.enable_cache(110)
    noise = torch.randn(13, 8, 4, 16, 16, generator=torch.Generator().manual_seed(4)).to(dev) if sample else None

    def both(ids):
        x = wide_pool[torch.as_tensor(ids, device=dev)].view(8, 13, 1, 128, 128).contiguous()
        want = plain.encode(x, noise=noise)
        for _ in range(2):
            assert torch.equal(cached.encode(x, noise=noise, ids=("train", np.asarray(ids))), want)
        return want

    base = list(range(104))
    want = both(base)
    assert want.shape == (8, 13, 4, 16, 16)
    # what the pass size does at this width: the same frame alone in a pass (informative: printed, not asserted)
    x0 = wide_pool[:1].view(1, 1, 1, 128, 128)
    alone = plain.encode(x0, noise=None if noise is None else noise[:1, :1].contiguous())
    print(f"frame 0 alone in a pass equals its latent in the pass of {chunk or 104}: {torch.equal(alone[0, 0], want[0, 0])}")
    order = torch.randperm(104, generator=torch.Generator().manual_seed(5)).tolist()
    new = 104
    for n_new in (13, 5, 1):
        ids = [base[i] for i in order]
        for j in range(n_new):
            ids[7 * j + 3] = new + j                    # unseen frames spread over the batch
        new += n_new
        misses = cache.misses
        both(ids)
        # 13: six get the last slots, seven stay fresh and miss again on the second call; 5 and 1: the table is full
        assert cache.misses - misses == (13 + 7 if n_new == 13 else 2 * n_new)
    assert (cache.frames_cached, cache.bypassed) == (110, 0)


@pytest.mark.parametrize("chunk", [0, 4])
def test_sampled_provider_is_bit_equal_and_moves_the_generator_alike(dev, pool, monkeypatch, chunk):
    plain, cached = provider(dev, True, chunk), provider(dev, True, chunk)
    cache = cached.enable_cache(16)
    ga, gb = torch.Generator(device=dev).manual_seed(5), torch.Generator(device=dev).manual_seed(5)
    ids = [3, 1, 4, 1, 5, 9, 2, 6]
    x = batch(pool, ids)
    z_miss, want_miss = cached.encode(x, generator=ga, ids=("train", np.asarray(ids))), plain.encode(x, generator=gb)
    assert z_miss.shape == (2, 4, 4, 8, 8) and torch.equal(z_miss, want_miss)
    assert torch.equal(ga.get_state(), gb.get_state())
    assert (cache.misses, cache.frames_cached, cache.bytes) == (7, 7, 16 * 512 * 4)
    with monkeypatch.context() as m:
        m.setattr(cached.autoencoder, "encode", refuse)
        m.setattr(cached.autoencoder, "moments", refuse)
        z_hit = cached.encode(x, generator=ga, ids=("train", np.asarray(ids)))
    want_hit = plain.encode(x, generator=gb)
    assert torch.equal(z_hit, want_hit) and not torch.equal(z_hit, z_miss)          # fresh noise on cached moments
    assert torch.equal(ga.get_state(), gb.get_state())
    # given noise replaces the draw on both paths
    noise = torch.randn(4, 2, 4, 8, 8, generator=torch.Generator().manual_seed(3)).to(dev)
    assert torch.equal(cached.encode(x, noise=noise, ids=("train", np.asarray(ids))), plain.encode(x, noise=noise))
    with pytest.raises(WfaeError, match="noise"):
        cached.encode(x, noise=noise[:3].contiguous(), ids=("train", np.asarray(ids)))


# ------------------------------------------------------------------------------------------------ the driver
def same(a, b, path="ckpt"):
    """every tensor under a and b bitwise equal, every other leaf equal"""
    if isinstance(a, torch.Tensor):
        assert isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b), path
        return 1
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), path
        return sum(same(a[key], b[key], f"{path}.{key}") for key in a)
    if isinstance(a, (list, tuple)):
        assert isinstance(b, (list, tuple)) and len(a) == len(b), path
        return sum(same(x, y, f"{path}[{i}]") for i, (x, y) in enumerate(zip(a, b)))
    assert a == b, path
    return 0


def run_main(main, capsys, argv):
    """-> (the JSON lines of the run, every line)"""
    capsys.readouterr()
    assert main(argv) == 0
    out = capsys.readouterr().out.splitlines()
    print("\n".join(out))
    assert out and out[-1] == "done"
    return [json.loads(line) for line in out if line.startswith("{")], out


def compare_runs(plain, cached, rate):
    """the JSON lines of the two runs: the cached one has the latent_cache line in front of `done` and nothing else differs
    but the throughput -> the latent_cache record"""
    assert not any("latent_cache" in log for log in plain)
    assert "latent_cache" in cached[-1] and not any("latent_cache" in log for log in cached[:-1])
    assert len(plain) == len(cached) - 1
    for x, y in zip(plain, cached):
        assert list(x) == list(y)
        for key in x:
            assert key == rate or x[key] == y[key], (key, x, y)
    return cached[-1]["latent_cache"]


def test_ae_s2_run_is_bit_equal_with_the_cache(dev, tmp_path, capsys):
    """synthetic events: 4 events x 25 frames, sequences of 13 every 6 frames (starts 0, 6, 12: every frame of an event is in
    one), 12 sequences, 6 batches of 2 an epoch.  13 steps walk the loader twice and start a third pass.  Two sequences of
    one event in a batch share frames: those are encoded once"""
    common = ["--max-steps", "13", "--no-test", *S2_OVER]
    plain, _ = run_main(ae_s2.main, capsys, [*common, f"experiment_path={tmp_path / 'plain'}"])
    cached, out = run_main(ae_s2.main, capsys, [*common, "--latent-cache", "4096", f"experiment_path={tmp_path / 'cached'}"])
    assert out[-2].startswith('{"latent_cache"')
    assert [log["step"] for log in plain] == list(range(1, 14))
    assert len({log["train_loss"] for log in plain}) == 13
    stats = compare_runs(plain, cached, "sequences_per_s")
    assert stats == {"hits": 13 * 26 - 100, "misses": 100, "frames_cached": 100, "capacity": 4096,
                     "MiB": 4096 * 2 * 4 * 32 * 32 * 4 / 2 ** 20, "bypassed": 0}
    a, b = last_ckpt(tmp_path / "plain"), last_ckpt(tmp_path / "cached")
    assert a["global_step"] == 13 and list(a) == list(b)           # the cache is not part of the checkpoint
    assert same(a["state_dict"], b["state_dict"]) == 3 * 4096 * 2
    assert same(a["optimizer_states"], b["optimizer_states"]) >= 2
    assert same(a["rng"], b["rng"]) >= 2                            # the noise generator moved alike
    same(a["lr_schedulers"], b["lr_schedulers"])


CONVAE_OVER = ["autoencoder.block_out_channels=[32,32,64,64]", "autoencoder.layers_per_block=1", "autoencoder.norm_num_groups=8",
               "dataset.batch_size=4", "trainer.log_every_n_steps=1"]


def test_convae_run_on_the_datamodule_path_is_bit_equal_with_the_cache(dev, tmp_path, capsys):
    """pretrained_ae_convae_sevir with config_autoencoder_kl.yaml (`sample: false`) on a store of 384 x 384 events of 8
    frames: five before 2019-06-01 = 40 single-frame sequences through SEVIRLightningDataModule, split 36 / 4; 9 training
    batches of 4 (one encoder pass of chunk_frames = 4 each) an epoch in a fresh order every epoch, one validation batch
    after each epoch and after the last step.  19 steps = two epochs and one batch; three validation passes over the same 4
    frames"""
    from tests.test_v1_run_cpu import STAMPS, write_store
    from weatherforecastingtoolkit_amd.experiments.v1_experiments.pretrained_ae_convae_sevir import train
    store = str(tmp_path / "sevir")
    write_store(store, STAMPS, shape=(384, 384, 8))
    common = ["--config", os.path.join(train.HERE, "config_autoencoder_kl.yaml"), "--data-dir", store, "--max-steps", "19",
              *CONVAE_OVER]
    plain, _ = run_main(train.main, capsys, [*common, f"experiment_path={tmp_path / 'plain'}"])
    cached, _ = run_main(train.main, capsys, [*common, "--latent-cache", "64", f"experiment_path={tmp_path / 'cached'}"])
    assert [log["step"] for log in plain if "train_loss" in log] == list(range(1, 20))
    assert sum("val_loss" in log for log in plain) == 3
    stats = compare_runs(plain, cached, "frames_per_s")
    assert stats == {"hits": 19 * 4 + 3 * 4 - 40, "misses": 40, "frames_cached": 40, "capacity": 64,
                     "MiB": 64 * 4 * 48 * 48 * 4 / 2 ** 20, "bypassed": 0}

    def ckpt(name):
        return torch.load(os.path.join(str(tmp_path / name), "outputs", "pretrained_ae_convae_sevir", "checkpoints", "last.ckpt"),
                          map_location="cpu", weights_only=False)
    a, b = ckpt("plain"), ckpt("cached")
    assert a["global_step"] == 19 and list(a) == list(b)
    assert same(a["state_dict"], b["state_dict"]) >= 4
    assert same(a["optimizer_states"], b["optimizer_states"]) >= 2
