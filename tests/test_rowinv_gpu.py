"""GPU: the pass-invariant frozen AutoencoderKL (csrc/linear_rowinv.hip, `AutoencoderKL.pass_invariant`, the provider's
`pass_invariant`, `--invariant-encode`).

The claim is about bits: the result for a row (a token, a frame) does not depend on what shares its call.  So every
comparison below is torch.equal, with two exceptions that are accuracy checks and carry their bound with them:
  * the kernel against the float64 product, |err| <= (In + 1) 2^-24 (sum_k |x_k w_k| + |bias|): the first-order bound of
    one fp32 accumulator chain of In products plus the bias add, In + 1 roundings (at 'medium' on bf16-rounded operands);
  * the pass-invariant model against the recorded fp64 values and the attention block against torch in fp64, with the bars
    of tests/test_aekl_gpu.py (max(4 x spread, 2e-6)).
Shapes: In = Out = 512 with 64 tokens a frame is where the default kernel's K-split follows the pass size (32 splits for one
frame, 16 for 5, 8 for 13, 2 for 104); (32, 96) has one k-stage pair and a masked column tile, (2048, 64) a long chain and a
single column tile; 832 rows are 13 row tiles, rows [3:100] start and end inside a tile, row 777 is B = 1."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import weatherforecastingtoolkit_amd as pkg
from tests import aekl_ref as A
from tests import convae_ref as R
from tests.test_ae_s2_gpu import OVER as S2_OVER
from tests.test_ae_s2_gpu import _offset, last_ckpt
from tests.test_aekl_gpu import G14, check_fixture, golden_input, golden_model, rel, rnd, tol
from tests.test_latent_cache_gpu import WIDE, compare_runs, refuse, run_main, same
from weatherforecastingtoolkit_amd import config as C
from weatherforecastingtoolkit_amd import functional as Fn
from weatherforecastingtoolkit_amd import ops
from weatherforecastingtoolkit_amd._lib import WfaeError
from weatherforecastingtoolkit_amd.experiments.ae_s2 import train as ae_s2
from weatherforecastingtoolkit_amd.experiments.v1_experiments._latents import Autoencoder
from weatherforecastingtoolkit_amd.pipeline.models.autoencoderkl import AutoencoderKL

pytestmark = pytest.mark.gpu

SHAPES = [(512, 512), (32, 96), (2048, 64)]
ROWS = 832
PARTS = [(0, 64), (320, 384), (777, 778), (3, 100)]


@pytest.fixture(params=["highest", "medium"])
def precision(request, dev):
    pkg.set_float32_matmul_precision(request.param)
    try:
        yield request.param
    finally:
        pkg.set_float32_matmul_precision("highest")


def operands(inf, out, rows=ROWS):
    g = torch.Generator().manual_seed(inf + out)
    x = torch.randn(rows, inf, generator=g)
    w = torch.randn(out, inf, generator=g) * inf ** -0.5
    return x, w, torch.randn(out, generator=g)


# ------------------------------------------------------------------------------------------------ T1, T2, T3: the kernel
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_row_does_not_depend_on_its_call(dev, precision, shape):
    """T1.  Y of 832 rows in one call; the rows [0:64], [320:384], 777 alone and [3:100] in calls of their own are the same
    bits, from 16-byte aligned operands and from operands one element off (the scalar-load path), and the two agree"""
    inf, out = shape
    x, w, bias = operands(inf, out)
    whole = {}
    for off in (0, 1):
        xd, wd, bd = _offset(x, off, dev), _offset(w, off, dev), _offset(bias, off, dev)
        assert xd.data_ptr() % 16 == 4 * off and wd.data_ptr() % 16 == 4 * off
        y = ops.linear_fwd_rowinv(xd, wd, bd)
        assert y.shape == (ROWS, out) and bool(torch.isfinite(y).all())
        for lo, hi in PARTS:
            part = ops.linear_fwd_rowinv(xd[lo:hi], wd, bd)
            assert part.shape == (hi - lo, out) and torch.equal(part, y[lo:hi]), (off, lo, hi)
        # the rows in another order and next to other rows
        perm = torch.randperm(ROWS, generator=torch.Generator().manual_seed(3))[:200].to(dev)
        assert torch.equal(ops.linear_fwd_rowinv(xd[perm].contiguous(), wd, bd), y[perm])
        assert torch.equal(ops.linear_fwd_rowinv(xd, wd, bd), y)                   # and twice the same
        whole[off] = y
    assert torch.equal(whole[0], whole[1])
    # a part off alignment against the aligned whole: row 777 again, B = 1
    assert torch.equal(ops.linear_fwd_rowinv(_offset(x[777:778], 1, dev), w.to(dev), bias.to(dev)), whole[0][777:778])


def chain_bound(x64, w64, bias64, inf):
    mag = x64.abs() @ w64.abs().t()
    if bias64 is not None:
        mag = mag + bias64.abs()
    return (inf + 1) * 2.0 ** -24 * mag


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_element_is_within_one_fp32_chain_of_fp64(dev, precision, shape, with_bias):
    """T2"""
    inf, out = shape
    x, w, bias = operands(inf, out, rows=197)                   # three full row tiles and five rows of a fourth
    if not with_bias:
        bias = None
    y = ops.linear_fwd_rowinv(x.to(dev), w.to(dev), None if bias is None else bias.to(dev)).cpu().double()
    if precision == "medium":
        x, w = x.bfloat16().float(), w.bfloat16().float()       # round to nearest even, as the kernel rounds its fragments
    x64, w64, b64 = x.double(), w.double(), None if bias is None else bias.double()
    want = x64 @ w64.t() + (0 if b64 is None else b64)
    err, bound = (y - want).abs(), chain_bound(x64, w64, b64, inf)
    print(f"{precision} {inf}x{out} bias={with_bias}: max err / bound {float((err / bound).max()):.3f}, "
          f"max |err| {float(err.max()):.3e}")
    assert bool((err <= bound).all())


def test_many_row_tiles_and_the_relation_to_linear_fwd(dev):
    """T3.  B = 16384, In = Out = 512: 256 row tiles x 8 column tiles.  Rows of the first and the last tiles are the bits
    of the same rows in a call of their own and meet T2's bound.  Informative, printed and not asserted: whether
    wfae_linear_fwd gives these bits, with and without the three-plane split, here (where it takes two K-splits) and at
    B = 32768 (where it takes one); DESIGN.md §4 has the outcome"""
    inf = out = 512
    x, w, bias = operands(inf, out, rows=16384)
    xd, wd, bd = x.to(dev), w.to(dev), bias.to(dev)
    y = ops.linear_fwd_rowinv(xd, wd, bd)
    for lo, hi in [(0, 64), (16384 - 70, 16384)]:
        assert torch.equal(ops.linear_fwd_rowinv(xd[lo:hi], wd, bd), y[lo:hi])
        x64, w64, b64 = x[lo:hi].double(), w.double(), bias.double()
        err = (y[lo:hi].cpu().double() - (x64 @ w64.t() + b64)).abs()
        assert bool((err <= chain_bound(x64, w64, b64, inf)).all())
    x2 = torch.cat([xd, xd.flip(0)])
    y2 = ops.linear_fwd_rowinv(x2, wd, bd)
    assert torch.equal(y2[:16384], y) and torch.equal(y2[16384:], y.flip(0))
    was = ops.split_gemm_enabled()
    try:
        for split in (True, False):
            ops.set_split_gemm(split)
            for xin, yin in ((xd, y), (x2, y2)):
                ref = ops.linear_fwd(xin, wd, bd)
                print(f"linear_fwd with split_gemm {split} gives the bits of linear_fwd_rowinv at B = {xin.shape[0]}: "
                      f"{torch.equal(ref, yin)}; max |difference| {float((ref - yin).abs().max()):.3e}")
    finally:
        ops.set_split_gemm(was)


def test_wrapper_refusals(dev):
    x, w = torch.zeros(4, 64, device=dev), torch.zeros(32, 64, device=dev)
    with pytest.raises(WfaeError, match="fp32"):
        ops.linear_fwd_rowinv(x.double(), w.double())
    with pytest.raises(WfaeError, match="contiguous"):
        ops.linear_fwd_rowinv(torch.zeros(4, 128, device=dev)[:, ::2], w)
    with pytest.raises(WfaeError, match="expected x"):
        ops.linear_fwd_rowinv(x, torch.zeros(32, 32, device=dev))
    with pytest.raises(WfaeError, match="expected x"):
        ops.linear_fwd_rowinv(x, w, torch.zeros(64, device=dev))
    with pytest.raises(WfaeError, match="multiples of 32"):
        ops.linear_fwd_rowinv(torch.zeros(4, 48, device=dev), torch.zeros(32, 48, device=dev))
    assert ops.linear_fwd_rowinv(x, w).shape == (4, 32)


# ------------------------------------------------------------------------------------------------ T4: the whole model
# WIDE with ResNet shortcuts of 128 and 256 input channels: on 128 x 128 frames the 128 -> 256 shortcut of the encoder has 1024
# pixels a frame, and gemm.hip's 1x1 forward takes the fp32 matrix instruction below 16 frames and the three-plane split
# from 16 on (launch_gemm_v: pick_bm(256, 8 frames) >= 64)
SHORTCUTS = dict(WIDE, block_out_channels=(32, 128, 256, 512))


def wide_model(dev, invariant, geometry=WIDE):
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        model = AutoencoderKL(**geometry)
    return model.to(dev).pass_invariant(invariant)


@pytest.mark.parametrize("geometry,size", [(WIDE, 64), (SHORTCUTS, 128)], ids=["wide-64", "shortcuts-128"])
def test_a_frame_is_the_same_bits_in_every_pass(dev, geometry, size):
    """T4.  WIDE on 64 x 64 frames: 64 tokens at a 512-wide mid block, where the K-split of the default projections follows
    the pass size; SHORTCUTS on 128 x 128 frames, where the instruction of the default 1x1 shortcut convolutions does.  The
    moments, the mode and the decoded frame of frame 0 alone, and in passes of 2, 5, 13 and 26 frames at different
    positions"""
    pool = torch.rand(27, 1, size, size, generator=torch.Generator().manual_seed(21)).to(dev)
    model, default = wide_model(dev, True, geometry), wide_model(dev, False, geometry)
    x0 = pool[:1]
    others = pool[1:]
    m0 = model.moments(x0)
    z0 = model.encode(x0).mode()
    d0 = model.decode(z0)
    assert m0.shape == (1, 8, size // 8, size // 8) and z0.shape == (1, 4, size // 8, size // 8) and d0.shape == (1, 1, size, size)
    zs = model.encode(others).mode()
    dm0, dd0 = default.moments(x0), default.decode(z0)
    differs = []
    for n, pos in [(2, 1), (5, 0), (5, 3), (13, 12), (13, 6), (26, 17)]:
        x = torch.cat([others[:pos], x0, others[pos:n - 1]])
        assert x.shape[0] == n
        assert torch.equal(model.moments(x)[pos:pos + 1], m0), (n, pos)
        assert torch.equal(model.encode(x).mode()[pos:pos + 1], z0), (n, pos)
        z = torch.cat([zs[:pos], z0, zs[pos:n - 1]])
        assert torch.equal(model.decode(z)[pos:pos + 1], d0), (n, pos)
        differs.append((n, pos, not torch.equal(default.moments(x)[pos:pos + 1], dm0),
                        not torch.equal(default.decode(z)[pos:pos + 1], dd0)))
    # informative, not asserted: that the default mode differs here is what gives the assertions above their teeth
    print("default mode, (frames, position, moments differ from the frame alone, decode differs): ", differs)
    print(f"pass-invariant against default moments of the frame alone: max |difference| {float((dm0 - m0).abs().max()):.3e} "
          f"at max |value| {float(dm0.abs().max()):.3e}")


# ------------------------------------------------------------------------------------------------ T5: still the right answer
@pytest.mark.parametrize("p", ["a", "b", "c"])
def test_golden_parity_in_pass_invariant_mode(dev, p):
    g14 = np.load(G14, allow_pickle=False)
    model = golden_model(g14, p, dev).pass_invariant()
    x = golden_input(g14, p).to(dev)
    noise = torch.from_numpy(g14[f"{p}_noise"]).to(dev)
    post = model.encode(x)
    bad = []
    check_fixture(g14, f"{p}_mean", post.mean, bad)
    check_fixture(g14, f"{p}_logvar", post.logvar, bad)
    check_fixture(g14, f"{p}_mode", post.mode(), bad)
    check_fixture(g14, f"{p}_draw", post.sample(noise=noise), bad)
    check_fixture(g14, f"{p}_decode", model.decode(post.mode()), bad)
    assert not bad, bad


@pytest.mark.parametrize("n,c,h,w,groups", [(2, 64, 16, 16, 8), (1, 512, 16, 16, 32), (1, 512, 48, 48, 32)],
                         ids=["S256-C64", "S256-C512", "S2304-C512"])
def test_attention_block_row_invariant(dev, n, c, h, w, groups):
    """the cases, the inputs and the bar of tests/test_aekl_gpu.py::test_attention_block"""
    g = torch.Generator().manual_seed(c + h)
    p = "a"
    sd = {f"{p}.group_norm.weight": rnd((c,), 1, 0.5, 1.5), f"{p}.group_norm.bias": rnd((c,), 2)}
    for i, nm in enumerate(("query", "key", "value", "proj_attn")):
        sd[f"{p}.{nm}.weight"] = torch.randn(c, c, generator=g) * c ** -0.5 * (2.0 if i < 2 else 1.0)
        sd[f"{p}.{nm}.bias"] = rnd((c,), 10 + i)
    x = torch.randn(n, c, h, w, generator=g)
    d = {k: v.to(dev) for k, v in sd.items()}
    xd = x.to(dev)
    gn = ops.aekl_gn_stats(xd, d[f"{p}.group_norm.weight"], d[f"{p}.group_norm.bias"], groups)[2:]
    args = [d[f"{p}.{nm}.{wb}"] for nm in ("query", "key", "value", "proj_attn") for wb in ("weight", "bias")]
    y = Fn.aekl_attention(xd, gn, *args, row_invariant=True)
    o64 = A.attention(A.cast(sd, torch.float64), p, x.double(), groups)
    o32 = A.attention(sd, p, x, groups)
    bound, err = tol(R.spread(o32, o64)), rel(y, o64)
    print(f"err {err:.3e} tol {bound:.3e}")
    assert err <= bound
    if n > 1:       # a sample alone is the same bits
        gn1 = tuple(t[1:2].contiguous() for t in gn)
        assert torch.equal(Fn.aekl_attention(xd[1:2], gn1, *args, row_invariant=True), y[1:2])


# ------------------------------------------------------------------------------------------------ T6: the compact cache
def provider(dev, sample=False, chunk=4, invariant=True, geometry=None, size=32):
    cfg = C.Cfg(dict(geometry or A.CONFIGS["small"], kind="autoencoder_kl", checkpoint=None, chunk_frames=chunk, seed=0,
                     sample=sample, pass_invariant=invariant))
    return Autoencoder(size, "autoencoder_kl", cfg).to(dev).eval()


class spy:
    """records the number of frames of every encoder pass of a provider"""

    def __init__(self, prov):
        self.ae, self.sizes = prov.autoencoder, []
        self.name = "moments" if prov.sample else "encode"

    def __enter__(self):
        inner = getattr(self.ae, self.name)
        setattr(self.ae, self.name, lambda f: (self.sizes.append(f.shape[0]), inner(f))[1])
        return self.sizes

    def __exit__(self, *exc):
        delattr(self.ae, self.name)


@pytest.fixture(scope="module")
def pool(dev):
    """14 frames, frame i is the frame with id i"""
    return torch.rand(14, 1, 32, 32, generator=torch.Generator().manual_seed(11)).to(dev)


def batch(pool, ids, b=2):
    return pool[torch.as_tensor(ids, device=pool.device)].view(b, len(ids) // b, 1, 32, 32).contiguous()


def test_cache_encodes_six_missing_frames_in_passes_of_four_and_two(dev, pool):
    plain, cached = provider(dev), provider(dev)
    cache = cached.enable_cache(16)
    ids = [0, 1, 2, 0, 4, 5, 6, 2]
    with spy(cached) as sizes:
        got = cached.encode(batch(pool, ids), ids=("train", np.asarray(ids)))
    assert sizes == [4, 2]
    assert torch.equal(got, plain.encode(batch(pool, ids)))
    assert (cache.hits, cache.misses, cache.frames_cached, cache.bypassed) == (2, 6, 6, 0)


def test_cache_encodes_one_missing_frame_of_eight_alone(dev, pool, monkeypatch):
    plain, cached = provider(dev, chunk=0), provider(dev, chunk=0)
    cache = cached.enable_cache(16)
    first, second = list(range(8)), [0, 1, 2, 3, 4, 9, 6, 7]
    with spy(cached) as sizes:
        assert torch.equal(cached.encode(batch(pool, first), ids=("train", np.asarray(first))), plain.encode(batch(pool, first)))
        assert torch.equal(cached.encode(batch(pool, second), ids=("train", np.asarray(second))),
                           plain.encode(batch(pool, second)))
    assert sizes == [8, 1]
    with monkeypatch.context() as m:
        m.setattr(cached.autoencoder, "encode", refuse)
        m.setattr(cached.autoencoder, "moments", refuse)
        assert torch.equal(cached.encode(batch(pool, second), ids=("train", np.asarray(second))), plain.encode(batch(pool, second)))
    assert (cache.hits, cache.misses, cache.frames_cached, cache.bypassed) == (7 + 8, 9, 9, 0)


@pytest.mark.parametrize("sample", [False, True], ids=["mode", "sampled"])
def test_a_short_batch_after_a_full_one_is_served(dev, pool, sample):
    plain, cached = provider(dev, sample, chunk=4), provider(dev, sample, chunk=4)
    cache = cached.enable_cache(16)
    full, short = list(range(8)), [2, 9, 4, 10, 0, 11]              # 6 frames: a pass of 4 and a tail of 2 when uncached
    noise = torch.randn(4, 2, 4, 8, 8, generator=torch.Generator().manual_seed(3)).to(dev) if sample else None
    kw = lambda t: {} if noise is None else {"noise": noise[:t].contiguous()}     # noqa: E731
    with spy(cached) as sizes:
        assert torch.equal(cached.encode(batch(pool, full), ids=("train", np.asarray(full)), **kw(4)),
                           plain.encode(batch(pool, full), **kw(4)))
        want = plain.encode(batch(pool, short), **kw(3))
        assert torch.equal(cached.encode(batch(pool, short), ids=("train", np.asarray(short)), **kw(3)), want)
        assert sizes == [4, 4, 3]                                   # the three unseen frames of the short batch
        assert torch.equal(cached.encode(batch(pool, short), ids=("train", np.asarray(short)), **kw(3)), want)
        assert sizes == [4, 4, 3]                                   # it hits the second time
    assert (cache.bypassed, cache.hits, cache.misses, cache.frames_cached) == (0, 3 + 6, 11, 11)
    assert cache.pass_frames == {}


def test_a_full_table_charges_later_misses_their_own_frames(dev, pool):
    plain, cached = provider(dev), provider(dev)
    cache = cached.enable_cache(3)
    ids = [5, 2, 8, 1, 0, 3, 9, 4]
    want = plain.encode(batch(pool, ids))
    with spy(cached) as sizes:
        for _ in range(2):
            assert torch.equal(cached.encode(batch(pool, ids), ids=("train", np.asarray(ids))), want)
    assert sizes == [4, 4, 4, 1]                                    # 8 misses, then the 5 frames that found no slot
    assert (cache.frames_cached, cache.misses, cache.hits, cache.bypassed) == (3, 8 + 5, 3, 0)
    later = [5, 12, 2, 13]
    with spy(cached) as sizes:
        assert torch.equal(cached.encode(batch(pool, later), ids=("train", np.asarray(later))), plain.encode(batch(pool, later)))
    assert sizes == [2]


# ------------------------------------------------------------------------------------------------ T7: the ae_s2 width
@pytest.fixture(scope="module")
def wide_pool(dev):
    """123 frames of 128 x 128, frame i is the frame with id i"""
    return torch.rand(123, 1, 128, 128, generator=torch.Generator().manual_seed(12)).to(dev)


@pytest.mark.parametrize("sample,chunk,geometry", [(True, 0, WIDE), (False, 8, WIDE), (True, 0, SHORTCUTS)],
                         ids=["sampled-one-pass", "mode-chunks-of-8", "sampled-one-pass-shortcuts"])
def test_partial_misses_cost_their_own_frames_at_the_ae_s2_width(dev, wide_pool, sample, chunk, geometry):
    """T7.  B T = 104 frames as in ae_s2 (256 tokens at a 512-wide mid block).  After a batch that fills the cache, batches
    of the same 104 slots with 13, 5 and 1 frames replaced by unseen ones: the encoder sees 13, 5 and 1 frames, and every
    batch equals the uncached pass-invariant encode of the same frames, also when it hits.  With SHORTCUTS the pass of 104
    and the passes of 13, 5 and 1 are on either side of the size at which the default 1x1 convolutions change instruction"""
    plain = provider(dev, sample, chunk, geometry=geometry, size=128)
    cached = provider(dev, sample, chunk, geometry=geometry, size=128)
    cache = cached.enable_cache(130)
    noise = torch.randn(13, 8, 4, 16, 16, generator=torch.Generator().manual_seed(4)).to(dev) if sample else None

    def both(ids):
        x = wide_pool[torch.as_tensor(ids, device=dev)].view(8, 13, 1, 128, 128).contiguous()
        want = plain.encode(x, noise=noise)
        with spy(cached) as sizes:
            for _ in range(2):
                assert torch.equal(cached.encode(x, noise=noise, ids=("train", np.asarray(ids))), want)
        return list(sizes)

    base = list(range(104))
    assert both(base) == ([104] if chunk == 0 else [8] * 13)
    order = torch.randperm(104, generator=torch.Generator().manual_seed(5)).tolist()
    new = 104
    for n_new in (13, 5, 1):
        ids = [base[i] for i in order]
        for j in range(n_new):
            ids[7 * j + 3] = new + j                    # unseen frames spread over the batch
        new += n_new
        sizes = both(ids)
        assert sum(sizes) == n_new
        assert sizes == ([n_new] if chunk == 0 or n_new <= chunk else [8, 5])
    assert (cache.frames_cached, cache.misses, cache.bypassed) == (123, 123, 0)


# ------------------------------------------------------------------------------------------------ T8: a run
def test_ae_s2_run_with_a_short_last_batch_is_bit_equal_with_the_cache(dev, tmp_path, capsys):
    """a store of five 25-frame training events through the DataModule: 15 sequences of 13 frames, 10 % of them held out, in
    batches of 4 — the last training batch is short, and so is the validation batch.  9 steps: two epochs in two orders and
    one step of a third, a validation pass after each epoch and after the last step"""
    from tests.test_v1_run_cpu import STAMPS, write_store
    store = str(tmp_path / "sevir")
    write_store(store, STAMPS)
    over = [o for o in S2_OVER if not o.startswith("dataset.batch_size")] + ["dataset.batch_size=4"]
    common = ["--max-steps", "9", "--no-test", "--data-dir", store, "--invariant-encode", *over]
    plain, _ = run_main(ae_s2.main, capsys, [*common, f"experiment_path={tmp_path / 'plain'}"])
    cached, out = run_main(ae_s2.main, capsys, [*common, "--latent-cache", "4096", f"experiment_path={tmp_path / 'cached'}"])
    assert out[-2].startswith('{"latent_cache"')
    steps = [log for log in plain if "train_loss" in log]
    assert [log["step"] for log in steps] == list(range(1, 10)) and len({log["train_loss"] for log in steps}) == 9
    assert sum("val_loss" in log for log in plain) >= 2
    stats = compare_runs(plain, cached, "sequences_per_s")
    assert list(stats) == ["hits", "misses", "frames_cached", "capacity", "MiB", "bypassed"]
    # a key is (split, frame): the validation sequence shares frames with training sequences and caches its own rows
    assert stats["bypassed"] == 0 and stats["misses"] == stats["frames_cached"] and stats["hits"] > stats["misses"]
    a, b = last_ckpt(tmp_path / "plain"), last_ckpt(tmp_path / "cached")
    assert a["global_step"] == 9 and list(a) == list(b)
    assert same(a["state_dict"], b["state_dict"]) == 3 * 4096 * 2
    assert same(a["optimizer_states"], b["optimizer_states"]) >= 2
    assert same(a["rng"], b["rng"]) >= 2                            # the noise generator moved alike
    same(a["lr_schedulers"], b["lr_schedulers"])
