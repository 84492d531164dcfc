"""Frozen latent provider of the v1 latent experiments (linear, DLinear, conv autoencoder): the reference's `Autoencoder`
wrapper around a pretrained AutoencoderKL (pretrained_ae_linear_sevir/train.py:21-56, the same class in the DLinear and
conv experiments), with the project's own encoders as further kinds.  The experiments' `train.py` and `_dlinear.py`
re-export it under the name `Autoencoder`.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as tnn

from ... import ops
from ..._lib import WfaeError
from ...pipeline.models.ae_64x8x8_lin import PosAwareAE_TF


class LatentCache:
    """Latents of a frozen provider, kept on the device so that a frame is encoded once: a table (capacity, L) fp32 of one
    row per frame — the posterior mode (L = C h w), or the moments (L = 2 C h w) of a sampling provider, whose noise is
    applied after the table is read — and a host dict key -> slot, a key being (split, frame id).  No eviction: slots are
    handed out in first-seen order until `capacity`; a frame met after that is encoded every time it appears.  The table
    is allocated at the first `rows()`, when L is known.
    `pass_frames[split]`: the number of frames per encoder pass that the split's cached rows were computed with (see
    `Autoencoder._encode_cached`: the encoder's GEMM routes depend on it, so it is part of what a row is).
    Counters: `misses` frames that were encoded, `hits` frames that were asked for and not encoded (read from the table,
    or a repeat inside one batch of a frame encoded in that step: `hits` is not the number of table reads), `bypassed`
    frames of batches that went around the cache, `frames_cached` slots in use, `bytes` of the table.
    With a pass-invariant provider (`Autoencoder.pass_invariant`) a row does not depend on its pass: `pass_frames` and
    `serves` are not used and `bypassed` stays 0."""

    def __init__(self, capacity):
        self.capacity = int(capacity)
        if self.capacity < 1:
            raise ValueError(f"LatentCache: capacity {capacity}, expected at least one frame")
        self.slot, self.table, self.latent_shape, self.pass_frames = {}, None, None, {}
        self.hits = self.misses = self.bypassed = 0

    @property
    def frames_cached(self):
        return len(self.slot)

    @property
    def bytes(self):
        return 0 if self.table is None else self.table.numel() * 4

    def stats(self):
        return {"hits": self.hits, "misses": self.misses, "frames_cached": self.frames_cached, "capacity": self.capacity,
                "MiB": round(self.bytes / 2 ** 20, 3), "bypassed": self.bypassed}

    def plan(self, keys):
        """host only.  keys: the B*T frames of a batch in (b, t) order -> (missing, slots, index):
        missing: the keys to encode, unique, in first-seen order (a frame that appears twice is encoded once);
        slots: int64, one per missing key: the table row it gets (and keeps), -1 once the table is full;
        index: int64, one per frame: the table row (>= 0) of a frame cached by an earlier batch, else -1 - j for row j of
        this batch's encoded frames — also for those that get a slot now: they are read from `fresh`, not from the table"""
        missing, slots, index, fresh = [], [], [], {}
        for k in keys:
            if k in fresh:
                index.append(-1 - fresh[k])
                continue
            s = self.slot.get(k)
            if s is not None:
                index.append(s)
                continue
            j = fresh[k] = len(missing)
            missing.append(k)
            if len(self.slot) < self.capacity:
                slots.append(len(self.slot))
                self.slot[k] = slots[-1]
            else:
                slots.append(-1)
            index.append(-1 - j)
        self.misses += len(missing)
        self.hits += len(index) - len(missing)
        return missing, np.asarray(slots, dtype=np.int64), np.asarray(index, dtype=np.int64)

    def rows(self, latent_shape, device):
        """the table for rows of `latent_shape` (C or 2C, h, w), allocated at the first call"""
        if self.table is None:
            self.latent_shape = tuple(int(v) for v in latent_shape)
            self.table = torch.empty((self.capacity, int(np.prod(self.latent_shape))), dtype=torch.float32, device=device)
        elif tuple(latent_shape) != self.latent_shape:
            raise WfaeError(f"LatentCache: rows of shape {tuple(latent_shape)}, the table holds {self.latent_shape}")
        return self.table

    def clear(self):
        """forget every frame (the table stays allocated and is refilled)"""
        self.slot.clear()

    def serves(self, split, n, chunk_frames):
        """host only.  Whether a batch of n frames of `split` goes through the cache, given that the uncached encode runs
        it in passes of `chunk_frames` frames (0: one pass of n) -> the pass size, or 0 for "go around the cache".
        A batch is served when all its uncached passes have one size and that size is the split's (set by its first
        served batch): a short last batch, or one with a smaller tail chunk, is not"""
        size = chunk_frames if chunk_frames > 0 else n
        if n % size or self.pass_frames.setdefault(split, size) != size:
            self.bypassed += n
            return 0
        return size


class Autoencoder(tnn.Module):
    """frozen latent provider with the reference wrapper's interface (:21-56): encode (B,T,1,H,W) -> (B,T,C,h,w).
    kind "ae_64x8x8_lin.enc": the conv encoder stack (64 channels at 1/16 resolution);
    kind "ae_vit.tokens": the structured token latent [64, 512] of AE_ViT_2048 (BASELINE config 4), i.e. the
    encoder tokens laid out as 512 channels on the 8x8 patch grid;
    kind "autoencoder_kl": the reference's own provider, the frozen AutoencoderKL (pipeline/models/autoencoderkl) built
    from the `autoencoder:` config block `cfg` (the reference's keys), with `cfg.checkpoint` loaded when given (a state
    dict, or a Lightning checkpoint that holds it under the `autoencoder.` / `model.` prefix, other modules' keys next to
    it being ignored), else a seeded initialisation
    (`cfg.seed`, default 0).  encode returns the posterior's mode; frames go through in chunks of `cfg.chunk_frames`
    (default 8; 0 = all B*T frames in one pass).  `cfg.pass_invariant: true` (the drivers' --invariant-encode; this kind
    only) puts the model into `AutoencoderKL.pass_invariant()` mode: a frame's latent is then the same bits in every pass,
    and a cache encodes exactly the frames it misses (`_encode_cached`).
    With `cfg.sample: true` (ae_s2) encode returns a sample instead,
    z = mean + std * noise, the noise drawn as the reference's loop over T draws it (`draw_noise`).
    kind "ae_gan.convautoencoder": the residual `ConvAutoencoderBIG` of ae_gan in evaluation mode (`cfg.latent_dim`, default
    2048; `cfg.checkpoint` / `cfg.seed` as for autoencoder_kl): encode (B, T, 1, 128, 128) -> (B, T, latent_dim, 1, 1), decode
    back to frames, the raw `final_conv` output as in the reference; frames go through in chunks of `cfg.chunk_frames`
    (default 64: the 1x1 .. 4x4 layers are a weight stream, so a chunk should be large; the 64 x 64 activations bound it).
    The conv, AutoencoderKL and ae_gan kinds also `decode` — act(dec(z)) for each frame — so that validation / test can score
    forecasts in frame space like the reference (pretrained_ae_dlinear_*/train.py:196-200)."""

    AEKL_KEYS = ("in_channels", "out_channels", "down_block_types", "up_block_types", "block_out_channels",
                 "layers_per_block", "act_fn", "latent_channels", "norm_num_groups", "sample_size", "scaling_factor")

    def __init__(self, img_size=128, kind="ae_64x8x8_lin.enc", cfg=None):
        super().__init__()
        self.kind = kind
        self.chunk_frames = 0
        self.sample = False
        self.cache = None
        self.pass_invariant = False
        if (cfg or {}).get("pass_invariant") is not None and kind != "autoencoder_kl":
            raise WfaeError(f"autoencoder.pass_invariant belongs to kind 'autoencoder_kl', not to {kind!r}: only the frozen "
                            "AutoencoderKL has a pass-invariant form")
        if kind == "autoencoder_kl":
            self.autoencoder = self._build_autoencoder_kl(cfg or {})
            chunk = (cfg or {}).get("chunk_frames")
            self.chunk_frames = 8 if chunk is None else int(chunk)      # 0: all B*T frames in one pass
            self.sample = bool((cfg or {}).get("sample") or False)
            if (cfg or {}).get("pass_invariant"):
                self.set_pass_invariant()
            if self.chunk_frames < 0:
                raise ValueError(f"autoencoder.chunk_frames={self.chunk_frames}")
        elif kind == "ae_gan.convautoencoder":
            self.autoencoder = self._build_ae_gan(cfg or {})
            self.chunk_frames = int((cfg or {}).get("chunk_frames") or 64)
            if self.chunk_frames < 1:
                raise ValueError(f"autoencoder.chunk_frames={self.chunk_frames}")
        elif kind == "ae_vit.tokens":
            from ...pipeline.models.ae_vit import AE_ViT_2048
            self.autoencoder = AE_ViT_2048().eval()
        elif kind == "ae_64x8x8_lin.enc":
            self.autoencoder = PosAwareAE_TF(img_size=img_size).eval()
        else:
            raise ValueError(f"autoencoder.kind={kind!r}")
        for p in self.autoencoder.parameters():
            p.requires_grad_(False)

    @classmethod
    def _build_autoencoder_kl(cls, cfg):
        from ...pipeline.models.autoencoderkl import AutoencoderKL
        kw = {k: cfg[k] for k in cls.AEKL_KEYS if cfg.get(k) is not None}
        ckpt = cfg.get("checkpoint")
        if ckpt:
            model = AutoencoderKL(**kw)
            sd = torch.load(ckpt, map_location="cpu")
            sd = sd.get("state_dict", sd) if isinstance(sd, dict) else sd
            # a Lightning checkpoint holds the provider under a prefix, next to other modules (predictor.*, loss.*): keep
            # the keys under the first prefix that holds the VAE, drop the rest; the strict load then checks what is kept
            probe = "encoder.conv_in.weight"
            for prefix in ("", "autoencoder.autoencoder.", "autoencoder.", "model."):
                if prefix + probe in sd:
                    sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)} if prefix else sd
                    break
            model.load_state_dict(sd, strict=True)
            return model
        with torch.random.fork_rng(devices=[]):     # the seeded initialisation does not move the caller's generator
            torch.manual_seed(int(cfg.get("seed") or 0))
            return AutoencoderKL(**kw)

    @staticmethod
    def _build_ae_gan(cfg):
        from ._ae_gan import ConvAutoencoderBIG, load_checkpoint
        latent_dim = int(cfg.get("latent_dim") or 2048)
        if cfg.get("checkpoint"):
            return load_checkpoint(ConvAutoencoderBIG(latent_dim=latent_dim), cfg["checkpoint"])
        with torch.random.fork_rng(devices=[]):     # the seeded initialisation does not move the caller's generator
            torch.manual_seed(int(cfg.get("seed") or 0))
            return ConvAutoencoderBIG(latent_dim=latent_dim)

    def _chunks(self, frames):
        n = self.chunk_frames if self.chunk_frames > 0 else frames.shape[0]
        return [frames[i:i + n].contiguous() for i in range(0, frames.shape[0], n)]

    def draw_noise(self, b, t, latent_shape, device, generator=None):
        """(T, B, C, h, w): the T draws torch.randn((B, C, h, w)) of the reference's per-frame `encode(frame).sample()`
        (ae_s2/train.py:34-37), in frame order from `generator` (None: the device's global generator), each written into
        its slice of one buffer.  One large draw is not the same stream."""
        noise = torch.empty((t, b, *latent_shape), dtype=torch.float32, device=device)
        for i in range(t):
            torch.randn((b, *latent_shape), generator=generator, device=device, dtype=torch.float32, out=noise[i])
        return noise

    def set_pass_invariant(self, flag=True):
        """put the frozen AutoencoderKL into (or take it out of) `AutoencoderKL.pass_invariant()` mode: a frame's latent
        no longer depends on the frames that share its encoder pass.  A cache filled in the other mode is emptied"""
        if self.kind != "autoencoder_kl":
            raise WfaeError(f"Autoencoder.set_pass_invariant: kind {self.kind!r} has no pass-invariant form, only "
                            "autoencoder_kl has (its attention projections then run on the row-invariant linear kernel)")
        self.autoencoder.pass_invariant(flag)
        if self.cache is not None and bool(flag) != self.pass_invariant:
            self.cache.clear()
            self.cache.pass_frames.clear()
        self.pass_invariant = bool(flag)
        return self

    def enable_cache(self, capacity_frames):
        """keep the latents of up to `capacity_frames` frames on the device (`LatentCache`); `encode(x, ids=...)` then
        encodes a frame once.  -> the cache"""
        if self.kind != "autoencoder_kl":
            raise WfaeError(f"Autoencoder.enable_cache: kind {self.kind!r} is not cached, only autoencoder_kl is.  The other "
                            "kinds' kernel routes are chosen from the batch size (ae_gan.convautoencoder: the K-split of its "
                            "small route depends on the total column count; for the rest this is a precaution), so a "
                            "cached latent would not be the bits of the uncached encode; for the AutoencoderKL encoder the "
                            "cache keeps the number of frames per pass that the uncached encode uses")
        self.cache = LatentCache(capacity_frames)
        return self.cache

    def _encode_cached(self, x, ids, generator, noise):
        """`encode` through the cache: plan, encode the missing frames, scatter them, one gather launch; None for a
        batch that goes around the cache.
        A frame's latent depends on how many frames share its encoder pass: the mid-block attention's projections are
        GEMMs of frames x tokens rows, and their K-split and tile size are chosen from the row count (gemm.hip
        `pick_splits`), i.e. their summation order is.  It does not depend on which frames those are, nor on the frame's
        place in the pass: convolutions, GroupNorm and attention work per sample, a GEMM row's sums per row.  So the
        missing frames are encoded in passes of exactly the size the uncached encode uses, filled up with repeats of the
        last missing frame whose results are dropped; one missing frame costs one whole pass.  A batch whose uncached
        passes are not all of that size (`LatentCache.serves`) is encoded as without the cache and neither read from
        nor written to the table.
        A pass-invariant provider has no such dependence (the projections run on linear_fwd_rowinv), so every batch is
        served, short ones and tail chunks included, and exactly the unique missing frames are encoded: in passes of at
        most `chunk_frames` frames, or in one pass when that is 0, with no fill-up repeats; a frame past the capacity
        costs itself"""
        b, t, c, h, w = x.shape
        split, fid = ids
        fid = np.asarray(fid).reshape(-1)
        if fid.size != b * t:
            raise WfaeError(f"Autoencoder.encode: {fid.size} frame ids for a batch of {b} x {t} frames")
        cache = self.cache
        if self.pass_invariant:
            size = 0
        else:
            size = cache.serves(split, b * t, self.chunk_frames)
            if not size:
                return None
        keys = [(split, int(i)) for i in fid]
        missing, slots, index = cache.plan(keys)
        fresh = None
        if missing:
            try:
                first = {}
                for f, k in enumerate(keys):
                    first.setdefault(k, f)
                rows = [first[k] for k in missing]
                if self.pass_invariant:
                    size = self.chunk_frames if self.chunk_frames > 0 else len(rows)    # the last pass may be short
                else:
                    rows += [rows[-1]] * (-len(rows) % size)          # whole passes of `size` frames
                frames = x.reshape(b * t, c, h, w)
                if rows != list(range(b * t)):
                    frames = frames[torch.as_tensor(rows, device=x.device)]
                ae = self.autoencoder
                fresh = torch.cat([ae.moments(f) if self.sample else ae.encode(f).mode()
                                   for f in (frames[i:i + size].contiguous() for i in range(0, len(rows), size))])
                table = cache.rows(fresh.shape[1:], fresh.device)
                fresh = fresh[:len(missing)].reshape(len(missing), -1)
                if (slots >= 0).any():
                    ops.latent_scatter(fresh, slots, table)
            except BaseException:
                cache.clear()       # the plan handed out slots for rows that may not have been written
                raise
        table, shape = cache.table, cache.latent_shape
        if self.sample:
            shape = (shape[0] // 2, *shape[1:])
            if noise is None:
                noise = self.draw_noise(b, t, shape, table.device, generator)
            elif tuple(noise.shape) != (t, b, *shape):
                raise WfaeError(f"Autoencoder.encode: noise {tuple(noise.shape)}, expected {(t, b, *shape)}")
            noise = noise.contiguous()
        return ops.latent_gather(table, fresh, index, (b, t), noise).view(b, t, *shape)

    @torch.no_grad()
    def encode(self, x, generator=None, noise=None, ids=None):
        """x (B, T, 1, H, W) -> (B, T, C, h, w).  `generator` / `noise` (T, B, C, h, w) belong to `sample: true`: `noise`
        replaces the draw.  `ids` = (split, the B*T int64 frame ids in (b, t) order) names the frames for the cache of
        `enable_cache`: the result is the same bits, frames met before are not encoded again (a batch whose encoder
        passes are not of the cached size goes around the cache, unless the provider is pass-invariant).  Without a cache
        `ids` is not read, and without `ids`
        the cache is not used"""
        b, t, c, h, w = x.shape
        frames = x.reshape(b * t, c, h, w)
        if not self.sample and (generator is not None or noise is not None):
            raise WfaeError("Autoencoder.encode: generator / noise need the sampled provider (autoencoder_kl with sample: true)")
        if self.cache is not None and ids is not None:
            z = self._encode_cached(x, ids, generator, noise)
            if z is not None:
                return z
        if self.kind == "autoencoder_kl" and self.sample:
            moments = torch.cat([self.autoencoder.moments(f) for f in self._chunks(frames)])
            shape = (moments.shape[1] // 2, *moments.shape[2:])
            if noise is None:
                noise = self.draw_noise(b, t, shape, moments.device, generator)
            elif tuple(noise.shape) != (t, b, *shape):
                raise WfaeError(f"Autoencoder.encode: noise {tuple(noise.shape)}, expected {(t, b, *shape)}")
            return ops.aekl_posterior_seq(moments, noise.contiguous())
        if self.kind == "autoencoder_kl":
            z = torch.cat([self.autoencoder.encode(f).mode() for f in self._chunks(frames)])
        elif self.kind == "ae_gan.convautoencoder":
            z = torch.cat([self.autoencoder.encode(f) for f in self._chunks(frames)])[:, :, None, None]
        elif self.kind == "ae_vit.tokens":
            tok = self.autoencoder.encode_tokens(frames)                      # (B*T, 64, 512)
            s = self.autoencoder.seq
            z = tok.transpose(1, 2).contiguous().view(b * t, tok.shape[2], s, s)
        else:
            z = self.autoencoder.enc(frames)
        return z.view(b, t, *z.shape[1:])

    def can_decode(self):
        return self.kind in ("ae_64x8x8_lin.enc", "autoencoder_kl", "ae_gan.convautoencoder")

    @torch.no_grad()
    def decode(self, z):
        """z (B, T, C, h, w) -> frames (B, T, 1, H, W)"""
        if not self.can_decode():
            raise WfaeError(f"Autoencoder.decode: kind {self.kind!r} has no decoder")
        b, t = z.shape[:2]
        ae = self.autoencoder
        if self.kind == "autoencoder_kl":
            x = torch.cat([ae.decode(f) for f in self._chunks(z.reshape(b * t, *z.shape[2:]))])
            return x.view(b, t, *x.shape[1:])
        if self.kind == "ae_gan.convautoencoder":
            x = torch.cat([ae.decode(f) for f in self._chunks(z.reshape(b * t, -1))])
            return x.view(b, t, *x.shape[1:])
        x = ae.act(ae.dec(z.reshape(b * t, *z.shape[2:]).contiguous()))
        return x.view(b, t, *x.shape[1:])
