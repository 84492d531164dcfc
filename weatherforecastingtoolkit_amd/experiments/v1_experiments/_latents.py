"""Frozen latent provider of the v1 latent experiments (linear, DLinear, conv autoencoder): the reference's `Autoencoder`
wrapper around a pretrained AutoencoderKL (pretrained_ae_linear_sevir/train.py:21-56, the same class in the DLinear and
conv experiments), with the project's own encoders as further kinds.  The experiments' `train.py` and `_dlinear.py`
re-export it under the name `Autoencoder`.
"""
from __future__ import annotations

import torch
import torch.nn as tnn

from ... import ops
from ..._lib import WfaeError
from ...pipeline.models.ae_64x8x8_lin import PosAwareAE_TF


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
    (default 8; 0 = all B*T frames in one pass).  With `cfg.sample: true` (ae_s2) encode returns a sample instead,
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
        if kind == "autoencoder_kl":
            self.autoencoder = self._build_autoencoder_kl(cfg or {})
            chunk = (cfg or {}).get("chunk_frames")
            self.chunk_frames = 8 if chunk is None else int(chunk)      # 0: all B*T frames in one pass
            self.sample = bool((cfg or {}).get("sample") or False)
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

    @torch.no_grad()
    def encode(self, x, generator=None, noise=None):
        """x (B, T, 1, H, W) -> (B, T, C, h, w).  `generator` / `noise` (T, B, C, h, w) belong to `sample: true`: `noise`
        replaces the draw"""
        b, t, c, h, w = x.shape
        frames = x.reshape(b * t, c, h, w)
        if not self.sample and (generator is not None or noise is not None):
            raise WfaeError("Autoencoder.encode: generator / noise need the sampled provider (autoencoder_kl with sample: true)")
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
