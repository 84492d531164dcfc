"""Residual autoencoders of the reference's experiments/v1_experiments/ae_gan/train.py without Lightning / W&B:
`ResidualBlock` (:46-77), `UpsampleBlock` (:79-86), `ConvAutoencoder` (:88-154), `ConvAutoencoderBIG` (:156-217) and
`Model` (:403-510) below `lpips.disc_start`, on csrc/resae.hip (forward) and csrc/resae_bwd.hip (backward).

The torch classes are parameter containers: created in the reference's order with torch's default initialisation, so
state_dict keys / order / shapes and the seeded initial values are the reference's.  In evaluation mode every layer of a
block is one launch of `ops.resae_conv`,
    y = act(conv(x, w) * scale + shift + res),
with BatchNorm's running statistics folded into scale / shift.  A block is three launches (two with an identity shortcut):
    shortcut = bn(conv1x1(x))                        at the block INPUT's resolution, also in an UpsampleBlock:
                                                     conv1x1(up(x)) == up(conv1x1(x)) exactly and the folded BatchNorm is
                                                     per channel, so the epilogue of conv2 reads it through the upsample
    h = gelu(bn1(conv1(x)))                          stride 1, stride 2, or over the x2 upsample, which is never written
    y = gelu(bn2(conv2(h)) + shortcut)
Packed weights and folded statistics are cached on the layer and redone when a parameter or buffer is written
(load_state_dict) or moved.

Training is an opt-in: blocks and models are created frozen (evaluation mode, no gradients, a training-mode call is
refused) and `unfreeze()` makes them trainable, as `AutoencoderKL.unfreeze()` does.  An unfrozen block in training mode
is one autograd Function (functional.ResaeBlockFn): raw convolutions, batch statistics with the running-statistics
update, the join kernel, and in the backward the data / weight gradients of csrc/resae_bwd.hip; in evaluation mode it
runs the folded path above.  `Model(cfg, trainable=True)` is the reference's training step below `disc_start`: L1 on the
autoencoder with one optimiser (the run its shipped config does: disc_start 1.0, disc_weight 0, perceptual_weight 0).

Not built: the discriminator / adaptive-weight branch of the loss and its second optimiser, LPIPS in this experiment,
`ConvAutoencoder2` and `AttentionChargedAutoencoder` (stride 4 / scale factor 4).
"""
from __future__ import annotations

import torch
import torch.nn as tnn

from ... import functional as Fn
from ... import ops
from ..._lib import WfaeError
from ...pipeline import helpers
from ._runner import Step

FOLLOW_UP = ("this block or model is frozen and runs forward-only (evaluation mode, running statistics): unfreeze() it, or "
             "build Model(cfg, trainable=True), to train it.  The discriminator branch of the GAN step remains the follow-up "
             "to this feature")
SKIPPED_PREFIXES = ("loss.discriminator.", "loss.perceptual_loss.")


class Conv(tnn.Conv2d):
    """nn.Conv2d as a container; the raw weights are packed once per (route, arithmetic mode) and again only when the
    parameter is written or moved"""

    def __init__(self, cin, cout, kernel_size, stride=1, bias=False):
        super().__init__(cin, cout, kernel_size=kernel_size, stride=stride, padding=kernel_size // 2, bias=bias)
        self._packed = {}
        self._packed_t = None

    def packed(self, kind, route, mode):
        w = self.weight
        key = (kind, w.device, w.data_ptr(), w._version)
        slot = (route, mode)
        hit = self._packed.get(slot)
        if hit is None or hit[0] != key:
            hit = (key, ops.resae_pack(w.detach(), kind, route, mode))
            self._packed[slot] = hit
        return hit[1]

    def packed_t(self, kind):
        """the data gradient's operand (ops.resae_bwd_pack), packed once per parameter version"""
        w = self.weight
        kind = ops.RESAE_KINDS[kind]
        key = (kind, w.device, w.data_ptr(), w._version)
        if self._packed_t is None or self._packed_t[0] != key:
            self._packed_t = (key, ops.resae_bwd_pack(w.detach(), kind))
        return self._packed_t[1]

    def forward(self, x, kind, scale=None, shift=None, res=None, res_up=False, act=False, route=None):
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise WfaeError(f"Conv: expected (N, {self.in_channels}, H, W), got {tuple(x.shape)}")
        kind = ops.RESAE_KINDS[kind]
        n, _, h, wd = x.shape
        route = ops.resae_route(kind, n, self.in_channels, self.out_channels, h, wd) if route is None else route
        return ops.resae_conv(x, self.packed(kind, route, ops.aekl_mode()), scale, shift, res, res_up, act, route=route)


class FoldedBatchNorm(tnn.BatchNorm2d):
    """nn.BatchNorm2d as a container of the affine and the running statistics; `folded()` is their per-channel
    (scale, shift), cached until one of the four is written or moved"""

    def __init__(self, c):
        super().__init__(c)
        self._folded = None
        self._nbt_pending = 0      # training steps not yet added to num_batches_tracked (nn.BatchNorm2d of this package)

    def flush(self):
        if self._nbt_pending:
            self.num_batches_tracked += self._nbt_pending
            self._nbt_pending = 0

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        self.flush()
        super()._save_to_state_dict(destination, prefix, keep_vars)

    def _load_from_state_dict(self, *a, **kw):
        self._nbt_pending = 0
        super()._load_from_state_dict(*a, **kw)

    def folded(self):
        ts = (self.weight, self.bias, self.running_mean, self.running_var)
        key = tuple((t.device, t.data_ptr(), t._version) for t in ts)
        if self._folded is None or self._folded[0] != key:
            self._folded = (key, ops.resae_fold(*ts, eps=self.eps))
        return self._folded[1]

    def forward(self, x):
        raise WfaeError("FoldedBatchNorm is not a layer of its own: it is applied in the epilogue of the convolution in front of "
                        "it (evaluation) or inside the block's autograd Function (training); a stand-alone BatchNorm of these "
                        "models would be a follow-up")


def _freeze(m):
    for p in m.parameters():
        p.requires_grad_(False)
    return m.eval()


class _Trainable:
    """`unfreeze()` / `freeze()` of the blocks and models, as AutoencoderKL has them; `_trainable` is what a training-mode
    call asks for"""

    _trainable = False

    def _set_trainable(self, flag):
        for m in self.modules():
            if isinstance(m, _Trainable):
                m._trainable = flag
        for p in self.parameters():
            p.requires_grad_(flag)
        return self

    def unfreeze(self):
        """parameters require gradients, `train(mode)` behaves as for any module; stays in the mode it is in"""
        return self._set_trainable(True)

    def freeze(self):
        return self._set_trainable(False).eval()


class ResidualBlock(_Trainable, tnn.Module):
    """reference :46-77"""

    def __init__(self, in_ch, out_ch, stride=1):
        super().__init__()
        if stride not in (1, 2):
            raise WfaeError(f"ResidualBlock: stride {stride!r}, only 1 and 2 are built (ConvAutoencoder2 and "
                            "AttentionChargedAutoencoder, which use 4, are not)")
        self.stride = stride
        self.conv1 = Conv(in_ch, out_ch, 3, stride)
        self.bn1 = FoldedBatchNorm(out_ch)
        self.act1 = tnn.GELU()
        self.conv2 = Conv(out_ch, out_ch, 3)
        self.bn2 = FoldedBatchNorm(out_ch)
        self.shortcut = tnn.Sequential()
        if stride != 1 or in_ch != out_ch:
            self.shortcut = tnn.Sequential(Conv(in_ch, out_ch, 1, stride), FoldedBatchNorm(out_ch))
        self.act2 = tnn.GELU()
        _freeze(self)

    def forward(self, x, up=False, route=None):
        """up: the block reads x through a x2 nearest upsample (UpsampleBlock); route: force "small" / "tile" (tests)"""
        if self.training and not self._trainable:
            raise WfaeError("ResidualBlock.forward in training mode: " + FOLLOW_UP)
        if up and self.stride != 1:
            raise WfaeError("ResidualBlock: the upsampled form has stride 1")
        if self.training:
            if x.dim() != 4 or x.shape[1] != self.conv1.in_channels:
                raise WfaeError(f"ResidualBlock: expected (N, {self.conv1.in_channels}, H, W), got {tuple(x.shape)}")
            return Fn.resae_block_train(self, x, up, route)
        with torch.no_grad():
            return self._eval(x, up, route)

    def _eval(self, x, up, route):
        short = x
        if len(self.shortcut):
            conv, bn = self.shortcut
            short = conv(x, "short_down" if self.stride == 2 else "short", *bn.folded(), route=route)
        h = self.conv1(x, "up" if up else "down" if self.stride == 2 else "conv", *self.bn1.folded(), act=True, route=route)
        return self.conv2(h, "conv", *self.bn2.folded(), res=short, res_up=up, act=True, route=route)


class UpsampleBlock(_Trainable, tnn.Module):
    """reference :79-86; the upsampled tensor is never written"""

    def __init__(self, in_ch, out_ch, scale_factor=2):
        super().__init__()
        if scale_factor != 2:
            raise WfaeError(f"UpsampleBlock: scale_factor {scale_factor!r}, only 2 is built")
        self.upsample = tnn.Upsample(scale_factor=scale_factor, mode="nearest")
        self.resblock = ResidualBlock(in_ch, out_ch, stride=1)
        self.eval()

    def forward(self, x, route=None):
        if self.training and not self._trainable:
            raise WfaeError("UpsampleBlock.forward in training mode: " + FOLLOW_UP)
        return self.resblock(x, up=True, route=route)


class _Autoencoder(_Trainable, tnn.Module):
    """what the two models share: encode / decode / forward over `enc1..enc7`, `fc_enc`, `fc_dec`, (`dec_init_conv`,)
    `dec1..dec7`, `final_conv`; `stages` collects every block's output (tests)"""

    top = 0     # channels at the 1x1 plane

    def _check(self, what, x, shape):
        if x.dim() != len(shape) or any(s is not None and s != d for s, d in zip(shape, x.shape)):
            raise WfaeError(f"{type(self).__name__}.{what}: expected {shape} (None = any), got {tuple(x.shape)}")
        if self.training and not self._trainable:
            raise WfaeError(f"{type(self).__name__}.{what} in training mode: " + FOLLOW_UP)

    def _grad_mode(self):
        """autograd sees the forward only in training mode (of an unfrozen model); evaluation runs the folded kernels"""
        return torch.enable_grad() if self.training and torch.is_grad_enabled() else torch.no_grad()

    def _linear(self, lin, x):
        if self.training:
            return Fn.LinearFn.apply(x, lin.weight, lin.bias)
        return ops.linear_fwd(x.contiguous(), lin.weight.detach(), lin.bias.detach())

    def encode(self, x, stages=None):
        self._check("encode", x, (None, self.enc1.conv1.in_channels, 128, 128))
        with self._grad_mode():
            for i in range(1, 8):
                x = getattr(self, f"enc{i}")(x)
                if stages is not None:
                    stages[f"enc{i}"] = x
            return self._linear(self.fc_enc, x.reshape(x.shape[0], -1))

    def decode(self, z, stages=None):
        self._check("decode", z, (None, self.fc_enc.out_features))
        with self._grad_mode():
            return self._decode(z, stages)

    def _decode(self, z, stages):
        x = self._linear(self.fc_dec, z).view(z.shape[0], self.top, 1, 1)
        if hasattr(self, "dec_init_conv"):
            x = self.dec_init_conv(x)
            if stages is not None:
                stages["dec_init_conv"] = x
        for i in range(1, 8):
            x = getattr(self, f"dec{i}")(x)
            if stages is not None:
                stages[f"dec{i}"] = x
        if self.training:
            return Fn.resae_conv_train(self.final_conv, x, "conv")
        return self.final_conv(x, "conv", shift=self.final_conv.bias.detach())

    def forward(self, x):
        z = self.encode(x)
        return self.decode(z), z


class ConvAutoencoder(_Autoencoder):
    """reference :88-154"""

    top = 1024

    def __init__(self, in_ch=1, latent_dim=1024):
        super().__init__()
        self.enc1 = ResidualBlock(in_ch, 64, stride=2)
        self.enc2 = ResidualBlock(64, 128, stride=2)
        self.enc3 = ResidualBlock(128, 256, stride=2)
        self.enc4 = ResidualBlock(256, 512, stride=2)
        self.enc5 = ResidualBlock(512, 1024, stride=2)
        self.enc6 = ResidualBlock(1024, 1024, stride=2)
        self.enc7 = ResidualBlock(1024, 1024, stride=2)
        self.flatten = tnn.Flatten()
        self.fc_enc = tnn.Linear(1024, latent_dim)
        self.fc_dec = tnn.Linear(latent_dim, 1024)
        self.unflatten = tnn.Unflatten(1, (1024, 1, 1))
        self.dec_init_conv = ResidualBlock(1024, 1024, stride=1)
        self.dec1 = UpsampleBlock(1024, 512, scale_factor=2)
        self.dec2 = UpsampleBlock(512, 256, scale_factor=2)
        self.dec3 = UpsampleBlock(256, 128, scale_factor=2)
        self.dec4 = UpsampleBlock(128, 64, scale_factor=2)
        self.dec5 = UpsampleBlock(64, 64, scale_factor=2)
        self.dec6 = UpsampleBlock(64, 64, scale_factor=2)
        self.dec7 = UpsampleBlock(64, 64, scale_factor=2)
        self.final_conv = Conv(64, in_ch, 3, bias=True)
        _freeze(self)


class ConvAutoencoderBIG(_Autoencoder):
    """reference :156-217"""

    top = 2048

    def __init__(self, in_ch: int = 1, latent_dim: int = 2048):
        super().__init__()
        self.enc1 = ResidualBlock(in_ch, 64, stride=2)
        self.enc2 = ResidualBlock(64, 128, stride=2)
        self.enc3 = ResidualBlock(128, 256, stride=2)
        self.enc4 = ResidualBlock(256, 512, stride=2)
        self.enc5 = ResidualBlock(512, 1024, stride=2)
        self.enc6 = ResidualBlock(1024, 2048, stride=2)
        self.enc7 = ResidualBlock(2048, 2048, stride=2)
        self.flatten = tnn.Flatten()
        self.fc_enc = tnn.Linear(2048, latent_dim)
        self.fc_dec = tnn.Linear(latent_dim, 2048)
        self.unflatten = tnn.Unflatten(1, (2048, 1, 1))
        self.dec1 = UpsampleBlock(2048, 1024)
        self.dec2 = UpsampleBlock(1024, 512)
        self.dec3 = UpsampleBlock(512, 256)
        self.dec4 = UpsampleBlock(256, 128)
        self.dec5 = UpsampleBlock(128, 64)
        self.dec6 = UpsampleBlock(64, 64)
        self.dec7 = UpsampleBlock(64, 32)
        self.final_conv = Conv(32, in_ch, 3, bias=True)
        _freeze(self)


def reference_keys(model):
    """state_dict keys of `model` in order: the reference's"""
    return list(model.state_dict().keys())


def autoencoder_state(state):
    """a state dict, or a Lightning checkpoint of the reference's `Model` -> the autoencoder's own state dict: keys under
    `autoencoder.` are kept (without the prefix), `loss.discriminator.*` and `loss.perceptual_loss.*` are ignored, anything
    else next to an `autoencoder.` key is an error; a dict without that prefix is taken as the autoencoder's"""
    state = state.get("state_dict", state) if isinstance(state, dict) else state
    if not any(k.startswith("autoencoder.") for k in state):
        return dict(state)
    kept = {k[len("autoencoder."):]: v for k, v in state.items() if k.startswith("autoencoder.")}
    other = [k for k in state if not k.startswith(("autoencoder.",) + SKIPPED_PREFIXES)]
    if other:
        raise WfaeError(f"ae_gan checkpoint: keys of neither the autoencoder nor the loss: {other[:4]}")
    return kept


def load_checkpoint(autoencoder, path):
    """strict load of what `autoencoder_state` keeps"""
    autoencoder.load_state_dict(autoencoder_state(torch.load(path, map_location="cpu")), strict=True)
    return autoencoder


class Model(Step, tnn.Module):
    """reference Model (:403-510) with the loss's `global_step < disc_start` branch (:359-373), the only one the shipped
    config (`disc_start: 1.0` of the total steps) reaches: `autoencoder`, `forward`, `get_last_layer`, `validation_step`,
    `test_step`, and with `trainable=True` the generator half of `training_step` (:439-457) on `_runner.Step`"""

    trained = "autoencoder"
    exact_complements = True

    def __init__(self, cfg, autoencoder=None, trainable=False):
        super().__init__()
        if autoencoder is not None:
            raise WfaeError("ae_gan evaluates its own autoencoder: it takes no latent provider")
        self.cfg = cfg
        self.trainable = bool(trainable)
        name = cfg.model.name
        if name == "convautoencoder":
            self.autoencoder = ConvAutoencoderBIG(latent_dim=cfg.ConvAutoencoder.latent_dim)       # reference :409-410
        elif name in ("convautoencoder2", "attentionchargedautoencoder"):
            raise WfaeError(f"model.name={name!r}: ConvAutoencoder2 and AttentionChargedAutoencoder (stride 4 / scale "
                            "factor 4) are not built; only 'convautoencoder' is")
        else:
            raise ValueError(f"Unknown model type: {name}")
        if cfg.model.get("checkpoint"):
            load_checkpoint(self.autoencoder, cfg.model.checkpoint)
        lp = cfg.lpips
        if lp.perceptual_weight > 0:
            raise WfaeError(f"lpips.perceptual_weight={lp.perceptual_weight}: the perceptual (LPIPS) term of this experiment "
                            "is not built; the shipped config has 0")
        self.disc_start, self.recon_weight = lp.disc_start, lp.recon_weight
        self.global_step = 0
        self.logs = {}
        if self.trainable:
            if cfg.trainer.accumulate_grad_batches != 1:
                raise WfaeError("Model: trainer.accumulate_grad_batches must be 1 (the shipped value)")
            self.total_steps = cfg.trainer.total_train_steps
            self.autoencoder.unfreeze()

    def train(self, mode=True):
        """a model that is not trainable keeps its autoencoder in evaluation mode"""
        super().train(mode)
        if not self.trainable:
            self.autoencoder.eval()
        return self

    def forward(self, x):
        return self.autoencoder(x)[0]

    def get_last_layer(self):
        return self.autoencoder.final_conv.weight

    @staticmethod
    def frames(batch):
        """the loader's batch (a tensor or its dict; (B, T, H, W) or (B, 1, H, W) frames) -> (B * T, 1, H, W)"""
        if isinstance(batch, dict):
            batch = batch["vil"]
        if batch.dim() != 4:
            raise WfaeError(f"Model: expected frames (B, T, H, W), got {tuple(batch.shape)}")
        return batch.reshape(-1, 1, batch.shape[2], batch.shape[3]).contiguous()

    def _refuse_disc(self, what):
        if self.global_step >= self.disc_start:
            raise WfaeError(f"Model.{what} at global_step {self.global_step} >= lpips.disc_start {self.disc_start}: "
                            "the discriminator branch of the loss and its optimiser are not built")

    def validation_refused(self):
        """why a validation / test pass cannot run at this `global_step` (the driver prints it and goes on), or None:
        from `disc_start` on the steps are refused, and a fit ends exactly there"""
        if self.global_step >= self.disc_start:
            return (f"global_step {self.global_step} >= lpips.disc_start {self.disc_start}: the discriminator branch of "
                    "the loss is not built")
        return None

    def training_step(self, batch, batch_idx=0):
        """reference :439-457 below disc_start: rec_loss = recon_weight * L1, backward, clip at optim.gradient_clip_val,
        AdamW, schedule -> (loss, gradient norm before clipping); the logs of the loss (:366-371) are left in `self.logs`"""
        if not self.trainable:
            raise WfaeError("Model.training_step: " + FOLLOW_UP)
        self._refuse_disc("training_step")
        if not hasattr(self, "opt"):
            raise WfaeError("Model.training_step: call configure_optimizers() first")
        self.autoencoder.train()        # the shared driver leaves `autoencoder` attributes in evaluation mode
        inp = self.frames(batch)
        pred = self(inp)
        rec = Fn.l1_loss(pred, inp, float(self.recon_weight))
        loss, gn = self.optimizer_step(rec)
        self.logs = {"train/total_loss": loss, "train/rec_loss": loss, "train/g_loss": 0.0, "train/d_weight": 0.0,
                     "train/g_grad_norm": gn}
        self.global_step += 1
        if self.panels is not None:
            self._plot(pred, inp, "train", self.panels.batch_idx)
        return loss, gn

    def _plot(self, pred, inp, split, batch_idx):
        """the figures of reference :478-480, :493-495, :508-510: the batch index against int(fraction * total), the train fraction and total in
        the training step, the validation ones in the validation AND the test step"""
        if self.panels is None:
            return
        e, tr = self.panels.epoch, split == "train"
        label = {"train": "Train Reconstruction", "val": "Val_Reconstruction", "test": "Test_Reconstruction"}[split] \
            + f" vs Original_epoch_{e}_batch_{batch_idx}" + ("_test" if split == "test" else "")
        helpers.plot_panels(self, pred, inp, label, batch_idx,
                            helpers.plot_fraction(self.cfg, "log_train_plots_n" if tr else "log_val_plots_n", 0.1),
                            self.panels.total("train" if tr else "val"))

    def configure_optimizers(self):
        if not self.trainable:
            raise WfaeError("Model.configure_optimizers: " + FOLLOW_UP)
        return Step.configure_optimizers(self)

    @torch.no_grad()
    def validation_step(self, batch, batch_idx=0, split="val"):
        """reference :482-510 below disc_start -> (rec_loss, logs)"""
        self._refuse_disc(f"{split} step")
        inp = self.frames(batch)
        pred = self(inp)
        rec = Fn.l1_loss(pred, inp, float(self.recon_weight))
        logs = {f"{split}/total_loss": rec, f"{split}/rec_loss": rec, f"{split}/g_loss": 0.0, f"{split}/d_weight": 0.0}
        logs.update(helpers.log_metrics(pred.unsqueeze(2), inp.unsqueeze(2), split))
        self._plot(pred, inp, split, batch_idx)
        return rec, logs

    def test_step(self, batch, batch_idx=0):
        return self.validation_step(batch, batch_idx, split="test")


def model_state(model):
    """what `last.ckpt` holds, in Lightning's spelling: `autoencoder.*` (`autoencoder_state` / `load_checkpoint` read it)"""
    return {"autoencoder." + k: v for k, v in model.autoencoder.state_dict().items()}
