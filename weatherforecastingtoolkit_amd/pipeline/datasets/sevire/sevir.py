"""SEVIR frame loader contract of the reference (pipeline/datasets/sevire/sevir.py)
for the AE train step, with the uint8 -> fp32 / 255 + layout change done on the
GPU by a HIP kernel.

Contract reproduced (reference lines):
  * events are uint8 VIL arrays (N_ev, H, W, raw_T)                 :453-482, 681-716
  * num_seq_per_event = 1 + (raw_T - seq_len) // stride             :403-404
  * batch `index` = batch_size consecutive (event, seq) pairs from
    event (index*B)//nspe, seq (index*B)%nspe                       :979-1003
  * len = total_num_seq // batch_size                               :657-661
  * x = (1/255) * (u8.float() + 0), layout 'NHWT' -> 'NTHW'         :749-794, 98-139, 163, 168
  * the outer DataLoader yields the dict of ONE pre-formed batch    :1132-1151
  * train events are shuffled ONCE with random_state=1              :363-367 (here: numpy RandomState(1) permutation)
Events come either from memory (synthetic `synth.blob_events`, or any uint8 array) or from an event store
(`catalog.CatalogEventStore`: filtered SEVIR catalog + .npy / HDF5 files).
`prefetch()` overlaps the host gather and the uint8 H2D copy of batch i+1 (pinned staging buffers, a copy
stream) with the training step of batch i.  AWS download of the reference is out of scope.

Train-time augmentation (`aug_mode`, the reference's SECOND loader, pipeline/datasets/sevir/sevir.py:1035-1058): one
h-flip / v-flip / rotation per sequence, drawn on the host by `augment_params` and applied on the device inside the
conversion kernel (`ops.vil_augment_u8_to_f32`), so the batch still crosses the bus as uint8 and is written once.

Downsampling (`ops.vil_pool_u8_to_f32`, the third kernel of that family): `presample=(ft, fh, fw)` applies the reference's
OFFLINE sevir_lr recipe (save_downsampled_dataset :575-616: frames [::ft], block max) on the fly, so a loader over raw
384 x 384 x 49 SEVIR is, batch for batch, the loader over the 128 x 128 x 25 dataset that recipe would have written;
`downsample_dict` is the reference's runtime option (downsample_data_dict :849-890: frames [::ft], avg_pool2d) and
`rescale_method` its choice of scale and offset (preprocess_data_dict :749-794).
"""
from __future__ import annotations

import math
import queue
import threading

import numpy as np
import torch

from .... import ops

PREPROCESS_SCALE_01 = {"vil": 1 / 255}
PREPROCESS_OFFSET_01 = {"vil": 0}
PREPROCESS_SCALE_SEVIR = {"vil": 1 / 47.54}           # reference sevire/sevir.py:150-159
PREPROCESS_OFFSET_SEVIR = {"vil": -33.44}
RESCALE = {"01": (PREPROCESS_SCALE_01, PREPROCESS_OFFSET_01), "sevir": (PREPROCESS_SCALE_SEVIR, PREPROCESS_OFFSET_SEVIR)}
RAW_EVENT_SHAPE = (384, 384, 49)
LR_PRESAMPLE = (2, 3, 3)                              # save_downsampled_dataset's defaults: 384 x 384 x 49 -> 128 x 128 x 25


def _factors(f, what):
    try:
        out = tuple(int(x) for x in f)
    except (TypeError, ValueError):
        out = ()
    if len(out) != 3 or min(out) < 1 or any(o != x for o, x in zip(out, f)):
        raise ValueError(f"{what}: three integer factors (t, h, w) >= 1, got {f!r}")
    return out


def lr_presample(dataset_name, event_shape):
    """the factors that turn the events at hand into what `dataset_name` means: (2, 3, 3) for a sevir_lr / sevirlr config
    over raw SEVIR events (384, 384, 49), None in every other case (a store that is already low-resolution, full SEVIR)"""
    if dataset_name in ("sevir_lr", "sevirlr") and tuple(event_shape) == RAW_EVENT_SHAPE:
        return LR_PRESAMPLE
    return None


def parse_presample(text):
    """--presample of the entry points: 'auto' -> "auto", 'none' -> None, 'T,H,W' -> (T, H, W)"""
    t = str(text).strip().lower()
    if t == "auto":
        return "auto"
    if t == "none":
        return None
    try:
        return _factors([int(x) for x in t.split(",")], "--presample")
    except ValueError:
        raise ValueError(f"--presample: 'auto', 'none' or three integers T,H,W >= 1, got {text!r}") from None


def resolve_presample(arg, dataset_name, event_shape):
    """(factors or None, pooled (H, W, T)) for a parsed --presample and the events of a store"""
    f = lr_presample(dataset_name, event_shape) if arg == "auto" else arg
    if f is None:
        return None, tuple(event_shape)
    h, w, t = event_shape
    return f, (-(-h // f[1]), -(-w // f[2]), -(-t // f[0]))


def presample_line(factors, raw_shape, pooled_shape):
    return "presample {}: {}x{}x{} -> {}x{}x{}".format(tuple(factors), *raw_shape, *pooled_shape)


# out_layout values of the reference's change_layout_torch (sevire/sevir.py:98-139).  The device kernel writes the frames
# as contiguous 'NTHW' (the ae_v2 setting, train.py:290-304; T plays the role of the channel dimension); the other
# layouts are the reference's own permute / unsqueeze VIEWS of that tensor (the reference returns views too unless
# ret_contiguous is set), so values, shapes and dtypes agree with change_layout_torch(x_nhwt, 'NHWT', layout).
LAYOUTS = {
    "NTHW": lambda t: t,
    "NHWT": lambda t: t.permute(0, 2, 3, 1),
    "NTCHW": lambda t: t.unsqueeze(2),
    "NTHWC": lambda t: t.unsqueeze(-1),
    "TNHW": lambda t: t.permute(1, 0, 2, 3),
    "TNCHW": lambda t: t.permute(1, 0, 2, 3).unsqueeze(2),
}


def change_layout_torch(data, in_layout="NHWT", out_layout="NHWT", ret_contiguous=False):
    """the reference's layout switch (sevire/sevir.py:98-139) for tensors that already live on the device"""
    to_nhwt = {"NHWT": lambda d: d, "NTHW": lambda d: d.permute(0, 2, 3, 1),
               "NTCHW": lambda d: d[:, :, 0].permute(0, 2, 3, 1), "NTHWC": lambda d: d[..., 0].permute(0, 2, 3, 1),
               "TNHW": lambda d: d.permute(1, 2, 3, 0), "TNCHW": lambda d: d[:, :, 0].permute(1, 2, 3, 0)}
    if in_layout not in to_nhwt or out_layout not in LAYOUTS:
        raise NotImplementedError
    data = LAYOUTS[out_layout](to_nhwt[in_layout](data).permute(0, 3, 1, 2))
    return data.contiguous() if ret_contiguous else data


AUG_MODES = ("0", "1", "2")
FIX_ROTATION_ANGLES = (0, 90, 180, 270)      # reference sevir/sevir.py:1047
_M64 = (1 << 64) - 1


def _mix64(x):
    """splitmix64 finaliser: one well-mixed 64-bit word from another"""
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def augment_params(mode, seed, epoch, sequence_index):
    """(hflip, vflip, angle_degrees) of ONE sequence for aug_mode `mode` ("1": angle ~ U(-180, 180); "2": angle from
    {0, 90, 180, 270}; reference sevir/sevir.py:1037-1048).

    A pure function of its arguments: the draws come from a torch.Generator seeded from (seed, epoch, global sequence
    index) and nothing else, so the transform of a sequence does not depend on batch size, shard count, rank, prefetch
    depth or the order of calls.  The draws are made the way the reference's transforms make them — `torch.rand(1) <
    0.5` for each flip (RandomHorizontalFlip / RandomVerticalFlip), `uniform_(-180, 180)` for RandomRotation, a uniform
    choice among the four angles for TransformsFixRotation.  Bit parity of the random STREAM with the reference is
    neither possible nor a goal: there the numbers come from the global generators of whichever DataLoader worker
    happens to serve the sample."""
    mode = str(mode)
    if mode not in AUG_MODES:
        raise NotImplementedError(f"aug_mode {mode!r}: the reference knows {AUG_MODES}")
    if mode == "0":
        return (False, False, 0.0)
    g = torch.Generator()
    g.manual_seed(_mix64(_mix64(_mix64(int(seed) & _M64) ^ (int(epoch) & _M64)) ^ (int(sequence_index) & _M64)))
    hflip = bool(torch.rand(1, generator=g) < 0.5)
    vflip = bool(torch.rand(1, generator=g) < 0.5)
    if mode == "1":
        angle = float(torch.empty(1).uniform_(-180.0, 180.0, generator=g).item())
    else:
        angle = float(FIX_ROTATION_ANGLES[int(torch.randint(len(FIX_ROTATION_ANGLES), (1,), generator=g))])
    return (hflip, vflip, angle)


_QUARTER_TURNS = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))


def transform_rows(params):
    """[(hflip, vflip, angle_degrees)] -> fp32 (B, 4) rows (cos, sin, hflip, vflip) of ops.vil_augment_u8_to_f32.
    cos and sin are taken in Python double and rounded to fp32 once, as torchvision builds its matrix; whole multiples
    of 90 degrees (all of mode "2") get the exact 0 / +-1, so that a square frame comes out as torch.rot90 of itself."""
    rows = torch.empty((len(params), 4), dtype=torch.float32)
    for i, (hflip, vflip, angle) in enumerate(params):
        q = angle / 90.0
        if q == int(q):
            c, s = _QUARTER_TURNS[int(q) % 4]
        else:
            th = math.radians(angle)
            c, s = math.cos(th), math.sin(th)
        rows[i, 0], rows[i, 1], rows[i, 2], rows[i, 3] = c, s, float(bool(hflip)), float(bool(vflip))
    return rows


class SEVIRFrameLoader:
    def __init__(self, events_u8, batch_size, seq_len=1, stride=1, layout="NTHW", shuffle=False,
                 shuffle_seed=1, device=None, num_shard=1, rank=0, aug_mode="0", aug_seed=0, presample=None,
                 downsample_dict=None, rescale_method="01"):
        if presample is not None and downsample_dict is not None:
            raise NotImplementedError("presample and downsample_dict together: no reference config uses downsample_dict")
        if rescale_method not in RESCALE:
            raise ValueError(f"Invalid rescale option: {rescale_method}.")
        if downsample_dict is not None and set(downsample_dict) != {"vil"}:
            raise NotImplementedError(f"downsample_dict for {sorted(downsample_dict)}: only 'vil' is loaded")
        self.presample = None if presample is None else _factors(presample, "presample")
        self.downsample = None if downsample_dict is None else _factors(downsample_dict["vil"], "downsample_dict['vil']")
        self.rescale_method = rescale_method
        if layout not in LAYOUTS:
            raise NotImplementedError(f"layout {layout!r}: the reference's change_layout_torch knows {sorted(LAYOUTS)}")
        if str(aug_mode) not in AUG_MODES:
            raise NotImplementedError(f"aug_mode {aug_mode!r}: the reference knows {AUG_MODES}")
        self.aug_mode, self.aug_seed, self.epoch = str(aug_mode), int(aug_seed), 0
        self.layout = layout
        if hasattr(events_u8, "read") and hasattr(events_u8, "event_shape"):
            # an event store (catalog + files): events are read on demand; shuffling is the catalog's job
            self.store, self.events = events_u8, None
            self.n_events = len(events_u8)
            self.raw_frames = events_u8.event_shape[2]
        else:
            ev = np.ascontiguousarray(events_u8)
            assert ev.dtype == np.uint8 and ev.ndim == 4, "events must be uint8 (N_ev, H, W, T)"
            if shuffle:
                ev = ev[np.random.RandomState(shuffle_seed).permutation(ev.shape[0])]
            self.store, self.events = None, ev
            self.n_events = ev.shape[0]
            self.raw_frames = ev.shape[3]
        # with presample the dataset is the low-resolution one: its frames are the raw frames 0, ft, 2 ft, ...
        self.raw_seq_len = self.raw_frames if self.presample is None else -(-self.raw_frames // self.presample[0])
        self._cache = {}
        self.batch_size, self.seq_len, self.stride = int(batch_size), int(seq_len), int(stride)
        self.device = torch.device(device) if device is not None else None
        self.num_shard, self.rank = int(num_shard), int(rank)

    @property
    def num_seq_per_event(self):
        return 1 + (self.raw_seq_len - self.seq_len) // self.stride

    @property
    def total_num_seq(self):
        return int(self.num_seq_per_event * self.n_events)

    def __len__(self):
        return (self.total_num_seq // self.batch_size) // self.num_shard

    def sample_indices(self, index):
        """[(event_idx, seq_idx)] of batch `index` — reference _idx_sample :992-1003."""
        event_idx = (index * self.batch_size) // self.num_seq_per_event
        seq_idx = (index * self.batch_size) % self.num_seq_per_event
        out = []
        while len(out) < self.batch_size:
            out.append((event_idx, seq_idx))
            seq_idx += 1
            if seq_idx >= self.num_seq_per_event:
                event_idx += 1
                seq_idx = 0
        return out

    def set_epoch(self, epoch):
        """the epoch the augmentation draws are keyed on; a running prefetch() keeps the epoch it started with"""
        self.epoch = int(epoch)

    def sequence_ids(self, index):
        """global sequence indices (event * num_seq_per_event + seq) of this rank's batch `index`"""
        n = self.num_seq_per_event
        return [e * n + s for e, s in self.sample_indices(index * self.num_shard + self.rank)]

    def frame_ids(self, index):
        """int64 (B, seq_len): the frame (event * raw_seq_len + its position in the event; the pooled frames with
        presample) behind every frame of this rank's batch `index`.  Two batch frames with one id are the same pixels
        as long as aug_mode is "0": what a cache of per-frame results keys on"""
        idx = self.sample_indices(index * self.num_shard + self.rank)
        first = np.asarray([e * self.raw_seq_len + s * self.stride for e, s in idx], dtype=np.int64)
        return first[:, None] + np.arange(self.seq_len, dtype=np.int64)[None, :]

    def batch_augment_params(self, index, epoch=None):
        """[(hflip, vflip, angle)] of this rank's batch `index`"""
        epoch = self.epoch if epoch is None else epoch
        return [augment_params(self.aug_mode, self.aug_seed, epoch, i) for i in self.sequence_ids(index)]

    def batch_transform_rows(self, index, epoch=None):
        """host fp32 (B, 4) rows of this rank's batch `index`; None with aug_mode "0", which builds no rows and runs the
        plain conversion kernel"""
        if self.aug_mode == "0":
            return None
        return transform_rows(self.batch_augment_params(index, epoch))

    def _convert(self, u8_dev, rows_dev):
        """device uint8 'NHWT' batch (+ transform rows unless aug_mode is "0") -> the batch the loader yields"""
        factors, mode = (self.presample, "max") if self.presample else (self.downsample, "mean")
        if factors is None and self.rescale_method == "01":
            if rows_dev is None:
                x = ops.vil_u8_to_f32(u8_dev, PREPROCESS_SCALE_01["vil"])
            else:
                x = ops.vil_augment_u8_to_f32(u8_dev, rows_dev, PREPROCESS_SCALE_01["vil"])
        else:
            scale, offset = RESCALE[self.rescale_method]
            x = ops.vil_pool_u8_to_f32(u8_dev, factors or (1, 1, 1), mode, rows_dev, scale["vil"], offset["vil"])
        return self._wrap(LAYOUTS[self.layout](x))

    @staticmethod
    def process_data_dict_back(data_dict, data_types=None, rescale="01"):
        """undo the preprocessing (reference :797-826): x / scale - offset, on whatever device the tensors are on"""
        if rescale not in RESCALE:
            raise ValueError(f"Invalid rescale option: {rescale}.")
        scale, offset = RESCALE[rescale]
        for key in (data_dict.keys() if data_types is None else data_types):
            data_dict[key] = data_dict[key].float() / scale[key] - offset[key]
        return data_dict

    def _wrap(self, x):
        return {"vil": x}

    def batch_u8(self, index):
        """uint8 (B, H, W, seq_len) host batch, before preprocessing: what crosses the bus.  With presample it is the raw
        span under the sequence, (B, H, W, ft * (seq_len - 1) + 1) from raw frame ft * seq_idx * stride."""
        idx = self.sample_indices(index * self.num_shard + self.rank)
        ft = 1 if self.presample is None else self.presample[0]
        span = ft * (self.seq_len - 1) + 1
        return np.stack([self._event(e)[:, :, ft * s * self.stride:ft * s * self.stride + span] for e, s in idx], 0)

    def _event(self, e):
        if self.events is not None:
            return self.events[e]
        ev = self._cache.get(e)
        if ev is None:
            if len(self._cache) >= 4:                 # consecutive batches walk the events in order
                self._cache.pop(next(iter(self._cache)))
            ev = self._cache[e] = self.store.read(e)
            if ev.dtype != np.uint8:
                raise TypeError(f"event {e}: expected uint8, got {ev.dtype}")
        return ev

    def prefetch(self, depth=2, start=0):
        """iterate (from batch `start`) with the host gather + uint8 H2D copy of the next `depth` batches running
        ahead on a copy stream"""
        return _Prefetcher(self, depth, start)

    def __getitem__(self, index):
        if index >= len(self):
            raise IndexError(index)
        u8 = torch.from_numpy(self.batch_u8(index))
        if self.device is None or self.device.type != "cuda":
            raise RuntimeError("SEVIRFrameLoader preprocesses on the GPU: pass device='cuda:N'")
        u8 = u8.to(self.device, non_blocking=True)
        rows = self.batch_transform_rows(index)
        return self._convert(u8, None if rows is None else rows.to(self.device, non_blocking=True))

    def __iter__(self):
        for i in range(len(self)):
            yield self[i]


class _Prefetcher:
    """Background thread: gather batch i+1 into a pinned uint8 buffer and start its H2D copy on a side stream while
    the consumer trains on batch i; the u8 -> fp32/255 + layout kernel runs on the consumer's stream after an event
    wait.  `depth` pinned buffers / device buffers are recycled.  With augmentation on, the (B, 4) transform rows of a
    batch travel with it: their own pinned buffer, a copy on the same stream in front of the same event.  A batch may be
    shorter than the first one (the last batch of a loader that keeps its remainder): it uses the head of its slot."""

    def __init__(self, loader, depth=2, start=0):
        if loader.device is None or loader.device.type != "cuda":
            raise RuntimeError("prefetch() needs a CUDA(HIP) device")
        self.loader, self.depth, self.start = loader, max(1, int(depth)), max(0, int(start))

    def __iter__(self):
        ld = self.loader
        n = len(ld)
        if n == 0 or self.start >= n:
            return
        dev = ld.device
        shape = ld.batch_u8(0).shape
        pinned = [torch.empty(shape, dtype=torch.uint8).pin_memory() for _ in range(self.depth + 1)]
        dbuf = [torch.empty(shape, dtype=torch.uint8, device=dev) for _ in range(self.depth + 1)]
        aug, epoch = ld.aug_mode != "0", ld.epoch
        if aug:
            pinned_xf = [torch.empty((shape[0], 4), dtype=torch.float32).pin_memory() for _ in range(self.depth + 1)]
            dbuf_xf = [torch.empty((shape[0], 4), dtype=torch.float32, device=dev) for _ in range(self.depth + 1)]
        free_slots = queue.Queue()
        for i in range(self.depth + 1):
            free_slots.put(i)
        ready = queue.Queue(maxsize=self.depth)
        copy_stream = torch.cuda.Stream(device=dev)
        stop = threading.Event()

        def producer():
            try:
                torch.cuda.set_device(dev)
                for i in range(self.start, n):
                    if stop.is_set():
                        return
                    slot = free_slots.get()
                    u8 = ld.batch_u8(i)
                    b = u8.shape[0]
                    pinned[slot].numpy()[:b] = u8
                    if aug:
                        pinned_xf[slot][:b] = ld.batch_transform_rows(i, epoch)
                    with torch.cuda.stream(copy_stream):
                        dbuf[slot][:b].copy_(pinned[slot][:b], non_blocking=True)
                        if aug:
                            dbuf_xf[slot][:b].copy_(pinned_xf[slot][:b], non_blocking=True)
                        ev = torch.cuda.Event()
                        ev.record(copy_stream)
                    ready.put((slot, b, ev, None))
                ready.put((None, 0, None, None))
            except BaseException as e:      # surface loader errors in the consumer
                ready.put((None, 0, None, e))

        th = threading.Thread(target=producer, daemon=True)
        th.start()
        try:
            while True:
                slot, b, ev, err = ready.get()
                if err is not None:
                    raise err
                if slot is None:
                    break
                torch.cuda.current_stream(dev).wait_event(ev)
                out = ld._convert(dbuf[slot][:b], dbuf_xf[slot][:b] if aug else None)
                done = torch.cuda.Event()
                done.record(torch.cuda.current_stream(dev))
                yield out
                done.synchronize()           # the conversion kernel has consumed the slot: recycle it
                free_slots.put(slot)
        finally:
            stop.set()                       # an early `break` in the consumer: unblock and retire the producer
            try:
                while True:
                    ready.get_nowait()
            except queue.Empty:
                pass
            for i in range(self.depth + 1):
                free_slots.put(i)
            th.join(timeout=5)
