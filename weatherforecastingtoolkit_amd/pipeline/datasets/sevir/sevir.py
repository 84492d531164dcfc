"""The reference's SECOND SEVIR loader (pipeline/datasets/sevir/sevir.py — the package name without the `e`):
`SEVIRLightningDataModule`, what experiments/ae_v2_2/train_data2.py trains on, without Lightning.

Contract reproduced (reference lines):
  * a sample is ONE sequence, `_idx_sample(index)` of the batch-size-1 loader        :1010-1033, 1052-1054
  * train / val = torch.utils.data.random_split(dataset, [1 - val_ratio, val_ratio],
    torch.Generator().manual_seed(seed)) — that function is called, its indices kept  :1182-1185
  * train batches: a fresh permutation every epoch (DataLoader(shuffle=True)); here
    from a generator seeded with (seed, epoch), so an epoch can be replayed           :1206-1210
  * val / test keep their order and are never augmented                               :1203, 1212-1222
  * the last batch keeps its remainder (DataLoader's drop_last=False)
  * a batch is a bare tensor in the requested layout, not a dict                      :1054-1064
  * train events are shuffled once (shuffle_seed 1), test events are not              :1169, 1192
  * aug_mode "1" / "2": flips + rotation per sequence, "0": none                      :1035-1050
  * presample / downsample_dict / rescale_method: the frame loader's, passed through (presample=(2, 3, 3) over raw
    SEVIR is the 'sevirlr' dataset; `lr_presample` tells when it applies)
The gather, the prefetcher and the augmentation are `sevire.sevir.SEVIRFrameLoader`'s: the host gathers uint8
sequences, the device kernel converts, re-lays and transforms them in one pass.  Events are a uint8 array or a
`catalog.CatalogEventStore`; the test events are whatever store the caller passes for them (the date split is the
catalog's job).  `num_workers` is accepted and ignored: there are no worker processes, `prefetch()` runs ahead instead.
"""
from __future__ import annotations

import torch
from torch.utils.data import random_split

from ..sevire.sevir import _M64, SEVIRFrameLoader, _mix64, lr_presample  # noqa: F401  (lr_presample: for the callers)

# the SEVIR VIL colour scale as runs of byte values: (first value of the run, (R, G, B)); a run ends where the next begins
VIL_RUNS = ((0, (77, 77, 77)), (16, (40, 190, 40)), (31, (25, 150, 25)), (59, (10, 105, 10)), (74, (10, 75, 10)),
            (100, (245, 245, 0)), (133, (237, 172, 0)), (160, (240, 110, 0)), (181, (160, 0, 0)), (219, (231, 0, 255)))


def vil_lut():
    """The reference's `vil_cmap()` (:1237-1268) in table form: uint8 (256, 3), row v the RGB that
    `imshow(u8, cmap=cmap, norm=norm)` paints for the byte value v, i.e. `cmap(norm(v), bytes=True)[:, :3]` of its
    ListedColormap + BoundaryNorm(VIL_LEVELS, 10).  Ten runs; value 255 takes the "over" colour, which the reference sets
    to the last bin's.  tests/golden/g23_panel_luts.npz holds the table as matplotlib evaluates it."""
    lut = torch.empty((256, 3), dtype=torch.uint8)
    for (start, rgb), (end, _) in zip(VIL_RUNS, VIL_RUNS[1:] + ((256, None),)):
        lut[start:end] = torch.tensor(rgb, dtype=torch.uint8)
    return lut


class SequenceBatchLoader(SEVIRFrameLoader):
    """Batches of `batch_size` single sequences in a given order of global sequence indices (`order`), the last one
    short if the count does not divide; `shuffle_order` draws a fresh permutation of `order` per epoch."""

    def __init__(self, events_u8, order, batch_size, seq_len, stride, layout, shuffle_events=False, device=None,
                 aug_mode="0", seed=0, shuffle_order=False, ret_contiguous=True, presample=None, downsample_dict=None,
                 rescale_method="01"):
        super().__init__(events_u8, batch_size, seq_len, stride, layout, shuffle=shuffle_events, device=device,
                         aug_mode=aug_mode, aug_seed=seed, presample=presample, downsample_dict=downsample_dict,
                         rescale_method=rescale_method)
        self.base_order = list(range(self.total_num_seq)) if order is None else [int(i) for i in order]
        self.seed, self.shuffle_order, self.ret_contiguous = int(seed), bool(shuffle_order), bool(ret_contiguous)
        self.set_epoch(0)

    def set_epoch(self, epoch):
        super().set_epoch(epoch)
        if self.shuffle_order:
            g = torch.Generator().manual_seed(_mix64(_mix64(self.seed & _M64) ^ (self.epoch & _M64)))
            self.order = [self.base_order[i] for i in torch.randperm(len(self.base_order), generator=g).tolist()]
        else:
            self.order = self.base_order

    def __len__(self):
        return (len(self.order) + self.batch_size - 1) // self.batch_size

    def sample_indices(self, index):
        ids = self.order[index * self.batch_size:(index + 1) * self.batch_size]
        return [divmod(i, self.num_seq_per_event) for i in ids]

    def _wrap(self, x):
        return x.contiguous() if self.ret_contiguous else x


class SEVIRLightningDataModule:
    def __init__(self, events, test_events=None, *, seq_len=25, stride=12, layout="NTHWC", aug_mode="0",
                 ret_contiguous=True, dataset_name="sevir", val_ratio=0.1, batch_size=1, num_workers=1, seed=0,
                 device=None, presample=None, downsample_dict=None, rescale_method="01"):
        if dataset_name not in ("sevir", "sevirlr"):
            raise ValueError(f"Wrong dataset name {dataset_name}. Must be 'sevir' or 'sevirlr'.")
        assert layout[0] == "N"
        self.events, self.test_events = events, test_events
        self.dataset_name, self.seq_len, self.stride, self.layout = dataset_name, seq_len, stride, layout
        self.aug_mode, self.ret_contiguous, self.val_ratio = str(aug_mode), ret_contiguous, val_ratio
        self.batch_size, self.num_workers, self.seed, self.device = batch_size, num_workers, seed, device
        self.presample, self.downsample_dict, self.rescale_method = presample, downsample_dict, rescale_method
        self.sevir_train = self.sevir_val = self.sevir_test = None

    def prepare_data(self):
        """nothing to fetch: the events are handed in"""

    def _loader(self, events, order, **kw):
        return SequenceBatchLoader(events, order, self.batch_size, self.seq_len, self.stride, self.layout,
                                   device=self.device, seed=self.seed, ret_contiguous=self.ret_contiguous,
                                   presample=self.presample, downsample_dict=self.downsample_dict,
                                   rescale_method=self.rescale_method, **kw)

    def setup(self, stage=None):
        if stage in (None, "fit"):
            probe = self._loader(self.events, None, shuffle_events=True)
            ev = self.events if probe.events is None else probe.events     # an array: shuffled once, shared by both loaders
            train, val = random_split(range(probe.total_num_seq), [1 - self.val_ratio, self.val_ratio],
                                      generator=torch.Generator().manual_seed(self.seed))
            self.train_indices, self.val_indices = list(train.indices), list(val.indices)
            self.sevir_train = self._loader(ev, self.train_indices, aug_mode=self.aug_mode, shuffle_order=True)
            self.sevir_val = self._loader(ev, self.val_indices)
        if stage in (None, "test") and self.test_events is not None:
            self.sevir_test = self._loader(self.test_events, None)

    def _get(self, name):
        ld = getattr(self, name)
        if ld is None:
            raise RuntimeError(f"{name}: call setup() first" + (" and pass test_events" if name == "sevir_test" else ""))
        return ld

    def train_dataloader(self):
        """the train loader; call its set_epoch(e) in front of every epoch for that epoch's order and transforms"""
        return self._get("sevir_train")

    def val_dataloader(self):
        return self._get("sevir_val")

    def test_dataloader(self):
        return self._get("sevir_test")

    @property
    def num_train_samples(self):
        return len(self._get("sevir_train").order)

    @property
    def num_val_samples(self):
        return len(self._get("sevir_val").order)

    @property
    def num_test_samples(self):
        return len(self._get("sevir_test").order)
