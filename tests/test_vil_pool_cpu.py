"""CPU side of the loader's pooling conversion: the numpy restatement against torch's pooling on the CPU, the bookkeeping of
a `presample` loader against a loader over host-pooled events, the new keyword arguments, the ABI of the new entry point
and the --presample option of the two entry points."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import vil_pool_ref as P
from weatherforecastingtoolkit_amd import _lib

CASES = [((2, 13, 10, 7), (2, 3, 3), P.SCALE_01, P.OFFSET_01),
         ((2, 12, 12, 5), (2, 3, 3), P.SCALE_01, P.OFFSET_01),
         ((1, 9, 9, 3), (2, 3, 3), P.SCALE_01, P.OFFSET_01),
         ((2, 8, 12, 4), (1, 2, 4), P.SCALE_SEVIR, P.OFFSET_SEVIR)]


def _sevir():
    from weatherforecastingtoolkit_amd.pipeline.datasets.sevire import sevir
    return sevir


def _u8(shape, seed=0):
    return np.random.RandomState(seed).randint(0, 256, shape, dtype=np.uint8)


@pytest.mark.parametrize("shape,f,scale,offset", CASES)
def test_restatement_equals_torch_pooling(shape, f, scale, offset):
    u8 = _u8(shape)
    x = torch.from_numpy(u8[..., ::f[0]]).permute(0, 3, 1, 2)                 # 'NTHW'
    v = np.float32(scale) * (x.float() + np.float32(offset))
    want_max = F.max_pool2d(v, (f[1], f[2]), ceil_mode=True)
    want_mean = F.avg_pool2d(v, (f[1], f[2]))
    got_max, got_mean = P.pool(u8, f, "max", scale, offset), P.pool(u8, f, "mean", scale, offset)
    assert got_max.dtype == np.float32 and got_max.shape == tuple(want_max.shape)
    assert got_max.tobytes() == want_max.contiguous().numpy().tobytes()
    assert got_mean.shape == tuple(want_mean.shape) == (shape[0], -(-shape[3] // f[0]), shape[1] // f[1], shape[2] // f[2])
    assert got_mean.tobytes() == want_mean.contiguous().numpy().tobytes()


def test_pool_max_u8_reduces_edge_blocks_over_their_pixels_inside():
    u8 = _u8((1, 4, 5, 3), 1)
    got = P.pool_max_u8(u8, (2, 3, 3))
    assert got.dtype == np.uint8 and got.shape == (1, 2, 2, 2)
    assert got[0, 1, 1, 1] == u8[0, 3:, 3:, 2].max() and got[0, 0, 1, 0] == u8[0, :3, 3:, 0].max()


@pytest.mark.parametrize("seq_len", [1, 2, 5])
@pytest.mark.parametrize("stride", [1, 2])
def test_presample_loader_is_the_loader_over_the_pooled_events(seq_len, stride):
    S = _sevir()
    ev = _u8((3, 12, 12, 9), 3)
    f = (2, 3, 3)
    lr = P.pool_max_u8(ev, f)
    assert lr.shape == (3, 4, 4, 5)
    a = S.SEVIRFrameLoader(ev, 2, seq_len=seq_len, stride=stride, presample=f)       # seq_len 5: 3 sequences in all
    b = S.SEVIRFrameLoader(lr, 2, seq_len=seq_len, stride=stride)
    assert a.raw_seq_len == 5 == b.raw_seq_len
    assert a.num_seq_per_event == b.num_seq_per_event and len(a) == len(b) >= 1
    assert a.total_num_seq == b.total_num_seq
    for i in range(len(a)):
        assert a.sample_indices(i) == b.sample_indices(i) and a.sequence_ids(i) == b.sequence_ids(i)
        raw = a.batch_u8(i)
        assert raw.shape == (2, 12, 12, 2 * (seq_len - 1) + 1)
        for k, (e, s) in enumerate(a.sample_indices(i)):
            assert np.array_equal(raw[k], ev[e][:, :, 2 * s * stride:2 * s * stride + 2 * (seq_len - 1) + 1])
        assert np.array_equal(P.pool_max_u8(raw, f), b.batch_u8(i))       # the same frames, whichever side pools


def test_default_arguments_change_nothing():
    S = _sevir()
    ev = _u8((3, 12, 12, 9), 3)
    a, b = S.SEVIRFrameLoader(ev, 4, seq_len=2, stride=3), S.SEVIRFrameLoader(ev, 4, 2, 3, presample=None,
                                                                             downsample_dict=None, rescale_method="01")
    assert a.raw_seq_len == b.raw_seq_len == 9 and len(a) == len(b)
    assert np.array_equal(a.batch_u8(1), b.batch_u8(1)) and a.batch_u8(1).shape == (4, 12, 12, 2)
    d = S.SEVIRFrameLoader(ev, 4, seq_len=2, stride=3, downsample_dict={"vil": (2, 3, 3)})
    assert d.raw_seq_len == 9 and d.batch_u8(0).shape == (4, 12, 12, 2)      # applied to the sequence, on the device


def test_keyword_refusals():
    S = _sevir()
    ev = _u8((3, 12, 12, 9), 3)
    with pytest.raises(NotImplementedError):
        S.SEVIRFrameLoader(ev, 4, presample=(2, 3, 3), downsample_dict={"vil": (1, 2, 2)})
    with pytest.raises(ValueError):
        S.SEVIRFrameLoader(ev, 4, rescale_method="minmax")
    with pytest.raises(ValueError):
        S.SEVIRFrameLoader(ev, 4, presample=(2, 0, 3))
    with pytest.raises(ValueError):
        S.SEVIRFrameLoader(ev, 4, presample=(2, 3))
    from weatherforecastingtoolkit_amd.pipeline.datasets.sevir.sevir import SEVIRLightningDataModule
    dm = SEVIRLightningDataModule(ev, dataset_name="sevirlr", batch_size=2, seq_len=2, stride=1, presample=(2, 3, 3),
                                  downsample_dict={"vil": (1, 2, 2)})
    with pytest.raises(NotImplementedError):
        dm.setup()
    dm = SEVIRLightningDataModule(ev, dataset_name="sevirlr", batch_size=2, seq_len=2, stride=1, presample=(2, 3, 3),
                                  rescale_method="sevir")
    dm.setup()
    train = dm.train_dataloader()
    assert train.presample == (2, 3, 3) and train.rescale_method == "sevir" and train.raw_seq_len == 5
    assert dm.num_train_samples + dm.num_val_samples == 3 * 4


def test_lr_presample_truth_table():
    S = _sevir()
    from weatherforecastingtoolkit_amd.pipeline.datasets.sevir import sevir as S2
    assert S2.lr_presample is S.lr_presample
    assert S.lr_presample("sevir_lr", (384, 384, 49)) == (2, 3, 3)
    assert S.lr_presample("sevirlr", (384, 384, 49)) == (2, 3, 3)
    assert S.lr_presample("sevirlr", [384, 384, 49]) == (2, 3, 3)
    assert S.lr_presample("sevir", (384, 384, 49)) is None
    assert S.lr_presample("sevir_lr", (128, 128, 25)) is None
    assert S.lr_presample("sevirlr", (128, 128, 25)) is None
    assert S.lr_presample("sevir_lr", (384, 384, 25)) is None
    assert S.lr_presample("sevir_lr", (192, 192, 49)) is None


def test_rescale_tables_and_process_data_dict_back():
    S = _sevir()
    assert S.PREPROCESS_SCALE_SEVIR["vil"] == 1 / 47.54 and S.PREPROCESS_OFFSET_SEVIR["vil"] == -33.44
    u8 = torch.arange(256, dtype=torch.uint8).reshape(1, 16, 16, 1)
    for rescale, scale, offset in (("01", 1 / 255, 0.0), ("sevir", 1 / 47.54, -33.44)):
        x = np.float32(scale) * (u8.float() + np.float32(offset))             # preprocess_data_dict
        back = S.SEVIRFrameLoader.process_data_dict_back({"vil": x.clone(), "mask": u8}, ["vil"], rescale)
        assert back["mask"] is u8
        assert back["vil"].dtype == torch.float32
        # two roundings forth, two back: a few ulps of 255
        assert torch.allclose(back["vil"], u8.float(), rtol=0, atol=1e-3)
        assert torch.equal(back["vil"].round().to(torch.uint8), u8)
    assert set(S.SEVIRFrameLoader.process_data_dict_back({"vil": torch.zeros(2)})) == {"vil"}
    with pytest.raises(ValueError):
        S.SEVIRFrameLoader.process_data_dict_back({"vil": torch.zeros(2)}, rescale="minmax")


def test_abi_of_the_new_entry_point():
    d = _lib.parse_header()
    assert "wfae_vil_pool_u8_to_f32" in d
    _, argtypes, argnames = d["wfae_vil_pool_u8_to_f32"]
    assert argnames == ["src", "xf", "dst", "NB", "H", "W", "T", "ft", "fh", "fw", "mode", "scale", "offset", "stream"]
    assert argtypes[11] is ctypes.c_float and argtypes[12] is ctypes.c_float and argtypes[10] is ctypes.c_int
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "wfae_vil_pool_u8_to_f32")
    lib = _lib.load()
    assert lib.wfae_version() == 103
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    fn = lib.wfae_vil_pool_u8_to_f32
    err = lib.wfae_last_error_string
    NULL, SHAPE, UNSUPPORTED = -2, -1, -5
    for src, dst in ((None, p), (p, None)):
        assert fn(src, None, dst, 1, 2, 2, 1, 1, 1, 1, 0, 1.0, 0.0, None) == NULL and b"null" in err()
    for ft, fh, fw in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1)):
        assert fn(p, None, p, 1, 2, 2, 1, ft, fh, fw, 0, 1.0, 0.0, None) == SHAPE and b"factors" in err()
    for nb, h, w, t in ((0, 2, 2, 1), (1, 0, 2, 1), (1, 2, 0, 1), (1, 2, 2, 0)):
        assert fn(p, None, p, nb, h, w, t, 1, 1, 1, 0, 1.0, 0.0, None) == SHAPE and b"bad shape" in err()
    for mode in (2, -1):
        assert fn(p, None, p, 1, 2, 2, 1, 1, 1, 1, mode, 1.0, 0.0, None) == UNSUPPORTED and b"mode" in err()
    assert fn(p, None, p, 1, 2, 4, 1, 1, 3, 1, 1, 1.0, 0.0, None) == SHAPE and b"mean" in err()      # fh > H
    assert fn(p, None, p, 1, 4, 2, 1, 1, 1, 3, 1, 1.0, 0.0, None) == SHAPE and b"mean" in err()      # fw > W
    assert fn(p, None, p, 1, 65536, 65536, 1, 1, 1, 1, 0, 1.0, 0.0, None) == SHAPE and b"frame" in err()
    hdr = open(_lib.HEADER).read()
    for word in ("acc = acc + v(", "(float)(fh * fw)", "scale * ((float)b + offset)", "exactly 0.f"):
        assert word in hdr, word


def test_ops_wrapper_raises_without_a_gpu():
    from weatherforecastingtoolkit_amd import ops
    with pytest.raises(_lib.WfaeError):
        ops.vil_pool_u8_to_f32(torch.zeros(2, 6, 6, 1, dtype=torch.uint8), (1, 3, 3))
    with pytest.raises(_lib.WfaeError):
        ops.vil_pool_u8_to_f32(torch.zeros(2, 6, 6, 1, dtype=torch.uint8), (1, 3, 3), mode="median")


@pytest.mark.parametrize("module", ["ae_v2.train", "ae_v2_2.train_data2"])
def test_presample_option_of_the_entry_points(module):
    import importlib
    m = importlib.import_module("weatherforecastingtoolkit_amd.experiments." + module)
    parse, resolve = m.parse_presample, m.resolve_presample
    assert parse("auto") == "auto" and parse("AUTO") == "auto" and parse("none") is None
    assert parse("2,3,3") == (2, 3, 3) and parse(" 1, 2 ,4") == (1, 2, 4)
    for bad in ("", "2,3", "2,3,3,1", "2,0,3", "a,b,c", "2.5,3,3", "yes"):
        with pytest.raises(ValueError):
            parse(bad)
    raw, lr = (384, 384, 49), (128, 128, 25)
    assert resolve(parse("auto"), "sevir_lr", raw) == ((2, 3, 3), lr)
    assert resolve(parse("auto"), "sevirlr", raw) == ((2, 3, 3), lr)
    assert resolve(parse("auto"), "sevir", raw) == (None, raw)
    assert resolve(parse("auto"), "sevir_lr", lr) == (None, lr)           # a store that is low-resolution already
    assert resolve(parse("none"), "sevir_lr", raw) == (None, raw)
    assert resolve(parse("1,2,2"), "sevir", raw) == ((1, 2, 2), (192, 192, 49))
    assert resolve(parse("2,5,5"), "sevir", raw) == ((2, 5, 5), (77, 77, 25))
    assert m.presample_line((2, 3, 3), raw, lr) == "presample (2, 3, 3): 384x384x49 -> 128x128x25"
    # the option is declared with that parser, default auto
    import inspect
    src = inspect.getsource(m.main)
    assert '"--presample", type=parse_presample, default="auto"' in src
