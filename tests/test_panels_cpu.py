"""CPU: the host side of `--plots DIR` — the two colour tables against matplotlib's (G23), the PNG writer read back by
a decoder written here (and by PIL where it is installed), the reference's plot cadence, label sanitising, the sink's
default, the ABI refusals before any launch, and tests/panels_ref.py against the reference's own three numpy lines."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import panels_ref as R
from weatherforecastingtoolkit_amd import _lib
from weatherforecastingtoolkit_amd.pipeline import helpers
from weatherforecastingtoolkit_amd.pipeline.datasets.sevir.sevir import vil_lut


def test_luts_equal_matplotlibs():
    g = np.load(R.GOLDEN)
    vil, reds = vil_lut(), helpers.reds_lut()
    assert vil.dtype == torch.uint8 and reds.dtype == torch.uint8 and vil.shape == reds.shape == (256, 3)
    assert np.array_equal(vil.numpy(), g["vil"]) and np.array_equal(reds.numpy(), g["reds"])
    # what the issue states about the table: ten runs, their starts, first and last colour, 255 = the last bin
    assert g["vil_starts"].tolist() == [0, 16, 31, 59, 74, 100, 133, 160, 181, 219]
    assert tuple(g["vil"][0]) == (77, 77, 77) and tuple(g["vil"][254]) == tuple(g["vil"][255]) == (231, 0, 255)


def test_package_does_not_import_matplotlib():
    import pathlib
    import re
    for f in pathlib.Path(_lib._PKG).rglob("*.py"):
        assert not re.search(r"^\s*(import|from)\s+matplotlib", f.read_text(), flags=re.M), f


@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (33, 130)])
def test_png_round_trip(tmp_path, h, w):
    rgb = np.random.default_rng(h * 1000 + w).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    plain, framed = str(tmp_path / "plain.png"), str(tmp_path / "framed.png")
    helpers.write_png(plain, rgb.tobytes(), w, h)
    helpers.write_png(framed, R.scanlines(rgb[None])[0].tobytes(), w, h)
    assert open(plain, "rb").read() == open(framed, "rb").read()
    assert np.array_equal(R.decode_png(plain), rgb)
    assert sorted(os.listdir(tmp_path)) == ["framed.png", "plain.png"]          # the temporary name is gone
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        with Image.open(plain) as im:
            assert im.mode == "RGB" and im.size == (w, h)
            assert np.array_equal(np.asarray(im), rgb)
    with pytest.raises(ValueError):
        helpers.write_png(plain, rgb.tobytes()[:-1], w, h)


def test_plot_due_is_the_references_cadence():
    # (counter, fraction, total) -> due, worked out from  interval = int(fraction * total); counter % interval == 0
    table = [
        (0, 0.01, 1000, True),      # interval 10
        (5, 0.01, 1000, False),
        (10, 0.01, 1000, True),
        (1010, 0.01, 1000, True),   # epoch * total + batch
        (1011, 0.01, 1000, False),
        (7, 0.05, 150, True),       # int(7.5) = 7
        (8, 0.05, 150, False),
        (3, 0.1, 12.5, True),       # a total scaled by limit_*_batches is a float: int(1.25) = 1
        (3, 0.1, 25.0, False),      # int(2.5) = 2
    ]
    for counter, fraction, total, want in table:
        interval = int(fraction * total)
        assert (counter % interval == 0) == want                                  # the table is the formula's
        assert helpers.plot_due(counter, fraction, total) == want, (counter, fraction, total)
    # the one deviation: interval == 0 (a short run), where the reference divides by zero, is an interval of 1
    for counter in (0, 1, 2, 17):
        assert int(0.01 * 4) == 0 and helpers.plot_due(counter, 0.01, 4)
        assert helpers.plot_due(counter, 0.05, 0)
    assert not helpers.plot_due(0, None, 100)                                     # prediff_mlp_sevir: null fraction


def test_label_sanitising():
    s = helpers.sanitise_label
    assert s("Train Reconstruction vs Original_epoch_0_batch_12") == "Train_Reconstruction_vs_Original_epoch_0_batch_12"
    assert s("Val_Reconstruction vs Original_epoch_3_batch_0") == "Val_Reconstruction_vs_Original_epoch_3_batch_0"
    assert s("../../etc/passwd") == "_.._etc_passwd" and "/" not in s("a/b\\c") and s("a/b\\c") == "a_b_c"
    assert s("...hidden") == "hidden" and s("") == "panel" and s("///") == "___" and s("é\n\0x") == "___x"
    assert len(s("x" * 500)) == 200


def test_panels_is_none_without_the_flag():
    from weatherforecastingtoolkit_amd.experiments.ae_v2 import train as ae_v2
    from weatherforecastingtoolkit_amd.experiments.ae_v2_2 import train as ae_v2_2
    from weatherforecastingtoolkit_amd.experiments.v1_experiments import (_ae_gan, _ae_gan_kl, _conv_disc, _convae,
                                                                          _convattn, _dlinear, _runner)
    assert _runner.Step.panels is None
    for mod in (_ae_gan, _ae_gan_kl, _conv_disc, _convae, _convattn, _dlinear):
        assert issubclass(mod.Model, _runner.Step) and mod.Model.panels is None
    from weatherforecastingtoolkit_amd import config as C
    for mod in (ae_v2, ae_v2_2):
        cfg = C.load(os.path.join(mod.HERE, "config.yaml"), mod.CARRIED_KEYS)
        cfg.trainer.total_train_steps = 10
        assert mod.Model(cfg).panels is None
    # no sink without a directory, and none for a rank other than 0
    tr = C.Cfg(max_epochs=2, accumulate_grad_batches=1, limit_val_batches=0.5)
    assert helpers.make_sink(None, 0, tr, 10, 4, 4) is None and helpers.make_sink("", 0, tr, 10, 4, 4) is None


def test_sink_totals_and_rank(tmp_path):
    from weatherforecastingtoolkit_amd import config as C
    tr = C.Cfg(max_epochs=3, accumulate_grad_batches=2, limit_val_batches=0.5)
    assert helpers.make_sink(str(tmp_path / "r1"), 1, tr, 10, 4, 5) is None and not (tmp_path / "r1").exists()
    sink = helpers.make_sink(str(tmp_path / "p"), 0, tr, 10, 4, 5)
    assert os.path.isdir(sink.dir) and sink.global_step == 0 and sink.epoch == 0
    # reference ae_v2/train.py:306-317: n * max_epochs / accumulate, int() without a limit, times the limit with one
    assert sink.total("train") == 10 and sink.total("val") == 4 * 3 / 2 * 0.5 and sink.total("test") == int(5 * 3 / 2)


def test_abi_refusals_before_any_launch():
    lib = _lib.load()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(buf)            # never dereferenced: every call below is refused on the host
    NULL, SHAPE, WS = -2, -1, -3
    render = lib.wfae_panel_render
    assert render(None, p, p, p, p, 1, 1, 1, 1, 1, 0, None) == NULL and b"null" in lib.wfae_last_error_string()
    for i in range(1, 5):
        args = [p] * 5
        args[i] = None
        assert render(*args, 1, 1, 1, 1, 1, 0, None) == NULL
    for b, nb, t, h, w, g in [(0, 1, 1, 1, 1, 0), (1, 1, 0, 1, 1, 0), (1, 1, 1, 0, 1, 0), (1, 1, 1, 1, -3, 0),
                              (2, 0, 1, 1, 1, 0), (2, 3, 1, 1, 1, 0), (2, -1, 1, 1, 1, 0), (1, 1, 1, 1, 1, -1),
                              (1, 1, 1, 20000, 40000, 0),          # 3 * 20000 * (1 + 120000) >= 2^31
                              (1, 1, 2, 2, 2, 2 ** 30)]:
        assert render(p, p, p, p, p, b, nb, t, h, w, g, None) == SHAPE, (b, nb, t, h, w, g)
        assert lib.wfae_panel_bytes(t, h, w, g) == 0 or not (1 <= nb <= b)
    assert lib.wfae_panel_bytes(1, 5, 7, 0) == 15 * 22 and lib.wfae_panel_bytes(3, 16, 16, 2) == 52 * (1 + 3 * 52)
    assert lib.wfae_panel_bytes(13, 128, 128, 2) == 388 * (1 + 3 * 1688)
    # the largest figure below 2^31 bytes is served, the next one is not
    assert lib.wfae_panel_bytes(1, 1, 238609293, 0) == 3 * (1 + 3 * 238609293) == 2 ** 31 - 8
    assert lib.wfae_panel_bytes(1, 1, 238609294, 0) == 0
    count = lib.wfae_range_count
    assert lib.wfae_range_count_workspace_bytes(0) == 0 and lib.wfae_range_count_workspace_bytes(1) == 8
    assert lib.wfae_range_count_workspace_bytes(100003) == 8 * 98 and lib.wfae_range_count_workspace_bytes(2 ** 40) == 8192
    assert count(None, 4, p, p, 64, None) == NULL and count(p, 4, None, p, 64, None) == NULL
    assert count(p, 4, p, None, 64, None) == NULL
    assert count(p, 0, p, p, 64, None) == SHAPE and count(p, -5, p, p, 64, None) == SHAPE
    assert count(p, 100003, p, p, 64, None) == WS and count(p, 4, p, p + 1, 64, None) == WS
    # the Python wrappers refuse host tensors: there is no CPU path
    from weatherforecastingtoolkit_amd import ops
    z = torch.zeros(1, 1, 2, 2)
    with pytest.raises(_lib.WfaeError):
        ops.panel_render(z, z, vil_lut(), helpers.reds_lut(), 1)
    with pytest.raises(_lib.WfaeError):
        ops.range_count(z)
    with pytest.raises(ValueError, match="B,T,1,H,W"):
        helpers.log_images(torch.zeros(1, 2, 3, 4, 4), torch.zeros(1, 2, 3, 4, 4), "x", None)


def test_ref_agrees_with_the_references_three_numpy_lines():
    """pipeline/helpers.py:181-183, transcribed literally, on a seeded tensor without NaN (where its cast is
    unspecified); +-inf and out-of-range values stay in"""
    x = R.edge_tensor((3, 2, 9, 11), seed=5)
    y = R.edge_tensor((3, 2, 9, 11), seed=6, offset=391)
    x[np.isnan(x)] = 0.25
    y[np.isnan(y)] = 0.75
    target, predicted = torch.from_numpy(x), torch.from_numpy(y)
    target_np = (target.clamp(0, 1) * 255).numpy().astype('uint8')
    pred_np = (predicted.clamp(0, 1) * 255).numpy().astype('uint8')
    diff_np = abs(target_np.astype(float) - pred_np.astype(float)).clip(0, 255).astype('uint8')
    assert np.array_equal(R.quantise(x), target_np) and np.array_equal(R.quantise(y), pred_np)
    vil, reds = R.luts()
    fig = R.render(y, x, 2, 2)
    hfig, wfig = R.figure_shape(2, 9, 11, 2)
    assert fig.shape == (2, hfig, wfig, 3) == (2, 31, 24, 3)
    for b in range(2):
        for t in range(2):
            x0 = t * 13
            assert np.array_equal(fig[b, 0:9, x0:x0 + 11], vil[target_np[b, t]])
            assert np.array_equal(fig[b, 11:20, x0:x0 + 11], vil[pred_np[b, t]])
            assert np.array_equal(fig[b, 22:31, x0:x0 + 11], reds[diff_np[b, t]])
    assert (fig[:, 9:11] == 255).all() and (fig[:, 20:22] == 255).all() and (fig[:, :, 11:13] == 255).all()
    assert R.quantise(np.array([np.nan, -np.inf, np.inf, 1.0, -0.0], dtype=np.float32)).tolist() == [0, 0, 255, 255, 0]
    assert R.range_count(np.array([np.nan, -np.inf, np.inf, 0.0, -0.0, 1.0, 1.0000001, 0.5], dtype=np.float32)) == 4
    assert R.holds_all_edges(R.edge_tensor((1, 1, 28, 28), seed=1)) and not R.holds_all_edges(np.zeros(4, np.float32))
