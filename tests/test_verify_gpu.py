"""GPU: verification per lead time — csrc/verify.hip through ops.verify_leads against the numpy restatement
tests/verify_ref.py (counts equal, fp64 sums within n * 2^-53 relative, n the cells of a lead) on both load routes,
strided views, several loop trips, 0 and 8 thresholds, the clamp and the exact ties of tests/golden/g25_verify.npz;
against ops.skill_scores; accumulation and repeatability; the DLinear validation step with `verification` set; and
`--verify` through the pretrained_ae_dlinear_sevir entry point."""
import json
import os

import numpy as np
import pytest
import torch

from tests import verify_ref
from tests.test_verify_cpu import g25_case

pytestmark = pytest.mark.gpu

THR = [16 / 255, 74 / 255, 133 / 255, 160 / 255, 181 / 255, 219 / 255]


def values(rng, shape, lo=0.0, hi=1.0):
    """fp32 values in [lo, hi), half of them quantised to k / 255 so that some equal a threshold exactly"""
    x = rng.random(shape, dtype=np.float32) * np.float32(hi - lo) + np.float32(lo)
    q = rng.integers(0, 256, shape).astype(np.float32) / np.float32(255)
    return np.where(rng.random(shape) < 0.5, q, x).astype(np.float32)


def check(dev, fields, target, thr=THR, clamp01=True):
    """fields / target: host arrays or views of host arrays; the device gets the same views of the same bases"""
    from weatherforecastingtoolkit_amd import ops
    counts, sums = ops.verify_leads([to_dev(f, dev) for f in fields], to_dev(target, dev), thr, clamp01=clamp01)
    want = verify_ref.verify_leads(fields, target, thr, clamp01)
    verify_ref.assert_tables(counts.cpu().numpy(), sums.cpu().numpy(), *want)
    return counts, sums


_bases = {}


def to_dev(a, dev):
    """a device tensor with the strides and the offset `a` has in its base array (one upload per base)"""
    base = a if a.base is None else a.base
    while base.base is not None:
        base = base.base
    key = (id(base), str(dev))
    if key not in _bases:
        _bases[key] = (base, torch.from_numpy(base).to(dev))
    off = (a.__array_interface__["data"][0] - base.__array_interface__["data"][0]) // 4
    return torch.as_strided(_bases[key][1], a.shape, [s // 4 for s in a.strides], off)


@pytest.fixture(autouse=True)
def _drop_bases():
    yield
    _bases.clear()


def test_smallest(dev):
    rng = np.random.default_rng(1)
    check(dev, [values(rng, (1, 1, 1))], values(rng, (1, 1, 1)))


def test_dword_route_with_four_contiguous_fields(dev):
    rng = np.random.default_rng(2)
    check(dev, [values(rng, (2, 3, 1027)) for _ in range(4)], values(rng, (2, 3, 1027)))


@pytest.mark.parametrize("S", [1027, 1024, 160000])
def test_views_of_one_batch(dev, S):
    """target = frames[:, 2:] and persistence = frames[:, 1] (lead stride 0) of one (B, 5, S) batch: with S = 1027 the
    bases are off a 16-byte boundary (dword loads), with S = 1024 every base and stride is aligned (16-byte loads), with
    S = 160000 the 16-byte route takes a second loop trip (80000 quads against 256 blocks x 256 lanes)"""
    from weatherforecastingtoolkit_amd import ops
    rng = np.random.default_rng(3)
    frames = values(rng, (2, 5, S))
    fields = [values(rng, (2, 3, S)), frames[:, 1], values(rng, (2, 3, 1, S))]
    check(dev, fields, frames[:, 2:])
    d = to_dev(frames, dev)
    assert (d[:, 1].data_ptr() % 16 == 0) == (S % 4 == 0) and d[:, 2:].data_ptr() == d.data_ptr() + 8 * S
    with pytest.raises(Exception, match="a frame must be contiguous"):
        ops.verify_leads([d[:, 2:, ::2]], d[:, 2:, ::2], THR)


def test_second_loop_trip_of_the_capped_grid(dev):
    rng = np.random.default_rng(4)
    frames = values(rng, (2, 4, 180001))
    check(dev, [values(rng, (2, 3, 180001)), frames[:, 0]], frames[:, 1:])


@pytest.mark.parametrize("n_thr", [0, 8])
def test_threshold_counts(dev, n_thr):
    rng = np.random.default_rng(5)
    thr = (THR + [0.0, 1.0])[:n_thr]
    counts, sums = check(dev, [values(rng, (2, 2, 480)), values(rng, (2, 480))], values(rng, (2, 2, 480)), thr=thr)
    assert counts.shape == (2, 2, 3 * n_thr + 1) and sums.shape == (2, 2, 2)


@pytest.mark.parametrize("clamp01", [True, False])
def test_clamp(dev, clamp01):
    rng = np.random.default_rng(6)
    f, t = [values(rng, (2, 2, 480), -0.5, 1.5), values(rng, (2, 1, 480), -0.5, 1.5)], values(rng, (2, 2, 480), -0.5, 1.5)
    _, sums = check(dev, f, t, thr=THR + [0.0, 1.0], clamp01=clamp01)
    other = verify_ref.verify_leads(f, t, THR + [0.0, 1.0], not clamp01)[1]
    assert not np.allclose(sums.cpu().numpy(), other)       # the case does tell the two settings apart


def test_exact_ties_of_g25(dev):
    from weatherforecastingtoolkit_amd.pipeline import metrics as M
    frames, forecast, L, thr, g = g25_case()
    counts, sums = check(dev, [forecast, frames[:, L - 1]], frames[:, L:], thr=thr)
    counts, sums, n = counts.cpu().numpy(), sums.cpu().numpy(), 2 * 24 * 20
    tol = verify_ref.sum_tolerance(n)
    for p in range(3):
        for f in range(2):
            for k in range(len(thr)):
                assert M.scores_from_counts(*counts[p, f, 3 * k:3 * k + 3], n) == (g["csi"][p, f, k], g["hss"][p, f, k])
            assert abs(sums[p, f, 0] / n - g["mse"][p, f]) <= tol * g["mse"][p, f]
            assert abs(sums[p, f, 1] / n - g["mae"][p, f]) <= tol * g["mae"][p, f]


def test_counts_equal_skill_scores(dev):
    from weatherforecastingtoolkit_amd import ops
    rng = np.random.default_rng(7)
    pred = torch.from_numpy(values(rng, (2, 3, 1, 40, 52), -0.2, 1.2)).to(dev)
    target = torch.from_numpy(values(rng, (2, 3, 1, 40, 52), -0.2, 1.2)).to(dev)
    counts, _ = ops.verify_leads([pred], target, THR, clamp01=True)
    skill = ops.skill_scores(pred, target, THR, [("none", 1)], clamp01=True)
    assert torch.equal(counts[:, 0, :18].sum(0), skill[0, :18])
    assert int(counts[:, 0, 18].sum()) == int(skill[0, 19]) == pred.numel()


def test_accumulate_and_repeat_bits(dev):
    from weatherforecastingtoolkit_amd import ops
    rng = np.random.default_rng(8)
    frames = [torch.from_numpy(values(rng, (2, 5, 1, 33, 31))).to(dev) for _ in range(2)]
    fcs = [torch.from_numpy(values(rng, (2, 3, 1, 33, 31))).to(dev) for _ in range(2)]
    fresh = [ops.verify_leads([fc, fr[:, 1]], fr[:, 2:], THR) for fc, fr in zip(fcs, frames)]
    again = ops.verify_leads([fcs[0], frames[0][:, 1]], frames[0][:, 2:], THR)
    assert torch.equal(again[0], fresh[0][0]) and torch.equal(again[1].view(torch.int64), fresh[0][1].view(torch.int64))
    out = (torch.zeros_like(fresh[0][0]), torch.zeros_like(fresh[0][1]))
    for fc, fr in zip(fcs, frames):
        got = ops.verify_leads([fc, fr[:, 1]], fr[:, 2:], THR, out=out)
        assert got[0] is out[0] and got[1] is out[1]
    assert torch.equal(out[0], fresh[0][0] + fresh[1][0])
    assert torch.equal(out[1].view(torch.int64), (fresh[0][1] + fresh[1][1]).view(torch.int64))
    with pytest.raises(Exception, match="out must hold"):
        ops.verify_leads([fcs[0]], frames[0][:, 2:], THR, out=out)


def test_validation_step_adds_the_three_fields(dev):
    """the DLinear validation step with `verification` set: the tables equal the restatement on what the step decoded,
    the persistence rows are those of the loader's own frames, and the step's logs keep their bits"""
    from weatherforecastingtoolkit_amd import config as C
    from weatherforecastingtoolkit_amd.experiments.v1_experiments import _dlinear as D
    from weatherforecastingtoolkit_amd.pipeline import metrics as M

    class Recording(M.LeadVerification):
        def add(self, fields, target):
            self.seen = (fields, target)
            super().add(fields, target)

    cfg = C.load(os.path.join(os.path.dirname(D.__file__), "pretrained_ae_dlinear_sevir", "config.yaml"))
    cfg.dlinear.enc_in, cfg.dlinear.features_per_step = 4096, 1
    torch.manual_seed(0)
    model = D.Model(cfg, autoencoder=D.Autoencoder(128)).to(dev).eval()
    frames = torch.rand(1, 25, 128, 128, device=dev)
    loss0, logs0 = model.validation_step(frames)
    model.verification = lv = Recording(("forecast", "persistence", "reconstruction"), 12)
    loss1, logs1 = model.validation_step(frames)
    assert len(logs0) == 57 and list(logs0) == list(logs1)
    for k in logs0:
        a, b = torch.as_tensor(logs0[k]).cpu().double(), torch.as_tensor(logs1[k]).cpu().double()
        assert torch.equal(a, b), k
    assert torch.equal(loss0, loss1)
    fields, target = lv.seen
    # views of the batch, no copies: persistence is the 13th frame with lead stride 0, the target the last 12
    assert fields["persistence"].data_ptr() == frames[:, 12].data_ptr() and target.data_ptr() == frames[:, 13:].data_ptr()
    host = [fields[n].cpu().numpy() for n in lv.names]
    fr = frames.cpu().numpy()
    want = verify_ref.verify_leads(host, fr[:, 13:], M.THRESHOLDS, True)
    verify_ref.assert_tables(lv.counts.cpu().numpy(), lv.sums.cpu().numpy(), *want)
    pers = verify_ref.verify_leads([fr[:, 12]], fr[:, 13:], M.THRESHOLDS, True)
    verify_ref.assert_tables(lv.counts[:, 1:2].cpu().numpy(), lv.sums[:, 1:2].cpu().numpy(), *pers)
    r = lv.result()
    assert r["cells_per_lead"] == 128 * 128 and len(r["leads"]) == 12
    # a batch of latents holds no frames: nothing is added
    lv.reset()
    model.validation_step(model.frames_latents(frames)[1])
    assert int(lv.counts.sum()) == 0 and "skipped" in lv.result()


def run_lines(train, argv, capsys):
    capsys.readouterr()
    assert train.main(argv) == 0
    out = capsys.readouterr().out.splitlines()
    assert out[-1] == "done"
    lines = []
    for line in out:
        d = json.loads(line) if line.startswith("{") else None
        if d is not None and "sequences_per_s" in d:        # the one field that is a wall-clock rate
            d.pop("sequences_per_s")
            line = json.dumps(d)
        lines.append(line)
    return lines


def check_verification(line, split, step):
    v = json.loads(line)["verification"]
    assert v["split"] == split and v["step"] == step and v["cells_per_lead"] % (128 * 128) == 0 and v["cells_per_lead"] > 0
    assert [e["lead"] for e in v["leads"]] == list(range(1, 13))
    assert list(v)[:6] == ["split", "step", "cells_per_lead", "leads", "total", "beats_persistence"]
    for e in v["leads"] + [v["total"]]:
        assert {"forecast", "persistence", "reconstruction", "skill", "skill_reconstruction"} <= set(e)
        assert e["persistence"]["mse"] > 0 and e["skill"] == 1 - e["forecast"]["mse"] / e["persistence"]["mse"]
    assert v["beats_persistence"] == [e["lead"] for e in v["leads"] if e["skill"] > 0]


def test_driver_prints_one_verification_line_per_pass(dev, tmp_path, capsys):
    from weatherforecastingtoolkit_amd.experiments.v1_experiments.pretrained_ae_dlinear_sevir import train
    common = ["trainer.log_every_n_steps=1", "dataset.batch_size=1", "dlinear.enc_in=4096"]
    fit = ["--mode", "fit", "--max-steps", "2", "--validate", "--test"]
    plain = run_lines(train, [*fit, f"experiment_path={tmp_path / 'a'}", *common], capsys)
    flagged = run_lines(train, [*fit, "--verify", f"experiment_path={tmp_path / 'b'}", *common], capsys)
    ver = [i for i, line in enumerate(flagged) if line.startswith('{"verification"')]
    assert len(ver) == 2 and [line for i, line in enumerate(flagged) if i not in ver] == plain
    # each follows the line of its pass: validation after the last step, then the test pass
    assert "val_loss" in flagged[ver[0] - 1] and "test_loss" in flagged[ver[1] - 1]
    check_verification(flagged[ver[0]], "val", 2)
    check_verification(flagged[ver[1]], "test", 2)


def test_driver_test_mode_prints_one_verification_line(dev, tmp_path, capsys):
    from weatherforecastingtoolkit_amd.experiments.v1_experiments.pretrained_ae_dlinear_sevir import train
    common = ["--mode", "test", "--max-steps", "1", "dataset.batch_size=1", "dlinear.enc_in=4096",
              f"experiment_path={tmp_path}"]
    plain = run_lines(train, common, capsys)
    flagged = run_lines(train, ["--verify", *common], capsys)
    assert flagged[:-2] == plain[:-1] and flagged[-1] == plain[-1] == "done"
    check_verification(flagged[-2], "test", 1)
    assert json.loads(flagged[-2])["verification"]["cells_per_lead"] == 128 * 128
