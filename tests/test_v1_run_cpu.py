"""CPU: the host side of running the v1 experiments on real SEVIR (experiments/v1_experiments/_runner.py) — which loader
an experiment reads a store through and what the splits hold, the empty-split errors, the resume state of a one- and a
two-optimiser `Step` through torch.save, and the flags the driver parses before it opens the device."""
import datetime
import os

import numpy as np
import pytest
import torch

from weatherforecastingtoolkit_amd import config as C
from weatherforecastingtoolkit_amd import functional as Fn
from weatherforecastingtoolkit_amd.experiments.v1_experiments import _runner
from weatherforecastingtoolkit_amd.pipeline.datasets.sevir.sevir import SequenceBatchLoader
from weatherforecastingtoolkit_amd.pipeline.datasets.sevire.sevir import SEVIRFrameLoader

EXP = os.path.dirname(_runner.__file__)
# time stamps of the six events: three before 2019-01-01, two up to 2019-06-01, one after
STAMPS = ["2018-03-01", "2018-07-15", "2018-11-30", "2019-02-10", "2019-04-20", "2019-08-05"]


def write_store(root, stamps=STAMPS, shape=(128, 128, 25), seed=0):
    """`<root>/CATALOG.csv` + `<root>/data/vil/SEVIR_VIL.npy`, one uint8 `vil` event of `shape` per time stamp"""
    import pandas as pd
    os.makedirs(os.path.join(root, "data", "vil"), exist_ok=True)
    events = np.random.RandomState(seed).randint(0, 255, size=(len(stamps), *shape), dtype=np.uint8)
    np.save(os.path.join(root, "data", "vil", "SEVIR_VIL.npy"), events)
    rows = [dict(id=f"S{i:04d}", img_type="vil", file_name="vil/SEVIR_VIL.h5", file_index=i,
                 time_utc=pd.Timestamp(s), pct_missing=0.0) for i, s in enumerate(stamps)]
    pd.DataFrame(rows).to_csv(os.path.join(root, "CATALOG.csv"), index=False)
    return events


def cfg_of(name, **dataset):
    cfg = C.load(os.path.join(EXP, name, "config.yaml"))
    cfg.dataset.update(dataset)
    return cfg


@pytest.mark.parametrize("name,want", [
    ("ae_gan", "date"), ("ae_gan_kl", "date"), ("pretrained_ae_conv_disc", "date"),
    ("pretrained_ae_linear_sevir", "datamodule"), ("pretrained_ae_dlinear_sevir", "datamodule"),
    ("pretrained_ae_dlinear_ind", "datamodule"), ("pretrained_ae_dlinear_indc_indp", "datamodule"),
    ("pretrained_ae_convae_sevir", "datamodule"), ("pretrained_ae_convattn_ae_sevir", "datamodule"),
    ("prediff_mlp_sevir", "datamodule"),
])
def test_loader_path_per_experiment(name, want):
    assert _runner.loader_path(os.path.join(EXP, name)) == want
    assert _runner.loader_path(os.path.join(EXP, name) + os.sep) == want
    assert os.path.isfile(os.path.join(EXP, name, "config.yaml"))


def test_date_path_splits_three_two_one(tmp_path):
    write_store(str(tmp_path))
    cfg = cfg_of("pretrained_ae_conv_disc", batch_size=2)
    train, val, test, size, line = _runner.open_data(cfg, "NTHW", "date", str(tmp_path))
    assert [type(x) for x in (train, val, test)] == [SEVIRFrameLoader] * 3
    assert [x.n_events for x in (train, val, test)] == [3, 2, 1]
    assert size == 128 and line is None
    # seq_len 1, stride 1: 25 sequences an event, batches of 2, the remainder left out
    assert [len(x) for x in (train, val, test)] == [37, 25, 12]
    ids = [set(x.store.catalog.samples.id) for x in (train, val, test)]
    assert ids == [{"S0000", "S0001", "S0002"}, {"S0003", "S0004"}, {"S0005"}]
    # sharded by rank: each of two ranks holds half the batches
    train2 = _runner.open_data(cfg, "NTHW", "date", str(tmp_path), rank=1, world=2, test=False)
    assert len(train2[0]) == 18 and train2[0].rank == 1 and train2[0].num_shard == 2 and train2[2] == ()


def test_datamodule_path_splits_by_val_ratio_and_seed(tmp_path):
    write_store(str(tmp_path))
    # seq_len 25 on 25-frame events: one sequence an event; five events before 2019-06-01
    cfg = cfg_of("pretrained_ae_dlinear_sevir", val_ratio=0.4, seed=3)
    train, val, test, size, line = _runner.open_data(cfg, "NTHW", "datamodule", str(tmp_path))
    assert [type(x) for x in (train, val, test)] == [SequenceBatchLoader] * 3
    assert size == 128 and line is None
    assert (len(train.order), len(val.order), len(test.order)) == (3, 2, 1)        # val_ratio of the five sequences
    assert sorted(train.base_order + val.base_order) == [0, 1, 2, 3, 4]
    assert train.aug_mode == "0" and train.shuffle_order and not val.shuffle_order
    again = _runner.open_data(cfg, "NTHW", "datamodule", str(tmp_path))
    assert again[0].base_order == train.base_order and again[1].base_order == val.base_order
    train.set_epoch(1)
    again[0].set_epoch(1)
    assert again[0].order == train.order and sorted(train.order) == sorted(train.base_order)
    others = [_runner.open_data(cfg_of("pretrained_ae_dlinear_sevir", val_ratio=0.4, seed=s), "NTHW", "datamodule",
                                str(tmp_path))[1].base_order for s in range(4, 12)]
    assert any(o != val.base_order for o in others)
    # the shipped val_ratio of the linear experiment is 0: no validation loader, the loop is skipped
    lin = _runner.open_data(cfg_of("pretrained_ae_linear_sevir"), "NTHW", "datamodule", str(tmp_path), test=False)
    assert len(lin[0].order) == 5 and lin[1] == () and lin[2] == ()
    # more than one rank: each takes every second batch, the fifth is left out
    sh = _runner.open_data(cfg_of("pretrained_ae_linear_sevir"), "NTHW", "datamodule", str(tmp_path), rank=1, world=2)
    assert isinstance(sh[0], _runner.RankShard) and len(sh[0]) == 2 and sh[0].rank == 1 and len(sh[2]) == 0


def test_shipped_configs_hold_the_keys_the_datamodule_reads():
    for name in os.listdir(EXP):
        path = os.path.join(EXP, name, "config.yaml")
        if not os.path.isfile(path) or _runner.loader_path(os.path.join(EXP, name)) == "date":
            continue
        cfg = C.load(path)
        assert {"aug_mode", "seed", "val_ratio", "num_workers"} <= set(cfg.dataset), name
        assert {"save_every_n_steps", "limit_val_batches", "limit_test_batches"} <= set(cfg.trainer), name


def test_pooling_is_resolved_from_the_store(tmp_path):
    write_store(str(tmp_path), ["2018-03-01", "2018-07-15"], shape=(384, 384, 49))
    cfg = cfg_of("pretrained_ae_dlinear_sevir")
    train, val, test, size, line = _runner.open_data(cfg, "NTHW", "datamodule", str(tmp_path))
    assert size == 128 and line == "presample (2, 3, 3): 384x384x49 -> 128x128x25"
    assert train.presample == (2, 3, 3) and train.raw_seq_len == 25 and test == ()
    train, _, _, size, line = _runner.open_data(cfg, "NTHW", "datamodule", str(tmp_path), presample=None)
    assert size == 384 and line is None and train.presample is None


@pytest.mark.parametrize("path,date", [("date", "2019-01-01"), ("datamodule", "2019-06-01")])
def test_an_empty_training_split_names_the_catalog_and_the_date(tmp_path, path, date):
    write_store(str(tmp_path), ["2019-08-05", "2019-09-01"])
    cfg = cfg_of("pretrained_ae_conv_disc" if path == "date" else "pretrained_ae_dlinear_sevir")
    with pytest.raises(ValueError) as e:
        _runner.open_data(cfg, "NTHW", path, str(tmp_path))
    assert os.path.join(str(tmp_path), "CATALOG.csv") in str(e.value) and date in str(e.value)


def test_empty_validation_and_test_splits_are_skipped(tmp_path, capsys):
    write_store(str(tmp_path), ["2018-03-01", "2018-07-15"])
    train, val, test, _, _ = _runner.open_data(cfg_of("pretrained_ae_conv_disc"), "NTHW", "date", str(tmp_path))
    assert train.n_events == 2 and val == () and test == ()
    assert _runner.VAL_DATE == datetime.datetime(2019, 1, 1) and _runner.TEST_DATE == datetime.datetime(2019, 6, 1)

    class NoSteps:
        def modules(self):
            return []

        def eval(self):
            return self

        def validation_step(self, batch, i):
            raise AssertionError("no batch to validate on")

    capsys.readouterr()
    logs = _runner.evaluate(NoSteps(), val, "val", 0.5, 1)
    assert logs == {"batches": 0}
    _runner.report(logs, 0, step=2, epoch=0)                 # a split without batches prints nothing
    assert capsys.readouterr().out == ""
    _runner.report({"val_loss": 0.5, "batches": 1}, 0, step=2, epoch=0)
    assert capsys.readouterr().out == '{"val_loss": 0.5, "batches": 1, "step": 2, "epoch": 0}\n'
    _runner.report({"val_loss": 0.5, "batches": 1}, 1, step=2, epoch=0)
    assert capsys.readouterr().out == ""


def test_a_refused_or_missing_step_skips_the_pass_with_one_plain_line(capsys):
    """ae_gan's fit ends at lpips.disc_start, where its validation_step is refused: the model tells the driver, which
    prints the reason in place of the line; a model without the step of a split is reported the same way"""
    import types
    from weatherforecastingtoolkit_amd.experiments.v1_experiments import _ae_gan
    assert _ae_gan.Model.validation_refused(types.SimpleNamespace(global_step=1, disc_start=2)) is None
    why = _ae_gan.Model.validation_refused(types.SimpleNamespace(global_step=2, disc_start=2))
    assert "global_step 2 >= lpips.disc_start 2" in why

    class Refusing:
        def validation_refused(self):
            return why

        def validation_step(self, batch, i):
            raise AssertionError("refused before any batch")

    logs = _runner.evaluate(Refusing(), [object()], "val", None, 1)
    assert logs == {"skipped": why}
    assert _runner.evaluate(Refusing(), [object()], "test", None, 1) == {"skipped": f"{__name__}.Model has no test_step"}
    capsys.readouterr()
    _runner.report(logs, 0, step=2, epoch=0)
    assert capsys.readouterr().out == f"pass skipped: {why}\n"


class StubOpt:
    def __init__(self, tag):
        self.tag, self.loaded = tag, None

    def state_dict(self):
        return {"tag": self.tag, "exp_avg": torch.full((3,), float(len(self.tag)))}

    def load_state_dict(self, sd):
        self.loaded = sd


class StubSch(StubOpt):
    def state_dict(self):
        return {"tag": self.tag, "last_epoch": 5}


class One(_runner.Step):
    def __init__(self):
        self.opt, self.sch = StubOpt("g"), StubSch("g_sch")


class Two(_runner.Step):
    def __init__(self):
        self.opt, self.sch, self.d_opt, self.d_sch = StubOpt("g"), StubSch("g_sch"), StubOpt("d"), StubSch("d_sch")
        self.global_step = 5

    def optimizers(self):
        return [(self.opt, self.sch), (self.d_opt, self.d_sch)]


@pytest.mark.parametrize("make,tags", [(One, ["g"]), (Two, ["g", "d"])])
def test_resume_state_round_trip(tmp_path, make, tags):
    model = make()
    torch.manual_seed(11)
    Fn._seed_counter[0] = 17
    state = {"predictor.w": torch.arange(4.0)}
    path = str(tmp_path / "out" / "last.ckpt")
    _runner.save_checkpoint(path, model, lambda m: state, 5, 2)
    assert os.listdir(os.path.dirname(path)) == ["last.ckpt"]                      # the temporary file was moved in place
    want_next = torch.rand(3)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    keys = ["state_dict", "global_step", "optimizer_states", "lr_schedulers", "epoch", "rng"]
    assert list(ck) == keys + (["model_global_step"] if make is Two else [])
    assert ck["global_step"] == 5 and ck["epoch"] == 2 and torch.equal(ck["state_dict"]["predictor.w"], state["predictor.w"])
    assert [o["tag"] for o in ck["optimizer_states"]] == tags                      # generator first, then discriminator
    assert [s["tag"] for s in ck["lr_schedulers"]] == [t + "_sch" for t in tags]
    assert set(ck["rng"]) == {"torch_state", "cuda_state", "dropout_counter"} and ck["rng"]["dropout_counter"] == 17
    other = make()
    if make is Two:
        other.global_step = 0
    Fn._seed_counter[0] = 0
    torch.manual_seed(99)
    assert _runner.load_resume_state(other, ck) == 2
    assert Fn._seed_counter[0] == 17 and torch.equal(torch.rand(3), want_next)    # the generator continues where it was
    assert [o.loaded["tag"] for o, _ in other.optimizers()] == tags
    assert [s.loaded for _, s in other.optimizers()] == ck["lr_schedulers"]
    assert all(torch.equal(o.loaded["exp_avg"], w["exp_avg"]) for (o, _), w in zip(other.optimizers(), ck["optimizer_states"]))
    assert other.global_step == 5 if make is Two else not hasattr(other, "global_step")
    live = {"predictor.w": torch.zeros(4)}
    _runner.load_state(live, ck["state_dict"])
    assert torch.equal(live["predictor.w"], torch.arange(4.0))
    with pytest.raises(ValueError, match="does not fit"):
        _runner.load_state({"predictor.v": torch.zeros(4)}, ck["state_dict"])
    # --resume: from the file's step; with no last.ckpt present from scratch, and nothing is touched
    third, live = make(), {"predictor.w": torch.zeros(4)}
    assert _runner.resume(path, third, lambda m: live) == 5 and torch.equal(live["predictor.w"], torch.arange(4.0))
    assert third.opt.loaded["tag"] == "g"
    fresh = make()
    assert _runner.resume(str(tmp_path / "out" / "none.ckpt"), fresh, lambda m: live) == 0
    assert fresh.opt.loaded is None and fresh.sch.loaded is None
    Fn._seed_counter[0] = 0


def test_a_checkpoint_without_optimiser_state_restarts_the_moments(capsys):
    model = Two()
    model.global_step = 0
    ck = _runner.checkpoint({"predictor.w": torch.zeros(2)}, 7)                   # what the driver wrote before
    assert list(ck) == ["state_dict", "global_step"]
    assert _runner.load_resume_state(model, ck) == 0
    assert "no optimiser state" in capsys.readouterr().err
    assert model.opt.loaded is None and model.d_opt.loaded is None and model.d_sch.loaded is None
    assert model.sch.loaded == {"last_epoch": 7} and model.global_step == 7
    with pytest.raises(ValueError, match="2 of each"):
        _runner.load_resume_state(model, dict(ck, optimizer_states=[{}], lr_schedulers=[{}]))


def test_total_steps_is_unchanged():
    assert _runner.total_steps(10, 2, 1, 4, "fit") == 4 and _runner.total_steps(10, 2, 1, -1, "fit") == 20
    assert _runner.total_steps(3, 1, 1, 2, "fit") == 2 and _runner.total_steps(10, 2, 4, 3, "test") == 3
    assert _runner.total_steps(1, 1, 4) == 1 and _runner.total_steps(6, 1, 1) == 6


def test_new_flags_are_flags_and_overrides_stay_key_value(monkeypatch, tmp_path):
    """the driver parses --data-dir, --validate, --test, --resume, --stop-after itself (they were refused as overrides that
    are not key=value); a `--resume` with no last.ckpt present starts from scratch: it reaches the device, not an error"""
    from weatherforecastingtoolkit_amd.experiments.v1_experiments.pretrained_ae_dlinear_ind import train

    class Reached(Exception):
        pass

    def init():
        raise Reached()

    monkeypatch.setattr(_runner.parallel, "init_from_env", init)
    with pytest.raises(Reached):
        train.main(["--max-steps", "2", "--data-dir", str(tmp_path), "--data-format", "npy", "--presample", "none",
                    "--validate", "--test", "--resume", "--stop-after", "1", f"experiment_path={tmp_path}"])
    assert not os.path.exists(tmp_path / "outputs")
    with pytest.raises(ValueError, match="override '--nonsense' is not key=value"):
        train.main(["--nonsense", f"experiment_path={tmp_path}"])
