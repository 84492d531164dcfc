"""CPU: verification per lead time (csrc/verify.hip, ops.verify_leads, metrics.LeadVerification, `--verify`) — the ABI
and host-side argument checks of wfae_verify_leads, the numpy restatement tests/verify_ref.py against
tests/golden/g25_verify.npz (recorded from the reference's own csi / hss), the host half of LeadVerification on
hand-written tables, its merge over two gloo ranks, and the refusals of `--verify`."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import verify_ref
from weatherforecastingtoolkit_amd import _lib
from weatherforecastingtoolkit_amd import config as C
from weatherforecastingtoolkit_amd._lib import WfaeError
from weatherforecastingtoolkit_amd.experiments.v1_experiments import _dlinear, _latents, _runner
from weatherforecastingtoolkit_amd.experiments.v1_experiments.pretrained_ae_linear_sevir import train as linear
from weatherforecastingtoolkit_amd.pipeline import metrics as M

G25 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g25_verify.npz")
EXP = os.path.dirname(_runner.__file__)


def g25_case():
    """-> (frames (B, T, 1, H, W), forecast (B, P, 1, H, W), L, thresholds, the fixture)"""
    g = np.load(G25, allow_pickle=False)
    frames = (g["frames_u8"].astype(np.float32) / np.float32(255))[:, :, None]
    forecast = (g["forecast_u8"].astype(np.float32) / np.float32(255))[:, :, None]
    return frames, forecast, int(g["input_frames"]), [float(t) for t in g["thresholds"]], g


def test_header_declares_and_library_exports_verify_leads():
    """the declaration lives in include/wfae_verify.h, which include/wfae.h includes inside its extern "C" block, and
    `_lib.load()` binds it with the argument types parsed from there"""
    assert _lib.INCLUDED_HEADERS == (os.path.join(os.path.dirname(_lib.HEADER), "wfae_verify.h"),)
    assert '#include "wfae_verify.h"' in open(_lib.HEADER).read()
    decls = _lib.parse_header(_lib.INCLUDED_HEADERS[0])
    assert list(decls) == ["wfae_verify_leads"]
    restype, argtypes, argnames = decls["wfae_verify_leads"]
    assert restype is ctypes.c_int and argnames[-1] == "stream" and len(argtypes) == 19
    assert argnames[:3] == ["fields", "field_bstride", "field_lstride"] and argnames[-3:] == ["ws", "ws_bytes", "stream"]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "wfae_verify_leads")
    lib = _lib.load()
    assert lib.wfae_version() == 103 and lib.wfae_verify_leads.argtypes == argtypes


def test_verify_leads_rejects_bad_arguments_without_gpu():
    """every check answers on the host before a launch; the fake device addresses are never dereferenced"""
    lib = _lib.load()
    D = [0x7F0000000000 + (i << 32) for i in range(8)]
    a = ctypes.addressof
    thr = (ctypes.c_float * 9)(*[0.1] * 9)

    def call(n_fields=2, ptrs=None, bs=None, ls=None, target=D[4], tb=5 * 480, tl=480, F=None, B=2, P=3, S=480,
             thr_p=a(thr), n_thr=6, counts=D[5], sums=D[6], ws=D[7], ws_bytes=1 << 20, host_arrays=True):
        fp = (ctypes.c_void_p * 5)(*(ptrs or D[:4]), None)
        fb = (ctypes.c_int64 * 5)(*(bs or [3 * 480] * 4), 0)
        fl = (ctypes.c_int64 * 5)(*(ls or [480, 0, 480, 480]), 0)
        rc = lib.wfae_verify_leads(a(fp) if host_arrays else None, a(fb), a(fl), target, tb, tl,
                                   n_fields if F is None else F, B, P, S, thr_p, n_thr, 1, 0, counts, sums, ws, ws_bytes,
                                   None)
        return rc, lib.wfae_last_error_string()

    for kw in (dict(host_arrays=False), dict(target=None), dict(counts=None), dict(sums=None), dict(ws=None),
               dict(ptrs=[D[0], None, D[2], D[3]])):
        rc, msg = call(**kw)
        assert rc == -2 and b"null" in msg, (kw, rc, msg)
    for kw, word in ((dict(F=0), b"F 0"), (dict(F=5), b"F 5"), (dict(n_thr=9), b"n_thr 9"), (dict(n_thr=-1), b"n_thr"),
                     (dict(thr_p=None), b"n_thr"), (dict(S=0), b"shape"), (dict(B=0), b"shape"), (dict(P=0), b"shape"),
                     (dict(bs=[3 * 480, -1, 0, 0]), b"negative stride of field 1"),
                     (dict(ls=[-480, 0, 0, 0]), b"negative stride of field 0"), (dict(tb=-1), b"negative target stride"),
                     (dict(tl=-1), b"negative target stride"), (dict(S=1 << 39), b"too large")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    # the workspace formula of the header: P * min(256, ceil(B * S / 1024)) * F * (3 n_thr + 2) * 8
    need = 3 * 1 * 2 * (3 * 6 + 2) * 8
    rc, msg = call(ws_bytes=need - 1)
    assert rc == -1 and b"workspace" in msg
    need = 3 * 256 * 4 * (3 * 8 + 2) * 8
    rc, msg = call(n_fields=4, S=1 << 20, n_thr=8, tb=5 << 20, tl=1 << 20, bs=[3 << 20] * 4, ls=[1 << 20] * 4,
                   ws_bytes=need - 1)
    assert rc == -1 and b"workspace" in msg


def test_verify_leads_has_no_cpu_fallback():
    from weatherforecastingtoolkit_amd import ops
    x = torch.zeros(1, 2, 1, 8, 8)
    with pytest.raises(WfaeError):
        ops.verify_leads([x], x, M.THRESHOLDS)


def test_restatement_reproduces_g25():
    """the counts through scores_from_counts equal the reference's CSI / HSS exactly (fp32 on both sides, 960 cells per
    lead < 2^24); mse / mae within n * 2^-53 relative, n = 960 terms per lead"""
    frames, forecast, L, thr, g = g25_case()
    assert int(g["ties"]) > 0 and frames.shape == (2, 5, 1, 24, 20) and forecast.shape == (2, 3, 1, 24, 20) and L == 2
    counts, sums = verify_ref.verify_leads([forecast, frames[:, L - 1]], frames[:, L:], thr, clamp01=True)
    assert counts.shape == (3, 2, 19) and sums.shape == (3, 2, 2)
    n = 2 * 24 * 20
    assert (counts[..., -1] == n).all()
    tol = verify_ref.sum_tolerance(n)
    for p in range(3):
        for f in range(2):
            for k in range(len(thr)):
                c, h = M.scores_from_counts(*counts[p, f, 3 * k:3 * k + 3], n)
                assert c == g["csi"][p, f, k] and h == g["hss"][p, f, k], (p, f, k)
            assert abs(sums[p, f, 0] / n - g["mse"][p, f]) <= tol * g["mse"][p, f]
            assert abs(sums[p, f, 1] / n - g["mae"][p, f]) <= tol * g["mae"][p, f]


def hand_tables():
    """P = 2 leads, fields (forecast, persistence, reconstruction), one threshold, 100 cells per lead"""
    lv = M.LeadVerification(("forecast", "persistence", "reconstruction"), 2, thresholds=[0.5], device="cpu")
    #                      tp fn fp cells
    counts = torch.tensor([[[1, 0, 0, 100], [5, 5, 5, 100], [10, 0, 0, 100]],
                           [[1, 9, 0, 100], [2, 4, 6, 100], [10, 0, 0, 100]]])
    sums = torch.tensor([[[4.0, 10.0], [0.0, 0.0], [1.0, 5.0]],
                         [[2.0, 8.0], [8.0, 20.0], [16.0, 30.0]]], dtype=torch.float64)
    lv.counts.copy_(counts)
    lv.sums.copy_(sums)
    return lv, counts.numpy(), sums.numpy()


def test_result_from_hand_written_tables():
    lv, counts, sums = hand_tables()
    r = lv.result()
    assert list(r) == ["cells_per_lead", "leads", "total", "beats_persistence"]
    assert r["cells_per_lead"] == 100 and [e["lead"] for e in r["leads"]] == [1, 2]
    for p, e in enumerate(r["leads"]):
        for f, name in enumerate(lv.names):
            c, h = M.scores_from_counts(*counts[p, f, :3], 100)
            assert e[name] == {"mse": sums[p, f, 0] / 100, "mae": sums[p, f, 1] / 100, "csi_0": c, "hss_0": h,
                               "csi_m": c, "hss_m": h}
    # lead 1: persistence has no error -> no division; lead 2: 1 - 0.02 / 0.08, and the reconstruction loses
    assert r["leads"][0]["skill"] is None and r["leads"][0]["skill_reconstruction"] is None
    assert r["leads"][1]["skill"] == 1 - 0.02 / 0.08 and r["leads"][1]["skill_reconstruction"] == 1 - 0.16 / 0.08
    assert r["beats_persistence"] == [2]
    # totals from the summed tables: CSI of (tp 2, fn 9, fp 0) is 2 / 11, the mean of the per-lead CSIs is 0.55
    tot = r["total"]
    c, h = M.scores_from_counts(2, 9, 0, 200)
    assert tot["forecast"]["csi_0"] == c and tot["forecast"]["hss_0"] == h
    per_lead = np.mean([e["forecast"]["csi_0"] for e in r["leads"]])
    assert abs(per_lead - 0.55) < 1e-6 and abs(c - 2 / 11) < 1e-6 and abs(per_lead - c) > 0.3
    assert tot["forecast"]["mse"] == 6.0 / 200 and tot["persistence"]["mae"] == 20.0 / 200
    assert tot["skill"] == 1 - (6.0 / 200) / (8.0 / 200)
    import json
    assert json.loads(json.dumps(r)) == r              # a plain dict: null for None, no numpy scalars


def test_result_without_cells_is_skipped():
    lv = M.LeadVerification(("forecast", "persistence"), 3)
    assert "skipped" in lv.result()
    lv = M.LeadVerification(("forecast", "persistence"), 3, device="cpu")
    assert "skipped" in lv.result()
    lv.reset()
    assert int(lv.counts.sum()) == 0


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _merge_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from weatherforecastingtoolkit_amd import parallel
    parallel.init_from_env("gloo")
    lv, counts, sums = hand_tables()
    lv.counts.mul_(rank + 1)
    lv.sums.mul_(rank + 1).add_(0.1 * rank)
    lv.merge(world)
    want_sums = sums * 1 + (sums * 2 + 0.1)
    q.put((rank, bool((lv.counts.numpy() == counts * 3).all()) and bool((lv.sums.numpy() == want_sums).all())))
    dist.barrier()
    dist.destroy_process_group()


def test_merge_over_two_gloo_ranks_is_the_elementwise_sum():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_merge_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = [q.get(timeout=120) for _ in ps]
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    assert sorted(res) == [(0, True), (1, True)]


def dlinear_model(autoencoder=None):
    cfg = C.load(os.path.join(EXP, "pretrained_ae_dlinear_ind", "config.yaml"))
    cfg.dlinear.update(enc_in=3)
    return _dlinear.Model(cfg, autoencoder=autoencoder)


def test_verify_is_refused_with_its_reason():
    lin = linear.Model(C.load(os.path.join(EXP, "pretrained_ae_linear_sevir", "config.yaml")), latent_channels=2)
    with pytest.raises(WfaeError, match="--verify: .*pretrained_ae_linear_sevir.* has no validation step that decodes"):
        _runner.enable_verification(lin)
    with pytest.raises(WfaeError, match="--verify: .* has no latent provider"):
        _runner.enable_verification(dlinear_model())
    model = dlinear_model(_latents.Autoencoder(64, "ae_vit.tokens"))
    with pytest.raises(WfaeError, match="--verify: the latent provider of kind 'ae_vit.tokens' cannot decode"):
        _runner.enable_verification(model)
    assert lin.verification is None and model.verification is None and _runner.Step.verification is None


def test_verify_sets_the_tables_of_a_decoding_dlinear_model():
    model = dlinear_model(_latents.Autoencoder(64, "ae_64x8x8_lin.enc"))
    lv = _runner.enable_verification(model)
    assert model.verification is lv and isinstance(lv, M.LeadVerification)
    assert lv.names == ("forecast", "persistence", "reconstruction") and lv.pred_frames == model.pred_frames == 12
    assert lv.thresholds == M.THRESHOLDS and lv.counts is None
    # a batch of latents holds no frames: the step hands None on, nothing is added
    import inspect
    assert inspect.signature(model.validate_latents).parameters["frames"].default is None
