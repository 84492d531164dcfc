"""What the one-launch verification pass (csrc/verify.hip, ops.verify_leads) costs, against the way the tree had to do the
same before it: `ops.skill_scores` on each lead slice of each field (a contiguous copy of the slice first, which that op
needs) plus torch for the two error sums.

    python tools/verify_bench.py [--rounds 5] [--out profiles/verify_bench.jsonl]

Per shape (B = 8 sequences of 25 frames, 13 in and P = 12 out, 384 x 384 and 128 x 128) one JSON line is appended to --out:
the three fields of `--verify` (forecast and reconstruction (B, P, 1, H, W), persistence = frames[:, 12] with lead stride 0)
against frames[:, 13:].  Both ways run on the same tensors and alternate inside every round, each window between a pair
of device events after one untimed call; the line holds the medians, every round's pair, the ratio, whether both ways
count the same, the entry point alone on prepared arguments (`entry_point_ms`: the two launches without the host work of
ops.verify_leads), the bytes the pass has to move (every operand once, persistence once) over that time, and next to it the
rate of a device copy of the same bytes measured in the same rounds and the copy rate recorded from
tools/probe/hbm_streams.hip.  A pass shorter than a few launch latencies is marked launch-bound; its GB/s is then no
statement about the memory system.  A last line holds one validation step of pretrained_ae_dlinear_sevir (its config, the
default provider, a (1, 25, 128, 128) batch) with `verification` set and unset, alternated.  No thresholds: the tool measures.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from weatherforecastingtoolkit_amd import config as C  # noqa: E402
from weatherforecastingtoolkit_amd import _lib, ops  # noqa: E402
from weatherforecastingtoolkit_amd.experiments.v1_experiments import _dlinear as D  # noqa: E402
from weatherforecastingtoolkit_amd.pipeline import metrics as M  # noqa: E402

HBM_STREAMS_COPY_TB_S = 5.7        # tools/probe/hbm_streams.hip, mode-0 copy (profiles/r04_probe_hbm_stream_shapes.txt)
LAUNCH_BOUND_MS = 0.03             # two launches back to back: a pass this short is launch latency, not bandwidth


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def shape_line(size, rounds, dev):
    b, t, n_in = 8, 25, 13
    p = t - n_in
    g = torch.Generator().manual_seed(size)
    frames = torch.rand(b, t, size, size, generator=g).to(dev)
    forecast = torch.rand(b, p, 1, size, size, generator=g).to(dev)
    recon = torch.rand(b, p, 1, size, size, generator=g).to(dev)
    fields, target = [forecast, frames[:, n_in - 1], recon], frames[:, n_in:]
    nt = len(M.THRESHOLDS)
    tables = (torch.zeros(p, 3, 3 * nt + 1, dtype=torch.int64, device=dev), torch.zeros(p, 3, 2, dtype=torch.float64, device=dev))

    def one_launch():
        return ops.verify_leads(fields, target, M.THRESHOLDS, clamp01=True, out=tables)

    def parent_way():
        """per lead and field: the counts from ops.skill_scores, the error sums from torch (fp64, clamped like the counts)"""
        counts, sums = [], []
        for lead in range(p):
            tg = target[:, lead].reshape(b, 1, 1, size, size).contiguous()
            td = tg.clamp(0, 1).double()
            for f in fields:
                v = (f[:, lead] if f.dim() == 5 else f).reshape(b, 1, 1, size, size).contiguous()
                counts.append(ops.skill_scores(v, tg, M.THRESHOLDS, [("none", 1)], clamp01=True))
                e = v.clamp(0, 1).double() - td
                sums.append(torch.stack([(e * e).sum(), e.abs().sum()]))
        return torch.stack(counts), torch.stack(sums)

    # the entry point on prepared arguments, back to back: the pass without the host work of ops.verify_leads
    s = size * size
    ptrs = (ctypes.c_void_p * 3)(*[f.data_ptr() for f in fields])
    fb = (ctypes.c_int64 * 3)(p * s, t * s, p * s)
    fl = (ctypes.c_int64 * 3)(s, 0, s)
    thr = (ctypes.c_float * nt)(*M.THRESHOLDS)
    ws = ops.workspace()
    args = (ctypes.addressof(ptrs), ctypes.addressof(fb), ctypes.addressof(fl), target.data_ptr(), t * s, s, 3, b, p, s,
            ctypes.addressof(thr), nt, 1, 1, tables[0].data_ptr(), tables[1].data_ptr(), ws.data_ptr(), ws.numel(),
            torch.cuda.current_stream().cuda_stream)

    def entry():
        _lib.call("wfae_verify_leads", *args)

    big = torch.empty(b * (3 * p + 1) * size * size // 2, device=dev)      # a copy that moves the pass's bytes: read + write
    dst = torch.empty_like(big)
    c1, s1 = ops.verify_leads(fields, target, M.THRESHOLDS, clamp01=True)
    c0, s0 = parent_way()
    same_counts = bool(torch.equal(c1[..., :3 * nt].reshape(-1, 3 * nt), c0[:, 0, :3 * nt]))
    sums_rel = float(((s1.reshape(-1, 2) - s0).abs() / s0.abs()).max())
    dst.copy_(big)
    rows = []
    for _ in range(rounds):
        rows.append((timed(one_launch, 50), timed(parent_way, 3), timed(lambda: dst.copy_(big), 50), timed(entry, 200)))
    ours, parent, copy, kern = (statistics.median(r[i] for r in rows) for i in range(4))
    nbytes = 4 * b * size * size * (3 * p + 1)
    launch_bound = kern < LAUNCH_BOUND_MS
    return {"case": f"verify_leads_{size}", "B": b, "P": p, "frame": [size, size], "fields": 3, "thresholds": nt,
            "one_launch_ms": round(ours, 4), "parent_way_ms": round(parent, 4), "parent_over_one_launch": round(parent / ours, 1),
            "entry_point_ms": round(kern, 4),
            "rounds_one_parent_copy_entry_ms": [[round(v, 4) for v in r] for r in rows],
            "same_counts": same_counts, "sums_max_rel_diff": sums_rel,
            "MB_moved": round(nbytes / 1e6, 2), "launch_bound": launch_bound,
            "GB_per_s": None if launch_bound else round(nbytes / kern / 1e6, 1),
            "device_copy_same_bytes_GB_per_s": round(nbytes / copy / 1e6, 1),
            "hbm_streams_copy_GB_per_s": HBM_STREAMS_COPY_TB_S * 1e3}


def step_line(rounds, dev):
    cfg = C.load(os.path.join(os.path.dirname(D.__file__), "pretrained_ae_dlinear_sevir", "config.yaml"))
    cfg.dlinear.enc_in = 4096
    torch.manual_seed(0)
    model = D.Model(cfg, autoencoder=D.Autoencoder(128)).to(dev).eval()
    frames = torch.rand(1, 25, 128, 128, device=dev)
    lv = M.LeadVerification(("forecast", "persistence", "reconstruction"), 12)

    def step(flag):
        def run():
            model.verification = lv if flag else None
            model.validation_step(frames)
        return run

    for flag in (False, True):
        timed(step(flag), 2)
    rows = [(timed(step(False), 10), timed(step(True), 10)) for _ in range(rounds)]
    off, on = (statistics.median(r[i] for r in rows) for i in range(2))
    return {"case": "validation_step_pretrained_ae_dlinear_sevir", "frames": list(frames.shape),
            "verify_off_ms": round(off, 3), "verify_on_ms": round(on, 3), "added_ms": round(on - off, 3),
            "off_spread_ms": [round(min(r[0] for r in rows), 3), round(max(r[0] for r in rows), 3)],
            "rounds_off_on_ms": [[round(v, 3) for v in r] for r in rows]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("verify_bench measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for line in (shape_line(384, a.rounds, dev), shape_line(128, a.rounds, dev), step_line(a.rounds, dev)):
        print(json.dumps(line), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
