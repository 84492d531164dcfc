"""numpy restatement of csrc/verify.hip (ops.verify_leads): per lead and per field, from strided views.

Values and thresholds are compared in fp32 (`value >= np.float32(threshold)`, after an fp32 clamp to [0, 1] when asked),
the counts are integers, the errors are fp64 differences of the fp32 values, and their sums are taken in extended
precision and rounded to fp64 once, so the restatement's own summation error is below one fp64 ulp.
"""
from __future__ import annotations

import numpy as np


def sum_tolerance(terms):
    """relative bound on an fp64 sum of `terms` non-negative terms taken in any order against the restatement:
    terms * 2^-53.  Any summation order is within (terms - 1) * 2^-53 of the exact sum to first order (Higham, Accuracy
    and Stability of Numerical Algorithms, section 4.2), and the restatement, summed in extended precision and rounded
    once, within 2^-53 of it."""
    return terms * 2.0 ** -53


def _frames(a, b, p, s):
    """field or target (a strided view is fine) as (B, P or 1, S)"""
    a = np.asarray(a)
    assert a.dtype == np.float32 and a.shape[0] == b, (a.dtype, a.shape)
    if a.ndim >= 3 and a.shape[1] in (p, 1) and a[0, 0].size == s:
        return a.reshape(b, a.shape[1], s)
    assert a[0].size == s, (a.shape, s)
    return a.reshape(b, 1, s)


def verify_leads(fields, target, thresholds, clamp01=True):
    """fields: fp32 arrays (B, P, ...), (B, 1, ...) or (B, ...); target (B, P, ...) ->
    (counts int64 (P, F, 3 n_thr + 1): [tp, fn, fp] per threshold then the cells of the lead, sums float64 (P, F, 2):
    sum e^2, sum |e|)"""
    target = np.asarray(target)
    b, p = target.shape[:2]
    s = target[0, 0].size
    tg = _frames(target, b, p, s)
    fs = [_frames(f, b, p, s) for f in fields]
    thr = [np.float32(t) for t in thresholds]
    nt = len(thr)
    counts = np.zeros((p, len(fs), 3 * nt + 1), dtype=np.int64)
    sums = np.zeros((p, len(fs), 2), dtype=np.float64)
    lo, hi = np.float32(0), np.float32(1)
    for lead in range(p):
        t = tg[:, lead]
        if clamp01:
            t = np.minimum(np.maximum(t, lo), hi)
        te = [t >= th for th in thr]
        for i, f in enumerate(fs):
            v = f[:, lead if f.shape[1] > 1 else 0]
            if clamp01:
                v = np.minimum(np.maximum(v, lo), hi)
            assert v.dtype == np.float32 and t.dtype == np.float32
            for k, th in enumerate(thr):
                fe = v >= th
                counts[lead, i, 3 * k] = np.count_nonzero(fe & te[k])
                counts[lead, i, 3 * k + 1] = np.count_nonzero(~fe & te[k])
                counts[lead, i, 3 * k + 2] = np.count_nonzero(fe & ~te[k])
            counts[lead, i, 3 * nt] = t.size
            e = v.astype(np.float64) - t.astype(np.float64)
            sums[lead, i, 0] = np.float64(np.sum(e * e, dtype=np.longdouble))
            sums[lead, i, 1] = np.float64(np.sum(np.abs(e), dtype=np.longdouble))
    return counts, sums


def assert_tables(got_counts, got_sums, want_counts, want_sums):
    """counts equal; each sum within sum_tolerance(cells of its lead) relative"""
    got_counts, got_sums = np.asarray(got_counts), np.asarray(got_sums)
    np.testing.assert_array_equal(got_counts, want_counts)
    tol = sum_tolerance(want_counts[..., -1].astype(np.float64))[..., None]
    err = np.abs(got_sums - want_sums)
    assert np.all(err <= tol * np.abs(want_sums)), (err.max(), float((err / np.maximum(np.abs(want_sums), 1e-300)).max()))
