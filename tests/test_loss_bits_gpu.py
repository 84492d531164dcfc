"""The scalar losses of csrc/loss.hip (sigmoid + L1, L1, mean, hinge, sum of squares, MSE, Huber, and SSIM's finalize)
give, bit for bit, what the separate kernels they replaced gave: tests/golden/g15_loss_bits.npz was recorded from the
library of the commit before the move (tests/golden/make_loss_goldens.py).  The bits of these sums depend on which
elements a thread adds, in which order and precision, and on the block count; tests/loss_bits_ref.py lists the sizes and
what each of them exercises.  No tolerance anywhere."""
import numpy as np
import pytest
import torch

from tests import loss_bits_ref as R
from tests._util import golden

pytestmark = pytest.mark.gpu


def _same_bits(got, g):
    assert got, "nothing was computed"
    for key, bits in got.items():
        want = g[key]
        assert bits.dtype == want.dtype and bits.shape == want.shape, (key, bits.dtype, bits.shape, want.dtype, want.shape)
        bad = np.flatnonzero(bits != want)
        assert np.array_equal(bits, want), f"{key}: {bad.size} of {bits.size} differ, first at {bad[:4]}: " \
                                           f"{[hex(int(b)) for b in bits[bad[:4]]]} != {[hex(int(b)) for b in want[bad[:4]]]}"


@pytest.mark.parametrize("index", range(len(R.CASES)), ids=[R.case_name(*c) for c in R.CASES])
def test_loss_bits(dev, index):
    from weatherforecastingtoolkit_amd import ops
    g = golden("g15_loss_bits")
    got = R.run_case(ops, torch, dev, index)
    prefix = R.case_name(*R.CASES[index]) + "/"
    assert sorted(got) == sorted(k for k in g.files if k.startswith(prefix))
    _same_bits(got, g)


def test_ssim_finalize_bits(dev):
    from weatherforecastingtoolkit_amd import ops
    _same_bits(R.run_ssim(ops, torch, dev, golden("g7_metrics")), golden("g15_loss_bits"))
