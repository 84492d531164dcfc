"""Generate tests/golden/g15_loss_bits.npz: what the scalar losses computed BEFORE they moved into csrc/loss.hip.

    python tests/golden/make_loss_goldens.py <libwfae.so built from the commit before csrc/loss.hip>

Runs on the GPU.  The C ABI did not change with the move, so the current Python package drives the old library:
`_lib.load(path)` binds it before anything else loads the in-tree one.  The fixture records that library's results as
bit patterns (inputs, cases and keys: tests/loss_bits_ref.py); tests/test_loss_bits_gpu.py asks the library under test
for the same bits.  Never regenerate it from the code under test: if a build disagrees with the fixture, the build is
wrong.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import loss_bits_ref as R  # noqa: E402
from tests._util import golden  # noqa: E402


def main(argv):
    if len(argv) < 2:
        raise SystemExit(__doc__)
    from weatherforecastingtoolkit_amd import _lib
    lib = _lib.load(os.path.abspath(argv[1]))
    assert lib is _lib.load(), "another libwfae.so was loaded first"
    from weatherforecastingtoolkit_amd import ops
    dev = torch.device("cuda:0")
    out = {}
    for index in range(len(R.CASES)):
        out.update(R.run_case(ops, torch, dev, index))
    out.update(R.run_ssim(ops, torch, dev, golden("g7_metrics")))
    path = argv[2] if len(argv) > 2 else os.path.join(HERE, "g15_loss_bits.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes,", len(out), "arrays from", os.path.abspath(argv[1]))
    if size > 1_000_000:
        raise SystemExit(f"{path}: {size} bytes exceeds the 1 000 000 byte limit for a committed fixture")


if __name__ == "__main__":
    main(sys.argv)
