"""Inputs and the recording run shared by tests/golden/make_loss_goldens.py (against the library of the commit before
csrc/loss.hip) and tests/test_loss_bits_gpu.py (against the library under test): every scalar-loss entry point and its
gradient, results as raw bit patterns.

Inputs come from numpy.random.default_rng(seed) on the CPU, so both sides see the same values on any machine:
h uniform in [-3, 3], targets x / t uniform in [0, 1], predictions p = t + uniform[-3, 3] (both Huber branches at
delta = 1), weight 0.7, upstream gradient 1.3, hinge with sign +1 and -1.

CASES (n, offset): the smallest sizes at which each piece of the launch geometry can go wrong.
  1            n / 16 == 0: the lower clamp of the block count; an empty quad loop with a tail
  1961         the quad path with a one-element tail; one block
  1961, +1     tensors sliced from element 1 of a longer one: misaligned pointers, the single-element path of the L1 forms
  4097         the two block-count formulas disagree (1 and 2 blocks)
  65539        several blocks, several strides per thread, n % 4 == 3
  4198403      = 1024 * 4096 + 4099: the 1024-block cap of both formulas, the 8192-block cap of the MSE / Huber gradients

Keys: `<n>[+1]/<entry point>`: losses as one uint32 (uint64 for sumsq), recon and gradients as uint32 vectors, in full
for n <= 4097 and every 4099th element above.  `ssim/0`: wfae_ssim_fwd on the first image pair of g7_metrics (the
shared finalize kernel behind a third block count)."""
import numpy as np

CASES = [(1, 0), (1961, 0), (1961, 1), (4097, 0), (65539, 0), (1024 * 4096 + 4099, 0)]
WEIGHT, GRAD, DELTA = 0.7, 1.3, 1.0
FULL_UP_TO, STRIDE = 4097, 4099


def case_name(n, off):
    return f"{n}+{off}" if off else str(n)


def inputs(index, n):
    rng = np.random.default_rng(1500 + index)
    h = rng.uniform(-3, 3, n).astype(np.float32)
    x = rng.uniform(0, 1, n).astype(np.float32)
    t = rng.uniform(0, 1, n).astype(np.float32)
    p = (t + rng.uniform(-3, 3, n).astype(np.float32)).astype(np.float32)
    return h, x, p, t


def _bits(v):
    """0-dim or 1-D float tensor -> its bit pattern (uint32 / uint64), vectors thinned above FULL_UP_TO elements"""
    a = np.ascontiguousarray(v.detach().cpu().numpy())
    a = a.reshape(-1).view(np.uint64 if a.dtype == np.float64 else np.uint32)
    return a if a.size <= FULL_UP_TO else a[::STRIDE].copy()


def run_case(ops, torch, dev, index):
    n, off = CASES[index]

    def put(a):   # element `off` of a longer tensor: off = 1 leaves the data pointer 4 bytes past a 16-byte boundary
        buf = torch.zeros(n + off, dtype=torch.float32, device=dev)
        buf[off:] = torch.from_numpy(a)
        v = buf[off:]
        assert v.is_contiguous() and (v.data_ptr() % 16 == 0) == (off == 0)
        return v

    h, x, p, t = (put(a) for a in inputs(index, n))
    g = torch.tensor(GRAD, dtype=torch.float32, device=dev)
    out = {}
    recon, out["sigmoid_l1_fwd"] = ops.sigmoid_l1_fwd(h, x, WEIGHT)
    out["sigmoid_l1_recon"] = recon
    out["sigmoid_l1_bwd"] = ops.sigmoid_l1_bwd(recon, x, g, WEIGHT)
    out["l1_fwd"] = ops.l1_fwd(p, x, WEIGHT)
    out["l1_bwd"] = ops.l1_bwd(p, x, g, WEIGHT)
    out["mean_fwd"] = ops.mean_fwd(h, False, 1.0, WEIGHT)
    out["mean_bwd"] = ops.mean_bwd(h, g, False, 1.0, WEIGHT)
    for tag, sign in (("pos", 1.0), ("neg", -1.0)):
        out[f"hinge_{tag}_fwd"] = ops.mean_fwd(h, True, sign, WEIGHT)
        out[f"hinge_{tag}_bwd"] = ops.mean_bwd(h, g, True, sign, WEIGHT)
    out["sumsq"] = ops.sumsq(h)
    out["mse_fwd"] = ops.mse_fwd(p, t)
    out["mse_bwd"] = ops.mse_bwd(p, t, g)
    out["huber_fwd"] = ops.huber_fwd(p, t, DELTA)
    out["huber_bwd"] = ops.huber_bwd(p, t, g, DELTA)
    torch.cuda.synchronize()
    return {f"{case_name(n, off)}/{k}": _bits(v) for k, v in out.items()}


def run_ssim(ops, torch, dev, g7):
    p, t = torch.from_numpy(g7["0/pred"]).to(dev), torch.from_numpy(g7["0/target"]).to(dev)
    return {"ssim/0": _bits(ops.ssim_fwd(p, t))}
