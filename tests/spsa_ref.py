"""References of the SPSA kernels (a helper, not a test module).

The directions are counter-based: Philox4x32-10 of tests/vt_ref.py (imported, the same generator
the variance-tuning noise uses), counter (element / 4, image0 + n, step, sample), key
(seed & 0xffffffff, seed >> 32); element i takes word i % 4 and v = +1 where its bit 31 is 0, −1
where it is 1. fp32, on the CPU, in the kernels' operation order (include/miattack.h) — one torch
fp32 op per kernel operation, so the results are the kernels' bits:
    mia_spsa_probe             t = v > 0 ? d : −d;  yp = clamp(x + t, lo, hi);
                               ym = clamp(x − t, lo, hi)
    mia_spsa_accumulate_norms  c = (fp[n] − fm[n])·s;  t = v > 0 ? c : −c;
                               r = first ? t : acc + t;  div ≠ 1: r = r / div
and, in fp64, the estimator itself:
    ĝ = (1/q)·Σ_i ((f(x⁺_i) − f(x⁻_i))/(2·d))·v_i"""
import numpy as np
import torch

from vt_ref import MASK, philox4x32_10

F32 = torch.float32


def words(shape, seed, image0, step, sample):
    """The Philox words of a batch of ``shape`` = (N, …) as a uint32 array of that shape: image n,
    element i of its flattened plane takes word i % 4 of the block (i // 4, image0 + n, step,
    sample)."""
    N = int(shape[0])
    plane = int(np.prod(shape[1:]))
    groups = (plane + 3) // 4
    j = np.arange(groups, dtype=np.uint64).reshape(1, groups)
    n = (np.arange(N, dtype=np.uint64) + np.uint64(image0)).reshape(N, 1)
    seed = int(seed)
    assert 0 <= seed < 1 << 64 and int(image0) + N <= 1 << 32
    w = philox4x32_10((j, n, int(step), int(sample)), (seed & MASK, seed >> 32))
    return np.stack(w, axis=-1).reshape(N, groups * 4)[:, :plane].reshape(tuple(shape))


def sign_of(bits):
    """v of the kernels for Philox words ``bits``: +1 where bit 31 is 0, −1 where it is 1 (fp32)."""
    b = np.asarray(bits, dtype=np.uint32)
    return np.where((b >> np.uint32(31)) == 0, np.float32(1.0), np.float32(-1.0))


def directions(shape, seed, image0, step, sample):
    """The Rademacher directions of a batch of ``shape`` as an fp32 tensor of ±1."""
    return torch.from_numpy(sign_of(words(shape, seed, image0, step, sample)))


def _scalar(v):
    return torch.tensor(float(v), dtype=F32)


def probe(x, d, seed, image0, step, sample, lo=-1.0, hi=1.0):
    """(yp, ym) of mia_spsa_probe on a CPU fp32 tensor: t = ±d (exact), one rounding for x + t and
    one for x − t, then the clamp."""
    assert x.dtype == F32 and x.device.type == "cpu"
    t = directions(tuple(x.shape), seed, image0, step, sample) * _scalar(d)
    return torch.clamp(x + t, float(lo), float(hi)), torch.clamp(x - t, float(lo), float(hi))


def coefficient(fp, fm, s):
    """c of mia_spsa_accumulate_norms, fp32 [N]: the difference rounded, then the product."""
    assert fp.dtype == F32 and fm.dtype == F32
    return (fp - fm) * _scalar(s)


def accumulate(acc, fp, fm, s, seed, image0, step, sample, first, div=1.0):
    """The new acc of mia_spsa_accumulate_norms on CPU fp32 tensors (acc is not read when first)."""
    assert acc.dtype == F32 and acc.device.type == "cpu"
    c = coefficient(fp, fm, s).reshape((-1,) + (1,) * (acc.dim() - 1))
    t = directions(tuple(acc.shape), seed, image0, step, sample) * c   # ±c: exact
    r = t if first else acc + t
    if float(div) != 1.0:
        r = r / _scalar(div)
    return r


def estimate(objective_fn, x, q, d, seed, image0, step):
    """The SPSA estimate in fp64: objective_fn maps an fp64 batch to its per-image objective
    (fp64 [N]); x is the iterate, d the probe radius in x's units. The probes are clamped to
    [−1, 1] as the attack's are."""
    x = x.double()
    g = torch.zeros_like(x)
    for i in range(q):
        v = directions(tuple(x.shape), seed, image0, step, i).double()
        fp = objective_fn(torch.clamp(x + d * v, -1.0, 1.0))
        fm = objective_fn(torch.clamp(x - d * v, -1.0, 1.0))
        c = (fp - fm) / (2.0 * d)
        g += c.reshape((-1,) + (1,) * (x.dim() - 1)) * v
    return g / q
