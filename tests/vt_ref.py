"""References of the variance-tuning kernels (a helper, not a test module).

The noise is counter-based: Philox4x32-10 as Random123 defines it (Salmon et al., "Parallel random
numbers: as easy as 1, 2, 3"; multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 /
0xBB67AE85, 10 rounds), in numpy on uint64 words masked to 32 bits. fp32, on the CPU, in the
kernels' operation order (include/miattack.h) — one torch fp32 op per kernel operation, so the
results are the kernels' bits:
    mia_vt_neighbor       t = m ? x + c·m : x;  y = t + r·u,
                          u = float(2·(bits >> 8) + 1 − 2^24)·2^-24, bits = word (element % 4) of
                          the block with counter (element / 4, image0 + n, step, sample) and key
                          (seed & 0xffffffff, seed >> 32)
    mia_vt_combine_norms  gt = g + v;  v' = gv ? gv − g : v"""
import numpy as np
import torch

F32 = torch.float32
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """The Philox4x32-10 block of ``counter`` (4 words) under ``key`` (2 words). Every word may be
    an integer or an integer array (broadcast against each other); returns 4 uint32 arrays."""
    c = [np.asarray(w, dtype=np.uint64) & np.uint64(MASK) for w in counter]
    k = [np.asarray(w, dtype=np.uint64) & np.uint64(MASK) for w in key]
    m0, m1, mask, sh = np.uint64(M0), np.uint64(M1), np.uint64(MASK), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]  # 32 × 32 bits: exact in uint64
        c = [(p1 >> sh) ^ c[1] ^ k[0], p1 & mask, (p0 >> sh) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + np.uint64(W0)) & mask, (k[1] + np.uint64(W1)) & mask]
    shape = np.broadcast(*c).shape
    return tuple(np.broadcast_to(w, shape).astype(np.uint32) for w in c)


def uniform64(bits):
    """u of the kernel in fp64 (exact): (2·(bits >> 8) + 1 − 2^24)·2^-24."""
    b = np.asarray(bits, dtype=np.uint32).astype(np.int64)
    return (2 * (b >> 8) + 1 - (1 << 24)).astype(np.float64) * 2.0 ** -24


def uniform(bits):
    """u of the kernel in fp32: an odd integer below 2^24 (exact in fp32) times 2^-24 (exact)."""
    b = np.asarray(bits, dtype=np.uint32).astype(np.int64)
    return (2 * (b >> 8) + 1 - (1 << 24)).astype(np.float32) * np.float32(2.0 ** -24)


def draw(shape, seed, image0, step, sample):
    """The noise u of a batch of ``shape`` = (N, …) as an fp32 tensor: image n, element i of its
    flattened plane takes word i % 4 of the block (i // 4, image0 + n, step, sample)."""
    N = int(shape[0])
    plane = int(np.prod(shape[1:]))
    groups = (plane + 3) // 4
    j = np.arange(groups, dtype=np.uint64).reshape(1, groups)
    n = (np.arange(N, dtype=np.uint64) + np.uint64(image0)).reshape(N, 1)
    seed = int(seed)
    assert 0 <= seed < 1 << 64 and int(image0) + N <= 1 << 32
    words = philox4x32_10((j, n, int(step), int(sample)), (seed & MASK, seed >> 32))
    bits = np.stack(words, axis=-1).reshape(N, groups * 4)[:, :plane]
    return torch.from_numpy(uniform(bits).reshape(tuple(shape)))


def _scalar(v):
    return torch.tensor(float(v), dtype=F32)


def neighbor(x, m, c, r, seed, image0, step, sample):
    """mia_vt_neighbor on CPU fp32 tensors: c·m is rounded, then the sum; r·u is rounded, then the
    sum."""
    assert x.dtype == F32 and x.device.type == "cpu"
    t = x.clone()
    if m is not None:
        assert m.dtype == F32
        look = m * _scalar(c)
        t = x + look
    ru = draw(tuple(x.shape), seed, image0, step, sample) * _scalar(r)
    return t + ru


def combine(g, gv, v):
    """(gt, new v) of mia_vt_combine_norms on CPU fp32 tensors: gt = g + v (the old v);
    v' = gv − g, or v itself when gv is None."""
    assert g.dtype == F32 and v.dtype == F32 and g.device.type == "cpu"
    gt = g + v
    if gv is None:
        return gt, v.clone()
    assert gv.dtype == F32
    return gt, gv - g
