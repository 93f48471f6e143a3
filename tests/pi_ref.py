"""fp32 CPU reference of the patch-wise attack's step (PI-FGSM; mia_pi_update, include/miattack.h):
one torch fp32 op per kernel operation, so the bits are the kernel's. The window sum is written as
explicit shifted additions in the contract order — from 0, window rows (dy) outer and columns (dx)
inner, both ascending, the centre left out, zero padding — never as a convolution, whose summation
order is torch's business. ``reverse=True`` walks the window backwards: a different rounding
sequence, used only to show that a test really depends on the order. Not a test module."""
import numpy as np
import torch

F32 = torch.float32


def f32(v):
    return float(np.float32(v))


def t32(v):
    return torch.tensor(v, dtype=F32)


def steps(alpha, beta, project=1.0):
    """(a, ab, gm) in [-1,1] units, one fp32 rounding per operation."""
    a = np.float32(2.0 * alpha)
    ab = np.float32(beta) * a
    gm = np.float32(project) * ab
    return float(a), float(ab), float(gm)


def sign(t):
    """−1, 0, +1 by comparison, as the kernel takes it (a NaN gives 0)."""
    return (t > 0).to(F32) - (t < 0).to(F32)


def window_sum(C, k, reverse=False):
    """S[y, x] = Σ_{dy} Σ_{dx, (dy, dx) ≠ (0, 0)} C[y + dy, x + dx] per plane of C (N,C,H,W): plain
    fp32 additions starting from 0 in the contract order; outside the plane C is 0. Adding a
    padded +0 leaves every partial sum's bits alone (a partial sum is never −0: it starts at +0,
    and x + (−x) = +0), so the padded form equals the one that skips those terms."""
    r = k // 2
    H, W = C.shape[-2:]
    P = torch.zeros(C.shape[:-2] + (H + 2 * r, W + 2 * r), dtype=F32)
    P[..., r:r + H, r:r + W] = C
    offs = [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if (dy, dx) != (0, 0)]
    if reverse:
        offs.reverse()
    S = torch.zeros_like(C)
    for dy, dx in offs:
        S = S + P[..., r + dy:r + dy + H, r + dx:r + dx + W]
    return S


def parts(g, l1, m, A, mu, ab, e, k, reverse=False):
    """Everything the step forms before it touches x: m', s, A', the cut noise C and S."""
    n, plane = g.shape[0], g[0].numel()
    mean = l1 / t32(float(plane))
    gh = (-g) / mean.reshape(n, 1, 1, 1)
    mm = gh + t32(mu) * m
    s = sign(mm)
    Ap = A + t32(ab) * s
    C = sign(Ap) * torch.clamp(Ap.abs() - t32(e), min=0.0)
    return dict(gh=gh, mm=mm, s=s, Ap=Ap, C=C, S=window_sum(C, k, reverse))


def update(x, x0, g, l1, m, A, mu, ab, gm, e, k, lo=-1.0, hi=1.0, reverse=False):
    """One step: (x, m, A, nonfinite) after it; the inputs are not modified."""
    q = parts(g, l1, m, A, mu, ab, e, k, reverse)
    p = t32(gm) * sign(q["S"])
    A1 = q["Ap"] + p
    u = x + t32(ab) * q["s"]
    v = u + p
    d = torch.clamp(v - x0, -e, e)
    x1 = torch.clamp(x0 + d, lo, hi)
    nf = (~torch.isfinite(q["gh"])).reshape(g.shape[0], -1).any(dim=1).to(torch.int32)
    return x1, q["mm"], A1, nf


def mi_update(x, x0, g, l1, m, mu, a, e, lo=-1.0, hi=1.0):
    """mia_mi_update's rule (torchattacks MIFGSM on cost = −L) in the same style: (x, m)."""
    n, plane = g.shape[0], g[0].numel()
    mean = l1 / t32(float(plane))
    gh = (-g) / mean.reshape(n, 1, 1, 1)
    mm = gh + t32(mu) * m
    adv = x + t32(a) * sign(mm)
    d = torch.clamp(adv - x0, -e, e)
    return torch.clamp(x0 + d, lo, hi), mm


def l1_of(g):
    """Σ|g| per image, fp32 (any positive value serves a kernel test: both sides read it)."""
    return g.abs().reshape(g.shape[0], -1).sum(dim=1)


def seeded(seed, shape):
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=gen) * 2 - 1


IMG_SCALES = (1e4, 1.0, 1e-4)  # per-image gradient scales: cross-image mixing cannot hide


def case(H, W, seed=0, n=3, c=3, e=f32(2 * 8 / 255)):
    """Seeded inputs of one kernel case: x0, x inside the ball, g with per-image scales, a non-zero
    m, and an A with |A| below and above e in both signs (3·e·U(−1, 1): a third inside)."""
    shape = (n, c, H, W)
    sc = torch.tensor(IMG_SCALES[:n], dtype=F32).reshape(n, 1, 1, 1)
    x0 = seeded(7000 + seed, shape)
    x = torch.clamp(x0 + t32(e) * seeded(7001 + seed, shape), -1.0, 1.0)
    g = seeded(7002 + seed, shape) * sc
    m = 2.0 * seeded(7003 + seed, shape)
    A = t32(3.0 * e) * seeded(7004 + seed, shape)
    return dict(x=x, x0=x0, g=g, l1=l1_of(g), m=m, A=A)


def order_case():
    """One 20 × 24 plane (k = 3) on which the order of the window sum decides signs. e = 0.5,
    ab = 0.25, μ = 0 and g < 0 everywhere, so s = +1 and A' = A + 0.25 exactly. Rows 4, 9 and 14
    carry the cut-noise triple (B, b, −B) = (2^20, 2^-4, −2^20) in columns 7, 8, 9 and 15, 16, 17
    (A = 2^20 + 0.25, 0.3125 and −2^20 − 0.75, all exact), magnitudes 2^24 apart: below them, the
    pixel in the middle column sums B + b = B (b is half an ulp of B, ties to even), then −B: 0 in
    the contract order, and −B + b = −(2^20 − 2^-4) exactly, then + B: b > 0, backwards. Elsewhere
    A is 0.2·U(−1, 1) − 0.25 or so: inside the ball, C = 0, with a seeded sprinkle of mixed
    overflows between 2^-6 and 2^18. Returns (inputs, constants)."""
    H, W, e, ab = 20, 24, 0.5, 0.25
    shape = (1, 1, H, W)
    A = 0.2 * seeded(7100, shape) - 0.25
    gen = torch.Generator().manual_seed(7101)
    for _ in range(24):
        y, xx = int(torch.randint(0, H, (1,), generator=gen)), int(torch.randint(0, W, (1,), generator=gen))
        mag = 2.0 ** float(torch.randint(-6, 19, (1,), generator=gen))
        sg = 1.0 if int(torch.randint(0, 2, (1,), generator=gen)) else -1.0
        A[0, 0, y, xx] = sg * (mag + e) - ab
    B = 2.0 ** 20
    for y in (4, 9, 14):
        for x0c in (7, 15):
            A[0, 0, y - 1:y + 3, x0c - 1:x0c + 4] = -0.25      # quiet round the triple and below
            A[0, 0, y, x0c], A[0, 0, y, x0c + 1], A[0, 0, y, x0c + 2] = B + 0.25, 0.3125, -B - 0.75
    g = -(seeded(7102, shape).abs() + 0.5)
    x0 = seeded(7103, shape)
    x = torch.clamp(x0 + 0.25 * seeded(7104, shape), -1.0, 1.0)
    m = seeded(7105, shape)
    return dict(x=x, x0=x0, g=g, l1=l1_of(g), m=m, A=A), dict(mu=0.0, ab=ab, gm=0.125, e=e, k=3)
