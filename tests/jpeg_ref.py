"""References of the JPEG round trip J and of the adjoint of its differentiable surrogate (not a
test module).

* ``roundtrip32`` / ``adjoint32``: elementwise torch fp32 with the operation order of
  include/miattack.h (mia_jpeg_roundtrip / mia_jpeg_bwd_norms) — every line below is one fp32
  operation, so the HIP kernels reproduce the bits.
* ``roundtrip64`` / ``adjoint64``: the same transform in fp64 on the same fp32-rounded constants
  (the difference to fp32 is then rounding of the operations alone); the adjoint comes from
  autograd on the surrogate r.detach() + (v − r.detach())³ of the coefficient rounding, straight
  through the pixel roundings and clamps.

Images are (N,3,S,S) in [-1,1], S % 8 == 0; ``qtab`` is the (2,64) table of quantiser steps
(luminance, chrominance; natural order) as any numeric tensor."""
import numpy as np
import torch

from gfa_amd.pgd import jpeg_dct_matrix


def f32(v):
    return float(np.float32(v))


# RGB → YCbCr (rows Y, Cb, Cr) and YCbCr → RGB (rows R, G, B), rounded to fp32 once
A = [[f32(0.299), f32(0.587), f32(0.114)],
     [f32(-0.168736), f32(-0.331264), f32(0.5)],
     [f32(0.5), f32(-0.418688), f32(-0.081312)]]
M_R_CR, M_G_CB, M_G_CR, M_B_CB = f32(1.402), f32(-0.344136), f32(-0.714136), f32(1.772)
D = [[float(v) for v in row] for row in jpeg_dct_matrix()]


def _blocks(p):
    """(N,3,S,S) → (N,3,S/8,8,S/8,8): axes (n, c, block row, iy, block column, ix)."""
    N, C, S, _ = p.shape
    return p.reshape(N, C, S // 8, 8, S // 8, 8)


def _dct_axis(v, axis, inv):
    """The 8-point pass along ``axis``: o[u] = Σ_k D[u][k]·v[k], or Σ_k D[k][u]·v[k] (inv):
    d[0]·v[0], then + d[k]·v[k] for k = 1 … 7."""
    v = v.movedim(axis, -1)
    out = []
    for u in range(8):
        s = (D[0][u] if inv else D[u][0]) * v[..., 0]
        for k in range(1, 8):
            s = s + (D[k][u] if inv else D[u][k]) * v[..., k]
        out.append(s)
    return torch.stack(out, -1).movedim(-1, axis)


def dct2(b):
    """F = D·B·Dᵀ per block of a (N,3,S/8,8,S/8,8) tensor: rows first, then columns."""
    return _dct_axis(_dct_axis(b, 5, False), 3, False)


def idct2(f):
    """o = Dᵀ·F·D: columns first, then rows."""
    return _dct_axis(_dct_axis(f, 3, True), 5, True)


def _qblocks(qtab, like):
    """The steps as (1,3,1,8,1,8) (channel 0: luminance; 1, 2: chrominance): Q[c][u][v] sits at
    vertical frequency u = iy, horizontal v = ix."""
    q = torch.as_tensor(qtab).to(like.dtype).reshape(2, 8, 8)
    return torch.stack([q[0], q[1], q[1]]).reshape(1, 3, 1, 8, 1, 8)


def pixels(x):
    """Step 1: floor(clamp((x + 1)·127.5 + 0.5, 0, 255))."""
    return torch.floor(torch.clamp((x + 1.0) * 127.5 + 0.5, 0.0, 255.0))


def to_ycc(p):
    r, g, b = p[:, 0], p[:, 1], p[:, 2]
    y = ((A[0][0] * r + A[0][1] * g) + A[0][2] * b) - 128.0
    cb = (A[1][0] * r + A[1][1] * g) + A[1][2] * b
    cr = (A[2][0] * r + A[2][1] * g) + A[2][2] * b
    return torch.stack([y, cb, cr], 1)


def to_rgb(o):
    y, cb, cr = o[:, 0] + 128.0, o[:, 1], o[:, 2]
    r = y + M_R_CR * cr
    g = (y + M_G_CB * cb) + M_G_CR * cr
    b = y + M_B_CB * cb
    return torch.stack([r, g, b], 1)


def coefficients(x, qtab):
    """Steps 1 – 4 up to the division: v = F / Q as (N,3,S/8,8,S/8,8), and Q in that shape."""
    F = dct2(_blocks(to_ycc(pixels(x))))
    q = _qblocks(qtab, x)
    return F / q, q


def _roundtrip(x, qtab):
    v, q = coefficients(x, qtab)
    r = torch.round(v)
    rgb = to_rgb(idct2(r * q).reshape(x.shape))
    y = torch.clamp(torch.round(rgb), 0.0, 255.0) / 127.5 - 1.0
    return y, v


def roundtrip32(x, qtab):
    """(J(x), v) in fp32 with the kernels' operation order; v are the coefficients before the
    rounding, (N,3,S/8,8,S/8,8)."""
    assert x.dtype == torch.float32
    return _roundtrip(x, qtab)


def roundtrip64(x, qtab):
    return _roundtrip(x.double(), qtab)


def adjoint32(x, g, qtab):
    """gx = Aᵀ·IDCT(w ⊙ DCT(Mᵀ·g)), w = 3·(v − round(v))² at x, in fp32 with the kernel's order."""
    assert x.dtype == torch.float32 and g.dtype == torch.float32
    v, _ = coefficients(x, qtab)
    d = v - torch.round(v)
    w = 3.0 * (d * d)
    gr, gg, gb = g[:, 0], g[:, 1], g[:, 2]
    h = torch.stack([(gr + gg) + gb, M_G_CB * gg + M_B_CB * gb, M_R_CR * gr + M_G_CR * gg], 1)
    u = idct2(w * dct2(_blocks(h))).reshape(x.shape)
    uy, ub, ur = u[:, 0], u[:, 1], u[:, 2]
    return torch.stack([(A[0][c] * uy + A[1][c] * ub) + A[2][c] * ur for c in range(3)], 1)


def surrogate64(x, qtab):
    """The differentiable surrogate of J in fp64 (autograd-ready): the coefficient rounding is
    r.detach() + (v − r.detach())³, the pixel roundings and clamps are straight through."""
    x1 = (x + 1.0) * 127.5
    p = x1 + (pixels(x) - x1).detach()
    F = dct2(_blocks(to_ycc(p)))
    q = _qblocks(qtab, x)
    v = F / q
    r = torch.round(v).detach()
    rgb = to_rgb(idct2((r + (v - r) ** 3) * q).reshape(x.shape))
    pq = rgb + (torch.clamp(torch.round(rgb), 0.0, 255.0) - rgb).detach()
    return pq / 127.5 - 1.0


def adjoint64(x, g, qtab):
    """J′(x)ᵀ g of the surrogate by autograd, fp64."""
    xd = x.double().requires_grad_(True)
    y = surrogate64(xd, qtab)
    gx, = torch.autograd.grad(y, xd, g.double())
    return gx


def test_image(seed=0, size=64):
    """A seeded (1,3,size,size) image with natural-image statistics: a bicubic-upsampled 9 × 9
    normal field ·0.5, plus 0.08·normal noise, clamped to [-1,1]."""
    gen = torch.Generator().manual_seed(seed)
    low = torch.randn(1, 3, 9, 9, generator=gen) * 0.5
    img = torch.nn.functional.interpolate(low, size=(size, size), mode="bicubic",
                                          align_corners=False)
    img = img + 0.08 * torch.randn(1, 3, size, size, generator=gen)
    return img.clamp(-1.0, 1.0).contiguous()
