"""fp64 reference of the input-diversity transform (a helper, not a test module).

D(x) = zero_pad(bilinear(x, (rnd, rnd), align_corners=False), top, left) is separable and linear:
per plane D(x) = Ry·x·Rxᵀ and Dᵀg = Ryᵀ·g·Rx with R = rmat(S, rnd, offset) of one axis, built from
the integer rule of mia_di_resize_pad (include/miattack.h): output o reads
    n = (2o+1)·S − rnd,  d = 2·rnd:  i0 = n // d,  i1 = min(i0 + 1, S − 1),  λ = (n − i0·d) / d
with weights 1 − λ = (d − (n − i0·d)) / d on i0 and λ on i1."""
import torch


def rmat(S, rnd, off):
    """The fp64 S × S matrix of one axis: row off + o holds the two weights of output o; the
    rows outside off … off + rnd − 1 (the padding) are zero."""
    if not (1 <= rnd <= S and 0 <= off and off + rnd <= S):
        raise ValueError("need 1 <= rnd <= S and 0 <= off <= S - rnd")
    R = torch.zeros(S, S, dtype=torch.float64)
    d = 2 * rnd
    for o in range(rnd):
        n = (2 * o + 1) * S - rnd
        i0 = n // d
        i1 = min(i0 + 1, S - 1)
        r = n - i0 * d
        R[off + o, i0] += (d - r) / d
        R[off + o, i1] += r / d
    return R


def resize_pad(x, rnd, top, left):
    """D(x) in fp64 for x of shape (..., S, S)."""
    S = x.shape[-1]
    return rmat(S, rnd, top) @ x.double() @ rmat(S, rnd, left).T


def resize_pad_adjoint(g, rnd, top, left):
    """Dᵀg in fp64 for g of shape (..., S, S)."""
    S = g.shape[-1]
    return rmat(S, rnd, top).T @ g.double() @ rmat(S, rnd, left)
