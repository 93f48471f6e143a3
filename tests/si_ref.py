"""References of the scale-invariant / Nesterov kernels (a helper, not a test module).

fp32, on the CPU, in the kernels' operation order (include/miattack.h) — one torch fp32 op per
kernel operation, so the results are the kernels' bits:
    mia_si_transform         t = m ? x + c·m : x;  y = s == 1 ? t : (t + 1)·s − 1
    mia_si_accumulate_norms  v = w·g;  r = first ? v : acc + v;  div ≠ 1: r = r / div
and the fp64 scale copy S_i(x) = (x + 1)·2^-i − 1: torchattacks SINIFGSM's p / 2^i on
p = (x + 1)/2 ∈ [0,1], written in [-1,1] units (towards black: −1 is the fixed point)."""
import torch

F32 = torch.float32


def _scalar(v):
    return torch.tensor(float(v), dtype=F32)


def transform(x, m, c, s):
    """mia_si_transform on CPU fp32 tensors: the product c·m is rounded, then the sum; the scale
    is an add, a multiplication and a subtraction, each rounded."""
    assert x.dtype == F32 and x.device.type == "cpu"
    t = x.clone()
    if m is not None:
        assert m.dtype == F32
        look = m * _scalar(c)
        t = x + look
    if float(s) != 1.0:
        p = t + _scalar(1.0)
        ps = p * _scalar(s)
        t = ps - _scalar(1.0)
    return t


def accumulate(g, acc, w, first, div=1.0):
    """mia_si_accumulate_norms' new accumulator on CPU fp32 tensors (acc is ignored when first).
    The division is IEEE, by a tensor (never a multiplication by a rounded reciprocal)."""
    assert g.dtype == F32 and g.device.type == "cpu"
    r = g * _scalar(w)
    if not first:
        assert acc.dtype == F32
        r = acc + r
    if float(div) != 1.0:
        r = r / torch.full_like(r, float(div))
    return r


def scale64(x, i):
    """S_i(x) in fp64."""
    return (x.double() + 1.0) * 2.0 ** -int(i) - 1.0
