"""References of the universal-perturbation kernels (a helper, not a test module).

fp32 and int64, on the CPU, in the kernels' operation order (include/miattack.h) — one torch fp32
op per kernel operation and exact integer sums, so the results are the kernels' bits:
    mia_uap_accumulate  ĝ = (−g) / (l1[n] / plane);  q = rint(ĝ·2^24) as int64 (0 and the image's
                        flag where |ĝ| < 2·plane does not hold);  acc = (first ? 0 : acc) + Σ_n q
    mia_uap_step        δ = clamp(δ + a·sgn(acc), −e, e);  x[n] = clamp(x0[n] + δ, lo, hi)"""
import torch

F32 = torch.float32
ONE = 2 ** 24  # the fixed point of the per-image terms


def _scalar(v):
    return torch.tensor(float(v), dtype=F32)


def ghat(g, l1):
    """ĝ of mia_uap_accumulate / mia_mi_update, fp32: two fp32 divisions, the mean first."""
    assert g.dtype == F32 and l1.dtype == F32 and g.device.type == "cpu"
    N = g.shape[0]
    plane = g.numel() // N
    mean = l1 / _scalar(plane)
    return (-g) / mean.reshape((N,) + (1,) * (g.dim() - 1))


def terms(g, l1):
    """(q, bad): the int64 terms of every image (g's shape) and the per-image flags (bool [N])."""
    N = g.shape[0]
    plane = g.numel() // N
    gh = ghat(g, l1)
    ok = gh.abs() < _scalar(2.0) * _scalar(plane)          # false for NaN
    q = torch.round(torch.where(ok, gh, torch.zeros_like(gh)).double() * ONE).to(torch.int64)
    return q, (~ok).reshape(N, -1).any(dim=1)


def accumulate(g, l1, acc=None):
    """(acc, bad) of mia_uap_accumulate: the int64 plane [plane] (added to ``acc`` unless it is
    None = first) and the images it flags."""
    q, bad = terms(g, l1)
    s = q.reshape(g.shape[0], -1).sum(dim=0)
    return (s if acc is None else acc.reshape(-1) + s), bad


def step(delta, acc, x0, a, e, lo=-1.0, hi=1.0):
    """(δ, x) of mia_uap_step: delta fp32 of one plane's shape, acc int64 [plane] or None (δ
    unchanged), x0 (N, …) or None (δ only: x is None)."""
    assert delta.dtype == F32
    d = delta
    if acc is not None:
        sg = torch.sign(acc).to(F32).reshape(delta.shape)
        d = torch.clamp(delta + _scalar(a) * sg, -float(e), float(e))
    if x0 is None:
        return d, None
    return d, torch.clamp(x0 + d.reshape((1,) + tuple(x0.shape[1:])), float(lo), float(hi))
