"""Host reference of SignHunter (Al-Dujaili & O'Reilly 2020; not a test module): the segment
schedule restated from the rule, the flip in torch fp32 / int8 on the CPU in the kernel's operation
order, the per-image accept / reject control, and the whole loop on an objective callback."""
import numpy as np
import torch


def schedule(steps, plane):
    """Rows (lo, hi) of queries 1 … steps: level h = 0, 1, … has chunks of len = ceil(plane / 2^h)
    elements, i·len … min((i + 1)·len, plane); after the level with len = 1 the levels restart."""
    rows, h = [], 0
    while len(rows) < steps:
        ln = -(-plane // 2 ** h)
        lo = 0
        while lo < plane and len(rows) < steps:
            rows.append((lo, min(lo + ln, plane)))
            lo += ln
        h = 0 if ln == 1 else h + 1
    return rows


def flip(x, x0, s, accept, prev, new, e, lo=-1.0, hi=1.0):
    """mia_sh_flip on CPU tensors, in place: x, x0 fp32 and s int8 of one (N, …) shape, accept a
    sequence of N 0 / 1 (or None: no revert), prev / new (lo, hi) or None. Per element of either
    range: s *= m, x = clamp(x0 + e·s) with e·s one exact fp32 product and one rounded sum."""
    N = x.shape[0]
    xf, x0f, sf = x.reshape(N, -1), x0.reshape(N, -1), s.reshape(N, -1)
    plane = xf.shape[1]
    j = torch.arange(plane)
    in_prev = (j >= prev[0]) & (j < prev[1]) if prev is not None else torch.zeros(plane, dtype=bool)
    in_new = (j >= new[0]) & (j < new[1]) if new is not None else torch.zeros(plane, dtype=bool)
    union = in_prev | in_new
    ev = torch.tensor(e, dtype=torch.float32)
    for n in range(N):
        revert = accept is not None and int(accept[n]) == 0
        neg = (in_prev & revert) ^ in_new
        sn = torch.where(neg, -sf[n], sf[n])
        xn = torch.clamp(x0f[n] + ev * sn.to(torch.float32), lo, hi)
        sf[n] = torch.where(union, sn, sf[n])
        xf[n] = torch.where(union, xn, xf[n])
    return x


class Control:
    """The decision of one image: best objective, the last accept flag, the count of kept flips
    and the history, all on fp32 values."""

    def __init__(self, L):
        L = np.float32(L)
        self.best, self.accept, self.n_accept = L, 1, 0
        self.loss = [L]
        self.nonfinite = int(not np.isfinite(L))

    def step(self, L):
        L = np.float32(L)
        ok = bool(np.isfinite(L)) and bool(L < self.best)   # a tie, NaN and ±Inf: rejected
        if ok:
            self.best = L
            self.n_accept += 1
        if not np.isfinite(L):
            self.nonfinite = 1
        self.accept = int(ok)
        self.loss.append(L)
        return self.accept

    def state(self):
        return dict(best=self.best, accept=self.accept, n_accept=self.n_accept,
                    nonfinite=self.nonfinite)


# Scripted objectives, one column per image: query 0 then six flips.
NAN, INF = float("nan"), float("inf")
SCRIPTS = {
    "fall": [10, 9, 8, 7, 6, 5, 4],              # every flip kept
    "never": [1, 2, 3, 1.5, 2, 9, 1.25],         # nothing ever below the start
    "tie": [5, 5, 4, 4, 4.5, 3, 3],              # exact ties are rejections
    "nan": [5, NAN, 4, NAN, 4.5, 3, NAN],        # NaN is a rejection, best stays finite
    "inf": [5, INF, 4, -INF, 6, 3.5, INF],       # −Inf is a rejection too
    "nan0": [NAN, 1, 2, 0, NAN, -1, 5],          # a NaN start: nothing compares below it
}


def scripted_losses():
    """(7, len(SCRIPTS)) fp32: row k is query k of every script."""
    return np.array([SCRIPTS[k] for k in SCRIPTS], dtype=np.float32).T.copy()


def replay(loss):
    """The controls of a (queries, N) fp32 history."""
    loss = np.asarray(loss, dtype=np.float32)
    ctl = [Control(loss[0, n]) for n in range(loss.shape[1])]
    for k in range(1, loss.shape[0]):
        for n, c in enumerate(ctl):
            c.step(loss[k, n])
    return ctl


def rebuild(x0, e, loss, rows):
    """(x, s) after replaying a recorded (steps + 1, N) history through the controls and flip():
    what the attack must return if its decisions are a function of the recorded objectives."""
    N = x0.shape[0]
    ctl = [Control(loss[0, n]) for n in range(N)]
    s = torch.full(x0.shape, -1, dtype=torch.int8)
    x = torch.full_like(x0, float("nan"))
    plane = x0[0].numel()
    flip(x, x0, s, None, None, (0, plane), e)
    prev = None
    for k, row in enumerate(rows, start=1):
        flip(x, x0, s, [c.accept for c in ctl], prev, row, e)
        for n, c in enumerate(ctl):
            c.step(loss[k, n])
        prev = row
    if prev is not None:
        flip(x, x0, s, [c.accept for c in ctl], prev, None, e)
    return x, s, ctl


def run(x0, e, steps, objective):
    """The whole attack on ``objective``: x (N, …) fp32 ↦ the per-image values (cast to fp32
    here). Returns dict(x, s, controls, loss (steps + 1, N) fp32)."""
    N = x0.shape[0]
    plane = x0[0].numel()
    if steps == 0:
        return dict(x=x0.clone(), s=None, controls=[], loss=np.zeros((0, N), dtype=np.float32))
    s = torch.full(x0.shape, -1, dtype=torch.int8)
    x = torch.full_like(x0, float("nan"))
    flip(x, x0, s, None, None, (0, plane), e)
    L = np.asarray(objective(x), dtype=np.float32)
    ctl = [Control(L[n]) for n in range(N)]
    prev = None
    for row in schedule(steps, plane):
        flip(x, x0, s, [c.accept for c in ctl], prev, row, e)
        L = np.asarray(objective(x), dtype=np.float32)
        for n, c in enumerate(ctl):
            c.step(L[n])
        prev = row
    flip(x, x0, s, [c.accept for c in ctl], prev, None, e)
    loss = np.array([c.loss for c in ctl], dtype=np.float32).T
    return dict(x=x, s=s, controls=ctl, loss=loss)


def linear_case(plane=192, seed=77):
    """The linear objective L(x) = Σ w_j·x_j of the tests: x0 = 0, e = 0.25, three images with
    w_j = σ_j·(1 + j/plane)·scale_n, σ seeded signs, scales 1e4, 1, 1e-4. Returns (x0, e, w fp64
    (3, plane), σ)."""
    g = torch.Generator().manual_seed(seed)
    sigma = (torch.randint(0, 2, (plane,), generator=g) * 2 - 1).double()
    j = torch.arange(plane, dtype=torch.float64)
    scales = torch.tensor([1e4, 1.0, 1e-4], dtype=torch.float64)
    w = sigma * (1.0 + j / plane) * scales[:, None]
    return torch.zeros(3, plane), 0.25, w, sigma


def linear_objective(w):
    """x ↦ Σ_j w_j·x_j per image in fp64, returned as fp32 (numpy)."""
    def fn(x):
        v = (x.detach().cpu().double().reshape(w.shape[0], -1) * w).sum(1)
        return v.to(torch.float32).numpy()
    return fn
