"""CPU references of the Auto-PGD kernels and of its control rule (torchattacks
APGD.attack_single_run, norm='Linf', eot_iter=1, descending the objective L):

    update    mia_apgd_update in torch fp32 on the CPU, in the kernel's operation order
              (include/miattack.h) — one torch fp32 op per kernel operation, so the bits are the
              kernel's;
    Control   mia_apgd_decide in pure Python, one image at a time, on fp32 objectives;
    schedule  the checkpoints of a run, restated from the rule rather than imported;
    run       the whole loop on a gradient callback (the tests pass the fp64 oracle).

One deviation from torchattacks, shared with the device code: at the first checkpoint step 0 is
compared with the objective at the starting point, not with a zero row reached by loss_steps[-1]."""
import numpy as np
import torch

SAVE, RESTORE = 1, 2
MOMENTUM = 0.75


def _scalar(v):
    return torch.tensor(float(np.float32(v)), dtype=torch.float32)


def schedule(steps):
    """Rows (step index, k, thr): the step at which the window of k steps closes and the integer
    threshold floor(0.75·k)."""
    k = max(int(0.22 * steps), 1)
    k_min = max(int(0.06 * steps), 1)
    dec = max(int(0.03 * steps), 1)
    rows, counter = [], 0
    for i in range(steps):
        counter += 1
        if counter == k:
            rows.append((i, k, int(np.floor(0.75 * k))))
            counter = 0
            k = max(k - dec, k_min)
    return rows


def update(x, x_old, x0, g, eta, a, e, lo=-1.0, hi=1.0):
    """(new x, new x_old) of mia_apgd_update on CPU fp32 tensors; eta: fp32 [N]."""
    assert all(t.dtype == torch.float32 for t in (x, x_old, x0, g, eta))
    a, e = _scalar(a), _scalar(e)
    eta = eta.reshape((-1,) + (1,) * (x.dim() - 1))
    d = x - x_old
    sg = torch.sign(torch.nan_to_num(g, nan=0.0))  # sign(NaN) = 0, as the kernel's comparisons
    lb, ub = x0 - e, x0 + e
    z = torch.clamp(torch.min(torch.max(x - eta * sg, lb), ub), lo, hi)
    b = _scalar(1.0) - a
    s = (x + (z - x) * a) + d * b
    return torch.clamp(torch.min(torch.max(s, lb), ub), lo, hi), x.clone()


class Control:
    """The step-size control of one image on fp32 values (numpy scalars)."""

    def __init__(self, loss0, eta0):
        L = np.float32(loss0)
        self.eta = np.float32(eta0)
        self.L_best = self.L_prev = self.L_check = L
        self.n_dec, self.reduced, self.best_step = 0, 1, 0
        self.loss, self.step_size = [L], [self.eta]
        self.halvings = 0

    def step(self, i, loss, checkpoint=None):
        """After update i with the objective ``loss``; checkpoint: None or (k, thr). Returns the
        action word."""
        L = np.float32(loss)
        act = 0
        if L < self.L_prev:
            self.n_dec += 1
        self.L_prev = L
        if L < self.L_best:
            self.L_best, self.best_step = L, i + 1
            act |= SAVE
        if checkpoint is not None:
            _, thr = checkpoint
            flag = self.n_dec <= thr or (self.reduced == 0 and self.L_check <= self.L_best)
            self.reduced = int(flag)
            self.L_check = self.L_best
            self.n_dec = 0
            if flag:
                self.eta = np.float32(self.eta / np.float32(2))
                self.halvings += 1
                act |= RESTORE
        self.loss.append(L)
        self.step_size.append(self.eta)
        return act

    def state(self):
        return dict(eta=self.eta, L_best=self.L_best, L_prev=self.L_prev, L_check=self.L_check,
                    n_dec=self.n_dec, reduced=self.reduced, best_step=self.best_step)


def replay(losses, eta0):
    """The controls of every image of a recorded (steps + 1, N) objective history."""
    losses = np.asarray(losses, dtype=np.float32)
    steps, N = losses.shape[0] - 1, losses.shape[1]
    rows = {i: (k, thr) for i, k, thr in schedule(steps)}
    ctl = [Control(losses[0, n], eta0) for n in range(N)]
    for i in range(steps):
        for n in range(N):
            ctl[n].step(i, losses[i + 1, n], rows.get(i))
    return ctl


def run(x0, e, steps, grad_loss, x_start=None):
    """The whole attack on the CPU. grad_loss(x) -> (g, L[N]) for an fp32 batch x (any float
    dtype back; both are rounded to fp32 here). Returns dict(x_best, controls, restores, xs) with
    ``restores`` the number of (step, image) restores that changed x and ``xs`` the iterate after
    every step (after the restore)."""
    e32 = float(np.float32(e))
    eta0 = float(np.float32(2.0 * e32))
    x = (x0 if x_start is None else x_start).clone()
    N = x.shape[0]
    g, L = grad_loss(x)
    g, L = g.float(), L.float()
    ctl = [Control(L[n].item(), eta0) for n in range(N)]
    x_old, x_best, g_best = x.clone(), x.clone(), g.clone()
    rows = {i: (k, thr) for i, k, thr in schedule(steps)}
    restores, xs = 0, []
    for i in range(steps):
        eta = torch.tensor([float(c.eta) for c in ctl], dtype=torch.float32)
        x, x_old = update(x, x_old, x0, g, eta, 1.0 if i == 0 else MOMENTUM, e32)
        g, L = grad_loss(x)
        g, L = g.float().clone(), L.float()
        x = x.clone()
        for n in range(N):
            act = ctl[n].step(i, L[n].item(), rows.get(i))
            if act & SAVE:
                x_best[n], g_best[n] = x[n], g[n]
            elif act & RESTORE:
                restores += int(not torch.equal(x[n], x_best[n]))
                x[n], g[n] = x_best[n], g_best[n]
        xs.append(x.clone())
    return dict(x_best=x_best, controls=ctl, restores=restores, xs=xs)


# ---- scripted objective sequences: 6 steps, checkpoints (k, thr) at steps 1, 3 and 5 --------------
# Every sequence starts at L(x_start) = 10 with eta0 = 1; NaN marks a non-finite objective. The
# thresholds are the control's inputs here, not floor(0.75·k): with thr = 1 on a window of 2 a
# checkpoint that does not flag always ends on a new best, so "no new best since a checkpoint that
# did not reduce" can only decide alone where the count's threshold is lower (step 3, thr = 0).
# The expected states, worked by hand, are in tests/test_apgd_host.py.
NAN = float("nan")
SCRIPT_CHECKPOINTS = {1: (2, 1), 3: (2, 0), 5: (2, 1)}
SCRIPTS = {
    # two decreases in every window: never flagged, every step a new best
    "steady": [10, 9, 8, 7, 6, 5, 4],
    # step 1: one decrease in the window, flagged by the count alone (reduced is still 1), and no
    # new best there, so the restore moves x; step 3: neither condition; step 5: the count again
    "count": [10, 9, 9.5, 9.2, 9.6, 9.3, 9.4],
    # step 1: no flag (reduced = 0, L_check = 8); step 3: one decrease > thr = 0, but no new best
    # since step 1: flagged by the second condition alone; step 5: no flag
    "stall": [10, 9, 8, 11, 10.5, 10.2, 10.1],
    # step 1 is the best so far AND flagged by the count: an improvement and a flag in one step
    "both": [10, 12, 9, 8, 7, 6, 5],
    # NaN objectives: never a decrease, never the best, and the step after one is no decrease
    "nan": [10, NAN, 9, NAN, NAN, 8, NAN],
}


def scripted_losses():
    """The scripts as an fp32 (7, 5) history, one column per script in SCRIPTS' order."""
    return np.array([SCRIPTS[k] for k in SCRIPTS], dtype=np.float32).T.copy()
