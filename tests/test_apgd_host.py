"""Host side of Auto-PGD (no GPU): the checkpoint schedule against hand-worked rows, the control
reference on scripted objective sequences against states written out by hand, attack()'s and
fgsm()'s argument validation before any device work, the wrappers' host checks, and the C ABI's
validation of mia_apgd_update / mia_apgd_decide / mia_apgd_apply."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

import apgd_ref
from test_si_host import _StubNet


# ---- the schedule ---------------------------------------------------------------------------------
def test_schedule_hand_worked_rows():
    from gfa_amd.pgd import apgd_schedule
    # steps = 10: k0 = int(2.2) = 2, k_min = max(int(0.6), 1) = 1, dec = max(int(0.3), 1) = 1
    want10 = [(1, 2, 1)] + [(i, 1, 0) for i in range(2, 10)]
    # steps = 100: k0 = 22, k_min = 6, dec = 3: windows 22, 19, 16, 13, 10, 7, 6, 6 close at
    # steps 21, 40, 56, 69, 79, 86, 92, 98; thr = floor(0.75·k)
    want100 = [(21, 22, 16), (40, 19, 14), (56, 16, 12), (69, 13, 9), (79, 10, 7), (86, 7, 5),
               (92, 6, 4), (98, 6, 4)]
    for fn in (apgd_schedule, apgd_ref.schedule):
        assert fn(10) == want10
        assert fn(100) == want100
        assert fn(1) == [(0, 1, 0)]          # k0 = k_min = dec = 1: the only step is a checkpoint
        assert fn(0) == []
        assert fn(3) == [(0, 1, 0), (1, 1, 0), (2, 1, 0)]
    for steps in range(0, 260):
        rows = apgd_schedule(steps)
        assert rows == apgd_ref.schedule(steps)
        assert all(thr == math.floor(0.75 * k) and 0 <= i < steps for i, k, thr in rows)
        ends = [i for i, _, _ in rows]
        assert ends == sorted(set(ends))
        # the windows tile the steps from 0 on
        assert all(e - (p if j else -1) == rows[j][1]
                   for j, (e, p) in enumerate(zip(ends, [None] + ends[:-1])))
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError):
            apgd_schedule(bad)
    assert apgd_schedule(np.int64(10)) == want10


# ---- the control reference on scripted sequences --------------------------------------------------
NAN = float("nan")
# per script: the action word of every step, eta after every step (row 0: the start) and the final
# state, worked by hand from the rule with checkpoints (k, thr) = (2, 1), (2, 0), (2, 1) at steps
# 1, 3, 5 (1 = SAVE, 2 = RESTORE, 3 = both)
EXPECT = {
    "steady": dict(actions=[1, 1, 1, 1, 1, 1], eta=[1, 1, 1, 1, 1, 1, 1], halvings=0,
                   state=dict(eta=1, L_best=4, L_prev=4, L_check=4, n_dec=0, reduced=0,
                              best_step=6)),
    "count": dict(actions=[1, 2, 0, 0, 0, 2], eta=[1, 1, .5, .5, .5, .5, .25], halvings=2,
                  state=dict(eta=.25, L_best=9, L_prev=9.4, L_check=9, n_dec=0, reduced=1,
                             best_step=1)),
    "stall": dict(actions=[1, 1, 0, 2, 0, 0], eta=[1, 1, 1, 1, .5, .5, .5], halvings=1,
                  state=dict(eta=.5, L_best=8, L_prev=10.1, L_check=8, n_dec=0, reduced=0,
                             best_step=2)),
    "both": dict(actions=[0, 3, 1, 1, 1, 1], eta=[1, 1, .5, .5, .5, .5, .5], halvings=1,
                 state=dict(eta=.5, L_best=5, L_prev=5, L_check=5, n_dec=0, reduced=0,
                            best_step=6)),
    "nan": dict(actions=[0, 3, 0, 2, 1, 2], eta=[1, 1, .5, .5, .25, .25, .125], halvings=3,
                state=dict(eta=.125, L_best=8, L_prev=NAN, L_check=8, n_dec=0, reduced=1,
                           best_step=5)),
}
# the state in the middle of two scripts, after step 3 (the checkpoint with thr = 0)
MIDWAY = {
    "stall": dict(eta=.5, L_best=8, L_prev=10.5, L_check=8, n_dec=0, reduced=1, best_step=2),
    "count": dict(eta=.5, L_best=9, L_prev=9.6, L_check=9, n_dec=0, reduced=0, best_step=1),
}


def same(a, b):
    a, b = np.float32(a), np.float32(b)
    return bool(a == b) or bool(np.isnan(a) and np.isnan(b))


def check_state(got, want, where):
    for k, v in want.items():
        assert same(got[k], v), (where, k, got[k], v)


@pytest.mark.parametrize("name", list(apgd_ref.SCRIPTS))
def test_control_reference_on_scripted_sequences(name):
    seq, exp = apgd_ref.SCRIPTS[name], EXPECT[name]
    assert list(apgd_ref.SCRIPTS) == list(EXPECT) and len(seq) == 7
    c = apgd_ref.Control(seq[0], 1.0)
    check_state(c.state(), dict(eta=1, L_best=10, L_prev=10, L_check=10, n_dec=0, reduced=1,
                                best_step=0), (name, "start"))
    acts = []
    for i in range(6):
        acts.append(c.step(i, seq[i + 1], apgd_ref.SCRIPT_CHECKPOINTS.get(i)))
        if i == 3 and name in MIDWAY:
            check_state(c.state(), MIDWAY[name], (name, "after step 3"))
    assert acts == exp["actions"]
    assert [float(v) for v in c.step_size] == exp["eta"]
    assert all(same(a, b) for a, b in zip(c.loss, seq)) and len(c.loss) == 7
    assert c.halvings == exp["halvings"]
    check_state(c.state(), exp["state"], (name, "end"))
    # the best objective is the minimum of the finite ones, first reached at best_step
    finite = [v for v in np.float32(seq) if not np.isnan(v)]
    assert c.L_best == min(finite) and np.float32(seq[c.best_step]) == c.L_best


def test_scripts_hit_every_branch():
    """By the expected action words and states: a flag by the count alone (count, step 1), a flag
    by the second condition alone (stall, step 3: one decrease against thr = 0), checkpoints
    without a flag (steady), an improvement and a flag in one step (both, step 1), a restore that
    is not an identity (count), and NaN objectives."""
    assert EXPECT["count"]["actions"][1] == apgd_ref.RESTORE
    assert EXPECT["stall"]["actions"][3] == apgd_ref.RESTORE
    assert EXPECT["steady"]["halvings"] == 0
    assert EXPECT["both"]["actions"][1] == apgd_ref.SAVE | apgd_ref.RESTORE
    assert math.isnan(EXPECT["nan"]["state"]["L_prev"])
    L = apgd_ref.scripted_losses()
    assert L.shape == (7, 5) and L.dtype == np.float32
    ctl = [apgd_ref.Control(L[0, n], 1.0) for n in range(5)]
    for i in range(6):
        for n in range(5):
            ctl[n].step(i, L[i + 1, n], apgd_ref.SCRIPT_CHECKPOINTS.get(i))
    for n, name in enumerate(apgd_ref.SCRIPTS):
        check_state(ctl[n].state(), EXPECT[name]["state"], name)


def test_replay_uses_the_schedule():
    """replay() on a (steps + 1, N) history: steps = 4 has a checkpoint with k = 1, thr = 0 after
    every step, so every step that is no decrease halves eta."""
    L = np.array([[5, 5], [4, 6], [4.5, 5.5], [3, 5.2], [3.5, 5.1]], dtype=np.float32)
    a, b = apgd_ref.replay(L, 0.25)
    assert [float(v) for v in a.step_size] == [.25, .25, .125, .125, .0625]
    assert a.best_step == 3 and a.halvings == 2
    # image 1 never gets below its start: step 0 is flagged by the count, steps 1 - 3 decrease
    # (n_dec = 1 > 0) but reduced is 1 after step 0 → no flag at step 1 (reduced becomes 0), then
    # "no new best since a checkpoint that did not reduce" at step 2, nothing at step 3
    assert [float(v) for v in b.step_size] == [.25, .125, .125, .0625, .0625]
    assert b.best_step == 0 and b.halvings == 2


def test_update_reference_by_hand():
    """Exact small numbers: e = 0.25, eta = 0.5, x0 = 0."""
    x0 = torch.zeros(1, 6)
    x = torch.tensor([[0.0, 0.125, -0.25, 0.25, 0.0, 0.0]])
    x_old = torch.tensor([[0.0, 0.0, -0.25, 0.125, 0.125, 0.0]])
    g = torch.tensor([[1.0, -1.0, -2.0, 3.0, 0.0, NAN]])
    eta = torch.tensor([0.5])
    # a = 1: z alone. x − eta·sign(g) = −0.5, 0.625, 0.25, −0.25, 0, 0 → the ball [−0.25, 0.25]
    got, old = apgd_ref.update(x, x_old, x0, g, eta, 1.0, 0.25)
    assert got.tolist() == [[-0.25, 0.25, 0.25, -0.25, 0.0, 0.0]] and torch.equal(old, x)
    # a = 0.75: x + 0.75·(z − x) + 0.25·(x − x_old)
    #   0 + 0.75·(−0.25) + 0 = −0.1875;  0.125 + 0.75·0.125 + 0.25·0.125 = 0.25;
    #   −0.25 + 0.75·0.5 + 0 = 0.125;  0.25 + 0.75·(−0.5) + 0.25·0.125 = −0.09375;
    #   0 + 0 + 0.25·(−0.125) = −0.03125;  0
    got, _ = apgd_ref.update(x, x_old, x0, g, eta, 0.75, 0.25)
    assert got.tolist() == [[-0.1875, 0.25, 0.125, -0.09375, -0.03125, 0.0]]
    # the range clamp: x0 = 0.9, e = 0.25 → the upper face is 1, not 1.15
    got, _ = apgd_ref.update(torch.tensor([[0.9]]), torch.tensor([[0.9]]), torch.tensor([[0.9]]),
                             torch.tensor([[-1.0]]), eta, 1.0, 0.25)
    assert got.tolist() == [[1.0]]


# ---- attack(): every rejection happens before any device work ------------------------------------
def test_apgd_validation_before_any_device_work():
    from gfa_amd import attack, fgsm
    x = torch.zeros(2, 3, 32, 32)
    t = torch.zeros(1, 3, 32, 32)
    net = _StubNet()
    kw = dict(target=t)
    for extra, word in ((dict(momentum=1.0), "momentum"), (dict(momentum=0.0), "momentum"),
                        (dict(momentum=1.0, nesterov=True), "nesterov"),
                        (dict(nesterov=True), "nesterov"), (dict(ti_kernel=15), "ti_kernel"),
                        (dict(di_prob=0.5), "di_prob"),
                        (dict(di_schedule=torch.tensor([[32, 0, 0, 0]] * 2)), "di_schedule"),
                        (dict(si_scales=5), "si_scales"), (dict(si_scales=1), "si_scales"),
                        (dict(vt_samples=5), "vt_samples")):
        with pytest.raises(ValueError, match="apgd.*does not combine.*" + word):
            attack(net, x, 8 / 255, 4, apgd=True, **extra, **kw)
    with pytest.raises(ValueError, match="L2 form is not implemented"):
        attack(net, x, 1.0, 4, norm="l2", apgd=True, alpha=0.2, **kw)
    for norm in ("adam", "l2_cw"):
        with pytest.raises(ValueError, match="apgd.*norm='linf' only"):
            attack(net, x, None, 4, norm=norm, apgd=True, **kw)
    for bad in (1, 0, "yes", None, 1.0, "False"):
        with pytest.raises(ValueError, match="apgd must be True or False"):
            attack(net, x, 8 / 255, 4, apgd=bad, **kw)
    for bad in (0, -1.0, None):
        with pytest.raises((ValueError, TypeError)):
            attack(net, x, bad, 4, apgd=True, **kw)
    with pytest.raises(ValueError, match="steps"):
        attack(net, x, 8 / 255, -1, apgd=True, **kw)
    with pytest.raises(ValueError, match="fgsm.*apgd"):
        fgsm(net, x, 8 / 255, apgd=True, **kw)
    with pytest.raises(ValueError, match="fgsm.*apgd"):
        fgsm(net, x, 8 / 255, apgd=np.bool_(True), **kw)
    # valid arguments get as far as the network bundle, which a stub is not
    for extra in (dict(apgd=True), dict(apgd=np.bool_(True)), dict(apgd=True, random_start=True),
                  dict(apgd=True, alpha=123.0), dict(apgd=False), dict(apgd=False, momentum=1.0),
                  dict(apgd=np.bool_(False), si_scales=5, ti_kernel=15)):
        with pytest.raises(ValueError, match="device network"):
            attack(net, x, 8 / 255, 4, **extra, **kw)
    with pytest.raises(ValueError, match="device network"):
        attack(net, x, 8 / 255, 0, apgd=True, **kw)
    with pytest.raises(ValueError, match="device network"):
        fgsm(net, x, 8 / 255, apgd=False, **kw)


def test_signatures_constants_and_docs():
    from gfa_amd import attack, fgsm, ops, pgd
    from gfa_amd import dist as gdist
    from gfa_amd.pgd import AttackEngine
    p = inspect.signature(attack).parameters
    assert p["apgd"].default is False and p["apgd"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(p)[-1] == "apgd"             # the existing parameters keep their places
    assert list(inspect.signature(AttackEngine.run_apgd).parameters) == [
        "self", "x0", "t", "steps", "eps", "random_start", "start_noise", "group"]
    assert list(inspect.signature(AttackEngine.step_apgd).parameters) == ["self", "x", "i"]
    assert pgd.APGD_RHO == 0.75 and pgd.APGD_MOMENTUM == 0.75
    assert (ops.APGD_SAVE, ops.APGD_RESTORE) == (apgd_ref.SAVE, apgd_ref.RESTORE) == (1, 2)
    for doc in (attack.__doc__, AttackEngine.run_apgd.__doc__):
        for word in ("Croce & Hein", "loss_steps[-1]", "negative indexing", "x0 − e",
                     "synchronisation"):
            assert word in doc, word
    for word in ("apgd", "L2 form is not implemented", "best_step", "halvings", "step_size",
                 "apgd_schedule"):
        assert word in attack.__doc__, word
    assert "apgd" in fgsm.__doc__
    assert "apgd" in gdist.attack_distributed.__doc__


def test_ops_wrappers_reject_before_the_library_call():
    from gfa_amd import ops
    x, xo, x0, g = (torch.zeros(2, 3, 8, 8) for _ in range(4))
    eta = torch.ones(2)
    up = ops.apgd_update
    for bad in ((x, x, x0, g), (x, xo, x, g), (x, xo, x0, x), (x, xo, xo, g), (x, xo, x0, xo),
                (x, xo[:1], x0, g), (x, xo, x0[:1], g), (x, xo, x0, g[:1]),
                (x.double(), xo, x0, g), (x, xo.double(), x0, g), (x, xo, x0.double(), g),
                (x, xo, x0, g.double()), (None, xo, x0, g), (x, None, x0, g), (x, xo, None, g),
                (x, xo, x0, None)):
        with pytest.raises(ValueError):
            up(*bad, eta, 0.75, 0.1)
    for bad_eta in (torch.ones(3), torch.ones(2).double(), None, torch.ones(2, 1)):
        with pytest.raises(ValueError):
            up(x, xo, x0, g, bad_eta, 0.75, 0.1)
    for a in (0.0, -0.5, 1.5, float("nan"), float("inf"), True, "1", None):
        with pytest.raises(ValueError, match="a must"):
            up(x, xo, x0, g, eta, a, 0.1)
    for e in (0.0, -0.1, float("nan"), float("inf"), True, "1", None):
        with pytest.raises(ValueError, match="e must"):
            up(x, xo, x0, g, eta, 0.75, e)
    with pytest.raises(ValueError, match="lo <= hi"):
        up(x, xo, x0, g, eta, 0.75, 0.1, lo=1.0, hi=-1.0)
    with pytest.raises(ValueError):
        up(x, xo, x0, g, eta, 0.75, 0.1, nonfinite=torch.zeros(2))           # not int32
    with pytest.raises(ValueError, match="device tensor"):
        up(x, xo, x0, g, eta, 1.0, 0.1)

    loss, fs, st = torch.zeros(2), torch.zeros(4, 2), torch.zeros(3, 2, dtype=torch.int32)
    act = torch.zeros(2, dtype=torch.int32)
    hl, he = torch.zeros(5, 2), torch.zeros(5, 2)
    dec = ops.apgd_decide
    for bad in ((None, fs, st, act, hl, he), (loss.double(), fs, st, act, hl, he),
                (torch.zeros(2, 1), fs, st, act, hl, he), (torch.zeros(0), fs, st, act, hl, he),
                (loss, torch.zeros(3, 2), st, act, hl, he), (loss, fs.double(), st, act, hl, he),
                (loss, fs, torch.zeros(3, 2), act, hl, he), (loss, fs, st[:2], act, hl, he),
                (loss, fs, st, act.float(), hl, he), (loss, fs, st, act[:1], hl, he),
                (loss, fs, st, act, torch.zeros(5, 3), he), (loss, fs, st, act, hl, he.double()),
                (loss, fs, st, act, hl[0], he), (loss, fs, st, act, hl, hl),
                (loss, fs, st, act, None, he)):
        with pytest.raises(ValueError):
            dec(*bad, 1)
    ok = (loss, fs, st, act, hl, he)
    for step in (-1, 5, 1.0, True, None):
        with pytest.raises(ValueError):
            dec(*ok, step)
    for thr in (-1, 1.5, True, None):
        with pytest.raises(ValueError, match="thr"):
            dec(*ok, 1, checkpoint=True, thr=thr)
    for ck in (2, "yes", None, 0.5):
        with pytest.raises(ValueError, match="checkpoint"):
            dec(*ok, 1, checkpoint=ck)
    with pytest.raises(ValueError, match="no checkpoint"):
        dec(*ok, 0, checkpoint=True, eta0=0.1)
    for eta0 in (None, 0.0, -1.0, float("nan"), float("inf"), True):
        with pytest.raises(ValueError, match="eta0"):
            dec(*ok, 0, eta0=eta0)
    with pytest.raises(ValueError, match="device tensor"):
        dec(*ok, 0, eta0=0.1)
    with pytest.raises(ValueError, match="device tensor"):
        dec(*ok, 4, checkpoint=True, thr=3)

    xb, gb = torch.zeros_like(x), torch.zeros_like(x)
    ap = ops.apgd_apply
    for bad in ((x, x, xb, gb), (x, g, x, gb), (x, g, xb, x), (x, g, g, gb), (x, g, xb, g),
                (x, g, xb, xb), (x, g[:1], xb, gb), (x, g, xb[:1], gb), (x, g, xb, gb[:1]),
                (x.double(), g, xb, gb), (x, g.double(), xb, gb), (x, g, xb.double(), gb),
                (x, g, xb, gb.double()), (None, g, xb, gb), (x, None, xb, gb), (x, g, None, gb),
                (x, g, xb, None)):
        with pytest.raises(ValueError):
            ap(*bad, act)
    for bad_act in (act.float(), act[:1], torch.zeros(3, dtype=torch.int32), None):
        with pytest.raises(ValueError):
            ap(x, g, xb, gb, bad_act)
    with pytest.raises(ValueError, match="device tensor"):
        ap(x, g, xb, gb, act)


# ---- C ABI validation (returns before any launch: runs without a GPU) ---------------------------
P = ctypes.c_void_p
MB = 1 << 20


def _expect_einval(lib, name, rc, what):
    msg = lib.mia_last_error_string().decode()
    assert rc == -1, (name, rc, what)            # MIA_EINVAL
    assert name in msg and len(msg) > len(name) + 2, msg


def test_abi_apgd_update_validation():
    from gfa_amd import _lib
    lib = _lib.load()
    # never dereferenced: validation fails first. 2·3·32² floats = 24 KiB per buffer
    b = [P(k * MB) for k in range(1, 6)]
    null = P(None)
    plane = 3 * 32 * 32
    last = 4 * (2 * plane - 1)                   # byte offset of a buffer's last float

    def bad(x=b[0], x_old=b[1], x0=b[2], g=b[3], eta=b[4], N=2, plane=plane, a=0.75, e=0.1,
            lo=-1.0, hi=1.0):
        rc = lib.mia_apgd_update(x, x_old, x0, g, eta, N, plane, a, e, lo, hi, null, null)
        _expect_einval(lib, "mia_apgd_update", rc, (N, plane, a, e, lo, hi))

    for name in ("x", "x_old", "x0", "g", "eta"):
        bad(**{name: null})
    bad(x_old=b[0])                              # x_old is x
    bad(x0=b[0])
    bad(g=b[0])
    bad(x0=b[1])                                 # x0 is x_old
    bad(g=b[1])
    bad(x_old=P(MB + 4))                         # overlapping, shifted by one float
    bad(x_old=P(MB + last))                      # the last float of x
    bad(x=P(2 * MB + 4096))                      # overlapping the other way round
    bad(g=P(MB + last))
    bad(x0=P(2 * MB + last))
    for N in (0, -4, 1 << 16, 70000):
        bad(N=N)
    for pl in (0, -4, 1 << 31, 1 << 40):
        bad(plane=pl)
    for a in (0.0, -0.75, 1.0000001, 2.0, float("nan"), float("inf")):
        bad(a=a)
    for e in (0.0, -0.1, float("nan"), float("inf")):
        bad(e=e)
    bad(lo=1.0, hi=-1.0)
    bad(lo=float("nan"))


def test_abi_apgd_decide_validation():
    from gfa_amd import _lib
    lib = _lib.load()
    b = [P(k * MB) for k in range(1, 7)]
    null = P(None)
    names = ("loss", "fstate", "istate", "action", "hist_loss", "hist_eta")

    def bad(N=64, step=1, checkpoint=0, thr=0, eta0=0.0, **over):
        args = [over.get(n, b[k]) for k, n in enumerate(names)]
        rc = lib.mia_apgd_decide(*args, N, step, checkpoint, thr, eta0, null)
        _expect_einval(lib, "mia_apgd_decide", rc, (N, step, checkpoint, thr, eta0, over))

    for n in names:
        bad(**{n: null})
    for k, n in enumerate(names):                # every pair shares a base address
        for m in names[k + 1:]:
            bad(**{m: b[k]})
    bad(loss=P(2 * MB + 4 * (4 * 64 - 1)))       # loss starts at fstate's last float
    bad(action=P(3 * MB + 4 * (3 * 64 - 1)))     # action starts at istate's last int
    bad(fstate=P(MB - 4 * (4 * 64 - 1)))         # fstate's last float is loss's first
    bad(hist_eta=P(5 * MB + 4 * 63))             # hist_eta starts at hist_loss's last float
    for N in (0, -1, 1 << 16, 70000):
        bad(N=N)
    bad(step=-1)
    bad(thr=-1, checkpoint=1)
    bad(thr=-1)
    for ck in (2, -1):
        bad(checkpoint=ck)
    bad(step=0, checkpoint=1, eta0=0.1)          # the start is no checkpoint
    for eta0 in (0.0, -0.1, float("nan"), float("inf")):
        bad(step=0, eta0=eta0)


def test_abi_apgd_apply_validation():
    from gfa_amd import _lib
    lib = _lib.load()
    b = [P(k * MB) for k in range(1, 6)]
    null = P(None)
    plane = 3 * 32 * 32
    last = 4 * (2 * plane - 1)
    names = ("x", "g", "x_best", "g_best", "action")

    def bad(N=2, plane=plane, **over):
        args = [over.get(n, b[k]) for k, n in enumerate(names)]
        rc = lib.mia_apgd_apply(*args, N, plane, null)
        _expect_einval(lib, "mia_apgd_apply", rc, (N, plane, over))

    for n in names:
        bad(**{n: null})
    for k, n in enumerate(names[:4]):            # every pair of the four images
        for m in names[k + 1:4]:
            bad(**{m: b[k]})
            bad(**{m: P((k + 1) * MB + last)})
            bad(**{n: P(names.index(m) * MB + MB + 4096)})
    for N in (0, -4, 1 << 16, 70000):
        bad(N=N)
    for pl in (0, -4, 1 << 31, 1 << 40):
        bad(plane=pl)
