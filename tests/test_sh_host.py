"""Host side of SignHunter (no GPU): the segment schedule against hand-worked rows, the control
reference on scripted objective sequences against states written out by hand, the whole reference
loop on a linear objective whose optimum is known, attack()'s and fgsm()'s argument validation
before any device work, the wrappers' host checks, and the C ABI's validation of mia_sh_flip /
mia_sh_decide."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import sh_ref
from test_si_host import _StubNet


# ---- the schedule ---------------------------------------------------------------------------------
def test_schedule_hand_worked_rows():
    from gfa_amd import sh_schedule as exported
    from gfa_amd.pgd import sh_schedule
    assert exported is sh_schedule
    # plane = 3: lengths 3, ceil(3/2) = 2, ceil(3/4) = 1, then the wrap to the whole plane
    want3 = [(0, 3), (0, 2), (2, 3), (0, 1), (1, 2), (2, 3), (0, 3), (0, 2)]
    for fn in (sh_schedule, sh_ref.schedule):
        assert fn(8, 3) == want3
        assert fn(3, 3) == want3[:3] and fn(0, 3) == []
        assert fn(3, 1) == [(0, 1)] * 3                     # one element: every level is len 1
        assert fn(4, 2) == [(0, 2), (0, 1), (1, 2), (0, 2)]
        # plane = 192: 192, 96, 48, 24, 12, 6, 3, 2, 1 → 1+2+4+8+16+32+64+96+192 = 415 rows
        rows = fn(416, 192)
        assert rows[415] == (0, 192) and rows[414] == (191, 192) and rows[:3] == [
            (0, 192), (0, 96), (96, 192)]
        # levels 0 … 6 hold 1+2+4+8+16+32+64 = 127 rows: row 126 is the last of length 3
        assert [hi - lo for lo, hi in rows[126:129]] == [3, 2, 2]
        assert rows[126] == (189, 192) and rows[127] == (0, 2)
        assert rows[222] == (190, 192) and rows[223] == (0, 1)      # + 96 rows of length 2
    # 32²: 31 rows complete the levels 0 … 4 (chunks of 3072 … 192)
    rows = sh_schedule(32, 3072)
    assert rows[30] == (2880, 3072) and rows[31] == (0, 96)
    assert sh_schedule(np.int64(5), np.int64(192)) == sh_ref.schedule(5, 192)
    for bad in ((-1, 3), (1.5, 3), (True, 3), (None, 3), ("3", 3), (3, 0), (3, -1), (3, 1 << 31),
                (3, 2.0), (3, True), (3, None)):
        with pytest.raises(ValueError):
            sh_schedule(*bad)
    assert len(sh_schedule(5, (1 << 31) - 1)) == 5


def levels(rows):
    """Split a schedule into its levels: a new level starts where lo returns to 0."""
    out = []
    for r in rows:
        if r[0] == 0:
            out.append([])
        out[-1].append(r)
    return out


def test_schedule_levels_tile_the_plane():
    from gfa_amd.pgd import sh_schedule
    for plane in list(range(1, 301)) + [3267]:
        # one full cycle: Σ over the levels of ceil(plane / len)
        n, h = 0, 0
        while True:
            ln = -(-plane // 2 ** h)
            n += -(-plane // ln)
            if ln == 1:
                break
            h += 1
        rows = sh_schedule(n + 1, plane)
        assert rows == sh_ref.schedule(n + 1, plane)
        assert rows[n] == (0, plane) and rows[n - 1] == (plane - 1, plane)
        lv = levels(rows[:n])
        assert len(lv) == h + 1
        for i, level in enumerate(lv):
            ln = -(-plane // 2 ** i)
            assert level[0][0] == 0 and level[-1][1] == plane
            assert all(a[1] == b[0] for a, b in zip(level, level[1:]))           # no gap
            assert all(hi - lo == ln for lo, hi in level[:-1]) and 1 <= level[-1][1] - level[-1][0] <= ln
        assert all(hi - lo == 1 for lo, hi in lv[-1]) and len(lv[-1]) == plane
    assert len(sh_schedule(500, 192)) == 500


# ---- the control reference on scripted sequences --------------------------------------------------
NAN = float("nan")
# per script, worked by hand from the rule: the accept flag of each of the six flips, and the end
# state
EXPECT = {
    "fall": dict(accepts=[1, 1, 1, 1, 1, 1], best=4, n_accept=6, nonfinite=0),
    "never": dict(accepts=[0, 0, 0, 0, 0, 0], best=1, n_accept=0, nonfinite=0),
    "tie": dict(accepts=[0, 1, 0, 0, 1, 0], best=3, n_accept=2, nonfinite=0),
    "nan": dict(accepts=[0, 1, 0, 0, 1, 0], best=3, n_accept=2, nonfinite=1),
    "inf": dict(accepts=[0, 1, 0, 0, 1, 0], best=3.5, n_accept=2, nonfinite=1),
    "nan0": dict(accepts=[0, 0, 0, 0, 0, 0], best=NAN, n_accept=0, nonfinite=1),
}


def same(a, b):
    a, b = np.float32(a), np.float32(b)
    return bool(a == b) or bool(np.isnan(a) and np.isnan(b))


@pytest.mark.parametrize("name", list(sh_ref.SCRIPTS))
def test_control_reference_on_scripted_sequences(name):
    seq, exp = sh_ref.SCRIPTS[name], EXPECT[name]
    assert list(sh_ref.SCRIPTS) == list(EXPECT) and len(seq) == 7
    c = sh_ref.Control(seq[0])
    assert same(c.best, seq[0]) and c.accept == 1 and c.n_accept == 0
    acc = [c.step(v) for v in seq[1:]]
    assert acc == exp["accepts"]
    st = c.state()
    assert same(st["best"], exp["best"]) and st["n_accept"] == exp["n_accept"]
    assert st["nonfinite"] == exp["nonfinite"] and st["accept"] == exp["accepts"][-1]
    assert all(same(a, b) for a, b in zip(c.loss, seq)) and len(c.loss) == 7
    # best is the running minimum of the finite values below the start, n_accept its new records
    L = sh_ref.scripted_losses()
    ctl = sh_ref.replay(L)
    for n, key in enumerate(sh_ref.SCRIPTS):
        assert same(ctl[n].best, EXPECT[key]["best"]) and ctl[n].n_accept == EXPECT[key]["n_accept"]


def test_flip_reference_by_hand():
    """e = 0.25 on six elements, two images; x0 reaches the range's ends so the clamp acts."""
    x0 = torch.tensor([[0.0, 0.5, 0.875, -0.875, 1.0, -1.0]] * 2)
    s = torch.full((2, 6), -1, dtype=torch.int8)
    x = torch.full((2, 6), NAN)
    sh_ref.flip(x, x0, s, None, None, (0, 6), 0.25)                   # the start: s = +1
    assert s.tolist() == [[1] * 6] * 2
    assert x.tolist() == [[0.25, 0.75, 1.0, -0.625, 1.0, -0.75]] * 2
    sh_ref.flip(x, x0, s, [1, 1], None, (0, 3), 0.25)                 # query 1: [0, 3)
    assert s.tolist() == [[-1, -1, -1, 1, 1, 1]] * 2
    assert x[0].tolist() == [-0.25, 0.25, 0.625, -0.625, 1.0, -0.75]
    # query 2 flips [3, 6); image 0 rejected query 1 and gets [0, 3) back, image 1 kept it
    sh_ref.flip(x, x0, s, [0, 1], (0, 3), (3, 6), 0.25)
    assert s.tolist() == [[1, 1, 1, -1, -1, -1], [-1, -1, -1, -1, -1, -1]]
    assert x[0].tolist() == [0.25, 0.75, 1.0, -1.0, 0.75, -1.0]
    assert x[1].tolist() == [-0.25, 0.25, 0.625, -1.0, 0.75, -1.0]
    # overlapping ranges (level 0 → level 1): a rejected [0, 6) and a new [0, 3) cancel on [0, 3)
    keep = s.clone()
    sh_ref.flip(x, x0, s, [0, 1], (0, 6), (0, 3), 0.25)
    assert s[0].tolist() == [1, 1, 1, 1, 1, 1] and s[1].tolist() == [1, 1, 1, -1, -1, -1]
    assert keep[0].tolist() == [1, 1, 1, -1, -1, -1]
    # the final revert: an empty new range; elements outside keep their bits (NaN planted)
    x[0, 5] = NAN
    sh_ref.flip(x, x0, s, [0, 0], (1, 2), None, 0.25)
    assert s[0].tolist() == [1, -1, 1, 1, 1, 1] and x[0, 1] == 0.25 and bool(torch.isnan(x[0, 5]))


# ---- the whole loop on a linear objective -----------------------------------------------------------
def test_reference_run_reaches_the_linear_optimum():
    """L(x) = Σ w_j·x_j in fp64 with w_j = σ_j·(1 + j/plane)·scale_n, x0 = 0, e = 0.25, plane = 192:
    after the 415 flips of one cycle s_j = −σ_j for every j. The last level tests every coordinate
    alone, where a flip moves L by 2·e·|w_j| ≥ 0.5·scale against an fp32 rounding of L of about
    4e-6·scale (|L| ≤ 0.25·Σ(1 + j/192)·scale ≈ 72·scale, half an ulp 3.8e-6·scale), so every
    decision of that level is the exact one."""
    x0, e, w, sigma = sh_ref.linear_case()
    out = sh_ref.run(x0, e, 415, sh_ref.linear_objective(w))
    assert out["loss"].shape == (416, 3) and np.isfinite(out["loss"]).all()
    for n in range(3):
        assert torch.equal(out["s"][n].double(), -sigma), n
        assert torch.equal(out["x"][n].double(), -0.25 * sigma)
        c = out["controls"][n]
        assert c.best == out["loss"][:, n].min() and c.n_accept >= 1
    # the best recorded objective is the objective of the returned vertex
    final = sh_ref.linear_objective(w)(out["x"])
    assert [c.best for c in out["controls"]] == final.tolist()
    # rebuild() replays the recorded history to the same point
    x, s, ctl = sh_ref.rebuild(x0, e, out["loss"], sh_ref.schedule(415, 192))
    assert torch.equal(x, out["x"]) and torch.equal(s, out["s"])
    assert [c.n_accept for c in ctl] == [c.n_accept for c in out["controls"]]
    assert torch.equal(sh_ref.run(x0, e, 0, None)["x"], x0)


# ---- attack(): every rejection happens before any device work ------------------------------------
def test_sign_hunter_validation_before_any_device_work():
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
                        (dict(vt_samples=5), "vt_samples"), (dict(spsa_samples=4), "spsa_samples"),
                        (dict(apgd=True), "apgd"), (dict(universal=True), "universal"),
                        (dict(random_start=True), "random_start")):
        with pytest.raises(ValueError, match="sign_hunter does not combine with.*" + word):
            attack(net, x, 8 / 255, 4, sign_hunter=True, **extra, **kw)
    with pytest.raises(ValueError, match="sign_hunter.*norm='linf' only"):
        attack(net, x, 1.0, 4, norm="l2", sign_hunter=True, alpha=0.2, **kw)
    for norm in ("adam", "l2_cw"):
        with pytest.raises(ValueError, match="sign_hunter.*norm='linf' only"):
            attack(net, x, None, 4, norm=norm, sign_hunter=True, **kw)
    for bad in (1, 0, "yes", None, 1.0, "False"):
        with pytest.raises(ValueError, match="sign_hunter must be True or False"):
            attack(net, x, 8 / 255, 4, sign_hunter=bad, **kw)
    for bad in (0, -1.0, None):
        with pytest.raises((ValueError, TypeError)):
            attack(net, x, bad, 4, sign_hunter=True, **kw)
    with pytest.raises(ValueError, match="steps"):
        attack(net, x, 8 / 255, -1, sign_hunter=True, **kw)
    with pytest.raises(ValueError, match="fgsm.*sign_hunter"):
        fgsm(net, x, 8 / 255, sign_hunter=True, **kw)
    with pytest.raises(ValueError, match="fgsm.*sign_hunter"):
        fgsm(net, x, 8 / 255, sign_hunter=np.bool_(True), **kw)
    # valid arguments get as far as the network bundle, which a stub is not; alpha is not used
    for extra in (dict(sign_hunter=True), dict(sign_hunter=np.bool_(True)),
                  dict(sign_hunter=True, alpha=123.0), dict(sign_hunter=True, alpha=0.0),
                  dict(sign_hunter=False), dict(sign_hunter=False, momentum=1.0),
                  dict(sign_hunter=np.bool_(False), si_scales=5, ti_kernel=15),
                  dict(sign_hunter=False, apgd=True), dict(sign_hunter=False, spsa_samples=4),
                  dict(sign_hunter=False, universal=True)):
        with pytest.raises(ValueError, match="device network"):
            attack(net, x, 8 / 255, 4, **extra, **kw)
    with pytest.raises(ValueError, match="device network"):
        attack(net, x, 8 / 255, 0, sign_hunter=True, **kw)
    with pytest.raises(ValueError, match="device network"):
        fgsm(net, x, 8 / 255, sign_hunter=False, **kw)


def test_signatures_and_docs():
    from gfa_amd import attack, fgsm
    from gfa_amd import dist as gdist
    from gfa_amd.pgd import AttackEngine, sh_schedule
    p = inspect.signature(attack).parameters
    assert p["sign_hunter"].default is False
    assert p["sign_hunter"].kind is inspect.Parameter.KEYWORD_ONLY
    names = list(p)
    assert names[-5:] == ["universal", "spsa_samples", "spsa_delta", "spsa_first_image", "apgd"]
    assert names[-7:-5] == ["vt_first_image", "sign_hunter"]
    assert list(inspect.signature(AttackEngine.run_sign_hunter).parameters) == [
        "self", "x0", "t", "steps", "eps", "group"]
    assert list(inspect.signature(AttackEngine.step_sign_hunter).parameters) == ["self", "x", "k"]
    assert list(inspect.signature(AttackEngine.start_sign_hunter).parameters)[:4] == [
        "self", "x0", "t", "eps"]
    assert list(inspect.signature(sh_schedule).parameters) == ["steps", "plane"]
    for doc in (attack.__doc__, AttackEngine.run_sign_hunter.__doc__):
        for word in ("Al-Dujaili", "vertex", "sh_schedule", "steps + 1", "tie"):
            assert word in doc, word
    for word in ("sign_hunter", "accepted", "int8"):
        assert word in attack.__doc__, word
    assert "sign_hunter" in fgsm.__doc__
    assert "sign_hunter" in gdist.attack_distributed.__doc__


def test_ops_wrappers_reject_before_the_library_call():
    from gfa_amd import ops
    x, x0 = torch.zeros(2, 3, 8, 8), torch.zeros(2, 3, 8, 8)
    s = torch.ones(2, 3, 8, 8, dtype=torch.int8)
    acc = torch.ones(2, dtype=torch.int32)
    fl = ops.sh_flip
    for bad in ((x, x, s), (x, x0[:1], s), (x.double(), x0, s), (x, x0.double(), s),
                (x, x0, s.float()), (x, x0, s[:1]), (x, x0, s.reshape(2, -1)), (None, x0, s),
                (x, None, s), (x, x0, None)):
        with pytest.raises(ValueError):
            fl(*bad, acc, None, (0, 192), 0.1)
    for bad_acc in (acc.float(), acc[:1], torch.ones(3, dtype=torch.int32)):
        with pytest.raises(ValueError):
            fl(x, x0, s, bad_acc, None, (0, 192), 0.1)
    for prev, new in ((None, None), ((5, 5), (7, 7)), (None, (0, 193)), (None, (-1, 4)),
                      (None, (5, 4)), ((0, 193), (0, 4)), ((4, 2), (0, 4)), (None, (0.0, 4)),
                      (None, (0, True)), (None, (0, 4, 5)), (None, 4), ((0, "4"), (0, 4))):
        with pytest.raises(ValueError):
            fl(x, x0, s, acc, prev, new, 0.1)
    for e in (0.0, -0.1, float("nan"), float("inf"), True, "1", None):
        with pytest.raises(ValueError, match="e must"):
            fl(x, x0, s, acc, None, (0, 192), e)
    with pytest.raises(ValueError, match="lo <= hi"):
        fl(x, x0, s, acc, None, (0, 192), 0.1, lo=1.0, hi=-1.0)
    with pytest.raises(ValueError, match="device tensor"):
        fl(x, x0, s, acc, (0, 96), (96, 192), 0.1)
    with pytest.raises(ValueError, match="device tensor"):
        fl(x, x0, s, None, (0, 96), None, 0.1)

    loss, best = torch.zeros(2), torch.zeros(2)
    n_acc = torch.zeros(2, dtype=torch.int32)
    hist = torch.zeros(5, 2)
    dec = ops.sh_decide
    for bad in ((None, best, acc, n_acc, hist), (loss.double(), best, acc, n_acc, hist),
                (torch.zeros(2, 1), best, acc, n_acc, hist), (torch.zeros(0), best, acc, n_acc, hist),
                (loss, best.double(), acc, n_acc, hist), (loss, best[:1], acc, n_acc, hist),
                (loss, None, acc, n_acc, hist), (loss, best, acc.float(), n_acc, hist),
                (loss, best, acc[:1], n_acc, hist), (loss, best, None, n_acc, hist),
                (loss, best, acc, n_acc.float(), hist), (loss, best, acc, None, hist),
                (loss, best, acc, acc, hist), (loss, loss, acc, n_acc, hist),
                (loss, best, acc, n_acc, torch.zeros(5, 3)), (loss, best, acc, n_acc, hist.double()),
                (loss, best, acc, n_acc, hist[0]), (loss, best, acc, n_acc, None)):
        with pytest.raises(ValueError):
            dec(*bad, 1)
    ok = (loss, best, acc, n_acc, hist)
    for q in (-1, 5, 1.0, True, None):
        with pytest.raises(ValueError):
            dec(*ok, q)
    with pytest.raises(ValueError):
        dec(*ok, 1, nonfinite=torch.zeros(2))                             # not int32
    with pytest.raises(ValueError, match="device tensor"):
        dec(*ok, 0)
    with pytest.raises(ValueError, match="device tensor"):
        dec(*ok, 4, nonfinite=torch.zeros(2, dtype=torch.int32))


# ---- C ABI validation (returns before any launch: runs without a GPU) ---------------------------
P = ctypes.c_void_p
MB = 1 << 20


def _expect_einval(lib, name, rc, what):
    msg = lib.mia_last_error_string().decode()
    assert rc == -1, (name, rc, what)            # MIA_EINVAL
    assert name in msg and len(msg) > len(name) + 2, msg


def test_abi_sh_flip_validation():
    from gfa_amd import _lib
    lib = _lib.load()
    # never dereferenced: validation fails first. 2·3·32² floats = 24 KiB per fp32 buffer
    b = [P(k * MB) for k in range(1, 5)]
    null = P(None)
    plane = 3 * 32 * 32
    last = 4 * (2 * plane - 1)                   # byte offset of an fp32 buffer's last float

    def bad(x=b[0], x0=b[1], s=b[2], accept=b[3], N=2, plane=plane, prev=(0, 96), new=(96, 192),
            e=0.1, lo=-1.0, hi=1.0):
        rc = lib.mia_sh_flip(x, x0, s, accept, N, plane, prev[0], prev[1], new[0], new[1], e, lo,
                             hi, null)
        _expect_einval(lib, "mia_sh_flip", rc, (N, plane, prev, new, e, lo, hi))

    for name in ("x", "x0", "s"):
        bad(**{name: null})
        bad(**{name: null}, accept=null)
    bad(x0=b[0])                                 # x0 is x
    bad(s=b[0])
    bad(s=b[1])
    bad(x0=P(MB + 4))                            # overlapping, shifted by one float
    bad(x0=P(MB + last))                         # the last float of x
    bad(x=P(2 * MB + 4096))                      # the other way round
    bad(s=P(MB + last + 3))                      # s starts at x's last byte
    bad(x0=P(3 * MB + 2 * plane - 1))            # x0 starts at s's last byte
    bad(accept=P(MB + last))                     # accept inside x
    bad(accept=P(3 * MB + 2 * plane - 1))        # accept inside s
    bad(s=P(4 * MB + 7))                         # s inside accept
    for N in (0, -4, 1 << 16, 70000):
        bad(N=N)
    for pl in (0, -4, 1 << 31, 1 << 40):
        bad(plane=pl)
    for r in ((-1, 4), (5, 4), (0, plane + 1), (plane + 1, plane + 2), (-4, -2)):
        bad(prev=r)
        bad(new=r)
    bad(prev=(0, 0), new=(0, 0))                 # both empty
    bad(prev=(7, 7), new=(plane, plane))
    bad(prev=(7, 7), new=(9, 9), accept=null)
    for e in (0.0, -0.1, float("nan"), float("inf")):
        bad(e=e)
    bad(lo=1.0, hi=-1.0)
    bad(lo=float("nan"))
    bad(hi=float("nan"))


def test_abi_sh_decide_validation():
    from gfa_amd import _lib
    lib = _lib.load()
    b = [P(k * MB) for k in range(1, 7)]
    null = P(None)
    names = ("loss", "best", "accept", "n_accept", "hist_loss", "nonfinite")

    def bad(N=64, first=0, **over):
        args = [over.get(n, b[k]) for k, n in enumerate(names)]
        rc = lib.mia_sh_decide(*args[:5], N, first, args[5], null)
        _expect_einval(lib, "mia_sh_decide", rc, (N, first, over))

    for n in names[:5]:
        bad(**{n: null})
        bad(**{n: null}, nonfinite=null)
    for k, n in enumerate(names):                # every pair shares a base address
        for m in names[k + 1:]:
            bad(**{m: b[k]})
    bad(best=P(MB + 4 * 63))                     # best starts at loss's last float
    bad(loss=P(2 * MB + 4 * 63))
    bad(n_accept=P(3 * MB + 4 * 63))
    bad(nonfinite=P(5 * MB + 4 * 63))
    bad(hist_loss=P(MB - 4 * 63))                # hist_loss's last float is loss's first
    for N in (0, -1, 1 << 16, 70000):
        bad(N=N)
    for first in (2, -1):
        bad(first=first)
