"""Host side of the patch-wise attack (PI-FGSM; no GPU): the reference's own identities and a
hand-worked window, attack()'s argument validation before any device work, the wrapper's host
checks, the engine's ping-pong and fp32 steps, and the C ABI's validation of mia_pi_update."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import pi_ref
from pi_ref import f32
from test_si_host import _StubNet

E = f32(2 * 8 / 255)


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- the reference --------------------------------------------------------------------------------
def test_window_sum_by_hand():
    """A 3 × 4 plane worked by hand, k = 3 and k = 5 (a window larger than the plane): the centre
    is left out, the padding adds nothing and no value crosses into the next plane."""
    C = torch.tensor([[1.0, 2.0, 4.0, 8.0], [16.0, 32.0, 64.0, 128.0], [256.0, 512.0, 1024.0, 2048.0]])
    two = torch.stack([C, -C]).reshape(1, 2, 3, 4)
    S = pi_ref.window_sum(two, 3)
    want = torch.tensor([[50.0, 117.0, 234.0, 196.0], [803.0, 1879.0, 3758.0, 3148.0],
                         [560.0, 1392.0, 2784.0, 1216.0]])
    assert torch.equal(S[0, 0], want) and torch.equal(S[0, 1], -want)
    total = float(C.sum())
    assert torch.equal(pi_ref.window_sum(two, 7)[0, 0], total - C)       # everything but itself
    S5 = pi_ref.window_sum(two, 5)[0, 0]
    assert S5[1, 1] == total - 32.0                                      # reaches the whole plane
    assert S5[1, 0] == total - 16.0 - (8.0 + 128.0 + 2048.0)             # column 3 is out of reach
    assert S5[0, 0] == total - 1.0 - (8.0 + 128.0 + 2048.0)
    for k in (3, 5, 7):                                                   # exact sums: any order
        assert torch.equal(pi_ref.window_sum(two, k, reverse=True), pi_ref.window_sum(two, k))


def test_order_case_depends_on_the_order():
    """The crafted plane: the contract order and the reversed one disagree in the sign of S, at
    the six planted pixels at least, with overflow magnitudes 2^24 apart and both signs."""
    inp, c = pi_ref.order_case()
    fwd = pi_ref.parts(inp["g"], inp["l1"], inp["m"], inp["A"], c["mu"], c["ab"], c["e"], c["k"])
    rev = pi_ref.parts(inp["g"], inp["l1"], inp["m"], inp["A"], c["mu"], c["ab"], c["e"], c["k"],
                       reverse=True)
    assert torch.equal(fwd["C"], rev["C"])
    mag = fwd["C"].abs()
    assert mag.max() == 2.0 ** 20 and mag[mag > 0].min() <= 2.0 ** -4
    assert (fwd["C"] > 0).any() and (fwd["C"] < 0).any() and (fwd["C"] == 0).any()
    differ = pi_ref.sign(fwd["S"]) != pi_ref.sign(rev["S"])
    for y in (5, 10, 15):
        for x in (8, 16):
            assert fwd["S"][0, 0, y, x] == 0 and rev["S"][0, 0, y, x] == 2.0 ** -4
            assert differ[0, 0, y, x]
    assert int(differ.sum()) >= 6


def test_reference_identities():
    """pi_project = 0 gives the MI reference's x and m with a = ab; β = 1 inside the ball
    (steps·a ≤ e) gives the MI reference, over three chained steps and μ ∈ {0, 1}."""
    a = f32(2 * 2 / 255)
    for mu in (0.0, 1.0):
        for beta, gamma in ((10.0, 0.0), (1.0, 1.0)):
            _, ab, gm = pi_ref.steps(2 / 255, beta, gamma)
            assert (gm == 0.0) == (gamma == 0.0) and (ab == a) == (beta == 1.0)
            c = pi_ref.case(9, 11, seed=3)
            x, m, A = c["x0"].clone(), torch.zeros_like(c["m"]), torch.zeros_like(c["A"])
            xm, mm = x.clone(), m.clone()
            for step in range(3):
                g = pi_ref.seeded(7200 + step, x.shape) * torch.tensor(pi_ref.IMG_SCALES).reshape(3, 1, 1, 1)
                l1 = pi_ref.l1_of(g)
                x, m, A, nf = pi_ref.update(x, c["x0"], g, l1, m, A, mu, ab, gm, E, 3)
                xm, mm = pi_ref.mi_update(xm, c["x0"], g, l1, mm, mu, ab, E)
                assert torch.equal(bits(x), bits(xm)) and torch.equal(bits(m), bits(mm)), (mu, beta, step)
                assert not nf.any()
            if beta == 1.0:
                assert (A.abs() <= E).all() and (A.abs() > 0).any()
            else:
                assert (A.abs() > E).any()
    # and the projection does act: γ = 1 at β = 10 moves x off the MI iterate
    c = pi_ref.case(9, 11, seed=3)
    _, ab, gm = pi_ref.steps(2 / 255, 10.0, 1.0)
    xp, _, _, _ = pi_ref.update(c["x"], c["x0"], c["g"], c["l1"], c["m"], c["A"], 1.0, ab, gm, E, 3)
    xq, _ = pi_ref.mi_update(c["x"], c["x0"], c["g"], c["l1"], c["m"], 1.0, ab, E)
    assert not torch.equal(xp, xq)
    assert ((xp - c["x0"]).abs() <= E).all() and xp.min() >= -1 and xp.max() <= 1


def test_reference_flags_nonfinite_and_keeps_inputs():
    c = pi_ref.case(6, 5, seed=4)
    keep = {k: v.clone() for k, v in c.items()}
    g = c["g"].clone()
    g[1, 2, 3, 4] = float("inf")
    l1 = c["l1"].clone()
    l1[2] = 0.0                                                       # 0/0 and x/0
    _, ab, gm = pi_ref.steps(2 / 255, 10.0)
    x, m, A, nf = pi_ref.update(c["x"], c["x0"], g, l1, c["m"], c["A"], 1.0, ab, gm, E, 5)
    assert nf.tolist() == [0, 1, 1]
    assert torch.isfinite(A).all() and torch.isfinite(x).all()        # s ∈ {−1, 0, 1}: A stays finite
    for k, v in keep.items():
        assert torch.equal(bits(c[k]), bits(v)), k


def test_pi_steps_are_fp32():
    from gfa_amd import pgd
    for alpha, beta, gamma in ((2 / 255, 10.0, 1.0), (0.01, 2.5, 0.3), (1 / 3, 7, 0)):
        ab, gm = pgd.pi_steps(alpha, beta, gamma)
        a = np.float32(2.0 * alpha)
        assert ab == float(np.float32(beta) * a) and gm == float(np.float32(gamma) * np.float32(ab))
        assert (ab, gm) == pi_ref.steps(alpha, beta, gamma)[1:]
    assert pgd.pi_steps(np.float32(0.5), np.float64(2), np.int64(1)) == (2.0, 2.0)
    for bad in (0, -1.0, float("nan"), float("inf"), True, "10", None, [10.0]):
        with pytest.raises(ValueError, match="pi_amplification"):
            pgd.pi_steps(0.01, bad)
    for bad in (-0.5, float("nan"), float("inf"), True, "1", None):
        with pytest.raises(ValueError, match="pi_project"):
            pgd.pi_steps(0.01, 10.0, bad)
    with pytest.raises(ValueError, match="pi_amplification.*finite"):
        pgd.pi_steps(1.0, 3e38)                                      # β·a overflows fp32
    with pytest.raises(ValueError, match="pi_amplification"):
        pgd.pi_steps(1e-30, 1e-30)                                    # β·a underflows to 0
    with pytest.raises(ValueError, match="pi_project.*finite"):
        pgd.pi_steps(1.0, 1e30, 1e30)
    assert pgd.PI_MAX_KERNEL == 15 and pgd.PiStep._fields == ("ab", "gm", "kernel")


# ---- attack(): every rejection happens before any device work ------------------------------------
def test_pi_validation_before_any_device_work():
    from gfa_amd import attack, fgsm
    x = torch.zeros(2, 3, 32, 32)
    t = torch.zeros(1, 3, 32, 32)
    net = _StubNet()
    kw = dict(target=t)
    for bad in (0, 0.0, -10.0, float("nan"), float("inf"), True, np.bool_(True), "10", [10.0]):
        with pytest.raises(ValueError, match="pi_amplification must be"):
            attack(net, x, 8 / 255, 4, pi_amplification=bad, **kw)
    for bad in (1, 2, 4, 16, 17, -3, 0, 3.0, 5.5, True, None, "3", (3,)):
        with pytest.raises(ValueError, match="pi_kernel must be an odd integer in 3"):
            attack(net, x, 8 / 255, 4, pi_amplification=10.0, pi_kernel=bad, **kw)
        with pytest.raises(ValueError, match="pi_kernel"):
            attack(net, x, 8 / 255, 4, pi_kernel=bad, **kw)
    for bad in (-1.0, -1e-9, float("nan"), float("inf"), -float("inf"), True, None, "1", [1.0]):
        with pytest.raises(ValueError, match="pi_project must be a finite number >= 0"):
            attack(net, x, 8 / 255, 4, pi_amplification=10.0, pi_project=bad, **kw)
        with pytest.raises(ValueError, match="pi_project"):
            attack(net, x, 8 / 255, 4, pi_project=bad, **kw)
    # pi_kernel / pi_project without pi_amplification
    for extra in (dict(pi_kernel=5), dict(pi_kernel=15), dict(pi_project=0.5), dict(pi_project=0),
                  dict(pi_kernel=7, pi_project=2.0), dict(pi_kernel=5, pi_amplification=None),
                  dict(pi_kernel=5, momentum=1.0, ti_kernel=5)):
        with pytest.raises(ValueError, match="need pi_amplification"):
            attack(net, x, 8 / 255, 4, **extra, **kw)
    # L∞ only
    with pytest.raises(ValueError, match="pi_amplification.*norm='linf' only"):
        attack(net, x, 1.0, 4, norm="l2", alpha=0.2, pi_amplification=10.0, **kw)
    for norm in ("adam", "l2_cw"):
        with pytest.raises(ValueError, match="pi_amplification.*norm='linf' only"):
            attack(net, x, None, 4, norm=norm, pi_amplification=10.0, **kw)
    # the other attacks' own lists name it, whichever other keywords come along
    for other, word in ((dict(apgd=True), "apgd"), (dict(universal=True), "universal"),
                        (dict(sign_hunter=True), "sign_hunter"),
                        (dict(spsa_samples=4), "spsa_samples")):
        for more in (dict(), dict(pi_kernel=5, pi_project=0.5)):
            with pytest.raises(ValueError, match=word + ".*does not combine with.*pi_amplification"):
                attack(net, x, 8 / 255, 4, pi_amplification=10.0, **other, **more, **kw)
        with pytest.raises(ValueError, match="device network"):      # and alone they still pass
            attack(net, x, 8 / 255, 4, **other, **kw)
    with pytest.raises(ValueError, match="spsa_samples.*does not combine with.*pi_amplification"):
        attack(net, x, 1.0, 4, norm="l2", alpha=0.2, spsa_samples=4, pi_amplification=10.0, **kw)
    # the fp32 steps must be usable numbers
    with pytest.raises(ValueError, match="pi_amplification"):
        attack(net, x, 8 / 255, 4, alpha=1.0, pi_amplification=3e38, **kw)
    with pytest.raises(ValueError, match="pi_project"):
        attack(net, x, 8 / 255, 4, alpha=1.0, pi_amplification=1e30, pi_project=1e30, **kw)
    with pytest.raises(ValueError, match="eps > 0 and alpha > 0"):
        attack(net, x, 8 / 255, 4, alpha=0.0, pi_amplification=10.0, **kw)
    with pytest.raises(ValueError, match="steps"):
        attack(net, x, 8 / 255, -1, pi_amplification=10.0, **kw)
    # valid arguments get as far as the network bundle, which a stub is not
    sched = torch.tensor([[30, 1, 1, 1]] * 4)
    for extra in (dict(pi_amplification=10.0), dict(pi_amplification=10), dict(pi_amplification=0.5),
                  dict(pi_amplification=np.float32(2.5), pi_kernel=np.int64(15), pi_project=np.float64(0)),
                  dict(pi_amplification=10.0, pi_kernel=3, pi_project=1.0),
                  dict(pi_amplification=10.0, momentum=1.0), dict(pi_amplification=10.0, momentum=0.0),
                  dict(pi_amplification=10.0, momentum=1.0, nesterov=True),
                  dict(pi_amplification=10.0, ti_kernel=5, di_prob=0.5, momentum=1.0),
                  dict(pi_amplification=10.0, di_schedule=sched), dict(pi_amplification=10.0, si_scales=3),
                  dict(pi_amplification=10.0, vt_samples=2), dict(pi_amplification=10.0, random_start=True),
                  dict(pi_amplification=None), dict(pi_amplification=None, pi_kernel=3, pi_project=1.0),
                  dict(pi_amplification=None, momentum=1.0, ti_kernel=5)):
        with pytest.raises(ValueError, match="device network"):
            attack(net, x, 8 / 255, 4, **extra, **kw)
    with pytest.raises(ValueError, match="device network"):
        fgsm(net, x, 8 / 255, pi_amplification=10.0, **kw)
    with pytest.raises(ValueError, match="pi_kernel"):
        fgsm(net, x, 8 / 255, pi_amplification=10.0, pi_kernel=4, **kw)


def test_signatures_and_docs():
    from gfa_amd import attack, fgsm, ops, pgd
    from gfa_amd import dist as gdist
    from gfa_amd.pgd import AttackEngine
    p = inspect.signature(attack).parameters
    assert p["pi_amplification"].default is None and p["pi_kernel"].default == 3
    assert p["pi_project"].default == 1.0
    for name in ("pi_amplification", "pi_kernel", "pi_project"):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(AttackEngine.step_pi).parameters) == [
        "self", "x", "m", "A", "momentum", "e", "pi", "ti_taps", "di", "nesterov", "si_scales", "vt"]
    q = list(inspect.signature(AttackEngine.run_pi).parameters)
    assert q[:9] == ["self", "x0", "t", "steps", "eps", "alpha", "pi_amplification", "pi_kernel",
                     "pi_project"]
    assert q[9:] == list(inspect.signature(AttackEngine.run_mi).parameters)[6:]
    assert list(inspect.signature(ops.pi_update).parameters) == [
        "x", "x0", "g", "l1", "m_in", "m_out", "A_in", "A_out", "mu", "ab", "gm", "e", "kernel", "lo",
        "hi", "nonfinite"]
    for doc in (attack.__doc__, AttackEngine.run_pi.__doc__):
        for word in ("Gao", "Patch-wise", "ECCV", "overflows", "neighbours", "fixed order"):
            assert word in doc, word
    for word in ("pi_amplification", "pi_kernel", "pi_project", "10000", "DI-TI-PI-FGSM",
                 "does not combine with apgd, universal, sign_hunter or spsa_samples"):
        assert word in attack.__doc__, word
    assert "pi_amplification" in fgsm.__doc__
    for word in ("pi_amplification", "world size"):
        assert word in gdist.attack_distributed.__doc__, word
    assert "ping-pong" in AttackEngine.run_pi.__doc__ and "pairs" in AttackEngine.step_pi.__doc__.lower()


# ---- the engine's ping-pong on recorded launches ---------------------------------------------------
def test_run_pi_swaps_the_state_and_restarts_from_zero(monkeypatch):
    """_run_mi with ``pi``: step k reads buffer k % 2 of (mi.m, mi.m1) and (pi.a0, pi.a1) and
    writes the other; mi.m and pi.a0 are zeroed before the first step; nothing is copied back."""
    from gfa_amd import ops, pgd
    from test_step_trace_host import _Recorder, N, S
    r = _Recorder(monkeypatch)
    eng = r.eng
    monkeypatch.setattr(eng, "_start", lambda x0, t, e, rs, noise: r.x)
    x0 = torch.zeros(N, 3, S, S)
    _, ab, gm = pi_ref.steps(2 / 255, 10.0, 0.5)
    eng._run_mi(x0, x0, 3, 8 / 255, 2 / 255, 1.0, False, None, pi=pgd.PiStep(ab, gm, 5))
    calls = [l for l in r.trace if l[0] == "mia_pi_update"]
    assert len(calls) == 3 and not any(l[0] == "mia_mi_update" for l in r.trace)
    # arguments: kernel, x, x0, g, l1, m_in, m_out, A_in, A_out, N, C, H, W, K, mu, ab, gm, e, …
    assert [c[5:9] for c in calls] == [["mi.m", "mi.m1", "pi.a0", "pi.a1"],
                                       ["mi.m1", "mi.m", "pi.a1", "pi.a0"],
                                       ["mi.m", "mi.m1", "pi.a0", "pi.a1"]]
    for c in calls:
        assert c[1:5] == ["adv", "x0", "g.full", "norm.sums"]
        assert c[9:14] == [N, 3, S, S, 5]
        assert c[14:18] == [1.0, ab, gm, f32(2 * 8 / 255)] and c[18:20] == [-1.0, 1.0]
        assert c[20] == "nonfinite"
    first = r.trace.index(calls[0])
    zeroed = [l[1] for l in r.trace[:first] if l[0] == "mia_memset"]
    assert "mi.m" in zeroed and "pi.a0" in zeroed
    assert not any(l[0] == "copy_" and l[1] in ("mi.m", "mi.m1", "pi.a0", "pi.a1") for l in r.trace)
    assert ops.PI_MAX_KERNEL == 15


# ---- the wrapper's host checks ----------------------------------------------------------------------
def test_ops_wrapper_rejects_before_the_library_call():
    from gfa_amd import ops
    names = ("x", "x0", "g", "m_in", "m_out", "A_in", "A_out")
    good = {n: torch.zeros(2, 3, 8, 8) for n in names}
    l1 = torch.ones(2)

    def call(l1=l1, mu=1.0, ab=0.1, gm=0.1, e=0.05, kernel=3, nonfinite=None, lo=-1.0, hi=1.0, **over):
        b = {**good, **over}
        return ops.pi_update(b["x"], b["x0"], b["g"], l1, b["m_in"], b["m_out"], b["A_in"], b["A_out"],
                             mu, ab, gm, e, kernel, lo, hi, nonfinite)

    for n in names:
        for bad in (None, torch.zeros(2, 3, 8, 9), torch.zeros(1, 3, 8, 8), torch.zeros(2, 3, 8, 8).double(),
                    torch.zeros(2, 192)):
            with pytest.raises(ValueError):
                call(**{n: bad})
    with pytest.raises(ValueError):
        call(x=torch.zeros(0, 3, 8, 8))
    for k, a in enumerate(names):                 # every pair shares a buffer: m and A in place too
        for b in names[k + 1:]:
            with pytest.raises(ValueError, match="distinct"):
                call(**{b: good[a]})
    for bad in (None, torch.ones(3), torch.ones(2).double(), torch.ones(2, 1)):
        with pytest.raises(ValueError):
            call(l1=bad)
    for bad in (1, 2, 4, 17, 3.0, True, None, "3"):
        with pytest.raises(ValueError, match="kernel must be an odd integer"):
            call(kernel=bad)
    for nm in ("mu", "ab", "gm", "e"):
        for bad in (-0.1, float("nan"), float("inf"), True, "1", None):
            with pytest.raises(ValueError, match=nm + " must be"):
                call(**{nm: bad})
    with pytest.raises(ValueError, match="lo <= hi"):
        call(lo=1.0, hi=-1.0)
    with pytest.raises(ValueError):
        call(nonfinite=torch.zeros(2))                               # not int32
    with pytest.raises(ValueError):
        call(nonfinite=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="device tensor"):
        call()
    with pytest.raises(ValueError, match="device tensor"):
        call(kernel=15, mu=0.0, gm=0.0, nonfinite=torch.zeros(2, dtype=torch.int32))


# ---- C ABI validation (returns before any launch: runs without a GPU) ---------------------------
P = ctypes.c_void_p
MB = 1 << 20


def test_abi_pi_update_validation():
    from gfa_amd import _lib
    lib = _lib.load()
    # never dereferenced: validation fails first. 2·3·32² floats = 24 KiB per buffer
    names = ("x", "x0", "g", "l1", "m_in", "m_out", "A_in", "A_out")
    base = {n: P((k + 1) * MB) for k, n in enumerate(names)}
    null = P(None)
    last = 4 * (2 * 3 * 32 * 32 - 1)             # byte offset of a buffer's last float

    def bad(N=2, C=3, H=32, W=32, K=3, mu=1.0, ab=0.1, gm=0.1, e=0.05, lo=-1.0, hi=1.0,
            nonfinite=null, **over):
        b = {**base, **over}
        rc = lib.mia_pi_update(*[b[n] for n in names], N, C, H, W, K, mu, ab, gm, e, lo, hi,
                               nonfinite, null)
        msg = lib.mia_last_error_string().decode()
        assert rc == -1, (rc, over, N, C, H, W, K, mu, ab, gm, e, lo, hi)   # MIA_EINVAL
        assert "mia_pi_update" in msg and len(msg) > len("mia_pi_update") + 2, msg
        return msg

    for n in names:
        bad(**{n: null})
    for K in (1, 2, 4, 16, 17, 63, 0, -3):
        assert "K must be odd" in bad(K=K)
    for v in (-0.5, float("nan"), float("inf"), -float("inf")):
        bad(ab=v)
        bad(gm=v)
        bad(e=v)
        assert "mu" in bad(mu=v)
    bad(lo=1.0, hi=-1.0)
    bad(lo=float("nan"))
    bad(hi=float("nan"))
    for N in (0, -4, 1 << 16, 70000):
        bad(N=N)
    for dims in (dict(C=0), dict(H=0), dict(W=0), dict(C=-3), dict(H=-1), dict(W=-8),
                 dict(H=1 << 16, W=1 << 15), dict(C=2, H=1 << 15, W=1 << 15),
                 dict(C=1 << 30, H=4, W=4)):
        bad(**dims)
    # the ping-pong: in place is rejected, and so is any overlap with a written buffer
    assert "m_in and m_out" in bad(m_out=base["m_in"])
    assert "A_in and A_out" in bad(A_out=base["A_in"])
    bad(m_out=P(5 * MB + 4))                     # shifted by one float
    bad(m_out=P(5 * MB + last))                  # m_out starts at m_in's last float
    bad(m_in=P(6 * MB + last))
    bad(A_out=P(7 * MB + last))
    bad(A_in=P(8 * MB + 4096))
    writes, reads = ("x", "m_out", "A_out"), ("x0", "g", "m_in", "A_in")
    for w in writes:
        for r in reads + tuple(o for o in writes if o != w):
            assert "distinct" in bad(**{r: base[w]})
            bad(**{r: P(base[w].value + last)})
        bad(l1=P(base[w].value + 64))            # l1 inside a written buffer
        bad(l1=P(base[w].value - 4))             # l1's second float is the buffer's first
