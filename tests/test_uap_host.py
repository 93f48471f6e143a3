"""Host side of the universal perturbation (no GPU): the reference (tests/uap_ref.py), attack()'s
argument validation before any device work, the range bound of the integer sum, the wrappers' host
checks, the C ABI's validation of mia_uap_accumulate / mia_uap_step, the docstrings, and the
collectives an empty-shard rank joins (pgd.idle_rank_universal against a fake group)."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import uap_ref
from test_si_host import _StubNet


# ---- the reference --------------------------------------------------------------------------------
def test_reference_ties_zeros_and_flags():
    """round-half-even on exact .5 ties, zeros, and an image with an Inf element: its flag, a zero
    term for that element, the other images untouched; the sum is order-free."""
    plane = 16
    g = torch.zeros(3, 1, 4, 4)
    l1 = torch.full((3,), float(plane))                     # mean 1: ĝ = −g
    g[0, 0, 0, :4] = torch.tensor([-(2.0 + 0.5) / 2 ** 24, -(3.0 + 0.5) / 2 ** 24,
                                   (2.0 + 0.5) / 2 ** 24, 0.0])
    g[1, 0, 0, :2] = torch.tensor([-1.0, 3.0])
    g[2, 0, 0, 0], g[2, 0, 0, 1] = float("inf"), -2.0
    q, bad = uap_ref.terms(g, l1)
    assert q.dtype == torch.int64 and bad.tolist() == [False, False, True]
    assert q[0, 0, 0, :4].tolist() == [2, 4, -2, 0]        # 2.5 → 2, 3.5 → 4, −2.5 → −2
    assert q[1, 0, 0, :2].tolist() == [2 ** 24, -3 * 2 ** 24]
    assert q[2, 0, 0, :2].tolist() == [0, 2 ** 25]
    acc, bad2 = uap_ref.accumulate(g, l1)
    assert torch.equal(bad, bad2) and acc.shape == (plane,)
    perm = torch.tensor([2, 0, 1])
    assert torch.equal(uap_ref.accumulate(g[perm], l1[perm])[0], acc)
    two = uap_ref.accumulate(g[2:], l1[2:], uap_ref.accumulate(g[:2], l1[:2])[0])[0]
    assert torch.equal(two, acc)
    # an all-zero gradient: 0/0 everywhere, flagged, contributes nothing
    z, badz = uap_ref.accumulate(torch.zeros(1, 1, 4, 4), torch.zeros(1))
    assert badz.tolist() == [True] and not z.any()


def test_reference_step():
    e, a = float(np.float32(16 / 255)), float(np.float32(4 / 255))
    delta = torch.tensor([0.0, e, -e, e, -e, 0.01]).reshape(1, 1, 2, 3)
    acc = torch.tensor([5, 7, -7, -1, 1, 0])
    x0 = torch.tensor([[0.99, -0.99, 0.0, 0.5, -0.5, 1.0]]).reshape(1, 1, 2, 3)
    d, x = uap_ref.step(delta, acc, x0, a, e)
    want = [a, e, -e, float(np.float32(e) - np.float32(a)), float(np.float32(a) - np.float32(e)),
            float(np.float32(0.01))]
    assert d.flatten().tolist() == want and d.abs().max() <= e
    assert torch.equal(x, torch.clamp(x0 + d, -1, 1)) and x.abs().max() <= 1
    d2, x2 = uap_ref.step(delta, None, x0, a, e)
    assert d2 is delta and torch.equal(x2, torch.clamp(x0 + delta, -1, 1))
    d3, x3 = uap_ref.step(delta, acc, None, a, e)
    assert torch.equal(d3, d) and x3 is None


# ---- attack(): every rejection happens before any device work ------------------------------------
def test_universal_validation_before_any_device_work():
    from gfa_amd import attack, fgsm
    x = torch.zeros(2, 3, 32, 32)
    t = torch.zeros(1, 3, 32, 32)
    net = _StubNet()
    kw = dict(target=t, alpha=2 / 255)
    for bad in (1, 0, "yes", None, 1.0, [True]):
        with pytest.raises(ValueError, match="universal must be"):
            attack(net, x, 8 / 255, 2, universal=bad, **kw)
    for norm in ("l2", "adam", "l2_cw"):
        with pytest.raises(ValueError, match="universal.*linf"):
            attack(net, x, 8 / 255, 2, universal=True, norm=norm, **kw)
    sched = np.array([[32, 0, 0, 0], [32, 0, 0, 0]])
    for name, extra in (("momentum", dict(momentum=1.0)), ("momentum", dict(momentum=0.0)),
                        ("nesterov", dict(nesterov=True)), ("ti_kernel", dict(ti_kernel=15)),
                        ("di_prob", dict(di_prob=0.5)), ("di_schedule", dict(di_schedule=sched)),
                        ("si_scales", dict(si_scales=2)), ("si_scales", dict(si_scales=1)),
                        ("vt_samples", dict(vt_samples=3)), ("spsa_samples", dict(spsa_samples=4)),
                        ("apgd", dict(apgd=True))):
        with pytest.raises(ValueError, match=f"universal does not combine with .*{name}"):
            attack(net, x, 8 / 255, 2, universal=True, **extra, **kw)
    with pytest.raises(ValueError, match="momentum, nesterov, ti_kernel"):
        attack(net, x, 8 / 255, 2, universal=True, momentum=1.0, nesterov=True, ti_kernel=15, **kw)
    with pytest.raises(ValueError, match="universal does not combine with .*vt_samples"):
        fgsm(net, x, 8 / 255, target=t, universal=True, vt_samples=3)
    # a start noise of the batch's shape is not the ONE draw the shared perturbation takes
    for shape in ((2, 3, 32, 32), (3, 32, 32), (1, 3, 16, 16)):
        with pytest.raises(ValueError, match=r"start_noise.*\(1,3,S,S\)"):
            attack(net, x, 8 / 255, 2, universal=True, random_start=True,
                   start_noise=torch.zeros(shape), **kw)
    # the range of the integer sum: images × 3·S² < 2^37 (a view, no memory behind it)
    n_bad = -(-(1 << 37) // (3 * 32 * 32))
    big = torch.zeros(1, 3, 32, 32).expand(n_bad, 3, 32, 32)
    with pytest.raises(ValueError, match="2\\^37"):
        attack(net, big, 8 / 255, 2, universal=True, **kw)
    # valid arguments get as far as the network bundle, which a stub is not
    for extra in (dict(universal=True), dict(universal=np.bool_(True)), dict(universal=False),
                  dict(universal=True, random_start=True),
                  dict(universal=True, random_start=True, start_noise=torch.zeros(1, 3, 32, 32))):
        with pytest.raises(ValueError, match="device network"):
            attack(net, x, 8 / 255, 2, **extra, **kw)
    with pytest.raises(ValueError, match="device network"):
        fgsm(net, x, 8 / 255, target=t, universal=True)


def test_range_bound():
    """n·plane < 2^37 keeps |Σ q| ≤ n·plane·2^25·(1 + 2^-24) inside int64."""
    from gfa_amd import ops, pgd
    assert ops.UAP_MAX_ELEMENTS == 1 << 37
    plane = 3 * 256 * 256
    pgd.check_universal_count((1 << 37) // plane, plane)    # 699050 images of 256²
    pgd.check_universal_count(1, (1 << 37) - 1)
    for n, pl in (((1 << 37) // plane + 1, plane), (1, 1 << 37), (1 << 20, 1 << 17)):
        with pytest.raises(ValueError, match="2\\^37"):
            pgd.check_universal_count(n, pl)
    assert ((1 << 37) - 1) * (1 << 25) * (1 + 2.0 ** -24) < 2 ** 63
    assert "2^37" in pgd.check_universal_count.__doc__


def test_signatures_and_docs():
    import gfa_amd
    from gfa_amd import attack, fgsm, pgd
    from gfa_amd import dist as gdist
    from gfa_amd.pgd import AttackEngine
    p = inspect.signature(attack).parameters
    assert p["universal"].default is False
    assert p["universal"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(p)[-5:] == ["universal", "spsa_samples", "spsa_delta", "spsa_first_image", "apgd"]
    assert list(inspect.signature(AttackEngine.run_universal).parameters) == [
        "self", "x0", "t", "steps", "eps", "alpha", "random_start", "start_noise", "group"]
    for name in ("start_universal", "step_universal", "run_universal"):
        assert callable(getattr(AttackEngine, name))
    assert "uap." in AttackEngine._uap_buffers.__doc__
    assert gfa_amd.apply_universal is pgd.apply_universal and "apply_universal" in gfa_amd.__all__
    assert list(inspect.signature(pgd.apply_universal).parameters) == ["imgs", "delta"]
    for word in ("universal", "apply_universal", "int64", "world size", "2^37"):
        assert word in attack.__doc__, word
    assert "universal" in fgsm.__doc__
    for word in ("universal", "collective per step", "idle_rank_universal", "return_info",
                 "not sliced"):
        assert word in gdist.attack_distributed.__doc__, word
    with pytest.raises(ValueError, match="delta must be"):
        pgd.apply_universal(torch.zeros(2, 3, 8, 8), torch.zeros(3, 8, 8))
    with pytest.raises(ValueError, match="imgs"):
        pgd.apply_universal(torch.zeros(2, 3, 4, 4), torch.zeros(1, 3, 8, 8))
    if not torch.cuda.is_available():
        with pytest.raises(ValueError, match="GPU"):
            pgd.apply_universal(torch.zeros(2, 3, 8, 8), torch.zeros(1, 3, 8, 8))


def test_ops_wrappers_reject_before_the_library_call():
    from gfa_amd import ops
    g, x, x0 = (torch.zeros(2, 3, 8, 8) for _ in range(3))
    plane = 3 * 8 * 8
    l1, acc = torch.ones(2), torch.zeros(plane, dtype=torch.int64)
    delta = torch.zeros(1, 3, 8, 8)
    nf = torch.zeros(2, dtype=torch.int32)
    for bad in ((None, l1, acc), (g.double(), l1, acc), (g[:0], l1, acc), (torch.zeros(4), l1, acc),
                (g, None, acc), (g, torch.ones(3), acc), (g, l1.double(), acc), (g, l1, None),
                (g, l1, acc.to(torch.int32)), (g, l1, acc.float()), (g, l1, acc[:-1]),
                (g, l1, torch.zeros(2 * plane, dtype=torch.int64))):
        with pytest.raises(ValueError):
            ops.uap_accumulate(*bad, True)
    with pytest.raises(ValueError, match="nonfinite"):
        ops.uap_accumulate(g, l1, acc, True, nonfinite=torch.zeros(2))
    with pytest.raises(ValueError, match="nonfinite"):
        ops.uap_accumulate(g, l1, acc, True, nonfinite=torch.zeros(3, dtype=torch.int32))
    wide = torch.zeros(1, 4).expand(65536, 4)
    with pytest.raises(ValueError, match="65535"):
        ops.uap_accumulate(wide, torch.ones(65536), torch.zeros(4, dtype=torch.int64), True)
    with pytest.raises(ValueError, match="device tensor"):
        ops.uap_accumulate(g, l1, acc, True, nonfinite=nf)
    for bad in ((None, acc, x, x0), (delta.double(), acc, x, x0), (delta[:, :2], acc, x, x0),
                (delta, acc.float(), x, x0), (delta, acc[:-1], x, x0), (delta, acc, None, x0),
                (delta, acc, x, None), (delta, None, None, None), (delta, acc, x, x),
                (delta, acc, x[:1], x0), (delta, acc, x.double(), x0), (delta, acc, x, x0.double()),
                (delta, acc, torch.zeros(2, 3, 4, 4), torch.ones(2, 3, 4, 4)),
                (x0[:1], acc, x, x0), (x[:1], acc, x, x0)):
        with pytest.raises(ValueError):
            ops.uap_step(*bad, 0.01, 0.06)
    for a in (-0.01, float("nan"), float("inf"), "0", None, True):
        with pytest.raises(ValueError):
            ops.uap_step(delta, acc, x, x0, a, 0.06)
    for e in (0, -0.06, float("nan"), float("inf"), "0", None, True):
        with pytest.raises(ValueError):
            ops.uap_step(delta, acc, x, x0, 0.01, e)
    with pytest.raises(ValueError, match="lo <= hi"):
        ops.uap_step(delta, acc, x, x0, 0.01, 0.06, lo=1.0, hi=-1.0)
    for args in ((delta, acc, x, x0), (delta, None, x, x0), (delta, acc, None, None)):
        with pytest.raises(ValueError, match="device tensor"):
            ops.uap_step(*args, 0.0, 0.06)


# ---- C ABI validation (returns before any launch: runs without a GPU) ---------------------------
@pytest.mark.parametrize("name", ["mia_uap_accumulate", "mia_uap_step"])
def test_abi_uap_validation(name):
    from gfa_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    # never dereferenced: validation fails first. 2·3·32² floats = 24 KiB per image buffer,
    # 3·32² int64 = 24 KiB for acc
    b1, b2, b3, b4, f1, null = P(1 << 20), P(2 << 20), P(3 << 20), P(4 << 20), P(5 << 20), P(None)
    plane = 3 * 32 * 32

    def bad(a=b1, b=None, c=None, d=b4, N=2, plane=plane, sa=0.01, e=0.06, lo=-1.0, hi=1.0):
        if name == "mia_uap_accumulate":          # a = g, b = l1, c = acc
            b, c = f1 if b is None else b, b3 if c is None else c
            rc = lib.mia_uap_accumulate(a, b, c, N, plane, 1, null, null)
        else:                                     # a = delta, b = acc, c = x, d = x0
            b, c = b2 if b is None else b, b3 if c is None else c
            rc = lib.mia_uap_step(a, b, c, d, N, plane, sa, e, lo, hi, null)
        msg = lib.mia_last_error_string().decode()
        assert rc == -1, (rc, N, plane, sa, e, lo, hi)  # MIA_EINVAL
        assert name in msg and len(msg) > len(name) + 2, msg

    bad(a=null)
    for N in (-4, 1 << 16, 70000):
        bad(N=N)
    for pl in (0, -4, 1 << 31, 1 << 40):
        bad(plane=pl)
    if name == "mia_uap_accumulate":
        bad(b=null)
        bad(c=null)
        bad(N=0)
        bad(c=b1)                                 # acc is g
        bad(c=P((1 << 20) + 8 * plane - 8))       # acc starts inside g
        bad(b=P((3 << 20) + 8))                   # l1 inside acc
        bad(b=P((1 << 20) + 4))                   # l1 inside g
        bad(c=P((3 << 20) + 4))                   # acc not 8-byte aligned
        bad(N=65535, plane=(1 << 21) + 64)        # N·plane ≥ 2^37
        bad(N=65, plane=(1 << 31) - 1)
    else:
        bad(c=null)                               # N > 0 needs x and x0
        bad(d=null)
        bad(N=0)                                  # N = 0 needs x = x0 = NULL
        bad(N=0, c=null)
        bad(N=0, b=null, c=null, d=null)          # … and then a sum: nothing to do otherwise
        bad(b=b1)                                 # acc is delta
        bad(b=P((1 << 20) + 4 * plane - 8))       # acc starts on delta's last floats
        bad(c=b1)                                 # x is delta
        bad(d=b1)
        bad(c=b4)                                 # x is x0
        bad(c=P((4 << 20) + 4 * (2 * plane - 1)))  # x on x0's last float
        bad(c=b2)                                 # x is acc
        bad(d=P((2 << 20) + 8 * plane - 8))       # x0 on acc's last element
        bad(b=P((2 << 20) + 4))                   # acc not 8-byte aligned
        for sa in (-0.01, float("nan")):
            bad(sa=sa)
        for e in (0.0, -0.06, float("nan")):
            bad(e=e)
        bad(lo=1.0, hi=-1.0)
        bad(lo=float("nan"))


# ---- the collectives of a rank with an empty shard -----------------------------------------------
def test_idle_rank_universal_all_reduce_count(monkeypatch):
    """pgd.idle_rank_universal against a fake group: per run ``steps`` SUM all-reduces of a zero
    int64 plane, each followed by one δ-only uap_step on the reduced plane, then one MAX
    all-reduce of the status; a RESCALE verdict re-runs from δ₀, OK returns δ."""
    import torch.distributed as dist
    from gfa_amd import ops, pgd
    group, steps, shape = object(), 3, (1, 3, 4, 4)
    plane = 3 * 4 * 4
    log, verdicts = [], [pgd.RUN_RESCALE, pgd.RUN_OK]

    def fake_all_reduce(t, op=None, group=None):
        assert group is fake_group
        if op == dist.ReduceOp.SUM:
            assert t.dtype == torch.int64 and t.numel() == plane and not t.any()  # a zero plane
            log.append("sum")
            t += 7                                                                 # the others' sum
        else:
            assert op == dist.ReduceOp.MAX and t.dtype == torch.int32 and t.tolist() == [pgd.RUN_OK]
            log.append("max")
            t.fill_(verdicts.pop(0))

    def fake_uap_step(delta, acc, x, x0, a, e):
        assert x is None and x0 is None and acc.dtype == torch.int64 and acc.abs().eq(7).all()
        log.append("step")
        delta += a * torch.sign(acc).to(torch.float32).reshape(delta.shape)
        delta.clamp_(-e, e)

    fake_group = group
    monkeypatch.setattr(dist, "all_reduce", fake_all_reduce)
    monkeypatch.setattr(dist, "get_backend", lambda g=None: "gloo")
    monkeypatch.setattr(ops, "uap_step", fake_uap_step)
    delta = pgd.idle_rank_universal(group, steps, shape, 8 / 255, 2 / 255, torch.device("cpu"))
    assert log == (["sum", "step"] * steps + ["max"]) * 2
    assert log.count("sum") == 2 * steps and not verdicts
    # the second run started again from δ₀ = 0: three steps of +a, below e (six would clamp)
    want = torch.zeros(shape)
    for _ in range(steps):
        want += float(np.float32(2 * 2 / 255))
    assert tuple(delta.shape) == shape and torch.equal(delta, want) and want.max() < 2 * 8 / 255
    log.clear()
    verdicts[:] = [pgd.RUN_FATAL]
    with pytest.raises(FloatingPointError):
        pgd.idle_rank_universal(group, steps, shape, 8 / 255, 2 / 255, torch.device("cpu"))
    assert log == ["sum", "step"] * steps + ["max"]
    with pytest.raises(ValueError, match="start_noise"):
        pgd.idle_rank_universal(group, steps, shape, 8 / 255, 2 / 255, torch.device("cpu"),
                                random_start=True, start_noise=torch.zeros(2, 3, 4, 4))
