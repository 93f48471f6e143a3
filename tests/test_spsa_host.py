"""Host side of the SPSA black-box attack (no GPU): the Rademacher directions of the reference
(tests/spsa_ref.py, on vt_ref's Philox4x32-10), the fp64 estimator on a linear objective, attack()'s
argument validation before any device work, the wrappers' host checks, the C ABI's validation of
mia_spsa_probe / mia_spsa_accumulate_norms, and attack_distributed's image offsets over gloo."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import spsa_ref
from test_dist_gloo import _free_port
from test_si_host import _StubNet

F = 0xFFFFFFFF


# ---- the reference --------------------------------------------------------------------------------
def test_directions_are_rademacher_and_bit_symmetric():
    """v is exactly ±1, decided by bit 31 of the word alone, and flips under ~bits."""
    bits = np.concatenate([np.array([0, 1, 0x7fffffff, 0x80000000, 0x80000001, 0xffffffff],
                                    dtype=np.uint32),
                           np.random.default_rng(3).integers(0, 1 << 32, 4096, dtype=np.uint64)
                           .astype(np.uint32)])
    v = spsa_ref.sign_of(bits)
    assert v.dtype == np.float32
    assert v[:6].tolist() == [1.0, 1.0, 1.0, -1.0, -1.0, -1.0]
    assert np.all(np.abs(v) == 1.0)
    assert np.array_equal(spsa_ref.sign_of(~bits), -v)
    d = spsa_ref.directions((2, 3, 5, 7), 5, 0, 0, 0)
    assert d.dtype == torch.float32 and tuple(d.shape) == (2, 3, 5, 7)
    assert torch.equal(d.abs(), torch.ones_like(d))
    # the words are vt_ref's: the same counter layout as the variance-tuning noise
    import vt_ref
    w = spsa_ref.words((2, 3, 5, 7), 5, 0, 0, 0)
    assert torch.equal(vt_ref.draw((2, 3, 5, 7), 5, 0, 0, 0),
                       torch.from_numpy(vt_ref.uniform(w)))


def test_directions_are_independent_and_image_indexed():
    shape = (3, 3, 5, 7)                                   # plane 105: a partial last group
    base = spsa_ref.directions(shape, 5, 0, 0, 0)
    assert torch.equal(base, spsa_ref.directions(shape, 5, 0, 0, 0))
    # another seed (either key word), step, sample or image: about half of the signs flip
    for other in (spsa_ref.directions(shape, 6, 0, 0, 0),
                  spsa_ref.directions(shape, 5 + (1 << 32), 0, 0, 0),
                  spsa_ref.directions(shape, 5, 0, 1, 0), spsa_ref.directions(shape, 5, 0, 0, 1),
                  spsa_ref.directions(shape, 5, 1, 0, 0)):
        assert 0.3 < (other != base).float().mean().item() < 0.7
    assert not torch.equal(base[0], base[1]) and not torch.equal(base[1], base[2])
    assert not torch.equal(spsa_ref.directions(shape, 5, 0, 1, 0),
                           spsa_ref.directions(shape, 5, 0, 0, 1))
    for n in range(3):
        assert torch.equal(spsa_ref.directions((1,) + shape[1:], 5, 10 + n, 2, 3)[0],
                           spsa_ref.directions(shape, 5, 10, 2, 3)[n])


def test_direction_mean():
    """Rademacher: mean 0, variance 1; the sample mean within 5/√n over the n = 6144 values of a
    2 × 3 × 32 × 32 draw."""
    v = spsa_ref.directions((2, 3, 32, 32), 7, 0, 0, 0).double()
    n = v.numel()
    assert n == 6144
    mean = v.mean().item()
    print(f"spsa directions, key (7, 0): mean {mean:.4f} (bound {5 / math.sqrt(n):.4f})")
    assert abs(mean) <= 5 / math.sqrt(n)


def test_probe_and_accumulate_references():
    """The references' rounding order, the clamp and the division."""
    shape = (2, 3, 5, 7)
    g = torch.Generator().manual_seed(8)
    x = torch.rand(shape, generator=g) * 2 - 1
    x[0, 0, 0, 0], x[1, 2, 4, 6] = 1.0, -1.0
    d = float(np.float32(0.02))
    v = spsa_ref.directions(shape, 5, 10, 2, 3)
    yp, ym = spsa_ref.probe(x, d, 5, 10, 2, 3)
    assert yp.dtype == torch.float32 and ym.dtype == torch.float32
    assert torch.equal(yp, torch.clamp(x + v * torch.tensor(d), -1, 1))
    assert torch.equal(ym, torch.clamp(x - v * torch.tensor(d), -1, 1))
    assert yp.abs().max() <= 1 and ym.abs().max() <= 1
    assert {float(yp[0, 0, 0, 0]), float(ym[0, 0, 0, 0])} == {1.0, float(np.float32(1) - np.float32(d))}
    fp, fm = torch.tensor([3.0, -1.0]), torch.tensor([2.5, 4.0])
    s = 25.0
    a1 = spsa_ref.accumulate(torch.full(shape, float("nan")), fp, fm, s, 5, 10, 2, 3, True)
    c = torch.tensor([12.5, -125.0]).reshape(2, 1, 1, 1)
    assert torch.equal(a1, v * c)
    a2 = spsa_ref.accumulate(a1, fp, fm, s, 5, 10, 2, 4, False, 2.0)
    assert torch.equal(a2, (a1 + spsa_ref.directions(shape, 5, 10, 2, 4) * c) / 2)


def test_estimate_on_a_linear_objective():
    """f(y) = w·y: ĝ = (1/q)·Σ_i (w·v_i)·v_i, whose expected cosine with w is √(q/(q + D − 1)) in the
    linear regime. At D = 3·16², q = 64 the reference estimate must reach half of it (a floor, not
    a measurement), per image."""
    D, q = 3 * 16 * 16, 64
    g = torch.Generator().manual_seed(11)
    w = torch.randn((2, 3, 16, 16), generator=g, dtype=torch.float64)
    x = torch.zeros(2, 3, 16, 16)                           # no clamp acts at d = 0.02
    est = spsa_ref.estimate(lambda y: (w * y).reshape(2, -1).sum(1), x, q, 0.02, 5, 0, 0)
    cos = torch.nn.functional.cosine_similarity(est.reshape(2, -1), w.reshape(2, -1), dim=1)
    floor = 0.5 * math.sqrt(q / (q + D - 1))
    print(f"spsa linear objective D={D} q={q}: cosine {cos.tolist()}, expected "
          f"{math.sqrt(q / (q + D - 1)):.4f}, floor {floor:.4f}")
    assert cos.min().item() >= floor
    # the closed form of the linear case
    want = torch.zeros_like(w)
    for i in range(q):
        v = spsa_ref.directions((2, 3, 16, 16), 5, 0, 0, i).double()
        want += (w * v).reshape(2, -1).sum(1).reshape(2, 1, 1, 1) * v
    assert torch.allclose(est, want / q, rtol=1e-9, atol=1e-12)


# ---- attack(): every rejection happens before any device work ------------------------------------
def test_spsa_validation_before_any_device_work():
    from gfa_amd import attack, fgsm
    x = torch.zeros(2, 3, 32, 32)
    t = torch.zeros(1, 3, 32, 32)
    net = _StubNet()
    kw = dict(target=t, alpha=2 / 255)
    for bad in (0, 257, 2.0, True, "5", -1):
        with pytest.raises(ValueError, match="spsa_samples"):
            attack(net, x, 8 / 255, 2, spsa_samples=bad, **kw)
    for bad in (0, -0.01, float("nan"), float("inf"), True, "0.01", None, 1e-60):
        with pytest.raises(ValueError, match="spsa_delta"):
            attack(net, x, 8 / 255, 2, spsa_samples=4, spsa_delta=bad, **kw)
    for bad in (-1, 1.5, True, "0", None, 1 << 32):
        with pytest.raises(ValueError, match="spsa_first_image"):
            attack(net, x, 8 / 255, 2, spsa_samples=4, spsa_first_image=bad, **kw)
    for norm in ("adam", "l2_cw"):
        with pytest.raises(ValueError, match="spsa_samples"):
            attack(net, x, None, 2, target=t, norm=norm, spsa_samples=4)
    sched = np.array([[32, 0, 0, 0], [32, 0, 0, 0]])
    for name, extra in (("nesterov", dict(momentum=1.0, nesterov=True)),
                        ("ti_kernel", dict(ti_kernel=15)), ("di_prob", dict(di_prob=0.5)),
                        ("di_schedule", dict(di_schedule=sched)), ("si_scales", dict(si_scales=2)),
                        ("si_scales", dict(si_scales=1)), ("vt_samples", dict(vt_samples=3)),
                        ("apgd", dict(apgd=True))):
        with pytest.raises(ValueError, match=f"spsa_samples.*{name}"):
            attack(net, x, 8 / 255, 2, spsa_samples=4, **extra, **kw)
    with pytest.raises(ValueError, match="ti_kernel, si_scales"):
        attack(net, x, 8 / 255, 2, spsa_samples=4, ti_kernel=15, si_scales=3, **kw)
    with pytest.raises(ValueError, match="spsa_samples.*vt_samples"):
        fgsm(net, x, 8 / 255, target=t, spsa_samples=4, vt_samples=3)
    # the other keywords' own rules stay
    with pytest.raises(ValueError, match="apgd"):
        attack(net, x, 8 / 255, 2, spsa_samples=4, apgd=True, momentum=1.0, **kw)
    with pytest.raises(ValueError, match="momentum"):
        attack(net, x, 1.0, 2, target=t, alpha=0.2, norm="l2", spsa_samples=4, momentum=1.0)
    # valid arguments get as far as the network bundle, which a stub is not
    for extra in (dict(spsa_samples=None), dict(spsa_samples=None, spsa_delta=0.02),
                  dict(spsa_samples=1), dict(spsa_samples=256), dict(spsa_samples=np.int64(3)),
                  dict(spsa_samples=4, spsa_delta=0.5), dict(spsa_samples=4, spsa_delta=1),
                  dict(spsa_samples=4, spsa_first_image=7),
                  dict(spsa_samples=4, spsa_first_image=(1 << 32) - 2),
                  dict(spsa_samples=4, momentum=0.0), dict(spsa_samples=4, momentum=1.0)):
        with pytest.raises(ValueError, match="device network"):
            attack(net, x, 8 / 255, 2, **extra, **kw)
    with pytest.raises(ValueError, match="device network"):
        attack(net, x, 1.0, 2, target=t, alpha=0.2, norm="l2", spsa_samples=4)
    with pytest.raises(ValueError, match="device network"):
        fgsm(net, x, 8 / 255, target=t, spsa_samples=4)


def test_signatures_constants_and_docs():
    from gfa_amd import attack, fgsm, pgd
    from gfa_amd import dist as gdist
    from gfa_amd.pgd import AttackEngine
    assert pgd.SPSA_MAX_SAMPLES == 256
    assert pgd.SPSA_SEED_OFFSET == 0x535053412D41544B
    assert pgd.SPSA_SEED_OFFSET.to_bytes(8, "big") == b"SPSA-ATK"
    assert pgd.SPSA_SEED_OFFSET not in (pgd.VT_SEED_OFFSET, pgd.DI_SEED_OFFSET)
    p = inspect.signature(attack).parameters
    assert p["spsa_samples"].default is None and p["spsa_delta"].default == 0.01
    assert p["spsa_first_image"].default == 0
    for name in ("spsa_samples", "spsa_delta", "spsa_first_image"):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(p)[-4:] == ["spsa_samples", "spsa_delta", "spsa_first_image", "apgd"]
    assert list(p)[-1] == "apgd"
    assert pgd.SpsaStep._fields == ("samples", "d", "seed", "image0", "step")
    assert list(inspect.signature(AttackEngine.spsa_gradient).parameters) == [
        "self", "x", "sp", "l1", "l2sq"]
    assert list(inspect.signature(AttackEngine.step_spsa).parameters) == [
        "self", "x", "m", "momentum", "a", "e", "sp", "norm"]
    assert inspect.signature(AttackEngine.step_spsa).parameters["norm"].default == "linf"
    q = inspect.signature(AttackEngine.run_spsa).parameters
    assert list(q) == ["self", "x0", "t", "steps", "eps", "alpha", "momentum", "norm",
                       "random_start", "start_noise", "group", "spsa_samples", "spsa_delta",
                       "spsa_seed", "spsa_first_image"]
    assert q["momentum"].default == 0.0 and q["norm"].default == "linf"
    assert q["spsa_delta"].default == 0.01 and q["spsa_seed"].default == 0
    # the white-box steps keep their signatures
    assert list(inspect.signature(AttackEngine._step_gradient).parameters) == [
        "self", "x", "m", "c", "si_scales", "di", "taps", "l1", "l2sq"]
    for word in ("spsa_samples", "spsa_delta", "spsa_first_image", "world size"):
        assert word in gdist.attack_distributed.__doc__, word
    for word in ("spsa_samples", "spsa_delta", "spsa_first_image", "score-based", "Rademacher",
                 "queries"):
        assert word in attack.__doc__, word
    assert "spsa_samples" in fgsm.__doc__
    assert pgd.NORMS == ("linf", "l2", "adam", "l2_cw")
    assert pgd._check_spsa_samples(5) == 5 and pgd._check_spsa_delta(0.02) == 0.02
    assert pgd._check_spsa_first_image(3, 2) == 3
    d = np.float32(0.02)
    assert pgd.spsa_scale(0.02) == float(np.float32(1) / (np.float32(2) * d))


def test_ops_wrappers_reject_before_the_library_call():
    from gfa_amd import ops
    x, yp, ym = (torch.zeros(2, 3, 8, 8) for _ in range(3))
    fp, fm, l1 = torch.zeros(2), torch.zeros(2), torch.zeros(2)
    pr = lambda a, b, c, d=0.02, seed=1, image0=0, step=0, sample=0, **k: \
        ops.spsa_probe(a, b, c, d, seed, image0, step, sample, **k)              # noqa: E731
    ac = lambda a, p, m, s1=l1, s2=None, s=25.0, seed=1, image0=0, step=0, sample=0, first=True, \
        **k: ops.spsa_accumulate_norms(a, p, m, s1, s2, s, seed, image0, step, sample, first, **k)  # noqa: E731,E501
    for bad in ((x, x, ym), (x, yp, x), (x, yp, yp), (x, yp[:1], ym), (x, yp, ym[:1]),
                (x.double(), yp, ym), (x, yp.double(), ym), (x, yp, ym.double()), (None, yp, ym),
                (x, None, ym), (x, yp, None)):
        with pytest.raises(ValueError):
            pr(*bad)
    for d in (0, -0.1, float("inf"), float("nan"), "0", None, True):
        with pytest.raises(ValueError, match="d must"):
            pr(x, yp, ym, d=d)
    with pytest.raises(ValueError, match="lo <= hi"):
        pr(x, yp, ym, lo=1.0, hi=-1.0)
    for bad in ((None, fp, fm), (x, None, fm), (x, fp, None), (x, fp, fp), (x.double(), fp, fm),
                (x, fp.double(), fm), (x, fp, fm.double()), (x, torch.zeros(3), fm),
                (x, fp, torch.zeros(2, 1))):
        with pytest.raises(ValueError):
            ac(*bad)
    with pytest.raises(ValueError):
        ac(x, fp, fm, s1=torch.zeros(3))
    with pytest.raises(ValueError):
        ac(x, fp, fm, s2=l1.double())
    with pytest.raises(ValueError):
        ac(x, fp, fm, nonfinite=torch.zeros(2))                  # not int32
    for s in (0, -1.0, float("inf"), float("nan"), "1", None, True):
        with pytest.raises(ValueError, match="s must"):
            ac(x, fp, fm, s=s)
    for div in (0, -2.0, float("inf"), float("nan"), "1", None, True):
        with pytest.raises(ValueError, match="div must"):
            ac(x, fp, fm, div=div)
    for fn, args in ((pr, (x, yp, ym)), (ac, (x, fp, fm))):
        for seed in (-1, 1 << 64, 1.0, True, None):
            with pytest.raises(ValueError, match="seed"):
                fn(*args, seed=seed)
        for name in ("image0", "step", "sample"):
            for v in (-1, 1 << 32, 1.0, True, None):
                with pytest.raises(ValueError, match=name):
                    fn(*args, **{name: v})
        with pytest.raises(ValueError, match="image0"):
            fn(*args, image0=(1 << 32) - 1)                       # image0 + N > 2^32
        with pytest.raises(ValueError, match="device tensor"):
            fn(*args, seed=(1 << 64) - 1, image0=(1 << 32) - 2, step=F, sample=F)


# ---- C ABI validation (returns before any launch: runs without a GPU) ---------------------------
@pytest.mark.parametrize("name", ["mia_spsa_probe", "mia_spsa_accumulate_norms"])
def test_abi_spsa_validation(name):
    from gfa_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    # never dereferenced: validation fails first. 2·3·32² floats = 24 KiB per buffer
    b1, b2, b3, f1, f2, null = P(1 << 20), P(2 << 20), P(3 << 20), P(4 << 20), P(5 << 20), P(None)
    plane = 3 * 32 * 32
    last = 4 * (2 * plane - 1)                  # byte offset of a buffer's last float

    def bad(a=b1, b=None, c=None, N=2, plane=plane, d=0.02, lo=-1.0, hi=1.0, s=25.0, div=1.0,
            image0=0):
        if name == "mia_spsa_probe":            # a = x, b = yp, c = ym
            b, c = b2 if b is None else b, b3 if c is None else c
            rc = lib.mia_spsa_probe(a, b, c, N, plane, d, lo, hi, 5, image0, 0, 0, null)
        else:                                   # a = acc, b = fp, c = fm
            b, c = f1 if b is None else b, f2 if c is None else c
            rc = lib.mia_spsa_accumulate_norms(a, b, c, null, null, N, plane, s, 5, image0, 0, 0,
                                               1, div, null, null)
        msg = lib.mia_last_error_string().decode()
        assert rc == -1, (rc, N, plane, d, s, div, image0)  # MIA_EINVAL
        assert name in msg and len(msg) > len(name) + 2, msg

    bad(a=null)
    bad(b=null)
    bad(c=null)
    bad(b=b1)                                   # yp is x / fp is acc
    bad(c=b1)
    bad(b=P((1 << 20) + last))                  # the last float of a
    for N in (0, -4, 1 << 16, 70000):
        bad(N=N)
    for pl in (0, -4, 1 << 31, 1 << 40):
        bad(plane=pl)
    bad(image0=(1 << 32) - 1)                   # image0 + N = 2^32 + 1
    if name == "mia_spsa_probe":
        bad(b=b3)                               # yp is ym
        bad(b=P((1 << 20) + 4))                 # overlapping, shifted by one float
        bad(a=P((1 << 20) + 4096), b=b1)        # overlapping the other way round
        bad(c=P((2 << 20) + last))              # ym on yp's last float
        for d in (0.0, -0.02, float("inf"), float("nan")):
            bad(d=d)
        bad(lo=1.0, hi=-1.0)
        bad(lo=float("nan"))
    else:
        bad(b=f2)                               # fp is fm
        bad(c=P((4 << 20) + 4))                 # fm on fp's second float
        bad(a=P((4 << 20) + 4))                 # acc starts inside fp
        for s in (0.0, -25.0, float("inf"), float("nan")):
            bad(s=s)
        for div in (0.0, -1.0, float("inf"), float("nan")):
            bad(div=div)


# ---- attack_distributed: every shard carries its global image offset -----------------------------
def _fake_spsa_attack(net, imgs, eps, steps, *, target, spsa_first_image=0, **kw):
    """Stand-in for pgd.attack: row n of its output holds spsa_first_image + n."""
    assert imgs.shape[0] >= 1 and kw["spsa_samples"] == 3 and "vt_first_image" not in kw
    rows = torch.arange(imgs.shape[0], dtype=torch.float32) + float(spsa_first_image)
    return rows.reshape(-1, 1, 1, 1).expand_as(imgs).contiguous()


def _spsa_dist_worker(rank, world, port, n, first, out_q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import types

    import gfa_import  # noqa: F401
    from gfa_amd import dist as gdist
    from gfa_amd import pgd
    pgd.attack = _fake_spsa_attack  # the distributed wrapper looks it up at call time
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        imgs = torch.zeros(n, 3, 4, 4)
        net = types.SimpleNamespace(decoder=types.SimpleNamespace(device=torch.device("cpu")))
        kw = dict(spsa_samples=3)
        if first is not None:
            kw["spsa_first_image"] = first
        got = gdist.attack_distributed(net, imgs, 8 / 255, 3, target=imgs[:1], **kw)
        want = torch.arange(n, dtype=torch.float32) + float(first or 0)
        out_q.put((rank, torch.equal(got, want.reshape(-1, 1, 1, 1).expand_as(imgs))))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n,first", [(2, 5, None), (2, 6, 100)])
def test_attack_distributed_passes_global_image_indices(world, n, first):
    """Over gloo (world 2, even and uneven n): every shard's attack receives spsa_first_image =
    the caller's value + its first row, so the gathered rows are the global indices on every
    rank."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_spsa_dist_worker, args=(r, world, port, n, first, q), daemon=True)
             for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert all(ok for _, ok in res), res
