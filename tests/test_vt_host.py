"""Host side of the variance-tuned attack (no GPU): the counter-based generator's reference against
the Random123 known-answer vectors, the uniform mapping, the independence of the draws, attack()'s
argument validation before any device work, the wrappers' host checks, the C ABI's validation of
mia_vt_neighbor / mia_vt_combine_norms, and attack_distributed's image offsets over gloo."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import vt_ref
from test_dist_gloo import _free_port
from test_si_host import _StubNet

F = 0xFFFFFFFF


# ---- the reference --------------------------------------------------------------------------------
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((F, F, F, F), (F, F), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(counter, key, want):
    """The Random123 known-answer vectors of Philox4x32-10, as scalars and as arrays."""
    got = vt_ref.philox4x32_10(counter, key)
    assert tuple(int(w) for w in got) == want
    arr = vt_ref.philox4x32_10(tuple(np.full(3, w, dtype=np.uint64) for w in counter), key)
    for w, ww in zip(arr, want):
        assert w.dtype == np.uint32 and w.tolist() == [ww] * 3


def test_uniform_is_exact_symmetric_and_open():
    bits = np.concatenate([np.array([0, 0xff, 0x100, 0x7fffffff, 0x80000000, 0xffffff00,
                                     0xffffffff], dtype=np.uint32),
                           np.random.default_rng(3).integers(0, 1 << 32, 4096, dtype=np.uint64)
                           .astype(np.uint32)])
    u = vt_ref.uniform(bits)
    assert u.dtype == np.float32
    assert np.array_equal(u.astype(np.float64), vt_ref.uniform64(bits))       # exact
    lo, hi = float(vt_ref.uniform(0)), float(vt_ref.uniform(0xffffffff))
    assert lo == -(1.0 - 2.0 ** -24) and hi == 1.0 - 2.0 ** -24
    assert -1.0 < lo < 0.0 < hi < 1.0
    assert np.all(np.abs(u) < 1.0) and np.all(u != 0.0)
    assert np.array_equal(vt_ref.uniform(~bits), -u)                          # symmetric
    # every value is an odd multiple of 2^-24
    k = vt_ref.uniform64(bits) * 2.0 ** 24
    assert np.array_equal(k, np.round(k)) and np.all(k.astype(np.int64) % 2 != 0)


def test_uniform_moments():
    """U(−1, 1): mean 0 with variance 1/3, and u² has variance 1/5 − 1/9; both sample moments
    within 5 standard errors over the n = 6144 values of a 2 × 3 × 32 × 32 draw."""
    u = vt_ref.draw((2, 3, 32, 32), 7, 0, 0, 0).double()
    n = u.numel()
    assert n == 6144
    mean, var = u.mean().item(), u.var(unbiased=False).item()
    print(f"vt noise, key (7, 0): mean {mean:.4f}, variance {var:.4f}")
    assert abs(mean) <= 5 * math.sqrt(1 / (3 * n))
    assert abs(var - 1 / 3) <= 5 * math.sqrt((1 / 5 - 1 / 9) / n)


def test_draws_are_independent_and_image_indexed():
    shape = (3, 3, 5, 7)                                   # plane 105: a partial last group
    base = vt_ref.draw(shape, 5, 0, 0, 0)
    assert base.dtype == torch.float32 and tuple(base.shape) == shape
    assert torch.equal(base, vt_ref.draw(shape, 5, 0, 0, 0))
    for other in (vt_ref.draw(shape, 6, 0, 0, 0), vt_ref.draw(shape, 5 + (1 << 32), 0, 0, 0),
                  vt_ref.draw(shape, 5, 0, 1, 0), vt_ref.draw(shape, 5, 0, 0, 1),
                  vt_ref.draw(shape, 5, 1, 0, 0)):
        assert (other != base).float().mean().item() > 0.99
    assert not torch.equal(base[0], base[1]) and not torch.equal(base[1], base[2])
    # step and sample are different counter words: (1, 0) is not (0, 1)
    assert not torch.equal(vt_ref.draw(shape, 5, 0, 1, 0), vt_ref.draw(shape, 5, 0, 0, 1))
    # a batch's draw is the per-image draws with image0 shifted
    for n in range(3):
        assert torch.equal(vt_ref.draw((1,) + shape[1:], 5, 10 + n, 2, 3)[0],
                           vt_ref.draw(shape, 5, 10, 2, 3)[n])
    # the neighbour: the rounding order, the look-ahead and r = 0
    g = torch.Generator().manual_seed(8)
    x = torch.rand(shape, generator=g) * 2 - 1
    m = torch.rand(shape, generator=g) * 6 - 3
    c, r = float(np.float32(2 * 2 / 255)), float(np.float32(np.float32(1.5) * np.float32(16 / 255)))
    y = vt_ref.neighbor(x, m, c, r, 5, 10, 2, 3)
    assert y.dtype == torch.float32
    u = vt_ref.draw(shape, 5, 10, 2, 3)
    assert torch.equal(y, (x + m * torch.tensor(c)) + u * torch.tensor(r))
    assert (y - x - m * c).abs().max().item() <= r + 1e-6
    assert torch.equal(vt_ref.neighbor(x, None, c, 0.0, 5, 10, 2, 3), x)
    gt, v1 = vt_ref.combine(x, m, y)
    assert torch.equal(gt, x + y) and torch.equal(v1, m - x)
    gt, v1 = vt_ref.combine(x, None, y)
    assert torch.equal(gt, x + y) and torch.equal(v1, y)


# ---- attack(): every rejection happens before any device work ------------------------------------
def test_vt_validation_before_any_device_work():
    from gfa_amd import attack
    x = torch.zeros(2, 3, 32, 32)
    t = torch.zeros(1, 3, 32, 32)
    net = _StubNet()
    kw = dict(target=t, alpha=2 / 255)
    for bad in (0, 33, 2.0, True, "5", -1):
        with pytest.raises(ValueError, match="vt_samples"):
            attack(net, x, 8 / 255, 2, vt_samples=bad, **kw)
    for bad in (0, -1, float("nan"), float("inf"), True, "1.5", None):
        with pytest.raises(ValueError, match="vt_beta"):
            attack(net, x, 8 / 255, 2, vt_samples=5, vt_beta=bad, **kw)
    for bad in (-1, 1.5, True, "0", None, 1 << 32):
        with pytest.raises(ValueError, match="vt_first_image"):
            attack(net, x, 8 / 255, 2, vt_samples=5, vt_first_image=bad, **kw)
    with pytest.raises(ValueError, match="norm='linf' only"):
        attack(net, x, 1.0, 2, target=t, alpha=0.2, norm="l2", vt_samples=5)
    for norm in ("adam", "l2_cw"):
        with pytest.raises(ValueError, match="norm='linf' only"):
            attack(net, x, None, 2, target=t, norm=norm, vt_samples=5)
    with pytest.raises(ValueError, match="nesterov"):          # the look-ahead's own rule stays
        attack(net, x, 8 / 255, 2, vt_samples=5, nesterov=True, **kw)
    # valid arguments get as far as the network bundle, which a stub is not
    for extra in (dict(vt_samples=None), dict(vt_samples=1), dict(vt_samples=5),
                  dict(vt_samples=32), dict(vt_samples=np.int64(3)),
                  dict(vt_samples=5, vt_beta=0.5), dict(vt_samples=5, vt_beta=2),
                  dict(vt_samples=5, vt_first_image=7),
                  dict(vt_samples=5, vt_first_image=(1 << 32) - 2),
                  dict(vt_samples=5, momentum=1.0), dict(vt_samples=5, momentum=1.0, nesterov=True),
                  dict(vt_samples=5, ti_kernel=15), dict(vt_samples=5, di_prob=0.5),
                  dict(vt_samples=5, si_scales=5),
                  dict(vt_samples=5, momentum=1.0, nesterov=True, ti_kernel=15, di_prob=0.5,
                       si_scales=5)):
        with pytest.raises(ValueError, match="device network"):
            attack(net, x, 8 / 255, 2, **extra, **kw)


def test_signatures_constants_and_docs():
    from gfa_amd import attack, fgsm, pgd
    from gfa_amd import dist as gdist
    from gfa_amd.pgd import AttackEngine
    assert pgd.VT_MAX_SAMPLES == 32
    assert pgd.VT_SEED_OFFSET == 0x564D492D4647534D
    assert pgd.VT_SEED_OFFSET.to_bytes(8, "big") == b"VMI-FGSM"
    p = inspect.signature(attack).parameters
    assert p["vt_samples"].default is None and p["vt_beta"].default == 1.5
    assert p["vt_first_image"].default == 0
    for name in ("vt_samples", "vt_beta", "vt_first_image"):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY
    # the existing parameters keep their places; the new ones follow them
    q = list(inspect.signature(AttackEngine.step_mi).parameters)
    assert q[:10] == ["self", "x", "m", "momentum", "a", "e", "ti_taps", "di", "nesterov",
                      "si_scales"] and q[10:] == ["vt"]
    assert inspect.signature(AttackEngine.step_mi).parameters["vt"].default is None
    q = list(inspect.signature(AttackEngine.run_mi).parameters)
    assert q[:14] == ["self", "x0", "t", "steps", "eps", "alpha", "momentum", "random_start",
                      "start_noise", "group", "ti_taps", "di", "nesterov", "si_scales"]
    assert q[14:] == ["vt_samples", "vt_beta", "vt_seed", "vt_first_image"]
    assert inspect.signature(AttackEngine.run_mi).parameters["vt_samples"].default is None
    assert list(inspect.signature(AttackEngine._step_gradient).parameters) == [
        "self", "x", "m", "c", "si_scales", "di", "taps", "l1", "l2sq"]
    assert pgd.VtStep._fields == ("samples", "r", "seed", "image0", "step", "last")
    assert any(k.kind is inspect.Parameter.VAR_KEYWORD
               for k in inspect.signature(fgsm).parameters.values())
    for word in ("vt_samples", "vt_first_image", "world size"):
        assert word in gdist.attack_distributed.__doc__, word
    for word in ("vt_samples", "vt_beta", "vt_first_image", "VMIFGSM defaults to decay 1.0",
                 "Philox4x32-10", "stateless"):
        assert word in attack.__doc__, word
    assert "vt_samples" in fgsm.__doc__
    for n in (0, 33, 2.0, True):
        with pytest.raises(ValueError, match="vt_samples"):
            pgd._check_vt_samples(n)
    assert pgd._check_vt_samples(5) == 5 and pgd._check_vt_beta(2) == 2.0
    assert pgd._check_vt_first_image(3, 2) == 3


def test_ops_wrappers_reject_before_the_library_call():
    from gfa_amd import ops
    x = torch.zeros(2, 3, 8, 8)
    y = torch.zeros(2, 3, 8, 8)
    m = torch.zeros(2, 3, 8, 8)
    w = torch.zeros(2, 3, 8, 8)
    l1 = torch.zeros(2)
    nb = lambda a, mm, b, c=0.0, r=0.1, seed=1, image0=0, step=0, sample=0: \
        ops.vt_neighbor(a, mm, b, c, r, seed, image0, step, sample)             # noqa: E731
    for bad in ((x, None, x), (x, y, y), (x, None, y[:1]), (x.double(), None, y),
                (x, None, y.double()), (x, m[:1], y), (x, m.double(), y), (None, None, y)):
        with pytest.raises(ValueError):
            nb(*bad)
    for c in (float("inf"), float("nan"), "0", None, True):
        with pytest.raises(ValueError, match="c must"):
            nb(x, m, y, c=c)
    for r in (-0.1, float("inf"), float("nan"), "0", None, True):
        with pytest.raises(ValueError, match="r must"):
            nb(x, m, y, r=r)
    for seed in (-1, 1 << 64, 1.0, True, None):
        with pytest.raises(ValueError, match="seed"):
            nb(x, m, y, seed=seed)
    for name in ("image0", "step", "sample"):
        for v in (-1, 1 << 32, 1.0, True, None):
            with pytest.raises(ValueError, match=name):
                nb(x, m, y, **{name: v})
    with pytest.raises(ValueError, match="image0"):
        nb(x, m, y, image0=(1 << 32) - 1)                         # image0 + N > 2^32
    with pytest.raises(ValueError, match="device tensor"):
        nb(x, m, y, c=0.1, seed=(1 << 64) - 1, image0=(1 << 32) - 2, step=F, sample=F)
    cb = ops.vt_combine_norms
    for bad in ((x, m, y, x), (x, m, x, w), (x, x, y, w), (x, m, y, y), (x, y, y, w),
                (x, m, y, m), (x, m, y[:1], w), (x, m[:1], y, w), (x, m, y, w[:1]),
                (x.double(), m, y, w), (x, m.double(), y, w), (x, m, y.double(), w),
                (x, m, y, w.double()), (None, m, y, w), (x, m, None, w), (x, m, y, None),
                (x, None, x, w), (x, None, y, y)):
        with pytest.raises(ValueError):
            cb(*bad, l1)
    with pytest.raises(ValueError):
        cb(x, m, y, w, torch.zeros(3))
    with pytest.raises(ValueError):
        cb(x, m, y, w, l1.double())
    with pytest.raises(ValueError):
        cb(x, m, y, w, l1, nonfinite=torch.zeros(2))             # not int32
    with pytest.raises(ValueError, match="device tensor"):
        cb(x, m, y, w, l1)
    with pytest.raises(ValueError, match="device tensor"):
        cb(x, None, y, w, None)


# ---- C ABI validation (returns before any launch: runs without a GPU) ---------------------------
@pytest.mark.parametrize("name", ["mia_vt_neighbor", "mia_vt_combine_norms"])
def test_abi_vt_validation(name):
    from gfa_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    # never dereferenced: validation fails first. 2·3·32² floats = 24 KiB per buffer
    b1, b2, b3, b4, null = P(1 << 20), P(2 << 20), P(3 << 20), P(4 << 20), P(None)
    plane = 3 * 32 * 32
    last = 4 * (2 * plane - 1)                  # byte offset of a buffer's last float

    def bad(a=b1, b=b2, c3=b3, d=b4, N=2, plane=plane, c=0.0, r=0.1, image0=0):
        if name == "mia_vt_neighbor":           # a = x, b = y, c3 = m (or null)
            rc = lib.mia_vt_neighbor(a, c3, b, N, plane, c, r, 5, image0, 0, 0, null)
        else:                                   # a = g, c3 = gv (or null), b = v, d = gt
            rc = lib.mia_vt_combine_norms(a, c3, b, d, null, N, plane, null, null)
        msg = lib.mia_last_error_string().decode()
        assert rc == -1, (rc, N, plane, c, r, image0)  # MIA_EINVAL
        assert name in msg and len(msg) > len(name) + 2, msg

    bad(a=null)
    bad(b=null)
    bad(b=b1)                                   # in place
    bad(b=P((1 << 20) + 4))                     # overlapping, shifted by one float
    bad(b=P((1 << 20) + last))                  # the last float of a
    bad(a=P((1 << 20) + 4096), b=b1)            # overlapping the other way round
    bad(c3=b2)                                  # m is y / gv is v
    bad(c3=P((2 << 20) + last))
    for N in (0, -4, 1 << 16, 70000):
        bad(N=N)
    for pl in (0, -4, 1 << 31, 1 << 40):
        bad(plane=pl)
    if name == "mia_vt_neighbor":
        bad(c3=null, b=b1)                      # in place without the look-ahead
        for c in (float("inf"), float("nan")):
            bad(c=c)
        for r in (-0.5, float("inf"), float("nan")):
            bad(r=r)
        bad(image0=(1 << 32) - 1)               # image0 + N = 2^32 + 1
        bad(image0=(1 << 32) - 1, c3=null)
    else:
        bad(d=null)
        bad(d=b1)                               # gt is g
        bad(d=b2)                               # gt is v
        bad(d=b3)                               # gt is gv
        bad(c3=b1)                              # gv is g
        bad(c3=null, d=b1)                      # the last step's form, gt is g
        bad(d=P((3 << 20) + last))              # gt overlaps gv's last float


# ---- attack_distributed: every shard carries its global image offset -----------------------------
def _fake_vt_attack(net, imgs, eps, steps, *, target, vt_first_image=0, **kw):
    """Stand-in for pgd.attack: row n of its output holds vt_first_image + n."""
    assert imgs.shape[0] >= 1 and kw["vt_samples"] == 3
    rows = torch.arange(imgs.shape[0], dtype=torch.float32) + float(vt_first_image)
    return rows.reshape(-1, 1, 1, 1).expand_as(imgs).contiguous()


def _vt_dist_worker(rank, world, port, n, first, out_q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import types

    import gfa_import  # noqa: F401
    from gfa_amd import dist as gdist
    from gfa_amd import pgd
    pgd.attack = _fake_vt_attack  # the distributed wrapper looks it up at call time
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        imgs = torch.zeros(n, 3, 4, 4)
        net = types.SimpleNamespace(decoder=types.SimpleNamespace(device=torch.device("cpu")))
        kw = dict(vt_samples=3)
        if first is not None:
            kw["vt_first_image"] = first
        got = gdist.attack_distributed(net, imgs, 8 / 255, 3, target=imgs[:1], **kw)
        want = torch.arange(n, dtype=torch.float32) + float(first or 0)
        out_q.put((rank, torch.equal(got, want.reshape(-1, 1, 1, 1).expand_as(imgs))))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n,first", [(2, 5, None), (3, 7, None), (3, 8, 100)])
def test_attack_distributed_passes_global_image_indices(world, n, first):
    """Over gloo (world 2 and 3, uneven n): every shard's attack receives vt_first_image = the
    caller's value + its first row, so the gathered rows are the global indices on every rank,
    whatever the world size. (Every rank has a shard: the fake attack takes no part in the
    status rounds that a rank with an empty shard waits in.)"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_vt_dist_worker, args=(r, world, port, n, first, q), daemon=True)
             for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert all(ok for _, ok in res), res
