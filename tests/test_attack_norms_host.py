"""Host side of the L2-ball PGD / momentum attacks (no GPU): argument validation, the random-start
draws, the C ABI's validation of the four new entry points, and the world-size independence of
the L2 random start in attack_distributed (gloo, a stand-in attack)."""
import ctypes
import os
import socket
import types

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


class _StubDecoder:
    size = 32
    device = torch.device("cpu")


class _StubNet:
    decoder = _StubDecoder()
    vgg = object()


def test_norm_and_momentum_validation_before_any_device_work():
    from gfa_amd import attack
    x = torch.zeros(2, 3, 32, 32)
    t = torch.zeros(1, 3, 32, 32)
    net = _StubNet()
    with pytest.raises(ValueError, match="norm='linf' only"):
        attack(net, x, 0.5, 2, target=t, norm="l2", alpha=0.1, momentum=1.0)
    with pytest.raises(ValueError, match="norm='linf' only"):
        attack(net, x, None, 2, target=t, norm="adam", momentum=0.5)
    with pytest.raises(ValueError, match="momentum must be >= 0"):
        attack(net, x, 8 / 255, 2, target=t, momentum=-0.1)
    with pytest.raises(ValueError, match="momentum must be >= 0"):
        attack(net, x, 8 / 255, 2, target=t, momentum=float("nan"))
    with pytest.raises(ValueError, match="norm must be one of"):
        attack(net, x, 8 / 255, 2, target=t, norm="l1")
    with pytest.raises(ValueError, match="eps > 0"):
        attack(net, x, None, 2, target=t, norm="l2")
    with pytest.raises(ValueError, match="eps > 0"):
        attack(net, x, 0.5, 2, target=t, norm="l2", alpha=0.0)
    with pytest.raises(ValueError, match="eps > 0"):
        attack(net, x, -1.0, 2, target=t, momentum=1.0)
    # valid L2 / momentum arguments get as far as the network bundle, which a stub is not
    with pytest.raises(ValueError, match="device network"):
        attack(net, x, 0.5, 2, target=t, norm="l2", alpha=0.1)
    with pytest.raises(ValueError, match="device network"):
        attack(net, x, 8 / 255, 2, target=t, momentum=1.0)


def test_norms_list():
    from gfa_amd import pgd
    assert set(pgd.NORMS) == {"linf", "l2", "adam", "l2_cw"}


def test_linf_start_noise_is_unchanged():
    from gfa_amd.pgd import make_start_noise
    for shape, seed in (((2, 3, 8, 8), 0), ((5, 3, 4, 4), 11)):
        want = torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1
        assert torch.equal(make_start_noise(shape, seed), want)
        assert torch.equal(make_start_noise(shape, seed, "linf"), want)
    with pytest.raises(ValueError):
        make_start_noise((2, 3, 4, 4), 0, "adam")


def test_l2_start_noise_is_a_point_of_the_unit_ball_per_image():
    from gfa_amd.pgd import make_start_noise
    n = make_start_noise((64, 3, 8, 8), 5, "l2")
    assert n.shape == (64, 3, 8, 8) and n.dtype == torch.float32
    r = n.reshape(64, -1).norm(dim=1)
    assert (r <= 1).all() and (r > 0).all()
    assert 0.3 < r.mean() < 0.7 and r.max() > 0.9 and r.min() < 0.1  # r ~ U(0, 1)
    # isotropic direction: no element dominates, both signs
    u = n.reshape(64, -1) / r[:, None]
    assert u.abs().max() < 0.4 and 0.4 < (u > 0).float().mean() < 0.6
    assert torch.equal(n, make_start_noise((64, 3, 8, 8), 5, "l2"))
    assert not torch.equal(n, make_start_noise((64, 3, 8, 8), 6, "l2"))


# ---- C ABI validation (returns before any launch: runs without a GPU) ---------------------------
def _abi():
    from gfa_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    ok = P(4096)  # never dereferenced: every call below fails validation first

    def expect_einval(name, *args):
        rc = getattr(lib, name)(*args)
        msg = lib.mia_last_error_string().decode()
        assert rc == -1, (name, rc)  # MIA_EINVAL
        assert name in msg and len(msg) > len(name) + 2, msg
    return expect_einval, ok, P(None)


def test_abi_grad_assemble_norms_validation():
    bad, ok, null = _abi()
    name = "mia_grad_assemble_norms"

    def call(x=ok, x0=ok, gv=ok, ge=ok, g=ok, N=2, S=32, pf=1, cpad=8, enc=16, dtype=0):
        bad(name, x, x0, gv, ge, g, ok, ok, N, S, pf, cpad, enc, 1.0, 1.0, null, dtype, null)
    call(x=null)
    call(x0=null)
    call(g=null)
    call(N=0)
    call(N=-3)
    call(N=70000)
    call(S=0)
    call(pf=0)
    call(pf=3)        # does not divide S
    call(enc=5)       # does not divide S
    call(enc=0)
    call(cpad=2)
    call(dtype=7)


def test_abi_l2_and_mi_validation():
    bad, ok, null = _abi()
    for k in range(5):
        a = [ok] * 5
        a[k] = null
        bad("mia_l2_step", *a, 2, 3072, 0.1, null, null)
        bad("mia_mi_update", *a, 2, 3072, 1.0, 0.1, 0.1, -1.0, 1.0, null, null)
    for k in range(3):
        a = [ok] * 3
        a[k] = null
        bad("mia_l2_project", *a, 2, 3072, 0.1, -1.0, 1.0, null)
    for N, plane in ((0, 3072), (-1, 3072), (2, 0), (2, -4), (2, 1 << 31), (1 << 16, 3072)):
        bad("mia_l2_step", ok, ok, ok, ok, ok, N, plane, 0.1, null, null)
        bad("mia_l2_project", ok, ok, ok, N, plane, 0.1, -1.0, 1.0, null)
        bad("mia_mi_update", ok, ok, ok, ok, ok, N, plane, 1.0, 0.1, 0.1, -1.0, 1.0, null, null)
    bad("mia_l2_step", ok, ok, ok, ok, ok, 2, 3072, 0.0, null, null)              # a <= 0
    bad("mia_l2_project", ok, ok, ok, 2, 3072, -0.5, -1.0, 1.0, null)             # e <= 0
    bad("mia_l2_project", ok, ok, ok, 2, 3072, 0.5, 1.0, -1.0, null)              # lo > hi
    bad("mia_mi_update", ok, ok, ok, ok, ok, 2, 3072, -1.0, 0.1, 0.1, -1.0, 1.0, null, null)
    bad("mia_mi_update", ok, ok, ok, ok, ok, 2, 3072, float("nan"), 0.1, 0.1, -1.0, 1.0, null,
        null)
    bad("mia_mi_update", ok, ok, ok, ok, ok, 2, 3072, 1.0, 0.1, 0.0, -1.0, 1.0, null, null)


# ---- attack_distributed: the L2 random start does not depend on the world size ------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _fake_attack(net, imgs, eps, steps, *, target, random_start=False, seed=0, start_noise=None,
                 norm="linf", **kw):
    """Elementwise stand-in for pgd.attack in which the image, its target row, the norm and the
    start noise are all visible."""
    assert imgs.shape[0] >= 1
    from gfa_amd import pgd
    pgd.rescale_consensus(pgd.RUN_OK, kw.get("group"))
    assert random_start and start_noise is not None and start_noise.shape == imgs.shape
    if norm == "l2":  # each row is one image's point of the unit ball
        assert (start_noise.reshape(imgs.shape[0], -1).norm(dim=1) <= 1).all()
    return imgs * 0.5 + target.expand_as(imgs) * 0.25 + start_noise


def _worker(rank, world, port, n, norm, out_q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import gfa_import  # noqa: F401
    from gfa_amd import dist as gdist
    from gfa_amd import pgd
    pgd.attack = _fake_attack  # the distributed wrapper looks it up at call time
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        g = torch.Generator().manual_seed(3)
        imgs = torch.rand(n, 3, 4, 4, generator=g) * 2 - 1
        target = torch.rand(n, 3, 4, 4, generator=g) * 2 - 1
        net = types.SimpleNamespace(decoder=types.SimpleNamespace(device=torch.device("cpu")))
        got = gdist.attack_distributed(net, imgs, 0.5, 3, target=target, random_start=True,
                                       seed=11, norm=norm)
        noise = pgd.make_start_noise(tuple(imgs.shape), 11, norm)
        want = _fake_attack(net, imgs, 0.5, 3, target=target, random_start=True,
                            start_noise=noise, norm=norm)
        other = pgd.make_start_noise(tuple(imgs.shape), 11, "linf" if norm == "l2" else "l2")
        out_q.put((rank, torch.equal(got, want), not torch.equal(noise, other)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n,norm", [(1, 5, "l2"), (2, 5, "l2"), (3, 7, "l2"),
                                          (2, 5, "linf")])
def test_attack_distributed_l2_start_is_world_size_independent(world, n, norm):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n, norm, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert all(ok and differs for _, ok, differs in res), res
