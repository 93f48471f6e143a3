"""Host side of the input-diversity attacks (no GPU): the fp64 reference's rational weights against
F.interpolate, the draw schedule, attack()'s argument validation before any device work, and the
C ABI's validation of mia_di_resize_pad / mia_di_resize_pad_bwd_norms."""
import ctypes
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import di_ref


# ---- the reference --------------------------------------------------------------------------------
@pytest.mark.parametrize("S,rnd,top,left", [(32, 29, 2, 1), (32, 28, 0, 3), (32, 31, 0, 0),
                                            (32, 16, 5, 9), (33, 29, 3, 1)])
def test_rmat_is_torch_bilinear_resize_and_pad(S, rnd, top, left):
    """Ry·x·Rxᵀ equals zero_pad(F.interpolate(x, (rnd, rnd), bilinear, align_corners=False)) in
    fp64 to ≤ 1e-12: the integer rule is PyTorch's source-coordinate rule."""
    x = torch.rand(2, 3, S, S, dtype=torch.float64, generator=torch.Generator().manual_seed(S + rnd))
    x = x * 2 - 1
    want = F.pad(F.interpolate(x, (rnd, rnd), mode="bilinear", align_corners=False),
                 (left, S - rnd - left, top, S - rnd - top))
    got = di_ref.resize_pad(x, rnd, top, left)
    err = (got - want).abs().max().item()
    print(f"rmat vs F.interpolate S={S} rnd={rnd}: max |err| = {err:.3e}")
    assert tuple(got.shape) == (2, 3, S, S) and err <= 1e-12
    # the adjoint helper is the transpose: <D u, v> = <u, Dᵀ v> in fp64
    v = torch.rand(2, 3, S, S, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    lhs = (got * v).sum().item()
    rhs = (x * di_ref.resize_pad_adjoint(v, rnd, top, left)).sum().item()
    assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), 1.0)


def test_rmat_rows_and_identity():
    R = di_ref.rmat(32, 29, 2)
    assert R.dtype == torch.float64 and tuple(R.shape) == (32, 32)
    assert not R[:2].any() and not R[31:].any()               # the padding rows
    assert torch.allclose(R[2:31].sum(1), torch.ones(29, dtype=torch.float64), atol=1e-15)
    assert (R >= 0).all() and ((R > 0).sum(1) <= 2).all()
    assert ((R > 0).sum(0) <= 2).all()                        # an input feeds at most 2 outputs
    assert torch.equal(di_ref.rmat(16, 16, 0), torch.eye(16, dtype=torch.float64))
    for bad in ((8, 0, 0), (8, 9, 0), (8, 7, 2), (8, 7, -1)):
        with pytest.raises(ValueError):
            di_ref.rmat(*bad)


# ---- the schedule ---------------------------------------------------------------------------------
@pytest.mark.parametrize("S,rate", [(32, 0.9), (256, 0.9), (33, 0.5), (8, 0.2)])
def test_schedule_shape_ranges_and_draws(S, rate):
    from gfa_amd.pgd import make_di_schedule
    steps = 200
    s = make_di_schedule(steps, S, rate, 0.5, seed=3)
    assert s.dtype == torch.int64 and tuple(s.shape) == (steps, 4) and s.device.type == "cpu"
    lo = int(S * rate)
    rnd, top, left, ap = s[:, 0], s[:, 1], s[:, 2], s[:, 3]
    assert (rnd >= lo).all() and (rnd <= S - 1).all()
    assert (top >= 0).all() and (top + rnd <= S - 1).all()
    assert (left >= 0).all() and (left + rnd <= S - 1).all()
    assert ((ap == 0) | (ap == 1)).all()
    assert 0 < int(ap.sum()) < steps                          # p = 0.5 over 200 steps
    if S - lo > 1:
        assert rnd.unique().numel() > 1
    assert not make_di_schedule(steps, S, rate, 0.0, seed=3)[:, 3].any()
    assert make_di_schedule(steps, S, rate, 1.0, seed=3)[:, 3].all()
    assert tuple(make_di_schedule(0, S, rate, 0.5).shape) == (0, 4)


def test_schedule_is_seeded_and_prefix_stable():
    """The same seed gives the same schedule, another seed another one, and a shorter schedule
    is a prefix of a longer one (four scalar draws per step, in the order rnd, top, left, apply).
    The geometry does not depend on diversity_prob, only the apply column does."""
    from gfa_amd.pgd import make_di_schedule
    a = make_di_schedule(40, 256, 0.9, 0.5, seed=7)
    assert torch.equal(a, make_di_schedule(40, 256, 0.9, 0.5, seed=7))
    assert not torch.equal(a, make_di_schedule(40, 256, 0.9, 0.5, seed=8))
    assert torch.equal(a[:13], make_di_schedule(13, 256, 0.9, 0.5, seed=7))
    assert torch.equal(a[:1], make_di_schedule(1, 256, 0.9, 0.5, seed=7))
    assert torch.equal(a[:, :3], make_di_schedule(40, 256, 0.9, 1.0, seed=7)[:, :3])
    assert torch.equal(make_di_schedule(5, 32), make_di_schedule(5, 32, 0.9, 0.5, 0))


def test_schedule_does_not_replay_the_start_noise_stream():
    """The schedule's generator is seeded with (seed + DI_SEED_OFFSET) mod 2^63, not with seed:
    drawing the same sequence from manual_seed(seed), make_start_noise's stream, differs."""
    from gfa_amd import pgd
    S, lo, steps = 256, int(256 * 0.9), 30
    assert pgd.DI_SEED_OFFSET % (1 << 63) != 0

    def draw(seed):
        g = torch.Generator().manual_seed(seed)
        rows = []
        for _ in range(steps):
            rnd = int(torch.randint(lo, S, (1,), generator=g))
            top = int(torch.randint(0, S - rnd, (1,), generator=g))
            left = int(torch.randint(0, S - rnd, (1,), generator=g))
            rows.append((rnd, top, left, int(float(torch.rand((1,), dtype=torch.float64,
                                                              generator=g)) < 0.5)))
        return torch.tensor(rows, dtype=torch.int64)

    s = pgd.make_di_schedule(steps, S, 0.9, 0.5, seed=11)
    assert not torch.equal(s, draw(11))
    assert torch.equal(s, draw((11 + pgd.DI_SEED_OFFSET) % (1 << 63)))   # the documented derivation


@pytest.mark.parametrize("rate", [1.0, 1.1, 2.0, 0.0, 0.01, -0.5, float("nan"), float("inf"),
                                  "0.9", None])
def test_schedule_rejects_bad_rates(rate):
    """int(32·rate) must lie in 1 … 31: rates ≥ 1 would change the networks' input size."""
    from gfa_amd.pgd import make_di_schedule
    with pytest.raises(ValueError, match="di_resize_rate"):
        make_di_schedule(4, 32, rate, 0.5)


@pytest.mark.parametrize("prob", [-0.1, 1.5, float("nan"), float("inf"), "x", None, True])
def test_schedule_rejects_bad_probabilities(prob):
    from gfa_amd.pgd import make_di_schedule
    with pytest.raises(ValueError, match="di_prob"):
        make_di_schedule(4, 32, 0.9, prob)


def test_schedule_rejects_bad_steps_and_sizes():
    from gfa_amd.pgd import make_di_schedule
    for steps in (-1, 2.5):
        with pytest.raises(ValueError, match="steps"):
            make_di_schedule(steps, 32)
    for size in (0, 1, -32, 32.0, True):
        with pytest.raises(ValueError, match="size"):
            make_di_schedule(4, size)
    assert make_di_schedule(3, 2, 0.5, 1.0).tolist() == [[1, 0, 0, 1]] * 3   # the smallest case


# ---- attack(): every rejection happens before any device work ------------------------------------
class _StubDecoder:
    size = 32
    device = torch.device("cpu")


class _StubNet:
    decoder = _StubDecoder()
    vgg = object()


def test_di_validation_before_any_device_work():
    from gfa_amd import attack
    x = torch.zeros(2, 3, 32, 32)
    t = torch.zeros(1, 3, 32, 32)
    net = _StubNet()
    kw = dict(target=t, alpha=2 / 255)
    for bad in (-0.1, 1.01, float("nan"), "0.5", True):
        with pytest.raises(ValueError, match="di_prob"):
            attack(net, x, 8 / 255, 2, di_prob=bad, **kw)
    for bad in (1.0, 1.1, 0.0, 0.03, -1.0, float("nan"), float("inf"), "0.9"):
        with pytest.raises(ValueError, match="di_resize_rate"):
            attack(net, x, 8 / 255, 2, di_prob=0.5, di_resize_rate=bad, **kw)
    for norm in ("adam", "l2_cw"):
        with pytest.raises(ValueError, match="norm='linf' and 'l2'"):
            attack(net, x, None, 2, target=t, norm=norm, di_prob=0.5)
        with pytest.raises(ValueError, match="norm='linf' and 'l2'"):
            attack(net, x, None, 2, target=t, norm=norm, di_schedule=[[29, 2, 1, 1]] * 2)
    # explicit schedules: the shape, the dtype and every row
    good = [[29, 2, 1, 1], [32, 0, 0, 0]]
    for bad in ([[29, 2, 1, 1]],                       # one row for two steps
                [[29, 2, 1]] * 2,                      # three columns
                [29, 2, 1, 1, 29, 2, 1, 1],            # flat
                torch.tensor(good, dtype=torch.float32),
                "schedule"):
        with pytest.raises(ValueError, match="di_schedule"):
            attack(net, x, 8 / 255, 2, di_schedule=bad, **kw)
    for row in ([0, 0, 0, 1], [33, 0, 0, 1], [29, 4, 1, 1], [29, 1, 4, 1], [29, -1, 0, 1],
                [29, 0, -1, 1], [29, 2, 1, 2], [29, 2, 1, -1], [-29, 2, 1, 1]):
        with pytest.raises(ValueError, match="di_schedule row 1"):
            attack(net, x, 8 / 255, 2, di_schedule=[good[0], row], **kw)
    # momentum with L2 stays rejected with DI
    with pytest.raises(ValueError, match="norm='linf' only"):
        attack(net, x, 1.0, 2, target=t, alpha=0.2, norm="l2", momentum=1.0, di_prob=0.5)
    # valid DI arguments get as far as the network bundle, which a stub is not
    for extra in (dict(di_prob=0.5), dict(di_prob=0), dict(di_prob=1, di_resize_rate=0.5),
                  dict(di_prob=np.float32(0.25), momentum=1.0),
                  dict(di_prob=0.5, ti_kernel=15), dict(di_schedule=good),
                  dict(di_schedule=torch.tensor(good, dtype=torch.int32), ti_kernel=7),
                  dict(di_schedule=np.array(good)), dict(di_prob=0.5, di_schedule=good)):
        with pytest.raises(ValueError, match="device network"):
            attack(net, x, 8 / 255, 2, **extra, **kw)
    with pytest.raises(ValueError, match="device network"):
        attack(net, x, 1.0, 2, target=t, alpha=0.2, norm="l2", di_prob=0.5)
    with pytest.raises(ValueError, match="device network"):
        attack(net, x, 8 / 255, 0, di_prob=0.5, **kw)         # no steps: an empty schedule


def test_engine_entry_points_take_di():
    from gfa_amd.pgd import AttackEngine
    for name in ("step_mi", "run_mi", "step_l2", "run_l2"):
        p = inspect.signature(getattr(AttackEngine, name)).parameters
        assert "di" in p and p["di"].default is None, name
        assert "ti_taps" in p and p["ti_taps"].default is None, name


def test_attack_signature_and_distributed_docs():
    from gfa_amd import attack
    from gfa_amd import dist as gdist
    p = inspect.signature(attack).parameters
    assert p["di_prob"].default is None and p["di_schedule"].default is None
    assert p["di_resize_rate"].default == 0.9
    sig = inspect.signature(gdist.attack_distributed)
    assert any(q.kind is inspect.Parameter.VAR_KEYWORD for q in sig.parameters.values())
    for kwd in ("di_prob", "di_resize_rate", "di_schedule"):
        assert kwd in gdist.attack_distributed.__doc__, kwd


def test_ops_wrappers_reject_before_the_library_call():
    """ops.di_resize_pad / di_resize_pad_bwd_norms validate shapes and geometry on the host."""
    from gfa_amd import ops
    x = torch.zeros(2, 3, 8, 8)
    y = torch.zeros(2, 3, 8, 8)
    v = torch.zeros(2)
    for fn in (ops.di_resize_pad, lambda a, b, *g: ops.di_resize_pad_bwd_norms(a, b, v, v, *g)):
        for rnd, top, left in ((0, 0, 0), (9, 0, 0), (7, 2, 0), (7, 0, 2), (7, -1, 0), (7, 0, -1),
                               (7.0, 0, 0), (7, True, 0), ("7", 0, 0)):
            with pytest.raises(ValueError):
                fn(x, y, rnd, top, left)
        with pytest.raises(ValueError):
            fn(x, x, 7, 0, 1)                                  # in place
        with pytest.raises(ValueError):
            fn(x, y[:1], 7, 0, 1)
        with pytest.raises(ValueError):
            fn(x.double(), y, 7, 0, 1)
        with pytest.raises(ValueError):
            fn(torch.zeros(2, 3, 8, 6), torch.zeros(2, 3, 8, 6), 5, 0, 0)
        with pytest.raises(ValueError):
            fn(None, y, 7, 0, 1)
    with pytest.raises(ValueError):
        ops.di_resize_pad_bwd_norms(x, y, torch.zeros(3), v, 7, 0, 1)
    with pytest.raises(ValueError):
        ops.di_resize_pad_bwd_norms(x, y, v, v.double(), 7, 0, 1)
    with pytest.raises(ValueError, match="device tensor"):
        ops.di_resize_pad(x, y, 7, 0, 1)                       # valid geometry, host tensors


# ---- C ABI validation (returns before any launch: runs without a GPU) ---------------------------
@pytest.mark.parametrize("name", ["mia_di_resize_pad", "mia_di_resize_pad_bwd_norms"])
def test_abi_di_validation(name):
    from gfa_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    # never dereferenced: validation fails first. 2·3·32² floats = 24 KiB per buffer
    ok, ok2, null = P(1 << 20), P(2 << 20), P(None)

    def bad(a=ok, b=ok2, N=2, C=3, S=32, rnd=29, top=2, left=1):
        if name == "mia_di_resize_pad":
            rc = lib.mia_di_resize_pad(a, b, N, C, S, rnd, top, left, null)
        else:
            rc = lib.mia_di_resize_pad_bwd_norms(a, b, ok, ok, N, C, S, rnd, top, left, null, null)
        msg = lib.mia_last_error_string().decode()
        assert rc == -1, (rc, N, C, S, rnd, top, left)  # MIA_EINVAL
        assert name in msg and len(msg) > len(name) + 2, msg

    bad(a=null)
    bad(b=null)
    bad(b=ok)                                   # in place
    bad(b=P((1 << 20) + 4))                     # overlapping, shifted by one float
    bad(b=P((1 << 20) + 4 * (2 * 3 * 32 * 32 - 1)))   # the last float of a
    bad(a=P((1 << 20) + 4096), b=ok)            # overlapping the other way round
    for rnd in (0, -1, 33, 1 << 20):
        bad(rnd=rnd, top=0, left=0)
    bad(top=4)                                  # top + rnd = 33
    bad(left=4)
    bad(top=-1)
    bad(left=-1)
    bad(top=(1 << 31) - 1)                      # top + rnd overflows an int
    bad(left=(1 << 31) - 1)
    for dim in ("N", "C", "S"):
        bad(**{dim: 0})
        bad(**{dim: -4})
    bad(N=1 << 16)                              # grid rows
    bad(N=70000)
    bad(C=2, S=1 << 15, rnd=100, top=0, left=0)     # C·S² = 2^31
    bad(C=1, S=46341, rnd=100, top=0, left=0)       # S² ≥ 2^31
    bad(C=1, S=1 << 16, rnd=100, top=0, left=0)     # S² = 2^32
    bad(C=(1 << 31) - 1, S=(1 << 31) - 1, rnd=1, top=0, left=0)
