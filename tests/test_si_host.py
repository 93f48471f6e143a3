"""Host side of the scale-invariant / Nesterov attacks (no GPU): the reference's identities,
attack()'s argument validation before any device work, the wrappers' host checks and the C ABI's
validation of mia_si_transform / mia_si_accumulate_norms."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import si_ref


# ---- the reference --------------------------------------------------------------------------------
def _x():
    g = torch.Generator().manual_seed(77)
    return torch.rand(2, 3, 5, 7, generator=g) * 2 - 1


def test_scale_copy_identities():
    """S_0 is the identity, S_i fixes −1 (black) and is affine with slope 2^-i; the fp32
    reference of the kernel agrees with the fp64 S_i to 2 roundings of values ≤ 2."""
    x = _x()
    assert torch.equal(si_ref.scale64(x, 0), x.double())
    assert torch.equal(si_ref.transform(x, None, 0.0, 1.0), x)
    black = torch.full((4,), -1.0)
    for i in range(8):
        s = 2.0 ** -i
        assert torch.equal(si_ref.scale64(black, i), black.double())
        assert torch.equal(si_ref.transform(black, None, 0.0, s), black)
        a, b = si_ref.scale64(x, i), si_ref.scale64(x + 0.25, i)
        assert torch.allclose(b - a, torch.full_like(a, 0.25 * s), rtol=0, atol=1e-15)
        mid = si_ref.scale64(0.5 * (x + x.flip(0)), i)
        assert torch.allclose(mid, 0.5 * (a + si_ref.scale64(x.flip(0), i)), rtol=0, atol=1e-15)
        err = (si_ref.transform(x, None, 0.0, s).double() - a).abs().max().item()
        assert err <= 2 * 2.0 ** -24 * 2.0, (i, err)
    # towards black, not towards mid-grey: a grey pixel (0) darkens, a black one stays
    assert si_ref.scale64(torch.zeros(1), 1).item() == -0.5


def test_reference_look_ahead_and_accumulate():
    x, m = _x(), _x().flip(1) * 3
    c = float(np.float32(2 * 2 / 255))
    t = si_ref.transform(x, m, c, 1.0)
    assert t.dtype == torch.float32
    assert torch.equal(t, x + m * torch.tensor(c))
    assert torch.equal(si_ref.transform(x, torch.zeros_like(x), c, 1.0), x)
    # three copies: the mean of 2^-i·g_i
    gs = [_x() * k for k in (1.0, 2.0, 4.0)]
    acc = si_ref.accumulate(gs[0], None, 1.0, True)
    assert torch.equal(acc, gs[0])
    acc = si_ref.accumulate(gs[1], acc, 0.5, False)
    acc = si_ref.accumulate(gs[2], acc, 0.25, False, 3.0)
    want = (gs[0].double() + 0.5 * gs[1].double() + 0.25 * gs[2].double()) / 3
    assert acc.dtype == torch.float32
    assert (acc.double() - want).abs().max().item() <= 3 * 2.0 ** -24 * want.abs().max().item()


# ---- attack(): every rejection happens before any device work ------------------------------------
class _StubDecoder:
    size = 32
    device = torch.device("cpu")


class _StubNet:
    decoder = _StubDecoder()
    vgg = object()


def test_si_validation_before_any_device_work():
    from gfa_amd import attack
    x = torch.zeros(2, 3, 32, 32)
    t = torch.zeros(1, 3, 32, 32)
    net = _StubNet()
    kw = dict(target=t, alpha=2 / 255)
    for bad in (0, 9, 2.0, True, -1, "5", np.float32(3)):
        with pytest.raises(ValueError, match="si_scales"):
            attack(net, x, 8 / 255, 2, si_scales=bad, **kw)
        with pytest.raises(ValueError, match="si_scales"):
            attack(net, x, 1.0, 2, target=t, alpha=0.2, norm="l2", si_scales=bad)
    for norm in ("adam", "l2_cw"):
        for n in (1, 5):
            with pytest.raises(ValueError, match="norm='linf' and 'l2'"):
                attack(net, x, None, 2, target=t, norm=norm, si_scales=n)
    with pytest.raises(ValueError, match="nesterov"):
        attack(net, x, 1.0, 2, target=t, alpha=0.2, norm="l2", nesterov=True)
    for norm in ("adam", "l2_cw"):
        with pytest.raises(ValueError, match="nesterov"):
            attack(net, x, None, 2, target=t, norm=norm, nesterov=True)
    for mu in (None, 0, 0.0):
        with pytest.raises(ValueError, match="nesterov"):
            attack(net, x, 8 / 255, 2, nesterov=True, momentum=mu, **kw)
        with pytest.raises(ValueError, match="nesterov"):
            attack(net, x, 8 / 255, 2, nesterov=True, momentum=mu, si_scales=5, ti_kernel=15,
                   di_prob=0.5, **kw)
    for bad in (1, "yes", None, 1.0):
        with pytest.raises(ValueError, match="nesterov"):
            attack(net, x, 8 / 255, 2, nesterov=bad, momentum=1.0, **kw)
    # valid arguments get as far as the network bundle, which a stub is not
    for extra in (dict(si_scales=None), dict(si_scales=1), dict(si_scales=5), dict(si_scales=8),
                  dict(si_scales=np.int64(3)), dict(si_scales=5, momentum=1.0, nesterov=True),
                  dict(momentum=0.5, nesterov=True), dict(momentum=1.0, nesterov=np.bool_(True)),
                  dict(si_scales=5, momentum=1.0, nesterov=True, ti_kernel=15, di_prob=0.5),
                  dict(si_scales=2, nesterov=False)):
        with pytest.raises(ValueError, match="device network"):
            attack(net, x, 8 / 255, 2, **extra, **kw)
    with pytest.raises(ValueError, match="device network"):
        attack(net, x, 1.0, 2, target=t, alpha=0.2, norm="l2", si_scales=5, ti_kernel=15)


def test_signatures_and_distributed_docs():
    from gfa_amd import attack, fgsm, pgd
    from gfa_amd import dist as gdist
    from gfa_amd.pgd import AttackEngine
    assert pgd.SI_MAX_SCALES == 8
    p = inspect.signature(attack).parameters
    assert p["si_scales"].default is None and p["nesterov"].default is False
    for name in ("step_mi", "run_mi", "step_l2", "run_l2"):
        q = inspect.signature(getattr(AttackEngine, name)).parameters
        assert q["si_scales"].default == 1, name
        assert ("nesterov" in q) == name.endswith("_mi"), name
    assert list(inspect.signature(AttackEngine._step_gradient).parameters) == [
        "self", "x", "m", "c", "si_scales", "di", "taps", "l1", "l2sq"]
    assert any(q.kind is inspect.Parameter.VAR_KEYWORD
               for q in inspect.signature(fgsm).parameters.values())
    for kwd in ("si_scales", "nesterov", "world size"):
        assert kwd in gdist.attack_distributed.__doc__, kwd
    for word in ("black", "grey", "Lin et al", "per copy"):
        assert word in attack.__doc__, word
    for n in (0, 9, 2.0, True):
        with pytest.raises(ValueError, match="si_scales"):
            pgd._check_si_scales(n)
    assert pgd._check_si_scales(None) == 1 and pgd._check_si_scales(5) == 5


def test_ops_wrappers_reject_before_the_library_call():
    from gfa_amd import ops
    x = torch.zeros(2, 3, 8, 8)
    y = torch.zeros(2, 3, 8, 8)
    m = torch.zeros(2, 3, 8, 8)
    v = torch.zeros(2)
    for s in (0.0, 3.0, 0.75, 2.0, 2.0 ** -8, -0.5, float("nan"), True, "1"):
        with pytest.raises(ValueError):
            ops.si_transform(x, None, y, 0.0, s)
        with pytest.raises(ValueError):
            ops.si_accumulate_norms(x, y, v, v, s, True)
    for bad in ((x, None, x), (x, y, y), (x, None, y[:1]), (x.double(), None, y),
                (x, None, y.double()), (x, m[:1], y), (x, m.double(), y), (None, None, y)):
        with pytest.raises(ValueError):
            ops.si_transform(bad[0], bad[1], bad[2], 0.0, 1.0)
    for c in (float("inf"), float("nan"), "0", None):
        with pytest.raises(ValueError):
            ops.si_transform(x, m, y, c, 1.0)
    for g, acc in ((x, x), (x, y[:1]), (x.double(), y), (x, y.double()), (None, y)):
        with pytest.raises(ValueError):
            ops.si_accumulate_norms(g, acc, v, v, 1.0, True)
    with pytest.raises(ValueError):
        ops.si_accumulate_norms(x, y, torch.zeros(3), v, 1.0, True)
    with pytest.raises(ValueError):
        ops.si_accumulate_norms(x, y, v, v.double(), 1.0, True)
    with pytest.raises(ValueError):
        ops.si_accumulate_norms(x, y, v, v, 1.0, True, nonfinite=torch.zeros(2))  # not int32
    for div in (0.5, 0, float("inf"), float("nan"), "3", None):
        with pytest.raises(ValueError):
            ops.si_accumulate_norms(x, y, v, v, 1.0, True, div)
    with pytest.raises(ValueError, match="device tensor"):
        ops.si_transform(x, m, y, 0.1, 0.5)                      # valid arguments, host tensors
    with pytest.raises(ValueError, match="device tensor"):
        ops.si_accumulate_norms(x, y, v, v, 0.5, False, 3.0)


# ---- C ABI validation (returns before any launch: runs without a GPU) ---------------------------
@pytest.mark.parametrize("name", ["mia_si_transform", "mia_si_accumulate_norms"])
def test_abi_si_validation(name):
    from gfa_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    # never dereferenced: validation fails first. 2·3·32² floats = 24 KiB per buffer
    ok, ok2, ok3, null = P(1 << 20), P(2 << 20), P(3 << 20), P(None)
    plane = 3 * 32 * 32

    def bad(a=ok, b=ok2, m=null, N=2, plane=plane, c=0.0, s=0.5, div=1.0):
        if name == "mia_si_transform":
            rc = lib.mia_si_transform(a, m, b, N, plane, c, s, null)
        else:
            rc = lib.mia_si_accumulate_norms(a, b, ok3, ok3, N, plane, s, 0, div, null, null)
        msg = lib.mia_last_error_string().decode()
        assert rc == -1, (rc, N, plane, c, s, div)  # MIA_EINVAL
        assert name in msg and len(msg) > len(name) + 2, msg

    bad(a=null)
    bad(b=null)
    bad(b=ok)                                   # in place
    bad(b=P((1 << 20) + 4))                     # overlapping, shifted by one float
    bad(b=P((1 << 20) + 4 * (2 * plane - 1)))   # the last float of a
    bad(a=P((1 << 20) + 4096), b=ok)            # overlapping the other way round
    for s in (0.0, -0.5, 2.0, 3.0, 0.75, 2.0 ** -8, float("nan"), float("inf")):
        bad(s=s)
    for N in (0, -4, 1 << 16, 70000):
        bad(N=N)
    for pl in (0, -4, 1 << 31, 1 << 40):
        bad(plane=pl)
    if name == "mia_si_transform":
        bad(m=ok2)                              # the look-ahead buffer is the output
        bad(m=P((2 << 20) + 4 * (2 * plane - 1)))
        bad(c=float("inf"))
        bad(c=float("nan"))
    else:
        for div in (0.0, 0.5, -3.0, float("nan"), float("inf")):
            bad(div=div)
