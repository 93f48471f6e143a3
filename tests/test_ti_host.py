"""Host side of the translation-invariant attacks (no GPU): the Gaussian taps, attack()'s argument
validation before any device work, and the C ABI's validation of mia_ti_smooth_norms."""
import ctypes

import numpy as np
import pytest
import torch


# ---- the taps -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kernlen,nsig", [(1, 3.0), (3, 3.0), (15, 3.0), (15, 1.5), (63, 3.0),
                                          (7, 4.0)])
def test_taps_sum_to_one_and_are_symmetric(kernlen, nsig):
    from gfa_amd.pgd import ti_gaussian_taps
    w = ti_gaussian_taps(kernlen, nsig)
    assert w.dtype == torch.float64 and tuple(w.shape) == (kernlen,)
    assert abs(float(w.sum()) - 1.0) <= 1e-15
    assert torch.equal(w, w.flip(0))
    assert (w > 0).all() and int(w.argmax()) == kernlen // 2
    w32 = w.float()
    assert torch.equal(w32, w32.flip(0))


def test_taps_defaults_and_single_tap():
    from gfa_amd.pgd import ti_gaussian_taps
    assert ti_gaussian_taps(1).tolist() == [1.0]
    assert ti_gaussian_taps(1, 0.5).tolist() == [1.0]
    assert torch.equal(ti_gaussian_taps(), ti_gaussian_taps(15, 3.0))
    # k/Σk with k = exp(−x²/2) on linspace(−nsig, nsig, kernlen)
    x = np.linspace(-3.0, 3.0, 15)
    k = np.exp(-x * x / 2)
    np.testing.assert_allclose(ti_gaussian_taps(15, 3.0).numpy(), k / k.sum(), rtol=1e-15, atol=0)


@pytest.mark.parametrize("bad", [0, 2, 14, 65, -3, 15.0, "15", None, True])
def test_taps_reject_bad_lengths(bad):
    from gfa_amd.pgd import ti_gaussian_taps
    with pytest.raises(ValueError):
        ti_gaussian_taps(bad)


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf")])
def test_taps_reject_bad_nsig(bad):
    from gfa_amd.pgd import ti_gaussian_taps
    with pytest.raises(ValueError):
        ti_gaussian_taps(15, bad)


def test_taps_are_torchattacks_gkern():
    """torchattacks TIFGSM.gkern(15, 3): kern1d = norm.pdf(linspace(−3, 3, 15));
    outer(kern1d, kern1d) / its sum — exactly outer(taps, taps)."""
    st = pytest.importorskip("scipy.stats")
    from gfa_amd.pgd import ti_gaussian_taps
    for kernlen, nsig in ((15, 3), (7, 3), (5, 2)):
        kern1d = st.norm.pdf(np.linspace(-nsig, nsig, kernlen))
        raw = np.outer(kern1d, kern1d)
        gkern = raw / raw.sum()
        w = ti_gaussian_taps(kernlen, float(nsig)).numpy()
        np.testing.assert_allclose(np.outer(w, w), gkern, rtol=1e-14, atol=0)


# ---- attack(): every rejection happens before any device work ------------------------------------
class _StubDecoder:
    size = 32
    device = torch.device("cpu")


class _StubNet:
    decoder = _StubDecoder()
    vgg = object()


def test_ti_validation_before_any_device_work():
    from gfa_amd import attack
    x = torch.zeros(2, 3, 32, 32)
    t = torch.zeros(1, 3, 32, 32)
    net = _StubNet()
    kw = dict(target=t, alpha=2 / 255)
    for bad in (14, 0, 2, 64, 65, 101, -15):          # even or out of range
        with pytest.raises(ValueError, match="odd integer"):
            attack(net, x, 8 / 255, 2, ti_kernel=bad, **kw)
    for bad in (15.0, "15", 7.5, True, (15,)):        # not an integer
        with pytest.raises(ValueError, match="odd integer"):
            attack(net, x, 8 / 255, 2, ti_kernel=bad, **kw)
    for bad in (0.0, -3.0, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="ti_nsig"):
            attack(net, x, 8 / 255, 2, ti_kernel=15, ti_nsig=bad, **kw)
    for norm in ("adam", "l2_cw"):
        with pytest.raises(ValueError, match="norm='linf' and 'l2'"):
            attack(net, x, None, 2, target=t, norm=norm, ti_kernel=15)
    # valid TI arguments get as far as the network bundle, which a stub is not
    with pytest.raises(ValueError, match="device network"):
        attack(net, x, 8 / 255, 2, ti_kernel=15, **kw)
    with pytest.raises(ValueError, match="device network"):
        attack(net, x, 8 / 255, 2, ti_kernel=1, ti_nsig=0.5, momentum=1.0, **kw)
    with pytest.raises(ValueError, match="device network"):
        attack(net, x, 8 / 255, 2, ti_kernel=np.int64(63), **kw)
    with pytest.raises(ValueError, match="device network"):
        attack(net, x, 1.0, 2, target=t, alpha=0.2, norm="l2", ti_kernel=15)
    # momentum with L2 stays rejected, with or without TI
    with pytest.raises(ValueError, match="norm='linf' only"):
        attack(net, x, 1.0, 2, target=t, alpha=0.2, norm="l2", momentum=1.0, ti_kernel=15)


def test_engine_entry_points_take_ti_taps():
    import inspect

    from gfa_amd.pgd import AttackEngine
    for name in ("step_mi", "run_mi", "step_l2", "run_l2"):
        p = inspect.signature(getattr(AttackEngine, name)).parameters
        assert "ti_taps" in p and p["ti_taps"].default is None, name


def test_attack_distributed_forwards_ti_arguments():
    """attack_distributed passes every extra keyword on to attack()."""
    import inspect

    from gfa_amd import dist as gdist
    sig = inspect.signature(gdist.attack_distributed)
    assert any(p.kind is inspect.Parameter.VAR_KEYWORD for p in sig.parameters.values())
    assert "ti_kernel" in gdist.attack_distributed.__doc__


# ---- C ABI validation (returns before any launch: runs without a GPU) ---------------------------
def test_abi_ti_smooth_norms_validation():
    from gfa_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    ok, ok2, null = P(4096), P(8192), P(None)  # never dereferenced: validation fails first
    name = "mia_ti_smooth_norms"

    def bad(g=ok, gs=ok2, taps=ok, K=15, N=2, C=3, H=32, W=32):
        rc = getattr(lib, name)(g, gs, taps, K, ok, ok, N, C, H, W, null, null)
        msg = lib.mia_last_error_string().decode()
        assert rc == -1, (rc, K, N, C, H, W)  # MIA_EINVAL
        assert name in msg and len(msg) > len(name) + 2, msg

    bad(g=null)
    bad(gs=null)
    bad(taps=null)
    bad(gs=ok)                      # in place
    for K in (0, 2, 14, 64, 65, -1, -15):
        bad(K=K)
    for dim in ("N", "C", "H", "W"):
        bad(**{dim: 0})
        bad(**{dim: -4})
    bad(N=1 << 16)                  # grid rows
    bad(N=70000)
    bad(H=1 << 16, W=1 << 15)       # H·W = 2^31
    bad(C=2, H=1 << 15, W=1 << 15)  # C·H·W = 2^31
    bad(C=1 << 20, H=1 << 20, W=1 << 30)
    bad(C=(1 << 31) - 1, H=(1 << 31) - 1, W=(1 << 31) - 1)
