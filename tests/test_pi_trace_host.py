"""The launch sequence of AttackEngine.step_pi against step_mi's, on the host (no GPU), with the
recorder of tests/test_step_trace_host.py: for every combination of the options the patch-wise
step launches exactly what the momentum step launches, with the one mia_mi_update replaced by
exactly one mia_pi_update on the same x, x0, gradient and sum. With the keyword off nothing new is
launched: that is test_step_trace_host.py itself, whose fixture pins step_mi."""
import itertools

import pytest

import pi_ref
from test_step_trace_host import DI, MU, A, E, N, S, TI, VT, _Recorder, mi_cases


def _traces(ti, di, nes, si, vt, beta):
    from gfa_amd import pgd
    import torch
    a, e = pgd._f32(A), pgd._f32(E)
    out = []
    for use_pi in (False, True):
        with pytest.MonkeyPatch.context() as mp:
            r = _Recorder(mp)
            step_vt = None if VT[vt] is None else pgd.VtStep(*VT[vt])
            if use_pi:
                ws = r.eng.ws
                m1 = ws.get("mi.m1", (N, 3, S, S), torch.float32)
                a0 = ws.get("pi.a0", (N, 3, S, S), torch.float32)
                a1 = ws.get("pi.a1", (N, 3, S, S), torch.float32)
                ab, gm = pgd.pi_steps(A / 2, beta, 0.5)
                r.eng.step_pi(r.x, (r.m, m1), (a0, a1), MU, e, pgd.PiStep(ab, gm, 7), r.taps(ti),
                              DI[di], nes, si, step_vt)
            else:
                r.eng.step_mi(r.x, r.m, MU, a, e, r.taps(ti), DI[di], nes, si, step_vt)
            out.append(r.trace)
    return out


@pytest.mark.parametrize("key,case", list(mi_cases()))
def test_pi_replaces_the_update_launch_only(key, case):
    from gfa_amd import pgd
    mi, pi = _traces(*case, beta=1.0)                       # β = 1: ab = a, the same look-ahead c
    assert [l[0] for l in mi].count("mia_mi_update") == 1 and mi[-1][0] == "mia_mi_update"
    assert [l[0] for l in pi].count("mia_pi_update") == 1 and pi[-1][0] == "mia_pi_update"
    assert not any(l[0] == "mia_mi_update" for l in pi)
    assert pi[:-1] == mi[:-1], key
    u, p = mi[-1], pi[-1]
    # mia_mi_update: x, x0, g, l1, m, N, plane, mu, a, e, lo, hi, nonfinite, stream
    # mia_pi_update: x, x0, g, l1, m_in, m_out, A_in, A_out, N, C, H, W, K, mu, ab, gm, e, lo, hi, …
    a, e = pgd._f32(A), pgd._f32(E)
    assert p[1:5] == u[1:5] and p[5:9] == ["mi.m", "mi.m1", "pi.a0", "pi.a1"] and u[5] == "mi.m"
    assert p[9:14] == [N, 3, S, S, 7] and u[6:8] == [N, 3 * S * S]
    assert p[14:21] == [MU, a, pgd._f32(0.5 * a), e, -1.0, 1.0, "nonfinite"]
    assert u[8:14] == [MU, a, e, -1.0, 1.0, "nonfinite"]


def test_the_look_ahead_follows_the_amplified_step():
    """With nesterov the only launch argument β changes before the update is c = μ·ab."""
    from gfa_amd import pgd
    _, ab, _ = pi_ref.steps(A / 2, 10.0)
    for ti, di, si in itertools.product(TI, DI, (1, 3)):
        mi, pi = _traces(ti, di, True, si, "none", beta=10.0)
        assert len(mi) == len(pi)
        c_mi, c_pi = pgd._f32(pgd._f32(MU) * pgd._f32(A)), pgd._f32(pgd._f32(MU) * ab)
        assert c_mi != c_pi
        changed = 0
        for lm, lp in zip(mi[:-1], pi[:-1]):
            assert lm[0] == lp[0]
            if lm != lp:
                assert lm[0] == "mia_si_transform"
                assert [c_pi if v == c_mi else v for v in lm] == lp
                changed += 1
        assert changed == si
        # without it no launch reads c (the scale copies pass it along with m = None)
        off, on = _traces(ti, di, False, si, "none", beta=10.0)
        for lm, lp in zip(off[:-1], on[:-1]):
            assert lm == lp or (lm[0] == "mia_si_transform" and lm[2] is None
                                and [c_pi if v == c_mi else v for v in lm] == lp)
