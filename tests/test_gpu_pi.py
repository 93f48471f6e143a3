"""The patch-wise attack (PI-FGSM, Gao et al. 2020): the fused kernel mia_pi_update against its fp32
reference (tests/pi_ref.py) bit for bit — tile borders, a plane smaller than the window, the vector
and the scalar path, the order of the window sum, run-to-run bits, zero padding and plane
isolation — then the engine's step on captured inputs and the attack end to end at 32².

All image-space quantities are in [-1,1] units (e = 2·eps, a = 2·alpha)."""
import pytest
import torch

import pi_ref
from pi_ref import f32
from gpu_helpers import free, seeded
from test_gpu_di import offset_copy
from test_gpu_ti import ALPHA, EPS, SIZE, check_linf, images

pytestmark = pytest.mark.gpu

F32 = torch.float32
E = f32(2 * EPS)
_, AB, GM = pi_ref.steps(ALPHA, 10.0, 1.0)
NAMES = ("x", "x0", "g", "l1", "m", "A")


def bits(t):
    return t.contiguous().view(torch.int32)


def launch(c, mu, ab, gm, e, k, dev, offset=False):
    """mia_pi_update on device copies of the case ``c``; the outputs start NaN-filled and the
    inputs are checked to be unchanged. ``offset``: every image buffer 4 bytes off 16-byte
    alignment (the scalar path). Returns host (x, m_out, A_out, nonfinite)."""
    from gfa_amd import ops
    put = (lambda t: offset_copy(t.to(dev))) if offset else (lambda t: t.to(dev))
    d = {k_: (put(c[k_]) if k_ != "l1" else c[k_].to(dev)) for k_ in NAMES}
    keep = {k_: d[k_].clone() for k_ in NAMES if k_ != "x"}
    nan = torch.full_like(c["x"], float("nan"))
    m_out, A_out = put(nan), put(nan)                      # two device buffers (nan is on the host)
    nf = torch.zeros(c["x"].shape[0], dtype=torch.int32, device=dev)
    ops.pi_update(d["x"], d["x0"], d["g"], d["l1"], d["m"], m_out, d["A"], A_out, mu, ab, gm, e, k,
                  nonfinite=nf)
    for k_, v in keep.items():
        assert torch.equal(bits(d[k_]), bits(v)), k_ + " was written"
    return d["x"].cpu(), m_out.cpu(), A_out.cpu(), nf.cpu()


def same(got, want, what):
    for name, a, b in zip(("x", "m_out", "A_out"), got[:3], want[:3]):
        assert not torch.isnan(a).any(), (what, name, "an element was not written")
        assert torch.equal(bits(a), bits(b)), (what, name, int((bits(a) != bits(b)).sum()))
    assert got[3].tolist() == want[3].tolist(), (what, "nonfinite")


# (H, W, k): a plane smaller than the window; one row; a partial tile; odd sizes on the scalar
# path that cross tile borders both ways; the vector path on one tile and on 2 × 2 tiles
SHAPES = [(2, 2, 7), (1, 5, 3), (20, 20, 3), (67, 35, 5), (64, 64, 15), (68, 128, 15)]


@pytest.mark.parametrize("H,W,k", SHAPES)
def test_kernel_is_the_reference_bit_for_bit(cuda, H, W, k):
    """x, m_out, A_out and the flags on 3 images × 3 planes with per-image gradient scales, from an
    A with |A| on both sides of e in both signs and a non-zero m, μ ∈ {0, 1}. W % 4 == 0 runs the
    vector path and, from buffers 4 bytes off alignment, the scalar one: the same bits."""
    c = pi_ref.case(H, W, seed=H + W)
    q = pi_ref.parts(c["g"], c["l1"], c["m"], c["A"], 1.0, AB, E, k)
    assert (q["C"] > 0).any() and (q["C"] < 0).any() and (q["C"] == 0).any()
    if H * W >= 400:
        assert (q["S"] > 0).any() and (q["S"] < 0).any()
    for mu in (0.0, 1.0):
        want = pi_ref.update(c["x"], c["x0"], c["g"], c["l1"], c["m"], c["A"], mu, AB, GM, E, k)
        same(launch(c, mu, AB, GM, E, k, cuda), want, (H, W, k, mu))
        if W % 4 == 0:
            same(launch(c, mu, AB, GM, E, k, cuda, offset=True), want, (H, W, k, mu, "scalar"))
    # γ = 0: no projection, the MI rule with a = ab
    got = launch(c, 1.0, AB, 0.0, E, k, cuda)
    xm, mm = pi_ref.mi_update(c["x"], c["x0"], c["g"], c["l1"], c["m"], 1.0, AB, E)
    assert torch.equal(bits(got[0]), bits(xm)) and torch.equal(bits(got[1]), bits(mm))


def test_every_kernel_size_and_the_flags(cuda):
    """k = 3 … 15 on one odd-sized two-tile plane; a non-finite gradient element and a zero l1
    flag their images and leave A finite (s ∈ {−1, 0, 1})."""
    c = pi_ref.case(9, 70, seed=1)
    for k in (3, 5, 7, 9, 11, 13, 15):
        want = pi_ref.update(c["x"], c["x0"], c["g"], c["l1"], c["m"], c["A"], 1.0, AB, GM, E, k)
        same(launch(c, 1.0, AB, GM, E, k, cuda), want, k)
    bad = dict(c)
    bad["g"] = c["g"].clone()
    bad["g"][1, 2, 8, 69] = float("inf")
    bad["l1"] = c["l1"].clone()
    bad["l1"][2] = 0.0
    want = pi_ref.update(bad["x"], bad["x0"], bad["g"], bad["l1"], bad["m"], bad["A"], 0.0, AB, GM, E, 5)
    got = launch(bad, 0.0, AB, GM, E, 5, cuda)
    assert got[3].tolist() == want[3].tolist() == [0, 1, 1]
    assert torch.isfinite(got[2]).all() and torch.equal(bits(got[2]), bits(want[2]))
    assert torch.equal(bits(got[0]), bits(want[0]))


def test_the_summation_order_is_the_contract(cuda):
    """The crafted plane of pi_ref.order_case: overflow values of both signs with magnitudes 2^24
    apart. On the CPU the contract order and the reversed one must differ in the sign of S
    somewhere, and so in x and A; the kernel equals the contract order everywhere."""
    inp, c = pi_ref.order_case()
    args = (c["mu"], c["ab"], c["gm"], c["e"], c["k"])
    fwd = pi_ref.parts(inp["g"], inp["l1"], inp["m"], inp["A"], c["mu"], c["ab"], c["e"], c["k"])
    rev = pi_ref.parts(inp["g"], inp["l1"], inp["m"], inp["A"], c["mu"], c["ab"], c["e"], c["k"],
                       reverse=True)
    differ = pi_ref.sign(fwd["S"]) != pi_ref.sign(rev["S"])
    assert int(differ.sum()) >= 1
    want = pi_ref.update(inp["x"], inp["x0"], inp["g"], inp["l1"], inp["m"], inp["A"], *args)
    other = pi_ref.update(inp["x"], inp["x0"], inp["g"], inp["l1"], inp["m"], inp["A"], *args,
                          reverse=True)
    assert (want[2] != other[2])[differ].all() and not torch.equal(want[0], other[0])
    same(launch(inp, *args, cuda), want, "order")
    same(launch(inp, *args, cuda, offset=True), want, "order, scalar")


def test_chained_steps_rerun_to_the_same_bits(cuda):
    """Six chained steps on (67, 35, k = 5) with the buffers swapped after each, twice from the
    same start: equal bits run to run (an in-place m / A would race between tiles), and the
    reference's."""
    from gfa_amd import ops
    c = pi_ref.case(67, 35, seed=9)
    gs = [seeded(7300 + i, c["g"].shape) * torch.tensor(pi_ref.IMG_SCALES).reshape(3, 1, 1, 1)
          for i in range(6)]

    def run():
        x, x0 = c["x"].to(cuda), c["x0"].to(cuda)
        m = [c["m"].to(cuda), torch.full_like(x, float("nan"))]
        A = [c["A"].to(cuda), torch.full_like(x, float("nan"))]
        for i, g in enumerate(gs):
            ops.pi_update(x, x0, g.to(cuda), pi_ref.l1_of(g).to(cuda), m[i % 2], m[(i + 1) % 2],
                          A[i % 2], A[(i + 1) % 2], 1.0, AB, GM, E, 5)
        return x.cpu(), m[0].cpu(), A[0].cpu()

    first, second = run(), run()
    for a, b in zip(first, second):
        assert torch.equal(bits(a), bits(b))
    x, m, A = c["x"], c["m"], c["A"]
    for g in gs:
        x, m, A, _ = pi_ref.update(x, c["x0"], g, pi_ref.l1_of(g), m, A, 1.0, AB, GM, E, 5)
    for a, b in zip(first, (x, m, A)):
        assert torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("k", [3, 5])
def test_zero_padding_and_plane_isolation(cuda, k):
    """Plane (0, 0) of 66 × 66 overflows only in its corner pixels (0, 0) and (65, 65), the latter
    in the last tile; plane (0, 1) and image 1 overflow everywhere. In plane (0, 0) only the
    corners' in-plane neighbours receive p ≠ 0 — not the corners themselves (the centre is left
    out) and nothing from over the plane's edge, the next plane or the next image."""
    H = W = 66
    r = k // 2
    c = pi_ref.case(H, W, seed=40 + k, n=2, c=2)
    c["m"] = torch.zeros_like(c["m"])
    c["g"] = -(c["g"].abs() + 1e-3 * torch.tensor(pi_ref.IMG_SCALES[:2]).reshape(2, 1, 1, 1))  # s = +1
    c["l1"] = pi_ref.l1_of(c["g"])
    A = torch.full_like(c["A"], 4.0 * E)                   # overflows everywhere …
    A[0, 0] = -AB                                          # … but here A' = 0
    A[0, 0, 0, 0] = A[0, 0, H - 1, W - 1] = 2.0 * E
    c["A"] = A
    x, m_out, A_out, nf = launch(c, 0.0, AB, GM, E, k, cuda)
    same((x, m_out, A_out, nf), pi_ref.update(c["x"], c["x0"], c["g"], c["l1"], c["m"], c["A"], 0.0,
                                              AB, GM, E, k), k)
    Ap = pi_ref.parts(c["g"], c["l1"], c["m"], c["A"], 0.0, AB, E, k)["Ap"]
    moved = bits(A_out) != bits(Ap)                        # p ≠ 0
    want = torch.zeros(H, W, dtype=torch.bool)
    want[:r + 1, :r + 1] = True
    want[H - r - 1:, W - r - 1:] = True
    want[0, 0] = want[H - 1, W - 1] = False
    assert torch.equal(moved[0, 0], want), int((moved[0, 0] != want).sum())
    assert int(want.sum()) == 2 * ((r + 1) ** 2 - 1)
    assert moved[0, 1].all() and moved[1].all()


# ---- the engine and the attack at 32² ---------------------------------------------------------------
@pytest.fixture(scope="module")
def net32(cuda):
    from gfa_amd import networks
    return networks.build_net(SIZE, seed=0, dtype=torch.float32, device=cuda)


@pytest.mark.parametrize("momentum", [0.0, 1.0])
def test_engine_steps_are_the_reference_on_captured_inputs(cuda, net32, monkeypatch, momentum):
    """run_pi at 32², two images, 4 steps, k = 3, β = 10: what ops.pi_update was given at every
    step is captured, the reference is applied to it, and x, m, A after every step must be the
    reference's bits. The state really ping-pongs (step k's m_in / A_in are step k − 1's outputs,
    A starts at 0), and at the end the iterate is inside the ball and the range with the
    objective below L(x0) for both images."""
    from gfa_amd import ops
    from gfa_amd.pgd import AttackEngine
    x0, t = images()
    calls = []
    real = ops.pi_update

    def spy(x, x0_, g, l1, m_in, m_out, A_in, A_out, mu, ab, gm, e, kernel, *a, **kw):
        before = dict(x=x.cpu(), x0=x0_.cpu(), g=g.cpu(), l1=l1.cpu(), m=m_in.cpu(), A=A_in.cpu())
        out = real(x, x0_, g, l1, m_in, m_out, A_in, A_out, mu, ab, gm, e, kernel, *a, **kw)
        calls.append((before, (mu, ab, gm, e, kernel), (x.cpu(), m_out.cpu(), A_out.cpu()),
                      (m_in.data_ptr(), m_out.data_ptr(), A_in.data_ptr(), A_out.data_ptr())))
        return out
    monkeypatch.setattr(ops, "pi_update", spy)
    eng = AttackEngine(net32.encoder.impl, net32.decoder.impl, net32.vgg.impl)
    adv = eng.run_pi(x0.to(cuda), t.to(cuda), 4, EPS, ALPHA, 10.0, 3, 1.0, momentum=momentum)
    assert len(calls) == 4 and not eng.overflowed()
    assert not calls[0][0]["A"].any() and not calls[0][0]["m"].any()
    assert torch.equal(calls[0][0]["x"], x0)
    for i, (before, sc, after, ptrs) in enumerate(calls):
        assert sc == (f32(momentum), AB, GM, E, 3)
        assert torch.equal(before["x0"], x0)
        want = pi_ref.update(before["x"], before["x0"], before["g"], before["l1"], before["m"],
                             before["A"], *sc)
        for name, a, b in zip(("x", "m", "A"), after, want):
            assert torch.equal(bits(a), bits(b)), (i, name)
        if i:
            prev = calls[i - 1]
            assert ptrs[0] == prev[3][1] and ptrs[2] == prev[3][3]      # in = the last out
            assert ptrs[1] == prev[3][0] and ptrs[3] == prev[3][2]      # out = the last in
            assert torch.equal(bits(before["m"]), bits(prev[2][1]))
            assert torch.equal(bits(before["A"]), bits(prev[2][2]))
            assert torch.equal(bits(before["x"]), bits(prev[2][0]))
    assert (calls[-1][2][2].abs() > E).any()                            # β = 10 leaves the ball
    assert torch.equal(adv.cpu(), calls[-1][2][0])
    check_linf(adv.cpu(), x0, E)
    l_adv, l_0 = eng.loss(adv), eng.loss(x0.to(cuda))
    print(f"PI engine μ={momentum}: L(x0) {l_0.tolist()} -> L(adv) {l_adv.tolist()}")
    assert (l_adv < l_0).all()
    del eng


@pytest.mark.parametrize("momentum", [0.0, 1.0])
def test_attack_identities(cuda, net32, momentum):
    """Through attack(), bit for bit: pi_project = 0 is the MI attack at the alpha whose fp32 step
    is ab; β = 1 with steps·alpha ≤ eps never leaves the ball and is today's MI attack. And the
    keyword off leaves attack() as it was, with the three info entries None."""
    from gfa_amd import attack
    x0, t = images()
    kw = dict(target=t, momentum=momentum)
    alpha_ab = AB / 2.0                                   # fp32(2·alpha_ab) == ab
    assert f32(2.0 * alpha_ab) == AB
    adv, info = attack(net32, x0, EPS, 3, alpha=ALPHA, pi_amplification=10.0, pi_project=0.0,
                       return_info=True, **kw)
    assert (info["pi_amplification"], info["pi_kernel"], info["pi_project"]) == (10.0, 3, 0.0)
    assert torch.equal(bits(adv), bits(attack(net32, x0, EPS, 3, alpha=alpha_ab, **kw)))
    assert 3 * ALPHA <= EPS
    plain, info = attack(net32, x0, EPS, 3, alpha=ALPHA, return_info=True, **kw)
    assert (info["pi_amplification"], info["pi_kernel"], info["pi_project"]) == (None, None, None)
    for k in (3, 7):
        assert torch.equal(bits(attack(net32, x0, EPS, 3, alpha=ALPHA, pi_amplification=1.0,
                                       pi_kernel=k, **kw)), bits(plain))
    # the projection acts as soon as the ball is left
    assert not torch.equal(attack(net32, x0, EPS, 3, alpha=ALPHA, pi_amplification=10.0, **kw),
                           adv)


def test_attack_composes_and_rows_do_not_depend_on_the_batch(cuda, net32):
    """DI-TI-PI with momentum at 32² on 3 images, then each image alone: equal rows. fgsm()
    forwards the keyword."""
    from gfa_amd import attack, fgsm
    x0, t = images()
    x0 = torch.cat([x0, 0.8 * seeded(914, (1, 3, SIZE, SIZE))])
    t = torch.cat([t, seeded(915, (1, 3, SIZE, SIZE))])
    kw = dict(alpha=ALPHA, pi_amplification=10.0, ti_kernel=5, di_prob=0.5, momentum=1.0, seed=0)
    adv, info = attack(net32, x0, EPS, 4, target=t, return_info=True, **kw)
    assert info["pi_amplification"] == 10.0 and info["ti_kernel"] == 5 and info["di_prob"] == 0.5
    assert info["di_applied"] == 2 and info["rescales"] == 0   # seed 0 draws D at steps 0 and 3
    check_linf(adv, x0, E)
    for n in range(3):
        alone = attack(net32, x0[n:n + 1], EPS, 4, target=t[n:n + 1], **kw)
        assert torch.equal(bits(alone[0]), bits(adv[n])), n
    assert not torch.equal(adv, attack(net32, x0, EPS, 4, target=t, **{**kw, "pi_amplification": None}))
    more = attack(net32, x0[:2], EPS, 3, target=t[:2], alpha=ALPHA, pi_amplification=10.0, pi_kernel=5,
                  momentum=1.0, nesterov=True, si_scales=2, vt_samples=2, random_start=True, seed=3)
    check_linf(more, x0[:2], E)
    one = fgsm(net32, x0[:2], EPS, target=t[:2], pi_amplification=10.0)
    assert torch.equal(bits(one), bits(attack(net32, x0[:2], EPS, 1, target=t[:2], alpha=EPS,
                                              pi_amplification=10.0)))
    check_linf(one, x0[:2], E)


def test_attack_pi_fp16(cuda):
    """fp16 networks (loss scale 2^8; a re-run restarts from A = 0): finite images in the ball."""
    from gfa_amd import attack, networks
    net = networks.build_net(SIZE, seed=0, dtype=torch.float16, device=cuda)
    x0, t = images()
    adv, info = attack(net, x0, EPS, 3, target=t, alpha=ALPHA, pi_amplification=10.0, ti_kernel=5,
                       di_prob=0.5, momentum=1.0, return_info=True)
    assert torch.isfinite(adv).all() and info["dtype"] == "torch.float16"
    check_linf(adv, x0, E)
    assert not torch.equal(adv, x0)
    del net
    free()
