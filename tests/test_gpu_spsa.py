"""SPSA, the score-based black-box attack: the fused kernels mia_spsa_probe and
mia_spsa_accumulate_norms against their fp32 references (tests/spsa_ref.py, bit for bit, the
counter-based directions included), the ordered per-image sums, the engine's estimate against the
fp64 oracle and against the device's own gradient, and the attack end to end at 32² (L∞ with and
without momentum, L2, fp16).

All image-space quantities are in [-1,1] units (e = 2·eps, a = 2·alpha, d = fp32(2·spsa_delta))."""
import math

import numpy as np
import pytest
import torch

import spsa_ref
from gpu_helpers import free, seeded, to64
from test_gpu_di import offset_copy
from test_gpu_ti import ALPHA, ALPHA_L2, EPS, EPS_L2, SIZE, check_linf, images

pytestmark = pytest.mark.gpu

F32 = torch.float32
U = 2.0 ** -24
IMG_SCALES = (1e4, 1.0, 1e-4)  # per-image scales: cross-image mixing cannot hide
# plane = 3·S²: 192 (one partial block), 3267 (no multiple of 4: the scalar form, a partial last
# group, 4 slots), 50700 (50 slots per image), 12288 (12 slots)
SIZES = (8, 33, 130, 64)
# The sums' longest addition chain, as the kernel is written: a thread owns one group of 4 elements
# per grid stride and the grid holds ceil(plane / 4 / 256) ≤ 1024 slots, so 1 addition per
# accumulator here (for Σr² an fma: r² enters unrounded, one rounding), + 2 (the 4 accumulators,
# pairwise) + 6 wave butterfly levels + 4 wave sums + the ordered finish over at most 50 slots
# (S = 130) = 63 additions of non-negative terms; × 3 margin: 3·63·2⁻²⁴ ≈ 1.13e-5.
SUM_TOL = 3 * 63 * U
assert SUM_TOL <= 2e-5
SEEDS = (5, (1 << 32) + 77)
D = float(np.float32(2 * 0.01))   # the probe radius of spsa_delta = 0.01
DELTA = 0.01
WIDE = 5e3                        # a clamp range that cuts into image 0 (scale 1e4) only


def f32(v):
    return float(np.float32(v))


def bits(t):
    return t.contiguous().view(torch.int32)


_inputs = {}


def case(S):
    """Per size, computed once and shared (CPU fp32): x with per-image scales, u in [-1,1] with
    entries at ±1 (the clamp acts), and the objective pairs (fp, fm) of three accumulations whose
    differences carry the per-image scales."""
    if S not in _inputs:
        sc = torch.tensor(IMG_SCALES, dtype=F32)
        u = seeded(800 + S, (3, 3, S, S))
        u[0, 0, 0, 0], u[1, 1, 2, 3], u[2, 2, S - 1, S - 1], u[1, 0, 0, 1] = 1.0, -1.0, 1.0, -1.0
        fm = [seeded(820 + S + i, (3,)) * 4 for i in range(3)]
        # |fp − fm| in [0.5, 1]·scale, either sign
        diff = [seeded(830 + S + i, (3,)) for i in range(3)]
        fp = [fm[i] + torch.sign(diff[i]) * (0.5 + 0.5 * diff[i].abs()) * sc for i in range(3)]
        _inputs[S] = dict(x=seeded(810 + S, (3, 3, S, S)) * sc.reshape(3, 1, 1, 1), u=u, fp=fp,
                          fm=fm)
    return _inputs[S]


def probe(x, d, seed, image0, step, sample, **kw):
    """(yp, ym) of mia_spsa_probe on a device tensor; both outputs start NaN-filled."""
    from gfa_amd import ops
    yp, ym = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
    return ops.spsa_probe(x, yp, ym, d, seed, image0, step, sample, **kw)


S_ACC = 25.0                      # s = 1/(2·0.02)
ACC_ARGS = (SEEDS[1], 10, 3)      # seed, image0, step of the accumulation tests


def accumulate3(S, dev, rows=slice(None), image0=ACC_ARGS[1], sums=True, start=None, off=False,
                fp=None, fm=None):
    """Three accumulations (first; a middle one; the last with div = 3) of mia_spsa_accumulate_norms
    on images of 3 × S × S with the objective pairs fp[i][rows], fm[i][rows] (default: case(S)'s):
    the acc after each, and (Σ|r|, Σr², nonfinite) of the last. acc starts NaN-filled (``off``: at
    a 4-byte offset, the scalar form)."""
    from gfa_amd import ops
    fp = case(S)["fp"] if fp is None else fp
    fm = case(S)["fm"] if fm is None else fm
    shape = (fp[0][rows].numel(), 3, S, S)
    acc = torch.full(shape, float("nan"), device=dev)
    if off:
        acc = offset_copy(acc)
    N = shape[0]
    s1 = torch.zeros(N, device=dev) if start is None else start.clone()
    s2 = torch.zeros(N, device=dev) if start is None else start.clone()
    nf = torch.zeros(N, dtype=torch.int32, device=dev)
    seed, _, step = ACC_ARGS
    after = []
    for i in range(3):
        last = i == 2
        ops.spsa_accumulate_norms(acc, fp[i][rows].contiguous().to(dev),
                                  fm[i][rows].contiguous().to(dev),
                                  s1 if last and sums else None, s2 if last and sums else None,
                                  S_ACC, seed, image0, step, i, i == 0, 3.0 if last else 1.0,
                                  nonfinite=nf)
        after.append(acc.clone())
    return after, s1, s2, nf


@pytest.mark.parametrize("S", SIZES)
def test_spsa_probe_is_the_reference_bit_for_bit(cuda, S):
    """yp and ym equal the fp32 reference, Philox directions included, for two seeds (one ≥ 2^32)
    and two (step, sample) pairs, on x in [-1,1] with entries at ±1 under the default clamp and on
    per-image scaled x under a clamp that cuts into image 0 alone; the outputs start NaN-filled;
    reruns are bit-identical; image 1 alone with image0 + 1 is row 1 of the batch; another seed,
    image0, step or sample changes the directions; the top image word image0 + N = 2^32."""
    c = case(S)
    for x_cpu, kw in ((c["u"], {}), (c["x"], dict(lo=-WIDE, hi=WIDE))):
        x = x_cpu.to(cuda)
        for seed in SEEDS:
            for step, sample in ((0, 0), (3, 2)):
                yp, ym = probe(x, D, seed, 10, step, sample, **kw)
                assert torch.isfinite(yp).all() and torch.isfinite(ym).all()
                wp, wm = spsa_ref.probe(x_cpu, D, seed, 10, step, sample, **kw)
                assert torch.equal(bits(yp.cpu()), bits(wp)), (seed, step, sample, kw)
                assert torch.equal(bits(ym.cpu()), bits(wm)), (seed, step, sample, kw)
                yp2, ym2 = probe(x, D, seed, 10, step, sample, **kw)
                assert torch.equal(bits(yp2), bits(yp)) and torch.equal(bits(ym2), bits(ym))
                ap, am = probe(x[1:2].contiguous(), D, seed, 11, step, sample, **kw)
                assert torch.equal(bits(ap[0]), bits(yp[1]))
                assert torch.equal(bits(am[0]), bits(ym[1]))
        lo, hi = kw.get("lo", -1.0), kw.get("hi", 1.0)
        assert yp.min() >= lo and yp.max() <= hi and ym.min() >= lo and ym.max() <= hi
    u = c["u"].to(cuda)
    yp, ym = probe(u, D, 5, 0, 0, 0)
    # the clamp acted: at x = ±1 one probe stays at ±1, the other steps inside by d
    for idx, edge in (((0, 0, 0, 0), 1.0), ((1, 1, 2, 3), -1.0)):
        inside = f32(np.float32(edge) * (np.float32(1) - np.float32(D)))
        assert {float(yp[idx]), float(ym[idx])} == {edge, inside}
    inner = (c["u"].abs() < 0.9).to(cuda)
    assert ((yp - ym).abs()[inner] > 0).all()
    for other in (probe(u, D, 6, 0, 0, 0), probe(u, D, 5, 1, 0, 0), probe(u, D, 5, 0, 1, 0),
                  probe(u, D, 5, 0, 0, 1)):
        assert not torch.equal(other[0][0], yp[0])
    top = probe(u, D, 5, (1 << 32) - 3, 0, 0)
    want = spsa_ref.probe(c["u"], D, 5, (1 << 32) - 3, 0, 0)
    assert torch.equal(bits(top[0].cpu()), bits(want[0]))
    assert torch.equal(bits(top[1].cpu()), bits(want[1]))


@pytest.mark.parametrize("S", SIZES)
def test_spsa_accumulate_is_the_reference_and_sums(cuda, S):
    """acc equals the fp32 reference bit for bit after each of 3 accumulations (first, a middle
    one, the last with div = 3); each image's Σ|r| and Σr² equal the fp64 sums of the device acc to
    SUM_TOL relative (the chain is counted above); the sums accumulate (+=) and may be absent;
    reruns are bit-identical and an image's results do not depend on the other images."""
    c = case(S)
    after, s1, s2, nf = accumulate3(S, cuda)
    want = torch.zeros(3, 3, S, S)
    seed, image0, step = ACC_ARGS
    for i in range(3):
        want = spsa_ref.accumulate(want, c["fp"][i], c["fm"][i], S_ACC, seed, image0, step, i,
                                   i == 0, 3.0 if i == 2 else 1.0)
        assert torch.equal(bits(after[i].cpu()), bits(want)), i
    assert not nf.any()
    acc = after[2]
    a64 = acc.double().reshape(3, -1)
    e1 = ((s1.double() - a64.abs().sum(1)).abs() / a64.abs().sum(1)).cpu()
    e2 = ((s2.double() - (a64 * a64).sum(1)).abs() / (a64 * a64).sum(1)).cpu()
    print(f"spsa sums S={S}: rel err of sum|r| {e1.tolist()}, of sum r^2 {e2.tolist()} "
          f"(bound {SUM_TOL:.2e})")
    assert e1.max() <= SUM_TOL and e2.max() <= SUM_TOL
    assert s1[0] > 1e3 * s1[1] > 1e6 * s1[2] > 0  # the per-image scales arrived
    after_b, s1_b, s2_b, _ = accumulate3(S, cuda)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(after, after_b))
    assert torch.equal(s1_b, s1) and torch.equal(s2_b, s2)
    after_1, s1_1, s2_1, _ = accumulate3(S, cuda, rows=slice(1, 2), image0=image0 + 1)
    assert torch.equal(bits(after_1[2][0]), bits(acc[1]))
    assert torch.equal(s1_1[0], s1[1]) and torch.equal(s2_1[0], s2[1])
    after_n, s1_n, s2_n, _ = accumulate3(S, cuda, sums=False)
    assert torch.equal(bits(after_n[2]), bits(acc)) and not s1_n.any() and not s2_n.any()
    _, s1_a, s2_a, _ = accumulate3(S, cuda, start=torch.ones(3, device=cuda))
    assert torch.equal(s1_a, 1.0 + s1) and torch.equal(s2_a, 1.0 + s2)


@pytest.mark.parametrize("S", [8, 130, 64])
def test_spsa_vector_and_scalar_paths_agree(cuda, S):
    """plane % 4 == 0 on 16-byte aligned buffers moves 16-byte vectors; the same data at a 4-byte
    offset takes the scalar form. The bits, the sums included, are the same."""
    from gfa_amd import ops
    c = case(S)
    x = c["u"].to(cuda)
    assert x.data_ptr() % 16 == 0
    args = (D, SEEDS[1], 4, 3, 2)
    yp, ym = probe(x, *args)
    for alt in probe(offset_copy(x), *args), \
            ops.spsa_probe(x, offset_copy(torch.zeros_like(x)), torch.zeros_like(x), *args), \
            ops.spsa_probe(x, torch.zeros_like(x), offset_copy(torch.zeros_like(x)), *args):
        assert torch.equal(bits(alt[0]), bits(yp)) and torch.equal(bits(alt[1]), bits(ym))
    after, s1, s2, _ = accumulate3(S, cuda)
    assert after[2].data_ptr() % 16 == 0
    after_o, s1_o, s2_o, _ = accumulate3(S, cuda, off=True)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(after, after_o))
    assert torch.equal(s1_o, s1) and torch.equal(s2_o, s2)


def test_spsa_accumulate_flags_nonfinite(cuda):
    """A non-finite objective reaches every r of its image through c: fp[1] = inf and fm[0] = nan
    flag exactly those images; the others stay finite, sums included."""
    c = case(33)
    fp = [t.clone() for t in c["fp"]]
    fp[1][1] = float("inf")
    after, s1, s2, nf = accumulate3(33, cuda, fp=fp)
    assert nf.tolist() == [0, 1, 0]
    assert torch.isfinite(after[2][0]).all() and torch.isfinite(after[2][2]).all()
    assert not torch.isfinite(after[2][1]).any()
    assert torch.isfinite(s1[0]) and torch.isfinite(s1[2]) and torch.isfinite(s2[0])
    fm = [t.clone() for t in c["fm"]]
    fm[0][0] = float("nan")
    after, s1, s2, nf = accumulate3(33, cuda, fm=fm)
    assert nf.tolist() == [1, 0, 0]
    assert torch.isfinite(after[2][1:]).all() and torch.isfinite(s1[1:]).all()
    fm[2][2] = float("inf")                                  # on the last accumulation only
    _, _, _, nf = accumulate3(33, cuda, fm=fm)
    assert nf.tolist() == [1, 0, 1]


def test_spsa_wrappers_reject_malformed_calls(cuda):
    from gfa_amd import ops
    x = torch.zeros(2, 3, 8, 8, device=cuda)
    yp, ym = torch.zeros_like(x), torch.zeros_like(x)
    fp, fm, l1 = (torch.zeros(2, device=cuda) for _ in range(3))
    pr = lambda a, b, c, d=0.02, image0=0: ops.spsa_probe(a, b, c, d, 5, image0, 0, 0)   # noqa: E731
    ac = lambda a, p, m, s=25.0, div=1.0, image0=0, **k: ops.spsa_accumulate_norms(      # noqa: E731
        a, p, m, l1, None, s, 5, image0, 0, 0, True, div, **k)
    for bad in ((x, x, ym), (x, yp, x), (x, yp, yp), (x, yp[:1], ym), (x, yp, ym[:1]),
                (x.double(), yp.double(), ym.double()), (x.cpu(), yp, ym), (x, yp.cpu(), ym),
                (x, yp, ym.cpu())):
        with pytest.raises(ValueError):
            pr(*bad)
    # overlapping views of one buffer: the library's own check (MIA_EINVAL)
    flat = torch.zeros(2 * 3 * 8 * 8 + 4, device=cuda)
    a, b = flat[:-4].view(2, 3, 8, 8), flat[4:].view(2, 3, 8, 8)
    for bad in ((a, b, ym), (a, yp, b), (x, a, b)):
        with pytest.raises(Exception, match="distinct"):
            pr(*bad)
    for d in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            pr(x, yp, ym, d=d)
    with pytest.raises(ValueError):
        pr(x, yp, ym, image0=(1 << 32) - 1)
    with pytest.raises(ValueError):
        ops.spsa_probe(x, yp, ym, 0.02, 5, 0, 0, 0, lo=1.0, hi=-1.0)
    for bad in ((x, fp, fp), (x, fp[:1], fm), (x, fp, fm.double()), (x.double(), fp, fm),
                (x.cpu(), fp, fm), (x, fp.cpu(), fm), (x, fp, fm.cpu()), (None, fp, fm)):
        with pytest.raises(ValueError):
            ac(*bad)
    f2 = torch.zeros(3, device=cuda)
    with pytest.raises(Exception, match="distinct"):
        ac(x, f2[:2], f2[1:])                                    # fm overlaps fp
    with pytest.raises(Exception, match="distinct"):
        ac(x, x.view(-1)[5:7], fm)                               # fp inside acc
    for s in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ac(x, fp, fm, s=s)
    for div in (0.0, -3.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ac(x, fp, fm, div=div)
    with pytest.raises(ValueError):
        ac(x, fp, fm, image0=(1 << 32) - 1)
    with pytest.raises(ValueError):
        ops.spsa_accumulate_norms(x, fp, fm, torch.zeros(3, device=cuda), None, 25.0, 5, 0, 0, 0,
                                  True)
    with pytest.raises(ValueError):
        ac(x, fp, fm, nonfinite=torch.zeros(2, device=cuda))     # not int32


# ---- the engine's estimate -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net32(cuda):
    from gfa_amd import networks
    return networks.build_net(SIZE, seed=0, dtype=torch.float32, device=cuda)


def engine32(net, cuda):
    from gfa_amd.pgd import AttackEngine
    x0, t = images()
    eng = AttackEngine(net.encoder.impl, net.decoder.impl, net.vgg.impl)
    eng.prepare(x0.to(cuda), t.to(cuda))
    return eng


KEY = 5 + 0x535053412D41544B      # (seed 5 + SPSA_SEED_OFFSET) mod 2^64
_oracle = {}


def oracle_objective():
    """The fp64 networks of build_net(32, seed=0) with the targets of x0 and t, as a function
    x ↦ the per-image objective (fp64 [N]) and x ↦ ∇L(x). Built once."""
    if "obj" not in _oracle:
        from gfa_amd.weights import make_encoder_weights, make_generator_weights, make_vgg_weights
        from oracle import attack_ref, vgg_ref
        p64 = to64((make_generator_weights(SIZE, seed=0),
                    vgg_ref.load_positional(make_vgg_weights(1234)),
                    make_encoder_weights(SIZE, seed=1)))
        x0, t = images()
        refs = attack_ref.Refs(*p64, x0.double(), t.double(), SIZE)
        _oracle["obj"] = lambda x: attack_ref.objective(*p64, x.double(), refs, SIZE,
                                                        per_image=True).detach()
        _oracle["grad"] = lambda x: attack_ref.loss_grad(*p64, x.double(), refs, SIZE)[1]
    return _oracle["obj"], _oracle["grad"]


def test_engine_estimate_vs_oracle(cuda, net32):
    """At x0 (N = 2, q = 2, spsa_delta = 0.01): the device's c_i[n], read back from a one-pair
    accumulation, against (f⁺ − f⁻)/(2d) of the fp64 oracle at the reference's probes (4 fp64
    evaluations): the same sign, and a relative error ≤ 1e-4·(|f⁺| + |f⁻|)/|f⁺ − f⁻| — the
    project's fp32 objective bound against this oracle (test_gpu_networks) times the difference's
    cancellation factor, which must stay ≤ 500 (asserted on the oracle alone; 125 / 169 for pair
    0 and 227 / 152 for pair 1 expected at spsa_delta = 0.01). The engine's two-pair estimate is
    then the reference's accumulation of the device's own c, bit for bit.
    Measured on an MI355X: relative errors 1.2e-5 / 1.1e-5 (pair 0) and 3.3e-5 / 5.3e-5 (pair 1)
    against bounds of 1.3e-2 … 2.3e-2."""
    from gfa_amd import ops, pgd
    from gfa_amd.pgd import SpsaStep
    assert pgd.SPSA_SEED_OFFSET + 5 == KEY and f32(2 * DELTA) == D
    x0, _ = images()
    obj, _ = oracle_objective()
    eng = engine32(net32, cuda)
    x = x0.to(cuda)
    s = pgd.spsa_scale(D)
    want_c, fac = [], []
    for i in range(2):
        yp, ym = spsa_ref.probe(x0, D, KEY, 0, 0, i)
        fp, fm = obj(yp), obj(ym)
        want_c.append((fp - fm) / (2.0 * D))
        fac.append((fp.abs() + fm.abs()) / (fp - fm).abs())
    print(f"SPSA oracle: c per pair {[c.tolist() for c in want_c]}; cancellation factors "
          f"{[f.tolist() for f in fac]} (cap 500)")
    assert max(f.max().item() for f in fac) <= 500
    ref = None
    for i in range(2):
        # one pair alone: ĝ = c·v, so c[n] = ĝ[n]·v[n] at any element
        yp, ym = probe(x, D, KEY, 0, 0, i)
        fp = eng.objective(yp, torch.zeros(2, device=cuda))
        fm = eng.objective(ym, torch.zeros(2, device=cuda))
        g1 = torch.full_like(x, float("nan"))
        ops.spsa_accumulate_norms(g1, fp, fm, None, None, s, KEY, 0, 0, i, True)
        v = spsa_ref.directions(tuple(x0.shape), KEY, 0, 0, i)
        c_dev = (g1.cpu() * v).reshape(2, -1)
        assert (c_dev == c_dev[:, :1]).all()
        c_dev = c_dev[:, 0].double()
        err = ((c_dev - want_c[i]).abs() / want_c[i].abs())
        print(f"SPSA engine pair {i}: device c {c_dev.tolist()}, rel err {err.tolist()}, bound "
              f"{(1e-4 * fac[i]).tolist()}")
        assert torch.equal(torch.sign(c_dev), torch.sign(want_c[i]))
        assert (err <= 1e-4 * fac[i]).all()
        ref = spsa_ref.accumulate(ref if ref is not None else torch.zeros_like(x0), fp.cpu(),
                                  fm.cpu(), s, KEY, 0, 0, i, i == 0, 2.0 if i == 1 else 1.0)
    sums = torch.zeros(2, 2, device=cuda)
    g = eng.spsa_gradient(x, SpsaStep(2, D, KEY, 0, 0), l1=sums[0], l2sq=sums[1])
    assert not eng.overflowed()
    assert torch.equal(bits(g.cpu()), bits(ref))
    r64 = ref.double().reshape(2, -1)
    assert torch.allclose(sums[0].double().cpu(), r64.abs().sum(1), rtol=SUM_TOL, atol=0)
    assert torch.allclose(sums[1].double().cpu(), (r64 * r64).sum(1), rtol=SUM_TOL, atol=0)
    del eng


def test_engine_estimate_vs_device_gradient(cuda, net32):
    """q = 64 at 32² (D = 3072 elements): cos(ĝ, ∇L) ≥ 0.5·√(q/(q + D − 1)) per image against the
    device's own full_gradient(x0) — half of the linear regime's expected cosine, a floor and not
    a measurement (0.0714; the fp64 oracle's estimate reaches 0.125 / 0.134). The cosine of the
    same directions on the objective linearised at x0 (fp64, the oracle's gradient) is printed
    next to it."""
    from gfa_amd.pgd import SpsaStep
    q, dim = 64, 3 * SIZE * SIZE
    x0, _ = images()
    _, grad = oracle_objective()
    eng = engine32(net32, cuda)
    x = x0.to(cuda)
    g = eng.spsa_gradient(x, SpsaStep(q, D, KEY, 0, 0)).clone()
    assert not eng.overflowed()
    gd = eng.full_gradient(x)
    cos = torch.nn.functional.cosine_similarity(g.double().reshape(2, -1),
                                                gd.double().reshape(2, -1), dim=1).cpu()
    g0 = grad(x0)
    lin = spsa_ref.estimate(lambda y: (g0 * (y - x0.double())).reshape(2, -1).sum(1), x0, q, D,
                            KEY, 0, 0)
    cl = torch.nn.functional.cosine_similarity(lin.reshape(2, -1), g0.reshape(2, -1), dim=1)
    floor = 0.5 * math.sqrt(q / (q + dim - 1))
    print(f"SPSA q={q}: cos(estimate, device gradient) {cos.tolist()}; linearised objective "
          f"(fp64) {cl.tolist()}; expected {math.sqrt(q / (q + dim - 1)):.4f}, floor {floor:.4f}")
    assert cos.min().item() >= floor
    del eng


# ---- end to end at 32² ----------------------------------------------------------------------------
Q, STEPS = 16, 3


def check_spsa_attack(net, name, norm, momentum):
    from gfa_amd import attack
    x0, t = images()
    keep = x0.clone()
    l2 = norm == "l2"
    eps, alpha = (EPS_L2, ALPHA_L2) if l2 else (EPS, ALPHA)
    e = f32(2 * eps)
    kw = dict(target=t, alpha=alpha, norm=norm, momentum=momentum, spsa_samples=Q, seed=5)
    adv, info = attack(net, x0, eps, STEPS, return_info=True, **kw)
    assert torch.equal(x0, keep)
    assert info["spsa_samples"] == Q and info["spsa_delta"] == 0.01
    assert info["queries"] == 2 * Q * STEPS and info["norm"] == norm
    assert info["momentum"] == momentum and info["rescales"] == 0
    if l2:
        nrm = (adv.double() - x0.double()).reshape(2, -1).norm(dim=1)
        assert (nrm <= e * (1 + 1e-5)).all() and (nrm > 0).all()
        assert adv.min() >= -1 and adv.max() <= 1
    else:
        check_linf(adv, x0, e)
        assert not torch.equal(adv, x0)
    assert torch.equal(adv, attack(net, x0, eps, STEPS, **kw))
    alone = attack(net, x0[1:2], eps, STEPS, **{**kw, "target": t[1:2]}, spsa_first_image=1)
    assert torch.equal(alone[0], adv[1])
    alone = attack(net, x0[:1], eps, STEPS, **{**kw, "target": t[:1]})
    assert torch.equal(alone[0], adv[0])
    others = dict(seed=attack(net, x0, eps, STEPS, **{**kw, "seed": 6}),
                  q=attack(net, x0, eps, STEPS, **{**kw, "spsa_samples": Q // 2}),
                  delta=attack(net, x0, eps, STEPS, spsa_delta=0.02, **kw))
    diff = {k: (adv != o).float().mean().item() for k, o in others.items()}
    print(f"SPSA {name}: share of pixels that differ with another seed {diff['seed']:.4f}, with "
          f"q = {Q // 2} {diff['q']:.4f}, with spsa_delta = 0.02 {diff['delta']:.4f}")
    assert all(d > 0 for d in diff.values())
    return info


@pytest.mark.parametrize("name,norm,momentum", [("linf", "linf", None), ("linf-mi", "linf", 1.0),
                                                ("l2", "l2", None)])
def test_attack_spsa(cuda, net32, name, norm, momentum):
    check_spsa_attack(net32, name, norm, momentum)


def test_attack_without_spsa_is_unchanged(cuda, net32):
    """spsa_samples = None runs today's paths: the bits of the attack without the keyword, and
    info reports no queries. fgsm(spsa_samples=q) is the one-step attack."""
    from gfa_amd import attack, fgsm
    x0, t = images()
    for kw in (dict(alpha=ALPHA), dict(alpha=ALPHA, momentum=1.0),
               dict(alpha=ALPHA_L2, norm="l2")):
        eps = EPS_L2 if kw.get("norm") == "l2" else EPS
        plain = attack(net32, x0, eps, 2, target=t, **kw)
        adv, info = attack(net32, x0, eps, 2, target=t, spsa_samples=None, spsa_delta=0.02,
                           spsa_first_image=3, return_info=True, **kw)
        assert torch.equal(adv, plain)
        assert info["spsa_samples"] is None and info["spsa_delta"] is None
        assert info["queries"] == 0
    one = fgsm(net32, x0, EPS, target=t, spsa_samples=4, seed=5)
    assert torch.equal(one, attack(net32, x0, EPS, 1, target=t, alpha=EPS, spsa_samples=4, seed=5))
    check_linf(one, x0, f32(2 * EPS))
    assert not torch.equal(one, x0)


Q_DEC, STEPS_DEC = 16, 10


DEC_RULES = {"linf": (EPS, dict(alpha=ALPHA, momentum=None)),
             "linf-mi": (EPS, dict(alpha=ALPHA, momentum=1.0)),
             "l2": (EPS_L2, dict(alpha=ALPHA_L2, norm="l2"))}


@pytest.mark.parametrize("name", list(DEC_RULES))
def test_attack_spsa_decreases_the_objective(cuda, net32, name):
    """steps = 10, q = 16: the black-box attack lowers the objective of every image
    (eng.loss(adv) < eng.loss(x0)) for L∞ (eps = 8/255, alpha = 2/255) with momentum None and 1.0
    and for L2 (eps = 1.0, alpha = 0.2), reading 320 objective values per image and no gradient.
    The white-box attack's decrease under the same rule, eps and steps is printed next to it; no
    ratio is fixed in advance. Measured on an MI355X, L(x0) = 3.6315 / 3.2793: L∞ 3.3154 / 3.0005
    (white-box 2.2298 / 1.8756), with momentum 1.0 3.2491 / 2.8843 (white-box 2.2557 / 1.8980),
    L2 3.3756 / 3.0241 (white-box 2.3806 / 2.0253); DESIGN.md §4 records them."""
    from gfa_amd import attack
    x0, t = images()
    eng = engine32(net32, cuda)
    l0 = eng.loss(x0.to(cuda)).double()
    eps, kw = DEC_RULES[name]
    adv, info = attack(net32, x0, eps, STEPS_DEC, target=t, spsa_samples=Q_DEC, seed=5,
                       return_info=True, **kw)
    assert info["queries"] == 2 * Q_DEC * STEPS_DEC
    ls = eng.loss(adv.to(cuda)).double()
    white = dict(kw, momentum=kw["momentum"] or 0.0) if "momentum" in kw else kw
    lw = eng.loss(attack(net32, x0, eps, STEPS_DEC, target=t, **white).to(cuda)).double()
    print(f"SPSA decrease {name} q={Q_DEC} steps={STEPS_DEC}: L(x0) {l0.tolist()}, SPSA L(adv) "
          f"{ls.tolist()} (decrease {(l0 - ls).tolist()}), white-box L(adv) {lw.tolist()} "
          f"(decrease {(l0 - lw).tolist()})")
    assert (ls < l0).all()
    del eng


def test_attack_spsa_fp16(cuda):
    """fp16 networks: the invariants only (bounds, determinism, batch independence, x0 untouched);
    the decrease is not checked. The loss scale plays no part: no rescale happens."""
    from gfa_amd import attack, networks
    net = networks.build_net(SIZE, seed=0, dtype=torch.float16, device=cuda)
    x0, t = images()
    keep = x0.clone()
    kw = dict(target=t, alpha=ALPHA, momentum=1.0, spsa_samples=4, seed=5)
    adv, info = attack(net, x0, EPS, 2, return_info=True, **kw)
    assert torch.equal(x0, keep) and info["rescales"] == 0 and info["queries"] == 16
    check_linf(adv, x0, f32(2 * EPS))
    assert not torch.equal(adv, x0)
    assert torch.equal(adv, attack(net, x0, EPS, 2, **kw))
    alone = attack(net, x0[1:2], EPS, 2, **{**kw, "target": t[1:2]}, spsa_first_image=1)
    assert torch.equal(alone[0], adv[1])
    del net
    free()
