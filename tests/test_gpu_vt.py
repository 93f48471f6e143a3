"""Variance-tuned attacks (torchattacks VMIFGSM, VNI with the look-ahead): the fused kernels
mia_vt_neighbor and mia_vt_combine_norms against their fp32 references (tests/vt_ref.py, bit for
bit, the counter-based noise included), the ordered per-image sum, and the attacks end to end at
32² (alone, with the look-ahead, the smoothing, input diversity and scale copies, fp16, one
teacher-forced engine step against the fp64 oracle).

All image-space quantities are in [-1,1] units (e = 2·eps, a = 2·alpha)."""
import numpy as np
import pytest
import torch

import vt_ref
from gpu_helpers import free, seeded
from test_gpu_di import offset_copy
from test_gpu_si import oracle, stable_mask
from test_gpu_ti import ALPHA, EPS, SIZE, check_linf, images

pytestmark = pytest.mark.gpu

F32 = torch.float32
U = 2.0 ** -24
IMG_SCALES = (1e4, 1.0, 1e-4)  # per-image scales: cross-image mixing cannot hide
# plane = 3·S²: 192 (one partial block), 3267 (no multiple of 4: the scalar form, a partial last
# group, 4 slots), 50700 (50 slots per image), 12288 (12 slots)
SIZES = (8, 33, 130, 64)
# The sum's longest addition chain, as the kernel is written: a thread owns one group of 4 elements
# per grid stride and the grid holds ceil(plane / 4 / 256) ≤ 1024 slots, so 1 addition per
# accumulator here, + 2 (the 4 accumulators, pairwise) + 6 wave butterfly levels + 4 wave sums +
# the ordered finish over at most 50 slots (S = 130) = 63 additions of non-negative terms; × 3
# margin: 3·63·2⁻²⁴ ≈ 1.13e-5.
SUM_TOL = 3 * 63 * U
assert SUM_TOL <= 2e-5
SEEDS = (5, (1 << 32) + 77)
C_LOOK = float(np.float32(np.float32(1.0) * np.float32(2 * ALPHA)))  # c = μ·a, μ = 1
R = float(np.float32(np.float32(1.5) * np.float32(2 * EPS)))         # r = fp32(β)·e


def f32(v):
    return float(np.float32(v))


def bits(t):
    return t.contiguous().view(torch.int32)


_inputs = {}


def case(S):
    """Per size, computed once and shared: x, m, g, gv and v (CPU fp32, per-image scales)."""
    if S not in _inputs:
        sc = torch.tensor(IMG_SCALES, dtype=F32).reshape(3, 1, 1, 1)
        _inputs[S] = {k: seeded(900 + S + 100 * i, (3, 3, S, S)) * sc
                      for i, k in enumerate(("x", "m", "g", "gv", "v"))}
    return _inputs[S]


def neighbor(x, m, c, r, seed, image0, step, sample):
    from gfa_amd import ops
    y = torch.full_like(x, float("nan"))
    return ops.vt_neighbor(x, m, y, c, r, seed, image0, step, sample)


def combine(g, gv, v, l1=True, start=None):
    """(gt, new v, Σ|gt|, nonfinite) of mia_vt_combine_norms on device tensors; v is updated in a
    copy and gt starts NaN-filled."""
    from gfa_amd import ops
    N = g.shape[0]
    v = offset_copy(v) if v.data_ptr() % 16 else v.clone()  # keep a 4-byte offset (scalar form)
    gt = torch.full_like(g, float("nan"))
    s1 = torch.zeros(N, device=g.device) if start is None else start.clone()
    nf = torch.zeros(N, dtype=torch.int32, device=g.device)
    ops.vt_combine_norms(g, gv, v, gt, s1 if l1 else None, nonfinite=nf)
    return gt, v, s1, nf


@pytest.mark.parametrize("S", SIZES)
def test_vt_neighbor_is_the_reference_bit_for_bit(cuda, S):
    """y equals the fp32 reference, Philox noise included, with and without the look-ahead, for
    two (step, sample) pairs and two seeds (one ≥ 2^32); reruns are bit-identical; image 1 alone
    with image0 + 1 is row 1 of the batch; r = 0 without m is a bit copy; y starts NaN-filled."""
    c = case(S)
    x, m = c["x"].to(cuda), c["m"].to(cuda)
    for seed in SEEDS:
        for step, sample in ((0, 0), (3, 2)):
            for mm, mref in ((None, None), (m, c["m"])):
                y = neighbor(x, mm, C_LOOK, R, seed, 10, step, sample)
                assert torch.isfinite(y).all()
                want = vt_ref.neighbor(c["x"], mref, C_LOOK, R, seed, 10, step, sample)
                assert torch.equal(bits(y.cpu()), bits(want)), (seed, step, sample, mm is not None)
                assert torch.equal(bits(y), bits(neighbor(x, mm, C_LOOK, R, seed, 10, step,
                                                          sample)))
                alone = neighbor(x[1:2].contiguous(),
                                 None if mm is None else mm[1:2].contiguous(), C_LOOK, R, seed, 11,
                                 step, sample)
                assert torch.equal(bits(alone[0]), bits(y[1]))
    assert torch.equal(bits(neighbor(x, None, C_LOOK, 0.0, 5, 0, 0, 0)), bits(x))
    y0 = neighbor(x, None, 0.0, R, 5, 0, 0, 0)
    for other in (neighbor(x, None, 0.0, R, 6, 0, 0, 0), neighbor(x, None, 0.0, R, 5, 1, 0, 0),
                  neighbor(x, None, 0.0, R, 5, 0, 1, 0), neighbor(x, None, 0.0, R, 5, 0, 0, 1)):
        assert not torch.equal(other[0], y0[0])
    # the largest image word: image0 + N = 2^32
    top = neighbor(x, None, 0.0, R, 5, (1 << 32) - 3, 0, 0)
    assert torch.equal(bits(top.cpu()),
                       bits(vt_ref.neighbor(c["x"], None, 0.0, R, 5, (1 << 32) - 3, 0, 0)))


@pytest.mark.parametrize("S", SIZES)
def test_vt_combine_is_the_reference_and_sums(cuda, S):
    """gt and the new v equal the fp32 reference bit for bit; gv = None leaves v unchanged; each
    image's Σ|gt| equals the fp64 sum of the device gt to SUM_TOL relative (the chain is counted
    above); the sum accumulates (+=) and may be absent; reruns are bit-identical and an image's
    results do not depend on the other images."""
    c = case(S)
    g, gv, v = c["g"].to(cuda), c["gv"].to(cuda), c["v"].to(cuda)
    gt, v1, s1, nf = combine(g, gv, v)
    want_gt, want_v = vt_ref.combine(c["g"], c["gv"], c["v"])
    assert torch.equal(bits(gt.cpu()), bits(want_gt)) and torch.equal(bits(v1.cpu()), bits(want_v))
    assert not nf.any()
    gt_l, v_l, s_l, nf_l = combine(g, None, v)
    assert torch.equal(bits(gt_l), bits(gt)) and torch.equal(bits(v_l), bits(v))
    assert torch.equal(s_l, s1) and not nf_l.any()
    a64 = gt.double().reshape(3, -1).abs().sum(1)
    err = ((s1.double() - a64).abs() / a64).cpu()
    print(f"vt sum S={S}: rel err of sum|gt| {err.tolist()} (bound {SUM_TOL:.2e})")
    assert err.max() <= SUM_TOL
    assert s1[0] > 1e3 * s1[1] > 1e6 * s1[2] > 0  # the per-image scales arrived
    gt_b, v_b, s_b, _ = combine(g, gv, v)
    assert torch.equal(bits(gt_b), bits(gt)) and torch.equal(bits(v_b), bits(v1))
    assert torch.equal(s_b, s1)
    gt_1, v_1, s_1, _ = combine(g[1:2].contiguous(), gv[1:2].contiguous(), v[1:2].contiguous())
    assert torch.equal(bits(gt_1[0]), bits(gt[1])) and torch.equal(bits(v_1[0]), bits(v1[1]))
    assert torch.equal(s_1[0], s1[1])
    gt_n, v_n, s_n, _ = combine(g, gv, v, l1=False)
    assert torch.equal(bits(gt_n), bits(gt)) and torch.equal(bits(v_n), bits(v1))
    assert not s_n.any()
    _, _, s_a, _ = combine(g, gv, v, start=torch.ones(3, device=cuda))
    assert torch.equal(s_a, 1.0 + s1)


@pytest.mark.parametrize("S", [8, 130, 64])
def test_vt_vector_and_scalar_paths_agree(cuda, S):
    """plane % 4 == 0 on 16-byte aligned buffers moves 16-byte vectors; the same data at a 4-byte
    offset takes the scalar form. The bits, the sum included, are the same."""
    from gfa_amd import ops
    c = case(S)
    x, m = c["x"].to(cuda), c["m"].to(cuda)
    g, gv, v = c["g"].to(cuda), c["gv"].to(cuda), c["v"].to(cuda)
    for t in (x, m, g, gv, v):
        assert t.data_ptr() % 16 == 0
    args = (C_LOOK, R, SEEDS[1], 4, 3, 2)
    y = neighbor(x, m, *args)
    assert torch.equal(bits(neighbor(offset_copy(x), m, *args)), bits(y))
    assert torch.equal(bits(neighbor(x, offset_copy(m), *args)), bits(y))
    y_o = offset_copy(torch.zeros_like(x))
    assert torch.equal(bits(ops.vt_neighbor(x, m, y_o, *args)), bits(y))
    gt, v1, s1, _ = combine(g, gv, v)
    for alt in ((offset_copy(g), gv, v), (g, offset_copy(gv), v), (g, gv, offset_copy(v))):
        gt_o, v_o, s_o, _ = combine(*alt)
        assert torch.equal(bits(gt_o), bits(gt)) and torch.equal(bits(v_o), bits(v1))
        assert torch.equal(s_o, s1)
    gt_o, t1 = offset_copy(torch.zeros_like(g)), torch.zeros(3, device=cuda)
    vv = v.clone()
    ops.vt_combine_norms(g, gv, vv, gt_o, t1)
    assert torch.equal(bits(gt_o), bits(gt)) and torch.equal(bits(vv), bits(v1))
    assert torch.equal(t1, s1)


def test_vt_combine_flags_nonfinite(cuda):
    c = case(33)
    g, gv, v = c["g"].to(cuda), c["gv"].to(cuda), c["v"].to(cuda)
    bad = g.clone()
    bad[1, 2, 10, 5] = float("inf")
    _, _, s1, nf = combine(bad, gv, v)
    assert nf.tolist() == [0, 1, 0]
    assert torch.isfinite(s1[0]) and torch.isfinite(s1[2])
    bad = gv.clone()
    bad[0, 0, 0, 0] = float("nan")
    gt, _, s1, nf = combine(g, bad, v)
    assert nf.tolist() == [1, 0, 0] and torch.isfinite(gt).all() and torch.isfinite(s1).all()
    bad = v.clone()
    bad[2, 2, 32, 32] = float("nan")                 # the last element: a partial group of 3
    _, _, _, nf = combine(g, gv, bad)
    assert nf.tolist() == [0, 0, 1]
    _, _, _, nf = combine(g, None, bad)
    assert nf.tolist() == [0, 0, 1]


def test_vt_wrappers_reject_malformed_calls(cuda):
    from gfa_amd import ops
    x = torch.zeros(2, 3, 8, 8, device=cuda)
    y, m, w = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    l1 = torch.zeros(2, device=cuda)
    nb = lambda a, b, mm=None, r=0.1, image0=0: ops.vt_neighbor(a, mm, b, 0.0, r, 5, image0, 0, 0)  # noqa: E731,E501
    cb = lambda a, b: ops.vt_combine_norms(a, m, w, b, l1)                                # noqa: E731
    for fn in (nb, cb):
        with pytest.raises(ValueError):
            fn(x, x)                                             # in place
        with pytest.raises(ValueError):
            fn(x, y[:1])
        with pytest.raises(ValueError):
            fn(x.double(), y.double())
        with pytest.raises(ValueError):
            fn(x.cpu(), y)
        with pytest.raises(ValueError):
            fn(x, y.cpu())
        # overlapping views of one buffer: the library's own check (MIA_EINVAL)
        flat = torch.zeros(2 * 3 * 8 * 8 + 4, device=cuda)
        a, b = flat[:-4].view(2, 3, 8, 8), flat[4:].view(2, 3, 8, 8)
        with pytest.raises(Exception, match="distinct"):
            fn(a, b)
    flat = torch.zeros(2 * 3 * 8 * 8 + 4, device=cuda)
    a, b = flat[:-4].view(2, 3, 8, 8), flat[4:].view(2, 3, 8, 8)
    with pytest.raises(Exception, match="distinct"):
        nb(x, a, mm=b)                                           # m overlaps y
    with pytest.raises(Exception, match="distinct"):
        ops.vt_combine_norms(x, a, b, y, l1)                     # gv overlaps v
    with pytest.raises(Exception, match="distinct"):
        ops.vt_combine_norms(x, None, a, b, l1)                  # v overlaps gt
    with pytest.raises(ValueError):
        nb(x, y, mm=y)
    with pytest.raises(ValueError):
        nb(x, y, mm=m.cpu())
    for r in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            nb(x, y, r=r)
    with pytest.raises(ValueError):
        nb(x, y, image0=(1 << 32) - 1)
    with pytest.raises(ValueError):
        ops.vt_combine_norms(x, m, w, y, torch.zeros(3, device=cuda))
    with pytest.raises(ValueError):
        ops.vt_combine_norms(x, m, w, y, l1, nonfinite=torch.zeros(2, device=cuda))  # not int32
    with pytest.raises(ValueError):
        ops.vt_combine_norms(x, m, m, y, l1)                     # gv is v


# ---- end to end at 32² --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net32(cuda):
    from gfa_amd import networks
    return networks.build_net(SIZE, seed=0, dtype=torch.float32, device=cuda)


def test_attack_without_vt_is_unchanged_and_one_step_is_mi(cuda, net32):
    """vt_samples = None runs today's path (the bits of the attack without the keyword, for
    momentum None / 0 / 1); at the only step v = 0, so steps = 1 with vt_samples = 3 gives the
    bits of the MI step, and fgsm too."""
    from gfa_amd import attack, fgsm
    x0, t = images()
    for mu in (None, 0.0, 1.0):
        kw = dict(target=t, alpha=ALPHA, momentum=mu)
        plain = attack(net32, x0, EPS, 3, **kw)
        adv, info = attack(net32, x0, EPS, 3, vt_samples=None, return_info=True, **kw)
        assert info["vt_samples"] is None and info["vt_beta"] is None
        assert torch.equal(adv, plain)
    for mu in (0.0, 1.0):
        kw = dict(target=t, alpha=ALPHA, momentum=mu)
        assert torch.equal(attack(net32, x0, EPS, 1, vt_samples=3, **kw),
                           attack(net32, x0, EPS, 1, **kw))
    assert torch.equal(attack(net32, x0, EPS, 1, target=t, alpha=ALPHA, vt_samples=3),
                       attack(net32, x0, EPS, 1, target=t, alpha=ALPHA, momentum=0.0))
    assert torch.equal(fgsm(net32, x0, EPS, target=t, vt_samples=3),
                       fgsm(net32, x0, EPS, target=t, momentum=0.0))
    assert torch.equal(fgsm(net32, x0, EPS, target=t, vt_samples=3, momentum=1.0, nesterov=True),
                       fgsm(net32, x0, EPS, target=t, momentum=1.0))


VT_VARIANTS = {
    "vt": dict(),
    "vt-ni": dict(momentum=1.0, nesterov=True),
    "vt-ti": dict(ti_kernel=15),
    "vt-si-ni-ti-dim": dict(momentum=1.0, nesterov=True, ti_kernel=15, di_prob=1.0, si_scales=2),
}


def check_vt_attack(net, name, extra):
    from gfa_amd import attack
    x0, t = images()
    keep = x0.clone()
    e = f32(2 * EPS)
    kw = dict(target=t, alpha=ALPHA, vt_samples=2, seed=5, **extra)
    adv, info = attack(net, x0, EPS, 3, return_info=True, **kw)
    assert torch.equal(x0, keep)
    assert info["vt_samples"] == 2 and info["vt_beta"] == 1.5
    assert info["nesterov"] is extra.get("nesterov", False) and info["norm"] == "linf"
    assert info["momentum"] == extra.get("momentum") and info["si_scales"] == extra.get("si_scales")
    assert info["ti_kernel"] == extra.get("ti_kernel") and info["di_prob"] == extra.get("di_prob")
    check_linf(adv, x0, e)
    assert torch.equal(adv, attack(net, x0, EPS, 3, **kw))
    alone = attack(net, x0[1:2], EPS, 3, **{**kw, "target": t[1:2]}, vt_first_image=1)
    assert torch.equal(alone[0], adv[1])
    alone = attack(net, x0[:1], EPS, 3, **{**kw, "target": t[:1]})
    assert torch.equal(alone[0], adv[0])
    base = {**kw, "vt_samples": None}
    if "momentum" not in base:
        base["momentum"] = 0.0
    others = dict(plain=attack(net, x0, EPS, 3, **base),
                  seed=attack(net, x0, EPS, 3, **{**kw, "seed": 6}),
                  beta=attack(net, x0, EPS, 3, vt_beta=1.0, **kw))
    diff = {k: (adv != o).float().mean().item() for k, o in others.items()}
    print(f"VT linf {name}: share of pixels that differ from the same attack without vt_samples "
          f"{diff['plain']:.4f}, with another seed {diff['seed']:.4f}, with vt_beta=1 "
          f"{diff['beta']:.4f}; rescales {info['rescales']}, loss scale {info['loss_scale']:g}")
    assert all(d > 0 for d in diff.values())
    return info


@pytest.mark.parametrize("name", list(VT_VARIANTS))
def test_attack_vt_linf(cuda, net32, name):
    info = check_vt_attack(net32, name, VT_VARIANTS[name])
    assert info["rescales"] == 0


def test_attack_vt_fp16(cuda):
    """fp16 networks (loss scale 2^8, divided out before v is formed; a loss-scale re-run starts
    from v = 0 and replays the same noise): the same invariants for vt + nesterov."""
    from gfa_amd import networks
    net = networks.build_net(SIZE, seed=0, dtype=torch.float16, device=cuda)
    check_vt_attack(net, "vt-ni fp16", VT_VARIANTS["vt-ni"])
    del net
    free()


# ---- one engine step against the fp64 oracle ------------------------------------------------------
_shared = {}


def oracle_variance(n, seed=5, step=0, beta=1.5):
    """(g0, gv, v1 = gv − g0) of the fp64 oracle at x0 for n neighbours x0 + f32(r·u_i),
    r = f32(f32(beta)·e). g0 and the per-neighbour gradients are computed once and shared."""
    x0, _ = images()
    grad = oracle()
    if "g0" not in _shared:
        _shared["g0"] = grad(x0.double())
    e = np.float32(f32(2 * EPS))
    r = float(np.float32(np.float32(beta) * e))
    per = _shared.setdefault("per", {})
    for i in range(n):
        if (seed, step, beta, i) not in per:
            y = vt_ref.neighbor(x0, None, 0.0, r, seed, 0, step, i)
            per[(seed, step, beta, i)] = grad(y.double())
    gv = sum(per[(seed, step, beta, i)] for i in range(n)) / n
    return _shared["g0"], gv, gv - _shared["g0"], r


def _norm(t):
    return t.double().reshape(t.shape[0], -1).norm(dim=1)


@pytest.mark.parametrize("n", [2, 5])
def test_engine_vt_step_vs_oracle(cuda, net32, n):
    """One step_mi from x = x0 with m = 0 and the variance buffer preset to v1.float(), v1 = gv − g0
    of the oracle (noise of step 0, Philox key 5): with m1 = −(g0 + v1)/mean|g0 + v1| the device's x1
    equals project_step(x0, x0, g0 + v1, e, a) wherever |m1| > 1e-3·max|m1| (at most 2 % excluded;
    0.24 % / 0.28 % expected for n = 2 / 5), and the step must differ from the one with v = 0 on at
    least 20 stable pixels (111 / 94 expected) — both asserted on the oracle alone. The step also
    recomputes v from the same noise: ‖v_dev − v1‖₂ ≤ 0.05·‖v1‖₂ per image, the project's fp32
    gradient bound against this oracle (1e-3) times the cancellation factor
    (‖gv‖ + ‖g0‖)/‖v1‖ ≤ 50 (34.6 / 49.7 expected), asserted on the oracle; another seed moves v1
    by more than 10 % (about 140 % expected)."""
    from gfa_amd.pgd import AttackEngine, VtStep
    from oracle import attack_ref
    x0, t = images()
    a, e = f32(2 * ALPHA), f32(2 * EPS)
    g0, gv, v1, r = oracle_variance(n)
    gt = g0 + v1.float().double()
    mean = gt.abs().reshape(2, -1).mean(dim=1).reshape(2, 1, 1, 1)
    m1 = -gt / mean
    stable = stable_mask(m1)
    share = 1.0 - stable.double().mean().item()
    want = attack_ref.project_step(x0, x0, gt.float(), e, a)
    want_plain = attack_ref.project_step(x0, x0, g0.float(), e, a)
    moved = int((want != want_plain)[stable].sum())
    factor = ((_norm(gv) + _norm(g0)) / _norm(v1)).max().item()
    other = (_norm(oracle_variance(2, seed=6)[2] - oracle_variance(2)[2])
             / _norm(oracle_variance(2)[2])).min().item()
    print(f"VT engine step N={n}: {share:.4%} of the pixels excluded; v changes the expected step "
          f"on {moved} stable pixels; cancellation factor {factor:.1f}; another seed moves v1 "
          f"(N=2) by {other:.1%}")
    assert share <= 0.02
    assert moved >= 20
    assert factor <= 50
    assert other > 0.10
    eng = AttackEngine(net32.encoder.impl, net32.decoder.impl, net32.vgg.impl)
    eng.prepare(x0.to(cuda), t.to(cuda))
    x = x0.to(cuda).clone()
    m = torch.zeros_like(x)
    v = eng.ws.get("vt.v", x.shape, F32)
    v.copy_(v1.float().to(cuda))
    eng.step_mi(x, m, 0.0, a, e, vt=VtStep(n, r, 5, 0, 0, False))
    assert not eng.overflowed()
    got = x.cpu()
    frac = (got == want).float().mean().item()
    v_dev = eng.ws.get("vt.v", x.shape, F32).cpu().double()
    ratio = (_norm(v_dev - v1) / _norm(v1)).tolist()
    print(f"VT engine step N={n}: equal to the oracle step on {frac:.6f} of all pixels; "
          f"|v_dev - v1| / |v1| per image {ratio} (bound 0.05)")
    assert torch.equal(got[stable], want[stable])
    assert max(ratio) <= 0.05
    del eng
