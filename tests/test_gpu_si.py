"""Scale-invariant and Nesterov attacks (torchattacks SINIFGSM / NIFGSM): the fused kernels
mia_si_transform and mia_si_accumulate_norms against their fp32 references (tests/si_ref.py, bit
for bit), the ordered per-image sums, and the attacks end to end at 32² (L∞ with and without
momentum, look-ahead, smoothing and input diversity, L2, fp16, one step against the oracle, one
Nesterov step of the engine against the oracle).

All image-space quantities are in [-1,1] units (e = 2·eps, a = 2·alpha)."""
import numpy as np
import pytest
import torch

import si_ref
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
# The sums' longest addition chain, as the kernel is written: a thread owns one group of 4
# elements per grid stride and the grid holds ceil(plane / 4 / 256) ≤ 1024 slots, so 1 addition
# per accumulator here, + 2 (the 4 accumulators, pairwise) + 6 wave butterfly levels + 4 wave sums
# + the ordered finish over at most 50 slots (S = 130) = 63 additions of non-negative terms (r²
# enters through an fma, unrounded); × 3 margin: 3·63·2⁻²⁴ ≈ 1.13e-5, within
# grad_assemble_norms' 2e-5.
SUM_TOL = 3 * 63 * U
assert SUM_TOL <= 2e-5
C_LOOK = float(np.float32(np.float32(1.0) * np.float32(2 * ALPHA)))  # c = μ·a, μ = 1


def f32(v):
    return float(np.float32(v))


def bits(t):
    return t.contiguous().view(torch.int32)


_inputs = {}


def case(S):
    """Per size, computed once and shared: x, m and three gradients (CPU fp32, per-image scales)
    and the reference accumulator after each copy of a 3-copy sequence (first, middle, last with
    div = 3)."""
    if S not in _inputs:
        sc = torch.tensor(IMG_SCALES, dtype=F32).reshape(3, 1, 1, 1)
        x = seeded(800 + S, (3, 3, S, S)) * sc
        m = seeded(820 + S, (3, 3, S, S)) * sc
        g = [seeded(840 + S + 100 * i, (3, 3, S, S)) * sc for i in range(3)]
        a0 = si_ref.accumulate(g[0], None, 1.0, True)
        a1 = si_ref.accumulate(g[1], a0, 0.5, False)
        a2 = si_ref.accumulate(g[2], a1, 0.25, False, 3.0)
        _inputs[S] = dict(x=x, m=m, g=g, acc=[a0, a1, a2])
    return _inputs[S]


def transform(x, m, c, s):
    from gfa_amd import ops
    y = torch.full_like(x, float("nan"))
    return ops.si_transform(x, m, y, c, s)


def accumulate(g, acc, w, first, div=1.0, l1=True, l2=True, start=None):
    """(acc, Σ|acc|, Σacc², nonfinite) of mia_si_accumulate_norms on device tensors; acc is
    updated in a copy (NaN-filled when first: the kernel must not read it)."""
    from gfa_amd import ops
    N = g.shape[0]
    acc = torch.full_like(g, float("nan")) if first else acc.clone()
    s1 = torch.zeros(N, device=g.device) if start is None else start.clone()
    s2 = torch.zeros(N, device=g.device) if start is None else start.clone()
    nf = torch.zeros(N, dtype=torch.int32, device=g.device)
    ops.si_accumulate_norms(g, acc, s1 if l1 else None, s2 if l2 else None, w, first, div,
                            nonfinite=nf)
    return acc, s1, s2, nf


@pytest.mark.parametrize("S", SIZES)
def test_si_transform_is_the_reference_bit_for_bit(cuda, S):
    """y equals the fp32 reference (one rounding per operation, in the kernel's order) for
    i ∈ {0, 1, 4} with and without the look-ahead; m = None with s = 1 is a bit copy; reruns are
    bit-identical and an image's output does not depend on the other images."""
    c = case(S)
    x, m = c["x"].to(cuda), c["m"].to(cuda)
    for i in (0, 1, 4):
        s = 2.0 ** -i
        for mm, mref in ((None, None), (m, c["m"])):
            y = transform(x, mm, C_LOOK, s)
            assert torch.isfinite(y).all()
            assert torch.equal(bits(y.cpu()), bits(si_ref.transform(c["x"], mref, C_LOOK, s))), \
                (i, mm is not None)
            assert torch.equal(bits(y), bits(transform(x, mm, C_LOOK, s)))
            alone = transform(x[1:2].contiguous(), None if mm is None else mm[1:2].contiguous(),
                              C_LOOK, s)
            assert torch.equal(bits(alone[0]), bits(y[1]))
    assert torch.equal(bits(transform(x, None, C_LOOK, 1.0)), bits(x))
    # the copies are not the identity, and not the scaling towards mid-grey (x·s)
    y1 = transform(x, None, 0.0, 0.5).cpu()
    assert not torch.equal(y1, c["x"]) and not torch.equal(y1, c["x"] * 0.5)
    assert not torch.equal(transform(x, m, C_LOOK, 1.0), x)


@pytest.mark.parametrize("S", SIZES)
def test_si_accumulate_sequence_sums_and_determinism(cuda, S):
    """A 3-copy sequence (first; middle; last with div = 3) gives the reference accumulator bit for
    bit after every copy. Each image's Σ|acc| and Σacc² equal the fp64 sums of the device acc to
    SUM_TOL relative (the chain is counted above). Reruns are bit-identical, an image's acc and
    sums do not depend on the other images, either sum may be absent, the sums accumulate (+=)."""
    c = case(S)
    g = [t.to(cuda) for t in c["g"]]
    a0, _, _, nf0 = accumulate(g[0], None, 1.0, True)
    a1, _, _, nf1 = accumulate(g[1], a0, 0.5, False)
    a2, s1, s2, nf2 = accumulate(g[2], a1, 0.25, False, 3.0)
    for k, got in enumerate((a0, a1, a2)):
        assert torch.equal(bits(got.cpu()), bits(c["acc"][k])), k
    assert not nf0.any() and not nf1.any() and not nf2.any()
    a64 = a2.double().reshape(3, -1)
    e1 = ((s1.double() - a64.abs().sum(1)).abs() / a64.abs().sum(1)).cpu()
    e2 = ((s2.double() - (a64 * a64).sum(1)).abs() / (a64 * a64).sum(1)).cpu()
    print(f"si sums S={S}: rel err of sum|acc| {e1.tolist()}, of sum acc^2 {e2.tolist()} "
          f"(bound {SUM_TOL:.2e})")
    assert e1.max() <= SUM_TOL and e2.max() <= SUM_TOL
    assert s1[0] > 1e3 * s1[1] > 1e6 * s1[2] > 0  # the per-image scales arrived
    last = (g[2], a1, 0.25, False, 3.0)
    a_b, s1_b, s2_b, _ = accumulate(*last)
    assert torch.equal(bits(a_b), bits(a2)) and torch.equal(s1_b, s1) and torch.equal(s2_b, s2)
    a_1, s1_1, s2_1, _ = accumulate(g[2][1:2].contiguous(), a1[1:2].contiguous(), 0.25, False, 3.0)
    assert torch.equal(bits(a_1[0]), bits(a2[1]))
    assert torch.equal(s1_1[0], s1[1]) and torch.equal(s2_1[0], s2[1])
    a_c, s1_c, s2_c, _ = accumulate(*last, l2=False)
    assert torch.equal(bits(a_c), bits(a2)) and torch.equal(s1_c, s1) and not s2_c.any()
    a_c, s1_c, s2_c, _ = accumulate(*last, l1=False)
    assert torch.equal(bits(a_c), bits(a2)) and torch.equal(s2_c, s2) and not s1_c.any()
    a_c, _, _, _ = accumulate(*last, l1=False, l2=False)
    assert torch.equal(bits(a_c), bits(a2))
    _, s1_a, s2_a, _ = accumulate(*last, start=torch.ones(3, device=cuda))
    assert torch.equal(s1_a, 1.0 + s1) and torch.equal(s2_a, 1.0 + s2)
    # the sums of a first copy too (the kernel that ends a 1-copy chain)
    _, t1, t2, _ = accumulate(g[0], None, 1.0, True)
    g64 = g[0].double().reshape(3, -1)
    assert ((t1.double() - g64.abs().sum(1)).abs() / g64.abs().sum(1)).max() <= SUM_TOL
    assert ((t2.double() - (g64 * g64).sum(1)).abs() / (g64 * g64).sum(1)).max() <= SUM_TOL


@pytest.mark.parametrize("S", [8, 130, 64])
def test_si_vector_and_scalar_paths_agree(cuda, S):
    """plane % 4 == 0 on 16-byte aligned buffers moves 16-byte vectors; the same data at a 4-byte
    offset takes the scalar form. The bits, sums included, are the same."""
    c = case(S)
    x, m = c["x"].to(cuda), c["m"].to(cuda)
    g, a1 = c["g"][2].to(cuda), c["acc"][1].to(cuda)
    assert x.data_ptr() % 16 == 0 and m.data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0
    y = transform(x, m, C_LOOK, 0.25)
    assert torch.equal(bits(transform(offset_copy(x), m, C_LOOK, 0.25)), bits(y))
    assert torch.equal(bits(transform(x, offset_copy(m), C_LOOK, 0.25)), bits(y))
    from gfa_amd import ops
    y_o = offset_copy(torch.zeros_like(x))
    assert torch.equal(bits(ops.si_transform(x, m, y_o, C_LOOK, 0.25)), bits(y))
    acc, s1, s2, _ = accumulate(g, a1, 0.25, False, 3.0)
    acc_o, s1_o, s2_o, _ = accumulate(offset_copy(g), a1, 0.25, False, 3.0)
    assert torch.equal(bits(acc_o), bits(acc)) and torch.equal(s1_o, s1) and torch.equal(s2_o, s2)
    nf = torch.zeros(3, dtype=torch.int32, device=cuda)
    t1, t2 = torch.zeros(3, device=cuda), torch.zeros(3, device=cuda)
    acc_o = offset_copy(a1)
    ops.si_accumulate_norms(g, acc_o, t1, t2, 0.25, False, 3.0, nonfinite=nf)
    assert torch.equal(bits(acc_o), bits(acc)) and torch.equal(t1, s1) and torch.equal(t2, s2)


def test_si_accumulate_flags_nonfinite(cuda):
    c = case(33)
    g = c["g"][1].to(cuda).clone()
    g[1, 2, 10, 5] = float("inf")
    _, s1, s2, nf = accumulate(g, c["acc"][0].to(cuda), 0.5, False)
    assert nf.tolist() == [0, 1, 0]
    assert torch.isfinite(s1[0]) and torch.isfinite(s1[2])
    assert torch.isfinite(s2[0]) and torch.isfinite(s2[2])
    acc = c["acc"][0].to(cuda).clone()
    acc[2, 2, 32, 32] = float("nan")                 # the last element: a partial group of 3
    _, _, _, nf = accumulate(c["g"][1].to(cuda), acc, 0.5, False)
    assert nf.tolist() == [0, 0, 1]


def test_si_wrappers_reject_malformed_calls(cuda):
    from gfa_amd import ops
    x = torch.zeros(2, 3, 8, 8, device=cuda)
    y = torch.zeros_like(x)
    m = torch.zeros_like(x)
    v = torch.zeros(2, device=cuda)
    tr = lambda a, b, s=0.5, mm=None: ops.si_transform(a, mm, b, 0.0, s)            # noqa: E731
    ac = lambda a, b, s=0.5: ops.si_accumulate_norms(a, b, v, v, s, False)          # noqa: E731
    for fn in (tr, ac):
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
        for s in (0.0, 3.0, 0.75, 2.0, 2.0 ** -8, float("nan")):  # not 2^-i, 0 <= i < 8
            with pytest.raises(ValueError):
                fn(x, y, s)
        # overlapping views of one buffer: the library's own check (MIA_EINVAL)
        flat = torch.zeros(2 * 3 * 8 * 8 + 4, device=cuda)
        a, b = flat[:-4].view(2, 3, 8, 8), flat[4:].view(2, 3, 8, 8)
        with pytest.raises(Exception, match="distinct"):
            fn(a, b)
    with pytest.raises(ValueError):
        tr(x, y, mm=y)                                           # the look-ahead buffer is y
    with pytest.raises(ValueError):
        tr(x, y, mm=m.cpu())
    with pytest.raises(ValueError):
        tr(x, y, mm=m[:1])
    with pytest.raises(ValueError):
        ops.si_accumulate_norms(x, y, torch.zeros(3, device=cuda), v, 0.5, False)
    with pytest.raises(ValueError):
        ops.si_accumulate_norms(x, y, v, v, 0.5, False,
                                nonfinite=torch.zeros(2, device=cuda))  # not int32
    with pytest.raises(ValueError):
        ops.si_accumulate_norms(x, y, v, v, 0.5, False, 0.5)     # div < 1


# ---- end to end at 32² --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net32(cuda):
    from gfa_amd import networks
    return networks.build_net(SIZE, seed=0, dtype=torch.float32, device=cuda)


def test_attack_si_one_scale_is_the_plain_attack(cuda, net32):
    """si_scales = 1, and si_scales = None with nesterov = False, run today's path: the bits of
    the attack without them, for L∞ with momentum 0 and 1 and for L2."""
    from gfa_amd import attack
    x0, t = images()
    for mu in (0.0, 1.0):
        kw = dict(target=t, alpha=ALPHA, momentum=mu)
        plain = attack(net32, x0, EPS, 3, **kw)
        adv, info = attack(net32, x0, EPS, 3, si_scales=1, return_info=True, **kw)
        assert info["si_scales"] == 1 and info["nesterov"] is False
        assert torch.equal(adv, plain)
        adv, info = attack(net32, x0, EPS, 3, si_scales=None, nesterov=False, return_info=True,
                           **kw)
        assert info["si_scales"] is None and info["nesterov"] is False
        assert torch.equal(adv, plain)
    kw = dict(target=t, alpha=ALPHA_L2, norm="l2")
    plain = attack(net32, x0, EPS_L2, 3, **kw)
    assert torch.equal(attack(net32, x0, EPS_L2, 3, si_scales=1, **kw), plain)
    assert torch.equal(attack(net32, x0, EPS_L2, 3, si_scales=None, nesterov=False, **kw), plain)
    # without momentum, TI or DI, si_scales = 1 stays on the plain PGD rule
    assert torch.equal(attack(net32, x0, EPS, 3, target=t, alpha=ALPHA, si_scales=1),
                       attack(net32, x0, EPS, 3, target=t, alpha=ALPHA))


LINF_VARIANTS = {
    "si": dict(),
    "si-ni": dict(momentum=1.0, nesterov=True),
    "si-ti": dict(ti_kernel=15),
    "si-di": dict(di_prob=1.0, seed=5),
    "si-ni-ti-dim": dict(momentum=1.0, nesterov=True, ti_kernel=15, di_prob=1.0, seed=5),
}


@pytest.mark.parametrize("name", list(LINF_VARIANTS))
def test_attack_si_linf(cuda, net32, name):
    from gfa_amd import attack
    extra = LINF_VARIANTS[name]
    x0, t = images()
    keep = x0.clone()
    e = f32(2 * EPS)
    kw = dict(target=t, alpha=ALPHA, si_scales=5, **extra)
    adv, info = attack(net32, x0, EPS, 3, return_info=True, **kw)
    assert torch.equal(x0, keep)
    assert info["si_scales"] == 5 and info["nesterov"] is extra.get("nesterov", False)
    assert info["norm"] == "linf" and info["momentum"] == extra.get("momentum")
    assert info["ti_kernel"] == extra.get("ti_kernel") and info["di_prob"] == extra.get("di_prob")
    assert info["di_applied"] == (3 if "di_prob" in extra else 0) and info["rescales"] == 0
    check_linf(adv, x0, e)
    assert torch.equal(adv, attack(net32, x0, EPS, 3, **kw))
    alone = attack(net32, x0[:1], EPS, 3, **{**kw, "target": t[:1]})
    assert torch.equal(alone[0], adv[0])
    base = {**kw, "si_scales": None}
    if "momentum" not in base:
        base["momentum"] = 0.0
    diff = (adv != attack(net32, x0, EPS, 3, **base)).float().mean().item()
    print(f"SI linf {name}: differs from the same attack without SI on {diff:.4f} of pixels")
    assert diff > 0


def test_attack_si_l2(cuda, net32):
    from gfa_amd import attack
    x0, t = images()
    keep = x0.clone()
    e = f32(2 * EPS_L2)
    for extra in (dict(), dict(ti_kernel=15, di_prob=1.0, seed=5)):
        kw = dict(target=t, alpha=ALPHA_L2, norm="l2", si_scales=5, **extra)
        adv, info = attack(net32, x0, EPS_L2, 3, return_info=True, **kw)
        assert torch.equal(x0, keep) and info["si_scales"] == 5 and info["norm"] == "l2"
        assert info["nesterov"] is False and info["di_applied"] == (3 if extra else 0)
        nrm = (adv.double() - x0.double()).reshape(2, -1).norm(dim=1)
        print(f"SI attack(norm='l2', {extra}, steps=3): |adv - x0| {nrm.tolist()} (e = {e})")
        assert (nrm <= e * (1 + 1e-5)).all() and (nrm > 0).all()
        assert adv.min() >= -1 and adv.max() <= 1
        assert torch.equal(adv, attack(net32, x0, EPS_L2, 3, **kw))
        alone = attack(net32, x0[:1], EPS_L2, 3, **{**kw, "target": t[:1]})
        assert torch.equal(alone[0], adv[0])
        assert not torch.equal(adv, attack(net32, x0, EPS_L2, 3, **{**kw, "si_scales": None}))


def test_attack_nesterov_acts_from_the_second_step(cuda, net32):
    """m = 0 at the start, so the look-ahead is a no-op at step 1 (fgsm too) and changes the
    attack afterwards."""
    from gfa_amd import attack, fgsm
    x0, t = images()
    kw = dict(target=t, alpha=ALPHA, momentum=1.0)
    assert torch.equal(attack(net32, x0, EPS, 1, nesterov=True, **kw),
                       attack(net32, x0, EPS, 1, **kw))
    adv, info = attack(net32, x0, EPS, 3, nesterov=True, return_info=True, **kw)
    assert info["nesterov"] is True and info["si_scales"] is None
    diff = (adv != attack(net32, x0, EPS, 3, **kw)).float().mean().item()
    print(f"NI linf momentum=1: differs from MI on {diff:.4f} of pixels after 3 steps")
    assert diff > 0
    check_linf(adv, x0, f32(2 * EPS))
    assert torch.equal(adv, attack(net32, x0, EPS, 3, nesterov=True, **kw))
    assert torch.equal(fgsm(net32, x0, EPS, target=t, momentum=1.0, nesterov=True, si_scales=2),
                       fgsm(net32, x0, EPS, target=t, momentum=1.0, si_scales=2))


def test_attack_si_with_the_di_identity_schedule(cuda, net32):
    """Rows (S, 0, 0, 1) run both DI kernels as the identity (bit for bit), so si_scales = 3 with
    them gives the bits of si_scales = 3 without DI: with momentum 0 the update reads only
    sign(g), and with the smoothing the norms are taken after it, from the same bits."""
    from gfa_amd import attack
    x0, t = images()
    ident = torch.tensor([[SIZE, 0, 0, 1]] * 3)
    kw = dict(target=t, alpha=ALPHA, si_scales=3)
    adv, info = attack(net32, x0, EPS, 3, di_schedule=ident, return_info=True, **kw)
    assert info["di_applied"] == 3 and info["si_scales"] == 3
    assert torch.equal(adv, attack(net32, x0, EPS, 3, **kw))
    kw = dict(target=t, alpha=ALPHA, si_scales=3, momentum=1.0, nesterov=True, ti_kernel=15)
    assert torch.equal(attack(net32, x0, EPS, 3, di_schedule=ident, **kw),
                       attack(net32, x0, EPS, 3, **kw))


def test_attack_si_fp16(cuda):
    """fp16 networks (loss scale 2^8, divided out before the accumulation): the same invariants
    for si_scales = 3 with the look-ahead."""
    from gfa_amd import attack, networks
    net = networks.build_net(SIZE, seed=0, dtype=torch.float16, device=cuda)
    x0, t = images()
    e = f32(2 * EPS)
    kw = dict(target=t, alpha=ALPHA, si_scales=3, momentum=1.0, nesterov=True)
    adv, info = attack(net, x0, EPS, 3, return_info=True, **kw)
    print(f"fp16 SI-NI attack: rescales {info['rescales']}, loss scale {info['loss_scale']:g}")
    assert info["si_scales"] == 3 and info["nesterov"] is True
    check_linf(adv, x0, e)
    assert torch.equal(adv, attack(net, x0, EPS, 3, **kw))
    alone = attack(net, x0[:1], EPS, 3, **{**kw, "target": t[:1]})
    assert torch.equal(alone[0], adv[0])
    assert not torch.equal(adv, attack(net, x0, EPS, 3, target=t, alpha=ALPHA, momentum=1.0))
    del net
    free()


# ---- against the fp64 oracle ----------------------------------------------------------------------
_oracle = {}


def oracle():
    """The fp64 networks of build_net(32, seed=0) (linear encoder) with the targets of x0 and t,
    as a function x ↦ ∇L(x). Built once."""
    if "grad" not in _oracle:
        from gfa_amd.weights import make_encoder_weights, make_generator_weights, make_vgg_weights
        from oracle import attack_ref, vgg_ref
        params = (make_generator_weights(SIZE, seed=0),
                  vgg_ref.load_positional(make_vgg_weights(1234)),
                  make_encoder_weights(SIZE, seed=1))
        p64 = to64(params)
        x0, t = images()
        refs = attack_ref.Refs(*p64, x0.double(), t.double(), SIZE)
        _oracle["grad"] = lambda x: attack_ref.loss_grad(*p64, x.double(), refs, SIZE)[1]
    return _oracle["grad"]


def stable_mask(v):
    return v.abs() > 1e-3 * v.abs().reshape(v.shape[0], -1).max(dim=1).values.reshape(-1, 1, 1, 1)


def oracle_si_gradient(x, n):
    """(1/n)·Σ_i 2^-i·∇L(S_i(x)) in fp64."""
    grad = oracle()
    return sum(2.0 ** -i * grad(si_ref.scale64(x, i)) for i in range(n)) / n


def oracle_si_at_x0(n):
    """The SI gradient at x0 from per-copy gradients computed once and shared by n = 2 and 5."""
    x0, _ = images()
    per = _oracle.setdefault("per_copy", {})
    for i in range(n):
        if i not in per:
            per[i] = 2.0 ** -i * oracle()(si_ref.scale64(x0, i))
    return sum(per[i] for i in range(n)) / n


@pytest.mark.parametrize("n", [2, 5])
def test_attack_si_one_step_vs_oracle(cuda, net32, n):
    """One SI step from x0 is clamp(x0 + clamp(a·sign(−g), −e, e), −1, 1) with
    g = (1/n)·Σ_i 2^-i·∇L(S_i(x0)) wherever g's sign is stable (|g| > 1e-3·max|g| per image); at
    most 2 % of the pixels may be excluded, asserted on the oracle's own mask before the device is
    looked at (0.24 % expected for n = 2, 0.28 % for n = 5). sign(g) differs from the plain
    gradient's on 11.5 % (n = 2) and 20.2 % (n = 5) of the pixels, so an attack that ignores the
    copies cannot pass; that too is asserted on the oracle alone (> 5 %)."""
    from gfa_amd import attack
    from oracle import attack_ref
    x0, t = images()
    g = oracle_si_at_x0(n)
    stable = stable_mask(g)
    share = 1.0 - stable.double().mean().item()
    flips = (torch.sign(g) != torch.sign(oracle_si_at_x0(1))).double().mean().item()
    print(f"SI one step n={n}: {share:.4%} of the pixels excluded (|g| <= 1e-3 max|g|); sign(g) "
          f"differs from the plain gradient's on {flips:.4%}")
    assert share <= 0.02
    assert flips > 0.05
    want = attack_ref.project_step(x0, x0, g.float(), 2 * EPS, 2 * ALPHA)
    for mu in (None, 1.0):
        got = attack(net32, x0, EPS, 1, target=t, alpha=ALPHA, momentum=mu, si_scales=n)
        frac = (got == want).float().mean().item()
        print(f"SI steps=1 n={n} momentum={mu}: equal to the oracle step on {frac:.6f} of all "
              "pixels")
        assert torch.equal(got[stable], want[stable]), mu


# α of the Nesterov test per number of scale copies. The expected steps with and without the
# look-ahead must differ on at least 20 sign-stable pixels (asserted in the test on the oracle
# alone). Without scale copies α = 2/255, as everywhere else, gives 35. With 3 copies 2/255
# gives 18 only, so that case runs at α = 3/255, which gives 23 (the look-ahead's length is μ·a).
ALPHA_NI = {1: ALPHA, 3: 3 / 255}


@pytest.mark.parametrize("n", [1, 3])
def test_engine_nesterov_step_vs_oracle(cuda, net32, n):
    """One step_mi(momentum = 1, nesterov = True) from x = x0 with the momentum buffer preset to
    m₀ = seeded(914): the gradient is taken at x0 + c·m₀ (c = μ·a in fp32), so with
        m₁ = −g/mean|g| + μ·m₀,  g = (1/n)·Σ_i 2^-i·∇L(S_i(x0 + c·m₀))  (fp64)
    x₁ equals project_step(x0, x0, −m₁, e, a) wherever |m₁| > 1e-3·max|m₁|, at most 2 % of the
    pixels excluded (0.29 % expected for n = 1, 0.18 % for n = 3 at its α). Asserted on the
    oracle alone: the expected step differs from the one without the look-ahead (g at x0) on at
    least 20 stable pixels, so a step that ignores the look-ahead cannot pass (ALPHA_NI above)."""
    from gfa_amd.pgd import AttackEngine
    from oracle import attack_ref
    x0, t = images()
    m0 = seeded(914, x0.shape)
    mu = 1.0
    alpha = ALPHA_NI[n]
    a, e = f32(2 * alpha), f32(2 * EPS)
    c = f32(np.float32(mu) * np.float32(a))

    def momentum_of(g):
        mean = g.abs().reshape(2, -1).mean(dim=1).reshape(2, 1, 1, 1)
        return -g / mean + mu * m0.double()

    m1 = momentum_of(oracle_si_gradient(x0.double() + c * m0.double(), n))
    m1_plain = momentum_of(oracle_si_at_x0(n))
    stable = stable_mask(m1)
    share = 1.0 - stable.double().mean().item()
    want = attack_ref.project_step(x0, x0, (-m1).float(), e, a)
    want_plain = attack_ref.project_step(x0, x0, (-m1_plain).float(), e, a)
    moved = int((want != want_plain)[stable].sum())
    print(f"NI engine step n={n} alpha={alpha:.6f}: {share:.4%} of the pixels excluded; the "
          f"look-ahead changes the expected step on {moved} stable pixels")
    assert share <= 0.02
    assert moved >= 20
    eng = AttackEngine(net32.encoder.impl, net32.decoder.impl, net32.vgg.impl)
    eng.prepare(x0.to(cuda), t.to(cuda))
    x = x0.to(cuda).clone()
    m = m0.to(cuda).clone()
    eng.step_mi(x, m, mu, a, e, nesterov=True, si_scales=n)
    assert not eng.overflowed()
    got = x.cpu()
    frac = (got == want).float().mean().item()
    print(f"NI engine step n={n}: equal to the oracle step on {frac:.6f} of all pixels; "
          f"max |m - m1| / max|m1| = "
          f"{((m.cpu().double() - m1).abs().max() / m1.abs().max()).item():.3e}")
    assert torch.equal(got[stable], want[stable])
    del eng
