"""Input-diversity attacks (torchattacks DIFGSM / TIFGSM input_diversity): the fused resize-pad
kernel mia_di_resize_pad and its adjoint mia_di_resize_pad_bwd_norms against the fp64 reference
(tests/di_ref.py), the adjoint's ordered per-image sums, and the attacks end to end at 32² (L∞ with
and without momentum and smoothing, L2, fp16, one step against the oracle).

All image-space quantities are in [-1,1] units (e = 2·eps, a = 2·alpha)."""
import numpy as np
import pytest
import torch

import di_ref
from gpu_helpers import free, seeded, to64
from test_gpu_ti import ALPHA, ALPHA_L2, EPS, EPS_L2, SIZE, check_linf, conv64, gauss, images

pytestmark = pytest.mark.gpu

F32 = torch.float32
U = 2.0 ** -24
IMG_SCALES = (1e4, 1.0, 1e-4)  # per-image scales: cross-image mixing cannot hide
# (S, rnd, top, left): a small image; a single output pixel in a corner; general; odd S (the scalar
# path); crossing block borders (256 × 32 tiles) flush to the bottom edge; exact 2:1; the identity
CASES = [(8, 7, 0, 1), (8, 1, 7, 0), (20, 18, 2, 0), (33, 29, 3, 4), (130, 117, 13, 0),
         (32, 16, 5, 9), (64, 64, 0, 0)]
# The elementwise bound 8·2⁻²⁴·A (A = D|x| resp. Dᵀ|g|, the weights are non-negative) is γ₈: a sum
# of ≤ 4 products of two weights and a value, nested as wy·(wx·v + wx'·v') + wy'·(…) — each weight
# carries ≤ 2 roundings (the kernels spend 1: one IEEE division), each product 1, each of the two
# addition levels 1: ≤ 8 roundings on any term. Derived, not measured.
K_ERR = 8 * U
# The sums' longest addition chain, as the kernel is written: 8 rows per thread and column + 2
# (the 4 column accumulators, pairwise) + 6 wave butterfly levels + 4 wave sums + the ordered
# finish over C·tiles slots, at most 3·1·5 = 15 here (S = 130: 1 × 5 tiles of 256 × 32) = 35
# additions of non-negative terms (gx² enters through an fma, unrounded); × 3 margin:
# 3·35·2⁻²⁴ ≈ 6.3e-6, tighter than grad_assemble_norms' 2e-5.
SUM_TOL = 3 * 35 * U
assert SUM_TOL <= 2e-5


def f32(v):
    return float(np.float32(v))


_inputs = {}


def case(S, rnd, top, left):
    """Per case, computed once and shared: x and g (CPU fp32, per-image scales) and the fp64
    references D x, D|x|, Dᵀg, Dᵀ|g|."""
    key = (S, rnd, top, left)
    if key not in _inputs:
        sc = torch.tensor(IMG_SCALES, dtype=F32).reshape(3, 1, 1, 1)
        x = seeded(500 + S + 3 * rnd, (3, 3, S, S)) * sc
        g = seeded(700 + S + 3 * rnd, (3, 3, S, S)) * sc
        geo = (rnd, top, left)
        _inputs[key] = dict(
            x=x, g=g, fwd=di_ref.resize_pad(x, *geo), fwd_abs=di_ref.resize_pad(x.abs(), *geo),
            adj=di_ref.resize_pad_adjoint(g, *geo), adj_abs=di_ref.resize_pad_adjoint(g.abs(), *geo))
    return _inputs[key]


def forward(x, rnd, top, left):
    from gfa_amd import ops
    y = torch.full_like(x, float("nan"))
    return ops.di_resize_pad(x, y, rnd, top, left)


def adjoint(g, rnd, top, left, l1=True, l2=True, acc=None):
    """(gx, Σ|gx|, Σgx², nonfinite) of mia_di_resize_pad_bwd_norms on device tensors."""
    from gfa_amd import ops
    N = g.shape[0]
    gx = torch.full_like(g, float("nan"))
    s1 = torch.zeros(N, device=g.device) if acc is None else acc.clone()
    s2 = torch.zeros(N, device=g.device) if acc is None else acc.clone()
    nf = torch.zeros(N, dtype=torch.int32, device=g.device)
    ops.di_resize_pad_bwd_norms(g, gx, s1 if l1 else None, s2 if l2 else None, rnd, top, left,
                                nonfinite=nf)
    return gx, s1, s2, nf


def window_mask(S, rnd, top, left):
    m = torch.zeros(S, S, dtype=torch.bool)
    m[top:top + rnd, left:left + rnd] = True
    return m


@pytest.mark.parametrize("S,rnd,top,left", CASES)
def test_di_forward_against_fp64(cuda, S, rnd, top, left):
    """|y − D x| ≤ 8·2⁻²⁴·D|x| elementwise (K_ERR above); the padding is exactly 0; rnd = S
    returns the input bit for bit."""
    c = case(S, rnd, top, left)
    y = forward(c["x"].to(cuda), rnd, top, left).cpu()
    err = (y.double() - c["fwd"]).abs()
    bound = K_ERR * c["fwd_abs"]
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"di forward S={S} rnd={rnd} ({top},{left}): worst |err| / bound = {ratio:.3f}")
    assert torch.isfinite(y).all()
    assert (err <= bound).all()
    pad = ~window_mask(S, rnd, top, left)
    assert (y[:, :, pad] == 0).all() and (c["fwd"][:, :, pad] == 0).all()
    if rnd == S:
        assert torch.equal(y.view(torch.int32), c["x"].view(torch.int32))


@pytest.mark.parametrize("S,rnd,top,left", CASES)
def test_di_adjoint_against_fp64(cuda, S, rnd, top, left):
    """|gx − Dᵀg| ≤ 8·2⁻²⁴·Dᵀ|g| elementwise; inputs that no output reads get exactly 0; rnd = S
    returns the input bit for bit."""
    c = case(S, rnd, top, left)
    gx, _, _, nf = adjoint(c["g"].to(cuda), rnd, top, left)
    gx = gx.cpu()
    err = (gx.double() - c["adj"]).abs()
    bound = K_ERR * c["adj_abs"]
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"di adjoint S={S} rnd={rnd} ({top},{left}): worst |err| / bound = {ratio:.3f}")
    assert torch.isfinite(gx).all() and not nf.any()
    assert (err <= bound).all()
    assert (gx[c["adj_abs"] == 0] == 0).all()
    if rnd == S:
        assert torch.equal(gx.view(torch.int32), c["g"].view(torch.int32))


@pytest.mark.parametrize("S,rnd,top,left", [k for k in CASES if k[2] != k[3]])
def test_di_adjoint_identity(cuda, S, rnd, top, left):
    """⟨D u, v⟩ = ⟨u, Dᵀ v⟩: in fp64 from the device outputs the two sides differ by at most
    Σ|v|·bound(u) + Σ|u|·bound(v), the elementwise bounds above. top ≠ left, so a transposed
    axis cannot pass."""
    c = case(S, rnd, top, left)
    u, v = c["x"][1:2], c["g"][1:2]
    Du = forward(u.to(cuda).contiguous(), rnd, top, left).double().cpu()
    Dtv = adjoint(v.to(cuda).contiguous(), rnd, top, left)[0].double().cpu()
    lhs = (Du * v.double()).sum().item()
    rhs = (u.double() * Dtv).sum().item()
    tol = (K_ERR * (v.double().abs() * c["fwd_abs"][1:2]).sum()
           + K_ERR * (u.double().abs() * c["adj_abs"][1:2]).sum()).item()
    print(f"di adjoint identity S={S} rnd={rnd}: <Du,v> = {lhs:.9e}, <u,Dtv> = {rhs:.9e}, "
          f"|diff| / tol = {abs(lhs - rhs) / max(tol, 1e-300):.3f}")
    assert abs(lhs - rhs) <= tol
    if rnd < S:  # the transposed placement is a different operator (the check can fail)
        wrong = di_ref.resize_pad_adjoint(v, rnd, left, top)
        assert abs(lhs - (u.double() * wrong).sum().item()) > tol


@pytest.mark.parametrize("S,rnd,top,left", CASES)
def test_di_adjoint_sums_and_determinism(cuda, S, rnd, top, left):
    """Each image's Σ|gx| and Σgx² equal the fp64 sums of the device gx to SUM_TOL relative (the
    chain is counted above). Reruns are bit-identical, an image's gx and sums do not depend on
    the other images, either sum may be absent, and the sums accumulate (+=)."""
    c = case(S, rnd, top, left)
    g = c["g"].to(cuda)
    geo = (rnd, top, left)
    gx, s1, s2, _ = adjoint(g, *geo)
    g64 = gx.double().reshape(3, -1)
    e1 = ((s1.double() - g64.abs().sum(1)).abs() / g64.abs().sum(1)).cpu()
    e2 = ((s2.double() - (g64 * g64).sum(1)).abs() / (g64 * g64).sum(1)).cpu()
    print(f"di sums S={S} rnd={rnd}: rel err of sum|gx| {e1.tolist()}, of sum gx^2 {e2.tolist()} "
          f"(bound {SUM_TOL:.2e})")
    assert e1.max() <= SUM_TOL and e2.max() <= SUM_TOL
    assert s1[0] > 10 * s1[1] > 100 * s1[2] > 0  # the per-image scales arrived
    gx_b, s1_b, s2_b, _ = adjoint(g, *geo)
    assert torch.equal(gx, gx_b) and torch.equal(s1, s1_b) and torch.equal(s2, s2_b)
    gx_1, s1_1, s2_1, _ = adjoint(g[1:2].contiguous(), *geo)
    assert torch.equal(gx_1[0], gx[1])
    assert torch.equal(s1_1[0], s1[1]) and torch.equal(s2_1[0], s2[1])
    gx_c, s1_c, s2_c, _ = adjoint(g, *geo, l2=False)
    assert torch.equal(gx_c, gx) and torch.equal(s1_c, s1) and not s2_c.any()
    gx_c, s1_c, s2_c, _ = adjoint(g, *geo, l1=False)
    assert torch.equal(gx_c, gx) and torch.equal(s2_c, s2) and not s1_c.any()
    gx_c, _, _, _ = adjoint(g, *geo, l1=False, l2=False)
    assert torch.equal(gx_c, gx)
    _, s1_a, s2_a, _ = adjoint(g, *geo, acc=torch.ones(3, device=cuda))
    assert torch.equal(s1_a, 1.0 + s1) and torch.equal(s2_a, 1.0 + s2)
    # the forward: reruns and batch independence
    x = c["x"].to(cuda)
    y = forward(x, *geo)
    assert torch.equal(y, forward(x, *geo))
    assert torch.equal(forward(x[1:2].contiguous(), *geo)[0], y[1])


def offset_copy(t):
    """The same data in a buffer 4 bytes off 16-byte alignment (the scalar path)."""
    flat = torch.zeros(t.numel() + 1, device=t.device)
    flat[1:].copy_(t.reshape(-1))
    o = flat[1:].view(t.shape)
    assert o.data_ptr() % 16 == 4 and o.is_contiguous()
    return o


@pytest.mark.parametrize("S,rnd,top,left", [(20, 18, 2, 0), (32, 16, 5, 9), (64, 64, 0, 0)])
def test_di_vector_and_scalar_paths_agree(cuda, S, rnd, top, left):
    """S % 4 == 0 on 16-byte aligned buffers moves 16-byte vectors; the same data at a 4-byte
    offset takes the scalar path. The bits, sums included, are the same."""
    c = case(S, rnd, top, left)
    geo = (rnd, top, left)
    g, x = c["g"].to(cuda), c["x"].to(cuda)
    assert g.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0
    gx, s1, s2, _ = adjoint(g, *geo)
    gx_o, s1_o, s2_o, _ = adjoint(offset_copy(g), *geo)
    assert torch.equal(gx_o, gx) and torch.equal(s1_o, s1) and torch.equal(s2_o, s2)
    assert torch.equal(forward(offset_copy(x), *geo), forward(x, *geo))


def test_di_adjoint_flags_nonfinite(cuda):
    S, rnd, top, left = 33, 29, 3, 4
    g = case(S, rnd, top, left)["g"].to(cuda).clone()
    g[1, 2, top + 10, left + 5] = float("inf")  # inside the window: the adjoint reads it
    _, s1, s2, nf = adjoint(g, rnd, top, left)
    assert nf.tolist() == [0, 1, 0]
    assert torch.isfinite(s1[0]) and torch.isfinite(s1[2])
    assert torch.isfinite(s2[0]) and torch.isfinite(s2[2])


def test_di_wrappers_reject_malformed_calls(cuda):
    from gfa_amd import ops
    x = torch.zeros(2, 3, 8, 8, device=cuda)
    y = torch.zeros_like(x)
    v = torch.zeros(2, device=cuda)
    for fn in (ops.di_resize_pad, lambda a, b, *g: ops.di_resize_pad_bwd_norms(a, b, v, v, *g)):
        for geo in ((0, 0, 0), (9, 0, 0), (7, 2, 0), (7, 0, 2), (7, -1, 0), (7.0, 0, 0)):
            with pytest.raises(ValueError):
                fn(x, y, *geo)
        with pytest.raises(ValueError):
            fn(x, x, 7, 0, 1)                                    # in place
        with pytest.raises(ValueError):
            fn(x, y[:1], 7, 0, 1)
        with pytest.raises(ValueError):
            fn(x.double(), y.double(), 7, 0, 1)
        with pytest.raises(ValueError):
            fn(x.cpu(), y, 7, 0, 1)
        with pytest.raises(ValueError):
            fn(x, y.cpu(), 7, 0, 1)
    with pytest.raises(ValueError):
        ops.di_resize_pad_bwd_norms(x, y, torch.zeros(3, device=cuda), v, 7, 0, 1)
    with pytest.raises(ValueError):
        ops.di_resize_pad_bwd_norms(x, y, v, v, 7, 0, 1,
                                    nonfinite=torch.zeros(2, device=cuda))  # not int32
    # overlapping views of one buffer: the library's own check (MIA_EINVAL)
    flat = torch.zeros(2 * 3 * 8 * 8 + 4, device=cuda)
    a, b = flat[:-4].view(2, 3, 8, 8), flat[4:].view(2, 3, 8, 8)
    with pytest.raises(Exception, match="distinct"):
        ops.di_resize_pad(a, b, 7, 0, 1)


# ---- end to end at 32² --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net32(cuda):
    from gfa_amd import networks
    return networks.build_net(SIZE, seed=0, dtype=torch.float32, device=cuda)


def test_attack_di_prob_zero_is_the_plain_attack(cuda, net32):
    """di_prob = 0 draws a schedule whose steps all run today's path: the bits of the attack
    without DI (L∞ with momentum 0, the rule DI routes to; and L2)."""
    from gfa_amd import attack
    x0, t = images()
    adv, info = attack(net32, x0, EPS, 3, target=t, alpha=ALPHA, di_prob=0.0, return_info=True)
    assert info["di_applied"] == 0 and info["di_prob"] == 0.0
    assert torch.equal(adv, attack(net32, x0, EPS, 3, target=t, alpha=ALPHA, momentum=0.0))
    kw = dict(target=t, alpha=ALPHA_L2, norm="l2")
    assert torch.equal(attack(net32, x0, EPS_L2, 3, di_prob=0.0, **kw),
                       attack(net32, x0, EPS_L2, 3, **kw))


@pytest.mark.parametrize("momentum,ti", [(None, None), (1.0, None), (None, 15), (1.0, 15)])
def test_attack_di_linf(cuda, net32, momentum, ti):
    from gfa_amd import attack
    x0, t = images()
    keep = x0.clone()
    e = f32(2 * EPS)
    kw = dict(target=t, alpha=ALPHA, momentum=momentum, ti_kernel=ti, di_prob=1.0, seed=5)
    adv, info = attack(net32, x0, EPS, 3, return_info=True, **kw)
    assert torch.equal(x0, keep)
    assert info["di_prob"] == 1.0 and info["di_resize_rate"] == 0.9 and info["di_applied"] == 3
    assert info["ti_kernel"] == ti and info["momentum"] == momentum and info["norm"] == "linf"
    check_linf(adv, x0, e)
    assert torch.equal(adv, attack(net32, x0, EPS, 3, **kw))
    alone = attack(net32, x0[:1], EPS, 3, **{**kw, "target": t[:1]})
    assert torch.equal(alone[0], adv[0])
    plain = attack(net32, x0, EPS, 3, target=t, alpha=ALPHA, ti_kernel=ti,
                   momentum=0.0 if momentum is None else momentum)
    diff = (adv != plain).float().mean().item()
    print(f"DI linf momentum={momentum} ti={ti}: differs from the attack without DI on "
          f"{diff:.4f} of pixels")
    assert diff > 0


def test_attack_di_l2(cuda, net32):
    from gfa_amd import attack
    x0, t = images()
    keep = x0.clone()
    e = f32(2 * EPS_L2)
    for ti in (None, 15):
        kw = dict(target=t, alpha=ALPHA_L2, norm="l2", ti_kernel=ti, di_prob=1.0, seed=5)
        adv, info = attack(net32, x0, EPS_L2, 3, return_info=True, **kw)
        assert torch.equal(x0, keep) and info["di_applied"] == 3 and info["norm"] == "l2"
        nrm = (adv.double() - x0.double()).reshape(2, -1).norm(dim=1)
        print(f"DI attack(norm='l2', ti={ti}, steps=3): |adv - x0| {nrm.tolist()} (e = {e})")
        assert (nrm <= e * (1 + 1e-5)).all() and (nrm > 0).all()
        assert adv.min() >= -1 and adv.max() <= 1
        assert torch.equal(adv, attack(net32, x0, EPS_L2, 3, **kw))
        alone = attack(net32, x0[:1], EPS_L2, 3, **{**kw, "target": t[:1]})
        assert torch.equal(alone[0], adv[0])
        assert not torch.equal(adv, attack(net32, x0, EPS_L2, 3, target=t, alpha=ALPHA_L2,
                                           norm="l2", ti_kernel=ti))


def test_attack_di_fp16(cuda):
    """fp16 networks (loss scale 2^8, divided out before the adjoint): the same invariants."""
    from gfa_amd import attack, networks
    net = networks.build_net(SIZE, seed=0, dtype=torch.float16, device=cuda)
    x0, t = images()
    e = f32(2 * EPS)
    for ti in (None, 15):
        kw = dict(target=t, alpha=ALPHA, ti_kernel=ti, di_prob=1.0, seed=5)
        adv, info = attack(net, x0, EPS, 3, return_info=True, **kw)
        print(f"fp16 DI attack ti={ti}: rescales {info['rescales']}, loss scale "
              f"{info['loss_scale']:g}")
        assert info["di_applied"] == 3
        check_linf(adv, x0, e)
        assert torch.equal(adv, attack(net, x0, EPS, 3, **kw))
        alone = attack(net, x0[:1], EPS, 3, **{**kw, "target": t[:1]})
        assert torch.equal(alone[0], adv[0])
        assert not torch.equal(adv, attack(net, x0, EPS, 3, target=t, alpha=ALPHA, momentum=0.0,
                                           ti_kernel=ti))
    del net
    free()


def test_attack_di_identity_schedule_is_the_plain_attack(cuda, net32):
    """Rows (S, 0, 0, 1) run both kernels as the identity (bit for bit), so the L∞ attack gives
    the bits of the attack without DI: with momentum 0 the update reads only sign(g), and with
    the smoothing the norms are taken after it, from the same bits."""
    from gfa_amd import attack
    x0, t = images()
    ident = torch.tensor([[SIZE, 0, 0, 1]] * 3)
    adv, info = attack(net32, x0, EPS, 3, target=t, alpha=ALPHA, di_schedule=ident,
                       return_info=True)
    assert info["di_applied"] == 3 and info["di_prob"] is None
    assert torch.equal(adv, attack(net32, x0, EPS, 3, target=t, alpha=ALPHA, momentum=0.0))
    kw = dict(target=t, alpha=ALPHA, momentum=1.0, ti_kernel=15)
    assert torch.equal(attack(net32, x0, EPS, 3, di_schedule=ident, **kw),
                       attack(net32, x0, EPS, 3, **kw))


# ---- one step against the oracle ----------------------------------------------------------------
DI_ROW = (29, 2, 1)
_oracle = {}


def oracle_di_gradient(ti):
    """g = Dᵀ ∇L(D x0) in fp64 (the networks of build_net(32, seed=0), linear encoder; the targets
    are those of x0 and t), smoothed with the 15-tap Gaussian when ti, and the sign-stable mask
    |g| > 1e-3·max|g| per image. Computed once."""
    if "g" not in _oracle:
        from gfa_amd.weights import make_encoder_weights, make_generator_weights, make_vgg_weights
        from oracle import attack_ref, vgg_ref
        params = (make_generator_weights(SIZE, seed=0),
                  vgg_ref.load_positional(make_vgg_weights(1234)),
                  make_encoder_weights(SIZE, seed=1))
        p64 = to64(params)
        x0, t = images()
        refs = attack_ref.Refs(*p64, x0.double(), t.double(), SIZE)
        xd = di_ref.resize_pad(x0, *DI_ROW)
        gr = attack_ref.loss_grad(*p64, xd, refs, SIZE)[1]
        _oracle["g"] = di_ref.resize_pad_adjoint(gr, *DI_ROW)
    g = _oracle["g"]
    if ti:
        g = conv64(g, gauss(15))
    stable = g.abs() > 1e-3 * g.abs().reshape(2, -1).max(dim=1).values.reshape(2, 1, 1, 1)
    return g, stable


@pytest.mark.parametrize("ti", [None, 15])
def test_attack_di_one_step_vs_oracle(cuda, net32, ti):
    """One DI step from x0 with the schedule [(29, 2, 1, 1)] is
    clamp(x0 + clamp(a·sign(−g), −e, e), −1, 1) with g = Dᵀ ∇L(D x0) wherever g's sign is stable;
    at most 2 % of the pixels may be excluded, asserted on the oracle's own mask before the
    device is looked at (0.46 % expected, 0.33 % with the smoothing)."""
    from gfa_amd import attack
    from oracle import attack_ref
    x0, t = images()
    g, stable = oracle_di_gradient(ti)
    share = 1.0 - stable.double().mean().item()
    print(f"DI one step ti={ti}: {share:.4%} of the pixels excluded (|g| <= 1e-3 max|g|)")
    assert share <= 0.02
    want = attack_ref.project_step(x0, x0, g.float(), 2 * EPS, 2 * ALPHA)
    sched = [DI_ROW + (1,)]
    for mu in (None, 1.0):
        got = attack(net32, x0, EPS, 1, target=t, alpha=ALPHA, momentum=mu, ti_kernel=ti,
                     di_schedule=sched)
        frac = (got == want).float().mean().item()
        print(f"DI steps=1 momentum={mu} ti={ti}: equal to the oracle step on {frac:.6f} of all "
              "pixels")
        assert torch.equal(got[stable], want[stable]), mu
