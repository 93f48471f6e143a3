"""Translation-invariant attacks (torchattacks TIFGSM without input diversity): the fused
separable blur mia_ti_smooth_norms against F.conv2d in fp64, its ordered per-image sums, and the
attacks end to end at 32² (L∞ with and without momentum, L2, fp16, one step against the oracle).

All image-space quantities are in [-1,1] units (e = 2·eps, a = 2·alpha)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_helpers import free, seeded, to64

pytestmark = pytest.mark.gpu

F32 = torch.float32
U = 2.0 ** -24
IMG_SCALES = (1e4, 1.0, 1e-4)  # per-image gradient scales: cross-image mixing cannot hide
# (H, W, K): narrower than the kernel; a partial tile; odd sizes (the scalar path) crossing tile
# borders both ways; the largest K; the identity
CASES = [(8, 8, 15), (20, 20, 3), (67, 35, 15), (64, 64, 63), (32, 32, 1)]


def f32(v):
    return float(np.float32(v))


def gauss(K):
    from gfa_amd.pgd import ti_gaussian_taps
    return ti_gaussian_taps(K, 3.0).float()


def conv64(g, w32):
    """(taps ⊗ taps) ⋆ g per plane in fp64 on the CPU, zero padded, from the fp32 taps."""
    N, C, H, W = g.shape
    w = w32.double().cpu()
    k2 = torch.outer(w, w)[None, None]
    out = F.conv2d(g.double().cpu().reshape(N * C, 1, H, W), k2, padding=w.numel() // 2)
    return out.reshape(N, C, H, W)


_inputs = {}


def case(H, W, K):
    """Per case, computed once and shared: g (CPU fp32, per-image scales), the fp32 taps, the fp64
    reference and the bound's magnitude A = conv(|g|, |w| ⊗ |w|)."""
    key = (H, W, K)
    if key not in _inputs:
        sc = torch.tensor(IMG_SCALES, dtype=F32).reshape(3, 1, 1, 1)
        g = seeded(100 + H + 7 * K, (3, 3, H, W)) * sc
        w = gauss(K)
        _inputs[key] = dict(g=g, w=w, ref=conv64(g, w), A=conv64(g.abs(), w.abs()))
    return _inputs[key]


def smooth(g, w, l1=True, l2=True, acc=None):
    """(gs, Σ|gs|, Σgs², nonfinite) of mia_ti_smooth_norms on device tensors."""
    from gfa_amd import ops
    N = g.shape[0]
    gs = torch.full_like(g, float("nan"))
    s1 = torch.zeros(N, device=g.device) if acc is None else acc.clone()
    s2 = torch.zeros(N, device=g.device) if acc is None else acc.clone()
    nf = torch.zeros(N, dtype=torch.int32, device=g.device)
    ops.ti_smooth_norms(g, w, gs, s1 if l1 else None, s2 if l2 else None, nonfinite=nf)
    return gs, s1, s2, nf


@pytest.mark.parametrize("H,W,K", CASES)
def test_ti_smooth_against_fp64(cuda, H, W, K):
    """|gs − ref| ≤ 2·(K+3)·2⁻²⁴·A elementwise: γ_K of a K-term fp32 dot product in any order,
    applied to two chained passes (the second pass also carries the first one's error through
    Σ|w| = 1-weighted taps), so the bound needs no measurement. K = 1 is the identity."""
    c = case(H, W, K)
    gs, _, _, nf = smooth(c["g"].to(cuda), c["w"].to(cuda))
    err = (gs.double().cpu() - c["ref"]).abs()
    bound = 2 * (K + 3) * U * c["A"]
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"ti_smooth {H}x{W} K={K}: worst |err| / bound = {ratio:.3f}")
    assert torch.isfinite(gs).all() and not nf.any()
    assert (err <= bound).all()
    if K == 1:
        assert c["w"].tolist() == [1.0]
        assert torch.equal(gs.cpu(), c["g"])


def test_ti_smooth_asymmetric_taps(cuda):
    """Random signed taps (no symmetry to hide a flipped or transposed pass): the F.conv2d
    convention, out[y, x] = Σ w[i]·w[j]·g[y + i − r, x + j − r], under the same bound."""
    H, W, K = 67, 35, 15
    g = case(H, W, K)["g"]
    w = seeded(7, (K,))
    gs, _, _, _ = smooth(g.to(cuda), w.to(cuda))
    err = (gs.double().cpu() - conv64(g, w)).abs()
    bound = 2 * (K + 3) * U * conv64(g.abs(), w.abs())
    print(f"ti_smooth asymmetric taps: worst |err| / bound = {(err / bound).max().item():.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("H,W,K", CASES)
def test_ti_smooth_sums_and_determinism(cuda, H, W, K):
    """Each image's Σ|gs| and Σgs² equal the fp64 sums of the device gs to ≤ 6e-6 relative: the
    longest addition chain is 16 per thread + 6 wave butterfly levels + 4 wave sums + the ordered
    finish over C·tiles ≤ 6 slots here = 32 additions of non-negative terms (gs² enters through an
    fma, unrounded), 32·2⁻²⁴ ≈ 1.9e-6, with 3× margin — shorter than grad_assemble_norms' ≈ 100.
    Reruns are bit-identical, an image's gs and sums do not depend on the other images, either
    sum may be absent, and the sums accumulate (+=)."""
    c = case(H, W, K)
    g, w = c["g"].to(cuda), c["w"].to(cuda)
    gs, s1, s2, _ = smooth(g, w)
    g64 = gs.double().reshape(3, -1)
    e1 = ((s1.double() - g64.abs().sum(1)).abs() / g64.abs().sum(1)).cpu()
    e2 = ((s2.double() - (g64 * g64).sum(1)).abs() / (g64 * g64).sum(1)).cpu()
    print(f"ti sums {H}x{W} K={K}: rel err of sum|gs| {e1.tolist()}, of sum gs^2 {e2.tolist()}")
    assert e1.max() <= 6e-6 and e2.max() <= 6e-6
    assert s1[0] > 1e3 * s1[1] > 1e6 * s1[2] > 0
    gs_b, s1_b, s2_b, _ = smooth(g, w)
    assert torch.equal(gs, gs_b) and torch.equal(s1, s1_b) and torch.equal(s2, s2_b)
    gs_1, s1_1, s2_1, _ = smooth(g[1:2].contiguous(), w)
    assert torch.equal(gs_1[0], gs[1])
    assert torch.equal(s1_1[0], s1[1]) and torch.equal(s2_1[0], s2[1])
    gs_c, s1_c, s2_c, _ = smooth(g, w, l2=False)
    assert torch.equal(gs_c, gs) and torch.equal(s1_c, s1) and not s2_c.any()
    gs_c, s1_c, s2_c, _ = smooth(g, w, l1=False)
    assert torch.equal(gs_c, gs) and torch.equal(s2_c, s2) and not s1_c.any()
    gs_c, _, _, _ = smooth(g, w, l1=False, l2=False)
    assert torch.equal(gs_c, gs)
    _, s1_a, s2_a, _ = smooth(g, w, acc=torch.ones(3, device=cuda))
    assert torch.equal(s1_a, 1.0 + s1) and torch.equal(s2_a, 1.0 + s2)


def test_ti_smooth_vector_and_scalar_paths_agree(cuda):
    """W % 4 == 0 on 16-byte aligned buffers moves 16-byte vectors; the same data at a 4-byte
    offset takes the scalar path. The bits, sums included, are the same."""
    H, W, K = 20, 20, 3
    c = case(H, W, K)
    g, w = c["g"].to(cuda), c["w"].to(cuda)
    gs, s1, s2, _ = smooth(g, w)
    flat = torch.zeros(g.numel() + 1, device=cuda)
    flat[1:].copy_(g.reshape(-1))
    g_off = flat[1:].view(g.shape)
    assert g_off.data_ptr() % 16 == 4 and g_off.is_contiguous()
    gs_o, s1_o, s2_o, _ = smooth(g_off, w)
    assert torch.equal(gs_o, gs) and torch.equal(s1_o, s1) and torch.equal(s2_o, s2)


@pytest.mark.parametrize("H,W,K", CASES)
def test_ti_smooth_is_self_adjoint(cuda, H, W, K):
    """Symmetric taps and zero padding: ⟨B u, v⟩ = ⟨u, B v⟩. In fp64 from the device outputs the
    two sides differ by at most Σ|v|·bound(u) + Σ|u|·bound(v), the elementwise bounds above."""
    c = case(H, W, K)
    u = c["g"][1:2]
    v = seeded(300 + H + K, u.shape)
    w = c["w"]
    Bu, _, _, _ = smooth(u.to(cuda).contiguous(), w.to(cuda))
    Bv, _, _, _ = smooth(v.to(cuda), w.to(cuda))
    lhs = (Bu.double().cpu() * v.double()).sum().item()
    rhs = (u.double() * Bv.double().cpu()).sum().item()
    k = 2 * (K + 3) * U
    tol = (k * (v.double().abs() * c["A"][1:2]).sum()
           + k * (u.double().abs() * conv64(v.abs(), w.abs())).sum()).item()
    print(f"ti adjoint {H}x{W} K={K}: <Bu,v> = {lhs:.9e}, <u,Bv> = {rhs:.9e}, "
          f"|diff| / tol = {abs(lhs - rhs) / max(tol, 1e-300):.3f}")
    assert abs(lhs - rhs) <= tol


def test_ti_smooth_flags_nonfinite(cuda):
    c = case(67, 35, 15)
    g = c["g"].to(cuda).clone()
    g[1, 2, 40, 17] = float("inf")
    _, s1, s2, nf = smooth(g, c["w"].to(cuda))
    assert nf.tolist() == [0, 1, 0]
    assert torch.isfinite(s1[0]) and torch.isfinite(s1[2])
    assert torch.isfinite(s2[0]) and torch.isfinite(s2[2])


def test_ti_wrapper_rejects_malformed_calls(cuda):
    from gfa_amd import ops
    g = torch.zeros(2, 3, 8, 8, device=cuda)
    gs = torch.zeros_like(g)
    v = torch.zeros(2, device=cuda)
    w = gauss(3).to(cuda)
    with pytest.raises(ValueError):
        ops.ti_smooth_norms(g, w, g, v, v)                       # in place
    with pytest.raises(ValueError):
        ops.ti_smooth_norms(g, w, gs[:1], v, v)
    with pytest.raises(ValueError):
        ops.ti_smooth_norms(g, torch.zeros(4, device=cuda), gs, v, v)   # even K
    with pytest.raises(ValueError):
        ops.ti_smooth_norms(g, torch.zeros(65, device=cuda), gs, v, v)
    with pytest.raises(ValueError):
        ops.ti_smooth_norms(g, w.double(), gs, v, v)
    with pytest.raises(ValueError):
        ops.ti_smooth_norms(g, w, gs, torch.zeros(3, device=cuda), v)
    with pytest.raises(ValueError):
        ops.ti_smooth_norms(g, w.cpu(), gs, v, v)


# ---- end to end at 32² --------------------------------------------------------------------------
SIZE = 32
EPS, ALPHA = 8 / 255, 2 / 255
EPS_L2, ALPHA_L2 = 1.0, 0.2
SEEDS = (910, 911, 912, 913)  # x0[0], x0[1], t[0], t[1]


def images():
    x0 = torch.cat([seeded(SEEDS[0], (1, 3, SIZE, SIZE)), 0.6 * seeded(SEEDS[1], (1, 3, SIZE, SIZE))])
    t = torch.cat([seeded(SEEDS[2], (1, 3, SIZE, SIZE)), seeded(SEEDS[3], (1, 3, SIZE, SIZE))])
    return x0, t


@pytest.fixture(scope="module")
def net32(cuda):
    from gfa_amd import networks
    return networks.build_net(SIZE, seed=0, dtype=torch.float32, device=cuda)


def check_linf(adv, x0, e):
    assert ((adv - x0).abs() <= e + 1e-7).all() and adv.min() >= -1 and adv.max() <= 1


@pytest.mark.parametrize("momentum", [None, 1.0])
def test_attack_ti_linf(cuda, net32, momentum):
    from gfa_amd import attack
    x0, t = images()
    keep = x0.clone()
    e = f32(2 * EPS)
    kw = dict(target=t, alpha=ALPHA, momentum=momentum, ti_kernel=15)
    adv, info = attack(net32, x0, EPS, 3, return_info=True, **kw)
    assert torch.equal(x0, keep)
    assert info["ti_kernel"] == 15 and info["momentum"] == momentum and info["norm"] == "linf"
    check_linf(adv, x0, e)
    assert torch.equal(adv, attack(net32, x0, EPS, 3, **kw))
    alone = attack(net32, x0[:1], EPS, 3, target=t[:1], alpha=ALPHA, momentum=momentum,
                   ti_kernel=15)
    assert torch.equal(alone[0], adv[0])
    plain = attack(net32, x0, EPS, 3, target=t, alpha=ALPHA,
                   momentum=0.0 if momentum is None else momentum)
    diff = (adv != plain).float().mean().item()
    print(f"TI linf momentum={momentum}: differs from the unsmoothed attack on {diff:.4f} of pixels")
    assert diff > 0
    if momentum is None:  # decay 0.0, torchattacks TIFGSM's default
        assert torch.equal(adv, attack(net32, x0, EPS, 3, target=t, alpha=ALPHA, momentum=0.0,
                                       ti_kernel=15))


def test_attack_ti_l2(cuda, net32):
    from gfa_amd import attack
    x0, t = images()
    keep = x0.clone()
    e = f32(2 * EPS_L2)
    kw = dict(target=t, alpha=ALPHA_L2, norm="l2", ti_kernel=15)
    adv, info = attack(net32, x0, EPS_L2, 3, return_info=True, **kw)
    assert torch.equal(x0, keep) and info["ti_kernel"] == 15 and info["norm"] == "l2"
    nrm = (adv.double() - x0.double()).reshape(2, -1).norm(dim=1)
    print(f"TI attack(norm='l2', steps=3): |adv - x0| {nrm.tolist()} (e = {e})")
    assert (nrm <= e * (1 + 1e-5)).all() and (nrm > 0).all()
    assert adv.min() >= -1 and adv.max() <= 1
    assert torch.equal(adv, attack(net32, x0, EPS_L2, 3, **kw))
    alone = attack(net32, x0[:1], EPS_L2, 3, target=t[:1], alpha=ALPHA_L2, norm="l2",
                   ti_kernel=15)
    assert torch.equal(alone[0], adv[0])
    assert not torch.equal(adv, attack(net32, x0, EPS_L2, 3, target=t, alpha=ALPHA_L2, norm="l2"))


def test_attack_ti_fp16(cuda):
    """fp16 networks (loss scale 2^8, divided out before the smoothing): the same invariants."""
    from gfa_amd import attack, networks
    net = networks.build_net(SIZE, seed=0, dtype=torch.float16, device=cuda)
    x0, t = images()
    e = f32(2 * EPS)
    kw = dict(target=t, alpha=ALPHA, ti_kernel=15)
    adv, info = attack(net, x0, EPS, 3, return_info=True, **kw)
    print(f"fp16 TI attack: rescales {info['rescales']}, loss scale {info['loss_scale']:g}")
    assert info["ti_kernel"] == 15
    check_linf(adv, x0, e)
    assert torch.equal(adv, attack(net, x0, EPS, 3, **kw))
    alone = attack(net, x0[:1], EPS, 3, target=t[:1], alpha=ALPHA, ti_kernel=15)
    assert torch.equal(alone[0], adv[0])
    assert not torch.equal(adv, attack(net, x0, EPS, 3, target=t, alpha=ALPHA, momentum=0.0))
    del net
    free()


def oracle_smoothed_gradient():
    """ĝ = W ⋆ ∇L at x0 in fp64 (the networks of build_net(32, seed=0), linear encoder) and the
    sign-stable mask |ĝ| > 1e-3·max|ĝ| per image."""
    from gfa_amd.weights import make_encoder_weights, make_generator_weights, make_vgg_weights
    from oracle import attack_ref, vgg_ref
    params = (make_generator_weights(SIZE, seed=0),
              vgg_ref.load_positional(make_vgg_weights(1234)), make_encoder_weights(SIZE, seed=1))
    p64 = to64(params)
    x0, t = images()
    refs = attack_ref.Refs(*p64, x0.double(), t.double(), SIZE)
    gr = attack_ref.loss_grad(*p64, x0.double(), refs, SIZE)[1]
    gh = conv64(gr, gauss(15))
    stable = gh.abs() > 1e-3 * gh.abs().reshape(2, -1).max(dim=1).values.reshape(2, 1, 1, 1)
    return gh, stable


def test_attack_ti_one_step_vs_oracle(cuda, net32):
    """One TI step from x0 is clamp(x0 + clamp(a·sign(−ĝ), −e, e), −1, 1) wherever ĝ's sign is
    stable; at most 2 % of the pixels may be excluded (≈ 0.3 % expected for Gaussian-like values:
    P(|z| < 1e-3·max) with max ≈ 3.5 σ)."""
    from gfa_amd import attack
    from oracle import attack_ref
    x0, t = images()
    gh, stable = oracle_smoothed_gradient()
    share = 1.0 - stable.double().mean().item()
    print(f"TI one step: {share:.4%} of the pixels excluded (|g^| <= 1e-3 max|g^|)")
    assert share <= 0.02
    want = attack_ref.project_step(x0, x0, gh.float(), 2 * EPS, 2 * ALPHA)
    for mu in (None, 1.0):
        got = attack(net32, x0, EPS, 1, target=t, alpha=ALPHA, momentum=mu, ti_kernel=15)
        frac = (got == want).float().mean().item()
        print(f"TI steps=1 momentum={mu}: equal to the oracle step on {frac:.6f} of all pixels")
        assert torch.equal(got[stable], want[stable]), mu
