"""L2-ball PGD (torchattacks PGDL2) and momentum iterative FGSM (torchattacks MIFGSM) on the fused
HIP updates: the four entry points on synthetic gradients (ordered per-image norms, bit-exact
updates against the torch fp32 CPU formulas given the device-reported norms), and the attacks end to
end at 256² against the forced-branch fp64 oracle.

All image-space quantities are in [-1,1] units (e = 2·eps, a = 2·alpha)."""
import numpy as np
import pytest
import torch

from gpu_helpers import capture_vgg, engine, forced_all, free, g_masks, seeded, to64
from oracle import attack_ref

pytestmark = pytest.mark.gpu

F32 = torch.float32
IMG_SCALES = (1e4, 1.0, 1e-4)  # per-image gradient scales: cross-image mixing cannot hide


def f32(v):
    return float(np.float32(v))


# ---- synthetic gradients ------------------------------------------------------------------------
def synth(cuda, S, pf, dtype=F32, enc=True, seed=0, scales=IMG_SCALES, zero_image=None):
    """Inputs of the gradient assembly for N = len(scales) images whose gradients are scaled per
    image; ``zero_image``: that image's gradient is exactly 0."""
    from gfa_amd.weights import ENC_POOL_RES
    N, R = len(scales), S // pf
    sc = torch.tensor(scales, dtype=F32).reshape(N, 1, 1, 1)
    x0 = seeded(seed + 1, (N, 3, S, S)) * 0.9
    dx = seeded(seed + 2, (N, 3, S, S)) * 0.05 * sc
    gv = seeded(seed + 3, (N, R, R, 8)) * sc
    gv[..., 3:] = 0
    ge = seeded(seed + 4, (N, 3, ENC_POOL_RES, ENC_POOL_RES)) * sc if enc else None
    if zero_image is not None:
        dx[zero_image] = 0
        gv[zero_image] = 0
        if ge is not None:
            ge[zero_image] = 0
    d = dict(x=(x0 + dx).to(cuda), x0=x0.to(cuda), gv=gv.to(cuda, dtype),
             ge=ge.to(cuda) if enc else None, pf=pf, enc_res=ENC_POOL_RES, coef=0.37)
    return d


def assemble_norms(d, sl=slice(None), l1=True, l2=True):
    """(g, Σ|g|, Σg², nonfinite) of mia_grad_assemble_norms on the images d[sl]."""
    from gfa_amd import ops
    x, x0, gv = d["x"][sl].contiguous(), d["x0"][sl].contiguous(), d["gv"][sl].contiguous()
    ge = d["ge"][sl].contiguous() if d["ge"] is not None else None
    N = x.shape[0]
    g = torch.full_like(x, float("nan"))
    s1 = torch.zeros(N, device=x.device)
    s2 = torch.zeros(N, device=x.device)
    nf = torch.zeros(N, dtype=torch.int32, device=x.device)
    ops.grad_assemble_norms(x, x0, gv, ge, g, s1 if l1 else None, s2 if l2 else None, d["pf"],
                            d["enc_res"], d["coef"], 1.0, nonfinite=nf)
    return g, s1, s2, nf


NORM_CASES = [(32, 1, F32, True), (32, 1, torch.float16, True), (32, 1, torch.bfloat16, True),
              (20, 2, F32, False),   # 1200 elements per image: a partial last block
              (15, 3, F32, False)]   # 675 elements per image (odd): the scalar path


@pytest.mark.parametrize("S,pf,dtype,enc", NORM_CASES)
def test_grad_assemble_norms(cuda, S, pf, dtype, enc):
    """g equals mia_grad_assemble's bit for bit; each image's Σ|g| and Σg² equal the fp64 sums of
    that device g to ≤ 2e-5 relative — the longest addition chain of the reduction (≤ 3 + 2 per
    thread, 6 wave butterfly levels, 4 wave sums, ≤ 64 + 16 in the ordered finish: ≤ ~100
    additions of non-negative terms) times 2⁻²⁴ ≈ 6e-6, with 3× margin; bit-identical reruns; an
    image's norms do not depend on the other images of the call."""
    from gfa_amd import ops
    d = synth(cuda, S, pf, dtype, enc)
    g, s1, s2, nf = assemble_norms(d)
    want = ops.grad_assemble(d["x"], d["x0"], d["gv"], d["ge"], torch.empty_like(g), pf,
                             d["enc_res"], d["coef"], 1.0)
    assert torch.equal(g, want)
    assert not nf.any()
    g64 = g.double().reshape(g.shape[0], -1)
    e1 = ((s1.double() - g64.abs().sum(1)).abs() / g64.abs().sum(1)).cpu()
    e2 = ((s2.double() - (g64 * g64).sum(1)).abs() / (g64 * g64).sum(1)).cpu()
    print(f"norms S={S} pf={pf} {dtype}: rel err of sum|g| {e1.tolist()}, of sum g^2 {e2.tolist()}")
    assert e1.max() <= 2e-5 and e2.max() <= 2e-5
    # image sums span the per-image scales: nothing leaked between images
    assert s1[0] > 1e3 * s1[1] > 1e6 * s1[2] > 0
    g_b, s1_b, s2_b, _ = assemble_norms(d)
    assert torch.equal(g, g_b) and torch.equal(s1, s1_b) and torch.equal(s2, s2_b)
    g_1, s1_1, s2_1, _ = assemble_norms(d, slice(1, 2))
    assert torch.equal(g_1[0], g[1])
    assert torch.equal(s1_1[0], s1[1]) and torch.equal(s2_1[0], s2[1])
    # either output may be absent; the += convention
    _, s1_c, s2_c, _ = assemble_norms(d, l2=False)
    assert torch.equal(s1_c, s1) and not s2_c.any()
    acc = torch.ones(g.shape[0], device=cuda)
    ops.grad_assemble_norms(d["x"], d["x0"], d["gv"], d["ge"], g_b, None, acc, pf, d["enc_res"],
                            d["coef"], 1.0)
    assert torch.equal(acc, 1.0 + s2)


def test_grad_assemble_norms_flags_nonfinite(cuda):
    d = synth(cuda, 32, 1, F32, True)
    d["ge"][1, 0, 0, 0] = float("inf")
    _, _, s2, nf = assemble_norms(d)
    assert nf.tolist() == [0, 1, 0]
    assert torch.isfinite(s2[0]) and torch.isfinite(s2[2])


# ---- L2 step + projection -----------------------------------------------------------------------
def ieee_sqrt(v):
    """The correctly rounded fp32 square root on any host: through fp64 (53 ≥ 2·24 + 2 bits, so the
    second rounding is innocuous). torch.sqrt on fp32 is not correctly rounded on every CPU: the
    test host returned 1.0 for 1 − 2⁻²⁴, whose root rounds to 1 − 2⁻²⁴."""
    return torch.sqrt(v.double()).float()


def l2_ref(x, x0, g, gsq, a):
    """torchattacks PGDL2's ascent on cost = −L, fp32 CPU ops, given Σg² per image."""
    n = x.shape[0]
    gn = ieee_sqrt(gsq) + torch.tensor(1e-10, dtype=F32)
    t = (-g) / gn.reshape(n, 1, 1, 1)
    return x + torch.tensor(a, dtype=F32) * t


def l2_project_ref(adv, x0, dsq, e):
    n = adv.shape[0]
    d = adv - x0
    f = torch.minimum(torch.tensor(e, dtype=F32) / ieee_sqrt(dsq), torch.ones(n))
    return torch.clamp(x0 + d * f.reshape(n, 1, 1, 1), -1.0, 1.0)


@pytest.mark.parametrize("S,pf", [(32, 1), (15, 3)])
@pytest.mark.parametrize("a,e", [(0.5, 1.0), (1.0, 0.25)], ids=["no_shrink", "shrink"])
def test_l2_step_and_project_bit_exact(cuda, S, pf, a, e):
    """From x = x0 (‖d‖₂ = a up to rounding): a < e leaves the factor at 1, a > e shrinks. The
    device x equals the torch fp32 CPU formula evaluated with the device-reported Σg² and Σd²."""
    from gfa_amd import ops
    a, e = f32(a), f32(e)
    d = synth(cuda, S, pf, F32, False, seed=10)
    g, _, gsq, _ = assemble_norms(d)
    x0 = d["x0"]
    x = x0.clone()
    dsq = torch.zeros(3, device=cuda)
    nf = torch.zeros(3, dtype=torch.int32, device=cuda)
    ops.l2_step(x, x0, g, gsq, dsq, a, nonfinite=nf)
    adv = l2_ref(x0.cpu(), x0.cpu(), g.cpu(), gsq.cpu(), a)
    assert torch.equal(x.cpu(), adv)
    d64 = (x.double() - x0.double()).reshape(3, -1)
    err = ((dsq.double() - (d64 * d64).sum(1)).abs() / (d64 * d64).sum(1)).max().item()
    print(f"l2_step S={S}: rel err of sum d^2 {err:.2e}")
    assert err <= 2e-5
    ops.l2_project(x, x0, dsq, e)
    want = l2_project_ref(adv, x0.cpu(), dsq.cpu(), e)
    assert torch.equal(x.cpu(), want)
    nrm = (x.double() - x0.double()).reshape(3, -1).norm(dim=1)
    assert (nrm <= e * (1 + 1e-5)).all(), nrm
    if a > e:
        assert (nrm >= 0.5 * e).all()  # x0 ∈ [-0.9, 0.9]: the range clamp takes little away
    assert x.min() >= -1 and x.max() <= 1 and not nf.any()


def test_l2_zero_gradient_image_stays_put(cuda):
    """g = 0 on one image: (−0)/(0 + 1e-10) = −0, d = 0, e/0 = +inf → factor 1 — the image stays
    at x0 with no flag (PGDL2's 1e-10 keeps it finite), and the other images are untouched by it."""
    from gfa_amd import ops
    a, e = f32(1.0), f32(0.25)
    res = []
    for zero in (None, 2):
        d = synth(cuda, 32, 1, F32, True, seed=20, zero_image=zero, scales=(1.0, 3.0, 0.5))
        g, _, gsq, _ = assemble_norms(d)
        x = d["x0"].clone()
        dsq = torch.zeros(3, device=cuda)
        nf = torch.zeros(3, dtype=torch.int32, device=cuda)
        ops.l2_step(x, d["x0"], g, gsq, dsq, a, nonfinite=nf)
        ops.l2_project(x, d["x0"], dsq, e)
        assert torch.isfinite(x).all() and not nf.any()
        res.append((x, d["x0"], gsq, dsq))
    (xa, _, _, _), (xb, x0b, gsq, dsq) = res
    assert gsq[2] == 0 and dsq[2] == 0 and torch.equal(xb[2], x0b[2])
    assert torch.equal(xa[:2], xb[:2])


# ---- MI update ----------------------------------------------------------------------------------
def mi_ref(x, x0, g, l1, m, mu, a, e):
    n, plane = x.shape[0], x[0].numel()
    mean = l1 / torch.tensor(float(plane), dtype=F32)
    gh = (-g) / mean.reshape(n, 1, 1, 1)
    m = gh + torch.tensor(mu, dtype=F32) * m
    adv = x + torch.tensor(a, dtype=F32) * torch.sign(m)
    delta = torch.clamp(adv - x0, -e, e)
    return torch.clamp(x0 + delta, -1.0, 1.0), m


@pytest.mark.parametrize("S,pf", [(32, 1), (15, 3)])
@pytest.mark.parametrize("mu", [1.0, 0.5])
def test_mi_update_bit_exact(cuda, S, pf, mu):
    """Three consecutive momentum steps with fresh gradients: x and m equal the torch fp32 CPU
    formula evaluated with the device-reported Σ|g|; the ε-ball and the range hold."""
    from gfa_amd import ops
    a, e = f32(2 * 2 / 255), f32(2 * 4 / 255)
    x0 = None
    for k in range(3):
        d = synth(cuda, S, pf, F32, pf == 1, seed=30 + 10 * k)
        if x0 is None:
            x0 = d["x0"]
            x, m = x0.clone(), torch.zeros_like(x0)
            xr, mr = x0.cpu().clone(), torch.zeros_like(x0).cpu()
            nf = torch.zeros(3, dtype=torch.int32, device=cuda)
        g, l1, _, _ = assemble_norms(d)
        ops.mi_update(x, x0, g, l1, m, mu, a, e, nonfinite=nf)
        xr, mr = mi_ref(xr, x0.cpu(), g.cpu(), l1.cpu(), mr, mu, a, e)
        assert torch.equal(m.cpu(), mr), k
        assert torch.equal(x.cpu(), xr), k
        # x = fl(x0 + δ) with |δ| ≤ e: half an ulp of |x| ≤ 1 beyond e at most
        assert ((x.double() - x0.double()).abs() <= e + 2.0 ** -24).all()
        assert x.min() >= -1 and x.max() <= 1
    assert not nf.any()
    assert (x != x0).float().mean() > 0.99


def test_mi_zero_gradient_image_is_flagged(cuda):
    """mean|g| = 0: ĝ = 0/0 is NaN — the image is flagged (the engine re-runs or raises) and the
    other images' results do not change."""
    from gfa_amd import ops
    a, e = f32(2 * 2 / 255), f32(2 * 4 / 255)
    res = []
    for zero in (None, 2):
        d = synth(cuda, 32, 1, F32, True, seed=50, zero_image=zero, scales=(1.0, 3.0, 0.5))
        g, l1, _, _ = assemble_norms(d)
        x, m = d["x0"].clone(), torch.zeros_like(d["x0"])
        nf = torch.zeros(3, dtype=torch.int32, device=cuda)
        ops.mi_update(x, d["x0"], g, l1, m, 1.0, a, e, nonfinite=nf)
        res.append((x, m, nf.tolist()))
    assert res[0][2] == [0, 0, 0] and res[1][2] == [0, 0, 1]
    assert torch.equal(res[0][0][:2], res[1][0][:2]) and torch.equal(res[0][1][:2], res[1][1][:2])


def test_wrappers_reject_mismatched_shapes(cuda):
    from gfa_amd import ops
    x = torch.zeros(2, 3, 8, 8, device=cuda)
    v = torch.zeros(2, device=cuda)
    with pytest.raises(ValueError):
        ops.l2_step(x, x[:1], x, v, v, 0.1)
    with pytest.raises(ValueError):
        ops.l2_step(x, x, x, v[:1], v, 0.1)
    with pytest.raises(ValueError):
        ops.l2_project(x, x, torch.zeros(3, device=cuda), 0.1)
    with pytest.raises(ValueError):
        ops.mi_update(x, x, x, v, x[:, :, :4].contiguous(), 1.0, 0.1, 0.1)
    with pytest.raises(ValueError):
        ops.grad_assemble_norms(x, x, None, None, x, v, torch.zeros(3, device=cuda), 1, 16, 1.0)
    with pytest.raises(ValueError):
        ops.grad_assemble_norms(x, x, None, None, x, v, v, 3, 16, 1.0)  # pf does not divide S


# ---- end to end at 256² -------------------------------------------------------------------------
SIZE = 256
EPS_L2, ALPHA_L2 = 1.0, 0.2  # ‖0.02·noise‖₂ ≈ 5.1 > e = 2: the second teacher-forced step shrinks


class forced_gv(forced_all):
    """forced_all for the linear encoder (no branches in E): generator LeakyReLUs and both VGG
    passes follow the device run."""

    def __init__(self, eng, vgg_cap):
        from oracle import forcing, stylegan2_ref, vgg_ref
        self.audit = forcing.audit()
        self.dtype = eng.dtype
        self.ctx = [self.audit, stylegan2_ref.forced_masks(g_masks(eng.G, eng.ws)),
                    vgg_ref.forced_masks(vgg_cap.masks[-2:])]


def images():
    x0 = torch.cat([seeded(810, (1, 3, SIZE, SIZE)), 0.6 * seeded(811, (1, 3, SIZE, SIZE))])
    t = torch.cat([seeded(812, (1, 3, SIZE, SIZE)), seeded(813, (1, 3, SIZE, SIZE))])
    return x0, t


def l2_full_ref(x, x0, g, a, e):
    """One PGDL2 step on cost = −L from an fp32 gradient, torch fp32 CPU ops."""
    n = x.shape[0]
    gsq = (g * g).reshape(n, -1).sum(1)
    adv = l2_ref(x, x0, g, gsq, a)
    d = adv - x0
    return l2_project_ref(adv, x0, (d * d).reshape(n, -1).sum(1), e)


# (dtype, 2 × the gradient bound the suite enforces at 256²: test_gpu_parity 1e-4 at fp32,
#  test_gpu_lowp_oracle CASES 1e-2 at fp16, forced-flip gap bound, flip fraction bound)
TF_CASES = [(torch.float32, 2e-4, None, None), (torch.float16, 2e-2, 1e-2, 2e-3)]
_oracle_g0 = {}


@pytest.mark.parametrize("dtype,bound,gap_tol,frac_tol", TF_CASES)
def test_l2_teacher_forced_vs_oracle(cuda, dtype, bound, gap_tol, frac_tol):
    """One L2 step from x0 and one from x0 + 0.02·noise (shrunk: ‖d‖₂ > e): the device step against
    the PGDL2 formula on the forced-branch fp64 oracle gradient. ‖û − v̂‖ ≤ 2‖u − v‖/‖v‖ for the
    normalised directions, and the clamp and the radial projection are non-expansive, so
    ‖adv_dev − adv_ref‖₂ / ‖adv_ref − x0‖₂ ≤ 2 × the gradient bound."""
    eng, params = engine(SIZE, dtype, cuda, encoder="synthetic")
    p64 = to64(params)
    x0, t = images()
    e, a = f32(2 * EPS_L2), f32(2 * ALPHA_L2)
    eng.prepare(x0.to(cuda), t.to(cuda))
    refs = attack_ref.Refs(*p64, x0.double(), t.double(), SIZE)
    starts = [x0, (x0 + 0.02 * seeded(814, x0.shape)).clamp(-1, 1)]
    for k, x in enumerate(starts):
        xd = x.to(cuda).clone()
        with capture_vgg(eng.V) as cap:
            eng.step_l2(xd, a, e)
        fa = forced_gv(eng, cap)
        with fa:
            _, gr = attack_ref.loss_grad(*p64, x.double(), refs, SIZE)
        print(f"{dtype} start {k}: " + (fa.check() if gap_tol is None
                                        else fa.check(tol=gap_tol, frac=frac_tol)))
        if k == 0 and dtype == torch.float32:
            _oracle_g0["g"] = gr
        want = l2_full_ref(x, x0, gr.float(), a, e)
        got = xd.cpu()
        num = (got.double() - want.double()).reshape(2, -1).norm(dim=1)
        den = (want.double() - x0.double()).reshape(2, -1).norm(dim=1)
        dn = (got.double() - x0.double()).reshape(2, -1).norm(dim=1)
        print(f"{dtype} L2 teacher-forced start {k}: ratio {(num / den).tolist()} (bound {bound:g})"
              f", |adv - x0| {dn.tolist()}")
        assert (num / den <= bound).all()
        assert (dn <= e * (1 + 1e-5)).all()
        if k == 1:
            assert (den > 0.9 * e).all()  # the shrink was active
    assert not eng.overflowed()
    del eng
    free()


@pytest.fixture(scope="module")
def net32(cuda):
    from gfa_amd import networks
    return networks.build_net(SIZE, seed=0, dtype=torch.float32, device=cuda)


def test_attack_l2(cuda, net32):
    from gfa_amd import attack, pgd
    x0, t = images()
    keep = x0.clone()
    e = f32(2 * EPS_L2)
    kw = dict(target=t, alpha=ALPHA_L2, norm="l2")
    adv, info = attack(net32, x0, EPS_L2, 3, return_info=True, **kw)
    assert torch.equal(x0, keep) and info["norm"] == "l2" and info["momentum"] is None
    nrm = (adv.double() - x0.double()).reshape(2, -1).norm(dim=1)
    print(f"attack(norm='l2', steps=3): |adv - x0| {nrm.tolist()} (e = {e})")
    assert (nrm <= e * (1 + 1e-5)).all() and (nrm > 0).all()
    assert adv.min() >= -1 and adv.max() <= 1
    assert torch.equal(adv, attack(net32, x0, EPS_L2, 3, **kw))
    alone = attack(net32, x0[:1], EPS_L2, 3, target=t[:1], alpha=ALPHA_L2, norm="l2")
    assert torch.equal(alone[0], adv[0])
    rs = attack(net32, x0, EPS_L2, 3, random_start=True, seed=5, **kw)
    assert torch.equal(rs, attack(net32, x0, EPS_L2, 3, random_start=True, seed=5, **kw))
    assert not torch.equal(rs, adv)
    nrm = (rs.double() - x0.double()).reshape(2, -1).norm(dim=1)
    assert (nrm <= e * (1 + 1e-5)).all()
    noise = pgd.make_start_noise(tuple(x0.shape), 5, "l2")
    assert (noise.reshape(2, -1).norm(dim=1) <= 1).all()


def test_attack_momentum(cuda, net32):
    from gfa_amd import attack, pgd
    x0, t = images()
    eps, alpha = 8 / 255, 2 / 255
    e = f32(2 * eps)
    kw = dict(target=t, alpha=alpha)
    adv, info = attack(net32, x0, eps, 3, momentum=1.0, return_info=True, **kw)
    assert info["momentum"] == 1.0
    assert ((adv - x0).abs() <= e + 1e-7).all() and adv.min() >= -1 and adv.max() <= 1
    assert torch.equal(adv, attack(net32, x0, eps, 3, momentum=1.0, **kw))
    plain = attack(net32, x0, eps, 3, **kw)
    assert not torch.equal(adv, plain)
    eng = pgd.AttackEngine(net32.encoder.impl, net32.decoder.impl, net32.vgg.impl)
    assert torch.equal(plain, eng.run(x0.to(cuda), t.to(cuda), 3, eps, alpha).cpu())
    # one step: m = ĝ has −g's sign, so any μ gives the plain sign step where the sign is stable
    if "g" not in _oracle_g0:
        eng0, params = engine(SIZE, torch.float32, cuda, encoder="synthetic")
        p64 = to64(params)
        refs = attack_ref.Refs(*p64, x0.double(), t.double(), SIZE)
        _oracle_g0["g"] = attack_ref.loss_grad(*p64, x0.double(), refs, SIZE)[1]
        del eng0
    gr = _oracle_g0["g"]
    stable = gr.abs() > 1e-3 * gr.abs().reshape(2, -1).max(dim=1).values.reshape(2, 1, 1, 1)
    one = attack(net32, x0, eps, 1, **kw)
    for mu in (0.0, 1.0, 2.5):
        got = attack(net32, x0, eps, 1, momentum=mu, **kw)
        assert torch.equal(got[stable], one[stable]), mu
        frac = (got == one).float().mean().item()
        print(f"MI steps=1 mu={mu}: equal to the plain step on {frac:.6f} of all pixels, "
              f"{int(stable.sum())} sign-stable")
        assert frac > 0.999


def test_attack_l2_fp16(cuda):
    """fp16 networks (loss scale 2^8, unscaled before the norms): the same invariants."""
    from gfa_amd import attack, networks
    net = networks.build_net(SIZE, seed=0, dtype=torch.float16, device=cuda)
    x0, t = images()
    e = f32(2 * EPS_L2)
    adv, info = attack(net, x0, EPS_L2, 3, target=t, alpha=ALPHA_L2, norm="l2", return_info=True)
    nrm = (adv.double() - x0.double()).reshape(2, -1).norm(dim=1)
    print(f"fp16 attack(norm='l2'): |adv - x0| {nrm.tolist()}, rescales {info['rescales']}")
    assert (nrm <= e * (1 + 1e-5)).all() and (nrm > 0).all()
    assert torch.equal(adv, attack(net, x0, EPS_L2, 3, target=t, alpha=ALPHA_L2, norm="l2"))
    del net
    free()
