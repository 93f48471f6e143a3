"""The JPEG stage on the GPU: mia_jpeg_roundtrip and mia_jpeg_bwd_norms bit for bit against the
fp32 torch reference (tests/jpeg_ref.py, the same operation order), the adjoint's ordered per-image
sums, the engine's stage order at 32² and the library's own argument checks.

Shapes: S = 8 is one 8 × 8 block, S = 24 a remainder of the 64 × 32 tile, S = 72 crosses the tile
both ways and leaves a remainder; N = 3 runs three images of different content."""
import ctypes

import numpy as np
import pytest
import torch

import jpeg_ref
from gpu_helpers import engine, seeded

pytestmark = pytest.mark.gpu

F32 = torch.float32
U = 2.0 ** -24
SIZES = (8, 24, 72)
QUALITIES = (10, 75, 100)
SIZE, EPS, ALPHA = 32, 8 / 255, 2 / 255
# The sums' longest addition chain, as the kernel is written: 6 per thread and lane (2 positions ×
# 3 planes) + 2 (the 4 lane accumulators, pairwise) + 6 wave butterfly levels + 4 wave sums + the
# ordered finish over the tiles, at most 2 × 3 = 6 slots here (S = 72) = 24 additions of
# non-negative terms (gx² enters through an fma, unrounded); × 3 margin: 3·24·2⁻²⁴ ≈ 4.3e-6.
SUM_TOL = 3 * 24 * U


def f32(v):
    return float(np.float32(v))


def bits(t):
    return t.contiguous().view(torch.int32)


def qtab(q):
    from gfa_amd import jpeg_quant_tables
    return jpeg_quant_tables(q).to(F32)


_inputs = {}


def case(S, q):
    """Per (S, q), computed once and shared: three images (CPU fp32) — natural statistics with
    saturated ±1 regions; uniform noise beyond [-1,1] (the clamp); half levels (2n − 1)/255 − 1,
    the floor's own boundary, where (x + 1)·127.5 + 0.5 is an exact integer in fp32 on most
    elements and an ulp off on the rest — a gradient with per-image scales, and the fp32 references
    J(x) and J′(x)ᵀg."""
    key = (S, q)
    if key not in _inputs:
        a = (jpeg_ref.test_image(40 + S, max(S, 16))[:, :, :S, :S] * 2.5).clamp(-1.0, 1.0)
        b = seeded(50 + S, (1, 3, S, S)) * 1.1
        gen = torch.Generator().manual_seed(60 + S)
        n = torch.randint(1, 256, (1, 3, S, S), generator=gen).double()
        c = ((2 * n - 1) / 255 - 1).to(F32)
        x = torch.cat([a, b, c]).contiguous()
        assert (a.abs() == 1).float().mean() > 0.02 and (b.abs() > 1).any()
        t = (c + 1.0) * 127.5 + 0.5
        assert (t == torch.round(t)).float().mean() > 0.4 and (t != torch.round(t)).any()
        sc = torch.tensor((1e3, 1.0, 1e-3), dtype=F32).reshape(3, 1, 1, 1)
        g = seeded(70 + S, (3, 3, S, S)) * sc
        y, _ = jpeg_ref.roundtrip32(x, qtab(q))
        _inputs[key] = dict(x=x, g=g, y=y, gx=jpeg_ref.adjoint32(x, g, qtab(q)))
    return _inputs[key]


def forward(x, q):
    from gfa_amd import ops
    return ops.jpeg_roundtrip(x, torch.full_like(x, float("nan")), qtab(q).to(x.device))


def adjoint(x, g, q, l1=True, l2=True, acc=None):
    """(gx, Σ|gx|, Σgx², nonfinite) of mia_jpeg_bwd_norms on device tensors."""
    from gfa_amd import ops
    N = g.shape[0]
    gx = torch.full_like(g, float("nan"))
    s1 = torch.zeros(N, device=g.device) if acc is None else acc.clone()
    s2 = torch.zeros(N, device=g.device) if acc is None else acc.clone()
    nf = torch.zeros(N, dtype=torch.int32, device=g.device)
    ops.jpeg_bwd_norms(x, g, gx, qtab(q).to(g.device), s1 if l1 else None, s2 if l2 else None,
                       nonfinite=nf)
    return gx, s1, s2, nf


def offset_copy(t):
    """The same data in a buffer 4 bytes off 16-byte alignment (the scalar path)."""
    flat = torch.zeros(t.numel() + 1, device=t.device)
    flat[1:].copy_(t.reshape(-1))
    o = flat[1:].view(t.shape)
    assert o.data_ptr() % 16 == 4 and o.is_contiguous()
    return o


@pytest.mark.parametrize("q", QUALITIES)
@pytest.mark.parametrize("S", SIZES)
def test_jpeg_roundtrip_bit_for_bit(cuda, S, q):
    """y = J(x) equals the fp32 torch reference bit for bit, for N = 3 and N = 1, on the vector
    and the scalar load path; reruns are identical and an image does not depend on its batch
    neighbours."""
    c = case(S, q)
    x = c["x"].to(cuda)
    assert x.data_ptr() % 16 == 0
    y = forward(x, q)
    diff = int((bits(y.cpu()) != bits(c["y"])).sum())
    print(f"jpeg roundtrip S={S} q={q}: {diff} of {y.numel()} elements differ from the reference")
    assert diff == 0
    assert torch.equal(bits(forward(x, q)), bits(y))
    for n in range(3):
        assert torch.equal(bits(forward(x[n:n + 1].contiguous(), q)[0]), bits(y[n]))
    assert torch.equal(bits(forward(offset_copy(x), q)), bits(y))
    assert torch.equal(bits(forward(offset_copy(x[1:2]), q)[0]), bits(y[1]))


def test_jpeg_compress_is_the_roundtrip(cuda):
    from gfa_amd import jpeg_compress
    c = case(24, 75)
    x = c["x"].to(cuda)
    keep = x.clone()
    y = jpeg_compress(x, 75)
    assert torch.equal(bits(y.cpu()), bits(c["y"])) and torch.equal(x, keep)
    assert torch.equal(jpeg_compress(x.double(), 75), y) and y.dtype == F32
    assert not torch.equal(jpeg_compress(x, 10), y)


@pytest.mark.parametrize("q", QUALITIES)
@pytest.mark.parametrize("S", SIZES)
def test_jpeg_adjoint_bit_for_bit_and_sums(cuda, S, q):
    """gx equals the fp32 torch reference bit for bit (N = 3 and N = 1, both load paths); each
    image's Σ|gx| and Σgx² equal the fp64 sums of the kernel's own gx to SUM_TOL relative (the
    chain is counted above); reruns are identical, an image's gx and sums do not depend on the
    other images, either sum or both may be absent with the same gx, and the sums accumulate."""
    c = case(S, q)
    x, g = c["x"].to(cuda), c["g"].to(cuda)
    gx, s1, s2, nf = adjoint(x, g, q)
    diff = int((bits(gx.cpu()) != bits(c["gx"])).sum())
    print(f"jpeg adjoint S={S} q={q}: {diff} of {gx.numel()} elements differ from the reference")
    assert diff == 0 and not nf.any()
    g64 = gx.double().reshape(3, -1)
    r1, r2 = g64.abs().sum(1), (g64 * g64).sum(1)
    assert (r1 > 0).all()
    e1 = ((s1.double() - r1).abs() / r1).cpu()
    e2 = ((s2.double() - r2).abs() / r2).cpu()
    print(f"jpeg sums S={S} q={q}: rel err of sum|gx| {e1.tolist()}, of sum gx^2 {e2.tolist()} "
          f"(bound {SUM_TOL:.2e})")
    assert e1.max() <= SUM_TOL and e2.max() <= SUM_TOL
    gx_b, s1_b, s2_b, _ = adjoint(x, g, q)
    assert torch.equal(bits(gx), bits(gx_b)) and torch.equal(s1, s1_b) and torch.equal(s2, s2_b)
    for n in range(3):
        gx_1, s1_1, s2_1, _ = adjoint(x[n:n + 1].contiguous(), g[n:n + 1].contiguous(), q)
        assert torch.equal(bits(gx_1[0]), bits(gx[n]))
        assert torch.equal(s1_1[0], s1[n]) and torch.equal(s2_1[0], s2[n])
    gx_c, s1_c, s2_c, _ = adjoint(x, g, q, l2=False)
    assert torch.equal(bits(gx_c), bits(gx)) and torch.equal(s1_c, s1) and not s2_c.any()
    gx_c, s1_c, s2_c, _ = adjoint(x, g, q, l1=False)
    assert torch.equal(bits(gx_c), bits(gx)) and torch.equal(s2_c, s2) and not s1_c.any()
    gx_c, _, _, _ = adjoint(x, g, q, l1=False, l2=False)
    assert torch.equal(bits(gx_c), bits(gx))
    _, s1_a, s2_a, _ = adjoint(x, g, q, acc=torch.ones(3, device=cuda))
    assert torch.equal(s1_a, 1.0 + s1) and torch.equal(s2_a, 1.0 + s2)
    gx_o, s1_o, s2_o, _ = adjoint(offset_copy(x), offset_copy(g), q)
    assert torch.equal(bits(gx_o), bits(gx)) and torch.equal(s1_o, s1) and torch.equal(s2_o, s2)


def test_jpeg_adjoint_flags_nonfinite(cuda):
    c = case(24, 75)
    g = c["g"].to(cuda).clone()
    g[1, 2, 10, 5] = float("inf")
    _, s1, s2, nf = adjoint(c["x"].to(cuda), g, 75)
    assert nf.tolist() == [0, 1, 0]
    assert torch.isfinite(s1[0]) and torch.isfinite(s1[2])
    assert torch.isfinite(s2[0]) and torch.isfinite(s2[2])


# ---- the engine at 32² ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng32(cuda):
    eng, _ = engine(SIZE, F32, cuda, encoder="synthetic")
    x0 = torch.cat([seeded(910, (1, 3, SIZE, SIZE)), 0.6 * seeded(911, (1, 3, SIZE, SIZE))])
    t = torch.cat([seeded(912, (1, 3, SIZE, SIZE)), seeded(913, (1, 3, SIZE, SIZE))])
    return eng, x0.to(cuda), t.to(cuda)


def manual_step(eng, x, m, mu, a, e, q, grad, di=None, taps=None):
    """step_mi after set_jpeg() out of the public ops: J, the existing chain on J(x) (step_mi
    with the stage off, up to its gradient), the adjoint, the smoothing, ops.mi_update."""
    from gfa_amd import ops
    from gfa_amd.weights import ENC_POOL_RES
    N = x.shape[0]
    xj = ops.jpeg_roundtrip(x, torch.empty_like(x), q)
    xi = xj if di is None else ops.di_resize_pad(xj, torch.empty_like(x), *di)
    g_xv, g_enc = eng.gradient(xi)
    g = ops.grad_assemble(xi, eng.x0, g_xv, g_enc, torch.empty_like(x), eng.pf, ENC_POOL_RES,
                          eng.c_img_o, 1.0 / eng.loss_scale)
    l1 = torch.zeros(N, device=x.device)

    def sums(last):
        return (l1, None) if last else (None, None)
    stages = []
    if di is not None:
        stages.append(lambda v, s: ops.di_resize_pad_bwd_norms(v, torch.empty_like(v), *s, *di))
    if grad == "cubic":
        stages.append(lambda v, s: ops.jpeg_bwd_norms(x, v, torch.empty_like(v), q, *s))
    if taps is not None:
        stages.append(lambda v, s: ops.ti_smooth_norms(v, taps, torch.empty_like(v), *s))
    if not stages:
        stages.append(lambda v, s: ops.si_accumulate_norms(v, torch.empty_like(v), *s, 1.0, True))
    for k, stage in enumerate(stages):
        g = stage(g, sums(k == len(stages) - 1))
    ops.mi_update(x, eng.x0, g, l1, m, f32(mu), f32(a), f32(e))
    return x, m


@pytest.mark.parametrize("grad", ["cubic", "ste"])
@pytest.mark.parametrize("stages", ["plain", "di_ti"])
def test_engine_step_is_the_composition_of_the_public_ops(cuda, eng32, grad, stages):
    """One step_mi after set_jpeg(75, grad) equals ops.jpeg_roundtrip → the existing chain →
    ops.jpeg_bwd_norms → ops.mi_update bit for bit ('ste': without the adjoint); with di and
    ti_taps the order is J, D, the networks, Dᵀ, J′ᵀ, W, as in g = W ⋆ J′(x)ᵀ Dᵀ ∇L(D J(x)). The step differs from the
    one with the stage off, and 'cubic' from 'ste'. (The stage is engine state, AttackEngine.jp:
    the signatures of _step_gradient and step_mi are pinned by the earlier attacks' tests.)"""
    eng, x0, t = eng32
    e, a, mu = f32(2 * EPS), f32(2 * ALPHA), 1.0
    q = qtab(75).to(cuda)
    di = (29, 2, 1, 1) if stages == "di_ti" else None
    taps = eng.ti_device_taps([0.25, 0.5, 0.25]) if stages == "di_ti" else None
    m0 = seeded(914, x0.shape).to(cuda)
    eng.prepare(x0, t)
    x, m = x0.clone(), m0.clone()
    qt, mode = eng.set_jpeg(75, grad)
    assert torch.equal(qt, q) and mode == grad
    eng.step_mi(x, m, mu, a, e, ti_taps=taps, di=di)
    eng.set_jpeg(None)
    assert not eng.overflowed() and eng.jp is None
    if grad == "ste" and stages == "plain":
        # 'ste' with no other stage: the norms come from the fused assembly kernel
        from gfa_amd import ops
        from gfa_amd.weights import ENC_POOL_RES
        xr, mr = x0.clone(), m0.clone()
        xj = ops.jpeg_roundtrip(xr, torch.empty_like(xr), q)
        g_xv, g_enc = eng.gradient(xj)
        l1 = torch.zeros(2, device=cuda)
        g = ops.grad_assemble_norms(xj, eng.x0, g_xv, g_enc, torch.empty_like(xr), l1, None,
                                    eng.pf, ENC_POOL_RES, eng.c_img_o, 1.0 / eng.loss_scale)
        ops.mi_update(xr, eng.x0, g, l1, mr, f32(mu), a, e)
    else:
        xr, mr = manual_step(eng, x0.clone(), m0.clone(), mu, a, e, q, grad,
                             None if di is None else di[:3], taps)
    assert torch.equal(bits(x), bits(xr)) and torch.equal(bits(m), bits(mr))
    x_plain, m_plain = x0.clone(), m0.clone()
    eng.step_mi(x_plain, m_plain, mu, a, e, ti_taps=taps, di=di)
    assert not torch.equal(m, m_plain)
    x_other, m_other = x0.clone(), m0.clone()
    eng.set_jpeg(75, "ste" if grad == "cubic" else "cubic")
    eng.step_mi(x_other, m_other, mu, a, e, ti_taps=taps, di=di)
    eng.set_jpeg(None)
    assert not torch.equal(m, m_other)


def test_engine_nesterov_lookahead_runs_before_the_roundtrip(cuda, eng32):
    """With nesterov the stage reads x̃ = x + c·m (ops.si_transform at s = 1): J(x̃) feeds the
    networks and the adjoint is taken at x̃."""
    from gfa_amd import ops
    from gfa_amd.weights import ENC_POOL_RES
    eng, x0, t = eng32
    e, a, mu = f32(2 * EPS), f32(2 * ALPHA), 1.0
    q = qtab(75).to(cuda)
    m0 = seeded(914, x0.shape).to(cuda)
    eng.prepare(x0, t)
    x, m = x0.clone(), m0.clone()
    eng.set_jpeg(75)
    eng.step_mi(x, m, mu, a, e, nesterov=True)
    eng.set_jpeg(None)
    xr, mr = x0.clone(), m0.clone()
    xt = ops.si_transform(xr, mr, torch.empty_like(xr), f32(f32(mu) * a), 1.0)
    xj = ops.jpeg_roundtrip(xt, torch.empty_like(xr), q)
    g_xv, g_enc = eng.gradient(xj)
    g = ops.grad_assemble(xj, eng.x0, g_xv, g_enc, torch.empty_like(xr), eng.pf, ENC_POOL_RES,
                          eng.c_img_o, 1.0 / eng.loss_scale)
    l1 = torch.zeros(2, device=cuda)
    gx = ops.jpeg_bwd_norms(xt, g, torch.empty_like(g), q, l1, None)
    ops.mi_update(xr, eng.x0, gx, l1, mr, f32(mu), a, e)
    assert torch.equal(bits(x), bits(xr)) and torch.equal(bits(m), bits(mr))


@pytest.fixture(scope="module")
def net32(cuda):
    from gfa_amd import networks
    return networks.build_net(SIZE, seed=0, dtype=F32, device=cuda)


def test_attack_jpeg_reruns_and_info(cuda, net32):
    """attack(..., jpeg_quality=75) twice gives identical bits; the result stays in the ε-ball and
    is the uncompressed iterate; return_info reports the stage and the objective at J(adv)."""
    from gfa_amd import attack, jpeg_compress
    from gfa_amd.pgd import AttackEngine
    x0 = torch.cat([seeded(910, (1, 3, SIZE, SIZE)), 0.6 * seeded(911, (1, 3, SIZE, SIZE))])
    t = torch.cat([seeded(912, (1, 3, SIZE, SIZE)), seeded(913, (1, 3, SIZE, SIZE))])
    kw = dict(target=t, alpha=ALPHA, jpeg_quality=75)
    adv, info = attack(net32, x0, EPS, 3, return_info=True, **kw)
    assert torch.equal(bits(adv), bits(attack(net32, x0, EPS, 3, **kw)))
    assert ((adv - x0).abs() <= 2 * EPS + 1e-7).all() and adv.abs().max() <= 1
    assert info["jpeg_quality"] == 75 and info["jpeg_grad"] == "cubic"
    eng = AttackEngine(net32.encoder.impl, net32.decoder.impl, net32.vgg.impl)
    eng.prepare(x0.to(cuda), t.to(cuda))
    want = eng.loss(jpeg_compress(adv.to(cuda), 75))
    assert torch.equal(info["loss_jpeg"], want) and not torch.equal(info["loss_jpeg"], info["loss"])
    ste, info_s = attack(net32, x0, EPS, 3, jpeg_grad="ste", return_info=True, **kw)
    assert info_s["jpeg_grad"] == "ste" and not torch.equal(ste, adv)
    adv_l2 = attack(net32, x0, 1.0, 2, target=t, alpha=0.2, norm="l2", jpeg_quality=75)
    assert ((adv_l2 - x0).reshape(2, -1).norm(dim=1) <= 2.0 * (1 + 1e-5)).all()
    assert not torch.equal(adv_l2, attack(net32, x0, 1.0, 2, target=t, alpha=0.2, norm="l2"))


def test_attack_without_the_keyword_is_unchanged(cuda, net32):
    """attack() without jpeg_quality launches what it launched before: the bits of a direct
    run_mi (momentum given) and of a direct run (the plain sign step), and the info says off."""
    from gfa_amd import attack
    from gfa_amd.pgd import AttackEngine
    x0 = torch.cat([seeded(910, (1, 3, SIZE, SIZE)), 0.6 * seeded(911, (1, 3, SIZE, SIZE))])
    t = torch.cat([seeded(912, (1, 3, SIZE, SIZE)), seeded(913, (1, 3, SIZE, SIZE))])
    eng = AttackEngine(net32.encoder.impl, net32.decoder.impl, net32.vgg.impl)
    want = eng.run_mi(x0.to(cuda), t.to(cuda), 3, EPS, ALPHA, momentum=1.0).cpu()
    adv, info = attack(net32, x0, EPS, 3, target=t, alpha=ALPHA, momentum=1.0, return_info=True)
    assert torch.equal(bits(adv), bits(want))
    assert info["jpeg_quality"] is None and info["jpeg_grad"] is None and info["loss_jpeg"] is None
    want = eng.run(x0.to(cuda), t.to(cuda), 3, EPS, ALPHA).cpu()
    assert torch.equal(bits(attack(net32, x0, EPS, 3, target=t, alpha=ALPHA)), bits(want))


def test_jpeg_error_codes(cuda):
    """MIA_EINVAL from the library itself, before any launch, and the wrappers' own checks."""
    from gfa_amd import _lib, jpeg_compress, ops
    lib = _lib.load()
    st = ops.stream()
    q = qtab(75).to(cuda)

    def P(t):
        return ctypes.c_void_p(t.data_ptr())
    x = torch.zeros(1, 3, 16, 16, device=cuda)
    y, g = torch.zeros_like(x), torch.zeros_like(x)
    x12 = torch.zeros(1, 3, 12, 12, device=cuda)
    y12 = torch.zeros_like(x12)
    OK, EINVAL = 0, -1
    assert lib.mia_jpeg_roundtrip(P(x), P(y), P(q), 1, 16, st) == OK
    assert lib.mia_jpeg_roundtrip(P(x12), P(y12), P(q), 1, 12, st) == EINVAL      # S = 12
    assert b"multiple of 8" in lib.mia_last_error_string()
    assert lib.mia_jpeg_bwd_norms(P(x12), P(y12), P(torch.zeros_like(x12)), P(q), None, None, 1, 12,
                                  None, st) == EINVAL
    assert lib.mia_jpeg_roundtrip(P(x), P(x), P(q), 1, 16, st) == EINVAL          # aliased
    assert b"distinct" in lib.mia_last_error_string()
    assert lib.mia_jpeg_bwd_norms(P(x), P(g), P(g), P(q), None, None, 1, 16, None, st) == EINVAL
    assert lib.mia_jpeg_bwd_norms(P(x), P(x), P(g), P(q), None, None, 1, 16, None, st) == EINVAL
    # (N, S); the last: 3·S² ≥ 2^31
    for bad in ((0, 16), (65536, 16), (1, 0), (1, 4), (1, -8), (1, 26760)):
        assert lib.mia_jpeg_roundtrip(P(x), P(y), P(q), *bad, st) == EINVAL
        assert lib.mia_jpeg_bwd_norms(P(x), P(g), P(y), P(q), None, None, *bad, None, st) == EINVAL
    assert lib.mia_jpeg_roundtrip(None, P(y), P(q), 1, 16, st) == EINVAL
    assert lib.mia_jpeg_roundtrip(P(x), P(y), None, 1, 16, st) == EINVAL
    assert lib.mia_jpeg_bwd_norms(P(x), P(g), None, P(q), None, None, 1, 16, None, st) == EINVAL
    # overlapping views of one buffer through the wrapper: the library's own check
    flat = torch.zeros(3 * 16 * 16 + 4, device=cuda)
    a, b = flat[:-4].view(1, 3, 16, 16), flat[4:].view(1, 3, 16, 16)
    with pytest.raises(Exception, match="distinct"):
        ops.jpeg_roundtrip(a, b, q)
    # the wrappers and the public helper
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.jpeg_roundtrip(x12, y12, q)
    with pytest.raises(ValueError, match="distinct"):
        ops.jpeg_roundtrip(x, x, q)
    with pytest.raises(ValueError, match="distinct"):
        ops.jpeg_bwd_norms(x, g, g, q, None, None)
    with pytest.raises(ValueError, match="qtab"):
        ops.jpeg_roundtrip(x, y, q.reshape(128))
    with pytest.raises(ValueError):
        ops.jpeg_roundtrip(x.double(), y.double(), q)
    with pytest.raises(ValueError):
        ops.jpeg_bwd_norms(x, g, y, q, torch.zeros(2, device=cuda), None)
    with pytest.raises(ValueError, match="jpeg_quality"):
        jpeg_compress(x, 0)                                                       # quality = 0
    torch.cuda.synchronize()
