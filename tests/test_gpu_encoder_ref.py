"""The non-conv kernels of the e4e encoder (csrc/encoder.hip), each called directly and compared
with a plain fp64 reference of the same operation computed from the values as the device holds
them (after the cast to fp16 / bf16 where a 2-byte type applies, and from the device's own
partials and u where a later kernel consumes an earlier one's output): the channel reductions
chan_dot / chan_sum, the SE forward and backward in their plain and from-partials forms, se_apply
at every combination of its optional arguments, se_grad_scale, the PReLU forward and backward,
subsample_add, cast at its nine dtype pairs and past the block cap, and the bilinear up-sampling
with its adjoint.

Inputs come from seeded CPU generators, every image of a batch has its own scale (IMG_SCALES)
wherever the operation is linear per image, and every output buffer is pre-filled with NaN, or
with seeded data that the reference includes where the kernel accumulates. Bounds are counts of
fp32 roundings times U = 2⁻²⁴ on the sum of the absolute values of the terms, plus half a spacing
of the output format for 2-byte outputs; the measured maxima are printed.

The one measured figure: the SE gate s = 1 / (1 + __expf(−z)) against fp64 sigmoid of the fp64
pre-activation z = W2·u (u as the device stored it). Largest |s − sigmoid(z)| over every case of
test_se_fwd on an MI355X (gfx950): 2.107e-07 (SE_S_MEASURED); the bound SE_S_BOUND = 2⁻²⁰ =
9.54e-07 is 4× that, rounded up to a power of two (and below the 1e-5 of its maximum that
test_se_kernels_vs_autograd holds s to)."""
import math

import pytest
import torch
import torch.nn.functional as F

from gpu_helpers import seeded
from test_gpu_pointwise_ref import BF16, F16, F32, NAN, SPACING, U, f32, scales, spacing

pytestmark = pytest.mark.gpu

DTYPES = [F32, F16, BF16]
SE_S_MEASURED = 2.107e-07  # at (C, Cr) = (512, 64)
SE_S_BOUND = 2.0 ** -20    # 4·2.107e-07 = 8.43e-07 ≤ 2⁻²⁰ = 9.54e-07


def img(seed, shape, dtype=F32, scaled=True):
    """Seeded values in (−1, 1), image n times IMG_SCALES[n % 3], as the device holds them."""
    x = seeded(seed, shape)
    if scaled:
        x = x * scales(shape[0]).reshape((-1,) + (1,) * (len(shape) - 1))
    return x.to(dtype)


def half_spacing(ref64, dtype):
    """The rounding of an fp32 result to a 2-byte output: half a spacing of the format at the
    reference (0 for fp32 outputs, whose roundings the counts hold)."""
    if dtype == F32:
        return torch.zeros_like(ref64)
    return 0.5 * spacing(ref64, *SPACING[dtype])


def held(tag, got, ref, tol):
    """Assert |got − ref| ≤ tol everywhere (NaN fails), and print the maximum of the ratio."""
    err = (got.double().cpu() - ref).abs()
    assert not torch.isnan(err).any(), tag
    worst = (err / tol.clamp_min(1e-300)).max().item()
    assert (err <= tol).all(), (tag, worst)
    return worst


# ---- 6. chan_dot / chan_sum ----------------------------------------------------------------------
CHAN_MAPS = [(1, 1), (3, 5), (7, 7), (10, 15), (32, 32)]
CHAN_NCH = {1: 1, 15: 1, 49: 3, 150: 9, 1024: 32}  # chunks per image at these H·W
CHAN_CASES = [(C, H, W) for C in (8, 24, 256, 2048) for H, W in CHAN_MAPS
              if C < 2048 or H * W <= 49]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,H,W", CHAN_CASES)
def test_chan_dot_sum(cuda, C, H, W, dtype):
    """chan_dot, and chan_sum in its dot and sum forms with out given: Σ_pixels a·b (Σ_pixels a)
    per (image, channel) against the fp64 sum of the device-held values, without and with
    accumulate (the destination pre-filled with seeded data the reference includes), within
    (HW + 4)·U·(Σ|a||b| [+ |dst|]) (Σ|a| for the sum form). The longest chain of roundings behind
    one output is the product, a thread's ⌈ppc/pr⌉ additions, the min(pr, ppc) non-zero partials
    of the LDS sum, the nch chunk additions and the accumulate: ≤ HW + 4 in every case here (the
    worst, C = 2048 with one pixel in flight: HW + 1 + 1 + 1). C = 8 / 24 / 256 / 2048 put 256 /
    85 / 8 / 1 pixels in flight (C = 24 leaves thread 255 idle); HW = 1 … 1024 give 1, 1, 3, 9 and
    32 chunks, 49 and 150 being no multiple of their chunk size."""
    from gfa_amd import ops
    N, HW = 3, H * W
    nch = ops.chan_sum_parts(N, HW)
    assert nch == CHAN_NCH[HW]
    a = img(700 + C + HW, (N, H, W, C), dtype)
    b = img(701 + C + HW, (N, H, W, C), dtype, scaled=False)
    base = img(702 + C + HW, (N, C))
    ad, bd = a.to(cuda), b.to(cuda)
    a64, b64 = a.double(), b.double()
    refs = {"dot": ((a64 * b64).sum((1, 2)), (a64 * b64).abs().sum((1, 2))),
            "sum": (a64.sum((1, 2)), a64.abs().sum((1, 2)))}
    worst = {}
    for acc in (False, True):
        def dst():
            return base.clone().to(cuda) if acc else torch.full((N, C), NAN, device=cuda)

        def part():
            return torch.full((N * nch * C,), NAN, device=cuda)
        outs = (("chan_dot", "dot", ops.chan_dot(ad, bd, dst(), accumulate=acc)),
                ("chan_sum dot", "dot", ops.chan_sum(ad, bd, part(), dst(), accumulate=acc)),
                ("chan_sum sum", "sum", ops.chan_sum(ad, None, part(), dst(), accumulate=acc)))
        for name, form, got in outs:
            ref, mag = refs[form]
            if acc:
                ref, mag = ref + base.double(), mag + base.double().abs()
            worst[f"{name} acc={int(acc)}"] = round(
                held(name, got, ref, (HW + 4) * U * mag) * (HW + 4), 3)
    print(f"chan C={C} {H}x{W} {dtype}: max error in U·Σ|terms| (≤ {HW + 4}): {worst}")


@pytest.mark.parametrize("C", [12, 2056])
def test_chan_dot_sum_refuse_bad_channels(cuda, C):
    """C that is no multiple of 8, or above 2048, raises ValueError before anything is launched:
    the destination keeps its pre-fill."""
    from gfa_amd import ops
    a = torch.ones(1, 2, 2, C, dtype=F16, device=cuda)
    gs = torch.full((1, C), 7.0, device=cuda)
    part = torch.full((C,), 7.0, device=cuda)
    with pytest.raises(ValueError):
        ops.chan_dot(a, a, gs)
    with pytest.raises(ValueError):
        ops.chan_sum(a, None, part, gs)
    with pytest.raises(ValueError):
        ops.chan_sum(a, a, part, gs, accumulate=True)
    assert (gs == 7.0).all() and (part == 7.0).all()


# ---- 7. SE forward / backward --------------------------------------------------------------------
SE_CASES = [(8, 1), (40, 3), (72, 9), (256, 16), (512, 32), (512, 64)]
SE_MAPS = {1: (3, 5), 3: (7, 7), 9: (10, 15), 32: (32, 32)}  # nch: the map that gives it


def se_weights(C, Cr, seed):
    w1 = seeded(seed, (Cr, C)) * (2.0 / math.sqrt(C))
    w2 = seeded(seed + 1, (C, Cr)) * (3.0 / math.sqrt(Cr))
    return w1, w2


def partials(part, N, nch, C):
    """(Σ_q, Σ_q|·|) in fp64 of the device's ordered chunk partials."""
    p = part.cpu()[:N * nch * C].reshape(N, nch, C).double()
    return p.sum(1), p.abs().sum(1)


def se_fwd_check(tag, k, avg, avg_abs, w1, w2, u, s):
    """u = relu(W1·avg) within k·U·Σ|w1||avg| (ReLU is 1-Lipschitz); s against fp64 sigmoid of
    z = W2·u from the device's u within SE_S_BOUND. Returns (u's error in U·Σ, max |Δs|)."""
    u_ref = torch.relu(avg @ w1.double().t())
    e_u = held(tag + " u", u, u_ref, k * U * (avg_abs @ w1.double().abs().t()))
    s_ref = torch.sigmoid(u.double().cpu() @ w2.double().t())
    d_s = (s.double().cpu() - s_ref).abs()
    assert not torch.isnan(d_s).any(), tag
    return e_u * k, d_s.max().item()


@pytest.mark.parametrize("C,Cr", SE_CASES)
def test_se_fwd(cuda, C, Cr):
    """se_fwd from a given (signed) channel sum, and se_fwd_parts from chan_sum's partials of
    non-negative maps with nch = 1, 3, 9, 32 (reference: the fp64 sum of those partials, times the
    fp32 1/hw the launcher passes). u of the plain form within (C + 4)·U·Σ|w1||avg|: ·1/hw, a
    lane's ⌈C/64⌉ fused terms and the butterfly's log2(min(C, 64)) ≤ 6 non-trivial additions,
    ⌈C/64⌉ + 7 ≤ C + 4 at most (C = 8: 1 + 1 + 3). The parts form has chan_total's nch − 1
    additions before them, so it is held to (C + nch + 4)·U·Σ|w1||avg|; the partials being
    non-negative, Σ|partials| = |avg|. s: see the module docstring. Cr % 8 ≠ 0 runs
    dot_strided's tail, C % 64 ≠ 0 lane_dot8's guards, (512, 64) fills avg[512] and uu[64]."""
    from gfa_amd import ops
    N = 3
    w1, w2 = se_weights(C, Cr, 800 + C + Cr)
    w1d, w2d = w1.to(cuda), w2.to(cuda)
    hw = 49
    csum = seeded(802 + C, (N, C)) * (2.0 * hw)
    u = torch.full((N, Cr), NAN, device=cuda)
    s = torch.full((N, C), NAN, device=cuda)
    ops.se_fwd(csum.to(cuda), w1d, w2d, u, s, hw)
    avg = csum.double() * f32(1.0 / hw)
    res = {"plain": se_fwd_check("se_fwd", C + 4, avg, avg.abs(), w1, w2, u, s)}
    for nch, (H, W) in SE_MAPS.items():
        x = (seeded(803 + C + nch, (N, H, W, C)).abs() * 2.0).to(cuda)
        assert ops.chan_sum_parts(N, H * W) == nch
        part = ops.chan_sum(x, None, torch.full((N * nch * C,), NAN, device=cuda), None)
        u.fill_(NAN)
        s.fill_(NAN)
        ops.se_fwd_parts(part, H * W, w1d, w2d, u, s)
        tot, tot_abs = partials(part, N, nch, C)
        inv = f32(1.0 / (H * W))
        res[f"nch={nch}"] = se_fwd_check(f"se_fwd_parts nch={nch}", C + nch + 4, tot * inv,
                                         tot_abs * inv, w1, w2, u, s)
    ds = max(v[1] for v in res.values())
    print(f"se_fwd C={C} Cr={Cr}: u max error {max(v[0] for v in res.values()):.3f} U·Σ|w1||avg| "
          f"(≤ {C + 4}, parts {C + 4} + nch), max |s − sigmoid(z)| {ds:.3e} (≤ {SE_S_BOUND:.3e})")
    assert SE_S_BOUND < 1e-5
    assert ds <= SE_S_BOUND


def se_bwd_check(tag, Cr, nch, gs, gs_abs, s, u, w1, w2, gavg, inv):
    """gavg = inv·W1ᵀ([u > 0]·W2ᵀ(gs·s·(1 − s))) within (Cr + nch + 18)·U·inv·|W1|ᵀ([u > 0]·
    |W2|ᵀ|gs|·s·(1 − s)): chan_total's nch additions, 1 − s and the two products (3), a lane's ≤ 8
    fused terms and 6 butterfly additions (14), dot_strided's Cr terms and the product with inv."""
    sg = s.double() * (1 - s.double())
    mask = (u > 0).double()
    ref = inv * (((gs * sg) @ w2.double()) * mask) @ w1.double()
    mag = inv * (((gs_abs * sg) @ w2.double().abs()) * mask) @ w1.double().abs()
    return held(tag, gavg, ref, (Cr + nch + 18) * U * mag) * (Cr + nch + 18)


@pytest.mark.parametrize("C,Cr", SE_CASES)
def test_se_bwd(cuda, C, Cr):
    """se_bwd from a given gs (one scale per image) and se_bwd_parts from chan_sum's dot partials
    at nch = 1, 3, 9, 32, with the test's own u (exact zeros, −0.0 and positives: the ReLU mask is
    an input) and s strictly inside (0, 1). Bound: se_bwd_check (nch = 0 for the plain form),
    with Σ|partials| in place of |gs| for the parts form."""
    from gfa_amd import ops
    N, hw = 3, 49
    w1, w2 = se_weights(C, Cr, 820 + C + Cr)
    w1d, w2d = w1.to(cuda), w2.to(cuda)
    s = 0.05 + 0.9 * torch.rand((N, C), generator=torch.Generator().manual_seed(822 + C))
    u = (seeded(823 + Cr, (N, Cr)).abs() + 0.1).flatten()
    u[1::3] = 0.0
    u[2::7] = -0.0
    u = u.reshape(N, Cr)
    assert (u > 0).any() and (u == 0).any()
    sd, ud = s.to(cuda), u.to(cuda)
    gs = img(824 + C, (N, C))
    gavg = ops.se_bwd(gs.to(cuda), sd, ud, w1d, w2d, torch.full((N, C), NAN, device=cuda), hw)
    res = {"plain": se_bwd_check("se_bwd", Cr, 0, gs.double(), gs.double().abs(), s, u, w1, w2,
                                 gavg, f32(1.0 / hw))}
    for nch, (H, W) in SE_MAPS.items():
        go = img(825 + C + nch, (N, H, W, C)).to(cuda)
        r = img(826 + C + nch, (N, H, W, C), scaled=False).to(cuda)
        part = ops.chan_sum(go, r, torch.full((N * nch * C,), NAN, device=cuda), None)
        gavg = ops.se_bwd_parts(part, H * W, sd, ud, w1d, w2d,
                                torch.full((N, C), NAN, device=cuda))
        tot, tot_abs = partials(part, N, nch, C)
        res[f"nch={nch}"] = se_bwd_check(f"se_bwd_parts nch={nch}", Cr, nch, tot, tot_abs, s, u,
                                         w1, w2, gavg, f32(1.0 / (H * W)))
    print(f"se_bwd C={C} Cr={Cr}: max error in U·Σ|terms| (≤ Cr + nch + 18): "
          f"{ {k: round(v, 3) for k, v in res.items()} }")


def test_se_refuses_sizes_past_its_lds(cuda):
    """C = 520 (avg[512]) and Cr = 65 (uu[64]) raise and leave the outputs untouched."""
    from gfa_amd import ops
    from gfa_amd._lib import MiaError
    for C, Cr in ((520, 8), (512, 65)):
        csum = torch.ones(1, C, device=cuda)
        w1, w2 = torch.ones(Cr, C, device=cuda), torch.ones(C, Cr, device=cuda)
        u, s = torch.full((1, Cr), 7.0, device=cuda), torch.full((1, C), 7.0, device=cuda)
        gavg = torch.full((1, C), 7.0, device=cuda)
        with pytest.raises(MiaError):
            ops.se_fwd(csum, w1, w2, u, s, 4)
        with pytest.raises(MiaError):
            ops.se_bwd(csum, torch.full((1, C), 0.5, device=cuda), torch.ones(1, Cr, device=cuda),
                       w1, w2, gavg, 4)
        assert (u == 7.0).all() and (s == 7.0).all() and (gavg == 7.0).all()


# ---- 8. se_apply ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [8, 24])
def test_se_apply_optional_arguments(cuda, C, dtype):
    """out = r·s + sc[::ss, ::ss] and xb = out·g + b at every combination the launcher accepts: s
    given or not, sc absent or read at stride 1 or 2, out alone, xb alone, both (18 calls), on a
    3 × 5 map. out within 2·U·(|r·s| + |sc|) (the product and the addition), xb, computed from the
    unrounded out, within 4·U·((|r·s| + |sc|)·|g| + |b|) (two more), each plus half a spacing of a
    2-byte output. The shortcut holds a distinct value at every pixel and one scale per image."""
    from gfa_amd import ops
    N, H, W = 2, 3, 5
    r = img(900 + C, (N, H, W, C), dtype)
    s = seeded(901 + C, (N, C))
    g = 1.0 + 0.1 * seeded(902 + C, (C,))
    b = seeded(903 + C, (C,))
    rd, sd, gd, bd = r.to(cuda), s.to(cuda), g.to(cuda), b.to(cuda)
    worst_o = worst_x = 0.0
    for use_s in (True, False):
        for ss in (None, 1, 2):
            sc = None if ss is None else img(904 + C + ss, (N, H * ss, W * ss, C), dtype)
            t1 = r.double() * (s.double()[:, None, None, :] if use_s else 1.0)
            t2 = torch.zeros_like(t1) if sc is None else sc.double()[:, ::ss, ::ss]
            ref_o, mag_o = t1 + t2, t1.abs() + t2.abs()
            ref_x = ref_o * g.double() + b.double()
            mag_x = mag_o * g.double().abs() + b.double().abs()
            for want_out, want_xb in ((True, False), (False, True), (True, True)):
                out = torch.full((N, H, W, C), NAN, dtype=dtype, device=cuda) if want_out else None
                xb = torch.full((N, H, W, C), NAN, dtype=dtype, device=cuda) if want_xb else None
                ops.se_apply(rd, sd if use_s else None, sc.to(cuda) if sc is not None else None,
                             ss or 1, out, gd if want_xb else None, bd if want_xb else None, xb)
                tag = f"s={int(use_s)} ss={ss} out={int(want_out)} xb={int(want_xb)}"
                if want_out:
                    tol = 2 * U * mag_o + half_spacing(ref_o, dtype)
                    worst_o = max(worst_o, held("se_apply out " + tag, out, ref_o, tol))
                if want_xb:
                    tol = 4 * U * mag_x + half_spacing(ref_x, dtype)
                    worst_x = max(worst_x, held("se_apply xb " + tag, xb, ref_x, tol))
    print(f"se_apply C={C} {dtype}: max error out {worst_o:.3f}, xb {worst_x:.3f} of the bound")


def test_se_apply_refuses(cuda):
    """Neither output, and a shortcut stride of 3, raise."""
    from gfa_amd import ops
    from gfa_amd._lib import MiaError
    r = torch.ones(1, 2, 2, 8, device=cuda)
    out = torch.full((1, 2, 2, 8), 7.0, device=cuda)
    with pytest.raises(MiaError):
        ops.se_apply(r, None, None, 1, None)
    with pytest.raises(MiaError):
        ops.se_apply(r, None, torch.ones(1, 6, 6, 8, device=cuda), 3, out)
    assert (out == 7.0).all()


# ---- 9. se_grad_scale ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [8, 24])
@pytest.mark.parametrize("with_gamma", [False, True])
def test_se_grad_scale(cuda, with_gamma, C, dtype):
    """g_r = gamma·(g_out·s + gavg) (gamma = 1 without it) on a 3 × 5 map within 3·U·|gamma|·
    (|g_out·s| + |gavg|) (two products and the addition), plus half a spacing of a 2-byte
    output."""
    from gfa_amd import ops
    N, H, W = 3, 3, 5
    go = img(1000 + C, (N, H, W, C), dtype)
    s = seeded(1001 + C, (N, C))
    ga = img(1002 + C, (N, C))
    gamma = seeded(1003 + C, (C,)) * 2 if with_gamma else None
    gr = ops.se_grad_scale(go.to(cuda), s.to(cuda), ga.to(cuda),
                           torch.full((N, H, W, C), NAN, dtype=dtype, device=cuda),
                           gamma.to(cuda) if with_gamma else None)
    gm = gamma.double() if with_gamma else torch.ones(C, dtype=torch.float64)
    t1, t2 = go.double() * s.double()[:, None, None, :], ga.double()[:, None, None, :]
    ref, mag = gm * (t1 + t2), gm.abs() * (t1.abs() + t2.abs())
    w = held("se_grad_scale", gr, ref, 3 * U * mag + half_spacing(ref, dtype))
    print(f"se_grad_scale gamma={int(with_gamma)} C={C} {dtype}: max error {w:.3f} of the bound")


# ---- 10. PReLU -----------------------------------------------------------------------------------
def prelu_inputs(C, dtype, seed):
    """(activation with exact +0.0 and −0.0, slopes of both signs)."""
    a = img(seed, (2, 3, 5, C), dtype).flatten()
    a[::5] = 0.0
    a[1::11] = -0.0
    slope = seeded(seed + 1, (C,))
    slope[0], slope[1] = -0.25, 0.25
    return a.reshape(2, 3, 5, C), slope


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [8, 24])
def test_prelu_fwd_and_bwd_scale(cuda, C, dtype):
    """prelu_fwd: a = pre > 0 ? pre : slope·pre within U·|ref| (one product). prelu_bwd_scale:
    g = g_a·(a > 0 ? 1 : slope)·gamma within 2·U·|ref| with gamma, U·|ref| without (gamma = 1 is
    exact): two roundings at most. Each plus half a spacing of a 2-byte output. Slopes of both
    signs; ±0.0 take the slope branch (the reference's a > 0)."""
    from gfa_amd import ops
    a, slope = prelu_inputs(C, dtype, 1100 + C)
    gamma = seeded(1102 + C, (C,)) * 2
    ga = img(1103 + C, a.shape, dtype)
    ad, sld = a.to(cuda), slope.to(cuda)
    pos = a.double() > 0
    assert (a == 0).sum() > 10 and (slope < 0).any() and (slope > 0).any()
    ref = torch.where(pos, a.double(), slope.double() * a.double())
    y = ops.prelu_fwd(ad, sld, torch.full(a.shape, NAN, dtype=dtype, device=cuda))
    w = {"fwd": held("prelu_fwd", y, ref, U * ref.abs() + half_spacing(ref, dtype))}
    assert (y.cpu()[a == 0] == 0).all()
    for name, gm, k in (("bwd", None, 1), ("bwd gamma", gamma, 2)):
        g = ops.prelu_bwd_scale(ga.to(cuda), ad, sld,
                                torch.full(a.shape, NAN, dtype=dtype, device=cuda),
                                gm.to(cuda) if gm is not None else None)
        ref = torch.where(pos, ga.double(), slope.double() * ga.double())
        if gm is not None:
            ref = ref * gm.double()
        w[name] = held("prelu_bwd_scale", g, ref, k * U * ref.abs() + half_spacing(ref, dtype))
    print(f"prelu C={C} {dtype}: max error of the bound { {k: round(v, 3) for k, v in w.items()} }")


# ---- 11. subsample_add ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [8, 24])
@pytest.mark.parametrize("H,W", [(3, 5), (4, 2)])
def test_subsample_add(cuda, H, W, C, dtype):
    """gx[n][2y][2x] += g[n][y][x] on non-square maps, gx pre-filled with seeded data: the even
    positions within U·(|gx0| + |g|) (one addition) plus half a spacing of a 2-byte output, the
    odd rows and columns bit-identical to the pre-fill."""
    from gfa_amd import ops
    N = 2
    g = img(1200 + C + H, (N, H, W, C), dtype)
    gx0 = img(1201 + C + H, (N, 2 * H, 2 * W, C), dtype)
    gx = ops.subsample_add(g.to(cuda), gx0.clone().to(cuda)).cpu()
    ref = gx0.double()[:, ::2, ::2] + g.double()
    mag = gx0.double()[:, ::2, ::2].abs() + g.double().abs()
    w = held("subsample_add", gx[:, ::2, ::2], ref, U * mag + half_spacing(ref, dtype))
    odd = torch.ones(2 * H, 2 * W, dtype=torch.bool)
    odd[::2, ::2] = False
    assert torch.equal(gx[:, odd], gx0[:, odd])
    print(f"subsample_add {H}x{W} C={C} {dtype}: max error {w:.3f} of the bound")


# ---- 12. cast ------------------------------------------------------------------------------------
BITS = {F32: torch.int32, F16: torch.int16, BF16: torch.int16}


def cast_input(n, seed, dtype):
    """Values in (−1, 1) times 1e4, 1, 1e-4 by element, as the source type holds them."""
    k = torch.tensor([1e4, 1.0, 1e-4])[torch.arange(n) % 3]
    return (seeded(seed, (n,)) * k).to(dtype)


@pytest.mark.parametrize("dst", DTYPES)
@pytest.mark.parametrize("src", DTYPES)
def test_cast_pairs(cuda, src, dst):
    """y = (dst)(fp32(x)·scale) at n = 1, 255, 257 and scale = 1, 2, 1/1024: bit-identical to
    torch's round-to-nearest-even conversion of the fp32 product on the CPU (powers of two: the
    product is exact unless it leaves the normal range)."""
    from gfa_amd import ops
    for n in (1, 255, 257):
        x = cast_input(n, 1300 + n, src)
        for scale in (1.0, 2.0, 1.0 / 1024):
            y = ops.cast(x.to(cuda), torch.full((n,), NAN, dtype=dst, device=cuda), scale).cpu()
            want = (x.float() * torch.tensor(scale, dtype=F32)).to(dst)
            assert torch.equal(y.view(BITS[dst]), want.view(BITS[dst])), (n, scale)
    print(f"cast {src} → {dst}: bit-identical at n = 1, 255, 257, scale = 1, 2, 1/1024")


def test_cast_past_the_block_cap(cuda):
    """fp32 → fp16 at n = 65536·256 + 1000, past the 65536-block cap of the launch, so the
    grid-stride loop's second trip does the tail: the last 1000 elements and a seeded sample of
    100 000 of the rest are bit-identical to torch's conversion. (The 8-vector elementwise kernels
    share this loop shape but are not taken past the cap: with 8 elements per thread that needs
    1.3·10⁸ elements and about 1 GB of fp64 reference.)"""
    from gfa_amd import ops
    n = 65536 * 256 + 1000
    x = cast_input(n, 1310, F32)
    y = ops.cast(x.to(cuda), torch.full((n,), NAN, dtype=F16, device=cuda), 2.0).cpu()
    gen = torch.Generator().manual_seed(1311)
    idx = torch.cat([torch.randint(n - 1000, (100000,), generator=gen), torch.arange(n - 1000, n)])
    want = (x[idx] * torch.tensor(2.0)).to(F16)
    assert torch.equal(y[idx].view(torch.int16), want.view(torch.int16))
    assert not torch.isnan(y).any()
    print(f"cast fp32 → fp16 n={n}: {idx.numel()} elements bit-identical, no element skipped")


# ---- 13. bilinear (align_corners = True) and its adjoint -----------------------------------------
BL_CASES = [(1, 1, 5, 7),    # one input pixel: scale 0 on both axes
            (2, 3, 64, 33),  # large ratios: the adjoint's widest windows
            (5, 8, 5, 8),    # the identity
            (4, 6, 9, 16), (7, 5, 8, 23),  # a ratio per axis, Hi ≠ Wi
            (3, 1, 3, 9)]    # the identity on one axis, scale 0 on the other


def contributing(n_in, n_out):
    """Outputs that read input i (as i0 or i1) along one axis, in exact integer arithmetic."""
    cnt = torch.zeros(n_in, dtype=torch.float64)
    for o in range(n_out):
        i0 = (o * (n_in - 1)) // (n_out - 1) if n_out > 1 else 0
        cnt[i0] += 1
        if i0 < n_in - 1:
            cnt[i0 + 1] += 1
    return cnt


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Hi,Wi,Ho,Wo", BL_CASES)
def test_bilinear_fwd_bwd(cuda, Hi, Wi, Ho, Wo, dtype):
    """bilinear_fwd against F.interpolate(align_corners=True) in fp64 and bilinear_bwd against its
    autograd gradient, N = 2 at two scales, C = 8 and 24, both accumulate values each.

    Forward: the kernel computes the source coordinate in fp32 (the rounding of the scale and of
    the product: off by ≤ 2·U·Hi), interpolation is continuous in it and moves by at most that
    times a neighbour difference ≤ 2·max|x|, per axis: 4·U·(Hi + Wi)·max|x|; the weights'
    1 − λ, four products and three additions stay within another 4·U·(Hi + Wi)·max|x| (Hi + Wi ≥
    2). So |y − ref| ≤ 8·U·(Hi + Wi)·max|x| of the image, plus U·(|y0| + |ref|) for the addition
    under accumulate, plus half a spacing of a 2-byte output.

    Adjoint: every contributing output carries a weight off by the same coordinate error, so the
    bound is 8·U·(Hi + Wi)·max|g| times the number of outputs that read the pixel (counted per
    axis in integer arithmetic, λ = 0 neighbours included). The gather's own n fp32 additions of
    partial sums bounded by Σ w·|g| add n·U·Σ w·|g| (Σ w·|g|: the fp64 adjoint applied to |g|; at
    2 × 3 → 64 × 33, where the weights of a pixel sum to 352, this term is the larger one). Plus
    the accumulate and output terms."""
    from gfa_amd import ops
    N = 2
    ncon = contributing(Hi, Ho)[:, None] * contributing(Wi, Wo)[None, :]
    worst = {}
    for C in (8, 24):
        x = img(1400 + C + Ho, (N, Hi, Wi, C), dtype)
        y0 = img(1401 + C + Ho, (N, Ho, Wo, C), dtype)
        # (÷ 64, exact: the 2 × 3 → 64 × 33 gather sums weights of 352, and fp16 ends at 65504)
        g = (img(1402 + C + Ho, (N, Ho, Wo, C)) / 64).to(dtype)
        gx0 = img(1403 + C + Ho, (N, Hi, Wi, C), dtype)
        xx = x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
        up = F.interpolate(xx, size=(Ho, Wo), mode="bilinear", align_corners=True)
        (gref,) = torch.autograd.grad(up, xx, g.double().permute(0, 3, 1, 2), retain_graph=True)
        (gabs,) = torch.autograd.grad(up, xx, g.double().abs().permute(0, 3, 1, 2))
        up, gref, gabs = (t.detach().permute(0, 2, 3, 1) for t in (up, gref, gabs))
        xmax = x.double().abs().amax((1, 2, 3)).reshape(N, 1, 1, 1)
        gmax = g.double().abs().amax((1, 2, 3)).reshape(N, 1, 1, 1)
        for acc in (False, True):
            y = ops.bilinear_fwd(x.to(cuda), y0.clone().to(cuda) if acc else torch.full(
                y0.shape, NAN, dtype=dtype, device=cuda), accumulate=acc)
            ref = up + y0.double() if acc else up
            tol = (8 * U * (Hi + Wi) * xmax + (U * (y0.double().abs() + up.abs()) if acc else 0)
                   + half_spacing(ref, dtype))
            w = held(f"bilinear_fwd C={C} acc={acc}", y, ref, tol)
            worst["fwd"] = max(worst.get("fwd", 0.0), w)
            gx = ops.bilinear_bwd(g.to(cuda), gx0.clone().to(cuda) if acc else torch.full(
                gx0.shape, NAN, dtype=dtype, device=cuda), accumulate=acc)
            ref = gref + gx0.double() if acc else gref
            tol = ((8 * U * (Hi + Wi) * gmax + U * gabs) * ncon[None, :, :, None]
                   + (U * (gx0.double().abs() + gref.abs()) if acc else 0)
                   + half_spacing(ref, dtype))
            w = held(f"bilinear_bwd C={C} acc={acc}", gx, ref, tol)
            worst["bwd"] = max(worst.get("bwd", 0.0), w)
    print(f"bilinear {Hi}x{Wi} → {Ho}x{Wo} {dtype}: max error of the bound "
          f"{ {k: round(v, 4) for k, v in worst.items()} }")


def test_bilinear_bwd_refuses_down_sampling(cuda):
    """Ho < Hi raises (the gather window is derived for up-sampling) and leaves gx untouched."""
    from gfa_amd import ops
    from gfa_amd._lib import MiaError
    gx = torch.full((1, 3, 4, 8), 7.0, device=cuda)
    with pytest.raises(MiaError):
        ops.bilinear_bwd(torch.ones(1, 2, 4, 8, device=cuda), gx)
    assert (gx == 7.0).all()
