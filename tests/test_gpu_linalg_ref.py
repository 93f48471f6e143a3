"""The small fp32 linear algebra of csrc/small_linalg.hip, each kernel called directly and compared
with a plain fp64 reference of the same operation computed from the fp32 values the device holds:
the strided SGEMM on both sides of its tile switch (single and grouped, across the launch split),
style_demod and demod_bwd over shape grids that reach every loop of the kernels.

Inputs come from seeded CPU generators, the per-image operations get one scale per image
(IMG_SCALES), outputs are pre-filled with NaN (or, where the kernel accumulates, with seeded data
the reference includes). Bounds are counts of fp32 roundings times U = 2⁻²⁴ on the sum of the
absolute values of the terms; the measured maxima are printed.

The SGEMM's tile rule (run_gemm_groups): with T64 = Σ_groups ⌈M/64⌉·⌈N/64⌉ over ALL groups of a
call, sgemm_grouped_kernel<64> runs when T64 ≥ 512 and sgemm_grouped_kernel<32> otherwise; a call
is launched in slices of kMaxGroups = 12 groups. A test cannot observe which instantiation ran:
the tile counts written next to each case are the evidence."""
import pytest
import torch

from gpu_helpers import seeded
from test_gpu_pointwise_ref import NAN, U, f32, scales

pytestmark = pytest.mark.gpu


def tiles64(groups):
    """T64 of the host's rule for [(M, N), …]."""
    return sum(-(-m // 64) * -(-n // 64) for m, n in groups)


def gemm_check(tag, got, ab, ab_abs, c0, bias, alpha, beta, K):
    """|got − (α·ab + β·c0 + bias)| ≤ (K + 4)·U·(|α|·Σ_k|a||b| + |β||c0| + |bias|) per element: the
    K products and K − 1 additions of the accumulator form a chain of at most K roundings per term
    (the products fused or not), then α·acc, β·c, and the two additions: K + 4."""
    a32, b32 = f32(alpha), f32(beta)
    ref = a32 * ab + b32 * c0.double() + bias.double()
    mag = abs(a32) * ab_abs + abs(b32) * c0.double().abs() + bias.double().abs()
    err = (got.double() - ref).abs()
    assert not torch.isnan(got).any()
    worst = (err / (U * mag).clamp_min(1e-300)).max().item()
    print(f"gemm {tag}: max error {worst:.3f} U·Σ|terms| (≤ {K + 4})")
    assert (err <= (K + 4) * U * mag).all()


# ---- 1. the single GEMM on both sides of the tile switch -----------------------------------------
GEMM_CASES = {
    # M, N, K, A k-fast, B k-fast, C transposed
    # a: ⌈1030/64⌉·⌈1950/64⌉ = 17·31 = 527 ≥ 512 → sgemm_grouped_kernel<64>
    "a-tm64": (1030, 1950, 37, True, True, True),
    # b: 17·⌈1920/64⌉ = 17·30 = 510 < 512 → sgemm_grouped_kernel<32>
    "b-tm32": (1030, 1920, 70, False, False, False),
}


def gemm_operands(cuda, M, N, K, a_kfast, b_kfast, seed):
    """(A64 (M, K), B64 (K, N), device A with (sam, sak), device B with (sbk, sbn))."""
    A = seeded(seed, (M, K))
    B = seeded(seed + 1, (K, N))
    Ad = (A if a_kfast else A.t()).contiguous().to(cuda)
    Bd = (B.t() if b_kfast else B).contiguous().to(cuda)
    sa = (K, 1) if a_kfast else (1, M)
    sb = (1, K) if b_kfast else (N, 1)
    return A.double(), B.double(), Ad, sa, Bd, sb


@pytest.mark.parametrize("case", list(GEMM_CASES))
def test_gemm_tile_switch(cuda, case):
    """C = 0.5·A·B + 2·C + bias at the two sizes of GEMM_CASES (527 and 510 64-tiles: one on each
    side of the host's switch), a: A row-major, B k-fast, C a transposed view (scm = 1, scn = M);
    b: A m-fast, B n-fast, C row-major. Bound: gemm_check."""
    from gfa_amd import ops
    M, N, K, a_kfast, b_kfast, c_t = GEMM_CASES[case]
    assert (tiles64([(M, N)]) >= 512) == (case == "a-tm64")
    assert tiles64([(M, N)]) == (527 if case == "a-tm64" else 510)
    A, B, Ad, (sam, sak), Bd, (sbk, sbn) = gemm_operands(cuda, M, N, K, a_kfast, b_kfast, 300 + K)
    C0 = seeded(310 + K, (M, N))
    bias = seeded(311 + K, (N,))
    Cd = (C0.t() if c_t else C0).contiguous().to(cuda)
    scm, scn = (1, M) if c_t else (N, 1)
    ops.gemm(M, N, K, 0.5, Ad, sam, sak, Bd, sbk, sbn, 2.0, Cd, scm, scn, bias.to(cuda))
    got = Cd.cpu().t() if c_t else Cd.cpu()
    gemm_check(case, got, A @ B, A.abs() @ B.abs(), C0, bias, 0.5, 2.0, K)


def test_gemm_beta_zero_does_not_read_c(cuda):
    """β = 0 with C pre-filled with NaN: the result is finite (C is not read) and within the
    bound of gemm_check. 527 64-tiles (the 64-tile kernel), A k-fast and B n-fast: exactly one
    operand is staged k-fast."""
    from gfa_amd import ops
    M, N, K = 1030, 1950, 37
    assert tiles64([(M, N)]) == 527
    A, B, Ad, (sam, sak), Bd, (sbk, sbn) = gemm_operands(cuda, M, N, K, True, False, 320)
    bias = seeded(322, (N,))
    Cd = torch.full((M, N), NAN, device=cuda)
    ops.gemm(M, N, K, 0.5, Ad, sam, sak, Bd, sbk, sbn, 0.0, Cd, N, 1, bias.to(cuda))
    got = Cd.cpu()
    assert torch.isfinite(got).all()
    gemm_check("beta=0", got, A @ B, A.abs() @ B.abs(), torch.zeros(M, N), bias, 0.5, 0.0, K)


# ---- 2. GemmPlan across the kMaxGroups split -----------------------------------------------------
def plan_case(cuda, M, Ns, tag):
    from gfa_amd import ops
    ng, K1, K2 = len(Ns), 33, 5
    lat = seeded(400 + M, (M, ng, K2))  # group i reads the strided row lat[:, i, :]
    latd = lat.to(cuda)
    plan = ops.GemmPlan()
    checks = []
    for i, N in enumerate(Ns):
        A1 = seeded(410 + i, (M, K1))
        B1 = seeded(430 + i, (N, K1))  # used transposed (k-fast)
        B2 = seeded(450 + i, (K2, N))
        C0 = seeded(470 + i, (M, N))
        bias = seeded(490 + i, (N,))
        two = i % 2 == 0
        ab = A1.double() @ B1.double().t()
        ab_abs = A1.double().abs() @ B1.double().abs().t()
        segs = [(A1.to(cuda), K1, 1, B1.to(cuda), 1, K1, K1)]
        if two:
            ab = ab + lat[:, i, :].double() @ B2.double()
            ab_abs = ab_abs + lat[:, i, :].double().abs() @ B2.double().abs()
            segs.append((latd[:, i, :], ng * K2, 1, B2.to(cuda), N, 1, K2))
        Cd = C0.clone().to(cuda)
        plan.add(Cd, N, 1, M, N, segs, alpha=0.5, beta=2.0, bias=bias.to(cuda))
        checks.append((Cd, ab, ab_abs, C0, bias, K1 + (K2 if two else 0)))
    plan.run()
    for i, (Cd, ab, ab_abs, C0, bias, K) in enumerate(checks):
        gemm_check(f"{tag} group {i}", Cd.cpu(), ab, ab_abs, C0, bias, 0.5, 2.0, K)


def test_gemm_plan_tm64_across_the_split(cuda):
    """13 groups of 200 × 700: ⌈200/64⌉·⌈700/64⌉ = 4·11 = 44 64-tiles per group, 13·44 = 572 ≥ 512
    → sgemm_grouped_kernel<64>, launched as 12 + 1 groups. Even groups sum two segments (K1 = 33
    k-fast, K2 = 5 from a strided row of a shared (M, 13, 5) tensor), odd groups have one;
    α = 0.5, β = 2, bias. Bound: gemm_check with K = K1 + K2 (the accumulator runs through both
    segments)."""
    Ns = [700] * 13
    assert tiles64([(200, n) for n in Ns]) == 572
    plan_case(cuda, 200, Ns, "plan tm64")


def test_gemm_plan_tm32_across_the_split(cuda):
    """13 groups of 200 × (33 + 7i): 4·(1·5 + 2·8) = 84 64-tiles < 512 → sgemm_grouped_kernel<32>,
    launched as 12 + 1 groups with a different N in each."""
    Ns = [33 + 7 * i for i in range(13)]
    assert tiles64([(200, n) for n in Ns]) == 84
    plan_case(cuda, 200, Ns, "plan tm32")


# ---- 4. style_demod ------------------------------------------------------------------------------
DEMOD_CIN = [1, 63, 64, 100, 449, 480, 512, 513, 1000, 1024]
DEMOD_COUT = [1, 3, 5, 96]


@pytest.mark.parametrize("Cout", DEMOD_COUT)
@pytest.mark.parametrize("Cin", DEMOD_CIN)
def test_style_demod_grid(cuda, Cin, Cout):
    """demod = rsqrt(scale2·(s²)·wsqᵀ + 1e-8) in fp64 from the fp32 s, wsq, scale2 and 1e-8, three
    images at IMG_SCALES, and again with image 1 at s = 0 (1e4 up to the rounding of rsqrt), at
    scale2 = 1 and 0.3. Every term is non-negative, so the bound is relative: (Cin + 8)·U covers
    the square, a lane's ⌈Cin/64⌉ fused terms, the 6 butterfly additions, scale2·acc, + 1e-8 and
    the hardware rsqrt (whose argument error is halved). Cin < 449 runs the tail loop alone,
    449 … 511 the 8-deep loop on the first lanes only, ≥ 512 on all; Cout % 4 ≠ 0 leaves waves of
    the last block without a row."""
    from gfa_amd import ops
    N = 3
    wsq = torch.rand((Cout, Cin), generator=torch.Generator().manual_seed(500 + Cin + Cout))
    s = seeded(501 + Cin, (N, Cin)) * scales(N).reshape(N, 1)
    s0 = s.clone()
    s0[1] = 0.0
    eps = f32(1e-8)
    worst = 0.0
    for scale2 in (1.0, 0.3):
        for tag, sv in (("scaled", s), ("zero", s0)):
            d = ops.style_demod(sv.to(cuda), wsq.to(cuda), torch.full((N, Cout), NAN, device=cuda),
                                scale2=scale2).cpu()
            ref = torch.rsqrt(f32(scale2) * (sv.double() ** 2) @ wsq.double().t() + eps)
            rel = ((d.double() - ref).abs() / ref)
            assert not torch.isnan(d).any()
            worst = max(worst, rel.max().item())
            assert (rel <= (Cin + 8) * U).all(), (scale2, tag, rel.max().item() / U)
            if tag == "zero":  # rsqrt(fp32(1e-8)) = 1e4·(1 + 3e-9), and the rsqrt's own rounding
                assert ((d[1].double() - 1e4).abs() <= 1e4 * 4 * U).all()
    print(f"style_demod Cin={Cin} Cout={Cout}: max rel err {worst / U:.3f} U (≤ {Cin + 8})")


# ---- 5. demod_bwd --------------------------------------------------------------------------------
@pytest.mark.parametrize("Cin", [1, 63, 65, 512])
@pytest.mark.parametrize("Cout", [1, 3, 5, 33, 96, 512])
def test_demod_bwd_grid(cuda, Cout, Cin):
    """gs = gs0 − scale2·s·Σ_co q·demod²·wsq[co] in fp64 from the fp32 inputs, gs pre-filled with
    seeded gs0, within (Cout + 8)·U·(|gs0| + scale2·|s|·Σ|q|·demod²·wsq): q·d·d (2 roundings), a
    quarter's ⌈Cout/4⌉ terms in order, the 3 additions of the quarters, −scale2·s·t (2) and the
    += (1): ⌈Cout/4⌉ + 8 ≤ Cout + 8. Cout < 4 leaves quarters empty, Cout/4 not a multiple of 8
    runs the per-quarter tail, Cin % 64 ≠ 0 leaves lanes of the last block idle."""
    from gfa_amd import ops
    N, scale2 = 3, 0.3
    q = seeded(600 + Cout, (N, Cout))
    demod = seeded(601 + Cout, (N, Cout)).abs() + 0.5
    wsq = torch.rand((Cout, Cin), generator=torch.Generator().manual_seed(602 + Cin + Cout))
    s = seeded(603 + Cin, (N, Cin)) * scales(N).reshape(N, 1)
    gs0 = seeded(604 + Cin, (N, Cin)) * scales(N).reshape(N, 1)
    gs = ops.demod_bwd(q.to(cuda), demod.to(cuda), wsq.to(cuda), s.to(cuda), gs0.clone().to(cuda),
                       scale2=scale2).cpu()
    r = q.double() * demod.double() ** 2
    t, t_abs = r @ wsq.double(), r.abs() @ wsq.double()
    ref = gs0.double() - f32(scale2) * s.double() * t
    mag = gs0.double().abs() + f32(scale2) * s.double().abs() * t_abs
    err = (gs.double() - ref).abs()
    assert not torch.isnan(gs).any()
    worst = (err / (U * mag).clamp_min(1e-300)).max().item()
    print(f"demod_bwd Cout={Cout} Cin={Cin}: max error {worst:.3f} U·Σ|terms| (≤ {Cout + 8})")
    assert (err <= (Cout + 8) * U * mag).all()
