"""The HBM-bound pointwise kernels of the attack step, each called directly and compared with a
plain fp64 reference of the same operation computed from the values as the device holds them
(after the cast to fp16 / bf16 where a 2-byte type applies): the fused L∞ update (mia_pgd_update)
and the image gradient, the average pool and its adjoint, the C&W tanh-space kernels, Adam, the
MSE reduction at every path of its finish, PixelNorm, the slice sum and the standalone bias /
activation.

Inputs come from seeded CPU generators, every image of a batch has its own scale (IMG_SCALES) so
that a value leaking from one image into another cannot hide, and every output buffer is
pre-filled with NaN or a sentinel so that an element a kernel skips fails its comparison. Bounds
are counts of fp32 roundings times U = 2⁻²⁴ (the relative error of one rounding); measured maxima
are printed."""
import ctypes
import ctypes.util
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_helpers import seeded
from oracle import attack_ref

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
U = 2.0 ** -24
IMG_SCALES = (1e4, 1.0, 1e-4)  # per-image scales: cross-image mixing cannot hide
NAN = float("nan")


def f32(v):
    return float(np.float32(v))


E, A, COEF = 16 / 255, 4 / 255, 0.37  # ε-ball, step and image-MSE weight of the pgd_update tests
E32, COEF32 = f32(E), f32(COEF)


def scales(n):
    return torch.tensor([IMG_SCALES[i % 3] for i in range(n)], dtype=F32)


def spacing(v64, mant_bits=24, min_exp=-149):
    """The format's spacing (1 ulp) at |v|: 2^(floor(log2|v|) − mant_bits + 1), no less than its
    subnormal spacing 2^min_exp. fp32: (24, −149); fp16: (11, −24); bf16: (8, −133)."""
    _, e = torch.frexp(v64.abs())  # |v| = m·2^e, m in [0.5, 1)
    e = torch.where(v64 == 0, torch.full_like(e, min_exp + mant_bits), e)
    return torch.pow(2.0, torch.clamp(e - mant_bits, min=min_exp).double())


SPACING = {F32: (24, -149), F16: (11, -24), BF16: (8, -133)}


# ---- pgd_update / image_grad: inputs and the fp64 gradient terms ---------------------------------
def pgd_inputs(S, pf, dtype, enc, vgg=True, enc_res=None, N=3, seed=0):
    """CPU inputs of the pixel-gradient assembly for N images, |x − x0| ≤ e. Rows 0 / 1 of x0 sit
    at +1 / −1 (the range clamp), rows 2 / 3 of x at x0 ± e (the ε-ball clamp). x == x0 in the
    left quarter of the columns, g_vgg is 0 in the left half of its columns and g_enc in the upper
    half of its rows, so every subset of the terms is exactly 0 somewhere. Channels ≥ 3 of g_vgg
    hold large values that no output may see."""
    from gfa_amd.weights import ENC_POOL_RES
    er = ENC_POOL_RES if enc_res is None else enc_res
    R = S // pf
    sc = scales(N).reshape(N, 1, 1, 1)
    x0 = seeded(seed + 1, (N, 3, S, S)) * 0.9
    x0[:, :, 0, :] = 1.0
    x0[:, :, 1, :] = -1.0
    dx = seeded(seed + 2, (N, 3, S, S)) * E32
    dx[:, :, :, :S // 4] = 0
    x = torch.clamp(x0 + dx, -1.0, 1.0)
    x[:, :, 2, :] = x0[:, :, 2, :] + E32
    x[:, :, 3, :] = x0[:, :, 3, :] - E32
    gv = ge = None
    if vgg:
        gv = seeded(seed + 3, (N, R, R, 8)) * sc
        gv[..., 3:] = 3e4
        gv[:, :, :R // 2, :3] = 0
        gv = gv.to(dtype)
    if enc:
        ge = seeded(seed + 4, (N, 3, er, er)) * sc
        ge[:, :, :er // 2, :] = 0
    return dict(x=x, x0=x0, gv=gv, ge=ge, pf=pf, er=er, S=S, N=N)


def pool_adjoint64(g_nchw, k):
    """fp64 gradient of Σ avg_pool2d(z, k)·g with respect to z (autograd)."""
    n, c, h, w = g_nchw.shape
    z = torch.zeros(n, c, h * k, w * k, dtype=torch.float64, requires_grad=True)
    (F.avg_pool2d(z, k) * g_nchw).sum().backward()
    return z.grad


def grad_terms64(d, a="x", b="x0", coef=COEF32):
    """The three terms of ∇_x L in fp64 from the values the device holds: coef·(x − x0), and the
    adjoints of avg_pool2d(pf) / avg_pool2d(S / enc_res) applied to the first three channels of
    g_vgg / to g_enc."""
    t_img = coef * (d[a].double() - d[b].double())
    t_vgg = torch.zeros_like(t_img)
    t_enc = torch.zeros_like(t_img)
    if d["gv"] is not None:
        t_vgg = pool_adjoint64(d["gv"][..., :3].permute(0, 3, 1, 2).double(), d["pf"])
    if d["ge"] is not None:
        t_enc = pool_adjoint64(d["ge"].double(), d["S"] // d["er"])
    return t_img, t_vgg, t_enc


def grad_terms64_at(d, idx):
    """grad_terms64 at the flat element indices idx only (index arithmetic instead of autograd:
    the 86-image case evaluates a sample)."""
    S, pf, er = d["S"], d["pf"], d["er"]
    R, ek = S // pf, S // er
    xx, yy = idx % S, (idx // S) % S
    c, n = (idx // (S * S)) % 3, idx // (3 * S * S)
    t_img = COEF32 * (d["x"].flatten()[idx].double() - d["x0"].flatten()[idx].double())
    t_vgg = torch.zeros_like(t_img)
    t_enc = torch.zeros_like(t_img)
    if d["gv"] is not None:
        cpad = d["gv"].shape[-1]
        j = ((n * R + yy // pf) * R + xx // pf) * cpad + c
        t_vgg = d["gv"].flatten()[j].double() / (pf * pf)
    if d["ge"] is not None:
        j = ((n * 3 + c) * er + yy // ek) * er + xx // ek
        t_enc = d["ge"].flatten()[j].double() / (ek * ek)
    return t_img, t_vgg, t_enc


def certain_sign(terms):
    """(sign(g64), mask of the elements whose sign no fp32 evaluation order can change, count of
    exactly-zero gradients). Each term carries at most two roundings (subtract and multiply; cast
    and divide) and two additions follow: the fp32 sum is within 4·U·(|t_img| + |t_vgg| + |t_enc|)
    of g64. Where every term is exactly 0 the fp32 sum is exactly 0 too."""
    g64 = terms[0] + terms[1] + terms[2]
    mag = terms[0].abs() + terms[1].abs() + terms[2].abs()
    certain = (g64.abs() > 4 * U * mag) | (mag == 0)
    return torch.sign(g64), certain, int((mag == 0).sum())


def dev(d, cuda, sl=slice(None)):
    """The device copies of d's tensors for the images sl."""
    return {k: (v[sl].contiguous().to(cuda) if torch.is_tensor(v) else v) for k, v in d.items()}


def run_pgd(dd, nonfinite="own"):
    from gfa_amd import ops
    x = dd["x"].clone()
    nf = (torch.zeros(x.shape[0], dtype=torch.int32, device=x.device) if nonfinite == "own"
          else nonfinite)
    ops.pgd_update(x, dd["x0"], dd["gv"], dd["ge"], dd["pf"], dd["er"], COEF, A, E, nonfinite=nf)
    return x, nf


def run_assemble_project(dd):
    """ops.sign_project of the gradient ops.grad_assemble materialises."""
    from gfa_amd import ops
    g = torch.full_like(dd["x"], NAN)
    ops.grad_assemble(dd["x"], dd["x0"], dd["gv"], dd["ge"], g, dd["pf"], dd["er"], COEF, 1.0)
    return ops.sign_project(dd["x"].clone(), dd["x0"], g, A, E), g


PGD_CASES = [
    # S, pf, dtype of g_vgg, encoder gradient, VGG gradient, enc_res (None: ENC_POOL_RES)
    (32, 1, F32, True, True, None), (32, 1, F16, True, True, None), (32, 2, BF16, True, True, None),
    (32, 4, F32, True, True, None),
    (20, 2, F32, False, True, None),  # 1200 elements per image: a partial last block
    (15, 3, F32, False, True, None),  # odd sizes, a pooling factor that is no power of two
    (32, 1, F32, True, False, None),  # the encoder gradient alone
    (32, 1, F32, False, False, None),  # the image term alone
    (32, 2, F32, True, True, 32),     # S / enc_res = 1 (ENC_POOL_RES = 16: 2 above)
]
PGD_IDS = [f"S{s}-pf{p}-{str(t).replace('torch.', '')}-enc{int(e)}-vgg{int(v)}-er{r}"
           for s, p, t, e, v, r in PGD_CASES]


@pytest.mark.parametrize("S,pf,dtype,enc,vgg,enc_res", PGD_CASES, ids=PGD_IDS)
def test_pgd_update(cuda, S, pf, dtype, enc, vgg, enc_res):
    """(a) x is bit-identical to ops.sign_project of ops.grad_assemble's gradient. (b) Wherever
    |g64| > 4·U·(|t_img| + |t_vgg| + |t_enc|) (two roundings per term at most, plus two additions:
    the sign is certain) x is bit-identical to oracle.attack_ref.project_step on the fp32 CPU with
    sign(g64); the elements left out are ≤ 0.1 % (measured: none in any case). Elements whose
    every term is exactly 0 take sign 0. A batch slice gives the bits of its row of the full
    call."""
    from gfa_amd.weights import ENC_POOL_RES
    assert ENC_POOL_RES == 16
    d = pgd_inputs(S, pf, dtype, enc, vgg, enc_res, seed=S + pf)
    dd = dev(d, cuda)
    got, nf = run_pgd(dd)
    want_dev, _ = run_assemble_project(dd)
    assert torch.equal(got, want_dev)
    assert nf.tolist() == [0, 0, 0]
    terms = grad_terms64(d)
    for t_full, t_at in zip(terms, grad_terms64_at(d, torch.arange(d["x"].numel()))):
        # the two references agree (to the last bit or two of fp64: ·(1/k²) against /k²)
        assert ((t_full.flatten() - t_at).abs() <= 2.0 ** -51 * t_at.abs()).all()
    sg, certain, nzero = certain_sign(terms)
    share = 1.0 - certain.double().mean().item()
    print(f"pgd_update {PGD_IDS[PGD_CASES.index((S, pf, dtype, enc, vgg, enc_res))]}: excluded "
          f"share {share:.2e}, exactly-zero gradients {nzero} of {sg.numel()}")
    assert share <= 1e-3
    assert nzero > 0
    want = attack_ref.project_step(d["x"], d["x0"], sg.float(), E, A)
    gc = got.cpu()
    assert torch.equal(gc[certain], want[certain])
    zero = sg == 0  # sign 0: only the projection moves x
    stay = torch.clamp(d["x0"] + torch.clamp(d["x"] - d["x0"], -E32, E32), -1.0, 1.0)
    assert torch.equal(gc[zero], stay[zero])
    # both clamps were exercised and hold
    assert gc.min() == -1.0 and gc.max() == 1.0
    assert ((gc - d["x0"]).abs() <= E32 + 2 * U).all()
    if vgg or enc:  # (the image term alone pulls x towards x0: the ε clamp is never reached)
        assert ((gc - d["x0"]).abs() >= E32 - 2 * U).any()
    got1, _ = run_pgd(dev(d, cuda, slice(1, 2)))
    assert torch.equal(got1[0], got[1])


def test_pgd_update_nonfinite_flags(cuda):
    """An inf in g_enc of image 1 flags image 1 alone and leaves the other images' bits; without
    a flag buffer the call completes with the same x."""
    d = pgd_inputs(32, 1, F32, True, seed=5)
    clean, _ = run_pgd(dev(d, cuda))
    d["ge"][1, 2, 9, 9] = float("inf")
    dd = dev(d, cuda)
    got, nf = run_pgd(dd)
    assert nf.tolist() == [0, 1, 0]
    assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2])
    assert torch.isfinite(got).all()
    got_noflag, _ = run_pgd(dd, nonfinite=None)
    assert torch.equal(got_noflag, got)


def test_pgd_update_past_the_block_cap(cuda):
    """N = 86 images of 256²: 86·196608 = 16 908 288 elements, the smallest batch of this size
    above 65536 blocks · 256 threads = 2²⁴, so the tail is done by the grid-stride loop. (a) on the
    device for the whole batch; (b) on the whole last image and on a random 1 % of the others."""
    N, S = 86, 256
    d = pgd_inputs(S, 1, F32, True, N=N, seed=77)
    assert d["x"].numel() > 65536 * 256 >= (N - 1) * 3 * S * S
    dd = dev(d, cuda)
    got, nf = run_pgd(dd)
    want_dev, g = run_assemble_project(dd)
    assert torch.equal(got, want_dev)
    assert not torch.isnan(g).any() and not nf.any()
    del want_dev, g
    plane = 3 * S * S
    gen = torch.Generator().manual_seed(78)
    sample = torch.randint((N - 1) * plane, ((N - 1) * plane // 100,), generator=gen)
    idx = torch.cat([sample, torch.arange((N - 1) * plane, N * plane)])
    sg, certain, nzero = certain_sign(grad_terms64_at(d, idx))
    share = 1.0 - certain.double().mean().item()
    print(f"pgd_update N=86 S=256: checked {idx.numel()} elements, excluded share {share:.2e}, "
          f"exactly-zero gradients {nzero}")
    assert share <= 1e-3 and nzero > 0
    want = attack_ref.project_step(d["x"].flatten()[idx], d["x0"].flatten()[idx], sg.float(), E, A)
    gc = got.cpu().flatten()[idx]
    assert torch.equal(gc[certain], want[certain])


@pytest.mark.parametrize("S,pf,dtype,vgg", [(s, p, t, v) for s, p, t, e, v, r in PGD_CASES[:6]]
                         + [(32, 1, F32, False)])
def test_image_grad(cuda, S, pf, dtype, vgg):
    """g_img = coef·(rec − t) + the adjoint of avg_pool2d(pf) of g_vgg's first three channels,
    within 3·U·(|coef·(rec − t)| + |adjoint|): subtract and multiply on the first term, the
    rounding of 1/pf² and the multiply on the second, and the addition (≤ 3·U·Σ|terms| in all).
    Where pf is a power of two (1/pf² exact) the result is bit-identical to ops.grad_assemble
    without an encoder gradient."""
    from gfa_amd import ops
    N, R = 3, S // pf
    sc = scales(N).reshape(N, 1, 1, 1)
    t = seeded(S + 11, (N, 3, S, S)) * 0.9
    rec = t + seeded(S + 12, (N, 3, S, S)) * 0.5 * sc
    gv = None
    if vgg:
        gv = seeded(S + 13, (N, R, R, 8)) * sc
        gv[..., 3:] = 3e4
        gv = gv.to(dtype)
    d = dict(rec=rec, t=t, gv=gv, ge=None, pf=pf, er=S, S=S, N=N)
    dd = dev(d, cuda)
    g = torch.full_like(dd["rec"], NAN)
    ops.image_grad(dd["rec"], dd["t"], dd["gv"], g, pf, COEF)
    t_img, t_vgg, _ = grad_terms64(d, "rec", "t")
    ref, mag = t_img + t_vgg, t_img.abs() + t_vgg.abs()
    err = (g.double().cpu() - ref).abs()
    worst = (err / (U * mag).clamp_min(1e-300)).max().item()
    print(f"image_grad S={S} pf={pf} {dtype} vgg={vgg}: max error {worst:.3f} U·Σ|terms| (≤ 3)")
    assert (err <= 3 * U * mag).all()
    if pf & (pf - 1) == 0:
        g2 = torch.full_like(g, NAN)
        ops.grad_assemble(dd["rec"], dd["t"], dd["gv"], None, g2, pf, S, COEF, 1.0)
        assert torch.equal(g, g2)


# ---- avg_pool2d(k, stride k) and its adjoint -----------------------------------------------------
POOL_CASES = [(5, 7, 9, 2),    # a remainder row and column: the forward floors
              (6, 32, 32, 4), (3, 15, 15, 3),
              (2, 8, 8, 8),    # one output per plane
              (4, 6, 10, 1)]   # the identity


def pool_run(cuda, planes, H, W, k):
    from gfa_amd import ops
    sc = scales(planes).reshape(planes, 1, 1)
    x = seeded(H * W + k, (planes, H, W)) * sc
    gy = seeded(H * W + k + 1, (planes, H // k, W // k)) * sc
    base = seeded(H * W + k + 2, (planes, H, W)) * sc
    xd, gyd = x.to(cuda), gy.to(cuda)
    y = ops.avgpool_fwd(xd, torch.full((planes, H // k, W // k), NAN, device=cuda), k)
    gx = ops.avgpool_bwd(gyd, torch.full((planes, H, W), NAN, device=cuda), k)
    gacc = ops.avgpool_bwd(gyd, base.clone().to(cuda), k, accumulate=True)
    return x, gy, base, y.cpu(), gx.cpu(), gacc.cpu()


@pytest.mark.parametrize("planes,H,W,k", POOL_CASES)
def test_avgpool_fwd_bwd(cuda, planes, H, W, k):
    """Forward against F.avg_pool2d in fp64 within (k² + 1)·U·mean|window| per output (k² − 1
    additions of partial sums bounded by Σ|window|, the rounding of 1/k² and the multiply).
    Backward against the fp64 autograd gradient within 2·U·|ref| (1/k², the multiply), and with
    accumulate within 2·U·|ref| + U·(|base| + |ref|) (the addition). The floor's remainder rows and
    columns get 0, or keep gx under accumulate. k = 1 is the identity, bit for bit. Adjointness:
    ⟨fwd(x), gy⟩ and ⟨x, bwd(gy)⟩, summed in fp64 from the device outputs, agree within
    (k² + 3)·U·Σ|x·bwd(gy)| (the two bounds above)."""
    x, gy, base, y, gx, gacc = pool_run(cuda, planes, H, W, k)
    x64 = x.double()[None].requires_grad_(True)
    ref = F.avg_pool2d(x64, k)
    ref.backward(gy.double()[None])
    ref, gref = ref.detach()[0], x64.grad[0]
    mean_abs = F.avg_pool2d(x.double().abs()[None], k)[0]
    e_f = ((y.double() - ref).abs() / (U * mean_abs)).max().item()
    assert ((y.double() - ref).abs() <= (k * k + 1) * U * mean_abs).all()
    assert not torch.isnan(gx).any()
    e_b = ((gx.double() - gref).abs() / (U * gref.abs()).clamp_min(1e-300)).max().item()
    assert ((gx.double() - gref).abs() <= 2 * U * gref.abs()).all()
    aref = base.double() + gref
    tol = 2 * U * gref.abs() + U * (base.double().abs() + gref.abs())
    e_a = ((gacc.double() - aref).abs() / tol.clamp_min(1e-300)).max().item()
    assert ((gacc.double() - aref).abs() <= tol).all()
    Hk, Wk = H // k * k, W // k * k
    rem = torch.ones(H, W, dtype=torch.bool)
    rem[:Hk, :Wk] = False
    assert (gx[:, rem] == 0).all() and torch.equal(gacc[:, rem], base[:, rem])
    assert rem.any() == (k == 2)
    if k == 1:
        assert torch.equal(y, x) and torch.equal(gx, gy)
    lhs = (y.double() * gy.double()).sum().item()
    rhs = (x.double() * gx.double()).sum().item()
    prod = (x.double() * gx.double()).abs().sum().item()
    e_adj = abs(lhs - rhs) / (U * prod)
    print(f"avgpool planes={planes} {H}x{W} k={k}: fwd {e_f:.3f} U·mean|window| (≤ {k * k + 1}), "
          f"bwd {e_b:.3f} U·|ref| (≤ 2), accumulate {e_a:.3f} of its bound, adjointness "
          f"{e_adj:.3f} U·Σ|products| (≤ {k * k + 3})")
    assert abs(lhs - rhs) <= (k * k + 3) * U * prod


def test_grad_assemble_terms_are_avgpool_bwd(cuda):
    """At S = 32, pf = 2 and x = x0 the VGG term of ops.grad_assemble is ops.avgpool_bwd(pf) of the
    NCHW-transposed g_vgg and its encoder term avgpool_bwd(S / enc_res) of g_enc, within 2·U
    relative per term (each is one value times or divided by the window size)."""
    from gfa_amd import ops
    d = pgd_inputs(32, 2, F32, True, seed=3)
    d["x"] = d["x0"].clone()
    dd = dev(d, cuda)
    S, pf, er = 32, 2, d["er"]
    for name, gv, ge, src, k in (("vgg", dd["gv"], None, dd["gv"][..., :3].permute(0, 3, 1, 2), pf),
                                 ("enc", None, dd["ge"], dd["ge"], S // er)):
        g = torch.full_like(dd["x"], NAN)
        ops.grad_assemble(dd["x"], dd["x0"], gv, ge, g, pf, er, COEF, 1.0)
        want = ops.avgpool_bwd(src.contiguous(), torch.full_like(g, NAN), k)
        err = (g.double() - want.double()).abs()
        worst = (err / (U * want.double().abs()).clamp_min(1e-300)).max().item()
        print(f"grad_assemble {name} term vs avgpool_bwd: max {worst:.3f} U relative (≤ 2)")
        assert (err <= 2 * U * want.double().abs()).all() and want.abs().max() > 1e3


# ---- C&W in tanh space ---------------------------------------------------------------------------
CW_SHAPE = (2, 3, 17, 17)  # 1734 elements: not a multiple of the 256-thread block
LIM = 1.0 - 2.0 ** -20


def ulps(got, ref64):
    """|got − ref| in fp32 spacings at the reference."""
    return (got.double() - ref64).abs() / spacing(ref64)


def cw_init_input():
    x = seeded(40, CW_SHAPE).flatten()
    for k, v in enumerate((1.0, 1.0 - 2.0 ** -20, 1.0 - 2.0 ** -24)):
        x[100 * k + 10:100 * k + 40] = v
        x[100 * k + 40:100 * k + 70] = -v
    x[400:430] = 0.0
    x[-1] = 1.0  # the tail of the last, partial block
    return x.reshape(CW_SHAPE)


def cw_tanh_input():
    w = seeded(41, CW_SHAPE).flatten() * 12
    w[5], w[6], w[7], w[-1] = 0.0, 20.0, -20.0, 20.0
    return w.reshape(CW_SHAPE)


def allowed_ulps(cpu_max):
    """The device's atanhf / tanhf may differ from the CPU's while both are faithful: twice the
    CPU's measured maximum plus 2 ulp."""
    return 2 * cpu_max + 2


def test_cw_init_tanh_and_round_trip(cuda):
    """cw_init against fp64 atanh of the fp32-clamped input (clamp ±(1 − 2⁻²⁰)), cw_tanh against
    fp64 tanh, in fp32 ulps of the reference; allowed: twice the maximum of torch's fp32 CPU result
    against the same reference, plus 2 ulp. Measured on MI355X (device / CPU, ulp): atanh
    0.525 / 0.715 (allowed 3.43), tanh 1.005 / 0.502 (allowed 3.00). The round trip
    cw_tanh(cw_init(x)) equals clamp(x, ±lim) within A·ulp(w)·(1 − xc²)·(1 + 2⁻¹⁰) + B·ulp(xc), A /
    B the allowed ulps of atanh / tanh (tanh' = 1 − tanh²; the factor covers the second-order term
    2·|t|·δw), and at x = ±1 it is within 2⁻¹⁹ of x."""
    from gfa_amd import ops
    x = cw_init_input()
    xc = torch.clamp(x, -f32(LIM), f32(LIM))
    assert (xc.abs().max().item() == LIM) and ((x.abs() == 1).sum() >= 60)
    w = ops.cw_init(x.to(cuda), torch.full(CW_SHAPE, NAN, device=cuda)).cpu()
    assert torch.isfinite(w).all()
    w64 = torch.atanh(xc.double())
    dev_a, cpu_a = ulps(w, w64).max().item(), ulps(torch.atanh(xc), w64).max().item()
    print(f"cw_init: atanh max error device {dev_a:.3f} ulp, CPU {cpu_a:.3f} ulp "
          f"(allowed {allowed_ulps(cpu_a):.3f})")
    assert dev_a <= allowed_ulps(cpu_a)
    assert (w[x == 0] == 0).all()

    wi = cw_tanh_input()
    adv = ops.cw_tanh(wi.to(cuda), torch.full(CW_SHAPE, NAN, device=cuda)).cpu()
    a64 = torch.tanh(wi.double())
    dev_t, cpu_t = ulps(adv, a64).max().item(), ulps(torch.tanh(wi), a64).max().item()
    print(f"cw_tanh: tanh max error device {dev_t:.3f} ulp, CPU {cpu_t:.3f} ulp "
          f"(allowed {allowed_ulps(cpu_t):.3f})")
    assert dev_t <= allowed_ulps(cpu_t)
    assert (adv.abs() <= 1).all() and adv.flatten()[5] == 0
    assert adv.flatten()[6] == 1 and adv.flatten()[7] == -1 and adv.flatten()[-1] == 1

    rt = ops.cw_tanh(w.to(cuda), torch.full(CW_SHAPE, NAN, device=cuda)).cpu()
    xc64 = xc.double()
    tol = (allowed_ulps(cpu_a) * spacing(w64) * (1 - xc64 * xc64) * (1 + 2.0 ** -10)
           + allowed_ulps(cpu_t) * spacing(xc64))
    err = (rt.double() - xc64).abs()
    print(f"cw round trip: max error {(err / tol).max().item():.3f} of its bound, "
          f"max |rt − x| at x = ±1 {(rt - x).abs()[x.abs() == 1].max().item():.3e} (≤ 2⁻¹⁹)")
    assert (err <= tol).all()
    assert ((rt - x).abs()[x.abs() == 1] <= 2.0 ** -19).all()


@pytest.mark.parametrize("c", [1e-4, 10.0])
@pytest.mark.parametrize("scale", [1.0, 1.0 / 1024])
def test_cw_grad(cuda, c, scale):
    """g_w = (½(adv − x) + c·scale·g_f)·(1 − adv²) against fp64 within 8·U·T·(1 + adv²), T = |½(adv
    − x)| + |c·scale·g_f|: the subtraction, c·scale, ·g_f, the addition, adv², 1 − adv² and the
    final multiply sum to ≤ 5·U·T·(1 + adv²) with or without fused multiply-adds (the halving is
    exact); the margin is 1.6×."""
    from gfa_amd import ops
    n = math.prod(CW_SHAPE)
    adv = seeded(42, CW_SHAPE).flatten()
    adv[10:20], adv[20:30] = 1.0, -1.0
    near = seeded(43, (40,)).abs() * 2.0 ** -12
    adv[30:50], adv[50:70] = 1.0 - near[:20], -1.0 + near[20:]
    adv[-1] = 1.0 - 2.0 ** -13
    adv = adv.reshape(CW_SHAPE)
    x = seeded(44, CW_SHAPE)
    gf = seeded(45, CW_SHAPE) * torch.tensor([1e4, 1e-4]).reshape(2, 1, 1, 1)
    gw = ops.cw_grad(adv.to(cuda), x.to(cuda), gf.to(cuda), torch.full(CW_SHAPE, NAN, device=cuda),
                     c, scale).cpu()
    a64, cs = adv.double(), f32(c) * f32(scale)
    t1, t2 = 0.5 * (a64 - x.double()), cs * gf.double()
    ref = (t1 + t2) * (1 - a64 * a64)
    unit = U * (t1.abs() + t2.abs()) * (1 + a64 * a64)
    err = (gw.double() - ref).abs()
    print(f"cw_grad c={c} scale={scale}: max error {(err / unit).max().item():.3f} "
          f"U·T·(1 + adv²) (≤ 8) over {n} elements")
    assert (err <= 8 * unit).all()
    assert (gw.flatten()[10:30] == 0).all()  # adv = ±1: 1 − adv² = 0


def test_cw_select(cuda):
    """The seven rows of the docstring table: a row is taken iff f < f0 and l2 < best_l2, both
    strict, l2 = the fp32 product l2_scale·sq. Taken rows equal adv over the whole 867-element
    plane, the others keep the sentinel and their best_l2; a second identical call is a no-op."""
    from gfa_amd import ops
    N, plane, l2_scale, SENT = 7, 3 * 17 * 17, 0.3, 123456.0
    inf, up = float("inf"), np.float32(np.inf)
    sq = (seeded(46, (N,)).abs() + 0.5) * scales(N)
    l2 = (np.float32(l2_scale) * sq.numpy()).astype(np.float32)
    f0 = (seeded(47, (N,)) * 3).numpy().astype(np.float32)
    f = f0.copy()
    best = l2.copy()
    # row 1: take, by one ulp on either comparison
    f[0], best[0] = np.nextafter(f0[0], -up), np.nextafter(l2[0], up)
    f[1], best[1] = f0[1] - 1.0, inf                     # 2: best_l2 = +inf: take
    f[2], best[2] = f0[2] - 1.0, l2[2]                   # 3: l2 == best_l2: no take
    f[3], best[3] = f0[3], inf                           # 4: f == f0: no take
    f[4], best[4] = np.nextafter(f0[4], up), inf         # 5: f > f0: no take
    f[5], best[5] = np.nan, inf                          # 6: f = NaN: no take
    f[6], best[6] = f0[6] - 1.0, np.nextafter(l2[6], -up)  # 7: l2 > best_l2: no take
    taken = [True, True, False, False, False, False, False]
    adv = (seeded(48, (N, 3, 17, 17)) * scales(N).reshape(N, 1, 1, 1)).to(cuda)
    best_adv = torch.full((N, 3, 17, 17), SENT, device=cuda)
    sq_d, f_d, f0_d = sq.to(cuda), torch.from_numpy(f).to(cuda), torch.from_numpy(f0).to(cuda)
    best_d = torch.from_numpy(best.copy()).to(cuda)
    for call in range(2):
        ops.cw_select(adv, best_adv, sq_d, best_d, f_d, f0_d, l2_scale)
        got_best = best_d.cpu().numpy()
        for n in range(N):
            if taken[n]:
                assert torch.equal(best_adv[n], adv[n]), (call, n)
                assert got_best[n] == l2[n], (call, n)
            else:
                assert (best_adv[n] == SENT).all(), (call, n)
                assert got_best[n].tobytes() == best[n].tobytes(), (call, n)
    print(f"cw_select: rows taken {taken}, plane {plane}")
    assert best_adv[0].numel() == plane


# ---- Adam ----------------------------------------------------------------------------------------
def _powf(base, t):
    """The host's C powf, which the launcher calls (numpy's float32 power where there is none)."""
    name = ctypes.util.find_library("m")
    if name is None:
        return np.power(np.float32(base), np.float32(t))
    fn = ctypes.CDLL(name).powf
    fn.restype, fn.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
    return np.float32(fn(float(np.float32(base)), float(t)))


def adam_check(tag, p0, g, m0, v0, p1, m1, v1, lr, b1, b2, eps, t):
    """One device step (p0, m0, v0) → (p1, m1, v1) against fp64 Adam from the device-held state
    with the launcher's fp32 bias corrections."""
    b1f, b2f = np.float32(b1), np.float32(b2)
    bc1 = float(np.float32(1) - _powf(b1f, t))
    bc2s = float(np.sqrt(np.float32(1) - _powf(b2f, t), dtype=np.float32))
    b1d, b2d, lrd, epsd = float(b1f), float(b2f), f32(lr), f32(eps)
    g64, m64, v64, p64 = g.double(), m0.double(), v0.double(), p0.double()
    m_ref = m64 + (1 - b1d) * (g64 - m64)
    v_ref = v64 * b2d + (1 - b2d) * g64 * g64
    e_m = (m1.double() - m_ref).abs() / (U * (m64.abs() + g64.abs())).clamp_min(1e-300)
    e_v = (v1.double() - v_ref).abs() / (U * v_ref).clamp_min(1e-300)
    # p from the moments the device stored (the kernel uses those very values)
    upd = (lrd / bc1) * (m1.double() / (v1.double().sqrt() / bc2s + epsd))
    p_ref = p64 - upd
    tol = U * p_ref.abs() + 8 * U * upd.abs()
    e_p = (p1.double() - p_ref).abs() / tol.clamp_min(1e-300)
    print(f"adam {tag}: m {e_m.max().item():.3f} U·(|m| + |g|) (≤ 3), v {e_v.max().item():.3f} "
          f"U·v (≤ 4), p {e_p.max().item():.3f} of U·|p| + 8·U·lr/bc1·|m/denom|")
    assert (e_m <= 3).all() and (e_v <= 4).all() and (e_p <= 1).all()


@pytest.mark.parametrize("n", [1, 257, 5000])
def test_adam_step_ref(cuda, n):
    """Five steps from zero moments and one step at t = 1000 from given moments, each step against
    fp64 Adam from the state the device held before it, with the fp32 bias corrections 1 − β₁ᵗ and
    sqrt(1 − β₂ᵗ) as the launcher computes them (powf). Per element: m within 3·U·(|m| + |g|)
    (subtract, multiply, add), v within 4·U·v (three multiplies and the addition of non-negative
    terms), p within U·|p| + 8·U·lr/bc1·|m/denom| (sqrt, divide, add eps, lr/bc1, m/denom, the
    product: 6, and the subtraction). g = 0 with m = v = 0: denom = eps and p keeps its bits."""
    from gfa_amd import ops
    lr, b1, b2, eps = 0.005, 0.9, 0.999, 1e-8
    seg = torch.tensor([IMG_SCALES[(3 * i) // n] for i in range(n)])
    dead = torch.zeros(n, dtype=torch.bool)
    if n > 1:
        dead[n // 2:n // 2 + 7] = True  # gradient 0 at every step
    p = seeded(50 + n, (n,))
    pd = p.clone().to(cuda)
    m, v = torch.zeros(n, device=cuda), torch.zeros(n, device=cuda)
    for t in range(1, 6):
        g = seeded(60 + n + t, (n,)) * seg
        g[dead] = 0
        p0, m0, v0 = pd.cpu().clone(), m.cpu().clone(), v.cpu().clone()
        ops.adam_step(pd, g.to(cuda), m, v, lr, b1, b2, eps, t)
        adam_check(f"n={n} t={t}", p0, g, m0, v0, pd.cpu(), m.cpu(), v.cpu(), lr, b1, b2, eps, t)
        assert torch.equal(pd.cpu()[dead], p[dead])
        assert (m.cpu()[dead] == 0).all() and (v.cpu()[dead] == 0).all()
    g = seeded(70 + n, (n,)) * seg
    m0 = seeded(71 + n, (n,)) * seg
    v0 = (seeded(72 + n, (n,)) * seg) ** 2
    p0 = seeded(73 + n, (n,))
    pd, m, v = p0.clone().to(cuda), m0.clone().to(cuda), v0.clone().to(cuda)
    ops.adam_step(pd, g.to(cuda), m, v, lr, b1, b2, eps, 1000)
    adam_check(f"n={n} t=1000", p0, g, m0, v0, pd.cpu(), m.cpu(), v.cpu(), lr, b1, b2, eps, 1000)


# ---- MSE reduction -------------------------------------------------------------------------------
MSE_LENGTHS = [1,        # one element
               255,      # a partial block
               32768,    # 128 slots: the last single-pass finish
               32769,    # 129 slots: the first chunked finish
               262144,   # 1024 slots: the cap
               262657]   # past the cap: the grid-stride loop (513 threads add two squares)


def mse_chain(L):
    """Longest chain of roundings on non-negative terms behind one loss: ceil(L / 262144)
    additions per thread and the square, 6 butterfly levels, 4 wave sums, the coef multiply, and at
    most 64 + 16 additions in the ordered finish."""
    return -(-L // 262144) + 1 + 6 + 4 + 1 + 64 + 16


@pytest.mark.parametrize("dtype", [F32, F16, BF16])
@pytest.mark.parametrize("L", MSE_LENGTHS)
def test_mse_sum_ref(cuda, L, dtype):
    """loss[n] = coef·Σ(a − b)² per image against the fp64 sum of the device-held values, relative
    error ≤ 3·mse_chain(L)·U = 3·(ceil(L / 262144) + 92)·U (every term is non-negative; 3× margin,
    which also holds the two roundings of the subtraction and the 128 additions of the single-pass
    finish at 65 … 128 slots). Bit-identical reruns, a batch slice gives its row's bits, and the
    result is added to what loss holds."""
    from gfa_amd import ops
    n = 3
    sc = scales(n).reshape(n, 1)
    a = (seeded(80 + L % 97, (n, L)) * sc).to(dtype)
    b = (seeded(81 + L % 97, (n, L)) * sc).to(dtype)
    ad, bd = a.to(cuda), b.to(cuda)
    loss = ops.mse_sum(ad, bd, torch.zeros(n, device=cuda), COEF)
    d64 = a.double() - b.double()
    ref = COEF32 * (d64 * d64).sum(1)
    err = ((loss.double().cpu() - ref).abs() / ref).max().item()
    bound = 3 * mse_chain(L) * U
    print(f"mse_sum L={L} {dtype}: max rel err {err:.3e} = {err / U:.2f} U (≤ {bound / U:.0f} U)")
    assert err <= bound
    if L >= 255:  # the sums span the per-image scales: nothing leaked between images
        assert loss[0] > 1e6 * loss[1] > 1e12 * loss[2] > 0
    again = ops.mse_sum(ad, bd, torch.zeros(n, device=cuda), COEF)
    assert torch.equal(again, loss)
    one = ops.mse_sum(ad[1:2].contiguous(), bd[1:2].contiguous(), torch.zeros(1, device=cuda), COEF)
    assert torch.equal(one[0], loss[1])
    acc = ops.mse_sum(ad, bd, torch.full((n,), 0.5, device=cuda), COEF)
    assert torch.equal(acc, 0.5 + loss)


# ---- PixelNorm -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [1, 63, 64, 256, 257, 512, 1000])
def test_pixel_norm_ref(cuda, cols):
    """y = x / sqrt(mean(x²) + eps) per row in fp64, relative error per element ≤
    (ceil(cols / 256) + 6 + 4 + 4)·U: the per-thread additions, 6 butterfly levels, 4 wave sums,
    and the divide, the add, the hardware reciprocal square root and the multiply. Rows at 1e15, 1
    and 1e-15 (eps = 1e-8 dominates the last; same formula) and an all-zero row, which stays 0."""
    from gfa_amd import ops
    eps = 1e-8
    x = seeded(90 + cols, (4, cols)) * torch.tensor([1e15, 1.0, 1e-15, 0.0]).reshape(4, 1)
    y = ops.pixel_norm(x.to(cuda), torch.full((4, cols), NAN, device=cuda), eps).cpu()
    x64 = x.double()
    ref = x64 / torch.sqrt((x64 * x64).mean(1, keepdim=True) + f32(eps))
    bound = (-(-cols // 256) + 6 + 4 + 4) * U
    assert torch.isfinite(y).all() and (y[3] == 0).all()
    err = (y.double() - ref).abs()[:3] / ref.abs()[:3].clamp_min(1e-300)
    rows = err.max(1).values / U
    print(f"pixel_norm cols={cols}: max rel err per row (1e15, 1, 1e-15) "
          f"{[round(r, 3) for r in rows.tolist()]} U (≤ {bound / U:.0f} U)")
    assert (err <= bound).all()
    assert (ref[2].abs() <= 1.1e-11).all() and ref[0].abs().max() > 0.5  # eps dominates row 2 only


# ---- slice sum -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,S,D", [(3, 18, 512), (2, 1, 5), (1, 7, 257)])
def test_sum_slices_ref(cuda, N, S, D):
    """y[n][d] = Σ_s x[n][s][d] against fp64 within (S − 1)·U·Σ_s|x| (S − 1 additions of partial
    sums bounded by Σ|x|); S = 1 copies the bits."""
    from gfa_amd import ops
    x = seeded(100 + D, (N, S, D)) * scales(N).reshape(N, 1, 1)
    y = ops.sum_slices(x.to(cuda), torch.full((N, D), NAN, device=cuda)).cpu()
    ref, mag = x.double().sum(1), x.double().abs().sum(1)
    err = (y.double() - ref).abs()
    print(f"sum_slices N={N} S={S} D={D}: max error {(err / (U * mag)).max().item():.3f} "
          f"U·Σ|x| (≤ {S - 1})")
    assert (err <= (S - 1) * U * mag).all()
    if S == 1:
        assert torch.equal(y, x[:, 0])


# ---- standalone bias / activation ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F16, BF16])
@pytest.mark.parametrize("N,H,W,C", [(2, 5, 7, 8), (1, 16, 16, 32)])
@pytest.mark.parametrize("parts", ["noise+bias", "bias", "noise"])
def test_bias_act_fwd_ref(cuda, dtype, N, H, W, C, parts):
    """y = leaky_relu(x + nw·noise[p] + b[c], 0.2)·√2 in fp64 from the device-held x, with the
    kernel's fp32 constants 0.2 and √2. fp32: within 4·U·(|x| + |nw·noise| + |b|)·slope·√2 (the
    noise multiply, two additions, the slope and the √2 multiplies; relative to the terms, whose
    sum may cancel). fp16 / bf16: within 1 ulp of the dtype of the reference rounded to it."""
    from gfa_amd import ops
    nw = 0.3
    x = (seeded(110 + C, (N, H, W, C)) * scales(N).reshape(N, 1, 1, 1)).to(dtype)
    noise = seeded(111 + C, (H * W,)) if "noise" in parts else None
    bias = seeded(112 + C, (C,)) if "bias" in parts else None
    y = ops.bias_act_fwd(x.to(cuda), noise.to(cuda) if noise is not None else None, nw,
                         bias.to(cuda) if bias is not None else None,
                         torch.full((N, H, W, C), NAN, dtype=dtype, device=cuda)).cpu()
    tn = (f32(nw) * noise.double()).reshape(1, H, W, 1) if noise is not None else torch.zeros(())
    tb = bias.double().reshape(1, 1, 1, C) if bias is not None else torch.zeros(())
    s = x.double() + tn + tb
    slope = torch.where(s > 0, torch.ones_like(s), torch.full_like(s, f32(0.2)))
    slope = slope * f32(math.sqrt(2.0))
    ref = s * slope
    if dtype == F32:
        unit = U * (x.double().abs() + tn.abs() + tb.abs()) * slope
        err = (y.double() - ref).abs() / unit.clamp_min(1e-300)
        print(f"bias_act_fwd fp32 {N}x{H}x{W}x{C} {parts}: max error {err.max().item():.3f} "
              f"U·Σ|terms|·slope·√2 (≤ 4)")
        assert (err <= 4).all()
    else:
        ref_r = ref.to(dtype).double()
        err = (y.double() - ref_r).abs() / spacing(ref_r, *SPACING[dtype])
        print(f"bias_act_fwd {dtype} {N}x{H}x{W}x{C} {parts}: max error {err.max().item():.3f} "
              f"ulp of the dtype (≤ 1)")
        assert (err <= 1).all()


@pytest.mark.parametrize("dtype,C", [(F32, 6), (F16, 4), (BF16, 12)])
def test_bias_act_fwd_refuses_a_partial_vector(cuda, dtype, C):
    from gfa_amd import ops
    from gfa_amd._lib import MiaError
    x = torch.zeros(1, 2, 2, C, dtype=dtype, device=cuda)
    with pytest.raises(MiaError, match="vector width"):
        ops.bias_act_fwd(x, None, 0.0, None, torch.empty_like(x))
