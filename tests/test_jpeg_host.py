"""The JPEG stage on the host: the quantiser tables against Pillow's, the fp32 reference of the
round trip (tests/jpeg_ref.py, the kernels' operation order) against its fp64 form and against
Pillow's own save-then-load, the fp32 adjoint against fp64 autograd on the surrogate, and
attack()'s argument validation before any device work. No GPU."""
import io

import numpy as np
import pytest
import torch

import jpeg_ref
from test_si_host import _StubNet

U = 2.0 ** -24
QUALITIES = (30, 75, 95)
TIE = 1e-3  # a coefficient is a near-tie when |frac(v) − ½| < TIE


@pytest.fixture(scope="module")
def image():
    return jpeg_ref.test_image(0, 64)


def qtab(q):
    from gfa_amd import jpeg_quant_tables
    return jpeg_quant_tables(q).to(torch.float32)


def test_quant_tables_ijg_scaling():
    from gfa_amd import jpeg_quant_tables
    from gfa_amd.pgd import JPEG_CHROMA, JPEG_LUMA
    t50 = jpeg_quant_tables(50)
    assert t50.dtype == torch.int64 and tuple(t50.shape) == (2, 64)
    assert t50[0].tolist() == list(JPEG_LUMA) and t50[1].tolist() == list(JPEG_CHROMA)
    assert len(JPEG_LUMA) == 64 and len(JPEG_CHROMA) == 64
    assert jpeg_quant_tables(100).eq(1).all()                       # s = 0: every step clamps to 1
    assert jpeg_quant_tables(1).eq(255).all()                       # s = 5000: all clamp to 255
    t75 = jpeg_quant_tables(75)                                     # s = 50
    assert t75[0][:8].tolist() == [8, 6, 5, 8, 12, 20, 26, 31]
    assert t75[1][:8].tolist() == [9, 9, 12, 24, 50, 50, 50, 50]
    assert jpeg_quant_tables(np.int64(10))[0][0].item() == (16 * 500 + 50) // 100
    for bad in (0, 101, -5, 75.0, True, "75", None, [75]):
        with pytest.raises(ValueError, match="jpeg_quality"):
            jpeg_quant_tables(bad)


@pytest.mark.parametrize("q", (10, 30, 50, 75, 95))
def test_quant_tables_match_pillow(q):
    """The tables Pillow writes at quality=q, as multisets (Pillow's order has changed between
    releases)."""
    Image = pytest.importorskip("PIL.Image")
    from gfa_amd import jpeg_quant_tables
    buf = io.BytesIO()
    Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(buf, "JPEG", quality=q, subsampling=0)
    tables = Image.open(io.BytesIO(buf.getvalue())).quantization
    ours = jpeg_quant_tables(q)
    assert sorted(tables[0]) == sorted(ours[0].tolist())
    assert sorted(tables[1]) == sorted(ours[1].tolist())


def test_dct_matrix():
    """D is what the kernels hold (csrc/jpeg.hip: seven constants and their signs), and it is
    orthonormal to fp32 rounding."""
    from gfa_amd import jpeg_dct_matrix
    D = jpeg_dct_matrix()
    assert D.dtype == torch.float32 and tuple(D.shape) == (8, 8)
    c = {k: float.fromhex(h) for k, h in (
        (1, "0x1.f6297cp-2"), (2, "0x1.d906bcp-2"), (3, "0x1.a9b662p-2"), (4, "0x1.6a09e6p-2"),
        (5, "0x1.1c73b4p-2"), (6, "0x1.87de2ap-3"), (7, "0x1.8f8b84p-4"))}
    want = [[4, 4, 4, 4, 4, 4, 4, 4], [1, 3, 5, 7, -7, -5, -3, -1], [2, 6, -6, -2, -2, -6, 6, 2],
            [3, -7, -1, -5, 5, 1, 7, -3], [4, -4, -4, 4, 4, -4, -4, 4],
            [5, -1, 7, 3, -3, -7, 1, -5], [6, -2, 2, -6, -6, 2, -2, 6],
            [7, -5, 3, -1, 1, -3, 5, -7]]
    want = torch.tensor([[np.sign(k) * c[abs(k)] for k in row] for row in want],
                        dtype=torch.float64)
    assert torch.equal(D.double(), want)
    eye = D.double() @ D.double().T
    assert (eye - torch.eye(8, dtype=torch.float64)).abs().max() < 8 * U


@pytest.mark.parametrize("q", QUALITIES)
def test_roundtrip_fp32_against_fp64(image, q):
    """The quantised coefficients of the fp32 reference equal the fp64 ones everywhere except
    near-ties, |frac(v) − ½| < 1e-3 (either precision), whose share is capped at 0.5 %; the output
    pixels are equal wherever every coefficient of their 8 × 8 block (three channels: the colour
    conversion mixes them) agrees."""
    y32, v32 = jpeg_ref.roundtrip32(image, qtab(q))
    y64, v64 = jpeg_ref.roundtrip64(image, qtab(q))
    near = (((v64 - torch.floor(v64)) - 0.5).abs() < TIE) | \
        (((v32.double() - torch.floor(v32.double())) - 0.5).abs() < TIE)
    differ = torch.round(v32).double() != torch.round(v64)
    share = near.double().mean().item()
    print(f"jpeg q={q}: near-tie share {100 * share:.3f} %, coefficient mismatches "
          f"{int(differ.sum())} (outside near-ties {int((differ & ~near).sum())}), "
          f"max |v32 - v64| {float((v32.double() - v64).abs().max()):.2e}")
    assert share <= 0.005
    assert not (differ & ~near).any()
    # blocks whose 3 × 64 coefficients all agree: (N, S/8, S/8)
    same = ~differ.any(dim=5).any(dim=3).any(dim=1)
    px = same[:, None, :, None, :, None].expand(-1, 3, -1, 8, -1, 8).reshape(image.shape)
    p32, p64 = (y32.double() + 1.0) * 127.5, (y64 + 1.0) * 127.5
    print(f"jpeg q={q}: {int(same.sum())} of {same.numel()} blocks agree in every coefficient; "
          f"pixel mismatches inside them {int((p32[px] - p64[px]).abs().gt(0.5).sum())}")
    assert same.double().mean() > 0.5
    # as 8-bit levels: p'/127.5 − 1 rounds twice in fp32 and never in fp64, the level is exact
    assert torch.equal(torch.round(p32[px]), torch.round(p64[px]))
    # J maps onto the 8-bit grid, and the round trip really quantises
    lv = (y32.double() + 1.0) * 127.5
    assert (lv - torch.round(lv)).abs().max() < 1e-4 and lv.min() >= -1e-4 and lv.max() <= 255.0001
    assert (y32 - image).abs().mean() > 1e-3


def _abs_ops(x, g, q):
    """The fp64 magnitudes the adjoint's error bound is made of (see the test below)."""
    Dm = jpeg_ref.jpeg_dct_matrix().double().abs()
    A = torch.tensor(jpeg_ref.A, dtype=torch.float64).abs()
    M = torch.tensor([[1.0, 0.0, jpeg_ref.M_R_CR], [1.0, jpeg_ref.M_G_CB, jpeg_ref.M_G_CR],
                      [1.0, jpeg_ref.M_B_CB, 0.0]], dtype=torch.float64).abs()

    def dct_abs(b):
        return torch.einsum("ui,ncyixj,vj->ncyuxv", Dm, b, Dm)

    def idct_abs(f):
        return torch.einsum("ui,ncyuxv,vj->ncyixj", Dm, f, Dm)

    p = jpeg_ref.pixels(x.double())
    ycc = torch.einsum("kc,nchw->nkhw", A, p)
    ycc[:, 0] += 128.0
    qb = jpeg_ref._qblocks(q, p)
    v_abs = dct_abs(jpeg_ref._blocks(ycc)) / qb
    h_abs = dct_abs(jpeg_ref._blocks(torch.einsum("ck,nchw->nkhw", M, g.double().abs())))
    v, _ = jpeg_ref.coefficients(x.double(), q)
    w = 3.0 * (v - torch.round(v)) ** 2

    def back(t):
        return torch.einsum("kc,nkhw->nchw", A, idct_abs(t).reshape(x.shape))
    return back(w * h_abs), back(v_abs * h_abs)


@pytest.mark.parametrize("q", QUALITIES)
def test_adjoint_fp32_against_fp64_autograd(image, q):
    """|gx32 − gx64| ≤ 3·2⁻²⁴·(39·B_lin + 63·B_w) elementwise, derived from the operation count:

    * the linear chain Aᵀ·IDCT·diag(w)·DCT·Mᵀ puts at most 3 (Mᵀ: a product and two additions on
      any term) + 8 + 8 (the two DCT passes: 8 products and 7 additions each) + 1 (w·H) + 8 + 8
      (IDCT) + 3 (Aᵀ) = 39 roundings on any term, so that part is within 39·2⁻²⁴ of
      B_lin = |A|ᵀ·|IDCT|·(w ⊙ |DCT|·|M|ᵀ·|g|), the same chain on magnitudes (‖g‖-scaled);
    * w = 3·(v − round(v))² carries the error of the fp32 coefficient v: at most 4 (YCbCr: a
      product, two additions, − 128) + 8 + 8 (DCT) + 1 (the division) = 21 roundings on any term of
      V_abs = |DCT|·(|A|·p + 128)/Q, so |Δv| ≤ 21·2⁻²⁴·V_abs. v − round(v) is exact (Sterbenz), and
      |dw/dv| = 6·|v − round(v)| ≤ 3 — w is continuous across ties, so a coefficient that rounds
      the other way in fp32 changes nothing here: |Δw| ≤ 63·2⁻²⁴·V_abs and that part is within
      B_w = |A|ᵀ·|IDCT|·(V_abs ⊙ |DCT|·|M|ᵀ·|g|) times 63·2⁻²⁴;
    * × 3, the repository's usual margin.
    A worst case over every term, so it is loose: measured on this image the worst |err| / bound is
    6.2e-5 (q = 30), 8.0e-5 (q = 75), 6.9e-5 (q = 95), max |err| 2.6e-6, 5.6e-6, 3.5e-5 at
    max |gx| ≈ 1. The sharp checks are the transpose identity below and, on the GPU, the kernel
    against adjoint32 bit for bit."""
    gen = torch.Generator().manual_seed(7)
    g = torch.randn(image.shape, generator=gen)
    g32 = jpeg_ref.adjoint32(image, g, qtab(q))
    g64 = jpeg_ref.adjoint64(image, g, qtab(q))
    b_lin, b_w = _abs_ops(image, g, qtab(q))
    bound = 3 * U * (39 * b_lin + 63 * b_w)
    err = (g32.double() - g64).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"jpeg adjoint q={q}: worst |err| / bound = {ratio:.2e}, max |err| {err.max():.2e}, "
          f"max |gx| {g64.abs().max():.2e}")
    assert torch.isfinite(g32).all() and g64.abs().max() > 0
    assert (err <= bound).all()


def test_adjoint_is_the_transpose(image):
    """⟨J′u, g⟩ = ⟨u, J′ᵀg⟩: the fp32 adjoint against the forward-mode product (autograd's jvp)
    of the fp64 surrogate at x, to 1e-5 of Σ|J′u|·|g| (the elementwise bound above is a worst
    case and far looser). A transposed colour matrix or a swapped pass order cannot pass."""
    q = qtab(75)
    gen = torch.Generator().manual_seed(11)
    u = torch.randn(image.shape, generator=gen, dtype=torch.float64)
    g = torch.randn(image.shape, generator=gen, dtype=torch.float64)
    _, ju = torch.autograd.functional.jvp(lambda t: jpeg_ref.surrogate64(t, q), image.double(), u)
    lhs = (ju * g).sum().item()
    rhs = (u * jpeg_ref.adjoint32(image, g.float(), q).double()).sum().item()
    scale = (ju.abs() * g.abs()).sum().item()
    print(f"jpeg adjoint identity: <J'u,g> = {lhs:.9e}, <u,J'^T g> = {rhs:.9e}, scale {scale:.3e}")
    assert abs(lhs - rhs) <= 1e-5 * scale


def test_roundtrip_against_pillow(image):
    """Statistical: libjpeg's integer DCT and colour conversion flip some near-tie coefficients,
    so the pixels of Pillow's own save(quality=75, subsampling=0) → load differ from J's on a
    few levels. Measured with this reference on the 64² image: mean |Δ| 1.03 of 255 levels (max
    13), while JPEG itself moves the image by 7.66 levels on average; asserted with a 2× margin."""
    Image = pytest.importorskip("PIL.Image")
    p = jpeg_ref.pixels(image)[0].permute(1, 2, 0).to(torch.uint8).numpy()
    buf = io.BytesIO()
    Image.fromarray(p).save(buf, "JPEG", quality=75, subsampling=0)
    back = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB")).astype(np.float64)
    y, _ = jpeg_ref.roundtrip32(image, qtab(75))
    ours = ((y[0].double() + 1.0) * 127.5).permute(1, 2, 0).numpy()
    d = np.abs(ours - back)
    moved = np.abs(back - p.astype(np.float64)).mean()
    print(f"jpeg vs Pillow q=75: mean |delta| {d.mean():.3f} levels, max {d.max():.0f}; "
          f"JPEG itself moves the image by {moved:.2f} levels on average")
    assert d.mean() <= 2 * 1.03
    assert moved > 2 * d.mean()


def test_jpeg_validation_before_any_device_work():
    from gfa_amd import attack, fgsm, jpeg_compress
    from gfa_amd import pgd
    x = torch.zeros(2, 3, 32, 32)
    t = torch.zeros(1, 3, 32, 32)
    net = _StubNet()
    kw = dict(target=t)
    for bad in (0, 101, -1, 75.0, True, np.bool_(True), "75", [75]):
        with pytest.raises(ValueError, match="jpeg_quality must be"):
            attack(net, x, 8 / 255, 4, jpeg_quality=bad, **kw)
        with pytest.raises(ValueError, match="jpeg_quality must be"):
            pgd._check_jpeg_quality(bad)
    assert pgd._check_jpeg_quality(np.int64(1)) == 1 and pgd._check_jpeg_quality(100) == 100
    for bad in ("linear", "STE", None, 1, True):
        with pytest.raises(ValueError, match="jpeg_grad must be one of"):
            attack(net, x, 8 / 255, 4, jpeg_quality=75, jpeg_grad=bad, **kw)
        with pytest.raises(ValueError, match="jpeg_grad must be one of"):
            pgd._check_jpeg_grad(bad)
    assert pgd._check_jpeg_grad("ste") == "ste" and pgd.JPEG_GRADS == ("cubic", "ste")
    with pytest.raises(ValueError, match="jpeg_grad needs jpeg_quality"):
        attack(net, x, 8 / 255, 4, jpeg_grad="ste", **kw)
    for norm in ("adam", "l2_cw"):
        with pytest.raises(ValueError, match="jpeg_quality.*norm='linf' and 'l2' only"):
            attack(net, x, None, 4, norm=norm, jpeg_quality=75, **kw)
    for other, word in ((dict(apgd=True), "apgd"), (dict(universal=True), "universal"),
                        (dict(sign_hunter=True), "sign_hunter"),
                        (dict(spsa_samples=4), "spsa_samples")):
        with pytest.raises(ValueError, match=word + ".*does not combine with.*jpeg_quality"):
            attack(net, x, 8 / 255, 4, jpeg_quality=75, **other, **kw)
    with pytest.raises(ValueError, match="fgsm\\(\\) takes no jpeg_quality"):
        fgsm(net, x, 8 / 255, jpeg_quality=75, **kw)

    class Odd(_StubNet):
        pass
    odd = Odd()
    odd.decoder = type("D", (), {"size": 20})()
    with pytest.raises(ValueError, match="multiple of 8"):
        attack(odd, torch.zeros(1, 3, 20, 20), 8 / 255, 4, jpeg_quality=75,
               target=torch.zeros(1, 3, 20, 20))
    # valid arguments get as far as the network bundle, which a stub is not
    sched = torch.tensor([[30, 1, 1, 1]] * 4)
    for extra in (dict(jpeg_quality=75), dict(jpeg_quality=np.int64(1), jpeg_grad="ste"),
                  dict(jpeg_quality=100, momentum=1.0, nesterov=True),
                  dict(jpeg_quality=75, ti_kernel=5, di_prob=0.5),
                  dict(jpeg_quality=75, si_scales=3), dict(jpeg_quality=75, di_schedule=sched),
                  dict(jpeg_quality=75, vt_samples=2), dict(jpeg_quality=75, pi_amplification=10.0),
                  dict(jpeg_quality=75, random_start=True),
                  dict(jpeg_quality=None), dict(jpeg_quality=None, jpeg_grad="cubic")):
        with pytest.raises(ValueError, match="device network"):
            attack(net, x, 8 / 255, 4, **extra, **kw)
    with pytest.raises(ValueError, match="device network"):
        attack(net, x, 1.0, 4, norm="l2", alpha=0.2, jpeg_quality=75, **kw)
    # the evaluation helper is device only
    with pytest.raises(ValueError, match="GPU only"):
        jpeg_compress(x, 75)
    with pytest.raises(ValueError, match="N,3,S,S"):
        jpeg_compress(torch.zeros(3, 32, 32), 75)


def test_runners_outside_the_chain_refuse_the_stage():
    """While set_jpeg() is on, the runs attack() rejects together with jpeg_quality raise before
    any device work instead of ignoring the stage or composing with it untested."""
    from gfa_amd import pgd
    eng = object.__new__(pgd.AttackEngine)
    eng.jp = (torch.ones(2, 64), "cubic")
    z = torch.zeros(1, 3, 32, 32)
    for name, args in (("run", (z, z, 1, 0.1, 0.01)), ("run_adam", (z, z, 1)),
                       ("run_cw", (z, z, 1)), ("run_spsa", (z, z, 1, 0.1, 0.01)),
                       ("run_universal", (z, z, 1, 0.1, 0.01)), ("run_apgd", (z, z, 1, 0.1)),
                       ("run_sign_hunter", (z, z, 1, 0.1)), ("run_patch", (z, z, z, z, 1))):
        with pytest.raises(ValueError, match=name + " does not combine with the JPEG stage"):
            getattr(eng, name)(*args)
