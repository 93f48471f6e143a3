"""Host test of tests/conv_bounds.py (no GPU): an emulated honest kernel (fp32 conv, fp32 epilogue,
one rounding to T) satisfies the element-wise bound everywhere, every injected fault fails it, and
every term of the bound is pinned to its closed form on hand cases — so the helper can be neither
loosened nor tightened without a test here failing."""
import math

import pytest
import torch
import torch.nn.functional as F

import conv_bounds as cb

DTYPES = [torch.float16, torch.bfloat16]


def _case(dtype, C, Co, N=2, H=16, W=16):
    """The 3×3 modulated-forward epilogue (out_scale, noise, bias, leaky ReLU·√2), seeded randn."""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, C, H, W, generator=g).to(dtype)
    w = (torch.randn(Co, C, 3, 3, generator=g) / math.sqrt(9 * C)).to(dtype)
    b = torch.randn(Co, generator=g) * 0.1
    nz = torch.randn(H * W, generator=g)
    d = torch.rand(N, Co, generator=g) + 0.5
    return x, w, b, nz, d


def _honest(conv32, d, nz, b, nw, dtype):
    """fp32 epilogue in the kernels' order on an fp32 conv result, one rounding to T."""
    N, Co, H, W = conv32.shape
    f = torch.float32
    v = conv32 * d.to(f).view(N, Co, 1, 1)
    v = v + torch.tensor(nw, dtype=f) * nz.to(f).view(1, 1, H, W)
    v = v + b.to(f).view(1, Co, 1, 1)
    v = torch.where(v > 0, v, torch.tensor(0.2, dtype=f) * v) * torch.tensor(cb.SQRT2_F, dtype=f)
    return v.to(dtype).double()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,Co", [(64, 64), (128, 128)])
def test_honest_kernel_within_bound_and_faults_outside(dtype, C, Co):
    N, H, W = 2, 16, 16
    x, w, b, nz, d = _case(dtype, C, Co)
    K = 9 * C
    epi = cb.Epilogue(out_scale=d, noise=nz, noise_w=0.3, bias=b, act_out=cb.ACT_LRELU_S2)
    r = cb.conv_ref_bound(x, w, dtype, K, epi)
    conv32 = F.conv2d(x.float(), w.float(), padding=1)

    def ratio(got):
        return cb.worst_ratio(got, r.ref, r.bound)

    honest = ratio(_honest(conv32, d, nz, b, 0.3, dtype))
    print(f"honest {dtype} {C}->{Co}: worst err/bound {honest:.3f}")
    assert honest <= 1.0
    # the bound is not slack: an honest kernel uses a good part of it
    assert honest > 0.25

    faults = {}
    faults["bias dropped"] = _honest(conv32, d, nz, torch.zeros(Co), 0.3, dtype)
    faults["noise weight 0.25"] = _honest(conv32, d, nz, b, 0.25, dtype)
    xf, wf = x.float(), w.float()
    c2 = conv32.clone()
    for yy, xx in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        dx = 1 if xx == 0 else -1  # the in-range horizontal neighbour tap of the corner pixel
        c2[:, :, yy, xx] -= torch.einsum("nc,oc->no", xf[:, :, yy, xx + dx], wf[:, :, 1, 1 + dx])
    faults["corner pixels miss one tap"] = _honest(c2, d, nz, b, 0.3, dtype)
    c3 = conv32.clone()
    xp = F.pad(xf, (1, 1, 1, 1))
    c3[:, 5] -= torch.einsum("nchw,c->nhw", xp[:, -8:, 2:2 + H, 2:2 + W], wf[5, -8:, 2, 2])
    faults["one channel misses its last 8 K terms"] = _honest(c3, d, nz, b, 0.3, dtype)
    c4 = conv32.clone()
    c4[1, :, 7, 9] = conv32[0, :, 7, 9]
    faults["one pixel reads the other image"] = _honest(c4, d, nz, b, 0.3, dtype)
    for name, got in faults.items():
        rr = ratio(got)
        print(f"  {name}: worst err/bound {rr:.1f}")
        assert rr > 10.0, name
        assert not ((got - r.ref).abs() <= r.bound).all(), name


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,Co", [(64, 64), (128, 128)])
def test_honest_sdot_within_bound_and_missing_segment_outside(dtype, C, Co):
    """The input-gradient form: y = conv·out_scale, sdot = Σ_p conv·aux on the fp32 accumulator."""
    N, H, W = 2, 16, 16
    x, w, _, _, d = _case(dtype, C, Co)
    g = torch.Generator().manual_seed(2)
    aux = torch.randn(N, Co, H, W, generator=g).to(dtype)
    r = cb.conv_ref_bound(x, w, dtype, 9 * C, cb.Epilogue(out_scale=d, aux_x=aux, sdot=True))
    ref, bound = r.sums["sdot"]
    conv32 = F.conv2d(x.float(), w.float(), padding=1)
    terms = conv32 * aux.float()
    honest = terms.sum((2, 3)).double()
    ratio = ((honest - ref).abs() / bound).max().item()
    print(f"honest sdot {dtype} {C}->{Co}: worst err/bound {ratio:.4f}")
    assert ((honest - ref).abs() <= bound).all()
    y = (conv32 * d.view(N, Co, 1, 1)).to(dtype).double()
    assert ((y - r.ref).abs() <= r.bound).all()
    t2 = terms.clone()
    t2[:, :, 3, 0:16] = 0  # one 16-pixel row segment never reaches the sum
    faulty = t2.sum((2, 3)).double()
    assert not ((faulty - ref).abs() <= bound).all()
    assert ((faulty - ref).abs() / bound).max().item() > 10.0
    # a sum formed from the outputs already rounded to T needs the extra u_T term, and only then
    rounded = (conv32.to(dtype).float() * aux.float()).sum((2, 3)).double()
    extra = cb.rounded_sum_term((F.conv2d(x.double().abs(), w.double().abs(), padding=1)
                                 * aux.double().abs()).sum((2, 3)), dtype)
    assert ((rounded - ref).abs() <= bound + extra).all()


def test_modulate_matches_the_kernels_rounding_order():
    """modulate<T> (csrc/conv_common.h) element by element: fp16 rounds v·0.2h and v·s to half each;
    bf16 goes through fp32 and rounds the fp32 product."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 8, 4, 4, generator=g)
    s = torch.rand(2, 8, generator=g) + 0.5
    h = torch.float16
    got = cb.modulate(x.to(h), s, True, h)
    sh = (s * torch.tensor(cb.SQRT2_F)).to(h).view(2, 8, 1, 1)
    xh = x.to(h)
    lo = (xh.double() * torch.tensor(0.2).to(h).double()).to(h)  # exact product, one rounding
    v = torch.maximum(xh, lo)
    assert torch.equal(got, (v.double() * sh.double()).to(h))
    b = torch.bfloat16
    got = cb.modulate(x.to(b), s, True, b)
    sb = (s * torch.tensor(cb.SQRT2_F)).to(b).view(2, 8, 1, 1)
    f = x.to(b).float()
    f = torch.maximum(f, torch.tensor(cb.SLOPE_F) * f)
    assert torch.equal(got, (f * sb.float()).to(b))
    # no activation, no style: the identity
    assert torch.equal(cb.modulate(x.to(b), None, False, b), x.to(b))


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_term_is_pinned_to_its_closed_form(dtype):
    """A 1×1 image, one input channel, a 3×3 window whose centre tap alone is in range: every term
    of the bound by hand. A term edited to be 4× smaller or larger fails here."""
    u, tiny = {torch.float16: (2.0 ** -11, 2.0 ** -14), torch.bfloat16: (2.0 ** -8, 2.0 ** -126)}[dtype]
    x = torch.tensor([[[[1.5]]]])
    w = torch.zeros(1, 1, 3, 3)
    w[0, 0, 1, 1] = -2.0
    K = 9
    # plain: ref = −3, A = 3, no epilogue operation
    r = cb.conv_ref_bound(x, w, dtype, K)
    E = 9 * 2.0 ** -24 * 3.0
    assert r.ref.item() == -3.0
    assert r.bound.item() == pytest.approx(E + u * (3.0 + E), rel=1e-12)
    # out_scale 0.5, bias −0.25, accumulate onto 4: ref = −1.5 − 0.25 + 4, A = 1.5 + 0.25 + 4, n_epi = 3
    epi = cb.Epilogue(out_scale=torch.tensor([[0.5]]), bias=torch.tensor([-0.25]),
                      y0=torch.tensor([[[[4.0]]]]))
    r = cb.conv_ref_bound(x, w, dtype, K, epi)
    E = (9 + 3) * 2.0 ** -24 * 5.75
    assert r.ref.item() == 2.25
    assert r.bound.item() == pytest.approx(E + u * (2.25 + E), rel=1e-12)
    # leaky ReLU·√2 on a negative value, noise: n_epi = 2 + 2
    epi = cb.Epilogue(noise=torch.tensor([1.0]), noise_w=0.5, act_out=cb.ACT_LRELU_S2)
    r = cb.conv_ref_bound(x, w, dtype, K, epi)
    E = (9 + 4) * 2.0 ** -24 * 3.5 * cb.SQRT2_F
    assert r.ref.item() == pytest.approx(-2.5 * cb.SLOPE_F * cb.SQRT2_F, rel=1e-15)
    assert r.bound.item() == pytest.approx(E + u * (abs(r.ref.item()) + E), rel=1e-12)
    # a zero result: the floor u_T·tiny_T alone
    r = cb.conv_ref_bound(x, torch.zeros(1, 1, 3, 3), dtype, K)
    assert r.ref.item() == 0.0 and r.bound.item() == u * tiny
    # the sums: sdot on the accumulator (one product), csum on the final value
    aux = torch.tensor([[[[0.5]]]])
    epi = cb.Epilogue(out_scale=torch.tensor([[0.5]]), aux_x=aux, sdot=True, csum=True)
    r = cb.conv_ref_bound(x, w, dtype, K, epi)
    assert r.sums["sdot"][0].item() == -1.5
    assert r.sums["sdot"][1].item() == pytest.approx((1 + 9 + 1) * 2.0 ** -24 * 1.5, rel=1e-12)
    assert r.sums["csum"][0].item() == -1.5
    assert r.sums["csum"][1].item() == pytest.approx((1 + 9 + 1) * 2.0 ** -24 * 1.5, rel=1e-12)
    assert cb.rounded_sum_term(torch.tensor(2.0), dtype).item() == 2.0 * u
    # the fused backward front on a positive stored activation a = 0.5: gr = √2, inv = 1/√2
    epi = cb.Epilogue(out_scale=torch.tensor([[0.5]]), aux_x=aux, sdot=True,
                      bab=dict(demod=torch.tensor([[2.0]]), noise=torch.tensor([1.0]), noise_w=0.25,
                               bias=torch.tensor([0.125])))
    r = cb.conv_ref_bound(x, w, dtype, K, epi)
    gp = -1.5 * cb.SQRT2_F
    assert r.ref.item() == pytest.approx(gp * 2.0, rel=1e-15)
    E = (9 + 3) * 2.0 ** -24 * abs(gp) * 2.0
    assert r.bound.item() == pytest.approx(E + u * (abs(gp) * 2.0 + E), rel=1e-12)
    inner = 0.5 * cb.INV_POS_F - 0.25 - 0.125
    inner_abs = 0.5 * cb.INV_POS_F + 0.25 + 0.125
    assert r.sums["bab_q"][0].item() == pytest.approx(gp * inner, rel=1e-15)
    assert r.sums["bab_q"][1].item() == pytest.approx((1 + 9 + 1 + 6) * 2.0 ** -24 * abs(gp) * inner_abs,
                                                      rel=1e-12)


def test_last_conv_path_is_empty_before_any_launch():
    """mia_last_conv_path (include/miattack.h): a static string, "" while no conv has been launched
    on this thread (host-only: nothing is launched here)."""
    import threading

    from gfa_amd import ops
    seen = []
    t = threading.Thread(target=lambda: seen.append(ops.last_conv_path()))
    t.start()
    t.join()
    assert seen == [""]


@pytest.mark.parametrize("dtype", DTYPES)
def test_pre_round_term_and_phase_taps_are_pinned(dtype):
    """The extra rounding of the 2-byte stride-2 input-gradient epilogue (csrc/conv_upconv.hip: the
    accumulator is rounded to T before the mask / accumulate and again on the store) and the
    per-element K of the sub-pixel phases, by hand."""
    u = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}[dtype]
    x = torch.tensor([[[[1.5]]]])
    w = torch.zeros(1, 1, 3, 3)
    w[0, 0, 1, 1] = -2.0
    m = torch.tensor([[[[-1.0]]]])  # masked: the slope 0.5 applies
    epi = cb.Epilogue(mask_a=m, mask_slope=torch.tensor([0.5]), y0=torch.tensor([[[[4.0]]]]),
                      pre_round=True)
    r = cb.conv_ref_bound(x, w, dtype, 9, epi)
    assert r.ref.item() == 2.5
    e_acc = 9 * 2.0 ** -24 * 3.0
    extra = 0.5 * u * (3.0 + e_acc)
    E = (9 + 2) * 2.0 ** -24 * 5.5 + extra
    assert r.bound.item() == pytest.approx(E + u * (2.5 + E), rel=1e-12)
    # an honest double rounding needs the term: emulate on a whole map
    g = torch.Generator().manual_seed(5)
    xg = torch.randn(2, 64, 8, 8, generator=g).to(dtype)
    wg = (torch.randn(64, 64, 3, 3, generator=g) / 24).to(dtype)
    y0 = torch.randn(2, 64, 16, 16, generator=g).to(dtype)
    K = cb.phase_taps(16, 1, 64)
    conv32 = cb.s2_dgrad()(xg.float(), wg.float())
    got = (conv32.to(dtype).float() + y0.float()).to(dtype).double()
    with_term = cb.conv_ref_bound(xg, wg, dtype, K, cb.Epilogue(y0=y0, pre_round=True), cb.s2_dgrad())
    without = cb.conv_ref_bound(xg, wg, dtype, K, cb.Epilogue(y0=y0), cb.s2_dgrad())
    assert ((got - with_term.ref).abs() <= with_term.bound).all()
    assert not ((got - without.ref).abs() <= without.bound).all()
    k = cb.phase_taps(5, 0, 64)
    assert k.shape == (1, 1, 5, 5)
    assert k[0, 0, 0].tolist() == [256.0, 128.0, 256.0, 128.0, 256.0]
    assert k[0, 0, 1].tolist() == [128.0, 64.0, 128.0, 64.0, 128.0]


def test_upconv_maps_are_adjoint_and_match_the_packed_weights():
    """upconv / upconv_dgrad are each other's adjoint, and the sub-pixel phase matrices the device
    gets (layouts.upconv_subpixel_matrices) are w's own values: phase (1, 1) is the centre tap."""
    from gfa_amd import layouts
    g = torch.Generator().manual_seed(6)
    x = torch.randn(1, 8, 4, 4, generator=g, dtype=torch.float64)
    w = torch.randn(16, 8, 3, 3, generator=g, dtype=torch.float64)
    t = cb.upconv()(x, w)
    assert t.shape == (1, 16, 9, 9)
    gt = torch.randn(t.shape, generator=g, dtype=torch.float64)
    assert torch.allclose((t * gt).sum(), (x * cb.upconv_dgrad()(gt, w)).sum(), rtol=1e-12)
    ph3 = layouts.upconv_subpixel_matrices(w, torch.float16)[3]
    assert torch.equal(ph3[:, :8], w[:, :, 1, 1].to(torch.float16))
    assert torch.allclose(t[0, :, 1::2, 1::2], torch.einsum("oc,chw->ohw", w[:, :, 1, 1], x[0]))
