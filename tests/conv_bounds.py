"""Element-wise fp64 references and PROVEN error bounds for the 2-byte (fp16 / bf16) conv kernels.

A case is a convolution on operands already rounded to T followed by the epilogue of
csrc/conv_common.h conv_epilogue (= csrc/halo_epilogue.h halo_epilogue[_f], same operations in the
same order). `conv_ref_bound` returns, as fp64 CPU tensors, the reference of every output element
and of every fused sum, and a bound on |kernel − reference| that holds for ANY kernel that

  * feeds the MFMAs the operands the case names (products of two T values are exact in fp32),
  * accumulates and runs the epilogue in fp32, in any order, with or without FMA contraction,
  * rounds once to T on the store.

Nothing here is measured: every term names the rounding it covers, there are no empirical
multipliers, and the assertion a test makes is `(err <= bound).all()`.

    E     = (K + n_epi) · 2⁻²⁴ · A          the fp32 work before the store
    bound = E + u_T · max(|ref| + E, tiny_T)  + the one rounding to T of the store

(terms: `accum_term`, `store_term`; sums: `sum_term`.) The standard first-order bound of a sum of
exact products carried through n roundings is n·u·Σ|terms| (Higham, Accuracy and Stability of
Numerical Algorithms, §3.1, with γ_n ≈ n·u at n·u ≈ 4e-5); A is that Σ|terms|, the same computation
on absolute values.

Constants the kernels hold in fp32 (0.2f, √2 as float, noise_w, tap_coef, the bab inverse slopes)
enter the reference as those fp32 values, so no term is needed for them.
"""
import math
from dataclasses import dataclass, field

import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24  # unit roundoff of fp32 (round to nearest)
ACT_NONE, ACT_RELU, ACT_LRELU_S2, ACT_PRELU = 0, 1, 2, 3  # include/miattack.h MIA_ACT_*


def f32c(v):
    """A host constant as the kernels hold it: rounded to fp32 (mia_conv_args float fields)."""
    return float(np.float32(v))


SQRT2_F = f32c(1.41421356237309504880)  # csrc/mia_common.h SQRT2
SLOPE_F = f32c(0.2)                     # csrc/mia_common.h lrelu_s2: 0.2f
INV_POS_F = f32c(0.70710678118654752)   # csrc/mia_common.h lrelu_s2_inv_grad
INV_NEG_F = f32c(3.5355339059327376)
GRAD_NEG_F = f32c(SLOPE_F * SQRT2_F)       # lrelu_s2_grad: 0.2f * SQRT2, one fp32 product


def unit_roundoff(dtype):
    """u_T of the one rounding to T on the store (store4 / store8 / the WIDE path's (T)vo casts in
    csrc/halo_epilogue.h, csrc/conv_common.h): 2⁻¹¹ for fp16, 2⁻⁸ for bf16."""
    return {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}[dtype]


def tiny(dtype):
    """Smallest normal of T: below it the store's rounding error is absolute, ≤ u_T · tiny_T."""
    return torch.finfo(dtype).tiny


def accum_term(K, n_epi, A):
    """E = (K + n_epi)·2⁻²⁴·A: the K fp32 additions of the MFMA accumulation (csrc/conv_common.h
    mfma_chunk: exact products, fp32 accumulator, any order) and the n_epi fp32 operations of the
    epilogue between the accumulator and the store (csrc/halo_epilogue.h halo_epilogue_f)."""
    return (K + n_epi) * U32 * A


def store_term(ref, E, dtype):
    """u_T·max(|ref| + E, tiny_T): the rounding to T of the fp32 value v on the store; |v| ≤ |ref| + E."""
    return unit_roundoff(dtype) * torch.clamp(ref.abs() + E, min=tiny(dtype))


def sum_term(n_terms, K, n_epi, abs_terms_sum):
    """(n_terms + K + n_epi)·2⁻²⁴·Σ|terms|: a fused per-(image, channel) sum (sdot, bab_q, csum) is
    an fp32 sum over the image's pixels of fp32 values that each went through K + n_epi roundings
    (csrc/halo_epilogue.h part / partq / pcs, row16_sum, red_put; csrc/reduce.hip red_finish adds
    the slots in fp32). The sums take the fp32 value, NOT the value rounded to T, in conv_epilogue,
    halo_epilogue and halo_epilogue_f alike, so no u_T term enters."""
    return (n_terms + K + n_epi) * U32 * abs_terms_sum


def pre_round_term(ref_acc, E_acc, dtype):
    """u_T·max(|acc| + E_acc, tiny_T): the EXTRA rounding to T of the fp32 accumulator in
    csrc/conv_upconv.hip upconv_halo_kernel's 2-byte epilogue (`(T)acc[ph][i][j][…]` before
    permlane16_swap), which in DG mode with mask_a / accumulate is converted back to fp32, masked,
    accumulated and rounded a second time by `v[e] = (T)f[e]`. The mask's slope scales it."""
    return unit_roundoff(dtype) * torch.clamp(ref_acc.abs() + E_acc, min=tiny(dtype))


def rounded_sum_term(abs_terms_sum, dtype):
    """u_T·Σ|terms|: only for a kernel whose sum takes the value already rounded to T."""
    return unit_roundoff(dtype) * abs_terms_sum


def q(t, dtype):
    """Round an fp32 / fp64 tensor to T (round to nearest even, as the device casts do)."""
    return t.to(dtype)


def modulate(x, s, lrelu, dtype):
    """x̃ = act(x)·s as csrc/conv_common.h modulate<T> rounds it, x a T tensor (N, C, H, W), s the
    fp32 style (N, C) or None. The table entry is T(s·√2) for a leaky-ReLU input, T(s) otherwise
    (csrc/conv_mfma.hip stab, same in conv_halo / conv_wres / conv_thin / conv_upconv).
    fp16: packed half arithmetic, max(v, v·0.2h) then v·s, each product rounded once to half (what
    torch's CPU half multiply does: the fp32 product of two halves is exact, rounded once).
    bf16: via fp32: f = max(f, 0.2f·f), then T(f·s) (fp32 product, then the rounding to bf16)."""
    N, C = x.shape[:2]
    sv = torch.ones(N, C) if s is None else s.float()
    if lrelu:
        sv = sv * torch.tensor(SQRT2_F, dtype=torch.float32)
    st = sv.to(dtype).view(N, C, 1, 1)
    if dtype == torch.float16:
        v = x
        if lrelu:
            v = torch.maximum(v, v * torch.tensor(0.2, dtype=torch.float32).to(dtype))
        return v * st
    f = x.float()
    if lrelu:
        f = torch.maximum(f, torch.tensor(SLOPE_F, dtype=torch.float32) * f)
    return (f * st.float()).to(dtype)


def modulate_weights(w, s, d, dtype):
    """Per-image weights as csrc/conv_halo.hip modulate_weights_kernel rounds them:
    T(float(w)·s[n][ci]·d[n][co]), two fp32 products in that order. w (Cout, Cin, kh, kw) of T."""
    N = s.shape[0]
    wf = w.float().unsqueeze(0) * s.float().view(N, 1, -1, 1, 1)
    if d is not None:
        wf = wf * d.float().view(N, -1, 1, 1, 1)
    return wf.to(dtype)


def conv3x3(stride=1, pad=1):
    """The linear map of a case: x (N, Cin, H, W), w (Cout, Cin, kh, kw) or per image (N, Cout, …)."""
    def run(x, w):
        if w.dim() == 5:
            return torch.cat([F.conv2d(x[n:n + 1], w[n], stride=stride, padding=pad)
                              for n in range(x.shape[0])])
        return F.conv2d(x, w, stride=stride, padding=pad)
    return run


def upconv():
    """mia_upconv_fwd: conv_transpose2d(stride 2), x (N, Cin, R, R), w (Cout, Cin, 3, 3) →
    (N, Cout, 2R+1, 2R+1): T[2m+p] = Σ_j x[m−j]·W[p+2j] (layouts.upconv_subpixel_matrices and
    layouts.upconv_halo_matrix hold exactly w's values rounded to T, rearranged)."""
    return lambda x, w: F.conv_transpose2d(x, w.transpose(0, 1), stride=2)


def upconv_dgrad():
    """mia_upconv_dgrad: its adjoint, gx[i] = Σ_k gT[2i+k]·W[k]: a stride-2 3×3 conv without
    padding over gT (N, Cout, 2R+1, 2R+1) with w (Cout, Cin, 3, 3) channel-transposed."""
    return lambda g, w: F.conv2d(g, w.transpose(0, 1), stride=2)


def s2_dgrad():
    """mia_conv_s2_dgrad_halo: the input gradient of a stride-2, pad-1 3×3 conv w (Cg, Cx, 3, 3):
    g (N, Cg, R, R) → (N, Cx, 2R, 2R)."""
    return lambda g, w: F.conv_transpose2d(g, w, stride=2, padding=1, output_padding=1)


def phase_taps(size, two_tap_parity, cin):
    """K per output element of a sub-pixel conv: along each axis the outputs of parity
    `two_tap_parity` sum two taps and the others one (up-conv: T[2m] = x[m]·W[0] + x[m−1]·W[2],
    T[2m+1] = x[m]·W[1]; stride-2 gradient: gin[2i] = g[i]·W[1], gin[2i+1] = g[i]·W[2] + g[i+1]·W[0]);
    K = taps_y·taps_x·Cin. Products with the zero slots of a packed K-step add exact zeros."""
    t = torch.where(torch.arange(size) % 2 == two_tap_parity, 2.0, 1.0).double()
    return (t.view(-1, 1) * t.view(1, -1) * cin).view(1, 1, size, size)


@dataclass
class Epilogue:
    """mia_conv_args' epilogue fields, NCHW CPU tensors (T tensors for the per-pixel operands the
    kernels read as T: aux_x, tap_a, tap_t, mask_a, y0; fp32 for the rest)."""
    out_scale: torch.Tensor = None   # (N, Cout) fp32
    noise: torch.Tensor = None       # (H·W) fp32
    noise_w: float = 0.0
    bias: torch.Tensor = None        # (Cout) fp32
    tap_a: torch.Tensor = None
    tap_t: torch.Tensor = None
    tap_coef: float = 0.0
    mask_a: torch.Tensor = None
    mask_slope: torch.Tensor = None  # (Cout) fp32 or None (the mask zeroes)
    act_out: int = ACT_NONE
    act_slope: torch.Tensor = None   # (Cout) fp32, ACT_PRELU
    y0: torch.Tensor = None          # accumulate: the old output, T
    aux_x: torch.Tensor = None       # sdot / bab: the stored activation, T
    sdot: bool = False
    act_aux: int = ACT_NONE
    bab: dict = None                 # demod (N, Cout), noise (H·W) or None, noise_w, bias or None
    csum: bool = False
    # the accumulator is rounded to T BEFORE the mask / accumulate and again on the store: the
    # 2-byte stride-2 input-gradient epilogue of csrc/conv_upconv.hip upconv_halo_kernel (DG with
    # mask_a or accumulate), which repacks (T)acc first and works on those values
    pre_round: bool = False


@dataclass
class Bounded:
    ref: torch.Tensor
    bound: torch.Tensor
    sums: dict = field(default_factory=dict)  # name → (ref (N, Cout), bound (N, Cout))


def _act(v, act):
    if act == ACT_RELU:
        return v.clamp_min(0)
    if act == ACT_LRELU_S2:
        return torch.where(v > 0, v, SLOPE_F * v) * SQRT2_F
    return v


def conv_ref_bound(x, w, dtype, K, epi=None, conv=None):
    """(ref, bound) of y and of every fused sum of one case.

    x, w: the operands the MFMAs consume, values of T (any float dtype; see `modulate`,
    `modulate_weights`); K = taps·Cin, the length of one accumulation; `conv`: the linear map
    (default: 3×3, stride 1, pad 1).

    n_epi counts one fp32 operation per line of halo_epilogue_f that the case's features enable:
    out_scale 1 (v·osc), noise 2 (noise_w·noise, +), bias 1, tap 3 (a − t, ·coef, +), mask 1
    (msl·v), leaky ReLU 2 (0.2·v, ·√2), PReLU 1, accumulate 1, bab 2 (v·gr, gp·dm).
    K may be a tensor broadcastable to y where the accumulation length differs by output element
    (the sub-pixel phases of the up-conv and of the stride-2 input gradient: `phase_taps`)."""
    epi = epi or Epilogue()
    conv = conv or conv3x3()
    d = torch.float64
    x, w = x.to(d), w.to(d)
    v = conv(x, w)
    A = conv(x.abs(), w.abs())
    N, C, H, W = v.shape
    n = 0
    sums = {}
    X = torch.zeros((), dtype=d)  # absolute error of roundings other than the fp32 ones and the store
    if epi.pre_round:
        assert not (epi.sdot or epi.bab or epi.csum or epi.out_scale is not None
                    or epi.noise is not None or epi.bias is not None or epi.tap_a is not None
                    or epi.act_out != ACT_NONE), "pre_round: the mask / accumulate epilogue only"
        X = pre_round_term(v, accum_term(K, 0, A), dtype)

    def chan(t):
        return t.to(d).view(1, C, 1, 1)

    def per_image(t):
        return t.to(d).view(N, C, 1, 1)

    def plane(t):
        return t.to(d).view(1, 1, H, W)

    if epi.sdot:
        # sdot takes the fp32 accumulator before out_scale (halo_epilogue_f: part += v·xv)
        ax = epi.aux_x.to(d)
        n_aux = 1
        if epi.act_aux == ACT_LRELU_S2:
            ax, n_aux = _act(ax, ACT_LRELU_S2), 3
        elif epi.act_aux == ACT_RELU:
            ax = _act(ax, ACT_RELU)
        sums["sdot"] = ((v * ax).sum((2, 3)),
                        sum_term(H * W, K, n_aux, (A * ax.abs()).sum((2, 3))))
    if epi.out_scale is not None:
        v, A, n = v * per_image(epi.out_scale), A * per_image(epi.out_scale).abs(), n + 1
    if epi.noise is not None:
        nz = f32c(epi.noise_w) * plane(epi.noise)
        v, A, n = v + nz, A + nz.abs(), n + 2
    if epi.bias is not None:
        v, A, n = v + chan(epi.bias), A + chan(epi.bias).abs(), n + 1
    if epi.tap_a is not None:
        ta, tt, c = epi.tap_a.to(d), epi.tap_t.to(d), f32c(epi.tap_coef)
        v, A, n = v + c * (ta - tt), A + abs(c) * (ta.abs() + tt.abs()), n + 3
    if epi.mask_a is not None:
        keep = epi.mask_a.to(d) > 0  # decided on a stored T value: no rounding can flip it
        if epi.mask_slope is not None:
            sl = chan(epi.mask_slope)
            v, A, n = torch.where(keep, v, sl * v), torch.where(keep, A, sl.abs() * A), n + 1
            X = torch.where(keep, X, sl.abs() * X)
        else:
            zero = torch.zeros((), dtype=d)
            v, A, X = torch.where(keep, v, zero), torch.where(keep, A, zero), torch.where(keep, X, zero)
    # activations are piecewise linear and continuous: a sign the fp32 value decides differently
    # from the reference moves the result by at most L·(the error already bounded), L their
    # largest slope; A carries L
    if epi.act_out == ACT_PRELU:
        sl = chan(epi.act_slope)
        v, A, n = torch.where(v > 0, v, sl * v), A * sl.abs().clamp_min(1.0), n + 1
    elif epi.act_out == ACT_LRELU_S2:
        v, A, n = _act(v, ACT_LRELU_S2), A * SQRT2_F, n + 2
    elif epi.act_out == ACT_RELU:
        v = _act(v, ACT_RELU)
    if epi.y0 is not None:
        v, A, n = v + epi.y0.to(d), A + epi.y0.to(d).abs(), n + 1
    if epi.bab is not None:
        b = epi.bab
        xv = epi.aux_x.to(d)
        pos = xv > 0  # on the stored activation: exact
        gr = torch.where(pos, torch.tensor(SQRT2_F, dtype=d), torch.tensor(GRAD_NEG_F, dtype=d))
        inv = torch.where(pos, torch.tensor(INV_POS_F, dtype=d), torch.tensor(INV_NEG_F, dtype=d))
        bnz = f32c(b.get("noise_w", 0.0)) * plane(b["noise"]) if b.get("noise") is not None else 0.0
        bb = chan(b["bias"]) if b.get("bias") is not None else 0.0
        gp, Agp = v * gr, A * gr
        inner = xv * inv - bnz - bb
        inner_abs = xv.abs() * inv + abs(bnz) + abs(bb)
        # q: gp·(xv·inv − bnz − bb): v's n roundings + v·gr + (·, −, −, noise_w·noise) + the product
        sums["bab_q"] = ((gp * inner).sum((2, 3)),
                         sum_term(H * W, K, n + 6, (Agp * inner_abs).sum((2, 3))))
        dm = per_image(b["demod"])
        v, A, n = gp * dm, Agp * dm.abs(), n + 2
    if epi.csum:
        # csum takes the fp32 value before the store's rounding (halo_epilogue_f: pcs += v)
        sums["csum"] = (v.sum((2, 3)), sum_term(H * W, K, n, A.sum((2, 3))))
    E = accum_term(K, n, A) + X
    return Bounded(v, E + store_term(v, E, dtype), sums)


def worst_ratio(got, ref, bound):
    """max over elements of err / bound (bound > 0 everywhere: it contains u_T·tiny_T)."""
    return ((got.double() - ref).abs() / bound).max().item()
