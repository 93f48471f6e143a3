"""Element-wise fp64 error bounds for the kernels that exist only for fp16 / bf16 (GPU).

One table row per dispatch target. Every case first asserts, by name, the kernel family the launch
dispatched to (ops.last_conv_path), then `(err <= bound).all()` over EVERY output element and
every fused sum, with the reference and the proven bound of tests/conv_bounds.py (operands rounded
as the kernel rounds them, exact products, fp32 accumulation in any order, one rounding on the
store; no tolerance, no share of elements exempt). Each case prints its worst err / bound:
profiles/conv_elementwise_bounds.txt summarises that output of one run by path, dtype and mask.

Every stride-1 launch is a forward 3×3 window conv on random weights: an input-gradient launch differs
from it only in the weight matrix the host packs, so the feature masks of the gradient launches
(sdot, bab, tap, mask, accumulate) are exercised on the same kernels with the same arithmetic.
"""
import functools
import math
import zlib

import pytest
import torch

import conv_bounds as cb
from gfa_amd import layouts, ops

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
ALL_OFF = {"MIA_CONV_HALO": 0, "MIA_CONV_WRES": 0, "MIA_CONV_WRES128": 0, "MIA_CONV_WRES32": 0,
           "MIA_CONV_THIN32": 0, "MIA_CONV_THIN": 0}

# masks that mia_conv3x3 cannot express (PReLU, mask slope, channel sum) go through mia_conv2d;
# both reach the same dispatch (csrc/conv_mfma.hip run_conv) with the same problem description
VIA_CONV2D = {"prelu", "bias_prelu", "bias_csum", "csum", "mask_slope", "mask_slope_acc"}


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def build(dtype, N, H, W, Cin, Cout, mask, stride=1):
    """Operands (CPU, rounded to T), the epilogue and (ref, bound) of one case; cached, so the
    variants of one case (epilogue forms, tiles) share one fp64 reference and never modify it."""
    g = torch.Generator().manual_seed(zlib.crc32(repr((N, H, W, Cin, Cout, mask, stride)).encode()))
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = torch.randn(N, Cin, H, W, generator=g).to(dtype)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)).to(dtype)
    f = {}  # the random operands a mask may use

    def out_like():
        return torch.randn(N, Cout, Ho, Wo, generator=g).to(dtype)
    f["bias"] = torch.randn(Cout, generator=g) * 0.1
    f["slope"] = torch.rand(Cout, generator=g) * 0.5 + 0.05
    f["s"] = torch.rand(N, Cin, generator=g) + 0.5
    f["d"] = torch.rand(N, Cout, generator=g) + 0.5
    f["nz"] = torch.randn(Ho * Wo, generator=g)
    f["y0"], f["aux"], f["m"], f["t"] = out_like(), out_like(), out_like(), out_like()
    f["a"] = out_like().relu()
    f["dm"] = torch.rand(N, Cout, generator=g) + 0.5
    f["bnz"] = torch.randn(Ho * Wo, generator=g)
    f["bb"] = torch.randn(Cout, generator=g) * 0.1
    e = cb.Epilogue()
    xe, we = x, w
    parts = set(mask.split("_")) if mask not in ("mod_lrelu_in", "mask_slope", "mask_slope_acc",
                                                 "tap_mask") else set()
    if mask in ("mod", "mod_lrelu_in"):
        xe = cb.modulate(x, f["s"], mask == "mod_lrelu_in", dtype)
        e.out_scale, e.noise, e.noise_w, e.bias = f["d"], f["nz"], 0.3, f["bias"]
        e.act_out = cb.ACT_LRELU_S2
    elif mask == "wmod":
        we = cb.modulate_weights(w, f["s"], f["d"], dtype)
        e.noise, e.noise_w, e.bias, e.act_out = f["nz"], 0.3, f["bias"], cb.ACT_LRELU_S2
    elif mask == "tap":
        e.tap_a, e.tap_t, e.tap_coef = f["a"], f["t"], 0.37
    elif mask == "tap_mask":
        e.tap_a, e.tap_t, e.tap_coef, e.mask_a = f["a"], f["t"], 0.37, f["a"]
    elif mask == "mask":
        e.mask_a = f["m"]
    elif mask in ("mask_slope", "mask_slope_acc"):
        e.mask_a, e.mask_slope = f["m"], f["slope"]
        if mask.endswith("acc"):
            e.y0 = f["y0"]
    else:
        if "bias" in parts:
            e.bias = f["bias"]
        if "relu" in parts:
            e.act_out = cb.ACT_RELU
        if "prelu" in parts:
            e.act_out, e.act_slope = cb.ACT_PRELU, f["slope"]
        if "csum" in parts:
            e.csum = True
        if "acc" in parts:
            e.y0 = f["y0"]
        if "sdot" in parts:
            e.out_scale, e.aux_x, e.sdot = f["d"], f["aux"], True
        if "bab" in parts:
            e.bab = dict(demod=f["dm"], noise=f["bnz"], noise_w=0.3, bias=f["bb"])
        assert parts <= {"plain", "bias", "relu", "prelu", "csum", "acc", "sdot", "bab"}, mask
    r = cb.conv_ref_bound(xe, we, dtype, 9 * Cin, e, cb.conv3x3(stride=stride))
    return x, w, f, e, r


def launch(dev, dtype, N, H, W, Cin, Cout, mask, stride=1):
    """Run one case on the device; returns y (N, Cout, Ho, Wo) and the sums, as CPU tensors."""
    x, w, f, e, _ = build(dtype, N, H, W, Cin, Cout, mask, stride)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1

    def dv(t):
        return None if t is None else (nhwc(t) if t.dim() == 4 else t).to(dev)
    xd, wd = dv(x), layouts.fwd_matrix(w, dtype).to(dev)
    y = dv(e.y0) if e.y0 is not None else torch.empty(N, Ho, Wo, Cout, dtype=dtype, device=dev)
    sums = {}
    if e.sdot:
        sums["sdot"] = torch.zeros(N, Cout, device=dev)
    if e.csum:
        sums["csum"] = torch.zeros(N, Cout, device=dev)
    if mask == "wmod":
        wm = torch.empty(N, Cout, wd.shape[1], dtype=dtype, device=dev)
        ops.conv3x3_modw(xd, wd, y, wm, cout=Cout, in_scale=f["s"].to(dev), out_scale=f["d"].to(dev),
                         bias=dv(e.bias), noise=dv(e.noise), noise_w=e.noise_w, act_out=e.act_out)
    elif mask in VIA_CONV2D or stride != 1:
        grp = [dict(w=wd, kh=3, kw=3, pad=(1, 1), ho=Ho, wo=Wo)]
        ops.conv2d(xd, grp, y, (Ho, Wo), cout=Cout, stride=stride, bias=dv(e.bias),
                   act_out=e.act_out, act_slope=dv(e.act_slope), mask_a=dv(e.mask_a),
                   mask_slope=dv(e.mask_slope), csum=sums.get("csum"),
                   accumulate=e.y0 is not None, out_scale=dv(e.out_scale))
    else:
        mod = mask in ("mod", "mod_lrelu_in")
        bab = None
        if e.bab is not None:
            sums["bab_q"] = torch.zeros(N, Cout, device=dev)
            bab = dict(demod=dv(e.bab["demod"]), noise=dv(e.bab["noise"]), noise_w=0.3,
                       bias=dv(e.bab["bias"]), q=sums["bab_q"])
        ta = dv(e.tap_a)
        ops.conv3x3(xd, wd, y, cout=Cout,
                    act_in=ops.ACT_LRELU_S2 if mask == "mod_lrelu_in" else ops.ACT_NONE,
                    in_scale=f["s"].to(dev) if mod else None, out_scale=dv(e.out_scale),
                    bias=dv(e.bias), noise=dv(e.noise), noise_w=e.noise_w, act_out=e.act_out,
                    aux_x=dv(e.aux_x), sdot=sums.get("sdot"), tap_a=ta, tap_t=dv(e.tap_t),
                    tap_coef=e.tap_coef, mask_a=ta if e.mask_a is e.tap_a else dv(e.mask_a),
                    accumulate=e.y0 is not None, bab=bab)
    path = ops.last_conv_path()
    torch.cuda.synchronize()
    return path, y.permute(0, 3, 1, 2).cpu(), {k: v.cpu() for k, v in sums.items()}


def verdict(want_path, path, dtype, what, y, sums, r):
    """The path by name, then every element of y and of every sum against its bound."""
    assert path == want_path, f"dispatched to {path}, the case is written for {want_path}"
    line = (f"BOUND {want_path:16s} {str(dtype).replace('torch.', ''):8s} {what} "
            f"y {cb.worst_ratio(y, r.ref, r.bound):.3f}")
    assert set(sums) == set(r.sums)
    for k in sorted(sums):
        line += f" {k} {cb.worst_ratio(sums[k], *r.sums[k]):.1e}"
    print(line, flush=True)
    assert ((y.double() - r.ref).abs() <= r.bound).all(), line
    for k, got in sums.items():
        ref, bound = r.sums[k]
        assert ((got.double() - ref).abs() <= bound).all(), line


def check(dev, tune, knobs, want_path, dtype, N, H, W, Cin, Cout, mask, stride=1):
    for name, value in knobs.items():
        tune(name, value)
    r = build(dtype, N, H, W, Cin, Cout, mask, stride)[4]
    path, y, sums = launch(dev, dtype, N, H, W, Cin, Cout, mask, stride)
    verdict(want_path, path, dtype, f"{Cin:3d}->{Cout:<3d} {N}x{H}x{W} s{stride} {mask:14s}", y, sums, r)


def cases(rows):
    """rows of (expected path, knobs, shapes, (Cin, Cout) pairs, masks) → pytest params."""
    out = []
    for path, knobs, shapes, chans, masks in rows:
        for (N, H, W) in shapes:
            for (ci, co) in chans:
                for m in masks:
                    kid = "".join(f"-{k[4:].lower()}{v}" for k, v in sorted(knobs.items())
                                  if k in ("MIA_HALO_EPI", "MIA_CONV_REGEPI", "MIA_CONV_SMALLTILE",
                                           "MIA_UPCONV_HALO"))
                    out.append(pytest.param(path, knobs, N, H, W, ci, co, m,
                                            id=f"{path}-{ci}-{co}-{N}x{H}x{W}-{m}{kid}"))
    return out


ARGS = "path,knobs,N,H,W,Cin,Cout,mask"

# ---- conv_wres.hip: the 64 → 64 weights-resident kernel (every mask of wres_mask_ok) -------------
WRES = cases([("wres/reg", {}, [(2, 16, 16), (2, 16, 32)], [(64, 64)],
               ["bias_relu", "tap_mask", "plain", "prelu", "bias_csum", "mask_slope", "acc", "bias"])])

# ---- the 32 → 32 layers: conv_wres.hip wres32 and conv_thin.hip conv_thin32_kernel ---------------
M32 = ["mod", "mod_lrelu_in", "sdot", "sdot_acc", "sdot_bab", "sdot_acc_bab", "plain", "acc"]
# 32×48: 96 sixteen-pixel groups per row block. The sums' two-level finish (csrc/reduce.hip
# RED_CHUNK: more than 128 slots) against fp64: wres32 has one slot per 16×16 patch (16×2064: 129
# patches), thin32 one per 64 sixteen-pixel groups (65×2032: 8255 groups, 129 slots)
WRES32 = cases([("wres32/reg", {}, [(3, 16, 16), (2, 32, 48)], [(32, 32)], M32),
                ("wres32/reg", {}, [(1, 16, 2064)], [(32, 32)], ["sdot_bab"])])
NO32 = {"MIA_CONV_WRES32": 0}
THIN32 = cases([("thin32/reg", NO32, [(3, 16, 16), (2, 32, 48), (2, 17, 16)], [(32, 32)], M32),
                ("thin32/reg", NO32, [(1, 65, 2032)], [(32, 32)], ["sdot_bab"])])

# ---- conv_wres128.hip: every (Cin, Cout) and mask conv_wres128_eligible accepts -----------------
S128 = [(1, 8, 16), (3, 40, 48)]
WRES128 = cases([("wres128/reg", {}, S128, [(128, 128)],
                  ["wmod", "sdot_bab", "bias_relu", "bias", "prelu", "mask", "mask_slope", "acc"]),
                 ("wres128/reg", {}, S128, [(64, 128), (64, 256), (128, 256)], ["bias_relu", "prelu"]),
                 ("wres128/reg", {}, S128, [(128, 64)], ["plain", "acc", "mask_slope"])])

# ---- conv_halo.hip, 2-byte: the halo tile (rolled) and its unrolled specialised form -------------
# MIA_HALO_EPI=1: the specialised unrolled form ("/reg") where the tile and the mask have one, else
# the rolled loop with the runtime-feature register epilogue ("/regrt"): TAP|MASK has none, and the
# 32-column tile (Cout = 8) has them only unmodulated at Cin = 64. MIA_HALO_EPI=0: the LDS-staged one.
HSH = [(2, 16, 16), (1, 32, 16)]
HBIG = [(ci, co) for ci in (64, 128) for co in (64, 128, 192)]
HMASKS = ["bias_relu", "mod", "sdot_bab", "tap_mask", "mask", "acc"]


def halo_knobs(epi):
    return {"MIA_CONV_WRES": 0, "MIA_CONV_WRES128": 0, "MIA_CONV_THIN": 0, "MIA_HALO_C64": 1,
            "MIA_HALO_EPI": epi}


HALO = cases([
    ("halo/reg", halo_knobs(1), HSH, HBIG, ["bias_relu", "mod", "sdot_bab", "mask", "acc"]),
    ("halo/regrt", halo_knobs(1), HSH, HBIG, ["tap_mask"]),
    ("halo/reg", halo_knobs(1), HSH, [(64, 8)], ["bias_relu", "sdot_bab", "mask", "acc"]),
    ("halo/regrt", halo_knobs(1), HSH, [(64, 8)], ["mod", "tap_mask"]),
    ("halo/regrt", halo_knobs(1), HSH, [(128, 8)], HMASKS),
    ("halo/lds", halo_knobs(0), HSH, HBIG + [(64, 8), (128, 8)], HMASKS)])

# ---- conv_mfma.hip: the generic tile, its 2-byte register epilogues and the 64×64 small tile -----
# Cout ≤ 64: the 128×64 tile; else the 64×64 tile below MIA_CONV_SMALLTILE 128×128 tiles (every
# shape here at the default 512), else 128×128. The register epilogue ("/reg"): MIA_CONV_REGEPI,
# whole 128-pixel tiles per image (16×16, not 17×18), an unmodulated launch with one of
# reg_epi_mask's masks, and on the 128×128 tile Cin ≥ 64 (Cin = 32 is the small-Cin variant).
REG_MASKS = ["sdot", "sdot_acc", "sdot_bab", "sdot_acc_bab", "bias_prelu", "bias", "acc", "bias_acc"]
LDS_MASKS = ["mod", "mod_lrelu_in", "tap_mask", "bias_csum", "mask_slope", "bias_relu"]
ANY = REG_MASKS + LDS_MASKS
G16, G17 = [(2, 16, 16)], [(2, 17, 18)]


def gen_knobs(regepi, smalltile):
    return dict(ALL_OFF, MIA_CONV_REGEPI=regepi, MIA_CONV_SMALLTILE=smalltile)


GENERIC = cases([
    ("tile128x128/reg", gen_knobs(1, 0), G16, [(128, 128)], REG_MASKS),
    ("tile128x128/lds", gen_knobs(1, 0), G16, [(128, 128)], LDS_MASKS),
    ("tile128x128/lds", gen_knobs(1, 0), G16, [(32, 128)], ANY),
    ("tile128x128/lds", gen_knobs(1, 0), G17, [(128, 128), (32, 128)], ANY),
    ("tile128x128/lds", gen_knobs(0, 0), G16, [(128, 128)], REG_MASKS),
    ("tile128x64/reg", gen_knobs(1, 0), G16, [(128, 64), (32, 64)], REG_MASKS),
    ("tile128x64/lds", gen_knobs(1, 0), G16, [(128, 64), (32, 64)], LDS_MASKS),
    ("tile128x64/lds", gen_knobs(1, 0), G17, [(128, 64), (32, 64)], ANY),
    ("tile128x64/lds", gen_knobs(0, 0), G16, [(128, 64), (32, 64)], REG_MASKS),
    ("tile64x64/lds", gen_knobs(1, 512), G16 + G17, [(128, 128), (32, 128)], ANY)])

# ---- conv_thin.hip: the 8 → 64 input layer and its 64 → 8 gradient, 2-byte -----------------------
THIN = cases([("thin", {}, [(2, 17, 16)], [(8, 64)], ["bias_relu", "bias_prelu"]),
              ("thin", {}, [(2, 17, 16)], [(64, 8)], ["plain", "acc"])])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize(ARGS, WRES + WRES32 + THIN32 + WRES128 + HALO + GENERIC + THIN)
def test_stride1_3x3(cuda, tune, dtype, path, knobs, N, H, W, Cin, Cout, mask):
    check(cuda, tune, knobs, path, dtype, N, H, W, Cin, Cout, mask)


# ---- mia_conv2d stride 2 on the generic tile (the e4e body / style-head convs) -------------------
# 8×8 outputs: 64 pixels per image, so no register epilogue; 2 tiles, so the 64×64 tile at Cout 128
S2MASKS = ["bias_prelu", "mask_slope_acc", "csum"]
S2 = cases([("tile128x64/lds", {}, [(2, 16, 16)], [(64, 64)], S2MASKS),
            ("tile64x64/lds", {}, [(2, 16, 16)], [(128, 128)], S2MASKS)])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize(ARGS, S2)
def test_conv2d_stride2(cuda, tune, dtype, path, knobs, N, H, W, Cin, Cout, mask):
    check(cuda, tune, knobs, path, dtype, N, H, W, Cin, Cout, mask, stride=2)


# ---- the up-sampling conv (conv_transpose2d stride 2) and its adjoint ----------------------------
def seeded(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


@functools.lru_cache(maxsize=None)
def build_upconv(dtype, N, R, Cin, Cout, mod):
    g = seeded("upconv", N, R, Cin, Cout, mod)
    x = torch.randn(N, Cin, R, R, generator=g).to(dtype)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(4 * Cin)).to(dtype)
    s = torch.rand(N, Cin, generator=g) + 0.5
    xe = cb.modulate(x, s, True, dtype) if mod == "style_lrelu" else x
    r = cb.conv_ref_bound(xe, w, dtype, cb.phase_taps(2 * R + 1, 0, Cin), None, cb.upconv())
    return x, w, s, r


# the halo kernel needs R % 16 == 0 (upconv_halo_eligible): R = 8 falls back to the phase GEMMs
# inside the library, R = 16 reaches them with MIA_UPCONV_HALO=0. The halo form also runs its last
# row / column as edge groups on the generic tile and must keep its own name over theirs.
UPFWD = [pytest.param(path, knobs, R, ci, co, mod, id=f"{path}-{ci}-{co}-R{R}-{mod}")
         for path, knobs, R in [("upconv_halo", {}, 16), ("phase_gemm", {}, 8),
                                ("phase_gemm", {"MIA_UPCONV_HALO": 0}, 16)]
         for ci, co in [(64, 64), (128, 64)] for mod in ("plain", "style_lrelu")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("path,knobs,R,Cin,Cout,mod", UPFWD)
def test_upconv_fwd(cuda, tune, dtype, path, knobs, R, Cin, Cout, mod):
    for name, value in knobs.items():
        tune(name, value)
    N = 2
    x, w, s, r = build_upconv(dtype, N, R, Cin, Cout, mod)
    wph = [m.to(cuda) for m in layouts.upconv_subpixel_matrices(w, dtype)]
    w_up = layouts.upconv_halo_matrix(w, dtype).to(cuda)
    t = torch.empty(N, 2 * R + 1, 2 * R + 1, Cout, dtype=dtype, device=cuda)
    pro = mod == "style_lrelu"
    ops.upconv_fwd(nhwc(x).to(cuda), wph, t, Cout, ops.ACT_LRELU_S2 if pro else ops.ACT_NONE,
                   s.to(cuda) if pro else None, w_up=w_up)
    got = ops.last_conv_path()
    torch.cuda.synchronize()
    verdict(path, got, dtype, f"{Cin:3d}->{Cout:<3d} {N}xR{R} upconv_fwd {mod:12s}",
            t.permute(0, 3, 1, 2).cpu(), {}, r)


@functools.lru_cache(maxsize=None)
def build_upconv_dgrad(dtype, N, R, Cin, Cout, mask):
    """The adjoint of the Cin → Cout up-conv: gT (N, Cout, 2R+1, 2R+1) → gx (N, Cin, R, R)."""
    g = seeded("upconv_dgrad", N, R, Cin, Cout, mask)
    gt = torch.randn(N, Cout, 2 * R + 1, 2 * R + 1, generator=g).to(dtype)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cout)).to(dtype)
    e = cb.Epilogue(out_scale=torch.rand(N, Cin, generator=g) + 0.5,
                    aux_x=torch.randn(N, Cin, R, R, generator=g).to(dtype), sdot=True)
    if mask == "sdot_lrelu":
        e.act_aux = cb.ACT_LRELU_S2
    y0 = torch.randn(N, Cin, R, R, generator=g).to(dtype)
    if "acc" in mask:
        e.y0 = y0
    if "bab" in mask:
        e.bab = dict(demod=torch.rand(N, Cin, generator=g) + 0.5,
                     noise=torch.randn(R * R, generator=g), noise_w=0.3,
                     bias=torch.randn(Cin, generator=g) * 0.1)
    r = cb.conv_ref_bound(gt, w, dtype, 9 * Cout, e, cb.upconv_dgrad())
    return gt, w, e, r


# gx has Cin channels: the 128×64 tile at 64, the 128×128 tile at 128 (MIA_CONV_SMALLTILE=0; the
# 64×64 tile at the default). Register epilogue: R = 16 (256 pixels per image) and act_x NONE.
BIG = {"MIA_CONV_SMALLTILE": 0}
UPDG = [pytest.param(path, knobs, R, ci, 64, m, id=f"{path}-{ci}-64-R{R}-{m}")
        for path, knobs, R, ci, masks in [
            ("tile128x64/reg", {}, 16, 64, ["sdot", "sdot_bab", "sdot_acc_bab"]),
            ("tile128x64/lds", {}, 16, 64, ["sdot_lrelu"]),
            ("tile128x64/lds", {}, 8, 64, ["sdot", "sdot_lrelu", "sdot_bab", "sdot_acc_bab"]),
            ("tile128x128/reg", BIG, 16, 128, ["sdot", "sdot_bab", "sdot_acc_bab"]),
            ("tile128x128/lds", BIG, 16, 128, ["sdot_lrelu"]),
            ("tile128x128/lds", BIG, 8, 128, ["sdot", "sdot_lrelu", "sdot_bab", "sdot_acc_bab"]),
            ("tile64x64/lds", {}, 16, 128, ["sdot", "sdot_bab"])]
        for m in masks]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("path,knobs,R,Cin,Cout,mask", UPDG)
def test_upconv_dgrad(cuda, tune, dtype, path, knobs, R, Cin, Cout, mask):
    """mia_upconv_dgrad (sdot, with and without act_x) and mia_upconv_dgrad_fused (+ bab_q)."""
    for name, value in knobs.items():
        tune(name, value)
    N = 2
    gt, w, e, r = build_upconv_dgrad(dtype, N, R, Cin, Cout, mask)
    wt = layouts.upconv_dgrad_matrix(w, dtype).to(cuda)
    gx = (nhwc(e.y0).to(cuda) if e.y0 is not None
          else torch.empty(N, R, R, Cin, dtype=dtype, device=cuda))
    sums = {"sdot": torch.zeros(N, Cin, device=cuda)}
    if e.bab is None:
        ops.upconv_dgrad(nhwc(gt).to(cuda), wt, gx, Cin, nhwc(e.aux_x).to(cuda),
                         ops.ACT_LRELU_S2 if e.act_aux else ops.ACT_NONE, e.out_scale.to(cuda),
                         sums["sdot"])
    else:
        sums["bab_q"] = torch.zeros(N, Cin, device=cuda)
        bab = dict(demod=e.bab["demod"].to(cuda), noise=e.bab["noise"].to(cuda), noise_w=0.3,
                   bias=e.bab["bias"].to(cuda), q=sums["bab_q"])
        ops.upconv_dgrad_fused(nhwc(gt).to(cuda), wt, gx, Cin, nhwc(e.aux_x).to(cuda),
                               e.out_scale.to(cuda), sums["sdot"], bab, e.y0 is not None)
    got = ops.last_conv_path()
    torch.cuda.synchronize()
    verdict(path, got, dtype, f"{Cout:3d}->{Cin:<3d} {N}xR{R} upconv_dgrad {mask:12s}",
            gx.permute(0, 3, 1, 2).cpu(), {k: v.cpu() for k, v in sums.items()}, r)


# ---- mia_conv_s2_dgrad_halo: the input gradient of a stride-2 conv on the halo kernel -------------
@functools.lru_cache(maxsize=None)
def build_s2dg(dtype, N, R, Cg, Cx, mask):
    g = seeded("s2dg", N, R, Cg, Cx, mask)
    gy = torch.randn(N, Cg, R, R, generator=g).to(dtype)
    w = (torch.randn(Cg, Cx, 3, 3, generator=g) / math.sqrt(4 * Cg)).to(dtype)
    e = cb.Epilogue()
    if "mask" in mask:
        e.mask_a = torch.randn(N, Cx, 2 * R, 2 * R, generator=g).to(dtype)
        e.mask_slope = torch.rand(Cx, generator=g) * 0.5 + 0.05
    if "acc" in mask:
        e.y0 = torch.randn(N, Cx, 2 * R, 2 * R, generator=g).to(dtype)
    # with a mask or accumulate the 2-byte epilogue works on the accumulator already rounded to T
    # and rounds again on the store (csrc/conv_upconv.hip upconv_halo_kernel): cb.pre_round_term
    e.pre_round = mask != "plain"
    r = cb.conv_ref_bound(gy, w, dtype, cb.phase_taps(2 * R, 1, Cg), e, cb.s2_dgrad())
    return gy, w, e, r


# the kernel needs R % 16 == 0 (s2_dgrad_halo_eligible; smaller maps are refused): the smallest
# accepted gradient map is 16×16, the gradient of a 32 → 16 conv
S2DG = [pytest.param(cg, 64, m, id=f"{cg}-64-{m}") for cg in (64, 128)
        for m in ("plain", "mask_slope", "acc", "mask_slope_acc")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Cg,Cx,mask", S2DG)
def test_s2_dgrad_halo(cuda, tune, dtype, Cg, Cx, mask):
    N, R = 2, 16
    gy, w, e, r = build_s2dg(dtype, N, R, Cg, Cx, mask)
    gx = (nhwc(e.y0).to(cuda) if e.y0 is not None
          else torch.empty(N, 2 * R, 2 * R, Cx, dtype=dtype, device=cuda))
    ops.s2_dgrad_halo(nhwc(gy).to(cuda), layouts.s2_dgrad_halo_matrix(w, dtype).to(cuda), gx,
                      mask_a=nhwc(e.mask_a).to(cuda) if e.mask_a is not None else None,
                      mask_slope=e.mask_slope.to(cuda) if e.mask_slope is not None else None,
                      accumulate=e.y0 is not None)
    got = ops.last_conv_path()
    torch.cuda.synchronize()
    verdict("s2dg_halo", got, dtype, f"{Cg:3d}->{Cx:<3d} {N}xR{R} s2_dgrad_halo {mask:14s}",
            gx.permute(0, 3, 1, 2).cpu(), {}, r)
