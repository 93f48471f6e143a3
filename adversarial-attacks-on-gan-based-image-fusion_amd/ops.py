"""Typed host wrappers over the C ABI: torch tensors in, device pointers + the current HIP stream
out. Every wrapper validates shapes/dtypes/contiguity on the host before a kernel is launched, so a
malformed call raises here instead of faulting on the GPU."""
import ctypes
import math
import numbers

import torch

from . import _lib, layouts
from ._lib import ACT_LRELU_S2, ACT_NONE, ACT_PRELU, ACT_RELU, ConvArgs, call  # noqa: F401

DTYPES = {torch.float32: _lib.MIA_F32, torch.float16: _lib.MIA_F16, torch.bfloat16: _lib.MIA_BF16}
VEC = {torch.float32: 4, torch.float16: 8, torch.bfloat16: 8}


def dt(t_or_dtype):
    d = t_or_dtype if isinstance(t_or_dtype, torch.dtype) else t_or_dtype.dtype
    if d not in DTYPES:
        raise TypeError(f"unsupported dtype {d}")
    return DTYPES[d]


def ptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise ValueError("device tensor required (the attack path runs on the GPU only)")
    if not t.is_contiguous():
        raise ValueError("contiguous tensor required")
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need(t, shape, dtype=None, name="tensor"):
    if t is None:
        raise ValueError(f"{name} is required")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: shape {tuple(t.shape)} != {tuple(shape)}")
    if dtype is not None and t.dtype != dtype:
        raise ValueError(f"{name}: dtype {t.dtype} != {dtype}")


def _numel_ok(t, n, dtype=None, name="tensor"):
    if t is None:
        return
    if t.numel() != n:
        raise ValueError(f"{name}: numel {t.numel()} != {n}")
    if dtype is not None and t.dtype != dtype:
        raise ValueError(f"{name}: dtype {t.dtype} != {dtype}")


def last_conv_path():
    """The kernel family this thread's last conv launch dispatched to (mia_last_conv_path), e.g.
    ``"halo/reg"``, ``"wres128/reg"``, ``"tile128x64/lds"``, ``"upconv_halo"``."""
    return _lib.load().mia_last_conv_path().decode()


def conv_kpad(cin, dtype):
    bk = 32 if dtype == torch.float32 else 64
    return (9 * cin + bk - 1) // bk * bk


# Live per-launch timing of the conv kernel (bench.py roofline): when PROFILE is a list, every
# conv3x3 call is bracketed by HIP events on the launch stream and (start, end, algorithmic
# FLOPs) is appended. None (default) = no events.
PROFILE = None
# Tuning aid (tools/layer_table.py): when a list, one label per PROFILE entry (API + shape).
PROFILE_TAGS = None


def _tag(label):
    if PROFILE_TAGS is not None:
        PROFILE_TAGS.append(label)


def conv3x3(x, w, y, *, cout, act_in=ACT_NONE, in_scale=None, out_scale=None, bias=None,
            noise=None, noise_w=0.0, act_out=ACT_NONE, shuffle_out=False, aux_x=None,
            act_aux=ACT_NONE, sdot=None, tap_a=None, tap_t=None, tap_coef=0.0, mask_a=None,
            accumulate=False, y_cstride=0, bab=None, flops=None):
    """Generic MFMA implicit-GEMM conv (mia_conv3x3). x: (N,H,W,Cin); w: (Cout,Kpad).
    ``bab``: dict(demod, noise, noise_w, bias, q) — fused StyledConv backward front of the layer
    whose stored activation is aux_x (mia_conv_args.bab_*).
    ``flops``: algorithmic FLOPs of this launch for profiling (default 2·N·H·W·9·Cin·Cout)."""
    N, H, W, Cin = x.shape
    T = x.dtype
    kpad = conv_kpad(Cin, T)
    _need(w, (cout, kpad), T, "w")
    if Cin % VEC[T]:
        raise ValueError("Cin must be a multiple of the 16-byte vector")
    cm = cout // 4 if shuffle_out else cout
    ys = y_cstride or cm
    if y is not None:
        if shuffle_out:
            _need(y, (N, 2 * H, 2 * W, ys), T, "y")
        else:
            _need(y, (N, H, W, ys), T, "y")
    f32 = torch.float32
    _numel_ok(in_scale, N * Cin, f32, "in_scale")
    _numel_ok(out_scale, N * cm, f32, "out_scale")
    _numel_ok(bias, cm, f32, "bias")
    Ho, Wo = (2 * H, 2 * W) if shuffle_out else (H, W)
    _numel_ok(noise, Ho * Wo, f32, "noise")
    for name, a in (("aux_x", aux_x), ("tap_a", tap_a), ("tap_t", tap_t), ("mask_a", mask_a)):
        if a is not None:
            _need(a, (N, H, W, cout), T, name)
    _numel_ok(sdot, N * cout, f32, "sdot")
    if bab is not None:
        _numel_ok(bab["demod"], N * cout, f32, "bab.demod")
        _numel_ok(bab["q"], N * cout, f32, "bab.q")
        _numel_ok(bab.get("noise"), H * W, f32, "bab.noise")
        _numel_ok(bab.get("bias"), cout, f32, "bab.bias")
        if aux_x is None:
            raise ValueError("bab needs aux_x (the stored activation)")
    a = ConvArgs()
    a.x, a.w, a.y = ptr(x), ptr(w), ptr(y)
    a.N, a.H, a.W, a.Cin, a.Cout, a.Kpad = N, H, W, Cin, cout, kpad
    a.y_cstride = ys
    a.act_in = act_in
    a.in_scale, a.out_scale, a.bias, a.noise = ptr(in_scale), ptr(out_scale), ptr(bias), ptr(noise)
    a.noise_w = float(noise_w)
    a.act_out = act_out
    a.shuffle_out = int(bool(shuffle_out))
    a.aux_x, a.act_aux, a.sdot = ptr(aux_x), act_aux, ptr(sdot)
    a.tap_a, a.tap_t, a.tap_coef, a.mask_a = ptr(tap_a), ptr(tap_t), float(tap_coef), ptr(mask_a)
    a.accumulate = int(bool(accumulate))
    ws = layouts.split_for(w) if T == torch.float32 and not shuffle_out else None
    a.w_split = ptr(ws)
    if bab is not None:
        a.bab_demod, a.bab_q = ptr(bab["demod"]), ptr(bab["q"])
        a.bab_noise, a.bab_noise_w = ptr(bab.get("noise")), float(bab.get("noise_w", 0.0))
        a.bab_bias = ptr(bab.get("bias"))
    prof = PROFILE
    if prof is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    call("mia_conv3x3", ctypes.byref(a), dt(T), stream())
    if prof is not None:
        e1.record()
        prof.append((e0, e1, flops if flops is not None else 2 * N * H * W * 9 * Cin * cout))
        _tag(f"conv3x3 {H}x{W} {Cin}->{cout}" + (" mod" if in_scale is not None else "")
             + (" bab" if bab is not None else "") + (" sdot" if sdot is not None else "")
             + (" tap" if tap_a is not None else "") + (" shuf" if shuffle_out else ""))
    return y


def conv3x3_modw(x, w, y, w_mod, *, cout, in_scale, out_scale=None, bias=None, noise=None,
                 noise_w=0.0, act_out=ACT_NONE, flops=None):
    """The StyledConv forward on per-image weights (fp16 / bf16): mia_modulate_weights writes
    w_mod[n] = w·in_scale[n]·out_scale[n] (the modulation and demodulation folded into the
    weights), then mia_conv3x3_wmod convolves the unmodulated x. Same result as
    conv3x3(x, w, y, in_scale=…, out_scale=…) up to where the one rounding to T happens.
    Profiled as ONE conv call (the weight pass included)."""
    N, H, W, Cin = x.shape
    T = x.dtype
    if T not in (torch.float16, torch.bfloat16):
        raise ValueError("per-image weights: fp16 / bf16 only")
    kpad = conv_kpad(Cin, T)
    _need(w, (cout, kpad), T, "w")
    _need(w_mod, (N, cout, kpad), T, "w_mod")
    _need(y, (N, H, W, cout), T, "y")
    f32 = torch.float32
    _numel_ok(in_scale, N * Cin, f32, "in_scale")
    _numel_ok(out_scale, N * cout, f32, "out_scale")
    _numel_ok(bias, cout, f32, "bias")
    _numel_ok(noise, H * W, f32, "noise")
    if in_scale is None:
        raise ValueError("in_scale (the style) is required")
    a = ConvArgs()
    a.x, a.w, a.y = ptr(x), ptr(w_mod), ptr(y)
    a.N, a.H, a.W, a.Cin, a.Cout, a.Kpad = N, H, W, Cin, cout, kpad
    a.y_cstride = cout
    a.act_in = ACT_NONE
    a.bias, a.noise = ptr(bias), ptr(noise)
    a.noise_w = float(noise_w)
    a.act_out = act_out
    prof = PROFILE
    if prof is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    call("mia_modulate_weights", ptr(w), ptr(in_scale), ptr(out_scale), ptr(w_mod), N, cout, Cin,
         kpad, dt(T), stream())
    call("mia_conv3x3_wmod", ctypes.byref(a), cout * kpad, dt(T), stream())
    if prof is not None:
        e1.record()
        prof.append((e0, e1, flops if flops is not None else 2 * N * H * W * 9 * Cin * cout))
        _tag(f"conv3x3 {H}x{W} {Cin}->{cout} mod wmod")
    return y


def _prof_call(name, flops, *args):
    prof = PROFILE
    if prof is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    call(name, *args)
    if prof is not None:
        e1.record()
        prof.append((e0, e1, flops))
        _tag(f"{name} " + (f"R{args[6]} x{args[1]}" if name == "mia_conv_s2_dgrad_halo_multi"
                             else f"{args[5:8]}" if name.endswith("_split")
                             else f"{args[4:7]}"))


def upconv_kpad(cin, phase, dtype):
    kh, kw = 2 - (phase >> 1), 2 - (phase & 1)
    bk = 32 if dtype == torch.float32 else 64
    return (kh * kw * cin + bk - 1) // bk * bk


def upconv_fwd(x, w_phases, t_out, cout, act_in=ACT_NONE, style=None, flops=None, w_up=None):
    """conv_transpose2d(stride 2) as 4 sub-pixel phase GEMMs (one launch). x: (N,R,R,Cin) →
    T: (N, 2R+1, 2R+1, Cout). ``w_up`` (layouts.upconv_halo_matrix): the halo-tiled kernel
    (mia_upconv_fwd_halo; the library falls back to the phase GEMMs where it does not apply)."""
    N, R, R2, Cin = x.shape
    T = x.dtype
    if R != R2:
        raise ValueError("square inputs only")
    if len(w_phases) != 4:
        raise ValueError("4 phase weight matrices required")
    for ph, w in enumerate(w_phases):
        _need(w, (cout, upconv_kpad(Cin, ph, T)), T, f"w_phase[{ph}]")
    _need(t_out, (N, 2 * R + 1, 2 * R + 1, cout), T, "t_out")
    _numel_ok(style, N * Cin, torch.float32, "style")
    wp = (ctypes.c_void_p * 4)(*[w.data_ptr() for w in w_phases])
    for w in w_phases:
        ptr(w)
    fl = flops if flops is not None else 2 * N * R * R * 9 * Cin * cout
    if w_up is not None:
        bk = layouts.halo_bk(T)
        _need(w_up, (Cin // bk, 5, 2, cout, bk), T, "w_up")
        ws = layouts.split_for(w_up) if T == torch.float32 else None
        _prof_call("mia_upconv_fwd_halo_split", fl, ptr(x), wp, ptr(w_up), ptr(ws), ptr(t_out), N,
                   R, Cin, cout, act_in, ptr(style), dt(T), stream())
        return t_out
    _prof_call("mia_upconv_fwd", fl, ptr(x), wp, ptr(t_out), N, R, Cin, cout, act_in, ptr(style),
               dt(T), stream())
    return t_out


def upconv_blur_fwd(t, pre, demod, noise, noise_w, bias, act_out=ACT_NONE):
    N, TS, _, C = t.shape
    R = (TS - 1) // 2
    _need(pre, (N, 2 * R, 2 * R, C), t.dtype, "pre")
    _numel_ok(demod, N * C, torch.float32, "demod")
    _numel_ok(noise, 4 * R * R, torch.float32, "noise")
    _numel_ok(bias, C, torch.float32, "bias")
    call("mia_upconv_blur_fwd", ptr(t), ptr(pre), ptr(demod), ptr(noise), float(noise_w),
         ptr(bias), N, R, C, int(act_out), dt(t), stream())
    return pre


def upconv_blur_bwd(gy, gt):
    N, S, _, C = gy.shape
    R = S // 2
    _need(gt, (N, 2 * R + 1, 2 * R + 1, C), gy.dtype, "gt")
    call("mia_upconv_blur_bwd", ptr(gy), ptr(gt), N, R, C, dt(gy), stream())
    return gt


def upconv_dgrad(g_t, w_t, gx, cin, x_fwd, act_x, style, sdot, flops=None):
    N, TS, _, Cout = g_t.shape
    R = (TS - 1) // 2
    T = g_t.dtype
    _need(w_t, (cin, conv_kpad(Cout, T)), T, "w_t")
    if gx is not None:
        _need(gx, (N, R, R, cin), T, "gx")
    _need(x_fwd, (N, R, R, cin), T, "x_fwd")
    _numel_ok(style, N * cin, torch.float32, "style")
    _numel_ok(sdot, N * cin, torch.float32, "sdot")
    _prof_call("mia_upconv_dgrad", flops if flops is not None else 2 * N * R * R * 9 * Cout * cin,
               ptr(g_t), ptr(w_t), ptr(gx), N, R, Cout, cin, ptr(x_fwd), act_x, ptr(style),
               ptr(sdot), dt(T), stream())
    return gx


def upconv_dgrad_fused(g_t, w_t, gx, cin, x_fwd, style, sdot, bab, accumulate, flops=None):
    """upconv_dgrad with the fused backward front of the layer below (mia_upconv_dgrad_fused):
    gx ← demod-scaled pre-activation gradient of that layer; bab = dict(demod, noise, noise_w,
    bias, q)."""
    N, TS, _, Cout = g_t.shape
    R = (TS - 1) // 2
    T = g_t.dtype
    _need(w_t, (cin, conv_kpad(Cout, T)), T, "w_t")
    _need(gx, (N, R, R, cin), T, "gx")
    _need(x_fwd, (N, R, R, cin), T, "x_fwd")
    _numel_ok(style, N * cin, torch.float32, "style")
    _numel_ok(sdot, N * cin, torch.float32, "sdot")
    _numel_ok(bab["demod"], N * cin, torch.float32, "bab.demod")
    _numel_ok(bab["q"], N * cin, torch.float32, "bab.q")
    _numel_ok(bab.get("noise"), R * R, torch.float32, "bab.noise")
    _numel_ok(bab.get("bias"), cin, torch.float32, "bab.bias")
    ws = layouts.split_for(w_t) if T == torch.float32 else None
    _prof_call("mia_upconv_dgrad_fused_split",
               flops if flops is not None else 2 * N * R * R * 9 * Cout * cin,
               ptr(g_t), ptr(w_t), ptr(ws), ptr(gx), N, R, Cout, cin, ptr(x_fwd), ptr(style),
               ptr(sdot),
               int(bool(accumulate)), ptr(bab["demod"]), ptr(bab.get("noise")),
               float(bab.get("noise_w", 0.0)), ptr(bab.get("bias")), ptr(bab["q"]), dt(T),
               stream())
    return gx


def bias_act_fwd(x, noise, noise_w, bias, y):
    N, H, W, C = x.shape
    _need(y, x.shape, x.dtype, "y")
    _numel_ok(noise, H * W, torch.float32, "noise")
    _numel_ok(bias, C, torch.float32, "bias")
    call("mia_bias_act_fwd", ptr(x), ptr(noise), float(noise_w), ptr(bias), ptr(y), N, H, W, C,
         dt(x), stream())
    return y


def bias_act_bwd(g_a, pre, noise, noise_w, bias, demod, gy, q, unshuffle=False, from_act=False):
    N, H, W, C = pre.shape
    _need(g_a, pre.shape, pre.dtype, "g_a")
    _numel_ok(noise, H * W, torch.float32, "noise")
    _numel_ok(bias, C, torch.float32, "bias")
    _numel_ok(demod, N * C, torch.float32, "demod")
    _numel_ok(q, N * C, torch.float32, "q")
    if unshuffle:
        _need(gy, (N, H // 2, W // 2, 4 * C), pre.dtype, "gy")
    else:
        _need(gy, pre.shape, pre.dtype, "gy")
    call("mia_bias_act_bwd", ptr(g_a), ptr(pre), ptr(noise), float(noise_w), ptr(bias), ptr(demod),
         ptr(gy), ptr(q), N, H, W, C, int(bool(unshuffle)), int(bool(from_act)), dt(pre), stream())
    return gy


def _updn_out(H, up, down, p0, p1, kt):
    return (H * up + p0 + p1 - kt) // down + 1


def upfirdn2d_fwd(x, y, k1d, up=1, down=1, pad=(0, 0)):
    """x: (..., H, W) fp32; k1d: host list of taps."""
    H, W = x.shape[-2:]
    planes = x.numel() // (H * W)
    kt = len(k1d)
    Ho, Wo = _updn_out(H, up, down, pad[0], pad[1], kt), _updn_out(W, up, down, pad[0], pad[1], kt)
    _need(y, tuple(x.shape[:-2]) + (Ho, Wo), torch.float32, "y")
    k = (ctypes.c_float * kt)(*k1d)
    call("mia_upfirdn2d_fwd", ptr(x), ptr(y), planes, H, W, k, kt, up, down, pad[0], pad[1],
         stream())
    return y


def upfirdn2d_bwd(gy, gx, k1d, up=1, down=1, pad=(0, 0)):
    H, W = gx.shape[-2:]
    planes = gx.numel() // (H * W)
    kt = len(k1d)
    Ho, Wo = _updn_out(H, up, down, pad[0], pad[1], kt), _updn_out(W, up, down, pad[0], pad[1], kt)
    _need(gy, tuple(gx.shape[:-2]) + (Ho, Wo), torch.float32, "gy")
    k = (ctypes.c_float * kt)(*k1d)
    call("mia_upfirdn2d_bwd", ptr(gy), ptr(gx), planes, H, W, k, kt, up, down, pad[0], pad[1],
         stream())
    return gx


def torgb_fwd(pre, style, wr, bias, skip, rgb, act_in=ACT_LRELU_S2):
    N, H, W, Cin = pre.shape
    _numel_ok(style, N * Cin, torch.float32, "style")
    _need(wr, (3, Cin), torch.float32, "wr")
    _numel_ok(bias, 3, torch.float32, "bias")
    if skip is not None:
        _need(skip, (N, 3, H // 2, W // 2), torch.float32, "skip")
    _need(rgb, (N, 3, H, W), torch.float32, "rgb")
    call("mia_torgb_fwd", ptr(pre), ptr(style), ptr(wr), ptr(bias), ptr(skip), ptr(rgb), N, H, W,
         Cin, int(act_in), dt(pre), stream())
    return rgb


def torgb_bwd(g_rgb, pre, style, wr, g_a, gs, accumulate, act_in=ACT_LRELU_S2):
    N, H, W, Cin = pre.shape
    _need(g_rgb, (N, 3, H, W), torch.float32, "g_rgb")
    _numel_ok(style, N * Cin, torch.float32, "style")
    _need(wr, (3, Cin), torch.float32, "wr")
    _need(g_a, pre.shape, pre.dtype, "g_a")
    _numel_ok(gs, N * Cin, torch.float32, "gs")
    call("mia_torgb_bwd", ptr(g_rgb), ptr(pre), ptr(style), ptr(wr), ptr(g_a), ptr(gs), N, H, W,
         Cin, int(bool(accumulate)), int(act_in), dt(pre), stream())


def torgb_bwd_front(g_rgb, act, style, wr, gy, gs, demod, noise, noise_w, bias, q):
    """ToRGB backward + the topmost StyledConv's backward front (mia_torgb_bwd_front)."""
    N, H, W, Cin = act.shape
    _need(g_rgb, (N, 3, H, W), torch.float32, "g_rgb")
    _need(gy, act.shape, act.dtype, "gy")
    _numel_ok(style, N * Cin, torch.float32, "style")
    _numel_ok(wr, 3 * Cin, torch.float32, "wr")
    _numel_ok(gs, N * Cin, torch.float32, "gs")
    _numel_ok(demod, N * Cin, torch.float32, "demod")
    _numel_ok(q, N * Cin, torch.float32, "q")
    _numel_ok(noise, H * W, torch.float32, "noise")
    _numel_ok(bias, Cin, torch.float32, "bias")
    call("mia_torgb_bwd_front", ptr(g_rgb), ptr(act), ptr(style), ptr(wr), ptr(gy), ptr(gs), N,
         H, W, Cin, ptr(demod), ptr(noise), float(noise_w), ptr(bias), ptr(q), dt(act), stream())
    return gy


def pool_out(H, ceil_mode):
    return (H + 1) // 2 if ceil_mode else H // 2


def maxpool2_fwd(x, y, ceil_mode=False):
    N, H, W, C = x.shape
    _need(y, (N, pool_out(H, ceil_mode), pool_out(W, ceil_mode), C), x.dtype, "y")
    call("mia_maxpool2_fwd", ptr(x), ptr(y), N, H, W, C, int(bool(ceil_mode)), dt(x), stream())
    return y


def maxpool2_bwd(x, g_out, g_in, ceil_mode=False, tap_t=None, tap_coef=0.0, mask=False):
    N, H, W, C = x.shape
    _need(g_out, (N, pool_out(H, ceil_mode), pool_out(W, ceil_mode), C), x.dtype, "g_out")
    _need(g_in, x.shape, x.dtype, "g_in")
    if tap_t is not None:
        _need(tap_t, x.shape, x.dtype, "tap_t")
    call("mia_maxpool2_bwd", ptr(x), ptr(g_out), ptr(g_in), N, H, W, C, int(bool(ceil_mode)),
         ptr(tap_t), float(tap_coef), int(bool(mask)), dt(x), stream())
    return g_in


def avgpool_fwd(x, y, k):
    H, W = x.shape[-2:]
    planes = x.numel() // (H * W)
    _need(y, tuple(x.shape[:-2]) + (H // k, W // k), torch.float32, "y")
    call("mia_avgpool_fwd", ptr(x), ptr(y), planes, H, W, k, stream())
    return y


def avgpool_bwd(gy, gx, k, accumulate=False):
    H, W = gx.shape[-2:]
    planes = gx.numel() // (H * W)
    _need(gy, tuple(gx.shape[:-2]) + (H // k, W // k), torch.float32, "gy")
    call("mia_avgpool_bwd", ptr(gy), ptr(gx), planes, H, W, k, int(bool(accumulate)), stream())
    return gx


def image_to_nhwc(x, y, pf, cpad):
    N, C, S, _ = x.shape
    if C != 3 or x.dtype != torch.float32:
        raise ValueError("x must be (N,3,S,S) fp32")
    _need(y, (N, S // pf, S // pf, cpad), None, "y")
    call("mia_image_to_nhwc", ptr(x), ptr(y), N, S, pf, cpad, dt(y), stream())
    return y


def mse_sum(a, b, loss, coef=1.0):
    """loss[n] += coef·Σ (a[n] − b[n])²."""
    n = a.shape[0]
    _need(b, a.shape, a.dtype, "b")
    _numel_ok(loss, n, torch.float32, "loss")
    call("mia_mse_sum", ptr(a), ptr(b), ptr(loss), n, a.numel() // n, float(coef), dt(a), stream())
    return loss


def ssim_workspace_numel(N, H, W):
    """fp64 elements of mia_ssim2's scratch (one partial per image and output tile)."""
    return int(_lib.load().mia_ssim_workspace_size(N, H, W)) // 8


def ssim(ref, imgs, data_range, work, out):
    """mia_ssim2: ref (3,H,W), imgs (N,3,H,W) fp32 → out[n] = SSIM(gray(ref), gray(imgs[n]))."""
    N, _, H, W = imgs.shape
    _need(ref, (3, H, W), torch.float32, "ref")
    _need(imgs, (N, 3, H, W), torch.float32, "imgs")
    _numel_ok(work, ssim_workspace_numel(N, H, W), torch.float64, "work")
    _numel_ok(out, N, torch.float32, "out")
    call("mia_ssim2", ptr(ref), ptr(imgs), N, H, W, float(data_range), ptr(work),
         work.numel() * work.element_size(), ptr(out), stream())
    return out


def mse_grad_f32(a, b, g, coef, accumulate=False):
    _need(b, a.shape, torch.float32, "b")
    _need(g, a.shape, torch.float32, "g")
    call("mia_mse_grad_f32", ptr(a), ptr(b), ptr(g), a.numel(), float(coef),
         int(bool(accumulate)), stream())
    return g


def tap_grad(a, t, g, coef, mask=True):
    _need(t, a.shape, a.dtype, "t")
    _need(g, a.shape, a.dtype, "g")
    call("mia_tap_grad", ptr(a), ptr(t), ptr(g), a.numel(), float(coef), int(bool(mask)), dt(a),
         stream())
    return g


def _pixel_grad_shape(x, g_vgg, pf, name="x"):
    """(N, S, cpad) of an (N,3,S,S) fp32 image batch and its pooled NHWC gradient g_vgg (or None),
    whose first three of cpad channels the kernels read."""
    if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3] or x.dtype != torch.float32:
        raise ValueError(f"{name} must be (N,3,S,S) fp32")
    N, _, S, _ = x.shape
    if pf < 1 or S % pf:
        raise ValueError("pf must divide S")
    cpad = 8
    if g_vgg is not None:
        cpad = g_vgg.shape[-1]
        if cpad < 3:
            raise ValueError(f"g_vgg: {cpad} channels, at least 3 are read")
        _need(g_vgg, (N, S // pf, S // pf, cpad), None, "g_vgg")
    return N, S, cpad


def image_grad(rec, t, g_vgg, g_img, pf, coef):
    N, S, cpad = _pixel_grad_shape(rec, g_vgg, pf, "rec")
    _need(t, rec.shape, torch.float32, "t")
    _need(g_img, rec.shape, torch.float32, "g_img")
    gdt = dt(g_vgg) if g_vgg is not None else _lib.MIA_F32
    call("mia_image_grad", ptr(rec), ptr(t), ptr(g_vgg), ptr(g_img), N, S, pf, cpad, float(coef),
         gdt, stream())
    return g_img


def pgd_update(x, x0, g_vgg, g_enc, pf, enc_res, coef_img, a, e, lo=-1.0, hi=1.0,
               nonfinite=None):
    N, S, cpad = _pixel_grad_shape(x, g_vgg, pf)
    _numel_ok(nonfinite, N, torch.int32, "nonfinite")
    _need(x0, x.shape, torch.float32, "x0")
    if g_enc is not None:
        _numel_ok(g_enc, N * 3 * enc_res * enc_res, torch.float32, "g_enc")
    gdt = dt(g_vgg) if g_vgg is not None else _lib.MIA_F32
    call("mia_pgd_update", ptr(x), ptr(x0), ptr(g_vgg), ptr(g_enc), N, S, pf, cpad, enc_res,
         float(coef_img), float(a), float(e), float(lo), float(hi), ptr(nonfinite), gdt, stream())
    return x


def grad_assemble(x, x0, g_vgg, g_enc, g, pf, enc_res, coef_img, scale=1.0, nonfinite=None):
    """∇_x L (fp32 NCHW) from the VGG input-path and encoder gradients (mia_grad_assemble)."""
    N, C, S, S2 = x.shape
    _numel_ok(nonfinite, N, torch.int32, "nonfinite")
    if C != 3 or S != S2:
        raise ValueError("x must be (N,3,S,S)")
    _need(x0, x.shape, torch.float32, "x0")
    _need(g, x.shape, torch.float32, "g")
    R = S // pf
    cpad = g_vgg.shape[-1] if g_vgg is not None else 8
    if g_vgg is not None:
        _need(g_vgg, (N, R, R, cpad), None, "g_vgg")
    if g_enc is not None:
        _need(g_enc, (N, 3, enc_res, enc_res), torch.float32, "g_enc")
    T = g_vgg.dtype if g_vgg is not None else torch.float32
    call("mia_grad_assemble", ptr(x), ptr(x0), ptr(g_vgg), ptr(g_enc), ptr(g), N, S, pf, cpad,
         enc_res, float(coef_img), float(scale), ptr(nonfinite), dt(T), stream())
    return g


def grad_assemble_norms(x, x0, g_vgg, g_enc, g, l1, l2sq, pf, enc_res, coef_img, scale=1.0,
                        nonfinite=None):
    """grad_assemble plus l1[n] += Σ|g_n| and l2sq[n] += Σ g_n² (either may be None), in one pass
    (mia_grad_assemble_norms)."""
    N, C, S, S2 = x.shape
    if C != 3 or S != S2:
        raise ValueError("x must be (N,3,S,S)")
    _need(x, x.shape, torch.float32, "x")
    _need(x0, x.shape, torch.float32, "x0")
    _need(g, x.shape, torch.float32, "g")
    _norm_outputs(N, l1, l2sq, nonfinite)
    if pf < 1 or S % pf:
        raise ValueError("pf must divide S")
    R = S // pf
    cpad = g_vgg.shape[-1] if g_vgg is not None else 8
    if g_vgg is not None:
        _need(g_vgg, (N, R, R, cpad), None, "g_vgg")
    if g_enc is not None:
        _need(g_enc, (N, 3, enc_res, enc_res), torch.float32, "g_enc")
    T = g_vgg.dtype if g_vgg is not None else torch.float32
    call("mia_grad_assemble_norms", ptr(x), ptr(x0), ptr(g_vgg), ptr(g_enc), ptr(g), ptr(l1),
         ptr(l2sq), N, S, pf, cpad, enc_res, float(coef_img), float(scale), ptr(nonfinite), dt(T),
         stream())
    return g


def _norm_outputs(N, l1, l2sq, nonfinite):
    """The optional per-image outputs of the *_norms entry points: N values each."""
    _numel_ok(l1, N, torch.float32, "l1")
    _numel_ok(l2sq, N, torch.float32, "l2sq")
    _numel_ok(nonfinite, N, torch.int32, "nonfinite")


def _image_rows(x, name="x"):
    """(N, elements per image) of a batch of fp32 images."""
    if x.dim() < 2 or x.dtype != torch.float32 or x.shape[0] < 1:
        raise ValueError(f"{name} must be a non-empty fp32 batch of images")
    return x.shape[0], x.numel() // x.shape[0]


def l2_step(x, x0, g, gnorm2sq, dsq, a, nonfinite=None):
    """x ← x + a·((−g)/(√gnorm2sq[n] + 1e-10)) (un-projected); dsq[n] += Σ(x − x0)²
    (mia_l2_step)."""
    N, plane = _image_rows(x)
    _need(x0, x.shape, torch.float32, "x0")
    _need(g, x.shape, torch.float32, "g")
    _need(gnorm2sq, (N,), torch.float32, "gnorm2sq")
    _need(dsq, (N,), torch.float32, "dsq")
    _numel_ok(nonfinite, N, torch.int32, "nonfinite")
    call("mia_l2_step", ptr(x), ptr(x0), ptr(g), ptr(gnorm2sq), ptr(dsq), N, plane, float(a),
         ptr(nonfinite), stream())
    return x


def l2_project(x, x0, dsq, e, lo=-1.0, hi=1.0):
    """x ← clamp(x0 + (x − x0)·min(e/√dsq[n], 1), lo, hi) (mia_l2_project)."""
    N, plane = _image_rows(x)
    _need(x0, x.shape, torch.float32, "x0")
    _need(dsq, (N,), torch.float32, "dsq")
    call("mia_l2_project", ptr(x), ptr(x0), ptr(dsq), N, plane, float(e), float(lo), float(hi),
         stream())
    return x


def mi_update(x, x0, g, l1, m, mu, a, e, lo=-1.0, hi=1.0, nonfinite=None):
    """m ← (−g)/(l1[n]/plane) + mu·m; x ← clamp(x0 + clamp(x + a·sign(m) − x0, −e, e), lo, hi)
    (mia_mi_update)."""
    N, plane = _image_rows(x)
    _need(x0, x.shape, torch.float32, "x0")
    _need(g, x.shape, torch.float32, "g")
    _need(m, x.shape, torch.float32, "m")
    _need(l1, (N,), torch.float32, "l1")
    _numel_ok(nonfinite, N, torch.int32, "nonfinite")
    call("mia_mi_update", ptr(x), ptr(x0), ptr(g), ptr(l1), ptr(m), N, plane, float(mu), float(a),
         float(e), float(lo), float(hi), ptr(nonfinite), stream())
    return x


def ti_smooth_norms(g, taps, gs, l1, l2sq, nonfinite=None):
    """gs ← (taps ⊗ taps) ⋆ g per plane, zero padded (the TI-FGSM smoothing), with
    l1[n] += Σ|gs_n| and l2sq[n] += Σ gs_n² (either may be None) (mia_ti_smooth_norms).
    g, gs: distinct fp32 (N,C,H,W); taps: K fp32 device values, K odd in 1 … 63."""
    if g is None or g.dim() != 4 or g.dtype != torch.float32 or g.numel() == 0:
        raise ValueError("g must be a non-empty fp32 (N,C,H,W) tensor")
    N, C, H, W = g.shape
    _need(gs, g.shape, torch.float32, "gs")
    if gs.data_ptr() == g.data_ptr():
        raise ValueError("g and gs must be distinct buffers")
    if taps is None or taps.dim() != 1 or taps.dtype != torch.float32:
        raise ValueError("taps must be a 1-D fp32 tensor")
    K = taps.numel()
    if K % 2 == 0 or not 1 <= K <= 63:
        raise ValueError("taps must hold an odd number of values, 1 … 63")
    _norm_outputs(N, l1, l2sq, nonfinite)
    call("mia_ti_smooth_norms", ptr(g), ptr(gs), ptr(taps), K, ptr(l1), ptr(l2sq), N, C, H, W,
         ptr(nonfinite), stream())
    return gs


def _di_args(x, y, rnd, top, left, xname, yname):
    """Shared checks of the input-diversity pair: distinct fp32 (N,C,S,S) tensors and a window
    rnd × rnd at (top, left) inside S × S. Returns (N, C, S, rnd, top, left) as ints."""
    if x is None or x.dim() != 4 or x.dtype != torch.float32 or x.numel() == 0:
        raise ValueError(f"{xname} must be a non-empty fp32 (N,C,S,S) tensor")
    N, C, S, S2 = x.shape
    if S != S2:
        raise ValueError(f"{xname} must have square planes (N,C,S,S)")
    _need(y, x.shape, torch.float32, yname)
    if y.data_ptr() == x.data_ptr():
        raise ValueError(f"{xname} and {yname} must be distinct buffers")
    for v in (rnd, top, left):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise ValueError("rnd, top and left must be integers")
    rnd, top, left = int(rnd), int(top), int(left)
    if not (1 <= rnd <= S and 0 <= top <= S - rnd and 0 <= left <= S - rnd):
        raise ValueError("need 1 <= rnd <= S, top, left >= 0, top + rnd <= S and left + rnd <= S")
    return N, C, S, rnd, top, left


def di_resize_pad(x, y, rnd, top, left):
    """y ← D(x): every plane of x resized bilinearly (align_corners=False) to rnd × rnd and placed
    at (top, left) of a zero S × S plane — torchattacks input_diversity at a fixed image size
    (mia_di_resize_pad). x, y: distinct fp32 (N,C,S,S)."""
    N, C, S, rnd, top, left = _di_args(x, y, rnd, top, left, "x", "y")
    call("mia_di_resize_pad", ptr(x), ptr(y), N, C, S, rnd, top, left, stream())
    return y


def di_resize_pad_bwd_norms(g, gx, l1, l2sq, rnd, top, left, nonfinite=None):
    """gx ← Dᵀ g, the adjoint of di_resize_pad, with l1[n] += Σ|gx_n| and l2sq[n] += Σ gx_n²
    (either may be None) (mia_di_resize_pad_bwd_norms). g, gx: distinct fp32 (N,C,S,S)."""
    N, C, S, rnd, top, left = _di_args(g, gx, rnd, top, left, "g", "gx")
    _norm_outputs(N, l1, l2sq, nonfinite)
    call("mia_di_resize_pad_bwd_norms", ptr(g), ptr(gx), ptr(l1), ptr(l2sq), N, C, S, rnd, top,
         left, ptr(nonfinite), stream())
    return gx


def _jpeg_args(x, qtab, others):
    """Shared checks of the JPEG pair: x a non-empty fp32 (N,3,S,S) tensor with S % 8 == 0, qtab
    the (2,64) fp32 device table of quantiser steps (luminance, chrominance; natural order),
    ``others`` = (name, tensor) pairs of x's shape, all distinct buffers. Returns (N, S)."""
    if x is None or x.dim() != 4 or x.dtype != torch.float32 or x.numel() == 0 or x.shape[1] != 3:
        raise ValueError("x must be a non-empty fp32 (N,3,S,S) tensor")
    N, _, S, S2 = x.shape
    if S != S2 or S < 8 or S % 8:
        raise ValueError("x must have square planes (N,3,S,S) with S a multiple of 8")
    _need(qtab, (2, 64), torch.float32, "qtab")
    bufs = [x.data_ptr()]
    for name, t in others:
        _need(t, x.shape, torch.float32, name)
        bufs.append(t.data_ptr())
    if len(set(bufs)) != len(bufs):
        raise ValueError("x" + "".join(f", {name}" for name, _ in others)
                         + " must be distinct buffers")
    return N, S


def jpeg_roundtrip(x, y, qtab):
    """y ← J(x): what saving x as a baseline 4:4:4 JPEG with the quantiser steps ``qtab`` and
    loading it again does to it — 8-bit pixels, JFIF YCbCr, the 8 × 8 DCT, quantise / dequantise,
    the inverse DCT, RGB, 8-bit pixels (mia_jpeg_roundtrip; the order of every fp32 operation is
    in include/miattack.h). x, y: distinct fp32 (N,3,S,S) in [-1,1], S % 8 == 0; qtab: (2,64)
    fp32 on the device (pgd.jpeg_quant_tables)."""
    N, S = _jpeg_args(x, qtab, (("y", y),))
    call("mia_jpeg_roundtrip", ptr(x), ptr(y), ptr(qtab), N, S, stream())
    return y


def jpeg_bwd_norms(x, g, gx, qtab, l1, l2sq, nonfinite=None):
    """gx ← J′(x)ᵀ g, the adjoint at x of the round trip whose coefficient rounding is replaced by
    round(v) + (v − round(v))³ (Shin & Song 2017), with l1[n] += Σ|gx_n| and l2sq[n] += Σ gx_n²
    (either may be None) (mia_jpeg_bwd_norms). x, g, gx: distinct fp32 (N,3,S,S); qtab as in
    jpeg_roundtrip."""
    N, S = _jpeg_args(x, qtab, (("g", g), ("gx", gx)))
    _norm_outputs(N, l1, l2sq, nonfinite)
    call("mia_jpeg_bwd_norms", ptr(x), ptr(g), ptr(gx), ptr(qtab), ptr(l1), ptr(l2sq), N, S,
         ptr(nonfinite), stream())
    return gx


SI_MAX_SCALES = 8  # MIA_SI_MAX_SCALES


def _si_scale(s, name):
    """A scale 2^-i with 0 <= i < SI_MAX_SCALES, as a float."""
    if isinstance(s, bool) or not isinstance(s, numbers.Real):
        raise ValueError(f"{name} must be a number")
    s = float(s)
    if s not in [2.0 ** -i for i in range(SI_MAX_SCALES)]:
        raise ValueError(f"{name} must be 2^-i with 0 <= i < {SI_MAX_SCALES}")
    return s


def _si_images(x, y, xname, yname):
    """Shared checks of the scale-invariance pair: distinct non-empty fp32 batches of one shape.
    Returns (N, elements per image)."""
    if x is None or x.dim() < 2 or x.dtype != torch.float32 or x.numel() == 0:
        raise ValueError(f"{xname} must be a non-empty fp32 batch of images")
    _need(y, x.shape, torch.float32, yname)
    if y.data_ptr() == x.data_ptr():
        raise ValueError(f"{xname} and {yname} must be distinct buffers")
    return x.shape[0], x.numel() // x.shape[0]


def si_transform(x, m, y, c, s):
    """y ← S(x + c·m): the Nesterov look-ahead (m None: none) followed by the scale copy
    S(t) = (t + 1)·s − 1 for s = 2^-i (s = 1: none) — torchattacks SINIFGSM's p / 2^i in [-1,1]
    units, towards black (mia_si_transform). x, y (and m): fp32 batches of one shape, y distinct
    from x and m."""
    N, plane = _si_images(x, y, "x", "y")
    if m is not None:
        _need(m, x.shape, torch.float32, "m")
        if m.data_ptr() == y.data_ptr():
            raise ValueError("m and y must be distinct buffers")
    c = _finite(c, "c")
    s = _si_scale(s, "s")
    call("mia_si_transform", ptr(x), ptr(m), ptr(y), N, plane, float(c), s, stream())
    return y


def si_accumulate_norms(g, acc, l1, l2sq, w, first, div=1.0, nonfinite=None):
    """acc ← (first ? w·g : acc + w·g) / div for w = 2^-i (div = 1: no division), with
    l1[n] += Σ|acc_n| and l2sq[n] += Σ acc_n² (either may be None) (mia_si_accumulate_norms).
    g, acc: distinct fp32 batches of one shape."""
    N, plane = _si_images(g, acc, "g", "acc")
    _norm_outputs(N, l1, l2sq, nonfinite)
    w = _si_scale(w, "w")
    div = _finite(div, "div", ">= 1")
    call("mia_si_accumulate_norms", ptr(g), ptr(acc), ptr(l1), ptr(l2sq), N, plane, w,
         1 if first else 0, float(div), ptr(nonfinite), stream())
    return acc


def _vt_u32(v, name):
    """A counter word of the variance-tuning noise: an integer in 0 … 2^32 − 1."""
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 0 <= v < 1 << 32:
        raise ValueError(f"{name} must be an integer in 0 … 2^32 − 1")
    return int(v)


def vt_neighbor(x, m, y, c, r, seed, image0, step, sample):
    """y ← (x + c·m) + r·u: one neighbour of the Nesterov look-ahead point (m None: of x) for the
    variance-tuned attack (torchattacks VMIFGSM), u in (−1, 1) from Philox4x32-10 with the key
    ``seed`` (0 … 2^64 − 1) and the counter (element index / 4, image0 + n, step, sample)
    (mia_vt_neighbor). Stateless: the noise of an element depends on (seed, global image index,
    step, sample, element index) only. x, y (and m): fp32 batches of one shape, y distinct from
    x and m; r finite and >= 0."""
    N, plane = _si_images(x, y, "x", "y")
    if m is not None:
        _need(m, x.shape, torch.float32, "m")
        if m.data_ptr() == y.data_ptr():
            raise ValueError("m and y must be distinct buffers")
    c = _finite(c, "c")
    r = _finite(r, "r", ">= 0")
    seed, image0, step, sample = _philox_counter(N, seed, image0, step, sample)
    call("mia_vt_neighbor", ptr(x), ptr(m), ptr(y), N, plane, c, r, seed, image0, step, sample,
         stream())
    return y


def vt_combine_norms(g, gv, v, gt, l1, nonfinite=None):
    """gt ← g + v (the old v) with l1[n] += Σ|gt_n| (l1 may be None), then v ← gv − g (gv None:
    v stays, the last step) — the tuned gradient and the next variance term of the variance-tuned
    attack in one pass (mia_vt_combine_norms). g, gv, v, gt: distinct fp32 batches of one shape."""
    N, plane = _si_images(g, gt, "g", "gt")
    _need(v, g.shape, torch.float32, "v")
    bufs = [("g", g), ("v", v), ("gt", gt)]
    if gv is not None:
        _need(gv, g.shape, torch.float32, "gv")
        bufs.append(("gv", gv))
    _distinct(bufs)
    _norm_outputs(N, l1, None, nonfinite)
    call("mia_vt_combine_norms", ptr(g), ptr(gv), ptr(v), ptr(gt), ptr(l1), N, plane,
         ptr(nonfinite), stream())
    return gt


def _philox_counter(N, seed, image0, step, sample):
    """The key and counter words of a counter-based launch (vt_neighbor, the SPSA pair)."""
    if isinstance(seed, bool) or not isinstance(seed, numbers.Integral) or not 0 <= seed < 1 << 64:
        raise ValueError("seed must be an integer in 0 … 2^64 − 1")
    image0, step, sample = (_vt_u32(v, nm) for v, nm in ((image0, "image0"), (step, "step"),
                                                         (sample, "sample")))
    if image0 + N > 1 << 32:
        raise ValueError("image0 + N must be <= 2^32")
    return int(seed), image0, step, sample


def _finite(v, name, bound=""):
    """v as a float: a finite real number (no bool) within ``bound`` ("", ">= 0", ">= 1", "> 0")."""
    ok = not isinstance(v, bool) and isinstance(v, numbers.Real) and math.isfinite(v)
    if not (ok and {"": True, ">= 0": v >= 0, ">= 1": v >= 1, "> 0": v > 0}[bound]):
        raise ValueError(f"{name} must be a finite number {bound}".rstrip())
    return float(v)


def spsa_probe(x, yp, ym, d, seed, image0, step, sample, lo=-1.0, hi=1.0):
    """yp ← clamp(x + d·v, lo, hi), ym ← clamp(x − d·v, lo, hi): the two probes of one antithetic
    SPSA pair in one pass, v = ±1 (Rademacher) from bit 31 of the Philox4x32-10 word with the key
    ``seed`` (0 … 2^64 − 1) and the counter (element index / 4, image0 + n, step, sample)
    (mia_spsa_probe). Stateless, as vt_neighbor. x, yp, ym: three distinct fp32 batches of one
    shape; d finite and > 0; lo <= hi."""
    N, plane = _si_images(x, yp, "x", "yp")
    _need(ym, x.shape, torch.float32, "ym")
    _distinct([("x", x), ("yp", yp), ("ym", ym)])
    d = _finite(d, "d", "> 0")
    if not float(lo) <= float(hi):
        raise ValueError("need lo <= hi")
    seed, image0, step, sample = _philox_counter(N, seed, image0, step, sample)
    call("mia_spsa_probe", ptr(x), ptr(yp), ptr(ym), N, plane, d, float(lo), float(hi), seed,
         image0, step, sample, stream())
    return yp, ym


def spsa_accumulate_norms(acc, fp, fm, l1, l2sq, s, seed, image0, step, sample, first, div=1.0,
                          nonfinite=None):
    """acc ← (first ? c·v : acc + c·v) / div with c = (fp[n] − fm[n])·s and the direction v of
    spsa_probe regenerated from the same counter (div = 1: no division), with l1[n] += Σ|acc_n|
    and l2sq[n] += Σ acc_n² (either may be None) (mia_spsa_accumulate_norms). acc: an fp32 batch;
    fp, fm: distinct fp32 (N,) device tensors, the objective at the two probes; s and div finite
    and > 0."""
    if acc is None or acc.dim() < 2 or acc.dtype != torch.float32 or acc.numel() == 0:
        raise ValueError("acc must be a non-empty fp32 batch of images")
    N, plane = acc.shape[0], acc.numel() // acc.shape[0]
    _need(fp, (N,), torch.float32, "fp")
    _need(fm, (N,), torch.float32, "fm")
    _distinct([("acc", acc), ("fp", fp), ("fm", fm)])
    _norm_outputs(N, l1, l2sq, nonfinite)
    s, div = _finite(s, "s", "> 0"), _finite(div, "div", "> 0")
    seed, image0, step, sample = _philox_counter(N, seed, image0, step, sample)
    call("mia_spsa_accumulate_norms", ptr(acc), ptr(fp), ptr(fm), ptr(l1), ptr(l2sq), N, plane, s,
         seed, image0, step, sample, 1 if first else 0, div, ptr(nonfinite), stream())
    return acc


UAP_MAX_ELEMENTS = 1 << 37  # mia_uap_accumulate: images × plane elements summed into one plane


def _uap_plane(t, dtype, name, plane=None):
    """A shared plane of the universal perturbation: a non-empty tensor of ``dtype`` (with
    ``plane`` elements, if given). Returns its element count."""
    if t is None or not torch.is_tensor(t) or t.dtype != dtype or t.numel() == 0:
        raise ValueError(f"{name} must be a non-empty {dtype} tensor")
    if plane is not None and t.numel() != plane:
        raise ValueError(f"{name}: numel {t.numel()} != {plane} (one plane)")
    return t.numel()


def uap_accumulate(g, l1, acc, first, nonfinite=None):
    """acc[j] ← (first ? 0 : acc[j]) + Σ_n rint(((−g[n][j]) / (l1[n]/plane))·2^24) as int64: the
    per-image normalised gradients (mi_update's normalisation) into the exact integer sum a
    universal perturbation steps along (mia_uap_accumulate). g: a non-empty fp32 batch of N ≤ 65535
    images; l1: fp32 (N,), Σ|g_n|; acc: int64, one plane; N·plane < 2^37. An element of the
    normalised gradient outside ±2·plane (NaN, ±Inf) marks nonfinite[n] and contributes 0."""
    if g is None or g.dim() < 2 or g.dtype != torch.float32 or g.numel() == 0:
        raise ValueError("g must be a non-empty fp32 batch of images")
    N, plane = g.shape[0], g.numel() // g.shape[0]
    _need(l1, (N,), torch.float32, "l1")
    _uap_plane(acc, torch.int64, "acc", plane)
    _numel_ok(nonfinite, N, torch.int32, "nonfinite")
    _distinct([("g", g), ("l1", l1), ("acc", acc)]
              + ([("nonfinite", nonfinite)] if nonfinite is not None else []))
    if N > 65535:
        raise ValueError("at most 65535 images per call")
    if N * plane >= UAP_MAX_ELEMENTS:
        raise ValueError("N * plane must be < 2^37 (the int64 sum's range)")
    call("mia_uap_accumulate", ptr(g), ptr(l1), ptr(acc), N, plane, 1 if first else 0,
         ptr(nonfinite), stream())
    return acc


def uap_step(delta, acc, x, x0, a, e, lo=-1.0, hi=1.0):
    """delta ← clamp(delta + a·sgn(acc), −e, e) (sgn(0) = 0), then x[n] ← clamp(x0[n] + delta, lo,
    hi) for every image, in one pass (mia_uap_step). acc None: delta is applied as it is. x and x0
    both None: delta is updated only (a rank with an empty shard; needs acc). delta: fp32, one
    plane; acc: int64, one plane; x, x0: distinct fp32 batches of one shape; a finite and >= 0,
    e finite and > 0, lo <= hi."""
    plane = _uap_plane(delta, torch.float32, "delta")
    if acc is not None:
        _uap_plane(acc, torch.int64, "acc", plane)
    if (x is None) != (x0 is None):
        raise ValueError("x and x0 must both be given or both be None")
    N = 0
    bufs = [("delta", delta)] + ([("acc", acc)] if acc is not None else [])
    if x0 is not None:
        N, per = _si_images(x0, x, "x0", "x")
        if per != plane:
            raise ValueError(f"x0: {per} elements per image != {plane} (delta's plane)")
        if N > 65535:
            raise ValueError("at most 65535 images per call")
        bufs += [("x", x), ("x0", x0)]
    elif acc is None:
        raise ValueError("nothing to do: no images and no acc")
    _distinct(bufs)
    for v, nm in ((a, "a"), (e, "e")):
        _finite(v, nm)
    if a < 0 or e <= 0:
        raise ValueError("need a >= 0 and e > 0")
    if not float(lo) <= float(hi):
        raise ValueError("need lo <= hi")
    call("mia_uap_step", ptr(delta), ptr(acc), ptr(x), ptr(x0), N, plane, float(a), float(e),
         float(lo), float(hi), stream())
    return delta


APGD_SAVE, APGD_RESTORE = 1, 2  # MIA_APGD_SAVE, MIA_APGD_RESTORE: the bits of an action word


def _distinct(bufs):
    """bufs: (name, tensor) pairs that must not share a base address."""
    for i, (na, a) in enumerate(bufs):
        for nb, b in bufs[i + 1:]:
            if a.data_ptr() == b.data_ptr():
                raise ValueError(f"{na} and {nb} must be distinct buffers")


def apgd_update(x, x_old, x0, g, eta, a, e, lo=-1.0, hi=1.0, nonfinite=None):
    """The Auto-PGD momentum step with the per-image step size eta[n] (mia_apgd_update):
    d = x − x_old; x_old ← x; z = clamp(min(max(x − eta·sign(g), x0 − e), x0 + e), lo, hi);
    x ← clamp(min(max((x + (z − x)·a) + d·(1 − a), x0 − e), x0 + e), lo, hi).
    x, x_old, x0, g: distinct fp32 batches of one shape; eta: fp32 [N]; a in (0, 1]."""
    N, plane = _si_images(x, x_old, "x", "x_old")
    _need(x0, x.shape, torch.float32, "x0")
    _need(g, x.shape, torch.float32, "g")
    _distinct([("x", x), ("x_old", x_old), ("x0", x0), ("g", g)])
    _need(eta, (N,), torch.float32, "eta")
    _numel_ok(nonfinite, N, torch.int32, "nonfinite")
    if isinstance(a, bool) or not isinstance(a, numbers.Real) or not 0.0 < a <= 1.0:
        raise ValueError("a must be a number in (0, 1]")
    e = _finite(e, "e", "> 0")
    if not float(lo) <= float(hi):
        raise ValueError("need lo <= hi")
    call("mia_apgd_update", ptr(x), ptr(x_old), ptr(x0), ptr(g), ptr(eta), N, plane, float(a),
         float(e), float(lo), float(hi), ptr(nonfinite), stream())
    return x


def apgd_decide(loss, fstate, istate, action, hist_loss, hist_eta, step, checkpoint=False, thr=0,
                eta0=None):
    """The per-image step-size control of Auto-PGD on loss[n] (mia_apgd_decide). fstate: fp32
    (4, N) rows eta, L_best, L_prev, L_check; istate: int32 (3, N) rows n_dec, reduced,
    best_step; action: int32 [N], overwritten with APGD_SAVE / APGD_RESTORE bits; hist_loss,
    hist_eta: fp32 (rows, N) histories whose row ``step`` receives (loss, eta after the step).
    step = 0 is the start (needs eta0, no checkpoint); step = i + 1 follows update i, a
    checkpoint with the integer threshold ``thr``."""
    if loss is None or loss.dim() != 1 or loss.dtype != torch.float32 or loss.numel() == 0:
        raise ValueError("loss must be a non-empty 1-D fp32 tensor")
    N = loss.numel()
    _need(fstate, (4, N), torch.float32, "fstate")
    _need(istate, (3, N), torch.int32, "istate")
    _need(action, (N,), torch.int32, "action")
    for v, nm in ((step, "step"), (thr, "thr")):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 0 <= v < 1 << 31:
            raise ValueError(f"{nm} must be an integer in 0 … 2^31 − 1")
    step, thr = int(step), int(thr)
    if not isinstance(checkpoint, (bool, int)) or checkpoint not in (0, 1):
        raise ValueError("checkpoint must be True or False")
    for h, nm in ((hist_loss, "hist_loss"), (hist_eta, "hist_eta")):
        if h is None or h.dim() != 2 or h.dtype != torch.float32 or h.shape[1] != N:
            raise ValueError(f"{nm} must be an fp32 (rows, N) tensor")
        if not step < h.shape[0]:
            raise ValueError(f"{nm} has no row {step}")
    _distinct([("loss", loss), ("fstate", fstate), ("hist_loss", hist_loss),
               ("hist_eta", hist_eta)])
    if step == 0:
        if checkpoint:
            raise ValueError("the start (step 0) is no checkpoint")
        if (isinstance(eta0, bool) or not isinstance(eta0, numbers.Real)
                or not math.isfinite(eta0) or eta0 <= 0):
            raise ValueError("the start (step 0) needs a finite eta0 > 0")
    call("mia_apgd_decide", ptr(loss), ptr(fstate), ptr(istate), ptr(action), ptr(hist_loss[step]),
         ptr(hist_eta[step]), N, step, int(checkpoint), thr, float(eta0) if step == 0 else 0.0,
         stream())
    return action


def apgd_apply(x, g, x_best, g_best, action):
    """The whole-image copies an action word asks for (mia_apgd_apply): APGD_SAVE: x_best ← x,
    g_best ← g; otherwise APGD_RESTORE: x ← x_best, g ← g_best; 0: the image is not touched.
    x, g, x_best, g_best: distinct fp32 batches of one shape; action: int32 [N]."""
    N, plane = _si_images(x, g, "x", "g")
    _need(x_best, x.shape, torch.float32, "x_best")
    _need(g_best, x.shape, torch.float32, "g_best")
    _distinct([("x", x), ("g", g), ("x_best", x_best), ("g_best", g_best)])
    _need(action, (N,), torch.int32, "action")
    call("mia_apgd_apply", ptr(x), ptr(g), ptr(x_best), ptr(g_best), ptr(action), N, plane,
         stream())
    return x


def _sh_range(r, plane, name):
    """A segment (lo, hi) of an image's elements, 0 <= lo <= hi <= plane; None is the empty one."""
    if r is None:
        return 0, 0
    try:
        lo, hi = r
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be None or a pair (lo, hi)") from None
    for v in (lo, hi):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise ValueError(f"{name} must hold integers")
    if not 0 <= lo <= hi <= plane:
        raise ValueError(f"{name}: need 0 <= lo <= hi <= {plane} (elements per image)")
    return int(lo), int(hi)


def sh_flip(x, x0, s, accept, prev, new, e, lo=-1.0, hi=1.0):
    """One SignHunter query's change of the iterate (mia_sh_flip): the sign plane s (int8, ±1) is
    flipped on the segment ``new`` = (lo, hi) of every image and flipped back on ``prev`` in the
    images with accept[n] == 0 (accept None: no image), and x = clamp(x0 + e·s, lo, hi) is
    rewritten on the union of the two segments only. x, x0: distinct fp32 batches of one shape; s:
    int8 of that shape; accept: int32 [N] or None; prev / new: (lo, hi) in elements of one image,
    or None for an empty segment (not both)."""
    N, plane = _si_images(x, x0, "x", "x0")
    _need(s, x.shape, torch.int8, "s")
    _numel_ok(accept, N, torch.int32, "accept")
    prev, new = _sh_range(prev, plane, "prev"), _sh_range(new, plane, "new")
    if prev[0] == prev[1] and new[0] == new[1]:
        raise ValueError("prev and new are both empty: nothing to do")
    e = _finite(e, "e", "> 0")
    if not float(lo) <= float(hi):
        raise ValueError("need lo <= hi")
    call("mia_sh_flip", ptr(x), ptr(x0), ptr(s), ptr(accept), N, plane, prev[0], prev[1], new[0],
         new[1], float(e), float(lo), float(hi), stream())
    return x


def sh_decide(loss, best, accept, n_accept, hist_loss, query, nonfinite=None):
    """The accept / reject decision of SignHunter's query ``query`` on loss[n] (mia_sh_decide).
    Query 0 initialises best = loss, accept = 1, n_accept = 0; a later query sets accept =
    loss < best and, where it holds, best = loss and n_accept += 1 (a tie, NaN or ±Inf: rejected;
    non-finite marks ``nonfinite``). best: fp32 [N]; accept, n_accept: int32 [N]; hist_loss: fp32
    (rows, N), whose row ``query`` receives the loss."""
    if loss is None or loss.dim() != 1 or loss.dtype != torch.float32 or loss.numel() == 0:
        raise ValueError("loss must be a non-empty 1-D fp32 tensor")
    N = loss.numel()
    _need(best, (N,), torch.float32, "best")
    _need(accept, (N,), torch.int32, "accept")
    _need(n_accept, (N,), torch.int32, "n_accept")
    _numel_ok(nonfinite, N, torch.int32, "nonfinite")
    if isinstance(query, bool) or not isinstance(query, numbers.Integral) or query < 0:
        raise ValueError("query must be an integer >= 0")
    if (hist_loss is None or hist_loss.dim() != 2 or hist_loss.dtype != torch.float32
            or hist_loss.shape[1] != N):
        raise ValueError("hist_loss must be an fp32 (rows, N) tensor")
    if not query < hist_loss.shape[0]:
        raise ValueError(f"hist_loss has no row {query}")
    _distinct([("loss", loss), ("best", best), ("hist_loss", hist_loss)])
    _distinct([("accept", accept), ("n_accept", n_accept)])
    call("mia_sh_decide", ptr(loss), ptr(best), ptr(accept), ptr(n_accept),
         ptr(hist_loss[int(query)]), N, 1 if query == 0 else 0, ptr(nonfinite), stream())
    return accept


PI_MAX_KERNEL = 15  # mia_pi_update


def pi_update(x, x0, g, l1, m_in, m_out, A_in, A_out, mu, ab, gm, e, kernel, lo=-1.0, hi=1.0,
              nonfinite=None):
    """The patch-wise attack's step (PI-FGSM, mia_pi_update), per plane of x (N,C,H,W):
    m' = (−g)/(l1[n]/plane) + mu·m_in; s = sign(m'); A' = A_in + ab·s;
    Cut = sign(A')·max(|A'| − e, 0); S = the sum of Cut over the kernel × kernel window without
    its centre (zero padded; dy outer, dx inner, ascending); p = gm·sign(S); A_out = A' + p;
    x ← clamp(x0 + clamp(x + ab·s + p − x0, −e, e), lo, hi); m_out = m'.
    x, x0, g, m_in, m_out, A_in, A_out: distinct fp32 (N,C,H,W) tensors (m and A ping-pong: the
    caller swaps in and out every step); l1: fp32 [N]; kernel odd in 3 … 15; mu, ab, gm, e finite
    and >= 0. Returns x."""
    if x is None or x.dim() != 4 or x.dtype != torch.float32 or x.numel() == 0:
        raise ValueError("x must be a non-empty fp32 (N,C,H,W) tensor")
    N, C, H, W = x.shape
    bufs = [("x", x), ("x0", x0), ("g", g), ("m_in", m_in), ("m_out", m_out), ("A_in", A_in),
            ("A_out", A_out)]
    for nm, b in bufs[1:]:
        _need(b, x.shape, torch.float32, nm)
    _distinct(bufs)
    _need(l1, (N,), torch.float32, "l1")
    _numel_ok(nonfinite, N, torch.int32, "nonfinite")
    if (isinstance(kernel, bool) or not isinstance(kernel, numbers.Integral)
            or kernel % 2 == 0 or not 3 <= kernel <= PI_MAX_KERNEL):
        raise ValueError(f"kernel must be an odd integer in 3 … {PI_MAX_KERNEL}")
    for v, nm in ((mu, "mu"), (ab, "ab"), (gm, "gm"), (e, "e")):
        _finite(v, nm, ">= 0")
    if not float(lo) <= float(hi):
        raise ValueError("need lo <= hi")
    call("mia_pi_update", ptr(x), ptr(x0), ptr(g), ptr(l1), ptr(m_in), ptr(m_out), ptr(A_in),
         ptr(A_out), N, C, H, W, int(kernel), float(mu), float(ab), float(gm), float(e), float(lo),
         float(hi), ptr(nonfinite), stream())
    return x


def fill_bytes_(t, value):
    """Every byte of t ← value (0 … 255), on the stream (mia_memset)."""
    call("mia_memset", ptr(t), int(value) & 0xFF, t.numel() * t.element_size(), stream())
    return t


def cw_init(x, w):
    _need(w, x.shape, torch.float32, "w")
    call("mia_cw_init", ptr(x), ptr(w), x.numel(), stream())
    return w


def cw_tanh(w, adv):
    _need(adv, w.shape, torch.float32, "adv")
    call("mia_cw_tanh", ptr(w), ptr(adv), w.numel(), stream())
    return adv


def cw_grad(adv, x, g_f, g_w, c, scale=1.0):
    for name, t in (("x", x), ("g_f", g_f), ("g_w", g_w)):
        _need(t, adv.shape, torch.float32, name)
    call("mia_cw_grad", ptr(adv), ptr(x), ptr(g_f), ptr(g_w), adv.numel(), float(c), float(scale),
         stream())
    return g_w


def cw_select(adv, best_adv, sq, best_l2, f, f0, l2_scale):
    N = adv.shape[0]
    _need(best_adv, adv.shape, torch.float32, "best_adv")
    for name, t in (("sq", sq), ("best_l2", best_l2), ("f", f), ("f0", f0)):
        _numel_ok(t, N, torch.float32, name)
    call("mia_cw_select", ptr(adv), ptr(best_adv), ptr(sq), ptr(best_l2), ptr(f), ptr(f0), N,
         adv.numel() // N, float(l2_scale), stream())
    return best_adv


def random_start(x, x0, u, e, lo=-1.0, hi=1.0):
    _need(x0, x.shape, torch.float32, "x0")
    _need(u, x.shape, torch.float32, "u")
    call("mia_random_start", ptr(x), ptr(x0), ptr(u), x.numel(), float(e), float(lo), float(hi),
         stream())
    return x


def sign_project(x, x0, g, a, e, lo=-1.0, hi=1.0):
    _need(x0, x.shape, torch.float32, "x0")
    _need(g, x.shape, torch.float32, "g")
    call("mia_sign_project", ptr(x), ptr(x0), ptr(g), x.numel(), float(a), float(e), float(lo),
         float(hi), stream())
    return x


def adam_step(p, g, m, v, lr, beta1, beta2, eps, t):
    for name, z in (("g", g), ("m", m), ("v", v)):
        _need(z, p.shape, torch.float32, name)
    call("mia_adam_step", ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), float(lr), float(beta1),
         float(beta2), float(eps), int(t), stream())
    return p


def patch_update(patch, g, img, mask, adv, lo, hi):
    """adversarial_patch.py:131-134: patch −= g (g None: composite only); adv ← clamp((1−m)·img +
    m·patch, lo, hi). patch / mask: img's shape, or one image's shape (composite only)."""
    _need(adv, img.shape, torch.float32, "adv")
    _need(img, img.shape, torch.float32, "img")
    full = patch.numel() == img.numel()
    if not full and (g is not None or img.numel() % patch.numel()):
        raise ValueError("patch / mask: img's shape, or one image's shape for the composite")
    _need(mask, patch.shape, torch.float32, "mask")
    if g is not None:
        _need(g, img.shape, torch.float32, "g")
    call("mia_patch_update", ptr(patch), ptr(g) if g is not None else None, ptr(img), ptr(mask),
         ptr(adv), img.numel(), 0 if full else patch.numel(), float(lo), float(hi), stream())
    return adv


def gemm(M, N, K, alpha, A, sam, sak, B, sbk, sbn, beta, C, scm, scn, bias=None):
    """C[m,n] = alpha Σ_k A[m*sam+k*sak] B[k*sbk+n*sbn] + beta C[m*scm+n*scn] + bias[n] (fp32).
    Offsets into A/B/C are given by passing views (data_ptr of a strided view is honoured)."""
    for name, t, span in (("A", A, (M - 1) * sam + (K - 1) * sak),
                          ("B", B, (K - 1) * sbk + (N - 1) * sbn),
                          ("C", C, (M - 1) * scm + (N - 1) * scn)):
        if t.dtype != torch.float32 or not t.is_cuda:
            raise ValueError(f"gemm {name}: cuda fp32 required")
        avail = t.untyped_storage().nbytes() // 4 - t.storage_offset()
        if span >= avail:
            raise ValueError(f"gemm {name}: strided span {span} exceeds storage {avail}")
    _numel_ok(bias, N, torch.float32, "bias")
    c = ctypes.c_void_p
    call("mia_gemm_f32", M, N, K, float(alpha), c(A.data_ptr()), sam, sak, c(B.data_ptr()), sbk,
         sbn, float(beta), c(C.data_ptr()), scm, scn, ptr(bias), stream())
    return C


def _span_ok(name, t, span):
    if t.dtype != torch.float32 or not t.is_cuda:
        raise ValueError(f"gemm {name}: cuda fp32 required")
    avail = t.untyped_storage().nbytes() // 4 - t.storage_offset()
    if span >= avail:
        raise ValueError(f"gemm {name}: strided span {span} exceeds storage {avail}")


class GemmPlan:
    """A validated, reusable list of grouped-GEMM descriptors (mia_gemm_f32_grouped).

    ``add(C, scm, scn, M, N, segs, alpha, beta, bias)`` with ``segs`` = [(A, sam, sak, B, sbk,
    sbn, K), ...] (≤ 2). Tensors are kept alive by the plan; the descriptor array is built once
    and launched by ``run()`` (the buffers are workspace-resident, so the pointers are stable)."""

    def __init__(self):
        self.groups = []
        self._keep = []
        self._arr = None

    def add(self, C, scm, scn, M, N, segs, alpha=1.0, beta=0.0, bias=None):
        if not 1 <= len(segs) <= 2:
            raise ValueError("1 or 2 segments per group")
        _span_ok("C", C, (M - 1) * scm + (N - 1) * scn)
        _numel_ok(bias, N, torch.float32, "bias")
        g = _lib.GemmGroup()
        g.C, g.bias = C.data_ptr(), (bias.data_ptr() if bias is not None else None)
        g.scm, g.scn, g.M, g.N = scm, scn, M, N
        g.alpha, g.beta, g.nseg = float(alpha), float(beta), len(segs)
        for i, (A, sam, sak, B, sbk, sbn, K) in enumerate(segs):
            _span_ok("A", A, (M - 1) * sam + (K - 1) * sak)
            _span_ok("B", B, (K - 1) * sbk + (N - 1) * sbn)
            g.seg[i] = _lib.GemmSeg(A.data_ptr(), B.data_ptr(), sam, sak, sbk, sbn, K)
            self._keep += [A, B]
        self._keep += [C] + ([bias] if bias is not None else [])
        self.groups.append(g)
        self._arr = None

    def run(self):
        if not self.groups:
            return
        if self._arr is None:
            self._arr = (_lib.GemmGroup * len(self.groups))(*self.groups)
        call("mia_gemm_f32_grouped", self._arr, len(self.groups), stream())


def style_demod(s, wsq, demod, scale2=1.0):
    N, Cin = s.shape
    Cout = wsq.shape[0]
    _need(wsq, (Cout, Cin), torch.float32, "wsq")
    _need(demod, (N, Cout), torch.float32, "demod")
    call("mia_style_demod", ptr(s), ptr(wsq), ptr(demod), N, Cin, Cout, float(scale2), stream())
    return demod


def demod_bwd(q, demod, wsq, s, gs, scale2=1.0):
    N, Cin = s.shape
    Cout = wsq.shape[0]
    _need(q, (N, Cout), torch.float32, "q")
    _need(demod, (N, Cout), torch.float32, "demod")
    _need(gs, (N, Cin), torch.float32, "gs")
    call("mia_demod_bwd", ptr(q), ptr(demod), ptr(wsq), ptr(s), ptr(gs), N, Cin, Cout,
         float(scale2), stream())
    return gs


def repeat(src, dst, count):
    if dst.numel() != src.numel() * count or dst.dtype != src.dtype:
        raise ValueError("repeat: size mismatch")
    call("mia_repeat", ptr(src), ptr(dst), src.numel() * src.element_size(), count, stream())
    return dst


def pixel_norm(x, y, eps=1e-8):
    rows, cols = x.shape
    _need(y, x.shape, torch.float32, "y")
    call("mia_pixel_norm", ptr(x), ptr(y), rows, cols, float(eps), stream())
    return y


def truncate(w, mean, psi, out):
    cols = w.shape[-1]
    rows = w.numel() // cols
    _need(out, w.shape, torch.float32, "out")
    _numel_ok(mean, cols, torch.float32, "mean")
    call("mia_truncate", ptr(w), ptr(mean), float(psi), ptr(out), rows, cols, stream())
    return out


def zero_(t):
    call("mia_memset", ptr(t), 0, t.numel() * t.element_size(), stream())
    return t


# ---- general-geometry conv and the e4e encoder kernels (csrc/encoder.hip) ----------------------
def conv2d_kpad(taps, cin, dtype):
    bk = 32 if dtype == torch.float32 else 64
    return (taps * cin + bk - 1) // bk * bk


def conv2d(x, groups, y, out_hw, *, cout, stride=1, bias=None, act_out=ACT_NONE, act_slope=None,
           mask_a=None, mask_slope=None, csum=None, accumulate=False, out_scale=None, flops=None):
    """mia_conv2d: 1..4 problems over x (N,H,W,Cin) sharing one epilogue. ``groups``: list of
    dict(w, kh, kw, pad=(py,px), ho, wo, a=(ay,ax), b=(by,bx)); w is [Cout][conv2d_kpad(kh·kw,
    Cin)]. y: (N, out_h, out_w, Cout). mask_a lives on y's pixel grid."""
    N, H, W, Cin = x.shape
    T = x.dtype
    oh, ow = out_hw
    if Cin % VEC[T]:
        raise ValueError("Cin must be a multiple of the 16-byte vector")
    if not 1 <= len(groups) <= 4:
        raise ValueError("1..4 groups")
    _need(y, (N, oh, ow, cout), T, "y")
    f32 = torch.float32
    _numel_ok(bias, cout, f32, "bias")
    _numel_ok(act_slope, cout, f32, "act_slope")
    _numel_ok(mask_slope, cout, f32, "mask_slope")
    _numel_ok(csum, N * cout, f32, "csum")
    _numel_ok(out_scale, N * cout, f32, "out_scale")
    if mask_a is not None:
        _need(mask_a, (N, oh, ow, cout), T, "mask_a")
    if act_out == ACT_PRELU and act_slope is None:
        raise ValueError("ACT_PRELU needs act_slope")
    garr = (_lib.ConvGroup * len(groups))()
    keep = []
    mac = 0
    for i, g in enumerate(groups):
        kh, kw = g["kh"], g["kw"]
        _need(g["w"], (cout, conv2d_kpad(kh * kw, Cin, T)), T, f"w[{i}]")
        py, px = g.get("pad", (0, 0))
        ay, ax = g.get("a", (1, 1))
        by, bx = g.get("b", (0, 0))
        ho, wo = g["ho"], g["wo"]
        if ho <= 0 or wo <= 0 or ay * (ho - 1) + by >= oh or ax * (wo - 1) + bx >= ow:
            raise ValueError(f"group {i}: placement outside the output grid")
        wsp = layouts.split_for(g["w"]) if T == torch.float32 else None
        garr[i] = _lib.ConvGroup(ptr(g["w"]).value, kh, kw, py, px, ho, wo, ay, by, ax, bx,
                                 ptr(wsp).value if wsp is not None else None)
        keep.append(g["w"])
        keep.append(wsp)
        mac += N * ho * wo * kh * kw * Cin * cout
    a = ConvArgs()
    a.x, a.y = ptr(x), ptr(y)
    a.N, a.H, a.W, a.Cin, a.Cout = N, H, W, Cin, cout
    a.bias, a.out_scale = ptr(bias), ptr(out_scale)
    a.act_out, a.act_slope = act_out, ptr(act_slope)
    a.mask_a, a.mask_slope, a.csum = ptr(mask_a), ptr(mask_slope), ptr(csum)
    a.accumulate = int(bool(accumulate))
    prof = PROFILE
    if prof is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    call("mia_conv2d", ctypes.byref(a), int(stride), garr, len(groups), oh, ow, dt(T), stream())
    if prof is not None:
        e1.record()
        prof.append((e0, e1, flops if flops is not None else 2 * mac))
        _tag(f"conv2d {H}x{W} {Cin}->{cout} s{stride} g{len(groups)} k{groups[0]['kh']}"
             + (" mask" if mask_a is not None else "") + (" acc" if accumulate else ""))
    return y


def conv2d_batched(x, groups, y, out_hw, *, n, cout, stride=1, bias=None, act_out=ACT_NONE,
                   act_slope=None, mask_a=None, mask_slope=None, accumulate=False, flops=None):
    """mia_conv2d_batched: up to 16 independent convs of one launch. x (Sx·n, H, W, Cin) and y
    (Sy·n, out_h, out_w, Cout) hold the groups' images stacked along N; each group dict is as in
    conv2d plus n_in / n_out (first input / output image) and c_off (channel offset into the
    concatenated per-channel operands bias, act_slope, mask_slope). mask_a lives on y's grid."""
    _, H, W, Cin = x.shape
    T = x.dtype
    oh, ow = out_hw
    if Cin % VEC[T]:
        raise ValueError("Cin must be a multiple of the 16-byte vector")
    if not 1 <= len(groups) <= 16:
        raise ValueError("1..16 groups")
    if y.dim() != 4 or tuple(y.shape[1:]) != (oh, ow, cout) or y.dtype != T:
        raise ValueError(f"y: (S·n, {oh}, {ow}, {cout}) {T} required")
    if mask_a is not None and (mask_a.shape != y.shape or mask_a.dtype != T):
        raise ValueError("mask_a must match y")
    if act_out == ACT_PRELU and act_slope is None:
        raise ValueError("ACT_PRELU needs act_slope")
    garr = (_lib.ConvGroup * len(groups))()
    barr = (_lib.ConvBatch * len(groups))()
    keep = []
    mac = 0
    for i, g in enumerate(groups):
        kh, kw = g["kh"], g["kw"]
        _need(g["w"], (cout, conv2d_kpad(kh * kw, Cin, T)), T, f"w[{i}]")
        py, px = g.get("pad", (0, 0))
        ay, ax = g.get("a", (1, 1))
        by, bx = g.get("b", (0, 0))
        ho, wo = g["ho"], g["wo"]
        if ho <= 0 or wo <= 0 or ay * (ho - 1) + by >= oh or ax * (wo - 1) + bx >= ow:
            raise ValueError(f"group {i}: placement outside the output grid")
        n_in, n_out, c_off = g.get("n_in", 0), g.get("n_out", 0), g.get("c_off", 0)
        if n_in < 0 or n_in + n > x.shape[0] or n_out < 0 or n_out + n > y.shape[0]:
            raise ValueError(f"group {i}: image range outside x / y")
        if c_off % 8:
            raise ValueError(f"group {i}: c_off must be a multiple of 8")
        for name, t in (("bias", bias), ("act_slope", act_slope), ("mask_slope", mask_slope)):
            if t is not None and (t.dtype != torch.float32 or t.numel() < c_off + cout):
                raise ValueError(f"group {i}: {name} shorter than c_off + cout")
        wsp = layouts.split_for(g["w"]) if T == torch.float32 else None
        garr[i] = _lib.ConvGroup(ptr(g["w"]).value, kh, kw, py, px, ho, wo, ay, by, ax, bx,
                                 ptr(wsp).value if wsp is not None else None)
        barr[i] = _lib.ConvBatch(n_in, n_out, c_off)
        keep += [g["w"], wsp]
        mac += n * ho * wo * kh * kw * Cin * cout
    a = ConvArgs()
    a.x, a.y = ptr(x), ptr(y)
    a.N, a.H, a.W, a.Cin, a.Cout = n, H, W, Cin, cout
    a.bias = ptr(bias)
    a.act_out, a.act_slope = act_out, ptr(act_slope)
    a.mask_a, a.mask_slope = ptr(mask_a), ptr(mask_slope)
    a.accumulate = int(bool(accumulate))
    prof = PROFILE
    if prof is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    call("mia_conv2d_batched", ctypes.byref(a), int(stride), garr, barr, len(groups), oh, ow, dt(T),
         stream())
    if prof is not None:
        e1.record()
        prof.append((e0, e1, flops if flops is not None else 2 * mac))
        _tag(f"conv2d_batched {H}x{W} {Cin}->{cout} s{stride} x{len(groups)} k{groups[0]['kh']}"
             + (" mask" if mask_a is not None else "") + (" acc" if accumulate else ""))
    return y


def conv2d_planes(x, w, b, y, out_hw, *, planes, act_out=ACT_NONE, act_slope=None, flops=None):
    """mia_conv2d_planes: one stride-2 pad-1 3×3 conv over x (N,H,W,Cin) with Cout = planes·C
    (w: [planes·C][Kpad], the heads' matrices concatenated along Cout; b: planes·C), output
    plane p (channels p·C … p·C+C−1) written to y[p·N:(p+1)·N] of y (planes·N, oh, ow, C)."""
    N, H, W, Cin = x.shape
    T = x.dtype
    oh, ow = out_hw
    P = int(planes)
    C = y.shape[-1]
    cout = P * C
    _need(y, (P * N, oh, ow, C), T, "y")
    _need(w, (cout, conv2d_kpad(9, Cin, T)), T, "w")
    _numel_ok(b, cout, torch.float32, "b")
    if act_out == ACT_PRELU and (act_slope is None or act_slope.numel() < cout):
        raise ValueError("ACT_PRELU needs act_slope of Cout entries")
    wsp = layouts.split_for(w) if T == torch.float32 else None
    g = _lib.ConvGroup(ptr(w).value, 3, 3, 1, 1, oh, ow, 1, 0, 1, 0,
                       ptr(wsp).value if wsp is not None else None)
    a = ConvArgs()
    a.x, a.y = ptr(x), ptr(y)
    a.N, a.H, a.W, a.Cin, a.Cout = N, H, W, Cin, cout
    a.y_cstride = C
    a.bias = ptr(b)
    a.act_out, a.act_slope = act_out, ptr(act_slope)
    prof = PROFILE
    if prof is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    call("mia_conv2d_planes", ctypes.byref(a), 2, ctypes.byref(g), oh, ow, C, N * oh * ow * C,
         dt(T), stream())
    if prof is not None:
        e1.record()
        prof.append((e0, e1, flops if flops is not None else 2 * N * oh * ow * 9 * Cin * cout))
        _tag(f"conv2d_planes {H}x{W} {Cin}->{C} s2 x{P}")
    return y


def se_fwd(csum, w1, w2, u, s, hw):
    N, C = csum.shape
    Cr = w1.shape[0]
    _need(w1, (Cr, C), torch.float32, "w1")
    _need(w2, (C, Cr), torch.float32, "w2")
    _need(u, (N, Cr), torch.float32, "u")
    _need(s, (N, C), torch.float32, "s")
    call("mia_se_fwd", ptr(csum), ptr(w1), ptr(w2), ptr(u), ptr(s), N, C, Cr, 1.0 / hw, stream())
    return s


def _parts_ok(part, N, hw, C):
    nch = chan_sum_parts(N, hw)
    if part.dtype != torch.float32 or part.numel() < N * nch * C:
        raise ValueError("SE partials: fp32 scratch of N · chan_sum_parts · C floats")
    return nch


def se_fwd_parts(part, hw, w1, w2, u, s):
    """se_fwd from chan_sum's partials (chan_sum(..., out=None)): the pool sum is finished inside
    the SE kernel in the same chunk order (mia_se_fwd_parts, bit-identical, one launch fewer)."""
    N, C = s.shape
    Cr = w1.shape[0]
    _need(w1, (Cr, C), torch.float32, "w1")
    _need(w2, (C, Cr), torch.float32, "w2")
    _need(u, (N, Cr), torch.float32, "u")
    nch = _parts_ok(part, N, hw, C)
    call("mia_se_fwd_parts", ptr(part), nch, ptr(w1), ptr(w2), ptr(u), ptr(s), N, C, Cr, 1.0 / hw,
         stream())
    return s


def se_bwd_parts(part, hw, s, u, w1, w2, gavg):
    """se_bwd from chan_sum's partials of gs = Σ ∂out·r (mia_se_bwd_parts)."""
    N, C = s.shape
    Cr = w1.shape[0]
    _need(u, (N, Cr), torch.float32, "u")
    _need(gavg, (N, C), torch.float32, "gavg")
    nch = _parts_ok(part, N, hw, C)
    call("mia_se_bwd_parts", ptr(part), nch, ptr(s), ptr(u), ptr(w1), ptr(w2), ptr(gavg), N, C,
         Cr, 1.0 / hw, stream())
    return gavg


def se_apply(r, s, sc, ss, out, g=None, b=None, xb=None):
    """out = r·s + sc (sc read at stride ss), xb = out·g + b (either output may be None)."""
    N, H, W, C = r.shape
    _numel_ok(s, N * C, torch.float32, "s")
    if sc is not None:
        _need(sc, (N, H * ss, W * ss, C), r.dtype, "sc")
    if out is not None:
        _need(out, r.shape, r.dtype, "out")
    if xb is not None:
        _need(xb, r.shape, r.dtype, "xb")
        _numel_ok(g, C, torch.float32, "g")
        _numel_ok(b, C, torch.float32, "b")
    call("mia_se_apply", ptr(r), ptr(s), ptr(sc), int(ss), ptr(out), ptr(g), ptr(b), ptr(xb), N,
         H, W, C, dt(r), stream())
    return out if out is not None else xb


def _chan_vec_ok(C, name):
    # the rule of mia_chan_dot / mia_chan_sum (csrc/encoder.hip: ENC_CHECK_C and C ≤ 2048), checked
    # here so that a bad channel count is a ValueError like the other shape errors; keep in step
    if C <= 0 or C % 8 or C > 2048:
        raise ValueError(f"{name}: C = {C} must be a multiple of 8, at most 2048")


def chan_dot(a, b, gs, accumulate=False):
    N, H, W, C = a.shape
    _chan_vec_ok(C, "chan_dot")
    _need(b, a.shape, a.dtype, "b")
    _need(gs, (N, C), torch.float32, "gs")
    call("mia_chan_dot", ptr(a), ptr(b), ptr(gs), N, H * W, C, int(bool(accumulate)), dt(a),
         stream())
    return gs


def chan_sum_parts(N, HW):
    """Chunks per image of mia_chan_sum (host-side helper of the library, no device work)."""
    return _lib.load().mia_chan_sum_parts(int(N), int(HW))


def chan_sum(a, b, part, out, accumulate=False):
    """mia_chan_sum: out (N, C) fp32 (+)= Σ_pixels a·b (b given) or Σ_pixels a, deterministic;
    part: fp32 scratch of N · chan_sum_parts(N, H·W) · C floats. out None: only the ordered
    per-chunk partials (for se_fwd_parts / se_bwd_parts); returns part then."""
    N, H, W, C = a.shape
    _chan_vec_ok(C, "chan_sum")
    if b is not None:
        _need(b, a.shape, a.dtype, "b")
    if out is not None:
        _need(out, (N, C), torch.float32, "out")
    elif accumulate:
        raise ValueError("chan_sum: accumulate needs out")
    if part.dtype != torch.float32 or part.numel() < N * chan_sum_parts(N, H * W) * C:
        raise ValueError("chan_sum: part scratch too small")
    call("mia_chan_sum", ptr(a), ptr(b), ptr(part), ptr(out), N, H * W, C,
         int(bool(accumulate)), dt(a), stream())
    return out if out is not None else part


def se_bwd(gs, s, u, w1, w2, gavg, hw):
    N, C = s.shape
    Cr = w1.shape[0]
    _need(gs, (N, C), torch.float32, "gs")
    _need(u, (N, Cr), torch.float32, "u")
    _need(gavg, (N, C), torch.float32, "gavg")
    call("mia_se_bwd", ptr(gs), ptr(s), ptr(u), ptr(w1), ptr(w2), ptr(gavg), N, C, Cr, 1.0 / hw,
         stream())
    return gavg


def se_grad_scale(g_out, s, gavg, g_r, gamma=None):
    N, H, W, C = g_out.shape
    _need(g_r, g_out.shape, g_out.dtype, "g_r")
    _numel_ok(gamma, C, torch.float32, "gamma")
    call("mia_se_grad_scale", ptr(g_out), ptr(s), ptr(gavg), ptr(gamma), ptr(g_r), N, H * W, C,
         dt(g_out), stream())
    return g_r


def prelu_bwd_scale(g_a, a, slope, g, gamma=None):
    C = g_a.shape[-1]
    _need(a, g_a.shape, g_a.dtype, "a")
    _need(g, g_a.shape, g_a.dtype, "g")
    _numel_ok(slope, C, torch.float32, "slope")
    _numel_ok(gamma, C, torch.float32, "gamma")
    call("mia_prelu_bwd_scale", ptr(g_a), ptr(a), ptr(slope), ptr(gamma), ptr(g),
         g_a.numel() // C, C, dt(g_a), stream())
    return g


def prelu_fwd(pre, slope, a):
    """a = pre > 0 ? pre : slope[c]·pre (NHWC, per-channel fp32 slope)."""
    C = pre.shape[-1]
    _need(a, pre.shape, pre.dtype, "a")
    _numel_ok(slope, C, torch.float32, "slope")
    call("mia_prelu_fwd", ptr(pre), ptr(slope), ptr(a), pre.numel() // C, C, dt(pre), stream())
    return a


def subsample_add(g, gx):
    N, H, W, C = g.shape
    _need(gx, (N, 2 * H, 2 * W, C), g.dtype, "gx")
    call("mia_subsample_add", ptr(g), ptr(gx), N, H, W, C, dt(g), stream())
    return gx


def bilinear_fwd(x, y, accumulate=False):
    N, Hi, Wi, C = x.shape
    _, Ho, Wo, C2 = y.shape
    if y.shape[0] != N or C2 != C or y.dtype != x.dtype:
        raise ValueError("bilinear_fwd: shape/dtype mismatch")
    call("mia_bilinear_fwd", ptr(x), ptr(y), N, Hi, Wi, Ho, Wo, C, int(bool(accumulate)), dt(x),
         stream())
    return y


def bilinear_bwd(gy, gx, accumulate=False):
    N, Ho, Wo, C = gy.shape
    _, Hi, Wi, C2 = gx.shape
    if gx.shape[0] != N or C2 != C or gx.dtype != gy.dtype:
        raise ValueError("bilinear_bwd: shape/dtype mismatch")
    call("mia_bilinear_bwd", ptr(gy), ptr(gx), N, Hi, Wi, Ho, Wo, C, int(bool(accumulate)),
         dt(gy), stream())
    return gx


def cast(x, y, scale=1.0):
    if x.numel() != y.numel():
        raise ValueError("cast: size mismatch")
    call("mia_cast", ptr(x), dt(x), ptr(y), dt(y), x.numel(), float(scale), stream())
    return y


def s2_dgrad_halo(g, w_halo, gx, mask_a=None, mask_slope=None, accumulate=False, flops=None):
    """mia_conv_s2_dgrad_halo(_multi): gx (N,2R,2R,Cx) ← input gradient of a stride-2 3×3 conv from
    g (N,R,R,Cg) (+ slope mask, + accumulate). ``g`` may be a list of up to 8 output gradients of
    convs reading the same tensor, with ``w_halo`` their packed matrices concatenated along dim 0:
    the sum of their input gradients in one K loop. fp32 passes the split_f32 copy of w_halo (the
    split-once kernel takes long K loops)."""
    gs = list(g) if isinstance(g, (list, tuple)) else [g]
    if not 1 <= len(gs) <= 8:
        raise ValueError("s2_dgrad_halo: 1..8 source gradients")
    N, R, R2, Cg = gs[0].shape
    for t in gs[1:]:
        _need(t, gs[0].shape, gs[0].dtype, "g[i]")
    Cx = gx.shape[-1]
    T = gs[0].dtype
    if R != R2:
        raise ValueError("square inputs only")
    bk = layouts.halo_bk(T)
    _need(w_halo, (len(gs) * Cg // bk, 5, 2, Cx, bk), T, "w_halo")
    _need(gx, (N, 2 * R, 2 * R, Cx), T, "gx")
    if mask_a is not None:
        _need(mask_a, gx.shape, T, "mask_a")
    _numel_ok(mask_slope, Cx, torch.float32, "mask_slope")
    gp = (ctypes.c_void_p * len(gs))(*[ptr(t).value for t in gs])
    ws = layouts.split_for(w_halo) if T == torch.float32 else None
    _prof_call("mia_conv_s2_dgrad_halo_multi",
               flops if flops is not None else 2 * N * R * R * 9 * len(gs) * Cg * Cx,
               gp, len(gs), ptr(w_halo), ptr(ws), ptr(gx), N, R, Cg, Cx, ptr(mask_a),
               ptr(mask_slope), int(bool(accumulate)), dt(T), stream())
    return gx


def s2_dgrad_halo_ok(dtype, R, Cg, Cx):
    """Host mirror of s2_dgrad_halo_eligible (csrc/conv_upconv.hip)."""
    if _lib.get_tuning("MIA_S2DG_HALO") == 0:
        return False
    return R % 16 == 0 and Cg % 64 == 0 and Cx % 64 == 0


def sum_slices(x, y):
    """y (N, D) = Σ_s x[:, s, :] for x (N, S, D) fp32."""
    N, S, D = x.shape
    _need(y, (N, D), torch.float32, "y")
    if x.dtype != torch.float32:
        raise ValueError("sum_slices: fp32 required")
    call("mia_sum_slices", ptr(x), ptr(y), N, S, D, stream())
    return y
