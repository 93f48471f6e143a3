"""The staggered K loop of the fp32 split-once halo kernel (conv_halo_x6.hip, 128-column tile).

Waves 4–7 of a block run their MFMAs half a K-step behind waves 0–3, on fragments they keep in
registers across the barrier; every wave issues the MFMAs of the unstaggered loop in its order,
so outputs and the ordered reduction sums (sdot, q) must be bit-identical. MIA_X6_STAGGER = 0 / 1
(mia_set_tuning) forces the unstaggered (the earlier loop, unchanged: the reference) / staggered
instantiation of every epilogue feature mask the attack launches:
0, 4 BIAS, 8 TAP, 16 MASK, 32 ACC, 193 OSC|SDOT|BAB, 260 BIAS|RELU, 519 the modulated StyledConv
forward (PRO), 768 PReLU, 1040 MASK|MSL.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from gfa_amd import layouts, ops

pytestmark = pytest.mark.gpu

TOL_F32 = 2e-5  # rel. to max |ref|: tests/test_gpu_kernels.py TOL[torch.float32]
MODES = ["plain", "bias", "tap", "mask", "acc", "sdot_bab", "bias_relu", "mod", "prelu",
         "mask_slope"]
SQRT2 = math.sqrt(2.0)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().float()


def nchw(y):
    return y.permute(0, 3, 1, 2).double().cpu()


def rel_err(a, b):
    return ((a.double() - b.double()).abs().max() / b.abs().max().clamp_min(1e-30)).item()


class Case:
    """Seeded operands of one (N, H, W, Cin, Cout) shape, shared by the modes."""

    def __init__(self, N, H, W, Cin, Cout, dev):
        g = torch.Generator().manual_seed(N * 1000 + H * 100 + W * 10 + Cin + Cout)
        self.dims = (N, H, W, Cin, Cout)
        self.dev = dev
        r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
        self.x = r(N, Cin, H, W)
        self.w = r(Cout, Cin, 3, 3) / math.sqrt(9 * Cin)
        self.y0 = r(N, Cout, H, W)
        self.b = r(Cout) * 0.1
        self.m = r(N, Cout, H, W)
        self.a = r(N, Cout, H, W)
        self.t = r(N, Cout, H, W)
        self.slope = torch.rand(Cout, generator=g) * 0.5 + 0.05
        self.s_in = torch.rand(N, Cin, generator=g) + 0.5
        self.s_out = torch.rand(N, Cout, generator=g) + 0.5
        self.d = torch.rand(N, Cout, generator=g) + 0.5
        self.noise = r(H * W)
        kp = ops.conv2d_kpad(9, Cin, torch.float32)
        wm = torch.zeros(Cout, kp)
        wm[:, :9 * Cin] = self.w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin)
        self.grp = [dict(w=wm.to(dev), kh=3, kw=3, pad=(1, 1), ho=H, wo=W)]
        self.wf = layouts.fwd_matrix(self.w, torch.float32).to(dev)
        self.xc = nhwc(self.x).to(dev)
        self.on = {k: nhwc(getattr(self, k)).to(dev) for k in ("m", "a", "t")}

    def run(self, mode):
        """(y, sdot, q) of one launch; sdot / q are None unless the mode sums them."""
        N, H, W, Cin, Cout = self.dims
        dev = self.dev
        y = nhwc(self.y0).to(dev)
        sd = q = None
        if mode in ("prelu", "mask_slope"):
            kw = dict(act_out=ops.ACT_PRELU, act_slope=self.slope.to(dev)) if mode == "prelu" \
                else dict(mask_a=self.on["m"], mask_slope=self.slope.to(dev))
            ops.conv2d(self.xc, self.grp, y, (H, W), cout=Cout, **kw)
        else:
            kw = {}
            if mode == "bias":
                kw = dict(bias=self.b.to(dev))
            elif mode == "bias_relu":
                kw = dict(bias=self.b.to(dev), act_out=ops.ACT_RELU)
            elif mode == "tap":
                kw = dict(tap_a=self.on["a"], tap_t=self.on["t"], tap_coef=0.37)
            elif mode == "mask":
                kw = dict(mask_a=self.on["m"])
            elif mode == "acc":
                kw = dict(accumulate=True)
            elif mode == "mod":
                kw = dict(in_scale=self.s_in.to(dev), act_in=ops.ACT_LRELU_S2,
                          out_scale=self.d.to(dev), noise=self.noise.to(dev), noise_w=0.3,
                          bias=self.b.to(dev), act_out=ops.ACT_LRELU_S2)
            elif mode == "sdot_bab":
                sd = torch.zeros(N * Cout, device=dev)
                q = torch.zeros(N * Cout, device=dev)
                kw = dict(out_scale=self.s_out.to(dev), aux_x=self.on["a"], sdot=sd,
                          bab=dict(demod=self.d.to(dev), noise=self.noise.to(dev), noise_w=0.3,
                                   bias=self.b.to(dev), q=q))
            ops.conv3x3(self.xc, self.wf, y, cout=Cout, **kw)
        torch.cuda.synchronize()
        return y, sd, q

    def ref(self, mode):
        """fp64 (y, sdot, q) on the CPU."""
        N, H, W, Cin, Cout = self.dims
        x, w = self.x.double(), self.w.double()
        cv = lambda v: v.double().view(1, Cout, 1, 1)  # noqa: E731
        if mode == "mod":
            xa = torch.where(x > 0, x, 0.2 * x) * SQRT2 * self.s_in.double().view(N, Cin, 1, 1)
            pre = F.conv2d(xa, w, padding=1) * self.d.double().view(N, Cout, 1, 1) \
                + 0.3 * self.noise.double().view(1, 1, H, W) + cv(self.b)
            return torch.where(pre > 0, pre, 0.2 * pre) * SQRT2, None, None
        conv = F.conv2d(x, w, padding=1)
        m, a, t = self.m.double(), self.a.double(), self.t.double()
        if mode == "sdot_bab":
            sd = (conv * a).sum(dim=(2, 3)).reshape(-1)
            gp = conv * self.s_out.double().view(N, Cout, 1, 1) \
                * torch.where(a > 0, SQRT2, 0.2 * SQRT2)
            pre = a * torch.where(a > 0, 1 / SQRT2, 1 / (0.2 * SQRT2))
            q = (gp * (pre - 0.3 * self.noise.double().view(1, 1, H, W) - cv(self.b))) \
                .sum(dim=(2, 3)).reshape(-1)
            return gp * self.d.double().view(N, Cout, 1, 1), sd, q
        y = {"plain": conv, "bias": conv + cv(self.b),
             "bias_relu": F.relu(conv + cv(self.b)),
             "tap": conv + 0.37 * (a - t),
             "mask": conv * (m > 0),
             "acc": conv + self.y0.double(),
             "prelu": torch.where(conv > 0, conv, cv(self.slope) * conv),
             "mask_slope": torch.where(m > 0, conv, cv(self.slope) * conv)}[mode]
        return y, None, None


# One patch, two patches, two images of four patches; one channel block (no next-halo prefetch:
# the lagging half's skipped first and peeled last half-step are 17 half-steps apart), two and
# four blocks (both weight-ring parities, both halo buffers reused); one and two column tiles.
# The library accepts power-of-two Cin only (run_conv), so an odd block count above one cannot be
# launched: 128 is the smallest accepted Cin above 64.
@pytest.mark.parametrize("cout", [128, 256])
@pytest.mark.parametrize("cin", [32, 64, 128])
@pytest.mark.parametrize("N,H,W", [(1, 16, 16), (1, 16, 32), (2, 32, 32)])
def test_x6_stagger_bitwise(cuda, tune, N, H, W, cin, cout):
    """Staggered vs unstaggered instantiation, every feature mask of the attack: outputs and the
    ordered sdot / q sums equal bit for bit."""
    c = Case(N, H, W, cin, cout, cuda)
    tune("MIA_X6_STAGGER", 0)
    want = {mode: c.run(mode) for mode in MODES}
    tune("MIA_X6_STAGGER", 1)
    for mode in MODES:
        got = c.run(mode)
        for name, u, v in zip(("y", "sdot", "q"), got, want[mode]):
            assert (u is None) == (v is None)
            if u is not None:
                assert torch.equal(u, v), (mode, name, (u - v).abs().max().item())


@pytest.fixture(scope="module")
def fp64_case(cuda):
    return Case(2, 32, 32, 128, 256, cuda)


@pytest.mark.parametrize("mode", MODES)
def test_x6_stagger_vs_fp64(cuda, tune, fp64_case, mode):
    """The staggered loop against a torch fp64 conv on the CPU, one shape per feature mask, at the
    fp32 kernel tests' tolerance (2 × TOL[float32] of tests/test_gpu_kernels.py
    test_x6_halo_variants_bitwise), so the check does not rest on the unstaggered kernel alone.
    The sdot / q sums add H·W products per output: the same bound relative to their largest."""
    tune("MIA_X6_STAGGER", 1)
    y, sd, q = fp64_case.run(mode)
    ry, rsd, rq = fp64_case.ref(mode)
    e = rel_err(nchw(y), ry)
    print(f"{mode}: y rel err {e:.3e}")
    assert e < 2 * TOL_F32
    for name, u, v in (("sdot", sd, rsd), ("q", q, rq)):
        if v is not None:
            e = rel_err(u.cpu(), v)
            print(f"{mode}: {name} rel err {e:.3e}")
            assert e < 2 * TOL_F32
