"""PGD / FGSM attack on GAN image fusion: the public ``attack(net, imgs, eps, steps)`` entry point.

Semantics:
* objective — ``optimize_vgg`` (code/attack/interpolation.py:743-818), per image, MSE means:
    L = 10·MSE(E(x'),E(t')) − MSE(E(x'),E(x0')) + MSE(t, G(E(x'))) + 0.1·Σ_k MSE(V_k(G'), V_k(t'))
        + 10·MSE(x0, x) + Σ_k MSE(V_k(x'), V_k(x0'))          (' = avg_pool2d(·, S/256))
  The decoder receives the raw encoder output (no latent_avg, interpolation.py:780).
* update — torchattacks PGD (commented copy at interpolation.py:62-96), descending L
  (cost = −L, the targeted form :83-86): x ← clamp(x0 + clamp(x + a·sign(−∇L) − x0, −e, e), −1, 1),
  with e = 2ε, a = 2α because ε, α are given in [0,1] pixel units and the tensors live in [-1,1].
  FGSM = one step with α = ε and no random start.

Execution: every step runs on libmiattack kernels (no autograd, no torch compute ops):
encoder → synthesis → VGG(rec') fwd/bwd → VGG(x') fwd/bwd → synthesis bwd → encoder bwd →
fused gradient-assembly + sign-project kernel. Images are independent, so the batch is processed
together (per-image MSE means; a batch's gradient equals the reference's per-image gradients).
The loss is never materialised on the device unless ``return_info`` asks for it: PGD needs only
sign(∇L), so there is no per-step host synchronisation.
"""
import collections
import numbers

import numpy as np
import torch

from . import ops
from .vgg import CPAD
from .weights import ENC_POOL_RES, STYLE_DIM
from .workspace import Workspace

LOSS_WEIGHTS = dict(lat_t=10.0, lat_o=-1.0, img_rec_t=1.0, vgg_rec_t=0.1, img_o=10.0, vgg_img=1.0)
# the patch attack's loss (code/attack/patch/adversarial_patch.py:125): only −MSE(E(x0'), E(x'))
PATCH_WEIGHTS = dict(lat_t=0.0, lat_o=-1.0, img_rec_t=0.0, vgg_rec_t=0.0, img_o=0.0, vgg_img=0.0)
# Gradient (loss) scale per compute dtype. fp16: its range tops out at 65504, and the e4e
# encoder's backward from the latent terms (weight 10·2/(n_latent·512) per element) reaches
# 1e3–1e4 × λ… at λ = 2^16 whole images overflowed to inf/NaN (3 of 8 at 256², measured); at
# λ ≤ 2^12 none did and the gradient's sign agreed with fp32 on 99.98 % of the significant
# pixels, at λ = 2^8 too — 2^8 keeps 16× headroom. bf16 has fp32's exponent range: no scaling.
# An overflow that still happens is caught (per-image non-finite flags, read once per attack):
# the engine divides λ by RESCALE and re-runs the attack, at most MAX_RESCALES times.
DEFAULT_LOSS_SCALE = {torch.float32: 1.0, torch.float16: 2.0 ** 8, torch.bfloat16: 1.0}
RESCALE, MAX_RESCALES = 16.0, 4
RUN_OK, RUN_RESCALE, RUN_FATAL = 0, 1, 2  # per-run status, MAX-reduced over the ranks


def rescale_consensus(status, group=None):
    """The job-wide status of one attack run: the MAX of every rank's (OK < RESCALE < FATAL).
    Without a process group (single process) the local status."""
    if group is None:
        return status
    import torch.distributed as dist
    dev = (torch.device("cpu") if dist.get_backend(group) == "gloo"
           else torch.device("cuda", torch.cuda.current_device()))
    t = torch.tensor([int(status)], dtype=torch.int32, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
    return int(t.item())


def idle_rank_consensus(group):
    """A rank with an empty shard takes part in the attack's status rounds (one all-reduce per
    run of the ranks that attack) until they finish or fail together."""
    while True:
        st = rescale_consensus(RUN_OK, group)
        if st == RUN_OK:
            return
        if st == RUN_FATAL:
            raise FloatingPointError("non-finite gradient on another rank")


def _f32(v):
    return float(np.float32(v))


def uap_all_reduce(acc, group=None):
    """The job-wide sum of the universal perturbation's int64 plane, in place: one
    all_reduce(SUM) over ``group`` (none without a group). Integer addition is associative, so the
    result does not depend on the reduction's order or on the world size. On the device for nccl;
    through a CPU copy for gloo (as rescale_consensus chooses its device)."""
    if group is None:
        return acc
    import torch.distributed as dist
    if dist.get_backend(group) == "gloo":
        host = acc.cpu()
        dist.all_reduce(host, op=dist.ReduceOp.SUM, group=group)
        acc.copy_(host)
    else:
        dist.all_reduce(acc, op=dist.ReduceOp.SUM, group=group)
    return acc


def check_universal_count(n_total, plane):
    """The range of the universal perturbation's integer sum: per image and element the term is
    q = rint(ĝ·2^24) with |ĝ| = |g|/mean|g| < 2·plane (|g_j| ≤ Σ|g| = plane·mean|g|, and the kernel
    drops anything outside), so |q| ≤ 2^25·plane and |Σ_n q| ≤ n_total·plane·2^25. That stays
    below 2^62 — inside int64 with a factor 2 to spare — for n_total·plane < 2^37, n_total counted
    over the whole job (every rank's images enter the one sum)."""
    if int(n_total) * int(plane) >= ops.UAP_MAX_ELEMENTS:
        raise ValueError(f"universal: images × elements per image = {int(n_total)} × {int(plane)} "
                         "must be < 2^37 (the range of the int64 sum over the images)")


def idle_rank_universal(group, steps, shape, eps, alpha, device, random_start=False,
                        start_noise=None):
    """A rank with an empty shard in a universal attack (``shape`` = (1,3,S,S)): it joins every
    step's all-reduce with a zero plane and applies the job's sum to a δ of its own
    (ops.uap_step with no images), so it ends with the δ every other rank has; after each run of
    ``steps`` steps it joins the status round, and re-runs from δ₀ with the others when they lower
    the loss scale. ``steps`` all-reduces of the plane and one of the status per run. Returns δ."""
    e, a = _f32(2.0 * eps), _f32(2.0 * alpha)
    plane = int(np.prod(shape))
    zero_acc = torch.zeros(plane, dtype=torch.int64, device=device)
    acc = torch.empty_like(zero_acc)
    zero = torch.zeros(tuple(shape), dtype=torch.float32, device=device)
    noise = None
    if random_start:
        if start_noise is None or tuple(start_noise.shape) != tuple(shape):
            raise ValueError("a universal start_noise must have the shape (1,3,S,S)")
        noise = start_noise.to(device, torch.float32).contiguous()
    while True:
        delta = torch.zeros_like(zero)
        if noise is not None:
            ops.random_start(delta, zero, noise, e, -e, e)
        for _ in range(int(steps)):
            acc.copy_(zero_acc)
            uap_all_reduce(acc, group)
            ops.uap_step(delta, acc, None, None, a, e)
        st = rescale_consensus(RUN_OK, group)
        if st == RUN_OK:
            return delta
        if st == RUN_FATAL:
            raise FloatingPointError("non-finite gradient on another rank")


def apply_universal(imgs, delta):
    """clamp(imgs + delta, −1, 1): a universal perturbation (``info["universal"]["delta"]`` of
    ``attack(..., universal=True)``, (1,3,S,S)) applied to any images of its size, held-out ones
    included, on the HIP kernel of the attack itself (ops.uap_step without a sum, bit-identical to
    the attack's own application). imgs: (N,3,S,S) floating point, on CPU or GPU, not modified;
    the computation runs on delta's device if that is a GPU, else on imgs', else (both on the
    host, as ``attack`` returns them for host images) on the current GPU; without a GPU it raises.
    Returns fp32 images on imgs' device."""
    if not torch.is_tensor(delta) or delta.dim() != 4 or delta.shape[0] != 1 or delta.shape[1] != 3 \
            or delta.shape[2] != delta.shape[3] or not delta.is_floating_point():
        raise ValueError("delta must be a (1,3,S,S) floating point tensor")
    _check_images(imgs, delta.shape[2], "imgs")
    if imgs.shape[0] < 1:
        raise ValueError("imgs must hold at least one image")
    dev = delta.device if delta.is_cuda else imgs.device
    if dev.type != "cuda":
        if not torch.cuda.is_available():
            raise ValueError("apply_universal runs on the GPU only, and there is none")
        dev = torch.device("cuda", torch.cuda.current_device())
    x0 = imgs.detach().to(dev, torch.float32).contiguous()
    d = delta.detach().to(dev, torch.float32).contiguous()
    out = torch.empty_like(x0)
    ops.uap_step(d, None, out, x0, 0.0, 1.0)
    return out.to(imgs.device)


class AttackEngine:
    """Owns the device networks and the step workspace for one (batch, size, dtype)."""

    def __init__(self, encoder, synth, vgg, loss_scale=None, weights=LOSS_WEIGHTS):
        self.E, self.G, self.V = encoder, synth, vgg
        self.size = synth.size
        self.dtype = synth.dtype
        if vgg.dtype != self.dtype:
            raise ValueError("VGG and generator must share the compute dtype")
        self.R = min(self.size, 256)  # the objective pools to 256² (attack_main2.py:590-591)
        self.pf = self.size // self.R
        self.ws = Workspace(synth.device)
        self.w = dict(weights)
        # latent terms only (the patch attack): the generator and VGG terms carry weight 0, so
        # their gradient is 0·g and the step runs the encoder forward / backward alone
        self.lat_only = all(self.w[k] == 0 for k in ("img_rec_t", "vgg_rec_t", "img_o",
                                                     "vgg_img"))
        R = self.R
        self.tap_numel = [64 * R * R, 64 * R * R, 128 * (R // 4) ** 2,
                          512 * ops.pool_out(R // 4, True) ** 2]
        self.rescales = 0  # loss-scale reductions of the last attack (overflow re-runs)
        self.jp = None  # the JPEG stage of _step_gradient (set_jpeg): (qtab, grad), None = off
        self.set_loss_scale(loss_scale if loss_scale is not None
                            else DEFAULT_LOSS_SCALE[self.dtype])

    def set_loss_scale(self, lam):
        """λ: every gradient coefficient carries it (fp16 range); the projections and the Adam /
        C&W updates divide it back out (sign(λ·g) = sign(g))."""
        self.loss_scale = lam = float(lam)
        S2 = 3 * self.size * self.size
        nl = self.G.n_latent * STYLE_DIM
        self.c_lat_t = lam * self.w["lat_t"] * 2.0 / nl
        self.c_lat_o = lam * self.w["lat_o"] * 2.0 / nl
        self.c_img_rec = lam * self.w["img_rec_t"] * 2.0 / S2
        self.c_img_o = lam * self.w["img_o"] * 2.0 / S2
        self.c_vgg_rec = [lam * self.w["vgg_rec_t"] * 2.0 / n for n in self.tap_numel]
        self.c_vgg_x = [lam * self.w["vgg_img"] * 2.0 / n for n in self.tap_numel]

    # ------------------------------------------------------------------------------------------
    def _vgg_input(self, img, name):
        N = img.shape[0]
        y = self.ws.get(name, (N, self.R, self.R, CPAD), self.dtype)
        return ops.image_to_nhwc(img, y, self.pf, CPAD)

    def prepare(self, x0, t):
        """Targets under no_grad (interpolation.py:757-764): E(t'), E(x0'), VGG taps of t', x0'."""
        ws = self.ws
        N = x0.shape[0]
        self.N = N
        self.x0 = x0
        self.t = t
        self.nonfinite = ops.zero_(ws.get("nonfinite", (N,), torch.int32))
        self.lat_t = ws.get("ref.lat_t", (N, self.G.n_latent, STYLE_DIM), torch.float32)
        self.lat_t.copy_(self._encode(t, "ref.in")[0])
        self.lat_o = ws.get("ref.lat_o", (N, self.G.n_latent, STYLE_DIM), torch.float32)
        self.lat_o.copy_(self._encode(x0, "ref.in")[0])
        self.taps_t, self.taps_o = [], []
        for img, dst, nm in ((t, self.taps_t, "t"), (x0, self.taps_o, "o")):
            a = self.V.forward(self._vgg_input(img, "ref.in"), ws, "")
            for k, tap in enumerate(self.V.taps(a)):
                keep = ws.get(f"ref.tap{nm}{k}", tap.shape, self.dtype)
                keep.copy_(tap)
                dst.append(keep)

    def _encode(self, img, name):
        """E(img'). The e4e encoder reads the VGG input tensor x' (N,R,R,8) (both networks see
        avg_pool2d(img, S/256), attack_main2.py:597,622); returns (lat, x' or None)."""
        if getattr(self.E, "input_nhwc", False):
            xin = self._vgg_input(img, name)
            return self.E.forward_nhwc(xin, self.ws), xin
        return self.E.forward(img, self.ws), None

    def _loss_terms(self, which, out, *tensors):
        """out[n] += the per-image objective terms of one stage (unscaled weights, MSE means)."""
        w, nl = self.w, self.G.n_latent * STYLE_DIM
        S2 = 3 * self.size * self.size
        if which == "lat":
            lat, = tensors
            ops.mse_sum(lat, self.lat_t, out, w["lat_t"] / nl)
            ops.mse_sum(lat, self.lat_o, out, w["lat_o"] / nl)
        elif which == "rec":
            rec, a = tensors
            ops.mse_sum(rec, self.t, out, w["img_rec_t"] / S2)
            for k, tap in enumerate(self.V.taps(a)):
                ops.mse_sum(tap, self.taps_t[k], out, w["vgg_rec_t"] / self.tap_numel[k])
        else:
            x, a = tensors
            ops.mse_sum(x, self.x0, out, w["img_o"] / S2)
            for k, tap in enumerate(self.V.taps(a)):
                ops.mse_sum(tap, self.taps_o[k], out, w["vgg_img"] / self.tap_numel[k])

    def gradient(self, x, loss=None):
        """One forward/backward of the objective at x. Leaves (g_vgg_x, g_enc) for the update and
        returns them; both are scaled by loss_scale. ``loss`` (fp32 [N], zeroed by the caller)
        receives the per-image objective at x from the same forward pass (no host sync)."""
        ws, G, V, E = self.ws, self.G, self.V, self.E
        if self.lat_only:
            return self._gradient_lat(x, loss)
        lat, xin = self._encode(x, "in.x")
        rec = G.forward(lat, ws)
        self.rec = rec
        if loss is not None:
            self._loss_terms("lat", loss, lat)
        # reconstruction path: VGG(rec') vs VGG(t'), pixel MSE vs t
        a = V.forward(self._vgg_input(rec, "in.rec"), ws, "")
        if loss is not None:
            self._loss_terms("rec", loss, rec, a)
        g_rv = V.backward(a, self.taps_t, self.c_vgg_rec, ws, "r")
        g_img = ws.get("g.img", rec.shape, torch.float32)
        ops.image_grad(rec, self.t, g_rv, g_img, self.pf, self.c_img_rec)
        # input path: VGG(x') vs VGG(x0')
        a = V.forward(xin if xin is not None else self._vgg_input(x, "in.x"), ws, "")
        if loss is not None:
            self._loss_terms("x", loss, x, a)
        g_xv = V.backward(a, self.taps_o, self.c_vgg_x, ws, "x")
        # latent terms, synthesis backward, encoder backward
        g_lat = ws.get("g.lat", lat.shape, torch.float32)
        ops.mse_grad_f32(lat, self.lat_t, g_lat, self.c_lat_t)
        ops.mse_grad_f32(lat, self.lat_o, g_lat, self.c_lat_o, accumulate=True)
        G.backward(g_img, g_lat, ws)
        if xin is not None:  # e4e: ∂L/∂x' joins the VGG input-path gradient (same x')
            E.backward_nhwc(g_lat, ws, g_xv, accumulate=True)
            return g_xv, None
        return g_xv, E.backward(g_lat, ws)

    def _gradient_lat(self, x, loss=None):
        """gradient() when only the latent terms carry weight: E forward, the two latent MSE
        gradients, E backward (no generator, no VGG). Same return convention."""
        ws, E = self.ws, self.E
        lat, xin = self._encode(x, "in.x")
        if loss is not None:
            self._loss_terms("lat", loss, lat)
        g_lat = ws.get("g.lat", lat.shape, torch.float32)
        ops.mse_grad_f32(lat, self.lat_t, g_lat, self.c_lat_t)
        ops.mse_grad_f32(lat, self.lat_o, g_lat, self.c_lat_o, accumulate=True)
        N = x.shape[0]
        g_xv = ops.zero_(ws.get("g.xv0", (N, self.R, self.R, CPAD), self.dtype))
        if xin is not None:
            E.backward_nhwc(g_lat, ws, g_xv, accumulate=True)
            return g_xv, None
        return g_xv, E.backward(g_lat, ws)

    def run_patch(self, img, t, patch, mask, max_count):
        """The adversarial-patch loop (code/attack/patch/adversarial_patch.py:103-160) on the
        engine's loss weights (PATCH_WEIGHTS for the reference's loss): adv = (1−m)·img + m·patch;
        max_count times: g = ∇_adv L, patch −= g (the full-image gradient, step 1), adv =
        clamp((1−m)·img + m·patch, min(img), max(img)). `patch` (img's shape, fp32) is updated in
        place, as the reference's. Returns (adv, rec) with rec = G(E(adv')) of the last
        iteration's input (the reference's adv_img_rec).

        A loss-scale overflow (fp16) lowers λ and re-runs the whole loop from the caller's
        patch, like PGD / Adam / C&W (the raw-gradient step would otherwise have written NaN /
        Inf into the patch)."""
        self._no_jpeg("run_patch")
        patch0 = patch.clone()

        def once():
            patch.copy_(patch0)
            return self._run_patch(img, t, patch, mask, max_count)
        return self._with_rescale(once)

    def _run_patch(self, img, t, patch, mask, max_count):
        ws = self.ws
        f32 = torch.float32
        self.prepare(img, t)
        lo, hi = float(img.min()), float(img.max())  # torch.min / torch.max of the batch (:134)
        adv = ws.get("adv", img.shape, f32)
        ops.patch_update(patch, None, img, mask, adv, -float("inf"), float("inf"))  # :111 no clamp
        last = ws.get("patch.last", img.shape, f32)
        g = ws.get("g.full", img.shape, f32)
        for it in range(int(max_count)):
            if it == max_count - 1:
                last.copy_(adv)
            # the reference's MSEs are batch means (nn.MSELoss over the whole batch, :116): the
            # raw-gradient step scales with 1/N, unlike the sign steps of PGD
            self._assemble(adv, g, 1.0 / (self.loss_scale * img.shape[0]))
            ops.patch_update(patch, g, img, mask, adv, lo, hi)
        lat, _ = self._encode(last if max_count > 0 else adv, "in.x")
        return adv.clone(), self.G.forward(lat, ws).clone()

    def step(self, x, a, e):
        g_xv, g_enc = self.gradient(x)
        ops.pgd_update(x, self.x0, g_xv, g_enc, self.pf, ENC_POOL_RES, self.c_img_o, _f32(a),
                       _f32(e), nonfinite=self.nonfinite)
        return x

    def overflowed(self):
        """Images whose gradient had a non-finite element since prepare() (one host sync)."""
        return self.nonfinite.nonzero().flatten().tolist()

    def _with_rescale(self, run_once, group=None):
        """Run an attack; if any image's gradient overflowed, lower λ and run it again (fp16).
        A non-finite gradient at λ that cannot be lowered (fp32 / bf16, or after MAX_RESCALES)
        raises: sign(NaN) = 0 would otherwise leave those pixels silently unattacked.

        ``group`` (attack_distributed): the decision is taken by every rank together — each
        rank's status (OK / RESCALE / FATAL) is MAX-all-reduced after every run, so all shards
        re-run at the same λ (the result does not depend on the world size) and a fatal overflow
        raises on every rank instead of leaving the others blocked in the final all-gather."""
        self.rescales = 0
        while True:
            out = run_once()
            bad = self.overflowed()
            status = (RUN_OK if not bad else RUN_RESCALE
                      if self.dtype == torch.float16 and self.rescales < MAX_RESCALES
                      else RUN_FATAL)
            status = rescale_consensus(status, group)
            if status == RUN_OK:
                return out
            if status == RUN_FATAL:
                raise FloatingPointError(
                    f"non-finite gradient for images {bad[:8]}"
                    + ("" if bad else " on another rank")
                    + f" (dtype {self.dtype}, loss scale {self.loss_scale:g}): check the weights "
                    "/ inputs, or run fp32")
            self.set_loss_scale(self.loss_scale / RESCALE)
            self.rescales += 1

    def _assemble(self, x, g, scale, flag=True, loss=None):
        """g ← scale·λ·∇_x L at x (fp32 NCHW): gradient(x, loss), then the gradient-assembly
        kernel on what it left. ``flag``: a non-finite element marks its image in
        self.nonfinite. Returns g."""
        g_xv, g_enc = self.gradient(x, loss)
        return ops.grad_assemble(x, self.x0, g_xv, g_enc, g, self.pf, ENC_POOL_RES, self.c_img_o,
                                 scale, nonfinite=self.nonfinite if flag else None)

    def full_gradient(self, x):
        """∇_x L (unscaled, fp32 NCHW) at x."""
        g = self.ws.get("g.full", x.shape, torch.float32)
        return self._assemble(x, g, 1.0 / self.loss_scale, flag=False).clone()

    def objective(self, x, out):
        """Per-image objective at x into out (fp32 [N], +=): forward passes only."""
        ws, G, V, E = self.ws, self.G, self.V, self.E
        lat, xin = self._encode(x, "in.x")
        rec = G.forward(lat, ws)
        self._loss_terms("lat", out, lat)
        a = V.forward(self._vgg_input(rec, "in.rec"), ws, "")
        self._loss_terms("rec", out, rec, a)
        a = V.forward(xin if xin is not None else self._vgg_input(x, "in.x"), ws, "")
        self._loss_terms("x", out, x, a)
        return out

    def loss(self, x):
        """Per-image objective value (fp32, host) — diagnostics (syncs)."""
        out = self.ws.get("loss.diag", (x.shape[0],), torch.float32)
        ops.zero_(out)
        return self.objective(x, out).cpu()

    def _full_grad(self, x, g, loss=None):
        """g ← ∇_x L (loss-scaled, fp32 NCHW) by the gradient-assembly kernel."""
        return self._assemble(x, g, 1.0, loss=loss)

    def run_adam(self, x0, t, steps, lr=0.01, betas=(0.9, 0.999), eps=1e-8, group=None):
        """``optimize_vgg`` literal mode (interpolation.py:743-843): Adam(lr) on the pixels,
        descending L, no ε-ball or clamp. The gradient carries the loss scale λ, so Adam's eps is
        scaled by λ too (m̂/(√v̂ + λ·eps) on λ·g ≡ m̂/(√v̂ + eps) on g)."""
        self._no_jpeg("run_adam")
        return self._with_rescale(lambda: self._run_adam(x0, t, steps, lr, betas, eps), group)

    def _run_adam(self, x0, t, steps, lr, betas, eps):
        self.prepare(x0, t)
        ws = self.ws
        x = ws.get("adv", x0.shape, torch.float32)
        x.copy_(x0)
        m = ops.zero_(ws.get("adam.m", x0.shape, torch.float32))
        v = ops.zero_(ws.get("adam.v", x0.shape, torch.float32))
        g = ws.get("g.full", x0.shape, torch.float32)
        for it in range(1, steps + 1):
            self._full_grad(x, g)
            ops.adam_step(x, g, m, v, lr, betas[0], betas[1], eps * self.loss_scale, it)
        return x.clone()

    def run_cw(self, x0, t, steps, c=1e-4, lr=0.01, betas=(0.9, 0.999), eps=1e-8, group=None,
               early_stop=True):
        """torchattacks C&W L2 (interpolation.py:98-193) composed with the GAN objective, in
        [-1,1] space: adv = tanh(w); cost = Σ‖(adv − x0)/2‖² + c·Σ L_n(adv); Adam(lr) on w;
        best-L2 tracking with success = L_n(adv) < L_n(x0); early stop every steps//10 when the
        cost rises (one host sync there). See oracle.attack_ref.cw_attack. ``early_stop=False``
        runs every iteration (a fixed-work timing; not the reference's semantics)."""
        self._no_jpeg("run_cw")
        return self._with_rescale(
            lambda: self._run_cw(x0, t, steps, c, lr, betas, eps, early_stop), group)

    def _run_cw(self, x0, t, steps, c, lr, betas, eps, early_stop=True):
        self.prepare(x0, t)
        ws = self.ws
        N = x0.shape[0]
        f32 = torch.float32
        f0 = ops.zero_(ws.get("cw.f0", (N,), f32))
        self.objective(x0, f0)
        w = ops.cw_init(x0, ws.get("cw.w", x0.shape, f32))
        adv = ws.get("adv", x0.shape, f32)
        best = ws.get("cw.best", x0.shape, f32)
        best.copy_(x0)
        best_l2 = ws.get("cw.best_l2", (N,), f32)
        best_l2.fill_(1e10)
        m = ops.zero_(ws.get("adam.m", x0.shape, f32))
        v = ops.zero_(ws.get("adam.v", x0.shape, f32))
        g = ws.get("g.full", x0.shape, f32)
        gw = ws.get("cw.gw", x0.shape, f32)
        f = ws.get("cw.f", (N,), f32)
        sq = ws.get("cw.sq", (N,), f32)
        prev = 1e10
        every = max(steps // 10, 1)
        self.cw_steps_run = 0  # iterations executed (early stop), for bench.py's report
        for step in range(steps):
            self.cw_steps_run = step + 1
            ops.cw_tanh(w, adv)
            ops.zero_(f)
            self._full_grad(adv, g, loss=f)
            ops.cw_grad(adv, x0, g, gw, c, 1.0 / self.loss_scale)
            ops.adam_step(w, gw, m, v, lr, betas[0], betas[1], eps, step + 1)
            ops.zero_(sq)
            ops.mse_sum(adv, x0, sq)
            ops.cw_select(adv, best, sq, best_l2, f, f0, 0.25)
            if early_stop and step % every == 0:
                cost = 0.25 * float(sq.cpu().double().sum()) + c * float(f.cpu().double().sum())
                if cost > prev:
                    break
                prev = cost
        return best.clone()

    def run(self, x0, t, steps, eps, alpha, random_start=False, start_noise=None, group=None):
        """PGD-steps from x0 toward the objective; returns the adversarial images (new tensor)."""
        self._no_jpeg("run")
        return self._with_rescale(
            lambda: self._run_pgd(x0, t, steps, eps, alpha, random_start, start_noise), group)

    def _run_pgd(self, x0, t, steps, eps, alpha, random_start, start_noise):
        e, a = 2.0 * eps, 2.0 * alpha
        x = self._start(x0, t, _f32(e), random_start, start_noise)
        for _ in range(steps):
            self.step(x, a, e)
        return x.clone()

    def _start(self, x0, t, e, random_start, start_noise):
        """prepare() and the iterate buffer at x0 (or clamp(x0 + e·noise) for a random start)."""
        self.prepare(x0, t)
        x = self.ws.get("adv", x0.shape, torch.float32)
        x.copy_(x0)
        if random_start:
            if start_noise is None:
                raise ValueError("random_start needs start_noise (make_start_noise)")
            ops.random_start(x, x0, start_noise, e)
        return x

    def _step_gradient(self, x, m=None, c=0.0, si_scales=1, di=None, taps=None, l1=None,
                       l2sq=None):
        """The gradient a normalised step follows, with its per-image Σ|·| (l1) / Σ·² (l2sq, either
        may be None; device-resident): one chain of stages, each on or off.

            once per step:     [x̃ = x + c·m → jp.x]  [J → jp.y]                 (with jp only)
            per scale copy i:  [x + c·m, S_i → si.x]  [D → di.x]  networks, assemble → g.full
                               [2^-i·g, /n on the last copy → g.si]
            once per step:     [Dᵀ → g.di]  [J′(x̃)ᵀ → g.jp]  [taps ⊗ taps ⋆ → g.ti]

            g = W ⋆ Dᵀ (1/n)·Σ_i 2^-i·∇L(D S_i(x + c·m)),  S_i(t) = (t + 1)·2^-i − 1,  i = 0 … n − 1
            g = W ⋆ J′(x̃)ᵀ Dᵀ (1/n)·Σ_i 2^-i·∇L(D S_i(J(x̃))),  x̃ = x + c·m            (with jp)

        ``jp`` = self.jp = (qtab, grad), engine state set by set_jpeg() (None: off) rather than a
        parameter, so every caller's signature stays what it was: the JPEG stage, closest to the
        pixels because the saved file is what every later stage sees. qtab is the (2,64) fp32
        device table (jpeg_quant_tables), grad 'cubic' or 'ste'. The look-ahead point x̃ is then
        materialised first (ops.si_transform at s = 1; x itself without m), J runs once per step on
        it (ops.jpeg_roundtrip) and the scale
        copies read J(x̃) without a look-ahead; its adjoint runs once per step, after Dᵀ and before
        the smoothing (ops.jpeg_bwd_norms, the surrogate of Shin & Song at x̃). 'ste' skips the
        adjoint: J′ᵀ is taken as the identity (BPDA).

        ``m``: the Nesterov look-ahead (torchattacks NIFGSM), ``si_scales`` = n: the scale copies
        (SINIFGSM; ops.si_transform does both, and is skipped where it would be a bit copy: the
        networks then read x itself). ``di`` = (rnd, top, left): the step's resize-and-pad D
        (ops.di_resize_pad); the 10·MSE(x0, ·) term and both networks read the transformed input,
        the targets stay those of x0 and t. The gradient is UNSCALED (scale 1/λ: the steps divide
        by its own norm, which must not overflow with λ). Each copy's gradient is accumulated with
        weight 2^-i, the copy's own Jacobian (ops.si_accumulate_norms) — also for a look-ahead
        with a single copy, where w = div = 1. One D serves every copy, so its adjoint runs once,
        on the accumulated gradient (ops.di_resize_pad_bwd_norms; Dᵀ is linear), then the TI
        smoothing (ops.ti_smooth_norms). The sums are taken by the last kernel that runs; with no
        stage after the assembly that is the fused ops.grad_assemble_norms. Returns that kernel's
        output, the buffer the update kernel reads (the next call overwrites it)."""
        ws, f32 = self.ws, torch.float32
        n = int(si_scales)
        if not 1 <= n <= SI_MAX_SCALES:
            raise ValueError(f"si_scales must be an integer in 1 … {SI_MAX_SCALES}")
        xt, jp = None, self.jp
        if jp is not None:
            qtab, jp_grad = jp
            xt = x if m is None else ops.si_transform(x, m, ws.get("jp.x", x.shape, f32), c, 1.0)
            x, m = ops.jpeg_roundtrip(xt, ws.get("jp.y", x.shape, f32), qtab), None
            if jp_grad == "ste":
                xt = None
        accumulate = m is not None or si_scales != 1
        last_stage = ("ti" if taps is not None else "jp" if xt is not None
                      else "di" if di is not None else "si" if accumulate else "full")

        def sums(stage, last_copy=True):
            return (l1, l2sq) if stage == last_stage and last_copy else (None, None)

        flag = self.nonfinite
        g = out = ws.get("g.full", x.shape, f32)
        for i in range(n):
            xi = x
            if m is not None or i > 0:
                xi = ops.si_transform(x, m, ws.get("si.x", x.shape, f32), c, 2.0 ** -i)
            if di is not None:
                xi = ops.di_resize_pad(xi, ws.get("di.x", x.shape, f32), *di)
            if last_stage == "full":
                g_xv, g_enc = self.gradient(xi)
                ops.grad_assemble_norms(xi, self.x0, g_xv, g_enc, g, *sums("full"), self.pf,
                                        ENC_POOL_RES, self.c_img_o, 1.0 / self.loss_scale,
                                        nonfinite=flag)
            else:
                self._assemble(xi, g, 1.0 / self.loss_scale)
            if accumulate:
                last = i == n - 1
                out = ops.si_accumulate_norms(g, ws.get("g.si", x.shape, f32), *sums("si", last),
                                              2.0 ** -i, i == 0, float(n) if last else 1.0,
                                              nonfinite=flag)
        if di is not None:
            out = ops.di_resize_pad_bwd_norms(out, ws.get("g.di", x.shape, f32), *sums("di"), *di,
                                              nonfinite=flag)
        if xt is not None:
            out = ops.jpeg_bwd_norms(xt, out, ws.get("g.jp", x.shape, f32), qtab, *sums("jp"),
                                     nonfinite=flag)
        if taps is not None:
            out = ops.ti_smooth_norms(out, taps, ws.get("g.ti", x.shape, f32), *sums("ti"),
                                      nonfinite=flag)
        return out

    def ti_device_taps(self, taps):
        """The 1-D taps (ti_gaussian_taps) rounded once to fp32, on the engine's device."""
        t = torch.as_tensor(taps, dtype=torch.float64).reshape(-1)
        if t.numel() % 2 == 0 or not 1 <= t.numel() <= 63:
            raise ValueError("ti_taps must hold an odd number of values, 1 … 63")
        return t.to(torch.float32).to(self.G.device).contiguous()

    def _no_jpeg(self, what):
        """The runners that take no gradient through _step_gradient's chain, or that attack()
        rejects together with jpeg_quality, refuse to start while the JPEG stage is on: it would
        be ignored or enter a composition that nothing tests."""
        if self.jp is not None:
            raise ValueError(f"{what} does not combine with the JPEG stage: call set_jpeg(None) "
                             "first (run_mi, run_pi and run_l2 are the runs that take it)")

    def set_jpeg(self, jpeg_quality, jpeg_grad="cubic"):
        """Turn the JPEG stage of _step_gradient on (``jpeg_quality`` an integer in 1 … 100,
        ``jpeg_grad`` 'cubic' or 'ste') or off (None): self.jp = (the quantiser steps of
        jpeg_quant_tables as (2,64) fp32 on the engine's device, the gradient mode), or None. It
        is engine state, like the loss scale: step_l2 / step_mi / step_pi and the run_* wrappers
        keep their signatures and every gradient they take goes through the stage until it is
        turned off — step_l2 / step_mi / step_pi, run_l2 / run_mi / run_pi and whatever else
        calls _step_gradient. The other runners (run, run_adam, run_cw, run_spsa, run_universal,
        run_apgd, run_sign_hunter, run_patch) raise while it is on (_no_jpeg), as attack()
        rejects those combinations by name. Returns self.jp."""
        self.jp = None
        if jpeg_quality is not None:
            if self.size % 8:
                raise ValueError("jpeg_quality needs an image size that is a multiple of 8")
            qtab = jpeg_quant_tables(jpeg_quality).to(torch.float32).to(self.G.device)
            self.jp = (qtab.contiguous(), _check_jpeg_grad(jpeg_grad))
        return self.jp

    def step_l2(self, x, a, e, ti_taps=None, di=None, si_scales=1):
        """One L2-ball PGD step on x in place (after prepare()); a, e in [-1,1] units.
        ``ti_taps`` (fp32 device taps, ti_device_taps): the step follows the smoothed gradient.
        ``di`` (a make_di_schedule row (rnd, top, left, apply) of host integers): with apply = 1
        the gradient is Dᵀ ∇L(D x); apply = 0 or None is the plain step.
        ``si_scales`` > 1: the gradient is the mean over that many scale copies; 1 is the step
        without them (_step_gradient for all three; after set_jpeg() the JPEG stage too)."""
        # sums: Σg², Σ(adv − x0)² per image
        sums = ops.zero_(self.ws.get("norm.sums", (2, x.shape[0]), torch.float32))
        g = self._step_gradient(x, si_scales=si_scales, di=_di_row(di), taps=ti_taps,
                                l2sq=sums[0])
        ops.l2_step(x, self.x0, g, sums[0], sums[1], _f32(a), nonfinite=self.nonfinite)
        ops.l2_project(x, self.x0, sums[1], _f32(e))
        return x

    def _vt_grad_norms(self, x, m, c, si_scales, di, taps, l1, vt):
        """The variance-tuned gradient (torchattacks VMIFGSM) at x_nes = x + c·m (m None: x):
            g = G(x_nes);  gt = g + v;  gv = (1/N)·Σ_i G(x_nes + r·u_i);  v ← gv − g
        with v the variance buffer (vt.v, in unscaled gradient units like every gradient here),
        u_i the step's neighbour noise (ops.vt_neighbor, buffer vt.x) and G the step's gradient
        BEFORE the smoothing and without norms (_step_gradient with no taps and no sums; one D
        serves x_nes and all neighbours). g is kept in vt.g and the neighbours' gradients are
        averaged into vt.gv (ops.si_accumulate_norms, dividing by N on the last one) because G's
        own buffers are overwritten by the next pass; ops.vt_combine_norms then forms gt (vt.gt)
        and the new v together. On the last step (``vt.last``) the neighbours are skipped: v is
        never read again. The TI smoothing, if ``taps``, acts on gt; l1 receives Σ|·| of what
        the update kernel reads, which is returned. After set_jpeg() G includes the JPEG stage,
        J and its adjoint at x_nes and at every neighbour (it is part of _step_gradient)."""
        ws, f32 = self.ws, torch.float32
        g = ws.get("vt.g", x.shape, f32)
        g.copy_(self._step_gradient(x, m, c, si_scales, di))
        v = ws.get("vt.v", x.shape, f32)
        gv = None
        if not vt.last:
            gv = ws.get("vt.gv", x.shape, f32)
            y = ws.get("vt.x", x.shape, f32)
            for i in range(vt.samples):
                ops.vt_neighbor(x, m, y, c, vt.r, vt.seed, vt.image0, vt.step, i)
                gi = self._step_gradient(y, si_scales=si_scales, di=di)
                ops.si_accumulate_norms(gi, gv, None, None, 1.0, i == 0,
                                        float(vt.samples) if i == vt.samples - 1 else 1.0,
                                        nonfinite=self.nonfinite)
        gt = ws.get("vt.gt", x.shape, f32)
        ops.vt_combine_norms(g, gv, v, gt, l1 if taps is None else None,
                             nonfinite=self.nonfinite)
        if taps is None:
            return gt
        gs = ws.get("g.ti", x.shape, f32)
        return ops.ti_smooth_norms(gt, taps, gs, l1, None, nonfinite=self.nonfinite)

    def step_mi(self, x, m, momentum, a, e, ti_taps=None, di=None, nesterov=False, si_scales=1,
                vt=None):
        """One momentum iterative FGSM step on x and the momentum buffer m, both in place.
        ``ti_taps`` (fp32 device taps, ti_device_taps): the TI-FGSM step, on the smoothed
        gradient and its mean. ``di`` (a make_di_schedule row (rnd, top, left, apply) of host
        integers): with apply = 1 the DI-FGSM step, on Dᵀ ∇L(D x); apply = 0 or None is the step
        without input diversity. ``nesterov``: the gradient is taken at the look-ahead point
        x + c·m, c = momentum·a rounded once to fp32 (torchattacks NIFGSM; not clamped).
        ``si_scales`` > 1: the gradient is the mean over that many scale copies (torchattacks
        SINIFGSM; _step_gradient for all four). ``vt`` (a VtStep: samples, r, seed, image0, step,
        last): the variance-tuned step (torchattacks VMIFGSM, _vt_grad_norms) on the variance
        buffer ws "vt.v", with the neighbour noise of step index ``vt.step``; None is the step
        without it. After set_jpeg(quality, grad) it is the JPEG-robust step, on the gradient of
        the objective at J(x) (_step_gradient). The update rule is the same in every case."""
        g, l1 = self._mi_gradient(x, m, momentum, a, ti_taps, di, nesterov, si_scales, vt)
        ops.mi_update(x, self.x0, g, l1, m, _f32(momentum), _f32(a), _f32(e),
                      nonfinite=self.nonfinite)
        return x

    def _mi_gradient(self, x, m, momentum, a, ti_taps, di, nesterov, si_scales, vt):
        """What the momentum family's update kernels read: the step's gradient (_step_gradient or,
        with ``vt``, _vt_grad_norms; at the look-ahead point x + c·m with ``nesterov``, c =
        momentum·a rounded once to fp32) and its per-image Σ|·| in the zeroed norm.sums[0].
        Returns (g, l1)."""
        l1 = ops.zero_(self.ws.get("norm.sums", (2, x.shape[0]), torch.float32))[0]
        di = _di_row(di)
        # No kernel reads c without the look-ahead buffer; the variance-tuned step then passes 0
        # where the others pass μ·a, and the launch trace pins both (tests/test_step_trace_host.py)
        c = _f32(_f32(momentum) * _f32(a)) if nesterov or vt is None else 0.0
        look = m if nesterov else None
        if vt is None:
            g = self._step_gradient(x, look, c, si_scales, di, ti_taps, l1)
        else:
            g = self._vt_grad_norms(x, look, c, si_scales, di, ti_taps, l1, vt)
        return g, l1

    def step_pi(self, x, m, A, momentum, e, pi, ti_taps=None, di=None, nesterov=False,
                si_scales=1, vt=None):
        """One patch-wise step (PI-FGSM, Gao et al. 2020) on x in place: step_mi's gradient, every
        option of it included, then ops.pi_update in place of ops.mi_update. ``pi`` is a PiStep
        (ab = the amplified step β·a, gm = the project step γ·ab, both fp32 and in [-1,1] units,
        and the project kernel's edge). ``m`` and ``A`` are (in, out) PAIRS of distinct buffers,
        the momentum and the accumulated amplified noise: the kernel reads the first and writes
        the second of each, because a tile's halo reads its neighbours' old state while they
        write the new one; the caller swaps the pair after every step. The Nesterov look-ahead
        reads m[0] with c = momentum·ab, the step this rule really takes."""
        g, l1 = self._mi_gradient(x, m[0], momentum, pi.ab, ti_taps, di, nesterov, si_scales, vt)
        ops.pi_update(x, self.x0, g, l1, m[0], m[1], A[0], A[1], _f32(momentum), pi.ab, pi.gm,
                      _f32(e), pi.kernel, nonfinite=self.nonfinite)
        return x

    def run_l2(self, x0, t, steps, eps, alpha, random_start=False, start_noise=None, group=None,
               ti_taps=None, di=None, si_scales=1):
        """L2-ball PGD (torchattacks PGDL2.forward) descending L: per image
        x ← x + a·(−g)/(‖g‖₂ + 1e-10); d = x − x0; x ← clamp(x0 + d·min(e/‖d‖₂, 1), −1, 1), with
        e = 2·eps, a = 2·alpha. ``start_noise``: make_start_noise(shape, seed, "l2"). The norms
        stay on the device (ordered reductions): no per-step host synchronisation.
        ``ti_taps`` (1-D taps, ti_gaussian_taps): g is replaced by (taps ⊗ taps) ⋆ g.
        ``di`` (a (steps, 4) schedule, make_di_schedule): step k with apply = 1 follows
        Dₖᵀ ∇L(Dₖ x) (smoothed after the adjoint when ti_taps is given). The schedule is host
        data fixed before the loop, so an fp16 loss-scale re-run replays the same draws.
        ``si_scales`` (1 … SI_MAX_SCALES): every step follows the mean gradient over that many
        scale copies (_step_gradient; one Dₖ serves all copies of step k).
        After set_jpeg(quality, grad) every step follows the gradient of the objective at J(x),
        the JPEG round trip of the iterate."""
        taps = None if ti_taps is None else self.ti_device_taps(ti_taps)
        rows = _di_rows(di, steps, self.size)
        n_si = _check_si_scales(si_scales)
        return self._with_rescale(
            lambda: self._run_l2(x0, t, steps, eps, alpha, random_start, start_noise, taps,
                                 rows, n_si), group)

    def _run_l2(self, x0, t, steps, eps, alpha, random_start, start_noise, ti_taps=None,
                di=None, si_scales=1):
        e, a = _f32(2.0 * eps), _f32(2.0 * alpha)
        x = self._start(x0, t, e, random_start, start_noise)
        for k in range(steps):
            self.step_l2(x, a, e, ti_taps, None if di is None else di[k], si_scales)
        return x.clone()

    def run_mi(self, x0, t, steps, eps, alpha, momentum=1.0, random_start=False, start_noise=None,
               group=None, ti_taps=None, di=None, nesterov=False, si_scales=1, vt_samples=None,
               vt_beta=1.5, vt_seed=0, vt_first_image=0):
        """Momentum iterative FGSM (torchattacks MIFGSM.forward) descending L: per image
        ĝ = (−g)/mean|g|; m ← ĝ + μ·m (m = 0 at the start);
        x ← clamp(x0 + clamp(x + a·sign(m) − x0, −e, e), −1, 1), with e = 2·eps, a = 2·alpha.
        An image whose gradient is all zero (0/0) is reported like an overflow, never left frozen
        silently. ``ti_taps`` (1-D taps, ti_gaussian_taps): torchattacks TIFGSM without input
        diversity, g replaced by (taps ⊗ taps) ⋆ g before the normalisation.
        ``di`` (a (steps, 4) schedule, make_di_schedule): torchattacks DIFGSM (TIFGSM with
        ti_taps) — step k with apply = 1 uses g = Dₖᵀ ∇L(Dₖ x), Dₖ the step's resize-and-pad
        (smoothed after the adjoint when ti_taps is given). The schedule is host data fixed before
        the loop, so an fp16 loss-scale re-run replays the same draws.
        ``nesterov`` (torchattacks NIFGSM): g is taken at x + μ·a·m instead of at x.
        ``si_scales`` (1 … SI_MAX_SCALES; torchattacks SINIFGSM's m): g is the mean over that many
        scale copies, g = (1/n)·Σ_i 2^-i·∇L(S_i(·)), S_i(t) = (t + 1)·2^-i − 1 (_step_gradient;
        one Dₖ serves all copies of step k). Within a step: look-ahead, scale copy, Dₖ, the
        networks, the accumulation over the copies, one adjoint Dₖᵀ, the smoothing, the update.
        ``vt_samples`` (1 … VT_MAX_SAMPLES; torchattacks VMIFGSM's N): the variance-tuned attack —
        the step follows g + v, v the variance term of the previous step (0 at the start):
        v ← (1/N)·Σ_i G(x_nes + r·u_{k,i}) − G(x_nes), r = fp32(vt_beta)·e in fp32, G the step's
        gradient before the smoothing (_vt_grad_norms). u_{k,i} is counter-based noise, a pure
        function of (vt_seed, vt_first_image + n, k, i, element): a loss-scale re-run starts from
        v = 0 and replays the same noise, and an image's result does not depend on the batch. The
        last step draws no neighbours.
        After set_jpeg(quality, grad): the JPEG-robust attack — every gradient above is that of the
        objective at J(·), the round trip through a baseline 4:4:4 JPEG of that quality
        (ops.jpeg_roundtrip, once per gradient, at the look-ahead point), pulled back through J by
        ``grad``: 'cubic', the adjoint of Shin & Song's surrogate (ops.jpeg_bwd_norms, after Dₖᵀ
        and before the smoothing), or 'ste', the identity. The iterate itself stays
        uncompressed."""
        return self._with_rescale(self._mi_runner(
            x0, t, steps, eps, alpha, momentum, random_start, start_noise, ti_taps, di, nesterov,
            si_scales, vt_samples, vt_beta, vt_seed, vt_first_image), group)

    def _mi_runner(self, x0, t, steps, eps, alpha, momentum, random_start, start_noise, ti_taps, di,
                   nesterov, si_scales, vt_samples, vt_beta, vt_seed, vt_first_image, pi=None):
        """run_mi's / run_pi's arguments checked and moved to the device once, before any re-run:
        the closure _with_rescale runs."""
        taps = None if ti_taps is None else self.ti_device_taps(ti_taps)
        rows = _di_rows(di, steps, self.size)
        n_si = _check_si_scales(si_scales)
        vt = None
        if vt_samples is not None:
            vt = (_check_vt_samples(vt_samples), _check_vt_beta(vt_beta),
                  int(vt_seed) % (1 << 64), _check_vt_first_image(vt_first_image, x0.shape[0]))
        return lambda: self._run_mi(x0, t, steps, eps, alpha, momentum, random_start, start_noise,
                                    taps, rows, bool(nesterov), n_si, vt, pi)

    def run_pi(self, x0, t, steps, eps, alpha, pi_amplification=10.0, pi_kernel=3, pi_project=1.0,
               momentum=0.0, random_start=False, start_noise=None, group=None, ti_taps=None,
               di=None, nesterov=False, si_scales=1, vt_samples=None, vt_beta=1.5, vt_seed=0,
               vt_first_image=0):
        """The patch-wise attack (Gao, Zhang et al., "Patch-wise Attack for Fooling Deep Neural
        Network", ECCV 2020; PI-FGSM), L∞, descending L. It changes run_mi's update, not its
        gradient: the step is amplified to ab = fp32(fp32(β)·a), β = ``pi_amplification``, and the
        part of the accumulated noise A that overflows the ε-ball is redistributed to each pixel's
        K × K neighbours (K = ``pi_kernel``, odd in 3 … 15) with the project step gm =
        fp32(fp32(γ)·ab), γ = ``pi_project``, instead of being clipped away. Per step, image,
        plane and pixel, with e = 2·eps, a = 2·alpha, m = 0 and A = 0 at the start:
            ĝ = (−g)/mean|g|;  m ← ĝ + μ·m;  s = sign(m);  A' = A + ab·s
            C = sign(A')·max(|A'| − e, 0);  S = Σ_{window without its centre} C;  p = gm·sign(S)
            A ← A' + p;  x ← clamp(x0 + clamp(x + ab·s + p − x0, −e, e), −1, 1)
        (one fused HIP kernel, ops.pi_update; S is a chain of fp32 additions in a fixed order, zero
        padded, see include/miattack.h). g is run_mi's gradient with every option of it:
        ``ti_taps``, ``di``, ``si_scales``, ``vt_*``, set_jpeg() and ``nesterov``, whose look-ahead
        is x + μ·ab·m. m and A ping-pong between two workspace buffers each (mi.m / mi.m1, pi.a0 /
        pi.a1), swapped every step. A random start and an fp16 loss-scale re-run begin from
        A = 0. There is no host read-back in the loop. γ = 0 gives run_mi with a = ab; β = 1 with
        steps·alpha ≤ eps gives run_mi, both bit for bit."""
        pi = PiStep(*pi_steps(alpha, pi_amplification, pi_project), _check_pi_kernel(pi_kernel))
        return self._with_rescale(self._mi_runner(
            x0, t, steps, eps, alpha, momentum, random_start, start_noise, ti_taps, di, nesterov,
            si_scales, vt_samples, vt_beta, vt_seed, vt_first_image, pi), group)

    def _run_mi(self, x0, t, steps, eps, alpha, momentum, random_start, start_noise,
                ti_taps=None, di=None, nesterov=False, si_scales=1, vt=None, pi=None):
        e, a = _f32(2.0 * eps), _f32(2.0 * alpha)
        f32 = torch.float32
        x = self._start(x0, t, e, random_start, start_noise)
        m = ops.zero_(self.ws.get("mi.m", x0.shape, f32))
        if vt is not None:
            n_vt, beta, key, image0 = vt
            r = _f32(np.float32(beta) * np.float32(e))
            ops.zero_(self.ws.get("vt.v", x0.shape, f32))
        if pi is not None:  # the state ping-pongs: step k reads buffer k % 2 and writes the other
            ms = (m, self.ws.get("mi.m1", x0.shape, f32))
            As = (ops.zero_(self.ws.get("pi.a0", x0.shape, f32)),
                  self.ws.get("pi.a1", x0.shape, f32))
        for k in range(steps):
            step_vt = None if vt is None else VtStep(n_vt, r, key, image0, k, k == steps - 1)
            row = None if di is None else di[k]
            if pi is None:
                self.step_mi(x, m, momentum, a, e, ti_taps, row, nesterov, si_scales, step_vt)
            else:
                i, o = k % 2, (k + 1) % 2
                self.step_pi(x, (ms[i], ms[o]), (As[i], As[o]), momentum, e, pi, ti_taps, row,
                             nesterov, si_scales, step_vt)
        return x.clone()

    # ---- SPSA: the score-based black-box attack ------------------------------------------------
    def spsa_gradient(self, x, sp, l1=None, l2sq=None):
        """The SPSA estimate of ∇_x L at x (Spall 1992; Uesato et al. 2018; torchattacks SPSA's
        estimator) from objective VALUES only, ``sp`` a SpsaStep (samples = q, d, seed, image0,
        step):
            per pair i = 0 … q − 1:  x⁺ = clamp(x + d·v_i, −1, 1), x⁻ = clamp(x − d·v_i, −1, 1)
                                     f⁺ = L(x⁺), f⁻ = L(x⁻)             (objective(): forward only)
                                     ĝ ← ĝ + (f⁺ − f⁻)·s·v_i,  s = fp32(1/(2·d));  / q on the last
        v_i is the Rademacher direction of (seed, image0 + n, step, i, element): ops.spsa_probe
        writes both probes in one pass (buffers spsa.xp, spsa.xm) and ops.spsa_accumulate_norms
        regenerates v_i from the same counter, so no direction is ever stored. f⁺ and f⁻ stay on
        the device (spsa.fp, spsa.fm): no host synchronisation. The last accumulation takes the
        per-image Σ|ĝ| (l1) / Σĝ² (l2sq; either may be None) and a non-finite objective marks
        its image in self.nonfinite. 2·q forward passes and no backward pass; the loss scale
        plays no part. Returns ĝ (spsa.g; the next call overwrites it)."""
        ws, f32 = self.ws, torch.float32
        N, q = x.shape[0], int(sp.samples)
        if not 1 <= q <= SPSA_MAX_SAMPLES:
            raise ValueError(f"spsa samples must be an integer in 1 … {SPSA_MAX_SAMPLES}")
        xp, xm = ws.get("spsa.xp", x.shape, f32), ws.get("spsa.xm", x.shape, f32)
        fp, fm = ws.get("spsa.fp", (N,), f32), ws.get("spsa.fm", (N,), f32)
        g = ws.get("spsa.g", x.shape, f32)
        s = spsa_scale(sp.d)
        for i in range(q):
            ops.spsa_probe(x, xp, xm, sp.d, sp.seed, sp.image0, sp.step, i)
            self.objective(xp, ops.zero_(fp))
            self.objective(xm, ops.zero_(fm))
            last = i == q - 1
            ops.spsa_accumulate_norms(g, fp, fm, l1 if last else None, l2sq if last else None, s,
                                      sp.seed, sp.image0, sp.step, i, i == 0,
                                      float(q) if last else 1.0, nonfinite=self.nonfinite)
        return g

    def step_spsa(self, x, m, momentum, a, e, sp, norm="linf"):
        """One SPSA step on x in place (after prepare()): the estimate spsa_gradient(x, sp) takes
        the update of ``norm`` unchanged — 'linf' the MIFGSM rule on the momentum buffer m
        (ops.mi_update; momentum 0 is the plain sign step), 'l2' the PGDL2 rule (ops.l2_step,
        ops.l2_project; m is not used). a, e in [-1,1] units."""
        sums = ops.zero_(self.ws.get("norm.sums", (2, x.shape[0]), torch.float32))
        if norm == "linf":
            g = self.spsa_gradient(x, sp, l1=sums[0])
            ops.mi_update(x, self.x0, g, sums[0], m, _f32(momentum), _f32(a), _f32(e),
                          nonfinite=self.nonfinite)
        elif norm == "l2":
            g = self.spsa_gradient(x, sp, l2sq=sums[0])
            ops.l2_step(x, self.x0, g, sums[0], sums[1], _f32(a), nonfinite=self.nonfinite)
            ops.l2_project(x, self.x0, sums[1], _f32(e))
        else:
            raise ValueError("SPSA is implemented for norm='linf' and 'l2' only")
        return x

    def run_spsa(self, x0, t, steps, eps, alpha, momentum=0.0, norm="linf", random_start=False,
                 start_noise=None, group=None, spsa_samples=16, spsa_delta=0.01, spsa_seed=0,
                 spsa_first_image=0):
        """SPSA, the score-based black-box attack: ``steps`` steps of step_spsa from x0, with
        e = 2·eps, a = 2·alpha and the probe radius d = fp32(2·spsa_delta), ``spsa_samples`` = q
        antithetic pairs per step (1 … SPSA_MAX_SAMPLES). The attack reads the objective's value
        only — 2·q queries per image per step, self.spsa_queries = 2·q·steps in all — and no
        gradient, so the loss scale plays no part; a non-finite objective raises as a non-finite
        gradient does (_with_rescale). The directions are a pure function of (spsa_seed,
        spsa_first_image + n, step, pair, element): reruns are bit-identical and an image's
        result depends on neither the batch nor the world size. An estimate that is entirely
        zero under 'linf' (every pair with f⁺ = f⁻) is reported like an overflow (0/0), as an
        all-zero gradient is by run_mi."""
        self._no_jpeg("run_spsa")
        if norm not in ("linf", "l2"):
            raise ValueError("SPSA is implemented for norm='linf' and 'l2' only")
        q = _check_spsa_samples(spsa_samples)
        d = _f32(2.0 * _check_spsa_delta(spsa_delta))
        key = int(spsa_seed) % (1 << 64)
        image0 = _check_spsa_first_image(spsa_first_image, x0.shape[0])
        self.spsa_queries = 2 * q * int(steps)
        return self._with_rescale(
            lambda: self._run_spsa(x0, t, steps, eps, alpha, momentum, norm, random_start,
                                   start_noise, q, d, key, image0), group)

    def _run_spsa(self, x0, t, steps, eps, alpha, momentum, norm, random_start, start_noise, q, d,
                  key, image0):
        e, a = _f32(2.0 * eps), _f32(2.0 * alpha)
        x = self._start(x0, t, e, random_start, start_noise)
        m = ops.zero_(self.ws.get("mi.m", x0.shape, torch.float32))
        for k in range(steps):
            self.step_spsa(x, m, momentum, a, e, SpsaStep(q, d, key, image0, k), norm)
        return x.clone()

    # ---- the universal perturbation: one δ for the whole batch --------------------------------
    def _uap_buffers(self, shape):
        """The workspace buffers ``uap.*`` of a batch of ``shape``: the shared plane ``delta``
        (1,3,S,S) fp32, a zero plane of its shape (x0 of the random start) and the int64 sum
        ``acc`` [3·S²]."""
        ws, one = self.ws, (1,) + tuple(shape[1:])
        plane = int(np.prod(shape[1:]))
        return dict(delta=ws.get("uap.delta", one, torch.float32),
                    zero=ws.get("uap.zero", one, torch.float32),
                    acc=ws.get("uap.acc", (plane,), torch.int64))

    def start_universal(self, x0, t, eps, random_start=False, start_noise=None):
        """prepare(), δ₀ (0, or clamp(e·u, −e, e) for a random start with the ONE (1,3,S,S) draw
        ``start_noise``: ops.random_start on a zero plane with the bounds ∓e) and the iterate
        x = clamp(x0 + δ₀, −1, 1) (ops.uap_step without a sum). Returns the iterate buffer for
        step_universal; δ lives in the workspace buffer ``uap.delta``."""
        self.prepare(x0, t)
        e = _f32(2.0 * eps)
        b = self._uap_buffers(x0.shape)
        delta, zero = ops.zero_(b["delta"]), ops.zero_(b["zero"])
        if random_start:
            if start_noise is None:
                raise ValueError("random_start needs start_noise (make_start_noise)")
            if tuple(start_noise.shape) != tuple(delta.shape):
                raise ValueError("a universal start_noise must have the shape (1,3,S,S)")
            ops.random_start(delta, zero, start_noise, e, -e, e)
        x = self.ws.get("adv", x0.shape, torch.float32)
        ops.uap_step(delta, None, x, x0, 0.0, e)
        return x

    def step_universal(self, x, a, e, group=None):
        """One step of the universal perturbation on δ (``uap.delta``) and the iterate x, both in
        place (after start_universal); a, e in [-1,1] units. Four stages:
            1. the gradient chain at x with the per-image Σ|g| (_step_gradient: unscaled g)
            2. ops.uap_accumulate: acc = Σ_n rint(ĝ_n·2^24), ĝ_n = (−g_n)/mean|g_n|, int64
            3. ``group``: one all_reduce(acc, SUM) over the job (uap_all_reduce)
            4. ops.uap_step: δ ← clamp(δ + a·sgn(acc), −e, e); x_n ← clamp(x0_n + δ, −1, 1)
        Nothing is read back to the host (a gloo group sums through a CPU copy). Every image is
        normalised by its own mean |g|, so the loss scale cancels; a non-finite ĝ marks its image
        in self.nonfinite and contributes 0."""
        b = self._uap_buffers(x.shape)
        l1 = ops.zero_(self.ws.get("norm.sums", (2, x.shape[0]), torch.float32))[0]
        g = self._step_gradient(x, l1=l1)
        ops.uap_accumulate(g, l1, b["acc"], True, nonfinite=self.nonfinite)
        uap_all_reduce(b["acc"], group)
        ops.uap_step(b["delta"], b["acc"], x, self.x0, _f32(a), _f32(e))
        return x

    def run_universal(self, x0, t, steps, eps, alpha, random_start=False, start_noise=None,
                      group=None):
        """The universal L∞ perturbation: ONE δ (1,3,S,S), ‖δ‖∞ ≤ e, fitted on all images of the
        job, with e = 2·eps, a = 2·alpha. δ₀ = 0 (or the random start), then ``steps`` times
            ĝ_n = (−∇L(x_n)) / mean|∇L(x_n)|;  A = Σ_n rint(ĝ_n·2^24)      (int64, over ALL images)
            δ ← clamp(δ + a·sgn(A), −e, e);  x_n ← clamp(x0_n + δ, −1, 1)
        (step_universal). The sum over the images is an integer sum, so δ depends on neither the
        order of the images, nor the batch split, nor the world size (``group``: one all-reduce
        per step, the one attack with a collective in its data path). Returns the batch
        clamp(x0 + δ) (new tensor); δ is kept in self.uap_delta (a clone, on the device). An fp16
        loss-scale re-run restarts from δ₀."""
        self._no_jpeg("run_universal")
        return self._with_rescale(
            lambda: self._run_universal(x0, t, steps, eps, alpha, random_start, start_noise,
                                        group), group)

    def _run_universal(self, x0, t, steps, eps, alpha, random_start, start_noise, group):
        e, a = _f32(2.0 * eps), _f32(2.0 * alpha)
        x = self.start_universal(x0, t, eps, random_start, start_noise)
        for _ in range(steps):
            self.step_universal(x, a, e, group)
        self.uap_delta = self._uap_buffers(x0.shape)["delta"].clone()
        return x.clone()

    # ---- Auto-PGD ------------------------------------------------------------------------------
    def _apgd_buffers(self, shape, steps=None):
        """The workspace buffers ``apgd.*`` of a batch of ``shape`` (``steps``: of the attack that
        start_apgd began): images x_old, x_best, g_best; the per-image state ``state_f`` (fp32
        rows eta, L_best, L_prev, L_check) and ``state_i`` (int32 rows n_dec, reduced, best_step);
        the action words; the step's objective ``f``; the histories ``loss`` / ``step_size``
        (steps + 1, N)."""
        ws, f32, i32, N = self.ws, torch.float32, torch.int32, shape[0]
        steps = self.apgd_steps if steps is None else steps
        b = {k: ws.get("apgd." + k, shape, f32) for k in ("x_old", "x_best", "g_best")}
        b.update(state_f=ws.get("apgd.state_f", (4, N), f32),
                 state_i=ws.get("apgd.state_i", (3, N), i32),
                 action=ws.get("apgd.action", (N,), i32), f=ws.get("apgd.f", (N,), f32),
                 loss=ws.get("apgd.loss", (steps + 1, N), f32),
                 step_size=ws.get("apgd.step_size", (steps + 1, N), f32),
                 g=ws.get("g.full", shape, f32))
        return b

    def start_apgd(self, x0, t, steps, eps, random_start=False, start_noise=None):
        """prepare(), the iterate at x0 (or the L∞ random start) and the Auto-PGD state of a
        ``steps``-step attack: one gradient pass at the start gives g and L(x), then x_old =
        x_best = x, g_best = g, L_best = L_prev = L_check = L(x), eta = 2·e, n_dec = 0,
        reduced = 1 and row 0 of the histories (ops.apgd_decide at step 0, ops.apgd_apply).
        Returns the iterate buffer for step_apgd."""
        self.apgd_steps = int(steps)
        self.apgd_e = e = _f32(2.0 * eps)
        self.apgd_rows = {i: (k, thr) for i, k, thr in apgd_schedule(steps)}
        x = self._start(x0, t, e, random_start, start_noise)
        b = self._apgd_buffers(x0.shape)
        ops.zero_(b["f"])
        self._full_grad(x, b["g"], loss=b["f"])
        b["x_old"].copy_(x)
        ops.apgd_decide(b["f"], b["state_f"], b["state_i"], b["action"], b["loss"],
                        b["step_size"], 0, eta0=_f32(2.0 * e))
        ops.apgd_apply(x, b["g"], b["x_best"], b["g_best"], b["action"])
        return x

    def step_apgd(self, x, i):
        """Step i (0-based) of the attack start_apgd began, on the iterate x in place: the
        momentum update with the per-image step size (ops.apgd_update; weight 1 at i = 0,
        APGD_MOMENTUM after), one gradient pass for g and L_i at the new x, the per-image control
        (ops.apgd_decide, a checkpoint where apgd_schedule has a row for i) and the copies it
        asks for (ops.apgd_apply: keep the best x and g, or restart from them). Nothing is read
        back to the host."""
        if not 0 <= i < self.apgd_steps:
            raise ValueError("step index outside the attack start_apgd began")
        b = self._apgd_buffers(x.shape)
        ops.apgd_update(x, b["x_old"], self.x0, b["g"], b["state_f"][0],
                        1.0 if i == 0 else _f32(APGD_MOMENTUM), self.apgd_e,
                        nonfinite=self.nonfinite)
        ops.zero_(b["f"])
        self._full_grad(x, b["g"], loss=b["f"])
        k, thr = self.apgd_rows.get(i, (0, 0))
        ops.apgd_decide(b["f"], b["state_f"], b["state_i"], b["action"], b["loss"],
                        b["step_size"], i + 1, checkpoint=k > 0, thr=thr)
        ops.apgd_apply(x, b["g"], b["x_best"], b["g_best"], b["action"])
        return x

    def run_apgd(self, x0, t, steps, eps, random_start=False, start_noise=None, group=None):
        """Auto-PGD, L∞ (Croce & Hein 2020; torchattacks APGD.attack_single_run with
        norm='Linf', eot_iter=1, one run) descending L, with e = 2·eps; no alpha. Per image n a
        step size eta[n] starts at 2·e; step i (a = 1 for i = 0, else 0.75) is
            d = x − x_old;  x_old ← x
            z = clamp(min(max(x − eta[n]·sign(g), x0 − e), x0 + e), −1, 1)
            x ← clamp(min(max((x + (z − x)·a) + d·(1 − a), x0 − e), x0 + e), −1, 1)
        followed by the gradient and the objective L_i at the new x in one pass, and per image
            L_i < L_prev: n_dec += 1;  L_prev = L_i;  L_i < L_best: L_best = L_i, x_best ← x, g_best ← g
            at a checkpoint (k, thr) of apgd_schedule(steps):
                flag = n_dec <= thr or (reduced == 0 and L_check <= L_best)
                reduced = flag;  L_check = L_best;  n_dec = 0;  flag: eta /= 2, x ← x_best, g ← g_best
        Returns x_best (steps + 1 gradient passes). All state lives on the device (workspace
        buffers ``apgd.*``): no per-step host synchronisation. An fp16 loss-scale re-run restarts
        every piece of it.

        One deviation from torchattacks: at the first checkpoint its check_oscillation compares
        step 0 with loss_steps[-1], a zero row reached by negative indexing; here step 0 is
        compared with the objective at the starting point, the paper's condition."""
        self._no_jpeg("run_apgd")
        return self._with_rescale(
            lambda: self._run_apgd(x0, t, steps, eps, random_start, start_noise), group)

    def _run_apgd(self, x0, t, steps, eps, random_start, start_noise):
        x = self.start_apgd(x0, t, steps, eps, random_start, start_noise)
        for i in range(steps):
            self.step_apgd(x, i)
        return self._apgd_buffers(x0.shape)["x_best"].clone()

    def apgd_info(self):
        """The record of the last Auto-PGD run, on the host (one sync): ``loss`` and ``step_size``
        (steps + 1, N) — L and eta at the start (row 0) and after step i (row i + 1) —
        ``best_step`` [N] (0: the start, i + 1: step i) and ``halvings`` [N], how often each
        image's step size was halved."""
        b = self._apgd_buffers(self.x0.shape)
        eta = b["step_size"].cpu()
        return dict(loss=b["loss"].cpu(), step_size=eta,
                    best_step=b["state_i"][2].cpu().to(torch.int64),
                    halvings=(eta[1:] < eta[:-1]).sum(dim=0))

    # ---- SignHunter: the deterministic score-based black-box attack ---------------------------
    def _sh_buffers(self, shape, steps=None):
        """The workspace buffers ``sh.*`` of a batch of ``shape`` (``steps``: of the attack that
        start_sign_hunter began): the sign plane ``s`` int8 (N, plane); per image ``best`` and the
        query's objective ``f`` (fp32), the last decision ``accept`` and the count ``n_accept``
        (int32); the history ``loss`` (steps + 1, N)."""
        ws, f32, i32, N = self.ws, torch.float32, torch.int32, shape[0]
        steps = self.sh_steps if steps is None else steps
        plane = int(np.prod(shape[1:]))
        return dict(s=ws.get("sh.s", (N, plane), torch.int8), best=ws.get("sh.best", (N,), f32),
                    f=ws.get("sh.f", (N,), f32), accept=ws.get("sh.accept", (N,), i32),
                    n_accept=ws.get("sh.n_accept", (N,), i32),
                    loss=ws.get("sh.loss", (steps + 1, N), f32))

    def _sh_query(self, x, b, k):
        """Query k at the iterate x: the objective (forward passes only) and the decision."""
        self.objective(x, ops.zero_(b["f"]))
        ops.sh_decide(b["f"], b["best"], b["accept"], b["n_accept"], b["loss"], k,
                      nonfinite=self.nonfinite)

    def start_sign_hunter(self, x0, t, eps, steps=0):
        """prepare() and query 0 of a SignHunter attack of ``steps`` flips: s = +1 everywhere
        (the sign plane prefilled with −1 and flipped whole), x = clamp(x0 + e·s, −1, 1),
        L_best = L(x), row 0 of the history. Returns the iterate buffer for step_sign_hunter."""
        self.prepare(x0, t)
        self.sh_steps = int(steps)
        self.sh_e = _f32(2.0 * eps)
        plane = int(np.prod(x0.shape[1:]))
        self.sh_rows = sh_schedule(self.sh_steps, plane)
        b = self._sh_buffers(x0.shape)
        x = self.ws.get("adv", x0.shape, torch.float32)
        ops.fill_bytes_(b["s"], 0xFF)
        ops.sh_flip(x, x0, b["s"].view(x0.shape), None, None, (0, plane), self.sh_e)
        self._sh_query(x, b, 0)
        return x

    def step_sign_hunter(self, x, k):
        """Query k (1 … steps) of the attack start_sign_hunter began, on the iterate x in place:
        one launch flips the signs on row k − 1 of sh_schedule and flips row k − 2 back in the
        images that rejected query k − 1 (ops.sh_flip, on those two segments only), then the
        objective at the new vertex and the per-image decision (ops.sh_decide). Nothing is read
        back to the host."""
        if not 1 <= k <= self.sh_steps:
            raise ValueError("query index outside the attack start_sign_hunter began")
        b = self._sh_buffers(x.shape)
        prev = self.sh_rows[k - 2] if k >= 2 else None
        ops.sh_flip(x, self.x0, b["s"].view(x.shape), b["accept"], prev, self.sh_rows[k - 1],
                    self.sh_e)
        self._sh_query(x, b, k)
        return x

    def finish_sign_hunter(self, x):
        """After the last query: the images that rejected it get their last segment flipped back,
        so x holds every image's best vertex."""
        if self.sh_steps >= 1:
            b = self._sh_buffers(x.shape)
            ops.sh_flip(x, self.x0, b["s"].view(x.shape), b["accept"], self.sh_rows[-1], None,
                        self.sh_e)
        return x

    def run_sign_hunter(self, x0, t, steps, eps, group=None):
        """SignHunter (Al-Dujaili & O'Reilly 2020), L∞, with e = fp32(2·eps); no alpha, no random
        numbers. Every iterate is a vertex clamp(x0 + e·s, −1, 1) of the ball, s ∈ {−1, +1} per
        element (kept as int8: a clamped element loses its sign). Per image independently:
            query 0:  s = +1;  L_best = L(x)
            query k = 1 … steps:  flip s on row k − 1 of sh_schedule(steps, 3·S²), evaluate L;
                                  L < L_best: keep the flip, L_best = L; else flip back
        (a tie or a NaN is a rejection). Returns every image's best vertex (new tensor);
        ``steps`` = 0 returns a copy of x0 without a query, else steps + 1 queries per image, one
        forward pass each (self.sh_queries). The attack reads the objective's value only, so the
        loss scale plays no part; a non-finite objective marks its image and raises as a
        non-finite gradient does (_with_rescale). All state lives on the device (workspace
        buffers ``sh.*``): no per-query host synchronisation. The schedule depends on the image
        size alone, so reruns are bit-identical and an image's result depends on neither the
        batch nor the world size."""
        self._no_jpeg("run_sign_hunter")
        steps = int(steps)
        self.sh_queries = steps + 1 if steps > 0 else 0
        return self._with_rescale(lambda: self._run_sign_hunter(x0, t, steps, eps), group)

    def _run_sign_hunter(self, x0, t, steps, eps):
        if steps == 0:
            self.prepare(x0, t)
            self.sh_steps = 0
            return x0.clone()
        x = self.start_sign_hunter(x0, t, eps, steps)
        for k in range(1, steps + 1):
            self.step_sign_hunter(x, k)
        return self.finish_sign_hunter(x).clone()

    def sign_hunter_info(self):
        """The record of the last SignHunter run, on the host (one sync): ``loss`` (steps + 1, N),
        the objective of every query; ``best`` [N], the objective of the returned vertex;
        ``accepted`` [N], the number of flips kept. A run of 0 steps made no query: ``loss`` has
        no row, ``best`` is NaN and ``accepted`` 0."""
        N = self.x0.shape[0]
        if self.sh_steps == 0:
            return dict(loss=torch.zeros((0, N)), best=torch.full((N,), float("nan")),
                        accepted=torch.zeros((N,), dtype=torch.int64))
        b = self._sh_buffers(self.x0.shape)
        return dict(loss=b["loss"].cpu(), best=b["best"].cpu(),
                    accepted=b["n_accept"].cpu().to(torch.int64))


APGD_RHO = 0.75       # a checkpoint flags an image with at most floor(ρ·k) decreases in k steps
APGD_MOMENTUM = 0.75  # the weight a of the new step against the previous displacement (i > 0)


def apgd_schedule(steps):
    """The checkpoints of an Auto-PGD run of ``steps`` steps (torchattacks APGD), a pure function
    of ``steps``: a list of rows (step index, k, thr). With k0 = max(int(0.22·steps), 1),
    k_min = max(int(0.06·steps), 1), dec = max(int(0.03·steps), 1): a counter starts at 0 and the
    window at k = k0; after every step the counter goes up by one; when it equals k, that step is
    a checkpoint with window k and threshold thr = floor(ρ·k), ρ = APGD_RHO (= 3k // 4, exact);
    then the counter restarts and k ← max(k − dec, k_min)."""
    if isinstance(steps, bool) or int(steps) != steps or steps < 0:
        raise ValueError("need integer steps >= 0")
    steps = int(steps)
    k = max(int(0.22 * steps), 1)
    k_min = max(int(0.06 * steps), 1)
    dec = max(int(0.03 * steps), 1)
    rows, counter = [], 0
    for i in range(steps):
        counter += 1
        if counter == k:
            rows.append((i, k, 3 * k // 4))
            counter = 0
            k = max(k - dec, k_min)
    return rows


def sh_schedule(steps, plane):
    """The segments SignHunter flips, a pure function of (``steps``, ``plane`` = elements per
    image): a list of ``steps`` rows (lo, hi), row k − 1 being the segment [lo, hi) of query k.
    Divide and conquer: level h starts at 0 and has the chunk length len = ceil(plane / 2^h); its
    rows are (i·len, min((i + 1)·len, plane)) for i = 0 … ceil(plane / len) − 1, which tile
    [0, plane). After the level with len = 1 (every element on its own) h wraps to 0, otherwise
    h += 1. plane = 192: the lengths 192, 96, 48, 24, 12, 6, 3, 2, 1, a cycle of 415 rows."""
    if isinstance(steps, (bool, np.bool_)) or not isinstance(steps, (int, np.integer)) or steps < 0:
        raise ValueError("need integer steps >= 0")
    if (isinstance(plane, (bool, np.bool_)) or not isinstance(plane, (int, np.integer))
            or not 1 <= plane < 1 << 31):
        raise ValueError("plane must be an integer in 1 … 2^31 − 1")
    steps, plane = int(steps), int(plane)
    rows, h = [], 0
    while len(rows) < steps:
        ln = (plane + (1 << h) - 1) >> h
        for i in range((plane + ln - 1) // ln):
            if len(rows) == steps:
                break
            rows.append((i * ln, min((i + 1) * ln, plane)))
        h = 0 if ln == 1 else h + 1
    return rows


def _check_images(imgs, size, name):
    if not torch.is_tensor(imgs) or imgs.dim() != 4 or imgs.shape[1] != 3:
        raise ValueError(f"{name} must be an (N,3,H,W) tensor")
    if imgs.shape[2] != size or imgs.shape[3] != size:
        raise ValueError(f"{name} must be {size}x{size} (net.decoder.size)")
    if not imgs.is_floating_point():
        raise ValueError(f"{name} must be floating point")


NORMS = ("linf", "l2", "adam", "l2_cw")
TI_MAX_KERNEL = 63  # mia_ti_smooth_norms
SI_MAX_SCALES = ops.SI_MAX_SCALES  # mia_si_transform (torchattacks SINIFGSM's default m is 5)


def _check_si_scales(si_scales):
    """attack()'s / run_*'s ``si_scales``: None (no scale copies) or an integer in
    1 … SI_MAX_SCALES; returns the number of copies (None → 1)."""
    if si_scales is None:
        return 1
    if (isinstance(si_scales, bool) or not isinstance(si_scales, (int, np.integer))
            or not 1 <= si_scales <= SI_MAX_SCALES):
        raise ValueError(f"si_scales must be None or an integer in 1 … {SI_MAX_SCALES}")
    return int(si_scales)


VT_MAX_SAMPLES = 32  # neighbours per step (torchattacks VMIFGSM's default N is 5)
# The Philox key of the neighbours' noise is (seed + VT_SEED_OFFSET) mod 2^64 ("VMI-FGSM" in
# ASCII): a stream of its own, like DI_SEED_OFFSET. Step and sample go into the counter.
VT_SEED_OFFSET = 0x564D492D4647534D
# One variance-tuned step (step_mi's ``vt``): the number of neighbours, their radius r in [-1,1]
# units (fp32), the Philox key, the global index of the batch's first image, the 0-based step
# index of the noise, and whether this is the last step (no neighbours: v is never read again).
VtStep = collections.namedtuple("VtStep", "samples r seed image0 step last")


def _check_vt_samples(vt_samples):
    """attack()'s / run_mi's ``vt_samples``: an integer in 1 … VT_MAX_SAMPLES."""
    if (isinstance(vt_samples, bool) or not isinstance(vt_samples, (int, np.integer))
            or not 1 <= vt_samples <= VT_MAX_SAMPLES):
        raise ValueError(f"vt_samples must be None or an integer in 1 … {VT_MAX_SAMPLES}")
    return int(vt_samples)


def _check_vt_beta(vt_beta):
    if (isinstance(vt_beta, (bool, np.bool_)) or not isinstance(vt_beta, numbers.Real)
            or not np.isfinite(float(vt_beta)) or not float(vt_beta) > 0):
        raise ValueError("vt_beta must be a finite number > 0")
    return float(vt_beta)


def _check_vt_first_image(vt_first_image, n):
    """The global index of imgs[0]: an integer >= 0 with vt_first_image + n <= 2^32 (the image
    word of the noise counter)."""
    if (isinstance(vt_first_image, (bool, np.bool_))
            or not isinstance(vt_first_image, (int, np.integer)) or vt_first_image < 0):
        raise ValueError("vt_first_image must be an integer >= 0")
    if int(vt_first_image) + int(n) > 1 << 32:
        raise ValueError("vt_first_image + the batch size must be <= 2^32")
    return int(vt_first_image)


PI_MAX_KERNEL = ops.PI_MAX_KERNEL  # mia_pi_update's largest project kernel
# One patch-wise step (step_pi's ``pi``): the amplified step ab = fp32(fp32(β)·a), the project step
# gm = fp32(fp32(γ)·ab), both in [-1,1] units, and the project kernel's edge K.
PiStep = collections.namedtuple("PiStep", "ab gm kernel")


def _check_pi_amplification(pi_amplification):
    """attack()'s / run_pi's ``pi_amplification`` (the paper's β): a finite number > 0."""
    if (isinstance(pi_amplification, (bool, np.bool_))
            or not isinstance(pi_amplification, numbers.Real)
            or not np.isfinite(float(pi_amplification)) or not float(pi_amplification) > 0):
        raise ValueError("pi_amplification must be None or a finite number > 0")
    return float(pi_amplification)


def _check_pi_kernel(pi_kernel):
    """attack()'s / run_pi's ``pi_kernel``: an odd integer in 3 … PI_MAX_KERNEL."""
    if (isinstance(pi_kernel, (bool, np.bool_)) or not isinstance(pi_kernel, (int, np.integer))
            or pi_kernel % 2 == 0 or not 3 <= pi_kernel <= PI_MAX_KERNEL):
        raise ValueError(f"pi_kernel must be an odd integer in 3 … {PI_MAX_KERNEL}")
    return int(pi_kernel)


def _check_pi_project(pi_project):
    """attack()'s / run_pi's ``pi_project`` (the paper's γ over β·α): a finite number >= 0."""
    if (isinstance(pi_project, (bool, np.bool_)) or not isinstance(pi_project, numbers.Real)
            or not np.isfinite(float(pi_project)) or not float(pi_project) >= 0):
        raise ValueError("pi_project must be a finite number >= 0")
    return float(pi_project)


def pi_steps(alpha, pi_amplification, pi_project=1.0):
    """(ab, gm) of the patch-wise attack in [-1,1] units, in fp32 arithmetic with one rounding per
    operation: a = fp32(2·alpha), ab = fp32(fp32(pi_amplification)·a), gm = fp32(fp32(pi_project)·ab).
    Raises where ab is not a finite number > 0 or gm is not finite."""
    beta, gamma = _check_pi_amplification(pi_amplification), _check_pi_project(pi_project)
    with np.errstate(over="ignore"):
        ab = np.float32(beta) * np.float32(2.0 * float(alpha))
        gm = np.float32(gamma) * ab
    if not (np.isfinite(ab) and ab > 0):
        raise ValueError("pi_amplification: the amplified step fp32(pi_amplification·2·alpha) must "
                         "be a finite number > 0")
    if not np.isfinite(gm):
        raise ValueError("pi_project: the project step fp32(pi_project·pi_amplification·2·alpha) "
                         "must be finite")
    return float(ab), float(gm)


SPSA_MAX_SAMPLES = 256  # antithetic pairs per step (torchattacks SPSA's default nb_sample is 128)
# The Philox key of the SPSA directions is (seed + SPSA_SEED_OFFSET) mod 2^64 ("SPSA-ATK" in
# ASCII): a stream of its own, like VT_SEED_OFFSET and DI_SEED_OFFSET.
SPSA_SEED_OFFSET = 0x535053412D41544B
# One SPSA step (step_spsa's ``sp``): the number of antithetic pairs q, the probe radius d in
# [-1,1] units (fp32), the Philox key, the global index of the batch's first image and the
# 0-based step index of the directions.
SpsaStep = collections.namedtuple("SpsaStep", "samples d seed image0 step")


def spsa_scale(d):
    """s = 1/(2·d) of the SPSA estimate for a probe radius d, in fp32 arithmetic (2·d is exact,
    one IEEE division)."""
    return float(np.float32(1.0) / (np.float32(2.0) * np.float32(d)))


def _check_spsa_samples(spsa_samples):
    """attack()'s / run_spsa's ``spsa_samples``: an integer in 1 … SPSA_MAX_SAMPLES."""
    if (isinstance(spsa_samples, (bool, np.bool_))
            or not isinstance(spsa_samples, (int, np.integer))
            or not 1 <= spsa_samples <= SPSA_MAX_SAMPLES):
        raise ValueError(f"spsa_samples must be None or an integer in 1 … {SPSA_MAX_SAMPLES}")
    return int(spsa_samples)


def _check_spsa_delta(spsa_delta):
    """attack()'s / run_spsa's ``spsa_delta``: finite and > 0, and so are the fp32 probe radius
    d = fp32(2·spsa_delta) and its scale 1/(2·d) (both normal fp32 numbers)."""
    ok = (not isinstance(spsa_delta, (bool, np.bool_)) and isinstance(spsa_delta, numbers.Real)
          and np.isfinite(float(spsa_delta)) and float(spsa_delta) > 0)
    if ok:
        d = 2.0 * float(spsa_delta)
        ok = 2.0 ** -126 <= d <= 2.0 ** 125
    if not ok:
        raise ValueError("spsa_delta must be a finite number > 0 (in [0,1] pixel units)")
    return float(spsa_delta)


def _check_spsa_first_image(spsa_first_image, n):
    """The global index of imgs[0]: an integer >= 0 with spsa_first_image + n <= 2^32 (the image
    word of the direction counter)."""
    if (isinstance(spsa_first_image, (bool, np.bool_))
            or not isinstance(spsa_first_image, (int, np.integer)) or spsa_first_image < 0):
        raise ValueError("spsa_first_image must be an integer >= 0")
    if int(spsa_first_image) + int(n) > 1 << 32:
        raise ValueError("spsa_first_image + the batch size must be <= 2^32")
    return int(spsa_first_image)


# ITU T.81 Annex K, tables K.1 (luminance) and K.2 (chrominance), natural (row-major) order
JPEG_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55,
             14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
             18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
             49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
JPEG_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
               24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
JPEG_GRADS = ("cubic", "ste")


def _check_jpeg_quality(quality):
    """attack()'s ``jpeg_quality`` / jpeg_compress's ``quality``: an integer in 1 … 100."""
    if (isinstance(quality, (bool, np.bool_)) or not isinstance(quality, (int, np.integer))
            or not 1 <= quality <= 100):
        raise ValueError("jpeg_quality must be None or an integer in 1 … 100")
    return int(quality)


def _check_jpeg_grad(jpeg_grad):
    """attack()'s ``jpeg_grad``: 'cubic' (the surrogate's adjoint) or 'ste' (the identity)."""
    if jpeg_grad not in JPEG_GRADS:
        raise ValueError(f"jpeg_grad must be one of {JPEG_GRADS}")
    return jpeg_grad


def jpeg_quant_tables(quality):
    """The quantiser steps a baseline JPEG of ``quality`` (an integer in 1 … 100) is written with:
    an int64 (2,64) host tensor, luminance then chrominance, natural order — the Annex K tables T
    under the IJG scaling s = 5000 // q if q < 50 else 200 − 2·q,
    Q = clamp((T·s + 50) // 100, 1, 255) (what libjpeg / Pillow write at that quality)."""
    q = _check_jpeg_quality(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    t = torch.tensor([JPEG_LUMA, JPEG_CHROMA], dtype=torch.int64)
    return torch.clamp((t * s + 50) // 100, 1, 255)


def jpeg_dct_matrix():
    """The orthonormal 8 × 8 DCT-II matrix of the JPEG kernels, fp32 (8,8):
    D[u][i] = c(u)/2·cos((2i+1)·u·π/16), c(0) = 1/√2, evaluated in fp64 and rounded once."""
    u = torch.arange(8, dtype=torch.float64).reshape(8, 1)
    i = torch.arange(8, dtype=torch.float64).reshape(1, 8)
    d = 0.5 * torch.cos((2 * i + 1) * u * (np.pi / 16))
    d[0] = 0.5 / np.sqrt(2.0)
    return d.to(torch.float32)


def jpeg_compress(imgs, quality):
    """J(imgs): what saving the images as baseline 4:4:4 JPEGs of ``quality`` and loading them
    again does to them, on the HIP kernel the attack itself uses (ops.jpeg_roundtrip). imgs:
    (N,3,S,S) floating point in [-1,1] ON THE GPU, S a multiple of 8, not modified. Returns fp32
    images on the same device."""
    if not torch.is_tensor(imgs) or imgs.dim() != 4 or imgs.shape[1] != 3 \
            or not imgs.is_floating_point():
        raise ValueError("imgs must be an (N,3,S,S) floating point tensor")
    if not imgs.is_cuda:
        raise ValueError("jpeg_compress runs on the GPU only: pass device tensors")
    qtab = jpeg_quant_tables(quality).to(imgs.device, torch.float32)
    x = imgs.detach().to(torch.float32).contiguous()
    return ops.jpeg_roundtrip(x, torch.empty_like(x), qtab)


def ti_gaussian_taps(kernlen=15, nsig=3.0):
    """The 1-D taps of torchattacks TIFGSM's Gaussian kernel, fp64: k/Σk with k = exp(−x²/2) on
    linspace(−nsig, nsig, kernlen). torchattacks' gkern (scipy.stats.norm.pdf, whose 1/√(2π)
    cancels in the normalisation) is exactly outer(taps, taps). The taps are symmetric bit for
    bit: linspace's two halves can differ by an ulp, so k is averaged with its mirror image."""
    if (isinstance(kernlen, bool) or not isinstance(kernlen, (int, np.integer))
            or kernlen % 2 == 0 or not 1 <= kernlen <= TI_MAX_KERNEL):
        raise ValueError(f"the TI kernel length must be an odd integer in 1 … {TI_MAX_KERNEL}")
    nsig = float(nsig)
    if not (np.isfinite(nsig) and nsig > 0):
        raise ValueError("ti_nsig must be finite and > 0")
    x = np.linspace(-nsig, nsig, int(kernlen))
    k = np.exp(-0.5 * x * x)
    k = 0.5 * (k + k[::-1])
    return torch.from_numpy(k / k.sum())


# make_di_schedule's generator is seeded with (seed + DI_SEED_OFFSET) mod 2^63 ("DI-FGSM" in
# ASCII): a stream of its own, never make_start_noise's manual_seed(seed) replayed.
DI_SEED_OFFSET = 0x44492D4647534D


def _check_di_rate(size, resize_rate):
    """lo = int(size·resize_rate), the smallest resized edge; it must lie in 1 … size − 1."""
    if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or size < 2:
        raise ValueError("the image size must be an integer >= 2")
    if isinstance(resize_rate, bool) or not isinstance(resize_rate, numbers.Real):
        raise ValueError("di_resize_rate must be a number")
    rate = float(resize_rate)
    if not np.isfinite(rate):
        raise ValueError("di_resize_rate must be finite")
    lo = int(size * rate)
    if not 1 <= lo <= size - 1:
        raise ValueError(
            f"di_resize_rate must give 1 <= int(size * rate) <= size - 1 (got {lo} at size "
            f"{size}): the networks are fixed-size, so rates >= 1 (torchattacks' enlarging "
            "form) are not supported")
    return lo


def _check_di_prob(prob):
    if (isinstance(prob, bool) or not isinstance(prob, numbers.Real)
            or not 0.0 <= float(prob) <= 1.0):  # NaN fails the comparison
        raise ValueError("di_prob must be a number in [0, 1]")
    return float(prob)


def make_di_schedule(steps, size, resize_rate=0.9, diversity_prob=0.5, seed=0):
    """The input-diversity draws of a whole attack: a host int64 (steps, 4) tensor of rows
    (rnd, top, left, apply), torchattacks ``input_diversity`` at a fixed image size ``size``:

        lo = int(size·resize_rate);  rnd = randint(lo, size)          lo <= rnd <= size − 1
        top = randint(0, size − rnd);  left = randint(0, size − rnd)  top + rnd <= size − 1
        apply = rand() < diversity_prob

    One row per step serves the whole batch (as torchattacks). The draws match torchattacks in
    distribution and order, not in values: they come from a generator of their own, seeded with
    (seed + DI_SEED_OFFSET) mod 2^63, and are taken step by step in the fixed order rnd, top,
    left, apply — one scalar draw each, all four at every step whatever ``apply`` turns out to be
    — so a shorter schedule of the same seed is a prefix of a longer one. Computed before the
    loop: a loss-scale re-run replays it, every rank of ``attack_distributed`` computes the same
    one, and an image's result does not depend on the batch or world size."""
    if isinstance(steps, bool) or int(steps) != steps or steps < 0:
        raise ValueError("need integer steps >= 0")
    lo = _check_di_rate(size, resize_rate)
    p = _check_di_prob(diversity_prob)
    size = int(size)
    g = torch.Generator().manual_seed((int(seed) + DI_SEED_OFFSET) % (1 << 63))
    rows = []
    for _ in range(int(steps)):
        rnd = int(torch.randint(lo, size, (1,), generator=g))
        top = int(torch.randint(0, size - rnd, (1,), generator=g))
        left = int(torch.randint(0, size - rnd, (1,), generator=g))
        u = float(torch.rand((1,), dtype=torch.float64, generator=g))
        rows.append((rnd, top, left, int(u < p)))
    return torch.tensor(rows, dtype=torch.int64).reshape(int(steps), 4)


def check_di_schedule(schedule, steps, size):
    """An explicit schedule as a host int64 (steps, 4) tensor: rows (rnd, top, left, apply) with
    1 <= rnd <= size, top, left >= 0, top + rnd <= size, left + rnd <= size (the kernels'
    constraints; rnd = size is the identity) and apply in {0, 1}."""
    try:
        s = torch.as_tensor(schedule)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError("di_schedule must be an integer (steps, 4) tensor") from None
    if s.is_floating_point() or s.is_complex() or s.dtype == torch.bool:
        raise ValueError("di_schedule must hold integers")
    if s.dim() != 2 or tuple(s.shape) != (int(steps), 4):
        raise ValueError(f"di_schedule must have shape (steps, 4) = ({int(steps)}, 4)")
    s = s.detach().to("cpu", torch.int64)
    rnd, top, left, ap = s[:, 0], s[:, 1], s[:, 2], s[:, 3]
    ok = ((rnd >= 1) & (rnd <= size) & (top >= 0) & (left >= 0) & (top <= size - rnd)
          & (left <= size - rnd) & ((ap == 0) | (ap == 1)))
    if not bool(ok.all()):
        k = int((~ok).nonzero()[0])
        raise ValueError(f"di_schedule row {k} = {s[k].tolist()}: need 1 <= rnd <= {size}, "
                         "top, left >= 0, top + rnd <= size, left + rnd <= size, apply in {0, 1}")
    return s


def _di_rows(schedule, steps, size):
    """run_*'s ``di``: None, or the checked schedule as a list of host-integer rows."""
    if schedule is None:
        return None
    return check_di_schedule(schedule, steps, size).tolist()


def _di_row(di):
    """step_*'s ``di``: (rnd, top, left) of a row with apply = 1, None for apply = 0 / None."""
    if di is None:
        return None
    rnd, top, left, ap = (int(v) for v in di)
    if ap not in (0, 1):
        raise ValueError("di: apply must be 0 or 1")
    return (rnd, top, left) if ap else None


def make_start_noise(shape, seed, norm="linf"):
    """The random-start draw of the FULL batch shape (scaled by e in the kernel, x = clamp(x0 +
    e·u)); ``attack_distributed`` slices it per shard so every world size sees the same noise.

    'linf': host-seeded U(-1,1) per element. 'l2': per image a point of the unit L2 ball by
    torchattacks PGDL2's construction — a Gaussian direction, normalised (‖·‖₂ + 1e-10), times
    r ~ U(0,1). This matches torchattacks in distribution, not in rounding order (there e
    multiplies r before the direction; here the kernel multiplies the finished sample)."""
    g = torch.Generator().manual_seed(int(seed))
    if norm == "linf":
        return torch.rand(shape, generator=g) * 2 - 1
    if norm != "l2":
        raise ValueError("start noise exists for norm 'linf' and 'l2'")
    shape = tuple(shape)
    d = torch.randn(shape, generator=g)
    r = torch.rand((shape[0],), generator=g)
    nrm = d.reshape(shape[0], -1).norm(p=2, dim=1) + 1e-10
    return d * (r / nrm).reshape((-1,) + (1,) * (len(shape) - 1))


def attack(net, imgs, eps, steps, *, target=None, vgg=None, alpha=0.01, random_start=False,
           seed=0, start_noise=None, norm="linf", momentum=None, loss="gan_vgg", loss_scale=None,
           lr=0.01, cw_c=1e-4, return_info=False, group=None, ti_kernel=None, ti_nsig=3.0,
           di_prob=None, di_resize_rate=0.9, di_schedule=None, nesterov=False, si_scales=None,
           pi_amplification=None, pi_kernel=3, pi_project=1.0, jpeg_quality=None,
           jpeg_grad="cubic", vt_samples=None, vt_beta=1.5, vt_first_image=0, sign_hunter=False,
           universal=False,
           spsa_samples=None, spsa_delta=0.01, spsa_first_image=0, apgd=False):
    """Craft adversarial images against the GAN fusion pipeline.

    net     pSp-like bundle: net.encoder, net.decoder (.size), net.latent_avg, net.opts
            (built by ``gfa_amd.networks.build_net``); may also carry ``net.vgg``.
    imgs    (N,3,S,S) float tensor in [-1,1] (reference normalisation, transforms_config.py:29-31),
            on CPU or GPU; not modified.
    eps     radius in [0,1] pixel units: L∞ for norm='linf' (8/255 in the reference's PGD call,
            interpolation.py:1343), per-image L2 for norm='l2'.
    steps   iterations (PGD: 1 with alpha=eps and random_start=False is FGSM).
    alpha   PGD step in [0,1] pixel units; default 0.01 = the reference's PGD call
            (interpolation.py:1343; torchattacks' own default is 2/255). That default is sized
            for L∞: for norm='l2' the step is an L2 length, pass alpha ≈ eps/5 (torchattacks
            PGDL2's own ratio, eps = 1.0 with alpha = 0.2).
    start_noise  optional host tensor of imgs' shape for random_start (default: drawn from
            ``seed`` by ``make_start_noise(imgs.shape, seed, norm)``: U(-1,1) per element for
            'linf', a point of the unit L2 ball per image for 'l2').
    target  white-box target image(s) (N or 1, 3, S, S) — the ``img_target`` of optimize_vgg.
    norm    'linf'  — torchattacks PGD rule (interpolation.py:62-96) on the objective;
            'l2'    — torchattacks PGDL2 rule, per image in [-1,1] space (e = 2·eps, a = 2·alpha):
                      x ← x + a·(−∇L)/(‖∇L‖₂ + 1e-10); d = x − x0;
                      x ← clamp(x0 + d·min(e/‖d‖₂, 1), −1, 1)   (AttackEngine.run_l2);
            'adam'  — optimize_vgg literal (interpolation.py:743-843): Adam(lr) on the pixels,
                      no ε-ball (eps is ignored and may be None);
            'l2_cw' — torchattacks C&W L2 (interpolation.py:98-193) with f = the objective,
                      c = cw_c, Adam(lr) in tanh space (eps ignored; see AttackEngine.run_cw).
    momentum  None (default): the plain rule of ``norm``. μ ≥ 0, with norm='linf' only: the
            torchattacks MIFGSM rule, per image with a momentum buffer m (0 at the start):
                      ĝ = (−∇L)/mean|∇L|; m ← ĝ + μ·m;
                      x ← clamp(x0 + clamp(x + a·sign(m) − x0, −e, e), −1, 1)
            (AttackEngine.run_mi; torchattacks' default decay is 1.0). An image whose gradient
            is entirely zero raises FloatingPointError instead of staying frozen.
    ti_kernel  None (default): no smoothing. An odd integer K in 1 … 63, with norm='linf' or 'l2':
            the translation-invariant attack, the pixel gradient smoothed per plane by the
            K × K Gaussian W = outer(w, w), w = ti_gaussian_taps(K, ti_nsig) (zero padded, on
            the fused HIP blur). norm='linf' is the torchattacks TIFGSM rule with
            diversity_prob = 0 (momentum=None means μ = 0, torchattacks' default decay):
                      ĝ = W ⋆ (−∇L); ĝ ← ĝ / mean|ĝ|; m ← ĝ + μ·m;
                      x ← clamp(x0 + clamp(x + a·sign(m) − x0, −e, e), −1, 1)
            norm='l2' takes the PGDL2 step above along W ⋆ ∇L and its L2 norm
            (AttackEngine.run_mi / run_l2 with ti_taps).
    ti_nsig  the Gaussian's half-width in standard deviations (torchattacks' nsig, 3).
    di_prob  None (default): no input diversity. p in [0, 1], with norm='linf' or 'l2': the
            diverse-input attack (torchattacks DIFGSM; TIFGSM together with ti_kernel, whose own
            default is diversity_prob = 0.5). Per step, with probability p, one random
            resize-and-pad D serves the whole batch (fused HIP kernels, both directions):
                      D(x) = zero_pad(bilinear(x, (rnd, rnd), align_corners=False), top, left)
            with int(S·di_resize_rate) <= rnd <= S − 1 and the pad offsets drawn as torchattacks
            does. The whole objective is evaluated at D(x) (the targets stay those of x0 and t)
            and the step follows g = Dᵀ ∇L(D x); then the smoothing, if any, and the update of
            ``norm`` run as without it: the MIFGSM rule for 'linf' (momentum=None means μ = 0,
            torchattacks DIFGSM's / TIFGSM's default decay), PGDL2 for 'l2'. The draws come from
            ``make_di_schedule(steps, S, di_resize_rate, di_prob, seed)`` before the loop.
    di_resize_rate  torchattacks' resize_rate, below 1 (default 0.9): the smallest resized edge is
            int(S·rate). Rates >= 1 would change the networks' input size and are rejected.
    di_schedule  an explicit host (steps, 4) integer schedule of rows (rnd, top, left, apply)
            instead of the seeded draws (``check_di_schedule``; rnd = S is the identity).
    si_scales  None (default) or 1: no scale copies. An integer n in 2 … 8 (SI_MAX_SCALES;
            torchattacks SINIFGSM's default m is 5), with norm='linf' or 'l2': the scale-invariant
            attack. Every step follows the mean gradient over n scaled copies of the iterate,
                      g = (1/n)·Σ_i 2^-i·∇L(S_i(x)),  S_i(x) = (x + 1)·2^-i − 1,  i = 0 … n − 1
            (fused HIP kernels for the copies and their accumulation; n gradient passes per
            step). S_i is torchattacks' p / 2^i on p = (x + 1)/2 ∈ [0,1]: in these [-1,1] units
            the copies scale towards black (−1 is the fixed point). Lin et al.'s own code scaled
            images that were already in [-1,1] and so scaled towards mid-grey; torchattacks is
            followed here. The whole objective is evaluated at the copy (the targets stay those
            of x0 and t), as with di_prob. norm='linf' takes the MIFGSM rule (momentum=None means
            μ = 0), 'l2' the PGDL2 rule. With input diversity ONE resize-and-pad D per step
            serves all n copies, so the adjoint runs once: g = Dᵀ (1/n)·Σ_i 2^-i·∇L(D S_i(x));
            the original SI-DIM code drew a fresh D per copy. Order within a step: look-ahead,
            scale copy, D, the networks, the accumulation, Dᵀ, the TI smoothing, the update.
    nesterov  False (default). True, with norm='linf' and an explicit momentum μ > 0 only: the
            torchattacks NIFGSM look-ahead — the step's gradient (or every scale copy) is taken
            at x + μ·a·m, m the momentum buffer, instead of at x (not clamped, as torchattacks;
            μ·a is rounded once to fp32). No default μ is guessed: torchattacks' decay defaults
            differ between NIFGSM / SINIFGSM (1.0) and TIFGSM / DIFGSM (0.0). At step 1 m = 0, so
            the look-ahead first acts at step 2 (for fgsm() it is a no-op).
    pi_amplification  None (default): off. A finite β > 0, with norm='linf' only: the patch-wise
            attack (Gao, Zhang et al., "Patch-wise Attack for Fooling Deep Neural Network", ECCV
            2020; PI-FGSM, DI-TI-PI-FGSM together with di_prob and ti_kernel; the paper uses
            β = 10 against normally trained models), AttackEngine.run_pi. It changes the update,
            not the gradient: the step is amplified to β·a, and the part of the accumulated noise
            that overflows the ε-ball is handed to each pixel's neighbours by a uniform project
            kernel instead of being clipped away. With ab = fp32(fp32(β)·a), gm =
            fp32(fp32(pi_project)·ab), K = pi_kernel, and per image a momentum buffer m and the
            accumulated amplified noise A, both 0 at the start (also after a random start and an
            fp16 loss-scale re-run), per step, plane and pixel:
                      ĝ = (−g)/mean|g|;  m ← ĝ + μ·m;  s = sign(m);  A' = A + ab·s
                      C = sign(A')·max(|A'| − e, 0)        (the cut noise; 0 inside the ball)
                      S = Σ C over the K × K window without its centre, zero padded
                      p = gm·sign(S);  A ← A' + p
                      x ← clamp(x0 + clamp(x + ab·s + p − x0, −e, e), −1, 1)
            one fused HIP kernel per step (momentum=None means μ = 0). Only the sign of S is
            used, so the paper's kernel weights 1/(K² − 1) drop out and S is a chain of fp32
            additions in a fixed order (window rows, then columns, ascending): the result is
            bit-reproducible and an image's result depends on neither the batch nor the world
            size. The paper's test ‖A'‖∞ ≥ ε is implied by C = 0; the authors' clip of C at 10000
            is unreachable (|A| ≤ steps·(ab + gm)) and left out. g is whatever the other keywords
            make it: it composes with momentum, nesterov (whose look-ahead becomes x + μ·ab·m),
            ti_kernel, di_prob / di_schedule, si_scales, vt_samples and random_start at no extra
            cost. It does not combine with apgd, universal, sign_hunter or spsa_samples.
            pi_project = 0 gives the MI attack with alpha replaced by β·alpha, and β = 1 with
            steps·alpha ≤ eps the MI attack itself, both bit for bit.
    pi_kernel  the project kernel's edge K (default 3, the paper's), an odd integer in 3 … 15.
            Needs pi_amplification.
    pi_project  the paper's project factor γ as a multiple of β·α (default 1.0, the paper's
            γ = β·α), finite and ≥ 0. Needs pi_amplification.
    vt_samples  None (default): no variance tuning. An integer N in 1 … 32 (VT_MAX_SAMPLES;
            torchattacks VMIFGSM's default N is 5), with norm='linf' only: the variance-tuned
            attack (Wang & He; VNI-FGSM together with nesterov). It takes the MIFGSM rule
            (momentum=None means μ = 0, as with ti_kernel / di_prob / si_scales; torchattacks
            VMIFGSM defaults to decay 1.0). Per step k, with v = 0 and m = 0 at the start:
                      x_nes = x + μ·a·m if nesterov else x
                      g  = G(x_nes);  gt = g + v;  ĝ = −(W ⋆ gt)/mean|W ⋆ gt|;  m ← ĝ + μ·m
                      gv = (1/N)·Σ_i G(x_nes + r·u_{k,i}),  r = vt_beta·e,  i = 0 … N − 1
                      v  ← gv − g;  x ← clamp(x0 + clamp(x + a·sign(m) − x0, −e, e), −1, 1)
            G is the step's gradient before the smoothing W (none without ti_kernel): the plain
            gradient, Dᵀ ∇L(D ·) with di_prob and the mean over the scale copies with si_scales,
            one D per step serving x_nes and all its neighbours — the composition Wang & He
            report as their strongest. N + 1 gradient passes per step; the last step draws no
            neighbours (v is never read again), so one step is the plain MI step. The noise
            u_{k,i} ∈ (−1, 1) is counter-based and stateless (Philox4x32-10 in the HIP kernel): a
            pure function of (seed, global image index, k, i, element index), keyed with
            (seed + VT_SEED_OFFSET) mod 2^64. Reruns are bit-identical, there is no host
            synchronisation, an fp16 loss-scale re-run replays the same draws from v = 0, and an
            image's result depends on neither the batch nor the world size. The values are not
            torchattacks' (torch.rand_like on the attack device), the distribution is.
    vt_beta  torchattacks' beta (default 1.5), finite and > 0: the neighbourhood's radius is
            vt_beta·eps per pixel (rounded to fp32 once, as fp32(vt_beta)·e).
    vt_first_image  the global index of imgs[0] (default 0), an integer ≥ 0: image n draws the
            noise of image vt_first_image + n, so attacking a slice of a batch with its offset
            gives the rows of the whole batch (``dist.attack_distributed`` passes the shard's).
    sign_hunter  False (default). True, with norm='linf' only: SignHunter (Al-Dujaili & O'Reilly,
            "Sign Bits Are All You Need for Black-Box Attacks", ICLR 2020), the deterministic
            score-based BLACK-BOX attack, AttackEngine.run_sign_hunter. The attacker sees the
            objective's value only, one forward pass per query, and draws no random number.
            ``alpha`` is not used. Every iterate is a vertex of the ε-ball; with e = fp32(2·eps),
            s ∈ {−1, +1} per element and flat element index j in NCHW order, per image:
                      query 0:  s = +1;  x = clamp(x0 + e·s, −1, 1);  L_best = L(x)
                      query k = 1 … steps:  flip s on [lo, hi) = row k − 1 of
                                sh_schedule(steps, 3·S²);  x = clamp(x0 + e·s, −1, 1)
                                L(x) < L_best: keep the flip, L_best = L(x);  else flip back
            A tie or a NaN is a rejection. ``sh_schedule`` is divide and conquer: the whole
            plane, its halves, quarters, … down to single elements, then again from the whole
            plane. The result is every image's best vertex; steps + 1 queries per image
            (info["queries"]; steps = 0 returns a copy of imgs without a query). The signs are
            kept in an int8 plane — a clamped element of x no longer shows its sign — and one
            fused HIP kernel per query flips the new segment and, in the images that rejected
            the previous query, flips that one back, touching those two segments only; a
            one-thread-per-image kernel takes the decision. Nothing is read back to the host
            inside the loop. The attack is deterministic by construction: reruns are
            bit-identical and an image's result depends on neither the batch nor the world size.
            The clean image is not a candidate (L(x0) is never queried). A non-finite objective
            raises FloatingPointError. It does not combine with momentum, nesterov, ti_kernel,
            di_prob / di_schedule, si_scales, vt_samples, spsa_samples, pi_amplification, apgd,
            universal or random_start. With return_info, info["sign_hunter"] holds ``loss`` (steps + 1, N:
            the objective of every query), ``best`` (N,) and ``accepted`` (N,), the number of
            flips kept, as host tensors (False without the keyword).
    universal  False (default): one perturbation per image. True, with norm='linf' only: ONE
            perturbation δ (1,3,S,S), ‖δ‖∞ ≤ e, fitted on the whole batch, that steers the
            fusion of any of its images (and, it is hoped, of held-out ones:
            ``apply_universal(imgs, delta)``) towards the target. δ₀ = 0, or clamp(e·u, −e, e)
            with random_start, u ONE draw ``make_start_noise((1,3,S,S), seed, "linf")`` or a
            ``start_noise`` of that shape. Per step, with x_n = clamp(x0_n + δ, −1, 1):
                      ĝ_n = (−∇L(x_n)) / mean|∇L(x_n)|             (the MIFGSM normalisation)
                      A   = Σ_n round_half_even(ĝ_n·2^24)          (int64, over ALL images)
                      δ   ← clamp(δ + a·sign(A), −e, e);  x_n ← clamp(x0_n + δ, −1, 1)
            Every image is normalised by its own mean |∇L|, so no image dominates and the fp16
            loss scale cancels. This is the one attack whose images are not independent: the sum
            over them is taken in 2^-24 fixed point on exact integer sums (fused HIP kernels),
            which are associative, so the result is bit-reproducible and depends on neither the
            order of the images, nor the batch split, nor the world size — a float sum could not
            promise that. The range needs images × 3·S² < 2^37, counted over the whole job
            (``check_universal_count``). An image whose gradient is entirely zero or non-finite
            raises FloatingPointError (fp16: after the loss-scale re-runs, which restart from
            δ₀). It does not combine with momentum, nesterov, ti_kernel, di_prob / di_schedule,
            si_scales, vt_samples, spsa_samples, pi_amplification or apgd. Returns the batch
            clamp(x0 + δ); with
            return_info, info["universal"] holds ``delta`` (1,3,S,S, on the input's device) and
            ``linf`` = max|δ| in [-1,1] units.
    spsa_samples  None (default): white-box, every rule above reads ∇L. An integer q in 1 … 256
            (SPSA_MAX_SAMPLES), with norm='linf' or 'l2': SPSA, the score-based BLACK-BOX attack
            (Spall 1992; Uesato et al. 2018; torchattacks SPSA's estimator). The attacker sees
            the objective's value only: no backward pass runs. Per step k, with q antithetic
            pairs i = 0 … q − 1 and d = fp32(2·spsa_delta):
                      v_{k,i} = ±1 per element (Rademacher)
                      x⁺ = clamp(x + d·v, −1, 1);  x⁻ = clamp(x − d·v, −1, 1)
                      ĝ = (1/q)·Σ_i ((L(x⁺) − L(x⁻))/(2·d))·v_{k,i}
            and ĝ takes the update of ``norm`` unchanged: 'linf' the MIFGSM rule (momentum=None
            means μ = 0, the plain sign step), 'l2' the PGDL2 rule. 2·q queries per image per
            step (info["queries"] = 2·q·steps); expect the step to cost 2·q forward passes. The
            directions are counter-based and stateless (Philox4x32-10 in the HIP kernels, bit 31
            of the element's word): a pure function of (seed, global image index, k, i, element
            index), keyed with (seed + SPSA_SEED_OFFSET) mod 2^64, never stored — one fused
            kernel writes both probes and another regenerates v while it accumulates. Reruns are
            bit-identical, there is no host synchronisation, and an image's result depends on
            neither the batch nor the world size. torchattacks SPSA feeds the same estimate to
            Adam; here it feeds the project's own updates. It does not combine with nesterov,
            ti_kernel, di_prob / di_schedule, si_scales, vt_samples, pi_amplification or apgd:
            each of those transforms or reuses a true gradient, or has an update of its own. A non-finite objective raises
            FloatingPointError; so does, under 'linf', a step whose pairs all return
            L(x⁺) = L(x⁻) exactly (an all-zero estimate, 0/0).
    spsa_delta  the probe radius in [0,1] pixel units (default 0.01, torchattacks' delta), finite
            and > 0. The probes are clamped to valid images but not to the ε-ball.
    spsa_first_image  the global index of imgs[0] (default 0), an integer ≥ 0: image n takes the
            directions of image spsa_first_image + n (``dist.attack_distributed`` passes the
            shard's), as vt_first_image.
    apgd    False (default). True, with norm='linf' only (the L2 form is not implemented):
            Auto-PGD (Croce & Hein 2020; torchattacks APGD with norm='Linf', eot_iter=1, one
            run) on the objective, AttackEngine.run_apgd. ``alpha`` is not used: every image has
            a step size of its own, eta = 2·e at the start, with momentum on the iterate
            (a = 1 at the first step, 0.75 after):
                      z = clamp(min(max(x − eta·sign(∇L), x0 − e), x0 + e), −1, 1)
                      x ← clamp(min(max(x + a·(z − x) + (1 − a)·(x − x_old), x0 − e), x0 + e), −1, 1)
            The per-image objective comes out of the same pass as the gradient. At the
            checkpoints of ``apgd_schedule(steps)`` (windows of k steps, k shrinking from
            0.22·steps to 0.06·steps) an image whose objective fell in at most floor(0.75·k) of
            the window's steps, or that found no new best since a checkpoint that did not
            halve, halves its eta and restarts from its best iterate and that iterate's
            gradient. The result is the BEST iterate of every image (the start included), not
            the last; steps + 1 gradient passes. Step sizes, counters, best points and the
            conditional copies all live on the device (fused HIP kernels): no per-step host
            synchronisation; an fp16 loss-scale re-run restarts all of it. One deviation from
            torchattacks: at the first checkpoint its check_oscillation compares step 0 with
            loss_steps[-1], a zero row reached by negative indexing; here step 0 is compared
            with the objective at the starting point, the paper's condition. It does not
            combine with momentum, nesterov, ti_kernel, di_prob / di_schedule, si_scales,
            vt_samples or pi_amplification. With return_info, info["apgd"] holds ``loss`` and ``step_size``
            (steps + 1, N: the start, then after every step), ``best_step`` (0 = the start,
            i + 1 = step i) and ``halvings`` per image, as host tensors.
    jpeg_quality  None (default): the attack assumes the pipeline reads the fp32 tensor it returns.
            An integer q in 1 … 100, with norm='linf' or 'l2': the JPEG-robust attack, for an
            adversarial image that is saved as a .jpg before the pipeline reads it (as the
            reference saves its inputs, interpolation.py:323-325). Every step follows the gradient
            of the objective at J(x), the round trip of the iterate through a baseline 4:4:4 JPEG
            of quality q (8-bit pixels, JFIF YCbCr, 8 × 8 DCT, the IJG-scaled Annex K tables
            ``jpeg_quant_tables(q)``; fused HIP kernels, the arithmetic in include/miattack.h).
            The stage sits closest to the pixels; with x̃ = x + μ·a·m under nesterov, else x:
                      g = W ⋆ J′(x̃)ᵀ Dᵀ (1/n)·Σ_i 2^-i·∇L(D S_i(J(x̃)))
            J runs once per gradient, its adjoint once, after Dᵀ and before the smoothing W; the
            targets stay those of x0 and t. norm='linf' takes the MIFGSM rule (momentum=None
            means μ = 0, as with ti_kernel / di_prob), 'l2' the PGDL2 rule. It composes with
            momentum, nesterov, ti_kernel, di_prob / di_schedule, si_scales, vt_samples,
            pi_amplification and random_start, and not with apgd, universal, sign_hunter,
            spsa_samples or norm 'adam' / 'l2_cw'. The image returned is the UNCOMPRESSED iterate,
            which the caller then saves; ``jpeg_compress(adv, q)`` is what the pipeline will see.
            4:2:0 chroma subsampling and sizes that are no multiple of 8 are not implemented.
    jpeg_grad  how the gradient passes the coefficient rounding of J (needs jpeg_quality):
            'cubic' (default) — the adjoint of the surrogate round(v) + (v − round(v))³ of Shin &
            Song (2017), derivative 3·(v − round(v))², one fused HIP kernel that recomputes the
            coefficients from x̃; 'ste' — straight through, J′ᵀ taken as the identity (BPDA).
    group   process group of a data-parallel job (``dist.attack_distributed``): the fp16
            loss-scale re-run decision is all-reduced over it so every shard runs at one λ.
    Returns the adversarial images on the input's device (fp32), and a dict if return_info
    (with jpeg_quality it holds ``loss_jpeg``, the per-image objective at J(adv), next to ``loss``).
    """
    if norm not in NORMS:
        raise ValueError(f"norm must be one of {NORMS}")
    if not isinstance(sign_hunter, (bool, np.bool_)):
        raise ValueError("sign_hunter must be True or False")
    sign_hunter = bool(sign_hunter)
    if sign_hunter:
        if norm != "linf":
            raise ValueError("sign_hunter (SignHunter) is implemented for norm='linf' only")
        mixed = [name for name, on in (
            ("momentum", momentum is not None),
            ("nesterov", not isinstance(nesterov, (bool, np.bool_)) or bool(nesterov)),
            ("ti_kernel", ti_kernel is not None), ("di_prob", di_prob is not None),
            ("di_schedule", di_schedule is not None), ("si_scales", si_scales is not None),
            ("vt_samples", vt_samples is not None), ("spsa_samples", spsa_samples is not None),
            ("pi_amplification", pi_amplification is not None),
            ("jpeg_quality", jpeg_quality is not None),
            ("apgd", not isinstance(apgd, (bool, np.bool_)) or bool(apgd)),
            ("universal", not isinstance(universal, (bool, np.bool_)) or bool(universal)),
            ("random_start", bool(random_start))) if on]
        if mixed:
            raise ValueError(f"sign_hunter does not combine with {', '.join(mixed)}: it reads "
                             "the objective's value only and every iterate is a vertex of the "
                             "ball, reached by sign flips from s = +1")
    if not isinstance(universal, (bool, np.bool_)):
        raise ValueError("universal must be True or False")
    universal = bool(universal)
    if universal:
        if norm != "linf":
            raise ValueError("universal (one perturbation per batch) is implemented for "
                             "norm='linf' only")
        mixed = [name for name, on in (
            ("momentum", momentum is not None),
            ("nesterov", not isinstance(nesterov, (bool, np.bool_)) or bool(nesterov)),
            ("ti_kernel", ti_kernel is not None), ("di_prob", di_prob is not None),
            ("di_schedule", di_schedule is not None), ("si_scales", si_scales is not None),
            ("vt_samples", vt_samples is not None), ("spsa_samples", spsa_samples is not None),
            ("pi_amplification", pi_amplification is not None),
            ("jpeg_quality", jpeg_quality is not None),
            ("apgd", not isinstance(apgd, (bool, np.bool_)) or bool(apgd)),
            ("sign_hunter", sign_hunter)) if on]
        if mixed:
            raise ValueError(f"universal does not combine with {', '.join(mixed)}: the shared "
                             "step follows the sign of the summed normalised gradients only")
    if not isinstance(apgd, (bool, np.bool_)):
        raise ValueError("apgd must be True or False")
    apgd = bool(apgd)
    if apgd:
        if norm == "l2":
            raise ValueError("apgd (Auto-PGD): the L2 form is not implemented, use norm='linf'")
        if norm != "linf":
            raise ValueError("apgd (Auto-PGD) is implemented for norm='linf' only")
        mixed = [name for name, on in (
            ("momentum", momentum is not None), ("nesterov", not isinstance(nesterov, (bool, np.bool_)) or bool(nesterov)),
            ("ti_kernel", ti_kernel is not None), ("di_prob", di_prob is not None),
            ("di_schedule", di_schedule is not None), ("si_scales", si_scales is not None),
            ("vt_samples", vt_samples is not None),
            ("pi_amplification", pi_amplification is not None),
            ("jpeg_quality", jpeg_quality is not None), ("sign_hunter", sign_hunter)) if on]
        if mixed:
            raise ValueError(f"apgd (Auto-PGD) does not combine with {', '.join(mixed)}: it has "
                             "its own momentum and step-size rule")
    if momentum is not None:
        if norm != "linf":
            raise ValueError("momentum (MI-FGSM) is implemented for norm='linf' only")
        if not float(momentum) >= 0:
            raise ValueError("momentum must be >= 0")
    ti_taps = None
    if ti_kernel is not None:
        if norm not in ("linf", "l2"):
            raise ValueError("ti_kernel (TI-FGSM) is implemented for norm='linf' and 'l2' only")
        ti_taps = ti_gaussian_taps(ti_kernel, ti_nsig)
    use_di = di_prob is not None or di_schedule is not None
    if use_di and norm not in ("linf", "l2"):
        raise ValueError("input diversity (DI-FGSM) is implemented for norm='linf' and 'l2' only")
    n_si = _check_si_scales(si_scales)
    if si_scales is not None and norm not in ("linf", "l2"):
        raise ValueError("si_scales (SI-FGSM) is implemented for norm='linf' and 'l2' only")
    if not isinstance(nesterov, (bool, np.bool_)):
        raise ValueError("nesterov must be True or False")
    nesterov = bool(nesterov)
    if nesterov:
        if norm != "linf":
            raise ValueError("nesterov (NI-FGSM) is implemented for norm='linf' only")
        if momentum is None or not float(momentum) > 0:
            raise ValueError("nesterov (NI-FGSM) needs an explicit momentum > 0 (torchattacks "
                             "NIFGSM's default decay is 1.0)")
    n_vt = None
    if vt_samples is not None:
        n_vt = _check_vt_samples(vt_samples)
        if norm != "linf":
            raise ValueError("vt_samples (VMI-FGSM) is implemented for norm='linf' only")
    vt_beta = _check_vt_beta(vt_beta)
    _check_vt_first_image(vt_first_image, 0)
    n_spsa = None
    if spsa_samples is not None:
        n_spsa = _check_spsa_samples(spsa_samples)
        if norm not in ("linf", "l2"):
            raise ValueError("spsa_samples (SPSA) is implemented for norm='linf' and 'l2' only")
        mixed = [name for name, on in (
            ("nesterov", nesterov), ("ti_kernel", ti_kernel is not None),
            ("di_prob", di_prob is not None), ("di_schedule", di_schedule is not None),
            ("si_scales", si_scales is not None), ("vt_samples", vt_samples is not None),
            ("pi_amplification", pi_amplification is not None),
            ("jpeg_quality", jpeg_quality is not None),
            ("apgd", apgd), ("sign_hunter", sign_hunter)) if on]
        if mixed:
            raise ValueError(f"spsa_samples (SPSA) does not combine with {', '.join(mixed)}: "
                             "they transform or reuse a true gradient, SPSA reads the "
                             "objective's value only")
    spsa_delta = _check_spsa_delta(spsa_delta)
    _check_spsa_first_image(spsa_first_image, 0)
    pi_kernel, pi_project = _check_pi_kernel(pi_kernel), _check_pi_project(pi_project)
    if pi_amplification is None:
        if pi_kernel != 3 or pi_project != 1.0:
            raise ValueError("pi_kernel / pi_project need pi_amplification (the patch-wise attack "
                             "is off without it)")
    else:
        _check_pi_amplification(pi_amplification)
        if norm != "linf":
            raise ValueError("pi_amplification (PI-FGSM) is implemented for norm='linf' only")
    jpeg_grad = _check_jpeg_grad(jpeg_grad)
    if jpeg_quality is None:
        if jpeg_grad != "cubic":
            raise ValueError("jpeg_grad needs jpeg_quality (the JPEG stage is off without it)")
    else:
        jpeg_quality = _check_jpeg_quality(jpeg_quality)
        if norm not in ("linf", "l2"):
            raise ValueError("jpeg_quality (the JPEG-robust attack) is implemented for "
                             "norm='linf' and 'l2' only")
    if loss != "gan_vgg":
        raise ValueError("only loss='gan_vgg' (the optimize_vgg objective) is implemented")
    size = net.decoder.size
    if jpeg_quality is not None and size % 8:
        raise ValueError("jpeg_quality needs an image size that is a multiple of 8 (JPEG's edge "
                         "replication is not implemented)")
    _check_images(imgs, size, "imgs")
    vt_first_image = _check_vt_first_image(vt_first_image, imgs.shape[0])
    spsa_first_image = _check_spsa_first_image(spsa_first_image, imgs.shape[0])
    if universal:
        check_universal_count(imgs.shape[0], 3 * size * size)
        if imgs.shape[0] < 1:
            raise ValueError("universal needs at least one image")
        if random_start and start_noise is not None and (
                not torch.is_tensor(start_noise) or tuple(start_noise.shape) != (1, 3, size, size)):
            raise ValueError("universal: start_noise must have the shape (1,3,S,S), one draw for "
                             "the shared perturbation")
    if target is None:
        target = getattr(net, "default_target", None)
    if target is None:
        raise ValueError("a white-box target image is required (optimize_vgg img_target)")
    if target.dim() == 4 and target.shape[0] == 1 and imgs.shape[0] > 1:
        target = target.expand(imgs.shape[0], -1, -1, -1)
    _check_images(target, size, "target")
    if target.shape[0] != imgs.shape[0]:
        raise ValueError("target batch must be 1 or match imgs")
    if steps < 0 or int(steps) != steps:
        raise ValueError("need integer steps >= 0")
    di = None
    if use_di:
        if di_prob is not None:
            _check_di_prob(di_prob)
        if di_schedule is not None:
            di = check_di_schedule(di_schedule, steps, size)
        else:
            di = make_di_schedule(int(steps), size, di_resize_rate, di_prob, seed)
    if sign_hunter:
        if not (eps is not None and eps > 0):
            raise ValueError("sign_hunter needs eps > 0")
    elif norm in ("linf", "l2") and not (eps is not None and eps > 0 and alpha > 0):
        raise ValueError("PGD needs eps > 0 and alpha > 0")
    if pi_amplification is not None:
        pi_steps(alpha, pi_amplification, pi_project)  # the fp32 steps are finite, β·a > 0
    if norm in ("adam", "l2_cw") and not lr > 0:
        raise ValueError("lr must be > 0")
    if float(imgs.min()) < -1.0 or float(imgs.max()) > 1.0:
        raise ValueError("imgs must lie in [-1, 1]")
    vgg = vgg if vgg is not None else getattr(net, "vgg", None)
    if vgg is None:
        raise ValueError("a VGG feature network is required (optimize_vgg's vgg)")
    for name, part in (("net.encoder", getattr(net, "encoder", None)),
                       ("net.decoder", net.decoder), ("vgg", vgg)):
        if not hasattr(part, "impl"):
            raise ValueError(f"{name} must be a device network of this package "
                             "(networks.build_net / build_net_from_checkpoint, vgg16)")
    dev = net.decoder.device
    x0 = imgs.detach().to(dev, torch.float32).contiguous()
    t = target.detach().to(dev, torch.float32).contiguous()
    eng = AttackEngine(net.encoder.impl, net.decoder.impl, vgg.impl, loss_scale=loss_scale)
    eng.set_jpeg(jpeg_quality, jpeg_grad)  # the stage of every gradient the run_* below take
    noise = None
    if random_start:
        noise_shape = (1,) + tuple(x0.shape[1:]) if universal else tuple(x0.shape)
        if start_noise is None:
            start_noise = make_start_noise(noise_shape, seed, "l2" if norm == "l2" else "linf")
        if tuple(start_noise.shape) != noise_shape:
            raise ValueError("start_noise must have the shape of imgs")
        noise = start_noise.to(dev, torch.float32).contiguous()
    if sign_hunter:
        adv = eng.run_sign_hunter(x0, t, int(steps), float(eps), group=group)
    elif universal:
        adv = eng.run_universal(x0, t, int(steps), float(eps), float(alpha), random_start, noise,
                                group=group)
    elif n_spsa is not None:
        adv = eng.run_spsa(x0, t, int(steps), float(eps), float(alpha),
                           float(momentum) if momentum is not None else 0.0, norm, random_start,
                           noise, group=group, spsa_samples=n_spsa, spsa_delta=spsa_delta,
                           spsa_seed=(int(seed) + SPSA_SEED_OFFSET) % (1 << 64),
                           spsa_first_image=spsa_first_image)
    elif apgd:
        adv = eng.run_apgd(x0, t, int(steps), float(eps), random_start, noise, group=group)
    elif pi_amplification is not None:
        adv = eng.run_pi(x0, t, int(steps), float(eps), float(alpha), pi_amplification, pi_kernel,
                         pi_project, float(momentum) if momentum is not None else 0.0,
                         random_start, noise, group=group, ti_taps=ti_taps, di=di,
                         nesterov=nesterov, si_scales=n_si, vt_samples=n_vt, vt_beta=vt_beta,
                         vt_seed=(int(seed) + VT_SEED_OFFSET) % (1 << 64),
                         vt_first_image=vt_first_image)
    elif norm == "linf" and (momentum is not None or ti_taps is not None or di is not None
                             or n_si > 1 or n_vt is not None or jpeg_quality is not None):
        adv = eng.run_mi(x0, t, int(steps), float(eps), float(alpha),
                         float(momentum) if momentum is not None else 0.0, random_start, noise,
                         group=group, ti_taps=ti_taps, di=di, nesterov=nesterov, si_scales=n_si,
                         vt_samples=n_vt, vt_beta=vt_beta,
                         vt_seed=(int(seed) + VT_SEED_OFFSET) % (1 << 64),
                         vt_first_image=vt_first_image)
    elif norm == "linf":
        adv = eng.run(x0, t, int(steps), float(eps), float(alpha), random_start, noise,
                      group=group)
    elif norm == "l2":
        adv = eng.run_l2(x0, t, int(steps), float(eps), float(alpha), random_start, noise,
                         group=group, ti_taps=ti_taps, di=di, si_scales=n_si)
    elif norm == "adam":
        adv = eng.run_adam(x0, t, int(steps), lr=float(lr), group=group)
    else:
        adv = eng.run_cw(x0, t, int(steps), c=float(cw_c), lr=float(lr), group=group)
    adv = adv.to(imgs.device)
    if return_info:
        info = dict(loss=eng.loss(adv.to(dev)), steps=int(steps), eps=eps, alpha=alpha, norm=norm,
                    momentum=momentum, ti_kernel=ti_kernel, dtype=str(eng.dtype),
                    loss_scale=eng.loss_scale, rescales=eng.rescales, di_prob=di_prob,
                    di_resize_rate=di_resize_rate if di_prob is not None else None,
                    di_applied=int(di[:, 3].sum()) if di is not None else 0,
                    si_scales=si_scales, nesterov=nesterov, vt_samples=vt_samples,
                    vt_beta=vt_beta if vt_samples is not None else None,
                    spsa_samples=spsa_samples,
                    spsa_delta=spsa_delta if spsa_samples is not None else None,
                    sign_hunter=False, pi_amplification=pi_amplification,
                    pi_kernel=pi_kernel if pi_amplification is not None else None,
                    pi_project=pi_project if pi_amplification is not None else None,
                    queries=(2 * n_spsa * int(steps) if n_spsa is not None
                             else eng.sh_queries if sign_hunter else 0),
                    jpeg_quality=jpeg_quality,
                    jpeg_grad=jpeg_grad if jpeg_quality is not None else None,
                    loss_jpeg=(eng.loss(jpeg_compress(adv.to(dev), jpeg_quality))
                               if jpeg_quality is not None else None))
        if sign_hunter:
            info["sign_hunter"] = eng.sign_hunter_info()
        if universal:
            delta = eng.uap_delta.to(imgs.device)
            info["universal"] = dict(delta=delta, linf=float(delta.abs().max()))
        if apgd:
            info["apgd"] = eng.apgd_info()
        return adv, info
    return adv


def fgsm(net, imgs, eps, **kw):
    """FGSM = one PGD step with α = ε and no random start. Every other keyword is forwarded
    unchanged (nesterov's look-ahead is a no-op at the only step, where the momentum is 0; so is
    vt_samples, whose variance term is 0 there: plain FGSM; ``spsa_samples=q`` is the one-step
    black-box form, the sign of the SPSA estimate; ``universal=True`` is the one-step universal
    perturbation, δ = e·sign of the summed normalised gradients). ``apgd=True`` is rejected: one step
    of Auto-PGD (step size 2·e, the better of the start and the step returned) is not FGSM.
    ``sign_hunter=True`` is rejected too: SignHunter follows no gradient. So is ``jpeg_quality``.
    ``pi_amplification=β`` is forwarded, the one-step patch-wise attack: every pixel moves by
    β·ε·s, s the sign of its gradient, its overflow (β − 1)·ε·s (β > 1) votes in its neighbours'
    windows, and a pixel receives p = ±pi_project·β·ε by the sign of the votes it gets before the
    ε-clip. The result is clamp(x0 + clamp(β·ε·s + p, −ε, ε)): FGSM's x0 + ε·s where the
    neighbours agree with the pixel or pi_project < 1, about x0 itself where they outvote it at
    pi_project = 1 (the two terms cancel), and x0 − ε·s beyond. β ≤ 1 cuts nothing and gives the
    step β·ε·s."""
    if kw.get("sign_hunter"):
        raise ValueError("fgsm() takes no sign_hunter: SignHunter follows no gradient, one flip "
                         "of it is not FGSM; call attack(..., steps=1, sign_hunter=True) for that")
    if kw.get("apgd"):
        raise ValueError("fgsm() takes no apgd: one step of Auto-PGD is not FGSM; call "
                         "attack(..., steps=1, apgd=True) for that")
    if kw.get("jpeg_quality") is not None:
        raise ValueError("fgsm() takes no jpeg_quality: the JPEG-robust attack is iterative; call "
                         "attack(..., steps=1, jpeg_quality=q) for one step of it")
    kw.pop("alpha", None)
    kw.pop("random_start", None)
    return attack(net, imgs, eps, 1, alpha=eps, random_start=False, **kw)


def algorithmic_flops_per_image_step(synth, vgg, encoder=None):
    """GEMM work one PGD iteration needs per image: G ×2 (forward + input gradient) + VGG ×4
    (two calls, forward + input gradient each) + the e4e encoder ×2 (forward + input gradient)
    when it is the real one (the linear stand-in's FLOPs are excluded).

    SURVEY.md §8d counted G ×3 with a separate style-gradient GEMM. The kernels never form the
    per-sample weight gradient: ∂L/∂s[n][ci] = Σ_p x[n,p,ci]·(Wᵀg)[n,p,ci] is a dot product
    over the dgrad output the input gradient computes anyway (2·H·W·Cin FLOP per layer, the
    `sdot` epilogue), so crediting it as a third GEMM would overstate the work by ~13 %."""
    enc = 2 * getattr(encoder, "flops_fwd_per_image", 0) if encoder is not None else 0
    return 2 * synth.flops_fwd_per_image + 4 * vgg.flops_fwd_per_image + enc

