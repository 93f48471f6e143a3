"""Auto-PGD (Croce & Hein 2020; torchattacks APGD, L∞): the fused update kernel against its fp32
reference bit for bit (tests/apgd_ref.py), the per-image control and copy kernels against the
pure-Python control rule on scripted objectives, one engine step against the fp64 oracle, and the
attack end to end at 32² — its decisions replayed from the recorded objectives, halvings that are
shown to occur on the oracle's own trajectory first, fp16 with a forced loss-scale re-run, and the
untouched existing paths.

All image-space quantities are in [-1,1] units (e = 2·eps)."""
import numpy as np
import pytest
import torch

import apgd_ref
from gpu_helpers import free, seeded, to64
from test_gpu_di import offset_copy
from test_gpu_si import stable_mask
from test_gpu_ti import ALPHA, EPS, SIZE, check_linf, images

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32
IMG_SCALES = (1e4, 1.0, 1e-4)  # per-image gradient scales: cross-image mixing cannot hide
# plane = 3·S²: 192 (one partial block), 3267 (no multiple of 4: the scalar form, a partial last
# group), 50700 (50 slots per image), 12288 (12 slots)
SIZES = (8, 33, 130, 64)
STEPS = 10
NAN = float("nan")


def f32(v):
    return float(np.float32(v))


E = f32(2 * EPS)
ETAS = (f32(2 * E), E, f32(E / 8))  # per-image step sizes


def bits(t):
    return t.contiguous().view(torch.int32)


_inputs = {}


def case(S):
    """Per size, computed once and shared (CPU fp32): x0; x inside, on and outside the faces of
    the ball; x_old near x; g with per-image scales and exact zeros planted."""
    if S not in _inputs:
        shape = (3, 3, S, S)
        x0 = seeded(700 + S, shape)                                      # up to the range's ends
        x = x0 + torch.tensor(E) * (1.5 * seeded(800 + S, shape))        # a third lies outside
        flat, f0 = x.reshape(-1), x0.reshape(-1)
        flat[0::7] = (f0 + torch.tensor(E))[0::7]                        # on the upper face
        flat[3::7] = (f0 - torch.tensor(E))[3::7]                        # on the lower face
        x_old = x + torch.tensor(f32(E / 2)) * seeded(900 + S, shape)
        g = seeded(1000 + S, shape) * torch.tensor(IMG_SCALES, dtype=F32).reshape(3, 1, 1, 1)
        g.reshape(-1)[0::5] = 0.0
        g.reshape(-1)[2::11] = -0.0
        _inputs[S] = dict(x0=x0, x=x.contiguous(), x_old=x_old, g=g,
                          eta=torch.tensor(ETAS, dtype=F32))
    return _inputs[S]


def update(c, a, dev, off=(), g=None):
    """(x, x_old, nonfinite) of mia_apgd_update on device copies of a case; ``off``: the names
    that get a 4-byte-offset buffer (the scalar form)."""
    from gfa_amd import ops
    t = {k: (offset_copy(v.to(dev)) if k in off else v.to(dev).clone()) for k, v in c.items()}
    if g is not None:
        t["g"] = g.to(dev)
    nf = torch.zeros(3, dtype=I32, device=dev)
    ops.apgd_update(t["x"], t["x_old"], t["x0"], t["g"], t["eta"], a, E, nonfinite=nf)
    return t["x"], t["x_old"], nf


@pytest.mark.parametrize("a", [1.0, 0.75])
@pytest.mark.parametrize("S", SIZES)
def test_apgd_update_is_the_reference_bit_for_bit(cuda, S, a):
    """x and x_old equal the fp32 reference bit for bit, per-image step sizes and gradient scales,
    exact zeros in g, x on and outside the faces; x_old afterwards is the old x; the result is
    inside the ball and the range; reruns are bit-identical; an image alone gives its row; a
    4-byte-offset copy of any buffer (the scalar form) gives the same bits."""
    c = case(S)
    want, want_old = apgd_ref.update(c["x"], c["x_old"], c["x0"], c["g"], c["eta"], a, E)
    assert torch.equal(want_old, c["x"])
    outside = ((c["x"] - c["x0"]).abs() > E).float().mean().item()
    onface = ((c["x"] == c["x0"] + E) | (c["x"] == c["x0"] - E)).float().mean().item()
    assert outside > 0.15 and onface > 0.2 and (c["g"] == 0).float().mean().item() > 0.2
    x, x_old, nf = update(c, a, cuda)
    assert torch.equal(bits(x.cpu()), bits(want)), (S, a)
    assert torch.equal(bits(x_old.cpu()), bits(c["x"]))
    assert not nf.any()
    assert ((x.cpu() - c["x0"]).abs() <= E + 1e-7).all() and x.min() >= -1 and x.max() <= 1
    assert (want != c["x"]).float().mean().item() > 0.5           # the step moved the images
    x2, _, _ = update(c, a, cuda)
    assert torch.equal(bits(x2), bits(x))
    one = {k: v[1:2].contiguous() for k, v in c.items()}
    from gfa_amd import ops
    t = {k: v.to(cuda) for k, v in one.items()}
    ops.apgd_update(t["x"], t["x_old"], t["x0"], t["g"], t["eta"], a, E)
    assert torch.equal(bits(t["x"][0]), bits(x[1]))
    for name in ("x", "x_old", "x0", "g"):
        xo, oo, _ = update(c, a, cuda, off=(name,))
        assert torch.equal(bits(xo), bits(x)) and torch.equal(bits(oo), bits(x_old)), name


def test_apgd_update_flags_nonfinite(cuda):
    c = case(33)
    for val, pos, who in ((float("inf"), (1, 2, 10, 5), [0, 1, 0]), (NAN, (0, 0, 0, 0), [1, 0, 0]),
                          (-float("inf"), (2, 2, 32, 32), [0, 0, 1])):   # the last: a partial group
        g = c["g"].clone()
        g[pos] = val
        x, _, nf = update(c, 0.75, cuda, g=g)
        assert nf.tolist() == who
        want, _ = apgd_ref.update(c["x"], c["x_old"], c["x0"], g, c["eta"], 0.75, E)
        assert torch.isfinite(x).all() and torch.equal(bits(x.cpu()), bits(want))


def test_apgd_wrappers_reject_malformed_calls(cuda):
    from gfa_amd import ops
    x = torch.zeros(2, 3, 8, 8, device=cuda)
    xo, x0, g = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    eta = torch.ones(2, device=cuda)
    act = torch.zeros(2, dtype=I32, device=cuda)
    flat = torch.zeros(2 * 3 * 8 * 8 + 4, device=cuda)
    a, b = flat[:-4].view(2, 3, 8, 8), flat[4:].view(2, 3, 8, 8)
    with pytest.raises(ValueError):
        ops.apgd_update(x, x, x0, g, eta, 0.75, 0.1)
    with pytest.raises(ValueError):
        ops.apgd_update(x, xo, x0.cpu(), g, eta, 0.75, 0.1)
    with pytest.raises(ValueError):
        ops.apgd_update(x, xo, x0, g, eta.cpu(), 0.75, 0.1)
    with pytest.raises(Exception, match="distinct"):            # the library's own check
        ops.apgd_update(a, b, x0, g, eta, 0.75, 0.1)
    with pytest.raises(Exception, match="distinct"):
        ops.apgd_update(x, a, x0, b, eta, 0.75, 0.1)
    with pytest.raises(Exception, match="distinct"):
        ops.apgd_apply(a, g, b, xo, act)
    with pytest.raises(Exception, match="distinct"):
        ops.apgd_apply(x, a, xo, b, act)
    with pytest.raises(ValueError):
        ops.apgd_apply(x, g, xo, x0, act.cpu())
    loss = torch.zeros(2, device=cuda)
    big = torch.zeros(16, device=cuda)
    with pytest.raises(Exception, match="distinct"):            # loss inside the state rows
        ops.apgd_decide(big[2:4], big[:8].view(4, 2), torch.zeros(3, 2, dtype=I32, device=cuda),
                        act, torch.zeros(3, 2, device=cuda), torch.zeros(3, 2, device=cuda), 1)
    with pytest.raises(ValueError):
        ops.apgd_decide(loss.cpu(), torch.zeros(4, 2, device=cuda),
                        torch.zeros(3, 2, dtype=I32, device=cuda), act,
                        torch.zeros(3, 2, device=cuda), torch.zeros(3, 2, device=cuda), 1)


# ---- the control and copy kernels against the control reference ---------------------------------
CANARY = 12345.0


def guarded(shape, fill, dev):
    """A buffer of ``shape`` with 4 canary floats before and after it."""
    n = int(np.prod(shape))
    flat = torch.full((n + 8,), CANARY, device=dev)
    flat[4:-4] = fill
    return flat[4:-4].view(shape), flat


def canaries_ok(flat):
    return bool((flat[:4] == CANARY).all() and (flat[-4:] == CANARY).all())


@pytest.mark.parametrize("S", [33, 32])
def test_apgd_bookkeeping_follows_the_control_reference(cuda, S):
    """N = 5 images of 3·33² (the scalar form, 4 slots per image; 3·32² for the copies' vector
    form), one per scripted sequence of
    the host test, 6 steps with checkpoints (2, 1), (2, 0), (2, 1) at steps 1, 3, 5. After every
    step: the state rows, the history rows and the action words equal the pure-Python control
    exactly; x_best, g_best, x and g are bit for bit the image the rule names (fresh x and g
    every step, so every copy is visible); rows of the history not yet reached stay NaN and the
    canaries around the image buffers stay intact."""
    from gfa_amd import ops
    L = apgd_ref.scripted_losses()
    N, shape = 5, (5, 3, S, S)
    assert L.shape == (7, N)
    fs = torch.full((4, N), NAN, device=cuda)
    st = torch.full((3, N), -7, dtype=I32, device=cuda)
    act = torch.full((N,), -7, dtype=I32, device=cuda)
    hl, he = torch.full((7, N), NAN, device=cuda), torch.full((7, N), NAN, device=cuda)
    x, fx = guarded(shape, 0.0, cuda)
    g, fg = guarded(shape, 0.0, cuda)
    xb, fxb = guarded(shape, NAN, cuda)
    gb, fgb = guarded(shape, NAN, cuda)
    ctl = [apgd_ref.Control(L[0, n], 1.0) for n in range(N)]
    want_xb = want_gb = None
    for step in range(7):
        nx, ng = seeded(40 + step, shape), 100.0 * seeded(60 + step, shape)
        x.copy_(nx)
        g.copy_(ng)
        loss = torch.from_numpy(L[step].copy()).to(cuda)
        if step == 0:
            ops.apgd_decide(loss, fs, st, act, hl, he, 0, eta0=1.0)
            acts = [apgd_ref.SAVE] * N
        else:
            ck = apgd_ref.SCRIPT_CHECKPOINTS.get(step - 1)
            ops.apgd_decide(loss, fs, st, act, hl, he, step, checkpoint=ck is not None,
                            thr=ck[1] if ck else 0)
            acts = [ctl[n].step(step - 1, L[step, n], ck) for n in range(N)]
        assert act.tolist() == acts, step
        ops.apgd_apply(x, g, xb, gb, act)
        want_x, want_g = nx.clone(), ng.clone()
        if step == 0:
            want_xb, want_gb = nx.clone(), ng.clone()
        for n, a in enumerate(acts):
            if a & apgd_ref.SAVE:                # with RESTORE too: the restore is the identity
                want_xb[n], want_gb[n] = nx[n], ng[n]
            elif a & apgd_ref.RESTORE:
                want_x[n], want_g[n] = want_xb[n], want_gb[n]
        for got, want, name in ((x, want_x, "x"), (g, want_g, "g"), (xb, want_xb, "x_best"),
                                (gb, want_gb, "g_best")):
            assert torch.equal(bits(got.cpu()), bits(want)), (step, name)
        fsc, stc = fs.cpu().numpy(), st.cpu().numpy()
        for n, c in enumerate(ctl):
            s = c.state()
            for row, key in enumerate(("eta", "L_best", "L_prev", "L_check")):
                assert np.array_equal(fsc[row, n], np.float32(s[key]), equal_nan=True), \
                    (step, n, key, fsc[row, n], s[key])
            for row, key in enumerate(("n_dec", "reduced", "best_step")):
                assert stc[row, n] == s[key], (step, n, key, stc[row, n], s[key])
        hlc, hec = hl.cpu().numpy(), he.cpu().numpy()
        assert np.array_equal(hlc[:step + 1], L[:step + 1], equal_nan=True)
        assert np.array_equal(hec[:step + 1],
                              np.array([c.step_size for c in ctl], dtype=np.float32).T)
        assert np.isnan(hlc[step + 1:]).all() and np.isnan(hec[step + 1:]).all()
        assert all(canaries_ok(f) for f in (fx, fg, fxb, fgb))
    assert [c.halvings for c in ctl] == [0, 2, 1, 1, 3]
    # an all-zero action touches nothing
    act.zero_()
    xb.fill_(NAN)
    keep = x.clone()
    ops.apgd_apply(x, g, xb, gb, act)
    assert torch.equal(bits(x), bits(keep)) and torch.isnan(xb).all()


# ---- end to end at 32² --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net32(cuda):
    from gfa_amd import networks
    return networks.build_net(SIZE, seed=0, dtype=torch.float32, device=cuda)


_oracle = {}


def oracle():
    """The fp64 networks of build_net(32, seed=0) (linear encoder) with the targets of x0 and t
    (test_gpu_si.oracle's, with the objective): x ↦ (∇L(x), L(x) per image). Built once."""
    if "fn" not in _oracle:
        from gfa_amd.weights import make_encoder_weights, make_generator_weights, make_vgg_weights
        from oracle import attack_ref, vgg_ref
        params = (make_generator_weights(SIZE, seed=0),
                  vgg_ref.load_positional(make_vgg_weights(1234)),
                  make_encoder_weights(SIZE, seed=1))
        p64 = to64(params)
        x0, t = images()
        refs = attack_ref.Refs(*p64, x0.double(), t.double(), SIZE)

        def fn(x):
            L, g = attack_ref.loss_grad(*p64, x.double(), refs, SIZE)
            return g, L
        _oracle["fn"] = fn
        # the same oracle in fp32: its own rounding error on these inputs
        refs32 = attack_ref.Refs(*params, x0, t, SIZE)
        with torch.no_grad():
            _oracle["L32"] = attack_ref.objective(*params, x0, refs32, SIZE, per_image=True)
    return _oracle["fn"]


def oracle_at_x0():
    if "x0" not in _oracle:
        _oracle["x0"] = oracle()(images()[0])
    return _oracle["x0"]


def oracle_run():
    """apgd_ref's whole loop on the oracle gradient and objective at (EPS, STEPS), once."""
    if "run" not in _oracle:
        fn = oracle()
        first = [oracle_at_x0()]
        _oracle["run"] = apgd_ref.run(images()[0], E, STEPS,
                                      lambda x: first.pop() if first else fn(x))
    return _oracle["run"]


def test_engine_apgd_step_vs_oracle(cuda, net32):
    """start_apgd then step_apgd(x, 0) from x0, fp32: x1 equals apgd_ref's update (a = 1,
    eta = 2·e) with the fp64 oracle gradient g0 wherever its sign is stable (at most 2 % excluded,
    asserted on the oracle alone). The recorded L(x0) agrees with the oracle's fp64 objective to
    4× the oracle's own fp32-vs-fp64 difference on these inputs (the device convs are an
    exact-split fp32; the figures are printed). That difference is ONE figure for the inputs, the
    larger of the two images': a single image's fp32 value can land within an ulp of the fp64 one
    by chance, which says nothing about the arithmetic. Measured: the oracle's own differences
    1.30e-6 and 2.31e-7 (bound 4 × 1.30e-6 = 5.18e-6), the device's 1.30e-6 and 1.66e-6 on
    objectives of 3.63 and 3.28 (5 – 7 fp32 ulps). Held per image instead, image 1 would miss
    (1.66e-6 against 4 × 2.31e-7 = 9.2e-7), the oracle's fp32 sum there being 1 ulp off."""
    from gfa_amd.pgd import AttackEngine
    x0, t = images()
    g0, L0 = oracle_at_x0()
    stable = stable_mask(g0)
    share = 1.0 - stable.double().mean().item()
    own = (_oracle["L32"].double() - L0).abs()
    print(f"APGD engine step: {share:.4%} of the pixels excluded; the oracle's own fp32-vs-fp64 "
          f"objective difference {own.tolist()} (relative {(own / L0.abs()).tolist()})")
    assert share <= 0.02
    eta = torch.full((2,), f32(2 * E))
    want, _ = apgd_ref.update(x0, x0, x0, g0.float(), eta, 1.0, E)
    assert (want != x0)[stable].float().mean().item() > 0.9
    eng = AttackEngine(net32.encoder.impl, net32.decoder.impl, net32.vgg.impl)
    x = eng.start_apgd(x0.to(cuda), t.to(cuda), STEPS, EPS)
    b = eng._apgd_buffers(x.shape)
    assert torch.equal(x.cpu(), x0) and torch.equal(b["x_best"].cpu(), x0)
    assert torch.equal(b["x_old"].cpu(), x0) and torch.equal(bits(b["g_best"]), bits(b["g"]))
    assert b["state_f"][0].tolist() == [f32(2 * E)] * 2
    assert b["state_i"].tolist() == [[0, 0], [1, 1], [0, 0]]
    L_dev = b["loss"][0].cpu().double()
    err = (L_dev - L0).abs()
    print(f"APGD engine step: device L(x0) {L_dev.tolist()}, oracle {L0.tolist()}, difference "
          f"{err.tolist()} (bound 4 x {own.max().item()})")
    assert torch.equal(b["state_f"][1].cpu().double(), L_dev)
    eng.step_apgd(x, 0)
    assert not eng.overflowed()
    got = x.cpu()
    frac = (got == want).float().mean().item()
    print(f"APGD engine step: equal to the oracle step on {frac:.6f} of all pixels")
    assert torch.equal(got[stable], want[stable])
    assert torch.equal(b["x_old"].cpu(), x0)
    assert (err <= 4 * own.max()).all()
    del eng


def check_replay(info, steps, e):
    """The decisions are a function of the recorded fp32 objectives alone: the control reference
    on info["apgd"]["loss"] reproduces step_size, best_step and halvings exactly."""
    a = info["apgd"]
    loss, eta = a["loss"], a["step_size"]
    N = loss.shape[1]
    assert tuple(loss.shape) == tuple(eta.shape) == (steps + 1, N)
    assert loss.dtype == eta.dtype == torch.float32 and not loss.is_cuda
    assert torch.isfinite(loss).all()
    ctl = apgd_ref.replay(loss.numpy(), f32(2 * e))
    for n, c in enumerate(ctl):
        assert eta[:, n].tolist() == [float(v) for v in c.step_size], n
        assert int(a["best_step"][n]) == c.best_step and int(a["halvings"][n]) == c.halvings
        assert loss[int(a["best_step"][n]), n] == loss[:, n].min()
    assert (loss.min(0).values <= loss[0]).all()
    return ctl


def test_attack_apgd_replay_end_to_end(cuda, net32):
    from gfa_amd import attack
    from gfa_amd.pgd import AttackEngine
    x0, t = images()
    keep = x0.clone()
    kw = dict(target=t, apgd=True)
    adv, info = attack(net32, x0, EPS, STEPS, return_info=True, **kw)
    assert torch.equal(x0, keep) and info["rescales"] == 0 and info["norm"] == "linf"
    check_replay(info, STEPS, E)
    check_linf(adv, x0, E)
    a = info["apgd"]
    print(f"APGD {STEPS} steps: objective per step {a['loss'].T.tolist()}, step sizes "
          f"{a['step_size'].T.tolist()}, best_step {a['best_step'].tolist()}, halvings "
          f"{a['halvings'].tolist()}")
    # info["loss"] is what it is for every attack: the objective of the returned images
    assert torch.allclose(info["loss"], a["loss"].min(0).values, rtol=1e-5)
    adv2, info2 = attack(net32, x0, EPS, STEPS, return_info=True, **kw)
    assert torch.equal(adv2, adv) and torch.equal(info2["apgd"]["loss"], a["loss"])
    alone = attack(net32, x0[1:2], EPS, STEPS, target=t[1:2], apgd=True)
    assert torch.equal(alone[0], adv[1])
    # by hand: the iterate after best_step[n] steps is adv[n]
    eng = AttackEngine(net32.encoder.impl, net32.decoder.impl, net32.vgg.impl)
    x = eng.start_apgd(x0.to(cuda), t.to(cuda), STEPS, EPS)
    snaps = [x.clone()]
    for i in range(STEPS):
        eng.step_apgd(x, i)
        snaps.append(x.clone())
    assert not eng.overflowed()
    for n in range(2):
        assert torch.equal(snaps[int(a["best_step"][n])][n].cpu(), adv[n]), n
    assert torch.equal(eng.apgd_info()["loss"], a["loss"])
    del eng
    # not the fixed-step attack
    plain, pinfo = attack(net32, x0, EPS, STEPS, target=t, alpha=ALPHA, momentum=None,
                          return_info=True)
    assert not torch.equal(plain, adv)
    print(f"APGD vs PGD(alpha={ALPHA:.5f}) at {STEPS} steps, final objective per image: "
          f"{info['loss'].tolist()} vs {pinfo['loss'].tolist()} (start {a['loss'][0].tolist()})")
    # a random start: inside the ball, reproducible, and another start
    r1 = attack(net32, x0, EPS, 4, target=t, apgd=True, random_start=True, seed=3)
    check_linf(r1, x0, E)
    assert torch.equal(r1, attack(net32, x0, EPS, 4, target=t, apgd=True, random_start=True,
                                  seed=3))
    assert not torch.equal(r1, attack(net32, x0, EPS, 4, target=t, apgd=True))
    # steps = 0 returns the start
    z, zi = attack(net32, x0, EPS, 0, return_info=True, **kw)
    assert torch.equal(z, x0) and tuple(zi["apgd"]["loss"].shape) == (1, 2)
    assert zi["apgd"]["best_step"].tolist() == [0, 0]


def test_attack_apgd_halvings_are_exercised(cuda, net32):
    """On the oracle's own trajectory (apgd_ref's loop on the fp64 gradient and objective) at
    (EPS, STEPS) every image halves its step at least once and at least one restore changes x —
    asserted before the device is looked at (2 halvings per image and 4 such restores expected:
    with eta0 = 2·e on a ball of radius e the second step overshoots). Then the device halves
    too."""
    from gfa_amd import attack
    x0, t = images()
    run = oracle_run()
    halv = [c.halvings for c in run["controls"]]
    print(f"APGD oracle trajectory: halvings {halv}, restores that change x {run['restores']}, "
          f"best_step {[c.best_step for c in run['controls']]}, objective "
          f"{[[round(float(v), 4) for v in c.loss] for c in run['controls']]}")
    assert min(halv) >= 1 and run["restores"] >= 1
    check_linf(run["x_best"], x0, E)
    _, info = attack(net32, x0, EPS, STEPS, target=t, apgd=True, return_info=True)
    print(f"APGD device: halvings {info['apgd']['halvings'].tolist()}")
    assert int(info["apgd"]["halvings"].sum()) >= 1


def test_attack_apgd_fp16(cuda):
    """fp16 networks: the same invariants as the replay test, with the rescales reported; a loss
    scale that overflows forces a re-run, after which the history has exactly steps + 1 rows that
    replay from the start (the state was reset)."""
    from gfa_amd import attack, networks
    net = networks.build_net(SIZE, seed=0, dtype=torch.float16, device=cuda)
    x0, t = images()
    adv, info = attack(net, x0, EPS, STEPS, target=t, apgd=True, return_info=True)
    print(f"fp16 APGD: rescales {info['rescales']}, loss scale {info['loss_scale']:g}, halvings "
          f"{info['apgd']['halvings'].tolist()}, best_step {info['apgd']['best_step'].tolist()}")
    assert info["dtype"] == "torch.float16" and info["rescales"] >= 0
    check_replay(info, STEPS, E)
    check_linf(adv, x0, E)
    assert torch.equal(adv, attack(net, x0, EPS, STEPS, target=t, apgd=True))
    alone = attack(net, x0[1:2], EPS, STEPS, target=t[1:2], apgd=True)
    assert torch.equal(alone[0], adv[1])
    adv_r, info_r = attack(net, x0, EPS, STEPS, target=t, apgd=True, return_info=True,
                           loss_scale=FORCED_LOSS_SCALE)
    print(f"fp16 APGD from loss scale {FORCED_LOSS_SCALE:g}: rescales {info_r['rescales']}, final "
          f"loss scale {info_r['loss_scale']:g}")
    assert info_r["rescales"] >= 1
    assert tuple(info_r["apgd"]["loss"].shape) == (STEPS + 1, 2)
    check_replay(info_r, STEPS, E)
    check_linf(adv_r, x0, E)
    del net
    free()


# fp16 tops out at 65504; the latent terms' gradient coefficient is λ·10·2/(8·512) per element,
# so λ = 2^24 puts it at 81920 before any difference multiplies it. Four divisions by 16 (the
# engine's limit) bring 2^24 back to the default 2^8. Measured at 32²: 2^16 does not overflow,
# 2^20 re-runs once, 2^24 twice (ending at 2^16).
FORCED_LOSS_SCALE = 2.0 ** 24


def test_existing_paths_are_untouched(cuda, net32):
    """apgd=False is the call without the keyword, bit for bit, for momentum None and 1.0."""
    from gfa_amd import attack
    x0, t = images()
    for mu in (None, 1.0):
        kw = dict(target=t, alpha=ALPHA, momentum=mu)
        plain = attack(net32, x0, EPS, 3, **kw)
        adv, info = attack(net32, x0, EPS, 3, apgd=False, return_info=True, **kw)
        assert torch.equal(adv, plain) and "apgd" not in info
