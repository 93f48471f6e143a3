"""SignHunter (Al-Dujaili & O'Reilly 2020; deterministic score-based black-box, L∞): the flip
kernel against its fp32 / int8 reference bit for bit (tests/sh_ref.py), the decision kernel against
the pure-Python control on scripted objectives, the device kernels driving a linear objective to
its known optimum, and the attack end to end at 32² — its decisions replayed from the recorded
objectives, the returned images rebuilt from them, the fp64 oracle at the result, batch
independence, fp16, and the untouched default path.

All image-space quantities are in [-1,1] units (e = 2·eps)."""
import numpy as np
import pytest
import torch

import sh_ref
from gpu_helpers import free, seeded, to64
from test_gpu_ti import EPS, SIZE, check_linf, images

pytestmark = pytest.mark.gpu

F32, I32, I8 = torch.float32, torch.int32, torch.int8
# per-image amplitudes of x0: cross-image mixing cannot hide; the last is absorbed by x0 ± e
IMG_SCALES = (1.0, 0.6, 1e-4)
# plane = 3·S²: 192 (one partial block), 3267 (no multiple of 4: the scalar form, a partial last
# group), 50700 (50 blocks per image), 12288 (12 blocks)
SIZES = (8, 33, 130, 64)
STEPS = 31     # levels 0 … 4 at plane = 3072
NAN = float("nan")


def f32(v):
    return float(np.float32(v))


E = f32(2 * EPS)


def bits(t):
    return t.contiguous().view(torch.int32)


_inputs = {}


def case(S):
    """Per size, computed once and shared (CPU): x0 with per-image amplitudes that reaches ±1
    (planted, so the clamp acts on both sides), a seeded ±1 sign plane and an x of seeded
    bits that no flip produces (what an untouched element must keep)."""
    if S not in _inputs:
        shape = (3, 3, S, S)
        x0 = seeded(700 + S, shape) * torch.tensor(IMG_SCALES).reshape(3, 1, 1, 1)
        f0 = x0.reshape(3, -1)
        f0[:, 0::7] = 1.0
        f0[:, 3::7] = -1.0
        f0[0, 5::7] = f32(1.0 - E / 2)               # x0 + e clamps, x0 − e does not
        s = ((seeded(800 + S, shape) > 0).to(I8) * 2 - 1).contiguous()
        x = 3.0 + seeded(900 + S, shape)
        _inputs[S] = dict(x0=x0.contiguous(), s=s, x=x.contiguous())
    return _inputs[S]


def flip_cases(plane):
    """(name, prev, new, accept, start) per case of the issue's list."""
    half = -(-plane // 2)
    l3, l4 = -(-plane // 8), -(-plane // 16)
    last3 = ((-(-plane // l3) - 1) * l3, plane)       # the last chunk of level 3
    odd = (plane // 2) | 1
    c = min(1024, plane - 8)
    return [
        ("start", None, (0, plane), None, True),
        ("level 0 rejected by image 1, level 1 begins", (0, plane), (0, half), (1, 0, 1), False),
        ("far apart: last chunk of level 3, first of level 4", last3, (0, l4), (0, 1, 0), False),
        ("adjacent single elements at odd offsets", (odd, odd + 1), (odd + 1, odd + 2), (0, 0, 1),
         False),
        ("ragged ends across element 1024 (or the plane's end)", None, (c - 3, c + 7), (0, 0, 0),
         False),
        ("ragged overlapping ranges", (c - 5, c + 2), (c - 1, c + 6), (0, 1, 0), False),
        ("the final revert: empty new range", last3, None, (0, 1, 0), False),
    ]


def offset_bytes(t, off):
    """The same data in a buffer ``off`` bytes past a 16-byte boundary."""
    raw = torch.zeros(t.numel() * t.element_size() + 16, dtype=torch.uint8, device=t.device)
    o = raw[off:off + t.numel() * t.element_size()].view(t.dtype).view(t.shape)
    o.copy_(t)
    assert o.data_ptr() % 16 == off and o.is_contiguous()
    return o


def device_flip(c, prev, new, accept, start, dev, rows=slice(None), off=False):
    from gfa_amd import ops
    x0, s, x = (c[k][rows].to(dev).contiguous() for k in ("x0", "s", "x"))
    if start:
        s.fill_(-1)
    if off:
        x0, x, s = offset_bytes(x0, 4), offset_bytes(x, 4), offset_bytes(s, 1)
    acc = None if accept is None else torch.tensor(accept, dtype=I32, device=dev)[rows].contiguous()
    ops.sh_flip(x, x0, s, acc, prev, new, E)
    return x, s


@pytest.mark.parametrize("S", SIZES)
def test_sh_flip_is_the_reference_bit_for_bit(cuda, S):
    """s and x equal the reference bit for bit in every case of flip_cases, and every element
    outside the two ranges keeps its old bits; reruns are bit-identical; one image alone gives its
    row; a 4-byte-offset copy of x / x0 with a 1-byte-offset copy of s (the scalar form) gives
    the same bits."""
    c = case(S)
    plane = 3 * S * S
    assert (c["x0"] == 1).any() and (c["x0"] == -1).any()
    j = torch.arange(plane)
    for name, prev, new, accept, start in flip_cases(plane):
        x_w, s_w = c["x"].clone(), (torch.full_like(c["s"], -1) if start else c["s"].clone())
        s_old = s_w.clone()
        sh_ref.flip(x_w, c["x0"], s_w, accept, prev, new, E)
        x, s = device_flip(c, prev, new, accept, start, cuda)
        assert torch.equal(s.cpu(), s_w), (S, name)
        assert torch.equal(bits(x.cpu()), bits(x_w)), (S, name)
        union = torch.zeros(plane, dtype=torch.bool)
        for r in (prev, new):
            if r is not None:
                union |= (j >= r[0]) & (j < r[1])
        out = ~union
        assert torch.equal(bits(x.cpu()).reshape(3, -1)[:, out], bits(c["x"]).reshape(3, -1)[:, out])
        assert torch.equal(s.cpu().reshape(3, -1)[:, out], s_old.reshape(3, -1)[:, out])
        touched = x.cpu().reshape(3, -1)[:, union]
        lo = torch.clamp(c["x0"] - E, -1, 1).reshape(3, -1)[:, union]
        hi = torch.clamp(c["x0"] + E, -1, 1).reshape(3, -1)[:, union]
        assert ((touched == lo) | (touched == hi)).all(), (S, name)
        x2, s2 = device_flip(c, prev, new, accept, start, cuda)
        assert torch.equal(bits(x2), bits(x)) and torch.equal(s2, s)
        x1, s1 = device_flip(c, prev, new, accept, start, cuda, rows=slice(1, 2))
        assert torch.equal(bits(x1[0]), bits(x[1])) and torch.equal(s1[0], s[1]), (S, name)
        xo, so = device_flip(c, prev, new, accept, start, cuda, off=True)
        assert torch.equal(bits(xo), bits(x)) and torch.equal(so, s), (S, name)
    # the clamp acted on both sides at the start
    x, _ = device_flip(c, None, (0, plane), None, True, cuda)
    assert (x == 1).any() and ((x.cpu() - c["x0"]) < E * 0.75).any()


def test_sh_flip_rejects_malformed_calls(cuda):
    from gfa_amd import ops
    x = torch.zeros(2, 3, 8, 8, device=cuda)
    x0 = torch.zeros_like(x)
    s = torch.ones(2, 3, 8, 8, dtype=I8, device=cuda)
    acc = torch.ones(2, dtype=I32, device=cuda)
    flat = torch.zeros(2 * 192 + 4, device=cuda)
    a, b = flat[:-4].view(2, 3, 8, 8), flat[4:].view(2, 3, 8, 8)
    with pytest.raises(Exception, match="distinct"):            # the library's own check
        ops.sh_flip(a, b, s, acc, None, (0, 192), 0.1)
    with pytest.raises(ValueError):
        ops.sh_flip(x, x0, s, acc.cpu(), None, (0, 192), 0.1)
    with pytest.raises(ValueError):
        ops.sh_flip(x, x0.cpu(), s, acc, None, (0, 192), 0.1)
    with pytest.raises(ValueError):
        ops.sh_flip(x, x0, s, acc, None, (0, 193), 0.1)
    with pytest.raises(ValueError):
        ops.sh_flip(x, x0, s, acc, (3, 3), None, 0.1)
    assert not x.any() and (s == 1).all()


# ---- the decision kernel against the control reference -----------------------------------------
def test_sh_decide_follows_the_control_reference(cuda):
    """One image per scripted sequence of the host test, query 0 and six flips: after every query
    accept, best, n_accept and the history rows equal the pure-Python control; rows not yet
    reached stay NaN; nonfinite is set exactly for the NaN / Inf columns."""
    from gfa_amd import ops
    L = sh_ref.scripted_losses()
    N = L.shape[1]
    assert L.shape == (7, 6) and list(sh_ref.SCRIPTS)[3:] == ["nan", "inf", "nan0"]
    best = torch.full((N,), NAN, device=cuda)
    acc = torch.full((N,), -7, dtype=I32, device=cuda)
    n_acc = torch.full((N,), -7, dtype=I32, device=cuda)
    hist = torch.full((7, N), NAN, device=cuda)
    nf = torch.zeros(N, dtype=I32, device=cuda)
    ctl = None
    for k in range(7):
        loss = torch.from_numpy(L[k].copy()).to(cuda)
        ops.sh_decide(loss, best, acc, n_acc, hist, k, nonfinite=nf)
        if k == 0:
            ctl = [sh_ref.Control(L[0, n]) for n in range(N)]
        else:
            for n in range(N):
                ctl[n].step(L[k, n])
        assert acc.tolist() == [c.accept for c in ctl], k
        assert n_acc.tolist() == [c.n_accept for c in ctl], k
        assert np.array_equal(best.cpu().numpy(), np.array([c.best for c in ctl], dtype=np.float32),
                              equal_nan=True), k
        assert nf.tolist() == [c.nonfinite for c in ctl], k
        h = hist.cpu().numpy()
        assert np.array_equal(h[:k + 1], L[:k + 1], equal_nan=True) and np.isnan(h[k + 1:]).all()
    assert nf.tolist() == [0, 0, 0, 1, 1, 1]
    assert n_acc.tolist() == [6, 0, 2, 2, 2, 0] and acc.tolist() == [1, 0, 0, 0, 0, 0]
    # without the flag array the decisions are the same
    acc2, n2, b2 = torch.zeros_like(acc), torch.zeros_like(n_acc), torch.zeros_like(best)
    for k in range(7):
        ops.sh_decide(torch.from_numpy(L[k].copy()).to(cuda), b2, acc2, n2, hist, k)
    assert torch.equal(n2, n_acc) and torch.equal(bits(b2), bits(best))
    with pytest.raises(Exception, match="distinct"):            # the library's own check
        big = torch.zeros(16, device=cuda)
        ops.sh_decide(big[0:6], big[3:9], acc, n_acc, hist, 1)
    with pytest.raises(ValueError):
        ops.sh_decide(torch.zeros(N), best, acc, n_acc, hist, 1)


# ---- the device kernels on the linear objective ----------------------------------------------------
def test_device_kernels_reach_the_linear_optimum(cuda):
    """The host test's linear objective (x0 = 0, e = 0.25, plane = 192, scales 1e4, 1, 1e-4),
    driven by mia_sh_flip and mia_sh_decide: the objective is computed by torch in fp64 from the
    device x and cast to fp32, as in sh_ref.run. After the 415 flips of one cycle s_j = −σ_j for
    every j, and s, x and the whole history equal sh_ref.run bit for bit."""
    from gfa_amd import ops
    from gfa_amd.pgd import sh_schedule
    x0c, e, w, sigma = sh_ref.linear_case()
    obj = sh_ref.linear_objective(w)
    want = sh_ref.run(x0c, e, 415, obj)
    for n in range(3):
        assert torch.equal(want["s"][n].double(), -sigma)           # the reference gets there
    N, plane = x0c.shape
    x0 = x0c.to(cuda)
    x = torch.full_like(x0, NAN)
    s = torch.full((N, plane), -1, dtype=I8, device=cuda)
    best = torch.zeros(N, device=cuda)
    acc, n_acc = torch.zeros(N, dtype=I32, device=cuda), torch.zeros(N, dtype=I32, device=cuda)
    hist = torch.full((416, N), NAN, device=cuda)
    nf = torch.zeros(N, dtype=I32, device=cuda)
    ops.sh_flip(x, x0, s, None, None, (0, plane), e)
    ops.sh_decide(torch.from_numpy(obj(x)).to(cuda), best, acc, n_acc, hist, 0, nonfinite=nf)
    prev = None
    rows = sh_schedule(415, plane)
    for k, row in enumerate(rows, start=1):
        ops.sh_flip(x, x0, s, acc, prev, row, e)
        ops.sh_decide(torch.from_numpy(obj(x)).to(cuda), best, acc, n_acc, hist, k, nonfinite=nf)
        prev = row
    ops.sh_flip(x, x0, s, acc, prev, None, e)
    assert not nf.any()
    assert torch.equal(s.cpu(), want["s"]) and torch.equal(bits(x.cpu()), bits(want["x"]))
    assert np.array_equal(hist.cpu().numpy(), want["loss"])
    for n in range(3):
        assert torch.equal(s[n].cpu().double(), -sigma), n
        assert torch.equal(x[n].cpu().double(), -0.25 * sigma)
    assert n_acc.tolist() == [c.n_accept for c in want["controls"]]
    assert best.tolist() == [float(c.best) for c in want["controls"]]


# ---- end to end at 32² --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net32(cuda):
    from gfa_amd import networks
    return networks.build_net(SIZE, seed=0, dtype=torch.float32, device=cuda)


_oracle = {}


def oracle_objective():
    """The fp64 networks of build_net(32, seed=0) with the targets of x0 and t: x ↦ the per-image
    objective (fp64 [N]). Built once."""
    if "obj" not in _oracle:
        from gfa_amd.weights import make_encoder_weights, make_generator_weights, make_vgg_weights
        from oracle import attack_ref, vgg_ref
        p64 = to64((make_generator_weights(SIZE, seed=0),
                    vgg_ref.load_positional(make_vgg_weights(1234)),
                    make_encoder_weights(SIZE, seed=1)))
        x0, t = images()
        refs = attack_ref.Refs(*p64, x0.double(), t.double(), SIZE)
        _oracle["obj"] = lambda x: attack_ref.objective(*p64, x.double(), refs, SIZE,
                                                        per_image=True).detach()
    return _oracle["obj"]


def check_vertices(adv, x0, e):
    """Every element is clamp(x0 + e) or clamp(x0 − e)."""
    ev = torch.tensor(e, dtype=F32)
    up, dn = torch.clamp(x0 + ev, -1, 1), torch.clamp(x0 - ev, -1, 1)
    assert ((adv == up) | (adv == dn)).all()
    check_linf(adv, x0, e)


def check_replay(adv, info, x0, steps, e):
    """The decisions are a function of the recorded fp32 objectives alone: the control reference
    on info["sign_hunter"]["loss"] and sh_ref.flip rebuild s and x, and the returned images are
    that x bit for bit; best is the column minimum under the rule, accepted its count."""
    sh = info["sign_hunter"]
    loss = sh["loss"]
    N = x0.shape[0]
    assert tuple(loss.shape) == (steps + 1, N) and loss.dtype == F32 and not loss.is_cuda
    assert torch.isfinite(loss).all()
    assert info["queries"] == steps + 1
    x, s, ctl = sh_ref.rebuild(x0, e, loss.numpy(), sh_ref.schedule(steps, x0[0].numel()))
    assert torch.equal(bits(adv), bits(x))
    assert sh["best"].tolist() == [float(c.best) for c in ctl]
    assert sh["accepted"].tolist() == [c.n_accept for c in ctl]
    assert torch.equal(sh["best"], loss.min(0).values)
    # the count of new records of the running minimum
    run_min = torch.cummin(loss, 0).values
    assert sh["accepted"].tolist() == (run_min[1:] < run_min[:-1]).sum(0).tolist()
    assert (sh["best"] <= loss[0]).all()
    check_vertices(adv, x0, e)
    return ctl


def test_attack_sign_hunter_replay_end_to_end(cuda, net32):
    """31 flips at 32² (levels 0 … 4): the replay of check_replay; the fp64 oracle objective at the
    returned images agrees with ``best`` within the project's fp32 objective bound against that
    oracle, relative 1e-4 (test_gpu_networks, as cited by test_gpu_spsa's
    test_engine_estimate_vs_oracle); at least one flip is kept; reruns are bit-identical; an image
    attacked alone gives its row of the batch; steps = 0 returns the images without a query."""
    from gfa_amd import attack
    x0, t = images()
    keep = x0.clone()
    kw = dict(target=t, sign_hunter=True)
    adv, info = attack(net32, x0, EPS, STEPS, return_info=True, **kw)
    assert torch.equal(x0, keep) and info["rescales"] == 0 and info["norm"] == "linf"
    sh = info["sign_hunter"]
    print(f"SignHunter {STEPS} flips: objective per query {sh['loss'].T.tolist()}, best "
          f"{sh['best'].tolist()}, accepted {sh['accepted'].tolist()}")
    check_replay(adv, info, x0, STEPS, E)
    assert int(sh["accepted"].sum()) >= 1
    # info["loss"] is what it is for every attack: the objective of the returned images
    assert torch.equal(info["loss"], sh["best"])
    want = oracle_objective()(adv)
    rel = ((sh["best"].double() - want).abs() / want.abs())
    print(f"SignHunter best vs the fp64 oracle at the returned images: {sh['best'].tolist()} vs "
          f"{want.tolist()}, relative {rel.tolist()} (bound 1e-4)")
    assert (rel <= 1e-4).all()
    adv2, info2 = attack(net32, x0, EPS, STEPS, return_info=True, **kw)
    assert torch.equal(adv2, adv) and torch.equal(info2["sign_hunter"]["loss"], sh["loss"])
    alone, ainfo = attack(net32, x0[1:2], EPS, STEPS, target=t[1:2], sign_hunter=True,
                          return_info=True)
    assert torch.equal(bits(alone[0]), bits(adv[1]))
    assert torch.equal(ainfo["sign_hunter"]["loss"][:, 0], sh["loss"][:, 1])
    # alpha plays no part
    assert torch.equal(attack(net32, x0, EPS, STEPS, alpha=0.5, **kw), adv)
    # a shorter attack is a prefix: the same queries, then the revert
    short, sinfo = attack(net32, x0, EPS, 7, return_info=True, **kw)
    assert torch.equal(sinfo["sign_hunter"]["loss"], sh["loss"][:8])
    check_replay(short, sinfo, x0, 7, E)
    z, zi = attack(net32, x0, EPS, 0, return_info=True, **kw)
    assert torch.equal(z, x0) and zi["queries"] == 0
    assert tuple(zi["sign_hunter"]["loss"].shape) == (0, 2)
    assert zi["sign_hunter"]["accepted"].tolist() == [0, 0]


def test_engine_sign_hunter_steps(cuda, net32):
    """start / step / finish by hand: query 0 is the all-plus vertex, the iterate after every
    query is a vertex, and the loop equals run_sign_hunter."""
    from gfa_amd.pgd import AttackEngine
    x0, t = images()
    eng = AttackEngine(net32.encoder.impl, net32.decoder.impl, net32.vgg.impl)
    x = eng.start_sign_hunter(x0.to(cuda), t.to(cuda), EPS, 3)
    assert torch.equal(x.cpu(), torch.clamp(x0 + torch.tensor(E), -1, 1))
    b = eng._sh_buffers(x.shape)
    assert (b["s"] == 1).all() and b["accept"].tolist() == [1, 1] and b["n_accept"].tolist() == [0, 0]
    assert torch.equal(b["best"], b["loss"][0])
    for k in (1, 2, 3):
        eng.step_sign_hunter(x, k)
        check_vertices(x.cpu(), x0, E)
    for bad in (0, 4):
        with pytest.raises(ValueError):
            eng.step_sign_hunter(x, bad)
    got = eng.finish_sign_hunter(x).clone()
    assert not eng.overflowed()
    hist = eng.sign_hunter_info()["loss"]
    want = eng.run_sign_hunter(x0.to(cuda), t.to(cuda), 3, EPS)
    assert torch.equal(bits(got), bits(want)) and torch.equal(eng.sign_hunter_info()["loss"], hist)
    assert eng.sh_queries == 4
    del eng


def test_attack_sign_hunter_flags_a_nonfinite_objective(cuda, net32):
    """A NaN pixel of the target makes the objective NaN: the run raises as a non-finite gradient
    does."""
    from gfa_amd.pgd import AttackEngine
    x0, t = images()
    t = t.clone()
    t[1, 0, 0, 0] = NAN
    eng = AttackEngine(net32.encoder.impl, net32.decoder.impl, net32.vgg.impl)
    with pytest.raises(FloatingPointError, match="non-finite"):
        eng.run_sign_hunter(x0.to(cuda), t.to(cuda), 2, EPS)
    del eng


def test_attack_sign_hunter_fp16(cuda):
    """fp16 networks: it runs, returns vertices, replays from its own history and is reproducible
    and batch-independent."""
    from gfa_amd import attack, networks
    net = networks.build_net(SIZE, seed=0, dtype=torch.float16, device=cuda)
    x0, t = images()
    adv, info = attack(net, x0, EPS, STEPS, target=t, sign_hunter=True, return_info=True)
    sh = info["sign_hunter"]
    print(f"fp16 SignHunter: rescales {info['rescales']}, start {sh['loss'][0].tolist()}, best "
          f"{sh['best'].tolist()}, accepted {sh['accepted'].tolist()}")
    assert info["dtype"] == "torch.float16" and info["rescales"] == 0
    check_replay(adv, info, x0, STEPS, E)
    assert torch.equal(adv, attack(net, x0, EPS, STEPS, target=t, sign_hunter=True))
    alone = attack(net, x0[1:2], EPS, STEPS, target=t[1:2], sign_hunter=True)
    assert torch.equal(alone[0], adv[1])
    del net
    free()


def test_existing_paths_are_untouched(cuda, net32):
    """sign_hunter=False is the call without the keyword, bit for bit, for momentum None and 1.0."""
    from gfa_amd import attack
    from test_gpu_ti import ALPHA
    x0, t = images()
    for mu in (None, 1.0):
        kw = dict(target=t, alpha=ALPHA, momentum=mu)
        plain, pinfo = attack(net32, x0, EPS, 3, return_info=True, **kw)
        adv, info = attack(net32, x0, EPS, 3, sign_hunter=False, return_info=True, **kw)
        assert torch.equal(adv, plain) and info["sign_hunter"] is False
        assert pinfo["sign_hunter"] is False and info["queries"] == 0
        assert not torch.equal(adv, attack(net32, x0, EPS, 3, target=t, sign_hunter=True))
