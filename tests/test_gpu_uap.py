"""The universal perturbation on the GPU: mia_uap_accumulate and mia_uap_step bit for bit against
the torch reference (tests/uap_ref.py), the order and split invariance of the integer sum, the
engine's step composed from the device's own gradient, the batch invariances of attack(...,
universal=True), the attack end to end at 32², and the world-size independence of
attack_distributed over gloo. Every value check is exact (torch.equal): integer sums and
single-rounding elementwise operations leave no tolerance to choose."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import uap_ref
from gpu_helpers import seeded
from test_gpu_di import offset_copy

pytestmark = pytest.mark.gpu

F32 = torch.float32
EPS, ALPHA, SIZE = 8 / 255, 2 / 255, 32
E, A = float(np.float32(2 * EPS)), float(np.float32(2 * ALPHA))
# plane = 3·S²: 75 (no multiple of 4: the scalar form, a partial last group), 192 (the vector form,
# one block), 12288 (12 blocks of 256 threads × 4 elements)
SIZES = (5, 8, 64)
EXPONENTS = (20, -20, 0, 7, -13)      # image n's gradient is of the order 2^EXPONENTS[n]
TIES = (0, 1, 2, 3, -1, -2, -3, 12345, -54321)   # ĝ·2^24 = k + ½ exactly


def synthetic(N, S, seed=0, inf=True):
    """(g, l1): N gradients whose scales differ by 2^±20. l1[n] = plane·2^m makes the mean the
    exact power of two 2^m, so ĝ = −g·2^-m exactly: elements 0 … 8 of every image are .5 ties by
    construction, elements 9 … 11 are ±0, and the LAST image carries a +Inf (element 13) and a
    finite element outside the range |ĝ| < 2·plane (element 14)."""
    plane = 3 * S * S
    g = seeded(100 + seed + S, (N, 3, S, S)).clone()
    l1 = torch.empty(N)
    flat = g.reshape(N, plane)
    for n in range(N):
        m = EXPONENTS[n % len(EXPONENTS)]
        flat[n] *= 2.0 ** m
        l1[n] = plane * 2.0 ** m
        for i, k in enumerate(TIES):
            flat[n, i] = -(k + 0.5) * 2.0 ** (m - 24)
        flat[n, 9:12] = torch.tensor([0.0, -0.0, 0.0])
    if inf:
        flat[N - 1, 13] = float("inf")
        flat[N - 1, 14] = -3.0 * plane * 2.0 ** EXPONENTS[(N - 1) % len(EXPONENTS)]
    return g, l1


def run_accumulate(cuda, g, l1, acc=None, misalign=False):
    """(acc, flags) of the device kernel; ``acc`` (int64, host): added to (first = 0), None:
    first = 1 over a garbage-filled plane."""
    from gfa_amd import ops
    N, plane = g.shape[0], g.numel() // g.shape[0]
    gd = offset_copy(g.to(cuda)) if misalign else g.to(cuda)
    if acc is None:
        ad = torch.full((plane,), -0x0123456789ABCDEF, dtype=torch.int64, device=cuda)
    else:
        ad = acc.to(cuda).clone()
    nf = torch.zeros(N, dtype=torch.int32, device=cuda)
    ops.uap_accumulate(gd, l1.to(cuda), ad, acc is None, nonfinite=nf)
    torch.cuda.synchronize()
    return ad.cpu(), nf.cpu().bool()


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("N", [1, 3, 5])
def test_accumulate_matches_reference(cuda, S, N):
    g, l1 = synthetic(N, S)
    plane = 3 * S * S
    want, bad = uap_ref.accumulate(g, l1)
    q, _ = uap_ref.terms(g, l1)
    # the construction holds: exact ties, round-half-even, and the last image alone is flagged
    qf = q.reshape(N, plane)
    assert qf[0, :9].tolist() == [2 * ((k + 1) // 2) for k in TIES]
    assert bad.tolist() == [False] * (N - 1) + [True]
    assert qf[N - 1, 13] == 0 and qf[N - 1, 14] == 0 and not qf[:, 9:12].any()
    got, flags = run_accumulate(cuda, g, l1)
    assert got.dtype == torch.int64 and torch.equal(got, want)      # first = 1 ignores the garbage
    assert torch.equal(flags, bad)
    # the flagged image's other elements are summed, and the other images' terms are untouched
    clean, _ = synthetic(N, S, inf=False)
    want_clean, bad_clean = uap_ref.accumulate(clean, l1)
    keep = torch.ones(plane, dtype=torch.bool)
    keep[13:15] = False
    assert not bad_clean.any() and torch.equal(got[keep], want_clean[keep])
    # first = 0 adds to what is there
    pre = torch.randint(-(1 << 40), 1 << 40, (plane,), generator=torch.Generator().manual_seed(S))
    got2, flags2 = run_accumulate(cuda, g, l1, acc=pre)
    assert torch.equal(got2, pre + want) and torch.equal(flags2, bad)
    # 4 bytes off 16-byte alignment: the scalar form, the same bits
    got3, flags3 = run_accumulate(cuda, g, l1, misalign=True)
    assert torch.equal(got3, want) and torch.equal(flags3, bad)


@pytest.mark.parametrize("S", [5, 8])
def test_accumulate_order_and_split_invariance(cuda, S):
    """The same five images permuted, in two calls (2 + 3) and in five single-image calls: one
    acc, bit for bit — the sum is an integer sum."""
    g, l1 = synthetic(5, S, seed=3)
    want, _ = uap_ref.accumulate(g, l1)
    whole, _ = run_accumulate(cuda, g, l1)
    perm = torch.tensor([3, 0, 4, 2, 1])
    permuted, flags = run_accumulate(cuda, g[perm].contiguous(), l1[perm].contiguous())
    assert flags.tolist() == [False, False, True, False, False]     # the flag follows its image
    two, _ = run_accumulate(cuda, g[:2], l1[:2])
    two, _ = run_accumulate(cuda, g[2:], l1[2:], acc=two)
    singles = None
    for n in (4, 1, 0, 3, 2):
        singles, _ = run_accumulate(cuda, g[n:n + 1], l1[n:n + 1], acc=singles)
    for got in (whole, permuted, two, singles):
        assert torch.equal(got, want)


def step_inputs(N, S):
    plane = 3 * S * S
    gen = torch.Generator().manual_seed(40 + S)
    delta = (torch.rand((1, 3, S, S), generator=gen) * 2 - 1) * E
    acc = torch.randint(-(1 << 50), 1 << 50, (plane,), generator=gen)
    d, a = delta.reshape(-1), acc
    d[0:6] = torch.tensor([E, E, E, -E, -E, -E])            # δ at ±e under every sign of acc
    a[0:6] = torch.tensor([1, -1, 0, 1, -1, 0])
    a[6:9] = torch.tensor([0, (1 << 62) + 1, -(1 << 62) - 1])
    x0 = seeded(50 + S, (N, 3, S, S)).clone()
    x0.reshape(N, plane)[:, 0:4] = torch.tensor([1.0, -1.0, 1.0, -1.0])
    return delta, acc, x0


@pytest.mark.parametrize("S", SIZES)
def test_step_matches_reference(cuda, S):
    from gfa_amd import apply_universal, ops
    N = 3
    delta, acc, x0 = step_inputs(N, S)
    want_d, want_x = uap_ref.step(delta, acc, x0, A, E)
    assert want_d.abs().max() <= E and (want_d != delta).any() and want_x.abs().max() <= 1
    for misalign in (False, True):
        dd, ad, x0d = delta.to(cuda), acc.to(cuda), x0.to(cuda)
        if misalign:
            x0d = offset_copy(x0d)
        xd = torch.full_like(x0.to(cuda), float("nan"))
        ops.uap_step(dd, ad, xd, x0d, A, E)
        torch.cuda.synchronize()
        assert torch.equal(dd.cpu(), want_d) and torch.equal(xd.cpu(), want_x)
    # acc = None: δ untouched, applied only
    dd, x0d = delta.to(cuda), x0.to(cuda)
    xd = torch.full_like(x0d, float("nan"))
    ops.uap_step(dd, None, xd, x0d, A, E)
    _, want_apply = uap_ref.step(delta, None, x0, A, E)
    assert torch.equal(dd.cpu(), delta) and torch.equal(xd.cpu(), want_apply)
    # N = 0: δ only
    ops.uap_step(dd, acc.to(cuda), None, None, A, E)
    assert torch.equal(dd.cpu(), want_d) and torch.equal(x0d.cpu(), x0)
    # apply_universal is the same kernel: from host and from device tensors
    got = apply_universal(x0, delta.to(cuda))
    assert got.device == x0.device and got.dtype == F32 and torch.equal(got, want_apply)
    assert torch.equal(apply_universal(x0, delta), want_apply)      # both on the host
    got = apply_universal(x0.to(cuda).double(), delta)
    assert got.is_cuda and torch.equal(got.cpu(), want_apply)


# ---- the engine at 32² ----------------------------------------------------------------------------
_nets = {}


def net32(cuda, dtype):
    from gfa_amd import networks
    if dtype not in _nets:
        _nets[dtype] = networks.build_net(SIZE, seed=0, dtype=dtype, device=cuda)
    return _nets[dtype]


def batch(n):
    return (torch.cat([seeded(700 + i, (1, 3, SIZE, SIZE)) * (0.6 if i % 2 else 1.0)
                       for i in range(n)]),
            torch.cat([seeded(800 + i, (1, 3, SIZE, SIZE)) for i in range(n)]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_engine_step_equals_reference_on_device_gradient(cuda, dtype):
    """One step_universal from a given δ equals the reference composed from the device's own g
    and Σ|g| at the same x (the gradient chain is bit-reproducible, so it is called twice)."""
    from gfa_amd import pgd
    net = net32(cuda, dtype)
    x0, t = batch(3)
    eng = pgd.AttackEngine(net.encoder.impl, net.decoder.impl, net.vgg.impl)
    noise = pgd.make_start_noise((1, 3, SIZE, SIZE), 9, "linf")
    x = eng.start_universal(x0.to(cuda), t.to(cuda), EPS, True, noise.to(cuda))
    delta0 = eng._uap_buffers(x0.shape)["delta"].cpu()
    assert torch.equal(delta0, torch.clamp(noise * torch.tensor(E), -E, E))
    assert torch.equal(x.cpu(), torch.clamp(x0 + delta0, -1, 1))
    l1 = torch.zeros(3, device=cuda)
    g = eng._step_gradient(x, l1=l1).clone()
    assert torch.isfinite(g).all() and (l1 > 0).all()
    acc, bad = uap_ref.accumulate(g.cpu(), l1.cpu())
    want_d, want_x = uap_ref.step(delta0, acc, x0, A, E)
    eng.step_universal(x, A, E)
    torch.cuda.synchronize()
    b = eng._uap_buffers(x0.shape)
    assert not bad.any() and not eng.overflowed()
    assert torch.equal(b["acc"].cpu(), acc)
    assert torch.equal(b["delta"].cpu(), want_d) and torch.equal(x.cpu(), want_x)
    assert (want_d != delta0).any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_attack_universal_batch_invariances(cuda, dtype):
    from gfa_amd import attack, fgsm
    net = net32(cuda, dtype)
    x0, t = batch(3)
    kw = dict(alpha=ALPHA, universal=True, return_info=True)
    keep = x0.clone()
    adv, info = attack(net, x0, EPS, 3, target=t, random_start=True, seed=5, **kw)
    delta = info["universal"]["delta"]
    assert torch.equal(x0, keep) and tuple(delta.shape) == (1, 3, SIZE, SIZE)
    assert delta.device == x0.device and delta.dtype == F32
    # ‖δ‖∞ ≤ e and the output is clamp(x0 + δ)
    assert info["universal"]["linf"] == float(delta.abs().max()) <= E
    assert torch.equal(adv, torch.clamp(x0 + delta, -1, 1))
    print(f"universal {dtype}: linf {info['universal']['linf']:.6f} (e {E:.6f}), rescales "
          f"{info['rescales']}, loss {info['loss'].tolist()}")
    # a rerun is bit-identical, random start included
    adv2, info2 = attack(net, x0, EPS, 3, target=t, random_start=True, seed=5, **kw)
    assert torch.equal(adv2, adv) and torch.equal(info2["universal"]["delta"], delta)
    other = attack(net, x0, EPS, 3, target=t, random_start=True, seed=6, **kw)[1]
    assert not torch.equal(other["universal"]["delta"], delta)
    # a permuted batch gives the same δ
    perm = torch.tensor([2, 0, 1])
    advp, infop = attack(net, x0[perm], EPS, 3, target=t[perm], random_start=True, seed=5, **kw)
    assert torch.equal(infop["universal"]["delta"], delta) and torch.equal(advp, adv[perm])
    # [x, x] with one target gives the δ of [x]
    one = attack(net, x0[:1], EPS, 3, target=t[:1], **kw)[1]["universal"]["delta"]
    twice = attack(net, x0[:1].repeat(2, 1, 1, 1), EPS, 3, target=t[:1], **kw)[1]
    assert torch.equal(twice["universal"]["delta"], one)
    # the one-step form
    advf, infof = fgsm(net, x0, EPS, target=t, universal=True, return_info=True)
    df = infof["universal"]["delta"]
    assert set(df.abs().unique().tolist()) <= {0.0, E}
    assert torch.equal(advf, torch.clamp(x0 + df, -1, 1))


def test_attack_universal_end_to_end(cuda):
    """N = 4, eps 8/255, alpha 2/255, 10 steps: the summed objective falls; the same δ on two
    held-out images is reported."""
    from gfa_amd import apply_universal, attack, pgd
    net = net32(cuda, torch.float32)
    x0, t = batch(4)
    adv, info = attack(net, x0, EPS, 10, target=t, alpha=ALPHA, universal=True, return_info=True)
    delta = info["universal"]["delta"]
    eng = pgd.AttackEngine(net.encoder.impl, net.decoder.impl, net.vgg.impl)
    eng.prepare(x0.to(cuda), t.to(cuda))
    before, after = eng.loss(x0.to(cuda)).double(), eng.loss(adv.to(cuda)).double()
    print(f"universal 10 steps, N = 4: L(x0) {before.tolist()} sum {before.sum():.6f} -> "
          f"L(clamp(x0 + delta)) {after.tolist()} sum {after.sum():.6f}")
    assert after.sum() < before.sum()
    held = torch.cat([seeded(750 + i, (1, 3, SIZE, SIZE)) for i in range(2)])
    moved = apply_universal(held, delta)
    assert torch.equal(moved, torch.clamp(held + delta, -1, 1))
    eng.prepare(held.to(cuda), t[:2].to(cuda))
    hb, ha = eng.loss(held.to(cuda)).double(), eng.loss(moved.to(cuda)).double()
    print(f"universal delta on 2 held-out images: L {hb.tolist()} sum {hb.sum():.6f} -> "
          f"{ha.tolist()} sum {ha.sum():.6f} (reported, not asserted)")


# ---- world-size independence ----------------------------------------------------------------------
FORCED_LOSS_SCALE = 2.0 ** 24   # fp16 at 32²: the first run overflows and re-runs (test_gpu_apgd.py)


@pytest.mark.parametrize("world,n,dtype,loss_scale",
                         [(2, 5, "fp32", None), (3, 2, "fp32", None),
                          (3, 2, "fp16", FORCED_LOSS_SCALE)])
def test_attack_distributed_universal_world_size(cuda, tmp_path, world, n, dtype, loss_scale):
    """`world` ranks (processes started by torch.distributed.run, a child of this test under its
    own time limit) share the one GPU over gloo: uneven shards at world 2, an empty shard at
    world 3. Every rank's gathered batch and δ equal the single-process attack(...,
    universal=True) bit for bit; with the forced loss scale every rank re-runs from δ₀ together."""
    from gfa_amd import attack, networks
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={world}", "--rdzv-backend=c10d", "--rdzv-endpoint=127.0.0.1:0",
           "--local-addr=127.0.0.1", os.path.join(root, "tests", "uap_rank_worker.py"),
           str(tmp_path), str(n), dtype, repr(loss_scale)]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=240, cwd=root)
    assert p.returncode == 0, p.stderr[-4000:]   # nothing further runs on the GPU after a failure
    T = {"fp32": torch.float32, "fp16": torch.float16}[dtype]
    net = networks.build_net(SIZE, seed=0, dtype=T, device=cuda)
    x0 = seeded(1, (n, 3, SIZE, SIZE)).to(cuda)
    t = seeded(2, (n, 3, SIZE, SIZE)).to(cuda)
    want, info = attack(net, x0, EPS, 3, target=t, random_start=True, seed=5, alpha=ALPHA,
                        universal=True, return_info=True, loss_scale=loss_scale)
    want, delta = want.cpu(), info["universal"]["delta"].cpu()
    if loss_scale is not None:
        assert info["rescales"] >= 1
    for r in range(world):
        res = torch.load(os.path.join(tmp_path, f"rank{r}.pt"), weights_only=True)
        print(f"world {world} rank {r}: {int((res['attack'] != want).sum())} of {want.numel()} "
              f"values and {int((res['delta'] != delta).sum())} of {delta.numel()} of delta "
              f"differ from attack(); rescales {res['rescales']}")
        assert torch.equal(res["attack"], want) and torch.equal(res["delta"], delta)
        assert res["linf"] == info["universal"]["linf"]
        if res["rescales"] >= 0:                 # a rank with a shard
            assert res["rescales"] == info["rescales"]
