"""Timing of the patch-wise attack's fused step kernel and its objective fall (one GPU, HIP events,
warm-up first):

    python tools/gpu/time_attack_pi.py [--kernel-reps 50] [--size 32] [--step-size 256]

Without --part the tool runs its three parts one after the other, each as a fresh child process
under a time limit of its own (`timeout -k 10 SECONDS`), stops at the first one that fails and
prints one JSON line with what the parts printed. With --part NAME it runs that part alone.

"kernel": mia_pi_update at 128 × 3 × 256² for k = 3, 7 and 15 in µs (the m / A buffers swapped
every call, as the engine does) next to mia_mi_update and a device-to-device copy_ of one fp32
tensor of that batch in the same process, with the bytes each kernel must move (PI: 5 planes read
and 3 written; MI: 4 and 2; copy_: 1 and 1 — the halo re-reads are not counted) and the effective
bandwidth that gives. "step": one whole engine step, step_pi against step_mi, on the seeded
synthetic networks at --step-size. "objective": on the seeded synthetic networks at --size, per
image, the objective at x0 and after 10 steps at equal eps of MI, TI-DI-MI, PI (β = 10) and
TI-DI-PI. A record, not a test."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PARTS = {"kernel": 240, "step": 300, "objective": 300}  # seconds allowed per part


def time_kernels(dev, reps):
    import torch
    from gfa_amd import ops
    from time_attack_si import event_ms
    N, S = 128, 256
    plane = 3 * S * S
    x0 = torch.rand(N, 3, S, S, device=dev) * 2 - 1
    e, a = 16 / 255, 4 / 255
    ab = 10 * a
    g = torch.rand_like(x0) * 2 - 1
    l1 = g.abs().reshape(N, -1).sum(1)
    x = x0.clone()
    y = torch.empty_like(x0)
    m = [torch.zeros_like(x0), torch.zeros_like(x0)]
    A = [torch.zeros_like(x0), torch.zeros_like(x0)]
    out = {"images": N, "size": S, "plane_bytes": 4 * N * plane}
    calls = [0]

    def pi(k):
        i = calls[0] % 2
        calls[0] += 1
        ops.pi_update(x, x0, g, l1, m[i], m[1 - i], A[i], A[1 - i], 1.0, ab, ab, e, k)

    for k in (3, 7, 15):
        ms = event_ms(lambda: pi(k), reps, 5)
        out[f"pi_k{k}_us"] = round(1e3 * ms, 1)
        out[f"pi_k{k}_GBps"] = round(8 * 4 * N * plane / (1e6 * ms), 1)
    ms = event_ms(lambda: ops.mi_update(x, x0, g, l1, m[0], 1.0, a, e), reps, 5)
    out["mi_us"] = round(1e3 * ms, 1)
    out["mi_GBps"] = round(6 * 4 * N * plane / (1e6 * ms), 1)
    ms = event_ms(lambda: y.copy_(x0), reps, 5)
    out["copy_us"] = round(1e3 * ms, 1)
    out["copy_GBps"] = round(2 * 4 * N * plane / (1e6 * ms), 1)
    assert bool((x - x0).abs().max() <= e + 1e-6) and bool(torch.isfinite(A[0]).all())
    return out


def _net_and_images(dev, size, n=2):
    import torch
    from gfa_amd import networks
    g = torch.Generator().manual_seed(910)
    x0 = torch.rand((n, 3, size, size), generator=g) * 2 - 1
    x0[1] *= 0.6
    t = torch.rand((n, 3, size, size), generator=g) * 2 - 1
    return networks.build_net(size, seed=0, dtype=torch.float32, device=dev), x0, t


def time_steps(dev, size, reps):
    import torch
    from gfa_amd.pgd import AttackEngine, PiStep, pi_steps
    from time_attack_si import event_ms
    net, x0, t = _net_and_images(dev, size, 4)
    eng = AttackEngine(net.encoder.impl, net.decoder.impl, net.vgg.impl)
    eng.prepare(x0.to(dev), t.to(dev))
    e, a = 16 / 255, 4 / 255
    x = x0.to(dev).clone()
    m = [torch.zeros_like(x), torch.zeros_like(x)]
    A = [torch.zeros_like(x), torch.zeros_like(x)]
    pi = PiStep(*pi_steps(2 / 255, 10.0), 3)
    calls = [0]

    def step_pi():
        i = calls[0] % 2
        calls[0] += 1
        eng.step_pi(x, (m[i], m[1 - i]), (A[i], A[1 - i]), 1.0, e, pi)

    out = {"images": 4, "size": size}
    out["step_mi_ms"] = round(event_ms(lambda: eng.step_mi(x, m[0], 1.0, a, e), reps, 3), 3)
    out["step_pi_ms"] = round(event_ms(step_pi, reps, 3), 3)
    assert not eng.overflowed()
    return out


def objective_fall(dev, size):
    from gfa_amd import attack
    from gfa_amd.pgd import AttackEngine
    net, x0, t = _net_and_images(dev, size)
    eps, alpha = 8 / 255, 2 / 255
    eng = AttackEngine(net.encoder.impl, net.decoder.impl, net.vgg.impl)
    eng.prepare(x0.to(dev), t.to(dev))
    out = {"size": size, "eps": eps, "alpha": alpha, "steps": 10, "at_x0": eng.loss(x0.to(dev)).tolist()}
    del eng
    runs = {"mi": dict(), "ti_di_mi": dict(ti_kernel=5, di_prob=0.5),
            "pi_b10": dict(pi_amplification=10.0),
            "ti_di_pi_b10": dict(pi_amplification=10.0, ti_kernel=5, di_prob=0.5)}
    for name, kw in runs.items():
        _, info = attack(net, x0, eps, 10, target=t, alpha=alpha, momentum=1.0, return_info=True,
                         **kw)
        out[name] = info["loss"].tolist()
    return out


def run_part(part, a):
    import torch
    import gfa_import  # noqa: F401
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    dev = torch.device("cuda:0")
    if part == "kernel":
        return time_kernels(dev, a.kernel_reps)
    if part == "step":
        return time_steps(dev, a.step_size, a.step_reps)
    return objective_fall(dev, a.size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--step-reps", type=int, default=10)
    ap.add_argument("--size", type=int, default=32)
    ap.add_argument("--step-size", type=int, default=256)
    ap.add_argument("--part", choices=list(PARTS))
    a = ap.parse_args()
    if a.part:
        print(json.dumps({a.part: run_part(a.part, a)}))
        return 0
    out = {}
    for part, limit in PARTS.items():
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__),
               "--part", part, "--kernel-reps", str(a.kernel_reps), "--step-reps", str(a.step_reps),
               "--size", str(a.size), "--step-size", str(a.step_size)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:  # a failed or hung part ends the run: nothing more starts on the GPU
            print(f"[time_attack_pi] part {part} ended with status {r.returncode}", file=sys.stderr)
            print(json.dumps(out))
            return r.returncode
        out.update(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
