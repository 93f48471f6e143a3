"""Timing of the two JPEG kernels and the effect of the JPEG-robust attack (one GPU, HIP events,
warm-up first):

    python tools/gpu/time_attack_jpeg.py [--kernel-reps 50] [--size 32] [--steps 10]

Without --part the tool runs its two parts one after the other, each as a fresh child process under
a time limit of its own (`timeout -k 10 SECONDS`), stops at the first one that fails and prints one
JSON line with what the parts printed. With --part NAME it runs that part alone.

"kernel": mia_jpeg_roundtrip and mia_jpeg_bwd_norms at 128 × 3 × 256² (quality 75) in µs next to
mia_di_resize_pad and a device-to-device copy_ of one fp32 tensor of that batch in the same process,
with the bytes each must move (round trip: 1 plane read and 1 written; adjoint: 2 and 1; copy_ and
DI: 1 and 1) and the effective bandwidth that gives. "effect": on the seeded synthetic networks at
--size, two images, equal eps and steps, per image the objective at J(adv) (quality 75) and the
share of the perturbation's energy that survives J, ‖J(adv) − J(x0)‖² / ‖adv − x0‖², for the
plain MI attack, jpeg_quality=75 with 'ste' and with 'cubic'. A record, not a test."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PARTS = {"kernel": 240, "effect": 300}  # seconds allowed per part


def time_kernels(dev, reps):
    import torch
    from gfa_amd import jpeg_quant_tables, ops
    from time_attack_si import event_ms
    N, S = 128, 256
    plane = 3 * S * S
    x = torch.rand(N, 3, S, S, device=dev) * 2 - 1
    g = torch.rand_like(x) * 2 - 1
    y = torch.empty_like(x)
    q = jpeg_quant_tables(75).to(dev, torch.float32)
    l1 = torch.zeros(N, device=dev)
    out = {"images": N, "size": S, "plane_bytes": 4 * N * plane}
    rows = (("jpeg_roundtrip", 2, lambda: ops.jpeg_roundtrip(x, y, q)),
            ("jpeg_bwd_norms", 3, lambda: ops.jpeg_bwd_norms(x, g, y, q, l1, None)),
            ("di_resize_pad", 2, lambda: ops.di_resize_pad(x, y, 230, 10, 12)),
            ("copy", 2, lambda: y.copy_(x)))
    for name, planes, fn in rows:
        ms = event_ms(fn, reps, 5)
        out[f"{name}_us"] = round(1e3 * ms, 1)
        out[f"{name}_GBps"] = round(planes * 4 * N * plane / (1e6 * ms), 1)
    assert bool(torch.isfinite(y).all())
    return out


def attack_effect(dev, size, steps):
    import torch
    from gfa_amd import attack, jpeg_compress, networks
    from gfa_amd.pgd import AttackEngine
    gen = torch.Generator().manual_seed(910)
    x0 = torch.rand((2, 3, size, size), generator=gen) * 2 - 1
    x0[1] *= 0.6
    t = torch.rand((2, 3, size, size), generator=gen) * 2 - 1
    net = networks.build_net(size, seed=0, dtype=torch.float32, device=dev)
    eps, alpha = 8 / 255, 2 / 255
    out = {"size": size, "eps": eps, "alpha": alpha, "steps": steps, "quality": 75}
    eng = AttackEngine(net.encoder.impl, net.decoder.impl, net.vgg.impl)
    eng.prepare(x0.to(dev), t.to(dev))
    jx0 = jpeg_compress(x0.to(dev), 75)
    out["at_x0"] = {"loss": eng.loss(x0.to(dev)).tolist(), "loss_jpeg": eng.loss(jx0).tolist()}
    runs = {"mi": dict(), "jpeg_ste": dict(jpeg_quality=75, jpeg_grad="ste"),
            "jpeg_cubic": dict(jpeg_quality=75, jpeg_grad="cubic")}
    for name, kw in runs.items():
        adv, info = attack(net, x0, eps, steps, target=t, alpha=alpha, momentum=1.0,
                           return_info=True, **kw)
        loss_j = eng.loss(jpeg_compress(adv.to(dev), 75))  # the plain attack reports none
        assert info["loss_jpeg"] is None or torch.equal(info["loss_jpeg"], loss_j)
        d = (adv.to(dev) - x0.to(dev)).reshape(2, -1)
        dj = (jpeg_compress(adv.to(dev), 75) - jx0).reshape(2, -1)
        out[name] = {"loss": info["loss"].tolist(), "loss_jpeg": loss_j.tolist(),
                     "energy_kept": ((dj * dj).sum(1) / (d * d).sum(1)).tolist()}
    return out


def run_part(part, a):
    import torch
    import gfa_import  # noqa: F401
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    dev = torch.device("cuda:0")
    if part == "kernel":
        return time_kernels(dev, a.kernel_reps)
    return attack_effect(dev, a.size, a.steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--size", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--part", choices=list(PARTS))
    a = ap.parse_args()
    if a.part:
        print(json.dumps({a.part: run_part(a.part, a)}))
        return 0
    out = {}
    for part, limit in PARTS.items():
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__),
               "--part", part, "--kernel-reps", str(a.kernel_reps), "--size", str(a.size),
               "--steps", str(a.steps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:  # a failed or hung part ends the run: nothing more starts on the GPU
            print(f"[time_attack_jpeg] part {part} ended with status {r.returncode}",
                  file=sys.stderr)
            print(json.dumps(out))
            return r.returncode
        out.update(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
