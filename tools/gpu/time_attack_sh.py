"""Timing of the SignHunter flip kernel and the attack's objective fall (one GPU, HIP events,
warm-up first):

    python tools/gpu/time_attack_sh.py [--kernel-reps 50] [--size 32]

Prints one JSON line. "kernel": mia_sh_flip at 128 × 256² (N = 128 images of 3·256² elements) for
three segments — the whole plane, plane/64 and a single element — in µs next to a device-to-device
copy_ of one fp32 tensor of that batch in the same process; each timed call flips the segment
and reverts nothing (accept = 1 everywhere), so every call does the same work. "objective": on the
seeded synthetic networks at --size, per image, the objective at x0, at SignHunter's query 0 and
after 31 flips (32 queries), next to SPSA with the same 32 queries (spsa_samples=4, 4 steps,
alpha = eps/4) on the same images. A record, not a test."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import gfa_import  # noqa: E402,F401
from time_attack_si import event_ms  # noqa: E402


def time_kernels(dev, reps):
    from gfa_amd import ops
    N, S = 128, 256
    plane = 3 * S * S
    x0 = torch.rand(N, 3, S, S, device=dev) * 2 - 1
    x, y = torch.empty_like(x0), torch.empty_like(x0)
    s = torch.full((N, 3, S, S), -1, dtype=torch.int8, device=dev)
    acc = torch.ones(N, dtype=torch.int32, device=dev)
    e = 16 / 255
    ops.sh_flip(x, x0, s, None, None, (0, plane), e)
    out = {"images": N, "size": S}
    mid = plane // 2 + 1
    for name, seg in (("whole_plane", (0, plane)), ("plane_64th", (mid, mid + plane // 64)),
                      ("one_element", (mid, mid + 1))):
        ms = event_ms(lambda: ops.sh_flip(x, x0, s, acc, seg, seg, e), reps, 5)
        out[name + "_us"] = round(1e3 * ms, 1)
    # prev = new with accept = 1 flips the segment once per call; both ranges are walked
    ms_copy = event_ms(lambda: y.copy_(x0), reps, 5)
    out["copy_us"] = round(1e3 * ms_copy, 1)
    out["whole_plane_bytes"] = N * plane * (4 + 4 + 1 + 1)
    assert bool((x - x0).abs().max() <= e + 1e-6) and bool((s.abs() == 1).all())
    print(f"[time_attack_sh] {N} x {S}^2: {out}", file=sys.stderr, flush=True)
    return out


def objective_fall(dev, size):
    from gfa_amd import attack, networks
    from gfa_amd.pgd import AttackEngine
    g = torch.Generator().manual_seed(910)
    x0 = torch.rand((2, 3, size, size), generator=g) * 2 - 1
    x0[1] *= 0.6
    t = torch.rand((2, 3, size, size), generator=g) * 2 - 1
    net = networks.build_net(size, seed=0, dtype=torch.float32, device=dev)
    eps = 8 / 255
    eng = AttackEngine(net.encoder.impl, net.decoder.impl, net.vgg.impl)
    eng.prepare(x0.to(dev), t.to(dev))
    at_x0 = eng.loss(x0.to(dev)).tolist()
    del eng
    _, info = attack(net, x0, eps, 31, target=t, sign_hunter=True, return_info=True)
    sh = info["sign_hunter"]
    _, sp = attack(net, x0, eps, 4, target=t, alpha=eps / 4, spsa_samples=4, return_info=True)
    out = {"size": size, "eps": eps, "at_x0": at_x0, "sh_query0": sh["loss"][0].tolist(),
           "sh_after_31_flips": sh["best"].tolist(), "sh_accepted": sh["accepted"].tolist(),
           "sh_queries": info["queries"], "spsa_q4_4steps": sp["loss"].tolist(),
           "spsa_queries": sp["queries"]}
    print(f"[time_attack_sh] objective: {out}", file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--size", type=int, default=32)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print(json.dumps({"kernel": time_kernels(dev, a.kernel_reps),
                      "objective": objective_fall(dev, a.size)}))


if __name__ == "__main__":
    main()
