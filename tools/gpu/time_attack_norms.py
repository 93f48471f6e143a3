"""Whole-attack timing of the three sign / normalised update rules on the bench's workload
(bench.py's networks, images, warm-up and timed-region discipline; one GPU):

    python tools/gpu/time_attack_norms.py [--batch 128 --size 256 --pgd-steps 20 --steps 2]

Prints one JSON line: seconds per attack and per PGD iteration for norm="linf" (the plain
bench.py rule), norm="l2" (AttackEngine.run_l2) and momentum=1.0 (AttackEngine.run_mi), and the
two new rules' ratio to linf. Compare the linf figure with the plain `bench.py` line of the same
box before reading the ratios."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--pgd-steps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=2, help="timed attacks per rule")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dtype", default="fp32", choices=list(bench.DT))
    ap.add_argument("--encoder", default="e4e", choices=["e4e", "linear"])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    eng = bench.build_engine(a, a.dtype, dev)
    g = torch.Generator().manual_seed(1000)
    S, B = a.size, a.batch
    x0 = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev)
    tgt = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev)
    k = a.pgd_steps
    rules = {
        "linf": lambda: eng.run(x0, tgt, k, bench.EPS, bench.ALPHA),
        "l2": lambda: eng.run_l2(x0, tgt, k, 1.0, 0.2),
        "mi": lambda: eng.run_mi(x0, tgt, k, bench.EPS, bench.ALPHA, 1.0),
    }
    out = {"batch": B, "size": S, "pgd_steps": k, "dtype": a.dtype, "encoder": a.encoder,
           "timed_attacks": a.steps}
    for name, run in rules.items():
        for _ in range(a.warmup):
            run()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            adv = run()
        torch.cuda.synchronize(dev)
        dt = (time.perf_counter() - t0) / a.steps
        assert bool(torch.isfinite(adv).all()) and float(adv.abs().max()) <= 1.0
        out[name] = {"s_per_attack": round(dt, 4), "ms_per_iter": round(1e3 * dt / k, 3)}
        print(f"[time_attack_norms] {name}: {dt:.3f} s per attack", file=sys.stderr, flush=True)
    for name in ("l2", "mi"):
        out[name]["vs_linf"] = round(out[name]["s_per_attack"] / out["linf"]["s_per_attack"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
