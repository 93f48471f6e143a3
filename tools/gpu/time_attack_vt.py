"""Timing of the variance-tuned attack and of its two kernels (one GPU, HIP events, warm-up first;
bench.py's networks and images for the attack):

    python tools/gpu/time_attack_vt.py [--batch 128 --size 256 --pgd-steps 3 --steps 1]
    python tools/gpu/time_attack_vt.py --kernel-only

Prints one JSON line:
* "attack": seconds per attack and milliseconds per iteration of the MI step (momentum=1.0) plain
  ("mi") and with --vt-samples 5 ("vt"), and "vt_vs_n1_mi" = step(vt) / ((N + 1) · step(mi)): 1.0
  means that N neighbours cost N further plain gradient passes and the kernels add nothing. The
  last step of an attack draws no neighbours and prepare() is shared, so the ratio of whole attacks
  lies below 1;
* "kernel": mia_vt_neighbor (with the look-ahead) and mia_vt_combine_norms (with gv and the sum;
  the last step's form without gv) alone at (planes, S) = (384, 256) and (96, 1024) as
  N = planes / 3 images: µs next to a device-to-device copy_ of the same tensor in the same
  process, and the neighbour kernel's element rate.
"mi" runs the same code as before variance tuning existed. A record, not a test."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from time_attack_si import event_ms  # noqa: E402


def time_kernels(dev, reps):
    from gfa_amd import ops
    rows = []
    for planes, S in ((384, 256), (96, 1024)):
        N = planes // 3
        x = torch.rand(N, 3, S, S, device=dev) * 2 - 1
        m = torch.rand(N, 3, S, S, device=dev) * 2 - 1
        gv = torch.rand(N, 3, S, S, device=dev) * 2 - 1
        y = torch.empty_like(x)
        v = torch.zeros_like(x)
        l1 = torch.zeros(N, device=dev)
        nf = torch.zeros(N, dtype=torch.int32, device=dev)
        ms_n = event_ms(lambda: ops.vt_neighbor(x, m, y, 0.0157, 0.094, 12345, 0, 3, 2), reps, 5)
        ms_p = event_ms(lambda: ops.vt_neighbor(x, None, y, 0.0, 0.094, 12345, 0, 3, 2), reps, 5)
        ms_c = event_ms(lambda: ops.vt_combine_norms(x, gv, v, y, l1, nf), reps, 5)
        ms_l = event_ms(lambda: ops.vt_combine_norms(x, None, v, y, l1, nf), reps, 5)
        ms_copy = event_ms(lambda: y.copy_(x), reps, 5)
        assert bool(torch.isfinite(y).all()) and not bool(nf.any())
        rows.append({"planes": planes, "size": S, "neighbor_us": round(1e3 * ms_n, 1),
                     "neighbor_no_lookahead_us": round(1e3 * ms_p, 1),
                     "combine_us": round(1e3 * ms_c, 1), "combine_last_us": round(1e3 * ms_l, 1),
                     "copy_us": round(1e3 * ms_copy, 1),
                     "neighbor_gelem_per_s": round(x.numel() / (1e6 * ms_p), 1)})
        print(f"[time_attack_vt] {planes} x {S}^2: neighbor {1e3 * ms_n:.1f} us (no look-ahead "
              f"{1e3 * ms_p:.1f} us), combine {1e3 * ms_c:.1f} us, last {1e3 * ms_l:.1f} us, copy "
              f"{1e3 * ms_copy:.1f} us", file=sys.stderr, flush=True)
        del x, m, gv, y, v
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--pgd-steps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=1, help="timed attacks per rule")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dtype", default="fp32", choices=list(bench.DT))
    ap.add_argument("--encoder", default="e4e", choices=["e4e", "linear"])
    ap.add_argument("--vt-samples", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--attack-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {}
    if not a.attack_only:
        out["kernel"] = time_kernels(dev, a.kernel_reps)
    if not a.kernel_only:
        eng = bench.build_engine(a, a.dtype, dev)
        g = torch.Generator().manual_seed(1000)
        S, B, k, n = a.size, a.batch, a.pgd_steps, a.vt_samples
        x0 = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev)
        tgt = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev)

        def rule(**kw):
            return lambda: eng.run_mi(x0, tgt, k, bench.EPS, bench.ALPHA, 1.0, **kw)
        rules = {"mi": rule(), "vt": rule(vt_samples=n, vt_seed=7)}
        res = {"batch": B, "size": S, "pgd_steps": k, "dtype": a.dtype, "encoder": a.encoder,
               "timed_attacks": a.steps, "vt_samples": n}
        for name, run in rules.items():
            holder = {}

            def once():
                holder["adv"] = run()
            ms = event_ms(once, a.steps, a.warmup)
            adv = holder["adv"]
            assert bool(torch.isfinite(adv).all()) and float(adv.abs().max()) <= 1.0
            res[name] = {"s_per_attack": round(ms / 1e3, 4), "ms_per_iter": round(ms / k, 3)}
            print(f"[time_attack_vt] {name}: {ms / 1e3:.3f} s per attack", file=sys.stderr,
                  flush=True)
        # k − 1 steps with N neighbours and one without: (k − 1)·(N + 1) + 1 gradient passes
        passes = (k - 1) * (n + 1) + 1
        res["vt"]["gradient_passes"] = passes
        res["vt"]["vt_vs_n1_mi"] = round(
            res["vt"]["ms_per_iter"] / ((n + 1) * res["mi"]["ms_per_iter"]), 4)
        res["vt"]["per_pass_vs_mi"] = round(
            res["vt"]["s_per_attack"] / passes / (res["mi"]["s_per_attack"] / k), 4)
        out["attack"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
