"""Timing of the scale-invariant / Nesterov attack and of its two kernels (one GPU, HIP events,
warm-up first; bench.py's networks and images for the attack):

    python tools/gpu/time_attack_si.py [--batch 128 --size 256 --pgd-steps 10 --steps 1]
    python tools/gpu/time_attack_si.py --kernel-only

Prints one JSON line:
* "attack": seconds per attack and milliseconds per iteration of the MI step (momentum=1.0) with
  si_scales 1 ("mi") and --si-scales 5 ("si"), each without and with the look-ahead ("ni",
  "si_ni"), and "si_vs_n_mi" = step(n) / (n · step(1)): 1.0 means that n scale copies cost n
  plain gradient passes and the kernels, the accumulation and the once-per-step work add nothing;
* "kernel": mia_si_transform (look-ahead and s = 1/2) and mia_si_accumulate_norms (a middle copy;
  the last copy with the division and both sums) alone at (planes, S) = (384, 256) and
  (96, 1024) as N = planes / 3 images: µs next to a device-to-device copy_ of the same tensor in
  the same process.
"mi" runs the same code as before scale invariance existed: compare it with the previous
library's figure of the same session before reading the ratio. A record, not a test."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def event_ms(fn, reps, warmup):
    """Mean milliseconds of fn() over reps launches between two HIP events, after warmup."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps


def time_kernels(dev, reps):
    from gfa_amd import ops
    rows = []
    for planes, S in ((384, 256), (96, 1024)):
        N = planes // 3
        x = torch.rand(N, 3, S, S, device=dev) * 2 - 1
        m = torch.rand(N, 3, S, S, device=dev) * 2 - 1
        y = torch.empty_like(x)
        acc = torch.zeros_like(x)
        sums = torch.zeros(2, N, device=dev)
        nf = torch.zeros(N, dtype=torch.int32, device=dev)
        ms_t = event_ms(lambda: ops.si_transform(x, m, y, 0.0157, 0.5), reps, 5)
        ms_a = event_ms(lambda: ops.si_accumulate_norms(x, acc, None, None, 0.5, False, 1.0, nf),
                        reps, 5)
        ops.zero_(acc)
        ms_l = event_ms(lambda: ops.si_accumulate_norms(x, acc, sums[0], sums[1], 0.0625, False,
                                                        5.0, nf), reps, 5)
        ms_c = event_ms(lambda: y.copy_(x), reps, 5)
        assert bool(torch.isfinite(acc).all()) and not bool(nf.any())
        rows.append({"planes": planes, "size": S,
                     "transform_us": round(1e3 * ms_t, 1), "accumulate_us": round(1e3 * ms_a, 1),
                     "accumulate_last_us": round(1e3 * ms_l, 1), "copy_us": round(1e3 * ms_c, 1)})
        print(f"[time_attack_si] {planes} x {S}^2: transform {1e3 * ms_t:.1f} us, accumulate "
              f"{1e3 * ms_a:.1f} us, last {1e3 * ms_l:.1f} us, copy {1e3 * ms_c:.1f} us",
              file=sys.stderr, flush=True)
        del x, m, y, acc
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--pgd-steps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=1, help="timed attacks per rule")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dtype", default="fp32", choices=list(bench.DT))
    ap.add_argument("--encoder", default="e4e", choices=["e4e", "linear"])
    ap.add_argument("--si-scales", type=int, default=5)
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
        S, B, k, n = a.size, a.batch, a.pgd_steps, a.si_scales
        x0 = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev)
        tgt = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev)

        def rule(**kw):
            return lambda: eng.run_mi(x0, tgt, k, bench.EPS, bench.ALPHA, 1.0, **kw)
        rules = {"mi": rule(), "ni": rule(nesterov=True), "si": rule(si_scales=n),
                 "si_ni": rule(si_scales=n, nesterov=True)}
        res = {"batch": B, "size": S, "pgd_steps": k, "dtype": a.dtype, "encoder": a.encoder,
               "timed_attacks": a.steps, "si_scales": n}
        for name, run in rules.items():
            holder = {}

            def once():
                holder["adv"] = run()
            ms = event_ms(once, a.steps, a.warmup)
            adv = holder["adv"]
            assert bool(torch.isfinite(adv).all()) and float(adv.abs().max()) <= 1.0
            res[name] = {"s_per_attack": round(ms / 1e3, 4), "ms_per_iter": round(ms / k, 3)}
            print(f"[time_attack_si] {name}: {ms / 1e3:.3f} s per attack", file=sys.stderr,
                  flush=True)
        res["si"]["si_vs_n_mi"] = round(res["si"]["ms_per_iter"] / (n * res["mi"]["ms_per_iter"]), 4)
        res["si_ni"]["si_vs_n_mi"] = round(
            res["si_ni"]["ms_per_iter"] / (n * res["ni"]["ms_per_iter"]), 4)
        res["ni"]["vs_mi"] = round(res["ni"]["ms_per_iter"] / res["mi"]["ms_per_iter"], 4)
        out["attack"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
