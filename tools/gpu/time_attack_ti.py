"""Timing of the translation-invariant attack and of its blur kernel (one GPU, HIP events, warm-up
first; bench.py's networks and images for the attack):

    python tools/gpu/time_attack_ti.py [--batch 128 --size 256 --pgd-steps 20 --steps 2]
    python tools/gpu/time_attack_ti.py --kernel-only

Prints one JSON line:
* "attack": seconds per attack and per iteration of momentum=1.0 without ("mi") and with
  ("ti", --ti-kernel taps) the smoothing, and their ratio;
* "kernel": mia_ti_smooth_norms alone (both sums on) at (planes, H, W) = (384, 256, 256) and
  (96, 1024, 1024) as N = planes / 3 images: µs, effective GB/s at 8 B per element (one read,
  one write), next to a device-to-device copy_ of the same tensor in the same process.
Compare "mi" with the previous library's figure of the same session before reading the ratio."""
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


def time_kernel(dev, K, nsig, reps):
    from gfa_amd import ops, pgd
    taps = pgd.ti_gaussian_taps(K, nsig).float().to(dev)
    rows = []
    for planes, S in ((384, 256), (96, 1024)):
        N = planes // 3
        g = torch.rand(N, 3, S, S, device=dev) * 2 - 1
        gs = torch.empty_like(g)
        sums = torch.zeros(2, N, device=dev)
        nf = torch.zeros(N, dtype=torch.int32, device=dev)
        ms_k = event_ms(lambda: ops.ti_smooth_norms(g, taps, gs, sums[0], sums[1], nf), reps, 5)
        ms_c = event_ms(lambda: gs.copy_(g), reps, 5)
        gb = 8.0 * g.numel() / 1e9
        assert bool(torch.isfinite(gs).all()) and not bool(nf.any())
        rows.append({"planes": planes, "size": S, "K": K,
                     "kernel_us": round(1e3 * ms_k, 1), "kernel_GBps": round(gb / (ms_k / 1e3), 1),
                     "copy_us": round(1e3 * ms_c, 1), "copy_GBps": round(gb / (ms_c / 1e3), 1),
                     "kernel_vs_copy_rate": round(ms_c / ms_k, 3)})
        print(f"[time_attack_ti] kernel {planes} x {S}^2: {1e3 * ms_k:.1f} us, copy "
              f"{1e3 * ms_c:.1f} us", file=sys.stderr, flush=True)
        del g, gs
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--pgd-steps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=2, help="timed attacks per rule")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dtype", default="fp32", choices=list(bench.DT))
    ap.add_argument("--encoder", default="e4e", choices=["e4e", "linear"])
    ap.add_argument("--ti-kernel", type=int, default=15)
    ap.add_argument("--ti-nsig", type=float, default=3.0)
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--attack-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {}
    if not a.attack_only:
        out["kernel"] = time_kernel(dev, a.ti_kernel, a.ti_nsig, a.kernel_reps)
    if not a.kernel_only:
        from gfa_amd import pgd
        eng = bench.build_engine(a, a.dtype, dev)
        g = torch.Generator().manual_seed(1000)
        S, B, k = a.size, a.batch, a.pgd_steps
        x0 = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev)
        tgt = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev)
        taps = pgd.ti_gaussian_taps(a.ti_kernel, a.ti_nsig)
        rules = {
            "mi": lambda: eng.run_mi(x0, tgt, k, bench.EPS, bench.ALPHA, 1.0),
            "ti": lambda: eng.run_mi(x0, tgt, k, bench.EPS, bench.ALPHA, 1.0, ti_taps=taps),
        }
        res = {"batch": B, "size": S, "pgd_steps": k, "dtype": a.dtype, "encoder": a.encoder,
               "timed_attacks": a.steps, "ti_kernel": a.ti_kernel}
        for name, run in rules.items():
            holder = {}

            def once():
                holder["adv"] = run()
            ms = event_ms(once, a.steps, a.warmup)
            adv = holder["adv"]
            assert bool(torch.isfinite(adv).all()) and float(adv.abs().max()) <= 1.0
            res[name] = {"s_per_attack": round(ms / 1e3, 4), "ms_per_iter": round(ms / k, 3)}
            print(f"[time_attack_ti] {name}: {ms / 1e3:.3f} s per attack", file=sys.stderr,
                  flush=True)
        res["ti"]["vs_mi"] = round(res["ti"]["s_per_attack"] / res["mi"]["s_per_attack"], 4)
        out["attack"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
