"""Timing of the input-diversity attack and of its two kernels (one GPU, HIP events, warm-up first;
bench.py's networks and images for the attack):

    python tools/gpu/time_attack_di.py [--batch 128 --size 256 --pgd-steps 20 --steps 2]
    python tools/gpu/time_attack_di.py --kernel-only

Prints one JSON line:
* "attack": seconds per attack and per iteration of momentum=1.0 without ("mi") and with ("di",
  di_prob = 1.0: every step pays both kernels and one more assembly pass) input diversity, and
  their ratio;
* "kernel": mia_di_resize_pad and mia_di_resize_pad_bwd_norms (both sums on) alone at
  (planes, S) = (384, 256) and (96, 1024) as N = planes / 3 images, rnd = int(0.9·S) placed at
  (top, left) = (S − rnd, 0): µs, effective GB/s at 8 B per element (one read, one write of the
  full tensor), next to a device-to-device copy_ of the same tensor in the same process.
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


def time_kernels(dev, rate, reps):
    from gfa_amd import ops
    rows = []
    for planes, S in ((384, 256), (96, 1024)):
        N = planes // 3
        rnd = int(S * rate)
        top, left = S - rnd, 0
        x = torch.rand(N, 3, S, S, device=dev) * 2 - 1
        y = torch.empty_like(x)
        sums = torch.zeros(2, N, device=dev)
        nf = torch.zeros(N, dtype=torch.int32, device=dev)
        ms_f = event_ms(lambda: ops.di_resize_pad(x, y, rnd, top, left), reps, 5)
        ms_b = event_ms(lambda: ops.di_resize_pad_bwd_norms(x, y, sums[0], sums[1], rnd, top,
                                                            left, nf), reps, 5)
        ms_c = event_ms(lambda: y.copy_(x), reps, 5)
        gb = 8.0 * x.numel() / 1e9
        assert bool(torch.isfinite(y).all()) and not bool(nf.any())
        rows.append({"planes": planes, "size": S, "rnd": rnd, "top": top, "left": left,
                     "fwd_us": round(1e3 * ms_f, 1), "fwd_GBps": round(gb / (ms_f / 1e3), 1),
                     "bwd_us": round(1e3 * ms_b, 1), "bwd_GBps": round(gb / (ms_b / 1e3), 1),
                     "copy_us": round(1e3 * ms_c, 1), "copy_GBps": round(gb / (ms_c / 1e3), 1),
                     "fwd_vs_copy_rate": round(ms_c / ms_f, 3),
                     "bwd_vs_copy_rate": round(ms_c / ms_b, 3)})
        print(f"[time_attack_di] {planes} x {S}^2 rnd {rnd}: fwd {1e3 * ms_f:.1f} us, bwd "
              f"{1e3 * ms_b:.1f} us, copy {1e3 * ms_c:.1f} us", file=sys.stderr, flush=True)
        del x, y
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
    ap.add_argument("--di-resize-rate", type=float, default=0.9)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--attack-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {}
    if not a.attack_only:
        out["kernel"] = time_kernels(dev, a.di_resize_rate, a.kernel_reps)
    if not a.kernel_only:
        from gfa_amd import pgd
        eng = bench.build_engine(a, a.dtype, dev)
        g = torch.Generator().manual_seed(1000)
        S, B, k = a.size, a.batch, a.pgd_steps
        x0 = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev)
        tgt = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev)
        sched = pgd.make_di_schedule(k, S, a.di_resize_rate, 1.0, a.seed)
        rules = {
            "mi": lambda: eng.run_mi(x0, tgt, k, bench.EPS, bench.ALPHA, 1.0),
            "di": lambda: eng.run_mi(x0, tgt, k, bench.EPS, bench.ALPHA, 1.0, di=sched),
        }
        res = {"batch": B, "size": S, "pgd_steps": k, "dtype": a.dtype, "encoder": a.encoder,
               "timed_attacks": a.steps, "di_resize_rate": a.di_resize_rate, "di_prob": 1.0}
        for name, run in rules.items():
            holder = {}

            def once():
                holder["adv"] = run()
            ms = event_ms(once, a.steps, a.warmup)
            adv = holder["adv"]
            assert bool(torch.isfinite(adv).all()) and float(adv.abs().max()) <= 1.0
            res[name] = {"s_per_attack": round(ms / 1e3, 4), "ms_per_iter": round(ms / k, 3)}
            print(f"[time_attack_di] {name}: {ms / 1e3:.3f} s per attack", file=sys.stderr,
                  flush=True)
        res["di"]["vs_mi"] = round(res["di"]["s_per_attack"] / res["mi"]["s_per_attack"], 4)
        out["attack"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
