"""Timing of the two SPSA kernels (one GPU, HIP events, warm-up first):

    python tools/gpu/time_attack_spsa.py [--kernel-reps 50]

Prints one JSON line: "kernel" holds mia_spsa_probe (one read, two writes, one Philox block per 4
elements) and mia_spsa_accumulate_norms (the first pair: write only; a middle pair: read + write;
the last pair: read + write, the division and both sums) alone at (planes, S) = (384, 256) and
(96, 1024) as N = planes / 3 images: µs next to a device-to-device copy_ of the same tensor in the
same process, and the probe kernel's element rate. The attack itself is 2·q forward passes per
step around these kernels and is not timed here. A record, not a test."""
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
    rows = []
    for planes, S in ((384, 256), (96, 1024)):
        N = planes // 3
        x = torch.rand(N, 3, S, S, device=dev) * 2 - 1
        yp, ym, acc = torch.empty_like(x), torch.empty_like(x), torch.zeros_like(x)
        fp, fm = torch.rand(N, device=dev), torch.rand(N, device=dev)
        l1, l2 = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
        nf = torch.zeros(N, dtype=torch.int32, device=dev)
        ms_p = event_ms(lambda: ops.spsa_probe(x, yp, ym, 0.02, 12345, 0, 3, 2), reps, 5)
        ms_f = event_ms(lambda: ops.spsa_accumulate_norms(acc, fp, fm, None, None, 25.0, 12345, 0,
                                                          3, 0, True, nonfinite=nf), reps, 5)
        ms_m = event_ms(lambda: ops.spsa_accumulate_norms(acc, fp, fm, None, None, 25.0, 12345, 0,
                                                          3, 1, False, nonfinite=nf), reps, 5)
        ops.spsa_accumulate_norms(acc, fp, fm, None, None, 25.0, 12345, 0, 3, 0, True)
        ms_l = event_ms(lambda: ops.spsa_accumulate_norms(acc, fp, fm, l1, l2, 25.0, 12345, 0, 3,
                                                          2, False, 1.0009765625, nonfinite=nf),
                        reps, 5)
        ms_copy = event_ms(lambda: yp.copy_(x), reps, 5)
        assert bool(torch.isfinite(acc).all()) and not bool(nf.any())
        rows.append({"planes": planes, "size": S, "probe_us": round(1e3 * ms_p, 1),
                     "accumulate_first_us": round(1e3 * ms_f, 1),
                     "accumulate_middle_us": round(1e3 * ms_m, 1),
                     "accumulate_last_us": round(1e3 * ms_l, 1),
                     "copy_us": round(1e3 * ms_copy, 1),
                     "probe_gelem_per_s": round(x.numel() / (1e6 * ms_p), 1)})
        print(f"[time_attack_spsa] {planes} x {S}^2: probe {1e3 * ms_p:.1f} us, accumulate first "
              f"{1e3 * ms_f:.1f} us, middle {1e3 * ms_m:.1f} us, last {1e3 * ms_l:.1f} us, copy "
              f"{1e3 * ms_copy:.1f} us", file=sys.stderr, flush=True)
        del x, yp, ym, acc
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-reps", type=int, default=50)
    a = ap.parse_args()
    print(json.dumps({"kernel": time_kernels(torch.device("cuda:0"), a.kernel_reps)}))


if __name__ == "__main__":
    main()
