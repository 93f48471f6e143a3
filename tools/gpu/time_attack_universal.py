"""Timing of the universal perturbation's two kernels and of its step (one GPU, HIP events,
warm-up first; bench.py's networks and images for the step):

    python tools/gpu/time_attack_universal.py [--batch 128 --size 256 --pgd-steps 3 --steps 2]
    python tools/gpu/time_attack_universal.py --kernel-only

Prints one JSON line:
* "kernel": mia_uap_accumulate (first = 1) and mia_uap_step (with the sum) alone on
  --batch × 3 × --size² fp32, µs per call and the achieved bytes/s against the traffic each must
  move: N planes read + 8·plane written for accumulate, N planes read + N written + δ read and
  written + acc read for step. Each call takes the next of --rotate sets of buffers, so that a
  batch that fits the last-level cache is not timed out of it; a device-to-device copy_ of the
  same batch (read N + write N planes) is timed the same way beside them. MIA_LIB_VARIANT selects
  an A/B build of the library (csrc/Makefile `variant`, e.g. -DMIA_UAP_SPLIT=8, the image-split
  form of accumulate on integer atomics); "acc_checksum" must agree between the two.
* "attack": milliseconds per iteration of the plain PGD step (AttackEngine.run) and of the
  universal step (run_universal) on the same batch, and their difference.
A record, not a test."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from time_attack_si import event_ms  # noqa: E402


def time_kernels(dev, N, S, reps, rotate):
    from gfa_amd import ops
    plane = 3 * S * S
    gen = torch.Generator().manual_seed(7)
    sets = []
    for _ in range(rotate):
        g = (torch.rand(N, 3, S, S, generator=gen) * 2 - 1).to(dev)
        sets.append(dict(g=g, l1=g.abs().reshape(N, -1).sum(1).contiguous(), x=torch.empty_like(g),
                         acc=torch.zeros(plane, dtype=torch.int64, device=dev),
                         delta=torch.zeros(1, 3, S, S, device=dev)))
    nf = torch.zeros(N, dtype=torch.int32, device=dev)
    turn = {"acc": 0, "step": 0, "copy": 0}

    def nxt(key):
        turn[key] += 1
        return sets[turn[key] % rotate]

    def accumulate():
        b = nxt("acc")
        ops.uap_accumulate(b["g"], b["l1"], b["acc"], True, nonfinite=nf)

    def step():
        b = nxt("step")
        ops.uap_step(b["delta"], b["acc"], b["x"], b["g"], 4 / 255, 16 / 255)

    def copy():
        b = nxt("copy")
        b["x"].copy_(b["g"])

    ms_a = event_ms(accumulate, reps, 2 * rotate)
    ms_s = event_ms(step, reps, 2 * rotate)
    ms_c = event_ms(copy, reps, 2 * rotate)
    assert not bool(nf.any())
    img = 4.0 * N * plane
    bytes_a, bytes_s, bytes_c = img + 8 * plane, 2 * img + 8 * plane + 8 * plane, 2 * img
    row = {"batch": N, "size": S, "rotate": rotate, "variant": os.environ.get("MIA_LIB_VARIANT"),
           "accumulate_us": round(1e3 * ms_a, 1), "step_us": round(1e3 * ms_s, 1),
           "copy_us": round(1e3 * ms_c, 1),
           "accumulate_tb_per_s": round(bytes_a / (1e9 * ms_a), 3),
           "step_tb_per_s": round(bytes_s / (1e9 * ms_s), 3),
           "copy_tb_per_s": round(bytes_c / (1e9 * ms_c), 3),
           "acc_checksum": int(sets[0]["acc"].sum())}
    print(f"[time_attack_universal] {N} x 3 x {S}^2: accumulate {1e3 * ms_a:.1f} us = "
          f"{row['accumulate_tb_per_s']} TB/s, step {1e3 * ms_s:.1f} us = {row['step_tb_per_s']} "
          f"TB/s, copy {1e3 * ms_c:.1f} us = {row['copy_tb_per_s']} TB/s", file=sys.stderr,
          flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--pgd-steps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=2, help="timed attacks per rule")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dtype", default="fp32", choices=list(bench.DT))
    ap.add_argument("--encoder", default="e4e", choices=["e4e", "linear"])
    ap.add_argument("--kernel-reps", type=int, default=60)
    ap.add_argument("--rotate", type=int, default=4)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--attack-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {}
    if not a.attack_only:
        out["kernel"] = time_kernels(dev, a.batch, a.size, a.kernel_reps, a.rotate)
    if not a.kernel_only:
        eng = bench.build_engine(a, a.dtype, dev)
        g = torch.Generator().manual_seed(1000)
        S, B, k = a.size, a.batch, a.pgd_steps
        x0 = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev)
        tgt = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev)
        rules = {"pgd": lambda: eng.run(x0, tgt, k, bench.EPS, bench.ALPHA),
                 "universal": lambda: eng.run_universal(x0, tgt, k, bench.EPS, bench.ALPHA)}
        res = {"batch": B, "size": S, "pgd_steps": k, "dtype": a.dtype, "encoder": a.encoder,
               "timed_attacks": a.steps}
        for name, run in rules.items():
            holder = {}

            def once():
                holder["adv"] = run()
            ms = event_ms(once, a.steps, a.warmup)
            adv = holder["adv"]
            assert bool(torch.isfinite(adv).all()) and float(adv.abs().max()) <= 1.0
            res[name] = {"s_per_attack": round(ms / 1e3, 4), "ms_per_iter": round(ms / k, 3)}
            print(f"[time_attack_universal] {name}: {ms / 1e3:.3f} s per attack", file=sys.stderr,
                  flush=True)
        res["universal_minus_pgd_ms_per_iter"] = round(
            res["universal"]["ms_per_iter"] - res["pgd"]["ms_per_iter"], 3)
        out["attack"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
