"""One rank of tests/test_gpu_uap.py's multi-process runs (launched by torch.distributed.run as a
child process of the test): attack_distributed(..., universal=True) on the REAL HIP engine, several
ranks sharing the box's one GPU over a gloo process group (the per-step all-reduce of the int64
plane goes through a CPU copy there). Writes this rank's gathered batch, its δ and its re-run
count (−1 for a rank with an empty shard) to $OUT/rank<r>.pt. Not a test module."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gfa_import  # noqa: E402,F401


def main():
    out_dir, n, dtype_name = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    loss_scale = None if sys.argv[4] == "None" else float(sys.argv[4])
    dtype = {"fp32": torch.float32, "fp16": torch.float16}[dtype_name]
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    try:
        torch.cuda.set_device(0)
        cuda = torch.device("cuda", 0)
        from gfa_amd import networks
        from gfa_amd.dist import attack_distributed
        from gpu_helpers import seeded
        net = networks.build_net(32, seed=0, dtype=dtype, device=cuda)
        x0 = seeded(1, (n, 3, 32, 32)).to(cuda)
        t = seeded(2, (n, 3, 32, 32)).to(cuda)
        got, info = attack_distributed(net, x0, 8 / 255, 3, target=t, random_start=True, seed=5,
                                       alpha=2 / 255, universal=True, return_info=True,
                                       loss_scale=loss_scale)
        torch.save({"attack": got.cpu(), "delta": info["universal"]["delta"].cpu(),
                    "linf": info["universal"]["linf"], "rescales": info.get("rescales", -1)},
                   os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
