"""Data-parallel attack over the GPUs of one node.

Images are independent, so the batch is split into contiguous shards, one per rank (one process
per GPU, ``torch.distributed`` with the ``nccl`` backend = RCCL over xGMI). Every rank runs the
whole PGD loop on its shard with no collective in the data path; the only exchange is ONE
``all_gather_into_tensor`` of the final adversarial images (shards padded to equal size).
The one exception is the universal perturbation (``universal=True``), whose images share one δ:
it adds one all-reduce of an int64 plane per step, exact in any order.
The reference itself is single-GPU (``device = "cuda:0"``, attack_main2.py:843).
"""
import numbers

import numpy as np
import torch
import torch.distributed as dist


def shard_bounds(n, world, rank):
    """Contiguous, balanced split of n items: the first n % world ranks take one extra."""
    if world < 1 or not 0 <= rank < world:
        raise ValueError("bad world/rank")
    q, r = divmod(n, world)
    lo = rank * q + min(rank, r)
    hi = lo + q + (1 if rank < r else 0)
    return lo, hi


def gather_shards(local, n_total, group=None):
    """All-gather equal-padded shards and trim back to the first n_total rows (rank order)."""
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    per = -(-n_total // world)
    lo, hi = shard_bounds(n_total, world, rank)
    if local.shape[0] != hi - lo:
        raise ValueError("local shard size does not match shard_bounds")
    send = local.new_zeros((per,) + tuple(local.shape[1:]))
    send[: hi - lo] = local
    out = local.new_empty((per * world,) + tuple(local.shape[1:]))
    dist.all_gather_into_tensor(out, send.contiguous(), group=group)
    pieces = []
    for r in range(world):
        a, b = shard_bounds(n_total, world, r)
        pieces.append(out[r * per: r * per + (b - a)])
    return torch.cat(pieces, 0)


def attack_distributed(net, imgs, eps, steps, *, target, group=None, random_start=False, seed=0,
                       **kw):
    """Every rank passes the full batch (or at least its shape-compatible copy); each attacks its
    contiguous shard on its own GPU and all ranks return the full adversarial batch.

    * A rank whose shard is empty (world > n) runs no attack and contributes only the zero padding
      of the all-gather (every rank must still enter the collective).
    * The random-start noise is drawn ONCE for the full batch from ``seed`` (the same host draw as
      a single-GPU ``attack(..., random_start=True, seed=seed)``, the unit-L2-ball draw for
      ``norm="l2"``) and sliced per shard, so the output does not depend on the world size.
    * fp16 loss-scale overflows are decided job-wide (``pgd.rescale_consensus``, one int32 MAX
      all-reduce per attack run): every shard re-runs at the same λ, and a fatal overflow raises
      FloatingPointError on EVERY rank (an empty-shard rank included) before the all-gather, so
      no rank is left blocked in the collective.
    * Every other keyword (``norm``, ``momentum``, ``ti_kernel``, ``ti_nsig``, …) is forwarded to
      ``pgd.attack`` unchanged; the TI smoothing acts per image plane, so it is shard-local.
    * Input diversity (``di_prob``, ``di_resize_rate``, ``di_schedule``) is shard-local too: the
      draws are a host schedule that every rank computes from ``seed`` alone
      (``pgd.make_di_schedule``; one draw per step serves the whole batch), and the transform
      acts per image plane, so the output does not depend on the world size.
    * The scale copies and the Nesterov look-ahead (``si_scales``, ``nesterov``) act per image
      element, and the accumulated gradient's norms are per image: both are shard-local, and the
      output does not depend on the world size.
    * Variance tuning (``vt_samples``, ``vt_beta``): the neighbours' noise is a pure function of
      (seed, global image index, step, sample, element index), computed in the kernel with no
      state on host or device. Every shard is attacked with ``vt_first_image`` = the caller's
      value (default 0, the global index of ``imgs[0]``) + the shard's first row, so each image
      draws the noise it draws in a single-process attack of the full batch, and the output
      does not depend on the world size.
    * SPSA (``spsa_samples``, ``spsa_delta``): the black-box attack's random directions are the
      same kind of pure function of (seed, global image index, step, pair, element index). Every
      shard is attacked with ``spsa_first_image`` = the caller's value (default 0) + the shard's
      first row, so each image probes along the directions it takes in a single-process attack
      of the full batch, and the output does not depend on the world size.
    * Auto-PGD (``apgd=True``) needs nothing more: its step sizes, counters and best iterates
      are per image and live on the shard's device, and its only random state is the start
      noise sliced above, so the output does not depend on the world size.
    * SignHunter (``sign_hunter=True``) needs nothing more either: it draws no random number,
      its segments (``pgd.sh_schedule``) depend on the image size alone, and its sign planes,
      best objectives and decisions are per image on the shard's device, so the output does not
      depend on the world size.
    * The patch-wise attack (``pi_amplification=β``) needs nothing more: its momentum and
      accumulated-noise planes are per image on the shard's device, its window sum runs in a
      fixed order inside one plane, and its only random state is what the composed keywords
      bring (the start noise, the DI schedule and the VT noise, handled above), so an image's
      result depends on neither the batch nor the world size.
    * The JPEG-robust attack (``jpeg_quality``, ``jpeg_grad``) needs nothing more: the round trip
      and its adjoint act per image on 8 × 8 blocks, the quantiser tables depend on the quality
      alone and nothing is drawn, so the output does not depend on the world size.
    * The universal perturbation (``universal=True``) is the one attack whose images are not
      independent, and the one attack with a collective per step: every step all-reduces (SUM)
      the int64 plane of the summed normalised gradients over ``group``
      (``pgd.uap_all_reduce``; on the device for nccl, through a CPU copy for gloo). Integer sums
      are associative, so δ and the output do not depend on the world size, bit for bit. The
      start noise is ONE (1,3,S,S) draw from ``seed``, the same on every rank and not sliced.
      The range check counts the full batch (``pgd.check_universal_count``). A rank with an
      empty shard joins every step's all-reduce with a zero plane and applies the sum to a δ of
      its own (``pgd.idle_rank_universal``), then joins the status round, so no rank blocks and
      every rank ends with the same δ. With ``universal=True`` only, ``return_info=True`` is
      accepted and returns (the gathered batch, this rank's info): ``info["universal"]`` holds
      δ on every rank, the other entries describe the rank's own shard (an empty shard's info
      holds ``universal`` alone)."""
    from . import pgd
    group = group if group is not None else dist.group.WORLD
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    n = imgs.shape[0]
    lo, hi = shard_bounds(n, world, rank)
    gather_dev = torch.device("cpu") if dist.get_backend(group) == "gloo" else net.decoder.device
    universal = kw.get("universal", False)  # anything but a bool: attack() rejects it
    universal = isinstance(universal, (bool, np.bool_)) and bool(universal)
    want_info = universal and bool(kw.get("return_info", False))
    noise = None
    if universal:
        pgd.check_universal_count(n, imgs[0].numel() if n else 0)
        if random_start:  # one draw for the shared δ, the same on every rank: not sliced
            noise = kw.pop("start_noise", None)
            if noise is None:
                noise = pgd.make_start_noise((1,) + tuple(imgs.shape[1:]), seed, "linf")
    if hi == lo:
        info = None
        if universal:
            delta = pgd.idle_rank_universal(group, int(steps), (1,) + tuple(imgs.shape[1:]), eps,
                                            kw.get("alpha", 0.01), net.decoder.device,
                                            random_start, noise)
            delta = delta.to(imgs.device)
            info = dict(universal=dict(delta=delta, linf=float(delta.abs().max())))
        else:
            pgd.idle_rank_consensus(group)
        local = torch.zeros((0,) + tuple(imgs.shape[1:]), dtype=torch.float32, device=gather_dev)
        out = gather_shards(local, n, group).to(imgs.device)
        return (out, info) if want_info else out
    tgt = target if target.shape[0] == 1 else target[lo:hi]
    if random_start and not universal:
        noise_norm = "l2" if kw.get("norm", "linf") == "l2" else "linf"
        noise = pgd.make_start_noise(tuple(imgs.shape), seed, noise_norm)[lo:hi]
    if "vt_samples" in kw or "vt_first_image" in kw:
        first = kw.get("vt_first_image", 0)
        if isinstance(first, numbers.Integral) and not isinstance(first, bool):
            kw = dict(kw, vt_first_image=int(first) + lo)  # anything else: attack() rejects it
    if "spsa_samples" in kw or "spsa_first_image" in kw:
        first = kw.get("spsa_first_image", 0)
        if isinstance(first, numbers.Integral) and not isinstance(first, bool):
            kw = dict(kw, spsa_first_image=int(first) + lo)
    local = pgd.attack(net, imgs[lo:hi], eps, steps, target=tgt, random_start=random_start,
                       seed=seed, start_noise=noise, group=group, **kw)
    info = None
    if want_info:
        local, info = local
    out = gather_shards(local.to(gather_dev, torch.float32), n, group).to(imgs.device)
    return (out, info) if want_info else out
