#!/usr/bin/env python3
"""Time and peak memory of the smooth lDDT (fcz_lddt_soft_dev, fcz_lddt_soft_grad_dev, foldcomp.smooth_lddt)
beside fcz_lddt_dev and beside the dense torch formulation with autograd, on the same tensors in one process -> one JSON document.

  --chains synthetic 350-residue chains as atom37 tensors (a CA random walk of 3.8 A steps), CA, cutoff 15, pred = true plus seeded
  Gaussian noise (sigma 0.5 A): the workload of tools/lddt_rate.py.

    lddt                  fcz_lddt_dev, the counting kernel the value kernel is a sibling of
    value                 fcz_lddt_soft_dev
    value_and_gradient    fcz_lddt_soft_dev, then fcz_lddt_soft_grad_dev with the row weights of the loss
    smooth_lddt           foldcomp.smooth_lddt(pred, true)["loss"].backward(): the two kernels, the chain sums in torch, pos.grad
    torch_dense           the dense formulation in torch float32 with autograd (two torch.cdist matrices [c, L, L], the
                          mask, four sigmoids, loss.backward()) on the first c chains, c the largest count whose matrices fit
                          --dense-bytes at DENSE_LIVE live matrices; a c that still runs out of memory is halved until it fits

Every side: --warmup calls, then --reps calls, each timed by the host clock around the call and a device synchronise; the kernels'
HIP-event times (groups "lddt", "lddt_soft", "lddt_soft_grad") are reported beside them. Peak memory is torch's allocator peak above
what was allocated before the call (the inputs), so it counts outputs, gradients and temporaries; for smooth_lddt that is above all
the gradient of pos's own shape, [n, L, 37, 3] (pos_grad_bytes), where the dense formulation differentiates a [c, L, 3] slice. No rate is asserted: what is
measured is recorded. A run without a GPU fails.

    python tools/lddt_soft_rate.py --out profiles/lddt_soft.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch

from knn_rate import stats, timed, walk

THRESHOLDS = (0.5, 1.0, 2.0, 4.0)
DENSE_LIVE = 12   # [c, L, L] float32 matrices the dense formulation is assumed to hold at its peak, forward results kept for the backward


def dense_loss(t, p, cutoff):
    """t, p [c, L, 3] (p requires grad) -> mean over the chains of 1 - sum eps / sum pairs, every row a site"""
    eye = torch.eye(t.shape[1], dtype=torch.bool, device=t.device)
    dt, dp = torch.cdist(t, t), torch.cdist(p, p)                             # (as tools/lddt_rate.py's baseline: the leanest torch has)
    inc = ((dt < cutoff) & ~eye).to(torch.float32)
    delta = (dt - dp).abs()
    eps = 0.25 * sum(torch.sigmoid(th - delta) for th in THRESHOLDS)
    return (1.0 - (eps * inc).sum(dim=(1, 2)) / inc.sum(dim=(1, 2)).clamp(min=1.0)).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=16384)
    ap.add_argument("--residues", type=int, default=350)
    ap.add_argument("--cutoff", type=float, default=15.0)
    ap.add_argument("--noise", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dense-bytes", type=float, default=32e9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lddt_soft.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lddt_soft_rate: no HIP device; a time is measured on the GPU or not at all")
    import foldcomp_amd as foldcomp
    from foldcomp_amd import _lib, api
    dev = torch.device("cuda:0")
    torch.cuda.init()
    codec = api.default_codec()
    codec.enable_timing(True)
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    n, L, A, cutoff = args.chains, args.residues, 37, args.cutoff
    th = (ctypes.c_float * 4)(*THRESHOLDS)
    doc = {"slot": "CA", "layout": "atom37", "chains": n, "residues_per_chain": L, "cutoff": cutoff, "thresholds": list(THRESHOLDS), "noise_sigma": args.noise,
           "device": torch.cuda.get_device_name(0),
           "method": f"host clock around call + synchronise, {args.warmup} warm-up and {args.reps} timed calls; *_kernel: HIP events of the named group; "
                     "peak_bytes: torch allocator peak above the inputs"}

    def sync():
        torch.cuda.synchronize(); codec.synchronize()

    def kernel_times(call, groups):
        ev = []

        def once():
            codec.reset_timing(); call(); codec.synchronize(); ev.append(sum(codec.kernel_time(g)[0] for g in groups))
        wall = timed(once, sync, args.warmup, args.reps)
        return wall, ev[args.warmup:]

    def peak_of(call, clear):
        clear()                                                               # (the gradient of the call before is no input)
        sync(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        call(); sync()
        return int(torch.cuda.max_memory_allocated(dev) - before)

    def entry(wall, chains, **more):
        d = dict(stats(wall), chains=chains, chains_per_s=chains / (statistics.median(wall) * 1e-3))
        d.update(more)
        return d

    pos = torch.zeros((n, L, A, 3), dtype=torch.float32, device=dev)
    mask = torch.zeros((n, L, A), dtype=torch.uint8, device=dev)
    pos[:, :, 1] = walk(n * L, dev, gen).view(n, L, 3).cumsum(dim=1)
    mask[:, :, 1] = 1
    pred = torch.zeros_like(pos)
    pred[:, :, 1] = pos[:, :, 1] + args.noise * torch.randn((n, L, 3), device=dev, generator=gen)
    score = torch.empty((n, L), dtype=torch.float32, device=dev)
    pairs = torch.empty((n, L), dtype=torch.int32, device=dev); hits = torch.empty((n, L), dtype=torch.int32, device=dev)
    soft = torch.empty((n, L), dtype=torch.float32, device=dev); spairs = torch.empty((n, L), dtype=torch.int32, device=dev)
    grad = torch.empty((n, L, 3), dtype=torch.float32, device=dev)
    lib, ctx = codec.lib, codec.ctx
    common = (pos.data_ptr(), mask.data_ptr(), pred.data_ptr(), None, None, n, L, 0, 1, cutoff, ctypes.addressof(th))

    def hard():
        _lib.check(lib.fcz_lddt_dev(ctx, *common, score.data_ptr(), pairs.data_ptr(), hits.data_ptr()), "fcz_lddt_dev")

    def value():
        _lib.check(lib.fcz_lddt_soft_dev(ctx, *common, soft.data_ptr(), spairs.data_ptr()), "fcz_lddt_soft_dev")

    sync()
    value(); sync()
    weight = (-1.0 / (n * spairs.sum(dim=1, keepdim=True).clamp(min=1).to(torch.float64))).to(torch.float32).expand(n, L).contiguous()

    def value_and_gradient():
        value()
        _lib.check(lib.fcz_lddt_soft_grad_dev(ctx, *common, weight.data_ptr(), grad.data_ptr()), "fcz_lddt_soft_grad_dev")

    wall, ev = kernel_times(hard, ("lddt",))
    doc["lddt"] = entry(wall, n, kernel=stats(ev))
    wall, ev = kernel_times(value, ("lddt_soft",))
    doc["value"] = entry(wall, n, kernel=stats(ev))
    wall, ev = kernel_times(value_and_gradient, ("lddt_soft", "lddt_soft_grad"))
    doc["value_and_gradient"] = entry(wall, n, kernel=stats(ev))
    hard(); sync()
    doc["pairs_equal_lddt_pairs"] = bool((pairs == spairs).all())
    doc["mean_pairs"] = float(spairs.to(torch.float32).mean())
    doc["mean_lddt"] = float(score.mean())
    doc["value_over_lddt"] = doc["value"]["kernel"]["median_ms"] / doc["lddt"]["kernel"]["median_ms"]
    doc["value_and_gradient_over_lddt"] = doc["value_and_gradient"]["kernel"]["median_ms"] / doc["lddt"]["kernel"]["median_ms"]
    print(json.dumps({k: doc[k] for k in ("lddt", "value", "value_and_gradient", "value_over_lddt", "value_and_gradient_over_lddt")}), flush=True)

    # ---- the Python surface: forward and backward ----------------------------------------------------------------------------------
    true = dict(pos=pos, mask=mask.view(torch.bool))
    leaf = pred.clone().requires_grad_()
    out = {}

    def no_grad_yet():
        leaf.grad = None

    def surface():
        leaf.grad = None
        out["loss"] = foldcomp.smooth_lddt(leaf, true, codec=codec)["loss"]
        out["loss"].backward()

    wall = timed(surface, sync, args.warmup, args.reps)
    doc["smooth_lddt"] = entry(wall, n, loss=float(out["loss"].detach()), peak_bytes=peak_of(surface, no_grad_yet),
                               pos_grad_bytes=int(leaf.numel() * 4), input_bytes=int(2 * pos.numel() * 4 + mask.numel()))
    surface_grad = leaf.grad[:, :, 1].clone()
    print(json.dumps(doc["smooth_lddt"]), flush=True)

    # ---- the dense torch formulation with autograd ---------------------------------------------------------------------------------
    c = max(1, min(n, int(args.dense_bytes // (4 * DENSE_LIVE * L * L))))
    ca = pos[:, :, 1].contiguous()
    dense = {}
    while True:
        cp = pred[:c, :, 1].clone().requires_grad_()

        def no_dense_grad_yet():
            cp.grad = None

        def dense_call():
            cp.grad = None
            dense["loss"] = dense_loss(ca[:c], cp, cutoff)
            dense["loss"].backward()
        try:
            wall = timed(dense_call, sync, args.warmup, args.reps)
            peak = peak_of(dense_call, no_dense_grad_yet)
            break
        except torch.cuda.OutOfMemoryError:
            del cp
            torch.cuda.empty_cache()
            if c == 1:
                raise
            c //= 2
    doc["torch_dense"] = entry(wall, c, loss=float(dense["loss"].detach()), peak_bytes=peak, live_matrices_assumed=DENSE_LIVE, dense_bytes=args.dense_bytes,
                               peak_bytes_per_chain=peak / c)
    # the two agree up to float32 rounding (a sanity check of the workload, not of the bits): the dense loss is the mean over c chains,
    # the surface's over n, so its gradient is rescaled
    doc["max_abs_gradient_difference_to_torch"] = float((cp.grad - surface_grad[:c] * (n / c)).abs().max())
    doc["max_abs_gradient_of_torch"] = float(cp.grad.abs().max())
    doc["smooth_lddt"]["peak_bytes_per_chain"] = doc["smooth_lddt"]["peak_bytes"] / n
    doc["smooth_lddt_over_torch_dense_chains_per_s"] = doc["smooth_lddt"]["chains_per_s"] / doc["torch_dense"]["chains_per_s"]
    print(json.dumps(doc["torch_dense"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
