#!/usr/bin/env python3
"""Time and peak memory of the backbone FAPE (fcz_fape_dev, fcz_fape_grad_dev, foldcomp.fape) beside
foldcomp.smooth_lddt and beside the dense torch formulation with autograd, on the same tensors in one process -> one JSON document.

  --chains synthetic 350-residue chains as atom37 tensors (a CA random walk of 3.8 A steps, the workload of tools/lddt_rate.py, with
  N and C at 1.46 A and 1.52 A of every CA in random directions so that every residue has a frame), CA, clamp 10, scale 10, eps 1e-4,
  pred = true plus seeded Gaussian noise (sigma 0.5 A) on N, CA and C; the frames of both come from the coordinates.

    value                 fcz_fape_dev on the frames fcz_frames_dev gives for truth and prediction
    value_and_gradient    fcz_fape_dev, then fcz_fape_grad_dev (both of its sweeps) with the row weights of the loss
    fape                  foldcomp.fape(pred, true)["loss"].backward(): the truth's frames (fcz_frames_dev), Algorithm 21 in torch for the
                          prediction's, the three kernels, the chain sums in torch, autograd through the frame builder to pos.grad
    smooth_lddt           foldcomp.smooth_lddt(pred, true)["loss"].backward() on the same tensors
    torch_dense           the dense formulation in torch float32 with autograd ([c, L, L, 3] local coordinates of both sides, the
                          clamp, loss.backward() through the same frame builder) on the first c chains, c the largest count whose arrays
                          fit --dense-bytes at DENSE_LIVE live arrays; a c that still runs out of memory is halved until it fits

Every side: --warmup calls, then --reps calls, each timed by the host clock around the call and a device synchronise; the kernels'
HIP-event times (groups "fape", "fape_grad") are reported beside them. Peak memory is torch's allocator peak above what was allocated
before the call (the inputs). No rate is asserted: what is measured is recorded. A run without a GPU fails.

    python tools/fape_rate.py --out profiles/fape.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch

from knn_rate import stats, timed, walk

DENSE_LIVE = 10   # [c, L, L, 3] float32 arrays the dense formulation is assumed to hold at its peak, forward results kept for the backward


def dense_loss(frames, true_frames, x_t, x_p, clamp, scale, eps):
    """(rot [c, L, 3, 3], trans [c, L, 3]) of both sides, points [c, L, 3] -> the mean over the chains of mean min(d, clamp) / scale"""
    (rp, tp), (rt, tt) = frames, true_frames
    lp = torch.einsum("cfak,cfpa->cfpk", rp, x_p[:, None, :, :] - tp[:, :, None, :])
    lt = torch.einsum("cfak,cfpa->cfpk", rt, x_t[:, None, :, :] - tt[:, :, None, :])
    d = torch.sqrt(((lp - lt) ** 2).sum(-1) + eps).clamp(max=clamp)
    return (d.mean(dim=(1, 2)) / scale).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=16384)
    ap.add_argument("--residues", type=int, default=350)
    ap.add_argument("--clamp", type=float, default=10.0)
    ap.add_argument("--scale", type=float, default=10.0)
    ap.add_argument("--eps", type=float, default=1e-4)
    ap.add_argument("--noise", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dense-bytes", type=float, default=32e9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fape.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fape_rate: no HIP device; a time is measured on the GPU or not at all")
    import foldcomp_amd as foldcomp
    from foldcomp_amd import _lib, api, tensors
    dev = torch.device("cuda:0")
    torch.cuda.init()
    codec = api.default_codec()
    codec.enable_timing(True)
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    n, L, A = args.chains, args.residues, 37
    doc = {"slot": "CA", "layout": "atom37", "chains": n, "residues_per_chain": L, "clamp": args.clamp, "scale": args.scale, "eps": args.eps,
           "noise_sigma": args.noise, "device": torch.cuda.get_device_name(0),
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
        clear()
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
    for slot, bond in ((0, 1.46), (2, 1.52)):
        pos[:, :, slot] = pos[:, :, 1] + walk(n * L, dev, gen).view(n, L, 3) * (bond / 3.8)
    mask[:, :, :3] = 1
    pred = torch.zeros_like(pos)
    pred[:, :, :3] = pos[:, :, :3] + args.noise * torch.randn((n, L, 3, 3), device=dev, generator=gen)
    true = dict(pos=pos, mask=mask.view(torch.bool))
    ft = foldcomp.rigid_frames(true, codec=codec)
    fp = foldcomp.rigid_frames(dict(pos=pred, mask=mask.view(torch.bool)), codec=codec)
    doc["frames_true"], doc["frames_pred"] = int(ft["frame_mask"].sum()), int(fp["frame_mask"].sum())
    total = torch.empty((n, L), dtype=torch.float32, device=dev); points = torch.empty((n, L), dtype=torch.int32, device=dev)
    grot = torch.empty((n, L, 3, 3), dtype=torch.float32, device=dev)
    gtrans = torch.empty((n, L, 3), dtype=torch.float32, device=dev); gpos = torch.empty((n, L, 3), dtype=torch.float32, device=dev)
    lib, ctx = codec.lib, codec.ctx
    common = (ft["rot"].data_ptr(), ft["trans"].data_ptr(), ft["frame_mask"].data_ptr(), pos.data_ptr(), mask.data_ptr(), fp["rot"].data_ptr(),
              fp["trans"].data_ptr(), fp["frame_mask"].data_ptr(), pred.data_ptr(), None, None, n, L, 0, 1, args.clamp, args.eps)

    def value():
        _lib.check(lib.fcz_fape_dev(ctx, *common, total.data_ptr(), points.data_ptr()), "fcz_fape_dev")

    sync()
    value(); sync()
    weight = (1.0 / (n * args.scale * points.sum(dim=1, keepdim=True).clamp(min=1).to(torch.float64))).to(torch.float32).expand(n, L).contiguous()

    def value_and_gradient():
        value()
        _lib.check(lib.fcz_fape_grad_dev(ctx, *common, weight.data_ptr(), grot.data_ptr(), gtrans.data_ptr(), gpos.data_ptr()), "fcz_fape_grad_dev")

    wall, ev = kernel_times(value, ("fape",))
    doc["value"] = entry(wall, n, kernel=stats(ev))
    wall, ev = kernel_times(value_and_gradient, ("fape", "fape_grad"))
    doc["value_and_gradient"] = entry(wall, n, kernel=stats(ev))
    terms = float(points.to(torch.float64).sum())
    doc["terms"] = terms
    doc["mean_term"] = float(total.to(torch.float64).sum() / max(terms, 1.0))
    doc["value_terms_per_s"] = terms / (doc["value"]["kernel"]["median_ms"] * 1e-3)
    doc["value_and_gradient_over_value"] = doc["value_and_gradient"]["kernel"]["median_ms"] / doc["value"]["kernel"]["median_ms"]
    print(json.dumps({k: doc[k] for k in ("value", "value_and_gradient", "mean_term", "value_terms_per_s", "value_and_gradient_over_value")}), flush=True)

    # ---- the Python surfaces: forward and backward ---------------------------------------------------------------------------------
    leaf = pred.clone().requires_grad_()
    out = {}

    def no_grad_yet():
        leaf.grad = None

    def surface():
        leaf.grad = None
        out["loss"] = foldcomp.fape(leaf, true, clamp=args.clamp, scale=args.scale, eps=args.eps, codec=codec)["loss"]
        out["loss"].backward()

    def soft_surface():
        leaf.grad = None
        out["soft"] = foldcomp.smooth_lddt(leaf, true, codec=codec)["loss"]
        out["soft"].backward()

    wall = timed(soft_surface, sync, args.warmup, args.reps)
    doc["smooth_lddt"] = entry(wall, n, loss=float(out["soft"].detach()), peak_bytes=peak_of(soft_surface, no_grad_yet))
    wall = timed(surface, sync, args.warmup, args.reps)
    doc["fape"] = entry(wall, n, loss=float(out["loss"].detach()), peak_bytes=peak_of(surface, no_grad_yet), pos_grad_bytes=int(leaf.numel() * 4),
                        input_bytes=int(2 * pos.numel() * 4 + mask.numel()))
    doc["fape"]["peak_bytes_per_chain"] = doc["fape"]["peak_bytes"] / n
    doc["fape_over_smooth_lddt_ms"] = doc["fape"]["median_ms"] / doc["smooth_lddt"]["median_ms"]
    surface_grad = leaf.grad[:, :, :3].clone()
    print(json.dumps({k: doc[k] for k in ("smooth_lddt", "fape")}), flush=True)

    # ---- the dense torch formulation with autograd ---------------------------------------------------------------------------------
    c = max(1, min(n, int(args.dense_bytes // (4 * 3 * DENSE_LIVE * L * L))))
    dense = {}
    while True:
        cp = pred[:c, :, :3].clone().requires_grad_()
        tt = (ft["rot"][:c], ft["trans"][:c])

        def no_dense_grad_yet():
            cp.grad = None

        def dense_call():
            cp.grad = None
            rot, trans, _ = tensors.backbone_frames_torch(cp)
            dense["loss"] = dense_loss((rot, trans), tt, pos[:c, :, 1], cp[:, :, 1], args.clamp, args.scale, args.eps)
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
    doc["torch_dense"] = entry(wall, c, loss=float(dense["loss"].detach()), peak_bytes=peak, live_arrays_assumed=DENSE_LIVE, dense_bytes=args.dense_bytes,
                               peak_bytes_per_chain=peak / c)
    # the two agree up to float32 rounding (a sanity check of the workload, not of the bits): the dense loss is the mean over c chains,
    # the surface's over n, so its gradient is rescaled
    doc["max_abs_gradient_difference_to_torch"] = float((cp.grad - surface_grad[:c] * (n / c)).abs().max())
    doc["max_abs_gradient_of_torch"] = float(cp.grad.abs().max())
    doc["fape_over_torch_dense_chains_per_s"] = doc["fape"]["chains_per_s"] / doc["torch_dense"]["chains_per_s"]
    print(json.dumps(doc["torch_dense"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
