#!/usr/bin/env python3
"""Time and peak memory of the all-atom FAPE (fcz_fape_atoms_dev, fcz_fape_atoms_grad_dev, foldcomp.fape_atoms)
beside the backbone foldcomp.fape and beside the dense torch formulation with autograd, on the same tensors in one process -> one
JSON document.

  --chains synthetic 350-residue chains as atom14 tensors: a CA random walk of 3.8 A steps, uniform residue types, every atom the type
  has (the non-zero entries of the default radii table) scattered 1.5 A about its CA, so that every group the type has is a frame (4.0
  a residue with uniform types) and every atom a point (8.4 a residue); pred = true plus seeded Gaussian noise (sigma 0.5 A); clamp 10, scale 10, eps 1e-4.

    value                 fcz_fape_atoms_dev on the eight-group frames fcz_frames_dev gives for truth and prediction, swapped from
                          foldcomp.lddt_atoms
    value_and_gradient    fcz_fape_atoms_dev, then fcz_fape_atoms_grad_dev (both of its sweeps) with the item weights of the loss
    fape_atoms            foldcomp.fape_atoms(pred, true)["loss"].backward(): lddt_atoms for the renaming, the truth's frames
                          (fcz_frames_dev), rigid_frames_torch for the prediction's, the three kernels, the chain sums in torch, autograd
                          through the frame builder to pos.grad
    fape_atoms_no_rename  the same with rename=None
    fape                  the backbone foldcomp.fape(pred, true)["loss"].backward() on the same tensors (CA)
    torch_dense           the dense formulation in torch float32 with autograd ([c, 8 L, A L, 3] local coordinates of both sides under
                          the frame and point masks, the clamp, loss.backward() through rigid_frames_torch) on the first c chains, c the
                          largest count whose arrays fit --dense-bytes at DENSE_LIVE live arrays; a c that still runs out of memory is
                          halved until it fits: the chunking the dense formulation needs

Every side: --warmup calls, then --reps calls, each timed by the host clock around the call and a device synchronise; the kernels'
HIP-event times (groups "fape_atoms", "fape_atoms_grad") are reported beside them. Peak memory is torch's allocator peak above what was
allocated before the call (the inputs). frame_lane_share is the share of the lanes of the frame sweeps' rounds that hold a frame
(tiles of fcz_fape_atoms_tile_rows rows, rounds of 256). No rate is asserted: what is measured is recorded. A run without a GPU fails.

    python tools/fape_atoms_rate.py --out profiles/fape_atoms.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

from knn_rate import stats, timed, walk

DENSE_LIVE = 10   # [c, 8 L, A L, 3] float32 arrays the dense formulation is assumed to hold at its peak, forward results kept for the backward
BLOCK = 256


def dense_loss(frames, true_frames, fmask, x_t, x_p, pmask, clamp, scale, eps):
    """(rot [c, F, 3, 3], trans [c, F, 3]) of both sides, fmask [c, F], points [c, P, 3], pmask [c, P] -> the mean over the chains of
    the masked mean of min(d, clamp) / scale"""
    (rp, tp), (rt, tt) = frames, true_frames
    lp = torch.einsum("cfak,cfpa->cfpk", rp, x_p[:, None, :, :] - tp[:, :, None, :])
    lt = torch.einsum("cfak,cfpa->cfpk", rt, x_t[:, None, :, :] - tt[:, :, None, :])
    d = torch.sqrt(((lp - lt) ** 2).sum(-1) + eps).clamp(max=clamp)
    pair = fmask[:, :, None] & pmask[:, None, :]
    return ((d * pair).sum(dim=(1, 2)) / (pair.sum(dim=(1, 2)).clamp(min=1) * scale)).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--residues", type=int, default=350)
    ap.add_argument("--clamp", type=float, default=10.0)
    ap.add_argument("--scale", type=float, default=10.0)
    ap.add_argument("--eps", type=float, default=1e-4)
    ap.add_argument("--noise", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dense-bytes", type=float, default=32e9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fape_atoms.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fape_atoms_rate: no HIP device; a time is measured on the GPU or not at all")
    import foldcomp_amd as foldcomp
    from foldcomp_amd import _lib, api, tensors
    dev = torch.device("cuda:0")
    torch.cuda.init()
    codec = api.default_codec()
    codec.enable_timing(True)
    lib, ctx = codec.lib, codec.ctx
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    n, L, A, G = args.chains, args.residues, 14, 8
    doc = {"layout": "atom14", "chains": n, "residues_per_chain": L, "clamp": args.clamp, "scale": args.scale, "eps": args.eps, "noise_sigma": args.noise,
           "device": torch.cuda.get_device_name(0), "point_pass": int(lib.fcz_fape_atoms_pass()), "frame_tile_rows": int(lib.fcz_fape_atoms_tile_rows(1)),
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

    radii = np.zeros((21, A), np.float32)
    _lib.check(lib.fcz_sasa_default_radii(1, radii.ctypes.data), "fcz_sasa_default_radii")
    has = torch.from_numpy(radii != 0).to(dev)
    aatype = torch.randint(0, 20, (n, L), device=dev, generator=gen, dtype=torch.int64).to(torch.uint8)
    mask = has[aatype.long()].contiguous()
    ca = walk(n * L, dev, gen).view(n, L, 3).cumsum(dim=1)
    pos = (ca[:, :, None, :] + torch.randn((n, L, A, 3), device=dev, generator=gen) * (1.5 / 3 ** 0.5)).contiguous()
    pos[:, :, 1] = ca
    pred = (pos + args.noise * torch.randn((n, L, A, 3), device=dev, generator=gen)).contiguous()
    true = dict(pos=pos, mask=mask, aatype=aatype)
    ft = foldcomp.rigid_frames(true, groups="all", codec=codec)
    fp = foldcomp.rigid_frames(dict(pos=pred, mask=mask, aatype=aatype), groups="all", codec=codec)
    swapped = foldcomp.lddt_atoms(dict(pos=pred, mask=mask), true, codec=codec)["swapped"].view(torch.uint8)
    both = ft["frame_mask"] & fp["frame_mask"]
    doc["frames_per_residue"] = float(both.sum()) / (n * L)
    doc["points_per_residue"] = float(mask.sum()) / (n * L)
    doc["rows_swapped"] = int(swapped.sum())
    T = doc["frame_tile_rows"]
    pad = (-L) % T
    per_tile = torch.nn.functional.pad(both.sum(-1), (0, pad)).view(n, -1, T).sum(-1)
    doc["frame_lane_share"] = float(per_tile.sum()) / float((torch.div(per_tile + BLOCK - 1, BLOCK, rounding_mode="floor") * BLOCK).sum())
    doc["frame_lane_share_without_compaction"] = float(both.sum()) / (n * ((L + T - 1) // T) * T * G)
    total = torch.empty((n, L, G), dtype=torch.float32, device=dev); points = torch.empty((n, L, G), dtype=torch.int32, device=dev)
    grot = torch.empty((n, L, G, 3, 3), dtype=torch.float32, device=dev)
    gtrans = torch.empty((n, L, G, 3), dtype=torch.float32, device=dev); gpos = torch.empty((n, L, A, 3), dtype=torch.float32, device=dev)
    mask8 = mask.view(torch.uint8)
    common = (ft["rot"].data_ptr(), ft["trans"].data_ptr(), ft["frame_mask"].data_ptr(), pos.data_ptr(), mask8.data_ptr(), aatype.data_ptr(), swapped.data_ptr(),
              fp["rot"].data_ptr(), fp["trans"].data_ptr(), fp["frame_mask"].data_ptr(), pred.data_ptr(), None, None, n, L, 1, args.clamp, args.eps, None)

    def value():
        _lib.check(lib.fcz_fape_atoms_dev(ctx, *common, total.data_ptr(), points.data_ptr()), "fcz_fape_atoms_dev")

    sync()
    value(); sync()
    weight = (1.0 / (n * args.scale * points.sum(dim=(1, 2), keepdim=True).clamp(min=1).to(torch.float64))).to(torch.float32).expand(n, L, G).contiguous()

    def value_and_gradient():
        value()
        _lib.check(lib.fcz_fape_atoms_grad_dev(ctx, *common, weight.data_ptr(), grot.data_ptr(), gtrans.data_ptr(), gpos.data_ptr()), "fcz_fape_atoms_grad_dev")

    wall, ev = kernel_times(value, ("fape_atoms",))
    doc["value"] = entry(wall, n, kernel=stats(ev))
    wall, ev = kernel_times(value_and_gradient, ("fape_atoms", "fape_atoms_grad"))
    doc["value_and_gradient"] = entry(wall, n, kernel=stats(ev))
    terms = float(points.to(torch.float64).sum())
    doc["terms"] = terms
    doc["terms_per_chain"] = terms / n
    doc["mean_term"] = float(total.to(torch.float64).sum() / max(terms, 1.0))
    doc["value_terms_per_s"] = terms / (doc["value"]["kernel"]["median_ms"] * 1e-3)
    doc["value_and_gradient_terms_per_s"] = terms / (doc["value_and_gradient"]["kernel"]["median_ms"] * 1e-3)
    doc["value_and_gradient_over_value"] = doc["value_and_gradient"]["kernel"]["median_ms"] / doc["value"]["kernel"]["median_ms"]
    print(json.dumps({k: doc[k] for k in ("value", "value_and_gradient", "mean_term", "value_terms_per_s", "value_and_gradient_over_value", "frame_lane_share")}), flush=True)
    del grot, gtrans, gpos

    # ---- the Python surfaces: forward and backward ---------------------------------------------------------------------------------
    leaf = pred.clone().requires_grad_()
    out = {}

    def no_grad_yet():
        leaf.grad = None

    def surface(key, **kw):
        def call():
            leaf.grad = None
            out[key] = foldcomp.fape_atoms(dict(pos=leaf, mask=mask), true, clamp=args.clamp, scale=args.scale, eps=args.eps, codec=codec, **kw)["loss"]
            out[key].backward()
        return call

    def backbone_surface():
        leaf.grad = None
        out["fape"] = foldcomp.fape(dict(pos=leaf, mask=mask), true, clamp=args.clamp, scale=args.scale, eps=args.eps, codec=codec)["loss"]
        out["fape"].backward()

    wall = timed(backbone_surface, sync, args.warmup, args.reps)
    doc["fape"] = entry(wall, n, loss=float(out["fape"].detach()), peak_bytes=peak_of(backbone_surface, no_grad_yet), terms=float(n) * L * L)
    for key, kw in (("fape_atoms_no_rename", dict(rename=None)), ("fape_atoms", {})):
        call = surface(key, **kw)
        wall = timed(call, sync, args.warmup, args.reps)
        doc[key] = entry(wall, n, loss=float(out[key].detach()), peak_bytes=peak_of(call, no_grad_yet), pos_grad_bytes=int(leaf.numel() * 4),
                         input_bytes=int(2 * pos.numel() * 4 + mask.numel() + aatype.numel()))
        doc[key]["peak_bytes_per_chain"] = doc[key]["peak_bytes"] / n
    doc["fape_atoms_over_fape_ms"] = doc["fape_atoms"]["median_ms"] / doc["fape"]["median_ms"]
    doc["terms_over_backbone_terms"] = terms / (float(n) * L * L)
    surface_grad = leaf.grad.clone()
    print(json.dumps({k: doc[k] for k in ("fape", "fape_atoms_no_rename", "fape_atoms")}), flush=True)

    # ---- the dense torch formulation with autograd, on the renamed truth ---------------------------------------------------------------
    from foldcomp_amd.api import frame_ambiguous, lddt_swaps
    table = torch.from_numpy(lddt_swaps("atom14").astype(np.int64)).to(dev)
    amb = torch.as_tensor(frame_ambiguous(), device=dev)                      # bool [21, 8]
    sw = swapped.bool()
    sel = torch.where(sw[..., None], table[aatype.long()], torch.arange(A, device=dev))
    pos_r = torch.gather(pos, 2, sel[..., None].expand(n, L, A, 3))
    mask_r = torch.gather(mask, 2, sel)
    turn = sw[..., None] & amb[aatype.long().clamp(max=20)]
    rot_r = torch.where(turn[..., None, None], ft["rot"] * torch.tensor([1.0, -1.0, -1.0], device=dev), ft["rot"])
    c = max(1, min(n, int(args.dense_bytes // (4 * 3 * DENSE_LIVE * (G * L) * (A * L)))))
    dense = {}
    while True:
        cp = pred[:c].clone().requires_grad_()

        def no_dense_grad_yet():
            cp.grad = None

        def dense_call():
            cp.grad = None
            rot, trans, fm = tensors.rigid_frames_torch(cp, mask[:c], aatype[:c])
            dense["loss"] = dense_loss((rot.reshape(c, G * L, 3, 3), trans.reshape(c, G * L, 3)), (rot_r[:c].reshape(c, G * L, 3, 3), ft["trans"][:c].reshape(c, G * L, 3)),
                                       (fm & ft["frame_mask"][:c]).reshape(c, G * L), pos_r[:c].reshape(c, A * L, 3), cp.reshape(c, A * L, 3),
                                       mask_r[:c].reshape(c, A * L), args.clamp, args.scale, args.eps)
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
    doc["fape_atoms_over_torch_dense_chains_per_s"] = doc["fape_atoms"]["chains_per_s"] / doc["torch_dense"]["chains_per_s"]
    print(json.dumps(doc["torch_dense"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
