#!/usr/bin/env python3
"""Time of the superposition kernels (fcz_superpose_dev / fcz_superpose_packed_dev and the apply calls)
beside the torch formulation on the same tensors, in one process -> one JSON document.

  padded   65 536 synthetic 350-residue chains as atom37 tensors (a CA random walk of 3.8 A steps), superposed on CA;
  packed   the same number of chains with the mixed benchmark's lengths (synthetic.mixed_lengths: log-normal, 16 .. 2 700), packed.

`pred` is a random rigid motion of `true`, one per chain, plus seeded Gaussian noise (sigma 0.5 A). The baseline is the usual torch
formulation in float32 on the CA slices: masked means, a batched [n, 3, L] @ [n, L, 3] product, torch.linalg.svd on [n, 3, 3] with
the determinant fix-up, and a second pass over the coordinates for the deviations, the RMSD, the five GDT counts and the TM sum;
for the packed batch it includes padding the packed rows to [n, max_seqlen, 3], which it needs. Both sides: --warmup calls, then
--reps calls, each timed by the host clock around the call and a device synchronise; the kernels' HIP-event time (group
"superpose") is reported beside it. The apply call moves the whole atom37 prediction; its rate (bytes read + written over the
kernel time) is given as a fraction of fcz_selftest_copy's read + write rate measured in the same process. Median, fastest and
slowest are given. A run without a GPU fails.

    python tools/superpose_rate.py --out profiles/superpose.json
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

import numpy as np
import torch

from knn_rate import stats, timed, walk

GDT = (0.5, 1.0, 2.0, 4.0, 8.0)


def baseline(t, p, valid):
    """t, p [n, L, 3] float32, valid [n, L] bool or None -> (rot, trans, rmsd, dev, gdt counts, tm)"""
    n, L = t.shape[:2]
    w = torch.ones((n, L, 1), dtype=torch.float32, device=t.device) if valid is None else valid.unsqueeze(-1).to(torch.float32)
    S = w.sum(dim=1).clamp(min=1.0)
    ca, cb = (p * w).sum(dim=1) / S, (t * w).sum(dim=1) / S
    a, b = (p - ca[:, None]) * w, (t - cb[:, None]) * w
    h = torch.bmm(a.transpose(1, 2), b)
    u, _, vt = torch.linalg.svd(h)
    d = torch.sign(torch.linalg.det(torch.bmm(vt.transpose(1, 2), u.transpose(1, 2))))
    fix = torch.ones((n, 3), dtype=torch.float32, device=t.device)
    fix[:, 2] = torch.where(d == 0, torch.ones_like(d), d)
    rot = torch.bmm(vt.transpose(1, 2) * fix[:, None, :], u.transpose(1, 2))
    trans = cb - torch.bmm(rot, ca[:, :, None])[:, :, 0]
    dev = (torch.bmm(p, rot.transpose(1, 2)) + trans[:, None] - t).norm(dim=-1) * w[:, :, 0]
    rmsd = ((dev * dev).sum(dim=1) / S[:, 0]).sqrt()
    counts = torch.stack([((dev <= th) & (w[:, :, 0] > 0)).sum(dim=1) for th in GDT], dim=1)
    d0 = torch.where(S[:, 0] > 15, (1.24 * (S[:, 0] - 15).clamp(min=0).pow(1.0 / 3.0) - 1.8).clamp(min=0.5), torch.full_like(S[:, 0], 0.5))
    tm = ((1.0 / (1.0 + (dev / d0[:, None]) ** 2)) * w[:, :, 0]).sum(dim=1) / S[:, 0]
    return rot, trans, rmsd, dev, counts, tm


def rigid(n, dev, gen):
    """n random proper rotations [n, 3, 3] (from unit quaternions) and translations [n, 3]"""
    q = torch.randn((n, 4), device=dev, generator=gen)
    w, x, y, z = (q / q.norm(dim=1, keepdim=True)).unbind(dim=1)
    rot = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                       2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).view(n, 3, 3)
    return rot, 30.0 * torch.randn((n, 3), device=dev, generator=gen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--residues", type=int, default=350)
    ap.add_argument("--noise", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "superpose.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("superpose_rate: no HIP device; a time is measured on the GPU or not at all")
    from foldcomp_amd import _lib, api, synthetic
    from foldcomp_amd.structure import CSuperposeOut
    dev = torch.device("cuda:0")
    torch.cuda.init()
    codec = api.default_codec()
    codec.enable_timing(True)
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    n, L, A = args.chains, args.residues, 37
    gbs = ctypes.c_double(0.0)
    _lib.check(codec.lib.fcz_selftest_copy(codec.ctx, ctypes.c_uint64(1 << 30), 10, ctypes.byref(gbs)), "fcz_selftest_copy")
    doc = {"slot": "CA", "layout": "atom37", "chains": n, "noise_sigma": args.noise, "device": torch.cuda.get_device_name(0),
           "copy_read_plus_write_gb_per_s": gbs.value,
           "method": f"host clock around call + synchronise, {args.warmup} warm-up and {args.reps} timed calls; *_kernel: HIP events, group 'superpose'; "
                     "apply fraction_of_copy = (bytes read + written by the apply call / its kernel median) / fcz_selftest_copy's read + write rate"}

    def sync():
        torch.cuda.synchronize(); codec.synchronize()

    def times(call):
        ev = []

        def once():
            codec.reset_timing(); call(); codec.synchronize(); ev.append(codec.kernel_time("superpose")[0])
        wall = timed(once, sync, args.warmup, args.reps)
        return wall, ev[args.warmup:]

    def outputs(rows_shape):
        o = dict(rot=torch.empty((n, 3, 3), dtype=torch.float32, device=dev), trans=torch.empty((n, 3), dtype=torch.float32, device=dev),
                 rmsd=torch.empty((n,), dtype=torch.float32, device=dev), sites=torch.empty((n,), dtype=torch.int32, device=dev),
                 gdt_counts=torch.empty((n, 5), dtype=torch.int32, device=dev), tm=torch.empty((n,), dtype=torch.float32, device=dev),
                 dev=torch.empty(rows_shape, dtype=torch.float32, device=dev))
        return o, CSuperposeOut(*(o[k].data_ptr() for k in ("rot", "trans", "rmsd", "sites", "gdt_counts", "tm", "dev")))

    def report(name, o, wall, ev, awall, aev, base, base_out, atoms, extra):
        apply_bytes = atoms * 24 + atoms                                     # 12 B in, 12 B out and the mask byte per atom slot
        rate = apply_bytes / (statistics.median(aev) * 1e-3) / 1e9
        doc[name] = dict(extra, superpose=stats(wall), superpose_kernel=stats(ev), apply=stats(awall), apply_kernel=stats(aev),
                         apply_gb_per_s=rate, apply_fraction_of_copy=rate / gbs.value, torch_svd_formulation=stats(base),
                         mean_rmsd=float(o["rmsd"].mean()), mean_tm=float(o["tm"].mean()),
                         max_abs_rmsd_difference_to_torch=float((base_out[2] - o["rmsd"]).abs().max()),
                         torch_over_superpose=statistics.median(base) / statistics.median(wall))
        print(json.dumps(doc[name]), flush=True)

    # ---- padded ------------------------------------------------------------------------------------------------------------------
    pos = torch.zeros((n, L, A, 3), dtype=torch.float32, device=dev)
    mask = torch.zeros((n, L, A), dtype=torch.uint8, device=dev)
    pos[:, :, 1] = walk(n * L, dev, gen).view(n, L, 3).cumsum(dim=1)
    mask[:, :, 1] = 1
    rot, trans = rigid(n, dev, gen)
    pred = torch.zeros_like(pos)
    pred[:, :, 1] = torch.bmm(pos[:, :, 1], rot.transpose(1, 2)) + trans[:, None] + args.noise * torch.randn((n, L, 3), device=dev, generator=gen)
    o, s = outputs((n, L))
    aligned = torch.empty_like(pred)
    sync()
    wall, ev = times(lambda: _lib.check(codec.lib.fcz_superpose_dev(codec.ctx, pos.data_ptr(), mask.data_ptr(), pred.data_ptr(), None, None, n, L, 0, 1,
                                                                     ctypes.byref(s)), "fcz_superpose_dev"))
    awall, aev = times(lambda: _lib.check(codec.lib.fcz_superpose_apply_dev(codec.ctx, pred.data_ptr(), mask.data_ptr(), None, n, L, 0, o["rot"].data_ptr(),
                                                                             o["trans"].data_ptr(), aligned.data_ptr()), "fcz_superpose_apply_dev"))
    ca, cap = pos[:, :, 1].contiguous(), pred[:, :, 1].contiguous()         # the slices are made once, outside the timed calls
    base = timed(lambda: baseline(ca, cap, None), sync, args.warmup, args.reps)
    report("padded", o, wall, ev, awall, aev, base, baseline(ca, cap, None), n * L * A, {"residues_per_chain": L, "rows": n * L})
    del pos, mask, pred, aligned, ca, cap, o, s
    torch.cuda.empty_cache()

    # ---- packed ------------------------------------------------------------------------------------------------------------------
    lens = synthetic.mixed_lengths(n, seed=7)
    cu = np.concatenate([[0], np.cumsum(lens)])
    R, Lmax = int(cu[-1]), int(lens.max())
    cu_t = torch.from_numpy(cu.astype(np.int32)).to(dev)
    chain = torch.repeat_interleave(torch.arange(n, device=dev), torch.from_numpy(lens).to(dev))
    within = torch.arange(R, device=dev) - cu_t[:-1].to(torch.int64)[chain]
    steps = walk(R, dev, gen).cumsum(dim=0)
    ca = steps - steps[cu_t[:-1].to(torch.int64)][chain]                     # every chain restarts at the origin
    pos = torch.zeros((R, A, 3), dtype=torch.float32, device=dev); pos[:, 1] = ca
    pred = torch.zeros_like(pos)
    pred[:, 1] = torch.bmm(ca[:, None], rot[chain].transpose(1, 2))[:, 0] + trans[chain] + args.noise * torch.randn((R, 3), device=dev, generator=gen)
    mask = torch.zeros((R, A), dtype=torch.uint8, device=dev); mask[:, 1] = 1
    o, s = outputs((R,))
    aligned = torch.empty_like(pred)
    del steps, ca
    sync()
    wall, ev = times(lambda: _lib.check(codec.lib.fcz_superpose_packed_dev(codec.ctx, pos.data_ptr(), mask.data_ptr(), pred.data_ptr(), None, cu_t.data_ptr(), n, R,
                                                                            0, 1, ctypes.byref(s)), "fcz_superpose_packed_dev"))
    awall, aev = times(lambda: _lib.check(codec.lib.fcz_superpose_apply_packed_dev(codec.ctx, pred.data_ptr(), mask.data_ptr(), cu_t.data_ptr(), n, R, 0,
                                                                                    o["rot"].data_ptr(), o["trans"].data_ptr(), aligned.data_ptr()),
                                               "fcz_superpose_apply_packed_dev"))
    pad_t = torch.empty((n, Lmax, 3), dtype=torch.float32, device=dev)       # allocated once; the padding itself is timed
    pad_p = torch.empty((n, Lmax, 3), dtype=torch.float32, device=dev)
    valid = torch.empty((n, Lmax), dtype=torch.bool, device=dev)

    def base_packed():
        pad_t.zero_(); pad_p.zero_(); valid.zero_()
        pad_t[chain, within] = pos[:, 1]; pad_p[chain, within] = pred[:, 1]; valid[chain, within] = True
        return baseline(pad_t, pad_p, valid)

    base = timed(base_packed, sync, args.warmup, args.reps)
    report("packed", o, wall, ev, awall, aev, base, base_packed(), R * A, {"rows": R, "max_seqlen": Lmax, "mean_seqlen": R / n})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
