#!/usr/bin/env python3
"""Time of the maximised TM-score (fcz_tmscore_dev / fcz_tmscore_packed_dev) on the two batches of
tools/superpose_rate.py, beside the fcz_superpose_dev call on the same tensors in the same process -> one JSON document.

  padded   65 536 synthetic 350-residue chains as atom37 tensors (a CA random walk of 3.8 A steps), scored on CA;
  packed   the same number of chains with the mixed benchmark's lengths (synthetic.mixed_lengths: log-normal, 16 .. 2 700), packed.

`pred` is a random rigid motion of `true`, one per chain, plus seeded Gaussian noise (sigma 0.5 A); with --hinge (the default) the last
3/8 of every chain's prediction is swung by 60 degrees about its first residue, the case the search is for. Reported: chains per
second from the host clock around the call and a device synchronise (--warmup calls, then --reps), the kernels' HIP-event time
(group "tmscore"), the seeds the batch has (fcz_tmscore_seeds of every length), and the ratio to the superpose call (group
"superpose") timed the same way. There is no threshold: the search does the work of some hundreds of superpositions per chain.
A run without a GPU fails.

    python tools/tmscore_rate.py --out profiles/tmscore.json
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

from knn_rate import stats, timed, walk
from superpose_rate import rigid


def hinge_rotation(dev):
    c, s = math.cos(math.pi / 3), math.sin(math.pi / 3)
    return torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32, device=dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--residues", type=int, default=350)
    ap.add_argument("--noise", type=float, default=0.5)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--no-hinge", dest="hinge", action="store_false")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tmscore.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tmscore_rate: no HIP device; a time is measured on the GPU or not at all")
    from foldcomp_amd import _lib, api, synthetic
    from foldcomp_amd.structure import CSuperposeOut, CTmScoreOut
    dev = torch.device("cuda:0")
    torch.cuda.init()
    codec = api.default_codec()
    codec.enable_timing(True)
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    n, L, A = args.chains, args.residues, 37
    lib = codec.lib
    doc = {"slot": "CA", "layout": "atom37", "chains": n, "noise_sigma": args.noise, "hinged": args.hinge, "iterations": args.iterations,
           "device": torch.cuda.get_device_name(0),
           "method": f"host clock around call + synchronise, {args.warmup} warm-up and {args.reps} timed calls; *_kernel: HIP events, groups 'tmscore' / 'superpose'"}

    def sync():
        torch.cuda.synchronize(); codec.synchronize()

    def times(call, group):
        ev = []

        def once():
            codec.reset_timing(); call(); codec.synchronize(); ev.append(codec.kernel_time(group)[0])
        wall = timed(once, sync, args.warmup, args.reps)
        return wall, ev[args.warmup:]

    def outputs(rows_shape):
        o = dict(rot=torch.empty((n, 3, 3), dtype=torch.float32, device=dev), trans=torch.empty((n, 3), dtype=torch.float32, device=dev),
                 rmsd=torch.empty((n,), dtype=torch.float32, device=dev), sites=torch.empty((n,), dtype=torch.int32, device=dev),
                 gdt_counts=torch.empty((n, 5), dtype=torch.int32, device=dev), tm=torch.empty((n,), dtype=torch.float32, device=dev),
                 dev=torch.empty(rows_shape, dtype=torch.float32, device=dev), seed=torch.empty((n,), dtype=torch.int32, device=dev),
                 selected=torch.empty((n,), dtype=torch.int32, device=dev))
        keys = ("rot", "trans", "rmsd", "sites", "gdt_counts", "tm", "dev")
        return o, CTmScoreOut(*(o[k].data_ptr() for k in keys + ("seed", "selected"))), CSuperposeOut(*(o[k].data_ptr() for k in keys))

    def report(name, o, wall, ev, kwall, kev, kab_tm, seeds, extra):
        med = statistics.median(wall)
        doc[name] = dict(extra, seeds=seeds, tmscore=stats(wall), tmscore_kernel=stats(ev), chains_per_s=n / (med * 1e-3), seeds_per_s=seeds / (med * 1e-3),
                         superpose=stats(kwall), superpose_kernel=stats(kev), tmscore_over_superpose=med / statistics.median(kwall),
                         mean_tm=float(o["tm"].mean()), mean_tm_at_the_kabsch_fit=float(kab_tm.mean()),
                         chains_gaining_0_05=float((o["tm"] - kab_tm >= 0.05).to(torch.float32).mean()), chains_won_by_seed_0=float((o["seed"] == 0).to(torch.float32).mean()),
                         mean_selected_fraction=float((o["selected"].to(torch.float32) / o["sites"].clamp(min=1).to(torch.float32)).mean()))
        print(json.dumps(doc[name]), flush=True)

    # ---- padded ------------------------------------------------------------------------------------------------------------------
    pos = torch.zeros((n, L, A, 3), dtype=torch.float32, device=dev)
    mask = torch.zeros((n, L, A), dtype=torch.uint8, device=dev)
    ca = walk(n * L, dev, gen).view(n, L, 3).cumsum(dim=1)
    pos[:, :, 1] = ca
    mask[:, :, 1] = 1
    rot, trans = rigid(n, dev, gen)
    moved = ca.clone()
    if args.hinge:
        at = L - (3 * L) // 8
        moved[:, at:] = (ca[:, at:] - ca[:, at:at + 1]) @ hinge_rotation(dev).T + ca[:, at:at + 1]
    pred = torch.zeros_like(pos)
    pred[:, :, 1] = torch.bmm(moved, rot.transpose(1, 2)) + trans[:, None] + args.noise * torch.randn((n, L, 3), device=dev, generator=gen)
    del ca, moved
    o, s, ks = outputs((n, L))
    sync()
    kwall, kev = times(lambda: _lib.check(lib.fcz_superpose_dev(codec.ctx, pos.data_ptr(), mask.data_ptr(), pred.data_ptr(), None, None, n, L, 0, 1, ctypes.byref(ks)),
                                          "fcz_superpose_dev"), "superpose")
    kab_tm = o["tm"].clone()
    wall, ev = times(lambda: _lib.check(lib.fcz_tmscore_dev(codec.ctx, pos.data_ptr(), mask.data_ptr(), pred.data_ptr(), None, None, n, L, 0, 1, 0, args.iterations,
                                                            ctypes.byref(s)), "fcz_tmscore_dev"), "tmscore")
    report("padded", o, wall, ev, kwall, kev, kab_tm, n * int(lib.fcz_tmscore_seeds(L, 0)), {"residues_per_chain": L, "rows": n * L})
    del pos, mask, pred, o, s, ks
    torch.cuda.empty_cache()

    # ---- packed ------------------------------------------------------------------------------------------------------------------
    lens = synthetic.mixed_lengths(n, seed=7)
    cu = np.concatenate([[0], np.cumsum(lens)])
    R, Lmax = int(cu[-1]), int(lens.max())
    cu_t = torch.from_numpy(cu.astype(np.int32)).to(dev)
    lens_t = torch.from_numpy(lens).to(dev)
    chain = torch.repeat_interleave(torch.arange(n, device=dev), lens_t)
    first = cu_t[:-1].to(torch.int64)
    within = torch.arange(R, device=dev) - first[chain]
    steps = walk(R, dev, gen).cumsum(dim=0)
    ca = steps - steps[first][chain]                                         # every chain restarts at the origin
    moved = ca
    if args.hinge:
        at = lens_t.to(torch.int64) - (3 * lens_t.to(torch.int64)) // 8      # the first residue of every chain's swung part
        pivot = ca[first + at][chain]
        moved = torch.where((within >= at[chain])[:, None], (ca - pivot) @ hinge_rotation(dev).T + pivot, ca)
    pos = torch.zeros((R, A, 3), dtype=torch.float32, device=dev); pos[:, 1] = ca
    pred = torch.zeros_like(pos)
    # (an elementwise product, not torch.bmm: a batched product of R ~ 2e7 one-row matrices is no shape for a BLAS call)
    pred[:, 1] = (rot[chain] * moved[:, None, :]).sum(dim=2) + trans[chain] + args.noise * torch.randn((R, 3), device=dev, generator=gen)
    mask = torch.zeros((R, A), dtype=torch.uint8, device=dev); mask[:, 1] = 1
    o, s, ks = outputs((R,))
    del steps, ca, moved
    sync()
    kwall, kev = times(lambda: _lib.check(lib.fcz_superpose_packed_dev(codec.ctx, pos.data_ptr(), mask.data_ptr(), pred.data_ptr(), None, cu_t.data_ptr(), n, R, 0, 1,
                                                                       ctypes.byref(ks)), "fcz_superpose_packed_dev"), "superpose")
    kab_tm = o["tm"].clone()
    wall, ev = times(lambda: _lib.check(lib.fcz_tmscore_packed_dev(codec.ctx, pos.data_ptr(), mask.data_ptr(), pred.data_ptr(), None, cu_t.data_ptr(), n, R, 0, 1, 0,
                                                                   args.iterations, ctypes.byref(s)), "fcz_tmscore_packed_dev"), "tmscore")
    seeds = sum(int(c) * int(lib.fcz_tmscore_seeds(int(m), 0)) for m, c in zip(*np.unique(lens, return_counts=True)))
    report("packed", o, wall, ev, kwall, kev, kab_tm, seeds, {"rows": R, "max_seqlen": Lmax, "mean_seqlen": R / n})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
