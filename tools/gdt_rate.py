#!/usr/bin/env python3
"""Time of the maximised GDT (fcz_gdt_dev / fcz_gdt_packed_dev) on the two hinged batches of
tools/tmscore_rate.py, beside the fcz_tmscore_dev call on the same tensors in the same process -> one JSON document.

  padded   synthetic 350-residue chains as atom37 tensors (a CA random walk of 3.8 A steps), scored on CA;
  packed   the same number of chains with the mixed benchmark's lengths (synthetic.mixed_lengths: log-normal, 16 .. 2 700), packed.

`pred` is tmscore_rate's: a random rigid motion of `true` per chain plus seeded Gaussian noise, the last 3/8 of every chain swung by
60 degrees about its first residue. Reported for runs = all six and for the TM run alone: chains per second from the host clock
around the call and a device synchronise (--warmup calls, then --reps), the kernels' HIP-event time (group "gdt"), the ratio to the
fcz_tmscore_dev call (group "tmscore") timed the same way, and the mean GDT-TS / GDT-HA beside those at the Kabsch fit
(fcz_superpose_dev) and at the TM-maximising fit. There is no threshold: nothing computed this before. A run without a GPU fails.

    python tools/gdt_rate.py --out profiles/gdt.json
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
from superpose_rate import rigid
from tmscore_rate import hinge_rotation

RUNS = (("all", 63), ("tm", 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=16384)
    ap.add_argument("--residues", type=int, default=350)
    ap.add_argument("--noise", type=float, default=0.5)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gdt.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gdt_rate: no HIP device; a time is measured on the GPU or not at all")
    from foldcomp_amd import _lib, api, synthetic
    from foldcomp_amd.structure import CGdtOut, CSuperposeOut, CTmScoreOut
    dev = torch.device("cuda:0")
    torch.cuda.init()
    codec = api.default_codec()
    codec.enable_timing(True)
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    n, L, A = args.chains, args.residues, 37
    lib = codec.lib
    doc = {"slot": "CA", "layout": "atom37", "chains": n, "noise_sigma": args.noise, "hinged": True, "iterations": args.iterations,
           "device": torch.cuda.get_device_name(0),
           "method": f"host clock around call + synchronise, {args.warmup} warm-up and {args.reps} timed calls; *_kernel: HIP events, groups 'gdt' / 'tmscore'"}

    def sync():
        torch.cuda.synchronize(); codec.synchronize()

    def times(call, group):
        ev = []

        def once():
            codec.reset_timing(); call(); codec.synchronize(); ev.append(codec.kernel_time(group)[0])
        wall = timed(once, sync, args.warmup, args.reps)
        return wall, ev[args.warmup:]

    def gdt_ts_ha(counts, sites):
        c, s = counts.to(torch.float64), sites.to(torch.float64).clamp(min=1.0)[:, None]
        return float((c[:, 1:5] / s).mean()), float((c[:, 0:4] / s).mean())

    def measure(name, packed, pos, mask, pred, bound, rows, extra):
        """superpose, tmscore and the two gdt calls on one batch"""
        suffix = "_packed_dev" if packed else "_dev"
        rows_shape = (rows,) if packed else (n, rows)
        f32, i32 = (lambda *s: torch.empty(s, dtype=torch.float32, device=dev)), (lambda *s: torch.empty(s, dtype=torch.int32, device=dev))
        o = dict(rot=f32(n, 3, 3), trans=f32(n, 3), rmsd=f32(n), sites=i32(n), gdt_counts=i32(n, 5), tm=f32(n), dev=f32(*rows_shape), seed=i32(n), selected=i32(n))
        keys = ("rot", "trans", "rmsd", "sites", "gdt_counts", "tm", "dev")
        ks, ts = CSuperposeOut(*(o[k].data_ptr() for k in keys)), CTmScoreOut(*(o[k].data_ptr() for k in keys + ("seed", "selected")))
        q = dict(gdt_counts=i32(n, 5), sites=i32(n), rot=f32(n, 5, 3, 3), trans=f32(n, 5, 3), seed=i32(n, 5), run=i32(n, 5), selected=i32(n, 5),
                 within=torch.empty(rows_shape, dtype=torch.uint8, device=dev))
        gs = CGdtOut(*(q[k].data_ptr() for k in ("gdt_counts", "sites", "rot", "trans", "seed", "run", "selected", "within")))
        head = (codec.ctx, pos.data_ptr(), mask.data_ptr(), pred.data_ptr(), None, bound, n, rows, 0, 1)
        sync()
        _lib.check(getattr(lib, "fcz_superpose" + suffix)(*head, ctypes.byref(ks)), "fcz_superpose" + suffix)
        sync()
        kab = gdt_ts_ha(o["gdt_counts"], o["sites"])
        twall, tev = times(lambda: _lib.check(getattr(lib, "fcz_tmscore" + suffix)(*head, 0, args.iterations, ctypes.byref(ts)), "fcz_tmscore" + suffix), "tmscore")
        at_tm = gdt_ts_ha(o["gdt_counts"], o["sites"])
        tm_counts = o["gdt_counts"].clone()
        tmed = statistics.median(twall)
        d = dict(extra, tmscore=stats(twall), tmscore_kernel=stats(tev), mean_gdt_ts_at_the_kabsch_fit=kab[0], mean_gdt_ha_at_the_kabsch_fit=kab[1],
                 mean_gdt_ts_at_the_tm_fit=at_tm[0], mean_gdt_ha_at_the_tm_fit=at_tm[1])
        for label, runs in RUNS:
            wall, ev = times(lambda: _lib.check(getattr(lib, "fcz_gdt" + suffix)(*head, 0, args.iterations, runs, ctypes.byref(gs)), "fcz_gdt" + suffix), "gdt")
            med = statistics.median(wall)
            best = gdt_ts_ha(q["gdt_counts"], q["sites"])
            d["runs_" + label] = dict(gdt=stats(wall), gdt_kernel=stats(ev), chains_per_s=n / (med * 1e-3), gdt_over_tmscore=med / tmed, mean_gdt_ts=best[0],
                                      mean_gdt_ha=best[1], never_below_the_tm_fit=bool((q["gdt_counts"] >= tm_counts).all()),
                                      share_of_winners_by_run=[float((q["run"] == r).to(torch.float32).mean()) for r in range(6)])
        doc[name] = d
        print(json.dumps(d), flush=True)

    # ---- padded ------------------------------------------------------------------------------------------------------------------
    pos = torch.zeros((n, L, A, 3), dtype=torch.float32, device=dev)
    mask = torch.zeros((n, L, A), dtype=torch.uint8, device=dev)
    ca = walk(n * L, dev, gen).view(n, L, 3).cumsum(dim=1)
    pos[:, :, 1] = ca
    mask[:, :, 1] = 1
    rot, trans = rigid(n, dev, gen)
    moved = ca.clone()
    at = L - (3 * L) // 8
    moved[:, at:] = (ca[:, at:] - ca[:, at:at + 1]) @ hinge_rotation(dev).T + ca[:, at:at + 1]
    pred = torch.zeros_like(pos)
    pred[:, :, 1] = torch.bmm(moved, rot.transpose(1, 2)) + trans[:, None] + args.noise * torch.randn((n, L, 3), device=dev, generator=gen)
    del ca, moved
    measure("padded", False, pos, mask, pred, None, L, {"residues_per_chain": L, "rows": n * L, "seeds": n * int(lib.fcz_tmscore_seeds(L, 0))})
    del pos, mask, pred
    torch.cuda.empty_cache()

    # ---- packed ------------------------------------------------------------------------------------------------------------------
    lens = synthetic.mixed_lengths(n, seed=7)
    cu = np.concatenate([[0], np.cumsum(lens)])
    R, Lmax = int(cu[-1]), int(lens.max())
    cu_t = torch.from_numpy(cu.astype(np.int32)).to(dev)
    lens_t = torch.from_numpy(lens).to(dev)
    chain = torch.repeat_interleave(torch.arange(n, device=dev), lens_t)
    first = cu_t[:-1].to(torch.int64)
    row_in_chain = torch.arange(R, device=dev) - first[chain]
    steps = walk(R, dev, gen).cumsum(dim=0)
    ca = steps - steps[first][chain]                                         # every chain restarts at the origin
    at = lens_t.to(torch.int64) - (3 * lens_t.to(torch.int64)) // 8          # the first residue of every chain's swung part
    pivot = ca[first + at][chain]
    moved = torch.where((row_in_chain >= at[chain])[:, None], (ca - pivot) @ hinge_rotation(dev).T + pivot, ca)
    pos = torch.zeros((R, A, 3), dtype=torch.float32, device=dev); pos[:, 1] = ca
    pred = torch.zeros_like(pos)
    pred[:, 1] = (rot[chain] * moved[:, None, :]).sum(dim=2) + trans[chain] + args.noise * torch.randn((R, 3), device=dev, generator=gen)
    mask = torch.zeros((R, A), dtype=torch.uint8, device=dev); mask[:, 1] = 1
    del steps, ca, moved
    seeds = sum(int(c) * int(lib.fcz_tmscore_seeds(int(m), 0)) for m, c in zip(*np.unique(lens, return_counts=True)))
    measure("packed", True, pos, mask, pred, cu_t.data_ptr(), R, {"rows": R, "max_seqlen": Lmax, "mean_seqlen": R / n, "seeds": seeds})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
