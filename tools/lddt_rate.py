#!/usr/bin/env python3
"""Time of the lDDT kernel (fcz_lddt_dev / fcz_lddt_packed_dev) beside the torch formulation on the same
tensors, in one process -> one JSON document.

  padded   65 536 synthetic 350-residue chains as atom37 tensors (a CA random walk of 3.8 A steps), lDDT on CA, cutoff 15;
  packed   the same number of chains with the mixed benchmark's lengths (synthetic.mixed_lengths: log-normal, 16 .. 2 700), packed.

`pred` is `true` plus seeded Gaussian noise (sigma 0.5 A). The baseline is the AlphaFold formulation in torch float32: two
torch.cdist on the CA slices, the mask dmat_true < cutoff without the diagonal, four compares and the sums, over chunks of chains
whose [c, L, L] matrices fit --chunk-bytes; for the packed batch it includes padding the packed rows to [n, max_seqlen, 3] (chains
sorted by length into chunks padded to the chunk's longest chain, sized by --chunk-bytes too, are kinder to it and are reported as
well; the better of the two is what the kernel is compared with). Both sides: --warmup calls, then --reps calls, each timed by the
host clock around the call and a device synchronise; the kernel's HIP-event time (group "lddt") is reported beside it. Median,
fastest and slowest are given. A run without a GPU fails.

    python tools/lddt_rate.py --out profiles/lddt.json
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

THRESHOLDS = (0.5, 1.0, 2.0, 4.0)
LIVE = 6          # [c, L, L] float32 matrices the baseline holds at its peak (two distances, the mask, the difference, two temporaries)


def baseline_padded(t, p, valid, cutoff, chunk):
    """t, p [n, L, 3], valid [n, L] bool or None -> per-residue score of the last chunk (dropped chunk by chunk, as a validation loop
    would reduce it)"""
    last = None
    for c0 in range(0, t.shape[0], chunk):
        a, b = t[c0:c0 + chunk], p[c0:c0 + chunk]
        dt, dp = torch.cdist(a, a), torch.cdist(b, b)
        score = (dt < cutoff) & ~torch.eye(a.shape[1], dtype=torch.bool, device=a.device)
        if valid is not None:
            v = valid[c0:c0 + chunk]
            score &= v[:, :, None] & v[:, None, :]
        score = score.to(torch.float32)
        l1 = (dt - dp).abs()
        hits = sum((l1 < th).to(torch.float32) for th in THRESHOLDS) * score
        last = hits.sum(dim=-1) / (4.0 * score.sum(dim=-1)).clamp(min=1.0)
    return last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--residues", type=int, default=350)
    ap.add_argument("--cutoff", type=float, default=15.0)
    ap.add_argument("--noise", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk-bytes", type=float, default=4e9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lddt.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lddt_rate: no HIP device; a time is measured on the GPU or not at all")
    from foldcomp_amd import _lib, api, synthetic
    dev = torch.device("cuda:0")
    torch.cuda.init()
    codec = api.default_codec()
    codec.enable_timing(True)
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    n, L, A, cutoff = args.chains, args.residues, 37, args.cutoff
    th = (ctypes.c_float * 4)(*THRESHOLDS)
    doc = {"slot": "CA", "layout": "atom37", "chains": n, "cutoff": cutoff, "thresholds": list(THRESHOLDS), "noise_sigma": args.noise,
           "device": torch.cuda.get_device_name(0),
           "method": f"host clock around call + synchronise, {args.warmup} warm-up and {args.reps} timed calls; lddt_kernel: HIP events, group 'lddt'"}

    def sync():
        torch.cuda.synchronize(); codec.synchronize()

    def lddt_times(call):
        ev = []

        def once():
            codec.reset_timing(); call(); codec.synchronize(); ev.append(codec.kernel_time("lddt")[0])
        wall = timed(once, sync, args.warmup, args.reps)
        return wall, ev[args.warmup:]

    # ---- padded ------------------------------------------------------------------------------------------------------------------
    pos = torch.zeros((n, L, A, 3), dtype=torch.float32, device=dev)
    mask = torch.zeros((n, L, A), dtype=torch.uint8, device=dev)
    pos[:, :, 1] = walk(n * L, dev, gen).view(n, L, 3).cumsum(dim=1)
    mask[:, :, 1] = 1
    pred = torch.zeros_like(pos)
    pred[:, :, 1] = pos[:, :, 1] + args.noise * torch.randn((n, L, 3), device=dev, generator=gen)
    score = torch.empty((n, L), dtype=torch.float32, device=dev)
    pairs = torch.empty((n, L), dtype=torch.int32, device=dev); hits = torch.empty((n, L), dtype=torch.int32, device=dev)
    sync()
    wall, ev = lddt_times(lambda: _lib.check(codec.lib.fcz_lddt_dev(codec.ctx, pos.data_ptr(), mask.data_ptr(), pred.data_ptr(), None, None, n, L, 0, 1, cutoff,
                                                                    ctypes.addressof(th), score.data_ptr(), pairs.data_ptr(), hits.data_ptr()), "fcz_lddt_dev"))
    chunk = max(1, int(args.chunk_bytes // (4 * LIVE * L * L)))
    ca, cap = pos[:, :, 1].contiguous(), pred[:, :, 1].contiguous()         # the slices are made once, outside the timed calls
    base = timed(lambda: baseline_padded(ca, cap, None, cutoff, chunk), sync, args.warmup, args.reps)
    # the two agree up to the baseline's rounding (a sanity check of the workload, not of the bits)
    bs = baseline_padded(ca[-chunk:], cap[-chunk:], None, cutoff, chunk)
    doc["padded"] = {"residues_per_chain": L, "rows": n * L, "lddt": stats(wall), "lddt_kernel": stats(ev), "torch_cdist_formulation": stats(base),
                     "chunk_chains": chunk, "mean_lddt": float(score.mean()), "mean_pairs": float(pairs.to(torch.float32).mean()),
                     "max_abs_score_difference_to_torch": float((bs - score[-chunk:]).abs().max()),
                     "torch_over_lddt": statistics.median(base) / statistics.median(wall)}
    print(json.dumps(doc["padded"]), flush=True)
    del pos, mask, pred, score, pairs, hits, bs, ca, cap
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
    pred = torch.zeros_like(pos); pred[:, 1] = ca + args.noise * torch.randn((R, 3), device=dev, generator=gen)
    mask = torch.zeros((R, A), dtype=torch.uint8, device=dev); mask[:, 1] = 1
    score = torch.empty((R,), dtype=torch.float32, device=dev)
    pairs = torch.empty((R,), dtype=torch.int32, device=dev); hits = torch.empty((R,), dtype=torch.int32, device=dev)
    del steps, ca
    sync()
    wall, ev = lddt_times(lambda: _lib.check(codec.lib.fcz_lddt_packed_dev(codec.ctx, pos.data_ptr(), mask.data_ptr(), pred.data_ptr(), None, cu_t.data_ptr(), n, R,
                                                                           0, 1, cutoff, ctypes.addressof(th), score.data_ptr(), pairs.data_ptr(), hits.data_ptr()),
                                             "fcz_lddt_packed_dev"))

    pad_t = torch.empty((n, Lmax, 3), dtype=torch.float32, device=dev)       # allocated once; the padding itself is timed
    pad_p = torch.empty((n, Lmax, 3), dtype=torch.float32, device=dev)
    valid = torch.empty((n, Lmax), dtype=torch.bool, device=dev)

    def pad():
        pad_t.zero_(); pad_p.zero_(); valid.zero_()
        pad_t[chain, within] = pos[:, 1]; pad_p[chain, within] = pred[:, 1]; valid[chain, within] = True

    def base_packed():
        pad()
        return baseline_padded(pad_t, pad_p, valid, cutoff, max(1, int(args.chunk_bytes // (4 * LIVE * Lmax * Lmax))))

    order = torch.from_numpy(np.argsort(lens, kind="stable")).to(dev)
    sorted_lens = np.sort(lens, kind="stable")
    cuts, c0 = [], 0                                                          # chunks of sorted chains whose [c, Lc, Lc] matrices fit --chunk-bytes
    while c0 < n:
        c = 1
        while c0 + c < n and 4.0 * LIVE * (c + 1) * float(sorted_lens[c0 + c]) ** 2 <= args.chunk_bytes and c < 8192:
            c += 1
        cuts.append((c0, c0 + c, int(sorted_lens[c0 + c - 1])))
        c0 += c

    def base_packed_sorted():
        """kinder to torch: chains sorted by length, every chunk padded to its own longest chain"""
        pad()
        st, sp, sv = pad_t[order], pad_p[order], valid[order]
        last = None
        for a, b, Lc in cuts:
            last = baseline_padded(st[a:b, :Lc], sp[a:b, :Lc], sv[a:b, :Lc], cutoff, b - a)
        return last

    base = timed(base_packed, sync, args.warmup, args.reps)
    base_sorted = timed(base_packed_sorted, sync, args.warmup, args.reps)
    best = min(statistics.median(base), statistics.median(base_sorted))
    doc["packed"] = {"rows": R, "max_seqlen": Lmax, "mean_seqlen": R / n, "lddt": stats(wall), "lddt_kernel": stats(ev),
                     "torch_pad_cdist_formulation": stats(base), "torch_pad_sorted_chunks_cdist_formulation": stats(base_sorted),
                     "mean_lddt": float(score.mean()), "torch_over_lddt": best / statistics.median(wall)}
    print(json.dumps(doc["packed"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
