#!/usr/bin/env python3
"""Time of the k-nearest-neighbour kernel (fcz_knn_dev / fcz_knn_packed_dev) beside the torch formulation on
the same tensors, in one process -> one JSON document.

  padded   65 536 synthetic 350-residue chains as atom37 tensors (a CA random walk of 3.8 A steps), k = 48 on CA;
  packed   the same number of chains with the mixed benchmark's lengths (synthetic.mixed_lengths: log-normal, 16 .. 2 700), packed.

The baseline is torch.cdist on the CA slice plus topk(k + 1, largest=False) over chunks of chains whose [c, L, L] matrix fits
--chunk-bytes; for the packed batch it includes padding the packed rows to [n, max_seqlen, 3] (chains sorted by length into chunks
padded to the chunk's longest chain, sized by --chunk-bytes too, are kinder to it and are reported as well; the better of the two
is what the kernel is compared with). Both sides: --warmup calls, then --reps calls, each
timed by the host clock around the call and a device synchronise; the kernel's HIP-event time (group "knn") is reported beside it.
Median, fastest and slowest are given. A run without a GPU fails.

    python tools/knn_rate.py --out profiles/knn.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch


def walk(rows, dev, gen):
    """CA trace: unit steps of 3.8 A in random directions, summed per call (the caller restarts it per chain)"""
    v = torch.randn((rows, 3), device=dev, generator=gen)
    return 3.8 * v / v.norm(dim=1, keepdim=True)


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "calls": len(ms)}


def timed(fn, sync, warmup, reps):
    for _ in range(warmup):
        fn(); sync()
    out = []
    for _ in range(reps):
        sync()
        t = time.perf_counter()
        fn(); sync()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def baseline_padded(ca, k, chunk):
    """ca [n, L, 3] -> (dist, index) of the last chunk (the result is dropped chunk by chunk, as a loader would consume it)"""
    last = None
    for c0 in range(0, ca.shape[0], chunk):
        x = ca[c0:c0 + chunk]
        last = torch.cdist(x, x).topk(min(k + 1, x.shape[1]), dim=-1, largest=False)
    return last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--residues", type=int, default=350)
    ap.add_argument("--k", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk-bytes", type=float, default=4e9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("knn_rate: no HIP device; a time is measured on the GPU or not at all")
    from foldcomp_amd import _lib, api, synthetic
    dev = torch.device("cuda:0")
    torch.cuda.init()
    codec = api.default_codec()
    codec.enable_timing(True)
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    n, L, k, A = args.chains, args.residues, args.k, 37
    doc = {"k": k, "slot": "CA", "layout": "atom37", "chains": n, "device": torch.cuda.get_device_name(0),
           "method": f"host clock around call + synchronise, {args.warmup} warm-up and {args.reps} timed calls; knn_kernel: HIP events, group 'knn'"}

    def sync():
        torch.cuda.synchronize(); codec.synchronize()

    def knn_times(call):
        ev = []

        def once():
            codec.reset_timing(); call(); codec.synchronize(); ev.append(codec.kernel_time("knn")[0])
        wall = timed(once, sync, args.warmup, args.reps)
        return wall, ev[args.warmup:]

    # ---- padded ------------------------------------------------------------------------------------------------------------------
    pos = torch.zeros((n, L, A, 3), dtype=torch.float32, device=dev)
    mask = torch.zeros((n, L, A), dtype=torch.uint8, device=dev)
    pos[:, :, 1] = walk(n * L, dev, gen).view(n, L, 3).cumsum(dim=1)
    mask[:, :, 1] = 1
    index = torch.empty((n, L, k), dtype=torch.int32, device=dev); dist = torch.empty((n, L, k), dtype=torch.float32, device=dev)
    sync()
    wall, ev = knn_times(lambda: _lib.check(codec.lib.fcz_knn_dev(codec.ctx, pos.data_ptr(), mask.data_ptr(), None, n, L, 0, 1, k, index.data_ptr(),
                                                                  dist.data_ptr()), "fcz_knn_dev"))
    chunk = max(1, int(args.chunk_bytes // (4 * L * L)))
    ca = pos[:, :, 1].contiguous()                                           # the slice is made once, outside the timed calls
    base = timed(lambda: baseline_padded(ca, k, chunk), sync, args.warmup, args.reps)
    # the two agree where the baseline's distances are not tied (a sanity check of the workload, not of the bits)
    bd, bi = baseline_padded(ca[-chunk:], k, chunk)
    agree = float((bi[:, :, 1:].to(torch.int32) == index[-chunk:]).float().mean())
    doc["padded"] = {"residues_per_chain": L, "rows": n * L, "knn": stats(wall), "knn_kernel": stats(ev), "torch_cdist_topk": stats(base),
                     "chunk_chains": chunk, "index_agreement_with_torch": agree,
                     "torch_over_knn": statistics.median(base) / statistics.median(wall)}
    print(json.dumps(doc["padded"]), flush=True)
    del pos, mask, index, dist, bd, bi, ca
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
    mask = torch.zeros((R, A), dtype=torch.uint8, device=dev); mask[:, 1] = 1
    index = torch.empty((R, k), dtype=torch.int32, device=dev); dist = torch.empty((R, k), dtype=torch.float32, device=dev)
    del steps
    sync()
    wall, ev = knn_times(lambda: _lib.check(codec.lib.fcz_knn_packed_dev(codec.ctx, pos.data_ptr(), mask.data_ptr(), cu_t.data_ptr(), n, R, 0, 1, k,
                                                                         index.data_ptr(), dist.data_ptr()), "fcz_knn_packed_dev"))

    pad = torch.empty((n, Lmax, 3), dtype=torch.float32, device=dev)         # allocated once; the padding itself is timed

    def base_packed():
        pad.zero_()
        pad[chain, within] = pos[:, 1]
        return baseline_padded(pad, k, max(1, int(args.chunk_bytes // (4 * Lmax * Lmax))))

    order = torch.from_numpy(np.argsort(lens, kind="stable")).to(dev)
    sorted_lens = np.sort(lens, kind="stable")
    cuts, c0 = [], 0                                                          # chunks of sorted chains whose [c, Lc, Lc] fits --chunk-bytes
    while c0 < n:
        c = 1
        while c0 + c < n and 4.0 * (c + 1) * float(sorted_lens[c0 + c]) ** 2 <= args.chunk_bytes and c < 8192:
            c += 1
        cuts.append((c0, c0 + c, int(sorted_lens[c0 + c - 1])))
        c0 += c

    def base_packed_sorted():
        """kinder to torch: chains sorted by length, every chunk padded to its own longest chain"""
        pad.zero_()
        pad[chain, within] = pos[:, 1]
        srt = pad[order]
        last = None
        for a, b, Lc in cuts:
            x = srt[a:b, :Lc]
            last = torch.cdist(x, x).topk(min(k + 1, Lc), dim=-1, largest=False)
        return last

    base = timed(base_packed, sync, args.warmup, args.reps)
    base_sorted = timed(base_packed_sorted, sync, args.warmup, args.reps)
    best = min(statistics.median(base), statistics.median(base_sorted))
    doc["packed"] = {"rows": R, "max_seqlen": Lmax, "mean_seqlen": R / n, "knn": stats(wall), "knn_kernel": stats(ev),
                     "torch_pad_cdist_topk": stats(base), "torch_pad_sorted_chunks_cdist_topk": stats(base_sorted),
                     "torch_over_knn": best / statistics.median(wall)}
    print(json.dumps(doc["packed"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
