#!/usr/bin/env python3
"""Time of the two DSSP kernels (fcz_hbond_dev and fcz_dssp_labels_dev and their packed forms) beside a plain
torch formulation of the same hydrogen-bond map on the same tensors, in one process -> one JSON document.

  padded   synthetic 350-residue chains as backbone4 tensors: an ideal alpha helix (NeRF, phi -57, psi -47) with Gaussian jitter of
           0.1 A per coordinate and chain -- every residue donates and accepts, the densest case the energy path sees;
  packed   the same number of chains with the mixed benchmark's lengths (synthetic.mixed_lengths: log-normal, 16 .. 2 700), packed.

The baseline is the textbook dense map in torch float32 on the same device: the amide hydrogens, four torch.cdist matrices
(O-N, C-H, O-H, C-N), the energy with its clamp, the masks (self, i - 1, CA distance under 9 A) and topk(2) along both axes, over
chunks of chains whose [c, L, L] matrices fit --chunk-bytes; for the packed batch it first pads the rows to [n, max_seqlen]. It
does not label. Both sides: --warmup calls, then --reps calls, each timed by the host clock around the call and a device
synchronise; the kernels' HIP-event time (group "dssp") is reported beside it. A run without a GPU fails.

    python tools/dssp_rate.py --out profiles/dssp.json
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

from knn_rate import stats, timed

LIVE = 8          # [c, L, L] float32 matrices the baseline holds at its peak (four distances, the energy, the masks, temporaries)


def _place(a, b, c, length, angle, torsion):
    bc = (c - b) / np.linalg.norm(c - b)
    n = np.cross(b - a, bc)
    n /= np.linalg.norm(n)
    t, p = np.radians(angle), np.radians(torsion)
    return c + length * (-np.cos(t) * bc + np.sin(t) * np.cos(p) * np.cross(n, bc) + np.sin(t) * np.sin(p) * n)


def helix(m, phi=-57.0, psi=-47.0):
    """N, CA, C, O of an ideal poly-Ala alpha helix -> float32 [m, 4, 3]"""
    N, CA = [np.zeros(3)], [np.array([1.458, 0.0, 0.0])]
    C, O = [CA[0] + 1.525 * np.array([np.cos(np.radians(69.0)), np.sin(np.radians(69.0)), 0.0])], []
    for r in range(m):
        if r:
            N.append(_place(N[r - 1], CA[r - 1], C[r - 1], 1.329, 116.2, psi))
            CA.append(_place(CA[r - 1], C[r - 1], N[r], 1.458, 121.7, 180.0))
            C.append(_place(C[r - 1], N[r], CA[r], 1.525, 111.0, phi))
        O.append(_place(N[r], CA[r], C[r], 1.231, 120.5, psi + 180.0))
    return np.stack([np.asarray(x) for x in (N, CA, C, O)], axis=1).astype(np.float32)


def baseline_padded(pos, valid, chunk):
    """pos [n, L, 4, 3], valid [n, L] bool or None -> (energy, index) of the two best acceptors of the last chunk's rows (dropped chunk
    by chunk, as a loader would consume it); the donor table is the same topk along the other axis and is computed too"""
    last = None
    L = pos.shape[1]
    eye = torch.eye(L, dtype=torch.bool, device=pos.device)
    prev = torch.diag(torch.ones(L - 1, dtype=torch.bool, device=pos.device), -1)            # j == i - 1
    for c0 in range(0, pos.shape[0], chunk):
        p = pos[c0:c0 + chunk]
        N, CA, C, O = p[:, :, 0], p[:, :, 1], p[:, :, 2], p[:, :, 3]
        co = C[:, :-1] - O[:, :-1]
        H = N.clone()
        H[:, 1:] += co / co.norm(dim=-1, keepdim=True)
        e = 27.888 * (1.0 / torch.cdist(N, O) + 1.0 / torch.cdist(H, C) - 1.0 / torch.cdist(H, O) - 1.0 / torch.cdist(N, C))
        e = e.clamp(min=-9.9)
        ok = (torch.cdist(CA, CA) < 9.0) & ~eye & ~prev
        ok[:, 0] = False                                                                      # the first row has no amide hydrogen
        if valid is not None:
            v = valid[c0:c0 + chunk]
            ok &= v[:, :, None] & v[:, None, :]
        e = torch.where(ok & (e < 0), e, torch.zeros((), device=pos.device))
        last = torch.topk(e, 2, dim=2, largest=False), torch.topk(e, 2, dim=1, largest=False)
    return last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=16384)
    ap.add_argument("--residues", type=int, default=350)
    ap.add_argument("--jitter", type=float, default=0.1)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk-bytes", type=float, default=4e9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dssp.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dssp_rate: no HIP device; a time is measured on the GPU or not at all")
    from foldcomp_amd import _lib, api, synthetic
    dev = torch.device("cuda:0")
    torch.cuda.init()
    codec = api.default_codec()
    codec.enable_timing(True)
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    n, L = args.chains, args.residues
    doc = {"layout": "backbone4", "chains": n, "jitter_sigma": args.jitter, "pass_rows": int(codec.lib.fcz_hbond_pass()), "device": torch.cuda.get_device_name(0),
           "method": f"host clock around call + synchronise, {args.warmup} warm-up and {args.reps} timed calls; *_kernel: HIP events, group 'dssp'"}

    def sync():
        torch.cuda.synchronize(); codec.synchronize()

    def times(call):
        ev = []

        def once():
            codec.reset_timing(); call(); codec.synchronize(); ev.append(codec.kernel_time("dssp")[0])
        wall = timed(once, sync, args.warmup, args.reps)
        return wall, ev[args.warmup:]

    def measure(pos, mask, bound, rows_n, rows, packed, lead):
        tabs = [torch.empty(lead + (2,), dtype=dt, device=dev) for dt in (torch.int32, torch.float32, torch.int32, torch.float32)]
        ss, sm = torch.empty(lead, dtype=torch.uint8, device=dev), torch.empty(lead, dtype=torch.uint8, device=dev)
        hb = codec.lib.fcz_hbond_packed_dev if packed else codec.lib.fcz_hbond_dev
        lb = codec.lib.fcz_dssp_labels_packed_dev if packed else codec.lib.fcz_dssp_labels_dev
        b = None if bound is None else bound.data_ptr()
        sync()
        w1, e1 = times(lambda: _lib.check(hb(codec.ctx, pos.data_ptr(), mask.data_ptr(), None, b, rows_n, rows, 2, *(t.data_ptr() for t in tabs)), "fcz_hbond"))
        w2, e2 = times(lambda: _lib.check(lb(codec.ctx, pos.data_ptr(), mask.data_ptr(), None, b, rows_n, rows, 2, tabs[0].data_ptr(), tabs[1].data_ptr(),
                                             ss.data_ptr(), sm.data_ptr()), "fcz_dssp_labels"))
        total = ss.numel()
        out = {"rows": total, "hbond": stats(w1), "hbond_kernel": stats(e1), "labels": stats(w2), "labels_kernel": stats(e2),
               "hbond_rows_per_s": total / (statistics.median(w1) * 1e-3), "labels_rows_per_s": total / (statistics.median(w2) * 1e-3),
               "bonds_per_row": float((tabs[1] < -0.5).sum()) / total,
               "ss_counts": dict(zip(api.SS_CLASSES, (int(v) for v in torch.bincount(ss.flatten().to(torch.int64), minlength=8).cpu())))}
        return out, tabs

    template = torch.from_numpy(helix(max(L, int(synthetic.mixed_lengths(n, seed=7).max())))).to(dev)

    # ---- padded ------------------------------------------------------------------------------------------------------------------
    pos = (template[:L][None] + args.jitter * torch.randn((n, L, 4, 3), device=dev, generator=gen)).contiguous()
    mask = torch.ones((n, L, 4), dtype=torch.uint8, device=dev)
    res, tabs = measure(pos, mask, None, n, L, False, (n, L))
    chunk = max(1, int(args.chunk_bytes // (4 * LIVE * L * L)))
    base = timed(lambda: baseline_padded(pos, None, chunk), sync, args.warmup, args.reps)
    (be, _), _ = baseline_padded(pos[-chunk:], None, chunk)
    res.update(residues_per_chain=L, torch_dense_map=stats(base), chunk_chains=chunk, torch_over_hbond=statistics.median(base) / res["hbond"]["median_ms"],
               max_abs_energy_difference_to_torch=float((be - tabs[1][-chunk:]).abs().max()))
    doc["padded"] = res
    print(json.dumps(res), flush=True)
    del pos, mask, tabs, be
    torch.cuda.empty_cache()

    # ---- packed ------------------------------------------------------------------------------------------------------------------
    lens = synthetic.mixed_lengths(n, seed=7)
    cu = np.concatenate([[0], np.cumsum(lens)])
    R, Lmax = int(cu[-1]), int(lens.max())
    cu_t = torch.from_numpy(cu.astype(np.int32)).to(dev)
    chain = torch.repeat_interleave(torch.arange(n, device=dev), torch.from_numpy(lens).to(dev))
    within = torch.arange(R, device=dev) - cu_t[:-1].to(torch.int64)[chain]
    pos = (template[within] + args.jitter * torch.randn((R, 4, 3), device=dev, generator=gen)).contiguous()
    mask = torch.ones((R, 4), dtype=torch.uint8, device=dev)
    res, tabs = measure(pos, mask, cu_t, n, R, True, (R,))
    pad_chunk = max(1, int(args.chunk_bytes // (4 * LIVE * Lmax * Lmax)))

    def base_packed():
        """padding chunk by chunk of chains: the whole [n, max_seqlen, 4, 3] batch need not exist at once"""
        last = None
        for c0 in range(0, n, pad_chunk):
            c1 = min(c0 + pad_chunk, n)
            r0, r1 = int(cu[c0]), int(cu[c1])
            pp = torch.zeros((c1 - c0, Lmax, 4, 3), dtype=torch.float32, device=dev)
            vv = torch.zeros((c1 - c0, Lmax), dtype=torch.bool, device=dev)
            pp[chain[r0:r1] - c0, within[r0:r1]] = pos[r0:r1]
            vv[chain[r0:r1] - c0, within[r0:r1]] = True
            last = baseline_padded(pp, vv, c1 - c0)
        return last

    base = timed(base_packed, sync, min(args.warmup, 1), min(args.reps, 3))
    res.update(max_seqlen=Lmax, mean_seqlen=R / n, torch_pad_dense_map=stats(base), chunk_chains=pad_chunk,
               torch_over_hbond=statistics.median(base) / res["hbond"]["median_ms"])
    doc["packed"] = res
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
