#!/usr/bin/env python3
"""Time of the TM-align-style alignment of chain pairs (fcz_tmalign_dev) -> one JSON document.

The batch: --pairs (4 096) pairs of a 350-residue chain (a CA random walk of 3.8 A steps, backbone4 tensors) and a copy of it with 12
residues cut out of the middle and the last 3/8 swung by 60 degrees about a hinge, under a random rigid motion plus Gaussian noise
(sigma 0.5 A). Configurations, EACH IN A PROCESS OF ITS OWN under its own time limit (--limit seconds), with 2 warm-up and 5 timed calls:

  fragments      fcz_tmalign_dev with the defaults (gapless shifts, the best one's DP iteration, fragment pairs)
  no_fragments   the same without the fragment pairs
  tm_score       fcz_tmscore_dev on the same number of 350-residue chains against a moved, hinged copy of the same shape: what the
                 row-for-row search costs on these tensors

Reported per configuration: median / min / max of the host clock around the call and a device synchronise, the kernels' HIP-event time
(groups "tmalign" / "tmscore"), pairs per second, the seeds per pair (fcz_tmalign_seeds), and for the alignments the dynamic
programmes the call ran and their cells per second (fcz_tmalign_last_work). A configuration that fails or runs out of time is
reported as such and the others still run. A run without a GPU fails.

    python tools/tmalign_rate.py --out profiles/tmalign.json
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CONFIGS = ("fragments", "no_fragments", "tm_score")
CUT = 12


def child(args):
    import torch
    from knn_rate import stats, timed, walk
    from superpose_rate import rigid
    if not torch.cuda.is_available():
        sys.exit("tmalign_rate: no HIP device; a time is measured on the GPU or not at all")
    from foldcomp_amd import _lib, api
    from foldcomp_amd.structure import CChainSet, CTmAlignOut, CTmAlignParams, CTmScoreOut, TM_ALIGN_OUTPUTS
    dev = torch.device("cuda:0")
    codec = api.default_codec()
    codec.enable_timing(True)
    lib = codec.lib
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    n, L, A = args.pairs, args.residues, 4
    ca = walk(n * L, dev, gen).view(n, L, 3).cumsum(dim=1)
    at = L - (3 * L) // 8
    c, s = math.cos(math.pi / 3), math.sin(math.pi / 3)
    hinge = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32, device=dev)
    moved = ca.clone()
    moved[:, at:] = (ca[:, at:] - ca[:, at:at + 1]) @ hinge.T + ca[:, at:at + 1]
    rot, trans = rigid(n, dev, gen)
    moved = torch.bmm(moved, rot.transpose(1, 2)) + trans[:, None] + args.noise * torch.randn((n, L, 3), device=dev, generator=gen)

    def dense(xyz):
        pos = torch.zeros(xyz.shape[:2] + (A, 3), dtype=torch.float32, device=dev)
        mask = torch.zeros(xyz.shape[:2] + (A,), dtype=torch.uint8, device=dev)
        pos[:, :, 1], mask[:, :, 1] = xyz, 1
        return pos, mask

    def sync():
        torch.cuda.synchronize(); codec.synchronize()

    def times(call, group):
        ev = []

        def once():
            codec.reset_timing(); call(); codec.synchronize(); ev.append(codec.kernel_time(group)[0])
        wall = timed(once, sync, args.warmup, args.reps)
        return wall, ev[args.warmup:]

    pos_a, mask_a = dense(ca)
    doc = {"pairs": n, "residues": L}
    if args.child == "tm_score":
        pos_p, _ = dense(moved)
        o = dict(rot=torch.empty((n, 3, 3), device=dev), trans=torch.empty((n, 3), device=dev), tm=torch.empty((n,), device=dev))
        out = CTmScoreOut(o["rot"].data_ptr(), o["trans"].data_ptr(), None, None, None, o["tm"].data_ptr(), None, None, None)
        wall, ev = times(lambda: _lib.check(lib.fcz_tmscore_dev(codec.ctx, pos_a.data_ptr(), mask_a.data_ptr(), pos_p.data_ptr(), None, None, n, L, 2, 1, 0, 20,
                                                                ctypes.byref(out)), "fcz_tmscore_dev"), "tmscore")
        doc.update(seeds_per_chain=int(lib.fcz_tmscore_seeds(L, 0)), mean_tm=float(o["tm"].mean()))
    else:
        mid = L // 2
        keep = torch.cat([torch.arange(0, mid, device=dev), torch.arange(mid + CUT, L, device=dev)])
        pos_b, mask_b = dense(moved[:, keep])
        Lb = L - CUT
        pairs = torch.arange(n, dtype=torch.int32, device=dev).repeat_interleave(2).reshape(n, 2).contiguous()
        o = {k: torch.empty((n,) + ((L,) if tail == "wa" else tail), dtype=getattr(torch, dt), device=dev) for k, dt, tail in TM_ALIGN_OUTPUTS}
        out = CTmAlignOut(*(o[k].data_ptr() for k, _, _ in TM_ALIGN_OUTPUTS))
        sa = CChainSet(pos_a.data_ptr(), mask_a.data_ptr(), None, None, n, L)
        sb = CChainSet(pos_b.data_ptr(), mask_b.data_ptr(), None, None, n, Lb)
        frag = 1 if args.child == "fragments" else 0
        par = CTmAlignParams(frag, 4, 20, 2, (ctypes.c_double * 4)(0.6, 0.0), 0, 20)
        wall, ev = times(lambda: _lib.check(lib.fcz_tmalign_dev(codec.ctx, ctypes.byref(sa), ctypes.byref(sb), pairs.data_ptr(), n, L, Lb, 2, 1, ctypes.byref(par),
                                                                ctypes.byref(out)), "fcz_tmalign_dev"), "tmalign")
        dps, cells = ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(lib.fcz_tmalign_last_work(codec.ctx, ctypes.byref(dps), ctypes.byref(cells)), "fcz_tmalign_last_work")
        planted = torch.full((n, L), -1, dtype=torch.int32, device=dev)
        planted[:, keep] = torch.arange(Lb, dtype=torch.int32, device=dev)
        med = statistics.median(wall)
        doc.update(residues_b=Lb, seeds_per_pair=int(lib.fcz_tmalign_seeds(L, Lb, frag)), dps_per_pair=dps.value / n, dp_cells=cells.value,
                   dp_cells_per_s=cells.value / (med * 1e-3), mean_tm=float(o["tm"].mean()), mean_aligned=float(o["aligned"].to(torch.float32).mean()),
                   planted_pairs_recovered=float(((o["map"] == planted) & (planted >= 0)).sum() / (planted >= 0).sum()),
                   pairs_won_by_a_dp_seed=float((o["seed"] >= int(lib.fcz_tmalign_seeds(L, Lb, 0)) - 1).to(torch.float32).mean()))
    med = statistics.median(wall)
    doc.update(wall=stats(wall), kernel=stats(ev), pairs_per_s=n / (med * 1e-3), device=torch.cuda.get_device_name(0))
    print("RESULT " + json.dumps(doc), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--residues", type=int, default=350)
    ap.add_argument("--noise", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds a configuration's process may take")
    ap.add_argument("--only", choices=CONFIGS, action="append")
    ap.add_argument("--child", choices=CONFIGS, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tmalign.json"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    doc = {"layout": "backbone4", "slot": "CA", "noise_sigma": args.noise, "cut": CUT,
           "method": f"a process per configuration; host clock around call + synchronise, {args.warmup} warm-up and {args.reps} timed calls; kernel: HIP events"}
    for name in args.only or CONFIGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--pairs", str(args.pairs), "--residues", str(args.residues), "--noise", str(args.noise),
               "--warmup", str(args.warmup), "--reps", str(args.reps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            doc[name] = {"failed": f"no result within {args.limit:g} s"}
            print(json.dumps({name: doc[name]}), flush=True)
            break                                                              # (nothing more is started on a device that may be hung)
        lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            doc[name] = {"failed": f"exit status {r.returncode}", "stderr": r.stderr[-400:]}
            print(json.dumps({name: doc[name]}), flush=True)
            break
        doc[name] = json.loads(lines[-1][len("RESULT "):])
        print(json.dumps({name: doc[name]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 1 if any("failed" in v for v in doc.values() if isinstance(v, dict)) else 0


if __name__ == "__main__":
    sys.exit(main())
