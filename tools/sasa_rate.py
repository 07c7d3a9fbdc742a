#!/usr/bin/env python3
"""Rate of the solvent-accessibility sweep (fcz_sasa_dev) beside a plain torch formulation of the same
surface on the same tensors -> one JSON document.

  chains   synthetic 350-residue chains (foldcomp_amd.synthetic) compressed, then decoded on the device into padded atom37 and
           atom14 tensors: 64 different chains, repeated to --chains. They are what the benchmark compresses: a plausible backbone
           walk with full side chains, not a packed globule, so a real fold buries more per atom than these do.
  steps    (layout, P) for P = 96, 128, 960. EVERY STEP IS A PROCESS OF ITS OWN under its own time limit (--step-timeout), run one
           after the other; the first that fails, is killed by a signal or runs out of time ends the script (nothing more is
           started on the device) and the document holds the steps that finished.
  baseline the dense formulation in torch float32 on the same device, chain by chain: the chain's atoms compacted, torch.cdist for
           the candidate mask, the surface points of a chunk of atoms, their squared distances to every atom, the masked
           comparison and any(); over --baseline-chains chains. It writes an atoms x atoms matrix and a [chunk, P, atoms] array
           per chain; the kernel writes neither.

Both sides: --warmup calls, then --reps calls, each timed by the host clock around the call and a device synchronise; the
kernel's HIP-event time (group "sasa") is reported beside it. A run without a GPU fails.

    python tools/sasa_rate.py --out profiles/sasa.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STEPS = [(layout, P) for layout in ("atom37", "atom14") for P in (96, 128, 960)]


def baseline_chain(torch, pos, mask, radius, probe, pts, chunk_bytes):
    """pos [L, A, 3], mask [L, A] bool, radius [L, A] -> the exposed points of the chain's atoms, int64 [atoms]"""
    atom = mask & (radius > 0)
    c, R = pos[atom], radius[atom] + probe
    near = torch.cdist(c, c) < (R[:, None] + R[None, :])
    near.fill_diagonal_(False)
    N, P = len(c), len(pts)
    out = torch.empty(N, dtype=torch.int64, device=pos.device)
    step = max(1, int(chunk_bytes // (4 * 4 * P * N)))
    R2 = (R * R)[None, None, :]
    for a in range(0, N, step):
        t = c[a:a + step, None, :] + R[a:a + step, None, None] * pts[None]                 # [s, P, 3]
        d2 = ((t[:, :, None, :] - c[None, None]) ** 2).sum(-1)                             # [s, P, N]
        out[a:a + step] = P - ((d2 < R2) & near[a:a + step, None, :]).any(-1).sum(-1)
    return out


def run_step(args, layout, P):
    import numpy as np
    import torch
    from knn_rate import stats, timed
    if not torch.cuda.is_available():
        sys.exit("sasa_rate: no HIP device; a time is measured on the GPU or not at all")
    import foldcomp_amd as foldcomp
    from foldcomp_amd import _lib, api, synthetic
    dev = torch.device("cuda:0")
    codec = api.default_codec()
    codec.enable_timing(True)
    L, n = args.residues, args.chains
    distinct = min(64, n)
    blob, off, st = codec.compress_batch(synthetic.to_chain_batch(synthetic.generate(distinct, [L] * distinct, seed=7)))
    assert (st == 0).all()
    records = [blob[int(off[k]):int(off[k + 1])].tobytes() for k in range(distinct)]
    t = foldcomp.decode_tensors(records, layout=layout, codec=codec)
    rep = (n + distinct - 1) // distinct
    pos = t["pos"].repeat(rep, 1, 1, 1)[:n].contiguous()
    mask = t["mask"].view(torch.uint8).repeat(rep, 1, 1)[:n].contiguous()
    aatype = t["aatype"].repeat(rep, 1)[:n].contiguous()
    A = pos.shape[2]
    lay = {37: 0, 14: 1}[A]
    pts = torch.from_numpy(api.sphere_points(P)).to(dev)
    counts = torch.empty((n, L, A), dtype=torch.int16, device=dev)
    sasa = torch.empty((n, L), dtype=torch.float32, device=dev)
    sm = torch.empty((n, L), dtype=torch.uint8, device=dev)

    def sync():
        torch.cuda.synchronize(); codec.synchronize()

    def call():
        _lib.check(codec.lib.fcz_sasa_dev(codec.ctx, pos.data_ptr(), mask.data_ptr(), aatype.data_ptr(), None, n, L, lay, None, api.SASA_PROBE, pts.data_ptr(), P,
                                          counts.data_ptr(), sasa.data_ptr(), sm.data_ptr()), "fcz_sasa_dev")

    ev = []

    def once():
        codec.reset_timing(); call(); codec.synchronize(); ev.append(codec.kernel_time("sasa")[0])

    sync()
    wall = timed(once, sync, args.warmup, args.reps)
    table = np.zeros((21, A), np.float32)
    _lib.check(codec.lib.fcz_sasa_default_radii(lay, table.ctypes.data), "fcz_sasa_default_radii")
    radius = torch.from_numpy(table).to(dev)[aatype.clamp(max=20).long()]
    atoms = int(((mask != 0) & (radius > 0)).sum())
    nb = min(args.baseline_chains, n)

    def base():
        last = None
        for e in range(nb):
            last = baseline_chain(torch, pos[e], mask[e] != 0, radius[e], api.SASA_PROBE, pts, args.chunk_bytes)
        return last

    bw = timed(base, sync, min(args.warmup, 1), min(args.reps, 3))
    got = counts[nb - 1][(mask[nb - 1] != 0) & (radius[nb - 1] > 0)].to(torch.int64)
    differ = int((got != base()).sum())                                        # (torch's cdist and fused sums round differently: a few decisions)
    med, bmed = statistics.median(wall) * 1e-3, statistics.median(bw) * 1e-3
    return {"layout": layout, "points": P, "chains": n, "residues_per_chain": L, "atoms_per_chain": atoms / n, "pass_atoms": int(codec.lib.fcz_sasa_pass()),
            "sasa": stats(wall), "sasa_kernel": stats(ev[args.warmup:]), "chains_per_s": n / med, "atoms_per_s": atoms / med,
            "mean_sasa_per_residue": float(sasa.sum() / sm.sum().clamp(min=1)), "torch_dense": stats(bw), "torch_chains": nb,
            "torch_chains_per_s": nb / bmed, "torch_over_sasa_per_chain": (bmed / nb) / (med / n), "atoms_differing_from_torch_in_one_chain": differ,
            "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=2048)
    ap.add_argument("--residues", type=int, default=350)
    ap.add_argument("--baseline-chains", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk-bytes", type=float, default=2e9)
    ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--step", nargs=2, metavar=("LAYOUT", "POINTS"), help="run one step in this process and print its JSON line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sasa.json"))
    args = ap.parse_args()
    if args.step:
        print(json.dumps(run_step(args, args.step[0], int(args.step[1]))), flush=True)
        return
    doc = {"method": f"host clock around call + synchronise, {args.warmup} warm-up and {args.reps} timed calls; sasa_kernel: HIP events, group 'sasa'; "
                     "torch_dense: per chain cdist + masked point tests, float32, same device, same process as the step", "steps": []}
    common = [f"--{k.replace('_', '-')}={getattr(args, k)}" for k in ("chains", "residues", "baseline_chains", "warmup", "reps", "chunk_bytes")]
    failed = None
    for layout, P in STEPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", layout, str(P)] + common, capture_output=True, text=True,
                               timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            failed = f"{layout} P = {P}: no result within {args.step_timeout} s"
            break
        if r.returncode != 0:
            failed = f"{layout} P = {P}: exit status {r.returncode}: {r.stderr[-400:]}"
            break
        doc["steps"].append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(doc["steps"][-1]), flush=True)
    if failed:
        doc["stopped"] = failed
        print("sasa_rate: stopped, nothing more is started: " + failed, file=sys.stderr)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
