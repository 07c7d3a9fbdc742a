#!/usr/bin/env python3
"""Rate of the structural-violations sweep (fcz_violations_dev) beside a dense torch formulation of the same
definition and beside fcz_sasa_dev at its defaults, all on the same tensors in the same process -> one JSON document.

  chains   synthetic 350-residue chains (foldcomp_amd.synthetic) compressed, then decoded on the device into padded atom37 or
           backbone4 tensors: 64 different chains, repeated to --chains, then every coordinate jittered by a normal deviate of
           --jitter Angstrom so that no two chains are the same. They are what the benchmark compresses: a plausible backbone walk
           with full side chains, not a packed globule.
  steps    the layouts atom37 and backbone4. EVERY STEP IS A PROCESS OF ITS OWN under its own time limit (--step-timeout), run one
           after the other; the first that fails, is killed by a signal or runs out of time ends the script (nothing more is
           started on the device) and the document holds the steps that finished.
  baseline the dense formulation in torch float32 on the same device, in batches of --baseline-batch chains over --baseline-chains
           chains: every slot of a chain an atom or not, T = (Ri + Rj) - tolerance and d2 as [b, L * A, L * A] matrices by
           broadcasting (the same operations in the same order, so the same decisions), the row, peptide-bond and disulfide masks, and
           the per-row sums. It writes several atoms x atoms arrays per chain; the kernel writes none. Its per-row clash counts are
           compared with the kernel's.
  sasa     fcz_sasa_dev with probe 1.4 and 128 points on the same tensors, timed the same way.

Every side: --warmup calls, then --reps calls, each timed by the host clock around the call and a device synchronise; the kernels'
HIP-event times (groups "violations" and "sasa") are reported beside it. A run without a GPU fails.

    python tools/violations_rate.py --out profiles/violations.json
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

STEPS = ("atom37", "backbone4")
TILE_ROWS = {37: 20, 14: 18, 4: 64}                                          # viol_tile_rows (foldcomp_amd/csrc/fcz_violations.h)


def baseline_batch(torch, pos, mask, aatype, radius, tol, sg_slot):
    """pos [b, L, A, 3], mask [b, L, A] bool, aatype [b, L], radius [b, L, A] -> clash_count int64 [b, L] of the dense formulation"""
    b, L, A = mask.shape
    atom = (mask & (radius > 0) & torch.isfinite(pos).all(-1)).reshape(b, L * A)
    c, R = pos.reshape(b, L * A, 3), radius.reshape(b, L * A)
    row = torch.arange(L, device=pos.device).repeat_interleave(A)
    slot = torch.arange(A, device=pos.device).repeat(L)
    T = (R[:, :, None] + R[:, None, :]) - tol
    d = c[:, :, None, :] - c[:, None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    clash = atom[:, :, None] & atom[:, None, :] & (row[:, None] != row[None, :])[None] & (T > 0) & (d2 < T * T)
    peptide = ((slot == 2)[:, None] & (slot == 0)[None, :] & (row[None, :] == row[:, None] + 1))
    clash &= ~(peptide | peptide.T)[None]
    if sg_slot >= 0:
        sg = (slot == sg_slot)[None] & (aatype == 4).repeat_interleave(A, dim=1)
        clash &= ~(sg[:, :, None] & sg[:, None, :])
    return clash.sum(-1).reshape(b, L, A).sum(-1)


def run_step(args, layout):
    import numpy as np
    import torch
    from knn_rate import stats, timed
    if not torch.cuda.is_available():
        sys.exit("violations_rate: no HIP device; a time is measured on the GPU or not at all")
    import foldcomp_amd as foldcomp
    from foldcomp_amd import _lib, api, synthetic
    from foldcomp_amd.tensors import _dense_written, _sasa_into, _viol_alloc, _viol_into
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
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    chunk = max(1, n // 16)
    for c0 in range(0, n, chunk):                                             # (in pieces: the deviates of 65536 chains are 10 GB at once)
        pos[c0:c0 + chunk] += torch.randn(pos[c0:c0 + chunk].shape, generator=gen, device=dev) * args.jitter
    pos *= mask[..., None]                                                    # (pos stays 0 where the mask is off, as the decoder leaves it)
    A = pos.shape[2]
    lay = {37: 0, 14: 1, 4: 2}[A]
    out = _viol_alloc(torch, dev, (n, L), A, n)
    dense = _dense_written(codec, torch, dev, pos, mask, aatype, lay, n, L, None, False)

    def sync():
        torch.cuda.synchronize(); codec.synchronize()

    def call():
        _viol_into(dense, None, api.VIOLATION_TOLERANCE, api.VIOLATION_LINK_FACTOR, out)

    ev = []

    def once():
        codec.reset_timing(); call(); codec.synchronize(); ev.append(codec.kernel_time("violations")[0])

    sync()
    wall = timed(once, sync, args.warmup, args.reps)
    counts = out["chain_counts"].cpu().numpy()
    # ---- fcz_sasa_dev at its defaults on the same tensors ----
    pts = torch.from_numpy(api.sphere_points(api.SASA_POINTS)).to(dev)
    sasa_counts = torch.empty((n, L, A), dtype=torch.int16, device=dev)
    sasa_out = dict(sasa=torch.empty((n, L), dtype=torch.float32, device=dev), sasa_mask=torch.empty((n, L), dtype=torch.uint8, device=dev))
    sev = []

    def sasa_once():
        codec.reset_timing()
        _sasa_into(dense, None, api.SASA_PROBE, pts, sasa_counts, sasa_out)
        codec.synchronize(); sev.append(codec.kernel_time("sasa")[0])

    swall = timed(sasa_once, sync, args.warmup, args.reps)
    # ---- the dense torch formulation ----
    table = np.zeros((21, A), np.float32)
    _lib.check(codec.lib.fcz_sasa_default_radii(lay, table.ctypes.data), "fcz_sasa_default_radii")
    radius = torch.from_numpy(table).to(dev)[aatype.clamp(max=20).long()]
    nb, bb = min(args.baseline_chains, n), max(1, args.baseline_batch)
    sg_slot = int(codec.lib.fcz_dense_slot(lay, 4, codec.lib.fcz_atom_code_from_name(b"SG")))
    tol = torch.tensor(api.VIOLATION_TOLERANCE, dtype=torch.float32, device=dev)

    def base():
        return torch.cat([baseline_batch(torch, pos[e:e + bb], mask[e:e + bb] != 0, aatype[e:e + bb], radius[e:e + bb], tol, sg_slot) for e in range(0, nb, bb)])

    bw = timed(base, sync, min(args.warmup, 1), min(args.reps, 3))
    differ = int((base() != out["clash_count"][:nb].to(torch.int64)).sum())
    med, smed, bmed = statistics.median(wall) * 1e-3, statistics.median(swall) * 1e-3, statistics.median(bw) * 1e-3
    return {"layout": layout, "chains": n, "residues_per_chain": L, "atoms_per_chain": float(counts[:, 0].sum()) / n, "jitter": args.jitter,
            "pass_atoms": int(codec.lib.fcz_violations_pass()), "tile_rows": TILE_ROWS[A], "tolerance": api.VIOLATION_TOLERANCE,
            "link_factor": api.VIOLATION_LINK_FACTOR, "violations": stats(wall), "violations_kernel": stats(ev[args.warmup:]), "chains_per_s": n / med,
            "atom_pairs_per_s": float((counts[:, 0].astype(np.float64) ** 2).sum()) / med,
            "clashing_pairs_per_chain": float(counts[:, 1].sum()) / n, "bond_rows_per_chain": float(counts[:, 2].sum()) / n,
            "angle_rows_per_chain": float(counts[:, 3].sum()) / n,
            "sasa": stats(swall), "sasa_kernel": stats(sev[args.warmup:]), "sasa_points": api.SASA_POINTS, "sasa_pass_atoms": int(codec.lib.fcz_sasa_pass()),
            "sasa_chains_per_s": n / smed, "sasa_over_violations": smed / med,
            "torch_dense": stats(bw), "torch_chains": nb, "torch_batch": bb, "torch_chains_per_s": nb / bmed,
            "torch_over_violations_per_chain": (bmed / nb) / (med / n), "rows_differing_from_torch": differ, "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--residues", type=int, default=350)
    ap.add_argument("--jitter", type=float, default=0.05)
    ap.add_argument("--baseline-chains", type=int, default=8)
    ap.add_argument("--baseline-batch", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--step", metavar="LAYOUT", help="run one step in this process and print its JSON line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "violations.json"))
    args = ap.parse_args()
    if args.step:
        print(json.dumps(run_step(args, args.step)), flush=True)
        return
    doc = {"method": f"host clock around call + synchronise, {args.warmup} warm-up and {args.reps} timed calls; violations_kernel / sasa_kernel: HIP events, "
                     "groups 'violations' / 'sasa'; torch_dense: [b, L * A, L * A] float32 matrices by broadcasting, same device, same process as the step",
           "steps": []}
    common = [f"--{k.replace('_', '-')}={getattr(args, k)}" for k in ("chains", "residues", "jitter", "baseline_chains", "baseline_batch", "warmup", "reps")]
    failed = None
    for layout in STEPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", layout] + common, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            failed = f"{layout}: no result within {args.step_timeout} s"
            break
        if r.returncode != 0:
            failed = f"{layout}: exit status {r.returncode}: {r.stderr[-400:]}"
            break
        doc["steps"].append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(doc["steps"][-1]), flush=True)
    if failed:
        doc["stopped"] = failed
        print("violations_rate: stopped, nothing more is started: " + failed, file=sys.stderr)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
