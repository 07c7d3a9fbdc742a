#!/usr/bin/env python3
"""Rate of the all-atom lDDT sweeps (fcz_lddt_atoms_dev) with the side-chain renaming on and off, and beside
them, from the same run on the same tensors, the rates of the CA lDDT (fcz_lddt_dev) and of the structural violations
(fcz_violations_dev) as context -> one JSON document.

  chains   synthetic 350-residue chains (foldcomp_amd.synthetic) compressed, then decoded on the device into padded atom37 tensors:
           64 different chains, repeated to --chains. They are what the benchmark compresses: a plausible backbone walk with full
           side chains, not a packed globule.
  pred     the truth plus a normal deviate of --noise Angstrom on every coordinate, different for every chain, with the symmetric
           atoms of every second swap-capable residue exchanged (foldcomp.lddt_swaps), so that the renaming has rows to find.
  steps    the layout atom37. EVERY STEP IS A PROCESS OF ITS OWN under its own time limit (--step-timeout); a step that fails, is
           killed by a signal or runs out of time ends the script (nothing more is started on the device).
  sides    lddt_atoms with swaps="alphafold" (both sweeps do work), lddt_atoms with swaps=None (the decide sweep finds no query atom),
           lddt on CA, violations at its defaults: the public calls, so the chain sums of the lDDT calls are inside their times.

Every side: --warmup calls, then --reps calls, each timed by the host clock around the call and a device synchronise; the kernels'
HIP-event times (groups "lddt_atoms", "lddt", "violations") are reported beside it. A run without a GPU fails.

    python tools/lddt_atoms_rate.py --out profiles/lddt_atoms.json
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

STEPS = ("atom37",)
TILE_ROWS = {37: 20, 14: 18, 4: 64}                                          # lddta_tile_rows of the score sweep (foldcomp_amd/csrc/fcz_lddt_atoms.h)
DECIDE_ROWS = 64


def run_step(args, layout):
    import torch
    from knn_rate import stats, timed
    if not torch.cuda.is_available():
        sys.exit("lddt_atoms_rate: no HIP device; a time is measured on the GPU or not at all")
    import foldcomp_amd as foldcomp
    from foldcomp_amd import api, synthetic
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
    mask = t["mask"].repeat(rep, 1, 1)[:n].contiguous()
    aatype = t["aatype"].repeat(rep, 1)[:n].contiguous()
    A = pos.shape[2]
    table = torch.from_numpy(foldcomp.lddt_swaps(layout)).to(dev).long()
    partner = table[aatype.clamp(max=20).long()]                              # [n, L, A]
    capable = (partner != torch.arange(A, device=dev)).any(-1)
    flat = capable.flatten().nonzero().flatten()[::2]
    exchanged = torch.zeros(n * L, dtype=torch.bool, device=dev)
    exchanged[flat] = True
    sel = torch.where(exchanged.view(n, L, 1), partner, torch.arange(A, device=dev).expand(n, L, A))
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    pred = torch.empty_like(pos)
    chunk = max(1, n // 16)
    for c0 in range(0, n, chunk):                                             # (in pieces: the deviates of many chains are gigabytes at once)
        p = pos[c0:c0 + chunk] + torch.randn(pos[c0:c0 + chunk].shape, generator=gen, device=dev) * args.noise
        pred[c0:c0 + chunk] = torch.gather(p, 2, sel[c0:c0 + chunk, :, :, None].expand(-1, -1, -1, 3))
    pred *= mask[..., None]
    true = dict(pos=pos, mask=mask, aatype=aatype)
    pred_d = dict(pos=pred, mask=mask)
    del partner, sel

    def sync():
        torch.cuda.synchronize(); codec.synchronize()

    last = {}

    def side(name, group, fn):
        ev = []

        def once():
            codec.reset_timing(); last[name] = fn(); codec.synchronize(); ev.append(codec.kernel_time(group)[0])

        sync()
        wall = timed(once, sync, args.warmup, args.reps)
        return stats(wall), stats(ev[args.warmup:]), n / (statistics.median(wall) * 1e-3)

    out = {"layout": layout, "chains": n, "residues_per_chain": L, "noise": args.noise, "pass_atoms": int(codec.lib.fcz_lddt_atoms_pass()),
           "tile_rows": TILE_ROWS[A], "decide_tile_rows": DECIDE_ROWS, "device": torch.cuda.get_device_name(0)}
    for name, group, fn in (("renaming_on", "lddt_atoms", lambda: foldcomp.lddt_atoms(pred_d, true, codec=codec)),
                            ("renaming_off", "lddt_atoms", lambda: foldcomp.lddt_atoms(pred_d, true, swaps=None, codec=codec)),
                            ("lddt_ca", "lddt", lambda: foldcomp.lddt(pred_d, true, codec=codec)),
                            ("violations", "violations", lambda: foldcomp.violations(true, codec=codec))):
        wall, kernel, rate = side(name, group, fn)
        out[name] = wall
        out[name + "_kernel"] = kernel
        out[name + "_chains_per_s"] = rate
    on, off_ = last["renaming_on"], last["renaming_off"]
    pairs = float(on["lddt_pairs"].sum(dtype=torch.int64))
    out.update(atoms_per_chain=float(last["violations"]["chain_counts"][:, 0].sum()) / n, atom_pairs_within_cutoff_per_chain=pairs / n,
               exchanged_rows=int(exchanged.sum()), swapped_rows=int(on["swapped"].sum()), swapped_and_exchanged=int((on["swapped"].flatten() & exchanged).sum()),
               mean_lddt_renaming_on=float(on["lddt_chain"].mean()), mean_lddt_renaming_off=float(off_["lddt_chain"].mean()),
               mean_lddt_ca=float(last["lddt_ca"]["lddt_chain"].mean()),
               lddt_atoms_over_lddt_ca=out["lddt_ca_chains_per_s"] / out["renaming_on_chains_per_s"],
               lddt_atoms_over_violations=out["violations_chains_per_s"] / out["renaming_on_chains_per_s"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=8192)
    ap.add_argument("--residues", type=int, default=350)
    ap.add_argument("--noise", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--step", metavar="LAYOUT", help="run one step in this process and print its JSON line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lddt_atoms.json"))
    args = ap.parse_args()
    if args.step:
        print(json.dumps(run_step(args, args.step)), flush=True)
        return
    doc = {"method": f"host clock around the public call + synchronise, {args.warmup} warm-up and {args.reps} timed calls; *_kernel: HIP events, groups "
                     "'lddt_atoms' / 'lddt' / 'violations'; all sides on the same tensors in the same process",
           "steps": []}
    common = [f"--{k.replace('_', '-')}={getattr(args, k)}" for k in ("chains", "residues", "noise", "warmup", "reps")]
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
        print("lddt_atoms_rate: stopped, nothing more is started: " + failed, file=sys.stderr)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
