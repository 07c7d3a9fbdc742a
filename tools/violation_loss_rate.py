#!/usr/bin/env python3
"""Time and peak memory of the violation loss (fcz_violation_loss_dev, fcz_violation_loss_grad_dev, foldcomp.violation_loss; DESIGN.md
section 6.21) beside fcz_violations_dev and beside the dense torch formulation with autograd, on the same tensors in one process ->
one JSON document.

  --chains synthetic 350-residue chains as padded atom37 tensors: the workload of tools/violations_rate.py (64 different chains of
  foldcomp_amd.synthetic, compressed, decoded on the device, repeated, every coordinate jittered by --jitter Angstrom).

    violations            fcz_violations_dev, the metric whose sweep the value kernel repeats
    value                 fcz_violation_loss_dev
    value_and_gradient    fcz_violation_loss_dev, then fcz_violation_loss_grad_dev with the weights of the loss
    violation_loss        foldcomp.violation_loss(pos, true)["loss"].backward(): the two kernels, the chain sums in torch, pos.grad
    torch_dense           the dense formulation in torch float32 with autograd (T and d as [b, L * A, L * A] matrices, relu, the three
                          link terms, loss.backward()) in batches of --dense-batch chains over --dense-chains chains

Every side: --warmup calls, then --reps calls, each timed by the host clock around the call and a device synchronise; the kernels'
HIP-event times (groups "violations", "violation_loss", "violation_loss_grad") are reported beside them. Peak memory is torch's
allocator peak above what was allocated before the call (the inputs). No rate is asserted: what is measured is recorded. A run
without a GPU fails.

    python tools/violation_loss_rate.py --out profiles/violation_loss.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch

from knn_rate import stats, timed

L0, SL, L0_PRO, SL_PRO, COS0, S0, COS1, S1 = 1.329, 0.014, 1.341, 0.016, -0.4473, 0.0311, -0.5203, 0.0353


def dense_loss(pos, mask, aatype, radius, tol, factor, sg_slot):
    """pos [b, L, A, 3] (requires grad), mask [b, L, A] bool, aatype [b, L], radius [b, L, A] -> the mean over the chains of
    clash sum / atoms + mean bond term + the two mean cosine terms"""
    b, L, A = mask.shape
    atom = (mask & (radius > 0)).reshape(b, L * A)
    c, R = pos.reshape(b, L * A, 3), radius.reshape(b, L * A)
    row = torch.arange(L, device=pos.device).repeat_interleave(A)
    slot = torch.arange(A, device=pos.device).repeat(L)
    pair = atom[:, :, None] & atom[:, None, :] & (row[:, None] != row[None, :])[None]
    peptide = ((slot == 2)[:, None] & (slot == 0)[None, :] & (row[None, :] == row[:, None] + 1))
    pair &= ~(peptide | peptide.T)[None]
    if sg_slot >= 0:
        sg = (slot == sg_slot)[None] & (aatype == 4).repeat_interleave(A, dim=1)
        pair &= ~(sg[:, :, None] & sg[:, None, :])
    T = (R[:, :, None] + R[:, None, :]) - tol
    d = torch.cdist(c, c)
    clash = (torch.relu(T - d) * pair).sum(dim=(1, 2)) / atom.sum(dim=1).clamp(min=1)
    ca, cc, n1, ca1 = pos[:, :-1, 1], pos[:, :-1, 2], pos[:, 1:, 0], pos[:, 1:, 1]
    link = (mask[:, :-1, 1] & mask[:, :-1, 2] & mask[:, 1:, 0] & mask[:, 1:, 1]).to(pos.dtype)
    cos = lambda a, m, e: ((a - m) * (e - m)).sum(-1) / ((a - m).norm(dim=-1) * (e - m).norm(dim=-1)).clamp(min=1e-12)
    pro = aatype[:, 1:] == 14
    l0, sl = torch.where(pro, L0_PRO, L0), torch.where(pro, SL_PRO, SL)
    terms = (torch.relu(((cc - n1).norm(dim=-1) - l0).abs() - factor * sl) + torch.relu((cos(ca, cc, n1) - COS0).abs() - factor * S0) +
             torch.relu((cos(cc, n1, ca1) - COS1).abs() - factor * S1))
    return (clash + (terms * link).sum(dim=1) / link.sum(dim=1).clamp(min=1)).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=16384)
    ap.add_argument("--residues", type=int, default=350)
    ap.add_argument("--jitter", type=float, default=0.2)
    ap.add_argument("--tolerance", type=float, default=1.5)
    ap.add_argument("--link-factor", type=float, default=12.0)
    ap.add_argument("--dense-chains", type=int, default=8)
    ap.add_argument("--dense-batch", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "violation_loss.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("violation_loss_rate: no HIP device; a time is measured on the GPU or not at all")
    import numpy as np
    import foldcomp_amd as foldcomp
    from foldcomp_amd import _lib, api, synthetic
    from foldcomp_amd.tensors import _dense_written, _viol_alloc, _viol_into
    dev = torch.device("cuda:0")
    codec = api.default_codec()
    codec.enable_timing(True)
    n, L, tol, factor = args.chains, args.residues, args.tolerance, args.link_factor
    distinct = min(64, n)
    blob, off, st = codec.compress_batch(synthetic.to_chain_batch(synthetic.generate(distinct, [L] * distinct, seed=7)))
    assert (st == 0).all()
    t = foldcomp.decode_tensors([blob[int(off[k]):int(off[k + 1])].tobytes() for k in range(distinct)], layout="atom37", codec=codec)
    rep = (n + distinct - 1) // distinct
    pos = t["pos"].repeat(rep, 1, 1, 1)[:n].contiguous()
    mask = t["mask"].view(torch.uint8).repeat(rep, 1, 1)[:n].contiguous()
    aatype = t["aatype"].repeat(rep, 1)[:n].contiguous()
    gen = torch.Generator(device=dev); gen.manual_seed(11)
    chunk = max(1, n // 16)
    for c0 in range(0, n, chunk):
        pos[c0:c0 + chunk] += torch.randn(pos[c0:c0 + chunk].shape, generator=gen, device=dev) * args.jitter
    pos *= mask[..., None]
    A = pos.shape[2]
    doc = {"layout": "atom37", "chains": n, "residues_per_chain": L, "jitter": args.jitter, "tolerance": tol, "link_factor": factor,
           "pass": int(codec.lib.fcz_violation_loss_pass()), "violations_pass": int(codec.lib.fcz_violations_pass()), "device": torch.cuda.get_device_name(0),
           "method": f"host clock around call + synchronise, {args.warmup} warm-up and {args.reps} timed calls; kernel: HIP events of the named groups; "
                     "peak_bytes: torch allocator peak above the inputs"}

    def sync():
        torch.cuda.synchronize(); codec.synchronize()

    def kernel_times(call, groups):
        ev = []

        def once():
            codec.reset_timing(); call(); codec.synchronize(); ev.append(sum(codec.kernel_time(g)[0] for g in groups))
        wall = timed(once, sync, args.warmup, args.reps)
        return wall, ev[args.warmup:]

    def peak_of(call, clear):
        clear()
        sync(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        call(); sync()
        return int(torch.cuda.max_memory_allocated(dev) - before)

    def entry(wall, chains, **more):
        d = dict(stats(wall), chains=chains, chains_per_s=chains / (statistics.median(wall) * 1e-3))
        d.update(more)
        return d

    metric = _viol_alloc(torch, dev, (n, L), A, n)
    dense = _dense_written(codec, torch, dev, pos, mask, aatype, 0, n, L, None, False)
    clash = torch.empty((n, L, A), dtype=torch.float32, device=dev); link = torch.empty((n, L, 3), dtype=torch.float32, device=dev)
    counts = torch.empty((n, 2), dtype=torch.int64, device=dev); grad = torch.empty((n, L, A, 3), dtype=torch.float32, device=dev)
    lib, ctx = codec.lib, codec.ctx
    common = (pos.data_ptr(), mask.data_ptr(), aatype.data_ptr(), None, n, L, 0, None, tol, factor)

    def hard():
        _viol_into(dense, None, tol, factor, metric)

    def value():
        _lib.check(lib.fcz_violation_loss_dev(ctx, *common, clash.data_ptr(), link.data_ptr(), counts.data_ptr()), "fcz_violation_loss_dev")

    sync()
    value(); sync()
    share = 1.0 / n
    w_clash = (share / counts[:, 0].clamp(min=1).to(torch.float64)).to(torch.float32)[:, None, None].expand(n, L, A).contiguous()
    w_link = (share / counts[:, 1].clamp(min=1).to(torch.float64)).to(torch.float32)[:, None, None].expand(n, L, 3).contiguous()

    def value_and_gradient():
        value()
        _lib.check(lib.fcz_violation_loss_grad_dev(ctx, *common, w_clash.data_ptr(), w_link.data_ptr(), grad.data_ptr()), "fcz_violation_loss_grad_dev")

    wall, ev = kernel_times(hard, ("violations",))
    doc["violations"] = entry(wall, n, kernel=stats(ev))
    wall, ev = kernel_times(value, ("violation_loss",))
    doc["value"] = entry(wall, n, kernel=stats(ev))
    wall, ev = kernel_times(value_and_gradient, ("violation_loss", "violation_loss_grad"))
    doc["value_and_gradient"] = entry(wall, n, kernel=stats(ev))
    hard(); sync()
    doc["atoms_per_chain"] = float(counts[:, 0].sum()) / n
    doc["atoms_equal_chain_counts"] = bool((counts[:, 0] == metric["chain_counts"][:, 0]).all())
    doc["clashing_pairs_per_chain"] = float(metric["chain_counts"][:, 1].sum()) / n
    doc["atoms_with_a_loss_equal_clash_atoms_with_depth"] = bool(((clash > 0).any(dim=2) >= (metric["clash_depth"] > 0)).all())
    base = doc["violations"]["kernel"]["median_ms"]
    doc["value_over_violations"] = doc["value"]["kernel"]["median_ms"] / base
    doc["value_and_gradient_over_violations"] = doc["value_and_gradient"]["kernel"]["median_ms"] / base
    print(json.dumps({k: doc[k] for k in ("violations", "value", "value_and_gradient", "value_over_violations", "value_and_gradient_over_violations")}), flush=True)

    # ---- the Python surface: forward and backward ----------------------------------------------------------------------------------
    true = dict(mask=mask.view(torch.bool), aatype=aatype)
    leaf = pos.clone().requires_grad_()
    out = {}

    def no_grad_yet():
        leaf.grad = None

    def surface():
        leaf.grad = None
        out["loss"] = foldcomp.violation_loss(leaf, true, tolerance=tol, link_factor=factor, codec=codec)["loss"]
        out["loss"].backward()

    wall = timed(surface, sync, args.warmup, args.reps)
    doc["violation_loss"] = entry(wall, n, loss=float(out["loss"].detach()), peak_bytes=peak_of(surface, no_grad_yet), pos_grad_bytes=int(leaf.numel() * 4),
                                  input_bytes=int(pos.numel() * 4 + mask.numel() + aatype.numel()))
    doc["violation_loss"]["peak_bytes_per_chain"] = doc["violation_loss"]["peak_bytes"] / n
    doc["violation_loss_over_violations"] = doc["violation_loss"]["median_ms"] / doc["violations"]["median_ms"]
    surface_grad = leaf.grad.clone()
    print(json.dumps(doc["violation_loss"]), flush=True)

    # ---- the dense torch formulation with autograd ---------------------------------------------------------------------------------
    c, b = min(args.dense_chains, n), max(1, args.dense_batch)
    table = np.zeros((21, A), np.float32)
    _lib.check(lib.fcz_sasa_default_radii(0, table.ctypes.data), "fcz_sasa_default_radii")
    radius = torch.from_numpy(table).to(dev)[aatype[:c].clamp(max=20).long()]
    sg_slot = int(lib.fcz_dense_slot(0, 4, lib.fcz_atom_code_from_name(b"SG")))
    cp = pos[:c].clone().requires_grad_()
    dl = {}

    def no_dense_grad_yet():
        cp.grad = None

    def dense_call():
        cp.grad = None
        total = 0.0
        for e in range(0, c, b):
            part = dense_loss(cp[e:e + b], mask[e:e + b] != 0, aatype[e:e + b], radius[e:e + b], tol, factor, sg_slot) * (min(e + b, c) - e) / c
            part.backward()
            total += float(part.detach())
        dl["loss"] = total

    wall = timed(dense_call, sync, args.warmup, args.reps)
    peak = peak_of(dense_call, no_dense_grad_yet)
    doc["torch_dense"] = entry(wall, c, loss=dl["loss"], batch=b, peak_bytes=peak, peak_bytes_per_chain=peak / min(b, c))
    # the two agree up to float32 rounding (a sanity check of the workload, not of the bits): the dense loss is the mean over c chains,
    # the surface's over n, so its gradient is rescaled
    doc["max_abs_gradient_difference_to_torch"] = float((cp.grad - surface_grad[:c] * (n / c)).abs().max())
    doc["max_abs_gradient_of_torch"] = float(cp.grad.abs().max())
    for k in ("value", "value_and_gradient", "violation_loss"):
        doc[f"{k}_over_torch_dense_chains_per_s"] = doc[k]["chains_per_s"] / doc["torch_dense"]["chains_per_s"]
    print(json.dumps(doc["torch_dense"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
