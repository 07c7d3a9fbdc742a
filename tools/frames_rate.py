#!/usr/bin/env python3
"""Time of the rigid-frame kernel (fcz_frames_dev) beside a torch formulation on the same tensors and beside
a device copy, in one process -> one JSON document.

  padded   65 536 synthetic 350-residue chains as atom37 tensors [n, L, 37, 3] (every slot set, random residue types);
  packed   the same number of chains with the mixed benchmark's lengths (synthetic.mixed_lengths: log-normal, 16 .. 2 700) as
           packed rows [R, 37, 3] -- the call is n = 1, L = R.

Both with groups = "all" and "backbone". The torch baseline is the straightforward one: a table gather of the three defining
atoms per group (three slices for the backbone), the same Gram-Schmidt, `stack`, `where` on the mask. Both sides: --warmup calls,
then --reps calls, each timed by the host clock around the call and a device synchronise; the kernel's HIP-event time (group
"frames") is reported beside it, and the bytes the kernel reads plus writes over that time beside fcz_selftest_copy's read +
written bytes per second. Median, fastest and slowest are given. A run without a GPU fails.

    python tools/frames_rate.py --out profiles/frames.json
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


def gram_schmidt(v1, v2):
    e1 = v1 / v1.norm(dim=-1, keepdim=True)
    u = v2 - e1 * (e1 * v2).sum(dim=-1, keepdim=True)
    e2 = u / u.norm(dim=-1, keepdim=True)
    return torch.stack([e1, e2, torch.cross(e1, e2, dim=-1)], dim=-1)


def torch_backbone(pos, mask):
    """pos [R, A, 3], mask [R, A] -> rot [R, 3, 3], trans [R, 3], frame_mask [R]"""
    n_, ca, c = pos[:, 0], pos[:, 1], pos[:, 2]
    rot = gram_schmidt(c - ca, n_ - ca)
    ok = mask[:, 0].bool() & mask[:, 1].bool() & mask[:, 2].bool() & torch.isfinite(rot).all(dim=-1).all(dim=-1)
    eye = torch.eye(3, device=pos.device)
    return torch.where(ok[:, None, None], rot, eye), torch.where(ok[:, None], ca, torch.zeros((), device=pos.device)), ok


def torch_all(pos, mask, aatype, slots, sign):
    """slots long [21, 8, 3] (-1 = none), sign [8, 1] (+1 for group 0, -1 else) -> rot [R, 8, 3, 3], trans [R, 8, 3], frame_mask [R, 8]"""
    R = pos.shape[0]
    sl = slots[aatype.clamp(max=20).long()]                                   # [R, 8, 3]
    have = (sl >= 0).all(dim=-1)
    s = sl.clamp(min=0).view(R, 24)
    atoms = pos.gather(1, s[:, :, None].expand(R, 24, 3)).view(R, 8, 3, 3)   # [row, group, atom j, xyz]
    ok = have & mask.gather(1, s).view(R, 8, 3).bool().all(dim=-1)
    a0, a1, a2 = atoms[:, :, 0], atoms[:, :, 1], atoms[:, :, 2]
    rot = gram_schmidt((a0 - a1) * sign, a2 - a1)
    ok = ok & torch.isfinite(rot).all(dim=-1).all(dim=-1)
    eye = torch.eye(3, device=pos.device)
    return torch.where(ok[..., None, None], rot, eye), torch.where(ok[..., None], a1, torch.zeros((), device=pos.device)), ok


def slot_table(lib, layout=0):
    """[21][8][3]: slot of defining atom j of (type, group) in the layout, -1 = none (fcz_frame_atom through fcz_dense_slot; groups 0
    and 3 through residue code 0: N, CA, C, O have the same slot in every type)"""
    tab = [[[-1] * 3 for _ in range(8)] for _ in range(21)]
    for ty in range(21):
        for g in range(8):
            if g >= 4 and ty >= 20:
                continue
            atoms = [lib.fcz_frame_atom(ty if ty < 20 else 0, g, j) for j in range(3)]
            if min(atoms) >= 0:
                tab[ty][g] = [lib.fcz_dense_slot(layout, ty if g >= 4 else 0, a) for a in atoms]
    return tab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--residues", type=int, default=350)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("frames_rate: no HIP device; a time is measured on the GPU or not at all")
    from foldcomp_amd import _lib, api, synthetic
    dev = torch.device("cuda:0")
    torch.cuda.init()
    codec = api.default_codec()
    codec.enable_timing(True)
    lib = codec.lib
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    n, L, A = args.chains, args.residues, 37
    slots = torch.tensor(slot_table(lib), dtype=torch.long, device=dev)
    sign = torch.tensor([1.0] + [-1.0] * 7, device=dev)[:, None]
    gbs = ctypes.c_double()
    _lib.check(lib.fcz_selftest_copy(codec.ctx, ctypes.c_uint64(1 << 30), 10, ctypes.byref(gbs)), "fcz_selftest_copy")
    doc = {"layout": "atom37", "chains": n, "device": torch.cuda.get_device_name(0), "device_copy_gb_per_s": gbs.value,
           "method": f"host clock around call + synchronise, {args.warmup} warm-up and {args.reps} timed calls; frames_kernel: HIP events, "
                     "group 'frames'; fraction_of_copy = (bytes read + written by the kernel / frames_kernel median) / fcz_selftest_copy "
                     "(1 GiB, read + written bytes) of the same process"}

    def sync():
        torch.cuda.synchronize(); codec.synchronize()

    def measure(pos, mask, aatype, rows_n, rows_L):
        R = rows_n * rows_L
        flat_pos, flat_mask, flat_aa = pos.view(R, A, 3), mask.view(R, A), aatype.view(R)
        res = {}
        for name, groups, G in (("all", 1, 8), ("backbone", 0, 1)):
            rot = torch.empty((R, G, 3, 3), dtype=torch.float32, device=dev)
            trans = torch.empty((R, G, 3), dtype=torch.float32, device=dev)
            fm = torch.empty((R, G), dtype=torch.uint8, device=dev)
            ev = []

            def once():
                codec.reset_timing()
                _lib.check(lib.fcz_frames_dev(codec.ctx, pos.data_ptr(), mask.data_ptr(), aatype.data_ptr() if groups else None, None, rows_n, rows_L, 0,
                                              groups, rot.data_ptr(), trans.data_ptr(), fm.data_ptr()), "fcz_frames_dev")
                codec.synchronize(); ev.append(codec.kernel_time("frames")[0])
            wall = timed(once, sync, args.warmup, args.reps)
            ev = ev[args.warmup:]
            base_fn = (lambda: torch_all(flat_pos, flat_mask, flat_aa, slots, sign)) if groups else (lambda: torch_backbone(flat_pos, flat_mask))
            base = timed(base_fn, sync, args.warmup, args.reps)
            b = base_fn()
            agree = float((b[2].view(R, G) == fm.bool()).float().mean())
            close = float(((b[0].view(R, G, 3, 3) - rot).abs().amax(dim=(-1, -2)) < 1e-4).float().mean())
            del b
            # what the kernel loads and stores: whole rows and the type byte for "all", N / CA / C and their mask bytes for "backbone"
            nbytes = R * ((A * 12 + A + 1) if groups else (36 + 3)) + R * G * 49
            rate = nbytes / (statistics.median(ev) * 1e-3) / 1e9
            res[name] = {"frames": stats(wall), "frames_kernel": stats(ev), "torch_gather_gram_schmidt_stack": stats(base), "bytes_read_plus_written": nbytes,
                         "gb_per_s": rate, "fraction_of_copy": rate / gbs.value, "torch_over_frames": statistics.median(base) / statistics.median(wall),
                         "mask_agreement_with_torch": agree, "rot_within_1e-4_of_torch": close}
            del rot, trans, fm
            torch.cuda.empty_cache()
        return res

    # ---- padded ------------------------------------------------------------------------------------------------------------------
    pos = (torch.randn((n, L, A, 3), device=dev, generator=gen) * 3.0).contiguous()
    mask = torch.ones((n, L, A), dtype=torch.uint8, device=dev)
    aatype = torch.randint(0, 20, (n, L), device=dev, generator=gen).to(torch.uint8)
    sync()
    doc["padded"] = dict(residues_per_chain=L, rows=n * L, **measure(pos, mask, aatype, n, L))
    print(json.dumps(doc["padded"]), flush=True)
    del pos, mask, aatype
    torch.cuda.empty_cache()

    # ---- packed ------------------------------------------------------------------------------------------------------------------
    lens = synthetic.mixed_lengths(n, seed=7)
    R = int(np.sum(lens))
    pos = (torch.randn((R, A, 3), device=dev, generator=gen) * 3.0).contiguous()
    mask = torch.ones((R, A), dtype=torch.uint8, device=dev)
    aatype = torch.randint(0, 20, (R,), device=dev, generator=gen).to(torch.uint8)
    sync()
    doc["packed"] = dict(rows=R, max_seqlen=int(lens.max()), mean_seqlen=R / n, **measure(pos, mask, aatype, 1, R))
    print(json.dumps(doc["packed"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
