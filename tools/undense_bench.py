#!/usr/bin/env python3
"""Measurements of the tensors -> FCZ path -> one JSON document.

  1. the `undense` kernel group (k_undense_count + k_undense_fill of fcz_undense_dev) by HIP events (fcz_ctx_kernel_time: median of
     9 calls after 3 warm-up calls) for 65 536 x 350-residue synthetic chains and a mixed-length batch, all three layouts, as read +
     written bytes per second beside fcz_selftest_copy's figure taken in the same process;
  2. the same group beside the compress kernels it precedes (compress_sizes + _index + _angles + _pack on the batch it built), from
     fcz_compress_dense_begin_dev in the same run;
  3. entries per second of foldcomp.encode_tensors on batches of 1 024 chains of 350 residues beside the route that exists without
     it: tensors to the host, PDB text written in Python, foldcomp.compress_many.

  4. the packed form (fcz_undense_packed_dev) on the same two batches in the same process, right behind the
     padded call of every layout: the same group, the same method, packed over padded time. No chain is refused for its length there.

    python tools/undense_bench.py --out profiles/undense.json
    python tools/undense_bench.py --skip-user-level --out profiles/undense_packed.json
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

from dense_bench import ATOM37, LAYOUTS

COMPRESS_GROUPS = ("compress_sizes", "compress_index", "compress_angles", "compress_pack")
RES3 = ["ALA", "ARG", "ASN", "ASP", "CYS", "GLN", "GLU", "GLY", "HIS", "ILE", "LEU", "LYS", "MET", "PHE", "PRO", "SER", "THR", "TRP", "TYR",
        "VAL", "UNK"]


def dense_tensors(codec, w, n, L, lay, A, dev):
    """the workload's records decoded into dense tensors of the layout (fcz_dense_dev)"""
    from foldcomp_amd import _lib
    from foldcomp_amd.structure import CDenseOut
    t = dict(pos=torch.empty((n, L, A, 3), dtype=torch.float32, device=dev), mask=torch.empty((n, L, A), dtype=torch.uint8, device=dev),
             aatype=torch.empty((n, L), dtype=torch.uint8, device=dev), plddt=torch.empty((n, L), dtype=torch.float32, device=dev),
             res_index=torch.empty((n, L), dtype=torch.int32, device=dev), length=torch.empty(n, dtype=torch.int32, device=dev))
    out = CDenseOut(*(t[k].data_ptr() for k in ("pos", "mask", "aatype", "plddt", "res_index", "length")))
    torch.cuda.synchronize()
    _lib.check(codec.lib.fcz_dense_dev(codec.ctx, w.blob_dev.data_ptr(), w.off_dev.data_ptr(), n, w.res_off_dev.data_ptr(),
                                       w.atom_off_dev.data_ptr(), ctypes.byref(w.cout), 0, lay, L, ctypes.byref(out)), "fcz_dense_dev")
    codec.synchronize()
    return t


def packed_tensors(codec, w, n, R, lay, A, dev):
    """the workload's records decoded into packed tensors of the layout (fcz_dense_packed_dev)"""
    from foldcomp_amd import _lib
    from foldcomp_amd.structure import CPackedOut
    t = dict(pos=torch.empty((R, A, 3), dtype=torch.float32, device=dev), mask=torch.empty((R, A), dtype=torch.uint8, device=dev),
             aatype=torch.empty(R, dtype=torch.uint8, device=dev), plddt=torch.empty(R, dtype=torch.float32, device=dev))
    out = CPackedOut(t["pos"].data_ptr(), t["mask"].data_ptr(), t["aatype"].data_ptr(), t["plddt"].data_ptr(), None, None, None)
    torch.cuda.synchronize()
    _lib.check(codec.lib.fcz_dense_packed_dev(codec.ctx, w.blob_dev.data_ptr(), w.off_dev.data_ptr(), n, w.res_off_dev.data_ptr(),
                                              w.atom_off_dev.data_ptr(), ctypes.byref(w.cout), 0, lay, ctypes.byref(out)), "fcz_dense_packed_dev")
    codec.synchronize()
    return t


def kernel_case(codec, bench, name, n_chains, n_res, mixed, L_cap, dev):
    from foldcomp_amd import _lib
    from foldcomp_amd.structure import CChainBatch, CDenseIn
    d = bench.generate_resident(n_chains, n_res, 25, 32768, dev, seed_base=0, mixed=mixed)
    w = bench.Workload(codec, d, dev)
    w.compress(); codec.synchronize()
    del d
    w.decompress(); codec.synchronize()
    lens = np.diff(w.res_off_dev.cpu().numpy().view(np.uint32).astype(np.int64))
    keep = lens <= L_cap                                                       # a chain longer than L is refused, not cropped
    L = int(lens[keep].max())
    n = n_chains
    res = {"case": name, "chains": n, "residues": int(lens[keep].sum()), "refused_longer_than_L": int((~keep).sum()), "L": L, "layouts": {}}
    codec.enable_timing(True)
    for lname, lay, A in LAYOUTS:
        t = dense_tensors(codec, w, n, L, lay, A, dev)
        s = CDenseIn(t["pos"].data_ptr(), t["mask"].data_ptr(), t["aatype"].data_ptr(), t["length"].data_ptr(), t["plddt"].data_ptr())
        out = CChainBatch(); counts = np.zeros(3, np.uint32); nbytes = ctypes.c_uint64(0)
        ms, comp = [], []
        for _ in range(3 + 9):
            codec.reset_timing()
            _lib.check(codec.lib.fcz_undense_dev(codec.ctx, ctypes.byref(s), n, L, lay, 25, ctypes.byref(out), counts.ctypes.data, None), "fcz_undense_dev")
            codec.synchronize()
            ms.append(codec.kernel_time("undense")[0])
        for _ in range(3 + 9):
            codec.reset_timing()
            _lib.check(codec.lib.fcz_compress_dense_begin_dev(codec.ctx, ctypes.byref(s), n, L, lay, 25, counts.ctypes.data, ctypes.byref(nbytes)),
                       "fcz_compress_dense_begin_dev")
            codec.synchronize()
            comp.append(sum(codec.kernel_time(g)[0] for g in COMPRESS_GROUPS))
        med, comp_ms = statistics.median(ms[3:]), statistics.median(comp[3:])
        R, M = int(counts[1]), int(counts[2])
        # read: pos of the rows that hold a residue, their mask (counting pass), aatype twice, plddt, the row words once per pass;
        # written: 13 B per atom, 9 B per residue, 2 B per row word, 12 B per chain
        read = R * (A * 13 + 2 + 4 + 4) + 4 * n
        written = 13 * M + 9 * R + 2 * R + 12 * n
        res["layouts"][lname] = dict(undense_ms=med, undense_ms_min=min(ms[3:]), undense_ms_max=max(ms[3:]), residues=R, atoms=M, bytes_read=read,
                                     bytes_written=written, gb_per_s=(read + written) / (med * 1e-3) / 1e9, residues_per_s=R / (med * 1e-3),
                                     compress_kernels_ms=comp_ms, share_of_undense_plus_compress=med / (med + comp_ms), fcz_bytes=int(nbytes.value))
        del t
        torch.cuda.empty_cache()
        # the packed form of the same batch: every chain, whatever its length; row_off is the decoder's res_off
        Rp = int(lens.sum())
        t = packed_tensors(codec, w, n, Rp, lay, A, dev)
        s = CDenseIn(t["pos"].data_ptr(), t["mask"].data_ptr(), t["aatype"].data_ptr(), None, t["plddt"].data_ptr())
        pms = []
        for _ in range(3 + 9):
            codec.reset_timing()
            _lib.check(codec.lib.fcz_undense_packed_dev(codec.ctx, ctypes.byref(s), w.res_off_dev.data_ptr(), n, Rp, lay, 25, ctypes.byref(out),
                                                        counts.ctypes.data, None), "fcz_undense_packed_dev")
            codec.synchronize()
            pms.append(codec.kernel_time("undense")[0])
        pmed = statistics.median(pms[3:])
        R2, M2 = int(counts[1]), int(counts[2])
        p_read = R2 * (A * 13 + 2 + 4 + 4) + 8 * n
        p_written = 13 * M2 + 9 * R2 + 2 * R2 + 16 * n
        res["layouts"][lname]["packed"] = dict(undense_ms=pmed, undense_ms_min=min(pms[3:]), undense_ms_max=max(pms[3:]), residues=R2, atoms=M2,
                                               bytes_read=p_read, bytes_written=p_written, gb_per_s=(p_read + p_written) / (pmed * 1e-3) / 1e9,
                                               residues_per_s=R2 / (pmed * 1e-3), ms_per_residue_over_padded=(pmed / R2) / (med / R),
                                               padded_spread=(max(ms[3:]) - min(ms[3:])) / med)
        del t
        torch.cuda.empty_cache()
    codec.enable_timing(False)
    del w
    torch.cuda.empty_cache()
    return res


def pdb_text(pos, mask, aatype, plddt, length, first):
    """one chain's host arrays -> PDB text, formatted in Python (the route without encode_tensors)"""
    lines, serial = [], 1
    for l in range(int(length)):
        rn = RES3[min(int(aatype[l]), 20)]
        for s in np.flatnonzero(mask[l]):
            x, y, z = pos[l, s]
            nm = ATOM37[s]
            lines.append("ATOM  %5d %-4s %3s A%4d    %8.3f%8.3f%8.3f%6.2f%6.2f          %2s  " %
                         (serial, (" " + nm) if len(nm) < 4 else nm, rn, first + l, x, y, z, 1.0, plddt[l], nm[0]))
            serial += 1
    return "\n".join(lines) + "\nTER\n"


def user_level(codec, bench, n_entries, n_text, dev):
    import foldcomp
    from foldcomp_amd import api
    api.set_codec(codec)
    d = bench.generate_resident(n_entries, 350, 25, 32768, dev, seed_base=0)
    w = bench.Workload(codec, d, dev)
    w.compress(); codec.synchronize()
    blob = w.blob_dev.cpu().numpy(); off = w.off_dev.cpu().numpy()
    del w, d
    entries = [blob[int(off[i]):int(off[i + 1])].tobytes() for i in range(n_entries)]
    batches = [foldcomp.decode_tensors(entries[i:i + 1024]) for i in range(0, n_entries, 1024)]
    for rep in range(2):                                      # the second pass is the measured one
        torch.cuda.synchronize(); t0 = time.perf_counter()
        n_rec = sum(len(foldcomp.encode_tensors(b)) for b in batches)
        t_new = time.perf_counter() - t0
    assert n_rec == n_entries
    t0 = time.perf_counter()
    done = 0
    for b in batches:
        if done >= n_text:
            break
        host = {k: b[k].cpu().numpy() for k in ("pos", "mask", "aatype", "plddt", "length", "res_index")}
        m = min(len(b["names"]), n_text - done)
        items = [(b["names"][i], pdb_text(host["pos"][i], host["mask"][i], host["aatype"][i], host["plddt"][i], host["length"][i],
                                           int(host["res_index"][i, 0]))) for i in range(m)]
        assert len(foldcomp.compress_many(items)) == m
        done += m
    t_old = time.perf_counter() - t0
    api.set_codec(None)
    return dict(entries=n_entries, residues_per_entry=350, batch_size=1024, encode_tensors_entries_per_s=n_entries / t_new,
                text_route_entries=done, text_route_entries_per_s=done / t_old, ratio=(n_entries / t_new) / (done / t_old))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    ap.add_argument("--skip-user-level", action="store_true")
    ap.add_argument("--entries", type=int, default=20000)
    ap.add_argument("--text-entries", type=int, default=2048, help="entries put through the text route (it formats and parses in Python)")
    ap.add_argument("--mixed-chains", type=int, default=100000)
    ap.add_argument("--mixed-max-len", type=int, default=1024, help="L of the mixed batch; longer chains are refused by the call")
    args = ap.parse_args()
    torch.cuda.init()
    dev = torch.device("cuda:0")
    import bench
    from foldcomp_amd import _lib
    from foldcomp_amd.codec import Codec
    codec = Codec(0)
    gbs = ctypes.c_double(0)
    _lib.check(codec.lib.fcz_selftest_copy(codec.ctx, ctypes.c_uint64(1 << 30), 10, ctypes.byref(gbs)), "fcz_selftest_copy")
    doc = {"label": args.label, "device": torch.cuda.get_device_name(0), "copy_ceiling_gb_per_s": gbs.value,
           "method": "HIP events on the ctx stream, median of 9 after 3 warm-up calls",
           "kernel": [kernel_case(codec, bench, "65536 x 350", 65536, 350, False, 1 << 30, dev),
                      kernel_case(codec, bench, f"{args.mixed_chains} mixed (L = {args.mixed_max_len})", args.mixed_chains, 0, True, args.mixed_max_len, dev)]}
    for c in doc["kernel"]:
        for v in c["layouts"].values():
            v["fraction_of_copy_ceiling"] = v["gb_per_s"] / gbs.value
            v["packed"]["fraction_of_copy_ceiling"] = v["packed"]["gb_per_s"] / gbs.value
    if not args.skip_user_level:
        doc["user_level"] = user_level(codec, bench, args.entries, args.text_entries, dev)
    codec.close()
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
