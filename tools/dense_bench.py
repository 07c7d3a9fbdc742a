#!/usr/bin/env python3
"""Measurements of the dense-tensor path -> one JSON document.

  1. k_dense by HIP events (fcz_ctx_kernel_time group "dense": median of 9 calls after 3 warm-up calls) for 65 536 x 350-residue
     synthetic chains and a 100 000-chain mixed-length batch, all three layouts, as read + written bytes per second beside
     fcz_selftest_copy's figure taken in the same process (the project's ceiling for a streaming kernel);
  2. the same kernel beside the decode it follows (decompress_backbone + decompress_index + decompress_sidechain of the same batch);
  3. entries per second of FoldcompDatabase.tensor_batches(1024, sort_by_length=True) over a database of 350-residue chains beside
     the route through PDB text (foldcomp.open iteration, a numpy column parse into atom37, one upload per batch), and the largest
     coordinate difference between the two.

  4. the packed form (k_dense_packed) on the same two batches in the same process, right behind the padded call
     of every layout: same method, same group "dense", bytes per second beside the same copy figure, and packed over padded time.

  5. the windowed form (k_dense_window) on the mixed batch: atom37, L = 256, random starts (crop_starts with a
     seeded generator), right behind the L = 1 024 call of fcz_dense_dev in the same process: same method, same group "dense", and
     windowed over padded time beside the ratio of the bytes the two calls write.

    python tools/dense_bench.py --out profiles/dense_layout.json [--lib other/libfcz_hip.so label]
    python tools/dense_bench.py --skip-user-level --mixed-only --out profiles/dense_window.json
    python tools/dense_bench.py --skip-user-level --out profiles/dense_packed.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

ATOM37 = ["N", "CA", "C", "CB", "O", "CG", "CG1", "CG2", "OG", "OG1", "SG", "CD", "CD1", "CD2", "ND1", "ND2", "OD1", "OD2", "SD", "CE",
          "CE1", "CE2", "CE3", "NE", "NE1", "NE2", "OE1", "OE2", "CH2", "NH1", "NH2", "OH", "CZ", "CZ2", "CZ3", "NZ", "OXT"]
LAYOUTS = (("atom37", 0, 37), ("atom14", 1, 14), ("backbone4", 2, 4))


def kernel_case(codec, bench, name, n_chains, n_res, mixed, L_cap, dev, window_L=0):
    from foldcomp_amd import _lib, tensors
    from foldcomp_amd.structure import CDenseOut, CPackedOut
    d = bench.generate_resident(n_chains, n_res, 25, 32768, dev, seed_base=0, mixed=mixed)
    w = bench.Workload(codec, d, dev)
    w.compress(); codec.synchronize()
    del d
    lens = None
    res = {"case": name, "chains": n_chains, "layouts": {}}
    codec.enable_timing(True)
    decode = []
    for _ in range(3 + 9):
        codec.reset_timing()
        w.decompress(); codec.synchronize()
        decode.append(sum(codec.kernel_time(g)[0] for g in ("decompress_backbone", "decompress_index", "decompress_sidechain")))
    decode_ms = statistics.median(decode[3:])
    lens = np.diff(w.res_off_dev.cpu().numpy().view(np.uint32).astype(np.int64))
    L = int(min(lens.max(), L_cap))
    res.update(residues=int(lens.sum()), longest=int(lens.max()), L=L, decode_kernels_ms=decode_ms)
    for lname, lay, A in LAYOUTS:
        n = n_chains
        pos = torch.empty((n, L, A, 3), dtype=torch.float32, device=dev); mask = torch.empty((n, L, A), dtype=torch.uint8, device=dev)
        aatype = torch.empty((n, L), dtype=torch.uint8, device=dev); plddt = torch.empty((n, L), dtype=torch.float32, device=dev)
        res_index = torch.empty((n, L), dtype=torch.int32, device=dev); length = torch.empty(n, dtype=torch.int32, device=dev)
        out = CDenseOut(*(t.data_ptr() for t in (pos, mask, aatype, plddt, res_index, length)))
        torch.cuda.synchronize()
        ms = []
        for _ in range(3 + 9):
            codec.reset_timing()
            _lib.check(codec.lib.fcz_dense_dev(codec.ctx, w.blob_dev.data_ptr(), w.off_dev.data_ptr(), n, w.res_off_dev.data_ptr(),
                                               w.atom_off_dev.data_ptr(), ctypes.byref(w.cout), 0, lay, L, ctypes.byref(out)), "fcz_dense_dev")
            codec.synchronize()
            ms.append(codec.kernel_time("dense")[0])
        med = statistics.median(ms[3:])
        atoms = int(mask.sum(dtype=torch.int64))
        kept = int(np.minimum(lens, L).sum())
        written = n * L * (A * 13 + 9) + 4 * n
        read = 12 * atoms + 5 * kept + 8 * n
        res["layouts"][lname] = dict(dense_ms=med, dense_ms_min=min(ms[3:]), dense_ms_max=max(ms[3:]), bytes_written=written, bytes_read=read,
                                     gb_per_s=(written + read) / (med * 1e-3) / 1e9, padding_fraction=1.0 - kept / (n * L),
                                     share_of_decode_plus_dense=med / (med + decode_ms))
        del pos, mask, aatype, plddt, res_index, length
        torch.cuda.empty_cache()
        if window_L and lname == "atom37":
            # a window of window_L rows at a random start per entry, right behind the padded call
            Lw = int(window_L)
            gen = torch.Generator(device=dev); gen.manual_seed(1)
            start = tensors.crop_starts(torch.from_numpy(lens.astype(np.int32)).to(dev), Lw, "random", gen)
            wo = (torch.empty((n, Lw, A, 3), dtype=torch.float32, device=dev), torch.empty((n, Lw, A), dtype=torch.uint8, device=dev),
                  torch.empty((n, Lw), dtype=torch.uint8, device=dev), torch.empty((n, Lw), dtype=torch.float32, device=dev),
                  torch.empty((n, Lw), dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
            wout = CDenseOut(*(t.data_ptr() for t in wo))
            torch.cuda.synchronize()
            wms = []
            for _ in range(3 + 9):
                codec.reset_timing()
                _lib.check(codec.lib.fcz_dense_window_dev(codec.ctx, w.blob_dev.data_ptr(), w.off_dev.data_ptr(), n, w.res_off_dev.data_ptr(),
                                                          w.atom_off_dev.data_ptr(), ctypes.byref(w.cout), 0, lay, Lw, start.data_ptr(), ctypes.byref(wout)),
                           "fcz_dense_window_dev")
                codec.synchronize()
                wms.append(codec.kernel_time("dense")[0])
            wmed = statistics.median(wms[3:])
            st = start.cpu().numpy().astype(np.int64)
            kept_w = np.minimum(lens - st, Lw)
            w_kept = int(kept_w.sum())
            w_written = n * Lw * (A * 13 + 9) + 4 * n
            # (the prefix in front of a tile: one byte per residue in front of it, per tile that holds a residue)
            tiles = -(-kept_w // 64)
            w_prefix = int((st * tiles + 32 * tiles * (tiles - 1)).sum())
            w_read = 12 * int(wo[1].sum(dtype=torch.int64)) + 5 * w_kept + 12 * n + w_prefix
            res["layouts"][lname]["window"] = dict(L=Lw, dense_ms=wmed, dense_ms_min=min(wms[3:]), dense_ms_max=max(wms[3:]), bytes_written=w_written,
                                                   bytes_read=w_read, prefix_bytes_read=w_prefix, gb_per_s=(w_written + w_read) / (wmed * 1e-3) / 1e9,
                                                   padding_fraction=1.0 - w_kept / (n * Lw), entries_moved=int((st > 0).sum()),
                                                   time_over_padded=wmed / med, bytes_written_over_padded=w_written / written)
            del wo, start
            torch.cuda.empty_cache()
        # the packed form of the same batch: R rows, nothing cropped
        R = int(lens.sum())
        pk = (torch.empty((R, A, 3), dtype=torch.float32, device=dev), torch.empty((R, A), dtype=torch.uint8, device=dev),
              torch.empty(R, dtype=torch.uint8, device=dev), torch.empty(R, dtype=torch.float32, device=dev), torch.empty(R, dtype=torch.int32, device=dev),
              torch.empty(R, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
        pout = CPackedOut(*(t.data_ptr() for t in pk))
        torch.cuda.synchronize()
        pms = []
        for _ in range(3 + 9):
            codec.reset_timing()
            _lib.check(codec.lib.fcz_dense_packed_dev(codec.ctx, w.blob_dev.data_ptr(), w.off_dev.data_ptr(), n, w.res_off_dev.data_ptr(),
                                                      w.atom_off_dev.data_ptr(), ctypes.byref(w.cout), 0, lay, ctypes.byref(pout)), "fcz_dense_packed_dev")
            codec.synchronize()
            pms.append(codec.kernel_time("dense")[0])
        pmed = statistics.median(pms[3:])
        p_atoms = int(pk[1].sum(dtype=torch.int64))
        p_written = R * (A * 13 + 13) + 4 * n
        p_read = 12 * p_atoms + 5 * R + 8 * n
        padded = res["layouts"][lname]
        padded["packed"] = dict(dense_ms=pmed, dense_ms_min=min(pms[3:]), dense_ms_max=max(pms[3:]), rows=R, bytes_written=p_written, bytes_read=p_read,
                                gb_per_s=(p_written + p_read) / (pmed * 1e-3) / 1e9, time_over_padded=pmed / med,
                                padded_spread=(max(ms[3:]) - min(ms[3:])) / med)
        del pk
        torch.cuda.empty_cache()
    codec.enable_timing(False)
    del w
    torch.cuda.empty_cache()
    return res


def parse_atom37(pdb: str):
    """the PDB text of one entry -> (pos [n_res, 37, 3] float32, mask [n_res, 37]) by plain numpy column slices"""
    raw = pdb.encode("latin-1")
    a0 = raw.index(b"ATOM  ")
    a1 = raw.rindex(b"TER")
    rows = np.frombuffer(raw[a0:a1], np.uint8).reshape(-1, 81)
    def col(lo, hi, dt): return np.ascontiguousarray(rows[:, lo:hi]).view(f"S{hi - lo}")[:, 0].astype(dt)
    xyz = np.stack([col(30, 38, np.float32), col(38, 46, np.float32), col(46, 54, np.float32)], 1)
    name = np.char.strip(col(12, 16, "S4"))
    resn = col(22, 26, np.int64)
    slot = np.asarray([ATOM37.index(s.decode()) for s in name])
    is_oxt = slot == 36
    row = resn - resn[0]
    if is_oxt.any():
        row[is_oxt] = row[~is_oxt].max()
    n_res = int(row.max()) + 1
    pos = np.zeros((n_res, 37, 3), np.float32); mask = np.zeros((n_res, 37), np.uint8)
    pos[row, slot] = xyz; mask[row, slot] = 1
    return pos, mask


def user_level(codec, bench, n_entries, dev):
    import foldcomp
    from foldcomp_amd import api
    from foldcomp_amd.database import DatabaseWriter
    api.set_codec(codec)
    d = bench.generate_resident(n_entries, 350, 25, 32768, dev, seed_base=0)
    w = bench.Workload(codec, d, dev)
    w.compress(); codec.synchronize()
    blob = w.blob_dev.cpu().numpy(); off = w.off_dev.cpu().numpy()
    del w, d
    torch.cuda.empty_cache()
    out = {"entries": n_entries, "residues_per_entry": 350, "batch_size": 1024}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "db")
        wr = DatabaseWriter(path)
        for i in range(n_entries):
            wr.append(blob[int(off[i]):int(off[i + 1])].tobytes(), i, f"e{i}")
        wr.close()
        dense = {}
        for rep in range(2):                                  # the second pass is the measured one (first: allocator, page cache)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            with foldcomp.open(path) as db:
                for b in db.tensor_batches(1024, sort_by_length=True):
                    if rep == 1 and len(dense) < 2:
                        dense[int(b["index"][0])] = (b["pos"][0].cpu().numpy(), b["mask"][0].cpu().numpy())
            torch.cuda.synchronize(); t_new = time.perf_counter() - t0
        worst = 0.0
        for rep in range(1):
            t0 = time.perf_counter()
            with foldcomp.open(path) as db:
                batch = []
                for i, (name, pdb) in enumerate(db):
                    pos, mask = parse_atom37(pdb)
                    if i in dense:
                        m = dense[i][1][:len(mask)].astype(bool)
                        assert np.array_equal(m, mask.astype(bool))
                        worst = max(worst, float(np.abs(dense[i][0][:len(pos)].astype(np.float64) - pos)[m].max()))
                    batch.append((pos, mask))
                    if len(batch) == 1024 or i == len(db) - 1:
                        L = max(len(p) for p, _ in batch)
                        P = np.zeros((len(batch), L, 37, 3), np.float32); M = np.zeros((len(batch), L, 37), np.uint8)
                        for j, (p, m) in enumerate(batch):
                            P[j, :len(p)] = p; M[j, :len(m)] = m
                        tp, tm = torch.from_numpy(P).to(dev), torch.from_numpy(M).to(dev)
                        batch = []
            torch.cuda.synchronize(); t_old = time.perf_counter() - t0
    api.set_codec(None)
    out.update(tensor_batches_entries_per_s=n_entries / t_new, text_route_entries_per_s=n_entries / t_old,
               ratio=t_old / t_new, max_abs_coordinate_difference=worst, entries_compared=len(dense))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    ap.add_argument("--skip-user-level", action="store_true")
    ap.add_argument("--db-entries", type=int, default=20000)
    ap.add_argument("--mixed-chains", type=int, default=100000)
    ap.add_argument("--window-len", type=int, default=256, help="L of the windowed leg on the mixed batch (atom37, random starts); 0 leaves it out")
    ap.add_argument("--mixed-only", action="store_true", help="leave out the 65 536 x 350 case")
    ap.add_argument("--mixed-max-len", type=int, default=1024, help="L of the mixed batch (longer chains are cropped): 100 000 x 2 700 x 444 B does not fit")
    args = ap.parse_args()
    torch.cuda.init()
    dev = torch.device("cuda:0")
    import bench
    from foldcomp_amd import _lib
    from foldcomp_amd.codec import Codec
    codec = Codec(0)
    gbs = ctypes.c_double(0)
    _lib.check(codec.lib.fcz_selftest_copy(codec.ctx, ctypes.c_uint64(1 << 30), 10, ctypes.byref(gbs)), "fcz_selftest_copy")
    doc = {"label": args.label, "library": _lib.LIB_PATH if os.environ.get("FCZ_HIP_LIB") else "foldcomp_amd/libfcz_hip.so",
           "device": torch.cuda.get_device_name(0), "copy_ceiling_gb_per_s": gbs.value, "method": "HIP events on the ctx stream, median of 9 after 3 warm-up calls",
           "kernel": ([] if args.mixed_only else [kernel_case(codec, bench, "65536 x 350", 65536, 350, False, 1 << 30, dev)]) +
                     [kernel_case(codec, bench, f"{args.mixed_chains} mixed (L capped at {args.mixed_max_len})", args.mixed_chains, 0, True, args.mixed_max_len, dev,
                                  window_L=args.window_len)]}
    for c in doc["kernel"]:
        for v in c["layouts"].values():
            v["fraction_of_copy_ceiling"] = v["gb_per_s"] / gbs.value
            v["packed"]["fraction_of_copy_ceiling"] = v["packed"]["gb_per_s"] / gbs.value
            if "window" in v:
                v["window"]["fraction_of_copy_ceiling"] = v["window"]["gb_per_s"] / gbs.value
    if not args.skip_user_level:
        doc["user_level"] = user_level(codec, bench, args.db_entries, dev)
    codec.close()
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
