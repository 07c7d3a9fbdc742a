"""GPU: dense atom37 / atom14 / backbone4 tensors (fcz_dense_dev, fcz_decompress_dense, decode_tensors, tensor_batches) against
the reference's own float32 output. Every comparison of coordinates and pLDDT is on the bit patterns: the kernel moves floats and
computes none."""
import ctypes

import numpy as np
import pytest

import _dense as D
import _harness as H
from _cases import db_cases, entries_blob, golden_records_raw
from _devpath import DevRecords
from foldcomp_amd import _lib, fczfile
from foldcomp_amd._aa_tables import ATOM_NAMES, RES3, RES_NATOMS
from foldcomp_amd.structure import CAtomsOut, CDenseOut

pytestmark = pytest.mark.gpu

KEYS = ("pos", "mask", "aatype", "plddt", "res_index", "length")
FILL = 0xA5


def raw_bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint8) if a.dtype == np.bool_ else a


def same(got, exp, what=""):
    """two dense dicts equal, floats by bit pattern"""
    for k in KEYS:
        if k not in exp:
            continue
        g, e = raw_bits(got[k]), raw_bits(exp[k])
        assert g.shape == e.shape, (what, k, g.shape, e.shape)
        assert np.array_equal(g.astype(np.int64), e.astype(np.int64)), (what, k, np.argwhere(g.astype(np.int64) != e.astype(np.int64))[:4])


def dense_dev(codec, entries, layout, L, alt_order=False, want=KEYS):
    """fcz_decompress_sizes_dev + fcz_decompress_batch_dev (in the given atom order) + fcz_dense_dev on arrays pre-filled with 0xA5
    bytes (every byte that comes back as specified was written by the kernel) -> dict of host arrays"""
    import torch
    blob, off = entries_blob(entries)
    rec = DevRecords(blob, off)
    rec.sizes(codec)
    atoms = rec.batch(codec, alt_order=alt_order, host=False)
    n, A = len(entries), D.WIDTH[layout]
    shape = dict(pos=(n, L, A, 3), mask=(n, L, A), aatype=(n, L), plddt=(n, L), res_index=(n, L), length=(n,))
    dt = dict(pos=np.float32, mask=np.uint8, aatype=np.uint8, plddt=np.float32, res_index=np.int32, length=np.uint32)
    nbytes = {k: int(np.prod(shape[k])) * np.dtype(dt[k]).itemsize for k in want}
    raw = {k: torch.full((max(nbytes[k], 1),), FILL, dtype=torch.uint8, device="cuda:0") for k in want}
    at = CAtomsOut(*(atoms[k].data_ptr() for k in ("x", "y", "z", "bfac_res", "res_code")), None)
    out = CDenseOut(*(raw[k].data_ptr() if k in raw else None for k in KEYS))
    torch.cuda.synchronize()
    _lib.check(codec.lib.fcz_dense_dev(codec.ctx, rec.blob_t.data_ptr(), rec.off_t.data_ptr(), n, rec.res_off_t.data_ptr(),
                                       rec.atom_off_t.data_ptr(), ctypes.byref(at), int(alt_order), D.LAYOUTS[layout], L, ctypes.byref(out)),
               "fcz_dense_dev")
    codec.synchronize()
    return {k: raw[k].cpu().numpy()[:nbytes[k]].view(dt[k]).reshape(shape[k]) for k in want}


@pytest.fixture(scope="module")
def records(golden):
    return golden_records_raw(golden)


@pytest.fixture(scope="module")
def flat(codec, records):
    blob, off = entries_blob(records[1])
    return codec.decompress_batch(blob, off)


def golden_expected(golden, records, flat, layout, L):
    z, _ = golden
    per = []
    for i, (nm, fcz) in enumerate(zip(*records)):
        seq, first, has_oxt = D.record_fields(fcz)
        r0 = int(flat["res_off"][i])
        per.append(D.dense_expected(z[f"{nm}/xyz0"], seq, first, has_oxt, layout, L, plddt=flat["bfac_res"][r0:r0 + len(seq)]))
    return D.stack_expected(per, L, D.WIDTH[layout])


@pytest.mark.parametrize("layout", list(D.LAYOUTS))
def test_golden_batch_matches_the_reference_output(codec, golden, records, flat, layout):
    z, _ = golden
    names, entries = records
    L = max(fczfile.residue_count(e) for e in entries)
    assert L == 1400
    exp = golden_expected(golden, records, flat, layout, L)
    got = dense_dev(codec, entries, layout, L)
    same(got, exp, layout)
    assert not got["pos"][got["mask"] == 0].view(np.uint32).any()
    # residue numbers of the reference's own ATOM records (columns 23-26)
    for i, nm in enumerate(names):
        nums = D.pdb_residue_numbers(z[f"{nm}/pdb0"].tobytes())
        assert list(got["res_index"][i, :len(nums)]) == nums and not got["res_index"][i, len(nums):].any(), nm
        assert got["length"][i] == len(nums)
    # the atoms decoded in the `-a` order give the same tensors
    same(dense_dev(codec, entries, layout, L, alt_order=True), got, layout + " alt")
    # the host convenience call (with its sizing call)
    host = codec.decompress_dense(*entries_blob(entries), layout=layout)
    assert host["pos"].shape == (56, L, D.WIDTH[layout], 3) and host["mask"].dtype == np.bool_ and not host["status"].any()
    same(host, got, layout + " host")
    # the live reference, atoms placed by the names it returns (this leg alone depends on oracle/_ref)
    if H.have_ref():
        for i, fcz in enumerate(entries):
            r = H.ref_decompress(fcz)
            pos = np.zeros((L, D.WIDTH[layout], 3), np.float32); mask = np.zeros((L, D.WIDTH[layout]), np.uint8)
            first = int(r["res_index"][0])
            for a, (an, rn, ri) in enumerate(zip(r["atom"], r["residue"], r["res_index"])):
                l = int(got["length"][i]) - 1 if an == "OXT" else int(ri) - first     # (the reference numbers the OXT header.nResidue)
                s = D.expected_slot(layout, RES3.index(rn), ATOM_NAMES.index(an))
                if s >= 0:
                    pos[l, s] = (r["x"][a], r["y"][a], r["z"][a]); mask[l, s] = 1
            assert np.array_equal(got["pos"][i].view(np.uint32), pos.view(np.uint32)), names[i]
            assert np.array_equal(got["mask"][i], mask), names[i]


def test_crop_and_pad(codec, golden, records, flat):
    names, entries = records
    full = dense_dev(codec, entries, "atom37", 1400)
    crop = dense_dev(codec, entries, "atom37", 64)
    same(crop, golden_expected(golden, records, flat, "atom37", 64), "crop")
    # rows = the first 64 residues of the uncropped result (the OXT of a longer entry lies behind them), length uncropped
    for k in ("pos", "mask", "aatype", "plddt", "res_index"):
        assert np.array_equal(raw_bits(crop[k]), raw_bits(full[k][:, :64])), k
    cropped = full["length"] > 64
    assert cropped.any() and (~cropped).any() and np.array_equal(crop["length"], full["length"]) and full["length"].max() == 1400
    assert not crop["mask"][cropped][:, :, 36].any()                            # no OXT in a cropped entry
    assert full["mask"][:, :, 36].sum() == 27
    pad = dense_dev(codec, entries, "atom37", 1437)
    same(pad, golden_expected(golden, records, flat, "atom37", 1437), "pad")
    for k in ("pos", "mask", "aatype", "plddt", "res_index"):
        assert np.array_equal(raw_bits(pad[k][:, :1400]), raw_bits(full[k])), k
    assert not pad["mask"][:, 1400:].any() and (pad["aatype"][:, 1400:] == 20).all()
    # optional outputs left out: the required ones are unchanged
    two = dense_dev(codec, entries, "atom14", 200, want=("pos", "mask"))
    same(two, {k: v for k, v in golden_expected(golden, records, flat, "atom14", 200).items() if k in ("pos", "mask")}, "pos+mask only")


def test_damaged_records_between_good_ones(codec, records):
    names, entries = records
    good = entries[:6]
    ref = dense_dev(codec, good, "atom37", 300)
    bad_magic = b"XXXX" + good[1][4:]
    truncated = good[2][:100]
    mixed = [good[0], bad_magic, good[1], truncated, good[2], good[3], good[4], good[5]]
    got = dense_dev(codec, mixed, "atom37", 300)
    at = [0, 2, 4, 5, 6, 7]
    for k in KEYS:
        assert np.array_equal(raw_bits(got[k][at]), raw_bits(ref[k])), k
    for i in (1, 3):
        assert got["length"][i] == 0 and not got["mask"][i].any() and not got["pos"][i].view(np.uint32).any()
        assert (got["aatype"][i] == 20).all() and not got["plddt"][i].view(np.uint32).any() and not got["res_index"][i].any()
    host = codec.decompress_dense(*entries_blob(mixed), max_len=300)
    assert list(host["status"]) == [0, -4, 0, -5, 0, 0, 0, 0]
    same(host, got, "host")


def scatter_expected(lib, d, layout, L):
    """Codec.decompress_batch output (canonical order) scattered by fcz_dense_slot in numpy"""
    lay, A = D.LAYOUTS[layout], D.WIDTH[layout]
    n = len(d["res_off"]) - 1
    table = np.full((24, 256), -1, np.int64)
    for rc in range(24):
        for code in range(37):
            table[rc, code] = lib.fcz_dense_slot(lay, rc, code)
    pos = np.zeros((n, L, A, 3), np.float32); mask = np.zeros((n, L, A), np.uint8)
    res_off = d["res_off"].astype(np.int64)
    lens = np.diff(res_off)
    natoms = np.asarray(RES_NATOMS, np.int64)[d["res_code"]]
    res_of_atom = np.repeat(np.arange(len(natoms)), natoms)
    ent_of_res = np.repeat(np.arange(n), lens)
    row_of_res = np.arange(len(natoms)) - res_off[ent_of_res]
    xyz = np.stack([d["x"], d["y"], d["z"]], 1)
    oxt = d["atom_code"] == 36
    body = np.flatnonzero(~oxt)
    assert len(body) == len(res_of_atom)
    slot = table[d["res_code"][res_of_atom], d["atom_code"][body]]
    e, l = ent_of_res[res_of_atom], row_of_res[res_of_atom]
    ok = (slot >= 0) & (l < L)
    pos[e[ok], l[ok], slot[ok]] = xyz[body][ok]; mask[e[ok], l[ok], slot[ok]] = 1
    if layout == "atom37":
        for a in np.flatnonzero(oxt):
            ee = int(np.searchsorted(d["atom_off"], a, side="right") - 1)
            if lens[ee] <= L:
                pos[ee, lens[ee] - 1, 36] = xyz[a]; mask[ee, lens[ee] - 1, 36] = 1
    aatype = np.full((n, L), 20, np.uint8); plddt = np.zeros((n, L), np.float32)
    okr = row_of_res < L
    aatype[ent_of_res[okr], row_of_res[okr]] = np.minimum(d["res_code"], 20)[okr]
    plddt[ent_of_res[okr], row_of_res[okr]] = d["bfac_res"][okr]
    return dict(pos=pos, mask=mask, aatype=aatype, plddt=plddt, length=lens.astype(np.uint32))


def test_synthetic_mixed_batch_both_numerics(codec):
    from foldcomp_amd import synthetic
    lens = np.concatenate([np.minimum(synthetic.mixed_lengths(2800, seed=11), 1200), 2 + np.arange(200) % 16])
    assert len(lens) == 3000 and lens.min() == 2 and lens.max() <= 1200
    b = synthetic.to_chain_batch(synthetic.generate(len(lens), lens, seed=5))
    trp = synthetic.to_chain_batch(synthetic.generate(96, [64, 65, 300] * 32, seed=6, res_code=17))
    lib = _lib.load()
    for batch, L, layouts in ((b, 512, ("atom37", "atom14", "backbone4")), (trp, 300, ("atom37", "atom14"))):
        blob, off, st = codec.compress_batch(batch)
        assert not st.any()
        entries = [blob[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(off) - 1)]
        try:
            for fast in (False, True):
                codec.set_numerics(fast)
                d = codec.decompress_batch(blob, off)
                for layout in layouts:
                    got = dense_dev(codec, entries, layout, L, want=("pos", "mask", "aatype", "plddt", "length"))
                    same(got, scatter_expected(lib, d, layout, L), f"{layout} fast={fast}")
        finally:
            codec.set_numerics(False)


def test_index_beyond_32_bits(codec, records):
    """one call whose pos holds more than 2^32 floats (64-bit indexing, include/fcz_hip.h): 16 entries, L = 2 500 000"""
    import torch
    entries = records[1][:16]
    n, L, A = 16, 2_500_000, 37
    assert n * L * A * 3 > 2 ** 32
    small_L = max(fczfile.residue_count(e) for e in entries)
    small = dense_dev(codec, entries, "atom37", small_L)
    blob, off = entries_blob(entries)
    rec = DevRecords(blob, off)
    rec.sizes(codec)
    atoms = rec.batch(codec, host=False)
    pos = torch.full((n, L, A, 3), float("nan"), dtype=torch.float32, device="cuda:0")
    mask = torch.full((n, L, A), FILL, dtype=torch.uint8, device="cuda:0")
    aatype = torch.full((n, L), FILL, dtype=torch.uint8, device="cuda:0")
    at = CAtomsOut(*(atoms[k].data_ptr() for k in ("x", "y", "z", "bfac_res", "res_code")), None)
    out = CDenseOut(pos.data_ptr(), mask.data_ptr(), aatype.data_ptr(), None, None, None)
    torch.cuda.synchronize()
    _lib.check(codec.lib.fcz_dense_dev(codec.ctx, rec.blob_t.data_ptr(), rec.off_t.data_ptr(), n, rec.res_off_t.data_ptr(),
                                       rec.atom_off_t.data_ptr(), ctypes.byref(at), 0, 0, L, ctypes.byref(out)), "fcz_dense_dev")
    codec.synchronize()
    assert np.array_equal(pos[:, :small_L].cpu().numpy().view(np.uint32), small["pos"].view(np.uint32))
    assert np.array_equal(mask[:, :small_L].cpu().numpy(), small["mask"])
    assert np.array_equal(aatype[:, :small_L].cpu().numpy(), small["aatype"])
    # padding: right behind the residues, the middle, the last row; around the 2^32-th float; the very last elements
    flat_pos, flat_mask = pos.view(-1), mask.view(-1)
    for e in (0, 7, 15):
        for l in (small_L, small_L + 1, L // 2, L - 1):
            assert not pos[e, l].cpu().numpy().view(np.uint32).any() and not mask[e, l].any().item() and aatype[e, l].item() == 20
    # (the middle of the flat arrays is where entry 8 starts: the 64 elements in front of it are the end of entry 7's padding)
    for lo in (2 ** 32 - 64, 2 ** 32, flat_pos.numel() // 2 - 64, flat_pos.numel() - 64):
        assert not flat_pos[lo:lo + 64].cpu().numpy().view(np.uint32).any(), lo
    assert not flat_mask[-64:].any().item() and not flat_mask[flat_mask.numel() // 2 - 64:flat_mask.numel() // 2].any().item()
    # every element behind the residues, in reductions on the device
    assert int(torch.count_nonzero(pos[15, small_L:].view(torch.int32)).item()) == 0
    assert int(torch.count_nonzero(mask[:, small_L:]).item()) == 0
    del pos, mask, aatype, flat_pos, flat_mask
    torch.cuda.empty_cache()


def test_decode_tensors(codec, records):
    import torch
    import foldcomp
    from foldcomp_amd import api
    names, entries = records
    api.set_codec(codec)
    try:
        titles = [foldcomp.decompress(e)[0] for e in entries]
        for layout in D.LAYOUTS:
            t = foldcomp.decode_tensors(entries, layout=layout)
            host = codec.decompress_dense(*entries_blob(entries), layout=layout)
            A = D.WIDTH[layout]
            want = dict(pos=((56, 1400, A, 3), torch.float32), mask=((56, 1400, A), torch.bool), aatype=((56, 1400), torch.uint8),
                        plddt=((56, 1400), torch.float32), res_index=((56, 1400), torch.int32), length=((56,), torch.int32))
            for k, (shape, dtype) in want.items():
                assert t[k].device == torch.device("cuda:0") and tuple(t[k].shape) == shape and t[k].dtype == dtype, k
            same({k: t[k].cpu().numpy() for k in want}, host, layout)
            assert t["names"] == titles
        t = foldcomp.decode_tensors(entries[:5], max_len=100, codec=codec)
        assert tuple(t["pos"].shape) == (5, 100, 37, 3)
        assert foldcomp.decode_tensors([], codec=codec)["pos"].shape[0] == 0
        with pytest.raises(foldcomp.error):
            foldcomp.decode_tensors(entries[:1], device="cpu")
        with pytest.raises(ValueError):
            foldcomp.decode_tensors(entries[:1], layout="atom38")
    finally:
        api.set_codec(None)


def test_tensor_batches(codec, golden, tmp_path, capsys):
    import torch
    import foldcomp
    from foldcomp_amd import api
    from foldcomp_amd.database import DatabaseWriter
    z, index = golden
    names = db_cases(index)
    assert len(names) == 24
    path = str(tmp_path / "db")
    w = DatabaseWriter(path)
    entries = [z[f"{n}/fcz"].tobytes() for n in names]
    lookup = [f"entry_{k:02d}" for k in range(24)]
    for k, (e, nm) in enumerate(zip(entries, lookup)):
        w.append(e, k, nm)
    w.close()

    def teq(a, b):
        if a.dtype == torch.float32:
            a, b = a.view(torch.int32), b.view(torch.int32)
        return bool((a == b).all())

    api.set_codec(codec)
    try:
        whole = foldcomp.decode_tensors(entries)
        picked = [17, 3, 3, 20, 0, 9]
        for use_ids in (None, [lookup[k] for k in picked]):
            sel = list(range(24)) if use_ids is None else picked
            for bs in (1, 5, 1024):
                for sort in (False, True):
                    with foldcomp.open(path, ids=use_ids) as db:
                        seen, n_batches = [], 0
                        for d in db.tensor_batches(bs, sort_by_length=sort):
                            n_batches += 1
                            assert len(d["index"]) == len(d["names"]) == d["pos"].shape[0] <= bs
                            lens = d["length"].cpu().numpy()
                            assert d["pos"].shape[1] == lens.max()
                            if sort:
                                assert list(lens) == sorted(lens)
                            for j, i in enumerate(d["index"]):
                                k, L = sel[int(i)], int(lens[j])
                                assert L == int(whole["length"][k]) and d["names"][j] == whole["names"][k]
                                for key in ("pos", "mask", "aatype", "plddt", "res_index"):
                                    assert teq(d[key][j, :L], whole[key][k, :L]), (key, k)
                                for key in ("pos", "mask", "plddt", "res_index"):
                                    assert not bool(d[key][j, L:].any()), (key, k)
                                assert bool((d["aatype"][j, L:] == 20).all())
                                seen.append(int(i))
                        assert sorted(seen) == list(range(len(sel))) and n_batches == -(-len(sel) // bs)
                        if not sort:
                            assert seen == list(range(len(sel)))
        # a missing id behaves as open() does: skipped with a message, or KeyError on request
        capsys.readouterr()
        with foldcomp.open(path, ids=[lookup[2], "no_such_entry"]) as db:
            got = list(db.tensor_batches(4))
        assert "no_such_entry" in capsys.readouterr().err and len(got) == 1 and list(got[0]["index"]) == [0]
        assert teq(got[0]["pos"][0, :int(whole["length"][2])], whole["pos"][2, :int(whole["length"][2])])
        with pytest.raises(KeyError):
            foldcomp.open(path, ids=["no_such_entry"], err_on_missing=True)
    finally:
        api.set_codec(None)
