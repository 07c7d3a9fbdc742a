"""GPU: packed dense tensors (fcz_dense_packed_dev, fcz_decompress_dense_packed, decode_tensors(packed=True),
tensor_batches(packed=True, max_residues=...)): the rows of all entries back to back, no padding. The expectation is the per-entry
reference expectation of tests/_dense.py concatenated in entry order; coordinates and pLDDT are compared by bit pattern. Every
output array is pre-filled with 0xA5 bytes and carries one guard row in front and one behind: every byte inside must have been
written, none outside."""
import ctypes

import numpy as np
import pytest

import _dense as D
from _cases import db_cases, entries_blob, golden_records_raw
from _devpath import DevRecords
from foldcomp_amd import _lib, fczfile
from foldcomp_amd.structure import CAtomsOut, CDenseOut, CPackedOut

pytestmark = pytest.mark.gpu

KEYS = ("pos", "mask", "aatype", "plddt", "res_index", "chain_index", "length")
ROW_KEYS = KEYS[:6]
DT = dict(pos=np.float32, mask=np.uint8, aatype=np.uint8, plddt=np.float32, res_index=np.int32, chain_index=np.int32, length=np.uint32)
FILL = 0xA5


def row_bytes(k, A):
    return dict(pos=12 * A, mask=A, aatype=1, plddt=4, res_index=4, chain_index=4, length=4)[k]


def raw_bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint8) if a.dtype == np.bool_ else a


def same(got, exp, what="", keys=KEYS):
    for k in keys:
        if k not in exp or k not in got:
            continue
        g, e = raw_bits(got[k]).astype(np.int64), raw_bits(exp[k]).astype(np.int64)
        assert g.shape == e.shape, (what, k, g.shape, e.shape)
        assert np.array_equal(g, e), (what, k, np.argwhere(g != e)[:4])


def packed_dev(codec, entries, layout, alt_order=False, want=KEYS):
    """sizes + decode (in the given atom order) + fcz_dense_packed_dev into guarded, 0xA5-filled arrays -> (dict of host arrays,
    res_off); asserts that both guard rows of every array still hold the fill"""
    import torch
    blob, off = entries_blob(entries)
    n, A = len(entries), D.WIDTH[layout]
    if n == 0:
        blob, off = np.zeros(16, np.uint8), np.zeros(1, np.uint64)
    rec = DevRecords(blob, off)
    ro, _ = rec.sizes(codec)
    R = int(ro[-1])
    atoms = rec.batch(codec, alt_order=alt_order, host=False) if R else None
    rows = {k: (n if k == "length" else R) for k in want}
    raw = {k: torch.full(((rows[k] + 2) * row_bytes(k, A),), FILL, dtype=torch.uint8, device="cuda:0") for k in want}
    if atoms is None:
        atoms = {k: torch.zeros(4, dtype=torch.float32 if k != "res_code" else torch.uint8, device="cuda:0") for k in ("x", "y", "z", "bfac_res", "res_code")}
    at = CAtomsOut(*(atoms[k].data_ptr() for k in ("x", "y", "z", "bfac_res", "res_code")), None)
    out = CPackedOut(*(raw[k].data_ptr() + row_bytes(k, A) if k in raw else None for k in KEYS))
    torch.cuda.synchronize()
    _lib.check(codec.lib.fcz_dense_packed_dev(codec.ctx, rec.blob_t.data_ptr(), rec.off_t.data_ptr(), n, rec.res_off_t.data_ptr(),
                                              rec.atom_off_t.data_ptr(), ctypes.byref(at), int(alt_order), D.LAYOUTS[layout], ctypes.byref(out)),
               "fcz_dense_packed_dev")
    codec.synchronize()
    got = {}
    for k in want:
        h, rb = raw[k].cpu().numpy(), row_bytes(k, A)
        assert (h[:rb] == FILL).all() and (h[len(h) - rb:] == FILL).all(), (k, "guard row written")
        body = h[rb:len(h) - rb].view(DT[k])
        got[k] = body.reshape(dict(pos=(R, A, 3), mask=(R, A)).get(k, (rows[k],)))
    return got, ro


def padded_dev(codec, entries, layout, L):
    """the padded call on the same records (fcz_dense_dev) -> dict of host arrays"""
    import torch
    rec = DevRecords(*entries_blob(entries))
    rec.sizes(codec)
    atoms = rec.batch(codec, host=False)
    n, A = len(entries), D.WIDTH[layout]
    t = dict(pos=torch.empty((n, L, A, 3), dtype=torch.float32, device="cuda:0"), mask=torch.empty((n, L, A), dtype=torch.uint8, device="cuda:0"),
             aatype=torch.empty((n, L), dtype=torch.uint8, device="cuda:0"), plddt=torch.empty((n, L), dtype=torch.float32, device="cuda:0"),
             res_index=torch.empty((n, L), dtype=torch.int32, device="cuda:0"), length=torch.empty(n, dtype=torch.int32, device="cuda:0"))
    at = CAtomsOut(*(atoms[k].data_ptr() for k in ("x", "y", "z", "bfac_res", "res_code")), None)
    out = CDenseOut(*(t[k].data_ptr() for k in ("pos", "mask", "aatype", "plddt", "res_index", "length")))
    torch.cuda.synchronize()
    _lib.check(codec.lib.fcz_dense_dev(codec.ctx, rec.blob_t.data_ptr(), rec.off_t.data_ptr(), n, rec.res_off_t.data_ptr(), rec.atom_off_t.data_ptr(),
                                       ctypes.byref(at), 0, D.LAYOUTS[layout], L, ctypes.byref(out)), "fcz_dense_dev")
    codec.synchronize()
    return {k: v.cpu().numpy() for k, v in t.items()}


@pytest.fixture(scope="module")
def records(golden):
    return golden_records_raw(golden)


@pytest.fixture(scope="module")
def per_entry(codec, golden, records):
    """the reference expectation of every golden record, per layout, unpadded (L = its own length): computed once, never changed"""
    z, _ = golden
    names, entries = records
    flat = codec.decompress_batch(*entries_blob(entries))
    exp = {}
    for layout in D.LAYOUTS:
        for i, (nm, fcz) in enumerate(zip(names, entries)):
            seq, first, has_oxt = D.record_fields(fcz)
            r0 = int(flat["res_off"][i])
            exp[layout, i] = D.dense_expected(z[f"{nm}/xyz0"], seq, first, has_oxt, layout, len(seq), plddt=flat["bfac_res"][r0:r0 + len(seq)])
    return exp


def concat_expected(per_entry, layout, picks):
    """picks: golden record numbers in batch order, None = an entry that does not decode (no row)"""
    A = D.WIDTH[layout]
    parts = [per_entry[layout, i] for i in picks if i is not None]
    d = {k: (np.concatenate([p[k] for p in parts]) if parts else np.zeros((0,) + dict(pos=(A, 3), mask=(A,)).get(k, ()), DT[k]))
         for k in ("pos", "mask", "aatype", "plddt", "res_index")}
    lens = [0 if i is None else per_entry[layout, i]["length"] for i in picks]
    d["length"] = np.asarray(lens, np.uint32)
    d["chain_index"] = np.repeat(np.arange(len(picks)), lens).astype(np.int32)
    return d


@pytest.mark.parametrize("layout", list(D.LAYOUTS))
def test_golden_batch_matches_the_concatenated_reference(codec, records, per_entry, layout):
    names, entries = records
    exp = concat_expected(per_entry, layout, range(56))
    for alt in (False, True):
        got, ro = packed_dev(codec, entries, layout, alt_order=alt)
        assert np.array_equal(ro, np.concatenate([[0], np.cumsum(exp["length"])]))
        same(got, exp, f"{layout} alt={alt}")
        assert not got["pos"][got["mask"] == 0].view(np.uint32).any()
    # optional outputs passed as NULL: the others are unchanged
    for want in (("pos", "mask"), ("pos", "mask", "chain_index"), ("pos", "mask", "aatype", "length"), ("pos", "mask", "plddt", "res_index")):
        part, _ = packed_dev(codec, entries, layout, want=want)
        assert set(part) == set(want)
        same(part, exp, f"{layout} {want}")
    # the host convenience call with its sizing call
    host = codec.decompress_dense(*entries_blob(entries), layout=layout, packed=True)
    assert host["mask"].dtype == np.bool_ and not host["status"].any() and np.array_equal(host["row_off"], ro)
    same(host, exp, layout + " host")


def synthetic_records(codec):
    """a few hundred synthetic chains: mixed lengths, every length 2 .. 17, the tile sizes and their neighbours, all-TRP chains"""
    from foldcomp_amd import synthetic
    lens = np.concatenate([np.minimum(synthetic.mixed_lengths(200, seed=11), 700), 2 + np.arange(16), [63, 64, 65, 127, 128, 129]])
    assert lens.min() == 2 and len(lens) == 222
    out = []
    for b in (synthetic.to_chain_batch(synthetic.generate(len(lens), lens, seed=5)),
              synthetic.to_chain_batch(synthetic.generate(12, [64, 65, 300] * 4, seed=6, res_code=17))):
        blob, off, st = codec.compress_batch(b)
        assert not st.any()
        out += [blob[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(off) - 1)]
    return out


def test_same_rows_as_the_padded_call_both_numerics(codec):
    entries = synthetic_records(codec)
    L = max(fczfile.residue_count(e) for e in entries)
    try:
        for fast in (False, True):
            codec.set_numerics(fast)
            for layout in ("atom37", "atom14", "backbone4"):
                pad = padded_dev(codec, entries, layout, L)
                got, ro = packed_dev(codec, entries, layout)
                lens = pad["length"].astype(np.int64)
                assert np.array_equal(got["length"], pad["length"].view(np.uint32)) and np.array_equal(np.diff(ro.astype(np.int64)), lens)
                keep = np.arange(L)[None, :] < lens[:, None]                      # [n, L] rows that hold a residue, in entry order
                for k in ("pos", "mask", "aatype", "plddt", "res_index"):
                    assert np.array_equal(raw_bits(got[k]), raw_bits(pad[k])[keep]), (layout, fast, k)
                assert np.array_equal(got["chain_index"], np.repeat(np.arange(len(entries)), lens))
    finally:
        codec.set_numerics(False)


def test_entry_boundaries_and_oxts_inside_a_tile(codec, records, per_entry):
    names, entries = records
    with_oxt = [i for i, e in enumerate(entries) if D.record_fields(e)[2]]
    short = min(with_oxt, key=lambda i: fczfile.residue_count(entries[i]))
    s = fczfile.residue_count(entries[short])
    assert s < 64                                                                 # several chain ends per 64-row tile
    picks = [short] * 131
    got, _ = packed_dev(codec, [entries[i] for i in picks], "atom37")
    exp = concat_expected(per_entry, "atom37", picks)
    assert exp["mask"][:, 36].sum() == 131
    same(got, exp, "copies of the shortest record with an OXT")
    # mixed with long records: 64 copies put a boundary exactly on a multiple of 64 rows, the long ones span many tiles
    longest = max(range(56), key=lambda i: fczfile.residue_count(entries[i]))
    other = max(with_oxt, key=lambda i: fczfile.residue_count(entries[i]))
    picks = [short] * 64 + [longest] + [short] * 3 + [other] + [short] * 64 + [other, longest, short]
    bounds = np.cumsum([fczfile.residue_count(entries[i]) for i in picks])
    assert bounds[63] % 64 == 0
    for layout in D.LAYOUTS:
        got, ro = packed_dev(codec, [entries[i] for i in picks], layout)
        assert np.array_equal(ro[1:], bounds)
        same(got, concat_expected(per_entry, layout, picks), "mixed " + layout)


def test_zero_row_entries(codec, records, per_entry):
    names, entries = records
    bad_magic = b"XXXX" + entries[1][4:]
    truncated = entries[2][:100]
    batch = [bad_magic, entries[0], entries[1], truncated, bad_magic, entries[2], entries[3], truncated]
    picks = [None, 0, 1, None, None, 2, 3, None]
    for layout in ("atom37", "atom14"):
        got, ro = packed_dev(codec, batch, layout)
        exp = concat_expected(per_entry, layout, picks)
        same(got, exp, "damaged first, last and two adjacent")
        assert list(got["length"][[0, 3, 4, 7]]) == [0, 0, 0, 0] and ro[0] == ro[1] and ro[3] == ro[4] == ro[5] and ro[7] == ro[8]
    host = codec.decompress_dense(*entries_blob(batch), packed=True)
    assert list(host["status"]) == [-4, 0, 0, -5, -4, 0, 0, -5]
    same(host, concat_expected(per_entry, "atom37", picks), "host")
    # nothing decodes: no row is written (the guard rows are adjacent), length is zeros
    got, ro = packed_dev(codec, [bad_magic, truncated, bad_magic], "atom37")
    assert not ro.any() and got["pos"].shape == (0, 37, 3) and list(got["length"]) == [0, 0, 0]
    host = codec.decompress_dense(*entries_blob([bad_magic, truncated]), packed=True)
    assert host["pos"].shape == (0, 37, 3) and list(host["length"]) == [0, 0] and list(host["row_off"]) == [0, 0, 0]
    # no entries
    got, ro = packed_dev(codec, [], "atom37")
    assert got["pos"].shape == (0, 37, 3) and got["length"].shape == (0,)
    host = codec.decompress_dense(np.zeros(0, np.uint8), np.zeros(1, np.uint64), packed=True)
    assert host["pos"].shape == (0, 37, 3) and list(host["row_off"]) == [0]


def test_index_beyond_32_bits(codec, records):
    """one call whose pos holds more than 2^32 floats (every index is 64-bit, include/fcz_hip.h): copies of the longest golden
    record, atom37; every copy's block of rows equals the single-record result, compared on the device as int32"""
    import torch
    names, entries = records
    e = max(entries, key=fczfile.residue_count)
    ne, A = fczfile.residue_count(e), 37
    c = 2 ** 32 // (ne * A * 3) + 2
    assert c * ne * A * 3 > 2 ** 32 and (c - 1) * ne * A * 3 > 2 ** 32
    one, _ = packed_dev(codec, [e], "atom37", want=("pos", "mask", "chain_index"))
    rec = DevRecords(np.tile(np.frombuffer(e, np.uint8), c), np.arange(c + 1, dtype=np.uint64) * len(e))
    ro, _ = rec.sizes(codec)
    R = c * ne
    assert int(ro[-1]) == R
    atoms = rec.batch(codec, host=False)
    pos = torch.full((R + 2, A, 3), float("nan"), dtype=torch.float32, device="cuda:0")
    mask = torch.full((R + 2, A), FILL, dtype=torch.uint8, device="cuda:0")
    chain = torch.full((R + 2,), -7, dtype=torch.int32, device="cuda:0")
    at = CAtomsOut(*(atoms[k].data_ptr() for k in ("x", "y", "z", "bfac_res", "res_code")), None)
    out = CPackedOut(pos[1:].data_ptr(), mask[1:].data_ptr(), None, None, None, chain[1:].data_ptr(), None)
    torch.cuda.synchronize()
    _lib.check(codec.lib.fcz_dense_packed_dev(codec.ctx, rec.blob_t.data_ptr(), rec.off_t.data_ptr(), c, rec.res_off_t.data_ptr(),
                                              rec.atom_off_t.data_ptr(), ctypes.byref(at), 0, 0, ctypes.byref(out)), "fcz_dense_packed_dev")
    codec.synchronize()
    want_pos = torch.from_numpy(one["pos"].view(np.int32)).to("cuda:0")
    want_mask = torch.from_numpy(one["mask"]).to("cuda:0")
    pv, mv = pos[1:R + 1].view(torch.int32).view(c, ne, A, 3), mask[1:R + 1].view(c, ne, A)
    for lo in range(0, c, 2048):
        assert bool((pv[lo:lo + 2048] == want_pos).all()), lo
        assert bool((mv[lo:lo + 2048] == want_mask).all()), lo
    assert bool((chain[1:R + 1].view(c, ne) == torch.arange(c, dtype=torch.int32, device="cuda:0")[:, None]).all())
    # the guard rows, in front and behind (the one behind lies beyond the 2^32-th float)
    for g in (0, R + 1):
        assert bool(torch.isnan(pos[g]).all()) and bool((mask[g] == FILL).all()) and int(chain[g]) == -7
    del pos, mask, chain, pv, mv, atoms, rec
    torch.cuda.empty_cache()


def test_decode_tensors_packed(codec, records, per_entry):
    import torch
    import foldcomp
    from foldcomp_amd import api
    names, entries = records
    api.set_codec(codec)
    try:
        titles = [fczfile.parse(e).title for e in entries]
        for layout in D.LAYOUTS:
            t = foldcomp.decode_tensors(entries, layout=layout, packed=True)
            A, exp = D.WIDTH[layout], concat_expected(per_entry, layout, range(56))
            R = int(exp["length"].sum())
            want = dict(pos=((R, A, 3), torch.float32), mask=((R, A), torch.bool), aatype=((R,), torch.uint8), plddt=((R,), torch.float32),
                        res_index=((R,), torch.int32), chain_index=((R,), torch.int32), cu_seqlens=((57,), torch.int32), length=((56,), torch.int32))
            assert set(t) == set(want) | {"names", "max_seqlen"}
            for k, (shape, dtype) in want.items():
                assert t[k].device == torch.device("cuda:0") and tuple(t[k].shape) == shape and t[k].dtype == dtype, k
            same({k: t[k].cpu().numpy() for k in KEYS}, exp, layout)
            cu = t["cu_seqlens"].cpu().numpy()
            assert np.array_equal(cu, np.concatenate([[0], np.cumsum(exp["length"])]))
            assert np.array_equal(t["chain_index"].cpu().numpy(), np.repeat(np.arange(56), np.diff(cu)))
            assert t["names"] == titles and t["max_seqlen"] == 1400 and isinstance(t["max_seqlen"], int)
        # an entry that does not decode is left out of the rows: cu_seqlens is the running sum over the accepted ones
        t = foldcomp.decode_tensors([entries[0], b"XXXX" + entries[1][4:], entries[2]], packed=True)
        ln = t["length"].cpu().numpy()
        assert ln[1] == 0 and list(t["cu_seqlens"].cpu().numpy()) == [0, ln[0], ln[0], ln[0] + ln[2]]
        assert sorted(set(t["chain_index"].cpu().numpy().tolist())) == [0, 2]
        with pytest.raises(ValueError):
            foldcomp.decode_tensors(entries[:2], packed=True, max_len=64)
        for empty in (foldcomp.decode_tensors([], packed=True), foldcomp.decode_tensors([entries[0][:100]], packed=True)):
            assert empty["pos"].shape == (0, 37, 3) and not empty["cu_seqlens"].any() and empty["max_seqlen"] == 0
    finally:
        api.set_codec(None)


def test_tensor_batches_packed_by_residue_budget(codec, golden, tmp_path):
    import torch
    import foldcomp
    from foldcomp_amd import api
    from foldcomp_amd.database import DatabaseWriter
    z, index = golden
    entries = [z[f"{n}/fcz"].tobytes() for n in db_cases(index)]
    path = str(tmp_path / "db")
    w = DatabaseWriter(path)
    for k, e in enumerate(entries):
        w.append(e, k, f"entry_{k:02d}")
    w.close()
    lens = [fczfile.residue_count(e) for e in entries]
    api.set_codec(codec)
    try:
        whole = foldcomp.decode_tensors(entries, packed=True)
        cu = whole["cu_seqlens"].cpu().numpy()
        # 300: two entries fit together, three do not; 140: some entries exceed the budget alone
        assert 2 * max(lens) > 300 > 2 * min(lens) and min(lens) < 140 < max(lens)
        for budget, bs, sort in ((300, 1024, False), (300, 1, False), (300, 1024, True), (140, 1024, False), (10 ** 6, 5, True)):
            with foldcomp.open(path) as db:
                seen, sizes = [], []
                for d in db.tensor_batches(bs, packed=True, max_residues=budget, sort_by_length=sort):
                    idx = [int(i) for i in d["index"]]
                    R = int(d["pos"].shape[0])
                    assert len(idx) <= bs and R == sum(lens[i] for i in idx) == int(d["cu_seqlens"][-1])     # nothing cropped
                    assert R <= budget or len(idx) == 1
                    for j, i in enumerate(idx):
                        a, b = int(d["cu_seqlens"][j]), int(d["cu_seqlens"][j + 1])
                        assert bool((d["pos"][a:b].view(torch.int32) == whole["pos"][cu[i]:cu[i + 1]].view(torch.int32)).all())
                        assert d["names"][j] == whole["names"][i]
                    seen += idx
                    sizes.append(len(idx))
                assert sorted(seen) == list(range(len(entries)))
                if not sort:
                    assert seen == list(range(len(entries)))
                assert max(sizes) == (2 if (budget, bs) == (300, 1024) else 5 if bs == 5 else 1)
        with foldcomp.open(path) as db:
            with pytest.raises(ValueError):
                next(db.tensor_batches(4, max_residues=1000))
            with pytest.raises(ValueError):
                next(db.tensor_batches(4, packed=True, max_len=100))
            # packed without a budget: batch_size entries per batch
            assert [len(d["index"]) for d in db.tensor_batches(10, packed=True)] == [10, 10, 4]
    finally:
        api.set_codec(None)
