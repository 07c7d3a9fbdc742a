"""GPU: packed dense tensors -> FCZ records (fcz_undense_packed_dev, fcz_compress_dense_packed_begin[_dev], Codec.compress_dense_packed,
encode_tensors on the packed dict). The bar is the bytes of the padded path on the same rows (tests/test_gpu_undense.py holds that
one to the oracle), and the committed reference records where the goldens pin them."""
import ctypes

import numpy as np
import pytest

import _dense as D
import _undense as U
from _cases import compress_cases, golden_batch, golden_records_raw
from foldcomp_amd import _lib
from foldcomp_amd.structure import CChainBatch, CDenseIn

pytestmark = pytest.mark.gpu

ROWS = ("pos", "mask", "aatype", "plddt")
META = ("first_res_index", "first_atom_index", "chain_id")


def first_diff(a: bytes, b: bytes):
    n = min(len(a), len(b))
    d = [i for i in range(n) if a[i] != b[i]]
    return len(a), len(b), len(d), d[:16]


def title_arrays(titles, n):
    tb = [t.encode("latin-1") for t in titles]
    toff = np.zeros(n + 1, np.uint32)
    toff[1:] = np.cumsum([len(t) for t in tb])
    return np.frombuffer(b"".join(tb) + b"\0", np.uint8).copy(), toff


def pack(d):
    """padded dict of tests/_undense.py -> packed dict: the rows l < length[c] of every chain back to back + row_off"""
    lens = d["length"].astype(np.int64)
    keep = np.arange(d["mask"].shape[1])[None, :] < lens[:, None]
    p = {k: np.ascontiguousarray(d[k][keep]) for k in ROWS if d.get(k) is not None}
    p["row_off"] = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    for k in META:
        if d.get(k) is not None:
            p[k] = d[k]
    return p


def unpack(p, row_off, valid):
    """packed rows -> padded dict with chain c = rows row_off[c] .. row_off[c + 1] (valid[c]) or no row (length 0)"""
    ro = np.asarray(row_off, np.int64)
    lens = np.where(valid, ro[1:] - ro[:-1], 0)
    n, L = len(lens), max(int(lens.max()), 1)
    d = {k: np.zeros((n, L) + p[k].shape[1:], p[k].dtype) for k in ROWS if k in p}
    for c in range(n):
        for k in d:
            d[k][c, :lens[c]] = p[k][ro[c]:ro[c] + lens[c]]
    d["length"] = lens.astype(np.uint32)
    return d


def compress_packed_dev(codec, p, row_off, R, layout, thr=25, titles=None, tail_rows=0):
    """fcz_compress_dense_packed_begin_dev / fcz_compress_dense_fetch_dev on device copies of the arrays (tail_rows rows of NaN /
    0xFF behind row R - 1: a guard region the call must not read as data) -> (blob, off, status, counts) on the host"""
    import torch
    n = len(row_off) - 1
    t = {}
    for k in ROWS + META:
        if p.get(k) is None:
            continue
        a = np.ascontiguousarray(p[k])
        if k in ROWS and tail_rows:
            tail = np.full((tail_rows,) + a.shape[1:], np.nan if a.dtype == np.float32 else 0xFF, a.dtype)
            a = np.concatenate([a[:R], tail])
        t[k] = torch.from_numpy(a).to("cuda:0")
    t["row_off"] = torch.from_numpy(np.ascontiguousarray(row_off, np.uint32).view(np.int32)).to("cuda:0")
    s = CDenseIn(t["pos"].data_ptr(), t["mask"].data_ptr(), t["aatype"].data_ptr(), None, t["plddt"].data_ptr() if "plddt" in t else None,
                 *(t[k].data_ptr() if k in t else None for k in META))
    if titles is not None:
        tt, toff = title_arrays(titles, n)
        t["titles"], t["title_off"] = torch.from_numpy(tt).to("cuda:0"), torch.from_numpy(toff.view(np.int32)).to("cuda:0")
        s.titles, s.title_off = t["titles"].data_ptr(), t["title_off"].data_ptr()
    torch.cuda.synchronize()
    counts = np.zeros(3, np.uint32); nbytes = ctypes.c_uint64(0)
    _lib.check(codec.lib.fcz_compress_dense_packed_begin_dev(codec.ctx, ctypes.byref(s), t["row_off"].data_ptr(), n, R, D.LAYOUTS[layout], thr,
                                                             counts.ctypes.data, ctypes.byref(nbytes)), "fcz_compress_dense_packed_begin_dev")
    blob = torch.full((max(int(nbytes.value), 1),), 0xA5, dtype=torch.uint8, device="cuda:0")
    off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda:0"); st = torch.full((n,), 77, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    _lib.check(codec.lib.fcz_compress_dense_fetch_dev(codec.ctx, off.data_ptr(), st.data_ptr(), blob.data_ptr()), "fcz_compress_dense_fetch_dev")
    codec.synchronize()
    return blob.cpu().numpy()[:int(nbytes.value)], off.cpu().numpy().view(np.uint64), st.cpu().numpy(), counts


def record(got, c):
    return got[0][int(got[1][c]):int(got[1][c + 1])].tobytes()


def padded_records(codec, d, layout, thr=25, titles=None):
    blob, off, st = codec.compress_dense(d["pos"], d["mask"], d["aatype"], d["length"], d.get("plddt"), layout=layout,
                                         first_res_index=d.get("first_res_index"), chain_id=d.get("chain_id"), titles=titles, anchor_threshold=thr)
    return blob, off, st


@pytest.fixture(scope="module")
def records(golden):
    return golden_records_raw(golden)


def test_round_trip_gives_the_records_of_the_padded_path(codec, records, golden):
    import foldcomp
    from foldcomp_amd import api
    names, entries = records
    api.set_codec(codec)
    try:
        for layout in D.LAYOUTS:
            via_padded = foldcomp.encode_tensors(foldcomp.decode_tensors(entries, layout=layout))
            t = foldcomp.decode_tensors(entries, layout=layout, packed=True)
            via_packed = foldcomp.encode_tensors(t)
            assert len(via_packed) == 56
            for c in range(56):
                assert via_packed[c] == via_padded[c], (layout, c, first_diff(via_packed[c], via_padded[c]))
        # the tensors as keywords: int64 cu_seqlens, uint8 mask, first_res_index in place of res_index
        t = foldcomp.decode_tensors(entries[:7], packed=True)
        import torch
        cu = t["cu_seqlens"].to(torch.int64)
        kw = foldcomp.encode_tensors(pos=t["pos"], mask=t["mask"].view(torch.uint8), aatype=t["aatype"], cu_seqlens=cu, plddt=t["plddt"],
                                     first_res_index=t["res_index"][cu[:-1]], names=t["names"], layout="atom37", codec=codec)
        assert kw == foldcomp.encode_tensors(t) == foldcomp.encode_tensors(foldcomp.decode_tensors(entries[:7]))
        # a refused chain: an error, or None under skip_bad
        t["aatype"][int(cu[2]) + 1] = 21
        with pytest.raises(foldcomp.error):
            foldcomp.encode_tensors(t)
        some = foldcomp.encode_tensors(t, skip_bad=True)
        assert some[2] is None and some[:2] + some[3:] == kw[:2] + kw[3:]
        assert foldcomp.encode_tensors(foldcomp.decode_tensors([], packed=True)) == []
    finally:
        api.set_codec(None)
    # the golden inputs that tests/test_gpu_undense.py pins to the committed reference records, several chains in one packed call
    z, index = golden
    used = [nm for nm in compress_cases(index) if U.all_atoms_have_slots(golden_batch(z, nm))]
    assert len(used) >= 1
    by_thr = {}
    for nm in used:
        by_thr.setdefault(int(golden_batch(z, nm).anchor_threshold), []).append(nm)
    for thr, group in by_thr.items():
        parts, titles = [], []
        for nm in group:
            gb = golden_batch(z, nm)
            d = U.dense_from_batch(gb, "atom37", gb.n_residues)
            d["first_atom_index"] = gb.first_atom_index; d["chain_id"] = gb.chain_id
            parts.append(pack(d)); titles.append(bytes(gb.titles).decode("latin-1"))
        p = {k: np.concatenate([q[k] for q in parts]) for k in ROWS + META}
        junk = (p["mask"] == 0)
        p["pos"].view(np.uint32)[junk] = 0x7FC00000
        row_off = np.concatenate([[0], np.cumsum([len(q["aatype"]) for q in parts])]).astype(np.uint32)
        got = compress_packed_dev(codec, p, row_off, int(row_off[-1]), "atom37", thr=thr, titles=titles, tail_rows=3)
        assert not got[2].any()
        for c, nm in enumerate(group):
            want = z[f"{nm}/fcz"].tobytes()
            assert record(got, c) == want, (nm, first_diff(record(got, c), want))


def synthetic_packed(codec, layout="atom37"):
    """a small seeded batch with OXTs as padded (tests/_undense.py) and packed arrays, its titles, and the padded path's records"""
    from foldcomp_amd import synthetic
    lens = np.asarray([40, 2, 3, 64, 65, 17, 128, 129, 90, 33, 200, 63, 5, 77], np.int64)
    b = synthetic.to_chain_batch(synthetic.generate(len(lens), lens, seed=20261018))
    d = U.dense_from_batch(b, layout, int(lens.max()))
    titles = [bytes(b.titles[int(b.title_off[c]):int(b.title_off[c + 1])]).decode() for c in range(b.n_chains)]
    return d, pack(d), titles


def test_contract_garbage_oxt_refusals_and_guard(codec):
    d, p, titles = synthetic_packed(codec)
    n, R = len(titles), int(p["row_off"][-1])
    ro = p["row_off"].astype(np.int64)
    assert d["mask"][:, :, 36].sum() == n                                          # every chain ends in an OXT
    base = padded_records(codec, d, "atom37", titles=titles)
    assert not base[2].any()
    clean = compress_packed_dev(codec, p, p["row_off"], R, "atom37", titles=titles)
    assert list(clean[3]) == [n, R, int(d["mask"][np.arange(d["mask"].shape[1])[None, :] < d["length"][:, None]].sum())]
    for c in range(n):
        assert record(clean, c) == record(base, c), (c, first_diff(record(clean, c), record(base, c)))
    # garbage where mask == 0, a stray slot-36 bit in mid-chain over a NaN, NaN / 0xFF rows behind row R - 1: no byte changes, and no
    # chain is FCZ_E_NONFINITE. The host form (Codec.compress_dense_packed) gives the same.
    g = {k: np.array(v, copy=True) for k, v in p.items()}
    rng = np.random.default_rng(7)
    junk = rng.integers(0, 2 ** 32, size=g["pos"].shape, dtype=np.uint64).astype(np.uint32)
    junk[rng.random(g["pos"].shape) < 0.5] = 0x7FC00000
    off_mask = g["mask"] == 0
    g["pos"].view(np.uint32)[off_mask] = junk[off_mask]
    for c in (0, 3, 6, 10):
        g["mask"][ro[c] + 1, 36] = 1; g["pos"][ro[c] + 1, 36] = np.nan
    dirty = compress_packed_dev(codec, g, g["row_off"], R, "atom37", titles=titles, tail_rows=70)
    assert not dirty[2].any() and np.array_equal(dirty[1], clean[1]) and dirty[0].tobytes() == clean[0].tobytes()
    host = codec.compress_dense_packed(g["pos"], g["mask"], g["aatype"], g["row_off"], g["plddt"], first_res_index=g["first_res_index"], titles=titles)
    assert not host[2].any() and host[0].tobytes() == clean[0].tobytes() and np.array_equal(host[1], clean[1])
    # the OXT comes from a chain's LAST row only: with it masked off there, the record is that of the chain without an OXT
    no_oxt = {k: np.array(v, copy=True) for k, v in g.items()}
    dd = {k: np.array(v, copy=True) for k, v in d.items()}
    for c in (3, 6):
        no_oxt["mask"][ro[c + 1] - 1, 36] = 0; dd["mask"][c, d["length"][c] - 1, 36] = 0
    got, want = compress_packed_dev(codec, no_oxt, no_oxt["row_off"], R, "atom37", titles=titles), padded_records(codec, dd, "atom37", titles=titles)
    for c in range(n):
        assert record(got, c) == record(want, c), c
    assert record(got, 3) != record(clean, 3) and record(got, 4) == record(clean, 4)

    # per-chain refusals: the other chains' records are those of the clean call
    def refused(got, bad, status, others=range(n), shift=0):
        for c in bad:
            assert got[2][c] == status and got[1][c + 1] > got[1][c] and not got[0][int(got[1][c]):int(got[1][c + 1])].any(), c
        for c in others:
            k = c + (shift if c > min(bad) else 0)
            if k not in bad:
                assert got[2][k] == 0 and record(got, k) == record(clean, c), (c, k)

    aa = {k: np.array(v, copy=True) for k, v in g.items()}
    aa["aatype"][ro[4] + 2] = 21                                                   # aatype > 20
    aa["mask"][ro[8 + 1] - 1, 1] = 0                                               # a row without CA
    refused(compress_packed_dev(codec, aa, aa["row_off"], R, "atom37", titles=titles, tail_rows=70), (4, 8), U.E_RESIDUE)
    # row_off[c + 1] > R: the last chain claims three of the guard rows
    over = g["row_off"].copy(); over[-1] = R + 3
    refused(compress_packed_dev(codec, g, over, R, "atom37", titles=titles, tail_rows=70), (n - 1,), U.E_INVALID_ARG)
    # a range that runs backwards, put in front of chain 6: [.., ro[6], ro[6] - 5 | ro[7], ..]. The chain behind it starts five rows
    # early, inside chain 5, whose last row (its OXT bit set) is now also a row in the middle of another chain: chain 5 keeps its OXT,
    # the other one ignores it. Its record is that of the same rows as a padded chain.
    back = np.concatenate([g["row_off"][:7], [ro[6] - 5], g["row_off"][7:]]).astype(np.uint32)
    t2 = titles[:6] + ["backwards"] + titles[6:]
    fr = np.concatenate([g["first_res_index"][:6], [1], g["first_res_index"][6:]]).astype(np.int32)
    g2 = dict(g, first_res_index=fr)
    got = compress_packed_dev(codec, g2, back, R, "atom37", titles=t2, tail_rows=70)
    refused(got, (6,), U.E_INVALID_ARG, others=[c for c in range(n) if c != 6], shift=1)
    valid = np.ones(n + 1, bool); valid[6] = False
    want = padded_records(codec, dict(unpack(g, back, valid), first_res_index=fr), "atom37", titles=t2)
    assert got[2][7] == 0 and record(got, 7) == record(want, 7) and record(got, 7) != record(clean, 6)
    # a length above 65 535: one chain of 65 536 rows (a short chain's rows over and over) behind the others
    reps = -(-65536 // int(d["length"][0]))
    big = {k: np.concatenate([g[k]] + [g[k][ro[0]:ro[1]]] * reps)[:R + 65536] for k in ROWS}
    big["first_res_index"] = np.append(g["first_res_index"], 1).astype(np.int32)
    long_off = np.append(g["row_off"], R + 65536).astype(np.uint32)
    got = compress_packed_dev(codec, big, long_off, R + 65536, "atom37", titles=titles + ["too long"], tail_rows=70)
    refused(got, (n,), U.E_INVALID_ARG)
    # ... and 65 535 rows are not refused by this stage
    long_off[-1] = R + 65535
    counts = np.zeros(3, np.uint32); out = CChainBatch()
    import torch
    t = {k: torch.from_numpy(big[k]).to("cuda:0") for k in ROWS}
    ro_t = torch.from_numpy(long_off.view(np.int32)).to("cuda:0"); st_t = torch.full((n + 1,), 77, dtype=torch.int32, device="cuda:0")
    s = CDenseIn(t["pos"].data_ptr(), t["mask"].data_ptr(), t["aatype"].data_ptr(), None, t["plddt"].data_ptr())
    torch.cuda.synchronize()
    _lib.check(codec.lib.fcz_undense_packed_dev(codec.ctx, ctypes.byref(s), ro_t.data_ptr(), n + 1, R + 65536, 0, 25, ctypes.byref(out), counts.ctypes.data,
                                                st_t.data_ptr()), "fcz_undense_packed_dev")
    codec.synchronize()
    assert not st_t.cpu().numpy().any() and list(counts[:2]) == [n + 1, R + 65535] and out.n_residues == R + 65535


def test_layouts_thresholds_and_bad_arguments(codec):
    for layout, thr in (("atom14", 25), ("backbone4", 25), ("atom37", 10)):
        d, p, titles = synthetic_packed(codec, layout)
        base = padded_records(codec, d, layout, thr=thr, titles=titles)
        got = compress_packed_dev(codec, p, p["row_off"], int(p["row_off"][-1]), layout, thr=thr, titles=titles, tail_rows=5)
        assert not got[2].any() and np.array_equal(got[1], base[1]) and got[0].tobytes() == base[0].tobytes(), layout
    lib = codec.lib
    import torch
    t = {k: torch.from_numpy(p[k]).to("cuda:0") for k in ROWS}
    ro_t = torch.from_numpy(p["row_off"].view(np.int32)).to("cuda:0")
    s = CDenseIn(t["pos"].data_ptr(), t["mask"].data_ptr(), t["aatype"].data_ptr(), None, t["plddt"].data_ptr())
    n, R = len(titles), int(p["row_off"][-1])
    counts = np.full(3, 9, np.uint32); nbytes = ctypes.c_uint64(9); out = CChainBatch()

    def calls(ctx, sp, ro, layout, thr, n=n):
        r = [f(ctx, sp, ro, n, R, layout, thr, counts.ctypes.data, ctypes.byref(nbytes))
             for f in (lib.fcz_compress_dense_packed_begin_dev, lib.fcz_compress_dense_packed_begin)]
        return r + [lib.fcz_undense_packed_dev(ctx, sp, ro, n, R, layout, thr, ctypes.byref(out), counts.ctypes.data, None)]

    sp = ctypes.byref(s)
    assert calls(None, sp, ro_t.data_ptr(), 0, 25) == [-1] * 3 and calls(codec.ctx, sp, ro_t.data_ptr(), 3, 25) == [-1] * 3
    assert calls(codec.ctx, sp, ro_t.data_ptr(), 0, 0) == [-1] * 3 and calls(codec.ctx, sp, None, 0, 25) == [-1] * 3
    assert calls(codec.ctx, None, ro_t.data_ptr(), 0, 25) == [-1] * 3
    for field in ("pos", "mask", "aatype"):
        s2 = CDenseIn.from_buffer_copy(s)
        setattr(s2, field, None)
        assert calls(codec.ctx, ctypes.byref(s2), ro_t.data_ptr(), 0, 25) == [-1] * 3, field
    assert calls(codec.ctx, None, None, 0, 25, n=0) == [0] * 3 and nbytes.value == 0 and not counts.any()
