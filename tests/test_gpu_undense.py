"""GPU: dense atom37 / atom14 / backbone4 tensors -> FCZ records (fcz_undense_dev, fcz_compress_dense_*, Codec.compress_dense,
encode_tensors). The bar is bit-identity of the FCZ bytes, and equality of the per-chain status, with the oracle's
fcz_oracle_compress_batch on the batch the numpy builder (tests/_undense.py) makes from the same arrays."""
import ctypes

import numpy as np
import pytest

import _dense as D
import _harness as H
import _undense as U
from _cases import compress_cases, entries_blob, golden_batch, golden_records_raw
from foldcomp_amd import _lib, fczfile
from foldcomp_amd._aa_tables import ATOM_NAMES, RES3, RES_NATOMS
from foldcomp_amd.structure import AtomTable, CChainBatch, CDenseIn, ChainBatch, batch_as_c

pytestmark = pytest.mark.gpu

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


class DevDense:
    """dense host arrays uploaded as torch tensors + the fcz_dense_in of their device pointers"""

    def __init__(self, d, titles=None):
        import torch
        self.n, self.L, self.A = d["mask"].shape
        self.t = {k: torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0") for k, v in d.items()
                  if k in ("pos", "mask", "aatype", "plddt") + META and v is not None}
        self.t["length"] = torch.from_numpy(np.ascontiguousarray(d["length"], np.uint32).view(np.int32)).to("cuda:0")
        self.s = CDenseIn(*(self.t[k].data_ptr() if k in self.t else None
                            for k in ("pos", "mask", "aatype", "length", "plddt") + META))
        if titles is not None:
            tt, toff = title_arrays(titles, self.n)
            self.t["titles"] = torch.from_numpy(tt).to("cuda:0"); self.t["title_off"] = torch.from_numpy(toff.view(np.int32)).to("cuda:0")
            self.s.titles, self.s.title_off = self.t["titles"].data_ptr(), self.t["title_off"].data_ptr()
        torch.cuda.synchronize()


def compress_dev(codec, d, layout, thr=25, titles=None):
    """fcz_compress_dense_begin_dev / _fetch_dev -> (blob, off, status) on the host"""
    import torch
    dd = DevDense(d, titles)
    counts = np.zeros(3, np.uint32); nbytes = ctypes.c_uint64(0)
    _lib.check(codec.lib.fcz_compress_dense_begin_dev(codec.ctx, ctypes.byref(dd.s), dd.n, dd.L, D.LAYOUTS[layout], thr, counts.ctypes.data,
                                                      ctypes.byref(nbytes)), "fcz_compress_dense_begin_dev")
    blob = torch.full((max(int(nbytes.value), 1),), 0xA5, dtype=torch.uint8, device="cuda:0")
    off = torch.full((dd.n + 1,), -1, dtype=torch.int64, device="cuda:0"); st = torch.full((dd.n,), 77, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    _lib.check(codec.lib.fcz_compress_dense_fetch_dev(codec.ctx, off.data_ptr(), st.data_ptr(), blob.data_ptr()), "fcz_compress_dense_fetch_dev")
    codec.synchronize()
    return blob.cpu().numpy()[:int(nbytes.value)], off.cpu().numpy().view(np.uint64), st.cpu().numpy(), counts


def compress_host(codec, d, layout, thr=25, titles=None):
    return codec.compress_dense(d["pos"], d["mask"], d["aatype"], d["length"], d.get("plddt"), layout=layout,
                                first_res_index=d.get("first_res_index"), chain_id=d.get("chain_id"), titles=titles, anchor_threshold=thr)


def expected(d, layout, thr=25, titles=None):
    """builder + oracle -> (ChainBatch, blob, off, status with this stage's refusals)"""
    b, refusal = U.batch_expected(d["pos"], d["mask"], d["aatype"], d["length"], layout, plddt=d.get("plddt"),
                                  first_res_index=d.get("first_res_index"), first_atom_index=d.get("first_atom_index"),
                                  chain_id=d.get("chain_id"), titles=titles, anchor_threshold=thr)
    blob, off, ost = H.oracle_compress(b, n_threads=8)
    return b, blob, off, U.expected_status(refusal, ost)


def same_records(got, want, what, skip=()):
    blob, off, st = got[:3]
    wblob, woff, wst = want
    assert np.array_equal(off, woff), (what, "offsets")
    assert np.array_equal(st, wst), (what, "status", np.flatnonzero(st != wst)[:8], st[st != wst][:8], wst[st != wst][:8])
    for c in range(len(st)):
        if c in skip:
            continue
        a, b = blob[int(off[c]):int(off[c + 1])].tobytes(), wblob[int(off[c]):int(off[c + 1])].tobytes()
        assert a == b, (what, c, first_diff(a, b))


def resident_batch(codec, d, layout, thr=25, titles=None):
    """fcz_undense_dev, then the resident batch and the per-chain verdicts fetched to the host"""
    dd = DevDense(d, titles)
    out = CChainBatch(); counts = np.zeros(3, np.uint32)
    _lib.check(codec.lib.fcz_undense_dev(codec.ctx, ctypes.byref(dd.s), dd.n, dd.L, D.LAYOUTS[layout], thr, ctypes.byref(out), counts.ctypes.data, None),
               "fcz_undense_dev")
    C, R, M = (int(v) for v in counts)
    assert (out.n_chains, out.n_residues, out.n_atoms, out.anchor_threshold) == (C, R, M, thr)
    TB = sum(len(t.encode("latin-1")) for t in titles) if titles is not None else 0
    b = ChainBatch(res_off=np.zeros(C + 1, np.uint32), atom_off=np.zeros(R + 1, np.uint32), x=np.zeros(M, np.float32), y=np.zeros(M, np.float32),
                   z=np.zeros(M, np.float32), atom_code=np.zeros(M, np.uint8), res_code=np.zeros(R, np.uint8), bfac_ca=np.zeros(R, np.float32),
                   first_res_index=np.zeros(C, np.int32), first_atom_index=np.zeros(C, np.int32), chain_id=np.zeros(C, np.uint8),
                   titles=np.zeros(max(TB, 1), np.uint8), title_off=np.zeros(C + 1, np.uint32), anchor_threshold=thr)
    st = np.full(C, 77, np.int32)
    cb = batch_as_c(b)
    _lib.check(codec.lib.fcz_undense_fetch(codec.ctx, ctypes.byref(cb), st.ctypes.data), "fcz_undense_fetch")
    b.titles = b.titles[:TB]
    return b, st


@pytest.fixture(scope="module")
def records(golden):
    return golden_records_raw(golden)


def golden_dense(records, layout, L, rng=None):
    """the oracle's decode of the 56 golden records as dense arrays (tests/_dense.py) + titles; garbage where nothing is read"""
    names, entries = records
    o = H.oracle_decompress(*entries_blob(entries))
    per, titles = [], []
    for i, fcz in enumerate(entries):
        seq, first, has_oxt = D.record_fields(fcz)
        a0, a1, r0 = int(o["atom_off"][i]), int(o["atom_off"][i + 1]), int(o["res_off"][i])
        xyz = np.stack([o["x"][a0:a1], o["y"][a0:a1], o["z"][a0:a1]], 1)
        per.append(D.dense_expected(xyz, seq, first, has_oxt, layout, L, plddt=o["bfac_res"][r0:r0 + len(seq)]))
        titles.append(fczfile.parse(fcz).title)
    d = D.stack_expected(per, L, D.WIDTH[layout])
    d["first_res_index"] = np.ascontiguousarray(d.pop("res_index")[:, 0])
    if rng is not None:
        U.poison(d, rng)
    return d, titles


@pytest.mark.parametrize("layout", list(D.LAYOUTS))
def test_golden_records_as_one_batch(codec, records, layout):
    d, titles = golden_dense(records, layout, 1437, np.random.default_rng(3))
    b, blob, off, st = expected(d, layout, titles=titles)
    assert not st.any() and b.n_chains == 56
    same_records(compress_dev(codec, d, layout, titles=titles), (blob, off, st), layout + " dev")
    same_records(compress_host(codec, d, layout, titles=titles), (blob, off, st), layout + " host")
    got, verdict = resident_batch(codec, d, layout, titles=titles)
    assert U.batches_equal(got, b) is None, (layout, U.batches_equal(got, b))
    assert not verdict.any()
    # without the optional arrays: pLDDT 0, residues from 1, chain A, no titles
    bare = {k: d[k] for k in ("pos", "mask", "aatype", "length")}
    wb, wblob, woff, wst = expected(bare, layout)
    assert not wb.bfac_ca.any() and (wb.first_res_index == 1).all() and wb.title_off[-1] == 0
    same_records(compress_dev(codec, bare, layout), (wblob, woff, wst), layout + " bare dev")
    same_records(compress_host(codec, bare, layout), (wblob, woff, wst), layout + " bare host")
    got, _ = resident_batch(codec, bare, layout)
    assert U.batches_equal(got, wb) is None, (layout, U.batches_equal(got, wb))


def test_golden_inputs_by_atom_name_give_the_committed_records(codec, golden):
    z, index = golden
    used = [nm for nm in compress_cases(index) if U.all_atoms_have_slots(golden_batch(z, nm))]
    assert len(used) >= 1
    for nm in used:
        gb = golden_batch(z, nm)
        d = U.dense_from_batch(gb, "atom37", gb.n_residues + 5)
        d["first_atom_index"] = gb.first_atom_index; d["chain_id"] = gb.chain_id
        U.poison(d, np.random.default_rng(len(nm)))
        blob, off, st, _ = compress_dev(codec, d, "atom37", thr=int(gb.anchor_threshold), titles=[bytes(gb.titles).decode("latin-1")])
        want = z[f"{nm}/fcz"].tobytes()
        assert st[0] == 0 and blob.tobytes() == want, (nm, first_diff(blob.tobytes(), want))


def atom_table(b: ChainBatch, c: int):
    """chain c of a flat batch as the reference's atom list"""
    r0, r1 = int(b.res_off[c]), int(b.res_off[c + 1])
    a0, a1 = int(b.atom_off[r0]), int(b.atom_off[r1])
    per = np.diff(b.atom_off[r0:r1 + 1].astype(np.int64))
    res_of = np.repeat(np.arange(r1 - r0), per)
    return AtomTable([ATOM_NAMES[int(k)] for k in b.atom_code[a0:a1]], [RES3[int(b.res_code[r0 + r])] for r in res_of],
                     [chr(int(b.chain_id[c]))] * (a1 - a0), (int(b.first_atom_index[c]) + np.arange(a1 - a0)).astype(np.int32),
                     (int(b.first_res_index[c]) + res_of).astype(np.int32),
                     np.stack([b.x[a0:a1], b.y[a0:a1], b.z[a0:a1]], 1).astype(np.float32), np.repeat(b.bfac_ca[r0:r1], per).astype(np.float32))


def test_sample_against_the_live_reference(codec, records):
    """the only leg that depends on oracle/_ref: Foldcomp::compress on the atom list the builder states"""
    if not H.have_ref():
        pytest.skip("oracle/_ref not built")
    d, titles = golden_dense(records, "atom37", 1400)
    pick = [0, 5, 17, 33, 40, 55]
    sub = {k: np.ascontiguousarray(v[pick]) for k, v in d.items()}
    tl = [titles[i] for i in pick]
    b, _, _, st = expected(sub, "atom37", titles=tl)
    blob, off, got_st, _ = compress_dev(codec, sub, "atom37", titles=tl)
    assert not got_st.any()
    for c in range(len(pick)):
        want = H.mask_pad(H.ref_compress(atom_table(b, c), tl[c], 25))
        have = H.mask_pad(blob[int(off[c]):int(off[c + 1])].tobytes())
        assert have == want, (pick[c], first_diff(have, want))


def synthetic_dense(layout, L, seed=20261017):
    """a seeded mixed-length batch in the file order of predicted structures (with OXT), placed into dense arrays by atom name"""
    from foldcomp_amd import synthetic
    lens = np.concatenate([np.minimum(synthetic.mixed_lengths(150, seed=seed), 600), [2, 2, 3, 3, 64, 65, 128, 129, 256, 257, L, 17, 40, 90, 91, 92, 93, 94, 95, 96, 97]])
    b = synthetic.to_chain_batch(synthetic.generate(len(lens), lens, seed=seed))
    d = U.dense_from_batch(b, layout, L)
    titles = [bytes(b.titles[int(b.title_off[c]):int(b.title_off[c + 1])]).decode() for c in range(b.n_chains)]
    return d, titles, len(lens)


def test_synthetic_mixed_batch_with_garbage_and_refusals(codec):
    L = 640
    d, titles, n = synthetic_dense("atom37", L)
    rng = np.random.default_rng(99)
    base = 150
    assert d["length"][base + 10] == L and d["length"].max() == L
    # chains of length 0 and 1 (the rows behind become padding), 2 and L are there already
    d["length"][base + 2] = 0; d["length"][base + 3] = 1
    # random side-chain atoms (and carbonyl oxygens) masked off; N, CA, C stay
    drop = rng.random(d["mask"].shape) < 0.12
    drop[:, :, :3] = False
    d["mask"][drop] = 0
    assert n // 2 < d["mask"][:, :, 36].sum() < n                                 # (some chains lost their OXT to the dropping)
    # a stray slot-36 bit in mid-chain (over a NaN), a set bit in a slot the residue type does not own, aatype 20 rows whose
    # side-chain bits stay set
    for c in (0, 1, 2, base + 6):
        d["mask"][c, 7, 36] = 1; d["pos"][c, 7, 36] = np.nan
    gly = np.argwhere((d["aatype"] == 7) & (np.arange(L)[None, :] < d["length"][:, None]))[:20]
    for c, l in gly:
        d["mask"][c, l, 3] = 1; d["pos"][c, l, 3] = np.inf                     # CB of a glycine
    unk = rng.random(d["aatype"].shape) < 0.03
    d["aatype"][unk] = 20
    # refusals: length > L, aatype 21, a residue without CA -- and input the codec refuses: NaN in a present atom, in a used pLDDT
    too_long, aa21, no_ca, nan_atom, nan_plddt = 20, 40, 60, 80, 100
    d["length"][too_long] = L + 5
    d["aatype"][aa21, 11] = 21
    d["mask"][no_ca, int(d["length"][no_ca]) - 1, 1] = 0
    d["pos"][nan_atom, 5, 1, 2] = np.nan
    d["plddt"][nan_plddt, 3] = np.inf
    pad = U.poison(d, rng)
    assert pad.any() and np.isnan(d["pos"]).any()
    nonfinite = (nan_atom, nan_plddt)
    for thr in (25, 7):
        b, blob, off, st = expected(d, "atom37", thr=thr, titles=titles)
        # (the oracle has no verdict on non-finite input: the codec's is FCZ_E_NONFINITE, and zeros in the record range)
        assert st[nan_atom] == 0 and st[nan_plddt] == 0
        st[list(nonfinite)] = U.E_NONFINITE
        assert st[too_long] == U.E_INVALID_ARG and st[aa21] == U.E_RESIDUE and st[no_ca] == U.E_RESIDUE
        assert st[base + 2] == U.E_TOO_SHORT and st[base + 3] == U.E_TOO_SHORT and (st != 0).sum() == 7
        for form in (compress_dev, compress_host):
            got = form(codec, d, "atom37", thr=thr, titles=titles)
            same_records(got, (blob, off, st), f"{form.__name__} thr={thr}", skip=nonfinite)
            for c in (too_long, aa21, no_ca) + nonfinite:
                assert off[c + 1] > off[c] and not got[0][int(off[c]):int(off[c + 1])].any(), c
        got_b, verdict = resident_batch(codec, d, "atom37", thr=thr, titles=titles)
        assert U.batches_equal(got_b, b) is None, U.batches_equal(got_b, b)
        assert list(np.flatnonzero(verdict)) == [too_long, aa21, no_ca]
        assert np.isfinite(got_b.z).sum() == got_b.n_atoms - 1 and np.isfinite(got_b.bfac_ca).sum() == got_b.n_residues - 1
    # the neighbours of the refused chains, compressed alone in a small call, give the same records
    full = compress_dev(codec, d, "atom37", titles=titles)
    near = sorted({c + k for c in (too_long, aa21, no_ca, nan_atom, nan_plddt) for k in (-1, 1)})
    sub = {k: np.ascontiguousarray(v[near]) for k, v in d.items()}
    alone = compress_dev(codec, sub, "atom37", titles=[titles[c] for c in near])
    assert not alone[2].any()
    for k, c in enumerate(near):
        a = alone[0][int(alone[1][k]):int(alone[1][k + 1])].tobytes()
        f = full[0][int(full[1][c]):int(full[1][c + 1])].tobytes()
        assert a == f and full[2][c] == 0, (c, first_diff(a, f))


@pytest.mark.parametrize("layout,thr", [("atom14", 25), ("backbone4", 25), ("atom37", 10), ("atom14", 33), ("atom37", 200)])
def test_synthetic_layouts_and_anchor_thresholds(codec, layout, thr):
    L = 613                                                                      # (rows that do not start on 16-byte boundaries)
    d, titles, n = synthetic_dense(layout, L, seed=5)
    U.poison(d, np.random.default_rng(thr))
    b, blob, off, st = expected(d, layout, thr=thr, titles=titles)
    assert not st.any()
    if layout != "atom37":
        assert not (b.atom_code == D.OXT_CODE).any()
    if layout == "backbone4":
        assert b.n_atoms == 4 * b.n_residues
    same_records(compress_dev(codec, d, layout, thr=thr, titles=titles), (blob, off, st), f"{layout} thr={thr} dev")
    same_records(compress_host(codec, d, layout, thr=thr, titles=titles), (blob, off, st), f"{layout} thr={thr} host")


def test_no_chains_and_bad_arguments(codec):
    lib = codec.lib
    d, titles, n = synthetic_dense("atom14", 613, seed=5)
    sub = {k: np.ascontiguousarray(v[:3]) for k, v in d.items()}
    dd = DevDense(sub, titles[:3])
    counts = np.full(3, 9, np.uint32); nbytes = ctypes.c_uint64(9); out = CChainBatch()
    for begin in (lib.fcz_compress_dense_begin_dev, lib.fcz_compress_dense_begin):
        nbytes.value = 9
        assert begin(codec.ctx, ctypes.byref(dd.s), 0, 613, 1, 25, counts.ctypes.data, ctypes.byref(nbytes)) == 0
        assert nbytes.value == 0 and not counts.any()
        assert begin(codec.ctx, None, 0, 613, 1, 25, counts.ctypes.data, ctypes.byref(nbytes)) == 0
    off = np.full(1, 5, np.uint64)
    assert lib.fcz_compress_dense_fetch(codec.ctx, off.ctypes.data, None, None) == 0 and off[0] == 0
    assert lib.fcz_undense_dev(codec.ctx, None, 0, 613, 1, 25, ctypes.byref(out), counts.ctypes.data, None) == 0 and out.n_chains == 0
    blob, off, st = codec.compress_dense(sub["pos"][:0], sub["mask"][:0], sub["aatype"][:0], sub["length"][:0], layout="atom14")
    assert len(blob) == 0 and list(off) == [0] and len(st) == 0

    def bad(**kw):
        a = dict(ctx=codec.ctx, s=dd.s, n=3, L=613, layout=1, thr=25)
        a.update(kw)
        s = ctypes.byref(a["s"]) if a["s"] is not None else None
        r = [f(a["ctx"], s, a["n"], a["L"], a["layout"], a["thr"], counts.ctypes.data, ctypes.byref(nbytes))
             for f in (lib.fcz_compress_dense_begin_dev, lib.fcz_compress_dense_begin)]
        r.append(lib.fcz_undense_dev(a["ctx"], s, a["n"], a["L"], a["layout"], a["thr"], ctypes.byref(out), counts.ctypes.data, None))
        return r

    def without(field):
        s = CDenseIn.from_buffer_copy(dd.s)
        setattr(s, field, None)
        return s

    assert bad(ctx=None) == [-1] * 3 and bad(layout=3) == [-1] * 3 and bad(layout=-1) == [-1] * 3 and bad(L=0) == [-1] * 3
    assert bad(thr=0) == [-1] * 3 and bad(s=None) == [-1] * 3
    for field in ("pos", "mask", "aatype", "length", "titles", "title_off"):
        assert bad(s=without(field)) == [-1] * 3, field
    # the ctx is as good as before
    b, blob, off, st = expected(sub, "atom14", titles=titles[:3])
    same_records(compress_dev(codec, sub, "atom14", titles=titles[:3]), (blob, off, st), "after bad arguments")


def test_index_beyond_32_bits(codec):
    """one call whose pos holds more than 2^32 floats (atom37, L = 1024, 37 800 chains: 17.2 GB of pos, 1.4 GB of mask), all of it
    padding full of NaN except the last 8 chains; their records equal those of the same chains in a small call. Sized as DESIGN.md
    section 9 item 7 sizes the launch-plan cases: 18.7 GB of tensors beside the session codec's scratch, far below the device's 288 GB."""
    import torch
    n, L, A, k = 37_800, 1024, 37, 8
    assert n * L * A * 3 > 2 ** 32 and (n - k) * L * A * 3 > 2 ** 32
    d, titles, _ = synthetic_dense("atom37", L, seed=8)
    pick = [150 + 10, 3, 150 + 4, 9, 150 + 8, 27, 150 + 0, 41]                    # among them the chain of L residues and a 2-residue one
    sub = {key: np.ascontiguousarray(v[pick]) for key, v in d.items()}
    U.poison(sub, np.random.default_rng(1))
    tl = [titles[c] for c in pick]
    b, blob, off, st = expected(sub, "atom37", titles=tl)
    assert not st.any() and sub["length"].max() == L
    small = compress_dev(codec, sub, "atom37", titles=tl)
    same_records(small, (blob, off, st), "small call")
    pos = torch.full((n, L, A, 3), float("nan"), dtype=torch.float32, device="cuda:0")
    mask = torch.full((n, L, A), 0xA5, dtype=torch.uint8, device="cuda:0")
    aatype = torch.full((n, L), 0xA5, dtype=torch.uint8, device="cuda:0")
    plddt = torch.full((n, L), float("nan"), dtype=torch.float32, device="cuda:0")
    length = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    first = torch.ones(n, dtype=torch.int32, device="cuda:0")
    for key, t in (("pos", pos), ("mask", mask), ("aatype", aatype), ("plddt", plddt)):
        t[n - k:] = torch.from_numpy(sub[key]).to("cuda:0")
    length[n - k:] = torch.from_numpy(sub["length"].view(np.int32)).to("cuda:0")
    first[n - k:] = torch.from_numpy(sub["first_res_index"]).to("cuda:0")
    tt, toff = title_arrays([""] * (n - k) + tl, n)
    tt_t, toff_t = torch.from_numpy(tt).to("cuda:0"), torch.from_numpy(toff.view(np.int32)).to("cuda:0")
    s = CDenseIn(pos.data_ptr(), mask.data_ptr(), aatype.data_ptr(), length.data_ptr(), plddt.data_ptr(), first.data_ptr(), None, None,
                 tt_t.data_ptr(), toff_t.data_ptr())
    torch.cuda.synchronize()
    counts = np.zeros(3, np.uint32); nbytes = ctypes.c_uint64(0)
    _lib.check(codec.lib.fcz_compress_dense_begin_dev(codec.ctx, ctypes.byref(s), n, L, 0, 25, counts.ctypes.data, ctypes.byref(nbytes)),
               "fcz_compress_dense_begin_dev")
    assert list(counts) == [n, b.n_residues, b.n_atoms]
    big_blob = torch.empty(int(nbytes.value), dtype=torch.uint8, device="cuda:0")
    big_off = torch.empty(n + 1, dtype=torch.int64, device="cuda:0"); big_st = torch.empty(n, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    _lib.check(codec.lib.fcz_compress_dense_fetch_dev(codec.ctx, big_off.data_ptr(), big_st.data_ptr(), big_blob.data_ptr()), "fcz_compress_dense_fetch_dev")
    codec.synchronize()
    g_off, g_st, g_blob = big_off.cpu().numpy(), big_st.cpu().numpy(), big_blob.cpu().numpy()
    assert (g_st[:n - k] == U.E_TOO_SHORT).all() and not g_st[n - k:].any()
    empty = int(g_off[1] - g_off[0])
    assert empty > 0 and (np.diff(g_off[:n - k + 1]) == empty).all() and not g_blob[:int(g_off[n - k])].any()
    for c in range(k):
        a = g_blob[int(g_off[n - k + c]):int(g_off[n - k + c + 1])].tobytes()
        w = blob[int(off[c]):int(off[c + 1])].tobytes()
        assert a == w, (c, first_diff(a, w))
    del pos, mask, aatype, plddt, big_blob
    torch.cuda.empty_cache()


def test_encode_tensors(codec, records, golden, tmp_path):
    import torch
    import foldcomp
    from foldcomp_amd import api
    from foldcomp_amd.database import DatabaseWriter
    names, entries = records
    api.set_codec(codec)
    try:
        for layout in D.LAYOUTS:
            t = foldcomp.decode_tensors(entries, layout=layout)
            got = foldcomp.encode_tensors(t)
            d, titles = golden_dense(records, layout, 1400)
            assert t["names"] == titles
            b, blob, off, st = expected(d, layout, titles=titles)
            assert not st.any() and len(got) == 56
            for c in range(56):
                w = blob[int(off[c]):int(off[c + 1])].tobytes()
                assert got[c] == w, (layout, c, first_diff(got[c], w))
            # the records decode again to the right names and residue counts
            back = foldcomp.decompress_many(got)
            assert [nm for nm, _ in back] == titles
            assert [fczfile.residue_count(e) for e in got] == [fczfile.residue_count(e) for e in entries]
        # the tensors as keywords, names and layout given, an int64 length, a uint8 mask
        t = foldcomp.decode_tensors(entries[:7], layout="atom37")
        kw = foldcomp.encode_tensors(pos=t["pos"], mask=t["mask"].view(torch.uint8), aatype=t["aatype"], length=t["length"].to(torch.int64),
                                     plddt=t["plddt"], res_index=t["res_index"], names=t["names"], layout="atom37", codec=codec)
        assert kw == foldcomp.encode_tensors(t)
        assert foldcomp.encode_tensors(t, names=["x%d" % i for i in range(7)])[3] != kw[3]
        assert foldcomp.encode_tensors(foldcomp.decode_tensors([])) == []
        # a batch of tensor_batches as it is
        path = str(tmp_path / "db")
        w = DatabaseWriter(path)
        for k, e in enumerate(entries[32:44]):
            w.append(e, k, f"entry_{k:02d}")
        w.close()
        whole = foldcomp.encode_tensors(foldcomp.decode_tensors(entries[32:44]))
        with foldcomp.open(path) as db:
            for bt in db.tensor_batches(5):
                recs = foldcomp.encode_tensors(bt)
                # (a batch is padded to its own longest entry: the records do not depend on L)
                assert recs == [whole[int(i)] for i in bt["index"]]
        # a refused chain: an error, or None under skip_bad
        t = foldcomp.decode_tensors(entries[:4], layout="atom14")
        t["aatype"][2, 1] = 21
        with pytest.raises(foldcomp.error):
            foldcomp.encode_tensors(t)
        some = foldcomp.encode_tensors(t, skip_bad=True)
        assert some[2] is None and all(isinstance(e, bytes) for e in some[:2] + some[3:])
        # tensors that are not where the codec works, or not all in one place
        t = foldcomp.decode_tensors(entries[:2])
        with pytest.raises(foldcomp.error, match="cpu"):
            foldcomp.encode_tensors({k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in t.items()})
        with pytest.raises(foldcomp.error, match="mask"):
            foldcomp.encode_tensors(dict(t, mask=t["mask"].cpu()))
        with pytest.raises(ValueError):
            foldcomp.encode_tensors(t, layout="atom14")
        with pytest.raises(ValueError, match="contiguous"):
            foldcomp.encode_tensors(dict(t, aatype=t["aatype"].t().contiguous().t()))
    finally:
        api.set_codec(None)
