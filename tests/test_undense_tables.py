"""CPU: the numpy restatement of the tensors -> batch contract (tests/_undense.py), which the GPU tests hold the kernels to, is
itself pinned to the goldens through the oracle; the aatype map is the inverse of the dense direction's; the new C-ABI entry points
exist and refuse to run without a context."""
import ctypes

import numpy as np
import pytest

import _dense as D
import _harness as H
import _undense as U
from _cases import compress_cases, db_cases, entries_blob, golden_batch
from foldcomp_amd import _lib, fczfile
from foldcomp_amd._aa_tables import RES_NATOMS
from foldcomp_amd.structure import CChainBatch, CDenseIn, ChainBatch

NEW = ["fcz_undense_dev", "fcz_undense_fetch", "fcz_compress_dense_begin_dev", "fcz_compress_dense_fetch_dev",
       "fcz_compress_dense_begin", "fcz_compress_dense_fetch"]


def flat_batch(o, i, title, keep=None):
    """entry i of an oracle decode (canonical order, OXT last) as a one-chain ChainBatch; keep(atom_code) drops atoms"""
    r0, r1 = int(o["res_off"][i]), int(o["res_off"][i + 1])
    a0, a1 = int(o["atom_off"][i]), int(o["atom_off"][i + 1])
    seq = o["res_code"][r0:r1]
    per = np.asarray(RES_NATOMS, np.int64)[seq]
    has_oxt = a1 - a0 == per.sum() + 1
    assert has_oxt or a1 - a0 == per.sum()
    res_of = np.repeat(np.arange(r1 - r0), per)
    if has_oxt:
        res_of = np.append(res_of, r1 - r0 - 1)
    code = o["atom_code"][a0:a1]
    sel = np.ones(a1 - a0, bool) if keep is None else keep(code)
    atom_off = np.zeros(r1 - r0 + 1, np.uint32)
    atom_off[1:] = np.cumsum(np.bincount(res_of[sel], minlength=r1 - r0))
    tb = title.encode("latin-1")
    info = o["info"][i]
    return ChainBatch(res_off=np.asarray([0, r1 - r0], np.uint32), atom_off=atom_off, x=o["x"][a0:a1][sel].copy(), y=o["y"][a0:a1][sel].copy(),
                      z=o["z"][a0:a1][sel].copy(), atom_code=code[sel].copy(), res_code=seq.copy(), bfac_ca=o["bfac_res"][r0:r1].copy(),
                      first_res_index=np.asarray([info.first_res_index], np.int32), first_atom_index=np.asarray([info.first_atom_index], np.int32),
                      chain_id=np.asarray([ord(info.chain_id)], np.uint8), titles=np.frombuffer(tb, np.uint8).copy(),
                      title_off=np.asarray([0, len(tb)], np.uint32)), bool(has_oxt)


def test_builder_is_pinned_to_the_goldens(golden):
    """every golden record: oracle decode -> dense_expected (the dense direction's own statement) -> builder -> oracle compress,
    against the oracle's compression of the same flat canonical atom list built directly"""
    z, index = golden
    names = compress_cases(index) + db_cases(index)
    assert len(names) == 56
    entries = [z[f"{n}/fcz"].tobytes() for n in names]
    o = H.oracle_decompress(*entries_blob(entries))
    n_oxt = 0
    for i, (nm, fcz) in enumerate(zip(names, entries)):
        assert o["info"][i].status == 0, nm
        title = fczfile.parse(fcz).title
        direct, has_oxt = flat_batch(o, i, title)
        n_oxt += has_oxt
        a0, a1 = int(o["atom_off"][i]), int(o["atom_off"][i + 1])
        r0 = int(o["res_off"][i])
        xyz = np.stack([o["x"][a0:a1], o["y"][a0:a1], o["z"][a0:a1]], 1)
        seq = [int(c) for c in direct.res_code]
        L = len(seq) + 3
        blobs = {}
        for layout in D.LAYOUTS:
            e = D.dense_expected(xyz, seq, int(direct.first_res_index[0]), has_oxt, layout, L, plddt=o["bfac_res"][r0:r0 + len(seq)])
            e["pos"][e["mask"] == 0] = np.nan                                  # masked-off values are no data
            b, refusal = U.batch_expected(e["pos"][None], e["mask"][None], e["aatype"][None], np.asarray([e["length"]]), layout,
                                          plddt=e["plddt"][None], first_res_index=e["res_index"][None, 0], first_atom_index=direct.first_atom_index,
                                          chain_id=direct.chain_id, titles=[title])
            assert not refusal.any(), (nm, layout)
            want = direct if layout == "atom37" else \
                flat_batch(o, i, title, keep=(lambda c: c != D.OXT_CODE) if layout == "atom14" else (lambda c: c < 4))[0]
            assert U.batches_equal(b, want) is None, (nm, layout, U.batches_equal(b, want))
            blob, off, st = H.oracle_compress(b)
            wblob, woff, wst = H.oracle_compress(want)
            assert st[0] == 0 and wst[0] == 0 and blob.tobytes() == wblob.tobytes(), (nm, layout)
            blobs[layout] = blob.tobytes()
        # atom14 differs from atom37 only by the OXT: header.nAtom (bytes 6-7) and the record's 13 OXT bytes (flag + coordinates)
        rec37, rec14 = fczfile.parse(blobs["atom37"]), fczfile.parse(blobs["atom14"])
        assert rec37.has_oxt == has_oxt and not rec14.has_oxt
        assert len(blobs["atom14"]) == len(blobs["atom37"])
        assert (blobs["atom14"] == blobs["atom37"]) == (not has_oxt), nm
        if has_oxt:
            diff = [k for k in range(len(blobs["atom37"])) if blobs["atom37"][k] != blobs["atom14"][k] and k not in (6, 7)]
            assert diff and max(diff) - min(diff) < 13, (nm, diff[:20])
            assert int.from_bytes(blobs["atom37"][6:8], "little") == int.from_bytes(blobs["atom14"][6:8], "little") + 1
    assert 0 < n_oxt < 56


def test_golden_inputs_by_atom_name_give_the_committed_records(golden):
    """the golden compress inputs whose atoms all have slots, gathered into atom37 by atom name and flattened again by the
    builder (canonical order instead of the file's), compress to the committed reference record"""
    z, index = golden
    used = 0
    for nm in compress_cases(index):
        gb = golden_batch(z, nm)
        if not U.all_atoms_have_slots(gb):
            continue
        used += 1
        L = gb.n_residues + 1
        d = U.dense_from_batch(gb, "atom37", L)
        title = bytes(gb.titles).decode("latin-1")
        b, refusal = U.batch_expected(d["pos"], d["mask"], d["aatype"], d["length"], "atom37", plddt=d["plddt"], first_res_index=gb.first_res_index,
                                      first_atom_index=gb.first_atom_index, chain_id=gb.chain_id, titles=[title], anchor_threshold=gb.anchor_threshold)
        assert not refusal.any() and b.n_atoms == gb.n_atoms, nm
        blob, off, st = H.oracle_compress(b)
        assert st[0] == 0 and blob.tobytes() == z[f"{nm}/fcz"].tobytes(), nm
    assert used >= 1


def test_aatype_map_is_the_inverse_of_the_dense_direction():
    for rc in range(24):
        aa = int(D.dense_expected(np.zeros((RES_NATOMS[rc], 3), np.float32), [rc], 1, False, "atom14", 1)["aatype"][0])
        assert aa == min(rc, 20)
        assert U.res_code_of_aatype(aa) == (rc if rc < 20 else U.UNK)
    assert [U.res_code_of_aatype(a) for a in range(21)] == list(range(20)) + [23]
    for bad in (21, 255):
        with pytest.raises(ValueError):
            U.res_code_of_aatype(bad)
    # refusals of the builder: a larger aatype, a row without CA, a length beyond L; neighbours stay
    pos = np.zeros((4, 3, 14, 3), np.float32); mask = np.zeros((4, 3, 14), np.uint8); mask[:, :, :4] = 1
    aatype = np.full((4, 3), 7, np.uint8); length = np.asarray([3, 3, 3, 4], np.uint32)
    aatype[1, 1] = 21; mask[2, 2, 1] = 0
    b, refusal = U.batch_expected(pos, mask, aatype, length, "atom14")
    assert list(refusal) == [0, U.E_RESIDUE, U.E_RESIDUE, U.E_INVALID_ARG] and list(b.res_off) == [0, 3, 3, 3, 3] and b.n_atoms == 12


def test_new_entry_points_are_exported_and_refuse_without_a_context():
    assert set(NEW) <= set(_lib.EXPORTS)
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name), name
    pos = np.zeros((1, 2, 37, 3), np.float32); mask = np.ones((1, 2, 37), np.uint8); aatype = np.zeros((1, 2), np.uint8)
    length = np.asarray([2], np.uint32)
    s = CDenseIn(pos.ctypes.data, mask.ctypes.data, aatype.ctypes.data, length.ctypes.data)
    counts = np.zeros(3, np.uint32); nbytes = ctypes.c_uint64(7); out = CChainBatch()
    # (no CPU fallback behind them: without a context nothing runs)
    assert lib.fcz_undense_dev(None, ctypes.byref(s), 1, 2, 0, 25, ctypes.byref(out), counts.ctypes.data, None) == -1
    assert lib.fcz_undense_fetch(None, None, None) == -1
    for begin in (lib.fcz_compress_dense_begin, lib.fcz_compress_dense_begin_dev):
        assert begin(None, ctypes.byref(s), 1, 2, 0, 25, counts.ctypes.data, ctypes.byref(nbytes)) == -1
        assert begin(None, ctypes.byref(s), 0, 2, 0, 25, counts.ctypes.data, ctypes.byref(nbytes)) == -1
    for fetch in (lib.fcz_compress_dense_fetch, lib.fcz_compress_dense_fetch_dev):
        assert fetch(None, None, None, None) == -1
    assert not counts.any()
