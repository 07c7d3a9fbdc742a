"""CPU: the dense-layout tables of the C-ABI (fcz_dense_width / fcz_dense_slot: pure host code, the table the kernel is handed),
the numpy builder of expected tensors (tests/_dense.py) pinned against the golden records alone, and the entry points' refusal
to run without a context."""
import subprocess
import sys

import numpy as np

import _dense as D
from _cases import compress_cases, db_cases
from foldcomp_amd import _lib
from foldcomp_amd._aa_tables import ATOM_NAMES, RES_ATOMS, RES_NATOMS


def test_dense_width():
    lib = _lib.load()
    assert [lib.fcz_dense_width(v) for v in (0, 1, 2)] == [37, 14, 4]
    assert [lib.fcz_dense_width(v) for v in (-1, 3, 255)] == [-1, -1, -1]


def test_dense_slot_tables():
    lib = _lib.load()
    # the list of the issue, written out: atom37 slot = position of the atom's name
    atom37 = ("N CA C CB O CG CG1 CG2 OG OG1 SG CD CD1 CD2 ND1 ND2 OD1 OD2 SD CE CE1 CE2 CE3 NE NE1 NE2 OE1 OE2 CH2 NH1 NH2 OH CZ "
              "CZ2 CZ3 NZ OXT").split()
    assert len(atom37) == 37 and atom37 == D.ATOM37 and sorted(atom37) == sorted(ATOM_NAMES)
    for res in range(24):
        for name, lay in D.LAYOUTS.items():
            slots = [lib.fcz_dense_slot(lay, res, code) for code in RES_ATOMS[res]]
            kept = [s for s in slots if s >= 0]
            assert len(set(kept)) == len(kept), (name, res)                        # injective
            assert all(0 <= s < D.WIDTH[name] for s in kept)
            if name == "atom37":
                assert slots == [atom37.index(ATOM_NAMES[code]) for code in RES_ATOMS[res]], res
            elif name == "atom14":
                assert slots == list(range(RES_NATOMS[res])), res
            else:
                assert slots == [code if code < 4 else -1 for code in RES_ATOMS[res]], res
            assert lib.fcz_dense_slot(lay, res, 36) == (36 if name == "atom37" else -1)
            # atoms the residue does not have, the "other" code, codes out of range
            for code in list(range(36)) + [37, 254, 255, -1]:
                if code not in RES_ATOMS[res]:
                    assert lib.fcz_dense_slot(lay, res, code) == -1, (name, res, code)
            # the helper's own table says the same
            for code in range(-1, 40):
                assert lib.fcz_dense_slot(lay, res, code) == D.expected_slot(name, res, code)
    for lay in (0, 1, 2):
        for res in (-1, 24, 31, 255):
            assert lib.fcz_dense_slot(lay, res, 1) == -1
    assert lib.fcz_dense_slot(3, 0, 1) == -1 and lib.fcz_dense_slot(-1, 0, 1) == -1
    # TRP fills all of atom14; GLY has no CB, UNK has N, CA, C only
    assert sorted(lib.fcz_dense_slot(1, 17, c) for c in RES_ATOMS[17]) == list(range(14))
    assert lib.fcz_dense_slot(0, 7, 4) == -1 and [lib.fcz_dense_slot(0, 23, c) for c in range(5)] == [0, 1, 2, -1, -1]


def test_expected_builder_against_goldens(golden):
    z, index = golden
    names = compress_cases(index) + db_cases(index)
    assert len(names) == 56
    n_oxt = n_unk = n_alt = longest = 0
    for nm in names:
        fcz = z[f"{nm}/fcz"].tobytes()
        seq, first, has_oxt = D.record_fields(fcz)
        xyz0 = z[f"{nm}/xyz0"]
        n_atoms = sum(RES_NATOMS[c] for c in seq)
        assert len(xyz0) == n_atoms + has_oxt, nm
        n_oxt += has_oxt; n_unk += 23 in seq; longest = max(longest, len(seq))
        nums = D.pdb_residue_numbers(z[f"{nm}/pdb0"].tobytes())
        assert nums == list(range(first, first + len(seq))), nm                  # residue numbers run on from the first
        for lay in D.LAYOUTS:
            d = D.dense_expected(xyz0, seq, first, has_oxt, lay, len(seq))
            want = n_atoms + has_oxt if lay == "atom37" else n_atoms if lay == "atom14" else \
                sum(sum(c < 4 for c in RES_ATOMS[r]) for r in seq)
            assert int(d["mask"].sum()) == want, (nm, lay)
            assert not d["pos"][d["mask"] == 0].view(np.uint32).any()
            assert list(d["res_index"]) == nums and list(d["aatype"]) == [min(c, 20) for c in seq]
        # cropped and padded forms of the same entry
        full = D.dense_expected(xyz0, seq, first, has_oxt, "atom37", len(seq))
        crop = D.dense_expected(xyz0, seq, first, has_oxt, "atom37", len(seq) - 1)
        assert np.array_equal(crop["pos"].view(np.uint32), full["pos"][:-1].view(np.uint32)) and crop["length"] == len(seq)
        assert not crop["mask"][:, 36].any()
        pad = D.dense_expected(xyz0, seq, first, has_oxt, "atom37", len(seq) + 5)
        assert np.array_equal(pad["mask"][:len(seq)], full["mask"]) and not pad["mask"][len(seq):].any()
        assert list(pad["aatype"][len(seq):]) == [20] * 5 and not pad["res_index"][len(seq):].any()
        if f"{nm}/xyz1" in z.files:
            n_alt += 1
            alt = D.dense_expected(D.canonical_from_alt(z[f"{nm}/xyz1"], seq, has_oxt), seq, first, has_oxt, "atom37", len(seq))
            assert np.array_equal(alt["pos"].view(np.uint32), full["pos"].view(np.uint32)), nm
            assert np.array_equal(alt["mask"], full["mask"]), nm
    assert (n_oxt, n_unk, n_alt, longest) == (27, 2, 54, 1400)


def test_dense_entry_points_refuse_a_null_ctx():
    lib = _lib.load()
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data
    from foldcomp_amd.structure import CAtomsOut, CDenseOut
    import ctypes
    atoms = CAtomsOut(p, p, p, p, p, None); out = CDenseOut(p, p, p, p, p, p)
    assert lib.fcz_dense_dev(None, p, p, 1, p, p, ctypes.byref(atoms), 0, 0, 8, ctypes.byref(out)) == -1
    L = ctypes.c_uint32(0)
    assert lib.fcz_decompress_dense(None, p, p, 1, 0, 0, ctypes.byref(L), ctypes.byref(out), None) == -1
    assert not buf.any()


def test_tensors_module_does_not_import_torch():
    code = ("import sys; import foldcomp, foldcomp_amd.tensors; assert 'torch' not in sys.modules, 'torch imported'; "
            "assert foldcomp.decode_tensors is foldcomp_amd.tensors.decode_tensors; "
            "assert hasattr(foldcomp.FoldcompDatabase, 'tensor_batches')")
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
