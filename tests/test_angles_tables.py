"""CPU: the chi table behind the angle tensors (fcz_chi_atom, the generated RES_CHI_SLOT), the exported names, and the meaning of the
table: the chi values the numpy helper (tests/_angles.py) reads out of the golden records are the dihedrals of the standard chi
quadruples, measured in float64 on the oracle's decoded coordinates."""
import os
import re

import numpy as np

import _angles as A
import _harness as H
from _cases import entries_blob, golden_records
from foldcomp_amd import _aa_tables as T
from foldcomp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# chi k -> atom per residue type; every other type, and codes 20 .. 23, have no such chi
CHI = [
    {**{r: "CG" for r in "ARG ASN ASP GLN GLU HIS LEU LYS MET PHE PRO TRP TYR".split()}, "CYS": "SG", "ILE": "CG1", "VAL": "CG1", "SER": "OG",
     "THR": "OG1"},
    {**{r: "CD" for r in "ARG GLN GLU LYS PRO".split()}, "ASN": "OD1", "ASP": "OD1", "HIS": "ND1",
     **{r: "CD1" for r in "ILE LEU PHE TRP TYR".split()}, "MET": "SD"},
    {"ARG": "NE", "GLN": "OE1", "GLU": "OE1", "LYS": "CE", "MET": "CE"},
    {"ARG": "CZ", "LYS": "NZ"},
]
NEW = ["fcz_chi_atom", "fcz_angles_dev", "fcz_angles_packed_dev", "fcz_decompress_angles", "fcz_decompress_angles_packed"]


def test_chi_atom_is_the_table():
    lib = _lib.load()
    for rc in range(24):
        for k in range(4):
            name = CHI[k].get(T.RES3[rc]) if rc < 20 else None
            want = T.ATOM_NAMES.index(name) if name else -1
            assert lib.fcz_chi_atom(rc, k) == want, (T.RES3[rc], k)
            slot = T.RES_CHI_SLOT[rc][k]
            assert (T.RES_ATOMS[rc][slot] if slot else -1) == want, (T.RES3[rc], k)
            assert slot == 0 or 5 <= slot <= 8          # the kernel reads a residue's chi bytes from its first eight torsion bytes
    for rc, k in ((-1, 0), (24, 0), (1, -1), (1, 4)):
        assert lib.fcz_chi_atom(rc, k) == -1


def test_chi_atoms_are_placed_by_the_chi_quadruple():
    """the predecessor triple of the atom chi k names is the standard chi quadruple's first three atoms: N CA CB for chi1, then the
    chain moves on by one atom per chi"""
    lib = _lib.load()
    for rc in range(20):
        chain = ["N", "CA", "CB"]
        for k in range(4):
            code = lib.fcz_chi_atom(rc, k)
            if code < 0:
                continue
            slot = T.RES_ATOMS[rc].index(code)
            assert [T.ATOM_NAMES[T.RES_ATOMS[rc][p]] for p in T.RES_PREV[rc][slot]] == chain[-3:], (T.RES3[rc], k)
            chain.append(T.ATOM_NAMES[code])
        assert all(lib.fcz_chi_atom(rc, j) < 0 for j in range(len(chain) - 3, 4))   # no chi behind a missing one


def test_new_symbols_are_exported():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "fcz_hip.h")).read()
    for name in NEW:
        assert name in _lib.EXPORTS
        assert re.search(r"\b%s\(" % name, hdr)
        assert getattr(lib, name) is not None
    assert re.search(r"#define FCZ_ANGLE_COLUMNS 10\b", hdr)
    import foldcomp_amd as foldcomp
    assert foldcomp.ANGLE_COLUMNS == ("phi", "psi", "omega", "n_ca_c", "ca_c_n", "c_n_ca", "chi1", "chi2", "chi3", "chi4")
    assert callable(foldcomp.decode_angles) and len(foldcomp.ANGLE_COLUMNS) == A.COLS


def test_helper_contract_on_a_golden_record(golden):
    ang, msk = A.entry_expected(golden_records(golden)[0])
    n = len(ang)
    assert not msk[0, [0, 3]].any() and msk[1:, [0, 3]].all()
    assert not msk[n - 1, [1, 2, 4, 5]].any() and msk[:n - 1, [1, 2, 4, 5]].all()
    assert not ang[msk == 0].view(np.uint32).any()
    assert A.entry_expected(b"FCMP" + bytes(100)) is None and A.entry_expected(b"") is None


def dihedral(p0, p1, p2, p3):
    b0, b1, b2 = p0 - p1, p2 - p1, p3 - p2
    b1 = b1 / np.linalg.norm(b1, axis=-1, keepdims=True)
    v = b0 - (b0 * b1).sum(-1, keepdims=True) * b1
    w = b2 - (b2 * b1).sum(-1, keepdims=True) * b1
    return np.degrees(np.arctan2((np.cross(b1, v) * w).sum(-1), (v * w).sum(-1)))


# largest |chi from the record - chi measured on the oracle's atoms| over the golden records, degrees modulo 360, as this test
# prints it; the bound is twice that
OBSERVED_MAX_DEG = 6.98e-4
CHI_TOL_DEG = 2 * OBSERVED_MAX_DEG


def test_chi_values_are_the_dihedrals_of_the_decoded_atoms(golden):
    recs = golden_records(golden)
    o = H.oracle_decompress(*entries_blob(recs))
    xyz = np.stack([o["x"], o["y"], o["z"]], 1).astype(np.float64)
    worst, count = 0.0, 0
    for i, raw in enumerate(recs):
        ang, msk = A.entry_expected(raw)
        rc = A.res_codes(A.decodes(raw))
        assert np.array_equal(rc, o["res_code"][o["res_off"][i]:o["res_off"][i + 1]])
        first = int(o["atom_off"][i]) + np.concatenate([[0], np.cumsum([T.RES_NATOMS[c] for c in rc])[:-1]])
        for l, c in enumerate(rc):
            for k, slot in enumerate(T.RES_CHI_SLOT[c]):
                assert bool(msk[l, 6 + k]) == bool(slot)
                if slot:
                    q = [xyz[first[l] + p] for p in T.RES_PREV[c][slot]] + [xyz[first[l] + slot]]
                    d = abs((float(dihedral(*q)) - float(ang[l, 6 + k]) + 180.0) % 360.0 - 180.0)
                    worst, count = max(worst, d), count + 1
    print(f"chi table: {count} chi angles of {len(recs)} golden records, largest deviation {worst:.3e} degrees (bound {CHI_TOL_DEG:.3e})")
    assert count > 1000
    assert worst <= CHI_TOL_DEG, worst
