"""Shared helpers of the dense-tensor tests: the expected atom37 / atom14 / backbone4 arrays in plain numpy, built from a flat atom
list in canonical order (the reference's own output), and the header fields of a golden record they need."""
import numpy as np

from foldcomp_amd import fczfile
from foldcomp_amd._aa_tables import ATOM_NAMES, RES1, RES_ALT_SLOT, RES_ATOMS, RES_NATOMS

# AlphaFold / OpenFold `atom_types`: the atom37 slot of an atom is the position of its name here
ATOM37 = ["N", "CA", "C", "CB", "O", "CG", "CG1", "CG2", "OG", "OG1", "SG", "CD", "CD1", "CD2", "ND1", "ND2", "OD1", "OD2", "SD", "CE",
          "CE1", "CE2", "CE3", "NE", "NE1", "NE2", "OE1", "OE2", "CH2", "NH1", "NH2", "OH", "CZ", "CZ2", "CZ3", "NZ", "OXT"]
LAYOUTS = {"atom37": 0, "atom14": 1, "backbone4": 2}
WIDTH = {"atom37": 37, "atom14": 14, "backbone4": 4}
OXT_CODE = 36


def expected_slot(layout, res_code, atom_code):
    """the slot table of the issue, restated without the library: -1 = no slot"""
    if not 0 <= res_code < 24 or not 0 <= atom_code < 37:
        return -1
    if atom_code == OXT_CODE:
        return 36 if layout == "atom37" else -1
    if atom_code not in RES_ATOMS[res_code]:
        return -1
    if layout == "atom37":
        return ATOM37.index(ATOM_NAMES[atom_code])
    if layout == "atom14":
        return RES_ATOMS[res_code].index(atom_code)
    return atom_code if atom_code < 4 else -1


def canonical_from_alt(xyz1, seq, has_oxt):
    """atoms in the `-a` order -> canonical order (position j of the alt list holds canonical slot RES_ALT_SLOT[res][j])"""
    out = np.array(xyz1, copy=True)
    a = 0
    for rc in seq:
        for j, slot in enumerate(RES_ALT_SLOT[rc]):
            out[a + slot] = xyz1[a + j]
        a += RES_NATOMS[rc]
    assert a + (1 if has_oxt else 0) == len(xyz1)
    return out


def dense_expected(xyz, seq, first_res_index, has_oxt, layout, L, plddt=None):
    """one entry: xyz float32 [atoms, 3] in canonical order (OXT last when has_oxt), seq = residue codes 0 .. 23 ->
    dict(pos [L, A, 3], mask [L, A], aatype [L], res_index [L], plddt [L] when given, length)"""
    A = WIDTH[layout]
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(seq)
    assert len(xyz) == sum(RES_NATOMS[rc] for rc in seq) + (1 if has_oxt else 0)
    pos = np.zeros((L, A, 3), np.float32); mask = np.zeros((L, A), np.uint8)
    aatype = np.full(L, 20, np.uint8); res_index = np.zeros(L, np.int32); pl = np.zeros(L, np.float32)
    a = 0
    for l, rc in enumerate(seq):
        if l < L:
            for j, code in enumerate(RES_ATOMS[rc]):
                s = expected_slot(layout, rc, code)
                if s >= 0:
                    pos[l, s] = xyz[a + j]; mask[l, s] = 1
            aatype[l] = min(rc, 20)
            res_index[l] = first_res_index + l
            if plddt is not None:
                pl[l] = plddt[l]
        a += RES_NATOMS[rc]
    if has_oxt and layout == "atom37" and n <= L:        # a cropped entry loses its OXT with its last residue
        pos[n - 1, 36] = xyz[a]; mask[n - 1, 36] = 1
    d = dict(pos=pos, mask=mask, aatype=aatype, res_index=res_index, length=n)
    if plddt is not None:
        d["plddt"] = pl
    return d


def record_fields(fcz: bytes):
    """-> (seq as decoded: the first residue from header.firstResidue, codes clamped to UNK; first_res_index; has_oxt)"""
    rec = fczfile.parse(fcz)
    seq = [int(c) for c in rec.res_codes]
    seq[0] = RES1.index(rec.first_residue) if rec.first_residue in RES1 else 23
    seq = [c if c < 24 else 23 for c in seq]
    return seq, rec.first_res_index, rec.has_oxt


def pdb_residue_numbers(pdb_text: bytes):
    """residue numbers (columns 23-26) of the ATOM records, one per residue in file order; the OXT line (which the reference
    numbers header.nResidue) is left out"""
    out, prev = [], None
    for line in pdb_text.decode("latin-1").split("\n"):
        if not line.startswith("ATOM") or line[12:16].strip() == "OXT":
            continue
        num = int(line[22:26])
        if num != prev:
            out.append(num); prev = num
    return out


def stack_expected(per_entry, L, A, keys=("pos", "mask", "aatype", "res_index", "plddt")):
    """list of dense_expected dicts -> batch arrays"""
    d = {k: np.stack([e[k] for e in per_entry]) for k in keys if all(k in e for e in per_entry)}
    d["length"] = np.asarray([e["length"] for e in per_entry], np.uint32)
    return d
