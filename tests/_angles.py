"""Shared helper of the angle-tensor tests: the expected output of fcz_angles_dev / fcz_angles_packed_dev in pure numpy, and the
batches both test files use.

The output contract restated (include/fcz_hip.h): per residue row ten float32 in degrees and ten mask bytes. For an entry of n
residues, row l holds
    0 phi     = `phi` of word l-1       for 1 <= l <= n-1        3 N-CA-C at l       = `n_ca_c` of word l-1   for 1 <= l <= n-1
    1 psi     = `psi` of word l         for l <= n-2             4 CA-C-N(l+1)       = `ca_c_n` of word l     for l <= n-2
    2 omega   = `omega` of word l       for l <= n-2             5 C-N(l+1)-CA(l+1)  = `c_n_ca` of word l     for l <= n-2
    6 .. 9 chi1 .. chi4 = the side-chain torsion byte of the atom in canonical slot RES_CHI_SLOT[code][k], where that is not 0
columns 0 .. 5 dequantised by fczfile.angle_lists (the header's min / cont_f pairs), the chis by the oracle's fixed-angle quantiser
(quant_fixed_angle, oracle/fcz_oracle.c: min -180, max 180, 255 steps); 0.0f where the mask is 0. A residue's torsion bytes start
at the sum of natoms - 3 over the residues in front of it; its code is the decoder's (residue 0: header.firstResidue, codes above
23 clamped to 23). Padded: [n][L][10], an entry longer than L keeps its first L rows, rows behind its length are 0 / 0, an entry
that does not decode is all 0 / 0. Packed: the rows of the entries that decode back to back."""
import numpy as np

import _harness as H
from foldcomp_amd import _aa_tables as T
from foldcomp_amd import fczfile, synthetic

COLS = 10
FIXED_MIN, FIXED_MAX, FIXED_STEPS = np.float32(-180.0), np.float32(180.0), np.float32(255)
FIXED_CONT = np.float32((FIXED_MAX - FIXED_MIN) / FIXED_STEPS)        # quant_fixed_angle().cont_f


def res_codes(rec) -> np.ndarray:
    """the residue codes the decoder uses"""
    rc = rec.res_codes.astype(np.int64).copy()
    rc[0] = T.RES1.index(rec.first_residue) if rec.first_residue in T.RES1 else 23
    rc[rc >= 24] = 23
    return rc


def decodes(raw: bytes):
    """the parsed record when the decoder accepts it (what the sizes pass checks), else None"""
    try:
        rec = fczfile.parse(raw)
    except fczfile.FczFormatError:
        return None
    if rec.n_residues < 2 or rec.n_anchors < 2:
        return None
    rc = res_codes(rec)
    if ((rc >= 20) & (rc != 23)).any() or int(sum(T.RES_NATOMS[c] - 3 for c in rc)) != rec.n_sidechain:
        return None
    return rec


def entry_expected(raw: bytes):
    """-> (angles float32 [n, 10], mask uint8 [n, 10]) of one record, None when it does not decode"""
    rec = decodes(raw)
    if rec is None:
        return None
    n = rec.n_residues
    a = fczfile.angle_lists(rec)
    bonds = a["bond_angles"].reshape(n, 3)                            # per word: ca_c_n, c_n_ca, n_ca_c
    ang = np.zeros((n, COLS), np.float32)
    msk = np.zeros((n, COLS), np.uint8)
    ang[1:, 0] = a["phi"][:n - 1]; msk[1:, 0] = 1
    ang[:n - 1, 1] = a["psi"][:n - 1]; msk[:n - 1, 1] = 1
    ang[:n - 1, 2] = a["omega"][:n - 1]; msk[:n - 1, 2] = 1
    ang[1:, 3] = bonds[:n - 1, 2]; msk[1:, 3] = 1
    ang[:n - 1, 4] = bonds[:n - 1, 0]; msk[:n - 1, 4] = 1
    ang[:n - 1, 5] = bonds[:n - 1, 1]; msk[:n - 1, 5] = 1
    rc = res_codes(rec)
    own = np.array([T.RES_NATOMS[c] - 3 for c in rc], np.int64)
    start = np.concatenate([[0], np.cumsum(own)[:-1]])
    sc = np.frombuffer(raw, np.uint8, rec.n_sidechain, rec.o_sc)
    for l in range(n):
        for k, slot in enumerate(T.RES_CHI_SLOT[rc[l]]):
            if slot:
                ang[l, 6 + k] = (np.float32(sc[start[l] + slot - 3]) * FIXED_CONT) + FIXED_MIN
                msk[l, 6 + k] = 1
    return ang, msk


def padded_expected(entries, L):
    ang = np.zeros((len(entries), L, COLS), np.float32)
    msk = np.zeros((len(entries), L, COLS), np.uint8)
    for i, e in enumerate(entries):
        x = e if isinstance(e, tuple) or e is None else entry_expected(e)
        if x is not None:
            k = min(L, len(x[0]))
            ang[i, :k] = x[0][:k]; msk[i, :k] = x[1][:k]
    return ang, msk


def packed_expected(entries):
    """-> (angles [R, 10], mask [R, 10], row_off [n + 1])"""
    xs = [e if isinstance(e, tuple) or e is None else entry_expected(e) for e in entries]
    lens = [0 if x is None else len(x[0]) for x in xs]
    ang = np.concatenate([x[0] for x in xs if x is not None] + [np.zeros((0, COLS), np.float32)])
    msk = np.concatenate([x[1] for x in xs if x is not None] + [np.zeros((0, COLS), np.uint8)])
    return ang, msk, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)


def longest(entries) -> int:
    return max([0] + [len(x[0]) for x in map(entry_expected, entries) if x is not None])


def synthetic_records(lengths, seed, res_code=None):
    """synthetic chains of the given lengths compressed by the oracle -> list of records"""
    b = synthetic.to_chain_batch(synthetic.generate(len(lengths), list(lengths), seed=seed, res_code=res_code))
    blob, off, st = H.oracle_compress(b)
    assert (st == 0).all(), st
    return [blob[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(lengths))]


_BATCHES = {}


def batches(golden_recs):
    """name -> list of records: the inputs of the GPU test, built once"""
    if not _BATCHES:
        mixed = synthetic_records([2, 3, 16, 17, 64, 65, 257, 1100], seed=11)
        gly = synthetic_records([70], seed=12, res_code=7)
        trp = synthetic_records([150], seed=13, res_code=17)
        _BATCHES.update(
            golden=list(golden_recs),
            synthetic=mixed,
            all_gly=mixed[3:6] + gly,
            trp_last=mixed[1:5] + trp,
            single=[mixed[6]],
            truncated=[mixed[4], mixed[5][:len(mixed[5]) - 40], mixed[3]])
    return _BATCHES
