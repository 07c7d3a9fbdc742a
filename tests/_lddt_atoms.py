"""The all-atom lDDT with symmetric side-chain renaming restated in numpy (include/fcz_hip.h, fcz_lddt_atoms_dev), and the device
calls into 0xA5-filled arrays.

One chain at a time, float32 throughout (numpy rounds every operation and fuses none; the atoms x atoms matrices are built the way
_lddt._d builds its rows x rows ones): first EVERY row of the chain is decided against the dense (ambiguous atoms x anchors)
matrices of the two namings, then the renamed truth is built as whole arrays, then the chain's atoms are scored against each other.
Nothing here is shared with the kernel's lane-per-query sweeps, its tiles or its passes."""
import ctypes

import numpy as np

from _analysis import bits, chains_of, ptr, to14  # noqa: F401  (to14: re-exported for the tests)
from _dense import expected_slot
from _devpath import GUARD, DevGuarded
from _lddt import THRESHOLDS, _d, score_of
from foldcomp_amd._aa_tables import ATOM_NAMES

F = np.float32
WIDTH_LAYOUT = {37: "atom37", 14: "atom14", 4: "backbone4"}
LAYOUT = {37: 0, 14: 1, 4: 2}
ASP, GLU, PHE, TYR, VAL = 3, 6, 13, 18, 19
SWAPS = {ASP: [("OD1", "OD2")], GLU: [("OE1", "OE2")], PHE: [("CD1", "CD2"), ("CE1", "CE2")], TYR: [("CD1", "CD2"), ("CE1", "CE2")]}
ROW_KEYS = ("score", "pairs", "hits", "swapped")
KEYS = ROW_KEYS + ("atom_pairs", "atom_hits")
DTYPES = dict(score=np.float32, pairs=np.int32, hits=np.int32, swapped=np.uint8, atom_pairs=np.int32, atom_hits=np.int32)


def table_of(A, swaps):
    """{type: [(name, name)]} -> uint8 [21, A] through the slot names of the layout (tests/_dense.py)"""
    t = np.tile(np.arange(A, dtype=np.uint8), (21, 1))
    for ty, pairs in swaps.items():
        for a, b in pairs:
            x, y = (expected_slot(WIDTH_LAYOUT[A], ty, ATOM_NAMES.index(nm)) for nm in (a, b))
            if x >= 0 and y >= 0:
                t[ty, x], t[ty, y] = y, x
    return t


def default_table(A):
    return table_of(A, SWAPS)


def max_rows(A):
    return (2 ** 31 - 1) // (4 * A * A)


def _finite(x):
    with np.errstate(invalid="ignore"):
        return np.isfinite(x).all(axis=-1)


def _count(dt, dp, inc, cutoff, th):
    """distance matrices [q, c] and the pairs that may count -> (pairs [q], hits [q]) as int64"""
    inc = inc & (dt < cutoff)
    with np.errstate(invalid="ignore"):
        diff = np.abs(dt - dp)
    assert diff.dtype == np.float32
    return inc.sum(axis=1).astype(np.int64), sum(((diff < v) & inc).sum(axis=1) for v in th).astype(np.int64)


def decide_chain(pt, mt, pp, mp, partner, cutoff, th):
    """one chain, partner int [m, A] -> swapped uint8 [m]"""
    m, A = mt.shape
    own = np.arange(A)[None, :]
    amb = partner != own
    present = (mt != 0) & (mp != 0) & _finite(pt) & _finite(pp)
    swapped = np.zeros(m, np.uint8)
    anchor = present & ~amb
    arow = np.argwhere(anchor)[:, 0]
    at, ap = np.ascontiguousarray(pt[anchor]), np.ascontiguousarray(pp[anchor])
    for r in np.flatnonzero(amb.any(axis=1) & (present | ~amb).all(axis=1)):
        slots = np.flatnonzero(amb[r])
        other = np.broadcast_to(arow[None, :] != r, (len(slots), len(arow)))
        dp = _d(ap, pp[r, slots])
        P0, H0 = (int(v.sum()) for v in _count(_d(at, pt[r, slots]), dp, other, cutoff, th))
        P1, H1 = (int(v.sum()) for v in _count(_d(at, pt[r, partner[r, slots]]), dp, other, cutoff, th))
        swapped[r] = 1 if H1 * P0 > H0 * P1 else 0
    return swapped


def lddt_atoms_chain(pt, mt, pp, mp, aatype, table, cutoff=15.0, thresholds=THRESHOLDS):
    """one chain: pos float32 [m, A, 3], masks [m, A] (mp may be None), aatype [m] or None, table [21, A] or None -> dict of KEYS"""
    pt, pp = np.asarray(pt, F), np.asarray(pp, F)
    mt = np.asarray(mt)
    m, A = mt.shape
    mp = np.ones((m, A), np.uint8) if mp is None else np.asarray(mp)
    cutoff = F(cutoff)
    th = [F(v) for v in thresholds]
    own = np.broadcast_to(np.arange(A)[None, :], (m, A))
    partner = own if aatype is None or table is None else np.asarray(table)[np.minimum(np.asarray(aatype), 20)].astype(np.int64)
    # 1. every row of the chain is decided
    swapped = decide_chain(pt, mt, pp, mp, partner, cutoff, th)
    # 2. the renamed truth
    sel = np.where(swapped[:, None] != 0, partner, own)
    rt = np.take_along_axis(pt, sel[:, :, None], axis=1)
    rm = np.take_along_axis(mt, sel, axis=1)
    atom = (rm != 0) & (mp != 0) & _finite(rt) & _finite(pp)
    idx = np.argwhere(atom)
    row = idx[:, 0]
    T, P = np.ascontiguousarray(rt[atom]), np.ascontiguousarray(pp[atom])
    out = dict(swapped=swapped, atom_pairs=np.zeros((m, A), np.int32), atom_hits=np.zeros((m, A), np.int32))
    # 3. the score
    for q0 in range(0, len(idx), 256):
        q = slice(q0, q0 + 256)
        pairs, hits = _count(_d(T, T[q]), _d(P, P[q]), row[None, :] != row[q, None], cutoff, th)
        out["atom_pairs"][idx[q, 0], idx[q, 1]] = pairs
        out["atom_hits"][idx[q, 0], idx[q, 1]] = hits
    out["pairs"] = out["atom_pairs"].sum(axis=1, dtype=np.int64).astype(np.int32)
    out["hits"] = out["atom_hits"].sum(axis=1, dtype=np.int64).astype(np.int32)
    out["score"] = score_of(out["pairs"], out["hits"])
    return out


def lddt_atoms(pos_t, mask_t, pos_p, mask_p, aatype, bound, table, cutoff=15.0, thresholds=THRESHOLDS, packed=False):
    """pos [n, L, A, 3] / [R, A, 3], masks (mask_p may be None), aatype or None, length [n] / None or row_off [n + 1] (ranges must not
    overlap), table [21, A] or None -> dict of KEYS; rows outside every chain hold 0"""
    lead, A = pos_t.shape[:-2], pos_t.shape[-2]
    out = {k: np.zeros(lead + ((A,) if k.startswith("atom_") else ()), DTYPES[k]) for k in KEYS}
    for sel, _, m in chains_of(pos_t.shape, bound, packed):
        if m == 0:
            continue
        got = lddt_atoms_chain(pos_t[sel], mask_t[sel], pos_p[sel], None if mask_p is None else mask_p[sel], None if aatype is None else aatype[sel],
                               table, cutoff, thresholds)
        for k in KEYS:
            out[k][sel] = got[k]
    return out


def chain_quotient(pairs, hits):
    """-> float64(sum hits) / float64(4 * sum pairs) from int64 sums, 0 where there is no pair"""
    p, h = int(np.sum(pairs, dtype=np.int64)), int(np.sum(hits, dtype=np.int64))
    return np.float64(h) / np.float64(4 * p) if p else np.float64(0)


def same(got, exp, what="", keys=KEYS):
    """integers equal, floats on bits"""
    for k in keys:
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        assert g.shape == e.shape, (what, k, g.shape, e.shape)
        if k == "score":
            assert g.dtype == e.dtype == np.float32, (what, k, g.dtype, e.dtype)
            g, e = bits(g), bits(e)
        elif k == "swapped":
            g, e = g.view(np.uint8), e.view(np.uint8)
        else:
            assert g.dtype == e.dtype == DTYPES[k], (what, k, g.dtype, e.dtype)
        assert np.array_equal(g, e), (what, k, np.argwhere(g != e)[:4], g[g != e][:4], e[g != e][:4])


def exchange(pos, aatype, rows, table):
    """pos [.., A, 3] with the partnered slots of the rows where `rows` [..] is set exchanged under `table`"""
    A = pos.shape[-2]
    partner = np.asarray(table)[np.minimum(aatype, 20)].astype(np.int64)
    sel = np.where(np.asarray(rows, bool)[..., None], partner, np.arange(A))
    return np.take_along_axis(pos, sel[..., None], axis=-2)


def out_spec(lead, A, keys=KEYS):
    """the outputs in `keys` for rows shaped `lead` of width A as a guard's spec"""
    return {k: (DTYPES[k], tuple(lead) + ((A,) if k.startswith("atom_") else ())) for k in keys}


class Outputs:
    """the device outputs, 0xA5 everywhere with guard bytes on both sides"""

    def __init__(self, lead, A, guard=GUARD):
        self.rows = DevGuarded(out_spec(lead, A, ROW_KEYS), guard)
        self.atoms = DevGuarded(out_spec(lead, A, KEYS[4:]), guard)

    def struct(self, per_atom=True, **replace):
        from foldcomp_amd.structure import CLddtAtomsOut
        at = dict(zip(KEYS, self.rows.ptrs() + (self.atoms.ptrs() if per_atom else [None, None])))
        at.update(replace)
        return CLddtAtomsOut(*(at[k] for k in KEYS))

    def fetch(self, per_atom=True):
        out = dict(zip(ROW_KEYS, self.rows.all()))
        if per_atom:
            out.update(zip(KEYS[4:], self.atoms.all()))
        else:
            assert self.atoms.untouched()
        return out

    def untouched(self):
        return self.rows.untouched() and self.atoms.untouched()


def run_dev(codec, pt, mt, pp, mp, aa, bound_t, n, rows, layout, packed, table=None, cutoff=15.0, thresholds=None, per_atom=True, guard=GUARD, expect=0):
    """fcz_lddt_atoms_dev (rows = L) or fcz_lddt_atoms_packed_dev (rows = R) on device tensors -> dict of the outputs as numpy, guards
    checked; table: uint8 [21, A] on the host or None"""
    import torch
    o = Outputs((rows,) if packed else (n, rows), {0: 37, 1: 14, 2: 4}[layout], guard)
    fn = codec.lib.fcz_lddt_atoms_packed_dev if packed else codec.lib.fcz_lddt_atoms_dev
    tab = None if table is None else np.ascontiguousarray(table, np.uint8)
    th = None if thresholds is None else np.asarray(thresholds, np.float32)
    c_out = o.struct(per_atom)
    torch.cuda.synchronize()
    rc = fn(codec.ctx, pt.data_ptr(), mt.data_ptr(), pp.data_ptr(), ptr(mp), ptr(aa), ptr(bound_t), n, rows, layout, float(cutoff),
            None if th is None else th.ctypes.data, None if tab is None else tab.ctypes.data, ctypes.byref(c_out))
    codec.synchronize()
    assert rc == expect, rc
    return o.fetch(per_atom)
