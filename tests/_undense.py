"""Shared helpers of the tensors -> FCZ tests: the ChainBatch the undense stage must build from dense arrays, in plain numpy,
restating the contract of include/fcz_hip.h (fcz_dense_in) without the library; and the way there from a flat batch (atoms placed
by their names), with garbage for everything the contract says is never read."""
import numpy as np

import _dense as D
from foldcomp_amd._aa_tables import RES_ATOMS, RES_NATOMS
from foldcomp_amd.structure import ChainBatch

E_INVALID_ARG, E_RESIDUE, E_TOO_SHORT, E_NONFINITE = -1, -6, -7, -9
UNK = 23


def res_code_of_aatype(aa: int) -> int:
    """aatype 0 .. 19 (A R N D C Q E G H I L K M F P S T W Y V) are the codec's residue codes 0 .. 19; 20 is UNK; more is refused"""
    if not 0 <= aa <= 20:
        raise ValueError(aa)
    return aa if aa < 20 else UNK


def slot_table(layout):
    """[24, 14]: slot of the residue's canonical atom j in the layout, -1 = none"""
    t = np.full((24, 14), -1, np.int64)
    for rc in range(24):
        for j in range(RES_NATOMS[rc]):
            t[rc, j] = D.expected_slot(layout, rc, RES_ATOMS[rc][j])
    return t


def batch_expected(pos, mask, aatype, length, layout, plddt=None, first_res_index=None, first_atom_index=None, chain_id=None,
                   titles=None, anchor_threshold=25):
    """dense arrays -> (ChainBatch, refusal int32[n]): per chain the rows l < length[c]; per row the residue type's own slots
    whose mask is set, in canonical order; the chain's OXT (atom37: slot 36 of the last row) as the last atom of the last residue.
    A refused chain (length > L or > 65535: -1; aatype > 20 or a row without N, CA, C: -6) has zero residues and keeps its title."""
    mask = np.asarray(mask) != 0
    n, L, A = mask.shape
    assert A == D.WIDTH[layout] and pos.shape == (n, L, A, 3) and aatype.shape == (n, L)
    T = slot_table(layout)
    codes = np.full((24, 14), 255, np.int64)
    for rc in range(24):
        codes[rc, :RES_NATOMS[rc]] = RES_ATOMS[rc]
    refusal = np.zeros(n, np.int32)
    res_off, atom_counts, xyz, acode, rcode, bfac = [0], [], [], [], [], []
    for c in range(n):
        ln = int(length[c])
        ok = ln <= L and ln <= 65535
        if not ok:
            refusal[c] = E_INVALID_ARG
        elif ln:
            aa = aatype[c, :ln].astype(np.int64)
            if (aa > 20).any():
                ok = False
            else:
                rc = np.where(aa < 20, aa, UNK)
                sl = T[rc]                                                    # [ln, 14]
                present = (sl >= 0) & np.take_along_axis(mask[c, :ln], np.maximum(sl, 0), 1)
                ok = bool(present[:, :3].all())                               # N, CA, C lead every residue's canonical order
            if not ok:
                refusal[c] = E_RESIDUE
        if not ok or ln == 0:
            res_off.append(res_off[-1])
            continue
        rows = np.repeat(np.arange(ln), 14).reshape(ln, 14)
        at = pos[c][rows[present], sl[present]]                               # row-major: residue by residue, canonical order
        cnt = present.sum(1)
        cd = codes[rc][present]
        if layout == "atom37" and mask[c, ln - 1, 36]:
            at = np.concatenate([at, pos[c, ln - 1, 36][None]])
            cd = np.append(cd, D.OXT_CODE)
            cnt[-1] += 1
        xyz.append(at); acode.append(cd); atom_counts.append(cnt); rcode.append(rc)
        bfac.append(plddt[c, :ln] if plddt is not None else np.zeros(ln, np.float32))
        res_off.append(res_off[-1] + ln)
    xyz = np.concatenate(xyz).astype(np.float32) if xyz else np.zeros((0, 3), np.float32)
    atom_off = np.zeros(res_off[-1] + 1, np.uint32)
    if atom_counts:
        atom_off[1:] = np.cumsum(np.concatenate(atom_counts))
    tb = [t.encode("latin-1") if isinstance(t, str) else bytes(t) for t in (titles if titles is not None else [b""] * n)]
    title_off = np.zeros(n + 1, np.uint32)
    title_off[1:] = np.cumsum([len(t) for t in tb])
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    b = ChainBatch(res_off=np.asarray(res_off, np.uint32), atom_off=atom_off, x=np.ascontiguousarray(xyz[:, 0]),
                   y=np.ascontiguousarray(xyz[:, 1]), z=np.ascontiguousarray(xyz[:, 2]), atom_code=cat(acode, np.uint8),
                   res_code=cat(rcode, np.uint8), bfac_ca=cat(bfac, np.float32),
                   first_res_index=np.ones(n, np.int32) if first_res_index is None else np.asarray(first_res_index, np.int32),
                   first_atom_index=np.ones(n, np.int32) if first_atom_index is None else np.asarray(first_atom_index, np.int32),
                   chain_id=np.full(n, ord("A"), np.uint8) if chain_id is None else np.asarray(chain_id, np.uint8),
                   titles=np.frombuffer(b"".join(tb), np.uint8).copy(), title_off=title_off, anchor_threshold=anchor_threshold)
    return b, refusal


def expected_status(refusal, oracle_status):
    """what fcz_compress_dense_* report: this stage's refusal, else the codec's verdict on the chain"""
    return np.where(refusal != 0, refusal, oracle_status).astype(np.int32)


def all_atoms_have_slots(b: ChainBatch, layout="atom37") -> bool:
    """every atom of the flat batch has a slot of its own in the layout: a known name its residue type owns, no name twice in a
    residue, the OXT only as the chain's last atom"""
    ao, ro = b.atom_off.astype(np.int64), b.res_off.astype(np.int64)
    for c in range(b.n_chains):
        for r in range(ro[c], ro[c + 1]):
            seen = set()
            for a in range(ao[r], ao[r + 1]):
                code, rc = int(b.atom_code[a]), int(b.res_code[r])
                if code == D.OXT_CODE:
                    if a != ao[ro[c + 1]] - 1:
                        return False
                elif D.expected_slot(layout, rc, code) < 0:
                    return False
                if code in seen:
                    return False
                seen.add(code)
    return True


def dense_from_batch(b: ChainBatch, layout, L):
    """flat batch (any atom order) -> dense arrays, every atom placed by its name (D.expected_slot); atoms without a slot are dropped,
    the first atom of a name wins. -> dict(pos, mask uint8, aatype, plddt, length uint32, first_res_index)"""
    n, A = b.n_chains, D.WIDTH[layout]
    tab = np.full((24, 256), -1, np.int64)
    for rc in range(24):
        for code in range(37):
            tab[rc, code] = D.expected_slot(layout, rc, code)
    ro, ao = b.res_off.astype(np.int64), b.atom_off.astype(np.int64)
    lens = np.diff(ro)
    assert lens.max(initial=0) <= L
    per_res = np.diff(ao)
    res_of_atom = np.repeat(np.arange(len(per_res)), per_res)
    chain_of_res = np.repeat(np.arange(n), lens)
    row_of_res = np.arange(len(per_res)) - ro[chain_of_res]
    slot = tab[b.res_code[res_of_atom], b.atom_code]
    ok = np.flatnonzero(slot >= 0)[::-1]                                      # reversed: of two atoms in one slot the first is written last
    pos = np.zeros((n, L, A, 3), np.float32); mask = np.zeros((n, L, A), np.uint8)
    e, l = chain_of_res[res_of_atom[ok]], row_of_res[res_of_atom[ok]]
    pos[e, l, slot[ok]] = np.stack([b.x[ok], b.y[ok], b.z[ok]], 1)
    mask[e, l, slot[ok]] = 1
    aatype = np.full((n, L), 20, np.uint8); plddt = np.zeros((n, L), np.float32)
    aatype[chain_of_res, row_of_res] = np.minimum(b.res_code, 20)
    plddt[chain_of_res, row_of_res] = b.bfac_ca
    return dict(pos=pos, mask=mask, aatype=aatype, plddt=plddt, length=lens.astype(np.uint32),
                first_res_index=b.first_res_index.astype(np.int32))


def poison(d, rng):
    """in place: NaN / infinities / random bits wherever the contract says nothing is read as data -- pos where mask == 0, and
    pos, mask, aatype, plddt in every row l >= length[c]"""
    n, L, A = d["mask"].shape
    pad = np.arange(L)[None, :] >= d["length"].astype(np.int64)[:, None]       # [n, L]
    junk = rng.integers(0, 2 ** 32, size=d["pos"].shape, dtype=np.uint64).astype(np.uint32)
    kind = rng.integers(0, 4, size=d["pos"].shape)
    junk[kind == 0] = 0x7FC00000; junk[kind == 1] = 0x7F800000; junk[kind == 2] = 0xFF800000
    d["mask"][pad] = rng.integers(0, 256, size=(int(pad.sum()), A), dtype=np.uint8)
    d["aatype"][pad] = rng.integers(0, 256, size=int(pad.sum()), dtype=np.uint8)
    pl = d["plddt"].view(np.uint32)
    pl[pad] = np.where(rng.integers(0, 2, size=int(pad.sum())) == 1, 0x7FC00000, 0xFF800000).astype(np.uint32)
    off = (d["mask"] == 0) | pad[:, :, None]
    d["pos"].view(np.uint32)[off] = junk[off]
    return pad


def batches_equal(a: ChainBatch, b: ChainBatch):
    """array by array, floats by bit pattern -> name of the first field that differs, or None"""
    for k in ("res_off", "atom_off", "x", "y", "z", "atom_code", "res_code", "bfac_ca", "first_res_index", "first_atom_index",
              "chain_id", "titles", "title_off"):
        u, v = np.ascontiguousarray(getattr(a, k)), np.ascontiguousarray(getattr(b, k))
        if u.dtype == np.float32:
            u, v = u.view(np.uint32), v.view(np.uint32)
        if u.shape != v.shape or not np.array_equal(u, v):
            return k
    return None
