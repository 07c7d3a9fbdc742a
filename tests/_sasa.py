"""Shrake-Rupley solvent accessibility restated in numpy atom by atom (include/fcz_hip.h, fcz_sasa_dev), and the device calls into
0xA5-filled arrays.

Per chain, float32 throughout (numpy rounds every operation and fuses none): the atoms of the chain as a flat list, and for every atom
in turn its candidates by the cull d2(c_i, c_j) < (Ri + Rj)^2, its points t_k = c_i + Ri * u_k, and the points no candidate buries.
The area of a row is summed in float64 slot by slot. Nothing here is shared with the kernel's ballot formulation; `f64=True` evaluates
the same geometry in float64 without the cull, for the comparison of the two."""
import numpy as np

from _analysis import bits, chains_of, ptr
from _devpath import GUARD, DevGuarded

F = np.float32
FOUR_PI = float.fromhex("0x1.921fb54442d18p+3")
BONDI = {"C": F(1.70), "N": F(1.55), "O": F(1.52), "S": F(1.80)}
PROBE = F(1.4)


def _d2(a, b):
    with np.errstate(over="ignore", invalid="ignore"):
        dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
        return (dx * dx + dy * dy) + dz * dz


def atoms_of(pos, mask, aatype, table):
    """pos [m, A, 3], mask [m, A], aatype [m] or None, table [21, A] -> (atom bool [m, A], radius float32 [m, A])"""
    m, A = mask.shape
    ty = np.zeros(m, np.int64) if aatype is None else np.minimum(np.asarray(aatype).astype(np.int64), 20)
    radius = np.asarray(table, F)[ty]
    with np.errstate(invalid="ignore"):
        atom = (np.asarray(mask) != 0) & np.isfinite(pos).all(axis=-1) & (radius != 0)
    return atom, radius


def counts_chain(pos, mask, aatype, table, probe, points, f64=False, order=None, decisions=None):
    """one chain -> the exposed points of every slot, int16 [m, A]. order: a permutation of the chain's atoms to meet the candidates in.
    f64: the same geometry in float64 with every other atom a candidate. decisions: a list that receives the bool [P] `buried` of every
    atom, in the order of np.argwhere(atom)."""
    T = np.float64 if f64 else F
    pos = np.asarray(pos, F)
    m, A = mask.shape
    P = len(points)
    atom, radius = atoms_of(pos, mask, aatype, table)
    out = np.zeros((m, A), np.int16)
    idx = np.argwhere(atom)
    N = len(idx)
    if N == 0:
        return out
    c = pos[atom].astype(T)
    R = (radius[atom] + F(probe)).astype(T) if not f64 else radius[atom].astype(T) + T(F(probe))
    u = np.asarray(points, F).astype(T)
    perm = np.arange(N) if order is None else np.asarray(order)
    cp, Rp = c[perm], R[perm]
    for i in range(N):
        Ri = R[i]
        if f64:
            near = perm != i
        else:
            S = Ri + Rp
            near = (_d2(c[i], cp) < S * S) & (perm != i)
        with np.errstate(over="ignore"):
            t = c[i][None, :] + Ri * u
        assert t.dtype == T
        cand = np.flatnonzero(near)
        buried = np.zeros(P, bool)
        if len(cand):
            d2 = _d2(t[:, None, :], cp[cand][None, :, :])
            assert d2.dtype == T
            buried = (d2 < (Rp[cand] * Rp[cand])[None, :]).any(axis=1)
        if decisions is not None:
            decisions.append(buried)
        out[idx[i, 0], idx[i, 1]] = P - int(buried.sum())
    return out


def area_rows(counts, pos, mask, aatype, table, probe, P):
    """counts [m, A] -> (sasa float32 [m], sasa_mask bool [m]): the float64 sum slot by slot, one multiplication, one rounding"""
    atom, radius = atoms_of(np.asarray(pos, F), mask, aatype, table)
    R = radius + F(probe)
    R2 = (R * R).astype(np.float64)
    assert R.dtype == np.float32
    total = np.zeros(len(counts), np.float64)
    for a in range(counts.shape[1]):
        total = total + np.where(atom[:, a], counts[:, a].astype(np.float64) * R2[:, a], 0.0)
    scale = np.float64(FOUR_PI) / np.float64(P)
    return (total * scale).astype(F), atom.any(axis=1)


def sasa_chain(pos, mask, aatype, table, probe, points, **kw):
    """-> (sasa_points int16 [m, A], sasa float32 [m], sasa_mask bool [m]) of one chain"""
    counts = counts_chain(pos, mask, aatype, table, probe, points, **kw)
    return (counts,) + area_rows(counts, pos, mask, aatype, table, probe, len(points))


def sasa(pos, mask, aatype, bound, table, probe, points, packed=False):
    """pos [n, L, A, 3] / [R, A, 3], mask, aatype or None, length [n] / None or row_off [n + 1] -> (sasa_points, sasa, sasa_mask)"""
    lead = pos.shape[:-2]
    out = [np.zeros(lead + (pos.shape[-2],), np.int16), np.zeros(lead, F), np.zeros(lead, bool)]
    for sel, _, m in chains_of(pos.shape, bound, packed):
        if m == 0:
            continue
        got = sasa_chain(pos[sel], mask[sel], None if aatype is None else aatype[sel], table, probe, points)
        for o, v in zip(out, got):
            o[sel] = v
    return out


def same_sasa(got, exp, what=""):
    """counts exact, sasa on bits, the mask as bytes"""
    for name, g, e in zip(("sasa_points", "sasa", "sasa_mask"), got, exp):
        g, e = np.asarray(g), np.asarray(e)
        assert g.shape == e.shape, (what, name, g.shape, e.shape)
        if name == "sasa":
            assert g.dtype == e.dtype == np.float32, (what, g.dtype, e.dtype)
            g, e = bits(g), bits(e)
        elif name == "sasa_mask":
            g, e = g.view(np.uint8), e.view(np.uint8)
        else:
            assert g.dtype == e.dtype == np.int16, (what, g.dtype, e.dtype)
        assert np.array_equal(g, e), (what, name, np.argwhere(g != e)[:4], g[g != e][:4], e[g != e][:4])


def default_table(A):
    """the default radii [21, A], built from the atom names without the library: atom14 per type (row 20: the backbone-only codes),
    atom37 / backbone4 by the slot's name in every row; OXT holds 0"""
    from _dense import ATOM37
    from foldcomp_amd._aa_tables import ATOM_NAMES, RES_ATOMS
    t = np.zeros((21, A), F)
    if A == 14:
        for ty in range(21):
            for j, code in enumerate(RES_ATOMS[ty]):
                if code != 255:
                    t[ty, j] = BONDI[ATOM_NAMES[code][0]]
    elif A == 37:
        t[:, :36] = [BONDI[name[0]] for name in ATOM37[:36]]
    else:
        t[:] = [BONDI[c] for c in "NCCO"]
    return t


def out_spec(lead, A):
    """the three outputs of rows shaped `lead` and width A as a guard's spec"""
    lead = tuple(lead)
    return dict(sasa_points=(np.int16, lead + (A,)), sasa=(np.float32, lead), sasa_mask=(np.uint8, lead))


def run_sasa(codec, pos_t, mask_t, aa_t, bound_t, n, rows, layout, packed, points_t, table=None, probe=PROBE, n_points=None, guard=GUARD, expect=0):
    """fcz_sasa_dev (rows = L) or fcz_sasa_packed_dev (rows = R) on device tensors -> (sasa_points, sasa, sasa_mask) as numpy, guards
    checked; table: float32 [21, A] on the host or None"""
    import torch
    g = DevGuarded(out_spec((rows,) if packed else (n, rows), {0: 37, 1: 14, 2: 4}[layout]), guard)
    fn = codec.lib.fcz_sasa_packed_dev if packed else codec.lib.fcz_sasa_dev
    tab = None if table is None else np.ascontiguousarray(table, F)
    torch.cuda.synchronize()
    rc = fn(codec.ctx, pos_t.data_ptr(), mask_t.data_ptr(), ptr(aa_t), ptr(bound_t), n, rows, layout, None if tab is None else tab.ctypes.data, float(probe),
            points_t.data_ptr(), int(points_t.shape[0]) if n_points is None else n_points, *g.ptrs())
    codec.synchronize()
    assert rc == expect, rc
    return g.all()


def globule(rng, m, A=4, spread=None):
    """m rows of A atoms each, uniformly in a ball that holds them at protein density (about one heavy atom per 20 cubic Angstrom),
    moved to coordinates near 37: float32 [m, A, 3]"""
    N = m * A
    radius = (N * 20.0 * 3 / (4 * np.pi)) ** (1 / 3) if spread is None else spread
    v = rng.normal(size=(N, 3))
    v *= (radius * rng.random(N) ** (1 / 3) / np.linalg.norm(v, axis=1))[:, None]
    return (v + 37.0).astype(F).reshape(m, A, 3)
