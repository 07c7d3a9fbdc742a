"""DSSP (Kabsch & Sander 1983) restated in numpy the sequential way (include/fcz_hip.h, fcz_hbond_dev / fcz_dssp_labels_dev), and the
device calls into 0xA5-filled arrays.

Per chain, float32 throughout (numpy rounds every operation and fuses none): backbone rows, chain breaks, the amide hydrogen, the
Kabsch-Sander energy of every donor / acceptor pair as a dense matrix, the two best partners of every row by (energy, row); then,
from the ACCEPTOR table alone, the labels: a list of bridges, ladders grown from it, ladders merged over bulges, and the priority
H > E > B > G > I > T > S. Nothing here is shared with the kernel's row-local formulation."""
import numpy as np

from _analysis import bits, chains_of, ptr
from _devpath import GUARD, DevGuarded

F = np.float32
SS = "-HBEGITS"
O_SLOT = {37: 4, 14: 3, 4: 3}
PRO = 14
HB_MIN, HB_BOND, HB_Q = F(-9.9), F(-0.5), F(27.888)


def _d2(a, b):
    with np.errstate(over="ignore", invalid="ignore"):
        dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
        d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == np.float32
    return d2


def _d(a, b):
    with np.errstate(invalid="ignore"):
        return np.sqrt(_d2(a, b))


class Chain:
    """the backbone of one chain: pos [m, A, 3] float32, mask [m, A] -> bb [m], N / CA / C / O [m, 3], brk [m] (a break behind
    row r), and with aatype [m] or None: has_h [m], H [m, 3]"""

    def __init__(self, pos, mask, aatype=None):
        pos = np.asarray(pos, F)
        m, A = pos.shape[:2]
        slots = [0, 1, 2, O_SLOT[A]]
        self.m = m
        with np.errstate(invalid="ignore"):
            self.bb = (np.asarray(mask)[:, slots] != 0).all(axis=1) & np.isfinite(pos[:, slots]).all(axis=(1, 2))
        self.N, self.CA, self.C, self.O = (pos[:, s] for s in slots)
        self.brk = np.ones(m, bool)
        if m > 1:
            with np.errstate(invalid="ignore"):
                self.brk[:-1] = ~(self.bb[:-1] & self.bb[1:]) | (_d(self.C[:-1], self.N[1:]) > F(2.5))
        self.has_h = np.zeros(m, bool)
        self.H = np.zeros((m, 3), F)
        if m > 1:
            d = _d(self.C[:-1], self.O[:-1])
            ok = ~self.brk[:-1] & (d != 0)
            if aatype is not None:
                ok &= np.asarray(aatype)[1:] != PRO
            with np.errstate(all="ignore"):
                h = self.N[1:] + (self.C[:-1] - self.O[:-1]) / d[:, None]
            assert h.dtype == np.float32
            self.has_h[1:] = ok
            self.H[1:][ok] = h[ok]

    def no_break(self, a, b):
        return 0 <= a and b < self.m and a <= b and not self.brk[a:b].any()


def energy_matrix(ch):
    """-> E [m, m] float32, E[i, j] the energy of donor i and acceptor j, +inf where it is not defined or does not count (E >= 0)"""
    m = ch.m
    E = np.full((m, m), np.inf, F)
    if m == 0:
        return E
    rows = np.arange(m)
    for i0 in range(0, m, 256):
        i = rows[i0:i0 + 256]
        N, H, CA = ch.N[i][:, None], ch.H[i][:, None], ch.CA[i][:, None]
        ok = ch.has_h[i][:, None] & ch.bb[None, :] & (rows[None, :] != i[:, None]) & (rows[None, :] != i[:, None] - 1)
        with np.errstate(invalid="ignore"):
            ok &= _d2(ch.CA[None], CA) < F(81.0)
        dON, dCH, dOH, dCN = _d(ch.O[None], N), _d(ch.C[None], H), _d(ch.O[None], H), _d(ch.C[None], N)
        with np.errstate(all="ignore"):
            e = HB_Q * ((((F(1) / dON) + (F(1) / dCH)) - (F(1) / dOH)) - (F(1) / dCN))
            assert e.dtype == np.float32
            e = np.where(e < HB_MIN, HB_MIN, e)
            e = np.where((dON < F(0.5)) | (dCH < F(0.5)) | (dOH < F(0.5)) | (dCN < F(0.5)), HB_MIN, e)
            ok &= e < 0
        E[i0:i0 + 256] = np.where(ok, e, F(np.inf))
    return E


def _best_two(E):
    """rows of E -> index [m, 2] int32 (-1 = none), energy [m, 2]: the two lowest by (energy, column)"""
    m = E.shape[0]
    index, energy = np.full((m, 2), -1, np.int32), np.zeros((m, 2), F)
    if m == 0:
        return index, energy
    order = np.argsort(E, axis=1, kind="stable")[:, :2]
    e = np.take_along_axis(E, order, axis=1)
    have = np.isfinite(e)
    index[:, :order.shape[1]][have] = order[have]
    energy[:, :order.shape[1]][have] = e[have]
    return index, energy


def hbond_chain(pos, mask, aatype=None):
    """-> acc_index, acc_energy, don_index, don_energy, each [m, 2], rows of the chain"""
    E = energy_matrix(Chain(pos, mask, aatype))
    return _best_two(E) + _best_two(np.ascontiguousarray(E.T))


def labels_chain(pos, mask, acc_index, acc_energy):
    """the labels of one chain from its acceptor table (rows of the chain) -> ss uint8 [m], ss_mask bool [m]"""
    ch = Chain(pos, mask)
    m = ch.m
    acc_index, acc_energy = np.asarray(acc_index).reshape(m, 2), np.asarray(acc_energy, F).reshape(m, 2)
    bonds = set()
    for d in range(m):
        for s in range(2):
            if acc_energy[d, s] < HB_BOND and 0 <= int(acc_index[d, s]) < m:
                bonds.add((d, int(acc_index[d, s])))

    def bond(d, a):
        return (d, a) in bonds

    def turn(n, i):
        return bond(i + n, i) and ch.no_break(i, i + n)

    ss = np.zeros(m, np.uint8)
    # H
    for i in range(1, m):
        if turn(4, i - 1) and turn(4, i):
            ss[i:i + 4] = 1
    # bridges: every pair near a bond is tried against the definition
    cand = set()
    for d, a in bonds:
        for x in (d - 1, d, d + 1):
            for y in (a - 1, a, a + 1):
                cand.add((min(x, y), max(x, y)))
    par, anti = set(), set()
    for i, j in sorted(cand):
        if i < 1 or j < i + 3 or j + 1 >= m or not ch.no_break(i - 1, i + 1) or not ch.no_break(j - 1, j + 1):
            continue
        if (bond(i + 1, j) and bond(j, i - 1)) or (bond(j + 1, i) and bond(i, j - 1)):
            par.add((i, j))
        if (bond(i + 1, j - 1) and bond(j + 1, i - 1)) or (bond(j, i) and bond(i, j)):
            anti.add((i, j))
    sheet = np.zeros(m, np.uint8)          # 1 = B, 2 = E
    for bridges, s in ((par, 1), (anti, -1)):
        ladders = []                        # lists of bridges, in the order of i
        for b in sorted(bridges):
            if (b[0] - 1, b[1] - s) in bridges:
                continue
            run = [b]
            while (run[-1][0] + 1, run[-1][1] + s) in bridges:
                run.append((run[-1][0] + 1, run[-1][1] + s))
            ladders.append(run)
        linked = [False] * len(ladders)
        gaps = []
        for x, X in enumerate(ladders):
            for y, Y in enumerate(ladders):
                (ie, je), (ib, jb) = X[-1], Y[0]
                gi, gj = ib - ie, (jb - je) * s
                if not (0 < gi < 6 and 0 < gj < 6 and (gi < 3 or gj < 3)):
                    continue
                if not ch.no_break(ie, ib) or not ch.no_break(min(je, jb), max(je, jb)):
                    continue
                linked[x] = linked[y] = True
                gaps.append((ie, ib))
                gaps.append((min(je, jb), max(je, jb)))
        for x, X in enumerate(ladders):
            v = 2 if len(X) > 1 or linked[x] else 1
            for i, j in X:
                sheet[i], sheet[j] = max(sheet[i], v), max(sheet[j], v)
        for a, b in gaps:
            sheet[a:b + 1] = 2
    ss[(ss == 0) & (sheet == 2)] = 3
    ss[(ss == 0) & (sheet == 1)] = 2
    # G, then I: against the labels that stood before either was written
    for n, code, block in ((3, 4, (1, 2, 3)), (5, 5, (1, 2, 3, 4))):
        before = ss.copy()
        for i in range(1, m):
            if turn(n, i - 1) and turn(n, i) and i + n <= m and not np.isin(before[i:i + n], block).any():
                ss[i:i + n] = code
    # T
    for r in range(m):
        if ss[r] == 0 and any(turn(n, r - k) for n in (3, 4, 5) for k in range(1, n)):
            ss[r] = 6
    # S
    for r in range(2, m - 2):
        if ss[r] == 0 and ch.no_break(r - 2, r + 2):
            u, v = ch.CA[r] - ch.CA[r - 2], ch.CA[r + 2] - ch.CA[r]
            dot = (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]
            nu, nv = np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]), np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
            assert dot.dtype == np.float32 and nu.dtype == np.float32
            if dot < F(0.34202015) * (nu * nv):
                ss[r] = 7
    return ss, ch.bb.copy()


def hbonds(pos, mask, aatype, bound, packed=False):
    """pos [n, L, A, 3] / [R, A, 3], mask, aatype or None, length [n] / None or row_off [n + 1] -> the four tables [.., 2]; the index
    is the row of the entry (padded) or the global row (packed)"""
    lead = pos.shape[:-2]
    out = [np.full(lead + (2,), -1, np.int32), np.zeros(lead + (2,), F), np.full(lead + (2,), -1, np.int32), np.zeros(lead + (2,), F)]
    for sel, base, m in chains_of(pos.shape, bound, packed):
        if m == 0:
            continue
        t = hbond_chain(pos[sel], mask[sel], None if aatype is None else aatype[sel])
        for o, v in zip(out, t):
            o[sel] = np.where(v >= 0, v + base, -1) if v.dtype == np.int32 else v
    return out


def labels(pos, mask, bound, acc_index, acc_energy, packed=False):
    """the same arrays and an acceptor table of the form hbonds() returns -> ss uint8 [n, L] / [R], ss_mask bool"""
    lead = pos.shape[:-2]
    ss, ss_mask = np.zeros(lead, np.uint8), np.zeros(lead, bool)
    for sel, base, m in chains_of(pos.shape, bound, packed):
        if m == 0:
            continue
        ai = acc_index[sel].astype(np.int64) - base
        ss[sel], ss_mask[sel] = labels_chain(pos[sel], mask[sel], ai, acc_energy[sel])
    return ss, ss_mask


def text(ss):
    return "".join(SS[c] for c in ss)


def same_tables(got, exp, what=""):
    for name, g, e in zip(("acc_index", "acc_energy", "don_index", "don_energy"), got, exp):
        assert g.shape == e.shape and g.dtype == e.dtype, (what, name, g.shape, e.shape, g.dtype, e.dtype)
        if g.dtype == np.float32:
            g, e = bits(g), bits(e)
        assert np.array_equal(g, e), (what, name, np.argwhere(g != e)[:4])


def same_labels(got, exp, what=""):
    for name, g, e in zip(("ss", "ss_mask"), got, exp):
        g, e = np.asarray(g).view(np.uint8), np.asarray(e).view(np.uint8)
        assert g.shape == e.shape, (what, name, g.shape, e.shape)
        assert np.array_equal(g, e), (what, name, np.argwhere(g != e)[:4], g[g != e][:4], e[g != e][:4])


def table_spec(lead):
    """the four tables of rows shaped `lead` as a guard's spec"""
    shape = tuple(lead) + (2,)
    return dict(acc_index=(np.int32, shape), acc_energy=(np.float32, shape), don_index=(np.int32, shape), don_energy=(np.float32, shape))


def run_hbond(codec, pos_t, mask_t, aa_t, bound_t, n, rows, layout, packed, guard=GUARD, expect=0):
    """fcz_hbond_dev (rows = L) or fcz_hbond_packed_dev (rows = R) on device tensors -> the four tables as numpy, guards checked"""
    import torch
    g = DevGuarded(table_spec((rows,) if packed else (n, rows)), guard)
    fn = codec.lib.fcz_hbond_packed_dev if packed else codec.lib.fcz_hbond_dev
    torch.cuda.synchronize()
    rc = fn(codec.ctx, pos_t.data_ptr(), mask_t.data_ptr(), ptr(aa_t), ptr(bound_t), n, rows, layout, *g.ptrs())
    codec.synchronize()
    assert rc == expect, rc
    return g.all()


def run_labels(codec, pos_t, mask_t, aa_t, bound_t, n, rows, layout, packed, acc_index_t, acc_energy_t, guard=GUARD, expect=0):
    """fcz_dssp_labels_dev / _packed_dev on device tensors -> (ss, ss_mask) as numpy uint8, guards checked"""
    import torch
    shape = (rows,) if packed else (n, rows)
    g = DevGuarded(dict(ss=(np.uint8, shape), ss_mask=(np.uint8, shape)), guard)
    fn = codec.lib.fcz_dssp_labels_packed_dev if packed else codec.lib.fcz_dssp_labels_dev
    torch.cuda.synchronize()
    rc = fn(codec.ctx, pos_t.data_ptr(), mask_t.data_ptr(), ptr(aa_t), ptr(bound_t), n, rows, layout, acc_index_t.data_ptr(),
            acc_energy_t.data_ptr(), *g.ptrs())
    codec.synchronize()
    assert rc == expect, rc
    return g.all()


def random_label_case(rng, lens):
    """a packed backbone4 batch and a hand-made acceptor table for the label kernel alone -> pos [R, 4, 3], mask [R, 4], row_off,
    acc_index [R, 2] (global rows), acc_energy [R, 2]. The geometry only decides breaks (C-N distances on both sides of 2.5), bends
    (a random CA walk) and missing atoms; the table holds random bonds within +-40 rows with energies on both sides of -0.5, and
    over them planted turns of 3, 4 and 5 and ladders of both kinds with bulges, written in random order so that they overwrite
    one another: every bridge, ladder, bulge and priority combination turns up."""
    R = int(np.sum(lens))
    row_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    pos = np.zeros((R, 4, 3), F)
    step = rng.normal(size=(R, 3))
    step *= 3.8 / np.linalg.norm(step, axis=1)[:, None]
    pos[:, 1] = np.cumsum(step, axis=0) % 50.0                     # CA
    pos[:, 2] = rng.normal(size=(R, 3)) * 20                        # C
    gap = np.where(rng.random(R) < 0.9, 1.33, rng.choice([2.4, 2.49, 2.5, 2.51, 2.6, 5.0], R))
    u = rng.normal(size=(R, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    pos[1:, 0] = pos[:-1, 2] + (u * gap[:, None])[:-1]              # N of the next row
    pos[:, 3] = pos[:, 2] + 1.2                                     # O
    mask = (rng.random((R, 4)) > 0.01).astype(np.uint8)
    acc_index = np.full((R, 2), -1, np.int64)
    acc_energy = np.zeros((R, 2), F)
    for lo, m in zip(row_off[:-1].astype(np.int64), lens):
        if m == 0:
            continue
        ai = np.arange(m)[:, None] + rng.integers(-40, 41, (m, 2))
        ae = rng.choice(np.asarray([-3.0, -1.0, -0.6, -0.5000001, -0.5, -0.4999999, -0.3, -0.01], F), (m, 2))
        ai[rng.random((m, 2)) < 0.3] = -1 - lo                      # (-1 once the chain's first row is added)
        edits = []
        for _ in range(max(1, m // 12)):
            kind = rng.integers(0, 3)
            if kind == 0:                                           # a helix of turns n
                n, a, k = int(rng.integers(3, 6)), int(rng.integers(0, m)), int(rng.integers(1, 12))
                edits += [(r + n, r) for r in range(a, a + k)]
            else:                                                   # ladders of one kind, bulges between them
                s = 1 if kind == 1 else -1
                i, j = int(rng.integers(0, m)), int(rng.integers(0, m))
                for _ in range(int(rng.integers(1, 4))):
                    for _ in range(int(rng.integers(1, 5))):
                        if s == 1:
                            edits += [(i + 1, j), (j, i - 1)] if rng.random() < 0.5 else [(j + 1, i), (i, j - 1)]
                        else:
                            edits += [(i + 1, j - 1), (j + 1, i - 1)] if rng.random() < 0.5 else [(j, i), (i, j)]
                        i, j = i + 1, j + s
                    i, j = i - 1 + int(rng.integers(1, 7)), j - s + s * int(rng.integers(1, 7))
        for k in rng.permutation(len(edits)):
            d, a = edits[k]
            if 0 <= d < m and 0 <= a < m:
                sl = int(rng.integers(0, 2))
                ai[d, sl], ae[d, sl] = a, F(-2.0) if rng.random() < 0.95 else F(-0.4)
        acc_index[lo:lo + m], acc_energy[lo:lo + m] = ai + lo, ae
    return pos, mask, row_off, acc_index.astype(np.int32), acc_energy


def _place(a, b, c, length, angle, torsion):
    """NeRF: the point at `length` from c, at `angle` (degrees) to b - c, at `torsion` about b -> c from a (float64)"""
    bc = (c - b) / np.linalg.norm(c - b)
    n = np.cross(b - a, bc)
    n /= np.linalg.norm(n)
    t, p = np.radians(angle), np.radians(torsion)
    d = np.array([-np.cos(t), np.sin(t) * np.cos(p), np.sin(t) * np.sin(p)])
    return c + length * (d[0] * bc + d[1] * np.cross(n, bc) + d[2] * n)


def ideal_backbone(phi, psi, m):
    """poly-Ala backbone4 tensors of m residues with the given torsions (omega 180), ideal bond lengths and angles"""
    N, CA, C, O = [np.array([0.0, 0.0, 0.0])], [np.array([1.458, 0.0, 0.0])], [], []
    C.append(CA[0] + 1.525 * np.array([np.cos(np.radians(180 - 111.0)), np.sin(np.radians(180 - 111.0)), 0.0]))
    for r in range(m):
        if r:
            N.append(_place(N[r - 1], CA[r - 1], C[r - 1], 1.329, 116.2, psi))
            CA.append(_place(CA[r - 1], C[r - 1], N[r], 1.458, 121.7, 180.0))
            C.append(_place(C[r - 1], N[r], CA[r], 1.525, 111.0, phi))
        O.append(_place(N[r], CA[r], C[r], 1.231, 120.5, psi + 180.0))
    pos = np.stack([np.asarray(x) for x in (N, CA, C, O)], axis=1).astype(F)
    return pos, np.ones((m, 4), np.uint8)
