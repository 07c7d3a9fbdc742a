"""Structural violations restated in numpy (include/fcz_hip.h, fcz_violations_dev), and the device calls into 0xA5-filled arrays.

Per chain, float32 throughout (numpy rounds every operation and fuses none): the atoms of the chain as a flat list, the dense
atoms x atoms matrices of T = (Ri + Rj) - tolerance and d2, the clash matrix with the peptide-bond and disulfide pairs struck out, and
from it the per-atom, per-row and per-chain outputs; the links row by row as whole-array expressions. Nothing here is shared with the
kernel's lane-per-query sweep."""
import ctypes

import numpy as np

from _analysis import bits as bits_of, chains_of, ptr           # (violations_chain has a local `bits`)
from _dense import ATOM37
from _devpath import GUARD, DevGuarded
from _sasa import atoms_of, default_table  # noqa: F401  (default_table: the radii, re-exported for the tests)

F = np.float32
TOL, FACTOR = F(1.5), F(12.0)
CYS, PRO = 4, 14
N_SLOT, CA_SLOT, C_SLOT = 0, 1, 2
SG_SLOT = {37: ATOM37.index("SG"), 14: 5, 4: -1}
KEYS = ("clash_atom", "clash_count", "clash_depth", "clash_partner", "viol_mask", "link_mask", "link_length", "link_cos", "link_violation",
        "chain_counts")
DTYPES = dict(clash_atom=np.uint8, clash_count=np.int32, clash_depth=np.float32, clash_partner=np.int32, viol_mask=np.uint8, link_mask=np.uint8,
              link_length=np.float32, link_cos=np.float32, link_violation=np.uint8, chain_counts=np.int64)
L0, SL, L0_PRO, SL_PRO = F(1.329), F(0.014), F(1.341), F(0.016)
COS0, S0, COS1, S1 = F(-0.4473), F(0.0311), F(-0.5203), F(0.0353)


def _d2(a, b):
    with np.errstate(over="ignore", invalid="ignore"):
        dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
        d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == np.float32
    return d2


def clash_matrix(pos, mask, aatype, table, tol=TOL):
    """one chain -> (idx [N, 2] the (row, slot) of its atoms, clash bool [N, N], depth float32 [N, N] = T - sqrt(d2))"""
    pos = np.asarray(pos, F)
    A = mask.shape[1]
    atom, radius = atoms_of(pos, mask, aatype, table)
    idx = np.argwhere(atom)
    c, R = pos[atom], radius[atom]
    row, slot = idx[:, 0], idx[:, 1]
    T = (R[:, None] + R[None, :]) - F(tol)
    d2 = _d2(c[:, None, :], c[None, :, :])
    assert T.dtype == np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        clash = (row[:, None] != row[None, :]) & (T > 0) & (d2 < T * T)
        depth = T - np.sqrt(d2)
    is_c, is_n = slot == C_SLOT, slot == N_SLOT
    peptide = is_c[:, None] & is_n[None, :] & (row[None, :] == row[:, None] + 1)
    clash &= ~(peptide | peptide.T)
    if aatype is not None and SG_SLOT[A] >= 0:
        sg = (slot == SG_SLOT[A]) & (np.asarray(aatype)[row] == CYS)
        clash &= ~(sg[:, None] & sg[None, :])
    return idx, clash, depth


def _cos(a, b, c):
    """the cosine of the angle at b between a and c, rows of [m, 3]"""
    u, v = a - b, c - b
    with np.errstate(all="ignore"):
        dot = (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]
        nu = np.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])
        nv = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        out = dot / (nu * nv)
    assert out.dtype == np.float32
    return out


def violations_chain(pos, mask, aatype, table, tol=TOL, factor=FACTOR):
    """one chain of m rows -> dict of the per-row outputs and `counts`, the chain's four integers"""
    pos = np.asarray(pos, F)
    mask = np.asarray(mask)
    m, A = mask.shape
    out = dict(clash_atom=np.zeros((m, A), np.uint8), clash_count=np.zeros(m, np.int32), clash_depth=np.zeros(m, F), clash_partner=np.full(m, -1, np.int32),
               viol_mask=np.zeros(m, bool), link_mask=np.zeros(m, bool), link_length=np.zeros(m, F), link_cos=np.zeros((m, 2), F),
               link_violation=np.zeros(m, np.uint8))
    idx, clash, depth = clash_matrix(pos, mask, aatype, table, tol)
    row = idx[:, 0]
    per_atom = clash.sum(axis=1)
    out["clash_atom"][idx[:, 0], idx[:, 1]] = per_atom > 0
    np.add.at(out["clash_count"], row, per_atom.astype(np.int32))
    out["viol_mask"][row] = True
    for r in np.unique(row[per_atom > 0]):
        mine = clash[row == r]
        d = np.where(mine, depth[row == r], F(-1))
        best = d.max()
        out["clash_depth"][r] = best
        out["clash_partner"][r] = row[(d == best).any(axis=0)].min()
    pairs = int(np.triu(clash, 1).sum())
    assert pairs * 2 == int(per_atom.sum()), "the predicate is symmetric"
    # ---- the links ----
    if m > 1:
        with np.errstate(invalid="ignore"):
            ok = lambda r, s: (mask[r, s] != 0) & np.isfinite(pos[r, s]).all(axis=-1)
            here, there = np.arange(m - 1), np.arange(1, m)
            link = ok(here, CA_SLOT) & ok(here, C_SLOT) & ok(there, N_SLOT) & ok(there, CA_SLOT)
        ca, c, n1, ca1 = pos[:-1, CA_SLOT], pos[:-1, C_SLOT], pos[1:, N_SLOT], pos[1:, CA_SLOT]
        with np.errstate(all="ignore"):
            length = np.sqrt(_d2(c, n1))
            cos0, cos1 = _cos(ca, c, n1), _cos(c, n1, ca1)
            pro = np.zeros(m - 1, bool) if aatype is None else np.asarray(aatype)[1:] == PRO
            l0, sl = np.where(pro, L0_PRO, L0), np.where(pro, SL_PRO, SL)
            bits = ((np.abs(length - l0) > F(factor) * sl).astype(np.uint8) | ((np.abs(cos0 - COS0) > F(factor) * S0).astype(np.uint8) << 1) |
                    ((np.abs(cos1 - COS1) > F(factor) * S1).astype(np.uint8) << 2))
            assert (F(factor) * sl).dtype == np.float32 and (length - l0).dtype == np.float32
        out["link_mask"][:-1] = link
        out["link_length"][:-1] = np.where(link, length, F(0))
        out["link_cos"][:-1] = np.where(link[:, None], np.stack([cos0, cos1], axis=1), F(0))
        out["link_violation"][:-1] = np.where(link, bits, 0)
    lv = out["link_violation"]
    out["counts"] = np.asarray([len(idx), pairs, int((lv & 1).astype(bool).sum()), int((lv & 6).astype(bool).sum())], np.int64)
    return out


def violations(pos, mask, aatype, bound, table, tol=TOL, factor=FACTOR, packed=False):
    """pos [n, L, A, 3] / [R, A, 3], mask, aatype or None, length [n] / None or row_off [n + 1] -> dict of the ten outputs"""
    lead, A = pos.shape[:-2], pos.shape[-2]
    n = len(bound) - 1 if packed else pos.shape[0]
    out = dict(clash_atom=np.zeros(lead + (A,), np.uint8), clash_count=np.zeros(lead, np.int32), clash_depth=np.zeros(lead, F),
               clash_partner=np.full(lead, -1, np.int32), viol_mask=np.zeros(lead, bool), link_mask=np.zeros(lead, bool), link_length=np.zeros(lead, F),
               link_cos=np.zeros(lead + (2,), F), link_violation=np.zeros(lead, np.uint8), chain_counts=np.zeros((n, 4), np.int64))
    chains = chains_of(pos.shape, bound, packed)
    entries = [e for e in range(n) if not packed or min(int(bound[e + 1]), pos.shape[0]) > min(int(bound[e]), pos.shape[0])]
    assert len(entries) == len(chains)
    for e, (sel, _, m) in zip(entries, chains):
        if m == 0:
            continue
        got = violations_chain(pos[sel], mask[sel], None if aatype is None else aatype[sel], table, tol, factor)
        for k in KEYS[:-1]:
            out[k][sel] = got[k]
        out["chain_counts"][e] = got["counts"]
    return out


def same_violations(got, exp, what=""):
    """integers and masks equal, floats on bits"""
    for k in KEYS:
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        assert g.shape == e.shape, (what, k, g.shape, e.shape)
        if DTYPES[k] == np.float32:
            assert g.dtype == e.dtype == np.float32, (what, k, g.dtype, e.dtype)
            g, e = bits_of(g), bits_of(e)
        elif DTYPES[k] == np.uint8:
            g, e = g.view(np.uint8), e.view(np.uint8)
        else:
            assert g.dtype == e.dtype == DTYPES[k], (what, k, g.dtype, e.dtype)
        assert np.array_equal(g, e), (what, k, np.argwhere(g != e)[:4], g[g != e][:4], e[g != e][:4])


def consistent(v, bound=None, packed=False):
    """chain_counts against the per-row outputs of the same dict"""
    lead = v["clash_count"].shape
    n = v["chain_counts"].shape[0]
    chains = chains_of(lead + (1, 3), bound, packed)
    entries = [e for e in range(n) if not packed or min(int(bound[e + 1]), lead[0]) > min(int(bound[e]), lead[0])]
    total = np.zeros((n, 4), np.int64)
    for e, (sel, _, m) in zip(entries, chains):
        lv = v["link_violation"][sel]
        s = int(v["clash_count"][sel].astype(np.int64).sum())
        assert s % 2 == 0
        total[e, 1:] = [s // 2, int((lv & 1).astype(bool).sum()), int((lv & 6).astype(bool).sum())]
    assert np.array_equal(v["chain_counts"][:, 1:], total[:, 1:]), (v["chain_counts"], total)


def out_spec(lead, A, n):
    """the ten outputs for rows shaped `lead` of width A and n chains as a guard's spec"""
    tail = dict(clash_atom=(A,), link_cos=(2,))
    return {k: (DTYPES[k], (n, 4) if k == "chain_counts" else tuple(lead) + tail.get(k, ())) for k in KEYS}


class Outputs:
    """the ten device outputs, 0xA5 everywhere with guard bytes on both sides"""

    def __init__(self, lead, A, n, guard=GUARD):
        self.g = DevGuarded(out_spec(lead, A, n), guard)

    def struct(self, **replace):
        from foldcomp_amd.structure import CViolationsOut
        return CViolationsOut(*(replace[k] if k in replace else self.g.ptr(k) for k in KEYS))

    def fetch(self):
        return {k: self.g.fetch(k) for k in KEYS}

    def untouched(self):
        return self.g.untouched()


def run_violations(codec, pos_t, mask_t, aa_t, bound_t, n, rows, layout, packed, table=None, tol=TOL, factor=FACTOR, guard=GUARD, expect=0):
    """fcz_violations_dev (rows = L) or fcz_violations_packed_dev (rows = R) on device tensors -> dict of the ten outputs as numpy, guards
    checked; table: float32 [21, A] on the host or None"""
    import torch
    o = Outputs((rows,) if packed else (n, rows), {0: 37, 1: 14, 2: 4}[layout], n, guard)
    fn = codec.lib.fcz_violations_packed_dev if packed else codec.lib.fcz_violations_dev
    tab = None if table is None else np.ascontiguousarray(table, F)
    c_out = o.struct()
    torch.cuda.synchronize()
    rc = fn(codec.ctx, pos_t.data_ptr(), mask_t.data_ptr(), ptr(aa_t), ptr(bound_t), n, rows, layout, None if tab is None else tab.ctypes.data, float(tol),
            float(factor), ctypes.byref(c_out))
    codec.synchronize()
    assert rc == expect, rc
    return o.fetch()


def chain_of_text(text, aa3):
    """ATOM records of one chain -> ({37: (pos, mask), 14: (pos, mask)}, aatype); OXT goes to slot 36 of atom37"""
    from _dense import expected_slot
    from foldcomp_amd._aa_tables import ATOM_NAMES
    res, key = [], None
    for line in text.splitlines():
        if line.startswith("ATOM"):
            k = (line[21], line[22:27])
            if k != key:
                res.append((line[17:20], {}))
                key = k
            res[-1][1][line[12:16].strip()] = [float(line[30:38]), float(line[38:46]), float(line[46:54])]
    m = len(res)
    out = {A: (np.zeros((m, A, 3), F), np.zeros((m, A), np.uint8)) for A in (37, 14)}
    aa = np.asarray([aa3.index(name) for name, _ in res], np.uint8)
    for r, (name, atoms) in enumerate(res):
        for a, xyz in atoms.items():
            code = ATOM_NAMES.index(a)
            for layout, A in (("atom37", 37), ("atom14", 14)):
                s = expected_slot(layout, int(aa[r]), code)
                if s >= 0:
                    out[A][0][r, s], out[A][1][r, s] = xyz, 1
    return out, aa
