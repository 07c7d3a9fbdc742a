"""The violation loss and its gradient restated in numpy (include/fcz_hip.h, fcz_violation_loss_dev and fcz_violation_loss_grad_dev), a
float64 form with autograd, and the device calls into 0xA5-filled arrays.

Per chain, float32 throughout (numpy rounds every operation and fuses none): the dense atoms x atoms matrices of tests/_violations.py
(clash_matrix), the terms of every pair as whole matrices, and a row's sum as np.cumsum along the row, which adds one element after
the other from the left: the ascending (row, slot) order of np.argwhere. The links are whole-array expressions over the chain's rows.
Nothing here is shared with the kernel's lane-per-query sweep, its staging or its link stash.

The float64 form (dense64) evaluates the same formulas in float64 torch on the CPU with autograd, on the float32 predicate's sets: the
clashing pairs, the pairs without a direction, the violated terms and their signs are taken from the float32 restatement, so that no
boundary flips between the two precisions. With it comes the bound on |float32 - float64| derived below."""
import numpy as np

import _violations as V
from _analysis import bits as bits_of, chains_of, ptr
from _devpath import GUARD, DevGuarded
from _sasa import atoms_of

F = np.float32
TOL, FACTOR = V.TOL, V.FACTOR
N_SLOT, CA_SLOT, C_SLOT = V.N_SLOT, V.CA_SLOT, V.C_SLOT
U = 2.0 ** -23                                  # the unit the bounds are written in: two float32 roundings


def _seq_sum(terms):
    """[N, K] float32 -> [N]: from 0, one element after the other (np.cumsum is a plain loop; the 0 in front makes a sum of -0 a +0)"""
    t = np.concatenate([np.zeros(terms.shape[:1] + (1,), F), terms], axis=1)
    out = np.cumsum(t, axis=1, dtype=F)[:, -1]
    assert out.dtype == np.float32
    return out


def _pairs(pos, mask, aatype, table, tol):
    """one chain -> (idx [N, 2], c [N, 3], clash bool [N, N], T, d float32 [N, N])"""
    pos = np.asarray(pos, F)
    idx, clash, depth = V.clash_matrix(pos, mask, aatype, table, tol)
    atom, radius = atoms_of(pos, mask, aatype, table)
    c, R = pos[atom], radius[atom]
    T = (R[:, None] + R[None, :]) - F(tol)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.sqrt(V._d2(c[:, None, :], c[None, :, :]))
    assert T.dtype == d.dtype == np.float32 and len(c) == len(idx)
    return idx, c, clash, T, d


def _links(pos, mask, aatype, factor):
    """one chain of m rows -> dict over its m - 1 links: exist, x [3, m - 1] (length, cos0, cos1), x0 and bound [3, m - 1], value [m - 1, 3]
    and the four atoms"""
    pos, mask = np.asarray(pos, F), np.asarray(mask)
    m = mask.shape[0]
    with np.errstate(invalid="ignore"):
        ok = lambda r, s: (mask[r, s] != 0) & np.isfinite(pos[r, s]).all(axis=-1)
        here, there = np.arange(m - 1), np.arange(1, m)
        exist = ok(here, CA_SLOT) & ok(here, C_SLOT) & ok(there, N_SLOT) & ok(there, CA_SLOT)
    ca, c, n1, ca1 = pos[:-1, CA_SLOT], pos[:-1, C_SLOT], pos[1:, N_SLOT], pos[1:, CA_SLOT]
    pro = np.zeros(m - 1, bool) if aatype is None else np.asarray(aatype)[1:] == V.PRO
    with np.errstate(all="ignore"):
        x = np.stack([np.sqrt(V._d2(c, n1)), V._cos(ca, c, n1), V._cos(c, n1, ca1)])
        x0 = np.stack([np.where(pro, V.L0_PRO, V.L0), np.full(m - 1, V.COS0, F), np.full(m - 1, V.COS1, F)])
        bound = np.stack([F(factor) * np.where(pro, V.SL_PRO, V.SL), np.full(m - 1, F(factor) * V.S0, F), np.full(m - 1, F(factor) * V.S1, F)])
        v = np.abs(x - x0) - bound
        value = np.where(exist & np.isfinite(x) & (v > 0), v, F(0))
    assert x.dtype == x0.dtype == bound.dtype == value.dtype == np.float32
    return dict(exist=exist, x=x, x0=x0, bound=bound, value=value.T.copy(), atoms=(ca, c, n1, ca1))


def loss_chain(pos, mask, aatype, table, tol=TOL, factor=FACTOR):
    """one chain of m rows -> (clash_loss [m, A], link_loss [m, 3], [atoms, links])"""
    mask = np.asarray(mask)
    m, A = mask.shape
    idx, _, clash, T, d = _pairs(pos, mask, aatype, table, tol)
    clash_loss, link_loss = np.zeros((m, A), F), np.zeros((m, 3), F)
    with np.errstate(invalid="ignore", over="ignore"):
        clash_loss[idx[:, 0], idx[:, 1]] = _seq_sum(np.where(clash, T - d, F(0)))
    links = 0
    if m > 1:
        lk = _links(pos, mask, aatype, factor)
        link_loss[:-1] = lk["value"]
        links = int(lk["exist"].sum())
    return clash_loss, link_loss, np.asarray([len(idx), links], np.int64)


def _cos_grad(a, b, c, cosv, k):
    """rows of [m, 3], cosv and k [m] -> the terms of a, b, c: the header's operations, one after the other"""
    u, v = a - b, c - b
    with np.errstate(all="ignore"):
        nu = np.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])[:, None]
        nv = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])[:, None]
        uh, vh = u / nu, v / nv
        ga = (vh - cosv[:, None] * uh) / nu
        gc = (uh - cosv[:, None] * vh) / nv
        out = k[:, None] * ga, k[:, None] * -(ga + gc), k[:, None] * gc
    assert all(t.dtype == np.float32 for t in out)
    return out


def grad_chain(pos, mask, aatype, table, w_clash, w_link, tol=TOL, factor=FACTOR):
    """one chain of m rows, w_clash [m, A], w_link [m, 3] -> grad [m, A, 3]"""
    pos, mask, w_clash, w_link = np.asarray(pos, F), np.asarray(mask), np.asarray(w_clash, F), np.asarray(w_link, F)
    m, A = mask.shape
    idx, c, clash, T, d = _pairs(pos, mask, aatype, table, tol)
    grad = np.zeros((m, A, 3), F)
    w = w_clash[idx[:, 0], idx[:, 1]]
    with np.errstate(all="ignore"):
        use = clash & (d != 0) & ((T - d) != 0)
        ws = w[:, None] + w[None, :]
        for x in range(3):
            q = (c[:, None, x] - c[None, :, x]) / d
            grad[idx[:, 0], idx[:, 1], x] = _seq_sum(np.where(use, ws * -q, F(0)))
    if m > 1:
        lk = _links(pos, mask, aatype, factor)
        ca, cc, n1, ca1 = lk["atoms"]
        with np.errstate(all="ignore"):
            e = lk["x"] - lk["x0"]
            on = lk["value"].T > 0                                            # [3, m - 1]: the terms that contribute
            k = np.where(e > 0, w_link[:-1].T, np.where(e < 0, -w_link[:-1].T, F(0)))
            zero = np.zeros((m - 1, 3), F)
            bond = np.where((on[0] & (lk["x"][0] != 0))[:, None], k[0][:, None] * ((cc - n1) / lk["x"][0][:, None]), zero)
            a0, b0, c0 = (np.where(on[1][:, None], t, zero) for t in _cos_grad(ca, cc, n1, lk["x"][1], k[1]))
            a1, b1, c1 = (np.where(on[2][:, None], t, zero) for t in _cos_grad(cc, n1, ca1, lk["x"][2], k[2]))
        assert bond.dtype == a0.dtype == np.float32
        none = np.zeros((1, 3), F)
        prev = lambda t: np.concatenate([none, t])                            # the term of link r - 1 at row r
        here = lambda t: np.concatenate([t, none])                            # the term of link r at row r
        for slot, terms in ((N_SLOT, (prev(-bond), prev(c0), prev(b1))), (CA_SLOT, (prev(c1), here(a0))), (C_SLOT, (here(bond), here(b0), here(a1)))):
            g = grad[:, slot]
            for t in terms:
                g = g + t
            assert g.dtype == np.float32
            grad[:, slot] = g
    return grad


def _each_chain(shape, bound, packed):
    n = len(bound) - 1 if packed else shape[0]
    chains = chains_of(shape, bound, packed)
    entries = [e for e in range(n) if not packed or min(int(bound[e + 1]), shape[0]) > min(int(bound[e]), shape[0])]
    assert len(entries) == len(chains)
    return n, [(e, sel, m) for e, (sel, _, m) in zip(entries, chains) if m]


def loss(pos, mask, aatype, bound, table, tol=TOL, factor=FACTOR, packed=False):
    """pos [n, L, A, 3] / [R, A, 3], mask, aatype or None, length [n] / None or row_off [n + 1] -> dict(clash_loss, link_loss, counts)"""
    lead, A = pos.shape[:-2], pos.shape[-2]
    n, chains = _each_chain(pos.shape, bound, packed)
    out = dict(clash_loss=np.zeros(lead + (A,), F), link_loss=np.zeros(lead + (3,), F), counts=np.zeros((n, 2), np.int64))
    for e, sel, m in chains:
        out["clash_loss"][sel], out["link_loss"][sel], out["counts"][e] = loss_chain(pos[sel], mask[sel], None if aatype is None else aatype[sel], table, tol, factor)
    return out


def grad(pos, mask, aatype, bound, table, w_clash, w_link, tol=TOL, factor=FACTOR, packed=False):
    """-> grad of pos's shape"""
    out = np.zeros(pos.shape, F)
    for e, sel, m in _each_chain(pos.shape, bound, packed)[1]:
        out[sel] = grad_chain(pos[sel], mask[sel], None if aatype is None else aatype[sel], table, w_clash[sel], w_link[sel], tol, factor)
    return out


def weights(shape, seed):
    """upstream gradients of both signs, none of them 0"""
    rng = np.random.default_rng(seed)
    return ((rng.random(shape) + 0.25) * rng.choice([-1.0, 1.0], size=shape)).astype(F)


def same(got, exp, what=""):
    """dicts or arrays: integers equal, floats on bits"""
    if not isinstance(got, dict):
        got, exp = dict(a=got), dict(a=exp)
    for k in exp:
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        assert g.shape == e.shape and g.dtype == e.dtype, (what, k, g.shape, e.shape, g.dtype, e.dtype)
        gb, eb = bits_of(g), bits_of(e)
        assert np.array_equal(gb, eb), (what, k, int((gb != eb).sum()), np.argwhere(gb != eb)[:4], g[gb != eb][:4], e[gb != eb][:4])


# ---- float64 with autograd, and the bound ---------------------------------------------------------------------------------------------
#
# The bound on |float32 - float64| of one output is  U * sum over its terms of (OPS + K) * magnitude,  U = 2^-23 (two roundings, so
# every count below is doubled once more), K the terms of the output (a sum of K terms in sequence adds at most (K - 1) * 2^-24 times
# the sum of their magnitudes), OPS the roundings on the path from the coordinates to one term, counted on the operands' magnitudes:
#   a distance    dx, dy, dz one rounding each (the coordinates are exact), three squares, two additions without cancellation (all
#                 terms >= 0), a root that halves what came before: (1 + 1 + 2) / 2 + 1 = 3 roundings of relative error: OPS_D = 3.
#   clash value   T = (Ri + Rj) - tol: 2 roundings on |Ri + Rj|; T - d: OPS_D on d, 1 on the result. Magnitude (Ri + Rj) + d: OPS = 6.
#   clash grad    w_i + w_j 1, dx 1, d OPS_D, the division 1, the product 1, on |term|: OPS = 7.
#   bond value    |length - l0| - bound: OPS_D on length, the difference 1, the product factor * sl 1, the last difference 1, on
#                 length + l0 + bound: OPS = 6.   bond grad   dx 1, length OPS_D, division 1, product 1 on |term|: OPS = 6.
#   cos           dot: three products and two additions WITH cancellation, 4 roundings on |u||v|; |u| and |v| OPS_D each, their
#                 product 1, the division 1: 4 + 2 * 3 + 2 = 12 on magnitude 1 (|cos| <= 1). cos value: 2 more differences and the
#                 product factor * s on 1 + |cos0| + bound: OPS = 15.
#   cos grad      uh = u / |u|: 1 + OPS_D + 1 = 5 on 1; cos * uh: 12 + 5 + 1 = 18; vh - cos * uh: 5 + 18 + 1 = 24 on magnitude 2 at
#                 most; / |u|: OPS_D + 1 more; * k: 1. OPS = 29 on 2 |w| / |u| for a, on 2 |w| / |v| for c, on their sum for b (one
#                 more addition: 30).
OPS_CLASH, OPS_CLASH_GRAD, OPS_BOND, OPS_BOND_GRAD, OPS_COS, OPS_COS_GRAD = 6, 7, 6, 6, 15, 30


def dense64(pos, mask, aatype, table, w_clash, w_link, tol=TOL, factor=FACTOR):
    """one chain -> dict(clash_loss [m, A], link_loss [m, 3], grad [m, A, 3]) in float64 and the bounds b_clash_loss, b_link_loss, b_grad
    on the float32 restatement's distance from them. The sets come from the float32 predicate; everything else is float64 torch."""
    import torch
    f8 = torch.float64
    pos32, mask = np.asarray(pos, F), np.asarray(mask)
    m, A = mask.shape
    idx, c32, clash, T32, d32 = _pairs(pos32, mask, aatype, table, tol)
    radius = atoms_of(pos32, mask, aatype, table)[1][idx[:, 0], idx[:, 1]].astype(np.float64)
    P = torch.tensor(np.where(np.isfinite(pos32), pos32, 0).astype(np.float64), requires_grad=True)
    rows, slots = torch.as_tensor(idx[:, 0]), torch.as_tensor(idx[:, 1])
    N = len(idx)
    c = P[rows, slots]
    with np.errstate(invalid="ignore"):
        direction = clash & (d32 != 0) & ((T32 - d32) != 0)                   # the pairs that have a gradient
    pair, moves = torch.as_tensor(clash), torch.as_tensor(direction)
    T = torch.as_tensor((radius[:, None] + radius[None, :]) - float(F(tol)))
    d2 = ((c[:, None, :] - c[None, :, :]) ** 2).sum(-1)
    d = torch.where(moves, torch.sqrt(torch.where(moves, d2, torch.ones_like(d2))), torch.sqrt(d2.detach()))
    per_atom = torch.where(pair, T - d, torch.zeros_like(d)).sum(dim=1)
    wc = torch.as_tensor(np.where(np.isfinite(w_clash), w_clash, 0).astype(np.float64))[rows, slots]
    total = (wc * per_atom).sum()
    K = clash.sum(axis=1)
    out = dict(clash_loss=np.zeros((m, A)), b_clash_loss=np.zeros((m, A)), link_loss=np.zeros((m, 3)), b_link_loss=np.zeros((m, 3)))
    out["clash_loss"][idx[:, 0], idx[:, 1]] = per_atom.detach().numpy()
    mag = np.where(clash, (radius[:, None] + radius[None, :]) + d.detach().numpy(), 0.0).sum(axis=1)
    out["b_clash_loss"][idx[:, 0], idx[:, 1]] = U * (OPS_CLASH + K) * mag
    # the gradient's bound: per component, the sum of |term|
    b_grad, n_terms = np.zeros((m, A, 3)), np.zeros((m, A))
    dn = d.detach().numpy()
    ws = np.abs(wc.numpy()[:, None] + wc.numpy()[None, :])
    cn = c.detach().numpy()
    with np.errstate(all="ignore"):
        for x in range(3):
            t = np.where(direction, ws * np.abs(cn[:, None, x] - cn[None, :, x]) / dn, 0.0)
            b_grad[idx[:, 0], idx[:, 1], x] = OPS_CLASH_GRAD * t.sum(axis=1)
    sum_abs = b_grad / OPS_CLASH_GRAD
    n_terms[idx[:, 0], idx[:, 1]] = direction.sum(axis=1)
    if m > 1:
        lk = _links(pos32, mask, aatype, factor)
        on = lk["value"] > 0                                                  # [m - 1, 3]
        sign = np.sign(lk["x"] - lk["x0"]).T.astype(np.float64)               # the float32 signs
        x0, bound = lk["x0"].T.astype(np.float64), (float(F(factor)) * np.stack([np.where(lk["x0"][0] == V.L0_PRO, V.SL_PRO, V.SL).astype(np.float64),
                                                                               np.full(m - 1, float(V.S0)), np.full(m - 1, float(V.S1))])).T
        wl = np.where(np.isfinite(w_link[:-1]), w_link[:-1], 0).astype(np.float64)
        link = torch.zeros((m, 3), dtype=f8)

        def add_abs(row, slot, v):
            sum_abs[row, slot] += v
            n_terms[row, slot] += 1

        for t, (ia, ib, ic) in enumerate(((None, None, None), ((0, CA_SLOT), (0, C_SLOT), (1, N_SLOT)), ((0, C_SLOT), (1, N_SLOT), (1, CA_SLOT)))):
            r = np.flatnonzero(on[:, t])
            if not len(r):
                continue
            rt = torch.as_tensor(r)
            if t == 0:
                cc, n1 = P[rt, C_SLOT], P[rt + 1, N_SLOT]
                still = torch.as_tensor(lk["x"][0][r] == 0)                   # a bond of length 0: a value, no direction
                l2 = ((cc - n1) ** 2).sum(-1)
                x = torch.where(still, torch.sqrt(l2.detach()), torch.sqrt(torch.where(still, torch.ones_like(l2), l2)))
                xn = x.detach().numpy()
                out["b_link_loss"][r, 0] = U * (OPS_BOND + 1) * (xn + x0[r, 0] + bound[r, 0])
                with np.errstate(all="ignore"):
                    g = np.where(xn[:, None] != 0, np.abs(wl[r, 0])[:, None] * np.abs((cc - n1).detach().numpy()) / xn[:, None], 0.0)
                for i, rr in enumerate(r):
                    for row, slot in ((rr, C_SLOT), (rr + 1, N_SLOT)):
                        b_grad[row, slot] += OPS_BOND_GRAD * g[i]
                        add_abs(row, slot, g[i])
            else:
                a, b, cc = (P[rt + dr, slot] for dr, slot in (ia, ib, ic))
                u, v = a - b, cc - b
                nu, nv = torch.sqrt((u * u).sum(-1)), torch.sqrt((v * v).sum(-1))
                x = (u * v).sum(-1) / (nu * nv)
                out["b_link_loss"][r, t] = U * (OPS_COS + 1) * (1 + abs(x0[r, t]) + bound[r, t])
                ga, gc = 2 * np.abs(wl[r, t]) / nu.detach().numpy(), 2 * np.abs(wl[r, t]) / nv.detach().numpy()
                for i, rr in enumerate(r):
                    for (dr, slot), g in ((ia, ga[i]), (ib, ga[i] + gc[i]), (ic, gc[i])):
                        b_grad[rr + dr, slot] += OPS_COS_GRAD * g
                        add_abs(rr + dr, slot, g)
            v = torch.as_tensor(sign[r, t]) * (x - torch.as_tensor(x0[r, t])) - torch.as_tensor(bound[r, t])
            link = link.index_put((rt, torch.full_like(rt, t)), v)
            total = total + (torch.as_tensor(wl[r, t]) * v).sum()
        out["link_loss"] = link.detach().numpy()
    total.backward()
    out["grad"] = P.grad.numpy() if P.grad is not None else np.zeros((m, A, 3))
    out["b_grad"] = U * (b_grad + n_terms[..., None] * sum_abs)
    return out


# ---- the device calls -------------------------------------------------------------------------------------------------------------------

VALUE_KEYS = ("clash_loss", "link_loss", "counts")


def value_spec(lead, A, n):
    return dict(clash_loss=(np.float32, tuple(lead) + (A,)), link_loss=(np.float32, tuple(lead) + (3,)), counts=(np.int64, (n, 2)))


def _table(table):
    return None if table is None else np.ascontiguousarray(table, F)


def run_value(codec, pos_t, mask_t, aa_t, bound_t, n, rows, layout, packed, table=None, tol=TOL, factor=FACTOR, guard=GUARD, expect=0):
    """fcz_violation_loss_dev (rows = L) or _packed_dev (rows = R) on device tensors -> dict of the three outputs as numpy, guards checked"""
    import torch
    A = {0: 37, 1: 14, 2: 4}[layout]
    o = DevGuarded(value_spec((rows,) if packed else (n, rows), A, n), guard)
    fn = codec.lib.fcz_violation_loss_packed_dev if packed else codec.lib.fcz_violation_loss_dev
    tab = _table(table)
    torch.cuda.synchronize()
    rc = fn(codec.ctx, pos_t.data_ptr(), mask_t.data_ptr(), ptr(aa_t), ptr(bound_t), n, rows, layout, None if tab is None else tab.ctypes.data, float(tol),
            float(factor), *o.ptrs())
    codec.synchronize()
    assert rc == expect, rc
    return {k: o.fetch(k) for k in VALUE_KEYS}


def run_grad(codec, pos_t, mask_t, aa_t, bound_t, n, rows, layout, packed, w_clash_t, w_link_t, table=None, tol=TOL, factor=FACTOR, guard=GUARD, expect=0):
    """fcz_violation_loss_grad_dev or _grad_packed_dev -> grad as numpy, guards checked"""
    import torch
    A = {0: 37, 1: 14, 2: 4}[layout]
    o = DevGuarded(dict(grad=(np.float32, ((rows,) if packed else (n, rows)) + (A, 3))), guard)
    fn = codec.lib.fcz_violation_loss_grad_packed_dev if packed else codec.lib.fcz_violation_loss_grad_dev
    tab = _table(table)
    torch.cuda.synchronize()
    rc = fn(codec.ctx, pos_t.data_ptr(), mask_t.data_ptr(), ptr(aa_t), ptr(bound_t), n, rows, layout, None if tab is None else tab.ctypes.data, float(tol),
            float(factor), w_clash_t.data_ptr(), w_link_t.data_ptr(), o.ptr("grad"))
    codec.synchronize()
    assert rc == expect, rc
    return o.fetch("grad")
