"""The TM-align-style alignment of chain pairs in float64 numpy (include/fcz_hip.h, fcz_tmalign_dev), written independently of the
kernel: the seeds are built as lists, an alignment is a stored array, every rotation comes from _superpose.kabsch (SVD), and the
dynamic programme keeps the whole matrix H -- cell by cell (dp_cells) or a row at a time with np.maximum.accumulate (dp_rows) -- and
traces back through it by comparing values, where the kernel keeps one row and two direction bits per cell. Beside it: chain sets in
both forms, the seeded pairs of the GPU test, the conditions that make a float64 judge with another solver fair, and the device calls
into 0xA5-filled arrays."""
import ctypes
import functools

import numpy as np

import _superpose as SP
import _tmscore as TM
from _analysis import ptr
from _devpath import DevGuarded

F = np.float32
Q = 65536
MAX_WIDTH = 1024
OUTPUTS = (("rot", F, (3, 3)), ("trans", F, (3,)), ("tm", F, ()), ("tm_a", F, ()), ("tm_b", F, ()), ("aligned", np.int32, ()), ("rmsd", F, ()),
           ("sites_a", np.int32, ()), ("sites_b", np.int32, ()), ("seed", np.int32, ()), ("status", np.int32, ()), ("map", np.int32, "wa"), ("dev", F, "wa"))
KEYS = tuple(k for k, _, _ in OUTPUTS)
DEFAULTS = dict(fragments=True, refine=4, dp_rounds=20, gaps=(0.6, 0.0), iterations=20, levels=0)


# ---- the seed schedule ---------------------------------------------------------------------------------------------------------------

def min_overlap(lmin):
    return max(lmin // 2, min(lmin, 5))


def frag_len(lmin):
    return min(lmin, min(max(lmin // 5, 8), 32))


def frag_starts(S, f):
    out, s = [], 0
    while s + f <= S:
        out.append(s)
        s += f
    if out[-1] != S - f:
        out.append(S - f)
    return out


def seed_list(Sa, Sb, fragments=True):
    """-> [(kind, shift, start_a, start_b, pairs)] in the order of the seeds' numbers: kind 0 a gapless shift, 1 the DP iteration
    from the best gapless seed, 2 a pair of fragments"""
    lmin = min(Sa, Sb)
    if lmin == 0:
        return []
    out = []
    for k in range(-Sa + 1, Sb):
        lo, hi = max(0, -k), min(Sa, Sb - k)
        if hi - lo >= min_overlap(lmin):
            out.append((0, k, lo, lo + k, hi - lo))
    out.append((1, 0, 0, 0, 0))
    if fragments:
        f = frag_len(lmin)
        out += [(2, sb - sa, sa, sb, f) for sa in frag_starts(Sa, f) for sb in frag_starts(Sb, f)]
    return out


# ---- the dynamic programme -------------------------------------------------------------------------------------------------------------

def gap_units(g):
    return int(np.rint(g * Q))


def scores(a, b, rot, trans, d0, raw=False):
    """a [Sa, 3], b [Sb, 3] float64 -> q int64 [Sa, Sb] (raw: the unquantised Q / (1 + d2 / d0^2) instead), in the contract's order of operations"""
    p = [((rot[k, 0] * a[:, 0] + rot[k, 1] * a[:, 1]) + rot[k, 2] * a[:, 2]) + trans[k] for k in range(3)]
    with np.errstate(all="ignore"):
        d = [p[k][:, None] - b[None, :, k] for k in range(3)]
        d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        z = Q / (1.0 + d2 / (d0 * d0))
        if raw:
            return z
        return np.where(np.isfinite(d2), np.floor(z), 0.0).astype(np.int64)


def dp_cells(q, G):
    """H [Sa + 1, Sb + 1] by the recurrence, one cell at a time"""
    Sa, Sb = q.shape
    H = np.zeros((Sa + 1, Sb + 1), np.int64)
    for i in range(1, Sa + 1):
        for j in range(1, Sb + 1):
            H[i, j] = max(H[i - 1, j - 1] + q[i - 1, j - 1], H[i - 1, j] - G, H[i, j - 1] - G)
    return H


def dp_rows(q, G):
    """the same H a row at a time: H[i][j] = max_{k <= j}(C_k + G k) - G j with C_j = max(diag, up) and C_0 = 0"""
    Sa, Sb = q.shape
    H = np.zeros((Sa + 1, Sb + 1), np.int64)
    ramp = G * np.arange(Sb + 1, dtype=np.int64)
    for i in range(1, Sa + 1):
        c = np.zeros(Sb + 1, np.int64)
        c[1:] = np.maximum(H[i - 1, :-1] + q[i - 1], H[i - 1, 1:] - G)
        H[i] = np.maximum.accumulate(c + ramp) - ramp
    return H


def traceback(H, q, G, decisions=None):
    """-> aln int64 [Sa]: the site of b of every site of a, -1 = none. decisions (a list) receives, for every cell on the path, the
    lead of the branch taken over the best branch behind it in the order of preference"""
    Sa, Sb = q.shape
    aln = np.full(Sa, -1, np.int64)
    if Sa == 0 or Sb == 0:
        return aln
    col, row = H[:, Sb], H[Sa, :Sb]
    i, j = int(np.argmax(col)), Sb                                             # (argmax: the first maximum)
    if row.size and row.max() > col.max():
        i, j = Sa, int(np.argmax(row))
    while i > 0 and j > 0:
        dg, up, lf = H[i - 1, j - 1] + q[i - 1, j - 1], H[i - 1, j] - G, H[i, j - 1] - G
        if H[i, j] == dg:
            if decisions is not None:
                decisions.append(int(dg - max(up, lf)))
            aln[i - 1] = j - 1
            i, j = i - 1, j - 1
        elif H[i, j] == up:
            if decisions is not None:
                decisions.append(int(up - lf))
            i -= 1
        else:
            j -= 1
    return aln


def dp_align(a, b, rot, trans, d0, G, cells=False, trace=None):
    q = scores(a, b, rot, trans, d0)
    dec = None if trace is None else []
    aln = traceback((dp_cells if cells else dp_rows)(q, G), q, G, dec)
    if trace is not None:
        z = scores(a, b, rot, trans, d0, raw=True)
        with np.errstate(invalid="ignore"):
            near = float(np.nanmin(np.abs(z - np.rint(z)))) if z.size else np.inf
        trace["dps"].append((near, min(dec, default=np.inf)))
    return aln


# ---- fits --------------------------------------------------------------------------------------------------------------------------------

def run_seed(a, b, start, length, iterations, lmin, margins=None, gaps=None):
    """_tmscore.run_seed on P pairs with the TM sum normalised by lmin -> [(round, tm, rot, trans, sel)]. gaps (a list) receives the
    Horn gap of every fit on three or more pairs"""
    P = len(a)
    d0 = SP.d0_of(lmin)
    sel = np.zeros(P, bool)
    sel[start:start + length] = True
    ds, need, rounds = min(max(d0, 4.5), 8.0), min(3, lmin), []
    for rnd in range(iterations + 1):
        rot, trans = SP.kabsch(a[sel], b[sel])
        if gaps is not None and sel.sum() >= 3:
            gaps.append(SP.horn_gap(b.astype(np.float64), a.astype(np.float64), sel))
        dev = np.sqrt((((a @ rot.T + trans) - b) ** 2).sum(axis=1))
        rounds.append((rnd, float((1.0 / (1.0 + (dev / d0) ** 2)).sum() / lmin), rot, trans, sel))
        if rnd == iterations:
            break
        new = TM.select(dev, ds - 1.0 if rnd == 0 else ds + 1.0, need, margins)
        if np.array_equal(new, sel):
            break
        sel = new
    return rounds


def best_round(rounds):
    best = rounds[0]
    for r in rounds[1:]:
        if r[1] > best[1]:
            best = r
    return best


def shared_rounds(entries, tie=1e-9):
    """entries [(tm, selection bytes)] in the order they are made -> whether every entry within `tie` of the largest tm has the
    selection of the FIRST largest (the one a search keeps), and the lead of that tm over the best entry with another selection"""
    top = max(e[0] for e in entries)
    win = next(e[1] for e in entries if e[0] == top)
    return all(e[1] == win for e in entries if e[0] >= top - tie), min((top - e[0] for e in entries if e[1] != win), default=np.inf)


def fit_alignment(a, b, aln, lmin, refine, trace=None):
    """(1): the fit of an alignment -> (tm, rot, trans, the selection of the winning round). trace["ties"] receives shared_rounds of
    the fit's rounds"""
    i = np.flatnonzero(aln >= 0)
    m, g = (None, None) if trace is None else (trace["margins"], trace["gaps"])
    rounds = run_seed(a[i], b[aln[i]], 0, len(i), refine, lmin, m, g)
    if trace is not None:
        trace["ties"].append(shared_rounds([(r[1], np.packbits(r[4]).tobytes()) for r in rounds]))
    _, tm, rot, trans, sel = best_round(rounds)
    return tm, rot, trans, sel


def dp_iterate(a, b, rot, trans, lmin, p, trace=None, cells=False):
    """(3) -> [(tm, rot, trans, aln, sel)], the candidates in the order they are made, sel the selection of the fit's winning round"""
    d0, need, out = SP.d0_of(lmin), min(3, lmin), []
    for g in p["gaps"]:
        prev = None
        for _ in range(p["dp_rounds"]):
            aln = dp_align(a, b, rot, trans, d0, gap_units(g), cells, trace)
            if (aln >= 0).sum() < need or (prev is not None and np.array_equal(aln, prev)):
                break
            tm, rot, trans, sel = fit_alignment(a, b, aln, lmin, p["refine"], trace)
            out.append((tm, rot, trans, aln, sel))
            prev = aln
    return out


def shift_alignment(Sa, Sb, k):
    j = np.arange(Sa) + k
    return np.where((j >= 0) & (j < Sb), j, -1)


def align_sites(a, b, trace=None, **params):
    """a [Sa, 3], b [Sb, 3] float64, the sites of two chains -> dict(rot, trans, tm, tm_a, tm_b, aligned, rmsd, seed, aln int64 [Sa],
    dev float64 [Sa]). trace (a dict) receives margins, gaps, dps [(nearest integer distance, smallest decision)], candidates
    [(seed, tm)], lead, ties [(shared, lead)]: shared_rounds of every fit's rounds and, last, of the final search's (seed, round)s
    together with the winning candidate, and exact_ties: whether every candidate with another alignment that does not trail the winner by
    1e-9 has EXACTLY its tm and a higher seed"""
    p = dict(DEFAULTS, **params)
    Sa, Sb = len(a), len(b)
    lmin = min(Sa, Sb)
    if trace is not None:
        trace.update(margins=[], gaps=[], dps=[], candidates=[], lead=np.inf, ties=[], exact_ties=True)
    out = dict(rot=np.eye(3), trans=np.zeros(3), tm=0.0, tm_a=0.0, tm_b=0.0, aligned=0, rmsd=0.0, seed=0, aln=np.full(Sa, -1, np.int64), dev=np.zeros(Sa))
    if lmin == 0:
        return out
    m, g = (None, None) if trace is None else (trace["margins"], trace["gaps"])
    cands, gapless = [], []                                                    # (tm, seed, rot, trans, aln, sel)
    for s, (kind, k, ia, ib, n) in enumerate(seed_list(Sa, Sb, p["fragments"])):
        if kind == 0:
            aln = shift_alignment(Sa, Sb, k)
            _, tm, rot, trans, _ = run_seed(a[ia:ia + n], b[ib:ib + n], 0, n, 0, lmin, m, g)[0]
            gapless.append((tm, s, rot, trans, aln, np.ones(n, bool)))
            cands.append(gapless[-1])
            continue
        if kind == 1:
            top = gapless[0]
            for c in gapless[1:]:
                if c[0] > top[0]:
                    top = c
            rot, trans = top[2], top[3]
        else:
            rot, trans = SP.kabsch(a[ia:ia + n], b[ib:ib + n])
            if g is not None and n >= 3:
                sel = np.ones(n, bool)
                g.append(SP.horn_gap(b[ib:ib + n], a[ia:ia + n], sel))
        cands += [(tm, s, r, t, aln, sel) for tm, r, t, aln, sel in dp_iterate(a, b, rot, trans, lmin, p, trace)]
    win = cands[0]
    for c in cands[1:]:
        if c[0] > win[0]:
            win = c
    tm_c, seed, rot, trans, aln, sel_c = win
    if trace is not None:
        others = [c for c in cands if not np.array_equal(c[4], aln)]
        trace["candidates"] = [(c[1], c[0]) for c in cands]
        trace["lead"] = min((tm_c - c[0] for c in others if tm_c - c[0] >= 1e-9), default=np.inf)
        trace["exact_ties"] = all(c[0] == tm_c and c[1] > seed for c in others if tm_c - c[0] < 1e-9)
    i = np.flatnonzero(aln >= 0)
    pa, pb = a[i], b[aln[i]]
    best, entries = None, [(tm_c, np.packbits(sel_c).tobytes())]              # (the candidate comes first: the search must beat it strictly)
    for k, (start, length) in enumerate(TM.seed_list(len(i), p["levels"])):
        rounds = run_seed(pa, pb, start, length, p["iterations"], lmin, m, g)
        entries += [(r[1], np.packbits(r[4]).tobytes()) for r in rounds]
        r = best_round(rounds)
        if best is None or r[1] > best[1]:
            best = r
    if trace is not None:
        trace["ties"].append(shared_rounds(entries))
    if best is not None and best[1] > tm_c:
        rot, trans = best[2], best[3]
    d = np.sqrt((((pa @ rot.T + trans) - pb) ** 2).sum(axis=1))
    tm_of = lambda S: float((1.0 / (1.0 + (d / SP.d0_of(S)) ** 2)).sum() / S)
    dev = np.zeros(Sa)
    dev[i] = d
    out.update(rot=rot, trans=trans, tm=tm_of(lmin), tm_a=tm_of(Sa), tm_b=tm_of(Sb), aligned=len(i), rmsd=float(np.sqrt((d ** 2).sum() / len(i))),
               seed=seed, aln=aln, dev=dev)
    return out


# ---- chain sets ----------------------------------------------------------------------------------------------------------------------------

def chain_rows(s, idx, width):
    """set s = dict(pos, mask, length=None, row_off=None), chain idx -> (status, first row or (entry, 0), rows)"""
    packed = s.get("row_off") is not None
    n = len(s["row_off"]) - 1 if packed else s["pos"].shape[0]
    if not 0 <= idx < n:
        return 2, None, 0
    if packed:
        R = s["pos"].shape[0]
        lo, hi = min(int(s["row_off"][idx]), R), min(int(s["row_off"][idx + 1]), R)
        m = max(hi - lo, 0)
    else:
        L = s["pos"].shape[1]
        lo, m = None, L if s.get("length") is None else min(int(s["length"][idx]), L)
    return (1, None, 0) if m > width else (0, lo, m)


def chain_sites(s, idx, width, slot):
    """-> (status, xyz float64 [S, 3] of the sites, their chain-relative rows)"""
    status, lo, m = chain_rows(s, idx, width)
    if status:
        return status, np.zeros((0, 3)), np.zeros(0, np.int64)
    pos, mask = (s["pos"][lo:lo + m], s["mask"][lo:lo + m]) if s.get("row_off") is not None else (s["pos"][idx, :m], s["mask"][idx, :m])
    with np.errstate(invalid="ignore"):
        site = (mask[:, slot] != 0) & np.isfinite(pos[:, slot, :]).all(axis=-1)
    rows = np.flatnonzero(site)
    return 0, pos[rows, slot].astype(np.float64), rows


def empty(m, wa):
    out = {k: np.zeros((m,) + ((wa,) if tail == "wa" else tail), np.float64 if dt == F else dt) for k, dt, tail in OUTPUTS}
    out["rot"][:] = np.eye(3)
    out["map"][:] = -1
    return out


def align_sets(sa, sb, pairs, wa, wb, slot, traces=None, **params):
    """the reference of fcz_tmalign_dev -> dict of float64 / int arrays"""
    out = empty(len(pairs), wa)
    for e, (i, j) in enumerate(pairs):
        st_a, a, ra = chain_sites(sa, int(i), wa, slot)
        st_b, b, rb = chain_sites(sb, int(j), wb, slot)
        out["status"][e] = max(st_a, st_b)
        if out["status"][e]:
            a, b = a[:0], b[:0]
        tr = None if traces is None else {}
        r = align_sites(a, b, tr, **params)
        if traces is not None:
            traces.append(tr)
        for k in ("rot", "trans", "tm", "tm_a", "tm_b", "aligned", "rmsd", "seed"):
            out[k][e] = r[k]
        out["sites_a"][e], out["sites_b"][e] = len(a), len(b)
        on = r["aln"] >= 0
        out["map"][e, ra[on]] = rb[r["aln"][on]]
        out["dev"][e, ra[on]] = r["dev"][on]
    return out


def dp_sets(sa, sb, pairs, wa, wb, slot, rot, trans, gap, cells=False):
    """the reference of fcz_tmalign_dp_dev -> (map int32 [m, wa], aligned int32 [m])"""
    mp, al = np.full((len(pairs), wa), -1, np.int32), np.zeros(len(pairs), np.int32)
    for e, (i, j) in enumerate(pairs):
        st_a, a, ra = chain_sites(sa, int(i), wa, slot)
        st_b, b, rb = chain_sites(sb, int(j), wb, slot)
        if st_a or st_b or not len(a) or not len(b):
            continue
        aln = dp_align(a, b, rot[e].astype(np.float64), trans[e].astype(np.float64), SP.d0_of(min(len(a), len(b))), gap_units(gap), cells)
        on = aln >= 0
        mp[e, ra[on]] = rb[aln[on]]
        al[e] = on.sum()
    return mp, al


def padded_set(chains, A=4, slot=1, L=None, fill=5.0):
    """chains: a list of float [m, 3] -> a padded set with every mask set inside the chains and `length`"""
    L = L or max(max((len(c) for c in chains), default=1), 1)
    pos, mask = np.full((len(chains), L, A, 3), fill, F), np.zeros((len(chains), L, A), np.uint8)
    for e, c in enumerate(chains):
        pos[e, :len(c), slot], mask[e, :len(c)] = c, 1
    return dict(pos=pos, mask=mask, length=np.asarray([len(c) for c in chains], np.uint32), row_off=None)


def packed_set(chains, A=4, slot=1, fill=5.0):
    R = sum(len(c) for c in chains)
    pos, mask = np.full((R, A, 3), fill, F), np.ones((R, A), np.uint8)
    off = np.zeros(len(chains) + 1, np.uint32)
    off[1:] = np.cumsum([len(c) for c in chains])
    for e, c in enumerate(chains):
        pos[off[e]:off[e + 1], slot] = c
    return dict(pos=pos, mask=mask, length=None, row_off=off)


# ---- the seeded pairs of the GPU test ---------------------------------------------------------------------------------------------------

# Generator seed 0 meets every condition that test_tmalign_cpu.py asserts, for every one of the 22 pairs, over 3 071 dynamic programmes
# and their fits: the smallest |dev - cut| of any selection step is 3.65e-5 A (asked: 1e-8); every round within 1e-9 of a fit's best, and
# every (seed, round) of a final search within 1e-9 of its best, shares the winner's selection -- the smallest lead of a best over a
# round with another selection is 4.48e-7 --; the smallest Horn gap of any fit is 1.45e-3 (asked: 1e-3); every DP has either no
# unquantised score within 1e-7 of an integer or no traceback decision won by 2 units or less; the winner leads every candidate with
# another alignment by 1.76e-5 or more (asked: 1e-9), but for the exact ties of chains with one or two sites, which keep the lowest seed.
ALIGN_SEED = 0
ALIGN_LENGTHS = (3, 5, 9, 17, 33, 63, 64, 65, 96, 129)


def related(rng, x, noise=0.4):
    """a copy of chain x with a deletion, an insertion and (from 24 residues on) a hinge, moved rigidly, plus noise"""
    m = len(x)
    y = x.copy()
    if m >= 24:
        at = m - (3 * m) // 8
        y[at:] = (y[at:] - y[at]) @ TM.rotation_about(rng.standard_normal(3), np.pi / 4).T + y[at]
    if m >= 9:
        cut = int(rng.integers(2, m - 4))
        y = np.concatenate([y[:cut], y[cut + min(3, m // 8):]])
        ins = int(rng.integers(1, len(y) - 1))
        y = np.concatenate([y[:ins], y[ins:ins + 1] + rng.standard_normal((min(2, m // 8) or 1, 3)) * 3.0, y[ins:]])
    return y @ SP.random_rotation(rng).T + rng.uniform(-30, 30, 3) + noise * rng.standard_normal(y.shape)


@functools.lru_cache(maxsize=None)
def align_batch(seed=ALIGN_SEED):
    """-> (chains of a, chains of b, pairs int32 [m, 2]): every length against a related chain, three unrelated pairs, and chains of 0, 1
    and 2 rows, the 2-row chains also against 2 and more rows (Lmin = 2). Shared: do not write"""
    rng = np.random.default_rng(seed)
    ca = [SP.walk_chain(rng, m) for m in ALIGN_LENGTHS]
    cb = [related(rng, x) for x in ca]
    few = [rng.uniform(-20, 20, (m, 3)) for m in (0, 1, 2)]
    two = rng.uniform(-20, 20, (2, 3))
    n = len(ca)
    ca, cb = ca + few, cb + [few[2], few[1], few[1], two]
    pairs = [(i, i) for i in range(len(ca))] + [(4, 7), (8, 5), (9, 3), (n, 2), (3, n + 1), (n + 2, n + 2), (n + 2, n + 3), (n + 2, 1), (2, n + 3)]
    ca, cb = [c.astype(F) for c in ca], [c.astype(F) for c in cb]
    return ca, cb, np.asarray(pairs, np.int32)


@functools.lru_cache(maxsize=None)
def align_batch_reference(fragments=True):
    """the reference of align_batch() as padded sets, with a trace per pair, computed once -> (dict, traces). Shared: do not write"""
    ca, cb, pairs = align_batch()
    sa, sb = padded_set(ca), padded_set(cb)
    traces = []
    ref = align_sets(sa, sb, pairs, sa["pos"].shape[1], sb["pos"].shape[1], 1, traces, fragments=fragments)
    for v in ref.values():
        v.setflags(write=False)
    return ref, traces


def fairness(trace):
    """-> (a) the smallest |dev - cut| of any selection step, (b) the smallest Horn gap of any fit, (c) whether every DP has either no
    unquantised score within 1e-7 of an integer or no traceback decision won by 2 units or less, (d) the winner's lead over the best
    candidate with another alignment that trails it by 1e-9 or more (the others: g), (e) whether in every fit, and in the final search taken together with the winning candidate,
    every round within 1e-9 of the best has the winner's selection, (f) the smallest lead of such a best over a round with another
    selection, (g) whether every candidate with another alignment within 1e-9 of the winner ties it exactly from a higher seed"""
    if not trace or "margins" not in trace:
        return np.inf, np.inf, True, np.inf, True, np.inf, True
    dps_ok = all(near >= 1e-7 or dec > 2 for near, dec in trace["dps"])
    return (min(trace["margins"], default=np.inf), min(trace["gaps"], default=np.inf), dps_ok, trace["lead"], all(t[0] for t in trace["ties"]),
            min((t[1] for t in trace["ties"]), default=np.inf), trace["exact_ties"])


# ---- the device calls ----------------------------------------------------------------------------------------------------------------------

def to_device(s):
    import torch
    return {k: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in s.items()}


def c_set(d):
    from foldcomp_amd.structure import CChainSet
    packed = d.get("row_off") is not None
    return CChainSet(d["pos"].data_ptr(), d["mask"].data_ptr(), None if packed else ptr(d.get("length")), ptr(d.get("row_off")) if packed else None,
                     len(d["row_off"]) - 1 if packed else d["pos"].shape[0], d["pos"].shape[0] if packed else d["pos"].shape[1])


def out_spec(m, wa, want=KEYS):
    """the outputs in `want` for m pairs of width wa as a guard's spec"""
    spec = {k: (d, (m,) + ((wa,) if tail == "wa" else tail)) for k, d, tail in OUTPUTS}
    return {k: spec[k] for k in want}


def run_dev(codec, da, db, pairs_t, wa, wb, layout, slot, want=KEYS, expect=0, m=None, **params):
    """fcz_tmalign_dev on device sets (dicts of torch tensors) -> dict of numpy arrays for the outputs in `want`, guards checked"""
    import torch
    from foldcomp_amd.structure import CTmAlignOut, CTmAlignParams
    p = dict(DEFAULTS, **params)
    m = len(pairs_t) if m is None else m
    g = DevGuarded(out_spec(m, wa, want))
    out = CTmAlignOut(*(g.ptr(k) if k in want else None for k in KEYS))
    par = CTmAlignParams(int(p["fragments"]), p["refine"], p["dp_rounds"], len(p["gaps"]), (ctypes.c_double * 4)(*p["gaps"][:4]), p["levels"], p["iterations"])
    sa, sb = c_set(da), c_set(db)
    torch.cuda.synchronize()
    rc = codec.lib.fcz_tmalign_dev(codec.ctx, ctypes.byref(sa), ctypes.byref(sb), ptr(pairs_t), m, wa, wb, layout, slot, ctypes.byref(par), ctypes.byref(out))
    codec.synchronize()
    assert rc == expect, rc
    if expect:
        assert g.untouched()
        return None
    return {k: g.fetch(k) for k in want}


def run_dp_dev(codec, da, db, pairs_t, wa, wb, layout, slot, rot_t, trans_t, gap, expect=0, want_aligned=True):
    """fcz_tmalign_dp_dev -> (map, aligned), guards checked"""
    import torch
    m = len(pairs_t)
    g = DevGuarded(out_spec(m, wa, ("map", "aligned")))
    sa, sb = c_set(da), c_set(db)
    torch.cuda.synchronize()
    rc = codec.lib.fcz_tmalign_dp_dev(codec.ctx, ctypes.byref(sa), ctypes.byref(sb), pairs_t.data_ptr(), m, wa, wb, layout, slot, ptr(rot_t), ptr(trans_t), gap,
                                      g.ptr("map"), g.ptr("aligned") if want_aligned else None)
    codec.synchronize()
    assert rc == expect, rc
    if expect:
        assert g.untouched()
        return None
    return g.all()
