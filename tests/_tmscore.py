"""The maximised TM-score by seeded iterative superposition in float64 numpy (include/fcz_hip.h, fcz_tmscore_dev), written
independently of the kernel: the seed schedule is built as lists, a selection is a stored boolean array (the kernel stores none),
and every rotation comes from _superpose.kabsch (SVD), not from Horn's quaternion matrix and Jacobi sweeps. Beside it: the padded
and the packed form, the seeded inputs of the GPU test (random walks, plain and hinged), the three conditions that make a float64
judge fair for a search with thresholds (trace -> margin, ties, horn gap), and the device calls into 0xA5-filled arrays."""
import ctypes
import functools

import numpy as np

import _superpose as SP
from _analysis import ptr
from _devpath import GUARD, DevGuarded

F = np.float32
KEYS = SP.KEYS + ("seed", "selected")
DTYPES = dict(SP.DTYPES, seed=np.int32, selected=np.int32)
CUT_STEPS = 16384


# ---- the definition ---------------------------------------------------------------------------------------------------------------

def fragment_lengths(S, levels=0):
    out, l = [], S
    while l > 4:
        out.append(l)
        l //= 2
    if S:
        out.append(min(S, 4))
    return out[:levels] if levels else out


def seed_list(S, levels=0):
    """-> [(start, length)] in the order of the seeds' numbers"""
    out = []
    for l in fragment_lengths(S, levels):
        step, starts, s = max(l // 2, 1), [], 0
        while s + l <= S:
            starts.append(s)
            s += step
        if starts[-1] != S - l:
            starts.append(S - l)
        out += [(s, l) for s in starts]
    return out


def d_search_of(S):
    return min(max(SP.d0_of(S), 4.5), 8.0)


def fit(a, b, sel):
    """a (pred), b (true) float64 [S, 3], sel bool [S] -> (rot, trans, dev [S], tm)"""
    rot, trans = SP.kabsch(a[sel], b[sel])
    dev = np.sqrt((((a @ rot.T + trans) - b) ** 2).sum(axis=1))
    return rot, trans, dev, float((1.0 / (1.0 + (dev / SP.d0_of(len(a))) ** 2)).sum() / len(a))


def select(dev, cut, need, margins=None):
    """{j : dev_j < cut}, the cut growing by 0.5 while fewer than `need` sites lie below it (+inf after CUT_STEPS steps)"""
    steps = 0
    while True:
        if margins is not None and np.isfinite(cut):
            margins.append(float(np.abs(dev - cut).min()))
        sel = dev < cut
        if sel.sum() >= need:
            return sel
        if steps == CUT_STEPS:
            cut = np.inf
        else:
            cut, steps = cut + 0.5, steps + 1


def run_seed(a, b, start, length, iterations, margins=None):
    """-> [(round, tm, rot, trans, sel)] for the rounds the seed runs"""
    S = len(a)
    sel = np.zeros(S, bool)
    sel[start:start + length] = True
    ds, need, rounds = d_search_of(S), min(3, S), []
    for rnd in range(iterations + 1):
        rot, trans, dev, tm = fit(a, b, sel)
        rounds.append((rnd, tm, rot, trans, sel))
        if rnd == iterations:
            break
        new = select(dev, ds - 1.0 if rnd == 0 else ds + 1.0, need, margins)
        if np.array_equal(new, sel):
            break
        sel = new
    return rounds


def search_chain(t, p, site, iterations=20, levels=0, trace=None):
    """t (true), p (pred) float32 [m, 3], site bool [m] -> dict of float64 / int values for the chain, dev float64 [m]. trace (a dict)
    receives margin (the smallest |dev - cut| of any selection step), rounds [(seed, round, tm, selection bytes)] and the winner's sel"""
    js = np.flatnonzero(site)
    a, b = p[js].astype(np.float64), t[js].astype(np.float64)
    S = len(js)
    best, margins, log = None, [], []
    for k, (start, length) in enumerate(seed_list(S, levels)):
        for rnd, tm, rot, trans, sel in run_seed(a, b, start, length, iterations, margins):
            if trace is not None:
                log.append((k, rnd, tm, np.packbits(sel).tobytes()))
            if best is None or tm > best[0]:
                best = (tm, k, rot, trans, sel)
    if best is None:
        rot, trans, seed, sel = np.eye(3), np.zeros(3), 0, np.zeros(0, bool)
    else:
        _, seed, rot, trans, sel = best
    dev = np.zeros(len(t))
    dev[js] = np.sqrt((((a @ rot.T + trans) - b) ** 2).sum(axis=1))
    d = dev[js]
    if trace is not None:
        trace.update(margin=min(margins, default=np.inf), rounds=log, sel=sel, sites=js)
    return dict(rot=rot, trans=trans, rmsd=float(np.sqrt((d ** 2).sum() / S)) if S else 0.0, sites=S,
                gdt_counts=np.asarray([(d <= th).sum() for th in SP.GDT], np.int32),
                tm=float((1.0 / (1.0 + (d / SP.d0_of(S)) ** 2)).sum() / S) if S else 0.0, dev=dev, seed=seed, selected=int(sel.sum()))


def _empty(n, rows_shape):
    return dict(SP._empty(n, rows_shape), seed=np.zeros(n, np.int32), selected=np.zeros(n, np.int32))


def tm_padded(pos_t, mask_t, pos_p, mask_p, length, slot, iterations=20, levels=0, traces=None):
    n, L = pos_t.shape[:2]
    out = _empty(n, (n, L))
    site = SP.site_of(pos_t, mask_t, pos_p, mask_p, slot)
    for e in range(n):
        m = L if length is None else min(int(length[e]), L)
        tr = None if traces is None else {}
        c = search_chain(pos_t[e, :m, slot], pos_p[e, :m, slot], site[e, :m], iterations, levels, tr)
        if traces is not None:
            traces.append(dict(tr, rows=(e, m)))
        for k in KEYS:
            if k != "dev":
                out[k][e] = c[k]
        out["dev"][e, :m] = c["dev"]
    return out


def tm_packed(pos_t, mask_t, pos_p, mask_p, row_off, slot, iterations=20, levels=0, traces=None):
    R, n = pos_t.shape[0], len(row_off) - 1
    out = _empty(n, (R,))
    site = SP.site_of(pos_t, mask_t, pos_p, mask_p, slot)
    for e in range(n):
        lo, hi = min(int(row_off[e]), R), min(int(row_off[e + 1]), R)
        hi = max(hi, lo)
        tr = None if traces is None else {}
        c = search_chain(pos_t[lo:hi, slot], pos_p[lo:hi, slot], site[lo:hi], iterations, levels, tr)
        if traces is not None:
            traces.append(dict(tr, rows=(lo, hi)))
        for k in KEYS:
            if k != "dev":
                out[k][e] = c[k]
        out["dev"][lo:hi] = c["dev"]
    return out


# ---- the seeded inputs of the GPU test ----------------------------------------------------------------------------------------------

TM_LENGTHS = (3, 4, 5, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1027)
HINGE_FROM = 8
# Generator seeds 0 .. 4 all meet the three conditions that test_tmscore_cpu.py asserts for the one chosen; the smallest |dev - cut|
# of any selection step is 1.4e-6, 3.2e-6, 1.1e-6, 9.7e-7, 2.3e-6 A for them. TM_SEED = 0 gives, over 15 512 (seed, round) fits: (a) that
# margin, against the 1e-8 A asked; (b) every (seed, round) within 1e-9 of a chain's maximum shares the winner's selection, and the best
# tm on any other selection trails by 2.3e-8 or more; (c) the smallest Horn gap of a winning selection, 0.165, against 1e-3. Seed 0 is
# also the one where 9 of the 10 hinged chains of 63 residues and more gain 0.05 or more over the Kabsch fit (smallest gain 0.047).
TM_SEED = 0
FOUND = dict(margin=1.359e-6, gap=0.16505)


def rotation_about(axis, angle):
    x, y, z = axis / np.linalg.norm(axis)
    c, s = np.cos(angle), np.sin(angle)
    k = np.asarray([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return c * np.eye(3) + s * k + (1 - c) * np.outer([x, y, z], [x, y, z])


def tm_cases(seed=TM_SEED, lengths=TM_LENGTHS, noise=0.5):
    """random-walk chains (_superpose.walk_chain) at every length, each plain and, from HINGE_FROM residues on, with the last 3/8 of
    the prediction rotated by 60 degrees about its first residue; the prediction is a random rigid motion of that plus Gaussian noise
    -> (lens, hinged bool [n], true [n, L, 3] float32, pred [n, L, 3] float32)"""
    rng = np.random.default_rng(seed)
    kinds = [(m, h) for m in lengths for h in ((False, True) if m >= HINGE_FROM else (False,))]
    L = max(m for m, _ in kinds)
    true, pred = np.zeros((len(kinds), L, 3), F), np.zeros((len(kinds), L, 3), F)
    for e, (m, hinged) in enumerate(kinds):
        x = SP.walk_chain(rng, m)
        y = x.copy()
        if hinged:
            at = m - (3 * m) // 8
            y[at:] = (x[at:] - x[at]) @ rotation_about(rng.standard_normal(3), np.pi / 3).T + x[at]
        y = y @ SP.random_rotation(rng).T + rng.uniform(-30, 30, 3) + noise * rng.standard_normal((m, 3))
        true[e, :m], pred[e, :m] = x, y
    return np.asarray([m for m, _ in kinds]), np.asarray([h for _, h in kinds]), true, pred


@functools.lru_cache(maxsize=None)
def tm_batch(A=4, slot=1):
    """the GPU test's seeded batch: chains of 0, 1 and 2 rows in front of tm_cases(), as padded tensors with every mask set ->
    (lens, hinged, pos_true [n, L, A, 3], mask [n, L, A], pos_pred); the other slots hold other finite numbers. Shared: do not write"""
    lens, hinged, true, pred = tm_cases()
    rng = np.random.default_rng(TM_SEED + 100)
    few_t, few_p = np.zeros((3,) + true.shape[1:], F), np.zeros((3,) + true.shape[1:], F)
    few_t[:, :2], few_p[:, :2] = rng.uniform(-20, 20, (3, 2, 3)), rng.uniform(-20, 20, (3, 2, 3))
    lens, hinged = np.concatenate([[0, 1, 2], lens]), np.concatenate([[False] * 3, hinged])
    true, pred = np.concatenate([few_t, true]), np.concatenate([few_p, pred])
    pos_t, pos_p = SP.in_slot(true, A, slot, 7.0), SP.in_slot(pred, A, slot, -3.0)
    out = (lens, hinged, pos_t, np.ones(pos_t.shape[:-1], np.uint8), pos_p)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def tm_batch_reference():
    """the reference of tm_batch() with a trace per chain, computed once -> (dict, traces). Shared: do not write"""
    lens, _, pos_t, mask, pos_p = tm_batch()
    traces = []
    ref = tm_padded(pos_t, mask, pos_p, None, lens, 1, traces=traces)
    for v in ref.values():
        v.setflags(write=False)
    return ref, traces


def fairness(t, p, trace, tie=1e-9):
    """-> (a) the smallest |dev - cut| of any selection step, (b) whether every (seed, round) whose tm lies within `tie` of the
    chain's maximum has the winner's selection, (c) the Horn gap of the winning selection (inf with fewer than three sites: the
    transform of such a selection is not compared), and the lead of the maximum over the best tm with another selection"""
    rounds = trace["rounds"]
    if not rounds:
        return np.inf, True, np.inf, np.inf
    top = max(r[2] for r in rounds)
    win = np.packbits(trace["sel"]).tobytes()
    shared = all(r[3] == win for r in rounds if r[2] >= top - tie)
    lead = min((top - r[2] for r in rounds if r[3] != win), default=np.inf)
    js = trace["sites"][trace["sel"]]
    site = np.zeros(len(t), bool)
    site[js] = True
    gap = SP.horn_gap(t, p, site) if len(js) >= 3 else np.inf
    return trace["margin"], shared, gap, lead


def assert_fair(pos_t, pos_p, slot, traces, what=""):
    """the three conditions for every chain of a batch whose reference was computed with traces (padded: rows = (entry, length);
    packed: rows = (first row, last row + 1)) -> the smallest margin, gap and lead"""
    worst = [np.inf, np.inf, np.inf]
    for tr in traces:
        lo, hi = tr["rows"]
        t, p = (pos_t[lo, :hi, slot], pos_p[lo, :hi, slot]) if pos_t.ndim == 4 else (pos_t[lo:hi, slot], pos_p[lo:hi, slot])
        a, shared, c, lead = fairness(t, p, tr)
        assert a >= 1e-8 and shared and c >= 1e-3, (what, tr["rows"], a, shared, c)
        worst = [min(worst[0], a), min(worst[1], c), min(worst[2], lead)]
    return worst


# ---- the device calls -------------------------------------------------------------------------------------------------------------

def out_shapes(n, rows, packed):
    return dict(SP.out_shapes(n, rows, packed), seed=(n,), selected=(n,))


def out_spec(n, rows, packed, want=KEYS):
    """the outputs in `want` as a guard's spec"""
    shapes = out_shapes(n, rows, packed)
    return {k: (DTYPES[k], shapes[k]) for k in want}


def run_dev(codec, pt, mt, pp, mp, bound_t, n, rows, layout, slot, packed, iterations=20, levels=0, want=KEYS, guard=GUARD, expect=0):
    """fcz_tmscore_dev (rows = L) or fcz_tmscore_packed_dev (rows = R) on device tensors -> dict of numpy arrays for the outputs in
    `want` (the others are passed as NULL), guards checked"""
    import torch
    from foldcomp_amd.structure import CTmScoreOut
    g = DevGuarded(out_spec(n, rows, packed, want), guard)
    out = CTmScoreOut(*(g.ptr(k) if k in want else None for k in KEYS))
    fn = codec.lib.fcz_tmscore_packed_dev if packed else codec.lib.fcz_tmscore_dev
    torch.cuda.synchronize()
    rc = fn(codec.ctx, pt.data_ptr(), mt.data_ptr(), pp.data_ptr(), ptr(mp), ptr(bound_t), n, rows, layout, slot, levels, iterations, ctypes.byref(out))
    codec.synchronize()
    assert rc == expect, rc
    if expect:
        assert g.untouched()
        return None
    return {k: g.fetch(k) for k in want}
