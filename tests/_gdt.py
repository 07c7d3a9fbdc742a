"""The maximised GDT counts by seeded superposition search in float64 numpy (include/fcz_hip.h, fcz_gdt_dev), written independently
of the kernel: the seeds are _tmscore's lists, a selection is a stored boolean array (the kernel stores none), the cuts of a run are a
list, every rotation comes from _superpose.kabsch (SVD), and the best fit per cutoff is kept as it is met, where the kernel keeps a
count and a seed and finds the fit again. Beside it: the padded and the packed form, a trace with the three conditions that make a
float64 judge fair for a search over thresholds, and the device calls into 0xA5-filled arrays."""
import ctypes
import functools

import numpy as np

import _superpose as SP
import _tmscore as TM
from _analysis import ptr
from _devpath import GUARD, DevGuarded

F = np.float32
CUTOFFS = SP.GDT
KEYS = ("gdt_counts", "sites", "rot", "trans", "seed", "run", "selected", "within")
DTYPES = dict(gdt_counts=np.int32, sites=np.int32, rot=np.float32, trans=np.float32, seed=np.int32, run=np.int32, selected=np.int32, within=np.uint8)
RUNS_ALL, RUNS_TM = 63, 1


# ---- the definition ---------------------------------------------------------------------------------------------------------------

def cuts_of(run, S, iterations):
    """the cut of rounds 1 .. iterations of a run, as a list"""
    if run == 0:
        ds = TM.d_search_of(S)
        return [ds - 1.0 if rnd == 1 else ds + 1.0 for rnd in range(1, iterations + 1)]
    return [CUTOFFS[run - 1]] * iterations


def fit(a, b, sel):
    """a (pred), b (true) float64 [S, 3], sel bool [S] -> (rot, trans, dev [S])"""
    rot, trans = SP.kabsch(a[sel], b[sel])
    return rot, trans, np.sqrt((((a @ rot.T + trans) - b) ** 2).sum(axis=1))


def search_chain(t, p, site, iterations=20, levels=0, runs=RUNS_ALL, trace=None):
    """t (true), p (pred) float32 [m, 3], site bool [m], runs a bit mask -> dict for the chain: gdt_counts [5], sites, rot [5, 3, 3],
    trans [5, 3], seed / run / selected [5], within uint8 [m]. trace (a dict) receives margin (the smallest |dev - cut| of any
    selection step), near (the smallest |dev - c_k| over the fits whose g_k >= the maximum - 1), fits (how many were made), sels
    (the five winning selections) and sites"""
    js = np.flatnonzero(site)
    a, b = p[js].astype(np.float64), t[js].astype(np.float64)
    S, need = len(js), min(3, len(js))
    run_list = [r for r in range(6) if runs >> r & 1]
    assert run_list and runs < 64
    best = [None] * 5                                                         # (count, seed, run, rot, trans, sel)
    margins, log_g, log_m = [], [], []

    def visit(seed, run, rot, trans, dev, sel):
        g = [int((dev <= c).sum()) for c in CUTOFFS]
        log_g.append(g)
        log_m.append([float(np.abs(dev - c).min()) for c in CUTOFFS])
        for k in range(5):
            if best[k] is None or g[k] > best[k][0]:                         # met in the order seed, run, round: a tie keeps the first
                best[k] = (g[k], seed, run, rot, trans, sel)

    for seed, (start, length) in enumerate(TM.seed_list(S, levels)):
        sel0 = np.zeros(S, bool)
        sel0[start:start + length] = True
        rot0, trans0, dev0 = fit(a, b, sel0)
        visit(seed, run_list[0], rot0, trans0, dev0, sel0)                    # round 0 of every run
        for run in run_list:
            sel, dev = sel0, dev0
            for cut in cuts_of(run, S, iterations):
                new = TM.select(dev, cut, need, margins)
                if np.array_equal(new, sel):
                    break
                sel = new
                rot, trans, dev = fit(a, b, sel)
                visit(seed, run, rot, trans, dev, sel)
    out = dict(gdt_counts=np.zeros(5, np.int32), sites=S, rot=np.tile(np.eye(3), (5, 1, 1)), trans=np.zeros((5, 3)), seed=np.zeros(5, np.int32),
               run=np.zeros(5, np.int32), selected=np.zeros(5, np.int32), within=np.zeros(len(t), np.uint8))
    sels = [np.zeros(S, bool)] * 5
    if S:
        for k, (count, seed, run, rot, trans, sel) in enumerate(best):
            out["gdt_counts"][k], out["seed"][k], out["run"][k], out["selected"][k] = count, seed, run, sel.sum()
            out["rot"][k], out["trans"][k] = rot, trans
            dev = np.sqrt((((a @ rot.T + trans) - b) ** 2).sum(axis=1))
            out["within"][js[dev <= CUTOFFS[k]]] |= 1 << k
            sels[k] = sel
    if trace is not None:
        near = np.inf
        if log_g:
            g, m = np.asarray(log_g), np.asarray(log_m)
            for k in range(5):
                near = min(near, float(m[g[:, k] >= out["gdt_counts"][k] - 1, k].min()))
        trace.update(margin=min(margins, default=np.inf), near=near, fits=len(log_g), sels=sels, sites=js)
    return out


def _empty(n, rows_shape):
    return dict(gdt_counts=np.zeros((n, 5), np.int32), sites=np.zeros(n, np.int32), rot=np.tile(np.eye(3), (n, 5, 1, 1)), trans=np.zeros((n, 5, 3)),
                seed=np.zeros((n, 5), np.int32), run=np.zeros((n, 5), np.int32), selected=np.zeros((n, 5), np.int32), within=np.zeros(rows_shape, np.uint8))


def gdt_padded(pos_t, mask_t, pos_p, mask_p, length, slot, iterations=20, levels=0, runs=RUNS_ALL, traces=None):
    n, L = pos_t.shape[:2]
    out = _empty(n, (n, L))
    site = SP.site_of(pos_t, mask_t, pos_p, mask_p, slot)
    for e in range(n):
        m = L if length is None else min(int(length[e]), L)
        tr = None if traces is None else {}
        c = search_chain(pos_t[e, :m, slot], pos_p[e, :m, slot], site[e, :m], iterations, levels, runs, tr)
        if traces is not None:
            traces.append(dict(tr, rows=(e, m)))
        for k in KEYS[:-1]:
            out[k][e] = c[k]
        out["within"][e, :m] = c["within"]
    return out


def gdt_packed(pos_t, mask_t, pos_p, mask_p, row_off, slot, iterations=20, levels=0, runs=RUNS_ALL, traces=None):
    R, n = pos_t.shape[0], len(row_off) - 1
    out = _empty(n, (R,))
    site = SP.site_of(pos_t, mask_t, pos_p, mask_p, slot)
    for e in range(n):
        lo, hi = min(int(row_off[e]), R), min(int(row_off[e + 1]), R)
        hi = max(hi, lo)
        tr = None if traces is None else {}
        c = search_chain(pos_t[lo:hi, slot], pos_p[lo:hi, slot], site[lo:hi], iterations, levels, runs, tr)
        if traces is not None:
            traces.append(dict(tr, rows=(lo, hi)))
        for k in KEYS[:-1]:
            out[k][e] = c[k]
        out["within"][lo:hi] = c["within"]
    return out


# ---- the conditions under which a float64 judge is fair ---------------------------------------------------------------------------
# Measured for the chains of _tmscore.tm_batch() up to 257 rows (generator seed _tmscore.TM_SEED = 0), iterations = 20, all runs,
# 58 895 fits: (a) 4.3e-8 A, (b) 7.6e-6 A, (c) 0.165 over the 125 (chain, cutoff) winners, none of fewer than 3 sites
# (tests/test_gdt_cpu.py asserts the conditions and prints the figures).
MARGIN = 1e-8
GAP = 1e-3


def fairness(t, p, trace):
    """-> (a) the smallest |dev - cut| of any selection step, (b) the smallest |dev - c_k| over the fits whose g_k reaches the chain's
    maximum - 1, (c) the Horn gaps [5] of the winning selections (inf with fewer than three sites: such a transform is not compared)"""
    gaps = []
    for sel in trace["sels"]:
        js = trace["sites"][sel]
        site = np.zeros(len(t), bool)
        site[js] = True
        gaps.append(SP.horn_gap(t, p, site) if len(js) >= 3 else np.inf)
    return trace["margin"], trace["near"], np.asarray(gaps)


def fair(pos_t, pos_p, slot, traces):
    """-> (a) [n], (b) [n], (c) [n, 5] for the chains of a batch whose reference was computed with traces"""
    a, b, c = [], [], []
    for tr in traces:
        lo, hi = tr["rows"]
        t, p = (pos_t[lo, :hi, slot], pos_p[lo, :hi, slot]) if pos_t.ndim == 4 else (pos_t[lo:hi, slot], pos_p[lo:hi, slot])
        x, y, z = fairness(t, p, tr)
        a.append(x); b.append(y); c.append(z)
    return np.asarray(a), np.asarray(b), np.asarray(c).reshape(len(traces), 5)


def assert_fair(pos_t, pos_p, slot, traces, what=""):
    """(a), (b) and (c) for every chain and cutoff -> the smallest of each"""
    a, b, c = fair(pos_t, pos_p, slot, traces)
    assert (a >= MARGIN).all() and (b >= MARGIN).all() and (c >= GAP).all(), (what, a.min(initial=np.inf), b.min(initial=np.inf), c.min(initial=np.inf))
    return a.min(initial=np.inf), b.min(initial=np.inf), c.min(initial=np.inf)


@functools.lru_cache(maxsize=None)
def gdt_batch_reference():
    """the reference of _tmscore.tm_batch() without its last, 1027-row chain, all runs, with a trace per chain, computed once ->
    (n, dict, traces). Shared: do not write"""
    lens, _, pos_t, mask, pos_p = TM.tm_batch()
    n = int(np.flatnonzero(lens <= 257)[-1]) + 1
    assert (lens[:n] <= 257).all() and (lens[n:] > 257).all()
    traces = []
    ref = gdt_padded(pos_t[:n], mask[:n], pos_p[:n], None, lens[:n], 1, traces=traces)
    for v in ref.values():
        v.setflags(write=False)
    return n, ref, traces


@functools.lru_cache(maxsize=None)
def gdt_long_reference():
    """the full search (iterations = 20, every level, all runs) of the hinged 1027-row chain of _tmscore.tm_batch(), with its trace,
    computed once -> (index of the chain in the batch, dict with a leading axis of one chain, traces). Shared: do not write"""
    lens, hinged, pos_t, mask, pos_p = TM.tm_batch()
    e = int(np.flatnonzero((lens == 1027) & hinged)[0])
    traces = []
    ref = gdt_padded(pos_t[e:e + 1], mask[e:e + 1], pos_p[e:e + 1], None, lens[e:e + 1], 1, traces=traces)
    for v in ref.values():
        v.setflags(write=False)
    return e, ref, traces


def close(got, ref, what="", compare=None):
    """the device's outputs against the reference: the integers and `within` exact; rot within 2^-22 absolute and trans within 2
    float32 ulps of the reference rounded to float32, for the (chain, cutoff) pairs of compare (bool [n, 5], None: all)"""
    for k in ("gdt_counts", "sites", "seed", "run", "selected", "within"):
        if k in got:
            assert got[k].dtype == DTYPES[k] and got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), (what, k, np.argwhere(got[k] != ref[k])[:4])
    sel = np.ones(ref["seed"].shape, bool) if compare is None else compare
    seen = {}
    if "rot" in got:
        err = np.abs(got["rot"].astype(np.float64) - np.asarray(ref["rot"]))[sel]
        assert got["rot"].dtype == F and not (err > SP.ROT_TOL).any(), (what, "rot", err.max())
        seen["rot"] = float(err.max()) if err.size else 0.0
    if "trans" in got:
        e = np.asarray(ref["trans"], np.float64)[sel]
        g = got["trans"].astype(np.float64)[sel]
        ulp = np.spacing(np.abs(e.astype(F))).astype(np.float64)
        err = np.abs(g - e.astype(F).astype(np.float64))
        assert got["trans"].dtype == F and not (err > 2.0 * ulp).any(), (what, "trans", (err / ulp).max())
        seen["trans"] = float((err / ulp).max()) if err.size else 0.0
    return seen


# ---- the device calls -------------------------------------------------------------------------------------------------------------

def out_shapes(n, rows, packed):
    return dict(gdt_counts=(n, 5), sites=(n,), rot=(n, 5, 3, 3), trans=(n, 5, 3), seed=(n, 5), run=(n, 5), selected=(n, 5),
                within=(rows,) if packed else (n, rows))


def out_spec(n, rows, packed, want=KEYS):
    shapes = out_shapes(n, rows, packed)
    return {k: (DTYPES[k], shapes[k]) for k in want}


def run_dev(codec, pt, mt, pp, mp, bound_t, n, rows, layout, slot, packed, iterations=20, levels=0, runs=RUNS_ALL, want=KEYS, guard=GUARD, expect=0):
    """fcz_gdt_dev (rows = L) or fcz_gdt_packed_dev (rows = R) on device tensors -> dict of numpy arrays for the outputs in `want`
    (the others are passed as NULL), guards checked"""
    import torch
    from foldcomp_amd.structure import CGdtOut
    g = DevGuarded(out_spec(n, rows, packed, want), guard)
    out = CGdtOut(*(g.ptr(k) if k in want else None for k in KEYS))
    fn = codec.lib.fcz_gdt_packed_dev if packed else codec.lib.fcz_gdt_dev
    torch.cuda.synchronize()
    rc = fn(codec.ctx, pt.data_ptr(), mt.data_ptr(), pp.data_ptr(), ptr(mp), ptr(bound_t), n, rows, layout, slot, levels, iterations, runs, ctypes.byref(out))
    codec.synchronize()
    assert rc == expect, rc
    if expect:
        assert g.untouched()
        return None
    return {k: g.fetch(k) for k in want}
