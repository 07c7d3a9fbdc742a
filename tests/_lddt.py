"""The per-residue lDDT restated in numpy (include/fcz_hip.h, fcz_lddt_dev), and the device calls into 0xA5-filled arrays.

Per chain: a row is a site when it lies inside the chain, both masks at the slot are set and its six coordinates are finite;
d2 = (dx*dx + dy*dy) + dz*dz in float32 (numpy rounds every operation and fuses none) and d = np.sqrt(d2) in float32 (correctly
rounded) in both tensors; j is a pair of i when j != i and d_true < cutoff in float32; diff = |d_true - d_pred| in float32 scores a
hit per threshold it lies under; score = float32(hits) / float32(4 * pairs), 0 where there is no pair."""
import numpy as np

from _analysis import bits, ptr
from _devpath import GUARD, DevGuarded

THRESHOLDS = (0.5, 1.0, 2.0, 4.0)


def _d(p, q):
    with np.errstate(over="ignore", invalid="ignore"):
        dx = p[None, :, 0] - q[:, None, 0]
        dy = p[None, :, 1] - q[:, None, 1]
        dz = p[None, :, 2] - q[:, None, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == np.float32
        return np.sqrt(d2)


def lddt_chain(t, p, site, cutoff=15.0, thresholds=THRESHOLDS):
    """t, p float32 [m, 3], site bool [m] -> score float32 [m], pairs int32 [m], hits int32 [m]"""
    m = len(t)
    pairs = np.zeros(m, np.int32)
    hits = np.zeros(m, np.int32)
    js = np.flatnonzero(site)
    tt, pp = np.ascontiguousarray(t[js], np.float32), np.ascontiguousarray(p[js], np.float32)
    cutoff = np.float32(cutoff)
    th = [np.float32(v) for v in thresholds]
    for q0 in range(0, len(js), 256):
        dt, dp = _d(tt, tt[q0:q0 + 256]), _d(pp, pp[q0:q0 + 256])
        inc = dt < cutoff
        inc[np.arange(dt.shape[0]), np.arange(q0, q0 + dt.shape[0])] = False
        with np.errstate(invalid="ignore"):
            diff = np.abs(dt - dp)                                       # (inf - inf = NaN only where dt is inf: no pair)
        assert diff.dtype == np.float32
        h = sum(((diff < v) & inc).sum(axis=1) for v in th)
        rows = js[q0:q0 + dt.shape[0]]
        pairs[rows] = inc.sum(axis=1)
        hits[rows] = h
    return score_of(pairs, hits), pairs, hits


def score_of(pairs, hits):
    score = np.zeros(pairs.shape, np.float32)
    nz = pairs > 0
    score[nz] = hits[nz].astype(np.float32) / (4 * pairs[nz]).astype(np.float32)
    assert score.dtype == np.float32
    return score


def _site(pos_t, mask_t, pos_p, mask_p, slot):
    with np.errstate(invalid="ignore"):
        s = (mask_t[..., slot] != 0) & np.isfinite(pos_t[..., slot, :]).all(axis=-1) & np.isfinite(pos_p[..., slot, :]).all(axis=-1)
    return s if mask_p is None else s & (mask_p[..., slot] != 0)


def lddt_padded(pos_t, mask_t, pos_p, mask_p, length, slot, cutoff=15.0, thresholds=THRESHOLDS):
    """pos [n, L, A, 3], mask [n, L, A] (mask_p may be None), length [n] or None -> score, pairs, hits [n, L]"""
    n, L = pos_t.shape[:2]
    out = np.zeros((n, L), np.float32), np.zeros((n, L), np.int32), np.zeros((n, L), np.int32)
    site = _site(pos_t, mask_t, pos_p, mask_p, slot)
    for e in range(n):
        m = L if length is None else min(int(length[e]), L)
        for o, v in zip(out, lddt_chain(pos_t[e, :m, slot], pos_p[e, :m, slot], site[e, :m], cutoff, thresholds)):
            o[e, :m] = v
    return out


def lddt_packed(pos_t, mask_t, pos_p, mask_p, row_off, slot, cutoff=15.0, thresholds=THRESHOLDS):
    """pos [R, A, 3], mask [R, A], row_off [n + 1] -> score, pairs, hits [R]; a chain's range is clamped to R and empty when it
    runs backwards (ranges must not overlap)"""
    R = pos_t.shape[0]
    out = np.zeros(R, np.float32), np.zeros(R, np.int32), np.zeros(R, np.int32)
    site = _site(pos_t, mask_t, pos_p, mask_p, slot)
    for e in range(len(row_off) - 1):
        lo, hi = min(int(row_off[e]), R), min(int(row_off[e + 1]), R)
        if hi <= lo:
            continue
        for o, v in zip(out, lddt_chain(pos_t[lo:hi, slot], pos_p[lo:hi, slot], site[lo:hi], cutoff, thresholds)):
            o[lo:hi] = v
    return out


def chain_mean(pairs, hits):
    """-> float32(float64(sum hits) / float64(4 * sum pairs)), 0 where there is no pair"""
    p, h = int(np.sum(pairs, dtype=np.int64)), int(np.sum(hits, dtype=np.int64))
    return np.float32(np.float64(h) / np.float64(4 * p)) if p else np.float32(0)


def same(got, exp, what=""):
    for name, g, e in zip(("score", "pairs", "hits"), got, exp):
        assert g.shape == e.shape and g.dtype == e.dtype, (what, name, g.shape, e.shape, g.dtype, e.dtype)
        if name == "score":
            g, e = bits(g), bits(e)
        assert np.array_equal(g, e), (what, name, np.argwhere(g != e)[:4])


def thresholds_arg(thresholds):
    """-> (the host float32 [4] array to keep alive, its address or None)"""
    if thresholds is None:
        return None, None
    a = np.asarray(thresholds, np.float32)
    return a, a.ctypes.data


def out_spec(shape):
    """the three per-row outputs as a guard's spec"""
    return dict(score=(np.float32, tuple(shape)), pairs=(np.int32, tuple(shape)), hits=(np.int32, tuple(shape)))


def run_dev(codec, pt, mt, pp, mp, bound_t, n, rows, layout, slot, packed, cutoff=15.0, thresholds=None, guard=GUARD, expect=0):
    """fcz_lddt_dev (rows = L) or fcz_lddt_packed_dev (rows = R) on device tensors -> (score, pairs, hits) as numpy, guards checked"""
    import torch
    g = DevGuarded(out_spec((rows,) if packed else (n, rows)), guard)
    fn = codec.lib.fcz_lddt_packed_dev if packed else codec.lib.fcz_lddt_dev
    keep, th = thresholds_arg(thresholds)
    torch.cuda.synchronize()
    rc = fn(codec.ctx, pt.data_ptr(), mt.data_ptr(), pp.data_ptr(), ptr(mp), ptr(bound_t), n, rows, layout, slot, cutoff, th, *g.ptrs())
    codec.synchronize()
    assert rc == expect, rc
    return g.all()
