"""The k-nearest-neighbour graph restated in numpy (include/fcz_hip.h, fcz_knn_dev), and the device calls into 0xA5-filled arrays.

Per chain: a row is a site when it lies inside the chain, its mask at the slot is set and its three coordinates are finite;
d2 = (dx*dx + dy*dy) + dz*dz in float32 (numpy rounds every operation and fuses none), the neighbours of site i are the other
sites ordered by np.lexsort on (j, bits of d2), dist is np.sqrt in float32 (correctly rounded)."""
import numpy as np

from _analysis import bits, ptr
from _devpath import GUARD, DevGuarded


def knn_chain(xyz, site, k):
    """xyz float32 [m, 3], site bool [m] -> index int32 [m, k] (rows of the chain, -1 = none), dist float32 [m, k]"""
    m = len(xyz)
    index = np.full((m, k), -1, np.int32)
    dist = np.zeros((m, k), np.float32)
    js = np.flatnonzero(site)
    S = len(js)
    if S < 2:
        return index, dist
    p = np.ascontiguousarray(xyz[js], np.float32)
    keep = min(k, S - 1)
    for q0 in range(0, S, 256):
        q = p[q0:q0 + 256]
        with np.errstate(over="ignore", invalid="ignore"):
            dx = p[None, :, 0] - q[:, None, 0]
            dy = p[None, :, 1] - q[:, None, 1]
            dz = p[None, :, 2] - q[:, None, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == np.float32
        bits = d2.view(np.uint32)
        order = np.lexsort((np.broadcast_to(js, bits.shape), bits), axis=-1)      # primary: bits of d2, then j
        me = np.arange(q0, q0 + len(q))[:, None]
        order = order[order != me].reshape(len(q), S - 1)[:, :keep]
        rows = js[q0:q0 + len(q)]
        index[rows, :keep] = js[order]
        dist[rows, :keep] = np.sqrt(np.take_along_axis(d2, order, axis=1))
    return index, dist


def _site(pos, mask, slot):
    with np.errstate(invalid="ignore"):
        return (mask[..., slot] != 0) & np.isfinite(pos[..., slot, :]).all(axis=-1)


def knn_padded(pos, mask, length, slot, k):
    """pos [n, L, A, 3], mask [n, L, A], length [n] or None -> index [n, L, k], dist [n, L, k]"""
    n, L = pos.shape[:2]
    index = np.full((n, L, k), -1, np.int32)
    dist = np.zeros((n, L, k), np.float32)
    site = _site(pos, mask, slot)
    for e in range(n):
        m = L if length is None else min(int(length[e]), L)
        index[e, :m], dist[e, :m] = knn_chain(pos[e, :m, slot], site[e, :m], k)
    return index, dist


def knn_packed(pos, mask, row_off, slot, k):
    """pos [R, A, 3], mask [R, A], row_off [n + 1] -> index [R, k] (global rows), dist [R, k]; a chain's range is clamped to R
    and empty when it runs backwards (ranges must not overlap)"""
    R = pos.shape[0]
    index = np.full((R, k), -1, np.int32)
    dist = np.zeros((R, k), np.float32)
    site = _site(pos, mask, slot)
    for e in range(len(row_off) - 1):
        lo, hi = min(int(row_off[e]), R), min(int(row_off[e + 1]), R)
        if hi <= lo:
            continue
        i, d = knn_chain(pos[lo:hi, slot], site[lo:hi], k)
        index[lo:hi] = np.where(i >= 0, i + lo, -1)
        dist[lo:hi] = d
    return index, dist


def same(got, exp, what=""):
    gi, gd = got
    ei, ed = exp
    assert gi.shape == ei.shape and gd.shape == ed.shape, (what, gi.shape, ei.shape)
    assert np.array_equal(gi, ei), (what, "index", np.argwhere(gi != ei)[:4])
    assert np.array_equal(bits(gd), bits(ed)), (what, "dist", np.argwhere(bits(gd) != bits(ed))[:4])


def out_spec(shape):
    """the two outputs [.., k] as a guard's spec"""
    return dict(index=(np.int32, tuple(shape)), dist=(np.float32, tuple(shape)))


def run_dev(codec, pos_t, mask_t, bound_t, n, rows, layout, slot, k, packed, guard=GUARD, expect=0):
    """fcz_knn_dev (rows = L) or fcz_knn_packed_dev (rows = R) on device tensors -> (index, dist) as numpy, guards checked"""
    import torch
    g = DevGuarded(out_spec((rows, k) if packed else (n, rows, k)), guard)
    fn = codec.lib.fcz_knn_packed_dev if packed else codec.lib.fcz_knn_dev
    torch.cuda.synchronize()
    rc = fn(codec.ctx, pos_t.data_ptr(), mask_t.data_ptr(), ptr(bound_t), n, rows, layout, slot, k, *g.ptrs())
    codec.synchronize()
    assert rc == expect, rc
    return g.all()
