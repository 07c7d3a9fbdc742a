"""The rigid frames restated in numpy (include/fcz_hip.h, fcz_frames_dev), and the device call into 0xA5-filled arrays.

Per row and group: three defining atoms (a0, a1, a2) = fcz_frame_atom(type, group, 0 .. 2) at the slots fcz_dense_slot gives them
(groups 0 and 3 through residue code 0: N, CA, C, O have the same slot in every type); v1 = a0 - a1 for group 0 and a1 - a0 for the
others, v2 = a2 - a1, origin a1;
    n1 = sqrt((v1x*v1x + v1y*v1y) + v1z*v1z)      e1 = v1 / n1
    d  = (e1x*v2x + e1y*v2y) + e1z*v2z             u  = v2 - e1*d
    n2 = sqrt((ux*ux + uy*uy) + uz*uz)             e2 = u / n2            e3 = e1 x e2
in float32 (numpy rounds every operation and fuses none; its sqrt and / are correctly rounded). The group exists when the row lies
inside its chain, the type and the layout have the three atoms, their masks are set, their nine coordinates are finite and n1, n2
are finite and > 0; otherwise rot = identity, trans = 0, mask = 0. The same code evaluates the definition in float64 when asked."""
import numpy as np

from _analysis import bits, ptr
from _devpath import GUARD, DevGuarded
from foldcomp_amd import _lib

LAYOUTS = {"atom37": 0, "atom14": 1, "backbone4": 2}
WIDTH = {0: 37, 1: 14, 2: 4}
GROUPS = {"backbone": 0, "all": 1}

_TABLES = {}


def slot_table(layout):
    """int [21, 8, 3]: slot of defining atom j of (type, group) in the layout (an integer of LAYOUTS), -1 = none; type 20 = any
    other aatype value: no chi group"""
    if layout not in _TABLES:
        lib = _lib.load()
        t = np.full((21, 8, 3), -1, np.int64)
        for ty in range(21):
            for g in range(8):
                if g >= 4 and ty >= 20:
                    continue
                rc = ty if ty < 20 else 0
                atoms = [lib.fcz_frame_atom(rc, g, j) for j in range(3)]
                if min(atoms) < 0:
                    continue
                slots = [lib.fcz_dense_slot(layout, rc if g >= 4 else 0, a) for a in atoms]
                if min(slots) >= 0:
                    t[ty, g] = slots
        _TABLES[layout] = t
    return _TABLES[layout]


def frames_rows(pos, mask, aatype, live, layout, groups, dtype=np.float32):
    """pos [R, A, 3] float32, mask [R, A], aatype [R] or None, live bool [R] -> rot [R, G, 3, 3], trans [R, G, 3] of `dtype`,
    frame_mask uint8 [R, G], plus the norms n1 [R, G] (0 where the group does not exist)"""
    R = pos.shape[0]
    G = 1 if groups == 0 else 8
    tab = slot_table(layout)
    ty = np.full(R, 20, np.int64) if aatype is None else np.minimum(np.asarray(aatype).astype(np.int64), 20)
    rot = np.zeros((R, G, 3, 3), dtype); rot[..., 0, 0] = rot[..., 1, 1] = rot[..., 2, 2] = 1
    trans = np.zeros((R, G, 3), dtype)
    fm = np.zeros((R, G), np.uint8)
    norm1 = np.zeros((R, G), dtype)
    rows = np.arange(R)
    p32 = np.asarray(pos, np.float32)
    for g in range(G):
        sl = tab[ty, g]                                               # [R, 3]
        have = (sl >= 0).all(axis=1) & np.asarray(live, bool)
        s = np.where(sl >= 0, sl, 0)
        m = have & (mask[rows, s[:, 0]] != 0) & (mask[rows, s[:, 1]] != 0) & (mask[rows, s[:, 2]] != 0)
        a0, a1, a2 = (p32[rows, s[:, j]] for j in range(3))
        with np.errstate(all="ignore"):
            m &= np.isfinite(a0).all(axis=1) & np.isfinite(a1).all(axis=1) & np.isfinite(a2).all(axis=1)
            a0, a1, a2 = a0.astype(dtype), a1.astype(dtype), a2.astype(dtype)
            v1 = a0 - a1 if g == 0 else a1 - a0
            v2 = a2 - a1
            n1 = np.sqrt((v1[:, 0] * v1[:, 0] + v1[:, 1] * v1[:, 1]) + v1[:, 2] * v1[:, 2])
            e1 = v1 / n1[:, None]
            d = (e1[:, 0] * v2[:, 0] + e1[:, 1] * v2[:, 1]) + e1[:, 2] * v2[:, 2]
            u = v2 - e1 * d[:, None]
            n2 = np.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])
            e2 = u / n2[:, None]
            e3 = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                           e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
            m &= np.isfinite(n1) & (n1 > 0) & np.isfinite(n2) & (n2 > 0)
        for x in (n1, e1, e2, e3):
            assert x.dtype == dtype
        r = np.stack([e1, e2, e3], axis=2)                            # columns are the axes
        rot[m, g] = r[m]
        trans[m, g] = a1[m]
        norm1[m, g] = n1[m]
        fm[m, g] = 1
    return rot, trans, fm, norm1


def live_rows(n, L, length):
    live = np.ones((n, L), bool)
    if length is not None:
        live = np.arange(L)[None, :] < np.minimum(np.asarray(length).astype(np.int64), L)[:, None]
    return live


def frames(pos, mask, aatype, length, layout, groups, dtype=np.float32):
    """pos [n, L, A, 3] (length [n] or None) or the packed [R, A, 3] -> (rot, trans, frame_mask) shaped like fcz_frames_dev's outputs:
    [n, L, G, 3, 3], [n, L, G, 3], [n, L, G] (G = 1 or 8 kept as an axis)"""
    lead = pos.shape[:-2]
    A = pos.shape[-2]
    R = int(np.prod(lead))
    live = live_rows(*lead, length).reshape(R) if len(lead) == 2 else np.ones(R, bool)
    rot, trans, fm, _ = frames_rows(pos.reshape(R, A, 3), np.asarray(mask).reshape(R, A).view(np.uint8), None if aatype is None else np.asarray(aatype).reshape(R),
                                    live, layout, groups, dtype)
    G = rot.shape[1]
    return rot.reshape(lead + (G, 3, 3)), trans.reshape(lead + (G, 3)), fm.reshape(lead + (G,))


def same(got, exp, what=""):
    for name, g, e in zip(("rot", "trans", "frame_mask"), got, exp):
        g, e = bits(g), bits(e)
        assert g.shape == e.shape, (what, name, g.shape, e.shape)
        assert np.array_equal(g, e), (what, name, np.argwhere(g != e)[:4])


def out_spec(lead, G):
    """the three outputs of rows shaped `lead` and G groups as a guard's spec"""
    lead = tuple(lead) + (G,)
    return dict(rot=(np.float32, lead + (3, 3)), trans=(np.float32, lead + (3,)), frame_mask=(np.uint8, lead))


def run_dev(codec, pos_t, mask_t, aatype_t, length_t, n, L, layout, groups, guard=GUARD, expect=0):
    """fcz_frames_dev on device tensors -> (rot [n, L, G, 3, 3], trans [n, L, G, 3], frame_mask [n, L, G]) as numpy, guards checked:
    a byte the call leaves unwritten stays 0xA5 and fails the comparison that follows"""
    import torch
    g = DevGuarded(out_spec((n, L), 1 if groups == 0 else 8), guard)
    torch.cuda.synchronize()
    rc = codec.lib.fcz_frames_dev(codec.ctx, pos_t.data_ptr(), mask_t.data_ptr(), ptr(aatype_t), ptr(length_t), n, L, layout, groups, *g.ptrs())
    codec.synchronize()
    assert rc == expect, rc
    return g.all()
