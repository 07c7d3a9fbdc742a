"""What the tests of the dense-tensor analyses share (knn, frames, lddt, lddt_atoms, superpose, tmscore, tmalign, dssp, sasa,
violations): comparison on bits, the chains of a batch, packing, the hostile row_off, the helix generator, the torch helpers, the
golden records as dense layouts and the inputs of the refusal tests. The guarded outputs are in tests/_devpath.py."""
import numpy as np

import _dense as DN
from _devpath import to_dev
from _window import Decoded

NAN_BITS = np.uint32(0x7FC00123)               # a NaN with a payload: what the generators put under cleared masks
# chain 0 runs backwards (empty), rows 0 .. 39 are left uncovered, chain 4 runs past R = 700 (clamped to the rows that exist)
HOSTILE_ROW_OFF = np.asarray([300, 40, 120, 400, 401, 950], np.uint32)


def bits(a):
    """float32 as uint32, anything else as bytes"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint8)


def ptr(t):
    return None if t is None else t.data_ptr()


def chains_of(shape, bound, packed):
    """-> [(index of the chain's rows, first row, rows of the chain)]"""
    if packed:
        R = shape[0]
        out = []
        for e in range(len(bound) - 1):
            lo, hi = min(int(bound[e]), R), min(int(bound[e + 1]), R)
            if hi > lo:
                out.append((slice(lo, hi), lo, hi - lo))
        return out
    n, L = shape[:2]
    return [((e, slice(0, L if bound is None else min(int(bound[e]), L))), 0, L if bound is None else min(int(bound[e]), L)) for e in range(n)]


def row_off_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)


def pack1(a, lens):
    """padded [n, L, ..] -> packed [sum(lens), ..]"""
    return np.concatenate([a[e, :m] for e, m in enumerate(lens)])


def pack(arrays, lens):
    return [pack1(a, lens) for a in arrays]


def to14(v37, aatype):
    """per-slot values of atom37 [.., 37] or [.., 37, 3] -> atom14 through the slot map of every row's type, 0 where a type has no atom"""
    slot = np.full((21, 14), -1, np.int64)
    for ty in range(21):
        for j, code in enumerate(DN.RES_ATOMS[ty]):
            slot[ty, j] = DN.expected_slot("atom37", ty, code)
    s = slot[np.minimum(aatype, 20)]
    if v37.ndim == s.ndim + 1:
        return np.where(s[..., None] >= 0, np.take_along_axis(v37, np.maximum(s, 0)[..., None], axis=-2), 0).astype(v37.dtype)
    return np.where(s >= 0, np.take_along_axis(v37, np.maximum(s, 0), axis=-1), 0).astype(v37.dtype)


def helix(rng, m, A):
    """m rows of A atoms: an ideal alpha helix (backbone4) with a jitter of 0.05, for A > 4 the other atoms scattered about every CA"""
    from _dssp import ideal_backbone           # (tests/_dssp.py imports this module)
    F = np.float32
    if m == 0:
        return np.zeros((0, A, 3), F)
    bb = ideal_backbone(-57, -47, m)[0] + (rng.standard_normal((m, 4, 3)) * 0.05).astype(F)
    if A == 4:
        return bb
    side = bb[:, 1:2] + (rng.standard_normal((m, A - 4, 3)) * 2.0).astype(F)
    full = np.concatenate([bb, side], axis=1)
    if A == 37:                                                               # O is slot 4 there, slot 3 the CB
        full[:, [3, 4]] = full[:, [4, 3]]
    return full


def decoded_layouts(codec, records, L, want):
    """the records as atom37 / atom14 / backbone4 at L rows -> ({layout: {key: numpy}}, the same on the device)"""
    dec = Decoded(codec, records)
    host = {lay: dec.dense(lay, L, want=want) for lay in DN.LAYOUTS}
    return host, {lay: {k: to_dev(v) for k, v in host[lay].items()} for lay in DN.LAYOUTS}


def refusal_inputs(n, L, A):
    """valid inputs for the calls that must be refused for another reason -> (pos zeros, mask ones, aatype zeros, row_off) on the device"""
    import torch
    pos = torch.zeros((n, L, A, 3), dtype=torch.float32, device="cuda:0")
    mask = torch.ones((n, L, A), dtype=torch.uint8, device="cuda:0")
    aa = torch.zeros((n, L), dtype=torch.uint8, device="cuda:0")
    return pos, mask, aa, to_dev(np.arange(n + 1, dtype=np.uint32) * np.uint32(L))


def teq(a, b):
    """two torch tensors of one shape and dtype hold the same bits"""
    import torch
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return a.shape == b.shape and a.dtype == b.dtype and bool((a == b).all())


def to_numpy(d, keys):
    """the tensors d[k] of a result dict on the host, in the order of `keys`"""
    return tuple(d[k].cpu().numpy() for k in keys)
