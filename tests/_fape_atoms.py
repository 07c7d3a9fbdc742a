"""The all-atom FAPE over the eight rigid groups and its gradient restated in numpy FLOAT64 (include/fcz_hip.h, fcz_fape_atoms_dev /
fcz_fape_atoms_grad_dev), the bounds the device results are held to, the inputs the CPU and the GPU tests share, and the device calls
into 0xA5-filled arrays.

The restatement is tests/_fape.py's, by import: a chain of m rows is laid out as 8 m frame items followed by A m point slots, the
renaming is applied while the chain is laid out (the truth's slots read through the swap table and its ambiguous groups turned by
rot @ diag(1, -1, -1) where the row is swapped, both exact), and _fape.fape_chain -- which takes separate frame and point masks -- does
the rest: _local32 / _local64, the float32 verdict on whether d is finite, the sums, the gradients and every bound. A frame item's
point count P is now the chain's points and a point's frame count its frames; the sums simply run longer.

The bounds are _fape.py's, derived there from the rounding of the stated operations and never fitted to device output. Their factor
1.001 covers the second-order terms and rests on P * 2^-24 <= 1.3e-4, that is P <= 2181 points (and as many frames) a chain: every
chain of this file stays below that (MAX_ITEMS, asserted by ref()): the longest are backbone4 at 515 rows (2060 points, 1030 frames)
and atom14 at 150 rows (2100 points, 1200 frame items).

Ties. A term whose float64 d lies within its error of the clamp may honestly fall on either side in the gradient and gets _fape.py's
allowance; at most 0.02 of the frame-or-point items of a noisy input may carry one (TIE_SHARE, asserted on the restatement before any
device result is read). Measured on the CPU with _fape.fape_chain on noisy chains of 4 frames x 8 atoms a residue (pred frames turned
0.15 rad and moved 0.5 A): shares of at most 0.009 at 64 residues and 0.015 at 128 over clamps 1, 2, 4, 10 and three seeds, 0.009 at
200 residues and clamp 10. So the noisy inputs are chains of at most 128 residues; longer chains use the integer lattice
(_fape.lattice's recipe widened to eight groups and A slots), which has no tie at clamp = 10.25."""
import numpy as np

import _analysis as AN
import _fape as FP
import _sweep_grids as G
from _analysis import NAN_BITS, ptr
from _devpath import GUARD, DevGuarded
from _lddt_soft import weights

F = np.float32
GROUPS = 8
TIE_SHARE = 0.02
MAX_ITEMS = 2181                                  # P * 2^-24 <= 1.3e-4: what the factor 1.001 of _fape.py's bounds rests on
LATTICE_CLAMP = FP.LATTICE_CLAMP
ORDER = ("rot_t", "trans_t", "fm_t", "pos_t", "mask_t", "aatype", "swapped", "rot_p", "trans_p", "fm_p", "pos_p", "mask_p")   # the C-ABI's order
OUT_KEYS = ("sum", "points", "grad_rot", "grad_trans", "grad_pos")
FRAME_KEYS = ("sum", "points", "grad_rot", "grad_trans", "b_sum", "b_rot", "b_trans", "tie_f", "frame", "clamped", "terms")
POINT_KEYS = ("grad_pos", "b_pos", "tie_p", "point")
REF_KEYS = FRAME_KEYS + POINT_KEYS
ASP, GLU, PHE, TYR = 3, 6, 13, 18
LAYOUT = {37: 0, 14: 1, 4: 2}

_TABLES = {}


def tables(A):
    """(swap table uint8 [21, A], ambiguous bool [21, 8]) of the library: fcz_lddt_default_swaps and fcz_frame_ambiguous (type 20 and
    backbone4 have no ambiguity)"""
    if A not in _TABLES:
        from foldcomp_amd import _lib
        lib = _lib.load()
        t = np.zeros((21, A), np.uint8)
        assert lib.fcz_lddt_default_swaps(LAYOUT[A], t.ctypes.data) == 0
        alt = np.zeros((21, GROUPS), bool)
        if A != 4:
            for ty in range(20):
                for g in range(GROUPS):
                    alt[ty, g] = lib.fcz_frame_ambiguous(ty, g) != 0
        _TABLES[A] = (t, alt)
    return _TABLES[A]


def _empty(m, A):
    z = lambda *s: np.zeros((m,) + s)
    out = {k: z(GROUPS) for k in ("sum", "b_sum", "b_rot", "b_trans", "tie_f", "clamped", "terms")}
    out.update(points=np.zeros((m, GROUPS), np.int32), grad_rot=z(GROUPS, 3, 3), grad_trans=z(GROUPS, 3), frame=np.zeros((m, GROUPS), bool),
               grad_pos=z(A, 3), b_pos=z(A), tie_p=z(A), point=np.zeros((m, A), bool))
    return out


def renamed(c, table, alt):
    """one chain (or any rows) of ORDER's arrays -> (rot_t with the ambiguous groups of swapped rows turned, pos_t and mask_t read
    through the swap table at swapped rows): what the sweep reads as the truth"""
    m, A = c["mask_t"].shape
    ty = np.full(m, 20, np.int64) if c.get("aatype") is None else np.minimum(c["aatype"].astype(np.int64), 20)
    sw = np.zeros(m, bool) if c.get("swapped") is None or c.get("aatype") is None else c["swapped"] != 0
    rot_t = c["rot_t"].copy()
    turn = sw[:, None] & alt[ty]
    rot_t[turn, :, 1:] = -rot_t[turn, :, 1:]                              # rot @ diag(1, -1, -1): the sign flips are exact
    s = np.where(sw[:, None], table[ty].astype(np.int64), np.arange(A)[None, :])
    rows = np.arange(m)[:, None]
    return rot_t, c["pos_t"][rows, s], c["mask_t"][rows, s]


def items(c, table=None, alt=None):
    """one chain of ORDER's arrays -> (rot_t, pos_t, mask_t as the sweep reads them, frame bool [m, 8], point bool [m, A]): which item is a
    FRAME and which slot a POINT, float32 facts of the inputs alone"""
    m, A = c["mask_t"].shape
    if table is None:
        table, alt = tables(A)
    rot_t, pos_t, mask_t = renamed(c, table, alt)
    frame = c["fm_t"] != 0
    if c.get("fm_p") is not None:
        frame &= c["fm_p"] != 0
    with np.errstate(all="ignore"):
        for r in (c["rot_t"], c["rot_p"]):
            frame &= np.isfinite(r).all(axis=(-1, -2))
        for t in (c["trans_t"], c["trans_p"]):
            frame &= np.isfinite(t).all(axis=-1)
        point = (mask_t != 0) & np.isfinite(pos_t).all(axis=-1) & np.isfinite(c["pos_p"]).all(axis=-1)
    if c.get("mask_p") is not None:
        point &= c["mask_p"] != 0
    if A == 4:
        frame[:, [1, 2, 4, 5, 6, 7]] = False                              # backbone4 holds the atoms of groups 0 and 3 alone
    return rot_t, pos_t, mask_t, frame, point


def chain(c, w=None, clamp=10.0, eps=1e-4, table=None, alt=None):
    """c: the twelve arrays of one chain of m rows (fm_p, mask_p, aatype, swapped may be None), w [m, 8] or None -> REF_KEYS"""
    m, A = c["mask_t"].shape
    out = _empty(m, A)
    if m == 0:
        return out
    rot_t, pos_t, mask_t, frame, point = items(c, table, alt)
    nf, npt = GROUPS * m, A * m
    assert int(frame.sum()) <= MAX_ITEMS and int(point.sum()) <= MAX_ITEMS, (int(frame.sum()), int(point.sum()), "the factor 1.001 of the bounds")
    pad_f = lambda a: np.concatenate([a.reshape((nf,) + a.shape[2:]), np.zeros((npt,) + a.shape[2:], a.dtype)])
    pad_p = lambda a: np.concatenate([np.zeros((nf,) + a.shape[2:], a.dtype), a.reshape((npt,) + a.shape[2:])])
    flat = dict(rot_t=pad_f(rot_t), trans_t=pad_f(c["trans_t"]), rot_p=pad_f(c["rot_p"]), trans_p=pad_f(c["trans_p"]), pos_t=pad_p(pos_t), pos_p=pad_p(c["pos_p"]))
    got = FP.fape_chain(flat, pad_f(frame), pad_p(point), None if w is None else pad_f(np.asarray(w, np.float64)), clamp, eps)
    for k in FRAME_KEYS:
        out[k] = got[k][:nf].reshape(out[k].shape)
    for k in POINT_KEYS:
        out[k] = got[k][nf:].reshape(out[k].shape)
    return out


def _ref(inp, ranges, w, clamp, eps, table=None, alt=None):
    R, A = inp["mask_t"].shape
    out = _empty(R, A)
    for lo, hi in ranges:
        got = chain({k: None if v is None else v[lo:hi] for k, v in inp.items()}, None if w is None else w[lo:hi], clamp, eps, table, alt)
        for k in REF_KEYS:
            out[k][lo:hi] = got[k]
    return out


def ref_padded(inp, length, w=None, clamp=10.0, eps=1e-4, table=None, alt=None):
    """inp: the dict of ORDER's arrays [n, L, ..] (fm_p, mask_p, aatype, swapped may be None), length [n] or None, w [n, L, 8] or None"""
    n, L = inp["mask_t"].shape[:2]
    flat = {k: None if v is None else v.reshape((n * L,) + v.shape[2:]) for k, v in inp.items()}
    ranges = [(e * L, e * L + (L if length is None else min(int(length[e]), L))) for e in range(n)]
    got = _ref(flat, ranges, None if w is None else np.asarray(w).reshape(n * L, GROUPS), clamp, eps, table, alt)
    return {k: v.reshape((n, L) + v.shape[1:]) for k, v in got.items()}


def ref_packed(inp, row_off, w=None, clamp=10.0, eps=1e-4, table=None, alt=None):
    """the same for [R, ..] and row_off [n + 1]; a chain's range is clamped to R and empty when it runs backwards"""
    R = inp["mask_t"].shape[0]
    ranges = []
    for e in range(len(row_off) - 1):
        lo, hi = min(int(row_off[e]), R), min(int(row_off[e + 1]), R)
        if hi > lo:
            ranges.append((lo, hi))
    return _ref(inp, ranges, w, clamp, eps, table, alt)


def pack_ref(ref, lens):
    return {k: AN.pack1(v, lens) for k, v in ref.items()}


def pack_inp(inp, lens):
    return {k: None if v is None else AN.pack1(v, lens) for k, v in inp.items()}


def tie_share(ref):
    """the share of the frame or point items with a non-zero tie allowance"""
    return float((ref["tie_f"] > 0).sum() + (ref["tie_p"] > 0).sum()) / max(int(ref["frame"].sum() + ref["point"].sum()), 1)


check_value = FP.check_value                      # (sum, points) against sum / points / b_sum / frame: the shapes carry the eight groups


def check_grad(got, ref, what=""):
    """(grad_rot, grad_trans, grad_pos) of the device against the restatement: each within its bound in its largest component, exactly
    0 at items that are no frame / slots that are no point -> the three largest observed ratios"""
    grot, gtr, gpos = got
    assert all(a.dtype == F for a in got) and grot.shape == ref["grad_rot"].shape and gtr.shape == ref["grad_trans"].shape and gpos.shape == ref["grad_pos"].shape
    assert not grot.view(np.uint32)[~ref["frame"]].any() and not gtr.view(np.uint32)[~ref["frame"]].any(), (what, "a gradient at an item that is no frame")
    assert not gpos.view(np.uint32)[~ref["point"]].any(), (what, "a gradient at a slot that is no point")
    ratios = (FP._ratio(np.abs(grot.astype(np.float64) - ref["grad_rot"]).max(axis=(-1, -2)), ref["b_rot"], what, "grad_rot"),
              FP._ratio(np.abs(gtr.astype(np.float64) - ref["grad_trans"]).max(axis=-1), ref["b_trans"], what, "grad_trans"),
              FP._ratio(np.abs(gpos.astype(np.float64) - ref["grad_pos"]).max(axis=-1), ref["b_pos"], what, "grad_pos"))
    print(f"{what}: grad_rot / grad_trans / grad_pos, largest |error| / bound = {ratios[0]:.4f} / {ratios[1]:.4f} / {ratios[2]:.4f}; "
          f"share of items with a tie allowance {tie_share(ref):.4f}")
    return ratios


# ---- the inputs the CPU and the GPU tests share -----------------------------------------------------------------------------------

def lattice(lens, L, A, seed, behind="nan", full=(), frames=0.7):
    """integer-lattice chains (every e an exact integer): coordinates and trans integers, rot one of the 24 proper signed permutations,
    pred = truth + small integer steps and another permutation; about half the frame items cleared (each side keeps `frames` of its
    mask, groups 1 and 2 included: the kernel takes the masks as they come), ~10 % of the point masks of either side (NaN patterns
    under every cleared mask); aatype cycles through ASP, GLU, PHE, TYR and types without a swap (0, 7, 19, 20, 255) and about a third
    of the rows of every kind are swapped, so swaps land on cleared true slots as well; per chain of 16 rows or more a NaN and an inf
    entry in a rot / trans under set masks of both sides, two points at +-3e19 in pred (a d that is not finite) and two non-finite
    coordinates in the truth (no point). The chains listed in `full` have every mask set and finite values. -> the dict of ORDER"""
    rng = np.random.default_rng(seed)
    n = len(lens)
    perms = FP.signed_permutations()
    d = dict(pos_t=rng.integers(-6, 7, size=(n, L, A, 3)).astype(F), trans_t=rng.integers(-6, 7, size=(n, L, GROUPS, 3)).astype(F),
             rot_t=perms[rng.integers(0, 24, size=(n, L, GROUPS))], rot_p=perms[rng.integers(0, 24, size=(n, L, GROUPS))])
    d["pos_p"] = d["pos_t"] + rng.integers(-2, 3, size=(n, L, A, 3)).astype(F)
    d["trans_p"] = d["trans_t"] + rng.integers(-2, 3, size=(n, L, GROUPS, 3)).astype(F)
    d["mask_t"], d["mask_p"] = (rng.random((n, L, A)) >= 0.10).astype(np.uint8), (rng.random((n, L, A)) >= 0.10).astype(np.uint8)
    d["fm_t"], d["fm_p"] = (rng.random((n, L, GROUPS)) < frames).astype(np.uint8), (rng.random((n, L, GROUPS)) < frames).astype(np.uint8)
    types = np.asarray((ASP, 0, GLU, 7, PHE, 19, TYR, 20, 255), np.uint8)
    d["aatype"] = types[np.arange(n * L) % len(types)].reshape(n, L).copy()
    d["swapped"] = (rng.random((n, L)) < 0.35).astype(np.uint8)
    for e, m in enumerate(lens):
        if e in full:
            for k in ("mask_t", "mask_p", "fm_t", "fm_p"):
                d[k][e] = 1
        elif m >= 16:
            r = rng.choice(m, size=8, replace=False)
            g = rng.integers(0, GROUPS, size=4) if A != 4 else np.asarray([0, 3, 0, 3])
            a = rng.integers(0, A, size=4)
            d["rot_t"][e, r[0], g[0], 1, 2] = np.nan; d["trans_t"][e, r[1], g[1], 0] = np.inf
            d["rot_p"][e, r[2], g[2], 0, 0] = -np.inf; d["trans_p"][e, r[3], g[3], 2] = np.nan
            for k in range(4):
                d["fm_t"][e, r[k], g[k]] = 1; d["fm_p"][e, r[k], g[k]] = 1
            d["pos_p"][e, r[4], a[0], 0] = 3e19; d["pos_p"][e, r[5], a[1], 1] = -3e19
            d["pos_t"][e, r[6], a[2], 0] = np.nan; d["pos_t"][e, r[7], a[3], 2] = np.inf
            d["swapped"][e, r[4:]] = 0                                    # (so that the slots named here are the ones the sweep reads)
            for k in range(4):
                d["mask_t"][e, r[4 + k], a[k]] = 1; d["mask_p"][e, r[4 + k], a[k]] = 1
        if behind == "nan":
            for k in ("pos_t", "pos_p", "rot_t", "rot_p", "trans_t", "trans_p"):
                d[k][e, m:] = np.nan
    for pos, mask in (("pos_t", "mask_t"), ("pos_p", "mask_p")):
        d[pos].view(np.uint32)[d[mask] == 0] = NAN_BITS
    for side in "tp":
        d["rot_" + side].view(np.uint32)[d["fm_" + side] == 0] = NAN_BITS
        d["trans_" + side].view(np.uint32)[d["fm_" + side] == 0] = NAN_BITS
    return {k: np.ascontiguousarray(d[k]) for k in ORDER}


NOISY_LENS, NOISY_SEED = (33, 65, 128), 47
NOISY_GROUPS, NOISY_SLOTS = (0, 3, 4, 5), (0, 1, 2, 3, 4, 5, 6, 7)


def noisy(lens=NOISY_LENS, A=14, seed=NOISY_SEED):
    """noisy chains of 4 frames x 8 atoms a residue: CA on a random walk of 3.8 A steps, the atoms scattered 1.5 A about it, pred =
    true + 0.5 A; true frames random rotations about an origin 1.5 A from the CA, pred frames those turned by about 0.15 rad and moved
    by 0.5 A; ~5 % of the true frame items and point slots cleared, no masks of the prediction; every ASP / GLU / PHE / TYR row
    swapped, every fourth other row as well (bytes equal to not swapped); rows behind the length hold NaN -> the dict of ORDER"""
    rng = np.random.default_rng(seed)
    n, L = len(lens), max(lens)
    step = rng.standard_normal((n, L, 3))
    ca = np.cumsum(3.8 * step / np.linalg.norm(step, axis=-1, keepdims=True), axis=1)
    true = (ca[:, :, None, :] + rng.standard_normal((n, L, A, 3)) * 1.5 / FP.SQ3).astype(F)
    pred = (true + (rng.standard_normal((n, L, A, 3)) * 0.5 / FP.SQ3).astype(F)).astype(F)
    mt = np.zeros((n, L, A), np.uint8)
    mt[..., list(NOISY_SLOTS)] = rng.random((n, L, len(NOISY_SLOTS))) >= 0.05
    rt = FP.random_rotations(rng, (n, L, GROUPS))
    rp = FP.small_rotations(rng, (n, L, GROUPS), 0.15) @ rt
    tt = (ca[:, :, None, :] + rng.standard_normal((n, L, GROUPS, 3)) * 1.5 / FP.SQ3).astype(F)
    tp = (tt + (rng.standard_normal((n, L, GROUPS, 3)) * 0.5 / FP.SQ3).astype(F)).astype(F)
    fm = np.zeros((n, L, GROUPS), np.uint8)
    fm[..., list(NOISY_GROUPS)] = rng.random((n, L, len(NOISY_GROUPS))) >= 0.05
    types = np.asarray((ASP, 0, GLU, 7, PHE, 19, TYR, 11), np.uint8)
    aa = types[np.arange(n * L) % len(types)].reshape(n, L).copy()
    sw = (np.isin(aa, (ASP, GLU, PHE, TYR)) | (np.arange(n * L).reshape(n, L) % 4 == 1)).astype(np.uint8)
    d = dict(rot_t=rt.astype(F), trans_t=tt, fm_t=fm, pos_t=true, mask_t=mt, aatype=aa, swapped=sw, rot_p=rp.astype(F), trans_p=tp, fm_p=None, pos_p=pred, mask_p=None)
    for e, m in enumerate(lens):
        for k in ("rot_t", "rot_p", "trans_t", "trans_p", "pos_t", "pos_p"):
            d[k][e, m:] = np.nan
    return d


def noisy_batch():
    """-> dict(lens, L, inp, w)"""
    L = max(NOISY_LENS)
    return dict(lens=np.asarray(NOISY_LENS, np.uint32), L=L, inp=noisy(), w=weights((len(NOISY_LENS), L, GROUPS), NOISY_SEED + 1))


SYNTH_SEED = 53


def synthetic_lens(T):
    """the lengths of the atom14 lattice batch for a frame tile of T rows: no row, one, two, the tile's edges, and a chain of more
    than two point passes when every mask is set (150 rows: 2100 points over passes of 1008)"""
    return [0, 1, 2, T - 1, T, T + 1, 150]


def synthetic_batch(T):
    """the atom14 lattice batch with its weights; the last chain has every mask set -> dict(lens, L, inp, w)"""
    lens = synthetic_lens(T)
    L = max(lens)
    return dict(lens=np.asarray(lens, np.uint32), L=L, inp=lattice(lens, L, 14, SYNTH_SEED, full=(len(lens) - 1,)), w=weights((len(lens), L, GROUPS), SYNTH_SEED + 1))


def backbone_batch(P):
    """backbone4 with every mask set, sized from the point pass P: a chain whose points close a pass at its fullest (P / 4 rows), one
    slot under it (the same rows, one mask cleared), and more than two passes (P / 2 + 3 rows) -> dict(lens, L, inp, w)"""
    lens = [P // 4, P // 4, P // 2 + 3]
    L = max(lens)
    inp = lattice(lens, L, 4, SYNTH_SEED + 2, full=(0, 1, 2))
    inp["mask_t"][1, 5, 2] = 0
    return dict(lens=np.asarray(lens, np.uint32), L=L, inp=inp, w=weights((3, L, GROUPS), SYNTH_SEED + 3))


# ---- the device calls -------------------------------------------------------------------------------------------------------------

def value_spec(lead):
    return dict(sum=(F, tuple(lead) + (GROUPS,)), points=(np.int32, tuple(lead) + (GROUPS,)))


def grad_spec(lead, A):
    return dict(grad_rot=(F, tuple(lead) + (GROUPS, 3, 3)), grad_trans=(F, tuple(lead) + (GROUPS, 3)), grad_pos=(F, tuple(lead) + (A, 3)))


def to_dev(inp):
    """the dict of ORDER on the device, in the C-ABI's order (None stays None)"""
    from _devpath import to_dev as up
    return [None if inp[k] is None else up(inp[k]) for k in ORDER]


def run_value(codec, dev, bound_t, n, rows, layout, packed, clamp=10.0, eps=1e-4, table=None, guard=GUARD, expect=0):
    """fcz_fape_atoms_dev (rows = L) or fcz_fape_atoms_packed_dev (rows = R) on the twelve device tensors -> (sum, points), guards checked"""
    import torch
    g = DevGuarded(value_spec((rows,) if packed else (n, rows)), guard)
    fn = codec.lib.fcz_fape_atoms_packed_dev if packed else codec.lib.fcz_fape_atoms_dev
    torch.cuda.synchronize()
    rc = fn(codec.ctx, *(ptr(t) for t in dev), ptr(bound_t), n, rows, layout, clamp, eps, None if table is None else table.ctypes.data, *g.ptrs())
    codec.synchronize()
    assert rc == expect, rc
    return g.all()


def run_grad(codec, dev, bound_t, n, rows, layout, packed, w, clamp=10.0, eps=1e-4, table=None, guard=GUARD, expect=0):
    """fcz_fape_atoms_grad_dev or _grad_packed_dev, w a device tensor -> (grad_rot, grad_trans, grad_pos), guards checked"""
    import torch
    A = {v: k for k, v in LAYOUT.items()}[layout]
    g = DevGuarded(grad_spec((rows,) if packed else (n, rows), A), guard)
    fn = codec.lib.fcz_fape_atoms_grad_packed_dev if packed else codec.lib.fcz_fape_atoms_grad_dev
    torch.cuda.synchronize()
    rc = fn(codec.ctx, *(ptr(t) for t in dev), ptr(bound_t), n, rows, layout, clamp, eps, None if table is None else table.ctypes.data, w.data_ptr(), *g.ptrs())
    codec.synchronize()
    assert rc == expect, rc
    return g.all()


def run_both(codec, dev, bound_t, n, rows, layout, packed, w, **kw):
    """-> (sum, points, grad_rot, grad_trans, grad_pos)"""
    return tuple(run_value(codec, dev, bound_t, n, rows, layout, packed, **kw)) + tuple(run_grad(codec, dev, bound_t, n, rows, layout, packed, w, **kw))


# ---- the three sweeps past their persistent grids (tests/_sweep_grids.py's engine) --------------------------------------------------
FAPEA_PASS = 1024               # fcz_fape_atoms.h: constexpr uint32_t FAPEA_PASS = 1024 (fcz_fape_atoms_pass())
FAPEA_PER_CU = 12               # fcz_abi.hip, fapea_rows: chain_tiles frames(ctx, packed, n, rows, fapea_tile_rows(A), 12u), the atom sweep alike


def fapea_tile_rows(A):
    """fcz_fape_atoms.h: A == 4u ? 128u : 64u"""
    return 128 if A == 4 else 64


class FapeAtoms(G.Analysis):
    """the value and the two gradient sweeps of one call each: the frame sweeps over fapea_tile_rows(A) rows a tile, the point sweep
    over lddta_tile_rows(A, false), 12 blocks a CU each. The pool is the integer lattice: no tie allowance at any length"""
    family = "fape_atoms"
    per_cu = FAPEA_PER_CU
    clamp = LATTICE_CLAMP

    def __init__(self, A=14):
        self.A, self.tile_rows, self.name = A, fapea_tile_rows(A), f"fape_atoms A={A}"

    def launches(self):
        return [(f"{self.name} value", fapea_tile_rows(self.A), self.per_cu), (f"{self.name} grad frames", fapea_tile_rows(self.A), self.per_cu),
                (f"{self.name} grad points", G.lddta_tile_rows(self.A, False), self.per_cu)]

    def pool(self, lens, L):
        inp = lattice(lens, L, self.A, SYNTH_SEED + 7, behind="data", full=(int(np.argmax(lens)),))
        return dict(inp, w=weights((len(lens), L, GROUPS), SYNTH_SEED + 8))

    def ref(self, inp, lens):
        return ref_padded({k: inp[k] for k in ORDER}, lens, inp["w"], self.clamp)

    def fair(self, inp, ref, lens):
        assert tie_share(ref) == 0 and ref["frame"].any() and ref["point"].any()
        if max(lens) * self.A > FAPEA_PASS:                                    # (a pool of long chains: its fullest one takes more than a pass)
            assert int(ref["points"].max()) > FAPEA_PASS, (int(ref["points"].max()), "the long chain takes one pass only")

    def run(self, codec, dev, bound_t, n, rows, packed):
        got = run_both(codec, [dev[k] for k in ORDER], bound_t, n, rows, self.layout, packed, dev["w"], clamp=self.clamp, guard=self.guard)
        return dict(zip(OUT_KEYS, got))

    def check(self, got, exp, what):
        check_value((got["sum"], got["points"]), exp, what)
        check_grad((got["grad_rot"], got["grad_trans"], got["grad_pos"]), exp, what)
