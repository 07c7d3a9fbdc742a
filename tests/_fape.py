"""The backbone FAPE and its gradient restated in numpy FLOAT64 (include/fcz_hip.h, fcz_fape_dev / fcz_fape_grad_dev), the bounds the
device results are held to, the inputs the CPU and the GPU tests share, and the device calls into 0xA5-filled arrays.

Per chain: row i is a FRAME when both frame masks are set and its 24 floats are finite, row j a POINT by tests/_lddt.py's site rule;
both are float32 facts. Whether the float32 d of a term is finite is a float32 fact too (3e19 squared overflows float32, not float64)
and is taken from a float32 evaluation of the stated operations. Everything else is float64 on the float32 inputs:
    u = x_j - t_i, l = R_i^T u (pred), u', l' (true), e = l - l', d = sqrt(|e|^2 + eps), term = min(d, clamp)
    sum[i] = sum_j term          h = e / d where d < clamp, else 0
    grad_rot[i] = w_i sum_j u (x) h      grad_trans[i] = -w_i R_i sum_j h      grad_pos[j] = sum_i w_i R_i h_ij

The bounds, derived from the rounding of the stated operations (eps_m = 2^-24, the unit roundoff; never fitted to device output), for
rotations whose columns have unit length, so that sum_a |R[a][k]| |u_a| <= sqrt(3) X with X = max(|u|_inf, |u'|_inf) of the term:
  * u_a carries one rounding, a product one, the two additions of l_k two: |dl_k| <= 4 sqrt(3) X eps_m = 6.93 X eps_m, the same for l';
    e_k = l_k - l'_k adds eps_m |e_k|: |de_k| <= 13.86 X eps_m + eps_m |e_k|, |de|_2 <= 24 X eps_m + eps_m |e|_2.
  * d = sqrt(s + eps): dd <= |de|_2 |e| / d + (3 roundings of s and one of s + eps: 4 eps_m (s + eps), halved by the root, plus the
    root's own) 3 eps_m d  =>  |d - exact| <= T = (26 X + 4 d) eps_m. (A numpy float32 evaluation of noisy walks differs from
    float64 by about 3 X eps_m: the products of a term do not all round the same way. 26 is the worst case of the 24 derived above
    and the eps_m |e|_2 <= eps_m d term folded into 4 d, with the slack for columns normalised in float32.)
  * sum: |sum - ref| <= sum_j T_ij + P eps_m S, S = ref (a sequential float32 sum of P non-negative terms).
  * h_k = e_k * rcp(d): |dh_k| <= |de_k| / d + |e_k| dd / d^2 + 3 eps_m (the reciprocal within an ulp, the product)
    <= (13.86 + 26) X eps_m / d + (1 + 4 + 3) eps_m = HB = (40 X / d + 8) eps_m.
  * grad_rot[i][a][k] = w_i sum_j u_a h_k: |u_a| <= X, |h_k| <= 1, two roundings a product, P for the sum, one for w:
    <= |w_i| (sum_j X HB + (P + 3) eps_m sum_j X) over the moving terms.
  * grad_trans[i]: |row of R|_1 <= sqrt(3), |sum_j h_k| <= Pm (the moving terms): <= sqrt(3) |w_i| (sum_j HB + (Pm + 4) eps_m Pm).
  * grad_pos[j] = sum_i w_i (R_i h_ij): <= sqrt(3) (sum_i |w_i| HB + (Fm + 4) eps_m sum_i |w_i|) over the moving frames.
Each of the last four carries a factor 1.001 for the second-order terms (P eps_m <= 1.3e-4 for the longest chain here).
The gradient switches off at d >= clamp: a term whose float64 d lies within T of clamp may honestly fall on either side. It gets a
`tie` allowance, the size of the term it may add or drop: |w_i| in grad_trans[i] and grad_pos[j] (|R h|_inf <= |h|_2 <= 1) and
|w_i| X in grad_rot[i]. An allowance, not an exclusion; tie_share() must stay at or below 0.02 on every noisy input."""
import itertools

import numpy as np

import _analysis as AN
from _analysis import NAN_BITS, ptr
from _devpath import GUARD, DevGuarded
from _lddt import _site
from _lddt_soft import walk, weights

F = np.float32
EPS_M = 2.0 ** -24
SQ3 = np.sqrt(3.0)
ORDER = ("rot_t", "trans_t", "fm_t", "pos_t", "mask_t", "rot_p", "trans_p", "fm_p", "pos_p", "mask_p")   # the C-ABI's order
OUT_KEYS = ("sum", "points", "grad_rot", "grad_trans", "grad_pos")
REF_KEYS = OUT_KEYS + ("b_sum", "b_rot", "b_trans", "b_pos", "tie_f", "tie_p", "frame", "point", "clamped", "terms")
CHUNK = 128


def _local32(R, t, x):
    """float32, the stated operations: R [f, 3, 3], t [f, 3], x [p, 3] -> l [f, p, 3]"""
    u = [x[None, :, a] - t[:, None, a] for a in range(3)]
    return np.stack([(R[:, 0, k, None] * u[0] + R[:, 1, k, None] * u[1]) + R[:, 2, k, None] * u[2] for k in range(3)], axis=-1)


def _local64(R, t, x):
    u = x[None, :, :].astype(np.float64) - t[:, None, :].astype(np.float64)
    return u, np.einsum("fak,fpa->fpk", R.astype(np.float64), u)


def _empty(m):
    z = lambda *s: np.zeros((m,) + s)
    return dict(sum=z(), points=np.zeros(m, np.int32), grad_rot=z(3, 3), grad_trans=z(3), grad_pos=z(3), b_sum=z(), b_rot=z(), b_trans=z(), b_pos=z(),
                tie_f=z(), tie_p=z(), frame=np.zeros(m, bool), point=np.zeros(m, bool), clamped=z(), terms=z())


def fape_chain(c, frame, point, w=None, clamp=10.0, eps=1e-4):
    """c: the ten arrays of one chain of m rows with pos already cut to the slot ([m, 3]); frame, point bool [m]; w [m] or None
    (zeros) -> the dict of REF_KEYS"""
    m = len(frame)
    out = _empty(m)
    out["frame"], out["point"] = frame.copy(), point.copy()
    fi, pj = np.flatnonzero(frame), np.flatnonzero(point)
    if len(fi) == 0 or len(pj) == 0:
        return out
    ww = np.zeros(m) if w is None else np.asarray(w, np.float64)
    x, y = np.ascontiguousarray(c["pos_p"][pj], F), np.ascontiguousarray(c["pos_t"][pj], F)
    clamp64, eps32 = np.float64(F(clamp)), F(eps)
    P = len(pj)
    for f0 in range(0, len(fi), CHUNK):
        rows = fi[f0:f0 + CHUNK]
        Rp, tp, Rt, tt = (np.ascontiguousarray(c[k][rows], F) for k in ("rot_p", "trans_p", "rot_t", "trans_t"))
        with np.errstate(all="ignore"):
            e32 = _local32(Rp, tp, x) - _local32(Rt, tt, y)
            d32 = np.sqrt(((e32[..., 0] * e32[..., 0] + e32[..., 1] * e32[..., 1]) + e32[..., 2] * e32[..., 2]) + eps32)
            assert d32.dtype == F
            live = np.isfinite(d32)
            u, l = _local64(Rp, tp, x)
            ut, lt = _local64(Rt, tt, y)
            e = np.where(live[..., None], l - lt, 0.0)
            u = np.where(live[..., None], u, 0.0)
            X = np.where(live, np.maximum(np.abs(u).max(axis=-1), np.abs(np.where(live[..., None], ut, 0.0)).max(axis=-1)), 0.0)
        d = np.sqrt((e * e).sum(axis=-1) + np.float64(eps32))
        T = (26.0 * X + 4.0 * d) * EPS_M
        term = np.where(live, np.minimum(d, clamp64), 0.0)
        moving = live & (d < clamp64)
        tie = live & (np.abs(d - clamp64) <= T)
        h = np.where(moving[..., None], e / d[..., None], 0.0)
        wf = ww[rows]
        S = term.sum(axis=1)
        out["sum"][rows] = S
        out["points"][rows] = P
        out["terms"][rows] = live.sum(axis=1)
        out["clamped"][rows] = (live & ~moving).sum(axis=1)
        out["b_sum"][rows] = (np.where(live, T, 0.0).sum(axis=1) + P * EPS_M * S) * 1.001
        out["grad_rot"][rows] = wf[:, None, None] * np.einsum("fpa,fpk->fak", u, h)
        H = h.sum(axis=1)
        out["grad_trans"][rows] = -wf[:, None] * np.einsum("fak,fk->fa", Rp.astype(np.float64), H)
        out["grad_pos"][pj] += np.einsum("f,fak,fpk->pa", wf, Rp.astype(np.float64), h)
        HB = np.where(moving, (40.0 * X / d + 8.0) * EPS_M, 0.0)
        Xm = np.where(moving, X, 0.0)
        Pm = moving.sum(axis=1)
        aw = np.abs(wf)
        out["b_rot"][rows] = aw * ((Xm * HB).sum(axis=1) + (P + 3) * EPS_M * Xm.sum(axis=1)) * 1.001
        out["b_trans"][rows] = SQ3 * aw * (HB.sum(axis=1) + (Pm + 4) * EPS_M * Pm) * 1.001
        out["b_pos"][pj] += SQ3 * (aw[:, None] * HB).sum(axis=0) * 1.001
        out["tie_f"][rows] = aw * tie.sum(axis=1)
        out["b_rot"][rows] += aw * np.where(tie, X, 0.0).sum(axis=1)
        out["b_trans"][rows] += out["tie_f"][rows]
        out["tie_p"][pj] += (aw[:, None] * tie).sum(axis=0)
        out.setdefault("_aw", np.zeros(m))[pj] += (aw[:, None] * moving).sum(axis=0)
        out.setdefault("_fm", np.zeros(m))[pj] += moving.sum(axis=0)
    out["b_pos"] += SQ3 * (out.pop("_fm") + 4) * EPS_M * out.pop("_aw") * 1.001 + out["tie_p"]
    out["b_pos"][~point] = 0.0
    return out


def _rows(inp, slot):
    """the ten arrays flattened to rows -> (dict with pos cut to the slot, frame bool [R], point bool [R])"""
    lead = inp["fm_t"].shape
    R = int(np.prod(lead))
    A = inp["pos_t"].shape[-2]
    c = dict(rot_t=inp["rot_t"].reshape(R, 3, 3), trans_t=inp["trans_t"].reshape(R, 3), rot_p=inp["rot_p"].reshape(R, 3, 3), trans_p=inp["trans_p"].reshape(R, 3),
             pos_t=inp["pos_t"].reshape(R, A, 3)[:, slot], pos_p=inp["pos_p"].reshape(R, A, 3)[:, slot])
    frame = inp["fm_t"].reshape(R) != 0
    if inp.get("fm_p") is not None:
        frame &= inp["fm_p"].reshape(R) != 0
    with np.errstate(all="ignore"):
        for k in ("rot_t", "rot_p"):
            frame &= np.isfinite(c[k]).all(axis=(1, 2))
        for k in ("trans_t", "trans_p"):
            frame &= np.isfinite(c[k]).all(axis=1)
    point = _site(inp["pos_t"].reshape(R, A, 3), inp["mask_t"].reshape(R, A), inp["pos_p"].reshape(R, A, 3),
                  None if inp.get("mask_p") is None else inp["mask_p"].reshape(R, A), slot)
    return c, frame, point


def _ref(inp, slot, ranges, w, clamp, eps):
    c, frame, point = _rows(inp, slot)
    R = len(frame)
    out = _empty(R)
    wr = None if w is None else np.asarray(w).reshape(R)
    for lo, hi in ranges:
        got = fape_chain({k: v[lo:hi] for k, v in c.items()}, frame[lo:hi], point[lo:hi], None if wr is None else wr[lo:hi], clamp, eps)
        for k in REF_KEYS:
            out[k][lo:hi] = got[k]
    return out


def fape_padded(inp, length, slot, w=None, clamp=10.0, eps=1e-4):
    """inp: the dict of ORDER's arrays, [n, L, ..] (fm_p / mask_p may be None), length [n] or None, w [n, L] or None -> REF_KEYS, [n, L, ..]"""
    n, L = inp["fm_t"].shape
    ranges = [(e * L, e * L + (L if length is None else min(int(length[e]), L))) for e in range(n)]
    return {k: v.reshape((n, L) + v.shape[1:]) for k, v in _ref(inp, slot, ranges, w, clamp, eps).items()}


def fape_packed(inp, row_off, slot, w=None, clamp=10.0, eps=1e-4):
    """the same for [R, ..] and row_off [n + 1]; a chain's range is clamped to R and empty when it runs backwards"""
    R = inp["fm_t"].shape[0]
    ranges = []
    for e in range(len(row_off) - 1):
        lo, hi = min(int(row_off[e]), R), min(int(row_off[e + 1]), R)
        if hi > lo:
            ranges.append((lo, hi))
    return _ref(inp, slot, ranges, w, clamp, eps)


def pack_ref(ref, lens):
    return {k: AN.pack1(v, lens) for k, v in ref.items()}


def pack_inp(inp, lens):
    return {k: None if v is None else AN.pack1(v, lens) for k, v in inp.items()}


def tie_share(ref):
    """the share of the frame or point rows with a non-zero tie allowance"""
    return float(((ref["tie_f"] > 0) | (ref["tie_p"] > 0)).sum()) / max(int((ref["frame"] | ref["point"]).sum()), 1)


def _ratio(err, bound, what, name):
    assert not err[bound == 0].any(), (what, name, "where nothing may differ", np.argwhere((bound == 0) & (err > 0))[:4])
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    assert (err <= bound).all(), (what, name, np.argwhere(err > bound)[:4], ratio)
    return ratio


def check_value(got, ref, what=""):
    """(sum, points) of the device against the restatement: points exact, sum within its bound, both exactly 0 at rows that are no
    frame -> the largest observed ratio to the bound"""
    total, points = got
    assert total.dtype == F and points.dtype == np.int32 and total.shape == ref["sum"].shape, (what, total.dtype, points.dtype, total.shape)
    assert np.array_equal(points, ref["points"]), (what, "points", np.argwhere(points != ref["points"])[:4])
    assert not total.view(np.uint32)[~ref["frame"]].any(), (what, "sum at a row that is no frame")
    ratio = _ratio(np.abs(total.astype(np.float64) - ref["sum"]), ref["b_sum"], what, "sum")
    print(f"{what}: sum, largest |error| / bound = {ratio:.4f} ({int(ref['frame'].sum())} frames, most points {int(ref['points'].max(initial=0))}, "
          f"{int(ref['clamped'].sum())} of {int(ref['terms'].sum())} terms clamped)")
    return ratio


def check_grad(got, ref, what=""):
    """(grad_rot, grad_trans, grad_pos) of the device against the restatement: each within its bound in its largest component, exactly
    0 at rows that are no frame / no point -> the three largest observed ratios"""
    grot, gtr, gpos = got
    assert all(a.dtype == F for a in got) and grot.shape == ref["grad_rot"].shape and gtr.shape == ref["grad_trans"].shape and gpos.shape == ref["grad_pos"].shape
    assert not grot.view(np.uint32)[~ref["frame"]].any() and not gtr.view(np.uint32)[~ref["frame"]].any(), (what, "a gradient at a row that is no frame")
    assert not gpos.view(np.uint32)[~ref["point"]].any(), (what, "a gradient at a row that is no point")
    ratios = (_ratio(np.abs(grot.astype(np.float64) - ref["grad_rot"]).max(axis=(-1, -2)), ref["b_rot"], what, "grad_rot"),
              _ratio(np.abs(gtr.astype(np.float64) - ref["grad_trans"]).max(axis=-1), ref["b_trans"], what, "grad_trans"),
              _ratio(np.abs(gpos.astype(np.float64) - ref["grad_pos"]).max(axis=-1), ref["b_pos"], what, "grad_pos"))
    print(f"{what}: grad_rot / grad_trans / grad_pos, largest |error| / bound = {ratios[0]:.4f} / {ratios[1]:.4f} / {ratios[2]:.4f}; "
          f"share of rows with a tie allowance {tie_share(ref):.4f}")
    return ratios


# ---- the inputs the CPU and the GPU tests share -----------------------------------------------------------------------------------

def signed_permutations():
    """the 24 proper signed permutation matrices, float32 [24, 3, 3]"""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            m = np.zeros((3, 3))
            for a in range(3):
                m[a, perm[a]] = signs[a]
            if np.linalg.det(m) > 0:
                out.append(m)
    assert len(out) == 24
    return np.asarray(out, F)


def random_rotations(rng, shape):
    """float64 [shape, 3, 3] proper rotations, uniform (QR of a gaussian matrix, signs fixed)"""
    q, r = np.linalg.qr(rng.standard_normal(tuple(shape) + (3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=-2, axis2=-1))[..., None, :]
    q[..., :, 2] *= np.sign(np.linalg.det(q))[..., None]
    return q


def small_rotations(rng, shape, angle):
    """rotations by about `angle` radians about random axes, float64"""
    ax = rng.standard_normal(tuple(shape) + (3,))
    ax /= np.linalg.norm(ax, axis=-1, keepdims=True)
    th = angle * (1.0 + 0.3 * rng.standard_normal(tuple(shape)))
    K = np.zeros(tuple(shape) + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0], K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -ax[..., 2], ax[..., 1], ax[..., 2], -ax[..., 0], -ax[..., 1], ax[..., 0]
    return np.eye(3) + np.sin(th)[..., None, None] * K + (1 - np.cos(th))[..., None, None] * (K @ K)


LATTICE_CLAMP = 10.25        # clamp^2 = 105.0625: no integer |e|^2 plus eps comes within 0.06 of it, so the lattice has no tie


def lattice(lens, L, A, slot, seed, behind="nan"):
    """integer-lattice chains (every e an exact integer): coordinates and trans integers, rot one of the 24 proper signed permutations,
    pred = truth + small integer steps and another permutation; ~10 % of the frame masks cleared in the truth only and ~10 % in the
    prediction only, the same for the point masks at `slot` (NaN patterns under every cleared mask); per chain of 16 rows or more a NaN
    and an inf entry in a rot / trans under a set mask, of both sides, two points at +-3e19 in pred (a d that is not finite) and two
    non-finite point coordinates in the truth (no point); NaN patterns in every row behind the length -> the dict of ORDER"""
    rng = np.random.default_rng(seed)
    n = len(lens)
    perms = signed_permutations()
    d = dict(pos_t=rng.integers(-6, 7, size=(n, L, A, 3)).astype(F), trans_t=rng.integers(-6, 7, size=(n, L, 3)).astype(F),
             rot_t=perms[rng.integers(0, 24, size=(n, L))], rot_p=perms[rng.integers(0, 24, size=(n, L))])
    d["pos_p"] = d["pos_t"] + rng.integers(-2, 3, size=(n, L, A, 3)).astype(F)
    d["trans_p"] = d["trans_t"] + rng.integers(-2, 3, size=(n, L, 3)).astype(F)
    d["mask_t"], d["mask_p"] = np.ones((n, L, A), np.uint8), np.ones((n, L, A), np.uint8)
    d["fm_t"], d["fm_p"] = np.ones((n, L), np.uint8), np.ones((n, L), np.uint8)
    u, v = rng.random((n, L)), rng.random((n, L))
    d["mask_t"][..., slot][u < 0.10] = 0
    d["mask_p"][..., slot][(u >= 0.10) & (u < 0.20)] = 0
    d["fm_t"][v < 0.10] = 0
    d["fm_p"][(v >= 0.10) & (v < 0.20)] = 0
    for e, m in enumerate(lens):
        if m >= 16:
            r = rng.choice(m, size=8, replace=False)
            d["rot_t"][e, r[0], 1, 2] = np.nan; d["trans_t"][e, r[1], 0] = np.inf; d["rot_p"][e, r[2], 0, 0] = -np.inf; d["trans_p"][e, r[3], 2] = np.nan
            d["fm_t"][e, r[:4]] = 1; d["fm_p"][e, r[:4]] = 1
            d["pos_p"][e, r[4], slot, 0] = 3e19; d["pos_p"][e, r[5], slot, 1] = -3e19
            d["pos_t"][e, r[6], slot, 0] = np.nan; d["pos_t"][e, r[7], slot, 2] = np.inf
            d["mask_t"][e, r[4:], slot] = 1; d["mask_p"][e, r[4:], slot] = 1
        if behind == "nan":
            for k in ("pos_t", "pos_p", "rot_t", "rot_p", "trans_t", "trans_p"):
                d[k][e, m:] = np.nan
    for pos, mask in (("pos_t", "mask_t"), ("pos_p", "mask_p")):
        d[pos].view(np.uint32)[d[mask] == 0] = NAN_BITS
    for side in "tp":
        d["rot_" + side].view(np.uint32)[d["fm_" + side] == 0] = NAN_BITS
        d["trans_" + side].view(np.uint32)[d["fm_" + side] == 0] = NAN_BITS
    return {k: np.ascontiguousarray(d[k]) for k in ORDER}


def walk_frames(lens, L, A, slot, seed):
    """noisy chains: _lddt_soft.walk's points (a random walk of 3.8 A steps, pred = true + 0.5 A), true frames random rotations about
    an origin 1.5 A from the point, pred frames those turned by about 0.15 rad and moved by 0.5 A; ~5 % of the true frame masks and
    point masks cleared, no masks of the prediction; rows behind the length hold NaN -> the dict of ORDER"""
    rng = np.random.default_rng(seed + 1000)
    true, mt, pred = walk(lens, L, A, slot, seed)
    n = len(lens)
    rt = random_rotations(rng, (n, L))
    rp = small_rotations(rng, (n, L), 0.15) @ rt
    tt = (true[:, :, slot].astype(np.float64) + rng.standard_normal((n, L, 3)) * 1.5 / SQ3).astype(F)
    tp = (tt + (rng.standard_normal((n, L, 3)) * 0.5).astype(F)).astype(F)
    fm = (rng.random((n, L)) >= 0.05).astype(np.uint8)
    d = dict(rot_t=rt.astype(F), trans_t=tt, fm_t=fm, pos_t=true, mask_t=mt, rot_p=rp.astype(F), trans_p=tp, fm_p=None, pos_p=pred, mask_p=None)
    for e, m in enumerate(lens):
        for k in ("rot_t", "rot_p", "trans_t", "trans_p"):
            d[k][e, m:] = np.nan
    return d


SYNTH_SEED, WALK_LENS, WALK_SEED = 41, (65, 257, 350), 43


def synthetic_lens(P):
    """the lengths of the lattice batch: the tile edges, one row, and more than two passes of P rows"""
    return [0, 1, 2, 63, 64, 65, 255, 256, 257, 2 * P + 3]


def synthetic_batch(P):
    """the lattice batch on backbone4 / CA with its weights -> dict(lens, L, inp, w)"""
    lens = synthetic_lens(P)
    L = max(lens)
    return dict(lens=np.asarray(lens, np.uint32), L=L, inp=lattice(lens, L, 4, 1, SYNTH_SEED), w=weights((len(lens), L), SYNTH_SEED + 1))


def walk_batch():
    """the noisy batch on atom14 / CB (slot 4) with its weights -> dict(lens, L, inp, w)"""
    L = max(WALK_LENS)
    return dict(lens=np.asarray(WALK_LENS, np.uint32), L=L, inp=walk_frames(WALK_LENS, L, 14, 4, WALK_SEED), w=weights((len(WALK_LENS), L), WALK_SEED + 1))


# ---- the device calls -------------------------------------------------------------------------------------------------------------

def value_spec(shape):
    return dict(sum=(F, tuple(shape)), points=(np.int32, tuple(shape)))


def grad_spec(shape):
    return dict(grad_rot=(F, tuple(shape) + (3, 3)), grad_trans=(F, tuple(shape) + (3,)), grad_pos=(F, tuple(shape) + (3,)))


def to_dev(inp):
    """the dict of ORDER on the device, in the C-ABI's order (None stays None)"""
    from _devpath import to_dev as up
    return [None if inp[k] is None else up(inp[k]) for k in ORDER]


def run_value(codec, dev, bound_t, n, rows, layout, slot, packed, clamp=10.0, eps=1e-4, guard=GUARD, expect=0):
    """fcz_fape_dev (rows = L) or fcz_fape_packed_dev (rows = R) on the ten device tensors -> (sum, points) as numpy, guards checked"""
    import torch
    g = DevGuarded(value_spec((rows,) if packed else (n, rows)), guard)
    fn = codec.lib.fcz_fape_packed_dev if packed else codec.lib.fcz_fape_dev
    torch.cuda.synchronize()
    rc = fn(codec.ctx, *(ptr(t) for t in dev), ptr(bound_t), n, rows, layout, slot, clamp, eps, *g.ptrs())
    codec.synchronize()
    assert rc == expect, rc
    return g.all()


def run_grad(codec, dev, bound_t, n, rows, layout, slot, packed, w, clamp=10.0, eps=1e-4, guard=GUARD, expect=0):
    """fcz_fape_grad_dev or fcz_fape_grad_packed_dev, w a device tensor -> (grad_rot, grad_trans, grad_pos) as numpy, guards checked"""
    import torch
    g = DevGuarded(grad_spec((rows,) if packed else (n, rows)), guard)
    fn = codec.lib.fcz_fape_grad_packed_dev if packed else codec.lib.fcz_fape_grad_dev
    torch.cuda.synchronize()
    rc = fn(codec.ctx, *(ptr(t) for t in dev), ptr(bound_t), n, rows, layout, slot, clamp, eps, w.data_ptr(), *g.ptrs())
    codec.synchronize()
    assert rc == expect, rc
    return g.all()


def run_both(codec, dev, bound_t, n, rows, layout, slot, packed, w, **kw):
    """-> (sum, points, grad_rot, grad_trans, grad_pos)"""
    return tuple(run_value(codec, dev, bound_t, n, rows, layout, slot, packed, **kw)) + tuple(run_grad(codec, dev, bound_t, n, rows, layout, slot, packed, w, **kw))
