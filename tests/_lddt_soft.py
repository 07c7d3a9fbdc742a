"""The smooth lDDT and its gradient restated in numpy FLOAT64 (include/fcz_hip.h, fcz_lddt_soft_dev / fcz_lddt_soft_grad_dev), the
bounds the device results are held to, the inputs the CPU and the GPU tests share, and the device calls into 0xA5-filled arrays.

Per chain: sites and pairs are tests/_lddt.py's, decided in float32 exactly as there, so `pairs` compares on integers. Whether a
predicted distance is infinite or zero is a float32 fact too (3e19 squared overflows float32, not float64) and is taken from the
float32 distance. Everything else is float64 on the float32 inputs: delta = |d_true - d_pred|, eps = 1/4 sum_k sigmoid(t_k - delta),
    soft[i] = sum_j eps_ij                 grad[i] = sum_j (w_i + w_j) eps'(delta_ij) sign(d_pred - d_true) (p_i - p_j) / d_pred
with eps' = -1/4 sum_k s_k (1 - s_k), sign(0) = 0, and no term from a pair whose d_pred is 0 or not finite.

The bounds (derived, not measured: a term is within 2^-19 for distances under 64 A, a sequential float32 sum of P terms adds at most
P^2 2^-24):   |soft - ref| <= P 2^-19 + P^2 2^-24          |grad - ref|_inf <= W 2^-19 + W P 2^-24 + tie
with W_i = sum_j |w_i + w_j| and tie_i = sum 2 c |w_i + w_j| over the pairs with 0 != delta <= 2^-21 (d_true + d_pred), in which
float32 may honestly take the other sign of d_pred - d_true (its error of delta is below 2^-22 (d_true + d_pred)); c = |eps'(0)|."""
import numpy as np

from _analysis import NAN_BITS, ptr
from _devpath import GUARD, DevGuarded
from _lddt import THRESHOLDS, _d, _site

F = np.float32


def _sig(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def eps(delta, thresholds=THRESHOLDS):
    return 0.25 * sum(_sig(np.float64(F(t)) - delta) for t in thresholds)


def deps(delta, thresholds=THRESHOLDS):
    return -0.25 * sum(_sig(np.float64(F(t)) - delta) * (1.0 - _sig(np.float64(F(t)) - delta)) for t in thresholds)


def _d64(p, q):
    d = p[None, :, :].astype(np.float64) - q[:, None, :].astype(np.float64)
    return np.sqrt((d * d).sum(axis=-1))


def soft_chain(t, p, site, w=None, cutoff=15.0, thresholds=THRESHOLDS):
    """t, p float32 [m, 3], site bool [m], w [m] or None (zeros) -> dict(soft float64 [m], pairs int32 [m], grad float64 [m, 3],
    W float64 [m], tie float64 [m])"""
    m = len(t)
    out = dict(soft=np.zeros(m), pairs=np.zeros(m, np.int32), grad=np.zeros((m, 3)), W=np.zeros(m), tie=np.zeros(m))
    js = np.flatnonzero(site)
    tt, pp = np.ascontiguousarray(t[js], F), np.ascontiguousarray(p[js], F)
    ww = np.zeros(len(js)) if w is None else np.asarray(w, np.float64)[js]
    c = -float(deps(0.0, thresholds))
    for q0 in range(0, len(js), 256):
        rows = js[q0:q0 + 256]
        k = len(rows)
        dt32, dp32 = _d(tt, tt[q0:q0 + k]), _d(pp, pp[q0:q0 + k])
        inc = dt32 < F(cutoff)
        inc[np.arange(k), np.arange(q0, q0 + k)] = False
        dt, dp = _d64(tt, tt[q0:q0 + k]), _d64(pp, pp[q0:q0 + k])
        live = inc & np.isfinite(dp32)                                    # a pair whose float32 delta is finite
        delta = np.where(live, np.abs(dt - dp), 0.0)
        out["soft"][rows] = np.where(live, eps(delta, thresholds), 0.0).sum(axis=1)
        out["pairs"][rows] = inc.sum(axis=1)
        wsum = ww[q0:q0 + k, None] + ww[None, :]
        out["W"][rows] = np.where(inc, np.abs(wsum), 0.0).sum(axis=1)
        moving = live & (dp32 != 0)
        coef = np.where(moving, wsum * deps(delta, thresholds) * np.sign(dp - dt) / np.where(moving, dp, 1.0), 0.0)
        diff = pp[q0:q0 + k, None, :].astype(np.float64) - pp[None, :, :].astype(np.float64)            # p_i - p_j
        out["grad"][rows] = (coef[:, :, None] * diff).sum(axis=1)
        near = moving & (delta != 0) & (delta <= 2.0 ** -21 * (dt + dp))
        out["tie"][rows] = np.where(near, 2.0 * c * np.abs(wsum), 0.0).sum(axis=1)
    return out


KEYS = ("soft", "pairs", "grad", "W", "tie")


def _empty(lead):
    return dict(soft=np.zeros(lead), pairs=np.zeros(lead, np.int32), grad=np.zeros(lead + (3,)), W=np.zeros(lead), tie=np.zeros(lead))


def soft_padded(pos_t, mask_t, pos_p, mask_p, length, slot, w=None, cutoff=15.0, thresholds=THRESHOLDS):
    """pos [n, L, A, 3], mask [n, L, A] (mask_p may be None), length [n] or None, w [n, L] or None -> the dict of soft_chain, [n, L]"""
    n, L = pos_t.shape[:2]
    out = _empty((n, L))
    site = _site(pos_t, mask_t, pos_p, mask_p, slot)
    for e in range(n):
        m = L if length is None else min(int(length[e]), L)
        got = soft_chain(pos_t[e, :m, slot], pos_p[e, :m, slot], site[e, :m], None if w is None else w[e, :m], cutoff, thresholds)
        for k in KEYS:
            out[k][e, :m] = got[k]
    out["site"] = site & (np.arange(L)[None, :] < (L if length is None else np.minimum(np.asarray(length, np.int64), L)[:, None]))
    return out


def soft_packed(pos_t, mask_t, pos_p, mask_p, row_off, slot, w=None, cutoff=15.0, thresholds=THRESHOLDS):
    """pos [R, A, 3], mask [R, A], row_off [n + 1], w [R] or None -> the dict of soft_chain, [R]; a chain's range is clamped to R and
    empty when it runs backwards (ranges must not overlap)"""
    R = pos_t.shape[0]
    out = _empty((R,))
    site = _site(pos_t, mask_t, pos_p, mask_p, slot)
    covered = np.zeros(R, bool)
    for e in range(len(row_off) - 1):
        lo, hi = min(int(row_off[e]), R), min(int(row_off[e + 1]), R)
        if hi <= lo:
            continue
        covered[lo:hi] = True
        got = soft_chain(pos_t[lo:hi, slot], pos_p[lo:hi, slot], site[lo:hi], None if w is None else w[lo:hi], cutoff, thresholds)
        for k in KEYS:
            out[k][lo:hi] = got[k]
    out["site"] = site & covered
    return out


def pack_ref(ref, lens):
    return {k: np.concatenate([v[e, :m] for e, m in enumerate(lens)]) for k, v in ref.items()}


def soft_bound(ref):
    P = ref["pairs"].astype(np.float64)
    return P * 2.0 ** -19 + P * P * 2.0 ** -24


def grad_bound(ref):
    P = ref["pairs"].astype(np.float64)
    return ref["W"] * 2.0 ** -19 + ref["W"] * P * 2.0 ** -24 + ref["tie"]


def check_value(got, ref, what=""):
    """(soft, pairs) of the device against the restatement: pairs exact, soft within its bound, exactly 0 where there is no pair ->
    the largest observed ratio to the bound"""
    soft, pairs = got
    assert soft.dtype == F and pairs.dtype == np.int32 and soft.shape == ref["soft"].shape, (what, soft.dtype, pairs.dtype, soft.shape)
    assert np.array_equal(pairs, ref["pairs"]), (what, "pairs", np.argwhere(pairs != ref["pairs"])[:4])
    assert not soft.view(np.uint32)[ref["pairs"] == 0].any(), (what, "soft where there is no pair")
    err, bound = np.abs(soft.astype(np.float64) - ref["soft"]), soft_bound(ref)
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f"{what}: soft, largest |error| / bound = {ratio:.4f} ({int((bound > 0).sum())} rows with a pair, most pairs {int(ref['pairs'].max(initial=0))})")
    assert (err <= bound).all(), (what, "soft", np.argwhere(err > bound)[:4], ratio)
    return ratio


def check_grad(grad, ref, what=""):
    """grad [.., 3] of the device against the restatement: within its bound in the largest component, exactly 0 at every row that is
    no site -> the largest observed ratio to the bound"""
    assert grad.dtype == F and grad.shape == ref["grad"].shape, (what, grad.dtype, grad.shape)
    assert not grad.view(np.uint32)[~ref["site"]].any(), (what, "gradient at a row that is no site")
    err, bound = np.abs(grad.astype(np.float64) - ref["grad"]).max(axis=-1), grad_bound(ref)
    assert not err[bound == 0].any(), (what, "gradient where nothing may move", np.argwhere((bound == 0) & (err > 0))[:4])
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f"{what}: grad, largest |error| / bound = {ratio:.4f}; rows with a tie allowance {int((ref['tie'] > 0).sum())} of {int(ref['site'].sum())} sites")
    assert (err <= bound).all(), (what, "grad", np.argwhere(err > bound)[:4], ratio)
    return ratio


def tie_share(ref):
    """the share of the site rows with a non-zero tie allowance"""
    return float((ref["tie"] > 0).sum()) / max(int(ref["site"].sum()), 1)


# ---- the inputs the CPU and the GPU tests share -----------------------------------------------------------------------------------

def lattice(lens, L, A, slot, seed, behind="nan"):
    """integer-lattice chains [n, L, A, 3], pred = true + a small integer step (exact ties only: delta is 0 or far from it): ~10 % of
    the sites cleared in mask_true only and ~10 % in mask_pred only (NaN patterns under every cleared mask); per chain of 16 rows or
    more a NaN / +inf coordinate in true, a -inf / NaN one in pred, two sites at +-3e19 in pred only (pairs with d_pred = +inf: eps 0,
    no gradient), two in true (d_true = +inf: no pair) and three predicted points on top of one another (d_pred == 0); NaN patterns in
    every row behind the length"""
    rng = np.random.default_rng(seed)
    n = len(lens)
    true = rng.integers(-6, 7, size=(n, L, A, 3)).astype(F)
    pred = true + rng.integers(-2, 3, size=(n, L, A, 3)).astype(F)
    mt, mp = np.ones((n, L, A), np.uint8), np.ones((n, L, A), np.uint8)
    u = rng.random((n, L))
    mt[..., slot][u < 0.10] = 0
    mp[..., slot][(u >= 0.10) & (u < 0.20)] = 0
    for e, m in enumerate(lens):
        if m >= 16:
            r = rng.choice(m, size=11, replace=False)
            true[e, r[0], slot, 0] = np.nan; true[e, r[1], slot, 1] = np.inf; pred[e, r[2], slot, 2] = -np.inf; pred[e, r[3], slot, 0] = np.nan
            pred[e, r[4], slot, 0] = 3e19; pred[e, r[5], slot, 1] = -3e19
            true[e, r[6], slot, 0] = 3e19; true[e, r[7], slot, 2] = -3e19
            pred[e, r[9], slot] = pred[e, r[8], slot]; pred[e, r[10], slot] = pred[e, r[8], slot]
            true[e, r[9], slot] = true[e, r[8], slot] + F(1)                                 # (near one another in the truth: pairs)
            mt[e, r, slot] = 1; mp[e, r, slot] = 1
        if behind == "nan":
            true[e, m:] = np.nan; pred[e, m:] = np.nan
    true.view(np.uint32)[mt == 0] = NAN_BITS
    pred.view(np.uint32)[mp == 0] = NAN_BITS
    return true, mt, pred, mp


def walk(lens, L, A, slot, seed, sigma=0.5):
    """noisy chains [n, L, A, 3]: at `slot` true is a random walk of 3.8 A steps and pred = true + N(0, sigma) in float32, the other
    slots hold other numbers; ~5 % of the sites cleared in mask_true; rows behind the length hold NaN -> true, mask_true, pred"""
    rng = np.random.default_rng(seed)
    n = len(lens)
    true = (rng.standard_normal((n, L, A, 3)) * 30).astype(F)
    step = rng.standard_normal((n, L, 3))
    step *= 3.8 / np.linalg.norm(step, axis=-1, keepdims=True)
    true[:, :, slot] = np.cumsum(step, axis=1).astype(F)
    pred = (true + (rng.standard_normal(true.shape) * sigma).astype(F)).astype(F)
    mt = np.ones((n, L, A), np.uint8)
    mt[..., slot][rng.random((n, L)) < 0.05] = 0
    for e, m in enumerate(lens):
        true[e, m:] = np.nan; pred[e, m:] = np.nan
    return true, mt, pred


def weights(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(F)


SYNTH_SEED, WALK_LENS, WALK_SEED = 11, (65, 257, 350), 23


def synthetic_lens(P):
    """the lengths of the lattice batch: the tile edges, one row, no pair, and more than one pass of P rows"""
    return [0, 1, 2, 63, 64, 65, 255, 256, 257, 2 * P + 3]


def synthetic_batch(P):
    """the lattice batch of the GPU tests on backbone4 / CA with its weights -> dict(lens, L, arrays, w)"""
    lens = synthetic_lens(P)
    L = max(lens)
    return dict(lens=np.asarray(lens, np.uint32), L=L, arrays=lattice(lens, L, 4, 1, SYNTH_SEED), w=weights((len(lens), L), SYNTH_SEED + 1))


def walk_batch():
    """the noisy batch of the GPU tests on atom14 / CB (slot 4) with its weights -> dict(lens, L, arrays (true, mask_true, pred), w)"""
    L = max(WALK_LENS)
    return dict(lens=np.asarray(WALK_LENS, np.uint32), L=L, arrays=walk(WALK_LENS, L, 14, 4, WALK_SEED), w=weights((len(WALK_LENS), L), WALK_SEED + 1))


# ---- the device calls -------------------------------------------------------------------------------------------------------------

def _th(thresholds):
    if thresholds is None:
        return None, None
    a = np.asarray(thresholds, F)
    return a, a.ctypes.data


def value_spec(shape):
    return dict(soft=(F, tuple(shape)), pairs=(np.int32, tuple(shape)))


def grad_spec(shape):
    return dict(grad=(F, tuple(shape) + (3,)))


def run_value(codec, pt, mt, pp, mp, bound_t, n, rows, layout, slot, packed, cutoff=15.0, thresholds=None, guard=GUARD, expect=0):
    """fcz_lddt_soft_dev (rows = L) or fcz_lddt_soft_packed_dev (rows = R) on device tensors -> (soft, pairs) as numpy, guards checked"""
    import torch
    g = DevGuarded(value_spec((rows,) if packed else (n, rows)), guard)
    fn = codec.lib.fcz_lddt_soft_packed_dev if packed else codec.lib.fcz_lddt_soft_dev
    keep, th = _th(thresholds)
    torch.cuda.synchronize()
    rc = fn(codec.ctx, pt.data_ptr(), mt.data_ptr(), pp.data_ptr(), ptr(mp), ptr(bound_t), n, rows, layout, slot, cutoff, th, *g.ptrs())
    codec.synchronize()
    assert rc == expect, rc
    return g.all()


def run_grad(codec, pt, mt, pp, mp, bound_t, n, rows, layout, slot, packed, w, cutoff=15.0, thresholds=None, guard=GUARD, expect=0):
    """fcz_lddt_soft_grad_dev or fcz_lddt_soft_grad_packed_dev on device tensors, w a device tensor -> grad as numpy, guards checked"""
    import torch
    g = DevGuarded(grad_spec((rows,) if packed else (n, rows)), guard)
    fn = codec.lib.fcz_lddt_soft_grad_packed_dev if packed else codec.lib.fcz_lddt_soft_grad_dev
    keep, th = _th(thresholds)
    torch.cuda.synchronize()
    rc = fn(codec.ctx, pt.data_ptr(), mt.data_ptr(), pp.data_ptr(), ptr(mp), ptr(bound_t), n, rows, layout, slot, cutoff, th, w.data_ptr(), *g.ptrs())
    codec.synchronize()
    assert rc == expect, rc
    return g.all()[0]
