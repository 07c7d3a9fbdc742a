"""CPU: the parts of the lDDT feature that need no device -- the numpy restatement (tests/_lddt.py) against a brute force over Python
integers on an integer lattice and against the dense AlphaFold-style formulation in float64, the cutoff's rounding boundary
(fcz_lddt_c2), the pure-host ABI (fcz_lddt_pass, the refusals, the export list), and the argument errors of foldcomp.lddt, raised
before torch or a device is touched."""
import ctypes
import math

import numpy as np
import pytest

import _knn as K
import _lddt as Q
from foldcomp_amd import _lib, api, tensors

NEW = ("fcz_lddt_pass", "fcz_lddt_dev", "fcz_lddt_packed_dev", "fcz_lddt", "fcz_lddt_packed")
F = np.float32


def _brute(tp, pp, site, cutoff, thresholds=Q.THRESHOLDS):
    """tp, pp: lists of integer triples; exact integer d2, its root rounded to float32 (d2 < 2^24: the double root rounds to the float
    root), float32 subtraction and compares"""
    m = len(tp)
    pairs, hits = np.zeros(m, np.int32), np.zeros(m, np.int32)
    for i in range(m):
        if not site[i]:
            continue
        for j in range(m):
            if j == i or not site[j]:
                continue
            dt = F(math.sqrt(sum((a - b) ** 2 for a, b in zip(tp[j], tp[i]))))
            if not dt < F(cutoff):
                continue
            dp = F(math.sqrt(sum((a - b) ** 2 for a, b in zip(pp[j], pp[i]))))
            diff = abs(F(dt - dp))
            pairs[i] += 1
            hits[i] += sum(1 for v in thresholds if diff < F(v))
    return Q.score_of(pairs, hits), pairs, hits


def _lattice(m, seed, span=4):
    """m integer points in -span .. span (true), pred = true + a small integer step, some duplicated; ~10 % cleared in each mask"""
    rng = np.random.default_rng(seed)
    t = rng.integers(-span, span + 1, size=(m, 3))
    if m > 12:
        t[10] = t[3]; t[11] = t[3]; t[m - 1] = t[m - 2]            # duplicated points: d_true = 0 is a pair
    p = t + rng.integers(-2, 3, size=(m, 3))
    site_t, site_p = rng.random(m) > 0.1, rng.random(m) > 0.1
    if m > 12:
        site_t[[3, 10, 11]] = True; site_p[[3, 10, 11]] = True
    return t, p, site_t & site_p, (site_t, site_p)


@pytest.mark.parametrize("m", list(range(0, 10)) + [90])
def test_restatement_on_an_integer_lattice(m):
    t, p, site, (st, sp) = _lattice(m, 5 + m)
    cutoff = 5.0
    got = Q.lddt_chain(t.astype(F), p.astype(F), site, cutoff)
    exp = _brute([tuple(int(v) for v in x) for x in t], [tuple(int(v) for v in x) for x in p], site, cutoff)
    Q.same(got, exp, f"m={m}")
    assert not got[1][~site].any() and not got[2][~site].any() and not got[0][~site].any()
    if m == 90:
        assert (~st & sp).any() and (st & ~sp).any() and got[1][3] >= 2 and 0 < got[2].sum() < 4 * got[1].sum()
        # the same through the masks of the padded form
        pos_t, pos_p = np.zeros((1, m, 4, 3), F), np.zeros((1, m, 4, 3), F)
        pos_t[0, :, 1], pos_p[0, :, 1] = t, p
        mt, mp = np.zeros((1, m, 4), np.uint8), np.zeros((1, m, 4), np.uint8)
        mt[0, :, 1], mp[0, :, 1] = st, sp
        Q.same([a[0] for a in Q.lddt_padded(pos_t, mt, pos_p, mp, None, 1, cutoff)], exp, "masks")


@pytest.mark.parametrize("seed", [21, 22, 23])
def test_restatement_against_the_dense_float64_formulation(seed):
    rng = np.random.default_rng(seed)
    m = 200
    t = rng.integers(-8, 9, (m, 3))
    p = t + rng.integers(-2, 3, (m, 3))
    # the AlphaFold lddt() in float64, without its epsilon under the root (which would break the exact ties below)
    dmat_true = np.sqrt(((t[:, None, :] - t[None, :, :]).astype(np.float64) ** 2).sum(axis=-1))
    dmat_pred = np.sqrt(((p[:, None, :] - p[None, :, :]).astype(np.float64) ** 2).sum(axis=-1))
    to_score = (dmat_true < 15.0) * (1.0 - np.eye(m))
    l1 = np.abs(dmat_true - dmat_pred)
    hits = sum(((l1 < v) * to_score).sum(axis=-1) for v in Q.THRESHOLDS)
    pairs = to_score.sum(axis=-1)
    # what makes float64 a valid judge of the float32 definition: nothing lies near a boundary without lying on it
    inc = to_score > 0
    gaps = np.concatenate([np.abs(l1[inc] - v) for v in Q.THRESHOLDS])
    cut = np.abs(dmat_true - 15.0)
    print(f"seed {seed}: smallest non-zero threshold gap {gaps[gaps > 0].min():.3g}, cutoff gap {cut[cut > 0].min():.3g}, exact ties {int((gaps == 0).sum())}")
    assert gaps[gaps > 0].min() > 1e-5 and cut[cut > 0].min() > 1e-5
    assert (gaps == 0).sum() > 0                                     # exact ties exist: the strict < is exercised
    got = Q.lddt_chain(t.astype(F), p.astype(F), np.ones(m, bool))
    assert np.array_equal(got[1], pairs.astype(np.int32)) and np.array_equal(got[2], hits.astype(np.int32))
    assert (pairs < m - 1).any() and (pairs > 0).all()


def test_a_structure_against_itself_scores_one():
    rng = np.random.default_rng(31)
    x = (rng.normal(size=(300, 3)) * 12).astype(F)
    site = rng.random(300) > 0.1
    score, pairs, hits = Q.lddt_chain(x, x.copy(), site)
    assert np.array_equal(hits, 4 * pairs) and (pairs[site] > 0).sum() > 200 and (pairs[site] < site.sum() - 1).any() and not pairs[~site].any()
    assert np.array_equal(K.bits(score[pairs > 0]), np.full((pairs > 0).sum(), K.bits(np.ones(1, F))[0]))
    assert not score[pairs == 0].any()


def _boundary_cutoffs(q):
    c = F(math.sqrt(q))
    return [c, np.nextafter(c, F(np.inf)), np.nextafter(c, F(0))]


@pytest.mark.parametrize("q", [50, 99, 170])
def test_cutoffs_at_the_rounding_boundary(q):
    lib = _lib.load()
    assert int(math.isqrt(q)) ** 2 != q
    t, p, site, _ = _lattice(90, 40, span=8)                        # d2 up to 768
    tp, pp = [tuple(int(v) for v in x) for x in t], [tuple(int(v) for v in x) for x in p]
    d2 = ((t[:, None] - t[None]) ** 2).sum(-1)
    on = int(((d2 == q) & site[:, None] & site[None]).sum())
    assert on > 0, "no pair at d2 == q on this lattice"
    counts = []
    for c in _boundary_cutoffs(q):
        c2 = F(lib.fcz_lddt_c2(float(c)))
        # the bound the kernel compares d2 with: the smallest float32 whose rounded root reaches the cutoff
        assert np.sqrt(c2) >= c and np.sqrt(np.nextafter(c2, F(0))) < c
        assert (F(q) < c2) == bool(np.sqrt(F(q)) < c)
        got = Q.lddt_chain(t.astype(F), p.astype(F), site, c)
        Q.same(got, _brute(tp, pp, site, c), f"q={q} cutoff={c!r}")
        assert np.array_equal(got[1], ((d2.astype(F) < c2) & site[:, None] & site[None] & ~np.eye(90, dtype=bool)).sum(1) * site)
        counts.append(int(got[1].sum()))
    # sqrt(q) rounded is the distance of the d2 == q pairs: excluded at c and below it, included one ulp above
    assert counts[1] - counts[0] == on and counts[0] == counts[2]


def test_c2_extremes():
    lib = _lib.load()
    assert np.isnan(lib.fcz_lddt_c2(0.0)) and np.isnan(lib.fcz_lddt_c2(-1.0)) and np.isnan(lib.fcz_lddt_c2(float("nan"))) and np.isnan(lib.fcz_lddt_c2(float("inf")))
    assert lib.fcz_lddt_c2(3e38) == float("inf") and lib.fcz_lddt_c2(15.0) == 225.0
    tiny = lib.fcz_lddt_c2(1e-30)
    assert tiny > 0 and np.sqrt(F(tiny)) >= F(1e-30) and np.sqrt(np.nextafter(F(tiny), F(0))) < F(1e-30)


def test_restatement_forms_agree():
    rng = np.random.default_rng(6)
    lens = [0, 1, 2, 5, 30]
    L, A = 32, 4
    pos = rng.integers(-3, 4, size=(len(lens), L, A, 3)).astype(F)
    pred = pos + rng.integers(-1, 2, size=pos.shape).astype(F)
    mask = (rng.random((len(lens), L, A)) > 0.1).astype(np.uint8)
    pmask = (rng.random((len(lens), L, A)) > 0.1).astype(np.uint8)
    pad = Q.lddt_padded(pos, mask, pred, pmask, np.asarray(lens), 1, 4.0)
    row_off = np.concatenate([[0], np.cumsum(lens)])
    cat = lambda a: np.concatenate([a[e, :n] for e, n in enumerate(lens)])
    pk = Q.lddt_packed(cat(pos), cat(mask), cat(pred), cat(pmask), row_off, 1, 4.0)
    Q.same(pk, [cat(a) for a in pad], "packed")
    for a in pad:
        for e, n in enumerate(lens):
            assert not a[e, n:].any()
    assert not pad[1][0].any() and not pad[1][1].any() and pad[1][4].any()       # no row, and one row: no pair
    assert Q.lddt_padded(pos, mask, pred, None, np.asarray(lens), 1, 4.0)[1].sum() > pad[1].sum()


def test_pure_host_abi():
    lib = _lib.load()
    assert set(NEW) <= set(_lib.EXPORTS)
    assert lib.fcz_lddt_pass() > 0
    buf = np.zeros(256, np.uint8)
    p = buf.ctypes.data
    th = np.asarray(Q.THRESHOLDS, F)
    for fn in (lib.fcz_lddt_dev, lib.fcz_lddt_packed_dev, lib.fcz_lddt, lib.fcz_lddt_packed):
        assert fn(None, p, p, p, p, p, 1, 4, 0, 1, 15.0, th.ctypes.data, p, p, p) == -1
    # refused before anything is touched (the ctx is never read)
    fake = ctypes.c_void_p(buf.ctypes.data)
    bad_th = np.asarray([0.5, np.nan, 2, 4], F)
    for fn in (lib.fcz_lddt_dev, lib.fcz_lddt_packed_dev, lib.fcz_lddt, lib.fcz_lddt_packed):
        for cutoff in (0.0, -1.0, float("nan"), float("inf")):
            assert fn(fake, p, p, p, p, p, 1, 4, 0, 1, cutoff, None, p, p, p) == -1
        assert fn(fake, p, p, p, p, p, 1, 4, 0, 1, 15.0, bad_th.ctypes.data, p, p, p) == -1
        assert fn(fake, p, p, p, p, p, 1, 2 ** 29 + 1, 0, 1, 15.0, None, p, p, p) == -1
        assert fn(fake, p, p, p, p, p, 1, 4, 0, 37, 15.0, None, p, p, p) == -1 and fn(fake, p, p, p, p, p, 1, 4, 3, 1, 15.0, None, p, p, p) == -1
        assert fn(fake, p, p, None, p, p, 1, 4, 0, 1, 15.0, None, p, p, p) == -1 and fn(fake, p, p, p, p, p, 1, 4, 0, 1, 15.0, None, p, p, None) == -1
    assert lib.fcz_lddt_dev(fake, p, p, p, p, p, 1, 0, 0, 1, 15.0, None, p, p, p) == -1            # L == 0
    assert lib.fcz_lddt_packed_dev(fake, p, p, p, p, None, 1, 4, 0, 1, 15.0, None, p, p, p) == -1  # chains without a row_off
    assert not buf.any()


def test_lddt_argument_errors_need_no_device():
    pos37, mask37 = np.zeros((2, 8, 37, 3), F), np.zeros((2, 8, 37), np.uint8)
    pos4, mask4 = np.zeros((2, 8, 4, 3), F), np.zeros((2, 8, 4), np.uint8)
    true37, true4 = dict(pos=pos37, mask=mask37), dict(pos=pos4, mask=mask4)
    for pred, true, kw in ((pos37, true37, dict(cutoff=0)), (pos37, true37, dict(cutoff=-1.0)), (pos37, true37, dict(cutoff=float("nan"))),
                           (pos37, true37, dict(cutoff=float("inf"))), (pos37, true37, dict(cutoff="15")), (pos37, true37, dict(cutoff=1e39)),
                           (pos37, true37, dict(thresholds=(0.5, 1, 2))), (pos37, true37, dict(thresholds=(0.5, 1, 2, float("nan")))),
                           (pos37, true37, dict(thresholds=(0.5, 1, 2, "4"))), (pos37, true37, dict(thresholds=4.0)),
                           (pos37, true37, dict(atom="XX")), (pos4, true4, dict(atom="CB")), (pos37, true37, dict(atom=37)),
                           (pos4, true4, dict(atom=4)), (pos37, true37, dict(atom=-1)), (pos37[:, :7], true37, {}), (pos4, true37, {}),
                           (dict(pos=pos37, mask=mask37[:1]), true37, {}), (dict(pos=pos37[:1], mask=mask37), true37, {})):
        with pytest.raises(ValueError):
            tensors.lddt(pred, true, **kw)
    with pytest.raises(TypeError):
        tensors.lddt(pos37, dict(pos=pos37))
    with pytest.raises(TypeError):
        tensors.lddt(dict(mask=mask37), true37)
    assert api.check_lddt(15, None, "CA", 37) == (1, 15.0, (0.5, 1.0, 2.0, 4.0)) and api.check_lddt(6.5, (1, 1, 2, 4), "CB", 14)[0] == 4
    assert api.check_lddt(np.float32(0.1), (0.25, 0.5, 1, np.inf), 2)[1:] == (float(F(0.1)), (0.25, 0.5, 1.0, float("inf")))
    import foldcomp
    import foldcomp_amd
    assert foldcomp.lddt is foldcomp_amd.lddt is tensors.lddt
