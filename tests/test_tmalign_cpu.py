"""CPU: the definition of the TM-align-style alignment (include/fcz_hip.h, fcz_tmalign_dev) as tests/_tmalign.py restates it in numpy
-- the seed schedule against the library's host helpers, the dynamic programme on a hand-computed matrix and on random ones, what the
search must recover on planted alignments -- the argument rules of foldcomp.tm_align, the refusals of the C-ABI that need no device,
and the conditions under which the float64 reference is a fair judge of the GPU test's seeded batch."""
import ctypes

import numpy as np
import pytest

import _superpose as SP
import _tmalign as TA
from foldcomp_amd import _lib, api
from foldcomp_amd.structure import CChainSet, CTmAlignOut, CTmAlignParams


def _what(lib, sa, sb, fragments, seed):
    kind, shift = ctypes.c_int32(), ctypes.c_int32()
    ia, ib, n = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    rc = lib.fcz_tmalign_seed(sa, sb, fragments, seed, ctypes.byref(kind), ctypes.byref(shift), ctypes.byref(ia), ctypes.byref(ib), ctypes.byref(n))
    return rc, (kind.value, shift.value, ia.value, ib.value, n.value)


def test_seed_schedule_against_the_host_helpers():
    lib = _lib.load()
    sizes = [(a, b) for a in range(71) for b in range(71)] + [(350, 350), (129, 1024), (1024, 1024), (1024, 7), (161, 159)]
    for sa, sb in sizes:
        for fragments in (0, 1):
            ref = TA.seed_list(sa, sb, bool(fragments))
            assert lib.fcz_tmalign_seeds(sa, sb, fragments) == len(ref), (sa, sb, fragments)
            if fragments:
                for s, want in enumerate(ref):
                    assert _what(lib, sa, sb, 1, s) == (0, want), (sa, sb, s)
                assert _what(lib, sa, sb, 1, len(ref))[0] == -1
    # the schedule itself: the gapless shifts ascend and keep the overlap, one DP seed follows, the fragments tile both chains
    ref = TA.seed_list(350, 300)
    shifts = [s for s in ref if s[0] == 0]
    assert [s[1] for s in shifts] == list(range(150 - 350, 300 - 150 + 1)) and min(s[4] for s in shifts) == 150 and ref[len(shifts)][0] == 1
    frags = [s for s in ref if s[0] == 2]
    assert TA.frag_len(300) == 32 and len(frags) == 11 * 10 and frags[0][2:] == (0, 0, 32) and frags[-1][2:] == (318, 268, 32) and frags[1][2:] == (0, 32, 32)
    assert TA.frag_len(3) == 3 and TA.frag_len(20) == 8 and TA.frag_len(100) == 20 and TA.min_overlap(3) == 3 and TA.min_overlap(8) == 5
    assert TA.seed_list(0, 9) == [] and lib.fcz_tmalign_seeds(0, 9, 1) == 0
    kind = ctypes.c_int32()
    assert lib.fcz_tmalign_seed(5, 5, 1, 0, None, None, None, None, None) == -1 and lib.fcz_tmalign_seed(0, 5, 1, 0, ctypes.byref(kind), None, None, None, None) == -1


def test_hand_computed_dp():
    """3 x 4, a gap of 2 units, worked by hand:
        q = 3 8  0 0      H = 0 0 0  0  0
            0 3  0 0          0 3 8  6  4
            0 0 20 0          0 1 6  8  6
                              0 0 4 26 24
    The last column holds 0, 4, 6, 24 and the last row in front of it 0, 0, 4, 26: the end cell is H[3][3], so b's last site hangs over
    the end for free. H[2][2] = 6 both by the diagonal (3 + 3) and from above (8 - 2): the diagonal is preferred and the alignment is
    0, 1, 2. From above the path would reach H[1][2] = 0 + 8 and the alignment would be 1, -, 2."""
    q = np.asarray([[3, 8, 0, 0], [0, 3, 0, 0], [0, 0, 20, 0]], np.int64)
    G = 2
    H = TA.dp_cells(q, G)
    assert H.tolist() == [[0, 0, 0, 0, 0], [0, 3, 8, 6, 4], [0, 1, 6, 8, 6], [0, 0, 4, 26, 24]]
    assert np.array_equal(TA.dp_rows(q, G), H)
    assert H[1, 1] + q[1, 1] == H[1, 2] - G == H[2, 2]
    dec = []
    assert TA.traceback(H, q, G, dec).tolist() == [0, 1, 2] and dec == [20, 0, 5]   # (the lead of every step taken: the tie is won by 0)
    # up against left on equal values: up is preferred. q = 4 0 / 0 0 without a gap penalty: H = 4 everywhere inside; the end cell is
    # the first maximum of the last column, H[1][2], reached from the left, so a's first site takes b's first
    q = np.asarray([[4, 0], [0, 0]], np.int64)
    H = TA.dp_cells(q, 0)
    assert H.tolist() == [[0, 0, 0], [0, 4, 4], [0, 4, 4]] and TA.traceback(H, q, 0).tolist() == [0, -1]
    # all q = 0 and a gap that costs: H = 0, the end cell is H[0][Sb], nothing is aligned
    z = np.zeros((3, 4), np.int64)
    assert not TA.dp_cells(z, 5).any() and TA.traceback(TA.dp_cells(z, 5), z, 5).tolist() == [-1, -1, -1]
    assert TA.gap_units(0.6) == 39322 and TA.gap_units(0.0) == 0


def test_cells_and_rows_agree_on_random_matrices():
    rng = np.random.default_rng(3)
    for _ in range(200):
        q = rng.integers(0, TA.Q + 1, (int(rng.integers(1, 12)), int(rng.integers(1, 12))))
        if rng.random() < 0.3:
            q //= 20000                                                        # few distinct values: many ties
        G = int(rng.choice([0, 1, 2, 39322, TA.Q]))
        H = TA.dp_cells(q, G)
        assert np.array_equal(TA.dp_rows(q, G), H)
        aln = TA.traceback(H, q, G)
        on = aln[aln >= 0]
        assert (np.diff(on) > 0).all()                                         # monotone


def test_rigidly_moved_copy_gives_the_identity_map():
    rng = np.random.default_rng(7)
    for m in (3, 17, 80):
        a = SP.walk_chain(rng, m).astype(np.float32).astype(np.float64)
        b = a @ SP.random_rotation(rng).T + rng.uniform(-30, 30, 3)
        r = TA.align_sites(a, b)
        assert r["aln"].tolist() == list(range(m)) and abs(r["tm"] - 1.0) <= 1e-12 and abs(r["tm_a"] - 1.0) <= 1e-12 and r["aligned"] == m
        assert np.abs(a @ r["rot"].T + r["trans"] - b).max() < 1e-9


CUT_SEED, CUT_LEN, CUT_AT, CUT_NOISE = 21, 120, 50, 0.3


def planted_with_a_cut():
    """a chain of CUT_LEN residues against itself with 12 residues cut out behind CUT_AT, moved, plus noise -> (a, b, the planted map)"""
    rng = np.random.default_rng(CUT_SEED)
    a = SP.walk_chain(rng, CUT_LEN)
    keep = np.r_[0:CUT_AT, CUT_AT + 12:CUT_LEN]
    b = a[keep] @ SP.random_rotation(rng).T + rng.uniform(-30, 30, 3) + CUT_NOISE * rng.standard_normal((len(keep), 3))
    planted = np.full(CUT_LEN, -1)
    planted[keep] = np.arange(len(keep))
    return a, b, planted


def test_a_cut_out_of_the_middle_is_recovered():
    """the reference alone recovers every planted pair further than 2 residues from the cut"""
    a, b, planted = planted_with_a_cut()
    r = TA.align_sites(a, b)
    far = (planted >= 0) & ((np.arange(CUT_LEN) < CUT_AT - 2) | (np.arange(CUT_LEN) >= CUT_AT + 12 + 2))
    assert np.array_equal(r["aln"][far], planted[far])
    recovered = (r["aln"][planted >= 0] == planted[planted >= 0]).mean()
    print(f"planted pairs recovered: {recovered:.4f} of {int((planted >= 0).sum())}, tm {r['tm']:.4f}, aligned {r['aligned']}")
    assert r["tm"] > 0.9 and r["seed"] >= len([s for s in TA.seed_list(len(a), len(b)) if s[0] == 0])   # no gapless shift spans the cut


def test_gapless_only_is_never_below_the_kabsch_fit():
    rng = np.random.default_rng(9)
    for m in (4, 30, 77):
        a = SP.walk_chain(rng, m)
        b = a @ SP.random_rotation(rng).T + 1.5 * rng.standard_normal((m, 3))
        r = TA.align_sites(a, b, fragments=False, dp_rounds=0)
        kab = SP.superpose_chain(b.astype(np.float32), a.astype(np.float32), np.ones(m, bool))
        r32 = TA.align_sites(a.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64), fragments=False, dp_rounds=0)
        assert r32["tm"] >= kab["tm"] - 1e-15 and r["tm"] > 0 and r32["seed"] < 2 * m


def test_status_and_empty_results():
    ca, cb, _ = TA.align_batch()
    sa, kb = TA.padded_set(ca), TA.packed_set(cb)
    pairs = np.asarray([(9, 9), (9, 3), (-1, 0), (0, len(cb)), (10, 0)], np.int32)
    out = TA.align_sets(sa, kb, pairs, sa["pos"].shape[1], 64, 1, fragments=False, dp_rounds=1)
    assert out["status"].tolist() == [1, 0, 2, 2, 0] and out["sites_b"][0] == 0 and out["aligned"][1] >= 3
    for e in (0, 2, 3, 4):
        assert np.array_equal(out["rot"][e], np.eye(3)) and (out["map"][e] == -1).all() and out["tm"][e] == 0 and out["aligned"][e] == 0


def test_check_tm_align():
    ok = ((4, 50, 37, 3), (200, 37, 3), 50, 120)
    assert api.check_tm_align("CA", *ok) == (1, 1, 4, 20, (0.6, 0.0), 20, 0)
    assert api.check_tm_align(0, *ok, (7, 2), False, 0, 64, [1], 0, 3, ((7, 3, 3), (7, 3))) == (0, 0, 0, 64, (1.0,), 0, 3)
    assert api.check_tm_align("CB", (4, 50, 14, 3), (9, 14, 3), None, None)[0] == 4
    for bad in (dict(shape_b=(200, 14, 3)), dict(shape_a=(4, 50, 37)), dict(wa=1025), dict(wb=2000), dict(pairs_shape=(7, 3)), dict(pairs_shape=(7,)),
                dict(fragments=1), dict(refine=-1), dict(refine=65), dict(refine=2.0), dict(dp_rounds=True), dict(dp_rounds=65), dict(gaps=()),
                dict(gaps=(0.1,) * 5), dict(gaps=(-0.5,)), dict(gaps=(16.5,)), dict(gaps=(float("nan"),)), dict(gaps=("a",)), dict(iterations=65),
                dict(levels=0), dict(atom="CG"), dict(atom=37), dict(transform=((7, 3, 3), (6, 3))), dict(transform=((7, 3), (7, 3))),
                dict(pairs_shape=(8, 2), transform=((7, 3, 3), (7, 3)))):
        kw = dict(atom="CA", shape_a=ok[0], shape_b=ok[1], wa=50, wb=120)
        kw.update(bad)
        with pytest.raises(ValueError):
            api.check_tm_align(**kw)
    with pytest.raises(ValueError):
        api.check_tm_align("CB", (4, 50, 4, 3), (4, 50, 4, 3), 50, 50)          # backbone4 has no CB
    assert api.tm_align_pairs(3, 3, True).tolist() == [[0, 1], [0, 2], [1, 2]] and api.tm_align_pairs(2, 2, False).tolist() == [[0, 0], [0, 1], [1, 0], [1, 1]]
    assert api.tm_align_pairs(1, 0, True).shape == (0, 2) and api.tm_align_pairs(1, 0, True).dtype == np.int32


def test_abi_refuses_without_a_device():
    """the entry points refuse a NULL ctx before anything else: no CPU path stands behind them"""
    lib = _lib.load()
    pos, mask = np.zeros((1, 8, 4, 3), np.float32), np.ones((1, 8, 4), np.uint8)
    s = CChainSet(pos.ctypes.data, mask.ctypes.data, None, None, 1, 8)
    pairs, rot, trans = np.zeros((1, 2), np.int32), np.zeros((1, 3, 3), np.float32), np.zeros((1, 3), np.float32)
    mp, al = np.full((1, 8), 7, np.int32), np.full(1, 7, np.int32)
    par = CTmAlignParams(1, 4, 20, 2, (ctypes.c_double * 4)(0.6, 0.0), 0, 20)
    out = CTmAlignOut(rot.ctypes.data, trans.ctypes.data, *([None] * 11))
    for fn in (lib.fcz_tmalign_dev, lib.fcz_tmalign):
        assert fn(None, ctypes.byref(s), ctypes.byref(s), pairs.ctypes.data, 1, 8, 8, 2, 1, ctypes.byref(par), ctypes.byref(out)) == -1
    for fn in (lib.fcz_tmalign_dp_dev, lib.fcz_tmalign_dp):
        assert fn(None, ctypes.byref(s), ctypes.byref(s), pairs.ctypes.data, 1, 8, 8, 2, 1, rot.ctypes.data, trans.ctypes.data, 0.6, mp.ctypes.data, al.ctypes.data) == -1
    assert (mp == 7).all() and (al == 7).all() and not rot.any()
    assert "fcz_tmalign_dev" in _lib.EXPORTS and "fcz_tmalign_dp_dev" in _lib.EXPORTS and "fcz_tmalign_seeds" in _lib.EXPORTS


# The generator seed of the GPU test's batch and what the reference finds for it are written beside _tmalign.ALIGN_SEED; FOUND restates
# the smallest figures so that a change of the batch shows here.
FOUND = dict(margin=3.65e-5, gap=1.45e-3, lead=1.76e-5, round_lead=4.48e-7)


def test_the_reference_is_a_fair_judge_of_the_seeded_batch():
    """for EVERY pair of the batch: section 6.14's three conditions for every fit -- no deviation within 1e-8 A of a cut in any
    selection step, every round within 1e-9 of a fit's best (and every (seed, round) of the final search within 1e-9 of the best of
    that search and the winning candidate) shares the winner's selection, Horn gap >= 1e-3 for every fit on three or more pairs --,
    every DP without a score within 1e-7 of an integer or without a traceback decision won by 2 units or less, and every candidate
    with another alignment either 1e-9 behind the winner or tied with it EXACTLY from a higher seed (one and two sites: several shifts
    fit without error, tm is the same double on both sides, and both sides keep the lowest seed)"""
    _, traces = TA.align_batch_reference()
    worst = [np.inf] * 4
    for e, tr in enumerate(traces):
        margin, gap, dps_ok, lead, shared, round_lead, exact_ties = TA.fairness(tr)
        assert margin >= 1e-8 and shared and gap >= 1e-3 and dps_ok and exact_ties, (e, margin, shared, gap, dps_ok, lead, exact_ties)
        assert lead >= 1e-9                                                    # (by construction: what trails by less is an exact tie, above)
        worst = [min(w, v) for w, v in zip(worst, (margin, gap, lead, round_lead))]
    print("seeded batch: smallest margin, Horn gap, candidate lead, round lead", worst)
    for got, key in zip(worst, ("margin", "gap", "lead", "round_lead")):
        assert abs(got / FOUND[key] - 1) < 0.01, (key, got)
