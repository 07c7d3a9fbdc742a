"""The maximised TM-score (include/fcz_hip.h, fcz_tmscore_dev) without a device: the seed schedule written out by hand, the numpy
reference of tests/_tmscore.py against a known rigid motion, against the Kabsch fit and on hinged chains, the padded and the packed
form, the conditions under which that reference may judge the kernel, the new ABI symbols' refusals and the argument errors of
foldcomp.tm_score."""
import ctypes

import numpy as np
import pytest

import _superpose as SP
import _tmscore as T
from foldcomp_amd import _lib, api, tensors
from foldcomp_amd.structure import CSuperposeOut, CTmScoreOut

F = np.float32
NEW = ("fcz_tmscore_seeds", "fcz_tmscore_seed_fragment", "fcz_tmscore_dev", "fcz_tmscore_packed_dev", "fcz_tmscore", "fcz_tmscore_packed")

# the schedule by hand: (start, length) of every seed, in the order of their numbers
BY_HAND = {
    0: [],
    1: [(0, 1)],
    2: [(0, 2)],
    3: [(0, 3)],
    4: [(0, 4)],
    5: [(0, 5), (0, 4), (1, 4)],
    6: [(0, 6), (0, 4), (2, 4)],
    7: [(0, 7), (0, 4), (2, 4), (3, 4)],
    8: [(0, 8), (0, 4), (2, 4), (4, 4)],
    9: [(0, 9), (0, 4), (2, 4), (4, 4), (5, 4)],
    10: [(0, 10), (0, 5), (2, 5), (4, 5), (5, 5), (0, 4), (2, 4), (4, 4), (6, 4)],
}
# S = 350: the lengths 350, 175, 87, 43, 21, 10, 5 and then 4, with steps 175, 87, 43, 21, 10, 5, 2, 2; the regular starts of each
# are 0 .. floor((350 - l) / step) * step, and the start 350 - l is one more wherever step does not divide 350 - l:
#   350: 1 | 175: 0, 87, 174 + 175 = 4 | 87: 0 .. 258 (7) + 263 = 8 | 43: 0 .. 294 (15) + 307 = 16 | 21: 0 .. 320 (33) + 329 = 34
#   10: 0 .. 340 (69), 340 is the last = 69 | 5: 0 .. 344 (173) + 345 = 174 | 4: 0 .. 346 (174), 346 is the last = 174
PER_LENGTH_350 = [(350, 1), (175, 4), (87, 8), (43, 16), (21, 34), (10, 69), (5, 174), (4, 174)]


def test_the_seed_schedule_by_hand():
    lib = _lib.load()
    for S, want in BY_HAND.items():
        assert T.seed_list(S) == want, S
        assert lib.fcz_tmscore_seeds(S, 0) == len(want), S
    seeds = T.seed_list(350)
    assert T.fragment_lengths(350) == [l for l, _ in PER_LENGTH_350]
    assert [sum(1 for _, l in seeds if l == k) for k, _ in PER_LENGTH_350] == [c for _, c in PER_LENGTH_350]
    assert len(seeds) == sum(c for _, c in PER_LENGTH_350) == 480 == lib.fcz_tmscore_seeds(350, 0)
    assert seeds[0] == (0, 350) and seeds[1:5] == [(0, 175), (87, 175), (174, 175), (175, 175)] and seeds[-1] == (346, 4)
    # levels keeps the first lengths only
    assert T.seed_list(350, 1) == [(0, 350)] and len(T.seed_list(350, 3)) == 13 and T.seed_list(350, 8) == T.seed_list(350, 9) == seeds
    for S in (1, 5, 10, 350, 1027):
        for levels in range(1, 12):
            assert lib.fcz_tmscore_seeds(S, levels) == len(T.seed_list(S, levels)), (S, levels)
    # every seed lies inside the chain, no two seeds of a chain are equal, and the library maps a seed's number to the same fragment
    start, length = ctypes.c_uint32(), ctypes.c_uint32()
    for S in list(range(0, 200)) + [255, 256, 257, 1027, 4099]:
        seeds = T.seed_list(S)
        assert lib.fcz_tmscore_seeds(S, 0) == len(seeds) == len(set(seeds)), S
        assert all(0 <= s and s + l <= S and l >= 1 for s, l in seeds), S
        for k, frag in enumerate(seeds):
            assert lib.fcz_tmscore_seed_fragment(S, 0, k, ctypes.byref(start), ctypes.byref(length)) == 0 and (start.value, length.value) == frag, (S, k)
        assert lib.fcz_tmscore_seed_fragment(S, 0, len(seeds), ctypes.byref(start), ctypes.byref(length)) == -1
    assert lib.fcz_tmscore_seed_fragment(350, 2, 4, ctypes.byref(start), ctypes.byref(length)) == 0 and (start.value, length.value) == (175, 175)
    assert lib.fcz_tmscore_seed_fragment(350, 2, 5, ctypes.byref(start), ctypes.byref(length)) == -1
    assert lib.fcz_tmscore_seed_fragment(350, 0, 0, None, ctypes.byref(length)) == -1


def test_the_scratch_bound_of_the_c_abi_holds():
    """the ctx keeps a double per seed in a buffer sized on the host from the rows alone: 1.7 S + 66 bounds the seeds of S sites"""
    lib = _lib.load()
    rng = np.random.default_rng(0)
    for S in list(range(0, 3000)) + [int(v) for v in rng.integers(3000, 2 ** 31 - 1, 300)] + [2 ** 31 - 1]:
        assert lib.fcz_tmscore_seeds(S, 0) <= (17 * S) // 10 + 66, S


def test_a_pure_rigid_motion_scores_one_on_seed_zero():
    rng = np.random.default_rng(3)
    for m in (3, 4, 5, 9, 64, 300):
        x = SP.walk_chain(rng, m).astype(F)
        y = (x.astype(np.float64) @ SP.random_rotation(rng).T + rng.uniform(-30, 30, 3))
        # (float64 prediction: the reference is not fed rounded coordinates here, so the fit is exact to rounding)
        c = T.search_chain(x.astype(np.float64), y, np.ones(m, bool))
        assert abs(c["tm"] - 1.0) < 1e-10 and c["seed"] == 0 and c["selected"] == m and c["rmsd"] < 1e-9, (m, c["tm"], c["seed"])


def test_never_below_the_kabsch_fit_and_the_gain_on_hinged_chains():
    lens, hinged, pos_t, mask, pos_p = T.tm_batch()
    ref, _ = T.tm_batch_reference()
    kab = SP.superpose_padded(pos_t, mask, pos_p, None, lens, 1)
    gain = ref["tm"] - kab["tm"]
    assert (gain >= 0).all(), gain.min()
    big = hinged & (lens >= 63)
    print("gains on the hinged chains of 63 residues and more:", np.round(np.sort(gain[big]), 3))
    assert big.sum() == 10 and (gain[big] > 0).all() and (gain[big] >= 0.05).sum() * 4 >= 3 * big.sum()
    assert np.array_equal(ref["sites"], lens) and (ref["selected"] <= ref["sites"]).all() and (ref["selected"][lens >= 3] >= 3).all()
    assert (ref["seed"][hinged & (lens >= 63)] > 0).any()


def test_one_level_and_no_iteration_is_the_kabsch_fit():
    lens, _, pos_t, mask, pos_p = T.tm_batch()
    keep = lens <= 257                                                        # (the long chains add nothing to this comparison)
    one = T.tm_padded(pos_t[keep], mask[keep], pos_p[keep], None, lens[keep], 1, iterations=0, levels=1)
    kab = SP.superpose_padded(pos_t[keep], mask[keep], pos_p[keep], None, lens[keep], 1)
    for k in SP.KEYS:
        assert np.array_equal(one[k], kab[k]), k
    assert not one["seed"].any() and np.array_equal(one["selected"], lens[keep])


def test_padded_against_packed_and_the_site_rules():
    rng = np.random.default_rng(6)
    lens = [0, 1, 2, 5, 30]
    L, A = 32, 4
    pos = rng.uniform(-20, 20, (len(lens), L, A, 3)).astype(F)
    pred = (pos + rng.standard_normal(pos.shape)).astype(F)
    mask = (rng.random((len(lens), L, A)) > 0.1).astype(np.uint8)
    pmask = (rng.random((len(lens), L, A)) > 0.1).astype(np.uint8)
    pos[4, 3, 1, 0] = np.nan; pred[4, 7, 1, 2] = np.inf; mask[4, [3, 7], 1] = 1; pmask[4, [3, 7], 1] = 1
    pad = T.tm_padded(pos, mask, pred, pmask, np.asarray(lens), 1)
    row_off = np.concatenate([[0], np.cumsum(lens)])
    pk = T.tm_packed(*SP.pack((pos, mask, pred, pmask), lens), row_off, 1)
    for k in T.KEYS:
        if k != "dev":
            assert np.array_equal(pad[k], pk[k]), k
    assert np.array_equal(SP.pack((pad["dev"],), lens)[0], pk["dev"])
    site = SP.site_of(pos, mask, pred, pmask, 1)
    assert not site[4, 3] and not site[4, 7] and pad["dev"][4, 3] == 0 and pad["dev"][4, 7] == 0
    assert pad["sites"][4] == site[4, :30].sum() < 30 and pad["sites"][0] == 0 and np.array_equal(pad["rot"][0], np.eye(3))
    assert pad["seed"][0] == 0 and pad["selected"][0] == 0 and pad["tm"][0] == 0
    # the fragments count SITES, not rows: the search of a chain equals the search of its sites alone
    js = np.flatnonzero(site[4, :30])
    alone = T.search_chain(pos[4, js, 1], pred[4, js, 1], np.ones(len(js), bool))
    assert alone["tm"] == pad["tm"][4] and alone["seed"] == pad["seed"][4] and alone["selected"] == pad["selected"][4]


def test_the_cut_grows_until_three_sites_lie_below_it():
    dev = np.asarray([0.2, 7.9, 9.1, 30.0])
    m = []
    assert T.select(dev, 3.5, 3, m).tolist() == [True, True, True, False] and len(m) == 13   # 3.5, 4.0, .. 9.5: the first cut above 9.1
    assert T.select(dev, 3.5, 1).tolist() == [True, False, False, False]
    assert T.select(np.asarray([1e6, 2e6, 3e6]), 3.5, 3).all()               # (CUT_STEPS steps do not reach them: the cut becomes +inf)
    assert T.d_search_of(10) == 4.5 and T.d_search_of(2000) == 8.0 and 4.5 < T.d_search_of(300) < 8.0


def test_the_gpu_tests_seeded_inputs_meet_its_conditions():
    """A float64 judge with another solver is fair to a search with thresholds only if, for EVERY chain of the GPU test's batch, (a) no
    deviation lies within 1e-8 A of a cut in any selection step of any seed (two implementations differ by ~1e-10 A in dev, so both
    select the same sets), (b) every (seed, round) whose tm lies within 1e-9 of the chain's maximum has the winner's selection (so
    whichever of them an implementation takes, it ends at one Kabsch fit on a known set), and (c) Horn's largest eigenvalue is well
    separated for the winning selection (section 6.11's condition for the 2-ulp tolerance)."""
    lens, hinged, pos_t, mask, pos_p = T.tm_batch()
    _, traces = T.tm_batch_reference()
    assert len(traces) == len(lens)
    margin, gap, lead = np.inf, np.inf, np.inf
    for e, m in enumerate(lens):
        a, shared, c, ahead = T.fairness(pos_t[e, :m, 1], pos_p[e, :m, 1], traces[e])
        assert a >= 1e-8, (e, m, a)
        assert shared, (e, m)
        assert c >= 1e-3, (e, m, c)
        margin, gap, lead = min(margin, a), min(gap, c), min(lead, ahead)
    print(f"seed {T.TM_SEED}: smallest |dev - cut| {margin:.3g} A, smallest Horn gap of a winning selection {gap:.3g}, "
          f"smallest lead over another selection {lead:.3g}, {sum(len(t['rounds']) for t in traces)} (seed, round) fits")
    assert abs(margin / T.FOUND["margin"] - 1) < 0.01 and abs(gap / T.FOUND["gap"] - 1) < 0.01
    kinds = [(m, h) for m in T.TM_LENGTHS for h in ((False, True) if m >= T.HINGE_FROM else (False,))]
    assert list(lens[:3]) == [0, 1, 2] and [(int(m), bool(h)) for m, h in zip(lens[3:], hinged[3:])] == kinds


def test_pure_host_abi():
    lib = _lib.load()
    assert set(NEW) <= set(_lib.EXPORTS)
    assert [f for f, _ in CTmScoreOut._fields_] == [f for f, _ in CSuperposeOut._fields_] + ["seed", "selected"]
    buf = np.zeros(256, np.uint8)
    p = buf.ctypes.data
    out = CTmScoreOut(p, p, p, p, p, p, p, p, p)
    fns = (lib.fcz_tmscore_dev, lib.fcz_tmscore_packed_dev, lib.fcz_tmscore, lib.fcz_tmscore_packed)
    for fn in fns:
        assert fn(None, p, p, p, p, p, 1, 4, 0, 1, 0, 20, ctypes.byref(out)) == -1
    fake = ctypes.c_void_p(buf.ctypes.data)                                  # refused before anything is touched (the ctx is never read)
    for fn in fns:
        assert fn(fake, p, p, p, p, p, 1, 4, 0, 37, 0, 20, ctypes.byref(out)) == -1 and fn(fake, p, p, p, p, p, 1, 4, 3, 1, 0, 20, ctypes.byref(out)) == -1
        assert fn(fake, p, p, p, p, p, 1, 4, 2, 4, 0, 20, ctypes.byref(out)) == -1 and fn(fake, p, p, p, p, p, 1, 4, 0, -1, 0, 20, ctypes.byref(out)) == -1
        assert fn(fake, None, p, p, p, p, 1, 4, 0, 1, 0, 20, ctypes.byref(out)) == -1 and fn(fake, p, None, p, p, p, 1, 4, 0, 1, 0, 20, ctypes.byref(out)) == -1
        assert fn(fake, p, p, None, p, p, 1, 4, 0, 1, 0, 20, ctypes.byref(out)) == -1 and fn(fake, p, p, p, p, p, 1, 4, 0, 1, 0, 20, None) == -1
        assert fn(fake, p, p, p, p, p, 1, 4, 0, 1, 0, 20, ctypes.byref(CTmScoreOut(None, p, p, p, p, p, p, p, p))) == -1
        assert fn(fake, p, p, p, p, p, 1, 4, 0, 1, 0, 20, ctypes.byref(CTmScoreOut(p, None, p, p, p, p, p, p, p))) == -1
        assert fn(fake, p, p, p, p, p, 1, 2 ** 31, 0, 1, 0, 20, ctypes.byref(out)) == -1
        assert fn(fake, p, p, p, p, p, 1, 4, 0, 1, 0, 65, ctypes.byref(out)) == -1                # iterations > 64
        assert fn(fake, p, p, p, p, p, 1, 4, 0, 1, 0, 2 ** 32 - 1, ctypes.byref(out)) == -1
    for fn in (lib.fcz_tmscore_dev, lib.fcz_tmscore):
        assert fn(fake, p, p, p, p, p, 1, 0, 0, 1, 0, 20, ctypes.byref(out)) == -1                # L == 0
    for fn in (lib.fcz_tmscore_packed_dev, lib.fcz_tmscore_packed):
        assert fn(fake, p, p, p, p, None, 1, 4, 0, 1, 0, 20, ctypes.byref(out)) == -1             # chains without a row_off
    assert not buf.any()


def test_argument_errors_need_no_device():
    pos37, mask37 = np.zeros((2, 8, 37, 3), F), np.zeros((2, 8, 37), np.uint8)
    pos4, mask4 = np.zeros((2, 8, 4, 3), F), np.zeros((2, 8, 4), np.uint8)
    true37, true4 = dict(pos=pos37, mask=mask37), dict(pos=pos4, mask=mask4)
    for pred, true, kw in ((pos37, true37, dict(atom="XX")), (pos4, true4, dict(atom="CB")), (pos37, true37, dict(atom=37)), (pos4, true4, dict(atom=4)),
                           (pos37, true37, dict(atom=-1)), (pos37, true37, dict(atom=1.5)), (pos37[:, :7], true37, {}), (pos4, true37, {}),
                           (dict(pos=pos37, mask=mask37[:1]), true37, {}), (dict(pos=pos37[:1], mask=mask37), true37, dict(apply=True)),
                           (pos37, true37, dict(iterations=65)), (pos37, true37, dict(iterations=-1)), (pos37, true37, dict(iterations=2.5)),
                           (pos37, true37, dict(iterations=True)), (pos37, true37, dict(iterations=None)), (pos37, true37, dict(levels=0)),
                           (pos37, true37, dict(levels=-2)), (pos37, true37, dict(levels=1.0)), (pos37, true37, dict(levels="all"))):
        with pytest.raises(ValueError):
            tensors.tm_score(pred, true, **kw)
    with pytest.raises(TypeError):
        tensors.tm_score(pos37, dict(pos=pos37))
    with pytest.raises(TypeError):
        tensors.tm_score(dict(mask=mask37), true37)
    assert api.check_tm_score("CA", pos37.shape, pos37.shape, mask37.shape) == (1, 20, 0)
    assert api.check_tm_score("CB", (9, 14, 3), (9, 14, 3), None, 0, 3) == (4, 0, 3) and api.check_tm_score(2, pos4.shape, pos4.shape, None, np.int64(64), np.int32(1)) == (2, 64, 1)
    assert api.check_tm_search() == (20, 0) and api.check_tm_search(0, 7) == (0, 7)
    for bad in (dict(iterations=65), dict(iterations=-1), dict(iterations=1.0), dict(iterations=False), dict(levels=0), dict(levels=-1), dict(levels=2.0), dict(levels=True)):
        with pytest.raises(ValueError):
            api.check_tm_search(**bad)
    import foldcomp
    import foldcomp_amd
    assert foldcomp.tm_score is foldcomp_amd.tm_score is tensors.tm_score
    assert "tm_score" in foldcomp.__all__ and "tm_score" in foldcomp_amd.__all__ and api.TM_MAX_ITERATIONS == 64
