"""CPU: the sizing of tests/test_gpu_sweep_grids.py without a device. For 64, 256 and 304 CUs every case's tiles exceed the cap of the
launch it names by an eighth, its grid is the cap, some block takes a second (a third) tile and the pool size is coprime with the grid;
the pool generators meet the margin conditions their comparators need; and the expansion of a pool to a batch is what the packed
restatements give on the batch itself."""
import numpy as np
import pytest

import _analysis as AN
import _knn as K
import _sweep_grids as G


@pytest.mark.parametrize("cus", G.N_CUS)
def test_every_case_crosses_its_cap(cus):
    for case in G.CASES:
        p = case.plan(cus).check()
        assert len(p.lens) == p.sizings[0].D and 0 in p.lens and p.n % len(p.lens) == 0
        assert all(s.units - s.cap >= s.cap // G.MARGIN and s.busiest >= p.loops for s in p.sizings)
        if case.kind == "triple":
            assert all(s.busiest >= 3 for s in p.sizings)
        if case.kind == "atoms":                                              # two full tiles and a row of the largest tile, and the long chain
            T = max(t for _, t, _ in case.an.launches())
            assert 2 * T + 1 in p.lens and G.LONG_ROWS in p.lens and len(p.sizings) == len(case.an.launches())


@pytest.mark.parametrize("cus", G.N_CUS)
def test_tmalign_crosses_its_three_caps(cus):
    """(tmalign_pool asserts the conditions of test_tmalign_cpu.py for the 49 distinct pairs)"""
    m, which, sizings = G.tmalign_plan(cus)
    for s in sizings:
        s.check()
    assert len(which) == m and sorted(which[:49]) == list(range(49)) and [s.cap for s in sizings] == [cus * 16, cus * 2, cus * 8]


def test_the_mirror_is_the_arithmetic_it_names():
    assert G.size_padded("", 256, 16, 256, 12).n == 4613 and G.size_padded("", 256, 16, 256, 513).units >= 4608
    assert G.size_waves("", 256).n >= 256 * 72 and G.size_waves("", 256).cap == 4096
    assert G.tm_items_bound(1000, 10) == (1700 + 660) // 4 + 11
    assert [G.viol_tile_rows(A) for A in (37, 14, 4)] == [20, 18, 64] and [G.lddta_tile_rows(A, True) for A in (37, 14, 4)] == [64] * 3
    assert (G.frames_tile_rows(1), G.frames_tile_rows(0)) == (32, 256)
    s = G.size_packed("", 256, 16, 256, [0, 1, 12, 11, 2, 6, 4])
    assert s.units == s.n // 7 * 6 and s.n > G.size_padded("", 256, 16, 256, 12).n          # a chain without a row has no tile
    with pytest.raises(AssertionError):
        G.Sizing("too few", 7, 7, 4096, 4608, 4096, 4096).check()


def test_the_pools_meet_their_margin_conditions():
    """pool_and_ref runs every analysis' `fair` on the pool: tie_share, the GDT threshold margins and eigenvalue gaps, the fairness
    conditions of _tmscore.py and _gdt.py for the searches, the long chain's atoms beyond one pass, rows renamed by lddt_atoms"""
    seen = set()
    for case in G.CASES:
        if type(case.an).fair is G.Analysis.fair:
            continue
        p = case.plan(256)
        case.an.pool_and_ref(p.lens, p.L)
        seen.add(type(case.an).__name__)
    assert seen == {"LddtSoft", "Sasa", "Violations", "LddtAtoms", "Superpose", "TmScore", "Gdt"}


def test_expansion_against_the_packed_restatement():
    """the pool's padded restatement, packed and repeated with its row indices moved, is K.knn_packed of the repeated batch"""
    an = G.Knn(4, 1, 5)
    lens, L, n = G.pool_lens(12, 7), 12, 21
    inp, ref = an.pool_and_ref(lens, L)
    big = G.expand(an, inp, lens, n, True)
    row_off = AN.row_off_of(lens * 3)
    exp = K.knn_packed(big["pos"], big["mask"], row_off, 1, an.K_REF)
    got = G.expand(an, ref, lens, n, True)
    K.same((got["index"], got["dist"]), exp, "packed expansion")
    assert (got["index"][len(got["index"]) // 3 * 2:].max() >= int(row_off[14])) and G.expand(an, inp, lens, n, False)["pos"][8].tobytes() == inp["pos"][1].tobytes()
