"""The three sweeps of the all-atom FAPE (k_fape_atoms, k_fape_atoms_grad_frames, k_fape_atoms_grad_points) past the block cap of their
persistent grids, through the engine of tests/_sweep_grids.py unchanged: a batch that repeats a pool of D adversarial chains, sized
from the CU count so that a block takes a second tile of ANOTHER pool chain; no output row keeps its 0xA5 fill, chain e holds the bytes
of pool chain e % D run alone, and the batch agrees with the restatement (tests/_fape_atoms.py). The pool is the integer lattice: its
terms are exact, so no chain carries a tie allowance. The frame sweeps and the point sweep have tiles of different rows, so one batch
is sized for the larger need. The grid arithmetic the cases rely on is asserted without a device for 64, 256 and 304 CUs."""
import pytest

import _fape_atoms as FA
import _sweep_grids as G

FAPE_ATOMS = FA.FapeAtoms(14)
CASES = [G.Case(FAPE_ATOMS, "one", False), G.Case(FAPE_ATOMS, "one", True), G.Case(FAPE_ATOMS, "atoms", False), G.Case(FAPE_ATOMS, "atoms", True)]


@pytest.mark.parametrize("cus", G.N_CUS)
def test_every_case_crosses_its_cap(cus):
    """chain_tiles::reserve as fapea_rows calls it: fapea_tile_rows(A) rows a tile for the two frame sweeps, lddta_tile_rows(A, false)
    for the point sweep, n_cu * 12 blocks at most each"""
    for case in CASES:
        p = case.plan(cus).check()
        assert len(p.sizings) == 3 and all(s.cap == cus * FA.FAPEA_PER_CU and s.blocks == s.cap for s in p.sizings)
        assert len(p.lens) == p.sizings[0].D and 0 in p.lens and p.n % len(p.lens) == 0
        assert all(s.units - s.cap >= s.cap // G.MARGIN and s.busiest >= p.loops for s in p.sizings)
        if case.kind == "atoms":                                              # a tile, two tiles, two tiles and a row of the frame sweeps' tile; the long chain
            T = FA.fapea_tile_rows(14)
            assert p.L == 2 * T + 1 and {1, T, 2 * T, 2 * T + 1, G.LONG_ROWS} <= set(p.lens) and G.LONG_ROWS * 14 > FA.FAPEA_PASS
            assert p.sizings[2].units > p.sizings[0].units                    # (18 rows a tile against 64: the point sweep has more tiles)
    assert FA.fapea_tile_rows(4) == 128 and FA.fapea_tile_rows(37) == 64 and G.lddta_tile_rows(14, False) == 18


@pytest.mark.gpu
def test_the_mirrored_constants_are_the_library_s(codec):
    assert codec.lib.fcz_fape_atoms_pass() == FA.FAPEA_PASS
    assert [codec.lib.fcz_fape_atoms_tile_rows(lay) for lay in (0, 1, 2)] == [FA.fapea_tile_rows(A) for A in (37, 14, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_past_the_cap(codec, case):
    case.drive(codec, G.n_cu())
