"""The three FAPE sweeps (k_fape, k_fape_grad_frames, k_fape_grad_points) past the block cap of their persistent grids, through the
engine of tests/_sweep_grids.py unchanged: a batch that repeats a pool of D adversarial chains, sized from the CU count so that a
block takes a second tile of ANOTHER pool chain; no output row keeps its 0xA5 fill, chain e holds the bytes of pool chain e % D run
alone, and the batch agrees with the restatement (tests/_fape.py). The pool is the integer lattice: its terms are exact, so a chain of
2049 rows carries no tie allowance (a noisy chain that long would: tests/_fape.py). The grid arithmetic the cases rely on is asserted
without a device for 64, 256 and 304 CUs."""
import numpy as np
import pytest

import _sweep_grids as G

FAPE_PASS = G.FAPE_PASS         # fcz_fape.h, mirrored in tests/_sweep_grids.py beside the Fape analysis (tests/_analysis_fuzz.py shares it)

FAPE = G.Fape()
CASES = [G.Case(FAPE, "one", False), G.Case(FAPE, "one", True), G.Case(FAPE, "three"), G.Case(FAPE, "passes", own_pass=FAPE_PASS)]


@pytest.mark.parametrize("cus", G.N_CUS)
def test_every_case_crosses_its_cap(cus):
    """chain_tiles::reserve as fape_rows calls it: CHAIN_TILE rows a tile, n_cu * 16 blocks at most, for each of the three launches"""
    for case in CASES:
        p = case.plan(cus).check()
        assert len(p.sizings) == 3 and all(s.cap == cus * G.SWEEP_PER_CU and s.blocks == s.cap for s in p.sizings)
        assert len(p.lens) == p.sizings[0].D and 0 in p.lens and p.n % len(p.lens) == 0
        assert all(s.units - s.cap >= s.cap // G.MARGIN and s.busiest >= p.loops for s in p.sizings)
        if case.kind == "passes":                                             # chains about the pass and of more than two passes
            assert {FAPE_PASS - 1, FAPE_PASS, FAPE_PASS + 1, 2 * FAPE_PASS + 1} <= set(p.lens) and p.L == 2 * FAPE_PASS + 1
        if case.kind == "three":
            assert p.L == 2 * G.CHAIN_TILE + 1 and p.sizings[0].units == p.n * 3
    assert G.size_padded("", 256, G.SWEEP_PER_CU, G.CHAIN_TILE, 2049).n * 9 >= 4608


@pytest.mark.gpu
def test_the_mirrored_pass_is_the_library_s(codec):
    assert codec.lib.fcz_fape_pass() == FAPE_PASS


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_past_the_cap(codec, case):
    case.drive(codec, G.n_cu())
