"""The two violation-loss sweeps (k_violation_loss, k_violation_loss_grad) past the block cap of their persistent grids, through the
engine of tests/_sweep_grids.py unchanged: a batch that repeats a pool of D adversarial chains, sized from the CU count so that a block
takes a second tile of ANOTHER pool chain; no output row keeps its 0xA5 fill, chain e holds the bytes of pool chain e % D run alone,
and the batch agrees with the restatement (tests/_violation_loss.py) on bits. The pool's longest chain holds more atoms than one pass.
The grid arithmetic the cases rely on is asserted without a device for 64, 256 and 304 CUs."""
import pytest

import _sweep_grids as G

VLOSS_PASS = G.VLOSS_PASS       # fcz_violation_loss.h: constexpr uint32_t VLOSS_PASS = 1280 (fcz_violation_loss_pass())
ViolationLoss = G.ViolationLoss # the analysis is shared with the fuzz (tests/_analysis_fuzz.py); here at tolerance 0 and link factor 0.5

CASES = [G.Case(ViolationLoss(14), "atoms", False), G.Case(ViolationLoss(14), "atoms", True), G.Case(ViolationLoss(37), "atoms", False)]


@pytest.mark.parametrize("cus", G.N_CUS)
def test_every_case_crosses_its_cap(cus):
    """chain_tiles::reserve as vloss_rows calls it: viol_tile_rows(A) rows a tile, n_cu * 12 blocks at most, for both launches"""
    for case in CASES:
        p = case.plan(cus).check()
        T = case.an.tile_rows
        assert len(p.sizings) == 2 and all(s.cap == cus * G.ATOMS_PER_CU and s.blocks == s.cap for s in p.sizings)
        assert len(p.lens) == p.sizings[0].D and 0 in p.lens and p.n % len(p.lens) == 0
        assert all(s.units - s.cap >= s.cap // G.MARGIN and s.busiest >= p.loops for s in p.sizings)
        assert {0, 1, T, 2 * T, 2 * T + 1, G.LONG_ROWS} <= set(p.lens) and p.L == max(2 * T + 1, G.LONG_ROWS)
    assert G.LONG_ROWS * 14 > VLOSS_PASS


@pytest.mark.gpu
def test_the_mirrored_pass_is_the_library_s(codec):
    assert codec.lib.fcz_violation_loss_pass() == VLOSS_PASS


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_past_the_cap(codec, case):
    case.drive(codec, G.n_cu())
