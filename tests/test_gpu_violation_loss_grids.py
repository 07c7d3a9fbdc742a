"""The two violation-loss sweeps (k_violation_loss, k_violation_loss_grad) past the block cap of their persistent grids, through the
engine of tests/_sweep_grids.py unchanged: a batch that repeats a pool of D adversarial chains, sized from the CU count so that a block
takes a second tile of ANOTHER pool chain; no output row keeps its 0xA5 fill, chain e holds the bytes of pool chain e % D run alone,
and the batch agrees with the restatement (tests/_violation_loss.py) on bits. The pool's longest chain holds more atoms than one pass.
The grid arithmetic the cases rely on is asserted without a device for 64, 256 and 304 CUs."""
import numpy as np
import pytest

import _sweep_grids as G
import _violation_loss as VL
import _violations as V

VLOSS_PASS = 1280               # fcz_violation_loss.h: constexpr uint32_t VLOSS_PASS = 1280 (fcz_violation_loss_pass())
F = np.float32


class ViolationLoss(G.Analysis):
    """the value and the gradient of one call each: two launches over viol_tile_rows(A) rows a tile, 12 blocks a CU (fcz_abi.hip,
    vloss_rows). Tolerance 0 and link factor 0.5, so that every term class is there"""
    family = "atoms"
    per_cu = G.ATOMS_PER_CU
    chain_keys = frozenset({"counts"})
    params = (F(0), F(0.5))

    def __init__(self, A=14):
        self.A, self.tile_rows, self.name = A, G.viol_tile_rows(A), f"violation_loss A={A}"

    def launches(self):
        return [(f"{self.name} {k}", self.tile_rows, self.per_cu) for k in ("value", "grad")]

    def pool(self, lens, L):
        inp = dict(zip(("pos", "mask", "aatype"), G.atoms_pool(lens, L, self.A, 131)))
        return dict(inp, w_clash=VL.weights((len(lens), L, self.A), 132), w_link=VL.weights((len(lens), L, 3), 133))

    def ref(self, inp, lens):
        table = V.default_table(self.A)
        out = VL.loss(inp["pos"], inp["mask"], inp["aatype"], lens, table, *self.params)
        return dict(out, grad=VL.grad(inp["pos"], inp["mask"], inp["aatype"], lens, table, inp["w_clash"], inp["w_link"], *self.params))

    def fair(self, inp, ref, lens):
        assert int(ref["counts"][:, 0].max()) > VLOSS_PASS, (ref["counts"][:, 0], "the long chain takes one pass only")
        assert (ref["clash_loss"] > 0).any() and all((ref["link_loss"][..., k] > 0).any() for k in range(3)) and np.isfinite(ref["grad"]).all()

    def run(self, codec, dev, bound_t, n, rows, packed):
        a = (dev["pos"], dev["mask"], dev["aatype"], bound_t, n, rows, self.layout, packed)
        kw = dict(tol=self.params[0], factor=self.params[1], guard=self.guard)
        return dict(VL.run_value(codec, *a, **kw), grad=VL.run_grad(codec, *a, dev["w_clash"], dev["w_link"], **kw))

    def check(self, got, exp, what):
        VL.same(got, exp, what)


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
