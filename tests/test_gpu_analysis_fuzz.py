"""GPU: the seeded differential fuzz of the dense-tensor analyses (tests/_analysis_fuzz.py). The other GPU tests of these analyses run at
hand-picked lengths on three input recipes that barely vary what the kernels' control flow depends on; here every (analysis, group)
runs its cases of the generator's list: masks from every mask set to a whole chain cleared, cleared runs longer than a staging step,
a query tile and a pass, 1 to 3 sites in a chain of hundreds of rows, residue types from GLY to the layout's largest and unknown
ones, NaN / inf / 3e19 under set masks, seven geometries from a compact globule to coincident sites, the tile and pass edges, chains
designed through the mirror of chain_stage_slots so that a pass closes exactly full, one slot under it and with a final pass that
stages nothing, in the padded form (length, clamped length, NULL) and the packed one (uncovered rows in front and behind), with
outputs at unaligned offsets.

Every case asserts (tests/_analysis_fuzz.py, drive): WRITTEN, ALONE and REFERENCE, the last under the analysis' own comparator and
bounds. The groups: edges (0 to 3 rows and the tile edges), passes (the row-pass edges), design (the atom-pass edges), few (0 to 3
sites, coincident and collinear chains for the wave-per-chain kernels), long (TM_LDS_ROWS - 1 .. + 1; for the atom-pass sweeps long4 /
long14 / long37: chains of three passes and more that are not designed, with cleared runs longer than a pass at either end and
non-finite values at the pass edges), mix (everything by seed), and for TM-align pairs (every chain of a fuzzed set against a related
or unrelated chain of a second set, 120 rows or under, through _sweep_grids.tmalign_check). The violation loss and its gradient run
with their own pass of 1280 atoms, staged in ascending order: their designed chains hold a clash partner at the last place of the
fullest pass, and their inputs carry upstream weights with zeros, a 1e15 and NaN patterns where no weight is read.

The all-atom FAPE (fape_atoms) runs its value and both gradient sweeps a case, all five outputs under WRITTEN, ALONE (on bytes: the
order of every sum is the chain's alone) and REFERENCE (_fape_atoms.check_value / check_grad, bounds unchanged). Its design group
aims at what masks that are all set never reach: point passes that close holding 1024 and 1023 (every mask set closes at 1024 / 1008 /
962), frame passes of k_fape_atoms_grad_points of 256 right behind steps that stage nothing, of 255 and of 1 and a final pass of
nothing, and chains of one tile whose frames or points end on the edges of a wavefront and of a round of 256. Its inputs carry
swapped rows, NULL aatype / swapped / mask_pred / fmask_pred, non-finite values either side of every pass edge and weights with NaN
patterns at every item that is no frame."""
import pytest

import _analysis_fuzz as FZ
import _fape_atoms as FA
import _sweep_grids as G

pytestmark = pytest.mark.gpu

CASES = FZ.cases()
ORDER = list(FZ.SPECS) + ["tmalign"]
GROUPS = sorted({(c.analysis, c.group) for c in CASES}, key=lambda g: (ORDER.index(g[0]), g[1]))


def test_the_mirrored_constants_are_the_library_s(codec):
    lib = codec.lib
    assert lib.fcz_sasa_pass() == lib.fcz_violations_pass() == lib.fcz_lddt_atoms_pass() == G.ATOM_PASS
    assert (lib.fcz_knn_pass(), lib.fcz_lddt_pass(), lib.fcz_hbond_pass(), lib.fcz_fape_pass()) == (G.KNN_PASS, G.LDDT_PASS, G.HBOND_PASS, G.FAPE_PASS)
    assert FZ.ATOM_STEP == 2 * G.BLOCK and FZ.ATOM_STEP % G.BLOCK == 0 and G.ATOM_PASS % FZ.ATOM_STEP == 0
    assert lib.fcz_violation_loss_pass() == G.VLOSS_PASS == 1280 and FZ.VLOSS_STEP == 2 * G.BLOCK and G.VLOSS_PASS % FZ.VLOSS_STEP != 0
    assert lib.fcz_fape_atoms_pass() == 1024 == FA.FAPEA_PASS == FZ.SPECS["fape_atoms"].pass_atoms and FZ.FAPEA_STEP == 2 * G.BLOCK
    assert [lib.fcz_fape_atoms_tile_rows(G.LAYOUT[A]) for A in (4, 14, 37)] == [FZ.SPECS["fape_atoms"].tile(A) for A in (4, 14, 37)] == [128, 64, 64]


@pytest.mark.parametrize("analysis,group", GROUPS, ids=[f"{a}-{g}" for a, g in GROUPS])
def test_fuzz(codec, analysis, group):
    for case in CASES:
        if (case.analysis, case.group) == (analysis, group):
            FZ.drive(codec, case)
