"""GPU: the analyses over dense tensors past the block caps of their persistent grids. Every sweep runs
`for (tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)` under a cap that scales with the CU count (fcz_abi.hip: chain_tiles,
superpose_rows, frames_rows); the other GPU tests of these analyses use a few chains, so no block of theirs takes a second tile. The
cases here are sized from the device's CU count through the mirrored arithmetic of tests/_sweep_grids.py and assert, before any
launch, that their tiles (chains, for the wave-per-chain kernel) exceed the cap by an eighth at least, that the grid is the cap and
that the pool size D is coprime with it -- so a block re-stages its LDS, resets its per-lane state and looks up its chain for a tile
of ANOTHER pool chain of another length. Each batch repeats a pool of D adversarial chains (lengths 0, 1, 2, the tile and pass edges,
cleared masks over NaN payloads, non-finite coordinates under set masks, data behind every length), so the float64 / float32
restatement is computed on D chains only and expanded.

Every case asserts (tests/_sweep_grids.py, drive): no output row still holds its 0xA5 fill and the guards survive; chain e of the
batch holds the bytes the device gave for pool chain e % D when the pool ran alone and nothing looped; and the batch agrees with the
restatement under the analysis' own comparator and bounds.

The cases: the CHAIN_TILE sweeps (kNN at k = 5 and at k = 17 on atom14 for the KCAP = 32 instance, lDDT, the smooth lDDT with its
gradient, the DSSP H-bonds and labels, superpose_apply) at an entry a tile (L = 12, padded and packed), at three tiles an entry with
a partial last one (L = 513), kNN at more than two grids' worth of tiles, and kNN / lDDT / smooth lDDT / H-bonds with chains of more
than one candidate pass inside the looping grid (L = 2049); the atom-slot sweeps with tiles of their own (SASA, violations on atom14
and atom37, all-atom lDDT with exchanged side chains, whose decide and score launches both pass the cap) with a chain of more than
one pass of 1 536 atoms; k_superpose, the TM-score and the GDT search at a wavefront a chain, with more search items (counted from
the restatement's own seed lists) than blocks and more chains than k_gdt_final's grid; k_frames over the flat row space for both
group sets; and TM-align over a pair list that cycles through the 49 pairs of two sets of seven chains, past the caps of k_ta_count,
of the search grid and of the direction slots / k_ta_final (there the 49 pairs alone already loop in the search grid, which is
n_cu * 2 blocks: the byte comparison is against the same code at another grid phase, the restatement is the judge)."""
import pytest

import _sweep_grids as G

pytestmark = pytest.mark.gpu


def test_the_mirrored_passes_are_the_library_s(codec):
    lib = codec.lib
    assert (lib.fcz_knn_pass(), lib.fcz_lddt_pass(), lib.fcz_hbond_pass()) == (G.KNN_PASS, G.LDDT_PASS, G.HBOND_PASS)
    assert lib.fcz_sasa_pass() == lib.fcz_violations_pass() == lib.fcz_lddt_atoms_pass() == G.ATOM_PASS
    assert (lib.fcz_frames_width(0), lib.fcz_frames_width(1)) == (G.FRAMES_WIDTH[0], G.FRAMES_WIDTH[1])


@pytest.mark.parametrize("case", G.CASES, ids=[c.id for c in G.CASES])
def test_past_the_cap(codec, case):
    case.drive(codec, G.n_cu())


def test_tmalign_past_the_caps(codec):
    G.drive_tmalign(codec, G.n_cu())
