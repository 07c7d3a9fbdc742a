"""CPU: what the all-atom lDDT has that needs no device -- the default swap table against the slot names, the refusal of tables that are no
involution, api.check_lddt_atoms, fcz_lddt_atoms_max_rows -- and the numpy restatement of the contract (tests/_lddt_atoms.py) on geometry
whose answer is known."""
import ctypes

import numpy as np
import pytest

import _lddt as LD
import _lddt_atoms as LA
from _dense import ATOM37
from foldcomp_amd import _lib, api

F = np.float32


@pytest.mark.parametrize("A", [37, 14, 4])
def test_default_swap_table(A):
    import foldcomp_amd as foldcomp
    lib = _lib.load()
    got = np.full((21, A), 0xA5, np.uint8)
    assert lib.fcz_lddt_default_swaps(LA.LAYOUT[A], got.ctypes.data) == 0
    assert np.array_equal(got, LA.default_table(A))
    assert np.array_equal(foldcomp.lddt_swaps(LA.WIDTH_LAYOUT[A]), got) and foldcomp.lddt_swaps(LA.WIDTH_LAYOUT[A]).dtype == np.uint8
    assert np.array_equal(np.take_along_axis(got, got.astype(np.int64), axis=1), np.tile(np.arange(A, dtype=np.uint8), (21, 1)))   # an involution
    moved = {(int(t), int(a)) for t, a in np.argwhere(got != np.arange(A))}
    if A == 37:
        s = ATOM37.index
        assert moved == ({(LA.ASP, s("OD1")), (LA.ASP, s("OD2")), (LA.GLU, s("OE1")), (LA.GLU, s("OE2"))} |
                         {(t, s(nm)) for t in (LA.PHE, LA.TYR) for nm in ("CD1", "CD2", "CE1", "CE2")})
    elif A == 14:
        assert len(moved) == 12 and {t for t, _ in moved} == {LA.ASP, LA.GLU, LA.PHE, LA.TYR}
    else:
        assert not moved
    assert lib.fcz_lddt_default_swaps(3, got.ctypes.data) == -1 and lib.fcz_lddt_default_swaps(LA.LAYOUT[A], None) == -1
    with pytest.raises(ValueError):
        foldcomp.lddt_swaps("atom5")


def test_max_rows_and_pass():
    lib = _lib.load()
    for A in (37, 14, 4):
        assert lib.fcz_lddt_atoms_max_rows(LA.LAYOUT[A]) == (2 ** 31 - 1) // (4 * A * A) == LA.max_rows(A)
    assert lib.fcz_lddt_atoms_max_rows(3) == -1 and lib.fcz_lddt_atoms_max_rows(-1) == -1
    assert lib.fcz_lddt_atoms_pass() > 0


def test_a_bad_table_is_refused():
    """a table that is no involution within a row or points outside the layout is refused by the argument check (the C calls refuse it
    too, behind their context check: tests/test_gpu_lddt_atoms.py); without a context every form answers FCZ_E_INVALID_ARG"""
    from foldcomp_amd.structure import CLddtAtomsOut
    lib = _lib.load()
    out = CLddtAtomsOut()
    for fn in (lib.fcz_lddt_atoms_dev, lib.fcz_lddt_atoms_packed_dev, lib.fcz_lddt_atoms, lib.fcz_lddt_atoms_packed):
        assert fn(None, None, None, None, None, None, None, 1, 8, 0, 15.0, None, None, ctypes.byref(out)) == -1
    for A in (37, 14):
        good = LA.default_table(A)
        chain, outside, one_way = good.copy(), good.copy(), good.copy()
        chain[5, 1], chain[5, 2], chain[5, 3] = 2, 3, 1                       # 1 -> 2 -> 3 -> 1
        outside[20, 0] = A
        one_way[0, 4] = 5                                                     # 4 -> 5, 5 -> 5
        for bad in (chain, outside, one_way, good.astype(np.int64) - 1, good[:20], good.astype(np.float32)):
            with pytest.raises(ValueError):
                api.check_lddt_atoms(15.0, None, bad, (2, 8, A, 3), (2, 8, A, 3))
        assert np.array_equal(api.check_lddt_atoms(15.0, None, good.astype(np.int64), (2, 8, A, 3), (2, 8, A, 3))[2], good)
    with pytest.raises(ValueError):
        api.check_lddt_atoms(15.0, None, LA.default_table(14), (2, 8, 37, 3), (2, 8, 37, 3))   # the table of another layout


def test_check_lddt_atoms():
    shape = (3, 50, 37, 3)
    cutoff, th, table = api.check_lddt_atoms(15, None, "alphafold", shape, shape)
    assert cutoff == 15.0 and th == (0.5, 1.0, 2.0, 4.0) and table is None
    assert api.check_lddt_atoms(15, (1, 2, 3, 4), None, shape, shape, has_aatype=False)[1:] == ((1.0, 2.0, 3.0, 4.0), False)
    custom = LA.table_of(37, {LA.VAL: [("CG1", "CG2")]})
    got = api.check_lddt_atoms(15, None, custom.astype(np.int32), (700, 37, 3), (700, 37, 3), (700, 37), per_atom=True)[2]
    assert got.dtype == np.uint8 and got.flags["C_CONTIGUOUS"] and np.array_equal(got, custom)
    bad = [dict(cutoff=0), dict(cutoff=float("nan")), dict(cutoff=float("inf")), dict(cutoff="15"), dict(cutoff=True), dict(thresholds=(1, 2, 3)),
           dict(thresholds=(1, 2, 3, float("nan"))), dict(swaps="openstructure"), dict(swaps=7), dict(has_aatype=False), dict(per_atom=1),
           dict(shape=(3, 50, 5, 3)), dict(shape=(3, 50, 37)), dict(shape=(50, 37, 3, 3, 3)), dict(pred_shape=(3, 50, 14, 3)), dict(pred_mask_shape=(3, 50)),
           dict(shape=(1, LA.max_rows(37) + 1, 37, 3), pred_shape=(1, LA.max_rows(37) + 1, 37, 3)),
           dict(shape=(LA.max_rows(4) + 1, 4, 3), pred_shape=(LA.max_rows(4) + 1, 4, 3))]
    for b in bad:
        a = dict(cutoff=15.0, thresholds=None, swaps="alphafold", shape=shape, pred_shape=shape, pred_mask_shape=None, has_aatype=True, per_atom=False)
        a.update(b)
        with pytest.raises(ValueError):
            api.check_lddt_atoms(**a)
    ok = (1, LA.max_rows(37), 37, 3)
    api.check_lddt_atoms(15.0, None, "alphafold", ok, ok)
    import foldcomp_amd as foldcomp
    with pytest.raises(TypeError):
        foldcomp.lddt_atoms(dict(pos=np.zeros(shape, F)), dict(pos=np.zeros(shape, F)))     # no mask of true
    with pytest.raises(ValueError):
        foldcomp.lddt_atoms(np.zeros(shape, F), dict(pos=np.zeros(shape, F), mask=np.ones(shape[:-1], bool)))   # no aatype, but a renaming


# ---- the restatement on known geometry -------------------------------------------------------------------------------------------

def _cloud(m, A, seed, spread=6.0):
    """m rows of A atoms scattered about a random walk of CA positions: every row has atoms of other rows within the cutoff"""
    rng = np.random.default_rng(seed)
    ca = np.cumsum(rng.standard_normal((m, 3)) * 2.2, axis=0).astype(F)
    pos = (ca[:, None, :] + rng.standard_normal((m, A, 3)) * spread / 3).astype(F)
    pos[:, 1] = ca
    return pos


def test_restatement_with_one_atom_a_row_is_the_ca_lddt():
    m = 90
    for A in (37, 14, 4):
        pt = _cloud(m, A, 5)
        pp = (pt + np.random.default_rng(6).standard_normal(pt.shape) * 0.8).astype(F)
        mask = np.zeros((m, A), np.uint8)
        mask[:, 1] = 1
        mask[[3, 40], 1] = 0
        pp[7, 1, 2] = np.nan
        aa = np.random.default_rng(7).integers(0, 21, m).astype(np.uint8)
        got = LA.lddt_atoms_chain(pt, mask, pp, None, aa, LA.default_table(A))
        site = (mask[:, 1] != 0) & np.isfinite(pp[:, 1]).all(axis=-1)
        exp = LD.lddt_chain(pt[:, 1], pp[:, 1], site)
        LD.same((got["score"], got["pairs"], got["hits"]), exp, f"A = {A}")
        assert got["pairs"].sum() > 1000 and not got["swapped"].any()
        assert np.array_equal(got["atom_pairs"][:, 1], exp[1]) and not np.delete(got["atom_pairs"], 1, axis=1).any()


def _phe_case(A):
    """a chain of 40 rows with every slot present, row 11 a PHE, rows 20 a TYR and 30 an ASP as further ambiguous rows"""
    m = 40
    pt = _cloud(m, A, 11)
    aa = np.zeros(m, np.uint8)                                                # ALA: no slot of the other rows has a partner
    aa[11], aa[20], aa[30] = LA.PHE, LA.TYR, LA.ASP
    pp = (pt + np.random.default_rng(12).standard_normal(pt.shape) * 0.3).astype(F)
    return pt, np.ones((m, A), np.uint8), pp, aa


@pytest.mark.parametrize("A", [37, 14])
def test_restatement_resolves_an_exchanged_phe(A):
    table = LA.default_table(A)
    pt, mask, pp, aa = _phe_case(A)
    plain = LA.lddt_atoms_chain(pt, mask, pp, mask, aa, table)
    assert not plain["swapped"].any() and plain["pairs"].sum() > 10000
    rows = np.zeros(len(aa), bool)
    rows[11] = True
    flipped = LA.exchange(pp, aa, rows, table)
    assert (flipped[11] != pp[11]).any(axis=-1).sum() == 4 and np.array_equal(np.delete(flipped, 11, axis=0), np.delete(pp, 11, axis=0))
    got = LA.lddt_atoms_chain(pt, mask, flipped, mask, aa, table)
    assert got["swapped"].tolist() == rows.astype(np.uint8).tolist()
    # the scores of the unexchanged prediction: per row, and per atom at the prediction's slot (row 11's four atoms exchanged)
    LA.same(got, plain, "rows", LA.ROW_KEYS[:3])
    for k in ("atom_pairs", "atom_hits"):
        assert np.array_equal(got[k], LA.exchange(plain[k][..., None], aa, rows, table)[..., 0]), k
    # without the renaming the exchanged ring is punished
    none = LA.lddt_atoms_chain(pt, mask, flipped, mask, aa, None)
    assert not none["swapped"].any() and none["hits"][11] < got["hits"][11] and none["pairs"][11] == got["pairs"][11]
    assert LA.chain_quotient(none["pairs"], none["hits"]) < LA.chain_quotient(got["pairs"], got["hits"])
    # the padded and the packed wrapper: two such chains, the second cut to 25 rows
    pos_t, pos_p = np.stack([pt, pt]), np.stack([flipped, flipped])
    m2, aa2 = np.stack([mask, mask]), np.stack([aa, aa])
    pad = LA.lddt_atoms(pos_t, m2, pos_p, m2, aa2, np.asarray([40, 25], np.uint32), table)
    LA.same({k: v[0] for k, v in pad.items()}, got, "padded")
    assert not pad["pairs"][1, 25:].any() and pad["pairs"][1, :25].all() and pad["swapped"][1, 11]
    cat = lambda a: np.concatenate([a[0], a[1, :25]])
    pk = LA.lddt_atoms(cat(pos_t), cat(m2), cat(pos_p), cat(m2), cat(aa2), np.asarray([0, 40, 65], np.uint32), table, packed=True)
    LA.same(pk, {k: cat(v) for k, v in pad.items()}, "packed")


def test_restatement_leaves_an_undecidable_row_alone():
    A = 37
    table = LA.default_table(A)
    pt, mask, pp, aa = _phe_case(A)
    rows = np.zeros(len(aa), bool)
    rows[[11, 20]] = True
    flipped = LA.exchange(pp, aa, rows, table)
    for which, m_t, m_p in (("true", 0, 1), ("pred", 1, 0)):
        mt, mp = mask.copy(), mask.copy()
        (mt if m_t == 0 else mp)[11, ATOM37.index("CE2")] = 0                 # one ambiguous atom of the PHE is masked off
        got = LA.lddt_atoms_chain(pt, mt, flipped, mp, aa, table)
        assert got["swapped"][11] == 0 and got["swapped"][20] == 1 and got["swapped"].sum() == 1, which
    # a coordinate that is not finite does the same
    bad = flipped.copy()
    bad[11, ATOM37.index("CD1"), 0] = np.inf
    got = LA.lddt_atoms_chain(pt, mask, bad, mask, aa, table)
    assert got["swapped"][11] == 0 and got["swapped"][20] == 1
    # a tie is no swap: the prediction is the truth and the two namings of a row coincide
    same = pt.copy()
    same[30, ATOM37.index("OD2")] = same[30, ATOM37.index("OD1")]
    assert not LA.lddt_atoms_chain(same, mask, same, mask, aa, table)["swapped"].any()
