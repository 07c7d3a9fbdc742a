"""CPU: the parts of the structural-violations feature that need no device -- the numpy restatement (tests/_violations.py) on geometry
whose answer is known (an ideal helix, a planted clash, the two exclusions, a stretched link, a proline link), the symmetry of the
clash count, the restatement on the reference's real structures, the pure-host ABI (fcz_violations_pass, the refusals, the export
list) and the argument errors of foldcomp.violations, raised before torch or a device is touched."""
import ctypes

import numpy as np
import pytest

import _dssp as D
import _violations as V
from foldcomp_amd import _lib, api, tensors
from foldcomp_amd.structure import CViolationsOut

F = np.float32
NEW = ("fcz_violations_pass", "fcz_violations_dev", "fcz_violations_packed_dev", "fcz_violations", "fcz_violations_packed")
AA3 = "ALA ARG ASN ASP CYS GLN GLU GLY HIS ILE LEU LYS MET PHE PRO SER THR TRP TYR VAL".split()
BB4 = V.default_table(4)
REAL = ("pdb:test", "pdb:test_af", "pdb:multichainA", "pdb:multichainB_0", "pdb:multichainB_1")


def _helix(m):
    pos, mask = D.ideal_backbone(-57, -47, m)
    return pos.copy(), mask.copy(), np.zeros(m, np.uint8)


@pytest.mark.parametrize("m", [1, 2, 30, 120])
def test_an_ideal_helix_has_no_violation(m):
    pos, mask, aa = _helix(m)
    v = V.violations_chain(pos, mask, aa, BB4)
    assert not v["clash_atom"].any() and not v["clash_count"].any() and not v["clash_depth"].any() and (v["clash_partner"] == -1).all()
    assert v["viol_mask"].all() and v["link_mask"][:-1].all() and not v["link_mask"][-1] and not v["link_violation"].any()
    assert list(v["counts"]) == [4 * m, 0, 0, 0]
    if m > 1:                                                                 # the geometry the backbone was built with
        assert np.abs(v["link_length"][:-1] - 1.329).max() < 1e-4 and not v["link_length"][-1]
        assert np.abs(v["link_cos"][:-1, 0] - np.cos(np.radians(116.2))).max() < 1e-4
        assert np.abs(v["link_cos"][:-1, 1] - np.cos(np.radians(121.7))).max() < 1e-4 and not v["link_cos"][-1].any()
    # without the peptide-bond exclusion the clashing pairs are exactly the peptide bonds: one per link, C - N' = 1.329 < 1.75
    idx, clash, _ = V.clash_matrix(pos, mask, aa, BB4)
    row, slot = idx[:, 0], idx[:, 1]
    T = (BB4[0][slot][:, None] + BB4[0][slot][None, :]) - V.TOL
    raw = (row[:, None] != row[None, :]) & (V._d2(pos[mask != 0][:, None], pos[mask != 0][None]) < T * T)
    assert int(np.triu(raw, 1).sum()) == m - 1 and not clash.any()


def test_a_planted_clash_is_counted_by_hand():
    """O of row 20 moved to 0.5 from CA of row 3 along x: it clashes with that CA (T = 1.52 + 1.70 - 1.5) and with whatever else of row 3
    and its neighbours lies inside T, each worked out here atom by atom"""
    pos, mask, aa = _helix(30)
    pos[20, 3] = pos[3, 1] + np.asarray([0.5, 0, 0], F)
    v = V.violations_chain(pos, mask, aa, BB4)
    radius = BB4[0]
    hits = []                                                                 # (row, slot, depth) of the atoms the moved O clashes with
    for r in range(30):
        for a in range(4):
            if r == 20:
                continue
            T = (radius[3] + radius[a]) - V.TOL
            d = pos[20, 3] - pos[r, a]
            d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            if T > 0 and d2 < T * T:
                hits.append((r, a, T - np.sqrt(d2)))
    assert (3, 1) in [(r, a) for r, a, _ in hits]
    assert v["clash_count"][20] == len(hits) and v["clash_atom"][20].tolist() == [0, 0, 0, 1]
    best = max(h[2] for h in hits)
    assert v["clash_depth"][20].view(np.uint32) == F(best).view(np.uint32)
    assert v["clash_partner"][20] == min(r for r, _, dep in hits if dep == best)
    for r in sorted({h[0] for h in hits}):                                    # and from the other side
        mine = [h for h in hits if h[0] == r]
        assert v["clash_count"][r] == len(mine) and v["clash_partner"][r] == 20
        assert v["clash_atom"][r].tolist() == [int(any(h[1] == a for h in mine)) for a in range(4)]
        assert v["clash_depth"][r].view(np.uint32) == F(max(h[2] for h in mine)).view(np.uint32)
    others = np.ones(30, bool)
    others[[20] + [h[0] for h in hits]] = False
    assert not v["clash_count"][others].any() and (v["clash_partner"][others] == -1).all()
    assert v["counts"][1] == len(hits) and v["clash_count"].sum() == 2 * len(hits)
    # a tie on depth goes to the smallest row: two atoms at the same distance on either side
    pos, mask, aa = _helix(3)
    pos[:] = 0
    pos[:, :, 0] = 100.0 + np.arange(3)[:, None] * 40.0 + np.arange(4)[None, :] * 8.0   # everything far apart
    pos[0, 1], pos[1, 1], pos[2, 1] = [1, 0, 0], [0, 0, 0], [-1, 0, 0]
    v = V.violations_chain(pos, mask, aa, BB4)
    assert v["clash_partner"].tolist() == [1, 0, 1] and v["clash_count"].tolist() == [1, 2, 1] and v["counts"][1] == 2
    assert v["clash_depth"][1].view(np.uint32) == (((F(1.7) + F(1.7)) - V.TOL) - F(1)).view(np.uint32)
    # coordinates like 3e19 (d2 = +inf) are no clash, NaN and cleared masks are no atoms
    pos[0, 1] = [3e19, 0, 0]
    pos[2, 1, 0] = np.nan
    v = V.violations_chain(pos, mask, aa, BB4)
    assert not v["clash_count"].any() and v["counts"][0] == 11


def test_exclusions():
    T37 = V.default_table(37)
    pos, mask = np.zeros((6, 37, 3), F), np.zeros((6, 37), np.uint8)
    bb, _ = D.ideal_backbone(-57, -47, 6)
    pos[:, [0, 1, 2, 4]], mask[:, [0, 1, 2, 4]] = bb, 1
    aa = np.zeros(6, np.uint8)
    base = V.violations_chain(pos, mask, aa, T37)
    assert not base["clash_count"].any()
    # N of row 3 moved onto C of row 2: that pair is the peptide bond, and no clash; the moved N may still clash with others
    moved = pos.copy()
    moved[3, 0] = pos[2, 2]
    idx, clash, _ = V.clash_matrix(moved, mask, aa, T37)
    i, j = [int(np.flatnonzero((idx == rs).all(axis=1))[0]) for rs in ((2, 2), (3, 0))]
    assert not clash[i, j] and not clash[j, i]
    # ... while C of row 2 onto N of row 4 (not the next row) is a clash
    far = pos.copy()
    far[4, 0] = pos[2, 2]
    idx, clash, _ = V.clash_matrix(far, mask, aa, T37)
    i, j = [int(np.flatnonzero((idx == rs).all(axis=1))[0]) for rs in ((2, 2), (4, 0))]
    assert clash[i, j] and clash[j, i]
    # two SG atoms 2.05 apart (T = 3.6 - 1.5 = 2.1): no clash between two CYS, a clash when one row is not CYS or aatype is missing
    sg = V.SG_SLOT[37]
    ss = pos.copy()
    m2 = mask.copy()
    ss[0, sg], ss[5, sg] = [50, 50, 50], [52.05, 50, 50]
    m2[0, sg] = m2[5, sg] = 1
    cys = aa.copy()
    cys[[0, 5]] = V.CYS
    assert not V.violations_chain(ss, m2, cys, T37)["clash_count"].any()
    one = cys.copy()
    one[5] = 15
    for types in (one, None):
        v = V.violations_chain(ss, m2, types, T37)
        assert v["clash_count"].tolist() == [1, 0, 0, 0, 0, 1] and v["clash_partner"].tolist() == [5, -1, -1, -1, -1, 0] and v["clash_atom"][0, sg] == 1
    # atom14: the same atoms, SG in slot 5 of a CYS row
    p14, m14 = np.zeros((6, 14, 3), F), np.zeros((6, 14), np.uint8)
    p14[:, :4], m14[:, :4] = bb, 1
    p14[0, 5], p14[5, 5], m14[0, 5], m14[5, 5] = ss[0, sg], ss[5, sg], 1, 1
    assert not V.violations_chain(p14, m14, cys, V.default_table(14))["clash_count"].any()
    assert not V.violations_chain(p14, m14, one, V.default_table(14))["clash_count"].any()   # (slot 5 of SER is OG, 1.52: T = 1.82 < 2.05)
    p14[5, 5] = [51.7, 50, 50]
    assert not V.violations_chain(p14, m14, cys, V.default_table(14))["clash_count"].any()
    assert V.violations_chain(p14, m14, one, V.default_table(14))["clash_count"].tolist() == [1, 0, 0, 0, 0, 1]


def test_links():
    pos, mask, aa = _helix(12)
    # the rows from 6 on moved along the C - N' bond of link 5 until it is 2 Angstrom long: the angles stay
    u = pos[6, 0] - pos[5, 2]
    pos[6:] += (u / np.linalg.norm(u) * (2.0 - np.linalg.norm(u))).astype(F)
    v = V.violations_chain(pos, mask, aa, BB4)
    assert v["link_violation"].tolist() == [0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0] and abs(float(v["link_length"][5]) - 2.0) < 1e-5
    assert list(v["counts"][2:]) == [1, 0]
    # PRO uses its own length: 1.329 + 12 * 0.014 = 1.497 against 1.341 + 12 * 0.016 = 1.533, a link of 1.515 lies between them
    pos, mask, aa = _helix(12)
    u = pos[6, 0] - pos[5, 2]
    pos[6:] += (u / np.linalg.norm(u) * (1.515 - np.linalg.norm(u))).astype(F)
    assert V.violations_chain(pos, mask, aa, BB4)["link_violation"][5] == 1
    pro = aa.copy()
    pro[6] = V.PRO
    assert V.violations_chain(pos, mask, pro, BB4)["link_violation"][5] == 0
    pro5 = aa.copy()
    pro5[5] = V.PRO                                                           # (the type of row r + 1 decides, not of row r)
    assert V.violations_chain(pos, mask, pro5, BB4)["link_violation"][5] == 1
    assert V.violations_chain(pos, mask, None, BB4)["link_violation"][5] == 1
    # a bent link sets the angle bits only; a missing CA or a NaN N' means no link, and every field 0
    pos, mask, aa = _helix(12)
    pos[6, 1] = pos[6, 0] + (pos[5, 2] - pos[6, 0]) * F(0.9) + F(0.4)         # CA' nearly on the C - N' line
    v = V.violations_chain(pos, mask, aa, BB4)
    assert v["link_violation"][5] == 4 and v["link_mask"][5]
    mask[5, 1] = 0
    pos[8, 0, 2] = np.nan
    v = V.violations_chain(pos, mask, aa, BB4)
    for r in (4, 5, 7):
        assert not v["link_mask"][r] and v["link_length"][r] == 0 and not v["link_cos"][r].any() and v["link_violation"][r] == 0
    # a zero norm gives NaN, which is no violation
    pos, mask, aa = _helix(4)
    pos[1, 1] = pos[1, 2]
    v = V.violations_chain(pos, mask, aa, BB4)
    assert np.isnan(v["link_cos"][1, 0]) and not v["link_violation"][1] & 2


def test_symmetry_and_forms():
    rng = np.random.default_rng(5)
    lens = [0, 1, 9, 40]
    L = 44
    pos, mask = np.zeros((4, L, 4, 3), F), (rng.random((4, L, 4)) < 0.9).astype(np.uint8)
    for e, m in enumerate(lens):
        pos[e, :m] = (rng.random((m, 4, 3)) * (m ** (1 / 3) * 3.5)).astype(F)  # dense: many clashes
        pos[e, m:] = rng.normal(size=(L - m, 4, 3))                           # behind length: never read
    aa = rng.integers(0, 25, size=(4, L)).astype(np.uint8)
    pad = V.violations(pos, mask, aa, np.asarray(lens), BB4)
    assert pad["clash_count"][3].sum() > 40 and pad["chain_counts"][3, 1] > 20 and pad["chain_counts"][3, 2] > 10
    for e in range(4):
        assert pad["clash_count"][e].sum() % 2 == 0 and pad["clash_count"][e].sum() == 2 * pad["chain_counts"][e, 1]
    V.consistent(pad, np.asarray(lens))
    row_off = np.concatenate([[0], np.cumsum(lens)])
    cat = lambda a: np.concatenate([a[e, :m] for e, m in enumerate(lens)])
    packed = V.violations(cat(pos), cat(mask), cat(aa), row_off, BB4, packed=True)
    V.same_violations(packed, {k: (pad[k] if k == "chain_counts" else cat(pad[k])) for k in V.KEYS}, "packed")
    for k in V.KEYS[:-1]:
        fill = -1 if k == "clash_partner" else 0
        assert all((pad[k][e, m:] == fill).all() for e, m in enumerate(lens)), k


def test_real_structures(golden):
    """the reference's real structures (test.pdb, test_af.pdb, the chains of multichain.pdb as the goldens hold them): whatever the
    restatement finds there is what the GPU test expects; here only what must hold of any folded chain is asserted, and the figures
    are printed"""
    z, _ = golden
    for name in REAL:
        views, aa = V.chain_of_text(z[f"{name}/pdb0"].tobytes().decode("latin-1"), AA3)
        v37 = V.violations_chain(*views[37], aa, V.default_table(37))
        v14 = V.violations_chain(*views[14], aa, V.default_table(14))
        print(name, len(aa), "atoms, pairs, bond rows, angle rows:", v37["counts"].tolist(), "deepest", float(v37["clash_depth"].max()))
        for k in V.KEYS[1:-1]:                                                 # the layouts describe the same atoms
            assert np.array_equal(np.asarray(v37[k]).view(np.uint8), np.asarray(v14[k]).view(np.uint8)), (name, k)
        assert np.array_equal(v37["counts"], v14["counts"]) and v37["viol_mask"].all() and v37["counts"][0] == views[14][1].sum()
        assert v37["link_mask"][:-1].all() and v37["clash_count"].sum() == 2 * v37["counts"][1]
        assert v37["counts"][1] * 50 <= len(aa), "a deposited or predicted structure has next to no clash at tolerance 1.5"


def test_the_pass_and_the_exports():
    lib = _lib.load()
    assert set(NEW) <= set(_lib.EXPORTS) and lib.fcz_violations_pass() > 0
    import foldcomp
    import foldcomp_amd
    assert foldcomp.violations is foldcomp_amd.violations is tensors.violations and "violations" in foldcomp.__all__
    assert [k for k, _, _ in api.VIOLATION_OUTPUTS] == list(V.KEYS) == [f[0] for f in CViolationsOut._fields_]


def test_refusals_need_no_device():
    lib = _lib.load()
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    fake = ctypes.c_void_p(p)                                                  # refused before anything is touched (the ctx is never read)
    tab = V.default_table(37)
    big, nan_tab, neg, small = tab.copy(), tab.copy(), tab.copy(), tab.copy()
    big[3, 5], nan_tab[20, 0], neg[0, 0], small[7, 7] = 8.0, np.nan, -1.0, 0.4

    def call(fn, **kw):
        a = dict(ctx=fake, pos=p, mask=p, aa=p, bound=p, n=1, rows=4, layout=0, table=None, tol=1.5, factor=12.0, out={})
        a.update(kw)
        out = None if a["out"] is None else ctypes.byref(CViolationsOut(*(a["out"].get(k, p) for k in V.KEYS)))
        return fn(a["ctx"], a["pos"], a["mask"], a["aa"], a["bound"], a["n"], a["rows"], a["layout"], a["table"], a["tol"], a["factor"], out)

    bad = [dict(ctx=None), dict(pos=None), dict(mask=None), dict(out=None), dict(layout=3), dict(layout=-1), dict(rows=2 ** 31),
           dict(tol=float("nan")), dict(tol=float("inf")), dict(tol=-0.1), dict(factor=float("nan")), dict(factor=float("inf")), dict(factor=-1.0),
           dict(table=big.ctypes.data), dict(table=nan_tab.ctypes.data), dict(table=neg.ctypes.data), dict(table=small.ctypes.data), dict(layout=1, aa=None)]
    bad += [dict(out={k: None}) for k in V.KEYS]
    for fn in (lib.fcz_violations_dev, lib.fcz_violations_packed_dev, lib.fcz_violations, lib.fcz_violations_packed):
        for b in bad:
            assert call(fn, **b) == -1, (fn.__name__, b)
    for fn in (lib.fcz_violations_dev, lib.fcz_violations):
        assert call(fn, rows=0) == -1                                         # L == 0
    for fn in (lib.fcz_violations_packed_dev, lib.fcz_violations_packed):
        assert call(fn, bound=None) == -1                                     # chains without a row_off
    assert not buf.any()


def test_argument_errors_need_no_device():
    pos, mask, aa = np.zeros((2, 8, 37, 3), F), np.zeros((2, 8, 37), np.uint8), np.zeros((2, 8), np.uint8)
    fn = tensors.violations
    for d in (dict(pos=pos[:, :, :5], mask=mask[:, :, :5]), dict(pos=pos[0, 0], mask=mask[0, 0]), dict(pos=pos, mask=mask[:1]),
              dict(pos=pos, mask=mask, aatype=aa[:, :7]), dict(pos=pos[..., :2], mask=mask), dict(pos=pos[0], mask=mask[0]),
              dict(pos=pos[:, :, :14], mask=mask[:, :, :14])):                 # (the last: atom14 without aatype)
        with pytest.raises(ValueError):
            fn(d)
        with pytest.raises(ValueError):
            fn(**d)
        with pytest.raises(ValueError):
            api.check_violations("x", d)
    with pytest.raises(TypeError):
        fn(dict(pos=pos))
    ok = dict(pos=pos, mask=mask, aatype=aa)
    for kw in (dict(tolerance=-1.0), dict(tolerance=float("nan")), dict(tolerance=float("inf")), dict(tolerance="1.5"), dict(tolerance=True),
               dict(link_factor=-1.0), dict(link_factor=float("nan")), dict(link_factor=1e39), dict(link_factor=None), dict(radii="vdw"),
               dict(radii=np.zeros((20, 37), F)), dict(radii=np.full((21, 37), 8.0, F)), dict(radii=np.full((21, 37), 0.4, F))):
        with pytest.raises(ValueError):
            fn(ok, **kw)
        with pytest.raises(ValueError):
            api.check_violations("x", ok, **kw)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            tensors.decode_tensors([], violations=bad)
    shape, packed, table = api.check_violations("x", ok, tolerance=0, link_factor=3, radii=np.full((21, 37), 1.5))
    assert shape == (2, 8, 37, 3) and not packed and table.dtype == np.float32 and api.check_violations("x", ok)[2] is None
    assert api.check_violations("x", dict(pos=pos[0], mask=mask[0], cu_seqlens=np.zeros(2, np.int32)))[1] is True
    assert api.VIOLATION_TOLERANCE == 1.5 and api.VIOLATION_LINK_FACTOR == 12.0
