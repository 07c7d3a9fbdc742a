"""CPU: the parts of the solvent-accessibility feature that need no device -- the numpy restatement (tests/_sasa.py) on geometry whose
answer is known (one atom, two atoms on an axis, an atom inside an octahedron), its independence of order and layout, the float32
contract against a float64 evaluation without the cull on a chain of the reference's multichain.pdb (PDB 6PP9), the pure-host ABI
(fcz_sasa_pass, fcz_sasa_default_radii, the refusals, the export list), foldcomp.MAX_ASA / sphere_points and the argument errors of
foldcomp.solvent_accessibility, raised before torch or a device is touched."""
import ctypes

import numpy as np
import pytest

import _dense as DN
import _sasa as S
from foldcomp_amd import _lib, api, tensors

F = np.float32
NEW = ("fcz_sasa_pass", "fcz_sasa_default_radii", "fcz_sasa_dev", "fcz_sasa_packed_dev", "fcz_sasa", "fcz_sasa_packed")
AA3 = "ALA ARG ASN ASP CYS GLN GLU GLY HIS ILE LEU LYS MET PHE PRO SER THR TRP TYR VAL".split()
BB4 = S.default_table(4)


def _single_atoms(xyz, radii, probe=S.PROBE):
    """atoms as backbone4 rows that hold slot 0 only, one residue type per atom (at most 21) -> pos, mask, aatype, table"""
    m = len(xyz)
    pos, mask = np.zeros((m, 4, 3), F), np.zeros((m, 4), np.uint8)
    pos[:, 0], mask[:, 0] = np.asarray(xyz, F), 1
    table = np.zeros((21, 4), F)
    table[:m, 0] = radii
    return pos, mask, np.arange(m, dtype=np.uint8), table


# ---- geometry whose answer is known ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 96, 128, 960, 1024])
def test_an_isolated_atom_is_all_surface(P):
    pos, mask, aa, table = _single_atoms([[3.0, -2.0, 40.0]], [1.7])
    counts, sasa, sm = S.sasa_chain(pos, mask, aa, table, S.PROBE, api.sphere_points(P))
    assert counts[0, 0] == P and not counts[0, 1:].any() and sm[0]
    R = F(1.7) + S.PROBE
    exact = 4 * np.pi * float(R) ** 2
    assert abs(float(sasa[0]) - exact) <= exact * 2.0 ** -22        # R * R rounded to float32, the result rounded to float32
    # a far atom changes nothing; an atom with a cleared mask, a NaN coordinate or a zero radius is no atom
    pos, mask, aa, table = _single_atoms([[0, 0, 0], [30, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], [1.7, 1.7, 1.7, 1.7, 0.0])
    mask[2, 0] = 0
    pos[3, 0, 1] = np.nan
    counts, sasa, sm = S.sasa_chain(pos, mask, aa, table, S.PROBE, api.sphere_points(P))
    assert list(counts[:, 0]) == [P, P, 0, 0, 0] and list(sm) == [True, True, False, False, False] and not sasa[2:].any()


@pytest.mark.parametrize("P", [96, 128, 960])
def test_two_atoms_on_the_z_axis_bury_a_cap(P):
    """the spiral's z_k are evenly spaced, so the cap z > z_0 = (Ri^2 + d^2 - Rj^2) / (2 Ri d) holds P (1 - z_0) / 2 points to within one"""
    pts = api.sphere_points(P)
    worst = 0.0
    for ri, rj in ((1.7, 1.7), (1.55, 1.8), (1.8, 1.52)):
        Ri, Rj = float(F(ri) + S.PROBE), float(F(rj) + S.PROBE)
        for d in np.linspace(0.7, 5.9, 53):
            pos, mask, aa, table = _single_atoms([[0, 0, 0], [0, 0, d]], [ri, rj])
            counts = S.counts_chain(pos, mask, aa, table, S.PROBE, pts)
            z0 = (Ri * Ri + float(F(d)) ** 2 - Rj * Rj) / (2 * Ri * float(F(d)))
            expect = P * (1 - min(max(z0, -1.0), 1.0)) / 2
            worst = max(worst, abs((P - int(counts[0, 0])) - expect))
    assert worst <= 1.0, worst


def test_an_atom_inside_an_octahedron_of_larger_neighbours_has_no_surface():
    xyz = [[0, 0, 0]] + [list(1.5 * s * np.eye(3)[k]) for k in range(3) for s in (1, -1)]
    pos, mask, aa, table = _single_atoms(xyz, [1.0] + [2.0] * 6)
    for P in (64, 128, 1000):
        counts, sasa, sm = S.sasa_chain(pos, mask, aa, table, S.PROBE, api.sphere_points(P))
        assert counts[0, 0] == 0 and sasa[0] == 0 and sm[0] and (counts[1:, 0] > 0).all()


# ---- a real chain: order, layout, float32 against float64 ------------------------------------------------------------------
def _chain_of_text(text):
    """ATOM records -> atom37 and atom14 arrays of the chain and aatype; OXT goes to slot 36 of atom37 (the default table leaves it out)"""
    res, key = [], None
    for line in text.splitlines():
        if line.startswith("ATOM"):
            k = (line[21], line[22:27])
            if k != key:
                res.append((line[17:20], {}))
                key = k
            res[-1][1][line[12:16].strip()] = [float(line[30:38]), float(line[38:46]), float(line[46:54])]
    m = len(res)
    out = {A: (np.zeros((m, A, 3), F), np.zeros((m, A), np.uint8)) for A in (37, 14)}
    aa = np.asarray([AA3.index(name) for name, _ in res], np.uint8)
    from foldcomp_amd._aa_tables import ATOM_NAMES
    for r, (name, atoms) in enumerate(res):
        for a, xyz in atoms.items():
            code = ATOM_NAMES.index(a)
            for layout, A in (("atom37", 37), ("atom14", 14)):
                s = DN.expected_slot(layout, int(aa[r]), code)
                if s >= 0:
                    out[A][0][r, s], out[A][1][r, s] = xyz, 1
    return out, aa


@pytest.fixture(scope="module")
def chain(golden):
    z, _ = golden
    views, aa = _chain_of_text(z["pdb:multichainB_1/pdb0"].tobytes().decode("latin-1"))
    assert len(aa) == 77 and views[37][1][:, :36].sum() == views[14][1].sum() > 550
    return views, aa


def test_order_and_layout_do_not_show(chain):
    views, aa = chain
    pts = api.sphere_points(128)
    t37, t14 = S.default_table(37), S.default_table(14)
    c37, s37, m37 = S.sasa_chain(*views[37], aa, t37, S.PROBE, pts)
    c14, s14, m14 = S.sasa_chain(*views[14], aa, t14, S.PROBE, pts)
    assert np.array_equal(S.bits(s37), S.bits(s14)) and np.array_equal(m37, m14) and m37.all()
    for r in range(len(aa)):                                                  # the counts agree through the slot map
        for j, code in enumerate(DN.RES_ATOMS[int(aa[r])]):
            assert c14[r, j] == c37[r, DN.expected_slot("atom37", int(aa[r]), code)]
    assert not c37[:, 36].any()                                              # OXT is left out
    assert (c37 == 0)[views[37][1] != 0].sum() > 100 and s37.max() > 150 and 4000 < s37.sum() < 7000   # a folded domain of 77 residues
    rng = np.random.default_rng(1)
    N = int(views[14][1].sum())
    assert np.array_equal(S.counts_chain(*views[14], aa, t14, S.PROBE, pts, order=rng.permutation(N)), c14)
    perm = rng.permutation(len(aa))                                           # the rows of the chain in another order
    cp, sp, _ = S.sasa_chain(views[14][0][perm], views[14][1][perm], aa[perm], t14, S.PROBE, pts)
    assert np.array_equal(cp, c14[perm]) and np.array_equal(S.bits(sp), S.bits(s14[perm]))
    # aatype NULL is harmless in atom37 (every row of the default table is the same) and row 0 for every row in atom14
    S.same_sasa(S.sasa_chain(*views[37], None, t37, S.PROBE, pts), (c37, s37, m37), "atom37 without aatype")
    assert S.sasa_chain(*views[14], None, t14, S.PROBE, pts)[1].sum() < s14.sum()


@pytest.mark.parametrize("P", [128, 960])
def test_float32_decisions_against_float64_without_the_cull(chain, P):
    """at most 1 in 10 000 (atom, point) decisions may differ; found on this chain: 0 of 78 336 at P = 128, 0 of 587 520 at P = 960"""
    views, aa = chain
    pts, t14 = api.sphere_points(P), S.default_table(14)
    d32, d64 = [], []
    c32 = S.counts_chain(*views[14], aa, t14, S.PROBE, pts, decisions=d32)
    c64 = S.counts_chain(*views[14], aa, t14, S.PROBE, pts, f64=True, decisions=d64)
    d32, d64 = np.asarray(d32), np.asarray(d64)
    differ = int((d32 != d64).sum())
    print(f"P = {P}: {differ} of {d32.size} decisions differ")
    assert d32.size == int(views[14][1].sum()) * P and differ * 10000 <= d32.size, (differ, d32.size)
    a32 = S.area_rows(c32, *views[14], aa, t14, S.PROBE, P)[0].astype(np.float64)
    a64 = S.area_rows(c64, *views[14], aa, t14, S.PROBE, P)[0].astype(np.float64)
    # a decision moves one point of at most 4 pi 3.2^2 / P: the chain's area and every residue's follow
    assert abs(a32.sum() - a64.sum()) <= differ * 4 * np.pi * 3.2 ** 2 / P + 1e-3 and np.abs(a32 - a64).max() <= differ * 4 * np.pi * 3.2 ** 2 / P + 1e-3


# ---- forms, ABI, arguments -------------------------------------------------------------------------------------------------
def test_restatement_forms_agree():
    rng = np.random.default_rng(4)
    lens = [0, 1, 5, 20]
    L = 22
    pos, mask = np.zeros((4, L, 4, 3), F), (rng.random((4, L, 4)) < 0.9).astype(np.uint8)
    for e, m in enumerate(lens):
        pos[e, :m] = S.globule(rng, m) if m else 0
        pos[e, m:] = rng.normal(size=(L - m, 4, 3))                           # behind length: never read
    aa = rng.integers(0, 25, size=(4, L)).astype(np.uint8)
    pts = api.sphere_points(65)
    pad = S.sasa(pos, mask, aa, np.asarray(lens), BB4, S.PROBE, pts)
    row_off = np.concatenate([[0], np.cumsum(lens)])
    cat = lambda a: np.concatenate([a[e, :m] for e, m in enumerate(lens)])
    S.same_sasa(S.sasa(cat(pos), cat(mask), cat(aa), row_off, BB4, S.PROBE, pts, packed=True), [cat(a) for a in pad], "packed")
    for a in pad:
        assert not any(a[e, m:].any() for e, m in enumerate(lens))
    assert (pad[0][3, :20] > 0).sum() > 30 and (pad[0][3, :20] < 65).sum() > 30


def test_default_radii_and_the_pass():
    lib = _lib.load()
    assert set(NEW) <= set(_lib.EXPORTS) and lib.fcz_sasa_pass() > 0
    for layout, A in ((0, 37), (1, 14), (2, 4)):
        out = np.full((21, A), np.nan, F)
        assert lib.fcz_sasa_default_radii(layout, out.ctypes.data) == 0
        assert np.array_equal(out.view(np.uint32), S.default_table(A).view(np.uint32)), layout
    t = S.default_table(14)
    assert t[0, 5] == 0 and t[4, 5] == F(1.8) and t[12, 6] == F(1.8) and t[17].all() and list(t[20]) == [F(1.55), F(1.7), F(1.7)] + [0] * 11
    assert (S.default_table(37)[:, 36] == 0).all() and (S.default_table(37)[:, :36] > 0).all()
    buf = np.zeros(21 * 37, F)
    assert lib.fcz_sasa_default_radii(3, buf.ctypes.data) == -1 and lib.fcz_sasa_default_radii(-1, buf.ctypes.data) == -1 and not buf.any()
    assert lib.fcz_sasa_default_radii(0, None) == -1


def test_refusals_need_no_device():
    lib = _lib.load()
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    fake = ctypes.c_void_p(p)                                                  # refused before anything is touched (the ctx is never read)
    pts = api.sphere_points(8)
    u = pts.ctypes.data
    tab = S.default_table(37)
    ok = dict(ctx=fake, pos=p, mask=p, aa=p, bound=p, n=1, rows=4, layout=0, table=None, probe=1.4, points=u, P=8, o0=p, o1=p, o2=p)
    big, nan_tab, neg = tab.copy(), tab.copy(), tab.copy()
    big[3, 5], nan_tab[20, 0], neg[0, 0] = 6.7, np.nan, -1.0                 # R = 8.1, NaN, 0.4
    bad = [dict(ctx=None), dict(pos=None), dict(mask=None), dict(points=None), dict(o0=None), dict(o1=None), dict(o2=None), dict(layout=3), dict(layout=-1),
           dict(rows=2 ** 31), dict(P=0), dict(P=1025), dict(probe=float("nan")), dict(probe=float("inf")), dict(probe=-0.1),
           dict(table=big.ctypes.data), dict(table=nan_tab.ctypes.data), dict(table=neg.ctypes.data), dict(probe=7.0), dict(layout=1, aa=None)]
    for fn in (lib.fcz_sasa_dev, lib.fcz_sasa_packed_dev, lib.fcz_sasa, lib.fcz_sasa_packed):
        for b in bad:
            assert fn(*dict(ok, **b).values()) == -1, (fn.__name__, b)
    for fn in (lib.fcz_sasa_dev, lib.fcz_sasa):
        assert fn(*dict(ok, rows=0).values()) == -1                           # L == 0
    for fn in (lib.fcz_sasa_packed_dev, lib.fcz_sasa_packed):
        assert fn(*dict(ok, bound=None).values()) == -1                       # chains without a row_off
    assert not buf.any()


def test_max_asa_and_sphere_points():
    import foldcomp
    import foldcomp_amd
    assert foldcomp.solvent_accessibility is foldcomp_amd.solvent_accessibility is tensors.solvent_accessibility
    assert foldcomp.sphere_points is api.sphere_points and foldcomp.MAX_ASA is api.MAX_ASA
    tien = dict(A=129, R=274, N=195, D=193, C=167, Q=225, E=223, G=104, H=224, I=197, L=201, K=236, M=224, F=240, P=159, S=155, T=172, W=285, Y=263, V=174)
    assert foldcomp.MAX_ASA.shape == (21,) and foldcomp.MAX_ASA.dtype == np.float32
    assert [float(v) for v in foldcomp.MAX_ASA] == [float(tien[c]) for c in "ARNDCQEGHILKMFPSTWYV"] + [0.0]
    for n in (1, 96, 128, 1024):
        pts = foldcomp.sphere_points(n)
        assert pts.shape == (n, 3) and pts.dtype == np.float32
        k = np.arange(n)
        assert np.array_equal(pts[:, 2], (1 - (2 * k + 1) / n).astype(F))
        assert np.abs(np.linalg.norm(pts.astype(np.float64), axis=1) - 1).max() < 1e-6
        phi = k * (np.pi * (3 - np.sqrt(5)))
        assert np.allclose(pts[:, 0], np.sqrt(1 - pts[:, 2].astype(np.float64) ** 2) * np.cos(phi), atol=1e-6)
    for bad in (0, 1025, -3):
        with pytest.raises(ValueError):
            foldcomp.sphere_points(bad)


def test_argument_errors_need_no_device():
    pos, mask, aa = np.zeros((2, 8, 37, 3), F), np.zeros((2, 8, 37), np.uint8), np.zeros((2, 8), np.uint8)
    fn = tensors.solvent_accessibility
    for d in (dict(pos=pos[:, :, :5], mask=mask[:, :, :5]), dict(pos=pos[0, 0], mask=mask[0, 0]), dict(pos=pos, mask=mask[:1]),
              dict(pos=pos, mask=mask, aatype=aa[:, :7]), dict(pos=pos[..., :2], mask=mask), dict(pos=pos[0], mask=mask[0]),
              dict(pos=pos[:, :, :14], mask=mask[:, :, :14])):                 # (the last: atom14 without aatype)
        with pytest.raises(ValueError):
            fn(d)
        with pytest.raises(ValueError):
            fn(**d)
    with pytest.raises(TypeError):
        fn(dict(pos=pos))
    ok = dict(pos=pos, mask=mask, aatype=aa)
    for kw in (dict(probe=-1.0), dict(probe=float("nan")), dict(n_points=0), dict(n_points=1025), dict(points=np.zeros((4, 2), F)),
               dict(points=np.zeros((1025, 3), F)), dict(radii="vdw"), dict(radii=np.zeros((20, 37), F)), dict(radii=np.full((21, 37), 7.0, F)),
               dict(radii=np.full((21, 37), 1.7, F), probe=0.0001 - 1.3)):
        with pytest.raises(ValueError):
            fn(ok, **kw)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            tensors.decode_tensors([], sasa=bad)
    shape, packed, pts, table = api.check_sasa("x", ok, points=np.eye(3), radii=np.full((21, 37), 1.5))
    assert shape == (2, 8, 37, 3) and not packed and pts.dtype == np.float32 and pts.shape == (3, 3) and table.dtype == np.float32
    assert api.check_sasa("x", dict(pos=pos[0], mask=mask[0], cu_seqlens=np.zeros(2, np.int32)))[1:] [0] is True
