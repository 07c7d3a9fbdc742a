"""CPU: the parts of the DSSP feature that need no device -- the numpy restatement (tests/_dssp.py) on ideal backbones built with NeRF,
its label rules on hand-written acceptor tables, the HELIX / SHEET records of the reference's own multichain.pdb (PDB 6PP9) as an
outside check, the padded against the packed form, the pure-host ABI (fcz_hbond_pass, the refusals, the export list) and the
argument errors of foldcomp.backbone_hbonds / secondary_structure, raised before torch or a device is touched."""
import ctypes
import os

import numpy as np
import pytest

import _dssp as D
from foldcomp_amd import _lib, api, tensors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fcz_hbond_pass", "fcz_hbond_dev", "fcz_hbond_packed_dev", "fcz_dssp_labels_dev", "fcz_dssp_labels_packed_dev", "fcz_dssp", "fcz_dssp_packed")
F = np.float32
AA3 = "ALA ARG ASN ASP CYS GLN GLU GLY HIS ILE LEU LYS MET PHE PRO SER THR TRP TYR VAL".split()


# ---- ideal geometry --------------------------------------------------------------------------------------------------------
ideal_backbone = D.ideal_backbone


def _ss(pos, mask, aatype=None):
    t = D.hbond_chain(pos, mask, aatype)
    return D.text(D.labels_chain(pos, mask, t[0], t[1])[0]), t


def test_ideal_alpha_helix_is_h():
    s, t = _ss(*ideal_backbone(-57, -47, 20))
    assert s == "-" + "H" * 18 + "-"
    # the i -> i - 4 bonds, each well under -0.5 and none at the floor
    assert [int(a) for a in t[0][4:, 0]] == list(range(0, 16)) and (t[1][4:, 0] < F(-1.0)).all() and (t[1][4:, 0] > F(-9.9)).all()
    assert [int(a) for a in t[2][:16, 0]] == list(range(4, 20))            # the donor table is the same bonds seen from the C=O
    assert np.array_equal(t[1][4:, 0].view(np.uint32), t[3][:16, 0].view(np.uint32))


def test_ideal_310_helix_is_g_and_pi_helix_is_i():
    s, _ = _ss(*ideal_backbone(-49, -26, 20))
    assert set(s[1:-1]) == {"G"} and s[0] == s[-1] == "-", s
    s, _ = _ss(*ideal_backbone(-57, -70, 20))
    assert set(s[1:-1]) == {"I"} and s[0] == s[-1] == "-", s


def test_an_extended_strand_alone_is_no_sheet():
    s, t = _ss(*ideal_backbone(-120, 130, 20))
    assert not set(s) & set("EBHGI"), s
    assert not (t[1] < F(-0.5)).any()


def test_a_proline_removes_exactly_the_bonds_its_amide_would_donate():
    pos, mask = ideal_backbone(-57, -47, 20)
    aa = np.zeros(20, np.uint8)
    _, free = _ss(pos, mask, aa)
    aa[10] = D.PRO
    s, t = _ss(pos, mask, aa)
    assert (t[0][10] == -1).all() and not t[1][10].any() and (free[0][10] >= 0).any()
    keep = np.arange(20) != 10
    D.same_tables([x[keep] for x in t[:2]], [x[keep] for x in free[:2]], "the other donors")
    E0, E1 = D.energy_matrix(D.Chain(pos, mask, np.zeros(20, np.uint8))), D.energy_matrix(D.Chain(pos, mask, aa))
    assert np.isfinite(E0[10]).any() and np.isinf(E1[10]).all()              # row 10 donates nothing any more ...
    assert np.array_equal(E0[keep].view(np.uint32), E1[keep].view(np.uint32))   # ... and every other energy is what it was
    assert not (t[2] == 10).any() and (free[2] == 10).any()
    assert s == "-" + "H" * 18 + "-"                                          # one missing turn: its neighbours still cover every row


# ---- label rules on hand-written acceptor tables ---------------------------------------------------------------------------
def straight_chain(m, breaks=(), zigzag=False):
    """backbone4 rows along x, 3.8 apart, C - N(+1) 1.4; a break behind row r moves everything behind it 10 further; zigzag: every CA
    bends by more than 70 degrees"""
    pos = np.zeros((m, 4, 3), F)
    x = 3.8 * np.arange(m) + 10.0 * np.cumsum([0] + [1 if r in breaks else 0 for r in range(m - 1)])
    pos[:, :, 0] = x[:, None]
    pos[:, 0, 0] -= 1.2; pos[:, 2, 0] += 1.2; pos[:, 3, 0] += 1.2
    pos[:, 3, 1] = 1.2
    if zigzag:
        pos[:, 1, 1] = 30.0 * (np.arange(m) // 2 % 2)
    return pos, np.ones((m, 4), np.uint8)


def table(m, bonds, energy=-2.0):
    """(donor, acceptor) pairs -> acc_index [m, 2], acc_energy [m, 2], filled in the order given"""
    ai, ae = np.full((m, 2), -1, np.int32), np.zeros((m, 2), F)
    for d, a in bonds:
        s = int(ai[d, 0] >= 0)
        assert ai[d, s] < 0, "a row has two acceptors"
        ai[d, s], ae[d, s] = a, energy
    return ai, ae


def label(m, bonds, energy=-2.0, **geometry):
    pos, mask = straight_chain(m, **geometry)
    return D.text(D.labels_chain(pos, mask, *table(m, bonds, energy))[0])


def _expect(m, marks):
    s = ["-"] * m
    for rows, c in marks:
        for r in rows:
            s[r] = c
    return "".join(s)


def test_a_single_bridge_is_b_and_two_in_a_row_are_e():
    assert label(30, [(5, 15), (15, 5)]) == _expect(30, [((5, 15), "B")])
    assert label(30, [(5, 15), (15, 5), (6, 14), (14, 6)]) == _expect(30, [((5, 6, 14, 15), "E")])
    assert label(30, [(5, 15), (15, 5)], energy=-0.5) == "-" * 30          # a bond is E < -0.5
    assert label(30, [(5, 7), (7, 5)]) == "-" * 30                          # j >= i + 3
    assert label(30, [(5, 8), (8, 5)]) == _expect(30, [((5, 8), "B"), ((6, 7), "T")])   # (bond(8, 5) is a 3-turn as well)
    assert label(30, [(0, 15), (15, 0)]) == "-" * 30 and label(30, [(5, 29), (29, 5)]) == "-" * 30   # the flanking rows must exist


def test_parallel_and_antiparallel_ladders_are_e():
    par = [(6, 15), (15, 4), (7, 16), (16, 5)]                                # bond(i + 1, j) and bond(j, i - 1) for (5, 15), (6, 16)
    assert label(30, par) == _expect(30, [((5, 6, 15, 16), "E")])
    par2 = [(16, 5), (5, 14), (17, 6), (6, 15)]                               # bond(j + 1, i) and bond(i, j - 1)
    assert label(30, par2) == _expect(30, [((5, 6, 15, 16), "E")])
    anti = [(6, 14), (16, 4), (7, 13), (15, 5)]                               # bond(i + 1, j - 1) and bond(j + 1, i - 1) for (5, 15), (6, 14)
    assert label(30, anti) == _expect(30, [((5, 6, 14, 15), "E")])
    assert label(30, par[:2]) == _expect(30, [((5, 15), "B")]) and label(30, anti[:2]) == _expect(30, [((5, 15), "B")])
    assert label(30, par, breaks=(15,)) == _expect(30, [((5, 16), "-")])     # a break beside a strand: neither bridge stands


def test_a_bulge_links_with_gaps_1_4_and_not_with_3_3():
    linked = [(5, 20), (20, 5), (6, 16), (16, 6)]                             # antiparallel (5, 20) and (6, 16): gi = 1, gj = 4
    assert label(30, linked) == _expect(30, [((5, 6), "E"), (range(16, 21), "E")])
    apart = [(5, 20), (20, 5), (8, 17), (17, 8)]                              # gi = 3, gj = 3
    assert label(30, apart) == _expect(30, [((5, 8, 17, 20), "B")])
    assert label(30, linked, breaks=(18,)) == _expect(30, [((5, 20, 6, 16), "B")])   # a break across the gap
    par = [(6, 15), (15, 4), (10, 16), (16, 8)]                               # parallel (5, 15) and (9, 16): gi = 4, gj = 1
    assert label(30, par) == _expect(30, [(range(5, 10), "E"), ((15, 16), "E")])
    edge = [(6, 15), (15, 4), (11, 17), (17, 9)]                              # parallel (5, 15) and (10, 17): gi = 5, gj = 2
    assert label(30, edge) == _expect(30, [(range(5, 11), "E"), ((15, 16, 17), "E")])
    far = [(6, 15), (15, 4), (12, 17), (17, 10)]                              # (5, 15) and (11, 17): gi = 6
    assert label(30, far) == _expect(30, [((5, 15, 11, 17), "B")])
    wide = [(6, 15), (15, 4), (9, 19), (19, 7)]                               # (5, 15) and (8, 19): gi = 3, gj = 4
    assert label(30, wide) == _expect(30, [((5, 15, 8, 19), "B")])


HELIX = [(7, 3), (8, 4), (9, 5)]                                              # turn_4 at 3, 4, 5: H on 4 .. 8


def test_priorities():
    assert label(30, HELIX) == _expect(30, [(range(4, 9), "H")])
    # E does not overwrite H: the ladder (6, 20), (7, 19) leaves rows 6 and 7 H
    assert label(30, HELIX + [(6, 20), (20, 6), (7, 19), (19, 7)]) == _expect(30, [(range(4, 9), "H"), ((19, 20), "E")])
    # G is blocked by a neighbouring H: turn_3 at 7 and 8 would make 8 .. 10 G, but 8 is H; 9 and 10 are left to T
    assert label(30, HELIX + [(10, 7), (11, 8)]) == _expect(30, [(range(4, 9), "H"), ((9, 10), "T")])
    assert label(30, [(10, 7), (11, 8)]) == _expect(30, [((8, 9, 10), "G")])
    assert label(30, [(12, 7), (13, 8)]) == _expect(30, [(range(8, 13), "I")])
    # I is blocked by G
    assert label(30, [(12, 7), (13, 8), (13, 10), (14, 11)]) == _expect(30, [(range(8, 11), "T"), (range(11, 14), "G")])
    # one turn alone: T inside it
    assert label(30, [(7, 3)]) == _expect(30, [((4, 5, 6), "T")]) and label(30, [(6, 3)]) == _expect(30, [((4, 5), "T")])


def test_a_turn_with_a_break_in_its_span_is_no_turn():
    assert label(30, HELIX, breaks=(5,)) == "-" * 30                          # behind row 5: inside 3 .. 7, 4 .. 8 and 5 .. 9
    assert label(30, HELIX, breaks=(3,)) == _expect(30, [(range(5, 9), "H")])  # inside 3 .. 7 only: turn_4(4) and turn_4(5) stand
    assert label(30, HELIX[:2], breaks=(3,)) == _expect(30, [((5, 6, 7), "T")])
    assert label(30, HELIX, breaks=(2,)) == label(30, HELIX) == label(30, HELIX, breaks=(9,))   # in front of the first turn, behind the last


def test_t_and_s_are_written_on_unlabelled_rows_only():
    s = label(30, HELIX + [(20, 14), (14, 20)], zigzag=True)
    assert s == _expect(30, [(range(2, 28), "S"), (range(4, 9), "H"), ((14, 20), "B")])
    s = label(30, [(7, 3), (20, 14), (14, 20)], zigzag=True)
    assert s == _expect(30, [(range(2, 28), "S"), ((4, 5, 6), "T"), ((14, 20), "B")])
    assert label(30, [], zigzag=True, breaks=(10,)) == _expect(30, [(range(2, 9), "S"), (range(13, 28), "S")])
    assert label(30, []) == "-" * 30


def test_a_third_best_bond_is_not_in_the_table():
    E = np.full((30, 30), np.inf, F)
    E[5, 15], E[15, 5] = -2.0, -2.0
    full = D.labels_chain(*straight_chain(30), *D._best_two(E))[0]
    assert D.text(full) == _expect(30, [((5, 15), "B")])
    E[5, 25], E[5, 26] = -3.0, -2.5                                            # two better acceptors push 15 out of row 5's table
    ai, ae = D._best_two(E)
    assert list(ai[5]) == [25, 26] and D.text(D.labels_chain(*straight_chain(30), ai, ae)[0]) == "-" * 30
    E[5, 26] = -2.0                                                            # a tie: the lower row wins, 15 is back
    ai, ae = D._best_two(E)
    assert list(ai[5]) == [25, 15] and D.text(D.labels_chain(*straight_chain(30), ai, ae)[0]) == D.text(full)
    E[5, 10] = -2.0                                                            # and out again
    assert list(D._best_two(E)[0][5]) == [25, 10]


# ---- the reference's multichain.pdb against its own HELIX / SHEET records --------------------------------------------------
def _backbone_of_text(text):
    res, key = [], None
    for line in text.splitlines():
        if line.startswith("ATOM"):
            k = (line[21], line[22:27])
            if k != key:
                res.append((line[17:20], {}))
                key = k
            res[-1][1][line[12:16].strip()] = [float(line[30:38]), float(line[38:46]), float(line[46:54])]
    m = len(res)
    pos, mask, aa = np.zeros((m, 4, 3), F), np.zeros((m, 4), np.uint8), np.full(m, 20, np.uint8)
    for r, (name, atoms) in enumerate(res):
        aa[r] = AA3.index(name) if name in AA3 else 20
        for s, a in enumerate(("N", "CA", "C", "O")):
            if a in atoms:
                pos[r, s], mask[r, s] = atoms[a], 1
    return pos, mask, aa


def _author_numbers(lines, chain):
    """per chain, the residues that have N, CA and C, in file order: the rows of the records"""
    out, key = [], None
    for line in lines:
        if line.startswith("ATOM") and line[21] == chain:
            if line[22:27] != key:
                out.append([int(line[22:26]), set()])
                key = line[22:27]
            out[-1][1].add(line[12:16].strip())
    return [n for n, atoms in out if {"N", "CA", "C"} <= atoms]


@pytest.mark.parametrize("chain,names,rows", [("A", ["pdb:multichainA"], [276]), ("B", ["pdb:multichainB_0", "pdb:multichainB_1"], [236, 77])])
def test_the_multichain_file_agrees_with_its_own_helix_and_sheet_records(golden, chain, names, rows):
    z, _ = golden
    lines = np.load(os.path.join(ROOT, "tests", "golden", "reference_ingest.npz"))["file:multichain.pdb"].tobytes().decode("latin-1").splitlines()
    author = _author_numbers(lines, chain)
    parts = [_backbone_of_text(z[f"{n}/pdb0"].tobytes().decode("latin-1")) for n in names]
    assert [len(p[0]) for p in parts] == rows and len(author) == sum(rows)
    ss, o = {}, 0
    for pos, mask, aa in parts:
        t = D.hbond_chain(pos, mask, aa)
        s = D.labels_chain(pos, mask, t[0], t[1])[0]
        ss.update({author[o + r]: D.SS[s[r]] for r in range(len(pos))})
        o += len(pos)
    helix = [r for l in lines if l.startswith("HELIX") and l[19] == chain and int(l[38:40]) == 1 for r in range(int(l[21:25]) + 1, int(l[33:37]))]
    sheet = [r for l in lines if l.startswith("SHEET") and l[21] == chain for r in range(int(l[22:26]), int(l[33:37]) + 1)]
    assert (len(helix), len(sheet)) == {"A": (94, 44), "B": (132, 43)}[chain]
    assert [r for r in helix if ss.get(r) != "H"] == []
    assert [r for r in sheet if ss.get(r) not in ("E", "B")] == []


# ---- forms, ABI, arguments -------------------------------------------------------------------------------------------------
def test_restatement_forms_agree():
    lens = [0, 1, 4, 5, 20, 33]
    L = 36
    pos, mask, aa = np.zeros((len(lens), L, 4, 3), F), np.zeros((len(lens), L, 4), np.uint8), np.zeros((len(lens), L), np.uint8)
    rng = np.random.default_rng(3)
    for e, m in enumerate(lens):
        if m:
            pos[e, :m], mask[e, :m] = ideal_backbone(-57, -47, m) if e % 2 else ideal_backbone(-120, 130, m)
        pos[e, m:] = rng.normal(size=(L - m, 4, 3))                       # behind length: never read
        mask[e, m:] = 1
    aa[5, 12] = D.PRO
    pad = D.hbonds(pos, mask, aa, np.asarray(lens))
    row_off = np.concatenate([[0], np.cumsum(lens)])
    cat = lambda a: np.concatenate([a[e, :m] for e, m in enumerate(lens)])
    pk = D.hbonds(cat(pos), cat(mask), cat(aa), row_off, packed=True)
    shifted = [np.concatenate([np.where(a[e, :m] >= 0, a[e, :m] + row_off[e], -1) if a.dtype == np.int32 else a[e, :m] for e, m in enumerate(lens)]) for a in pad]
    D.same_tables(pk, [s.astype(p.dtype) for s, p in zip(shifted, pk)], "packed")
    for a in pad:
        for e, m in enumerate(lens):
            assert (a[e, m:] == (-1 if a.dtype == np.int32 else 0)).all()
    lp = D.labels(pos, mask, np.asarray(lens), pad[0], pad[1])
    lk = D.labels(cat(pos), cat(mask), row_off, pk[0], pk[1], packed=True)
    D.same_labels(lk, [cat(a) for a in lp], "packed labels")
    assert D.text(lp[0][5, :33]).count("H") > 20 and not lp[0][5, 33:].any() and not lp[1][5, 33:].any() and lp[1][5, :33].all()


def test_pure_host_abi():
    lib = _lib.load()
    assert set(NEW) <= set(_lib.EXPORTS)
    assert lib.fcz_hbond_pass() > 0
    buf = np.zeros(256, np.uint8)
    p = buf.ctypes.data
    fake = ctypes.c_void_p(p)                                                  # refused before anything is touched (the ctx is never read)
    four = (lib.fcz_hbond_dev, lib.fcz_hbond_packed_dev, lib.fcz_dssp_labels_dev, lib.fcz_dssp_labels_packed_dev)
    for fn in four:
        assert fn(None, p, p, p, p, 1, 4, 0, p, p, p, p) == -1
        assert fn(fake, None, p, p, p, 1, 4, 0, p, p, p, p) == -1 and fn(fake, p, None, p, p, 1, 4, 0, p, p, p, p) == -1
        assert fn(fake, p, p, p, p, 1, 4, 3, p, p, p, p) == -1 and fn(fake, p, p, p, p, 1, 4, -1, p, p, p, p) == -1
        assert fn(fake, p, p, p, p, 1, 2 ** 31, 0, p, p, p, p) == -1
        for k in range(4):
            out = [p] * 4
            out[k] = None
            assert fn(fake, p, p, p, p, 1, 4, 0, *out) == -1
    for fn in (lib.fcz_dssp, lib.fcz_dssp_packed):
        assert fn(None, p, p, p, p, 1, 4, 0, p, p, p, p, p, p) == -1 and fn(fake, p, p, p, p, 1, 4, 5, p, p, p, p, p, p) == -1
        assert fn(fake, p, p, p, p, 1, 2 ** 31, 0, p, p, p, p, p, p) == -1
        for k in range(6):
            out = [p] * 6
            out[k] = None
            assert fn(fake, p, p, p, p, 1, 4, 0, *out) == -1
    for fn in (lib.fcz_hbond_dev, lib.fcz_dssp_labels_dev):
        assert fn(fake, p, p, p, p, 1, 0, 0, p, p, p, p) == -1                # L == 0
    for fn in (lib.fcz_hbond_packed_dev, lib.fcz_dssp_labels_packed_dev):
        assert fn(fake, p, p, p, None, 1, 4, 0, p, p, p, p) == -1             # chains without a row_off
    assert lib.fcz_dssp(fake, p, p, p, p, 1, 0, 0, p, p, p, p, p, p) == -1 and lib.fcz_dssp_packed(fake, p, p, p, None, 1, 4, 0, p, p, p, p, p, p) == -1
    assert not buf.any()


def test_argument_errors_need_no_device():
    pos, mask, aa = np.zeros((2, 8, 37, 3), F), np.zeros((2, 8, 37), np.uint8), np.zeros((2, 8), np.uint8)
    tab = dict(hbond_acc_index=np.zeros((2, 8, 2), np.int32), hbond_acc_energy=np.zeros((2, 8, 2), F))
    for fn in (tensors.backbone_hbonds, tensors.secondary_structure):
        for d in (dict(pos=pos[:, :, :5], mask=mask[:, :, :5]), dict(pos=pos[0, 0], mask=mask[0, 0]), dict(pos=pos, mask=mask[:1]),
                  dict(pos=pos, mask=mask, aatype=aa[:, :7]), dict(pos=pos[..., :2], mask=mask), dict(pos=pos[0], mask=mask[0])):
            with pytest.raises(ValueError):
                fn(d)
            with pytest.raises(ValueError):
                fn(**d)
        with pytest.raises(TypeError):
            fn(dict(pos=pos))
        with pytest.raises(TypeError):
            fn(mask=mask)
    with pytest.raises(ValueError):
        tensors.secondary_structure(dict(pos=pos, mask=mask), hbonds=dict(tab, hbond_acc_index=tab["hbond_acc_index"][:1]))
    with pytest.raises(ValueError):
        tensors.secondary_structure(dict(pos=pos, mask=mask), hbonds=dict(tab, hbond_acc_energy=np.zeros((2, 8, 3), F)))
    with pytest.raises(TypeError):
        tensors.secondary_structure(dict(pos=pos, mask=mask), hbonds=dict(hbond_acc_index=tab["hbond_acc_index"]))
    with pytest.raises(TypeError):
        tensors.secondary_structure(dict(pos=pos, mask=mask), hbonds=tab["hbond_acc_index"])
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            tensors.decode_tensors([], secondary_structure=bad)
    assert api.check_dssp("x", dict(pos=pos, mask=mask, aatype=aa), tab) == ((2, 8, 37, 3), False)
    assert api.check_dssp("x", dict(pos=pos[0], mask=mask[0], cu_seqlens=np.zeros(2, np.int32))) == ((8, 37, 3), True)


def test_constants_and_re_exports():
    import foldcomp
    import foldcomp_amd
    assert foldcomp.secondary_structure is foldcomp_amd.secondary_structure is tensors.secondary_structure
    assert foldcomp.backbone_hbonds is foldcomp_amd.backbone_hbonds is tensors.backbone_hbonds
    assert foldcomp.SS_CLASSES == ("-", "H", "B", "E", "G", "I", "T", "S") == tuple(D.SS)
    t = foldcomp.SS3_OF_SS8
    assert t.dtype == np.uint8 and t.shape == (8,)
    assert [int(t[foldcomp.SS_CLASSES.index(c)]) for c in "HGIEB-TS"] == [0, 0, 0, 1, 1, 2, 2, 2]
