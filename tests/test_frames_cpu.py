"""CPU: the parts of the rigid-frame feature that need no device -- the pure-host tables (fcz_frame_atom, fcz_frame_ambiguous,
fcz_frames_width), the meaning of the numpy restatement (tests/_frames.py) on the goldens' reference-decoded coordinates, its
degenerate cases, and the argument errors of foldcomp.rigid_frames / decode_tensors(frames=) / tensor_batches(frames=), raised
before torch or a device is touched."""
import ctypes
import os

import numpy as np
import pytest

import _angles as A
import _dense as D
import _frames as F
from _cases import compress_cases, db_cases
from foldcomp_amd import _lib, api, tensors
from foldcomp_amd._aa_tables import RES3

NEW = ("fcz_frames_width", "fcz_frame_atom", "fcz_frame_ambiguous", "fcz_frames_dev", "fcz_frames")
N_, CA, C, O, CB = 0, 1, 2, 3, 4                                     # atom codes (aa_tables: N CA C O CB ...)

# The largest deviation on the 56 golden records (float32 restatement against a float64 evaluation of the same definition on the
# same float32 coordinates; the local coordinates of the defining atoms, R^T R - I, det - 1 and rot itself), measured on the CPU:
# 4.562e-07 (test_meaning_on_the_goldens prints the figure). The bound is 4 x that: float32 Gram-Schmidt at protein bond angles,
# and nothing in the project fixes the tolerance in advance.
MEASURED = 4.562e-07
BOUND = 4 * MEASURED


# ---- tables ---------------------------------------------------------------------------------------------------------------------

def test_tables():
    lib = _lib.load()
    for rc in range(24):
        assert [lib.fcz_frame_atom(rc, 0, j) for j in range(3)] == [C, CA, N_], rc      # x axis CA -> C, origin CA, N fixes the plane
        assert [lib.fcz_frame_atom(rc, 3, j) for j in range(3)] == [CA, C, O], rc       # x axis CA -> C, origin C, O fixes the plane
        for g in (1, 2):
            assert [lib.fcz_frame_atom(rc, g, j) for j in range(3)] == [-1] * 3
        chain = [N_, CA, CB] + [lib.fcz_chi_atom(rc, k) for k in range(4)]
        for k in range(4):
            got = [lib.fcz_frame_atom(rc, 4 + k, j) for j in range(3)]
            if lib.fcz_chi_atom(rc, k) >= 0:
                assert got == chain[k + 1:k + 4] and min(got) >= 0, (rc, k)               # the last three atoms of the chi quadruple
            else:
                assert got == [-1] * 3, (rc, k)
    amb = {(RES3[rc], g) for rc in range(24) for g in range(8) if lib.fcz_frame_ambiguous(rc, g)}
    assert amb == {("ASP", 5), ("GLU", 6), ("PHE", 5), ("TYR", 5)}
    assert [lib.fcz_frames_width(g) for g in (0, 1, 2, -1)] == [1, 8, -1, -1]
    for a in ((-1, 0, 0), (24, 0, 0), (0, -1, 0), (0, 8, 0), (0, 0, -1), (0, 0, 3)):
        assert lib.fcz_frame_atom(*a) == -1, a
    assert lib.fcz_frame_ambiguous(-1, 5) == 0 and lib.fcz_frame_ambiguous(24, 5) == 0 and lib.fcz_frame_ambiguous(3, 8) == 0
    assert set(NEW) <= set(_lib.EXPORTS)
    for name in NEW:
        assert getattr(lib, name).argtypes is not None
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__))), "include", "fcz_hip.h")).read()
    for name in NEW:
        assert f" {name}(" in header, name


def test_python_tables():
    import foldcomp_amd as foldcomp
    assert foldcomp.FRAME_GROUPS == ("backbone", "unused_1", "unused_2", "psi", "chi1", "chi2", "chi3", "chi4")
    t = foldcomp.frame_ambiguous()
    assert t.shape == (21, 8) and t.dtype == np.bool_
    assert sorted(map(tuple, np.argwhere(t))) == [(3, 5), (6, 6), (13, 5), (18, 5)] and not t[20].any()
    # backbone4 has slots for groups 0 and 3 only; the chi slots of atom37 are the names' positions in the atom37 order
    assert (F.slot_table(2)[:, [0, 3]] >= 0).all() and (F.slot_table(2)[:, [1, 2, 4, 5, 6, 7]] == -1).all()
    assert F.slot_table(0)[1, 7].tolist() == [D.ATOM37.index(x) for x in ("CD", "NE", "CZ")]      # ARG chi4
    assert F.slot_table(1)[1, 7].tolist() == [6, 7, 8] and (F.slot_table(0)[20, 4:] == -1).all()


# ---- meaning, on the goldens ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gold37(golden):
    """the 56 golden records' reference-decoded coordinates as packed atom37 rows, with the chi columns of the angle restatement"""
    z, index = golden
    names = compress_cases(index) + db_cases(index)
    assert len(names) == 56
    pos, mask, aatype, chi, owner, codes = [], [], [], [], [], []
    for i, nm in enumerate(names):
        fcz = z[f"{nm}/fcz"].tobytes()
        seq, first, has_oxt = D.record_fields(fcz)
        d = D.dense_expected(z[f"{nm}/xyz0"], seq, first, has_oxt, "atom37", len(seq))
        pos.append(d["pos"]); mask.append(d["mask"]); aatype.append(d["aatype"]); owner += [i] * len(seq); codes += seq
        chi.append(A.entry_expected(fcz)[1][:, 6:10])
    return dict(names=names, pos=np.concatenate(pos), mask=np.concatenate(mask), aatype=np.concatenate(aatype), chi=np.concatenate(chi),
                owner=np.asarray(owner), codes=np.asarray(codes))


def test_not_vacuous_on_the_goldens(gold37):
    g = gold37
    R = len(g["pos"])
    rot, trans, fm, _ = F.frames_rows(g["pos"], g["mask"], g["aatype"], np.ones(R, bool), 0, 1)
    assert R > 5000 and fm[:, 0].all()                               # every row has its backbone frame
    # psi needs the O: the decoder gives a residue of code 23 (UNK) N, CA, C only, so exactly those rows have no group 3.
    # They are rows of two golden records, named here rather than loosening the rule:
    no_psi = fm[:, 3] == 0
    assert np.array_equal(no_psi, g["codes"] == 23)
    assert sorted({g["names"][i] for i in g["owner"][no_psi]}) == sorted({g["names"][i] for i in g["owner"][g["codes"] == 23]})
    assert 0 < no_psi.sum() < 100 and len(set(g["owner"][no_psi])) == 2
    assert not fm[:, 1:3].any()
    assert np.array_equal(fm[:, 4:8], g["chi"]) and fm[:, 7].sum() > 100
    # backbone only = column 0 of all, and needs no aatype
    r1, t1, m1, _ = F.frames_rows(g["pos"], g["mask"], None, np.ones(R, bool), 0, 0)
    assert np.array_equal(F.bits(r1[:, 0]), F.bits(rot[:, 0])) and np.array_equal(F.bits(t1[:, 0]), F.bits(trans[:, 0])) and np.array_equal(m1[:, 0], fm[:, 0])


def test_meaning_on_the_goldens(gold37):
    g = gold37
    R = len(g["pos"])
    live = np.ones(R, bool)
    rot, trans, fm, _ = F.frames_rows(g["pos"], g["mask"], g["aatype"], live, 0, 1)
    rot64, trans64, fm64, n1 = F.frames_rows(g["pos"], g["mask"], g["aatype"], live, 0, 1, dtype=np.float64)
    assert np.array_equal(fm, fm64) and np.array_equal(trans.astype(np.float64), trans64)
    tab = F.slot_table(0)
    ty = np.minimum(g["aatype"].astype(np.int64), 20)
    worst = 0.0
    rows = np.arange(R)
    for grp in range(8):
        m = fm[:, grp] != 0
        if not m.any():
            continue
        Rm, t = rot[m, grp].astype(np.float64), trans[m, grp].astype(np.float64)
        sl = tab[ty[m], grp]
        local = [np.einsum("rij,ri->rj", Rm, g["pos"][rows[m], sl[:, j]].astype(np.float64) - t) for j in range(3)]   # R^T (x - t)
        want0 = np.zeros_like(local[0]); want0[:, 0] = n1[m, grp] * (1.0 if grp == 0 else -1.0)
        assert not local[1].any()                                     # trans is the origin atom's bits
        assert (local[2][:, 1] > 0).all(), grp                        # the plane atom lies at y > 0
        eye = np.einsum("rki,rkj->rij", Rm, Rm) - np.eye(3)
        dev = max(np.abs(local[0] - want0).max(), np.abs(local[2][:, 2]).max(), np.abs(eye).max(), np.abs(np.linalg.det(Rm) - 1.0).max(),
                  np.abs(Rm - rot64[m, grp]).max())
        worst = max(worst, float(dev))
    print(f"largest deviation of the float32 frames on the golden records: {worst:.3e} (bound {BOUND:.3e})")
    assert worst <= BOUND, worst


# ---- degenerate cases through the restatement ---------------------------------------------------------------------------------------

def _one_residue(ty=1):
    """an ARG-like row in atom37 with every slot set: well-conditioned integer coordinates"""
    rng = np.random.default_rng(3)
    pos = rng.integers(-9, 10, size=(1, 37, 3)).astype(np.float32) + np.arange(37, dtype=np.float32)[None, :, None] * np.float32(0.25)
    return pos, np.ones((1, 37), np.uint8), np.asarray([ty], np.uint8)


def _is_blank(rot, trans, fm, grp):
    return np.array_equal(rot[0, grp], np.eye(3, dtype=np.float32)) and not F.bits(trans[0, grp]).any() and fm[0, grp] == 0


def test_degenerate_cases():
    pos, mask, aa = _one_residue()
    live = np.ones(1, bool)
    rot, trans, fm, _ = F.frames_rows(pos, mask, aa, live, 0, 1)
    assert fm[0].tolist() == [1, 0, 0, 1, 1, 1, 1, 1]
    s = F.slot_table(0)[1]
    for grp in (0, 3, 4, 7):
        a0, a1, a2 = s[grp]
        cases = {}
        p = pos.copy(); p[0, a0] = p[0, a1]; cases["coincident, n1 = 0"] = p
        p = pos.copy(); p[0, a0] = p[0, a1] + np.asarray([3, 0, 0], np.float32); p[0, a2] = p[0, a1] - np.asarray([6, 0, 0], np.float32)
        cases["collinear, n2 = 0"] = p                                # (on a coordinate axis: e1 and u = v2 - e1*d are exact)
        p = pos.copy(); p[0, a0] = np.float32(3e38); p[0, a1] = np.float32(-3e38); cases["n1 overflows"] = p
        p = pos.copy(); p[0, a2] = np.float32(3e38); cases["n2 overflows"] = p
        p = pos.copy(); p[0, a2, 1] = np.nan; cases["NaN"] = p
        p = pos.copy(); p[0, a1, 2] = -np.inf; cases["-inf"] = p
        for what, p in cases.items():
            r, t, m, _ = F.frames_rows(p, mask, aa, live, 0, 1)
            assert _is_blank(r, t, m, grp), (grp, what)
            assert not np.isnan(r).any() and not np.isnan(t).any(), (grp, what)
            for other in range(8):                                    # a group that shares none of the three atoms is unchanged
                if fm[0, other] and not set(s[other]) & {a0, a1, a2}:
                    assert m[0, other] and np.array_equal(F.bits(r[0, other]), F.bits(rot[0, other])), (grp, what, other)
        for a in (a0, a1, a2):
            mk = mask.copy(); mk[0, a] = 0
            assert _is_blank(*F.frames_rows(pos, mk, aa, live, 0, 1)[:3], grp), (grp, a)
    # a row outside its chain, a type without chi groups, a layout without their slots
    assert not F.frames_rows(pos, mask, aa, np.zeros(1, bool), 0, 1)[2].any()
    assert F.frames_rows(pos, mask, np.asarray([200], np.uint8), live, 0, 1)[2][0].tolist() == [1, 0, 0, 1, 0, 0, 0, 0]
    assert F.frames_rows(pos[:, :4], mask[:, :4], aa, live, 2, 1)[2][0].tolist() == [1, 0, 0, 1, 0, 0, 0, 0]
    # -0.0 is a finite coordinate and the origin keeps its bits
    p = pos.copy(); p[0, 1] = np.float32(-0.0)
    r, t, m, _ = F.frames_rows(p, mask, aa, live, 0, 0)
    assert m[0, 0] == 1 and (F.bits(t[0, 0]) == 0x80000000).all()


def test_restatement_padded_and_packed_forms_agree():
    rng = np.random.default_rng(4)
    lens = np.asarray([0, 3, 5, 9], np.uint32)
    pos = rng.integers(-9, 10, size=(4, 5, 14, 3)).astype(np.float32)
    mask = (rng.random((4, 5, 14)) > 0.1).astype(np.uint8)
    aa = rng.integers(0, 21, size=(4, 5)).astype(np.uint8)
    rot, trans, fm = F.frames(pos, mask, aa, lens, 1, 1)
    assert rot.shape == (4, 5, 8, 3, 3) and trans.shape == (4, 5, 8, 3) and fm.shape == (4, 5, 8)
    assert not fm[0].any() and not fm[1, 3:].any() and fm[3, :, 0].sum() >= 3
    pr, pt, pm = F.frames(pos.reshape(20, 14, 3), mask.reshape(20, 14), aa.reshape(20), None, 1, 1)
    live = F.live_rows(4, 5, lens).reshape(20)
    assert np.array_equal(F.bits(pr[live]), F.bits(rot.reshape(20, 8, 3, 3)[live])) and np.array_equal(pm[live], fm.reshape(20, 8)[live])


# ---- argument errors without a device -------------------------------------------------------------------------------------------------

def test_pure_host_refusals():
    lib = _lib.load()
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    assert lib.fcz_frames(None, p, p, p, None, 1, 4, 0, 1, p, p, p) == -1
    assert lib.fcz_frames_dev(None, p, p, p, None, 1, 4, 0, 1, p, p, p) == -1
    fake = ctypes.c_void_p(p)                                          # refused before the ctx is read
    for fn in (lib.fcz_frames, lib.fcz_frames_dev):
        for a in ((fake, None, p, p, None, 1, 4, 0, 1, p, p, p), (fake, p, None, p, None, 1, 4, 0, 1, p, p, p), (fake, p, p, None, None, 1, 4, 0, 1, p, p, p),
                  (fake, p, p, p, None, 1, 4, 0, 1, None, p, p), (fake, p, p, p, None, 1, 4, 0, 1, p, None, p), (fake, p, p, p, None, 1, 4, 0, 1, p, p, None),
                  (fake, p, p, p, None, 1, 4, 3, 1, p, p, p), (fake, p, p, p, None, 1, 4, -1, 1, p, p, p), (fake, p, p, p, None, 1, 4, 0, 2, p, p, p),
                  (fake, p, p, p, None, 1, 4, 0, -1, p, p, p), (fake, p, p, p, None, 1, 0, 0, 1, p, p, p)):
            assert fn(*a) == -1, a
    assert not buf.any()


def test_argument_errors_need_no_device():
    pos37, mask37, aa = np.zeros((2, 8, 37, 3), np.float32), np.zeros((2, 8, 37), np.uint8), np.zeros((2, 8), np.uint8)
    for kw in (dict(pos=pos37, mask=mask37, aatype=aa, groups="chi"), dict(pos=pos37, mask=mask37, aatype=aa, groups=1),
               dict(pos=pos37, mask=mask37, aatype=aa, groups=None), dict(pos=pos37, mask=mask37, groups="all"),
               dict(pos=np.zeros((2, 8, 5, 3), np.float32), mask=mask37), dict(pos=np.zeros((2, 8, 37), np.float32), mask=mask37),
               dict(pos=np.zeros((2, 8, 37, 4), np.float32), mask=mask37), dict(pos=np.zeros((1, 2, 8, 37, 3), np.float32), mask=mask37)):
        with pytest.raises(ValueError):
            tensors.rigid_frames(**kw)
    with pytest.raises(TypeError):
        tensors.rigid_frames(mask=mask37)
    assert api.check_frames("backbone") == 0 and api.check_frames("all") == 1 and api.check_frames("backbone", has_aatype=False) == 0

    class NoRecords(api.FoldcompDatabase):
        def __init__(self):
            pass

        def __len__(self):
            raise AssertionError("tensor_batches read the database before it checked its arguments")

    for kw in (dict(frames="chi"), dict(frames=True), dict(frames=8), dict(frames="ALL")):
        with pytest.raises(ValueError):
            tensors.decode_tensors([b"x"], device="cuda:99", **kw)
        with pytest.raises(ValueError):
            next(NoRecords().tensor_batches(4, device="cuda:99", **kw))
        with pytest.raises(ValueError):
            next(NoRecords().tensor_batches(4, packed=True, device="cuda:99", **kw))
