"""CPU: the parts of the superposition feature that need no device -- the float64 numpy reference (tests/_superpose.py) on known
rigid motions, mirrored predictions and degenerate chains, its padded form against its packed form, the float32 apply step, the
conditions the GPU test's seeded inputs must meet for a float64 judge to be fair, the new ABI symbols and their refusal of a NULL
ctx, and the argument errors of foldcomp.superpose / apply_transform, raised before torch or a device is touched."""
import ctypes

import numpy as np
import pytest

import _superpose as S
from foldcomp_amd import _lib, api, tensors
from foldcomp_amd.structure import CSuperposeOut

NEW = ("fcz_superpose_dev", "fcz_superpose_packed_dev", "fcz_superpose", "fcz_superpose_packed",
       "fcz_superpose_apply_dev", "fcz_superpose_apply_packed_dev", "fcz_superpose_apply", "fcz_superpose_apply_packed")
F = np.float32


def _lattice(m, seed):
    """m distinct points of an integer lattice, not collinear and not coplanar for m >= 4"""
    rng = np.random.default_rng(seed)
    pts = rng.permutation(np.stack(np.meshgrid(*[np.arange(-4, 5)] * 3), -1).reshape(-1, 3))[:m].astype(np.float64)
    return pts


@pytest.mark.parametrize("m", [3, 4, 17, 300])
def test_reference_recovers_a_known_rigid_motion(m):
    rng = np.random.default_rng(m)
    a = _lattice(m, m)
    rot, trans = S.random_rotation(rng), rng.uniform(-30, 30, 3)
    b = a @ rot.T + trans
    got_r, got_t = S.kabsch(a, b)
    assert np.abs(got_r - rot).max() < 1e-10 and np.abs(got_t - trans).max() < 1e-10
    assert np.abs((a @ got_r.T + got_t) - b).max() < 1e-10


def test_a_mirrored_prediction_gets_a_proper_rotation_and_the_larger_rmsd():
    rng = np.random.default_rng(9)
    b = _lattice(60, 9)
    a = (b * np.asarray([-1.0, 1.0, 1.0])) @ S.random_rotation(rng).T + rng.uniform(-10, 10, 3)
    rot, trans = S.kabsch(a, b)
    assert abs(np.linalg.det(rot) - 1.0) < 1e-12 and np.abs(rot @ rot.T - np.eye(3)).max() < 1e-12
    rmsd = np.sqrt((((a @ rot.T + trans) - b) ** 2).sum(axis=1).mean())
    # what a determinant-free SVD returns: the improper minimiser, which lays the mirror image onto the target exactly
    ca, cb = a.mean(axis=0), b.mean(axis=0)
    u, _, vt = np.linalg.svd((a - ca).T @ (b - cb))
    improper = vt.T @ u.T
    assert np.linalg.det(improper) < 0 and np.abs((a - ca) @ improper.T - (b - cb)).max() < 1e-10
    assert rmsd > 1.0
    # no proper rotation does better than the one returned
    for _ in range(200):
        r = S.random_rotation(rng)
        assert np.sqrt(((((a - ca) @ r.T) - (b - cb)) ** 2).sum(axis=1).mean()) >= rmsd - 1e-12
    # ... and small turns away from it do not either (a local check of the minimum)
    for _ in range(50):
        w = rng.standard_normal(3) * 1e-3
        k = np.asarray([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        r = (np.eye(3) + k + k @ k / 2) @ rot
        u2, _, vt2 = np.linalg.svd(r)
        r = u2 @ vt2
        assert np.sqrt(((((a - ca) @ r.T) - (b - cb)) ** 2).sum(axis=1).mean()) >= rmsd - 1e-12
    c = S.superpose_chain(b.astype(F), a.astype(F), np.ones(60, bool))
    assert abs(c["rmsd"] - rmsd) < 1e-4 and c["sites"] == 60 and c["gdt_counts"][4] < 60


def test_degenerate_chains():
    rng = np.random.default_rng(3)
    t, p = rng.uniform(-9, 9, (8, 3)).astype(F), rng.uniform(-9, 9, (8, 3)).astype(F)
    none = S.superpose_chain(t, p, np.zeros(8, bool))
    assert np.array_equal(none["rot"], np.eye(3)) and not none["trans"].any() and none["rmsd"] == 0 and none["sites"] == 0
    assert not none["gdt_counts"].any() and none["tm"] == 0 and not none["dev"].any()
    site = np.zeros(8, bool); site[5] = True
    one = S.superpose_chain(t, p, site)
    assert np.abs(one["rot"] - np.eye(3)).max() < 1e-15 and np.abs(one["trans"] - (t[5].astype(np.float64) - p[5])).max() < 1e-14
    assert one["rmsd"] < 1e-14 and one["sites"] == 1 and list(one["gdt_counts"]) == [1] * 5 and abs(one["tm"] - 1) < 1e-14
    site[2] = True
    two = S.superpose_chain(t, p, site)
    half = abs(np.linalg.norm(t[5].astype(np.float64) - t[2]) - np.linalg.norm(p[5].astype(np.float64) - p[2])) / 2
    assert abs(np.linalg.det(two["rot"]) - 1) < 1e-12 and abs(two["rmsd"] - half) < 1e-12 and np.abs(two["dev"][[2, 5]] - half).max() < 1e-12
    # collinear sites: a minimiser, a proper rotation; an exact copy along another line is matched exactly
    line = np.arange(6)[:, None] * np.asarray([[1.0, 2.0, -1.0]])
    moved = line @ S.random_rotation(rng).T + 4.0
    col = S.superpose_chain(moved.astype(F), line.astype(F), np.ones(6, bool))
    assert abs(np.linalg.det(col["rot"]) - 1) < 1e-12 and col["rmsd"] < 1e-5 and col["sites"] == 6


def test_padded_against_packed_and_the_site_rules():
    rng = np.random.default_rng(6)
    lens = [0, 1, 2, 5, 30]
    L, A = 32, 4
    pos = rng.uniform(-20, 20, (len(lens), L, A, 3)).astype(F)
    pred = (pos + rng.standard_normal(pos.shape)).astype(F)
    mask = (rng.random((len(lens), L, A)) > 0.1).astype(np.uint8)
    pmask = (rng.random((len(lens), L, A)) > 0.1).astype(np.uint8)
    pos[4, 3, 1, 0] = np.nan; pred[4, 7, 1, 2] = np.inf; mask[4, [3, 7], 1] = 1; pmask[4, [3, 7], 1] = 1
    pad = S.superpose_padded(pos, mask, pred, pmask, np.asarray(lens), 1)
    row_off = np.concatenate([[0], np.cumsum(lens)])
    pk = S.superpose_packed(*S.pack((pos, mask, pred, pmask), lens), row_off, 1)
    for k in S.KEYS[:-1]:
        assert np.array_equal(pad[k], pk[k]), k
    assert np.array_equal(S.pack((pad["dev"],), lens)[0], pk["dev"])
    for e, m in enumerate(lens):
        assert not pad["dev"][e, m:].any()
    site = S.site_of(pos, mask, pred, pmask, 1)
    assert not site[4, 3] and not site[4, 7] and pad["dev"][4, 3] == 0 and pad["dev"][4, 7] == 0
    assert pad["sites"][4] == site[4, :30].sum() < 30 and pad["sites"][0] == 0 and np.array_equal(pad["rot"][0], np.eye(3))
    assert S.superpose_padded(pos, mask, pred, None, np.asarray(lens), 1)["sites"][4] > pad["sites"][4]
    ts, ha = S.gdt_scores(pad["gdt_counts"], pad["sites"])
    assert ts[0] == 0 and ha[0] == 0 and (ts >= ha).all() and ts[4] > 0.5
    assert abs(float(ts[4]) - pad["gdt_counts"][4, 1:].sum() / (4 * pad["sites"][4])) < 1e-7


def test_the_apply_step_in_float32():
    rng = np.random.default_rng(8)
    n, L, A = 3, 6, 4
    pos = rng.uniform(-50, 50, (n, L, A, 3)).astype(F)
    mask = (rng.random((n, L, A)) > 0.2).astype(np.uint8)
    rot = np.stack([S.random_rotation(rng) for _ in range(n)]).astype(F)
    trans = rng.uniform(-9, 9, (n, 3)).astype(F)
    lens = np.asarray([6, 2, 0])
    out = S.apply_expected(pos, mask, rot, trans, length=lens)
    assert out.dtype == F and not out[2].any() and not out[1, 2:].any() and not out[mask == 0].any()
    e, l, a = 1, 1, int(np.flatnonzero(mask[1, 1])[0])
    x, y, z = pos[e, l, a]
    r = rot[e]
    assert out[e, l, a, 1] == F(F(F(r[1, 0] * x) + F(r[1, 1] * y)) + F(r[1, 2] * z)) + trans[e, 1]
    assert np.abs(out[0].astype(np.float64) - (pos[0].astype(np.float64) @ rot[0].astype(np.float64).T + trans[0]) * mask[0, ..., None]).max() < 1e-4
    row_off = np.asarray([0, 6, 8, 8])
    pk = S.apply_expected(*S.pack((pos, mask), lens), rot, trans, row_off=row_off)
    assert np.array_equal(pk, S.pack((out,), lens)[0])


def test_the_gpu_tests_seeded_inputs_meet_its_conditions():
    """exact integers and the 2-ulp tolerance of tests/test_gpu_superpose.py are fair only if, in float64, Horn's largest eigenvalue is
    well separated (a float64 Jacobi then has the rotation to ~1e-12) and no deviation lies near a GDT threshold"""
    lens, pos_t, mask, pos_p = S.walk_batch()
    ref = S.superpose_padded(pos_t, mask, pos_p, None, lens, 1)
    gaps, margin = [], np.inf
    for e, m in enumerate(lens):
        margin = min(margin, S.threshold_margin(ref["dev"][e, :m]))
        if m >= 3:
            gaps.append(S.horn_gap(pos_t[e, :m, 1], pos_p[e, :m, 1], np.ones(m, bool)))
    print(f"seed {S.WALK_SEED}: smallest eigenvalue gap {min(gaps):.3g}, smallest threshold margin {margin:.3g} A over {int(lens.sum())} sites")
    assert min(gaps) >= 1e-3 and margin >= 1e-4
    assert list(lens[:3]) == [0, 1, 2] and sorted(set(lens[3:])) == sorted(S.WALK_LENGTHS) and len(lens) == 3 + 2 * len(S.WALK_LENGTHS)
    # the mirrored half is scored worse by a proper rotation than the plain half
    plain, mirrored = ref["rmsd"][3::2], ref["rmsd"][4::2]
    assert (mirrored[3:] > plain[3:]).all() and plain[3:].max() < 3.5 and (np.abs(np.linalg.det(ref["rot"]) - 1) < 1e-12).all()
    assert (ref["gdt_counts"][:, 0] < ref["gdt_counts"][:, 4]).sum() > 20


def test_pure_host_abi():
    lib = _lib.load()
    assert set(NEW) <= set(_lib.EXPORTS)
    buf = np.zeros(256, np.uint8)
    p = buf.ctypes.data
    out = CSuperposeOut(p, p, p, p, p, p, p)
    for fn in (lib.fcz_superpose_dev, lib.fcz_superpose_packed_dev, lib.fcz_superpose, lib.fcz_superpose_packed):
        assert fn(None, p, p, p, p, p, 1, 4, 0, 1, ctypes.byref(out)) == -1
    for fn in (lib.fcz_superpose_apply_dev, lib.fcz_superpose_apply_packed_dev, lib.fcz_superpose_apply, lib.fcz_superpose_apply_packed):
        assert fn(None, p, p, p, 1, 4, 0, p, p, p) == -1
    # refused before anything is touched (the ctx is never read)
    fake = ctypes.c_void_p(buf.ctypes.data)
    for fn in (lib.fcz_superpose_dev, lib.fcz_superpose_packed_dev, lib.fcz_superpose, lib.fcz_superpose_packed):
        assert fn(fake, p, p, p, p, p, 1, 4, 0, 37, ctypes.byref(out)) == -1 and fn(fake, p, p, p, p, p, 1, 4, 3, 1, ctypes.byref(out)) == -1
        assert fn(fake, p, p, p, p, p, 1, 4, 2, 4, ctypes.byref(out)) == -1 and fn(fake, p, p, p, p, p, 1, 4, 0, -1, ctypes.byref(out)) == -1
        assert fn(fake, None, p, p, p, p, 1, 4, 0, 1, ctypes.byref(out)) == -1 and fn(fake, p, None, p, p, p, 1, 4, 0, 1, ctypes.byref(out)) == -1
        assert fn(fake, p, p, None, p, p, 1, 4, 0, 1, ctypes.byref(out)) == -1 and fn(fake, p, p, p, p, p, 1, 4, 0, 1, None) == -1
        assert fn(fake, p, p, p, p, p, 1, 4, 0, 1, ctypes.byref(CSuperposeOut(None, p, p, p, p, p, p))) == -1
        assert fn(fake, p, p, p, p, p, 1, 4, 0, 1, ctypes.byref(CSuperposeOut(p, None, p, p, p, p, p))) == -1
        assert fn(fake, p, p, p, p, p, 1, 2 ** 31, 0, 1, ctypes.byref(out)) == -1
    for fn in (lib.fcz_superpose_apply_dev, lib.fcz_superpose_apply_packed_dev, lib.fcz_superpose_apply, lib.fcz_superpose_apply_packed):
        assert fn(fake, None, p, p, 1, 4, 0, p, p, p) == -1 and fn(fake, p, p, p, 1, 4, 3, p, p, p) == -1 and fn(fake, p, p, p, 1, 4, -1, p, p, p) == -1
        assert fn(fake, p, p, p, 1, 4, 0, None, p, p) == -1 and fn(fake, p, p, p, 1, 4, 0, p, None, p) == -1 and fn(fake, p, p, p, 1, 4, 0, p, p, None) == -1
        assert fn(fake, p, p, p, 1, 2 ** 31, 0, p, p, p) == -1
    for fn in (lib.fcz_superpose_dev, lib.fcz_superpose):
        assert fn(fake, p, p, p, p, p, 1, 0, 0, 1, ctypes.byref(out)) == -1                       # L == 0
    for fn in (lib.fcz_superpose_packed_dev, lib.fcz_superpose_packed):
        assert fn(fake, p, p, p, p, None, 1, 4, 0, 1, ctypes.byref(out)) == -1                    # chains without a row_off
    for fn in (lib.fcz_superpose_apply_dev, lib.fcz_superpose_apply):
        assert fn(fake, p, p, p, 1, 0, 0, p, p, p) == -1
    for fn in (lib.fcz_superpose_apply_packed_dev, lib.fcz_superpose_apply_packed):
        assert fn(fake, p, p, None, 1, 4, 0, p, p, p) == -1
    assert not buf.any()


def test_argument_errors_need_no_device():
    pos37, mask37 = np.zeros((2, 8, 37, 3), F), np.zeros((2, 8, 37), np.uint8)
    pos4, mask4 = np.zeros((2, 8, 4, 3), F), np.zeros((2, 8, 4), np.uint8)
    true37, true4 = dict(pos=pos37, mask=mask37), dict(pos=pos4, mask=mask4)
    for pred, true, kw in ((pos37, true37, dict(atom="XX")), (pos4, true4, dict(atom="CB")), (pos37, true37, dict(atom=37)), (pos4, true4, dict(atom=4)),
                           (pos37, true37, dict(atom=-1)), (pos37, true37, dict(atom=1.5)), (pos37[:, :7], true37, {}), (pos4, true37, {}),
                           (dict(pos=pos37, mask=mask37[:1]), true37, {}), (dict(pos=pos37[:1], mask=mask37), true37, dict(apply=True))):
        with pytest.raises(ValueError):
            tensors.superpose(pred, true, **kw)
    with pytest.raises(TypeError):
        tensors.superpose(pos37, dict(pos=pos37))
    with pytest.raises(TypeError):
        tensors.superpose(dict(mask=mask37), true37)
    assert api.check_superpose("CA", pos37.shape, pos37.shape, mask37.shape) == 1 and api.check_superpose("CB", (9, 14, 3), (9, 14, 3)) == 4
    assert api.check_superpose(2, pos4.shape, pos4.shape) == 2
    rot, trans = np.zeros((2, 3, 3), F), np.zeros((2, 3), F)
    for args, kw in (((pos37[0, 0], rot, trans), {}), ((np.zeros((2, 8, 5, 3), F), rot, trans), {}), ((pos37, rot[:1], trans), {}), ((pos37, rot, trans[:, :2]), {}),
                     ((pos37, rot, trans), dict(mask=mask37[:, :7])), ((pos37[0], rot, trans), dict(cu_seqlens=np.asarray([0, 8]))),
                     ((dict(pos=pos37, mask=mask4), rot, trans), {})):
        with pytest.raises(ValueError):
            tensors.apply_transform(*args, **kw)
    with pytest.raises(TypeError):
        tensors.apply_transform(dict(mask=mask37), rot, trans)
    import foldcomp
    import foldcomp_amd
    assert foldcomp.superpose is foldcomp_amd.superpose is tensors.superpose
    assert foldcomp.apply_transform is foldcomp_amd.apply_transform is tensors.apply_transform
    assert api.GDT_THRESHOLDS == S.GDT
