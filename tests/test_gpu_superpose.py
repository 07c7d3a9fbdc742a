"""GPU: the least-squares superposition of two dense tensor batches (fcz_superpose_dev, fcz_superpose_packed_dev, the apply calls,
their host forms, Codec.superpose / apply_transform, foldcomp.superpose / apply_transform) against the independent float64 numpy
reference (tests/_superpose.py: SVD with the determinant correction). Integers are compared exactly, the float outputs by the
tolerance the header's single rounding allows, determinism and the apply step on bits; the device calls write into arrays
pre-filled with 0xA5 with guard bytes on both sides.

Why the tolerance is fair: tests/test_superpose_cpu.py asserts that on the seeded inputs Horn's largest eigenvalue is separated by
at least 1e-3 of itself, so a float64 Jacobi has the rotation to ~1e-12, far below a float32 ulp: the device value and the
reference differ by one rounding flip at most (2 ulps allowed), and no deviation lies within 1e-4 A of a GDT threshold."""
import numpy as np
import pytest

import _analysis as AN
import _superpose as S
from _cases import golden_records_raw
from _devpath import DevGuarded, HostGuarded, host_ptr, to_dev
from _window import Decoded

pytestmark = pytest.mark.gpu

L_GOLD = 1400
F = np.float32
POISON = (np.nan, np.inf, -np.inf)


@pytest.fixture(scope="module")
def walk():
    """the seeded batch (chains of 0, 1, 2 rows, then random walks of 3 .. 1027 rows, plain and mirrored) on backbone4 / CA, padded
    and packed, with the reference: computed once, never changed"""
    lens, pos_t, mask, pos_p = S.walk_batch()
    ref = S.superpose_padded(pos_t, mask, pos_p, mask, lens, 1)
    row_off = AN.row_off_of(lens)
    return dict(lens=lens.astype(np.uint32), n=len(lens), L=pos_t.shape[1], arrays=(pos_t, mask, pos_p), ref=ref, row_off=row_off,
                packed=S.pack((pos_t, mask, pos_p), lens), solved=lens >= 3)


def _show(what, seen):
    print(f"{what}: largest deviation from the float64 reference rounded to float32: " +
          ", ".join(f"{k} {v:.3g}{'' if k == 'rot' else ' ulp'}" for k, v in seen.items()))


def test_walks_padded_and_packed(codec, walk):
    w = walk
    pt, mt, pp = (to_dev(a) for a in w["arrays"])
    dl = to_dev(w["lens"])
    got = S.run_dev(codec, pt, mt, pp, mt, dl, w["n"], w["L"], 2, 1, False)
    _show("walks, padded", S.close(got, w["ref"], "padded", compare_rot=w["solved"]))
    S.proper(got["rot"], "padded")
    # the degenerate chains: none, one site (the identity, trans = b - a rounded once), two sites
    eye = np.eye(3, dtype=F)
    t, p = w["arrays"][0], w["arrays"][2]
    assert got["rot"][0].tobytes() == eye.tobytes() and not got["trans"][0].any() and got["sites"][0] == 0 and got["rmsd"][0] == 0 and got["tm"][0] == 0
    assert np.array_equal(got["rot"][1], eye) and got["sites"][1] == 1 and got["rmsd"][1] == 0 and list(got["gdt_counts"][1]) == [1] * 5
    assert got["trans"][1].tobytes() == (t[1, 0, 1].astype(np.float64) - p[1, 0, 1].astype(np.float64)).astype(F).tobytes()
    assert got["sites"][2] == 2 and got["rmsd"][2] > 0
    for e, m in enumerate(w["lens"]):
        assert not got["dev"][e, m:].view(np.uint32).any()
    # determinism on bits: the same call again, and the packed form
    S.same_bytes(S.run_dev(codec, pt, mt, pp, mt, dl, w["n"], w["L"], 2, 1, False), got, "second call")
    kt, km, kp = (to_dev(a) for a in w["packed"])
    R = int(w["row_off"][-1])
    pk = S.run_dev(codec, kt, km, kp, km, to_dev(w["row_off"]), w["n"], R, 2, 1, True)
    S.same_bytes({k: pk[k] for k in S.KEYS[:-1]}, {k: got[k] for k in S.KEYS[:-1]}, "packed")
    assert pk["dev"].tobytes() == S.pack((got["dev"],), w["lens"])[0].tobytes()
    # the host-pointer forms give the same bytes
    h = codec.superpose(w["arrays"][0], w["arrays"][1], w["arrays"][2], w["arrays"][1], 1, length=w["lens"])
    S.same_bytes({k: h[k] for k in S.KEYS}, got, "fcz_superpose")
    h = codec.superpose(*w["packed"], w["packed"][1], 1, row_off=w["row_off"])
    S.same_bytes({k: h[k] for k in S.KEYS}, pk, "fcz_superpose_packed")


def test_other_layouts_and_slots_give_the_same_bits(codec, walk):
    w = walk
    base = S.run_dev(codec, *(to_dev(a) for a in w["arrays"]), None, to_dev(w["lens"]), w["n"], w["L"], 2, 1, False)
    xt, xp = w["arrays"][0][:, :, 1], w["arrays"][2][:, :, 1]
    for layout, A, slot in ((1, 14, 4), (0, 37, 3), (0, 37, 36), (2, 4, 0)):
        pos_t, pos_p = S.in_slot(xt, A, slot, 5.0), S.in_slot(xp, A, slot, -2.0)
        mask = np.zeros(pos_t.shape[:-1], np.uint8); mask[..., slot] = 1
        got = S.run_dev(codec, to_dev(pos_t), to_dev(mask), to_dev(pos_p), None, to_dev(w["lens"]), w["n"], w["L"], layout, slot, False, guard=4)
        S.same_bytes(got, base, f"layout {layout} slot {slot}, outputs not 16-byte aligned")


def _poisoned(rng, m=3 * 64 + 1, A=4, slot=1):
    """one chain of 3 * 64 + 1 rows inside a padded entry of m + 40 rows: ~15 % of the sites cleared in mask_true only, ~15 % in mask_pred
    only, a NaN at one site's slot in true and one in pred (both masks set), and the clean twin with those sites cleared in both"""
    L = m + 40
    x = S.walk_chain(rng, L)
    y = x @ S.random_rotation(rng).T + rng.uniform(-20, 20, 3) + 1.5 * rng.standard_normal((L, 3))
    pos_t, pos_p = S.in_slot(x[None].astype(F), A, slot, 1.0), S.in_slot(y[None].astype(F), A, slot, 2.0)
    mt, mp = np.ones((1, L, A), np.uint8), np.ones((1, L, A), np.uint8)
    u = rng.random(L)
    mt[0, u < 0.15, slot] = 0
    mp[0, (u >= 0.15) & (u < 0.30), slot] = 0
    ok = np.flatnonzero(u[:m] >= 0.30)
    nan_t, nan_p = int(ok[5]), int(ok[40])
    clean = (pos_t.copy(), mt.copy(), pos_p.copy(), mp.copy())
    clean[1][0, [nan_t, nan_p], slot] = 0
    pos_t[0, nan_t, slot, 1] = np.nan
    pos_p[0, nan_p, slot, 2] = -np.inf
    return m, L, (pos_t, mt, pos_p, mp), clean, (nan_t, nan_p)


def test_poisoned_inputs_change_nothing(codec):
    rng = np.random.default_rng(21)
    m, L, dirty, clean, (nan_t, nan_p) = _poisoned(rng)
    length = np.asarray([m], np.uint32)
    ref = S.superpose_padded(*clean, length, 1)
    assert S.threshold_margin(ref["dev"][0, :m][ref["dev"][0, :m] > 0]) >= 1e-4 and S.horn_gap(clean[0][0, :m, 1], clean[2][0, :m, 1], S.site_of(*clean, 1)[0, :m]) >= 1e-3
    assert 100 < ref["sites"][0] < 0.8 * m and (clean[1][0, :m, 1] != clean[3][0, :m, 1]).sum() > 30
    base = S.run_dev(codec, *(to_dev(a) for a in clean), to_dev(length), 1, L, 2, 1, False)
    _show("a chain of 3 * 64 + 1 rows, sites cleared in one mask only", S.close(base, ref, "clean"))
    # a NaN at a site's slot in either tensor removes that site only
    got = S.run_dev(codec, *(to_dev(a) for a in dirty), to_dev(length), 1, L, 2, 1, False)
    S.same_bytes(got, base, "a non-finite coordinate at a site")
    assert got["dev"][0, nan_t] == 0 and got["dev"][0, nan_p] == 0
    # patterns behind the length and under every cleared mask, in both tensors
    for fill in POISON + ("0xA5",):
        pos_t, mt, pos_p, mp = (a.copy() for a in dirty)
        for pos, mask in ((pos_t, mt), (pos_p, mp)):
            if fill == "0xA5":
                pos.view(np.uint8)[0, m:] = 0xA5
                pos.view(np.uint32)[mask == 0] = 0xA5A5A5A5
            else:
                pos[0, m:] = fill
                pos[mask == 0] = fill
        got = S.run_dev(codec, to_dev(pos_t), to_dev(mt), to_dev(pos_p), to_dev(mp), to_dev(length), 1, L, 2, 1, False)
        S.same_bytes(got, base, f"poison {fill}")
        # packed: the chain in the middle of rows no chain covers, which hold the same poison
        row_off = np.asarray([20, 20 + m], np.uint32)
        shift = lambda a: np.concatenate([a[0, m:m + 20], a[0, :m], a[0, m + 20:]])
        pk = S.run_dev(codec, *(to_dev(shift(a)) for a in (pos_t, mt, pos_p, mp)), to_dev(row_off), 1, L, 2, 1, True)
        S.same_bytes({k: pk[k] for k in S.KEYS[:-1]}, {k: base[k] for k in S.KEYS[:-1]}, f"packed, poison {fill}")
        assert pk["dev"][20:20 + m].tobytes() == base["dev"][0, :m].tobytes() and not pk["dev"][:20].view(np.uint32).any()
        assert not pk["dev"][20 + m:].view(np.uint32).any()


def test_mask_pred_null_and_optional_outputs(codec, walk):
    w = walk
    pos_t, mask, pos_p = (a[9:15].copy() for a in w["arrays"])                # the chains of 63, 64 and 65 rows
    lens = w["lens"][9:15]
    mp = mask.copy()
    mp[:, ::3, 1] = 0
    dev = [to_dev(a) for a in (pos_t, mask, pos_p)]
    with_mask = S.run_dev(codec, *dev, to_dev(mp), to_dev(lens), 6, w["L"], 2, 1, False)
    without = S.run_dev(codec, *dev, None, to_dev(lens), 6, w["L"], 2, 1, False)
    assert (without["sites"] == lens).all() and (with_mask["sites"] < lens).all()
    S.close(with_mask, S.superpose_padded(pos_t, mask, pos_p, mp, lens, 1), "mask_pred", compare_rot=with_mask["sites"] >= 3)
    S.same_bytes(without, {k: v[9:15] for k, v in S.run_dev(codec, *(to_dev(a) for a in w["arrays"]), None, to_dev(w["lens"]), w["n"], w["L"], 2, 1, False).items()},
                 "a chain's result does not depend on the batch around it")
    # NULL optional outputs leave the others unchanged
    for want in (("rot", "trans"), ("rot", "trans", "dev"), ("rot", "trans", "rmsd", "tm"), ("rot", "trans", "sites", "gdt_counts")):
        part = S.run_dev(codec, *dev, None, to_dev(lens), 6, w["L"], 2, 1, False, want=want)
        S.same_bytes(part, {k: without[k] for k in want}, f"only {want}")


def test_length_null_and_clamped(codec):
    rng = np.random.default_rng(12)
    n, L = 3, 300
    x = np.stack([S.walk_chain(rng, L) for _ in range(n)])
    y = x + 1.5 * rng.standard_normal(x.shape)
    pos_t, pos_p = S.in_slot(x.astype(F), 14, 4), S.in_slot(y.astype(F), 14, 4)
    mask = np.ones((n, L, 14), np.uint8)
    dev = [to_dev(a) for a in (pos_t, mask, pos_p)]
    whole = S.run_dev(codec, *dev, None, None, n, L, 1, 4, False)
    assert (whole["sites"] == L).all()
    S.close(whole, S.superpose_padded(pos_t, mask, pos_p, None, None, 4), "NULL", floor=1e-8)
    S.same_bytes(S.run_dev(codec, *dev, None, to_dev(np.full(n, L, np.uint32)), n, L, 1, 4, False), whole, "length = L")
    S.same_bytes(S.run_dev(codec, *dev, None, to_dev(np.asarray([L + 1, 65535, 0xFFFFFFFF], np.uint32)), n, L, 1, 4, False), whole, "length > L")
    lens = np.asarray([40, 300, 257], np.uint32)
    part = S.run_dev(codec, *dev, None, to_dev(lens), n, L, 1, 4, False)
    assert list(part["sites"]) == [40, 300, 257] and part["dev"][1].tobytes() == whole["dev"][1].tobytes() and not part["dev"][0, 40:].any()


def test_hostile_row_off(codec):
    rng = np.random.default_rng(13)
    R = 700
    x = S.walk_chain(rng, R)
    y = x + 1.5 * rng.standard_normal(x.shape)
    pos_t, pos_p = S.in_slot(x.astype(F), 4, 1), S.in_slot(y.astype(F), 4, 1)
    mask = np.ones((R, 4), np.uint8)
    dev = [to_dev(a) for a in (pos_t, mask, pos_p)]
    row_off = AN.HOSTILE_ROW_OFF
    ref = S.superpose_packed(pos_t, mask, pos_p, None, row_off, 1)
    got = S.run_dev(codec, *dev, None, to_dev(row_off), 5, R, 2, 1, True)
    assert list(got["sites"]) == [0, 80, 280, 1, 299] == list(ref["sites"])
    assert np.array_equal(got["gdt_counts"], ref["gdt_counts"]) and not got["dev"][:40].view(np.uint32).any()
    S.close(got, ref, "hostile row_off", compare_rot=got["sites"] >= 3)
    out = S.run_apply(codec, dev[2], None, to_dev(row_off), 5, R, 2, to_dev(got["rot"]), to_dev(got["trans"]), True)
    assert out.tobytes() == S.apply_expected(pos_p, None, got["rot"], got["trans"], row_off=row_off).tobytes() and not out[:40].any() and out[40:].any()
    # no chain at all: every row is uncovered
    none = S.run_dev(codec, *dev, None, to_dev(row_off), 0, R, 2, 1, True, want=("rot", "trans", "dev"))
    assert not none["dev"].view(np.uint32).any()
    out_none = S.run_apply(codec, dev[2], None, to_dev(row_off), 0, R, 2, dev[2], dev[2], True)
    assert not out_none.view(np.uint32).any()

    def host_form(arrays, off, n, rows):
        """fcz_superpose_packed on host arrays (pos_true, mask_true, pos_pred), its outputs between guard bytes"""
        import ctypes
        from foldcomp_amd.structure import CSuperposeOut
        h = HostGuarded(S.out_spec(n, rows, True))
        o = CSuperposeOut(*h.ptrs())
        assert codec.lib.fcz_superpose_packed(codec.ctx, *(host_ptr(a) for a in arrays), None, host_ptr(off), n, rows, 2, 1, ctypes.byref(o)) == 0
        return {k: h.fetch(k) for k in S.KEYS}

    def host_apply(pos, off, n, rows, rot, trans):
        """fcz_superpose_apply_packed on host arrays, pos_out between guard bytes"""
        h = HostGuarded(dict(out=(F, (rows, 4, 3))))
        assert codec.lib.fcz_superpose_apply_packed(codec.ctx, host_ptr(pos), None, host_ptr(off), n, rows, 2, host_ptr(rot), host_ptr(trans), h.ptr("out")) == 0
        return h

    # the host forms on the same arrays: what the device forms gave
    S.same_bytes(host_form((pos_t, mask, pos_p), row_off, 5, R), got, "fcz_superpose_packed n=5")
    host = host_form((pos_t, mask, pos_p), row_off, 0, R)
    S.same_bytes({k: host[k] for k in none}, none, "fcz_superpose_packed n=0")
    assert host_apply(pos_p, row_off, 5, R, got["rot"], got["trans"]).fetch("out").tobytes() == out.tobytes()
    assert host_apply(pos_p, row_off, 0, R, pos_p, pos_p).fetch("out").tobytes() == out_none.tobytes()
    # chains without a row (R = 0): the per-chain outputs of an empty chain in both forms, and apply writes nothing
    one, zeros = (pos_t[:1], mask[:1], pos_p[:1]), np.zeros(4, np.uint32)
    empty = S.run_dev(codec, *(to_dev(a) for a in one), None, to_dev(zeros), 3, 0, 2, 1, True)
    S.close(empty, S._empty(3, (0,)), "R = 0")
    assert not empty["rmsd"].view(np.uint32).any() and not empty["tm"].view(np.uint32).any()
    S.same_bytes(host_form(one, zeros, 3, 0), empty, "fcz_superpose_packed R=0")
    import torch
    g, tensors = DevGuarded({"out": (F, (1, 4, 3))}), [to_dev(a) for a in (zeros, empty["rot"], empty["trans"])]
    torch.cuda.synchronize()
    assert codec.lib.fcz_superpose_apply_packed_dev(codec.ctx, dev[2].data_ptr(), None, tensors[0].data_ptr(), 3, 0, 2, tensors[1].data_ptr(),
                                                    tensors[2].data_ptr(), g.ptr("out")) == 0
    codec.synchronize()
    assert g.untouched()
    assert host_apply(pos_p[:1], zeros, 3, 0, empty["rot"], empty["trans"]).untouched()


def test_apply_on_bits(codec, walk):
    """pos_out against the numpy apply step fed the device's own float32 rot / trans: slots under a cleared mask and rows behind the
    length are 0 whatever they hold, inputs and outputs need not begin on 16 bytes, any transform is taken"""
    import torch
    w = walk
    rng = np.random.default_rng(31)
    lens = w["lens"]
    solved = S.run_dev(codec, *(to_dev(a) for a in w["arrays"]), None, to_dev(lens), w["n"], w["L"], 2, 1, False, want=("rot", "trans"))
    rot, trans = solved["rot"], solved["trans"]
    for layout, A, L in ((0, 37, 70), (1, 14, 300), (2, 4, w["L"])):
        n = w["n"]
        ln = np.minimum(lens, L).astype(np.uint32)
        pos = rng.uniform(-80, 80, (n, L, A, 3)).astype(F)
        mask = (rng.random((n, L, A)) > 0.25).astype(np.uint8)
        exp = S.apply_expected(pos, mask, rot, trans, length=ln)
        for fill in POISON:
            dirty = pos.copy()
            dirty[mask == 0] = fill
            for e, m in enumerate(ln):
                dirty[e, m:] = fill
            # one float in front of the tensor: pos begins 4 bytes past an allocation, and so does pos_out (guard = 4)
            flat = torch.empty(dirty.size + 1, dtype=torch.float32, device="cuda:0")
            flat[1:] = to_dev(dirty).reshape(-1)
            got = S.run_apply(codec, flat[1:].view(n, L, A, 3), to_dev(mask), to_dev(ln), n, L, layout, to_dev(rot), to_dev(trans), False, guard=4)
            assert got.tobytes() == exp.tobytes(), (layout, fill)
        assert exp.any() and not exp[mask == 0].any()
        # packed, mask NULL, transforms that are no rotations
        any_rot, any_trans = rng.uniform(-2, 2, (n, 3, 3)).astype(F), rng.uniform(-100, 100, (n, 3)).astype(F)
        row_off = AN.row_off_of(ln)
        ppos, pmask = S.pack((pos, mask), ln)
        got = S.run_apply(codec, to_dev(ppos), None, to_dev(row_off), n, len(ppos), layout, to_dev(any_rot), to_dev(any_trans), True)
        assert got.tobytes() == S.apply_expected(ppos, None, any_rot, any_trans, row_off=row_off).tobytes(), layout
        got = S.run_apply(codec, to_dev(ppos), to_dev(pmask), to_dev(row_off), n, len(ppos), layout, to_dev(rot), to_dev(trans), True, guard=12)
        assert got.tobytes() == S.pack((exp,), ln)[0].tobytes(), layout
        host = codec.apply_transform(pos, rot, trans, mask=mask, length=ln)
        assert host.tobytes() == exp.tobytes()
    host = codec.apply_transform(ppos, rot, trans, mask=pmask, row_off=row_off)
    assert host.tobytes() == S.pack((exp,), ln)[0].tobytes()


def test_refusals_leave_the_outputs_untouched(codec):
    import ctypes
    import torch
    from foldcomp_amd.structure import CSuperposeOut
    n, L, A = 2, 8, 37
    pos, mask, _, off = AN.refusal_inputs(n, L, A)
    g = DevGuarded(S.out_spec(n, L, False))
    g2 = DevGuarded({"out": (F, (n, L, A, 3))})
    out = CSuperposeOut(*(g.ptr(k) for k in S.KEYS))
    no_rot = CSuperposeOut(None, *(g.ptr(k) for k in S.KEYS[1:]))
    no_trans = CSuperposeOut(g.ptr("rot"), None, *(g.ptr(k) for k in S.KEYS[2:]))
    lib, ctx, P, M, O = codec.lib, codec.ctx, pos.data_ptr(), mask.data_ptr(), off.data_ptr()
    ok = dict(ctx=ctx, pt=P, mt=M, pp=P, mp=M, bound=None, n=n, L=L, layout=0, slot=1, out=ctypes.byref(out))
    bad = [dict(ctx=None), dict(pt=None), dict(mt=None), dict(pp=None), dict(out=None), dict(out=ctypes.byref(no_rot)), dict(out=ctypes.byref(no_trans)),
           dict(layout=3), dict(layout=-1), dict(slot=37), dict(slot=-1), dict(layout=1, slot=14), dict(layout=2, slot=4), dict(L=2 ** 31), dict(L=0)]
    torch.cuda.synchronize()
    for b in bad:
        assert lib.fcz_superpose_dev(*dict(ok, **b).values()) == -1, b
    for b in bad[:-1]:
        a = dict(ok, bound=O, L=n * L)
        a.update(b)
        assert lib.fcz_superpose_packed_dev(*a.values()) == -1, b
    assert lib.fcz_superpose_packed_dev(*dict(ok, L=n * L).values()) == -1                    # chains without a row_off
    assert lib.fcz_superpose_dev(*dict(ok, n=0).values()) == 0 and lib.fcz_superpose_packed_dev(*dict(ok, bound=O, n=0, L=0).values()) == 0
    R, T = g.ptr("rot"), g.ptr("trans")
    ok = dict(ctx=ctx, pos=P, mask=M, bound=None, n=n, L=L, layout=0, rot=R, trans=T, out=g2.ptr("out"))
    bad = [dict(ctx=None), dict(pos=None), dict(rot=None), dict(trans=None), dict(out=None), dict(layout=3), dict(layout=-1), dict(L=2 ** 31), dict(L=0)]
    for b in bad:
        assert lib.fcz_superpose_apply_dev(*dict(ok, **b).values()) == -1, b
    for b in bad[:-1]:
        a = dict(ok, bound=O, L=n * L)
        a.update(b)
        assert lib.fcz_superpose_apply_packed_dev(*a.values()) == -1, b
    assert lib.fcz_superpose_apply_packed_dev(*dict(ok, L=n * L).values()) == -1
    assert lib.fcz_superpose_apply_dev(*dict(ok, n=0).values()) == 0 and lib.fcz_superpose_apply_packed_dev(*dict(ok, bound=O, L=0).values()) == 0
    codec.synchronize()
    assert g.untouched() and g2.untouched()


# ---- the golden records and the Python surface -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def records(golden):
    return golden_records_raw(golden)[1]


def _moved(pos, rng, noise):
    """pos float32 [n, L, A, 3] -> every entry under a random rigid motion of its own plus Gaussian noise, float32"""
    out = np.empty_like(pos)
    for e in range(len(pos)):
        out[e] = pos[e].astype(np.float64) @ S.random_rotation(rng).T + rng.uniform(-40, 40, 3) + noise * rng.standard_normal(pos[e].shape)
    return out


def test_golden_records(codec, records):
    """the 56 golden records at L = 1400 against themselves under a rigid motion plus noise, atom37, CA and CB. The deviations of
    ~30 000 sites cannot all stay 1e-4 A off the thresholds; what exact counts need is that none lies within the float64 error of the
    two implementations, ~1e-12 rad of rotation times a lever of under 1e3 A: asserted with a margin of 1e-9 A."""
    dec = Decoded(codec, records)
    h = dec.dense("atom37", L_GOLD, want=("pos", "mask", "length"))
    rng = np.random.default_rng(17)
    pred = _moved(h["pos"], rng, 0.5)
    pred[::7] = _moved(h["pos"][::7], rng, 0.0)                                # every seventh chain: a rigid motion only
    dev = [to_dev(a) for a in (h["pos"], h["mask"], pred)]
    dl = to_dev(h["length"])
    n = len(records)
    for slot, name in ((1, "CA"), (3, "CB")):
        ref = S.superpose_padded(h["pos"], h["mask"], pred, None, h["length"], slot)
        site = S.site_of(h["pos"], h["mask"], pred, None, slot)
        assert S.threshold_margin(ref["dev"][site & (np.arange(L_GOLD)[None] < h["length"][:, None])]) >= 1e-9
        solved = ref["sites"] >= 3
        gaps = [S.horn_gap(h["pos"][e, :, slot], pred[e, :, slot], site[e] & (np.arange(L_GOLD) < h["length"][e])) for e in np.flatnonzero(solved)]
        assert min(gaps) >= 1e-3
        got = S.run_dev(codec, *dev, None, dl, n, L_GOLD, 0, slot, False)
        # a rigid motion of float32 coordinates stored as float32 leaves ~1e-5 A; the floor is for a structure against itself
        _show(f"golden records, {name}", S.close(got, ref, name, compare_rot=solved))
        S.proper(got["rot"], name)
        assert got["rmsd"][::7].max() < 1e-3 and np.median(got["rmsd"]) > 0.5 and (got["sites"] > 0).sum() >= 50
        lens = np.minimum(h["length"].astype(np.int64), L_GOLD)
        row_off = AN.row_off_of(lens)
        pk = S.run_dev(codec, *(to_dev(a) for a in S.pack((h["pos"], h["mask"], pred), lens)), None, to_dev(row_off), n, int(row_off[-1]), 0, slot, True)
        S.same_bytes({k: pk[k] for k in S.KEYS[:-1]}, {k: got[k] for k in S.KEYS[:-1]}, f"packed {name}")
        assert pk["dev"].tobytes() == S.pack((got["dev"],), lens)[0].tobytes()
    assert (ref["sites"] < S.superpose_padded(h["pos"], h["mask"], pred, None, h["length"], 1)["sites"]).any()   # glycines are no CB site


def test_foldcomp_superpose(codec, records):
    import torch
    import foldcomp_amd as foldcomp
    n = len(records)
    t = foldcomp.decode_tensors(records, codec=codec)
    rng = np.random.default_rng(3)
    pred = to_dev(_moved(t["pos"].cpu().numpy(), rng, 0.5))
    model_out = dict(pos=pred, mask=t["mask"])
    out = foldcomp.superpose(model_out, t, apply=True, codec=codec)
    assert set(out) == {"rot", "trans", "rmsd", "sites", "dev", "gdt_counts", "gdt_ts", "gdt_ha", "tm", "pos_aligned"}
    assert out["rot"].shape == (n, 3, 3) and out["trans"].shape == (n, 3) and out["dev"].shape == (n, L_GOLD) and out["gdt_counts"].shape == (n, 5)
    assert out["sites"].dtype == torch.int32 and out["gdt_counts"].dtype == torch.int32 and out["pos_aligned"].shape == pred.shape
    assert all(out[k].dtype == torch.float32 and out[k].device.type == "cuda" for k in ("rot", "trans", "rmsd", "dev", "gdt_ts", "gdt_ha", "tm", "pos_aligned"))
    npy = {k: v.cpu().numpy() for k, v in out.items()}
    mask = t["mask"].cpu().numpy().view(np.uint8)
    length = t["length"].cpu().numpy()
    abi = S.run_dev(codec, t["pos"], t["mask"].view(torch.uint8), pred, t["mask"].view(torch.uint8), t["length"], n, L_GOLD, 0, 1, False)
    S.same_bytes({k: npy[k] for k in S.KEYS}, abi, "against the ABI call")
    ts, ha = S.gdt_scores(npy["gdt_counts"], npy["sites"])
    assert npy["gdt_ts"].tobytes() == ts.tobytes() and npy["gdt_ha"].tobytes() == ha.tobytes() and (ts >= ha).all() and 0.5 < ts.mean() < 1
    assert 0.5 < npy["rmsd"].mean() < 1.5 and (npy["tm"] > 0).all() and (npy["tm"] <= 1).all()
    exp = S.apply_expected(pred.cpu().numpy(), mask, npy["rot"], npy["trans"], length=length)
    assert npy["pos_aligned"].tobytes() == exp.tobytes()
    # the moved prediction lies on the target: its own superposition is the identity up to rounding, and lDDT, which is counted on
    # the target's own distances, sees the same pairs
    again = foldcomp.superpose(out["pos_aligned"], t, codec=codec)
    big = out["sites"] >= 10                                                  # (two or three sites leave the rotation free or nearly so)
    assert float((again["rot"] - torch.eye(3, device="cuda:0"))[big].abs().max()) < 1e-4 and float(again["trans"][big].abs().max()) < 1e-2
    assert float((again["rmsd"] - out["rmsd"]).abs().max()) < 1e-4 and int(big.sum()) > 40
    a, b = foldcomp.lddt(dict(pos=out["pos_aligned"], mask=t["mask"]), t, codec=codec), foldcomp.lddt(model_out, t, codec=codec)
    assert torch.equal(a["lddt_pairs"], b["lddt_pairs"]) and int(a["lddt_pairs"].sum()) > 0
    assert float((a["lddt_hits"] != b["lddt_hits"]).to(torch.float32).mean()) < 0.01          # (d_pred moves by float32 rounding only)
    # apply_transform alone, CB, pred as a bare tensor
    moved = foldcomp.apply_transform(model_out, out["rot"], out["trans"], t, codec=codec)
    assert torch.equal(moved, out["pos_aligned"])
    cb = foldcomp.superpose(pred, t, atom="CB", codec=codec)
    assert "pos_aligned" not in cb and (cb["sites"] <= out["sites"]).all() and (cb["sites"] < out["sites"]).any()
    # packed
    p = foldcomp.decode_tensors(records, codec=codec, packed=True)
    cu = p["cu_seqlens"].cpu().numpy()
    ppred = to_dev(np.concatenate([pred.cpu().numpy()[e, :cu[e + 1] - cu[e]] for e in range(n)]))
    po = foldcomp.superpose(ppred, p, apply=True, codec=codec)
    bare = foldcomp.superpose(pred, t, codec=codec)
    for k in ("rot", "trans", "rmsd", "sites", "gdt_counts", "tm", "gdt_ts", "gdt_ha"):
        assert torch.equal(po[k], bare[k]), k
    assert po["dev"].shape == (int(cu[-1]),) and po["pos_aligned"].shape == ppred.shape
    assert po["pos_aligned"].cpu().numpy().tobytes() == S.apply_expected(ppred.cpu().numpy(), None, po["rot"].cpu().numpy(), po["trans"].cpu().numpy(), row_off=cu).tobytes()
    assert torch.equal(foldcomp.apply_transform(ppred, po["rot"], po["trans"], cu_seqlens=p["cu_seqlens"], codec=codec), po["pos_aligned"])
    # a window: crop_start in the dict, length is not used
    w = foldcomp.decode_tensors(records, codec=codec, max_len=64, crop="center", layout="atom14")
    wpred = to_dev(_moved(w["pos"].cpu().numpy(), rng, 0.5))
    wo = foldcomp.superpose(dict(pos=wpred), w, codec=codec)
    wm = w["mask"].cpu().numpy().view(np.uint8)
    wref = S.superpose_padded(w["pos"].cpu().numpy(), wm, wpred.cpu().numpy(), None, None, 1)
    assert np.array_equal(wo["sites"].cpu().numpy(), wref["sites"]) and (wref["sites"][length > 64] == 64).all()
    # nothing to superpose
    e = foldcomp.superpose(torch.zeros((0, 8, 37, 3), device="cuda:0"), foldcomp.decode_tensors([], codec=codec, max_len=8), apply=True, codec=codec)
    assert e["rot"].shape == (0, 3, 3) and e["dev"].shape == (0, 8) and e["gdt_ts"].shape == (0,) and e["pos_aligned"].shape == (0, 8, 37, 3)
    e = foldcomp.decode_tensors([], codec=codec, packed=True)
    assert foldcomp.superpose(e["pos"], e, codec=codec)["rmsd"].shape == (0,)
    with pytest.raises(ValueError):
        foldcomp.superpose(pred[:, :, :14].contiguous(), t, codec=codec)
    with pytest.raises(ValueError):
        foldcomp.superpose(pred.transpose(0, 1).contiguous().transpose(0, 1), t, codec=codec)  # not contiguous
    with pytest.raises(foldcomp.error):
        foldcomp.superpose(pred.cpu(), t, codec=codec)
    with pytest.raises(foldcomp.error):
        foldcomp.apply_transform(pred.cpu(), out["rot"], out["trans"], t, codec=codec)
