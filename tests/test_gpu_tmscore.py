"""GPU: the maximised TM-score by seeded iterative superposition (fcz_tmscore_dev, fcz_tmscore_packed_dev, their host forms,
Codec.tm_score, foldcomp.tm_score) against the independent float64 numpy reference of the definition (tests/_tmscore.py: stored
selections, SVD). sites, gdt_counts, seed and selected are compared exactly, the float outputs by _superpose.close's tolerance
(2 float32 ulps, rot within 2^-22, floor 1e-8 A), determinism, the two forms and the one-level call on bytes; the device calls write
into arrays pre-filled with 0xA5 with guard bytes on both sides.

Why a float64 judge with another solver is fair to a search with thresholds: for every batch that is compared with the reference the
test asserts (seeded batch: tests/test_tmscore_cpu.py; the others: here, _tmscore.assert_fair) that no deviation lies within 1e-8 A
of a cut in any selection step, that every (seed, round) within 1e-9 of a chain's maximum has the winner's selection, and that Horn's
largest eigenvalue is separated for the winning selection. Two float64 implementations differ by ~1e-10 A in dev, so both walk through
the same selections, and the winning fit is one Kabsch on a known set: what _superpose.close's tolerance was derived for."""
import numpy as np
import pytest

import _analysis as AN
import _superpose as SP
import _tmscore as T
from _cases import golden_records_raw
from _devpath import DevGuarded, HostGuarded, host_ptr, to_dev
from _window import Decoded

pytestmark = pytest.mark.gpu

F = np.float32
POISON = (np.nan, np.inf, -np.inf)


@pytest.fixture(scope="module")
def walk():
    """the seeded batch (chains of 0, 1, 2 rows, then random walks of 3 .. 1027 rows, plain and hinged) on backbone4 / CA, padded and
    packed, with the reference: computed once, never changed"""
    lens, hinged, pos_t, mask, pos_p = (a.copy() for a in T.tm_batch())          # (copies: torch takes no read-only array)
    ref, _ = T.tm_batch_reference()
    row_off = AN.row_off_of(lens)
    return dict(lens=lens.astype(np.uint32), hinged=hinged, n=len(lens), L=pos_t.shape[1], arrays=(pos_t, mask, pos_p), ref=ref, row_off=row_off,
                packed=SP.pack((pos_t, mask, pos_p), lens), solved=lens >= 3)


@pytest.fixture(scope="module")
def walk_dev(codec, walk):
    """the seeded batch on the device and fcz_tmscore_dev's outputs for it, run once"""
    w = walk
    dev = [to_dev(a) for a in w["arrays"]] + [to_dev(w["lens"])]
    return dev, T.run_dev(codec, dev[0], dev[1], dev[2], None, dev[3], w["n"], w["L"], 2, 1, False)


def _exact(got, ref, what):
    for k in ("seed", "selected"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), (what, k, np.argwhere(got[k] != ref[k])[:4], got[k][got[k] != ref[k]][:4], ref[k][got[k] != ref[k]][:4])


def _show(what, seen):
    print(f"{what}: largest deviation from the float64 reference rounded to float32: " +
          ", ".join(f"{k} {v:.3g}{'' if k == 'rot' else ' ulp'}" for k, v in seen.items()))


def test_walks_padded_and_packed(codec, walk, walk_dev):
    w = walk
    (pt, mt, pp, dl), got = walk_dev
    _exact(got, w["ref"], "padded")
    _show("walks, padded", SP.close(got, w["ref"], "padded", compare_rot=w["solved"]))
    SP.proper(got["rot"], "padded")
    assert (got["seed"][w["hinged"] & (w["lens"] >= 63)] > 0).any() and got["seed"].max() > 100
    # the degenerate chains: none, one site, two sites
    eye = np.eye(3, dtype=F)
    assert got["rot"][0].tobytes() == eye.tobytes() and not got["trans"][0].any() and got["sites"][0] == 0 and got["rmsd"][0] == 0 and got["tm"][0] == 0
    assert got["seed"][0] == 0 and got["selected"][0] == 0
    assert np.array_equal(got["rot"][1], eye) and got["sites"][1] == 1 and got["rmsd"][1] == 0 and got["tm"][1] == 1 and got["selected"][1] == 1
    assert got["sites"][2] == 2 and got["selected"][2] == 2
    for e, m in enumerate(w["lens"]):
        assert not got["dev"][e, m:].view(np.uint32).any()
    # never below the TM-score at the least-squares superposition, on the float32 values
    kab = SP.run_dev(codec, pt, mt, pp, None, dl, w["n"], w["L"], 2, 1, False)
    assert (got["tm"] >= kab["tm"]).all() and (got["tm"][w["hinged"] & (w["lens"] >= 63)] > kab["tm"][w["hinged"] & (w["lens"] >= 63)]).all()
    # determinism on bytes: the same call again, and the packed form
    SP.same_bytes(T.run_dev(codec, pt, mt, pp, None, dl, w["n"], w["L"], 2, 1, False), got, "second call")
    kt, km, kp = (to_dev(a) for a in w["packed"])
    R = int(w["row_off"][-1])
    pk = T.run_dev(codec, kt, km, kp, None, to_dev(w["row_off"]), w["n"], R, 2, 1, True)
    SP.same_bytes({k: pk[k] for k in T.KEYS if k != "dev"}, {k: got[k] for k in T.KEYS if k != "dev"}, "packed")
    assert pk["dev"].tobytes() == SP.pack((got["dev"],), w["lens"])[0].tobytes()
    SP.same_bytes(T.run_dev(codec, kt, km, kp, None, to_dev(w["row_off"]), w["n"], R, 2, 1, True), pk, "packed, second call")


def test_host_forms_give_the_same_bytes(codec, walk, walk_dev):
    w = walk
    keep = w["lens"] <= 257                                                   # (the staging is what is tested: the long chains add time only)
    arrays = [a[keep] for a in w["arrays"]]
    lens = w["lens"][keep]
    got = {k: v[keep] for k, v in walk_dev[1].items()}
    h = codec.tm_score(arrays[0], arrays[1], arrays[2], None, 1, length=lens)
    SP.same_bytes({k: h[k] for k in T.KEYS}, got, "fcz_tmscore")
    row_off = AN.row_off_of(lens)
    h = codec.tm_score(*SP.pack(arrays, lens), None, 1, row_off=row_off)
    SP.same_bytes({k: h[k] for k in T.KEYS if k != "dev"}, {k: got[k] for k in T.KEYS if k != "dev"}, "fcz_tmscore_packed")
    assert h["dev"].tobytes() == SP.pack((got["dev"],), lens)[0].tobytes()
    for bad in (dict(levels=0), dict(levels=1.0), dict(iterations=65), dict(iterations=True)):   # the integer rules of foldcomp.tm_score
        with pytest.raises(ValueError):
            codec.tm_score(arrays[0], arrays[1], arrays[2], None, 1, length=lens, **bad)


def test_one_level_and_no_iteration_is_fcz_superpose_on_bytes(codec, walk, walk_dev):
    w = walk
    pt, mt, pp, dl = walk_dev[0]
    one = T.run_dev(codec, pt, mt, pp, None, dl, w["n"], w["L"], 2, 1, False, iterations=0, levels=1)
    kab = SP.run_dev(codec, pt, mt, pp, None, dl, w["n"], w["L"], 2, 1, False)
    SP.same_bytes({k: one[k] for k in SP.KEYS}, kab, "levels = 1, iterations = 0")
    assert not one["seed"].any() and np.array_equal(one["selected"], one["sites"])
    kt, km, kp = (to_dev(a) for a in w["packed"])
    R = int(w["row_off"][-1])
    one = T.run_dev(codec, kt, km, kp, None, to_dev(w["row_off"]), w["n"], R, 2, 1, True, iterations=0, levels=1)
    SP.same_bytes({k: one[k] for k in SP.KEYS}, SP.run_dev(codec, kt, km, kp, None, to_dev(w["row_off"]), w["n"], R, 2, 1, True), "packed, levels = 1, iterations = 0")
    # fewer levels or rounds are the reference's with as many, and never score higher than more of them
    keep = (w["lens"] <= 129)
    few = T.run_dev(codec, to_dev(w["arrays"][0][keep]), to_dev(w["arrays"][1][keep]), to_dev(w["arrays"][2][keep]), None, to_dev(w["lens"][keep]), int(keep.sum()),
                    w["L"], 2, 1, False, iterations=2, levels=3)
    traces = []
    ref = T.tm_padded(w["arrays"][0][keep], w["arrays"][1][keep], w["arrays"][2][keep], None, w["lens"][keep], 1, iterations=2, levels=3, traces=traces)
    T.assert_fair(w["arrays"][0][keep], w["arrays"][2][keep], 1, traces, "levels = 3, iterations = 2")
    _exact(few, ref, "levels = 3, iterations = 2")
    SP.close(few, ref, "levels = 3, iterations = 2", compare_rot=w["solved"][keep])
    assert (few["tm"] <= walk_dev[1]["tm"][keep]).all()


def test_self_consistency_of_the_transform(walk, walk_dev):
    """dev and tm recomputed in float64 numpy from the device's own float32 rot / trans, for the chains that lie within 200 A of the
    origin: entries off by at most 2^-25 move a point there by at most 2.4e-5 A, and d tm / d dev <= 0.65 / d0 <= 1.3 per A, so dev
    agrees within 1e-4 A and tm within 1e-4"""
    w = walk
    got = walk_dev[1]
    pos_t, _, pos_p = w["arrays"]
    checked = 0
    for e, m in enumerate(w["lens"]):
        a, b = pos_p[e, :m, 1].astype(np.float64), pos_t[e, :m, 1].astype(np.float64)
        if m == 0 or max(np.abs(a).max(), np.abs(b).max()) > 200.0:
            continue
        dev = np.sqrt((((a @ got["rot"][e].astype(np.float64).T + got["trans"][e].astype(np.float64)) - b) ** 2).sum(axis=1))
        tm = float((1.0 / (1.0 + (dev / SP.d0_of(m)) ** 2)).sum() / m)
        assert np.abs(dev - got["dev"][e, :m]).max() <= 1e-4 and abs(tm - float(got["tm"][e])) <= 1e-4, (e, m)
        checked += 1
    assert checked >= 20, checked


def _poisoned(rng, m=3 * 64 + 1, A=4, slot=1):
    """one chain of 3 * 64 + 1 rows inside a padded entry of m + 40 rows, its last 3/8 hinged: ~15 % of the sites cleared in mask_true
    only, ~15 % in mask_pred only, a NaN at one site's slot in true and an inf at one in pred (both masks set), and the clean twin with
    those two sites cleared"""
    L = m + 40
    x = SP.walk_chain(rng, L)
    y = x.copy()
    at = m - (3 * m) // 8
    y[at:] = (x[at:] - x[at]) @ T.rotation_about(rng.standard_normal(3), np.pi / 3).T + x[at]
    y = y @ SP.random_rotation(rng).T + rng.uniform(-20, 20, 3) + 0.5 * rng.standard_normal((L, 3))
    pos_t, pos_p = SP.in_slot(x[None].astype(F), A, slot, 1.0), SP.in_slot(y[None].astype(F), A, slot, 2.0)
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
    traces = []
    ref = T.tm_padded(*clean, length, 1, traces=traces)
    print("a chain of 3 * 64 + 1 rows: margin, Horn gap, lead", T.assert_fair(clean[0], clean[2], 1, traces, "poisoned"))
    assert 100 < ref["sites"][0] < 0.8 * m and (clean[1][0, :m, 1] != clean[3][0, :m, 1]).sum() > 30
    base = T.run_dev(codec, *(to_dev(a) for a in clean), to_dev(length), 1, L, 2, 1, False)
    _exact(base, ref, "clean")
    _show("a chain of 3 * 64 + 1 rows, sites cleared in one mask only", SP.close(base, ref, "clean"))
    # a non-finite coordinate at a site's slot in either tensor removes that site only
    got = T.run_dev(codec, *(to_dev(a) for a in dirty), to_dev(length), 1, L, 2, 1, False)
    SP.same_bytes(got, base, "a non-finite coordinate at a site")
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
        got = T.run_dev(codec, to_dev(pos_t), to_dev(mt), to_dev(pos_p), to_dev(mp), to_dev(length), 1, L, 2, 1, False)
        SP.same_bytes(got, base, f"poison {fill}")
        # packed: the chain in the middle of rows no chain covers, which hold the same poison
        row_off = np.asarray([20, 20 + m], np.uint32)
        shift = lambda a: np.concatenate([a[0, m:m + 20], a[0, :m], a[0, m + 20:]])
        pk = T.run_dev(codec, *(to_dev(shift(a)) for a in (pos_t, mt, pos_p, mp)), to_dev(row_off), 1, L, 2, 1, True)
        SP.same_bytes({k: pk[k] for k in T.KEYS if k != "dev"}, {k: base[k] for k in T.KEYS if k != "dev"}, f"packed, poison {fill}")
        assert pk["dev"][20:20 + m].tobytes() == base["dev"][0, :m].tobytes() and not pk["dev"][:20].view(np.uint32).any()
        assert not pk["dev"][20 + m:].view(np.uint32).any()


def test_mask_pred_null_and_optional_outputs(codec, walk, walk_dev):
    w = walk
    sel = np.flatnonzero((w["lens"] >= 63) & (w["lens"] <= 65))               # the chains of 63, 64 and 65 rows, plain and hinged
    pos_t, mask, pos_p = (a[sel].copy() for a in w["arrays"])
    lens = w["lens"][sel]
    mp = mask.copy()
    mp[:, ::3, 1] = 0
    dev = [to_dev(a) for a in (pos_t, mask, pos_p)]
    with_mask = T.run_dev(codec, *dev, to_dev(mp), to_dev(lens), len(sel), w["L"], 2, 1, False)
    without = T.run_dev(codec, *dev, None, to_dev(lens), len(sel), w["L"], 2, 1, False)
    assert (without["sites"] == lens).all() and (with_mask["sites"] < lens).all()
    traces = []
    ref = T.tm_padded(pos_t, mask, pos_p, mp, lens, 1, traces=traces)
    T.assert_fair(pos_t, pos_p, 1, traces, "mask_pred")
    _exact(with_mask, ref, "mask_pred")
    SP.close(with_mask, ref, "mask_pred")
    SP.same_bytes(without, {k: v[sel] for k, v in walk_dev[1].items()}, "a chain's result does not depend on the batch around it")
    # NULL optional outputs leave the others unchanged
    for want in (("rot", "trans"), ("rot", "trans", "dev"), ("rot", "trans", "rmsd", "tm"), ("rot", "trans", "sites", "gdt_counts"), ("rot", "trans", "seed"),
                 ("rot", "trans", "selected", "tm")):
        part = T.run_dev(codec, *dev, None, to_dev(lens), len(sel), w["L"], 2, 1, False, want=want)
        SP.same_bytes(part, {k: without[k] for k in want}, f"only {want}")


def test_hostile_row_off(codec):
    rng = np.random.default_rng(13)
    R = 700
    x = SP.walk_chain(rng, R)
    y = x + 0.5 * rng.standard_normal(x.shape)
    y[500:] = (x[500:] - x[500]) @ T.rotation_about(rng.standard_normal(3), np.pi / 3).T + x[500] + 0.5 * rng.standard_normal((200, 3))
    pos_t, pos_p = SP.in_slot(x.astype(F), 4, 1), SP.in_slot(y.astype(F), 4, 1)
    mask = np.ones((R, 4), np.uint8)
    dev = [to_dev(a) for a in (pos_t, mask, pos_p)]
    row_off = AN.HOSTILE_ROW_OFF
    traces = []
    ref = T.tm_packed(pos_t, mask, pos_p, None, row_off, 1, traces=traces)
    T.assert_fair(pos_t, pos_p, 1, traces, "hostile row_off")
    got = T.run_dev(codec, *dev, None, to_dev(row_off), 5, R, 2, 1, True)
    assert list(got["sites"]) == [0, 80, 280, 1, 299] == list(ref["sites"]) and not got["dev"][:40].view(np.uint32).any()
    _exact(got, ref, "hostile row_off")
    SP.close(got, ref, "hostile row_off", compare_rot=got["sites"] >= 3)
    assert got["seed"][4] > 0                                                 # (the hinge lies in chain 4)
    # no chain at all: every row is uncovered
    none = T.run_dev(codec, *dev, None, to_dev(row_off), 0, R, 2, 1, True, want=("rot", "trans", "dev"))
    assert not none["dev"].view(np.uint32).any()

    def host_form(arrays, off, n, rows):
        """fcz_tmscore_packed on host arrays (pos_true, mask_true, pos_pred), its outputs between guard bytes"""
        import ctypes
        from foldcomp_amd.structure import CTmScoreOut
        h = HostGuarded(T.out_spec(n, rows, True))
        o = CTmScoreOut(*h.ptrs())
        assert codec.lib.fcz_tmscore_packed(codec.ctx, *(host_ptr(a) for a in arrays), None, host_ptr(off), n, rows, 2, 1, 0, 20, ctypes.byref(o)) == 0
        return {k: h.fetch(k) for k in T.KEYS}

    # the host form on the same arrays: what the device form gave
    SP.same_bytes(host_form((pos_t, mask, pos_p), row_off, 5, R), got, "fcz_tmscore_packed n=5")
    host = host_form((pos_t, mask, pos_p), row_off, 0, R)
    SP.same_bytes({k: host[k] for k in none}, none, "fcz_tmscore_packed n=0")
    # chains without a row (R = 0): the per-chain outputs of an empty chain in both forms
    one, zeros = (pos_t[:1], mask[:1], pos_p[:1]), np.zeros(4, np.uint32)
    empty = T.run_dev(codec, *(to_dev(a) for a in one), None, to_dev(zeros), 3, 0, 2, 1, True)
    SP.close(empty, T._empty(3, (0,)), "R = 0")
    assert not any(empty[k].view(np.uint32).any() for k in ("rmsd", "tm", "seed", "selected"))
    SP.same_bytes(host_form(one, zeros, 3, 0), empty, "fcz_tmscore_packed R=0")
    # ranges that overlap hold more seeds than the scratch, which is sized from R: nothing outside the outputs is written, the chain
    # whose seeds all fit has its full result, and the other the maximum over the seeds that fit (the header says so)
    lone = T.run_dev(codec, *dev, None, to_dev(np.asarray([0, R], np.uint32)), 1, R, 2, 1, True)
    kab = SP.run_dev(codec, *dev, None, to_dev(np.asarray([0, R], np.uint32)), 1, R, 2, 1, True)
    twice = T.run_dev(codec, *dev, None, to_dev(np.asarray([0, R, 0, R], np.uint32)), 3, R, 2, 1, True)
    assert 2 * codec.lib.fcz_tmscore_seeds(R, 0) > (17 * R) // 10 + 70 * 3 + 4 and list(twice["sites"]) == [R, 0, R]
    for k in T.KEYS:
        if k != "dev":
            assert twice[k][0].tobytes() == lone[k][0].tobytes(), k
    assert kab["tm"][0] <= twice["tm"][2] <= lone["tm"][0] and 0 <= twice["seed"][2] < codec.lib.fcz_tmscore_seeds(R, 0)
    SP.proper(twice["rot"], "overlapping ranges")


def test_refusals_leave_the_outputs_untouched(codec):
    import ctypes
    import torch
    from foldcomp_amd.structure import CTmScoreOut
    n, L, A = 2, 8, 37
    pos, mask, _, off = AN.refusal_inputs(n, L, A)
    g = DevGuarded(T.out_spec(n, L, False))
    out = CTmScoreOut(*(g.ptr(k) for k in T.KEYS))
    no_rot = CTmScoreOut(None, *(g.ptr(k) for k in T.KEYS[1:]))
    no_trans = CTmScoreOut(g.ptr("rot"), None, *(g.ptr(k) for k in T.KEYS[2:]))
    lib, ctx, P, M, O = codec.lib, codec.ctx, pos.data_ptr(), mask.data_ptr(), off.data_ptr()
    ok = dict(ctx=ctx, pt=P, mt=M, pp=P, mp=M, bound=None, n=n, L=L, layout=0, slot=1, levels=0, iterations=20, out=ctypes.byref(out))
    bad = [dict(ctx=None), dict(pt=None), dict(mt=None), dict(pp=None), dict(out=None), dict(out=ctypes.byref(no_rot)), dict(out=ctypes.byref(no_trans)),
           dict(layout=3), dict(layout=-1), dict(slot=37), dict(slot=-1), dict(layout=1, slot=14), dict(layout=2, slot=4), dict(L=2 ** 31),
           dict(iterations=65), dict(iterations=2 ** 31), dict(L=0)]
    torch.cuda.synchronize()
    for b in bad:
        assert lib.fcz_tmscore_dev(*dict(ok, **b).values()) == -1, b
    for b in bad[:-1]:
        a = dict(ok, bound=O, L=n * L)
        a.update(b)
        assert lib.fcz_tmscore_packed_dev(*a.values()) == -1, b
    assert lib.fcz_tmscore_packed_dev(*dict(ok, L=n * L).values()) == -1                      # chains without a row_off
    assert lib.fcz_tmscore_dev(*dict(ok, n=0).values()) == 0 and lib.fcz_tmscore_packed_dev(*dict(ok, bound=O, n=0, L=0).values()) == 0
    codec.synchronize()
    assert g.untouched()
    # the largest number of rounds that is accepted runs
    assert lib.fcz_tmscore_dev(*dict(ok, iterations=64).values()) == 0
    codec.synchronize()
    assert not g.untouched()


# ---- the golden records and the Python surface -------------------------------------------------------------------------------------

L_GOLD = 160


@pytest.fixture(scope="module")
def records(golden):
    """the first sixteen golden records of at most L_GOLD residues (2 .. 129): a reference of the whole search costs seeds x rounds"""
    z = golden[0]
    short = [e for n, e in zip(*golden_records_raw(golden)) if len(z[f"{n}/fasta"]) <= L_GOLD][:16]
    assert len(short) == 16
    return short


def _moved(pos, length, rng, noise):
    """pos float32 [n, L, A, 3] -> every entry with the last 3/8 of its residues swung by 60 degrees about the CA of the first of
    them (every second entry), under a random rigid motion of its own plus Gaussian noise, float32"""
    out = np.empty_like(pos)
    for e in range(len(pos)):
        x = pos[e].astype(np.float64)
        m = int(length[e])
        at = m - (3 * m) // 8
        if e % 2 and m >= 8:
            x[at:m] = (x[at:m] - x[at, 1]) @ T.rotation_about(rng.standard_normal(3), np.pi / 3).T + x[at, 1]
        out[e] = x @ SP.random_rotation(rng).T + rng.uniform(-40, 40, 3) + noise * rng.standard_normal(x.shape)
    return out


def test_golden_records(codec, records):
    """sixteen golden records against themselves, hinged and moved, in atom37 on CA and CB against the reference, and in atom14 and
    backbone4 on CA against atom37 on bytes (the same coordinates in another layout)"""
    dec = Decoded(codec, records)
    h = dec.dense("atom37", L_GOLD, want=("pos", "mask", "length"))
    rng = np.random.default_rng(17)
    pred = _moved(h["pos"], h["length"], rng, 0.5)
    n = len(records)
    dl = to_dev(h["length"])
    dev = [to_dev(a) for a in (h["pos"], h["mask"], pred)]
    by_slot = {}
    for slot, name in ((1, "CA"), (3, "CB")):
        traces = []
        ref = T.tm_padded(h["pos"], h["mask"], pred, None, h["length"], slot, traces=traces)
        print(f"golden records, {name}: margin, Horn gap, lead", T.assert_fair(h["pos"], pred, slot, traces, name))
        got = by_slot[slot] = T.run_dev(codec, *dev, None, dl, n, L_GOLD, 0, slot, False)
        _exact(got, ref, name)
        _show(f"golden records, {name}", SP.close(got, ref, name, compare_rot=ref["selected"] >= 3))
        SP.proper(got["rot"], name)
        lens = np.minimum(h["length"].astype(np.int64), L_GOLD)
        row_off = AN.row_off_of(lens)
        pk = T.run_dev(codec, *(to_dev(a) for a in SP.pack((h["pos"], h["mask"], pred), lens)), None, to_dev(row_off), n, int(row_off[-1]), 0, slot, True)
        SP.same_bytes({k: pk[k] for k in T.KEYS if k != "dev"}, {k: got[k] for k in T.KEYS if k != "dev"}, f"packed {name}")
        assert pk["dev"].tobytes() == SP.pack((got["dev"],), lens)[0].tobytes()
    assert (by_slot[3]["sites"] < by_slot[1]["sites"]).any() and (by_slot[1]["seed"] > 0).any()   # glycines are no CB site
    for layout, lay, A in (("atom14", 1, 14), ("backbone4", 2, 4)):
        o = dec.dense(layout, L_GOLD, want=("pos", "mask", "length"))
        assert np.array_equal(o["pos"][:, :, 1], h["pos"][:, :, 1])
        p = np.zeros(o["pos"].shape, F)
        p[:, :, 1] = pred[:, :, 1]
        got = T.run_dev(codec, to_dev(o["pos"]), to_dev(o["mask"]), to_dev(p), None, dl, n, L_GOLD, lay, 1, False)
        SP.same_bytes(got, by_slot[1], layout)


def test_foldcomp_tm_score(codec, records):
    import torch
    import foldcomp_amd as foldcomp
    n = len(records)
    t = foldcomp.decode_tensors(records, codec=codec)
    Lt = t["pos"].shape[1]
    rng = np.random.default_rng(3)
    length = t["length"].cpu().numpy()
    pred = to_dev(_moved(t["pos"].cpu().numpy(), length, rng, 0.5))
    model_out = dict(pos=pred, mask=t["mask"])
    out = foldcomp.tm_score(model_out, t, apply=True, codec=codec)
    assert set(out) == {"rot", "trans", "rmsd", "sites", "dev", "gdt_counts", "gdt_ts", "gdt_ha", "tm", "seed", "selected", "pos_aligned"}
    assert out["rot"].shape == (n, 3, 3) and out["trans"].shape == (n, 3) and out["dev"].shape == (n, Lt) and out["gdt_counts"].shape == (n, 5)
    assert all(out[k].dtype == torch.int32 and out[k].shape == (n,) for k in ("sites", "seed", "selected")) and out["gdt_counts"].dtype == torch.int32
    assert all(out[k].dtype == torch.float32 and out[k].device.type == "cuda" for k in ("rot", "trans", "rmsd", "dev", "gdt_ts", "gdt_ha", "tm", "pos_aligned"))
    npy = {k: v.cpu().numpy() for k, v in out.items()}
    mask = t["mask"].cpu().numpy().view(np.uint8)
    abi = T.run_dev(codec, t["pos"], t["mask"].view(torch.uint8), pred, t["mask"].view(torch.uint8), t["length"], n, Lt, 0, 1, False)
    SP.same_bytes({k: npy[k] for k in T.KEYS}, abi, "against the ABI call")
    ts, ha = SP.gdt_scores(npy["gdt_counts"], npy["sites"])
    assert npy["gdt_ts"].tobytes() == ts.tobytes() and npy["gdt_ha"].tobytes() == ha.tobytes()
    # pos_aligned on bits against the numpy apply step fed the device's own rot / trans
    exp = SP.apply_expected(pred.cpu().numpy(), mask, npy["rot"], npy["trans"], length=length)
    assert npy["pos_aligned"].tobytes() == exp.tobytes() and exp.any()
    # against superpose: never a lower tm, a higher one somewhere; levels = 1, iterations = 0 is superpose
    kab = foldcomp.superpose(model_out, t, codec=codec)
    assert bool((out["tm"] >= kab["tm"]).all()) and bool((out["tm"] > kab["tm"]).any()) and bool((out["seed"] > 0).any())
    one = foldcomp.tm_score(model_out, t, iterations=0, levels=1, codec=codec)
    for k in kab:
        assert torch.equal(one[k], kab[k]), k
    cb = foldcomp.tm_score(pred, t, atom="CB", iterations=3, levels=2, codec=codec)
    assert "pos_aligned" not in cb and (cb["sites"] <= out["sites"]).all() and (cb["sites"] < out["sites"]).any()
    # packed
    p = foldcomp.decode_tensors(records, codec=codec, packed=True)
    cu = p["cu_seqlens"].cpu().numpy()
    ppred = to_dev(np.concatenate([pred.cpu().numpy()[e, :cu[e + 1] - cu[e]] for e in range(n)]))
    po = foldcomp.tm_score(ppred, p, apply=True, codec=codec)
    bare = foldcomp.tm_score(pred, t, codec=codec)
    for k in ("rot", "trans", "rmsd", "sites", "gdt_counts", "tm", "gdt_ts", "gdt_ha", "seed", "selected"):
        assert torch.equal(po[k], bare[k]), k
    assert po["dev"].shape == (int(cu[-1]),) and po["pos_aligned"].shape == ppred.shape
    assert po["pos_aligned"].cpu().numpy().tobytes() == SP.apply_expected(ppred.cpu().numpy(), None, po["rot"].cpu().numpy(), po["trans"].cpu().numpy(), row_off=cu).tobytes()
    # nothing to score
    e = foldcomp.tm_score(torch.zeros((0, 8, 37, 3), device="cuda:0"), foldcomp.decode_tensors([], codec=codec, max_len=8), apply=True, codec=codec)
    assert e["rot"].shape == (0, 3, 3) and e["dev"].shape == (0, 8) and e["seed"].shape == (0,) and e["pos_aligned"].shape == (0, 8, 37, 3)
    with pytest.raises(ValueError):
        foldcomp.tm_score(pred, t, iterations=65, codec=codec)
    with pytest.raises(foldcomp.error):
        foldcomp.tm_score(pred.cpu(), t, codec=codec)
