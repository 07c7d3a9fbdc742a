"""GPU: the maximised GDT counts by seeded superposition search (fcz_gdt_dev, fcz_gdt_packed_dev, their host forms, Codec.gdt,
foldcomp.gdt) against the independent float64 numpy reference of the definition (tests/_gdt.py: stored selections, SVD, the best fit
kept as it is met). gdt_counts, sites, seed, run, selected and within are compared exactly, rot / trans per cutoff by
_superpose.close's tolerances (rot within 2^-22, trans within 2 float32 ulps), determinism, the two forms and the identities with
fcz_superpose_dev / fcz_tmscore_dev on bytes; the device calls write into arrays pre-filled with 0xA5 with guard bytes on both sides.

Why a float64 judge with another solver is fair to a search over thresholds: for every batch that is compared with the reference the
test asserts (_gdt.assert_fair) that (a) no deviation lies within 1e-8 A of a cut in any selection step, (b) at every fit whose
count at a cutoff reaches the chain's maximum - 1 no deviation lies within 1e-8 A of that cutoff, and (c) Horn's largest eigenvalue
is separated for every winning selection. Two float64 implementations differ by ~1e-10 A in dev, so both walk through the same
selections and count the same integers wherever the count can decide: seed, run and round of every winner are then the same, and the
winning fit is one Kabsch on a known set."""
import ctypes

import numpy as np
import pytest

import _analysis as AN
import _gdt as G
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
    """the seeded batch (chains of 0, 1, 2 rows, then random walks of 3 .. 257 rows, plain and hinged) on backbone4 / CA, padded and
    packed, with the reference: computed once, never changed"""
    n, ref, traces = G.gdt_batch_reference()
    lens, hinged, pos_t, mask, pos_p = (a[:n].copy() for a in T.tm_batch())     # (copies: torch takes no read-only array)
    L = 260                                                                      # (the batch's own width, 1027, only adds rows behind every length)
    pos_t, mask, pos_p = (np.ascontiguousarray(a[:, :L]) for a in (pos_t, mask, pos_p))
    ref = dict(ref, within=ref["within"][:, :L])
    return dict(lens=lens.astype(np.uint32), hinged=hinged, n=n, L=L, arrays=(pos_t, mask, pos_p), ref=ref, traces=traces, row_off=AN.row_off_of(lens),
                packed=SP.pack((pos_t, mask, pos_p), lens), solved=lens >= 3)


@pytest.fixture(scope="module")
def walk_dev(codec, walk):
    """the seeded batch on the device and fcz_gdt_dev's outputs for it, run once"""
    w = walk
    dev = [to_dev(a) for a in w["arrays"]] + [to_dev(w["lens"])]
    return dev, G.run_dev(codec, dev[0], dev[1], dev[2], None, dev[3], w["n"], w["L"], 2, 1, False)


def _less_within(d):
    return {k: v for k, v in d.items() if k != "within"}


def test_walks_padded_and_packed(codec, walk, walk_dev):
    w = walk
    (pt, mt, pp, dl), got = walk_dev
    a, b, c = G.assert_fair(w["arrays"][0], w["arrays"][2], 1, w["traces"], "walks")
    print(f"walks: (a) {a:.3g} A, (b) {b:.3g} A, (c) {c:.3g}; {sum(t['fits'] for t in w['traces'])} fits in the reference")
    print("walks, largest deviation from the float64 reference:", G.close(got, w["ref"], "padded", compare=np.repeat(w["solved"][:, None], 5, axis=1)))
    # (every (chain, cutoff) of the chains with three sites or more: (c) holds for all of them; two sites have no unique minimiser)
    SP.proper(got["rot"][w["solved"]], "padded")
    for k in range(5):
        assert np.array_equal((got["within"] >> k & 1).sum(axis=1), got["gdt_counts"][:, k]), k
    assert (np.diff(got["gdt_counts"], axis=1) >= 0).all()
    big = w["hinged"] & (w["lens"] >= 63)
    assert (got["seed"][big] > 0).any() and got["seed"].max() > 100 and len(np.unique(got["run"])) >= 3
    # the degenerate chains: none, one site, two sites
    eye5 = np.tile(np.eye(3, dtype=F), (5, 1, 1))
    assert got["rot"][0].tobytes() == eye5.tobytes() and not got["trans"][0].any() and got["sites"][0] == 0
    assert not any(got[k][0].any() for k in ("gdt_counts", "seed", "run", "selected", "within"))
    assert np.array_equal(got["rot"][1], eye5) and got["sites"][1] == 1 and (got["gdt_counts"][1] == 1).all() and (got["selected"][1] == 1).all()
    assert got["sites"][2] == 2 and (got["selected"][2] == 2).all()
    for e, m in enumerate(w["lens"]):
        assert not got["within"][e, m:].any()
    # determinism on bytes: the same call again, and the packed form
    SP.same_bytes(G.run_dev(codec, pt, mt, pp, None, dl, w["n"], w["L"], 2, 1, False), got, "second call")
    kt, km, kp = (to_dev(a) for a in w["packed"])
    R = int(w["row_off"][-1])
    pk = G.run_dev(codec, kt, km, kp, None, to_dev(w["row_off"]), w["n"], R, 2, 1, True)
    SP.same_bytes(_less_within(pk), _less_within(got), "packed")
    assert pk["within"].tobytes() == SP.pack((got["within"],), w["lens"])[0].tobytes()
    SP.same_bytes(G.run_dev(codec, kt, km, kp, None, to_dev(w["row_off"]), w["n"], R, 2, 1, True), pk, "packed, second call")


def test_a_chain_beyond_the_staged_rows_takes_the_global_path(codec):
    lens, hinged, pos_t, mask, pos_p = (a.copy() for a in T.tm_batch())
    long = np.flatnonzero(lens == 1027)
    assert len(long) == 2 and hinged[long].tolist() == [False, True]
    arrays = [np.ascontiguousarray(a[long]) for a in (pos_t, mask, pos_p)]
    ln = lens[long].astype(np.uint32)
    traces = []
    ref = G.gdt_padded(*arrays[:2], arrays[2], None, ln, 1, iterations=2, levels=3, traces=traces)
    print("1027 rows, levels = 3, iterations = 2: (a), (b), (c)", G.assert_fair(arrays[0], arrays[2], 1, traces, "1027 rows"))
    dev = [to_dev(a) for a in arrays]
    got = G.run_dev(codec, *dev, None, to_dev(ln), 2, 1027, 2, 1, False, iterations=2, levels=3)
    print("1027 rows:", G.close(got, ref, "1027 rows"))
    pk = G.run_dev(codec, *(to_dev(a) for a in SP.pack(arrays, ln)), None, to_dev(AN.row_off_of(ln)), 2, 2054, 2, 1, True, iterations=2, levels=3)
    SP.same_bytes(_less_within(pk), _less_within(got), "packed")
    assert pk["within"].tobytes() == got["within"].tobytes()


def _masked(rng, m=3 * 64 + 1, A=4, slot=1):
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


MASKED_SEED = 21          # (generator seeds 21 .. 24 all meet (a), (b), (c) for this chain)


def test_masks_and_hostile_bytes_change_nothing(codec):
    rng = np.random.default_rng(MASKED_SEED)
    m, L, dirty, clean, (nan_t, nan_p) = _masked(rng)
    length = np.asarray([m], np.uint32)
    traces = []
    ref = G.gdt_padded(*clean, length, 1, traces=traces)
    print("a chain of 3 * 64 + 1 rows: (a), (b), (c)", G.assert_fair(clean[0], clean[2], 1, traces, "masked"))
    assert 100 < ref["sites"][0] < 0.8 * m and (clean[1][0, :m, 1] != clean[3][0, :m, 1]).sum() > 30
    base = G.run_dev(codec, *(to_dev(a) for a in clean), to_dev(length), 1, L, 2, 1, False)
    print("a chain of 3 * 64 + 1 rows, sites cleared in one mask only:", G.close(base, ref, "clean"))
    # a non-finite coordinate at a site's slot in either tensor removes that site only
    got = G.run_dev(codec, *(to_dev(a) for a in dirty), to_dev(length), 1, L, 2, 1, False)
    SP.same_bytes(got, base, "a non-finite coordinate at a site")
    assert got["within"][0, nan_t] == 0 and got["within"][0, nan_p] == 0
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
        got = G.run_dev(codec, to_dev(pos_t), to_dev(mt), to_dev(pos_p), to_dev(mp), to_dev(length), 1, L, 2, 1, False)
        SP.same_bytes(got, base, f"poison {fill}")
        # packed: the chain in the middle of rows no chain covers, which hold the same poison
        row_off = np.asarray([20, 20 + m], np.uint32)
        shift = lambda a: np.concatenate([a[0, m:m + 20], a[0, :m], a[0, m + 20:]])
        pk = G.run_dev(codec, *(to_dev(shift(a)) for a in (pos_t, mt, pos_p, mp)), to_dev(row_off), 1, L, 2, 1, True)
        SP.same_bytes(_less_within(pk), _less_within(base), f"packed, poison {fill}")
        assert pk["within"][20:20 + m].tobytes() == base["within"][0, :m].tobytes() and not pk["within"][:20].any() and not pk["within"][20 + m:].any()


HOSTILE_SEED = 13


def _hostile(rng, R=700):
    x = SP.walk_chain(rng, R)
    y = x + 0.5 * rng.standard_normal(x.shape)
    y[500:] = (x[500:] - x[500]) @ T.rotation_about(rng.standard_normal(3), np.pi / 3).T + x[500] + 0.5 * rng.standard_normal((200, 3))
    return SP.in_slot(x.astype(F), 4, 1), np.ones((R, 4), np.uint8), SP.in_slot(y.astype(F), 4, 1)


def test_hostile_row_off(codec):
    R = 700
    pos_t, mask, pos_p = _hostile(np.random.default_rng(HOSTILE_SEED), R)
    dev = [to_dev(a) for a in (pos_t, mask, pos_p)]
    row_off = AN.HOSTILE_ROW_OFF
    kw = dict(iterations=3, levels=5)
    traces = []
    ref = G.gdt_packed(pos_t, mask, pos_p, None, row_off, 1, traces=traces, **kw)
    print("hostile row_off: (a), (b), (c)", G.assert_fair(pos_t, pos_p, 1, traces, "hostile row_off"))
    got = G.run_dev(codec, *dev, None, to_dev(row_off), 5, R, 2, 1, True, **kw)
    assert list(got["sites"]) == [0, 80, 280, 1, 299] == list(ref["sites"]) and not got["within"][:40].any()
    G.close(got, ref, "hostile row_off")
    # no chain at all: every row is uncovered
    none = G.run_dev(codec, *dev, None, to_dev(row_off), 0, R, 2, 1, True, want=("gdt_counts", "within"), **kw)
    assert not none["within"].any()

    def host_form(arrays, off, n, rows):
        """fcz_gdt_packed on host arrays (pos_true, mask_true, pos_pred), its outputs between guard bytes"""
        from foldcomp_amd.structure import CGdtOut
        h = HostGuarded(G.out_spec(n, rows, True))
        o = CGdtOut(*h.ptrs())
        assert codec.lib.fcz_gdt_packed(codec.ctx, *(host_ptr(a) for a in arrays), None, host_ptr(off), n, rows, 2, 1, 5, 3, 63, ctypes.byref(o)) == 0
        return {k: h.fetch(k) for k in G.KEYS}

    SP.same_bytes(host_form((pos_t, mask, pos_p), row_off, 5, R), got, "fcz_gdt_packed n=5")
    host = host_form((pos_t, mask, pos_p), row_off, 0, R)
    SP.same_bytes({k: host[k] for k in none}, none, "fcz_gdt_packed n=0")
    # chains without a row (R = 0): the per-chain outputs of an empty chain in both forms
    one, zeros = (pos_t[:1], mask[:1], pos_p[:1]), np.zeros(4, np.uint32)
    empty = G.run_dev(codec, *(to_dev(a) for a in one), None, to_dev(zeros), 3, 0, 2, 1, True)
    G.close(empty, G._empty(3, (0,)), "R = 0")
    assert empty["rot"].tobytes() == np.tile(np.eye(3, dtype=F), (3, 5, 1, 1)).tobytes() and not empty["trans"].view(np.uint32).any()
    SP.same_bytes(host_form(one, zeros, 3, 0), empty, "fcz_gdt_packed R=0")
    # ranges that overlap: no scratch scales with the seeds, so each of them has its full result
    lone = G.run_dev(codec, *dev, None, to_dev(np.asarray([0, R], np.uint32)), 1, R, 2, 1, True, want=G.KEYS[:-1], iterations=1, levels=4)
    twice = G.run_dev(codec, *dev, None, to_dev(np.asarray([0, R, 0, R], np.uint32)), 3, R, 2, 1, True, want=G.KEYS[:-1], iterations=1, levels=4)
    assert list(twice["sites"]) == [R, 0, R]
    for k in G.KEYS[:-1]:
        assert twice[k][0].tobytes() == lone[k][0].tobytes() == twice[k][2].tobytes(), k


def test_a_recount_from_the_float32_transforms(walk, walk_dev):
    """the five counts recomputed in float64 numpy from the device's own float32 rot / trans, for the chains that lie within 200 A of
    the origin: entries off by at most 2^-25 move a point there by at most 2.4e-5 A, so only a site whose deviation under the float64
    reference transform lies within 1e-3 A of the cutoff may fall on the other side of it"""
    w = walk
    got, ref = walk_dev[1], w["ref"]
    pos_t, _, pos_p = w["arrays"]
    checked = 0
    for e, m in enumerate(w["lens"]):
        a, b = pos_p[e, :m, 1].astype(np.float64), pos_t[e, :m, 1].astype(np.float64)
        if m == 0 or max(np.abs(a).max(), np.abs(b).max()) > 200.0:
            continue
        for k, c in enumerate(G.CUTOFFS):
            dev = np.sqrt((((a @ got["rot"][e, k].astype(np.float64).T + got["trans"][e, k].astype(np.float64)) - b) ** 2).sum(axis=1))
            exact = np.sqrt((((a @ ref["rot"][e, k].T + ref["trans"][e, k]) - b) ** 2).sum(axis=1))
            assert abs(int((dev <= c).sum()) - int(got["gdt_counts"][e, k])) <= int((np.abs(exact - c) < 1e-3).sum()), (e, m, k)
        checked += 1
    assert checked >= 20, checked


def test_identities_with_superpose_and_tmscore_on_bytes(codec, walk, walk_dev):
    w = walk
    (pt, mt, pp, dl), got = walk_dev
    n, L = w["n"], w["L"]
    kab = SP.run_dev(codec, pt, mt, pp, None, dl, n, L, 2, 1, False)
    tm = T.run_dev(codec, pt, mt, pp, None, dl, n, L, 2, 1, False)
    # levels = 1, iterations = 0: fcz_superpose_dev's counts, and its transform in all five places, whatever the runs
    for runs in (G.RUNS_ALL, G.RUNS_TM, 1 << 4):
        one = G.run_dev(codec, pt, mt, pp, None, dl, n, L, 2, 1, False, iterations=0, levels=1, runs=runs)
        assert one["gdt_counts"].tobytes() == kab["gdt_counts"].tobytes() and one["sites"].tobytes() == kab["sites"].tobytes()
        for k in range(5):
            assert one["rot"][:, k].tobytes() == kab["rot"].tobytes() and one["trans"][:, k].tobytes() == kab["trans"].tobytes(), k
            assert np.array_equal((one["within"] >> k & 1).sum(axis=1), kab["gdt_counts"][:, k]), k
        assert not one["seed"].any() and np.array_equal(one["selected"], np.repeat(one["sites"][:, None], 5, axis=1))
        assert (one["run"][w["lens"] > 0] == (runs & -runs).bit_length() - 1).all()
    kt, km, kp = (to_dev(a) for a in w["packed"])
    R = int(w["row_off"][-1])
    one = G.run_dev(codec, kt, km, kp, None, to_dev(w["row_off"]), n, R, 2, 1, True, iterations=0, levels=1)
    assert one["gdt_counts"].tobytes() == SP.run_dev(codec, kt, km, kp, None, to_dev(w["row_off"]), n, R, 2, 1, True)["gdt_counts"].tobytes()
    # never below the counts at the least-squares fit, nor (with the TM run) below those at the TM-maximising fit
    assert (got["gdt_counts"] >= kab["gdt_counts"]).all() and (got["gdt_counts"] >= tm["gdt_counts"]).all()
    big = w["hinged"] & (w["lens"] >= 63)
    assert (got["gdt_counts"][big].sum(axis=1) > kab["gdt_counts"][big].sum(axis=1)).all()
    only = G.run_dev(codec, pt, mt, pp, None, dl, n, L, 2, 1, False, runs=G.RUNS_TM)
    assert (only["gdt_counts"] >= tm["gdt_counts"]).all() and (only["gdt_counts"] <= got["gdt_counts"]).all() and not only["run"].any()
    for runs in (1 << 1, 1 << 5, 0b101010):
        part = G.run_dev(codec, pt, mt, pp, None, dl, n, L, 2, 1, False, runs=runs, want=("gdt_counts", "run"))
        assert (part["gdt_counts"] >= kab["gdt_counts"]).all() and (part["gdt_counts"] <= got["gdt_counts"]).all()
        assert ((runs >> part["run"][w["lens"] > 0]) & 1).all() and not part["run"][0].any()
    # fewer levels or rounds are the reference's with as many
    keep = w["lens"] <= 129
    arrays = [a[keep] for a in w["arrays"]]
    few = G.run_dev(codec, *(to_dev(a) for a in arrays), None, to_dev(w["lens"][keep]), int(keep.sum()), L, 2, 1, False, iterations=2, levels=3, runs=0b001101)
    traces = []
    ref = G.gdt_padded(*arrays[:2], arrays[2], None, w["lens"][keep], 1, iterations=2, levels=3, runs=0b001101, traces=traces)
    G.assert_fair(arrays[0], arrays[2], 1, traces, "levels = 3, iterations = 2, runs 0, 2, 3")
    G.close(few, dict(ref, within=ref["within"][:, :L]), "levels = 3, iterations = 2, runs 0, 2, 3", compare=np.repeat(w["solved"][keep][:, None], 5, axis=1))
    assert (few["gdt_counts"] <= got["gdt_counts"][keep]).all()


def test_host_forms_and_optional_outputs(codec, walk, walk_dev):
    w = walk
    keep = w["lens"] <= 129                                                   # (the staging is what is tested)
    arrays = [a[keep] for a in w["arrays"]]
    lens = w["lens"][keep]
    got = {k: v[keep] for k, v in walk_dev[1].items()}
    h = codec.gdt(arrays[0], arrays[1], arrays[2], None, 1, length=lens)
    SP.same_bytes({k: h[k] for k in G.KEYS}, got, "fcz_gdt")
    h = codec.gdt(*SP.pack(arrays, lens), None, 1, row_off=AN.row_off_of(lens))
    SP.same_bytes({k: h[k] for k in G.KEYS[:-1]}, _less_within(got), "fcz_gdt_packed")
    assert h["within"].tobytes() == SP.pack((got["within"],), lens)[0].tobytes()
    for bad in (dict(levels=0), dict(iterations=65), dict(runs="some"), dict(runs=())):
        with pytest.raises(ValueError):
            codec.gdt(arrays[0], arrays[1], arrays[2], None, 1, length=lens, **bad)
    # a chain's result does not depend on the batch around it
    sel = np.flatnonzero((w["lens"] >= 63) & (w["lens"] <= 65))
    pos_t, mask, pos_p = (a[sel].copy() for a in w["arrays"])
    ln = w["lens"][sel]
    dev = [to_dev(a) for a in (pos_t, mask, pos_p)]
    without = G.run_dev(codec, *dev, None, to_dev(ln), len(sel), w["L"], 2, 1, False)
    SP.same_bytes(without, {k: v[sel] for k, v in walk_dev[1].items()}, "a chain's result does not depend on the batch around it")
    # NULL optional outputs leave the others unchanged
    for want in (("gdt_counts",), ("gdt_counts", "within"), ("gdt_counts", "rot", "trans"), ("gdt_counts", "sites", "seed"), ("gdt_counts", "run", "selected"),
                 ("gdt_counts", "trans", "within", "selected")):
        part = G.run_dev(codec, *dev, None, to_dev(ln), len(sel), w["L"], 2, 1, False, want=want)
        SP.same_bytes(part, {k: without[k] for k in want}, f"only {want}")


def test_refusals_leave_the_outputs_untouched(codec):
    import torch
    from foldcomp_amd.structure import CGdtOut
    n, L, A = 2, 8, 37
    pos, mask, _, off = AN.refusal_inputs(n, L, A)
    g = DevGuarded(G.out_spec(n, L, False))
    out = CGdtOut(*(g.ptr(k) for k in G.KEYS))
    no_counts = CGdtOut(None, *(g.ptr(k) for k in G.KEYS[1:]))
    lib, ctx, P, M, O = codec.lib, codec.ctx, pos.data_ptr(), mask.data_ptr(), off.data_ptr()
    ok = dict(ctx=ctx, pt=P, mt=M, pp=P, mp=M, bound=None, n=n, L=L, layout=0, slot=1, levels=0, iterations=20, runs=63, out=ctypes.byref(out))
    bad = [dict(ctx=None), dict(pt=None), dict(mt=None), dict(pp=None), dict(out=None), dict(out=ctypes.byref(no_counts)),
           dict(layout=3), dict(layout=-1), dict(slot=37), dict(slot=-1), dict(layout=1, slot=14), dict(layout=2, slot=4), dict(L=2 ** 31),
           dict(iterations=65), dict(iterations=2 ** 31), dict(runs=0), dict(runs=64), dict(runs=2 ** 31), dict(L=0)]
    torch.cuda.synchronize()
    for b in bad:
        assert lib.fcz_gdt_dev(*dict(ok, **b).values()) == -1, b
    for b in bad[:-1]:
        a = dict(ok, bound=O, L=n * L)
        a.update(b)
        assert lib.fcz_gdt_packed_dev(*a.values()) == -1, b
    assert lib.fcz_gdt_packed_dev(*dict(ok, L=n * L).values()) == -1                              # chains without a row_off
    assert lib.fcz_gdt_dev(*dict(ok, n=0).values()) == 0 and lib.fcz_gdt_packed_dev(*dict(ok, bound=O, n=0, L=0).values()) == 0
    codec.synchronize()
    assert g.untouched()
    # the largest number of rounds that is accepted runs
    assert lib.fcz_gdt_dev(*dict(ok, iterations=64).values()) == 0
    codec.synchronize()
    assert not g.untouched()


# ---- the golden records and the Python surface -------------------------------------------------------------------------------------

L_GOLD = 96
N_GOLD = 8


@pytest.fixture(scope="module")
def records(golden):
    """the first golden records of 8 .. L_GOLD residues: a reference of the whole search costs seeds x runs x rounds"""
    z = golden[0]
    short = [e for n, e in zip(*golden_records_raw(golden)) if 8 <= len(z[f"{n}/fasta"]) <= L_GOLD][:N_GOLD]
    assert len(short) == N_GOLD
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
    """golden records against themselves, hinged and moved, in atom37 on CA and CB against the reference, and in atom14 and backbone4
    on CA against atom37 on bytes (the same coordinates in another layout). The reference meets (a) and (b) for every one of these
    records under generator seed 17, on CA and on CB, which the test asserts: all integers and `within` are exact. The transforms are
    compared where (c) holds, and at most a quarter of the (chain, cutoff) pairs with three sites or more may be left out"""
    dec = Decoded(codec, records)
    h = dec.dense("atom37", L_GOLD, want=("pos", "mask", "length"))
    rng = np.random.default_rng(17)
    pred = _moved(h["pos"], h["length"], rng, 0.5)
    n = len(records)
    dl = to_dev(h["length"])
    dev = [to_dev(a) for a in (h["pos"], h["mask"], pred)]
    lens = np.minimum(h["length"].astype(np.int64), L_GOLD)
    by_slot = {}
    for slot, name in ((1, "CA"), (3, "CB")):
        traces = []
        ref = G.gdt_padded(h["pos"], h["mask"], pred, None, h["length"], slot, traces=traces)
        a, b, c = G.fair(h["pos"], pred, slot, traces)
        fair = (a >= G.MARGIN) & (b >= G.MARGIN)
        assert fair.all(), (name, a, b)                                       # (the records and the generator seed were picked so that every one is judged)
        got = by_slot[slot] = G.run_dev(codec, *dev, None, dl, n, L_GOLD, 0, slot, False)
        compare = (c >= G.GAP) & (ref["selected"] >= 3)
        solved = np.repeat((ref["sites"] >= 3)[:, None], 5, axis=1)
        left_out = int((solved & ~compare)[fair].sum())
        print(f"golden records, {name}: {int(fair.sum())} of {n} records judged, {left_out} of {int(solved[fair].sum())} transforms left out; (a) {a[fair].min():.3g} (b) {b[fair].min():.3g}")
        assert left_out * 4 <= solved[fair].sum()
        print(f"golden records, {name}:", G.close({k: v[fair] for k, v in got.items()}, {k: v[fair] for k, v in ref.items()}, name, compare=compare[fair]))
        for k in range(5):
            assert np.array_equal((got["within"] >> k & 1).sum(axis=1), got["gdt_counts"][:, k]), k
        row_off = AN.row_off_of(lens)
        pk = G.run_dev(codec, *(to_dev(a) for a in SP.pack((h["pos"], h["mask"], pred), lens)), None, to_dev(row_off), n, int(row_off[-1]), 0, slot, True)
        SP.same_bytes(_less_within(pk), _less_within(got), f"packed {name}")
        assert pk["within"].tobytes() == SP.pack((got["within"],), lens)[0].tobytes()
    assert (by_slot[3]["sites"] < by_slot[1]["sites"]).any() and (by_slot[1]["seed"] > 0).any()   # glycines are no CB site
    for layout, lay, A in (("atom14", 1, 14), ("backbone4", 2, 4)):
        o = dec.dense(layout, L_GOLD, want=("pos", "mask", "length"))
        assert np.array_equal(o["pos"][:, :, 1], h["pos"][:, :, 1])
        p = np.zeros(o["pos"].shape, F)
        p[:, :, 1] = pred[:, :, 1]
        got = G.run_dev(codec, to_dev(o["pos"]), to_dev(o["mask"]), to_dev(p), None, dl, n, L_GOLD, lay, 1, False)
        SP.same_bytes(got, by_slot[1], layout)


def test_foldcomp_gdt(codec, records):
    import torch
    import foldcomp_amd as foldcomp
    n = len(records)
    t = foldcomp.decode_tensors(records, codec=codec)
    Lt = t["pos"].shape[1]
    rng = np.random.default_rng(3)
    length = t["length"].cpu().numpy()
    pred = to_dev(_moved(t["pos"].cpu().numpy(), length, rng, 0.5))
    model_out = dict(pos=pred, mask=t["mask"])
    out = foldcomp.gdt(model_out, t, codec=codec)
    assert set(out) == {"gdt_counts", "sites", "rot", "trans", "seed", "run", "selected", "within", "gdt_ts", "gdt_ha"}
    assert out["rot"].shape == (n, 5, 3, 3) and out["trans"].shape == (n, 5, 3) and out["within"].shape == (n, Lt) and out["within"].dtype == torch.uint8
    assert all(out[k].dtype == torch.int32 and out[k].shape == (n, 5) for k in ("gdt_counts", "seed", "run", "selected")) and out["sites"].shape == (n,)
    assert all(out[k].dtype == torch.float32 and out[k].device.type == "cuda" for k in ("rot", "trans", "gdt_ts", "gdt_ha"))
    npy = {k: v.cpu().numpy() for k, v in out.items()}
    m8 = t["mask"].view(torch.uint8)
    abi = G.run_dev(codec, t["pos"], m8, pred, m8, t["length"], n, Lt, 0, 1, False)
    SP.same_bytes({k: npy[k] for k in G.KEYS}, abi, "against the ABI call")
    ts, ha = SP.gdt_scores(npy["gdt_counts"], npy["sites"])
    assert npy["gdt_ts"].tobytes() == ts.tobytes() and npy["gdt_ha"].tobytes() == ha.tobytes()
    # against superpose and tm_score: never fewer, more somewhere; levels = 1, iterations = 0 is superpose
    kab = foldcomp.superpose(model_out, t, codec=codec)
    tm = foldcomp.tm_score(model_out, t, codec=codec)
    assert bool((out["gdt_counts"] >= kab["gdt_counts"]).all()) and bool((out["gdt_counts"] >= tm["gdt_counts"]).all())
    assert bool((out["gdt_ts"] >= tm["gdt_ts"]).all()) and bool((out["gdt_ts"] > kab["gdt_ts"]).any())
    one = foldcomp.gdt(model_out, t, iterations=0, levels=1, codec=codec)
    assert torch.equal(one["gdt_counts"], kab["gdt_counts"]) and torch.equal(one["gdt_ts"], kab["gdt_ts"]) and torch.equal(one["gdt_ha"], kab["gdt_ha"])
    assert all(torch.equal(one["rot"][:, k], kab["rot"]) and torch.equal(one["trans"][:, k], kab["trans"]) for k in range(5))
    # runs
    only = foldcomp.gdt(model_out, t, runs="tm", codec=codec)
    assert bool((only["gdt_counts"] >= tm["gdt_counts"]).all()) and bool((only["gdt_counts"] <= out["gdt_counts"]).all()) and not bool(only["run"].any())
    some = foldcomp.gdt(pred, t, runs=(1, 4.0), atom="CB", iterations=3, levels=2, codec=codec)
    assert bool(((some["run"] == 2) | (some["run"] == 4) | (some["sites"][:, None] == 0)).all()) and bool((some["sites"] <= out["sites"]).all())
    # the apply_transform recipe of the docstring: the prediction moved by the k-th transform lies within cutoff k where `within` says so
    k = 2
    moved = foldcomp.apply_transform(pred, out["rot"][:, k].contiguous(), out["trans"][:, k].contiguous(), t, codec=codec)
    exp = SP.apply_expected(pred.cpu().numpy(), None, npy["rot"][:, k].copy(), npy["trans"][:, k].copy(), length=length)
    assert moved.cpu().numpy().tobytes() == exp.tobytes() and exp.any()
    d = np.sqrt(((exp[:, :, 1].astype(np.float64) - t["pos"].cpu().numpy()[:, :, 1]) ** 2).sum(axis=-1))
    site = (np.arange(Lt)[None, :] < length[:, None]) & (t["mask"].cpu().numpy()[:, :, 1] != 0)
    bit = (npy["within"] >> k & 1).astype(bool)
    assert not (bit & ~site).any() and (d[bit] <= G.CUTOFFS[k] + 1e-3).all() and (d[site & ~bit] > G.CUTOFFS[k] - 1e-3).all()
    # packed
    p = foldcomp.decode_tensors(records, codec=codec, packed=True)
    cu = p["cu_seqlens"].cpu().numpy()
    ppred = to_dev(np.concatenate([pred.cpu().numpy()[e, :cu[e + 1] - cu[e]] for e in range(n)]))
    po = foldcomp.gdt(ppred, p, codec=codec)
    bare = foldcomp.gdt(pred, t, codec=codec)
    for key in ("gdt_counts", "sites", "rot", "trans", "seed", "run", "selected", "gdt_ts", "gdt_ha"):
        assert torch.equal(po[key], bare[key]), key
    assert po["within"].shape == (int(cu[-1]),)
    assert po["within"].cpu().numpy().tobytes() == np.concatenate([bare["within"].cpu().numpy()[e, :cu[e + 1] - cu[e]] for e in range(n)]).tobytes()
    # nothing to score
    e = foldcomp.gdt(torch.zeros((0, 8, 37, 3), device="cuda:0"), foldcomp.decode_tensors([], codec=codec, max_len=8), codec=codec)
    assert e["rot"].shape == (0, 5, 3, 3) and e["within"].shape == (0, 8) and e["seed"].shape == (0, 5) and e["gdt_ts"].shape == (0,)
    with pytest.raises(ValueError):
        foldcomp.gdt(pred, t, runs="some", codec=codec)
    with pytest.raises(foldcomp.error):
        foldcomp.gdt(pred.cpu(), t, codec=codec)
