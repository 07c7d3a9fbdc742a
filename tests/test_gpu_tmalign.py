"""GPU: the TM-align-style alignment of chain pairs (fcz_tmalign_dev, fcz_tmalign_dp_dev, their host forms, Codec.tm_align,
Codec.tm_align_dp, foldcomp.tm_align) against the independent numpy reference of the definition (tests/_tmalign.py: whole DP matrices,
stored alignments, SVD). The dynamic programme alone is integer and is compared on every byte of map and aligned. The full search is
compared exactly in map, aligned, seed, sites and status and by _superpose.close's tolerance in the floats; that a float64 judge with
another solver is fair to it is asserted for the seeded batch in tests/test_tmalign_cpu.py (no deviation within 1e-8 A of a cut, rounds that tie
within 1e-9 share their selection, Horn gap >= 1e-3 for every fit, every DP either without a score within 1e-7 of an integer or without a traceback decision won by 2 units or
less, the winner 1e-9 ahead of every candidate with another alignment). The device calls write into arrays pre-filled with 0xA5
between guard bytes."""
import numpy as np
import pytest

import _superpose as SP
import _tmalign as TA
from _cases import golden_records_raw
from _devpath import DevGuarded, HostGuarded

pytestmark = pytest.mark.gpu

F = np.float32
LAY, SLOT = 2, 1                                                               # backbone4, CA
DP_SIZES = ((0, 5), (1, 1), (1, 64), (63, 65), (64, 64), (65, 129), (129, 5))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dp_chains(sizes, seed):
    """for every (Sa, Sb) a random walk a and a chain b whose first min(Sa, Sb) residues are a's, moved rigidly, plus noise; the rest of
    b walks on -> (chains a, chains b, rot [m, 3, 3], trans [m, 3] float32: the motions)"""
    rng = np.random.default_rng(seed)
    ca, cb, rot, trans = [], [], [], []
    for sa, sb in sizes:
        a, b = SP.walk_chain(rng, sa), SP.walk_chain(rng, sb)
        r, t = SP.random_rotation(rng), rng.uniform(-30, 30, 3)
        k = min(sa, sb)
        b[:k] = a[:k] @ r.T + t + 0.3 * rng.standard_normal((k, 3))
        b[k:] += b[k - 1] - b[k] + 3.8 if 0 < k < sb else 0.0
        ca.append(a.astype(F)); cb.append(b.astype(F)); rot.append(r); trans.append(t)
    return ca, cb, np.asarray(rot, F), np.asarray(trans, F)


def _check_dp(codec, sa, sb, pairs, wa, wb, rot, trans, gap, what):
    da, db = TA.to_device(sa), TA.to_device(sb)
    got = TA.run_dp_dev(codec, da, db, _dev(pairs), wa, wb, LAY, SLOT, _dev(rot), _dev(trans), gap)
    ref = TA.dp_sets(sa, sb, pairs, wa, wb, SLOT, rot, trans, gap)
    assert got[0].tobytes() == ref[0].tobytes(), (what, np.argwhere(got[0] != ref[0])[:4])
    assert got[1].tobytes() == ref[1].tobytes(), (what, got[1], ref[1])
    return got


def test_dp_alone_is_exact_on_every_byte(codec):
    ca, cb, rot, trans = _dp_chains(DP_SIZES, 11)
    m = len(ca)
    pairs = np.stack([np.arange(m), np.arange(m)], axis=1).astype(np.int32)
    sa, sb = TA.padded_set(ca), TA.padded_set(cb)
    wa, wb = sa["pos"].shape[1], sb["pos"].shape[1]
    eye, zero = np.tile(np.eye(3, dtype=F), (m, 1, 1)), np.zeros((m, 3), F)
    far = zero + F(1e6)
    for gap in (0.0, 0.6):
        got = _check_dp(codec, sa, sb, pairs, wa, wb, rot, trans, gap, f"motion, gap {gap}")
        # the planted prefix is found: most of the shorter chain is aligned
        assert (got[1][1:] >= np.asarray([min(s) for s in DP_SIZES[1:]]) * 0.8).all(), got[1]
        _check_dp(codec, sa, sb, pairs, wa, wb, eye, zero, gap, f"identity, gap {gap}")
        far_got = _check_dp(codec, sa, sb, pairs, wa, wb, eye, far, gap, f"far away, gap {gap}")
    assert gap == 0.6 and not far_got[1].any() and (far_got[0] == -1).all()       # every q is 0 and a gap costs: nothing is aligned
    # the same call twice, and padded against packed in either set, on bytes
    da, db, pt = TA.to_device(sa), TA.to_device(sb), _dev(pairs)
    one = TA.run_dp_dev(codec, da, db, pt, wa, wb, LAY, SLOT, _dev(rot), _dev(trans), 0.6)
    two = TA.run_dp_dev(codec, da, db, pt, wa, wb, LAY, SLOT, _dev(rot), _dev(trans), 0.6)
    assert one[0].tobytes() == two[0].tobytes() and one[1].tobytes() == two[1].tobytes()
    ka, kb = TA.packed_set(ca), TA.packed_set(cb)
    for xa, xb in ((ka, sb), (sa, kb), (ka, kb)):
        pk = TA.run_dp_dev(codec, TA.to_device(xa), TA.to_device(xb), pt, wa, wb, LAY, SLOT, _dev(rot), _dev(trans), 0.6)
        assert pk[0].tobytes() == one[0].tobytes() and pk[1].tobytes() == one[1].tobytes()
    # aligned may be NULL
    assert TA.run_dp_dev(codec, da, db, pt, wa, wb, LAY, SLOT, _dev(rot), _dev(trans), 0.6, want_aligned=False)[0].tobytes() == one[0].tobytes()


def test_dp_with_masked_and_non_finite_rows(codec):
    ca, cb, rot, trans = _dp_chains(((65, 129), (64, 64), (63, 65)), 12)
    sa, sb = TA.padded_set(ca), TA.padded_set(cb)
    rng = np.random.default_rng(5)
    for s, rows in ((sa, (0, 7, 8, 40, 62)), (sb, (3, 30, 31, 64))):
        for e in range(3):
            for r, bad in zip(rows, (np.nan, np.inf, -np.inf, 3e19, None)):
                if bad is None:
                    s["mask"][e, r, SLOT] = 0
                else:
                    s["pos"][e, r, SLOT, rng.integers(0, 3)] = bad
    sa["pos"][0, 20, SLOT] = 3e19                                              # a site: finite, and |a - b|^2 is finite in float64
    pairs = np.asarray([(0, 0), (1, 1), (2, 2), (0, 2)], np.int32)
    r4, t4 = np.concatenate([rot, rot[:1]]), np.concatenate([trans, trans[:1]])
    for gap in (0.0, 0.6):
        got = _check_dp(codec, sa, sb, pairs, 65, 129, r4, t4, gap, f"poisoned, gap {gap}")
        assert (got[0][:, [0, 7, 8, 62]] == -1).all()
        assert not np.isin(got[0][:3], [3, 30, 31]).any()


def test_dp_at_the_largest_width(codec):
    ca, cb, rot, trans = _dp_chains(((TA.MAX_WIDTH, TA.MAX_WIDTH),), 13)
    cb[0][500:] = cb[0][499:-1].copy()                                         # an insertion in the middle: the path leaves the diagonal
    sa, sb = TA.padded_set(ca), TA.padded_set(cb)
    pairs = np.zeros((1, 2), np.int32)
    got = _check_dp(codec, sa, sb, pairs, TA.MAX_WIDTH, TA.MAX_WIDTH, rot, trans, 0.6, "1024 x 1024")
    assert got[1][0] > 900 and got[0][0, 100] == 100 and got[0][0, 900] == 901
    # above the largest width: refused, nothing written
    TA.run_dp_dev(codec, TA.to_device(sa), TA.to_device(sb), _dev(pairs), TA.MAX_WIDTH + 1, TA.MAX_WIDTH, LAY, SLOT, _dev(rot), _dev(trans), 0.6, expect=-1)


# ---- the full search -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def batch():
    ca, cb, pairs = TA.align_batch()
    sa, sb = TA.padded_set(ca), TA.padded_set(cb)
    ref, _ = TA.align_batch_reference()
    return dict(ca=ca, cb=cb, pairs=pairs, sa=sa, sb=sb, wa=sa["pos"].shape[1], wb=sb["pos"].shape[1], ref=ref)


@pytest.fixture(scope="module")
def batch_dev(codec, batch):
    b = batch
    da, db, pt = TA.to_device(b["sa"]), TA.to_device(b["sb"]), _dev(b["pairs"])
    return (da, db, pt), TA.run_dev(codec, da, db, pt, b["wa"], b["wb"], LAY, SLOT)


def _close(got, ref, what):
    solved = ref["aligned"] >= 3
    seen = {}
    for tm in ("tm", "tm_a", "tm_b"):
        g = dict(sites=got["aligned"], gdt_counts=np.zeros((len(solved), 5), np.int32), trans=got["trans"], rmsd=got["rmsd"], tm=got[tm], dev=got["dev"], rot=got["rot"])
        r = dict(sites=ref["aligned"], gdt_counts=g["gdt_counts"], trans=ref["trans"], rmsd=ref["rmsd"], tm=ref[tm], dev=ref["dev"], rot=ref["rot"])
        seen[tm] = SP.close(g, r, what, compare_rot=solved)
    print(what, seen["tm"], "tm_a", seen["tm_a"]["tm"], "tm_b", seen["tm_b"]["tm"])


def _exact(got, ref, what):
    for k in ("map", "aligned", "seed", "sites_a", "sites_b", "status"):
        bad = got[k] != ref[k]
        assert got[k].dtype == np.int32 and not bad.any(), (what, k, np.argwhere(bad)[:4], got[k][bad][:4], ref[k][bad][:4])


def test_seeded_batch_against_the_reference(codec, batch, batch_dev):
    b = batch
    (da, db, pt), got = batch_dev
    _exact(got, b["ref"], "padded")
    _close(got, b["ref"], "seeded batch")
    SP.proper(got["rot"], "seeded batch")
    assert (got["seed"] > 0).sum() >= 8 and (got["tm"][:10] > 0.3).all()
    # a chain without rows: the empty result
    e = 10
    assert got["rot"][e].tobytes() == np.eye(3, dtype=F).tobytes() and not got["trans"][e].any() and got["tm"][e] == 0 and got["aligned"][e] == 0
    assert (got["map"][e] == -1).all() and not got["dev"][e].view(np.uint32).any() and got["seed"][e] == 0
    # never below the gapless-only search, on the float32 values
    gapless = TA.run_dev(codec, da, db, pt, b["wa"], b["wb"], LAY, SLOT, fragments=False, dp_rounds=0)
    assert (got["tm"] >= gapless["tm"]).all() and (got["tm"][4:10] > gapless["tm"][4:10]).all()
    # determinism on bytes: the same call again, packed against padded, NULL outputs
    SP.same_bytes(TA.run_dev(codec, da, db, pt, b["wa"], b["wb"], LAY, SLOT), got, "second call")
    ka, kb = TA.to_device(TA.packed_set(b["ca"])), TA.to_device(TA.packed_set(b["cb"]))
    SP.same_bytes(TA.run_dev(codec, ka, kb, pt, b["wa"], b["wb"], LAY, SLOT), got, "packed")
    SP.same_bytes(TA.run_dev(codec, ka, db, pt, b["wa"], b["wb"], LAY, SLOT), got, "packed a, padded b")
    few = TA.run_dev(codec, da, db, pt, b["wa"], b["wb"], LAY, SLOT, want=("rot", "trans", "map"))
    SP.same_bytes(few, {k: got[k] for k in few}, "optional outputs")


def test_without_fragments_against_the_reference(codec, batch, batch_dev):
    b = batch
    (da, db, pt), _ = batch_dev
    got = TA.run_dev(codec, da, db, pt, b["wa"], b["wb"], LAY, SLOT, fragments=False, gaps=(1.0,), refine=1, dp_rounds=3, iterations=2, levels=2)
    ref = TA.align_sets(b["sa"], b["sb"], b["pairs"], b["wa"], b["wb"], SLOT, fragments=False, gaps=(1.0,), refine=1, dp_rounds=3, iterations=2, levels=2)
    _exact(got, ref, "no fragments")
    _close(got, ref, "no fragments")


def test_host_forms_give_the_same_bytes(codec, batch, batch_dev):
    b = batch
    got = batch_dev[1]
    sa, sb = b["sa"], b["sb"]
    h = codec.tm_align(sa["pos"], sa["mask"], sb["pos"], sb["mask"], b["pairs"], SLOT, length_a=sa["length"], length_b=sb["length"])
    SP.same_bytes({k: h[k] for k in TA.KEYS}, got, "fcz_tmalign")
    ka, kb = TA.packed_set(b["ca"]), TA.packed_set(b["cb"])
    h = codec.tm_align(ka["pos"], ka["mask"], kb["pos"], kb["mask"], b["pairs"], SLOT, row_off_a=ka["row_off"], row_off_b=kb["row_off"])
    SP.same_bytes({k: h[k] for k in TA.KEYS}, got, "fcz_tmalign, packed")
    d = codec.tm_align_dp(sa["pos"], sa["mask"], sb["pos"], sb["mask"], b["pairs"], got["rot"], got["trans"], 0.6, SLOT, length_a=sa["length"], length_b=sb["length"])
    ref = TA.dp_sets(sa, sb, b["pairs"], b["wa"], b["wb"], SLOT, got["rot"], got["trans"], 0.6)
    assert d["map"].tobytes() == ref[0].tobytes() and d["aligned"].tobytes() == ref[1].tobytes()
    for bad in (dict(gaps=()), dict(gaps=(17.0,)), dict(refine=65), dict(dp_rounds=True), dict(fragments=1), dict(iterations=65), dict(levels=0)):
        with pytest.raises(ValueError):
            codec.tm_align(sa["pos"], sa["mask"], sb["pos"], sb["mask"], b["pairs"], SLOT, **bad)


def test_status_hostile_row_off_and_pairs(codec, batch):
    b = batch
    ka = TA.packed_set(b["ca"])
    n, R = len(b["ca"]), ka["pos"].shape[0]
    hostile = ka["row_off"].copy()
    hostile[3], hostile[6] = 0xFFFFFFF0, 5                                       # chain 2 runs past the end, 3 backwards; 5 backwards, 6 from row 5
    ka_h = dict(ka, row_off=hostile)
    pairs = np.asarray([(2, 2), (3, 3), (5, 5), (6, 6), (-1, 0), (0, 10 ** 6), (n, 0), (9, 9), (-2 ** 31, 2 ** 31 - 1)], np.int32)
    sb = b["sb"]
    got = TA.run_dev(codec, TA.to_device(ka_h), TA.to_device(sb), _dev(pairs), 64, b["wb"], LAY, SLOT, fragments=False, dp_rounds=2)
    ref = TA.align_sets(ka_h, sb, pairs, 64, b["wb"], SLOT, fragments=False, dp_rounds=2)
    _exact(got, ref, "hostile")
    assert list(got["status"]) == [1, 0, 0, 1, 2, 2, 2, 1, 2] and got["sites_a"][1] == 0 and got["sites_a"][2] == 0
    for e in np.flatnonzero(got["status"]):
        assert got["rot"][e].tobytes() == np.eye(3, dtype=F).tobytes() and (got["map"][e] == -1).all() and got["aligned"][e] == 0 and got["tm"][e] == 0
    assert R > 64


def test_refusals_leave_the_outputs_untouched(codec, batch, batch_dev):
    b = batch
    (da, db, pt), _ = batch_dev
    ok = dict(wa=b["wa"], wb=b["wb"], layout=LAY, slot=SLOT)
    for change in (dict(wa=0), dict(wb=TA.MAX_WIDTH + 1), dict(layout=9), dict(slot=4), dict(slot=-1), dict(gaps=(-0.1,)), dict(gaps=(float("nan"),)),
                   dict(gaps=(16.5,)), dict(gaps=()), dict(gaps=(0.1,) * 5), dict(refine=65), dict(dp_rounds=65), dict(iterations=65)):
        a = dict(ok, **{k: v for k, v in change.items() if k in ok})
        p = {k: v for k, v in change.items() if k not in ok}
        TA.run_dev(codec, da, db, pt, a["wa"], a["wb"], a["layout"], a["slot"], expect=-1, **p)
    TA.run_dev(codec, da, db, None, b["wa"], b["wb"], LAY, SLOT, expect=-1, m=3)
    TA.run_dev(codec, da, db, pt, b["wa"], b["wb"], LAY, SLOT, want=("trans", "tm"), expect=-1)       # rot is required
    assert TA.run_dev(codec, da, db, pt[:0], b["wa"], b["wb"], LAY, SLOT, want=("rot", "trans"))["rot"].shape == (0, 3, 3)


def _refused(codec, bt, host, dp, **change):
    """one call of fcz_tmalign_dev / fcz_tmalign (host) / fcz_tmalign_dp_dev / fcz_tmalign_dp (dp) on the seeded batch with ONE argument
    changed: it must return FCZ_E_INVALID_ARG and leave every output byte, guards included, as it was. change: a / b = None or a dict
    of CChainSet fields to replace; pairs, params, out, rot, trans, map = None; wa, wb, layout, slot, gap; nulls = output names"""
    import ctypes
    import torch
    from foldcomp_amd.structure import CTmAlignOut, CTmAlignParams
    m, wa = len(bt["pairs"]), bt["wa"]
    put = (lambda x: np.ascontiguousarray(x)) if host else _dev
    addr = (lambda x: x.ctypes.data) if host else (lambda x: x.data_ptr())
    keep = []

    def cset(s, change):
        if change is None:
            return None
        arrays = {k: (None if s[k] is None else put(s[k])) for k in ("pos", "mask", "length")}
        keep.append(arrays)
        c = TA.c_set(dict({k: (None if v is None else (torch.from_numpy(v) if host else v)) for k, v in arrays.items()}, row_off=None))
        if host:
            c.pos, c.mask, c.length = (None if arrays[k] is None else arrays[k].ctypes.data for k in ("pos", "mask", "length"))
        for k, v in change.items():
            setattr(c, k, v)
        return c
    sa, sb = cset(bt["sa"], change.get("a", {})), cset(bt["sb"], change.get("b", {}))
    pairs = put(bt["pairs"])
    spec = TA.out_spec(m, wa, ("map", "aligned", "rot", "trans") if dp else TA.KEYS)
    g = HostGuarded(spec, guard=64) if host else DevGuarded(spec)
    ptr, untouched = g.ptr, g.untouched
    nulls = change.get("nulls", ())
    ref = lambda o: None if o is None else ctypes.byref(o)
    args = [codec.ctx, ref(sa), ref(sb), None if "pairs" in change else addr(pairs), m, change.get("wa", wa), change.get("wb", bt["wb"]),
            change.get("layout", LAY), change.get("slot", SLOT)]
    if dp:
        rot, trans = put(np.tile(np.eye(3, dtype=F), (m, 1, 1))), put(np.zeros((m, 3), F))
        args += [None if "rot" in change else addr(rot), None if "trans" in change else addr(trans), change.get("gap", 0.6),
                 None if "map" in change else ptr("map"), ptr("aligned")]
        fn = codec.lib.fcz_tmalign_dp if host else codec.lib.fcz_tmalign_dp_dev
    else:
        par = None if "params" in change else CTmAlignParams(1, 4, 20, 2, (ctypes.c_double * 4)(0.6, 0.0), 0, 20)
        out = None if "out" in change else CTmAlignOut(*(None if k in nulls else ptr(k) for k in TA.KEYS))
        args += [ref(par), ref(out)]
        fn = codec.lib.fcz_tmalign if host else codec.lib.fcz_tmalign_dev
    if not host:
        torch.cuda.synchronize()
    rc = fn(*args)
    codec.synchronize()
    assert rc == -1 and untouched(), (host, dp, change, rc)


SET_REFUSALS = (None, dict(pos=None), dict(mask=None), dict(rows=0), dict(rows=2 ** 31))   # (a padded set: row_off NULL)


@pytest.mark.parametrize("host", (False, True), ids=("device", "host"))
def test_every_refusal_of_the_four_entry_points(codec, batch, host):
    """what include/fcz_hip.h lists as FCZ_E_INVALID_ARG, one argument at a time, through the device and the host forms of the search and
    of the DP alone: nothing is launched, no byte of an output changes. (A NULL ctx is refused in tests/test_tmalign_cpu.py; a packed set
    is marked by its row_off, so "a packed set without row_off" is a padded set and no refusal.)"""
    b = batch
    common = [dict(a=c) for c in SET_REFUSALS] + [dict(b=c) for c in SET_REFUSALS]
    common += [dict(pairs=None), dict(wa=0), dict(wb=0), dict(wa=TA.MAX_WIDTH + 1), dict(wb=TA.MAX_WIDTH + 1), dict(layout=3), dict(layout=-1), dict(slot=4),
               dict(slot=-1)]
    for change in common + [dict(params=None), dict(out=None), dict(nulls=("rot",)), dict(nulls=("trans",))]:
        _refused(codec, b, host, False, **change)
    for change in common + [dict(rot=None), dict(trans=None), dict(map=None), dict(gap=-0.1), dict(gap=float("nan")), dict(gap=16.5), dict(gap=float("inf"))]:
        _refused(codec, b, host, True, **change)
    # the parameters of the search, through the host form too
    if host:
        sa, sb = b["sa"], b["sb"]
        for bad in (dict(gaps=(16.5,)), dict(refine=65), dict(dp_rounds=65), dict(iterations=65)):
            with pytest.raises(ValueError):
                codec.tm_align(sa["pos"], sa["mask"], sb["pos"], sb["mask"], b["pairs"], SLOT, **bad)


# ---- the Python surface, on the golden records ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def records(golden):
    z = golden[0]
    six = [(e, len(z[f"{n}/fasta"])) for n, e in zip(*golden_records_raw(golden)) if 40 <= len(z[f"{n}/fasta"]) <= 160][:6]
    assert len(six) == 6
    return [e for e, _ in six], min(m for _, m in six)


def test_foldcomp_tm_align_on_windows_of_the_golden_records(codec, records):
    import foldcomp
    import torch
    recs, shortest = records
    n, W = len(recs), shortest - 20
    out = {}
    for layout in ("atom37", "atom14"):
        full = foldcomp.decode_tensors(recs, layout=layout, codec=codec)
        win = foldcomp.decode_tensors(recs, layout=layout, codec=codec, max_len=W, crop=[10] * n)
        pairs = torch.arange(n, dtype=torch.int32, device="cuda:0").repeat_interleave(2).reshape(n, 2).contiguous()
        r = foldcomp.tm_align(full, win, pairs, codec=codec)
        out[layout] = {k: v.cpu().numpy() for k, v in r.items()}
        g = out[layout]
        sites_win = (win["mask"][:, :, 1] != 0).sum(dim=1).cpu().numpy()
        assert np.array_equal(g["aligned"], sites_win) and np.array_equal(g["sites_b"], sites_win) and not g["status"].any()
        on = win["mask"][:, :, 1].cpu().numpy() != 0
        want = np.full(g["map"].shape, -1, np.int32)
        want[:, 10:10 + W] = np.where(on, np.arange(W, dtype=np.int32), -1)
        assert np.array_equal(g["map"], want)
        assert np.abs(g["tm_b"] - 1.0).max() <= 4 * np.finfo(F).eps and (g["rmsd"] < 1e-4).all() and (g["tm_a"] < 1.0).all()
        SP.proper(g["rot"], layout)
    SP.same_bytes(out["atom37"], out["atom14"], "atom37 against atom14")
    # b=None: every i < j of a, in either form, and the DP alone from the transforms just found
    full = foldcomp.decode_tensors(recs, layout="backbone4", codec=codec)
    r = foldcomp.tm_align(full, codec=codec, fragments=False)
    assert r["pairs"].cpu().numpy().tolist() == [[i, j] for i in range(n) for j in range(i + 1, n)]
    assert (r["tm"] > 0).all() and (r["tm"] <= 1).all() and (r["aligned"] >= 3).all()
    p = foldcomp.tm_align(foldcomp.decode_tensors(recs, layout="backbone4", codec=codec, packed=True), codec=codec, fragments=False)
    for k in ("rot", "trans", "tm", "tm_a", "tm_b", "aligned", "seed", "rmsd"):
        assert p[k].cpu().numpy().tobytes() == r[k].cpu().numpy().tobytes(), k
    wa = p["map"].shape[1]
    assert np.array_equal(p["map"].cpu().numpy(), r["map"].cpu().numpy()[:, :wa]) and (r["map"].cpu().numpy()[:, wa:] == -1).all()
    d = foldcomp.tm_align(full, pairs=r["pairs"], transform=(r["rot"], r["trans"]), gaps=(0.6,), codec=codec)
    assert sorted(d) == ["aligned", "map", "pairs"] and (d["aligned"] >= 3).all()
    with pytest.raises(ValueError):
        foldcomp.tm_align(full, codec=codec, gaps=(99.0,))
