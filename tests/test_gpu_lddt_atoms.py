"""GPU: the all-atom lDDT with symmetric side-chain renaming (fcz_lddt_atoms_dev, its packed and host forms, Codec.lddt_atoms,
foldcomp.lddt_atoms) against the numpy restatement of the contract (tests/_lddt_atoms.py). Every output is compared exactly, integers
equal and floats on bits; the device calls write into arrays pre-filled with 0xA5 with guard bytes on both sides."""
import ctypes

import numpy as np
import pytest

import _analysis as AN
import _dense as DN
import _lddt_atoms as LA
from _analysis import NAN_BITS
from _cases import golden_records_raw
from _devpath import HostGuarded, host_ptr, to_dev
from foldcomp_amd import _lib

pytestmark = pytest.mark.gpu

L_GOLD = 256
F = np.float32
TABLE = {A: LA.default_table(A) for A in (37, 14, 4)}
TILE = {37: 20, 14: 18, 4: 64}                                               # rows per query tile of the score sweep (fcz_lddt_atoms.h)
DECIDE_TILE = 64                                                             # and of the decide sweep
BB37 = [0, 1, 2, 4]                                                          # N, CA, C, O in atom37


@pytest.fixture(scope="module")
def records(golden):
    return golden_records_raw(golden)[1]


def _capable(aatype, A):
    """rows whose type has a slot with another naming in the default table"""
    return (TABLE[A] != np.arange(A))[np.minimum(aatype, 20)].any(axis=-1)


def _every_second(flags):
    """bool array -> the same with every second set element cleared"""
    out = np.zeros(flags.shape, bool).ravel()
    out[np.flatnonzero(flags.ravel())[::2]] = True
    return out.reshape(flags.shape)


@pytest.fixture(scope="module")
def gold(codec, records):
    """The 56 golden records as atom37 / atom14 / backbone4 at L = 256 on the host, a prediction = the truth plus seeded Gaussian
    noise of 0.5 with the symmetric atoms of every second swap-capable row exchanged, drawn once in atom37 and carried to the other
    layouts atom by atom, and the restatement on atom37 and backbone4: computed once, never changed. The prediction's mask is the
    truth's without the chain's OXT (atom37 slot 36), which atom14 has no slot for, so that the layouts hold the same atoms."""
    host, _ = AN.decoded_layouts(codec, records, L_GOLD, ("pos", "mask", "aatype", "length"))
    a = host["atom37"]
    aa = a["aatype"]
    assert a["length"].max() >= L_GOLD and a["mask"][..., 36].sum() > 0
    inside = np.arange(L_GOLD)[None, :] < np.minimum(a["length"], L_GOLD)[:, None]
    exchanged = _every_second(_capable(aa, 37) & inside)
    noisy = (a["pos"] + np.random.default_rng(2024).standard_normal(a["pos"].shape) * 0.5).astype(F)
    p37 = LA.exchange(noisy, aa, exchanged, TABLE[37])
    m37 = a["mask"].copy()
    m37[..., 36] = 0
    pred = dict(atom37=(p37, m37), atom14=(LA.to14(p37, aa), LA.to14(m37, aa)), backbone4=(np.ascontiguousarray(p37[..., BB37, :]), np.ascontiguousarray(m37[..., BB37])))
    assert np.array_equal(LA.to14(a["pos"], aa) * host["atom14"]["mask"][..., None], host["atom14"]["pos"] * host["atom14"]["mask"][..., None])
    exp37 = LA.lddt_atoms(a["pos"], a["mask"], p37, m37, aa, a["length"], TABLE[37])
    b = host["backbone4"]
    exp4 = LA.lddt_atoms(b["pos"], b["mask"], *pred["backbone4"], b["aatype"], b["length"], TABLE[4])
    exp = dict(atom37=exp37, atom14=dict(exp37, atom_pairs=LA.to14(exp37["atom_pairs"], aa), atom_hits=LA.to14(exp37["atom_hits"], aa)), backbone4=exp4)
    # the renaming path is not vacuous: rows that are swapped and ambiguous rows that are not
    amb = _capable(aa, 37) & inside
    sw = exp37["swapped"] != 0
    print("golden: ambiguous rows", int(amb.sum()), "exchanged", int(exchanged.sum()), "swapped", int(sw.sum()), "pairs", int(exp37["pairs"].sum(dtype=np.int64)))
    assert sw.sum() >= 1 and (amb & ~sw).sum() >= 1 and not (sw & ~amb).any() and not exp4["swapped"].any()
    assert (sw & exchanged).sum() > (sw & ~exchanged).sum()                   # (noise of 0.5 seldom makes the other naming the better one)
    return dict(host=host, pred=pred, n=len(records), exp=exp)


def _dev_inputs(h, pred):
    return [to_dev(x) for x in (h["pos"], h["mask"], pred[0], pred[1], h["aatype"])]


def test_golden_padded(codec, gold):
    n = gold["n"]
    got = {}
    for lay in DN.LAYOUTS:
        h = gold["host"][lay]
        got[lay] = LA.run_dev(codec, *_dev_inputs(h, gold["pred"][lay]), to_dev(h["length"]), n, L_GOLD, DN.LAYOUTS[lay], False)
        LA.same(got[lay], gold["exp"][lay], lay)
    for k in LA.ROW_KEYS:                                                     # the same atoms, the same values
        assert np.array_equal(got["atom37"][k].view(np.uint8), got["atom14"][k].view(np.uint8)), k
    exp = gold["exp"]["atom37"]
    for e, m in enumerate(np.minimum(gold["host"]["atom37"]["length"], L_GOLD)):
        for k in LA.KEYS:
            assert not exp[k][e, m:].any(), (e, k)
    assert exp["pairs"].sum(dtype=np.int64) > 10 ** 6 and 0.5 < LA.chain_quotient(exp["pairs"], exp["hits"]) < 1


def test_golden_packed(codec, gold):
    lens = np.minimum(gold["host"]["atom37"]["length"].astype(np.int64), L_GOLD)
    row_off = AN.row_off_of(lens)
    R = int(row_off[-1])
    cat = lambda a: AN.pack1(a, lens)
    for lay in DN.LAYOUTS:
        h = gold["host"][lay]
        arrays = [to_dev(cat(x)) for x in (h["pos"], h["mask"], *gold["pred"][lay], h["aatype"])]
        got = LA.run_dev(codec, *arrays, to_dev(row_off), gold["n"], R, DN.LAYOUTS[lay], True)
        LA.same(got, {k: cat(v) for k, v in gold["exp"][lay].items()}, f"packed {lay}")


# ---- synthetic tensors ----------------------------------------------------------------------------------------------------------

TYPES = np.asarray([LA.PHE, 0, LA.ASP, 7, LA.TYR, LA.VAL, LA.GLU, 22, 255, 10, LA.PHE, LA.VAL, 14], np.uint8)   # swap-capable rows are guaranteed
DENSITY = {37: 0.21, 14: 0.56, 4: 1.0}                                       # about 7.8 atoms a row in atom37 and atom14


def _walk(rng, m, A):
    """m rows of A atoms scattered about a random walk: every row has atoms of other rows inside the cutoff"""
    ca = np.cumsum(rng.standard_normal((m, 3)) * 2.2, axis=0).astype(F)
    return (ca[:, None, :] + rng.standard_normal((m, A, 3)) * 2.0).astype(F)


def _synthetic(lens, A, seed, hostile=True):
    """chains [n, L, A, 3]: the truth a scattered walk, masks of the layout's density with the partnered slots of three rows in four
    set in both masks, the prediction the truth plus noise of 0.5 with the partnered slots of every second swap-capable row exchanged.
    With hostile, chains from 12 rows on get NaN, +inf, -inf and 3e19 coordinates under set masks in either tensor, one of them on a
    partnered slot (the row is then undecidable); NaN patterns under cleared masks of the truth and in every row behind the length."""
    rng = np.random.default_rng(seed)
    n, L = len(lens), max(max(lens), 1)
    pt, pp = np.zeros((n, L, A, 3), F), np.zeros((n, L, A, 3), F)
    mt, mp = (rng.random((n, L, A)) < DENSITY[A]).astype(np.uint8), (rng.random((n, L, A)) < min(1.0, DENSITY[A] * 4)).astype(np.uint8)
    aa = TYPES[(np.arange(n * L) * 5 % len(TYPES))].reshape(n, L).copy()
    partnered = (TABLE[A] != np.arange(A))[np.minimum(aa, 20)]
    keep = partnered & (rng.random((n, L)) < 0.75)[..., None]
    mt[keep] = 1
    mp[keep] = 1
    for e, m in enumerate(lens):
        pt[e, :m] = _walk(rng, m, A)
        pp[e, :m] = pt[e, :m] + (rng.standard_normal((m, A, 3)) * 0.5).astype(F)
        if hostile and m >= 12:
            r = rng.choice(m, size=6, replace=False)
            pt[e, r[0], 0, 0] = np.nan; pp[e, r[1], 1, 1] = np.inf; pt[e, r[2], A - 1, 2] = -np.inf
            pp[e, r[3], 2, 0] = 3e19; pt[e, r[4], 0, 1] = -3e19
            mt[e, r[:5]] = mp[e, r[:5]] = 1
            cap = np.flatnonzero(partnered[e, :m].any(axis=1))
            if len(cap):
                pp[e, cap[-1], np.flatnonzero(partnered[e, cap[-1]])[0], 1] = np.nan
        pt[e, m:] = np.nan
        pp[e, m:] = np.nan
    exchanged = _every_second(_capable(aa, A))
    pp = np.ascontiguousarray(LA.exchange(pp, aa, exchanged, TABLE[A]))
    pt.view(np.uint32)[mt == 0] = NAN_BITS
    return dict(pt=pt, mt=mt, pp=pp, mp=mp, aa=aa, lens=np.asarray(lens, np.uint32), L=L, n=n, A=A, layout=LA.LAYOUT[A])


def _run(codec, s, packed=False, bound="lens", **kw):
    """the device form on the synthetic set `s`; replacements of its arrays and run_dev's arguments as keywords"""
    arr = {k: kw.pop(k, s[k]) for k in ("pt", "mt", "pp", "mp", "aa")}
    if packed:
        arr = {k: None if v is None else AN.pack1(v, s["lens"]) for k, v in arr.items()}
        off = AN.row_off_of(s["lens"])
        return LA.run_dev(codec, *(None if arr[k] is None else to_dev(arr[k]) for k in ("pt", "mt", "pp", "mp", "aa")), to_dev(off), s["n"], int(off[-1]),
                          s["layout"], True, **kw)
    b = s["lens"] if isinstance(bound, str) else bound
    return LA.run_dev(codec, *(None if arr[k] is None else to_dev(arr[k]) for k in ("pt", "mt", "pp", "mp", "aa")), None if b is None else to_dev(b), s["n"], s["L"],
                      s["layout"], False, **kw)


def _restate(s, bound="lens", table="default", **kw):
    arr = {k: kw.pop(k, s[k]) for k in ("pt", "mt", "pp", "mp", "aa")}
    return LA.lddt_atoms(arr["pt"], arr["mt"], arr["pp"], arr["mp"], arr["aa"], s["lens"] if isinstance(bound, str) else bound,
                         TABLE[s["A"]] if isinstance(table, str) else table, **kw)


@pytest.fixture(scope="module", params=[37, 14, 4])
def synthetic(request):
    """chains of 0, 1, 2 rows, of one row fewer and one row more than a tile of the score sweep and of the decide sweep, and a chain
    whose anchors -- and so its atoms -- exceed one candidate pass by a little, so that both sweeps take a second pass"""
    A = request.param
    Q = _lib.load().fcz_lddt_atoms_pass()
    T = TILE[A]
    lens = sorted({0, 1, 2, T - 1, T + 1, DECIDE_TILE - 1, DECIDE_TILE + 1}) + [Q // 3]   # (the last: long enough at four anchors a row)
    s = _synthetic(lens, A, 100 + A)
    e = len(lens) - 1
    with np.errstate(invalid="ignore"):
        pres = (s["mt"][e] != 0) & (s["mp"][e] != 0) & np.isfinite(s["pt"][e]).all(axis=-1) & np.isfinite(s["pp"][e]).all(axis=-1)
    is_anchor = pres & (TABLE[A][np.minimum(s["aa"][e], 20)] == np.arange(A))
    big = int(np.searchsorted(np.cumsum(is_anchor.sum(axis=1)), Q, side="right")) + 2   # the first length with more than Q anchors, and a row
    assert big <= lens[-1]
    s["lens"][e] = big                                                        # the long chain is cut there
    s["pt"][e, big:] = np.nan
    s["pp"][e, big:] = np.nan
    n_anchor, pres = int(is_anchor[:big].sum()), pres[:big]
    s["exp"] = _restate(s)
    s["big"] = (e, big, n_anchor, int(pres.sum()), Q)
    return s


def test_synthetic_padded_and_packed(codec, synthetic):
    s = synthetic
    e, big, n_anchor, n_atom, Q = s["big"]
    print("A", s["A"], "lens", s["lens"].tolist(), "anchors / atoms of the long chain", n_anchor, n_atom, "pass", Q)
    assert Q < n_anchor < Q + 3 * s["A"] and n_anchor <= n_atom < 2 * Q, s["big"]   # two passes in either sweep
    exp = s["exp"]
    if s["A"] != 4:
        sw = exp["swapped"] != 0
        amb = _capable(s["aa"], s["A"]) & (np.arange(s["L"])[None, :] < s["lens"][:, None])
        assert sw.sum() > 20 and (amb & ~sw).sum() > 20 and sw[e].sum() > 5
    assert exp["pairs"].sum() > 10000
    got = _run(codec, s)
    LA.same(got, exp, "padded")
    LA.same(_run(codec, s), got, "again")                                     # two calls give the same bytes
    gp = _run(codec, s, packed=True, guard=8)
    LA.same(gp, {k: AN.pack1(v, s["lens"]) for k, v in exp.items()}, "packed")    # padded and packed give the same values
    # the optional outputs NULL: the others are what they were, the two arrays untouched
    LA.same(_run(codec, s, per_atom=False), exp, "per_atom NULL", LA.ROW_KEYS)
    LA.same(_run(codec, s, packed=True, per_atom=False), gp, "packed, per_atom NULL", LA.ROW_KEYS)
    # the host-pointer forms against the device forms
    h = codec.lddt_atoms(s["pt"], s["mt"], s["pp"], s["mp"], s["aa"], length=s["lens"], per_atom=True)
    LA.same(h, got, "fcz_lddt_atoms")
    off = AN.row_off_of(s["lens"])
    h = codec.lddt_atoms(*(AN.pack1(s[k], s["lens"]) for k in ("pt", "mt", "pp", "mp", "aa")), row_off=off)
    LA.same(h, gp, "fcz_lddt_atoms_packed", LA.ROW_KEYS)
    assert "atom_pairs" not in h and h["swapped"].dtype == np.bool_


def test_masks_types_tables_and_thresholds(codec, synthetic):
    s = synthetic
    A = s["A"]
    # mask_pred NULL: every slot of the prediction present (its NaN and 3e19 coordinates are then read)
    LA.same(_run(codec, s, mp=None), _restate(s, mp=None), "mask_pred NULL")
    # aatype NULL: nothing is renamed, whatever the table
    none = _restate(s, aa=None)
    assert not none["swapped"].any()
    LA.same(_run(codec, s, aa=None), none, "aatype NULL")
    LA.same(_run(codec, s, aa=None, packed=True), {k: AN.pack1(v, s["lens"]) for k, v in none.items()}, "aatype NULL, packed")
    if A != 4:
        assert (none["hits"] < s["exp"]["hits"]).sum() > 10                   # the exchanged rings are punished without the renaming
        # a custom table: VAL CG1 / CG2 beside ASP; the other types have no partner any more
        custom = LA.table_of(A, {LA.VAL: [("CG1", "CG2")], LA.ASP: [("OD1", "OD2")]})
        pt, mt, mp = s["pt"].copy(), s["mt"].copy(), s["mp"].copy()
        val = (custom != np.arange(A))[np.minimum(s["aa"], 20)] & (s["aa"] == LA.VAL)[..., None]
        mt[val] = mp[val] = 1                                                 # every VAL has its two CG, the truth half an Angstrom from the prediction
        pt[val] = s["pp"][val] + (np.random.default_rng(5).standard_normal((int(val.sum()), 3)) * 0.5).astype(F)
        pp = np.ascontiguousarray(LA.exchange(s["pp"], s["aa"], _every_second(s["aa"] == LA.VAL), custom))
        exp = _restate(s, pt=pt, pp=pp, mt=mt, mp=mp, table=custom)
        assert (exp["swapped"] != 0)[s["aa"] == LA.VAL].sum() > 5 and not (exp["swapped"] != 0)[s["aa"] == LA.PHE].any()
        LA.same(_run(codec, s, pt=pt, pp=pp, mt=mt, mp=mp, table=custom), exp, "custom table")
    # masks off: no atom, every output 0
    zero = np.zeros_like(s["mt"])
    off = _run(codec, s, mt=zero)
    assert not any(off[k].any() for k in LA.KEYS)
    LA.same(_run(codec, s, mp=zero), off, "mask_pred off")
    # another cutoff and other thresholds (one of them never reached, one always)
    kw = dict(cutoff=7.5, thresholds=(0.25, 0.0, 3.0, np.inf))
    exp = _restate(s, **kw)
    assert 0 < exp["pairs"].sum() < s["exp"]["pairs"].sum()
    LA.same(_run(codec, s, **kw), exp, "cutoff 7.5")


def test_length_null_and_clamped(codec):
    L = 70
    s = _synthetic([L] * 3, 14, 23, hostile=False)                            # finite rows behind every length below
    whole = _restate(s, bound=None)
    LA.same(_run(codec, s, bound=None), whole, "NULL")
    LA.same(_run(codec, s, bound=np.asarray([L + 1, 65535, 0xFFFFFFFF], np.uint32)), whole, "length > L")
    lens = np.asarray([40, 70, 7], np.uint32)
    exp = _restate(s, bound=lens)
    assert exp["pairs"][0, :40].sum() < whole["pairs"][0, :40].sum() and not exp["pairs"][0, 40:].any() and not exp["atom_pairs"][2, 7:].any()
    LA.same(_run(codec, s, bound=lens), exp, "length < L")


def test_hostile_row_off(codec):
    R = 300
    s = _synthetic([R], 37, 24)
    arrays = [s[k][0] for k in ("pt", "mt", "pp", "mp", "aa")]
    dev = [to_dev(a) for a in arrays]
    # chain 0 runs backwards (empty), rows 0 .. 29 are left uncovered, chain 4 runs past R (clamped to the rows that exist)
    row_off = np.asarray([200, 30, 90, 180, 181, 950], np.uint32)
    exp = LA.lddt_atoms(*arrays, row_off, TABLE[37], packed=True)
    assert exp["pairs"][180] == 0 and exp["pairs"][181:].sum() > 1000 and (exp["swapped"] != 0).sum() > 5
    got = LA.run_dev(codec, *dev, to_dev(row_off), 5, R, 0, True, guard=8)
    LA.same(got, exp, "hostile row_off")
    assert not any(got[k][:30].any() for k in LA.KEYS)
    # no chain at all: every row is uncovered
    none = LA.run_dev(codec, *dev, to_dev(row_off), 0, R, 0, True)
    assert not any(none[k].any() for k in LA.KEYS)

    def host_form(n, rows):
        """fcz_lddt_atoms_packed on the host arrays, its outputs between guard bytes"""
        from foldcomp_amd.structure import CLddtAtomsOut
        h = HostGuarded(LA.out_spec((rows,), 37))
        out = CLddtAtomsOut(*h.ptrs())
        assert codec.lib.fcz_lddt_atoms_packed(codec.ctx, *(host_ptr(a[:max(rows, 1)]) for a in arrays), host_ptr(row_off), n, rows, 0, 15.0, None, None,
                                               ctypes.byref(out)) == 0
        return {k: h.fetch(k) for k in LA.KEYS}

    LA.same(host_form(5, R), got, "fcz_lddt_atoms_packed n=5")
    LA.same(host_form(0, R), none, "fcz_lddt_atoms_packed n=0")
    assert all(v.size == 0 for v in host_form(3, 0).values())                 # chains without a row: nothing to write


def test_refusals_leave_the_outputs_untouched(codec):
    import torch
    n, L, A = 2, 8, 37
    pos, mask, aa, off = AN.refusal_inputs(n, L, A)
    o = LA.Outputs((n * L,), A)
    chain, outside, nan_th = TABLE[37].copy(), TABLE[37].copy(), np.asarray([0.5, np.nan, 2, 4], F)
    chain[5, 1], chain[5, 2], chain[5, 3] = 2, 3, 1
    outside[20, 0] = 37
    lib, ctx = codec.lib, codec.ctx

    def call(fn, **kw):
        a = dict(ctx=ctx, pt=pos.data_ptr(), mt=mask.data_ptr(), pp=pos.data_ptr(), mp=mask.data_ptr(), aa=aa.data_ptr(), bound=None, n=n, rows=L, layout=0,
                 cutoff=15.0, th=None, table=None, out={})
        a.update(kw)
        out = None if a["out"] is None else ctypes.byref(o.struct(**a["out"]))
        return fn(a["ctx"], a["pt"], a["mt"], a["pp"], a["mp"], a["aa"], a["bound"], a["n"], a["rows"], a["layout"], a["cutoff"], a["th"], a["table"], out)

    bad = [dict(ctx=None), dict(pt=None), dict(mt=None), dict(pp=None), dict(out=None), dict(layout=3), dict(layout=-1), dict(cutoff=0.0),
           dict(cutoff=float("nan")), dict(cutoff=float("inf")), dict(th=nan_th.ctypes.data), dict(table=chain.ctypes.data), dict(table=outside.ctypes.data),
           dict(rows=LA.max_rows(37) + 1)] + [dict(out={k: None}) for k in LA.ROW_KEYS]
    torch.cuda.synchronize()
    for b in bad:
        assert call(lib.fcz_lddt_atoms_dev, **b) == -1, b
        assert call(lib.fcz_lddt_atoms_packed_dev, **dict(dict(bound=off.data_ptr(), rows=n * L), **b)) == -1, b
    assert call(lib.fcz_lddt_atoms_dev, layout=1, rows=LA.max_rows(14) + 1) == -1   # every layout has a bound of its own
    assert call(lib.fcz_lddt_atoms_dev, rows=0) == -1                         # L == 0
    assert call(lib.fcz_lddt_atoms_packed_dev, rows=n * L) == -1              # chains without a row_off
    assert call(lib.fcz_lddt_atoms_dev, n=0) == 0 and call(lib.fcz_lddt_atoms_packed_dev, bound=off.data_ptr(), n=0, rows=0) == 0
    codec.synchronize()
    assert o.untouched()


# ---- Python surface -------------------------------------------------------------------------------------------------------------

def _np(d, keys):
    names = dict(score="lddt", pairs="lddt_pairs", hits="lddt_hits")
    return {k: d[names.get(k, k)].cpu().numpy() for k in keys}


def test_foldcomp_lddt_atoms(codec, records):
    import torch
    import foldcomp_amd as foldcomp
    sub = records[:12]
    t = foldcomp.decode_tensors(sub, codec=codec, max_len=200)
    n = len(sub)
    pos, mask, aa, length = (t[k].cpu().numpy() for k in ("pos", "mask", "aatype", "length"))
    mask = mask.view(np.uint8)
    inside = np.arange(200)[None, :] < np.minimum(length, 200)[:, None]
    amb_slots = (TABLE[37] != np.arange(37))[np.minimum(aa, 20)]
    capable = amb_slots.any(axis=-1) & inside
    complete = capable & (~amb_slots | (mask != 0)).all(axis=-1)              # every atom with another naming is there
    print("swap-capable rows", int(capable.sum()), "of them complete", int(complete.sum()))
    flipped = np.ascontiguousarray(LA.exchange(pos, aa, complete, TABLE[37]))  # the truth itself, every such side chain exchanged
    pred = dict(pos=torch.from_numpy(flipped).to(t["pos"].device))
    out = foldcomp.lddt_atoms(pred, t, per_atom=True, codec=codec)
    assert out["lddt"].shape == (n, 200) and out["lddt"].dtype == torch.float32 and out["lddt_pairs"].dtype == out["lddt_hits"].dtype == torch.int32
    assert out["swapped"].dtype == torch.bool and out["lddt_chain"].shape == (n,) and out["lddt_chain"].dtype == torch.float64
    assert out["atom_pairs"].shape == (n, 200, 37) and out["atom_hits"].dtype == torch.int32 and out["lddt"].device.type == "cuda"
    exp = LA.lddt_atoms(pos, mask, flipped, None, aa, length, TABLE[37])
    got = _np(out, LA.KEYS)
    LA.same(got, exp, "lddt_atoms")
    # On the REAL chains (the first five records: test.pdb, test_af.pdb and the three pieces of multichain.pdb) the exchanged side
    # chains are found on exactly the decidable rows and the score is 1. The synthetic records behind them are left out of these
    # two claims, not of the comparison above: their generator puts the two symmetric atoms of a side chain 0.3 A apart, so for some
    # of their rows both namings lie under every threshold and score the same, and a tie is no swap (include/fcz_hip.h).
    real = slice(0, 5)
    assert (length[real] > 1).all() and complete[real].sum() > 100
    assert np.array_equal(got["swapped"][real], complete[real]) and not (got["swapped"] & ~complete).any()
    assert (got["score"][real][got["pairs"][real] > 0] == 1).all() and (got["pairs"][real] > 0).sum() > 600
    chain = np.asarray([LA.chain_quotient(exp["pairs"][e], exp["hits"][e]) for e in range(n)], np.float64)
    assert np.array_equal(out["lddt_chain"].cpu().numpy(), chain) and (chain[real] == 1).all()
    assert "atom_pairs" not in foldcomp.lddt_atoms(pred, t, codec=codec)
    # no renaming: the exchanged side chains are punished
    plain = foldcomp.lddt_atoms(pred, t, swaps=None, codec=codec)
    LA.same(_np(plain, LA.ROW_KEYS), LA.lddt_atoms(pos, mask, flipped, None, None, length, None), "swaps=None", LA.ROW_KEYS)
    assert not plain["swapped"].any() and (plain["lddt"].cpu().numpy()[real][complete[real]] < 1).sum() > 100
    assert (plain["lddt_chain"][real] < out["lddt_chain"][real]).all()
    noaa = {k: v for k, v in t.items() if k != "aatype"}
    LA.same(_np(foldcomp.lddt_atoms(pred["pos"], noaa, swaps=None, codec=codec), LA.ROW_KEYS), _np(plain, LA.ROW_KEYS), "no aatype", LA.ROW_KEYS)
    with pytest.raises(ValueError):
        foldcomp.lddt_atoms(pred, noaa, codec=codec)
    # an array as the table, and the numpy form
    table = foldcomp.lddt_swaps("atom37")
    LA.same(_np(foldcomp.lddt_atoms(pred, t, swaps=table.astype(np.int64), per_atom=True, codec=codec), LA.KEYS), got, "swaps as an array")
    h = codec.lddt_atoms(pos, mask, flipped, None, aa, length=length, per_atom=True)
    LA.same(h, got, "Codec.lddt_atoms")
    # packed
    p = foldcomp.decode_tensors(sub, codec=codec, packed=True)
    lens = np.diff(p["cu_seqlens"].cpu().numpy())
    full = foldcomp.decode_tensors(sub, codec=codec)
    fl = np.ascontiguousarray(LA.exchange(full["pos"].cpu().numpy(), full["aatype"].cpu().numpy(), _capable(full["aatype"].cpu().numpy(), 37), TABLE[37]))
    fo = foldcomp.lddt_atoms(torch.from_numpy(fl).to(full["pos"].device), full, per_atom=True, codec=codec)
    po = foldcomp.lddt_atoms(torch.from_numpy(AN.pack1(fl, lens)).to(p["pos"].device), p, per_atom=True, codec=codec)
    LA.same(_np(po, LA.KEYS), {k: AN.pack1(v, lens) for k, v in _np(fo, LA.KEYS).items()}, "packed against padded")
    assert np.array_equal(po["lddt_chain"].cpu().numpy(), fo["lddt_chain"].cpu().numpy()) and po["swapped"].sum() > 100
    # nothing to compute, and what is refused
    e = foldcomp.decode_tensors([], codec=codec, max_len=8)
    z = foldcomp.lddt_atoms(e["pos"], e, per_atom=True, codec=codec)
    assert z["lddt"].shape == (0, 8) and z["atom_hits"].shape == (0, 8, 37) and z["lddt_chain"].shape == (0,)
    with pytest.raises(ValueError):
        foldcomp.lddt_atoms(dict(pos=pred["pos"].transpose(0, 1).contiguous().transpose(0, 1)), t, codec=codec)   # not contiguous
    with pytest.raises(foldcomp.error):
        foldcomp.lddt_atoms(pred["pos"].cpu(), {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in t.items()}, codec=codec)
