"""GPU: steric clashes and peptide-link violations of dense tensors (fcz_violations_dev, its packed and host forms, Codec.violations,
foldcomp.violations, decode_tensors(violations=True), tensor_batches(violations=True)) against the numpy restatement of the contract
(tests/_violations.py). Every output is compared exactly, integers equal and floats on bits; the device calls write into arrays
pre-filled with 0xA5 with guard bytes on both sides."""
import ctypes

import numpy as np
import pytest

import _analysis as AN
import _dense as DN
import _violations as V
from _analysis import NAN_BITS
from _cases import golden_records_raw
from _devpath import HostGuarded, host_ptr, to_dev
from foldcomp_amd import _lib, api

pytestmark = pytest.mark.gpu

L_GOLD = 256
F = np.float32
TABLE = {A: V.default_table(A) for A in (37, 14, 4)}
TILE = {37: 20, 14: 18, 4: 64}                                               # rows per query tile (fcz_violations.h, viol_tile_rows)
ROW_KEYS = V.KEYS[1:-1]


@pytest.fixture(scope="module")
def records(golden):
    return golden_records_raw(golden)[1]


@pytest.fixture(scope="module")
def gold(codec, records):
    """the 56 golden records as atom37 / atom14 / backbone4 at L = 256 on the host and the device, and the restatement on atom37 and
    on backbone4: computed once, never changed"""
    host, dev = AN.decoded_layouts(codec, records, L_GOLD, ("pos", "mask", "aatype", "length"))
    a, b = host["atom37"], host["backbone4"]
    assert a["length"].max() >= L_GOLD
    exp37 = V.violations(a["pos"], a["mask"], a["aatype"], a["length"], TABLE[37])
    exp4 = V.violations(b["pos"], b["mask"], b["aatype"], b["length"], TABLE[4])
    exp = dict(atom37=exp37, atom14=dict(exp37, clash_atom=AN.to14(exp37["clash_atom"], a["aatype"])), backbone4=exp4)
    return dict(host=host, dev=dev, n=len(records), exp=exp)


def test_golden_padded(codec, gold):
    n = gold["n"]
    got = {}
    for lay in DN.LAYOUTS:
        d = gold["dev"][lay]
        got[lay] = V.run_violations(codec, d["pos"], d["mask"], d["aatype"], d["length"], n, L_GOLD, DN.LAYOUTS[lay], False)
        V.same_violations(got[lay], gold["exp"][lay], lay)
        V.consistent(got[lay], gold["host"][lay]["length"])
    for k in ROW_KEYS + ("chain_counts",):                                    # the same atoms, the same values
        assert np.array_equal(got["atom37"][k].view(np.uint8), got["atom14"][k].view(np.uint8)), k
    a, exp = gold["host"]["atom37"], gold["exp"]["atom37"]
    assert not got["atom37"]["clash_atom"][..., 36].any() and a["mask"][..., 36].sum() > 0   # OXT is there and is left out
    assert exp["viol_mask"][:5].sum() == np.minimum(a["length"][:5], L_GOLD).sum() > 700      # the real chains: every row has atoms
    assert exp["link_mask"].sum() > 800 and exp["chain_counts"][:, 0].sum() > 6000
    for e, m in enumerate(np.minimum(a["length"], L_GOLD)):
        for k in ROW_KEYS:
            assert (exp[k][e, m:] == (-1 if k == "clash_partner" else 0)).all(), (e, k)
    print("golden atom37 chain_counts of the real chains:", exp["chain_counts"][:5].tolist(), "all chains:", exp["chain_counts"].sum(axis=0).tolist())
    # aatype NULL in atom37 (no proline link, no disulfide exclusion) on the first eight records; outputs that are not 16-byte aligned
    d = gold["dev"]["atom37"]
    null = V.violations(a["pos"][:8], a["mask"][:8], None, a["length"][:8], TABLE[37])
    V.same_violations(V.run_violations(codec, d["pos"], d["mask"], None, d["length"], 8, L_GOLD, 0, False, guard=8), null, "aatype NULL")


def test_golden_packed(codec, gold):
    lens = np.minimum(gold["host"]["atom37"]["length"].astype(np.int64), L_GOLD)
    row_off = AN.row_off_of(lens)
    R = int(row_off[-1])
    cat = lambda a: AN.pack1(a, lens)
    for lay in DN.LAYOUTS:
        hh = gold["host"][lay]
        got = V.run_violations(codec, to_dev(cat(hh["pos"])), to_dev(cat(hh["mask"])), to_dev(cat(hh["aatype"])), to_dev(row_off), gold["n"], R, DN.LAYOUTS[lay], True)
        V.same_violations(got, {k: (v if k == "chain_counts" else cat(v)) for k, v in gold["exp"][lay].items()}, f"packed {lay}")
        V.consistent(got, row_off, packed=True)


# ---- synthetic tensors ----------------------------------------------------------------------------------------------------------

def _synthetic(lens, A, seed, full=(), hostile=True):
    """chains [n, L, A, 3] of jittered helices; the chains in `full` keep every mask set, the others lose ~1 % of their masks (NaN
    patterns under the cleared masks) and, from 12 rows on and with hostile, get a NaN, +inf, -inf and two 3e19 coordinates under
    set masks; NaN patterns in every row behind the length. aatype random 0 .. 24 and 255"""
    rng = np.random.default_rng(seed)
    n, L = len(lens), max(max(lens), 1)
    pos, mask = np.zeros((n, L, A, 3), F), np.ones((n, L, A), np.uint8)
    for e, m in enumerate(lens):
        pos[e, :m] = AN.helix(rng, m, A)
        if e not in full:
            mask[e, :m][rng.random((m, A)) < 0.01] = 0
            if hostile and m >= 12:
                r = rng.choice(m, size=5, replace=False)
                pos[e, r[0], 0, 0] = np.nan; pos[e, r[1], 1, 1] = np.inf; pos[e, r[2], 3, 2] = -np.inf
                pos[e, r[3], 2, 0] = 3e19; pos[e, r[4], 0, 1] = -3e19
                mask[e, r, :4] = 1
        pos[e, m:] = np.nan
    pos.view(np.uint32)[mask == 0] = NAN_BITS
    aatype = rng.integers(0, 25, size=(n, L)).astype(np.uint8)
    aatype[rng.random((n, L)) < 0.05] = 255
    return pos, mask, aatype


def _pack_dict(exp, lens):
    return {k: (v if k == "chain_counts" else AN.pack1(v, lens)) for k, v in exp.items()}


@pytest.fixture(scope="module", params=[37, 14, 4])
def synthetic(request):
    """chains of 0, 1, 2, 3 rows, of one query tile and one row less and more, a chain with every mask set whose atoms exceed the
    pass by one row (atom37: 36 atoms a row, the OXT has no radius; atom14: the atoms the types own), and two hostile chains. In the
    long chain an atom of the last row is moved onto one of the first (a pair across two passes and two tiles), in the first hostile
    chain two atoms are put at exactly 1 from a third, on either side (a tie on depth), and a link is stretched and one bent."""
    A = request.param
    Q = _lib.load().fcz_violations_pass()
    T = TILE[A]
    per_row = {37: 36, 14: 14, 4: 4}[A]                                      # (atom37: the OXT has no radius; atom14: TRP below)
    big = Q // per_row + 1
    lens = [0, 1, 2, 3, T - 1, T, T + 1, big, 45, 130 if A != 37 else 50]
    pos, mask, aa = _synthetic(lens, A, 31 + A, full=(7,))
    if A == 14:
        aa[7, :big] = 17                                                      # TRP owns all 14 slots
    pos[7, big - 1, 1] = pos[7, 0, 1] + np.asarray([0.25, 0, 0], F)
    e = 8
    pos[e, 7, 1], pos[e, 5, 1], pos[e, 9, 1] = [200, 200, 200], [201, 200, 200], [199, 200, 200]
    mask[e, [5, 7, 9]] = 0                                                    # (the three rows keep their CA only)
    mask[e, [5, 7, 9], 1] = 1
    pos[e, 20:lens[e]] += np.asarray([0.9, 0.3, -0.2], F)                     # link 19 stretched
    pos[e, 30, 1] = pos[e, 30, 0] + (pos[e, 29, 2] - pos[e, 30, 0]) * F(0.9) + F(0.3)   # link 29 bent at N'
    mask[e, 19:21, :3] = mask[e, 29:31, :3] = 1
    aa[e, 12] = aa[e, 13] = V.PRO
    atoms = [int(V.atoms_of(pos[c, :m], mask[c, :m], aa[c, :m], TABLE[A])[0].sum()) for c, m in enumerate(lens)]
    assert Q < atoms[7] <= Q + per_row, (atoms, Q)
    ln = np.asarray(lens, np.uint32)
    exp = V.violations(pos, mask, aa, ln, TABLE[A])
    # the planted cases are what they were planted to be
    assert exp["clash_atom"][7, 0, 1] == 1 and exp["clash_atom"][7, big - 1, 1] == 1 and exp["clash_count"][7, 0] >= 1
    assert exp["clash_partner"][e, 7] == 5 and exp["clash_partner"][e, 5] == 7 and exp["clash_partner"][e, 9] == 7 and exp["clash_count"][e, 7] >= 2
    assert exp["clash_depth"][e, 5].view(np.uint32) == exp["clash_depth"][e, 7].view(np.uint32) == exp["clash_depth"][e, 9].view(np.uint32)
    assert exp["link_violation"][e, 19] & 1 and exp["link_violation"][e, 29] & 4 and exp["chain_counts"][e, 2] >= 1 and exp["chain_counts"][e, 3] >= 1
    return dict(A=A, layout={37: 0, 14: 1, 4: 2}[A], lens=ln, L=max(lens), arrays=(pos, mask, aa),
                row_off=AN.row_off_of(lens), exp=exp)


def test_synthetic_padded_and_packed(codec, synthetic):
    s = synthetic
    n = len(s["lens"])
    pos, mask, aa = (to_dev(a) for a in s["arrays"])
    got = V.run_violations(codec, pos, mask, aa, to_dev(s["lens"]), n, s["L"], s["layout"], False)
    V.same_violations(got, s["exp"], "padded")
    V.consistent(got, s["lens"])
    assert got["clash_count"].sum() > 0 and got["link_violation"].any() and got["viol_mask"].sum() > 200
    V.same_violations(V.run_violations(codec, pos, mask, aa, to_dev(s["lens"]), n, s["L"], s["layout"], False), got, "again")   # two calls give the same bytes
    packed = AN.pack(s["arrays"], s["lens"])
    R = int(s["row_off"][-1])
    gp = V.run_violations(codec, *(to_dev(a) for a in packed), to_dev(s["row_off"]), n, R, s["layout"], True, guard=8)
    V.same_violations(gp, _pack_dict(s["exp"], s["lens"]), "packed")           # padded and packed give the same values
    # the host-pointer forms against the device forms
    h = codec.violations(*s["arrays"], length=s["lens"])
    V.same_violations(h, got, "fcz_violations")
    h = codec.violations(*packed, row_off=s["row_off"])
    V.same_violations(h, gp, "fcz_violations_packed")


def test_tolerance_factor_and_custom_radii(codec):
    """a custom table, tolerance 0 (everything within the sum of the radii clashes), a small link factor (most links of a jittered helix
    are outside one sigma) and a large tolerance (T <= 0: nothing clashes); atom14 rows with every mask set, types above 20 use row 20"""
    lens = [1, 17, 18, 19, 60]
    pos, mask, aa = _synthetic(lens, 14, 52, full=range(5))
    ln = np.asarray(lens, np.uint32)
    n, L = len(lens), max(lens)
    dev = [to_dev(a) for a in (pos, mask, aa)]
    rng = np.random.default_rng(3)
    table = (rng.integers(4, 12, size=(21, 14)) * 0.25).astype(F)              # 1.0 .. 2.75
    table[rng.random((21, 14)) < 0.2] = 0
    for tol, factor in ((0.0, 1.0), (0.75, 0.0), (6.0, 12.0)):
        exp = V.violations(pos, mask, aa, ln, table, F(tol), F(factor))
        got = V.run_violations(codec, *dev, to_dev(ln), n, L, 1, False, table=table, tol=tol, factor=factor)
        V.same_violations(got, exp, f"tolerance {tol}, factor {factor}")
        assert (got["clash_count"].sum() > 1000) == (tol < 6) and (got["link_violation"].sum() > 50) == (factor < 12)
    assert not got["clash_atom"][np.broadcast_to(table[np.minimum(aa, 20)] == 0, got["clash_atom"].shape)].any()


def test_length_null_and_clamped(codec):
    lens = [40, 100, 77]
    L = 100
    pos, mask, aa = _synthetic([L] * 3, 4, 23)                                # finite rows behind every length below
    dev = [to_dev(a) for a in (pos, mask, aa)]
    whole = V.violations(pos, mask, aa, None, TABLE[4])
    V.same_violations(V.run_violations(codec, *dev, None, 3, L, 2, False), whole, "NULL")
    V.same_violations(V.run_violations(codec, *dev, to_dev(np.asarray([L + 1, 65535, 0xFFFFFFFF], np.uint32)), 3, L, 2, False), whole, "length > L")
    exp = V.violations(pos, mask, aa, lens, TABLE[4])
    assert whole["link_mask"][0, 39] and not exp["link_mask"][0, 39] and exp["chain_counts"][0, 0] < whole["chain_counts"][0, 0]   # the chain's new end has no link
    V.same_violations(V.run_violations(codec, *dev, to_dev(np.asarray(lens, np.uint32)), 3, L, 2, False), exp, "length < L")


def test_hostile_row_off(codec):
    R = 700
    pos, mask, aa = (a[0] for a in _synthetic([R], 4, 24))
    pos[350, 1] = pos[130, 1]                                                 # a clash inside chain 2 ...
    pos[20, 1], pos[60, 1] = pos[500, 1], pos[600, 1]                         # ... and none with an uncovered row or across chains
    mask[[350, 130, 20, 60, 500, 600], 1] = 1
    dev = [to_dev(a) for a in (pos, mask, aa)]
    row_off = AN.HOSTILE_ROW_OFF
    exp = V.violations(pos, mask, aa, row_off, TABLE[4], packed=True)
    assert exp["chain_counts"][0, 0] == 0 and exp["chain_counts"][3, 0] <= 4 and exp["clash_partner"][350] == 130 - 120 and exp["clash_partner"][130] == 350 - 120
    assert not exp["clash_count"][[20, 60, 500, 600]].any()
    got = V.run_violations(codec, *dev, to_dev(row_off), 5, R, 2, True, guard=8)
    V.same_violations(got, exp, "hostile row_off")
    V.consistent(got, row_off, packed=True)
    for k in ROW_KEYS:
        assert (got[k][:40] == (-1 if k == "clash_partner" else 0)).all(), k
    assert not got["clash_atom"][:40].any() and got["viol_mask"][40:].sum() > 640
    # no chain at all: every row is uncovered
    none = V.run_violations(codec, *dev, to_dev(row_off), 0, R, 2, True)
    assert not none["clash_atom"].any() and not none["viol_mask"].any() and (none["clash_partner"] == -1).all() and not none["link_cos"].view(np.uint32).any()

    def host_form(arrays, off, n, rows):
        """fcz_violations_packed on host arrays, its outputs between guard bytes"""
        from foldcomp_amd.structure import CViolationsOut
        h = HostGuarded(V.out_spec((rows,), 4, n))
        out = CViolationsOut(*h.ptrs())
        assert codec.lib.fcz_violations_packed(codec.ctx, *(host_ptr(a) for a in arrays), host_ptr(off), n, rows, 2, None, float(V.TOL), float(V.FACTOR),
                                               ctypes.byref(out)) == 0
        return {k: h.fetch(k) for k in V.KEYS}

    # the host form on the same arrays: what the device form gave
    V.same_violations(host_form((pos, mask, aa), row_off, 5, R), got, "fcz_violations_packed n=5")
    V.same_violations(host_form((pos, mask, aa), row_off, 0, R), none, "fcz_violations_packed n=0")
    # chains without a row (R = 0): their counters are 0 and nothing else is written (every other output has no element: all guard)
    one, zeros = (pos[:1], mask[:1], aa[:1]), np.zeros(4, np.uint32)
    for form in (V.run_violations(codec, *(to_dev(a) for a in one), to_dev(zeros), 3, 0, 2, True), host_form(one, zeros, 3, 0)):
        assert form["chain_counts"].shape == (3, 4) and form["chain_counts"].dtype == np.int64 and not form["chain_counts"].any()


def test_refusals_leave_the_outputs_untouched(codec):
    import torch
    n, L, A = 2, 8, 37
    pos, mask, aa, off = AN.refusal_inputs(n, L, A)
    o = V.Outputs((n * L,), A, n)
    big, nan_tab = TABLE[37].copy(), TABLE[37].copy()
    big[3, 5], nan_tab[20, 0] = 8.0, np.nan
    lib, ctx = codec.lib, codec.ctx

    def call(fn, **kw):
        a = dict(ctx=ctx, pos=pos.data_ptr(), mask=mask.data_ptr(), aa=aa.data_ptr(), bound=None, n=n, rows=L, layout=0, table=None, tol=1.5, factor=12.0, out={})
        a.update(kw)
        out = None if a["out"] is None else ctypes.byref(o.struct(**a["out"]))
        return fn(a["ctx"], a["pos"], a["mask"], a["aa"], a["bound"], a["n"], a["rows"], a["layout"], a["table"], a["tol"], a["factor"], out)

    bad = [dict(ctx=None), dict(pos=None), dict(mask=None), dict(out=None), dict(layout=3), dict(layout=-1), dict(rows=2 ** 31), dict(tol=float("nan")),
           dict(tol=float("inf")), dict(tol=-0.5), dict(factor=float("nan")), dict(factor=float("inf")), dict(factor=-12.0), dict(table=big.ctypes.data),
           dict(table=nan_tab.ctypes.data), dict(layout=1, aa=None)] + [dict(out={k: None}) for k in V.KEYS]
    torch.cuda.synchronize()
    for b in bad:
        assert call(lib.fcz_violations_dev, **b) == -1, b
        assert call(lib.fcz_violations_packed_dev, **dict(dict(bound=off.data_ptr(), rows=n * L), **b)) == -1, b
    assert call(lib.fcz_violations_dev, rows=0) == -1                         # L == 0
    assert call(lib.fcz_violations_packed_dev, rows=n * L) == -1              # chains without a row_off
    assert call(lib.fcz_violations_dev, n=0) == 0 and call(lib.fcz_violations_packed_dev, bound=off.data_ptr(), n=0, rows=0) == 0
    codec.synchronize()
    assert o.untouched()


# ---- Python surface -------------------------------------------------------------------------------------------------------------

def _host(d):
    return {k: d[k].cpu().numpy() for k in V.KEYS}


def _three(d, exp, what):
    for k in api.VIOLATION_BATCH_KEYS:
        assert np.array_equal(d[k].cpu().numpy().view(np.uint8), np.asarray(exp[k]).view(np.uint8)), (what, k)


def test_foldcomp_violations(codec, gold, records):
    import torch
    import foldcomp_amd as foldcomp
    n = len(records)
    exp = gold["exp"]["atom37"]
    t = foldcomp.decode_tensors(records, codec=codec, max_len=L_GOLD, violations=True)
    assert t["clash_count"].shape == (n, L_GOLD) and t["clash_count"].dtype == torch.int32 and t["link_violation"].dtype == torch.uint8
    assert t["viol_mask"].dtype == torch.bool and t["clash_count"].device.type == "cuda" and "clash_atom" not in t and "chain_counts" not in t
    _three(t, exp, "decode_tensors(violations=True)")
    plain = foldcomp.decode_tensors(records, codec=codec, max_len=L_GOLD)
    assert not set(V.KEYS) & set(plain)
    out = foldcomp.violations(plain, codec=codec)
    assert set(out) == set(V.KEYS) and out["clash_atom"].shape == (n, L_GOLD, 37) and out["chain_counts"].shape == (n, 4) and out["chain_counts"].dtype == torch.int64
    assert out["link_mask"].dtype == torch.bool and out["link_cos"].shape == (n, L_GOLD, 2)
    V.same_violations(_host(out), exp, "violations")
    kw = foldcomp.violations(pos=plain["pos"], mask=plain["mask"], aatype=plain["aatype"], length=plain["length"], codec=codec)
    V.same_violations(_host(kw), exp, "keywords")
    # the numpy form, a custom table, tolerance and factor
    h14 = gold["host"]["atom14"]
    sub = [h14[k][:6, :200] for k in ("pos", "mask", "aatype")]
    table = TABLE[14] * F(1.1)
    h = codec.violations(*sub, length=h14["length"][:6], radii=table, tolerance=0.5, link_factor=2.0)
    p14 = foldcomp.decode_tensors(records[:6], codec=codec, layout="atom14", max_len=200)
    dev = foldcomp.violations(p14, radii=table, tolerance=0.5, link_factor=2.0, codec=codec)
    V.same_violations(h, _host(dev), "Codec.violations")
    V.same_violations(h, V.violations(*sub, h14["length"][:6], table, F(0.5), F(2.0)), "Codec.violations against the restatement")
    assert h["clash_count"].sum() > 100 and h["link_violation"].any()
    # packed
    p = foldcomp.decode_tensors(records[:12], codec=codec, packed=True, violations=True)
    po = foldcomp.violations(p, codec=codec)
    _three(p, _host(po), "packed decode_tensors")
    full = foldcomp.violations(foldcomp.decode_tensors(records[:12], codec=codec), codec=codec)
    lens = np.diff(p["cu_seqlens"].cpu().numpy())
    V.same_violations(_host(po), _pack_dict(_host(full), lens), "packed against padded")
    # a cropped window's values are the window's own: the restatement of the window alone, with no length
    w = foldcomp.decode_tensors(records, codec=codec, max_len=64, crop="center", layout="backbone4", violations=True)
    wexp = V.violations(w["pos"].cpu().numpy(), w["mask"].cpu().numpy().view(np.uint8), w["aatype"].cpu().numpy(), None, TABLE[4])
    _three(w, wexp, "window")
    V.same_violations(_host(foldcomp.violations(w, codec=codec)), wexp, "window, separate call")
    # nothing to compute
    e = foldcomp.decode_tensors([], codec=codec, max_len=8, violations=True)
    assert e["clash_count"].shape == e["viol_mask"].shape == (0, 8) and foldcomp.violations(e, codec=codec)["clash_atom"].shape == (0, 8, 37)
    e = foldcomp.decode_tensors([], codec=codec, packed=True, violations=True)
    assert e["clash_count"].shape == (0,) and foldcomp.violations(e, codec=codec)["chain_counts"].shape == (0, 4)
    with pytest.raises(ValueError):
        foldcomp.violations(dict(plain, pos=plain["pos"].transpose(0, 1).contiguous().transpose(0, 1)), codec=codec)   # not contiguous
    with pytest.raises(foldcomp.error):
        foldcomp.violations(dict(pos=plain["pos"].cpu(), mask=plain["mask"].cpu()), codec=codec)


def test_tensor_batches_violations(codec, records, tmp_path):
    import foldcomp_amd as foldcomp
    from foldcomp_amd.database import DatabaseWriter
    path = str(tmp_path / "db")
    w = DatabaseWriter(path)
    for k, e in enumerate(records[:6]):
        w.append(e, k, f"entry_{k:02d}")
    w.close()
    api.set_codec(codec)
    try:
        with foldcomp.open(path) as db:
            for packed in (False, True):
                batches = list(db.tensor_batches(4, packed=packed, violations=True))
                assert len(batches) == 2 and all(set(api.VIOLATION_BATCH_KEYS) <= set(b) and "clash_atom" not in b for b in batches)
                sep = foldcomp.violations(batches[0])
                _three(batches[0], {k: sep[k].cpu().numpy() for k in api.VIOLATION_BATCH_KEYS}, packed)
                assert int(batches[0]["viol_mask"].sum()) > 500
            assert not set(api.VIOLATION_BATCH_KEYS) & set(next(iter(db.tensor_batches(4))))
    finally:
        api.set_codec(None)
