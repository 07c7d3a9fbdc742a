"""GPU: backbone hydrogen bonds and DSSP labels of dense tensors (fcz_hbond_dev, fcz_dssp_labels_dev, their packed and host forms,
Codec.secondary_structure, foldcomp.backbone_hbonds / secondary_structure, decode_tensors(secondary_structure=True)) against the
numpy restatement of the contract (tests/_dssp.py). Indices and labels are compared exactly and energies on bits; the device calls
write into arrays pre-filled with 0xA5 with guard bytes on both sides."""
import numpy as np
import pytest

import _analysis as AN
import _dense as DN
import _dssp as D
import _knn as K
from _analysis import NAN_BITS
from _cases import golden_records_raw
from _devpath import DevGuarded, HostGuarded, host_ptr, to_dev
from foldcomp_amd import _lib

pytestmark = pytest.mark.gpu

L_GOLD = 1400
F = np.float32


@pytest.fixture(scope="module")
def records(golden):
    return golden_records_raw(golden)[1]


@pytest.fixture(scope="module")
def gold(codec, records):
    """the 56 golden records as atom37 / atom14 / backbone4 at L = 1400 on the host and the device, and the restatement on atom37:
    computed once, never changed"""
    host, dev = AN.decoded_layouts(codec, records, L_GOLD, ("pos", "mask", "aatype", "length"))
    a = host["atom37"]
    assert a["length"].max() == L_GOLD
    tables = D.hbonds(a["pos"], a["mask"], a["aatype"], a["length"])
    lab = D.labels(a["pos"], a["mask"], a["length"], tables[0], tables[1])
    return dict(host=host, dev=dev, n=len(records), tables=tables, labels=lab)


def test_golden_padded(codec, gold):
    n = gold["n"]
    ai, ae = to_dev(gold["tables"][0]), to_dev(gold["tables"][1])
    for lay in DN.LAYOUTS:                                                    # atom14 and backbone4 give the bits of atom37
        d = gold["dev"][lay]
        D.same_tables(D.run_hbond(codec, d["pos"], d["mask"], d["aatype"], d["length"], n, L_GOLD, DN.LAYOUTS[lay], False), gold["tables"], lay)
        D.same_labels(D.run_labels(codec, d["pos"], d["mask"], d["aatype"], d["length"], n, L_GOLD, DN.LAYOUTS[lay], False, ai, ae), gold["labels"], lay)
    ss, sm = gold["labels"]
    lens = gold["host"]["atom37"]["length"]
    counts = np.bincount(ss[sm], minlength=8)
    assert counts[1] > 1000 and counts[3] > 200 and (counts[[2, 4, 6, 7]] > 0).all(), counts    # real helices and sheets among the goldens
    for e, m in enumerate(lens):
        assert not ss[e, m:].any() and not sm[e, m:].any() and (gold["tables"][0][e, m:] == -1).all() and not K.bits(gold["tables"][1][e, m:]).any()
    # prolines donate nothing; aatype NULL gives them an amide hydrogen
    pro = (gold["host"]["atom37"]["aatype"] == D.PRO) & sm
    assert pro.sum() > 50 and (gold["tables"][0][pro] == -1).all()
    d = gold["dev"]["atom37"]
    free = D.run_hbond(codec, d["pos"], d["mask"], None, d["length"], n, L_GOLD, 0, False, guard=4)    # outputs that are not 16-byte aligned
    a = gold["host"]["atom37"]
    D.same_tables(free, D.hbonds(a["pos"], a["mask"], None, a["length"]), "aatype NULL")
    assert (free[0][pro] >= 0).any()


def test_golden_packed(codec, gold):
    h = gold["host"]["atom37"]
    lens = np.minimum(h["length"].astype(np.int64), L_GOLD)
    row_off = AN.row_off_of(lens)
    R = int(row_off[-1])
    cat = lambda a: AN.pack1(a, lens)
    exp = D.hbonds(cat(h["pos"]), cat(h["mask"]), cat(h["aatype"]), row_off, packed=True)
    D.same_tables(exp, _shift(gold["tables"], lens, row_off), "restatement, packed against padded")
    for lay in DN.LAYOUTS:
        hh = gold["host"][lay]
        pos, mask, aa, ro = to_dev(cat(hh["pos"])), to_dev(cat(hh["mask"])), to_dev(cat(hh["aatype"])), to_dev(row_off)
        got = D.run_hbond(codec, pos, mask, aa, ro, gold["n"], R, DN.LAYOUTS[lay], True)
        D.same_tables(got, exp, f"packed {lay}")
        lab = D.run_labels(codec, pos, mask, aa, ro, gold["n"], R, DN.LAYOUTS[lay], True, to_dev(got[0]), to_dev(got[1]))
        D.same_labels(lab, [cat(a) for a in gold["labels"]], f"packed labels {lay}")


# ---- synthetic tensors ----------------------------------------------------------------------------------------------------------

def _mirror_chain():
    """six rows: rows 0 and 1 in the plane z = 0 (row 1 has an amide hydrogen in it), rows 3 and 5 mirror images of each other in
    that plane, rows 2 and 4 without a CA: the two acceptors of row 1 tie on every bit of the energy, and the lower row comes first"""
    pos = np.zeros((6, 4, 3), F)
    pos[0] = [[0, 0, 0], [1.4, 0.3, 0], [2.4, -0.7, 0], [2.2, -1.9, 0]]
    pos[1] = [[3.6, -0.2, 0], [4.8, -1.0, 0], [6.0, -0.1, 0], [6.1, 1.1, 0]]
    pos[3] = [[5.5, 5.0, 2.5], [4.5, 4.5, 2.0], [3.9, 3.4, 1.5], [3.8, 2.4, 1.0]]
    pos[5] = pos[3] * np.asarray([1, 1, -1], F)
    pos[2], pos[4] = pos[3] + 1, pos[5] + 1
    mask = np.ones((6, 4), np.uint8)
    mask[[2, 4], 1] = 0
    return pos, mask


def _synthetic(lens, L, seed):
    """backbone4 chains [n, L, 4, 3]: even chains on the integer lattice -1 .. 1 (duplicated atoms, d = 0, ties at -9.9), odd chains
    ideal alpha helices with a jitter of 0.05 (real energies), the chain of length 6 the mirror pair; ~3 % of the rows with one of
    N / CA / C / O cleared (NaN patterns under the cleared masks), per chain of 12 rows or more a NaN, +inf, -inf and two 3e19
    coordinates under set masks, NaN patterns in every row behind the length; aatype random with ~10 % proline"""
    rng = np.random.default_rng(seed)
    n = len(lens)
    pos = np.zeros((n, L, 4, 3), F)
    mask = np.ones((n, L, 4), np.uint8)
    for e, m in enumerate(lens):
        if m == 6:
            pos[e, :6], mask[e, :6] = _mirror_chain()
            continue
        if e % 2:
            pos[e, :m] = D.ideal_backbone(-57, -47, m)[0] + (rng.standard_normal((m, 4, 3)) * 0.05).astype(F) if m else 0
        else:
            pos[e, :m] = rng.integers(-1, 2, size=(m, 4, 3)).astype(F)
        clear = rng.random((m, 4)) < 0.008
        mask[e, :m][clear] = 0
        if m >= 12:
            r = rng.choice(m, size=5, replace=False)
            pos[e, r[0], 0, 0] = np.nan; pos[e, r[1], 1, 1] = np.inf; pos[e, r[2], 3, 2] = -np.inf
            pos[e, r[3], 2, 0] = 3e19; pos[e, r[4], 0, 1] = -3e19
            mask[e, r] = 1
        pos[e, m:] = np.nan
    pos.view(np.uint32)[mask == 0] = NAN_BITS
    aatype = rng.integers(0, 21, size=(n, L)).astype(np.uint8)
    aatype[rng.random((n, L)) < 0.1] = D.PRO
    for e, m in enumerate(lens):
        if m == 6:
            aatype[e, :6] = 0
    return pos, mask, aatype


def _shift(tables, lens, row_off):
    return [np.concatenate([np.where(a[e, :m] >= 0, a[e, :m] + int(row_off[e]), -1).astype(np.int32) if a.dtype == np.int32 else a[e, :m]
                            for e, m in enumerate(lens)]) for a in tables]


@pytest.fixture(scope="module")
def synthetic():
    """lengths 0 .. 6, 255, 256, 257 and P - 1, P, P + 1, 2 P + 3 for the pass size P, as one padded and one packed batch, and the
    restatement with aatype and without"""
    P = _lib.load().fcz_hbond_pass()
    lens = [0, 1, 2, 3, 4, 5, 6, 255, 256, 257, P - 1, P, P + 1, 2 * P + 3]
    L = max(lens)
    pos, mask, aa = _synthetic(lens, L, 11)
    ln = np.asarray(lens, np.uint32)
    row_off = AN.row_off_of(lens)
    exp = D.hbonds(pos, mask, aa, ln)
    lab = D.labels(pos, mask, ln, exp[0], exp[1])
    ai, ae = exp[0], exp[1]
    assert (ae == F(-9.9)).any() and ((ae < 0) & (ae > F(-9.9))).any() and ((ae < 0) & (ae >= F(-0.5))).any()
    tie = (ai[..., 0] >= 0) & (K.bits(ae[..., 0]) == K.bits(ae[..., 1])) & (ai[..., 1] > ai[..., 0])
    assert tie[6, 1] and list(ai[6, 1]) == [3, 5] and ae[6, 1, 0] > F(-9.9) and tie.sum() > 10   # the mirror pair, and the lattice's ties at -9.9
    assert (ai[-1] > P).any() and (ai[-1][P + 5:] >= 0).any() and (ai[-1][P + 5:] < P).any() and (lab[0][-1] == 1).sum() > P
    assert len(np.unique(lab[0])) >= 5
    return dict(lens=ln, L=L, arrays=(pos, mask, aa), row_off=row_off, exp=exp, lab=lab, exp_free=D.hbonds(pos, mask, None, ln))


def test_synthetic_padded_and_packed(codec, synthetic):
    s = synthetic
    n = len(s["lens"])
    pos, mask, aa = (to_dev(a) for a in s["arrays"])
    got = D.run_hbond(codec, pos, mask, aa, to_dev(s["lens"]), n, s["L"], 2, False)
    D.same_tables(got, s["exp"], "padded")
    for e, m in enumerate(s["lens"]):
        assert (got[0][e, m:] == -1).all() and (got[2][e, m:] == -1).all() and not K.bits(got[1][e, m:]).any() and not K.bits(got[3][e, m:]).any()
    D.same_labels(D.run_labels(codec, pos, mask, aa, to_dev(s["lens"]), n, s["L"], 2, False, to_dev(got[0]), to_dev(got[1])), s["lab"], "padded labels")
    D.same_tables(D.run_hbond(codec, pos, mask, None, to_dev(s["lens"]), n, s["L"], 2, False), s["exp_free"], "aatype NULL")
    assert (s["exp_free"][0] >= 0).sum() > (s["exp"][0] >= 0).sum()
    # two calls give the same bits
    D.same_tables(D.run_hbond(codec, pos, mask, aa, to_dev(s["lens"]), n, s["L"], 2, False), got, "again")
    # packed
    packed = AN.pack(s["arrays"], s["lens"])
    R = int(s["row_off"][-1])
    exp_packed = _shift(s["exp"], s["lens"], s["row_off"])
    D.same_tables(D.hbonds(*packed, s["row_off"], packed=True), exp_packed, "restatement, packed")
    pp, pm, pa = (to_dev(a) for a in packed)
    gp = D.run_hbond(codec, pp, pm, pa, to_dev(s["row_off"]), n, R, 2, True)
    D.same_tables(gp, exp_packed, "packed")
    lab_packed = AN.pack(s["lab"], s["lens"])
    D.same_labels(D.run_labels(codec, pp, pm, None, to_dev(s["row_off"]), n, R, 2, True, to_dev(gp[0]), to_dev(gp[1])), lab_packed, "packed labels")
    # the host-pointer forms run both steps
    h = codec.secondary_structure(*s["arrays"], length=s["lens"])
    D.same_tables([h[k] for k in ("hbond_acc_index", "hbond_acc_energy", "hbond_don_index", "hbond_don_energy")], s["exp"], "fcz_dssp")
    D.same_labels((h["ss"], h["ss_mask"]), s["lab"], "fcz_dssp labels")
    h = codec.secondary_structure(*packed, row_off=s["row_off"])
    D.same_tables([h[k] for k in ("hbond_acc_index", "hbond_acc_energy", "hbond_don_index", "hbond_don_energy")], exp_packed, "fcz_dssp_packed")
    D.same_labels((h["ss"], h["ss_mask"]), lab_packed, "fcz_dssp_packed labels")


def test_length_null_and_clamped(codec):
    lens = [40, 300, 257]
    L = 300
    pos, mask, aa = _synthetic([L] * 3, L, 12)                                # finite rows behind every length below
    dev = [to_dev(a) for a in (pos, mask, aa)]
    whole = D.hbonds(pos, mask, aa, None)
    wl = D.labels(pos, mask, None, whole[0], whole[1])
    D.same_tables(D.run_hbond(codec, *dev, None, 3, L, 2, False), whole, "NULL")
    D.same_labels(D.run_labels(codec, *dev, None, 3, L, 2, False, to_dev(whole[0]), to_dev(whole[1])), wl, "NULL labels")
    D.same_tables(D.run_hbond(codec, *dev, to_dev(np.asarray([L + 1, 65535, 0xFFFFFFFF], np.uint32)), 3, L, 2, False), whole, "length > L")
    exp = D.hbonds(pos, mask, aa, lens)
    assert (exp[0] >= 0).sum() < (whole[0] >= 0).sum()
    dl = to_dev(np.asarray(lens, np.uint32))
    D.same_tables(D.run_hbond(codec, *dev, dl, 3, L, 2, False), exp, "length < L")
    D.same_labels(D.run_labels(codec, *dev, dl, 3, L, 2, False, to_dev(exp[0]), to_dev(exp[1])), D.labels(pos, mask, lens, exp[0], exp[1]), "length < L labels")


def test_hostile_row_off(codec):
    R = 700
    pos, mask, aa = (a[0] for a in _synthetic([R], R, 13))
    pos[:] = D.ideal_backbone(-57, -47, R)[0] * (mask[..., None] != 0)
    pos.view(np.uint32)[mask == 0] = NAN_BITS
    dev = [to_dev(a) for a in (pos, mask, aa)]
    row_off = AN.HOSTILE_ROW_OFF
    exp = D.hbonds(pos, mask, aa, row_off, packed=True)
    got = D.run_hbond(codec, *dev, to_dev(row_off), 5, R, 2, True)
    D.same_tables(got, exp, "hostile row_off")
    assert (got[0][:40] == -1).all() and not K.bits(got[1][:40]).any() and (got[0][400] == -1).all() and (got[0][40:120] >= 40).sum() > 40
    assert got[0][:120].max() < 120 and got[0][401:].max() < R and (got[0][401:][got[0][401:] >= 0] >= 401).all()
    lab = D.run_labels(codec, *dev, to_dev(row_off), 5, R, 2, True, to_dev(got[0]), to_dev(got[1]))
    D.same_labels(lab, D.labels(pos, mask, row_off, exp[0], exp[1], packed=True), "hostile row_off labels")
    assert not lab[0][:40].any() and not lab[1][:40].any() and (lab[0][401:] == 1).sum() > 100

    def host_form(n, tables, labels):
        """fcz_dssp_packed on the same host arrays, its outputs between guard bytes: what the two device steps gave"""
        h = HostGuarded(dict(D.table_spec((R,)), ss=(np.uint8, (R,)), ss_mask=(np.uint8, (R,))))
        assert codec.lib.fcz_dssp_packed(codec.ctx, host_ptr(pos), host_ptr(mask), host_ptr(aa), host_ptr(row_off), n, R, 2, *h.ptrs()) == 0
        out = h.all()
        D.same_tables(out[:4], tables, f"fcz_dssp_packed n={n}")
        D.same_labels(out[4:], labels, f"fcz_dssp_packed n={n} labels")

    host_form(5, got, lab)
    # a table that points anywhere: indices outside the chain, outside the arrays, negative -- compared, never followed
    wild = np.random.default_rng(5).integers(-2 ** 31, 2 ** 31, size=(R, 2)).astype(np.int32)
    wild[::3] = got[0][::3]
    ae = np.full((R, 2), -2.0, F)
    lab = D.run_labels(codec, *dev, to_dev(row_off), 5, R, 2, True, to_dev(wild), to_dev(ae))
    D.same_labels(lab, D.labels(pos, mask, row_off, wild, ae, packed=True), "wild table")
    # no chain at all: every row is uncovered
    got = D.run_hbond(codec, *dev, to_dev(row_off), 0, R, 2, True)
    assert (got[0] == -1).all() and (got[2] == -1).all() and not K.bits(got[1]).any() and not K.bits(got[3]).any()
    lab = D.run_labels(codec, *dev, to_dev(row_off), 0, R, 2, True, to_dev(wild), to_dev(ae))
    assert not lab[0].any() and not lab[1].any()
    host_form(0, got, lab)


def test_label_kernel_alone_on_random_tables(codec):
    rng = np.random.default_rng(20261019)
    lens = [int(v) for v in rng.integers(1, 301, 13)] + [300, 1]
    pos, mask, row_off, ai, ae = D.random_label_case(rng, lens)
    R = len(pos)
    assert 1500 < R < 4000
    exp = D.labels(pos, mask, row_off, ai, ae, packed=True)
    counts = np.bincount(exp[0], minlength=8)
    assert (counts >= 10).all(), counts                                        # every class, bridges and ladders of both kinds
    got = D.run_labels(codec, to_dev(pos), to_dev(mask), None, to_dev(row_off), len(lens), R, 2, True, to_dev(ai), to_dev(ae))
    D.same_labels(got, exp, "random tables, packed")
    # the same chains padded, the table holding rows of the entry
    L, n = max(lens), len(lens)
    ppos, pmask = np.full((n, L, 4, 3), np.nan, F), np.ones((n, L, 4), np.uint8)
    pai, pae = np.full((n, L, 2), -1, np.int32), np.zeros((n, L, 2), F)
    for e, m in enumerate(lens):
        lo = int(row_off[e])
        ppos[e, :m], pmask[e, :m], pai[e, :m], pae[e, :m] = pos[lo:lo + m], mask[lo:lo + m], ai[lo:lo + m] - lo, ae[lo:lo + m]
    got = D.run_labels(codec, to_dev(ppos), to_dev(pmask), None, to_dev(np.asarray(lens, np.uint32)), n, L, 2, False, to_dev(pai), to_dev(pae))
    for k in range(2):
        assert np.array_equal(np.concatenate([got[k][e, :m] for e, m in enumerate(lens)]), np.asarray(exp[k]).view(np.uint8))
        assert not any(got[k][e, m:].any() for e, m in enumerate(lens))


def test_refusals_leave_the_outputs_untouched(codec):
    import torch
    n, L, A = 2, 8, 37
    pos, mask, _, off = AN.refusal_inputs(n, L, A)
    g = DevGuarded(D.table_spec((n * L,)))
    o = g.ptrs()
    lib, ctx, P, M, O = codec.lib, codec.ctx, pos.data_ptr(), mask.data_ptr(), off.data_ptr()
    ok = dict(ctx=ctx, pos=P, mask=M, aa=None, bound=None, n=n, L=L, layout=0, o0=o[0], o1=o[1], o2=o[2], o3=o[3])
    bad = [dict(ctx=None), dict(pos=None), dict(mask=None), dict(o0=None), dict(o1=None), dict(o2=None), dict(o3=None), dict(layout=3), dict(layout=-1),
           dict(L=2 ** 31), dict(L=0)]
    torch.cuda.synchronize()
    for b in bad:
        assert lib.fcz_hbond_dev(*dict(ok, **b).values()) == -1, b
        assert lib.fcz_dssp_labels_dev(*dict(ok, **b).values()) == -1, b
    for b in bad[:-1]:
        a = dict(ok, bound=O, L=n * L)
        a.update(b)
        assert lib.fcz_hbond_packed_dev(*a.values()) == -1 and lib.fcz_dssp_labels_packed_dev(*a.values()) == -1, b
    assert lib.fcz_hbond_packed_dev(*dict(ok, L=n * L).values()) == -1 and lib.fcz_dssp_labels_packed_dev(*dict(ok, L=n * L).values()) == -1
    assert lib.fcz_hbond_dev(*dict(ok, n=0).values()) == 0 and lib.fcz_hbond_packed_dev(*dict(ok, bound=O, L=0).values()) == 0
    assert lib.fcz_dssp_labels_dev(*dict(ok, n=0).values()) == 0 and lib.fcz_dssp_labels_packed_dev(*dict(ok, bound=O, L=0).values()) == 0
    codec.synchronize()
    assert g.untouched()


# ---- Python surface -------------------------------------------------------------------------------------------------------------

TABLES = ("hbond_acc_index", "hbond_acc_energy", "hbond_don_index", "hbond_don_energy")


def _tables(d):
    return [d[k].cpu().numpy() for k in TABLES]


def _labels(d):
    return d["ss"].cpu().numpy(), d["ss_mask"].cpu().numpy()


def test_foldcomp_secondary_structure(codec, gold, records):
    import torch
    import foldcomp_amd as foldcomp
    n = len(records)
    t = foldcomp.decode_tensors(records, codec=codec, secondary_structure=True)
    assert t["ss"].shape == (n, L_GOLD) and t["ss"].dtype == torch.uint8 and t["ss_mask"].dtype == torch.bool and t["ss"].device.type == "cuda"
    assert not set(TABLES) & set(t)
    D.same_labels(_labels(t), gold["labels"], "decode_tensors(secondary_structure=True)")
    plain = foldcomp.decode_tensors(records, codec=codec)
    assert "ss" not in plain and "ss_mask" not in plain
    out = foldcomp.secondary_structure(plain, codec=codec)
    assert set(out) == {"ss", "ss_mask", *TABLES} and out["hbond_acc_index"].dtype == torch.int32 and out["hbond_acc_energy"].dtype == torch.float32
    D.same_labels(_labels(out), gold["labels"], "secondary_structure")
    D.same_tables(_tables(out), gold["tables"], "secondary_structure tables")
    hb = foldcomp.backbone_hbonds(plain, codec=codec)
    assert set(hb) == set(TABLES)
    D.same_tables(_tables(hb), gold["tables"], "backbone_hbonds")
    D.same_tables(_tables(foldcomp.backbone_hbonds(pos=plain["pos"], mask=plain["mask"], aatype=plain["aatype"], length=plain["length"], codec=codec)),
                  gold["tables"], "keywords")
    # hbonds=: the labels follow the table given; without a bond nothing but bends is left
    again = foldcomp.secondary_structure(plain, hbonds=hb, codec=codec)
    D.same_labels(_labels(again), gold["labels"], "hbonds=")
    assert again["hbond_acc_index"] is hb["hbond_acc_index"]
    none = foldcomp.secondary_structure(plain, hbonds=dict(hbond_acc_index=torch.full_like(hb["hbond_acc_index"], -1),
                                                           hbond_acc_energy=torch.zeros_like(hb["hbond_acc_energy"])), codec=codec)
    assert set(np.unique(none["ss"].cpu().numpy())) == {0, 7}
    # the numpy form
    h = codec.secondary_structure(gold["host"]["atom14"]["pos"][:6, :300], gold["host"]["atom14"]["mask"][:6, :300], gold["host"]["atom14"]["aatype"][:6, :300],
                                  length=gold["host"]["atom14"]["length"][:6])
    sub = {k: v[:6, :300].contiguous() for k, v in plain.items() if k in ("pos", "mask", "aatype")}
    dev = foldcomp.secondary_structure(sub, length=plain["length"][:6].contiguous(), codec=codec)
    D.same_tables([h[k] for k in TABLES], _tables(dev), "Codec.secondary_structure")
    D.same_labels((h["ss"], h["ss_mask"]), _labels(dev), "Codec.secondary_structure labels")
    assert (h["ss"] == 1).sum() > 100
    # packed
    p = foldcomp.decode_tensors(records, codec=codec, packed=True, secondary_structure=True)
    cu = p["cu_seqlens"].cpu().numpy()
    lens = np.diff(cu)
    D.same_labels(_labels(p), AN.pack(gold["labels"], lens), "packed decode_tensors")
    po = foldcomp.secondary_structure(p, codec=codec)
    D.same_labels(_labels(po), _labels(p), "packed secondary_structure")
    D.same_tables(_tables(po), _shift(gold["tables"], lens, cu), "packed tables")
    # a cropped window's labels are the window's own: the restatement of the window alone, with no length
    w = foldcomp.decode_tensors(records, codec=codec, max_len=64, crop="center", layout="atom14", secondary_structure=True)
    wp, wm, wa = w["pos"].cpu().numpy(), w["mask"].cpu().numpy().view(np.uint8), w["aatype"].cpu().numpy()
    wt = D.hbonds(wp, wm, wa, None)
    wexp = D.labels(wp, wm, None, wt[0], wt[1])
    D.same_labels(_labels(w), wexp, "window")
    wo = foldcomp.secondary_structure(w, codec=codec)
    D.same_labels(_labels(wo), wexp, "window, separate call")
    D.same_tables(_tables(wo), wt, "window tables")
    st = w["crop_start"].cpu().numpy()
    full = gold["labels"][0]
    differs = [e for e in range(n) if st[e] > 0 and not np.array_equal(wexp[0][e], full[e, st[e]:st[e] + 64])]
    assert differs, "a window cut out of a chain loses the bonds that leave it"
    # nothing to label
    e = foldcomp.decode_tensors([], codec=codec, max_len=8, secondary_structure=True)
    assert e["ss"].shape == (0, 8) and foldcomp.secondary_structure(e, codec=codec)["hbond_acc_index"].shape == (0, 8, 2)
    e = foldcomp.decode_tensors([], codec=codec, packed=True, secondary_structure=True)
    assert e["ss"].shape == (0,) and foldcomp.backbone_hbonds(e, codec=codec)["hbond_don_energy"].shape == (0, 2)
    with pytest.raises(ValueError):
        foldcomp.secondary_structure(dict(plain, pos=plain["pos"].transpose(0, 1).contiguous().transpose(0, 1)), codec=codec)   # not contiguous
    with pytest.raises(foldcomp.error):
        foldcomp.secondary_structure(dict(pos=plain["pos"].cpu(), mask=plain["mask"].cpu()), codec=codec)


def test_tensor_batches_secondary_structure(codec, records, tmp_path):
    import foldcomp_amd as foldcomp
    from foldcomp_amd import api
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
                batches = list(db.tensor_batches(4, packed=packed, secondary_structure=True))
                assert len(batches) == 2 and all("ss" in b and "ss_mask" in b for b in batches)
                D.same_labels(_labels(batches[0]), _labels(foldcomp.secondary_structure(batches[0])), f"tensor_batches packed={packed}")
            assert "ss" not in next(iter(db.tensor_batches(4)))
    finally:
        api.set_codec(None)
