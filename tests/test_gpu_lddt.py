"""GPU: the per-residue lDDT of two dense tensor batches (fcz_lddt_dev, fcz_lddt_packed_dev, their host forms, Codec.lddt,
foldcomp.lddt) against the numpy restatement of the contract (tests/_lddt.py). The counters are compared exactly and the score on
bits; the device calls write into arrays pre-filled with 0xA5 with guard bytes on both sides."""
import math

import numpy as np
import pytest

import _analysis as AN
import _dense as D
import _knn as K
import _lddt as Q
from _analysis import NAN_BITS
from _cases import golden_records_raw
from _devpath import DevGuarded, HostGuarded, host_ptr, to_dev
from foldcomp_amd import _lib

pytestmark = pytest.mark.gpu

L_GOLD = 1400
F = np.float32
CA = dict(atom37=1, atom14=1, backbone4=1)
CB = dict(atom37=3, atom14=4)


@pytest.fixture(scope="module")
def records(golden):
    return golden_records_raw(golden)[1]


@pytest.fixture(scope="module")
def gold(codec, records):
    """the 56 golden records as atom37 / atom14 / backbone4 at L = 1400: `true` is the decode, `pred` is true plus float32 noise of
    sigma 0.5 A made on the host (the same noise on CA and on CB in every layout; every seventh chain is `true` itself), both on the
    host and the device, and the restatement on CA and on CB: computed once, never changed"""
    host, dev = AN.decoded_layouts(codec, records, L_GOLD, ("pos", "mask", "length"))
    n = len(records)
    rng = np.random.default_rng(17)
    noise = {"CA": (rng.standard_normal((n, L_GOLD, 3)) * 0.5).astype(F), "CB": (rng.standard_normal((n, L_GOLD, 3)) * 0.5).astype(F)}
    for v in noise.values():
        v[::7] = 0
    pred = {}
    for lay in D.LAYOUTS:
        p = host[lay]["pos"].copy()
        p[:, :, CA[lay]] += noise["CA"]
        if lay in CB:
            p[:, :, CB[lay]] += noise["CB"]
        pred[lay] = p
    for lay in D.LAYOUTS:
        dev[lay]["pred"] = to_dev(pred[lay])
    a37 = host["atom37"]
    assert a37["length"].max() == L_GOLD
    ca = Q.lddt_padded(a37["pos"], a37["mask"], pred["atom37"], a37["mask"], a37["length"], 1)
    cb = Q.lddt_padded(a37["pos"], a37["mask"], pred["atom37"], a37["mask"], a37["length"], 3)
    return dict(host=host, pred=pred, dev=dev, n=n, ca=ca, cb=cb)


def _padded(codec, gold, layout, slot, mask_pred=True, length=True, **kw):
    d = gold["dev"][layout]
    return Q.run_dev(codec, d["pos"], d["mask"], d["pred"], d["mask"] if mask_pred else None, d["length"] if length else None, gold["n"], L_GOLD,
                     D.LAYOUTS[layout], slot, False, **kw)


def test_golden_padded(codec, gold):
    Q.same(_padded(codec, gold, "atom37", 1), gold["ca"], "CA")
    score, pairs, hits = gold["ca"]
    lens = gold["host"]["atom37"]["length"]
    assert (pairs.sum(axis=1) > 0).all() and np.array_equal(hits[::7], 4 * pairs[::7]) and (hits[1] < 4 * pairs[1]).any()
    means = [float(Q.chain_mean(pairs[e], hits[e])) for e in range(gold["n"])]
    # noise of sigma 0.5 A per coordinate moves a distance by about 0.7 A: a chain of 100 residues or more (thousands of pairs)
    # cannot keep every pair under 0.5 A, a chain of two or three residues may
    noisy = [m for e, m in enumerate(means) if e % 7 and lens[e] >= 100]
    assert all(m == 1.0 for m in means[::7]) and 0.3 < min(means) and len(noisy) > 20 and max(noisy) < 1.0
    for e, m in enumerate(lens):
        assert not pairs[e, m:].any() and not K.bits(score[e, m:]).any()
    Q.same(_padded(codec, gold, "atom37", 3), gold["cb"], "CB")
    assert (gold["cb"][1] == 0).sum() > (pairs == 0).sum()                                   # glycines are no CB site
    Q.same(_padded(codec, gold, "atom14", 1), gold["ca"], "atom14 CA")
    Q.same(_padded(codec, gold, "backbone4", 1), gold["ca"], "backbone4 CA")
    Q.same(_padded(codec, gold, "atom14", 4), gold["cb"], "atom14 CB")
    # every slot of pred present: the decode's masks are the sites either way; outputs that are not 16-byte aligned
    Q.same(_padded(codec, gold, "atom37", 1, mask_pred=False, guard=4), gold["ca"], "mask_pred NULL, unaligned outputs")


def test_golden_packed(codec, gold):
    h = gold["host"]["atom37"]
    lens = np.minimum(h["length"].astype(np.int64), L_GOLD)
    row_off = AN.row_off_of(lens)
    R = int(row_off[-1])
    cat = lambda a: AN.pack1(a, lens)
    pos, mask, pred = to_dev(cat(h["pos"])), to_dev(cat(h["mask"])), to_dev(cat(gold["pred"]["atom37"]))
    for slot, exp in ((1, gold["ca"]), (3, gold["cb"])):
        got = Q.run_dev(codec, pos, mask, pred, mask, to_dev(row_off), gold["n"], R, 0, slot, True)
        Q.same(got, [cat(a) for a in exp], f"packed slot={slot}")


# ---- synthetic tensors ----------------------------------------------------------------------------------------------------------

def _synthetic(lens, L, A, slot, seed, behind="nan"):
    """integer-lattice chains [n, L, A, 3], pred = true + a small integer step: ~10 % of the sites cleared in mask_true only and
    another ~10 % in mask_pred only (NaN patterns under every cleared mask), per chain of 12 rows or more a NaN / +inf coordinate in
    true, a -inf / NaN one in pred, two sites at +-3e19 in pred only (a pair, d_pred = +inf: no hit) and two in true (d_true = +inf:
    no pair), NaN patterns in every row behind the length"""
    rng = np.random.default_rng(seed)
    n = len(lens)
    true = rng.integers(-6, 7, size=(n, L, A, 3)).astype(F)
    pred = true + rng.integers(-2, 3, size=(n, L, A, 3)).astype(F)
    mt, mp = np.ones((n, L, A), np.uint8), np.ones((n, L, A), np.uint8)
    u = rng.random((n, L))
    mt[..., slot][u < 0.10] = 0
    mp[..., slot][(u >= 0.10) & (u < 0.20)] = 0
    for e, m in enumerate(lens):
        if m >= 12:
            r = rng.choice(m, size=8, replace=False)
            true[e, r[0], slot, 0] = np.nan; true[e, r[1], slot, 1] = np.inf; pred[e, r[2], slot, 2] = -np.inf; pred[e, r[3], slot, 0] = np.nan
            pred[e, r[4], slot, 0] = 3e19; pred[e, r[5], slot, 1] = -3e19
            true[e, r[6], slot, 0] = 3e19; true[e, r[7], slot, 2] = -3e19
            mt[e, r, slot] = 1; mp[e, r, slot] = 1
        if behind == "nan":
            true[e, m:] = np.nan; pred[e, m:] = np.nan
    true.view(np.uint32)[mt == 0] = NAN_BITS
    pred.view(np.uint32)[mp == 0] = NAN_BITS
    return true, mt, pred, mp


@pytest.fixture(scope="module")
def synthetic():
    """lengths 0, 1, 2, 63, 64, 65, 129, 255, 256, 257 and 2 * fcz_lddt_pass() + 3, as one padded and one packed batch on
    backbone4 / CA, and the restatement with mask_pred and without it (`filled`: pred with finite values where mask_pred is
    cleared, which count once no mask says otherwise)"""
    P = _lib.load().fcz_lddt_pass()
    lens = [0, 1, 2, 63, 64, 65, 129, 255, 256, 257, 2 * P + 3]
    L = max(lens)
    t, mt, p, mp = _synthetic(lens, L, 4, 1, 11)
    row_off = AN.row_off_of(lens)
    exp = Q.lddt_padded(t, mt, p, mp, np.asarray(lens), 1)
    score, pairs, hits = exp
    assert ((pairs > 0) & (hits == 0)).any() and (pairs[-1] > P).any() and (hits < 4 * pairs).any() and (hits > 0).any()
    filled = p.copy()
    filled[mp == 0] = 2.0
    return dict(lens=np.asarray(lens, np.uint32), L=L, arrays=(t, mt, p, mp), row_off=row_off, packed=AN.pack((t, mt, p, mp), lens), exp=exp,
                filled=filled, exp_nomask=Q.lddt_padded(t, mt, filled, None, np.asarray(lens), 1))


def test_synthetic_padded_and_packed(codec, synthetic):
    s = synthetic
    n = len(s["lens"])
    t, mt, p, mp = (to_dev(a) for a in s["arrays"])
    got = Q.run_dev(codec, t, mt, p, mp, to_dev(s["lens"]), n, s["L"], 2, 1, False)
    Q.same(got, s["exp"], "padded")
    for e, m in enumerate(s["lens"]):
        assert not got[1][e, m:].any() and not got[2][e, m:].any() and not K.bits(got[0][e, m:]).any()
    pt, pmt, pp, pmp = (to_dev(a) for a in s["packed"])
    R = int(s["row_off"][-1])
    exp_packed = AN.pack(s["exp"], s["lens"])
    Q.same(Q.run_dev(codec, pt, pmt, pp, pmp, to_dev(s["row_off"]), n, R, 2, 1, True), exp_packed, "packed")
    Q.same(Q.lddt_packed(*s["packed"], s["row_off"], 1), exp_packed, "restatement, packed")
    # the host-pointer forms give the same arrays
    h = codec.lddt(s["arrays"][0], s["arrays"][1], s["arrays"][2], s["arrays"][3], 1, length=s["lens"])
    Q.same((h["score"], h["pairs"], h["hits"]), s["exp"], "fcz_lddt")
    h = codec.lddt(s["packed"][0], s["packed"][1], s["packed"][2], s["packed"][3], 1, row_off=s["row_off"])
    Q.same((h["score"], h["pairs"], h["hits"]), exp_packed, "fcz_lddt_packed")


def test_mask_pred_null(codec, synthetic):
    s = synthetic
    n = len(s["lens"])
    t, mt, p = to_dev(s["arrays"][0]), to_dev(s["arrays"][1]), to_dev(s["filled"])
    assert s["exp_nomask"][1].sum() > s["exp"][1].sum()
    Q.same(Q.run_dev(codec, t, mt, p, None, to_dev(s["lens"]), n, s["L"], 2, 1, False), s["exp_nomask"], "padded")
    # with the mask the filled values are not read as data
    Q.same(Q.run_dev(codec, t, mt, p, to_dev(s["arrays"][3]), to_dev(s["lens"]), n, s["L"], 2, 1, False), s["exp"], "padded, masked")
    pt, pmt, pp = (to_dev(a) for a in AN.pack((s["arrays"][0], s["arrays"][1], s["filled"]), s["lens"]))
    got = Q.run_dev(codec, pt, pmt, pp, None, to_dev(s["row_off"]), n, int(s["row_off"][-1]), 2, 1, True)
    Q.same(got, AN.pack(s["exp_nomask"], s["lens"]), "packed")
    h = codec.lddt(s["arrays"][0], s["arrays"][1], s["filled"], None, 1, length=s["lens"])
    Q.same((h["score"], h["pairs"], h["hits"]), s["exp_nomask"], "fcz_lddt")


def _boundary_cutoffs():
    out = []
    for q in (50, 99, 170):
        c = F(math.sqrt(q))
        out += [c, np.nextafter(c, F(np.inf)), np.nextafter(c, F(0))]
    return out


def test_custom_parameters(codec):
    lens = [65, 257, 300]
    L = 300
    arrays = _synthetic(lens, L, 14, 4, 14)
    dev = [to_dev(a) for a in arrays]
    dl = to_dev(np.asarray(lens, np.uint32))
    cases = [(6.5, (0.25, 0.5, 1.0, 8.0)), (15.0, (1.0, 1.0, 2.0, 4.0)), (15.0, (4.0, 0.0, np.inf, -1.0))] + [(float(c), None) for c in _boundary_cutoffs()]
    total = []
    for cutoff, th in cases:
        exp = Q.lddt_padded(*arrays, np.asarray(lens), 4, cutoff, th or Q.THRESHOLDS)
        Q.same(Q.run_dev(codec, *dev, dl, 3, L, 1, 4, False, cutoff=cutoff, thresholds=th), exp, f"cutoff={cutoff!r} thresholds={th}")
        total.append(int(exp[1].sum()))
    assert total[0] < total[1] == total[2]
    # the pairs at d2 == q are excluded at float32(sqrt(q)) and below it, included one ulp above
    for c, up, down in zip(total[3::3], total[4::3], total[5::3]):
        assert up > c == down


def test_length_null_and_clamped(codec):
    lens = [40, 300, 257]
    L = 300
    arrays = _synthetic([L] * 3, L, 14, 4, 12, behind="data")                  # finite rows behind every length below
    dev = [to_dev(a) for a in arrays]
    whole = Q.lddt_padded(*arrays, None, 4)
    Q.same(Q.run_dev(codec, *dev, None, 3, L, 1, 4, False), whole, "NULL")
    Q.same(Q.run_dev(codec, *dev, to_dev(np.full(3, L, np.uint32)), 3, L, 1, 4, False), whole, "length = L")
    Q.same(Q.run_dev(codec, *dev, to_dev(np.asarray([L + 1, 65535, 0xFFFFFFFF], np.uint32)), 3, L, 1, 4, False), whole, "length > L")
    exp = Q.lddt_padded(*arrays, lens, 4)
    assert exp[1].sum() < whole[1].sum()
    Q.same(Q.run_dev(codec, *dev, to_dev(np.asarray(lens, np.uint32)), 3, L, 1, 4, False), exp, "length < L")


def test_hostile_row_off(codec):
    R = 700
    arrays = [a[0] for a in _synthetic([R], R, 4, 1, 13)]
    dev = [to_dev(a) for a in arrays]
    row_off = AN.HOSTILE_ROW_OFF
    exp = Q.lddt_packed(*arrays, row_off, 1)
    got = Q.run_dev(codec, *dev, to_dev(row_off), 5, R, 2, 1, True)
    Q.same(got, exp, "hostile row_off")
    assert not got[1][:40].any() and not K.bits(got[0][:40]).any() and got[1][400] == 0
    assert (got[1][40:120] > 0).sum() > 40 and (got[1][401:] > 0).sum() > 200 and got[1][401:].max() < R - 401
    # no chain at all: every row is uncovered
    none = Q.run_dev(codec, *dev, to_dev(row_off), 0, R, 2, 1, True)
    assert not none[1].any() and not none[2].any() and not K.bits(none[0]).any()
    # fcz_lddt_packed on the same host arrays, its outputs between guard bytes: what the device form gave
    for n, dev_form in ((5, got), (0, none)):
        h = HostGuarded(Q.out_spec((R,)))
        assert codec.lib.fcz_lddt_packed(codec.ctx, *(host_ptr(a) for a in arrays), host_ptr(row_off), n, R, 2, 1, 15.0, None, *h.ptrs()) == 0
        Q.same(h.all(), dev_form, f"fcz_lddt_packed n={n}")


def test_refusals_leave_the_outputs_untouched(codec):
    import torch
    n, L, A = 2, 8, 37
    pos, mask, _, off = AN.refusal_inputs(n, L, A)
    g = DevGuarded(Q.out_spec((n * L,)))
    sp, pp, hp = g.ptrs()
    lib, ctx, P, M, O = codec.lib, codec.ctx, pos.data_ptr(), mask.data_ptr(), off.data_ptr()
    nan_th = np.asarray([0.5, 1, np.nan, 4], F)
    ok = dict(ctx=ctx, pt=P, mt=M, pp=P, mp=M, bound=None, n=n, L=L, layout=0, slot=1, cutoff=15.0, th=None, score=sp, pairs=pp, hits=hp)
    bad = [dict(ctx=None), dict(pt=None), dict(mt=None), dict(pp=None), dict(score=None), dict(pairs=None), dict(hits=None), dict(layout=3), dict(layout=-1),
           dict(slot=37), dict(slot=-1), dict(layout=1, slot=14), dict(layout=2, slot=4), dict(cutoff=0.0), dict(cutoff=-1.0), dict(cutoff=float("nan")),
           dict(cutoff=float("inf")), dict(th=nan_th.ctypes.data), dict(L=2 ** 29 + 1), dict(L=0)]
    torch.cuda.synchronize()
    for b in bad:
        assert lib.fcz_lddt_dev(*dict(ok, **b).values()) == -1, b
    for b in bad[:-1]:
        a = dict(ok, bound=O, L=n * L)
        a.update(b)
        assert lib.fcz_lddt_packed_dev(*a.values()) == -1, b
    assert lib.fcz_lddt_packed_dev(*dict(ok, L=n * L).values()) == -1                        # chains without a row_off
    assert lib.fcz_lddt_dev(*dict(ok, n=0).values()) == 0 and lib.fcz_lddt_packed_dev(*dict(ok, bound=O, L=0).values()) == 0
    codec.synchronize()
    assert g.untouched()


# ---- Python surface -------------------------------------------------------------------------------------------------------------

def _np(d):
    return AN.to_numpy(d, ("lddt", "lddt_pairs", "lddt_hits"))


def _noisy(t, seed):
    import torch
    gen = torch.Generator(device=t["pos"].device); gen.manual_seed(seed)
    return t["pos"] + 0.5 * torch.randn(t["pos"].shape, device=t["pos"].device, generator=gen)


def test_foldcomp_lddt(codec, gold, records):
    import torch
    import foldcomp_amd as foldcomp
    n = len(records)
    t = foldcomp.decode_tensors(records, codec=codec)
    pred = _noisy(t, 3)
    out = foldcomp.lddt(dict(pos=pred, mask=t["mask"]), t, codec=codec)
    assert set(out) == {"lddt", "lddt_pairs", "lddt_hits", "lddt_chain"} and out["lddt"].dtype == torch.float32 and out["lddt_pairs"].dtype == torch.int32
    assert out["lddt_hits"].dtype == torch.int32 and out["lddt_chain"].dtype == torch.float32 and out["lddt"].device.type == "cuda"
    assert out["lddt"].shape == (n, L_GOLD) and out["lddt_chain"].shape == (n,)
    mask = t["mask"].cpu().numpy().view(np.uint8)
    exp = Q.lddt_padded(t["pos"].cpu().numpy(), mask, pred.cpu().numpy(), mask, t["length"].cpu().numpy(), 1)
    Q.same(_np(out), exp, "padded")
    chain = np.asarray([Q.chain_mean(exp[1][e], exp[2][e]) for e in range(n)], F)
    assert np.array_equal(K.bits(out["lddt_chain"].cpu().numpy()), K.bits(chain)) and 0.3 < chain.min() and chain.max() < 1
    # pred as a bare tensor, CB, other parameters
    cb = foldcomp.lddt(pred, t, atom="CB", cutoff=8.0, thresholds=(0.5, 1, 2, 3), codec=codec)
    Q.same(_np(cb), Q.lddt_padded(t["pos"].cpu().numpy(), mask, pred.cpu().numpy(), None, t["length"].cpu().numpy(), 3, 8.0, (0.5, 1, 2, 3)), "bare tensor")
    # packed
    p = foldcomp.decode_tensors(records, codec=codec, packed=True)
    ppred = _noisy(p, 4)
    po = foldcomp.lddt(ppred, p, codec=codec)
    cu = p["cu_seqlens"].cpu().numpy()
    pm = p["mask"].cpu().numpy().view(np.uint8)
    pexp = Q.lddt_packed(p["pos"].cpu().numpy(), pm, ppred.cpu().numpy(), None, cu, 1)
    Q.same(_np(po), pexp, "packed")
    pchain = np.asarray([Q.chain_mean(pexp[1][cu[e]:cu[e + 1]], pexp[2][cu[e]:cu[e + 1]]) for e in range(n)], F)
    assert po["lddt"].shape == (int(cu[-1]),) and np.array_equal(K.bits(po["lddt_chain"].cpu().numpy()), K.bits(pchain))
    abi = Q.run_dev(codec, p["pos"], p["mask"].view(torch.uint8), ppred, None, p["cu_seqlens"], n, int(cu[-1]), 0, 1, True)
    Q.same(_np(po), abi, "packed against the ABI call")
    # a window: crop_start in the dict, length is not used
    w = foldcomp.decode_tensors(records, codec=codec, max_len=64, crop="center", layout="atom14")
    wpred = _noisy(w, 5)
    wo = foldcomp.lddt(dict(pos=wpred), w, atom="CB", codec=codec)
    wm = w["mask"].cpu().numpy().view(np.uint8)
    wexp = Q.lddt_padded(w["pos"].cpu().numpy(), wm, wpred.cpu().numpy(), None, None, 4)
    Q.same(_np(wo), wexp, "window")
    assert (wexp[1][gold["host"]["atom37"]["length"] > 64] > 0).any(axis=1).all()
    # nothing to score
    e = foldcomp.lddt(torch.zeros((0, 8, 37, 3), device="cuda:0"), foldcomp.decode_tensors([], codec=codec, max_len=8), codec=codec)
    assert e["lddt"].shape == (0, 8) and e["lddt_chain"].shape == (0,)
    e = foldcomp.decode_tensors([], codec=codec, packed=True)
    assert foldcomp.lddt(e["pos"], e, codec=codec)["lddt_chain"].shape == (0,)
    with pytest.raises(ValueError):
        foldcomp.lddt(pred[:, :, :14].contiguous(), t, codec=codec)
    with pytest.raises(ValueError):
        foldcomp.lddt(pred.transpose(0, 1).contiguous().transpose(0, 1), t, codec=codec)      # not contiguous
    with pytest.raises(foldcomp.error):
        foldcomp.lddt(pred.cpu(), t, codec=codec)


def test_codec_lddt_against_the_device_call(codec, gold):
    h, d = gold["host"]["atom14"], gold["dev"]["atom14"]
    sl = slice(0, 6)
    got = codec.lddt(h["pos"][sl, :300], h["mask"][sl, :300], gold["pred"]["atom14"][sl, :300], None, 4, length=h["length"][sl], cutoff=10.0)
    dev = Q.run_dev(codec, d["pos"][sl, :300].contiguous(), d["mask"][sl, :300].contiguous(), d["pred"][sl, :300].contiguous(), None, d["length"][sl].contiguous(),
                    6, 300, 1, 4, False, cutoff=10.0)
    Q.same((got["score"], got["pairs"], got["hits"]), dev, "Codec.lddt")
    assert got["pairs"].sum() > 0
    assert codec.lddt(h["pos"][:0], h["mask"][:0], h["pos"][:0])["score"].shape == (0, L_GOLD)


def test_the_codec_loss_in_lddt(codec, records):
    """decode -> encode_tensors -> decode: what the codec's quantisation costs in lDDT-CA. The mean is printed, not bounded: nobody
    has measured it before (DESIGN section 6.10 records it)."""
    import foldcomp_amd as foldcomp
    first = foldcomp.decode_tensors(records, codec=codec)
    second = foldcomp.decode_tensors(foldcomp.encode_tensors(first, codec=codec), codec=codec, max_len=L_GOLD)
    out = foldcomp.lddt(second, first, codec=codec)
    mask = first["mask"].cpu().numpy().view(np.uint8)
    exp = Q.lddt_padded(first["pos"].cpu().numpy(), mask, second["pos"].cpu().numpy(), second["mask"].cpu().numpy().view(np.uint8),
                        first["length"].cpu().numpy(), 1)
    Q.same(_np(out), exp, "codec loss")
    chain = out["lddt_chain"].cpu().numpy()
    print(f"lDDT-CA of decode(encode(decode(x))) against decode(x), 56 golden chains: mean {chain.mean():.6f}, min {chain.min():.6f}; "
          f"per residue: mean {exp[0][exp[1] > 0].mean():.6f}, min {exp[0][exp[1] > 0].min():.6f}")
