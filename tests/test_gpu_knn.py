"""GPU: the k-nearest-neighbour residue graph (fcz_knn_dev, fcz_knn_packed_dev, their host forms, foldcomp.neighbor_graph,
decode_tensors(neighbors=k), tensor_batches(neighbors=k)) against the numpy restatement of the contract (tests/_knn.py). Every
comparison is on bits; the device calls write into arrays pre-filled with 0xA5 with guard bytes on both sides."""
import numpy as np
import pytest

import _analysis as AN
import _dense as D
import _knn as K
from _analysis import NAN_BITS
from _cases import db_cases, golden_records_raw
from _devpath import DevGuarded, HostGuarded, host_ptr, to_dev
from foldcomp_amd import _lib

pytestmark = pytest.mark.gpu

L_GOLD = 1400


@pytest.fixture(scope="module")
def records(golden):
    return golden_records_raw(golden)[1]


@pytest.fixture(scope="module")
def gold(codec, records):
    """the 56 golden records as atom37 / atom14 / backbone4 at L = 1400 (host and device), the restatement on CA at k = 64 and on
    CB at k = 48: computed once, never changed (a smaller k is the first k columns of the same order)"""
    host, dev = AN.decoded_layouts(codec, records, L_GOLD, ("pos", "mask", "length"))
    a37 = host["atom37"]
    assert a37["length"].max() == L_GOLD
    return dict(host=host, dev=dev, n=len(records), ca=K.knn_padded(a37["pos"], a37["mask"], a37["length"], 1, 64),
                cb=K.knn_padded(a37["pos"], a37["mask"], a37["length"], 3, 48))


def _padded(codec, gold, layout, slot, k, length=True, guard=K.GUARD):
    d = gold["dev"][layout]
    return K.run_dev(codec, d["pos"], d["mask"], d["length"] if length else None, gold["n"], L_GOLD, D.LAYOUTS[layout], slot, k, False, guard)


def _first(exp, k):
    return exp[0][..., :k], exp[1][..., :k]


@pytest.mark.parametrize("k", [1, 30, 48, 64])
def test_golden_padded_ca(codec, gold, k):
    K.same(_padded(codec, gold, "atom37", 1, k), _first(gold["ca"], k), f"CA k={k}")


def test_golden_padded_cb_and_the_other_layouts(codec, gold):
    K.same(_padded(codec, gold, "atom37", 3, 48), gold["cb"], "CB k=48")
    assert (gold["cb"][0][..., 0] == -1).sum() > (gold["ca"][0][..., 0] == -1).sum()          # glycines are no CB site
    K.same(_padded(codec, gold, "atom14", 1, 30), _first(gold["ca"], 30), "atom14 CA")
    K.same(_padded(codec, gold, "backbone4", 1, 30), _first(gold["ca"], 30), "backbone4 CA")
    K.same(_padded(codec, gold, "atom14", 4, 48), gold["cb"], "atom14 CB")
    # outputs that are not 16-byte aligned take the single-element stores
    K.same(_padded(codec, gold, "atom37", 1, 48, guard=4), _first(gold["ca"], 48), "unaligned outputs")


def test_golden_packed(codec, gold):
    h = gold["host"]["atom37"]
    lens = np.minimum(h["length"].astype(np.int64), L_GOLD)
    row_off = AN.row_off_of(lens)
    R = int(row_off[-1])
    pos, mask = AN.pack((h["pos"], h["mask"]), lens)
    for slot, k, exp in ((1, 48, _first(gold["ca"], 48)), (3, 48, gold["cb"]), (1, 3, _first(gold["ca"], 3))):
        ei = np.concatenate([np.where(exp[0][e, :n] >= 0, exp[0][e, :n] + row_off[e], -1) for e, n in enumerate(lens)]).astype(np.int32)
        ed = AN.pack1(exp[1], lens)
        got = K.run_dev(codec, to_dev(pos), to_dev(mask), to_dev(row_off), gold["n"], R, 0, slot, k, True)
        K.same(got, (ei, ed), f"packed slot={slot} k={k}")


# ---- synthetic tensors ----------------------------------------------------------------------------------------------------------

def _synthetic(lens, L, A, slot, seed, behind="nan"):
    """integer-lattice chains [n, L, A, 3]: ~10 % of the sites with a cleared mask (NaN patterns under it), a few sites with a NaN /
    +inf / -inf coordinate, two sites at +-3e19 (their d2 is +inf), NaN patterns in every row behind the length"""
    rng = np.random.default_rng(seed)
    n = len(lens)
    pos = rng.integers(-6, 7, size=(n, L, A, 3)).astype(np.float32)
    mask = np.ones((n, L, A), np.uint8)
    off = rng.random((n, L)) < 0.10
    mask[..., slot][off] = 0
    for e, m in enumerate(lens):
        if m >= 8:
            r = rng.choice(m, size=5, replace=False)
            pos[e, r[0], slot, 0] = np.nan; pos[e, r[1], slot, 1] = np.inf; pos[e, r[2], slot, 2] = -np.inf
            pos[e, r[3], slot, 0] = 3e19; pos[e, r[4], slot, 0] = -3e19
            mask[e, r, slot] = 1
        if behind == "nan":
            pos[e, m:] = np.nan
    pos.view(np.uint32)[mask == 0] = NAN_BITS
    return pos, mask


@pytest.fixture(scope="module")
def synthetic():
    """lengths 0, 1, 2, k, k + 1 (for k = 3 and 64), 63, 64, 65, 129 and 2 * fcz_knn_pass() + 3, as one padded and one packed
    batch on backbone4 / CA, and the restatement at k = 64"""
    P = _lib.load().fcz_knn_pass()
    lens = [0, 1, 2, 3, 4, 63, 64, 65, 129] + ([2 * P + 3] if P else [])
    L = max(lens)
    pos, mask = _synthetic(lens, L, 4, 1, 11)
    row_off = AN.row_off_of(lens)
    ppos, pmask = AN.pack((pos, mask), lens)
    exp = K.knn_padded(pos, mask, np.asarray(lens), 1, 64)
    assert np.isinf(exp[1]).any() and (exp[1] == 0).sum() > 0 and (exp[0][-1, :, -1] >= 0).sum() > P
    return dict(lens=np.asarray(lens, np.uint32), L=L, pos=pos, mask=mask, row_off=row_off, ppos=ppos, pmask=pmask, exp=exp,
                exp_packed=K.knn_packed(ppos, pmask, row_off, 1, 64))


@pytest.mark.parametrize("k", [3, 64])
def test_synthetic_padded_and_packed(codec, synthetic, k):
    s = synthetic
    n = len(s["lens"])
    got = K.run_dev(codec, to_dev(s["pos"]), to_dev(s["mask"]), to_dev(s["lens"]), n, s["L"], 2, 1, k, False)
    K.same(got, _first(s["exp"], k), f"padded k={k}")
    for e, m in enumerate(s["lens"]):
        assert (got[0][e, m:] == -1).all() and not K.bits(got[1][e, m:]).any()
    got = K.run_dev(codec, to_dev(s["ppos"]), to_dev(s["pmask"]), to_dev(s["row_off"]), n, int(s["row_off"][-1]), 2, 1, k, True)
    K.same(got, _first(s["exp_packed"], k), f"packed k={k}")
    # the host-pointer forms give the same arrays
    h = codec.neighbors(s["pos"], s["mask"], k, 1, length=s["lens"])
    K.same((h["index"], h["dist"]), _first(s["exp"], k), "fcz_knn")
    h = codec.neighbors(s["ppos"], s["pmask"], k, 1, row_off=s["row_off"])
    K.same((h["index"], h["dist"]), _first(s["exp_packed"], k), "fcz_knn_packed")


def test_length_null_and_clamped(codec):
    lens = [40, 300, 257]
    L, k = 300, 16
    pos, mask = _synthetic([L] * 3, L, 14, 4, 12, behind="data")               # finite rows behind every length below
    dp, dm = to_dev(pos), to_dev(mask)
    whole = K.knn_padded(pos, mask, None, 4, k)
    K.same(K.run_dev(codec, dp, dm, None, 3, L, 1, 4, k, False), whole, "NULL")
    K.same(K.run_dev(codec, dp, dm, to_dev(np.full(3, L, np.uint32)), 3, L, 1, 4, k, False), whole, "length = L")
    K.same(K.run_dev(codec, dp, dm, to_dev(np.asarray([L + 1, 65535, 0xFFFFFFFF], np.uint32)), 3, L, 1, 4, k, False), whole, "length > L")
    K.same(K.run_dev(codec, dp, dm, to_dev(np.asarray(lens, np.uint32)), 3, L, 1, 4, k, False), K.knn_padded(pos, mask, lens, 4, k), "length < L")


def test_hostile_row_off(codec):
    R, k = 700, 8
    pos, mask = _synthetic([R], R, 4, 1, 13)
    pos, mask = pos[0], mask[0]
    row_off = AN.HOSTILE_ROW_OFF
    exp = K.knn_packed(pos, mask, row_off, 1, k)
    got = K.run_dev(codec, to_dev(pos), to_dev(mask), to_dev(row_off), 5, R, 2, 1, k, True)
    K.same(got, exp, "hostile row_off")
    assert (got[0][:40] == -1).all() and not K.bits(got[1][:40]).any() and (got[0][400] == -1).all()
    assert (got[0][40:120, 0] >= 40).sum() > 50 and got[0][401:].max() < R and (got[0][401:, 0] >= 401).sum() > 250
    # no chain at all: every row is uncovered
    none = K.run_dev(codec, to_dev(pos), to_dev(mask), to_dev(row_off), 0, R, 2, 1, k, True)
    assert (none[0] == -1).all() and not K.bits(none[1]).any()
    # fcz_knn_packed on the same host arrays, its outputs between guard bytes: what the device form gave
    for n, dev_form in ((5, got), (0, none)):
        h = HostGuarded(K.out_spec((R, k)))
        assert codec.lib.fcz_knn_packed(codec.ctx, host_ptr(pos), host_ptr(mask), host_ptr(row_off), n, R, 2, 1, k, *h.ptrs()) == 0
        K.same(h.all(), dev_form, f"fcz_knn_packed n={n}")


def test_refusals_leave_the_outputs_untouched(codec):
    import torch
    n, L, A, k = 2, 8, 37, 4
    pos, mask, _, off = AN.refusal_inputs(n, L, A)
    g = DevGuarded(K.out_spec((n * L * 8,)))
    ip, dp = g.ptrs()
    lib, ctx, P, M, O = codec.lib, codec.ctx, pos.data_ptr(), mask.data_ptr(), off.data_ptr()
    bad = [(None, P, M, None, n, L, 0, 1, k, ip, dp), (ctx, None, M, None, n, L, 0, 1, k, ip, dp), (ctx, P, None, None, n, L, 0, 1, k, ip, dp),
           (ctx, P, M, None, n, L, 0, 1, k, None, dp), (ctx, P, M, None, n, L, 0, 1, k, ip, None), (ctx, P, M, None, n, L, 3, 1, k, ip, dp),
           (ctx, P, M, None, n, L, -1, 1, k, ip, dp), (ctx, P, M, None, n, L, 0, 37, k, ip, dp), (ctx, P, M, None, n, L, 0, -1, k, ip, dp),
           (ctx, P, M, None, n, L, 1, 14, k, ip, dp), (ctx, P, M, None, n, L, 2, 4, k, ip, dp), (ctx, P, M, None, n, L, 0, 1, 0, ip, dp),
           (ctx, P, M, None, n, L, 0, 1, 65, ip, dp), (ctx, P, M, None, n, 0, 0, 1, k, ip, dp)]
    torch.cuda.synchronize()
    for a in bad:
        assert lib.fcz_knn_dev(*a) == -1, a
    for a in bad[:-1]:
        a = a[:3] + (O,) + (n, n * L) + a[6:]
        assert lib.fcz_knn_packed_dev(*a) == -1, a
    assert lib.fcz_knn_packed_dev(ctx, P, M, None, n, n * L, 0, 1, k, ip, dp) == -1        # chains without a row_off
    assert lib.fcz_knn_dev(ctx, P, M, None, 0, L, 0, 1, k, ip, dp) == 0 and lib.fcz_knn_packed_dev(ctx, P, M, O, n, 0, 0, 1, k, ip, dp) == 0
    codec.synchronize()
    assert g.untouched()


# ---- Python surface -------------------------------------------------------------------------------------------------------------

def test_decode_tensors_neighbors(codec, gold, records):
    import torch
    import foldcomp_amd as foldcomp
    plain = foldcomp.decode_tensors(records, codec=codec)
    t = foldcomp.decode_tensors(records, codec=codec, neighbors=48)
    assert set(t) == set(plain) | {"nbr_index", "nbr_dist"} and t["nbr_index"].dtype == torch.int32 and t["nbr_dist"].dtype == torch.float32
    assert t["pos"].shape[1] == L_GOLD and t["nbr_index"].device.type == "cuda"
    K.same((t["nbr_index"].cpu().numpy(), t["nbr_dist"].cpu().numpy()), _first(gold["ca"], 48), "decode_tensors")
    again = foldcomp.decode_tensors(records, codec=codec, neighbors=48)
    assert AN.teq(t["nbr_index"], again["nbr_index"]) and AN.teq(t["nbr_dist"], again["nbr_dist"])
    # packed: the ABI call on the tensors it returns
    pp = foldcomp.decode_tensors(records, codec=codec, packed=True)
    p = foldcomp.decode_tensors(records, codec=codec, packed=True, neighbors=48, neighbor_atom="CB")
    assert set(p) == set(pp) | {"nbr_index", "nbr_dist"}
    R = p["pos"].shape[0]
    abi = K.run_dev(codec, p["pos"], p["mask"].view(torch.uint8), p["cu_seqlens"], len(records), R, 0, 3, 48, True)
    K.same((p["nbr_index"].cpu().numpy(), p["nbr_dist"].cpu().numpy()), abi, "decode_tensors packed")
    g = foldcomp.neighbor_graph(p, k=48, atom="CB", codec=codec)
    assert AN.teq(g["nbr_index"], p["nbr_index"]) and AN.teq(g["nbr_dist"], p["nbr_dist"])
    # a window: the restatement on the returned rows only
    lens = gold["host"]["atom37"]["length"].astype(np.int64)
    starts = np.maximum(lens - 64, 0) // 2
    w = foldcomp.decode_tensors(records, codec=codec, max_len=64, crop=starts, neighbors=30, layout="atom14")
    exp = K.knn_padded(w["pos"].cpu().numpy(), w["mask"].cpu().numpy().view(np.uint8), None, 1, 30)
    K.same((w["nbr_index"].cpu().numpy(), w["nbr_dist"].cpu().numpy()), exp, "window")
    assert (exp[0][lens > 64, :, -1] >= 0).all()
    g = foldcomp.neighbor_graph(w, k=30, codec=codec)                                      # crop_start in the dict: length is not used
    assert AN.teq(g["nbr_index"], w["nbr_index"]) and AN.teq(g["nbr_dist"], w["nbr_dist"])
    e = foldcomp.decode_tensors([], codec=codec, max_len=8, neighbors=5)
    assert e["nbr_index"].shape == (0, 8, 5) and foldcomp.decode_tensors([], codec=codec, packed=True, neighbors=5)["nbr_dist"].shape == (0, 5)


def test_neighbor_graph_model_style_call(codec, gold):
    import torch
    import foldcomp_amd as foldcomp
    d = gold["dev"]["atom37"]
    pos, mask = d["pos"][:6, :200].contiguous(), d["mask"][:6, :200].contiguous().view(torch.bool)
    a = foldcomp.neighbor_graph(pos=pos, mask=mask, k=30, codec=codec)
    b = foldcomp.neighbor_graph(pos=pos, mask=mask, k=30, codec=codec)
    assert AN.teq(a["nbr_index"], b["nbr_index"]) and AN.teq(a["nbr_dist"], b["nbr_dist"])
    exp = K.knn_padded(pos.cpu().numpy(), mask.cpu().numpy().view(np.uint8), None, 1, 30)
    K.same((a["nbr_index"].cpu().numpy(), a["nbr_dist"].cpu().numpy()), exp, "keywords")
    c = foldcomp.neighbor_graph(pos=pos, mask=mask, length=torch.tensor([200, 5, 0, 1, 300, 64], device="cuda:0"), k=4, atom=0, codec=codec)
    exp = K.knn_padded(pos.cpu().numpy(), mask.cpu().numpy().view(np.uint8), [200, 5, 0, 1, 200, 64], 0, 4)
    K.same((c["nbr_index"].cpu().numpy(), c["nbr_dist"].cpu().numpy()), exp, "length")
    with pytest.raises(ValueError):
        foldcomp.neighbor_graph(pos=pos.reshape(1200, 37, 3), mask=mask.reshape(1200, 37), cu_seqlens=torch.tensor([0, 700, 600, 1200], device="cuda:0"),
                                codec=codec)
    with pytest.raises(ValueError):
        foldcomp.neighbor_graph(pos=pos.reshape(1200, 37, 3), mask=mask.reshape(1200, 37), cu_seqlens=torch.tensor([0, 700, 1100], device="cuda:0"),
                                codec=codec)


def test_tensor_batches_neighbors(codec, golden, tmp_path):
    import foldcomp_amd as foldcomp
    from foldcomp_amd import api
    from foldcomp_amd.database import DatabaseWriter
    z, index = golden
    entries = [z[f"{n}/fcz"].tobytes() for n in db_cases(index)[:8]]
    path = str(tmp_path / "db")
    w = DatabaseWriter(path)
    for i, e in enumerate(entries):
        w.append(e, i, f"entry_{i:02d}")
    w.close()
    api.set_codec(codec)
    try:
        with foldcomp.open(path) as db:
            old = set(next(iter(db.tensor_batches(5))))
            for kw in (dict(), dict(packed=True, max_residues=2000)):
                seen = 0
                for b in db.tensor_batches(5, neighbors=30, **kw):
                    assert set(b) >= {"nbr_index", "nbr_dist"} and b["nbr_index"].shape == b["pos"].shape[:-2] + (30,)
                    ref = foldcomp.neighbor_graph(b, k=30)
                    assert AN.teq(ref["nbr_index"], b["nbr_index"]) and AN.teq(ref["nbr_dist"], b["nbr_dist"])
                    seen += len(b["names"])
                assert seen == 8
            assert set(next(iter(db.tensor_batches(5)))) == old and "nbr_index" not in old
    finally:
        api.set_codec(None)
