"""GPU: a per-entry residue window of the dense tensors (fcz_dense_window_dev, fcz_decompress_dense_window, decode_tensors(crop=...),
tensor_batches(crop=...)). The reference of a window is the UNCROPPED output of fcz_dense_dev at L = the longest entry -- pinned to
the goldens by tests/test_gpu_dense.py -- sliced on the host: row l of entry e is row start[e] + l of it, or a padding row. Every
comparison is on bits, and the device calls write into arrays pre-filled with 0xA5 so that an unwritten byte shows."""
import ctypes

import numpy as np
import pytest

import _dense as D
from _cases import db_cases, entries_blob, golden_records_raw
from _window import KEYS, Decoded, raw_bits, same, sweep_starts, window_of
from foldcomp_amd import fczfile

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def records(golden):
    return golden_records_raw(golden)


@pytest.fixture(scope="module")
def lens(records):
    return np.asarray([fczfile.residue_count(e) for e in records[1]], np.int64)


@pytest.fixture(scope="module")
def decoded(codec, records):
    return Decoded(codec, records[1])


@pytest.fixture(scope="module")
def full(decoded, lens):
    """layout -> fcz_dense_dev at L = the longest entry (1400): computed once, never changed"""
    assert lens.max() == 1400
    return {layout: decoded.dense(layout, 1400) for layout in D.LAYOUTS}


SWEEP = [(layout, L) for layout in D.LAYOUTS for L in (1, 64, 65, 200)]


@pytest.mark.parametrize("layout,L", SWEEP)
def test_starts_sweep_matches_the_sliced_uncropped_output(decoded, full, lens, layout, L):
    shift = SWEEP.index((layout, L))           # over the 12 cases every entry meets every kind of start
    starts = sweep_starts(lens, L, shift)
    got = decoded.dense(layout, L, starts)
    same(got, window_of(full[layout], starts, L), f"{layout} L={L}")
    assert np.array_equal(got["length"], lens)
    assert not got["pos"][got["mask"] == 0].view(np.uint32).any()


def test_oxt_only_in_windows_that_reach_the_last_residue(decoded, full, records, lens):
    L = 64
    has_oxt = np.asarray([D.record_fields(e)[2] for e in records[1]])
    assert has_oxt.sum() == 27 and full["atom37"]["mask"][:, :, 36].sum() == 27
    seen_reach = seen_miss = 0
    for shift in range(11):
        starts = sweep_starts(lens, L, shift).astype(np.int64)
        got = decoded.dense("atom37", L, starts, want=("pos", "mask"))
        reach = has_oxt & (starts <= lens - 1) & (starts + L >= lens)      # from the record fields, not from the output
        assert got["mask"][:, :, 36].sum() == reach.sum(), shift
        for e in np.flatnonzero(reach):
            assert got["mask"][e, lens[e] - 1 - starts[e], 36] == 1, (shift, e)
        seen_reach += int(reach.sum()); seen_miss += int((has_oxt & ~reach).sum())
    assert seen_reach >= 27 and seen_miss >= 27


def test_alt_order_atoms_give_the_same_tensors(codec, records, full, lens):
    alt = Decoded(codec, records[1], alt_order=True)
    for layout, L, shift in (("atom37", 65, 3), ("atom14", 200, 5)):
        starts = sweep_starts(lens, L, shift)
        same(alt.dense(layout, L, starts), window_of(full[layout], starts, L), f"alt {layout}")


@pytest.mark.parametrize("layout", list(D.LAYOUTS))
def test_null_and_zero_starts_are_the_unwindowed_call(decoded, layout):
    for L in (64, 200, 1437):
        plain = decoded.dense(layout, L)
        same(decoded.dense(layout, L, None), plain, f"{layout} NULL L={L}")
        same(decoded.dense(layout, L, np.zeros(56, np.uint32)), plain, f"{layout} zeros L={L}")


def test_damaged_records_between_good_ones(codec, records):
    good = records[1][:6]
    L = 100
    ref_full = Decoded(codec, good).dense("atom37", 1400)
    bad_magic = b"XXXX" + good[1][4:]
    truncated = good[2][:100]
    mixed = [good[0], bad_magic, good[1], truncated, good[2], good[3], good[4], good[5]]
    at = [0, 2, 4, 5, 6, 7]
    starts = np.asarray([5, 7, 0, 3, 40, 64, 1, 65], np.uint32)
    got = Decoded(codec, mixed).dense("atom37", L, starts)
    exp = window_of(ref_full, starts[at], L)
    for k in KEYS:
        assert np.array_equal(raw_bits(got[k][at]), raw_bits(exp[k])), k
    for i in (1, 3):
        assert got["length"][i] == 0 and not got["mask"][i].any() and not got["pos"][i].view(np.uint32).any()
        assert (got["aatype"][i] == 20).all() and not got["plddt"][i].view(np.uint32).any() and not got["res_index"][i].any()
    host = codec.decompress_dense(*entries_blob(mixed), max_len=L, start=starts)
    assert list(host["status"]) == [0, -4, 0, -5, 0, 0, 0, 0]
    same(host, got, "host")


def test_optional_outputs_left_out(decoded, full, lens):
    starts = sweep_starts(lens, 200, 7)
    two = decoded.dense("atom14", 200, starts, want=("pos", "mask"))
    exp = window_of(full["atom14"], starts, 200)
    same(two, {k: exp[k] for k in ("pos", "mask")}, "pos+mask only")


def test_host_form(codec, decoded, full, records, lens):
    entries = records[1]
    blob, off = entries_blob(entries)
    starts = sweep_starts(lens, 64, 2)
    host = codec.decompress_dense(blob, off, layout="atom37", max_len=64, start=starts)
    assert host["mask"].dtype == np.bool_ and not host["status"].any()
    same(host, decoded.dense("atom37", 64, starts), "host L=64")
    # the sizing call: no max_len is the longest entry of the batch
    six, s6 = entries[:6], np.asarray([0, 1, 2, 30, 64, 65], np.uint32)
    L6 = int(lens[:6].max())
    host = codec.decompress_dense(*entries_blob(six), layout="atom14", start=s6)
    assert host["pos"].shape == (6, L6, 14, 3)
    same(host, window_of({k: v[:6] for k, v in full["atom14"].items()}, s6, L6), "host sized")
    w = ctypes.c_uint32(0)
    b6, o6 = entries_blob(six)
    assert codec.lib.fcz_decompress_dense_window(codec.ctx, b6.ctypes.data, o6.ctypes.data, 6, 0, 0, None, ctypes.byref(w), None, None) == 0
    assert w.value == L6
    with pytest.raises(ValueError):
        codec.decompress_dense(blob, off, packed=True, start=starts)
    with pytest.raises(ValueError):
        codec.decompress_dense(blob, off, max_len=64, start=starts[:5])
    with pytest.raises(ValueError):
        codec.decompress_dense(blob, off, max_len=64, start=-np.ones(56, np.int64))


def test_decode_tensors_crop(codec, decoded, records, lens):
    import torch
    import foldcomp_amd as foldcomp
    entries = records[1]
    L = 64
    span = np.maximum(lens - L, 0)
    assert (lens > L).sum() >= 20 and (lens <= L).sum() >= 1

    def host(t):
        return {k: t[k].cpu().numpy() for k in KEYS}

    starts = sweep_starts(lens, L, 4)
    starts[starts > 2 ** 31 - 1] = 2 ** 31 - 1                           # crop_start is int32; anything at or behind the end is padding
    plain = foldcomp.decode_tensors(entries, codec=codec, max_len=L)
    assert "crop_start" not in plain
    for crop in (starts, starts.astype(np.int64).tolist(), torch.from_numpy(starts.astype(np.int64)).to("cuda:0")):
        t = foldcomp.decode_tensors(entries, codec=codec, max_len=L, crop=crop)
        assert set(t) == set(plain) | {"crop_start"} and t["crop_start"].dtype == torch.int32 and t["crop_start"].device.type == "cuda"
        assert np.array_equal(t["crop_start"].cpu().numpy(), starts)
        same(host(t), decoded.dense("atom37", L, starts), "crop=<array>")
    t = foldcomp.decode_tensors(entries, codec=codec, max_len=L, crop="start")
    assert not t["crop_start"].any().item()
    same(host(t), host(plain), "crop=start")
    t = foldcomp.decode_tensors(entries, codec=codec, max_len=L, crop="center", layout="atom14")
    assert np.array_equal(t["crop_start"].cpu().numpy(), span // 2)
    same(host(t), decoded.dense("atom14", L, span // 2), "crop=center")

    def random(seed):
        g = torch.Generator(device="cuda:0"); g.manual_seed(seed)
        return foldcomp.decode_tensors(entries, codec=codec, max_len=L, crop="random", generator=g)

    a, b, c = random(1), random(1), random(2)
    sa, sc = a["crop_start"].cpu().numpy(), c["crop_start"].cpu().numpy()
    assert np.array_equal(sa, b["crop_start"].cpu().numpy())
    same(host(a), host(b), "same seed")
    same(host(a), decoded.dense("atom37", L, sa), "crop=random")
    for s in (sa, sc):
        assert (s >= 0).all() and (s <= span).all() and not s[lens <= L].any()
    assert not np.array_equal(sa, sc)
    g = torch.Generator(); g.manual_seed(5)                               # a generator on the host drives it too
    s = foldcomp.decode_tensors(entries, codec=codec, max_len=L, crop="random", generator=g)["crop_start"].cpu().numpy()
    assert (s >= 0).all() and (s <= span).all()
    e = foldcomp.decode_tensors([], codec=codec, max_len=L, crop="center")
    assert e["pos"].shape == (0, L, 37, 3) and e["crop_start"].shape == (0,)


def test_tensor_batches_crop(codec, golden, tmp_path):
    import torch
    import foldcomp_amd as foldcomp
    from foldcomp_amd import api
    from foldcomp_amd.database import DatabaseWriter
    z, index = golden
    names = db_cases(index)[:12]
    entries = [z[f"{n}/fcz"].tobytes() for n in names]
    path = str(tmp_path / "db")
    w = DatabaseWriter(path)
    for k, e in enumerate(entries):
        w.append(e, k, f"entry_{k:02d}")
    w.close()
    L = 64

    def teq(a, b):
        if a.dtype == torch.float32:
            a, b = a.view(torch.int32), b.view(torch.int32)
        return bool((a == b).all())

    api.set_codec(codec)
    try:
        whole = foldcomp.decode_tensors(entries)
        Lf = whole["pos"].shape[1]
        with foldcomp.open(path) as db:
            runs = [list(db.tensor_batches(5, max_len=L, crop="random", seed=1)) for _ in range(2)]
            other = list(db.tensor_batches(5, max_len=L, crop="random", seed=2))
            assert "crop_start" not in next(iter(db.tensor_batches(5, max_len=L)))
        assert len(runs[0]) == len(runs[1]) == 3
        for b0, b1 in zip(*runs):
            for k in ("pos", "mask", "aatype", "plddt", "res_index", "length", "crop_start"):
                assert teq(b0[k], b1[k]), k
        assert any(not teq(b0["crop_start"], b2["crop_start"]) for b0, b2 in zip(runs[0], other))
        moved = 0
        for b in runs[0]:
            assert b["pos"].shape[1] == L
            for j, i in enumerate(b["index"]):
                i, s, n = int(i), int(b["crop_start"][j]), int(whole["length"][int(i)])
                assert 0 <= s <= max(n - L, 0) and int(b["length"][j]) == n
                m = min(L, Lf - s)
                for key in ("pos", "mask", "aatype", "plddt", "res_index"):
                    assert teq(b[key][j, :m], whole[key][i, s:s + m]), (key, i)
                for key in ("pos", "mask", "plddt", "res_index"):
                    assert not bool(b[key][j, m:].any()), (key, i)
                assert bool((b["aatype"][j, m:] == 20).all())
                moved += s > 0
        assert moved > 0
    finally:
        api.set_codec(None)
