"""GPU: a per-entry residue window of the angle tensors (fcz_angles_window_dev, fcz_decompress_angles_window, decode_angles(crop=...),
decode_tensors(crop=..., angles=True)). The expectation of a window is the uncropped padded expectation of tests/_angles.py sliced
on the host: row l of entry e is row start[e] + l of it, or zeros. Values by bit pattern, masks equal; the device calls write into
0xFF-filled arrays with a guard band in front and behind."""
import ctypes

import numpy as np
import pytest

import _angles as A
from _cases import entries_blob, golden_records
from _devpath import DevRecords, to_dev
from _window import Decoded, sweep_starts
from foldcomp_amd import _lib
from foldcomp_amd.tensors import _aatype_rows

pytestmark = pytest.mark.gpu

W = A.COLS
GUARD = 4096
SYNTHETIC = [2, 3, 63, 64, 65, 128, 129, 300]  # both sides of the 64-row steps of the walk in front of a window and of its tiles


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint8)


def same(got_ang, got_msk, exp_ang, exp_msk, what):
    assert got_ang.shape == exp_ang.shape and got_msk.shape == exp_msk.shape, (what, got_ang.shape, exp_ang.shape)
    assert np.array_equal(bits(got_msk), bits(exp_msk)), (what, "mask", np.argwhere(bits(got_msk) != bits(exp_msk))[:4])
    assert np.array_equal(bits(got_ang), bits(exp_ang)), (what, "angles", np.argwhere(bits(got_ang) != bits(exp_ang))[:4])


def window_dev(codec, rec, L, start, aatype=True, plain=False):
    """fcz_angles_window_dev (plain: fcz_angles_dev) on sized records into guarded, 0xFF-filled arrays -> (angles [n, L, 10], mask,
    aatype [n, L] or None) on the host; start None = a NULL start_dev"""
    import torch
    rows = rec.n * L
    raw = [torch.full((2 * GUARD + rows * k,), 0xFF, dtype=torch.uint8, device="cuda:0") for k in (W * 4, W, 1)]
    st = None if start is None else to_dev(np.asarray(start, np.uint32))
    torch.cuda.synchronize()
    head = (codec.ctx, rec.blob_t.data_ptr(), rec.off_t.data_ptr(), rec.n, rec.res_off_t.data_ptr(), L)
    if plain:
        _lib.check(codec.lib.fcz_angles_dev(*head, raw[0].data_ptr() + GUARD, raw[1].data_ptr() + GUARD), "fcz_angles_dev")
    else:
        _lib.check(codec.lib.fcz_angles_window_dev(*head, None if st is None else st.data_ptr(), raw[0].data_ptr() + GUARD, raw[1].data_ptr() + GUARD,
                                                   raw[2].data_ptr() + GUARD if aatype else None), "fcz_angles_window_dev")
    codec.synchronize()
    h = [r.cpu().numpy() for r in raw]
    for x in h:
        assert (x[:GUARD] == 0xFF).all() and (x[len(x) - GUARD:] == 0xFF).all(), "guard band written"
    body = [x[GUARD:len(x) - GUARD] for x in h]
    if not aatype or plain:
        assert (body[2] == 0xFF).all()
    return body[0].view(np.float32).reshape(rec.n, L, W), body[1].reshape(rec.n, L, W), body[2].reshape(rec.n, L) if aatype and not plain else None


def window_of(full_ang, full_msk, starts, L):
    n, Lf, _ = full_ang.shape
    ang = np.zeros((n, L, W), np.float32); msk = np.zeros((n, L, W), np.uint8)
    for e, s in enumerate(starts):
        s = int(s)
        if s < Lf:
            m = min(L, Lf - s)
            ang[e, :m] = full_ang[e, s:s + m]; msk[e, :m] = full_msk[e, s:s + m]
    return ang, msk


@pytest.fixture(scope="module")
def cases(codec, golden):
    """name -> (records, their lengths, the uncropped padded expectation, the records sized on the device): built once"""
    out = {}
    for name, entries in (("golden", list(golden_records(golden))), ("synthetic", A.synthetic_records(SYNTHETIC, seed=21))):
        exp = [A.entry_expected(e) for e in entries]
        lens = np.asarray([0 if x is None else len(x[0]) for x in exp], np.int64)    # (a record that does not decode: no rows)
        rec = DevRecords(*entries_blob(entries))
        ro, _ = rec.sizes(codec)
        assert np.array_equal(np.diff(ro.astype(np.int64)), lens)
        out[name] = (entries, lens, A.padded_expected(exp, int(lens.max())), rec)
    assert list(out["synthetic"][1]) == SYNTHETIC
    return out


SWEEP = [(name, L) for name in ("golden", "synthetic") for L in (1, 64, 65, 200)]


@pytest.mark.parametrize("name,L", SWEEP)
def test_starts_sweep_matches_the_sliced_uncropped_expectation(codec, cases, name, L):
    entries, lens, (f_ang, f_msk), rec = cases[name]
    for shift in range(11) if name == "synthetic" else (SWEEP.index((name, L)), SWEEP.index((name, L)) + 5):
        starts = sweep_starts(lens, L, shift)
        ang, msk, _ = window_dev(codec, rec, L, starts)
        same(ang, msk, *window_of(f_ang, f_msk, starts, L), f"{name} L={L} shift={shift}")
        assert msk.max() <= 1 and not ang[msk == 0].view(np.uint32).any()


def test_first_row_of_a_window_inside_the_chain_has_phi_and_n_ca_c(codec, cases):
    for name in ("golden", "synthetic"):
        entries, lens, (f_ang, f_msk), rec = cases[name]
        L = 64
        for s in (1, 64, 65):
            ang, msk, _ = window_dev(codec, rec, L, np.full(len(lens), s))
            inside = lens > s
            assert inside.any() and msk[inside][:, 0, [0, 3]].all() and not msk[~inside].any(), (name, s)
            same(ang, msk, *window_of(f_ang, f_msk, np.full(len(lens), s), L), f"{name} start={s}")
            ends_inside = lens > s + L                                       # the last row has what lies behind it
            assert msk[ends_inside][:, L - 1, [1, 2, 4, 5]].all()
            ends_here = lens == s + L
            assert not msk[ends_here][:, L - 1, [1, 2, 4, 5]].any()
        _, msk, _ = window_dev(codec, rec, L, np.zeros(len(lens)))
        assert not msk[:, 0, [0, 3]].any()


def test_windowed_aatype_is_the_windowed_dense_aatype(codec, cases):
    for name in ("golden", "synthetic"):
        entries, lens, _, rec = cases[name]
        dec = Decoded(codec, entries)
        for L, shift in ((64, 0), (65, 6), (200, 9)):
            starts = sweep_starts(lens, L, shift)
            _, _, aa = window_dev(codec, rec, L, starts)
            assert np.array_equal(aa, dec.dense("atom14", L, starts, want=("pos", "mask", "aatype"))["aatype"]), (name, L)
        _, _, aa = window_dev(codec, rec, 64, None)
        assert np.array_equal(aa, dec.dense("backbone4", 64, want=("pos", "mask", "aatype"))["aatype"]), name


def test_null_start_is_the_unwindowed_call(codec, cases):
    for name in ("golden", "synthetic"):
        entries, lens, (f_ang, f_msk), rec = cases[name]
        for L in (1, 64, 100, int(lens.max()) + 37):
            p_ang, p_msk, _ = window_dev(codec, rec, L, None, plain=True)
            for start, aatype in ((None, True), (None, False), (np.zeros(len(lens)), True)):
                ang, msk, _ = window_dev(codec, rec, L, start, aatype=aatype)
                same(ang, msk, p_ang, p_msk, f"{name} L={L}")


def test_same_output_before_and_after_a_decode_and_the_decode_is_unchanged(codec, cases):
    entries, lens, _, _ = cases["golden"]
    plain = DevRecords(*entries_blob(entries)).decompress(codec)            # sizes, then the decode: no angle call in between
    rec = DevRecords(*entries_blob(entries))
    rec.sizes(codec)
    starts = sweep_starts(lens, 100, 3)
    before = window_dev(codec, rec, 100, starts)
    got = rec.batch(codec)                                                  # the decode that follows the sizes call on the same pointers
    for k in ("x", "y", "z", "bfac_res", "res_code", "atom_code"):
        assert np.array_equal(bits(got[k]), bits(plain[k])), k
    after = window_dev(codec, rec, 100, starts)
    same(after[0], after[1], before[0], before[1], "after the decode")
    assert np.array_equal(after[2], before[2])


def test_torch_surfaces_share_one_crop_start(codec, cases):
    import torch
    import foldcomp_amd as foldcomp
    entries, lens, (f_ang, f_msk), rec = cases["golden"]
    L = 64
    span = np.maximum(lens - L, 0)
    g = torch.Generator(device="cuda:0"); g.manual_seed(7)
    t = foldcomp.decode_tensors(entries, codec=codec, max_len=L, crop="random", generator=g, angles=True)
    s = t["crop_start"].cpu().numpy()
    assert (s >= 0).all() and (s <= span).all() and s.any()
    same(t["angles"].cpu().numpy(), t["angle_mask"].cpu().numpy(), *window_of(f_ang, f_msk, s, L), "decode_tensors(angles=True)")
    a = foldcomp.decode_angles(entries, codec=codec, max_len=L, crop=t["crop_start"])
    assert set(a) == {"angles", "angle_mask", "aatype", "length", "names", "crop_start"}
    assert np.array_equal(a["crop_start"].cpu().numpy(), s)
    same(a["angles"].cpu().numpy(), a["angle_mask"].cpu().numpy(), *window_of(f_ang, f_msk, s, L), "decode_angles(crop=)")
    assert np.array_equal(a["aatype"].cpu().numpy(), t["aatype"].cpu().numpy())
    c = foldcomp.decode_angles(entries, codec=codec, max_len=L, crop="center")
    assert np.array_equal(c["crop_start"].cpu().numpy(), span // 2)
    same(c["angles"].cpu().numpy(), c["angle_mask"].cpu().numpy(), *window_of(f_ang, f_msk, span // 2, L), "center")
    host = codec.decompress_angles(*entries_blob(entries), L=L, start=span // 2)
    same(host["angles"], host["angle_mask"], *window_of(f_ang, f_msk, span // 2, L), "host")
    assert np.array_equal(host["aatype"], c["aatype"].cpu().numpy()) and not host["status"].any()
    sized = codec.decompress_angles(*entries_blob(entries), start=np.zeros(len(lens), np.uint32))
    same(sized["angles"], sized["angle_mask"], f_ang, f_msk, "host sized")
    with pytest.raises(ValueError):
        codec.decompress_angles(*entries_blob(entries), packed=True, start=span)
    # without crop: aatype as the record bytes give it, now written by the kernel
    for kw in (dict(), dict(max_len=L)):
        p = foldcomp.decode_angles(entries, codec=codec, **kw)
        assert set(p) == {"angles", "angle_mask", "aatype", "length", "names"}
        Lp = p["aatype"].shape[1]
        exp = np.full((len(entries), Lp), 20, np.uint8)
        for i, (e, k) in enumerate(zip(entries, lens)):
            exp[i, :min(int(k), Lp)] = _aatype_rows(e, min(int(k), Lp))
        assert np.array_equal(p["aatype"].cpu().numpy(), exp) and np.array_equal(p["length"].cpu().numpy(), lens)


def test_argument_refusals(codec, cases):
    import torch
    entries, lens, _, rec = cases["synthetic"]
    lib, INV, n, L = codec.lib, -1, len(lens), 16
    a = torch.zeros(n * L * W, dtype=torch.float32, device="cuda:0")
    m = torch.zeros(n * L * W, dtype=torch.uint8, device="cuda:0")
    good = [codec.ctx, rec.blob_t.data_ptr(), rec.off_t.data_ptr(), n, rec.res_off_t.data_ptr(), L, None, a.data_ptr(), m.data_ptr(), None]
    for i in (0, 1, 2, 4, 7, 8):                                            # ctx, blob, off, res_off, angles, mask
        bad = list(good); bad[i] = None
        assert lib.fcz_angles_window_dev(*bad) == INV, i
    assert lib.fcz_angles_window_dev(*(good[:5] + [0] + good[6:])) == INV   # L == 0
    assert lib.fcz_angles_window_dev(*(good[:3] + [0] + good[4:])) == 0     # n == 0
    blob, off = entries_blob(entries)
    w = ctypes.c_uint32(0)
    head = (codec.ctx, blob.ctypes.data, off.ctypes.data, n, 0, None)
    assert lib.fcz_decompress_angles_window(*head, None, None, None, None, None) == INV
    assert lib.fcz_decompress_angles_window(*head, ctypes.byref(w), blob.ctypes.data, None, None, None) == INV
    assert lib.fcz_decompress_angles_window(*head, ctypes.byref(w), None, None, None, None) == 0 and w.value == lens.max()
