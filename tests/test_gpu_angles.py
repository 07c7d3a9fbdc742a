"""GPU: torsion-angle tensors straight from the record bytes (fcz_angles_dev, fcz_angles_packed_dev, fcz_decompress_angles[_packed],
decode_angles, decode_tensors(angles=True)) against the pure-numpy expectation of tests/_angles.py: values by bit pattern, masks
equal. The device calls write into arrays pre-filled with 0xFF that carry a guard band in front and behind: every byte inside must
have been written, none outside."""
import ctypes

import numpy as np
import pytest

import _angles as A
from _cases import entries_blob, golden_records
from _devpath import DevRecords
from foldcomp_amd import _lib

pytestmark = pytest.mark.gpu

W = A.COLS
GUARD = 4096                                   # bytes in front of and behind every output array
NAMES = ("golden", "synthetic", "all_gly", "trp_last", "single", "truncated")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint8)


def same(got_ang, got_msk, exp_ang, exp_msk, what):
    assert got_ang.shape == exp_ang.shape and got_msk.shape == exp_msk.shape, (what, got_ang.shape, exp_ang.shape)
    assert np.array_equal(bits(got_msk), bits(exp_msk)), (what, "mask", np.argwhere(bits(got_msk) != bits(exp_msk))[:4])
    assert np.array_equal(bits(got_ang), bits(exp_ang)), (what, "angles", np.argwhere(bits(got_ang) != bits(exp_ang))[:4])


def angles_dev(codec, rec, rows, L=None):
    """fcz_angles_dev (L given) or fcz_angles_packed_dev on sized records into guarded, 0xFF-filled arrays -> (angles, mask) on the
    host, flat rows; asserts that the guard bands still hold the fill"""
    import torch
    raw_a = torch.full((2 * GUARD + rows * W * 4,), 0xFF, dtype=torch.uint8, device="cuda:0")
    raw_m = torch.full((2 * GUARD + rows * W,), 0xFF, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    args = (codec.ctx, rec.blob_t.data_ptr(), rec.off_t.data_ptr(), rec.n, rec.res_off_t.data_ptr())
    if L is None:
        _lib.check(codec.lib.fcz_angles_packed_dev(*args, raw_a.data_ptr() + GUARD, raw_m.data_ptr() + GUARD), "fcz_angles_packed_dev")
    else:
        _lib.check(codec.lib.fcz_angles_dev(*args, L, raw_a.data_ptr() + GUARD, raw_m.data_ptr() + GUARD), "fcz_angles_dev")
    codec.synchronize()
    ha, hm = raw_a.cpu().numpy(), raw_m.cpu().numpy()
    for h in (ha, hm):
        assert (h[:GUARD] == 0xFF).all() and (h[len(h) - GUARD:] == 0xFF).all(), "guard band written"
    return ha[GUARD:len(ha) - GUARD].view(np.float32).reshape(rows, W), hm[GUARD:len(hm) - GUARD].reshape(rows, W)


@pytest.fixture(scope="module")
def cases(golden):
    """name -> (records, their expectation per entry): computed once, never changed"""
    return {k: (v, [A.entry_expected(e) for e in v]) for k, v in A.batches(golden_records(golden)).items()}


@pytest.mark.parametrize("name", NAMES)
def test_device_calls_match_the_helper(codec, cases, name):
    entries, exp = cases[name]
    n = len(entries)
    L = max(len(x[0]) for x in exp if x is not None)
    rec = DevRecords(*entries_blob(entries))
    ro, _ = rec.sizes(codec)
    e_ang, e_msk, e_off = A.packed_expected(exp)
    assert np.array_equal(ro, e_off)
    p_ang, p_msk = A.padded_expected(exp, L)
    ang, msk = angles_dev(codec, rec, n * L, L)
    same(ang.reshape(n, L, W), msk.reshape(n, L, W), p_ang, p_msk, f"{name} padded")
    assert msk.max() <= 1 and not ang[msk == 0].view(np.uint32).any()
    ang, msk = angles_dev(codec, rec, int(ro[-1]))
    same(ang, msk, e_ang, e_msk, f"{name} packed")
    if name == "truncated":
        assert exp[1] is None and not p_msk[1].any() and ro[2] == ro[1]


@pytest.mark.parametrize("name", NAMES)
def test_host_and_torch_surfaces_match_the_helper(codec, cases, name):
    import foldcomp_amd as foldcomp
    entries, exp = cases[name]
    L = max(len(x[0]) for x in exp if x is not None)
    e_ang, e_msk, e_off = A.packed_expected(exp)
    p_ang, p_msk = A.padded_expected(exp, L)
    lens = np.diff(e_off.astype(np.int64))
    host = codec.decompress_angles(*entries_blob(entries))
    same(host["angles"], host["angle_mask"], p_ang, p_msk, f"{name} host padded")
    assert np.array_equal(host["status"] == 0, lens > 0)
    host = codec.decompress_angles(*entries_blob(entries), packed=True)
    same(host["angles"], host["angle_mask"], e_ang, e_msk, f"{name} host packed")
    assert np.array_equal(host["row_off"], e_off)
    t = foldcomp.decode_angles(entries, codec=codec)
    assert set(t) == {"angles", "angle_mask", "aatype", "length", "names"} and str(t["angle_mask"].dtype) == "torch.bool"
    same(t["angles"].cpu().numpy(), t["angle_mask"].cpu().numpy(), p_ang, p_msk, f"{name} torch padded")
    assert np.array_equal(t["length"].cpu().numpy(), lens) and len(t["names"]) == len(entries)
    dense = foldcomp.decode_tensors(entries[:8], codec=codec, max_len=L)
    t8 = foldcomp.decode_angles(entries[:8], codec=codec, max_len=L)
    assert np.array_equal(t8["aatype"].cpu().numpy(), dense["aatype"].cpu().numpy())
    t = foldcomp.decode_angles(entries, codec=codec, packed=True)
    assert set(t) == {"angles", "angle_mask", "aatype", "length", "names", "cu_seqlens", "max_seqlen"}
    same(t["angles"].cpu().numpy(), t["angle_mask"].cpu().numpy(), e_ang, e_msk, f"{name} torch packed")
    assert np.array_equal(t["cu_seqlens"].cpu().numpy(), e_off) and t["max_seqlen"] == L
    assert np.array_equal(t["aatype"].cpu().numpy(), foldcomp.decode_tensors(entries, codec=codec, packed=True)["aatype"].cpu().numpy())


def test_crop_keeps_psi_and_omega_of_the_last_row(codec, cases):
    entries, exp = cases["synthetic"]                       # 2 .. 1 100 residues
    rec = DevRecords(*entries_blob(entries))
    rec.sizes(codec)
    for L in (1, 16, 64, 65, 100):
        p_ang, p_msk = A.padded_expected(exp, L)
        ang, msk = angles_dev(codec, rec, len(entries) * L, L)
        same(ang.reshape(-1, L, W), msk.reshape(-1, L, W), p_ang, p_msk, f"L={L}")
        m = msk.reshape(-1, L, W)
        for i, x in enumerate(exp):
            if len(x[0]) > L:
                assert m[i, L - 1, [1, 2, 4, 5]].all(), (L, i)              # word L - 1 exists
            elif len(x[0]) == L:
                assert not m[i, L - 1, [1, 2, 4, 5]].any(), (L, i)
    host = codec.decompress_angles(*entries_blob(entries), L=100)
    same(host["angles"], host["angle_mask"], *A.padded_expected(exp, 100), "host L=100")


def test_same_output_before_and_after_a_decode_and_the_decode_is_unchanged(codec, cases):
    entries, exp = cases["golden"]
    plain = DevRecords(*entries_blob(entries)).decompress(codec)            # sizes, then the decode: no angle call in between
    rec = DevRecords(*entries_blob(entries))
    ro, _ = rec.sizes(codec)
    R, L = int(ro[-1]), 300
    before = angles_dev(codec, rec, R), angles_dev(codec, rec, rec.n * L, L)
    got = rec.batch(codec)                                                  # the decode that follows the sizes call on the same pointers
    for k in ("x", "y", "z", "bfac_res", "res_code", "atom_code"):
        assert np.array_equal(bits(got[k]), bits(plain[k])), k
    after = angles_dev(codec, rec, R), angles_dev(codec, rec, rec.n * L, L)
    for b, a in zip(before, after):
        same(a[0], a[1], b[0], b[1], "after the decode")
    same(*before[0], *A.packed_expected(exp)[:2], "before the decode")


def test_decode_tensors_with_angles(codec, cases):
    import foldcomp_amd as foldcomp
    entries, exp = cases["trp_last"]
    plain = foldcomp.decode_tensors(entries, codec=codec)
    assert set(plain) == {"pos", "mask", "aatype", "plddt", "res_index", "length", "names"}
    assert set(foldcomp.decode_tensors(entries, codec=codec, angles=False)) == set(plain)
    assert set(foldcomp.decode_tensors(entries, codec=codec, packed=True)) == {"pos", "mask", "aatype", "plddt", "res_index", "chain_index",
                                                                               "cu_seqlens", "length", "names", "max_seqlen"}
    for kw in (dict(), dict(max_len=20), dict(packed=True)):
        t = foldcomp.decode_tensors(entries, codec=codec, angles=True, **kw)
        a = foldcomp.decode_angles(entries, codec=codec, **kw)
        p = foldcomp.decode_tensors(entries, codec=codec, **kw)
        assert set(t) == set(p) | {"angles", "angle_mask"}
        same(t["angles"].cpu().numpy(), t["angle_mask"].cpu().numpy(), a["angles"].cpu().numpy(), a["angle_mask"].cpu().numpy(), str(kw))
        for k in ("pos", "mask", "aatype", "plddt", "res_index", "length"):
            assert np.array_equal(bits(t[k].cpu().numpy()) if t[k].dtype.is_floating_point else t[k].cpu().numpy(),
                                  bits(p[k].cpu().numpy()) if p[k].dtype.is_floating_point else p[k].cpu().numpy()), (kw, k)
    same(t["angles"].cpu().numpy(), t["angle_mask"].cpu().numpy(), *A.packed_expected(exp)[:2], "packed")
    e = foldcomp.decode_tensors([], codec=codec, angles=True)
    assert e["angles"].shape == (0, 0, W) and foldcomp.decode_angles([], codec=codec, packed=True)["angles"].shape == (0, W)


def test_argument_refusals(codec, cases):
    import torch
    import foldcomp_amd as foldcomp
    entries, _ = cases["single"]
    rec = DevRecords(*entries_blob(entries))
    ro, _ = rec.sizes(codec)
    lib, INV = codec.lib, -1
    a = torch.zeros(int(ro[-1]) * W, dtype=torch.float32, device="cuda:0")
    m = torch.zeros(int(ro[-1]) * W, dtype=torch.uint8, device="cuda:0")
    good = [codec.ctx, rec.blob_t.data_ptr(), rec.off_t.data_ptr(), 1, rec.res_off_t.data_ptr(), int(ro[-1]), a.data_ptr(), m.data_ptr()]
    for i in (0, 1, 2, 4, 6, 7):
        bad = list(good); bad[i] = None
        assert lib.fcz_angles_dev(*bad) == INV
        assert lib.fcz_angles_packed_dev(*(bad[:5] + bad[6:])) == INV
    assert lib.fcz_angles_dev(*(good[:5] + [0] + good[6:])) == INV                      # L == 0
    assert lib.fcz_angles_dev(*(good[:3] + [0] + good[4:])) == 0 and lib.fcz_angles_packed_dev(*(good[:3] + [0] + good[4:5] + good[6:])) == 0
    blob, off = entries_blob(entries)
    w = ctypes.c_uint32(0)
    assert lib.fcz_decompress_angles(codec.ctx, blob.ctypes.data, off.ctypes.data, 1, 0, None, None, None, None) == INV
    assert lib.fcz_decompress_angles(codec.ctx, blob.ctypes.data, off.ctypes.data, 1, 0, ctypes.byref(w), blob.ctypes.data, None, None) == INV
    assert lib.fcz_decompress_angles_packed(codec.ctx, None, off.ctypes.data, 1, ctypes.byref(w), None, None, None, None) == INV
    assert lib.fcz_decompress_angles_packed(codec.ctx, blob.ctypes.data, off.ctypes.data, 1, ctypes.byref(w), None, None, None, None) == 0
    assert w.value == ro[-1]
    with pytest.raises(ValueError):
        foldcomp.decode_angles(entries, codec=codec, packed=True, max_len=10)
    with pytest.raises(ValueError):
        foldcomp.decode_angles(entries, codec=codec, max_len=0)
    with pytest.raises(ValueError):
        foldcomp.decode_tensors(entries, codec=codec, packed=True, max_len=10, angles=True)
    with pytest.raises(ValueError):
        codec.decompress_angles(blob, off, L=5, packed=True)
    with pytest.raises(foldcomp.error):
        foldcomp.decode_angles(entries, codec=codec, device="cpu")
    with pytest.raises(foldcomp.error):                                     # no such device, or not the codec's
        foldcomp.decode_angles(entries, codec=codec, device="cuda:1")


def test_tensor_batches_with_angles(codec, cases, tmp_path):
    import foldcomp_amd as foldcomp
    from foldcomp_amd import api
    from foldcomp_amd.database import DatabaseWriter
    entries = cases["golden"][0][32:42]                     # ten database records
    path = str(tmp_path / "db")
    w = DatabaseWriter(path)
    for k, e in enumerate(entries):
        w.append(e, k, f"entry_{k:02d}")
    w.close()
    api.set_codec(codec)
    try:
        with foldcomp.open(path) as db:
            assert "angles" not in next(iter(db.tensor_batches(4)))
            for kw in (dict(), dict(max_len=30), dict(packed=True), dict(packed=True, max_residues=400)):
                seen = []
                for b in db.tensor_batches(4, angles=True, sort_by_length=True, **kw):
                    sel = [entries[int(i)] for i in b["index"]]
                    a = foldcomp.decode_angles(sel, codec=codec, **{k: v for k, v in kw.items() if k != "max_residues"})
                    same(b["angles"].cpu().numpy(), b["angle_mask"].cpu().numpy(), a["angles"].cpu().numpy(), a["angle_mask"].cpu().numpy(), str(kw))
                    assert b["angles"].shape[:-1] == b["aatype"].shape and str(b["angle_mask"].dtype) == "torch.bool"
                    seen += [int(i) for i in b["index"]]
                assert sorted(seen) == list(range(10)), kw
    finally:
        api.set_codec(None)
