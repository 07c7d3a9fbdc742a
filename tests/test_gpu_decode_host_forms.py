"""GPU: the host-pointer forms of the record decode (fcz_decompress_batch, fcz_decompress_pdb_begin / _fetch / _sizes, fcz_extract,
fcz_decompress_dense / _window / _packed, fcz_decompress_angles / _window / _packed) against the device forms they stage for, on
bytes, and the corners each form has of its own: the empty batch, a sizing call, a batch none of whose records decodes, the refused
argument combinations. Every host output starts as 0xA5 bytes between guard bytes, so that a byte written where none may be shows.
The device forms themselves are pinned to the goldens by the tests of each entry point; here they are the reference."""
import ctypes

import numpy as np
import pytest

import _dense as D
from _cases import entries_blob
from _devpath import FILL, HostGuarded, to_dev
from _window import KEYS, Decoded
from foldcomp_amd import _lib, synthetic
from foldcomp_amd.structure import CAtomsOut, CDenseOut, CPackedOut

pytestmark = pytest.mark.gpu

LENS = (2, 3, 63, 64, 65, 129)          # 64 rows = DN_TILE, the tile of the dense kernels; 129: a third tile of one row
WIDTHS = (0, 1, 64, 65, 200)            # 0: the longest entry
INVALID = -1                            # FCZ_E_INVALID_ARG
COLS = 10                               # FCZ_ANGLE_COLUMNS
NUL = 0x100                             # FCZ_PDB_NUL_TERMINATED
OPTIONAL = ("aatype", "plddt", "res_index", "length")
DT = dict(pos=np.float32, mask=np.uint8, aatype=np.uint8, plddt=np.float32, res_index=np.int32, chain_index=np.int32, length=np.uint32)
PACKED_KEYS = ("pos", "mask", "aatype", "plddt", "res_index", "chain_index", "length")


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def same_bytes(got, exp, what):
    assert set(got) == set(exp), (what, sorted(got), sorted(exp))
    for k in exp:
        g, e = raw(got[k]), raw(exp[k])
        assert g.shape == e.shape and np.array_equal(g, e), (what, k, g.shape, e.shape)


class Batch:
    """records on the host, and the same records sized and decoded on the device once (the reference of every comparison)"""

    def __init__(self, codec, entries, lens):
        self.entries, self.n, self.lens = entries, len(entries), np.asarray(lens, np.int64)
        self.blob, self.off = entries_blob(entries)
        self.blob = np.concatenate([self.blob, np.zeros(16, np.uint8)])      # (a host array of 0 bytes has no address worth passing)
        self.longest = int(self.lens.max()) if self.n else 0
        self.dev = Decoded(codec, entries)
        self.res_off = self.dev.rec.res_off_t.cpu().numpy().view(np.uint32)
        self.atom_off = self.dev.rec.atom_off_t.cpu().numpy().view(np.uint32)
        assert np.array_equal(np.diff(self.res_off.astype(np.int64)), self.lens)
        self.R, self.M = int(self.res_off[-1]), int(self.atom_off[-1])
        if self.M == 0:                                # (a slice of no element has no address: the device forms refuse NULL atoms)
            import torch
            self.dev.atoms = {k: torch.zeros(1, dtype=v.dtype, device=v.device) for k, v in self.dev.atoms.items()}

    def head(self, codec):
        return codec.ctx, self.blob.ctypes.data, self.off.ctypes.data, self.n


@pytest.fixture(scope="module")
def batches(codec):
    b = synthetic.to_chain_batch(synthetic.generate(len(LENS), list(LENS), seed=4242))
    blob, off, st = codec.compress_batch(b)
    assert (st == 0).all()
    good = [blob[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(LENS))]
    bad = [b"XXXX" + good[5][4:], good[5][:90], good[5][:40]]             # bad magic, cut at 90 bytes, cut at 40
    mixed = [good[0], bad[0], good[1], good[2], bad[1], good[3], good[4], bad[2], good[5]]
    return {"mixed": Batch(codec, mixed, [2, 0, 3, 63, 0, 64, 65, 0, 129]), "bad": Batch(codec, bad, [0, 0, 0]), "empty": Batch(codec, [], [])}


BAD_STATUS = [-4, -5, -5]               # FCZ_E_BAD_MAGIC, FCZ_E_TRUNCATED
MIXED_STATUS = [0, -4, 0, 0, -5, 0, 0, -5, 0]


def starts_of(b, kind):
    """the window starts of a case: NULL, all 0, all 1, one start beyond its chain's length"""
    if kind == "null":
        return None
    s = np.full(b.n, 1 if kind == "one" else 0, np.uint32)
    if kind == "beyond" and b.n:
        s[:] = np.arange(b.n) % 3
        s[b.n - 1] = int(b.lens[b.n - 1]) + 1
    return s


# ---- the host calls, each into guarded 0xA5 arrays ---------------------------------------------------------------------------------
def host_dense(codec, b, layout, L, start="plain", want=KEYS, status=True, width=None, sizing=False, w_out=True):
    """fcz_decompress_dense (start == "plain") or _window (start: None or [n]) -> (rc, L_out or None, {name: array}, status, guarded);
    width: the L the arrays are sized for when L == 0"""
    W = L if L else (b.longest if width is None else width)
    A, n = D.WIDTH[layout], b.n
    shape = dict(pos=(n, W, A, 3), mask=(n, W, A), aatype=(n, W), plddt=(n, W), res_index=(n, W), length=(n,), status=(n,))
    g = HostGuarded({k: (np.int32 if k == "status" else DT[k], shape[k]) for k in tuple(want) + (("status",) if status else ())})
    out = CDenseOut(*(g.ptr(k) if k in want else None for k in KEYS))
    lo = ctypes.c_uint32(0xA5A5A5A5)
    tail = (ctypes.byref(lo) if w_out else None, None if sizing else ctypes.byref(out), g.ptr("status") if status else None)
    if isinstance(start, str):
        rc = codec.lib.fcz_decompress_dense(*b.head(codec), D.LAYOUTS[layout], L, *tail)
    else:
        rc = codec.lib.fcz_decompress_dense_window(*b.head(codec), D.LAYOUTS[layout], L, None if start is None else start.ctypes.data, *tail)
    return rc, (lo.value if w_out else None), g


def host_packed(codec, b, layout, want=PACKED_KEYS, status=True, sizing=False, R_out=True, row_off=True, rows=None):
    rows = b.R if rows is None else rows
    A, n = D.WIDTH[layout], b.n
    shape = dict(pos=(rows, A, 3), mask=(rows, A), aatype=(rows,), plddt=(rows,), res_index=(rows,), chain_index=(rows,), length=(n,),
                 status=(n,), row_off=(n + 1,))
    names = tuple(want) + (("status",) if status else ()) + (("row_off",) if row_off else ())
    g = HostGuarded({k: (np.int32 if k == "status" else np.uint32 if k == "row_off" else DT[k], shape[k]) for k in names})
    out = CPackedOut(*(g.ptr(k) if k in want else None for k in PACKED_KEYS))
    ro = ctypes.c_uint32(0xA5A5A5A5)
    rc = codec.lib.fcz_decompress_dense_packed(*b.head(codec), D.LAYOUTS[layout], ctypes.byref(ro) if R_out else None,
                                               g.ptr("row_off") if row_off else None, None if sizing else ctypes.byref(out),
                                               g.ptr("status") if status else None)
    return rc, (ro.value if R_out else None), g


def host_angles(codec, b, form, L=0, start=None, aatype=True, status=True, sizing=False, w_out=True, row_off=True, width=None, only=None):
    """form: "padded", "window", "packed" -> (rc, width or None, guarded); only: "angles" / "mask" = the other one is NULL"""
    n = b.n
    W = L if L else (b.longest if width is None else width)
    rows = (b.R if width is None else width) if form == "packed" else n * W
    spec = {"angles": (np.float32, (rows, COLS)), "mask": (np.uint8, (rows, COLS))}
    if form == "window" and aatype:
        spec["aatype"] = (np.uint8, (rows,))
    if status:
        spec["status"] = (np.int32, (n,))
    if form == "packed" and row_off:
        spec["row_off"] = (np.uint32, (n + 1,))
    g = HostGuarded(spec)
    wo = ctypes.c_uint32(0xA5A5A5A5)
    ap = None if sizing or only == "mask" else g.ptr("angles")
    mp = None if sizing or only == "angles" else g.ptr("mask")
    sp, wp = (g.ptr("status") if status else None), (ctypes.byref(wo) if w_out else None)
    if form == "padded":
        rc = codec.lib.fcz_decompress_angles(*b.head(codec), L, wp, ap, mp, sp)
    elif form == "window":
        rc = codec.lib.fcz_decompress_angles_window(*b.head(codec), L, None if start is None else start.ctypes.data, wp, ap, mp,
                                                    g.ptr("aatype") if aatype and not sizing else None, sp)
    else:
        rc = codec.lib.fcz_decompress_angles_packed(*b.head(codec), wp, g.ptr("row_off") if row_off else None, ap, mp, sp)
    return rc, (wo.value if w_out else None), g


def dev_angles(codec, b, form, L=0, start=None):
    """fcz_angles_dev / _window_dev / _packed_dev over the batch's device records -> {angles, mask[, aatype]} on the host"""
    import torch
    rec, n = b.dev.rec, b.n
    rows = b.R if form == "packed" else n * L
    t = {k: torch.full((max(rows * COLS * s, 1),), FILL, dtype=torch.uint8, device="cuda:0") for k, s in (("angles", 4), ("mask", 1))}
    if form == "window":
        t["aatype"] = torch.full((max(rows, 1),), FILL, dtype=torch.uint8, device="cuda:0")
    st = None if start is None else to_dev(np.asarray(start, np.uint32))
    head = (codec.ctx, rec.blob_t.data_ptr(), rec.off_t.data_ptr(), n, rec.res_off_t.data_ptr())
    torch.cuda.synchronize()
    if form == "padded":
        rc = codec.lib.fcz_angles_dev(*head, L, t["angles"].data_ptr(), t["mask"].data_ptr())
    elif form == "window":
        rc = codec.lib.fcz_angles_window_dev(*head, L, None if st is None else st.data_ptr(), t["angles"].data_ptr(), t["mask"].data_ptr(), t["aatype"].data_ptr())
    else:
        rc = codec.lib.fcz_angles_packed_dev(*head, t["angles"].data_ptr(), t["mask"].data_ptr())
    _lib.check(rc, "fcz_angles*_dev")
    codec.synchronize()
    size = dict(angles=rows * COLS * 4, mask=rows * COLS, aatype=rows)
    return {k: v.cpu().numpy()[:size[k]] for k, v in t.items()}


_DENSE_REF = {}


def dev_dense(b, layout, L, start="plain"):
    """fcz_dense_dev / fcz_dense_window_dev over the batch's device records, computed once per case"""
    key = (id(b), layout, L, "plain" if isinstance(start, str) else None if start is None else start.tobytes())
    if key not in _DENSE_REF:
        _DENSE_REF[key] = b.dev.dense(layout, L) if isinstance(start, str) else b.dev.dense(layout, L, start)
    return _DENSE_REF[key]


def fetched(g, names):
    return {k: g.fetch(k) for k in names}


# ---- padded and windowed dense ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(D.LAYOUTS))
def test_dense_and_window_host_forms_are_the_device_forms(codec, batches, layout):
    b = batches["mixed"]
    for L in WIDTHS:
        W = L or b.longest
        for kind in ("plain", "null", "zero", "one", "beyond"):
            start = "plain" if kind == "plain" else starts_of(b, kind)
            ref = dev_dense(b, layout, W, start)
            rc, w, g = host_dense(codec, b, layout, L, start)
            assert rc == 0 and w == W, (layout, L, kind, rc, w)
            same_bytes(fetched(g, KEYS), ref, (layout, L, kind))
            assert list(g.fetch("status")) == MIXED_STATUS
            # every optional output left NULL, the width and the status too (L == 0 needs the width: the arrays are the caller's)
            rc, w, g = host_dense(codec, b, layout, W, start, want=("pos", "mask"), status=False, w_out=False)
            assert rc == 0
            same_bytes(fetched(g, ("pos", "mask")), {k: ref[k] for k in ("pos", "mask")}, (layout, L, kind, "bare"))
    # each optional output left NULL on its own
    start = starts_of(b, "beyond")
    ref = dev_dense(b, layout, 65, start)
    for leave in OPTIONAL:
        want = tuple(k for k in KEYS if k != leave)
        rc, w, g = host_dense(codec, b, layout, 65, start, want=want)
        assert rc == 0 and w == 65
        same_bytes(fetched(g, want), {k: ref[k] for k in want}, (layout, "without", leave))


@pytest.mark.parametrize("layout", list(D.LAYOUTS))
def test_dense_of_records_none_of_which_decodes(codec, batches, layout):
    b = batches["bad"]
    assert b.R == 0 and b.M == 0
    # L > 0: no decode, but the dense kernel runs and every row is written as padding -- what the device form writes
    for L in (1, 64, 65, 200):
        for start in ("plain", None, starts_of(b, "one")):
            rc, w, g = host_dense(codec, b, layout, L, start)
            assert rc == 0 and w == L
            got = fetched(g, KEYS)
            same_bytes(got, dev_dense(b, layout, L, start), (layout, L))
            assert not got["pos"].view(np.uint32).any() and not got["mask"].any() and (got["aatype"] == 20).all() and not got["length"].any()
            assert list(g.fetch("status")) == BAD_STATUS
    # L == 0: the width is 0, length is zeroed on the host and nothing else is written
    for start in ("plain", None):
        rc, w, g = host_dense(codec, b, layout, 0, start, width=3)
        assert rc == 0 and w == 0
        assert list(g.fetch("length")) == [0, 0, 0] and list(g.fetch("status")) == BAD_STATUS
        for k in ("pos", "mask", "aatype", "plddt", "res_index"):
            assert (g.raw[k] == FILL).all(), k
        rc, w, g = host_dense(codec, b, layout, 0, start, want=("pos", "mask"), status=False, width=3)
        assert rc == 0 and w == 0 and g.untouched()


def test_dense_empty_batch_sizing_call_and_refusals(codec, batches):
    mixed, empty = batches["mixed"], batches["empty"]
    for start in ("plain", None):
        # n == 0: OK, *L_out = L as given, nothing else written
        for L in (0, 7):
            rc, w, g = host_dense(codec, empty, "atom37", L, start, width=2)
            assert rc == 0 and w == L and g.untouched()
        # a sizing call delivers the width and the status and writes no array
        for L, W in ((0, 129), (64, 64)):
            rc, w, g = host_dense(codec, mixed, "atom14", L, start, sizing=True)
            assert rc == 0 and w == W and list(g.fetch("status")) == MIXED_STATUS
            assert all((g.raw[k] == FILL).all() for k in KEYS)
        # refusals: neither out nor L_out; out without pos or without mask; an unknown layout
        rc, w, g = host_dense(codec, mixed, "atom37", 64, start, sizing=True, w_out=False)
        assert rc == INVALID and g.untouched()
        for want in (("mask", "aatype"), ("pos", "length"), OPTIONAL):
            rc, w, g = host_dense(codec, mixed, "atom37", 64, start, want=want)
            assert rc == INVALID and w == 0xA5A5A5A5 and g.untouched()
    lo = ctypes.c_uint32(0)
    assert codec.lib.fcz_decompress_dense(*mixed.head(codec), 3, 64, ctypes.byref(lo), None, None) == INVALID
    assert codec.lib.fcz_decompress_dense_packed(*mixed.head(codec), 3, ctypes.byref(lo), None, None, None) == INVALID


# ---- packed dense ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(D.LAYOUTS))
def test_packed_host_form_is_the_padded_one_without_padding(codec, batches, layout):
    b = batches["mixed"]
    rc, w, gp = host_dense(codec, b, layout, 0)
    assert rc == 0 and w == 129
    pad = fetched(gp, KEYS)
    rc, R, g = host_packed(codec, b, layout)
    assert rc == 0 and R == b.R == sum(LENS)
    got = fetched(g, PACKED_KEYS)
    assert np.array_equal(g.fetch("row_off"), b.res_off) and list(g.fetch("status")) == MIXED_STATUS
    assert np.array_equal(got["length"], pad["length"]) and np.array_equal(got["length"], b.lens)
    assert np.array_equal(got["chain_index"], np.repeat(np.arange(b.n), b.lens))
    for e in range(b.n):
        r0, m = int(b.res_off[e]), int(b.lens[e])
        for k in ("pos", "mask", "aatype", "plddt", "res_index"):
            assert np.array_equal(raw(got[k][r0:r0 + m]), raw(pad[k][e, :m])), (layout, e, k)
    # every optional output left NULL, then each on its own
    for want in [("pos", "mask")] + [tuple(k for k in PACKED_KEYS if k != leave) for leave in OPTIONAL + ("chain_index",)]:
        rc, R, g2 = host_packed(codec, b, layout, want=want, status=len(want) > 2, row_off=len(want) > 2, R_out=len(want) > 2)
        assert rc == 0
        same_bytes(fetched(g2, want), {k: got[k] for k in want}, (layout, want))


def test_packed_dense_corners(codec, batches):
    mixed, bad, empty = batches["mixed"], batches["bad"], batches["empty"]
    # n == 0: *R_out = 0, row_off[0] = 0, nothing else
    rc, R, g = host_packed(codec, empty, "atom37", rows=2)
    assert rc == 0 and R == 0 and list(g.fetch("row_off")) == [0]
    assert all((g.raw[k] == FILL).all() for k in PACKED_KEYS)
    # a sizing call: R, row_off, status
    rc, R, g = host_packed(codec, mixed, "atom14", sizing=True)
    assert rc == 0 and R == mixed.R and np.array_equal(g.fetch("row_off"), mixed.res_off) and list(g.fetch("status")) == MIXED_STATUS
    assert all((g.raw[k] == FILL).all() for k in PACKED_KEYS)
    # no record decodes: length zeroed on the host, nothing else written
    rc, R, g = host_packed(codec, bad, "atom37", rows=2)
    assert rc == 0 and R == 0 and list(g.fetch("row_off")) == [0, 0, 0, 0] and list(g.fetch("status")) == BAD_STATUS
    assert list(g.fetch("length")) == [0, 0, 0]
    assert all((g.raw[k] == FILL).all() for k in PACKED_KEYS if k != "length")
    rc, R, g = host_packed(codec, bad, "atom37", want=("pos", "mask"), status=False, row_off=False, rows=2)
    assert rc == 0 and R == 0 and g.untouched()
    # refusals
    rc, R, g = host_packed(codec, mixed, "atom37", sizing=True, R_out=False)
    assert rc == INVALID and g.untouched()
    for want in (("mask", "aatype"), ("pos", "chain_index")):
        rc, R, g = host_packed(codec, mixed, "atom37", want=want)
        assert rc == INVALID and R == 0xA5A5A5A5 and g.untouched()


# ---- angles ------------------------------------------------------------------------------------------------------------------------
def test_angles_host_forms_are_the_device_forms(codec, batches):
    b = batches["mixed"]
    for L in WIDTHS:
        W = L or b.longest
        ref = dev_angles(codec, b, "padded", W)
        rc, w, g = host_angles(codec, b, "padded", L)
        assert rc == 0 and w == W and list(g.fetch("status")) == MIXED_STATUS
        same_bytes(fetched(g, ("angles", "mask")), ref, ("padded", L))
        rc, w, g = host_angles(codec, b, "padded", W, status=False, w_out=False)
        assert rc == 0
        same_bytes(fetched(g, ("angles", "mask")), ref, ("padded", L, "bare"))
        for kind in ("null", "zero", "one", "beyond"):
            start = starts_of(b, kind)
            ref = dev_angles(codec, b, "window", W, start)
            rc, w, g = host_angles(codec, b, "window", L, start)
            assert rc == 0 and w == W and list(g.fetch("status")) == MIXED_STATUS
            same_bytes(fetched(g, ("angles", "mask", "aatype")), ref, ("window", L, kind))
            rc, w, g = host_angles(codec, b, "window", W, start, aatype=False, status=False, w_out=False)
            assert rc == 0
            same_bytes(fetched(g, ("angles", "mask")), {k: ref[k] for k in ("angles", "mask")}, ("window", L, kind, "bare"))
    ref = dev_angles(codec, b, "packed")
    rc, w, g = host_angles(codec, b, "packed")
    assert rc == 0 and w == b.R and np.array_equal(g.fetch("row_off"), b.res_off) and list(g.fetch("status")) == MIXED_STATUS
    same_bytes(fetched(g, ("angles", "mask")), ref, "packed")
    rc, w, g = host_angles(codec, b, "packed", status=False, row_off=False, w_out=False)
    assert rc == 0
    same_bytes(fetched(g, ("angles", "mask")), ref, "packed bare")


def test_angles_corners(codec, batches):
    mixed, bad, empty = batches["mixed"], batches["bad"], batches["empty"]
    for form in ("padded", "window", "packed"):
        packed = form == "packed"
        # n == 0: the width is 0 (packed) or L as given, row_off[0] = 0, nothing else
        for L in ((0,) if packed else (0, 7)):
            rc, w, g = host_angles(codec, empty, form, L, width=2)
            assert rc == 0 and w == L
            if packed:
                assert list(g.fetch("row_off")) == [0]
            assert all((g.raw[k] == FILL).all() for k in g.raw if k != "row_off")
        # a sizing call: the width, row_off and status
        for L, W in (((0, mixed.R),) if packed else ((0, 129), (64, 64))):
            rc, w, g = host_angles(codec, mixed, form, L, sizing=True)
            assert rc == 0 and w == W and list(g.fetch("status")) == MIXED_STATUS
            if packed:
                assert np.array_equal(g.fetch("row_off"), mixed.res_off)
            assert all((g.raw[k] == FILL).all() for k in ("angles", "mask", "aatype") if k in g.raw)
        # no row: returns after the width, row_off and status
        rc, w, g = host_angles(codec, bad, form, 0, width=2)
        assert rc == 0 and w == 0 and list(g.fetch("status")) == BAD_STATUS
        if packed:
            assert list(g.fetch("row_off")) == [0, 0, 0, 0]
        assert all((g.raw[k] == FILL).all() for k in ("angles", "mask", "aatype") if k in g.raw)
        # refusals: exactly one of angles / mask; a sizing call without the width
        for only in ("angles", "mask"):
            rc, w, g = host_angles(codec, mixed, form, 0 if packed else 64, only=only)
            assert rc == INVALID and w == 0xA5A5A5A5 and g.untouched()
        rc, w, g = host_angles(codec, mixed, form, 0 if packed else 64, sizing=True, w_out=False)
        assert rc == INVALID and g.untouched()
    # records none of which decodes at a width of the caller's: every row is written, as the device forms write it
    for form, start in (("padded", None), ("window", None), ("window", starts_of(bad, "one"))):
        rc, w, g = host_angles(codec, bad, form, 65, start)
        assert rc == 0 and w == 65
        same_bytes(fetched(g, [k for k in ("angles", "mask", "aatype") if k in g.raw]), dev_angles(codec, bad, form, 65, start), (form, "bad"))


# ---- fcz_decompress_batch -----------------------------------------------------------------------------------------------------------
ATOM_KEYS = ("x", "y", "z", "bfac_res", "res_code", "atom_code")


def host_batch(codec, b, want=ATOM_KEYS, alt=False, rows=None):
    R, M = (b.R, b.M) if rows is None else (rows, rows)
    dt = dict(x=np.float32, y=np.float32, z=np.float32, bfac_res=np.float32, res_code=np.uint8, atom_code=np.uint8)
    g = HostGuarded({k: (dt[k], (R if k in ("bfac_res", "res_code") else M,)) for k in want})
    out = CAtomsOut(*(g.ptr(k) if k in want else None for k in ATOM_KEYS))
    rc = codec.lib.fcz_decompress_batch(*b.head(codec), b.res_off.ctypes.data, b.atom_off.ctypes.data, int(alt), ctypes.byref(out))
    return rc, g


def test_batch_host_form_is_the_device_form(codec, batches):
    b = batches["mixed"]
    for alt in (False, True):
        b.dev.rec.sizes(codec)
        ref = b.dev.rec.batch(codec, alt_order=alt)
        for want in (ATOM_KEYS, ATOM_KEYS[:5], ATOM_KEYS[:4] + ATOM_KEYS[5:], ATOM_KEYS[:4]):
            rc, g = host_batch(codec, b, want, alt)
            assert rc == 0
            same_bytes(fetched(g, want), {k: ref[k] for k in want}, (alt, want))
    # no atom and no residue: nothing is copied
    for key in ("bad", "empty"):
        rc, g = host_batch(codec, batches[key], rows=2)
        assert rc == 0 and g.untouched(), key


# ---- PDB text ----------------------------------------------------------------------------------------------------------------------
def dev_pdb(codec, b, alt):
    """fcz_pdb_sizes_dev + fcz_pdb_format_dev over the batch's device records -> (text_off, text)"""
    import torch
    rec = b.dev.rec
    rec.sizes(codec)
    atoms = rec.batch(codec, alt_order=alt, host=False)
    at = CAtomsOut(*(atoms[k].data_ptr() for k in ("x", "y", "z", "bfac_res", "res_code")), None)
    head = (codec.ctx, rec.blob_t.data_ptr(), rec.off_t.data_ptr(), b.n, rec.res_off_t.data_ptr(), rec.atom_off_t.data_ptr(), ctypes.byref(at))
    toff = torch.zeros(b.n + 1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    _lib.check(codec.lib.fcz_pdb_sizes_dev(*head, toff.data_ptr()), "fcz_pdb_sizes_dev")
    codec.synchronize()
    off = toff.cpu().numpy().view(np.uint64)
    text = torch.full((max(int(off[-1]), 1),), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    _lib.check(codec.lib.fcz_pdb_format_dev(*head, int(alt), toff.data_ptr(), text.data_ptr()), "fcz_pdb_format_dev")
    codec.synchronize()
    return off, text.cpu().numpy()[:int(off[-1])].tobytes()


def host_pdb(codec, b, flags, status=True, sizes_only=False):
    g = HostGuarded({"text_off": (np.uint64, (b.n + 1,)), **({"status": (np.int32, (b.n,))} if status else {})})
    fn = codec.lib.fcz_decompress_pdb_sizes if sizes_only else codec.lib.fcz_decompress_pdb_begin
    rc = fn(*b.head(codec), flags, g.ptr("text_off"), g.ptr("status") if status else None)
    return rc, g


def test_pdb_host_form_is_the_device_form(codec, batches):
    b = batches["mixed"]
    for alt in (0, 1):
        off, text = dev_pdb(codec, b, alt)
        texts = [text[int(off[i]):int(off[i + 1])] for i in range(b.n)]
        assert all(bool(t) == (m == 0) for t, m in zip(texts, MIXED_STATUS))
        for nul in (0, NUL):
            want = [t + b"\0" if nul and t else t for t in texts]          # every entry that decodes is followed by one NUL
            want_off = np.concatenate([[0], np.cumsum([len(t) for t in want])]).astype(np.uint64)
            for status in (True, False):
                rc, g = host_pdb(codec, b, alt | nul, status)
                assert rc == 0 and np.array_equal(g.fetch("text_off"), want_off)
                assert not status or list(g.fetch("status")) == MIXED_STATUS
                t = HostGuarded({"text": (np.uint8, (int(want_off[-1]),))})
                assert codec.lib.fcz_decompress_pdb_fetch(codec.ctx, t.ptr("text")) == 0
                assert t.fetch("text").tobytes() == b"".join(want), (alt, nul)
            # the sizes form gives the same offsets and keeps no text: its fetch copies nothing
            rc, g = host_pdb(codec, b, alt | nul, sizes_only=True)
            assert rc == 0 and np.array_equal(g.fetch("text_off"), want_off) and list(g.fetch("status")) == MIXED_STATUS
            t = HostGuarded({"text": (np.uint8, (16,))})
            assert codec.lib.fcz_decompress_pdb_fetch(codec.ctx, t.ptr("text")) == 0 and t.untouched()
            assert codec.lib.fcz_decompress_pdb_fetch(codec.ctx, None) == 0


def test_pdb_corners(codec, batches):
    for key, offs, st in (("empty", [0], []), ("bad", [0, 0, 0, 0], BAD_STATUS)):
        b = batches[key]
        for nul in (0, NUL):
            rc, g = host_pdb(codec, batches["mixed"], 0)                   # a text is resident: the next begin must end that
            assert rc == 0
            rc, g = host_pdb(codec, b, nul)
            assert rc == 0 and list(g.fetch("text_off")) == offs
            assert list(g.fetch("status")) == st if st else (g.raw["status"] == FILL).all()
            t = HostGuarded({"text": (np.uint8, (16,))})
            assert codec.lib.fcz_decompress_pdb_fetch(codec.ctx, None) == 0             # pdb_bytes == 0
            assert codec.lib.fcz_decompress_pdb_fetch(codec.ctx, t.ptr("text")) == 0 and t.untouched()
    rc = codec.lib.fcz_decompress_pdb_begin(*batches["mixed"].head(codec), 0, None, None)
    assert rc == INVALID


# ---- extract -----------------------------------------------------------------------------------------------------------------------
def test_extract_host_form_is_the_device_form(codec, batches):
    import torch
    for key in ("mixed", "bad", "empty"):
        b = batches[key]
        rec = b.dev.rec
        for mode, digits in ((0, 1), (0, 4), (1, 2)):
            doff_t = torch.zeros(b.n + 1, dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            _lib.check(codec.lib.fcz_extract_sizes_dev(codec.ctx, rec.blob_t.data_ptr(), rec.off_t.data_ptr(), b.n, mode, digits, doff_t.data_ptr()), "fcz_extract_sizes_dev")
            codec.synchronize()
            doff = doff_t.cpu().numpy().view(np.uint64)
            data_t = torch.full((max(int(doff[-1]), 1),), FILL, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            _lib.check(codec.lib.fcz_extract_dev(codec.ctx, rec.blob_t.data_ptr(), rec.off_t.data_ptr(), b.n, mode, digits, doff_t.data_ptr(), data_t.data_ptr()), "fcz_extract_dev")
            codec.synchronize()
            hoff = np.zeros(b.n + 1, np.uint64)
            assert codec.lib.fcz_extract_sizes(b.blob.ctypes.data, b.off.ctypes.data, b.n, mode, digits, hoff.ctypes.data) == 0
            assert np.array_equal(hoff, doff), (key, mode, digits)
            g = HostGuarded({"data": (np.uint8, (int(hoff[-1]),))})
            rc = codec.lib.fcz_extract(*b.head(codec), mode, digits, hoff.ctypes.data, g.ptr("data") if hoff[-1] else None)
            assert rc == 0 and g.fetch("data").tobytes() == data_t.cpu().numpy()[:int(doff[-1])].tobytes(), (key, mode, digits)
            if key == "mixed":
                assert int(hoff[-1]) > 0
                assert codec.lib.fcz_extract(*b.head(codec), mode, digits, hoff.ctypes.data, None) == INVALID
    assert codec.lib.fcz_extract(*batches["mixed"].head(codec), 0, 5, hoff.ctypes.data, None) == INVALID


def batch_step(codec, b):
    rc, g = host_batch(codec, b)
    return rc, None, g


# ---- one ctx, alternating forms -------------------------------------------------------------------------------------------------
def test_alternating_forms_on_one_ctx_give_what_a_fresh_ctx_gives(batches):
    from foldcomp_amd.codec import Codec
    b = batches["mixed"]
    start = starts_of(b, "beyond")
    steps = [("packed dense", lambda c: host_packed(c, b, "atom37")),
             ("padded angles", lambda c: host_angles(c, b, "padded", 0)),
             ("windowed dense", lambda c: host_dense(c, b, "atom14", 65, start)),
             ("batch", lambda c: batch_step(c, b)),
             ("packed angles", lambda c: host_angles(c, b, "packed")),
             ("padded dense", lambda c: host_dense(c, b, "atom37", 0))]
    one = Codec(0)
    try:
        got = [run(one) for _, run in steps]
    finally:
        one.close()
    for (name, run), (rc, w, g) in zip(steps, got):
        fresh = Codec(0)
        try:
            frc, fw, fg = run(fresh)
        finally:
            fresh.close()
        assert (rc, w) == (0, fw) and frc == 0, name
        assert list(g.spec) == list(fg.spec)
        for k, a, f in zip(g.spec, g.all(), fg.all()):
            assert np.array_equal(raw(a), raw(f)), (name, k)
