"""Shared helpers of the residue-window tests: the device calls fcz_dense_dev / fcz_dense_window_dev on records decoded once, into
arrays pre-filled with 0xA5 bytes; the expectation of a window as a host slice of the uncropped arrays; the starts of the sweep."""
import ctypes

import numpy as np

import _dense as D
from _cases import entries_blob
from _devpath import FILL, DevRecords, to_dev
from foldcomp_amd import _lib
from foldcomp_amd.structure import CAtomsOut, CDenseOut

KEYS = ("pos", "mask", "aatype", "plddt", "res_index", "length")
PAD = dict(pos=0, mask=0, aatype=20, plddt=0, res_index=0)
NO_START = object()                            # fcz_dense_dev itself, not the windowed call


def raw_bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint8) if a.dtype == np.bool_ else a


def same(got, exp, what=""):
    for k in KEYS:
        if k not in exp:
            continue
        g, e = raw_bits(got[k]), raw_bits(exp[k])
        assert g.shape == e.shape, (what, k, g.shape, e.shape)
        assert np.array_equal(g.astype(np.int64), e.astype(np.int64)), (what, k, np.argwhere(g.astype(np.int64) != e.astype(np.int64))[:4])


class Decoded:
    """records sized and decoded on the device once; dense(...) runs fcz_dense_dev or fcz_dense_window_dev over them"""

    def __init__(self, codec, entries, alt_order=False):
        self.codec, self.n, self.alt = codec, len(entries), alt_order
        self.rec = DevRecords(*entries_blob(entries))
        self.rec.sizes(codec)
        self.atoms = self.rec.batch(codec, alt_order=alt_order, host=False)

    def dense(self, layout, L, start=NO_START, want=KEYS):
        """start: NO_START = fcz_dense_dev; None = fcz_dense_window_dev with start_dev NULL; else the starts [n]"""
        import torch
        codec, rec, n, A = self.codec, self.rec, self.n, D.WIDTH[layout]
        shape = dict(pos=(n, L, A, 3), mask=(n, L, A), aatype=(n, L), plddt=(n, L), res_index=(n, L), length=(n,))
        dt = dict(pos=np.float32, mask=np.uint8, aatype=np.uint8, plddt=np.float32, res_index=np.int32, length=np.uint32)
        nbytes = {k: int(np.prod(shape[k])) * np.dtype(dt[k]).itemsize for k in want}
        raw = {k: torch.full((max(nbytes[k], 1),), FILL, dtype=torch.uint8, device="cuda:0") for k in want}
        at = CAtomsOut(*(self.atoms[k].data_ptr() for k in ("x", "y", "z", "bfac_res", "res_code")), None)
        out = CDenseOut(*(raw[k].data_ptr() if k in raw else None for k in KEYS))
        head = (codec.ctx, rec.blob_t.data_ptr(), rec.off_t.data_ptr(), n, rec.res_off_t.data_ptr(), rec.atom_off_t.data_ptr(), ctypes.byref(at),
                int(self.alt), D.LAYOUTS[layout], L)
        st = None if start is NO_START or start is None else to_dev(np.asarray(start, np.uint32))
        torch.cuda.synchronize()
        if start is NO_START:
            _lib.check(codec.lib.fcz_dense_dev(*head, ctypes.byref(out)), "fcz_dense_dev")
        else:
            _lib.check(codec.lib.fcz_dense_window_dev(*head, None if st is None else st.data_ptr(), ctypes.byref(out)), "fcz_dense_window_dev")
        codec.synchronize()
        return {k: raw[k].cpu().numpy()[:nbytes[k]].view(dt[k]).reshape(shape[k]) for k in want}


def window_of(full, starts, L):
    """the expectation: rows start[e] .. start[e] + L - 1 of the uncropped arrays, padding rows behind their end"""
    n, Lf = full["aatype"].shape
    out = {}
    for k, pad in PAD.items():
        if k not in full:
            continue
        a = full[k]
        o = np.full((n, L) + a.shape[2:], pad, a.dtype)
        for e, s in enumerate(starts):
            s = int(s)
            if s < Lf:
                m = min(L, Lf - s)
                o[e, :m] = a[e, s:s + m]
        out[k] = o
    if "length" in full:
        out["length"] = full["length"]
    return out


def sweep_starts(lens, L, shift):
    """per entry one of 0, 1, 63, 64, 65, len-L, len-L+1, len-1, len, len+1, 0xFFFFFFFF (negatives clamped to 0), cycling"""
    out = []
    for i, n in enumerate(int(x) for x in lens):
        kinds = [0, 1, 63, 64, 65, n - L, n - L + 1, n - 1, n, n + 1, 0xFFFFFFFF]
        out.append(max(kinds[(i + shift) % len(kinds)], 0))
    return np.asarray(out, np.uint32)
