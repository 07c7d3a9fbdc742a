"""Batch codec object over the C-ABI: the host-side mirror of the reference's `Foldcomp` class
(src/foldcomp.h:267-402) for many chains at once.

    Foldcomp::compress + writeStream   ->  Codec.compress_batch(ChainBatch)   -> FCZ blob + offsets
    Foldcomp::read + decompress        ->  Codec.decompress_batch(blob, off)  -> SoA atoms

Host numpy arrays in, host numpy arrays out (copies ride the ctx stream). The device-resident entry
points used by bench.py take raw device pointers (e.g. torch tensors' .data_ptr()).
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import numpy as np

from . import _lib
from .structure import CAtomsOut, CChainBatch, CDenseIn, CDenseOut, CEntryInfo, ChainBatch, CPackedOut, CGdtOut, CSuperposeOut, CTmScoreOut, batch_as_c


# the columns of the angle tensors (FCZ_ANGLE_COLUMNS, include/fcz_hip.h), degrees
ANGLE_COLUMNS = ("phi", "psi", "omega", "n_ca_c", "ca_c_n", "c_n_ca", "chi1", "chi2", "chi3", "chi4")
DENSE_LAYOUTS = {"atom37": 0, "atom14": 1, "backbone4": 2}     # enum fcz_dense_layout
WIDTH_LAYOUTS = {37: 0, 14: 1, 4: 2}                           # slots per residue A -> enum fcz_dense_layout


def dense_layout(layout) -> int:
    """layout name (or enum value) -> enum fcz_dense_layout"""
    if layout in DENSE_LAYOUTS:
        return DENSE_LAYOUTS[layout]
    if isinstance(layout, int) and layout in DENSE_LAYOUTS.values():
        return layout
    raise ValueError(f"unknown dense layout {layout!r}: one of {', '.join(DENSE_LAYOUTS)}")


class _Arrays(NamedTuple):
    """checked dense arrays on the host, what every analysis call reads: pos contiguous float32 [.., A, 3] with lead = its shape without
    (A, 3), mask bool / uint8 or None, aatype uint8 or None, `lay` the enum fcz_dense_layout of A; n chains of `rows` rows each (padded:
    bound = length as uint32 or None) or over `rows` rows in all (packed: bound = row_off as uint32)"""
    pos: np.ndarray
    mask: Optional[np.ndarray]
    aatype: Optional[np.ndarray]
    lay: int
    lead: tuple
    A: int
    packed: bool
    n: int
    rows: int
    bound: Optional[np.ndarray]

    def as_dict(self, row_off):
        """the arrays as the dict the device-free checks of foldcomp_amd.api read"""
        d = dict(pos=self.pos, mask=self.mask, aatype=self.aatype)
        if self.packed:
            d["cu_seqlens"] = row_off
        return d


def _pos_error(name, packed, shape):
    return ValueError(f"{name} must be float32 {'[R, A, 3]' if packed else '[n, L, A, 3]'} with A = 37, 14 or 4, not {shape}")


def _mask_array(mask, shape, name="mask"):
    mask = np.ascontiguousarray(mask)
    if mask.shape != shape or mask.dtype not in (np.bool_, np.uint8):
        raise ValueError(f"{name} must be bool / uint8 {shape}, not {mask.dtype} {mask.shape}")
    return mask


def _addr(a):
    return None if a is None else a.ctypes.data


def _dense_arrays(pos, mask, aatype, length, row_off, *, name="pos", mask_name="mask", mask_optional=False,
                  limit=(2 ** 31 - 1, "at most 2^31 - 1 rows per chain")):
    """the one prelude of the analyses on dense host arrays -> _Arrays: pos [n, L, A, 3] beside length [n] or None, or [R, A, 3] beside
    row_off [n + 1] (which makes the form packed), A = 37, 14 or 4; mask of pos's shape without its last axis (None passes only with
    mask_optional); aatype, when given, uint8 without the last two. limit = (rows, message): the most rows the caller's counters hold,
    or None"""
    pos = np.ascontiguousarray(pos, np.float32)
    packed = row_off is not None
    if pos.ndim != (3 if packed else 4) or pos.shape[-1] != 3 or pos.shape[-2] not in WIDTH_LAYOUTS:
        raise _pos_error(name, packed, pos.shape)
    lead, A = pos.shape[:-2], pos.shape[-2]
    if mask is not None or not mask_optional:
        mask = _mask_array(mask, pos.shape[:-1], mask_name)
    if aatype is not None:
        aatype = np.ascontiguousarray(aatype)
        if aatype.shape != lead or aatype.dtype != np.uint8:
            raise ValueError(f"aatype must be uint8 {lead}, not {aatype.dtype} {aatype.shape}")
    if packed:
        bound = np.ascontiguousarray(row_off, np.uint32)
        if bound.ndim != 1 or len(bound) < 1:
            raise ValueError("row_off must be [n + 1]")
        n, rows = len(bound) - 1, pos.shape[0]
    else:
        n, rows, bound = pos.shape[0], pos.shape[1], None
        if length is not None:
            bound = np.ascontiguousarray(length, np.uint32)
            if bound.shape != (n,):
                raise ValueError(f"length must be [{n}], not {bound.shape}")
    if limit is not None and rows > limit[0]:
        raise ValueError(limit[1])
    return _Arrays(pos, mask, aatype, WIDTH_LAYOUTS[A], lead, A, packed, n, rows, bound)


def _pair_arrays(pos_true, mask_true, pos_pred, mask_pred, aatype, length, row_off, slot=None, **rules):
    """the one prelude of the analyses of a prediction against its truth -> (_Arrays of true, pos_pred contiguous float32 of its shape,
    mask_pred of its mask's shape or None, slot): mask_true is needed, slot (when the analysis has one) lies in 0 .. A - 1"""
    a = _dense_arrays(pos_true, mask_true, aatype, length, row_off, name="pos_true", mask_name="mask_true", mask_optional=True, **rules)
    pos_pred = np.ascontiguousarray(pos_pred, np.float32)
    if pos_pred.shape != a.pos.shape:
        raise ValueError(f"pos_pred must have the shape of pos_true, {a.pos.shape}, not {pos_pred.shape}")
    if mask_pred is not None:
        mask_pred = _mask_array(mask_pred, a.pos.shape[:-1], "mask_pred")
    if a.mask is None:
        raise ValueError("mask_true is needed")
    if slot is not None:
        slot = int(slot)
        if not 0 <= slot < a.A:
            raise ValueError(f"slot must be 0 .. {a.A - 1}")
    return a, pos_pred, mask_pred, slot


def _tm_align_inputs(pos_a, mask_a, pos_b, mask_b, pairs, slot, length_a, row_off_a, length_b, row_off_b, fragments, refine, dp_rounds, gaps,
                     iterations, levels, transform):
    """the prelude of Codec.tm_align and Codec.tm_align_dp -> (CChainSet a, CChainSet b, pairs int32 [m, 2], wa, wb, the layout, api.check_tm_align's
    tuple (the slot first), the arrays the two structs point into: the caller keeps them until its call returns)"""
    from . import api
    from .structure import CChainSet
    xa = _dense_arrays(pos_a, mask_a, None, length_a, row_off_a, name="pos_a", mask_name="mask_a")
    same = pos_b is None
    xb = xa if same else _dense_arrays(pos_b, mask_b, None, length_b, row_off_b, name="pos_b", mask_name="mask_b")
    pairs = api.tm_align_pairs(xa.n, xb.n, same) if pairs is None else np.ascontiguousarray(pairs, np.int32)
    width = lambda x: int(np.diff(x.bound.astype(np.int64)).clip(min=0).max(initial=1)) if x.packed else x.rows
    wa, wb = max(min(width(xa), max(xa.rows, 1)), 1), max(min(width(xb), max(xb.rows, 1)), 1)
    shapes = None if transform is None else (np.shape(transform[0]), np.shape(transform[1]))
    par = api.check_tm_align(int(slot), xa.pos.shape, xb.pos.shape, wa, wb, pairs.shape, fragments, refine, dp_rounds, gaps, iterations, levels, shapes)
    sets = [CChainSet(x.pos.ctypes.data, x.mask.ctypes.data, None if x.packed else _addr(x.bound), _addr(x.bound) if x.packed else None, x.n, x.rows)
            for x in (xa, xb)]
    return sets[0], sets[1], pairs, wa, wb, xa.lay, par, (xa, xb)


class Codec:
    def __init__(self, device: int = 0):
        self.lib = _lib.load()
        h = ctypes.c_void_p()
        _lib.check(self.lib.fcz_ctx_create(int(device), ctypes.byref(h)), "fcz_ctx_create")
        self.ctx = h
        self.device = device

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.fcz_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def stream(self) -> int:
        return int(self.lib.fcz_ctx_stream(self.ctx) or 0)

    def set_numerics(self, fast: bool):
        """decompress numerics: False = bit-identical to the reference (default), True = plain float arithmetic (FCZ_NUMERICS_FAST)"""
        _lib.check(self.lib.fcz_ctx_set_numerics(self.ctx, 1 if fast else 0), "fcz_ctx_set_numerics")

    def synchronize(self):
        _lib.check(self.lib.fcz_ctx_synchronize(self.ctx), "fcz_ctx_synchronize")

    # ---- compress -------------------------------------------------------------------------------
    def compress_sizes(self, b: ChainBatch) -> np.ndarray:
        cb = batch_as_c(b)
        off = np.zeros(b.n_chains + 1, np.uint64)
        _lib.check(self.lib.fcz_compress_sizes(ctypes.byref(cb), off.ctypes.data), "fcz_compress_sizes")
        return off

    def compress_batch(self, b: ChainBatch, strict: bool = True):
        """-> (blob uint8[...], off uint64[C+1], status int32[C])"""
        off = self.compress_sizes(b)
        cb = batch_as_c(b)
        out = np.zeros(int(off[-1]), np.uint8)
        st = np.zeros(b.n_chains, np.int32)
        rc = self.lib.fcz_compress_batch(self.ctx, ctypes.byref(cb), off.ctypes.data, out.ctypes.data, st.ctypes.data)
        # rc = the worst per-chain status, or a failure of the call itself (-1 is both: a refused chain, or bad arguments --
        # the latter leaves every per-chain status at 0)
        if rc != 0 and (strict or rc in (-2, -3, -8) or (rc == -1 and not (st == -1).any())):
            _lib.check(rc, "fcz_compress_batch")
        return out, off, st

    def compress_angles(self, b: ChainBatch) -> np.ndarray:
        """-> float32 [6, R]: phi, psi, omega, n_ca_c, ca_c_n, c_n_ca before quantisation"""
        cb = batch_as_c(b)
        out = np.zeros((6, b.n_residues), np.float32)
        _lib.check(self.lib.fcz_compress_angles(self.ctx, ctypes.byref(cb), out.ctypes.data), "fcz_compress_angles")
        return out

    # ---- decompress -----------------------------------------------------------------------------
    def decompress_sizes(self, blob: np.ndarray, off: np.ndarray):
        n = len(off) - 1
        blob = np.ascontiguousarray(blob, np.uint8)
        off = np.ascontiguousarray(off, np.uint64)
        info = (CEntryInfo * max(n, 1))()
        res_off = np.zeros(n + 1, np.uint32)
        atom_off = np.zeros(n + 1, np.uint32)
        _lib.check(self.lib.fcz_decompress_sizes(blob.ctypes.data, off.ctypes.data, n, ctypes.addressof(info),
                                                 res_off.ctypes.data, atom_off.ctypes.data), "fcz_decompress_sizes")
        return info, res_off, atom_off

    def decompress_batch(self, blob: np.ndarray, off: np.ndarray, alt_order: bool = False):
        blob = np.ascontiguousarray(blob, np.uint8)
        off = np.ascontiguousarray(off, np.uint64)
        n = len(off) - 1
        info, res_off, atom_off = self.decompress_sizes(blob, off)
        M, R = int(atom_off[-1]), int(res_off[-1])
        x = np.zeros(M, np.float32); y = np.zeros(M, np.float32); z = np.zeros(M, np.float32)
        bf = np.zeros(R, np.float32); rc = np.zeros(R, np.uint8); ac = np.zeros(M, np.uint8)
        out = CAtomsOut(x.ctypes.data, y.ctypes.data, z.ctypes.data, bf.ctypes.data, rc.ctypes.data, ac.ctypes.data)
        if M:
            _lib.check(self.lib.fcz_decompress_batch(self.ctx, blob.ctypes.data, off.ctypes.data, n, res_off.ctypes.data,
                                                     atom_off.ctypes.data, int(alt_order), ctypes.byref(out)),
                       "fcz_decompress_batch")
        return dict(x=x, y=y, z=z, bfac_res=bf, res_code=rc, atom_code=ac, res_off=res_off, atom_off=atom_off, info=info)

    @staticmethod
    def _window_starts(start, n: int) -> np.ndarray:
        """per-entry first residues of a windowed call -> uint32 [n]"""
        st = np.asarray(start)
        if st.shape != (n,) or st.dtype.kind not in "iu":
            raise ValueError(f"start must be {n} integers, one per entry, not {st.dtype} {st.shape}")
        if n and (st.astype(np.int64) < 0).any() or n and (st.astype(np.uint64) > 2 ** 32 - 1).any():
            raise ValueError("start must fit unsigned 32 bits")
        return np.ascontiguousarray(st, np.uint32)

    def decompress_dense(self, blob: np.ndarray, off: np.ndarray, layout="atom37", max_len: Optional[int] = None, packed: bool = False,
                         start=None):
        """FCZ entries -> dense padded arrays on the host (fcz_decompress_dense): pos float32 [n, L, A, 3], mask bool [n, L, A],
        aatype uint8 [n, L] (20 = unknown / padding), plddt float32 [n, L], res_index int32 [n, L], length uint32 [n] (uncropped;
        0 = the entry did not decode), status int32 [n]. L = max_len, or the longest entry of the batch; longer entries are cropped.
        packed=True (fcz_decompress_dense_packed): the rows of all entries back to back, pos [R, A, 3], mask [R, A], aatype, plddt,
        res_index, chain_index int32 [R], row_off uint32 [n + 1] (the cu_seqlens), length, status; no padding and no crop, so no max_len.
        start [n] (fcz_decompress_dense_window): row l of entry e holds its residue start[e] + l, or padding when it has none; length
        stays uncropped. Not with packed=True."""
        blob = np.ascontiguousarray(blob, np.uint8)
        off = np.ascontiguousarray(off, np.uint64)
        n = len(off) - 1
        lay = dense_layout(layout)
        A = self.lib.fcz_dense_width(lay)
        if start is not None and packed:
            raise ValueError("start keeps a window of rows per entry; the packed form keeps every residue (packed=True takes no start)")
        st = None if start is None else self._window_starts(start, n)

        def padded(L, L_out, out, status):
            if st is None:
                _lib.check(self.lib.fcz_decompress_dense(self.ctx, blob.ctypes.data, off.ctypes.data, n, lay, L, L_out, out, status), "fcz_decompress_dense")
            else:
                _lib.check(self.lib.fcz_decompress_dense_window(self.ctx, blob.ctypes.data, off.ctypes.data, n, lay, L, st.ctypes.data, L_out, out, status),
                           "fcz_decompress_dense_window")
        if packed and max_len is not None:
            raise ValueError("max_len crops to a common length; the packed form keeps every residue (packed=True takes no max_len)")
        if max_len is not None and int(max_len) < 1:
            raise ValueError("max_len must be at least 1")
        if packed:
            R = ctypes.c_uint32(0)
            status = np.zeros(max(n, 1), np.int32)
            row_off = np.zeros(n + 1, np.uint32)
            if n:
                _lib.check(self.lib.fcz_decompress_dense_packed(self.ctx, blob.ctypes.data, off.ctypes.data, n, lay, ctypes.byref(R), row_off.ctypes.data,
                                                                None, status.ctypes.data), "fcz_decompress_dense_packed")
            Rv = int(R.value)
            d = dict(pos=np.zeros((Rv, A, 3), np.float32), mask=np.zeros((Rv, A), np.uint8), aatype=np.zeros(Rv, np.uint8), plddt=np.zeros(Rv, np.float32),
                     res_index=np.zeros(Rv, np.int32), chain_index=np.zeros(Rv, np.int32), length=np.zeros(n, np.uint32))
            if n and Rv:
                out = CPackedOut(*(d[k].ctypes.data for k in ("pos", "mask", "aatype", "plddt", "res_index", "chain_index", "length")))
                _lib.check(self.lib.fcz_decompress_dense_packed(self.ctx, blob.ctypes.data, off.ctypes.data, n, lay, None, None, ctypes.byref(out),
                                                                None), "fcz_decompress_dense_packed")
            d["mask"] = d["mask"].view(np.bool_)
            d["row_off"] = row_off
            d["status"] = status[:n]
            return d
        L = ctypes.c_uint32(0)
        status = np.zeros(max(n, 1), np.int32)
        if max_len is None:
            padded(0, ctypes.byref(L), None, status.ctypes.data)
        else:
            L.value = int(max_len)
        Lv = int(L.value)
        d = dict(pos=np.zeros((n, Lv, A, 3), np.float32), mask=np.zeros((n, Lv, A), np.uint8), aatype=np.full((n, Lv), 20, np.uint8),
                 plddt=np.zeros((n, Lv), np.float32), res_index=np.zeros((n, Lv), np.int32), length=np.zeros(n, np.uint32))
        if n and Lv:
            out = CDenseOut(*(d[k].ctypes.data for k in ("pos", "mask", "aatype", "plddt", "res_index", "length")))
            padded(Lv, None, ctypes.byref(out), status.ctypes.data)
        d["mask"] = d["mask"].view(np.bool_)
        d["status"] = status[:n]
        return d

    def neighbors(self, pos: np.ndarray, mask: np.ndarray, k: int, slot: int, length=None, row_off=None):
        """dense arrays on the host -> the k-nearest-neighbour graph of every chain on the sites at `slot` (fcz_knn, or
        fcz_knn_packed when row_off is given): index int32 [n, L, k] / [R, k] (-1 = none) and dist float32 of the same shape.
        pos float32 [n, L, A, 3] with mask [n, L, A] and optionally length [n]; or pos [R, A, 3], mask [R, A], row_off [n + 1]."""
        a = _dense_arrays(pos, mask, None, length, row_off,
                          limit=None if row_off is None else (2 ** 31 - 1, "the packed index holds global rows as int32: at most 2^31 - 1 rows"))
        k, slot = int(k), int(slot)
        if not 1 <= k <= 64 or not 0 <= slot < a.A:
            raise ValueError(f"k must be 1 .. 64 and slot 0 .. {a.A - 1}")
        index = np.full(a.lead + (k,), -1, np.int32)
        dist = np.zeros(a.lead + (k,), np.float32)
        if index.size:
            self._call("fcz_knn", a.packed, a.pos.ctypes.data, a.mask.ctypes.data, _addr(a.bound), a.n, a.rows, a.lay, slot, k, index.ctypes.data, dist.ctypes.data)
        return dict(index=index, dist=dist)

    def _call(self, name, packed, *args):
        """the packed or the padded host entry point of one analysis, checked under its own name"""
        name += "_packed" if packed else ""
        _lib.check(getattr(self.lib, name)(self.ctx, *args), name)

    def lddt(self, pos_true: np.ndarray, mask_true: np.ndarray, pos_pred: np.ndarray, mask_pred=None, slot: int = 1, length=None, row_off=None,
             cutoff: float = 15.0, thresholds=None):
        """two sets of dense arrays of one shape on the host -> the per-residue lDDT of `pred` against `true` on the sites at `slot`
        (fcz_lddt, or fcz_lddt_packed when row_off is given): score float32 [n, L] / [R], pairs int32 and hits int32 of the same shape,
        score = hits / (4 * pairs), 0 where a row has no pair. pos float32 [n, L, A, 3] with mask [n, L, A] and optionally length [n];
        or pos [R, A, 3], mask [R, A], row_off [n + 1]. mask_pred=None: every slot of pred is present. These are counts: the result
        is reproducible bit for bit and not differentiable."""
        a, pos_pred, mask_pred, slot = _pair_arrays(pos_true, mask_true, pos_pred, mask_pred, None, length, row_off, slot,
                                                    limit=(2 ** 29, "hits must fit int32: at most 2^29 rows per chain"))
        cutoff = np.float32(cutoff)
        if not np.isfinite(cutoff) or not cutoff > 0:
            raise ValueError("cutoff must be finite and > 0")
        th = None
        if thresholds is not None:
            th = np.ascontiguousarray(thresholds, np.float32)
            if th.shape != (4,) or np.isnan(th).any():
                raise ValueError("thresholds must be four numbers, none of them NaN")
        score = np.zeros(a.lead, np.float32)
        pairs = np.zeros(a.lead, np.int32)
        hits = np.zeros(a.lead, np.int32)
        if score.size:
            self._call("fcz_lddt", a.packed, a.pos.ctypes.data, a.mask.ctypes.data, pos_pred.ctypes.data, _addr(mask_pred), _addr(a.bound), a.n, a.rows, a.lay, slot,
                       float(cutoff), _addr(th), score.ctypes.data, pairs.ctypes.data, hits.ctypes.data)
        return dict(score=score, pairs=pairs, hits=hits)

    def _lddt_soft_inputs(self, pos_true, mask_true, pos_pred, mask_pred, slot, length, row_off, cutoff, thresholds):
        """the prelude of lddt_soft and lddt_soft_grad -> (_Arrays of true, pos_pred, mask_pred, slot, cutoff, thresholds float32 [4] or None)"""
        from . import api
        a, pos_pred, mask_pred, slot = _pair_arrays(pos_true, mask_true, pos_pred, mask_pred, None, length, row_off, slot,
                                                    limit=(2 ** 29, "at most 2^29 rows per chain"))
        _, cutoff, th = api.check_lddt_soft(cutoff, thresholds, slot, a.A)
        return a, pos_pred, mask_pred, slot, cutoff, None if thresholds is None else np.asarray(th, np.float32)

    def lddt_soft(self, pos_true: np.ndarray, mask_true: np.ndarray, pos_pred: np.ndarray, mask_pred=None, slot: int = 1, length=None, row_off=None,
                  cutoff: float = 15.0, thresholds=None):
        """two sets of dense arrays of one shape on the host -> the smooth lDDT sums of `pred` against `true` on the sites at `slot`
        (fcz_lddt_soft, or fcz_lddt_soft_packed when row_off is given): soft float32 [n, L] / [R], the sum over a row's pairs of
        1/4 sum_k sigmoid(t_k - |d_true - d_pred|) in float32 in ascending row order, and pairs int32, which is Codec.lddt's. The
        arrays are Codec.lddt's; thresholds must be finite. soft / pairs is the per-residue smooth lDDT."""
        a, pos_pred, mask_pred, slot, cutoff, th = self._lddt_soft_inputs(pos_true, mask_true, pos_pred, mask_pred, slot, length, row_off, cutoff, thresholds)
        soft = np.zeros(a.lead, np.float32)
        pairs = np.zeros(a.lead, np.int32)
        if soft.size:
            self._call("fcz_lddt_soft", a.packed, a.pos.ctypes.data, a.mask.ctypes.data, pos_pred.ctypes.data, _addr(mask_pred), _addr(a.bound), a.n, a.rows, a.lay,
                       slot, cutoff, _addr(th), soft.ctypes.data, pairs.ctypes.data)
        return dict(soft=soft, pairs=pairs)

    def lddt_soft_grad(self, pos_true: np.ndarray, mask_true: np.ndarray, pos_pred: np.ndarray, weight: np.ndarray, mask_pred=None, slot: int = 1, length=None,
                       row_off=None, cutoff: float = 15.0, thresholds=None):
        """the gradient of sum_i weight[i] * soft[i] of lddt_soft with respect to pos_pred[.., slot, :] (fcz_lddt_soft_grad, or
        fcz_lddt_soft_grad_packed when row_off is given): float32 [n, L, 3] / [R, 3], 0 where a row is no site. weight float32
        [n, L] / [R]. Gathered per row in a fixed order without atomics: reproducible bit for bit."""
        a, pos_pred, mask_pred, slot, cutoff, th = self._lddt_soft_inputs(pos_true, mask_true, pos_pred, mask_pred, slot, length, row_off, cutoff, thresholds)
        weight = np.ascontiguousarray(weight, np.float32)
        if weight.shape != a.lead:
            raise ValueError(f"weight must be float32 {a.lead}, not {weight.shape}")
        grad = np.zeros(a.lead + (3,), np.float32)
        if grad.size:
            self._call("fcz_lddt_soft_grad", a.packed, a.pos.ctypes.data, a.mask.ctypes.data, pos_pred.ctypes.data, _addr(mask_pred), _addr(a.bound), a.n, a.rows,
                       a.lay, slot, cutoff, _addr(th), weight.ctypes.data, grad.ctypes.data)
        return grad

    def _fape_inputs(self, frames_true, pos_true, mask_true, frames_pred, pos_pred, mask_pred, slot, length, row_off, clamp, eps):
        """the prelude of fape and fape_grad -> (_Arrays of true, the ten addresses of the call in its order, slot, clamp, eps, the arrays
        the addresses point into). frames_*: (rot [.., 3, 3] float32, trans [.., 3] float32, frame_mask [..] bool / uint8; None for the
        prediction's: every frame present)"""
        from . import api
        a, pos_pred, mask_pred, slot = _pair_arrays(pos_true, mask_true, pos_pred, mask_pred, None, length, row_off, slot,
                                                    limit=(2 ** 29, "at most 2^29 rows per chain"))
        _, clamp, _, eps = api.check_fape(clamp, 1.0, eps, slot, a.A)
        keep = []
        for which, (rot, trans, fmask) in (("true", frames_true), ("pred", frames_pred)):
            rot, trans = np.ascontiguousarray(rot, np.float32), np.ascontiguousarray(trans, np.float32)
            if rot.shape != a.lead + (3, 3) or trans.shape != a.lead + (3,):
                raise ValueError(f"rot_{which} must be float32 {a.lead + (3, 3)} and trans_{which} {a.lead + (3,)}, not {rot.shape} and {trans.shape}")
            if fmask is None and which == "true":
                raise ValueError("frame_mask of the truth is needed")
            keep += [rot, trans, None if fmask is None else _mask_array(fmask, a.lead, f"frame_mask_{which}")]
        ptrs = [_addr(keep[0]), _addr(keep[1]), _addr(keep[2]), a.pos.ctypes.data, a.mask.ctypes.data, _addr(keep[3]), _addr(keep[4]), _addr(keep[5]),
                pos_pred.ctypes.data, _addr(mask_pred)]
        return a, ptrs, slot, clamp, eps, (keep, pos_pred, mask_pred)

    def fape(self, frames_true, pos_true: np.ndarray, mask_true: np.ndarray, frames_pred, pos_pred: np.ndarray, mask_pred=None, slot: int = 1, length=None,
             row_off=None, clamp=10.0, eps: float = 1e-4):
        """frames and dense arrays of a truth and a prediction on the host -> the backbone FAPE sums (fcz_fape, or fcz_fape_packed when
        row_off is given): sum float32 [n, L] / [R], at a frame row the sum over its chain's points at `slot` of min(sqrt(|R^T (x - t)
        - R'^T (x' - t')|^2 + eps), clamp) in float32 in ascending row order, and points int32, the number of those points.
        frames_true = (rot [.., 3, 3], trans [.., 3], frame_mask [..]) as Codec.frames gives them, frames_pred the same with a
        frame_mask that may be None; the dense arrays are Codec.lddt's. clamp=None or +inf: unclamped. sum / points is the row's FAPE
        before the scale."""
        a, ptrs, slot, clamp, eps, keep = self._fape_inputs(frames_true, pos_true, mask_true, frames_pred, pos_pred, mask_pred, slot, length, row_off, clamp, eps)
        total = np.zeros(a.lead, np.float32)
        points = np.zeros(a.lead, np.int32)
        if total.size:
            self._call("fcz_fape", a.packed, *ptrs, _addr(a.bound), a.n, a.rows, a.lay, slot, clamp, eps, total.ctypes.data, points.ctypes.data)
        return dict(sum=total, points=points)

    def fape_grad(self, frames_true, pos_true: np.ndarray, mask_true: np.ndarray, frames_pred, pos_pred: np.ndarray, weight: np.ndarray, mask_pred=None,
                  slot: int = 1, length=None, row_off=None, clamp=10.0, eps: float = 1e-4):
        """the gradient of sum_i weight[i] * sum[i] of fape with respect to the prediction's rot, trans and pos_pred[.., slot, :]
        (fcz_fape_grad, or fcz_fape_grad_packed when row_off is given): dict(grad_rot float32 [.., 3, 3], grad_trans [.., 3],
        grad_pos [.., 3]), 0 where a row is no frame (grad_rot, grad_trans) or no point (grad_pos). weight float32 [n, L] / [R].
        Gathered per row in a fixed order without atomics: reproducible bit for bit."""
        a, ptrs, slot, clamp, eps, keep = self._fape_inputs(frames_true, pos_true, mask_true, frames_pred, pos_pred, mask_pred, slot, length, row_off, clamp, eps)
        weight = np.ascontiguousarray(weight, np.float32)
        if weight.shape != a.lead:
            raise ValueError(f"weight must be float32 {a.lead}, not {weight.shape}")
        out = dict(grad_rot=np.zeros(a.lead + (3, 3), np.float32), grad_trans=np.zeros(a.lead + (3,), np.float32), grad_pos=np.zeros(a.lead + (3,), np.float32))
        if weight.size:
            self._call("fcz_fape_grad", a.packed, *ptrs, _addr(a.bound), a.n, a.rows, a.lay, slot, clamp, eps, weight.ctypes.data,
                       *(out[k].ctypes.data for k in ("grad_rot", "grad_trans", "grad_pos")))
        return out

    def _fape_atoms_inputs(self, frames_true, pos_true, mask_true, frames_pred, pos_pred, mask_pred, aatype, swapped, length, row_off, clamp, eps, swaps):
        """the prelude of fape_atoms and fape_atoms_grad -> (_Arrays of true, the twelve addresses of the call in its order, clamp, eps,
        the swap table or None, the arrays the addresses point into). frames_*: (rot [.., 8, 3, 3] float32, trans [.., 8, 3] float32,
        frame_mask [.., 8] bool / uint8; None for the prediction's: every frame present)"""
        from . import api
        a, pos_pred, mask_pred, _ = _pair_arrays(pos_true, mask_true, pos_pred, mask_pred, aatype, length, row_off)
        if swapped is not None:
            swapped = _mask_array(swapped, a.lead, "swapped")
        clamp, _, eps, _, table = api.check_fape_atoms(clamp, 1.0, eps, swapped, a.pos.shape, a.aatype is not None, swaps)
        keep = []
        for which, (rot, trans, fmask) in (("true", frames_true), ("pred", frames_pred)):
            rot, trans = np.ascontiguousarray(rot, np.float32), np.ascontiguousarray(trans, np.float32)
            if rot.shape != a.lead + (8, 3, 3) or trans.shape != a.lead + (8, 3):
                raise ValueError(f"rot_{which} must be float32 {a.lead + (8, 3, 3)} and trans_{which} {a.lead + (8, 3)}, not {rot.shape} and {trans.shape}")
            if fmask is None and which == "true":
                raise ValueError("frame_mask of the truth is needed")
            keep += [rot, trans, None if fmask is None else _mask_array(fmask, a.lead + (8,), f"frame_mask_{which}")]
        ptrs = [_addr(keep[0]), _addr(keep[1]), _addr(keep[2]), a.pos.ctypes.data, a.mask.ctypes.data, _addr(a.aatype), _addr(swapped), _addr(keep[3]),
                _addr(keep[4]), _addr(keep[5]), pos_pred.ctypes.data, _addr(mask_pred)]
        return a, ptrs, clamp, eps, table, (keep, pos_pred, mask_pred, swapped)

    def fape_atoms(self, frames_true, pos_true: np.ndarray, mask_true: np.ndarray, frames_pred, pos_pred: np.ndarray, mask_pred=None, aatype=None, swapped=None,
                   length=None, row_off=None, clamp=10.0, eps: float = 1e-4, swaps="alphafold"):
        """frames of the eight rigid groups and dense arrays of a truth and a prediction on the host -> the all-atom FAPE sums
        (fcz_fape_atoms, or fcz_fape_atoms_packed when row_off is given): sum float32 [n, L, 8] / [R, 8], at a frame the sum over
        its chain's points (every atom of every residue) of min(sqrt(|R^T (x - t) - R'^T (x' - t')|^2 + eps), clamp) in float32 in
        ascending (row, slot), and points int32, the number of those points. frames_* = (rot [.., 8, 3, 3], trans [.., 8, 3],
        frame_mask [.., 8]) as Codec.frames(groups="all") gives them; swapped bool / uint8 [n, L] / [R] (Codec.lddt_atoms' output;
        needs aatype) reads the truth of those rows under its other naming: the slots through `swaps`, the ambiguous groups turned
        by 180 degrees. The dense arrays are Codec.lddt_atoms'."""
        a, ptrs, clamp, eps, table, keep = self._fape_atoms_inputs(frames_true, pos_true, mask_true, frames_pred, pos_pred, mask_pred, aatype, swapped, length,
                                                                   row_off, clamp, eps, swaps)
        total = np.zeros(a.lead + (8,), np.float32)
        points = np.zeros(a.lead + (8,), np.int32)
        if total.size:
            self._call("fcz_fape_atoms", a.packed, *ptrs, _addr(a.bound), a.n, a.rows, a.lay, clamp, eps, _addr(table), total.ctypes.data, points.ctypes.data)
        return dict(sum=total, points=points)

    def fape_atoms_grad(self, frames_true, pos_true: np.ndarray, mask_true: np.ndarray, frames_pred, pos_pred: np.ndarray, weight: np.ndarray, mask_pred=None,
                        aatype=None, swapped=None, length=None, row_off=None, clamp=10.0, eps: float = 1e-4, swaps="alphafold"):
        """the gradient of sum weight * sum of fape_atoms with respect to the prediction's rot, trans and pos_pred (fcz_fape_atoms_grad,
        or fcz_fape_atoms_grad_packed when row_off is given): dict(grad_rot float32 [.., 8, 3, 3], grad_trans [.., 8, 3], grad_pos
        [.., A, 3]), 0 where an item is no frame (grad_rot, grad_trans) or a slot no point (grad_pos). weight float32 [.., 8].
        Gathered per element in a fixed order without atomics: reproducible bit for bit."""
        a, ptrs, clamp, eps, table, keep = self._fape_atoms_inputs(frames_true, pos_true, mask_true, frames_pred, pos_pred, mask_pred, aatype, swapped, length,
                                                                   row_off, clamp, eps, swaps)
        weight = np.ascontiguousarray(weight, np.float32)
        if weight.shape != a.lead + (8,):
            raise ValueError(f"weight must be float32 {a.lead + (8,)}, not {weight.shape}")
        out = dict(grad_rot=np.zeros(a.lead + (8, 3, 3), np.float32), grad_trans=np.zeros(a.lead + (8, 3), np.float32), grad_pos=np.zeros(a.pos.shape, np.float32))
        if weight.size:
            self._call("fcz_fape_atoms_grad", a.packed, *ptrs, _addr(a.bound), a.n, a.rows, a.lay, clamp, eps, _addr(table), weight.ctypes.data,
                       *(out[k].ctypes.data for k in ("grad_rot", "grad_trans", "grad_pos")))
        return out

    def lddt_atoms(self, pos_true: np.ndarray, mask_true: np.ndarray, pos_pred: np.ndarray, mask_pred=None, aatype=None, length=None, row_off=None, *,
                   cutoff: float = 15.0, thresholds=None, swaps="alphafold", per_atom: bool = False):
        """two sets of dense arrays of one shape on the host -> the all-atom lDDT of `pred` against `true` after the symmetric
        side-chain namings of the truth have been resolved (fcz_lddt_atoms, or fcz_lddt_atoms_packed when row_off is given): score
        float32 [n, L] / [R], pairs int32, hits int32, swapped bool and, with per_atom, atom_pairs / atom_hits int32 [.., A]. The
        arrays are Codec.lddt's, with aatype uint8 [n, L] / [R] (needed unless swaps=None); cutoff, thresholds, swaps and per_atom
        are foldcomp.lddt_atoms'. These are counts: reproducible bit for bit and not differentiable."""
        from . import api
        from .structure import CLddtAtomsOut
        pos_true, pos_pred = np.ascontiguousarray(pos_true, np.float32), np.ascontiguousarray(pos_pred, np.float32)
        if pos_true.ndim != (3 if row_off is not None else 4):
            raise _pos_error("pos_true", row_off is not None, pos_true.shape)
        cutoff, th, table = api.check_lddt_atoms(cutoff, thresholds, swaps, pos_true.shape, pos_pred.shape, None, aatype is not None, per_atom)
        a, pos_pred, mask_pred, _ = _pair_arrays(pos_true, mask_true, pos_pred, mask_pred, None if table is False else aatype, length, row_off)
        out = dict(score=np.zeros(a.lead, np.float32), pairs=np.zeros(a.lead, np.int32), hits=np.zeros(a.lead, np.int32), swapped=np.zeros(a.lead, np.uint8))
        if per_atom:
            out.update(atom_pairs=np.zeros(a.lead + (a.A,), np.int32), atom_hits=np.zeros(a.lead + (a.A,), np.int32))
        if out["score"].size:
            th = np.asarray(th, np.float32)
            c_out = CLddtAtomsOut(*(out[k].ctypes.data if k in out else None for k in ("score", "pairs", "hits", "swapped", "atom_pairs", "atom_hits")))
            self._call("fcz_lddt_atoms", a.packed, a.pos.ctypes.data, a.mask.ctypes.data, pos_pred.ctypes.data, _addr(mask_pred), _addr(a.aatype), _addr(a.bound),
                       a.n, a.rows, a.lay, cutoff, th.ctypes.data, table.ctypes.data if isinstance(table, np.ndarray) else None, ctypes.byref(c_out))
        out["swapped"] = out["swapped"].view(np.bool_)
        return out

    def secondary_structure(self, pos: np.ndarray, mask: np.ndarray, aatype=None, length=None, row_off=None):
        """dense arrays on the host -> the DSSP labels and backbone hydrogen bonds of every chain (fcz_dssp, or fcz_dssp_packed when
        row_off is given): ss uint8 [n, L] / [R] (codes in the order of foldcomp.SS_CLASSES), ss_mask bool, and the tables
        hbond_acc_index / hbond_don_index int32 [.., 2] (-1 = none) with hbond_acc_energy / hbond_don_energy float32. pos float32
        [n, L, A, 3] with mask [n, L, A], optionally aatype [n, L] uint8 (proline has no amide hydrogen) and length [n]; or pos
        [R, A, 3], mask [R, A], aatype [R], row_off [n + 1]. Reproducible bit for bit, not differentiable."""
        a = _dense_arrays(pos, mask, aatype, length, row_off)
        out = dict(ss=np.zeros(a.lead, np.uint8), ss_mask=np.zeros(a.lead, np.uint8),
                   hbond_acc_index=np.full(a.lead + (2,), -1, np.int32), hbond_acc_energy=np.zeros(a.lead + (2,), np.float32),
                   hbond_don_index=np.full(a.lead + (2,), -1, np.int32), hbond_don_energy=np.zeros(a.lead + (2,), np.float32))
        if out["ss"].size:
            self._call("fcz_dssp", a.packed, a.pos.ctypes.data, a.mask.ctypes.data, _addr(a.aatype), _addr(a.bound), a.n, a.rows, a.lay,
                       out["hbond_acc_index"].ctypes.data, out["hbond_acc_energy"].ctypes.data, out["hbond_don_index"].ctypes.data,
                       out["hbond_don_energy"].ctypes.data, out["ss"].ctypes.data, out["ss_mask"].ctypes.data)
        out["ss_mask"] = out["ss_mask"].view(np.bool_)
        return out

    def solvent_accessibility(self, pos: np.ndarray, mask: np.ndarray, aatype=None, length=None, row_off=None, *, probe: float = 1.4,
                              n_points: int = 128, points=None, radii="bondi"):
        """dense arrays on the host -> the Shrake-Rupley solvent accessibility of every residue (fcz_sasa, or fcz_sasa_packed when
        row_off is given): sasa float32 [n, L] / [R] in square Angstrom, rsa float32 (sasa / foldcomp.MAX_ASA[aatype]; 0 without
        aatype, where the maximum is 0 or sasa_mask is off), sasa_mask bool (the row has an atom) and sasa_points int16 [.., A], the
        exposed points of every atom slot. pos float32 [n, L, A, 3] with mask [n, L, A], aatype [n, L] uint8 (needed for atom14) and
        optionally length [n]; or pos [R, A, 3], mask [R, A], aatype [R], row_off [n + 1]. probe, n_points, points and radii are
        foldcomp.solvent_accessibility's. Reproducible bit for bit, not differentiable."""
        from . import api
        a = _dense_arrays(pos, mask, aatype, length, row_off)
        _, _, pts, table = api.check_sasa("Codec.solvent_accessibility", a.as_dict(row_off), probe, n_points, points, radii)
        out = dict(sasa=np.zeros(a.lead, np.float32), rsa=np.zeros(a.lead, np.float32), sasa_mask=np.zeros(a.lead, np.uint8),
                   sasa_points=np.zeros(a.lead + (a.A,), np.int16))
        if out["sasa"].size:
            self._call("fcz_sasa", a.packed, a.pos.ctypes.data, a.mask.ctypes.data, _addr(a.aatype), _addr(a.bound), a.n, a.rows, a.lay, _addr(table), float(probe),
                       pts.ctypes.data, len(pts), out["sasa_points"].ctypes.data, out["sasa"].ctypes.data, out["sasa_mask"].ctypes.data)
        out["sasa_mask"] = out["sasa_mask"].view(np.bool_)
        if a.aatype is not None:
            mx = api.MAX_ASA[np.minimum(a.aatype, 20)]
            ok = (mx > 0) & out["sasa_mask"]
            out["rsa"][ok] = out["sasa"][ok] / mx[ok]
        return out

    def violations(self, pos: np.ndarray, mask: np.ndarray, aatype=None, length=None, row_off=None, *, tolerance: float = 1.5,
                   link_factor: float = 12.0, radii="bondi"):
        """dense arrays on the host -> the steric clashes and peptide-link violations of every chain (fcz_violations, or
        fcz_violations_packed when row_off is given): clash_atom uint8 [.., A], clash_count int32, clash_depth float32, clash_partner
        int32 (-1 = none), viol_mask bool, link_mask bool, link_length float32, link_cos float32 [.., 2], link_violation uint8 (three
        bits) per row [n, L] / [R], and chain_counts int64 [n, 4]. pos float32 [n, L, A, 3] with mask [n, L, A], aatype [n, L] uint8
        (needed for atom14) and optionally length [n]; or pos [R, A, 3], mask [R, A], aatype [R], row_off [n + 1]. tolerance,
        link_factor and radii are foldcomp.violations'. Reproducible bit for bit, not differentiable."""
        from . import api
        from .structure import CViolationsOut
        a = _dense_arrays(pos, mask, aatype, length, row_off)
        _, _, table = api.check_violations("Codec.violations", a.as_dict(row_off), tolerance, link_factor, radii)
        out = {}
        for key, dt, tail in api.VIOLATION_OUTPUTS:
            shape = (a.n, 4) if tail == "n4" else a.lead + ((a.A,) if tail == "A" else tail)
            out[key] = np.full(shape, -1, np.int32) if key == "clash_partner" else np.zeros(shape, np.uint8 if dt == "bool" else dt)
        if out["clash_count"].size:
            c_out = CViolationsOut(*(out[key].ctypes.data for key, _, _ in api.VIOLATION_OUTPUTS))
            self._call("fcz_violations", a.packed, a.pos.ctypes.data, a.mask.ctypes.data, _addr(a.aatype), _addr(a.bound), a.n, a.rows, a.lay, _addr(table),
                       float(tolerance), float(link_factor), ctypes.byref(c_out))
        for key, dt, _ in api.VIOLATION_OUTPUTS:
            if dt == "bool":
                out[key] = out[key].view(np.bool_)
        return out

    def violation_loss(self, pos: np.ndarray, mask: np.ndarray, aatype=None, length=None, row_off=None, *, tolerance: float = 1.5,
                       link_factor: float = 12.0, radii="bondi"):
        """dense arrays on the host -> the violation loss of every chain (fcz_violation_loss, or fcz_violation_loss_packed when
        row_off is given): clash_loss float32 [.., A], for every atom the sum of (Ri + Rj) - tolerance - distance over the atoms of
        other residues it clashes with, in ascending (row, slot); link_loss float32 [.., 3], how far the C-N' length and the two
        peptide cosines of the link to the next row lie outside link_factor sigmas; counts int64 [n, 2], the chain's atoms and links.
        The arrays and the parameters are Codec.violations'; atoms, pairs and links are its too. Reproducible bit for bit."""
        from . import api
        a = _dense_arrays(pos, mask, aatype, length, row_off)
        _, _, table = api.check_violation_loss("Codec.violation_loss", a.as_dict(row_off), tolerance, link_factor, radii)
        out = dict(clash_loss=np.zeros(a.lead + (a.A,), np.float32), link_loss=np.zeros(a.lead + (3,), np.float32), counts=np.zeros((a.n, 2), np.int64))
        if out["link_loss"].size:
            self._call("fcz_violation_loss", a.packed, a.pos.ctypes.data, a.mask.ctypes.data, _addr(a.aatype), _addr(a.bound), a.n, a.rows, a.lay, _addr(table),
                       float(tolerance), float(link_factor), out["clash_loss"].ctypes.data, out["link_loss"].ctypes.data, out["counts"].ctypes.data)
        return out

    def violation_loss_grad(self, pos: np.ndarray, mask: np.ndarray, w_clash: np.ndarray, w_link: np.ndarray, aatype=None, length=None, row_off=None, *,
                            tolerance: float = 1.5, link_factor: float = 12.0, radii="bondi"):
        """the gradient of sum w_clash * clash_loss + sum w_link * link_loss of violation_loss with respect to pos
        (fcz_violation_loss_grad, or fcz_violation_loss_grad_packed when row_off is given): float32 of pos' shape, 0 where a slot is
        neither an atom nor a link atom. w_clash float32 [.., A], w_link float32 [.., 3]. Gathered per slot in a fixed order without
        atomics: reproducible bit for bit."""
        from . import api
        a = _dense_arrays(pos, mask, aatype, length, row_off)
        _, _, table = api.check_violation_loss("Codec.violation_loss_grad", a.as_dict(row_off), tolerance, link_factor, radii)
        w_clash, w_link = np.ascontiguousarray(w_clash, np.float32), np.ascontiguousarray(w_link, np.float32)
        if w_clash.shape != a.lead + (a.A,) or w_link.shape != a.lead + (3,):
            raise ValueError(f"w_clash must be float32 {a.lead + (a.A,)} and w_link {a.lead + (3,)}, not {w_clash.shape} and {w_link.shape}")
        grad = np.zeros(a.lead + (a.A, 3), np.float32)
        if grad.size:
            self._call("fcz_violation_loss_grad", a.packed, a.pos.ctypes.data, a.mask.ctypes.data, _addr(a.aatype), _addr(a.bound), a.n, a.rows, a.lay,
                       _addr(table), float(tolerance), float(link_factor), w_clash.ctypes.data, w_link.ctypes.data, grad.ctypes.data)
        return grad

    def superpose(self, pos_true: np.ndarray, mask_true: np.ndarray, pos_pred: np.ndarray, mask_pred=None, slot: int = 1, length=None, row_off=None):
        """two sets of dense arrays of one shape on the host -> the least-squares superposition of every chain of `pred` onto `true`
        on the sites at `slot` (fcz_superpose, or fcz_superpose_packed when row_off is given): rot float32 [n, 3, 3] and trans [n, 3]
        (x_true ~ rot @ x_pred + trans), rmsd [n], sites int32 [n], gdt_counts int32 [n, 5] (dev <= 0.5, 1, 2, 4, 8), tm [n] (the
        TM-score at this superposition, a lower bound of the maximised one) and dev float32 [n, L] / [R], every site's deviation.
        The arrays are those of Codec.lddt. The sums are float64 in a fixed order: reproducible bit for bit, not differentiable."""
        a, pos_pred, mask_pred, slot = _pair_arrays(pos_true, mask_true, pos_pred, mask_pred, None, length, row_off, slot)
        d = self._superpose_outputs(a.n, a.lead)
        if a.n and a.rows:
            out = CSuperposeOut(*(d[k].ctypes.data for k in ("rot", "trans", "rmsd", "sites", "gdt_counts", "tm", "dev")))
            self._call("fcz_superpose", a.packed, a.pos.ctypes.data, a.mask.ctypes.data, pos_pred.ctypes.data, _addr(mask_pred), _addr(a.bound), a.n, a.rows, a.lay,
                       slot, ctypes.byref(out))
        return d

    def tm_score(self, pos_true: np.ndarray, mask_true: np.ndarray, pos_pred: np.ndarray, mask_pred=None, slot: int = 1, length=None, row_off=None,
                 iterations: int = 20, levels=None):
        """two sets of dense arrays of one shape on the host -> per chain the superposition that maximises the TM-score over the
        seeded iterative search of fcz_tmscore (fcz_tmscore_packed when row_off is given; the definition: include/fcz_hip.h), and
        Codec.superpose's outputs at it: rot, trans, rmsd, sites, gdt_counts, tm, dev; beside them seed int32 [n], the winning
        seed's number, and selected int32 [n], the size of the winning selection. tm >= Codec.superpose's tm. iterations: rounds of
        refinement per seed, 0 .. 64; levels: only the first so many fragment lengths (None: all). Reproducible bit for bit."""
        a, pos_pred, mask_pred, slot = _pair_arrays(pos_true, mask_true, pos_pred, mask_pred, None, length, row_off, slot)
        from .api import check_tm_search
        iterations, levels = check_tm_search(iterations, levels)
        d = self._superpose_outputs(a.n, a.lead)
        d.update(seed=np.zeros(a.n, np.int32), selected=np.zeros(a.n, np.int32))
        if a.n and a.rows:
            out = CTmScoreOut(*(d[k].ctypes.data for k in ("rot", "trans", "rmsd", "sites", "gdt_counts", "tm", "dev", "seed", "selected")))
            self._call("fcz_tmscore", a.packed, a.pos.ctypes.data, a.mask.ctypes.data, pos_pred.ctypes.data, _addr(mask_pred), _addr(a.bound), a.n, a.rows, a.lay,
                       slot, levels, iterations, ctypes.byref(out))
        return d

    def gdt(self, pos_true: np.ndarray, mask_true: np.ndarray, pos_pred: np.ndarray, mask_pred=None, slot: int = 1, length=None, row_off=None,
            iterations: int = 20, levels=None, runs="all"):
        """two sets of dense arrays of one shape on the host -> per chain and per cutoff of 0.5, 1, 2, 4, 8 A the largest number of sites
        that a superposition of the seeded search of fcz_gdt brings under it (fcz_gdt_packed when row_off is given; the definition:
        include/fcz_hip.h): gdt_counts int32 [n, 5], sites int32 [n], rot float32 [n, 5, 3, 3] and trans [n, 5, 3] (the
        superposition behind each count), seed, run, selected int32 [n, 5] and within uint8 [n, L] / [R] (bit k: the row lies
        within cutoff k under transform k). gdt_counts >= Codec.superpose's. iterations and levels are Codec.tm_score's; runs:
        "all", "tm" or an iterable of "tm" and cutoffs. Reproducible bit for bit."""
        a, pos_pred, mask_pred, slot = _pair_arrays(pos_true, mask_true, pos_pred, mask_pred, None, length, row_off, slot)
        from .api import check_gdt_runs, check_tm_search
        iterations, levels = check_tm_search(iterations, levels)
        runs = check_gdt_runs(runs)
        n = a.n
        d = dict(gdt_counts=np.zeros((n, 5), np.int32), sites=np.zeros(n, np.int32), rot=np.tile(np.eye(3, dtype=np.float32), (n, 5, 1, 1)),
                 trans=np.zeros((n, 5, 3), np.float32), seed=np.zeros((n, 5), np.int32), run=np.zeros((n, 5), np.int32),
                 selected=np.zeros((n, 5), np.int32), within=np.zeros(a.lead, np.uint8))
        if a.n and a.rows:
            out = CGdtOut(*(d[k].ctypes.data for k in ("gdt_counts", "sites", "rot", "trans", "seed", "run", "selected", "within")))
            self._call("fcz_gdt", a.packed, a.pos.ctypes.data, a.mask.ctypes.data, pos_pred.ctypes.data, _addr(mask_pred), _addr(a.bound), a.n, a.rows, a.lay,
                       slot, levels, iterations, runs, ctypes.byref(out))
        return d

    def tm_align(self, pos_a: np.ndarray, mask_a: np.ndarray, pos_b=None, mask_b=None, pairs=None, slot: int = 1, *, length_a=None, row_off_a=None,
                 length_b=None, row_off_b=None, fragments: bool = True, refine: int = 4, dp_rounds: int = 20, gaps=(0.6, 0.0), iterations: int = 20,
                 levels=None):
        """two sets of chains on the host, each padded (pos [n, L, A, 3], mask [n, L, A], length [n] or None) or packed (pos [R, A, 3],
        mask [R, A], row_off [n + 1]), and pairs int32 [m, 2] of chain indices -> the TM-align-style alignment of every pair (fcz_tmalign;
        the definition: include/fcz_hip.h): rot [m, 3, 3], trans [m, 3] (x_b ~ rot @ x_a + trans), tm (by the shorter chain), tm_a, tm_b,
        rmsd float32 [m], aligned, sites_a, sites_b, seed, status int32 [m], map int32 [m, wa] (the chain-relative row of b of every row of
        a, -1 = unaligned) and dev float32 [m, wa], wa being L or the longest chain of a packed a. pos_b None: b is a; pairs None: every
        i < j of a, or every (i, j) of a and b. The other arguments are foldcomp.tm_align's. Reproducible bit for bit."""
        a, b, pairs, wa, wb, lay, par, _kept = _tm_align_inputs(pos_a, mask_a, pos_b, mask_b, pairs, slot, length_a, row_off_a, length_b, row_off_b,
                                                                fragments, refine, dp_rounds, gaps, iterations, levels, None)
        from .structure import TM_ALIGN_OUTPUTS, CTmAlignOut, CTmAlignParams
        m = len(pairs)
        d = {k: np.zeros((m,) + ((wa,) if tail == "wa" else tail), dt) for k, dt, tail in TM_ALIGN_OUTPUTS}
        d["rot"][:] = np.eye(3, dtype=np.float32)
        d["map"][:] = -1
        if m:
            slot, frag, refine, dp_rounds, gs, iterations, levels = par
            p = CTmAlignParams(frag, refine, dp_rounds, len(gs), (ctypes.c_double * 4)(*gs), levels, iterations)
            out = CTmAlignOut(*(d[k].ctypes.data for k, _, _ in TM_ALIGN_OUTPUTS))
            _lib.check(self.lib.fcz_tmalign(self.ctx, ctypes.byref(a), ctypes.byref(b), pairs.ctypes.data, m, wa, wb, lay, slot, ctypes.byref(p),
                                            ctypes.byref(out)), "fcz_tmalign")
        d["pairs"] = pairs
        return d

    def tm_align_dp(self, pos_a: np.ndarray, mask_a: np.ndarray, pos_b, mask_b, pairs, rot, trans, gap: float = 0.6, slot: int = 1, *, length_a=None,
                    row_off_a=None, length_b=None, row_off_b=None):
        """the dynamic programme of tm_align alone (fcz_tmalign_dp), once per pair from the caller's transforms rot float32 [m, 3, 3],
        trans [m, 3] (x_b ~ rot @ x_a + trans) and one gap penalty -> map int32 [m, wa], aligned int32 [m], pairs. The integer DP is exact:
        numpy reproduces it bit for bit from the same transforms (include/fcz_hip.h)."""
        a, b, pairs, wa, wb, lay, par, _kept = _tm_align_inputs(pos_a, mask_a, pos_b, mask_b, pairs, slot, length_a, row_off_a, length_b, row_off_b,
                                                                True, 4, 20, (gap,), 20, None, (rot, trans))
        m = len(pairs)
        rot, trans = np.ascontiguousarray(rot, np.float32), np.ascontiguousarray(trans, np.float32)
        d = dict(map=np.full((m, wa), -1, np.int32), aligned=np.zeros(m, np.int32), pairs=pairs)
        if m:
            _lib.check(self.lib.fcz_tmalign_dp(self.ctx, ctypes.byref(a), ctypes.byref(b), pairs.ctypes.data, m, wa, wb, lay, par[0], rot.ctypes.data,
                                               trans.ctypes.data, float(gap), d["map"].ctypes.data, d["aligned"].ctypes.data), "fcz_tmalign_dp")
        return d

    @staticmethod
    def _superpose_outputs(n, rows_shape):
        return dict(rot=np.tile(np.eye(3, dtype=np.float32), (n, 1, 1)), trans=np.zeros((n, 3), np.float32), rmsd=np.zeros(n, np.float32),
                    sites=np.zeros(n, np.int32), gdt_counts=np.zeros((n, 5), np.int32), tm=np.zeros(n, np.float32), dev=np.zeros(rows_shape, np.float32))

    def apply_transform(self, pos: np.ndarray, rot: np.ndarray, trans: np.ndarray, mask=None, length=None, row_off=None):
        """dense coordinates on the host moved by one rigid transform per chain (fcz_superpose_apply, or fcz_superpose_apply_packed
        when row_off is given) -> pos_out float32 of the shape of pos: rot[e] @ x + trans[e] for every slot whose mask is set (None:
        every slot) in the rows of chain e, 0 elsewhere; float32 in the order x' = ((r00 x + r01 y) + r02 z) + tx."""
        a = _dense_arrays(pos, mask, None, length, row_off, mask_optional=True)
        n = a.n
        rot, trans = np.ascontiguousarray(rot, np.float32), np.ascontiguousarray(trans, np.float32)
        if rot.shape != (n, 3, 3) or trans.shape != (n, 3):
            raise ValueError(f"rot must be [{n}, 3, 3] and trans [{n}, 3], one transform per chain, not {rot.shape} and {trans.shape}")
        out = np.zeros(a.pos.shape, np.float32)
        if n and out.size:
            self._call("fcz_superpose_apply", a.packed, a.pos.ctypes.data, _addr(a.mask), _addr(a.bound), n, a.rows, a.lay, rot.ctypes.data, trans.ctypes.data,
                       out.ctypes.data)
        return out

    def frames(self, pos: np.ndarray, mask: np.ndarray, aatype=None, length=None, layout=None, groups="backbone"):
        """dense arrays on the host -> the rigid frames of every residue (fcz_frames): rot float32 [.., 3, 3], trans [.., 3] and
        frame_mask bool [..] for groups="backbone", [.., 8, 3, 3] / [.., 8, 3] / [.., 8] for "all" (which needs aatype). pos float32
        [n, L, A, 3] with mask [n, L, A], aatype [n, L] and optionally length [n]; or the packed pos [R, A, 3], mask [R, A], aatype [R].
        layout: inferred from A when None."""
        pos = np.ascontiguousarray(pos, np.float32)
        if pos.ndim not in (3, 4) or pos.shape[-1] != 3 or pos.shape[-2] not in WIDTH_LAYOUTS:
            raise ValueError(f"pos must be float32 [n, L, A, 3] or [R, A, 3] with A = 37, 14 or 4, not {pos.shape}")
        A = pos.shape[-2]
        lay = WIDTH_LAYOUTS[A]
        if layout is not None and dense_layout(layout) != lay:
            raise ValueError(f"layout {layout!r} does not have {A} slots per residue")
        if groups not in ("backbone", "all"):
            raise ValueError(f"groups must be 'backbone' or 'all', not {groups!r}")
        fgroups = 1 if groups == "all" else 0
        mask = _mask_array(mask, pos.shape[:-1])
        rows = pos.shape[:-2]
        if aatype is None:
            if fgroups:
                raise ValueError("groups='all' needs aatype: the chi groups depend on the residue type")
        else:
            aatype = np.ascontiguousarray(aatype, np.uint8)
            if aatype.shape != rows:
                raise ValueError(f"aatype must be uint8 {rows}, not {aatype.shape}")
        n, L = (1, rows[0]) if len(rows) == 1 else rows
        bound = None
        if length is not None:
            if len(rows) == 1:
                raise ValueError("the packed form takes no length")
            bound = np.ascontiguousarray(length, np.uint32)
            if bound.shape != (n,):
                raise ValueError(f"length must be [{n}], not {bound.shape}")
        g = (8,) if fgroups else ()
        rot = np.zeros(rows + g + (3, 3), np.float32)
        rot[..., 0, 0] = rot[..., 1, 1] = rot[..., 2, 2] = 1.0
        trans = np.zeros(rows + g + (3,), np.float32)
        fm = np.zeros(rows + g, np.uint8)
        if fm.size:
            self._call("fcz_frames", False, pos.ctypes.data, mask.ctypes.data, _addr(aatype), _addr(bound), n, L, lay, fgroups, rot.ctypes.data, trans.ctypes.data,
                       fm.ctypes.data)
        return dict(rot=rot, trans=trans, frame_mask=fm.view(np.bool_))

    def decompress_angles(self, blob: np.ndarray, off: np.ndarray, L: int = 0, packed: bool = False, start=None):
        """FCZ entries -> the record's internal coordinates on the host (fcz_decompress_angles): angles float32 [n, L, 10] in degrees
        (ANGLE_COLUMNS), angle_mask bool [n, L, 10], status int32 [n]; L = 0: the longest entry of the batch, longer entries are
        cropped. packed=True (fcz_decompress_angles_packed): angles [R, 10], angle_mask [R, 10], row_off uint32 [n + 1]; no L.
        The sizes pass and the angle kernel only: nothing is reconstructed.
        start [n] (fcz_decompress_angles_window): row l of entry e holds its residue start[e] + l, or zeros when it has none, and the
        dict gains aatype uint8 [n, L] (20 in the padding). Not with packed=True."""
        blob = np.ascontiguousarray(blob, np.uint8)
        off = np.ascontiguousarray(off, np.uint64)
        n = len(off) - 1
        if start is not None and packed:
            raise ValueError("start keeps a window of rows per entry; the packed form keeps every residue (packed=True takes no start)")
        st = None if start is None else self._window_starts(start, n)
        aatype = None
        if packed and L:
            raise ValueError("L crops to a common length; the packed form keeps every residue (packed=True takes no L)")
        if int(L) < 0:
            raise ValueError("L must not be negative")
        W = len(ANGLE_COLUMNS)
        width = ctypes.c_uint32(int(L))
        status = np.zeros(max(n, 1), np.int32)
        row_off = np.zeros(n + 1, np.uint32)

        def call(angles, mask, status):
            if packed:
                _lib.check(self.lib.fcz_decompress_angles_packed(self.ctx, blob.ctypes.data, off.ctypes.data, n, ctypes.byref(width), row_off.ctypes.data,
                                                                 angles, mask, status), "fcz_decompress_angles_packed")
            elif st is not None:
                _lib.check(self.lib.fcz_decompress_angles_window(self.ctx, blob.ctypes.data, off.ctypes.data, n, int(L), st.ctypes.data, ctypes.byref(width),
                                                                 angles, mask, None if aatype is None else aatype.ctypes.data, status),
                           "fcz_decompress_angles_window")
            else:
                _lib.check(self.lib.fcz_decompress_angles(self.ctx, blob.ctypes.data, off.ctypes.data, n, int(L), ctypes.byref(width), angles, mask, status),
                           "fcz_decompress_angles")

        if n:
            call(None, None, status.ctypes.data)
        Wd = int(width.value)
        shape = (Wd, W) if packed else (n, Wd, W)
        d = dict(angles=np.zeros(shape, np.float32), angle_mask=np.zeros(shape, np.uint8))
        if st is not None:
            d["aatype"] = aatype = np.full((n, Wd), 20, np.uint8)
        if n and Wd:
            call(d["angles"].ctypes.data, d["angle_mask"].ctypes.data, None)
        d["angle_mask"] = d["angle_mask"].view(np.bool_)
        if packed:
            d["row_off"] = row_off
        d["status"] = status[:n]
        return d

    def _dense_in(self, pos, mask, aatype, length, plddt, layout, first_res_index, chain_id, titles):
        """numpy arrays of one dense batch, checked against each other -> (CDenseIn of host pointers, n, L, layout enum, keep-alive)"""
        lay = dense_layout(layout)
        A = self.lib.fcz_dense_width(lay)
        pos = np.ascontiguousarray(pos, np.float32)
        if pos.ndim != 4 or pos.shape[2:] != (A, 3):
            raise ValueError(f"pos must be [n, L, {A}, 3] for layout {layout!r}, not {tuple(pos.shape)}")
        n, L = int(pos.shape[0]), int(pos.shape[1])
        mask = np.ascontiguousarray(mask)
        mask = mask.view(np.uint8) if mask.dtype == np.bool_ else np.ascontiguousarray(mask, np.uint8)
        aatype = np.ascontiguousarray(aatype, np.uint8)
        length = np.asarray(length)
        if length.size and (length.astype(np.int64) < 0).any():
            raise ValueError("length must not be negative")
        length = np.ascontiguousarray(length, np.uint32)
        if mask.shape != (n, L, A) or aatype.shape != (n, L) or length.shape != (n,):
            raise ValueError(f"mask {mask.shape}, aatype {aatype.shape}, length {length.shape} do not fit pos {tuple(pos.shape)}")
        keep = [pos, mask, aatype, length]
        s = CDenseIn(pos.ctypes.data, mask.ctypes.data, aatype.ctypes.data, length.ctypes.data)

        def per(a, dtype, shape, what):
            a = np.ascontiguousarray(a, dtype)
            if a.shape != shape:
                raise ValueError(f"{what} must have shape {shape}, not {a.shape}")
            keep.append(a)
            return a.ctypes.data

        if plddt is not None:
            s.plddt = per(plddt, np.float32, (n, L), "plddt")
        if first_res_index is not None:
            s.first_res_index = per(first_res_index, np.int32, (n,), "first_res_index")
        if chain_id is not None:
            ids = [ord(c) if isinstance(c, str) else int(c) for c in chain_id]
            s.chain_id = per(ids, np.uint8, (n,), "chain_id")
        if titles is not None:
            tb = [t.encode("latin-1", "replace") if isinstance(t, str) else bytes(t) for t in titles]
            if len(tb) != n:
                raise ValueError(f"{len(tb)} titles for {n} chains")
            toff = np.zeros(n + 1, np.uint32)
            toff[1:] = np.cumsum([len(t) for t in tb])
            tt = np.frombuffer(b"".join(tb) or b"\0", np.uint8)
            keep += [toff, tt]
            s.titles, s.title_off = tt.ctypes.data, toff.ctypes.data
        return s, n, L, lay, keep

    def compress_dense(self, pos, mask, aatype, length, plddt=None, *, layout="atom37", first_res_index=None, chain_id=None, titles=None,
                       anchor_threshold: int = 25):
        """dense padded arrays on the host -> (blob uint8[...], off uint64[n + 1], status int32[n]): fcz_compress_dense_begin /
        _fetch, the gather into the codec's flat batch and the codec both on the GPU. pos [n, L, A, 3] float32, mask [n, L, A] (bool
        or uint8), aatype [n, L], length [n], plddt [n, L] or None (0). Rows behind length[c] and atoms whose mask is 0 are never
        read as data. A refused chain (status != 0; include/fcz_hip.h, fcz_dense_in) leaves zeros in its record range."""
        s, n, L, lay, keep = self._dense_in(pos, mask, aatype, length, plddt, layout, first_res_index, chain_id, titles)
        if n == 0:
            return np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.int32)
        counts = np.zeros(3, np.uint32); nbytes = ctypes.c_uint64(0)
        _lib.check(self.lib.fcz_compress_dense_begin(self.ctx, ctypes.byref(s), n, L, lay, int(anchor_threshold), counts.ctypes.data,
                                                     ctypes.byref(nbytes)), "fcz_compress_dense_begin")
        off = np.zeros(n + 1, np.uint64); st = np.zeros(n, np.int32); blob = np.zeros(max(int(nbytes.value), 1), np.uint8)
        _lib.check(self.lib.fcz_compress_dense_fetch(self.ctx, off.ctypes.data, st.ctypes.data, blob.ctypes.data), "fcz_compress_dense_fetch")
        return blob[:int(nbytes.value)], off, st

    def compress_dense_packed(self, pos, mask, aatype, row_off, plddt=None, *, layout="atom37", first_res_index=None, chain_id=None, titles=None,
                              anchor_threshold: int = 25):
        """packed dense arrays on the host -> (blob, off uint64[n + 1], status int32[n]): fcz_compress_dense_packed_begin / fcz_compress_dense_fetch.
        pos [R, A, 3] float32, mask [R, A], aatype [R], plddt [R] or None, row_off [n + 1]: chain c is rows row_off[c] .. row_off[c + 1] - 1.
        The contract is compress_dense's; a chain whose range runs backwards, leaves the R rows or holds more than 65 535 of them is refused."""
        lay = dense_layout(layout)
        A = self.lib.fcz_dense_width(lay)
        pos = np.ascontiguousarray(pos, np.float32)
        if pos.ndim != 3 or pos.shape[1:] != (A, 3):
            raise ValueError(f"pos must be [R, {A}, 3] for layout {layout!r}, not {tuple(pos.shape)}")
        R = int(pos.shape[0])
        row_off = np.asarray(row_off)
        if row_off.ndim != 1 or len(row_off) < 1:
            raise ValueError("row_off must be [n + 1]")
        if (row_off.astype(np.int64) < 0).any() or (row_off.astype(np.int64) > 2 ** 32 - 1).any():
            raise ValueError("row_off must fit unsigned 32 bits")
        n = len(row_off) - 1
        # the padded checker over [1, R]: shapes, dtypes, per-chain header fields (its length and L are not handed on)
        s, _, _, _, keep = self._dense_in(pos[None], np.asarray(mask)[None], np.asarray(aatype)[None], np.zeros(1, np.uint32),
                                          None if plddt is None else np.asarray(plddt)[None], layout, None, None, None)
        s.length = None
        ro = np.ascontiguousarray(row_off, np.uint32)
        keep.append(ro)

        def per(a, dtype, what):
            a = np.ascontiguousarray(a, dtype)
            if a.shape != (n,):
                raise ValueError(f"{what} must have shape {(n,)}, not {a.shape}")
            keep.append(a)
            return a.ctypes.data

        if first_res_index is not None:
            s.first_res_index = per(first_res_index, np.int32, "first_res_index")
        if chain_id is not None:
            s.chain_id = per([ord(c) if isinstance(c, str) else int(c) for c in chain_id], np.uint8, "chain_id")
        if titles is not None:
            tb = [t.encode("latin-1", "replace") if isinstance(t, str) else bytes(t) for t in titles]
            if len(tb) != n:
                raise ValueError(f"{len(tb)} titles for {n} chains")
            toff = np.zeros(n + 1, np.uint32)
            toff[1:] = np.cumsum([len(t) for t in tb])
            tt = np.frombuffer(b"".join(tb) or b"\0", np.uint8)
            keep += [toff, tt]
            s.titles, s.title_off = tt.ctypes.data, toff.ctypes.data
        if n == 0:
            return np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.int32)
        if R == 0:
            raise ValueError("compress_dense_packed: the arrays have no rows (R = 0)")
        counts = np.zeros(3, np.uint32); nbytes = ctypes.c_uint64(0)
        _lib.check(self.lib.fcz_compress_dense_packed_begin(self.ctx, ctypes.byref(s), ro.ctypes.data, n, R, lay, int(anchor_threshold),
                                                            counts.ctypes.data, ctypes.byref(nbytes)), "fcz_compress_dense_packed_begin")
        off = np.zeros(n + 1, np.uint64); st = np.zeros(n, np.int32); blob = np.zeros(max(int(nbytes.value), 1), np.uint8)
        _lib.check(self.lib.fcz_compress_dense_fetch(self.ctx, off.ctypes.data, st.ctypes.data, blob.ctypes.data), "fcz_compress_dense_fetch")
        return blob[:int(nbytes.value)], off, st

    def decompress_pdb(self, blob: np.ndarray, off: np.ndarray, alt_order: bool = False, nul_terminated: bool = False):
        """FCZ entries -> (list of PDB texts as bytes, per-entry status); decoding and text formatting both on the GPU.
        nul_terminated: every text that decodes ends in the NUL a database record carries (FCZ_PDB_NUL_TERMINATED)"""
        blob = np.ascontiguousarray(blob, np.uint8)
        off = np.ascontiguousarray(off, np.uint64)
        n = len(off) - 1
        text_off = np.zeros(n + 1, np.uint64)
        status = np.zeros(max(n, 1), np.int32)
        _lib.check(self.lib.fcz_decompress_pdb_begin(self.ctx, blob.ctypes.data, off.ctypes.data, n, int(bool(alt_order)) | (0x100 if nul_terminated else 0),
                                                     text_off.ctypes.data, status.ctypes.data), "fcz_decompress_pdb_begin")
        text = np.zeros(int(text_off[-1]), np.uint8)
        _lib.check(self.lib.fcz_decompress_pdb_fetch(self.ctx, text.ctypes.data if len(text) else None), "fcz_decompress_pdb_fetch")
        raw = text.tobytes()
        return [raw[int(text_off[i]):int(text_off[i + 1])] for i in range(n)], status[:n]

    def extract(self, blob: np.ndarray, off: np.ndarray, mode: int = 0, digits: int = 2):
        """FCZ entries -> list of data strings (bytes): pLDDT digits (mode 0) or the amino-acid sequence (mode 1); entries
        that cannot be read give b''"""
        blob = np.ascontiguousarray(blob, np.uint8)
        off = np.ascontiguousarray(off, np.uint64)
        n = len(off) - 1
        data_off = np.zeros(n + 1, np.uint64)
        _lib.check(self.lib.fcz_extract_sizes(blob.ctypes.data, off.ctypes.data, n, int(mode), int(digits), data_off.ctypes.data), "fcz_extract_sizes")
        data = np.zeros(int(data_off[-1]), np.uint8)
        _lib.check(self.lib.fcz_extract(self.ctx, blob.ctypes.data, off.ctypes.data, n, int(mode), int(digits), data_off.ctypes.data,
                                        data.ctypes.data if len(data) else None), "fcz_extract")
        raw = data.tobytes()
        return [raw[int(data_off[i]):int(data_off[i + 1])] for i in range(n)]

    # ---- structure ingest on the device -----------------------------------------------------------
    @staticmethod
    def _pack_files(texts, names):
        """bytes of the files back to back + offsets, base names + offsets, stem lengths (getFileParts: split at the last dot)"""
        file_off = np.zeros(len(texts) + 1, np.uint64)
        file_off[1:] = np.cumsum([len(t) for t in texts])
        text = np.frombuffer(b"".join(texts) or b"\0", np.uint8)
        nb = [n.encode() for n in names]
        name_off = np.zeros(len(nb) + 1, np.uint32)
        name_off[1:] = np.cumsum([len(n) for n in nb])
        name_blob = np.frombuffer(b"".join(nb) or b"\0", np.uint8)
        # byte counts of the ENCODED names (name_blob is UTF-8: a character index would cut a non-ASCII stem short)
        stem_len = np.asarray([n.rfind(b".") if b"." in n else len(n) for n in nb], np.uint32)
        return text, file_off, name_blob, name_off, stem_len

    def ingest_pdb(self, texts, names, anchor_threshold: int = 25, skip_discontinuous: bool = False):
        """PDB texts (bytes) + base names -> (ChainBatch, chain_file, chain_meta, file_status, refused[n, 2]) with every step on
        the GPU (fcz_ingest_pdb_*): what the reference's driver makes of the files before Foldcomp::compress"""
        text, file_off, name_blob, name_off, stem_len = self._pack_files(texts, names)
        counts = np.zeros(5, np.uint32)
        _lib.check(self.lib.fcz_ingest_pdb_begin(self.ctx, text.ctypes.data, file_off.ctypes.data, len(texts), name_blob.ctypes.data,
                                                 name_off.ctypes.data, stem_len.ctypes.data, int(anchor_threshold),
                                                 1 if skip_discontinuous else 0, counts.ctypes.data), "fcz_ingest_pdb_begin")
        C, R, M, TB, NR = (int(v) for v in counts)
        b = ChainBatch(res_off=np.zeros(C + 1, np.uint32), atom_off=np.zeros(R + 1, np.uint32), x=np.zeros(M, np.float32),
                       y=np.zeros(M, np.float32), z=np.zeros(M, np.float32), atom_code=np.zeros(M, np.uint8),
                       res_code=np.zeros(R, np.uint8), bfac_ca=np.zeros(R, np.float32), first_res_index=np.zeros(C, np.int32),
                       first_atom_index=np.zeros(C, np.int32), chain_id=np.zeros(C, np.uint8), titles=np.zeros(max(TB, 1), np.uint8),
                       title_off=np.zeros(C + 1, np.uint32), anchor_threshold=int(anchor_threshold))
        cb = batch_as_c(b)
        chain_file = np.zeros(C, np.uint32); chain_meta = np.zeros(C, np.uint32)
        file_status = np.zeros(len(texts), np.int32); refused = np.zeros((NR, 2), np.uint32)
        _lib.check(self.lib.fcz_ingest_pdb_fetch(self.ctx, ctypes.byref(cb), chain_file.ctypes.data, chain_meta.ctypes.data,
                                                 file_status.ctypes.data, refused.ctypes.data), "fcz_ingest_pdb_fetch")
        b.titles = b.titles[:TB]
        return b, chain_file, chain_meta, file_status, refused

    def compress_pdb(self, texts, names, anchor_threshold: int = 25, skip_discontinuous: bool = False):
        """PDB texts -> FCZ records, parse and codec both on the GPU: dict(blob, off, status, chain_file, chain_meta, file_status,
        refused)"""
        text, file_off, name_blob, name_off, stem_len = self._pack_files(texts, names)
        counts = np.zeros(5, np.uint32); nbytes = ctypes.c_uint64(0)
        _lib.check(self.lib.fcz_compress_pdb_begin(self.ctx, text.ctypes.data, file_off.ctypes.data, len(texts), name_blob.ctypes.data,
                                                   name_off.ctypes.data, stem_len.ctypes.data, int(anchor_threshold),
                                                   1 if skip_discontinuous else 0, counts.ctypes.data, ctypes.byref(nbytes)),
                   "fcz_compress_pdb_begin")
        C, NR = int(counts[0]), int(counts[4])
        off = np.zeros(C + 1, np.uint64); st = np.zeros(C, np.int32); blob = np.zeros(max(int(nbytes.value), 1), np.uint8)
        chain_file = np.zeros(C, np.uint32); chain_meta = np.zeros(C, np.uint32)
        file_status = np.zeros(len(texts), np.int32); refused = np.zeros((NR, 2), np.uint32)
        _lib.check(self.lib.fcz_compress_pdb_fetch(self.ctx, off.ctypes.data, st.ctypes.data, chain_file.ctypes.data, chain_meta.ctypes.data,
                                                   file_status.ctypes.data, refused.ctypes.data, blob.ctypes.data), "fcz_compress_pdb_fetch")
        return dict(blob=blob[:int(nbytes.value)], off=off, status=st, chain_file=chain_file, chain_meta=chain_meta,
                    file_status=file_status, refused=refused, counts=counts)

    def chain_names(self, n_chains: int):
        """names of the chains of the batch the last ingest / compress_pdb / compress_gz call left in the ctx: list of str (mmCIF chain
        names have up to four characters; chain_meta's low byte is only the first)"""
        nm = np.zeros(max(int(n_chains), 1), np.uint32)
        _lib.check(self.lib.fcz_ingest_chain_names_fetch(self.ctx, nm.ctypes.data), "fcz_ingest_chain_names_fetch")
        return [int(v).to_bytes(4, "little").rstrip(b"\0").decode("latin-1") for v in nm[:int(n_chains)]]

    # ---- gzip members on the device ----------------------------------------------------------------
    INFLATE_STATUS = {0: "ok", 1: "header", 2: "block", 3: "code", 4: "size", 5: "input", 6: "check"}

    def inflate(self, members, kind=None):
        """gzip members (bytes each) -> (list of texts, status[n]): fcz_inflate_sizes + fcz_inflate. A member with a non-zero status
        was NOT inflated on the device (the caller's zlib decides about it); its text is returned as blanks of the ISIZE it claims."""
        n = len(members)
        off = np.zeros(n + 1, np.uint64)
        off[1:] = np.cumsum([len(m) for m in members])
        raw = np.frombuffer(b"".join(members) or b"\0", np.uint8)
        kd = None if kind is None else np.ascontiguousarray(kind, np.uint8)
        toff = np.zeros(n + 1, np.uint64)
        _lib.check(self.lib.fcz_inflate_sizes(raw.ctypes.data, off.ctypes.data, n, None if kd is None else kd.ctypes.data, toff.ctypes.data),
                   "fcz_inflate_sizes")
        text = np.zeros(max(int(toff[n]), 1), np.uint8); st = np.zeros(n, np.int32)
        _lib.check(self.lib.fcz_inflate(self.ctx, raw.ctypes.data, off.ctypes.data, n, None if kd is None else kd.ctypes.data, toff.ctypes.data,
                                        text.ctypes.data, st.ctypes.data), "fcz_inflate")
        tb = text.tobytes()
        return [tb[int(toff[i]):int(toff[i + 1])] for i in range(n)], st

    def compress_gz(self, files, names, is_gz=None, anchor_threshold: int = 25, skip_discontinuous: bool = False):
        """Structure files as they lie on disk (gzip members where is_gz, by default where the name ends in .gz) -> FCZ records:
        inflate, parse and codec on the GPU. Same dict as compress_pdb; file_status 5 = the member is left to the caller's zlib."""
        data, file_off, name_blob, name_off, stem_len = self._pack_files(files, names)
        gz = np.asarray([n.endswith(".gz") for n in names] if is_gz is None else is_gz, np.uint8)
        counts = np.zeros(5, np.uint32); nbytes = ctypes.c_uint64(0)
        _lib.check(self.lib.fcz_compress_gz_begin(self.ctx, data.ctypes.data, file_off.ctypes.data, len(files), gz.ctypes.data, name_blob.ctypes.data,
                                                  name_off.ctypes.data, stem_len.ctypes.data, int(anchor_threshold),
                                                  1 if skip_discontinuous else 0, counts.ctypes.data, ctypes.byref(nbytes)),
                   "fcz_compress_gz_begin")
        C, NR = int(counts[0]), int(counts[4])
        off = np.zeros(C + 1, np.uint64); st = np.zeros(C, np.int32); blob = np.zeros(max(int(nbytes.value), 1), np.uint8)
        chain_file = np.zeros(C, np.uint32); chain_meta = np.zeros(C, np.uint32)
        file_status = np.zeros(len(files), np.int32); refused = np.zeros((NR, 2), np.uint32)
        _lib.check(self.lib.fcz_compress_pdb_fetch(self.ctx, off.ctypes.data, st.ctypes.data, chain_file.ctypes.data, chain_meta.ctypes.data,
                                                   file_status.ctypes.data, refused.ctypes.data, blob.ctypes.data), "fcz_compress_pdb_fetch")
        return dict(blob=blob[:int(nbytes.value)], off=off, status=st, chain_file=chain_file, chain_meta=chain_meta,
                    file_status=file_status, refused=refused, counts=counts)

    # ---- timing ---------------------------------------------------------------------------------
    def enable_timing(self, on: bool = True):
        self.lib.fcz_ctx_enable_timing(self.ctx, int(on))

    def reset_timing(self):
        self.lib.fcz_ctx_reset_timing(self.ctx)

    def kernel_time(self, name: str):
        ms = ctypes.c_double(0); n = ctypes.c_uint64(0)
        self.lib.fcz_ctx_kernel_time(self.ctx, name.encode(), ctypes.byref(ms), ctypes.byref(n))
        return ms.value, n.value

    # ---- numerics self-test hook ------------------------------------------------------------------
    def selftest_math(self, mode: int, start_bits: int, stride: int, count: int) -> np.ndarray:
        out = np.zeros(count, np.float32)
        _lib.check(self.lib.fcz_selftest_math(self.ctx, mode, start_bits, stride, count, out.ctypes.data), "fcz_selftest_math")
        return out
