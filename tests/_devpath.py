"""Shared helpers: the device-pointer entry points of the C-ABI (fcz_*_dev) driven from host ChainBatch / record lists. The host entry
points of Codec stage through the ctx and compute sizes on the host; these go the way bench.py goes: device sizes pass (the
device scans, the sizes memo), then the batch call on the caller's own device arrays."""
import ctypes

import numpy as np

from foldcomp_amd import _lib
from foldcomp_amd.structure import CAtomsOut, CChainBatch, ChainBatch

_FIELDS = ("res_off", "atom_off", "x", "y", "z", "atom_code", "res_code", "bfac_ca", "first_res_index", "first_atom_index",
           "chain_id", "titles", "title_off")
_SIGNED = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


def to_dev(a, dev="cuda:0"):
    """numpy array -> device tensor of the same bytes (torch has no unsigned 32/64-bit arithmetic: viewed as signed)"""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype in _SIGNED:
        a = a.view(_SIGNED[a.dtype])
    if a.size == 0:
        return torch.zeros(1, dtype=torch.from_numpy(np.zeros(1, a.dtype)).dtype, device=dev)
    return torch.from_numpy(a).to(dev)


FILL = 0xA5          # the byte every guarded output holds before the call
GUARD = 256          # bytes of FILL on both sides of an output that must survive (a multiple of 16: the outputs stay aligned)


class HostGuarded:
    """host outputs of a host-pointer entry point, {name: (dtype, shape)} in the call's order: 0xA5 everywhere, `guard` bytes in
    front of and behind each, which must survive the call"""

    def __init__(self, spec, guard=GUARD):
        self.spec = {k: (np.dtype(d), tuple(shape)) for k, (d, shape) in spec.items()}
        self.guard = guard
        self.raw = {k: self._filled(2 * guard + d.itemsize * int(np.prod(shape))) for k, (d, shape) in self.spec.items()}

    def _filled(self, nbytes):
        return np.full(nbytes, FILL, np.uint8)

    def _address(self, buf):
        return buf.ctypes.data

    def _bytes(self, buf):
        """the buffer as a host uint8 array"""
        return buf

    def ptr(self, k):
        return self._address(self.raw[k]) + self.guard

    def ptrs(self):
        return [self.ptr(k) for k in self.spec]

    def fetch(self, k):
        a, g = self._bytes(self.raw[k]), self.guard
        assert (a[:g] == FILL).all() and (a[len(a) - g:] == FILL).all(), f"guard bytes of {k} overwritten"
        d, shape = self.spec[k]
        return a[g:len(a) - g].copy().view(d).reshape(shape)

    def all(self):
        return [self.fetch(k) for k in self.spec]

    def untouched(self):
        return all(bool((self._bytes(a) == FILL).all()) for a in self.raw.values())


class DevGuarded(HostGuarded):
    """the same for the device outputs of a device-pointer entry point: a byte the call leaves unwritten stays 0xA5 and fails the
    comparison that follows (device: for the CPU test of this class, nothing else passes it)"""

    def __init__(self, spec, guard=GUARD, device="cuda:0"):
        self.device = device
        super().__init__(spec, guard)

    def _filled(self, nbytes):
        import torch
        return torch.full((nbytes,), FILL, dtype=torch.uint8, device=self.device)

    def _address(self, buf):
        return buf.data_ptr()

    def _bytes(self, buf):
        return buf.cpu().numpy()


def host_ptr(a):
    """address of a C-contiguous host array the caller keeps alive, None for None"""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data


def dev_batch(b: ChainBatch, dev="cuda:0"):
    """-> (fcz_chain_batch of device pointers, the tensors that own them)"""
    t = {k: to_dev(getattr(b, k), dev) for k in _FIELDS}
    s = CChainBatch()
    s.n_chains, s.n_residues, s.n_atoms = b.n_chains, b.n_residues, b.n_atoms
    s.anchor_threshold = int(b.anchor_threshold)
    for k in _FIELDS:
        setattr(s, k, t[k].data_ptr())
    return s, t


def compress_dev(codec, b: ChainBatch, dev="cuda:0"):
    """fcz_compress_sizes_dev + fcz_compress_batch_dev -> (blob uint8, off uint64[C+1], status int32[C]) on the host"""
    import torch
    cb, keep = dev_batch(b, dev)
    C = b.n_chains
    off_t = torch.zeros(C + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    _lib.check(codec.lib.fcz_compress_sizes_dev(codec.ctx, ctypes.byref(cb), off_t.data_ptr()), "fcz_compress_sizes_dev")
    codec.synchronize()
    off = off_t.cpu().numpy().view(np.uint64)
    blob_t = torch.zeros(max(int(off[-1]), 1), dtype=torch.uint8, device=dev)
    st_t = torch.zeros(max(C, 1), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rc = codec.lib.fcz_compress_batch_dev(codec.ctx, ctypes.byref(cb), off_t.data_ptr(), blob_t.data_ptr(), st_t.data_ptr())
    _lib.check(rc, "fcz_compress_batch_dev")
    codec.synchronize()
    del keep
    return blob_t.cpu().numpy()[:int(off[-1])], off, st_t.cpu().numpy()[:C]


class DevRecords:
    """FCZ records resident on the device with every array a decompress call needs"""

    def __init__(self, blob, off, dev="cuda:0"):
        import torch
        self.n = len(off) - 1
        self.blob_t = to_dev(np.concatenate([np.ascontiguousarray(blob, np.uint8), np.zeros(16, np.uint8)]), dev)
        self.off_t = to_dev(np.ascontiguousarray(off, np.uint64), dev)
        self.res_off_t = torch.zeros(self.n + 1, dtype=torch.int32, device=dev)
        self.atom_off_t = torch.zeros(self.n + 1, dtype=torch.int32, device=dev)
        self.dev = dev
        torch.cuda.synchronize()

    def sizes(self, codec):
        """fcz_decompress_sizes_dev -> (res_off, atom_off) on the host"""
        tr, ta = ctypes.c_uint32(0), ctypes.c_uint32(0)
        _lib.check(codec.lib.fcz_decompress_sizes_dev(codec.ctx, self.blob_t.data_ptr(), self.off_t.data_ptr(), self.n, self.res_off_t.data_ptr(),
                                                      self.atom_off_t.data_ptr(), ctypes.byref(tr), ctypes.byref(ta)), "fcz_decompress_sizes_dev")
        ro = self.res_off_t.cpu().numpy().view(np.uint32); ao = self.atom_off_t.cpu().numpy().view(np.uint32)
        assert (tr.value, ta.value) == (int(ro[-1]), int(ao[-1]))
        return ro, ao

    def batch(self, codec, alt_order=False, host=True):
        """fcz_decompress_batch_dev on the offsets the arrays hold now -> dict of host arrays like Codec.decompress_batch's (host=False:
        the device tensors, cut to size)"""
        import torch
        R = int(self.res_off_t[-1]) & 0xFFFFFFFF; M = int(self.atom_off_t[-1]) & 0xFFFFFFFF
        o = {k: torch.zeros(max(M, 1), dtype=torch.float32, device=self.dev) for k in ("x", "y", "z")}
        o["bfac_res"] = torch.zeros(max(R, 1), dtype=torch.float32, device=self.dev)
        o["res_code"] = torch.zeros(max(R, 1), dtype=torch.uint8, device=self.dev)
        o["atom_code"] = torch.zeros(max(M, 1), dtype=torch.uint8, device=self.dev)
        out = CAtomsOut(*(o[k].data_ptr() for k in ("x", "y", "z", "bfac_res", "res_code", "atom_code")))
        torch.cuda.synchronize()
        _lib.check(codec.lib.fcz_decompress_batch_dev(codec.ctx, self.blob_t.data_ptr(), self.off_t.data_ptr(), self.n, self.res_off_t.data_ptr(),
                                                      self.atom_off_t.data_ptr(), int(alt_order), ctypes.byref(out)), "fcz_decompress_batch_dev")
        codec.synchronize()
        if not host:
            return {k: o[k][:(R if k in ("bfac_res", "res_code") else M)] for k in o}
        d = {k: o[k].cpu().numpy()[:(R if k in ("bfac_res", "res_code") else M)] for k in o}
        d["res_off"] = self.res_off_t.cpu().numpy().view(np.uint32); d["atom_off"] = self.atom_off_t.cpu().numpy().view(np.uint32)
        return d

    def decompress(self, codec, alt_order=False):
        self.sizes(codec)
        return self.batch(codec, alt_order)
