"""FCZ records -> dense padded model-input tensors that never leave the GPU.

    decode_tensors(entries) -> dict(pos [n, L, A, 3] float32, mask [n, L, A] bool, aatype [n, L] uint8, plddt [n, L] float32,
                                    res_index [n, L] int32, length [n] int32, names list[str])

What a structure model's data loader wants from a Foldcomp database (atom37 / atom14 coordinates with a mask, residue types,
pLDDT), without the PDB text `foldcomp.decompress` returns and without a host copy of the result: the records go up once, torch
allocates the outputs, and fcz_decompress_sizes_dev / fcz_decompress_batch_dev / fcz_dense_dev (include/fcz_hip.h) fill them in
place. The coordinates are the decoder's float32 values bit for bit (the text keeps three decimals).

torch is imported inside the functions only: `import foldcomp` does not touch it.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np

from . import _lib, api, fczfile
from .codec import Codec, dense_layout
from .structure import CAtomsOut, CDenseOut

__all__ = ["decode_tensors"]


def _torch_device(device):
    """torch with its device initialised (before the codec's ctx exists: torch's wheel bundles its own HIP runtime, which finds the
    GPU only when it initialises ahead of the system runtime libfcz_hip.so links) -> (torch, torch.device)"""
    try:
        import torch
    except ImportError as e:
        raise api.error(f"decode_tensors needs PyTorch (ROCm build): {e}") from None
    dev = torch.device(device)
    if dev.type != "cuda":
        raise api.error(f"decode_tensors fills tensors on a GPU: device must be 'cuda:<i>', not {device!r}")
    if not torch.cuda.is_available():
        raise api.error("decode_tensors: torch cannot see a HIP device (torch.cuda.is_available() is False); "
                        "the dense tensors are built on the GPU and there is no CPU fallback")
    torch.cuda.init()
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if dev.index >= torch.cuda.device_count():
        raise api.error(f"decode_tensors: no such device {device!r} ({torch.cuda.device_count()} visible)")
    return torch, dev


def _title(entry: bytes) -> str:
    try:
        return fczfile.parse(entry).title
    except fczfile.FczFormatError:
        return ""


def decode_tensors(entries: Sequence[bytes], *, layout="atom37", max_len: Optional[int] = None, device="cuda:0",
                   codec: Optional[Codec] = None) -> dict:
    """[fcz, ...] -> dict of torch tensors on `device` plus `names` (the records' titles, a Python list).

    layout: "atom37" (A = 37, AlphaFold / OpenFold atom order, the chain's OXT in slot 36 of its last residue), "atom14" (A = 14,
    the residue's canonical order) or "backbone4" (N, CA, C, O). L = max_len, or the longest entry of the batch; an entry longer
    than L is cropped to its first L residues and `length` still reports its full size. pos is 0 where mask is False; aatype is
    0 .. 19 in the order A R N D C Q E G H I L K M F P S T W Y V, 20 for anything else and for padding; plddt and res_index are 0
    in the padding. An entry that does not decode has length 0, name "" when it has no readable header, and padding only.
    length is int32 (torch has no arithmetic on unsigned 32-bit integers).

    Ordering against torch: the uploads and allocations are made on torch's current stream, which is synchronised before the
    codec's calls; the codec works on its own stream, which is synchronised before the tensors are returned. No output byte
    visits the host.
    """
    torch, dev = _torch_device(device)
    c = codec or api.default_codec()
    if int(c.device) != dev.index:
        raise api.error(f"decode_tensors: the codec works on device {c.device}, the tensors were asked for on {dev}")
    lay = dense_layout(layout)
    A = c.lib.fcz_dense_width(lay)
    if max_len is not None and int(max_len) < 1:
        raise ValueError("max_len must be at least 1")
    entries = [bytes(e) for e in entries]
    n = len(entries)
    names = [_title(e) for e in entries]

    def result(L, pos, mask, aatype, plddt, res_index, length):
        return dict(pos=pos, mask=mask.view(torch.bool), aatype=aatype, plddt=plddt, res_index=res_index, length=length, names=names)

    def alloc(L):
        return (torch.empty((n, L, A, 3), dtype=torch.float32, device=dev), torch.empty((n, L, A), dtype=torch.uint8, device=dev),
                torch.empty((n, L), dtype=torch.uint8, device=dev), torch.empty((n, L), dtype=torch.float32, device=dev),
                torch.empty((n, L), dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))

    if n == 0:
        L = int(max_len or 0)
        return result(L, *alloc(L))
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(e) for e in entries])
    # (16 spare bytes behind the last record: the decoder's dword loads of a record's last bytes stay inside the allocation)
    blob_t = torch.from_numpy(np.frombuffer(b"".join(entries) + bytes(16), np.uint8).copy()).to(dev)
    off_t = torch.from_numpy(off.view(np.int64)).to(dev)
    res_off_t = torch.empty(n + 1, dtype=torch.int32, device=dev)
    atom_off_t = torch.empty(n + 1, dtype=torch.int32, device=dev)
    torch.cuda.current_stream(dev).synchronize()
    R, M = ctypes.c_uint32(0), ctypes.c_uint32(0)
    _lib.check(c.lib.fcz_decompress_sizes_dev(c.ctx, blob_t.data_ptr(), off_t.data_ptr(), n, res_off_t.data_ptr(), atom_off_t.data_ptr(),
                                              ctypes.byref(R), ctypes.byref(M)), "fcz_decompress_sizes_dev")
    if max_len is None:
        ro = res_off_t.cpu().numpy().view(np.uint32).astype(np.int64)      # n + 1 offsets: the only words that come back
        L = int(np.diff(ro).max())
    else:
        L = int(max_len)
    out = alloc(L)
    if L == 0:                                                             # nothing decodes and no width was asked for
        return result(L, *out)
    x, y, z = (torch.empty(max(M.value, 1), dtype=torch.float32, device=dev) for _ in range(3))
    bfac = torch.empty(max(R.value, 1), dtype=torch.float32, device=dev)
    res_code = torch.empty(max(R.value, 1), dtype=torch.uint8, device=dev)
    atoms = CAtomsOut(x.data_ptr(), y.data_ptr(), z.data_ptr(), bfac.data_ptr(), res_code.data_ptr(), None)
    dense = CDenseOut(*(t.data_ptr() for t in out))
    torch.cuda.current_stream(dev).synchronize()
    if R.value:
        _lib.check(c.lib.fcz_decompress_batch_dev(c.ctx, blob_t.data_ptr(), off_t.data_ptr(), n, res_off_t.data_ptr(), atom_off_t.data_ptr(),
                                                  0, ctypes.byref(atoms)), "fcz_decompress_batch_dev")
    _lib.check(c.lib.fcz_dense_dev(c.ctx, blob_t.data_ptr(), off_t.data_ptr(), n, res_off_t.data_ptr(), atom_off_t.data_ptr(),
                                   ctypes.byref(atoms), 0, lay, L, ctypes.byref(dense)), "fcz_dense_dev")
    c.synchronize()
    return result(L, *out)
