"""FCZ records <-> dense padded or packed model-input tensors that never leave the GPU.

    decode_tensors(entries) -> dict(pos [n, L, A, 3] float32, mask [n, L, A] bool, aatype [n, L] uint8, plddt [n, L] float32,
                                    res_index [n, L] int32, length [n] int32, names list[str])
    decode_tensors(entries, packed=True) -> dict(pos [R, A, 3], mask [R, A], aatype [R], plddt [R], res_index [R], chain_index [R],
                                    cu_seqlens [n + 1] int32, length [n] int32, names, max_seqlen int): no padding, no crop
    encode_tensors(either dict, or the tensors as keywords) -> [fcz, ...]
    decode_angles(entries) -> dict(angles [n, L, 10] float32 degrees, angle_mask [n, L, 10] bool, aatype [n, L] uint8, length [n] int32,
                                   names list[str]); packed=True: angles [R, 10], angle_mask [R, 10], aatype [R], cu_seqlens, max_seqlen
    decode_tensors / decode_angles(entries, max_len=L, crop="start" | "center" | "random" | starts [n]) -> the same padded dicts
                                   with row l of entry e = its residue crop_start[e] + l, plus crop_start [n] int32
    crop_starts(length, L, how, generator) -> the starts of such a crop, on the device the lengths lie on
    neighbor_graph(either dict, or the tensors as keywords, k=48, atom="CA") -> dict(nbr_index [.., k] int32, nbr_dist [.., k] float32):
                                   the k nearest CA / CB sites of every residue inside its chain; decode_tensors(neighbors=k) adds them
    lddt(pred, true, atom="CA", cutoff=15.0) -> dict(lddt [..] float32, lddt_pairs, lddt_hits int32, lddt_chain [n] float32): the per-residue
                                   lDDT of predicted coordinates against a decoded batch, and its chain mean
    smooth_lddt(pred, true, atom="CA", cutoff=15.0) -> dict(lddt_soft [..] float32, lddt_pairs int32, lddt_soft_chain [n] float32, loss):
                                   the smooth lDDT of AlphaFold 3 on the same pairs, a loss: differentiable with respect to pred's
                                   pos, with a fused backward on the GPU
    fape(pred, true, atom="CA", clamp=10.0, scale=10.0) -> dict(fape_frame [..] float32, fape_points int32, frame_mask bool, fape_chain [n]
                                   float32, loss): the backbone FAPE of AlphaFold 2 (Algorithm 28) of predicted frames and points against
                                   the truth's, a loss: differentiable with respect to pred's rot / trans / pos, with a fused backward
    fape_atoms(pred, true, clamp=10.0, scale=10.0, rename="lddt_atoms") -> dict(fape_frame [.., 8] float32, fape_points int32, frame_mask
                                   bool, swapped [..] bool, fape_chain [n] float32, loss): the all-atom FAPE of AlphaFold 2, the eight
                                   rigid groups of every residue against every atom of the chain with the truth renamed first, a loss
                                   with a fused backward; rigid_frames_torch(pos, mask, aatype) builds the eight groups differentiably
    lddt_atoms(pred, true, swaps="alphafold", per_atom=False) -> dict(lddt, lddt_pairs, lddt_hits, swapped [..] bool, lddt_chain [n]
                                   float64, atom_pairs / atom_hits [.., A]): the all-atom lDDT of every residue after the symmetric
                                   side-chain namings of the truth have been resolved towards the prediction
    superpose(pred, true, atom="CA", apply=False) -> dict(rot [n, 3, 3], trans [n, 3], rmsd [n], sites [n], dev [..], gdt_counts [n, 5],
                                   gdt_ts, gdt_ha, tm [n]): the least-squares superposition of every chain of pred onto true;
                                   apply=True adds pos_aligned; apply_transform(pos, rot, trans, batch) is that step alone
    tm_score(pred, true, atom="CA", apply=False, iterations=20, levels=None) -> the same dict at the superposition that MAXIMISES the
                                   TM-score over a seeded iterative search, plus seed [n] and selected [n]
    gdt(pred, true, atom="CA", iterations=20, levels=None, runs="all") -> dict(gdt_counts [n, 5], gdt_ts, gdt_ha, sites [n], rot
                                   [n, 5, 3, 3], trans [n, 5, 3], seed, run, selected [n, 5], within [..] uint8): the MAXIMISED GDT, per
                                   cutoff the largest count over the same seeds searched with six cut schedules, and its superposition
    backbone_hbonds(either dict, or the tensors as keywords) -> dict(hbond_acc_index, hbond_acc_energy, hbond_don_index, hbond_don_energy
                                   [.., 2]): DSSP's four H-bond columns, the two best acceptors and donors of every residue
    secondary_structure(either dict, or the tensors as keywords) -> dict(ss [..] uint8, ss_mask [..] bool, the four tables): the DSSP
                                   label of every residue (foldcomp.SS_CLASSES); decode_tensors(secondary_structure=True) adds ss / ss_mask
    solvent_accessibility(either dict, or the tensors as keywords) -> dict(sasa [..] float32, rsa, sasa_mask bool, sasa_points [.., A] int16):
                                   the Shrake-Rupley accessible surface of every residue; decode_tensors(sasa=True) adds sasa / rsa / sasa_mask
    violation_loss(pred, true, tolerance=1.5, link_factor=12.0) -> dict(clash_loss [.., A] float32, link_loss [.., 3], clash_chain [n],
                                   bond_chain, angle_chain, violation_chain, loss): the clash energy and the peptide-link penalties of
                                   violations' pairs and links as a LOSS, differentiable with a fused backward on the GPU
    violations(either dict, or the tensors as keywords) -> dict(clash_atom [.., A] uint8, clash_count, clash_depth, clash_partner, viol_mask,
                                   link_mask, link_length, link_cos [.., 2], link_violation [..], chain_counts [n, 4] int64): steric clashes
                                   between residues and broken peptide links; decode_tensors(violations=True) adds clash_count /
                                   link_violation / viol_mask
    rigid_frames(either dict, or the tensors as keywords, groups="backbone" | "all") -> dict(rot [.., 3, 3], trans [.., 3], frame_mask):
                                   every residue's backbone frame, or the eight rigid groups; decode_tensors(frames=...) adds them

What a structure model's data loader wants from a Foldcomp database (atom37 / atom14 coordinates with a mask, residue types,
pLDDT), without the PDB text `foldcomp.decompress` returns and without a host copy of the result: the records go up once, torch
allocates the outputs, and fcz_decompress_sizes_dev / fcz_decompress_batch_dev / fcz_dense_dev (include/fcz_hip.h) fill them in
place. The coordinates are the decoder's float32 values bit for bit (the text keeps three decimals). The way back
(fcz_compress_dense_begin_dev / _fetch_dev) gathers the masked atoms into the codec's flat batch and compresses it where the tensors
lie: only the records and their offsets come to the host.

torch is imported inside the functions only: `import foldcomp` does not touch it.
"""
from __future__ import annotations

import ctypes
from typing import Callable, NamedTuple, Optional, Sequence

import numpy as np

from . import _lib, api, fczfile
from ._aa_tables import RES1
from .codec import ANGLE_COLUMNS, WIDTH_LAYOUTS, Codec, dense_layout
from .structure import CAtomsOut, CDenseIn, CDenseOut, CLddtAtomsOut, CPackedOut, CSuperposeOut, CTmScoreOut, CGdtOut, CViolationsOut, CChainSet, CTmAlignOut, CTmAlignParams, TM_ALIGN_OUTPUTS

__all__ = ["decode_tensors", "encode_tensors", "decode_angles", "crop_starts", "neighbor_graph", "rigid_frames", "lddt", "smooth_lddt", "fape", "fape_atoms", "lddt_atoms", "superpose", "tm_score", "gdt", "tm_align", "apply_transform",
           "backbone_hbonds", "secondary_structure", "solvent_accessibility", "violations", "violation_loss"]


def crop_starts(length, L: int, how, generator=None):
    """first kept residue of every entry for a window of L rows -> int32 tensor [n] on the device of `length` (torch tensor [n] of
    residue counts, any device, `cpu` included). Pure: no codec, no host copy of a device tensor.

    how: "start": 0; "center": max(len - L, 0) // 2; "random": uniform over the integers 0 .. max(len - L, 0), drawn from
    `generator` (a torch.Generator on any device; None: torch's default one of the lengths' device) -- an entry no longer than L
    starts at 0; or the starts themselves, an integer tensor / array / sequence [n]: a negative one is a ValueError where the
    values lie on the host, and values on a device are clamped to 0 .. 2^31 - 1 unseen (a start at or behind the entry's length
    gives padding only, so the upper clamp changes nothing)."""
    import torch
    n = int(length.shape[0])
    L = int(L)
    if L < 1:
        raise ValueError("max_len must be at least 1")
    if not isinstance(how, str):
        if isinstance(how, torch.Tensor):
            st, on_host, integers = how, how.device.type == "cpu", not (how.dtype.is_floating_point or how.dtype.is_complex or how.dtype == torch.bool)
        else:
            a = np.asarray(how)
            integers = a.dtype.kind in "iu"
            st, on_host = torch.from_numpy(np.minimum(a, 2 ** 31 - 1).astype(np.int64) if integers else np.zeros(a.shape)), True
        if tuple(st.shape) != (n,) or not integers:
            raise ValueError(f"crop must be {n} integer starts, one per entry, not {getattr(how, 'dtype', type(how).__name__)} {tuple(st.shape)}")
        if on_host and n and bool((st < 0).any()):
            raise ValueError("crop starts must not be negative")
        return st.to(length.device).clamp(0, 2 ** 31 - 1).to(torch.int32).contiguous()
    if how not in api.CROP_MODES:
        raise ValueError(f"crop must be one of {api.CROP_MODES} or per-entry starts [n], not {how!r}")
    span = (length.to(torch.int64) - L).clamp_(min=0)                       # the last start that keeps the window inside the entry
    if how == "start":
        st = torch.zeros_like(span)
    elif how == "center":
        st = span // 2
    else:
        gdev = generator.device if generator is not None else length.device
        u = torch.rand(n, generator=generator, dtype=torch.float64, device=gdev).to(length.device)
        st = torch.minimum((u * (span + 1).to(torch.float64)).floor().to(torch.int64), span)   # (u < 1: the minimum guards the rounding alone)
    return st.to(torch.int32).contiguous()


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


def _upload_and_size(c, torch, dev, entries):
    """records -> (blob, off, res_off, atom_off) tensors on dev with fcz_decompress_sizes_dev run over them, and its totals R, M"""
    n = len(entries)
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
    return blob_t, off_t, res_off_t, atom_off_t, int(R.value), int(M.value)


def _angles_into(c, torch, dev, n, blob_t, off_t, res_off_t, L, R=None, start_t=None, aatype=False):
    """the angle tensors of a sized batch (fcz_angles_dev, or fcz_angles_packed_dev when R is given), enqueued on the codec's stream:
    the caller synchronises. It reads the records and res_off only, and leaves the sizes memo to the decode that may follow.
    Padded, with start_t (int32 [n] on dev) or aatype=True: fcz_angles_window_dev, the dict then holds `aatype` [n, L] too."""
    shape = (R, len(ANGLE_COLUMNS)) if R is not None else (n, L, len(ANGLE_COLUMNS))
    ang = torch.empty(shape, dtype=torch.float32, device=dev)
    msk = torch.empty(shape, dtype=torch.uint8, device=dev)
    if R is None and (start_t is not None or aatype):
        aa = torch.full((n, L), 20, dtype=torch.uint8, device=dev) if aatype else None
        if ang.numel():
            torch.cuda.current_stream(dev).synchronize()
            _lib.check(c.lib.fcz_angles_window_dev(c.ctx, blob_t.data_ptr(), off_t.data_ptr(), n, res_off_t.data_ptr(), L,
                                                   _ptr(start_t), ang.data_ptr(), msk.data_ptr(), _ptr(aa)), "fcz_angles_window_dev")
        d = dict(angles=ang, angle_mask=msk.view(torch.bool))
        return dict(d, aatype=aa) if aatype else d
    if ang.numel():
        torch.cuda.current_stream(dev).synchronize()
        if R is not None:
            _lib.check(c.lib.fcz_angles_packed_dev(c.ctx, blob_t.data_ptr(), off_t.data_ptr(), n, res_off_t.data_ptr(), ang.data_ptr(), msk.data_ptr()),
                       "fcz_angles_packed_dev")
        else:
            _lib.check(c.lib.fcz_angles_dev(c.ctx, blob_t.data_ptr(), off_t.data_ptr(), n, res_off_t.data_ptr(), L, ang.data_ptr(), msk.data_ptr()),
                       "fcz_angles_dev")
    return dict(angles=ang, angle_mask=msk.view(torch.bool))


def _aatype_rows(entry: bytes, n_res: int) -> np.ndarray:
    """aatype of the first n_res residues of a record that decodes, from its bytes: min(residue code, 20) with the decoder's codes
    (residue 0: header.firstResidue)"""
    rec = fczfile.parse(entry)
    rc = rec.res_codes[:n_res].astype(np.uint8)
    if n_res:
        rc[0] = RES1.index(rec.first_residue) if rec.first_residue in RES1 else 23
    return np.minimum(rc, 20).astype(np.uint8)


def _entry_lengths(res_off_t):
    """residue counts [n] int32 on the device: the diff of the res_off that is there already (uint32 bits; a count fits 16)"""
    return res_off_t[1:] - res_off_t[:-1]


def decode_angles(entries: Sequence[bytes], *, max_len: Optional[int] = None, packed: bool = False, device="cuda:0",
                  codec: Optional[Codec] = None, crop=None, generator=None) -> dict:
    """[fcz, ...] -> the records' internal coordinates as torch tensors on `device`, without reconstructing an atom: the sizes pass
    and fcz_angles_dev only (include/fcz_hip.h).

    angles [n, L, 10] float32 in degrees, columns foldcomp.ANGLE_COLUMNS (phi, psi, omega, the bond angles N-CA-C / CA-C-N(+1) /
    C-N(+1)-CA(+1), chi1 .. chi4); angle_mask [n, L, 10] bool, False where the record holds no such value (phi and N-CA-C of the
    first residue, psi / omega and the two bond angles behind the last, a chi the residue type does not have, padding), and the
    angle is 0 there. omega in row l is the peptide bond BEHIND residue l. The values are the floats the decoder places atoms with.
    aatype [n, L] uint8 and length [n] int32 as decode_tensors gives them, names the titles. L = max_len, or the longest entry; a
    longer entry is cropped. packed=True: angles [R, 10], angle_mask [R, 10], aatype [R], cu_seqlens [n + 1] int32 and max_seqlen;
    no padding, no crop, no max_len. An entry that does not decode has length 0 and no value. Argument errors and the ordering
    against torch are decode_tensors'.

    crop (with max_len=L, not with packed): "start", "center", "random" (drawn from `generator`, a torch.Generator) or the starts
    [n] themselves, as crop_starts takes them: row l of entry e then holds its residue crop_start[e] + l, bit for bit the row the
    uncropped call gives it (row 0 of a window that starts inside the chain has phi and N-CA-C), and the dict gains crop_start
    [n] int32. The starts are computed on the device from res_off.

    Host work: the angles never visit the host. In the padded form aatype is written by the angle kernel itself
    (fcz_angles_window_dev) and only `names` is read from the record headers in Python. The packed form still reads aatype from
    the record bytes here, one record at a time (one byte per residue, uploaded as one array): for large packed batches that
    loop, not the kernel, is what the call costs, and decode_tensors(packed=True, angles=True) takes aatype from the decode."""
    api.check_crop(crop, max_len, packed)
    torch, dev = _torch_device(device)
    c = codec or api.default_codec()
    if int(c.device) != dev.index:
        raise api.error(f"decode_angles: the codec works on device {c.device}, the tensors were asked for on {dev}")
    if packed and max_len is not None:
        raise ValueError("max_len crops to a common length; the packed form keeps every residue (packed=True takes no max_len)")
    if max_len is not None and int(max_len) < 1:
        raise ValueError("max_len must be at least 1")
    entries = [bytes(e) for e in entries]
    n = len(entries)
    names = [_title(e) for e in entries]
    W = len(ANGLE_COLUMNS)
    if n == 0:
        length = torch.zeros(0, dtype=torch.int32, device=dev)
        if packed:
            return dict(angles=torch.empty((0, W), dtype=torch.float32, device=dev), angle_mask=torch.empty((0, W), dtype=torch.bool, device=dev),
                        aatype=torch.empty(0, dtype=torch.uint8, device=dev), length=length, names=names,
                        cu_seqlens=torch.zeros(1, dtype=torch.int32, device=dev), max_seqlen=0)
        L = int(max_len or 0)
        d = dict(angles=torch.empty((0, L, W), dtype=torch.float32, device=dev), angle_mask=torch.empty((0, L, W), dtype=torch.bool, device=dev),
                 aatype=torch.empty((0, L), dtype=torch.uint8, device=dev), length=length, names=names)
        return d if crop is None else dict(d, crop_start=crop_starts(length, L, crop, generator))
    blob_t, off_t, res_off_t, _, R, _ = _upload_and_size(c, torch, dev, entries)
    if packed and R > 2 ** 31 - 1:
        raise api.error(f"decode_angles: {R} residues do not fit the int32 cu_seqlens; split the batch")
    if not packed:
        length = _entry_lengths(res_off_t)
        L = int(length.max()) if max_len is None else int(max_len)         # (no max_len: one word comes back)
        start_t = None if crop is None else crop_starts(length, L, crop, generator)
        d = _angles_into(c, torch, dev, n, blob_t, off_t, res_off_t, L, start_t=start_t, aatype=True)
        d.update(length=length, names=names)
        if crop is not None:
            d["crop_start"] = start_t
        c.synchronize()
        return d
    ro = res_off_t.cpu().numpy().view(np.uint32).astype(np.int64)          # n + 1 offsets: the only words that come back
    lens = np.diff(ro)
    aatype = np.zeros(R, np.uint8)
    for e, k, r0 in zip(entries, lens, ro):
        aatype[r0:r0 + k] = _aatype_rows(e, int(k)) if k else 0
    d = _angles_into(c, torch, dev, n, blob_t, off_t, res_off_t, 0, R)
    d.update(cu_seqlens=res_off_t, max_seqlen=int(lens.max()))
    d.update(aatype=torch.from_numpy(aatype).to(dev), length=torch.from_numpy(lens.astype(np.int32)).to(dev), names=names)
    c.synchronize()
    return d


def decode_tensors(entries: Sequence[bytes], *, layout="atom37", max_len: Optional[int] = None, device="cuda:0",
                   codec: Optional[Codec] = None, packed: bool = False, angles: bool = False, crop=None, generator=None,
                   neighbors: Optional[int] = None, neighbor_atom="CA", frames: Optional[str] = None,
                   secondary_structure: bool = False, sasa: bool = False, violations: bool = False) -> dict:
    """[fcz, ...] -> dict of torch tensors on `device` plus `names` (the records' titles, a Python list).

    layout: "atom37" (A = 37, AlphaFold / OpenFold atom order, the chain's OXT in slot 36 of its last residue), "atom14" (A = 14,
    the residue's canonical order) or "backbone4" (N, CA, C, O). L = max_len, or the longest entry of the batch; an entry longer
    than L is cropped to its first L residues and `length` still reports its full size. pos is 0 where mask is False; aatype is
    0 .. 19 in the order A R N D C Q E G H I L K M F P S T W Y V, 20 for anything else and for padding; plddt and res_index are 0
    in the padding. An entry that does not decode has length 0, name "" when it has no readable header, and padding only.
    length is int32 (torch has no arithmetic on unsigned 32-bit integers).

    packed=True: the rows of all entries back to back instead (fcz_dense_packed_dev): pos [R, A, 3], mask [R, A], aatype, plddt,
    res_index, chain_index [R] (the entry number of the row), cu_seqlens [n + 1] int32 (row cu_seqlens[e] + l is residue l of entry
    e), length [n], names and max_seqlen (a Python int). R counts the residues of the entries that decode: one that does not has no
    row (length 0). Nothing is padded or cropped, so max_len with packed=True is a ValueError.

    crop (with max_len=L; a ValueError without it or with packed=True) keeps a window of L residues at an offset instead of the
    first L: "start" (offset 0), "center" (max(len - L, 0) // 2), "random" (uniform over 0 .. max(len - L, 0), drawn from
    `generator`, a torch.Generator) or the starts [n] themselves (crop_starts). Row l of entry e then holds its residue
    crop_start[e] + l -- bit for bit the row the uncropped call gives that residue -- or padding when the entry has no such
    residue; the OXT appears only in a window that reaches the chain's last residue, res_index counts on from the start, `length`
    stays the full size, and the dict gains crop_start [n] int32. The starts are computed on the device from res_off
    (fcz_dense_window_dev reads them there); with angles=True both calls use the same starts. crop=None: the dict has no new key.

    neighbors=k (1 .. 64) adds the k-nearest-neighbour graph of the tensors just written, in either form, with no host round trip
    (fcz_knn_dev / fcz_knn_packed_dev on the codec's stream behind the dense call): nbr_index [n, L, k] / [R, k] int32 and nbr_dist
    float32, as neighbor_graph describes them, on the sites of neighbor_atom ("CA", "CB" or a slot). With crop the graph is the
    window's own. neighbors=None: the dict has no new key.

    frames="backbone" | "all" adds the rigid frames of the tensors just written, in either form, with no host round trip
    (fcz_frames_dev on the codec's stream behind the dense call): rot [n, L, 3, 3] / [R, 3, 3], trans [.., 3] float32 and frame_mask
    [..] bool for "backbone", rot [.., 8, 3, 3], trans [.., 8, 3], frame_mask [.., 8] for "all", as rigid_frames describes them.
    frames=None: the dict has no new key.

    secondary_structure=True adds the DSSP labels of the tensors just written, in either form, with no host round trip
    (fcz_hbond_dev and fcz_dssp_labels_dev on the codec's stream behind the dense call): ss [n, L] / [R] uint8 and ss_mask bool, as
    secondary_structure describes them (which also returns the H-bond tables). With crop the labels are the window's own.
    False: the dict has no new key.

    sasa=True adds the solvent accessibility of the tensors just written, in either form, with no host round trip (fcz_sasa_dev on the
    codec's stream behind the dense call, with the defaults of solvent_accessibility: probe 1.4, 128 points, Bondi radii): sasa
    [n, L] / [R] float32, rsa float32 and sasa_mask bool, as solvent_accessibility describes them (which also returns the per-atom
    counts). With crop the values are the window's own: atoms outside the window bury nothing. False: the dict has no new key.

    violations=True adds the structural violations of the tensors just written, in either form, with no host round trip
    (fcz_violations_dev on the codec's stream behind the dense call, with the defaults of foldcomp.violations: tolerance 1.5, link
    factor 12, Bondi radii): clash_count [n, L] / [R] int32, link_violation uint8 and viol_mask bool, as violations describes them
    (which also returns the per-atom flags, depths, partners, link geometry and per-chain counts). With crop the values are the
    window's own. False: the dict has no new key.

    Ordering against torch: the uploads and allocations are made on torch's current stream, which is synchronised before the
    codec's calls; the codec works on its own stream, which is synchronised before the tensors are returned. No output byte
    visits the host.
    """
    api.check_crop(crop, max_len, packed)
    nbr = None
    if neighbors is not None:
        nbr = (int(neighbors), api.check_neighbors(neighbors, neighbor_atom, _LAYOUT_WIDTH[dense_layout(layout)]))
    fgroups = None if frames is None else api.check_frames(frames)
    api.check_secondary_structure_flag(secondary_structure)
    api.check_sasa_flag(sasa)
    api.check_violations_flag(violations)
    torch, dev = _torch_device(device)
    c = codec or api.default_codec()
    if int(c.device) != dev.index:
        raise api.error(f"decode_tensors: the codec works on device {c.device}, the tensors were asked for on {dev}")
    lay = dense_layout(layout)
    A = c.lib.fcz_dense_width(lay)
    if packed and max_len is not None:
        raise ValueError("max_len crops to a common length; the packed form keeps every residue (packed=True takes no max_len)")
    if max_len is not None and int(max_len) < 1:
        raise ValueError("max_len must be at least 1")
    entries = [bytes(e) for e in entries]
    n = len(entries)
    names = [_title(e) for e in entries]
    riders = _riders(torch, dev, A, n, nbr, fgroups, bool(secondary_structure), bool(sasa), bool(violations))

    def packed_result(R, cu_seqlens, max_seqlen):
        out = (torch.empty((R, A, 3), dtype=torch.float32, device=dev), torch.empty((R, A), dtype=torch.uint8, device=dev),
               torch.empty(R, dtype=torch.uint8, device=dev), torch.empty(R, dtype=torch.float32, device=dev),
               torch.empty(R, dtype=torch.int32, device=dev), torch.empty(R, dtype=torch.int32, device=dev),
               torch.zeros(n, dtype=torch.int32, device=dev))
        pos, mask, aatype, plddt, res_index, chain_index, length = out
        return out, dict(pos=pos, mask=mask.view(torch.bool), aatype=aatype, plddt=plddt, res_index=res_index, chain_index=chain_index,
                         cu_seqlens=cu_seqlens, length=length, names=names, max_seqlen=int(max_seqlen))

    def result(L, pos, mask, aatype, plddt, res_index, length):
        return dict(pos=pos, mask=mask.view(torch.bool), aatype=aatype, plddt=plddt, res_index=res_index, length=length, names=names)

    def alloc(L):
        return (torch.empty((n, L, A, 3), dtype=torch.float32, device=dev), torch.empty((n, L, A), dtype=torch.uint8, device=dev),
                torch.empty((n, L), dtype=torch.uint8, device=dev), torch.empty((n, L), dtype=torch.float32, device=dev),
                torch.empty((n, L), dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))

    def no_angles(*rows):
        W = len(ANGLE_COLUMNS)
        return dict(angles=torch.empty(rows + (W,), dtype=torch.float32, device=dev), angle_mask=torch.empty(rows + (W,), dtype=torch.bool, device=dev))

    if n == 0:
        if packed:
            d = dict(packed_result(0, torch.zeros(1, dtype=torch.int32, device=dev), 0)[1], **_ride(riders, (0,))[1])
            return dict(d, **no_angles(0)) if angles else d
        L = int(max_len or 0)
        d = dict(result(L, *alloc(L)), **_ride(riders, (0, L))[1])
        if crop is not None:
            d["crop_start"] = crop_starts(d["length"], L, crop, generator)
        return dict(d, **no_angles(0, L)) if angles else d
    blob_t, off_t, res_off_t, atom_off_t, Rv, Mv = _upload_and_size(c, torch, dev, entries)
    R, M = ctypes.c_uint32(Rv), ctypes.c_uint32(Mv)
    if packed:
        # (the angle call is enqueued in front of the decode and leaves it the sizes memo; _decode_packed synchronises the codec)
        extra = _angles_into(c, torch, dev, n, blob_t, off_t, res_off_t, 0, Rv) if angles else {}
        d = _decode_packed(c, torch, dev, lay, n, Rv, Mv, blob_t, off_t, res_off_t, atom_off_t, packed_result, riders)
        return dict(d, **extra)
    if max_len is None:
        ro = res_off_t.cpu().numpy().view(np.uint32).astype(np.int64)      # n + 1 offsets: the only words that come back
        L = int(np.diff(ro).max())
    else:
        L = int(max_len)
    out = alloc(L)
    if L == 0:                                                             # nothing decodes and no width was asked for
        d = dict(result(L, *out), **_ride(riders, (n, 0))[1])
        return dict(d, **no_angles(n, 0)) if angles else d
    start_t = None if crop is None else crop_starts(_entry_lengths(res_off_t), L, crop, generator)
    extra = _angles_into(c, torch, dev, n, blob_t, off_t, res_off_t, L, start_t=start_t) if angles else {}
    if crop is not None:
        extra["crop_start"] = start_t
    made, keys = _ride(riders, (n, L))
    extra.update(keys)
    x, y, z = (torch.empty(max(M.value, 1), dtype=torch.float32, device=dev) for _ in range(3))
    bfac = torch.empty(max(R.value, 1), dtype=torch.float32, device=dev)
    res_code = torch.empty(max(R.value, 1), dtype=torch.uint8, device=dev)
    atoms = CAtomsOut(x.data_ptr(), y.data_ptr(), z.data_ptr(), bfac.data_ptr(), res_code.data_ptr(), None)
    dense = CDenseOut(*(t.data_ptr() for t in out))
    torch.cuda.current_stream(dev).synchronize()
    if R.value:
        _lib.check(c.lib.fcz_decompress_batch_dev(c.ctx, blob_t.data_ptr(), off_t.data_ptr(), n, res_off_t.data_ptr(), atom_off_t.data_ptr(),
                                                  0, ctypes.byref(atoms)), "fcz_decompress_batch_dev")
    if crop is None:
        _lib.check(c.lib.fcz_dense_dev(c.ctx, blob_t.data_ptr(), off_t.data_ptr(), n, res_off_t.data_ptr(), atom_off_t.data_ptr(),
                                       ctypes.byref(atoms), 0, lay, L, ctypes.byref(dense)), "fcz_dense_dev")
    else:
        _lib.check(c.lib.fcz_dense_window_dev(c.ctx, blob_t.data_ptr(), off_t.data_ptr(), n, res_off_t.data_ptr(), atom_off_t.data_ptr(),
                                              ctypes.byref(atoms), 0, lay, L, start_t.data_ptr(), ctypes.byref(dense)), "fcz_dense_window_dev")
    # (a window's padding rows have a cleared mask: no length; otherwise the length the dense call just wrote)
    written = _dense_written(c, torch, dev, out[0], out[1], out[2], lay, n, L, out[5] if crop is None else None, False)
    for rider, t in made:
        rider.enqueue(written, t)
    c.synchronize()
    if "sasa" in extra:
        extra["rsa"] = _rsa(torch, extra["sasa"], extra["sasa_mask"], out[2])
    return dict(result(L, *out), **extra)


class _Rider(NamedTuple):
    """one optional analysis of decode_tensors: alloc(lead) makes its tensors for the leading shape `lead`, `keys` are those of them the
    batch gains, enqueue(written, tensors) puts its calls on the codec's stream behind the dense call"""
    alloc: Callable
    keys: tuple
    enqueue: Callable


def _riders(torch, dev, A, n, nbr, fgroups, want_ss, want_sasa, want_viol):
    """the analyses decode_tensors was asked to add, in the order of their keys: neighbours (nbr = (k, slot)), frames, DSSP labels, solvent
    accessibility and violations, the last three with the defaults of their functions"""
    riders = []
    if nbr is not None:
        k, slot = nbr
        riders.append(_Rider(lambda lead: dict(nbr_index=torch.empty(lead + (k,), dtype=torch.int32, device=dev),
                                               nbr_dist=torch.empty(lead + (k,), dtype=torch.float32, device=dev)),
                             ("nbr_index", "nbr_dist"), lambda w, t: _knn_into(w, slot, k, t["nbr_index"], t["nbr_dist"])))
    if fgroups is not None:
        riders.append(_Rider(lambda lead: _frames_alloc(torch, dev, lead, fgroups), ("rot", "trans", "frame_mask"), lambda w, t: _frames_into(w, fgroups, t)))
    if want_ss:
        riders.append(_Rider(lambda lead: dict(_ss_alloc(torch, dev, lead), **_hbond_alloc(torch, dev, lead)), ("ss", "ss_mask"), lambda w, t: _dssp_into(w, t, t)))
    if want_sasa:
        def sasa_alloc(lead):
            points, counts = _sasa_work(torch, dev, lead + (A,))
            return dict(_sasa_alloc(torch, dev, lead), points=points, counts=counts)
        riders.append(_Rider(sasa_alloc, ("sasa", "rsa", "sasa_mask"), lambda w, t: _sasa_into(w, None, api.SASA_PROBE, t["points"], t["counts"], t)))
    if want_viol:
        riders.append(_Rider(lambda lead: _viol_alloc(torch, dev, lead, A, n), api.VIOLATION_BATCH_KEYS,
                             lambda w, t: _viol_into(w, None, api.VIOLATION_TOLERANCE, api.VIOLATION_LINK_FACTOR, t)))
    return riders


def _ride(riders, lead):
    """every rider's tensors for the leading shape `lead` -> ([(rider, its tensors)], the keys the batch gains)"""
    made = [(r, r.alloc(lead)) for r in riders]
    return made, {k: t[k] for r, t in made for k in r.keys}


def _decode_packed(c, torch, dev, lay, n, R, M, blob_t, off_t, res_off_t, atom_off_t, packed_result, riders):
    """the packed leg of decode_tensors behind fcz_decompress_sizes_dev: R and M are its totals, res_off_t becomes cu_seqlens; the
    riders' analyses follow the dense call on the rows just written"""
    if R > 2 ** 31 - 1:
        raise api.error(f"decode_tensors: {R} residues do not fit the int32 cu_seqlens; split the batch")
    ro = res_off_t.cpu().numpy().view(np.uint32).astype(np.int64)          # n + 1 offsets: the only words that come back
    out, d = packed_result(R, res_off_t, int(np.diff(ro).max()))
    made, keys = _ride(riders, (R,))
    d.update(keys)
    if R == 0:                                                             # nothing decodes: no row, length stays 0
        return d
    x, y, z = (torch.empty(max(M, 1), dtype=torch.float32, device=dev) for _ in range(3))
    bfac = torch.empty(R, dtype=torch.float32, device=dev)
    res_code = torch.empty(R, dtype=torch.uint8, device=dev)
    atoms = CAtomsOut(x.data_ptr(), y.data_ptr(), z.data_ptr(), bfac.data_ptr(), res_code.data_ptr(), None)
    dense = CPackedOut(*(t.data_ptr() for t in out))
    torch.cuda.current_stream(dev).synchronize()
    _lib.check(c.lib.fcz_decompress_batch_dev(c.ctx, blob_t.data_ptr(), off_t.data_ptr(), n, res_off_t.data_ptr(), atom_off_t.data_ptr(),
                                              0, ctypes.byref(atoms)), "fcz_decompress_batch_dev")
    _lib.check(c.lib.fcz_dense_packed_dev(c.ctx, blob_t.data_ptr(), off_t.data_ptr(), n, res_off_t.data_ptr(), atom_off_t.data_ptr(),
                                          ctypes.byref(atoms), 0, lay, ctypes.byref(dense)), "fcz_dense_packed_dev")
    written = _dense_written(c, torch, dev, out[0], out[1], out[2], lay, n, R, res_off_t, True)
    for rider, t in made:
        rider.enqueue(written, t)
    c.synchronize()
    if "sasa" in d:
        d["rsa"] = _rsa(torch, d["sasa"], d["sasa_mask"], out[2])
    return d


_WIDTH_LAYOUT = {37: "atom37", 14: "atom14", 4: "backbone4"}
_LAYOUT_WIDTH = {0: 37, 1: 14, 2: 4}                                        # enum fcz_dense_layout -> A (fcz_dense_width)


def neighbor_graph(batch=None, *, k: int = 48, atom="CA", codec: Optional[Codec] = None, **tensors) -> dict:
    """dense tensors on the GPU -> dict(nbr_index, nbr_dist): the k nearest sites of every residue inside its own chain.

    `batch` is the dict decode_tensors / tensor_batches return, padded or packed, or the tensors come as keywords: pos
    [n, L, A, 3] float32 and mask [n, L, A] bool or uint8, optionally length [n]; or the packed pos [R, A, 3], mask [R, A] with
    cu_seqlens [n + 1] int32 / int64 (recognised as encode_tensors does). atom: "CA", "CB" (atom37 / atom14) or an integer slot;
    the layout is inferred from A. A row is a site when it lies inside its chain, its mask at that slot is set and its
    coordinates there are finite; everything else may hold anything. nbr_index [n, L, k] int32 is the row of the neighbour inside
    the entry (padded) or [R, k] the global row (packed), nearest first, ties by row number; nbr_dist float32 the distance;
    -1 / 0.0 where there is no such neighbour (fewer than k other sites, a row that is no site). The distances are
    sqrt((dx*dx + dy*dy) + dz*dz) in float32, so the result is reproducible bit for bit.

    Padded: `length` is used when the dict has no crop_start (a window's padding rows carry a cleared mask and `length` is the
    uncropped size). Packed: cu_seqlens must be non-decreasing and end at R (checked on the device). The tensors must be contiguous
    and lie on the codec's device; ordering against torch is decode_tensors'. k and atom are checked first, without a device."""
    def check(d):
        shape = tuple(getattr(d.get("pos"), "shape", ()))
        slot = api.check_neighbors(k, atom, shape[-2] if len(shape) in (3, 4) else None)
        _need("neighbor_graph", d)
        return shape, d.get("cu_seqlens") is not None and len(shape) == 3, slot

    x, checked = _inputs("neighbor_graph", "Codec.neighbors", batch, tensors, codec, check, pos_rule="full", aatype=False)
    k, torch, dev = int(k), x.torch, x.dev
    index = torch.empty(x.lead + (k,), dtype=torch.int32, device=dev)
    dist = torch.empty(x.lead + (k,), dtype=torch.float32, device=dev)
    out = dict(nbr_index=index, nbr_dist=dist)
    if x.n == 0 and not x.is_packed or x.rows == 0:
        return out
    torch.cuda.current_stream(dev).synchronize()
    _knn_into(x, checked[2], k, index, dist)
    x.codec.synchronize()
    return out


def _on_device(torch, what, dev, key, t, want, dtypes):
    """tensor `key` of the call `what`: on the device `dev`, of the shape `want`, one of `dtypes`, contiguous"""
    if not isinstance(t, torch.Tensor) or t.device != dev:
        where = t.device if isinstance(t, torch.Tensor) else type(t).__name__
        raise api.error(f"{what}: {key} lies on {where}, pos on {dev}; every tensor must be on the codec's device")
    if t.shape != want or t.dtype not in dtypes:
        raise ValueError(f"{key} must be {' / '.join(str(x) for x in dtypes)} {want}, not {t.dtype} {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: {key} must be contiguous")
    return t


def _chain_bound(torch, what, dev, d, shape, is_packed, one_entry=False):
    """the chains of the dense dict `d` whose pos has `shape` -> (n, rows, bound): packed, rows = R and bound = cu_seqlens as int32
    (non-decreasing and ending at R, checked on the device); padded, rows = L and bound = length as int32, or None when the dict has
    none or carries crop_start (a window's padding rows carry a cleared mask and `length` is the uncropped size). one_entry: what
    rigid_frames reads, which uses atoms of a row's own only -- the packed form is one entry of R rows and cu_seqlens is not looked
    at, and length is clamped at both ends"""
    if is_packed and one_entry:
        return 1, shape[0], None
    if is_packed:
        cu = d["cu_seqlens"]
        if not isinstance(cu, torch.Tensor) or cu.dim() != 1 or cu.shape[0] < 1:
            raise ValueError("cu_seqlens must be a tensor [n + 1]")
        n, R = int(cu.shape[0]) - 1, shape[0]
        cu = _on_device(torch, what, dev, "cu_seqlens", cu, (n + 1,), (torch.int32, torch.int64))
        if bool((cu[1:] < cu[:-1]).any()) or bool(cu[0] < 0) or int(cu[-1]) != R:
            raise ValueError(f"cu_seqlens must be non-decreasing and end at the {R} rows of pos")
        return n, R, cu.to(torch.int32)
    n, L = shape[0], shape[1]
    bound = None
    if d.get("length") is not None and d.get("crop_start") is None:
        # (int32 >= 0 and uint32 share their bits; a negative length reads as a large one and is clamped to L)
        bound = _on_device(torch, what, dev, "length", d["length"], (n,), (torch.int32, torch.int64))
        bound = (bound.clamp(min=0, max=2 ** 31 - 1) if one_entry else bound.clamp(min=0)).to(torch.int32)
    return n, L, bound


class _Dense(NamedTuple):
    """checked dense tensors on the device, what every analysis call reads: pos [.., A, 3] float32 of `shape` = lead + (A, 3), mask
    viewed as uint8 (None only for apply_transform), aatype uint8 or None, `lay` the enum fcz_dense_layout of A; n chains of `rows`
    rows each (padded: rows = L, bound = length as int32 or None) or over `rows` rows in all (packed: rows = R, bound = cu_seqlens)"""
    codec: Codec
    torch: object
    dev: object
    pos: object
    mask: object
    aatype: object
    shape: tuple
    lead: tuple
    A: int
    lay: int
    n: int
    rows: int
    bound: object
    is_packed: bool


def _dense_written(c, torch, dev, pos, mask, aatype, lay, n, rows, bound, is_packed):
    """the record of tensors decode_tensors allocated and had written: nothing to check"""
    shape = tuple(pos.shape)
    return _Dense(c, torch, dev, pos, mask, aatype, shape, shape[:-2], shape[-2], lay, n, rows, bound, is_packed)


def _dense_checked(what, numpy_form, codec, d, shape, is_packed, pos_rule=None, aatype=True, one_entry=False):
    """the record of the dense dict `d` a user gave, behind the device-free checks that found `shape` and `is_packed`: the codec, torch,
    where pos lies, then every tensor on that device, of its shape and dtype, contiguous, and the chains (_chain_bound). pos_rule: the
    shape rule of the functions whose device-free check leaves pos alone, "full" (rank, last axis, dtype) or "rank"; aatype=False: the
    function reads no residue types, whatever the dict holds; numpy_form names the host form in the refusal of numpy arrays"""
    pos = d["pos"]
    c = codec or api.default_codec()
    try:
        import torch
    except ImportError as e:
        raise api.error(f"{what} needs PyTorch (ROCm build): {e}") from None
    if not isinstance(pos, torch.Tensor):
        raise api.error(f"{what} takes torch tensors on the GPU (numpy arrays: {numpy_form})")
    dev = pos.device
    if dev.type != "cuda" or dev.index != int(c.device):
        raise api.error(f"{what}: pos lies on {dev}, the codec works on cuda:{int(c.device)}; there is no CPU path")
    if pos_rule and (len(shape) != (3 if is_packed else 4) or pos_rule == "full" and (shape[-1] != 3 or pos.dtype != torch.float32)):
        raise ValueError(f"pos must be float32 [n, L, A, 3], or [R, A, 3] beside cu_seqlens, not {pos.dtype} {shape}")
    lead, A = shape[:-2], shape[-2]
    if pos.dtype != torch.float32 or not pos.is_contiguous():                 # (pos lies where it lies and has its own shape: the rest of
        _on_device(torch, what, dev, "pos", pos, shape, (torch.float32,))     # its rule, which raises with the rule's message)
    mask = d.get("mask")
    if mask is not None:
        mask = _on_device(torch, what, dev, "mask", mask, shape[:-1], (torch.bool, torch.uint8)).view(torch.uint8)
    aa = d.get("aatype") if aatype else None
    if aa is not None:
        aa = _on_device(torch, what, dev, "aatype", aa, lead, (torch.uint8,))
    n, rows, bound = _chain_bound(torch, what, dev, d, shape, is_packed, one_entry)
    return _Dense(c, torch, dev, pos, mask, aa, shape, lead, A, WIDTH_LAYOUTS[A], n, rows, bound, is_packed)


def _need(what, d, keys=("pos", "mask"), of=""):
    for key in keys:
        if d.get(key) is None:
            raise TypeError(f"{what} needs the tensor {key!r}{of}")


def _inputs(what, numpy_form, batch, tensors, codec, check, pos_rule=None, aatype=True, one_entry=False):
    """the one prelude of the functions on a dense batch: `batch` merged with the keyword tensors, the caller's device-free
    check(d) -> (shape of pos, packed, ...) before a codec is made, then _dense_checked under the same rules -> (the record, what
    check returned)"""
    d = dict(batch) if batch is not None else {}
    d.update(tensors)
    checked = check(d)
    return _dense_checked(what, numpy_form, codec, d, checked[0], checked[1], pos_rule, aatype, one_entry), checked


def _pair_inputs(what, pred, true, codec, check, pos_rule="full", aatype=False, numpy_form=None):
    """the one prelude of the functions on a prediction and its truth: both as dicts (pred may be its bare pos), the tensors that must
    be there, pred's shapes against true's, the caller's device-free check(shape, pred pos shape, pred mask shape or None, true) before
    a codec is made, _dense_checked on `true`, then pred's tensors on its device -> (the record of true, pred pos, pred mask viewed as
    uint8 or None, what check returned)"""
    t = dict(true) if isinstance(true, dict) else {"pos": true}
    p = dict(pred) if isinstance(pred, dict) else {"pos": pred}
    _need(what, t, of=" of true")
    _need(what, p, ("pos",), " of pred")
    ppos, pmask = p["pos"], p.get("mask")
    shape, pshape = tuple(getattr(t["pos"], "shape", ())), tuple(getattr(ppos, "shape", ()))
    mshape = None if pmask is None else tuple(getattr(pmask, "shape", ()))
    if pshape != shape:
        raise ValueError(f"pred pos must have the shape of true pos, {shape}, not {pshape}")
    if mshape is not None and mshape != shape[:-1]:
        raise ValueError(f"pred mask must have the shape of true mask, {shape[:-1]}, not {mshape}")
    checked = check(shape, pshape, mshape, t)
    x = _dense_checked(what, numpy_form or f"Codec.{what}", codec, t, shape, t.get("cu_seqlens") is not None and len(shape) == 3, pos_rule, aatype)
    _on_device(x.torch, what, x.dev, "pred pos", ppos, shape, (x.torch.float32,))
    if pmask is not None:
        pmask = _on_device(x.torch, what, x.dev, "pred mask", pmask, shape[:-1], (x.torch.bool, x.torch.uint8)).view(x.torch.uint8)
    return x, ppos, pmask, checked


def _ptr(t):
    return None if t is None else t.data_ptr()


def _call(c, name, is_packed, *args):
    """the packed or the padded entry point of one analysis, checked under its own name"""
    name += "_packed_dev" if is_packed else "_dev"
    _lib.check(getattr(c.lib, name)(c.ctx, *args), name)


def _chain_score(hits, pairs, bound, is_packed):
    """sum of hits / (4 * sum of pairs) over every chain's rows -> float64 [n], from int64 sums, 0 where the chain has no pair: a
    cumulative sum differenced at cu_seqlens (packed) or a row sum (padded)"""
    import torch
    if is_packed:
        zero = torch.zeros(1, dtype=torch.int64, device=hits.device)
        at = bound.to(torch.int64)
        ch, cp = (torch.cat([zero, x.to(torch.int64).cumsum(0)])[at].diff() for x in (hits, pairs))
    else:
        ch, cp = hits.to(torch.int64).sum(dim=1), pairs.to(torch.int64).sum(dim=1)
    return torch.where(cp > 0, ch.to(torch.float64) / (4 * cp).clamp(min=1).to(torch.float64), torch.zeros((), dtype=torch.float64, device=hits.device))


def _knn_into(x, slot, k, index, dist):
    """fcz_knn_dev / _packed_dev on a record into index and dist [.., k], enqueued on the codec's stream"""
    _call(x.codec, "fcz_knn", x.is_packed, x.pos.data_ptr(), x.mask.data_ptr(), _ptr(x.bound), x.n, x.rows, x.lay, slot, k, index.data_ptr(), dist.data_ptr())


def lddt(pred, true, *, atom="CA", cutoff: float = 15.0, thresholds=(0.5, 1.0, 2.0, 4.0), codec: Optional[Codec] = None) -> dict:
    """predicted coordinates against true ones, both dense tensors on the GPU -> dict(lddt, lddt_pairs, lddt_hits, lddt_chain): the
    per-residue lDDT on the sites of one atom, with no superposition and no L x L matrix.

    `true` is the dict decode_tensors / tensor_batches return, padded (pos [n, L, A, 3], mask [n, L, A], optionally length [n]) or
    packed (pos [R, A, 3], mask [R, A], cu_seqlens [n + 1]), recognised as neighbor_graph recognises them; `length` is ignored when
    the dict carries crop_start. `pred` is a dict with `pos` and optionally `mask` (none: every atom predicted), or just the pos
    tensor, of the same shape. atom: "CA", "CB" (atom37 / atom14) or an integer slot. A row is a site when it lies inside its chain,
    both masks at the slot are set and its six coordinates are finite. For a site i the pairs are the other sites j of its chain
    with d_true(i, j) < cutoff; a pair scores one hit for every threshold that |d_true - d_pred| lies under.
        lddt        [n, L] / [R] float32   hits / (4 * pairs), 0 where the row is no site or has no pair
        lddt_pairs  int32, lddt_hits int32 the two counts
        lddt_chain  [n] float32            sum of hits / (4 * sum of pairs) over the chain's rows (in float64 from int64 sums, so
                                           exact whatever the order), 0 where the chain has no pair
    Distances are sqrt((dx*dx + dy*dy) + dz*dz) in float32 and the counters integers, so the result is reproducible bit for bit.
    It is NOT differentiable: it returns counts (a training target or a validation metric, not a loss; smooth_lddt is the loss on
    the same pairs).

    The tensors must be contiguous and lie on the codec's device; ordering against torch is decode_tensors'. cutoff, thresholds,
    atom and shapes that differ are checked first, without torch or a device (api.check_lddt)."""
    x, ppos, pmask, (slot, cutoff, th) = _pair_inputs(
        "lddt", pred, true, codec, lambda shape, pshape, mshape, t: api.check_lddt(cutoff, thresholds, atom, shape[-2] if len(shape) in (3, 4) else None))
    if x.rows > 2 ** 29:
        raise ValueError("lddt_hits must fit int32: at most 2^29 rows per chain")
    torch, dev = x.torch, x.dev
    score = torch.zeros(x.lead, dtype=torch.float32, device=dev)
    pairs = torch.zeros(x.lead, dtype=torch.int32, device=dev)
    hits = torch.zeros(x.lead, dtype=torch.int32, device=dev)
    if score.numel():
        th_c = (ctypes.c_float * 4)(*th)
        torch.cuda.current_stream(dev).synchronize()
        _call(x.codec, "fcz_lddt", x.is_packed, x.pos.data_ptr(), x.mask.data_ptr(), ppos.data_ptr(), _ptr(pmask), _ptr(x.bound), x.n, x.rows, x.lay, slot, cutoff,
              ctypes.addressof(th_c), score.data_ptr(), pairs.data_ptr(), hits.data_ptr())
        x.codec.synchronize()
    return dict(lddt=score, lddt_pairs=pairs, lddt_hits=hits, lddt_chain=_chain_score(hits, pairs, x.bound, x.is_packed).to(torch.float32))


_autograd = {}


def _autograd_functions(torch):
    """the two torch.autograd.Function classes of smooth_lddt, made once torch is there (this module imports without it)"""
    if _autograd:
        return _autograd["soft"], _autograd["chain_sum"]
    from torch.autograd.function import once_differentiable

    class SoftLddt(torch.autograd.Function):
        """pred pos -> soft [..] (fcz_lddt_soft_dev); `call` holds everything else of the call and receives pairs. The backward is
        the gradient kernel (fcz_lddt_soft_grad_dev) on the saved pos: nothing else is kept from the forward."""

        @staticmethod
        def forward(ctx, ppos, call):
            ctx.call = call
            ctx.save_for_backward(ppos)
            return call.value(ppos)

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_soft):
            (ppos,) = ctx.saved_tensors
            return ctx.call.gradient(ppos, grad_soft.contiguous()), None

    class ChainSum(torch.autograd.Function):
        """packed rows v [R] float64 -> their sums per chain [n], a cumulative sum differenced at cu_seqlens. The backward hands every
        row its chain's gradient by a gather: torch's own backward of the indexing would scatter with float atomics."""

        @staticmethod
        def forward(ctx, v, at):
            ctx.save_for_backward(at)
            ctx.rows = v.shape[0]
            return torch.cat([v.new_zeros(1), v.cumsum(0)])[at].diff()

        @staticmethod
        @once_differentiable
        def backward(ctx, g):
            (at,) = ctx.saved_tensors
            r = torch.arange(ctx.rows, dtype=torch.int64, device=g.device)
            if g.numel() == 0:
                return g.new_zeros(ctx.rows), None
            e = torch.searchsorted(at[1:].contiguous(), r, right=True).clamp(max=g.numel() - 1)     # the chain whose end lies behind row r
            return torch.where((r >= at[0]) & (r < at[-1]), g[e], g.new_zeros(())), None

    _autograd.update(soft=SoftLddt, chain_sum=ChainSum)
    return SoftLddt, ChainSum


class _SoftLddtCall:
    """one call of smooth_lddt: the checked truth, pred's mask and the parameters; value() and gradient() enqueue the two kernels on
    the codec's stream between a wait for torch's stream and codec.synchronize(), as every analysis function does"""

    def __init__(self, x, pmask, slot, cutoff, th):
        self.x, self.pmask, self.slot, self.cutoff, self.th = x, pmask, slot, cutoff, (ctypes.c_float * 4)(*th)
        self.pairs = None

    def _run(self, name, ppos, *outs):
        x = self.x
        x.torch.cuda.current_stream(x.dev).synchronize()
        _call(x.codec, name, x.is_packed, x.pos.data_ptr(), x.mask.data_ptr(), ppos.data_ptr(), _ptr(self.pmask), _ptr(x.bound), x.n, x.rows, x.lay, self.slot,
              self.cutoff, ctypes.addressof(self.th), *(o.data_ptr() for o in outs))
        x.codec.synchronize()

    def value(self, ppos):
        x = self.x
        soft = x.torch.zeros(x.lead, dtype=x.torch.float32, device=x.dev)
        self.pairs = x.torch.zeros(x.lead, dtype=x.torch.int32, device=x.dev)
        if soft.numel():
            self._run("fcz_lddt_soft", ppos, soft, self.pairs)
        return soft

    def gradient(self, ppos, weight):
        x = self.x
        full = x.torch.zeros(x.shape, dtype=x.torch.float32, device=x.dev)
        if weight.numel():
            grad = x.torch.zeros(x.lead + (3,), dtype=x.torch.float32, device=x.dev)
            self._run("fcz_lddt_soft_grad", ppos, weight, grad)
            full[..., self.slot, :] = grad
        return full


def smooth_lddt(pred, true, *, atom="CA", cutoff: float = 15.0, thresholds=(0.5, 1.0, 2.0, 4.0), codec: Optional[Codec] = None) -> dict:
    """predicted coordinates against true ones, both dense tensors on the GPU -> dict(lddt_soft, lddt_pairs, lddt_soft_chain, loss):
    the smooth lDDT of AlphaFold 3 (Algorithm 27), a LOSS: differentiable with respect to pred's pos, with a fused backward on the
    GPU and no L x L matrix in either direction.

    `true` and `pred` are lddt's, padded, packed or a window with crop_start, `pred` a dict with `pos` and optionally `mask`, or the
    bare pos tensor; sites and pairs are lddt's exactly (lddt_pairs equals lddt's). For a pair, delta = |d_true - d_pred| and
    eps = 1/4 sum_k sigmoid(thresholds[k] - delta): lddt's four step functions, smoothed. thresholds must be finite.
        lddt_soft        [n, L] / [R] float32   the mean of eps over the row's pairs, 0 where the row is no site or has no pair
        lddt_pairs       int32                  the pairs of the row
        lddt_soft_chain  [n] float32            the sum of eps over the sum of pairs of the chain's rows, 0 where it has no pair
        loss             scalar float32         the mean of 1 - lddt_soft_chain over the chains that have a pair (0 without one)
    When pred's pos requires a gradient (and gradients are enabled) the four carry a graph: loss.backward() runs the gradient kernel
    once and leaves d loss / d pos in pos.grad, non-zero at the atom's slot of the site rows only. Gradients flow to pred's pos and
    to nothing else; the graph can be walked once and not differentiated twice. Under torch.no_grad(), or for a pos that needs no
    gradient, only the value kernel runs. Every sum has a fixed order (rows in float32 in ascending row order on the device, chains
    in float64, no atomics in either direction): value and gradient are reproducible bit for bit.

    The tensors must be contiguous and lie on the codec's device; ordering against torch is decode_tensors'. The arguments are
    checked first, without torch or a device (api.check_lddt_soft)."""
    x, ppos, pmask, (slot, cutoff, th) = _pair_inputs(
        "smooth_lddt", pred, true, codec, lambda shape, pshape, mshape, t: api.check_lddt_soft(cutoff, thresholds, atom, shape[-2] if len(shape) in (3, 4) else None),
        numpy_form="Codec.lddt_soft")
    if x.rows > 2 ** 29:
        raise ValueError("at most 2^29 rows per chain")
    torch = x.torch
    soft_fn, chain_sum = _autograd_functions(torch)
    call = _SoftLddtCall(x, pmask, slot, cutoff, th)
    soft = soft_fn.apply(ppos, call) if torch.is_grad_enabled() and ppos.requires_grad else call.value(ppos.detach())
    pairs = call.pairs
    has = pairs > 0
    per_row = torch.where(has, soft / pairs.clamp(min=1).to(torch.float32), soft.new_zeros(()))
    if x.is_packed:
        at = x.bound.to(torch.int64)
        cs, cp = chain_sum.apply(soft.to(torch.float64), at), torch.cat([at.new_zeros(1), pairs.to(torch.int64).cumsum(0)])[at].diff()
    else:
        cs, cp = soft.to(torch.float64).sum(dim=1), pairs.to(torch.int64).sum(dim=1)
    scored = cp > 0
    chain = torch.where(scored, cs / cp.clamp(min=1).to(torch.float64), cs.new_zeros(()))
    loss = (torch.where(scored, 1.0 - chain, chain.new_zeros(())).sum() / scored.sum().clamp(min=1).to(torch.float64)).to(torch.float32)
    return dict(lddt_soft=per_row, lddt_pairs=pairs, lddt_soft_chain=chain.to(torch.float32), loss=loss)


def backbone_frames_torch(pos, mask=None):
    """pos [.., A, 3] (N, CA, C in slots 0, 1, 2 as in every layout), mask [.., A] bool / uint8 or None -> (rot [.., 3, 3], trans
    [.., 3], frame_mask [..] bool): AlphaFold's Algorithm 21 as rigid_frames(groups="backbone") defines it (origin CA, x axis CA -> C,
    N in the half-plane y > 0, columns are the axes), in plain differentiable torch operations on any device, O(rows). A residue
    whose three atoms are masked, not finite, coincident or collinear has frame_mask False, the identity and 0, and gives pos a
    gradient that is exactly 0: every normalisation is guarded by a torch.where in FRONT of the root and the division, and what a
    row that is no frame feeds the next step is replaced by 0, so no 0 * inf arises in the backward pass."""
    import torch
    n_, ca, c = pos[..., 0, :], pos[..., 1, :], pos[..., 2, :]
    ok = torch.isfinite(n_).all(-1) & torch.isfinite(ca).all(-1) & torch.isfinite(c).all(-1)
    if mask is not None:
        m = mask.to(torch.bool)
        ok = ok & m[..., 0] & m[..., 1] & m[..., 2]
    zero, one = pos.new_zeros(()), pos.new_ones(())
    ca0 = torch.where(ok[..., None], ca, zero)
    v1 = torch.where(ok[..., None], c, zero) - ca0
    v2 = torch.where(ok[..., None], n_, zero) - ca0
    s1 = (v1 * v1).sum(-1)
    g1 = ok & torch.isfinite(s1) & (s1 > 0)
    v1, v2 = torch.where(g1[..., None], v1, zero), torch.where(g1[..., None], v2, zero)
    e1 = v1 / torch.sqrt(torch.where(g1, s1, one))[..., None]
    d = (e1 * v2).sum(-1)
    gd = g1 & torch.isfinite(d)
    u = torch.where(gd[..., None], v2, zero) - e1 * torch.where(gd, d, zero)[..., None]
    s2 = (u * u).sum(-1)
    g2 = gd & torch.isfinite(s2) & (s2 > 0)
    u = torch.where(g2[..., None], u, zero)
    e2 = u / torch.sqrt(torch.where(g2, s2, one))[..., None]
    e1 = torch.where(g2[..., None], e1, zero)
    e3 = torch.cross(e1, e2, dim=-1)
    eye = torch.eye(3, dtype=pos.dtype, device=pos.device)
    rot = torch.where(g2[..., None, None], torch.stack([e1, e2, e3], dim=-1), eye)
    return rot, torch.where(g2[..., None], ca0, zero), g2


_fape_autograd = {}


def _fape_function(torch):
    """the torch.autograd.Function of fape, made once torch is there"""
    if _fape_autograd:
        return _fape_autograd["fape"]
    from torch.autograd.function import once_differentiable

    class Fape(torch.autograd.Function):
        """(pred rot, pred trans, pred points [.., 3]) -> sum [..] (fcz_fape_dev); `call` holds everything else of the call and
        receives points. The backward is one gradient call (fcz_fape_grad_dev) on the saved inputs: nothing else is kept."""

        @staticmethod
        def forward(ctx, rot, trans, pts, call):
            ctx.call = call
            ctx.save_for_backward(rot, trans, pts)
            return call.value(rot, trans, pts)

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_sum):
            rot, trans, pts = ctx.saved_tensors
            return (*ctx.call.gradient(rot, trans, pts, grad_sum.contiguous()), None)

    _fape_autograd["fape"] = Fape
    return Fape


class _FapeCall:
    """one call of fape: the checked truth and its frames, the prediction's masks and the parameters; value() and gradient() enqueue
    the kernels on the codec's stream between a wait for torch's stream and codec.synchronize(), as every analysis function does.
    pos_full: the prediction's whole pos tensor (detached) when it has one, whose slot the points are; None: the points are embedded
    in a tensor of the truth's shape for the call"""

    def __init__(self, x, tframes, pfmask, pos_full, pmask, slot, clamp, eps):
        self.x, self.tframes, self.pfmask, self.pos_full, self.pmask = x, tframes, pfmask, pos_full, pmask
        self.slot, self.clamp, self.eps = slot, clamp, eps
        self.points = None

    def _run(self, name, rot, trans, pts, *rest):
        x, torch = self.x, self.x.torch
        pos = self.pos_full
        if pos is None:
            pos = torch.zeros(x.shape, dtype=torch.float32, device=x.dev)
            pos[..., self.slot, :] = pts
        trot, ttrans, tfm = self.tframes
        torch.cuda.current_stream(x.dev).synchronize()
        _call(x.codec, name, x.is_packed, trot.data_ptr(), ttrans.data_ptr(), tfm.data_ptr(), x.pos.data_ptr(), x.mask.data_ptr(), rot.data_ptr(), trans.data_ptr(),
              _ptr(self.pfmask), pos.data_ptr(), _ptr(self.pmask), _ptr(x.bound), x.n, x.rows, x.lay, self.slot, self.clamp, self.eps, *(o.data_ptr() for o in rest))
        x.codec.synchronize()

    def value(self, rot, trans, pts):
        x = self.x
        total = x.torch.zeros(x.lead, dtype=x.torch.float32, device=x.dev)
        self.points = x.torch.zeros(x.lead, dtype=x.torch.int32, device=x.dev)
        if total.numel():
            self._run("fcz_fape", rot.detach().contiguous(), trans.detach().contiguous(), pts.detach(), total, self.points)
        return total

    def gradient(self, rot, trans, pts, weight):
        x = self.x
        grads = [x.torch.zeros(x.lead + s, dtype=x.torch.float32, device=x.dev) for s in ((3, 3), (3,), (3,))]
        if weight.numel():
            self._run("fcz_fape_grad", rot.contiguous(), trans.contiguous(), pts, weight, *grads)
        return grads


def fape(pred, true, *, atom="CA", clamp=10.0, scale: float = 10.0, eps: float = 1e-4, codec: Optional[Codec] = None) -> dict:
    """predicted frames and points against true ones, dense tensors on the GPU -> dict(fape_frame, fape_points, frame_mask, fape_chain,
    loss): the backbone FAPE (frame aligned point error; AlphaFold 2 supplement, Algorithm 28), a LOSS with a fused backward on the GPU
    and no L x L array in either direction.

    `true` is the dict decode_tensors / tensor_batches return, padded, packed or a window with crop_start. Its frames are its rot /
    trans / frame_mask when it carries the backbone ones (decode_tensors(..., frames="backbone")), and are computed inside the call
    (fcz_frames_dev) otherwise. `pred` is either
      * a dict with rot [.., 3, 3] and trans [.., 3], the model's own frames, optionally frame_mask [..] and optionally pos / mask
        of true's shape: the points are pos at `atom`, or trans when there is no pos (AlphaFold's backbone FAPE; trans.grad then
        receives both contributions); or
      * a pos tensor of true's shape, or a dict with pos (and mask): the predicted frames are built from N, CA, C of pos by
        Algorithm 21 in differentiable torch operations (backbone_frames_torch) and autograd carries the gradient on to pos; a
        degenerate or masked residue is no frame and gets a gradient of exactly 0.
    A row is a frame when it lies inside its chain, both frame masks are set and the 24 floats are finite; a point as lddt's site.
    Every frame meets every point of its chain: d = sqrt(|R^T (x - t) - R'^T (x' - t')|^2 + eps), term = min(d, clamp).
        fape_frame   [n, L] / [R] float32   the mean of term over the chain's points, over scale; 0 where there is no frame or no point
        fape_points  int32                  the points a frame row met
        frame_mask   bool                   the frame rows
        fape_chain   [n] float32            the chain's sum of term over (frames * points * scale), summed in float64
        loss         scalar float32         the mean of fape_chain over the chains that have a frame and a point (0 without one)
    clamp=None (or +inf) is the unclamped FAPE. When any of the prediction's tensors requires a gradient (and gradients are enabled)
    the results carry a graph: loss.backward() runs the gradient call once (one torch.autograd.Function over rot, trans and the
    points); the graph can be walked once and not differentiated twice. Under torch.no_grad(), or with nothing that requires a
    gradient, only the value kernel runs. Every sum has a fixed order (rows in float32 in ascending row order on the device, chains
    in float64, no atomics): value and gradient are reproducible bit for bit.

    The tensors must be contiguous and lie on the codec's device; ordering against torch is decode_tensors'. The arguments are
    checked first, without torch or a device (api.check_fape)."""
    what = "fape"
    t = dict(true) if isinstance(true, dict) else {"pos": true}
    p = dict(pred) if isinstance(pred, dict) else {"pos": pred}
    _need(what, t, of=" of true")
    shape = tuple(getattr(t["pos"], "shape", ()))
    slot, clamp, scale, eps = api.check_fape(clamp, scale, eps, atom, shape[-2] if len(shape) in (3, 4) else None)
    if len(shape) not in (3, 4) or shape[-1] != 3 or shape[-2] not in _WIDTH_LAYOUT:
        raise ValueError(f"pos must be float32 [n, L, A, 3], or [R, A, 3] beside cu_seqlens, with A = 37, 14 or 4, not {shape}")
    lead = shape[:-2]
    given = p.get("rot") is not None or p.get("trans") is not None
    if given:
        _need(what, p, ("rot", "trans"), " of pred")
        for key, want in (("rot", lead + (3, 3)), ("trans", lead + (3,)), ("frame_mask", lead)):
            if p.get(key) is not None and tuple(getattr(p[key], "shape", ())) != want:
                raise ValueError(f"pred {key} must have the shape {want}, not {tuple(getattr(p[key], 'shape', ()))}")
    else:
        _need(what, p, ("pos",), " of pred")
    for key, want in (("pos", shape), ("mask", shape[:-1])):
        if p.get(key) is not None and tuple(getattr(p[key], "shape", ())) != want:
            raise ValueError(f"pred {key} must have the shape of true {key}, {want}, not {tuple(getattr(p[key], 'shape', ()))}")
    x = _dense_checked(what, "Codec.fape", codec, t, shape, t.get("cu_seqlens") is not None and len(shape) == 3, "full", aatype=False)
    if x.rows > 2 ** 29:
        raise ValueError("at most 2^29 rows per chain")
    torch, dev = x.torch, x.dev
    # the truth's frames: the dict's backbone ones, or fcz_frames_dev here
    if all(t.get(k) is not None for k in ("rot", "trans", "frame_mask")) and tuple(getattr(t["rot"], "shape", ())) == lead + (3, 3):
        tframes = (_on_device(torch, what, dev, "rot", t["rot"], lead + (3, 3), (torch.float32,)),
                   _on_device(torch, what, dev, "trans", t["trans"], lead + (3,), (torch.float32,)),
                   _on_device(torch, what, dev, "frame_mask", t["frame_mask"], lead, (torch.bool, torch.uint8)).view(torch.uint8))
    else:
        made = _frames_alloc(torch, dev, lead, 0)
        if x.n and x.rows:
            torch.cuda.current_stream(dev).synchronize()
            _frames_into(x, 0, made)
            x.codec.synchronize()
        tframes = (made["rot"], made["trans"], made["frame_mask"].view(torch.uint8))
    ppos, pmask = p.get("pos"), p.get("mask")
    if ppos is not None:
        _on_device(torch, what, dev, "pred pos", ppos, shape, (torch.float32,))
    if pmask is not None:
        pmask = _on_device(torch, what, dev, "pred mask", pmask, shape[:-1], (torch.bool, torch.uint8)).view(torch.uint8)
    if given:
        rot = _on_device(torch, what, dev, "pred rot", p["rot"], lead + (3, 3), (torch.float32,))
        trans = _on_device(torch, what, dev, "pred trans", p["trans"], lead + (3,), (torch.float32,))
        pfm = p.get("frame_mask")
        if pfm is not None:
            pfm = _on_device(torch, what, dev, "pred frame_mask", pfm, lead, (torch.bool, torch.uint8)).view(torch.uint8)
    else:
        rot, trans, pfm = backbone_frames_torch(ppos, pmask)
        pfm = pfm.view(torch.uint8)
    pts = trans if ppos is None else ppos[..., slot, :]
    call = _FapeCall(x, tframes, pfm, None if ppos is None else ppos.detach(), pmask, slot, clamp, eps)
    if torch.is_grad_enabled() and (rot.requires_grad or trans.requires_grad or pts.requires_grad):
        total = _fape_function(torch).apply(rot, trans, pts, call)
    else:
        total = call.value(rot, trans, pts)
    points = call.points
    # the frame rows: inside their chain, both masks, 24 finite floats
    with torch.no_grad():
        fm = tframes[2] != 0
        if pfm is not None:
            fm = fm & (pfm != 0)
        for v in (tframes[0], rot.detach()):
            fm = fm & torch.isfinite(v).all(-1).all(-1)
        for v in (tframes[1], trans.detach()):
            fm = fm & torch.isfinite(v).all(-1)
        if x.is_packed:
            r = torch.arange(x.rows, device=dev)
            fm = fm & (r >= x.bound[0]) & (r < x.bound[-1])
        elif x.bound is not None:
            fm = fm & (torch.arange(x.rows, device=dev)[None, :] < x.bound[:, None])
    has = points > 0
    per_row = torch.where(has, total / (points.clamp(min=1).to(torch.float32) * scale), total.new_zeros(()))
    if x.is_packed:
        at = x.bound.to(torch.int64)
        cs = _autograd_functions(torch)[1].apply(total.to(torch.float64), at)
        cp = torch.cat([at.new_zeros(1), points.to(torch.int64).cumsum(0)])[at].diff()
    else:
        cs, cp = total.to(torch.float64).sum(dim=1), points.to(torch.int64).sum(dim=1)
    scored = cp > 0                                                           # (sum of points over the frame rows = frames * points)
    chain = torch.where(scored, cs / (cp.clamp(min=1).to(torch.float64) * scale), cs.new_zeros(()))
    loss = (chain.sum() / scored.sum().clamp(min=1).to(torch.float64)).to(torch.float32)
    return dict(fape_frame=per_row, fape_points=points, frame_mask=fm, fape_chain=chain.to(torch.float32), loss=loss)


_frame_slots = {}


def _frame_slot_table(lay):
    """int64 [21, 8, 3] as nested lists: the slot of defining atom j (fcz_frame_atom's order p, o, q) of (type, group) in the layout
    `lay` (the enum), -1 where the type or the layout has no such atom; type 20 = every other aatype value: groups 0 and 3 only"""
    if lay not in _frame_slots:
        lib = _lib.load()
        t = np.full((21, 8, 3), -1, np.int64)
        for ty in range(21):
            for g in range(8):
                if g >= 4 and ty >= 20:
                    continue
                atoms = [lib.fcz_frame_atom(ty if ty < 20 else 0, g, j) for j in range(3)]
                if min(atoms) < 0:
                    continue
                slots = [lib.fcz_dense_slot(lay, ty if g >= 4 else 0, a) for a in atoms]   # (N, CA, C, O: the same slot in every type)
                if min(slots) >= 0:
                    t[ty, g] = slots
        _frame_slots[lay] = t
    return _frame_slots[lay]


def rigid_frames_torch(pos, mask=None, aatype=None, layout=None):
    """pos [.., A, 3], mask [.., A] bool / uint8 or None, aatype [..] uint8 or None (then only the backbone and the psi group can
    exist), layout "atom37" / "atom14" / "backbone4" or None (read from A) -> (rot [.., 8, 3, 3], trans [.., 8, 3], frame_mask
    [.., 8] bool): the eight rigid groups as rigid_frames(groups="all") defines them (the three atoms of fcz_frame_atom at the slots
    of fcz_dense_slot; v1 = p - o for the backbone group and o - p for the others, v2 = q - o, origin o, columns are the axes), in
    plain differentiable torch operations on any device, O(rows). It generalises backbone_frames_torch, guard for guard: a group
    that does not exist (no such atoms in the type or the layout, a cleared mask, a coordinate that is not finite, coincident or
    collinear atoms) has frame_mask False, the identity and 0, and gives pos a gradient that is exactly 0."""
    import torch
    A = pos.shape[-2]
    lay = WIDTH_LAYOUTS.get(A) if layout is None else dense_layout(layout)
    if lay is None or WIDTH_LAYOUTS.get(A) != lay:
        raise ValueError(f"pos [.., {A}, 3] does not have the width of the layout {layout!r}: A = 37, 14 or 4")
    table = torch.as_tensor(_frame_slot_table(lay), device=pos.device)
    lead = tuple(pos.shape[:-2])
    ty = torch.full(lead, 20, dtype=torch.int64, device=pos.device) if aatype is None else aatype.to(torch.int64).clamp(max=20)
    sl = table[ty]                                                            # [.., 8, 3]
    ok = (sl >= 0).all(-1)
    idx = sl.clamp(min=0)
    p_, o_, q_ = (torch.gather(pos, -2, idx[..., j, None].expand(lead + (8, 3))) for j in range(3))
    ok = ok & torch.isfinite(p_).all(-1) & torch.isfinite(o_).all(-1) & torch.isfinite(q_).all(-1)
    if mask is not None:
        m = mask.to(torch.bool)
        ok = ok & torch.gather(m, -1, idx[..., 0]) & torch.gather(m, -1, idx[..., 1]) & torch.gather(m, -1, idx[..., 2])
    zero, one = pos.new_zeros(()), pos.new_ones(())
    o0 = torch.where(ok[..., None], o_, zero)
    p0, q0 = torch.where(ok[..., None], p_, zero), torch.where(ok[..., None], q_, zero)
    backbone = (torch.arange(8, device=pos.device) == 0)[:, None]
    v1 = torch.where(backbone, p0 - o0, o0 - p0)
    v2 = q0 - o0
    s1 = (v1 * v1).sum(-1)
    g1 = ok & torch.isfinite(s1) & (s1 > 0)
    v1, v2 = torch.where(g1[..., None], v1, zero), torch.where(g1[..., None], v2, zero)
    e1 = v1 / torch.sqrt(torch.where(g1, s1, one))[..., None]
    d = (e1 * v2).sum(-1)
    gd = g1 & torch.isfinite(d)
    u = torch.where(gd[..., None], v2, zero) - e1 * torch.where(gd, d, zero)[..., None]
    s2 = (u * u).sum(-1)
    g2 = gd & torch.isfinite(s2) & (s2 > 0)
    u = torch.where(g2[..., None], u, zero)
    e2 = u / torch.sqrt(torch.where(g2, s2, one))[..., None]
    e1 = torch.where(g2[..., None], e1, zero)
    e3 = torch.cross(e1, e2, dim=-1)
    eye = torch.eye(3, dtype=pos.dtype, device=pos.device)
    rot = torch.where(g2[..., None, None], torch.stack([e1, e2, e3], dim=-1), eye)
    return rot, torch.where(g2[..., None], o0, zero), g2


def _fape_atoms_function(torch):
    """the torch.autograd.Function of fape_atoms, made once torch is there"""
    if "fape_atoms" in _fape_autograd:
        return _fape_autograd["fape_atoms"]
    from torch.autograd.function import once_differentiable

    class FapeAtoms(torch.autograd.Function):
        """(pred rot [.., 8, 3, 3], pred trans [.., 8, 3], pred pos [.., A, 3]) -> sum [.., 8] (fcz_fape_atoms_dev); `call` holds
        everything else of the call and receives points. The backward is one gradient call (fcz_fape_atoms_grad_dev) on the saved
        inputs: nothing else is kept."""

        @staticmethod
        def forward(ctx, rot, trans, pos, call):
            ctx.call = call
            ctx.save_for_backward(rot, trans, pos)
            return call.value(rot, trans, pos)

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_sum):
            rot, trans, pos = ctx.saved_tensors
            return (*ctx.call.gradient(rot, trans, pos, grad_sum.contiguous()), None)

    _fape_autograd["fape_atoms"] = FapeAtoms
    return FapeAtoms


class _FapeAtomsCall:
    """one call of fape_atoms: the checked truth and its eight-group frames, the renaming decision, the prediction's masks and the
    parameters; value() and gradient() enqueue the kernels on the codec's stream between a wait for torch's stream and
    codec.synchronize(), as every analysis function does"""

    def __init__(self, x, tframes, swapped, pfmask, pmask, clamp, eps, table):
        self.x, self.tframes, self.swapped, self.pfmask, self.pmask = x, tframes, swapped, pfmask, pmask
        self.clamp, self.eps, self.table = clamp, eps, table
        self.points = None

    def _run(self, name, rot, trans, pos, *rest):
        x, torch = self.x, self.x.torch
        trot, ttrans, tfm = self.tframes
        torch.cuda.current_stream(x.dev).synchronize()
        _call(x.codec, name, x.is_packed, trot.data_ptr(), ttrans.data_ptr(), tfm.data_ptr(), x.pos.data_ptr(), x.mask.data_ptr(),
              _ptr(x.aatype) if self.swapped is not None else None, _ptr(self.swapped), rot.data_ptr(), trans.data_ptr(), _ptr(self.pfmask), pos.data_ptr(),
              _ptr(self.pmask), _ptr(x.bound), x.n, x.rows, x.lay, self.clamp, self.eps, None if self.table is None else self.table.ctypes.data,
              *(o.data_ptr() for o in rest))
        x.codec.synchronize()

    def value(self, rot, trans, pos):
        x = self.x
        total = x.torch.zeros(x.lead + (8,), dtype=x.torch.float32, device=x.dev)
        self.points = x.torch.zeros(x.lead + (8,), dtype=x.torch.int32, device=x.dev)
        if total.numel():
            self._run("fcz_fape_atoms", rot.detach().contiguous(), trans.detach().contiguous(), pos.detach().contiguous(), total, self.points)
        return total

    def gradient(self, rot, trans, pos, weight):
        x = self.x
        grads = [x.torch.zeros(x.lead + s, dtype=x.torch.float32, device=x.dev) for s in ((8, 3, 3), (8, 3), (x.A, 3))]
        if weight.numel():
            self._run("fcz_fape_atoms_grad", rot.contiguous(), trans.contiguous(), pos.contiguous(), weight, *grads)
        return grads


def fape_atoms(pred, true, *, clamp=10.0, scale: float = 10.0, eps: float = 1e-4, rename="lddt_atoms", swaps="alphafold",
               codec: Optional[Codec] = None) -> dict:
    """the eight rigid groups of every residue of a prediction against every atom of its chain, dense tensors on the GPU ->
    dict(fape_frame, fape_points, frame_mask, swapped, fape_chain, loss): the all-atom ("side-chain") half of AlphaFold 2's structure
    module FAPE, with the truth renamed towards the prediction first, a LOSS with a fused backward on the GPU and no frames x atoms
    array in either direction. It stands beside fape, which is the backbone half.

    `true` is the dict decode_tensors / tensor_batches return, padded, packed or a window with crop_start. Its frames are its rot /
    trans / frame_mask when it carries the eight-group ones (decode_tensors(..., frames="all")), and are computed inside the call
    (fcz_frames_dev, which needs aatype) otherwise. `pred` is either
      * a dict with rot [.., 8, 3, 3], trans [.., 8, 3] and pos of true's shape, optionally frame_mask [.., 8] and mask: the model's
        own side-chain frames and atoms; or
      * a pos tensor of true's shape, or a dict with pos (and mask): the predicted frames are built from pos in differentiable
        torch operations (rigid_frames_torch with true's aatype) and autograd carries the gradient on to pos.
    rename: "lddt_atoms" runs lddt_atoms(pred.detach(), true)["swapped"] inside the call; a bool / uint8 tensor [..] is a decision
    already made (one lddt_atoms call can serve both); None renames nothing. Where a residue is swapped the truth's atoms are read
    at the slots of `swaps` (lddt_atoms' table) and its ambiguous groups (frame_ambiguous) turned by 180 degrees, AlphaFold's
    rigidgroups_alt_gt_frames. An item (row, group) is a frame when the row lies inside its chain, both frame masks are set and the
    24 floats are finite; a slot is a point as lddt_atoms' atom. Every frame meets every point of its chain, its own residue's
    included: d = sqrt(|R^T (x - t) - R'^T (x' - t')|^2 + eps), term = min(d, clamp).
        fape_frame   [n, L, 8] / [R, 8] float32   the mean of term over the chain's points, over scale; 0 without a frame or a point
        fape_points  int32                        the points a frame met
        frame_mask   bool                         the frames
        swapped      [n, L] / [R] bool            the renaming that was applied
        fape_chain   [n] float32                  the chain's sum of term over (the points summed over its frames * scale), in float64
        loss         scalar float32               the mean of fape_chain over the chains that have a term (0 without one)
    clamp=None (or +inf) is the unclamped FAPE. When any of the prediction's tensors requires a gradient (and gradients are enabled)
    loss.backward() runs the gradient call once (one torch.autograd.Function over rot, trans and pos); the graph can be walked once
    and not differentiated twice. Under torch.no_grad(), or with nothing that requires a gradient, only the value kernel runs. Every
    sum has a fixed order (float32 in ascending (row, slot) on the device, chains in float64, no atomics): value and gradient are
    reproducible bit for bit.

    The tensors must be contiguous and lie on the codec's device; ordering against torch is decode_tensors'. The arguments are
    checked first, without torch or a device (api.check_fape_atoms)."""
    what = "fape_atoms"
    t = dict(true) if isinstance(true, dict) else {"pos": true}
    p = dict(pred) if isinstance(pred, dict) else {"pos": pred}
    _need(what, t, of=" of true")
    _need(what, p, ("pos",), " of pred")
    shape = tuple(getattr(t["pos"], "shape", ()))
    clamp, scale, eps, rename, table = api.check_fape_atoms(clamp, scale, eps, rename, shape, t.get("aatype") is not None, swaps)
    lead = shape[:-2]
    given = p.get("rot") is not None or p.get("trans") is not None
    if given:
        _need(what, p, ("rot", "trans"), " of pred")
    for key, want in (("rot", lead + (8, 3, 3)), ("trans", lead + (8, 3)), ("frame_mask", lead + (8,))):
        if given and p.get(key) is not None and tuple(getattr(p[key], "shape", ())) != want:
            raise ValueError(f"pred {key} must have the shape {want}, not {tuple(getattr(p[key], 'shape', ()))}")
    for key, want in (("pos", shape), ("mask", shape[:-1])):
        if p.get(key) is not None and tuple(getattr(p[key], "shape", ())) != want:
            raise ValueError(f"pred {key} must have the shape of true {key}, {want}, not {tuple(getattr(p[key], 'shape', ()))}")
    own = all(t.get(k) is not None for k in ("rot", "trans", "frame_mask")) and tuple(getattr(t["rot"], "shape", ())) == lead + (8, 3, 3)
    if not own and t.get("aatype") is None:
        raise ValueError("fape_atoms needs aatype in `true` to build its eight-group frames (or rot / trans / frame_mask of frames='all')")
    x = _dense_checked(what, "Codec.fape_atoms", codec, t, shape, t.get("cu_seqlens") is not None and len(shape) == 3, "full", aatype=True)
    torch, dev = x.torch, x.dev
    if own:
        tframes = (_on_device(torch, what, dev, "rot", t["rot"], lead + (8, 3, 3), (torch.float32,)),
                   _on_device(torch, what, dev, "trans", t["trans"], lead + (8, 3), (torch.float32,)),
                   _on_device(torch, what, dev, "frame_mask", t["frame_mask"], lead + (8,), (torch.bool, torch.uint8)).view(torch.uint8))
    else:
        made = _frames_alloc(torch, dev, lead, 1)
        if x.n and x.rows:
            torch.cuda.current_stream(dev).synchronize()
            _frames_into(x, 1, made)
            x.codec.synchronize()
        tframes = (made["rot"], made["trans"], made["frame_mask"].view(torch.uint8))
    ppos, pmask = p["pos"], p.get("mask")
    _on_device(torch, what, dev, "pred pos", ppos, shape, (torch.float32,))
    if pmask is not None:
        pmask = _on_device(torch, what, dev, "pred mask", pmask, shape[:-1], (torch.bool, torch.uint8)).view(torch.uint8)
    if given:
        rot = _on_device(torch, what, dev, "pred rot", p["rot"], lead + (8, 3, 3), (torch.float32,))
        trans = _on_device(torch, what, dev, "pred trans", p["trans"], lead + (8, 3), (torch.float32,))
        pfm = p.get("frame_mask")
        if pfm is not None:
            pfm = _on_device(torch, what, dev, "pred frame_mask", pfm, lead + (8,), (torch.bool, torch.uint8)).view(torch.uint8)
    else:
        rot, trans, pfm = rigid_frames_torch(ppos, pmask, x.aatype)
        pfm = pfm.contiguous().view(torch.uint8)
    # the renaming decision
    if rename is None:
        swapped = None
    elif isinstance(rename, str):
        with torch.no_grad():
            swapped = lddt_atoms(dict(pos=ppos.detach(), mask=None if pmask is None else pmask), t, swaps=swaps, codec=x.codec)["swapped"].view(torch.uint8)
    else:
        swapped = _on_device(torch, what, dev, "rename", rename, lead, (torch.bool, torch.uint8)).view(torch.uint8)
    call = _FapeAtomsCall(x, tframes, swapped, pfm, pmask, clamp, eps, table)
    if torch.is_grad_enabled() and (rot.requires_grad or trans.requires_grad or ppos.requires_grad):
        total = _fape_atoms_function(torch).apply(rot, trans, ppos, call)
    else:
        total = call.value(rot, trans, ppos)
    points = call.points
    # the frames: inside their chain, both masks, 24 finite floats; backbone4 holds groups 0 and 3 alone
    with torch.no_grad():
        fm = tframes[2] != 0
        if pfm is not None:
            fm = fm & (pfm != 0)
        for v in (tframes[0], rot.detach()):
            fm = fm & torch.isfinite(v).all(-1).all(-1)
        for v in (tframes[1], trans.detach()):
            fm = fm & torch.isfinite(v).all(-1)
        if x.A == 4:
            fm = fm & torch.tensor([True, False, False, True, False, False, False, False], device=dev)
        if x.is_packed:
            r = torch.arange(x.rows, device=dev)
            fm = fm & ((r >= x.bound[0]) & (r < x.bound[-1]))[:, None]
        elif x.bound is not None:
            fm = fm & (torch.arange(x.rows, device=dev)[None, :] < x.bound[:, None])[..., None]
    has = points > 0
    per_item = torch.where(has, total / (points.clamp(min=1).to(torch.float32) * scale), total.new_zeros(()))
    row_sum, row_points = total.to(torch.float64).sum(-1), points.to(torch.int64).sum(-1)
    if x.is_packed:
        at = x.bound.to(torch.int64)
        cs = _autograd_functions(torch)[1].apply(row_sum, at)
        cp = torch.cat([at.new_zeros(1), row_points.cumsum(0)])[at].diff()
    else:
        cs, cp = row_sum.sum(dim=1), row_points.sum(dim=1)
    scored = cp > 0
    chain = torch.where(scored, cs / (cp.clamp(min=1).to(torch.float64) * scale), cs.new_zeros(()))
    loss = (chain.sum() / scored.sum().clamp(min=1).to(torch.float64)).to(torch.float32)
    sw = torch.zeros(lead, dtype=torch.bool, device=dev) if swapped is None else swapped.view(torch.bool) if swapped.dtype == torch.uint8 else swapped
    return dict(fape_frame=per_item, fape_points=points, frame_mask=fm, swapped=sw, fape_chain=chain.to(torch.float32), loss=loss)


def lddt_atoms(pred, true, *, cutoff: float = 15.0, thresholds=(0.5, 1.0, 2.0, 4.0), swaps="alphafold", per_atom: bool = False,
               codec: Optional[Codec] = None) -> dict:
    """predicted coordinates against true ones, both dense tensors on the GPU -> the all-atom lDDT of every residue, after the
    chemically equivalent side-chain namings of the truth have been resolved towards the prediction; no atoms x atoms matrix.

    `true` and `pred` are lddt's: `true` the dict decode_tensors / tensor_batches return, padded or packed, `pred` a dict with `pos`
    and optionally `mask`, or just the pos tensor, of the same shape. `true` must carry `aatype` unless swaps=None. An atom is a slot
    of a row inside its chain with both masks set and six finite coordinates. For an atom i the pairs are the atoms j of the OTHER
    residues of its chain with d_true(i, j) < cutoff; a pair scores one hit for every threshold |d_true - d_pred| lies under.
        swapped      [n, L] / [R] bool       True where the truth of the residue is read under its other naming: the residue has
                                             atoms with one (ASP OD1 / OD2, GLU OE1 / OE2, PHE and TYR CD1 / CD2 with CE1 / CE2), all of
                                             them are present, and against the atoms without one of the chain's other residues the
                                             other naming scores the strictly larger hits / pairs (AlphaFold's alt_naming_is_better)
        lddt         float32                 hits / (4 * pairs) over the residue's atoms, 0 where it has no pair
        lddt_pairs   int32, lddt_hits int32  the two sums
        lddt_chain   [n] float64             sum of hits / (4 * sum of pairs) over the chain's rows (float64 from int64 sums, so
                                             exact whatever the order), 0 where the chain has no pair
        atom_pairs, atom_hits [.., A] int32  with per_atom=True: the two counts of every atom, at the prediction's slot
    swaps: "alphafold" (foldcomp.lddt_swaps(layout)), None (no renaming) or an integer array [21, A]: swaps[aatype][slot] is the
    slot of the other naming, the slot itself where there is none. Distances are sqrt((dx*dx + dy*dy) + dz*dz) in float32 and all
    counters integers (include/fcz_hip.h, fcz_lddt_atoms_dev): reproducible bit for bit, the same in atom37 and atom14, NOT
    differentiable. The tensors must be contiguous and lie on the codec's device; the arguments are checked first, without torch or a
    device (api.check_lddt_atoms)."""
    def check(shape, pshape, mshape, t):
        checked = api.check_lddt_atoms(cutoff, thresholds, swaps, shape, pshape, mshape, t.get("aatype") is not None, per_atom)
        if checked[2] is False:
            t["aatype"] = None                                                # (no renaming: the residue types are not looked at)
        return checked

    x, ppos, pmask, (cutoff, th, table) = _pair_inputs("lddt_atoms", pred, true, codec, check, pos_rule="rank", aatype=True)
    torch, dev, lead = x.torch, x.dev, x.lead
    score = torch.zeros(lead, dtype=torch.float32, device=dev)
    pairs = torch.zeros(lead, dtype=torch.int32, device=dev)
    hits = torch.zeros(lead, dtype=torch.int32, device=dev)
    swapped = torch.zeros(lead, dtype=torch.uint8, device=dev)
    atom = [torch.zeros(lead + (x.A,), dtype=torch.int32, device=dev) for _ in range(2)] if per_atom else None
    if score.numel():
        th_c = (ctypes.c_float * 4)(*th)
        c_out = CLddtAtomsOut(score.data_ptr(), pairs.data_ptr(), hits.data_ptr(), swapped.data_ptr(), *((a.data_ptr() for a in atom) if atom else (None, None)))
        torch.cuda.current_stream(dev).synchronize()
        _call(x.codec, "fcz_lddt_atoms", x.is_packed, x.pos.data_ptr(), x.mask.data_ptr(), ppos.data_ptr(), _ptr(pmask), _ptr(x.aatype), _ptr(x.bound), x.n, x.rows,
              x.lay, cutoff, ctypes.addressof(th_c), table.ctypes.data if isinstance(table, np.ndarray) else None, ctypes.byref(c_out))
        x.codec.synchronize()
    out = dict(lddt=score, lddt_pairs=pairs, lddt_hits=hits, swapped=swapped.view(torch.bool), lddt_chain=_chain_score(hits, pairs, x.bound, x.is_packed))
    if atom:
        out.update(atom_pairs=atom[0], atom_hits=atom[1])
    return out


def superpose(pred, true, *, atom="CA", apply: bool = False, codec: Optional[Codec] = None) -> dict:
    """predicted coordinates against true ones, both dense tensors on the GPU -> the least-squares (Kabsch) superposition of every
    chain of `pred` onto `true` on the sites of one atom, and the scores that depend on it.

    The inputs are lddt's: `true` is the dict decode_tensors / tensor_batches return, padded or packed (`length` is ignored when the
    dict carries crop_start); `pred` is a dict with `pos` and optionally `mask`, or just the pos tensor, of the same shape. atom:
    "CA", "CB" (atom37 / atom14) or an integer slot. A row is a site by lddt's rule. Per chain, from float64 sums in a fixed order
    (include/fcz_hip.h, fcz_superpose_dev), so two calls, or the padded and the packed form, give the same bits:
        rot [n, 3, 3], trans [n, 3] float32   x_true ~ rot @ x_pred + trans (rigid_frames' convention); rot is a proper rotation
        rmsd [n] float32                      the RMSD of the sites after the superposition
        sites [n] int32                       the number of sites
        dev [n, L] / [R] float32              every site's deviation after the superposition, 0 where the row is no site
        gdt_counts [n, 5] int32               the sites with dev <= 0.5, 1, 2, 4, 8 AT THIS SUPERPOSITION: GDT is NOT maximised here
                                              (`gdt` searches for the largest count per cutoff, the published kind of number)
        gdt_ts, gdt_ha [n] float32            the mean fraction at 1, 2, 4, 8 and at 0.5, 1, 2, 4 (in float64 from the integers)
        tm [n] float32                        the TM-score AT THIS SUPERPOSITION, normalised by the sites: a lower bound of what
                                              TM-score programs report, which search for the superposition that maximises it
    A chain without sites gets the identity, 0 and scores of 0; one site the identity rotation; two or collinear sites a minimiser.
    apply=True adds pos_aligned, pred's pos moved onto true (apply_transform), enqueued behind the solve with no host round trip.
    It is NOT differentiable. The tensors must be contiguous and lie on the codec's device; ordering against torch is
    decode_tensors'. atom and shapes that differ are checked first, without torch or a device (api.check_superpose)."""
    return _superpose(pred, true, atom, apply, codec, "superpose", None)


def tm_score(pred, true, *, atom="CA", apply: bool = False, iterations: int = 20, levels=None, codec: Optional[Codec] = None) -> dict:
    """predicted coordinates against true ones, both dense tensors on the GPU -> per chain the superposition of `pred` onto `true`
    that MAXIMISES the TM-score over a seeded iterative search, the number TM-score programs report, and the scores at it.

    superpose's `tm` is the TM-score at the least-squares fit, a lower bound: one domain placed right and one swung about a hinge
    spread their error over both. Here every chain is searched from fragments of its sites (the whole chain, halves, quarters, ..
    down to four sites, at half-length steps: 480 seeds for 350 sites); a seed is superposed on its fragment, then up to
    `iterations` times on the sites that lie within a cut of d0 +- 1 A (clamped to 4.5 .. 8 A) of the target, until that set repeats;
    the (seed, round) of the largest TM wins, of equal ones the lowest seed and the earliest round. The definition, deterministic
    to the bit, is fcz_tmscore_dev's in include/fcz_hip.h; the inputs, the site rule and `atom` are superpose's. Per chain:
        rot, trans, rmsd, sites, dev, gdt_counts, gdt_ts, gdt_ha   as superpose returns them, at the winning superposition
        tm [n] float32          the maximised TM-score, normalised by the sites; >= superpose's tm
        seed [n] int32          the number of the winning seed (0: the whole chain)
        selected [n] int32      the sites the winning fit was made on
    levels=k keeps only the first k fragment lengths (None: all); levels=1, iterations=0 is superpose, bit for bit. GDT is NOT
    maximised here: gdt_counts are the counts at the TM-maximising superposition, and `gdt` searches for the maximum per cutoff. apply=True adds pos_aligned as in superpose.
    It is NOT differentiable. Cost: the seeds times a handful of superpositions per chain, where superpose does one.
    atom, shapes, iterations and levels are checked first, without torch or a device (api.check_tm_score)."""
    return _superpose(pred, true, atom, apply, codec, "tm_score", (iterations, levels))


def gdt(pred, true, *, atom="CA", iterations: int = 20, levels=None, runs="all", codec: Optional[Codec] = None) -> dict:
    """predicted coordinates against true ones, both dense tensors on the GPU -> per chain the MAXIMISED GDT counts: for each cutoff of
    0.5, 1, 2, 4 and 8 A (GDT_CUTOFFS) the largest number of sites that some superposition of a seeded search brings under it, the
    kind of number LGA and the TM-score program print and CASP tables hold.

    superpose counts the five cutoffs at the least-squares fit and tm_score at the TM-maximising fit; GDT is defined as a maximum
    per cutoff. Every seed of tm_score's schedule (levels) is searched in up to six runs of at most `iterations` rounds each: one
    with tm_score's cuts ("tm") and one per cutoff c with the constant cut c, the selection of a round being the sites within the
    cut of the target under the fit before. Every fit visited is scored by its five counts, and per cutoff the largest wins, of equal
    ones the lowest seed, then run, then round. The definition, deterministic to the bit, is fcz_gdt_dev's in include/fcz_hip.h;
    the inputs, the site rule and `atom` are superpose's. runs: "all"; "tm" (what the TM-score program's GDT lines amount to, at
    about tm_score's cost); or an iterable of "tm" and cutoffs. Per chain:
        gdt_counts [n, 5] int32               the maxima; >= superpose's, and with the "tm" run >= tm_score's
        gdt_ts, gdt_ha [n] float32            the mean fraction at 1, 2, 4, 8 and at 0.5, 1, 2, 4 (in float64 from the integers)
        sites [n] int32                       the number of sites
        rot [n, 5, 3, 3], trans [n, 5, 3]     float32: the superposition behind each cutoff's count, x_true ~ rot @ x_pred + trans
        seed, run, selected [n, 5] int32      the winning seed, its run (0: "tm", 1 + k: cutoff k) and the sites that fit was made on
        within [n, L] / [R] uint8             bit k: the row is a site within cutoff k under transform k; its popcount is gdt_counts
    There is no `apply`, as there are five transforms per chain:
    apply_transform(pos, out["rot"][:, k].contiguous(), out["trans"][:, k].contiguous(), batch) moves a prediction by the k-th.
    It is NOT differentiable. Cost with runs="all": several times tm_score's. The arguments are checked first, without torch or a
    device (api.check_gdt)."""
    x, ppos, pmask, (slot, iterations, levels, runs) = _pair_inputs(
        "gdt", pred, true, codec, lambda shape, pshape, mshape, t: api.check_gdt(atom, shape, pshape, mshape, iterations, levels, runs))
    if x.rows > 2 ** 31 - 1:
        raise ValueError("sites must fit int32: at most 2^31 - 1 rows per chain")
    torch, dev, n = x.torch, x.dev, x.n
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
    out = dict(gdt_counts=i32(n, 5), sites=i32(n), rot=torch.eye(3, dtype=torch.float32, device=dev).repeat(n, 5, 1, 1),
               trans=torch.zeros((n, 5, 3), dtype=torch.float32, device=dev), seed=i32(n, 5), run=i32(n, 5), selected=i32(n, 5),
               within=torch.zeros(x.lead, dtype=torch.uint8, device=dev))
    if n and x.rows:                                                          # (chains of no rows keep what a chain without sites gets)
        s = CGdtOut(*(out[k].data_ptr() for k in ("gdt_counts", "sites", "rot", "trans", "seed", "run", "selected", "within")))
        torch.cuda.current_stream(dev).synchronize()
        _call(x.codec, "fcz_gdt", x.is_packed, x.pos.data_ptr(), x.mask.data_ptr(), ppos.data_ptr(), _ptr(pmask), _ptr(x.bound), n, x.rows, x.lay, slot,
              levels, iterations, runs, ctypes.byref(s))
        x.codec.synchronize()
    counts, S = out["gdt_counts"].to(torch.float64), out["sites"].to(torch.float64).clamp(min=1.0)
    out["gdt_ts"] = (counts[:, 1:5].sum(dim=1) / (4.0 * S)).to(torch.float32)
    out["gdt_ha"] = (counts[:, 0:4].sum(dim=1) / (4.0 * S)).to(torch.float32)
    return out


def tm_align(a, b=None, pairs=None, *, atom="CA", fragments: bool = True, refine: int = 4, dp_rounds: int = 20, gaps=(0.6, 0.0), iterations: int = 20,
             levels=None, transform=None, codec: Optional[Codec] = None) -> dict:
    """two sets of chains as dense tensors on the GPU -> for every requested pair of DIFFERENT chains a TM-align-style structural
    alignment: which residues of a correspond to which of b, the rigid motion that lays a onto b, and the TM-scores.

    lddt, superpose and tm_score compare two tensors row for row. Here the chains differ in length and sequence and the
    correspondence is what is looked for. `a` and `b` are dicts as decode_tensors / tensor_batches return, each padded (pos
    [n, L, A, 3], mask, optionally length) or packed (pos [R, A, 3], mask, cu_seqlens), each in its own form, of one layout; b=None:
    b is a. pairs: int32 [m, 2] on the device, (chain of a, chain of b); None: every i < j of a (b=None) or every (i, j). A site is
    a row inside its chain whose mask at `atom` is set and whose coordinates are finite. Chains of at most 1024 rows.
    The search (the definition, deterministic to the bit: include/fcz_hip.h, fcz_tmalign_dev): gapless shifts and, with fragments,
    pairs of fragments seed a transform; a Needleman-Wunsch over the scores 1 / (1 + d^2 / d0^2) with free end gaps and the gap
    penalties `gaps` in turn gives an alignment, its TM-maximising fit (refine rounds) the next transform, for up to dp_rounds rounds;
    the best alignment then gets tm_score's full search (iterations, levels). Per pair:
        rot [m, 3, 3], trans [m, 3] float32   x_b ~ rot @ x_a + trans
        tm [m] float32                        the TM-score normalised by the shorter chain; tm_a, tm_b: by a's and by b's sites.
                                              LOWER BOUNDS of what TM-align prints (no secondary-structure seed, one search for all three)
        aligned, sites_a, sites_b [m] int32   the aligned pairs and the sites of the two chains; rmsd [m] over the pairs
        map [m, wa] int32                     for every row of chain a the chain-relative row of b it is aligned with, -1 elsewhere
        dev [m, wa] float32                   the deviation of an aligned row; wa = L, or the longest chain of a packed a
        seed [m] int32                        the winning seed; status [m] int32: 0, 1 (a chain longer than its width), 2 (no such chain)
        pairs [m, 2] int32                    the pairs that were aligned
    transform=(rot [m, 3, 3], trans [m, 3]) runs ONE dynamic programme per pair from the caller's transforms instead, with the gap
    gaps[0] (fcz_tmalign_dp_dev), and returns map, aligned and pairs alone; numpy reproduces that integer DP bit for bit.
    It is NOT differentiable. The arguments are checked first, without torch or a device (api.check_tm_align)."""
    what = "tm_align"
    da = dict(a) if isinstance(a, dict) else {"pos": a}
    same = b is None
    db = da if same else (dict(b) if isinstance(b, dict) else {"pos": b})
    _need(what, da, of=" of a")
    _need(what, db, of=" of b")
    shape_a, shape_b = tuple(getattr(da["pos"], "shape", ())), tuple(getattr(db["pos"], "shape", ()))
    tshapes = None if transform is None else tuple(tuple(getattr(t, "shape", ())) for t in transform)
    pshape = None if pairs is None else tuple(getattr(pairs, "shape", ()))
    width = lambda d, s: s[1] if len(s) == 4 and d.get("cu_seqlens") is None else None
    checked = api.check_tm_align(atom, shape_a, shape_b, width(da, shape_a), width(db, shape_b), pshape, fragments, refine, dp_rounds, gaps, iterations, levels, tshapes)
    slot, frag, refine, dp_rounds, gs, iterations, levels = checked
    packed = lambda d, s: d.get("cu_seqlens") is not None and len(s) == 3
    xa = _dense_checked(what, "Codec.tm_align", codec, da, shape_a, packed(da, shape_a), "full", False)
    xb = xa if same else _dense_checked(what, "Codec.tm_align", xa.codec, db, shape_b, packed(db, shape_b), "full", False)
    torch, dev = xa.torch, xa.dev

    def width_of(x):
        if not x.is_packed:
            return max(x.rows, 1)
        return max(int((x.bound[1:] - x.bound[:-1]).max()) if x.n else 1, 1)
    wa, wb = width_of(xa), width_of(xb)
    api.check_tm_align(atom, shape_a, shape_b, wa, wb)
    if pairs is None:
        pairs = torch.from_numpy(api.tm_align_pairs(xa.n, xb.n, same)).to(dev)
    else:
        pairs = _on_device(torch, what, dev, "pairs", pairs, pshape, (torch.int32,))
    m = int(pairs.shape[0])
    sets = [CChainSet(x.pos.data_ptr(), x.mask.data_ptr(), None if x.is_packed else _ptr(x.bound), _ptr(x.bound) if x.is_packed else None, x.n, x.rows)
            for x in (xa, xb)]
    c = xa.codec
    if transform is not None:
        rot = _on_device(torch, what, dev, "rot", transform[0], (m, 3, 3), (torch.float32,))
        trans = _on_device(torch, what, dev, "trans", transform[1], (m, 3), (torch.float32,))
        out = dict(map=torch.full((m, wa), -1, dtype=torch.int32, device=dev), aligned=torch.zeros((m,), dtype=torch.int32, device=dev), pairs=pairs)
        if m:
            torch.cuda.current_stream(dev).synchronize()
            _lib.check(c.lib.fcz_tmalign_dp_dev(c.ctx, ctypes.byref(sets[0]), ctypes.byref(sets[1]), pairs.data_ptr(), m, wa, wb, xa.lay, slot, rot.data_ptr(),
                                                trans.data_ptr(), gs[0], out["map"].data_ptr(), out["aligned"].data_ptr()), "fcz_tmalign_dp_dev")
            c.synchronize()
        return out
    out = {k: torch.empty((m,) + ((wa,) if tail == "wa" else tail), dtype=getattr(torch, dt), device=dev) for k, dt, tail in TM_ALIGN_OUTPUTS}
    if m:
        par = CTmAlignParams(frag, refine, dp_rounds, len(gs), (ctypes.c_double * 4)(*gs), levels, iterations)
        s = CTmAlignOut(*(out[k].data_ptr() for k, _, _ in TM_ALIGN_OUTPUTS))
        torch.cuda.current_stream(dev).synchronize()
        _lib.check(c.lib.fcz_tmalign_dev(c.ctx, ctypes.byref(sets[0]), ctypes.byref(sets[1]), pairs.data_ptr(), m, wa, wb, xa.lay, slot, ctypes.byref(par),
                                         ctypes.byref(s)), "fcz_tmalign_dev")
        c.synchronize()
    out["pairs"] = pairs
    return out


def _superpose(pred, true, atom, apply, codec, what, search):
    """superpose (search None) and tm_score (search = (iterations, levels)): the shared checks, outputs and apply step"""
    if search is None:
        x, ppos, pmask, slot = _pair_inputs(what, pred, true, codec, lambda shape, pshape, mshape, t: api.check_superpose(atom, shape, pshape, mshape))
    else:
        x, ppos, pmask, (slot, iterations, levels) = _pair_inputs(
            what, pred, true, codec, lambda shape, pshape, mshape, t: api.check_tm_score(atom, shape, pshape, mshape, *search))
    if x.rows > 2 ** 31 - 1:
        raise ValueError("sites must fit int32: at most 2^31 - 1 rows per chain")
    torch, dev, n = x.torch, x.dev, x.n
    out = dict(rot=torch.empty((n, 3, 3), dtype=torch.float32, device=dev), trans=torch.empty((n, 3), dtype=torch.float32, device=dev),
               rmsd=torch.empty((n,), dtype=torch.float32, device=dev), sites=torch.empty((n,), dtype=torch.int32, device=dev),
               dev=torch.zeros(x.lead, dtype=torch.float32, device=dev), gdt_counts=torch.empty((n, 5), dtype=torch.int32, device=dev),
               tm=torch.empty((n,), dtype=torch.float32, device=dev))
    keys = ("rot", "trans", "rmsd", "sites", "gdt_counts", "tm", "dev")
    if search is not None:
        out.update(seed=torch.empty((n,), dtype=torch.int32, device=dev), selected=torch.empty((n,), dtype=torch.int32, device=dev))
        keys += ("seed", "selected")
    if apply:
        out["pos_aligned"] = torch.empty_like(ppos)
    solve = bool(n and x.rows)
    if n and not solve:                                                       # chains of no rows: what a chain without sites gets
        out["rot"].copy_(torch.eye(3, device=dev).expand(n, 3, 3))
        for k in keys:
            if k not in ("rot", "dev"):
                out[k].zero_()
    torch.cuda.current_stream(dev).synchronize()
    if solve:
        args = (x.pos.data_ptr(), x.mask.data_ptr(), ppos.data_ptr(), _ptr(pmask), _ptr(x.bound), n, x.rows, x.lay, slot)
        if search is None:
            s = CSuperposeOut(*(out[k].data_ptr() for k in keys))
            _call(x.codec, "fcz_superpose", x.is_packed, *args, ctypes.byref(s))
        else:
            s = CTmScoreOut(*(out[k].data_ptr() for k in keys))
            _call(x.codec, "fcz_tmscore", x.is_packed, *args, levels, iterations, ctypes.byref(s))
    if apply:
        _apply_transform(x._replace(pos=ppos, mask=pmask), out["rot"], out["trans"], out["pos_aligned"])
    x.codec.synchronize()
    counts, S = out["gdt_counts"].to(torch.float64), out["sites"].to(torch.float64).clamp(min=1.0)
    out["gdt_ts"] = (counts[:, 1:5].sum(dim=1) / (4.0 * S)).to(torch.float32)
    out["gdt_ha"] = (counts[:, 0:4].sum(dim=1) / (4.0 * S)).to(torch.float32)
    return out


def _apply_transform(x, rot, trans, out):
    """fcz_superpose_apply_dev / _packed_dev on a record, whose mask may be None, into `out`, enqueued on the codec's stream"""
    if x.n == 0:                                                              # (packed rows without a chain: covered by none)
        out.zero_()
    elif out.numel():
        _call(x.codec, "fcz_superpose_apply", x.is_packed, x.pos.data_ptr(), _ptr(x.mask), _ptr(x.bound), x.n, x.rows, x.lay, rot.data_ptr(), trans.data_ptr(),
              out.data_ptr())


def apply_transform(pos, rot, trans, batch=None, *, mask=None, length=None, cu_seqlens=None, codec: Optional[Codec] = None):
    """dense coordinates on the GPU moved by one rigid transform per chain -> pos_out of the shape of pos: rot[e] @ x + trans[e] for
    every slot whose mask is set (mask=None: every slot) in the rows of chain e, 0 elsewhere. The apply step of superpose alone, for
    transforms that came from elsewhere.

    pos [n, L, A, 3] float32, or the packed [R, A, 3] beside cu_seqlens [n + 1]; rot [n, 3, 3], trans [n, 3] float32. The chains come
    from `batch`, a dict as decode_tensors returns (its length, ignored beside crop_start, or its cu_seqlens; its mask is NOT used:
    it says which atoms the target has, not which were predicted), or from the keywords length / cu_seqlens. pos may also be a dict
    with `pos` and optionally `mask`. The arithmetic is float32 in a fixed order, x' = ((r00 x + r01 y) + r02 z) + tx with every
    operation rounded (include/fcz_hip.h, fcz_superpose_apply_dev), so numpy reproduces it bit for bit."""
    if isinstance(pos, dict):
        mask = pos.get("mask") if mask is None else mask
        pos = pos.get("pos")
    d = {k: batch[k] for k in ("length", "cu_seqlens", "crop_start") if batch is not None and batch.get(k) is not None}
    if length is not None:
        d["length"] = length
    if cu_seqlens is not None:
        d["cu_seqlens"] = cu_seqlens
    d.update(pos=pos, mask=mask)
    _need("apply_transform", d, ("pos",))
    shape = tuple(getattr(pos, "shape", ()))
    is_packed = d.get("cu_seqlens") is not None and len(shape) == 3
    if len(shape) != (3 if is_packed else 4) or shape[-1] != 3 or shape[-2] not in _WIDTH_LAYOUT:
        raise ValueError(f"pos must be float32 [n, L, A, 3], or [R, A, 3] beside cu_seqlens, with A = 37, 14 or 4, not {shape}")
    n = (int(getattr(d["cu_seqlens"], "shape", (1,))[0]) - 1) if is_packed else shape[0]
    for key, v, want in (("rot", rot, (n, 3, 3)), ("trans", trans, (n, 3))):
        if tuple(getattr(v, "shape", ())) != want:
            raise ValueError(f"{key} must be float32 {want}, one transform per chain, not {tuple(getattr(v, 'shape', ()))}")
    if mask is not None and tuple(getattr(mask, "shape", ())) != shape[:-1]:
        raise ValueError(f"mask must have the shape {shape[:-1]}, not {tuple(getattr(mask, 'shape', ()))}")
    x = _dense_checked("apply_transform", "Codec.apply_transform", codec, d, shape, is_packed, aatype=False)
    _on_device(x.torch, "apply_transform", x.dev, "rot", rot, (n, 3, 3), (x.torch.float32,))
    _on_device(x.torch, "apply_transform", x.dev, "trans", trans, (n, 3), (x.torch.float32,))
    if x.rows > 2 ** 31 - 1:
        raise ValueError("at most 2^31 - 1 rows per chain")
    out = x.torch.empty_like(pos)
    x.torch.cuda.current_stream(x.dev).synchronize()
    _apply_transform(x, rot, trans, out)
    x.codec.synchronize()
    return out


def _hbond_alloc(torch, dev, rows):
    """the four H-bond tables for the leading shape `rows`"""
    return {k: torch.empty(tuple(rows) + (2,), dtype=getattr(torch, dt), device=dev) for k, dt in api.HBOND_TABLES}


def _ss_alloc(torch, dev, rows):
    """ss and ss_mask for the leading shape `rows`; ss_mask is written as 0 / 1 bytes"""
    return dict(ss=torch.empty(tuple(rows), dtype=torch.uint8, device=dev), ss_mask=torch.empty(tuple(rows), dtype=torch.uint8, device=dev).view(torch.bool))


def _hbonds_into(x, tables):
    """fcz_hbond_dev / _packed_dev on a record into the four `tables`, enqueued on the codec's stream"""
    _call(x.codec, "fcz_hbond", x.is_packed, x.pos.data_ptr(), x.mask.data_ptr(), _ptr(x.aatype), _ptr(x.bound), x.n, x.rows, x.lay,
          *(tables[k].data_ptr() for k, _ in api.HBOND_TABLES))


def _labels_into(x, tables, out):
    """fcz_dssp_labels_dev / _packed_dev from the acceptor tables of `tables` into out["ss"], out["ss_mask"], enqueued alike"""
    _call(x.codec, "fcz_dssp_labels", x.is_packed, x.pos.data_ptr(), x.mask.data_ptr(), _ptr(x.aatype), _ptr(x.bound), x.n, x.rows, x.lay,
          tables["hbond_acc_index"].data_ptr(), tables["hbond_acc_energy"].data_ptr(), out["ss"].data_ptr(), out["ss_mask"].data_ptr())


def _dssp_into(x, tables, out):
    """both steps behind one another on the codec's stream"""
    _hbonds_into(x, tables)
    _labels_into(x, tables, out)


def backbone_hbonds(batch=None, *, codec: Optional[Codec] = None, **tensors) -> dict:
    """dense tensors on the GPU -> DSSP's four hydrogen-bond columns: the two best acceptors of every residue's N-H and the two best
    donors onto its C=O, inside its own chain, with no L x L array.

    `batch` is the dict decode_tensors / tensor_batches return, padded or packed, or the tensors come as keywords, recognised as
    neighbor_graph recognises them: pos [n, L, A, 3] float32, mask [n, L, A], optionally aatype [n, L] uint8 (a proline has no
    amide hydrogen; none: no row is proline) and length [n]; or the packed pos [R, A, 3], mask [R, A], aatype [R] with cu_seqlens
    [n + 1]. `length` is ignored beside crop_start. Only N, CA, C and O are read, so the three layouts give the same result.
        hbond_acc_index [.., 2] int32, hbond_acc_energy [.., 2] float32   the acceptors of the row's N-H, lowest energy first
        hbond_don_index, hbond_don_energy                                 the donors onto the row's C=O
    An index is the row inside the entry (padded) or the global row (packed), as nbr_index; -1 / 0.0 where there is none. The
    energy is Kabsch and Sander's electrostatic one in kcal/mol (include/fcz_hip.h, fcz_hbond_dev), in float32 with every operation
    rounded and no rounding to 0.001; an entry is listed when its energy is below 0, and is a hydrogen bond when below -0.5.
    Reproducible bit for bit; NOT differentiable. The shapes are checked first, without torch or a device (api.check_dssp)."""
    x, _ = _inputs("backbone_hbonds", "Codec.secondary_structure", batch, tensors, codec, lambda d: api.check_dssp("backbone_hbonds", d))
    out = _hbond_alloc(x.torch, x.dev, x.lead)
    if out["hbond_acc_index"].numel():
        x.torch.cuda.current_stream(x.dev).synchronize()
        _hbonds_into(x, out)
        x.codec.synchronize()
    return out


def secondary_structure(batch=None, *, hbonds: Optional[dict] = None, codec: Optional[Codec] = None, **tensors) -> dict:
    """dense tensors on the GPU -> the DSSP secondary structure of every residue (Kabsch & Sander 1983) and the hydrogen bonds it
    rests on.

    The inputs are backbone_hbonds'. hbonds: a dict with hbond_acc_index and hbond_acc_energy [.., 2] to label from instead of
    computing them (what backbone_hbonds returned, or tables edited since); the labels depend on the acceptor table alone.
        ss [n, L] / [R] uint8      the code of the label in foldcomp.SS_CLASSES = ("-", "H", "B", "E", "G", "I", "T", "S");
                                   foldcomp.SS3_OF_SS8[ss] reduces it to helix 0 / strand 1 / coil 2
        ss_mask bool               True where the row has N, CA, C and O: elsewhere ss is 0 and means nothing
        hbond_* [.., 2]            the four tables (with hbonds=: the tables given)
    The priority is the 1983 one, H > B, E > G > I > T > S; the rules are in include/fcz_hip.h (fcz_dssp_labels_dev). Sheet labels,
    bridge partners, accessibility and bonds between chains are not computed. A cropped window's labels are the window's own: a
    strand whose partner lies outside the window is not seen. Reproducible bit for bit; NOT differentiable."""
    what = "secondary_structure"
    x, _ = _inputs(what, "Codec.secondary_structure", batch, tensors, codec, lambda d: api.check_dssp(what, d, hbonds))
    if hbonds is not None:
        hbonds = dict(hbonds)
        for key, dt in api.HBOND_TABLES[:2]:
            hbonds[key] = _on_device(x.torch, what, x.dev, key, hbonds[key], x.lead + (2,), (getattr(x.torch, dt),))
    tables = _hbond_alloc(x.torch, x.dev, x.lead) if hbonds is None else hbonds
    out = _ss_alloc(x.torch, x.dev, x.lead)
    if out["ss"].numel():
        x.torch.cuda.current_stream(x.dev).synchronize()
        if hbonds is None:
            _hbonds_into(x, tables)
        _labels_into(x, tables, out)
        x.codec.synchronize()
    return dict(out, **tables)


def _sasa_alloc(torch, dev, rows):
    """sasa, rsa and sasa_mask for the leading shape `rows`; sasa_mask is written as 0 / 1 bytes, rsa by _rsa behind the call"""
    return dict(sasa=torch.empty(tuple(rows), dtype=torch.float32, device=dev), rsa=torch.zeros(tuple(rows), dtype=torch.float32, device=dev),
                sasa_mask=torch.empty(tuple(rows), dtype=torch.uint8, device=dev).view(torch.bool))


def _sasa_work(torch, dev, shape, points=None):
    """what fcz_sasa_dev needs beside the outputs -> (the surface points on the device, the per-atom counts of `shape`)"""
    pts = api.sphere_points(api.SASA_POINTS) if points is None else points
    return torch.from_numpy(pts).to(dev), torch.empty(tuple(shape), dtype=torch.int16, device=dev)


def _sasa_into(x, table, probe, points_t, counts_t, out):
    """fcz_sasa_dev / _packed_dev on a record into counts_t, out["sasa"], out["sasa_mask"], enqueued on the codec's stream; table: the radii
    as a contiguous float32 [21, A] array on the host, or None"""
    _call(x.codec, "fcz_sasa", x.is_packed, x.pos.data_ptr(), x.mask.data_ptr(), _ptr(x.aatype), _ptr(x.bound), x.n, x.rows, x.lay,
          None if table is None else table.ctypes.data, float(probe), points_t.data_ptr(), int(points_t.shape[0]), counts_t.data_ptr(),
          out["sasa"].data_ptr(), out["sasa_mask"].data_ptr())


def _rsa(torch, sasa, sasa_mask, aatype):
    """sasa / foldcomp.MAX_ASA[aatype]: one division on the device; 0 where the maximum is 0, where sasa_mask is off, without aatype"""
    if aatype is None or not sasa.numel():
        return torch.zeros_like(sasa)
    mx = torch.from_numpy(api.MAX_ASA).to(sasa.device)[aatype.clamp(max=20).long()]
    return torch.where((mx > 0) & sasa_mask, sasa / mx, torch.zeros_like(sasa))


def solvent_accessibility(batch=None, *, probe: float = 1.4, n_points: int = 128, points=None, radii="bondi", codec: Optional[Codec] = None,
                          **tensors) -> dict:
    """dense tensors on the GPU -> the solvent-accessible surface of every residue (Shrake & Rupley 1973), every atom of a chain
    against every other atom of it, with no atoms x atoms array.

    The inputs are secondary_structure's: `batch` is the dict decode_tensors / tensor_batches return, padded or packed, or the
    tensors come as keywords: pos [n, L, A, 3] float32, mask [n, L, A], aatype [n, L] uint8 (needed for atom14, where a slot's
    atom depends on the type; without it rsa is 0) and optionally length [n]; or the packed pos [R, A, 3], mask [R, A], aatype [R]
    with cu_seqlens [n + 1]. `length` is ignored beside crop_start. Every slot whose mask is set and whose coordinates are finite is
    an atom; only atoms of the same chain bury each other.
        sasa [n, L] / [R] float32   the accessible surface of the residue in square Angstrom
        rsa float32                 sasa / foldcomp.MAX_ASA[aatype] (Tien et al. 2013): the relative accessibility, usually cut at
                                    0.05 (buried) .. 0.5 (exposed); 0 where the maximum is 0 (aatype 20), sasa_mask is off or
                                    there is no aatype. One torch division, not part of the kernel.
        sasa_mask bool              True where the row has an atom
        sasa_points [.., A] int16   the surface points of every atom that no other atom buries, 0 .. P
    probe: the radius of the solvent sphere (water: 1.4). n_points: the surface points per atom, foldcomp.sphere_points(n_points);
    points: the unit directions [P, 3] themselves instead, 1 <= P <= 1024 (an array or tensor; used as given). radii: "bondi" (C
    1.70, N 1.55, O 1.52, S 1.80 by the atom's element; the chain's OXT is left out, so the layouts agree) or an array [21, A] indexed
    [aatype][slot], 0 for a slot that holds no atom; radius + probe must lie in [0.5, 8). The arithmetic is fixed (include/fcz_hip.h,
    fcz_sasa_dev): atom37 and atom14 give the same bits. A cropped window's values are the window's own: atoms outside it bury
    nothing, so residues at the cut look more exposed than in the whole chain. Reproducible bit for bit; NOT differentiable. The
    arguments are checked first, without torch or a device (api.check_sasa)."""
    x, (_, _, pts, table) = _inputs("solvent_accessibility", "Codec.solvent_accessibility", batch, tensors, codec,
                                    lambda d: api.check_sasa("solvent_accessibility", d, probe, n_points, points, radii))
    out = _sasa_alloc(x.torch, x.dev, x.lead)
    points_t, counts = _sasa_work(x.torch, x.dev, x.lead + (x.A,), pts)
    if out["sasa"].numel():
        x.torch.cuda.current_stream(x.dev).synchronize()
        _sasa_into(x, table, probe, points_t, counts, out)
        x.codec.synchronize()
        out["rsa"] = _rsa(x.torch, out["sasa"], out["sasa_mask"], x.aatype)
    return dict(out, sasa_points=counts)


def _viol_alloc(torch, dev, rows, A, n):
    """the ten output tensors of fcz_violations_dev (api.VIOLATION_OUTPUTS) for the leading shape `rows`, width A and n chains; the masks
    are written as 0 / 1 bytes"""
    out = {}
    for key, dt, tail in api.VIOLATION_OUTPUTS:
        shape = (n, 4) if tail == "n4" else tuple(rows) + ((A,) if tail == "A" else tail)
        make = torch.zeros if tail == "n4" else torch.empty                 # (chains without a row: the call is not made and the counts are 0)
        t = make(shape, dtype=torch.uint8 if dt == "bool" else getattr(torch, dt), device=dev)
        out[key] = t.view(torch.bool) if dt == "bool" else t
    return out


def _viol_into(x, table, tolerance, link_factor, out):
    """fcz_violations_dev / _packed_dev on a record into the tensors of _viol_alloc, enqueued on the codec's stream; table: the radii as a
    contiguous float32 [21, A] array on the host, or None"""
    c_out = CViolationsOut(*(out[key].data_ptr() for key, _, _ in api.VIOLATION_OUTPUTS))
    _call(x.codec, "fcz_violations", x.is_packed, x.pos.data_ptr(), x.mask.data_ptr(), _ptr(x.aatype), _ptr(x.bound), x.n, x.rows, x.lay,
          None if table is None else table.ctypes.data, float(tolerance), float(link_factor), ctypes.byref(c_out))


def violations(batch=None, *, tolerance: float = 1.5, link_factor: float = 12.0, radii="bondi", codec: Optional[Codec] = None, **tensors) -> dict:
    """dense tensors on the GPU -> the structural violations of every chain: atoms of different residues that sit inside each other,
    and peptide links whose length or angles are far from a peptide's, with no atoms x atoms array.

    The inputs are solvent_accessibility's: `batch` is the dict decode_tensors / tensor_batches return, padded or packed, or the
    tensors come as keywords: pos [n, L, A, 3] float32, mask [n, L, A], aatype [n, L] uint8 (needed for atom14; without it no
    disulfide is excluded and no link is a proline's) and optionally length [n]; or the packed pos [R, A, 3], mask [R, A], aatype [R]
    with cu_seqlens [n + 1]. `length` is ignored beside crop_start. Every slot whose mask is set, whose coordinates are finite and
    whose radius is not 0 is an atom; only atoms of the same chain are compared.
        clash_atom [.., A] uint8     1 where the slot's atom clashes: it lies closer than (Ri + Rj) - tolerance to an atom of
                                     another residue that is neither its peptide-bond partner (C and the next N) nor, SG to SG
                                     between two CYS, its disulfide partner
        clash_count [..] int32       the clashing (atom of the residue, atom of another residue) pairs
        clash_depth [..] float32     the deepest overlap (Ri + Rj) - tolerance - distance among them; 0 when none
        clash_partner [..] int32     the row, counted inside the chain, of the atom at that depth (the smallest on a tie); -1 when none
        viol_mask [..] bool          True where the row has an atom
        link_mask [..] bool          True where the link to the NEXT row exists: CA and C here, N and CA there
        link_length [..] float32     the C-N' distance
        link_cos [.., 2] float32     the cosines of the angles CA-C-N' and C-N'-CA'
        link_violation [..] uint8    bit 0: the length is further than link_factor sigmas from 1.329 (1.341 before a PRO); bit 1 / bit
                                     2: the first / second cosine is further than link_factor sigmas from -0.4473 / -0.5203
        chain_counts [n, 4] int64    per chain: atoms, clashing pairs (each once), links with bit 0, links with bit 1 or 2
    tolerance: how far two atoms may overlap (AlphaFold: 1.5). link_factor: the sigmas a link may deviate (AlphaFold: 12). radii:
    "bondi" (solvent_accessibility's table, the chain's OXT left out) or an array [21, A] indexed [aatype][slot], 0 for a slot that
    holds no atom, every other radius in [0.5, 8). The arithmetic is fixed (include/fcz_hip.h, fcz_violations_dev): atom37 and atom14
    give the same values. Bonds and angles inside a residue are not checked. A cropped window's values are the window's own.
    Reproducible bit for bit; NOT differentiable (violation_loss is the loss on the same atoms, pairs and links). The arguments are
    checked first, without torch or a device (api.check_violations)."""
    x, checked = _inputs("violations", "Codec.violations", batch, tensors, codec, lambda d: api.check_violations("violations", d, tolerance, link_factor, radii))
    out = _viol_alloc(x.torch, x.dev, x.lead, x.A, x.n)
    if out["clash_count"].numel():
        x.torch.cuda.current_stream(x.dev).synchronize()
        _viol_into(x, checked[2], tolerance, link_factor, out)
        x.codec.synchronize()
    return out


_violation_autograd = {}


def _violation_function(torch):
    """the torch.autograd.Function of violation_loss, made once torch is there (this module imports without it)"""
    if _violation_autograd:
        return _violation_autograd["loss"]
    from torch.autograd.function import once_differentiable

    class ViolationLoss(torch.autograd.Function):
        """pred pos -> (clash_loss [.., A], link_loss [.., 3]) (fcz_violation_loss_dev); `call` holds everything else of the call and
        receives counts. The backward is the gradient kernel (fcz_violation_loss_grad_dev) on the saved pos: nothing else is kept
        from the forward."""

        @staticmethod
        def forward(ctx, ppos, call):
            ctx.call = call
            ctx.save_for_backward(ppos)
            return call.value(ppos)

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_clash, grad_link):
            (ppos,) = ctx.saved_tensors
            return ctx.call.gradient(ppos, grad_clash, grad_link), None

    _violation_autograd["loss"] = ViolationLoss
    return ViolationLoss


class _ViolationLossCall:
    """one call of violation_loss: the checked tensors (mask: the two masks combined), the radii and the parameters; value() and
    gradient() enqueue the two kernels on the codec's stream between a wait for torch's stream and codec.synchronize(), as every
    analysis function does"""

    def __init__(self, x, table, tolerance, link_factor):
        self.x, self.table, self.tolerance, self.link_factor = x, table, float(tolerance), float(link_factor)
        self.counts = None

    def _run(self, name, ppos, *tensors):
        x = self.x
        x.torch.cuda.current_stream(x.dev).synchronize()
        _call(x.codec, name, x.is_packed, ppos.data_ptr(), x.mask.data_ptr(), _ptr(x.aatype), _ptr(x.bound), x.n, x.rows, x.lay,
              None if self.table is None else self.table.ctypes.data, self.tolerance, self.link_factor, *(t.data_ptr() for t in tensors))
        x.codec.synchronize()

    def value(self, ppos):
        x, torch = self.x, self.x.torch
        clash = torch.zeros(x.lead + (x.A,), dtype=torch.float32, device=x.dev)
        link = torch.zeros(x.lead + (3,), dtype=torch.float32, device=x.dev)
        self.counts = torch.zeros((x.n, 2), dtype=torch.int64, device=x.dev)
        if link.numel():
            self._run("fcz_violation_loss", ppos, clash, link, self.counts)
        return clash, link

    def gradient(self, ppos, w_clash, w_link):
        x, torch = self.x, self.x.torch
        grad = torch.zeros(x.shape, dtype=torch.float32, device=x.dev)
        if grad.numel():
            w_clash = torch.zeros(x.lead + (x.A,), dtype=torch.float32, device=x.dev) if w_clash is None else w_clash.contiguous()
            w_link = torch.zeros(x.lead + (3,), dtype=torch.float32, device=x.dev) if w_link is None else w_link.contiguous()
            self._run("fcz_violation_loss_grad", ppos, w_clash, w_link, grad)
        return grad


def violation_loss(pred, true, *, tolerance: float = 1.5, link_factor: float = 12.0, radii="bondi", codec: Optional[Codec] = None) -> dict:
    """predicted coordinates on the GPU -> dict(clash_loss, link_loss, clash_chain, bond_chain, angle_chain, violation_chain, loss): the
    between-residue part of AlphaFold's structural-violation loss, a LOSS: differentiable with respect to pred's pos, with a fused
    backward on the GPU and no atoms x atoms array in either direction.

    `pred` is the pos tensor, or a dict with `pos` and optionally `mask`. `true` is the dict decode_tensors / tensor_batches return,
    padded (mask [n, L, A], aatype [n, L], optionally length [n]), packed (mask [R, A], aatype [R], cu_seqlens [n + 1]) or a window
    with crop_start: it supplies mask, aatype (needed for atom14; without it no disulfide is excluded and no link is a proline's)
    and the chains. Its pos is NOT read: the loss looks at the prediction alone. A slot is used when it is set in both masks. Atoms,
    clashing pairs, links, tolerance, link_factor and radii are violations' exactly, on pred's pos.
        clash_loss [.., A] float32     for every atom the sum of (Ri + Rj) - tolerance - distance over the atoms of other residues
                                       it clashes with; every pair stands in both of its atoms (AlphaFold's per_atom_loss_sum)
        link_loss [.., 3] float32      for the link to the NEXT row, how far the C-N' length and the cosines of CA-C-N' and C-N'-CA'
                                       lie outside link_factor sigmas: (|x - x0| - link_factor * sigma)+, 0 where there is no link
        clash_chain [n] float32        the sum of clash_loss over the chain's atoms, divided by max(atoms, 1)
        bond_chain [n] float32         the mean of the length term over the chain's links (0 without a link)
        angle_chain [n] float32        the mean of the first cosine term plus the mean of the second
        violation_chain [n] float32    the three added
        loss scalar float32            the mean of violation_chain over the chains that have an atom (0 without one)
    When pred's pos requires a gradient (and gradients are enabled) all seven carry a graph: loss.backward() runs the gradient kernel
    once and leaves d loss / d pos in pos.grad. Gradients flow to pred's pos and to nothing else; the graph can be walked once and
    not differentiated twice. Under torch.no_grad(), or for a pos that needs no gradient, only the value kernel runs. Every sum has
    a fixed order (an atom's partners in float32 in ascending (row, slot) on the device, chains in float64, no float atomics in
    either direction): value and gradient are reproducible bit for bit. atom37 and atom14 agree to rounding, not on bits: the slot
    order differs.

    Two departures from AlphaFold's code: there are no epsilons (its sqrt(1e-10 + d2) and 1e-6 + norm), the few places where a
    direction does not exist -- coincident atoms, a bond of length 0 -- have the gradient 0 instead; and the within-residue bounds,
    its third term, are not computed (their tables are not part of this package).

    The tensors must be contiguous and lie on the codec's device; ordering against torch is decode_tensors'. The arguments are
    checked first, without torch or a device (api.check_violation_loss)."""
    what = "violation_loss"
    if not isinstance(true, dict):
        raise TypeError(f"{what}: true must be a dict with mask, aatype and length or cu_seqlens")
    p = dict(pred) if isinstance(pred, dict) else {"pos": pred}
    _need(what, p, ("pos",), " of pred")
    _need(what, true, ("mask",), " of true")
    ppos, pmask = p["pos"], p.get("mask")
    d = dict(true, pos=ppos)
    shape = tuple(getattr(ppos, "shape", ()))
    if pmask is not None and tuple(getattr(pmask, "shape", ())) != shape[:-1]:
        raise ValueError(f"pred mask must have the shape {shape[:-1]}, not {tuple(getattr(pmask, 'shape', ()))}")
    shape, is_packed, table = api.check_violation_loss(what, d, tolerance, link_factor, radii)
    x = _dense_checked(what, "Codec.violation_loss", codec, d, shape, is_packed, pos_rule="full")
    torch = x.torch
    if pmask is not None:
        pmask = _on_device(torch, what, x.dev, "pred mask", pmask, shape[:-1], (torch.bool, torch.uint8)).view(torch.uint8)
        x = x._replace(mask=((x.mask != 0) & (pmask != 0)).view(torch.uint8))
    call = _ViolationLossCall(x, table, tolerance, link_factor)
    if torch.is_grad_enabled() and ppos.requires_grad:
        clash, link = _violation_function(torch).apply(ppos, call)
    else:
        clash, link = call.value(ppos.detach())
    atoms, links = call.counts[:, 0], call.counts[:, 1]
    rows64 = torch.cat([clash.to(torch.float64).sum(dim=-1, keepdim=True), link.to(torch.float64)], dim=-1)      # [.., 4]: clash, bond, cos0, cos1
    if x.is_packed:
        _, chain_sum = _autograd_functions(torch)
        at = x.bound.to(torch.int64)
        sums = torch.stack([chain_sum.apply(rows64[:, k].contiguous(), at) for k in range(4)], dim=1)
    else:
        sums = rows64.sum(dim=1)
    per_atom, per_link = atoms.clamp(min=1).to(torch.float64), links.clamp(min=1).to(torch.float64)
    clash_chain, bond_chain = sums[:, 0] / per_atom, sums[:, 1] / per_link
    angle_chain = sums[:, 2] / per_link + sums[:, 3] / per_link
    chain = clash_chain + bond_chain + angle_chain
    has = atoms > 0
    loss = (torch.where(has, chain, chain.new_zeros(())).sum() / has.sum().clamp(min=1).to(torch.float64)).to(torch.float32)
    f32 = torch.float32
    return dict(clash_loss=clash, link_loss=link, clash_chain=clash_chain.to(f32), bond_chain=bond_chain.to(f32), angle_chain=angle_chain.to(f32),
                violation_chain=chain.to(f32), loss=loss)


def _frames_alloc(torch, dev, rows, fgroups):
    """the three output tensors of fcz_frames_dev for the leading shape `rows`; frame_mask is written as 0 / 1 bytes"""
    g = () if fgroups == 0 else (8,)
    return dict(rot=torch.empty(tuple(rows) + g + (3, 3), dtype=torch.float32, device=dev),
                trans=torch.empty(tuple(rows) + g + (3,), dtype=torch.float32, device=dev),
                frame_mask=torch.empty(tuple(rows) + g, dtype=torch.uint8, device=dev).view(torch.bool))


def _frames_into(x, fgroups, out):
    """fcz_frames_dev on a record into the tensors of _frames_alloc, enqueued on the codec's stream. Frames use atoms of their own row
    only, so the packed form goes as one entry of R rows with no length"""
    bound, n = (None, 1) if x.is_packed else (x.bound, x.n)
    _lib.check(x.codec.lib.fcz_frames_dev(x.codec.ctx, x.pos.data_ptr(), x.mask.data_ptr(), _ptr(x.aatype), _ptr(bound), n, x.rows, x.lay, fgroups,
                                          out["rot"].data_ptr(), out["trans"].data_ptr(), out["frame_mask"].data_ptr()), "fcz_frames_dev")


def rigid_frames(batch=None, *, groups="backbone", codec: Optional[Codec] = None, **tensors) -> dict:
    """dense tensors on the GPU -> dict(rot, trans, frame_mask): every residue as rigid transforms, global = rot @ local + trans.

    `batch` is the dict decode_tensors / tensor_batches return, padded or packed, or the tensors come as keywords: pos
    [n, L, A, 3] float32, mask [n, L, A] bool or uint8, aatype [n, L] uint8 (needed for "all"), optionally length [n]; or the packed
    pos [R, A, 3], mask [R, A], aatype [R] (recognised by the shape of pos: frames use atoms of their own row only, so cu_seqlens is
    not read). groups="backbone": rot [n, L, 3, 3], trans [n, L, 3], frame_mask [n, L] bool -- AlphaFold's Algorithm 21 on (N, CA,
    C): origin CA, x axis CA -> C, N in the xy half-plane y > 0. groups="all": rot [n, L, 8, 3, 3], trans [n, L, 8, 3], frame_mask
    [n, L, 8], indexed like rigidgroups_gt_frames (FRAME_GROUPS: backbone, two unused groups, psi, chi1 .. chi4);
    frame_ambiguous()[aatype] tells which of them have a 180-degree alternative, rot @ diag(1, -1, -1). The packed form has [R]
    in place of [n, L]. A group exists where the row lies inside its chain, the type and the layout have its three atoms, their
    masks are set, their coordinates finite and they are neither coincident nor collinear; elsewhere rot is the identity, trans 0,
    frame_mask False. The arithmetic is float32 in a fixed order (include/fcz_hip.h), so the result is reproducible bit for bit.

    Padded: `length` is used when the dict has no crop_start (as neighbor_graph does). The tensors must be contiguous and lie on
    the codec's device; ordering against torch is decode_tensors'. groups is checked first, without a device."""
    def check(d):
        fgroups = api.check_frames(groups, d.get("aatype") is not None)
        _need("rigid_frames", d)
        shape = tuple(getattr(d["pos"], "shape", ()))
        if len(shape) not in (3, 4) or shape[-1] != 3 or shape[-2] not in _WIDTH_LAYOUT:
            raise ValueError(f"pos must be float32 [n, L, A, 3] or [R, A, 3] with A = 37, 14 or 4, not {shape}")
        if fgroups == 0:
            d["aatype"] = None                                                # (the backbone frame reads no residue type: aatype is not looked at)
        return shape, len(shape) == 3, fgroups                                # (the packed form: recognised by the shape of pos alone)

    x, (_, _, fgroups) = _inputs("rigid_frames", "Codec.frames", batch, tensors, codec, check, one_entry=True)
    out = _frames_alloc(x.torch, x.dev, x.lead, fgroups)
    if x.n == 0 or x.rows == 0:
        return out
    x.torch.cuda.current_stream(x.dev).synchronize()
    _frames_into(x, fgroups, out)
    x.codec.synchronize()
    return out


def encode_tensors(batch=None, *, names=None, layout=None, anchor_residue_threshold: int = 25, codec: Optional[Codec] = None,
                   skip_bad: bool = False, **tensors) -> list:
    """dense tensors on the GPU -> [fcz bytes, ...], one record per chain.

    `batch` is the dict decode_tensors / FoldcompDatabase.tensor_batches return, as it is (its `names` become the records' titles,
    res_index[:, 0] the first residue number), or the tensors come as keywords: pos [n, L, A, 3] float32, mask [n, L, A] bool or
    uint8, aatype [n, L] uint8, length [n] int32 / int64, and optionally plddt [n, L] float32 (default 0) and res_index [n, L] or
    first_res_index [n] (default 1). `names` given here wins over the dict's. layout: inferred from A (37 / 14 / 4) when None.

    The packed form (decode_tensors(packed=True)) is recognised by a 3-D pos [R, A, 3] together with cu_seqlens [n + 1] int32 /
    int64: mask [R, A], aatype [R], plddt [R], and res_index [R] (its value at every chain's first row is the first residue
    number) or first_res_index [n]. Chain c is rows cu_seqlens[c] .. cu_seqlens[c + 1] - 1; `length` is not read. A chain whose
    range runs backwards, leaves the R rows or holds more than 65 535 of them is refused like the others below.

    Of row l of chain c only l < length[c] counts, and of its atoms only those whose mask is set in a slot the residue type owns;
    everything else may hold anything. A chain the codec refuses (aatype > 20, a residue without N, CA and C, length above L,
    fewer than two residues, a NaN or an infinity in a present atom) raises foldcomp.error, or gives None under skip_bad=True.

    The tensors must be contiguous and lie on the codec's device. Ordering against torch is decode_tensors': torch's current stream
    is synchronised before the codec's calls, the codec's stream before the function returns. Only the records, their offsets and
    the per-chain status come to the host.
    """
    if not isinstance(anchor_residue_threshold, int):
        raise TypeError("anchor_residue_threshold must be an integer")
    d = dict(batch) if batch is not None else {}
    d.update(tensors)
    is_packed = d.get("cu_seqlens") is not None and getattr(d.get("pos"), "ndim", 4) == 3
    for k in ("pos", "mask", "aatype", "cu_seqlens" if is_packed else "length"):
        if d.get(k) is None:
            raise TypeError(f"encode_tensors needs the tensor {k!r}")
    c = codec or api.default_codec()
    try:
        import torch
    except ImportError as e:
        raise api.error(f"encode_tensors needs PyTorch (ROCm build): {e}") from None
    pos = d["pos"]
    if not isinstance(pos, torch.Tensor):
        raise api.error("encode_tensors takes torch tensors on the GPU (numpy arrays: Codec.compress_dense)")
    if pos.device.type != "cuda" or pos.device.index != int(c.device):
        raise api.error(f"encode_tensors: pos lies on {pos.device}, the codec works on cuda:{int(c.device)}; "
                        "the records are built where the tensors are and there is no CPU path")
    dev = pos.device
    if is_packed:
        if pos.shape[2] != 3 or pos.dtype != torch.float32:
            raise ValueError(f"pos must be float32 [R, A, 3] beside cu_seqlens, not {pos.dtype} {tuple(pos.shape)}")
        cu = d["cu_seqlens"]
        if not isinstance(cu, torch.Tensor) or cu.dim() != 1 or cu.shape[0] < 1:
            raise ValueError("cu_seqlens must be a tensor [n + 1]")
        n, L, A = int(cu.shape[0]) - 1, int(pos.shape[0]), int(pos.shape[1])          # (L: the rows of the packed arrays, R)
    elif pos.dim() != 4 or pos.shape[3] != 3 or pos.dtype != torch.float32:
        raise ValueError(f"pos must be float32 [n, L, A, 3], not {pos.dtype} {tuple(pos.shape)}")
    else:
        n, L, A = int(pos.shape[0]), int(pos.shape[1]), int(pos.shape[2])
    if layout is None:
        if A not in _WIDTH_LAYOUT:
            raise ValueError(f"no dense layout has {A} slots per residue (37, 14 or 4)")
        layout = _WIDTH_LAYOUT[A]
    lay = dense_layout(layout)
    if c.lib.fcz_dense_width(lay) != A:
        raise ValueError(f"layout {layout!r} has {c.lib.fcz_dense_width(lay)} slots per residue, pos has {A}")
    names = d.get("names") if names is None else names
    if names is not None and len(names) != n:
        raise ValueError(f"{len(names)} names for {n} chains")

    rows, what = (L,) if is_packed else (n, L), "encode_tensors"
    _on_device(torch, what, dev, "pos", pos, rows + (A, 3), (torch.float32,))
    mask = _on_device(torch, what, dev, "mask", d["mask"], rows + (A,), (torch.bool, torch.uint8))
    aatype = _on_device(torch, what, dev, "aatype", d["aatype"], rows, (torch.uint8,))
    length = _on_device(torch, what, dev, "cu_seqlens" if is_packed else "length", d["cu_seqlens" if is_packed else "length"],
                        (n + 1,) if is_packed else (n,), (torch.int32, torch.int64))
    plddt = _on_device(torch, what, dev, "plddt", d["plddt"], rows, (torch.float32,)) if d.get("plddt") is not None else None
    first = None
    if d.get("first_res_index") is not None:
        first = _on_device(torch, what, dev, "first_res_index", d["first_res_index"], (n,), (torch.int32, torch.int64)).to(torch.int32)
    elif d.get("res_index") is not None and L:
        ri = _on_device(torch, what, dev, "res_index", d["res_index"], rows, (torch.int32,))
        # (packed: a chain without rows may start at R; its record is refused or empty, any row serves)
        first = ri[length[:-1].to(torch.int64).clamp(0, L - 1)].contiguous() if is_packed else ri[:, 0].contiguous()
    if n == 0:
        return []
    if L == 0:
        raise ValueError("encode_tensors: the tensors have no rows (L = 0)")
    if bool((length < 0).any()):
        raise ValueError(("cu_seqlens" if is_packed else "length") + " must not be negative")
    if is_packed and length.dtype == torch.int64 and bool((length > 2 ** 32 - 1).any()):
        raise ValueError("cu_seqlens must fit 32 bits")
    # (int32 >= 0 and uint32 share their bits; an int64 offset above 2^31 keeps its low word, which is its value)
    keep = [mask.view(torch.uint8), length.to(torch.int32)]
    s = CDenseIn(pos.data_ptr(), keep[0].data_ptr(), aatype.data_ptr(), None if is_packed else keep[1].data_ptr())
    if plddt is not None:
        s.plddt = plddt.data_ptr()
    if first is not None:
        keep.append(first)
        s.first_res_index = first.data_ptr()
    if names is not None:
        tb = [str(t).encode("latin-1", "replace") for t in names]
        toff = np.zeros(n + 1, np.uint32)
        toff[1:] = np.cumsum([len(t) for t in tb])
        keep += [torch.from_numpy(np.frombuffer(b"".join(tb) + b"\0", np.uint8).copy()).to(dev),
                 torch.from_numpy(toff.view(np.int32)).to(dev)]
        s.titles, s.title_off = keep[-2].data_ptr(), keep[-1].data_ptr()
    torch.cuda.current_stream(dev).synchronize()
    counts = np.zeros(3, np.uint32)
    nbytes = ctypes.c_uint64(0)
    if is_packed:
        _lib.check(c.lib.fcz_compress_dense_packed_begin_dev(c.ctx, ctypes.byref(s), keep[1].data_ptr(), n, L, lay, int(anchor_residue_threshold),
                                                             counts.ctypes.data, ctypes.byref(nbytes)), "fcz_compress_dense_packed_begin_dev")
    else:
        _lib.check(c.lib.fcz_compress_dense_begin_dev(c.ctx, ctypes.byref(s), n, L, lay, int(anchor_residue_threshold), counts.ctypes.data,
                                                      ctypes.byref(nbytes)), "fcz_compress_dense_begin_dev")
    blob_t = torch.empty(max(int(nbytes.value), 1), dtype=torch.uint8, device=dev)
    off_t = torch.empty(n + 1, dtype=torch.int64, device=dev)
    st_t = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.current_stream(dev).synchronize()
    _lib.check(c.lib.fcz_compress_dense_fetch_dev(c.ctx, off_t.data_ptr(), st_t.data_ptr(), blob_t.data_ptr()), "fcz_compress_dense_fetch_dev")
    c.synchronize()
    off = off_t.cpu().numpy()
    st = st_t.cpu().numpy()
    blob = blob_t.cpu().numpy()
    out = []
    for i in range(n):
        if st[i] != 0:
            if not skip_bad:
                raise api.error(f"Error compressing chain {i}: " + c.lib.fcz_status_string(int(st[i])).decode())
            out.append(None)
        else:
            out.append(blob[int(off[i]):int(off[i + 1])].tobytes())
    return out
