"""Python surface of the reference's `foldcomp` module on top of the MI355X codec.

Same names, argument meaning and error behaviour as foldcomp/foldcomp.cxx:
    compress(name, pdb_content, *, anchor_residue_threshold=25) -> bytes          (:295-328)
    decompress(fcz_bytes) -> (name, pdb_text)                                      (:222-239)
    get_data(bytes_or_str) -> dict(phi, psi, omega, torsion_angles, bond_angles,
                                   residues, b_factors, coordinates)               (:673-695)
    open(path, *, ids=None, decompress=True, err_on_missing=False) -> FoldcompDatabase (:333-435)
plus batch forms (`compress_many`, `decompress_many`) because one chain per call cannot fill a GPU.
All geometry runs on the GPU through libfcz_hip.so; only text parsing/formatting happens here.
"""
from __future__ import annotations

import os
import sys
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import fczfile
from ._aa_tables import RES1, RES3
from . import _lib
from .codec import Codec, dense_layout
from .database import DatabaseReader
from .structure import (Chain, MultipleChainsError, StructureError, build_batch, parse_pdb, remove_alternative_position)

DEFAULT_ANCHOR_THRESHOLD = 25


class error(Exception):
    """foldcomp.error of the reference module"""


FoldcompError = error
_codec: Optional[Codec] = None


def default_codec() -> Codec:
    global _codec
    if _codec is None or _codec.ctx is None:
        _codec = Codec(int(os.environ.get("FOLDCOMP_AMD_DEVICE", "0")))
    return _codec


def set_codec(c: Optional[Codec]):
    global _codec
    _codec = c


# ---- compress ------------------------------------------------------------------------------------
def _chain_from_pdb(name: str, pdb_content: str) -> Chain:
    try:
        t = parse_pdb(pdb_content, single_chain=True)
    except MultipleChainsError:
        raise error("Multiple chains found. Please provide a single chain using 'foldcomp.split_pdb_by_chain'")
    except StructureError as e:
        # (std::stoi / std::stof / substr throw inside the reference's extension and end the interpreter: an exception here)
        raise error(f"Error parsing the PDB string: {e}")
    if len(t) == 0:
        raise error("No ATOM lines found")
    return Chain(name, remove_alternative_position(t))


def compress_many(items: Sequence[Tuple[str, str]], *, anchor_residue_threshold: int = DEFAULT_ANCHOR_THRESHOLD,
                  codec: Optional[Codec] = None) -> List[bytes]:
    """[(name, pdb_content), ...] -> [fcz bytes, ...] in one GPU batch"""
    if not isinstance(anchor_residue_threshold, int):
        raise TypeError("anchor_residue_threshold must be an integer")
    chains = [_chain_from_pdb(n, p) for n, p in items]
    try:
        batch = build_batch(chains, anchor_residue_threshold)
    except StructureError as e:
        raise error(f"Error compressing: {e}")
    c = codec or default_codec()
    blob, off, st = c.compress_batch(batch, strict=False)
    if (st != 0).any():
        # (a refused chain: residue names the reference cannot process, fewer than two residues, a NaN / infinite coordinate or
        # B-factor -- FCZ_E_NONFINITE, include/fcz_hip.h)
        bad = int(st[st != 0][0])
        raise error("Error compressing: " + _lib.load().fcz_status_string(bad).decode())
    return [blob[off[i]:off[i + 1]].tobytes() for i in range(len(chains))]


def compress(name: str, pdb_content: str, *, anchor_residue_threshold: int = DEFAULT_ANCHOR_THRESHOLD) -> bytes:
    if not isinstance(name, str) or not isinstance(pdb_content, str):
        raise TypeError("compress(name: str, pdb_content: str)")
    return compress_many([(name, pdb_content)], anchor_residue_threshold=anchor_residue_threshold)[0]


# ---- decompress ----------------------------------------------------------------------------------
def decompress_many(entries: Sequence[bytes], *, alt_order: bool = False, codec: Optional[Codec] = None,
                    skip_bad: bool = False) -> List[Optional[Tuple[str, str]]]:
    """[fcz, ...] -> [(name, pdb_text), ...] in one GPU batch"""
    c = codec or default_codec()
    off = np.zeros(len(entries) + 1, np.uint64)
    off[1:] = np.cumsum([len(e) for e in entries])
    blob = np.frombuffer(b"".join(entries), np.uint8) if entries else np.zeros(0, np.uint8)
    texts, status = c.decompress_pdb(blob, off, alt_order=alt_order)   # reconstruction and PDB text both on the device
    out = []
    for i, e in enumerate(entries):
        if status[i] != 0:
            if skip_bad:
                out.append(None); continue
            raise error("Error decompressing.")
        rec = fczfile.parse(e)
        out.append((rec.title, texts[i].decode("latin-1")))
    return out


def decompress(fcz: bytes) -> Tuple[str, str]:
    if not isinstance(fcz, (bytes, bytearray, memoryview)):
        raise TypeError(f"a bytes-like object is required, not '{type(fcz).__name__}'")      # ("y#", foldcomp.cxx:204)
    return decompress_many([bytes(fcz)])[0]


# ---- get_data ------------------------------------------------------------------------------------
def get_data(input) -> dict:  # noqa: A002
    if isinstance(input, str):
        raw = input.encode("latin-1")
    elif isinstance(input, (bytes, bytearray, memoryview)):
        raw = bytes(input)
    else:
        raise TypeError(f"a bytes-like object is required, not '{type(input).__name__}'")
    if len(raw) == 0:
        raise ValueError("Input is empty")
    if len(raw) >= 4 and raw[:4] == b"FCMP":
        try:
            rec = fczfile.parse(raw)
        except fczfile.FczFormatError:
            raise ValueError("Could not read FCZ file")
        c = default_codec()
        off = np.asarray([0, len(raw)], np.uint64)
        d = c.decompress_batch(np.frombuffer(raw, np.uint8), off)
        if d["info"][0].status != 0:
            raise ValueError("Could not decompress FCZ file")
        a = fczfile.angle_lists(rec)
        coords = list(zip(d["x"].tolist(), d["y"].tolist(), d["z"].tolist()))
        return dict(phi=a["phi"].tolist(), psi=a["psi"].tolist(), omega=a["omega"].tolist(),
                    torsion_angles=a["torsion_angles"].tolist(), bond_angles=a["bond_angles"].tolist(),
                    residues=fczfile.sequence(rec), b_factors=fczfile.temp_factors(rec).tolist(), coordinates=coords)
    if len(raw) >= 4:
        # PDB text: note the reference skips removeAlternativePosition here (foldcomp.cxx:633-662)
        t = parse_pdb(raw.decode("latin-1"))
        if len(t) == 0:
            raise ValueError("No ATOM lines found in PDB file")
        batch = build_batch([Chain("", t)], DEFAULT_ANCHOR_THRESHOLD)
        ang = default_codec().compress_angles(batch)
        n = batch.n_residues
        phi, psi, omg, nca, can, cna = (ang[q][:n - 1] for q in range(6))
        tors = np.stack([psi, omg, phi], 1).reshape(-1)
        # getBondAngles order: angle at atom 1 (first N-CA-C), then (ca_c_n, c_n_ca, n_ca_c) per window
        bonds = np.concatenate([[ang[3][n - 1]], np.stack([can, cna, nca], 1).reshape(-1)]).astype(np.float32)
        return dict(phi=phi.tolist(), psi=psi.tolist(), omega=omg.tolist(), torsion_angles=tors.tolist(),
                    bond_angles=bonds.tolist(), residues="".join(RES1[c] for c in batch.res_code),
                    b_factors=batch.bfac_ca.tolist(), coordinates=list(map(tuple, t.xyz.tolist())))
    raise ValueError("Input is not a FCZ file or PDB file")


# ---- open ----------------------------------------------------------------------------------------
class FoldcompDatabase:
    """Sequence over a Foldcomp database (foldcomp.cxx:44-185): len(), db[i], iteration, context manager."""

    def __init__(self, path, ids=None, decompress=True, err_on_missing=False):
        try:
            self._reader = DatabaseReader(os.fspath(path), use_lookup=bool(ids))
        except ValueError as e:                  # an index line the reader cannot take (database.py): the module's own error, not a stray ValueError
            raise error(str(e)) from None
        self._decompress = decompress
        self._ids = None
        if ids:
            self._ids = []
            for name in ids:
                i = self._reader.id_of_name(name)
                if i < 0:
                    msg = f"Skipping entry {name} which is not in the database."
                    if err_on_missing:
                        self._reader.close()
                        raise KeyError(msg)
                    print(msg, file=sys.stderr)
                    continue
                self._ids.append(i)

    def __len__(self):
        return len(self._ids) if self._ids is not None else len(self._reader)

    def _entry(self, index: int) -> bytes:
        if index < 0 or index >= len(self):
            raise IndexError("index out of range")
        i = self._ids[index] if self._ids is not None else index
        # The reference drops the last byte of every entry (foldcomp.cxx:66,73), which is right for MMseqs2-made databases
        # (entries end in a NUL) and one byte short for the ones `foldcomp compress --db` writes (no terminator,
        # src/main.cpp:516). Here only a real terminator is dropped: the byte after the record's header-derived length, or
        # the NUL that closes a non-FCZ (text) entry.
        data = self._reader.data(i)
        size = fczfile.record_size(data)
        if size >= 0:
            return data[:size] if len(data) > size else data
        return data[:-1] if data.endswith(b"\0") else data

    # The reference's module is per entry by construction (foldcomp.cxx:44-90: one Foldcomp::read + decompress + PDB text per
    # __getitem__, :197-220). A GPU call per entry would spend its time in launches and copies, so sequential access -- the loop a
    # program written against the reference runs, `for name, pdb in db:` or db[0], db[1], ... -- is served from a read-ahead
    # WINDOW: READAHEAD entries (FOLDCOMP_READAHEAD, default 1024: ~240 MB of text at 350 residues) decoded and formatted by ONE
    # fcz_decompress_pdb call. Same values, same exception at the entry that does not decode; random access decodes the one entry.
    READAHEAD = max(1, int(os.environ.get("FOLDCOMP_READAHEAD", "1024")))

    def _window(self, start: int):
        ents = [self._entry(i) for i in range(start, min(start + self.READAHEAD, len(self)))]
        self._win_start, self._win = start, decompress_many(ents, skip_bad=True)

    def __getitem__(self, index):
        index = int(index)
        if index < 0:
            index += len(self)                        # the sequence protocol of the reference's type (sq_item behind PySequence_GetItem): db[-1] is the last entry
        if not self._decompress:
            return self._entry(index)
        if index < 0 or index >= len(self):
            raise IndexError("index out of range")
        win = getattr(self, "_win", None)
        if win is not None and self._win_start <= index < self._win_start + len(win):
            r = win[index - self._win_start]
        elif index == getattr(self, "_next", 0):
            self._window(index)                       # the access after the last one (or the first): the caller is walking the database
            r = self._win[0]
        else:
            r = decompress_many([self._entry(index)], skip_bad=True)[0]
        self._next = index + 1
        if r is None:
            raise error("Error decompressing: ")
        return r

    def __iter__(self):
        for i in range(len(self)):
            yield self[i]

    def decompress_all(self, batch: int = 4096):
        """GPU-sized iteration: yields (name, pdb) for every entry, decoding `batch` entries per launch"""
        for s in range(0, len(self), batch):
            ents = [self._entry(i) for i in range(s, min(s + batch, len(self)))]
            for r in decompress_many(ents):
                yield r

    def tensor_batches(self, batch_size: int = 1024, *, layout="atom37", max_len: Optional[int] = None, device="cuda:0",
                       sort_by_length: bool = False, packed: bool = False, max_residues: Optional[int] = None,
                       angles: bool = False, crop: Optional[str] = None, seed: Optional[int] = None,
                       neighbors: Optional[int] = None, neighbor_atom="CA", frames: Optional[str] = None,
                       secondary_structure: bool = False, sasa: bool = False, violations: bool = False):
        """Generator over the database (its `ids` selection when it has one) in batches of dense model-input tensors on the GPU:
        the dicts of foldcomp_amd.tensors.decode_tensors, each with `names` (the records' titles) and `index` (int64 array: the
        entries' positions in this database, what db[i] takes). sort_by_length orders every window of 16 * batch_size entries by
        residue count (from the record headers) before it is cut into batches, so that a batch pads little; `index` undoes it.
        packed=True yields the packed dicts (decode_tensors(packed=True): no padding, no crop, cu_seqlens), and max_residues then
        cuts the batches by a residue budget (cut_batches): a batch closes before the entry that would take it over the budget
        or at batch_size entries; an entry longer than the budget forms a batch of its own. angles=True adds `angles` and
        `angle_mask` to every dict (decode_tensors(angles=True)). crop="start" / "center" / "random" with max_len=L keeps a window
        of L residues of every longer entry (decode_tensors(crop=...)) and adds `crop_start` to every dict; "random" draws from ONE
        generator for the whole iteration, seeded once with `seed` (None: from the system), so the same seed gives the same crops.
        neighbors=k adds the k-nearest-neighbour graph of every chain, `nbr_index` / `nbr_dist`, on the sites of `neighbor_atom`
        (decode_tensors(neighbors=k)); like the other argument rules, a bad k or atom raises at the first next(), before a record
        is read. frames="backbone" | "all" adds the rigid frames `rot` / `trans` / `frame_mask` (decode_tensors(frames=...)), checked
        at the first next() too. secondary_structure=True adds the DSSP labels `ss` / `ss_mask` of every chain
        (decode_tensors(secondary_structure=True)). sasa=True adds the solvent accessibility `sasa` / `rsa` / `sasa_mask` of every
        residue (decode_tensors(sasa=True)). violations=True adds `clash_count` / `link_violation` / `viol_mask`, the steric clashes
        and peptide-link violations of every residue (decode_tensors(violations=True))."""
        from .tensors import decode_tensors
        check_secondary_structure_flag(secondary_structure)
        check_sasa_flag(sasa)
        check_violations_flag(violations)
        if frames is not None:
            check_frames(frames)
        if neighbors is not None:
            check_neighbors(neighbors, neighbor_atom, {0: 37, 1: 14, 2: 4}[dense_layout(layout)])
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError("batch_size must be at least 1")
        check_batch_cut(packed, max_len, max_residues)
        if crop is not None and not isinstance(crop, str):
            raise ValueError("tensor_batches takes crop='start', 'center' or 'random' (per-entry starts belong to one batch: decode_tensors)")
        check_crop(crop, max_len, packed)
        gen = None
        window = 16 * batch_size if sort_by_length else batch_size
        if max_residues is not None:
            window = 16 * batch_size                    # (a budget closes batches early: read ahead as the sort does)
        for start in range(0, len(self), window):
            idx = np.arange(start, min(start + window, len(self)), dtype=np.int64)
            ents = [self._entry(int(i)) for i in idx]
            lens = [fczfile.residue_count(e) for e in ents] if sort_by_length or max_residues is not None else [0] * len(ents)
            for sel in cut_batches(lens, batch_size, max_residues, sort_by_length):
                sel = np.asarray(sel, np.int64)
                if packed:
                    d = decode_tensors([ents[k] for k in sel], layout=layout, device=device, packed=True, angles=angles,
                                       neighbors=neighbors, neighbor_atom=neighbor_atom, frames=frames, secondary_structure=secondary_structure,
                                       sasa=sasa, violations=violations)
                else:
                    if crop == "random" and gen is None:
                        import torch
                        gen = torch.Generator(device=device)
                        gen.manual_seed(int(seed)) if seed is not None else gen.seed()
                    d = decode_tensors([ents[k] for k in sel], layout=layout, max_len=max_len, device=device, angles=angles, crop=crop,
                                       generator=gen, neighbors=neighbors, neighbor_atom=neighbor_atom, frames=frames,
                                       secondary_structure=secondary_structure, sasa=sasa, violations=violations)
                d["index"] = idx[sel]
                yield d

    def close(self):
        self._win = None
        if self._reader is not None:
            self._reader.close()
            self._reader = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def check_batch_cut(packed, max_len, max_residues):
    """the argument rules of tensor_batches that need no database and no GPU"""
    if max_residues is not None and not packed:
        raise ValueError("max_residues cuts packed batches: pass packed=True (a padded batch is sized by batch_size and max_len)")
    if max_residues is not None and int(max_residues) < 1:
        raise ValueError("max_residues must be at least 1")
    if packed and max_len is not None:
        raise ValueError("max_len crops to a common length; the packed form keeps every residue (packed=True takes no max_len)")


CROP_MODES = ("start", "center", "random")


def check_crop(crop, max_len, packed):
    """the argument rules of crop= (decode_tensors, decode_angles, tensor_batches) that need no records and no GPU"""
    if crop is None:
        return
    if isinstance(crop, str) and crop not in CROP_MODES:
        raise ValueError(f"crop must be one of {CROP_MODES} or per-entry starts [n], not {crop!r}")
    if packed:
        raise ValueError("crop keeps a window of max_len rows per entry; the packed form keeps every residue (packed=True takes no crop)")
    if max_len is None:
        raise ValueError("crop needs max_len: the window is max_len residues long")


# slot of the named atom per layout width (atom37: N CA C CB ..; atom14: N CA C O CB ..; backbone4: N CA C O -- no CB)
NEIGHBOR_ATOMS = {"CA": {37: 1, 14: 1, 4: 1}, "CB": {37: 3, 14: 4}}
MAX_NEIGHBORS = 64


def check_neighbors(k, atom, width=None):
    """the argument rules of neighbors= / neighbor_graph that need no tensors' device and no GPU -> the slot (None while the
    layout width A is unknown): k an integer 1 .. 64; atom "CA", "CB" (atom37 / atom14 only) or an integer slot 0 .. A - 1"""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= MAX_NEIGHBORS:
        raise ValueError(f"k must be an integer 1 .. {MAX_NEIGHBORS}, not {k!r}")
    if isinstance(atom, str):
        if atom not in NEIGHBOR_ATOMS:
            raise ValueError(f"atom must be one of {', '.join(NEIGHBOR_ATOMS)} or an integer slot, not {atom!r}")
        if width is None:
            return None
        if width not in NEIGHBOR_ATOMS[atom]:
            raise ValueError(f"a layout of {width} slots per residue has no {atom}")
        return NEIGHBOR_ATOMS[atom][width]
    if isinstance(atom, bool) or not isinstance(atom, (int, np.integer)) or not 0 <= int(atom) < (37 if width is None else width):
        raise ValueError(f"atom must be 'CA', 'CB' or a slot 0 .. {(37 if width is None else width) - 1}, not {atom!r}")
    if width is not None and width not in (37, 14, 4):
        raise ValueError(f"no dense layout has {width} slots per residue (37, 14 or 4)")
    return int(atom)


LDDT_THRESHOLDS = (0.5, 1.0, 2.0, 4.0)


def check_lddt(cutoff, thresholds, atom, width=None):
    """the argument rules of lddt that need no tensors' device and no GPU -> (slot, cutoff, thresholds): cutoff a finite number > 0,
    thresholds four numbers, none NaN (None: 0.5, 1, 2, 4), all three as float32 values; atom as check_neighbors reads it (the slot
    is None while the layout width A is unknown)"""
    slot = check_neighbors(1, atom, width)

    def number(v):
        return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating))

    with np.errstate(over="ignore"):
        if not number(cutoff) or not np.isfinite(np.float32(cutoff)) or not np.float32(cutoff) > 0:
            raise ValueError(f"cutoff must be a finite number > 0 (as float32), not {cutoff!r}")
    if thresholds is None:
        thresholds = LDDT_THRESHOLDS
    try:
        th = tuple(thresholds)
    except TypeError:
        raise ValueError(f"thresholds must be four numbers, not {thresholds!r}") from None
    if len(th) != 4 or not all(number(v) and not np.isnan(v) for v in th):
        raise ValueError(f"thresholds must be four numbers, none of them NaN, not {thresholds!r}")
    with np.errstate(over="ignore"):
        return slot, float(np.float32(cutoff)), tuple(float(np.float32(v)) for v in th)


def check_lddt_soft(cutoff, thresholds, atom, width=None):
    """the argument rules of smooth_lddt that need no tensors' device and no GPU -> (slot, cutoff, thresholds): check_lddt's, and
    every threshold finite as float32 (a sigmoid about an infinite threshold is a constant, which has no place in a loss)"""
    slot, cutoff, th = check_lddt(cutoff, thresholds, atom, width)
    if not all(np.isfinite(v) for v in th):
        raise ValueError(f"thresholds must be four finite numbers (as float32), not {thresholds!r}")
    return slot, cutoff, th


def check_fape(clamp, scale, eps, atom, width=None):
    """the argument rules of fape that need no tensors' device and no GPU -> (slot, clamp, scale, eps): clamp a number > 0 (as
    float32; +inf or None: unclamped, returned as +inf), scale and eps finite numbers > 0 (eps as float32, scale as a Python float);
    atom as check_neighbors reads it (the slot is None while the layout width A is unknown)"""
    slot = check_neighbors(1, atom, width)

    def number(v):
        return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating))

    with np.errstate(over="ignore", under="ignore"):
        if clamp is None:
            clamp = float("inf")
        if not number(clamp) or np.isnan(np.float32(clamp)) or not np.float32(clamp) > 0:
            raise ValueError(f"clamp must be a number > 0 (as float32), +inf or None for unclamped, not {clamp!r}")
        if not number(scale) or not np.isfinite(float(scale)) or not float(scale) > 0:
            raise ValueError(f"scale must be a finite number > 0, not {scale!r}")
        if not number(eps) or not np.isfinite(np.float32(eps)) or not np.float32(eps) > 0:
            raise ValueError(f"eps must be a finite number > 0 (as float32), not {eps!r}")
        return slot, float(np.float32(clamp)), float(scale), float(np.float32(eps))


def _swap_table(swaps, A, what="swaps"):
    """an integer array [21, A] that is an involution within each row with entries < A -> uint8 [21, A] (lddt_atoms' rule)"""
    table = np.asarray(swaps)
    if table.shape != (21, A) or table.dtype.kind not in "iu":
        raise ValueError(f"{what} must be an integer array of the shape (21, {A}), not {table.dtype} {table.shape}")
    if (table < 0).any() or (table >= A).any():
        raise ValueError(f"every entry of {what} must be a slot 0 .. {A - 1}")
    table = np.ascontiguousarray(table, np.uint8)
    if not np.array_equal(np.take_along_axis(table, table.astype(np.int64), axis=1), np.broadcast_to(np.arange(A, dtype=np.uint8), (21, A))):
        raise ValueError(f"{what} must be an involution within each row: the partner of a slot's partner is the slot")
    return table


def check_fape_atoms(clamp, scale, eps, rename, shape, has_aatype=True, swaps="alphafold"):
    """the argument rules of fape_atoms that need no torch and no GPU -> (clamp, scale, eps, rename, table): clamp, scale and eps as
    check_fape reads them; pos [n, L, A, 3] or [R, A, 3] with A = 37, 14 or 4 and a chain bound of at most min(2^29, (2^31 - 1) // A)
    rows, so that a frame's points fit int32. rename: "lddt_atoms" (decide inside the call), None (rename nothing) or an array /
    tensor of the shape of pos without its last two axes, the decision already made (returned as it is); anything but None needs
    aatype. swaps: "alphafold" (table None: the library's default) or lddt_atoms' integer array [21, A] (table: uint8 [21, A])."""
    _, clamp, scale, eps = check_fape(clamp, scale, eps, 1)
    shape = tuple(shape)
    if len(shape) not in (3, 4) or shape[-1] != 3 or shape[-2] not in (37, 14, 4):
        raise ValueError(f"pos must be float32 [n, L, A, 3] or [R, A, 3] with A = 37, 14 or 4, not {shape}")
    A = shape[-2]
    limit = min(2 ** 29, (2 ** 31 - 1) // A)
    if shape[-3] > limit:
        raise ValueError(f"fape_points must fit int32: at most {limit} rows per chain in a layout of {A} slots")
    if isinstance(rename, str):
        if rename != "lddt_atoms":
            raise ValueError(f"rename must be 'lddt_atoms', None or a bool array {shape[:-2]}, not {rename!r}")
    elif rename is not None:
        if tuple(getattr(rename, "shape", ())) != shape[:-2] or isinstance(rename, (bool, int, float)):
            raise ValueError(f"rename must be 'lddt_atoms', None or a bool array {shape[:-2]}, not {type(rename).__name__} {tuple(getattr(rename, 'shape', ()))}")
    if rename is not None and not has_aatype:
        raise ValueError("fape_atoms needs aatype in `true` to rename side chains (rename=None: no renaming)")
    if isinstance(swaps, str):
        if swaps != "alphafold":
            raise ValueError(f"swaps must be 'alphafold' or an integer array [21, {A}], not {swaps!r}")
        return clamp, scale, eps, rename, None
    return clamp, scale, eps, rename, _swap_table(swaps, A)


_LAYOUT_WIDTHS = {"atom37": (0, 37), "atom14": (1, 14), "backbone4": (2, 4)}  # name -> (enum fcz_dense_layout, A)


def lddt_swaps(layout="atom37"):
    """the default swap table of lddt_atoms as uint8 [21, A] (fcz_lddt_default_swaps): table[aatype][slot] is the slot that holds the
    other naming of a chemically equivalent atom (ASP OD1 / OD2, GLU OE1 / OE2, PHE and TYR CD1 / CD2 and CE1 / CE2), the slot
    itself everywhere else; backbone4 has none"""
    if layout not in _LAYOUT_WIDTHS:
        raise ValueError(f"unknown dense layout {layout!r}: one of {', '.join(_LAYOUT_WIDTHS)}")
    lay, A = _LAYOUT_WIDTHS[layout]
    table = np.zeros((21, A), np.uint8)
    _lib.check(_lib.load().fcz_lddt_default_swaps(lay, table.ctypes.data), "fcz_lddt_default_swaps")
    return table


def check_lddt_atoms(cutoff, thresholds, swaps, shape, pred_shape, pred_mask_shape=None, has_aatype=True, per_atom=False):
    """the argument rules of lddt_atoms that need no torch and no GPU -> (cutoff, thresholds, table): cutoff and thresholds as
    check_lddt reads them; pos [n, L, A, 3] or [R, A, 3] with A = 37, 14 or 4, pred's pos of that shape and pred's mask, when there
    is one, of the shape without its last axis; a chain bound of at most fcz_lddt_atoms_max_rows rows. swaps: "alphafold" (table
    None: the library's default), None (no renaming: table False) or an integer array [21, A] that is an involution within each row
    with entries < A (table: uint8 [21, A]); anything but None needs aatype. per_atom is a switch."""
    _, cutoff, th = check_lddt(cutoff, thresholds, 1)
    shape = tuple(shape)
    if len(shape) not in (3, 4) or shape[-1] != 3 or shape[-2] not in (37, 14, 4):
        raise ValueError(f"pos must be float32 [n, L, A, 3] or [R, A, 3] with A = 37, 14 or 4, not {shape}")
    if tuple(pred_shape) != shape:
        raise ValueError(f"pred pos must have the shape of true pos, {shape}, not {tuple(pred_shape)}")
    if pred_mask_shape is not None and tuple(pred_mask_shape) != shape[:-1]:
        raise ValueError(f"pred mask must have the shape of true mask, {shape[:-1]}, not {tuple(pred_mask_shape)}")
    if not isinstance(per_atom, (bool, np.bool_)):
        raise ValueError(f"per_atom must be True or False, not {per_atom!r}")
    A = shape[-2]
    limit = (2 ** 31 - 1) // (4 * A * A)
    if shape[-3] > limit:
        raise ValueError(f"lddt_hits must fit int32: at most {limit} rows per chain in a layout of {A} slots")
    if swaps is None:
        return cutoff, th, False
    if not has_aatype:
        raise ValueError("lddt_atoms needs aatype in `true` to rename side chains (swaps=None: no renaming)")
    if isinstance(swaps, str):
        if swaps != "alphafold":
            raise ValueError(f"swaps must be 'alphafold', None or an integer array [21, {A}], not {swaps!r}")
        return cutoff, th, None
    return cutoff, th, _swap_table(swaps, A)


GDT_THRESHOLDS = (0.5, 1.0, 2.0, 4.0, 8.0)                                  # the five counters of gdt_counts (include/fcz_hip.h, fcz_superpose_dev)


def check_superpose(atom, shape, pred_shape, pred_mask_shape=None):
    """the argument rules of superpose that need no torch and no GPU -> the slot (None while the layout width A is unknown): atom as
    check_lddt reads it, against the width of `shape`, the shape of true's pos; pred's pos must have that shape, and pred's mask, when
    there is one (pred_mask_shape is not None), the shape without its last axis"""
    shape = tuple(shape)
    slot = check_neighbors(1, atom, shape[-2] if len(shape) in (3, 4) else None)
    if tuple(pred_shape) != shape:
        raise ValueError(f"pred pos must have the shape of true pos, {shape}, not {tuple(pred_shape)}")
    if pred_mask_shape is not None and tuple(pred_mask_shape) != shape[:-1]:
        raise ValueError(f"pred mask must have the shape of true mask, {shape[:-1]}, not {tuple(pred_mask_shape)}")
    return slot


TM_MAX_ITERATIONS = 64                                                     # what fcz_tmscore_dev accepts (include/fcz_hip.h)


def check_tm_score(atom, shape, pred_shape, pred_mask_shape=None, iterations=20, levels=None):
    """the argument rules of tm_score that need no torch and no GPU -> (slot, iterations, levels as the C call takes it: 0 = every
    fragment length): check_superpose's rules, iterations an integer 0 .. 64, levels None or an integer >= 1"""
    return (check_superpose(atom, shape, pred_shape, pred_mask_shape),) + check_tm_search(iterations, levels)


def check_tm_search(iterations=20, levels=None):
    """iterations an integer 0 .. 64, levels None or an integer >= 1 -> (iterations, levels as the C call takes it: 0 = every length)"""
    if isinstance(iterations, (bool, np.bool_)) or not isinstance(iterations, (int, np.integer)) or not 0 <= int(iterations) <= TM_MAX_ITERATIONS:
        raise ValueError(f"iterations must be an integer 0 .. {TM_MAX_ITERATIONS}, not {iterations!r}")
    if levels is not None and (isinstance(levels, (bool, np.bool_)) or not isinstance(levels, (int, np.integer)) or not 1 <= int(levels) < 2 ** 32):
        raise ValueError(f"levels must be None (every fragment length) or an integer >= 1, not {levels!r}")
    return int(iterations), 0 if levels is None else int(levels)


GDT_CUTOFFS = GDT_THRESHOLDS                                               # the cutoffs of gdt; run 1 + k of its search has the constant cut GDT_CUTOFFS[k]
GDT_RUNS_ALL, GDT_RUNS_TM = 63, 1                                          # FCZ_GDT_RUNS_ALL, FCZ_GDT_RUNS_TM (include/fcz_hip.h)


def check_gdt_runs(runs="all"):
    """runs of gdt -> the bit mask the C call takes (bit 0: the TM cuts; bit 1 + k: the constant cut GDT_CUTOFFS[k]): "all", "tm", or
    an iterable, not empty, of "tm" and cutoffs out of GDT_CUTOFFS"""
    if isinstance(runs, str):
        if runs not in ("all", "tm"):
            raise ValueError(f"runs must be 'all', 'tm' or an iterable of 'tm' and cutoffs out of {GDT_CUTOFFS}, not {runs!r}")
        return GDT_RUNS_ALL if runs == "all" else GDT_RUNS_TM
    try:
        items = list(runs)
    except TypeError:
        raise ValueError(f"runs must be 'all', 'tm' or an iterable of 'tm' and cutoffs out of {GDT_CUTOFFS}, not {runs!r}") from None
    mask = 0
    for r in items:
        if isinstance(r, str) and r == "tm":
            mask |= 1
        elif isinstance(r, (int, float, np.integer, np.floating)) and not isinstance(r, (bool, np.bool_)) and float(r) in GDT_CUTOFFS:
            mask |= 2 << GDT_CUTOFFS.index(float(r))
        else:
            raise ValueError(f"a run must be 'tm' or a cutoff out of {GDT_CUTOFFS}, not {r!r}")
    if not mask:
        raise ValueError("runs must name at least one run")
    return mask


def check_gdt(atom, shape, pred_shape, pred_mask_shape=None, iterations=20, levels=None, runs="all"):
    """the argument rules of gdt that need no torch and no GPU -> (slot, iterations, levels as the C call takes it, runs as its bit
    mask): check_tm_score's rules, and check_gdt_runs' for runs"""
    return check_tm_score(atom, shape, pred_shape, pred_mask_shape, iterations, levels) + (check_gdt_runs(runs),)


TM_ALIGN_MAX_WIDTH = 1024                                                  # FCZ_TMALIGN_MAX_WIDTH (include/fcz_hip.h)
TM_ALIGN_MAX_ROUNDS = 64
TM_ALIGN_MAX_GAP = 16.0


def check_tm_align(atom, shape_a, shape_b, wa, wb, pairs_shape=None, fragments=True, refine=4, dp_rounds=20, gaps=(0.6, 0.0), iterations=20, levels=None,
                   transform=None):
    """the argument rules of tm_align that need no torch and no GPU -> (slot, fragments 0 / 1, refine, dp_rounds, gaps as a tuple of
    floats, iterations, levels as the C call takes it). shape_a / shape_b: pos of the two chain sets, each [n, L, A, 3] or [R, A, 3], of
    one width A; wa / wb: the widths (L of a padded set, the longest chain of a packed one, None while unknown), at most 1024;
    pairs_shape: the shape of pairs, [m, 2], when pairs are given; fragments a switch; refine and dp_rounds integers 0 .. 64; gaps one
    to four numbers in [0, 16]; iterations and levels as tm_score's; transform, when given, the shapes of (rot, trans): [m, 3, 3] and
    [m, 3] with pairs' m"""
    shape_a, shape_b = tuple(shape_a), tuple(shape_b)
    for name, shape in (("a", shape_a), ("b", shape_b)):
        if len(shape) not in (3, 4) or shape[-1] != 3 or shape[-2] not in (37, 14, 4):
            raise ValueError(f"pos of {name} must be float32 [n, L, A, 3], or [R, A, 3] beside cu_seqlens, with A = 37, 14 or 4, not {shape}")
    if shape_a[-2] != shape_b[-2]:
        raise ValueError(f"a and b must share one layout, not widths {shape_a[-2]} and {shape_b[-2]}")
    slot = check_neighbors(1, atom, shape_a[-2])
    for name, w in (("a", wa), ("b", wb)):
        if w is not None and int(w) > TM_ALIGN_MAX_WIDTH:
            raise ValueError(f"tm_align handles chains of at most {TM_ALIGN_MAX_WIDTH} rows; {name} has one of {int(w)} (crop it, or align windows)")
    if pairs_shape is not None and (len(tuple(pairs_shape)) != 2 or tuple(pairs_shape)[1] != 2):
        raise ValueError(f"pairs must be int32 [m, 2] (chain of a, chain of b), not {tuple(pairs_shape)}")
    if not isinstance(fragments, (bool, np.bool_)):
        raise ValueError(f"fragments must be True or False, not {fragments!r}")
    for name, v in (("refine", refine), ("dp_rounds", dp_rounds)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= TM_ALIGN_MAX_ROUNDS:
            raise ValueError(f"{name} must be an integer 0 .. {TM_ALIGN_MAX_ROUNDS}, not {v!r}")
    number = lambda v: isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))
    try:
        gs = tuple(gaps)
    except TypeError:
        gs = (gaps,)
    if not 1 <= len(gs) <= 4 or not all(number(g) and 0.0 <= float(g) <= TM_ALIGN_MAX_GAP for g in gs):
        raise ValueError(f"gaps must be one to four numbers in [0, {TM_ALIGN_MAX_GAP:g}], not {gaps!r}")
    iterations, levels = check_tm_search(iterations, levels)
    if transform is not None:
        rs, ts = (tuple(x) for x in transform)
        if len(rs) != 3 or rs[1:] != (3, 3) or ts != (rs[0], 3) or (pairs_shape is not None and rs[0] != tuple(pairs_shape)[0]):
            raise ValueError(f"transform must be (rot [m, 3, 3], trans [m, 3]) with one transform per pair, not {rs} and {ts}")
    return slot, int(bool(fragments)), int(refine), int(dp_rounds), tuple(float(g) for g in gs), iterations, levels


def tm_align_pairs(n_a, n_b, same):
    """the pairs tm_align takes when none are given -> int32 [m, 2]: every i < j of one set, or every (i, j) of two, a-major"""
    if same:
        i, j = np.triu_indices(n_a, 1)
    else:
        i, j = (x.ravel() for x in np.meshgrid(np.arange(n_a), np.arange(n_b), indexing="ij"))
    return np.ascontiguousarray(np.stack([i, j], axis=1), np.int32)


# the labels of `ss`, in the order of their codes (include/fcz_hip.h, fcz_dssp_labels_dev), and the usual reduction to three states
# (helix 0: H, G, I; strand 1: E, B; coil 2: the rest) as a table to index with `ss`
SS_CLASSES = ("-", "H", "B", "E", "G", "I", "T", "S")
SS3_OF_SS8 = np.array([2, 0, 1, 1, 0, 0, 2, 2], np.uint8)
HBOND_TABLES = (("hbond_acc_index", "int32"), ("hbond_acc_energy", "float32"), ("hbond_don_index", "int32"), ("hbond_don_energy", "float32"))


def check_secondary_structure_flag(flag):
    """secondary_structure= of decode_tensors / tensor_batches is a switch"""
    if not isinstance(flag, (bool, np.bool_)):
        raise ValueError(f"secondary_structure must be True or False, not {flag!r}")


def check_dssp(what, d, hbonds=None):
    """the argument rules of backbone_hbonds / secondary_structure that need no torch and no GPU, on the dict `d` of tensors or
    arrays (anything with a shape) -> (shape of pos, packed): pos [n, L, A, 3], or [R, A, 3] beside cu_seqlens, with A = 37, 14 or
    4; mask of pos's shape without its last axis; aatype, when given, without its last two; hbonds, when given, a dict of the two
    acceptor tables [.., 2]"""
    for key in ("pos", "mask"):
        if d.get(key) is None:
            raise TypeError(f"{what} needs the tensor {key!r}")
    shape = tuple(getattr(d["pos"], "shape", ()))
    packed = d.get("cu_seqlens") is not None and len(shape) == 3
    if len(shape) != (3 if packed else 4) or shape[-1] != 3 or shape[-2] not in (37, 14, 4):
        raise ValueError(f"pos must be float32 [n, L, A, 3], or [R, A, 3] beside cu_seqlens, with A = 37, 14 or 4, not {shape}")
    if tuple(getattr(d["mask"], "shape", ())) != shape[:-1]:
        raise ValueError(f"mask must have the shape {shape[:-1]}, not {tuple(getattr(d['mask'], 'shape', ()))}")
    if d.get("aatype") is not None and tuple(getattr(d["aatype"], "shape", ())) != shape[:-2]:
        raise ValueError(f"aatype must have the shape {shape[:-2]}, not {tuple(getattr(d['aatype'], 'shape', ()))}")
    if max(shape[:-2], default=0) > 2 ** 31 - 1:
        raise ValueError("the H-bond tables hold rows as int32: at most 2^31 - 1 rows")
    if hbonds is not None:
        if not isinstance(hbonds, dict):
            raise TypeError(f"hbonds must be a dict of the tables backbone_hbonds returns, not {type(hbonds).__name__}")
        for key in ("hbond_acc_index", "hbond_acc_energy"):
            if hbonds.get(key) is None:
                raise TypeError(f"hbonds needs the table {key!r}")
            if tuple(getattr(hbonds[key], "shape", ())) != shape[:-2] + (2,):
                raise ValueError(f"{key} must have the shape {shape[:-2] + (2,)}, not {tuple(getattr(hbonds[key], 'shape', ()))}")
    return shape, packed


# Solvent accessibility (include/fcz_hip.h, fcz_sasa_dev). MAX_ASA: the theoretical maximum accessible surface of a residue in
# Gly-X-Gly (Tien et al. 2013, PLoS ONE 8:e80635) in square Angstrom, in aatype order A R N D C Q E G H I L K M F P S T W Y V; 0 for
# index 20 (no such maximum: rsa is 0 there).
MAX_ASA = np.array([129, 274, 195, 193, 167, 225, 223, 104, 224, 197, 201, 236, 224, 240, 159, 155, 172, 285, 263, 174, 0], np.float32)
SASA_MAX_POINTS = 1024
SASA_PROBE = 1.4
SASA_POINTS = 128


def sphere_points(n):
    """n directions on the unit sphere as float32 [n, 3]: the golden spiral z_k = 1 - (2 k + 1) / n at the angle k * pi * (3 - sqrt(5)),
    computed in float64 and rounded once. The default surface points of solvent_accessibility."""
    n = int(n)
    if not 1 <= n <= SASA_MAX_POINTS:
        raise ValueError(f"n must be 1 .. {SASA_MAX_POINTS}, not {n}")
    k = np.arange(n, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / n
    r = np.sqrt(1.0 - z * z)
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1).astype(np.float32)


def check_sasa_flag(flag):
    """sasa= of decode_tensors / tensor_batches is a switch"""
    if not isinstance(flag, (bool, np.bool_)):
        raise ValueError(f"sasa must be True or False, not {flag!r}")


def check_sasa(what, d, probe=SASA_PROBE, n_points=SASA_POINTS, points=None, radii="bondi"):
    """the argument rules of solvent_accessibility that need no torch and no GPU, on the dict `d` of tensors or arrays -> (shape of
    pos, packed, points float32 [P, 3], radii float32 [21, A] or None for the library's default): check_dssp's rules for pos, mask
    and aatype; atom14 needs aatype (a slot's atom depends on the type there); probe finite and not negative; 1 .. 1024 points"""
    shape, packed = check_dssp(what, d)
    A = shape[-2]
    if A == 14 and d.get("aatype") is None:
        raise ValueError(f"{what}: atom14 needs aatype (which atom a slot holds depends on the residue type)")
    probe = float(probe)
    if not np.isfinite(probe) or probe < 0:
        raise ValueError(f"probe must be finite and not negative, not {probe}")
    if points is None:
        points = sphere_points(n_points)
    else:
        points = np.ascontiguousarray(np.asarray(points.cpu() if hasattr(points, "cpu") else points), np.float32)
        if points.ndim != 2 or points.shape[1] != 3 or not 1 <= points.shape[0] <= SASA_MAX_POINTS:
            raise ValueError(f"points must be float32 [P, 3] with 1 <= P <= {SASA_MAX_POINTS}, not {points.shape}")
    if isinstance(radii, str):
        if radii != "bondi":
            raise ValueError(f"radii must be 'bondi' or an array [21, {A}], not {radii!r}")
        table = None
    else:
        table = np.ascontiguousarray(np.asarray(radii), np.float32)
        if table.shape != (21, A):
            raise ValueError(f"radii must have the shape (21, {A}), not {table.shape}")
        R = (table + np.float32(probe))[table != 0]
        if not ((R >= 0.5) & (R < 8.0)).all():
            raise ValueError("every non-zero radius plus the probe must lie in [0.5, 8)")
    return shape, packed, points, table


# Structural violations (include/fcz_hip.h, fcz_violations_dev): the outputs of a call as (key, dtype, trailing shape; "A" = the layout
# width, "n4" = per chain), in the order of fcz_violations_out
VIOLATION_TOLERANCE = 1.5
VIOLATION_LINK_FACTOR = 12.0
VIOLATION_OUTPUTS = (("clash_atom", "uint8", "A"), ("clash_count", "int32", ()), ("clash_depth", "float32", ()), ("clash_partner", "int32", ()),
                     ("viol_mask", "bool", ()), ("link_mask", "bool", ()), ("link_length", "float32", ()), ("link_cos", "float32", (2,)),
                     ("link_violation", "uint8", ()), ("chain_counts", "int64", "n4"))
VIOLATION_BATCH_KEYS = ("clash_count", "link_violation", "viol_mask")      # what violations=True adds to a decoded batch


def check_violations_flag(flag):
    """violations= of decode_tensors / tensor_batches is a switch"""
    if not isinstance(flag, (bool, np.bool_)):
        raise ValueError(f"violations must be True or False, not {flag!r}")


def check_violations(what, d, tolerance=VIOLATION_TOLERANCE, link_factor=VIOLATION_LINK_FACTOR, radii="bondi"):
    """the argument rules of violations that need no torch and no GPU, on the dict `d` of tensors or arrays -> (shape of pos, packed,
    radii float32 [21, A] or None for the library's default): check_dssp's rules for pos, mask and aatype; atom14 needs aatype (a
    slot's atom depends on the type there); tolerance and link_factor finite and not negative (as float32); every non-zero radius
    in [0.5, 8)"""
    shape, packed = check_dssp(what, d)
    A = shape[-2]
    if A == 14 and d.get("aatype") is None:
        raise ValueError(f"{what}: atom14 needs aatype (which atom a slot holds depends on the residue type)")
    for name, v in (("tolerance", tolerance), ("link_factor", link_factor)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"{name} must be a number, not {v!r}")
        with np.errstate(over="ignore"):
            v32 = np.float32(v)
        if not np.isfinite(v32) or v32 < 0:
            raise ValueError(f"{name} must be finite and not negative (as float32), not {v!r}")
    if isinstance(radii, str):
        if radii != "bondi":
            raise ValueError(f"radii must be 'bondi' or an array [21, {A}], not {radii!r}")
        table = None
    else:
        table = np.ascontiguousarray(np.asarray(radii), np.float32)
        if table.shape != (21, A):
            raise ValueError(f"radii must have the shape (21, {A}), not {table.shape}")
        R = table[table != 0]
        if not ((R >= 0.5) & (R < 8.0)).all():
            raise ValueError("every non-zero radius must lie in [0.5, 8)")
    return shape, packed, table


def check_violation_loss(what, d, tolerance=VIOLATION_TOLERANCE, link_factor=VIOLATION_LINK_FACTOR, radii="bondi"):
    """the argument rules of violation_loss that need no torch and no GPU, on the dict `d` that holds the prediction's pos beside the
    truth's mask, aatype and length or cu_seqlens -> (shape of pos, packed, radii float32 [21, A] or None): check_violations' rules,
    all of them (include/fcz_hip.h, fcz_violation_loss_dev refuses what fcz_violations_dev refuses)"""
    return check_violations(what, d, tolerance, link_factor, radii)


# the rigid groups of groups="all", indexed like AlphaFold / OpenFold rigidgroups_gt_frames (include/fcz_hip.h, fcz_frames_dev)
FRAME_GROUPS = ("backbone", "unused_1", "unused_2", "psi", "chi1", "chi2", "chi3", "chi4")
FRAME_GROUP_SETS = {"backbone": 0, "all": 1}                                 # enum fcz_frame_groups


def check_frames(groups, has_aatype=True):
    """the argument rules of frames= / rigid_frames that need no device -> enum fcz_frame_groups: "backbone" or "all"; "all" reads
    the residue types"""
    if not isinstance(groups, str) or groups not in FRAME_GROUP_SETS:
        raise ValueError(f"groups must be one of {', '.join(repr(g) for g in FRAME_GROUP_SETS)}, not {groups!r}")
    if groups == "all" and not has_aatype:
        raise ValueError("groups='all' needs aatype: the chi groups depend on the residue type")
    return FRAME_GROUP_SETS[groups]


def frame_ambiguous():
    """bool [21, 8]: table[aatype] is rigidgroups_group_is_ambiguous -- the groups whose frame has an alternative, rot @ diag(1, -1, -1),
    under the 180-degree symmetric renamings (chi2 of ASP, PHE, TYR; chi3 of GLU); row 20 (any other type) has none"""
    lib = _lib.load()
    return np.array([[bool(lib.fcz_frame_ambiguous(t, g)) if t < 20 else False for g in range(8)] for t in range(21)], dtype=bool)


def cut_batches(lengths, batch_size: int, max_residues: Optional[int] = None, sort_by_length: bool = False) -> list:
    """Positions 0 .. len(lengths) - 1 of one window cut into batches -> list of lists of positions, every position once.

    The positions are taken in their own order, or by residue count (stable) under sort_by_length. A batch closes at batch_size
    entries, and, with max_residues, before the entry that would take its residues over the budget; an entry longer than the
    budget forms a batch of its own (nothing is cropped or dropped). Pure: what tensor_batches does with the record headers'
    residue counts."""
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError("batch_size must be at least 1")
    if max_residues is not None and int(max_residues) < 1:
        raise ValueError("max_residues must be at least 1")
    lengths = [int(x) for x in lengths]
    order = sorted(range(len(lengths)), key=lengths.__getitem__) if sort_by_length else list(range(len(lengths)))   # (sorted is stable)
    out, cur, total = [], [], 0
    for k in order:
        if cur and (len(cur) == batch_size or (max_residues is not None and total + lengths[k] > int(max_residues))):
            out.append(cur)
            cur, total = [], 0
        cur.append(k)
        total += lengths[k]
    if cur:
        out.append(cur)
    return out


def open(path, *, ids=None, decompress=True, err_on_missing=False) -> FoldcompDatabase:  # noqa: A001
    if ids is not None and not isinstance(ids, list):
        raise TypeError("user_ids must be a list.")
    if not isinstance(decompress, bool):
        raise TypeError("decompress must be a boolean")
    if not isinstance(err_on_missing, bool):
        raise TypeError("err_on_missing must be a boolean")
    return FoldcompDatabase(path, ids=ids, decompress=decompress, err_on_missing=err_on_missing)


def split_pdb_by_chain(pdb_str: str):
    """Split a PDB string into a list of PDB strings, one per run of ATOM lines with the same chain id
    (foldcomp/util.py:1-18)."""
    pdb_list, chain, cur = [], None, ""
    for line in pdb_str.splitlines():
        if line.startswith("ATOM"):
            if chain is None:
                chain = line[21]
            elif line[21] != chain:
                pdb_list.append(cur); cur = ""; chain = line[21]
            cur += line + "\n"
    pdb_list.append(cur)
    return pdb_list
