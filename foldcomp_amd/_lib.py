"""ctypes binding of libfcz_hip.so (the C-ABI of include/fcz_hip.h).

The library is built in-tree (foldcomp_amd/libfcz_hip.so) by `__graft_entry__.build()` or
`make -C foldcomp_amd/csrc`. There is no Python/NumPy/CPU implementation of the codec in this package:
if the shared library is missing, or no HIP device is present, the codec entry points raise.
"""
from __future__ import annotations

import ctypes
import os

from .structure import (CAtomsOut, CChainBatch, CDenseIn, CDenseOut, CEntryInfo, CIngestResult, CLddtAtomsOut, CPackedOut, CSuperposeOut, CTmScoreOut, CGdtOut, CChainSet, CTmAlignParams, CTmAlignOut,
                        CViolationsOut)

_HERE = os.path.dirname(os.path.abspath(__file__))
# FCZ_HIP_LIB selects another build of the same library (A/B timing of kernel variants); it is still a HIP build
LIB_PATH = os.environ.get("FCZ_HIP_LIB") or os.path.join(_HERE, "libfcz_hip.so")

FCZ_OK = 0
STATUS = {0: "FCZ_OK", -1: "FCZ_E_INVALID_ARG", -2: "FCZ_E_NO_DEVICE", -3: "FCZ_E_HIP", -4: "FCZ_E_BAD_MAGIC",
          -5: "FCZ_E_TRUNCATED", -6: "FCZ_E_RESIDUE", -7: "FCZ_E_TOO_SHORT", -8: "FCZ_E_NOMEM", -9: "FCZ_E_NONFINITE"}

_lib = None


class FczLibraryError(RuntimeError):
    pass


def load():
    """Load libfcz_hip.so (once). Raises FczLibraryError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FczLibraryError(
            f"{LIB_PATH} is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()' "
            "or make -C foldcomp_amd/csrc). foldcomp_amd has no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    vp, u32, i32, u64, f32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint64, ctypes.c_float
    PB, PO = ctypes.POINTER(CChainBatch), ctypes.POINTER(CAtomsOut)
    sig = {
        "fcz_ctx_create": (i32, [i32, ctypes.POINTER(vp)]),
        "fcz_ctx_destroy": (None, [vp]),
        "fcz_ctx_stream": (vp, [vp]),
        "fcz_ctx_synchronize": (i32, [vp]),
        "fcz_device_count": (i32, []),
        "fcz_pinned_alloc": (vp, [ctypes.c_size_t]),
        "fcz_pinned_free": (None, [vp]),
        "fcz_ctx_set_numerics": (i32, [vp, i32]),
        "fcz_ctx_get_numerics": (i32, [vp]),
        "fcz_status_string": (ctypes.c_char_p, [i32]),
        "fcz_atom_code_name": (ctypes.c_char_p, [i32]),
        "fcz_atom_code_from_name": (i32, [ctypes.c_char_p]),
        "fcz_res_code_from_name": (i32, [ctypes.c_char_p]),
        "fcz_res_code_name": (ctypes.c_char_p, [i32]),
        "fcz_res_code_natoms": (i32, [i32]),
        "fcz_res_code_atom": (i32, [i32, i32, i32]),
        "fcz_compress_sizes": (i32, [PB, vp]),
        "fcz_compress_batch": (i32, [vp, PB, vp, vp, vp]),
        "fcz_compress_angles": (i32, [vp, PB, vp]),
        "fcz_compress_sizes_dev": (i32, [vp, PB, vp]),
        "fcz_compress_batch_dev": (i32, [vp, PB, vp, vp, vp]),
        "fcz_decompress_sizes": (i32, [vp, vp, u32, vp, vp, vp]),
        "fcz_decompress_batch": (i32, [vp, vp, vp, u32, vp, vp, i32, PO]),
        "fcz_decompress_sizes_dev": (i32, [vp, vp, vp, u32, vp, vp, ctypes.POINTER(u32), ctypes.POINTER(u32)]),
        "fcz_decompress_batch_dev": (i32, [vp, vp, vp, u32, vp, vp, i32, PO]),
        "fcz_pdb_sizes_dev": (i32, [vp, vp, vp, u32, vp, vp, PO, vp]),
        "fcz_pdb_format_dev": (i32, [vp, vp, vp, u32, vp, vp, PO, i32, vp, vp]),
        "fcz_decompress_pdb_begin": (i32, [vp, vp, vp, u32, i32, vp, vp]),
        "fcz_decompress_pdb_fetch": (i32, [vp, vp]),
        "fcz_decompress_pdb_sizes": (i32, [vp, vp, vp, u32, i32, vp, vp]),
        "fcz_dense_width": (i32, [i32]),
        "fcz_dense_slot": (i32, [i32, i32, i32]),
        "fcz_dense_dev": (i32, [vp, vp, vp, u32, vp, vp, PO, i32, i32, u32, ctypes.POINTER(CDenseOut)]),
        "fcz_decompress_dense": (i32, [vp, vp, vp, u32, i32, u32, ctypes.POINTER(u32), ctypes.POINTER(CDenseOut), vp]),
        "fcz_dense_window_dev": (i32, [vp, vp, vp, u32, vp, vp, PO, i32, i32, u32, vp, ctypes.POINTER(CDenseOut)]),
        "fcz_decompress_dense_window": (i32, [vp, vp, vp, u32, i32, u32, vp, ctypes.POINTER(u32), ctypes.POINTER(CDenseOut), vp]),
        "fcz_angles_window_dev": (i32, [vp, vp, vp, u32, vp, u32, vp, vp, vp, vp]),
        "fcz_decompress_angles_window": (i32, [vp, vp, vp, u32, u32, vp, ctypes.POINTER(u32), vp, vp, vp, vp]),
        "fcz_dense_packed_dev": (i32, [vp, vp, vp, u32, vp, vp, PO, i32, i32, ctypes.POINTER(CPackedOut)]),
        "fcz_decompress_dense_packed": (i32, [vp, vp, vp, u32, i32, ctypes.POINTER(u32), vp, ctypes.POINTER(CPackedOut), vp]),
        "fcz_knn_pass": (i32, []),
        "fcz_knn_dev": (i32, [vp, vp, vp, vp, u32, u32, i32, i32, u32, vp, vp]),
        "fcz_knn_packed_dev": (i32, [vp, vp, vp, vp, u32, u32, i32, i32, u32, vp, vp]),
        "fcz_knn": (i32, [vp, vp, vp, vp, u32, u32, i32, i32, u32, vp, vp]),
        "fcz_knn_packed": (i32, [vp, vp, vp, vp, u32, u32, i32, i32, u32, vp, vp]),
        "fcz_lddt_pass": (i32, []),
        "fcz_lddt_c2": (f32, [f32]),
        "fcz_lddt_dev": (i32, [vp, vp, vp, vp, vp, vp, u32, u32, i32, i32, f32, vp, vp, vp, vp]),
        "fcz_lddt_packed_dev": (i32, [vp, vp, vp, vp, vp, vp, u32, u32, i32, i32, f32, vp, vp, vp, vp]),
        "fcz_lddt": (i32, [vp, vp, vp, vp, vp, vp, u32, u32, i32, i32, f32, vp, vp, vp, vp]),
        "fcz_lddt_packed": (i32, [vp, vp, vp, vp, vp, vp, u32, u32, i32, i32, f32, vp, vp, vp, vp]),
        "fcz_lddt_soft_dev": (i32, [vp, vp, vp, vp, vp, vp, u32, u32, i32, i32, f32, vp, vp, vp]),
        "fcz_lddt_soft_packed_dev": (i32, [vp, vp, vp, vp, vp, vp, u32, u32, i32, i32, f32, vp, vp, vp]),
        "fcz_lddt_soft_grad_dev": (i32, [vp, vp, vp, vp, vp, vp, u32, u32, i32, i32, f32, vp, vp, vp]),
        "fcz_lddt_soft_grad_packed_dev": (i32, [vp, vp, vp, vp, vp, vp, u32, u32, i32, i32, f32, vp, vp, vp]),
        "fcz_lddt_soft": (i32, [vp, vp, vp, vp, vp, vp, u32, u32, i32, i32, f32, vp, vp, vp]),
        "fcz_lddt_soft_packed": (i32, [vp, vp, vp, vp, vp, vp, u32, u32, i32, i32, f32, vp, vp, vp]),
        "fcz_lddt_soft_grad": (i32, [vp, vp, vp, vp, vp, vp, u32, u32, i32, i32, f32, vp, vp, vp]),
        "fcz_lddt_soft_grad_packed": (i32, [vp, vp, vp, vp, vp, vp, u32, u32, i32, i32, f32, vp, vp, vp]),
        "fcz_fape_pass": (i32, []),
        **{name: (i32, [vp] * 12 + [u32, u32, i32, i32, f32, f32, vp, vp])
           for name in ("fcz_fape_dev", "fcz_fape_packed_dev", "fcz_fape", "fcz_fape_packed")},
        **{name: (i32, [vp] * 12 + [u32, u32, i32, i32, f32, f32, vp, vp, vp, vp])
           for name in ("fcz_fape_grad_dev", "fcz_fape_grad_packed_dev", "fcz_fape_grad", "fcz_fape_grad_packed")},
        "fcz_fape_atoms_pass": (i32, []),
        "fcz_fape_atoms_tile_rows": (i32, [i32]),
        **{name: (i32, [vp] * 14 + [u32, u32, i32, f32, f32, vp, vp, vp])
           for name in ("fcz_fape_atoms_dev", "fcz_fape_atoms_packed_dev", "fcz_fape_atoms", "fcz_fape_atoms_packed")},
        **{name: (i32, [vp] * 14 + [u32, u32, i32, f32, f32, vp, vp, vp, vp, vp])
           for name in ("fcz_fape_atoms_grad_dev", "fcz_fape_atoms_grad_packed_dev", "fcz_fape_atoms_grad", "fcz_fape_atoms_grad_packed")},
        "fcz_lddt_atoms_pass": (i32, []),
        "fcz_lddt_atoms_max_rows": (i32, [i32]),
        "fcz_lddt_default_swaps": (i32, [i32, vp]),
        "fcz_lddt_atoms_dev": (i32, [vp, vp, vp, vp, vp, vp, vp, u32, u32, i32, f32, vp, vp, ctypes.POINTER(CLddtAtomsOut)]),
        "fcz_lddt_atoms_packed_dev": (i32, [vp, vp, vp, vp, vp, vp, vp, u32, u32, i32, f32, vp, vp, ctypes.POINTER(CLddtAtomsOut)]),
        "fcz_lddt_atoms": (i32, [vp, vp, vp, vp, vp, vp, vp, u32, u32, i32, f32, vp, vp, ctypes.POINTER(CLddtAtomsOut)]),
        "fcz_lddt_atoms_packed": (i32, [vp, vp, vp, vp, vp, vp, vp, u32, u32, i32, f32, vp, vp, ctypes.POINTER(CLddtAtomsOut)]),
        "fcz_hbond_pass": (i32, []),
        "fcz_hbond_dev": (i32, [vp, vp, vp, vp, vp, u32, u32, i32, vp, vp, vp, vp]),
        "fcz_hbond_packed_dev": (i32, [vp, vp, vp, vp, vp, u32, u32, i32, vp, vp, vp, vp]),
        "fcz_dssp_labels_dev": (i32, [vp, vp, vp, vp, vp, u32, u32, i32, vp, vp, vp, vp]),
        "fcz_dssp_labels_packed_dev": (i32, [vp, vp, vp, vp, vp, u32, u32, i32, vp, vp, vp, vp]),
        "fcz_dssp": (i32, [vp, vp, vp, vp, vp, u32, u32, i32, vp, vp, vp, vp, vp, vp]),
        "fcz_dssp_packed": (i32, [vp, vp, vp, vp, vp, u32, u32, i32, vp, vp, vp, vp, vp, vp]),
        "fcz_sasa_pass": (i32, []),
        "fcz_sasa_default_radii": (i32, [i32, vp]),
        "fcz_sasa_dev": (i32, [vp, vp, vp, vp, vp, u32, u32, i32, vp, f32, vp, u32, vp, vp, vp]),
        "fcz_sasa_packed_dev": (i32, [vp, vp, vp, vp, vp, u32, u32, i32, vp, f32, vp, u32, vp, vp, vp]),
        "fcz_sasa": (i32, [vp, vp, vp, vp, vp, u32, u32, i32, vp, f32, vp, u32, vp, vp, vp]),
        "fcz_sasa_packed": (i32, [vp, vp, vp, vp, vp, u32, u32, i32, vp, f32, vp, u32, vp, vp, vp]),
        "fcz_violations_pass": (i32, []),
        "fcz_violations_dev": (i32, [vp, vp, vp, vp, vp, u32, u32, i32, vp, f32, f32, ctypes.POINTER(CViolationsOut)]),
        "fcz_violations_packed_dev": (i32, [vp, vp, vp, vp, vp, u32, u32, i32, vp, f32, f32, ctypes.POINTER(CViolationsOut)]),
        "fcz_violations": (i32, [vp, vp, vp, vp, vp, u32, u32, i32, vp, f32, f32, ctypes.POINTER(CViolationsOut)]),
        "fcz_violations_packed": (i32, [vp, vp, vp, vp, vp, u32, u32, i32, vp, f32, f32, ctypes.POINTER(CViolationsOut)]),
        "fcz_violation_loss_pass": (i32, []),
        "fcz_violation_loss_dev": (i32, [vp, vp, vp, vp, vp, u32, u32, i32, vp, f32, f32, vp, vp, vp]),
        "fcz_violation_loss_packed_dev": (i32, [vp, vp, vp, vp, vp, u32, u32, i32, vp, f32, f32, vp, vp, vp]),
        "fcz_violation_loss_grad_dev": (i32, [vp, vp, vp, vp, vp, u32, u32, i32, vp, f32, f32, vp, vp, vp]),
        "fcz_violation_loss_grad_packed_dev": (i32, [vp, vp, vp, vp, vp, u32, u32, i32, vp, f32, f32, vp, vp, vp]),
        "fcz_violation_loss": (i32, [vp, vp, vp, vp, vp, u32, u32, i32, vp, f32, f32, vp, vp, vp]),
        "fcz_violation_loss_packed": (i32, [vp, vp, vp, vp, vp, u32, u32, i32, vp, f32, f32, vp, vp, vp]),
        "fcz_violation_loss_grad": (i32, [vp, vp, vp, vp, vp, u32, u32, i32, vp, f32, f32, vp, vp, vp]),
        "fcz_violation_loss_grad_packed": (i32, [vp, vp, vp, vp, vp, u32, u32, i32, vp, f32, f32, vp, vp, vp]),
        "fcz_superpose_dev": (i32, [vp, vp, vp, vp, vp, vp, u32, u32, i32, i32, ctypes.POINTER(CSuperposeOut)]),
        "fcz_superpose_packed_dev": (i32, [vp, vp, vp, vp, vp, vp, u32, u32, i32, i32, ctypes.POINTER(CSuperposeOut)]),
        "fcz_superpose": (i32, [vp, vp, vp, vp, vp, vp, u32, u32, i32, i32, ctypes.POINTER(CSuperposeOut)]),
        "fcz_superpose_packed": (i32, [vp, vp, vp, vp, vp, vp, u32, u32, i32, i32, ctypes.POINTER(CSuperposeOut)]),
        "fcz_superpose_apply_dev": (i32, [vp, vp, vp, vp, u32, u32, i32, vp, vp, vp]),
        "fcz_superpose_apply_packed_dev": (i32, [vp, vp, vp, vp, u32, u32, i32, vp, vp, vp]),
        "fcz_superpose_apply": (i32, [vp, vp, vp, vp, u32, u32, i32, vp, vp, vp]),
        "fcz_superpose_apply_packed": (i32, [vp, vp, vp, vp, u32, u32, i32, vp, vp, vp]),
        "fcz_tmscore_seeds": (u64, [u32, u32]),
        "fcz_tmscore_seed_fragment": (i32, [u32, u32, u64, ctypes.POINTER(u32), ctypes.POINTER(u32)]),
        "fcz_tmscore_dev": (i32, [vp, vp, vp, vp, vp, vp, u32, u32, i32, i32, u32, u32, ctypes.POINTER(CTmScoreOut)]),
        "fcz_tmscore_packed_dev": (i32, [vp, vp, vp, vp, vp, vp, u32, u32, i32, i32, u32, u32, ctypes.POINTER(CTmScoreOut)]),
        "fcz_tmscore": (i32, [vp, vp, vp, vp, vp, vp, u32, u32, i32, i32, u32, u32, ctypes.POINTER(CTmScoreOut)]),
        "fcz_tmscore_packed": (i32, [vp, vp, vp, vp, vp, vp, u32, u32, i32, i32, u32, u32, ctypes.POINTER(CTmScoreOut)]),
        "fcz_gdt_dev": (i32, [vp, vp, vp, vp, vp, vp, u32, u32, i32, i32, u32, u32, u32, ctypes.POINTER(CGdtOut)]),
        "fcz_gdt_packed_dev": (i32, [vp, vp, vp, vp, vp, vp, u32, u32, i32, i32, u32, u32, u32, ctypes.POINTER(CGdtOut)]),
        "fcz_gdt": (i32, [vp, vp, vp, vp, vp, vp, u32, u32, i32, i32, u32, u32, u32, ctypes.POINTER(CGdtOut)]),
        "fcz_gdt_packed": (i32, [vp, vp, vp, vp, vp, vp, u32, u32, i32, i32, u32, u32, u32, ctypes.POINTER(CGdtOut)]),
        "fcz_tmalign_seeds": (u64, [u32, u32, u32]),
        "fcz_tmalign_seed": (i32, [u32, u32, u32, u64, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(u32)]),
        "fcz_tmalign_last_work": (i32, [vp, ctypes.POINTER(u64), ctypes.POINTER(u64)]),
        "fcz_tmalign_dev": (i32, [vp, ctypes.POINTER(CChainSet), ctypes.POINTER(CChainSet), vp, u32, u32, u32, i32, i32, ctypes.POINTER(CTmAlignParams),
                            ctypes.POINTER(CTmAlignOut)]),
        "fcz_tmalign": (i32, [vp, ctypes.POINTER(CChainSet), ctypes.POINTER(CChainSet), vp, u32, u32, u32, i32, i32, ctypes.POINTER(CTmAlignParams),
                        ctypes.POINTER(CTmAlignOut)]),
        "fcz_tmalign_dp_dev": (i32, [vp, ctypes.POINTER(CChainSet), ctypes.POINTER(CChainSet), vp, u32, u32, u32, i32, i32, vp, vp, ctypes.c_double, vp, vp]),
        "fcz_tmalign_dp": (i32, [vp, ctypes.POINTER(CChainSet), ctypes.POINTER(CChainSet), vp, u32, u32, u32, i32, i32, vp, vp, ctypes.c_double, vp, vp]),
        "fcz_frames_width": (i32, [i32]),
        "fcz_frame_atom": (i32, [i32, i32, i32]),
        "fcz_frame_ambiguous": (i32, [i32, i32]),
        "fcz_frames_dev": (i32, [vp, vp, vp, vp, vp, u32, u32, i32, i32, vp, vp, vp]),
        "fcz_frames": (i32, [vp, vp, vp, vp, vp, u32, u32, i32, i32, vp, vp, vp]),
        "fcz_chi_atom": (i32, [i32, i32]),
        "fcz_angles_dev": (i32, [vp, vp, vp, u32, vp, u32, vp, vp]),
        "fcz_angles_packed_dev": (i32, [vp, vp, vp, u32, vp, vp, vp]),
        "fcz_decompress_angles": (i32, [vp, vp, vp, u32, u32, ctypes.POINTER(u32), vp, vp, vp]),
        "fcz_decompress_angles_packed": (i32, [vp, vp, vp, u32, ctypes.POINTER(u32), vp, vp, vp, vp]),
        "fcz_undense_packed_dev": (i32, [vp, ctypes.POINTER(CDenseIn), vp, u32, u32, i32, i32, PB, vp, vp]),
        "fcz_compress_dense_packed_begin_dev": (i32, [vp, ctypes.POINTER(CDenseIn), vp, u32, u32, i32, i32, vp, ctypes.POINTER(u64)]),
        "fcz_compress_dense_packed_begin": (i32, [vp, ctypes.POINTER(CDenseIn), vp, u32, u32, i32, i32, vp, ctypes.POINTER(u64)]),
        "fcz_undense_dev": (i32, [vp, ctypes.POINTER(CDenseIn), u32, u32, i32, i32, PB, vp, vp]),
        "fcz_undense_fetch": (i32, [vp, PB, vp]),
        "fcz_compress_dense_begin_dev": (i32, [vp, ctypes.POINTER(CDenseIn), u32, u32, i32, i32, vp, ctypes.POINTER(u64)]),
        "fcz_compress_dense_fetch_dev": (i32, [vp, vp, vp, vp]),
        "fcz_compress_dense_begin": (i32, [vp, ctypes.POINTER(CDenseIn), u32, u32, i32, i32, vp, ctypes.POINTER(u64)]),
        "fcz_compress_dense_fetch": (i32, [vp, vp, vp, vp]),
        "fcz_extract_sizes": (i32, [vp, vp, u32, i32, i32, vp]),
        "fcz_extract": (i32, [vp, vp, vp, u32, i32, i32, vp, vp]),
        "fcz_extract_sizes_dev": (i32, [vp, vp, vp, u32, i32, i32, vp]),
        "fcz_extract_dev": (i32, [vp, vp, vp, u32, i32, i32, vp, vp]),
        "fcz_ingest_pdb_dev": (i32, [vp, vp, vp, u32, u64, vp, vp, vp, i32, i32, vp]),
        "fcz_ingest_pdb_begin": (i32, [vp, vp, vp, u32, vp, vp, vp, i32, i32, vp]),
        "fcz_ingest_pdb_fetch": (i32, [vp, PB, vp, vp, vp, vp]),
        "fcz_ingest_chain_names_fetch": (i32, [vp, vp]),
        "fcz_compress_pdb_begin": (i32, [vp, vp, vp, u32, vp, vp, vp, i32, i32, vp, ctypes.POINTER(u64)]),
        "fcz_compress_pdb_fetch": (i32, [vp, vp, vp, vp, vp, vp, vp, vp]),
        "fcz_inflate_sizes": (i32, [vp, vp, u32, vp, vp]),
        "fcz_inflate_dev": (i32, [vp, vp, vp, u32, vp, vp, vp, vp]),
        "fcz_inflate": (i32, [vp, vp, vp, u32, vp, vp, vp, vp]),
        "fcz_ingest_gz_begin": (i32, [vp, vp, vp, u32, vp, vp, vp, vp, i32, i32, vp]),
        "fcz_compress_gz_begin": (i32, [vp, vp, vp, u32, vp, vp, vp, vp, i32, i32, vp, ctypes.POINTER(u64)]),
        "fcz_check": (i32, [vp, u64]),
        "fcz_ctx_enable_timing": (i32, [vp, i32]),
        "fcz_ctx_kernel_time": (i32, [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(u64)]),
        "fcz_ctx_reset_timing": (None, [vp]),
        "fcz_selftest_math": (i32, [vp, i32, u32, u32, u32, vp]),
        "fcz_selftest_copy": (i32, [vp, u64, i32, ctypes.POINTER(ctypes.c_double)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


EXPORTS = ["fcz_ctx_create", "fcz_ctx_destroy", "fcz_ctx_stream", "fcz_ctx_synchronize", "fcz_status_string",
           "fcz_atom_code_name", "fcz_atom_code_from_name", "fcz_res_code_from_name", "fcz_res_code_name",
           "fcz_res_code_natoms", "fcz_res_code_atom", "fcz_compress_sizes", "fcz_compress_batch",
           "fcz_compress_angles", "fcz_compress_sizes_dev", "fcz_compress_batch_dev", "fcz_decompress_sizes", "fcz_decompress_batch",
           "fcz_decompress_sizes_dev", "fcz_decompress_batch_dev", "fcz_pdb_sizes_dev", "fcz_pdb_format_dev",
           "fcz_decompress_pdb_begin", "fcz_decompress_pdb_fetch", "fcz_decompress_pdb_sizes",
           "fcz_dense_width", "fcz_dense_slot", "fcz_dense_dev", "fcz_decompress_dense", "fcz_undense_dev", "fcz_undense_fetch",
           "fcz_compress_dense_begin_dev", "fcz_compress_dense_fetch_dev", "fcz_compress_dense_begin", "fcz_compress_dense_fetch",
           "fcz_dense_packed_dev", "fcz_decompress_dense_packed", "fcz_undense_packed_dev", "fcz_compress_dense_packed_begin_dev",
           "fcz_compress_dense_packed_begin",
           "fcz_chi_atom", "fcz_angles_dev", "fcz_angles_packed_dev", "fcz_decompress_angles", "fcz_decompress_angles_packed",
           "fcz_dense_window_dev", "fcz_decompress_dense_window", "fcz_angles_window_dev", "fcz_decompress_angles_window",
           "fcz_knn_pass", "fcz_knn_dev", "fcz_knn_packed_dev", "fcz_knn", "fcz_knn_packed",
           "fcz_lddt_pass", "fcz_lddt_c2", "fcz_lddt_dev", "fcz_lddt_packed_dev", "fcz_lddt", "fcz_lddt_packed",
           "fcz_lddt_soft_dev", "fcz_lddt_soft_packed_dev", "fcz_lddt_soft_grad_dev", "fcz_lddt_soft_grad_packed_dev", "fcz_lddt_soft", "fcz_lddt_soft_packed",
           "fcz_lddt_soft_grad", "fcz_lddt_soft_grad_packed",
           "fcz_fape_pass", "fcz_fape_dev", "fcz_fape_packed_dev", "fcz_fape_grad_dev", "fcz_fape_grad_packed_dev", "fcz_fape", "fcz_fape_packed", "fcz_fape_grad",
           "fcz_fape_grad_packed",
           "fcz_fape_atoms_pass", "fcz_fape_atoms_tile_rows", "fcz_fape_atoms_dev", "fcz_fape_atoms_packed_dev", "fcz_fape_atoms_grad_dev",
           "fcz_fape_atoms_grad_packed_dev", "fcz_fape_atoms", "fcz_fape_atoms_packed", "fcz_fape_atoms_grad", "fcz_fape_atoms_grad_packed",
           "fcz_lddt_atoms_pass", "fcz_lddt_atoms_max_rows", "fcz_lddt_default_swaps", "fcz_lddt_atoms_dev", "fcz_lddt_atoms_packed_dev", "fcz_lddt_atoms",
           "fcz_lddt_atoms_packed",
           "fcz_hbond_pass", "fcz_hbond_dev", "fcz_hbond_packed_dev", "fcz_dssp_labels_dev", "fcz_dssp_labels_packed_dev", "fcz_dssp", "fcz_dssp_packed",
           "fcz_sasa_pass", "fcz_sasa_default_radii", "fcz_sasa_dev", "fcz_sasa_packed_dev", "fcz_sasa", "fcz_sasa_packed",
           "fcz_violations_pass", "fcz_violations_dev", "fcz_violations_packed_dev", "fcz_violations", "fcz_violations_packed",
           "fcz_violation_loss_pass", "fcz_violation_loss_dev", "fcz_violation_loss_packed_dev", "fcz_violation_loss_grad_dev",
           "fcz_violation_loss_grad_packed_dev", "fcz_violation_loss", "fcz_violation_loss_packed", "fcz_violation_loss_grad", "fcz_violation_loss_grad_packed",
           "fcz_superpose_dev", "fcz_superpose_packed_dev", "fcz_superpose", "fcz_superpose_packed",
           "fcz_superpose_apply_dev", "fcz_superpose_apply_packed_dev", "fcz_superpose_apply", "fcz_superpose_apply_packed",
           "fcz_tmscore_seeds", "fcz_tmscore_seed_fragment", "fcz_tmscore_dev", "fcz_tmscore_packed_dev", "fcz_tmscore", "fcz_tmscore_packed",
           "fcz_gdt_dev", "fcz_gdt_packed_dev", "fcz_gdt", "fcz_gdt_packed",
           "fcz_tmalign_seeds", "fcz_tmalign_seed", "fcz_tmalign_last_work", "fcz_tmalign_dev", "fcz_tmalign", "fcz_tmalign_dp_dev", "fcz_tmalign_dp",
           "fcz_frames_width", "fcz_frame_atom", "fcz_frame_ambiguous", "fcz_frames_dev", "fcz_frames",
           "fcz_extract_sizes", "fcz_extract",
           "fcz_extract_sizes_dev", "fcz_extract_dev", "fcz_ingest_pdb_dev", "fcz_ingest_pdb_begin", "fcz_ingest_pdb_fetch", "fcz_ingest_chain_names_fetch",
           "fcz_compress_pdb_begin", "fcz_compress_pdb_fetch", "fcz_inflate_sizes", "fcz_inflate_dev", "fcz_inflate",
           "fcz_ingest_gz_begin", "fcz_compress_gz_begin", "fcz_check", "fcz_ctx_enable_timing",
           "fcz_ctx_kernel_time", "fcz_ctx_reset_timing", "fcz_selftest_math", "fcz_selftest_copy"]


def status_name(code: int) -> str:
    return STATUS.get(int(code), f"status {code}")


def check(code: int, what: str):
    if code != FCZ_OK:
        msg = load().fcz_status_string(int(code)).decode()
        raise FczLibraryError(f"{what}: {status_name(code)} ({msg})")
