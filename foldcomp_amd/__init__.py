"""foldcomp_amd -- MI355X-native Foldcomp codec hot path (host side).

`import foldcomp_amd as foldcomp` gives the reference module's surface
(compress / decompress / get_data / open / error); see api.py.
"""
from .api import (FoldcompDatabase, FoldcompError, compress, compress_many, decompress, decompress_many, error, get_data,
                  open, split_pdb_by_chain)
from .api import FRAME_GROUPS, GDT_CUTOFFS, MAX_ASA, SS3_OF_SS8, SS_CLASSES, frame_ambiguous, lddt_swaps, sphere_points
from .codec import ANGLE_COLUMNS
from .tensors import (apply_transform, backbone_hbonds, decode_angles, decode_tensors, encode_tensors, fape, fape_atoms, gdt, lddt, lddt_atoms, neighbor_graph, rigid_frames,
                      secondary_structure, smooth_lddt, solvent_accessibility, superpose, tm_align, tm_score, violation_loss, violations)

__all__ = ["compress", "decompress", "get_data", "open", "error", "FoldcompError", "FoldcompDatabase", "compress_many",
           "decompress_many", "split_pdb_by_chain", "decode_tensors", "encode_tensors", "decode_angles", "neighbor_graph", "lddt",
           "lddt_atoms", "lddt_swaps", "smooth_lddt", "fape", "fape_atoms",
           "superpose", "tm_score", "gdt", "GDT_CUTOFFS", "tm_align", "apply_transform", "backbone_hbonds", "secondary_structure", "SS_CLASSES", "SS3_OF_SS8",
           "solvent_accessibility", "sphere_points", "MAX_ASA", "violations", "violation_loss",
           "rigid_frames", "frame_ambiguous", "FRAME_GROUPS", "ANGLE_COLUMNS"]
