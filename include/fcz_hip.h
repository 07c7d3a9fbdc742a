/* fcz_hip.h -- C-ABI of the MI355X-native Foldcomp codec hot path (libfcz_hip.so).
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types, integer status codes,
 * no exceptions. The reference (steineggerlab/foldcomp) has no FFI for this path -- it is entered
 * through the C++ class `Foldcomp`. Each entry point below names the reference interface it replaces
 * (file:line under the reference tree); INTEGRATION.md shows the binding a maintainer would add.
 *
 *   reference                                              this ABI
 *   ---------------------------------------------------    ------------------------------------------
 *   Foldcomp::compress(span<AtomCoordinate>)               fcz_compress_batch / fcz_compress_batch_dev
 *     src/foldcomp.cpp:562 (+preprocess :450)
 *   Foldcomp::writeStream(ostream&)  src/foldcomp.cpp:1038   (the FCZ bytes are what compress returns)
 *   Foldcomp::getSize()              src/foldcomp.cpp:1190   fcz_compress_sizes / fcz_compress_sizes_dev
 *   Foldcomp::read(istream&)         src/foldcomp.cpp:904    fcz_decompress_sizes (+ header parse)
 *   Foldcomp::decompress(vector<AtomCoordinate>&)          fcz_decompress_batch / fcz_decompress_batch_dev
 *     src/foldcomp.cpp:779
 *   Foldcomp::checkValidity()        src/foldcomp.cpp:1492   fcz_check
 *   (none: the reference stops at the flat atom vector)    fcz_dense_dev / fcz_decompress_dense, fcz_dense_packed_dev / fcz_decompress_dense_packed,
 *                                                          fcz_dense_window_dev / fcz_decompress_dense_window
 *   (none: no neighbour graph of the decoded chain)        fcz_knn_dev / fcz_knn_packed_dev, fcz_knn / fcz_knn_packed
 *   (none: no score of one structure against another)      fcz_lddt_dev / fcz_lddt_packed_dev, fcz_lddt / fcz_lddt_packed
 *   (none: no loss, nothing with a gradient)               fcz_lddt_soft_dev / fcz_lddt_soft_grad_dev (+ _packed and host forms)
 *   (none: no loss on frames)                              fcz_fape_dev / fcz_fape_grad_dev (+ _packed and host forms)
 *   (none: no loss on side-chain frames)                   fcz_fape_atoms_dev / fcz_fape_atoms_grad_dev (+ _packed and host forms)
 *   (none: no all-atom score, no side-chain renaming)      fcz_lddt_atoms_dev / fcz_lddt_atoms_packed_dev, fcz_lddt_atoms / fcz_lddt_atoms_packed
 *   (none: no secondary structure)                         fcz_hbond_dev, fcz_dssp_labels_dev, fcz_dssp (+ _packed forms)
 *   (none: no solvent accessibility)                       fcz_sasa_dev / fcz_sasa_packed_dev, fcz_sasa / fcz_sasa_packed
 *   (none: no structural violations)                       fcz_violations_dev / fcz_violations_packed_dev, fcz_violations / fcz_violations_packed
 *   (none: no loss on clashes and peptide links)           fcz_violation_loss_dev / fcz_violation_loss_grad_dev (+ _packed and host forms)
 *   (none: `rmsd` compares two files unsuperposed)         fcz_superpose_dev / fcz_superpose_packed_dev, fcz_superpose_apply_dev /
 *                                                          fcz_superpose_apply_packed_dev and their host forms
 *   (none: no TM-score)                                    fcz_tmscore_dev / fcz_tmscore_packed_dev and their host forms
 *   (none: no GDT)                                         fcz_gdt_dev / fcz_gdt_packed_dev and their host forms
 *   (none: no rigid frames of the decoded chain)           fcz_frames_dev / fcz_frames
 *   Foldcomp::decompress, the dequantisation :784-804     fcz_angles_dev / fcz_angles_packed_dev, fcz_decompress_angles[_packed],
 *                                                          fcz_angles_window_dev / fcz_decompress_angles_window
 *     (get_data's FCZ branch, foldcomp/foldcomp.cxx)
 *   (none: Foldcomp::compress starts from the flat list)   fcz_undense_dev / fcz_compress_dense_begin[_dev], fcz_undense_packed_dev /
 *                                                          fcz_compress_dense_packed_begin[_dev]
 *
 * Batch-first: one call handles C independent chains ("one wavefront per chain" on the device).
 * Data layout is structure-of-arrays; all offsets are element indices, not bytes, unless noted.
 *
 * Threading: an fcz_ctx owns one HIP stream + device scratch on one GPU; use one ctx per host thread.
 */
#ifndef FCZ_HIP_H
#define FCZ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------------------------ */
enum fcz_status {
    FCZ_OK = 0,
    FCZ_E_INVALID_ARG = -1,
    FCZ_E_NO_DEVICE = -2,       /* no HIP device / HIP runtime error; the library has NO CPU fallback */
    FCZ_E_HIP = -3,
    FCZ_E_BAD_MAGIC = -4,       /* Foldcomp::read returns -1 (src/foldcomp.cpp:911-915) */
    FCZ_E_TRUNCATED = -5,       /* FCZ entry shorter than its header promises */
    FCZ_E_RESIDUE = -6,         /* residue code the reference cannot process (AAS.at throws, src/sidechain.cpp:177) */
    FCZ_E_TOO_SHORT = -7,       /* chain with < 2 residues: undefined in the reference */
    FCZ_E_NOMEM = -8,
    FCZ_E_NONFINITE = -9        /* compress: a NaN or an infinity in a coordinate of a named atom (atom_code != 255) or in a CA
                                 * B-factor of the chain. The reference's readers can produce them (mmCIF `?` / `.` -> NaN,
                                 * lib/gemmi/numb.hpp:19-40; "nan" in a PDB column, lib/gemmi/pdb.hpp:49-54) and its compressor
                                 * then writes NaN quantiser parameters carrying the input's sign and payload
                                 * (src/discretizer.cpp:22-33): a record that decodes to no structure. Refused here, at every
                                 * level (C-ABI status, `[Error]` line of the hosts, foldcomp.error in Python). */
};

/* ---- vocabulary --------------------------------------------------------------------------- */
/* Residue codes: the reference's 5-bit codes (src/utility.h:133-206):
 *   ALA0 ARG1 ASN2 ASP3 CYS4 GLN5 GLU6 GLY7 HIS8 ILE9 LEU10 LYS11 MET12 PHE13 PRO14 SER15 THR16
 *   TRP17 TYR18 VAL19 ASX20 GLX21 STP22 UNK23.
 * Atom codes: 0=N 1=CA 2=C 3=O 4=CB ... 35=OH, 36=OXT, 255=any other name (see fcz_atom_code_name).
 */
#define FCZ_ATOM_CODE_OXT 36
#define FCZ_ATOM_CODE_OTHER 255

/* Compress input: C chains, R residues in total, M atoms in total. Caller-owned.
 * Replaces the tcb::span<AtomCoordinate> handed to Foldcomp::compress (src/main.cpp:485-488).
 * Preconditions (the reference's input domain): every residue holds exactly one atom
 * named N, one CA and one C, in that order (the reference counts residues on the flat list of every N / CA / C
 * atom, src/atom_coordinate.cpp:135-143, src/foldcomp.cpp:462: with one of each per residue that list is this
 * batch's residues); residues of a chain are gap-free; residue names are the 20 standard ones or UNK; the
 * chain's last atom belongs to its last residue by name as well (its residue name is header.lastResidue,
 * src/foldcomp.cpp:469). The structure ingest and the hosts of this repository refuse what does not comply. */
typedef struct fcz_chain_batch {
    uint32_t n_chains;              /* C */
    uint32_t n_residues;            /* R */
    uint32_t n_atoms;               /* M */
    int32_t  anchor_threshold;      /* `-b`, Foldcomp::anchorThreshold (default 25) */
    const uint32_t* res_off;        /* [C+1] residues of chain c = [res_off[c], res_off[c+1]) */
    const uint32_t* atom_off;       /* [R+1] atoms of residue r = [atom_off[r], atom_off[r+1]) (input order) */
    const float*    x;              /* [M] */
    const float*    y;              /* [M] */
    const float*    z;              /* [M] */
    const uint8_t*  atom_code;      /* [M] */
    const uint8_t*  res_code;       /* [R] */
    const float*    bfac_ca;        /* [R] tempFactor of the residue's CA atom (src/foldcomp.cpp:543-547) */
    const int32_t*  first_res_index;  /* [C] header.idxResidue (src/foldcomp.cpp:464) */
    const int32_t*  first_atom_index; /* [C] header.idxAtom */
    const char*     chain_id;       /* [C] */
    const char*     titles;         /* concatenated titles, no NULs */
    const uint32_t* title_off;      /* [C+1] byte offsets into titles */
} fcz_chain_batch;

/* Decompress output: SoA coordinates of all atoms of all chains in reference output order
 * (canonical atom order of src/amino_acid.h, or the `-a` order), OXT last when present.
 * Replaces the std::vector<AtomCoordinate>& filled by Foldcomp::decompress. Caller-owned. */
typedef struct fcz_atoms_out {
    float*    x;            /* [M] */
    float*    y;            /* [M] */
    float*    z;            /* [M] */
    float*    bfac_res;     /* [R] de-quantised B-factor of each residue (src/foldcomp.cpp:884-892) */
    uint8_t*  res_code;     /* [R] */
    uint8_t*  atom_code;    /* [M] optional (may be NULL) */
} fcz_atoms_out;

/* Parsed per-entry header fields a caller needs to rebuild AtomCoordinate records / PDB text. */
typedef struct fcz_entry_info {
    uint32_t n_residues;
    uint32_t n_atoms_out;       /* atoms the decompressor emits (incl. OXT) */
    uint32_t n_atoms_header;    /* header.nAtom */
    int32_t  first_res_index;
    int32_t  first_atom_index;
    uint32_t n_anchors;
    uint32_t n_sidechain_torsions;
    uint32_t title_off;         /* byte offset of the title inside the entry */
    uint32_t title_len;
    char     chain_id;
    char     first_residue;     /* one-letter */
    char     last_residue;
    uint8_t  has_oxt;
    int32_t  status;            /* FCZ_OK or the reason this entry is skipped */
} fcz_entry_info;

typedef struct fcz_ctx fcz_ctx;

/* ---- lifecycle ---------------------------------------------------------------------------- */
int  fcz_ctx_create(int device, fcz_ctx** out);
void fcz_ctx_destroy(fcz_ctx* ctx);
/* hipStream_t of the ctx as an opaque pointer (all *_dev entry points enqueue on it). */
void* fcz_ctx_stream(fcz_ctx* ctx);
int  fcz_ctx_synchronize(fcz_ctx* ctx);

/* Numerics of the decompress side (the compress side always writes the reference's bytes).
 *   FCZ_NUMERICS_EXACT (default): decompressed float32 coordinates are bit-identical to Foldcomp::decompress built with
 *     g++ -O3 on x86-64 / glibc 2.35 -- the reference's evaluation order, its double promotions and glibc's sinf/cosf are
 *     reproduced operation by operation (fcz_math.h).
 *   FCZ_NUMERICS_FAST: the same algorithm (Foldcomp::decompress src/foldcomp.cpp:779-900: forward NeRF, reverse NeRF from the
 *     next anchor, weighted average, side chains) in plain float arithmetic with FMA and hardware rsq, the backbone as a
 *     parallel composition of per-residue rigid transforms (fcz_backbone_fast.h). Coordinates differ from the exact path by
 *     float rounding only (< 1e-3 A, typically 1e-4 A; the reference's RMSD pins of build.sh:35,37 hold unchanged), which is
 *     what `foldcomp check` / the RMSD tolerance of the reference's own tests ask of a decoder. */
/* Host-side helpers for callers that feed the host-pointer entry points from their own threads (one ctx per thread and GPU):
 * the number of visible devices, and page-locked host memory (hipHostMalloc): copies from / to such buffers are true
 * asynchronous DMA on the ctx stream, so two ctxs on one GPU overlap one batch's transfers with the other's kernels. */
int   fcz_device_count(void);
void* fcz_pinned_alloc(size_t bytes);
void  fcz_pinned_free(void* p);

enum fcz_numerics { FCZ_NUMERICS_EXACT = 0, FCZ_NUMERICS_FAST = 1 };
int  fcz_ctx_set_numerics(fcz_ctx* ctx, int mode);
int  fcz_ctx_get_numerics(fcz_ctx* ctx);
const char* fcz_status_string(int status);
const char* fcz_atom_code_name(int atom_code);     /* "N", "CA", ... "OXT"; NULL if out of range */
int  fcz_atom_code_from_name(const char* name);    /* 255 for unknown names */
int  fcz_res_code_from_name(const char* three_letter); /* -1 for names the reference rejects */
const char* fcz_res_code_name(int res_code);
int  fcz_res_code_natoms(int res_code);            /* atoms emitted per residue (3 for UNK) */
/* canonical atom code of output position j of a residue (alt_order: the `-a` order) */
int  fcz_res_code_atom(int res_code, int j, int alt_order);

/* ---- compress ----------------------------------------------------------------------------- */
/* Exact FCZ size of every chain -> exclusive prefix in out_off[C+1] (bytes). Host arrays.
 * Pure host integer work (Foldcomp::getSize, src/foldcomp.cpp:1190-1214). */
int fcz_compress_sizes(const fcz_chain_batch* in, uint64_t* out_off);

/* Host-pointer convenience: copies the batch to the GPU, runs the kernels, copies FCZ bytes back
 * into out[out_off[c] .. out_off[c+1]). status[c] (may be NULL) receives a per-chain fcz_status.
 * Limit: the records of one batch total less than 2^39 bytes (512 GB; more than any device holds) -- a larger out_off[C] is
 * refused with FCZ_E_INVALID_ARG (the kernels hand side-chain byte addresses on in 39 bits). */
int fcz_compress_batch(fcz_ctx* ctx, const fcz_chain_batch* in, const uint64_t* out_off,
                       uint8_t* out, int32_t* status);

/* Device-resident variant: every pointer inside `in`, plus out_off/out/status, is a device pointer
 * (titles included). Work is enqueued on the ctx stream; no host synchronisation. */
int fcz_compress_sizes_dev(fcz_ctx* ctx, const fcz_chain_batch* in, uint64_t* out_off_dev);
int fcz_compress_batch_dev(fcz_ctx* ctx, const fcz_chain_batch* in, const uint64_t* out_off_dev,
                           uint8_t* out_dev, int32_t* status_dev);

/* Pre-quantisation backbone angles of a host batch -- what `get_data()` of the reference's Python module
 * returns for PDB input (foldcomp/foldcomp.cxx:633-662). angles_out = [6][R] floats, order phi, psi, omega,
 * n_ca_c, ca_c_n, c_n_ca; entry r0+k (k < n-1) belongs to packed word k; n_ca_c[r0+n-1] holds the first
 * residue's N-CA-C angle, which the FCZ format never stores (src/foldcomp.cpp:497). */
int fcz_compress_angles(fcz_ctx* ctx, const fcz_chain_batch* in, float* angles_out);

/* ---- decompress --------------------------------------------------------------------------- */
/* Parse the n entries blob[off[i] .. off[i+1]) (trailing bytes such as the MMseqs '\0' are ignored,
 * like Foldcomp::read). Fills info[n] and the exclusive prefixes res_off[n+1] / atom_off[n+1]
 * that size the output arrays. Entries that fail validation get info[i].status != FCZ_OK and
 * contribute zero residues/atoms. Host arrays. */
int fcz_decompress_sizes(const uint8_t* blob, const uint64_t* off, uint32_t n,
                         fcz_entry_info* info, uint32_t* res_off, uint32_t* atom_off);

int fcz_decompress_batch(fcz_ctx* ctx, const uint8_t* blob, const uint64_t* off, uint32_t n,
                         const uint32_t* res_off, const uint32_t* atom_off, int alt_order,
                         const fcz_atoms_out* out);

/* Device-resident variants. fcz_decompress_sizes_dev fills res_off_dev/atom_off_dev (n+1 each)
 * and returns the totals through pinned host words after a stream sync (the only sync on this path:
 * the caller needs R and M to allocate outputs).
 * The ctx remembers that pass -- the totals, the order of the entries by length, their residue codes -- for ONE
 * following fcz_decompress_batch_dev call that names the same blob_dev, off_dev and n; that call then runs no sizes
 * pass of its own. The memo is keyed on the pointers, not on the bytes behind them: the records must not change
 * between a sizes call and the batch call that follows it on the same pointers (rewrite them and the batch call
 * decodes the new bytes with the old lengths and codes: undefined output). A batch call on other
 * pointers or another n, and every entry point that stages records through the ctx, drop the memo; a batch call without a preceding sizes call, with
 * res_off_dev / atom_off_dev computed elsewhere (fcz_decompress_sizes, another ctx), runs its own pass. */
int fcz_decompress_sizes_dev(fcz_ctx* ctx, const uint8_t* blob_dev, const uint64_t* off_dev, uint32_t n,
                             uint32_t* res_off_dev, uint32_t* atom_off_dev,
                             uint32_t* total_res, uint32_t* total_atoms);
int fcz_decompress_batch_dev(fcz_ctx* ctx, const uint8_t* blob_dev, const uint64_t* off_dev, uint32_t n,
                             const uint32_t* res_off_dev, const uint32_t* atom_off_dev, int alt_order,
                             const fcz_atoms_out* out_dev);

/* ---- PDB text -------------------------------------------------------------------------------- */
/* The text `foldcomp decompress` writes for every entry (writeAtomCoordinatesToPDB, src/atom_coordinate.cpp:220-291,
 * called from src/main.cpp:625-637 and foldcomp/foldcomp.cxx:224-250): TITLE records wrapped at 70 columns, one
 * 81-byte ATOM record per atom (numbers by fast_ftoa<1000,3> / <100,2>, :185-218; printf widens a column that
 * overflows), one TER record. Inputs: the same FCZ entries plus the arrays fcz_decompress_batch_dev filled
 * (x, y, z, bfac_res, res_code required); everything else comes from the entry headers.
 * fcz_pdb_sizes_dev: exclusive prefix of the exact text sizes in text_off_dev[n+1] (bytes; skipped entries: 0). */
int fcz_pdb_sizes_dev(fcz_ctx* ctx, const uint8_t* blob_dev, const uint64_t* off_dev, uint32_t n,
                      const uint32_t* res_off_dev, const uint32_t* atom_off_dev, const fcz_atoms_out* atoms_dev,
                      uint64_t* text_off_dev);
int fcz_pdb_format_dev(fcz_ctx* ctx, const uint8_t* blob_dev, const uint64_t* off_dev, uint32_t n,
                       const uint32_t* res_off_dev, const uint32_t* atom_off_dev, const fcz_atoms_out* atoms_dev,
                       int alt_order, const uint64_t* text_off_dev, uint8_t* text_dev);
/* Host-pointer convenience: FCZ entries -> PDB text with every stage on the device. begin() fills text_off[n+1]
 * (host) and status[n] (may be NULL) and keeps the text in the ctx; fetch() copies text_off[n] bytes out.
 * alt_order here is a set of flags: FCZ_PDB_ALT_ORDER (--use-alt-order), FCZ_PDB_NUL_TERMINATED (every entry that decodes
 * is followed by one NUL, counted in text_off: the record `foldcomp decompress` appends to a database, src/main.cpp:656-664,
 * so that a job's records are one contiguous byte range of the data file). */
#define FCZ_PDB_ALT_ORDER      1
#define FCZ_PDB_NUL_TERMINATED 0x100
int fcz_decompress_pdb_begin(fcz_ctx* ctx, const uint8_t* blob, const uint64_t* off, uint32_t n, int alt_order,
                             uint64_t* text_off, int32_t* status);
int fcz_decompress_pdb_fetch(fcz_ctx* ctx, uint8_t* text_out);
/* The sizes half of begin(): the entries are decoded on the device and text_off[n+1] / status[n] filled exactly as begin() fills
 * them (a line's width depends on the decoded numbers: printf widens a column that overflows), but no text is formatted or kept.
 * What a rank of a sharded `decompress --db` run calls over its range BEFORE it writes, so that the ranks exchange their record
 * and byte counts first and every record is appended once at its final offset -- writer_append, src/database_writer.cpp:36-58,
 * called once per record from src/main.cpp:656-664. */
int fcz_decompress_pdb_sizes(fcz_ctx* ctx, const uint8_t* blob, const uint64_t* off, uint32_t n, int alt_order,
                             uint64_t* text_off, int32_t* status);

/* ---- dense model-input tensors ------------------------------------------------------------------ */
/* Decoded chains as the padded arrays protein models read (atom37 / atom14 coordinates with a mask, residue types, pLDDT), built
 * on the device from what fcz_decompress_batch_dev filled: no text, no host copy of the result. They stand beside
 * Foldcomp::decompress (src/foldcomp.cpp:779), which ends at a flat vector<AtomCoordinate>; the reference has no dense output.
 * Layouts (A = fcz_dense_width): the slot of an atom depends on its name and its residue only, never on the order the atoms were
 * decoded in (alt_order tells the call which order atoms_dev holds; the tensors are the same either way).
 *   FCZ_DENSE_ATOM37    A = 37  slot = position of the atom's name in
 *                               N CA C CB O CG CG1 CG2 OG OG1 SG CD CD1 CD2 ND1 ND2 OD1 OD2 SD CE CE1 CE2 CE3 NE NE1 NE2 OE1 OE2
 *                               CH2 NH1 NH2 OH CZ CZ2 CZ3 NZ OXT; the chain's OXT goes to slot 36 of its last residue
 *   FCZ_DENSE_ATOM14    A = 14  slot j = the atom fcz_res_code_atom(res_code, j, 0) names; the OXT is dropped
 *   FCZ_DENSE_BACKBONE4 A = 4   N, CA, C, O; everything else is dropped
 * Outputs for n entries padded (or cropped) to L residues, row-major, caller-owned; every byte of every array is written:
 *   pos [n][L][A][3] float32 coordinates, 0.0f where mask is 0       mask [n][L][A] uint8   1 where the decoder emitted the atom
 *   aatype [n][L] uint8      min(res_code, 20); padding 20           plddt [n][L] float32   bfac_res; padding 0
 *   res_index [n][L] int32   first_res_index + l; padding 0          length [n] uint32      residues of the entry, UNCROPPED
 * An entry longer than L keeps its first L residues (its OXT leaves with its last residue); an entry the decoder skips
 * (fcz_entry_info.status != FCZ_OK) has length 0 and padding only. aatype, plddt, res_index, length may be NULL (not wanted).
 * Sizes: every index is 64-bit -- n * L * A may exceed 2^32 elements (a pos array beyond 16 GiB); nothing wraps. */
enum fcz_dense_layout { FCZ_DENSE_ATOM37 = 0, FCZ_DENSE_ATOM14 = 1, FCZ_DENSE_BACKBONE4 = 2 };
typedef struct fcz_dense_out {
    float*    pos;          /* [n][L][A][3] */
    uint8_t*  mask;         /* [n][L][A] */
    uint8_t*  aatype;       /* [n][L] optional */
    float*    plddt;        /* [n][L] optional */
    int32_t*  res_index;    /* [n][L] optional */
    uint32_t* length;       /* [n] optional */
} fcz_dense_out;
/* pure host: 37 / 14 / 4, -1 for an unknown layout */
int fcz_dense_width(int layout);
/* pure host, the table the kernel uses: slot of atom_code in a residue of res_code, -1 when the residue has no such atom, the
 * layout no slot for it, or a code is out of range (atom code 255, residue codes outside 0 .. 23) */
int fcz_dense_slot(int layout, int res_code, int atom_code);
/* Device-resident: every pointer (those inside atoms_dev / out_dev too) a device pointer; atoms_dev = what
 * fcz_decompress_batch_dev filled for the same entries and offsets (x, y, z, bfac_res, res_code required), as for
 * fcz_pdb_format_dev. Enqueued on the ctx stream, no synchronisation. Unknown layout, L == 0, NULL pos or mask:
 * FCZ_E_INVALID_ARG, nothing launched; n == 0: FCZ_OK. */
int fcz_dense_dev(fcz_ctx* ctx, const uint8_t* blob_dev, const uint64_t* off_dev, uint32_t n,
                  const uint32_t* res_off_dev, const uint32_t* atom_off_dev, const fcz_atoms_out* atoms_dev, int alt_order,
                  int layout, uint32_t L, const fcz_dense_out* out_dev);
/* Host-pointer convenience: records in, dense host arrays out; decodes through the ctx like fcz_decompress_batch
 * (Foldcomp::read + Foldcomp::decompress, src/foldcomp.cpp:904 / :779, for every entry). L = 0: the longest entry of the batch;
 * the width used comes back through *L_out (may be NULL), so a first call with out = NULL sizes the arrays. status[n] (may be
 * NULL) receives the per-entry fcz_status. */
int fcz_decompress_dense(fcz_ctx* ctx, const uint8_t* blob, const uint64_t* off, uint32_t n, int layout, uint32_t L,
                         uint32_t* L_out, const fcz_dense_out* out, int32_t* status);

/* ---- a per-entry residue window of the padded tensors: a crop at an offset ------------------------------ */
/* Beside fcz_dense_dev, which can only keep an entry's FIRST L residues (like it, beside Foldcomp::decompress, src/foldcomp.cpp:779;
 * the reference has no dense output and no crop). start_dev[e] (uint32, device data, [n]) is the first residue of entry e that is
 * kept: row l of the output holds residue start[e] + l when that is below the entry's length, and is a padding row otherwise. A row
 * that holds a residue equals, bit for bit, row start[e] + l of what fcz_dense_dev writes at L = the longest entry; a padding row is
 * its padding row. So the atom37 OXT (slot 36) appears only when the window contains the entry's last residue, res_index is
 * first_res_index + start[e] + l, and length[e] stays the UNCROPPED residue count. start[e] >= length is no error (the starts are
 * device data: no entry point can check them on the host): all L rows are padding, 0xFFFFFFFF included -- start[e] + l never wraps.
 * A skipped entry is padding only. start_dev == NULL means all zeros: the output is then byte-identical to fcz_dense_dev's.
 * Arguments, refusals, stream and sizes are fcz_dense_dev's; the time goes to its "dense" group. */
int fcz_dense_window_dev(fcz_ctx* ctx, const uint8_t* blob_dev, const uint64_t* off_dev, uint32_t n,
                         const uint32_t* res_off_dev, const uint32_t* atom_off_dev, const fcz_atoms_out* atoms_dev, int alt_order,
                         int layout, uint32_t L, const uint32_t* start_dev, const fcz_dense_out* out_dev);
/* Host-pointer convenience, beside fcz_decompress_dense and shaped like it (Foldcomp::read + Foldcomp::decompress,
 * src/foldcomp.cpp:904 / :779, for every entry): start[n] is a host array (NULL: all zeros). L = 0 is the longest entry of the
 * batch, the width used comes back through *L_out, and a first call with out = NULL sizes the arrays. Refusals are
 * fcz_decompress_dense's. */
int fcz_decompress_dense_window(fcz_ctx* ctx, const uint8_t* blob, const uint64_t* off, uint32_t n, int layout, uint32_t L,
                                const uint32_t* start, uint32_t* L_out, const fcz_dense_out* out, int32_t* status);

/* ---- packed dense tensors: rows of all entries back to back, no padding ------------------------------ */
/* The same tensors for a batch of mixed lengths, as varlen models and token-budget loaders read them: no common L, no padding row
 * and no crop. Like the padded form they stand beside Foldcomp::decompress (src/foldcomp.cpp:779); the reference has no such output.
 * For n entries, R = res_off[n] (what fcz_decompress_sizes_dev leaves on the device and reports as *total_res) is the number of
 * residues of the entries the decoder accepts; an entry it skips has ZERO rows. Row res_off[e] + l is residue l of entry e, so
 * res_off itself is the cu_seqlens of the batch: no second copy is written.
 *   pos [R][A][3] float32     mask [R][A] uint8     aatype [R] uint8     plddt [R] float32     res_index [R] int32
 *   chain_index [R] int32     the entry number e of the row (segment reductions, block-diagonal attention masks)
 *   length [n] uint32         residues of the entry, 0 for a skipped one
 * aatype, plddt, res_index, chain_index, length may be NULL (not wanted). A slot's value follows the padded rules: the
 * fcz_dense_slot table, the chain's OXT in slot 36 of its last row in atom37, pos 0.0f where mask is 0, aatype min(res_code, 20),
 * res_index first_res_index + l. Every byte of rows 0 .. R - 1 of every requested array is written exactly once and nothing outside
 * them; R == 0 writes length only. Every index is 64-bit (R * 111 floats passes 2^32 at 38.7 M residues). */
typedef struct fcz_packed_out {
    float*    pos;          /* [R][A][3] */
    uint8_t*  mask;         /* [R][A] */
    uint8_t*  aatype;       /* [R] optional */
    float*    plddt;        /* [R] optional */
    int32_t*  res_index;    /* [R] optional */
    int32_t*  chain_index;  /* [R] optional */
    uint32_t* length;       /* [n] optional */
} fcz_packed_out;
/* Device-resident, beside fcz_dense_dev and with its arguments but L: every pointer a device pointer, atoms_dev = what
 * fcz_decompress_batch_dev filled for the same entries and offsets, the arrays of out_dev allocated for the R rows the sizes call
 * reported. Enqueued on the ctx stream, no synchronisation: the kernel reads R from res_off_dev[n]. Unknown layout, NULL pos or
 * mask (or any other required pointer): FCZ_E_INVALID_ARG, nothing launched; n == 0: FCZ_OK. */
int fcz_dense_packed_dev(fcz_ctx* ctx, const uint8_t* blob_dev, const uint64_t* off_dev, uint32_t n,
                         const uint32_t* res_off_dev, const uint32_t* atom_off_dev, const fcz_atoms_out* atoms_dev, int alt_order,
                         int layout, const fcz_packed_out* out_dev);
/* Host-pointer convenience, beside fcz_decompress_dense (Foldcomp::read + Foldcomp::decompress, src/foldcomp.cpp:904 / :779, for
 * every entry): records in, packed host arrays out. *R_out (may be NULL when out is given) receives R and row_off[n + 1] (may be
 * NULL) the row offsets, so a first call with out = NULL sizes the arrays. status[n] (may be NULL) receives the per-entry
 * fcz_status. NULL ctx / blob / off, unknown layout, out and R_out both NULL, out with NULL pos or mask: FCZ_E_INVALID_ARG. */
int fcz_decompress_dense_packed(fcz_ctx* ctx, const uint8_t* blob, const uint64_t* off, uint32_t n, int layout,
                                uint32_t* R_out, uint32_t* row_off, const fcz_packed_out* out, int32_t* status);

/* ---- k-nearest-neighbour residue graph of the dense tensors ---------------------------------------------- */
/* The neighbour lists graph models start from (the k nearest CA or CB sites of every residue), built on the device from the dense
 * tensors above without the L x L distance matrix. The reference has no such output: like the dense calls these stand beside
 * Foldcomp::decompress (src/foldcomp.cpp:779) and read what fcz_dense_dev / fcz_dense_window_dev / fcz_dense_packed_dev wrote, or
 * any tensors of those shapes. Padded: pos [n][L][A][3] float32, mask [n][L][A] uint8, length [n] uint32 (may be NULL). Packed:
 * pos [R][A][3], mask [R][A], row_off [n + 1] uint32. A = fcz_dense_width(layout), slot in 0 .. A - 1 (CA is slot 1 in every
 * layout, CB slot 3 in atom37 and slot 4 in atom14), 1 <= k <= 64.
 *   site        row l of chain e is a site when it lies inside the chain (padded: l < min(length[e], L), or l < L when length is
 *               NULL; packed: row_off[e] <= row < row_off[e + 1], both clamped to R, a range that runs backwards being empty),
 *               mask[row][slot] != 0, and the three coordinates at the slot are finite. Rows outside the chain and pos under a
 *               cleared mask are never read as data: they may hold anything, so a window batch needs no length.
 *   distance    for sites i, j of one chain: dx = xj - xi, dy, dz in float32, d2 = (dx*dx + dy*dy) + dz*dz, every operation rounded
 *               to float32, no FMA; d2 may be +inf.
 *   neighbours  of site i: the other sites j of its chain ordered by (bits of d2 as uint32, j) ascending, the first
 *               min(k, sites - 1) of them, in that order.
 *   index [rows][k] int32    j as a row of the entry (padded, 0 .. L - 1) or as the global row row_off[e] + j (packed)
 *   dist  [rows][k] float32  the correctly rounded float32 square root of d2
 * rows = n * L (padded) or R (packed). Unused columns, rows that are no site and packed rows no chain covers hold index -1 and
 * dist 0.0f. Every byte of both outputs is written whatever the inputs hold, nothing outside them is written, and nothing outside
 * pos / mask / length / row_off is read, whatever row_off holds (ranges that overlap are each computed; which of them a shared
 * row's list belongs to is then unspecified). Every index that scales with rows * k or rows * A is 64-bit.
 * Candidates are staged per chain in passes of fcz_knn_pass() rows (pure host; 0 would mean no passes): a chain longer than that
 * takes several, with the same result. Enqueued on the ctx stream, no synchronisation (the packed form keeps n + n + 1 words of
 * scratch in the ctx). FCZ_E_INVALID_ARG with nothing launched: NULL ctx / pos / mask / index / dist, NULL row_off with n > 0,
 * unknown layout, slot outside the layout's width, k outside 1 .. 64, L == 0,
 * packed R above 2^31 - 1 (index holds global rows as int32; the padded form holds rows of the entry, any n * L).
 * n == 0 or R == 0: FCZ_OK (packed, n == 0 < R: every row is uncovered and is filled). The time goes to a group of its own,
 * "knn", for both forms. */
int fcz_knn_pass(void);
int fcz_knn_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint32_t* length_dev, uint32_t n, uint32_t L,
                int layout, int slot, uint32_t k, int32_t* index_dev, float* dist_dev);
int fcz_knn_packed_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint32_t* row_off_dev, uint32_t n,
                       uint32_t R, int layout, int slot, uint32_t k, int32_t* index_dev, float* dist_dev);
/* Host-pointer conveniences: the same arrays on the host, staged through the ctx like fcz_decompress_dense; synchronous. */
int fcz_knn(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint32_t* length, uint32_t n, uint32_t L, int layout,
            int slot, uint32_t k, int32_t* index, float* dist);
int fcz_knn_packed(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint32_t* row_off, uint32_t n, uint32_t R,
                   int layout, int slot, uint32_t k, int32_t* index, float* dist);

/* ---- per-residue lDDT of two dense tensor batches --------------------------------------------------------- */
/* The superposition-free score of predicted coordinates against true ones (Mariani et al. 2013; the lDDT-CA a pLDDT head is trained
 * on), per residue, for a whole batch on the device without the L x L distance matrices. The reference has no such output: like
 * fcz_knn_dev these stand beside Foldcomp::decompress (src/foldcomp.cpp:779) and read what the dense calls wrote, or any tensors of
 * those shapes. Two tensors of ONE shape and layout: pos_true / mask_true and pos_pred / mask_pred (mask_pred may be NULL: every
 * slot present). Padded: pos [n][L][A][3] float32, mask [n][L][A] uint8, length [n] uint32 (may be NULL). Packed: pos [R][A][3],
 * mask [R][A], row_off [n + 1] uint32. A = fcz_dense_width(layout), slot in 0 .. A - 1 as for fcz_knn_dev, cutoff float32 (15 is
 * the usual inclusion radius), thresholds: four float32 on the HOST in every form (NULL: 0.5, 1, 2, 4).
 *   site        row l of chain e is a site when it lies inside the chain (fcz_knn_dev's rules: padded l < min(length[e], L), or
 *               l < L when length is NULL; packed row_off[e] <= row < row_off[e + 1], both clamped to R, a range that runs
 *               backwards being empty), mask_true[row][slot] != 0, mask_pred[row][slot] != 0 (if a mask was given) and all six
 *               coordinates at the slot are finite. Nothing else is read as data: rows outside the chain and pos under a cleared
 *               mask may hold anything.
 *   distances   for sites i, j of one chain and each of the two tensors: d2 = (dx*dx + dy*dy) + dz*dz in float32, every operation
 *               rounded, no FMA (fcz_knn_dev's d2); d = the correctly rounded float32 square root of d2.
 *   pairs       j counts for i when j != i and d_true(i, j) < cutoff, compared in float32; a d_true of +inf is no pair.
 *               pairs[i] = the number of such j.
 *   hits        diff = |d_true - d_pred|, one rounded float32 subtraction; hits[i] = sum over the pairs j and the four thresholds t
 *               of [diff < thresholds[t]]. A NaN or +inf diff (a d_pred of +inf) is a pair with no hit.
 *   score [rows] float32     (float)hits / (float)(4 * pairs), a single rounded float32 division; 0.0 where pairs == 0
 *   pairs [rows] int32, hits [rows] int32
 * rows = n * L (padded) or R (packed). Rows that are no site, rows behind length and packed rows no chain covers hold 0 / 0 / 0.
 * Every byte of the three outputs is written whatever the inputs hold, nothing outside them is written, and nothing outside the
 * inputs is read, whatever row_off holds (ranges that overlap are each computed; which of them a shared row's values belong to is
 * then unspecified). Every index that scales with rows * A is 64-bit. The counters are integers, so the result does not depend on
 * any order of evaluation: it is reproducible bit for bit. It is NOT differentiable: these are counts.
 * Candidates are staged per chain in passes of fcz_lddt_pass() rows (pure host, > 0): a longer chain takes several, with the same
 * result. fcz_lddt_c2(cutoff) (pure host) is the bound the kernel compares d2_true with: the smallest float32 whose correctly
 * rounded root is >= cutoff, so that d2_true < c2 <=> d_true < cutoff (+inf when no finite d2 reaches the cutoff; NaN for a cutoff
 * the calls refuse). Enqueued on the ctx stream, no synchronisation (the packed form shares fcz_knn_packed_dev's scratch in the
 * ctx). FCZ_E_INVALID_ARG with nothing launched: NULL ctx / pos_true / mask_true / pos_pred / score / pairs / hits, NULL row_off
 * with n > 0, unknown layout, slot outside the layout's width, L == 0, a cutoff that is not finite and > 0, a threshold that is NaN,
 * L (padded) or R (packed) above 2^29 (hits must fit int32). n == 0 or R == 0: FCZ_OK (packed, n == 0 < R: every row is uncovered
 * and is filled). The time goes to a group of its own, "lddt", for both forms. */
int fcz_lddt_pass(void);
float fcz_lddt_c2(float cutoff);
int fcz_lddt_dev(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev,
                 const uint8_t* mask_pred_dev, const uint32_t* length_dev, uint32_t n, uint32_t L, int layout, int slot, float cutoff,
                 const float* thresholds, float* score_dev, int32_t* pairs_dev, int32_t* hits_dev);
int fcz_lddt_packed_dev(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev,
                        const uint8_t* mask_pred_dev, const uint32_t* row_off_dev, uint32_t n, uint32_t R, int layout, int slot,
                        float cutoff, const float* thresholds, float* score_dev, int32_t* pairs_dev, int32_t* hits_dev);
/* Host-pointer conveniences: the same arrays on the host, staged through the ctx like fcz_knn; synchronous. */
int fcz_lddt(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, const uint8_t* mask_pred,
             const uint32_t* length, uint32_t n, uint32_t L, int layout, int slot, float cutoff, const float* thresholds,
             float* score, int32_t* pairs, int32_t* hits);
int fcz_lddt_packed(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, const uint8_t* mask_pred,
                    const uint32_t* row_off, uint32_t n, uint32_t R, int layout, int slot, float cutoff, const float* thresholds,
                    float* score, int32_t* pairs, int32_t* hits);

/* ---- smooth lDDT and its gradient ------------------------------------------------------------------------- */
/* The differentiable form of fcz_lddt_dev: the smooth lDDT of AlphaFold 3 (Abramson et al. 2024, Algorithm 27), each step function
 * of the score replaced by a sigmoid, with a fused backward pass, for a whole batch on the device without an L x L matrix in either
 * direction. The reference has no such output. The inputs, the forms (padded / packed), sites, chains, distances (d2, d = the
 * correctly rounded root) and the PAIRS are fcz_lddt_dev's, unchanged: j is a pair of i when j != i and d2_true < fcz_lddt_c2(cutoff).
 * pairs [rows] int32 equals fcz_lddt_dev's pairs on the same inputs exactly. thresholds: four FINITE float32 on the host (NULL: 0.5,
 * 1, 2, 4). For a pair
 *   delta = |d_true - d_pred|                      one rounded float32 subtraction
 *   eps(delta) = 1/4 sum_k sigmoid(t_k - delta)    over the four thresholds; 0 when delta is not finite (a d_pred of +inf)
 * Value (fcz_lddt_soft_dev):
 *   soft [rows] float32   the sum of eps over the pairs j of row i, in float32, in ASCENDING ROW ORDER of j within the chain. The
 *                         order is fixed: it does not depend on the tile, the pass, the launch geometry or the other chains of the
 *                         batch, so the same chain gives the same bytes alone, in any batch, padded or packed, call after call.
 *                         0 where the row is no site or has no pair.
 *   pairs [rows] int32
 * Gradient (fcz_lddt_soft_grad_dev), for the caller's row weights weight [rows] float32, the upstream gradient of soft: with
 * eps'(delta) = -1/4 sum_k s_k (1 - s_k), s_k = sigmoid(t_k - delta),
 *   grad [rows][3] float32   grad[i] = sum over the pairs j of (w_i + w_j) eps'(delta_ij) sign(d_pred - d_true) (p_i - p_j) / d_pred,
 *                         again in ascending j, in float32: the gradient of sum_i w_i soft[i] with respect to the predicted
 *                         coordinates of row i at the slot. sign(0) = 0: a pair at delta == 0 adds nothing (the subgradient of
 *                         |x| that torch takes). A pair whose d_pred is 0 or not finite adds nothing. The pair relation is
 *                         symmetric, pair (i, j) stands in soft[i] and in soft[j]: hence (w_i + w_j), and row i gathers its whole
 *                         gradient itself. No atomics, no scatter: the result is reproducible bit for bit. 0 where the row is no
 *                         site. The weights of rows that are no site are not read as data.
 * The sigmoid is 1 / (1 + e^-x) with the hardware's exp2 of a scaled argument and its reciprocal (foldcomp_amd/csrc/fcz_lddt_soft.h):
 * a term is within 2^-19 of its exact value for distances under 64 A, |soft - exact| <= P 2^-19 + P^2 2^-24 for a row of P pairs.
 * Everything behind soft (soft / pairs, the quotient of a chain, 1 - ...) is the caller's arithmetic.
 * rows = n * L (padded) or R (packed). Every byte of the outputs is written whatever the inputs hold, nothing outside them, and
 * nothing outside the inputs is read, whatever row_off holds (as for fcz_lddt_dev). Passes are fcz_lddt_pass() rows. Enqueued on the
 * ctx stream, no synchronisation. FCZ_E_INVALID_ARG with nothing launched and no output touched: what fcz_lddt_dev refuses (its
 * outputs here being soft / pairs, or weight / grad), and a threshold that is not finite. n == 0 or R == 0: FCZ_OK. The time goes to
 * the groups "lddt_soft" and "lddt_soft_grad". */
int fcz_lddt_soft_dev(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev,
                      const uint8_t* mask_pred_dev, const uint32_t* length_dev, uint32_t n, uint32_t L, int layout, int slot,
                      float cutoff, const float* thresholds, float* soft_dev, int32_t* pairs_dev);
int fcz_lddt_soft_packed_dev(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev,
                             const uint8_t* mask_pred_dev, const uint32_t* row_off_dev, uint32_t n, uint32_t R, int layout, int slot,
                             float cutoff, const float* thresholds, float* soft_dev, int32_t* pairs_dev);
int fcz_lddt_soft_grad_dev(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev,
                           const uint8_t* mask_pred_dev, const uint32_t* length_dev, uint32_t n, uint32_t L, int layout, int slot,
                           float cutoff, const float* thresholds, const float* weight_dev, float* grad_dev);
int fcz_lddt_soft_grad_packed_dev(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev,
                                  const uint8_t* mask_pred_dev, const uint32_t* row_off_dev, uint32_t n, uint32_t R, int layout,
                                  int slot, float cutoff, const float* thresholds, const float* weight_dev, float* grad_dev);
/* Host-pointer conveniences: the same arrays on the host, staged through the ctx like fcz_lddt; synchronous. */
int fcz_lddt_soft(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, const uint8_t* mask_pred,
                  const uint32_t* length, uint32_t n, uint32_t L, int layout, int slot, float cutoff, const float* thresholds,
                  float* soft, int32_t* pairs);
int fcz_lddt_soft_packed(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred,
                         const uint8_t* mask_pred, const uint32_t* row_off, uint32_t n, uint32_t R, int layout, int slot, float cutoff,
                         const float* thresholds, float* soft, int32_t* pairs);
int fcz_lddt_soft_grad(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, const uint8_t* mask_pred,
                       const uint32_t* length, uint32_t n, uint32_t L, int layout, int slot, float cutoff, const float* thresholds,
                       const float* weight, float* grad);
int fcz_lddt_soft_grad_packed(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred,
                              const uint8_t* mask_pred, const uint32_t* row_off, uint32_t n, uint32_t R, int layout, int slot,
                              float cutoff, const float* thresholds, const float* weight, float* grad);

/* ---- backbone FAPE and its gradient ----------------------------------------------------------------------- */
/* The frame aligned point error that frame-based structure models train on (Jumper et al. 2021, supplement, Algorithm 28), of the
 * rigid frames and the points of one slot of a prediction against the truth's, with a fused backward pass, for a whole batch on the
 * device without an L x L array in either direction. The reference has no such output. Everything is per chain, padded or packed,
 * with fcz_lddt_dev's chain rules (length / row_off, ranges clamped, a range that runs backwards empty).
 * Frames: rot [rows][3][3], trans [rows][3] float32 with global = rot . local + trans (fcz_frames_dev's convention, columns are the
 * axes) and frame_mask [rows] bytes, for the truth and for the prediction. Row i is a FRAME when it lies inside its chain,
 * fmask_true[i] != 0, fmask_pred[i] != 0 (a NULL fmask_pred is all set) and all 24 floats are finite.
 * Points: pos [rows][A][3], mask [rows][A] of both. Row j is a POINT when it lies inside its chain, both masks at `slot` are set (a
 * NULL mask_pred is all set) and its six coordinates are finite (the site rule of fcz_lddt_dev).
 * Term, for frame i and point j of the same chain, j == i included; unprimed is the prediction, primed the truth:
 *   u  = x_j - t_i            u' = x'_j - t'_i          three subtractions each
 *   l  = R_i^T u              l' = R'_i^T u'            l_k = (R[0][k]*u0 + R[1][k]*u1) + R[2][k]*u2
 *   e  = l - l'               s = (e0*e0 + e1*e1) + e2*e2
 *   d  = sqrt(s + eps)        correctly rounded         term = min(d, clamp)
 * all float32, every operation a single rounded one, no FMA. eps is finite and > 0 (Algorithm 28: 1e-4 A^2), clamp > 0 with +inf
 * for unclamped. A d that is not finite adds nothing and has no gradient.
 * Value (fcz_fape_dev):
 *   sum [rows] float32    at a frame row the sum of term over the chain's points, in float32, in ASCENDING ROW ORDER of j; 0 elsewhere
 *   points [rows] int32   at a frame row the number of points of its chain (whatever their d); 0 elsewhere
 * Dividing by points, by the scale Z and by the number of frames is the caller's arithmetic.
 * Gradient (fcz_fape_grad_dev) of sum_i w_i sum[i] for the caller's weight [rows] float32, with respect to the prediction's rot
 * (the unconstrained partial derivative of its nine entries), trans and the slot's coordinates. With inv = the hardware reciprocal
 * of d (within an ulp) and h = (e0 * inv, e1 * inv, e2 * inv) where d is finite and d < clamp, and no term otherwise:
 *   grad_rot [rows][3][3]   grad_rot[i][a][k] = w_i * M[a][k], M[a][k] the sum over j, ascending, of u_a * h_k
 *   grad_trans [rows][3]    grad_trans[i][a] = -(w_i * ((R[a][0]*H0 + R[a][1]*H1) + R[a][2]*H2)), H the sum over j, ascending, of h
 *   grad_pos [rows][3]      grad_pos[j][a] = the sum over i, ascending, of w_i * ((R_i[a][0]*h0 + R_i[a][1]*h1) + R_i[a][2]*h2)
 * every product and sum one rounded float32 operation. grad_rot and grad_trans are 0 at rows that are no frame, grad_pos at rows that
 * are no point; a point's gradient belongs to pos_pred[j][slot]. One writer per output, no atomics, no scatter: the same chain gives
 * the same bytes alone, in any batch, padded or packed, call after call. Weights of rows that are no frame are not read as data.
 * When the prediction's points ARE its translations (AlphaFold's backbone FAPE) the caller adds grad_pos to grad_trans.
 * Error, for rotations with orthonormal columns: with X the largest of |u|_inf, |u'|_inf of a term, |d - exact| <= (26 X + 4 d) 2^-24
 * (tests/_fape.py derives it and the bounds of the sums).
 * rows = n * L (padded) or R (packed). Every byte of the outputs is written whatever the inputs hold, nothing outside them, and
 * nothing outside the inputs is read, whatever row_off holds. Every index that scales with rows * A is 64-bit. Passes are at most
 * fcz_fape_pass() rows. Enqueued on the ctx stream, no synchronisation; one gradient call enqueues both of its sweeps.
 * FCZ_E_INVALID_ARG with nothing launched and no output touched: a NULL required pointer (everything but fmask_pred, mask_pred and
 * the padded form's length), NULL row_off with n > 0, an unknown layout, a slot outside the layout's width, L == 0, L or R above
 * 2^29, a clamp that is NaN or not > 0, an eps that is not finite or not > 0. n == 0 or R == 0: FCZ_OK. The time goes to the groups
 * "fape" and "fape_grad". */
int fcz_fape_pass(void);
int fcz_fape_dev(fcz_ctx* ctx, const float* rot_true_dev, const float* trans_true_dev, const uint8_t* fmask_true_dev,
                 const float* pos_true_dev, const uint8_t* mask_true_dev, const float* rot_pred_dev, const float* trans_pred_dev,
                 const uint8_t* fmask_pred_dev, const float* pos_pred_dev, const uint8_t* mask_pred_dev, const uint32_t* length_dev,
                 uint32_t n, uint32_t L, int layout, int slot, float clamp, float eps, float* sum_dev, int32_t* points_dev);
int fcz_fape_packed_dev(fcz_ctx* ctx, const float* rot_true_dev, const float* trans_true_dev, const uint8_t* fmask_true_dev,
                        const float* pos_true_dev, const uint8_t* mask_true_dev, const float* rot_pred_dev, const float* trans_pred_dev,
                        const uint8_t* fmask_pred_dev, const float* pos_pred_dev, const uint8_t* mask_pred_dev,
                        const uint32_t* row_off_dev, uint32_t n, uint32_t R, int layout, int slot, float clamp, float eps,
                        float* sum_dev, int32_t* points_dev);
int fcz_fape_grad_dev(fcz_ctx* ctx, const float* rot_true_dev, const float* trans_true_dev, const uint8_t* fmask_true_dev,
                      const float* pos_true_dev, const uint8_t* mask_true_dev, const float* rot_pred_dev, const float* trans_pred_dev,
                      const uint8_t* fmask_pred_dev, const float* pos_pred_dev, const uint8_t* mask_pred_dev,
                      const uint32_t* length_dev, uint32_t n, uint32_t L, int layout, int slot, float clamp, float eps,
                      const float* weight_dev, float* grad_rot_dev, float* grad_trans_dev, float* grad_pos_dev);
int fcz_fape_grad_packed_dev(fcz_ctx* ctx, const float* rot_true_dev, const float* trans_true_dev, const uint8_t* fmask_true_dev,
                             const float* pos_true_dev, const uint8_t* mask_true_dev, const float* rot_pred_dev,
                             const float* trans_pred_dev, const uint8_t* fmask_pred_dev, const float* pos_pred_dev,
                             const uint8_t* mask_pred_dev, const uint32_t* row_off_dev, uint32_t n, uint32_t R, int layout, int slot,
                             float clamp, float eps, const float* weight_dev, float* grad_rot_dev, float* grad_trans_dev,
                             float* grad_pos_dev);
/* Host-pointer conveniences: the same arrays on the host, staged through the ctx like fcz_lddt_soft; synchronous. */
int fcz_fape(fcz_ctx* ctx, const float* rot_true, const float* trans_true, const uint8_t* fmask_true, const float* pos_true,
             const uint8_t* mask_true, const float* rot_pred, const float* trans_pred, const uint8_t* fmask_pred, const float* pos_pred,
             const uint8_t* mask_pred, const uint32_t* length, uint32_t n, uint32_t L, int layout, int slot, float clamp, float eps,
             float* sum, int32_t* points);
int fcz_fape_packed(fcz_ctx* ctx, const float* rot_true, const float* trans_true, const uint8_t* fmask_true, const float* pos_true,
                    const uint8_t* mask_true, const float* rot_pred, const float* trans_pred, const uint8_t* fmask_pred,
                    const float* pos_pred, const uint8_t* mask_pred, const uint32_t* row_off, uint32_t n, uint32_t R, int layout,
                    int slot, float clamp, float eps, float* sum, int32_t* points);
int fcz_fape_grad(fcz_ctx* ctx, const float* rot_true, const float* trans_true, const uint8_t* fmask_true, const float* pos_true,
                  const uint8_t* mask_true, const float* rot_pred, const float* trans_pred, const uint8_t* fmask_pred,
                  const float* pos_pred, const uint8_t* mask_pred, const uint32_t* length, uint32_t n, uint32_t L, int layout, int slot,
                  float clamp, float eps, const float* weight, float* grad_rot, float* grad_trans, float* grad_pos);
int fcz_fape_grad_packed(fcz_ctx* ctx, const float* rot_true, const float* trans_true, const uint8_t* fmask_true, const float* pos_true,
                         const uint8_t* mask_true, const float* rot_pred, const float* trans_pred, const uint8_t* fmask_pred,
                         const float* pos_pred, const uint8_t* mask_pred, const uint32_t* row_off, uint32_t n, uint32_t R, int layout,
                         int slot, float clamp, float eps, const float* weight, float* grad_rot, float* grad_trans, float* grad_pos);

/* ---- all-atom FAPE over the eight rigid groups and its gradient ------------------------------------------ */
/* The other half of AlphaFold 2's structure-module FAPE (Jumper et al. 2021, supplement 1.9.2): the frame aligned point error of
 * all eight rigid groups of every residue against every atom of the chain, after the truth has been renamed towards the prediction
 * where a side chain has two equivalent namings. For a whole batch on the device with a fused backward pass and without a
 * frames x atoms array in either direction. The reference has no such output. Chains follow fcz_fape_dev's rules, padded (length
 * or NULL) or packed (row_off); the layout is atom37, atom14 or backbone4.
 * Inputs: rot [rows][8][3][3], trans [rows][8][3] float32 and frame_mask [rows][8] bytes of the truth and of the prediction (what
 * fcz_frames_dev writes for FCZ_FRAMES_ALL, global = rot . local + trans, columns are the axes); pos [rows][A][3], mask [rows][A]
 * of both; aatype [rows] or NULL; swapped [rows] bytes or NULL (fcz_lddt_atoms_dev's output: rows whose truth is read under its
 * other naming); swap_table host uint8 [21][A] or NULL for fcz_lddt_default_swaps, validated as fcz_lddt_atoms_dev validates it.
 * With type = min(aatype[r], 20) and row r SWAPPED when swapped and aatype are given and swapped[r] != 0:
 * FRAME. Item (r, g), g in 0 .. 7, is a FRAME when row r lies inside its chain, fmask_true[r][g] != 0, fmask_pred is NULL or
 *   fmask_pred[r][g] != 0, and the 24 floats of both sides are finite; in backbone4 only g = 0 and g = 3 can be frames, whatever
 *   the masks hold, and nothing is renamed. Where r is swapped and fcz_frame_ambiguous(type, g) (type 20: never) the truth's
 *   rotation is read with its second and third columns negated, rot' . diag(1, -1, -1), AlphaFold's rigidgroups_alt_gt_frames:
 *   R'[a][1] and R'[a][2] change sign, which is exact.
 * POINT. Slot (r, a) is a POINT when row r lies inside its chain and, with s = swap_table[type][a] where r is swapped and s = a
 *   elsewhere, mask_true[r][s] != 0, mask_pred is NULL or mask_pred[r][a] != 0, and pos_true[r][s] and pos_pred[r][a] are finite.
 *   The point's true coordinates are pos_true[r][s], its predicted ones pos_pred[r][a].
 * Term. Every frame of a chain meets every point of that chain, its own residue's included. The term is fcz_fape_dev's,
 * operation for operation, unprimed the prediction and primed the truth:
 *   u  = x - t                u' = x' - t'              three subtractions each
 *   l  = R^T u                l' = R'^T u'              l_k = (R[0][k]*u0 + R[1][k]*u1) + R[2][k]*u2
 *   e  = l - l'               s = (e0*e0 + e1*e1) + e2*e2
 *   d  = sqrt(s + eps)        correctly rounded         term = min(d, clamp)
 * all float32, every operation a single rounded one, no FMA. A d that is not finite counts as a point and adds nothing.
 * Value (fcz_fape_atoms_dev):
 *   sum [rows][8] float32    at a frame the sum of term over the chain's points in ASCENDING (row, slot), in float32; 0 elsewhere
 *   points [rows][8] int32   at a frame the number of points of its chain (whatever their d); 0 elsewhere
 * Gradient (fcz_fape_atoms_grad_dev) of sum_{r,g} w[r][g] * sum[r][g] for the caller's weight [rows][8] float32, with fcz_fape_grad_dev's
 * h = (e0 * inv, e1 * inv, e2 * inv), inv the hardware reciprocal of d, where d is finite and d < clamp, and its operation orders:
 *   grad_rot [rows][8][3][3]   grad_rot[r][g][a][k] = w * M[a][k], M[a][k] the sum over the points, ascending, of u_a * h_k
 *   grad_trans [rows][8][3]    grad_trans[r][g][a] = -(w * ((R[a][0]*H0 + R[a][1]*H1) + R[a][2]*H2)), H the ascending sum of h
 *   grad_pos [rows][A][3]      at a point the sum over the chain's frames in ASCENDING (row, group) of
 *                              w * ((R[a][0]*h0 + R[a][1]*h1) + R[a][2]*h2), R the frame's predicted rotation
 * with respect to the prediction's rot (the unconstrained partial derivative of its nine entries), trans and pos_pred[r][a]. Zeros
 * at every item that is no frame, at every slot that is no point and in every row no chain covers. One writer per output element,
 * no float atomics, nothing kept from the value pass: a chain gives the same bytes alone, in any batch, padded or packed, call
 * after call. A weight is read only at a frame. The error bounds are fcz_fape_dev's with the longer sums (tests/_fape_atoms.py).
 * rows = n * L (padded) or R (packed). Every byte of the outputs is written whatever the inputs hold, nothing outside them, and
 * nothing outside the inputs is read, whatever row_off holds. Every index that scales with rows * A or rows * 8 is 64-bit. The
 * points are staged in passes of at most fcz_fape_atoms_pass(); the frame sweeps run over tiles of fcz_fape_atoms_tile_rows(layout)
 * rows. Enqueued on the ctx stream, no synchronisation; one gradient call enqueues both of its sweeps.
 * FCZ_E_INVALID_ARG with nothing launched and no output touched: fcz_fape_dev's refusals (a NULL required pointer -- everything but
 * aatype, swapped, fmask_pred, mask_pred, swap_table and the padded form's length --, NULL row_off with n > 0, an unknown layout,
 * L == 0, a clamp that is NaN or not > 0, an eps that is not finite or not > 0), a swapped without an aatype, a swap_table with an
 * entry >= A or a row that is no involution, and L or R above min(2^29, (2^31 - 1) / A): a frame's points must fit int32.
 * n == 0 or R == 0: FCZ_OK. The time goes to the groups "fape_atoms" and "fape_atoms_grad". */
int fcz_fape_atoms_pass(void);
int fcz_fape_atoms_tile_rows(int layout);
int fcz_fape_atoms_dev(fcz_ctx* ctx, const float* rot_true_dev, const float* trans_true_dev, const uint8_t* fmask_true_dev,
                       const float* pos_true_dev, const uint8_t* mask_true_dev, const uint8_t* aatype_dev, const uint8_t* swapped_dev,
                       const float* rot_pred_dev, const float* trans_pred_dev, const uint8_t* fmask_pred_dev, const float* pos_pred_dev,
                       const uint8_t* mask_pred_dev, const uint32_t* length_dev, uint32_t n, uint32_t L, int layout, float clamp,
                       float eps, const uint8_t* swap_table, float* sum_dev, int32_t* points_dev);
int fcz_fape_atoms_packed_dev(fcz_ctx* ctx, const float* rot_true_dev, const float* trans_true_dev, const uint8_t* fmask_true_dev,
                              const float* pos_true_dev, const uint8_t* mask_true_dev, const uint8_t* aatype_dev,
                              const uint8_t* swapped_dev, const float* rot_pred_dev, const float* trans_pred_dev,
                              const uint8_t* fmask_pred_dev, const float* pos_pred_dev, const uint8_t* mask_pred_dev,
                              const uint32_t* row_off_dev, uint32_t n, uint32_t R, int layout, float clamp, float eps,
                              const uint8_t* swap_table, float* sum_dev, int32_t* points_dev);
int fcz_fape_atoms_grad_dev(fcz_ctx* ctx, const float* rot_true_dev, const float* trans_true_dev, const uint8_t* fmask_true_dev,
                            const float* pos_true_dev, const uint8_t* mask_true_dev, const uint8_t* aatype_dev,
                            const uint8_t* swapped_dev, const float* rot_pred_dev, const float* trans_pred_dev,
                            const uint8_t* fmask_pred_dev, const float* pos_pred_dev, const uint8_t* mask_pred_dev,
                            const uint32_t* length_dev, uint32_t n, uint32_t L, int layout, float clamp, float eps,
                            const uint8_t* swap_table, const float* weight_dev, float* grad_rot_dev, float* grad_trans_dev,
                            float* grad_pos_dev);
int fcz_fape_atoms_grad_packed_dev(fcz_ctx* ctx, const float* rot_true_dev, const float* trans_true_dev, const uint8_t* fmask_true_dev,
                                   const float* pos_true_dev, const uint8_t* mask_true_dev, const uint8_t* aatype_dev,
                                   const uint8_t* swapped_dev, const float* rot_pred_dev, const float* trans_pred_dev,
                                   const uint8_t* fmask_pred_dev, const float* pos_pred_dev, const uint8_t* mask_pred_dev,
                                   const uint32_t* row_off_dev, uint32_t n, uint32_t R, int layout, float clamp, float eps,
                                   const uint8_t* swap_table, const float* weight_dev, float* grad_rot_dev, float* grad_trans_dev,
                                   float* grad_pos_dev);
/* Host-pointer conveniences: the same arrays on the host, staged through the ctx like fcz_fape; synchronous. */
int fcz_fape_atoms(fcz_ctx* ctx, const float* rot_true, const float* trans_true, const uint8_t* fmask_true, const float* pos_true,
                   const uint8_t* mask_true, const uint8_t* aatype, const uint8_t* swapped, const float* rot_pred, const float* trans_pred,
                   const uint8_t* fmask_pred, const float* pos_pred, const uint8_t* mask_pred, const uint32_t* length, uint32_t n,
                   uint32_t L, int layout, float clamp, float eps, const uint8_t* swap_table, float* sum, int32_t* points);
int fcz_fape_atoms_packed(fcz_ctx* ctx, const float* rot_true, const float* trans_true, const uint8_t* fmask_true, const float* pos_true,
                          const uint8_t* mask_true, const uint8_t* aatype, const uint8_t* swapped, const float* rot_pred,
                          const float* trans_pred, const uint8_t* fmask_pred, const float* pos_pred, const uint8_t* mask_pred,
                          const uint32_t* row_off, uint32_t n, uint32_t R, int layout, float clamp, float eps,
                          const uint8_t* swap_table, float* sum, int32_t* points);
int fcz_fape_atoms_grad(fcz_ctx* ctx, const float* rot_true, const float* trans_true, const uint8_t* fmask_true, const float* pos_true,
                        const uint8_t* mask_true, const uint8_t* aatype, const uint8_t* swapped, const float* rot_pred,
                        const float* trans_pred, const uint8_t* fmask_pred, const float* pos_pred, const uint8_t* mask_pred,
                        const uint32_t* length, uint32_t n, uint32_t L, int layout, float clamp, float eps, const uint8_t* swap_table,
                        const float* weight, float* grad_rot, float* grad_trans, float* grad_pos);
int fcz_fape_atoms_grad_packed(fcz_ctx* ctx, const float* rot_true, const float* trans_true, const uint8_t* fmask_true,
                               const float* pos_true, const uint8_t* mask_true, const uint8_t* aatype, const uint8_t* swapped,
                               const float* rot_pred, const float* trans_pred, const uint8_t* fmask_pred, const float* pos_pred,
                               const uint8_t* mask_pred, const uint32_t* row_off, uint32_t n, uint32_t R, int layout, float clamp,
                               float eps, const uint8_t* swap_table, const float* weight, float* grad_rot, float* grad_trans,
                               float* grad_pos);

/* ---- all-atom lDDT with symmetric side-chain renaming ------------------------------------------------------ */
/* The lDDT that CASP, CAMEO and model papers report: every heavy atom against every heavy atom of the other residues of its chain,
 * after the chemically equivalent namings of the truth's side chains (ASP OD1 / OD2, GLU OE1 / OE2, PHE and TYR CD1 / CD2 with
 * CE1 / CE2) have been resolved towards the prediction, so that a ring flipped by 180 degrees is not punished. The renaming decision
 * is an output of its own (AlphaFold's alt_naming_is_better). For a whole batch on the device, without a rows x rows or an
 * atoms x atoms array. The reference has no such output: like fcz_lddt_dev these stand beside Foldcomp::decompress
 * (src/foldcomp.cpp:779). The inputs are fcz_lddt_dev's: two tensors of ONE shape and layout, pos_true / mask_true and pos_pred /
 * mask_pred (mask_pred may be NULL: every slot present); padded pos [n][L][A][3] float32, mask [n][L][A] uint8, length [n] uint32 (may
 * be NULL); packed pos [R][A][3], mask [R][A], row_off [n + 1] uint32; and with them
 *   aatype        [n][L] / [R] uint8 or NULL. NULL: no slot has another naming, nothing is renamed. A type above 20 uses row 20.
 *   swap_table    a HOST table [21][A] uint8, handed to the kernel by value: swap_table[t][a] is the PARTNER slot of slot a in a
 *                 residue of type t, a itself where the slot has no other naming. NULL selects fcz_lddt_default_swaps(layout, ..)
 *                 (pure host): the four AlphaFold swaps above at the slots fcz_dense_slot gives the atoms, so atom37 and atom14
 *                 describe the same atoms, and none in backbone4. A table must be an involution within each row with entries < A.
 *   cutoff, thresholds   as for fcz_lddt_dev (thresholds: four float32 on the HOST, NULL: 0.5, 1, 2, 4).
 * All arithmetic is float32 with every operation rounded and no FMA: d2 = (dx*dx + dy*dy) + dz*dz, d its correctly rounded root;
 * d_true < cutoff is decided as d2 < fcz_lddt_c2(cutoff), which is the same. A row is inside its chain by fcz_lddt_dev's rules. A
 * slot (row, a) is PRESENT when mask_true and mask_pred are set at a and the six coordinates at a are finite.
 *   1. renaming   Row r inside its chain is AMBIGUOUS when some slot a has partner(a) != a under its type, and DECIDABLE when every
 *                 such slot is present. Its ANCHORS are the present slots (j, b) of the rows j != r of its chain where b has no
 *                 partner under row j's type. Under naming v = 0 the true coordinate of (r, a) is true[r][a], under v = 1 it is
 *                 true[r][partner(a)]; the prediction is pred[r][a] under both. P_v = the (ambiguous slot a of r, anchor) pairs
 *                 with d_true_v < cutoff, H_v = the sum over those pairs and the four thresholds t of
 *                 [|d_true_v - d_pred| < thresholds[t]], d_pred between pred[r][a] and the anchor's prediction.
 *                 swapped[r] = 1 exactly when (uint64)H_1 * P_0 > (uint64)H_0 * P_1: naming 1 has the strictly larger H / P, compared
 *                 without a division. 0 otherwise, for rows that are not decidable, and everywhere when aatype is NULL.
 *   2. score      The RENAMED TRUTH reads pos_true and mask_true of row r at partner(a) where swapped[r], at a elsewhere. An ATOM
 *                 is a slot (row, a) of a row inside its chain whose renamed-true mask and pred mask are set and whose six
 *                 coordinates are finite. For atoms i, j of DIFFERENT rows of one chain: j is a pair of i when d_true'(i, j) <
 *                 cutoff; a pair scores one hit per threshold that |d_true' - d_pred| lies under (one rounded subtraction; a NaN
 *                 or +inf difference is a pair with no hit).
 *   score [rows] float32      (float)hits / (float)(4 * pairs), a single rounded division; 0.0 where pairs == 0
 *   pairs [rows] int32, hits [rows] int32     the sums over the row's atoms
 *   swapped [rows] uint8
 *   atom_pairs, atom_hits [rows][A] int32     optional (NULL: not wanted): the two counts of the atom at the PREDICTION's slot, 0
 *                                             where the slot holds no atom
 * rows = n * L (padded) or R (packed). Rows that are not inside a chain, rows behind length and packed rows no chain covers hold 0
 * everywhere. Every element of every wanted output is written whatever the inputs hold, nothing outside them is written, and
 * nothing outside the inputs is read, whatever row_off or aatype holds (ranges that overlap are each computed and a shared row's
 * values are then unspecified). Every index that scales with rows * A is 64-bit. All counters are integers, so no order of
 * evaluation changes a result: reproducible bit for bit, the same for the same atoms in atom37 and atom14, NOT differentiable.
 * A row's hits, at most 4 * A * A * (rows of the chain), must fit int32: fcz_lddt_atoms_max_rows(layout) (pure host) is
 * floor((2^31 - 1) / (4 * A * A)), -1 for an unknown layout. A chain's candidates are staged in passes of at most
 * fcz_lddt_atoms_pass() (pure host, > 0): a chain with more takes several, with the same result. The work is two sweeps in stream
 * order, the renaming of every row of a chain before the score of any. Enqueued on the ctx stream, no synchronisation (the packed
 * forms share fcz_knn_packed_dev's scratch in the ctx). FCZ_E_INVALID_ARG with nothing launched: NULL ctx / pos_true / mask_true /
 * pos_pred / out / score / pairs / hits / swapped, NULL row_off with n > 0, unknown layout, L == 0, a cutoff that is not finite and
 * > 0, a threshold that is NaN, L (padded) or R (packed) above fcz_lddt_atoms_max_rows(layout), a swap_table with an entry >= A or
 * a row that is no involution. n == 0 or R == 0: FCZ_OK (packed, n == 0 < R: every row is uncovered and is filled). The time goes
 * to a group of its own, "lddt_atoms", for both forms. */
typedef struct fcz_lddt_atoms_out {
    float*   score;             /* [rows] */
    int32_t* pairs;             /* [rows] */
    int32_t* hits;              /* [rows] */
    uint8_t* swapped;           /* [rows] */
    int32_t* atom_pairs;        /* [rows][A] optional */
    int32_t* atom_hits;         /* [rows][A] optional */
} fcz_lddt_atoms_out;
int fcz_lddt_atoms_pass(void);
int fcz_lddt_atoms_max_rows(int layout);
/* pure host: out [21][A] uint8, the default swap_table; FCZ_E_INVALID_ARG for an unknown layout or a NULL out */
int fcz_lddt_default_swaps(int layout, uint8_t* out);
int fcz_lddt_atoms_dev(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev,
                       const uint8_t* mask_pred_dev, const uint8_t* aatype_dev, const uint32_t* length_dev, uint32_t n, uint32_t L,
                       int layout, float cutoff, const float* thresholds, const uint8_t* swap_table /* host, or NULL */,
                       const fcz_lddt_atoms_out* out_dev);
int fcz_lddt_atoms_packed_dev(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev,
                              const uint8_t* mask_pred_dev, const uint8_t* aatype_dev, const uint32_t* row_off_dev, uint32_t n,
                              uint32_t R, int layout, float cutoff, const float* thresholds,
                              const uint8_t* swap_table /* host, or NULL */, const fcz_lddt_atoms_out* out_dev);
/* Host-pointer conveniences: the same arrays on the host, staged through the ctx like fcz_lddt; synchronous. */
int fcz_lddt_atoms(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, const uint8_t* mask_pred,
                   const uint8_t* aatype, const uint32_t* length, uint32_t n, uint32_t L, int layout, float cutoff,
                   const float* thresholds, const uint8_t* swap_table, const fcz_lddt_atoms_out* out);
int fcz_lddt_atoms_packed(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred,
                          const uint8_t* mask_pred, const uint8_t* aatype, const uint32_t* row_off, uint32_t n, uint32_t R, int layout,
                          float cutoff, const float* thresholds, const uint8_t* swap_table, const fcz_lddt_atoms_out* out);

/* ---- backbone hydrogen bonds and DSSP secondary structure of the dense tensors ------------------------------ */
/* The per-residue secondary structure of Kabsch & Sander (1983) and the backbone hydrogen bonds it rests on, for a whole batch on
 * the device without an L x L array. The reference has no such output: like fcz_knn_dev these stand beside Foldcomp::decompress
 * (src/foldcomp.cpp:779) and read what the dense calls wrote, or any tensors of those shapes. Padded: pos [n][L][A][3] float32, mask
 * [n][L][A] uint8, aatype [n][L] uint8 or NULL (no row is proline), length [n] uint32 (may be NULL). Packed: pos [R][A][3], mask
 * [R][A], aatype [R] or NULL, row_off [n + 1] uint32. A = fcz_dense_width(layout); only N, CA, C, O are read: slots 0, 1, 2, 4 in
 * atom37 and 0, 1, 2, 3 in atom14 and backbone4, so the three layouts give the same bits. All arithmetic is float32 with every
 * operation rounded, no FMA; d2 = (dx*dx + dy*dy) + dz*dz and d = the correctly rounded float32 root of d2 (fcz_knn_dev's d2);
 * a / b is the correctly rounded float32 quotient.
 *   backbone row  row r lies inside its chain (fcz_knn_dev's rules for length / row_off), its mask is set at N, CA, C and O and
 *                 those twelve coordinates are finite. Nothing else is read as data.
 *   break         there is a break behind row r when r or r + 1 is no backbone row of the chain or d(C[r], N[r+1]) > 2.5f.
 *                 "No break in a .. b" (a <= b rows of the chain): no break behind any of a .. b - 1.
 *   amide H       row r has one when r and r - 1 are backbone rows of the chain, there is no break behind r - 1, aatype[r] != 14
 *                 (proline) and d(C[r-1], O[r-1]) != 0: H = N[r] + (C[r-1] - O[r-1]) / d(C[r-1], O[r-1]), per component one
 *                 subtraction, one division, one addition.
 *   energy        of donor i (a row with H) and acceptor j (a backbone row of the same chain, j != i, j != i - 1) with
 *                 d2(CA[i], CA[j]) < 81.0f: with dON = d(O[j], N[i]), dCH = d(C[j], H[i]), dOH = d(O[j], H[i]), dCN = d(C[j], N[i]),
 *                 E = -9.9f when any of the four is < 0.5f, else E = 27.888f * (((1/dON + 1/dCH) - 1/dOH) - 1/dCN), raised to -9.9f
 *                 when below it. The energy COUNTS when E < 0 (a NaN does not); a HYDROGEN BOND is E < -0.5f. DSSP's rounding of
 *                 E to 0.001 is not done.
 *   tables        acc_index [rows][2] int32, acc_energy [rows][2] float32: the two acceptors of the row's N-H whose energies count,
 *                 ordered by (E, row) ascending; don_index, don_energy: the two donors onto the row's C=O, alike. The order is
 *                 total, so the tables do not depend on any order of evaluation. An index is the row inside the entry (padded,
 *                 0 .. L - 1) or the global row (packed), as fcz_knn_dev's; an empty slot holds -1 / 0.0f.
 *   bond(d, a)    a is one of the two entries of acc_index[d] and its acc_energy < -0.5f. The labels use bond() only.
 *   turn_n(i)     n = 3, 4, 5: bond(i + n, i) and no break in i .. i + n.
 *   H             turn_4(i - 1) and turn_4(i) make rows i .. i + 3 H.
 *   bridge (i, j) i >= 1, j >= i + 3, rows i - 1, i + 1, j - 1, j + 1 inside the chain, no break in i - 1 .. i + 1 nor in
 *                 j - 1 .. j + 1; PARALLEL when (bond(i+1, j) and bond(j, i-1)) or (bond(j+1, i) and bond(i, j-1)), ANTIPARALLEL
 *                 when (bond(i+1, j-1) and bond(j+1, i-1)) or (bond(j, i) and bond(i, j)). The two kinds are kept apart: a pair
 *                 may be a bridge of both.
 *   ladder        a maximal run of bridges of one kind: (i, j), (i+1, j+1), .. parallel; (i, j), (i+1, j-1), .. antiparallel.
 *   bulge link    ladders X, Y of one kind, gi = ib(Y) - ie(X), gj = jb(Y) - je(X) (parallel) or je(X) - jb(Y) (antiparallel), with
 *                 (ie, je) the last bridge of X and (ib, jb) the first of Y: 0 < gi < 6, 0 < gj < 6, gi < 3 or gj < 3, no break in
 *                 ie .. ib and none between je and jb.
 *   E             every row of a ladder of two or more bridges, every row of a bulge-linked ladder, and the rows ie .. ib and
 *                 between je and jb of a link. B: the rows of a ladder of one bridge that is not linked. A row that is both is E.
 *                 Neither overwrites H.
 *   G             turn_3(i - 1) and turn_3(i) with none of rows i .. i + 2 labelled H, B or E make those rows G.
 *   I             turn_5(i - 1) and turn_5(i) with none of rows i .. i + 4 labelled H, B, E or G make those rows I.
 *   T             a row still unlabelled with turn_n(r - k) for some n and 1 <= k < n.
 *   S             a row still unlabelled, no break in r - 2 .. r + 2, and dot < 0.34202015f * (|u| * |v|) for u = CA[r] - CA[r-2],
 *                 v = CA[r+2] - CA[r], dot = (ux*vx + uy*vy) + uz*vz, |u| = sqrt((ux*ux + uy*uy) + uz*uz): a bend above 70 degrees.
 *   ss [rows] uint8       0 .. 7 in the order "-HBEGITS" (the 1983 priority H > B, E > G > I > T > S); 0 on every row that is
 *                         no backbone row
 *   ss_mask [rows] uint8  1 on backbone rows, else 0
 * rows = n * L (padded) or R (packed). Rows behind length and packed rows no chain covers hold -1 / 0.0f, ss 0 and ss_mask 0. Every
 * byte of the outputs is written whatever the inputs hold, nothing outside them is written, and nothing outside the inputs is read,
 * whatever row_off or a given acceptor table holds (an index of the table is compared, or checked against the chain's range before
 * a row is read through it; ranges that overlap are each computed and a shared row's values are then unspecified). Every index that
 * scales with rows * A is 64-bit.
 * fcz_hbond_dev writes the four tables. Candidates are staged per chain in passes of fcz_hbond_pass() rows (pure host, > 0): a
 * longer chain takes several, with the same result. fcz_dssp_labels_dev reads pos, mask and the two ACCEPTOR tables (any tables of
 * that shape, not only ones fcz_hbond_dev wrote; aatype is accepted and not read) and writes ss and ss_mask; it recomputes no energy.
 * Enqueued on the ctx stream, no synchronisation (the packed forms share fcz_knn_packed_dev's scratch in the ctx; the label calls
 * keep a byte per row of scratch there). FCZ_E_INVALID_ARG with nothing launched: NULL ctx / pos / mask / any table or output, NULL
 * row_off with n > 0, unknown layout, L == 0, L (padded) or R (packed) above 2^31 - 1 (the indices are int32). n == 0 or R == 0:
 * FCZ_OK (packed, n == 0 < R: every row is uncovered and is filled). The time goes to a group of its own, "dssp", for all the calls
 * of this block. The results are integers and selected energies: reproducible bit for bit, NOT differentiable. */
int fcz_hbond_pass(void);
int fcz_hbond_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint8_t* aatype_dev, const uint32_t* length_dev,
                  uint32_t n, uint32_t L, int layout, int32_t* acc_index_dev, float* acc_energy_dev, int32_t* don_index_dev,
                  float* don_energy_dev);
int fcz_hbond_packed_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint8_t* aatype_dev,
                         const uint32_t* row_off_dev, uint32_t n, uint32_t R, int layout, int32_t* acc_index_dev, float* acc_energy_dev,
                         int32_t* don_index_dev, float* don_energy_dev);
int fcz_dssp_labels_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint8_t* aatype_dev,
                        const uint32_t* length_dev, uint32_t n, uint32_t L, int layout, const int32_t* acc_index_dev,
                        const float* acc_energy_dev, uint8_t* ss_dev, uint8_t* ss_mask_dev);
int fcz_dssp_labels_packed_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint8_t* aatype_dev,
                               const uint32_t* row_off_dev, uint32_t n, uint32_t R, int layout, const int32_t* acc_index_dev,
                               const float* acc_energy_dev, uint8_t* ss_dev, uint8_t* ss_mask_dev);
/* Host-pointer conveniences: the same arrays on the host, staged through the ctx like fcz_lddt, both steps; synchronous. */
int fcz_dssp(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint8_t* aatype, const uint32_t* length, uint32_t n, uint32_t L,
             int layout, int32_t* acc_index, float* acc_energy, int32_t* don_index, float* don_energy, uint8_t* ss, uint8_t* ss_mask);
int fcz_dssp_packed(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint8_t* aatype, const uint32_t* row_off, uint32_t n,
                    uint32_t R, int layout, int32_t* acc_index, float* acc_energy, int32_t* don_index, float* don_energy, uint8_t* ss,
                    uint8_t* ss_mask);

/* ---- per-residue solvent accessibility of the dense tensors ------------------------------------------------ */
/* The Shrake-Rupley accessible surface of every chain of a dense batch, for a whole batch on the device, without a rows x rows or an
 * atoms x atoms array. The reference has no such output: like fcz_hbond_dev these stand beside Foldcomp::decompress
 * (src/foldcomp.cpp:779) and read what the dense calls wrote, or any tensors of those shapes. Padded: pos [n][L][A][3] float32, mask
 * [n][L][A] uint8, aatype [n][L] uint8 or NULL, length [n] uint32 (may be NULL). Packed: pos [R][A][3], mask [R][A], aatype [R] or
 * NULL, row_off [n + 1] uint32. A = fcz_dense_width(layout); every slot is read. All arithmetic is float32 with every operation
 * rounded, no FMA; d2(p, q) = (dx*dx + dy*dy) + dz*dz (fcz_knn_dev's d2).
 *   atom          a slot (row, a) of a row inside its chain (fcz_hbond_dev's rules for length / row_off) whose mask is non-zero,
 *                 whose three coordinates are finite and whose radius is non-zero. Only atoms of the same chain bury each other;
 *                 a slot that is no atom has 0 points, 0 area and buries nothing. Nothing else is read as data.
 *   radius        radius_table[21][A] float32, a HOST table indexed [aatype][slot]; aatype is what fcz_dense_dev writes, 0 .. 20,
 *                 and a value above 20 uses row 20. aatype_dev == NULL: every row uses row 0. The table goes to the kernel by
 *                 value. NULL selects the default, fcz_sasa_default_radii(layout, ..): the Bondi radius of the element (the first
 *                 letter of the atom's name: C 1.70, N 1.55, O 1.52, S 1.80) of the atom that fcz_dense_slot puts into the slot. In
 *                 atom14 that depends on the type: row t < 20 holds the atoms of residue code t, row 20 those of the backbone-only
 *                 codes (N, CA, C), and a slot the type does not own holds 0. In atom37 and backbone4 a slot holds the same atom in
 *                 every type that has it, so all 21 rows are the same (the mask says which atoms a residue has) and a NULL aatype
 *                 is harmless; in atom14 a NULL aatype is refused. OXT (slot 36 of atom37) is in no residue's table and holds 0, so
 *                 atom37 and atom14 describe the same atoms.
 *   R             R = radius + probe (one float32 addition). The host refuses a call when R is outside [0.5, 8) for some entry of
 *                 the table whose radius is non-zero.
 *   points        points_dev [P][3] float32, 1 <= P <= 1024: the directions u_k, used as given (the library generates none and
 *                 does not normalise them, so no transcendental function enters the contract). Point k of atom i is
 *                 t_k = c_i + Ri * u_k, per component one multiplication and one addition.
 *   candidate     atom j is a candidate of atom i when (row, slot) of j differs from that of i and d2(c_i, c_j) < S * S with
 *                 S = Ri + Rj. The cull is part of the definition, so that coordinates like 3e19 or duplicated atoms cannot make
 *                 two evaluations disagree; geometrically it changes nothing (a sphere further away cannot reach a point).
 *   buried        point k of atom i is buried when some candidate j has d2(t_k, c_j) < Rj * Rj.
 *   sasa_points [rows][A] int16   the points of the slot's atom that are not buried, 0 .. P: an integer that does not depend on
 *                                 the order the candidates are met in
 *   sasa [rows] float32           (float)(sum_a (double)sasa_points[row][a] * (double)(Ra * Ra) * (4 pi / P)): the sum in float64
 *                                 over the row's atoms with Ra * Ra the float32 product, then ONE double multiplication by
 *                                 0x1.921fb54442d18p+3 / P and one rounding to float32; in square Angstrom when the inputs are
 *                                 in Angstrom. Every term is an integer of at most 11 bits times a float32 in [0.25, 64) and at
 *                                 most 37 terms are summed, so the float64 sum is EXACT: the result does not depend on the order
 *                                 of the slots, and atom37 and atom14 give the same bits for the same atoms.
 *   sasa_mask [rows] uint8        1 when the row has at least one atom, else 0
 * rows = n * L (padded) or R (packed). Rows behind length and packed rows no chain covers hold 0 everywhere. Every byte of the
 * outputs is written whatever the inputs hold, nothing outside them is written, and nothing outside the inputs is read, whatever
 * row_off or aatype holds (ranges that overlap are each computed and a shared row's values are then unspecified). Every index that
 * scales with rows * A is 64-bit. A chain's atoms are staged in passes of at most fcz_sasa_pass() (pure host, > 0): a chain with
 * more takes several, with the same result.
 * Enqueued on the ctx stream, no synchronisation (the packed forms share fcz_knn_packed_dev's scratch in the ctx).
 * FCZ_E_INVALID_ARG with nothing launched: NULL ctx / pos / mask / points / any output, NULL row_off with n > 0, unknown layout,
 * L == 0, L (padded) or R (packed) above 2^31 - 1, n_points outside 1 .. 1024, probe not finite or negative, the rule on R above,
 * atom14 without aatype. n == 0 or R == 0: FCZ_OK (packed, n == 0 < R: every row is uncovered and is filled). The time goes to a
 * group of its own, "sasa". The results are counts and sums of counts: reproducible bit for bit, NOT differentiable. */
int fcz_sasa_pass(void);
/* out [21][A] float32 (host): the default radius table of the layout. Pure host. Unknown layout or NULL out: FCZ_E_INVALID_ARG. */
int fcz_sasa_default_radii(int layout, float* out);
int fcz_sasa_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint8_t* aatype_dev, const uint32_t* length_dev,
                 uint32_t n, uint32_t L, int layout, const float* radius_table /* host, or NULL */, float probe,
                 const float* points_dev, uint32_t n_points, int16_t* sasa_points_dev, float* sasa_dev, uint8_t* sasa_mask_dev);
int fcz_sasa_packed_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint8_t* aatype_dev,
                        const uint32_t* row_off_dev, uint32_t n, uint32_t R, int layout, const float* radius_table /* host, or NULL */,
                        float probe, const float* points_dev, uint32_t n_points, int16_t* sasa_points_dev, float* sasa_dev,
                        uint8_t* sasa_mask_dev);
/* Host-pointer conveniences: the same arrays on the host (points too), staged through the ctx like fcz_dssp; synchronous. */
int fcz_sasa(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint8_t* aatype, const uint32_t* length, uint32_t n, uint32_t L,
             int layout, const float* radius_table, float probe, const float* points, uint32_t n_points, int16_t* sasa_points,
             float* sasa, uint8_t* sasa_mask);
int fcz_sasa_packed(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint8_t* aatype, const uint32_t* row_off, uint32_t n,
                    uint32_t R, int layout, const float* radius_table, float probe, const float* points, uint32_t n_points,
                    int16_t* sasa_points, float* sasa, uint8_t* sasa_mask);

/* ---- steric clashes and peptide-link violations of the dense tensors ------------------------------------- */
/* Is the structure physically possible: do atoms of different residues sit inside each other, and is the chain still connected? The
 * two between-residue terms of AlphaFold's "structural violations", for a whole batch on the device, without a rows x rows or an
 * atoms x atoms array. The reference has no such output: like fcz_sasa_dev these stand beside Foldcomp::decompress
 * (src/foldcomp.cpp:779) and read what the dense calls wrote, or any tensors of those shapes. The inputs are fcz_sasa_dev's: padded
 * pos [n][L][A][3] float32, mask [n][L][A] uint8, aatype [n][L] uint8 or NULL, length [n] uint32 (may be NULL); packed pos [R][A][3],
 * mask [R][A], aatype [R] or NULL, row_off [n + 1] uint32. A = fcz_dense_width(layout); every slot is read. All arithmetic is float32
 * with every operation rounded, no FMA; d2(p, q) = (dx*dx + dy*dy) + dz*dz (fcz_knn_dev's d2); sqrt is the correctly rounded one.
 *   atom          exactly fcz_sasa_dev's atom with probe 0: a slot (row, a) of a row inside its chain whose mask is non-zero, whose
 *                 three coordinates are finite and whose radius R = radius_table[min(aatype, 20)][a] is non-zero. radius_table is
 *                 fcz_sasa_dev's HOST table [21][A], NULL for fcz_sasa_default_radii(layout, ..) (Bondi; OXT holds 0 and is left
 *                 out, so atom37 and atom14 describe the same atoms); aatype NULL: every row uses row 0 (refused in atom14). Only
 *                 atoms of the same chain are compared. Nothing else is read as data.
 *   clash         atoms i and j of DIFFERENT ROWS clash when T = (Ri + Rj) - tolerance (one addition, one subtraction) is > 0 and
 *                 d2(c_i, c_j) < T * T. Ri + Rj commutes and d2(p, q) == d2(q, p) bit for bit, so the predicate is SYMMETRIC in
 *                 float32: j clashes with i whenever i clashes with j. d2 = +inf (coordinates like 3e19) or NaN is no clash. Two
 *                 kinds of pair never clash: the peptide bond, C of row r with N of row r + 1 of the same chain, and the
 *                 disulfide, SG with SG when both rows have aatype == 4 (CYS). N and C are the slots fcz_dense_slot(layout, 0, ..)
 *                 gives them, SG the slot fcz_dense_slot(layout, 4, SG) gives; in backbone4, or with a NULL aatype, the disulfide
 *                 exclusion never applies. The kernel uses NO cull: every pair of atoms of a chain is put to this test.
 *   clash_atom [rows][A] uint8    1 when the slot's atom clashes with some atom, else 0
 *   clash_count [rows] int32      the (atom of this row, atom of another row) clashing pairs; every pair is therefore counted once
 *                                 from each side, and the sum over a chain is even (modulo 2^32 for a row with more)
 *   clash_depth [rows] float32    the largest T - sqrt(d2) (one subtraction) over those pairs, 0 when none. It is >= 0 (sqrt is
 *                                 monotone and sqrt(T * T) == T) and a maximum, so no order of evaluation changes it
 *   clash_partner [rows] int32    the CHAIN-RELATIVE row of the other atom of the pair behind clash_depth; of equal depths the
 *                                 smallest row; -1 when none
 *   viol_mask [rows] uint8        1 when the row has at least one atom, else 0
 *   link          between rows r and r + 1 of a chain, stored at row r; the chain's last row has none. It exists when CA and C of r
 *                 and N and CA of r + 1 are set in the mask and finite; the radius table plays no part here.
 *   link_mask [rows] uint8        1 when the link exists. Where it does not, the three fields below are 0.
 *   link_length [rows] float32    sqrt(d2(C, N'))
 *   link_cos [rows][2] float32    the cosines of the angles CA-C-N' and C-N'-CA'. The angle at b between a and c: u = a - b,
 *                                 v = c - b, dot = (ux*vx + uy*vy) + uz*vz, |u| = sqrt((ux*ux + uy*uy) + uz*uz), |v| alike, and
 *                                 cos = dot / (|u| * |v|): one multiplication, one division. A zero norm gives what IEEE gives
 *                                 (NaN or +-inf); NaN compares false below, so it is no violation
 *   link_violation [rows] uint8   bit 0: |link_length - l0| > link_factor * sl, with (l0, sl) = (1.341, 0.016) when row r + 1 has
 *                                 aatype == 14 (PRO; never with a NULL aatype), else (1.329, 0.014);
 *                                 bit 1: |cos0 - (-0.4473)| > link_factor * 0.0311; bit 2: |cos1 - (-0.5203)| > link_factor * 0.0353.
 *                                 Each constant is the float32 nearest to the decimal, each product link_factor * s one float32
 *                                 multiplication, each difference one subtraction. The constants are the Engh & Huber peptide
 *                                 geometry that AlphaFold's violation terms use: defaults of this definition, not measurements.
 *   chain_counts [n][4] int64     per chain: its atoms; its clashing pairs, each ONCE (the pairs counted from the side with the
 *                                 smaller row, which by the symmetry is exactly half the sum of the chain's clash_count); its rows
 *                                 with bit 0; its rows with bit 1 or bit 2. Integer sums: no order changes them.
 * rows = n * L (padded) or R (packed). Rows behind length and packed rows no chain covers hold 0 everywhere (-1 in clash_partner).
 * Every byte of the outputs is written whatever the inputs hold, nothing outside them is written, and nothing outside the inputs is
 * read, whatever row_off or aatype holds (ranges that overlap are each computed and a shared row's values are then unspecified).
 * Every index that scales with rows * A is 64-bit. A chain's atoms are staged in passes of at most fcz_violations_pass() (pure host,
 * > 0): a chain with more takes several, with the same result. Within-residue bond and angle bounds, AlphaFold's third term, are
 * not computed. Every output needs the alignment of its type (chain_counts is added to with 64-bit atomics) and no more.
 * Enqueued on the ctx stream, no synchronisation (the packed forms share fcz_knn_packed_dev's scratch in the ctx).
 * FCZ_E_INVALID_ARG with nothing launched: NULL ctx / pos / mask / out / any of out's ten pointers, NULL row_off with n > 0, unknown
 * layout, L == 0, L (padded) or R (packed) above 2^31 - 1, tolerance or link_factor not finite or negative, a table with a non-zero
 * radius outside [0.5, 8), atom14 without aatype. n == 0 or R == 0: FCZ_OK (packed, n == 0 < R: every row is uncovered and is
 * filled). The time goes to a group of its own, "violations". The results are integers, maxima and values of single rows:
 * reproducible bit for bit, the same for the same atoms in atom37 and atom14, NOT differentiable. */
typedef struct fcz_violations_out {
    uint8_t* clash_atom;        /* [rows][A] */
    int32_t* clash_count;       /* [rows] */
    float*   clash_depth;       /* [rows] */
    int32_t* clash_partner;     /* [rows] */
    uint8_t* viol_mask;         /* [rows] */
    uint8_t* link_mask;         /* [rows] */
    float*   link_length;       /* [rows] */
    float*   link_cos;          /* [rows][2] */
    uint8_t* link_violation;    /* [rows] */
    int64_t* chain_counts;      /* [n][4] */
} fcz_violations_out;
int fcz_violations_pass(void);
int fcz_violations_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint8_t* aatype_dev, const uint32_t* length_dev,
                       uint32_t n, uint32_t L, int layout, const float* radius_table /* host, or NULL */, float tolerance,
                       float link_factor, const fcz_violations_out* out_dev);
int fcz_violations_packed_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint8_t* aatype_dev,
                              const uint32_t* row_off_dev, uint32_t n, uint32_t R, int layout,
                              const float* radius_table /* host, or NULL */, float tolerance, float link_factor,
                              const fcz_violations_out* out_dev);
/* Host-pointer conveniences: the same arrays on the host, staged through the ctx like fcz_sasa; synchronous. */
int fcz_violations(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint8_t* aatype, const uint32_t* length, uint32_t n,
                   uint32_t L, int layout, const float* radius_table, float tolerance, float link_factor, const fcz_violations_out* out);
int fcz_violations_packed(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint8_t* aatype, const uint32_t* row_off,
                          uint32_t n, uint32_t R, int layout, const float* radius_table, float tolerance, float link_factor,
                          const fcz_violations_out* out);

/* ---- the violation loss: clashes and peptide links as a differentiable loss, and its gradient ------------- */
/* The two between-residue terms of AlphaFold's structural-violation loss (between_residue_clash_loss and
 * between_residue_bond_loss) on the geometry of fcz_violations_dev, as float32 values with a fused backward on the device: no atoms x
 * atoms array in either direction. The reference has no such output. Inputs, forms (padded, packed; atom37, atom14, backbone4),
 * chains, ATOMS, radii (radius_table on the host or NULL for Bondi; aatype may be NULL, except in atom14), exclusions and arithmetic
 * rules are fcz_violations_dev's, unchanged: float32 throughout, every operation rounded, no FMA,
 * d2(p, q) = (dx*dx + dy*dy) + dz*dz with dx = p.x - q.x, the correctly rounded sqrt and division.
 *   clash pairs   fcz_violations_dev's pairs exactly: atoms i, j of different rows of a chain with T = (Ri + Rj) - tolerance > 0 and
 *                 d2(c_i, c_j) < T * T, the peptide bond and the CYS-CYS SG pairs struck out. The relation is symmetric.
 * Value (fcz_violation_loss_dev):
 *   clash_loss [rows][A] float32  for atom i the float32 sum of T_ij - sqrt(d2_ij) (one subtraction; >= 0) over its clashing partners
 *                                 j, added one after the other from 0 in ASCENDING (chain row of j, slot of j); 0 for a slot that is
 *                                 no atom. Every pair stands in both of its atoms: AlphaFold's per_atom_loss_sum.
 *   link_loss [rows][3] float32   at row r for the link r -> r + 1 where fcz_violations_dev's link exists (link_mask), else 0; with
 *                                 x+ = x when x > 0, else 0:   (|length - l0| - link_factor * sl)+,
 *                                 (|cos0 - (-0.4473)| - link_factor * 0.0311)+,   (|cos1 - (-0.5203)| - link_factor * 0.0353)+
 *                                 with length, cos0, cos1, (l0, sl), the PRO case and every operation as link_length, link_cos and
 *                                 link_violation have them; |x - x0| - bound is one more subtraction. A term whose length or cosine
 *                                 is not finite is 0: the loss stays finite where the metric sets a bit for +-inf. So
 *                                 link_loss[r][k] > 0 exactly where bit k of link_violation[r] is set and the quantity is finite.
 *   counts [n][2] int64           per chain its atoms (chain_counts[.][0]) and its links: integer atomics, cleared by the call.
 * Gradient (fcz_violation_loss_grad_dev) of  sum w_clash * clash_loss + sum w_link * link_loss  with respect to pos, for the caller's
 * w_clash [rows][A] and w_link [rows][3] float32, the upstream gradients of the two outputs; the weight of a slot that is no atom and
 * of a link that does not exist is not read as data. grad [rows][A][3] float32, per slot, every component x alike:
 *   1. from 0, over the atom's clashing partners j in the same ascending order:  g = g + (w_i + w_j) * (-((p_i.x - p_j.x) / d)),
 *      d = sqrt(d2): one addition of the weights, one subtraction, one division, an exact negation, one multiplication, one
 *      addition. A pair with d == 0 adds nothing (no direction), and a pair with T - d == 0 adds nothing (the subgradient 0 of
 *      x+ at 0, as torch's relu has it). A slot that is no atom starts from 0 and has no partners.
 *   2. then the link terms, added one after the other: row r's N receives the bond, cos0 and cos1 terms of link r - 1, its CA the cos1
 *      term of link r - 1 and then the cos0 term of link r, its C the bond, cos0 and cos1 terms of link r. Link atoms are defined by
 *      mask and finiteness alone: a slot with a zero radius receives its link terms all the same. Only a term whose link_loss is > 0
 *      (strictly positive, hence finite) contributes; every other term is 0. With k = w_link[r][t] * sign(x - x0) (that is w, -w, or
 *      0 for a difference of 0):
 *        bond   C:  k * ((C.x - N'.x) / length);  N': the exact negation of C's term. A length of 0 gives 0.
 *        cos    of the angle at b between a and c (cos0: CA, C, N'; cos1: C, N', CA'), u = a - b, v = c - b, |u|, |v| and cos as
 *               link_cos has them:  uh = u.x / |u|, vh = v.x / |v|,  ga = (vh - cos * uh) / |u|,  gc = (uh - cos * vh) / |v|,
 *               gb = -(ga + gc);  a receives k * ga, b receives k * gb, c receives k * gc (one multiplication each).
 * Every slot gathers its whole gradient itself: no float atomics, no scatter, one writer a slot. With every operation spelled out,
 * numpy reproduces value and gradient bit for bit.
 * rows = n * L (padded) or R (packed). Every byte of every output is written whatever the inputs hold and nothing outside the outputs
 * is written; rows behind length and packed rows no chain covers hold 0; nothing outside the inputs is read, whatever row_off or
 * aatype holds (ranges that overlap are each computed and a shared row's values are then unspecified). Every index that scales with
 * rows * A is 64-bit. A chain's atoms are staged in passes of at most fcz_violation_loss_pass() (pure host, > 0). The result does
 * not depend on tile, pass, launch geometry or the other chains of the batch: a chain gives the same bytes alone, in any batch,
 * padded or packed, call after call. Bit agreement between atom37 and atom14 is NOT promised: the slot order inside a row differs,
 * and with it the order of a float32 sum. Within-residue bounds are not computed, and there are no second derivatives.
 * Enqueued on the ctx stream, no synchronisation (the packed forms share fcz_knn_packed_dev's scratch in the ctx).
 * FCZ_E_INVALID_ARG with nothing launched and no output touched: everything fcz_violations_dev refuses (NULL ctx / pos / mask, NULL
 * row_off with n > 0, unknown layout, L == 0, L or R above 2^31 - 1, tolerance or link_factor not finite or negative, a table with a
 * non-zero radius outside [0.5, 8), atom14 without aatype), a NULL output or weight pointer. n == 0 or R == 0: FCZ_OK (packed,
 * n == 0 < R: every row is uncovered and is filled). The time goes to the groups "violation_loss" and "violation_loss_grad". */
int fcz_violation_loss_pass(void);
int fcz_violation_loss_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint8_t* aatype_dev,
                           const uint32_t* length_dev, uint32_t n, uint32_t L, int layout, const float* radius_table /* host, or NULL */,
                           float tolerance, float link_factor, float* clash_loss_dev, float* link_loss_dev, int64_t* counts_dev);
int fcz_violation_loss_packed_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint8_t* aatype_dev,
                                  const uint32_t* row_off_dev, uint32_t n, uint32_t R, int layout,
                                  const float* radius_table /* host, or NULL */, float tolerance, float link_factor,
                                  float* clash_loss_dev, float* link_loss_dev, int64_t* counts_dev);
int fcz_violation_loss_grad_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint8_t* aatype_dev,
                                const uint32_t* length_dev, uint32_t n, uint32_t L, int layout,
                                const float* radius_table /* host, or NULL */, float tolerance, float link_factor,
                                const float* w_clash_dev, const float* w_link_dev, float* grad_dev);
int fcz_violation_loss_grad_packed_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint8_t* aatype_dev,
                                       const uint32_t* row_off_dev, uint32_t n, uint32_t R, int layout,
                                       const float* radius_table /* host, or NULL */, float tolerance, float link_factor,
                                       const float* w_clash_dev, const float* w_link_dev, float* grad_dev);
/* Host-pointer conveniences: the same arrays on the host, staged through the ctx like fcz_violations; synchronous. */
int fcz_violation_loss(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint8_t* aatype, const uint32_t* length, uint32_t n,
                       uint32_t L, int layout, const float* radius_table, float tolerance, float link_factor, float* clash_loss,
                       float* link_loss, int64_t* counts);
int fcz_violation_loss_packed(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint8_t* aatype, const uint32_t* row_off,
                              uint32_t n, uint32_t R, int layout, const float* radius_table, float tolerance, float link_factor,
                              float* clash_loss, float* link_loss, int64_t* counts);
int fcz_violation_loss_grad(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint8_t* aatype, const uint32_t* length,
                            uint32_t n, uint32_t L, int layout, const float* radius_table, float tolerance, float link_factor,
                            const float* w_clash, const float* w_link, float* grad);
int fcz_violation_loss_grad_packed(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint8_t* aatype, const uint32_t* row_off,
                                   uint32_t n, uint32_t R, int layout, const float* radius_table, float tolerance, float link_factor,
                                   const float* w_clash, const float* w_link, float* grad);

/* ---- least-squares (Kabsch) superposition of two dense tensor batches ------------------------------------ */
/* The superposition-based half of what a validation loop logs, per chain, for a whole batch on the device: the rigid motion that
 * lays the prediction onto the target, the RMSD after it, the GDT counts, a TM-score at that superposition, every site's
 * deviation, and (fcz_superpose_apply_dev) the prediction moved onto the target. The reference has no such output (its `rmsd` is
 * the unsuperposed sum over two files): like fcz_lddt_dev these stand beside Foldcomp::decompress (src/foldcomp.cpp:779). The inputs
 * are fcz_lddt_dev's: two tensors of ONE shape and layout, pos_true / mask_true and pos_pred / mask_pred (mask_pred may be NULL:
 * every slot present), padded with length [n] (may be NULL) or packed with row_off [n + 1], a layout and a slot. A row is a SITE by
 * exactly fcz_lddt_dev's rule (inside its chain, both masks set at the slot, six finite coordinates); nothing else is read as data.
 * For chain e with S sites a_i (pred) and b_i (true), all in float64, every operation rounded, no FMA:
 *   centroids   ca, cb = the sums over the sites divided by S (the centroid first, the centring second)
 *   M           sum (a_i - ca)(b_i - cb)^T, centred
 *   R           the proper rotation (det = +1) that minimises sum |R (a_i - ca) - (b_i - cb)|^2: the unit eigenvector of the largest
 *               eigenvalue of Horn's symmetric 4 x 4 quaternion matrix of M (Horn 1987), found by cyclic Jacobi sweeps from the
 *               identity; of equal largest eigenvalues the first. A quaternion always gives a proper rotation: there is no
 *               determinant fix-up. t = cb - R ca.
 *   dev_i       |R a_i + t - b_i|, with x' = ((r00 x + r01 y) + r02 z) + tx and d2 = (dx dx + dy dy) + dz dz, from the float64 R, t
 * Per chain, float32 unless stated, each value rounded once from float64:
 *   rot [n][3][3], trans [n][3]   R and t: x_true ~ rot @ x_pred + trans, the convention of fcz_frames_dev
 *   rmsd [n]                      sqrt(sum dev^2 / S)
 *   sites [n] int32               S
 *   gdt_counts [n][5] int32       the sites with dev <= 0.5, 1, 2, 4, 8 (compared in float64). GDT-TS is the mean of the fractions
 *                                 at 1, 2, 4, 8 and GDT-HA of those at 0.5, 1, 2, 4: integers over S, left to the caller
 *   tm [n]                        (1 / S) sum 1 / (1 + (dev_i / d0)^2), d0 = max(1.24 cbrt(S - 15) - 1.8, 0.5) for S > 15, else 0.5:
 *                                 the TM-score AT THE LEAST-SQUARES SUPERPOSITION, normalised by the sites. It is a lower bound of
 *                                 what TM-score programs report, which maximise the sum over superpositions.
 * Per row: dev [rows] float32, dev_i rounded once; 0 where the row is no site, lies behind length, or (packed) is covered by no chain.
 * rows = n * L (padded) or R (packed). Degenerate chains fall out of the solver: S = 0 gives the identity, trans 0 and every score 0;
 * S = 1 the identity rotation (Horn's matrix is zero and Jacobi leaves the identity), trans = b - a and rmsd 0; two sites or
 * collinear sites give A minimiser (it is not unique; rot is still a proper rotation and rmsd / dev are well defined).
 * Reproducibility: a sum over the sites has a fixed order -- lane l of the chain's 64-lane wavefront adds its rows l, l + 64, .. in
 * ascending order, then an xor-butterfly over the lanes (distances 32, 16, .. 1) -- so the result depends on neither the launch
 * geometry nor the form: two runs give the same bits, and padded against packed gives the same bits. Against another float64
 * implementation it agrees to rounding, not on bits. It is NOT differentiable.
 * All of rmsd, sites, gdt_counts, tm and dev may be NULL (not wanted); rot and trans are required. Every byte of the outputs given
 * is written whatever the inputs hold, nothing outside them is written, and nothing outside the inputs is read, whatever row_off
 * holds (ranges that overlap are each computed; which of them a shared row's dev belongs to is then unspecified). Every index that
 * scales with rows * A is 64-bit. Enqueued on the ctx stream, no synchronisation, no scratch. FCZ_E_INVALID_ARG with nothing
 * launched: NULL ctx / pos_true / mask_true / pos_pred / out / out->rot / out->trans, NULL row_off with n > 0, unknown layout, slot
 * outside the layout's width, L == 0, L (padded) or R (packed) above 2^31 - 1 (sites is int32). n == 0: FCZ_OK (packed, n == 0 < R:
 * every row is uncovered and dev is filled). The time goes to a group of its own, "superpose", for all the calls of this block. */
typedef struct fcz_superpose_out {
    float*   rot;           /* [n][3][3] */
    float*   trans;         /* [n][3] */
    float*   rmsd;          /* [n] optional */
    int32_t* sites;         /* [n] optional */
    int32_t* gdt_counts;    /* [n][5] optional */
    float*   tm;            /* [n] optional */
    float*   dev;           /* [n][L] / [R] optional */
} fcz_superpose_out;
int fcz_superpose_dev(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev,
                      const uint8_t* mask_pred_dev, const uint32_t* length_dev, uint32_t n, uint32_t L, int layout, int slot,
                      const fcz_superpose_out* out_dev);
int fcz_superpose_packed_dev(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev,
                             const uint8_t* mask_pred_dev, const uint32_t* row_off_dev, uint32_t n, uint32_t R, int layout, int slot,
                             const fcz_superpose_out* out_dev);
/* The transform applied to the WHOLE prediction: pos_out[row][a] = rot_e @ pos[row][a] + trans_e for every slot a whose mask is set
 * (mask NULL: every slot) in rows inside chain e, and 0 elsewhere (cleared slots, rows behind length, packed rows no chain covers):
 * every byte of pos_out, of the shape of pos, is written. It is computed in float32 from the float32 rot / trans in a stated order,
 * every operation rounded, no FMA: x' = ((r00 x + r01 y) + r02 z) + tx, and y', z' alike from rows 1 and 2, so a caller reproduces
 * it bit for bit from the transform. rot [n][3][3] and trans [n][3] may be any transforms, not only ones fcz_superpose_dev wrote.
 * pos and pos_out need no alignment beyond float's and must not overlap. Refusals and the n == 0 rule are those above (there is no
 * slot). Enqueued on the ctx stream (the packed form shares fcz_knn_packed_dev's scratch in the ctx). */
int fcz_superpose_apply_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint32_t* length_dev, uint32_t n,
                            uint32_t L, int layout, const float* rot_dev, const float* trans_dev, float* pos_out_dev);
int fcz_superpose_apply_packed_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint32_t* row_off_dev,
                                   uint32_t n, uint32_t R, int layout, const float* rot_dev, const float* trans_dev,
                                   float* pos_out_dev);
/* Host-pointer conveniences: the same arrays on the host, staged through the ctx like fcz_lddt; synchronous. */
int fcz_superpose(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, const uint8_t* mask_pred,
                  const uint32_t* length, uint32_t n, uint32_t L, int layout, int slot, const fcz_superpose_out* out);
int fcz_superpose_packed(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred,
                         const uint8_t* mask_pred, const uint32_t* row_off, uint32_t n, uint32_t R, int layout, int slot,
                         const fcz_superpose_out* out);
int fcz_superpose_apply(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint32_t* length, uint32_t n, uint32_t L,
                        int layout, const float* rot, const float* trans, float* pos_out);
int fcz_superpose_apply_packed(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint32_t* row_off, uint32_t n, uint32_t R,
                               int layout, const float* rot, const float* trans, float* pos_out);

/* ---- maximised TM-score: seeded iterative superposition of two dense tensor batches ------------------------ */
/* fcz_superpose_dev's tm is the TM-score AT the least-squares superposition, a lower bound. TM-score programs report the maximum over
 * superpositions, found by a search that is seeded with fragments and refined iteratively; these calls run that search per chain for
 * a whole batch on the device and return the superposition it ends at. The reference has no such output. The inputs, the two forms
 * (padded / packed), the layouts and slots, the site rule, d0(S), the float64 arithmetic (every operation rounded, no FMA) and the
 * refusals are those of fcz_superpose_dev above. This is the definition; it is deterministic, so an implementation is checked
 * against it, not against a TM-score program.
 * Per chain with S sites, numbered 0 .. S - 1 in row order, and d_search = min(max(d0, 4.5), 8.0):
 *   fragment lengths   l = S; while l > 4: take l, then l = l / 2 (rounded down); finally take min(S, 4). levels > 0 keeps only the
 *                      first `levels` of these lengths (levels == 0: all).
 *   seeds              for each length in that order the starts 0, step, 2 step, .. while start + l <= S, step = max(l / 2, 1), then
 *                      the start S - l if it is not the last one already taken. The seeds are numbered in this order, so seed 0 is
 *                      the whole chain; fcz_tmscore_seeds(S, levels) is their number (S = 350: 480). S = 0: no seed.
 *   one seed           The selection starts as the fragment's sites. (1) Superpose the selection exactly as fcz_superpose_dev
 *                      superposes all sites: centroids, centred cross sums, Horn's matrix by Jacobi sweeps, t = cb - R ca; a sum over
 *                      the selection keeps that call's order BY CHAIN ROW (lane l adds rows l, l + 64, .., a row outside the
 *                      selection adds nothing, then the xor-butterfly). (2) dev_j for all S sites. (3) tm = (1 / S) sum
 *                      1 / (1 + (dev_j / d0)^2) over all S sites, in the same order. That is round 0. Then at most `iterations`
 *                      further rounds: cut = d_search - 1 in round 1 and d_search + 1 in the later ones; the new selection is
 *                      {j : dev_j < cut}, compared in float64, and while it holds fewer than min(3, S) sites, cut += 0.5 and select
 *                      again (after 16 384 such steps, a deviation beyond 8 000 A, cut = +inf: every site); stop if the new selection
 *                      equals the previous one, otherwise superpose on it and score as above.
 *   the result         the (seed, round) with the largest float64 tm; of equal ones the lowest seed, then the earliest round.
 * Outputs per chain: rot, trans, rmsd (over all S sites), sites, gdt_counts, tm as fcz_superpose_dev defines them, at that
 * superposition; seed [n] int32, the winning seed's number, and selected [n] int32, the size of the winning selection; per row dev.
 * Floats are rounded once from float64. S = 0: the identity, 0, every score 0, seed 0, selected 0. All but rot / trans may be NULL.
 * Seed 0, round 0 is fcz_superpose_dev's fit: with levels = 1, iterations = 0 every shared output holds that call's bytes, and for any
 * levels and iterations tm >= that call's tm, as float32 bits. The result depends on neither the launch geometry, the scratch nor
 * the form: two calls, and padded against packed, give the same bytes. Work: about fcz_tmscore_seeds(S) seeds of a handful of
 * superpositions each, where fcz_superpose_dev does one. Scratch in the ctx: a double per seed (at most 1.7 rows + 70 n + 4 of
 * them, sized on the host from the rows alone), no transform per seed. That size bounds the seeds of chains that do NOT overlap. A packed row_off
 * whose ranges overlap (fcz_superpose_packed_dev computes each such chain fully) may hold more seeds than the scratch: nothing is
 * read or written outside it, but the seeds beyond it are left out, so for overlapping ranges -- and only for them -- a chain's result
 * is the maximum over the seeds that fit (seed 0 alone when none does), and is then no longer independent of the scratch.
 * Enqueued on the ctx stream, no synchronisation. FCZ_E_INVALID_ARG with nothing launched: what fcz_superpose_dev refuses, and iterations > 64. FCZ_E_NOMEM: no room for the scratch. The time goes to a group of its own, "tmscore". */
typedef struct fcz_tmscore_out {
    float*   rot;           /* [n][3][3] */
    float*   trans;         /* [n][3] */
    float*   rmsd;          /* [n] optional */
    int32_t* sites;         /* [n] optional */
    int32_t* gdt_counts;    /* [n][5] optional */
    float*   tm;            /* [n] optional */
    float*   dev;           /* [n][L] / [R] optional */
    int32_t* seed;          /* [n] optional */
    int32_t* selected;      /* [n] optional */
} fcz_tmscore_out;
uint64_t fcz_tmscore_seeds(uint32_t sites, uint32_t levels);   /* the seeds of a chain with that many sites; needs no device */
/* what the output `seed` stands for: the first site and the number of sites of that seed's fragment; FCZ_E_INVALID_ARG for a seed
 * the chain does not have. Needs no device. */
int fcz_tmscore_seed_fragment(uint32_t sites, uint32_t levels, uint64_t seed, uint32_t* start, uint32_t* length);
int fcz_tmscore_dev(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev,
                    const uint8_t* mask_pred_dev, const uint32_t* length_dev, uint32_t n, uint32_t L, int layout, int slot,
                    uint32_t levels, uint32_t iterations, const fcz_tmscore_out* out_dev);
int fcz_tmscore_packed_dev(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev,
                           const uint8_t* mask_pred_dev, const uint32_t* row_off_dev, uint32_t n, uint32_t R, int layout, int slot,
                           uint32_t levels, uint32_t iterations, const fcz_tmscore_out* out_dev);
/* Host-pointer conveniences: the same arrays on the host, staged through the ctx like fcz_superpose; synchronous. */
int fcz_tmscore(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, const uint8_t* mask_pred,
                const uint32_t* length, uint32_t n, uint32_t L, int layout, int slot, uint32_t levels, uint32_t iterations,
                const fcz_tmscore_out* out);
int fcz_tmscore_packed(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred,
                       const uint8_t* mask_pred, const uint32_t* row_off, uint32_t n, uint32_t R, int layout, int slot,
                       uint32_t levels, uint32_t iterations, const fcz_tmscore_out* out);

/* ---- maximised GDT-TS / GDT-HA: a seeded superposition search per cutoff ---------------------------------- */
/* fcz_superpose_dev counts the sites under 0.5, 1, 2, 4 and 8 A at the least-squares fit and fcz_tmscore_dev at the TM-maximising
 * fit. GDT is defined as a MAXIMUM: for each cutoff the largest number of residues that some superposition brings under it, which
 * is what LGA and the TM-score program print. These calls search for it per chain and per cutoff, for a whole batch on the device.
 * The reference has no such output. The inputs, the two forms (padded / packed), the layouts and slots, the site rule, the float64
 * arithmetic (every operation rounded, no FMA) and the refusals are those of fcz_superpose_dev; the seeds, `levels`,
 * iterations <= 64 and the "one seed" procedure are those of fcz_tmscore_dev. This is the definition; it is deterministic, so an
 * implementation is checked against it, not against LGA.
 * Per chain with S sites and the cutoffs c = (0.5, 1, 2, 4, 8):
 *   runs               Every seed is searched in up to six runs, in this order. Each run starts from the seed's fragment and follows
 *                      fcz_tmscore_dev's rounds verbatim: the selection {j : dev_j < cut}, cut += 0.5 while it holds fewer than
 *                      min(3, S) sites, +inf after 16 384 steps, stop when the selection repeats or after `iterations` rounds. Only
 *                      the cut differs. Run 0 has the TM cuts, d_search - 1 in round 1 and d_search + 1 later; run 1 + k has the
 *                      constant cut c_k in every round. `runs` is a bit mask of the six (bit r = run r).
 *   score of a fit     g_k = #{j : dev_j <= c_k} over all S sites, compared in float64, k = 0 .. 4. No TM sum is formed.
 *   result, cutoff k   the (seed, run, round) with the largest g_k among all fits visited; of equal ones the lowest seed, then the
 *                      lowest run, then the earliest round. Round 0 of every run of a seed is one and the same fit (it belongs to
 *                      the lowest run of the mask), so an implementation may skip whatever cannot change the result.
 * Outputs per chain: gdt_counts [n][5] int32, the five maxima (GDT-TS is the mean of the fractions at 1, 2, 4, 8 and GDT-HA of those
 * at 0.5, 1, 2, 4: integers over S, left to the caller); sites [n] int32; rot [n][5][3][3] and trans [n][5][3] float32, rounded
 * once from float64, the superposition behind each cutoff's count (x_true ~ rot @ x_pred + trans); seed, run, selected [n][5]
 * int32: the winning seed's number, the run, and the size of the selection the winning fit was made on. Per row: within [rows]
 * uint8, bit k set iff the row is a site and its deviation under transform k, from the float64 transform, is <= c_k; 0 where the
 * row is no site, lies behind length, or (packed) is covered by no chain, as dev is. The popcount of bit k over a chain is
 * gdt_counts[k]. S = 0: identities and zeros. All outputs but gdt_counts may be NULL. Every byte of what is given is written
 * whatever the inputs hold, and nothing outside it.
 * It follows that levels = 1, iterations = 0 gives fcz_superpose_dev's gdt_counts, and its rot / trans in all five places; that
 * gdt_counts >= fcz_superpose_dev's elementwise for any arguments; that with bit 0 of `runs` set gdt_counts >= fcz_tmscore_dev's at
 * the same levels / iterations; and that gdt_counts[k] <= gdt_counts[k + 1] (a fit's own counts ascend). The result depends on
 * neither the launch geometry nor the form: two calls, and padded against packed, give the same bytes; unlike fcz_tmscore_dev that
 * also holds for packed ranges that overlap, because no scratch scales with the seeds. Work: the seeds times up to six runs of a
 * handful of superpositions each. Scratch in the ctx: 7 n + 1 words of 8 bytes and n of 4.
 * Enqueued on the ctx stream, no synchronisation. FCZ_E_INVALID_ARG with nothing launched: what fcz_tmscore_dev refuses (but rot and
 * trans may be NULL), and runs == 0, runs >= 64, NULL out->gdt_counts. FCZ_E_NOMEM: no room for the scratch. n == 0: FCZ_OK (packed,
 * n == 0 < R: `within` is filled). The time goes to a group of its own, "gdt". */
#define FCZ_GDT_RUNS_ALL 63u   /* the TM cuts and the five constant cuts */
#define FCZ_GDT_RUNS_TM  1u    /* run 0 alone: what a TM-score program's GDT lines amount to, at about fcz_tmscore_dev's cost */
typedef struct fcz_gdt_out {
    int32_t* gdt_counts;    /* [n][5] */
    int32_t* sites;         /* [n] optional */
    float*   rot;           /* [n][5][3][3] optional */
    float*   trans;         /* [n][5][3] optional */
    int32_t* seed;          /* [n][5] optional */
    int32_t* run;           /* [n][5] optional */
    int32_t* selected;      /* [n][5] optional */
    uint8_t* within;        /* [n][L] / [R] optional */
} fcz_gdt_out;
int fcz_gdt_dev(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev,
                const uint8_t* mask_pred_dev, const uint32_t* length_dev, uint32_t n, uint32_t L, int layout, int slot,
                uint32_t levels, uint32_t iterations, uint32_t runs, const fcz_gdt_out* out_dev);
int fcz_gdt_packed_dev(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev,
                       const uint8_t* mask_pred_dev, const uint32_t* row_off_dev, uint32_t n, uint32_t R, int layout, int slot,
                       uint32_t levels, uint32_t iterations, uint32_t runs, const fcz_gdt_out* out_dev);
/* Host-pointer conveniences: the same arrays on the host, staged through the ctx like fcz_superpose; synchronous. */
int fcz_gdt(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, const uint8_t* mask_pred,
            const uint32_t* length, uint32_t n, uint32_t L, int layout, int slot, uint32_t levels, uint32_t iterations, uint32_t runs,
            const fcz_gdt_out* out);
int fcz_gdt_packed(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, const uint8_t* mask_pred,
                   const uint32_t* row_off, uint32_t n, uint32_t R, int layout, int slot, uint32_t levels, uint32_t iterations,
                   uint32_t runs, const fcz_gdt_out* out);

/* ---- TM-align-style structural alignment of chain pairs ------------------------------------------------- */
/* Everything above compares two tensors row for row. These calls compare two DIFFERENT chains, of different lengths and with the
 * correspondence unknown: for every requested pair (chain i of set a, chain j of set b) they find an alignment -- a monotone partial
 * map of a's residues onto b's -- by a dynamic programme that alternates with superposition, and return it with the rigid motion that
 * lays a onto b (x_b ~ rot @ x_a + trans) and the TM-scores normalised by either chain. The reference has no such output. The search
 * follows TM-align's structure but is a definition of its own, given here; it is deterministic, and an implementation is checked
 * against it, not against any program. There is no secondary-structure seed and no search per normalisation, so tm, tm_a and tm_b are
 * LOWER BOUNDS of what TM-align prints.
 * A chain set is padded (pos [n][L][A][3], mask [n][L][A], length [n] or NULL, rows = L) or packed (pos [R][A][3], mask [R][A],
 * row_off [n + 1], rows = R); row_off != NULL means packed. Each set has its own n, form and rows; layout and slot are shared; b may be
 * the same set as a. pairs [m][2] int32 holds chain indices. A chain's rows are those of fcz_superpose_dev (a packed range is clamped
 * to the R rows that exist, one that runs backwards is empty). A SITE is fcz_superpose_dev's site restricted to one tensor: a row
 * inside the chain whose mask is set at the slot and whose three coordinates are finite. Sa and Sb are the sites of the two chains,
 * numbered in row order; Lmin = min(Sa, Sb). wa and wb are the widths: L for a padded set, the largest chain (max_seqlen) for a packed
 * one; both at most FCZ_TMALIGN_MAX_WIDTH. status [m]: 0; 1 for a pair with a chain of more rows than its width; 2 for a pair with an
 * index outside either set. For status 1 and 2 the outputs are the empty result (Lmin = 0 below) and no row of the pair is read.
 * All arithmetic is float64, every operation rounded, no FMA; fits and deviations are fcz_superpose_dev's expressions.
 *   (1) fit of an alignment with P pairs: fcz_tmscore_dev's "one seed" procedure with the pairs in the part of the sites, taken in the
 *       order of a's site number (lane l of the wavefront adds a's sites l, l + 64, .., a site without a partner adds nothing, then the
 *       xor-butterfly), the selection starting as all P pairs, tm = (1 / Lmin) sum_pairs 1 / (1 + (dev / d0)^2) with d0 = d0(Lmin),
 *       d_search from that d0, and at most `refine` rounds of re-selection after round 0 (fewer than min(3, Lmin) selected: the cut
 *       grows as there). The round with the largest tm gives the fit; of equal ones the earliest.
 *   (2) one DP, given (R, t) and a gap g: Q = 65536; d2_ij = |R a_i + t - b_j|^2 in fcz_superpose_dev's order of operations;
 *       q_ij = (int32) floor(Q / (1 + d2_ij / (d0 d0))), 0 for a non-finite d2_ij; G = (int32) rint(g Q) (ties to even).
 *       H[0][j] = H[i][0] = 0 and H[i][j] = max(H[i-1][j-1] + q_ij, H[i-1][j] - G, H[i][j-1] - G) in int32 for i = 1 .. Sa, j = 1 .. Sb
 *       (with widths up to 1024 and g <= 16, |H| <= 2^30 + 2^20: it cannot overflow). End gaps are free: the end cell is the first
 *       maximum of H over (0 .. Sa, Sb) in ascending i, then over (Sa, 0 .. Sb - 1) in ascending j. Trace back from it until i = 0 or
 *       j = 0, at every cell taking the diagonal if H[i][j] == H[i-1][j-1] + q_ij, else up if H[i][j] == H[i-1][j] - G, else left. The
 *       diagonal steps (i, j) align a's site i - 1 with b's site j - 1. Being integer, the DP is exact in whatever order its cells
 *       are evaluated, and a caller reproduces it bit for bit from the same (R, t).
 *   (3) DP iteration from a transform: cur = the transform; for each g of gaps, in order, for up to dp_rounds rounds: the alignment is
 *       DP(cur, g); stop this g if it has fewer than min(3, Lmin) pairs or equals the previous alignment of this g; otherwise fit it
 *       (1) -- a CANDIDATE -- and cur becomes that fit. cur carries over to the next g.
 *   (4) seeds, numbered in this order. Gapless: every shift k with pairs (i, i + k) and an overlap of at least
 *       max(Lmin / 2, min(Lmin, 5)) pairs, in ascending k (k = max(..) - Sa .. Sb - max(..)); each is one fit of the overlap with round 0
 *       only, and a candidate. Then ONE seed: the best gapless seed's transform (largest tm, of equal ones the lowest k) runs (3). Then,
 *       when `fragments` is set: f = min(Lmin, clamp(Lmin / 5, 8, 32)); the starts in each chain are 0, f, 2 f, .. while start + f <= S,
 *       then S - f if it is not the last taken; each pair of starts (a-major) gives the least-squares fit of the f pairs
 *       (sa + u, sb + u), which is no candidate itself, then (3). fcz_tmalign_seeds / fcz_tmalign_seed restate this on the host.
 *   (5) the candidate with the largest float64 tm wins; of equal ones the lowest seed, then the earliest (g, round). On its alignment
 *       run fcz_tmscore_dev's full search over the P pairs (levels, iterations; fragments are ranges of pair numbers), normalised by
 *       Lmin as in (1). The result is the search's fit if its tm is strictly larger than the candidate's, else the candidate's fit: the
 *       final tm is never below any candidate's.
 * Outputs per pair, floats rounded once from float64: rot [m][3][3], trans [m][3] (required); tm (by Lmin); tm_a, tm_b: the same pairs
 * and transform with d0 and the divisor of Sa and of Sb; aligned = P; rmsd = sqrt(sum dev^2 / P) over the pairs; sites_a, sites_b;
 * seed: the winning candidate's seed; status; map [m][wa] int32: for every row of chain a the chain-relative row of b it is aligned
 * with, -1 elsewhere; dev [m][wa] float32: the deviation of an aligned row, 0 elsewhere. Lmin = 0: the identity, zeros, seed 0, map all
 * -1. One and two sites: what fcz_superpose_dev does for them. All but rot / trans may be NULL. Every byte of every output given is
 * written; nothing outside the inputs is read, whatever pairs, length or row_off hold. The result depends on neither the launch
 * geometry nor the form of either set. Scratch in the ctx, sized on the host from m, wa and wb alone: a double per seed and 256 wa
 * bytes of traceback bits per resident wavefront. Enqueued on the ctx stream, no synchronisation. FCZ_E_INVALID_ARG with nothing
 * launched: NULL ctx / a / b / params / out / rot / trans, a set without pos or mask, a padded set with rows == 0, rows above
 * 2^31 - 1, NULL pairs with m > 0, unknown layout, slot outside it, wa or wb of 0 or above FCZ_TMALIGN_MAX_WIDTH,
 * n_gaps outside 1 .. 4, a gap that is not in [0, 16], refine or dp_rounds above 64, iterations above 64. m == 0: FCZ_OK.
 * FCZ_E_NOMEM: no room for the scratch. The time goes to a group of its own, "tmalign". */
#define FCZ_TMALIGN_MAX_WIDTH 1024
typedef struct fcz_chain_set {
    const float*    pos;
    const uint8_t*  mask;
    const uint32_t* length;     /* padded: [n] or NULL */
    const uint32_t* row_off;    /* packed: [n + 1]; NULL: the set is padded */
    uint32_t        n;
    uint32_t        rows;       /* L (padded) or R (packed) */
} fcz_chain_set;
typedef struct fcz_tmalign_params {
    uint32_t fragments;         /* 0 / 1; default 1 */
    uint32_t refine;            /* default 4 */
    uint32_t dp_rounds;         /* default 20 */
    uint32_t n_gaps;            /* default 2 */
    double   gaps[4];           /* default 0.6, 0.0 */
    uint32_t levels;            /* of the final search; 0: all */
    uint32_t iterations;        /* of the final search; default 20 */
} fcz_tmalign_params;
typedef struct fcz_tmalign_out {
    float*   rot;               /* [m][3][3] */
    float*   trans;             /* [m][3] */
    float*   tm;                /* [m] optional, as all below */
    float*   tm_a;
    float*   tm_b;
    int32_t* aligned;
    float*   rmsd;
    int32_t* sites_a;
    int32_t* sites_b;
    int32_t* seed;
    int32_t* status;
    int32_t* map;               /* [m][wa] */
    float*   dev;               /* [m][wa] */
} fcz_tmalign_out;
uint64_t fcz_tmalign_seeds(uint32_t sites_a, uint32_t sites_b, uint32_t fragments);   /* the seeds of a pair; needs no device */
/* what the output `seed` stands for: kind 0 a gapless shift, 1 the DP iteration from the best gapless seed, 2 a fragment pair; shift
 * (kinds 0 and 2: start_b - start_a), the first site in a and in b and the number of pairs of the seed's fit (kind 1: zeros).
 * FCZ_E_INVALID_ARG for a seed the pair does not have. Needs no device. */
int fcz_tmalign_seed(uint32_t sites_a, uint32_t sites_b, uint32_t fragments, uint64_t seed, int32_t* kind, int32_t* shift,
                     uint32_t* start_a, uint32_t* start_b, uint32_t* length);
int fcz_tmalign_dev(fcz_ctx* ctx, const fcz_chain_set* a_dev, const fcz_chain_set* b_dev, const int32_t* pairs_dev, uint32_t m,
                    uint32_t wa, uint32_t wb, int layout, int slot, const fcz_tmalign_params* params, const fcz_tmalign_out* out_dev);
/* What the last fcz_tmalign_dev / fcz_tmalign call of this ctx did in step (3): the dynamic programmes it ran (the winner's second
 * run included) and the sum of their Sa * Sb cells; zeros before the first call. Waits for the ctx stream. For measurements. */
int fcz_tmalign_last_work(fcz_ctx* ctx, uint64_t* dps, uint64_t* cells);
/* The DP of (2) alone, once per pair, from caller-given float32 transforms rot [m][3][3], trans [m][3] (promoted exactly to float64),
 * with d0(Lmin) and the gap `gap`: map [m][wa] (required) and aligned [m] (may be NULL) as above; a pair with a status gets a map of
 * -1 and aligned 0. For callers who superposed some other way. Refusals as above (NULL rot / trans / map). */
int fcz_tmalign_dp_dev(fcz_ctx* ctx, const fcz_chain_set* a_dev, const fcz_chain_set* b_dev, const int32_t* pairs_dev, uint32_t m,
                       uint32_t wa, uint32_t wb, int layout, int slot, const float* rot_dev, const float* trans_dev, double gap,
                       int32_t* map_dev, int32_t* aligned_dev);
/* Host-pointer conveniences: the sets' arrays, pairs and the outputs on the host (the structs themselves always are), staged through
 * the ctx; synchronous. */
int fcz_tmalign(fcz_ctx* ctx, const fcz_chain_set* a, const fcz_chain_set* b, const int32_t* pairs, uint32_t m, uint32_t wa,
                uint32_t wb, int layout, int slot, const fcz_tmalign_params* params, const fcz_tmalign_out* out);
int fcz_tmalign_dp(fcz_ctx* ctx, const fcz_chain_set* a, const fcz_chain_set* b, const int32_t* pairs, uint32_t m, uint32_t wa,
                   uint32_t wb, int layout, int slot, const float* rot, const float* trans, double gap, int32_t* map,
                   int32_t* aligned);

/* ---- torsion-angle tensors: the record's internal coordinates, no reconstruction ------------------------ */
/* What Foldcomp::decompress dequantises before it places an atom (src/foldcomp.cpp:784-804: the backbone torsions and bond angles of
 * every packed word; :338-369 for the side-chain torsion bytes) and the FCZ branch of foldcomp.cxx's get_data returns as Python lists
 * (phi / psi / omega / bond_angles; it omits the side-chain torsions), as tensors for a whole batch. The values come straight from
 * the record bytes: no atom is decoded, no coordinate kernel runs, and they are the very floats the decoder places atoms with.
 * Per residue row FCZ_ANGLE_COLUMNS float32 in degrees and as many mask bytes (1 = the record holds the value). For entry e with
 * n residues, row l:
 *   0 phi    C(l-1)-N-CA-C                 `phi` of word l-1      1 <= l <= n-1
 *   1 psi    N-CA-C-N(l+1)                 `psi` of word l        l <= n-2
 *   2 omega  CA-C-N(l+1)-CA(l+1)           `omega` of word l      l <= n-2     (the peptide bond BEHIND residue l)
 *   3 N-CA-C at l                          `n_ca_c` of word l-1   1 <= l <= n-1
 *   4 CA-C-N(l+1)                          `ca_c_n` of word l     l <= n-2
 *   5 C-N(l+1)-CA(l+1)                     `c_n_ca` of word l     l <= n-2
 *   6 .. 9 chi1 .. chi4                    the side-chain torsion byte of the atom fcz_chi_atom names, where the type has that chi
 * Word k holds psi of k, omega of k -> k+1, and phi and N-CA-C of k+1 (src/foldcomp.cpp:784-841); residue 0's N-CA-C is not in the
 * format, and the fields of word n-1 are not angles and never reach the output. Columns 0 .. 5 are dequantised with the header's six
 * min / cont_f pairs, the chis with the fixed-angle quantiser (FixedAngleDiscretizer(255), src/discretizer.h:89-106). The residue
 * code that selects the chi atoms is the decoder's (residue 0: header.firstResidue). Where the mask is 0 the value is 0.0f.
 *   padded   angles [n][L][10], mask [n][L][10]: an entry longer than L keeps its first L rows (row L-1 of a cropped entry still has
 *            psi and omega: word L-1 exists); rows behind an entry's length, and all L rows of an entry the decoder skips, are 0 / 0.
 *   packed   angles [R][10], mask [R][10] over the rows of res_off (R = res_off[n]); a skipped entry has no row.
 * Every byte of both arrays is written exactly once and nothing outside them; every index is 64-bit. */
#define FCZ_ANGLE_COLUMNS 10
/* pure host: atom code of the atom whose torsion is chi k + 1 (k = 0 .. 3) of a residue of res_code, -1 when the type has no such
 * chi (ALA, GLY, codes 20 .. 23) or an argument is out of range. The atom's predecessors in the reference's src/amino_acid.h are
 * the standard chi quadruple's first three atoms. */
int fcz_chi_atom(int res_code, int k);
/* Device-resident, beside Foldcomp::decompress (src/foldcomp.cpp:784-804) and the FCZ branch of foldcomp.cxx's get_data: every pointer
 * a device pointer, res_off_dev what fcz_decompress_sizes_dev left for the same entries. Enqueued on the ctx stream, no
 * synchronisation. The calls read only their arguments: nothing of a decode, nothing the ctx keeps -- the same output before and
 * after a fcz_decompress_batch_dev on the same pointers, and the sizes memo stays as it was. A NULL pointer, or L == 0 in the padded
 * form: FCZ_E_INVALID_ARG, nothing launched; n == 0: FCZ_OK. */
int fcz_angles_dev(fcz_ctx* ctx, const uint8_t* blob_dev, const uint64_t* off_dev, uint32_t n, const uint32_t* res_off_dev,
                   uint32_t L, float* angles_dev, uint8_t* mask_dev);
int fcz_angles_packed_dev(fcz_ctx* ctx, const uint8_t* blob_dev, const uint64_t* off_dev, uint32_t n, const uint32_t* res_off_dev,
                          float* angles_dev, uint8_t* mask_dev);
/* Host-pointer conveniences, shaped like fcz_decompress_dense / fcz_decompress_dense_packed (Foldcomp::read, src/foldcomp.cpp:904,
 * then the dequantisation of Foldcomp::decompress, :784-804, for every entry; the batched form of get_data's FCZ branch in
 * foldcomp.cxx): records in, host arrays out, the sizes pass and the angle kernel only. Padded: L = 0 is the longest entry of the
 * batch, the width used comes back through *L_out (may be NULL). Packed: *R_out (may be NULL) receives R and row_off[n + 1] (may be
 * NULL) the row offsets. angles and mask both NULL: a sizing call (L_out / R_out required). status[n] (may be NULL) receives the
 * per-entry fcz_status. NULL ctx / blob / off, one of angles / mask without the other, neither of them nor L_out / R_out:
 * FCZ_E_INVALID_ARG. */
int fcz_decompress_angles(fcz_ctx* ctx, const uint8_t* blob, const uint64_t* off, uint32_t n, uint32_t L, uint32_t* L_out,
                          float* angles, uint8_t* mask, int32_t* status);
int fcz_decompress_angles_packed(fcz_ctx* ctx, const uint8_t* blob, const uint64_t* off, uint32_t n, uint32_t* R_out, uint32_t* row_off,
                                 float* angles, uint8_t* mask, int32_t* status);
/* The per-entry residue window of the padded angle tensors, beside fcz_angles_dev (the dequantisation of Foldcomp::decompress,
 * src/foldcomp.cpp:784-804) and with the rule of fcz_dense_window_dev: row l holds residue start_dev[e] + l of entry e, bit for bit
 * the row fcz_angles_dev writes for that residue at L = the longest entry, or zeros when the entry has no such residue. Row 0 of a
 * window with start >= 1 therefore HAS phi and N-CA-C (word start - 1 exists), and the last row of a window that ends inside the chain
 * has psi, omega and the two bond angles behind it. start[e] at or behind the entry's length (0xFFFFFFFF included), or a skipped
 * entry: all L rows are 0 / 0. start_dev == NULL means all zeros: angles and mask are byte-identical to fcz_angles_dev's.
 * aatype_dev (may be NULL) receives [n][L] uint8: min(residue code, 20) with the decoder's codes (residue 0: header.firstResidue) in
 * a residue row, 20 in a padding row -- what fcz_dense_dev writes as aatype, without a decode. Like fcz_angles_dev the call reads
 * only its arguments; its refusals, stream and "angles" timing group are fcz_angles_dev's. */
int fcz_angles_window_dev(fcz_ctx* ctx, const uint8_t* blob_dev, const uint64_t* off_dev, uint32_t n, const uint32_t* res_off_dev,
                          uint32_t L, const uint32_t* start_dev, float* angles_dev, uint8_t* mask_dev, uint8_t* aatype_dev);
/* Host-pointer convenience, beside fcz_decompress_angles and shaped like it (Foldcomp::read, src/foldcomp.cpp:904, then the
 * dequantisation of :784-804): start[n] is a host array (NULL: all zeros), aatype [n][L] may be NULL. L = 0 is the longest entry;
 * angles and mask both NULL: a sizing call (L_out required). Refusals are fcz_decompress_angles'. */
int fcz_decompress_angles_window(fcz_ctx* ctx, const uint8_t* blob, const uint64_t* off, uint32_t n, uint32_t L, const uint32_t* start,
                                 uint32_t* L_out, float* angles, uint8_t* mask, uint8_t* aatype, int32_t* status);

/* ---- rigid frames of the dense tensors: backbone, psi and chi groups per residue -------------------------- */
/* What frame-based models start from (invariant-point attention and FAPE, SE(3) diffusion, local-frame edge features): every
 * residue as rigid transforms, global = rot * local + trans, built on the device from the dense tensors above. The reference has no
 * such output; like the dense calls these stand beside Foldcomp::decompress (src/foldcomp.cpp:779) and read what fcz_dense_dev /
 * fcz_dense_window_dev / fcz_dense_packed_dev wrote, or any tensors of those shapes.
 * Inputs, rows = n * L: pos [rows][A][3] float32, mask [rows][A] uint8, aatype [rows] uint8 (types 0 .. 19 in the dense tensors'
 * order = residue codes 0 .. 19; every other value is a type without chi groups), length [n] uint32 or NULL. A =
 * fcz_dense_width(layout). The PACKED form is n = 1, L = R, length = NULL: frames use atoms of their own row only, so there is no
 * second entry point.
 * groups selects the output width G = fcz_frames_width(groups):
 *   FCZ_FRAMES_BACKBONE  G = 1  group 0 only; aatype may be NULL
 *   FCZ_FRAMES_ALL       G = 8  indexed like AlphaFold / OpenFold rigidgroups_gt_frames: 0 backbone, 1 and 2 unused (they never
 *                               exist), 3 psi, 4 .. 7 chi1 .. chi4
 * Every group has three defining atoms (a0, a1, a2) = fcz_frame_atom(type, group, 0 .. 2), two vectors and the origin t = a1:
 *   group 0 backbone     (C, CA, N)                    v1 = a0 - a1 = C - CA               v2 = a2 - a1 = N - CA    t = CA
 *   group 3 psi          (CA, C, O)                    v1 = a1 - a0 = C - CA               v2 = a2 - a1 = O - C     t = C
 *   group 4 + k, k < 4   (c[k+1], c[k+2], c[k+3])      v1 = a1 - a0 = c[k+2] - c[k+1]      v2 = a2 - a1             t = c[k+2]
 * where c is the chain N, CA, CB, X1, X2, X3, X4 and Xi the atom fcz_chi_atom(type, i - 1) names: chi1 has origin CB, its x axis
 * runs CA -> CB and X1 lies in the xy half-plane y > 0. So a1 is always the origin, a2 always the atom that fixes the xy plane
 * (local (x, y > 0, 0)), and a0 the other atom on the x axis: at local (+|v1|, 0, 0) for group 0, at (-|v1|, 0, 0) for the others.
 * N, CA, C, O have the same slot in every type, so groups 0 and 3 are defined for every aatype value and every layout; the chi
 * groups for types 0 .. 19 in atom37 and atom14 (backbone4 has no slot for them).
 * A group EXISTS for a row when the row lies inside its chain (l < min(length[e], L), or always when length is NULL), the type has
 * the group, the layout has a slot for all three atoms, their three masks are set, their nine coordinates are finite, and both
 * norms below are finite and > 0. All arithmetic is float32, every operation rounded, no FMA, in exactly this order:
 *   n1 = sqrt((v1x*v1x + v1y*v1y) + v1z*v1z)          e1 = v1 / n1            (three divisions)
 *   d  = (e1x*v2x + e1y*v2y) + e1z*v2z                 u  = v2 - e1*d          (ux = v2x - e1x*d, ...)
 *   n2 = sqrt((ux*ux + uy*uy) + uz*uz)                 e2 = u / n2
 *   e3 = e1 x e2     (e3x = e1y*e2z - e1z*e2y, e3y = e1z*e2x - e1x*e2z, e3z = e1x*e2y - e1y*e2x)
 * with sqrt and / the correctly rounded float32 results. Outputs, caller-owned, every byte written:
 *   rot [rows][G][3][3] float32   rot[i][j] = e_(j+1)[i]: the columns are the axes
 *   trans [rows][G][3] float32    the origin atom's bits
 *   frame_mask [rows][G] uint8    1 where the group exists
 * Where a group does not exist rot is the identity, trans 0 and the mask 0: groups 1 and 2, padding rows, rows at or behind
 * length (whatever pos / mask / aatype hold there: they are not read as data), a NaN atom, coincident (n1 = 0) or collinear
 * (n2 = 0) atoms, norms that overflow. For group 0 this is AlphaFold supplement Algorithm 21 on (N, CA, C); for the others it is
 * from_3_points(neg_x = a0, origin = a1, xy_plane = a2) on the last three atoms of the chi quadruple. Negating both e1 and e3 is
 * exact, so OpenFold's axis flip of group 0 is the same frame.
 * Ambiguity is a table, not an output: fcz_frame_ambiguous is 1 for group 5 of ASP, PHE, TYR and group 6 of GLU, whose plane atom
 * a2 has a partner (OD1 / OD2, CD1 / CD2, OE1 / OE2) that a 180-degree turn about the group's x axis exchanges with it. Renaming the
 * pair keeps e1 and t and negates the in-plane direction e2, hence e3 = e1 x e2 too: the alternative frame is rot * diag(1, -1, -1)
 * with the same trans. It is not written.
 * Every index that scales with rows * A or rows * G is 64-bit. The time goes to the group "frames". */
enum fcz_frame_groups { FCZ_FRAMES_BACKBONE = 0, FCZ_FRAMES_ALL = 1 };
/* pure host: 1 / 8, -1 for an unknown value */
int fcz_frames_width(int groups);
/* pure host: atom code of defining atom j = 0 .. 2 of `group` (0 .. 7) in a residue of res_code (0 .. 23), in the order above: j = 1
 * the origin, j = 2 the atom that fixes the xy plane, j = 0 the other atom on the x axis (the tail of v1 for every group but 0,
 * where it is the head C). -1 when the type has no such group (groups 1, 2; a chi the type lacks) or an argument is out of range.
 * Groups 0 and 3 answer (C, CA, N) and (CA, C, O) for all 24 codes. The slot is fcz_dense_slot(layout, res_code, atom) for the chi
 * groups and the type-independent slot of N / CA / C / O (fcz_dense_slot(layout, 0, atom)) for groups 0 and 3. */
int fcz_frame_atom(int res_code, int group, int j);
/* pure host: 1 where the group's frame is ambiguous under the symmetric renamings above, else 0 (out-of-range arguments too) */
int fcz_frame_ambiguous(int res_code, int group);
/* Device-resident: every pointer a device pointer. Enqueued on the ctx stream, no synchronisation. NULL ctx / pos / mask / rot /
 * trans / frame_mask, NULL aatype with FCZ_FRAMES_ALL, unknown layout or groups, L == 0: FCZ_E_INVALID_ARG, nothing launched;
 * n == 0: FCZ_OK. */
int fcz_frames_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint8_t* aatype_dev, const uint32_t* length_dev,
                   uint32_t n, uint32_t L, int layout, int groups, float* rot_dev, float* trans_dev, uint8_t* frame_mask_dev);
/* Host-pointer convenience: the same arrays on the host, staged through the ctx like fcz_knn; synchronous. */
int fcz_frames(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint8_t* aatype, const uint32_t* length, uint32_t n, uint32_t L,
               int layout, int groups, float* rot, float* trans, uint8_t* frame_mask);

/* ---- dense model-input tensors -> fcz_chain_batch -> FCZ records ---------------------------------------- */
/* The way back: n chains held as the padded arrays above (a model's predictions, a filtered or re-cropped set, what fcz_dense_dev
 * wrote) become the flat structure-of-arrays batch fcz_compress_sizes_dev / fcz_compress_batch_dev take, on the device. These entry
 * points stand in front of Foldcomp::compress (src/foldcomp.cpp:562; preprocess :450), which starts from a flat
 * span<AtomCoordinate>; the reference has no dense input.
 * Input (layouts and A as above; every array row-major and naturally aligned):
 *   pos [n][L][A][3] float32, mask [n][L][A] uint8 (any non-zero byte = present), aatype [n][L] uint8, length [n] uint32: required
 *   plddt [n][L] float32: optional, NULL = 0 (the residue's B-factor, bfac_ca)
 *   first_res_index [n] (NULL = 1), first_atom_index [n] (NULL = 1), chain_id [n] (NULL = 'A'), titles + title_off [n + 1] (byte
 *   offsets; both or neither, NULL = empty titles): the header fields of the records.
 * Contract:
 *   residue codes    aatype 0 .. 19 = A R N D C Q E G H I L K M F P S T W Y V = residue codes 0 .. 19 (what fcz_dense_dev wrote);
 *                    20 = UNK (code 23); a larger value refuses the chain (FCZ_E_RESIDUE).
 *   atoms            of row l < length[c]: the slots with mask != 0 that the residue's type owns in the layout (fcz_dense_slot), in
 *                    the canonical order fcz_res_code_atom(res_code, j, 0). A set mask byte in a slot the type does not own is
 *                    ignored; UNK owns N, CA, C only; backbone4 gives N, CA, C, O.
 *   missing atoms    a side-chain atom whose mask is 0 is absent from the batch; the compress kernels read the all-zero record
 *                    for it, as the reference does (findFirstAtomCoords, src/sidechain.cpp:140-147).
 *   OXT              atom37 only: slot 36 of row length[c] - 1, when its mask is set, becomes the chain's last atom (code 36, inside
 *                    the last residue's atom range). A set slot 36 on any other row is ignored. atom14 / backbone4: no OXT.
 *   never data       pos where mask == 0, and every array in rows l >= length[c], may hold NaN, infinities or garbage: nothing of
 *                    it reaches the batch or raises FCZ_E_NONFINITE. A non-finite value in a present atom or in the plddt of a row
 *                    l < length[c] is refused by the compress kernels as for any batch (FCZ_E_NONFINITE).
 *   refusals         per chain; the call succeeds and the neighbours are untouched. length[c] > L or > 65535: FCZ_E_INVALID_ARG;
 *                    aatype > 20, or a row l < length[c] without all of N, CA and C: FCZ_E_RESIDUE. A refused chain keeps its place
 *                    in the batch with ZERO residues and atoms (its title and header fields stay): its record range has the size
 *                    fcz_compress_sizes gives a chain without residues and is filled with zeros, as for every chain the pack
 *                    kernels refuse. length[c] < 2 is not refused here: the chain enters the batch as it is and the compress
 *                    kernels answer FCZ_E_TOO_SHORT. fcz_compress_dense_* report the refusal of this stage in status[c] in place
 *                    of the FCZ_E_TOO_SHORT the empty range would earn.
 *   sizes            every index into the dense arrays is 64-bit (n * L * A * 3 may pass 2^32). The flat batch counts in 32 bits:
 *                    when the chains' residues or atoms sum beyond 2^32 - 1 the call returns FCZ_E_INVALID_ARG before the batch
 *                    is allocated or filled (the sums exist only after the counting pass over the masks).
 * Bad arguments (NULL ctx, unknown layout, L == 0, anchor_threshold <= 0, NULL pos / mask / aatype / length, titles without
 * title_off or the reverse): FCZ_E_INVALID_ARG, nothing launched; n == 0: FCZ_OK. */
typedef struct fcz_dense_in {
    const float*    pos;              /* [n][L][A][3] */
    const uint8_t*  mask;             /* [n][L][A] */
    const uint8_t*  aatype;           /* [n][L] */
    const uint32_t* length;           /* [n] */
    const float*    plddt;            /* [n][L] optional */
    const int32_t*  first_res_index;  /* [n] optional */
    const int32_t*  first_atom_index; /* [n] optional */
    const char*     chain_id;         /* [n] optional */
    const char*     titles;           /* optional, with title_off */
    const uint32_t* title_off;        /* [n + 1] */
} fcz_dense_in;
/* Device-resident: every pointer inside in_dev a device pointer. *out = the batch in HBM, as fcz_ingest_pdb_dev leaves one: its
 * arrays are owned by the ctx and valid until its next undense call, except the header fields and titles the caller passed, which
 * the batch refers to where they are (keep them until the compress calls have run). counts = {chains, residues, atoms};
 * chain_status_dev[n] (may be NULL) receives FCZ_OK or the refusal of this stage. One stream synchronisation (the totals). */
int fcz_undense_dev(fcz_ctx* ctx, const fcz_dense_in* in_dev, uint32_t n, uint32_t L, int layout, int anchor_threshold,
                    fcz_chain_batch* out, uint32_t counts[3], int32_t* chain_status_dev);
/* the resident batch of the last undense call copied to the host (every pointer of host_batch caller-allocated for its counts, titles
 * for title_off[n] bytes; the struct's const is cast away; NULL = not wanted) and its per-chain verdicts (may be NULL) */
int fcz_undense_fetch(fcz_ctx* ctx, const fcz_chain_batch* host_batch, int32_t* chain_status);
/* Tensors in, FCZ records out: fcz_undense_dev + fcz_compress_sizes_dev + fcz_compress_batch_dev on the resident batch, begin / fetch
 * as fcz_compress_pdb_begin / _fetch because the blob's size is known only after the sizes pass. begin(): counts as above,
 * *fcz_bytes = size of the blob; fetch(): record offsets out_off[n + 1], per-chain status[n] (either may be NULL), then the blob.
 * _dev: device pointers in, and the records are copied device-to-device into caller-allocated buffers (torch tensors) on the ctx
 * stream, no synchronisation in fetch. Without _dev: host pointers, for numpy callers and tests. */
int fcz_compress_dense_begin_dev(fcz_ctx* ctx, const fcz_dense_in* in_dev, uint32_t n, uint32_t L, int layout, int anchor_threshold,
                                 uint32_t counts[3], uint64_t* fcz_bytes);
int fcz_compress_dense_fetch_dev(fcz_ctx* ctx, uint64_t* out_off_dev, int32_t* status_dev, uint8_t* blob_dev);
int fcz_compress_dense_begin(fcz_ctx* ctx, const fcz_dense_in* in, uint32_t n, uint32_t L, int layout, int anchor_threshold,
                             uint32_t counts[3], uint64_t* fcz_bytes);
int fcz_compress_dense_fetch(fcz_ctx* ctx, uint64_t* out_off, int32_t* status, uint8_t* blob);
/* The packed form of the three calls above, in front of Foldcomp::compress (src/foldcomp.cpp:562) like them: chain c occupies rows
 * row_off[c] .. row_off[c + 1] - 1 of pos [R][A][3], mask [R][A], aatype [R] and plddt [R] (in->length is not read and may be
 * NULL); R is the number of rows the caller's arrays have. The fcz_dense_in contract holds unchanged (residue codes, missing
 * atoms, the OXT in slot 36 of the chain's LAST row, never data, refusals, 32-bit totals), with these refusals per chain, each
 * answered with FCZ_E_INVALID_ARG and zero residues, the neighbours untouched and nothing read outside rows 0 .. R - 1:
 * row_off[c + 1] < row_off[c]; row_off[c + 1] > R; a length above 65535. Chains may share rows. fcz_undense_fetch and
 * fcz_compress_dense_fetch[_dev] serve both forms. Bad arguments (NULL ctx, unknown layout, anchor_threshold <= 0, NULL pos / mask /
 * aatype / row_off, titles without title_off or the reverse): FCZ_E_INVALID_ARG, nothing launched; n == 0: FCZ_OK. */
int fcz_undense_packed_dev(fcz_ctx* ctx, const fcz_dense_in* in_dev, const uint32_t* row_off_dev, uint32_t n, uint32_t R, int layout,
                           int anchor_threshold, fcz_chain_batch* out, uint32_t counts[3], int32_t* chain_status_dev);
int fcz_compress_dense_packed_begin_dev(fcz_ctx* ctx, const fcz_dense_in* in_dev, const uint32_t* row_off_dev, uint32_t n, uint32_t R,
                                        int layout, int anchor_threshold, uint32_t counts[3], uint64_t* fcz_bytes);
int fcz_compress_dense_packed_begin(fcz_ctx* ctx, const fcz_dense_in* in, const uint32_t* row_off, uint32_t n, uint32_t R,
                                    int layout, int anchor_threshold, uint32_t counts[3], uint64_t* fcz_bytes);

/* ---- structure ingest: PDB / mmCIF text -> fcz_chain_batch on the device ----------------------------- */
/* What the reference's driver does to every input file before Foldcomp::compress (src/main.cpp:455-508): StructureReader
 * (src/structure_reader.cpp:31-61; the fixed-column ATOM / HETATM record as foldcomp/foldcomp.cxx:259-278 reads it),
 * removeAlternativePosition (src/atom_coordinate.cpp:362-370), identifyChains (:469-497), identifyDiscontinousResInd (:506-530),
 * then per fragment the residue split, residue codes and CA B-factors of Foldcomp::preprocess (src/foldcomp.cpp:450-559).
 * Input: the bytes of n_files PDB files back to back (file i = text[file_off[i] .. file_off[i+1])), their base names
 * (names[name_off[i] .. name_off[i+1]); the first stem_len[i] characters are the stem that names the records and replaces an
 * absent title, src/main.cpp:465). Output: one fcz_chain_batch in HBM holding every fragment the codec can take, file order
 * then fragment order, ready for fcz_compress_sizes_dev / fcz_compress_batch_dev, plus per chain the file it came from and
 * how the reference names it:
 *   chain_meta = chain id | fragment ordinal << 8 | FCZ_INGEST_MULTI_CHAIN (the file holds several chains: the id is appended
 *                to the name) | FCZ_INGEST_MULTI_FRAG (the chain has gaps: "_<ordinal>" is appended).
 * The reading rules are those of the reference's reader (gemmi 0.5.1 read_pdb, lib/gemmi/pdb.hpp:262-365): record names on
 * four letters case-insensitively, END stops the reading, B-factor 20 on a line that ends before column 65, title = last
 * HEADER id code else the TITLE texts concatenated; MODEL n / atoms / ENDMDL groups under rising plain numbers (ensembles) are read in
 * file order with a new chain at every group, as the reader keeps them.
 * file_status[i]: FCZ_OK, FCZ_INGEST_NO_ATOMS, or FCZ_INGEST_HOST_*: something this path does not decide the way that reader
 * would on its own (a number field the exact fixed-point rule does not cover, a blank or hybrid-36 number, a two-character chain
 * name, an ATOM record shorter than its coordinates, an ANISOU record that does not stand directly behind its atom, models not numbered upwards or atoms outside them, a NUL byte, a residue whose (number,
 * insertion code) does not grow inside its run of one chain name -- the reader regroups such lines --, a title beyond 512 bytes,
 * more than 32 fragments) -- nothing of that file is in the batch and the caller's own reader has to take it (the hosts of this
 * repository restate every rule: foldcomp_amd/structure.py parse_pdb_gemmi, host/foldcomp_hip.cpp parse_pdb_gemmi). refused[2k], refused[2k+1] = file, chain_meta | reason << 24 of the
 * fragments that were left out (residue name the codec does not know, residue without N, CA, C in order or with a second one
 * of them, a last atom that carries another residue name than its residue, chain beyond the header's counts,
 * --skip-discontinuous). Gzipped files: fcz_ingest_gz_begin below (inflated on the device in front of this stage).
 * mmCIF text (round 4, k_ingest_parse_cif + k_ingest_rows_cif): a file that opens with data_ (gemmi::coor_format_from_content, lib/gemmi/mmread.hpp:31-47)
 * is read by gemmi's mmCIF rules (cif.hpp:37-148 grammar, mmcif.hpp:560-680 make_structure: the _atom_site loop's 23 columns by any
 * case, chain = auth_asym_id else label_asym_id, residue = auth_seq_id + comp id, atom name = auth_atom_id else label_atom_id,
 * title = _entry.id) when it has the shape every predicted-structure file has: one block, one item per line (or a tag line and its
 * value / text field on the following lines), loops of whole-line rows, _atom_site rows of one line each without quoted values
 * other than the atom name ("O5'"), chain names of up to four characters, integer residue numbers with an optional one-character
 * insertion code, models one after the other under rising plain numbers (1, 2, 3 ...), residues rising by (number, insertion code) inside a chain run, coordinates as plain decimals of at
 * most 15 digits (round 6: the PDB archive's shape beside AFDB's). Every other mmCIF file comes back as FCZ_INGEST_HOST_FIELD exactly
 * as a PDB file outside the fixed layout does (save_ frames, several blocks, comments after values, other quoted values, longer chain
 * names, a model that comes back or is not a plain number, '?' coordinates, duplicate tags, a _cell angle that is not plainly non-zero, lines beyond 255 characters ...). */
enum fcz_ingest_status { FCZ_INGEST_HOST_FIELD = 1, FCZ_INGEST_HOST_TITLE = 2, FCZ_INGEST_HOST_FRAGS = 3, FCZ_INGEST_NO_ATOMS = 4 };
enum fcz_ingest_reason { FCZ_INGEST_REF_RESNAME = 1, FCZ_INGEST_REF_BACKBONE = 2, FCZ_INGEST_REF_TOO_LONG = 3, FCZ_INGEST_REF_SKIP_DISC = 4,
                         FCZ_INGEST_REF_BACKBONE_TWICE = 5, FCZ_INGEST_REF_LAST_NAME = 6 };
#define FCZ_INGEST_MULTI_CHAIN (1u << 16)
#define FCZ_INGEST_MULTI_FRAG  (1u << 17)
#define FCZ_INGEST_SKIP_DISCONTINUOUS 1   /* flags: --skip-discontinuous (src/main.cpp:476-480) */
typedef struct fcz_ingest_result {        /* device pointers owned by the ctx, valid until its next ingest call */
    fcz_chain_batch batch;
    const uint32_t* chain_file;           /* [C] */
    const uint32_t* chain_meta;           /* [C] */
    const int32_t*  file_status;          /* [F] */
    const uint32_t* refused;              /* [2 * n_refused], in no particular order */
    uint32_t n_files, n_refused;
    const uint32_t* chain_name4;          /* [C] the chain's NAME, up to four characters packed little-endian (mmCIF auth_asym_id of large
                                           * complexes: "AA", "B2" ...; chain_meta's low byte is its first character, what the FCZ header
                                           * keeps): what the reference appends to a record's name when the file holds several chains
                                           * (src/main.cpp:489-491) */
} fcz_ingest_result;
/* Device-resident: text_dev / file_off_dev / names_dev / name_off_dev / stem_len_dev are device pointers; one stream
 * synchronisation (the totals). */
int fcz_ingest_pdb_dev(fcz_ctx* ctx, const uint8_t* text_dev, const uint64_t* file_off_dev, uint32_t n_files, uint64_t text_bytes,
                       const char* names_dev, const uint32_t* name_off_dev, const uint32_t* stem_len_dev, int anchor_threshold,
                       int flags, fcz_ingest_result* out);
/* Host-pointer convenience: copies the text in (true DMA from fcz_pinned_alloc memory) and runs the ingest; the batch stays
 * in the ctx. counts = {chains, residues, atoms, title bytes, refused fragments}. fetch() copies the batch arrays (every
 * pointer of host_batch must be caller-allocated for those counts; the struct's const is cast away) and the per-chain /
 * per-file / refusal arrays (any of them may be NULL) to the host. */
int fcz_ingest_pdb_begin(fcz_ctx* ctx, const uint8_t* text, const uint64_t* file_off, uint32_t n_files, const char* names,
                         const uint32_t* name_off, const uint32_t* stem_len, int anchor_threshold, int flags, uint32_t counts[5]);
int fcz_ingest_pdb_fetch(fcz_ctx* ctx, const fcz_chain_batch* host_batch, uint32_t* chain_file, uint32_t* chain_meta,
                         int32_t* file_status, uint32_t* refused);
/* the chains' names of the resident batch (fcz_ingest_result.chain_name4) copied to chain_name4[C]; after any *_begin call */
int fcz_ingest_chain_names_fetch(fcz_ctx* ctx, uint32_t* chain_name4);
/* Text in, FCZ records out: ingest + fcz_compress_sizes_dev + fcz_compress_batch_dev on the resident batch.
 * begin(): counts = {chains, residues, atoms, title bytes, refused fragments}, *fcz_bytes = size of the blob; fetch(): record
 * offsets out_off[C+1], per-chain status[C] and the arrays of fcz_ingest_pdb_fetch (any may be NULL), then the blob. */
int fcz_compress_pdb_begin(fcz_ctx* ctx, const uint8_t* text, const uint64_t* file_off, uint32_t n_files, const char* names,
                           const uint32_t* name_off, const uint32_t* stem_len, int anchor_threshold, int flags, uint32_t counts[5],
                           uint64_t* fcz_bytes);
int fcz_compress_pdb_fetch(fcz_ctx* ctx, uint64_t* out_off, int32_t* status, uint32_t* chain_file, uint32_t* chain_meta,
                           int32_t* file_status, uint32_t* refused, uint8_t* blob);

/* ---- inflate: gzip members -> text in HBM (round 6) -------------------------------------------------------- */
/* What the reference's reader does with zlib before it parses a `.pdb.gz` / `.cif.gz` input: gemmi::MaybeGzipped
 * (lib/gemmi/gz.hpp:105-133: gzread into a buffer sized from ISIZE, the member's last four bytes) for files, uncompressBuffer
 * (src/structure_reader.cpp:156-203: inflateInit2(15 | 32), inflate()) for database / tar entries. Here: one wavefront per member
 * (k_inflate, foldcomp_amd/csrc/fcz_inflate.h: RFC 1952 header and trailer, RFC 1951 stored / fixed / dynamic blocks, CRC-32 and ISIZE
 * verified on the device), the text written where the structure ingest reads it.
 * The device never guesses: status[i] != FCZ_INFLATE_OK means the member was NOT inflated here (its text range holds blanks) and
 * the caller's zlib has to take it -- that covers every stream zlib's inflate() rejects (invalid block type / stored lengths /
 * code-length set, over-subscribed or incomplete code, invalid literal/length or distance code, distance too far back, incorrect
 * data or length check, truncation) and streams this decoder does not read although zlib does: a header CRC (FHCRC), a header
 * beyond 252 bytes, an incomplete literal/length code, more than one member / bytes after the trailer, an ISIZE that is not the
 * text's size. FCZ_INFLATE_OK: the bytes are what zlib's inflate() returns for the member, checked by CRC-32 and ISIZE. */
enum fcz_inflate_status {
    FCZ_INFLATE_OK = 0,
    FCZ_INFLATE_HEADER = 1,     /* not a gzip member this decoder reads (magic, method, flags, header length, member < 18 bytes) */
    FCZ_INFLATE_BLOCK = 2,      /* a block header zlib rejects (or an incomplete literal/length code: zlib's to judge) */
    FCZ_INFLATE_CODE = 3,       /* invalid code / distance symbol, distance before the start of the text */
    FCZ_INFLATE_SIZE = 4,       /* the text is not text_off[i + 1] - text_off[i] bytes long */
    FCZ_INFLATE_INPUT = 5,      /* the stream runs past the member's end, or bytes are left before the trailer */
    FCZ_INFLATE_CHECK = 6       /* CRC-32 or ISIZE of the trailer do not match */
};
/* Host: exclusive prefix of the text sizes in text_off[n + 1], member i sized from its ISIZE (gemmi estimate_uncompressed_size,
 * lib/gemmi/gz.hpp:25-45). kind (may be NULL = every entry a gzip member): 1 gzip member, 0 plain bytes (size = length). A member
 * shorter than 18 bytes, or whose ISIZE exceeds what DEFLATE can expand its bytes to (1032 : 1), is sized 0 and will be refused. */
int fcz_inflate_sizes(const uint8_t* gz, const uint64_t* gz_off, uint32_t n, const uint8_t* kind, uint64_t* text_off);
/* Device-resident: every pointer a device pointer (kind_dev may be NULL); enqueued on the ctx stream, no synchronisation.
 * text_dev[text_off[i] .. text_off[i + 1]) receives member i's text (kind 0: a copy of its bytes), status_dev[i] its status. */
int fcz_inflate_dev(fcz_ctx* ctx, const uint8_t* gz_dev, const uint64_t* gz_off_dev, uint32_t n, const uint8_t* kind_dev,
                    const uint64_t* text_off_dev, uint8_t* text_dev, int32_t* status_dev);
/* Host-pointer convenience (tests, small callers): members in, text + status out. */
int fcz_inflate(fcz_ctx* ctx, const uint8_t* gz, const uint64_t* gz_off, uint32_t n, const uint8_t* kind, const uint64_t* text_off,
                uint8_t* text, int32_t* status);
/* Structure files as they lie on disk -> batch / FCZ records: fcz_ingest_pdb_begin / fcz_compress_pdb_begin with an inflate stage in
 * front. data = the files' bytes back to back, is_gz[i] != 0: file i is a gzip member (the reference decides by the name's `.gz`,
 * gemmi::MaybeGzipped::is_compressed) -- a fifth of the text's bytes cross the link. The results are fetched with
 * fcz_ingest_pdb_fetch / fcz_compress_pdb_fetch; file_status[i] == FCZ_INGEST_HOST_GZIP: the member was not inflated here (see
 * above), the caller inflates and reads the file itself. */
#define FCZ_INGEST_HOST_GZIP 5
int fcz_ingest_gz_begin(fcz_ctx* ctx, const uint8_t* data, const uint64_t* file_off, uint32_t n_files, const uint8_t* is_gz,
                        const char* names, const uint32_t* name_off, const uint32_t* stem_len, int anchor_threshold, int flags,
                        uint32_t counts[5]);
int fcz_compress_gz_begin(fcz_ctx* ctx, const uint8_t* data, const uint64_t* file_off, uint32_t n_files, const uint8_t* is_gz,
                          const char* names, const uint32_t* name_off, const uint32_t* stem_len, int anchor_threshold, int flags,
                          uint32_t counts[5], uint64_t* fcz_bytes);

/* ---- extract ---------------------------------------------------------------------------------- */
/* Foldcomp::extract (src/foldcomp.cpp:1260-1336) straight from the FCZ bytes, no reconstruction.
 *   mode 0: pLDDT (B-factor) of every residue with `digits` in 1..4 characters ("d", "dd", "dd.d", "dd.dd"; digit rules
 *           :1286-1325), joined by ',' when digits > 1;   mode 1: one-letter amino-acid sequence (digits ignored).
 * data_off[n+1] = exclusive prefix of the data sizes (entries that fail Foldcomp::read's checks: 0 bytes); the caller wraps
 * each string into the FASTA-like / TSV line (writeFASTALike / writeTSV, :1223-1237). */
int fcz_extract_sizes(const uint8_t* blob, const uint64_t* off, uint32_t n, int mode, int digits, uint64_t* data_off);
int fcz_extract(fcz_ctx* ctx, const uint8_t* blob, const uint64_t* off, uint32_t n, int mode, int digits,
                const uint64_t* data_off, uint8_t* data_out);
int fcz_extract_sizes_dev(fcz_ctx* ctx, const uint8_t* blob_dev, const uint64_t* off_dev, uint32_t n, int mode, int digits,
                          uint64_t* data_off_dev);
int fcz_extract_dev(fcz_ctx* ctx, const uint8_t* blob_dev, const uint64_t* off_dev, uint32_t n, int mode, int digits,
                    const uint64_t* data_off_dev, uint8_t* data_dev);

/* ---- check -------------------------------------------------------------------------------- */
/* Foldcomp::checkValidity (src/foldcomp.cpp:1492-1532) on one entry; returns the reference's
 * ValidityError value (0 = SUCCESS .. 6) or a negative fcz_status if the entry cannot be read. */
int fcz_check(const uint8_t* entry, uint64_t len);

/* ---- introspection for benchmarks --------------------------------------------------------- */
/* Accumulated device time (ms, HIP events on the ctx stream) and launch count of the named kernel
 * group since the last reset: "compress_sizes", "compress_index", "compress_angles", "compress_pack",
 * "decompress_sizes", "decompress_backbone", "decompress_index", "decompress_sidechain", "pdb_sizes", "pdb_format", "extract_sizes", "extract",
 * "ingest_parse", "ingest_parse_cif", "ingest_rows_cif", "ingest_frags", "ingest_fill", "inflate", "dense", "undense" (the counting and the fill
 * kernel of fcz_undense_dev: two launches per call), "angles" (fcz_angles_dev), "knn" (fcz_knn_dev and fcz_knn_packed_dev), "lddt" (fcz_lddt_dev and fcz_lddt_packed_dev), "lddt_atoms" (fcz_lddt_atoms_dev and fcz_lddt_atoms_packed_dev), "superpose" (fcz_superpose_dev, fcz_superpose_apply_dev and their packed forms), "tmscore" (fcz_tmscore_dev and fcz_tmscore_packed_dev), "tmalign" (fcz_tmalign_dev and fcz_tmalign_dp_dev), "frames" (fcz_frames_dev). Every other packed or windowed entry point is timed under the
 * group of its padded form: fcz_dense_packed_dev and fcz_dense_window_dev under "dense", fcz_undense_packed_dev under "undense",
 * fcz_angles_packed_dev and fcz_angles_window_dev under "angles". */
int  fcz_ctx_enable_timing(fcz_ctx* ctx, int enable);
int  fcz_ctx_kernel_time(fcz_ctx* ctx, const char* name, double* ms, uint64_t* launches);
void fcz_ctx_reset_timing(fcz_ctx* ctx);

/* ---- diagnostics --------------------------------------------------------------------------- */
/* Device numerics self-test used by tests/test_device_math.py: evaluates one math primitive of the codec (mode 0..13:
 * acos->degrees, glibc sinf / cosf restatements, norm, cosine, NeRF placement, the kernels' paired and any-float sine / cosine ...) on `count` inputs generated from
 * the float bit patterns start_bits, start_bits + stride, ... and copies the float results to out_host. */
int fcz_selftest_math(fcz_ctx* ctx, int mode, uint32_t start_bits, uint32_t stride, uint32_t count, float* out_host);
/* Device copy ceiling used by bench.py beside the 8 TB/s peak: `reps` copies of `bytes` bytes (rounded down to 16) between two
 * scratch buffers by a float4-per-lane grid-stride kernel on a persistent grid (the kernel /opt/skills/guides/MI355X_MICROARCH.md
 * quotes its 6.29 TB/s "float4 copy" with), in a few launch shapes (8 / 16 / 32 blocks per CU, one or four loads in flight per lane,
 * default and non-temporal cache policy); *gb_per_s = the best (read + written bytes) / HIP-event time on the ctx stream. */
int fcz_selftest_copy(fcz_ctx* ctx, uint64_t bytes, int reps, double* gb_per_s);

#ifdef __cplusplus
}
#endif
#endif /* FCZ_HIP_H */
