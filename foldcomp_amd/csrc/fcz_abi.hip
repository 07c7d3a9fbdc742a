// fcz_abi.hip -- C-ABI (include/fcz_hip.h) over the gfx950 kernels. No torch, no C++ types cross the ABI.
// There is deliberately NO CPU fallback in this library: without a HIP device every compute entry
// point returns FCZ_E_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

#include "fcz_kernels.h"
#include "fcz_compress.h"
// persistent grids: blocks per resident slot. Measured (1 M chains): 1 block per slot is 5 % slower than 4, 16 is 3-5 % faster
// than 4 (k_compress_angles_w 17.2 -> 16.4 ms, k_sidechain 16.0 -> 15.5 ms), 64 no better: with more, shorter blocks the
// hardware dispatcher evens out what the CUs finish at different times, and the table prologue is still paid once per ~30+ tiles
#ifndef FCZ_CW_GRID_FACTOR
#define FCZ_CW_GRID_FACTOR 16u
#endif
#ifndef FCZ_SC_GRID_FACTOR
#define FCZ_SC_GRID_FACTOR 16u
#endif
#include "fcz_sidechain.h"
#include "fcz_backbone_fast.h"
#include "fcz_pdb.h"
#include "fcz_extract.h"
#include "fcz_ingest.h"
#include "fcz_ingest_cif.h"
#include "fcz_inflate.h"
#include "fcz_dense.h"
#include "fcz_undense.h"
#include "fcz_knn.h"
#include "fcz_lddt.h"
#include "fcz_lddt_soft.h"
#include "fcz_fape.h"
#include "fcz_fape_atoms.h"
#include "fcz_dssp.h"
#include "fcz_sasa.h"
#include "fcz_violations.h"
#include "fcz_violation_loss.h"
#include "fcz_lddt_atoms.h"
#include "fcz_superpose.h"
#include "fcz_tmscore.h"
#include "fcz_gdt.h"
#include "fcz_tmalign.h"
#include "fcz_frames.h"
#include "fcz_angles.h"

// second, host-side instance of the generated tables (integer metadata for sizes/validation)
namespace host_tab {
#undef FCZ_TABLE_QUAL
#undef FCZ_T
#define FCZ_TABLE_QUAL static const
#define FCZ_T(name) h_##name
#include "aa_tables.inc"
#include "aa_tables_chi.inc"
}  // namespace host_tab

using namespace fcz;

#define HIP_TRY(expr)                                                                     \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess) {                                                           \
            fprintf(stderr, "fcz_hip: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return FCZ_E_HIP;                                                             \
        }                                                                                 \
    } while (0)

namespace {

// a device allocation that only grows; freed with its owner
struct dev_buf {
    void* p = nullptr;
    size_t cap = 0;
    dev_buf() = default;
    dev_buf(const dev_buf&) = delete; dev_buf& operator=(const dev_buf&) = delete;
    ~dev_buf() { if (p) (void)hipFree(p); }
    int ensure(size_t bytes) {
        if (bytes <= cap) return FCZ_OK;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        size_t want = bytes + bytes / 8 + 256;
        if (hipMalloc(&p, want) != hipSuccess) { p = nullptr; return FCZ_E_NOMEM; }
        cap = want;
        return FCZ_OK;
    }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

struct timed_span { std::string name; hipEvent_t a, b; };

// fcz_ctx::pool, the staging of the host-pointer entry points: the names a buffer has, one per role. Roles that share a buffer are
// never live together (table in fcz_ctx). REC_*: uploaded FCZ records (n + 1 u64 offsets), their res_off / atom_off (n + 1 u32) and
// the fcz_atoms_out decoded from them; FILES_*: structure files of an ingest call; BATCH_IN / DENSE_IN / DENSE_OUT: first of the 13
// arrays of a fcz_chain_batch, the 10 of a fcz_dense_in (slot 3, length, holds row_off [n + 1] in the packed form), the 6 of a
// fcz_dense_out in the struct's order, DENSE_CHAIN_INDEX: the chain_index a fcz_packed_out adds to them; ANGLES_OUT: the angles, their mask and
// (windowed form) aatype; WINDOW_START: the n u32 starts of a windowed host call; KEPT_*: the records a *_begin call leaves for its fetch
// (C + 1 u64 offsets, the bytes, C i32 status); LDDT_PRED: pos and mask of the second tensor batch of fcz_lddt, LDDT_OUT: score, pairs, hits
// (fcz_lddt_soft: soft, pairs; fcz_lddt_soft_grad: grad), LDDT_WEIGHT: the row weights of fcz_lddt_soft_grad;
// FAPE_FRAMES: rot, trans, frame_mask of the truth, then of the prediction, of fcz_fape (its pos, mask, bound and weight go through DENSE_IN, LDDT_PRED
// and LDDT_WEIGHT), FAPE_OUT: sum, points (fcz_fape_grad: grad_rot, grad_trans, grad_pos); fcz_fape_atoms uses the same names for its arrays of eight
// groups a row, DENSE_IN + 2 for aatype and FAPEA_SWAPPED for swapped;
// DSSP_OUT: acc_index, acc_energy, don_index, don_energy, ss, ss_mask of fcz_dssp; SASA_POINTS: the directions of fcz_sasa, SASA_OUT: sasa_points, sasa, sasa_mask;
// SUPERPOSE_OUT: the seven arrays of a fcz_superpose_out in the struct's order; APPLY_ROT, APPLY_TRANS, APPLY_OUT: the transforms and the moved
// coordinates of fcz_superpose_apply (its pos and mask go through LDDT_PRED); TM_SEED, TM_SELECTED: the two arrays a fcz_tmscore_out adds to those seven;
// GDT_OUT: the eight arrays of a fcz_gdt_out in the struct's order;
// VIOL_OUT .. VIOL_OUT_LAST: the ten arrays of a fcz_violations_out in the struct's order; VLOSS_WEIGHT: w_clash, w_link of fcz_violation_loss_grad,
// VLOSS_OUT: clash_loss, link_loss, counts of fcz_violation_loss (fcz_violation_loss_grad: grad); LDDTA_OUT: the six of a fcz_lddt_atoms_out;
// TA_SETS: pos, mask, length / row_off of the two fcz_chain_set of fcz_tmalign, TA_PAIRS: its pairs, TA_OUT: the thirteen arrays of a fcz_tmalign_out in the
// struct's order; TA_DP_*: the transforms, map and aligned of fcz_tmalign_dp
enum { REC_BLOB, REC_OFF, REC_RES_OFF, REC_ATOM_OFF, REC_X, REC_Y, REC_Z, REC_BFAC, REC_RES_CODE, REC_ATOM_CODE,
       FILES_TEXT = 0, FILES_OFF, FILES_NAMES, FILES_NAME_OFF, FILES_STEM_LEN, BATCH_IN = 0, DENSE_IN = 0, LDDT_PRED = 4, LDDT_WEIGHT = 6, FAPE_FRAMES = 7, FAPE_OUT = 13, DENSE_OUT = 10, LDDT_OUT = 10, SUPERPOSE_OUT = 10, DSSP_OUT = 10,
       SASA_POINTS = 4, SASA_OUT = 10,
       APPLY_ROT = 10, APPLY_TRANS, APPLY_OUT,
       ANGLES_OUT = 10, KEPT_OFF = 13, KEPT_BYTES, KEPT_STATUS, DENSE_CHAIN_INDEX, WINDOW_START = DENSE_CHAIN_INDEX, TM_SEED, TM_SELECTED,
       FAPEA_SWAPPED = 16,
       VIOL_OUT = 10, VLOSS_WEIGHT = 4, VLOSS_OUT = 10, LDDTA_OUT = 10, GDT_OUT = 10, TA_SETS = 0, TA_PAIRS = 6, TA_OUT = 7, TA_DP_ROT = 7, TA_DP_TRANS, TA_DP_MAP, TA_DP_ALIGNED, VIOL_OUT_LAST = 19, POOL_COUNT };
static_assert(POOL_COUNT == VIOL_OUT_LAST + 1 && DENSE_OUT + 6 == DENSE_CHAIN_INDEX && LDDTA_OUT + 6 <= POOL_COUNT && TM_SELECTED < POOL_COUNT && GDT_OUT + 8 <= POOL_COUNT && TA_OUT + 13 <= POOL_COUNT && TA_SETS + 6 == TA_PAIRS &&
              TA_PAIRS < TA_OUT && TA_DP_ALIGNED < POOL_COUNT && FAPE_FRAMES + 6 == FAPE_OUT && FAPE_OUT + 3 <= FAPEA_SWAPPED && FAPEA_SWAPPED < POOL_COUNT, "the last name of the enum sizes fcz_ctx::pool");

// what the device reports to the host in the middle of a call: one pinned allocation, a member per reader
struct pinned_words {
    sizes_totals sizes;                                                                     // run_entry_sizes (one copy of the device's struct)
    struct { uint32_t chains, residues, atoms, title_bytes, overflow, refused; } ingest;    // fcz_ingest_pdb_dev
    uint64_t record_bytes;                                                                  // compress_resident_batch
    struct { uint32_t residues, atoms, overflow; } undense;                                 // fcz_undense_dev
};

// fcz_ctx::ig, the buffers of the structure ingest: scratch atom table and per-file lists of fcz_ingest_pdb_dev, then (B_OUT_*) the
// arrays of the resident batch, which fcz_ingest_pdb_fetch / fcz_compress_pdb_fetch read until the next ingest call
enum { B_CAP, B_ABASE, B_NAME, B_RESN, B_SERIAL, B_RESSEQ, B_X, B_Y, B_Z, B_B, B_CHAIN, B_ACODE, B_RCODE, B_RFIRST, B_RBFAC, B_RCODE2,
       B_TITLES, B_TLEN, B_NKEPT, B_STATUS, B_FRAGS, B_NFRAGS, B_TOTC, B_TOTR, B_TOTA, B_TOTT, B_USESTEM, B_OFFC, B_OFFR, B_OFFA, B_OFFT,
       B_REFUSED, B_NREF, B_OUT_A, B_OUT_R, B_OUT_C, B_OUT_T, B_CIFROWS, B_COUNT };
// fcz_ctx::ud, the buffers of fcz_undense_dev: per-row words, per-chain counts / verdicts / offsets, then (U_OUT_*) the arrays of
// the resident batch, which fcz_undense_fetch reads until the next undense call
enum { U_ROWS, U_CHAIN, U_OUT_A, U_OUT_R, U_OUT_C, U_COUNT };

}  // namespace

struct fcz_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // scratch of the device entry points: dead when the call that filled it returns, unless it says otherwise
    dev_buf ang;        // compress: 6 x R floats (read once more by fcz_compress_angles)
    dev_buf sizes;      // compress: C x u64
    dev_buf scan_tmp;   // block partials of the device scans
    dev_buf codes;      // decompress: residue codes, one byte per residue at (record offset >> 3) + k (k_entry_sizes -> k_res_index); kept for the sizes memo
    dev_buf res_sc_addr; // compress: residue -> output byte offset of its side-chain torsion bytes
    // one layout per direction, each derived in one place. fcz_compress_batch_dev: [n_tiles] flag per 256-residue tile, [n_tiles] list and
    // [4] count of the tiles left to the block-tile kernel, then one bit per chain (a batch without residues: the bits alone).
    // fcz_decompress_batch_dev: [4] count and [2 x n_tiles] list of the half tiles the first k_sidechain launch leaves to the second
    dev_buf tile_work;
    // decompress: the totals and the length order computed by fcz_decompress_sizes_dev are reused by the
    // fcz_decompress_batch_dev call that follows on the same entries
    struct { const void* blob = nullptr; const void* off = nullptr; uint32_t n = 0; } sizes_key;
    sizes_totals sizes_memo{};
    bool sizes_fresh = false;
    dev_buf cnt;        // decompress: 2 x n u32 counts (residues, atoms) + n i32 status (cnt_status) + n u32 segment info; kept for the sizes memo
    dev_buf fwd;        // decompress: per-group ring of forward atoms (one segment deep)
    dev_buf wring;      // decompress: per-group ring of cos/sin of the segment's torsions
    dev_buf fwd_long, wring_long;   // decompress: the same per (group, segment) for the long chains' split form
    dev_buf bb;         // decompress: blended backbone
    dev_buf len_perm;   // decompress: entries ordered by residue count (n u32) + bucket counters (2 x LEN_BUCKETS + 1); kept for the sizes memo
    dev_buf res_aoff;   // decompress: residue -> first output atom
    dev_buf res_rc;     // decompress: residue -> residue code
    dev_buf res_sc;     // decompress: residue -> its side-chain torsion bytes, 3 x R dwords
    dev_buf sizes_res_off;   // decompress: the res_off of a batch call that has to run its own sizes pass (ensure_sizes)
    dev_buf selftest_out;    // fcz_selftest_math
    dev_buf sweep_tiles;     // the packed form of every per-chain sweep (chain_tiles): n u64 tile counts, then their n + 1 offsets
    dev_buf ta_work;              // fcz_tmalign_dev: two u64, the DPs and DP cells of the last call (fcz_tmalign_last_work)
    dev_buf ta_scratch, ta_dir;   // fcz_tmalign_dev: m u64 item counts, their m + 1 offsets, a double per seed, 2 m u32 site counts; the traceback bits, wa * 256 bytes a resident wavefront
    dev_buf tm_scratch;      // fcz_tmscore_dev / _packed_dev: n u64 item counts, their n + 1 offsets, a double per seed (tm_items_bound), n u32 site counts
    dev_buf gdt_scratch;     // fcz_gdt_dev / _packed_dev: n u64 item counts, their n + 1 offsets, 5 n u64 best words (count << 32 | ~seed), n u32 site counts
    dev_buf dssp_flags;      // fcz_dssp_labels_dev / _packed_dev: a byte per row (k_dssp_flags -> k_dssp_labels)
    dev_buf fast_scratch;    // decompress, FCZ_NUMERICS_FAST: forward atoms of segments longer than one chunk
    // Staging of the host-pointer entry points. Every entry point that writes it calls claim_staging first. Nothing outlives the call
    // that wrote it but KEPT_*, which a begin leaves for its fetch: any later call that writes 13 .. 15 ends that.
    //   entry point                                 writes pool[]                               left for a fetch
    //   fcz_decompress_batch                        REC_* 0 .. 9
    //   fcz_decompress_pdb_begin / _sizes           REC_* 0 .. 8                                (pdb_text, pdb_bytes)
    //   fcz_extract                                 REC_BLOB, REC_OFF
    //   fcz_decompress_dense                        REC_* 0 .. 8, DENSE_OUT 10 .. 15
    //   fcz_decompress_dense_packed                 REC_* 0 .. 8, DENSE_OUT 10 .. 15, DENSE_CHAIN_INDEX 16
    //   fcz_decompress_angles[_packed]              REC_* 0 .. 3, ANGLES_OUT 10 .. 11
    //   fcz_decompress_dense_window                 REC_* 0 .. 8, DENSE_OUT 10 .. 15, WINDOW_START 16
    //   fcz_decompress_angles_window                REC_* 0 .. 3, ANGLES_OUT 10 .. 12, WINDOW_START 16
    //   fcz_compress_batch                          BATCH_IN 0 .. 12, KEPT_* 13 .. 15
    //   fcz_inflate                                 FILES_TEXT
    //   fcz_ingest_pdb_begin / fcz_ingest_gz_begin  FILES_* 0 .. 4 (gz: no FILES_OFF, gz_toff)      (ig[], ig_res, ig_counts)
    //   fcz_compress_pdb_begin / _gz_begin          the same, then KEPT_* 13 .. 15              KEPT_*, ig_fcz_bytes (+ ig[], ig_res)
    //   fcz_compress_dense_begin                    DENSE_IN 0 .. 9, then KEPT_* 13 .. 15       KEPT_*, ud_fcz_bytes (+ ud_batch)
    //   fcz_compress_dense_begin_dev                KEPT_* 13 .. 15                             KEPT_*, ud_fcz_bytes (+ ud_batch)
    //   fcz_compress_dense_packed_begin[_dev]       as the two above (DENSE_IN 3 = row_off)     the same
    //   fcz_knn / fcz_knn_packed                    DENSE_IN 0, 1, 3 (pos, mask, length / row_off), DENSE_OUT 10 .. 11 (index, dist)
    //   fcz_lddt / fcz_lddt_packed                  DENSE_IN 0, 1, 3 (pos_true, mask_true, length / row_off), LDDT_PRED 4 .. 5 (pos_pred, mask_pred), LDDT_OUT 10 .. 12
    //   fcz_lddt_soft / fcz_lddt_soft_packed        the inputs of fcz_lddt, LDDT_OUT 10 .. 11 (soft, pairs)
    //   fcz_lddt_soft_grad / _grad_packed           the inputs of fcz_lddt, LDDT_WEIGHT 6, LDDT_OUT 10 (grad)
    //   fcz_fape / fcz_fape_packed                  the inputs of fcz_lddt, FAPE_FRAMES 7 .. 12, FAPE_OUT 13 .. 14 (sum, points)
    //   fcz_fape_grad / fcz_fape_grad_packed        the same inputs, LDDT_WEIGHT 6, FAPE_OUT 13 .. 15 (grad_rot, grad_trans, grad_pos)
    //   fcz_fape_atoms / _packed / _grad / _grad_packed   as fcz_fape / fcz_fape_grad, and DENSE_IN 2 (aatype), FAPEA_SWAPPED 16
    //   fcz_lddt_atoms / fcz_lddt_atoms_packed      DENSE_IN 0 .. 3 (pos_true, mask_true, aatype, length / row_off), LDDT_PRED 4 .. 5, LDDTA_OUT 10 .. 15
    //   fcz_superpose / fcz_superpose_packed        DENSE_IN 0, 1, 3 and LDDT_PRED 4 .. 5 as fcz_lddt, SUPERPOSE_OUT 10 .. 16
    //   fcz_tmscore / fcz_tmscore_packed            the same, then TM_SEED 17, TM_SELECTED 18
    //   fcz_gdt / fcz_gdt_packed                    DENSE_IN 0, 1, 3 and LDDT_PRED 4 .. 5 as fcz_lddt, GDT_OUT 10 .. 17
    //   fcz_superpose_apply[_packed]                LDDT_PRED 4 .. 5 (pos, mask), DENSE_IN 3 (length / row_off), APPLY_ROT 10, APPLY_TRANS 11, APPLY_OUT 12
    //   fcz_dssp / fcz_dssp_packed                  DENSE_IN 0 .. 3 (pos, mask, aatype, length / row_off), DSSP_OUT 10 .. 15 (the four tables, ss, ss_mask)
    //   fcz_frames                                  DENSE_IN 0 .. 3 (pos, mask, aatype, length), DENSE_OUT 10 .. 12 (rot, trans, frame_mask)
    //   fcz_sasa / fcz_sasa_packed                  DENSE_IN 0 .. 3 (pos, mask, aatype, length / row_off), SASA_POINTS 4, SASA_OUT 10 .. 12 (sasa_points, sasa, sasa_mask)
    //   fcz_violations / fcz_violations_packed      DENSE_IN 0 .. 3 (pos, mask, aatype, length / row_off), VIOL_OUT 10 .. 19 (the arrays of fcz_violations_out)
    //   fcz_violation_loss / _packed                the inputs of fcz_violations, VLOSS_OUT 10 .. 12 (clash_loss, link_loss, counts)
    //   fcz_violation_loss_grad / _grad_packed      the inputs of fcz_violations, VLOSS_WEIGHT 4 .. 5 (w_clash, w_link), VLOSS_OUT 10 (grad)
    //   fcz_tmalign                                 TA_SETS 0 .. 5 (pos, mask, length / row_off of a, then of b), TA_PAIRS 6, TA_OUT 7 .. 19
    //   fcz_tmalign_dp                              TA_SETS 0 .. 5, TA_PAIRS 6, TA_DP_ROT 7, TA_DP_TRANS 8, TA_DP_MAP 9, TA_DP_ALIGNED 10
    dev_buf pool[POOL_COUNT];
    // PDB text / extracted data: per-entry sizes (any call), offsets (n + 1 u64) and the text of the last fcz_decompress_pdb_begin,
    // which fcz_decompress_pdb_fetch reads: live until the next fcz_decompress_pdb_begin / _sizes or fcz_extract
    dev_buf pdb_size, pdb_off, pdb_text;
    uint64_t pdb_bytes = 0;
    pinned_words* pinned = nullptr;
    hipStream_t stream2 = nullptr;   // long chains of a decompress batch run beside the rest
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int n_cu = 256;
    bool timing = false;
    bool keep_first_angle = false;
    int numerics = FCZ_NUMERICS_EXACT;
    // profiling aid (tools/hbm_busy_probe.py): FCZ_PROFILE_STAGES=<mask> in the environment (read at every decompress batch call)
    // leaves out stages of the call so that ONE kernel fills the device for seconds (1 backbone, 2 residue index, 4 side chains;
    // unset = all). The outputs are then stale by construction: never set outside a profiling run.
    unsigned profile_stages = 7u;
    // structure ingest: its buffers, and the resident batch of the last ingest call as pointers into them (live until the next ingest call)
    dev_buf ig[B_COUNT];
    fcz_ingest_result ig_res{};
    uint32_t ig_counts[5] = {0, 0, 0, 0, 0};
    uint64_t ig_fcz_bytes = 0;       // size of KEPT_BYTES after fcz_compress_pdb_begin / _gz_begin
    // inflate in front of the ingest: the files' bytes as they came over the link, their offsets / kinds / text offsets / statuses
    // (fcz_inflate, fcz_ingest_gz_begin: dead when the call returns)
    dev_buf gz_raw, gz_off, gz_kind, gz_toff, gz_status;
    // dense tensors -> batch (fcz_undense.h): its buffers, the resident batch of the last undense call and its per-chain verdicts as
    // pointers into them -- and, for the optional arrays the caller gave, into the caller's (live until the next undense call)
    dev_buf ud[U_COUNT];
    fcz_chain_batch ud_batch{};
    const int32_t* ud_status = nullptr;
    uint64_t ud_fcz_bytes = 0;       // size of KEPT_BYTES after fcz_compress_dense_begin[_dev]
    std::vector<timed_span> spans;
    std::map<std::string, std::pair<double, uint64_t>> acc;
};

namespace {

struct span_guard {
    fcz_ctx* ctx; hipEvent_t a = nullptr, b = nullptr; const char* name;
    span_guard(fcz_ctx* c, const char* n) : ctx(c), name(n) {
        if (ctx->timing) { (void)hipEventCreate(&a); (void)hipEventCreate(&b); (void)hipEventRecord(a, ctx->stream); }
    }
    ~span_guard() {
        if (ctx->timing) { (void)hipEventRecord(b, ctx->stream); ctx->spans.push_back({name, a, b}); }
    }
};

void drain_spans(fcz_ctx* ctx) {
    if (ctx->spans.empty()) return;
    (void)hipStreamSynchronize(ctx->stream);
    for (auto& s : ctx->spans) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) { auto& e = ctx->acc[s.name]; e.first += ms; e.second += 1; }
        (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b);
    }
    ctx->spans.clear();
}

inline unsigned grid_for(uint32_t items, unsigned per_block) { return (items + per_block - 1) / per_block; }

// exclusive scan of n elements into out[n+1] on the ctx stream (three launches, any n)
// overflow (may be null): set to 1 on the device when the total does not fit T
template <class T>
int device_scan(fcz_ctx* ctx, const T* in, T* out, uint32_t n, uint32_t* overflow = nullptr) {
    if (n == 0) { if (hipMemsetAsync(out, 0, sizeof(T), ctx->stream) != hipSuccess) return FCZ_E_HIP; return FCZ_OK; }
    const unsigned nb = grid_for(n, SCAN_CHUNK);
    int rc = ctx->scan_tmp.ensure(sizeof(unsigned long long) * 2 * ((size_t)nb + 1));
    if (rc) return rc;
    unsigned long long* part = ctx->scan_tmp.as<unsigned long long>();
    unsigned long long* part_ex = part + nb + 1;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_scan_reduce<T>), dim3(nb), dim3(1024), 0, ctx->stream, n, in, part);
    hipLaunchKernelGGL(k_scan_u64, dim3(1), dim3(1024), 0, ctx->stream, nb, (const uint64_t*)part, (uint64_t*)part_ex);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_scan_apply<T>), dim3(nb), dim3(1024), 0, ctx->stream, n, in, part_ex, out, overflow);
    return FCZ_OK;
}

// Called by every entry point before it writes fcz_ctx::pool: the sizes memo may be keyed on buffers of the pool (an entry point that
// sized the records it uploaded and decoded none), so it is dropped here and never outlives their contents.
void claim_staging(fcz_ctx* ctx) { ctx->sizes_fresh = false; }

// the arrays every reader of decoded atoms needs (atom_code is optional everywhere, res_code for the decoder that writes them)
bool atoms_out_ok(const fcz_atoms_out* a, bool need_res_code = true) {
    return a && a->x && a->y && a->z && a->bfac_res && (a->res_code || !need_res_code);
}

// per-entry status of the last sizes pass over n entries (cnt: 2 x n counts, then n status words, then n segment words)
int32_t* cnt_status(fcz_ctx* ctx, uint32_t n) { return ctx->cnt.as<int32_t>() + 2 * (size_t)n; }

// f(std::integral_constant<int, A>) for the width A of a dense layout that fcz_dense_width has accepted
template <class F> void dispatch_layout(int layout, F&& f) {
    if (layout == FCZ_DENSE_ATOM37) f(std::integral_constant<int, 37>{});
    else if (layout == FCZ_DENSE_ATOM14) f(std::integral_constant<int, 14>{});
    else f(std::integral_constant<int, 4>{});
}

// f(i, a.member, b.member, bytes) for the 13 arrays of a fcz_chain_batch in the order of BATCH_IN, until one does not return FCZ_OK;
// a and b are batches with the counts of n and TB title bytes
template <class A, class B, class F> int each_batch_array(A& a, B& b, const fcz_chain_batch& n, size_t TB, F f) {
    const size_t C = n.n_chains, R = n.n_residues, M = n.n_atoms;
    int rc;
    if ((rc = f(0, a.res_off, b.res_off, 4 * (C + 1))) || (rc = f(1, a.atom_off, b.atom_off, 4 * (R + 1))) || (rc = f(2, a.x, b.x, 4 * M)) ||
        (rc = f(3, a.y, b.y, 4 * M)) || (rc = f(4, a.z, b.z, 4 * M)) || (rc = f(5, a.atom_code, b.atom_code, M)) || (rc = f(6, a.res_code, b.res_code, R)) ||
        (rc = f(7, a.bfac_ca, b.bfac_ca, 4 * R)) || (rc = f(8, a.first_res_index, b.first_res_index, 4 * C)) ||
        (rc = f(9, a.first_atom_index, b.first_atom_index, 4 * C)) || (rc = f(10, a.chain_id, b.chain_id, C)) || (rc = f(11, a.titles, b.titles, TB)) ||
        (rc = f(12, a.title_off, b.title_off, 4 * (C + 1))))
        return rc;
    return FCZ_OK;
}
// resident batch d -> the host arrays hb names (every array that has an element must be named)
int fetch_batch(fcz_ctx* ctx, const fcz_chain_batch& hb, const fcz_chain_batch& d, size_t TB) {
    return each_batch_array(hb, d, d, TB, [&](int, auto* dst, auto* src, size_t bytes) -> int {
        if (!bytes) return FCZ_OK;
        if (!dst) return FCZ_E_INVALID_ARG;
        HIP_TRY(hipMemcpyAsync(const_cast<void*>((const void*)dst), src, bytes, hipMemcpyDeviceToHost, ctx->stream));
        return FCZ_OK;
    });
}

// the resident records of the last *_begin call (C chains, n_bytes) -> out_off[C + 1], status[C] (either may be null), blob; kind: to the host or the device
int fetch_resident(fcz_ctx* ctx, uint32_t C, uint64_t n_bytes, uint64_t* out_off, int32_t* status, uint8_t* blob, hipMemcpyKind kind) {
    if (C) {
        if (out_off) HIP_TRY(hipMemcpyAsync(out_off, ctx->pool[KEPT_OFF].p, 8 * ((size_t)C + 1), kind, ctx->stream));
        if (status) HIP_TRY(hipMemcpyAsync(status, ctx->pool[KEPT_STATUS].p, 4 * (size_t)C, kind, ctx->stream));
        if (n_bytes) {
            if (!blob) return FCZ_E_INVALID_ARG;
            HIP_TRY(hipMemcpyAsync(blob, ctx->pool[KEPT_BYTES].p, n_bytes, kind, ctx->stream));
        }
    } else if (out_off) {
        if (kind == hipMemcpyDeviceToHost) out_off[0] = 0; else HIP_TRY(hipMemsetAsync(out_off, 0, 8, ctx->stream));
    }
    return FCZ_OK;
}

// An array of a host-pointer call: the caller's pointer (NULL: an input that is absent, an output that is not wanted), its bytes, and
// the slot of fcz_ctx::pool it goes through (table in fcz_ctx).
struct staged_in { const void* host; size_t bytes; int slot; };
struct staged_out { void* host; size_t bytes; int slot; };
constexpr int STAGED_MAX = 14;

// The three steps of staging, for the rules below. Room for every input, then their upload; dev[] gets the device pointers in the
// list's order. floor: what a present array is given at least (fcz_compress_dense_begin).
int stage_in(fcz_ctx* ctx, std::initializer_list<staged_in> in, const void** dev, size_t floor = 0) {
    int rc, i = 0;
    for (const staged_in& a : in) {
        const size_t nb = a.host ? std::max(a.bytes, floor) : 0;
        if ((rc = ctx->pool[a.slot].ensure(nb))) return rc;
        dev[i++] = nb ? ctx->pool[a.slot].p : nullptr;
    }
    for (const staged_in& a : in)
        if (a.host && a.bytes) HIP_TRY(hipMemcpyAsync(ctx->pool[a.slot].p, a.host, a.bytes, hipMemcpyHostToDevice, ctx->stream));
    return FCZ_OK;
}
// room for every wanted output; dev[] gets the device pointers in the list's order
int reserve_out(fcz_ctx* ctx, std::initializer_list<staged_out> out, void** dev) {
    int rc, i = 0;
    for (const staged_out& o : out) {
        if ((rc = ctx->pool[o.slot].ensure(o.host ? o.bytes : 0))) return rc;
        dev[i++] = o.host ? ctx->pool[o.slot].p : nullptr;
    }
    return FCZ_OK;
}
// the wanted outputs back to the caller (enqueued: the caller drains the stream)
int fetch_out(fcz_ctx* ctx, std::initializer_list<staged_out> out) {
    for (const staged_out& o : out)
        if (o.host && o.bytes) HIP_TRY(hipMemcpyAsync(o.host, ctx->pool[o.slot].p, o.bytes, hipMemcpyDeviceToHost, ctx->stream));
    return FCZ_OK;
}

// The host-pointer form of an analysis: its inputs to the device, run(in, out) on the device pointers in the order of the lists (it
// enqueues the *_rows call), the outputs back, and the stream drained. The host forms of the record decode put the same three steps
// behind a preamble of their own (the sizes pass, which decides what there is to write) and say where they differ. One set of rules:
//   * A call whose wanted outputs have no byte returns FCZ_OK with nothing enqueued: there is nothing it could write. That is rows == 0
//     for the per-row analyses, and rows == 0 with n == 0 for violations, superpose and TM-score: they have per-chain outputs, so chains
//     without a row (packed, R == 0) go on and get the counters and the transform of an empty chain.
//   * An array of zero bytes is not copied, in either direction: hipMemcpyAsync is given no NULL or unallocated pointer.
//   * An input that is absent or has zero bytes reaches run() as NULL. Absent is what the *_rows functions take NULL to mean (no
//     length, no aatype, no second mask); of a zero-byte array no kernel reads an element -- every chain is clamped to the rows that
//     exist and a launch without chains (n == 0: the fill kernels) reads no per-chain array such as the transforms of apply.
//   * An output that is not wanted reaches run() as NULL, which is what the optional members of the out structs mean.
//   * Every buffer is made large enough before the first copy is enqueued, so FCZ_E_NOMEM leaves nothing in flight.
template <class Run>
int staged_call(fcz_ctx* ctx, std::initializer_list<staged_in> in, std::initializer_list<staged_out> out, Run run) {
    HIP_TRY(hipSetDevice(ctx->device));
    claim_staging(ctx);
    size_t wanted = 0;
    for (const staged_out& o : out) wanted += o.host ? o.bytes : 0;
    if (wanted == 0) return FCZ_OK;
    const void* din[STAGED_MAX]; void* dout[STAGED_MAX];
    int rc;
    if ((rc = reserve_out(ctx, out, dout)) || (rc = stage_in(ctx, in, din)) || (rc = run(din, dout)) || (rc = fetch_out(ctx, out))) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return FCZ_OK;
}

// the rows a dense or an angle call writes: n x L, n x L from the entry's start on, or the R residues back to back
enum rows_form { ROWS_PADDED, ROWS_WINDOW, ROWS_PACKED };

// per-entry byte counts into ctx->pdb_size by launch(sizes), which is not called for n == 0, then their exclusive prefix into off_dev[n + 1]
template <class Launch> int sizes_then_scan(fcz_ctx* ctx, uint32_t n, const char* span, uint64_t* off_dev, Launch launch) {
    HIP_TRY(hipSetDevice(ctx->device));
    int rc = ctx->pdb_size.ensure(sizeof(uint64_t) * (size_t)std::max<uint32_t>(n, 1)); if (rc) return rc;
    span_guard g(ctx, span);
    if (n) launch(ctx->pdb_size.as<uint64_t>());
    if ((rc = device_scan<uint64_t>(ctx, ctx->pdb_size.as<uint64_t>(), off_dev, n))) return rc;
    HIP_TRY(hipGetLastError());
    return FCZ_OK;
}

}  // namespace

extern "C" {

const char* fcz_status_string(int s) {
    switch (s) {
        case FCZ_OK: return "ok";
        case FCZ_E_INVALID_ARG: return "invalid argument";
        case FCZ_E_NO_DEVICE: return "no HIP device (libfcz_hip has no CPU fallback)";
        case FCZ_E_HIP: return "HIP runtime error";
        case FCZ_E_BAD_MAGIC: return "not an FCZ entry (bad magic)";
        case FCZ_E_TRUNCATED: return "truncated or inconsistent FCZ entry";
        case FCZ_E_RESIDUE: return "residue code not supported by the codec";
        case FCZ_E_TOO_SHORT: return "chain shorter than 2 residues";
        case FCZ_E_NOMEM: return "out of device memory";
        case FCZ_E_NONFINITE: return "a coordinate or B-factor of the chain is not a finite number";
        default: return "unknown status";
    }
}

const char* fcz_atom_code_name(int code) {
    if (code < 0 || code >= FCZ_N_ATOM_CODES) return nullptr;
    return host_tab::h_atom_name[code];
}
int fcz_atom_code_from_name(const char* name) {
    for (int i = 0; i < FCZ_N_ATOM_CODES; i++) if (strcmp(host_tab::h_atom_name[i], name) == 0) return i;
    return FCZ_ATOM_CODE_OTHER;
}
int fcz_res_code_from_name(const char* n3) {
    for (int i = 0; i < FCZ_N_RES_CODES; i++)
        if (strcmp(host_tab::h_res3[i], n3) == 0) return (i < 20 || i == 23) ? i : -1;
    return -1;
}
const char* fcz_res_code_name(int rc) { return (rc >= 0 && rc < FCZ_N_RES_CODES) ? host_tab::h_res3[rc] : "UNK"; }
int fcz_res_code_natoms(int rc) { return (rc >= 0 && rc < FCZ_N_RES_CODES) ? host_tab::h_res_natoms[rc] : 3; }
int fcz_res_code_atom(int rc, int j, int alt) {
    if (rc < 0 || rc >= FCZ_N_RES_CODES) rc = 23;
    if (j < 0 || j >= host_tab::h_res_natoms[rc]) return FCZ_ATOM_CODE_OTHER;
    int slot = alt ? host_tab::h_res_alt_slot[rc][j] : j;
    return host_tab::h_res_atom[rc][slot];
}

int fcz_device_count(void) { int n = 0; return hipGetDeviceCount(&n) == hipSuccess ? n : 0; }
void* fcz_pinned_alloc(size_t bytes) { void* p = nullptr; return hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) == hipSuccess ? p : nullptr; }
void fcz_pinned_free(void* p) { if (p) (void)hipHostFree(p); }

void fcz_ctx_destroy(fcz_ctx* c);
int fcz_ctx_create(int device, fcz_ctx** out) {
    if (!out) return FCZ_E_INVALID_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return FCZ_E_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return FCZ_E_NO_DEVICE;
    fcz_ctx* c = new fcz_ctx();
    c->device = device;
    hipDeviceProp_t prop;
    c->n_cu = (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return FCZ_E_HIP; }
    if (hipHostMalloc((void**)&c->pinned, sizeof(pinned_words), hipHostMallocDefault) != hipSuccess) { (void)hipStreamDestroy(c->stream); delete c; return FCZ_E_HIP; }
    if (hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess) { fcz_ctx_destroy(c); return FCZ_E_HIP; }
    *out = c;
    return FCZ_OK;
}

void fcz_ctx_destroy(fcz_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    drain_spans(c);
    (void)hipStreamSynchronize(c->stream);
    if (c->stream2) (void)hipStreamSynchronize(c->stream2);
    if (c->pinned) (void)hipHostFree(c->pinned);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->stream2) (void)hipStreamDestroy(c->stream2);
    (void)hipStreamDestroy(c->stream);
    delete c;                                   // the device buffers go with it
}

void* fcz_ctx_stream(fcz_ctx* c) { return c ? (void*)c->stream : nullptr; }
int fcz_ctx_set_numerics(fcz_ctx* c, int mode) {
    if (!c || (mode != FCZ_NUMERICS_EXACT && mode != FCZ_NUMERICS_FAST)) return FCZ_E_INVALID_ARG;
    c->numerics = mode;
    return FCZ_OK;
}
int fcz_ctx_get_numerics(fcz_ctx* c) { return c ? c->numerics : FCZ_E_INVALID_ARG; }
int fcz_ctx_synchronize(fcz_ctx* c) {
    if (!c) return FCZ_E_INVALID_ARG;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FCZ_OK;
}
// ------------------------------------------------------------------------------------------------
// PDB text of decompressed chains (writeAtomCoordinatesToPDB, reference src/atom_coordinate.cpp:220-291)
// ------------------------------------------------------------------------------------------------
static int pdb_sizes_impl(fcz_ctx* ctx, const uint8_t* blob_dev, const uint64_t* off_dev, uint32_t n, const uint32_t* res_off_dev,
                          const uint32_t* atom_off_dev, const fcz_atoms_out* atoms_dev, uint32_t pad, uint64_t* text_off_dev) {
    if (!ctx || !blob_dev || !off_dev || !res_off_dev || !atom_off_dev || !atoms_out_ok(atoms_dev) || !text_off_dev) return FCZ_E_INVALID_ARG;
    return sizes_then_scan(ctx, n, "pdb_sizes", text_off_dev, [&](uint64_t* sizes) {
        hipLaunchKernelGGL(k_pdb_sizes, dim3(grid_for(n, WAVES_PER_BLOCK)), dim3(BLOCK), 0, ctx->stream, blob_dev, off_dev, n, res_off_dev, atom_off_dev,
                           *atoms_dev, pad, sizes);
    });
}
int fcz_pdb_sizes_dev(fcz_ctx* ctx, const uint8_t* blob_dev, const uint64_t* off_dev, uint32_t n, const uint32_t* res_off_dev,
                      const uint32_t* atom_off_dev, const fcz_atoms_out* atoms_dev, uint64_t* text_off_dev) {
    return pdb_sizes_impl(ctx, blob_dev, off_dev, n, res_off_dev, atom_off_dev, atoms_dev, 0, text_off_dev);
}

int fcz_pdb_format_dev(fcz_ctx* ctx, const uint8_t* blob_dev, const uint64_t* off_dev, uint32_t n, const uint32_t* res_off_dev,
                       const uint32_t* atom_off_dev, const fcz_atoms_out* atoms_dev, int alt_order, const uint64_t* text_off_dev,
                       uint8_t* text_dev) {
    if (!ctx || !blob_dev || !off_dev || !res_off_dev || !atom_off_dev || !atoms_out_ok(atoms_dev) || !text_off_dev || !text_dev) return FCZ_E_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    if (n == 0) return FCZ_OK;
    span_guard g(ctx, "pdb_format");
    hipLaunchKernelGGL(k_pdb_format, dim3(grid_for(n, WAVES_PER_BLOCK)), dim3(BLOCK), 0, ctx->stream, blob_dev, off_dev, n, res_off_dev,
                       atom_off_dev, *atoms_dev, alt_order, text_off_dev, text_dev);
    HIP_TRY(hipGetLastError());
    return FCZ_OK;
}

// The records of a host-pointer call -> pool[REC_BLOB], [REC_OFF]; with R and M also the sizes pass over them into [REC_RES_OFF] /
// [REC_ATOM_OFF] (*R residues, *M atoms, the per-entry status at cnt_status()) ...
static int upload_records(fcz_ctx* ctx, const uint8_t* blob, const uint64_t* off, uint32_t n, uint32_t* R = nullptr, uint32_t* M = nullptr) {
    int rc;
    if ((rc = ctx->pool[REC_BLOB].ensure(std::max<uint64_t>(off[n], 16))) || (rc = ctx->pool[REC_OFF].ensure(sizeof(uint64_t) * ((size_t)n + 1)))) return rc;
    if (R && ((rc = ctx->pool[REC_RES_OFF].ensure(sizeof(uint32_t) * ((size_t)n + 1))) || (rc = ctx->pool[REC_ATOM_OFF].ensure(sizeof(uint32_t) * ((size_t)n + 1))))) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->pool[REC_BLOB].p, blob, off[n], hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->pool[REC_OFF].p, off, sizeof(uint64_t) * ((size_t)n + 1), hipMemcpyHostToDevice, ctx->stream));
    if (!R) return FCZ_OK;
    return fcz_decompress_sizes_dev(ctx, ctx->pool[REC_BLOB].as<uint8_t>(), ctx->pool[REC_OFF].as<uint64_t>(), n, ctx->pool[REC_RES_OFF].as<uint32_t>(),
                                    ctx->pool[REC_ATOM_OFF].as<uint32_t>(), R, M);
}
// ... the fcz_atoms_out of R residues and M atoms staged beside them ...
static int stage_atoms(fcz_ctx* ctx, uint32_t R, uint32_t M, bool atom_code, fcz_atoms_out* dv) {
    int rc;
    for (dev_buf* b : {&ctx->pool[REC_X], &ctx->pool[REC_Y], &ctx->pool[REC_Z]}) if ((rc = b->ensure(std::max<size_t>(sizeof(float) * (size_t)M, 16)))) return rc;
    if ((rc = ctx->pool[REC_BFAC].ensure(std::max<size_t>(sizeof(float) * (size_t)R, 16))) || (rc = ctx->pool[REC_RES_CODE].ensure(std::max<size_t>((size_t)R, 16)))) return rc;
    if (atom_code && (rc = ctx->pool[REC_ATOM_CODE].ensure(std::max<size_t>((size_t)M, 16)))) return rc;
    *dv = {ctx->pool[REC_X].as<float>(), ctx->pool[REC_Y].as<float>(), ctx->pool[REC_Z].as<float>(), ctx->pool[REC_BFAC].as<float>(), ctx->pool[REC_RES_CODE].as<uint8_t>(),
           atom_code ? ctx->pool[REC_ATOM_CODE].as<uint8_t>() : nullptr};
    return FCZ_OK;
}
// ... and the decode into them
static int decode_records(fcz_ctx* ctx, uint32_t n, int alt_order, const fcz_atoms_out* dv) {
    return fcz_decompress_batch_dev(ctx, ctx->pool[REC_BLOB].as<uint8_t>(), ctx->pool[REC_OFF].as<uint64_t>(), n, ctx->pool[REC_RES_OFF].as<uint32_t>(),
                                    ctx->pool[REC_ATOM_OFF].as<uint32_t>(), alt_order, dv);
}

// What the host forms that size what they upload begin with: the records and the sizes pass over them (upload_records: *R residues,
// *M atoms), the per-entry status into the caller's array (may be NULL), res_off [n + 1] into res_off -- NULL: into a vector of its
// own when *longest, the residues of the longest entry, is asked for (may be NULL), else not at all -- and the stream drained.
static int upload_sized(fcz_ctx* ctx, const uint8_t* blob, const uint64_t* off, uint32_t n, int32_t* status, uint32_t* res_off, uint32_t* R, uint32_t* M,
                        uint32_t* longest = nullptr) {
    int rc = upload_records(ctx, blob, off, n, R, M); if (rc) return rc;
    std::vector<uint32_t> own(res_off || !longest ? 0 : (size_t)n + 1);
    if (!res_off && longest) res_off = own.data();
    if (res_off) HIP_TRY(hipMemcpyAsync(res_off, ctx->pool[REC_RES_OFF].p, sizeof(uint32_t) * ((size_t)n + 1), hipMemcpyDeviceToHost, ctx->stream));
    if (status) HIP_TRY(hipMemcpyAsync(status, cnt_status(ctx, n), sizeof(int32_t) * n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (longest) { *longest = 0; for (uint32_t i = 0; i < n; i++) *longest = std::max(*longest, res_off[i + 1] - res_off[i]); }
    return FCZ_OK;
}

// Host-pointer convenience: FCZ entries in, PDB text out, everything in between on the device. begin() leaves the text in
// the ctx and reports the per-entry text offsets; fetch() copies it out.
static int pdb_begin_impl(fcz_ctx* ctx, const uint8_t* blob, const uint64_t* off, uint32_t n, int alt_order, uint64_t* text_off,
                          int32_t* status, bool format) {
    if (!ctx || !blob || !off || !text_off) return FCZ_E_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    claim_staging(ctx);
    const uint32_t pad = (alt_order & FCZ_PDB_NUL_TERMINATED) ? 1u : 0u;   // every entry followed by one NUL (a database record)
    alt_order &= FCZ_PDB_ALT_ORDER;
    ctx->pdb_bytes = 0;
    if (n == 0) { text_off[0] = 0; return FCZ_OK; }
    uint32_t R = 0, M = 0;
    int rc = upload_sized(ctx, blob, off, n, status, nullptr, &R, &M); if (rc) return rc;
    fcz_atoms_out dv;
    if ((rc = stage_atoms(ctx, R, M, false, &dv))) return rc;
    if ((rc = ctx->pdb_off.ensure(sizeof(uint64_t) * ((size_t)n + 1)))) return rc;
    if (R && (rc = decode_records(ctx, n, alt_order, &dv))) return rc;
    rc = pdb_sizes_impl(ctx, ctx->pool[REC_BLOB].as<uint8_t>(), ctx->pool[REC_OFF].as<uint64_t>(), n, ctx->pool[REC_RES_OFF].as<uint32_t>(),
                        ctx->pool[REC_ATOM_OFF].as<uint32_t>(), &dv, pad, ctx->pdb_off.as<uint64_t>());
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(text_off, ctx->pdb_off.p, sizeof(uint64_t) * ((size_t)n + 1), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (!format) return FCZ_OK;           // sizes only: nothing is kept for a fetch
    ctx->pdb_bytes = text_off[n];
    if ((rc = ctx->pdb_text.ensure(std::max<uint64_t>(ctx->pdb_bytes, 16)))) return rc;
    if (pad && ctx->pdb_bytes) HIP_TRY(hipMemsetAsync(ctx->pdb_text.p, 0, ctx->pdb_bytes, ctx->stream));   // the terminators: the format pass writes the text around them
    return fcz_pdb_format_dev(ctx, ctx->pool[REC_BLOB].as<uint8_t>(), ctx->pool[REC_OFF].as<uint64_t>(), n, ctx->pool[REC_RES_OFF].as<uint32_t>(),
                              ctx->pool[REC_ATOM_OFF].as<uint32_t>(), &dv, alt_order, ctx->pdb_off.as<uint64_t>(), ctx->pdb_text.as<uint8_t>());
}

int fcz_decompress_pdb_begin(fcz_ctx* ctx, const uint8_t* blob, const uint64_t* off, uint32_t n, int alt_order, uint64_t* text_off,
                             int32_t* status) {
    return pdb_begin_impl(ctx, blob, off, n, alt_order, text_off, status, true);
}

int fcz_decompress_pdb_sizes(fcz_ctx* ctx, const uint8_t* blob, const uint64_t* off, uint32_t n, int alt_order, uint64_t* text_off,
                             int32_t* status) {
    return pdb_begin_impl(ctx, blob, off, n, alt_order, text_off, status, false);
}

int fcz_decompress_pdb_fetch(fcz_ctx* ctx, uint8_t* text_out) {
    if (!ctx || (!text_out && ctx->pdb_bytes)) return FCZ_E_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    if (ctx->pdb_bytes) HIP_TRY(hipMemcpyAsync(text_out, ctx->pdb_text.p, ctx->pdb_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return FCZ_OK;
}

// ------------------------------------------------------------------------------------------------
// extract (Foldcomp::extract, reference src/foldcomp.cpp:1260-1336)
// ------------------------------------------------------------------------------------------------
static inline int extract_args_ok(int mode, int digits) { return (mode == 0 && digits >= 1 && digits <= 4) || mode == 1; }

int fcz_extract_sizes(const uint8_t* blob, const uint64_t* off, uint32_t n, int mode, int digits, uint64_t* data_off) {
    if (!blob || !off || !data_off || !extract_args_ok(mode, digits)) return FCZ_E_INVALID_ARG;
    data_off[0] = 0;
    for (uint32_t i = 0; i < n; i++)
        data_off[i + 1] = data_off[i] + extract_bytes(extract_entry_residues(blob + off[i], off[i + 1] - off[i]), mode, digits);
    return FCZ_OK;
}

int fcz_extract_sizes_dev(fcz_ctx* ctx, const uint8_t* blob_dev, const uint64_t* off_dev, uint32_t n, int mode, int digits,
                          uint64_t* data_off_dev) {
    if (!ctx || !blob_dev || !off_dev || !data_off_dev || !extract_args_ok(mode, digits)) return FCZ_E_INVALID_ARG;
    return sizes_then_scan(ctx, n, "extract_sizes", data_off_dev, [&](uint64_t* sizes) {
        hipLaunchKernelGGL(k_extract_sizes, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, ctx->stream, blob_dev, off_dev, n, mode, digits, sizes);
    });
}

int fcz_extract_dev(fcz_ctx* ctx, const uint8_t* blob_dev, const uint64_t* off_dev, uint32_t n, int mode, int digits,
                    const uint64_t* data_off_dev, uint8_t* data_dev) {
    if (!ctx || !blob_dev || !off_dev || !data_off_dev || !data_dev || !extract_args_ok(mode, digits)) return FCZ_E_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    if (n == 0) return FCZ_OK;
    span_guard g(ctx, "extract");
    hipLaunchKernelGGL(k_extract, dim3(grid_for(n, WAVES_PER_BLOCK)), dim3(BLOCK), 0, ctx->stream, blob_dev, off_dev, n, mode, digits,
                       data_off_dev, data_dev);
    HIP_TRY(hipGetLastError());
    return FCZ_OK;
}

int fcz_extract(fcz_ctx* ctx, const uint8_t* blob, const uint64_t* off, uint32_t n, int mode, int digits, const uint64_t* data_off,
                uint8_t* data_out) {
    if (!ctx || !blob || !off || !data_off || !extract_args_ok(mode, digits)) return FCZ_E_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    if (n == 0 || data_off[n] == 0) return FCZ_OK;
    if (!data_out) return FCZ_E_INVALID_ARG;
    claim_staging(ctx);
    const uint64_t data_bytes = data_off[n];
    int rc = ctx->pdb_off.ensure(sizeof(uint64_t) * ((size_t)n + 1)); if (rc) return rc;
    if ((rc = ctx->pdb_text.ensure(std::max<uint64_t>(data_bytes, 16)))) return rc;
    if ((rc = upload_records(ctx, blob, off, n))) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->pdb_off.p, data_off, sizeof(uint64_t) * ((size_t)n + 1), hipMemcpyHostToDevice, ctx->stream));
    rc = fcz_extract_dev(ctx, ctx->pool[REC_BLOB].as<uint8_t>(), ctx->pool[REC_OFF].as<uint64_t>(), n, mode, digits, ctx->pdb_off.as<uint64_t>(),
                         ctx->pdb_text.as<uint8_t>());
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(data_out, ctx->pdb_text.p, data_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return FCZ_OK;
}

int fcz_ctx_enable_timing(fcz_ctx* c, int enable) { if (!c) return FCZ_E_INVALID_ARG; drain_spans(c); c->timing = enable != 0; return FCZ_OK; }
void fcz_ctx_reset_timing(fcz_ctx* c) { if (!c) return; drain_spans(c); c->acc.clear(); }
int fcz_ctx_kernel_time(fcz_ctx* c, const char* name, double* ms, uint64_t* launches) {
    if (!c || !name) return FCZ_E_INVALID_ARG;
    drain_spans(c);
    auto it = c->acc.find(name);
    if (ms) *ms = it == c->acc.end() ? 0.0 : it->second.first;
    if (launches) *launches = it == c->acc.end() ? 0 : it->second.second;
    return FCZ_OK;
}

// ------------------------------------------------------------------------------------------------
// compress
// ------------------------------------------------------------------------------------------------
int fcz_compress_sizes(const fcz_chain_batch* in, uint64_t* out_off) {
    if (!in || !out_off || in->anchor_threshold <= 0) return FCZ_E_INVALID_ARG;
    uint64_t o = 0;
    for (uint32_t c = 0; c < in->n_chains; c++) {
        out_off[c] = o;
        const uint32_t r0 = in->res_off[c], n = in->res_off[c + 1] - r0;
        uint32_t nsc = 0;
        for (uint32_t k = 0; k < n; k++) { uint32_t rc = in->res_code[r0 + k]; nsc += host_tab::h_res_natoms[rc < 24 ? rc : 23] - 3; }
        o += make_layout(n, n / (uint32_t)in->anchor_threshold + 2, in->title_off[c + 1] - in->title_off[c], nsc).size;
    }
    out_off[in->n_chains] = o;
    return FCZ_OK;
}

int fcz_compress_sizes_dev(fcz_ctx* ctx, const fcz_chain_batch* in, uint64_t* out_off_dev) {
    if (!ctx || !in || !out_off_dev || in->anchor_threshold <= 0) return FCZ_E_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    if (in->n_chains == 0) { HIP_TRY(hipMemsetAsync(out_off_dev, 0, sizeof(uint64_t), ctx->stream)); return FCZ_OK; }
    int rc = ctx->sizes.ensure(sizeof(uint64_t) * (size_t)in->n_chains);
    if (rc) return rc;
    span_guard g(ctx, "compress_sizes");
    hipLaunchKernelGGL(k_compress_sizes, dim3(grid_for(in->n_chains, GROUPS_PER_BLOCK)), dim3(BLOCK), 0, ctx->stream, *in, ctx->sizes.as<uint64_t>());
    rc = device_scan<uint64_t>(ctx, ctx->sizes.as<uint64_t>(), out_off_dev, in->n_chains);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return FCZ_OK;
}

int fcz_compress_batch_dev(fcz_ctx* ctx, const fcz_chain_batch* in, const uint64_t* out_off_dev, uint8_t* out_dev,
                           int32_t* status_dev) {
    if (!ctx || !in || !out_off_dev || !out_dev) return FCZ_E_INVALID_ARG;
    if (in->anchor_threshold <= 0) return FCZ_E_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    if (in->n_chains == 0) return FCZ_OK;
    int rc = ctx->ang.ensure(sizeof(float) * 6 * (size_t)std::max<uint32_t>(in->n_residues, 1));
    if (rc) return rc;
    rc = ctx->res_sc_addr.ensure(sizeof(uint64_t) * (size_t)std::max<uint32_t>(in->n_residues, 1));
    if (rc) return rc;
    const dim3 per_chain(grid_for(in->n_chains, WAVES_PER_BLOCK));
    {
        span_guard g(ctx, "compress_index");
        hipLaunchKernelGGL(k_compress_index, dim3(grid_for(in->n_chains, GROUPS_PER_BLOCK)), dim3(BLOCK), 0, ctx->stream, *in, out_off_dev, ctx->res_sc_addr.as<uint64_t>());
    }
    const size_t nf_words = ((size_t)in->n_chains + 31) / 32;
    uint32_t* nonfinite = nullptr;         // one bit per chain: a named atom with a NaN / infinite coordinate (set by the angle kernels)
    if (in->n_residues) {
        // wavefront-private tiles first; what does not fit them (atom-rich stretches, the tail of the arrays) is listed per
        // 256-residue tile and taken by the block-tile kernel, which handles every special case
        span_guard g(ctx, "compress_angles");
        const uint32_t n_tiles = grid_for(in->n_residues, CK_TILE);
        const uint32_t n_wtiles = grid_for(in->n_residues, CW_RES);
        rc = ctx->tile_work.ensure(sizeof(uint32_t) * (2 * (size_t)n_tiles + 4 + nf_words)); if (rc) return rc;
        uint32_t* flags = ctx->tile_work.as<uint32_t>(); uint32_t* list = flags + n_tiles; uint32_t* count = list + n_tiles;
        nonfinite = count + 4;
        HIP_TRY(hipMemsetAsync(flags, 0, sizeof(uint32_t) * (2 * (size_t)n_tiles + 4 + nf_words), ctx->stream));
        const uint32_t blocks_w = std::min<uint32_t>(grid_for(n_wtiles, WAVES_PER_BLOCK), (uint32_t)ctx->n_cu * 3u * FCZ_CW_GRID_FACTOR);
        hipLaunchKernelGGL(k_compress_angles_w, dim3(blocks_w), dim3(BLOCK), 0, ctx->stream, *in, n_wtiles, ctx->res_sc_addr.as<uint64_t>(), out_dev,
                           ctx->ang.as<float>(), flags, list, count, nonfinite);
        const uint32_t blocks = std::min<uint32_t>(n_tiles, (uint32_t)ctx->n_cu * FCZ_COMPRESS_MIN_BLOCKS);
        hipLaunchKernelGGL(k_compress_angles, dim3(blocks), dim3(BLOCK), 0, ctx->stream, *in, n_tiles, (const uint32_t*)list, (const uint32_t*)count,
                           ctx->res_sc_addr.as<uint64_t>(), out_dev, ctx->ang.as<float>(), nonfinite);
    } else {
        rc = ctx->tile_work.ensure(sizeof(uint32_t) * (4 + nf_words)); if (rc) return rc;
        nonfinite = ctx->tile_work.as<uint32_t>();
        HIP_TRY(hipMemsetAsync(nonfinite, 0, sizeof(uint32_t) * nf_words, ctx->stream));
    }
    {
        span_guard g(ctx, "compress_pack");
        auto pack = [&](auto kernel, dim3 grid) {
            hipLaunchKernelGGL(kernel, grid, dim3(BLOCK), 0, ctx->stream, *in, out_off_dev, out_dev, status_dev, ctx->ang.as<float>(),
                               ctx->keep_first_angle ? 1 : 0, (const uint32_t*)nonfinite);
        };
        pack(k_compress_pack, per_chain);
        // chains of 2 .. 128 residues (k_compress_pack leaves them): four to a wavefront, a persistent grid over chunks of 16 chains
        // (one launch per length class -- 2..16, 17..32, 33..64, 65..128 residues in 1, 2, 4, 8 rounds of 16 -- each a scan of the chunks' lengths)
        const dim3 rows_blocks(std::min<uint32_t>(grid_for(grid_for(in->n_chains, CP_CHUNK), WAVES_PER_BLOCK), (uint32_t)ctx->n_cu * 4u));
        // (every class launch is tied to the bound k_compress_pack skips by: a build with fewer rounds must not run a class twice)
        static_assert(FCZ_PACK_ROWS_MAX_ROUNDS == 1 || FCZ_PACK_ROWS_MAX_ROUNDS == 2 || FCZ_PACK_ROWS_MAX_ROUNDS == 4 || FCZ_PACK_ROWS_MAX_ROUNDS == 8,
                      "k_compress_pack_rows has the classes of 1, 2, 4 and 8 rounds");
        pack(HIP_KERNEL_NAME(k_compress_pack_rows<1>), rows_blocks);
#if FCZ_PACK_ROWS_MAX_ROUNDS >= 2
        pack(HIP_KERNEL_NAME(k_compress_pack_rows<2>), rows_blocks);
#endif
#if FCZ_PACK_ROWS_MAX_ROUNDS >= 4
        pack(HIP_KERNEL_NAME(k_compress_pack_rows<4>), rows_blocks);
#endif
#if FCZ_PACK_ROWS_MAX_ROUNDS >= 8
        pack(HIP_KERNEL_NAME(k_compress_pack_rows<8>), rows_blocks);
#endif
    }
    HIP_TRY(hipGetLastError());
    return FCZ_OK;
}

int fcz_compress_batch(fcz_ctx* ctx, const fcz_chain_batch* in, const uint64_t* out_off, uint8_t* out, int32_t* status) {
    if (!ctx || !in || !out_off || !out) return FCZ_E_INVALID_ARG;
    if (in->anchor_threshold <= 0) return FCZ_E_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    const uint32_t C = in->n_chains;
    if (C == 0) return FCZ_OK;
    claim_staging(ctx);
    const uint64_t out_bytes = out_off[C];
    // the side-chain byte addresses handed from k_compress_index to the angle kernels keep 39 bits (fcz_compress.h, sc_addr_put):
    // a blob of 512 GB or more is refused, not truncated (no device holds one: a device-resident out_dev cannot reach the limit)
    if (out_bytes >= (1ull << 39)) return FCZ_E_INVALID_ARG;
    fcz_chain_batch dv = *in;               // the batch with its pointers on the device
    int rc = each_batch_array(dv, *in, *in, in->title_off[C], [&](int i, auto& dst, auto* src, size_t bytes) -> int {
        dev_buf& b = ctx->pool[BATCH_IN + i];
        int e = b.ensure(std::max<size_t>(bytes, 16)); if (e) return e;
        if (bytes) HIP_TRY(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
        dst = b.as<std::remove_pointer_t<std::decay_t<decltype(dst)>>>();
        return FCZ_OK;
    });
    if (rc) return rc;
    if ((rc = ctx->pool[KEPT_OFF].ensure(sizeof(uint64_t) * ((size_t)C + 1)))) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->pool[KEPT_OFF].p, out_off, sizeof(uint64_t) * ((size_t)C + 1), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = ctx->pool[KEPT_BYTES].ensure(std::max<uint64_t>(out_bytes, 16))) || (rc = ctx->pool[KEPT_STATUS].ensure(sizeof(int32_t) * C))) return rc;
    rc = fcz_compress_batch_dev(ctx, &dv, ctx->pool[KEPT_OFF].as<uint64_t>(), ctx->pool[KEPT_BYTES].as<uint8_t>(), ctx->pool[KEPT_STATUS].as<int32_t>());
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out, ctx->pool[KEPT_BYTES].p, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    std::vector<int32_t> st_host;
    int32_t* st = status;
    if (!st) { st_host.resize(C); st = st_host.data(); }
    HIP_TRY(hipMemcpyAsync(st, ctx->pool[KEPT_STATUS].p, sizeof(int32_t) * C, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    int worst = FCZ_OK;
    for (uint32_t c = 0; c < C; c++) if (st[c] != FCZ_OK) worst = st[c];
    return worst;
}

// Pre-quantisation backbone angles of a host batch (what get_data() of the Python module reports for
// PDB input, foldcomp/foldcomp.cxx:633-662): angles_out is [6][R] floats in the order phi, psi, omega,
// n_ca_c, ca_c_n, c_n_ca; entry r0+k (k < n-1) belongs to packed word k of the chain starting at residue
// r0; n_ca_c[r0+n-1] holds the first residue's N-CA-C angle that the FCZ format drops.
int fcz_compress_angles(fcz_ctx* ctx, const fcz_chain_batch* in, float* angles_out) {
    if (!ctx || !in || !angles_out) return FCZ_E_INVALID_ARG;
    std::vector<uint64_t> off((size_t)in->n_chains + 1);
    int rc = fcz_compress_sizes(in, off.data());
    if (rc) return rc;
    std::vector<uint8_t> out(off[in->n_chains] ? off[in->n_chains] : 1);
    ctx->keep_first_angle = true;
    rc = fcz_compress_batch(ctx, in, off.data(), out.data(), nullptr);
    ctx->keep_first_angle = false;
    if (rc) return rc;
    HIP_TRY(hipMemcpy(angles_out, ctx->ang.p, sizeof(float) * 6 * (size_t)in->n_residues, hipMemcpyDeviceToHost));
    return FCZ_OK;
}

// the compress half of fcz_compress_pdb_begin / fcz_compress_gz_begin / fcz_compress_dense_begin: sizes, then the codec, on a batch
// an earlier stage left in the ctx; the records stay in pool[KEPT_*] for the fetch, their size in *kept_bytes
static int compress_resident_batch(fcz_ctx* ctx, const fcz_chain_batch& b, uint64_t* kept_bytes, uint64_t* fcz_bytes) {
    int rc;
    const uint32_t C = b.n_chains;
    if (C == 0) return FCZ_OK;
    dev_buf* k = ctx->pool;
    if ((rc = k[KEPT_OFF].ensure(8 * ((size_t)C + 1))) || (rc = k[KEPT_STATUS].ensure(4 * (size_t)C))) return rc;
    if ((rc = fcz_compress_sizes_dev(ctx, &b, k[KEPT_OFF].as<uint64_t>()))) return rc;
    HIP_TRY(hipMemcpyAsync(&ctx->pinned->record_bytes, k[KEPT_OFF].as<uint64_t>() + C, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const uint64_t bytes = ctx->pinned->record_bytes;
    if ((rc = k[KEPT_BYTES].ensure(std::max<uint64_t>(bytes, 16)))) return rc;
    if ((rc = fcz_compress_batch_dev(ctx, &b, k[KEPT_OFF].as<uint64_t>(), k[KEPT_BYTES].as<uint8_t>(), k[KEPT_STATUS].as<int32_t>()))) return rc;
    *kept_bytes = bytes; *fcz_bytes = bytes;
    return FCZ_OK;
}


// ------------------------------------------------------------------------------------------------
// structure ingest: PDB text -> fcz_chain_batch on the device (fcz_ingest.h)
// ------------------------------------------------------------------------------------------------
int fcz_ingest_pdb_dev(fcz_ctx* ctx, const uint8_t* text_dev, const uint64_t* file_off_dev, uint32_t n_files, uint64_t text_bytes,
                       const char* names_dev, const uint32_t* name_off_dev, const uint32_t* stem_len_dev, int anchor_threshold, int flags,
                       fcz_ingest_result* out) {
    if (!ctx || !out || anchor_threshold <= 0) return FCZ_E_INVALID_ARG;
    if (n_files && (!text_dev || !file_off_dev || !names_dev || !name_off_dev || !stem_len_dev)) return FCZ_E_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    memset(out, 0, sizeof *out);
    memset(&ctx->ig_res, 0, sizeof ctx->ig_res);
    memset(ctx->ig_counts, 0, sizeof ctx->ig_counts);
    out->n_files = n_files;
    if (n_files == 0) return FCZ_OK;
    // every accepted ATOM record has >= 54 characters (+ its line end, except possibly the file's last line)
    const uint64_t cap64 = text_bytes / 54u + (uint64_t)n_files;
    if (cap64 >> 32) return FCZ_E_INVALID_ARG;                 // atom offsets are 32-bit: split the batch
    const size_t cap = (size_t)cap64, F = n_files;
    int rc;
    auto need = [&](int i, size_t bytes) { return ctx->ig[i].ensure(std::max<size_t>(bytes, 16)); };
    if ((rc = need(B_CAP, 8 * F)) || (rc = need(B_ABASE, 8 * (F + 1))) || (rc = need(B_NAME, 4 * cap)) || (rc = need(B_RESN, 4 * cap)) ||
        (rc = need(B_SERIAL, 4 * cap)) || (rc = need(B_RESSEQ, 4 * cap)) || (rc = need(B_X, 4 * cap)) || (rc = need(B_Y, 4 * cap)) ||
        (rc = need(B_Z, 4 * cap)) || (rc = need(B_B, 4 * cap)) || (rc = need(B_CHAIN, 4 * cap)) || (rc = need(B_ACODE, cap)) || (rc = need(B_RCODE, cap)) ||
        (rc = need(B_RFIRST, 4 * cap)) || (rc = need(B_RBFAC, 4 * cap)) || (rc = need(B_RCODE2, cap)) || (rc = need(B_TITLES, (size_t)IG_TITLE_CAP * F)) ||
        (rc = need(B_TLEN, 4 * F)) || (rc = need(B_NKEPT, 4 * F)) || (rc = need(B_STATUS, 4 * F)) || (rc = need(B_FRAGS, sizeof(ingest_frag) * IG_MAX_FRAGS * F)) ||
        (rc = need(B_NFRAGS, 4 * F)) || (rc = need(B_TOTC, 4 * F)) || (rc = need(B_TOTR, 4 * F)) || (rc = need(B_TOTA, 4 * F)) || (rc = need(B_TOTT, 4 * F)) ||
        (rc = need(B_USESTEM, 4 * F)) || (rc = need(B_OFFC, 4 * (F + 1))) || (rc = need(B_OFFR, 4 * (F + 1))) || (rc = need(B_OFFA, 4 * (F + 1))) ||
        (rc = need(B_OFFT, 4 * (F + 1))) || (rc = need(B_REFUSED, 8 * (size_t)IG_MAX_FRAGS * F)) || (rc = need(B_NREF, 16)) || (rc = need(B_CIFROWS, 4 * F)))
        return rc;
    auto P = [&](int i) { return ctx->ig[i].p; };
    ingest_scratch T;
    T.name = (uint32_t*)P(B_NAME); T.resn = (uint32_t*)P(B_RESN); T.serial = (int32_t*)P(B_SERIAL); T.resseq = (int32_t*)P(B_RESSEQ);
    T.x = (float*)P(B_X); T.y = (float*)P(B_Y); T.z = (float*)P(B_Z); T.b = (float*)P(B_B);
    T.chain = (uint32_t*)P(B_CHAIN); T.acode = (uint8_t*)P(B_ACODE); T.rcode = (int8_t*)P(B_RCODE);
    T.r_first = (uint32_t*)P(B_RFIRST); T.r_bfac = (float*)P(B_RBFAC); T.r_code = (uint8_t*)P(B_RCODE2);
    hipLaunchKernelGGL(k_ingest_caps, dim3(grid_for(n_files, 256)), dim3(256), 0, ctx->stream, file_off_dev, n_files, (uint64_t*)P(B_CAP));
    if ((rc = device_scan<uint64_t>(ctx, (const uint64_t*)P(B_CAP), (uint64_t*)P(B_ABASE), n_files))) return rc;
    {
        span_guard g(ctx, "ingest_parse");
        hipLaunchKernelGGL(k_ingest_parse, dim3(n_files), dim3(WAVE), 0, ctx->stream, text_dev, file_off_dev, n_files, text_bytes,
                           (const uint64_t*)P(B_ABASE), T, (uint8_t*)P(B_TITLES), (uint32_t*)P(B_TLEN), (uint32_t*)P(B_NKEPT), (int32_t*)P(B_STATUS));
    }
    {
        // mmCIF text: the files the PDB kernel left to the host because they open with `data_` (a wavefront of any other file returns
        // at once); what this kernel cannot promise to read as the reference's reader would stays handed back
        span_guard g(ctx, "ingest_parse_cif");
        hipLaunchKernelGGL(k_ingest_parse_cif, dim3(n_files), dim3(WAVE), 0, ctx->stream, text_dev, file_off_dev, n_files,
                           (const uint64_t*)P(B_ABASE), T, (uint8_t*)P(B_TITLES), (uint32_t*)P(B_TLEN), (const int32_t*)P(B_STATUS), (uint32_t*)P(B_CIFROWS));
    }
    {
        // ... and the rows it marked, read by a kernel of their own (fcz_ingest_cif.h: the register file)
        span_guard g(ctx, "ingest_rows_cif");
        hipLaunchKernelGGL(k_ingest_rows_cif, dim3(n_files), dim3(WAVE), 0, ctx->stream, text_dev, file_off_dev, n_files, text_bytes,
                           (const uint64_t*)P(B_ABASE), T, (uint32_t*)P(B_NKEPT), (int32_t*)P(B_STATUS), (const uint32_t*)P(B_CIFROWS));
    }
    ingest_counts tot{(uint32_t*)P(B_TOTC), (uint32_t*)P(B_TOTR), (uint32_t*)P(B_TOTA), (uint32_t*)P(B_TOTT)};
    {
        span_guard g(ctx, "ingest_frags");
        hipLaunchKernelGGL(k_ingest_frags, dim3(n_files), dim3(WAVE), 0, ctx->stream, n_files, (const uint64_t*)P(B_ABASE), T, (const uint32_t*)P(B_NKEPT),
                           (int32_t*)P(B_STATUS), (const uint32_t*)P(B_TLEN), names_dev, name_off_dev, stem_len_dev, (const uint8_t*)P(B_TITLES),
                           anchor_threshold, (flags & FCZ_INGEST_SKIP_DISCONTINUOUS) ? 1 : 0, (ingest_frag*)P(B_FRAGS), (uint32_t*)P(B_NFRAGS), tot,
                           (uint32_t*)P(B_USESTEM));
    }
    uint32_t* ovf = (uint32_t*)P(B_NREF) + 1;
    HIP_TRY(hipMemsetAsync(P(B_NREF), 0, 16, ctx->stream));
    if ((rc = device_scan<uint32_t>(ctx, tot.chains, (uint32_t*)P(B_OFFC), n_files, ovf)) || (rc = device_scan<uint32_t>(ctx, tot.residues, (uint32_t*)P(B_OFFR), n_files, ovf)) ||
        (rc = device_scan<uint32_t>(ctx, tot.atoms, (uint32_t*)P(B_OFFA), n_files, ovf)) || (rc = device_scan<uint32_t>(ctx, tot.title_bytes, (uint32_t*)P(B_OFFT), n_files, ovf)))
        return rc;
    auto& pin = ctx->pinned->ingest;
    HIP_TRY(hipMemcpyAsync(&pin.chains, (uint32_t*)P(B_OFFC) + n_files, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(&pin.residues, (uint32_t*)P(B_OFFR) + n_files, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(&pin.atoms, (uint32_t*)P(B_OFFA) + n_files, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(&pin.title_bytes, (uint32_t*)P(B_OFFT) + n_files, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(&pin.overflow, ovf, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (pin.overflow) return FCZ_E_INVALID_ARG;
    const uint32_t C = pin.chains, R = pin.residues, M = pin.atoms, TB = pin.title_bytes;
    // the batch arrays: [atoms] x y z code | [residues + 1] atom_off, [residues] code bfac | [chains (+1)] ... | titles
    const size_t oa_x = 0, oa_y = 4 * (size_t)M, oa_z = 8 * (size_t)M, oa_c = 12 * (size_t)M;
    const size_t or_off = 0, or_bf = 4 * ((size_t)R + 1), or_rc = or_bf + 4 * (size_t)R;
    const size_t oc_res = 0, oc_tit = 4 * ((size_t)C + 1), oc_fr = 2 * oc_tit, oc_fa = oc_fr + 4 * (size_t)C, oc_file = oc_fa + 4 * (size_t)C,
                 oc_meta = oc_file + 4 * (size_t)C, oc_name = oc_meta + 4 * (size_t)C, oc_id = oc_name + 4 * (size_t)C;
    if ((rc = need(B_OUT_A, 13 * (size_t)M + 16)) || (rc = need(B_OUT_R, or_rc + R + 16)) || (rc = need(B_OUT_C, oc_id + C + 16)) || (rc = need(B_OUT_T, (size_t)TB + 16))) return rc;
    char* ba = (char*)P(B_OUT_A); char* br = (char*)P(B_OUT_R); char* bc = (char*)P(B_OUT_C);
    ingest_out O;
    O.x = (float*)(ba + oa_x); O.y = (float*)(ba + oa_y); O.z = (float*)(ba + oa_z); O.atom_code = (uint8_t*)(ba + oa_c);
    O.atom_off = (uint32_t*)(br + or_off); O.bfac_ca = (float*)(br + or_bf); O.res_code = (uint8_t*)(br + or_rc);
    O.res_off = (uint32_t*)(bc + oc_res); O.title_off = (uint32_t*)(bc + oc_tit); O.first_res = (int32_t*)(bc + oc_fr); O.first_atom = (int32_t*)(bc + oc_fa);
    O.chain_file = (uint32_t*)(bc + oc_file); O.chain_meta = (uint32_t*)(bc + oc_meta); O.chain_name4 = (uint32_t*)(bc + oc_name); O.chain_id = bc + oc_id;
    O.titles = (char*)P(B_OUT_T);
    {
        span_guard g(ctx, "ingest_fill");
        hipLaunchKernelGGL(k_ingest_fill, dim3(n_files), dim3(WAVE), 0, ctx->stream, n_files, (const uint64_t*)P(B_ABASE), T, (const ingest_frag*)P(B_FRAGS),
                           (const uint32_t*)P(B_NFRAGS), (const uint32_t*)P(B_OFFC), (const uint32_t*)P(B_OFFR), (const uint32_t*)P(B_OFFA), (const uint32_t*)P(B_OFFT),
                           (const uint32_t*)P(B_TLEN), (const uint32_t*)P(B_USESTEM), names_dev, name_off_dev, stem_len_dev, (const uint8_t*)P(B_TITLES), O,
                           (uint32_t*)P(B_REFUSED), (uint32_t*)P(B_NREF));
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&pin.refused, P(B_NREF), 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    fcz_ingest_result& r = ctx->ig_res;
    r.batch.n_chains = C; r.batch.n_residues = R; r.batch.n_atoms = M; r.batch.anchor_threshold = anchor_threshold;
    r.batch.res_off = O.res_off; r.batch.atom_off = O.atom_off; r.batch.x = O.x; r.batch.y = O.y; r.batch.z = O.z;
    r.batch.atom_code = O.atom_code; r.batch.res_code = O.res_code; r.batch.bfac_ca = O.bfac_ca;
    r.batch.first_res_index = O.first_res; r.batch.first_atom_index = O.first_atom; r.batch.chain_id = O.chain_id;
    r.batch.titles = O.titles; r.batch.title_off = O.title_off;
    r.chain_file = O.chain_file; r.chain_meta = O.chain_meta; r.chain_name4 = O.chain_name4; r.file_status = (const int32_t*)P(B_STATUS); r.refused = (const uint32_t*)P(B_REFUSED);
    r.n_files = n_files; r.n_refused = pin.refused;
    ctx->ig_counts[0] = C; ctx->ig_counts[1] = R; ctx->ig_counts[2] = M; ctx->ig_counts[3] = TB; ctx->ig_counts[4] = pin.refused;
    *out = r;
    return FCZ_OK;
}

static int ingest_fetch_meta(fcz_ctx* ctx, uint32_t* chain_file, uint32_t* chain_meta, int32_t* file_status, uint32_t* refused) {
    const fcz_ingest_result& r = ctx->ig_res;
    const uint32_t C = r.batch.n_chains;
    if (chain_file && C) HIP_TRY(hipMemcpyAsync(chain_file, r.chain_file, 4 * (size_t)C, hipMemcpyDeviceToHost, ctx->stream));
    if (chain_meta && C) HIP_TRY(hipMemcpyAsync(chain_meta, r.chain_meta, 4 * (size_t)C, hipMemcpyDeviceToHost, ctx->stream));
    if (file_status && r.n_files) HIP_TRY(hipMemcpyAsync(file_status, r.file_status, 4 * (size_t)r.n_files, hipMemcpyDeviceToHost, ctx->stream));
    if (refused && r.n_refused) HIP_TRY(hipMemcpyAsync(refused, r.refused, 8 * (size_t)r.n_refused, hipMemcpyDeviceToHost, ctx->stream));
    return FCZ_OK;
}

int fcz_ingest_chain_names_fetch(fcz_ctx* ctx, uint32_t* chain_name4) {
    if (!ctx) return FCZ_E_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    const fcz_ingest_result& r = ctx->ig_res;
    if (r.batch.n_chains) {
        if (!chain_name4) return FCZ_E_INVALID_ARG;
        HIP_TRY(hipMemcpyAsync(chain_name4, r.chain_name4, 4 * (size_t)r.batch.n_chains, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return FCZ_OK;
}

int fcz_ingest_pdb_fetch(fcz_ctx* ctx, const fcz_chain_batch* hb, uint32_t* chain_file, uint32_t* chain_meta, int32_t* file_status, uint32_t* refused) {
    if (!ctx) return FCZ_E_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    int rc = (hb && ctx->ig_res.n_files) ? fetch_batch(ctx, *hb, ctx->ig_res.batch, ctx->ig_counts[3]) : FCZ_OK; if (rc) return rc;
    if ((rc = ingest_fetch_meta(ctx, chain_file, chain_meta, file_status, refused))) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return FCZ_OK;
}

// ------------------------------------------------------------------------------------------------
// inflate: gzip members -> text on the device (fcz_inflate.h)
// ------------------------------------------------------------------------------------------------
int fcz_inflate_sizes(const uint8_t* gz, const uint64_t* gz_off, uint32_t n, const uint8_t* kind, uint64_t* text_off) {
    if (!text_off || (n && (!gz || !gz_off))) return FCZ_E_INVALID_ARG;
    uint64_t pos = 0;
    for (uint32_t i = 0; i < n; i++) {
        text_off[i] = pos;
        if (gz_off[i + 1] < gz_off[i]) return FCZ_E_INVALID_ARG;
        const uint64_t len = gz_off[i + 1] - gz_off[i];
        if (kind && kind[i] == 0) { pos += len; continue; }
        if (len < 18) continue;
        const uint8_t* t = gz + gz_off[i + 1] - 4;
        const uint64_t isize = (uint64_t)t[0] | ((uint64_t)t[1] << 8) | ((uint64_t)t[2] << 16) | ((uint64_t)t[3] << 24);
        // DEFLATE expands by at most 1032 : 1 (258 bytes per two bits, zlib's documented bound); an ISIZE beyond that is not this
        // member's text size (a corrupt trailer, several members, > 4 GB of text): zlib's to read
        if (isize > (len - 18) * 1032 + 1024 || isize >= (1ull << 31)) continue;
        pos += isize;
    }
    text_off[n] = pos;
    return FCZ_OK;
}

int fcz_inflate_dev(fcz_ctx* ctx, const uint8_t* gz_dev, const uint64_t* gz_off_dev, uint32_t n, const uint8_t* kind_dev,
                    const uint64_t* text_off_dev, uint8_t* text_dev, int32_t* status_dev) {
    if (!ctx) return FCZ_E_INVALID_ARG;
    if (n == 0) return FCZ_OK;
    if (!gz_dev || !gz_off_dev || !text_off_dev || !text_dev || !status_dev) return FCZ_E_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    {
        span_guard g(ctx, "inflate");
        hipLaunchKernelGGL(inflate::k_inflate, dim3(n), dim3(WAVE), 0, ctx->stream, gz_dev, gz_off_dev, n, kind_dev, text_off_dev, text_dev, status_dev);
    }
    HIP_TRY(hipGetLastError());
    return FCZ_OK;
}

// the files' bytes -> ctx->gz_raw, their text -> ctx->pool[FILES_TEXT] (text offsets in ctx->gz_toff, statuses in ctx->gz_status)
static int inflate_into_text(fcz_ctx* ctx, const uint8_t* data, const uint64_t* file_off, uint32_t n, const uint8_t* kind, const uint64_t* text_off) {
    const uint64_t raw_bytes = file_off[n], text_bytes = text_off[n];
    int rc;
    if ((rc = ctx->gz_raw.ensure(std::max<uint64_t>(raw_bytes, 16))) || (rc = ctx->gz_off.ensure(8 * ((size_t)n + 1))) || (rc = ctx->gz_kind.ensure(std::max<size_t>(n, 16))) ||
        (rc = ctx->gz_toff.ensure(8 * ((size_t)n + 1))) || (rc = ctx->gz_status.ensure(4 * (size_t)n + 16)) || (rc = ctx->pool[FILES_TEXT].ensure(std::max<uint64_t>(text_bytes, 16))))
        return rc;
    if (raw_bytes) HIP_TRY(hipMemcpyAsync(ctx->gz_raw.p, data, raw_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->gz_off.p, file_off, 8 * ((size_t)n + 1), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->gz_toff.p, text_off, 8 * ((size_t)n + 1), hipMemcpyHostToDevice, ctx->stream));
    if (kind) HIP_TRY(hipMemcpyAsync(ctx->gz_kind.p, kind, n, hipMemcpyHostToDevice, ctx->stream));
    return fcz_inflate_dev(ctx, ctx->gz_raw.as<uint8_t>(), ctx->gz_off.as<uint64_t>(), n, kind ? ctx->gz_kind.as<uint8_t>() : nullptr,
                           ctx->gz_toff.as<uint64_t>(), ctx->pool[FILES_TEXT].as<uint8_t>(), ctx->gz_status.as<int32_t>());
}

int fcz_inflate(fcz_ctx* ctx, const uint8_t* gz, const uint64_t* gz_off, uint32_t n, const uint8_t* kind, const uint64_t* text_off,
                uint8_t* text, int32_t* status) {
    if (!ctx) return FCZ_E_INVALID_ARG;
    if (n == 0) return FCZ_OK;
    if (!gz || !gz_off || !text_off || !status || (text_off[n] && !text)) return FCZ_E_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    claim_staging(ctx);
    int rc = inflate_into_text(ctx, gz, gz_off, n, kind, text_off); if (rc) return rc;
    if (text_off[n]) HIP_TRY(hipMemcpyAsync(text, ctx->pool[FILES_TEXT].p, text_off[n], hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(status, ctx->gz_status.p, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return FCZ_OK;
}

// fcz_ingest_pdb_begin / fcz_compress_pdb_begin (gz false: data is text) and fcz_ingest_gz_begin / fcz_compress_gz_begin (gz true: the
// files as they lie on disk, inflated on the device first); with fcz_bytes the resident batch is compressed too
static int ingest_begin(fcz_ctx* ctx, const uint8_t* data, const uint64_t* file_off, uint32_t n_files, bool gz, const uint8_t* is_gz, const char* names,
                        const uint32_t* name_off, const uint32_t* stem_len, int anchor_threshold, int flags, uint32_t counts[5], uint64_t* fcz_bytes) {
    if (!ctx || !counts || anchor_threshold <= 0) return FCZ_E_INVALID_ARG;
    if (n_files && (!data || !file_off || !names || !name_off || !stem_len)) return FCZ_E_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    claim_staging(ctx);
    memset(counts, 0, 5 * sizeof(uint32_t));
    if (n_files == 0) { memset(&ctx->ig_res, 0, sizeof ctx->ig_res); memset(ctx->ig_counts, 0, sizeof ctx->ig_counts); return FCZ_OK; }
    dev_buf* f = ctx->pool;
    int rc;
    uint64_t text_bytes = file_off[n_files];
    if (gz) {
        std::vector<uint64_t> text_off((size_t)n_files + 1);
        if ((rc = fcz_inflate_sizes(data, file_off, n_files, is_gz, text_off.data()))) return rc;
        if ((rc = inflate_into_text(ctx, data, file_off, n_files, is_gz, text_off.data()))) return rc;
        text_bytes = text_off[n_files];
    } else {
        if ((rc = f[FILES_TEXT].ensure(std::max<uint64_t>(text_bytes, 16))) || (rc = f[FILES_OFF].ensure(8 * ((size_t)n_files + 1)))) return rc;
        HIP_TRY(hipMemcpyAsync(f[FILES_TEXT].p, data, text_bytes, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(f[FILES_OFF].p, file_off, 8 * ((size_t)n_files + 1), hipMemcpyHostToDevice, ctx->stream));
    }
    const uint32_t name_bytes = name_off[n_files];
    if ((rc = f[FILES_NAMES].ensure(std::max<size_t>(name_bytes, 16))) || (rc = f[FILES_NAME_OFF].ensure(4 * ((size_t)n_files + 1))) || (rc = f[FILES_STEM_LEN].ensure(4 * (size_t)n_files))) return rc;
    if (name_bytes) HIP_TRY(hipMemcpyAsync(f[FILES_NAMES].p, names, name_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(f[FILES_NAME_OFF].p, name_off, 4 * ((size_t)n_files + 1), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(f[FILES_STEM_LEN].p, stem_len, 4 * (size_t)n_files, hipMemcpyHostToDevice, ctx->stream));
    fcz_ingest_result res;
    rc = fcz_ingest_pdb_dev(ctx, f[FILES_TEXT].as<uint8_t>(), gz ? ctx->gz_toff.as<uint64_t>() : f[FILES_OFF].as<uint64_t>(), n_files, text_bytes,
                            f[FILES_NAMES].as<char>(), f[FILES_NAME_OFF].as<uint32_t>(), f[FILES_STEM_LEN].as<uint32_t>(), anchor_threshold, flags, &res);
    if (rc) return rc;
    if (gz) {   // a member the device did not inflate left blanks (no atoms): the FILE goes back to the caller's zlib and reader
        hipLaunchKernelGGL(inflate::k_inflate_merge_status, dim3(grid_for(n_files, 256)), dim3(256), 0, ctx->stream, ctx->gz_status.as<int32_t>(), n_files,
                           (int32_t)FCZ_INGEST_HOST_GZIP, ctx->ig[B_STATUS].as<int32_t>());
        HIP_TRY(hipGetLastError());
    }
    memcpy(counts, ctx->ig_counts, sizeof ctx->ig_counts);
    return fcz_bytes ? compress_resident_batch(ctx, ctx->ig_res.batch, &ctx->ig_fcz_bytes, fcz_bytes) : FCZ_OK;
}

int fcz_ingest_pdb_begin(fcz_ctx* ctx, const uint8_t* text, const uint64_t* file_off, uint32_t n_files, const char* names, const uint32_t* name_off,
                         const uint32_t* stem_len, int anchor_threshold, int flags, uint32_t counts[5]) {
    return ingest_begin(ctx, text, file_off, n_files, false, nullptr, names, name_off, stem_len, anchor_threshold, flags, counts, nullptr);
}

int fcz_ingest_gz_begin(fcz_ctx* ctx, const uint8_t* data, const uint64_t* file_off, uint32_t n_files, const uint8_t* is_gz, const char* names,
                        const uint32_t* name_off, const uint32_t* stem_len, int anchor_threshold, int flags, uint32_t counts[5]) {
    return ingest_begin(ctx, data, file_off, n_files, true, is_gz, names, name_off, stem_len, anchor_threshold, flags, counts, nullptr);
}

int fcz_compress_pdb_begin(fcz_ctx* ctx, const uint8_t* text, const uint64_t* file_off, uint32_t n_files, const char* names, const uint32_t* name_off,
                           const uint32_t* stem_len, int anchor_threshold, int flags, uint32_t counts[5], uint64_t* fcz_bytes) {
    if (!fcz_bytes) return FCZ_E_INVALID_ARG;
    *fcz_bytes = 0; if (ctx) ctx->ig_fcz_bytes = 0;
    return ingest_begin(ctx, text, file_off, n_files, false, nullptr, names, name_off, stem_len, anchor_threshold, flags, counts, fcz_bytes);
}

int fcz_compress_gz_begin(fcz_ctx* ctx, const uint8_t* data, const uint64_t* file_off, uint32_t n_files, const uint8_t* is_gz, const char* names,
                          const uint32_t* name_off, const uint32_t* stem_len, int anchor_threshold, int flags, uint32_t counts[5], uint64_t* fcz_bytes) {
    if (!fcz_bytes) return FCZ_E_INVALID_ARG;
    *fcz_bytes = 0; if (ctx) ctx->ig_fcz_bytes = 0;
    return ingest_begin(ctx, data, file_off, n_files, true, is_gz, names, name_off, stem_len, anchor_threshold, flags, counts, fcz_bytes);
}

int fcz_compress_pdb_fetch(fcz_ctx* ctx, uint64_t* out_off, int32_t* status, uint32_t* chain_file, uint32_t* chain_meta, int32_t* file_status,
                           uint32_t* refused, uint8_t* blob) {
    if (!ctx) return FCZ_E_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    int rc = fetch_resident(ctx, ctx->ig_res.batch.n_chains, ctx->ig_fcz_bytes, out_off, status, blob, hipMemcpyDeviceToHost); if (rc) return rc;
    if ((rc = ingest_fetch_meta(ctx, chain_file, chain_meta, file_status, refused))) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return FCZ_OK;
}

// ------------------------------------------------------------------------------------------------
// decompress
// ------------------------------------------------------------------------------------------------
static inline uint32_t h_u16(const uint8_t* p) { return p[0] | (p[1] << 8); }
static inline uint32_t h_u32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }

static void parse_entry(const uint8_t* e, uint64_t len, fcz_entry_info* info) {
    memset(info, 0, sizeof *info);
    if (len < 76) { info->status = FCZ_E_TRUNCATED; return; }
    if (memcmp(e, "FCMP", 4) != 0) { info->status = FCZ_E_BAD_MAGIC; return; }
    const uint32_t n = h_u16(e + 4);
    info->n_residues = n;
    info->n_atoms_header = h_u16(e + 6);
    info->first_res_index = (int32_t)h_u16(e + 8);
    info->first_atom_index = (int32_t)h_u16(e + 10);
    info->n_anchors = e[12];
    info->chain_id = (char)e[13];
    info->n_sidechain_torsions = h_u32(e + 16);
    info->first_residue = (char)e[20];
    info->last_residue = (char)e[21];
    info->title_len = h_u32(e + 24);
    info->title_off = 76 + 4 * info->n_anchors;
    if (info->title_len > len || info->n_sidechain_torsions > len) { info->status = FCZ_E_TRUNCATED; return; }
    const rec_layout L = make_layout(n, info->n_anchors, info->title_len, info->n_sidechain_torsions);
    if ((uint64_t)L.size > len) { info->status = FCZ_E_TRUNCATED; return; }
    if (n < 2 || info->n_anchors < 2) { info->status = FCZ_E_TOO_SHORT; return; }
    info->has_oxt = e[L.o_oxt];
    uint32_t na = 0, nsc = 0;
    for (uint32_t k = 0; k < n; k++) {
        uint32_t rc = e[L.o_words + 8 * k] >> 3;
        if (k == 0) { rc = 23; for (int i = 0; i < 24; i++) if (host_tab::h_res1[i] == info->first_residue) { rc = i; break; } }
        if (rc >= 24) rc = 23;
        if (!(rc < 20 || rc == 23)) { info->status = FCZ_E_RESIDUE; return; }
        na += host_tab::h_res_natoms[rc]; nsc += host_tab::h_res_natoms[rc] - 3;
    }
    if (nsc != info->n_sidechain_torsions) { info->status = FCZ_E_TRUNCATED; return; }
    for (uint32_t s = 0; s + 1 < info->n_anchors; s++) {
        const int a = (int)h_u32(e + L.o_aidx + 4 * s), b = (int)h_u32(e + L.o_aidx + 4 * (s + 1));
        if (a < 0 || b < a || b > (int)n - 1 || (s == 0 && a != 0) || (s + 2 == info->n_anchors && b != (int)n - 1)) {
            info->status = FCZ_E_TRUNCATED; return;
        }
    }
    info->n_atoms_out = na + (info->has_oxt ? 1 : 0);
    info->status = FCZ_OK;
}

int fcz_decompress_sizes(const uint8_t* blob, const uint64_t* off, uint32_t n, fcz_entry_info* info, uint32_t* res_off,
                         uint32_t* atom_off) {
    if (!blob || !off || !res_off || !atom_off) return FCZ_E_INVALID_ARG;
    uint64_t r = 0, a = 0;
    for (uint32_t i = 0; i < n; i++) {
        res_off[i] = (uint32_t)r; atom_off[i] = (uint32_t)a;
        fcz_entry_info tmp;
        fcz_entry_info* pi = info ? &info[i] : &tmp;
        parse_entry(blob + off[i], off[i + 1] - off[i], pi);
        if (pi->status == FCZ_OK) { r += pi->n_residues; a += pi->n_atoms_out; }
    }
    res_off[n] = (uint32_t)r; atom_off[n] = (uint32_t)a;
    // offsets are 32-bit: a batch whose residues or atoms reach 2^32 is refused, not wrapped
    if ((r >> 32) || (a >> 32)) return FCZ_E_INVALID_ARG;
    return FCZ_OK;
}

int fcz_check(const uint8_t* e, uint64_t len) {
    fcz_entry_info info;
    parse_entry(e, len, &info);
    if (info.status == FCZ_E_BAD_MAGIC || info.status == FCZ_E_TRUNCATED) return info.status;
    const rec_layout L = make_layout(info.n_residues, info.n_anchors, info.title_len, info.n_sidechain_torsions);
    bool empty_bb = true, empty_sc = true, empty_t = true;
    for (uint32_t k = 0; k < info.n_residues; k++) {
        const uint8_t* b = e + L.o_words + 8 * k;
        if ((b[0] & 7) | b[1] | b[2] | b[3] | b[4]) empty_bb = false;
        if (e[L.o_tbytes + k]) empty_t = false;
    }
    for (uint32_t k = 0; k < info.n_sidechain_torsions; k++) if (e[L.o_sc + k]) empty_sc = false;
    if (empty_bb) return 4;
    if (empty_sc) return 5;
    if (empty_t) return 6;
    return 0;
}

// The sizes pass of the decompress path: per-entry validation and counts (k_entry_sizes), then -- in three launches -- their
// exclusive prefixes, the longest anchor segment of the batch (sizes the ring of k_backbone), the totals, and the entries ordered by
// residue count for k_backbone (counting sort, longest first): k_sizes_reduce / _mid / _apply (fcz_kernels.h). The totals come
// back as ONE 32-byte copy into ctx->pinned->sizes after one stream synchronisation. atom_off_dev may be null (prefix not needed).
static int run_entry_sizes(fcz_ctx* ctx, const uint8_t* blob_dev, const uint64_t* off_dev, uint32_t n, uint32_t* res_off_dev,
                           uint32_t* atom_off_dev) {
    sizes_totals& tot = ctx->pinned->sizes;
    tot = sizes_totals{};
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(res_off_dev, 0, 4, ctx->stream));
        if (atom_off_dev) HIP_TRY(hipMemsetAsync(atom_off_dev, 0, 4, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return FCZ_OK;
    }
    int rc = ctx->cnt.ensure(sizeof(uint32_t) * 4 * (size_t)n); if (rc) return rc;
    uint32_t* cr = ctx->cnt.as<uint32_t>(); uint32_t* ca = cr + n; int32_t* st = cnt_status(ctx, n); uint32_t* seg = (uint32_t*)(st + n);
    // len_perm: [perm n][hist LEN_BUCKETS][cursor LEN_BUCKETS + 1][pad][maxseg 2][pad 2][totals 8]
    if ((rc = ctx->len_perm.ensure(sizeof(uint32_t) * ((size_t)n + 2 * LEN_BUCKETS + 16)))) return rc;
    uint32_t* perm = ctx->len_perm.as<uint32_t>(); uint32_t* hist = perm + n; uint32_t* cursor = hist + LEN_BUCKETS;
    uint32_t* maxseg = cursor + LEN_BUCKETS + 4; sizes_totals* totals = (sizes_totals*)(maxseg + 4);
    const unsigned nb = grid_for(n, SZ_CHUNK);
    if ((rc = ctx->scan_tmp.ensure(sizeof(unsigned long long) * 2 * ((size_t)nb + 1)))) return rc;
    unsigned long long* part_r = ctx->scan_tmp.as<unsigned long long>(); unsigned long long* part_a = part_r + nb + 1;
    // The residue-code array (k_entry_sizes -> k_res_index) has one slot per 8 bytes of the records; their total size is only known
    // on the device, so the array grows when a pass reports that it needed more -- that pass runs again (the first call, or a larger
    // batch than any before), every later one runs once with no host round trip before the launches.
    for (int attempt = 0; attempt < 2; attempt++) {
        HIP_TRY(hipMemsetAsync(hist, 0, sizeof(uint32_t) * (2 * LEN_BUCKETS + 16), ctx->stream));
        hipLaunchKernelGGL(k_entry_sizes, dim3(grid_for(n, GROUPS_PER_BLOCK)), dim3(BLOCK), 0, ctx->stream, blob_dev, off_dev, n, cr, ca, st, seg,
                           ctx->codes.as<uint8_t>(), (uint64_t)ctx->codes.cap);
        hipLaunchKernelGGL(k_sizes_reduce, dim3(nb), dim3(1024), 0, ctx->stream, cr, ca, seg, n, part_r, part_a, hist, maxseg);
        hipLaunchKernelGGL(k_sizes_mid, dim3(1), dim3(1024), 0, ctx->stream, nb, part_r, part_a, hist, cursor, maxseg, totals, off_dev + n);
        hipLaunchKernelGGL(k_sizes_apply, dim3(nb), dim3(1024), 0, ctx->stream, cr, ca, n, part_r, part_a, res_off_dev, atom_off_dev, cursor, perm);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&tot, totals, sizeof(sizes_totals), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        const uint64_t need = (uint64_t)tot.codes_lo | ((uint64_t)tot.codes_hi << 32);
        if (need <= ctx->codes.cap) break;
        if (attempt == 1) return FCZ_E_HIP;
        if ((rc = ctx->codes.ensure((size_t)(need + need / 8)))) return rc;
    }
    if (tot.overflow) return FCZ_E_INVALID_ARG;   // 2^32 residues or atoms in one batch: split it
    return FCZ_OK;
}

int fcz_decompress_sizes_dev(fcz_ctx* ctx, const uint8_t* blob_dev, const uint64_t* off_dev, uint32_t n,
                             uint32_t* res_off_dev, uint32_t* atom_off_dev, uint32_t* total_res, uint32_t* total_atoms) {
    if (!ctx || !blob_dev || !off_dev || !res_off_dev || !atom_off_dev) return FCZ_E_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    ctx->sizes_fresh = false;   // the pass below overwrites what an earlier sizes call left; set again only when it succeeds
    {
        span_guard g(ctx, "decompress_sizes");
        int rc = run_entry_sizes(ctx, blob_dev, off_dev, n, res_off_dev, atom_off_dev);
        if (rc) return rc;
    }
    const sizes_totals& tot = ctx->pinned->sizes;
    if (total_res) *total_res = tot.residues;
    if (total_atoms) *total_atoms = tot.atoms;
    // the fcz_decompress_batch_dev call that follows on the same entries reuses the totals and the length order
    ctx->sizes_key = {blob_dev, off_dev, n};
    ctx->sizes_memo = tot;
    ctx->sizes_fresh = true;
    return FCZ_OK;
}

// Totals and length order for a batch call: taken from the preceding sizes call on the same entries, else recomputed.
static int ensure_sizes(fcz_ctx* ctx, const uint8_t* blob_dev, const uint64_t* off_dev, uint32_t n, sizes_totals* tot) {
    if (ctx->sizes_fresh && ctx->sizes_key.blob == blob_dev && ctx->sizes_key.off == off_dev && ctx->sizes_key.n == n) {
        ctx->sizes_fresh = false;   // single use: the records may be rewritten before the next call
        *tot = ctx->sizes_memo;
        return FCZ_OK;
    }
    ctx->sizes_fresh = false;   // the pass below overwrites what a remembered sizes call left (length order, residue codes)
    int rc = ctx->sizes_res_off.ensure(sizeof(uint32_t) * ((size_t)n + 1)); if (rc) return rc;
    if ((rc = run_entry_sizes(ctx, blob_dev, off_dev, n, ctx->sizes_res_off.as<uint32_t>(), nullptr))) return rc;
    *tot = ctx->pinned->sizes;
    return FCZ_OK;
}

int fcz_decompress_batch_dev(fcz_ctx* ctx, const uint8_t* blob_dev, const uint64_t* off_dev, uint32_t n,
                             const uint32_t* res_off_dev, const uint32_t* atom_off_dev, int alt_order,
                             const fcz_atoms_out* out_dev) {
    if (!ctx || !blob_dev || !off_dev || !res_off_dev || !atom_off_dev || !atoms_out_ok(out_dev, false)) return FCZ_E_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    if (n == 0) return FCZ_OK;
    sizes_totals tot;
    int rc = ensure_sizes(ctx, blob_dev, off_dev, n, &tot);
    if (rc) return rc;
    const uint32_t R = tot.residues, max_seg = tot.max_seg, max_nseg = tot.max_nseg, n_long = tot.n_long;
    if (R == 0) return FCZ_OK;
    rc = ctx->bb.ensure(sizeof(v3) * 3 * (size_t)R); if (rc) return rc;
    const uint32_t* perm = ctx->len_perm.as<uint32_t>();
    const bool fast_bb = ctx->numerics == FCZ_NUMERICS_FAST, fast_sc = fast_bb;
#ifdef FCZ_PROFILING
    // measurement builds only (tools/hbm_busy_probe.py builds its own library with -DFCZ_PROFILING): FCZ_PROFILE_STAGES=<mask> leaves
    // stages out. The product library never reads the environment here -- a leaked variable must not turn a decompress into a no-op.
    { const char* ps = getenv("FCZ_PROFILE_STAGES"); ctx->profile_stages = ps ? ((unsigned)strtoul(ps, nullptr, 0) & 7u) : 7u; }
#else
    ctx->profile_stages = 7u;
#endif
    if (!(ctx->profile_stages & 1u)) { /* profiling aid: no backbone launch */ }
    else if (fast_bb) {
        // plain-float backbone: 8 chains per wavefront, the forward atoms of a segment stay in LDS; only segments longer than
        // one chunk (FB_K residue steps) park them in a scratch column, and then the launch is cut so that the columns of the
        // wavefronts in flight fit 4 GB
        span_guard g(ctx, "decompress_backbone");
        const uint32_t groups = grid_for(n, FB_CH);
        const bool need_scratch = max_seg > (uint32_t)FB_K + 1;
        const uint32_t col = need_scratch ? 3 * max_seg : 0;
        uint32_t chunk = groups;
        if (need_scratch) {
            chunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(groups, ((size_t)4 << 30) / ((size_t)FB_CH * col * sizeof(v3))));
            rc = ctx->fast_scratch.ensure((size_t)chunk * FB_CH * col * sizeof(v3)); if (rc) return rc;
        }
        for (uint32_t g0 = 0; g0 < groups; g0 += chunk) {
            const uint32_t gn = std::min(chunk, groups - g0);
            const uint32_t slots = std::min<uint32_t>(n - g0 * FB_CH, gn * FB_CH);
            hipLaunchKernelGGL(k_backbone_fast, dim3(gn), dim3(WAVE), 0, ctx->stream, blob_dev, off_dev, n, slots, res_off_dev,
                               perm + (size_t)g0 * FB_CH, need_scratch ? ctx->fast_scratch.as<v3>() : nullptr, col, ctx->bb.as<v3>());
        }
    } else {
        const uint32_t ring_rows = 3 * (max_seg ? max_seg : 1);
        const size_t slot_atoms = (size_t)ring_rows * WAVE, slot_trig = (size_t)(ring_rows / 3) * 6 * WAVE;
        // Long chains (>= FCZ_LONG_CHAIN residues, the head of the length order): when there are too few of them to fill the
        // GPU their serial forward pass would hold the launch for ~8 us per residue, so they take the split form (forward
        // pass, then one block per segment for the reverse pass) on a second stream beside the fused kernel of the rest.
        const uint32_t groups_long_all = grid_for(n_long, WAVE);
        const bool split_long = n_long > 0 && max_nseg > 0 && groups_long_all < 2u * 4u * (uint32_t)ctx->n_cu;
        const uint32_t n_split = split_long ? n_long : 0;
        if (split_long) {
            const size_t per_group = (size_t)max_nseg * (slot_atoms * sizeof(v3) + slot_trig * sizeof(float));
            const uint32_t chunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(groups_long_all, ((size_t)6 << 30) / per_group));
            rc = ctx->fwd_long.ensure(sizeof(v3) * slot_atoms * max_nseg * chunk); if (rc) return rc;
            rc = ctx->wring_long.ensure(sizeof(float) * slot_trig * max_nseg * chunk); if (rc) return rc;
            HIP_TRY(hipEventRecord(ctx->ev_fork, ctx->stream));
            HIP_TRY(hipStreamWaitEvent(ctx->stream2, ctx->ev_fork, 0));
            for (uint32_t g0 = 0; g0 < groups_long_all; g0 += chunk) {
                const uint32_t g = std::min(chunk, groups_long_all - g0);
                const uint32_t slots = std::min<uint32_t>(n_long - g0 * WAVE, g * WAVE);
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_backbone<1>), dim3(g), dim3(WAVE), 0, ctx->stream2, blob_dev, off_dev, n, slots, res_off_dev,
                                   perm + (size_t)g0 * WAVE, ctx->fwd_long.as<v3>(), ctx->wring_long.as<float>(), ring_rows, max_nseg, ctx->bb.as<v3>(), 0u, (uint32_t*)nullptr);
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_backbone<2>), dim3(g * max_nseg), dim3(WAVE), 0, ctx->stream2, blob_dev, off_dev, n, slots, res_off_dev,
                                   perm + (size_t)g0 * WAVE, ctx->fwd_long.as<v3>(), ctx->wring_long.as<float>(), ring_rows, max_nseg, ctx->bb.as<v3>(), 0u, (uint32_t*)nullptr);
            }
            HIP_TRY(hipEventRecord(ctx->ev_join, ctx->stream2));
        }
        const uint32_t n_fused = n - n_split;
        const uint32_t groups = grid_for(n_fused, WAVE);
        // persistent grid: as many wavefronts as the chip keeps in flight (FCZ_BACKBONE_MIN_WAVES per SIMD), one ring slot each --
        // 2 048 x 107.5 KB = 220 MB at the headline batch whatever its size, and a slot is rewritten by the wavefront's next
        // group instead of being left behind dirty (one slot per group was 1.68 GB at 1 M chains)
        const uint32_t resident = (uint32_t)ctx->n_cu * 4u * FCZ_BACKBONE_MIN_WAVES;
        const uint32_t blocks0 = std::min(groups, resident);
        rc = ctx->fwd.ensure(sizeof(v3) * (size_t)std::max<uint32_t>(blocks0, 1) * slot_atoms + 64); if (rc) return rc;
        rc = ctx->wring.ensure(sizeof(float) * (size_t)std::max<uint32_t>(blocks0, 1) * slot_trig); if (rc) return rc;
        uint32_t* next_group = (uint32_t*)(ctx->fwd.as<uint8_t>() + sizeof(v3) * (size_t)std::max<uint32_t>(blocks0, 1) * slot_atoms);
        if (groups) HIP_TRY(hipMemsetAsync(next_group, 0, sizeof(uint32_t), ctx->stream));
        {
            span_guard g(ctx, "decompress_backbone");
            if (groups)
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_backbone<0>), dim3(blocks0), dim3(WAVE), 0, ctx->stream, blob_dev, off_dev, n, n_fused, res_off_dev,
                                   perm + n_split, ctx->fwd.as<v3>(), ctx->wring.as<float>(), ring_rows, 1u, ctx->bb.as<v3>(), groups, next_group);
            if (split_long) HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
        }
    }
    rc = ctx->res_aoff.ensure(sizeof(uint32_t) * ((size_t)R + 1)); if (rc) return rc;
    rc = ctx->res_rc.ensure((size_t)R); if (rc) return rc;
    rc = ctx->res_sc.ensure(sizeof(uint32_t) * 3 * (size_t)R); if (rc) return rc;
    if (ctx->profile_stages & 2u) {
        span_guard g(ctx, "decompress_index");
        hipLaunchKernelGGL(k_res_index, dim3(grid_for(n, WAVES_PER_BLOCK)), dim3(BLOCK), 0, ctx->stream, blob_dev, off_dev, n,
                           res_off_dev, atom_off_dev, R, ctx->res_aoff.as<uint32_t>(), ctx->res_rc.as<uint8_t>(),
                           ctx->res_sc.as<uint32_t>(), *out_dev, ctx->codes.as<uint8_t>());
        // entries of up to 64 residues (k_res_index leaves them): four to a wavefront, a persistent grid over chunks of 16 entries
        hipLaunchKernelGGL(k_res_index_rows, dim3(std::min<uint32_t>(grid_for(grid_for(n, RI_CHUNK), WAVES_PER_BLOCK), (uint32_t)ctx->n_cu * 8u)), dim3(BLOCK), 0, ctx->stream, blob_dev, off_dev, n,
                           res_off_dev, atom_off_dev, R, ctx->res_aoff.as<uint32_t>(), ctx->res_rc.as<uint8_t>(),
                           ctx->res_sc.as<uint32_t>(), *out_dev, ctx->codes.as<uint8_t>());
    }
    if (ctx->profile_stages & 4u) {
        span_guard g(ctx, "decompress_sidechain");
        const uint32_t n_tiles = grid_for(R, SC_TILE);
        const uint32_t blocks = std::min<uint32_t>(n_tiles, (uint32_t)ctx->n_cu * FCZ_SIDECHAIN_MIN_BLOCKS * FCZ_SC_GRID_FACTOR);
        // 256-residue tiles; a tile with more atoms than the staging buffer holds is listed as two 128-residue halves for
        // the second launch (an empty list on any real protein: that launch then costs its table prologue)
        rc = ctx->tile_work.ensure(sizeof(uint32_t) * (2 * (size_t)n_tiles + 4)); if (rc) return rc;
        uint32_t* punt_count = ctx->tile_work.as<uint32_t>(); uint32_t* punt_list = punt_count + 4;
        HIP_TRY(hipMemsetAsync(punt_count, 0, sizeof(uint32_t) * 4, ctx->stream));
        const uint32_t blocks_half = std::min<uint32_t>(2 * n_tiles, (uint32_t)ctx->n_cu);
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(blocks), dim3(BLOCK), 0, ctx->stream, R, n_tiles, (uint32_t)SC_TILE, (const uint32_t*)nullptr,
                               (const uint32_t*)nullptr, punt_list, punt_count, ctx->res_aoff.as<uint32_t>(), ctx->res_rc.as<uint8_t>(),
                               ctx->res_sc.as<uint32_t>(), ctx->bb.as<v3>(), alt_order, *out_dev);
            hipLaunchKernelGGL(kernel, dim3(blocks_half), dim3(BLOCK), 0, ctx->stream, R, 2 * n_tiles, (uint32_t)SC_TILE / 2, (const uint32_t*)punt_list,
                               (const uint32_t*)punt_count, (uint32_t*)nullptr, (uint32_t*)nullptr, ctx->res_aoff.as<uint32_t>(),
                               ctx->res_rc.as<uint8_t>(), ctx->res_sc.as<uint32_t>(), ctx->bb.as<v3>(), alt_order, *out_dev);
        };
        if (fast_sc) launch(HIP_KERNEL_NAME(k_sidechain<true>)); else launch(HIP_KERNEL_NAME(k_sidechain<false>));
    }
    HIP_TRY(hipGetLastError());
    return FCZ_OK;
}

int fcz_decompress_batch(fcz_ctx* ctx, const uint8_t* blob, const uint64_t* off, uint32_t n, const uint32_t* res_off,
                         const uint32_t* atom_off, int alt_order, const fcz_atoms_out* out) {
    if (!ctx || !blob || !off || !res_off || !atom_off || !out) return FCZ_E_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    claim_staging(ctx);
    if (n == 0) return FCZ_OK;
    int rc;
    const uint32_t R = res_off[n], M = atom_off[n];
    fcz_atoms_out dv;
    const size_t offs = sizeof(uint32_t) * ((size_t)n + 1), fM = sizeof(float) * (size_t)M, fR = sizeof(float) * (size_t)R;
    const void* unused[2];
    // room for the atoms by stage_atoms, not reserve_out: the decode takes no NULL x, y, z or bfac_res, so an array without a byte (no
    // record decodes) still gets its 16 bytes. Only res_code and atom_code reach it as NULL when they are not wanted.
    if ((rc = stage_atoms(ctx, R, M, true, &dv)) || (rc = upload_records(ctx, blob, off, n)) ||
        (rc = stage_in(ctx, {{res_off, offs, REC_RES_OFF}, {atom_off, offs, REC_ATOM_OFF}}, unused)))
        return rc;
    if (!out->res_code) dv.res_code = nullptr;
    if (!out->atom_code) dv.atom_code = nullptr;
    if ((rc = decode_records(ctx, n, alt_order, &dv)) ||
        (rc = fetch_out(ctx, {{out->x, fM, REC_X}, {out->y, fM, REC_Y}, {out->z, fM, REC_Z}, {out->bfac_res, fR, REC_BFAC}, {out->res_code, R, REC_RES_CODE},
                              {out->atom_code, M, REC_ATOM_CODE}})))
        return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return FCZ_OK;
}

// ------------------------------------------------------------------------------------------------
// dense model-input tensors of decoded chains (fcz_dense.h; the reference stops at Foldcomp::decompress, src/foldcomp.cpp:779)
// ------------------------------------------------------------------------------------------------
// atom37: the slot is the position of the atom's NAME in this list (what AlphaFold / OpenFold call atom_types)
static const char* const DENSE_ATOM37[37] = {"N", "CA", "C", "CB", "O", "CG", "CG1", "CG2", "OG", "OG1", "SG", "CD", "CD1", "CD2", "ND1", "ND2",
                                             "OD1", "OD2", "SD", "CE", "CE1", "CE2", "CE3", "NE", "NE1", "NE2", "OE1", "OE2", "CH2", "NH1", "NH2",
                                             "OH", "CZ", "CZ2", "CZ3", "NZ", "OXT"};

int fcz_dense_width(int layout) {
    return layout == FCZ_DENSE_ATOM37 ? 37 : layout == FCZ_DENSE_ATOM14 ? 14 : layout == FCZ_DENSE_BACKBONE4 ? 4 : -1;
}

int fcz_dense_slot(int layout, int rc, int ac) {
    if (fcz_dense_width(layout) < 0 || rc < 0 || rc >= FCZ_N_RES_CODES || ac < 0 || ac >= FCZ_N_ATOM_CODES) return -1;
    if (ac == FCZ_ATOM_OXT) return layout == FCZ_DENSE_ATOM37 ? 36 : -1;     // the chain's last atom: no residue's table lists it
    int j = 0;
    while (j < host_tab::h_res_natoms[rc] && host_tab::h_res_atom[rc][j] != ac) j++;
    if (j == host_tab::h_res_natoms[rc]) return -1;                          // the residue has no such atom
    if (layout == FCZ_DENSE_ATOM14) return j;                                // canonical position inside the residue
    if (layout == FCZ_DENSE_BACKBONE4) return ac < 4 ? ac : -1;              // N, CA, C, O are the codes 0 .. 3
    for (int s = 0; s < 37; s++) if (strcmp(DENSE_ATOM37[s], host_tab::h_atom_name[ac]) == 0) return s;
    return -1;
}

// the kernel's table: slot -> position among the residue's decoded atoms, for the order they were decoded in
static dense_table dense_make_table(int layout, int alt_order) {
    dense_table t;
    memset(t.inv, 255, sizeof t.inv);
    const int A = fcz_dense_width(layout);
    for (int rc = 0; rc < FCZ_N_RES_CODES; rc++)
        for (int j = 0; j < host_tab::h_res_natoms[rc]; j++) {
            const int slot = fcz_dense_slot(layout, rc, fcz_res_code_atom(rc, j, alt_order));
            if (slot >= 0) t.inv[rc * A + slot] = (uint8_t)j;
        }
    return t;
}

// fcz_dense_dev (k_dense), fcz_dense_window_dev (k_dense_window with start_dev, which may be NULL) and fcz_dense_packed_dev (k_dense_packed:
// no L, and chain_index_dev beside the arrays the three share)
static int dense_rows(fcz_ctx* ctx, const uint8_t* blob_dev, const uint64_t* off_dev, uint32_t n, const uint32_t* res_off_dev,
                      const uint32_t* atom_off_dev, const fcz_atoms_out* atoms_dev, int alt_order, int layout, rows_form form, uint32_t L,
                      const uint32_t* start_dev, const fcz_dense_out* out_dev, int32_t* chain_index_dev) {
    if (!ctx || !blob_dev || !off_dev || !res_off_dev || !atom_off_dev || !atoms_out_ok(atoms_dev) || !out_dev) return FCZ_E_INVALID_ARG;
    if (fcz_dense_width(layout) < 0 || (L == 0 && form != ROWS_PACKED) || !out_dev->pos || !out_dev->mask) return FCZ_E_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    if (n == 0) return FCZ_OK;
    const dense_table tab = dense_make_table(layout, alt_order ? 1 : 0);
    const dense_args g{off_dev, res_off_dev, atom_off_dev, atoms_dev->x, atoms_dev->y, atoms_dev->z, atoms_dev->bfac_res, atoms_dev->res_code,
                       out_dev->pos, out_dev->mask, out_dev->aatype, out_dev->plddt, out_dev->res_index, out_dev->length};
    // packed: the tiles are counted on the device (res_off[n] / DN_TILE), at most 1 024 per entry, a record holds 65 535 residues
    const uint32_t tiles_per_entry = form == ROWS_PACKED ? 1024u : grid_for(L, DN_TILE);
    const uint64_t n_tiles = (uint64_t)n * tiles_per_entry;                  // every index behind it is 64-bit: n * L * A may pass 2^32
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(n_tiles, (uint64_t)ctx->n_cu * 32u);
    span_guard sg(ctx, "dense");
    dispatch_layout(layout, [&](auto A) {
        constexpr int W = decltype(A)::value;
        if (form == ROWS_PACKED)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dense_packed<W>), dim3(blocks), dim3(BLOCK), 0, ctx->stream, blob_dev, g, chain_index_dev, n, tab);
        else if (form == ROWS_WINDOW)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dense_window<W>), dim3(blocks), dim3(BLOCK), 0, ctx->stream, blob_dev, g, start_dev, n, L, tiles_per_entry, n_tiles, tab);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dense<W>), dim3(blocks), dim3(BLOCK), 0, ctx->stream, blob_dev, g, n, L, tiles_per_entry, n_tiles, tab);
    });
    HIP_TRY(hipGetLastError());
    return FCZ_OK;
}

int fcz_dense_dev(fcz_ctx* ctx, const uint8_t* blob_dev, const uint64_t* off_dev, uint32_t n, const uint32_t* res_off_dev,
                  const uint32_t* atom_off_dev, const fcz_atoms_out* atoms_dev, int alt_order, int layout, uint32_t L,
                  const fcz_dense_out* out_dev) {
    return dense_rows(ctx, blob_dev, off_dev, n, res_off_dev, atom_off_dev, atoms_dev, alt_order, layout, ROWS_PADDED, L, nullptr, out_dev, nullptr);
}

int fcz_dense_window_dev(fcz_ctx* ctx, const uint8_t* blob_dev, const uint64_t* off_dev, uint32_t n, const uint32_t* res_off_dev,
                         const uint32_t* atom_off_dev, const fcz_atoms_out* atoms_dev, int alt_order, int layout, uint32_t L,
                         const uint32_t* start_dev, const fcz_dense_out* out_dev) {
    return dense_rows(ctx, blob_dev, off_dev, n, res_off_dev, atom_off_dev, atoms_dev, alt_order, layout, ROWS_WINDOW, L, start_dev, out_dev, nullptr);
}

// the arrays a fcz_packed_out shares with a fcz_dense_out (NULL: none)
static fcz_dense_out padded_part(const fcz_packed_out* o) {
    return o ? fcz_dense_out{o->pos, o->mask, o->aatype, o->plddt, o->res_index, o->length} : fcz_dense_out{};
}

int fcz_dense_packed_dev(fcz_ctx* ctx, const uint8_t* blob_dev, const uint64_t* off_dev, uint32_t n, const uint32_t* res_off_dev,
                         const uint32_t* atom_off_dev, const fcz_atoms_out* atoms_dev, int alt_order, int layout, const fcz_packed_out* out_dev) {
    const fcz_dense_out d = padded_part(out_dev);
    return dense_rows(ctx, blob_dev, off_dev, n, res_off_dev, atom_off_dev, atoms_dev, alt_order, layout, ROWS_PACKED, 0u, nullptr, out_dev ? &d : nullptr,
                      out_dev ? out_dev->chain_index : nullptr);
}

// The three host-pointer forms. width_out is L_out (padded, windowed) or R_out (packed), row_off and chain_index are the packed form's;
// windowed: the starts of the host array `start`, which may be NULL. Staged by the rules of staged_call.
static int decompress_dense_impl(fcz_ctx* ctx, const uint8_t* blob, const uint64_t* off, uint32_t n, int layout, rows_form form, uint32_t L,
                                 const uint32_t* start, uint32_t* width_out, uint32_t* row_off, const fcz_dense_out* out, int32_t* chain_index,
                                 int32_t* status) {
    const bool packed = form == ROWS_PACKED;
    const size_t A = (size_t)fcz_dense_width(layout);
    if (!ctx || !blob || !off || fcz_dense_width(layout) < 0 || (!out && !width_out) || (out && (!out->pos || !out->mask))) return FCZ_E_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    claim_staging(ctx);
    if (width_out && (packed || n == 0)) *width_out = packed ? 0u : L;
    if (n == 0) { if (row_off) row_off[0] = 0; return FCZ_OK; }
    uint32_t R = 0, M = 0, longest = 0;
    int rc = upload_sized(ctx, blob, off, n, status, row_off, &R, &M, packed ? nullptr : &longest); if (rc) return rc;
    if (!packed && L == 0) L = longest;
    if (width_out) *width_out = packed ? R : L;
    if (!out) return FCZ_OK;
    const size_t rows = packed ? (size_t)R : (size_t)n * L;
    if (rows == 0) {            // no entry decodes and (padded) no width was asked for: the arrays are empty
        if (out->length) memset(out->length, 0, sizeof(uint32_t) * n);
        return FCZ_OK;
    }
    fcz_atoms_out dv;
    if ((rc = stage_atoms(ctx, R, M, false, &dv))) return rc;
    if (R && (rc = decode_records(ctx, n, 0, &dv))) return rc;             // R == 0 (padded): the dense kernel still writes every row as padding
    const std::initializer_list<staged_out> outs = {{out->pos, rows * A * 3 * sizeof(float), DENSE_OUT}, {out->mask, rows * A, DENSE_OUT + 1},
        {out->aatype, rows, DENSE_OUT + 2}, {out->plddt, rows * sizeof(float), DENSE_OUT + 3}, {out->res_index, rows * sizeof(int32_t), DENSE_OUT + 4},
        {out->length, sizeof(uint32_t) * n, DENSE_OUT + 5}, {chain_index, rows * sizeof(int32_t), DENSE_CHAIN_INDEX}};
    void* d[7]; const void* start_dev = nullptr;
    if ((rc = reserve_out(ctx, outs, d)) || (form == ROWS_WINDOW && (rc = stage_in(ctx, {{start, sizeof(uint32_t) * n, WINDOW_START}}, &start_dev)))) return rc;
    const fcz_dense_out dd{(float*)d[0], (uint8_t*)d[1], (uint8_t*)d[2], (float*)d[3], (int32_t*)d[4], (uint32_t*)d[5]};
    if ((rc = dense_rows(ctx, ctx->pool[REC_BLOB].as<uint8_t>(), ctx->pool[REC_OFF].as<uint64_t>(), n, ctx->pool[REC_RES_OFF].as<uint32_t>(),
                         ctx->pool[REC_ATOM_OFF].as<uint32_t>(), &dv, 0, layout, form, L, (const uint32_t*)start_dev, &dd, (int32_t*)d[6])) ||
        (rc = fetch_out(ctx, outs)))
        return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return FCZ_OK;
}

int fcz_decompress_dense(fcz_ctx* ctx, const uint8_t* blob, const uint64_t* off, uint32_t n, int layout, uint32_t L, uint32_t* L_out,
                         const fcz_dense_out* out, int32_t* status) {
    return decompress_dense_impl(ctx, blob, off, n, layout, ROWS_PADDED, L, nullptr, L_out, nullptr, out, nullptr, status);
}

int fcz_decompress_dense_window(fcz_ctx* ctx, const uint8_t* blob, const uint64_t* off, uint32_t n, int layout, uint32_t L, const uint32_t* start,
                                uint32_t* L_out, const fcz_dense_out* out, int32_t* status) {
    return decompress_dense_impl(ctx, blob, off, n, layout, ROWS_WINDOW, L, start, L_out, nullptr, out, nullptr, status);
}

int fcz_decompress_dense_packed(fcz_ctx* ctx, const uint8_t* blob, const uint64_t* off, uint32_t n, int layout, uint32_t* R_out, uint32_t* row_off,
                                const fcz_packed_out* out, int32_t* status) {
    const fcz_dense_out d = padded_part(out);
    return decompress_dense_impl(ctx, blob, off, n, layout, ROWS_PACKED, 0u, nullptr, R_out, row_off, out ? &d : nullptr, out ? out->chain_index : nullptr, status);
}

// ------------------------------------------------------------------------------------------------
// torsion-angle tensors straight from the record bytes (fcz_angles.h; the dequantisation of Foldcomp::decompress, src/foldcomp.cpp:784-804)
// ------------------------------------------------------------------------------------------------
int fcz_chi_atom(int rc, int k) {
    if (rc < 0 || rc >= FCZ_N_RES_CODES || k < 0 || k >= 4) return -1;
    const int slot = host_tab::h_res_chi_slot[rc][k];
    return slot ? host_tab::h_res_atom[rc][slot] : -1;
}

// fcz_angles_dev (k_angles), fcz_angles_window_dev (k_angles_window with start_dev and aatype_dev, either may be NULL) and
// fcz_angles_packed_dev (k_angles_packed: no L)
static int angles_rows(fcz_ctx* ctx, const uint8_t* blob_dev, const uint64_t* off_dev, uint32_t n, const uint32_t* res_off_dev, rows_form form, uint32_t L,
                       const uint32_t* start_dev, float* angles_dev, uint8_t* mask_dev, uint8_t* aatype_dev) {
    if (!ctx || !blob_dev || !off_dev || !res_off_dev || !angles_dev || !mask_dev || (L == 0 && form != ROWS_PACKED)) return FCZ_E_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    if (n == 0) return FCZ_OK;
    // one wavefront per entry on a persistent grid
    const dim3 blocks(std::min<uint32_t>(grid_for(n, WAVES_PER_BLOCK), (uint32_t)ctx->n_cu * 32u));
    span_guard sg(ctx, "angles");
    if (form == ROWS_PACKED)
        hipLaunchKernelGGL(k_angles_packed, blocks, dim3(BLOCK), 0, ctx->stream, blob_dev, off_dev, res_off_dev, n, angles_dev, mask_dev);
    else if (form == ROWS_WINDOW)
        hipLaunchKernelGGL(k_angles_window, blocks, dim3(BLOCK), 0, ctx->stream, blob_dev, off_dev, res_off_dev, n, L, start_dev, angles_dev, mask_dev, aatype_dev);
    else
        hipLaunchKernelGGL(k_angles, blocks, dim3(BLOCK), 0, ctx->stream, blob_dev, off_dev, res_off_dev, n, L, angles_dev, mask_dev);
    HIP_TRY(hipGetLastError());
    return FCZ_OK;
}

int fcz_angles_dev(fcz_ctx* ctx, const uint8_t* blob_dev, const uint64_t* off_dev, uint32_t n, const uint32_t* res_off_dev, uint32_t L,
                   float* angles_dev, uint8_t* mask_dev) {
    return angles_rows(ctx, blob_dev, off_dev, n, res_off_dev, ROWS_PADDED, L, nullptr, angles_dev, mask_dev, nullptr);
}

int fcz_angles_window_dev(fcz_ctx* ctx, const uint8_t* blob_dev, const uint64_t* off_dev, uint32_t n, const uint32_t* res_off_dev, uint32_t L,
                          const uint32_t* start_dev, float* angles_dev, uint8_t* mask_dev, uint8_t* aatype_dev) {
    return angles_rows(ctx, blob_dev, off_dev, n, res_off_dev, ROWS_WINDOW, L, start_dev, angles_dev, mask_dev, aatype_dev);
}

int fcz_angles_packed_dev(fcz_ctx* ctx, const uint8_t* blob_dev, const uint64_t* off_dev, uint32_t n, const uint32_t* res_off_dev,
                          float* angles_dev, uint8_t* mask_dev) {
    return angles_rows(ctx, blob_dev, off_dev, n, res_off_dev, ROWS_PACKED, 0u, nullptr, angles_dev, mask_dev, nullptr);
}

// The three host-pointer forms. width_out is L_out (padded, windowed) or R_out (packed), row_off is the packed form's; windowed: the
// starts of the host array `start` (may be NULL) and the optional host array aatype. Staged by the rules of staged_call.
static int decompress_angles_impl(fcz_ctx* ctx, const uint8_t* blob, const uint64_t* off, uint32_t n, rows_form form, uint32_t L, const uint32_t* start,
                                  uint32_t* width_out, uint32_t* row_off, float* angles, uint8_t* mask, uint8_t* aatype, int32_t* status) {
    const bool packed = form == ROWS_PACKED;
    if (!ctx || !blob || !off || (!angles != !mask) || (!angles && !width_out)) return FCZ_E_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    claim_staging(ctx);
    if (width_out) *width_out = packed ? 0u : L;
    if (n == 0) { if (row_off) row_off[0] = 0; return FCZ_OK; }
    uint32_t R = 0, M = 0, longest = 0;
    int rc = upload_sized(ctx, blob, off, n, status, row_off, &R, &M, packed ? nullptr : &longest); if (rc) return rc;
    if (!packed && L == 0) L = longest;
    if (width_out) *width_out = packed ? R : L;
    const size_t rows = packed ? (size_t)R : (size_t)n * L;
    if (!angles || rows == 0) return FCZ_OK;                      // a sizing call, or no row to fill
    const size_t elems = rows * FCZ_ANGLE_COLUMNS;
    const std::initializer_list<staged_out> outs = {{angles, elems * sizeof(float), ANGLES_OUT}, {mask, elems, ANGLES_OUT + 1}, {aatype, rows, ANGLES_OUT + 2}};
    void* d[3]; const void* start_dev = nullptr;
    if ((rc = reserve_out(ctx, outs, d)) || (form == ROWS_WINDOW && (rc = stage_in(ctx, {{start, sizeof(uint32_t) * n, WINDOW_START}}, &start_dev))) ||
        (rc = angles_rows(ctx, ctx->pool[REC_BLOB].as<uint8_t>(), ctx->pool[REC_OFF].as<uint64_t>(), n, ctx->pool[REC_RES_OFF].as<uint32_t>(), form, L,
                          (const uint32_t*)start_dev, (float*)d[0], (uint8_t*)d[1], (uint8_t*)d[2])) ||
        (rc = fetch_out(ctx, outs)))
        return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return FCZ_OK;
}

int fcz_decompress_angles(fcz_ctx* ctx, const uint8_t* blob, const uint64_t* off, uint32_t n, uint32_t L, uint32_t* L_out, float* angles,
                          uint8_t* mask, int32_t* status) {
    return decompress_angles_impl(ctx, blob, off, n, ROWS_PADDED, L, nullptr, L_out, nullptr, angles, mask, nullptr, status);
}

int fcz_decompress_angles_window(fcz_ctx* ctx, const uint8_t* blob, const uint64_t* off, uint32_t n, uint32_t L, const uint32_t* start,
                                 uint32_t* L_out, float* angles, uint8_t* mask, uint8_t* aatype, int32_t* status) {
    return decompress_angles_impl(ctx, blob, off, n, ROWS_WINDOW, L, start, L_out, nullptr, angles, mask, aatype, status);
}

int fcz_decompress_angles_packed(fcz_ctx* ctx, const uint8_t* blob, const uint64_t* off, uint32_t n, uint32_t* R_out, uint32_t* row_off,
                                 float* angles, uint8_t* mask, int32_t* status) {
    return decompress_angles_impl(ctx, blob, off, n, ROWS_PACKED, 0u, nullptr, R_out, row_off, angles, mask, nullptr, status);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// analyses of dense tensors: what they share (no counterpart in the reference)
// ------------------------------------------------------------------------------------------------
// What every form refuses beside its analysis' own *_args_ok: the padded form (bound = length [n] or NULL, rows = L) an entry without a
// row, the packed form (bound = row_off [n + 1], rows = R) chains without a row_off.
static bool bound_ok(bool packed, const uint32_t* bound, uint32_t n, uint32_t rows) { return packed ? n == 0 || bound : rows != 0; }

// The query tiles of a per-chain sweep (fcz_chains.h) and the blocks that run them: tile_rows rows a tile, at most blocks_per_cu blocks a
// CU. Padded: n * tiles_per_entry tiles. Packed (n > 0): reserve() makes room for n tile counts and their n + 1 offsets in
// ctx->sweep_tiles, scan() counts them on the device behind whatever the caller has enqueued -- the scratch is dead when the sweep that
// reads tile_off has run, so the sweeps share it. A *_rows function calls reserve(), opens its span and calls run(): every allocation
// lies in front of the span and every launch inside it.
struct chain_tiles {
    fcz_ctx* ctx; bool packed; uint32_t n, rows, tile_rows, max_blocks;
    uint64_t* tile_off = nullptr; uint32_t tiles_per_entry = 0; uint64_t n_padded = 0, blocks = 0;
    chain_tiles(fcz_ctx* c, bool p, uint32_t n_, uint32_t rows_, uint32_t tile_rows_ = CHAIN_TILE, uint32_t blocks_per_cu = 16u)
        : ctx(c), packed(p), n(n_), rows(rows_), tile_rows(tile_rows_), max_blocks((uint32_t)c->n_cu * blocks_per_cu) {}
    int reserve() {
        if (packed) {
            if (n == 0) return FCZ_OK;                                            // no chain, no tile: run() ends behind the fill
            int rc = ctx->sweep_tiles.ensure(sizeof(uint64_t) * (2 * (size_t)n + 1)); if (rc) return rc;
            tile_off = ctx->sweep_tiles.as<uint64_t>() + n;
            blocks = std::min<uint64_t>((uint64_t)rows / tile_rows + n, max_blocks);   // the tiles are counted on the device: at most this many
        } else {
            tiles_per_entry = (uint32_t)(((uint64_t)rows + tile_rows - 1) / tile_rows);   // (rows + 255 may pass 2^32)
            n_padded = (uint64_t)n * tiles_per_entry;
            blocks = std::min<uint64_t>(n_padded, max_blocks);
        }
        return FCZ_OK;
    }
    int scan(const uint32_t* row_off_dev) {
        hipLaunchKernelGGL(k_chain_tiles, dim3(std::min(grid_for(n, BLOCK), max_blocks)), dim3(BLOCK), 0, ctx->stream, row_off_dev, n, rows, tile_rows,
                           ctx->sweep_tiles.as<uint64_t>());
        return device_scan<uint64_t>(ctx, ctx->sweep_tiles.as<uint64_t>(), tile_off, n);
    }
    // the grid of a fill kernel over `items` elements, a thread each
    dim3 fill_grid(uint64_t items) const { return dim3((uint32_t)std::min<uint64_t>((items + BLOCK - 1) / BLOCK, max_blocks)); }
    // The launches of a sweep. Packed: fill() launches the analysis' fill kernel over the rows no chain covers, then the tiles are
    // scanned; sweep(std::bool_constant<PACKED>, grid, tile_off, tiles_per_entry, n_padded) launches its kernel or kernels with those
    // as their last three arguments.
    template <class Fill, class Sweep> int run(const uint32_t* bound_dev, Fill fill, Sweep sweep) {
        if (packed) {
            fill();
            if (n == 0) { HIP_TRY(hipGetLastError()); return FCZ_OK; }
            int rc = scan(bound_dev); if (rc) return rc;
            sweep(std::true_type{}, dim3((uint32_t)blocks), (const uint64_t*)tile_off, 0u, (uint64_t)0);
        } else
            sweep(std::false_type{}, dim3((uint32_t)blocks), (const uint64_t*)nullptr, tiles_per_entry, n_padded);
        HIP_TRY(hipGetLastError());
        return FCZ_OK;
    }
};

// the bytes of the host arrays of a call: its rows in all, pos [rows][A][3], mask [rows][A], bound (length [n] / row_off [n + 1]; NULL: 0)
struct dense_bytes {
    size_t rows, pos, mask, bound;
    dense_bytes(bool packed, uint32_t n, uint32_t rows_per, int layout, const uint32_t* b)
        : rows(packed ? (size_t)rows_per : (size_t)n * rows_per), pos(rows * (size_t)fcz_dense_width(layout) * 3 * sizeof(float)),
          mask(rows * (size_t)fcz_dense_width(layout)), bound(b ? sizeof(uint32_t) * ((size_t)n + (packed ? 1 : 0)) : 0) {}
};

// ------------------------------------------------------------------------------------------------
// k-nearest-neighbour residue graph of dense tensors (fcz_knn.h; no counterpart in the reference)
// ------------------------------------------------------------------------------------------------
static bool knn_args_ok(const fcz_ctx* ctx, const float* pos, const uint8_t* mask, int layout, int slot, uint32_t k, const int32_t* index, const float* dist) {
    return ctx && pos && mask && index && dist && fcz_dense_width(layout) > 0 && slot >= 0 && slot < fcz_dense_width(layout) && k >= 1 && k <= KNN_MAX_K;
}

// fcz_knn_dev (bound_dev is length [n] or NULL, rows = L) and fcz_knn_packed_dev (bound_dev = row_off [n + 1], rows = R)
static int knn_rows(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint32_t* bound_dev, bool packed, uint32_t n, uint32_t rows,
                    int layout, int slot, uint32_t k, int32_t* index_dev, float* dist_dev) {
    HIP_TRY(hipSetDevice(ctx->device));
    if (rows == 0 || (n == 0 && !packed)) return FCZ_OK;
    const knn_args g{pos_dev, mask_dev, bound_dev, n, rows, (uint32_t)fcz_dense_width(layout), (uint32_t)slot, k, index_dev, dist_dev};
    chain_tiles ct(ctx, packed, n, rows);
    int rc = ct.reserve(); if (rc) return rc;
    span_guard sg(ctx, "knn");
    return ct.run(bound_dev, [&] { hipLaunchKernelGGL(k_chain_fill<knn_args>, ct.fill_grid(rows), dim3(BLOCK), 0, ctx->stream, g); },
                  [&](auto P, dim3 grid, const uint64_t* tile_off, uint32_t tiles_per_entry, uint64_t n_padded) {
        auto launch = [&](auto KCAP) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_knn<decltype(KCAP)::value, decltype(P)::value>), grid, dim3(BLOCK), 0, ctx->stream, g, tile_off, tiles_per_entry, n_padded);
        };
        if (k <= 16) launch(std::integral_constant<int, 16>{});
        else if (k <= 32) launch(std::integral_constant<int, 32>{});
        else if (k <= 48) launch(std::integral_constant<int, 48>{});
        else launch(std::integral_constant<int, 64>{});
    });
}

// fcz_knn and fcz_knn_packed: the host arrays through DENSE_IN 0, 1, 3 and DENSE_OUT 10, 11
static int knn_host(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint32_t* bound, bool packed, uint32_t n, uint32_t rows_per, int layout,
                    int slot, uint32_t k, int32_t* index, float* dist) {
    const dense_bytes b(packed, n, rows_per, layout, bound);
    const size_t no = b.rows * k * sizeof(int32_t);
    return staged_call(ctx, {{pos, b.pos, DENSE_IN}, {mask, b.mask, DENSE_IN + 1}, {bound, b.bound, DENSE_IN + 3}}, {{index, no, DENSE_OUT}, {dist, no, DENSE_OUT + 1}},
                       [&](const void* const* in, void* const* out) {
        return knn_rows(ctx, (const float*)in[0], (const uint8_t*)in[1], (const uint32_t*)in[2], packed, n, rows_per, layout, slot, k, (int32_t*)out[0], (float*)out[1]);
    });
}

extern "C" {

int fcz_knn_pass(void) { return (int)KNN_PASS; }

int fcz_knn_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint32_t* length_dev, uint32_t n, uint32_t L, int layout, int slot,
                uint32_t k, int32_t* index_dev, float* dist_dev) {
    if (!knn_args_ok(ctx, pos_dev, mask_dev, layout, slot, k, index_dev, dist_dev) || !bound_ok(false, length_dev, n, L)) return FCZ_E_INVALID_ARG;
    return knn_rows(ctx, pos_dev, mask_dev, length_dev, false, n, L, layout, slot, k, index_dev, dist_dev);
}

int fcz_knn_packed_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint32_t* row_off_dev, uint32_t n, uint32_t R, int layout,
                       int slot, uint32_t k, int32_t* index_dev, float* dist_dev) {
    if (!knn_args_ok(ctx, pos_dev, mask_dev, layout, slot, k, index_dev, dist_dev) || !bound_ok(true, row_off_dev, n, R) || R > 0x7FFFFFFFu)
        return FCZ_E_INVALID_ARG;                                             // (index holds global rows as int32)
    return knn_rows(ctx, pos_dev, mask_dev, row_off_dev, true, n, R, layout, slot, k, index_dev, dist_dev);
}

int fcz_knn(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint32_t* length, uint32_t n, uint32_t L, int layout, int slot, uint32_t k,
            int32_t* index, float* dist) {
    if (!knn_args_ok(ctx, pos, mask, layout, slot, k, index, dist) || !bound_ok(false, length, n, L)) return FCZ_E_INVALID_ARG;
    return knn_host(ctx, pos, mask, length, false, n, L, layout, slot, k, index, dist);
}

int fcz_knn_packed(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint32_t* row_off, uint32_t n, uint32_t R, int layout, int slot, uint32_t k,
                   int32_t* index, float* dist) {
    if (!knn_args_ok(ctx, pos, mask, layout, slot, k, index, dist) || !bound_ok(true, row_off, n, R) || R > 0x7FFFFFFFu) return FCZ_E_INVALID_ARG;
    return knn_host(ctx, pos, mask, row_off, true, n, R, layout, slot, k, index, dist);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// per-residue lDDT of two dense tensor batches (fcz_lddt.h; no counterpart in the reference)
// ------------------------------------------------------------------------------------------------
static const float LDDT_THRESHOLDS[4] = {0.5f, 1.0f, 2.0f, 4.0f};

// rows: L (padded) or R (packed)
static bool lddt_args_ok(const fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, int layout, int slot, float cutoff,
                         const float* thresholds, uint32_t rows, const float* score, const int32_t* pairs, const int32_t* hits) {
    if (!ctx || !pos_true || !mask_true || !pos_pred || !score || !pairs || !hits) return false;
    if (fcz_dense_width(layout) <= 0 || slot < 0 || slot >= fcz_dense_width(layout)) return false;
    if (!std::isfinite(cutoff) || !(cutoff > 0.0f) || rows > LDDT_MAX_ROWS) return false;
    if (thresholds) for (int t = 0; t < 4; t++) if (std::isnan(thresholds[t])) return false;
    return true;
}

// fcz_lddt_dev (bound_dev is length [n] or NULL, rows = L) and fcz_lddt_packed_dev (bound_dev = row_off [n + 1], rows = R)
static int lddt_rows(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev, const uint8_t* mask_pred_dev,
                     const uint32_t* bound_dev, bool packed, uint32_t n, uint32_t rows, int layout, int slot, float cutoff, const float* thresholds,
                     float* score_dev, int32_t* pairs_dev, int32_t* hits_dev) {
    HIP_TRY(hipSetDevice(ctx->device));
    if (rows == 0 || (n == 0 && !packed)) return FCZ_OK;
    const float* th = thresholds ? thresholds : LDDT_THRESHOLDS;
    const lddt_args g{pos_true_dev, mask_true_dev, pos_pred_dev, mask_pred_dev, bound_dev, n, rows, (uint32_t)fcz_dense_width(layout), (uint32_t)slot,
                      lddt_c2(cutoff), th[0], th[1], th[2], th[3], score_dev, pairs_dev, hits_dev};
    chain_tiles ct(ctx, packed, n, rows);
    int rc = ct.reserve(); if (rc) return rc;
    span_guard sg(ctx, "lddt");
    return ct.run(bound_dev, [&] { hipLaunchKernelGGL(k_chain_fill<lddt_args>, ct.fill_grid(rows), dim3(BLOCK), 0, ctx->stream, g); },
                  [&](auto P, dim3 grid, const uint64_t* tile_off, uint32_t tiles_per_entry, uint64_t n_padded) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lddt<decltype(P)::value>), grid, dim3(BLOCK), 0, ctx->stream, g, tile_off, tiles_per_entry, n_padded);
    });
}

// fcz_lddt and fcz_lddt_packed: the host arrays through DENSE_IN 0, 1, 3, LDDT_PRED 4, 5 and LDDT_OUT 10 .. 12
static int lddt_host(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, const uint8_t* mask_pred, const uint32_t* bound,
                     bool packed, uint32_t n, uint32_t rows_per, int layout, int slot, float cutoff, const float* thresholds, float* score, int32_t* pairs,
                     int32_t* hits) {
    const dense_bytes b(packed, n, rows_per, layout, bound);
    const size_t no = b.rows * 4;
    return staged_call(ctx, {{pos_true, b.pos, DENSE_IN}, {mask_true, b.mask, DENSE_IN + 1}, {bound, b.bound, DENSE_IN + 3}, {pos_pred, b.pos, LDDT_PRED},
                             {mask_pred, b.mask, LDDT_PRED + 1}},
                       {{score, no, LDDT_OUT}, {pairs, no, LDDT_OUT + 1}, {hits, no, LDDT_OUT + 2}}, [&](const void* const* in, void* const* out) {
        return lddt_rows(ctx, (const float*)in[0], (const uint8_t*)in[1], (const float*)in[3], (const uint8_t*)in[4], (const uint32_t*)in[2], packed, n, rows_per,
                         layout, slot, cutoff, thresholds, (float*)out[0], (int32_t*)out[1], (int32_t*)out[2]);
    });
}

extern "C" {

int fcz_lddt_pass(void) { return (int)LDDT_PASS; }
float fcz_lddt_c2(float cutoff) { return std::isfinite(cutoff) && cutoff > 0.0f ? lddt_c2(cutoff) : NAN; }

int fcz_lddt_dev(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev, const uint8_t* mask_pred_dev,
                 const uint32_t* length_dev, uint32_t n, uint32_t L, int layout, int slot, float cutoff, const float* thresholds, float* score_dev,
                 int32_t* pairs_dev, int32_t* hits_dev) {
    if (!lddt_args_ok(ctx, pos_true_dev, mask_true_dev, pos_pred_dev, layout, slot, cutoff, thresholds, L, score_dev, pairs_dev, hits_dev) ||
        !bound_ok(false, length_dev, n, L))
        return FCZ_E_INVALID_ARG;
    return lddt_rows(ctx, pos_true_dev, mask_true_dev, pos_pred_dev, mask_pred_dev, length_dev, false, n, L, layout, slot, cutoff, thresholds, score_dev,
                     pairs_dev, hits_dev);
}

int fcz_lddt_packed_dev(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev, const uint8_t* mask_pred_dev,
                        const uint32_t* row_off_dev, uint32_t n, uint32_t R, int layout, int slot, float cutoff, const float* thresholds, float* score_dev,
                        int32_t* pairs_dev, int32_t* hits_dev) {
    if (!lddt_args_ok(ctx, pos_true_dev, mask_true_dev, pos_pred_dev, layout, slot, cutoff, thresholds, R, score_dev, pairs_dev, hits_dev) ||
        !bound_ok(true, row_off_dev, n, R))
        return FCZ_E_INVALID_ARG;
    return lddt_rows(ctx, pos_true_dev, mask_true_dev, pos_pred_dev, mask_pred_dev, row_off_dev, true, n, R, layout, slot, cutoff, thresholds, score_dev,
                     pairs_dev, hits_dev);
}

int fcz_lddt(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, const uint8_t* mask_pred, const uint32_t* length,
             uint32_t n, uint32_t L, int layout, int slot, float cutoff, const float* thresholds, float* score, int32_t* pairs, int32_t* hits) {
    if (!lddt_args_ok(ctx, pos_true, mask_true, pos_pred, layout, slot, cutoff, thresholds, L, score, pairs, hits) || !bound_ok(false, length, n, L))
        return FCZ_E_INVALID_ARG;
    return lddt_host(ctx, pos_true, mask_true, pos_pred, mask_pred, length, false, n, L, layout, slot, cutoff, thresholds, score, pairs, hits);
}

int fcz_lddt_packed(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, const uint8_t* mask_pred, const uint32_t* row_off,
                    uint32_t n, uint32_t R, int layout, int slot, float cutoff, const float* thresholds, float* score, int32_t* pairs, int32_t* hits) {
    if (!lddt_args_ok(ctx, pos_true, mask_true, pos_pred, layout, slot, cutoff, thresholds, R, score, pairs, hits) || !bound_ok(true, row_off, n, R))
        return FCZ_E_INVALID_ARG;
    return lddt_host(ctx, pos_true, mask_true, pos_pred, mask_pred, row_off, true, n, R, layout, slot, cutoff, thresholds, score, pairs, hits);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// smooth lDDT and its gradient (fcz_lddt_soft.h; no counterpart in the reference)
// ------------------------------------------------------------------------------------------------
// fcz_lddt_dev's rules with finite thresholds; the outputs are checked by the caller. rows: L (padded) or R (packed)
static bool lddt_soft_args_ok(const fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, int layout, int slot, float cutoff,
                              const float* thresholds, uint32_t rows) {
    if (!ctx || !pos_true || !mask_true || !pos_pred) return false;
    if (fcz_dense_width(layout) <= 0 || slot < 0 || slot >= fcz_dense_width(layout)) return false;
    if (!std::isfinite(cutoff) || !(cutoff > 0.0f) || rows > LDDT_MAX_ROWS) return false;
    if (thresholds) for (int t = 0; t < 4; t++) if (!std::isfinite(thresholds[t])) return false;
    return true;
}

// the device forms of the value (weight_dev and grad_dev NULL) and of the gradient (soft_dev and pairs_dev NULL); bound_dev is length [n]
// or NULL with rows = L, or row_off [n + 1] with rows = R
static int lddt_soft_rows(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev, const uint8_t* mask_pred_dev,
                          const uint32_t* bound_dev, bool packed, uint32_t n, uint32_t rows, int layout, int slot, float cutoff, const float* thresholds,
                          float* soft_dev, int32_t* pairs_dev, const float* weight_dev, float* grad_dev) {
    HIP_TRY(hipSetDevice(ctx->device));
    if (rows == 0 || (n == 0 && !packed)) return FCZ_OK;
    const float* th = thresholds ? thresholds : LDDT_THRESHOLDS;
    const uint32_t A = (uint32_t)fcz_dense_width(layout);
    const float c2 = lddt_c2(cutoff);
    chain_tiles ct(ctx, packed, n, rows);
    int rc = ct.reserve(); if (rc) return rc;
    if (grad_dev) {
        const lddt_soft_grad_args g{pos_true_dev, mask_true_dev, pos_pred_dev, mask_pred_dev, bound_dev, n, rows, A, (uint32_t)slot, c2, th[0], th[1], th[2], th[3],
                                    weight_dev, grad_dev};
        span_guard sg(ctx, "lddt_soft_grad");
        return ct.run(bound_dev, [&] { hipLaunchKernelGGL(k_chain_fill<lddt_soft_grad_args>, ct.fill_grid(rows), dim3(BLOCK), 0, ctx->stream, g); },
                      [&](auto P, dim3 grid, const uint64_t* tile_off, uint32_t tiles_per_entry, uint64_t n_padded) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lddt_soft_grad<decltype(P)::value>), grid, dim3(BLOCK), 0, ctx->stream, g, tile_off, tiles_per_entry, n_padded);
        });
    }
    const lddt_soft_args g{pos_true_dev, mask_true_dev, pos_pred_dev, mask_pred_dev, bound_dev, n, rows, A, (uint32_t)slot, c2, th[0], th[1], th[2], th[3],
                           soft_dev, pairs_dev};
    span_guard sg(ctx, "lddt_soft");
    return ct.run(bound_dev, [&] { hipLaunchKernelGGL(k_chain_fill<lddt_soft_args>, ct.fill_grid(rows), dim3(BLOCK), 0, ctx->stream, g); },
                  [&](auto P, dim3 grid, const uint64_t* tile_off, uint32_t tiles_per_entry, uint64_t n_padded) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lddt_soft<decltype(P)::value>), grid, dim3(BLOCK), 0, ctx->stream, g, tile_off, tiles_per_entry, n_padded);
    });
}

// the host forms: the host arrays through DENSE_IN 0, 1, 3, LDDT_PRED 4, 5, LDDT_WEIGHT 6 and LDDT_OUT 10 .. 11 (soft, pairs) or 10 (grad)
static int lddt_soft_host(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, const uint8_t* mask_pred, const uint32_t* bound,
                          bool packed, uint32_t n, uint32_t rows_per, int layout, int slot, float cutoff, const float* thresholds, float* soft, int32_t* pairs,
                          const float* weight, float* grad) {
    const dense_bytes b(packed, n, rows_per, layout, bound);
    const size_t no = b.rows * 4;
    auto run = [&](const void* const* in, void* const* out) {
        return lddt_soft_rows(ctx, (const float*)in[0], (const uint8_t*)in[1], (const float*)in[3], (const uint8_t*)in[4], (const uint32_t*)in[2], packed, n, rows_per,
                              layout, slot, cutoff, thresholds, grad ? nullptr : (float*)out[0], grad ? nullptr : (int32_t*)out[1], (const float*)in[5],
                              grad ? (float*)out[0] : nullptr);
    };
    if (grad)
        return staged_call(ctx, {{pos_true, b.pos, DENSE_IN}, {mask_true, b.mask, DENSE_IN + 1}, {bound, b.bound, DENSE_IN + 3}, {pos_pred, b.pos, LDDT_PRED},
                                 {mask_pred, b.mask, LDDT_PRED + 1}, {weight, no, LDDT_WEIGHT}}, {{grad, 3 * no, LDDT_OUT}}, run);
    return staged_call(ctx, {{pos_true, b.pos, DENSE_IN}, {mask_true, b.mask, DENSE_IN + 1}, {bound, b.bound, DENSE_IN + 3}, {pos_pred, b.pos, LDDT_PRED},
                             {mask_pred, b.mask, LDDT_PRED + 1}, {nullptr, 0, LDDT_WEIGHT}}, {{soft, no, LDDT_OUT}, {pairs, no, LDDT_OUT + 1}}, run);
}

extern "C" {

int fcz_lddt_soft_dev(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev, const uint8_t* mask_pred_dev,
                      const uint32_t* length_dev, uint32_t n, uint32_t L, int layout, int slot, float cutoff, const float* thresholds, float* soft_dev,
                      int32_t* pairs_dev) {
    if (!lddt_soft_args_ok(ctx, pos_true_dev, mask_true_dev, pos_pred_dev, layout, slot, cutoff, thresholds, L) || !soft_dev || !pairs_dev ||
        !bound_ok(false, length_dev, n, L))
        return FCZ_E_INVALID_ARG;
    return lddt_soft_rows(ctx, pos_true_dev, mask_true_dev, pos_pred_dev, mask_pred_dev, length_dev, false, n, L, layout, slot, cutoff, thresholds, soft_dev,
                          pairs_dev, nullptr, nullptr);
}

int fcz_lddt_soft_packed_dev(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev, const uint8_t* mask_pred_dev,
                             const uint32_t* row_off_dev, uint32_t n, uint32_t R, int layout, int slot, float cutoff, const float* thresholds, float* soft_dev,
                             int32_t* pairs_dev) {
    if (!lddt_soft_args_ok(ctx, pos_true_dev, mask_true_dev, pos_pred_dev, layout, slot, cutoff, thresholds, R) || !soft_dev || !pairs_dev ||
        !bound_ok(true, row_off_dev, n, R))
        return FCZ_E_INVALID_ARG;
    return lddt_soft_rows(ctx, pos_true_dev, mask_true_dev, pos_pred_dev, mask_pred_dev, row_off_dev, true, n, R, layout, slot, cutoff, thresholds, soft_dev,
                          pairs_dev, nullptr, nullptr);
}

int fcz_lddt_soft_grad_dev(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev, const uint8_t* mask_pred_dev,
                           const uint32_t* length_dev, uint32_t n, uint32_t L, int layout, int slot, float cutoff, const float* thresholds,
                           const float* weight_dev, float* grad_dev) {
    if (!lddt_soft_args_ok(ctx, pos_true_dev, mask_true_dev, pos_pred_dev, layout, slot, cutoff, thresholds, L) || !weight_dev || !grad_dev ||
        !bound_ok(false, length_dev, n, L))
        return FCZ_E_INVALID_ARG;
    return lddt_soft_rows(ctx, pos_true_dev, mask_true_dev, pos_pred_dev, mask_pred_dev, length_dev, false, n, L, layout, slot, cutoff, thresholds, nullptr, nullptr,
                          weight_dev, grad_dev);
}

int fcz_lddt_soft_grad_packed_dev(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev, const uint8_t* mask_pred_dev,
                                  const uint32_t* row_off_dev, uint32_t n, uint32_t R, int layout, int slot, float cutoff, const float* thresholds,
                                  const float* weight_dev, float* grad_dev) {
    if (!lddt_soft_args_ok(ctx, pos_true_dev, mask_true_dev, pos_pred_dev, layout, slot, cutoff, thresholds, R) || !weight_dev || !grad_dev ||
        !bound_ok(true, row_off_dev, n, R))
        return FCZ_E_INVALID_ARG;
    return lddt_soft_rows(ctx, pos_true_dev, mask_true_dev, pos_pred_dev, mask_pred_dev, row_off_dev, true, n, R, layout, slot, cutoff, thresholds, nullptr, nullptr,
                          weight_dev, grad_dev);
}

int fcz_lddt_soft(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, const uint8_t* mask_pred, const uint32_t* length,
                  uint32_t n, uint32_t L, int layout, int slot, float cutoff, const float* thresholds, float* soft, int32_t* pairs) {
    if (!lddt_soft_args_ok(ctx, pos_true, mask_true, pos_pred, layout, slot, cutoff, thresholds, L) || !soft || !pairs || !bound_ok(false, length, n, L))
        return FCZ_E_INVALID_ARG;
    return lddt_soft_host(ctx, pos_true, mask_true, pos_pred, mask_pred, length, false, n, L, layout, slot, cutoff, thresholds, soft, pairs, nullptr, nullptr);
}

int fcz_lddt_soft_packed(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, const uint8_t* mask_pred, const uint32_t* row_off,
                         uint32_t n, uint32_t R, int layout, int slot, float cutoff, const float* thresholds, float* soft, int32_t* pairs) {
    if (!lddt_soft_args_ok(ctx, pos_true, mask_true, pos_pred, layout, slot, cutoff, thresholds, R) || !soft || !pairs || !bound_ok(true, row_off, n, R))
        return FCZ_E_INVALID_ARG;
    return lddt_soft_host(ctx, pos_true, mask_true, pos_pred, mask_pred, row_off, true, n, R, layout, slot, cutoff, thresholds, soft, pairs, nullptr, nullptr);
}

int fcz_lddt_soft_grad(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, const uint8_t* mask_pred, const uint32_t* length,
                       uint32_t n, uint32_t L, int layout, int slot, float cutoff, const float* thresholds, const float* weight, float* grad) {
    if (!lddt_soft_args_ok(ctx, pos_true, mask_true, pos_pred, layout, slot, cutoff, thresholds, L) || !weight || !grad || !bound_ok(false, length, n, L))
        return FCZ_E_INVALID_ARG;
    return lddt_soft_host(ctx, pos_true, mask_true, pos_pred, mask_pred, length, false, n, L, layout, slot, cutoff, thresholds, nullptr, nullptr, weight, grad);
}

int fcz_lddt_soft_grad_packed(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, const uint8_t* mask_pred,
                              const uint32_t* row_off, uint32_t n, uint32_t R, int layout, int slot, float cutoff, const float* thresholds, const float* weight,
                              float* grad) {
    if (!lddt_soft_args_ok(ctx, pos_true, mask_true, pos_pred, layout, slot, cutoff, thresholds, R) || !weight || !grad || !bound_ok(true, row_off, n, R))
        return FCZ_E_INVALID_ARG;
    return lddt_soft_host(ctx, pos_true, mask_true, pos_pred, mask_pred, row_off, true, n, R, layout, slot, cutoff, thresholds, nullptr, nullptr, weight, grad);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// backbone FAPE and its gradient (fcz_fape.h; no counterpart in the reference)
// ------------------------------------------------------------------------------------------------
// the ten input arrays of a FAPE call, device or host pointers: frames and points of the truth, then of the prediction
struct fape_in {
    const float* rot_true; const float* trans_true; const uint8_t* fmask_true; const float* pos_true; const uint8_t* mask_true;
    const float* rot_pred; const float* trans_pred; const uint8_t* fmask_pred; const float* pos_pred; const uint8_t* mask_pred;
};

// the outputs are checked by the caller. rows: L (padded) or R (packed)
static bool fape_args_ok(const fcz_ctx* ctx, const fape_in& a, int layout, int slot, float clamp, float eps, uint32_t rows) {
    if (!ctx || !a.rot_true || !a.trans_true || !a.fmask_true || !a.pos_true || !a.mask_true || !a.rot_pred || !a.trans_pred || !a.pos_pred) return false;
    if (fcz_dense_width(layout) <= 0 || slot < 0 || slot >= fcz_dense_width(layout)) return false;
    if (std::isnan(clamp) || !(clamp > 0.0f) || !std::isfinite(eps) || !(eps > 0.0f) || rows > FAPE_MAX_ROWS) return false;
    return true;
}

// the device forms of the value (weight_dev and the gradients NULL) and of the gradient (sum_dev and points_dev NULL); bound_dev is
// length [n] or NULL with rows = L, or row_off [n + 1] with rows = R. The gradient is two sweeps behind one fill, in one span.
static int fape_rows(fcz_ctx* ctx, const fape_in& a, const uint32_t* bound_dev, bool packed, uint32_t n, uint32_t rows, int layout, int slot, float clamp,
                     float eps, float* sum_dev, int32_t* points_dev, const float* weight_dev, float* grad_rot_dev, float* grad_trans_dev, float* grad_pos_dev) {
    HIP_TRY(hipSetDevice(ctx->device));
    if (rows == 0 || (n == 0 && !packed)) return FCZ_OK;
    const uint32_t A = (uint32_t)fcz_dense_width(layout);
    chain_tiles ct(ctx, packed, n, rows);
    int rc = ct.reserve(); if (rc) return rc;
    if (grad_rot_dev) {
        const fape_grad_args g{a.rot_true, a.trans_true, a.fmask_true, a.pos_true, a.mask_true, a.rot_pred, a.trans_pred, a.fmask_pred, a.pos_pred, a.mask_pred,
                               bound_dev, n, rows, A, (uint32_t)slot, clamp, eps, weight_dev, grad_rot_dev, grad_trans_dev, grad_pos_dev};
        span_guard sg(ctx, "fape_grad");
        return ct.run(bound_dev, [&] { hipLaunchKernelGGL(k_chain_fill<fape_grad_args>, ct.fill_grid(rows), dim3(BLOCK), 0, ctx->stream, g); },
                      [&](auto P, dim3 grid, const uint64_t* tile_off, uint32_t tiles_per_entry, uint64_t n_padded) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fape_grad_frames<decltype(P)::value>), grid, dim3(BLOCK), 0, ctx->stream, g, tile_off, tiles_per_entry, n_padded);
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fape_grad_points<decltype(P)::value>), grid, dim3(BLOCK), 0, ctx->stream, g, tile_off, tiles_per_entry, n_padded);
        });
    }
    const fape_args g{a.rot_true, a.trans_true, a.fmask_true, a.pos_true, a.mask_true, a.rot_pred, a.trans_pred, a.fmask_pred, a.pos_pred, a.mask_pred,
                      bound_dev, n, rows, A, (uint32_t)slot, clamp, eps, sum_dev, points_dev};
    span_guard sg(ctx, "fape");
    return ct.run(bound_dev, [&] { hipLaunchKernelGGL(k_chain_fill<fape_args>, ct.fill_grid(rows), dim3(BLOCK), 0, ctx->stream, g); },
                  [&](auto P, dim3 grid, const uint64_t* tile_off, uint32_t tiles_per_entry, uint64_t n_padded) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fape<decltype(P)::value>), grid, dim3(BLOCK), 0, ctx->stream, g, tile_off, tiles_per_entry, n_padded);
    });
}

// the host forms: the host arrays through DENSE_IN 0, 1, 3, LDDT_PRED 4, 5, LDDT_WEIGHT 6, FAPE_FRAMES 7 .. 12 and FAPE_OUT 13 .. 14 (sum, points) or
// 13 .. 15 (grad_rot, grad_trans, grad_pos)
static int fape_host(fcz_ctx* ctx, const fape_in& a, const uint32_t* bound, bool packed, uint32_t n, uint32_t rows_per, int layout, int slot, float clamp, float eps,
                     float* sum, int32_t* points, const float* weight, float* grad_rot, float* grad_trans, float* grad_pos) {
    const dense_bytes b(packed, n, rows_per, layout, bound);
    const size_t no = b.rows * 4;
    auto run = [&](const void* const* in, void* const* out) {
        const fape_in d{(const float*)in[6], (const float*)in[7], (const uint8_t*)in[8], (const float*)in[0], (const uint8_t*)in[1],
                        (const float*)in[9], (const float*)in[10], (const uint8_t*)in[11], (const float*)in[3], (const uint8_t*)in[4]};
        const bool grad = grad_rot != nullptr;
        return fape_rows(ctx, d, (const uint32_t*)in[2], packed, n, rows_per, layout, slot, clamp, eps, grad ? nullptr : (float*)out[0],
                         grad ? nullptr : (int32_t*)out[1], (const float*)in[5], grad ? (float*)out[0] : nullptr, grad ? (float*)out[1] : nullptr,
                         grad ? (float*)out[2] : nullptr);
    };
    const std::initializer_list<staged_in> in = {
        {a.pos_true, b.pos, DENSE_IN}, {a.mask_true, b.mask, DENSE_IN + 1}, {bound, b.bound, DENSE_IN + 3}, {a.pos_pred, b.pos, LDDT_PRED},
        {a.mask_pred, b.mask, LDDT_PRED + 1}, {weight, no, LDDT_WEIGHT}, {a.rot_true, 9 * no, FAPE_FRAMES}, {a.trans_true, 3 * no, FAPE_FRAMES + 1},
        {a.fmask_true, b.rows, FAPE_FRAMES + 2}, {a.rot_pred, 9 * no, FAPE_FRAMES + 3}, {a.trans_pred, 3 * no, FAPE_FRAMES + 4},
        {a.fmask_pred, b.rows, FAPE_FRAMES + 5}};
    if (grad_rot) return staged_call(ctx, in, {{grad_rot, 9 * no, FAPE_OUT}, {grad_trans, 3 * no, FAPE_OUT + 1}, {grad_pos, 3 * no, FAPE_OUT + 2}}, run);
    return staged_call(ctx, in, {{sum, no, FAPE_OUT}, {points, no, FAPE_OUT + 1}}, run);
}

extern "C" {

int fcz_fape_pass(void) { return (int)(FAPE_PASS > FAPE_FRAME_PASS ? FAPE_PASS : FAPE_FRAME_PASS); }

#define FCZ_FAPE_INPUTS(S) const float* rot_true##S, const float* trans_true##S, const uint8_t* fmask_true##S, const float* pos_true##S, \
    const uint8_t* mask_true##S, const float* rot_pred##S, const float* trans_pred##S, const uint8_t* fmask_pred##S, const float* pos_pred##S, \
    const uint8_t* mask_pred##S
#define FCZ_FAPE_IN(S) fape_in{rot_true##S, trans_true##S, fmask_true##S, pos_true##S, mask_true##S, rot_pred##S, trans_pred##S, fmask_pred##S, pos_pred##S, mask_pred##S}

int fcz_fape_dev(fcz_ctx* ctx, FCZ_FAPE_INPUTS(_dev), const uint32_t* length_dev, uint32_t n, uint32_t L, int layout, int slot, float clamp, float eps,
                 float* sum_dev, int32_t* points_dev) {
    const fape_in a = FCZ_FAPE_IN(_dev);
    if (!fape_args_ok(ctx, a, layout, slot, clamp, eps, L) || !sum_dev || !points_dev || !bound_ok(false, length_dev, n, L)) return FCZ_E_INVALID_ARG;
    return fape_rows(ctx, a, length_dev, false, n, L, layout, slot, clamp, eps, sum_dev, points_dev, nullptr, nullptr, nullptr, nullptr);
}

int fcz_fape_packed_dev(fcz_ctx* ctx, FCZ_FAPE_INPUTS(_dev), const uint32_t* row_off_dev, uint32_t n, uint32_t R, int layout, int slot, float clamp, float eps,
                        float* sum_dev, int32_t* points_dev) {
    const fape_in a = FCZ_FAPE_IN(_dev);
    if (!fape_args_ok(ctx, a, layout, slot, clamp, eps, R) || !sum_dev || !points_dev || !bound_ok(true, row_off_dev, n, R)) return FCZ_E_INVALID_ARG;
    return fape_rows(ctx, a, row_off_dev, true, n, R, layout, slot, clamp, eps, sum_dev, points_dev, nullptr, nullptr, nullptr, nullptr);
}

int fcz_fape_grad_dev(fcz_ctx* ctx, FCZ_FAPE_INPUTS(_dev), const uint32_t* length_dev, uint32_t n, uint32_t L, int layout, int slot, float clamp, float eps,
                      const float* weight_dev, float* grad_rot_dev, float* grad_trans_dev, float* grad_pos_dev) {
    const fape_in a = FCZ_FAPE_IN(_dev);
    if (!fape_args_ok(ctx, a, layout, slot, clamp, eps, L) || !weight_dev || !grad_rot_dev || !grad_trans_dev || !grad_pos_dev || !bound_ok(false, length_dev, n, L))
        return FCZ_E_INVALID_ARG;
    return fape_rows(ctx, a, length_dev, false, n, L, layout, slot, clamp, eps, nullptr, nullptr, weight_dev, grad_rot_dev, grad_trans_dev, grad_pos_dev);
}

int fcz_fape_grad_packed_dev(fcz_ctx* ctx, FCZ_FAPE_INPUTS(_dev), const uint32_t* row_off_dev, uint32_t n, uint32_t R, int layout, int slot, float clamp,
                             float eps, const float* weight_dev, float* grad_rot_dev, float* grad_trans_dev, float* grad_pos_dev) {
    const fape_in a = FCZ_FAPE_IN(_dev);
    if (!fape_args_ok(ctx, a, layout, slot, clamp, eps, R) || !weight_dev || !grad_rot_dev || !grad_trans_dev || !grad_pos_dev || !bound_ok(true, row_off_dev, n, R))
        return FCZ_E_INVALID_ARG;
    return fape_rows(ctx, a, row_off_dev, true, n, R, layout, slot, clamp, eps, nullptr, nullptr, weight_dev, grad_rot_dev, grad_trans_dev, grad_pos_dev);
}

int fcz_fape(fcz_ctx* ctx, FCZ_FAPE_INPUTS(), const uint32_t* length, uint32_t n, uint32_t L, int layout, int slot, float clamp, float eps, float* sum,
             int32_t* points) {
    const fape_in a = FCZ_FAPE_IN();
    if (!fape_args_ok(ctx, a, layout, slot, clamp, eps, L) || !sum || !points || !bound_ok(false, length, n, L)) return FCZ_E_INVALID_ARG;
    return fape_host(ctx, a, length, false, n, L, layout, slot, clamp, eps, sum, points, nullptr, nullptr, nullptr, nullptr);
}

int fcz_fape_packed(fcz_ctx* ctx, FCZ_FAPE_INPUTS(), const uint32_t* row_off, uint32_t n, uint32_t R, int layout, int slot, float clamp, float eps, float* sum,
                    int32_t* points) {
    const fape_in a = FCZ_FAPE_IN();
    if (!fape_args_ok(ctx, a, layout, slot, clamp, eps, R) || !sum || !points || !bound_ok(true, row_off, n, R)) return FCZ_E_INVALID_ARG;
    return fape_host(ctx, a, row_off, true, n, R, layout, slot, clamp, eps, sum, points, nullptr, nullptr, nullptr, nullptr);
}

int fcz_fape_grad(fcz_ctx* ctx, FCZ_FAPE_INPUTS(), const uint32_t* length, uint32_t n, uint32_t L, int layout, int slot, float clamp, float eps,
                  const float* weight, float* grad_rot, float* grad_trans, float* grad_pos) {
    const fape_in a = FCZ_FAPE_IN();
    if (!fape_args_ok(ctx, a, layout, slot, clamp, eps, L) || !weight || !grad_rot || !grad_trans || !grad_pos || !bound_ok(false, length, n, L))
        return FCZ_E_INVALID_ARG;
    return fape_host(ctx, a, length, false, n, L, layout, slot, clamp, eps, nullptr, nullptr, weight, grad_rot, grad_trans, grad_pos);
}

int fcz_fape_grad_packed(fcz_ctx* ctx, FCZ_FAPE_INPUTS(), const uint32_t* row_off, uint32_t n, uint32_t R, int layout, int slot, float clamp, float eps,
                         const float* weight, float* grad_rot, float* grad_trans, float* grad_pos) {
    const fape_in a = FCZ_FAPE_IN();
    if (!fape_args_ok(ctx, a, layout, slot, clamp, eps, R) || !weight || !grad_rot || !grad_trans || !grad_pos || !bound_ok(true, row_off, n, R))
        return FCZ_E_INVALID_ARG;
    return fape_host(ctx, a, row_off, true, n, R, layout, slot, clamp, eps, nullptr, nullptr, weight, grad_rot, grad_trans, grad_pos);
}

#undef FCZ_FAPE_INPUTS
#undef FCZ_FAPE_IN

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// all-atom lDDT with symmetric side-chain renaming (fcz_lddt_atoms.h; no counterpart in the reference)
// ------------------------------------------------------------------------------------------------
// tab from swap_table [21][A] (NULL: the default) -> true when every entry lies inside its row and the row is an involution
static bool lddta_table_ok(int layout, const uint8_t* swap_table, lddta_table* tab) {
    const int A = fcz_dense_width(layout);
    if (A <= 0) return false;
    memset(tab->partner, 0, sizeof tab->partner);
    if (swap_table) memcpy(tab->partner, swap_table, LDDTA_TYPES * (size_t)A);
    else if (fcz_lddt_default_swaps(layout, tab->partner) != FCZ_OK) return false;
    for (int ty = 0; ty < (int)LDDTA_TYPES; ty++)
        for (int a = 0; a < A; a++) {
            const int p = tab->partner[ty * A + a];
            if (p >= A || tab->partner[ty * A + p] != a) return false;        // inside the row, and an involution
        }
    return true;
}

// rows: L (padded) or R (packed). Fills tab from swap_table (NULL: the default) when everything is acceptable.
static bool lddta_args_ok(const fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, int layout, float cutoff,
                          const float* thresholds, const uint8_t* swap_table, uint32_t rows, const fcz_lddt_atoms_out* out, lddta_table* tab) {
    const int A = fcz_dense_width(layout);
    if (!ctx || !pos_true || !mask_true || !pos_pred || !out || !out->score || !out->pairs || !out->hits || !out->swapped || A <= 0) return false;
    if (!std::isfinite(cutoff) || !(cutoff > 0.0f) || rows > (uint32_t)fcz_lddt_atoms_max_rows(layout)) return false;
    if (thresholds) for (int t = 0; t < 4; t++) if (std::isnan(thresholds[t])) return false;
    return lddta_table_ok(layout, swap_table, tab);
}

// fcz_lddt_atoms_dev (bound_dev is length [n] or NULL, rows = L) and fcz_lddt_atoms_packed_dev (bound_dev = row_off [n + 1], rows = R):
// the fill (packed), then the decide sweep over tiles of its own, then the score sweep, in stream order
static int lddta_rows(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev, const uint8_t* mask_pred_dev,
                      const uint8_t* aatype_dev, const uint32_t* bound_dev, bool packed, uint32_t n, uint32_t rows, int layout, float cutoff,
                      const float* thresholds, const lddta_table& tab, const fcz_lddt_atoms_out& o) {
    HIP_TRY(hipSetDevice(ctx->device));
    if (rows == 0 || (n == 0 && !packed)) return FCZ_OK;
    const float* th = thresholds ? thresholds : LDDT_THRESHOLDS;
    const lddta_args g{pos_true_dev, mask_true_dev, pos_pred_dev, mask_pred_dev, aatype_dev, bound_dev, n, rows, (uint32_t)fcz_dense_width(layout),
                       lddt_c2(cutoff), th[0], th[1], th[2], th[3], o.score, o.pairs, o.hits, o.swapped, o.atom_pairs, o.atom_hits};
    chain_tiles decide(ctx, packed, n, rows, lddta_tile_rows(g.A, true), 12u), score(ctx, packed, n, rows, lddta_tile_rows(g.A, false), 12u);
    int rc = decide.reserve(); if (rc) return rc;
    rc = score.reserve(); if (rc) return rc;                                  // (the same scratch: the decide sweep has read its tiles by then)
    span_guard sg(ctx, "lddt_atoms");
    rc = decide.run(bound_dev, [&] { hipLaunchKernelGGL(k_chain_fill<lddta_args>, decide.fill_grid(rows), dim3(BLOCK), 0, ctx->stream, g); },
                    [&](auto P, dim3 grid, const uint64_t* tile_off, uint32_t tiles_per_entry, uint64_t n_padded) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lddt_atoms<decltype(P)::value, true>), grid, dim3(BLOCK), 0, ctx->stream, g, tab, tile_off, tiles_per_entry, n_padded);
    });
    if (rc) return rc;
    return score.run(bound_dev, [] {}, [&](auto P, dim3 grid, const uint64_t* tile_off, uint32_t tiles_per_entry, uint64_t n_padded) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lddt_atoms<decltype(P)::value, false>), grid, dim3(BLOCK), 0, ctx->stream, g, tab, tile_off, tiles_per_entry, n_padded);
    });
}

// fcz_lddt_atoms and fcz_lddt_atoms_packed: the host arrays through DENSE_IN 0 .. 3, LDDT_PRED 4, 5 and LDDTA_OUT 10 .. 15
static int lddta_host(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, const uint8_t* mask_pred, const uint8_t* aatype,
                      const uint32_t* bound, bool packed, uint32_t n, uint32_t rows_per, int layout, float cutoff, const float* thresholds,
                      const lddta_table& tab, const fcz_lddt_atoms_out& o) {
    const dense_bytes b(packed, n, rows_per, layout, bound);
    const size_t r = b.rows;
    return staged_call(ctx, {{pos_true, b.pos, DENSE_IN}, {mask_true, b.mask, DENSE_IN + 1}, {aatype, r, DENSE_IN + 2}, {bound, b.bound, DENSE_IN + 3},
                             {pos_pred, b.pos, LDDT_PRED}, {mask_pred, b.mask, LDDT_PRED + 1}},
                       {{o.score, r * 4, LDDTA_OUT}, {o.pairs, r * 4, LDDTA_OUT + 1}, {o.hits, r * 4, LDDTA_OUT + 2}, {o.swapped, r, LDDTA_OUT + 3},
                        {o.atom_pairs, b.mask * 4, LDDTA_OUT + 4}, {o.atom_hits, b.mask * 4, LDDTA_OUT + 5}},
                       [&](const void* const* in, void* const* out) {
        const fcz_lddt_atoms_out d{(float*)out[0], (int32_t*)out[1], (int32_t*)out[2], (uint8_t*)out[3], (int32_t*)out[4], (int32_t*)out[5]};
        return lddta_rows(ctx, (const float*)in[0], (const uint8_t*)in[1], (const float*)in[4], (const uint8_t*)in[5], (const uint8_t*)in[2],
                          (const uint32_t*)in[3], packed, n, rows_per, layout, cutoff, thresholds, tab, d);
    });
}

extern "C" {

int fcz_lddt_atoms_pass(void) { return (int)LDDTA_PASS; }

int fcz_lddt_atoms_max_rows(int layout) {
    const int A = fcz_dense_width(layout);
    return A > 0 ? (int)lddta_max_rows((uint32_t)A) : -1;
}

int fcz_lddt_default_swaps(int layout, uint8_t* out) {
    const int A = fcz_dense_width(layout);
    if (A <= 0 || !out) return FCZ_E_INVALID_ARG;
    for (int ty = 0; ty < (int)LDDTA_TYPES; ty++)
        for (int a = 0; a < A; a++) out[ty * A + a] = (uint8_t)a;
    // the renamings of AlphaFold's residue_atom_renaming_swaps: ASP, GLU, PHE, TYR by their aatype (= residue code)
    static const struct { int type; const char* a; const char* b; } swaps[] = {{3, "OD1", "OD2"}, {6, "OE1", "OE2"}, {13, "CD1", "CD2"}, {13, "CE1", "CE2"},
                                                                               {18, "CD1", "CD2"}, {18, "CE1", "CE2"}};
    for (const auto& s : swaps) {
        const int x = fcz_dense_slot(layout, s.type, fcz_atom_code_from_name(s.a)), y = fcz_dense_slot(layout, s.type, fcz_atom_code_from_name(s.b));
        if (x < 0 || y < 0) continue;                                         // (backbone4 holds neither)
        out[s.type * A + x] = (uint8_t)y; out[s.type * A + y] = (uint8_t)x;
    }
    return FCZ_OK;
}

int fcz_lddt_atoms_dev(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev, const uint8_t* mask_pred_dev,
                       const uint8_t* aatype_dev, const uint32_t* length_dev, uint32_t n, uint32_t L, int layout, float cutoff, const float* thresholds,
                       const uint8_t* swap_table, const fcz_lddt_atoms_out* out_dev) {
    lddta_table tab;
    if (!lddta_args_ok(ctx, pos_true_dev, mask_true_dev, pos_pred_dev, layout, cutoff, thresholds, swap_table, L, out_dev, &tab) ||
        !bound_ok(false, length_dev, n, L))
        return FCZ_E_INVALID_ARG;
    return lddta_rows(ctx, pos_true_dev, mask_true_dev, pos_pred_dev, mask_pred_dev, aatype_dev, length_dev, false, n, L, layout, cutoff, thresholds, tab, *out_dev);
}

int fcz_lddt_atoms_packed_dev(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev, const uint8_t* mask_pred_dev,
                              const uint8_t* aatype_dev, const uint32_t* row_off_dev, uint32_t n, uint32_t R, int layout, float cutoff, const float* thresholds,
                              const uint8_t* swap_table, const fcz_lddt_atoms_out* out_dev) {
    lddta_table tab;
    if (!lddta_args_ok(ctx, pos_true_dev, mask_true_dev, pos_pred_dev, layout, cutoff, thresholds, swap_table, R, out_dev, &tab) ||
        !bound_ok(true, row_off_dev, n, R))
        return FCZ_E_INVALID_ARG;
    return lddta_rows(ctx, pos_true_dev, mask_true_dev, pos_pred_dev, mask_pred_dev, aatype_dev, row_off_dev, true, n, R, layout, cutoff, thresholds, tab, *out_dev);
}

int fcz_lddt_atoms(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, const uint8_t* mask_pred, const uint8_t* aatype,
                   const uint32_t* length, uint32_t n, uint32_t L, int layout, float cutoff, const float* thresholds, const uint8_t* swap_table,
                   const fcz_lddt_atoms_out* out) {
    lddta_table tab;
    if (!lddta_args_ok(ctx, pos_true, mask_true, pos_pred, layout, cutoff, thresholds, swap_table, L, out, &tab) || !bound_ok(false, length, n, L))
        return FCZ_E_INVALID_ARG;
    return lddta_host(ctx, pos_true, mask_true, pos_pred, mask_pred, aatype, length, false, n, L, layout, cutoff, thresholds, tab, *out);
}

int fcz_lddt_atoms_packed(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, const uint8_t* mask_pred,
                          const uint8_t* aatype, const uint32_t* row_off, uint32_t n, uint32_t R, int layout, float cutoff, const float* thresholds,
                          const uint8_t* swap_table, const fcz_lddt_atoms_out* out) {
    lddta_table tab;
    if (!lddta_args_ok(ctx, pos_true, mask_true, pos_pred, layout, cutoff, thresholds, swap_table, R, out, &tab) || !bound_ok(true, row_off, n, R))
        return FCZ_E_INVALID_ARG;
    return lddta_host(ctx, pos_true, mask_true, pos_pred, mask_pred, aatype, row_off, true, n, R, layout, cutoff, thresholds, tab, *out);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// all-atom FAPE over the eight rigid groups and its gradient (fcz_fape_atoms.h; no counterpart in the reference)
// ------------------------------------------------------------------------------------------------
// the fourteen input arrays of a call, device or host pointers, in the order of the entry points' arguments
struct fapea_in {
    const float* rot_true; const float* trans_true; const uint8_t* fmask_true; const float* pos_true; const uint8_t* mask_true;
    const uint8_t* aatype; const uint8_t* swapped;
    const float* rot_pred; const float* trans_pred; const uint8_t* fmask_pred; const float* pos_pred; const uint8_t* mask_pred;
};

// the outputs are checked by the caller. rows: L (padded) or R (packed). Fills tab when everything is acceptable.
static bool fapea_args_ok(const fcz_ctx* ctx, const fapea_in& a, int layout, float clamp, float eps, const uint8_t* swap_table, uint32_t rows, fapea_table* tab) {
    if (!ctx || !a.rot_true || !a.trans_true || !a.fmask_true || !a.pos_true || !a.mask_true || !a.rot_pred || !a.trans_pred || !a.pos_pred) return false;
    const int A = fcz_dense_width(layout);
    if (A <= 0 || (a.swapped && !a.aatype)) return false;
    if (std::isnan(clamp) || !(clamp > 0.0f) || !std::isfinite(eps) || !(eps > 0.0f) || rows > fapea_max_rows((uint32_t)A)) return false;
    if (!lddta_table_ok(layout, swap_table, &tab->swap)) return false;
    for (int ty = 0; ty < (int)LDDTA_TYPES; ty++) {
        tab->alt[ty] = 0;
        if (ty >= 20 || layout == FCZ_DENSE_BACKBONE4) continue;              // (type 20 has no ambiguity; backbone4 renames nothing)
        for (int g = 0; g < (int)FAPEA_GROUPS; g++) tab->alt[ty] |= (uint8_t)(fcz_frame_ambiguous(ty, g) ? 1u << g : 0u);
    }
    return true;
}

// the device forms of the value (weight_dev and the gradients NULL) and of the gradient (sum_dev and points_dev NULL). The gradient
// is two sweeps over tiles of their own behind one fill, in one span.
static int fapea_rows(fcz_ctx* ctx, const fapea_in& a, const uint32_t* bound_dev, bool packed, uint32_t n, uint32_t rows, int layout, float clamp, float eps,
                      const fapea_table& tab, float* sum_dev, int32_t* points_dev, const float* weight_dev, float* grad_rot_dev, float* grad_trans_dev,
                      float* grad_pos_dev) {
    HIP_TRY(hipSetDevice(ctx->device));
    if (rows == 0 || (n == 0 && !packed)) return FCZ_OK;
    const uint32_t A = (uint32_t)fcz_dense_width(layout);
    chain_tiles frames(ctx, packed, n, rows, fapea_tile_rows(A), 12u);
    int rc = frames.reserve(); if (rc) return rc;
    if (grad_rot_dev) {
        const fapea_grad_args g{a.rot_true, a.trans_true, a.fmask_true, a.pos_true, a.mask_true, a.aatype, a.swapped, a.rot_pred, a.trans_pred, a.fmask_pred,
                                a.pos_pred, a.mask_pred, bound_dev, n, rows, A, clamp, eps, weight_dev, grad_rot_dev, grad_trans_dev, grad_pos_dev};
        chain_tiles atoms(ctx, packed, n, rows, lddta_tile_rows(A, false), 12u);
        rc = atoms.reserve(); if (rc) return rc;                              // (the same scratch: the frame sweep has read its tiles by then)
        span_guard sg(ctx, "fape_atoms_grad");
        rc = frames.run(bound_dev, [&] { hipLaunchKernelGGL(k_chain_fill<fapea_grad_args>, frames.fill_grid(rows), dim3(BLOCK), 0, ctx->stream, g); },
                        [&](auto P, dim3 grid, const uint64_t* tile_off, uint32_t tiles_per_entry, uint64_t n_padded) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fape_atoms_grad_frames<decltype(P)::value>), grid, dim3(BLOCK), 0, ctx->stream, g, tab, tile_off, tiles_per_entry, n_padded);
        });
        if (rc) return rc;
        return atoms.run(bound_dev, [] {}, [&](auto P, dim3 grid, const uint64_t* tile_off, uint32_t tiles_per_entry, uint64_t n_padded) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fape_atoms_grad_points<decltype(P)::value>), grid, dim3(BLOCK), 0, ctx->stream, g, tab, tile_off, tiles_per_entry, n_padded);
        });
    }
    const fapea_args g{a.rot_true, a.trans_true, a.fmask_true, a.pos_true, a.mask_true, a.aatype, a.swapped, a.rot_pred, a.trans_pred, a.fmask_pred,
                       a.pos_pred, a.mask_pred, bound_dev, n, rows, A, clamp, eps, sum_dev, points_dev};
    span_guard sg(ctx, "fape_atoms");
    return frames.run(bound_dev, [&] { hipLaunchKernelGGL(k_chain_fill<fapea_args>, frames.fill_grid(rows), dim3(BLOCK), 0, ctx->stream, g); },
                      [&](auto P, dim3 grid, const uint64_t* tile_off, uint32_t tiles_per_entry, uint64_t n_padded) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fape_atoms<decltype(P)::value>), grid, dim3(BLOCK), 0, ctx->stream, g, tab, tile_off, tiles_per_entry, n_padded);
    });
}

// the host forms: the host arrays through DENSE_IN 0 .. 3, LDDT_PRED 4, 5, LDDT_WEIGHT 6, FAPE_FRAMES 7 .. 12, FAPEA_SWAPPED 16 and FAPE_OUT 13 .. 14
// (sum, points) or 13 .. 15 (grad_rot, grad_trans, grad_pos)
static int fapea_host(fcz_ctx* ctx, const fapea_in& a, const uint32_t* bound, bool packed, uint32_t n, uint32_t rows_per, int layout, float clamp, float eps,
                      const fapea_table& tab, float* sum, int32_t* points, const float* weight, float* grad_rot, float* grad_trans, float* grad_pos) {
    const dense_bytes b(packed, n, rows_per, layout, bound);
    const size_t items = b.rows * FAPEA_GROUPS, no = items * 4;
    auto run = [&](const void* const* in, void* const* out) {
        const fapea_in d{(const float*)in[7], (const float*)in[8], (const uint8_t*)in[9], (const float*)in[0], (const uint8_t*)in[1], (const uint8_t*)in[2],
                         (const uint8_t*)in[13], (const float*)in[10], (const float*)in[11], (const uint8_t*)in[12], (const float*)in[4], (const uint8_t*)in[5]};
        const bool grad = grad_rot != nullptr;
        return fapea_rows(ctx, d, (const uint32_t*)in[3], packed, n, rows_per, layout, clamp, eps, tab, grad ? nullptr : (float*)out[0],
                          grad ? nullptr : (int32_t*)out[1], (const float*)in[6], grad ? (float*)out[0] : nullptr, grad ? (float*)out[1] : nullptr,
                          grad ? (float*)out[2] : nullptr);
    };
    const std::initializer_list<staged_in> in = {
        {a.pos_true, b.pos, DENSE_IN}, {a.mask_true, b.mask, DENSE_IN + 1}, {a.aatype, b.rows, DENSE_IN + 2}, {bound, b.bound, DENSE_IN + 3},
        {a.pos_pred, b.pos, LDDT_PRED}, {a.mask_pred, b.mask, LDDT_PRED + 1}, {weight, no, LDDT_WEIGHT}, {a.rot_true, 9 * no, FAPE_FRAMES},
        {a.trans_true, 3 * no, FAPE_FRAMES + 1}, {a.fmask_true, items, FAPE_FRAMES + 2}, {a.rot_pred, 9 * no, FAPE_FRAMES + 3},
        {a.trans_pred, 3 * no, FAPE_FRAMES + 4}, {a.fmask_pred, items, FAPE_FRAMES + 5}, {a.swapped, b.rows, FAPEA_SWAPPED}};
    if (grad_rot) return staged_call(ctx, in, {{grad_rot, 9 * no, FAPE_OUT}, {grad_trans, 3 * no, FAPE_OUT + 1}, {grad_pos, b.pos, FAPE_OUT + 2}}, run);
    return staged_call(ctx, in, {{sum, no, FAPE_OUT}, {points, no, FAPE_OUT + 1}}, run);
}

extern "C" {

int fcz_fape_atoms_pass(void) { return (int)FAPEA_PASS; }

int fcz_fape_atoms_tile_rows(int layout) {
    const int A = fcz_dense_width(layout);
    return A > 0 ? (int)fapea_tile_rows((uint32_t)A) : -1;
}

#define FCZ_FAPEA_INPUTS(S) const float* rot_true##S, const float* trans_true##S, const uint8_t* fmask_true##S, const float* pos_true##S, \
    const uint8_t* mask_true##S, const uint8_t* aatype##S, const uint8_t* swapped##S, const float* rot_pred##S, const float* trans_pred##S, \
    const uint8_t* fmask_pred##S, const float* pos_pred##S, const uint8_t* mask_pred##S
#define FCZ_FAPEA_IN(S) fapea_in{rot_true##S, trans_true##S, fmask_true##S, pos_true##S, mask_true##S, aatype##S, swapped##S, rot_pred##S, trans_pred##S, \
                                 fmask_pred##S, pos_pred##S, mask_pred##S}
// the eight entry points differ in the name of the bound, the form and the outputs
#define FCZ_FAPEA_VALUE(NAME, S, BOUND, ROWS, PACKED, CALL) \
    int NAME(fcz_ctx* ctx, FCZ_FAPEA_INPUTS(S), const uint32_t* BOUND, uint32_t n, uint32_t ROWS, int layout, float clamp, float eps, \
             const uint8_t* swap_table, float* sum##S, int32_t* points##S) { \
        const fapea_in a = FCZ_FAPEA_IN(S); \
        fapea_table tab; \
        if (!sum##S || !points##S || !bound_ok(PACKED, BOUND, n, ROWS) || !fapea_args_ok(ctx, a, layout, clamp, eps, swap_table, ROWS, &tab)) \
            return FCZ_E_INVALID_ARG; \
        return CALL(ctx, a, BOUND, PACKED, n, ROWS, layout, clamp, eps, tab, sum##S, points##S, nullptr, nullptr, nullptr, nullptr); \
    }
#define FCZ_FAPEA_GRAD(NAME, S, BOUND, ROWS, PACKED, CALL) \
    int NAME(fcz_ctx* ctx, FCZ_FAPEA_INPUTS(S), const uint32_t* BOUND, uint32_t n, uint32_t ROWS, int layout, float clamp, float eps, \
             const uint8_t* swap_table, const float* weight##S, float* grad_rot##S, float* grad_trans##S, float* grad_pos##S) { \
        const fapea_in a = FCZ_FAPEA_IN(S); \
        fapea_table tab; \
        if (!weight##S || !grad_rot##S || !grad_trans##S || !grad_pos##S || !bound_ok(PACKED, BOUND, n, ROWS) || \
            !fapea_args_ok(ctx, a, layout, clamp, eps, swap_table, ROWS, &tab)) \
            return FCZ_E_INVALID_ARG; \
        return CALL(ctx, a, BOUND, PACKED, n, ROWS, layout, clamp, eps, tab, nullptr, nullptr, weight##S, grad_rot##S, grad_trans##S, grad_pos##S); \
    }

FCZ_FAPEA_VALUE(fcz_fape_atoms_dev, _dev, length_dev, L, false, fapea_rows)
FCZ_FAPEA_VALUE(fcz_fape_atoms_packed_dev, _dev, row_off_dev, R, true, fapea_rows)
FCZ_FAPEA_GRAD(fcz_fape_atoms_grad_dev, _dev, length_dev, L, false, fapea_rows)
FCZ_FAPEA_GRAD(fcz_fape_atoms_grad_packed_dev, _dev, row_off_dev, R, true, fapea_rows)
FCZ_FAPEA_VALUE(fcz_fape_atoms, , length, L, false, fapea_host)
FCZ_FAPEA_VALUE(fcz_fape_atoms_packed, , row_off, R, true, fapea_host)
FCZ_FAPEA_GRAD(fcz_fape_atoms_grad, , length, L, false, fapea_host)
FCZ_FAPEA_GRAD(fcz_fape_atoms_grad_packed, , row_off, R, true, fapea_host)

#undef FCZ_FAPEA_INPUTS
#undef FCZ_FAPEA_IN
#undef FCZ_FAPEA_VALUE
#undef FCZ_FAPEA_GRAD

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// backbone hydrogen bonds and DSSP secondary structure of dense tensors (fcz_dssp.h; no counterpart in the reference)
// ------------------------------------------------------------------------------------------------
// rows: L (padded) or R (packed); out: every output pointer of the call
static bool dssp_args_ok(const fcz_ctx* ctx, const float* pos, const uint8_t* mask, int layout, uint32_t rows, std::initializer_list<const void*> out) {
    if (!ctx || !pos || !mask || fcz_dense_width(layout) <= 0 || rows > DSSP_MAX_ROWS) return false;
    for (const void* p : out) if (!p) return false;
    return true;
}

static dssp_args dssp_pack(const float* pos, const uint8_t* mask, const uint8_t* aatype, const uint32_t* bound, uint32_t n, uint32_t rows, int layout) {
    dssp_args g{};
    g.pos = pos; g.mask = mask; g.aatype = aatype; g.bound = bound; g.n = n; g.L = rows;
    g.A = (uint32_t)fcz_dense_width(layout); g.o_slot = layout == FCZ_DENSE_ATOM37 ? 4u : 3u;
    return g;
}

// fcz_hbond_dev (bound_dev is length [n] or NULL, rows = L) and fcz_hbond_packed_dev (bound_dev = row_off [n + 1], rows = R)
static int hbond_rows(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint8_t* aatype_dev, const uint32_t* bound_dev, bool packed, uint32_t n,
                      uint32_t rows, int layout, int32_t* acc_index_dev, float* acc_energy_dev, int32_t* don_index_dev, float* don_energy_dev) {
    HIP_TRY(hipSetDevice(ctx->device));
    if (rows == 0 || (n == 0 && !packed)) return FCZ_OK;
    dssp_args g = dssp_pack(pos_dev, mask_dev, aatype_dev, bound_dev, n, rows, layout);
    g.acc_index = acc_index_dev; g.acc_energy = acc_energy_dev; g.don_index = don_index_dev; g.don_energy = don_energy_dev;
    chain_tiles ct(ctx, packed, n, rows);
    int rc = ct.reserve(); if (rc) return rc;
    span_guard sg(ctx, "dssp");
    return ct.run(bound_dev, [&] { hipLaunchKernelGGL(k_chain_fill<hbond_fill_args>, ct.fill_grid(rows), dim3(BLOCK), 0, ctx->stream, hbond_fill_args{g}); },
                  [&](auto P, dim3 grid, const uint64_t* tile_off, uint32_t tiles_per_entry, uint64_t n_padded) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_hbond<decltype(P)::value>), grid, dim3(BLOCK), 0, ctx->stream, g, tile_off, tiles_per_entry, n_padded);
    });
}

// fcz_dssp_labels_dev and fcz_dssp_labels_packed_dev: the flags of every row into ctx->dssp_flags, then the labels from them and the table
static int dssp_label_rows(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint8_t* aatype_dev, const uint32_t* bound_dev, bool packed,
                           uint32_t n, uint32_t rows, int layout, const int32_t* acc_index_dev, const float* acc_energy_dev, uint8_t* ss_dev, uint8_t* ss_mask_dev) {
    HIP_TRY(hipSetDevice(ctx->device));
    if (rows == 0 || (n == 0 && !packed)) return FCZ_OK;
    dssp_args g = dssp_pack(pos_dev, mask_dev, aatype_dev, bound_dev, n, rows, layout);
    g.acc_index = const_cast<int32_t*>(acc_index_dev); g.acc_energy = const_cast<float*>(acc_energy_dev); g.ss = ss_dev; g.ss_mask = ss_mask_dev;
    chain_tiles ct(ctx, packed, n, rows);
    int rc = ct.reserve(); if (rc) return rc;
    if (!packed || n) {                                                       // (no chain: the fill alone runs, and it writes no flag)
        if ((rc = ctx->dssp_flags.ensure(packed ? (size_t)rows : (size_t)n * rows))) return rc;
        g.flags = ctx->dssp_flags.as<uint8_t>();
    }
    span_guard sg(ctx, "dssp");
    return ct.run(bound_dev, [&] { hipLaunchKernelGGL(k_chain_fill<label_fill_args>, ct.fill_grid(rows), dim3(BLOCK), 0, ctx->stream, label_fill_args{g}); },
                  [&](auto P, dim3 grid, const uint64_t* tile_off, uint32_t tiles_per_entry, uint64_t n_padded) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dssp_flags<decltype(P)::value>), grid, dim3(BLOCK), 0, ctx->stream, g, tile_off, tiles_per_entry, n_padded);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dssp_labels<decltype(P)::value>), grid, dim3(BLOCK), 0, ctx->stream, g, tile_off, tiles_per_entry, n_padded);
    });
}

// fcz_dssp and fcz_dssp_packed: the host arrays through DENSE_IN 0 .. 3 and DSSP_OUT 10 .. 15, both steps
static int dssp_host(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint8_t* aatype, const uint32_t* bound, bool packed, uint32_t n, uint32_t rows_per,
                     int layout, int32_t* acc_index, float* acc_energy, int32_t* don_index, float* don_energy, uint8_t* ss, uint8_t* ss_mask) {
    const dense_bytes b(packed, n, rows_per, layout, bound);
    const size_t nt = b.rows * 2 * 4;
    return staged_call(ctx, {{pos, b.pos, DENSE_IN}, {mask, b.mask, DENSE_IN + 1}, {aatype, b.rows, DENSE_IN + 2}, {bound, b.bound, DENSE_IN + 3}},
                       {{acc_index, nt, DSSP_OUT}, {acc_energy, nt, DSSP_OUT + 1}, {don_index, nt, DSSP_OUT + 2}, {don_energy, nt, DSSP_OUT + 3},
                        {ss, b.rows, DSSP_OUT + 4}, {ss_mask, b.rows, DSSP_OUT + 5}},
                       [&](const void* const* in, void* const* out) {
        const float* pos_dev = (const float*)in[0];
        const uint8_t* mask_dev = (const uint8_t*)in[1], * aatype_dev = (const uint8_t*)in[2];
        const uint32_t* bound_dev = (const uint32_t*)in[3];
        int rc = hbond_rows(ctx, pos_dev, mask_dev, aatype_dev, bound_dev, packed, n, rows_per, layout, (int32_t*)out[0], (float*)out[1], (int32_t*)out[2], (float*)out[3]);
        if (rc) return rc;
        return dssp_label_rows(ctx, pos_dev, mask_dev, aatype_dev, bound_dev, packed, n, rows_per, layout, (int32_t*)out[0], (float*)out[1], (uint8_t*)out[4],
                               (uint8_t*)out[5]);
    });
}

extern "C" {

int fcz_hbond_pass(void) { return (int)HBOND_PASS; }

int fcz_hbond_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint8_t* aatype_dev, const uint32_t* length_dev, uint32_t n, uint32_t L,
                  int layout, int32_t* acc_index_dev, float* acc_energy_dev, int32_t* don_index_dev, float* don_energy_dev) {
    if (!dssp_args_ok(ctx, pos_dev, mask_dev, layout, L, {acc_index_dev, acc_energy_dev, don_index_dev, don_energy_dev}) || !bound_ok(false, length_dev, n, L))
        return FCZ_E_INVALID_ARG;
    return hbond_rows(ctx, pos_dev, mask_dev, aatype_dev, length_dev, false, n, L, layout, acc_index_dev, acc_energy_dev, don_index_dev, don_energy_dev);
}

int fcz_hbond_packed_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint8_t* aatype_dev, const uint32_t* row_off_dev, uint32_t n,
                         uint32_t R, int layout, int32_t* acc_index_dev, float* acc_energy_dev, int32_t* don_index_dev, float* don_energy_dev) {
    if (!dssp_args_ok(ctx, pos_dev, mask_dev, layout, R, {acc_index_dev, acc_energy_dev, don_index_dev, don_energy_dev}) || !bound_ok(true, row_off_dev, n, R))
        return FCZ_E_INVALID_ARG;
    return hbond_rows(ctx, pos_dev, mask_dev, aatype_dev, row_off_dev, true, n, R, layout, acc_index_dev, acc_energy_dev, don_index_dev, don_energy_dev);
}

int fcz_dssp_labels_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint8_t* aatype_dev, const uint32_t* length_dev, uint32_t n,
                        uint32_t L, int layout, const int32_t* acc_index_dev, const float* acc_energy_dev, uint8_t* ss_dev, uint8_t* ss_mask_dev) {
    if (!dssp_args_ok(ctx, pos_dev, mask_dev, layout, L, {acc_index_dev, acc_energy_dev, ss_dev, ss_mask_dev}) || !bound_ok(false, length_dev, n, L))
        return FCZ_E_INVALID_ARG;
    return dssp_label_rows(ctx, pos_dev, mask_dev, aatype_dev, length_dev, false, n, L, layout, acc_index_dev, acc_energy_dev, ss_dev, ss_mask_dev);
}

int fcz_dssp_labels_packed_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint8_t* aatype_dev, const uint32_t* row_off_dev, uint32_t n,
                               uint32_t R, int layout, const int32_t* acc_index_dev, const float* acc_energy_dev, uint8_t* ss_dev, uint8_t* ss_mask_dev) {
    if (!dssp_args_ok(ctx, pos_dev, mask_dev, layout, R, {acc_index_dev, acc_energy_dev, ss_dev, ss_mask_dev}) || !bound_ok(true, row_off_dev, n, R))
        return FCZ_E_INVALID_ARG;
    return dssp_label_rows(ctx, pos_dev, mask_dev, aatype_dev, row_off_dev, true, n, R, layout, acc_index_dev, acc_energy_dev, ss_dev, ss_mask_dev);
}

int fcz_dssp(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint8_t* aatype, const uint32_t* length, uint32_t n, uint32_t L, int layout,
             int32_t* acc_index, float* acc_energy, int32_t* don_index, float* don_energy, uint8_t* ss, uint8_t* ss_mask) {
    if (!dssp_args_ok(ctx, pos, mask, layout, L, {acc_index, acc_energy, don_index, don_energy, ss, ss_mask}) || !bound_ok(false, length, n, L))
        return FCZ_E_INVALID_ARG;
    return dssp_host(ctx, pos, mask, aatype, length, false, n, L, layout, acc_index, acc_energy, don_index, don_energy, ss, ss_mask);
}

int fcz_dssp_packed(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint8_t* aatype, const uint32_t* row_off, uint32_t n, uint32_t R, int layout,
                    int32_t* acc_index, float* acc_energy, int32_t* don_index, float* don_energy, uint8_t* ss, uint8_t* ss_mask) {
    if (!dssp_args_ok(ctx, pos, mask, layout, R, {acc_index, acc_energy, don_index, don_energy, ss, ss_mask}) || !bound_ok(true, row_off, n, R))
        return FCZ_E_INVALID_ARG;
    return dssp_host(ctx, pos, mask, aatype, row_off, true, n, R, layout, acc_index, acc_energy, don_index, don_energy, ss, ss_mask);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// per-residue solvent accessibility of dense tensors (fcz_sasa.h; no counterpart in the reference)
// ------------------------------------------------------------------------------------------------
// Bondi's radius of the element an atom's name begins with; 0: no such element among the twenty types
static float sasa_element_radius(const char* name) {
    switch (name[0]) { case 'C': return 1.70f; case 'N': return 1.55f; case 'O': return 1.52f; case 'S': return 1.80f; default: return 0.0f; }
}

// rows: L (padded) or R (packed). Fills tab from radius_table (NULL: the default) when everything is acceptable.
static bool sasa_args_ok(const fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint8_t* aatype, int layout, uint32_t rows, const float* radius_table,
                         float probe, const float* points, uint32_t n_points, std::initializer_list<const void*> out, chain_radii* tab) {
    const int A = fcz_dense_width(layout);
    if (!ctx || !pos || !mask || !points || A <= 0 || rows > SASA_MAX_ROWS) return false;
    for (const void* p : out) if (!p) return false;
    if (n_points < 1 || n_points > SASA_MAX_POINTS || !std::isfinite(probe) || probe < 0.0f) return false;
    if (layout == FCZ_DENSE_ATOM14 && !aatype) return false;                  // a slot's atom depends on the type there
    memset(tab->radius, 0, sizeof tab->radius);
    if (radius_table) memcpy(tab->radius, radius_table, sizeof(float) * CHAIN_TYPES * (size_t)A);
    else if (fcz_sasa_default_radii(layout, tab->radius) != FCZ_OK) return false;
    for (int i = 0; i < (int)CHAIN_TYPES * A; i++) {
        const float r = tab->radius[i];
        if (r == 0.0f) continue;                                              // no atom in this slot
        const volatile float R = r + probe;                                   // (one float32 addition, as the kernel's)
        if (!(R >= 0.5f && R < 8.0f)) return false;                           // (a NaN radius ends here)
    }
    return true;
}

// fcz_sasa_dev (bound_dev is length [n] or NULL, rows = L) and fcz_sasa_packed_dev (bound_dev = row_off [n + 1], rows = R)
static int sasa_rows(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint8_t* aatype_dev, const uint32_t* bound_dev, bool packed, uint32_t n,
                     uint32_t rows, int layout, const chain_radii& tab, float probe, const float* points_dev, uint32_t n_points, int16_t* sasa_points_dev,
                     float* sasa_dev, uint8_t* sasa_mask_dev) {
    HIP_TRY(hipSetDevice(ctx->device));
    if (rows == 0 || (n == 0 && !packed)) return FCZ_OK;
    sasa_args g{};
    g.pos = pos_dev; g.mask = mask_dev; g.aatype = aatype_dev; g.bound = bound_dev; g.n = n; g.L = rows;
    g.A = (uint32_t)fcz_dense_width(layout); g.P = n_points; g.probe = probe; g.points = points_dev;
    g.scale = 0x1.921fb54442d18p+3 / (double)n_points;                        // 4 pi / P: one double division
    g.sasa_points = sasa_points_dev; g.sasa = sasa_dev; g.sasa_mask = sasa_mask_dev;
    const bool small = n_points <= SASA_SMALL_POINTS;
    chain_tiles ct(ctx, packed, n, rows, SASA_TILE_ROWS);
    int rc = ct.reserve(); if (rc) return rc;
    span_guard sg(ctx, "sasa");
    return ct.run(bound_dev, [&] { hipLaunchKernelGGL(k_chain_fill<sasa_args>, ct.fill_grid(rows), dim3(BLOCK), 0, ctx->stream, g); },
                  [&](auto P, dim3 grid, const uint64_t* tile_off, uint32_t tiles_per_entry, uint64_t n_padded) {
        if (small) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sasa_points<decltype(P)::value, true>), grid, dim3(BLOCK), 0, ctx->stream, g, tab, tile_off, tiles_per_entry, n_padded);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sasa_points<decltype(P)::value, false>), grid, dim3(BLOCK), 0, ctx->stream, g, tab, tile_off, tiles_per_entry, n_padded);
    });
}

// fcz_sasa and fcz_sasa_packed: the host arrays through DENSE_IN 0 .. 3, SASA_POINTS 4 and SASA_OUT 10 .. 12
static int sasa_host(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint8_t* aatype, const uint32_t* bound, bool packed, uint32_t n, uint32_t rows_per,
                     int layout, const chain_radii& tab, float probe, const float* points, uint32_t n_points, int16_t* sasa_points, float* sasa, uint8_t* sasa_mask) {
    const dense_bytes b(packed, n, rows_per, layout, bound);
    return staged_call(ctx, {{pos, b.pos, DENSE_IN}, {mask, b.mask, DENSE_IN + 1}, {aatype, b.rows, DENSE_IN + 2}, {bound, b.bound, DENSE_IN + 3},
                             {points, (size_t)n_points * 3 * sizeof(float), SASA_POINTS}},
                       {{sasa_points, b.mask * sizeof(int16_t), SASA_OUT}, {sasa, b.rows * sizeof(float), SASA_OUT + 1}, {sasa_mask, b.rows, SASA_OUT + 2}},
                       [&](const void* const* in, void* const* out) {
        return sasa_rows(ctx, (const float*)in[0], (const uint8_t*)in[1], (const uint8_t*)in[2], (const uint32_t*)in[3], packed, n, rows_per, layout, tab, probe,
                         (const float*)in[4], n_points, (int16_t*)out[0], (float*)out[1], (uint8_t*)out[2]);
    });
}

extern "C" {

int fcz_sasa_pass(void) { return (int)SASA_PASS; }

int fcz_sasa_default_radii(int layout, float* out) {
    const int A = fcz_dense_width(layout);
    if (A <= 0 || !out) return FCZ_E_INVALID_ARG;
    float own[FCZ_N_RES_CODES][DN_MAX_WIDTH] = {}, any[DN_MAX_WIDTH] = {};    // per residue code, and over all of them
    for (int rc = 0; rc < FCZ_N_RES_CODES; rc++)
        for (int j = 0; j < host_tab::h_res_natoms[rc]; j++) {
            const int ac = host_tab::h_res_atom[rc][j], slot = fcz_dense_slot(layout, rc, ac);
            if (slot >= 0) own[rc][slot] = any[slot] = sasa_element_radius(host_tab::h_atom_name[ac]);
        }
    // atom14: a slot's atom depends on the type (row 20: the backbone-only codes). atom37 / backbone4: a slot holds the same atom in
    // every type, so every row is the same and the mask alone says which atoms a residue has. OXT is in no residue's table: 0.
    for (int ty = 0; ty < (int)CHAIN_TYPES; ty++)
        for (int a = 0; a < A; a++) out[ty * A + a] = layout == FCZ_DENSE_ATOM14 ? own[ty][a] : any[a];
    return FCZ_OK;
}

int fcz_sasa_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint8_t* aatype_dev, const uint32_t* length_dev, uint32_t n, uint32_t L,
                 int layout, const float* radius_table, float probe, const float* points_dev, uint32_t n_points, int16_t* sasa_points_dev, float* sasa_dev,
                 uint8_t* sasa_mask_dev) {
    chain_radii tab;
    if (!sasa_args_ok(ctx, pos_dev, mask_dev, aatype_dev, layout, L, radius_table, probe, points_dev, n_points, {sasa_points_dev, sasa_dev, sasa_mask_dev}, &tab) ||
        !bound_ok(false, length_dev, n, L))
        return FCZ_E_INVALID_ARG;
    return sasa_rows(ctx, pos_dev, mask_dev, aatype_dev, length_dev, false, n, L, layout, tab, probe, points_dev, n_points, sasa_points_dev, sasa_dev, sasa_mask_dev);
}

int fcz_sasa_packed_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint8_t* aatype_dev, const uint32_t* row_off_dev, uint32_t n, uint32_t R,
                        int layout, const float* radius_table, float probe, const float* points_dev, uint32_t n_points, int16_t* sasa_points_dev,
                        float* sasa_dev, uint8_t* sasa_mask_dev) {
    chain_radii tab;
    if (!sasa_args_ok(ctx, pos_dev, mask_dev, aatype_dev, layout, R, radius_table, probe, points_dev, n_points, {sasa_points_dev, sasa_dev, sasa_mask_dev}, &tab) ||
        !bound_ok(true, row_off_dev, n, R))
        return FCZ_E_INVALID_ARG;
    return sasa_rows(ctx, pos_dev, mask_dev, aatype_dev, row_off_dev, true, n, R, layout, tab, probe, points_dev, n_points, sasa_points_dev, sasa_dev, sasa_mask_dev);
}

int fcz_sasa(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint8_t* aatype, const uint32_t* length, uint32_t n, uint32_t L, int layout,
             const float* radius_table, float probe, const float* points, uint32_t n_points, int16_t* sasa_points, float* sasa, uint8_t* sasa_mask) {
    chain_radii tab;
    if (!sasa_args_ok(ctx, pos, mask, aatype, layout, L, radius_table, probe, points, n_points, {sasa_points, sasa, sasa_mask}, &tab) || !bound_ok(false, length, n, L))
        return FCZ_E_INVALID_ARG;
    return sasa_host(ctx, pos, mask, aatype, length, false, n, L, layout, tab, probe, points, n_points, sasa_points, sasa, sasa_mask);
}

int fcz_sasa_packed(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint8_t* aatype, const uint32_t* row_off, uint32_t n, uint32_t R, int layout,
                    const float* radius_table, float probe, const float* points, uint32_t n_points, int16_t* sasa_points, float* sasa, uint8_t* sasa_mask) {
    chain_radii tab;
    if (!sasa_args_ok(ctx, pos, mask, aatype, layout, R, radius_table, probe, points, n_points, {sasa_points, sasa, sasa_mask}, &tab) || !bound_ok(true, row_off, n, R))
        return FCZ_E_INVALID_ARG;
    return sasa_host(ctx, pos, mask, aatype, row_off, true, n, R, layout, tab, probe, points, n_points, sasa_points, sasa, sasa_mask);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// steric clashes and peptide-link violations of dense tensors (fcz_violations.h; no counterpart in the reference)
// ------------------------------------------------------------------------------------------------
static bool viol_out_ok(const fcz_violations_out* o) {
    return o && o->clash_atom && o->clash_count && o->clash_depth && o->clash_partner && o->viol_mask && o->link_mask && o->link_length && o->link_cos &&
           o->link_violation && o->chain_counts;
}

// rows: L (padded) or R (packed). Fills tab from radius_table (NULL: the default) when everything is acceptable.
// (the outputs are checked by the caller: fcz_violation_loss_dev shares the rest)
static bool viol_in_ok(const fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint8_t* aatype, int layout, uint32_t rows, const float* radius_table,
                       float tolerance, float link_factor, chain_radii* tab) {
    const int A = fcz_dense_width(layout);
    if (!ctx || !pos || !mask || A <= 0 || rows > SASA_MAX_ROWS) return false;
    if (!std::isfinite(tolerance) || tolerance < 0.0f || !std::isfinite(link_factor) || link_factor < 0.0f) return false;
    if (layout == FCZ_DENSE_ATOM14 && !aatype) return false;                  // a slot's atom depends on the type there
    memset(tab->radius, 0, sizeof tab->radius);
    if (radius_table) memcpy(tab->radius, radius_table, sizeof(float) * CHAIN_TYPES * (size_t)A);
    else if (fcz_sasa_default_radii(layout, tab->radius) != FCZ_OK) return false;
    for (int i = 0; i < (int)CHAIN_TYPES * A; i++) {
        const float r = tab->radius[i];
        if (r == 0.0f) continue;                                              // no atom in this slot
        if (!(r >= 0.5f && r < 8.0f)) return false;                           // (a NaN radius ends here)
    }
    return true;
}

static bool viol_args_ok(const fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint8_t* aatype, int layout, uint32_t rows, const float* radius_table,
                         float tolerance, float link_factor, const fcz_violations_out* out, chain_radii* tab) {
    return viol_out_ok(out) && viol_in_ok(ctx, pos, mask, aatype, layout, rows, radius_table, tolerance, link_factor, tab);
}

// fcz_violations_dev (bound_dev is length [n] or NULL, rows = L) and fcz_violations_packed_dev (bound_dev = row_off [n + 1], rows = R)
static int viol_rows(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint8_t* aatype_dev, const uint32_t* bound_dev, bool packed, uint32_t n,
                     uint32_t rows, int layout, const chain_radii& tab, float tolerance, float link_factor, const fcz_violations_out& o) {
    HIP_TRY(hipSetDevice(ctx->device));
    if (n == 0 && (rows == 0 || !packed)) return FCZ_OK;
    viol_args g{};
    g.pos = pos_dev; g.mask = mask_dev; g.aatype = aatype_dev; g.bound = bound_dev; g.n = n; g.L = rows;
    g.A = (uint32_t)fcz_dense_width(layout);
    g.n_slot = (uint32_t)fcz_dense_slot(layout, 0, fcz_atom_code_from_name("N")); g.ca_slot = (uint32_t)fcz_dense_slot(layout, 0, fcz_atom_code_from_name("CA"));
    g.c_slot = (uint32_t)fcz_dense_slot(layout, 0, fcz_atom_code_from_name("C"));
    g.sg_slot = fcz_dense_slot(layout, (int)VIOL_CYS, fcz_atom_code_from_name("SG"));   // (-1 in backbone4)
    g.tolerance = tolerance; g.link_factor = link_factor;
    g.clash_atom = o.clash_atom; g.clash_count = o.clash_count; g.clash_depth = o.clash_depth; g.clash_partner = o.clash_partner; g.viol_mask = o.viol_mask;
    g.link_mask = o.link_mask; g.link_length = o.link_length; g.link_cos = o.link_cos; g.link_violation = o.link_violation;
    g.chain_counts = reinterpret_cast<unsigned long long*>(o.chain_counts);
    chain_tiles ct(ctx, packed, n, rows, viol_tile_rows(g.A), 12u);
    int rc = ct.reserve(); if (rc) return rc;
    span_guard sg(ctx, "violations");
    if (n) HIP_TRY(hipMemsetAsync(o.chain_counts, 0, sizeof(int64_t) * 4 * (size_t)n, ctx->stream));
    if (rows == 0) return FCZ_OK;                                             // (packed, chains without a row: their counters are 0)
    return ct.run(bound_dev, [&] { hipLaunchKernelGGL(k_chain_fill<viol_args>, ct.fill_grid(rows), dim3(BLOCK), 0, ctx->stream, g); },
                  [&](auto P, dim3 grid, const uint64_t* tile_off, uint32_t tiles_per_entry, uint64_t n_padded) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_violations<decltype(P)::value>), grid, dim3(BLOCK), 0, ctx->stream, g, tab, tile_off, tiles_per_entry, n_padded);
    });
}

// fcz_violations and fcz_violations_packed: the host arrays through DENSE_IN 0 .. 3 and VIOL_OUT 10 .. 19, the outputs in the struct's order
static int viol_host(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint8_t* aatype, const uint32_t* bound, bool packed, uint32_t n, uint32_t rows_per,
                     int layout, const chain_radii& tab, float tolerance, float link_factor, const fcz_violations_out& o) {
    const dense_bytes b(packed, n, rows_per, layout, bound);
    const size_t r = b.rows;
    return staged_call(ctx, {{pos, b.pos, DENSE_IN}, {mask, b.mask, DENSE_IN + 1}, {aatype, r, DENSE_IN + 2}, {bound, b.bound, DENSE_IN + 3}},
                       {{o.clash_atom, b.mask, VIOL_OUT}, {o.clash_count, r * 4, VIOL_OUT + 1}, {o.clash_depth, r * 4, VIOL_OUT + 2}, {o.clash_partner, r * 4, VIOL_OUT + 3},
                        {o.viol_mask, r, VIOL_OUT + 4}, {o.link_mask, r, VIOL_OUT + 5}, {o.link_length, r * 4, VIOL_OUT + 6}, {o.link_cos, r * 8, VIOL_OUT + 7},
                        {o.link_violation, r, VIOL_OUT + 8}, {o.chain_counts, (size_t)n * 4 * sizeof(int64_t), VIOL_OUT + 9}},
                       [&](const void* const* in, void* const* out) {
        const fcz_violations_out d{(uint8_t*)out[0], (int32_t*)out[1], (float*)out[2], (int32_t*)out[3], (uint8_t*)out[4], (uint8_t*)out[5], (float*)out[6],
                                   (float*)out[7], (uint8_t*)out[8], (int64_t*)out[9]};
        return viol_rows(ctx, (const float*)in[0], (const uint8_t*)in[1], (const uint8_t*)in[2], (const uint32_t*)in[3], packed, n, rows_per, layout, tab, tolerance,
                         link_factor, d);
    });
}

extern "C" {

int fcz_violations_pass(void) { return (int)VIOL_PASS; }

int fcz_violations_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint8_t* aatype_dev, const uint32_t* length_dev, uint32_t n, uint32_t L,
                       int layout, const float* radius_table, float tolerance, float link_factor, const fcz_violations_out* out_dev) {
    chain_radii tab;
    if (!viol_args_ok(ctx, pos_dev, mask_dev, aatype_dev, layout, L, radius_table, tolerance, link_factor, out_dev, &tab) || !bound_ok(false, length_dev, n, L))
        return FCZ_E_INVALID_ARG;
    return viol_rows(ctx, pos_dev, mask_dev, aatype_dev, length_dev, false, n, L, layout, tab, tolerance, link_factor, *out_dev);
}

int fcz_violations_packed_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint8_t* aatype_dev, const uint32_t* row_off_dev, uint32_t n,
                              uint32_t R, int layout, const float* radius_table, float tolerance, float link_factor, const fcz_violations_out* out_dev) {
    chain_radii tab;
    if (!viol_args_ok(ctx, pos_dev, mask_dev, aatype_dev, layout, R, radius_table, tolerance, link_factor, out_dev, &tab) || !bound_ok(true, row_off_dev, n, R))
        return FCZ_E_INVALID_ARG;
    return viol_rows(ctx, pos_dev, mask_dev, aatype_dev, row_off_dev, true, n, R, layout, tab, tolerance, link_factor, *out_dev);
}

int fcz_violations(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint8_t* aatype, const uint32_t* length, uint32_t n, uint32_t L, int layout,
                   const float* radius_table, float tolerance, float link_factor, const fcz_violations_out* out) {
    chain_radii tab;
    if (!viol_args_ok(ctx, pos, mask, aatype, layout, L, radius_table, tolerance, link_factor, out, &tab) || !bound_ok(false, length, n, L)) return FCZ_E_INVALID_ARG;
    return viol_host(ctx, pos, mask, aatype, length, false, n, L, layout, tab, tolerance, link_factor, *out);
}

int fcz_violations_packed(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint8_t* aatype, const uint32_t* row_off, uint32_t n, uint32_t R, int layout,
                          const float* radius_table, float tolerance, float link_factor, const fcz_violations_out* out) {
    chain_radii tab;
    if (!viol_args_ok(ctx, pos, mask, aatype, layout, R, radius_table, tolerance, link_factor, out, &tab) || !bound_ok(true, row_off, n, R)) return FCZ_E_INVALID_ARG;
    return viol_host(ctx, pos, mask, aatype, row_off, true, n, R, layout, tab, tolerance, link_factor, *out);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// the violation loss and its gradient (fcz_violation_loss.h; no counterpart in the reference)
// ------------------------------------------------------------------------------------------------
// the device forms of the value (w_clash_dev, w_link_dev and grad_dev NULL) and of the gradient (the three outputs of the value NULL);
// bound_dev is length [n] or NULL with rows = L, or row_off [n + 1] with rows = R
static int vloss_rows(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint8_t* aatype_dev, const uint32_t* bound_dev, bool packed, uint32_t n,
                      uint32_t rows, int layout, const chain_radii& tab, float tolerance, float link_factor, float* clash_loss_dev, float* link_loss_dev,
                      int64_t* counts_dev, const float* w_clash_dev, const float* w_link_dev, float* grad_dev) {
    HIP_TRY(hipSetDevice(ctx->device));
    if (n == 0 && (rows == 0 || !packed)) return FCZ_OK;
    const uint32_t A = (uint32_t)fcz_dense_width(layout);
    const uint32_t n_slot = (uint32_t)fcz_dense_slot(layout, 0, fcz_atom_code_from_name("N")), ca_slot = (uint32_t)fcz_dense_slot(layout, 0, fcz_atom_code_from_name("CA"));
    const uint32_t c_slot = (uint32_t)fcz_dense_slot(layout, 0, fcz_atom_code_from_name("C"));
    const int32_t sg_slot = fcz_dense_slot(layout, (int)VIOL_CYS, fcz_atom_code_from_name("SG"));   // (-1 in backbone4)
    chain_tiles ct(ctx, packed, n, rows, viol_tile_rows(A), 12u);
    int rc = ct.reserve(); if (rc) return rc;
    if (grad_dev) {
        if (rows == 0) return FCZ_OK;
        const vloss_grad_args g{pos_dev, mask_dev, aatype_dev, bound_dev, n, rows, A, n_slot, ca_slot, c_slot, sg_slot, tolerance, link_factor, w_clash_dev, w_link_dev,
                                grad_dev};
        span_guard sg(ctx, "violation_loss_grad");
        return ct.run(bound_dev, [&] { hipLaunchKernelGGL(k_chain_fill<vloss_grad_args>, ct.fill_grid(rows), dim3(BLOCK), 0, ctx->stream, g); },
                      [&](auto P, dim3 grid, const uint64_t* tile_off, uint32_t tiles_per_entry, uint64_t n_padded) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_violation_loss_grad<decltype(P)::value>), grid, dim3(BLOCK), 0, ctx->stream, g, tab, tile_off, tiles_per_entry, n_padded);
        });
    }
    const vloss_args g{pos_dev, mask_dev, aatype_dev, bound_dev, n, rows, A, n_slot, ca_slot, c_slot, sg_slot, tolerance, link_factor, clash_loss_dev, link_loss_dev,
                       reinterpret_cast<unsigned long long*>(counts_dev)};
    span_guard sg(ctx, "violation_loss");
    if (n) HIP_TRY(hipMemsetAsync(counts_dev, 0, sizeof(int64_t) * 2 * (size_t)n, ctx->stream));
    if (rows == 0) return FCZ_OK;                                             // (packed, chains without a row: their counters are 0)
    return ct.run(bound_dev, [&] { hipLaunchKernelGGL(k_chain_fill<vloss_args>, ct.fill_grid(rows), dim3(BLOCK), 0, ctx->stream, g); },
                  [&](auto P, dim3 grid, const uint64_t* tile_off, uint32_t tiles_per_entry, uint64_t n_padded) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_violation_loss<decltype(P)::value>), grid, dim3(BLOCK), 0, ctx->stream, g, tab, tile_off, tiles_per_entry, n_padded);
    });
}

// the host forms: the host arrays through DENSE_IN 0 .. 3, VLOSS_WEIGHT 4 .. 5 and VLOSS_OUT 10 .. 12 (clash_loss, link_loss, counts) or 10 (grad)
static int vloss_host(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint8_t* aatype, const uint32_t* bound, bool packed, uint32_t n, uint32_t rows_per,
                      int layout, const chain_radii& tab, float tolerance, float link_factor, float* clash_loss, float* link_loss, int64_t* counts,
                      const float* w_clash, const float* w_link, float* grad) {
    const dense_bytes b(packed, n, rows_per, layout, bound);
    const size_t r = b.rows;
    auto run = [&](const void* const* in, void* const* out) {
        return vloss_rows(ctx, (const float*)in[0], (const uint8_t*)in[1], (const uint8_t*)in[2], (const uint32_t*)in[3], packed, n, rows_per, layout, tab, tolerance,
                          link_factor, grad ? nullptr : (float*)out[0], grad ? nullptr : (float*)out[1], grad ? nullptr : (int64_t*)out[2], (const float*)in[4],
                          (const float*)in[5], grad ? (float*)out[0] : nullptr);
    };
    if (grad)
        return staged_call(ctx, {{pos, b.pos, DENSE_IN}, {mask, b.mask, DENSE_IN + 1}, {aatype, r, DENSE_IN + 2}, {bound, b.bound, DENSE_IN + 3},
                                 {w_clash, b.mask * 4, VLOSS_WEIGHT}, {w_link, r * 12, VLOSS_WEIGHT + 1}}, {{grad, b.pos, VLOSS_OUT}}, run);
    return staged_call(ctx, {{pos, b.pos, DENSE_IN}, {mask, b.mask, DENSE_IN + 1}, {aatype, r, DENSE_IN + 2}, {bound, b.bound, DENSE_IN + 3},
                             {nullptr, 0, VLOSS_WEIGHT}, {nullptr, 0, VLOSS_WEIGHT + 1}},
                       {{clash_loss, b.mask * 4, VLOSS_OUT}, {link_loss, r * 12, VLOSS_OUT + 1}, {counts, (size_t)n * 2 * sizeof(int64_t), VLOSS_OUT + 2}}, run);
}

extern "C" {

int fcz_violation_loss_pass(void) { return (int)VLOSS_PASS; }

int fcz_violation_loss_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint8_t* aatype_dev, const uint32_t* length_dev, uint32_t n, uint32_t L,
                           int layout, const float* radius_table, float tolerance, float link_factor, float* clash_loss_dev, float* link_loss_dev,
                           int64_t* counts_dev) {
    chain_radii tab;
    if (!clash_loss_dev || !link_loss_dev || !counts_dev || !viol_in_ok(ctx, pos_dev, mask_dev, aatype_dev, layout, L, radius_table, tolerance, link_factor, &tab) ||
        !bound_ok(false, length_dev, n, L))
        return FCZ_E_INVALID_ARG;
    return vloss_rows(ctx, pos_dev, mask_dev, aatype_dev, length_dev, false, n, L, layout, tab, tolerance, link_factor, clash_loss_dev, link_loss_dev, counts_dev,
                      nullptr, nullptr, nullptr);
}

int fcz_violation_loss_packed_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint8_t* aatype_dev, const uint32_t* row_off_dev, uint32_t n,
                                  uint32_t R, int layout, const float* radius_table, float tolerance, float link_factor, float* clash_loss_dev,
                                  float* link_loss_dev, int64_t* counts_dev) {
    chain_radii tab;
    if (!clash_loss_dev || !link_loss_dev || !counts_dev || !viol_in_ok(ctx, pos_dev, mask_dev, aatype_dev, layout, R, radius_table, tolerance, link_factor, &tab) ||
        !bound_ok(true, row_off_dev, n, R))
        return FCZ_E_INVALID_ARG;
    return vloss_rows(ctx, pos_dev, mask_dev, aatype_dev, row_off_dev, true, n, R, layout, tab, tolerance, link_factor, clash_loss_dev, link_loss_dev, counts_dev,
                      nullptr, nullptr, nullptr);
}

int fcz_violation_loss_grad_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint8_t* aatype_dev, const uint32_t* length_dev, uint32_t n,
                                uint32_t L, int layout, const float* radius_table, float tolerance, float link_factor, const float* w_clash_dev,
                                const float* w_link_dev, float* grad_dev) {
    chain_radii tab;
    if (!w_clash_dev || !w_link_dev || !grad_dev || !viol_in_ok(ctx, pos_dev, mask_dev, aatype_dev, layout, L, radius_table, tolerance, link_factor, &tab) ||
        !bound_ok(false, length_dev, n, L))
        return FCZ_E_INVALID_ARG;
    return vloss_rows(ctx, pos_dev, mask_dev, aatype_dev, length_dev, false, n, L, layout, tab, tolerance, link_factor, nullptr, nullptr, nullptr, w_clash_dev,
                      w_link_dev, grad_dev);
}

int fcz_violation_loss_grad_packed_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint8_t* aatype_dev, const uint32_t* row_off_dev,
                                       uint32_t n, uint32_t R, int layout, const float* radius_table, float tolerance, float link_factor,
                                       const float* w_clash_dev, const float* w_link_dev, float* grad_dev) {
    chain_radii tab;
    if (!w_clash_dev || !w_link_dev || !grad_dev || !viol_in_ok(ctx, pos_dev, mask_dev, aatype_dev, layout, R, radius_table, tolerance, link_factor, &tab) ||
        !bound_ok(true, row_off_dev, n, R))
        return FCZ_E_INVALID_ARG;
    return vloss_rows(ctx, pos_dev, mask_dev, aatype_dev, row_off_dev, true, n, R, layout, tab, tolerance, link_factor, nullptr, nullptr, nullptr, w_clash_dev,
                      w_link_dev, grad_dev);
}

int fcz_violation_loss(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint8_t* aatype, const uint32_t* length, uint32_t n, uint32_t L, int layout,
                       const float* radius_table, float tolerance, float link_factor, float* clash_loss, float* link_loss, int64_t* counts) {
    chain_radii tab;
    if (!clash_loss || !link_loss || !counts || !viol_in_ok(ctx, pos, mask, aatype, layout, L, radius_table, tolerance, link_factor, &tab) ||
        !bound_ok(false, length, n, L))
        return FCZ_E_INVALID_ARG;
    return vloss_host(ctx, pos, mask, aatype, length, false, n, L, layout, tab, tolerance, link_factor, clash_loss, link_loss, counts, nullptr, nullptr, nullptr);
}

int fcz_violation_loss_packed(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint8_t* aatype, const uint32_t* row_off, uint32_t n, uint32_t R,
                              int layout, const float* radius_table, float tolerance, float link_factor, float* clash_loss, float* link_loss, int64_t* counts) {
    chain_radii tab;
    if (!clash_loss || !link_loss || !counts || !viol_in_ok(ctx, pos, mask, aatype, layout, R, radius_table, tolerance, link_factor, &tab) ||
        !bound_ok(true, row_off, n, R))
        return FCZ_E_INVALID_ARG;
    return vloss_host(ctx, pos, mask, aatype, row_off, true, n, R, layout, tab, tolerance, link_factor, clash_loss, link_loss, counts, nullptr, nullptr, nullptr);
}

int fcz_violation_loss_grad(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint8_t* aatype, const uint32_t* length, uint32_t n, uint32_t L, int layout,
                            const float* radius_table, float tolerance, float link_factor, const float* w_clash, const float* w_link, float* grad) {
    chain_radii tab;
    if (!w_clash || !w_link || !grad || !viol_in_ok(ctx, pos, mask, aatype, layout, L, radius_table, tolerance, link_factor, &tab) || !bound_ok(false, length, n, L))
        return FCZ_E_INVALID_ARG;
    return vloss_host(ctx, pos, mask, aatype, length, false, n, L, layout, tab, tolerance, link_factor, nullptr, nullptr, nullptr, w_clash, w_link, grad);
}

int fcz_violation_loss_grad_packed(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint8_t* aatype, const uint32_t* row_off, uint32_t n, uint32_t R,
                                   int layout, const float* radius_table, float tolerance, float link_factor, const float* w_clash, const float* w_link,
                                   float* grad) {
    chain_radii tab;
    if (!w_clash || !w_link || !grad || !viol_in_ok(ctx, pos, mask, aatype, layout, R, radius_table, tolerance, link_factor, &tab) || !bound_ok(true, row_off, n, R))
        return FCZ_E_INVALID_ARG;
    return vloss_host(ctx, pos, mask, aatype, row_off, true, n, R, layout, tab, tolerance, link_factor, nullptr, nullptr, nullptr, w_clash, w_link, grad);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// least-squares superposition of two dense tensor batches (fcz_superpose.h; no counterpart in the reference)
// ------------------------------------------------------------------------------------------------
// rows: L (padded) or R (packed)
static bool superpose_args_ok(const fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, int layout, int slot, uint32_t rows,
                              const fcz_superpose_out* out) {
    if (!ctx || !pos_true || !mask_true || !pos_pred || !out || !out->rot || !out->trans) return false;
    if (fcz_dense_width(layout) <= 0 || slot < 0 || slot >= fcz_dense_width(layout)) return false;
    return rows <= SUPERPOSE_MAX_ROWS;
}

// fcz_superpose_dev (bound_dev is length [n] or NULL, rows = L) and fcz_superpose_packed_dev (bound_dev = row_off [n + 1], rows = R)
static int superpose_rows(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev, const uint8_t* mask_pred_dev,
                          const uint32_t* bound_dev, bool packed, uint32_t n, uint32_t rows, int layout, int slot, const fcz_superpose_out& o) {
    HIP_TRY(hipSetDevice(ctx->device));
    const bool fill = packed && rows && o.dev;
    if (n == 0 && !fill) return FCZ_OK;
    const superpose_args g{pos_true_dev, mask_true_dev, pos_pred_dev, mask_pred_dev, bound_dev, n, rows, (uint32_t)fcz_dense_width(layout), (uint32_t)slot,
                           o.rot, o.trans, o.rmsd, o.sites, o.gdt_counts, o.tm, o.dev};
    const uint32_t max_blocks = (uint32_t)ctx->n_cu * 16u;
    span_guard sg(ctx, "superpose");
    if (fill)
        hipLaunchKernelGGL(k_chain_fill<superpose_args>, dim3((uint32_t)std::min<uint64_t>(((uint64_t)rows + BLOCK - 1) / BLOCK, max_blocks)), dim3(BLOCK), 0, ctx->stream, g);
    if (n) {
        const dim3 grid(std::min(grid_for(n, WAVES_PER_BLOCK), max_blocks));
        if (packed) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_superpose<true>), grid, dim3(BLOCK), 0, ctx->stream, g);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_superpose<false>), grid, dim3(BLOCK), 0, ctx->stream, g);
    }
    HIP_TRY(hipGetLastError());
    return FCZ_OK;
}

// fcz_superpose and fcz_superpose_packed: the host arrays through DENSE_IN 0, 1, 3, LDDT_PRED 4, 5 and SUPERPOSE_OUT 10 .. 16, the outputs in the struct's order
static int superpose_host(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, const uint8_t* mask_pred, const uint32_t* bound,
                          bool packed, uint32_t n, uint32_t rows_per, int layout, int slot, const fcz_superpose_out& o) {
    const dense_bytes b(packed, n, rows_per, layout, bound);
    const size_t c = n;
    return staged_call(ctx, {{pos_true, b.pos, DENSE_IN}, {mask_true, b.mask, DENSE_IN + 1}, {bound, b.bound, DENSE_IN + 3}, {pos_pred, b.pos, LDDT_PRED},
                             {mask_pred, b.mask, LDDT_PRED + 1}},
                       {{o.rot, 36 * c, SUPERPOSE_OUT}, {o.trans, 12 * c, SUPERPOSE_OUT + 1}, {o.rmsd, 4 * c, SUPERPOSE_OUT + 2}, {o.sites, 4 * c, SUPERPOSE_OUT + 3},
                        {o.gdt_counts, 20 * c, SUPERPOSE_OUT + 4}, {o.tm, 4 * c, SUPERPOSE_OUT + 5}, {o.dev, 4 * b.rows, SUPERPOSE_OUT + 6}},
                       [&](const void* const* in, void* const* out) {
        const fcz_superpose_out d{(float*)out[0], (float*)out[1], (float*)out[2], (int32_t*)out[3], (int32_t*)out[4], (float*)out[5], (float*)out[6]};
        return superpose_rows(ctx, (const float*)in[0], (const uint8_t*)in[1], (const float*)in[3], (const uint8_t*)in[4], (const uint32_t*)in[2], packed, n, rows_per,
                              layout, slot, d);
    });
}

static bool superpose_apply_args_ok(const fcz_ctx* ctx, const float* pos, int layout, uint32_t rows, const float* rot, const float* trans, const float* pos_out) {
    return ctx && pos && rot && trans && pos_out && fcz_dense_width(layout) > 0 && rows <= SUPERPOSE_MAX_ROWS;
}

// fcz_superpose_apply_dev (rows = L) and fcz_superpose_apply_packed_dev (rows = R)
static int superpose_apply_rows(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint32_t* bound_dev, bool packed, uint32_t n, uint32_t rows,
                                int layout, const float* rot_dev, const float* trans_dev, float* pos_out_dev) {
    HIP_TRY(hipSetDevice(ctx->device));
    if (rows == 0 || (n == 0 && !packed)) return FCZ_OK;
    const superpose_apply_args g{pos_dev, mask_dev, bound_dev, n, rows, (uint32_t)fcz_dense_width(layout), rot_dev, trans_dev, pos_out_dev};
    chain_tiles ct(ctx, packed, n, rows);
    int rc = ct.reserve(); if (rc) return rc;
    span_guard sg(ctx, "superpose");
    dispatch_layout(layout, [&](auto W) {
        constexpr int A = decltype(W)::value;
        rc = ct.run(bound_dev, [&] { hipLaunchKernelGGL(k_chain_fill<superpose_apply_args>, ct.fill_grid(rows), dim3(BLOCK), 0, ctx->stream, g); },
                    [&](auto P, dim3 grid, const uint64_t* tile_off, uint32_t tiles_per_entry, uint64_t n_padded) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_superpose_apply<A, decltype(P)::value>), grid, dim3(BLOCK), 0, ctx->stream, g, tile_off, tiles_per_entry, n_padded);
        });
    });
    return rc;
}

// fcz_superpose_apply and fcz_superpose_apply_packed: the host arrays through LDDT_PRED 4, 5, DENSE_IN 3 and APPLY_ROT, APPLY_TRANS, APPLY_OUT.
// (Without a chain rot and trans have no byte and are NULL on the device: the fill, the only launch then, reads neither.)
static int superpose_apply_host(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint32_t* bound, bool packed, uint32_t n, uint32_t rows_per,
                                int layout, const float* rot, const float* trans, float* pos_out) {
    const dense_bytes b(packed, n, rows_per, layout, bound);
    return staged_call(ctx, {{pos, b.pos, LDDT_PRED}, {mask, b.mask, LDDT_PRED + 1}, {bound, b.bound, DENSE_IN + 3}, {rot, 36 * (size_t)n, APPLY_ROT},
                             {trans, 12 * (size_t)n, APPLY_TRANS}},
                       {{pos_out, b.pos, APPLY_OUT}}, [&](const void* const* in, void* const* out) {
        return superpose_apply_rows(ctx, (const float*)in[0], (const uint8_t*)in[1], (const uint32_t*)in[2], packed, n, rows_per, layout, (const float*)in[3],
                                    (const float*)in[4], (float*)out[0]);
    });
}

extern "C" {

int fcz_superpose_dev(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev, const uint8_t* mask_pred_dev,
                      const uint32_t* length_dev, uint32_t n, uint32_t L, int layout, int slot, const fcz_superpose_out* out_dev) {
    if (!superpose_args_ok(ctx, pos_true_dev, mask_true_dev, pos_pred_dev, layout, slot, L, out_dev) || !bound_ok(false, length_dev, n, L)) return FCZ_E_INVALID_ARG;
    return superpose_rows(ctx, pos_true_dev, mask_true_dev, pos_pred_dev, mask_pred_dev, length_dev, false, n, L, layout, slot, *out_dev);
}

int fcz_superpose_packed_dev(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev, const uint8_t* mask_pred_dev,
                             const uint32_t* row_off_dev, uint32_t n, uint32_t R, int layout, int slot, const fcz_superpose_out* out_dev) {
    if (!superpose_args_ok(ctx, pos_true_dev, mask_true_dev, pos_pred_dev, layout, slot, R, out_dev) || !bound_ok(true, row_off_dev, n, R)) return FCZ_E_INVALID_ARG;
    return superpose_rows(ctx, pos_true_dev, mask_true_dev, pos_pred_dev, mask_pred_dev, row_off_dev, true, n, R, layout, slot, *out_dev);
}

int fcz_superpose(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, const uint8_t* mask_pred, const uint32_t* length,
                  uint32_t n, uint32_t L, int layout, int slot, const fcz_superpose_out* out) {
    if (!superpose_args_ok(ctx, pos_true, mask_true, pos_pred, layout, slot, L, out) || !bound_ok(false, length, n, L)) return FCZ_E_INVALID_ARG;
    return superpose_host(ctx, pos_true, mask_true, pos_pred, mask_pred, length, false, n, L, layout, slot, *out);
}

int fcz_superpose_packed(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, const uint8_t* mask_pred, const uint32_t* row_off,
                         uint32_t n, uint32_t R, int layout, int slot, const fcz_superpose_out* out) {
    if (!superpose_args_ok(ctx, pos_true, mask_true, pos_pred, layout, slot, R, out) || !bound_ok(true, row_off, n, R)) return FCZ_E_INVALID_ARG;
    return superpose_host(ctx, pos_true, mask_true, pos_pred, mask_pred, row_off, true, n, R, layout, slot, *out);
}

int fcz_superpose_apply_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint32_t* length_dev, uint32_t n, uint32_t L, int layout,
                            const float* rot_dev, const float* trans_dev, float* pos_out_dev) {
    if (!superpose_apply_args_ok(ctx, pos_dev, layout, L, rot_dev, trans_dev, pos_out_dev) || !bound_ok(false, length_dev, n, L)) return FCZ_E_INVALID_ARG;
    return superpose_apply_rows(ctx, pos_dev, mask_dev, length_dev, false, n, L, layout, rot_dev, trans_dev, pos_out_dev);
}

int fcz_superpose_apply_packed_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint32_t* row_off_dev, uint32_t n, uint32_t R, int layout,
                                   const float* rot_dev, const float* trans_dev, float* pos_out_dev) {
    if (!superpose_apply_args_ok(ctx, pos_dev, layout, R, rot_dev, trans_dev, pos_out_dev) || !bound_ok(true, row_off_dev, n, R)) return FCZ_E_INVALID_ARG;
    return superpose_apply_rows(ctx, pos_dev, mask_dev, row_off_dev, true, n, R, layout, rot_dev, trans_dev, pos_out_dev);
}

int fcz_superpose_apply(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint32_t* length, uint32_t n, uint32_t L, int layout, const float* rot,
                        const float* trans, float* pos_out) {
    if (!superpose_apply_args_ok(ctx, pos, layout, L, rot, trans, pos_out) || !bound_ok(false, length, n, L)) return FCZ_E_INVALID_ARG;
    return superpose_apply_host(ctx, pos, mask, length, false, n, L, layout, rot, trans, pos_out);
}

int fcz_superpose_apply_packed(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint32_t* row_off, uint32_t n, uint32_t R, int layout, const float* rot,
                               const float* trans, float* pos_out) {
    if (!superpose_apply_args_ok(ctx, pos, layout, R, rot, trans, pos_out) || !bound_ok(true, row_off, n, R)) return FCZ_E_INVALID_ARG;
    return superpose_apply_host(ctx, pos, mask, row_off, true, n, R, layout, rot, trans, pos_out);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// maximised TM-score by seeded iterative superposition (fcz_tmscore.h; no counterpart in the reference)
// ------------------------------------------------------------------------------------------------
static bool tmscore_args_ok(const fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, int layout, int slot, uint32_t rows,
                            uint32_t iterations, const fcz_tmscore_out* out) {
    if (!ctx || !pos_true || !mask_true || !pos_pred || !out || !out->rot || !out->trans) return false;
    if (fcz_dense_width(layout) <= 0 || slot < 0 || slot >= fcz_dense_width(layout)) return false;
    return rows <= SUPERPOSE_MAX_ROWS && iterations <= TM_MAX_ITERATIONS;
}

// fcz_tmscore_dev (bound_dev is length [n] or NULL, rows = L) and fcz_tmscore_packed_dev (bound_dev = row_off [n + 1], rows = R)
static int tmscore_rows(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev, const uint8_t* mask_pred_dev,
                        const uint32_t* bound_dev, bool packed, uint32_t n, uint32_t rows, int layout, int slot, uint32_t levels, uint32_t iterations,
                        const fcz_tmscore_out& o) {
    HIP_TRY(hipSetDevice(ctx->device));
    const bool fill = packed && rows && o.dev;
    if (n == 0 && !fill) return FCZ_OK;
    tmscore_args g{{pos_true_dev, mask_true_dev, pos_pred_dev, mask_pred_dev, bound_dev, n, rows, (uint32_t)fcz_dense_width(layout), (uint32_t)slot,
                    o.rot, o.trans, o.rmsd, o.sites, o.gdt_counts, o.tm, o.dev},
                   o.seed, o.selected, levels, iterations, nullptr, nullptr, nullptr, 0};
    const uint32_t max_blocks = (uint32_t)ctx->n_cu * 16u;
    // the seeds are counted on the device: at most this many items of WAVES_PER_BLOCK seeds, a double per seed
    const uint64_t items = tm_items_bound(packed ? (uint64_t)rows : (uint64_t)n * rows, n);
    uint64_t* counts = nullptr;
    if (n) {
        int rc = ctx->tm_scratch.ensure(sizeof(uint64_t) * (2 * (size_t)n + 1) + sizeof(double) * WAVES_PER_BLOCK * (size_t)items + sizeof(uint32_t) * (size_t)n);
        if (rc) return rc;
        counts = ctx->tm_scratch.as<uint64_t>();
        g.item_off = counts + n;
        g.score = reinterpret_cast<double*>(g.item_off + n + 1); g.score_cap = WAVES_PER_BLOCK * items;
        g.nsites = reinterpret_cast<uint32_t*>(g.score + g.score_cap);
    }
    span_guard sg(ctx, "tmscore");
    if (fill)
        hipLaunchKernelGGL(k_chain_fill<superpose_args>, dim3((uint32_t)std::min<uint64_t>(((uint64_t)rows + BLOCK - 1) / BLOCK, max_blocks)), dim3(BLOCK), 0, ctx->stream, g.s);
    if (n) {
        const dim3 chains(std::min(grid_for(n, WAVES_PER_BLOCK), max_blocks)), search((uint32_t)std::min<uint64_t>(items, max_blocks));
        if (packed) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tm_count<true>), chains, dim3(BLOCK), 0, ctx->stream, g, counts);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tm_count<false>), chains, dim3(BLOCK), 0, ctx->stream, g, counts);
        int rc = device_scan<uint64_t>(ctx, counts, g.item_off, n); if (rc) return rc;
        if (packed) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tm_search<true>), search, dim3(BLOCK), 0, ctx->stream, g);
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tm_final<true>), chains, dim3(BLOCK), 0, ctx->stream, g);
        } else {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tm_search<false>), search, dim3(BLOCK), 0, ctx->stream, g);
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tm_final<false>), chains, dim3(BLOCK), 0, ctx->stream, g);
        }
    }
    HIP_TRY(hipGetLastError());
    return FCZ_OK;
}

// fcz_tmscore and fcz_tmscore_packed: the host arrays as fcz_superpose's, then TM_SEED, TM_SELECTED, the outputs in the struct's order
static int tmscore_host(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, const uint8_t* mask_pred, const uint32_t* bound,
                        bool packed, uint32_t n, uint32_t rows_per, int layout, int slot, uint32_t levels, uint32_t iterations, const fcz_tmscore_out& o) {
    const dense_bytes b(packed, n, rows_per, layout, bound);
    const size_t c = n;
    return staged_call(ctx, {{pos_true, b.pos, DENSE_IN}, {mask_true, b.mask, DENSE_IN + 1}, {bound, b.bound, DENSE_IN + 3}, {pos_pred, b.pos, LDDT_PRED},
                             {mask_pred, b.mask, LDDT_PRED + 1}},
                       {{o.rot, 36 * c, SUPERPOSE_OUT}, {o.trans, 12 * c, SUPERPOSE_OUT + 1}, {o.rmsd, 4 * c, SUPERPOSE_OUT + 2}, {o.sites, 4 * c, SUPERPOSE_OUT + 3},
                        {o.gdt_counts, 20 * c, SUPERPOSE_OUT + 4}, {o.tm, 4 * c, SUPERPOSE_OUT + 5}, {o.dev, 4 * b.rows, SUPERPOSE_OUT + 6}, {o.seed, 4 * c, TM_SEED},
                        {o.selected, 4 * c, TM_SELECTED}},
                       [&](const void* const* in, void* const* out) {
        const fcz_tmscore_out d{(float*)out[0], (float*)out[1], (float*)out[2], (int32_t*)out[3], (int32_t*)out[4], (float*)out[5], (float*)out[6], (int32_t*)out[7],
                                (int32_t*)out[8]};
        return tmscore_rows(ctx, (const float*)in[0], (const uint8_t*)in[1], (const float*)in[3], (const uint8_t*)in[4], (const uint32_t*)in[2], packed, n, rows_per,
                            layout, slot, levels, iterations, d);
    });
}

extern "C" {

uint64_t fcz_tmscore_seeds(uint32_t sites, uint32_t levels) { return tm_seed_count(sites, levels); }

int fcz_tmscore_seed_fragment(uint32_t sites, uint32_t levels, uint64_t seed, uint32_t* start, uint32_t* length) {
    if (!start || !length || seed >= tm_seed_count(sites, levels)) return FCZ_E_INVALID_ARG;
    tm_seed_fragment(sites, seed, start, length);
    return FCZ_OK;
}

int fcz_tmscore_dev(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev, const uint8_t* mask_pred_dev,
                    const uint32_t* length_dev, uint32_t n, uint32_t L, int layout, int slot, uint32_t levels, uint32_t iterations, const fcz_tmscore_out* out_dev) {
    if (!tmscore_args_ok(ctx, pos_true_dev, mask_true_dev, pos_pred_dev, layout, slot, L, iterations, out_dev) || !bound_ok(false, length_dev, n, L))
        return FCZ_E_INVALID_ARG;
    return tmscore_rows(ctx, pos_true_dev, mask_true_dev, pos_pred_dev, mask_pred_dev, length_dev, false, n, L, layout, slot, levels, iterations, *out_dev);
}

int fcz_tmscore_packed_dev(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev, const uint8_t* mask_pred_dev,
                           const uint32_t* row_off_dev, uint32_t n, uint32_t R, int layout, int slot, uint32_t levels, uint32_t iterations,
                           const fcz_tmscore_out* out_dev) {
    if (!tmscore_args_ok(ctx, pos_true_dev, mask_true_dev, pos_pred_dev, layout, slot, R, iterations, out_dev) || !bound_ok(true, row_off_dev, n, R))
        return FCZ_E_INVALID_ARG;
    return tmscore_rows(ctx, pos_true_dev, mask_true_dev, pos_pred_dev, mask_pred_dev, row_off_dev, true, n, R, layout, slot, levels, iterations, *out_dev);
}

int fcz_tmscore(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, const uint8_t* mask_pred, const uint32_t* length,
                uint32_t n, uint32_t L, int layout, int slot, uint32_t levels, uint32_t iterations, const fcz_tmscore_out* out) {
    if (!tmscore_args_ok(ctx, pos_true, mask_true, pos_pred, layout, slot, L, iterations, out) || !bound_ok(false, length, n, L)) return FCZ_E_INVALID_ARG;
    return tmscore_host(ctx, pos_true, mask_true, pos_pred, mask_pred, length, false, n, L, layout, slot, levels, iterations, *out);
}

int fcz_tmscore_packed(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, const uint8_t* mask_pred, const uint32_t* row_off,
                       uint32_t n, uint32_t R, int layout, int slot, uint32_t levels, uint32_t iterations, const fcz_tmscore_out* out) {
    if (!tmscore_args_ok(ctx, pos_true, mask_true, pos_pred, layout, slot, R, iterations, out) || !bound_ok(true, row_off, n, R)) return FCZ_E_INVALID_ARG;
    return tmscore_host(ctx, pos_true, mask_true, pos_pred, mask_pred, row_off, true, n, R, layout, slot, levels, iterations, *out);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// maximised GDT counts by seeded superposition search (fcz_gdt.h; no counterpart in the reference)
// ------------------------------------------------------------------------------------------------
static bool gdt_args_ok(const fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, int layout, int slot, uint32_t rows,
                        uint32_t iterations, uint32_t runs, const fcz_gdt_out* out) {
    if (!ctx || !pos_true || !mask_true || !pos_pred || !out || !out->gdt_counts) return false;
    if (fcz_dense_width(layout) <= 0 || slot < 0 || slot >= fcz_dense_width(layout)) return false;
    return rows <= SUPERPOSE_MAX_ROWS && iterations <= TM_MAX_ITERATIONS && runs != 0 && runs < (1u << GDT_RUNS);
}

// fcz_gdt_dev (bound_dev is length [n] or NULL, rows = L) and fcz_gdt_packed_dev (bound_dev = row_off [n + 1], rows = R)
static int gdt_rows(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev, const uint8_t* mask_pred_dev,
                    const uint32_t* bound_dev, bool packed, uint32_t n, uint32_t rows, int layout, int slot, uint32_t levels, uint32_t iterations, uint32_t runs,
                    const fcz_gdt_out& o) {
    HIP_TRY(hipSetDevice(ctx->device));
    const bool fill = packed && rows && o.within;
    if (n == 0 && !fill) return FCZ_OK;
    const uint32_t max_blocks = (uint32_t)ctx->n_cu * 16u;
    span_guard sg(ctx, "gdt");
    if (fill) {
        const gdt_fill_args f{bound_dev, n, rows, o.within};
        hipLaunchKernelGGL(k_chain_fill<gdt_fill_args>, dim3((uint32_t)std::min<uint64_t>(((uint64_t)rows + BLOCK - 1) / BLOCK, max_blocks)), dim3(BLOCK), 0, ctx->stream, f);
    }
    if (n) {
        // k_tm_count as fcz_tmscore_dev launches it: S and the work items of every chain, counted on the device and scanned
        int rc = ctx->gdt_scratch.ensure(sizeof(uint64_t) * (2 * (size_t)n + 1 + GDT_CUTOFFS * (size_t)n) + sizeof(uint32_t) * (size_t)n);
        if (rc) return rc;
        uint64_t* counts = ctx->gdt_scratch.as<uint64_t>();
        uint64_t* item_off = counts + n;
        unsigned long long* best = reinterpret_cast<unsigned long long*>(item_off + n + 1);
        uint32_t* nsites = reinterpret_cast<uint32_t*>(best + GDT_CUTOFFS * (size_t)n);
        const superpose_args in{pos_true_dev, mask_true_dev, pos_pred_dev, mask_pred_dev, bound_dev, n, rows, (uint32_t)fcz_dense_width(layout), (uint32_t)slot,
                                nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        const tmscore_args tc{in, nullptr, nullptr, levels, iterations, nsites, item_off, nullptr, 0};
        const gdt_args g{in, o.gdt_counts, o.sites, o.rot, o.trans, o.seed, o.run, o.selected, o.within, levels, iterations, runs, nsites, item_off, best};
        const uint64_t items = tm_items_bound(packed ? (uint64_t)rows : (uint64_t)n * rows, n);
        const dim3 chains(std::min(grid_for(n, WAVES_PER_BLOCK), max_blocks)), search((uint32_t)std::min<uint64_t>(items, max_blocks)), final_grid(std::min(n, max_blocks));
        HIP_TRY(hipMemsetAsync(best, 0, sizeof(unsigned long long) * GDT_CUTOFFS * (size_t)n, ctx->stream));
        if (packed) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tm_count<true>), chains, dim3(BLOCK), 0, ctx->stream, tc, counts);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tm_count<false>), chains, dim3(BLOCK), 0, ctx->stream, tc, counts);
        rc = device_scan<uint64_t>(ctx, counts, item_off, n); if (rc) return rc;
        if (packed) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gdt_search<true>), search, dim3(BLOCK), 0, ctx->stream, g);
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gdt_final<true>), final_grid, dim3(BLOCK), 0, ctx->stream, g);
        } else {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gdt_search<false>), search, dim3(BLOCK), 0, ctx->stream, g);
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gdt_final<false>), final_grid, dim3(BLOCK), 0, ctx->stream, g);
        }
    }
    HIP_TRY(hipGetLastError());
    return FCZ_OK;
}

// fcz_gdt and fcz_gdt_packed: the host arrays as fcz_superpose's inputs, then GDT_OUT 10 .. 17, the outputs in the struct's order
static int gdt_host(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, const uint8_t* mask_pred, const uint32_t* bound,
                    bool packed, uint32_t n, uint32_t rows_per, int layout, int slot, uint32_t levels, uint32_t iterations, uint32_t runs, const fcz_gdt_out& o) {
    const dense_bytes b(packed, n, rows_per, layout, bound);
    const size_t c = n;
    return staged_call(ctx, {{pos_true, b.pos, DENSE_IN}, {mask_true, b.mask, DENSE_IN + 1}, {bound, b.bound, DENSE_IN + 3}, {pos_pred, b.pos, LDDT_PRED},
                             {mask_pred, b.mask, LDDT_PRED + 1}},
                       {{o.gdt_counts, 20 * c, GDT_OUT}, {o.sites, 4 * c, GDT_OUT + 1}, {o.rot, 180 * c, GDT_OUT + 2}, {o.trans, 60 * c, GDT_OUT + 3},
                        {o.seed, 20 * c, GDT_OUT + 4}, {o.run, 20 * c, GDT_OUT + 5}, {o.selected, 20 * c, GDT_OUT + 6}, {o.within, b.rows, GDT_OUT + 7}},
                       [&](const void* const* in, void* const* out) {
        const fcz_gdt_out d{(int32_t*)out[0], (int32_t*)out[1], (float*)out[2], (float*)out[3], (int32_t*)out[4], (int32_t*)out[5], (int32_t*)out[6], (uint8_t*)out[7]};
        return gdt_rows(ctx, (const float*)in[0], (const uint8_t*)in[1], (const float*)in[3], (const uint8_t*)in[4], (const uint32_t*)in[2], packed, n, rows_per,
                        layout, slot, levels, iterations, runs, d);
    });
}

extern "C" {

int fcz_gdt_dev(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev, const uint8_t* mask_pred_dev,
                const uint32_t* length_dev, uint32_t n, uint32_t L, int layout, int slot, uint32_t levels, uint32_t iterations, uint32_t runs,
                const fcz_gdt_out* out_dev) {
    if (!gdt_args_ok(ctx, pos_true_dev, mask_true_dev, pos_pred_dev, layout, slot, L, iterations, runs, out_dev) || !bound_ok(false, length_dev, n, L))
        return FCZ_E_INVALID_ARG;
    return gdt_rows(ctx, pos_true_dev, mask_true_dev, pos_pred_dev, mask_pred_dev, length_dev, false, n, L, layout, slot, levels, iterations, runs, *out_dev);
}

int fcz_gdt_packed_dev(fcz_ctx* ctx, const float* pos_true_dev, const uint8_t* mask_true_dev, const float* pos_pred_dev, const uint8_t* mask_pred_dev,
                       const uint32_t* row_off_dev, uint32_t n, uint32_t R, int layout, int slot, uint32_t levels, uint32_t iterations, uint32_t runs,
                       const fcz_gdt_out* out_dev) {
    if (!gdt_args_ok(ctx, pos_true_dev, mask_true_dev, pos_pred_dev, layout, slot, R, iterations, runs, out_dev) || !bound_ok(true, row_off_dev, n, R))
        return FCZ_E_INVALID_ARG;
    return gdt_rows(ctx, pos_true_dev, mask_true_dev, pos_pred_dev, mask_pred_dev, row_off_dev, true, n, R, layout, slot, levels, iterations, runs, *out_dev);
}

int fcz_gdt(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, const uint8_t* mask_pred, const uint32_t* length,
            uint32_t n, uint32_t L, int layout, int slot, uint32_t levels, uint32_t iterations, uint32_t runs, const fcz_gdt_out* out) {
    if (!gdt_args_ok(ctx, pos_true, mask_true, pos_pred, layout, slot, L, iterations, runs, out) || !bound_ok(false, length, n, L)) return FCZ_E_INVALID_ARG;
    return gdt_host(ctx, pos_true, mask_true, pos_pred, mask_pred, length, false, n, L, layout, slot, levels, iterations, runs, *out);
}

int fcz_gdt_packed(fcz_ctx* ctx, const float* pos_true, const uint8_t* mask_true, const float* pos_pred, const uint8_t* mask_pred, const uint32_t* row_off,
                   uint32_t n, uint32_t R, int layout, int slot, uint32_t levels, uint32_t iterations, uint32_t runs, const fcz_gdt_out* out) {
    if (!gdt_args_ok(ctx, pos_true, mask_true, pos_pred, layout, slot, R, iterations, runs, out) || !bound_ok(true, row_off, n, R)) return FCZ_E_INVALID_ARG;
    return gdt_host(ctx, pos_true, mask_true, pos_pred, mask_pred, row_off, true, n, R, layout, slot, levels, iterations, runs, *out);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// TM-align-style structural alignment of chain pairs (fcz_tmalign.h; no counterpart in the reference)
// ------------------------------------------------------------------------------------------------
constexpr size_t TMALIGN_DIR_BUDGET = (size_t)256 << 20;   // bytes of traceback bits a call may hold: it bounds the resident wavefronts

static bool tmalign_set_ok(const fcz_chain_set* s) {
    return s && s->pos && s->mask && (s->row_off ? true : s->rows != 0) && s->rows <= SUPERPOSE_MAX_ROWS;
}

static bool tmalign_common_ok(const fcz_ctx* ctx, const fcz_chain_set* a, const fcz_chain_set* b, const int32_t* pairs, uint32_t m, uint32_t wa, uint32_t wb,
                              int layout, int slot) {
    if (!ctx || !tmalign_set_ok(a) || !tmalign_set_ok(b) || (m && !pairs)) return false;
    if (fcz_dense_width(layout) <= 0 || slot < 0 || slot >= fcz_dense_width(layout)) return false;
    return wa >= 1 && wa <= TMALIGN_MAX_WIDTH && wb >= 1 && wb <= TMALIGN_MAX_WIDTH;
}

static bool tmalign_gap_ok(double g) { return g >= 0.0 && g <= TMALIGN_MAX_GAP; }   // (false for a NaN)

static bool tmalign_params_ok(const fcz_tmalign_params* p) {
    if (!p || p->n_gaps < 1 || p->n_gaps > TMALIGN_MAX_GAPS || p->refine > TMALIGN_MAX_ROUNDS || p->dp_rounds > TMALIGN_MAX_ROUNDS ||
        p->iterations > TM_MAX_ITERATIONS)
        return false;
    for (uint32_t i = 0; i < p->n_gaps; i++) if (!tmalign_gap_ok(p->gaps[i])) return false;
    return true;
}

static tmalign_set tmalign_set_of(const fcz_chain_set& s) { return tmalign_set{s.pos, s.mask, s.length, s.row_off, s.n, s.rows}; }

// the wavefront slots of traceback bits a call gets: as many as `want`, within the budget, at least one
static uint32_t tmalign_dir_slots(uint64_t want, uint32_t wa) {
    const uint64_t fit = TMALIGN_DIR_BUDGET / ((size_t)wa * WAVE * sizeof(uint32_t));
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, fit));
}

// fcz_tmalign_dev (params, o) and fcz_tmalign_dp_dev (params NULL: rot_in, trans_in, gap, o.map, o.aligned)
static int tmalign_rows(fcz_ctx* ctx, const fcz_chain_set& a, const fcz_chain_set& b, const int32_t* pairs_dev, uint32_t m, uint32_t wa, uint32_t wb, int layout,
                        int slot, const fcz_tmalign_params* params, const fcz_tmalign_out& o, const float* rot_in, const float* trans_in, double gap) {
    HIP_TRY(hipSetDevice(ctx->device));
    if (m == 0) return FCZ_OK;
    tmalign_args g{};
    g.a = tmalign_set_of(a); g.b = tmalign_set_of(b);
    g.pairs = pairs_dev; g.m = m; g.wa = wa; g.wb = wb; g.A = (uint32_t)fcz_dense_width(layout); g.slot = (uint32_t)slot;
    g.rot = o.rot; g.trans = o.trans; g.tm = o.tm; g.tm_a = o.tm_a; g.tm_b = o.tm_b; g.aligned = o.aligned; g.rmsd = o.rmsd; g.sites_a = o.sites_a;
    g.sites_b = o.sites_b; g.seed = o.seed; g.status = o.status; g.map = o.map; g.dev = o.dev;
    g.rot_in = rot_in; g.trans_in = trans_in;
    if (!params) {
        g.n_gaps = 1; g.G[0] = (int32_t)rint(gap * (double)TMALIGN_Q);
        g.dir_slots = tmalign_dir_slots(std::min<uint64_t>(m, (uint64_t)ctx->n_cu * 4u), wa);
        int rc = ctx->ta_dir.ensure((size_t)g.dir_slots * wa * WAVE * sizeof(uint32_t)); if (rc) return rc;
        g.dir = ctx->ta_dir.as<uint32_t>();
        span_guard sg(ctx, "tmalign");
        hipLaunchKernelGGL(k_ta_dp, dim3(g.dir_slots), dim3(BLOCK), 0, ctx->stream, g);
        HIP_TRY(hipGetLastError());
        return FCZ_OK;
    }
    g.fragments = params->fragments ? 1u : 0u; g.refine = params->refine; g.dp_rounds = params->dp_rounds; g.n_gaps = params->n_gaps;
    for (uint32_t i = 0; i < params->n_gaps; i++) g.G[i] = (int32_t)rint(params->gaps[i] * (double)TMALIGN_Q);
    g.levels = params->levels; g.iterations = params->iterations;
    // the seeds are counted on the device: at most this many items of WAVES_PER_BLOCK seeds a pair, a double per seed
    const uint64_t items = (uint64_t)m * ((ta_seed_bound(wa, wb, g.fragments) + WAVES_PER_BLOCK - 1u) / WAVES_PER_BLOCK);
    const uint32_t search = std::max<uint32_t>(1u, tmalign_dir_slots(std::min<uint64_t>(items, (uint64_t)ctx->n_cu * 2u) * WAVES_PER_BLOCK, wa) / WAVES_PER_BLOCK);
    const uint32_t final_blocks = (uint32_t)std::min<uint64_t>(m, (uint64_t)search * WAVES_PER_BLOCK);
    g.dir_slots = search * WAVES_PER_BLOCK;
    int rc = ctx->ta_dir.ensure((size_t)g.dir_slots * wa * WAVE * sizeof(uint32_t)); if (rc) return rc;
    rc = ctx->ta_scratch.ensure(sizeof(uint64_t) * (2 * (size_t)m + 1) + sizeof(double) * WAVES_PER_BLOCK * (size_t)items + sizeof(uint32_t) * 2 * (size_t)m);
    if (rc) return rc;
    g.dir = ctx->ta_dir.as<uint32_t>();
    uint64_t* counts = ctx->ta_scratch.as<uint64_t>();
    g.item_off = counts + m;
    g.score = reinterpret_cast<double*>(g.item_off + m + 1); g.score_cap = WAVES_PER_BLOCK * items;
    g.nsites = reinterpret_cast<uint32_t*>(g.score + g.score_cap);
    rc = ctx->ta_work.ensure(2 * sizeof(unsigned long long)); if (rc) return rc;
    g.work = ctx->ta_work.as<unsigned long long>();
    HIP_TRY(hipMemsetAsync(g.work, 0, 2 * sizeof(unsigned long long), ctx->stream));
    span_guard sg(ctx, "tmalign");
    hipLaunchKernelGGL(k_ta_count, dim3(std::min(grid_for(m, WAVES_PER_BLOCK), (uint32_t)ctx->n_cu * 16u)), dim3(BLOCK), 0, ctx->stream, g, counts);
    rc = device_scan<uint64_t>(ctx, counts, g.item_off, m); if (rc) return rc;
    hipLaunchKernelGGL(k_ta_search, dim3(search), dim3(BLOCK), 0, ctx->stream, g, 0u);
    hipLaunchKernelGGL(k_ta_search, dim3(search), dim3(BLOCK), 0, ctx->stream, g, 1u);
    hipLaunchKernelGGL(k_ta_final, dim3(final_blocks), dim3(BLOCK), 0, ctx->stream, g);
    HIP_TRY(hipGetLastError());
    return FCZ_OK;
}

// the host forms: the sets' arrays through TA_SETS .. + 5, pairs through TA_PAIRS, then (dp) rot, trans in and map, aligned out through TA_DP_*, or the
// thirteen outputs through TA_OUT .. + 12
static int tmalign_host(fcz_ctx* ctx, const fcz_chain_set& a, const fcz_chain_set& b, const int32_t* pairs, uint32_t m, uint32_t wa, uint32_t wb, int layout, int slot,
                        const fcz_tmalign_params* params, const fcz_tmalign_out& o, const float* rot, const float* trans, double gap) {
    const dense_bytes ba(a.row_off != nullptr, a.n, a.rows, layout, a.row_off ? a.row_off : a.length);
    const dense_bytes bb(b.row_off != nullptr, b.n, b.rows, layout, b.row_off ? b.row_off : b.length);
    const size_t c = m, w = (size_t)m * wa;
    // an array without a byte has no copy on the device (staged_call). No kernel reads an element of it -- its chains are empty or do not exist -- so the
    // pairs, which exist whenever m > 0, stand in where a pointer must not be NULL
    auto sets = [&](const void* const* in, fcz_chain_set* da, fcz_chain_set* db) {
        auto at = [&](int i) { return in[i] ? in[i] : in[6]; };   // (in[6]: the pairs, the seventh input of both lists)
        *da = fcz_chain_set{(const float*)at(0), (const uint8_t*)at(1), a.row_off ? nullptr : (const uint32_t*)in[2], a.row_off ? (const uint32_t*)at(2) : nullptr, a.n, a.rows};
        *db = fcz_chain_set{(const float*)at(3), (const uint8_t*)at(4), b.row_off ? nullptr : (const uint32_t*)in[5], b.row_off ? (const uint32_t*)at(5) : nullptr, b.n, b.rows};
    };
    if (!params)
        return staged_call(ctx, {{a.pos, ba.pos, TA_SETS}, {a.mask, ba.mask, TA_SETS + 1}, {a.row_off ? a.row_off : a.length, ba.bound, TA_SETS + 2}, {b.pos, bb.pos, TA_SETS + 3},
                             {b.mask, bb.mask, TA_SETS + 4},
                                 {b.row_off ? b.row_off : b.length, bb.bound, TA_SETS + 5}, {pairs, 8 * c, TA_PAIRS}, {rot, 36 * c, TA_DP_ROT}, {trans, 12 * c, TA_DP_TRANS}},
                           {{o.map, 4 * w, TA_DP_MAP}, {o.aligned, 4 * c, TA_DP_ALIGNED}}, [&](const void* const* in, void* const* out) {
            fcz_chain_set da, db; sets(in, &da, &db);
            fcz_tmalign_out d{}; d.map = (int32_t*)out[0]; d.aligned = (int32_t*)out[1];
            return tmalign_rows(ctx, da, db, (const int32_t*)in[6], m, wa, wb, layout, slot, nullptr, d, (const float*)in[7], (const float*)in[8], gap);
        });
    return staged_call(ctx, {{a.pos, ba.pos, TA_SETS}, {a.mask, ba.mask, TA_SETS + 1}, {a.row_off ? a.row_off : a.length, ba.bound, TA_SETS + 2}, {b.pos, bb.pos, TA_SETS + 3},
                             {b.mask, bb.mask, TA_SETS + 4},
                             {b.row_off ? b.row_off : b.length, bb.bound, TA_SETS + 5}, {pairs, 8 * c, TA_PAIRS}},
                       {{o.rot, 36 * c, TA_OUT}, {o.trans, 12 * c, TA_OUT + 1}, {o.tm, 4 * c, TA_OUT + 2}, {o.tm_a, 4 * c, TA_OUT + 3}, {o.tm_b, 4 * c, TA_OUT + 4},
                        {o.aligned, 4 * c, TA_OUT + 5}, {o.rmsd, 4 * c, TA_OUT + 6}, {o.sites_a, 4 * c, TA_OUT + 7}, {o.sites_b, 4 * c, TA_OUT + 8}, {o.seed, 4 * c, TA_OUT + 9},
                        {o.status, 4 * c, TA_OUT + 10}, {o.map, 4 * w, TA_OUT + 11}, {o.dev, 4 * w, TA_OUT + 12}},
                       [&](const void* const* in, void* const* out) {
        fcz_chain_set da, db; sets(in, &da, &db);
        const fcz_tmalign_out d{(float*)out[0], (float*)out[1], (float*)out[2], (float*)out[3], (float*)out[4], (int32_t*)out[5], (float*)out[6], (int32_t*)out[7],
                                (int32_t*)out[8], (int32_t*)out[9], (int32_t*)out[10], (int32_t*)out[11], (float*)out[12]};
        return tmalign_rows(ctx, da, db, (const int32_t*)in[6], m, wa, wb, layout, slot, params, d, nullptr, nullptr, 0.0);
    });
}

extern "C" {

uint64_t fcz_tmalign_seeds(uint32_t sites_a, uint32_t sites_b, uint32_t fragments) { return ta_seed_count(sites_a, sites_b, fragments); }

int fcz_tmalign_seed(uint32_t sites_a, uint32_t sites_b, uint32_t fragments, uint64_t seed, int32_t* kind, int32_t* shift, uint32_t* start_a, uint32_t* start_b,
                     uint32_t* length) {
    if (!kind || !shift || !start_a || !start_b || !length || seed >= ta_seed_count(sites_a, sites_b, fragments)) return FCZ_E_INVALID_ARG;
    ta_seed_what(sites_a, sites_b, seed, kind, shift, start_a, start_b, length);
    return FCZ_OK;
}

int fcz_tmalign_last_work(fcz_ctx* ctx, uint64_t* dps, uint64_t* cells) {
    if (!ctx || !dps || !cells) return FCZ_E_INVALID_ARG;
    unsigned long long w[2] = {0, 0};
    if (ctx->ta_work.p) {
        HIP_TRY(hipSetDevice(ctx->device));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        HIP_TRY(hipMemcpy(w, ctx->ta_work.p, sizeof w, hipMemcpyDeviceToHost));
    }
    *dps = w[0]; *cells = w[1];
    return FCZ_OK;
}

int fcz_tmalign_dev(fcz_ctx* ctx, const fcz_chain_set* a_dev, const fcz_chain_set* b_dev, const int32_t* pairs_dev, uint32_t m, uint32_t wa, uint32_t wb, int layout,
                    int slot, const fcz_tmalign_params* params, const fcz_tmalign_out* out_dev) {
    if (!tmalign_common_ok(ctx, a_dev, b_dev, pairs_dev, m, wa, wb, layout, slot) || !tmalign_params_ok(params) || !out_dev || !out_dev->rot || !out_dev->trans)
        return FCZ_E_INVALID_ARG;
    return tmalign_rows(ctx, *a_dev, *b_dev, pairs_dev, m, wa, wb, layout, slot, params, *out_dev, nullptr, nullptr, 0.0);
}

int fcz_tmalign_dp_dev(fcz_ctx* ctx, const fcz_chain_set* a_dev, const fcz_chain_set* b_dev, const int32_t* pairs_dev, uint32_t m, uint32_t wa, uint32_t wb, int layout,
                       int slot, const float* rot_dev, const float* trans_dev, double gap, int32_t* map_dev, int32_t* aligned_dev) {
    if (!tmalign_common_ok(ctx, a_dev, b_dev, pairs_dev, m, wa, wb, layout, slot) || !tmalign_gap_ok(gap) || !rot_dev || !trans_dev || !map_dev) return FCZ_E_INVALID_ARG;
    fcz_tmalign_out o{}; o.map = map_dev; o.aligned = aligned_dev;
    return tmalign_rows(ctx, *a_dev, *b_dev, pairs_dev, m, wa, wb, layout, slot, nullptr, o, rot_dev, trans_dev, gap);
}

int fcz_tmalign(fcz_ctx* ctx, const fcz_chain_set* a, const fcz_chain_set* b, const int32_t* pairs, uint32_t m, uint32_t wa, uint32_t wb, int layout, int slot,
                const fcz_tmalign_params* params, const fcz_tmalign_out* out) {
    if (!tmalign_common_ok(ctx, a, b, pairs, m, wa, wb, layout, slot) || !tmalign_params_ok(params) || !out || !out->rot || !out->trans) return FCZ_E_INVALID_ARG;
    return tmalign_host(ctx, *a, *b, pairs, m, wa, wb, layout, slot, params, *out, nullptr, nullptr, 0.0);
}

int fcz_tmalign_dp(fcz_ctx* ctx, const fcz_chain_set* a, const fcz_chain_set* b, const int32_t* pairs, uint32_t m, uint32_t wa, uint32_t wb, int layout, int slot,
                   const float* rot, const float* trans, double gap, int32_t* map, int32_t* aligned) {
    if (!tmalign_common_ok(ctx, a, b, pairs, m, wa, wb, layout, slot) || !tmalign_gap_ok(gap) || !rot || !trans || !map) return FCZ_E_INVALID_ARG;
    fcz_tmalign_out o{}; o.map = map; o.aligned = aligned;
    return tmalign_host(ctx, *a, *b, pairs, m, wa, wb, layout, slot, nullptr, o, rot, trans, gap);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// rigid frames of dense tensors (fcz_frames.h; no counterpart in the reference)
// ------------------------------------------------------------------------------------------------
// the kernel's table: slots of the three defining atoms per (type, group) in the layout
static frames_table frames_make_table(int layout) {
    frames_table t;
    memset(t.slot, 255, sizeof t.slot);
    for (int ty = 0; ty < (int)FR_TYPES; ty++)
        for (int g = 0; g < (int)FR_GROUPS; g++) {
            if (g >= 4 && ty >= 20) continue;
            int s[3];
            bool all = true;
            for (int j = 0; j < 3; j++) {
                const int ac = fcz_frame_atom(ty < 20 ? ty : 0, g, j);
                // N, CA, C, O have the same slot in every type: groups 0 and 3 are read through ALA, so a type without an O of its own keeps them
                s[j] = ac < 0 ? -1 : fcz_dense_slot(layout, g < 4 ? 0 : ty, ac);
                all = all && s[j] >= 0;
            }
            if (all) for (int j = 0; j < 3; j++) t.slot[ty][g][j] = (uint8_t)s[j];
        }
    return t;
}

static bool frames_args_ok(const fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint8_t* aatype, uint32_t L, int layout, int groups,
                           const float* rot, const float* trans, const uint8_t* frame_mask) {
    return ctx && pos && mask && rot && trans && frame_mask && fcz_dense_width(layout) > 0 && fcz_frames_width(groups) > 0 &&
           (aatype || groups == FCZ_FRAMES_BACKBONE) && L != 0;
}

static int frames_rows(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint8_t* aatype_dev, const uint32_t* length_dev, uint32_t n,
                       uint32_t L, int layout, int groups, float* rot_dev, float* trans_dev, uint8_t* frame_mask_dev) {
    HIP_TRY(hipSetDevice(ctx->device));
    if (n == 0) return FCZ_OK;
    const frames_args g{pos_dev, mask_dev, aatype_dev, length_dev, (uint64_t)n * L, L, rot_dev, trans_dev, frame_mask_dev};
    const uint32_t G = (uint32_t)fcz_frames_width(groups), T = FR_ITEMS / G;
    const uint64_t n_tiles = (g.rows + T - 1) / T;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(n_tiles, (uint64_t)ctx->n_cu * 8u);
    const frames_table tab = frames_make_table(layout);
    span_guard sg(ctx, "frames");
    dispatch_layout(layout, [&](auto A) {
        if (G == 1) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_frames<decltype(A)::value, 1>), dim3(blocks), dim3(BLOCK), 0, ctx->stream, g, n_tiles, tab);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_frames<decltype(A)::value, 8>), dim3(blocks), dim3(BLOCK), 0, ctx->stream, g, n_tiles, tab);
    });
    HIP_TRY(hipGetLastError());
    return FCZ_OK;
}

extern "C" {

int fcz_frames_width(int groups) { return groups == FCZ_FRAMES_BACKBONE ? 1 : groups == FCZ_FRAMES_ALL ? 8 : -1; }

int fcz_frame_atom(int rc, int group, int j) {
    if (rc < 0 || rc >= FCZ_N_RES_CODES || group < 0 || group >= (int)FR_GROUPS || j < 0 || j > 2) return -1;
    static const int backbone[3] = {2, 1, 0}, psi[3] = {1, 2, 3};             // (C, CA, N) and (CA, C, O): atom codes 0 .. 3 are N, CA, C, O
    if (group == 0) return backbone[j];
    if (group == 3) return psi[j];
    if (group < 4) return -1;
    const int k = group - 4;
    if (fcz_chi_atom(rc, k) < 0) return -1;
    const int c = k + 1 + j;                                                  // position in the chain N, CA, CB, X1 .. X4
    return c == 0 ? 0 : c == 1 ? 1 : c == 2 ? 4 : fcz_chi_atom(rc, c - 3);    // (atom code 4 is CB)
}

int fcz_frame_ambiguous(int rc, int group) {
    // the types whose chi ends in two atoms that a 180-degree turn exchanges: ASP OD1 / OD2, PHE and TYR CD1 / CD2 (chi2), GLU OE1 / OE2 (chi3)
    return ((rc == 3 || rc == 13 || rc == 18) && group == 5) || (rc == 6 && group == 6) ? 1 : 0;
}

int fcz_frames_dev(fcz_ctx* ctx, const float* pos_dev, const uint8_t* mask_dev, const uint8_t* aatype_dev, const uint32_t* length_dev, uint32_t n, uint32_t L,
                   int layout, int groups, float* rot_dev, float* trans_dev, uint8_t* frame_mask_dev) {
    if (!frames_args_ok(ctx, pos_dev, mask_dev, aatype_dev, L, layout, groups, rot_dev, trans_dev, frame_mask_dev)) return FCZ_E_INVALID_ARG;
    return frames_rows(ctx, pos_dev, mask_dev, aatype_dev, length_dev, n, L, layout, groups, rot_dev, trans_dev, frame_mask_dev);
}

// the host arrays through DENSE_IN 0 .. 3 and DENSE_OUT 10 .. 12
int fcz_frames(fcz_ctx* ctx, const float* pos, const uint8_t* mask, const uint8_t* aatype, const uint32_t* length, uint32_t n, uint32_t L, int layout,
               int groups, float* rot, float* trans, uint8_t* frame_mask) {
    if (!frames_args_ok(ctx, pos, mask, aatype, L, layout, groups, rot, trans, frame_mask)) return FCZ_E_INVALID_ARG;
    const dense_bytes b(false, n, L, layout, length);
    const size_t items = b.rows * (size_t)fcz_frames_width(groups);
    return staged_call(ctx, {{pos, b.pos, DENSE_IN}, {mask, b.mask, DENSE_IN + 1}, {aatype, b.rows, DENSE_IN + 2}, {length, b.bound, DENSE_IN + 3}},
                       {{rot, items * 9 * sizeof(float), DENSE_OUT}, {trans, items * 3 * sizeof(float), DENSE_OUT + 1}, {frame_mask, items, DENSE_OUT + 2}},
                       [&](const void* const* in, void* const* out) {
        return frames_rows(ctx, (const float*)in[0], (const uint8_t*)in[1], (const uint8_t*)in[2], (const uint32_t*)in[3], n, L, layout, groups, (float*)out[0],
                           (float*)out[1], (uint8_t*)out[2]);
    });
}

// ------------------------------------------------------------------------------------------------
// dense tensors -> fcz_chain_batch -> FCZ records (fcz_undense.h; beside Foldcomp::compress, src/foldcomp.cpp:562, which takes
// the flat atom list these entry points build)
// ------------------------------------------------------------------------------------------------
// the kernels' table: canonical position -> slot of the layout
static undense_table undense_make_table(int layout) {
    undense_table t;
    memset(t.slot, 255, sizeof t.slot);
    for (int rc = 0; rc < FCZ_N_RES_CODES; rc++)
        for (int j = 0; j < host_tab::h_res_natoms[rc]; j++) {
            const int slot = fcz_dense_slot(layout, rc, fcz_res_code_atom(rc, j, 0));
            if (slot >= 0) t.slot[rc * FCZ_MAX_RES_ATOMS + j] = (uint8_t)slot;
        }
    return t;
}

static bool undense_args_ok(const fcz_ctx* ctx, const fcz_dense_in* in, uint32_t n, uint32_t L, int layout, int anchor_threshold) {
    if (!ctx || fcz_dense_width(layout) < 0 || L == 0 || anchor_threshold <= 0) return false;
    if (n == 0) return true;
    return in && in->pos && in->mask && in->aatype && in->length && (!in->titles == !in->title_off);
}
// the packed form: row_off in place of length and L
static bool undense_packed_args_ok(const fcz_ctx* ctx, const fcz_dense_in* in, const uint32_t* row_off, uint32_t n, int layout, int anchor_threshold) {
    if (!ctx || fcz_dense_width(layout) < 0 || anchor_threshold <= 0) return false;
    if (n == 0) return true;
    return in && in->pos && in->mask && in->aatype && row_off && (!in->titles == !in->title_off);
}

// fcz_undense_dev and fcz_undense_packed_dev: row_off == NULL is the padded form [n][L], otherwise chain c = rows row_off[c] ..
// row_off[c + 1] of R (arguments checked by the caller)
static int undense_rows(fcz_ctx* ctx, const fcz_dense_in* in, uint32_t n, uint32_t L, const uint32_t* row_off, uint32_t R_in, int layout,
                        int anchor_threshold, fcz_chain_batch* out, uint32_t counts[3], int32_t* chain_status_dev) {
    HIP_TRY(hipSetDevice(ctx->device));
    memset(out, 0, sizeof *out);
    memset(&ctx->ud_batch, 0, sizeof ctx->ud_batch);
    ctx->ud_status = nullptr;
    counts[0] = counts[1] = counts[2] = 0;
    out->anchor_threshold = ctx->ud_batch.anchor_threshold = anchor_threshold;
    if (n == 0) return FCZ_OK;
    const size_t C = n, rows = row_off ? (size_t)R_in : C * (size_t)L;
    // per chain: residues, atoms, status, flags (overflow of the scans) | res_off, first atom of the chain | packed: tiles, first tile
    const size_t ch_nres = 0, ch_natoms = 4 * C, ch_status = 8 * C, ch_flags = 12 * C, ch_resoff = ch_flags + 16, ch_aoff = ch_resoff + 4 * (C + 1);
    const size_t ch_tiles = ch_aoff + 4 * (C + 1), ch_toff = ch_tiles + 4 * C;
    int rc;
    if ((rc = ctx->ud[U_ROWS].ensure(2 * rows + 16)) || (rc = ctx->ud[U_CHAIN].ensure(ch_toff + 4 * (C + 1)))) return rc;
    char* bc = (char*)ctx->ud[U_CHAIN].p;
    uint16_t* row_word = ctx->ud[U_ROWS].as<uint16_t>();
    uint32_t* n_res = (uint32_t*)(bc + ch_nres); uint32_t* n_atoms = (uint32_t*)(bc + ch_natoms); int32_t* status = (int32_t*)(bc + ch_status);
    uint32_t* ovf = (uint32_t*)(bc + ch_flags); uint32_t* res_off = (uint32_t*)(bc + ch_resoff); uint32_t* chain_aoff = (uint32_t*)(bc + ch_aoff);
    uint32_t* chain_tiles = (uint32_t*)(bc + ch_tiles); uint32_t* tile_off = (uint32_t*)(bc + ch_toff);
    const undense_table tab = undense_make_table(layout);
    const undense_in g{in->pos, in->mask, in->aatype, in->length, in->plddt};
    const uint32_t tiles_per_chain = grid_for(L, DN_TILE);
    const ud_padded padded{in->length, L, tiles_per_chain, (uint64_t)n * tiles_per_chain};   // every index into the dense arrays is 64-bit: n * L * A * 3 may pass 2^32
    const ud_packed packed{row_off, R_in, n, tile_off};
    HIP_TRY(hipMemsetAsync(ovf, 0, 16, ctx->stream));
    {
        span_guard sg(ctx, "undense");
        const dim3 grid(std::min<uint32_t>(n, (uint32_t)ctx->n_cu * 16u));
        dispatch_layout(layout, [&](auto A) {
            if (row_off)
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_undense_count<decltype(A)::value, ud_packed>), grid, dim3(BLOCK), 0, ctx->stream, g, n, packed, tab, row_word,
                                   n_res, n_atoms, status, chain_tiles);
            else
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_undense_count<decltype(A)::value, ud_padded>), grid, dim3(BLOCK), 0, ctx->stream, g, n, padded, tab, row_word,
                                   n_res, n_atoms, status, (uint32_t*)nullptr);
        });
    }
    if ((rc = device_scan<uint32_t>(ctx, n_res, res_off, n, ovf)) || (rc = device_scan<uint32_t>(ctx, n_atoms, chain_aoff, n, ovf))) return rc;
    if (row_off && (rc = device_scan<uint32_t>(ctx, chain_tiles, tile_off, n))) return rc;   // (at most residues / 64 + n tiles: no overflow the first scan does not see)
    HIP_TRY(hipGetLastError());
    auto& pin = ctx->pinned->undense;
    HIP_TRY(hipMemcpyAsync(&pin.residues, res_off + n, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(&pin.atoms, chain_aoff + n, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(&pin.overflow, ovf, 4, hipMemcpyDeviceToHost, ctx->stream));
    if (chain_status_dev) HIP_TRY(hipMemcpyAsync(chain_status_dev, status, 4 * C, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (pin.overflow) return FCZ_E_INVALID_ARG;                // the flat batch counts residues and atoms in 32 bits: split the call
    const uint32_t R = pin.residues, M = pin.atoms;
    // the batch arrays: [atoms] x y z code | [residues + 1] atom_off, [residues] bfac code | [chains] first residue, first atom,
    // [chains + 1] zero title offsets, [chains] chain id
    const size_t oa_y = 4 * (size_t)M, oa_z = 8 * (size_t)M, oa_c = 12 * (size_t)M;
    const size_t or_bf = 4 * ((size_t)R + 1), or_rc = or_bf + 4 * (size_t)R;
    const size_t oc_fa = 4 * C, oc_tit = 8 * C, oc_id = oc_tit + 4 * (C + 1);
    if ((rc = ctx->ud[U_OUT_A].ensure(13 * (size_t)M + 16)) || (rc = ctx->ud[U_OUT_R].ensure(or_rc + R + 16)) || (rc = ctx->ud[U_OUT_C].ensure(oc_id + C + 16))) return rc;
    char* ba = (char*)ctx->ud[U_OUT_A].p; char* br = (char*)ctx->ud[U_OUT_R].p; char* bm = (char*)ctx->ud[U_OUT_C].p;
    const undense_out o{(uint32_t*)br, (float*)ba, (float*)(ba + oa_y), (float*)(ba + oa_z), (uint8_t*)(ba + oa_c), (uint8_t*)(br + or_rc), (float*)(br + or_bf)};
    HIP_TRY(hipMemsetAsync(o.atom_off, 0, 4, ctx->stream));    // (a batch without residues: atom_off[0] has no writer)
    if (!in->title_off) HIP_TRY(hipMemsetAsync(bm + oc_tit, 0, 4 * (C + 1), ctx->stream));
    if (!in->first_res_index || !in->first_atom_index || !in->chain_id)
        hipLaunchKernelGGL(k_undense_defaults, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, ctx->stream, n, in->first_res_index ? nullptr : (int32_t*)bm,
                           in->first_atom_index ? nullptr : (int32_t*)(bm + oc_fa), in->chain_id ? nullptr : bm + oc_id);
    if (R) {
        span_guard sg(ctx, "undense");
        // (packed: the tiles are counted on the device only; at most one per 64 residues and one more per chain)
        const uint64_t n_tiles = row_off ? (uint64_t)R / DN_TILE + n : padded.tiles;
        const dim3 grid((uint32_t)std::min<uint64_t>(n_tiles, (uint64_t)ctx->n_cu * 16u));
        dispatch_layout(layout, [&](auto A) {
            if (row_off)
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_undense_fill<decltype(A)::value, ud_packed>), grid, dim3(BLOCK), 0, ctx->stream, g, packed, tab,
                                   (const uint16_t*)row_word, (const uint32_t*)res_off, (const uint32_t*)chain_aoff, o);
            else
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_undense_fill<decltype(A)::value, ud_padded>), grid, dim3(BLOCK), 0, ctx->stream, g, padded, tab,
                                   (const uint16_t*)row_word, (const uint32_t*)res_off, (const uint32_t*)chain_aoff, o);
        });
    }
    HIP_TRY(hipGetLastError());
    fcz_chain_batch& b = ctx->ud_batch;
    b.n_chains = n; b.n_residues = R; b.n_atoms = M; b.anchor_threshold = anchor_threshold;
    b.res_off = res_off; b.atom_off = o.atom_off; b.x = o.x; b.y = o.y; b.z = o.z; b.atom_code = o.atom_code; b.res_code = o.res_code; b.bfac_ca = o.bfac_ca;
    b.first_res_index = in->first_res_index ? in->first_res_index : (const int32_t*)bm;
    b.first_atom_index = in->first_atom_index ? in->first_atom_index : (const int32_t*)(bm + oc_fa);
    b.chain_id = in->chain_id ? in->chain_id : bm + oc_id;
    b.title_off = in->title_off ? in->title_off : (const uint32_t*)(bm + oc_tit);
    b.titles = in->titles ? in->titles : bm + oc_tit;         // (no title has a byte: any valid pointer)
    ctx->ud_status = status;
    counts[0] = n; counts[1] = R; counts[2] = M;
    *out = b;
    return FCZ_OK;
}

int fcz_undense_dev(fcz_ctx* ctx, const fcz_dense_in* in, uint32_t n, uint32_t L, int layout, int anchor_threshold,
                    fcz_chain_batch* out, uint32_t counts[3], int32_t* chain_status_dev) {
    if (!undense_args_ok(ctx, in, n, L, layout, anchor_threshold) || !out || !counts) return FCZ_E_INVALID_ARG;
    return undense_rows(ctx, in, n, L, nullptr, 0, layout, anchor_threshold, out, counts, chain_status_dev);
}

int fcz_undense_packed_dev(fcz_ctx* ctx, const fcz_dense_in* in, const uint32_t* row_off_dev, uint32_t n, uint32_t R, int layout,
                           int anchor_threshold, fcz_chain_batch* out, uint32_t counts[3], int32_t* chain_status_dev) {
    if (!undense_packed_args_ok(ctx, in, row_off_dev, n, layout, anchor_threshold) || !out || !counts) return FCZ_E_INVALID_ARG;
    return undense_rows(ctx, in, n, 1, row_off_dev, R, layout, anchor_threshold, out, counts, chain_status_dev);
}

int fcz_undense_fetch(fcz_ctx* ctx, const fcz_chain_batch* hb, int32_t* chain_status) {
    if (!ctx) return FCZ_E_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    const fcz_chain_batch& d = ctx->ud_batch;
    const size_t C = d.n_chains;
    if (C == 0) return FCZ_OK;
    if (hb) {
        uint32_t TB = 0;
        HIP_TRY(hipMemcpyAsync(&TB, d.title_off + C, 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        int rc = fetch_batch(ctx, *hb, d, TB);
        if (rc) return rc;
    }
    if (chain_status) HIP_TRY(hipMemcpyAsync(chain_status, ctx->ud_status, 4 * C, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return FCZ_OK;
}

// fcz_compress_dense_begin_dev and its packed form (row_off_dev != NULL), arguments checked by the caller
static int compress_dense_rows(fcz_ctx* ctx, const fcz_dense_in* in, uint32_t n, uint32_t L, const uint32_t* row_off_dev, uint32_t R, int layout,
                               int anchor_threshold, uint32_t counts[3], uint64_t* fcz_bytes) {
    *fcz_bytes = 0; ctx->ud_fcz_bytes = 0;
    fcz_chain_batch b;
    int rc = undense_rows(ctx, in, n, L, row_off_dev, R, layout, anchor_threshold, &b, counts, nullptr);
    if (rc || n == 0) return rc;
    claim_staging(ctx);
    if ((rc = compress_resident_batch(ctx, ctx->ud_batch, &ctx->ud_fcz_bytes, fcz_bytes))) return rc;
    hipLaunchKernelGGL(k_undense_merge_status, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, ctx->stream, n, ctx->ud_status, ctx->pool[KEPT_STATUS].as<int32_t>());
    HIP_TRY(hipGetLastError());
    return FCZ_OK;
}

int fcz_compress_dense_begin_dev(fcz_ctx* ctx, const fcz_dense_in* in, uint32_t n, uint32_t L, int layout, int anchor_threshold,
                                 uint32_t counts[3], uint64_t* fcz_bytes) {
    if (!fcz_bytes || !counts || !undense_args_ok(ctx, in, n, L, layout, anchor_threshold)) return FCZ_E_INVALID_ARG;
    return compress_dense_rows(ctx, in, n, L, nullptr, 0, layout, anchor_threshold, counts, fcz_bytes);
}

int fcz_compress_dense_packed_begin_dev(fcz_ctx* ctx, const fcz_dense_in* in, const uint32_t* row_off_dev, uint32_t n, uint32_t R, int layout,
                                        int anchor_threshold, uint32_t counts[3], uint64_t* fcz_bytes) {
    if (!fcz_bytes || !counts || !undense_packed_args_ok(ctx, in, row_off_dev, n, layout, anchor_threshold)) return FCZ_E_INVALID_ARG;
    return compress_dense_rows(ctx, in, n, 1, row_off_dev, R, layout, anchor_threshold, counts, fcz_bytes);
}

static int compress_dense_fetch(fcz_ctx* ctx, uint64_t* out_off, int32_t* status, uint8_t* blob, hipMemcpyKind kind) {
    if (!ctx) return FCZ_E_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    int rc = fetch_resident(ctx, ctx->ud_batch.n_chains, ctx->ud_fcz_bytes, out_off, status, blob, kind);
    if (rc) return rc;
    if (kind == hipMemcpyDeviceToHost) HIP_TRY(hipStreamSynchronize(ctx->stream));
    return FCZ_OK;
}

int fcz_compress_dense_fetch_dev(fcz_ctx* ctx, uint64_t* out_off_dev, int32_t* status_dev, uint8_t* blob_dev) {
    return compress_dense_fetch(ctx, out_off_dev, status_dev, blob_dev, hipMemcpyDeviceToDevice);
}

// the host arrays of a fcz_dense_in of `rows` rows -> DENSE_IN 0 .. 9 (slot 3: length [n], or row_off [n + 1] of the packed form) -> *dv
static int upload_dense_in(fcz_ctx* ctx, const fcz_dense_in* in, const uint32_t* row_off, uint32_t n, size_t rows, int layout, fcz_dense_in* dv) {
    const size_t C = n, A = (size_t)fcz_dense_width(layout);
    const size_t title_bytes = in->title_off ? in->title_off[n] : 0;
    // floor 16: a present array of zero bytes still gets a device pointer -- undense_rows tells "absent" from "empty" by the pointer, where
    // the rules of staged_call would give it NULL
    const void* dev[10];
    int rc = stage_in(ctx, {{in->pos, rows * A * 3 * sizeof(float), DENSE_IN}, {in->mask, rows * A, DENSE_IN + 1}, {in->aatype, rows, DENSE_IN + 2},
                            {row_off ? row_off : in->length, row_off ? 4 * (C + 1) : 4 * C, DENSE_IN + 3}, {in->plddt, rows * sizeof(float), DENSE_IN + 4},
                            {in->first_res_index, 4 * C, DENSE_IN + 5}, {in->first_atom_index, 4 * C, DENSE_IN + 6}, {in->chain_id, C, DENSE_IN + 7},
                            {in->titles, title_bytes, DENSE_IN + 8}, {in->title_off, 4 * (C + 1), DENSE_IN + 9}}, dev, 16);
    if (rc) return rc;
    *dv = {(const float*)dev[0], (const uint8_t*)dev[1], (const uint8_t*)dev[2], (const uint32_t*)dev[3], (const float*)dev[4],
           (const int32_t*)dev[5], (const int32_t*)dev[6], (const char*)dev[7], (const char*)dev[8], (const uint32_t*)dev[9]};
    return FCZ_OK;
}

int fcz_compress_dense_begin(fcz_ctx* ctx, const fcz_dense_in* in, uint32_t n, uint32_t L, int layout, int anchor_threshold,
                             uint32_t counts[3], uint64_t* fcz_bytes) {
    if (!fcz_bytes || !counts || !undense_args_ok(ctx, in, n, L, layout, anchor_threshold)) return FCZ_E_INVALID_ARG;
    *fcz_bytes = 0; ctx->ud_fcz_bytes = 0;
    HIP_TRY(hipSetDevice(ctx->device));
    if (n == 0) return fcz_compress_dense_begin_dev(ctx, in, 0, L, layout, anchor_threshold, counts, fcz_bytes);
    claim_staging(ctx);
    fcz_dense_in dv;
    int rc = upload_dense_in(ctx, in, nullptr, n, (size_t)n * L, layout, &dv);
    if (rc) return rc;
    return fcz_compress_dense_begin_dev(ctx, &dv, n, L, layout, anchor_threshold, counts, fcz_bytes);
}

int fcz_compress_dense_packed_begin(fcz_ctx* ctx, const fcz_dense_in* in, const uint32_t* row_off, uint32_t n, uint32_t R, int layout,
                                    int anchor_threshold, uint32_t counts[3], uint64_t* fcz_bytes) {
    if (!fcz_bytes || !counts || !undense_packed_args_ok(ctx, in, row_off, n, layout, anchor_threshold)) return FCZ_E_INVALID_ARG;
    *fcz_bytes = 0; ctx->ud_fcz_bytes = 0;
    HIP_TRY(hipSetDevice(ctx->device));
    if (n == 0) return fcz_compress_dense_packed_begin_dev(ctx, in, row_off, 0, R, layout, anchor_threshold, counts, fcz_bytes);
    claim_staging(ctx);
    fcz_dense_in dv;
    int rc = upload_dense_in(ctx, in, row_off, n, R, layout, &dv);
    if (rc) return rc;
    return fcz_compress_dense_packed_begin_dev(ctx, &dv, dv.length, n, R, layout, anchor_threshold, counts, fcz_bytes);
}

int fcz_compress_dense_fetch(fcz_ctx* ctx, uint64_t* out_off, int32_t* status, uint8_t* blob) {
    return compress_dense_fetch(ctx, out_off, status, blob, hipMemcpyDeviceToHost);
}

// ------------------------------------------------------------------------------------------------
// self-test hooks: run the device numerics over caller-chosen float bit patterns so tests can pin
// them against the host libm (tests/test_device_math.py). mode 0: acos_deg, 1: sinf, 2: cosf, 3: deg2rad, 4: norm,
// 5: getCosineTheta, 6-8: place_atom x/y/z, 9/10: sine / cosine of sincosf_pair (the form the kernels call),
// 11: acos_deg_f32 (the float approximation behind the side-chain torsion byte), 12/13: sine / cosine of sincosf_pair_any (any float)
// ------------------------------------------------------------------------------------------------
}  // extern "C"

namespace fcz {
// inputs of the multi-argument self tests come from an integer hash of the index so that the host
// checker (oracle/fcz_oracle.c: fcz_oracle_math_sweep) regenerates exactly the same floats
__device__ __forceinline__ float st_hash_float(uint32_t u, uint32_t salt, float scale) {
    uint32_t h = (u ^ salt) * 2654435761u;
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
    return (float)(int32_t)h * scale;
}
__global__ void k_selftest_math(int mode, uint32_t start_bits, uint32_t stride, uint32_t count, float* __restrict__ outv) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t u = start_bits + i * stride;
    const float x = __uint_as_float(u);
    const float sc = 0x1p-29f;   // hashed coordinates in (-4, 4)
    float r;
    if (mode == 0) r = acos_deg(x);
    else if (mode == 1) r = sinf_glibc(x);
    else if (mode == 2) r = cosf_glibc(x);
    else if (mode == 3) r = deg2rad(x);
    else if (mode == 11) r = acos_deg_f32(x);
    else if (mode == 9 || mode == 10) { float sn, cs; sincosf_pair(x, &sn, &cs); r = mode == 9 ? sn : cs; }
    else if (mode == 12 || mode == 13) { float sn, cs; sincosf_pair_any(x, &sn, &cs); r = mode == 12 ? sn : cs; }
    else if (mode == 4) r = vnorm(v3{st_hash_float(u, 1, sc), st_hash_float(u, 2, sc), st_hash_float(u, 3, sc)});
    else if (mode == 5) r = vcos_theta(v3{st_hash_float(u, 1, sc), st_hash_float(u, 2, sc), st_hash_float(u, 3, sc)},
                                       v3{st_hash_float(u, 4, sc), st_hash_float(u, 5, sc), st_hash_float(u, 6, sc)});
    else {
        // modes 6..8: x / y / z of place_atom on hashed geometry
        const v3 a{st_hash_float(u, 1, sc), st_hash_float(u, 2, sc), st_hash_float(u, 3, sc)};
        const v3 b{st_hash_float(u, 4, sc), st_hash_float(u, 5, sc), st_hash_float(u, 6, sc)};
        const v3 c{st_hash_float(u, 7, sc), st_hash_float(u, 8, sc), st_hash_float(u, 9, sc)};
        const float L = 1.2f + __builtin_fabsf(st_hash_float(u, 10, 0x1p-33f));
        const float ba = 90.0f + st_hash_float(u, 11, 0x1p-25f);          // (26, 154) degrees
        const float ta = st_hash_float(u, 12, 0x1.6p-24f);                // (-176, 176) degrees
        const v3 d = place_atom(a, b, c, L, ba, ta);
        r = (mode == 6) ? d.x : (mode == 7) ? d.y : d.z;
    }
    outv[i] = r;
}
}  // namespace fcz

namespace fcz {
// float4 per lane, grid-stride; U independent loads in flight per lane before the stores; NT: non-temporal loads and stores
typedef float f4v __attribute__((ext_vector_type(4)));
template <int U, bool NT>
__global__ __launch_bounds__(256) void k_copy_f4(const f4v* __restrict__ src, f4v* __restrict__ dst, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride * U) {
        f4v v[U];
#pragma unroll
        for (int u = 0; u < U; u++) { const size_t j = i + (size_t)u * stride; if (j < n) v[u] = NT ? __builtin_nontemporal_load(&src[j]) : src[j]; }
#pragma unroll
        for (int u = 0; u < U; u++) { const size_t j = i + (size_t)u * stride; if (j < n) { if (NT) __builtin_nontemporal_store(v[u], &dst[j]); else dst[j] = v[u]; } }
    }
}
}  // namespace fcz
extern "C" int fcz_selftest_copy(fcz_ctx* ctx, uint64_t bytes, int reps, double* gb_per_s) {
    if (!ctx || !gb_per_s || bytes < 16 || reps < 1) return FCZ_E_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    *gb_per_s = 0.0;
    const size_t n = (size_t)(bytes / 16);
    void *a = nullptr, *b = nullptr;
    if (hipMalloc(&a, n * 16) != hipSuccess) return FCZ_E_NOMEM;
    if (hipMalloc(&b, n * 16) != hipSuccess) { (void)hipFree(a); return FCZ_E_NOMEM; }
    (void)hipMemsetAsync(a, 1, n * 16, ctx->stream);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    // the best of a few shapes of the same kernel (wavefronts in flight per CU, loads in flight per lane, cache policy): the ceiling
    // is what the memory system gives the friendliest access pattern, not what one launch shape happens to reach
    double best = 0.0;
    hipError_t err = hipSuccess;
    for (int shape = 0; shape < 12 && err == hipSuccess; shape++) {
        const unsigned grid = (unsigned)ctx->n_cu * (shape % 3 == 0 ? 8u : shape % 3 == 1 ? 16u : 32u);
        const int variant = shape / 3;                          // 0: one load per lane, 1: four, 2: four non-temporal, 3: one non-temporal
        auto launch = [&]() {
            if (variant == 0) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_copy_f4<1, false>), dim3(grid), dim3(256), 0, ctx->stream, (const f4v*)a, (f4v*)b, n);
            else if (variant == 1) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_copy_f4<4, false>), dim3(grid), dim3(256), 0, ctx->stream, (const f4v*)a, (f4v*)b, n);
            else if (variant == 2) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_copy_f4<4, true>), dim3(grid), dim3(256), 0, ctx->stream, (const f4v*)a, (f4v*)b, n);
            else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_copy_f4<1, true>), dim3(grid), dim3(256), 0, ctx->stream, (const f4v*)a, (f4v*)b, n);
        };
        launch();                                               // warm-up
        (void)hipEventRecord(e0, ctx->stream);
        for (int r = 0; r < reps; r++) launch();
        (void)hipEventRecord(e1, ctx->stream);
        err = hipStreamSynchronize(ctx->stream);
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        if (err == hipSuccess && ms > 0.f) best = std::max(best, 2.0 * (double)(n * 16) * reps / (ms * 1e-3) / 1e9);
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    (void)hipFree(a); (void)hipFree(b);
    if (err != hipSuccess || best <= 0.0) return FCZ_E_HIP;
    *gb_per_s = best;
    return FCZ_OK;
}

extern "C" int fcz_selftest_math(fcz_ctx* ctx, int mode, uint32_t start_bits, uint32_t stride, uint32_t count, float* out_host) {
    if (!ctx || !out_host || mode < 0 || mode > 13) return FCZ_E_INVALID_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    if (count == 0) return FCZ_OK;
    int rc = ctx->selftest_out.ensure(sizeof(float) * (size_t)count); if (rc) return rc;
    hipLaunchKernelGGL(fcz::k_selftest_math, dim3(grid_for(count, 256)), dim3(256), 0, ctx->stream, mode, start_bits, stride, count,
                       ctx->selftest_out.as<float>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_host, ctx->selftest_out.p, sizeof(float) * (size_t)count, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return FCZ_OK;
}
