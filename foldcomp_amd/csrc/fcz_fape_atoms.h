// fcz_fape_atoms.h -- the ALL-ATOM FAPE (AlphaFold 2's side-chain FAPE: the frame aligned point error of the eight rigid groups of every
// residue against every atom of the chain, the truth renamed towards the prediction first) of two batches of frames and dense
// tensors, and its gradient: rot / trans / frame_mask [rows][8] and pos / mask [rows][A] of the truth and of the prediction, aatype
// and swapped [rows] -> sum [rows][8] float32 and points [rows][8] int32, and, for the caller's weights w [rows][8], grad_rot
// [rows][8][3][3], grad_trans [rows][8][3] and grad_pos [rows][A][3] float32. The reference has no such output (include/fcz_hip.h,
// fcz_fape_atoms_dev and fcz_fape_atoms_grad_dev hold the contract). The arithmetic of a term is fcz_fape.h's, by include:
// fape_frame_row, fape_local, fape_term, fape_h.
//
// Item (r, g) is a FRAME (fapea_frame: fape_frame_row on the item r * 8 + g, the truth's second and third columns negated where the
// row is swapped and the group ambiguous), slot (r, a) a POINT (fapea_point: chain_site2 with the truth read at the swap table's
// slot where the row is swapped); every frame of a chain meets every point of it.
//
//   k_fape_atoms<PACKED>               persistent blocks over query tiles of fapea_tile_rows rows (chain_tile). The tile's FRAMES are
//                                      compacted into an LDS list of item numbers in any order (an LDS counter: which lane holds a
//                                      frame changes nothing it computes; every item that is none is written 0 there) and taken in
//                                      rounds of BLOCK, a lane a frame with its 24 floats in registers. Groups 1 and 2 never exist and
//                                      a residue has 3.7 frames on average: 64 rows give about 237 frames, most of one round. The
//                                      chain's POINTS are staged in passes of at most FAPEA_PASS, compacted in ascending (row, slot)
//                                      (chain_stage_slots_ordered), SoA pred x / y / z and true x / y / z with the renaming applied at
//                                      staging time, 24 bytes a point: a lane's sum is a float32 sum in that order whatever the tile,
//                                      pass, grid or batch. Every read of a candidate is a broadcast; a wavefront without a frame in
//                                      the round skips the sweep (wave-uniform) and keeps the barriers.
//   k_fape_atoms_grad_frames<PACKED>   the same sweep with the 3 + 9 accumulators of k_fape_grad_frames.
//   k_fape_atoms_grad_points<PACKED>   the roles exchanged: tiles of lddta_tile_rows rows, the tile's POINTS compacted as slot numbers
//                                      and taken in rounds, a lane a point (six floats); the chain's FRAMES staged in passes of at most
//                                      FAPEA_FRAME_PASS, compacted in ascending (row, group) by the same helper with a divider of 8
//                                      (fapea_div_groups), 25 floats a frame with its weight. A lane gathers grad_pos = sum w (R h).
//   k_chain_fill<fapea_args / fapea_grad_args>   (fcz_chains.h) packed form only, in front of the sweeps.
// Nothing is kept from the value pass; one writer per output element, no atomics on floats; a lane's sums depend on its chain's rows
// alone, so a chain gives the same bytes alone, in any batch, padded or packed.
//
// LDS and occupancy. Value and grad_frames: 1024 points * 24 bytes = 24 576, the frame list 1024 * 2 = 2 048, s_wave and the counter
// 36: 26 660 bytes a block, room for SIX blocks in a CU's 160 KiB. grad_points: FAPEA_FRAME_PASS = 256 frames * 100 bytes = 25 600,
// the point list 64 * 37 * 2 = 4 736, 20 more: 30 356 bytes, room for FIVE. The frame staging examines one item a lane and step
// (FAPEA_FRAME_STEP = BLOCK, 32 rows), and the helper closes a pass when another step might not fit, so a pass is ONE step: about
// 118 frames of the 256 slots, a barrier pair every 32 rows. The alternative the helper allows, 512 slots with the same step (three
// steps, about 354 frames a pass, 51 200 bytes, three blocks a CU), has NOT been tried; neither have other tile rows or point passes:
// tools/fape_atoms_rate.py reports the rate of the constants as they stand.
// `make asm` (gfx950), padded / packed: k_fape_atoms 81 / 93 VGPRs, 26 660 bytes of LDS, 5 / 5 waves per SIMD;
// k_fape_atoms_grad_frames 100 / 112 VGPRs, 26 660 bytes, 4 / 4; k_fape_atoms_grad_points 96 / 98 VGPRs, 30 356 bytes, 5 / 4; no
// scratch in any of the six. REGISTERS, not LDS, bound the blocks on a CU: five, four and five (four) blocks of four wavefronts. The
// compacted sweep costs k_fape's kernels 30 to 40 registers (the two staged slots a lane with their six coordinates, the ballots and
// the round's bookkeeping beside the frame's 24 floats); nobody has tried to win them back.
//
// Every index that scales with rows * A or rows * 8 is 64-bit. A chain's range is clamped to the R rows that exist and a range that
// runs backwards is empty (chain_range), so no read leaves the inputs whatever row_off holds; aatype is clamped to 20 before a table
// is read and the ABI admits only tables whose entries are < A. A weight is read only at an item that is a frame.
#pragma once
#include "fcz_fape.h"
#include "fcz_lddt_atoms.h"

namespace fcz {

constexpr uint32_t FAPEA_GROUPS = 8;
constexpr uint32_t FAPEA_PASS = 1024;             // points staged per candidate pass, at most: 24 KiB of LDS
constexpr uint32_t FAPEA_STEP = 2 * BLOCK;        // slots examined per staging step of the points: two a lane
constexpr uint32_t FAPEA_FRAME_PASS = 256;        // frames staged per candidate pass of k_fape_atoms_grad_points, at most: 25 KiB
constexpr uint32_t FAPEA_FRAME_STEP = BLOCK;      // items examined per staging step of the frames: one a lane, 32 rows
constexpr uint32_t FAPEA_MAX_TILE_ROWS = 128;
constexpr uint32_t FAPEA_TILE_ITEMS = FAPEA_MAX_TILE_ROWS * FAPEA_GROUPS;
static_assert(FAPEA_STEP <= FAPEA_PASS && FAPEA_PASS % BLOCK == 0 && FAPEA_FRAME_STEP <= FAPEA_FRAME_PASS && FAPEA_TILE_ITEMS < 65536, "fcz_fape_atoms.h");

// rows per query tile of the two frame sweeps: backbone4 has two groups a row, the other layouts 3.7 on average
__host__ __device__ __forceinline__ uint32_t fapea_tile_rows(uint32_t A) { return A == 4u ? 128u : 64u; }
// the rows a chain may have: a frame's points, at most A * rows, must fit int32
inline uint32_t fapea_max_rows(uint32_t A) { return 0x7FFFFFFFu / A < FAPE_MAX_ROWS ? 0x7FFFFFFFu / A : FAPE_MAX_ROWS; }

// the renaming: partner [min(aatype, 20)][slot] with rows of A bytes (lddt_atoms' table), alt [type] = the groups, a bit each, whose
// true frame has a 180-degree alternative (fcz_frame_ambiguous)
struct fapea_table { lddta_table swap; uint8_t alt[LDDTA_TYPES]; };

struct fapea_args {
    const float* rot_true; const float* trans_true; const uint8_t* fmask_true;   // [rows][8][3][3], [rows][8][3], [rows][8]
    const float* pos_true; const uint8_t* mask_true;                             // [rows][A][3], [rows][A]
    const uint8_t* aatype; const uint8_t* swapped;                               // [rows]; each may be NULL (swapped only with aatype)
    const float* rot_pred; const float* trans_pred; const uint8_t* fmask_pred;   // fmask_pred may be NULL: every frame present
    const float* pos_pred; const uint8_t* mask_pred;                             // mask_pred may be NULL: every slot present
    const uint32_t* bound;                  // padded: length [n] or NULL; packed: row_off [n + 1]
    uint32_t n, L;                          // padded: rows per entry; packed: L = R, the rows of the arrays
    uint32_t A;
    float clamp, eps;
    float* sum; int32_t* points;            // [rows][8]
};

struct fapea_grad_args {
    const float* rot_true; const float* trans_true; const uint8_t* fmask_true;
    const float* pos_true; const uint8_t* mask_true;
    const uint8_t* aatype; const uint8_t* swapped;
    const float* rot_pred; const float* trans_pred; const uint8_t* fmask_pred;
    const float* pos_pred; const uint8_t* mask_pred;
    const uint32_t* bound;
    uint32_t n, L;
    uint32_t A;
    float clamp, eps;
    const float* weight;                    // [rows][8]: the upstream gradient of sum
    float* grad_rot; float* grad_trans; float* grad_pos;   // [rows][8][3][3], [rows][8][3], [rows][A][3]
};

// x / 8, the divider of a staging over the eight groups of a row
struct fapea_div_groups { __device__ __forceinline__ uint32_t operator()(uint32_t x, uint32_t) const { return x >> 3; } };

// array row r (a row inside its chain): is it read under its other naming, and its clamped type
template <class Args>
__device__ __forceinline__ bool fapea_swapped(const Args& g, uint64_t r, uint32_t* ty) {
    if (!g.swapped || !g.aatype || g.swapped[r] == 0) return false;
    const uint32_t aa = g.aatype[r];
    *ty = aa > 20u ? 20u : aa;
    return true;
}

// group grp of array row r (a row inside its chain) -> true when it is a FRAME; t is the truth's frame as the sweep reads it
template <class Args>
__device__ __forceinline__ bool fapea_frame(const Args& g, const fapea_table& tab, uint64_t r, uint32_t grp, fape_frame* p, fape_frame* t) {
    if (g.A == 4u && grp != 0u && grp != 3u) return false;            // backbone4 holds the atoms of groups 0 and 3 alone
    if (!fape_frame_row(g, r * FAPEA_GROUPS + grp, p, t)) return false;
    uint32_t ty;
    if (fapea_swapped(g, r, &ty) && ((tab.alt[ty] >> grp) & 1u)) {    // rot @ diag(1, -1, -1): exact
#pragma unroll
        for (uint32_t a = 0; a < 3; a++) { t->r[3u * a + 1u] = -t->r[3u * a + 1u]; t->r[3u * a + 2u] = -t->r[3u * a + 2u]; }
    }
    return true;
}

// slot a of array row r (a row inside its chain) -> true when it is a POINT; t the truth under the row's naming, p the prediction
template <class Args>
__device__ __forceinline__ bool fapea_point(const Args& g, const fapea_table& tab, uint64_t r, uint32_t a, float* t, float* p) {
    uint32_t ty, s = a;
    if (fapea_swapped(g, r, &ty)) s = tab.swap.partner[ty * g.A + a];
    return chain_site2(g.pos_true, g.mask_true, r * g.A + s, g.pos_pred, g.mask_pred, r * g.A + a, t, p);
}

// row r of the arrays holds nothing
__device__ __forceinline__ void chain_empty_row(const fapea_args& g, uint64_t r) {
    for (uint32_t k = 0; k < FAPEA_GROUPS; k++) { g.sum[r * FAPEA_GROUPS + k] = 0.0f; g.points[r * FAPEA_GROUPS + k] = 0; }
}
__device__ __forceinline__ void chain_empty_row(const fapea_grad_args& g, uint64_t r) {
    for (uint32_t k = 0; k < FAPEA_GROUPS * 9u; k++) g.grad_rot[r * (FAPEA_GROUPS * 9u) + k] = 0.0f;
    for (uint32_t k = 0; k < FAPEA_GROUPS * 3u; k++) g.grad_trans[r * (FAPEA_GROUPS * 3u) + k] = 0.0f;
    for (uint32_t k = 0; k < g.A * 3u; k++) g.grad_pos[r * g.A * 3u + k] = 0.0f;
}

// The tile's frames into q_it as item numbers of the tile (row of the tile * 8 + group), in any order; none(o) for every item o of the
// arrays that the tile writes and that is no frame. All BLOCK threads; the caller has cleared *s_nq behind a barrier and puts one
// behind the call.
template <class Args, class None>
__device__ __forceinline__ void fapea_tile_frames(const Args& g, const fapea_table& tab, uint32_t TR, uint64_t row0, uint64_t q0, uint32_t len, uint32_t rows,
                                                  uint16_t* q_it, uint32_t* s_nq, None none) {
    for (uint32_t x = threadIdx.x; x < TR * FAPEA_GROUPS; x += BLOCK) {
        const uint64_t q = q0 + (x >> 3);
        if (q >= rows) continue;
        fape_frame p, t;
        if (q < len && fapea_frame(g, tab, row0 + q, x & 7u, &p, &t)) q_it[atomicAdd(s_nq, 1u)] = (uint16_t)x;   // (< TR * 8: one slot per item)
        else none((row0 + q) * FAPEA_GROUPS + (x & 7u));
    }
}

// one pass of the chain's points from row *r0, compacted in ascending (row, slot) -> the staged count
template <class Args>
__device__ __forceinline__ uint32_t fapea_stage_points(const Args& g, const fapea_table& tab, uint64_t row0, uint32_t len, uint32_t* r0, uint32_t* s_wave,
                                                       float* s_px, float* s_py, float* s_pz, float* s_tx, float* s_ty, float* s_tz) {
    float t2[FAPEA_STEP / BLOCK][3], p2[FAPEA_STEP / BLOCK][3];
    return chain_stage_slots_ordered<FAPEA_PASS, FAPEA_STEP>(
        s_wave, g.A, len, r0,
        [&](uint32_t r, uint32_t a, uint32_t h) __attribute__((always_inline)) { return fapea_point(g, tab, row0 + r, a, t2[h], p2[h]); },
        [&](uint32_t h, uint32_t i) __attribute__((always_inline)) {
            s_px[i] = p2[h][0]; s_py[i] = p2[h][1]; s_pz[i] = p2[h][2]; s_tx[i] = t2[h][0]; s_ty[i] = t2[h][1]; s_tz[i] = t2[h][2];
        });
}

template <bool PACKED>
__global__ __launch_bounds__(BLOCK) void k_fape_atoms(fapea_args g, const fapea_table tab, const uint64_t* __restrict__ tile_off, uint32_t tiles_per_entry,
                                                      uint64_t n_tiles_padded) {
    __shared__ float s_px[FAPEA_PASS], s_py[FAPEA_PASS], s_pz[FAPEA_PASS], s_tx[FAPEA_PASS], s_ty[FAPEA_PASS], s_tz[FAPEA_PASS];
    __shared__ uint16_t q_it[FAPEA_TILE_ITEMS];
    __shared__ uint32_t s_wave[FAPEA_STEP / 64], s_nq;
    const uint32_t tid = threadIdx.x;
    const uint32_t TR = fapea_tile_rows(g.A);
    const uint64_t n_tiles = chain_tile_count<PACKED>(tile_off, g.n, n_tiles_padded);
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const chain_tile<PACKED> ct(tile_off, g.n, tiles_per_entry, g.bound, g.L, tile, TR);
        if (tid == 0) s_nq = 0;
        __syncthreads();
        fapea_tile_frames(g, tab, TR, ct.row0, ct.q0, ct.len, ct.rows, q_it, &s_nq, [&](uint64_t o) __attribute__((always_inline)) { g.sum[o] = 0.0f; g.points[o] = 0; });
        __syncthreads();
        const uint32_t nq = s_nq;
        for (uint32_t base = 0; base < nq; base += BLOCK) {
            const uint32_t qi = base + tid;
            const bool have = qi < nq;
            const bool wave_has = base + (tid & ~63u) < nq;           // wave-uniform: some lane of this wavefront holds a frame
            const uint32_t it = have ? q_it[qi] : 0u;
            const uint64_t ri = ct.row0 + ct.q0 + (it >> 3);          // the frame's row of the arrays
            fape_frame fp = {}, ft = {};
            if (have) (void)fapea_frame(g, tab, ri, it & 7u, &fp, &ft);
            uint32_t points = 0;
            float sum = 0.0f;                                         // lives across the passes: they ascend
            for (uint32_t r0 = 0; r0 < ct.len;) {
                const uint32_t count = fapea_stage_points(g, tab, ct.row0, ct.len, &r0, s_wave, s_px, s_py, s_pz, s_tx, s_ty, s_tz);
                if (wave_has) {
                    for (uint32_t c = 0; c < count; c++) {
                        const float x[3] = {s_px[c], s_py[c], s_pz[c]};   // broadcast reads
                        const float y[3] = {s_tx[c], s_ty[c], s_tz[c]};
                        float u[3], e[3];
                        const float d = fape_term(fp, ft, x, y, g.eps, u, e);
                        sum = isfinite(d) ? __fadd_rn(sum, d < g.clamp ? d : g.clamp) : sum;
                    }
                }
                points += count;
                __syncthreads();                                      // the next pass (or round, or tile) rewrites the staging
            }
            if (have) {
                const uint64_t o = ri * FAPEA_GROUPS + (it & 7u);
                g.sum[o] = sum; g.points[o] = (int32_t)points;
            }
        }
        __syncthreads();                                              // the next tile rewrites the frame list and its counter
    }
}

template <bool PACKED>
__global__ __launch_bounds__(BLOCK) void k_fape_atoms_grad_frames(fapea_grad_args g, const fapea_table tab, const uint64_t* __restrict__ tile_off,
                                                                  uint32_t tiles_per_entry, uint64_t n_tiles_padded) {
    __shared__ float s_px[FAPEA_PASS], s_py[FAPEA_PASS], s_pz[FAPEA_PASS], s_tx[FAPEA_PASS], s_ty[FAPEA_PASS], s_tz[FAPEA_PASS];
    __shared__ uint16_t q_it[FAPEA_TILE_ITEMS];
    __shared__ uint32_t s_wave[FAPEA_STEP / 64], s_nq;
    const uint32_t tid = threadIdx.x;
    const uint32_t TR = fapea_tile_rows(g.A);
    const uint64_t n_tiles = chain_tile_count<PACKED>(tile_off, g.n, n_tiles_padded);
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const chain_tile<PACKED> ct(tile_off, g.n, tiles_per_entry, g.bound, g.L, tile, TR);
        if (tid == 0) s_nq = 0;
        __syncthreads();
        fapea_tile_frames(g, tab, TR, ct.row0, ct.q0, ct.len, ct.rows, q_it, &s_nq, [&](uint64_t o) __attribute__((always_inline)) {
#pragma unroll
            for (uint32_t k = 0; k < 9; k++) g.grad_rot[o * 9u + k] = 0.0f;
#pragma unroll
            for (uint32_t k = 0; k < 3; k++) g.grad_trans[o * 3u + k] = 0.0f;
        });
        __syncthreads();
        const uint32_t nq = s_nq;
        for (uint32_t base = 0; base < nq; base += BLOCK) {
            const uint32_t qi = base + tid;
            const bool have = qi < nq;
            const bool wave_has = base + (tid & ~63u) < nq;
            const uint32_t it = have ? q_it[qi] : 0u;
            const uint64_t ri = ct.row0 + ct.q0 + (it >> 3);
            const uint64_t o = ri * FAPEA_GROUPS + (it & 7u);
            fape_frame fp = {}, ft = {};
            if (have) (void)fapea_frame(g, tab, ri, it & 7u, &fp, &ft);
            const float w = have ? g.weight[o] : 0.0f;
            float sh[3] = {0.0f, 0.0f, 0.0f};                         // sum_j h
            float m[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};   // sum_j u_a h_k at 3 a + k
            for (uint32_t r0 = 0; r0 < ct.len;) {
                const uint32_t count = fapea_stage_points(g, tab, ct.row0, ct.len, &r0, s_wave, s_px, s_py, s_pz, s_tx, s_ty, s_tz);
                if (wave_has) {
                    for (uint32_t c = 0; c < count; c++) {
                        const float x[3] = {s_px[c], s_py[c], s_pz[c]};
                        const float y[3] = {s_tx[c], s_ty[c], s_tz[c]};
                        float u[3], e[3], h[3];
                        const float d = fape_term(fp, ft, x, y, g.eps, u, e);
                        const bool add = fape_h(d, g.clamp, e, h);
#pragma unroll
                        for (uint32_t k = 0; k < 3; k++) sh[k] = add ? __fadd_rn(sh[k], h[k]) : sh[k];
#pragma unroll
                        for (uint32_t a = 0; a < 3; a++)
#pragma unroll
                            for (uint32_t k = 0; k < 3; k++) m[3u * a + k] = add ? __fadd_rn(m[3u * a + k], __fmul_rn(u[a], h[k])) : m[3u * a + k];
                    }
                }
                __syncthreads();
            }
            if (have) {
                float* orot = g.grad_rot + o * 9u;
                float* otr = g.grad_trans + o * 3u;
#pragma unroll
                for (uint32_t k = 0; k < 9; k++) orot[k] = __fmul_rn(w, m[k]);
#pragma unroll
                for (uint32_t a = 0; a < 3; a++) {                    // -w (R sum h)_a
                    const float v = __fadd_rn(__fadd_rn(__fmul_rn(fp.r[3u * a], sh[0]), __fmul_rn(fp.r[3u * a + 1u], sh[1])), __fmul_rn(fp.r[3u * a + 2u], sh[2]));
                    otr[a] = -__fmul_rn(w, v);
                }
            }
        }
        __syncthreads();
    }
}

template <bool PACKED>
__global__ __launch_bounds__(BLOCK) void k_fape_atoms_grad_points(fapea_grad_args g, const fapea_table tab, const uint64_t* __restrict__ tile_off,
                                                                  uint32_t tiles_per_entry, uint64_t n_tiles_padded) {
    __shared__ float s_f[FAPE_FRAME_FLOATS][FAPEA_FRAME_PASS];        // rot_pred 0 .. 8, trans_pred 9 .. 11, rot_true 12 .. 20, trans_true 21 .. 23, w 24
    __shared__ uint16_t q_at[LDDTA_TILE_SLOTS];                       // the point's slot of the tile, row of the tile * A + a
    __shared__ uint32_t s_wave[FAPEA_FRAME_STEP / 64], s_nq;
    const uint32_t tid = threadIdx.x;
    const uint32_t A = g.A;
    const uint32_t TR = lddta_tile_rows(A, false);
    const uint64_t n_tiles = chain_tile_count<PACKED>(tile_off, g.n, n_tiles_padded);
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const chain_tile<PACKED> ct(tile_off, g.n, tiles_per_entry, g.bound, g.L, tile, TR);
        if (tid == 0) s_nq = 0;
        __syncthreads();
        // ---- the tile's points, compacted in any order; every slot that is none is written 0 here, every point at the end of its round ----
        chain_tile_slots(TR, A, ct.q0, [&](uint32_t x, uint32_t, uint32_t a, uint64_t q) __attribute__((always_inline)) {
            if (q < ct.rows) {
                float t[3], p[3];
                if (q < ct.len && fapea_point(g, tab, ct.row0 + q, a, t, p)) {
                    q_at[atomicAdd(&s_nq, 1u)] = (uint16_t)x;         // (< LDDTA_TILE_SLOTS: one slot per slot of the tile)
                } else {
                    float* o = g.grad_pos + ((ct.row0 + q) * A + a) * 3u;
                    o[0] = 0.0f; o[1] = 0.0f; o[2] = 0.0f;
                }
            }
        });
        __syncthreads();
        const uint32_t nq = s_nq;
        for (uint32_t base = 0; base < nq; base += BLOCK) {
            const uint32_t qi = base + tid;
            const bool have = qi < nq;
            const bool wave_has = base + (tid & ~63u) < nq;
            const uint32_t at = have ? q_at[qi] : 0u;
            const uint32_t rr = chain_div_a(at, A), a = at - rr * A;
            const uint64_t ri = ct.row0 + ct.q0 + rr;                 // the point's row of the arrays
            float y[3] = {0.0f, 0.0f, 0.0f}, x[3] = {0.0f, 0.0f, 0.0f};
            if (have) (void)fapea_point(g, tab, ri, a, y, x);
            float gp[3] = {0.0f, 0.0f, 0.0f};                         // live across the passes: they ascend
            for (uint32_t r0 = 0; r0 < ct.len;) {
                fape_frame p2[FAPEA_FRAME_STEP / BLOCK], t2[FAPEA_FRAME_STEP / BLOCK];
                uint64_t o2[FAPEA_FRAME_STEP / BLOCK];
                const uint32_t count = chain_stage_slots_ordered<FAPEA_FRAME_PASS, FAPEA_FRAME_STEP>(
                    s_wave, FAPEA_GROUPS, ct.len, &r0,
                    [&](uint32_t r, uint32_t grp, uint32_t h) __attribute__((always_inline)) {
                        o2[h] = (ct.row0 + r) * FAPEA_GROUPS + grp;
                        return fapea_frame(g, tab, ct.row0 + r, grp, &p2[h], &t2[h]);
                    },
                    [&](uint32_t h, uint32_t i) __attribute__((always_inline)) {
#pragma unroll
                        for (uint32_t k = 0; k < 9; k++) { s_f[k][i] = p2[h].r[k]; s_f[12u + k][i] = t2[h].r[k]; }
#pragma unroll
                        for (uint32_t k = 0; k < 3; k++) { s_f[9u + k][i] = p2[h].t[k]; s_f[21u + k][i] = t2[h].t[k]; }
                        s_f[24][i] = g.weight[o2[h]];
                    },
                    fapea_div_groups{});
                if (wave_has) {
                    for (uint32_t c = 0; c < count; c++) {
                        fape_frame p, t;
#pragma unroll
                        for (uint32_t k = 0; k < 9; k++) { p.r[k] = s_f[k][c]; t.r[k] = s_f[12u + k][c]; }
#pragma unroll
                        for (uint32_t k = 0; k < 3; k++) { p.t[k] = s_f[9u + k][c]; t.t[k] = s_f[21u + k][c]; }
                        const float w = s_f[24][c];
                        float u[3], e[3], h[3];
                        const float d = fape_term(p, t, x, y, g.eps, u, e);
                        const bool add = fape_h(d, g.clamp, e, h);
#pragma unroll
                        for (uint32_t k = 0; k < 3; k++) {            // + w (R h)_k
                            const float v = __fadd_rn(__fadd_rn(__fmul_rn(p.r[3u * k], h[0]), __fmul_rn(p.r[3u * k + 1u], h[1])), __fmul_rn(p.r[3u * k + 2u], h[2]));
                            gp[k] = add ? __fadd_rn(gp[k], __fmul_rn(w, v)) : gp[k];
                        }
                    }
                }
                __syncthreads();                                      // the next pass (or round, or tile) rewrites the staging
            }
            if (have) {
                float* o = g.grad_pos + (ri * A + a) * 3u;
                o[0] = gp[0]; o[1] = gp[1]; o[2] = gp[2];
            }
        }
        __syncthreads();                                              // the next tile rewrites the point list and its counter
    }
}

}  // namespace fcz
