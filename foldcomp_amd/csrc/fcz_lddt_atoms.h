// fcz_lddt_atoms.h -- two dense tensor batches of one shape (true, pred) -> the ALL-ATOM lDDT of every residue, with the chemically
// equivalent side-chain namings of the truth resolved first: swapped [rows] uint8, score [rows] float32, pairs / hits [rows] int32 and,
// when wanted, atom_pairs / atom_hits [rows][A] int32, on the device. The reference has no such output (Foldcomp::decompress,
// src/foldcomp.cpp:779, ends at a flat vector<AtomCoordinate>); the calls stand beside fcz_lddt_dev and fcz_violations_dev and read what
// fcz_dense_dev / fcz_dense_packed_dev write, or any tensors of those shapes (include/fcz_hip.h, fcz_lddt_atoms_dev).
//
// The contract (include/fcz_hip.h): all arithmetic is float32, every operation rounded, no FMA; d2 = (dx*dx + dy*dy) + dz*dz (fcz_knn's
// d2), d its correctly rounded root, d_true < cutoff decided as d2 < c2 (lddt_c2). A slot is PRESENT when both masks are set (a NULL
// mask_pred is all set) and its six coordinates are finite. partner(a) = swap_table[min(aatype, 20)][a] is the slot's other naming
// (a itself where it has none). 1. A row with a partnered slot is decided when every partnered slot of it is present: its partnered
// slots are scored against the ANCHORS, the present slots without a partner of the chain's other rows, once with the truth as it is
// named (P_0, H_0) and once with the truth read at partner(a) (P_1, H_1); swapped = (u64)H_1 * P_0 > (u64)H_0 * P_1. 2. The renamed
// truth reads pos_true and mask_true of a swapped row at partner(a); an ATOM is a present slot of it; atoms of DIFFERENT rows of a
// chain are pairs when d_true' < cutoff, a pair scores a hit per threshold |d_true' - d_pred| lies under. Every counter is an
// integer, so no order of evaluation changes a result.
//
//   k_lddt_atoms<PACKED, DECIDE>
//       One kernel, two launches in stream order: DECIDE = true writes swapped for every row, DECIDE = false reads it and writes the
//       scores. A chain's rows are all decided before any of them is scored because the launches follow each other on the stream.
//       Both are persistent blocks over QUERY TILES of whole rows of one chain (tiles are counted in rows by k_chain_tiles and the scan
//       of fcz_chains.h, each launch with the tile count of its own):
//         score    20 rows in atom37, 18 in atom14, 64 in backbone4 (fcz_violations.h's tiles: 156 atoms a tile at 7.8 heavy atoms a
//                  residue, 61 % of a round's lanes); the query atoms are all atoms of the tile.
//         decide   64 rows in every layout; the query atoms are the partnered slots of the tile's decidable rows. About one residue in
//                  seven is ASP, GLU, PHE or TYR with four such slots, so 64 rows give about 38 query atoms: most of one wavefront.
//                  With 20 rows the decide launch would sweep every chain as often as the score launch for a twelfth of its lanes.
//       The tile's query atoms are COMPACTED into LDS as their slot numbers (uint16: row of the tile * A + a) and taken in ROUNDS of
//       BLOCK = 256, A LANE PER QUERY ATOM. A lane fetches its coordinates from HBM (L2: the compaction just read them) into VGPRs:
//       the truth (decide: under both namings), the prediction, and its two (decide: four) counters. Keeping only the slot numbers in
//       LDS is what leaves room for the candidates.
//       The chain's candidates (score: its atoms under the renamed truth; decide: its anchors) are staged COMPACTED in passes of at most
//       LDDTA_PASS = 1536 as SoA true x / y / z, pred x / y / z and the chain row, 28 bytes each, in steps of two slots a lane
//       (chain_stage_slots, fcz_chains.h, as k_violations stages them; slots are handed out by an LDS counter: the order inside a
//       pass is free, see above). Every lane walks the pass; all 64 lanes of a wavefront read the SAME candidate (broadcast reads,
//       no bank conflict), compute the true d2 (decide: two of them) and compare with c2. Only when some lane of the wavefront has a pair (__any) does the wavefront pay for the pred
//       d2, the roots and the four compares, as k_lddt does. A wavefront without a query atom in the round skips the sweep
//       (wave-uniform) and keeps the barriers; a tile without a query atom (decide: most tiles of a batch without aatype, all of them)
//       stages nothing.
//       The tile's epilogue: a lane adds its counters to its row's by integer LDS atomics (score: and writes its atom's two counts
//       when they are wanted; the slots that hold no atom were written 0 by the compaction, so every element is written once); then
//       a lane per row writes swapped, or score / pairs / hits.
//       LDS: 1536 * 28 = 43008 bytes of candidates, 64 * 37 * 2 = 4736 of query slots, 64 * 16 = 1024 of per-row counters, 256 of row
//       flags, 8 of counters: 49032 bytes a block, so THREE blocks (12 wavefronts, three per SIMD) share a CU's 160 KiB and a
//       wavefront may hold 170 VGPRs. `make asm` prints the VGPRs: score padded 54, packed 54; decide padded 58, packed 56; no scratch
//       (LDS is the limit; a pass of 1024 candidates would buy the fourth block and cost a 350-residue chain of 2730 atoms a third pass).
//       NOBODY HAS MEASURED tile rows or pass size: tools/lddt_atoms_rate.py reports the rate of the constants as they stand.
//       HBM sees the inputs, one byte and twelve bytes a row, and eight bytes a slot when the per-atom counts are wanted: no rows x rows
//       and no atoms x atoms array.
//   k_chain_fill<lddta_args>   (fcz_chains.h) packed form only, in front of the sweeps: 0 (chain_empty_row) into every row that no
//                       chain is seen to cover (chain_covers: a covered row it misses is rewritten by the sweeps behind it).
//
// Every index that scales with rows * A is 64-bit. A chain's range is clamped to the R rows that exist and a range that runs
// backwards is empty (chain_range), so no read leaves the inputs whatever row_off holds; aatype is clamped to 20 before the table is
// read and the ABI admits only tables whose entries are < A. A row's hits <= 4 * A * (A * rows of a chain) fit int32 because the
// ABI refuses more than lddta_max_rows(A) rows per chain.
#pragma once
#include "fcz_lddt.h"

namespace fcz {

constexpr uint32_t LDDTA_PASS = 1536;       // candidates staged per pass, at most
constexpr uint32_t LDDTA_STEP = 2 * BLOCK;  // slots examined per staging step: two a lane
constexpr uint32_t LDDTA_DECIDE_ROWS = 64;  // rows per query tile of the decide launch
constexpr uint32_t LDDTA_MAX_TILE_ROWS = 64;
constexpr uint32_t LDDTA_TILE_SLOTS = LDDTA_MAX_TILE_ROWS * DN_MAX_WIDTH;   // >= tile rows * A of either launch
constexpr uint32_t LDDTA_TYPES = 21;

__host__ __device__ __forceinline__ uint32_t lddta_tile_rows(uint32_t A, bool decide) {
    return decide ? LDDTA_DECIDE_ROWS : A == 37u ? 20u : A == 14u ? 18u : 64u;
}
// the rows a chain may have: a row's hits, at most 4 * A * (A * rows), must fit int32
inline uint32_t lddta_max_rows(uint32_t A) { return 0x7FFFFFFFu / (4u * A * A); }
static_assert(LDDTA_PASS % LDDTA_STEP == 0 && LDDTA_STEP <= LDDTA_PASS && LDDTA_TILE_SLOTS < 65536 && LDDTA_MAX_TILE_ROWS <= BLOCK &&
              LDDTA_DECIDE_ROWS <= LDDTA_MAX_TILE_ROWS && DN_MAX_WIDTH == 37, "fcz_lddt_atoms.h");

struct lddta_table { uint8_t partner[LDDTA_TYPES * DN_MAX_WIDTH]; };   // [min(aatype, 20)][slot] with rows of A bytes, every entry < A

struct lddta_args {
    const float* pos_true; const uint8_t* mask_true;
    const float* pos_pred; const uint8_t* mask_pred;   // mask_pred may be NULL: every slot present
    const uint8_t* aatype;                  // may be NULL: no slot has a partner
    const uint32_t* bound;                  // padded: length [n] or NULL; packed: row_off [n + 1]
    uint32_t n, L;                          // padded: rows per entry; packed: L = R, the rows of the arrays
    uint32_t A;
    float c2;                               // d_true < cutoff <=> d2_true < c2 (lddt_c2)
    float t0, t1, t2, t3;
    float* score; int32_t* pairs; int32_t* hits; uint8_t* swapped;
    int32_t* atom_pairs; int32_t* atom_hits;   // [rows][A], each may be NULL: not wanted
};

// the other naming of slot a of array row r (a itself where it has none, and everywhere without aatype)
__device__ __forceinline__ uint32_t lddta_partner(const lddta_args& g, const lddta_table& tab, uint64_t r, uint32_t a) {
    if (!g.aatype) return a;
    const uint32_t aa = g.aatype[r];
    return tab.partner[(aa > 20u ? 20u : aa) * g.A + a];
}

// slot `at` of the truth and slot a of the prediction of array row r -> true when the slot is present (both masks set, six finite values)
__device__ __forceinline__ bool lddta_present(const lddta_args& g, uint64_t r, uint32_t at, uint32_t a, float* t, float* p) {
    return chain_site2(g.pos_true, g.mask_true, r * g.A + at, g.pos_pred, g.mask_pred, r * g.A + a, t, p);
}

// A candidate of the sweep at slot a of array row r (a row inside its chain). DECIDE: an anchor, a present slot without a partner.
// Score: an atom, a present slot of the renamed truth (read at the partner where the row is swapped).
template <bool DECIDE>
__device__ __forceinline__ bool lddta_candidate(const lddta_args& g, const lddta_table& tab, uint64_t r, uint32_t a, float* t, float* p) {
    const uint32_t pa = lddta_partner(g, tab, r, a);
    if constexpr (DECIDE) return pa == a && lddta_present(g, r, a, a, t, p);
    else return lddta_present(g, r, pa != a && g.swapped[r] ? pa : a, a, t, p);
}

// row r of the arrays holds nothing
__device__ __forceinline__ void chain_empty_row(const lddta_args& g, uint64_t r) {
    g.score[r] = 0.0f; g.pairs[r] = 0; g.hits[r] = 0; g.swapped[r] = 0;
    for (uint32_t a = 0; a < g.A; a++) {
        if (g.atom_pairs) g.atom_pairs[r * g.A + a] = 0;
        if (g.atom_hits) g.atom_hits[r * g.A + a] = 0;
    }
}

template <bool PACKED, bool DECIDE>
__global__ __launch_bounds__(BLOCK) void k_lddt_atoms(lddta_args g, const lddta_table tab, const uint64_t* __restrict__ tile_off, uint32_t tiles_per_entry,
                                                      uint64_t n_tiles_padded) {
    __shared__ float s_tx[LDDTA_PASS], s_ty[LDDTA_PASS], s_tz[LDDTA_PASS], s_px[LDDTA_PASS], s_py[LDDTA_PASS], s_pz[LDDTA_PASS];
    __shared__ uint32_t s_row[LDDTA_PASS];
    __shared__ uint16_t q_at[LDDTA_TILE_SLOTS];                       // the query atom's slot of the tile, row of the tile * A + a
    __shared__ uint32_t r_cnt[LDDTA_MAX_TILE_ROWS][4];                // score: pairs, hits; decide: P_0, H_0, P_1, H_1
    __shared__ uint32_t r_flag[LDDTA_MAX_TILE_ROWS];                  // decide: bit 0 a partnered slot, bit 1 one of them is not present
    __shared__ uint32_t s_count, s_nq;
    const uint32_t tid = threadIdx.x;
    const uint32_t A = g.A;
    const uint32_t TR = lddta_tile_rows(A, DECIDE);
    const uint64_t n_tiles = chain_tile_count<PACKED>(tile_off, g.n, n_tiles_padded);
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const chain_tile<PACKED> ct(tile_off, g.n, tiles_per_entry, g.bound, g.L, tile, TR);
        if (tid == 0) s_nq = 0;
        if (tid < TR) { r_cnt[tid][0] = 0; r_cnt[tid][1] = 0; r_cnt[tid][2] = 0; r_cnt[tid][3] = 0; r_flag[tid] = 0; }
        __syncthreads();
        // ---- the tile's query atoms, compacted ----
        if constexpr (DECIDE) {
            if (g.aatype) {                                           // (uniform; without aatype no row is ambiguous)
                chain_tile_slots(TR, A, ct.q0, [&](uint32_t, uint32_t rr, uint32_t a, uint64_t q) __attribute__((always_inline)) {
                    if (q < ct.len && lddta_partner(g, tab, ct.row0 + q, a) != a) {
                        float c[3], p[3];
                        atomicOr(&r_flag[rr], lddta_present(g, ct.row0 + q, a, a, c, p) ? 1u : 3u);
                    }
                });
            }
            __syncthreads();
            if (g.aatype) {
                chain_tile_slots(TR, A, ct.q0, [&](uint32_t x, uint32_t rr, uint32_t a, uint64_t q) __attribute__((always_inline)) {
                    if (q < ct.len && r_flag[rr] == 1u && lddta_partner(g, tab, ct.row0 + q, a) != a) q_at[atomicAdd(&s_nq, 1u)] = (uint16_t)x;
                });
            }
        } else {
            // every slot that holds no atom gets its two counts here, every atom at the end of its round
            chain_tile_slots(TR, A, ct.q0, [&](uint32_t x, uint32_t, uint32_t a, uint64_t q) __attribute__((always_inline)) {
                if (q < ct.rows) {
                    float c[3], p[3];
                    if (q < ct.len && lddta_candidate<false>(g, tab, ct.row0 + q, a, c, p)) {
                        q_at[atomicAdd(&s_nq, 1u)] = (uint16_t)x;     // (< LDDTA_TILE_SLOTS: one slot per slot of the tile)
                    } else {
                        if (g.atom_pairs) g.atom_pairs[(ct.row0 + q) * A + a] = 0;
                        if (g.atom_hits) g.atom_hits[(ct.row0 + q) * A + a] = 0;
                    }
                }
            });
        }
        __syncthreads();
        const uint32_t nq = s_nq;
        for (uint32_t base = 0; base < nq; base += BLOCK) {
            const uint32_t qi = base + tid;
            const bool have = qi < nq;
            const bool wave_has = base + (tid & ~63u) < nq;           // wave-uniform: some lane of this wavefront holds a query atom
            const uint32_t at = have ? q_at[qi] : 0u;
            const uint32_t rr = chain_div_a(at, A), a = at - rr * A;
            const uint32_t ri = (uint32_t)ct.q0 + rr;                 // the query atom's row of the chain
            // the truth as it is named (score: as it is renamed), the truth under the other naming (decide only), the prediction
            float qt[3] = {0.0f, 0.0f, 0.0f}, qu[3] = {0.0f, 0.0f, 0.0f}, qp[3] = {0.0f, 0.0f, 0.0f};
            if (have) {
                const uint64_t r = ct.row0 + ri;
                const uint32_t pa = lddta_partner(g, tab, r, a);
                if constexpr (DECIDE) {
                    (void)lddta_present(g, r, a, a, qt, qp);
                    const float* fu = g.pos_true + (r * A + pa) * 3u;
                    qu[0] = fu[0]; qu[1] = fu[1]; qu[2] = fu[2];
                } else {
                    (void)lddta_present(g, r, pa != a && g.swapped[r] ? pa : a, a, qt, qp);
                }
            }
            uint32_t n0 = 0, h0 = 0, n1 = 0, h1 = 0;                  // pairs and hits (decide: of naming 0, and of naming 1)
            // ---- the chain's candidates in passes ----
            for (uint32_t r0 = 0; r0 < ct.len;) {
                const uint32_t count = chain_stage_slots<LDDTA_PASS, LDDTA_STEP>(&s_count, A, ct.len, &r0, [&](uint32_t r, uint32_t a, chain_slots slots) __attribute__((always_inline)) {
                    float c[3], p[3];
                    if (lddta_candidate<DECIDE>(g, tab, ct.row0 + r, a, c, p)) {
                        const uint32_t i = slots.next();
                        s_tx[i] = c[0]; s_ty[i] = c[1]; s_tz[i] = c[2]; s_px[i] = p[0]; s_py[i] = p[1]; s_pz[i] = p[2]; s_row[i] = r;
                    }
                });
                // ---- the sweep: every lane meets every staged candidate, all lanes of a wavefront the same one at a time ----
                if (wave_has) {
                    for (uint32_t j = 0; j < count; j++) {
                        const float cx = s_tx[j], cy = s_ty[j], cz = s_tz[j];
                        const bool other = have && s_row[j] != ri;
                        const float d0 = chain_d2(cx, cy, cz, qt[0], qt[1], qt[2]);
                        const bool pair0 = other && d0 < g.c2;        // (a d2 of +inf or NaN is no pair: c2 <= +inf)
                        if constexpr (DECIDE) {
                            const float d1 = chain_d2(cx, cy, cz, qu[0], qu[1], qu[2]);
                            const bool pair1 = other && d1 < g.c2;
                            if (__any(pair0 || pair1)) {
                                const float sp = f32_sqrt_rn(chain_d2(s_px[j], s_py[j], s_pz[j], qp[0], qp[1], qp[2]));
                                const uint32_t k0 = lddt_hits(g, d0, sp), k1 = lddt_hits(g, d1, sp);
                                n0 += pair0 ? 1u : 0u; h0 += pair0 ? k0 : 0u;
                                n1 += pair1 ? 1u : 0u; h1 += pair1 ? k1 : 0u;
                            }
                        } else {
                            if (__any(pair0)) {
                                const float sp = f32_sqrt_rn(chain_d2(s_px[j], s_py[j], s_pz[j], qp[0], qp[1], qp[2]));
                                const uint32_t k0 = lddt_hits(g, d0, sp);
                                n0 += pair0 ? 1u : 0u; h0 += pair0 ? k0 : 0u;
                            }
                        }
                    }
                }
                __syncthreads();                                      // the next pass (or round, or tile) rewrites the staging
            }
            // ---- the round's atoms ----
            if (have) {
                if (n0) { atomicAdd(&r_cnt[rr][0], n0); atomicAdd(&r_cnt[rr][1], h0); }
                if constexpr (DECIDE) {
                    if (n1) { atomicAdd(&r_cnt[rr][2], n1); atomicAdd(&r_cnt[rr][3], h1); }
                } else {
                    if (g.atom_pairs) g.atom_pairs[(ct.row0 + ri) * A + a] = (int32_t)n0;
                    if (g.atom_hits) g.atom_hits[(ct.row0 + ri) * A + a] = (int32_t)h0;
                }
            }
        }
        __syncthreads();
        // ---- the tile's rows (rows behind the chain's length have no query atom: 0) ----
        if (tid < TR && ct.q0 + tid < ct.rows) {
            const uint64_t o = ct.row0 + ct.q0 + tid;
            if constexpr (DECIDE) {
                const unsigned long long P0 = r_cnt[tid][0], H0 = r_cnt[tid][1], P1 = r_cnt[tid][2], H1 = r_cnt[tid][3];
                g.swapped[o] = H1 * P0 > H0 * P1 ? 1 : 0;
            } else {
                const uint32_t pairs = r_cnt[tid][0], hits = r_cnt[tid][1];
                g.score[o] = pairs ? f32_div_rn((float)hits, (float)(4u * pairs)) : 0.0f;
                g.pairs[o] = (int32_t)pairs; g.hits[o] = (int32_t)hits;
            }
        }
        __syncthreads();                                              // the next tile rewrites the query list and the counters
    }
}

}  // namespace fcz
