// fcz_lddt.h -- two dense tensor batches of one shape (true, pred) -> per-residue lDDT on the sites of one slot: score [rows] float32,
// pairs [rows] int32, hits [rows] int32, on the device. The reference has no such output (Foldcomp::decompress, src/foldcomp.cpp:779,
// ends at a flat vector<AtomCoordinate>); the call stands beside fcz_knn_dev and reads what fcz_dense_dev / fcz_dense_packed_dev
// write, or any tensors of those shapes (include/fcz_hip.h, fcz_lddt_dev).
//
// The contract (include/fcz_hip.h): a row is a SITE when it lies inside its chain, both masks at the slot are set (a NULL mask_pred
// is all set) and its six coordinates there are finite. For sites i != j of one chain d2 = (dx*dx + dy*dy) + dz*dz in float32, every
// operation rounded, no FMA (fcz_knn's d2), in either tensor, and d its correctly rounded root (f32_sqrt_rn). j is a PAIR of i when
// d_true < cutoff; a pair scores one HIT per threshold that |d_true - d_pred| lies under. The counters are integers, so the result
// does not depend on the order the candidates are met in.
//
//   k_lddt<PACKED>        the shape of k_knn: persistent blocks over QUERY TILES of CHAIN_TILE = 256 rows of one chain, a lane per
//                         query (fcz_chains.h gives the chain of a tile and its rows). The chain's sites are staged in LDS in passes
//                         of LDDT_PASS chain rows: SoA true x / y / z, pred x / y / z and the compacted row number, 28 bytes a row
//                         (slots are handed out by an LDS counter -- the order inside a pass is free, see above). Every lane sweeps
//                         the pass: one broadcast LDS read per candidate, eight float operations for the true d2 and ONE compare:
//                         the rounded root is monotone, so d_true < cutoff <=> d2 < c2 with c2 the smallest float32 whose rounded
//                         root is >= cutoff (lddt_c2, on the host). Only when some lane of the wavefront has a pair does the
//                         wavefront pay for the pred d2, the two roots and the four compares. A lane keeps two integer counters and
//                         no list. A wavefront without a query skips the sweep and keeps the barriers.
//                         LDDT_PASS = 1024 rows is 28 KiB of LDS a block, so five blocks (20 wavefronts, five per SIMD) share a
//                         CU's 160 KiB; the kernel needs few registers, so LDS is what bounds the blocks on a CU, and the sweep has
//                         nothing but other wavefronts to hide its LDS reads and double-precision roots behind. 2048 rows (k_knn's
//                         pass, 16 bytes a row there) would be 56 KiB and two blocks. Chains of up to 1024 residues, nearly all
//                         there are, still take one pass; a longer chain pays three barriers per further pass.
//                         The L x L matrices are never written: HBM sees the slot's 24 bytes per row and 12 bytes of output.
//                         Padded form: every row of the entry is written, 0 / 0 / 0 where it is no site.
//   k_chain_fill<lddt_args>   (fcz_chains.h) packed form only, in front of k_lddt: 0 / 0 / 0 (chain_empty_row) into every row that
//                         no chain is seen to cover (chain_covers: a covered row it misses is rewritten by k_lddt behind it).
//
// Every index that scales with rows * A is 64-bit. A chain's range is clamped to the R rows that exist and a range that runs
// backwards is empty (chain_range), so no read leaves the inputs whatever row_off holds. hits <= 4 * (rows of a chain - 1) fits
// int32 because the ABI refuses more than 2^29 rows per chain.
#pragma once
#include "fcz_chains.h"

namespace fcz {

constexpr uint32_t LDDT_PASS = 1024;        // chain rows staged per candidate pass: 28 KiB of LDS
constexpr uint32_t LDDT_MAX_ROWS = 1u << 29;

struct lddt_args {
    const float* pos_true; const uint8_t* mask_true;
    const float* pos_pred; const uint8_t* mask_pred;   // mask_pred may be NULL: every slot present
    const uint32_t* bound;                  // padded: length [n] or NULL; packed: row_off [n + 1]
    uint32_t n, L;                          // padded: rows per entry; packed: L = R, the rows of the arrays
    uint32_t A, slot;
    float c2;                               // d_true < cutoff <=> d2_true < c2 (lddt_c2)
    float t0, t1, t2, t3;
    float* score; int32_t* pairs; int32_t* hits;
};

// the smallest float32 whose correctly rounded root is >= cutoff (cutoff finite and > 0; +inf when no finite d2 reaches it). The
// rounded product cutoff * cutoff is within an ulp of it, so both loops take a step or two (from 0 or +inf: one).
inline float lddt_c2(float cutoff) {
    float x = cutoff * cutoff;
    while (f32_sqrt_rn(x) < cutoff) x = nextafterf(x, INFINITY);
    while (x > 0.0f && f32_sqrt_rn(nextafterf(x, 0.0f)) >= cutoff) x = nextafterf(x, 0.0f);
    return x;
}

// the slot's coordinates of array row r in both tensors -> true when the row is a site (both masks set, six finite values)
__device__ __forceinline__ bool lddt_site(const lddt_args& g, uint64_t r, float* t, float* p) {
    return chain_site2(g.pos_true, g.mask_true, r * g.A + g.slot, g.pos_pred, g.mask_pred, r * g.A + g.slot, t, p);
}

// the hits of a pair: the thresholds of g (lddt_args or lddta_args) that |d_true - d_pred| lies under, from d2_true and d_pred
template <class Args>
__device__ __forceinline__ uint32_t lddt_hits(const Args& g, float d2, float sp) {
    const float diff = fabsf(__fsub_rn(f32_sqrt_rn(d2), sp));                 // +inf or NaN when d_pred is +inf: under no threshold
    return (diff < g.t0 ? 1u : 0u) + (diff < g.t1 ? 1u : 0u) + (diff < g.t2 ? 1u : 0u) + (diff < g.t3 ? 1u : 0u);
}

// row r of the arrays holds nothing
__device__ __forceinline__ void chain_empty_row(const lddt_args& g, uint64_t r) { g.score[r] = 0.0f; g.pairs[r] = 0; g.hits[r] = 0; }

template <bool PACKED>
__global__ __launch_bounds__(BLOCK) void k_lddt(lddt_args g, const uint64_t* __restrict__ tile_off, uint32_t tiles_per_entry, uint64_t n_tiles_padded) {
    __shared__ float s_tx[LDDT_PASS], s_ty[LDDT_PASS], s_tz[LDDT_PASS], s_px[LDDT_PASS], s_py[LDDT_PASS], s_pz[LDDT_PASS];
    __shared__ uint32_t s_j[LDDT_PASS];
    __shared__ uint32_t s_count;
    const uint32_t tid = threadIdx.x;
    const uint64_t n_tiles = chain_tile_count<PACKED>(tile_off, g.n, n_tiles_padded);
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const chain_tile<PACKED> ct(tile_off, g.n, tiles_per_entry, g.bound, g.L, tile, CHAIN_TILE);
        const uint64_t q = ct.q0 + tid;                               // this lane's row of the chain
        float qt[3] = {0.0f, 0.0f, 0.0f}, qp[3] = {0.0f, 0.0f, 0.0f};
        const bool query = q < ct.len && lddt_site(g, ct.row0 + q, qt, qp);
        const uint32_t qj = (uint32_t)q;
        uint32_t pairs = 0, hits = 0;
        for (uint32_t c0 = 0; c0 < ct.len;) {
            const uint32_t count = chain_stage_rows<LDDT_PASS>(&s_count, ct.len, &c0, [&](uint64_t r, chain_slots slots) __attribute__((always_inline)) {
                float t[3], p[3];
                if (lddt_site(g, ct.row0 + r, t, p)) {
                    const uint32_t i = slots.next();
                    s_tx[i] = t[0]; s_ty[i] = t[1]; s_tz[i] = t[2]; s_px[i] = p[0]; s_py[i] = p[1]; s_pz[i] = p[2]; s_j[i] = (uint32_t)r;
                }
            });
            if (__any(query)) {
                for (uint32_t c = 0; c < count; c++) {
                    const float d2 = chain_d2(s_tx[c], s_ty[c], s_tz[c], qt[0], qt[1], qt[2]);
                    const bool pair = query && s_j[c] != qj && d2 < g.c2;   // (a d2 of +inf is no pair: c2 <= +inf)
                    if (__any(pair)) {
                        const uint32_t h = lddt_hits(g, d2, f32_sqrt_rn(chain_d2(s_px[c], s_py[c], s_pz[c], qp[0], qp[1], qp[2])));
                        pairs += pair ? 1u : 0u;
                        hits += pair ? h : 0u;
                    }
                }
            }
            __syncthreads();                                          // the next pass (or tile) rewrites the staging
        }
        if (q < ct.rows) {
            const uint64_t o = ct.row0 + q;
            g.score[o] = pairs ? f32_div_rn((float)hits, (float)(4u * pairs)) : 0.0f;
            g.pairs[o] = (int32_t)pairs; g.hits[o] = (int32_t)hits;
        }
    }
}

}  // namespace fcz
