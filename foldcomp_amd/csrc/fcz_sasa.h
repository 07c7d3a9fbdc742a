// fcz_sasa.h -- dense tensors -> per-residue solvent accessibility (Shrake & Rupley 1973) on the device: the exposed surface points
// of every atom slot, sasa_points [rows][A] int16, the area of every residue, sasa [rows] float32 in square Angstrom, and sasa_mask
// [rows] uint8. The reference has no such output (Foldcomp::decompress, src/foldcomp.cpp:779, ends at a flat vector<AtomCoordinate>);
// the calls stand beside fcz_hbond_dev / fcz_lddt_dev and read what fcz_dense_dev / fcz_dense_packed_dev write (include/fcz_hip.h,
// fcz_sasa_dev). This is the first sweep that visits every atom of the tensors, not one site or four atoms of a row.
//
// The contract (include/fcz_hip.h): an ATOM is a slot (row, a) of a row inside its chain with its mask set, three finite coordinates
// and a non-zero radius in radius_table[min(aatype, 20)][a]. R = radius + probe. All arithmetic is float32, every operation rounded, no
// FMA; d2 = (dx*dx + dy*dy) + dz*dz (fcz_knn's d2). Atom j is a CANDIDATE of atom i when (row, slot) differ and d2(c_i, c_j) < S * S
// with S = Ri + Rj; point k of atom i, t_k = c_i + Ri * u_k per component, is BURIED when a candidate has d2(t_k, c_j) < Rj * Rj. The
// result of an atom is the number of its points no candidate buries: an integer that no order of evaluation changes.
//
//   k_sasa_points<PACKED, SMALL>
//       Persistent blocks over QUERY TILES of SASA_TILE_ROWS = 3 rows of one chain (tiles are counted in rows by k_chain_tiles and the
//       scan of fcz_chains.h, with this header's own rows per tile: CHAIN_TILE is a lane per row and does not fit). A tile's
//       atoms are compacted into LDS (at most 3 * 37 = 111) and taken in ROUNDS of SASA_GROUP = 32: the four wavefronts of the block
//       take a round's atoms round-robin, SASA_Q = 8 each. A WAVEFRONT PER QUERY ATOM, the lanes over two things in turn:
//         * the chain's atoms are staged in LDS in passes of at most SASA_PASS = 1536, compacted: float4 (x, y, z, Rj), the chain row
//           (uint32) and the slot (uint8), 21 bytes an atom (row * A + slot in one word would wrap for chains above 2^32 / 37 rows, so
//           the identity keeps both). A pass is staged in steps of the rows that hold at most 512 slots, two slots a lane, and is
//           closed when another step might not fit; in backbone4 with every mask set that is exactly 1536 atoms
//           (chain_stage_slots, fcz_chains.h, which k_violations and k_lddt_atoms stage through as well);
//         * per 64 staged candidates lane = candidate: one d2(c_i, c_j) < S * S test a lane, and the ballot of that test is the
//           wavefront's candidate set for this query atom. The candidate is read once for all eight query atoms of the wavefront;
//         * for every set bit the candidate comes back as one broadcast LDS read and lane = point: lane l owns points l, l + 64, ..
//           (at most 16), one "still exposed" bit each in ONE VGPR per query atom. There is no per-atom neighbour list, no lane idles
//           while another walks its points, and every branch on a ballot is wave-uniform. t_k is computed once per (query atom,
//           64 candidates with a hit, point), not per candidate. SMALL (P <= 128): a lane's two directions stay in six VGPRs;
//           otherwise they are read from points_dev (12 KiB at most: L1 / L2) per use;
//         * a query atom whose bits are all cleared skips the rest of the sweep; the barriers are kept.
//       The exposure bits have to survive the passes, which is why a wavefront holds a fixed SASA_Q of query atoms (eight VGPRs, the
//       loop over them fully unrolled) and sweeps a staged pass for each in turn. The trade: every round restages the whole chain
//       out of L2, atoms^2 / 32 * 21 bytes per chain at full rounds (2700 atoms: about 4.8 MB), and a larger round would restage
//       less for more registers and more unrolled code. A round of a 3-row tile holds 23 atoms on average in atom37 (7.8 heavy atoms
//       a residue), so a quarter of the query slots idle; 4 rows would overflow into a second, nearly empty round in almost half the
//       tiles. NOBODY HAS MEASURED pass, round or tile size: tools/sasa_rate.py reports the rate of the constants as they stand.
//       LDS: 1536 * 21 = 32256 bytes of candidates, 112 * 25 = 2800 bytes of query atoms (float4, row, slot, count), 8 of counters:
//       35064 bytes a block, so FOUR blocks (16 wavefronts, four per SIMD) share a CU's 160 KiB and a wavefront may hold 128 VGPRs
//       (k_lddt / k_hbond run five blocks at 30 KiB; the slot byte and the query list cost the fifth). `make asm` prints the VGPRs:
//       padded SMALL 59, padded large 53, packed SMALL 56, packed large 53, no scratch (all run four blocks; LDS is the limit, and
//       1280 atoms a pass would buy the fifth).
//       The tile's epilogue also writes the per-residue outputs: a tile is whole rows, so the block has every count of the row in LDS
//       and one lane per row does the float64 sum. (A separate lane-per-row kernel would need a second tiling of the packed form,
//       CHAIN_TILE rows, and would read the counts back from HBM.) Every term is an integer of at most 11 bits times a float32 in
//       [0.25, 64) and at most 37 are summed, so the float64 sum is exact and does not depend on the order the compaction gave.
//       HBM sees the inputs, 2 bytes a slot and 5 bytes a row: no rows x rows and no atoms x atoms array.
//   k_chain_fill<sasa_args>   (fcz_chains.h) packed form only, in front of the sweep: 0 (chain_empty_row) into every row that no
//                 chain is seen to cover (chain_covers: a covered row it misses is rewritten by the sweep behind it).
//
// Every index that scales with rows * A is 64-bit. A chain's range is clamped to the R rows that exist and a range that runs
// backwards is empty (chain_range), so no read leaves the inputs whatever row_off holds; aatype is clamped to 20 before the table
// is read. Rows behind a padded entry's length are written 0 without being read.
#pragma once
#include "fcz_chains.h"

namespace fcz {

constexpr uint32_t SASA_PASS = 1536;        // candidate atoms staged per pass, at most
constexpr uint32_t SASA_STEP = 2 * BLOCK;   // slots examined per staging step: two a lane
constexpr uint32_t SASA_Q = 8;              // query atoms a wavefront holds: one VGPR of exposure bits each
constexpr uint32_t SASA_GROUP = SASA_Q * (BLOCK / 64);   // query atoms per round
constexpr uint32_t SASA_TILE_ROWS = 3;      // rows per query tile
constexpr uint32_t SASA_TILE_ATOMS = 112;   // >= SASA_TILE_ROWS * DN_MAX_WIDTH
constexpr uint32_t SASA_MAX_POINTS = 1024;  // 16 points a lane
constexpr uint32_t SASA_SMALL_POINTS = 128; // two points a lane: their directions stay in registers
constexpr uint32_t SASA_MAX_ROWS = 0x7FFFFFFFu;
static_assert(SASA_TILE_ATOMS >= SASA_TILE_ROWS * DN_MAX_WIDTH && SASA_PASS % SASA_STEP == 0 && SASA_GROUP == 32, "fcz_sasa.h");

struct sasa_args {
    const float* pos; const uint8_t* mask; const uint8_t* aatype;   // aatype may be NULL: every row uses row 0 of the table
    const uint32_t* bound;                  // padded: length [n] or NULL; packed: row_off [n + 1]
    uint32_t n, L;                          // padded: rows per entry; packed: L = R, the rows of the arrays
    uint32_t A, P;
    float probe;
    const float* points;                    // [P][3]
    double scale;                           // 4 pi / P
    int16_t* sasa_points; float* sasa; uint8_t* sasa_mask;
};

// slot a of array row r (a row inside its chain) -> true when it is an atom (chain_atom); c = (x, y, z, R) with R = radius + probe
__device__ __forceinline__ bool sasa_atom(const sasa_args& g, const chain_radii& tab, uint64_t r, uint32_t a, float4* c) {
    uint32_t ty;
    if (!chain_atom(g, tab, r, a, c, &ty)) return false;
    c->w = __fadd_rn(c->w, g.probe);
    return true;
}

// row r of the arrays holds nothing
__device__ __forceinline__ void chain_empty_row(const sasa_args& g, uint64_t r) {
    for (uint32_t a = 0; a < g.A; a++) g.sasa_points[r * g.A + a] = 0;
    g.sasa[r] = 0.0f; g.sasa_mask[r] = 0;
}

// the lane's p-th point (number p * 64 + lane) of the query atom ci against the candidates `hits` of the 64 staged at c0: clears the
// point's bit when one of them buries it. u: the point's direction.
__device__ __forceinline__ uint32_t sasa_point(uint32_t bits, uint32_t p, float4 ci, float ux, float uy, float uz, uint64_t hits, const float4* s_c, uint32_t c0) {
    const float tx = __fadd_rn(ci.x, __fmul_rn(ci.w, ux)), ty = __fadd_rn(ci.y, __fmul_rn(ci.w, uy)), tz = __fadd_rn(ci.z, __fmul_rn(ci.w, uz));
    bool buried = false;
    while (hits) {                                                    // wave-uniform: hits is a ballot
        const uint32_t b = (uint32_t)__ffsll((unsigned long long)hits) - 1u;
        hits &= hits - 1u;
        const float4 cj = s_c[c0 + b];                                // one broadcast read
        buried = buried || chain_d2(tx, ty, tz, cj.x, cj.y, cj.z) < __fmul_rn(cj.w, cj.w);
    }
    return buried ? bits & ~(1u << p) : bits;
}

template <bool PACKED, bool SMALL>
__global__ __launch_bounds__(BLOCK) void k_sasa_points(sasa_args g, const chain_radii tab, const uint64_t* __restrict__ tile_off, uint32_t tiles_per_entry,
                                                       uint64_t n_tiles_padded) {
    __shared__ float4 s_c[SASA_PASS];
    __shared__ uint32_t s_row[SASA_PASS];
    __shared__ uint8_t s_slot[SASA_PASS];
    __shared__ float4 q_c[SASA_TILE_ATOMS];
    __shared__ uint32_t q_row[SASA_TILE_ATOMS], q_cnt[SASA_TILE_ATOMS];
    __shared__ uint8_t q_slot[SASA_TILE_ATOMS];
    __shared__ uint32_t s_count, s_nq;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t A = g.A, P = g.P;
    const uint32_t per_lane = (P + 63u) / 64u;                        // points a lane may own, 1 .. 16
    const uint32_t mine = lane < P ? (P - lane + 63u) / 64u : 0u;     // points this lane owns
    const uint32_t full = mine ? (0xFFFFFFFFu >> (32u - mine)) : 0u;
    float u0[3] = {0.0f, 0.0f, 0.0f}, u1[3] = {0.0f, 0.0f, 0.0f};
    if constexpr (SMALL) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            if (lane < P) u0[k] = g.points[lane * 3u + k];
            if (lane + 64u < P) u1[k] = g.points[(lane + 64u) * 3u + k];
        }
    }
    const uint64_t n_tiles = chain_tile_count<PACKED>(tile_off, g.n, n_tiles_padded);
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const chain_tile<PACKED> ct(tile_off, g.n, tiles_per_entry, g.bound, g.L, tile, SASA_TILE_ROWS);
        // ---- the tile's atoms, compacted; every slot that is none is written 0 here, every atom at the end of its round ----
        if (tid == 0) s_nq = 0;
        __syncthreads();
        chain_tile_slots(SASA_TILE_ROWS, A, ct.q0, [&](uint32_t, uint32_t, uint32_t a, uint64_t q) __attribute__((always_inline)) {
            if (q < ct.rows) {
                float4 c;
                if (q < ct.len && sasa_atom(g, tab, ct.row0 + q, a, &c)) {
                    const uint32_t i = atomicAdd(&s_nq, 1u);          // (< SASA_TILE_ATOMS: one slot per slot of the tile)
                    q_c[i] = c; q_row[i] = (uint32_t)q; q_slot[i] = (uint8_t)a; q_cnt[i] = 0;
                } else {
                    g.sasa_points[(ct.row0 + q) * A + a] = 0;
                }
            }
        });
        __syncthreads();
        const uint32_t nq = s_nq;
        for (uint32_t base = 0; base < nq; base += SASA_GROUP) {
            uint32_t bits[SASA_Q];
#pragma unroll
            for (uint32_t k = 0; k < SASA_Q; k++) bits[k] = base + wave + 4u * k < nq ? full : 0u;
            // ---- the chain's atoms in passes ----
            for (uint32_t r0 = 0; r0 < ct.len;) {
                const uint32_t count = chain_stage_slots<SASA_PASS, SASA_STEP>(&s_count, A, ct.len, &r0, [&](uint32_t r, uint32_t a, chain_slots slots) __attribute__((always_inline)) {
                    float4 c;
                    if (sasa_atom(g, tab, ct.row0 + r, a, &c)) {
                        const uint32_t i = slots.next();
                        s_c[i] = c; s_row[i] = r; s_slot[i] = (uint8_t)a;
                    }
                });
                // ---- the sweep: 64 candidates at a time, the wavefront's query atoms in turn ----
                for (uint32_t c0 = 0; c0 < count; c0 += 64u) {
                    const uint32_t j = c0 + lane;
                    const bool have = j < count;
                    const float4 cj = have ? s_c[j] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    const uint32_t jrow = have ? s_row[j] : 0u, jslot = have ? s_slot[j] : 0u;
#pragma unroll
                    for (uint32_t k = 0; k < SASA_Q; k++) {
                        if (!__any(bits[k] != 0u)) continue;          // no such query atom, or every point of it is buried
                        const uint32_t qi = base + wave + 4u * k;
                        const float4 ci = q_c[qi];
                        const float S = __fadd_rn(ci.w, cj.w);
                        const bool near = have && !(jrow == q_row[qi] && jslot == q_slot[qi]) &&
                                          chain_d2(ci.x, ci.y, ci.z, cj.x, cj.y, cj.z) < __fmul_rn(S, S);
                        const uint64_t hits = __ballot(near);
                        if (hits == 0) continue;
                        if constexpr (SMALL) {
                            bits[k] = sasa_point(bits[k], 0u, ci, u0[0], u0[1], u0[2], hits, s_c, c0);
                            if (per_lane > 1u) bits[k] = sasa_point(bits[k], 1u, ci, u1[0], u1[1], u1[2], hits, s_c, c0);
                        } else {
                            for (uint32_t p = 0; p < per_lane; p++) {
                                if (!__any((bits[k] >> p) & 1u)) continue;
                                const uint32_t pt = p * 64u + lane;
                                const float* u = g.points + (pt < P ? pt : 0u) * 3u;   // (a lane without this point: its bit is clear and stays so)
                                bits[k] = sasa_point(bits[k], p, ci, u[0], u[1], u[2], hits, s_c, c0);
                            }
                        }
                    }
                }
                __syncthreads();                                      // the next pass (or round, or tile) rewrites the staging
            }
            // ---- the round's counts ----
#pragma unroll
            for (uint32_t k = 0; k < SASA_Q; k++) {
                const uint32_t qi = base + wave + 4u * k;
                if (qi >= nq) continue;
                uint32_t total = 0;
                for (uint32_t p = 0; p < per_lane; p++) total += (uint32_t)__popcll(__ballot((bits[k] >> p) & 1u));
                if (lane == 0) {
                    q_cnt[qi] = total;
                    g.sasa_points[(ct.row0 + q_row[qi]) * A + q_slot[qi]] = (int16_t)total;
                }
            }
        }
        __syncthreads();
        // ---- the tile's rows: the float64 sum of count * R * R is exact, so the compaction's order does not show ----
        if (tid < SASA_TILE_ROWS && ct.q0 + tid < ct.rows) {
            const uint32_t q = (uint32_t)(ct.q0 + tid);
            double sum = 0.0;
            bool any = false;
            for (uint32_t i = 0; i < nq; i++)
                if (q_row[i] == q) { sum += (double)q_cnt[i] * (double)__fmul_rn(q_c[i].w, q_c[i].w); any = true; }
            g.sasa[ct.row0 + q] = (float)(sum * g.scale);
            g.sasa_mask[ct.row0 + q] = any ? 1 : 0;
        }
        __syncthreads();                                              // the next tile rewrites the query list
    }
}

}  // namespace fcz
