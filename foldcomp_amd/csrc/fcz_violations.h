// fcz_violations.h -- dense tensors -> the structural violations of every chain on the device: which atoms of different residues sit
// inside each other (steric clashes), and whether consecutive residues are still linked by a peptide bond of sane length and angles.
// The reference has no such output (Foldcomp::decompress, src/foldcomp.cpp:779, ends at a flat vector<AtomCoordinate>); the calls
// stand beside fcz_sasa_dev and read what fcz_dense_dev / fcz_dense_packed_dev write (include/fcz_hip.h, fcz_violations_dev).
//
// The contract (include/fcz_hip.h): an ATOM is fcz_sasa_dev's atom with probe 0: a slot (row, a) of a row inside its chain with its
// mask set, three finite coordinates and a non-zero radius R in radius_table[min(aatype, 20)][a]. All arithmetic is float32, every
// operation rounded, no FMA; d2 = (dx*dx + dy*dy) + dz*dz (fcz_knn's d2). Atoms i and j of DIFFERENT ROWS of one chain CLASH when
// T = (Ri + Rj) - tolerance is > 0 and d2(c_i, c_j) < T * T, unless the pair is a peptide bond (C of row r, N of row r + 1) or a
// disulfide (SG and SG of two rows with aatype 4). Ri + Rj commutes and d2(a, b) == d2(b, a) bit for bit (the differences are
// negated, the squares are the same), so the predicate is symmetric: every pair is met once from each side.
//
//   k_violations<PACKED>
//       Persistent blocks over QUERY TILES of whole rows of one chain: 20 rows in atom37, 18 in atom14, 64 in backbone4
//       (viol_tile_rows; tiles are counted in rows by k_chain_tiles and the scan of fcz_chains.h). A tile's atoms are
//       compacted into LDS (at most VIOL_TILE_SLOTS = 20 * 37 = 740) and taken in ROUNDS of BLOCK = 256: A LANE PER QUERY ATOM.
//       The chain's atoms are staged in LDS in passes of at most VIOL_PASS = 1536, compacted as k_sasa_points stages them
//       (chain_stage_slots, fcz_chains.h): float4 (x, y, z, R), the chain row (uint32) and a kind byte (0, 1 = N, 2 = C, 3 = SG of a CYS row: all the exclusions need), 21
//       bytes an atom. Every lane then walks the pass from its first atom to its last: all 64 lanes of a wavefront read the SAME
//       candidate, one broadcast ds_read_b128 and one ds_read_b32 (no bank conflict: a single address), and do one d2 and one
//       compare each. The kind byte is read only behind a hit.
//       Why a lane per query and not SASA's wavefront per query with a ballot: SASA needs the ballot because a hit starts work for
//       64 lanes (the points). Here a hit is three integer operations, the test itself is the work, and with a lane per candidate
//       the per-query results (count, best key) would need a wavefront reduction per query atom and the candidate would have to be
//       re-read for every query atom (SASA_Q = 8 LDS reads of 21 bytes a lane and candidate chunk); with a lane per query the results
//       stay in three VGPRs, a candidate costs a wavefront two LDS instructions for 64 tests, and the only divergent branch is the
//       hit itself, which is rare (a sane structure has none). A wavefront whose 64 query slots of the round are all empty skips the
//       sweep (wave-uniform); the barriers are kept. 20 rows of atom37 hold 156 atoms on average (7.8 heavy atoms a residue), so a
//       round fills 61 % of its lanes and a second round is needed only above 12.8 atoms a row; NOBODY HAS MEASURED tile or pass
//       size: tools/violations_rate.py reports the rate of the constants as they stand.
//       There is NO CULL: every (query atom, candidate) pair of a chain is tested, so nothing but the definition decides a result.
//       LDS: 1536 * 21 = 32256 bytes of candidates, 740 * 19 = 14060 of query atoms (float4, tile slot uint16, kind), 64 * 16 = 1024
//       of per-row results, 24 of counters: 47376 bytes a block with the alignment, so THREE blocks (12 wavefronts, three per SIMD)
//       share a CU's 160 KiB and a wavefront may hold 170 VGPRs. `make asm` prints the VGPRs: padded 79, packed 75, no scratch (LDS
//       is the limit; a pass of 1024 atoms would buy the fourth block).
//       The tile's epilogue writes the per-row outputs: a lane's count goes to its row by an LDS atomic add, its best pair to the
//       row by an LDS atomic max of the 64-bit key (bits of depth << 32) | (0xFFFFFFFF - partner row) -- depth >= 0 orders as an
//       unsigned integer, and of equal depths the smallest row wins, as fcz_knn.h builds its keys the other way round; key 0 is "no
//       pair": a row is below 2^31, so no pair has the low word 0). Both are integer operations: no order of evaluation changes them.
//       The LINK of row r (C of r to N of r + 1) is computed by the same lane per row from HBM (eight slots, just staged: L2).
//       The chain's four counters get the tile's sums by one 64-bit atomic add each (ordinary vector atomics on integers; the host
//       clears them in front). Pairs are counted once as the hits with partner row > own row, which the symmetry makes exactly half.
//       HBM sees the inputs, one byte a slot and 23 bytes a row: no rows x rows and no atoms x atoms array.
//   k_chain_fill<viol_args>   (fcz_chains.h) packed form only, in front of the sweep: 0, -1 for clash_partner (chain_empty_row),
//                 into every row that no chain is seen to cover.
//
// Every index that scales with rows * A is 64-bit. A chain's range is clamped to the R rows that exist and a range that runs
// backwards is empty (chain_range), so no read leaves the inputs whatever row_off holds; aatype is clamped to 20 before the table
// is read. Rows behind a padded entry's length are written 0 without being read.
#pragma once
#include "fcz_chains.h"

namespace fcz {

constexpr uint32_t VIOL_PASS = 1536;        // candidate atoms staged per pass, at most
constexpr uint32_t VIOL_STEP = 2 * BLOCK;   // slots examined per staging step: two a lane
constexpr uint32_t VIOL_TILE_SLOTS = 740;   // >= viol_tile_rows(A) * A
constexpr uint32_t VIOL_MAX_TILE_ROWS = 64;
constexpr uint32_t VIOL_CYS = 4, VIOL_PRO = 14;   // aatype of the disulfide exclusion and of the proline link
enum : uint32_t { VIOL_KIND_N = 1, VIOL_KIND_C = 2, VIOL_KIND_SG = 3 };

__host__ __device__ __forceinline__ uint32_t viol_tile_rows(uint32_t A) { return A == 37u ? 20u : A == 14u ? 18u : 64u; }
static_assert(VIOL_PASS % VIOL_STEP == 0 && 20 * 37 <= VIOL_TILE_SLOTS && 18 * 14 <= VIOL_TILE_SLOTS && 64 * 4 <= VIOL_TILE_SLOTS &&
              VIOL_TILE_SLOTS < 65536 && VIOL_MAX_TILE_ROWS <= BLOCK, "fcz_violations.h");

struct viol_args {
    const float* pos; const uint8_t* mask; const uint8_t* aatype;   // aatype may be NULL: every row uses row 0 of the table
    const uint32_t* bound;                  // padded: length [n] or NULL; packed: row_off [n + 1]
    uint32_t n, L;                          // padded: rows per entry; packed: L = R, the rows of the arrays
    uint32_t A;
    uint32_t n_slot, ca_slot, c_slot;       // fcz_dense_slot of N, CA, C in the layout
    int32_t sg_slot;                        // of CYS SG, -1 in backbone4
    float tolerance, link_factor;
    uint8_t* clash_atom; int32_t* clash_count; float* clash_depth; int32_t* clash_partner; uint8_t* viol_mask;
    uint8_t* link_mask; float* link_length; float* link_cos; uint8_t* link_violation;
    unsigned long long* chain_counts;       // [n][4], cleared by the host in front of the sweep
};

// slot a of array row r (a row inside its chain) -> true when it is an atom (chain_atom); c = (x, y, z, R), kind = what the exclusions ask
__device__ __forceinline__ bool viol_atom(const viol_args& g, const chain_radii& tab, uint64_t r, uint32_t a, float4* c, uint32_t* kind) {
    uint32_t aa;
    if (!chain_atom(g, tab, r, a, c, &aa)) return false;
    *kind = a == g.n_slot ? VIOL_KIND_N : a == g.c_slot ? VIOL_KIND_C : ((int32_t)a == g.sg_slot && g.aatype && aa == VIOL_CYS) ? VIOL_KIND_SG : 0u;
    return true;
}

// slot a of array row r -> true when mask and finiteness make it an atom of a link (the radius table plays no part)
__device__ __forceinline__ bool viol_link_atom(const viol_args& g, uint64_t r, uint32_t a, float* c) { return chain_site(g.pos, g.mask, r * g.A + a, c); }

// the cosine of the angle at b between a and c: u = a - b, v = c - b, dot / (|u| * |v|)
__device__ __forceinline__ float viol_cos(const float* a, const float* b, const float* c) {
    const float ux = __fsub_rn(a[0], b[0]), uy = __fsub_rn(a[1], b[1]), uz = __fsub_rn(a[2], b[2]);
    const float vx = __fsub_rn(c[0], b[0]), vy = __fsub_rn(c[1], b[1]), vz = __fsub_rn(c[2], b[2]);
    const float dot = __fadd_rn(__fadd_rn(__fmul_rn(ux, vx), __fmul_rn(uy, vy)), __fmul_rn(uz, vz));
    const float nu = f32_sqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(ux, ux), __fmul_rn(uy, uy)), __fmul_rn(uz, uz)));
    const float nv = f32_sqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(vx, vx), __fmul_rn(vy, vy)), __fmul_rn(vz, vz)));
    return __fdiv_rn(dot, __fmul_rn(nu, nv));
}

// row r of the arrays holds nothing: the per-row outputs, which the sweep's epilogue also writes behind a chain's length, and with
// the row's slots what the fill in front of the sweep writes
__device__ __forceinline__ void viol_empty_row(const viol_args& g, uint64_t r) {
    g.clash_count[r] = 0; g.clash_depth[r] = 0.0f; g.clash_partner[r] = -1; g.viol_mask[r] = 0;
    g.link_mask[r] = 0; g.link_length[r] = 0.0f; g.link_cos[r * 2u] = 0.0f; g.link_cos[r * 2u + 1u] = 0.0f; g.link_violation[r] = 0;
}
__device__ __forceinline__ void chain_empty_row(const viol_args& g, uint64_t r) {
    for (uint32_t a = 0; a < g.A; a++) g.clash_atom[r * g.A + a] = 0;
    viol_empty_row(g, r);
}

template <bool PACKED>
__global__ __launch_bounds__(BLOCK) void k_violations(viol_args g, const chain_radii tab, const uint64_t* __restrict__ tile_off, uint32_t tiles_per_entry,
                                                      uint64_t n_tiles_padded) {
    __shared__ float4 s_c[VIOL_PASS];
    __shared__ uint32_t s_row[VIOL_PASS];
    __shared__ uint8_t s_kind[VIOL_PASS];
    __shared__ float4 q_c[VIOL_TILE_SLOTS];
    __shared__ uint16_t q_at[VIOL_TILE_SLOTS];                        // the atom's slot of the tile, row of the tile * A + a
    __shared__ uint8_t q_kind[VIOL_TILE_SLOTS];
    __shared__ unsigned long long r_key[VIOL_MAX_TILE_ROWS];
    __shared__ uint32_t r_cnt[VIOL_MAX_TILE_ROWS], r_any[VIOL_MAX_TILE_ROWS];
    __shared__ uint32_t s_count, s_nq, s_sum[4];                      // s_sum: atoms (unused slot), pairs once, rows with bit 0, rows with bit 1 or 2
    const uint32_t tid = threadIdx.x;
    const uint32_t A = g.A;
    const uint32_t TR = viol_tile_rows(A);
    const float tol = g.tolerance;
    const uint64_t n_tiles = chain_tile_count<PACKED>(tile_off, g.n, n_tiles_padded);
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const chain_tile<PACKED> ct(tile_off, g.n, tiles_per_entry, g.bound, g.L, tile, TR);
        // ---- the tile's atoms, compacted; every slot that is none is written 0 here, every atom at the end of its round ----
        if (tid == 0) s_nq = 0;
        if (tid < 4) s_sum[tid] = 0;
        if (tid < TR) { r_key[tid] = 0ull; r_cnt[tid] = 0; r_any[tid] = 0; }
        __syncthreads();
        chain_tile_slots(TR, A, ct.q0, [&](uint32_t x, uint32_t rr, uint32_t a, uint64_t q) __attribute__((always_inline)) {
            if (q < ct.rows) {
                float4 c; uint32_t kind;
                if (q < ct.len && viol_atom(g, tab, ct.row0 + q, a, &c, &kind)) {
                    const uint32_t i = atomicAdd(&s_nq, 1u);          // (< VIOL_TILE_SLOTS: one slot per slot of the tile)
                    q_c[i] = c; q_at[i] = (uint16_t)x; q_kind[i] = (uint8_t)kind;
                    r_any[rr] = 1u;                                   // (every writer stores the same value)
                } else {
                    g.clash_atom[(ct.row0 + q) * A + a] = 0;
                }
            }
        });
        __syncthreads();
        const uint32_t nq = s_nq;
        for (uint32_t base = 0; base < nq; base += BLOCK) {
            const uint32_t qi = base + tid;
            const bool have = qi < nq;
            const bool wave_has = base + (tid & ~63u) < nq;           // wave-uniform: some lane of this wavefront holds a query atom
            const float4 ci = have ? q_c[qi] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            const uint32_t at = have ? q_at[qi] : 0u, ki = have ? q_kind[qi] : 0u;
            const uint32_t rr = chain_div_a(at, A);
            const uint32_t ri = (uint32_t)ct.q0 + rr;                 // the query atom's row of the chain (< len <= 2^31 - 1)
            uint32_t cnt = 0, cnt_up = 0;
            unsigned long long key = 0ull;
            // ---- the chain's atoms in passes ----
            for (uint32_t r0 = 0; r0 < ct.len;) {
                const uint32_t count = chain_stage_slots<VIOL_PASS, VIOL_STEP>(&s_count, A, ct.len, &r0, [&](uint32_t r, uint32_t a, chain_slots slots) __attribute__((always_inline)) {
                    float4 c; uint32_t kind;
                    if (viol_atom(g, tab, ct.row0 + r, a, &c, &kind)) {
                        const uint32_t i = slots.next();
                        s_c[i] = c; s_row[i] = r; s_kind[i] = (uint8_t)kind;
                    }
                });
                // ---- the sweep: every lane meets every staged atom, all lanes of a wavefront the same one at a time ----
                if (wave_has) {
                    for (uint32_t j = 0; j < count; j++) {
                        const float4 cj = s_c[j];                     // one broadcast read
                        const uint32_t rj = s_row[j];
                        const float T = __fsub_rn(__fadd_rn(ci.w, cj.w), tol);
                        const float d2 = chain_d2(ci.x, ci.y, ci.z, cj.x, cj.y, cj.z);
                        if (have && rj != ri && T > 0.0f && d2 < __fmul_rn(T, T)) {
                            const uint32_t kj = s_kind[j];
                            const bool bonded = (ki == VIOL_KIND_C && kj == VIOL_KIND_N && rj == ri + 1u) ||
                                                (ki == VIOL_KIND_N && kj == VIOL_KIND_C && rj + 1u == ri) || (ki == VIOL_KIND_SG && kj == VIOL_KIND_SG);
                            if (!bonded) {
                                cnt++;
                                cnt_up += rj > ri ? 1u : 0u;
                                const float depth = __fsub_rn(T, f32_sqrt_rn(d2));   // >= 0: sqrt is monotone and sqrt(T * T) == T
                                const unsigned long long k = ((unsigned long long)__float_as_uint(depth) << 32) | (unsigned long long)(0xFFFFFFFFu - rj);
                                key = k > key ? k : key;
                            }
                        }
                    }
                }
                __syncthreads();                                      // the next pass (or round, or tile) rewrites the staging
            }
            // ---- the round's atoms ----
            if (have) {
                g.clash_atom[(ct.row0 + ri) * A + (at - rr * A)] = cnt ? 1 : 0;
                if (cnt) { atomicAdd(&r_cnt[rr], cnt); atomicMax(&r_key[rr], key); }
                if (cnt_up) atomicAdd(&s_sum[1], cnt_up);
            }
        }
        __syncthreads();
        // ---- the tile's rows: the clash summary and the link to the next row ----
        if (tid < TR && ct.q0 + tid < ct.rows) {
            const uint32_t q = (uint32_t)(ct.q0 + tid);
            const uint64_t r = ct.row0 + q;
            if (q >= ct.len) {
                viol_empty_row(g, r);
            } else {
                const unsigned long long key = r_key[tid];
                g.clash_count[r] = (int32_t)r_cnt[tid];
                g.clash_depth[r] = key ? __uint_as_float((uint32_t)(key >> 32)) : 0.0f;
                g.clash_partner[r] = key ? (int32_t)(0xFFFFFFFFu - (uint32_t)key) : -1;
                g.viol_mask[r] = r_any[tid] ? 1 : 0;
                float ca[3], c[3], n1[3], ca1[3];
                bool link = q + 1u < ct.len;
                if (link) {                                           // (row r + 1 is a row of the chain: inside the arrays)
                    const bool a0 = viol_link_atom(g, r, g.ca_slot, ca), a1 = viol_link_atom(g, r, g.c_slot, c);
                    const bool a2 = viol_link_atom(g, r + 1u, g.n_slot, n1), a3 = viol_link_atom(g, r + 1u, g.ca_slot, ca1);
                    link = a0 && a1 && a2 && a3;
                }
                float length = 0.0f, cos0 = 0.0f, cos1 = 0.0f;
                uint32_t bits = 0;
                if (link) {
                    const bool pro = g.aatype && g.aatype[r + 1u] == VIOL_PRO;
                    length = f32_sqrt_rn(chain_d2(c[0], c[1], c[2], n1[0], n1[1], n1[2]));
                    cos0 = viol_cos(ca, c, n1);
                    cos1 = viol_cos(c, n1, ca1);
                    const float l0 = pro ? 1.341f : 1.329f, sl = pro ? 0.016f : 0.014f;
                    if (fabsf(__fsub_rn(length, l0)) > __fmul_rn(g.link_factor, sl)) bits |= 1u;
                    if (fabsf(__fsub_rn(cos0, -0.4473f)) > __fmul_rn(g.link_factor, 0.0311f)) bits |= 2u;
                    if (fabsf(__fsub_rn(cos1, -0.5203f)) > __fmul_rn(g.link_factor, 0.0353f)) bits |= 4u;
                    if (bits & 1u) atomicAdd(&s_sum[2], 1u);
                    if (bits & 6u) atomicAdd(&s_sum[3], 1u);
                }
                g.link_mask[r] = link ? 1 : 0; g.link_length[r] = length; g.link_cos[r * 2u] = cos0; g.link_cos[r * 2u + 1u] = cos1;
                g.link_violation[r] = (uint8_t)bits;
            }
        }
        __syncthreads();
        if (tid < 4) {
            const uint32_t v = tid == 0 ? nq : s_sum[tid];
            if (v) atomicAdd(&g.chain_counts[(uint64_t)ct.e * 4u + tid], (unsigned long long)v);
        }
        __syncthreads();                                              // the next tile rewrites the query list and the sums
    }
}

}  // namespace fcz
