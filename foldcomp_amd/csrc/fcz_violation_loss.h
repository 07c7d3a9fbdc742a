// fcz_violation_loss.h -- the structural-violation LOSS of dense tensors and its gradient: the clash energy between atoms of different
// residues and the flat-bottomed penalties on the C-N' bond and the two peptide angles, on exactly the atoms, pairs and links of
// fcz_violations.h, as float32 sums with a fixed order and a fused backward. The reference has no such output (include/fcz_hip.h,
// fcz_violation_loss_dev and fcz_violation_loss_grad_dev hold the contract, every operation of it).
//
//   k_violation_loss<PACKED>        the shape of k_violations: persistent blocks over query tiles of whole rows (viol_tile_rows), the
//                                   tile's atoms compacted into LDS and taken in rounds of BLOCK, A LANE PER QUERY ATOM, the chain's
//                                   atoms staged in LDS in passes and read by broadcast. What differs:
//                                   * a lane's result is a float32 SUM of T - sqrt(d2) over its hits, so the order in which it meets
//                                     its candidates is part of the contract: ascending (row, slot). chain_stage_slots hands out
//                                     slots by an LDS atomic, an arbitrary order; the passes here are staged by
//                                     chain_stage_slots_ordered (fcz_chains.h: a ballot and a popcount inside a wavefront, a scan of
//                                     the wavefronts' totals). Passes ascend and the sum is a register that lives across them, so
//                                     the sum depends on the chain's atoms alone: not on the tile, the pass size, the grid or the
//                                     chains beside it. The ORDER OF THE QUERY ATOMS in a tile stays free (an LDS counter): which
//                                     lane holds an atom changes nothing the atom computes.
//                                   * the hit branch is the only divergent one, and the root sits behind it.
//                                   * the tile's epilogue computes the three link terms of every row, a lane a row, from HBM (eight
//                                     slots, just staged: L2), and adds the tile's atoms and links to the chain's two counters by
//                                     one 64-bit integer atomic each (the host clears them in front).
//   k_violation_loss_grad<PACKED>   the same sweep with the upstream weight w_j of every staged atom beside it, four more bytes an
//                                   atom, and three sums a lane. The pair relation is symmetric (fcz_violations.h), so pair (i, j)
//                                   stands in clash_loss[i] and in clash_loss[j] and atom i gathers its whole gradient with the
//                                   factor (w_i + w_j); nothing is kept from the value pass. A link moves four atoms of two rows:
//                                   row r recomputes link r - 1 beside link r, so that it owns its N and CA as well as its C. The
//                                   clash part and the link part land in the same slots of grad, and there is ONE WRITER A SLOT:
//                                   in front of the rounds a lane a row stashes the row's eight link terms in LDS (N: bond, cos0,
//                                   cos1 of link r - 1; CA: cos1 of link r - 1, cos0 of link r; C: bond, cos0, cos1 of link r), and
//                                   whoever writes a slot adds them in that order behind the clash sum -- the round for a slot that
//                                   is an atom, the tile compaction for one that is none (a zero radius does not stop a slot from
//                                   being a link atom). No float atomics, no scatter.
//   k_chain_fill<vloss_args / vloss_grad_args>   (fcz_chains.h) packed form only, in front of the sweep: zeros into every row that no
//                                   chain is seen to cover.
//
// Sizes. VLOSS_PASS = 1280 atoms a pass, for both kernels, so that fcz_violation_loss_pass() is one number. A staged atom is 21 bytes
// in the value kernel (float4 x y z R, the row, a kind byte) and 25 in the gradient kernel (w_j); the query tile is k_violations' 19
// bytes a slot of 740; the gradient's link stash is 64 rows * 8 terms * 12 bytes = 6144. At k_violations' 1536 atoms the gradient
// kernel would need 38400 + 14060 + 6144 bytes and THREE blocks would no longer share a CU's 160 KiB (54613 bytes a block); at 1280
// they do. `make asm` prints (gfx950): k_violation_loss 40 992 bytes of LDS, 87 VGPRs padded and 83 packed; k_violation_loss_grad
// 52 256 bytes, 98 and 99 VGPRs; no scratch in any of the four, 3 waves per SIMD in all: LDS is what bounds the blocks on a CU (three
// blocks are 12 wavefronts, so a wavefront may hold 170 VGPRs). NOBODY HAS MEASURED tile or pass
// size, here or in k_violations: the tile rows are k_violations', the pass is the largest multiple of BLOCK that keeps three blocks,
// and tools/violation_loss_rate.py reports the rate of the constants as they stand.
//
// Every index that scales with rows * A is 64-bit. A chain's range is clamped to the R rows that exist and a range that runs
// backwards is empty (chain_range), so no read leaves the inputs whatever row_off holds; aatype is clamped to 20 before the table is
// read. A weight is read only where its slot is an atom or its link exists. Rows behind a padded entry's length are written 0
// without being read.
#pragma once
#include "fcz_violations.h"

namespace fcz {

constexpr uint32_t VLOSS_PASS = 1280;       // candidate atoms staged per pass, at most
constexpr uint32_t VLOSS_STEP = 2 * BLOCK;  // slots examined per staging step: two a lane
constexpr uint32_t VLOSS_LINK_TERMS = 8;    // the link terms a row's N (3), CA (2) and C (3) receive
static_assert(VLOSS_STEP <= VLOSS_PASS && VLOSS_PASS % BLOCK == 0, "fcz_violation_loss.h");
static_assert(VLOSS_PASS * 25 + VIOL_TILE_SLOTS * 19 + VIOL_MAX_TILE_ROWS * VLOSS_LINK_TERMS * 12 + 256 <= 160 * 1024 / 3, "three blocks a CU");

struct vloss_args {
    const float* pos; const uint8_t* mask; const uint8_t* aatype;   // aatype may be NULL: every row uses row 0 of the table
    const uint32_t* bound;                  // padded: length [n] or NULL; packed: row_off [n + 1]
    uint32_t n, L;                          // padded: rows per entry; packed: L = R, the rows of the arrays
    uint32_t A;
    uint32_t n_slot, ca_slot, c_slot;       // fcz_dense_slot of N, CA, C in the layout
    int32_t sg_slot;                        // of CYS SG, -1 in backbone4
    float tolerance, link_factor;
    float* clash_loss; float* link_loss;    // [rows][A], [rows][3]
    unsigned long long* counts;             // [n][2], cleared by the host in front of the sweep
};

struct vloss_grad_args {
    const float* pos; const uint8_t* mask; const uint8_t* aatype;
    const uint32_t* bound;
    uint32_t n, L;
    uint32_t A;
    uint32_t n_slot, ca_slot, c_slot;
    int32_t sg_slot;
    float tolerance, link_factor;
    const float* w_clash; const float* w_link;   // [rows][A], [rows][3]: the upstream gradients of clash_loss and link_loss
    float* grad;                            // [rows][A][3]
};

// viol_atom for either args
template <class Args>
__device__ __forceinline__ bool vloss_atom(const Args& g, const chain_radii& tab, uint64_t r, uint32_t a, float4* c, uint32_t* kind) {
    uint32_t aa;
    if (!chain_atom(g, tab, r, a, c, &aa)) return false;
    *kind = a == g.n_slot ? VIOL_KIND_N : a == g.c_slot ? VIOL_KIND_C : ((int32_t)a == g.sg_slot && g.aatype && aa == VIOL_CYS) ? VIOL_KIND_SG : 0u;
    return true;
}

// the pair (i, j) that passed the distance test: is it struck out as a peptide bond or a disulfide? (k_violations' rule)
__device__ __forceinline__ bool vloss_bonded(uint32_t ki, uint32_t ri, uint32_t kj, uint32_t rj) {
    return (ki == VIOL_KIND_C && kj == VIOL_KIND_N && rj == ri + 1u) || (ki == VIOL_KIND_N && kj == VIOL_KIND_C && rj + 1u == ri) ||
           (ki == VIOL_KIND_SG && kj == VIOL_KIND_SG);
}

// the link from array row r to row r + 1, both rows of one chain: CA, C, N', CA' -> true when it exists (mask and finiteness alone)
template <class Args>
__device__ __forceinline__ bool vloss_link(const Args& g, uint64_t r, float* ca, float* c, float* n1, float* ca1) {
    const bool a0 = chain_site(g.pos, g.mask, r * g.A + g.ca_slot, ca), a1 = chain_site(g.pos, g.mask, r * g.A + g.c_slot, c);
    const bool a2 = chain_site(g.pos, g.mask, (r + 1u) * g.A + g.n_slot, n1), a3 = chain_site(g.pos, g.mask, (r + 1u) * g.A + g.ca_slot, ca1);
    return a0 && a1 && a2 && a3;
}

// (|x - x0| - bound)+ of a finite x, 0 of any other
__device__ __forceinline__ float vloss_term(float x, float x0, float bound) {
    const float v = __fsub_rn(fabsf(__fsub_rn(x, x0)), bound);
    return isfinite(x) && v > 0.0f ? v : 0.0f;
}

// the three terms of an existing link whose second row has the type aa1 (only read with an aatype)
template <class Args>
__device__ __forceinline__ void vloss_link_terms(const Args& g, uint64_t r, const float* ca, const float* c, const float* n1, const float* ca1, float* length,
                                                 float* cos0, float* cos1, float* t) {
    const bool pro = g.aatype && g.aatype[r + 1u] == VIOL_PRO;
    const float l0 = pro ? 1.341f : 1.329f, sl = pro ? 0.016f : 0.014f;
    *length = f32_sqrt_rn(chain_d2(c[0], c[1], c[2], n1[0], n1[1], n1[2]));
    *cos0 = viol_cos(ca, c, n1);
    *cos1 = viol_cos(c, n1, ca1);
    t[0] = vloss_term(*length, l0, __fmul_rn(g.link_factor, sl));
    t[1] = vloss_term(*cos0, -0.4473f, __fmul_rn(g.link_factor, 0.0311f));
    t[2] = vloss_term(*cos1, -0.5203f, __fmul_rn(g.link_factor, 0.0353f));
}

// k * d cos / d (a, b, c) of the angle at b between a and c, cosv = viol_cos(a, b, c): u = a - b, v = c - b,
// d cos / d a = (v / |v| - cos * (u / |u|)) / |u|, the mirror image for c, the negated sum for b; then one multiplication by k
__device__ __forceinline__ void vloss_cos_grad(const float* a, const float* b, const float* c, float cosv, float k, float* ta, float* tb, float* tc) {
    float u[3], v[3];
#pragma unroll
    for (int x = 0; x < 3; x++) { u[x] = __fsub_rn(a[x], b[x]); v[x] = __fsub_rn(c[x], b[x]); }
    const float nu = f32_sqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(u[0], u[0]), __fmul_rn(u[1], u[1])), __fmul_rn(u[2], u[2])));
    const float nv = f32_sqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(v[0], v[0]), __fmul_rn(v[1], v[1])), __fmul_rn(v[2], v[2])));
#pragma unroll
    for (int x = 0; x < 3; x++) {
        const float uh = __fdiv_rn(u[x], nu), vh = __fdiv_rn(v[x], nv);
        const float ga = __fdiv_rn(__fsub_rn(vh, __fmul_rn(cosv, uh)), nu);
        const float gc = __fdiv_rn(__fsub_rn(uh, __fmul_rn(cosv, vh)), nv);
        ta[x] = __fmul_rn(k, ga); tb[x] = __fmul_rn(k, -__fadd_rn(ga, gc)); tc[x] = __fmul_rn(k, gc);
    }
}

// w * sign(x - x0): the factor of a term that contributes (sign(0) = 0)
__device__ __forceinline__ float vloss_signed(float w, float x, float x0) {
    const float e = __fsub_rn(x, x0);
    return e > 0.0f ? w : e < 0.0f ? -w : 0.0f;
}

// The gradient terms of the link from array row r to r + 1 into t [7][3]: 0 bond -> C (N' receives its negation), 1 .. 3 cos0 -> CA, C,
// N', 4 .. 6 cos1 -> C, N', CA'. Everything is 0 where the link does not exist; a term that is 0 in the value (not violated, or not
// finite) gives 0; a bond of length 0 gives 0. w_link[r] is read only where the link exists.
__device__ __forceinline__ void vloss_link_grad(const vloss_grad_args& g, uint64_t r, float (*t)[3]) {
#pragma unroll
    for (int k = 0; k < 7; k++) { t[k][0] = 0.0f; t[k][1] = 0.0f; t[k][2] = 0.0f; }
    float ca[3], c[3], n1[3], ca1[3];
    if (!vloss_link(g, r, ca, c, n1, ca1)) return;
    float length, cos0, cos1, v[3];
    vloss_link_terms(g, r, ca, c, n1, ca1, &length, &cos0, &cos1, v);
    const float* w = g.w_link + r * 3u;
    if (v[0] > 0.0f && length != 0.0f) {
        const bool pro = g.aatype && g.aatype[r + 1u] == VIOL_PRO;
        const float k = vloss_signed(w[0], length, pro ? 1.341f : 1.329f);
#pragma unroll
        for (int x = 0; x < 3; x++) t[0][x] = __fmul_rn(k, __fdiv_rn(__fsub_rn(c[x], n1[x]), length));
    }
    if (v[1] > 0.0f) vloss_cos_grad(ca, c, n1, cos0, vloss_signed(w[1], cos0, -0.4473f), t[1], t[2], t[3]);
    if (v[2] > 0.0f) vloss_cos_grad(c, n1, ca1, cos1, vloss_signed(w[2], cos1, -0.5203f), t[4], t[5], t[6]);
}

// slot a of a row whose eight link terms lie at s: the terms of its atom added to (gx, gy, gz) one after the other
__device__ __forceinline__ void vloss_add_link(const vloss_grad_args& g, const float* s, uint32_t a, float* gx, float* gy, float* gz) {
    const uint32_t k0 = a == g.n_slot ? 0u : a == g.ca_slot ? 3u : a == g.c_slot ? 5u : 8u;
    const uint32_t k1 = a == g.n_slot ? 3u : a == g.ca_slot ? 5u : 8u;
    for (uint32_t k = k0; k < k1; k++) {
        *gx = __fadd_rn(*gx, s[k * 3u]); *gy = __fadd_rn(*gy, s[k * 3u + 1u]); *gz = __fadd_rn(*gz, s[k * 3u + 2u]);
    }
}

// row r of the arrays holds nothing
__device__ __forceinline__ void chain_empty_row(const vloss_args& g, uint64_t r) {
    for (uint32_t a = 0; a < g.A; a++) g.clash_loss[r * g.A + a] = 0.0f;
    g.link_loss[r * 3u] = 0.0f; g.link_loss[r * 3u + 1u] = 0.0f; g.link_loss[r * 3u + 2u] = 0.0f;
}
__device__ __forceinline__ void chain_empty_row(const vloss_grad_args& g, uint64_t r) {
    for (uint32_t x = 0; x < g.A * 3u; x++) g.grad[r * g.A * 3u + x] = 0.0f;
}

template <bool PACKED>
__global__ __launch_bounds__(BLOCK) void k_violation_loss(vloss_args g, const chain_radii tab, const uint64_t* __restrict__ tile_off, uint32_t tiles_per_entry,
                                                          uint64_t n_tiles_padded) {
    __shared__ float4 s_c[VLOSS_PASS];
    __shared__ uint32_t s_row[VLOSS_PASS];
    __shared__ uint8_t s_kind[VLOSS_PASS];
    __shared__ float4 q_c[VIOL_TILE_SLOTS];
    __shared__ uint16_t q_at[VIOL_TILE_SLOTS];                        // the atom's slot of the tile, row of the tile * A + a
    __shared__ uint8_t q_kind[VIOL_TILE_SLOTS];
    __shared__ uint32_t s_wave[VLOSS_STEP / 64], s_nq, s_links;
    const uint32_t tid = threadIdx.x;
    const uint32_t A = g.A;
    const uint32_t TR = viol_tile_rows(A);
    const float tol = g.tolerance;
    const uint64_t n_tiles = chain_tile_count<PACKED>(tile_off, g.n, n_tiles_padded);
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const chain_tile<PACKED> ct(tile_off, g.n, tiles_per_entry, g.bound, g.L, tile, TR);
        // ---- the tile's atoms, compacted in any order; every slot that is none is written 0 here, every atom at the end of its round ----
        if (tid == 0) { s_nq = 0; s_links = 0; }
        __syncthreads();
        chain_tile_slots(TR, A, ct.q0, [&](uint32_t x, uint32_t rr, uint32_t a, uint64_t q) __attribute__((always_inline)) {
            if (q < ct.rows) {
                float4 c; uint32_t kind;
                if (q < ct.len && vloss_atom(g, tab, ct.row0 + q, a, &c, &kind)) {
                    const uint32_t i = atomicAdd(&s_nq, 1u);          // (< VIOL_TILE_SLOTS: one slot per slot of the tile)
                    q_c[i] = c; q_at[i] = (uint16_t)x; q_kind[i] = (uint8_t)kind;
                } else {
                    g.clash_loss[(ct.row0 + q) * A + a] = 0.0f;
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
            float sum = 0.0f;                                         // lives across the passes: they ascend
            for (uint32_t r0 = 0; r0 < ct.len;) {
                float4 c2[VLOSS_STEP / BLOCK]; uint32_t k2[VLOSS_STEP / BLOCK], row2[VLOSS_STEP / BLOCK];
                const uint32_t count = chain_stage_slots_ordered<VLOSS_PASS, VLOSS_STEP>(
                    s_wave, A, ct.len, &r0,
                    [&](uint32_t r, uint32_t a, uint32_t h) __attribute__((always_inline)) { row2[h] = r; return vloss_atom(g, tab, ct.row0 + r, a, &c2[h], &k2[h]); },
                    [&](uint32_t h, uint32_t i) __attribute__((always_inline)) { s_c[i] = c2[h]; s_row[i] = row2[h]; s_kind[i] = (uint8_t)k2[h]; });
                // ---- the sweep: every lane meets every staged atom in ascending (row, slot), all lanes of a wavefront the same one ----
                if (wave_has) {
                    for (uint32_t j = 0; j < count; j++) {
                        const float4 cj = s_c[j];                     // one broadcast read
                        const uint32_t rj = s_row[j];
                        const float T = __fsub_rn(__fadd_rn(ci.w, cj.w), tol);
                        const float d2 = chain_d2(ci.x, ci.y, ci.z, cj.x, cj.y, cj.z);
                        if (have && rj != ri && T > 0.0f && d2 < __fmul_rn(T, T)) {
                            if (!vloss_bonded(ki, ri, s_kind[j], rj)) sum = __fadd_rn(sum, __fsub_rn(T, f32_sqrt_rn(d2)));
                        }
                    }
                }
                __syncthreads();                                      // the next pass (or round, or tile) rewrites the staging
            }
            if (have) g.clash_loss[(ct.row0 + ri) * A + (at - rr * A)] = sum;
        }
        // ---- the tile's rows: the three terms of the link to the next row ----
        if (tid < TR && ct.q0 + tid < ct.rows) {
            const uint32_t q = (uint32_t)(ct.q0 + tid);
            const uint64_t r = ct.row0 + q;
            float t[3] = {0.0f, 0.0f, 0.0f};
            float ca[3], c[3], n1[3], ca1[3];
            if (q + 1u < ct.len && vloss_link(g, r, ca, c, n1, ca1)) {   // (row r + 1 is a row of the chain: inside the arrays)
                float length, cos0, cos1;
                vloss_link_terms(g, r, ca, c, n1, ca1, &length, &cos0, &cos1, t);
                atomicAdd(&s_links, 1u);
            }
            g.link_loss[r * 3u] = t[0]; g.link_loss[r * 3u + 1u] = t[1]; g.link_loss[r * 3u + 2u] = t[2];
        }
        __syncthreads();
        if (tid < 2) {
            const uint32_t v = tid == 0 ? nq : s_links;
            if (v) atomicAdd(&g.counts[(uint64_t)ct.e * 2u + tid], (unsigned long long)v);
        }
        __syncthreads();                                              // the next tile rewrites the query list and the counters
    }
}

template <bool PACKED>
__global__ __launch_bounds__(BLOCK) void k_violation_loss_grad(vloss_grad_args g, const chain_radii tab, const uint64_t* __restrict__ tile_off,
                                                               uint32_t tiles_per_entry, uint64_t n_tiles_padded) {
    __shared__ float4 s_c[VLOSS_PASS];
    __shared__ uint32_t s_row[VLOSS_PASS];
    __shared__ float s_w[VLOSS_PASS];
    __shared__ uint8_t s_kind[VLOSS_PASS];
    __shared__ float4 q_c[VIOL_TILE_SLOTS];
    __shared__ uint16_t q_at[VIOL_TILE_SLOTS];
    __shared__ uint8_t q_kind[VIOL_TILE_SLOTS];
    __shared__ float s_link[VIOL_MAX_TILE_ROWS * VLOSS_LINK_TERMS * 3];   // a row's eight link terms: N 0 .. 2, CA 3 .. 4, C 5 .. 7
    __shared__ uint32_t s_wave[VLOSS_STEP / 64], s_nq;
    const uint32_t tid = threadIdx.x;
    const uint32_t A = g.A;
    const uint32_t TR = viol_tile_rows(A);
    const float tol = g.tolerance;
    const uint64_t n_tiles = chain_tile_count<PACKED>(tile_off, g.n, n_tiles_padded);
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const chain_tile<PACKED> ct(tile_off, g.n, tiles_per_entry, g.bound, g.L, tile, TR);
        if (tid == 0) s_nq = 0;
        // ---- the link terms of the tile's rows, a lane a row: link r - 1 for N and CA, link r for CA and C ----
        if (tid < TR && ct.q0 + tid < ct.len) {
            const uint32_t q = (uint32_t)(ct.q0 + tid);
            const uint64_t r = ct.row0 + q;
            float* s = s_link + tid * (VLOSS_LINK_TERMS * 3u);
            float t[7][3];
#pragma unroll
            for (uint32_t x = 0; x < VLOSS_LINK_TERMS * 3u; x++) s[x] = 0.0f;
            if (q >= 1u) {
                vloss_link_grad(g, r - 1u, t);
#pragma unroll
                for (int x = 0; x < 3; x++) { s[x] = -t[0][x]; s[3 + x] = t[3][x]; s[6 + x] = t[5][x]; s[9 + x] = t[6][x]; }
            }
            if (q + 1u < ct.len) {                                    // (row r + 1 is a row of the chain: inside the arrays)
                vloss_link_grad(g, r, t);
#pragma unroll
                for (int x = 0; x < 3; x++) { s[12 + x] = t[1][x]; s[15 + x] = t[0][x]; s[18 + x] = t[2][x]; s[21 + x] = t[4][x]; }
            }
        }
        __syncthreads();
        // ---- the tile's atoms, compacted in any order; every slot that is none is written here, every atom at the end of its round ----
        chain_tile_slots(TR, A, ct.q0, [&](uint32_t x, uint32_t rr, uint32_t a, uint64_t q) __attribute__((always_inline)) {
            if (q < ct.rows) {
                float4 c; uint32_t kind;
                if (q < ct.len && vloss_atom(g, tab, ct.row0 + q, a, &c, &kind)) {
                    const uint32_t i = atomicAdd(&s_nq, 1u);          // (< VIOL_TILE_SLOTS: one slot per slot of the tile)
                    q_c[i] = c; q_at[i] = (uint16_t)x; q_kind[i] = (uint8_t)kind;
                } else {
                    float gx = 0.0f, gy = 0.0f, gz = 0.0f;            // no clash atom, but it may be a link atom
                    if (q < ct.len) vloss_add_link(g, s_link + rr * (VLOSS_LINK_TERMS * 3u), a, &gx, &gy, &gz);
                    float* o = g.grad + ((ct.row0 + q) * A + a) * 3u;
                    o[0] = gx; o[1] = gy; o[2] = gz;
                }
            }
        });
        __syncthreads();
        const uint32_t nq = s_nq;
        for (uint32_t base = 0; base < nq; base += BLOCK) {
            const uint32_t qi = base + tid;
            const bool have = qi < nq;
            const bool wave_has = base + (tid & ~63u) < nq;
            const float4 ci = have ? q_c[qi] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            const uint32_t at = have ? q_at[qi] : 0u, ki = have ? q_kind[qi] : 0u;
            const uint32_t rr = chain_div_a(at, A);
            const uint32_t ri = (uint32_t)ct.q0 + rr;
            const uint64_t oi = (ct.row0 + ri) * A + (at - rr * A);   // the query atom's slot of the arrays
            const float wi = have ? g.w_clash[oi] : 0.0f;
            float gx = 0.0f, gy = 0.0f, gz = 0.0f;                    // live across the passes: they ascend
            for (uint32_t r0 = 0; r0 < ct.len;) {
                float4 c2[VLOSS_STEP / BLOCK]; uint32_t k2[VLOSS_STEP / BLOCK], row2[VLOSS_STEP / BLOCK], a2[VLOSS_STEP / BLOCK];
                const uint32_t count = chain_stage_slots_ordered<VLOSS_PASS, VLOSS_STEP>(
                    s_wave, A, ct.len, &r0,
                    [&](uint32_t r, uint32_t a, uint32_t h) __attribute__((always_inline)) {
                        row2[h] = r; a2[h] = a;
                        return vloss_atom(g, tab, ct.row0 + r, a, &c2[h], &k2[h]);
                    },
                    [&](uint32_t h, uint32_t i) __attribute__((always_inline)) {
                        s_c[i] = c2[h]; s_row[i] = row2[h]; s_kind[i] = (uint8_t)k2[h];
                        s_w[i] = g.w_clash[(ct.row0 + row2[h]) * A + a2[h]];
                    });
                if (wave_has) {
                    for (uint32_t j = 0; j < count; j++) {
                        const float4 cj = s_c[j];                     // one broadcast read
                        const uint32_t rj = s_row[j];
                        const float T = __fsub_rn(__fadd_rn(ci.w, cj.w), tol);
                        const float d2 = chain_d2(ci.x, ci.y, ci.z, cj.x, cj.y, cj.z);
                        if (have && rj != ri && T > 0.0f && d2 < __fmul_rn(T, T)) {
                            const float d = f32_sqrt_rn(d2);
                            // coincident atoms have no direction, and relu has the subgradient 0 at 0
                            if (!vloss_bonded(ki, ri, s_kind[j], rj) && d != 0.0f && __fsub_rn(T, d) != 0.0f) {
                                const float w = __fadd_rn(wi, s_w[j]);
                                gx = __fadd_rn(gx, __fmul_rn(w, -__fdiv_rn(__fsub_rn(ci.x, cj.x), d)));
                                gy = __fadd_rn(gy, __fmul_rn(w, -__fdiv_rn(__fsub_rn(ci.y, cj.y), d)));
                                gz = __fadd_rn(gz, __fmul_rn(w, -__fdiv_rn(__fsub_rn(ci.z, cj.z), d)));
                            }
                        }
                    }
                }
                __syncthreads();                                      // the next pass (or round, or tile) rewrites the staging
            }
            if (have) {
                vloss_add_link(g, s_link + rr * (VLOSS_LINK_TERMS * 3u), at - rr * A, &gx, &gy, &gz);
                float* o = g.grad + oi * 3u;
                o[0] = gx; o[1] = gy; o[2] = gz;
            }
        }
        __syncthreads();                                              // the next tile rewrites the query list and the link terms
    }
}

}  // namespace fcz
