// fcz_dssp.h -- dense tensors -> backbone hydrogen bonds and DSSP secondary structure (Kabsch & Sander 1983) on the device: the four
// H-bond columns of DSSP as tables (acc_index / acc_energy / don_index / don_energy [rows][2]) and the labels ss [rows] uint8 with
// ss_mask [rows] uint8. The reference has no such output (Foldcomp::decompress, src/foldcomp.cpp:779, ends at a flat
// vector<AtomCoordinate>); the calls stand beside fcz_knn_dev / fcz_lddt_dev and read what fcz_dense_dev / fcz_dense_packed_dev write
// (include/fcz_hip.h, fcz_hbond_dev).
//
// The contract (include/fcz_hip.h): a BACKBONE ROW lies inside its chain, has its mask set at N, CA, C and O and twelve finite
// coordinates there. All arithmetic is float32, every operation rounded, no FMA; d2 = (dx*dx + dy*dy) + dz*dz and d its correctly
// rounded root (fcz_knn's d2). A candidate's key is (~bits of E << 32) | row: E < 0 has its sign bit set, so the complement orders as
// E does, and the row makes the order total -- the tables do not depend on the order the candidates are met in.
//
//   k_hbond<PACKED>       the shape of k_lddt: persistent blocks over QUERY TILES of CHAIN_TILE = 256 rows of one chain, a lane per
//                         row (fcz_chains.h). A lane keeps its own N, H, CA, C, O in registers. The chain's backbone rows are
//                         staged in LDS in passes of HBOND_PASS chain rows: SoA N, H, CA, C, O (15 floats) and the compacted row
//                         number with "has an amide hydrogen" in bit 31 -- 64 bytes a row; H is computed once per row there, not
//                         per pair. Every lane sweeps the pass: one broadcast LDS read of the candidate's CA and row, eight float
//                         operations and ONE compare (d2(CA, CA) < 81). Only when some lane of the wavefront passes does the
//                         wavefront read the other twelve floats and pay for the energies, in both directions at once: the lane as
//                         donor with the candidate as acceptor, and the candidate as donor with the lane as acceptor. A lane keeps
//                         two two-entry lists of keys in registers. A wavefront without a backbone row skips the sweep and keeps
//                         the barriers.
//                         HBOND_PASS = 480 rows is 30 KiB of LDS a block (and the counter's word), so five blocks (20 wavefronts,
//                         five per SIMD) share a CU's 160 KiB, as for k_lddt -- 512 rows would be 32 KiB and that word, and the
//                         fifth block would no longer fit. Five wavefronts per SIMD may hold 96 VGPRs each: the padded form
//                         compiles to 74 and gets them, the packed form to 100 (the tile search's 64-bit state stays live) and
//                         runs four (`make asm` prints both). 1024 rows would be 64 KiB and two blocks. Chains of up to 480
//                         residues, most there are, take one pass; a longer chain pays three barriers per further pass.
//                         No L x L array is written: HBM sees the 48 bytes of a backbone row and 32 bytes of tables.
//                         Padded form: every row of the entry is written, -1 / 0 where it has no partner.
//   k_dssp_flags<PACKED>  a lane per row: bit 0 backbone row, bit 1 NO break behind the row, bit 2 the CA bend at the row is above 70
//                         degrees (rows r - 2, r, r + 2 backbone rows of the chain), into a per-row scratch byte; ss_mask = bit 0.
//   k_dssp_labels<PACKED> a lane per row, from the flags and the ACCEPTOR table alone (no coordinate, no energy is recomputed): every
//                         DSSP rule is local, so a lane recomputes what it needs from neighbouring table entries (dssp_label).
//                         Turns look at most 5 rows ahead. A row's bridge partners are among acc[r], acc[r] + 1, acc[r + 1] and
//                         acc[r + 1] + 1; a ladder has two bridges when the bridge one step along it exists; a bulge link is
//                         searched in the 5 x 5 window of gaps at a ladder's end. O(rows), not hot, no atomics, no scratch but the
//                         flags. dssp_label is integer code and compiles for the host as well.
//   k_chain_fill<hbond_fill_args>, k_chain_fill<label_fill_args>   (fcz_chains.h) packed form only, in front of the sweeps: -1 / 0
//                         (tables) or 0 / 0 (labels) into every row that no chain is seen to cover (chain_covers: a covered row it
//                         misses is rewritten by the sweep behind it).
//
// Every index that scales with rows * A is 64-bit. A chain's range is clamped to the R rows that exist and a range that runs
// backwards is empty (chain_range), so no read leaves the inputs whatever row_off holds; an index read from an acceptor table is only
// compared or checked against the chain's range before a row is read through it.
#pragma once
#include "fcz_chains.h"

namespace fcz {

constexpr uint32_t HBOND_PASS = 480;        // chain rows staged per candidate pass: 30 KiB of LDS
constexpr uint32_t DSSP_MAX_ROWS = 0x7FFFFFFFu;   // int32 indices, and bit 31 of a staged row number is taken
constexpr uint64_t HB_NONE = ~0ull;         // no partner: above every key
constexpr uint32_t HB_HAS_H = 1u << 31;
constexpr uint8_t DSSP_PRO = 14;            // aatype of proline

enum { DSSP_BB = 1, DSSP_LINK = 2, DSSP_BEND = 4 };                    // the bits of a row's flags
enum { SS_LOOP = 0, SS_H, SS_B, SS_E, SS_G, SS_I, SS_T, SS_S };        // "-HBEGITS"

struct dssp_args {
    const float* pos; const uint8_t* mask; const uint8_t* aatype;      // aatype may be NULL: no row is proline
    const uint32_t* bound;                  // padded: length [n] or NULL; packed: row_off [n + 1]
    uint32_t n, L;                          // padded: rows per entry; packed: L = R, the rows of the arrays
    uint32_t A, o_slot;
    int32_t* acc_index; float* acc_energy; int32_t* don_index; float* don_energy;   // k_hbond writes all four, k_dssp_labels reads acc_*
    uint8_t* flags;                         // k_dssp_flags -> k_dssp_labels
    uint8_t* ss; uint8_t* ss_mask;
};

struct bb_row { float n[3], ca[3], c[3], o[3]; };

// N, CA, C, O of array row r -> true when the row is a backbone row (four masks set, twelve finite values)
__device__ __forceinline__ bool dssp_backbone(const dssp_args& g, uint64_t r, bb_row* b) {
    const uint8_t* m = g.mask + r * g.A;
    if (m[0] == 0 || m[1] == 0 || m[2] == 0 || m[g.o_slot] == 0) return false;
    const float* p = g.pos + r * g.A * 3u;
    const float* po = p + g.o_slot * 3u;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        b->n[k] = p[k]; b->ca[k] = p[3 + k]; b->c[k] = p[6 + k]; b->o[k] = po[k];
        ok = ok && isfinite(b->n[k]) && isfinite(b->ca[k]) && isfinite(b->c[k]) && isfinite(b->o[k]);
    }
    return ok;
}

__device__ __forceinline__ float dssp_d(const float* a, const float* b) { return f32_sqrt_rn(chain_d2(a, b)); }

// the amide hydrogen of row q (> 0 rows into its chain, a backbone row b) -> true when it has one
__device__ __forceinline__ bool dssp_amide_h(const dssp_args& g, uint64_t row0, uint64_t q, const bb_row& b, float* h) {
    if (q == 0 || (g.aatype && g.aatype[row0 + q] == DSSP_PRO)) return false;
    bb_row p;
    if (!dssp_backbone(g, row0 + q - 1, &p) || dssp_d(p.c, b.n) > 2.5f) return false;
    const float d = dssp_d(p.c, p.o);
    if (d == 0.0f) return false;
#pragma unroll
    for (int k = 0; k < 3; k++) h[k] = __fadd_rn(b.n[k], f32_div_rn(__fsub_rn(p.c[k], p.o[k]), d));
    return true;
}

// the Kabsch-Sander energy of the donor's N-H and the acceptor's C=O
__device__ __forceinline__ float dssp_energy(const float* n, const float* h, const float* c, const float* o) {
    const float dON = dssp_d(o, n), dCH = dssp_d(c, h), dOH = dssp_d(o, h), dCN = dssp_d(c, n);
    if (dON < 0.5f || dCH < 0.5f || dOH < 0.5f || dCN < 0.5f) return -9.9f;
    const float s = __fsub_rn(__fsub_rn(__fadd_rn(f32_div_rn(1.0f, dON), f32_div_rn(1.0f, dCH)), f32_div_rn(1.0f, dOH)), f32_div_rn(1.0f, dCN));
    const float e = __fmul_rn(27.888f, s);
    return e < -9.9f ? -9.9f : e;
}

__device__ __forceinline__ uint64_t hb_key(bool counts, float e, uint32_t row) {
    return counts && e < 0.0f ? ((uint64_t)(~__float_as_uint(e)) << 32) | row : HB_NONE;   // (a NaN energy does not count)
}
__device__ __forceinline__ void hb_insert(uint64_t key, uint64_t* k0, uint64_t* k1) {
    const uint64_t a = *k0, b = *k1;
    *k0 = key < a ? key : a;
    *k1 = key < a ? a : (key < b ? key : b);
}
__device__ __forceinline__ void hb_decode(uint64_t key, uint32_t base, int32_t* idx, float* e) {
    const bool none = key == HB_NONE;
    *idx = none ? -1 : (int32_t)(base + (uint32_t)key);
    *e = none ? 0.0f : __uint_as_float(~(uint32_t)(key >> 32));
}

// what a fill in front of k_hbond (the four tables) and in front of k_dssp_flags (the labels) works on: k_chain_fill picks the empty
// row by the type
struct hbond_fill_args : dssp_args {};
struct label_fill_args : dssp_args {};
__device__ __forceinline__ void chain_empty_row(const hbond_fill_args& g, uint64_t r) {
    for (uint32_t s = 0; s < 2; s++) {
        g.acc_index[r * 2 + s] = -1; g.acc_energy[r * 2 + s] = 0.0f; g.don_index[r * 2 + s] = -1; g.don_energy[r * 2 + s] = 0.0f;
    }
}
__device__ __forceinline__ void chain_empty_row(const label_fill_args& g, uint64_t r) { g.ss[r] = 0; g.ss_mask[r] = 0; }

template <bool PACKED>
__global__ __launch_bounds__(BLOCK) void k_hbond(dssp_args g, const uint64_t* __restrict__ tile_off, uint32_t tiles_per_entry, uint64_t n_tiles_padded) {
    __shared__ float s_n[3][HBOND_PASS], s_h[3][HBOND_PASS], s_ca[3][HBOND_PASS], s_c[3][HBOND_PASS], s_o[3][HBOND_PASS];
    __shared__ uint32_t s_j[HBOND_PASS];
    __shared__ uint32_t s_count;
    const uint32_t tid = threadIdx.x;
    const uint64_t n_tiles = chain_tile_count<PACKED>(tile_off, g.n, n_tiles_padded);
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const chain_tile<PACKED> ct(tile_off, g.n, tiles_per_entry, g.bound, g.L, tile, CHAIN_TILE);
        const uint64_t q = ct.q0 + tid;                               // this lane's row of the chain
        bb_row me{};
        float my_h[3] = {0.0f, 0.0f, 0.0f};
        const bool active = q < ct.len && dssp_backbone(g, ct.row0 + q, &me);
        const bool has_h = active && dssp_amide_h(g, ct.row0, q, me, my_h);
        const uint32_t qj = (uint32_t)q;
        uint64_t acc0 = HB_NONE, acc1 = HB_NONE, don0 = HB_NONE, don1 = HB_NONE;
        for (uint32_t c0 = 0; c0 < ct.len;) {
            const uint32_t count = chain_stage_rows<HBOND_PASS>(&s_count, ct.len, &c0, [&](uint64_t r, chain_slots slots) __attribute__((always_inline)) {
                bb_row b;
                if (dssp_backbone(g, ct.row0 + r, &b)) {
                    float h[3] = {0.0f, 0.0f, 0.0f};
                    const bool hh = dssp_amide_h(g, ct.row0, r, b, h);
                    const uint32_t i = slots.next();
#pragma unroll
                    for (int k = 0; k < 3; k++) { s_n[k][i] = b.n[k]; s_h[k][i] = h[k]; s_ca[k][i] = b.ca[k]; s_c[k][i] = b.c[k]; s_o[k][i] = b.o[k]; }
                    s_j[i] = (uint32_t)r | (hh ? HB_HAS_H : 0u);
                }
            });
            if (__any(active)) {
                for (uint32_t c = 0; c < count; c++) {
                    const uint32_t jw = s_j[c], j = jw & ~HB_HAS_H;
                    const float cca[3] = {s_ca[0][c], s_ca[1][c], s_ca[2][c]};
                    const bool near = active && j != qj && chain_d2(cca, me.ca) < 81.0f;
                    if (__any(near)) {
                        const bool as_donor = near && has_h && j + 1u != qj;              // the lane's N-H onto the candidate's C=O (j != i - 1)
                        const bool as_acceptor = near && (jw & HB_HAS_H) != 0u && qj + 1u != j;   // the candidate's N-H onto the lane's C=O
                        float e1 = 0.0f, e2 = 0.0f;
                        if (__any(as_donor)) {
                            const float cc[3] = {s_c[0][c], s_c[1][c], s_c[2][c]}, co[3] = {s_o[0][c], s_o[1][c], s_o[2][c]};
                            e1 = dssp_energy(me.n, my_h, cc, co);
                        }
                        if (__any(as_acceptor)) {
                            const float cn[3] = {s_n[0][c], s_n[1][c], s_n[2][c]}, chh[3] = {s_h[0][c], s_h[1][c], s_h[2][c]};
                            e2 = dssp_energy(cn, chh, me.c, me.o);
                        }
                        hb_insert(hb_key(as_donor, e1, j), &acc0, &acc1);
                        hb_insert(hb_key(as_acceptor, e2, j), &don0, &don1);
                    }
                }
            }
            __syncthreads();                                          // the next pass (or tile) rewrites the staging
        }
        if (q < ct.rows) {
            const uint32_t base = PACKED ? (uint32_t)ct.row0 : 0u;
            const uint64_t o = (ct.row0 + q) * 2u;
            hb_decode(acc0, base, &g.acc_index[o], &g.acc_energy[o]);
            hb_decode(acc1, base, &g.acc_index[o + 1], &g.acc_energy[o + 1]);
            hb_decode(don0, base, &g.don_index[o], &g.don_energy[o]);
            hb_decode(don1, base, &g.don_index[o + 1], &g.don_energy[o + 1]);
        }
    }
}

template <bool PACKED>
__global__ __launch_bounds__(BLOCK) void k_dssp_flags(dssp_args g, const uint64_t* __restrict__ tile_off, uint32_t tiles_per_entry, uint64_t n_tiles_padded) {
    const uint64_t n_tiles = chain_tile_count<PACKED>(tile_off, g.n, n_tiles_padded);
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const chain_tile<PACKED> ct(tile_off, g.n, tiles_per_entry, g.bound, g.L, tile, CHAIN_TILE);
        const uint64_t q = ct.q0 + threadIdx.x;
        if (q >= ct.rows) continue;
        uint8_t f = 0;
        bb_row b, o;
        if (q < ct.len && dssp_backbone(g, ct.row0 + q, &b)) {
            f = DSSP_BB;
            if (q + 1 < ct.len && dssp_backbone(g, ct.row0 + q + 1, &o) && !(dssp_d(b.c, o.n) > 2.5f)) f |= DSSP_LINK;
            if (q >= 2 && q + 2 < ct.len && dssp_backbone(g, ct.row0 + q - 2, &o)) {
                const float u[3] = {__fsub_rn(b.ca[0], o.ca[0]), __fsub_rn(b.ca[1], o.ca[1]), __fsub_rn(b.ca[2], o.ca[2])};
                if (dssp_backbone(g, ct.row0 + q + 2, &o)) {
                    const float v[3] = {__fsub_rn(o.ca[0], b.ca[0]), __fsub_rn(o.ca[1], b.ca[1]), __fsub_rn(o.ca[2], b.ca[2])};
                    const float dot = __fadd_rn(__fadd_rn(__fmul_rn(u[0], v[0]), __fmul_rn(u[1], v[1])), __fmul_rn(u[2], v[2]));
                    const float nu = f32_sqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(u[0], u[0]), __fmul_rn(u[1], u[1])), __fmul_rn(u[2], u[2])));
                    const float nv = f32_sqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(v[0], v[0]), __fmul_rn(v[1], v[1])), __fmul_rn(v[2], v[2])));
                    if (dot < __fmul_rn(0.34202015f, __fmul_rn(nu, nv))) f |= DSSP_BEND;
                }
            }
        }
        g.flags[ct.row0 + q] = f;
        g.ss_mask[ct.row0 + q] = f & DSSP_BB;
    }
}

// ---- the labels of one chain from its flags and its acceptor table: integer code, for the device and for the host ----
// flags, acc_index and acc_energy point at the chain's first row; base is what an index of the table exceeds a row of the chain by
// (padded 0, packed the chain's first row); rows of the chain are int64 so that a hostile index cannot wrap
struct dssp_view { const uint8_t* flags; const int32_t* acc_index; const float* acc_energy; int64_t base, len; };

__host__ __device__ inline bool dv_in(const dssp_view& v, int64_t r) { return r >= 0 && r < v.len; }
__host__ __device__ inline bool dv_bond(const dssp_view& v, int64_t d, int64_t a) {
    if (!dv_in(v, d) || !dv_in(v, a)) return false;
    for (int s = 0; s < 2; s++)
        if ((int64_t)v.acc_index[d * 2 + s] - v.base == a && v.acc_energy[d * 2 + s] < -0.5f) return true;
    return false;
}
// no break behind any of a .. b - 1
__host__ __device__ inline bool dv_no_break(const dssp_view& v, int64_t a, int64_t b) {
    if (a < 0 || b >= v.len || a > b) return false;
    for (int64_t r = a; r < b; r++)
        if (!(v.flags[r] & DSSP_LINK)) return false;
    return true;
}
__host__ __device__ inline bool dv_turn(const dssp_view& v, int n, int64_t i) { return dv_bond(v, i + n, i) && dv_no_break(v, i, i + n); }
__host__ __device__ inline bool dv_helix_start(const dssp_view& v, int n, int64_t i) { return dv_turn(v, n, i - 1) && dv_turn(v, n, i); }
__host__ __device__ inline bool dv_is_h(const dssp_view& v, int64_t r) {
    for (int64_t i = r - 3; i <= r; i++)
        if (dv_helix_start(v, 4, i)) return true;
    return false;
}
// type 0 parallel, 1 antiparallel; i < j
__host__ __device__ inline bool dv_bridge(const dssp_view& v, int type, int64_t i, int64_t j) {
    if (i < 1 || j < i + 3 || j + 1 >= v.len) return false;
    if (!dv_no_break(v, i - 1, i + 1) || !dv_no_break(v, j - 1, j + 1)) return false;
    if (type == 0) return (dv_bond(v, i + 1, j) && dv_bond(v, j, i - 1)) || (dv_bond(v, j + 1, i) && dv_bond(v, i, j - 1));
    return (dv_bond(v, i + 1, j - 1) && dv_bond(v, j + 1, i - 1)) || (dv_bond(v, j, i) && dv_bond(v, i, j));
}
// (ie, je) the last bridge of a ladder, (ib, jb) the first of another of the same type, and a bulge between them
__host__ __device__ inline bool dv_link(const dssp_view& v, int type, int64_t ie, int64_t je, int64_t ib, int64_t jb) {
    const int64_t s = type ? -1 : 1, gi = ib - ie, gj = (jb - je) * s;
    if (!(gi > 0 && gi < 6 && gj > 0 && gj < 6 && (gi < 3 || gj < 3))) return false;
    if (!dv_bridge(v, type, ie, je) || dv_bridge(v, type, ie + 1, je + s)) return false;
    if (!dv_bridge(v, type, ib, jb) || dv_bridge(v, type, ib - 1, jb - s)) return false;
    return dv_no_break(v, ie, ib) && (type ? dv_no_break(v, jb, je) : dv_no_break(v, je, jb));
}
// candidate k (0 .. 3) for a bridge partner of row u: parallel acc[u + 1], acc[u] + 1; antiparallel acc[u + 1] + 1, acc[u]
__host__ __device__ inline int64_t dv_partner(const dssp_view& v, int type, int64_t u, int k) {
    const int64_t d = k < 2 ? u + 1 : u;
    if (!dv_in(v, d)) return -1;
    return (int64_t)v.acc_index[d * 2 + (k & 1)] - v.base + ((k < 2) == (type == 1) ? 1 : 0);
}
// -> 0: row r is in no bridge and no bulge, 1: B, 2: E
__host__ __device__ inline int dv_sheet(const dssp_view& v, int64_t r) {
    if (!dv_in(v, r)) return 0;
    bool bridged = false;
    for (int type = 0; type < 2; type++) {
        const int64_t s = type ? -1 : 1;
        for (int k = 0; k < 4; k++) {                                 // the row's own bridges
            const int64_t p = dv_partner(v, type, r, k), i = p < r ? p : r, j = p < r ? r : p;
            if (!dv_bridge(v, type, i, j)) continue;
            bridged = true;
            if (dv_bridge(v, type, i - 1, j - s) || dv_bridge(v, type, i + 1, j + s)) return 2;
            for (int64_t gi = 1; gi < 6; gi++)
                for (int64_t gj = 1; gj < 6; gj++)
                    if ((gi < 3 || gj < 3) && (dv_link(v, type, i, j, i + gi, j + s * gj) || dv_link(v, type, i - gi, j - s * gj, i, j))) return 2;
        }
        for (int64_t a = r - 4; a < r; a++)                           // the row inside a bulge: a < r < b on one strand
            for (int k = 0; k < 4; k++) {
                const int64_t p = dv_partner(v, type, a, k);
                if (p > a && dv_bridge(v, type, a, p))                // the i strand: (a, p) ends a ladder, (b, ..) begins one
                    for (int64_t b = r + 1; b < a + 6; b++)
                        for (int64_t gj = 1; gj < 6; gj++)
                            if (dv_link(v, type, a, p, b, p + s * gj)) return 2;
                if (p >= 0 && p < a && dv_bridge(v, type, p, a))      // the j strand: parallel (p, a) ends and (.., b) begins, antiparallel the reverse
                    for (int64_t b = r + 1; b < a + 6; b++)
                        for (int64_t gi = 1; gi < 6; gi++)
                            if (type == 0 ? dv_link(v, type, p, a, p + gi, b) : dv_link(v, type, p - gi, b, p, a)) return 2;
            }
    }
    return bridged ? 1 : 0;
}
__host__ __device__ inline bool dv_is_hbe(const dssp_view& v, int64_t r) { return dv_is_h(v, r) || dv_sheet(v, r) != 0; }
__host__ __device__ inline bool dv_is_g(const dssp_view& v, int64_t r) {
    for (int64_t i = r - 2; i <= r; i++)
        if (dv_helix_start(v, 3, i) && !dv_is_hbe(v, i) && !dv_is_hbe(v, i + 1) && !dv_is_hbe(v, i + 2)) return true;
    return false;
}
__host__ __device__ inline bool dv_is_i(const dssp_view& v, int64_t r) {
    for (int64_t i = r - 4; i <= r; i++) {
        if (!dv_helix_start(v, 5, i)) continue;
        bool free_rows = true;
        for (int64_t x = i; x < i + 5 && free_rows; x++) free_rows = !dv_is_hbe(v, x) && !dv_is_g(v, x);
        if (free_rows) return true;
    }
    return false;
}
__host__ __device__ inline uint8_t dssp_label(const dssp_view& v, int64_t r) {
    if (!(v.flags[r] & DSSP_BB)) return SS_LOOP;                       // (every rule below needs the row unbroken from a neighbour)
    if (dv_is_h(v, r)) return SS_H;
    const int sheet = dv_sheet(v, r);
    if (sheet) return sheet == 2 ? SS_E : SS_B;
    if (dv_is_g(v, r)) return SS_G;
    if (dv_is_i(v, r)) return SS_I;
    for (int n = 3; n <= 5; n++)
        for (int k = 1; k < n; k++)
            if (dv_turn(v, n, r - k)) return SS_T;
    if ((v.flags[r] & DSSP_BEND) && dv_no_break(v, r - 2, r + 2)) return SS_S;
    return SS_LOOP;
}

template <bool PACKED>
__global__ __launch_bounds__(BLOCK) void k_dssp_labels(dssp_args g, const uint64_t* __restrict__ tile_off, uint32_t tiles_per_entry, uint64_t n_tiles_padded) {
    const uint64_t n_tiles = chain_tile_count<PACKED>(tile_off, g.n, n_tiles_padded);
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const chain_tile<PACKED> ct(tile_off, g.n, tiles_per_entry, g.bound, g.L, tile, CHAIN_TILE);
        const uint64_t q = ct.q0 + threadIdx.x;
        if (q >= ct.rows) continue;
        const dssp_view v{g.flags + ct.row0, g.acc_index + ct.row0 * 2u, g.acc_energy + ct.row0 * 2u, PACKED ? (int64_t)ct.row0 : 0, (int64_t)ct.len};
        g.ss[ct.row0 + q] = q < ct.len ? dssp_label(v, (int64_t)q) : (uint8_t)SS_LOOP;
    }
}

}  // namespace fcz
