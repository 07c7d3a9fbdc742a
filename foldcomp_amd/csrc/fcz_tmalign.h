// fcz_tmalign.h -- two sets of chains (dense tensors, padded or packed, each set in its own form) and a list of chain pairs -> per pair
// a TM-align-style structural alignment: a monotone partial map of a's residues onto b's, found by a Needleman-Wunsch dynamic programme
// that alternates with superposition, the rigid motion that lays a onto b and the TM-scores normalised by either chain
// (include/fcz_hip.h, fcz_tmalign_dev, is the contract). The reference has no such output.
//
// Everything numeric is fcz_superpose.h's and fcz_tmscore.h's: float64, every operation rounded, no FMA; a fit of an alignment is
// tm_run_seed over a source that reads pair i through the alignment (ta_src_aln), so the sums keep that file's lane order and butterfly.
// The DP is integer: q_ij = floor(65536 / (1 + d2_ij / d0^2)), G = rint(65536 g), H in int32, so its cells may be evaluated in any order.
//   the bound      |H| never leaves int32: H[i][j] <= min(i, j) * 65536 <= 2^26 for widths up to TMALIGN_MAX_WIDTH = 1024, and
//                  H[i][j] >= -i * G >= -2^30 with G <= 2^20 (gap <= TMALIGN_MAX_GAP = 16); the prefix-max operand C_k + G k stays
//                  below 2^26 + 2^30, and H - G above -2^30 - 2^20.
//
// The sites of both chains are COMPACTED into LDS once per block (float planes x, y, z and the chain-relative row of every site, 14
// bytes a site), so a site's number is its index and every source below is indexed by a's site number. An alignment is int16 per a-site
// (the site of b, or -1), kept in LDS per wavefront.
//
//   ta_dp              one wavefront, row by row over a's sites. Lane l owns the columns l, l + 64, ..; the previous row of H stays in
//                      VGPRs (the chunk loop is unrolled over the 16 chunks of the largest width, so the indices are constants).
//                      Per row: p = R a_i + t once (wave-uniform), per cell d2, q, C = max(diag + q, up - G), then
//                      H[i][j] = max_{k <= j}(C_k + G k) - G j as an inclusive max-scan over the 64 lanes (__shfl_up, six steps) with a
//                      carry between chunks. Two direction bits per cell (diagonal, up, left, in the order of preference) are packed
//                      into one 32-bit word per lane and row -- 2 bits x 16 chunks -- and go to the wavefront's scratch in the ctx, 256
//                      bytes a row. The traceback is wave-uniform: a row's 64 words are loaded by the lanes that wrote them (the next
//                      row up is prefetched) and the cell's word is broadcast with __shfl.
//   k_ta_count         a wavefront per pair: status, Sa, Sb and the pair's work items, one per WAVES_PER_BLOCK seeds; scanned.
//   k_ta_search        persistent blocks over contiguous ranges of the items, run twice: phase 0 the gapless seeds (one Kabsch each),
//                      phase 1 the seeds that run the DP iteration (the best gapless one -- found from phase 0's scores -- and the
//                      fragment pairs). The four wavefronts of a block take four consecutive seeds of ONE pair and share its staged
//                      sites. A seed leaves ONE double, its best candidate's tm.
//   k_ta_final         a block per pair: wavefront 0 picks the winner (largest tm, lowest seed) and runs it again keeping the
//                      alignment and fit of its best candidate; then the four wavefronts share fcz_tmscore_dev's full search over the
//                      aligned pairs, and the outputs are written.
//   k_ta_dp            fcz_tmalign_dp_dev: a block per pair, one DP from the caller's transform, map and aligned written. The block's four
//                      wavefronts stage the pair and clear map; the DP itself runs on wavefront 0 while the other three wait at the
//                      barrier, and the grid is at most four blocks a CU. It is a secondary entry point; nobody has measured it.
#pragma once
#include "fcz_tmscore.h"

namespace fcz {

constexpr uint32_t TMALIGN_MAX_WIDTH = 1024;                    // rows of a chain (wa, wb): the LDS planes and int16 alignments
constexpr uint32_t TMALIGN_CHUNKS = TMALIGN_MAX_WIDTH / WAVE;   // columns a lane owns at the largest width: 2 bits each in one word
constexpr double TMALIGN_MAX_GAP = 16.0;
constexpr uint32_t TMALIGN_MAX_GAPS = 4;
constexpr uint32_t TMALIGN_MAX_ROUNDS = 64;                     // dp_rounds and refine
constexpr int32_t TMALIGN_Q = 65536;
static_assert(TMALIGN_CHUNKS == 16, "a lane's direction bits of one row fill one 32-bit word");

struct tmalign_set {
    const float* pos; const uint8_t* mask;
    const uint32_t* length; const uint32_t* row_off;    // row_off != NULL: packed
    uint32_t n, rows;                                   // rows: L (padded) or R (packed)
};

struct tmalign_args {
    tmalign_set a, b;
    const int32_t* pairs; uint32_t m, wa, wb, A, slot;
    uint32_t fragments, refine, dp_rounds, n_gaps; int32_t G[TMALIGN_MAX_GAPS];
    uint32_t levels, iterations;
    // outputs, all but rot / trans may be NULL
    float* rot; float* trans; float* tm; float* tm_a; float* tm_b; int32_t* aligned; float* rmsd; int32_t* sites_a; int32_t* sites_b;
    int32_t* seed; int32_t* status; int32_t* map; float* dev;
    // scratch
    uint32_t* nsites;                       // [2 m]: Sa, Sb (0 for a pair with a status)
    uint64_t* item_off;                     // [m + 1]
    double* score; uint64_t score_cap;
    uint32_t* dir; uint32_t dir_slots;      // dir_slots wavefront slots of wa * 64 words
    unsigned long long* work;               // [2] or NULL: the DPs of the iteration and their cells, counted for fcz_tmalign_last_work
    // fcz_tmalign_dp_dev
    const float* rot_in; const float* trans_in;
};

// ---- the seed schedule (host and device) ---------------------------------------------------------------------------------------------
__host__ __device__ inline uint32_t ta_min_overlap(uint32_t lmin) {
    const uint32_t h = lmin / 2u, f = lmin < 5u ? lmin : 5u;
    return h > f ? h : f;
}
__host__ __device__ inline uint32_t ta_frag_len(uint32_t lmin) {
    uint32_t f = lmin / 5u;
    f = f < 8u ? 8u : f > 32u ? 32u : f;
    return f < lmin ? f : lmin;
}
// the starts 0, f, 2 f, .. while start + f <= S, then S - f if it is not the last one taken (f <= S)
__host__ __device__ inline uint32_t ta_starts(uint32_t S, uint32_t f) {
    const uint32_t k = (S - f) / f + 1u;
    return (k - 1u) * f == S - f ? k : k + 1u;
}
__host__ __device__ inline uint32_t ta_start_at(uint32_t S, uint32_t f, uint32_t s) { return s * f + f <= S ? s * f : S - f; }
__host__ __device__ inline uint32_t ta_gapless_count(uint32_t Sa, uint32_t Sb) {
    const uint32_t lmin = Sa < Sb ? Sa : Sb;
    return lmin ? Sa + Sb - 2u * ta_min_overlap(lmin) + 1u : 0u;
}
__host__ __device__ inline uint64_t ta_seed_count(uint32_t Sa, uint32_t Sb, uint32_t fragments) {
    const uint32_t lmin = Sa < Sb ? Sa : Sb;
    if (lmin == 0u) return 0;
    const uint32_t f = ta_frag_len(lmin);
    return (uint64_t)ta_gapless_count(Sa, Sb) + 1u + (fragments ? (uint64_t)ta_starts(Sa, f) * ta_starts(Sb, f) : 0u);
}
// seed -> kind (0 gapless, 1 the best gapless seed's DP iteration, 2 a fragment pair), the shift k (kind 0), the first site in a and
// in b and the number of pairs (kinds 0 and 2)
__host__ __device__ inline void ta_seed_what(uint32_t Sa, uint32_t Sb, uint64_t seed, int32_t* kind, int32_t* shift, uint32_t* ia, uint32_t* ib, uint32_t* np) {
    const uint32_t lmin = Sa < Sb ? Sa : Sb, ng = ta_gapless_count(Sa, Sb);
    if (seed < ng) {
        const int32_t k = (int32_t)ta_min_overlap(lmin) - (int32_t)Sa + (int32_t)seed;
        const uint32_t lo = k < 0 ? (uint32_t)-k : 0u, hi = (int64_t)Sb - k < (int64_t)Sa ? (uint32_t)((int64_t)Sb - k) : Sa;
        *kind = 0; *shift = k; *ia = lo; *ib = (uint32_t)((int32_t)lo + k); *np = hi - lo;
    } else if (seed == ng) {
        *kind = 1; *shift = 0; *ia = 0; *ib = 0; *np = 0;
    } else {
        const uint32_t f = ta_frag_len(lmin), nb = ta_starts(Sb, f);
        const uint64_t s = seed - ng - 1u;
        *kind = 2; *ia = ta_start_at(Sa, f, (uint32_t)(s / nb)); *ib = ta_start_at(Sb, f, (uint32_t)(s % nb)); *np = f;
        *shift = (int32_t)*ib - (int32_t)*ia;
    }
}
// the most seeds a pair can have when its chains have at most wa and wb sites (host: sizes the scratch). The count grows with the
// longer chain while the shorter one is fixed, so the longer one is taken at its width
inline uint64_t ta_seed_bound(uint32_t wa, uint32_t wb, uint32_t fragments) {
    uint64_t top = 0;
    const uint32_t lo = wa < wb ? wa : wb;
    for (uint32_t s = 0; s <= lo; s++) {
        const uint64_t x = ta_seed_count(s, wb, fragments), y = ta_seed_count(wa, s, fragments);
        top = x > top ? x : top; top = y > top ? y : top;
    }
    return top;
}

// ---- a pair's chains -------------------------------------------------------------------------------------------------------------------
// chain idx of a set: its first row and its rows -> status 0, 1 (more rows than the width) or 2 (no such chain); nothing is read for 2
__device__ __forceinline__ uint32_t ta_range(const tmalign_set& s, uint32_t width, int32_t idx, uint64_t* row0, uint32_t* len) {
    *row0 = 0; *len = 0;
    if (idx < 0 || (uint32_t)idx >= s.n) return 2u;
    uint64_t r0; uint32_t n;
    if (s.row_off) {
        uint32_t lo = s.row_off[idx], hi = s.row_off[idx + 1];
        if (lo > s.rows) lo = s.rows;
        if (hi > s.rows) hi = s.rows;
        r0 = lo; n = hi > lo ? hi - lo : 0u;
    } else {
        const uint32_t le = s.length ? s.length[idx] : s.rows;
        r0 = (uint64_t)idx * s.rows; n = le < s.rows ? le : s.rows;
    }
    if (n > width) return 1u;
    *row0 = r0; *len = n;
    return 0u;
}

__device__ __forceinline__ bool ta_site(const tmalign_set& s, uint32_t A, uint32_t slot, uint64_t r, float* x) {
    const uint64_t o = r * A + slot;
    if (s.mask[o] == 0) return false;
    const float* p = s.pos + o * 3u;
    x[0] = p[0]; x[1] = p[1]; x[2] = p[2];
    return isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]);
}

// what a block holds of one pair in LDS
struct ta_stage {
    float ca[3 * TMALIGN_MAX_WIDTH], cb[3 * TMALIGN_MAX_WIDTH];   // planes x, y, z by site number
    int16_t ra[TMALIGN_MAX_WIDTH], rb[TMALIGN_MAX_WIDTH];         // the chain-relative row of a site
    uint32_t S[2];
};

// one wavefront compacts one chain's sites into planes c and rows r -> their number
__device__ __forceinline__ uint32_t ta_compact(const tmalign_set& s, uint32_t A, uint32_t slot, uint64_t row0, uint32_t len, uint32_t lane, float* c, int16_t* r) {
    uint32_t base = 0;
    for (uint32_t r0 = 0; r0 < len; r0 += WAVE) {
        float x[3];
        const uint32_t row = r0 + lane;
        const bool is = row < len && ta_site(s, A, slot, row0 + row, x);
        const uint64_t m = __ballot(is);
        if (is) {
            const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            c[at] = x[0]; c[TMALIGN_MAX_WIDTH + at] = x[1]; c[2 * TMALIGN_MAX_WIDTH + at] = x[2];
            r[at] = (int16_t)row;
        }
        base += (uint32_t)__popcll(m);
    }
    return base;
}

// the whole block stages pair p (wavefront 0 chain a, wavefront 1 chain b) -> its status; ends with a barrier
__device__ __forceinline__ uint32_t ta_stage_pair(const tmalign_args& g, uint32_t p, ta_stage& st, uint32_t* len_a) {
    const uint32_t lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    uint64_t row_a, row_b; uint32_t la, lb;
    const int32_t ia = g.pairs[2u * (uint64_t)p], ib = g.pairs[2u * (uint64_t)p + 1u];
    const uint32_t sa = ta_range(g.a, g.wa, ia, &row_a, &la), sb = ta_range(g.b, g.wb, ib, &row_b, &lb);
    const uint32_t status = sa > sb ? sa : sb;
    if (status) { la = 0; lb = 0; }
    __syncthreads();                                                           // whoever read the pair before is done with it
    if (wave == 0) { const uint32_t n = ta_compact(g.a, g.A, g.slot, row_a, la, lane, st.ca, st.ra); if (lane == 0) st.S[0] = n; }
    if (wave == 1) { const uint32_t n = ta_compact(g.b, g.A, g.slot, row_b, lb, lane, st.cb, st.rb); if (lane == 0) st.S[1] = n; }
    __syncthreads();
    *len_a = la;
    return status;
}

// ---- sources: where a wavefront reads pair r (a's site r) from -----------------------------------------------------------------------
struct ta_src_aln {
    const float* ca; const float* cb; const int16_t* aln;
    __device__ __forceinline__ bool site(uint32_t r, double* a, double* b) const {
        const int32_t j = aln[r];
        if (j < 0) return false;
#pragma unroll
        for (int i = 0; i < 3; i++) { a[i] = ca[i * TMALIGN_MAX_WIDTH + r]; b[i] = cb[i * TMALIGN_MAX_WIDTH + j]; }
        return true;
    }
};
struct ta_src_shift {
    const float* ca; const float* cb; int32_t k; uint32_t Sb;
    __device__ __forceinline__ bool site(uint32_t r, double* a, double* b) const {
        const int32_t j = (int32_t)r + k;
        if (j < 0 || (uint32_t)j >= Sb) return false;
#pragma unroll
        for (int i = 0; i < 3; i++) { a[i] = ca[i * TMALIGN_MAX_WIDTH + r]; b[i] = cb[i * TMALIGN_MAX_WIDTH + j]; }
        return true;
    }
};

// ---- the dynamic programme -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int32_t ta_quant(double d2, double d0sq) {
    if (!isfinite(d2)) return 0;
    return (int32_t)floor((double)TMALIGN_Q / __dadd_rn(1.0, d2 / d0sq));
}

// one DP of a wavefront from (R, t) with gap G -> the number of aligned pairs; aln [Sa] receives the site of b or -1 for every site of a.
// dir: this wavefront's Sa * 64 words. Every lane calls it with the same arguments.
__device__ __forceinline__ uint32_t ta_dp(const float* ca, const float* cb, uint32_t Sa, uint32_t Sb, uint32_t lane, const double* R, const double* t, double d0sq,
                                          int32_t G, uint32_t* __restrict__ dir, int16_t* aln) {
    for (uint32_t i = lane; i < Sa; i += WAVE) aln[i] = -1;
    if (Sa == 0u || Sb == 0u) return 0u;
    int32_t hp[TMALIGN_CHUNKS];
#pragma unroll
    for (int c = 0; c < (int)TMALIGN_CHUNKS; c++) hp[c] = 0;
    const uint32_t cl = (Sb - 1u) / WAVE, ll = (Sb - 1u) % WAVE;              // the chunk and lane of the last column
    int32_t end_v = 0; uint32_t end_i = 0, end_j = Sb;                        // the end cell (1-based); H[0][Sb] = 0 comes first
    for (uint32_t i = 0; i < Sa; i++) {
        double a[3], p[3];
#pragma unroll
        for (int k = 0; k < 3; k++) a[k] = ca[k * TMALIGN_MAX_WIDTH + i];
#pragma unroll
        for (int k = 0; k < 3; k++)
            p[k] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(R[3 * k], a[0]), __dmul_rn(R[3 * k + 1], a[1])), __dmul_rn(R[3 * k + 2], a[2])), t[k]);
        uint32_t word = 0;
        int32_t carry = 0;                                                     // max of C_k + G k over the columns before this chunk; column 0 gives 0
        int32_t left_diag = 0;                                                 // H[i - 1][column before this chunk's first]
        int32_t last = 0;
#pragma unroll
        for (int c = 0; c < (int)TMALIGN_CHUNKS; c++) {
            if ((uint32_t)c * WAVE >= Sb) break;
            const uint32_t j = (uint32_t)c * WAVE + lane;                      // site of b; the DP column is j + 1
            int32_t q = 0;
            if (j < Sb) {
                double d[3];
#pragma unroll
                for (int k = 0; k < 3; k++) d[k] = __dsub_rn(p[k], (double)cb[k * TMALIGN_MAX_WIDTH + j]);
                q = ta_quant(__dadd_rn(__dadd_rn(__dmul_rn(d[0], d[0]), __dmul_rn(d[1], d[1])), __dmul_rn(d[2], d[2])), d0sq);
            }
            const int32_t up = hp[c];
            int32_t diag = __shfl_up(up, 1, WAVE);
            if (lane == 0) diag = left_diag;
            left_diag = __shfl(up, WAVE - 1, WAVE);
            const int32_t dq = diag + q, ug = up - G;
            const int32_t gj = G * (int32_t)(j + 1u);
            int32_t v = (dq > ug ? dq : ug) + gj;
#pragma unroll
            for (int s = 1; s < WAVE; s <<= 1) {
                const int32_t o = __shfl_up(v, s, WAVE);
                if ((int)lane >= s) v = o > v ? o : v;
            }
            v = carry > v ? carry : v;
            carry = __shfl(v, WAVE - 1, WAVE);
            const int32_t h = v - gj;
            hp[c] = h;
            word |= (h == dq ? 0u : h == ug ? 1u : 2u) << (2 * c);
            if ((uint32_t)c == cl) last = __shfl(h, ll, WAVE);
        }
        dir[(uint64_t)i * WAVE + lane] = word;
        if (last > end_v) { end_v = last; end_i = i + 1u; }
    }
    // the last row, columns 1 .. Sb - 1, in ascending order: only a strictly larger value replaces the last column's
    {
        int32_t bv = end_v; uint32_t bj = 0xFFFFFFFFu;
#pragma unroll
        for (int c = 0; c < (int)TMALIGN_CHUNKS; c++) {
            const uint32_t j = (uint32_t)c * WAVE + lane;
            if (j + 1u < Sb && hp[c] > bv) { bv = hp[c]; bj = j + 1u; }
        }
        for (int d = WAVE / 2; d > 0; d >>= 1) {
            const int32_t ov = __shfl_xor(bv, d, WAVE);
            const uint32_t oj = __shfl_xor(bj, d, WAVE);
            if (ov > bv || (ov == bv && oj < bj)) { bv = ov; bj = oj; }
        }
        if (bj != 0xFFFFFFFFu) { end_v = bv; end_i = Sa; end_j = bj; }
    }
    // traceback, wave-uniform
    uint32_t i = end_i, j = end_j, P = 0;
    uint32_t w = i ? dir[(uint64_t)(i - 1u) * WAVE + lane] : 0u;
    uint32_t wn = i > 1u ? dir[(uint64_t)(i - 2u) * WAVE + lane] : 0u;
    while (i > 0u && j > 0u) {
        const uint32_t c = (j - 1u) / WAVE, l = (j - 1u) % WAVE;
        const uint32_t d = ((uint32_t)__shfl((int32_t)w, (int)l, WAVE) >> (2u * c)) & 3u;
        if (d == 2u) { j--; continue; }
        if (d == 0u) { if (lane == 0) aln[i - 1u] = (int16_t)(j - 1u); P++; j--; }
        i--;
        w = wn;
        wn = i > 1u ? dir[(uint64_t)(i - 2u) * WAVE + lane] : 0u;
    }
    __threadfence_block();
    return P;
}

// ---- one seed ----------------------------------------------------------------------------------------------------------------------------
struct ta_params { uint32_t Sa, Sb, lmin, refine, dp_rounds, n_gaps; const int32_t* G; double d0sq; unsigned long long* work; };

struct ta_best { double tm; double R[9], t[3]; uint32_t P; };

// (3): the DP iteration from the transform cur. cur_a / prev_a: this wavefront's two alignments in LDS. KEEP: best_a receives the best
// candidate's alignment and best its fit.
template <bool KEEP>
__device__ __forceinline__ void ta_dp_iterate(const ta_stage& st, const ta_params& q, uint32_t lane, double* R, double* t, uint32_t* dir, int16_t* cur_a,
                                              int16_t* prev_a, int16_t* best_a, ta_best* best) {
    const uint32_t need = q.lmin < 3u ? q.lmin : 3u;
    for (uint32_t gi = 0; gi < q.n_gaps; gi++) {
        bool have_prev = false;
        for (uint32_t round = 0; round < q.dp_rounds; round++) {
            const uint32_t P = ta_dp(st.ca, st.cb, q.Sa, q.Sb, lane, R, t, q.d0sq, q.G[gi], dir, cur_a);
            if (lane == 0 && q.work) { atomicAdd(q.work, 1ull); atomicAdd(q.work + 1, (unsigned long long)q.Sa * q.Sb); }
            if (P < need) break;
            if (have_prev) {
                uint32_t diff = 0;
                for (uint32_t i = lane; i < q.Sa; i += WAVE) diff += cur_a[i] != prev_a[i] ? 1u : 0u;
                if (superpose_wave_count(diff) == 0u) break;
            }
            tm_best b;
            tm_run_seed<true>(ta_src_aln{st.ca, st.cb, cur_a}, q.Sa, lane, q.lmin, 0u, P, q.refine, &b);
            if (b.tm > best->tm) {
                best->tm = b.tm;
                if constexpr (KEEP) {
                    best->P = P;
#pragma unroll
                    for (int k = 0; k < 9; k++) best->R[k] = b.R[k];
#pragma unroll
                    for (int k = 0; k < 3; k++) best->t[k] = b.t[k];
                    for (uint32_t i = lane; i < q.Sa; i += WAVE) best_a[i] = cur_a[i];
                }
            }
#pragma unroll
            for (int k = 0; k < 9; k++) R[k] = b.R[k];
#pragma unroll
            for (int k = 0; k < 3; k++) t[k] = b.t[k];
            for (uint32_t i = lane; i < q.Sa; i += WAVE) prev_a[i] = cur_a[i];
            __threadfence_block();
            have_prev = true;
        }
    }
}

// the largest score among the gapless seeds, of equal ones the lowest seed (every lane gets it)
__device__ __forceinline__ uint64_t ta_top_seed(const double* score, uint64_t at, uint64_t count, uint64_t cap, uint32_t lane, double* top_out) {
    double top = -1.0; uint64_t top_seed = 0;
    for (uint64_t s = lane; s < count && at + s < cap; s += WAVE) {
        const double v = score[at + s];
        if (v > top) { top = v; top_seed = s; }
    }
    for (int d = WAVE / 2; d > 0; d >>= 1) {
        const double ov = __shfl_xor(top, d, WAVE);
        const uint64_t os = __shfl_xor(top_seed, d, WAVE);
        if (ov > top || (ov == top && os < top_seed)) { top = ov; top_seed = os; }
    }
    *top_out = top;
    return top_seed;
}

// one seed of a pair -> best (tm = -1: no candidate). gapless_top: the best gapless seed (needed by kind 1 only)
template <bool KEEP>
__device__ __forceinline__ void ta_run_seed(const ta_stage& st, const ta_params& q, uint64_t seed, uint64_t gapless_top, uint32_t lane, uint32_t* dir, int16_t* cur_a,
                                            int16_t* prev_a, int16_t* best_a, ta_best* best) {
    int32_t kind, shift; uint32_t ia, ib, np;
    ta_seed_what(q.Sa, q.Sb, seed, &kind, &shift, &ia, &ib, &np);
    best->tm = -1.0; best->P = 0;
    if (kind == 0) {
        tm_best b;
        tm_run_seed<true>(ta_src_shift{st.ca, st.cb, shift, q.Sb}, q.Sa, lane, q.lmin, 0u, np, 0u, &b);
        best->tm = b.tm;
        if constexpr (KEEP) {
            best->P = np;
#pragma unroll
            for (int k = 0; k < 9; k++) best->R[k] = b.R[k];
#pragma unroll
            for (int k = 0; k < 3; k++) best->t[k] = b.t[k];
            for (uint32_t i = lane; i < q.Sa; i += WAVE) {
                const int32_t j = (int32_t)i + shift;
                best_a[i] = j >= 0 && (uint32_t)j < q.Sb ? (int16_t)j : (int16_t)-1;
            }
            __threadfence_block();
        }
        return;
    }
    if (kind == 1) ta_seed_what(q.Sa, q.Sb, gapless_top, &kind, &shift, &ia, &ib, &np);
    // the Kabsch fit on the pairs (ia + u, ib + u), u < np: they are the shifted source's pairs numbered from ia - (its first a-site)
    const uint32_t first = shift < 0 ? (uint32_t)-shift : 0u;
    tm_sel sel;
    sel.frag = true; sel.lo = ia - first; sel.n = np; sel.cut = 0.0;
#pragma unroll
    for (int k = 0; k < 9; k++) sel.R[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) sel.t[k] = 0.0;
    double R[9], t[3];
    (void)tm_fit(ta_src_shift{st.ca, st.cb, shift, q.Sb}, q.Sa, lane, sel, R, t);
    ta_dp_iterate<KEEP>(st, q, lane, R, t, dir, cur_a, prev_a, best_a, best);
}

__device__ __forceinline__ ta_params ta_params_of(const tmalign_args& g, const ta_stage& st) {
    ta_params q;
    q.Sa = st.S[0]; q.Sb = st.S[1]; q.lmin = q.Sa < q.Sb ? q.Sa : q.Sb;
    q.refine = g.refine; q.dp_rounds = g.dp_rounds; q.n_gaps = g.n_gaps; q.G = g.G; q.work = g.work;
    const double d0 = superpose_d0(q.lmin);
    q.d0sq = __dmul_rn(d0, d0);
    return q;
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_ta_count(tmalign_args g, uint64_t* __restrict__ items) {
    const uint32_t lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    for (uint64_t c = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + wave; c < g.m; c += (uint64_t)gridDim.x * WAVES_PER_BLOCK) {
        uint64_t row_a, row_b; uint32_t la, lb;
        const uint32_t sa = ta_range(g.a, g.wa, g.pairs[2u * c], &row_a, &la), sb = ta_range(g.b, g.wb, g.pairs[2u * c + 1u], &row_b, &lb);
        uint32_t na = 0, nb = 0;
        if (sa == 0u && sb == 0u) {
            float x[3];
            for (uint64_t r = lane; r < la; r += WAVE) na += ta_site(g.a, g.A, g.slot, row_a + r, x) ? 1u : 0u;
            for (uint64_t r = lane; r < lb; r += WAVE) nb += ta_site(g.b, g.A, g.slot, row_b + r, x) ? 1u : 0u;
        }
        na = superpose_wave_count(na); nb = superpose_wave_count(nb);
        if (lane == 0) {
            g.nsites[2u * c] = na; g.nsites[2u * c + 1u] = nb;
            items[c] = (ta_seed_count(na, nb, g.fragments) + WAVES_PER_BLOCK - 1u) / WAVES_PER_BLOCK;
        }
    }
}

__global__ __launch_bounds__(BLOCK) void k_ta_search(tmalign_args g, uint32_t phase) {
    __shared__ ta_stage st;
    __shared__ int16_t s_aln[WAVES_PER_BLOCK][2][TMALIGN_MAX_WIDTH];
    const uint32_t lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    const uint64_t n_items = g.item_off[g.m];
    uint32_t staged = 0xFFFFFFFFu;
    const uint64_t per = (n_items + gridDim.x - 1u) / gridDim.x, first = (uint64_t)blockIdx.x * per;
    const uint64_t last = first + per < n_items ? first + per : n_items;
    uint32_t* dir = g.dir + ((uint64_t)blockIdx.x * WAVES_PER_BLOCK + wave) * g.wa * WAVE;
    for (uint64_t item = first; item < last; item++) {
        uint32_t p, qi;
        chain_of_tile<true>(g.item_off, g.m, 0u, item, &p, &qi);
        const uint32_t Sa = g.nsites[2u * (uint64_t)p], Sb = g.nsites[2u * (uint64_t)p + 1u];
        const uint64_t n_seeds = ta_seed_count(Sa, Sb, g.fragments), ng = ta_gapless_count(Sa, Sb);
        const uint64_t seed0 = (uint64_t)qi * WAVES_PER_BLOCK;
        // (uniform over the block) an item none of whose seeds belongs to this phase is not staged
        if (phase == 0u ? seed0 >= ng : seed0 + WAVES_PER_BLOCK <= ng) continue;
        if (staged != p) { uint32_t la; (void)ta_stage_pair(g, p, st, &la); staged = p; }
        const uint64_t seed = seed0 + wave, base = g.item_off[p] * WAVES_PER_BLOCK, at = base + seed;
        if (seed >= n_seeds || at >= g.score_cap || (phase == 0u) != (seed < ng)) continue;
        if ((uint64_t)blockIdx.x * WAVES_PER_BLOCK + wave >= g.dir_slots) continue;
        const ta_params q = ta_params_of(g, st);
        uint64_t gtop = 0;
        if (seed == ng) { double v; gtop = ta_top_seed(g.score, base, ng, g.score_cap, lane, &v); }
        ta_best best;
        ta_run_seed<false>(st, q, seed, gtop, lane, dir, s_aln[wave][0], s_aln[wave][1], nullptr, &best);
        if (lane == 0) g.score[at] = best.tm;
    }
}

// what the four wavefronts of k_ta_final hand to wavefront 0
struct ta_wave_best { double tm; double R[9], t[3]; uint64_t seed; };

__global__ __launch_bounds__(BLOCK) void k_ta_final(tmalign_args g) {
    __shared__ ta_stage st;
    __shared__ int16_t s_aln[3][TMALIGN_MAX_WIDTH];                            // current, previous, best
    __shared__ ta_wave_best s_wb[WAVES_PER_BLOCK];
    __shared__ double s_fit[13];                                               // the candidate's R, t, tm
    __shared__ uint32_t s_P, s_seed;
    const uint32_t lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    for (uint32_t p = blockIdx.x; p < g.m; p += gridDim.x) {
        uint32_t la;
        const uint32_t status = ta_stage_pair(g, p, st, &la);
        const ta_params q = ta_params_of(g, st);
        const uint64_t n_seeds = ta_seed_count(q.Sa, q.Sb, g.fragments), ng = ta_gapless_count(q.Sa, q.Sb), base = g.item_off[p] * WAVES_PER_BLOCK;
        if (wave == 0) {
            ta_best best;
            best.tm = 0.0; best.P = 0;
#pragma unroll
            for (int k = 0; k < 9; k++) best.R[k] = k % 4 == 0 ? 1.0 : 0.0;
#pragma unroll
            for (int k = 0; k < 3; k++) best.t[k] = 0.0;
            for (uint32_t i = lane; i < TMALIGN_MAX_WIDTH; i += WAVE) s_aln[2][i] = -1;
            __threadfence_block();
            uint64_t top_seed = 0;
            if (n_seeds && blockIdx.x < g.dir_slots) {
                double v, gv;
                top_seed = ta_top_seed(g.score, base, n_seeds, g.score_cap, lane, &v);
                const uint64_t gtop = ta_top_seed(g.score, base, ng, g.score_cap, lane, &gv);
                ta_run_seed<true>(st, q, top_seed, gtop, lane, g.dir + (uint64_t)blockIdx.x * g.wa * WAVE, s_aln[0], s_aln[1], s_aln[2], &best);
            }
            if (lane == 0) {
                for (int k = 0; k < 9; k++) s_fit[k] = best.R[k];
                for (int k = 0; k < 3; k++) s_fit[9 + k] = best.t[k];
                s_fit[12] = best.tm; s_P = best.P; s_seed = (uint32_t)top_seed;
            }
        }
        __syncthreads();
        const uint32_t P = s_P;
        // fcz_tmscore_dev's full search over the aligned pairs, normalised by Lmin: the seeds wave, wave + 4, ..
        {
            const ta_src_aln src{st.ca, st.cb, s_aln[2]};
            ta_wave_best mine;
            mine.tm = -1.0; mine.seed = 0;
#pragma unroll
            for (int k = 0; k < 9; k++) mine.R[k] = 0.0;
#pragma unroll
            for (int k = 0; k < 3; k++) mine.t[k] = 0.0;
            const uint64_t ts = tm_seed_count(P, g.levels);
            for (uint64_t s = wave; s < ts; s += WAVES_PER_BLOCK) {
                uint32_t start, flen;
                tm_seed_fragment(P, s, &start, &flen);
                tm_best b;
                tm_run_seed<true>(src, q.Sa, lane, q.lmin, start, flen, g.iterations, &b);
                if (b.tm > mine.tm) {
                    mine.tm = b.tm; mine.seed = s;
#pragma unroll
                    for (int k = 0; k < 9; k++) mine.R[k] = b.R[k];
#pragma unroll
                    for (int k = 0; k < 3; k++) mine.t[k] = b.t[k];
                }
            }
            if (lane == 0) s_wb[wave] = mine;
        }
        __syncthreads();
        // the final fit: the search's when it is strictly better than the candidate's
        double R[9], t[3];
        {
            double top = s_fit[12]; int from = -1; uint64_t top_seed = 0;
            for (int w = 0; w < WAVES_PER_BLOCK; w++) {
                const double v = s_wb[w].tm; const uint64_t sd = s_wb[w].seed;
                if (v > top || (from >= 0 && v == top && sd < top_seed)) { top = v; from = w; top_seed = sd; }
            }
#pragma unroll
            for (int k = 0; k < 9; k++) R[k] = from < 0 ? s_fit[k] : s_wb[from].R[k];
#pragma unroll
            for (int k = 0; k < 3; k++) t[k] = from < 0 ? s_fit[9 + k] : s_wb[from].t[k];
        }
        // per row of a: map and dev
        int32_t* map = g.map ? g.map + (uint64_t)p * g.wa : nullptr;
        float* dev = g.dev ? g.dev + (uint64_t)p * g.wa : nullptr;
        for (uint32_t r = threadIdx.x; r < g.wa; r += BLOCK) { if (map) map[r] = -1; if (dev) dev[r] = 0.0f; }
        __syncthreads();
        if (wave == 0) {
            const double d0 = superpose_d0(q.lmin), d0a = superpose_d0(q.Sa), d0b = superpose_d0(q.Sb);
            double sq = 0.0, tms = 0.0, tma = 0.0, tmb = 0.0;
            for (uint32_t i = lane; i < q.Sa; i += WAVE) {
                const int32_t j = s_aln[2][i];
                if (j < 0) continue;
                double a[3], b[3];
#pragma unroll
                for (int k = 0; k < 3; k++) { a[k] = st.ca[k * TMALIGN_MAX_WIDTH + i]; b[k] = st.cb[k * TMALIGN_MAX_WIDTH + j]; }
                const double d2 = superpose_dev2(R, t, a, b), dv = sqrt(d2);
                const double x = dv / d0, xa = dv / d0a, xb = dv / d0b;
                sq = __dadd_rn(sq, d2);
                tms = __dadd_rn(tms, 1.0 / __dadd_rn(1.0, __dmul_rn(x, x)));
                tma = __dadd_rn(tma, 1.0 / __dadd_rn(1.0, __dmul_rn(xa, xa)));
                tmb = __dadd_rn(tmb, 1.0 / __dadd_rn(1.0, __dmul_rn(xb, xb)));
                if (map) map[st.ra[i]] = (int32_t)st.rb[j];
                if (dev) dev[st.ra[i]] = (float)dv;
            }
            sq = superpose_wave_sum(sq); tms = superpose_wave_sum(tms); tma = superpose_wave_sum(tma); tmb = superpose_wave_sum(tmb);
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < 9; k++) g.rot[(uint64_t)p * 9u + k] = (float)R[k];
#pragma unroll
                for (int k = 0; k < 3; k++) g.trans[(uint64_t)p * 3u + k] = (float)t[k];
                if (g.tm) g.tm[p] = q.lmin ? (float)(tms / (double)q.lmin) : 0.0f;
                if (g.tm_a) g.tm_a[p] = q.Sa ? (float)(tma / (double)q.Sa) : 0.0f;
                if (g.tm_b) g.tm_b[p] = q.Sb ? (float)(tmb / (double)q.Sb) : 0.0f;
                if (g.aligned) g.aligned[p] = (int32_t)P;
                if (g.rmsd) g.rmsd[p] = P ? (float)sqrt(sq / (double)P) : 0.0f;
                if (g.sites_a) g.sites_a[p] = (int32_t)q.Sa;
                if (g.sites_b) g.sites_b[p] = (int32_t)q.Sb;
                if (g.seed) g.seed[p] = (int32_t)s_seed;
                if (g.status) g.status[p] = (int32_t)status;
            }
        }
    }
}

// fcz_tmalign_dp_dev: one DP per pair from the caller's float32 transform
__global__ __launch_bounds__(BLOCK) void k_ta_dp(tmalign_args g) {
    __shared__ ta_stage st;
    __shared__ int16_t s_aln[TMALIGN_MAX_WIDTH];
    const uint32_t lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    for (uint32_t p = blockIdx.x; p < g.m; p += gridDim.x) {
        uint32_t la;
        (void)ta_stage_pair(g, p, st, &la);
        const ta_params q = ta_params_of(g, st);
        int32_t* map = g.map ? g.map + (uint64_t)p * g.wa : nullptr;
        for (uint32_t r = threadIdx.x; r < g.wa; r += BLOCK) if (map) map[r] = -1;
        __syncthreads();
        if (wave == 0) {
            double R[9], t[3];
#pragma unroll
            for (int k = 0; k < 9; k++) R[k] = g.rot_in[(uint64_t)p * 9u + k];
#pragma unroll
            for (int k = 0; k < 3; k++) t[k] = g.trans_in[(uint64_t)p * 3u + k];
            uint32_t P = 0;
            if (blockIdx.x < g.dir_slots) P = ta_dp(st.ca, st.cb, q.Sa, q.Sb, lane, R, t, q.d0sq, g.G[0], g.dir + (uint64_t)blockIdx.x * g.wa * WAVE, s_aln);
            if (map)
                for (uint32_t i = lane; i < q.Sa; i += WAVE) { const int32_t j = s_aln[i]; if (j >= 0) map[st.ra[i]] = (int32_t)st.rb[j]; }
            if (lane == 0 && g.aligned) g.aligned[p] = (int32_t)P;
        }
    }
}

}  // namespace fcz
