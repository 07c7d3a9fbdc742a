// fcz_tmscore.h -- two dense tensor batches of one shape (true, pred) -> per chain the superposition that MAXIMISES the TM-score over
// a search seeded with fragments and refined iteratively, and what fcz_superpose.h writes at that superposition: rot, trans, tm, rmsd,
// sites, gdt_counts, dev, and beside them the winning seed's number and the size of the winning selection (include/fcz_hip.h,
// fcz_tmscore_dev, is the contract). The reference has no such output.
//
// Everything numeric is fcz_superpose.h's: the site rule (superpose_site), float64 sums in the fixed order by chain row
// (superpose_wave_sum: a row outside the selection adds nothing), Horn's matrix by Jacobi sweeps (superpose_solve), and k_superpose's
// expressions for t = cb - R ca, the deviation and d0, restated here operation for operation (superpose_trans, superpose_dev2,
// superpose_d0). So seed 0, round 0 -- the whole chain -- is k_superpose's fit on bits.
//
// A selection is never stored. It is either a range of site numbers (the seed's fragment) or {j : dev_j under a fit < cut}, so it is
// RECOMPUTED from twelve doubles and a cut wherever it is needed: a chain of any length needs no scratch per row, and "the new
// selection equals the previous one" is one pass that evaluates both memberships. A site's number is its rank among the chain's
// sites in row order: a ballot and a popcount per 64 rows.
//
//   k_tm_count<PACKED>     a wavefront per chain: S, the chain's sites, and the number of its work items, one per WAVES_PER_BLOCK
//                          seeds. Only the device knows S. The item counts are scanned (device_scan) into item_off [n + 1].
//   k_tm_search<PACKED>    persistent blocks, each over a contiguous range of the items, an item's chain found by binary search in
//                          item_off (chain_of_tile); a block that stays on a chain does not stage it again. The four
//                          wavefronts of a block take four consecutive seeds of ONE chain, so they share one staged copy of the
//                          slot in LDS: six float planes and a site flag per row, 25 bytes, against a row pitch of 444 bytes in
//                          atom37, read some tens of times per seed. A chain of more than TM_LDS_ROWS rows is read from global
//                          memory instead (the same floats, so the same bits). A seed runs all its rounds on one wavefront and
//                          leaves ONE double, its best tm, in score[4 * item_off[e] + seed]: no transform per seed is kept.
//   k_tm_final<PACKED>     a wavefront per chain: the largest score, of equal ones the lowest seed; that seed is run again (the search
//                          is deterministic), now keeping the fit of its best round (of equal ones the earliest), and the outputs
//                          and dev are written as k_superpose's pass 3 writes them.
//   k_chain_fill<superpose_args>   (fcz_chains.h) packed form only, in front: dev = 0 in every row that no chain is seen to cover.
//
// Every index that scales with rows * A is 64-bit; a chain's range is clamped to the rows that exist (chain_range).
#pragma once
#include "fcz_superpose.h"

namespace fcz {

constexpr uint32_t TM_MAX_ITERATIONS = 64;
constexpr uint32_t TM_LDS_ROWS = 1024;      // rows of a chain that k_tm_search stages: 25 KiB a block
constexpr uint32_t TM_CUT_STEPS = 16384;    // steps of 0.5 A that a cut may grow by before it becomes +inf (tm_run_seed)

struct tmscore_args {
    superpose_args s;                       // the inputs and the outputs shared with fcz_superpose_dev
    int32_t* seed; int32_t* selected;       // [n], may be NULL
    uint32_t levels, iterations;            // levels == 0: every fragment length
    uint32_t* nsites;                       // scratch [n]: S of every chain (k_tm_count)
    uint64_t* item_off;                     // scratch [n + 1]: the scanned item counts
    double* score; uint64_t score_cap;      // scratch: the best tm of every seed; score_cap doubles exist
};

// ---- the seed schedule (host and device) ---------------------------------------------------------------------------------------
// the starts of one fragment length l <= S: 0, step, 2 step, .. while start + l <= S, then S - l if it is not the last one taken
__host__ __device__ inline uint32_t tm_starts(uint32_t S, uint32_t l) {
    const uint32_t step = l / 2u > 1u ? l / 2u : 1u;
    const uint32_t k = (S - l) / step + 1u;
    return (k - 1u) * step == S - l ? k : k + 1u;
}

// the seeds of a chain with S sites: the lengths S, S / 2, .. while they exceed 4, then min(S, 4); only the first `levels` of them
__host__ __device__ inline uint64_t tm_seed_count(uint32_t S, uint32_t levels) {
    uint64_t total = 0;
    uint32_t taken = 0;
    if (S == 0u) return 0;
    for (uint32_t l = S; l > 4u; l /= 2u) {
        if (levels && taken == levels) return total;
        total += tm_starts(S, l); taken++;
    }
    if (levels && taken == levels) return total;
    return total + tm_starts(S, S < 4u ? S : 4u);
}

// seed (< tm_seed_count) -> the first site and the number of sites of its fragment
__host__ __device__ inline void tm_seed_fragment(uint32_t S, uint64_t seed, uint32_t* start, uint32_t* flen) {
    uint32_t l = S;
    for (; l > 4u; l /= 2u) {
        const uint32_t k = tm_starts(S, l);
        if (seed < k) break;
        seed -= k;
    }
    if (l <= 4u) l = S < 4u ? S : 4u;
    const uint32_t step = l / 2u > 1u ? l / 2u : 1u;
    const uint64_t at = seed * step;
    *start = at + l <= S ? (uint32_t)at : S - l;
    *flen = l;
}

// an upper bound of the sum of ceil(seeds / WAVES_PER_BLOCK) over n chains that hold `rows` rows between them: a length l > 4 has at
// most (S - l) / (l / 2) + 2 <= 2.5 S / l + 2 starts, the lengths are >= S / 2^k / 1.2 with 2^k <= S / 5, so these sum to at most
// 1.2 S + 2 * 32; the last length has at most S / 2 + 2 (tests/test_tmscore_cpu.py checks tm_seed_count against it). It holds for
// chains that do not overlap (their sites sum to at most `rows`); 17 * rows wraps only for rows near 2^59, which no allocation reaches
inline uint64_t tm_items_bound(uint64_t rows, uint64_t n) { return ((17u * rows) / 10u + 66u * n) / WAVES_PER_BLOCK + n + 1u; }

// k_superpose's own expressions, operation for operation (fcz_superpose.h stays as it is, so that kernel compiles to what it was):
// t = cb - R ca
__device__ __forceinline__ void superpose_trans(const double* R, const double* ca, const double* cb, double* t) {
#pragma unroll
    for (int i = 0; i < 3; i++)
        t[i] = __dsub_rn(cb[i], __dadd_rn(__dadd_rn(__dmul_rn(R[3 * i], ca[0]), __dmul_rn(R[3 * i + 1], ca[1])), __dmul_rn(R[3 * i + 2], ca[2])));
}
// |R a + t - b|^2
__device__ __forceinline__ double superpose_dev2(const double* R, const double* t, const double* a, const double* b) {
    double d[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double p = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(R[3 * i], a[0]), __dmul_rn(R[3 * i + 1], a[1])), __dmul_rn(R[3 * i + 2], a[2])), t[i]);
        d[i] = __dsub_rn(p, b[i]);
    }
    return __dadd_rn(__dadd_rn(__dmul_rn(d[0], d[0]), __dmul_rn(d[1], d[1])), __dmul_rn(d[2], d[2]));
}
// d0 of the TM sum for S sites
__device__ __forceinline__ double superpose_d0(uint32_t S) { return S > 15u ? fmax(1.24 * cbrt((double)(S - 15u)) - 1.8, 0.5) : 0.5; }

// ---- where a wavefront reads the slot from -----------------------------------------------------------------------------------------
struct tm_src_global {
    const superpose_args& g; uint64_t row0;
    __device__ __forceinline__ bool site(uint32_t r, double* a, double* b) const { return superpose_site(g, row0 + r, a, b); }
};
struct tm_src_lds {
    const float* c; const uint8_t* f;       // c[6][TM_LDS_ROWS]: pred x, y, z, true x, y, z; f: the row is a site
    __device__ __forceinline__ bool site(uint32_t r, double* a, double* b) const {
        if (f[r] == 0) return false;
#pragma unroll
        for (int i = 0; i < 3; i++) { a[i] = c[i * TM_LDS_ROWS + r]; b[i] = c[(3 + i) * TM_LDS_ROWS + r]; }
        return true;
    }
};

// rows r0 .. r0 + 63 of the chain, a lane each: is the lane's row a site, and its number among the chain's sites. Every lane calls it.
template <class Src>
__device__ __forceinline__ bool tm_site(const Src& src, uint32_t r0, uint32_t len, uint32_t lane, uint32_t* base, uint32_t* ord, double* a, double* b) {
    const uint32_t r = r0 + lane;
    const bool s = r < len && src.site(r, a, b);
    const uint64_t m = __ballot(s);
    *ord = *base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    *base += (uint32_t)__popcll(m);
    return s;
}

// a selection: the sites numbered lo .. lo + n - 1 (frag), or the sites whose deviation under the fit R, t lies below cut
struct tm_sel { bool frag; uint32_t lo, n; double R[9], t[3], cut; };

__device__ __forceinline__ bool tm_member(const tm_sel& s, uint32_t ord, const double* a, const double* b) {
    return s.frag ? ord - s.lo < s.n : sqrt(superpose_dev2(s.R, s.t, a, b)) < s.cut;
}

// k_superpose's passes 1 and 2 and its solve on the sites of a selection -> R, t and the size of the selection
template <class Src>
__device__ __forceinline__ uint32_t tm_fit(const Src& src, uint32_t len, uint32_t lane, const tm_sel& sel, double* R, double* t) {
    double a[3], b[3];
    uint32_t count = 0, base = 0, ord;
    double sa[3] = {0.0, 0.0, 0.0}, sb[3] = {0.0, 0.0, 0.0};
    for (uint32_t r0 = 0; r0 < len; r0 += WAVE) {
        if (tm_site(src, r0, len, lane, &base, &ord, a, b) && tm_member(sel, ord, a, b)) {
            count++;
#pragma unroll
            for (int i = 0; i < 3; i++) { sa[i] = __dadd_rn(sa[i], a[i]); sb[i] = __dadd_rn(sb[i], b[i]); }
        }
    }
    const uint32_t n = superpose_wave_count(count);
    const double dn = (double)(n ? n : 1u);
    double ca[3], cb[3];
#pragma unroll
    for (int i = 0; i < 3; i++) { ca[i] = superpose_wave_sum(sa[i]) / dn; cb[i] = superpose_wave_sum(sb[i]) / dn; }
    double m[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    base = 0;
    for (uint32_t r0 = 0; r0 < len; r0 += WAVE) {
        if (tm_site(src, r0, len, lane, &base, &ord, a, b) && tm_member(sel, ord, a, b)) {
#pragma unroll
            for (int i = 0; i < 3; i++) { a[i] = __dsub_rn(a[i], ca[i]); b[i] = __dsub_rn(b[i], cb[i]); }
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) m[3 * i + j] = __dadd_rn(m[3 * i + j], __dmul_rn(a[i], b[j]));
        }
    }
#pragma unroll
    for (int i = 0; i < 9; i++) m[i] = superpose_wave_sum(m[i]);
    superpose_solve(m, R);
    superpose_trans(R, ca, cb, t);
    return n;
}

// (1 / S) sum 1 / (1 + (dev / d0)^2) over all the chain's sites under R, t
template <class Src>
__device__ __forceinline__ double tm_score(const Src& src, uint32_t len, uint32_t lane, uint32_t S, double d0, const double* R, const double* t) {
    double a[3], b[3], tms = 0.0;
    for (uint32_t r = lane; r < len; r += WAVE) {
        if (src.site(r, a, b)) {
            const double q = sqrt(superpose_dev2(R, t, a, b)) / d0;
            tms = __dadd_rn(tms, 1.0 / __dadd_rn(1.0, __dmul_rn(q, q)));
        }
    }
    return superpose_wave_sum(tms) / (double)S;
}

// the sites with dev under R, t below cut, and how many sites lie in exactly one of that set and `sel`
template <class Src>
__device__ __forceinline__ uint32_t tm_select(const Src& src, uint32_t len, uint32_t lane, const tm_sel& sel, const double* R, const double* t, double cut,
                                              uint32_t* differ) {
    double a[3], b[3];
    uint32_t count = 0, diff = 0, base = 0, ord;
    for (uint32_t r0 = 0; r0 < len; r0 += WAVE) {
        if (tm_site(src, r0, len, lane, &base, &ord, a, b)) {
            const bool now = sqrt(superpose_dev2(R, t, a, b)) < cut;
            count += now ? 1u : 0u;
            diff += now != tm_member(sel, ord, a, b) ? 1u : 0u;
        }
    }
    *differ = superpose_wave_count(diff);
    return superpose_wave_count(count);
}

// the need-th smallest deviation under R, t (need <= 3 <= S ... or need = S < 3); the same bits in every lane
template <class Src>
__device__ __forceinline__ double tm_nth_dev(const Src& src, uint32_t len, uint32_t lane, const double* R, const double* t, uint32_t need) {
    double a[3], b[3], d1 = INFINITY, d2 = INFINITY, d3 = INFINITY;
    auto put = [&](double x) __attribute__((always_inline)) {
        double lo = fmin(d1, x); x = fmax(d1, x); d1 = lo;
        lo = fmin(d2, x); x = fmax(d2, x); d2 = lo;
        d3 = fmin(d3, x);
    };
    for (uint32_t r = lane; r < len; r += WAVE)
        if (src.site(r, a, b)) put(sqrt(superpose_dev2(R, t, a, b)));
    for (int d = WAVE / 2; d > 0; d >>= 1) {                                   // (the halves hold different sites: nothing is counted twice)
        const double o1 = __shfl_xor(d1, d, WAVE), o2 = __shfl_xor(d2, d, WAVE), o3 = __shfl_xor(d3, d, WAVE);
        put(o1); put(o2); put(o3);
    }
    return need == 1u ? d1 : need == 2u ? d2 : d3;
}

struct tm_best { double tm; uint32_t round, selected; double R[9], t[3]; };

// one seed: the fit on its fragment, then up to `iterations` rounds of selecting by deviation and fitting again -> the largest tm of
// its rounds, of equal ones the earliest; KEEP: with that round's fit and the size of its selection
template <bool KEEP, class Src>
__device__ __forceinline__ void tm_run_seed(const Src& src, uint32_t len, uint32_t lane, uint32_t S, uint32_t start, uint32_t flen, uint32_t iterations,
                                            tm_best* best) {
    const double d0 = superpose_d0(S);
    const double d_search = fmin(fmax(d0, 4.5), 8.0);
    const uint32_t need = S < 3u ? S : 3u;
    tm_sel sel;
    sel.frag = true; sel.lo = start; sel.n = flen; sel.cut = 0.0;
#pragma unroll
    for (int i = 0; i < 9; i++) sel.R[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) sel.t[i] = 0.0;
    best->tm = -1.0; best->round = 0; best->selected = 0;
    double R[9], t[3];
    for (uint32_t round = 0;; round++) {
        const uint32_t nsel = tm_fit(src, len, lane, sel, R, t);
        const double tm = tm_score(src, len, lane, S, d0, R, t);
        if (tm > best->tm) {
            best->tm = tm; best->round = round; best->selected = nsel;
            if constexpr (KEEP) {
#pragma unroll
                for (int i = 0; i < 9; i++) best->R[i] = R[i];
#pragma unroll
                for (int i = 0; i < 3; i++) best->t[i] = t[i];
            }
        }
        if (round == iterations) break;
        double cut = round == 0u ? d_search - 1.0 : d_search + 1.0;
        uint32_t differ;
        if (tm_select(src, len, lane, sel, R, t, cut, &differ) < need) {
            // cut += 0.5 until `need` sites lie below it, that is until the need-th smallest deviation does: no pass per step. A cut that
            // TM_CUT_STEPS steps do not bring there becomes +inf and selects every site (adding 0.5 to a double above 2^53 changes nothing)
            const double dn = tm_nth_dev(src, len, lane, R, t, need);
            for (uint32_t k = 0; k < TM_CUT_STEPS && !(dn < cut); k++) cut += 0.5;
            if (!(dn < cut)) cut = INFINITY;
            (void)tm_select(src, len, lane, sel, R, t, cut, &differ);
        }
        if (differ == 0u) break;
        sel.frag = false; sel.cut = cut;
#pragma unroll
        for (int i = 0; i < 9; i++) sel.R[i] = R[i];
#pragma unroll
        for (int i = 0; i < 3; i++) sel.t[i] = t[i];
    }
}

// ---- kernels -------------------------------------------------------------------------------------------------------------------------
template <bool PACKED>
__global__ __launch_bounds__(BLOCK) void k_tm_count(tmscore_args g, uint64_t* __restrict__ items) {
    const uint32_t lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    for (uint64_t c = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + wave; c < g.s.n; c += (uint64_t)gridDim.x * WAVES_PER_BLOCK) {
        const uint32_t e = (uint32_t)c;
        uint64_t row0; uint32_t len, rows;
        chain_range<PACKED>(g.s.bound, g.s.L, e, &row0, &len, &rows);
        double a[3], b[3];
        uint32_t count = 0;
        for (uint64_t r = lane; r < len; r += WAVE) count += superpose_site(g.s, row0 + r, a, b) ? 1u : 0u;
        const uint32_t S = superpose_wave_count(count);
        if (lane == 0) {
            g.nsites[e] = S;
            items[e] = (tm_seed_count(S, g.levels) + WAVES_PER_BLOCK - 1u) / WAVES_PER_BLOCK;
        }
    }
}

template <bool PACKED>
__global__ __launch_bounds__(BLOCK) void k_tm_search(tmscore_args g) {
    __shared__ float s_c[6 * TM_LDS_ROWS];
    __shared__ uint8_t s_f[TM_LDS_ROWS];
    const uint32_t lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    const uint64_t n_items = g.item_off[g.s.n];
    uint32_t staged = 0xFFFFFFFFu;                                             // the chain whose slot the LDS holds
    // a block takes a contiguous range of items, so that its successive items are mostly seeds of one chain and the copy is reused
    const uint64_t per = (n_items + gridDim.x - 1u) / gridDim.x, first = (uint64_t)blockIdx.x * per;
    const uint64_t last = first + per < n_items ? first + per : n_items;
    for (uint64_t item = first; item < last; item++) {
        uint32_t e, q;
        chain_of_tile<true>(g.item_off, g.s.n, 0u, item, &e, &q);
        uint64_t row0; uint32_t len, rows;
        chain_range<PACKED>(g.s.bound, g.s.L, e, &row0, &len, &rows);
        const bool in_lds = len <= TM_LDS_ROWS;
        if (in_lds && staged != e) {                                           // (uniform over the block)
            __syncthreads();                                                   // the seeds of the chain before are done with it
            for (uint32_t r = threadIdx.x; r < len; r += BLOCK) {
                double a[3], b[3];
                const bool s = superpose_site(g.s, row0 + r, a, b);
                s_f[r] = s ? 1 : 0;
#pragma unroll
                for (int i = 0; i < 3; i++) { s_c[i * TM_LDS_ROWS + r] = s ? (float)a[i] : 0.0f; s_c[(3 + i) * TM_LDS_ROWS + r] = s ? (float)b[i] : 0.0f; }
            }
            __syncthreads();
            staged = e;
        }
        const uint32_t S = g.nsites[e];
        const uint64_t seed = (uint64_t)q * WAVES_PER_BLOCK + wave, at = g.item_off[e] * WAVES_PER_BLOCK + seed;
        if (seed >= tm_seed_count(S, g.levels) || at >= g.score_cap) continue;
        uint32_t start, flen;
        tm_seed_fragment(S, seed, &start, &flen);
        tm_best best;
        if (in_lds) tm_run_seed<false>(tm_src_lds{s_c, s_f}, len, lane, S, start, flen, g.iterations, &best);
        else tm_run_seed<false>(tm_src_global{g.s, row0}, len, lane, S, start, flen, g.iterations, &best);
        if (lane == 0) g.score[at] = best.tm;
    }
}

template <bool PACKED>
__global__ __launch_bounds__(BLOCK) void k_tm_final(tmscore_args g) {
    const uint32_t lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    for (uint64_t c = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + wave; c < g.s.n; c += (uint64_t)gridDim.x * WAVES_PER_BLOCK) {
        const uint32_t e = (uint32_t)c;
        uint64_t row0; uint32_t len, rows;
        chain_range<PACKED>(g.s.bound, g.s.L, e, &row0, &len, &rows);
        const uint32_t S = g.nsites[e];
        const uint64_t n_seeds = tm_seed_count(S, g.levels), at = g.item_off[e] * WAVES_PER_BLOCK;
        // the largest score, of equal ones the lowest seed
        double top = -1.0; uint64_t top_seed = 0;
        for (uint64_t s = lane; s < n_seeds && at + s < g.score_cap; s += WAVE) {
            const double v = g.score[at + s];
            if (v > top) { top = v; top_seed = s; }
        }
        for (int d = WAVE / 2; d > 0; d >>= 1) {
            const double ov = __shfl_xor(top, d, WAVE);
            const uint64_t os = __shfl_xor(top_seed, d, WAVE);
            if (ov > top || (ov == top && os < top_seed)) { top = ov; top_seed = os; }
        }
        const tm_src_global src{g.s, row0};
        tm_best best;
        best.tm = 0.0; best.round = 0; best.selected = 0;
#pragma unroll
        for (int i = 0; i < 9; i++) best.R[i] = i % 4 == 0 ? 1.0 : 0.0;
#pragma unroll
        for (int i = 0; i < 3; i++) best.t[i] = 0.0;
        if (n_seeds) {
            uint32_t start, flen;
            tm_seed_fragment(S, top_seed, &start, &flen);
            tm_run_seed<true>(src, len, lane, S, start, flen, g.iterations, &best);
        }
        // k_superpose's pass 3 at that fit
        const double d0 = superpose_d0(S), dS = (double)(S ? S : 1u);
        double a[3], b[3], sq = 0.0, tms = 0.0;
        uint32_t g0 = 0, g1 = 0, g2 = 0, g3 = 0, g4 = 0;
        for (uint64_t r = lane; r < rows; r += WAVE) {
            float out = 0.0f;
            if (r < len && superpose_site(g.s, row0 + r, a, b)) {
                const double d2 = superpose_dev2(best.R, best.t, a, b);
                const double dv = sqrt(d2), q = dv / d0;
                sq = __dadd_rn(sq, d2);
                tms = __dadd_rn(tms, 1.0 / __dadd_rn(1.0, __dmul_rn(q, q)));
                g0 += dv <= 0.5 ? 1u : 0u; g1 += dv <= 1.0 ? 1u : 0u; g2 += dv <= 2.0 ? 1u : 0u; g3 += dv <= 4.0 ? 1u : 0u; g4 += dv <= 8.0 ? 1u : 0u;
                out = (float)dv;
            }
            if (g.s.dev) g.s.dev[row0 + r] = out;
        }
        sq = superpose_wave_sum(sq); tms = superpose_wave_sum(tms);
        g0 = superpose_wave_count(g0); g1 = superpose_wave_count(g1); g2 = superpose_wave_count(g2); g3 = superpose_wave_count(g3);
        g4 = superpose_wave_count(g4);
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 9; i++) g.s.rot[(uint64_t)e * 9u + i] = (float)best.R[i];
#pragma unroll
            for (int i = 0; i < 3; i++) g.s.trans[(uint64_t)e * 3u + i] = (float)best.t[i];
            if (g.s.rmsd) g.s.rmsd[e] = S ? (float)sqrt(sq / dS) : 0.0f;
            if (g.s.sites) g.s.sites[e] = (int32_t)S;
            if (g.s.tm) g.s.tm[e] = S ? (float)(tms / dS) : 0.0f;
            if (g.s.gdt_counts) {
                int32_t* o = g.s.gdt_counts + (uint64_t)e * 5u;
                o[0] = (int32_t)g0; o[1] = (int32_t)g1; o[2] = (int32_t)g2; o[3] = (int32_t)g3; o[4] = (int32_t)g4;
            }
            if (g.seed) g.seed[e] = (int32_t)top_seed;
            if (g.selected) g.selected[e] = (int32_t)best.selected;
        }
    }
}

}  // namespace fcz
