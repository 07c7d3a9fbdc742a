// fcz_gdt.h -- two dense tensor batches of one shape (true, pred) -> per chain and per GDT cutoff (0.5, 1, 2, 4, 8 A) the LARGEST number
// of sites that some superposition of the seeded search brings under that cutoff, the superposition behind each count, and per row
// which of the five it lies under (include/fcz_hip.h, fcz_gdt_dev, is the contract). fcz_superpose.h and
// fcz_tmscore.h count the five thresholds at ONE fit; GDT is defined as a maximum per cutoff. The reference has no such output.
//
// Everything numeric is fcz_tmscore.h's, used as it is: the seed schedule, tm_fit (k_superpose's passes on a selection), tm_select,
// tm_nth_dev, tm_site and the two sources. What differs is the objective -- five integers per fit in place of one double -- and that a
// seed is searched in up to six RUNS that differ in the cut of their selections only: run 0 has fcz_tmscore_dev's cuts, run 1 + k the
// constant cut c_k. Round 0 of every run of a seed is the fit on the fragment: it is made once.
//
//   k_tm_count<PACKED>     (fcz_tmscore.h, as it is) S of every chain and its work items, one per WAVES_PER_BLOCK seeds.
//   k_gdt_search<PACKED>   k_tm_search's shape: persistent blocks over contiguous ranges of the items, four wavefronts on four
//                          consecutive seeds of ONE chain staged in LDS (a chain above TM_LDS_ROWS rows is read from global memory
//                          through the same code). A wavefront runs all runs and rounds of its seed and keeps the largest count per
//                          cutoff; it leaves them by a 64-bit atomicMax into best[chain][k] = count << 32 | (0xFFFFFFFF - seed):
//                          the larger count wins, of equal ones the lower seed. An integer maximum does not depend on the order
//                          of its operands, so neither the launch geometry nor the timing shows in the result, and no scratch per
//                          seed exists. A wavefront whose key does not exceed what the word already holds leaves it alone.
//   k_gdt_final<PACKED>    a block per chain. Wavefront w takes cutoffs w, w + 4: it runs the winning seed again (the search is
//                          deterministic) and stops at the first fit, in the order of runs and rounds, that reaches the count, which
//                          gives run, selection size and transform. The five float64 transforms meet in LDS; then every row of the
//                          chain belongs to ONE thread, which evaluates it under all five and writes its byte of `within` once.
//   k_chain_fill<gdt_fill_args>   (fcz_chains.h) packed form only, in front: within = 0 in every row that no chain is seen to cover.
//
// Every index that scales with rows * A is 64-bit; a chain's range is clamped to the rows that exist (chain_range).
#pragma once
#include "fcz_tmscore.h"

namespace fcz {

constexpr uint32_t GDT_CUTOFFS = 5;         // c_k = 0.5 * 2^k
constexpr uint32_t GDT_RUNS = 6;            // run 0: the TM cuts; run 1 + k: the constant cut c_k

struct gdt_args {
    superpose_args s;                       // the inputs; none of its outputs is used (all NULL)
    int32_t* gdt_counts; int32_t* sites;    // [n][5], [n]
    float* rot; float* trans;               // [n][5][3][3], [n][5][3]
    int32_t* seed; int32_t* run; int32_t* selected;   // [n][5]
    uint8_t* within;                        // [rows]; all but gdt_counts may be NULL
    uint32_t levels, iterations, runs;      // runs: bit r = run r, 1 .. 63
    const uint32_t* nsites;                 // scratch [n]: S of every chain (k_tm_count)
    const uint64_t* item_off;               // scratch [n + 1]: the scanned item counts
    unsigned long long* best;               // scratch [n][5], zeroed: count << 32 | (0xFFFFFFFF - seed)
};

struct gdt_fill_args { const uint32_t* bound; uint32_t n, L; uint8_t* within; };
__device__ __forceinline__ void chain_empty_row(const gdt_fill_args& g, uint64_t r) { g.within[r] = 0; }

__device__ __forceinline__ double gdt_cutoff(uint32_t k) { return 0.5 * (double)(1u << k); }   // exact

// the sites with dev <= c[0 .. N - 1] under R, t, over all the chain's sites
template <int N, class Src>
__device__ __forceinline__ void gdt_count(const Src& src, uint32_t len, uint32_t lane, const double* R, const double* t, const double* c, uint32_t* g) {
    double a[3], b[3];
#pragma unroll
    for (int k = 0; k < N; k++) g[k] = 0;
    for (uint32_t r = lane; r < len; r += WAVE) {
        if (src.site(r, a, b)) {
            const double dv = sqrt(superpose_dev2(R, t, a, b));
#pragma unroll
            for (int k = 0; k < N; k++) g[k] += dv <= c[k] ? 1u : 0u;
        }
    }
#pragma unroll
    for (int k = 0; k < N; k++) g[k] = superpose_wave_count(g[k]);
}

struct gdt_hit { uint32_t run, selected; double R[9], t[3]; };

// one seed: the fit on its fragment, then for every run of `runs` up to `iterations` rounds of selecting by deviation and fitting again,
// by tm_run_seed's rules with the run's cuts.
//   FIND false: best[k] = the largest count under c_k over all fits visited.
//   FIND true:  the first fit, in the order of runs and rounds, with `target` sites under the ONE cutoff c -> hit (true), which is
//               left as it was when no fit has that many.
template <bool FIND, class Src>
__device__ __forceinline__ bool gdt_run_seed(const Src& src, uint32_t len, uint32_t lane, uint32_t S, uint32_t start, uint32_t flen, uint32_t iterations,
                                             uint32_t runs, uint32_t* best, double c, uint32_t target, gdt_hit* hit) {
    const double d_search = fmin(fmax(superpose_d0(S), 4.5), 8.0);
    const uint32_t need = S < 3u ? S : 3u;
    const double c5[GDT_CUTOFFS] = {0.5, 1.0, 2.0, 4.0, 8.0};
    // a fit was made: count it -> true when the search is over
    auto visit = [&](uint32_t run, uint32_t nsel, const double* R, const double* t) __attribute__((always_inline)) -> bool {
        if constexpr (FIND) {
            uint32_t g1;
            gdt_count<1>(src, len, lane, R, t, &c, &g1);
            if (g1 < target) return false;
            hit->run = run; hit->selected = nsel;
#pragma unroll
            for (int i = 0; i < 9; i++) hit->R[i] = R[i];
#pragma unroll
            for (int i = 0; i < 3; i++) hit->t[i] = t[i];
            return true;
        } else {
            uint32_t g[GDT_CUTOFFS];
            gdt_count<(int)GDT_CUTOFFS>(src, len, lane, R, t, c5, g);
#pragma unroll
            for (int k = 0; k < (int)GDT_CUTOFFS; k++) best[k] = g[k] > best[k] ? g[k] : best[k];
            return false;
        }
    };
    tm_sel sel;
    sel.frag = true; sel.lo = start; sel.n = flen; sel.cut = 0.0;
#pragma unroll
    for (int i = 0; i < 9; i++) sel.R[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) sel.t[i] = 0.0;
    double R0[9], t0[3], R[9], t[3];
    const uint32_t n0 = tm_fit(src, len, lane, sel, R0, t0);                   // round 0 of every run
    if (visit((uint32_t)__ffs((int)runs) - 1u, n0, R0, t0)) return true;
    for (uint32_t run = 0; run < GDT_RUNS; run++) {
        if (!((runs >> run) & 1u)) continue;
        sel.frag = true;
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = R0[i];
#pragma unroll
        for (int i = 0; i < 3; i++) t[i] = t0[i];
        for (uint32_t round = 1; round <= iterations; round++) {
            double cut = run ? gdt_cutoff(run - 1u) : round == 1u ? d_search - 1.0 : d_search + 1.0;
            uint32_t differ;
            if (tm_select(src, len, lane, sel, R, t, cut, &differ) < need) {       // tm_run_seed's widening of the cut
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
            const uint32_t nsel = tm_fit(src, len, lane, sel, R, t);
            if (visit(run, nsel, R, t)) return true;
        }
    }
    return false;
}

// ---- kernels -------------------------------------------------------------------------------------------------------------------------
template <bool PACKED>
__global__ __launch_bounds__(BLOCK) void k_gdt_search(gdt_args g) {
    __shared__ float s_c[6 * TM_LDS_ROWS];
    __shared__ uint8_t s_f[TM_LDS_ROWS];
    const uint32_t lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    const uint64_t n_items = g.item_off[g.s.n];
    uint32_t staged = 0xFFFFFFFFu;                                             // the chain whose slot the LDS holds
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
        const uint64_t seed = (uint64_t)q * WAVES_PER_BLOCK + wave;
        if (seed >= tm_seed_count(S, g.levels)) continue;
        uint32_t start, flen;
        tm_seed_fragment(S, seed, &start, &flen);
        uint32_t best[GDT_CUTOFFS] = {0, 0, 0, 0, 0};
        if (in_lds) (void)gdt_run_seed<false>(tm_src_lds{s_c, s_f}, len, lane, S, start, flen, g.iterations, g.runs, best, 0.0, 0u, nullptr);
        else (void)gdt_run_seed<false>(tm_src_global{g.s, row0}, len, lane, S, start, flen, g.iterations, g.runs, best, 0.0, 0u, nullptr);
        // lane k leaves the key of cutoff k (every lane holds all five counts)
        uint32_t mine = best[0];
#pragma unroll
        for (int k = 1; k < (int)GDT_CUTOFFS; k++) mine = lane == (uint32_t)k ? best[k] : mine;
        if (lane < GDT_CUTOFFS) {
            const unsigned long long key = ((unsigned long long)mine << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)seed);
            unsigned long long* word = g.best + (uint64_t)e * GDT_CUTOFFS + lane;
            if (key > __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) (void)atomicMax(word, key);
        }
    }
}

template <bool PACKED>
__global__ __launch_bounds__(BLOCK) void k_gdt_final(gdt_args g) {
    __shared__ double s_fit[GDT_CUTOFFS][12];
    const uint32_t lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    for (uint32_t e = blockIdx.x; e < g.s.n; e += gridDim.x) {
        uint64_t row0; uint32_t len, rows;
        chain_range<PACKED>(g.s.bound, g.s.L, e, &row0, &len, &rows);
        const uint32_t S = g.nsites[e];
        const uint64_t n_seeds = tm_seed_count(S, g.levels);
        const tm_src_global src{g.s, row0};
        for (uint32_t k = wave; k < GDT_CUTOFFS; k += WAVES_PER_BLOCK) {
            const unsigned long long key = g.best[(uint64_t)e * GDT_CUTOFFS + k];
            gdt_hit hit;
            hit.run = 0; hit.selected = 0;
#pragma unroll
            for (int i = 0; i < 9; i++) hit.R[i] = i % 4 == 0 ? 1.0 : 0.0;
#pragma unroll
            for (int i = 0; i < 3; i++) hit.t[i] = 0.0;
            uint64_t seed = 0;
            if (n_seeds) {
                seed = 0xFFFFFFFFu - (uint32_t)key;
                if (seed >= n_seeds) seed = 0;                                 // (a word nothing was left in: cannot happen with n_seeds > 0)
                uint32_t start, flen;
                tm_seed_fragment(S, seed, &start, &flen);
                (void)gdt_run_seed<true>(src, len, lane, S, start, flen, g.iterations, g.runs, nullptr, gdt_cutoff(k), (uint32_t)(key >> 32), &hit);
            }
            if (lane == 0) {
                const uint64_t at = (uint64_t)e * GDT_CUTOFFS + k;
#pragma unroll
                for (int i = 0; i < 9; i++) { s_fit[k][i] = hit.R[i]; if (g.rot) g.rot[at * 9u + i] = (float)hit.R[i]; }
#pragma unroll
                for (int i = 0; i < 3; i++) { s_fit[k][9 + i] = hit.t[i]; if (g.trans) g.trans[at * 3u + i] = (float)hit.t[i]; }
                g.gdt_counts[at] = (int32_t)(key >> 32);
                if (g.seed) g.seed[at] = (int32_t)seed;
                if (g.run) g.run[at] = (int32_t)hit.run;
                if (g.selected) g.selected[at] = (int32_t)hit.selected;
                if (k == 0 && g.sites) g.sites[e] = (int32_t)S;
            }
        }
        if (g.within) {                                                        // (uniform over the grid)
            __syncthreads();
            double a[3], b[3];
            for (uint64_t r = threadIdx.x; r < rows; r += BLOCK) {
                uint32_t bits = 0;
                if (r < len && superpose_site(g.s, row0 + r, a, b)) {
#pragma unroll
                    for (int k = 0; k < (int)GDT_CUTOFFS; k++)
                        bits |= sqrt(superpose_dev2(s_fit[k], s_fit[k] + 9, a, b)) <= gdt_cutoff((uint32_t)k) ? 1u << k : 0u;
                }
                g.within[row0 + r] = (uint8_t)bits;
            }
            __syncthreads();                                                   // the next chain's fits overwrite s_fit
        }
    }
}

}  // namespace fcz
