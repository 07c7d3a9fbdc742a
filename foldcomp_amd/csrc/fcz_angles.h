// fcz_angles.h -- FCZ records -> torsion-angle tensors on the device: the internal coordinates the record stores, dequantised where
// they lie. No atom is placed (no NeRF, no decoded atoms in): the values are the ones Foldcomp::decompress hands to its
// reconstruction (src/foldcomp.cpp:784-804 for the backbone, :338-369 for the side-chain torsions) and the FCZ branch of
// foldcomp.cxx's get_data returns as lists. Layout (include/fcz_hip.h, fcz_angles_dev): per residue row FCZ_ANGLE_COLUMNS float32
// in degrees -- phi psi omega, the bond angles N-CA-C / CA-C-N(+1) / C-N(+1)-CA(+1), chi1 .. chi4 -- and as many mask bytes; 0.0f
// where the mask is 0.
//
//   k_angles          padded: angles [n][L][10], mask [n][L][10]; rows behind an entry's length (and a skipped entry's L rows): zeros
//   k_angles_packed   packed: angles [R][10], mask [R][10] over the rows of res_off; a skipped entry has no row
//   k_angles_window   padded with a per-entry first residue start[e] (a crop at an offset) and an optional aatype [n][L]: the wavefront
//                     first walks the start[e] residues in front of its window, 64 per step, for their torsion-byte total -- one byte
//                     per residue (the code sits in the word's first byte), nothing stored -- takes word start - 1 as its carry, and
//                     runs the same tile loop from there. The window's first row has phi and N-CA-C when start >= 1.
//
// One wavefront per entry, a persistent grid over the entries. The wavefront walks its entry in tiles of 64 rows, lane = residue:
// word l (psi, omega and the two bond angles behind residue l) is the lane's own 8-byte load, word l - 1 (phi and N-CA-C of l) comes
// from the lane below, across tiles from the last lane of the tile before. The side-chain torsion bytes of residue l start at the
// sum of natoms - 3 over the residues in front of it: a wavefront scan per tile on top of the running total, as k_res_index does
// it; the chi bytes sit among the residue's first six (fcz_res_chi_slot <= 8), one unaligned 8-byte load. About 14 bytes read per
// residue (8 of the word, ~4.4 torsion bytes, the header once per entry).
// The 50 bytes a row leaves with are staged in LDS (640 floats + 640 bytes per tile) and stored as the byte range of the output they
// are: lane = 16 consecutive bytes, consecutive lanes = consecutive addresses, the few elements in front of and behind the 16-byte
// boundaries as single stores (dn_emit with a wavefront's index and stride). A lane-per-row store of 40 bytes would put 64 lanes on 64 segments
// of 2 560 bytes with a stride of 40: every store instruction touches all 20 cache lines of the tile for 4 bytes each.
// Every byte of both arrays is written exactly once and nothing outside them; every index into them is 64-bit.
#pragma once
#include "fcz_compress.h"
#include "fcz_dense.h"

namespace fcz {

constexpr uint32_t AN_COLS = FCZ_ANGLE_COLUMNS;
constexpr uint32_t AN_TILE = WAVE;                                 // rows per tile: one lane per residue

struct angles_lds {
    float val[WAVES_PER_BLOCK][AN_TILE * AN_COLS];
    uint8_t msk[WAVES_PER_BLOCK][AN_TILE * AN_COLS];
    uint32_t chi[FCZ_N_RES_CODES];                                 // fcz_res_chi_slot of the code, a byte per chi
    uint8_t nsc[FCZ_N_RES_CODES];                                  // side-chain torsion bytes of the code: natoms - 3
};

// all rows of entry e: rows_total rows at row `row_base` of the output (padded: L rows at e * L; packed: the entry's own at res_off[e]).
// WIN: row l holds residue min(start, ne) + l, and aatype (may be NULL) receives min(code, 20) per residue row, 20 per padding row.
template <bool WIN>
__device__ __forceinline__ void angles_entry(angles_lds& S, const uint32_t wave, const uint32_t lane, const uint8_t* __restrict__ rec, uint32_t ne,
                                             const uint32_t rows_total, const uint64_t row_base, float* __restrict__ angles, uint8_t* __restrict__ mask,
                                             const uint32_t start = 0, uint8_t* __restrict__ aatype = nullptr) {
    float* sv = S.val[wave];
    uint8_t* sm = S.msk[wave];
    float* const A = angles + row_base * (uint64_t)AN_COLS;
    uint8_t* const M = mask + row_base * (uint64_t)AN_COLS;
    entry_view v; v.n = 0; v.n_sc = 0; v.L = make_layout(0, 0, 0, 0);
    bb_params P{};
    uint32_t rc_first = 23;
    if (ne) {
        v = view_entry(rec);
        if (ne > v.n) ne = v.n;                                    // (res_off is the sizes pass's: equal; a read never leaves the record's own words)
        P = load_params(rec);
        rc_first = (uint32_t)res_code_from_letter(rec[20]);        // header.firstResidue, src/foldcomp.cpp:863
    }
    const uint8_t* words = rec + v.L.o_words;
    const uint8_t* scb = rec + v.L.o_sc;
    const uint32_t w0 = WIN ? (start < ne ? start : ne) : 0u;      // first residue of the window: w0 + l never wraps
    const uint32_t len = ne - w0 < rows_total ? ne - w0 : rows_total;   // rows that hold a residue (padded: cropped to L)
    const float cont = (180.0f - (-180.0f)) / 255.0f;              // FixedAngleDiscretizer(255), src/discretizer.h:89-106
    uint32_t run = 0;                                              // torsion bytes of the residues in front of the tile
    uint32_t carry_lo = 0, carry_hi = 0;                           // word w0 + l0 - 1
    if constexpr (WIN) {
        for (uint32_t k0 = 0; k0 < w0; k0 += AN_TILE) {            // the residues in front of the window: their codes only
            const uint32_t k = k0 + lane;
            uint32_t na = 0;
            if (k < w0) {
                uint32_t rc = k == 0 ? rc_first : (uint32_t)words[8 * (size_t)k] >> 3;
                if (rc >= 24u) rc = 23u;
                na = S.nsc[rc];
            }
            run += wave_sum(na);
        }
        if (w0 >= 1u) { const uint64_t c = ld_u64(words + 8 * (size_t)(w0 - 1u)); carry_lo = (uint32_t)c; carry_hi = (uint32_t)(c >> 32); }
    }
    for (uint32_t l0 = 0; l0 < rows_total; l0 += AN_TILE) {
        const uint32_t rows = rows_total - l0 < AN_TILE ? rows_total - l0 : AN_TILE;
        float* const At = A + (uint64_t)l0 * AN_COLS;
        uint8_t* const Mt = M + (uint64_t)l0 * AN_COLS;
        if (l0 >= len) {   // padding only: constants, no loads
            dn_emit(At, rows * AN_COLS, [](uint32_t) { return 0.0f; }, lane, WAVE);
            dn_emit(Mt, rows * AN_COLS, [](uint32_t) { return (uint8_t)0; }, lane, WAVE);
            if constexpr (WIN) { if (aatype && lane < rows) aatype[row_base + l0 + lane] = 20; }
            continue;
        }
        const uint32_t l = w0 + l0 + lane;                         // residue of the lane
        const bool has = l0 + lane < len;
        const uint64_t w = has ? ld_u64(words + 8 * (size_t)l) : 0ull;
        const uint32_t w_lo = (uint32_t)w, w_hi = (uint32_t)(w >> 32);
        uint32_t p_lo = (uint32_t)__shfl_up((int)w_lo, 1, WAVE), p_hi = (uint32_t)__shfl_up((int)w_hi, 1, WAVE);
        if (lane == 0) { p_lo = carry_lo; p_hi = carry_hi; }
        carry_lo = (uint32_t)__builtin_amdgcn_readlane((int)w_lo, WAVE - 1); carry_hi = (uint32_t)__builtin_amdgcn_readlane((int)w_hi, WAVE - 1);
        const bb_word cur = decode_word(w, P), prv = decode_word((uint64_t)p_lo | ((uint64_t)p_hi << 32), P);
        uint32_t rc = l == 0 ? rc_first : cur.res;                 // the code the decoder uses, clamped as k_entry_sizes clamps it
        if (rc >= 24u) rc = 23u;
        const uint32_t na = has ? (uint32_t)S.nsc[rc] : 0u;
        uint32_t tot;
        const uint32_t ex = run + wave_excl_scan(na, (int)lane, &tot);
        run += tot;
        // the residue's torsion bytes; the load reads at most 7 bytes behind its first one: inside the record (8 + n bytes follow)
        const bool sc_ok = has && na != 0u && ex + na <= v.n_sc;
        const uint64_t sc = sc_ok ? ld_u64(scb + ex) : 0ull;
        const uint32_t chi = S.chi[rc];
        const bool m_prev = has && l >= 1u, m_cur = has && l + 1u < ne;   // word l - 1 / word l hold angles (word n - 1 does not)
        float val[AN_COLS]; bool on[AN_COLS];
        on[0] = m_prev; val[0] = prv.phi;
        on[1] = m_cur; val[1] = cur.psi;
        on[2] = m_cur; val[2] = cur.omega;
        on[3] = m_prev; val[3] = prv.nca;
        on[4] = m_cur; val[4] = cur.can;
        on[5] = m_cur; val[5] = cur.cna;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t slot = (chi >> (8u * k)) & 0xffu;
            on[6 + k] = sc_ok && slot != 0u;
            val[6 + k] = dequant((uint32_t)(sc >> (8u * ((slot - 3u) & 7u))) & 0xffu, -180.0f, cont);
        }
#pragma unroll
        for (uint32_t c = 0; c < AN_COLS; c++) {
            sv[lane * AN_COLS + c] = on[c] ? val[c] : 0.0f;
            sm[lane * AN_COLS + c] = on[c] ? (uint8_t)1 : (uint8_t)0;
        }
        if constexpr (WIN) { if (aatype && lane < rows) aatype[row_base + l0 + lane] = (uint8_t)(has && rc < 20u ? rc : 20u); }
        wave_sync();                       // the rows of all lanes are in LDS
        dn_emit(At, rows * AN_COLS, [&](uint32_t t) { return sv[t]; }, lane, WAVE);
        dn_emit(Mt, rows * AN_COLS, [&](uint32_t t) { return sm[t]; }, lane, WAVE);
        wave_sync();                       // the next tile rewrites the staging
    }
}

template <bool PACKED, bool WIN = false>
__device__ __forceinline__ void angles_grid(const uint8_t* __restrict__ blob, const uint64_t* __restrict__ off, const uint32_t* __restrict__ res_off,
                                            uint32_t n_entries, uint32_t L, float* __restrict__ angles, uint8_t* __restrict__ mask,
                                            const uint32_t* __restrict__ start = nullptr, uint8_t* __restrict__ aatype = nullptr) {
    __shared__ angles_lds S;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    if (tid < FCZ_N_RES_CODES) {
        S.nsc[tid] = (uint8_t)(fcz_res_natoms[tid] - 3);
        S.chi[tid] = (uint32_t)fcz_res_chi_slot[tid][0] | ((uint32_t)fcz_res_chi_slot[tid][1] << 8) | ((uint32_t)fcz_res_chi_slot[tid][2] << 16) |
                     ((uint32_t)fcz_res_chi_slot[tid][3] << 24);
    }
    __syncthreads();
    const uint64_t n_waves = (uint64_t)gridDim.x * WAVES_PER_BLOCK;
    for (uint64_t e = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + wave; e < n_entries; e += n_waves) {
        const uint32_t r0 = res_off[e], ne = res_off[e + 1] - r0;
        if (PACKED && ne == 0u) continue;                          // a skipped entry has no row
        if constexpr (WIN) angles_entry<true>(S, wave, lane, blob + off[e], ne, L, e * (uint64_t)L, angles, mask, start ? start[e] : 0u, aatype);
        else angles_entry<false>(S, wave, lane, blob + off[e], ne, PACKED ? ne : L, PACKED ? (uint64_t)r0 : e * (uint64_t)L, angles, mask);
    }
}

__global__ __launch_bounds__(BLOCK) void k_angles(const uint8_t* __restrict__ blob, const uint64_t* __restrict__ off, const uint32_t* __restrict__ res_off,
                                                  uint32_t n_entries, uint32_t L, float* __restrict__ angles, uint8_t* __restrict__ mask) {
    angles_grid<false>(blob, off, res_off, n_entries, L, angles, mask);
}
__global__ __launch_bounds__(BLOCK) void k_angles_packed(const uint8_t* __restrict__ blob, const uint64_t* __restrict__ off, const uint32_t* __restrict__ res_off,
                                                         uint32_t n_entries, float* __restrict__ angles, uint8_t* __restrict__ mask) {
    angles_grid<true>(blob, off, res_off, n_entries, 0u, angles, mask);
}
__global__ __launch_bounds__(BLOCK) void k_angles_window(const uint8_t* __restrict__ blob, const uint64_t* __restrict__ off, const uint32_t* __restrict__ res_off,
                                                         uint32_t n_entries, uint32_t L, const uint32_t* __restrict__ start, float* __restrict__ angles,
                                                         uint8_t* __restrict__ mask, uint8_t* __restrict__ aatype) {
    angles_grid<false, true>(blob, off, res_off, n_entries, L, angles, mask, start, aatype);
}

}  // namespace fcz
