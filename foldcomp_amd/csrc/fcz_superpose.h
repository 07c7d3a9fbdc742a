// fcz_superpose.h -- two dense tensor batches of one shape (true, pred) -> the least-squares superposition of pred onto true on the
// sites of one slot, per chain: rot [n][3][3], trans [n][3], rmsd [n], sites [n], gdt_counts [n][5], tm [n], and dev [rows], the
// deviation of every site at that superposition; and the transform applied to the whole prediction (pos_out). The reference has no
// such output (its `rmsd` is the unsuperposed sum over two files on the host); the calls stand beside fcz_lddt_dev and read what
// fcz_dense_dev / fcz_dense_packed_dev write, or any tensors of those shapes (include/fcz_hip.h, fcz_superpose_dev).
//
// The contract (include/fcz_hip.h): a row is a SITE by fcz_lddt_dev's rule. Everything per chain is float64, every operation
// rounded, no FMA (-ffp-contract=off for the whole file; the sums spell it out with __dadd_rn / __dmul_rn as the float32 kernels
// do with __fadd_rn). A sum over the sites has a FIXED ORDER: lane l of the chain's wavefront adds its rows l, l + 64, .. in
// ascending order (a row that is no site adds nothing), then an xor-butterfly over the lanes with the distances 32, 16, .. 1, which
// leaves the same bits in every lane (a + b == b + a). So the result depends on neither the launch geometry nor the form.
//
//   k_superpose<PACKED>        one wavefront per chain, four chains a block, persistent over the chains. No LDS: there are no
//                              pairs, and every pass reads the slot's 24 bytes per row (pass 1 brings them into L2, 2 and 3 read
//                              them again). Pass 1: the sites and the two centroids. Pass 2: the nine centred cross sums
//                              M = sum (a - ca)(b - cb)^T (centroid first, centre second: no sum(ab) - S ca cb, which cancels far
//                              from the origin). Then Horn's symmetric 4 x 4 matrix of M and its eigenvectors by cyclic Jacobi
//                              sweeps, on all 64 lanes redundantly from the broadcast sums: identical bits, no divergence, no
//                              scratch round trip. The eigenvector of the largest eigenvalue is a unit quaternion, so R is a
//                              proper rotation by construction; on ties the FIRST largest is taken, and Jacobi starts from the
//                              identity, so a chain with no or one site (Horn's matrix is zero) gets the identity quaternion.
//                              t = cb - R ca. Pass 3: dev = |R a + t - b|, its squared sum, the five GDT counters and the TM sum.
//                              Lane 0 writes the chain's outputs; dev is written for every row of the entry (0 where no site).
//   k_chain_fill<superpose_args>   (fcz_chains.h) packed form only, in front of k_superpose: dev = 0 in every row that no chain is seen to cover
//                              (chain_covers: a covered row it misses is rewritten by k_superpose behind it).
//   k_superpose_apply<A, PACKED>   pos_out = rot_e @ pos_pred + trans_e in float32, x' = ((r00 x + r01 y) + r02 z) + tx, every
//                              operation rounded, no FMA, for every slot whose mask_pred is set in rows inside the chain; 0
//                              elsewhere. The shape of k_lddt's tiling (fcz_chains.h): persistent blocks over tiles of CHAIN_TILE
//                              rows of ONE chain, so the chain's twelve floats are read once per tile through wave-uniform
//                              addresses, and the tile's rows x A x 3 floats leave through dn_emit (fcz_dense.h): 16-byte
//                              stores over the aligned middle, consecutive lanes on consecutive addresses.
//   k_chain_fill<superpose_apply_args>   packed form only: 0 into every row of pos_out that no chain is seen to cover.
//
// Every index that scales with rows * A is 64-bit. A chain's range is clamped to the rows that exist and a range that runs
// backwards is empty (chain_range), so no read leaves the inputs whatever row_off holds.
#pragma once
#include "fcz_chains.h"

namespace fcz {

constexpr uint32_t SUPERPOSE_MAX_ROWS = 0x7FFFFFFFu;   // sites and gdt_counts are int32
constexpr int SUPERPOSE_MAX_SWEEPS = 32;               // cyclic Jacobi on 4 x 4 converges in under ten; the bound ends the loop whatever it is fed

struct superpose_args {
    const float* pos_true; const uint8_t* mask_true;
    const float* pos_pred; const uint8_t* mask_pred;   // mask_pred may be NULL: every slot present
    const uint32_t* bound;                  // padded: length [n] or NULL; packed: row_off [n + 1]
    uint32_t n, L;                          // padded: rows per entry; packed: L = R, the rows of the arrays
    uint32_t A, slot;
    float* rot; float* trans; float* rmsd; int32_t* sites; int32_t* gdt_counts; float* tm; float* dev;   // all but rot / trans may be NULL
};

struct superpose_apply_args {
    const float* pos; const uint8_t* mask;  // mask may be NULL: every slot present
    const uint32_t* bound; uint32_t n, L, A;
    const float* rot; const float* trans;
    float* out;
};

// row r of the arrays holds nothing
__device__ __forceinline__ void chain_empty_row(const superpose_args& g, uint64_t r) { g.dev[r] = 0.0f; }
__device__ __forceinline__ void chain_empty_row(const superpose_apply_args& g, uint64_t r) {
    for (uint32_t i = 0; i < g.A * 3u; i++) g.out[r * (g.A * 3u) + i] = 0.0f;
}

// the slot's coordinates of array row r: a = pred, b = true -> true when the row is a site (both masks set, six finite values)
__device__ __forceinline__ bool superpose_site(const superpose_args& g, uint64_t r, double* a, double* b) {
    const uint64_t o = r * g.A + g.slot;
    if (g.mask_true[o] == 0) return false;
    if (g.mask_pred && g.mask_pred[o] == 0) return false;
    const float* t = g.pos_true + o * 3u;
    const float* p = g.pos_pred + o * 3u;
    const float tx = t[0], ty = t[1], tz = t[2], px = p[0], py = p[1], pz = p[2];
    a[0] = px; a[1] = py; a[2] = pz; b[0] = tx; b[1] = ty; b[2] = tz;
    return isfinite(tx) && isfinite(ty) && isfinite(tz) && isfinite(px) && isfinite(py) && isfinite(pz);
}

// the lanes' partial sums -> their sum, the same bits in every lane
__device__ __forceinline__ double superpose_wave_sum(double v) {
    for (int d = WAVE / 2; d > 0; d >>= 1) v = __dadd_rn(v, __shfl_xor(v, d, WAVE));
    return v;
}
__device__ __forceinline__ uint32_t superpose_wave_count(uint32_t v) {
    for (int d = WAVE / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, WAVE);
    return v;
}

// one Jacobi rotation in the (P, Q) plane of the symmetric a, accumulated into the columns of v; false when a[P][Q] is already
// negligible beside the two diagonal entries (it is then set to 0). P and Q are template arguments so that every index is a
// constant and both matrices stay in registers.
template <int P, int Q> __device__ __forceinline__ bool superpose_rotate(double (&a)[4][4], double (&v)[4][4]) {
    const double apq = a[P][Q], app = a[P][P], aqq = a[Q][Q];
    if (apq == 0.0) return false;
    if (fabs(apq) <= 0x1p-70 * (fabs(app) + fabs(aqq))) { a[P][Q] = 0.0; a[Q][P] = 0.0; return false; }
    const double theta = (aqq - app) / (2.0 * apq);                          // (may overflow to +-inf: t = +-0)
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    a[P][P] = app - t * apq; a[Q][Q] = aqq + t * apq; a[P][Q] = 0.0; a[Q][P] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (k != P && k != Q) {
            const double akp = a[k][P], akq = a[k][Q];
            const double np = c * akp - s * akq, nq = s * akp + c * akq;
            a[k][P] = np; a[P][k] = np; a[k][Q] = nq; a[Q][k] = nq;
        }
        const double vkp = v[k][P], vkq = v[k][Q];
        v[k][P] = c * vkp - s * vkq; v[k][Q] = s * vkp + c * vkq;
    }
    return true;
}

// M = sum (a - ca)(b - cb)^T, row-major -> the rotation R (row-major) that minimises sum |R (a - ca) - (b - cb)|^2
__device__ __forceinline__ void superpose_solve(const double* m, double* R) {
    const double sxx = m[0], sxy = m[1], sxz = m[2], syx = m[3], syy = m[4], syz = m[5], szx = m[6], szy = m[7], szz = m[8];
    double a[4][4] = {{(sxx + syy) + szz, syz - szy, szx - sxz, sxy - syx},
                      {syz - szy, (sxx - syy) - szz, sxy + syx, szx + sxz},
                      {szx - sxz, sxy + syx, (syy - sxx) - szz, syz + szy},
                      {sxy - syx, szx + sxz, syz + szy, (szz - sxx) - syy}};
    double v[4][4] = {{1.0, 0.0, 0.0, 0.0}, {0.0, 1.0, 0.0, 0.0}, {0.0, 0.0, 1.0, 0.0}, {0.0, 0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < SUPERPOSE_MAX_SWEEPS; sweep++) {
        bool any = superpose_rotate<0, 1>(a, v);
        any |= superpose_rotate<0, 2>(a, v);
        any |= superpose_rotate<0, 3>(a, v);
        any |= superpose_rotate<1, 2>(a, v);
        any |= superpose_rotate<1, 3>(a, v);
        any |= superpose_rotate<2, 3>(a, v);
        if (!any) break;
    }
    // the column of the first largest eigenvalue (a NaN matrix compares false everywhere and keeps column 0 of whatever v became)
    double best = a[0][0], w = v[0][0], x = v[1][0], y = v[2][0], z = v[3][0];
#pragma unroll
    for (int j = 1; j < 4; j++) {
        const bool take = a[j][j] > best;
        best = take ? a[j][j] : best;
        w = take ? v[0][j] : w; x = take ? v[1][j] : x; y = take ? v[2][j] : y; z = take ? v[3][j] : z;
    }
    const double norm = sqrt(((w * w + x * x) + y * y) + z * z);              // 1 up to the rotations' rounding
    w = w / norm; x = x / norm; y = y / norm; z = z / norm;
    const double ww = w * w, xx = x * x, yy = y * y, zz = z * z, xy = x * y, wz = w * z, xz = x * z, wy = w * y, yz = y * z, wx = w * x;
    R[0] = ((ww + xx) - yy) - zz; R[1] = 2.0 * (xy - wz);       R[2] = 2.0 * (xz + wy);
    R[3] = 2.0 * (xy + wz);       R[4] = ((ww - xx) + yy) - zz; R[5] = 2.0 * (yz - wx);
    R[6] = 2.0 * (xz - wy);       R[7] = 2.0 * (yz + wx);       R[8] = ((ww - xx) - yy) + zz;
}

template <bool PACKED>
__global__ __launch_bounds__(BLOCK) void k_superpose(superpose_args g) {
    const uint32_t lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    for (uint64_t c = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + wave; c < g.n; c += (uint64_t)gridDim.x * WAVES_PER_BLOCK) {
        const uint32_t e = (uint32_t)c;
        uint64_t row0; uint32_t len, rows;
        chain_range<PACKED>(g.bound, g.L, e, &row0, &len, &rows);
        double a[3], b[3];
        // pass 1: the sites and the centroids
        uint32_t count = 0;
        double sa[3] = {0.0, 0.0, 0.0}, sb[3] = {0.0, 0.0, 0.0};
        for (uint64_t r = lane; r < len; r += WAVE) {
            if (superpose_site(g, row0 + r, a, b)) {
                count++;
#pragma unroll
                for (int i = 0; i < 3; i++) { sa[i] = __dadd_rn(sa[i], a[i]); sb[i] = __dadd_rn(sb[i], b[i]); }
            }
        }
        const uint32_t S = superpose_wave_count(count);
        const double dS = (double)(S ? S : 1u);
        double ca[3], cb[3];
#pragma unroll
        for (int i = 0; i < 3; i++) { ca[i] = superpose_wave_sum(sa[i]) / dS; cb[i] = superpose_wave_sum(sb[i]) / dS; }
        // pass 2: the centred cross sums
        double m[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (uint64_t r = lane; r < len; r += WAVE) {
            if (superpose_site(g, row0 + r, a, b)) {
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
        double R[9], t[3];
        superpose_solve(m, R);
#pragma unroll
        for (int i = 0; i < 3; i++)
            t[i] = __dsub_rn(cb[i], __dadd_rn(__dadd_rn(__dmul_rn(R[3 * i], ca[0]), __dmul_rn(R[3 * i + 1], ca[1])), __dmul_rn(R[3 * i + 2], ca[2])));
        // pass 3: the deviations and what is summed over them
        const double d0 = S > 15u ? fmax(1.24 * cbrt((double)(S - 15u)) - 1.8, 0.5) : 0.5;
        double sq = 0.0, tms = 0.0;
        uint32_t g0 = 0, g1 = 0, g2 = 0, g3 = 0, g4 = 0;
        for (uint64_t r = lane; r < rows; r += WAVE) {
            float out = 0.0f;
            if (r < len && superpose_site(g, row0 + r, a, b)) {
                double d[3];
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    const double p = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(R[3 * i], a[0]), __dmul_rn(R[3 * i + 1], a[1])), __dmul_rn(R[3 * i + 2], a[2])), t[i]);
                    d[i] = __dsub_rn(p, b[i]);
                }
                const double d2 = __dadd_rn(__dadd_rn(__dmul_rn(d[0], d[0]), __dmul_rn(d[1], d[1])), __dmul_rn(d[2], d[2]));
                const double dv = sqrt(d2), q = dv / d0;
                sq = __dadd_rn(sq, d2);
                tms = __dadd_rn(tms, 1.0 / __dadd_rn(1.0, __dmul_rn(q, q)));
                g0 += dv <= 0.5 ? 1u : 0u; g1 += dv <= 1.0 ? 1u : 0u; g2 += dv <= 2.0 ? 1u : 0u; g3 += dv <= 4.0 ? 1u : 0u; g4 += dv <= 8.0 ? 1u : 0u;
                out = (float)dv;
            }
            if (g.dev) g.dev[row0 + r] = out;
        }
        sq = superpose_wave_sum(sq); tms = superpose_wave_sum(tms);
        g0 = superpose_wave_count(g0); g1 = superpose_wave_count(g1); g2 = superpose_wave_count(g2); g3 = superpose_wave_count(g3);
        g4 = superpose_wave_count(g4);
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 9; i++) g.rot[(uint64_t)e * 9u + i] = (float)R[i];
#pragma unroll
            for (int i = 0; i < 3; i++) g.trans[(uint64_t)e * 3u + i] = (float)t[i];
            if (g.rmsd) g.rmsd[e] = S ? (float)sqrt(sq / dS) : 0.0f;
            if (g.sites) g.sites[e] = (int32_t)S;
            if (g.tm) g.tm[e] = S ? (float)(tms / dS) : 0.0f;
            if (g.gdt_counts) {
                int32_t* o = g.gdt_counts + (uint64_t)e * 5u;
                o[0] = (int32_t)g0; o[1] = (int32_t)g1; o[2] = (int32_t)g2; o[3] = (int32_t)g3; o[4] = (int32_t)g4;
            }
        }
    }
}

template <int A, bool PACKED>
__global__ __launch_bounds__(BLOCK) void k_superpose_apply(superpose_apply_args g, const uint64_t* __restrict__ tile_off, uint32_t tiles_per_entry,
                                                           uint64_t n_tiles_padded) {
    const uint64_t n_tiles = chain_tile_count<PACKED>(tile_off, g.n, n_tiles_padded);
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const chain_tile<PACKED> ct(tile_off, g.n, tiles_per_entry, g.bound, g.L, tile, CHAIN_TILE);
        const uint32_t q0 = (uint32_t)ct.q0;                                   // the tile's first row of the chain (< rows)
        const uint32_t nq = ct.rows - q0 < CHAIN_TILE ? ct.rows - q0 : CHAIN_TILE;
        const uint32_t inside = ct.len > q0 ? ct.len - q0 : 0u;                // rows of the tile that lie inside the chain
        const float* rt = g.rot + (uint64_t)ct.e * 9u;
        const float* tr = g.trans + (uint64_t)ct.e * 3u;
        const float r00 = rt[0], r01 = rt[1], r02 = rt[2], r10 = rt[3], r11 = rt[4], r12 = rt[5], r20 = rt[6], r21 = rt[7], r22 = rt[8];
        const float t0 = tr[0], t1 = tr[1], t2 = tr[2];
        const uint64_t atom0 = (ct.row0 + q0) * A;                             // the tile's first atom slot in the arrays
        const float* src = g.pos + atom0 * 3u;
        const uint8_t* msk = g.mask ? g.mask + atom0 : nullptr;
        dn_emit(g.out + atom0 * 3u, nq * (A * 3u), [=](uint32_t f) __attribute__((always_inline)) -> float {
            const uint32_t atom = f / 3u, comp = f - atom * 3u;
            if (atom >= inside * A) return 0.0f;
            if (msk && msk[atom] == 0) return 0.0f;
            const float* p = src + atom * 3u;
            const float x = p[0], y = p[1], z = p[2];
            const float ra = comp == 0 ? r00 : comp == 1 ? r10 : r20, rb = comp == 0 ? r01 : comp == 1 ? r11 : r21;
            const float rc = comp == 0 ? r02 : comp == 1 ? r12 : r22, tt = comp == 0 ? t0 : comp == 1 ? t1 : t2;
            return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(ra, x), __fmul_rn(rb, y)), __fmul_rn(rc, z)), tt);
        });
    }
}

}  // namespace fcz
