// fcz_lddt_soft.h -- the smooth lDDT of AlphaFold 3 (Algorithm 27) on the sites of one slot, and its gradient: two dense tensor batches
// of one shape (true, pred) -> soft [rows] float32 and pairs [rows] int32, and, for the caller's row weights w [rows], grad [rows][3]
// float32 with respect to the slot's predicted coordinates. The only analysis with a backward pass; the reference has no such output
// (include/fcz_hip.h, fcz_lddt_soft_dev and fcz_lddt_soft_grad_dev hold the contract).
//
// The pairs are fcz_lddt.h's to the bit: the site rule (lddt_site), d2 (chain_d2), d = f32_sqrt_rn(d2), j != i and d2_true < c2. Each
// step function [diff < t_k] of fcz_lddt.h becomes sigmoid(t_k - delta): eps = 1/4 sum_k sigmoid(t_k - delta), delta = |d_true - d_pred|.
//
//   k_lddt_soft<PACKED>        the shape of k_lddt: persistent blocks over query tiles of CHAIN_TILE rows (chain_tile), a lane per
//                              query, the chain's rows staged in LDS in passes of LDDT_PASS rows. A lane's result is a float32 SUM, so
//                              the order in which it meets its candidates is part of the contract: ascending row of the chain. The
//                              staging is therefore ORDERED (chain_stage_ordered): the slot of a row is the row minus the first row
//                              of the pass, and a row that is no site is staged with a NaN true x -- its d2 is NaN, d2 < c2 is false,
//                              and the marker costs neither a word of LDS nor a compare. A row's slot gives its row number, so
//                              k_lddt's list of row numbers goes too: SoA true x / y / z and pred x / y / z, 24 bytes a row.
//                              The sum a lane keeps depends on the chain's rows alone: not on the tile (a lane is a row), the pass
//                              (passes are taken in order), the grid or the chains beside it in the batch.
//                              As in k_lddt only a wavefront with a pair under __any pays for the prediction's d2, the two roots and,
//                              here, the four sigmoids.
//   k_lddt_soft_grad<PACKED>   the same sweep with the weight w of every staged row beside its coordinates, 28 bytes a row. It
//                              recomputes delta and the four sigmoids from the coordinates: nothing is kept from the value pass (the
//                              way flash attention recomputes its probabilities), so HBM sees the slot's 24 bytes a row, w and 12
//                              bytes of output. The pair relation is symmetric (chain_d2(a, b) == chain_d2(b, a) bit for bit), so
//                              pair (i, j) stands in soft[i] and in soft[j] and row i gathers its whole gradient with the factor
//                              (w_i + w_j): no scatter, no atomics, one writer per output.
//   k_chain_fill<lddt_soft_args / lddt_soft_grad_args>   (fcz_chains.h) packed form only, in front of the sweep: zeros into every row
//                              that no chain is seen to cover.
//
// LDS and occupancy. LDDT_PASS = 1024 rows a pass is 24 KiB of LDS a block for the value and 28 KiB, k_lddt's budget, for the gradient,
// so six and five blocks (24 and 20 wavefronts) share a CU's 160 KiB, k_lddt's five or better (`make asm`: 38 VGPRs and 24 576 bytes, 6
// waves per SIMD, for the value; 44 .. 48 VGPRs and 28 672 bytes, 5 waves per SIMD, for the gradient; no scratch). The sweep is a chain of dependent
// LDS broadcast reads, double-precision roots and transcendental instructions with nothing but other wavefronts to hide them behind,
// and LDS, not registers, is what bounds the blocks on a CU; a pass of 2048 rows would halve them for nothing: chains of up to 1024
// rows, nearly all there are, take one pass either way.
//
// The exponential. sigmoid(x) = 1 / (1 + e^-x) with e^-x = __expf(-x), the hardware's exp2 of the argument times log2(e), and the
// reciprocal as v_rcp_f32 (both within an ulp or two of their results). The rounding of the scaled argument moves e^-x by a relative
// |x| 2^-24, which moves the sigmoid by at most |x| e^-|x| 2^-24 < 2^-25; with the reciprocal a sigmoid is within 2^-22 or so of its
// value, far inside the 2^-19 a term is allowed, which the float32 roots of two distances use up long before. libm's expf buys
// nothing the tolerance can see and costs a few times the instructions in a loop that is nothing but this. Both are plain
// instructions without a mode or a table: two calls give the same bytes, and so do the padded and the packed kernel, because every
// operation on the path from the coordinates to the sum is written as one rounded operation (__f*_rn; the build contracts nothing).
// An overflowing e^-x is +inf and its sigmoid 0; thresholds are finite (the ABI refuses others), a non-finite delta gives eps = 0.
#pragma once
#include "fcz_lddt.h"

namespace fcz {

struct lddt_soft_args {
    const float* pos_true; const uint8_t* mask_true;
    const float* pos_pred; const uint8_t* mask_pred;   // mask_pred may be NULL: every slot present
    const uint32_t* bound;                  // padded: length [n] or NULL; packed: row_off [n + 1]
    uint32_t n, L;                          // padded: rows per entry; packed: L = R, the rows of the arrays
    uint32_t A, slot;
    float c2;                               // d_true < cutoff <=> d2_true < c2 (lddt_c2)
    float t0, t1, t2, t3;
    float* soft; int32_t* pairs;
};

struct lddt_soft_grad_args {
    const float* pos_true; const uint8_t* mask_true;
    const float* pos_pred; const uint8_t* mask_pred;
    const uint32_t* bound;
    uint32_t n, L;
    uint32_t A, slot;
    float c2;
    float t0, t1, t2, t3;
    const float* weight;                    // [rows]: the upstream gradient of soft
    float* grad;                            // [rows][3]
};

template <class Args>
__device__ __forceinline__ bool lddt_soft_site(const Args& g, uint64_t r, float* t, float* p) {
    return chain_site2(g.pos_true, g.mask_true, r * g.A + g.slot, g.pos_pred, g.mask_pred, r * g.A + g.slot, t, p);
}

// sigmoid(x) for a finite or infinite x (the file's head says why this exp and this reciprocal)
__device__ __forceinline__ float lddt_sigmoid(float x) { return __builtin_amdgcn_rcpf(__fadd_rn(1.0f, __expf(-x))); }

// eps(delta) = 1/4 sum_k sigmoid(t_k - delta), the sum from the first threshold on; 0 for a delta that is not finite
template <class Args>
__device__ __forceinline__ float lddt_soft_eps(const Args& g, float delta) {
    const float s0 = lddt_sigmoid(__fsub_rn(g.t0, delta)), s1 = lddt_sigmoid(__fsub_rn(g.t1, delta));
    const float s2 = lddt_sigmoid(__fsub_rn(g.t2, delta)), s3 = lddt_sigmoid(__fsub_rn(g.t3, delta));
    const float e = __fmul_rn(0.25f, __fadd_rn(__fadd_rn(__fadd_rn(s0, s1), s2), s3));
    return isfinite(delta) ? e : 0.0f;
}

// eps'(delta) = -1/4 sum_k s_k (1 - s_k), for a finite delta
template <class Args>
__device__ __forceinline__ float lddt_soft_deps(const Args& g, float delta) {
    const float s0 = lddt_sigmoid(__fsub_rn(g.t0, delta)), s1 = lddt_sigmoid(__fsub_rn(g.t1, delta));
    const float s2 = lddt_sigmoid(__fsub_rn(g.t2, delta)), s3 = lddt_sigmoid(__fsub_rn(g.t3, delta));
    const float a0 = __fmul_rn(s0, __fsub_rn(1.0f, s0)), a1 = __fmul_rn(s1, __fsub_rn(1.0f, s1));
    const float a2 = __fmul_rn(s2, __fsub_rn(1.0f, s2)), a3 = __fmul_rn(s3, __fsub_rn(1.0f, s3));
    return __fmul_rn(-0.25f, __fadd_rn(__fadd_rn(__fadd_rn(a0, a1), a2), a3));
}

// row r of the arrays holds nothing
__device__ __forceinline__ void chain_empty_row(const lddt_soft_args& g, uint64_t r) { g.soft[r] = 0.0f; g.pairs[r] = 0; }
__device__ __forceinline__ void chain_empty_row(const lddt_soft_grad_args& g, uint64_t r) { g.grad[r * 3u] = 0.0f; g.grad[r * 3u + 1u] = 0.0f; g.grad[r * 3u + 2u] = 0.0f; }

template <bool PACKED>
__global__ __launch_bounds__(BLOCK) void k_lddt_soft(lddt_soft_args g, const uint64_t* __restrict__ tile_off, uint32_t tiles_per_entry, uint64_t n_tiles_padded) {
    __shared__ float s_tx[LDDT_PASS], s_ty[LDDT_PASS], s_tz[LDDT_PASS], s_px[LDDT_PASS], s_py[LDDT_PASS], s_pz[LDDT_PASS];
    const uint32_t tid = threadIdx.x;
    const uint64_t n_tiles = chain_tile_count<PACKED>(tile_off, g.n, n_tiles_padded);
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const chain_tile<PACKED> ct(tile_off, g.n, tiles_per_entry, g.bound, g.L, tile, CHAIN_TILE);
        const uint64_t q = ct.q0 + tid;                               // this lane's row of the chain
        float qt[3] = {0.0f, 0.0f, 0.0f}, qp[3] = {0.0f, 0.0f, 0.0f};
        const bool query = q < ct.len && lddt_soft_site(g, ct.row0 + q, qt, qp);
        const uint32_t qj = (uint32_t)q;
        uint32_t pairs = 0;
        float soft = 0.0f;
        for (uint32_t c0 = 0; c0 < ct.len;) {
            const uint32_t first = c0;
            const uint32_t count = chain_stage_ordered<LDDT_PASS>(ct.len, &c0, [&](uint64_t r, uint32_t i) __attribute__((always_inline)) {
                float t[3] = {0.0f, 0.0f, 0.0f}, p[3] = {0.0f, 0.0f, 0.0f};
                const bool site = lddt_soft_site(g, ct.row0 + r, t, p);
                s_tx[i] = site ? t[0] : NAN; s_ty[i] = t[1]; s_tz[i] = t[2]; s_px[i] = p[0]; s_py[i] = p[1]; s_pz[i] = p[2];
            });
            if (__any(query)) {
                for (uint32_t c = 0; c < count; c++) {
                    const float d2 = chain_d2(s_tx[c], s_ty[c], s_tz[c], qt[0], qt[1], qt[2]);
                    const bool pair = query && first + c != qj && d2 < g.c2;   // (a NaN d2, no site, and a d2 of +inf are no pair)
                    if (__any(pair)) {
                        const float sp = f32_sqrt_rn(chain_d2(s_px[c], s_py[c], s_pz[c], qp[0], qp[1], qp[2]));
                        const float e = lddt_soft_eps(g, fabsf(__fsub_rn(f32_sqrt_rn(d2), sp)));
                        pairs += pair ? 1u : 0u;
                        soft = pair ? __fadd_rn(soft, e) : soft;
                    }
                }
            }
            __syncthreads();                                          // the next pass (or tile) rewrites the staging
        }
        if (q < ct.rows) {
            const uint64_t o = ct.row0 + q;
            g.soft[o] = soft; g.pairs[o] = (int32_t)pairs;
        }
    }
}

template <bool PACKED>
__global__ __launch_bounds__(BLOCK) void k_lddt_soft_grad(lddt_soft_grad_args g, const uint64_t* __restrict__ tile_off, uint32_t tiles_per_entry,
                                                          uint64_t n_tiles_padded) {
    __shared__ float s_tx[LDDT_PASS], s_ty[LDDT_PASS], s_tz[LDDT_PASS], s_px[LDDT_PASS], s_py[LDDT_PASS], s_pz[LDDT_PASS], s_w[LDDT_PASS];
    const uint32_t tid = threadIdx.x;
    const uint64_t n_tiles = chain_tile_count<PACKED>(tile_off, g.n, n_tiles_padded);
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const chain_tile<PACKED> ct(tile_off, g.n, tiles_per_entry, g.bound, g.L, tile, CHAIN_TILE);
        const uint64_t q = ct.q0 + tid;
        float qt[3] = {0.0f, 0.0f, 0.0f}, qp[3] = {0.0f, 0.0f, 0.0f};
        const bool query = q < ct.len && lddt_soft_site(g, ct.row0 + q, qt, qp);
        const float qw = query ? g.weight[ct.row0 + q] : 0.0f;
        const uint32_t qj = (uint32_t)q;
        float gx = 0.0f, gy = 0.0f, gz = 0.0f;
        for (uint32_t c0 = 0; c0 < ct.len;) {
            const uint32_t first = c0;
            const uint32_t count = chain_stage_ordered<LDDT_PASS>(ct.len, &c0, [&](uint64_t r, uint32_t i) __attribute__((always_inline)) {
                float t[3] = {0.0f, 0.0f, 0.0f}, p[3] = {0.0f, 0.0f, 0.0f};
                const bool site = lddt_soft_site(g, ct.row0 + r, t, p);
                s_tx[i] = site ? t[0] : NAN; s_ty[i] = t[1]; s_tz[i] = t[2]; s_px[i] = p[0]; s_py[i] = p[1]; s_pz[i] = p[2];
                s_w[i] = site ? g.weight[ct.row0 + r] : 0.0f;
            });
            if (__any(query)) {
                for (uint32_t c = 0; c < count; c++) {
                    const float d2 = chain_d2(s_tx[c], s_ty[c], s_tz[c], qt[0], qt[1], qt[2]);
                    const bool pair = query && first + c != qj && d2 < g.c2;
                    if (__any(pair)) {
                        const float px = s_px[c], py = s_py[c], pz = s_pz[c];
                        const float sp = f32_sqrt_rn(chain_d2(px, py, pz, qp[0], qp[1], qp[2]));
                        const float diff = __fsub_rn(sp, f32_sqrt_rn(d2));                    // d_pred - d_true
                        // sign(0) = 0, no d_pred of 0 under the division, and a diff that is not finite (a d_pred of +inf) adds nothing
                        const bool add = pair && isfinite(diff) && diff != 0.0f && sp != 0.0f;
                        const float de = lddt_soft_deps(g, fabsf(diff));
                        const float k = __fmul_rn(__fmul_rn(__fadd_rn(qw, s_w[c]), diff < 0.0f ? -de : de), __builtin_amdgcn_rcpf(sp));
                        gx = add ? __fadd_rn(gx, __fmul_rn(k, __fsub_rn(qp[0], px))) : gx;
                        gy = add ? __fadd_rn(gy, __fmul_rn(k, __fsub_rn(qp[1], py))) : gy;
                        gz = add ? __fadd_rn(gz, __fmul_rn(k, __fsub_rn(qp[2], pz))) : gz;
                    }
                }
            }
            __syncthreads();
        }
        if (q < ct.rows) {
            float* o = g.grad + (ct.row0 + q) * 3u;
            o[0] = gx; o[1] = gy; o[2] = gz;
        }
    }
}

}  // namespace fcz
