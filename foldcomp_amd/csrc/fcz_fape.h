// fcz_fape.h -- the backbone FAPE (frame aligned point error; AlphaFold 2 supplement, Algorithm 28) of two batches of rigid frames and
// points of one slot, and its gradient: rot / trans / frame_mask and pos / mask of the truth and of the prediction -> sum [rows] float32
// and points [rows] int32, and, for the caller's row weights w [rows], grad_rot [rows][3][3], grad_trans [rows][3] and grad_pos
// [rows][3] float32 with respect to the prediction's frames and the slot's predicted coordinates. The reference has no such output
// (include/fcz_hip.h, fcz_fape_dev and fcz_fape_grad_dev hold the contract).
//
// A row is a FRAME (fape_frame_row) or a POINT (chain_site2 at the slot) or both; frame i meets every point j of its chain, j == i
// included: u = x_j - t_i, l = R_i^T u for the prediction, the same primed for the truth, e = l - l', d = sqrt(|e|^2 + eps), term =
// min(d, clamp) (fape_term: every operation one rounded float32 operation, the build contracts nothing).
//
//   k_fape<PACKED>               the shape of k_lddt_soft: persistent blocks over query tiles of CHAIN_TILE rows (chain_tile), a lane per
//                                query. A lane is a FRAME and keeps its 24 floats in registers; the chain's POINTS are staged in LDS in
//                                passes of FAPE_PASS rows, ordered (chain_stage_ordered: a lane's result is a float32 sum in ascending row
//                                order), SoA pred x / y / z and true x / y / z, 24 bytes a row, a row that is no point with a NaN pred
//                                x. Every read of a candidate is a broadcast and the test for the marker is wavefront-uniform; a
//                                wavefront without a frame skips the pass (__any).
//   k_fape_grad_frames<PACKED>   the same sweep. A lane accumulates sum_j h (3 floats) and sum_j u (x) h (9 floats) with h = e / d
//                                where d is finite and under the clamp, and applies w_i and R_i in the epilogue: grad_rot and grad_trans.
//   k_fape_grad_points<PACKED>   the roles exchanged: a lane is a POINT (six floats), the chain's FRAMES are staged in passes of
//                                FAPE_FRAME_PASS rows with their weight beside them, 25 floats a row, a row that is no frame with a NaN
//                                rot_pred[0][0]. u = x - t is computed as defined: a constant R^T t per frame would save three
//                                subtractions and make the error scale with the coordinates instead of with the distances. The lane
//                                gathers grad_pos[j] = sum_i w_i R_i h_ij in ascending i.
//   k_chain_fill<fape_args / fape_grad_args>   (fcz_chains.h) packed form only, in front of the sweeps: zeros into every row that no
//                                chain is seen to cover.
// Nothing is kept from the value pass: the gradient recomputes e and d from the inputs (the two gradient sweeps compute the same h,
// from the same operations in the same order). One writer per output element, no atomics; a lane's sums depend on its chain's rows
// alone, so a chain gives the same bytes alone, in any batch, padded or packed.
//
// The reciprocal. h = e * (1 / d) with 1 / d as v_rcp_f32 (within an ulp of its result; d >= sqrt(eps) > 0 is finite where it is
// used): a plain instruction without a mode or a table, as in fcz_lddt_soft.h, so two calls give the same bytes.
//
// LDS and occupancy. FAPE_PASS = 1024 points a pass is 24 KiB of LDS a block (k_lddt_soft's budget), so six blocks (24 wavefronts)
// share a CU's 160 KiB; FAPE_FRAME_PASS = 256 frames a pass is 25 KiB, six blocks as well. A frame is four times a point in LDS, and
// a pass of 1024 frames (100 KiB) would leave one block a CU for a loop of dependent broadcast reads that has nothing but other
// wavefronts to hide behind; the price of the smaller pass is a barrier every 256 candidates.
// `make asm`: k_fape 49 (padded) / 50 (packed) VGPRs, 24 576 bytes of LDS; k_fape_grad_frames 76 VGPRs, 24 576 bytes;
// k_fape_grad_points 62 / 67 VGPRs, 25 600 bytes; six waves per SIMD and no scratch in any of them.
#pragma once
#include "fcz_lddt.h"

namespace fcz {

constexpr uint32_t FAPE_PASS = 1024;        // points staged per candidate pass of k_fape / k_fape_grad_frames: 24 KiB of LDS
constexpr uint32_t FAPE_FRAME_PASS = 256;   // frames staged per candidate pass of k_fape_grad_points: 25 KiB of LDS
constexpr uint32_t FAPE_FRAME_FLOATS = 25;  // rot_pred 9, trans_pred 3, rot_true 9, trans_true 3, weight
constexpr uint32_t FAPE_MAX_ROWS = LDDT_MAX_ROWS;

struct fape_args {
    const float* rot_true; const float* trans_true; const uint8_t* fmask_true;
    const float* pos_true; const uint8_t* mask_true;
    const float* rot_pred; const float* trans_pred; const uint8_t* fmask_pred;   // fmask_pred may be NULL: every frame present
    const float* pos_pred; const uint8_t* mask_pred;                             // mask_pred may be NULL: every slot present
    const uint32_t* bound;                  // padded: length [n] or NULL; packed: row_off [n + 1]
    uint32_t n, L;                          // padded: rows per entry; packed: L = R, the rows of the arrays
    uint32_t A, slot;
    float clamp, eps;
    float* sum; int32_t* points;
};

struct fape_grad_args {
    const float* rot_true; const float* trans_true; const uint8_t* fmask_true;
    const float* pos_true; const uint8_t* mask_true;
    const float* rot_pred; const float* trans_pred; const uint8_t* fmask_pred;
    const float* pos_pred; const uint8_t* mask_pred;
    const uint32_t* bound;
    uint32_t n, L;
    uint32_t A, slot;
    float clamp, eps;
    const float* weight;                    // [rows]: the upstream gradient of sum
    float* grad_rot; float* grad_trans; float* grad_pos;   // [rows][3][3], [rows][3], [rows][3]
};

// a frame in registers: rot [a][k] at 3 a + k (columns are the axes), then trans
struct fape_frame { float r[9], t[3]; };

// row r of the arrays (a row inside its chain) -> true when it is a FRAME: both frame masks set (a NULL fmask_pred is all set) and
// the 24 floats finite; with both masks set the 24 are loaded whatever they hold
template <class Args>
__device__ __forceinline__ bool fape_frame_row(const Args& g, uint64_t r, fape_frame* p, fape_frame* t) {
    if (g.fmask_true[r] == 0) return false;
    if (g.fmask_pred && g.fmask_pred[r] == 0) return false;
    bool fin = true;
#pragma unroll
    for (uint32_t k = 0; k < 9; k++) {
        p->r[k] = g.rot_pred[r * 9u + k]; t->r[k] = g.rot_true[r * 9u + k];
        fin = fin && isfinite(p->r[k]) && isfinite(t->r[k]);
    }
#pragma unroll
    for (uint32_t k = 0; k < 3; k++) {
        p->t[k] = g.trans_pred[r * 3u + k]; t->t[k] = g.trans_true[r * 3u + k];
        fin = fin && isfinite(p->t[k]) && isfinite(t->t[k]);
    }
    return fin;
}

template <class Args>
__device__ __forceinline__ bool fape_point_row(const Args& g, uint64_t r, float* t, float* p) {
    return chain_site2(g.pos_true, g.mask_true, r * g.A + g.slot, g.pos_pred, g.mask_pred, r * g.A + g.slot, t, p);
}

// u = x - t, l = R^T u: l_k = (R[0][k] u0 + R[1][k] u1) + R[2][k] u2
__device__ __forceinline__ void fape_local(const fape_frame& f, float x, float y, float z, float* u, float* l) {
    u[0] = __fsub_rn(x, f.t[0]); u[1] = __fsub_rn(y, f.t[1]); u[2] = __fsub_rn(z, f.t[2]);
#pragma unroll
    for (uint32_t k = 0; k < 3; k++)
        l[k] = __fadd_rn(__fadd_rn(__fmul_rn(f.r[k], u[0]), __fmul_rn(f.r[3u + k], u[1])), __fmul_rn(f.r[6u + k], u[2]));
}

// frame (p, t) against the point with predicted coordinates x and true coordinates y -> d = sqrt(|e|^2 + eps); u the prediction's
// x - t, e = l - l'
__device__ __forceinline__ float fape_term(const fape_frame& p, const fape_frame& t, const float* x, const float* y, float eps, float* u, float* e) {
    float l[3], ut[3], lt[3];
    fape_local(p, x[0], x[1], x[2], u, l);
    fape_local(t, y[0], y[1], y[2], ut, lt);
    e[0] = __fsub_rn(l[0], lt[0]); e[1] = __fsub_rn(l[1], lt[1]); e[2] = __fsub_rn(l[2], lt[2]);
    const float s = __fadd_rn(__fadd_rn(__fmul_rn(e[0], e[0]), __fmul_rn(e[1], e[1])), __fmul_rn(e[2], e[2]));
    return f32_sqrt_rn(__fadd_rn(s, eps));
}

// h = e / d where the term moves: d finite and under the clamp -> true, with h = e * rcp(d)
__device__ __forceinline__ bool fape_h(float d, float clamp, const float* e, float* h) {
    const float inv = __builtin_amdgcn_rcpf(d);
    h[0] = __fmul_rn(e[0], inv); h[1] = __fmul_rn(e[1], inv); h[2] = __fmul_rn(e[2], inv);
    return isfinite(d) && d < clamp;
}

// row r of the arrays holds nothing
__device__ __forceinline__ void chain_empty_row(const fape_args& g, uint64_t r) { g.sum[r] = 0.0f; g.points[r] = 0; }
__device__ __forceinline__ void chain_empty_row(const fape_grad_args& g, uint64_t r) {
#pragma unroll
    for (uint32_t k = 0; k < 9; k++) g.grad_rot[r * 9u + k] = 0.0f;
#pragma unroll
    for (uint32_t k = 0; k < 3; k++) { g.grad_trans[r * 3u + k] = 0.0f; g.grad_pos[r * 3u + k] = 0.0f; }
}

// the staging of a pass of points: slot i of the pass holds row r
template <class Args>
__device__ __forceinline__ void fape_stage_point(const Args& g, uint64_t r, uint32_t i, float* s_px, float* s_py, float* s_pz, float* s_tx, float* s_ty,
                                                 float* s_tz) {
    float t[3] = {0.0f, 0.0f, 0.0f}, p[3] = {0.0f, 0.0f, 0.0f};
    const bool point = fape_point_row(g, r, t, p);
    s_px[i] = point ? p[0] : NAN; s_py[i] = p[1]; s_pz[i] = p[2]; s_tx[i] = t[0]; s_ty[i] = t[1]; s_tz[i] = t[2];
}

template <bool PACKED>
__global__ __launch_bounds__(BLOCK) void k_fape(fape_args g, const uint64_t* __restrict__ tile_off, uint32_t tiles_per_entry, uint64_t n_tiles_padded) {
    __shared__ float s_px[FAPE_PASS], s_py[FAPE_PASS], s_pz[FAPE_PASS], s_tx[FAPE_PASS], s_ty[FAPE_PASS], s_tz[FAPE_PASS];
    const uint32_t tid = threadIdx.x;
    const uint64_t n_tiles = chain_tile_count<PACKED>(tile_off, g.n, n_tiles_padded);
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const chain_tile<PACKED> ct(tile_off, g.n, tiles_per_entry, g.bound, g.L, tile, CHAIN_TILE);
        const uint64_t q = ct.q0 + tid;                               // this lane's row of the chain
        fape_frame fp = {}, ft = {};
        const bool frame = q < ct.len && fape_frame_row(g, ct.row0 + q, &fp, &ft);
        uint32_t points = 0;
        float sum = 0.0f;
        for (uint32_t c0 = 0; c0 < ct.len;) {
            const uint32_t count = chain_stage_ordered<FAPE_PASS>(ct.len, &c0, [&](uint64_t r, uint32_t i) __attribute__((always_inline)) {
                fape_stage_point(g, ct.row0 + r, i, s_px, s_py, s_pz, s_tx, s_ty, s_tz);
            });
            if (__any(frame)) {
                for (uint32_t c = 0; c < count; c++) {
                    const float x[3] = {s_px[c], s_py[c], s_pz[c]};
                    if (x[0] != x[0]) continue;                       // no point (the same word in every lane)
                    const float y[3] = {s_tx[c], s_ty[c], s_tz[c]};
                    float u[3], e[3];
                    const float d = fape_term(fp, ft, x, y, g.eps, u, e);
                    points += 1u;
                    sum = frame && isfinite(d) ? __fadd_rn(sum, d < g.clamp ? d : g.clamp) : sum;
                }
            }
            __syncthreads();                                          // the next pass (or tile) rewrites the staging
        }
        if (q < ct.rows) {
            const uint64_t o = ct.row0 + q;
            g.sum[o] = frame ? sum : 0.0f; g.points[o] = frame ? (int32_t)points : 0;
        }
    }
}

template <bool PACKED>
__global__ __launch_bounds__(BLOCK) void k_fape_grad_frames(fape_grad_args g, const uint64_t* __restrict__ tile_off, uint32_t tiles_per_entry,
                                                            uint64_t n_tiles_padded) {
    __shared__ float s_px[FAPE_PASS], s_py[FAPE_PASS], s_pz[FAPE_PASS], s_tx[FAPE_PASS], s_ty[FAPE_PASS], s_tz[FAPE_PASS];
    const uint32_t tid = threadIdx.x;
    const uint64_t n_tiles = chain_tile_count<PACKED>(tile_off, g.n, n_tiles_padded);
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const chain_tile<PACKED> ct(tile_off, g.n, tiles_per_entry, g.bound, g.L, tile, CHAIN_TILE);
        const uint64_t q = ct.q0 + tid;
        fape_frame fp = {}, ft = {};
        const bool frame = q < ct.len && fape_frame_row(g, ct.row0 + q, &fp, &ft);
        const float w = frame ? g.weight[ct.row0 + q] : 0.0f;
        float sh[3] = {0.0f, 0.0f, 0.0f};                             // sum_j h
        float m[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};   // sum_j u_a h_k at 3 a + k
        for (uint32_t c0 = 0; c0 < ct.len;) {
            const uint32_t count = chain_stage_ordered<FAPE_PASS>(ct.len, &c0, [&](uint64_t r, uint32_t i) __attribute__((always_inline)) {
                fape_stage_point(g, ct.row0 + r, i, s_px, s_py, s_pz, s_tx, s_ty, s_tz);
            });
            if (__any(frame)) {
                for (uint32_t c = 0; c < count; c++) {
                    const float x[3] = {s_px[c], s_py[c], s_pz[c]};
                    if (x[0] != x[0]) continue;
                    const float y[3] = {s_tx[c], s_ty[c], s_tz[c]};
                    float u[3], e[3], h[3];
                    const float d = fape_term(fp, ft, x, y, g.eps, u, e);
                    const bool add = fape_h(d, g.clamp, e, h) && frame;
#pragma unroll
                    for (uint32_t k = 0; k < 3; k++) sh[k] = add ? __fadd_rn(sh[k], h[k]) : sh[k];
#pragma unroll
                    for (uint32_t a = 0; a < 3; a++)
#pragma unroll
                        for (uint32_t k = 0; k < 3; k++) m[3u * a + k] = add ? __fadd_rn(m[3u * a + k], __fmul_rn(u[a], h[k])) : m[3u * a + k];
                }
            }
            __syncthreads();
        }
        if (q < ct.rows) {
            float* orot = g.grad_rot + (ct.row0 + q) * 9u;
            float* otr = g.grad_trans + (ct.row0 + q) * 3u;
#pragma unroll
            for (uint32_t k = 0; k < 9; k++) orot[k] = frame ? __fmul_rn(w, m[k]) : 0.0f;
#pragma unroll
            for (uint32_t a = 0; a < 3; a++) {                        // -w (R sum h)_a
                const float v = __fadd_rn(__fadd_rn(__fmul_rn(fp.r[3u * a], sh[0]), __fmul_rn(fp.r[3u * a + 1u], sh[1])), __fmul_rn(fp.r[3u * a + 2u], sh[2]));
                otr[a] = frame ? -__fmul_rn(w, v) : 0.0f;
            }
        }
    }
}

template <bool PACKED>
__global__ __launch_bounds__(BLOCK) void k_fape_grad_points(fape_grad_args g, const uint64_t* __restrict__ tile_off, uint32_t tiles_per_entry,
                                                            uint64_t n_tiles_padded) {
    __shared__ float s_f[FAPE_FRAME_FLOATS][FAPE_FRAME_PASS];         // rot_pred 0 .. 8, trans_pred 9 .. 11, rot_true 12 .. 20, trans_true 21 .. 23, w 24
    const uint32_t tid = threadIdx.x;
    const uint64_t n_tiles = chain_tile_count<PACKED>(tile_off, g.n, n_tiles_padded);
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const chain_tile<PACKED> ct(tile_off, g.n, tiles_per_entry, g.bound, g.L, tile, CHAIN_TILE);
        const uint64_t q = ct.q0 + tid;
        float y[3] = {0.0f, 0.0f, 0.0f}, x[3] = {0.0f, 0.0f, 0.0f};
        const bool point = q < ct.len && fape_point_row(g, ct.row0 + q, y, x);
        float gp[3] = {0.0f, 0.0f, 0.0f};
        for (uint32_t c0 = 0; c0 < ct.len;) {
            const uint32_t count = chain_stage_ordered<FAPE_FRAME_PASS>(ct.len, &c0, [&](uint64_t r, uint32_t i) __attribute__((always_inline)) {
                fape_frame p = {}, t = {};
                const bool frame = fape_frame_row(g, ct.row0 + r, &p, &t);
#pragma unroll
                for (uint32_t k = 0; k < 9; k++) { s_f[k][i] = p.r[k]; s_f[12u + k][i] = t.r[k]; }
#pragma unroll
                for (uint32_t k = 0; k < 3; k++) { s_f[9u + k][i] = p.t[k]; s_f[21u + k][i] = t.t[k]; }
                if (!frame) s_f[0][i] = NAN;
                s_f[24][i] = frame ? g.weight[ct.row0 + r] : 0.0f;
            });
            if (__any(point)) {
                for (uint32_t c = 0; c < count; c++) {
                    if (s_f[0][c] != s_f[0][c]) continue;             // no frame (the same word in every lane)
                    fape_frame p, t;
#pragma unroll
                    for (uint32_t k = 0; k < 9; k++) { p.r[k] = s_f[k][c]; t.r[k] = s_f[12u + k][c]; }
#pragma unroll
                    for (uint32_t k = 0; k < 3; k++) { p.t[k] = s_f[9u + k][c]; t.t[k] = s_f[21u + k][c]; }
                    const float w = s_f[24][c];
                    float u[3], e[3], h[3];
                    const float d = fape_term(p, t, x, y, g.eps, u, e);
                    const bool add = fape_h(d, g.clamp, e, h) && point;
#pragma unroll
                    for (uint32_t a = 0; a < 3; a++) {                // + w (R h)_a
                        const float v = __fadd_rn(__fadd_rn(__fmul_rn(p.r[3u * a], h[0]), __fmul_rn(p.r[3u * a + 1u], h[1])), __fmul_rn(p.r[3u * a + 2u], h[2]));
                        gp[a] = add ? __fadd_rn(gp[a], __fmul_rn(w, v)) : gp[a];
                    }
                }
            }
            __syncthreads();
        }
        if (q < ct.rows) {
            float* o = g.grad_pos + (ct.row0 + q) * 3u;
            o[0] = point ? gp[0] : 0.0f; o[1] = point ? gp[1] : 0.0f; o[2] = point ? gp[2] : 0.0f;
        }
    }
}

}  // namespace fcz
