// fcz_frames.h -- dense tensors -> rigid frames per residue (rot [rows][G][3][3], trans [rows][G][3] float32, frame_mask [rows][G])
// on the device. The reference has no such output (Foldcomp::decompress, src/foldcomp.cpp:779, ends at a flat
// vector<AtomCoordinate>); the call stands beside it like the dense ones and reads what fcz_dense_dev / fcz_dense_window_dev /
// fcz_dense_packed_dev write (include/fcz_hip.h, fcz_frames_dev).
//
// The contract (include/fcz_hip.h): group g of a row is built from three atoms (p, o, q) of that row: v1 = p - o for the backbone
// group and o - p for the others, v2 = q - o, origin o; e1 = v1 / |v1|, e2 = the part of v2 orthogonal to e1, normalised,
// e3 = e1 x e2, every float32 operation rounded, no FMA, square roots and divisions correctly rounded. A group that does not
// exist (the row lies outside its chain, the type or the layout has no such atom, a cleared mask, a coordinate or a norm that is
// not finite, a norm of 0) is the identity, origin 0, mask 0.
//
//   k_frames<A, G>   persistent blocks over tiles of FR_ITEMS / G consecutive rows of the FLAT row space 0 .. n * L - 1: frames
//                    use atoms of their own row only, so an entry matters for the `length` test alone (one division per row) and
//                    a tile is one contiguous byte range of every array, in the padded, the windowed and the packed form alike.
//                    A tile's rows are staged in LDS with coalesced loads -- whole rows for G = 8 (16 bytes per lane over the
//                    aligned middle of the range), the first three slots N, CA, C of every row for G = 1 (36 of a row's 444 bytes
//                    in atom37) -- and the 16-byte pieces that hold no row inside its chain are not loaded at all. Then a lane
//                    computes one (row, group) item from LDS and leaves its 9 + 3 floats and its mask byte in LDS in output order;
//                    the tile's rot / trans / frame_mask ranges leave through dn_emit (fcz_dense.h): 16-byte stores over the
//                    aligned middle, single elements in front and behind, every byte written once.
//                    The three slots of a (type, group) come from frames_table, which the host builds from fcz_frame_atom and
//                    fcz_dense_slot for the layout and hands over by value.
//
// Every index that scales with rows * A or rows * G is 64-bit. No scratch: the nine coordinates of an item are scalars.
#pragma once
#include "fcz_dense.h"

namespace fcz {

constexpr uint32_t FR_ITEMS = BLOCK;        // (row, group) items per tile: a lane each
constexpr uint32_t FR_GROUPS = 8;
constexpr uint32_t FR_TYPES = 21;           // aatype 0 .. 19, 20 = every other value: backbone and psi only

// slot[type][group][j] = slot of defining atom j (fcz_frame_atom's order: p, o, q) in the layout, 255 = no such group / slot
struct frames_table { uint8_t slot[FR_TYPES][FR_GROUPS][3]; };

struct frames_args {
    const float* pos; const uint8_t* mask; const uint8_t* aatype; const uint32_t* length;
    uint64_t rows;                          // n * L
    uint32_t L;
    float* rot; float* trans; uint8_t* frame_mask;
};

// `count` elements of T from src into LDS dst, rows of ROW elements, element t wanted when live(t): 16-byte loads over the aligned
// middle of the range (a piece is loaded when an element of it is wanted: its last one and one per ROW elements are asked, which
// meets every row the piece touches), single elements around it
template <uint32_t ROW, class T, class F> __device__ __forceinline__ void fr_stage(T* dst, const T* __restrict__ src, uint32_t count, F live) {
    constexpr uint32_t PER = 16 / sizeof(T);
    constexpr uint32_t STEP = ROW < PER ? ROW : PER;
    const uint32_t mis = (uint32_t)((uintptr_t)src & 15u) / (uint32_t)sizeof(T);
    uint32_t head = (PER - mis) % PER;
    if (head > count) head = count;
    const uint32_t body = (count - head) / PER, tail0 = head + body * PER;
    for (uint32_t q = threadIdx.x; q < body; q += BLOCK) {
        const uint32_t t = head + q * PER;
        bool any = live(t + PER - 1u);
#pragma unroll
        for (uint32_t i = 0; i < PER - 1u; i += STEP) any = any || live(t + i);
        if (!any) continue;
        const dn_u4 v = *reinterpret_cast<const dn_u4*>(src + t);
        if constexpr (sizeof(T) == 4) {
            uint32_t* d = reinterpret_cast<uint32_t*>(dst + t);
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        } else {
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 0; i < 16; i++) dst[t + i] = (T)(w[i >> 2] >> (8 * (i & 3)));
        }
    }
    if (threadIdx.x < head && live(threadIdx.x)) dst[threadIdx.x] = src[threadIdx.x];
    if (threadIdx.x < count - tail0 && live(tail0 + threadIdx.x)) dst[tail0 + threadIdx.x] = src[tail0 + threadIdx.x];
}

template <int A, int G>
__global__ __launch_bounds__(BLOCK) void k_frames(frames_args g, uint64_t n_tiles, frames_table tab) {
    constexpr uint32_t T = FR_ITEMS / G;                 // rows per tile (a multiple of 4: a tile of whole atom37 rows begins on 16 bytes)
    constexpr uint32_t NEED = G == 1 ? 3u : (uint32_t)A; // slots staged per row: N, CA, C for the backbone group, the row otherwise
    __shared__ __attribute__((aligned(16))) float s_pos[T * NEED * 3];
    __shared__ __attribute__((aligned(16))) uint8_t s_mask[T * NEED];
    __shared__ __attribute__((aligned(16))) float s_rot[FR_ITEMS * 9];
    __shared__ __attribute__((aligned(16))) float s_trans[FR_ITEMS * 3];
    __shared__ __attribute__((aligned(16))) uint8_t s_fm[FR_ITEMS];
    __shared__ uint8_t s_type[T];                        // the row's type 0 .. 20; 255 = the row lies outside its chain
    __shared__ uint8_t s_slot[FR_TYPES * FR_GROUPS * 3];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < FR_TYPES * FR_GROUPS * 3; i += BLOCK) s_slot[i] = (&tab.slot[0][0][0])[i];
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t row0 = tile * T;
        const uint32_t rows = g.rows - row0 < T ? (uint32_t)(g.rows - row0) : T;
        if (tid < rows) {
            const uint64_t r = row0 + tid;
            bool in = true;
            if (g.length) { const uint64_t e = r / g.L; in = (uint32_t)(r - e * g.L) < g.length[e]; }   // (l < L always: min(length, L))
            uint32_t ty = 20;
            if (G != 1 && in) { ty = g.aatype[r]; if (ty > 20u) ty = 20u; }
            s_type[tid] = (uint8_t)(in ? ty : 255u);
        }
        __syncthreads();
        if constexpr (NEED == (uint32_t)A) {             // whole rows: one contiguous range
            fr_stage<(uint32_t)(A * 3)>(s_pos, g.pos + row0 * (uint64_t)(A * 3), rows * (uint32_t)(A * 3), [&](uint32_t t) { return s_type[t / (uint32_t)(A * 3)] != 255u; });
            fr_stage<(uint32_t)A>(s_mask, g.mask + row0 * (uint64_t)A, rows * (uint32_t)A, [&](uint32_t t) { return s_type[t / (uint32_t)A] != 255u; });
        } else {                                         // the first NEED slots of every row: consecutive lanes, consecutive floats of a row
            for (uint32_t t = tid; t < rows * NEED * 3u; t += BLOCK) {
                const uint32_t lr = t / (NEED * 3u), c = t - lr * (NEED * 3u);
                if (s_type[lr] != 255u) s_pos[t] = g.pos[(row0 + lr) * (uint64_t)(A * 3) + c];
            }
            for (uint32_t t = tid; t < rows * NEED; t += BLOCK) {
                const uint32_t lr = t / NEED, c = t - lr * NEED;
                if (s_type[lr] != 255u) s_mask[t] = g.mask[(row0 + lr) * (uint64_t)A + c];
            }
        }
        __syncthreads();
        {   // item = (row, group) in output order
            const uint32_t lr = tid / (uint32_t)G, gr = tid - lr * (uint32_t)G;
            float r00 = 1.0f, r01 = 0.0f, r02 = 0.0f, r10 = 0.0f, r11 = 1.0f, r12 = 0.0f, r20 = 0.0f, r21 = 0.0f, r22 = 1.0f;
            float tx = 0.0f, ty = 0.0f, tz = 0.0f;
            bool ok = false;
            const uint32_t type = lr < rows ? s_type[lr] : 255u;
            if (type != 255u) {
                const uint8_t* sl = s_slot + (type * FR_GROUPS + (G == 1 ? 0u : gr)) * 3u;
                const uint32_t sp = sl[0], so = sl[1], sq = sl[2];
                if (sp < NEED && so < NEED && sq < NEED) {
                    const uint8_t* m = s_mask + lr * NEED;
                    const float* P = s_pos + (lr * NEED + sp) * 3u;
                    const float* O = s_pos + (lr * NEED + so) * 3u;
                    const float* Q = s_pos + (lr * NEED + sq) * 3u;
                    if (m[sp] != 0 && m[so] != 0 && m[sq] != 0) {
                        const float px = P[0], py = P[1], pz = P[2], ox = O[0], oy = O[1], oz = O[2], qx = Q[0], qy = Q[1], qz = Q[2];
                        const bool fin = isfinite(px) && isfinite(py) && isfinite(pz) && isfinite(ox) && isfinite(oy) && isfinite(oz) &&
                                         isfinite(qx) && isfinite(qy) && isfinite(qz);
                        const bool bb = gr == 0u;        // the backbone group: v1 = p - o (C - CA); the others: v1 = o - p
                        const float v1x = bb ? __fsub_rn(px, ox) : __fsub_rn(ox, px);
                        const float v1y = bb ? __fsub_rn(py, oy) : __fsub_rn(oy, py);
                        const float v1z = bb ? __fsub_rn(pz, oz) : __fsub_rn(oz, pz);
                        const float v2x = __fsub_rn(qx, ox), v2y = __fsub_rn(qy, oy), v2z = __fsub_rn(qz, oz);
                        const float n1 = f32_sqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(v1x, v1x), __fmul_rn(v1y, v1y)), __fmul_rn(v1z, v1z)));
                        const float e1x = f32_div_rn(v1x, n1), e1y = f32_div_rn(v1y, n1), e1z = f32_div_rn(v1z, n1);
                        const float d = __fadd_rn(__fadd_rn(__fmul_rn(e1x, v2x), __fmul_rn(e1y, v2y)), __fmul_rn(e1z, v2z));
                        const float ux = __fsub_rn(v2x, __fmul_rn(e1x, d)), uy = __fsub_rn(v2y, __fmul_rn(e1y, d)), uz = __fsub_rn(v2z, __fmul_rn(e1z, d));
                        const float n2 = f32_sqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(ux, ux), __fmul_rn(uy, uy)), __fmul_rn(uz, uz)));
                        const float e2x = f32_div_rn(ux, n2), e2y = f32_div_rn(uy, n2), e2z = f32_div_rn(uz, n2);
                        ok = fin && isfinite(n1) && n1 > 0.0f && isfinite(n2) && n2 > 0.0f;
                        if (ok) {
                            r00 = e1x; r10 = e1y; r20 = e1z;
                            r01 = e2x; r11 = e2y; r21 = e2z;
                            r02 = __fsub_rn(__fmul_rn(e1y, e2z), __fmul_rn(e1z, e2y));
                            r12 = __fsub_rn(__fmul_rn(e1z, e2x), __fmul_rn(e1x, e2z));
                            r22 = __fsub_rn(__fmul_rn(e1x, e2y), __fmul_rn(e1y, e2x));
                            tx = ox; ty = oy; tz = oz;
                        }
                    }
                }
            }
            float* R = s_rot + tid * 9u;
            R[0] = r00; R[1] = r01; R[2] = r02; R[3] = r10; R[4] = r11; R[5] = r12; R[6] = r20; R[7] = r21; R[8] = r22;
            float* t3 = s_trans + tid * 3u;
            t3[0] = tx; t3[1] = ty; t3[2] = tz;
            s_fm[tid] = ok ? 1 : 0;
        }
        __syncthreads();
        const uint64_t item0 = row0 * (uint64_t)G;
        const uint32_t items = rows * (uint32_t)G;
        dn_emit(g.rot + item0 * 9u, items * 9u, [&](uint32_t t) { return s_rot[t]; });
        dn_emit(g.trans + item0 * 3u, items * 3u, [&](uint32_t t) { return s_trans[t]; });
        dn_emit(g.frame_mask + item0, items, [&](uint32_t t) { return s_fm[t]; });
        __syncthreads();   // the next tile rewrites the staging
    }
}

}  // namespace fcz
