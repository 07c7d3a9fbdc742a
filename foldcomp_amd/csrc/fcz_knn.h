// fcz_knn.h -- dense tensors -> k-nearest-neighbour residue graph (index [rows][k] int32, dist [rows][k] float32) on the device.
// The reference has no such output (Foldcomp::decompress, src/foldcomp.cpp:779, ends at a flat vector<AtomCoordinate>); the call
// stands beside it like the dense ones and reads what fcz_dense_dev / fcz_dense_packed_dev write (include/fcz_hip.h, fcz_knn_dev).
//
// The contract (include/fcz_hip.h): a row is a SITE when it lies inside its chain, its mask at the slot is set and its three
// coordinates there are finite. d2 = (dx*dx + dy*dy) + dz*dz in float32, every operation rounded, no FMA. The neighbours of site i
// are the other sites of its chain in the order of the 64-bit key (bits of d2 << 32) | j: d2 >= 0 orders as an unsigned integer,
// j makes the order total, so the list does not depend on the order the candidates are met in.
//
//   k_knn<KCAP, PACKED>   persistent blocks over QUERY TILES of KNN_TILE = 256 rows of one chain, a lane per query. The chain's
//                         sites are staged in LDS in passes of KNN_PASS chain rows (SoA x / y / z and the compacted row number;
//                         slots are handed out by an LDS counter -- the order inside a pass is free, see above), and every lane
//                         sweeps the pass: one broadcast LDS read per candidate, eight float operations, one 64-bit compare
//                         against the worst key it keeps. The KCAP best keys of a lane are a sorted list in REGISTERS: an
//                         accepted key goes through KCAP compare-exchange steps with static indices (a list indexed by a
//                         variable would go to scratch, a list in LDS costs the CU's shared LDS cycles on every insertion),
//                         and the steps run only when some lane of the wavefront accepts. KCAP = 16 / 32 / 48 / 64 is the
//                         smallest that holds k. A wavefront without a query skips the sweep and keeps the barriers.
//                         The L x L matrix is never written: HBM sees the slot's 12 bytes per row and the [rows][k] outputs.
//                         Padded form: tile -> (entry, tile of the entry) by division; every row of the entry is written,
//                         -1 / 0 where it is no site. Packed form: the chains' tile counts are scanned on the device
//                         (k_chain_tiles, device_scan) and a tile finds its chain by binary search (fcz_chains.h, shared
//                         with every other per-chain sweep).
//   k_chain_fill<knn_args>   (fcz_chains.h) packed form only, in front of k_knn: -1 / 0 (chain_empty_row) into every row that no
//                         chain is seen to cover (a search of row_off that a hostile row_off may mislead: a covered row it misses is
//                         rewritten by k_knn behind it).
//
// Every index that scales with rows * k or rows * A is 64-bit. A chain's range is clamped to the R rows that exist and a range
// that runs backwards is empty, so no read leaves pos / mask whatever row_off holds.
#pragma once
#include "fcz_chains.h"

namespace fcz {

constexpr uint32_t KNN_TILE = CHAIN_TILE;   // query rows per tile (a lane per query)
constexpr uint32_t KNN_PASS = 2048;         // chain rows staged per candidate pass: 32 KiB of LDS
constexpr uint32_t KNN_MAX_K = 64;
constexpr uint64_t KNN_NONE = ~0ull;        // no neighbour: above every key (its d2 half is a NaN pattern)

typedef int32_t knn_i4 __attribute__((ext_vector_type(4)));
typedef float knn_f4 __attribute__((ext_vector_type(4)));

struct knn_args {
    const float* pos; const uint8_t* mask;
    const uint32_t* bound;                  // padded: length [n] or NULL; packed: row_off [n + 1]
    uint32_t n, L;                          // padded: rows per entry; packed: L = R, the rows of the arrays
    uint32_t A, slot, k;
    int32_t* index; float* dist;
};

// the slot's coordinates of array row r -> true when the row is a site (mask set, three finite values)
__device__ __forceinline__ bool knn_site(const knn_args& g, uint64_t r, float* c) { return chain_site(g.pos, g.mask, r * g.A + g.slot, c); }

__device__ __forceinline__ void knn_decode(uint64_t key, uint32_t base, int32_t* idx, float* d) {
    const bool none = key == KNN_NONE;
    *idx = none ? -1 : (int32_t)(base + (uint32_t)key);
    *d = none ? 0.0f : f32_sqrt_rn(__uint_as_float((uint32_t)(key >> 32)));
}

// row r of the arrays holds nothing
__device__ __forceinline__ void chain_empty_row(const knn_args& g, uint64_t r) {
    for (uint32_t s = 0; s < g.k; s++) { g.index[r * g.k + s] = -1; g.dist[r * g.k + s] = 0.0f; }
}

template <int KCAP, bool PACKED>
__global__ __launch_bounds__(BLOCK) void k_knn(knn_args g, const uint64_t* __restrict__ tile_off, uint32_t tiles_per_entry, uint64_t n_tiles_padded) {
    __shared__ float s_x[KNN_PASS], s_y[KNN_PASS], s_z[KNN_PASS];
    __shared__ uint32_t s_j[KNN_PASS];
    __shared__ uint32_t s_count;
    const uint32_t tid = threadIdx.x;
    const uint64_t n_tiles = chain_tile_count<PACKED>(tile_off, g.n, n_tiles_padded);
    const bool wide = (g.k & 3u) == 0 && (((uintptr_t)g.index | (uintptr_t)g.dist) & 15u) == 0;   // 16-byte stores of four columns
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const chain_tile<PACKED> ct(tile_off, g.n, tiles_per_entry, g.bound, g.L, tile, KNN_TILE);
        const uint64_t q = ct.q0 + tid;                               // this lane's row of the chain
        float qc[3] = {0.0f, 0.0f, 0.0f};
        const bool query = q < ct.len && knn_site(g, ct.row0 + q, qc);
        const uint32_t qj = (uint32_t)q;
        uint64_t list[KCAP];
#pragma unroll
        for (int s = 0; s < KCAP; s++) list[s] = KNN_NONE;
        for (uint32_t c0 = 0; c0 < ct.len;) {
            const uint32_t count = chain_stage_rows<KNN_PASS>(&s_count, ct.len, &c0, [&](uint64_t r, chain_slots slots) __attribute__((always_inline)) {
                float c[3];
                if (knn_site(g, ct.row0 + r, c)) {
                    const uint32_t i = slots.next();
                    s_x[i] = c[0]; s_y[i] = c[1]; s_z[i] = c[2]; s_j[i] = (uint32_t)r;
                }
            });
            if (__any(query)) {
                for (uint32_t c = 0; c < count; c++) {
                    const uint32_t j = s_j[c];
                    const float d2 = chain_d2(s_x[c], s_y[c], s_z[c], qc[0], qc[1], qc[2]);
                    uint64_t key = ((uint64_t)__float_as_uint(d2) << 32) | j;
                    if (!query || j == qj) key = KNN_NONE;
                    if (__any(key < list[KCAP - 1])) {
#pragma unroll
                        for (int s = 0; s < KCAP; s++) {              // sorted insertion: the key sinks to its place, the worst falls out
                            const uint64_t o = list[s];
                            const bool lt = key < o;
                            list[s] = lt ? key : o;
                            key = lt ? o : key;
                        }
                    }
                }
            }
            __syncthreads();                                          // the next pass (or tile) rewrites the staging
        }
        if (q < ct.rows) {
            const uint32_t base = PACKED ? (uint32_t)ct.row0 : 0u;
            const uint64_t o = (ct.row0 + q) * (uint64_t)g.k;
            if (wide) {
#pragma unroll
                for (int s = 0; s < KCAP; s += 4)
                    if ((uint32_t)s < g.k) {
                        knn_i4 vi; knn_f4 vd; int32_t i; float d;
                        knn_decode(list[s], base, &i, &d); vi.x = i; vd.x = d;
                        knn_decode(list[s + 1], base, &i, &d); vi.y = i; vd.y = d;
                        knn_decode(list[s + 2], base, &i, &d); vi.z = i; vd.z = d;
                        knn_decode(list[s + 3], base, &i, &d); vi.w = i; vd.w = d;
                        *reinterpret_cast<knn_i4*>(g.index + o + s) = vi;
                        *reinterpret_cast<knn_f4*>(g.dist + o + s) = vd;
                    }
            } else {
#pragma unroll
                for (int s = 0; s < KCAP; s++)
                    if ((uint32_t)s < g.k) knn_decode(list[s], base, &g.index[o + s], &g.dist[o + s]);
            }
        }
    }
}

}  // namespace fcz
