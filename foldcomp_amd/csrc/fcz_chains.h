// fcz_chains.h -- what the per-chain sweeps over dense tensors share (k-NN, lDDT, DSSP, SASA, violations, superpose apply): which rows
// of the arrays are chain e's, which chain a query tile belongs to, and which packed rows no chain covers.
//
// Padded form: bound is length [n] or NULL, L the rows per entry; chain e is rows e * L .. e * L + min(length[e], L) and every one
// of the entry's L rows is written. Packed form: bound is row_off [n + 1], L = R, the rows of the arrays; a chain's range is clamped
// to the R rows that exist and a range that runs backwards is empty, so no read leaves the arrays whatever row_off holds.
// A sweep runs persistent blocks over QUERY TILES of whole rows of one chain (CHAIN_TILE rows, a lane per query, unless the sweep
// has a tile size of its own: fcz_sasa.h, fcz_violations.h): padded, tile -> (entry, tile of the entry) by division; packed, the
// chains' tile counts are scanned on the device (k_chain_tiles with the sweep's rows per tile, device_scan) and a tile finds its
// chain by binary search, as k_dense_packed's rows do.
#pragma once
#include "fcz_dense.h"

namespace fcz {

constexpr uint32_t CHAIN_TILE = BLOCK;      // query rows per tile (a lane per query)

// chain e: its first row in the arrays, the rows that may hold a site, the rows the sweep writes
template <bool PACKED>
__device__ __forceinline__ void chain_range(const uint32_t* __restrict__ bound, uint32_t L, uint32_t e, uint64_t* row0, uint32_t* len, uint32_t* rows) {
    if constexpr (PACKED) {
        uint32_t lo = bound[e], hi = bound[e + 1];
        if (lo > L) lo = L;
        if (hi > L) hi = L;
        *row0 = lo; *len = hi > lo ? hi - lo : 0u; *rows = *len;
    } else {
        const uint32_t le = bound ? bound[e] : L;
        *row0 = (uint64_t)e * L; *len = le < L ? le : L; *rows = L;
    }
}

// packed form: tiles of tile_rows rows of every chain, for the scan that gives each tile its chain
__global__ __launch_bounds__(BLOCK) void k_chain_tiles(const uint32_t* __restrict__ row_off, uint32_t n, uint32_t R, uint32_t tile_rows, uint64_t* __restrict__ tiles) {
    for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < n; e += (uint64_t)gridDim.x * BLOCK) {
        uint64_t row0; uint32_t len, rows;
        chain_range<true>(row_off, R, (uint32_t)e, &row0, &len, &rows);
        tiles[e] = rows / tile_rows + (rows % tile_rows ? 1u : 0u);
    }
}

// tile -> its chain e and the tile's number t inside the chain
template <bool PACKED>
__device__ __forceinline__ void chain_of_tile(const uint64_t* __restrict__ tile_off, uint32_t n, uint32_t tiles_per_entry, uint64_t tile, uint32_t* e, uint32_t* t) {
    if constexpr (PACKED) {   // the largest e with tile_off[e] <= tile: a chain that has tiles
        uint32_t lo = 0, hi = n;
        while (hi - lo > 1u) { const uint32_t mid = lo + ((hi - lo) >> 1); if (tile_off[mid] <= tile) lo = mid; else hi = mid; }
        *e = lo; *t = (uint32_t)(tile - tile_off[lo]);
    } else {
        *e = (uint32_t)(tile / tiles_per_entry); *t = (uint32_t)(tile - (uint64_t)*e * tiles_per_entry);
    }
}

// packed form: is row r (< R) seen to lie in a chain? A search of row_off that a hostile row_off may mislead: a covered row it
// misses is filled in front of the sweep and rewritten by the sweep behind it.
__device__ __forceinline__ bool chain_covers(const uint32_t* __restrict__ row_off, uint32_t n, uint64_t r) {
    if (n == 0) return false;
    const uint32_t e = dn_entry_of(row_off, 0u, n, (uint32_t)r);
    return row_off[e] <= r && r < row_off[e + 1];                     // (r < R: chain e's clamped range holds the row)
}

}  // namespace fcz
