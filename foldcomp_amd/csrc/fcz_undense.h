// fcz_undense.h -- dense padded tensors (atom37 / atom14 / backbone4) -> a flat fcz_chain_batch on the device: k_dense in reverse.
// The reference has no such input (Foldcomp::compress, src/foldcomp.cpp:562, takes a flat span<AtomCoordinate>); the layouts are
// those of fcz_dense.h, the contract is stated in include/fcz_hip.h (fcz_dense_in) and restated by tests/_undense.py.
//
// A gather whose cost is its loads (444 B of pos per atom37 row against ~110 B written), so the INPUT index space is the work:
//
//   k_undense_count<A>  one block per chain, lane = row. A tile of 256 mask rows is one contiguous byte range: coalesced 16-byte
//                       loads into LDS, then every lane reads its row's slots through the layout's table (canonical position ->
//                       slot). Out: one 16-bit word per row (bit j = the residue's canonical atom j is present, bit 14 = the chain's
//                       OXT), the chain's residue and atom counts (0 when the chain is refused) and its status. The row words
//                       are the only thing the fill pass knows about the mask: the two passes cannot disagree about an atom,
//                       so no store of the fill pass depends on the caller leaving the mask alone between them.
//   (two exclusive scans over the chains: res_off, first atom of every chain; the totals reach the host once)
//   k_undense_fill<A>   persistent blocks over tiles of DN_TILE = 64 rows of one chain. The tile's pos rows are one contiguous range
//                       (coalesced 16-byte non-temporal loads into LDS, read once; rows behind the chain's end and tiles of
//                       padding or of a refused chain load nothing), the rows' first atoms come from a wave scan of the row words
//                       on top of the block's sum over the rows in front of the tile (2 B per row, from L2, as k_dense does with
//                       the residue codes). Then lane = (row, canonical position): the present ones are consecutive output atoms,
//                       so a wavefront's stores to x / y / z / atom_code cover one contiguous range.
//
// Nothing is read as data where mask == 0 or behind length[c]: such bytes are staged with their row at most, never selected.
//
// Where a chain's rows lie is the kernels' template parameter: ud_padded (chain c = rows c * L .. of [n][L], length[c] of them; tile t
// = chain t / tiles_per_chain) or ud_packed (chain c = rows row_off[c] .. row_off[c + 1] of [R]; its tiles are tile_off[c] ..
// tile_off[c + 1], the scan of the per-chain tile counts the counting pass leaves, searched by the fill pass). The row words are
// indexed by the row of the input either way.
#pragma once
#include "fcz_dense.h"

namespace fcz {

constexpr uint32_t UD_OXT_BIT = 1u << FCZ_MAX_RES_ATOMS;          // row word: the chain's OXT sits in slot 36 of this (last) row
constexpr uint32_t UD_ITEMS = FCZ_MAX_RES_ATOMS + 1;              // work items of a row: its canonical positions, then the OXT
constexpr uint32_t UD_COUNT_ROWS = BLOCK;                         // rows per tile of k_undense_count (lane = row)

// slot[res_code * 14 + j] = slot of the residue's canonical atom j in the layout, 255 = the layout has none
struct undense_table { uint8_t slot[FCZ_N_RES_CODES * FCZ_MAX_RES_ATOMS]; };

struct undense_in { const float* pos; const uint8_t* mask; const uint8_t* aatype; const uint32_t* length; const float* plddt; };
struct undense_out { uint32_t* atom_off; float* x; float* y; float* z; uint8_t* atom_code; uint8_t* res_code; float* bfac_ca; };

// the padded form [n][L]: rows of chain c, and the chain and first row of a tile of the fill pass
struct ud_padded {
    static constexpr bool packed = false;
    const uint32_t* length; uint32_t L, tiles_per_chain; uint64_t tiles;
    __device__ __forceinline__ uint64_t base(uint32_t c) const { return (uint64_t)c * L; }
    __device__ __forceinline__ uint32_t len(uint32_t c, bool* refused) const {   // (nResidue is a uint16 in the record's header)
        const uint32_t v = length[c];
        *refused = v > L || v > 65535u;
        return v;
    }
    __device__ __forceinline__ uint64_t n_tiles() const { return tiles; }
    __device__ __forceinline__ void tile(uint64_t t, uint32_t* c, uint32_t* l0) const {
        *c = (uint32_t)(t / tiles_per_chain);
        *l0 = (uint32_t)(t - (uint64_t)*c * tiles_per_chain) * DN_TILE;
    }
};
// the packed form [R]: chain c = rows row_off[c] .. row_off[c + 1]; refused when the range runs backwards, leaves the R rows the
// caller has, or is longer than a record can say
struct ud_packed {
    static constexpr bool packed = true;
    const uint32_t* row_off; uint32_t R, n; const uint32_t* tile_off;
    __device__ __forceinline__ uint64_t base(uint32_t c) const { return row_off[c]; }
    __device__ __forceinline__ uint32_t len(uint32_t c, bool* refused) const {
        const uint32_t b = row_off[c], e = row_off[c + 1];
        *refused = e < b || e > R || e - b > 65535u;
        return *refused ? 0u : e - b;
    }
    __device__ __forceinline__ uint64_t n_tiles() const { return tile_off[n]; }
    __device__ __forceinline__ void tile(uint64_t t, uint32_t* c, uint32_t* l0) const {
        *c = dn_entry_of(tile_off, 0u, n, (uint32_t)t);                         // (chains without tiles are passed over)
        *l0 = ((uint32_t)t - tile_off[*c]) * DN_TILE;
    }
};

__device__ __forceinline__ uint32_t ud_res_code(uint32_t aatype) { return aatype < 20u ? aatype : (uint32_t)FCZ_RES_UNK; }

// `count` elements of T at p -> img[0 .. count), img = an LDS buffer + the elements p lies behind a 16-byte boundary (so that
// 16-byte global loads meet 16-byte LDS stores): vector loads over the aligned middle, single elements in front and behind
template <class T> __device__ __forceinline__ uint32_t ud_misalign(const T* p) { return (uint32_t)((uintptr_t)p & 15u) / (uint32_t)sizeof(T); }
template <class T> __device__ __forceinline__ void ud_stage(const T* __restrict__ p, uint32_t count, T* img) {
    constexpr uint32_t PER = 16 / sizeof(T);
    uint32_t head = (PER - ud_misalign(p)) % PER;
    if (head > count) head = count;
    const uint32_t body = (count - head) / PER, tail0 = head + body * PER;
    for (uint32_t q = threadIdx.x; q < body; q += BLOCK) {
        const uint32_t t = head + q * PER;
        *reinterpret_cast<dn_u4*>(img + t) = __builtin_nontemporal_load(reinterpret_cast<const dn_u4*>(p + t));
    }
    if (threadIdx.x < head) img[threadIdx.x] = p[threadIdx.x];
    if (threadIdx.x < count - tail0) img[tail0 + threadIdx.x] = p[tail0 + threadIdx.x];
}

template <int A, class RA>
__global__ __launch_bounds__(BLOCK) void k_undense_count(undense_in g, uint32_t n, RA ra, undense_table tab, uint16_t* __restrict__ row_word,
                                                         uint32_t* __restrict__ n_res, uint32_t* __restrict__ n_atoms, int32_t* __restrict__ status,
                                                         uint32_t* __restrict__ chain_tiles) {
    __shared__ __attribute__((aligned(16))) uint8_t s_mask[UD_COUNT_ROWS * A + 16];
    __shared__ uint8_t s_slot[FCZ_N_RES_CODES * FCZ_MAX_RES_ATOMS];
    __shared__ uint8_t s_na[FCZ_N_RES_CODES];
    __shared__ uint32_t s_cnt[WAVES_PER_BLOCK], s_bad[WAVES_PER_BLOCK];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t i = tid; i < FCZ_N_RES_CODES * FCZ_MAX_RES_ATOMS; i += BLOCK) s_slot[i] = tab.slot[i];
    if (tid < FCZ_N_RES_CODES) s_na[tid] = fcz_res_natoms[tid];
    __syncthreads();
    for (uint32_t c = blockIdx.x; c < n; c += gridDim.x) {
        bool too_long;
        const uint32_t len_in = ra.len(c, &too_long);
        const uint32_t len = too_long ? 0u : len_in;
        const uint64_t chain_row = ra.base(c);
        uint32_t cnt = 0, bad = 0;
        for (uint32_t l0 = 0; l0 < len; l0 += UD_COUNT_ROWS) {
            const uint32_t rows = len - l0 < UD_COUNT_ROWS ? len - l0 : UD_COUNT_ROWS;
            const uint64_t row0 = chain_row + l0;
            const uint8_t* mp = g.mask + row0 * (uint64_t)A;
            uint8_t* img = s_mask + ud_misalign(mp);
            const uint32_t aa = tid < rows ? (uint32_t)g.aatype[row0 + tid] : 0u;
            ud_stage(mp, rows * (uint32_t)A, img);
            __syncthreads();
            if (tid < rows) {
                const uint32_t rc = ud_res_code(aa), na = s_na[rc];
                const uint8_t* m = img + tid * (uint32_t)A;
                uint32_t w = 0;
#pragma unroll
                for (uint32_t j = 0; j < (uint32_t)FCZ_MAX_RES_ATOMS; j++) {
                    const uint32_t s = s_slot[rc * FCZ_MAX_RES_ATOMS + j];
                    if (j < na && s != 255u && m[s]) w |= 1u << j;
                }
                // N, CA, C are the canonical positions 0, 1, 2 of every residue code
                if (aa > 20u || (w & 7u) != 7u) bad = 1;
                const uint32_t oxt = (A == 37 && l0 + tid + 1u == len && m[36]) ? UD_OXT_BIT : 0u;
                // (packed: chains may share rows, and a row that ends one chain may lie inside another -- the OXT is counted here
                // and found again by the fill pass from the chain's atom count, the row's word says nothing of it)
                row_word[row0 + tid] = (uint16_t)(RA::packed ? w : w | oxt);
                cnt += __popc(w | oxt);
            }
            __syncthreads();   // the next tile rewrites the staging
        }
        cnt = wave_sum(cnt); bad = wave_sum(bad);
        if (lane == 0) { s_cnt[wave] = cnt; s_bad[wave] = bad; }
        __syncthreads();
        if (tid == 0) {
            const uint32_t total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
            const int st = too_long ? FCZ_E_INVALID_ARG : ((s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3]) ? FCZ_E_RESIDUE : FCZ_OK);
            n_res[c] = st ? 0u : len; n_atoms[c] = st ? 0u : total; status[c] = st;
            if constexpr (RA::packed) chain_tiles[c] = st ? 0u : (len + DN_TILE - 1u) / DN_TILE;
        }
        __syncthreads();
    }
}

template <int A, class RA>
__global__ __launch_bounds__(BLOCK) void k_undense_fill(undense_in g, RA ra, undense_table tab,
                                                        const uint16_t* __restrict__ row_word, const uint32_t* __restrict__ res_off,
                                                        const uint32_t* __restrict__ chain_atom_off, undense_out o) {
    __shared__ __attribute__((aligned(16))) float s_pos[DN_TILE * A * 3 + 4];
    __shared__ uint32_t s_pk[DN_TILE];                 // row word | residue code << 16
    __shared__ uint32_t s_first[DN_TILE];              // tile-local first atom of the row
    __shared__ uint32_t s_part[WAVES_PER_BLOCK];       // per-wave sums of the atoms in front of the tile
    __shared__ uint8_t s_slot[FCZ_N_RES_CODES * FCZ_MAX_RES_ATOMS], s_code[FCZ_N_RES_CODES * FCZ_MAX_RES_ATOMS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t i = tid; i < FCZ_N_RES_CODES * FCZ_MAX_RES_ATOMS; i += BLOCK) {
        s_slot[i] = tab.slot[i];
        s_code[i] = fcz_res_atom[i / FCZ_MAX_RES_ATOMS][i % FCZ_MAX_RES_ATOMS];
    }
    __syncthreads();
    const uint64_t n_tiles = ra.n_tiles();
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        uint32_t c, l0;
        ra.tile(tile, &c, &l0);
        const uint32_t r0 = res_off[c], ne = res_off[c + 1] - r0;               // ne <= L; 0 for a refused chain
        if (l0 >= ne) continue;                                                 // padding only: two offsets loaded, nothing else
        const uint32_t nv = ne - l0 < DN_TILE ? ne - l0 : DN_TILE;              // rows of the tile that hold a residue
        const uint64_t chain_row = ra.base(c), row0 = chain_row + l0;
        const float* pp = g.pos + row0 * (uint64_t)(A * 3);
        float* img = s_pos + ud_misalign(pp);
        ud_stage(pp, nv * (uint32_t)(A * 3), img);
        // atoms of the chain in front of the tile (block sum; the OXT bit is set on the chain's last row only, never in front)
        uint32_t part = 0;
        for (uint32_t k = tid; k < l0; k += BLOCK) part += __popc((uint32_t)row_word[chain_row + k]);
        part = wave_sum(part);
        if (lane == 0) s_part[wave] = part;
        uint32_t my_rc = FCZ_RES_UNK, my_first = 0;
        if (wave == 0) {
            uint32_t w = 0;
            if (lane < nv) { w = row_word[row0 + lane]; my_rc = ud_res_code(g.aatype[row0 + lane]); }
            uint32_t tot;
            my_first = wave_excl_scan((uint32_t)__popc(w), (int)lane, &tot);
            s_pk[lane] = w | (my_rc << 16);
            s_first[lane] = my_first;
        }
        __syncthreads();
        const uint32_t a0 = chain_atom_off[c], aend = chain_atom_off[c + 1];
        const uint32_t base = a0 + s_part[0] + s_part[1] + s_part[2] + s_part[3];
        if (tid < nv) {   // wavefront 0: lane = row
            const uint32_t r = r0 + l0 + tid;
            o.atom_off[r] = base + my_first;
            o.res_code[r] = (uint8_t)my_rc;
            o.bfac_ca[r] = g.plddt ? g.plddt[row0 + tid] : 0.0f;
            if (l0 + tid + 1u == ne) o.atom_off[r + 1u] = aend;                 // (the next chain with residues writes the same value)
        }
        for (uint32_t it = tid; it < nv * UD_ITEMS; it += BLOCK) {
            const uint32_t lr = it / UD_ITEMS, j = it - lr * UD_ITEMS;
            const uint32_t pk = s_pk[lr];
            uint32_t w = pk & 0xFFFFu;
            if constexpr (RA::packed)     // the chain's OXT: its last row, and the chain has one more atom than its rows' words own
                if (A == 37 && l0 + lr + 1u == ne && base + s_first[lr] + (uint32_t)__popc(w) + 1u == aend) w |= UD_OXT_BIT;
            if (!((w >> j) & 1u)) continue;
            const uint32_t rc = pk >> 16;
            const bool oxt = j == (uint32_t)FCZ_MAX_RES_ATOMS;                    // set for atom37 only
            const uint32_t slot = oxt ? 36u : s_slot[rc * FCZ_MAX_RES_ATOMS + j];
            const uint32_t a = base + s_first[lr] + (uint32_t)__popc(w & ((1u << j) - 1u));
            if (a < aend) {                                                     // (holds by construction: both sides are sums of the row words)
                const float* s = img + (lr * (uint32_t)A + slot) * 3u;
                o.x[a] = s[0]; o.y[a] = s[1]; o.z[a] = s[2];
                o.atom_code[a] = oxt ? (uint8_t)FCZ_ATOM_OXT : s_code[rc * FCZ_MAX_RES_ATOMS + j];
            }
        }
        __syncthreads();   // the next tile rewrites the staging
    }
}

// defaults of the per-chain metadata the caller left out
__global__ __launch_bounds__(BLOCK) void k_undense_defaults(uint32_t n, int32_t* __restrict__ first_res, int32_t* __restrict__ first_atom,
                                                            char* __restrict__ chain_id) {
    const uint32_t c = blockIdx.x * BLOCK + threadIdx.x;
    if (c >= n) return;
    if (first_res) first_res[c] = 1;
    if (first_atom) first_atom[c] = 1;
    if (chain_id) chain_id[c] = 'A';
}

// a chain this stage refused keeps that verdict over the one the pack kernels reach for its empty residue range (FCZ_E_TOO_SHORT)
__global__ __launch_bounds__(BLOCK) void k_undense_merge_status(uint32_t n, const int32_t* __restrict__ refused, int32_t* __restrict__ status) {
    const uint32_t c = blockIdx.x * BLOCK + threadIdx.x;
    if (c < n && refused[c] != FCZ_OK) status[c] = refused[c];
}

}  // namespace fcz
