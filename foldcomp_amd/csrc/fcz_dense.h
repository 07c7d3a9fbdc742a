// fcz_dense.h -- decoded atoms -> dense padded model-input tensors (atom37 / atom14 / backbone4) on the device.
// The reference has no such output (Foldcomp::decompress, src/foldcomp.cpp:779, ends at a flat vector<AtomCoordinate>); the
// layouts are the ones protein models read: pos [n][L][A][3] float32, mask [n][L][A] uint8, aatype / plddt / res_index [n][L],
// length [n] (include/fcz_hip.h, fcz_dense_out).
//
// A gather whose cost is its stores (481 B written per atom37 residue against ~95 B read), so the OUTPUT index space is the work:
//
//   k_dense<A>   persistent blocks over tiles of DN_TILE = 64 residue rows of one entry. A tile is one contiguous byte range of
//                every output array; lane = output element, consecutive lanes = consecutive addresses, 16 bytes per lane
//                (the few floats / bytes in front of and behind the 16-byte boundaries of the range leave as single stores), and
//                every byte of every array -- padding included -- is written exactly once. No clear in front, no scatter behind.
//                A tile that holds residues stages them first: the residues' codes and first-atom offsets (one wave scan of
//                fcz_res_natoms over the tile, on top of the block's sum over the entry's residues in front of the tile), then
//                the tile's atoms (one contiguous range of x / y / z: coalesced loads into LDS, 12 B per atom, read once). The
//                source of slot (l, a) is then LDS[first_atom[l] + inv[res_code[l]][a]]; inv is the constant table the host
//                builds for the layout and the decode order (fcz_dense_slot) and hands over by value.
//                A tile past the entry's end (padding, a skipped entry) loads two offsets and stores constants.
//   k_dense_window<A>   the same tile loop with the entry's row origin moved by a per-entry start (a crop at an offset), below.
//
// The per-residue first-atom offset is not taken from a pass of its own: that pass needs a buffer of one word per residue of the
// batch, and the device entry point knows the batch's residue count only on the device (no synchronisation on this path). The
// prefix is one byte per residue in front of the tile, read from L2 (the entry's tiles share them): 0.5 % of the tile's stores at
// 350 residues, 3 % at 2 000.
#pragma once
#include "fcz_kernels.h"

namespace fcz {

constexpr uint32_t DN_TILE = 64;                                  // residue rows per tile (one wavefront scans a tile's residues)
constexpr uint32_t DN_MAX_ATOMS = DN_TILE * FCZ_MAX_RES_ATOMS;    // atoms a tile can hold; index DN_MAX_ATOMS is the chain's OXT
constexpr uint32_t DN_MAX_WIDTH = 37;
// write-once stream: non-temporal stores measured against plain ones, the faster kept
#ifndef FCZ_DENSE_NT
#define FCZ_DENSE_NT 1
#endif

// what the readers of the dense tensors state their float32 contracts with (fcz_knn.h, fcz_frames.h, fcz_lddt.h): the correctly rounded
// float32 quotient and square root. double has more than 2 * 24 + 2 bits, so the double result rounded to float is the float result
// rounded once.
__host__ __device__ __forceinline__ float f32_div_rn(float a, float b) { return (float)((double)a / (double)b); }
__host__ __device__ __forceinline__ float f32_sqrt_rn(float a) { return (float)sqrt((double)a); }

typedef float dn_f4 __attribute__((ext_vector_type(4)));
typedef uint32_t dn_u4 __attribute__((ext_vector_type(4)));

// inv[res_code * A + slot] = position of the slot's atom among the residue's decoded atoms, 255 = the residue has none
struct dense_table { uint8_t inv[FCZ_N_RES_CODES * DN_MAX_WIDTH]; };

struct dense_args {
    const uint64_t* off; const uint32_t* res_off; const uint32_t* atom_off;
    const float* x; const float* y; const float* z; const float* bfac; const uint8_t* res_code;
    float* pos; uint8_t* mask; uint8_t* aatype; float* plddt; int32_t* res_index; uint32_t* length;
};

template <class V, class T> __device__ __forceinline__ void dn_store(T* p, V v) {
#if FCZ_DENSE_NT
    __builtin_nontemporal_store(v, reinterpret_cast<V*>(p));
#else
    *reinterpret_cast<V*>(p) = v;
#endif
}

// `count` elements of T at p, element t = val(t): 16-byte stores over the aligned middle of the range, single elements in
// front of it and behind it. Lane = 16 consecutive bytes, consecutive lanes = consecutive addresses. The work is shared by `stride`
// threads, this one being number idx of them: a block (the default) or one wavefront (idx = lane, stride = WAVE).
template <class T, class F> __device__ __forceinline__ void dn_emit(T* p, uint32_t count, F val, const uint32_t idx = threadIdx.x, const uint32_t stride = BLOCK) {
    constexpr uint32_t PER = 16 / sizeof(T);
    const uint32_t mis = (uint32_t)((uintptr_t)p & 15u) / (uint32_t)sizeof(T);
    uint32_t head = (PER - mis) % PER;
    if (head > count) head = count;
    const uint32_t body = (count - head) / PER, tail0 = head + body * PER;
    for (uint32_t q = idx; q < body; q += stride) {
        const uint32_t t = head + q * PER;
        if constexpr (sizeof(T) == 4) {
            dn_f4 v;
            v.x = val(t); v.y = val(t + 1); v.z = val(t + 2); v.w = val(t + 3);
            dn_store(p + t, v);
        } else {
            uint32_t w[4];
#pragma unroll
            for (int i = 0; i < 4; i++)
                w[i] = (uint32_t)val(t + 4 * i) | ((uint32_t)val(t + 4 * i + 1) << 8) | ((uint32_t)val(t + 4 * i + 2) << 16) | ((uint32_t)val(t + 4 * i + 3) << 24);
            dn_u4 v; v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
            dn_store(p + t, v);
        }
    }
    if (idx < head) p[idx] = val(idx);
    if (idx < count - tail0) p[tail0 + idx] = val(tail0 + idx);
}

// the tile loop of k_dense (WIN = false: start is not read) and of k_dense_window (WIN = true: row l of entry e holds residue
// w0 + l, w0 = min(start[e], the entry's length); start == NULL is all zeros)
template <int A, bool WIN>
__device__ __forceinline__ void dense_tiles(const uint8_t* __restrict__ blob, const dense_args g, const uint32_t* __restrict__ start, uint32_t L,
                                            uint32_t tiles_per_entry, uint64_t n_tiles, const dense_table tab) {
    __shared__ float s_xyz[3][DN_MAX_ATOMS + 1];
    __shared__ uint32_t s_pk[DN_TILE];                 // tile-local first atom | residue code << 16
    __shared__ uint32_t s_part[WAVES_PER_BLOCK + 1];   // per-wave sums of the atoms in front of the tile; [4] = atoms of the tile
    __shared__ uint8_t s_inv[FCZ_N_RES_CODES * A];
    __shared__ uint8_t s_na[FCZ_N_RES_CODES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t i = tid; i < FCZ_N_RES_CODES * A; i += BLOCK) s_inv[i] = tab.inv[i];
    if (tid < FCZ_N_RES_CODES) s_na[tid] = fcz_res_natoms[tid];
    __syncthreads();
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t e = (uint32_t)(tile / tiles_per_entry);
        const uint32_t l0 = (uint32_t)(tile - (uint64_t)e * tiles_per_entry) * DN_TILE;
        const uint32_t r0 = g.res_off[e], ne = g.res_off[e + 1] - r0;
        // first residue of the window, clamped to the entry's length: w0 + l never wraps, a start at or behind the end leaves padding only
        uint32_t w0 = 0;
        if constexpr (WIN) { w0 = start ? start[e] : 0u; if (w0 > ne) w0 = ne; }
        const uint32_t len = ne - w0 < L ? ne - w0 : L;                      // rows of the entry that hold a residue (cropped to L)
        const uint32_t rows = L - l0 < DN_TILE ? L - l0 : DN_TILE;             // rows of the tile
        const uint32_t nv = l0 < len ? (len - l0 < DN_TILE ? len - l0 : DN_TILE) : 0u;   // of them, rows that hold a residue
        const uint64_t row0 = (uint64_t)e * L + l0;
        float* pos = g.pos + row0 * (uint64_t)(A * 3);
        uint8_t* mask = g.mask + row0 * (uint64_t)A;
        if (l0 == 0 && tid == 0 && g.length) g.length[e] = ne;
        if (nv == 0) {   // padding only: constants, no loads
            dn_emit(pos, rows * (uint32_t)(A * 3), [](uint32_t) { return 0.0f; });
            dn_emit(mask, rows * (uint32_t)A, [](uint32_t) { return (uint8_t)0; });
            if (tid < rows) {
                if (g.aatype) g.aatype[row0 + tid] = 20;
                if (g.plddt) g.plddt[row0 + tid] = 0.0f;
                if (g.res_index) g.res_index[row0 + tid] = 0;
            }
            continue;
        }
        // atoms of the entry in front of the tile (block sum), first atom of every residue of the tile (scan by wavefront 0)
        uint32_t part = 0;
        for (uint32_t k = tid; k < w0 + l0; k += BLOCK) { const uint32_t rc = g.res_code[r0 + k]; part += s_na[rc < 24u ? rc : 23u]; }
        part = wave_sum(part);
        if (lane == 0) s_part[wave] = part;
        uint32_t my_rc = 23;
        if (wave == 0) {
            uint32_t na = 0;
            if (lane < nv) { my_rc = g.res_code[r0 + w0 + l0 + lane]; if (my_rc >= 24u) my_rc = 23u; na = s_na[my_rc]; }
            uint32_t tot;
            const uint32_t ex = wave_excl_scan(na, (int)lane, &tot);
            s_pk[lane] = ex | (my_rc << 16);
            if (lane == 0) s_part[WAVES_PER_BLOCK] = tot;
        }
        __syncthreads();
        const uint32_t pre = s_part[0] + s_part[1] + s_part[2] + s_part[3];
        const uint32_t count = s_part[WAVES_PER_BLOCK];                        // <= DN_MAX_ATOMS: at most 14 atoms per residue code
        const uint32_t a0 = g.atom_off[e], aend = g.atom_off[e + 1];
        const uint32_t base = a0 + pre;
        // (a read never leaves the entry's own atom range, whatever the residue codes say)
        for (uint32_t i = tid; i < count; i += BLOCK) {
            const bool ok = base + i < aend;
            s_xyz[0][i] = ok ? g.x[base + i] : 0.0f; s_xyz[1][i] = ok ? g.y[base + i] : 0.0f; s_xyz[2][i] = ok ? g.z[base + i] : 0.0f;
        }
        // the chain's OXT: the decoder's last atom when the entry has one more atom than its residues own; slot 36 of the last
        // residue in atom37, no slot elsewhere (and none when the crop dropped the last residue)
        const bool last_here = w0 + l0 + nv == ne;
        const bool oxt = A == 37 && last_here && aend - a0 == pre + count + 1u;
        const uint32_t oxt_row = oxt ? nv - 1u : 0xFFFFFFFFu;
        if (oxt && tid < 3) s_xyz[tid][DN_MAX_ATOMS] = (tid == 0 ? g.x : tid == 1 ? g.y : g.z)[aend - 1u];
        __syncthreads();
        auto src = [&](uint32_t lr, uint32_t a) -> uint32_t {                   // LDS index of the atom in slot (lr, a), ~0u = none
            if (lr >= nv) return 0xFFFFFFFFu;
            if (A == 37 && a == 36u) return lr == oxt_row ? DN_MAX_ATOMS : 0xFFFFFFFFu;
            const uint32_t pk = s_pk[lr];
            const uint32_t j = s_inv[(pk >> 16) * (uint32_t)A + a];
            const uint32_t i = (pk & 0xFFFFu) + j;
            return (j != 255u && i < count) ? i : 0xFFFFFFFFu;
        };
        dn_emit(pos, rows * (uint32_t)(A * 3), [&](uint32_t t) {
            const uint32_t s = t / 3u, c = t - 3u * s, lr = s / (uint32_t)A, a = s - lr * (uint32_t)A;
            const uint32_t i = src(lr, a);
            return i != 0xFFFFFFFFu ? s_xyz[c][i] : 0.0f;
        });
        dn_emit(mask, rows * (uint32_t)A, [&](uint32_t s) {
            const uint32_t lr = s / (uint32_t)A, a = s - lr * (uint32_t)A;
            return (uint8_t)(src(lr, a) != 0xFFFFFFFFu ? 1 : 0);
        });
        if (tid < rows) {   // wavefront 0: lane = row, my_rc is the row's residue code
            const bool res = tid < nv;
            if (g.aatype) g.aatype[row0 + tid] = (uint8_t)(res && my_rc < 20u ? my_rc : 20u);
            if (g.plddt) g.plddt[row0 + tid] = res ? g.bfac[r0 + w0 + l0 + tid] : 0.0f;
            if (g.res_index) g.res_index[row0 + tid] = res ? (int32_t)(ld_u16(blob + g.off[e] + 8) + w0 + l0 + tid) : 0;
        }
        __syncthreads();   // the next tile rewrites the staging
    }
}

template <int A>
__global__ __launch_bounds__(BLOCK) void k_dense(const uint8_t* __restrict__ blob, dense_args g, uint32_t n_entries, uint32_t L,
                                                 uint32_t tiles_per_entry, uint64_t n_tiles, dense_table tab) {
    dense_tiles<A, false>(blob, g, nullptr, L, tiles_per_entry, n_tiles, tab);
}

//   k_dense_window<A>   k_dense with a per-entry row origin (include/fcz_hip.h, fcz_dense_window_dev): the tile is still 64 output
//                       rows of one entry and one contiguous byte range of every output array; the residues read, the block's prefix
//                       sum in front of the tile and the test for the chain's last residue move by start[e]. The prefix now runs over
//                       start + l0 bytes whatever l0 is: a window at the end of a 2 700-residue chain reads 2.7 KB of residue codes
//                       per tile from L2, 9 % of the tile's 30 KB of stores.
template <int A>
__global__ __launch_bounds__(BLOCK) void k_dense_window(const uint8_t* __restrict__ blob, dense_args g, const uint32_t* __restrict__ start,
                                                        uint32_t n_entries, uint32_t L, uint32_t tiles_per_entry, uint64_t n_tiles, dense_table tab) {
    dense_tiles<A, true>(blob, g, start, L, tiles_per_entry, n_tiles, tab);
}

// ---- packed form: rows of all entries back to back, no padding (include/fcz_hip.h, fcz_packed_out) ----------------------------
//
//   k_dense_packed<A>   persistent blocks over tiles of DN_TILE consecutive rows of the FLAT row space 0 .. R - 1, R = res_off[n]
//                       read in the kernel (the entry point knows it only on the device). A tile may span any number of entries:
//                       every row finds its entry by a binary search of res_off (entries without rows are passed over by it), and
//                       its first atom restarts at atom_off[e] for every entry that begins inside the tile -- a chain's OXT lies
//                       between its last residue's atoms and the next entry's first. The tile's atoms, OXTs included, are still
//                       ONE contiguous range of x / y / z: staged once, up to DN_TILE chain ends wide. Every row keeps the clamp
//                       against its own entry's atom range. length[e] has no tile of its own: a grid-stride loop over n writes it.

constexpr uint32_t DN_PACKED_ATOMS = DN_MAX_ATOMS + DN_TILE;      // atoms a packed tile can hold: every row may end a chain

// the entry of flat row r: the largest e in [lo, n) with res_off[e] <= r (res_off[lo] <= r < res_off[n])
__device__ __forceinline__ uint32_t dn_entry_of(const uint32_t* __restrict__ res_off, uint32_t lo, uint32_t n, uint32_t r) {
    uint32_t hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (res_off[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}

template <int A>
__global__ __launch_bounds__(BLOCK) void k_dense_packed(const uint8_t* __restrict__ blob, dense_args g, int32_t* __restrict__ chain_index,
                                                        uint32_t n_entries, dense_table tab) {
    __shared__ float s_xyz[3][DN_PACKED_ATOMS];
    __shared__ uint32_t s_pk[DN_TILE];                 // tile-local first atom | atoms of the row's entry inside the staging << 10 | residue code << 20 | OXT << 25
    __shared__ uint32_t s_part[WAVES_PER_BLOCK];       // per-wave sums of the atoms of the first entry in front of the tile
    __shared__ uint32_t s_end[3];                      // end of the tile's atom range: value, "add the prefix" flag, clamp
    __shared__ uint8_t s_inv[FCZ_N_RES_CODES * A];
    __shared__ uint8_t s_na[FCZ_N_RES_CODES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t R = g.res_off[n_entries];
    const uint32_t n_tiles = R / DN_TILE + (R % DN_TILE ? 1u : 0u);
    if (g.length)
        for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + tid; e < n_entries; e += (uint64_t)gridDim.x * BLOCK) g.length[e] = g.res_off[e + 1] - g.res_off[e];
    if (blockIdx.x >= n_tiles) return;
    for (uint32_t i = tid; i < FCZ_N_RES_CODES * A; i += BLOCK) s_inv[i] = tab.inv[i];
    if (tid < FCZ_N_RES_CODES) s_na[tid] = fcz_res_natoms[tid];
    __syncthreads();
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t t0 = tile * DN_TILE;
        const uint32_t rows = R - t0 < DN_TILE ? R - t0 : DN_TILE;              // every row of a packed tile holds a residue
        const uint32_t e0 = dn_entry_of(g.res_off, 0u, n_entries, t0);          // the entry of the tile's first row
        float* pos = g.pos + (uint64_t)t0 * (uint64_t)(A * 3);
        uint8_t* mask = g.mask + (uint64_t)t0 * (uint64_t)A;
        // atoms of entry e0 in front of the tile (block sum); per row: its entry, its first atom (scan by wavefront 0, restarted
        // at atom_off[e] where an entry begins inside the tile)
        uint32_t part = 0;
        for (uint32_t k = g.res_off[e0] + tid; k < t0; k += BLOCK) { const uint32_t rc = g.res_code[k]; part += s_na[rc < 24u ? rc : 23u]; }
        part = wave_sum(part);
        if (lane == 0) s_part[wave] = part;
        uint32_t my_e = 0, my_l = 0, my_rc = 23, my_na = 0, my_first = 0, my_aend = 0;
        bool my_last = false;
        if (wave == 0) {
            const bool act = lane < rows;
            const uint32_t r = t0 + (act ? lane : 0u);
            my_e = dn_entry_of(g.res_off, e0, n_entries, r);
            const uint32_t rs = g.res_off[my_e];
            my_l = r - rs;
            my_last = act && r + 1u == g.res_off[my_e + 1];
            if (act) { my_rc = g.res_code[r]; if (my_rc >= 24u) my_rc = 23u; my_na = s_na[my_rc]; }
            uint32_t tot;
            const uint32_t ex = wave_excl_scan(my_na, (int)lane, &tot);
            const uint32_t ex_start = __shfl(ex, (int)(rs > t0 ? rs - t0 : 0u), WAVE);   // the scan at the entry's first row in the tile
            my_aend = g.atom_off[my_e + 1];
            my_first = g.atom_off[my_e] + (ex - ex_start);                     // (+ the prefix for the rows of e0, below)
            if (lane == rows - 1u) { s_end[0] = my_last ? my_aend : my_first + my_na; s_end[1] = (my_e == e0 && !my_last) ? 1u : 0u; s_end[2] = my_aend; }
        }
        __syncthreads();
        const uint32_t pre = s_part[0] + s_part[1] + s_part[2] + s_part[3];
        const uint32_t g0 = g.atom_off[e0] + pre;                              // first atom of the tile's first row
        uint32_t g1 = s_end[0] + (s_end[1] ? pre : 0u);                        // behind the last row's atoms (and its chain's OXT)
        if (g1 > s_end[2]) g1 = s_end[2];                                      // (a read never leaves the last entry's atom range)
        const uint32_t count = g1 > g0 ? (g1 - g0 < DN_PACKED_ATOMS ? g1 - g0 : DN_PACKED_ATOMS) : 0u;
        for (uint32_t i = tid; i < count; i += BLOCK) { s_xyz[0][i] = g.x[g0 + i]; s_xyz[1][i] = g.y[g0 + i]; s_xyz[2][i] = g.z[g0 + i]; }
        if (wave == 0) {
            if (my_e == e0) my_first += pre;
            uint32_t first = my_first - g0;                                    // (wraps for inconsistent offsets: clamped, selects nothing)
            if (first > 1023u) first = 1023u;
            uint32_t lim = my_aend > g0 ? my_aend - g0 : 0u;                   // the row's entry ends here: base + i < aend, per entry
            if (lim > count) lim = count;
            // the chain's OXT: the entry has one more atom than its residues own; slot 36 of its last row in atom37
            const bool oxt = A == 37 && my_last && my_aend == my_first + my_na + 1u && first + my_na < count;
            s_pk[lane] = lane < rows ? (first | (lim << 10) | (my_rc << 20) | (oxt ? 1u << 25 : 0u)) : 0u;
        }
        __syncthreads();
        auto src = [&](uint32_t lr, uint32_t a) -> uint32_t {                   // LDS index of the atom in slot (lr, a), ~0u = none
            const uint32_t pk = s_pk[lr], first = pk & 1023u, rc = (pk >> 20) & 31u;
            if (A == 37 && a == 36u) return ((pk >> 25) & 1u) ? first + s_na[rc] : 0xFFFFFFFFu;
            const uint32_t j = s_inv[rc * (uint32_t)A + a];
            const uint32_t i = first + j;
            return (j != 255u && i < ((pk >> 10) & 1023u)) ? i : 0xFFFFFFFFu;
        };
        dn_emit(pos, rows * (uint32_t)(A * 3), [&](uint32_t t) {
            const uint32_t s = t / 3u, c = t - 3u * s, lr = s / (uint32_t)A, a = s - lr * (uint32_t)A;
            const uint32_t i = src(lr, a);
            return i != 0xFFFFFFFFu ? s_xyz[c][i] : 0.0f;
        });
        dn_emit(mask, rows * (uint32_t)A, [&](uint32_t s) {
            const uint32_t lr = s / (uint32_t)A, a = s - lr * (uint32_t)A;
            return (uint8_t)(src(lr, a) != 0xFFFFFFFFu ? 1 : 0);
        });
        if (tid < rows) {   // wavefront 0: lane = row
            const uint64_t r = (uint64_t)t0 + tid;
            if (g.aatype) g.aatype[r] = (uint8_t)(my_rc < 20u ? my_rc : 20u);
            if (g.plddt) g.plddt[r] = g.bfac[r];
            if (g.res_index) g.res_index[r] = (int32_t)(ld_u16(blob + g.off[my_e] + 8) + my_l);
            if (chain_index) chain_index[r] = (int32_t)my_e;
        }
        __syncthreads();   // the next tile rewrites the staging
    }
}

}  // namespace fcz
