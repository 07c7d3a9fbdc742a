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
//
// The skeleton every sweep kernel is built on lives here once; the kernels keep their LDS arrays, their sweep over the staged
// candidates and their epilogue:
//   chain_tile<PACKED>     the head of a kernel's tile loop: the tile's chain, its rows and the tile's first row (chain_tile_count
//                          ends the loop).
//   chain_stage_rows       one candidate pass of PASS chain rows, a row a lane and step (k_knn, k_lddt, k_hbond).
//   chain_stage_ordered    the same pass with a row's slot fixed by its place in the pass, for a sweep that sums floats in row order
//                          (k_lddt_soft, k_lddt_soft_grad).
//   chain_stage_slots      one candidate pass of at most PASS atoms, staged in steps of the rows that hold at most STEP slots
//                          (k_sasa_points, k_violations, k_lddt_atoms).
//   chain_stage_slots_ordered   the same pass compacted in ascending (row, slot) by ballots and a scan of the wavefronts' totals, for a
//                          sweep that sums floats over atoms (k_violation_loss, k_violation_loss_grad).
//                          chain_stage_rows and chain_stage_slots hand the caller's functor a row (and slot) and a chain_slots; the
//                          functor decides whether that is a candidate, claims a slot with next() and writes its own LDS arrays;
//                          the ordered two hand out the slot themselves. All four hold barriers, so all BLOCK
//                          threads call them under block-uniform control flow and no functor holds a barrier. The barrier that
//                          closes a pass, behind the caller's sweep, stays in the caller.
//   chain_tile_slots       the slots of a query tile of whole rows, strided over the block.
//   k_chain_fill<Args>     packed form only, in front of a sweep: chain_empty_row(g, r), which every analysis defines beside its
//                          args, for every row that no chain is seen to cover.
//   chain_d2, chain_div_a, chain_site, chain_site2, chain_atom     the arithmetic and the "is this a site / an atom" rules.
#pragma once
#include "fcz_dense.h"

namespace fcz {

constexpr uint32_t CHAIN_TILE = BLOCK;      // query rows per tile (a lane per query)
constexpr uint32_t CHAIN_TYPES = 21;

struct chain_radii { float radius[CHAIN_TYPES * DN_MAX_WIDTH]; };   // [min(aatype, 20)][slot] with rows of A floats

// x / A for the three widths there are, without a division by a variable
__device__ __forceinline__ uint32_t chain_div_a(uint32_t x, uint32_t A) { return A == 37u ? x / 37u : A == 14u ? x / 14u : x / 4u; }
// the divider of a staging over the slots of a layout (chain_stage_slots_ordered's default); a sweep over rows of another width
// brings its own (fcz_fape_atoms.h: the eight rigid groups of a row)
struct chain_div_layout { __device__ __forceinline__ uint32_t operator()(uint32_t x, uint32_t A) const { return chain_div_a(x, A); } };

// float32, every operation rounded, no FMA. d2(a, b) == d2(b, a) bit for bit: the differences are negated, the squares are the same.
__device__ __forceinline__ float chain_d2(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by), dz = __fsub_rn(az, bz);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}
__device__ __forceinline__ float chain_d2(const float* a, const float* b) { return chain_d2(a[0], a[1], a[2], b[0], b[1], b[2]); }

// the three coordinates of element o (= row * A + slot) of a tensor -> true when they are finite
__device__ __forceinline__ bool chain_xyz(const float* pos, uint64_t o, float* c) {
    const float* p = pos + o * 3u;
    c[0] = p[0]; c[1] = p[1]; c[2] = p[2];
    return isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]);
}

// element o of one tensor -> true when its mask is set and its three coordinates are finite
__device__ __forceinline__ bool chain_site(const float* pos, const uint8_t* mask, uint64_t o, float* c) { return mask[o] != 0 && chain_xyz(pos, o, c); }

// element ot of the truth and op of the prediction -> true when both masks are set (a NULL mask_pred is all set) and the six
// coordinates are finite; with both masks set the six are loaded whatever they hold
__device__ __forceinline__ bool chain_site2(const float* pos_true, const uint8_t* mask_true, uint64_t ot, const float* pos_pred, const uint8_t* mask_pred,
                                            uint64_t op, float* t, float* p) {
    if (mask_true[ot] == 0) return false;
    if (mask_pred && mask_pred[op] == 0) return false;
    const bool ft = chain_xyz(pos_true, ot, t), fp = chain_xyz(pos_pred, op, p);
    return ft && fp;
}

// slot a of array row r (a row inside its chain) of g.pos / g.mask / g.aatype -> true when it is an ATOM: mask set, a non-zero radius
// in tab[min(aatype, 20)][a] and three finite coordinates. c = (x, y, z, that radius), ty = the clamped aatype (0 without aatype).
template <class Args>
__device__ __forceinline__ bool chain_atom(const Args& g, const chain_radii& tab, uint64_t r, uint32_t a, float4* c, uint32_t* ty) {
    if (g.mask[r * g.A + a] == 0) return false;
    const uint32_t aa = g.aatype ? g.aatype[r] : 0u;
    *ty = aa > 20u ? 20u : aa;
    const float radius = tab.radius[*ty * g.A + a];
    if (radius == 0.0f) return false;
    float p[3];
    if (!chain_xyz(g.pos, r * g.A + a, p)) return false;
    *c = make_float4(p[0], p[1], p[2], radius);
    return true;
}

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

// packed form only, in front of a sweep: what an empty row holds into every row that no chain is seen to cover
template <class Args>
__global__ __launch_bounds__(BLOCK) void k_chain_fill(Args g) {
    for (uint64_t r = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; r < g.L; r += (uint64_t)gridDim.x * BLOCK) {
        if (chain_covers(g.bound, g.n, r)) continue;
        chain_empty_row(g, r);
    }
}

// the tiles of a launch: a sweep kernel's last three arguments are tile_off, tiles_per_entry and the padded form's tile count
template <bool PACKED>
__device__ __forceinline__ uint64_t chain_tile_count(const uint64_t* __restrict__ tile_off, uint32_t n, uint64_t n_tiles_padded) {
    return PACKED ? tile_off[n] : n_tiles_padded;
}

// query tile `tile` of tile_rows rows: its chain e and number t inside the chain, the chain's range (chain_range) and q0, the tile's
// first row of the chain
template <bool PACKED>
struct chain_tile {
    uint32_t e, t, len, rows;
    uint64_t row0, q0;
    __device__ __forceinline__ chain_tile(const uint64_t* __restrict__ tile_off, uint32_t n, uint32_t tiles_per_entry, const uint32_t* __restrict__ bound,
                                          uint32_t L, uint64_t tile, uint32_t tile_rows) {
        chain_of_tile<PACKED>(tile_off, n, tiles_per_entry, tile, &e, &t);
        chain_range<PACKED>(bound, L, e, &row0, &len, &rows);
        q0 = (uint64_t)t * tile_rows;
    }
};

// The slots of a candidate pass, handed out by an LDS counter: the order inside a pass is free, because every result of a sweep is
// an integer or a key with a total order.
struct chain_slots {
    uint32_t* count;
    __device__ __forceinline__ uint32_t next() const { return atomicAdd(count, 1u); }
};

// One candidate pass of PASS chain rows from row *c0 of a chain of len rows: site(r, slots) for every row r of the pass, a row a lane
// and step. A site claims at most one slot, so next() stays below PASS. -> the staged count; *c0 becomes the next pass' first row.
// The caller sweeps the pass and closes it with a barrier before it stages the next.
template <uint32_t PASS, class Site>
__device__ __forceinline__ uint32_t chain_stage_rows(uint32_t* s_count, uint32_t len, uint32_t* c0, Site site) {
    const uint32_t c1 = len - *c0 < PASS ? len : *c0 + PASS;
    if (threadIdx.x == 0) *s_count = 0;
    __syncthreads();
    for (uint64_t r = (uint64_t)*c0 + threadIdx.x; r < c1; r += BLOCK) site(r, chain_slots{s_count});
    __syncthreads();
    *c0 = c1;
    return *s_count;
}

// The ordered sibling of chain_stage_rows, for a sweep whose result is a float sum and so depends on the order the candidates are met
// in (k_lddt_soft): one candidate pass of PASS chain rows from row *c0, row(r, r - *c0) for EVERY row r of the pass, a row a lane and
// step -- the slot is the row's place in the pass, and the functor marks in its own arrays a row that is no candidate. There is no
// counter, so no barrier in front: the caller's barrier that closed the pass before has freed the staging. -> the rows staged; *c0
// becomes the next pass' first row. The caller sweeps the pass and closes it with a barrier before it stages the next.
template <uint32_t PASS, class Row>
__device__ __forceinline__ uint32_t chain_stage_ordered(uint32_t len, uint32_t* c0, Row row) {
    const uint32_t first = *c0, c1 = len - first < PASS ? len : first + PASS;
    for (uint64_t r = (uint64_t)first + threadIdx.x; r < c1; r += BLOCK) row(r, (uint32_t)(r - first));
    __syncthreads();
    *c0 = c1;
    return c1 - first;
}

// One candidate pass of at most PASS atoms from row *r0 of a chain of len rows of A slots: atom(r, a, slots) for every slot a of every
// row r of the pass. The pass is staged in steps of the rows that hold at most STEP slots, STEP / BLOCK slots a lane, and is closed
// when another step might not fit, so next() stays below PASS (backbone4 with every mask set fills a pass of 1536 exactly). The
// functor keeps the identity of a candidate as (r, a): r * A + a in one word would wrap for chains above 2^32 / 37 rows.
// -> the staged count; *r0 becomes the next pass' first row. The caller sweeps the pass and closes it with a barrier.
template <uint32_t PASS, uint32_t STEP, class Atom>
__device__ __forceinline__ uint32_t chain_stage_slots(uint32_t* s_count, uint32_t A, uint32_t len, uint32_t* r0, Atom atom) {
    static_assert(STEP % BLOCK == 0 && PASS % STEP == 0, "chain_stage_slots");
    const uint32_t tid = threadIdx.x;
    const uint32_t step_rows = chain_div_a(STEP, A);                  // rows a staging step examines: 13, 36, 128 at two slots a lane
    if (tid == 0) *s_count = 0;
    __syncthreads();
    for (;;) {                                                        // steps of step_rows rows until the pass is full or the chain ends
        const uint32_t nr = len - *r0 < step_rows ? len - *r0 : step_rows;
#pragma unroll
        for (uint32_t h = 0; h < STEP / BLOCK; h++) {
            const uint32_t x = tid + h * BLOCK;
            if (x < nr * A) {
                const uint32_t rr = chain_div_a(x, A);
                atom(*r0 + rr, x - rr * A, chain_slots{s_count});
            }
        }
        *r0 += nr;
        __syncthreads();
        const uint32_t staged = *s_count;
        __syncthreads();                                              // (every lane has read the count before the next step adds to it)
        if (*r0 >= len || staged + step_rows * A > PASS) break;
    }
    return *s_count;
}

// The ordered sibling of chain_stage_slots, for a sweep whose result is a float sum over atoms and so depends on the order the
// candidates are met in (k_violation_loss, k_violation_loss_grad): one candidate pass of at most PASS atoms from row *r0, compacted
// in ASCENDING (row, slot). There is no counter to race for: is = test(r, a, h) says whether slot a of row r is a candidate and keeps
// what it loaded in the caller's registers under h (< STEP / BLOCK, the lane's h-th slot of the step), a ballot and a popcount give
// the candidate its place inside its wavefront, the wavefronts' totals of the step (s_wave [STEP / 64], one word a wavefront and h)
// are scanned by every lane, and put(h, i) writes the candidate to slot i of the caller's LDS arrays. A lane's h-th slot of a step is
// slot tid + h * BLOCK of the step, so (h, wavefront, lane) ascends with (row, slot). The steps, the rule that closes a pass and the
// barriers are chain_stage_slots': two barriers a step, all BLOCK threads under block-uniform control flow, none in a functor. There
// is no barrier in front: the caller's barrier that closed the pass before has freed the staging and s_wave.
// div(x, A) = x / A: chain_div_a for the widths of the layouts, the caller's own for rows of another width.
// -> the staged count; *r0 becomes the next pass' first row. The caller sweeps the pass and closes it with a barrier.
template <uint32_t PASS, uint32_t STEP, class Test, class Put, class Div = chain_div_layout>
__device__ __forceinline__ uint32_t chain_stage_slots_ordered(uint32_t* s_wave, uint32_t A, uint32_t len, uint32_t* r0, Test test, Put put, Div div = Div()) {
    static_assert(STEP % BLOCK == 0 && BLOCK % 64 == 0 && STEP <= PASS, "chain_stage_slots_ordered");
    constexpr uint32_t H = STEP / BLOCK, W = BLOCK / 64;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t step_rows = div(STEP, A);
    uint32_t staged = 0;
    for (;;) {
        const uint32_t nr = len - *r0 < step_rows ? len - *r0 : step_rows;
        bool is[H];
        uint32_t before[H];                                           // the candidates of this wavefront and h in front of the lane's
#pragma unroll
        for (uint32_t h = 0; h < H; h++) {
            const uint32_t x = tid + h * BLOCK;
            is[h] = false;
            if (x < nr * A) {
                const uint32_t rr = div(x, A);
                is[h] = test(*r0 + rr, x - rr * A, h);
            }
            const unsigned long long m = __ballot(is[h]);
            before[h] = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (lane == 0) s_wave[h * W + wave] = (uint32_t)__popcll(m);
        }
        __syncthreads();
        uint32_t run = staged;                                        // the place of (h, wave): the totals of every (h', w') in front of it
#pragma unroll
        for (uint32_t h = 0; h < H; h++) {
            uint32_t mine = run;
#pragma unroll
            for (uint32_t w = 0; w < W; w++) {
                const uint32_t t = s_wave[h * W + w];                 // (a broadcast read)
                mine += w < wave ? t : 0u;
                run += t;
            }
            if (is[h]) put(h, mine + before[h]);
        }
        staged = run;
        *r0 += nr;
        __syncthreads();                                              // (every lane has read s_wave before the next step rewrites it)
        if (*r0 >= len || staged + step_rows * A > PASS) break;
    }
    return staged;
}

// the slots of a query tile of tile_rows rows that begins at row q0 of its chain, strided over the block: slot(x, rr, a, q) with x the
// slot's number in the tile, rr = x / A its row of the tile, a its slot of the row and q = q0 + rr its row of the chain
template <class Slot>
__device__ __forceinline__ void chain_tile_slots(uint32_t tile_rows, uint32_t A, uint64_t q0, Slot slot) {
    for (uint32_t x = threadIdx.x; x < tile_rows * A; x += BLOCK) {
        const uint32_t rr = chain_div_a(x, A);
        slot(x, rr, x - rr * A, q0 + rr);
    }
}

}  // namespace fcz
