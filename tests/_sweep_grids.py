"""What tests/test_gpu_sweep_grids.py and tests/test_sweep_grids_cpu.py share: the grid arithmetic of the analysis launchers of
foldcomp_amd/csrc/fcz_abi.hip mirrored in Python (the idiom of test_gpu_launch_plan.py), the pools of D distinct adversarial chains
that a large batch repeats (chain e of the batch is pool chain e % D), the expansion of a pool's arrays, reference and device outputs
to the large batch in the padded and the packed form, and the three assertions every case makes:

  written    no row of an output of the large batch still holds the 0xA5 bytes it was filled with (a tile no block ran), the guards
             around it survive (the run_* helpers check them), and in the padded form every row behind a chain's length holds the
             analysis' empty-row value;
  bytes      chain e of the large batch holds exactly the bytes the device gave for pool chain e % D when the pool ran alone, where
             one tile takes one block and nothing loops (packed row indices after subtracting the chain's first row);
  reference  the large batch against the float64 / float32 restatement of the pool, expanded, with the analysis' own comparator.

A case sizes its batch from the CU count alone (size_padded / size_packed / size_rows / size_waves, tmalign_plan), and `Sizing.check` asserts before any
launch that the tiles exceed the block cap by an eighth, that the grid is the cap, and that D is coprime with it: the successive
tiles of one block then belong to different pool chains."""
import dataclasses
import math

import numpy as np

import _analysis as AN
import _dssp as DS
import _fape as FP
import _frames as FRM
import _gdt as GD
import _knn as K
import _lddt as Q
import _lddt_atoms as LA
import _lddt_soft as S
import _sasa as SA
import _superpose as SP
import _tmscore as TM
import _violation_loss as VL
import _violations as V
from _devpath import FILL, GUARD, to_dev

F = np.float32

# ---- the grid arithmetic of fcz_abi.hip and the kernels' headers, mirrored -------------------------------------------------------
WAVES_PER_BLOCK = 4             # fcz_kernels.h: constexpr int WAVES_PER_BLOCK = 4
BLOCK = 64 * WAVES_PER_BLOCK    # fcz_kernels.h: constexpr int BLOCK = WAVE * WAVES_PER_BLOCK
CHAIN_TILE = BLOCK              # fcz_chains.h: constexpr uint32_t CHAIN_TILE = BLOCK
SASA_TILE_ROWS = 3              # fcz_sasa.h: constexpr uint32_t SASA_TILE_ROWS = 3
LDDTA_DECIDE_ROWS = 64          # fcz_lddt_atoms.h: constexpr uint32_t LDDTA_DECIDE_ROWS = 64
KNN_PASS = 2048                 # fcz_knn.h: constexpr uint32_t KNN_PASS = 2048 (fcz_knn_pass())
LDDT_PASS = 1024                # fcz_lddt.h: constexpr uint32_t LDDT_PASS = 1024 (fcz_lddt_pass(); k_lddt_soft stages the same rows)
HBOND_PASS = 480                # fcz_dssp.h: constexpr uint32_t HBOND_PASS = 480 (fcz_hbond_pass())
ATOM_PASS = 1536                # fcz_sasa.h / fcz_violations.h / fcz_lddt_atoms.h: SASA_PASS = VIOL_PASS = LDDTA_PASS = 1536
VLOSS_PASS = 1280               # fcz_violation_loss.h: constexpr uint32_t VLOSS_PASS = 1280 (fcz_violation_loss_pass())
SWEEP_PER_CU = 16               # fcz_abi.hip, chain_tiles: uint32_t blocks_per_cu = 16u (knn, lddt, lddt_soft, dssp, sasa)
ATOMS_PER_CU = 12               # fcz_abi.hip: chain_tiles ct(ctx, packed, n, rows, viol_tile_rows(g.A), 12u); lddt_atoms' decide and score alike
WAVES_PER_CU = 16               # fcz_abi.hip, superpose / tmscore / gdt / k_ta_count: max_blocks = (uint32_t)ctx->n_cu * 16u
FRAMES_PER_CU = 8               # fcz_abi.hip, frames_rows: std::min<uint64_t>(n_tiles, (uint64_t)ctx->n_cu * 8u)
FR_ITEMS = BLOCK                # fcz_frames.h: constexpr uint32_t FR_ITEMS = BLOCK
FRAMES_WIDTH = {0: 1, 1: 8}     # fcz_abi.hip, fcz_frames_width: backbone 1, all 8
LAYOUT = {37: 0, 14: 1, 4: 2}   # fcz_dense.h: atom37, atom14, backbone4
LONG_ROWS = 120                 # rows of the pool chain whose atoms, every mask set and 14 a row, exceed a pass of ATOM_PASS
MARGIN = 8                      # every case exceeds its cap by cap / MARGIN tiles at least
N_CUS = (64, 256, 304)          # the CU counts the CPU test sizes every case for


def viol_tile_rows(A):
    """fcz_violations.h: A == 37u ? 20u : A == 14u ? 18u : 64u"""
    return 20 if A == 37 else 18 if A == 14 else 64


def lddta_tile_rows(A, decide):
    """fcz_lddt_atoms.h: decide ? LDDTA_DECIDE_ROWS : A == 37u ? 20u : A == 14u ? 18u : 64u"""
    return LDDTA_DECIDE_ROWS if decide else viol_tile_rows(A)


def frames_tile_rows(groups):
    """fcz_abi.hip, frames_rows: T = FR_ITEMS / G"""
    return FR_ITEMS // FRAMES_WIDTH[groups]


def tm_items_bound(rows, n):
    """fcz_tmscore.h: ((17u * rows) / 10u + 66u * n) / WAVES_PER_BLOCK + n + 1u"""
    return ((17 * rows) // 10 + 66 * n) // WAVES_PER_BLOCK + n + 1


def ceil_div(a, b):
    return (a + b - 1) // b


def n_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)     # fcz_ctx_create: hipDeviceAttributeMultiprocessorCount


def pick_d(blocks):
    """the pool size: the first of 7, 11, 13 that is coprime with the grid"""
    for D in (7, 11, 13):
        if math.gcd(D, blocks) == 1:
            return D
    raise AssertionError(f"no pool size is coprime with a grid of {blocks} blocks")


@dataclasses.dataclass(frozen=True)
class Sizing:
    """one launch of one case: `units` tiles (or chains, or items) over a grid of `blocks`, capped at `cap`"""
    what: str
    n: int
    D: int
    units: int
    need: int
    cap: int
    blocks: int

    @property
    def busiest(self):
        return ceil_div(self.units, self.blocks)

    def check(self, loops=2):
        over = self.units - self.cap
        print(f"{self.what}: n = {self.n} (D = {self.D}), {self.units} units over a cap of {self.cap}: {over} beyond it, the busiest block takes {self.busiest}")
        assert self.units >= self.need > self.cap and over >= self.cap // MARGIN, (self.what, self.units, self.need, self.cap)
        assert self.blocks == self.cap and self.busiest >= loops, (self.what, self.blocks, self.cap, self.busiest)
        assert self.n % self.D == 0 and math.gcd(self.D, self.blocks) == 1, (self.what, self.n, self.D, self.blocks)
        return self


def size_padded(what, cus, per_cu, tile_rows, L, need=None, D=None, n=None):
    """chain_tiles::reserve, padded: tiles_per_entry = ceil(L / tile_rows), n_padded = n * tiles_per_entry, blocks = min(n_padded, cap);
    n is the smallest multiple of D whose tiles reach `need` (cap + cap / 8 unless given)"""
    cap = cus * per_cu
    D = D or pick_d(cap)
    need = need or cap + cap // MARGIN
    tpe = ceil_div(L, tile_rows)
    n = n or ceil_div(ceil_div(need, tpe), D) * D
    return Sizing(what, n, D, n * tpe, need, cap, min(n * tpe, cap))


def size_packed(what, cus, per_cu, tile_rows, lens, need=None, reps=None):
    """chain_tiles::reserve, packed: the tiles are the sum over chains of ceil(len / tile_rows) (k_chain_tiles),
    blocks = min(R / tile_rows + n, cap); the pool `lens` is repeated until its tiles reach `need`"""
    cap = cus * per_cu
    D = len(lens)
    need = need or cap + cap // MARGIN
    per_pool = sum(ceil_div(int(m), tile_rows) for m in lens)
    reps = reps or ceil_div(need, per_pool)
    R = reps * int(np.sum(lens))
    return Sizing(what, reps * D, D, reps * per_pool, need, cap, min(R // tile_rows + reps * D, cap))


def size_rows(what, cus, per_cu, tile_rows, L, D=None, n=None):
    """frames_rows: tiles of tile_rows rows of the flat row space n * L, blocks = min(n_tiles, cap)"""
    cap = cus * per_cu
    D = D or pick_d(cap)
    need = cap + cap // MARGIN
    n = n or ceil_div(ceil_div(need * tile_rows, L), D) * D
    tiles = ceil_div(n * L, tile_rows)
    return Sizing(what, n, D, tiles, need, cap, min(tiles, cap))


def size_waves(what, cus, D=None, n=None):
    """superpose_rows and its kin: a wavefront a chain, grid = min(grid_for(n, WAVES_PER_BLOCK), n_cu * 16); the units are blocks' worth
    of chains, n >= n_cu * 64 + n_cu * 8"""
    cap = cus * WAVES_PER_CU
    D = D or pick_d(cap)
    n = n or ceil_div(cus * 64 + cus * 8, D) * D
    return Sizing(what, n, D, ceil_div(n, WAVES_PER_BLOCK), cap + cap // MARGIN, cap, min(ceil_div(n, WAVES_PER_BLOCK), cap))


def pool_lens(L, D, special=()):
    """D distinct lengths for entries of L rows: the `special` ones, then 0, 1, L, L - 1, 2, the middle and others"""
    out = []
    for m in list(special) + [0, 1, L, L - 1, 2, L // 2, L // 3, L - 2, 3, (2 * L) // 3, 4, 5, 6]:
        m = max(0, min(int(m), L))
        if m not in out:
            out.append(m)
    assert len(out) >= D, (L, D, out)
    out = out[:D]
    assert {0, 1, L} <= set(out), out
    return out


# ---- a pool's arrays in the two forms, repeated -------------------------------------------------------------------------------------

def pack_rows(v, lens, index=False):
    """padded [D, L, ..] -> packed [sum(lens), ..]; an index array holds rows of the entry and gets the chain's first row added"""
    off = AN.row_off_of(lens)
    if not index:
        return AN.pack1(v, lens)
    return np.concatenate([np.where(v[e, :m] >= 0, v[e, :m] + int(off[e]), -1).astype(v.dtype) for e, m in enumerate(lens)])


def tile_rows_of(p, reps, index=False):
    """packed pool [Rp, ..] -> the pool `reps` times over; copy r of an index array gets r * Rp added"""
    if not index:
        return np.concatenate([p] * reps) if reps > 1 else p
    shift = (np.arange(reps, dtype=np.int64) * len(p)).reshape((reps,) + (1,) * p.ndim)
    return np.where(p[None] >= 0, p[None] + shift, -1).astype(p.dtype).reshape((reps * len(p),) + p.shape[1:])


def expand(an, arrays, lens, n, packed, already_packed=False):
    """the dict `arrays` of a pool (inputs, a reference or the device's outputs for the pool alone) as the batch of n chains"""
    D = len(lens)
    idx = np.arange(n) % D
    out = {}
    for k, v in arrays.items():
        if v is None:
            out[k] = None
        elif k in an.chain_keys or not packed:
            out[k] = v[idx]
        else:
            index = k in an.index_keys
            out[k] = tile_rows_of(v if already_packed else pack_rows(v, lens, index), n // D, index)
    return out


def _raw(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape[0] if a.ndim else 1, -1) if a.size else a.view(np.uint8).reshape(0, 0)


def assert_written(an, got, lens, n, packed, empty, what):
    """no unit of an output is still the fill; padded: the rows behind every length hold the bytes of `empty` (an empty row of the pool run)"""
    D = len(lens)
    for k, g in got.items():
        lead = 1 if (k in an.chain_keys or packed) else 2
        flat = np.ascontiguousarray(g).reshape((-1,) + g.shape[lead:])
        raw = _raw(flat)
        left = (raw == FILL).all(axis=1) if raw.shape[1] else np.zeros(len(raw), bool)
        assert not left.any(), (what, k, "units still 0xA5", int(left.sum()), np.flatnonzero(left)[:4])
        if lead == 2 and k in empty:
            e_raw = np.ascontiguousarray(empty[k]).view(np.uint8).reshape(-1)
            for d, m in enumerate(lens):
                tail = np.ascontiguousarray(g[d::D, m:])
                if tail.size:
                    assert (tail.view(np.uint8).reshape(tail.shape[0] * tail.shape[1], -1) == e_raw).all(), (what, k, "behind the length of pool chain", d)


def assert_bytes(got, exp, what):
    for k, g in got.items():
        e = exp[k]
        assert g.shape == e.shape and g.dtype == e.dtype, (what, k, g.shape, e.shape, g.dtype, e.dtype)
        if g.tobytes() != e.tobytes():
            bad = np.argwhere(AN.bits(g) != AN.bits(e))
            raise AssertionError((what, k, "differs from the pool run on bytes", len(bad), bad[:4]))


class Analysis:
    """one analysis as the engine sees it. Arrays are dicts; a key in chain_keys is [n, ..], every other [n, L, ..] / [R, ..]; a key
    in index_keys holds row numbers (rows of the entry when padded, rows of the arrays when packed, -1 = none)."""
    name = ""
    key = None                                        # what the pool and its restatement depend on, where that is less than the name
    A, slot = 4, 1
    tile_rows, per_cu = CHAIN_TILE, SWEEP_PER_CU
    chain_keys = frozenset()
    index_keys = frozenset()
    guard = GUARD                                     # bytes of fill around every output of run(); 4: no output begins on 16 bytes
    family = "pair"                                   # which generator of tests/_analysis_fuzz.py draws the inputs of fuzz_pool

    @property
    def layout(self):
        return LAYOUT[self.A]

    def fuzz_pool(self, rng, lens, L, profile):
        """the inputs of pool() for any lengths, drawn by tests/_analysis_fuzz.py from `profile` (a string per chain and one for the case)"""
        import _analysis_fuzz as FZ
        return FZ.draw(self, rng, lens, L, profile)

    def launches(self):
        """(what, tile rows, blocks per CU) of every sweep launch of one call"""
        return [(self.name, self.tile_rows, self.per_cu)]

    def pool(self, lens, L):
        raise NotImplementedError

    def ref(self, inp, lens):
        raise NotImplementedError

    def run(self, codec, dev, bound_t, n, rows, packed):
        raise NotImplementedError

    def check(self, got, exp, what):
        raise NotImplementedError

    def fair(self, inp, ref, lens):
        """the margin conditions the comparator needs of the pool (the pool, not the kernel, must satisfy them)"""

    def pool_and_ref(self, lens, L):
        """the pool's inputs and its restatement: computed once per (analysis, lengths), shared, never changed"""
        key = (self.key or self.name, tuple(int(m) for m in lens), int(L))
        if key not in _POOLS:
            inp = self.pool(list(key[1]), key[2])
            ref = self.ref(inp, np.asarray(key[1], np.uint32))
            self.fair(inp, ref, key[1])
            for v in list(inp.values()) + list(ref.values()):
                if v is not None:
                    v.setflags(write=False)
            _POOLS[key] = (inp, ref)
        return _POOLS[key]


_POOLS = {}


def _dev(arrays):
    return {k: None if v is None else to_dev(v) for k, v in arrays.items()}


def drive(codec, an, lens, L, n, packed, what):
    """the three assertions for one analysis, one pool and one form -> the outputs of the pool alone and of the batch"""
    D = len(lens)
    lens_a = np.asarray(lens, np.uint32)
    inp, ref = an.pool_and_ref(lens, L)

    def bound_of(count):
        return AN.row_off_of(list(lens) * (count // D)) if packed else lens_a[np.arange(count) % D]

    def call(count):
        arrays = expand(an, inp, lens, count, packed)
        rows = int(np.sum(lens)) * (count // D) if packed else L
        return an.run(codec, _dev(arrays), to_dev(bound_of(count)), count, rows, packed)

    small = call(D)
    big = call(n)
    zero = list(lens).index(0)
    empty = {} if packed else {k: v[zero, 0] for k, v in small.items() if k not in an.chain_keys}
    assert_written(an, big, lens, n, packed, empty, what)
    assert_bytes(big, expand(an, small, lens, n, packed, already_packed=True), what)
    an.check(big, expand(an, ref, lens, n, packed), what)
    return small, big


# ---- pools ---------------------------------------------------------------------------------------------------------------------------

def _payload(pos, mask):
    """a NaN with a payload under every cleared mask"""
    pos.view(np.uint32)[mask == 0] = AN.NAN_BITS


def lattice_pool(lens, L, A, slot, seed):
    """integer-lattice chains [D, L, A, 3] (ties in every neighbour list): ~10 % of the sites cleared (NaN payloads under them), per
    chain of 8 rows or more a NaN, +inf, -inf and two 3e19 coordinates under set masks; data, not NaN, behind every length"""
    rng = np.random.default_rng(seed)
    n = len(lens)
    pos = rng.integers(-6, 7, size=(n, L, A, 3)).astype(F)
    mask = np.ones((n, L, A), np.uint8)
    mask[..., slot][rng.random((n, L)) < 0.10] = 0
    for e, m in enumerate(lens):
        if m >= 8:
            r = rng.choice(m, size=5, replace=False)
            pos[e, r[0], slot, 0] = np.nan; pos[e, r[1], slot, 1] = np.inf; pos[e, r[2], slot, 2] = -np.inf
            pos[e, r[3], slot, 0] = 3e19; pos[e, r[4], slot, 0] = -3e19
            mask[e, r, slot] = 1
    _payload(pos, mask)
    return pos, mask


class Knn(Analysis):
    family = "site"
    index_keys = frozenset({"index"})
    K_REF = 17                                       # the restatement's k: a smaller k is the first k columns of the same order

    def __init__(self, A=4, slot=1, k=5):
        self.A, self.slot, self.k, self.name, self.key = A, slot, k, f"knn k={k} A={A}", f"knn A={A}"

    def pool(self, lens, L):
        pos, mask = lattice_pool(lens, L, self.A, self.slot, 101)
        return dict(pos=pos, mask=mask)

    def ref(self, inp, lens):
        index, dist = K.knn_padded(inp["pos"], inp["mask"], lens, self.slot, self.K_REF)
        return dict(index=index, dist=dist)

    def run(self, codec, dev, bound_t, n, rows, packed):
        index, dist = K.run_dev(codec, dev["pos"], dev["mask"], bound_t, n, rows, self.layout, self.slot, self.k, packed, guard=self.guard)
        return dict(index=index, dist=dist)

    def check(self, got, exp, what):
        K.same((got["index"], got["dist"]), (exp["index"][..., :self.k], exp["dist"][..., :self.k]), what)


class Lddt(Analysis):
    def __init__(self, A=4, slot=1):
        self.A, self.slot, self.name = A, slot, f"lddt A={A}"

    def pool(self, lens, L):
        t, mt, p, mp = S.lattice(lens, L, self.A, self.slot, 103, behind="data")
        for e, m in enumerate(lens):                                       # (S.lattice plants its non-finite coordinates from 16 rows on)
            if 8 <= m < 16:
                t[e, 3, self.slot, 0] = np.nan; p[e, 5, self.slot, 1] = np.inf
                mt[e, [3, 5], self.slot] = 1; mp[e, [3, 5], self.slot] = 1
        return dict(pt=t, mt=mt, pp=p, mp=mp)

    def ref(self, inp, lens):
        return dict(zip(("score", "pairs", "hits"), Q.lddt_padded(inp["pt"], inp["mt"], inp["pp"], inp["mp"], lens, self.slot)))

    def run(self, codec, dev, bound_t, n, rows, packed):
        got = Q.run_dev(codec, dev["pt"], dev["mt"], dev["pp"], dev["mp"], bound_t, n, rows, self.layout, self.slot, packed, guard=self.guard)
        return dict(zip(("score", "pairs", "hits"), got))

    def check(self, got, exp, what):
        Q.same(tuple(got[k] for k in ("score", "pairs", "hits")), tuple(exp[k] for k in ("score", "pairs", "hits")), what)


class LddtSoft(Analysis):
    """the value and the gradient in one: prediction = truth + noise (S.walk), so the bounds of _lddt_soft.py need tie_share <= 0.02"""
    name = "lddt_soft"
    TIE_SHARE = 0.02

    def pool(self, lens, L):
        t, mt, p = S.walk(lens, L, self.A, self.slot, S.WALK_SEED)
        rng = np.random.default_rng(S.WALK_SEED + 7)
        for e, m in enumerate(lens):                                       # data behind the length; a non-finite coordinate under set masks
            t[e, m:] = rng.standard_normal((L - m, self.A, 3)) * 5
            p[e, m:] = rng.standard_normal((L - m, self.A, 3)) * 5
            if m >= 8:
                r = rng.choice(m, size=2, replace=False)
                mt[e, r, self.slot] = 1
                p[e, r[0], self.slot, 1] = np.inf; t[e, r[1], self.slot, 2] = np.nan
        _payload(t, mt)
        return dict(pt=t, mt=mt, pp=p, mp=None, w=S.weights((len(lens), L), S.WALK_SEED + 1))

    def ref(self, inp, lens):
        return S.soft_padded(inp["pt"], inp["mt"], inp["pp"], None, lens, self.slot, inp["w"])

    def fair(self, inp, ref, lens):
        assert S.tie_share(ref) <= self.TIE_SHARE, S.tie_share(ref)

    def run(self, codec, dev, bound_t, n, rows, packed):
        a = (dev["pt"], dev["mt"], dev["pp"], None, bound_t, n, rows, self.layout, self.slot, packed)
        soft, pairs = S.run_value(codec, *a, guard=self.guard)
        return dict(soft=soft, pairs=pairs, grad=S.run_grad(codec, *a, dev["w"], guard=self.guard))

    def check(self, got, exp, what):
        S.check_value((got["soft"], got["pairs"]), exp, what)
        S.check_grad(got["grad"], exp, what)


def backbone_pool(lens, L, seed):
    """backbone4 chains [D, L, 4, 3] as test_gpu_dssp.py draws them: even chains on the integer lattice -1 .. 1, odd chains jittered
    ideal helices; ~1 % of the atoms cleared (NaN payloads), per chain of 12 rows or more non-finite coordinates under set masks;
    data behind every length; aatype random with ~10 % proline"""
    rng = np.random.default_rng(seed)
    n = len(lens)
    pos = rng.integers(-1, 2, size=(n, L, 4, 3)).astype(F)
    mask = np.ones((n, L, 4), np.uint8)
    for e, m in enumerate(lens):
        if e % 2 and m:
            pos[e, :m] = DS.ideal_backbone(-57, -47, m)[0] + (rng.standard_normal((m, 4, 3)) * 0.05).astype(F)
        mask[e, :m][rng.random((m, 4)) < 0.008] = 0
        if m >= 12:
            r = rng.choice(m, size=5, replace=False)
            pos[e, r[0], 0, 0] = np.nan; pos[e, r[1], 1, 1] = np.inf; pos[e, r[2], 3, 2] = -np.inf
            pos[e, r[3], 2, 0] = 3e19; pos[e, r[4], 0, 1] = -3e19
            mask[e, r] = 1
    _payload(pos, mask)
    aatype = rng.integers(0, 21, size=(n, L)).astype(np.uint8)
    aatype[rng.random((n, L)) < 0.1] = DS.PRO
    return pos, mask, aatype


TABLE_KEYS = ("acc_index", "acc_energy", "don_index", "don_energy")


class Hbond(Analysis):
    family = "backbone"
    name = "hbond"
    index_keys = frozenset({"acc_index", "don_index"})

    def pool(self, lens, L):
        return dict(zip(("pos", "mask", "aatype"), backbone_pool(lens, L, 107)))

    def ref(self, inp, lens):
        return dict(zip(TABLE_KEYS, DS.hbonds(inp["pos"], inp["mask"], inp["aatype"], lens)))

    def run(self, codec, dev, bound_t, n, rows, packed):
        return dict(zip(TABLE_KEYS, DS.run_hbond(codec, dev["pos"], dev["mask"], dev["aatype"], bound_t, n, rows, self.layout, packed, guard=self.guard)))

    def check(self, got, exp, what):
        DS.same_tables([got[k] for k in TABLE_KEYS], [exp[k] for k in TABLE_KEYS], what)


class Labels(Analysis):
    """the label kernels on the acceptor table of the restatement"""
    family = "labels"
    name = "dssp labels"
    index_keys = frozenset({"acc_index"})

    def pool(self, lens, L):
        inp, ref = HBOND.pool_and_ref(lens, L)
        return dict(inp, acc_index=ref["acc_index"], acc_energy=ref["acc_energy"])

    def ref(self, inp, lens):
        ss, ss_mask = DS.labels(inp["pos"], inp["mask"], lens, inp["acc_index"], inp["acc_energy"])
        return dict(ss=ss, ss_mask=ss_mask.view(np.uint8))

    def run(self, codec, dev, bound_t, n, rows, packed):
        ss, ss_mask = DS.run_labels(codec, dev["pos"], dev["mask"], dev["aatype"], bound_t, n, rows, self.layout, packed, dev["acc_index"], dev["acc_energy"], guard=self.guard)
        return dict(ss=ss, ss_mask=ss_mask)

    def check(self, got, exp, what):
        DS.same_labels((got["ss"], got["ss_mask"]), (exp["ss"], exp["ss_mask"]), what)


class Apply(Analysis):
    """k_superpose_apply: a transform per chain on every atom of its rows (no non-finite coordinate under a set mask here: the payload
    of a NaN result is not part of the contract, and the comparison is on bytes)"""
    family = "apply"
    name = "superpose_apply"
    chain_keys = frozenset({"rot", "trans"})

    def pool(self, lens, L):
        rng = np.random.default_rng(109)
        n = len(lens)
        pos = rng.uniform(-80, 80, (n, L, self.A, 3)).astype(F)
        mask = (rng.random((n, L, self.A)) > 0.25).astype(np.uint8)
        _payload(pos, mask)
        return dict(pos=pos, mask=mask, rot=rng.uniform(-2, 2, (n, 3, 3)).astype(F), trans=rng.uniform(-100, 100, (n, 3)).astype(F))

    def ref(self, inp, lens):
        return dict(out=SP.apply_expected(inp["pos"], inp["mask"], inp["rot"], inp["trans"], length=lens))

    def run(self, codec, dev, bound_t, n, rows, packed):
        return dict(out=SP.run_apply(codec, dev["pos"], dev["mask"], bound_t, n, rows, self.layout, dev["rot"], dev["trans"], packed, guard=self.guard))

    def check(self, got, exp, what):
        assert got["out"].shape == exp["out"].shape and got["out"].tobytes() == exp["out"].tobytes(), (what, np.argwhere(AN.bits(got["out"]) != AN.bits(exp["out"]))[:4])


# ---- the atom-slot sweeps ---------------------------------------------------------------------------------------------------------------

def biggest_type(A=14):
    """the residue type with the most atoms of the default radii table"""
    return int(np.argmax((SA.default_table(A) != 0).sum(axis=1)))


def atoms_pool(lens, L, A, seed):
    """jittered helices with scattered side chains [D, L, A, 3] as test_gpu_sasa.py draws them: ~1 % of the masks cleared (NaN payloads),
    per chain of 12 rows or more non-finite coordinates under set masks, data behind every length, aatype random 0 .. 24 and 255;
    the LONGEST chain has every mask set, finite coordinates and the type with the most atoms, so that its atoms exceed one pass"""
    rng = np.random.default_rng(seed)
    n = len(lens)
    pos, mask = np.zeros((n, L, A, 3), F), np.ones((n, L, A), np.uint8)
    aatype = rng.integers(0, 25, size=(n, L)).astype(np.uint8)
    aatype[rng.random((n, L)) < 0.05] = 255
    full = int(np.argmax(lens))
    for e, m in enumerate(lens):
        pos[e] = AN.helix(rng, L, A)
        if e == full:
            aatype[e] = biggest_type(A)
            continue
        mask[e, :m][rng.random((m, A)) < 0.01] = 0
        if m >= 12:
            r = rng.choice(m, size=5, replace=False)
            pos[e, r[0], 0, 0] = np.nan; pos[e, r[1], 1, 1] = np.inf; pos[e, r[2], 3, 2] = -np.inf
            pos[e, r[3], 2, 0] = 3e19; pos[e, r[4], 0, 1] = -3e19
            mask[e, r, :4] = 1
    _payload(pos, mask)
    return pos, mask, aatype


def atoms_lens(T, D, long_rows):
    """pool lengths for a sweep of T rows a tile: 0, 1, 2, a tile less one, a tile, two tiles, two tiles and a row, and the long chain"""
    L = max(2 * T + 1, long_rows)
    lens = [0, 1, 2 * T + 1, T, long_rows, 2 * T, L - 1, 2, T + 1, T - 1, 3, L, 2 * T - 1][:D]
    return [min(m, L) for m in lens], L


SASA_KEYS = ("sasa_points", "sasa", "sasa_mask")


class Sasa(Analysis):
    family = "atoms"
    tile_rows = SASA_TILE_ROWS
    N_POINTS = 1                                       # the smallest point set test_gpu_sasa.py passes to run_sasa

    def __init__(self, A=14):
        self.A, self.name = A, f"sasa A={A}"

    def points(self):
        from foldcomp_amd import api
        return api.sphere_points(self.N_POINTS)

    def pool(self, lens, L):
        return dict(zip(("pos", "mask", "aatype"), atoms_pool(lens, L, self.A, 113)))

    def ref(self, inp, lens):
        got = SA.sasa(inp["pos"], inp["mask"], inp["aatype"], lens, SA.default_table(self.A), SA.PROBE, self.points())
        return dict(sasa_points=got[0], sasa=got[1], sasa_mask=got[2].view(np.uint8))

    def fair(self, inp, ref, lens):
        e = int(np.argmax(lens))
        atoms = int(SA.atoms_of(inp["pos"][e, :lens[e]], inp["mask"][e, :lens[e]], inp["aatype"][e, :lens[e]], SA.default_table(self.A))[0].sum())
        assert atoms > ATOM_PASS, (atoms, "the long chain takes one pass only")

    def run(self, codec, dev, bound_t, n, rows, packed):
        return dict(zip(SASA_KEYS, SA.run_sasa(codec, dev["pos"], dev["mask"], dev["aatype"], bound_t, n, rows, self.layout, packed, to_dev(self.points()), guard=self.guard)))

    def check(self, got, exp, what):
        SA.same_sasa([got[k] for k in SASA_KEYS], [exp[k] for k in SASA_KEYS], what)


class Violations(Analysis):
    family = "atoms"
    per_cu = ATOMS_PER_CU
    chain_keys = frozenset({"chain_counts"})

    def __init__(self, A=14):
        self.A, self.tile_rows, self.name = A, viol_tile_rows(A), f"violations A={A}"

    def pool(self, lens, L):
        return dict(zip(("pos", "mask", "aatype"), atoms_pool(lens, L, self.A, 127)))

    def ref(self, inp, lens):
        out = V.violations(inp["pos"], inp["mask"], inp["aatype"], lens, V.default_table(self.A))
        return {k: (v.view(np.uint8) if v.dtype == bool else v) for k, v in out.items()}

    fair = Sasa.fair

    def run(self, codec, dev, bound_t, n, rows, packed):
        return V.run_violations(codec, dev["pos"], dev["mask"], dev["aatype"], bound_t, n, rows, self.layout, packed, guard=self.guard)

    def check(self, got, exp, what):
        V.same_violations(got, exp, what)
        assert exp["clash_count"].any() and exp["link_violation"].any()


class ViolationLoss(Analysis):
    """the value and the gradient of one call each: two launches over viol_tile_rows(A) rows a tile, 12 blocks a CU (fcz_abi.hip,
    vloss_rows). param 0: tolerance 0 and link factor 0.5, so that every term class is there; param 1: the defaults (1.5, 12.0)"""
    family = "vloss"
    per_cu = ATOMS_PER_CU
    chain_keys = frozenset({"counts"})
    PARAMS = ((F(0), F(0.5)), (VL.TOL, VL.FACTOR))

    def __init__(self, A=14, param=0):
        self.A, self.tile_rows, self.name, self.params = A, viol_tile_rows(A), f"violation_loss A={A}" + (" defaults" if param else ""), self.PARAMS[param]

    def launches(self):
        return [(f"{self.name} {k}", self.tile_rows, self.per_cu) for k in ("value", "grad")]

    def pool(self, lens, L):
        inp = dict(zip(("pos", "mask", "aatype"), atoms_pool(lens, L, self.A, 131)))
        return dict(inp, w_clash=VL.weights((len(lens), L, self.A), 132), w_link=VL.weights((len(lens), L, 3), 133))

    def ref(self, inp, lens):
        table = V.default_table(self.A)
        out = VL.loss(inp["pos"], inp["mask"], inp["aatype"], lens, table, *self.params)
        return dict(out, grad=VL.grad(inp["pos"], inp["mask"], inp["aatype"], lens, table, inp["w_clash"], inp["w_link"], *self.params))

    def fair(self, inp, ref, lens):
        assert int(ref["counts"][:, 0].max()) > VLOSS_PASS, (ref["counts"][:, 0], "the long chain takes one pass only")
        assert (ref["clash_loss"] > 0).any() and all((ref["link_loss"][..., k] > 0).any() for k in range(3)) and np.isfinite(ref["grad"]).all()

    def run(self, codec, dev, bound_t, n, rows, packed):
        a = (dev["pos"], dev["mask"], dev["aatype"], bound_t, n, rows, self.layout, packed)
        kw = dict(tol=self.params[0], factor=self.params[1], guard=self.guard)
        return dict(VL.run_value(codec, *a, **kw), grad=VL.run_grad(codec, *a, dev["w_clash"], dev["w_link"], **kw))

    def check(self, got, exp, what):
        VL.same(got, exp, what)


SWAP_TYPES = (LA.ASP, LA.GLU, LA.PHE, LA.TYR)


class LddtAtoms(Analysis):
    family = "atom_pair"
    per_cu = ATOMS_PER_CU

    def __init__(self, A=14):
        self.A, self.tile_rows, self.name = A, lddta_tile_rows(A, False), f"lddt_atoms A={A}"

    def launches(self):
        return [(self.name + " decide", lddta_tile_rows(self.A, True), self.per_cu), (self.name + " score", lddta_tile_rows(self.A, False), self.per_cu)]

    def pool(self, lens, L):
        """test_gpu_lddt_atoms.py's synthetic set: the truth atoms scattered about a walk, the prediction the truth plus noise of 0.5 with
        the partnered slots of every second ASP / GLU / PHE / TYR row exchanged; the longest chain has every mask set"""
        A = self.A
        rng = np.random.default_rng(131)
        n = len(lens)
        table = LA.default_table(A)
        types = np.asarray(SWAP_TYPES + (0, 7, 11, 19, 20, 255), np.uint8)
        aa = types[(np.arange(n * L) * 3 % len(types))].reshape(n, L).copy()
        ca = np.cumsum(rng.standard_normal((n, L, 3)) * 2.2, axis=1)
        pt = (ca[:, :, None, :] + rng.standard_normal((n, L, A, 3)) * 2.0).astype(F)
        pp = pt + (rng.standard_normal((n, L, A, 3)) * 0.5).astype(F)
        density = {37: 0.21, 14: 0.56, 4: 1.0}[A]
        mt, mp = (rng.random((n, L, A)) < density).astype(np.uint8), (rng.random((n, L, A)) < min(1.0, density * 4)).astype(np.uint8)
        partnered = (table != np.arange(A))[np.minimum(aa, 20)]
        keep = partnered & (rng.random((n, L)) < 0.75)[..., None]
        mt[keep] = 1; mp[keep] = 1
        full = int(np.argmax(lens))
        mt[full] = 1; mp[full] = 1
        for e, m in enumerate(lens):
            if e != full and m >= 12:
                r = rng.choice(m, size=5, replace=False)
                pt[e, r[0], 0, 0] = np.nan; pp[e, r[1], 1, 1] = np.inf; pt[e, r[2], A - 1, 2] = -np.inf
                pp[e, r[3], 2, 0] = 3e19; pt[e, r[4], 0, 1] = -3e19
                mt[e, r] = 1; mp[e, r] = 1
        capable = partnered.any(axis=-1)
        exchanged = np.zeros(capable.size, bool)
        exchanged[np.flatnonzero(capable.ravel())[::2]] = True
        pp = np.ascontiguousarray(LA.exchange(pp, aa, exchanged.reshape(capable.shape), table))
        _payload(pt, mt)
        return dict(pt=pt, mt=mt, pp=pp, mp=mp, aatype=aa)

    def ref(self, inp, lens):
        out = LA.lddt_atoms(inp["pt"], inp["mt"], inp["pp"], inp["mp"], inp["aatype"], lens, LA.default_table(self.A))
        return {k: (v.view(np.uint8) if v.dtype == bool else v) for k, v in out.items()}

    def fair(self, inp, ref, lens):
        e = int(np.argmax(lens))
        with np.errstate(invalid="ignore"):
            both = (inp["mt"][e, :lens[e]] != 0) & (inp["mp"][e, :lens[e]] != 0)
        assert int(both.sum()) > ATOM_PASS, int(both.sum())
        sw = ref["swapped"].astype(bool)
        assert sw.any() and (np.diff(sw.astype(np.int8), axis=1) != 0).any(), "no row was renamed"

    def run(self, codec, dev, bound_t, n, rows, packed):
        return LA.run_dev(codec, dev["pt"], dev["mt"], dev["pp"], dev["mp"], dev["aatype"], bound_t, n, rows, self.layout, packed, guard=self.guard)

    def check(self, got, exp, what):
        LA.same(got, exp, what)


# ---- the wave-per-chain and the flat-row grids -----------------------------------------------------------------------------------------

SUPERPOSE_LENS = (0, 1, 2, 3, 4, 7, 8, 5, 6, 8, 3, 8, 4)
SUPERPOSE_L = 8


class Superpose(Analysis):
    """k_superpose, a wavefront a chain: the units of its grid are chains, not tiles"""
    name = "superpose"
    chain_keys = frozenset(SP.KEYS[:-1])

    def pool(self, lens, L):
        rng = np.random.default_rng(SP.WALK_SEED)
        n = len(lens)
        true, pred = rng.uniform(-20, 20, (n, L, 3)).astype(F), rng.uniform(-20, 20, (n, L, 3)).astype(F)      # (data behind every length)
        for e, m in enumerate(lens):
            if m >= 3:
                x = SP.walk_chain(rng, m)
                true[e, :m], pred[e, :m] = x, x @ SP.random_rotation(rng).T + rng.uniform(-30, 30, 3) + 1.5 * rng.standard_normal((m, 3))
        pt, pp = SP.in_slot(true, self.A, self.slot, 7.0), SP.in_slot(pred, self.A, self.slot, -3.0)
        mt, mp = np.ones(pt.shape[:-1], np.uint8), np.ones(pt.shape[:-1], np.uint8)
        for e, m in enumerate(lens):                                       # one cleared site and one non-finite one in the chains that can spare them
            if m >= 7:
                mt[e, 1, self.slot] = 0
                pp[e, 4, self.slot, 0] = np.inf
        _payload(pt, mt)
        return dict(pt=pt, mt=mt, pp=pp, mp=mp)

    def ref(self, inp, lens):
        return SP.superpose_padded(inp["pt"], inp["mt"], inp["pp"], inp["mp"], lens, self.slot)

    def fair(self, inp, ref, lens):
        site = SP.site_of(inp["pt"], inp["mt"], inp["pp"], inp["mp"], self.slot)
        for e, m in enumerate(lens):
            s = site[e, :m]
            assert SP.threshold_margin(ref["dev"][e, :m][s]) >= 1e-4, e
            if ref["sites"][e] >= 3:
                assert SP.horn_gap(inp["pt"][e, :m, self.slot], inp["pp"][e, :m, self.slot], s) >= 1e-3, e

    def run(self, codec, dev, bound_t, n, rows, packed):
        return SP.run_dev(codec, dev["pt"], dev["mt"], dev["pp"], dev["mp"], bound_t, n, rows, self.layout, self.slot, packed, guard=self.guard)

    def check(self, got, exp, what):
        SP.close(got, exp, what, compare_rot=exp["sites"] >= 3)
        SP.proper(got["rot"], what)
        self.degenerate(got, exp)
        assert not got["tm"][exp["sites"] == 0].any()

    @staticmethod
    def degenerate(got, exp):
        """no site, one site: the identity and no deviation; no site: nothing else either"""
        few, none = exp["sites"] < 2, exp["sites"] == 0
        assert few.any() and none.any() and (got["rot"][few] == np.eye(3, dtype=F)).all() and not got["trans"][none].any()
        if "rmsd" in got:
            assert not got["rmsd"][few].any()
        assert not got["gdt_counts"][none].any() and (got["gdt_counts"][exp["sites"] == 1] == 1).all()


def search_items(sites):
    """k_tm_count: (tm_seed_count(S, levels) + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK items a chain, from the restatement's own seed
    lists (levels = 0)"""
    return [ceil_div(len(TM.seed_list(int(S))), WAVES_PER_BLOCK) if S else 0 for S in sites]


class TmScore(Superpose):
    """k_tm_count and k_tm_final a wavefront a chain, k_tm_search over the items (four seeds each) of every chain"""
    name = "tmscore"
    key = "tmscore"
    chain_keys = frozenset(TM.KEYS) - {"dev"}
    searches = True

    def ref(self, inp, lens):
        self.traces = []
        return TM.tm_padded(inp["pt"], inp["mt"], inp["pp"], inp["mp"], lens, self.slot, traces=self.traces)

    def fair(self, inp, ref, lens):
        print(f"{self.name} pool: margin, Horn gap, lead", TM.assert_fair(inp["pt"], inp["pp"], self.slot, self.traces, self.name))

    def run(self, codec, dev, bound_t, n, rows, packed):
        return TM.run_dev(codec, dev["pt"], dev["mt"], dev["pp"], dev["mp"], bound_t, n, rows, self.layout, self.slot, packed, guard=self.guard)

    def check(self, got, exp, what):
        for k in ("seed", "selected"):
            assert got[k].dtype == np.int32 and np.array_equal(got[k], exp[k]), (what, k, np.argwhere(got[k] != exp[k])[:4])
        SP.close(got, exp, what, compare_rot=exp["selected"] >= 3)
        SP.proper(got["rot"], what)
        self.degenerate(got, exp)
        assert (got["tm"][exp["sites"] == 1] == 1).all() and not got["seed"][exp["sites"] < 3].any()


class Gdt(Superpose):
    """k_tm_count a wavefront a chain, k_gdt_search over the items, k_gdt_final a block a chain (grid min(n, n_cu * 16))"""
    name = "gdt"
    key = "gdt"
    chain_keys = frozenset(GD.KEYS) - {"within"}
    searches = True

    def ref(self, inp, lens):
        self.traces = []
        return GD.gdt_padded(inp["pt"], inp["mt"], inp["pp"], inp["mp"], lens, self.slot, traces=self.traces)

    def fair(self, inp, ref, lens):
        print(f"{self.name} pool: (a), (b), (c)", GD.assert_fair(inp["pt"], inp["pp"], self.slot, self.traces, self.name))

    def run(self, codec, dev, bound_t, n, rows, packed):
        return GD.run_dev(codec, dev["pt"], dev["mt"], dev["pp"], dev["mp"], bound_t, n, rows, self.layout, self.slot, packed, guard=self.guard)

    def check(self, got, exp, what):
        solved = exp["sites"] >= 3
        GD.close(got, exp, what, compare=np.repeat(solved[:, None], 5, axis=1))
        SP.proper(got["rot"][solved], what)
        none = exp["sites"] == 0
        assert none.any() and (got["rot"][none] == np.eye(3, dtype=F)).all() and not got["trans"][none].any() and not got["gdt_counts"][none].any()


class Frames(Analysis):
    """k_frames: tiles of FR_ITEMS / G rows of the FLAT row space, so a tile spans entries; padded only"""
    family = "atoms"
    A = 14
    per_cu = FRAMES_PER_CU

    def __init__(self, groups):
        self.groups, self.tile_rows, self.name = groups, frames_tile_rows(groups), f"frames groups={groups}"

    def pool(self, lens, L):
        rng = np.random.default_rng(137)
        n = len(lens)
        pos = np.stack([AN.helix(rng, L, self.A) for _ in range(n)])
        mask = (rng.random((n, L, self.A)) > 0.03).astype(np.uint8)
        for e, m in enumerate(lens):
            if m >= 12:
                r = rng.choice(m, size=3, replace=False)
                pos[e, r[0], 0, 0] = np.nan; pos[e, r[1], 1, 1] = np.inf; pos[e, r[2], 2, 2] = -np.inf
                mask[e, r, :4] = 1
        _payload(pos, mask)
        aatype = rng.integers(0, 25, size=(n, L)).astype(np.uint8)
        aatype[rng.random((n, L)) < 0.05] = 255
        return dict(pos=pos, mask=mask, aatype=aatype)

    def ref(self, inp, lens):
        return dict(zip(("rot", "trans", "frame_mask"), FRM.frames(inp["pos"], inp["mask"], inp["aatype"], lens, self.layout, self.groups)))

    def run(self, codec, dev, bound_t, n, rows, packed):
        return dict(zip(("rot", "trans", "frame_mask"), FRM.run_dev(codec, dev["pos"], dev["mask"], dev["aatype"], bound_t, n, rows, self.layout, self.groups, guard=self.guard)))

    def check(self, got, exp, what):
        FRM.same([got[k] for k in ("rot", "trans", "frame_mask")], [exp[k] for k in ("rot", "trans", "frame_mask")], what)


FAPE_PASS = 1024                # fcz_fape.h: constexpr uint32_t FAPE_PASS = 1024 (fcz_fape_pass(); k_fape_grad_points stages 256 frames a pass)
FAPE_FRAME_PASS = 256           # fcz_fape.h: constexpr uint32_t FAPE_FRAME_PASS = 256


class Fape(Analysis):
    """the value and the two gradient sweeps of one call each: three launches over CHAIN_TILE rows a tile, 16 blocks a CU"""
    name = "fape"
    family = "fape"
    clamp = FP.LATTICE_CLAMP

    def launches(self):
        return [(f"{self.name} {k}", self.tile_rows, self.per_cu) for k in ("value", "grad frames", "grad points")]

    def pool(self, lens, L):
        inp = FP.lattice(lens, L, self.A, self.slot, FP.SYNTH_SEED + 7, behind="data")
        return dict(inp, w=FP.weights((len(lens), L), FP.SYNTH_SEED + 8))

    def ref(self, inp, lens):
        return FP.fape_padded(inp, lens, self.slot, inp["w"], self.clamp)

    def fair(self, inp, ref, lens):
        assert FP.tie_share(ref) == 0 and ref["frame"].any() and ref["point"].any()

    def run(self, codec, dev, bound_t, n, rows, packed):
        got = FP.run_both(codec, [dev[k] for k in FP.ORDER], bound_t, n, rows, self.layout, self.slot, packed, dev["w"], clamp=self.clamp, guard=self.guard)
        return dict(zip(FP.OUT_KEYS, got))

    def check(self, got, exp, what):
        FP.check_value((got["sum"], got["points"]), exp, what)
        FP.check_grad((got["grad_rot"], got["grad_trans"], got["grad_pos"]), exp, what)


HBOND = Hbond()
FRAMES_L = 33


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------

@dataclasses.dataclass(frozen=True)
class Plan:
    lens: tuple
    L: int
    n: int
    packed: bool
    sizings: tuple
    loops: int

    def check(self):
        for s in self.sizings:
            s.check(self.loops)
        return self


@dataclasses.dataclass(frozen=True)
class Case:
    """one analysis at one shape and form. kind: "one" an entry a tile (L = 12), "three" three tiles an entry with a partial last one
    (L = 2 * CHAIN_TILE + 1), "triple" L = 12 with more than two grids' worth of tiles, "passes" L = the largest pass + 1 with lengths
    about the analysis' own pass, "atoms" two tiles and a row of the analysis' largest tile (and the chain of more than one pass),
    "waves" a wavefront a chain at L = 8, "rows" tiles of the flat row space at L = 33"""
    an: Analysis
    kind: str
    packed: bool = False
    own_pass: int = 0

    @property
    def id(self):
        return f"{self.an.name}, {self.kind}, {'packed' if self.packed else 'padded'}".replace(" ", "_")

    def shape(self, D):
        """-> (pool lengths, L)"""
        an = self.an
        if self.kind in ("one", "triple"):
            return pool_lens(12, D), 12
        if self.kind == "three":
            L = 2 * CHAIN_TILE + 1
            return pool_lens(L, D, (CHAIN_TILE - 1, CHAIN_TILE, CHAIN_TILE + 1, 2 * CHAIN_TILE, L)), L
        if self.kind == "passes":
            L, P = max(KNN_PASS, LDDT_PASS, HBOND_PASS) + 1, self.own_pass
            return pool_lens(L, D, (P - 1, P + 1, min(2 * P + 1, L), P)), L
        if self.kind == "atoms":
            T = max(t for _, t, _ in an.launches())
            return atoms_lens(T, D, LONG_ROWS)
        if self.kind == "waves":
            return list(SUPERPOSE_LENS[:D]), SUPERPOSE_L
        if self.kind == "rows":
            return pool_lens(FRAMES_L, D), FRAMES_L
        raise AssertionError(self.kind)

    def plan(self, cus):
        an = self.an
        launches = an.launches()
        cap = cus * launches[0][2]
        D = pick_d(cap)
        lens, L = self.shape(D)
        loops = 3 if self.kind == "triple" else 2

        def sizings(n):
            out = []
            for what, tile, per_cu in launches:
                what = f"{what}, {self.kind}, {'packed' if self.packed else 'padded'}, {cus} CUs"
                need = 2 * cus * per_cu + D if self.kind == "triple" else None
                if self.kind == "waves":
                    out.append(size_waves(what, cus, D, n))
                elif self.kind == "rows":
                    out.append(size_rows(what, cus, per_cu, tile, L, D, n))
                elif self.packed:
                    out.append(size_packed(what, cus, per_cu, tile, lens, need, None if n is None else n // D))
                else:
                    out.append(size_padded(what, cus, per_cu, tile, L, need, D, n))
            return out

        n = max(s.n for s in sizings(None))
        out = sizings(n)
        if getattr(an, "searches", False):
            # tmscore_rows / gdt_rows: search grid = min(tm_items_bound(packed ? rows : n * rows, n), n_cu * 16) over the items the device counts
            _, ref = an.pool_and_ref(lens, L)
            items = n // D * sum(search_items(ref["sites"]))
            rows = n // D * int(np.sum(lens)) if self.packed else n * L
            cap = cus * WAVES_PER_CU
            assert tm_items_bound(rows, n) >= items, (tm_items_bound(rows, n), items)
            out.append(Sizing(f"{an.name} search items, {'packed' if self.packed else 'padded'}, {cus} CUs", n, D, items, cap + cap // MARGIN, cap,
                              min(tm_items_bound(rows, n), cap)))
            if an.name == "gdt":                                          # k_gdt_final: final_grid(std::min(n, max_blocks))
                out.append(Sizing(f"gdt final, {cus} CUs", n, D, n, cap + cap // MARGIN, cap, min(n, cap)))
        return Plan(tuple(lens), L, n, self.packed, tuple(out), loops)

    def drive(self, codec, cus):
        p = self.plan(cus).check()
        return drive(codec, self.an, list(p.lens), p.L, p.n, p.packed, self.id)



def _cases():
    row = [Knn(4, 1, 5), Knn(14, 4, 17), Lddt(4, 1), Lddt(14, 4), LddtSoft(), HBOND, Labels(), Apply()]
    out = [Case(an, "one", packed) for an in row for packed in (False, True)]
    out += [Case(an, "three") for an in (row[0], row[2], row[4], row[5], row[6], row[7])]
    out += [Case(row[0], "triple")]
    out += [Case(row[0], "passes", own_pass=KNN_PASS), Case(row[2], "passes", own_pass=LDDT_PASS), Case(row[4], "passes", own_pass=LDDT_PASS),
            Case(HBOND, "passes", own_pass=HBOND_PASS)]
    out += [Case(an, "atoms", packed) for an in (Sasa(14), Violations(14), Violations(37), LddtAtoms(14)) for packed in (False, True)]
    out += [Case(Superpose(), "waves", packed) for packed in (False, True)]
    out += [Case(an, "waves", packed) for an in (TmScore(), Gdt()) for packed in (False, True)]
    out += [Case(Frames(1), "rows"), Case(Frames(0), "rows")]
    return out


CASES = _cases()


# ---- TM-align: pairs of chains of two small sets --------------------------------------------------------------------------------------------
TMALIGN_DIR_BUDGET = 256 << 20  # fcz_abi.hip: constexpr size_t TMALIGN_DIR_BUDGET = (size_t)256 << 20
TMALIGN_LENS = (0, 1, 3, 5, 9, 17, 33)                                        # _tmalign.ALIGN_LENGTHS up to 33 behind a chain of no row and of one
TMALIGN_STRIDE = 10             # pair k of the list is distinct pair k * 10 % 49: coprime with 49, so every pair is met in turn


def tmalign_dir_slots(want, wa):
    """fcz_abi.hip: max(1, min(want, TMALIGN_DIR_BUDGET / (wa * WAVE * sizeof(uint32_t))))"""
    return max(1, min(want, TMALIGN_DIR_BUDGET // (wa * 64 * 4)))


def tmalign_pool():
    """-> (sa, sb, the D * D distinct pairs, the restatement of those pairs): every chain of a against every chain of b, b's chains related
    to a's (TA.related) and so mostly unrelated to the other six. The conditions of test_tmalign_cpu.py are asserted for all 49."""
    import _tmalign as TA
    if "tmalign" not in _POOLS:
        rng = np.random.default_rng(TA.ALIGN_SEED)
        ca = [SP.walk_chain(rng, m) if m >= 3 else rng.uniform(-20, 20, (m, 3)) for m in TMALIGN_LENS]
        cb = [TA.related(rng, x) if len(x) >= 3 else rng.uniform(-20, 20, (len(x), 3)) for x in ca]
        sa, sb = TA.padded_set([c.astype(F) for c in ca]), TA.padded_set([c.astype(F) for c in cb])
        D = len(TMALIGN_LENS)
        pairs = np.asarray([(i, j) for i in range(D) for j in range(D)], np.int32)
        traces = []
        ref = TA.align_sets(sa, sb, pairs, sa["pos"].shape[1], sb["pos"].shape[1], 1, traces)
        for e, tr in enumerate(traces):
            margin, gap, dps_ok, lead, shared, _, exact_ties = TA.fairness(tr)
            assert margin >= 1e-8 and shared and gap >= 1e-3 and dps_ok and exact_ties and lead >= 1e-9, (e, margin, shared, gap, dps_ok, lead, exact_ties)
        _POOLS["tmalign"] = (sa, sb, pairs, ref)
    return _POOLS["tmalign"]


def tmalign_plan(cus):
    """-> (m, which distinct pair every pair of the list is, the sizings of tmalign_rows' three grids)"""
    import _tmalign as TA
    sa, sb, pairs, ref = tmalign_pool()
    wa, D2 = sa["pos"].shape[1], len(pairs)
    assert math.gcd(TMALIGN_STRIDE, D2) == 1
    m = ceil_div(cus * 64 + cus * 8, D2) * D2
    which = np.arange(m) * TMALIGN_STRIDE % D2
    # k_ta_count: min(grid_for(m, WAVES_PER_BLOCK), n_cu * 16) blocks, a wavefront a pair
    cap = cus * WAVES_PER_CU
    count = Sizing(f"tmalign count, {cus} CUs", m, 7, ceil_div(m, WAVES_PER_BLOCK), cap + cap // MARGIN, cap, min(ceil_div(m, WAVES_PER_BLOCK), cap))
    # k_ta_search: search = max(1, dir_slots(min(items, n_cu * 2) * 4, wa) / 4) blocks over the items the device counts, four seeds each; the
    # launcher's bound on the items is m times a per-pair bound, so at least m
    per_pair = [ceil_div(len(TA.seed_list(int(a), int(b))), WAVES_PER_BLOCK) for a, b in zip(ref["sites_a"], ref["sites_b"])]
    items = int(np.asarray(per_pair)[which].sum())
    assert m >= cus * 2
    search = max(1, tmalign_dir_slots(cus * 2 * WAVES_PER_BLOCK, wa) // WAVES_PER_BLOCK)
    assert search == cus * 2, (search, "the traceback budget, not the CU count, bounds the search grid")
    srch = Sizing(f"tmalign search items, {cus} CUs", m, 7, items, search + search // MARGIN, search, min(items, search))
    # the direction slots are search * 4, and k_ta_final runs min(m, search * 4) blocks, a pair each
    slots = search * WAVES_PER_BLOCK
    final = Sizing(f"tmalign direction slots / final, {cus} CUs", m, 7, m, slots + slots // MARGIN, slots, min(m, slots))
    return m, which, (count, srch, final)


def tmalign_check(got, ref, what):
    """test_gpu_tmalign.py's comparison: map, aligned, seed, sites and status exactly, the floats by _superpose.close's tolerance for each
    of the three normalisations, the transform where three or more pairs are aligned"""
    for k in ("map", "aligned", "seed", "sites_a", "sites_b", "status"):
        bad = got[k] != ref[k]
        assert got[k].dtype == np.int32 and not bad.any(), (what, k, np.argwhere(bad)[:4], got[k][bad][:4], ref[k][bad][:4])
    solved = ref["aligned"] >= 3
    zeros = np.zeros((len(solved), 5), np.int32)
    for tm in ("tm", "tm_a", "tm_b"):
        g = dict(sites=got["aligned"], gdt_counts=zeros, trans=got["trans"], rmsd=got["rmsd"], tm=got[tm], dev=got["dev"], rot=got["rot"])
        r = dict(sites=ref["aligned"], gdt_counts=zeros, trans=ref["trans"], rmsd=ref["rmsd"], tm=ref[tm], dev=ref["dev"], rot=ref["rot"])
        SP.close(g, r, what, compare_rot=solved)
    SP.proper(got["rot"], what)


def drive_tmalign(codec, cus):
    """the three assertions for fcz_tmalign_dev: m pairs cycling through the 49 distinct ones against the 49 alone"""
    import _tmalign as TA
    m, which, sizings = tmalign_plan(cus)
    for s in sizings:
        s.check()
    sa, sb, pairs, ref = tmalign_pool()
    wa, wb = sa["pos"].shape[1], sb["pos"].shape[1]
    da, db = TA.to_device(sa), TA.to_device(sb)
    small = TA.run_dev(codec, da, db, to_dev(pairs), wa, wb, LAYOUT[4], 1)
    big = TA.run_dev(codec, da, db, to_dev(pairs[which]), wa, wb, LAYOUT[4], 1)
    for k, g in big.items():
        left = (_raw(g) == FILL).all(axis=1)
        assert not left.any(), ("tmalign", k, "pairs still 0xA5", int(left.sum()), np.flatnonzero(left)[:4])
    assert_bytes(big, {k: v[which] for k, v in small.items()}, "tmalign")
    tmalign_check(big, {k: v[which] for k, v in ref.items()}, "tmalign")
    assert (ref["seed"] > 0).any() and (ref["aligned"] >= 3).sum() >= 16 and (ref["status"] == 0).all()
    return small, big
