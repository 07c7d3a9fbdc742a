"""GPU: the launch plan that fcz_compress_batch_dev / fcz_decompress_batch_dev (foldcomp_amd/csrc/fcz_abi.hip) build per batch,
HIP vs oracle, bit for bit. The plan is a function of batch-level quantities -- the longest segment and the most segments of ANY
record, the number of long chains, the residue total, the chain count -- so one unusual record changes ring sizes, kernel
variants and the number of launches for every other record. Every case below mirrors the plan arithmetic in Python (`_plan`),
asserts from the records it built that the batch takes the branch it names, and only then compares with the oracle (which is
per-chain and stateless, hence blind to batch shape by construction).

Not covered: the NON-split long route (n_long >= 2 * 4 * n_cu * 64, about 131 000 chains of >= 1 024 residues = more than 134 M
residues) does not fit a test's time; long chains reach k_backbone<0> only through that route.
The persistent grids of the analyses over dense tensors are crossed in tests/test_gpu_sweep_grids.py."""
import dataclasses
import functools

import numpy as np
import pytest

import _harness as H
from _cases import concat_batches, entries_blob
from _devpath import DevRecords, compress_dev
from foldcomp_amd import synthetic
from foldcomp_amd._aa_tables import RES_NATOMS
from foldcomp_amd.structure import ChainBatch

pytestmark = pytest.mark.gpu

# ---- the plan arithmetic of fcz_abi.hip, mirrored ---------------------------------------------------------------------------
WAVE = 64                       # fcz_kernels.h: constexpr int WAVE = 64
WAVES_PER_BLOCK = 4             # fcz_kernels.h: constexpr int WAVES_PER_BLOCK = 4
BLOCK = WAVE * WAVES_PER_BLOCK  # fcz_kernels.h: constexpr int BLOCK = WAVE * WAVES_PER_BLOCK
FB_G = 8                        # fcz_backbone_fast.h: #define FCZ_FB_G 8
FB_CH = WAVE // FB_G            # fcz_backbone_fast.h: constexpr int FB_CH = WAVE / FB_G
FB_K = 32                       # fcz_backbone_fast.h: FB_K = FB_G * FB_S, FB_S = 32 / FB_G
FCZ_LONG_CHAIN = 1024           # fcz_kernels.h: constexpr uint32_t FCZ_LONG_CHAIN = 1024
SPLIT_CAP = 6 << 30             # fcz_abi.hip, split_long block: chunk = min(groups_long_all, ((size_t)6 << 30) / per_group)
FAST_CAP = 4 << 30              # fcz_abi.hip, fast_bb block: chunk = min(groups, ((size_t)4 << 30) / (FB_CH * col * sizeof(v3)))
V3 = 12                         # fcz_math.h: struct v3 { float x, y, z; }
MIN_WAVES = 2                   # fcz_kernels.h: #define FCZ_BACKBONE_MIN_WAVES 2
SZ_CHUNK = SCAN_CHUNK = 4096    # fcz_kernels.h: constexpr int SZ_CHUNK = 4096 / SCAN_CHUNK = 4096
CP_CHUNK = RI_CHUNK = 16        # fcz_compress.h: constexpr int CP_CHUNK = 16; fcz_sidechain.h: constexpr int RI_CHUNK = 16
CW_RES = WAVE - 1               # fcz_compress.h: constexpr int CW_RES = WAVE - 1
CW_GRID_FACTOR = 16             # fcz_abi.hip: #define FCZ_CW_GRID_FACTOR 16u
SC_TILE = CK_TILE = BLOCK       # fcz_sidechain.h: constexpr int SC_TILE = BLOCK; fcz_compress.h: constexpr int CK_TILE = BLOCK
SC_MIN_BLOCKS = 4               # fcz_sidechain.h: #define FCZ_SIDECHAIN_MIN_BLOCKS 4
SC_GRID_FACTOR = 16             # fcz_abi.hip: #define FCZ_SC_GRID_FACTOR 16u
CK_MIN_BLOCKS = 3               # fcz_compress.h: #define FCZ_COMPRESS_MIN_BLOCKS 3
MEM_BUDGET = 12 << 30           # what a case may ask of fwd + wring + fwd_long + wring_long + fast_scratch together
ORACLE_THREADS = 16


def _ceil(a, b):
    return (a + b - 1) // b


def _n_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)     # fcz_ctx_create: hipDeviceAttributeMultiprocessorCount


def _segments(fcz: bytes):
    """(longest segment, segments) of a record as k_entry_sizes counts them: nAnchor at byte 12, the anchor indices at byte 76; a
    segment between anchors a and b counts b - a + 1 residues"""
    na = fcz[12]
    idx = np.frombuffer(fcz, np.int32, na, 76)
    return (int(np.diff(idx).max()) + 1 if na > 1 else 0), na - 1


def _shape(entries, res_counts):
    """the batch-level quantities the sizes pass reduces (k_sizes_reduce / k_sizes_mid), and the records they come from"""
    seg = [_segments(e) for e in entries]
    i_seg = int(np.argmax([s[0] for s in seg])); i_nseg = int(np.argmax([s[1] for s in seg]))
    return dict(n=len(entries), R=int(np.sum(res_counts)), max_seg=seg[i_seg][0], max_nseg=seg[i_nseg][1], i_seg=i_seg, i_nseg=i_nseg,
                n_long=int(np.sum(np.asarray(res_counts) >= FCZ_LONG_CHAIN)))


def _plan(s, n_cu):
    """fcz_decompress_batch_dev's choices for a batch of shape s: the exact route (split long chains + fused rest) and the fast one"""
    p = dict(s)
    ring_rows = 3 * max(s["max_seg"], 1)
    slot_bytes = ring_rows * WAVE * V3 + (ring_rows // 3) * 6 * WAVE * 4         # slot_atoms * sizeof(v3) + slot_trig * sizeof(float)
    p["groups_long_all"] = _ceil(s["n_long"], WAVE)
    p["split_long"] = s["n_long"] > 0 and s["max_nseg"] > 0 and p["groups_long_all"] < 2 * 4 * n_cu
    p["per_group"] = s["max_nseg"] * slot_bytes
    p["long_chunk"] = max(1, min(p["groups_long_all"], SPLIT_CAP // p["per_group"])) if p["split_long"] else 0
    p["long_launches"] = _ceil(p["groups_long_all"], p["long_chunk"]) if p["split_long"] else 0
    n_split = s["n_long"] if p["split_long"] else 0
    p["groups"] = _ceil(s["n"] - n_split, WAVE)
    p["blocks0"] = min(p["groups"], n_cu * 4 * MIN_WAVES)
    p["exact_bytes"] = p["long_chunk"] * p["per_group"] + max(p["blocks0"], 1) * slot_bytes
    # fast numerics
    p["fast_groups"] = _ceil(s["n"], FB_CH)
    p["need_scratch"] = s["max_seg"] > FB_K + 1
    col = 3 * s["max_seg"] if p["need_scratch"] else 0
    p["fast_chunk"] = max(1, min(p["fast_groups"], FAST_CAP // (FB_CH * col * V3))) if p["need_scratch"] else p["fast_groups"]
    p["fast_launches"] = _ceil(p["fast_groups"], p["fast_chunk"])
    p["fast_bytes"] = p["fast_chunk"] * FB_CH * col * V3
    # dev_buf::ensure asks for an eighth more than it needs
    p["bytes"] = (p["exact_bytes"] + p["fast_bytes"]) * 9 // 8
    return p


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _gen(lens, seed, thr=25, res_code=None, device="cpu"):
    """(the generator walks the longest chain residue by residue: a few long chains are quicker on the host, many short ones on the device)"""
    return synthetic.to_chain_batch(synthetic.generate(len(lens), lens, seed=seed, anchor_threshold=thr, res_code=res_code, device=device))


@functools.lru_cache(maxsize=None)
def _pool(name):
    """chains that several cases use (the generator's cost grows with the longest chain: made once)"""
    if name == "deep":                  # a 6 000- and a 5 000-residue chain: many segments at -b 25, one long segment at -b 5000 and more
        return _gen([6000, 5000], 1001)
    if name == "edge":                  # 65 chains of 1 024 .. 1 028 residues, 65 of 1 023 and fewer
        return _gen([1024] * 3 + [1024 + (i % 5) for i in range(62)] + [1023] * 3 + [2 + (37 * i) % 1022 for i in range(62)], 1030)
    raise KeyError(name)


def _at(b, thr):
    return dataclasses.replace(b, anchor_threshold=thr)


def _records(codec, b):
    """compress on the device and with the oracle: same statuses, offsets and bytes -> the records as a list"""
    blob, off, st = codec.compress_batch(b)
    oblob, ooff, ost = H.oracle_compress(b, n_threads=ORACLE_THREADS)
    assert (st == 0).all() and (ost == 0).all()
    assert np.array_equal(off, ooff) and blob.tobytes() == oblob.tobytes()
    return [oblob[int(ooff[c]):int(ooff[c + 1])].tobytes() for c in range(b.n_chains)]


def _same_as_oracle(d, o, what):
    assert np.array_equal(d["res_off"], o["res_off"]) and np.array_equal(d["atom_off"], o["atom_off"]), what
    for k in ("x", "y", "z", "bfac_res"):
        if not np.array_equal(_bits(d[k]), _bits(o[k])):
            bad = np.nonzero(_bits(d[k]) != _bits(o[k]))[0]
            off = o["res_off"] if k == "bfac_res" else o["atom_off"]
            recs = np.unique(np.searchsorted(off, bad, side="right") - 1)
            raise AssertionError((what, k, "differs in", len(bad), "values of records", recs[:8].tolist(), "of", len(off) - 1))
    assert np.array_equal(d["atom_code"], o["atom_code"]) and np.array_equal(d["res_code"], o["res_code"]), what
    if "info" in d:
        n = len(o["res_off"]) - 1
        assert [d["info"][i].status for i in range(n)] == [o["info"][i].status for i in range(n)], what


def _decode_check(codec, entries, alts=(False, True), what=""):
    blob, off = entries_blob(entries)
    out = None
    for alt in alts:
        d = codec.decompress_batch(blob, off, alt_order=alt)
        o = H.oracle_decompress(blob, off, alt_order=alt, n_threads=ORACLE_THREADS)
        _same_as_oracle(d, o, (what, "alt" if alt else "default"))
        out = d
    return blob, off, out


def _res_counts(entries):
    blob, off = entries_blob(entries)
    o = H.oracle_decompress(blob, off, n_threads=ORACLE_THREADS)
    assert all(o["info"][i].status == 0 for i in range(len(entries)))
    return np.diff(o["res_off"].astype(np.int64))


# ---- (a) (b) (c) (d): the exact decoder's long-chain routes ------------------------------------------------------------------
def test_split_long_route_in_several_chunks(codec):
    """(a) one record with many segments (6 000 residues at -b 25) and one with a long segment (5 000 at -b 5000) make the
    per-group ring of the split long route gigabytes, so the 6 GB cap cuts it: k_backbone<1> / <2> are launched once per chunk on
    the second stream over the same fwd_long, each with perm + g0 * 64 and its own slot count. One long chain more than the
    chunks before it hold, so the last launch carries a single chain; four short chains take the fused kernel beside them."""
    n_cu = _n_cu()
    many = _records(codec, _at(_pool("deep"), 25))[:1]
    deep = _records(codec, _at(_pool("deep"), 5000))[1:]
    s0 = _shape(many + deep, [6000, 5000])
    p0 = _plan(s0, n_cu)
    chunk = SPLIT_CAP // p0["per_group"]
    assert 1 <= chunk <= 4, ("the two records no longer make the ring gigabytes", p0)
    n_long = chunk * WAVE + 1                       # ceil(n_long / 64) = chunk + 1 groups: two launches, the last with one chain
    lens = [1024 + (i % 7) for i in range(n_long - 2)]
    rest = _records(codec, _gen(lens, 1003, 25))
    short = _records(codec, _gen([2, 63, 350, 1023], 1004, 25))
    entries = rest[:40] + many + short[:2] + rest[40:] + deep + short[2:]
    p = _plan(_shape(entries, _res_counts(entries)), n_cu)
    assert p["i_seg"] != p["i_nseg"]                                    # ring depth and segment count come from different records
    assert p["split_long"] and p["groups_long_all"] > p["long_chunk"] and p["long_launches"] >= 2, p
    assert p["n_long"] - (p["long_launches"] - 1) * p["long_chunk"] * WAVE == 1, p     # the last launch is ragged: one slot
    assert p["groups"] == 1 and p["bytes"] < MEM_BUDGET, p
    _decode_check(codec, entries, what="split long route, several chunks")


def test_batch_of_long_chains_only(codec):
    """(b) every chain is long: no fused launch at all (groups == 0, no k_backbone<0>, next_group is not cleared); the residue index
    and side-chain stages are ordered behind the second stream by the join event alone"""
    lens = [1024, 1025, 2700]
    entries = _records(codec, _gen(lens, 1011, 25))
    p = _plan(_shape(entries, _res_counts(entries)), _n_cu())
    assert p["split_long"] and p["n_long"] == p["n"] == 3 and p["groups"] == 0 and p["blocks0"] == 0, p
    _decode_check(codec, entries, what="long chains only")


def test_mixed_anchor_thresholds_in_one_batch(codec):
    """(c) records written at -b 2, 7, 25, 200 and 5000 decoded as one batch: the ring depth (max_seg) comes from a -b 5000 record,
    the segment count (max_nseg) from a -b 2 one, and every other record walks a ring sized by neither of its own numbers. Lengths
    on both sides of 64 (k_res_index_rows / k_res_index) and 1 024 (fused / split)."""
    upper = _gen([2, 63, 64, 65, 1023, 1024, 1025, 2700], 1022)                  # (-b 2 and -b 7 cannot hold them: n / b + 2 anchors <= 255)
    entries, thr_of = [], []
    for thr, b in ((2, _gen([30, 63, 64, 65, 506], 1020, 2)), (7, _gen([2, 63, 65, 1023, 1024, 1500], 1021, 7)), (25, upper), (200, upper), (5000, upper)):
        entries += _records(codec, _at(b, thr)); thr_of += [thr] * b.n_chains
    order = np.random.default_rng(1021).permutation(len(entries))
    entries = [entries[i] for i in order]; thr_of = [thr_of[i] for i in order]
    p = _plan(_shape(entries, _res_counts(entries)), _n_cu())
    assert thr_of[p["i_seg"]] == 5000 and thr_of[p["i_nseg"]] == 2 and p["max_seg"] == 2700 and p["max_nseg"] == 506 // 2 + 1, p
    assert p["split_long"] and p["n_long"] == 11 and p["groups"] == 1 and p["bytes"] < MEM_BUDGET, p
    _decode_check(codec, entries, what="mixed thresholds")
    # the same records through the device-pointer entry points (sizes pass + remembered totals), both offsets against the oracle's
    blob, off = entries_blob(entries)
    o = H.oracle_decompress(blob, off, n_threads=ORACLE_THREADS)
    _same_as_oracle(DevRecords(blob, off).decompress(codec), o, "mixed thresholds, device arrays")


@pytest.mark.parametrize("n_long", [1, 63, 64, 65])
def test_long_chain_count_at_the_wavefront_edges(codec, n_long):
    """(d) the long chains are the head of the length order (perm), the fused kernel starts at perm + n_split: 1, 63, 64 and 65 long
    chains (one wavefront group nearly full, full, and one chain into the second) with 0, 1 and 65 shorter chains behind them.
    1 023- and 1 024-residue chains sit side by side: they share no bucket of the counting sort, and only the latter is long."""
    both = _records(codec, _pool("edge"))
    longs, shorts = both[:n_long], both[65:]
    n_cu = _n_cu()
    for n_short in (0, 1, 65):
        # long and short interleaved in input order: the order the kernels walk is perm's, not the caller's
        entries = list(longs); rng = np.random.default_rng(n_long * 100 + n_short)
        for e in shorts[:n_short]:
            entries.insert(int(rng.integers(0, len(entries) + 1)), e)
        p = _plan(_shape(entries, _res_counts(entries)), n_cu)
        assert p["split_long"] and p["n_long"] == n_long and p["n"] == n_long + n_short, p
        assert p["groups_long_all"] == _ceil(n_long, 64) and p["long_launches"] == 1 and p["groups"] == _ceil(n_short, 64), p
        _decode_check(codec, entries, alts=(bool(n_short & 1),), what=(n_long, n_short))


# ---- (e) (f): the fast backbone's scratch columns -----------------------------------------------------------------------------
def _backbone_dev_per_chain(a, b):
    """largest |a - b| over the backbone atoms (N, CA, C lead every residue in the default order) of every chain"""
    dev = np.max(np.abs(np.stack([a[k].astype(np.float64) - b[k] for k in ("x", "y", "z")])), axis=0)
    ro = a["res_off"].astype(np.int64); ao = a["atom_off"].astype(np.int64)
    nat = np.asarray(RES_NATOMS, np.int64)[a["res_code"]]
    before = np.concatenate([[0], np.cumsum(nat)[:-1]])                 # atoms of the residues before, OXT not counted
    chain = np.searchsorted(ro, np.arange(len(nat)), side="right") - 1
    start = ao[chain] + before - before[ro[chain]]
    dev_res = np.maximum(np.maximum(dev[start], dev[start + 1]), dev[start + 2])
    return np.maximum.reduceat(dev_res, ro[:-1]), dev


@pytest.mark.parametrize("launches,ragged", [(3, 0), (2, 1), (2, 47)])
def test_fast_backbone_scratch_in_several_launches(codec, launches, ragged):
    """(e) (f) fast numerics: one record with a 6 000-residue segment makes the scratch column of EVERY chain 18 000 atoms, so the
    4 GB cap cuts the launch of ~20 000 tiny chains: k_backbone_fast relaunched with perm + g0 * 8 over the same scratch.
    (3, 0): three launches, n a multiple of 8. (2, 1) and (2, 47): the last launch holds 1 / 47 chains (n = 1, 7 mod 8: a last
    group of one / seven chains). The yardstick is the oracle's decode of the same records (the exact decoder equals it bit for bit
    in every other test; run on this batch it would ask 23 MB of ring per wavefront). The fast decoder is
    held to the bars of test_gpu_fast_numerics.py (backbone per chain under 2e-3 * max(1, seg / 32) ** 1.5; median < 1e-4 and
    99.9 % < 2e-3 over the atoms of the chains whose segments are short) and to itself: a chain decoded alone in a small batch gives the same bits as in
    the launch that carried it here -- its arithmetic does not depend on its lane group, launch or column."""
    n_cu = _n_cu()
    deep = _records(codec, _at(_pool("deep"), 30000))[:1]
    seg0 = _segments(deep[0])[0]
    assert seg0 == 6000
    chunk = FAST_CAP // (FB_CH * 3 * seg0 * V3)
    last = ragged or 24                                                         # chains in the last launch
    n = (launches - 1) * chunk * FB_CH + last
    lens = np.random.default_rng(1042).integers(2, 41, n - 1)
    tiny = _records(codec, _gen(lens, 1043, 25, device="cuda:0"))
    at = n // 3
    entries = tiny[:at] + deep + tiny[at:]
    p = _plan(_shape(entries, _res_counts(entries)), n_cu)
    assert p["need_scratch"] and p["fast_chunk"] == chunk and p["fast_groups"] * FB_CH * 3 * p["max_seg"] * V3 > FAST_CAP, p
    assert p["fast_launches"] == launches and p["n"] == n and n % FB_CH == ragged % FB_CH, p
    assert min(n - (launches - 1) * chunk * FB_CH, chunk * FB_CH) == last, p      # slots of the last launch
    assert p["fast_bytes"] * 9 // 8 < MEM_BUDGET, p
    blob, off = entries_blob(entries)
    a = H.oracle_decompress(blob, off, n_threads=ORACLE_THREADS)
    codec.set_numerics(True)
    try:
        b = codec.decompress_batch(blob, off)
        # alone: the long-segment record and a sample of the tiny ones (first, last, the neighbours of the long one, every 97th)
        pick = sorted(set([0, 1, at - 1, at, at + 1, n - 2, n - 1] + list(range(5, n, 97))))
        sblob, soff = entries_blob([entries[i] for i in pick])
        alone = codec.decompress_batch(sblob, soff)
    finally:
        codec.set_numerics(False)
    assert np.array_equal(a["atom_off"], b["atom_off"]) and np.array_equal(a["res_off"], b["res_off"])
    assert np.array_equal(a["atom_code"], b["atom_code"]) and np.array_equal(a["res_code"], b["res_code"])
    assert np.array_equal(_bits(a["bfac_res"]), _bits(b["bfac_res"]))
    assert all(np.isfinite(b[k]).all() for k in ("x", "y", "z"))
    per_chain, dev = _backbone_dev_per_chain(a, b)
    seg = np.asarray([_segments(e)[0] - 1 for e in entries], np.float64)         # residue steps, as _longest_segment counts
    bar = 2e-3 * np.maximum(1.0, seg / 32.0) ** 1.5
    worst = int(np.argmax(per_chain / bar))
    assert (per_chain < bar).all(), (worst, per_chain[worst], bar[worst])
    ao = a["atom_off"].astype(np.int64)
    rest = np.ones(len(dev), bool); rest[ao[at]:ao[at + 1]] = False             # the -b 25 chains: the quantile rule
    med, p999 = float(np.median(dev[rest])), float(np.quantile(dev[rest], 0.999))
    assert med < 1e-4 and p999 < 2e-3, (med, p999)
    sao = alone["atom_off"].astype(np.int64)
    for j, i in enumerate(pick):
        for k in ("x", "y", "z"):
            assert np.array_equal(_bits(alone[k][sao[j]:sao[j + 1]]), _bits(b[k][ao[i]:ao[i + 1]])), ("alone vs in the batch", i, k)


# ---- (g): compress_pack_rows classes and the chunk-of-16 scan --------------------------------------------------------------------
def _refuse(b, chains):
    """chains[c] = 'nan' | 'inf': a non-finite coordinate / B-factor in chain c. -> (batch, expected statuses)"""
    x, bf = b.x.copy(), b.bfac_ca.copy()
    want = np.zeros(b.n_chains, np.int32)
    for c, how in chains.items():
        r0, n = int(b.res_off[c]), int(b.res_off[c + 1] - b.res_off[c])
        if n < 2:
            continue
        if how == "nan":
            bf[r0 + n - 1] = np.nan
        else:
            x[int(b.atom_off[r0 + n // 2])] = np.inf
        want[c] = -9                                                             # FCZ_E_NONFINITE
    return ChainBatch(res_off=b.res_off, atom_off=b.atom_off, x=x, y=b.y, z=b.z, atom_code=b.atom_code, res_code=b.res_code, bfac_ca=bf,
                      first_res_index=b.first_res_index, first_atom_index=b.first_atom_index, chain_id=b.chain_id, titles=b.titles,
                      title_off=b.title_off, anchor_threshold=b.anchor_threshold), want


@pytest.mark.parametrize("thr", [25, 3])
def test_pack_rows_class_edges_across_the_chunk_scan(codec, thr):
    """(g) k_compress_pack_rows<1|2|4|8> each scan chunks of 16 consecutive chains for the lengths of their class (2..16, 17..32,
    33..64, 65..128); 129 and more are k_compress_pack's. Chunks that hold every class edge at once, runs of more than 16 chains
    of one class next to runs of another (whole chunks a class launch finds empty, chunks it owns entirely), refused chains (one
    residue: FCZ_E_TOO_SHORT; a NaN B-factor, an infinite coordinate: FCZ_E_NONFINITE) inside the chunks, and a chain count of
    16 k - 1, 16 k and 16 k + 1. Statuses as expected (the oracle's where it has the rule), refused records zero, every other record the oracle's.
    The same three batches through fcz_compress_sizes_dev / fcz_compress_batch_dev on device arrays."""
    edges = [2, 16, 17, 32, 33, 64, 65, 128, 129]
    lens = []
    lens += (edges + [1] + edges[:6]) * 3                                        # 16-chain chunks: every class edge and a refused chain
    lens += (edges[::-1] + [1, 1] + edges[3:8]) * 2
    for a, b_, na, nb in ((16, 17, 19, 23), (32, 33, 40, 17), (64, 65, 18, 35), (128, 129, 33, 20), (2, 128, 21, 21), (129, 2, 17, 30)):
        lens += [a] * na + [b_] * nb                                             # runs longer than a chunk, class against class
    lens += [1] * 17                                                             # a chunk of refused chains only
    lens += [2] * (-len(lens) % 16) + [129, 128, 65, 64, 33, 32, 17, 16, 2, 1, 2, 16, 17, 32, 33, 64, 65]
    k16 = len(lens) // 16 * 16
    assert len(lens) == k16 + 1
    full = _gen(lens, 1050 + thr, thr)
    classes = lambda ls: {u for u in (1, 2, 4, 8) for v in ls if (2 if u == 1 else u * 8 + 1) <= v <= u * 16}
    for C in (k16 - 1, k16, k16 + 1):
        assert classes(lens[:C]) == {1, 2, 4, 8} and any(classes(lens[c:c + 16]) == {1, 2, 4, 8} and 1 in lens[c:c + 16] for c in range(0, C - 15, 16))
        b0 = _prefix(full, C)
        bad = {c: ("nan", "inf")[c // 7 % 2] for c in range(3, C, 7)}
        bad[C - 1] = "inf"                                                       # the last chain of the batch, in a ragged chunk or not
        b, want = _refuse(b0, bad)
        want[np.asarray(lens[:C]) == 1] = -7                                     # FCZ_E_TOO_SHORT
        # (the reference has no rule for non-finite input and writes NaN records: the oracle compresses the clean chains, per chain)
        oblob, ooff, ost = H.oracle_compress(b0, n_threads=ORACLE_THREADS)
        assert np.array_equal(ost != 0, np.asarray(lens[:C]) == 1) and np.array_equal(ost[ost != 0], want[ost != 0])
        for how in ("host arrays", "device arrays"):
            blob, off, st = codec.compress_batch(b, strict=False) if how == "host arrays" else compress_dev(codec, b)
            assert np.array_equal(st, want), (how, thr, C, np.nonzero(st != want)[0][:10], st[st != want][:10])
            assert np.array_equal(off, ooff), (how, thr, C)
            for c in range(C):
                rec = blob[int(off[c]):int(off[c + 1])].tobytes()
                assert rec == (bytes(len(rec)) if want[c] else oblob[int(ooff[c]):int(ooff[c + 1])].tobytes()), (how, thr, C, c, lens[c])
        good = [oblob[int(ooff[c]):int(ooff[c + 1])].tobytes() for c in range(C) if want[c] == 0]
        _decode_check(codec, good, alts=(C == k16,), what=("decode of the class-edge batch", thr, C))


def _prefix(b: ChainBatch, C: int) -> ChainBatch:
    """the first C chains of a batch"""
    R = int(b.res_off[C]); M = int(b.atom_off[R]); T = int(b.title_off[C])
    return ChainBatch(res_off=b.res_off[:C + 1].copy(), atom_off=b.atom_off[:R + 1].copy(), x=b.x[:M].copy(), y=b.y[:M].copy(), z=b.z[:M].copy(),
                      atom_code=b.atom_code[:M].copy(), res_code=b.res_code[:R].copy(), bfac_ca=b.bfac_ca[:R].copy(),
                      first_res_index=b.first_res_index[:C].copy(), first_atom_index=b.first_atom_index[:C].copy(), chain_id=b.chain_id[:C].copy(),
                      titles=b.titles[:T].copy(), title_off=b.title_off[:C + 1].copy(), anchor_threshold=b.anchor_threshold)


# ---- (h): the persistent grids, just under their caps and beyond ---------------------------------------------------------------
def _roundtrip_dev(codec, b, what, alt=False, compress=True, decompress=True):
    """device-array compress and / or decompress of a batch against the oracle: offsets, records, coordinates"""
    oblob, ooff, ost = H.oracle_compress(b, n_threads=ORACLE_THREADS)
    assert (ost == 0).all()
    if compress:
        blob, off, st = compress_dev(codec, b)
        assert (st == 0).all(), what
        assert np.array_equal(off, ooff), what                                   # == cumsum of the oracle's record sizes
        if blob.tobytes() != oblob.tobytes():
            bad = [c for c in range(b.n_chains) if blob[int(off[c]):int(off[c + 1])].tobytes() != oblob[int(off[c]):int(off[c + 1])].tobytes()]
            raise AssertionError((what, "records differ", bad[:8], len(bad)))
    if not decompress:
        return
    blob, off = oblob, ooff
    o = H.oracle_decompress(oblob, ooff, alt_order=alt, n_threads=ORACLE_THREADS)
    assert np.array_equal(o["res_off"], b.res_off)
    _same_as_oracle(DevRecords(blob, off).decompress(codec, alt), o, what)


def test_chain_count_caps_of_the_persistent_grids(codec):
    """(h) grids sized by the CHAIN count: k_compress_pack_rows runs min(ceil(ceil(C / 16) / 4), n_cu * 4) blocks, k_res_index_rows
    min(ceil(ceil(n / 16) / 4), n_cu * 8), k_backbone<0> min(ceil(n / 64), n_cu * 4 * 2) -- one block under each cap, at it, and one
    beyond (the first batch whose blocks take a second chunk / group). Chains of 2 .. 5 residues keep the batches small."""
    n_cu = _n_cu()
    rows_cap, index_cap, bb_cap = n_cu * 4, n_cu * 8, n_cu * 4 * MIN_WAVES
    assert index_cap == bb_cap                          # k_res_index_rows and k_backbone<0> cap at the same chain count: 64 per block
    counts = []
    for cap in (rows_cap, index_cap):
        counts += [(cap - 1) * 64, cap * 64, cap * 64 + 1]
    pool = _gen([2 + (i * 7) % 4 for i in range(max(counts))], 1060, 25, device="cuda:0")
    for C in counts:
        rows = _ceil(_ceil(C, CP_CHUNK), WAVES_PER_BLOCK); groups = _ceil(C, WAVE)
        cap = rows_cap if C <= rows_cap * 64 + 1 else index_cap
        assert rows == groups and rows in (cap - 1, cap, cap + 1), (C, rows, cap)
        _roundtrip_dev(codec, _prefix(pool, C), ("chain-count cap", C), alt=bool(C & 1))


def test_residue_count_caps_of_the_persistent_grids(codec):
    """(h) grids sized by the RESIDUE total: k_compress_angles_w runs min(ceil(ceil(R / 63) / 4), n_cu * 3 * 16) blocks, k_compress_angles
    min(ceil(R / 256), n_cu * 3), the side-chain stage min(ceil(R / 256), n_cu * 4 * 16): R one block under each cap, at it, one residue
    beyond. 350-residue chains and one tail chain that lands the total. The two large grids are run on the side they belong to only (the
    records of the decompress batches are the oracle's)."""
    n_cu = _n_cu()
    targets = []
    # (residues per block, cap in blocks, the side whose grid it is)
    for per_block, cap, side in ((CK_TILE, n_cu * CK_MIN_BLOCKS, "both"), (CW_RES * WAVES_PER_BLOCK, n_cu * 3 * CW_GRID_FACTOR, "compress"),
                                 (SC_TILE, n_cu * SC_MIN_BLOCKS * SC_GRID_FACTOR, "decompress")):
        targets += [(per_block * (cap - 1), per_block, cap, cap - 1, side), (per_block * cap, per_block, cap, cap, side),
                    (per_block * cap + 1, per_block, cap, cap + 1, side)]
    L = 350
    pool = _gen([L] * (max(t[0] for t in targets) // L), 1070, 25, device="cuda:0")
    for i, (R, per_block, cap, blocks, side) in enumerate(targets):
        k = (R - 2) // L
        tail = R - k * L
        assert 2 <= tail <= L + 1
        b = concat_batches([_prefix(pool, k), _gen([tail], 1071 + i, 25)])
        assert b.n_residues == R and _ceil(R, per_block) == blocks, (R, per_block, cap)
        _roundtrip_dev(codec, b, ("residue-count cap", R, per_block, cap), alt=bool(i & 1), compress=side != "decompress", decompress=side != "compress")


# ---- (i): chunk edges of the scans and of the sizes pass -------------------------------------------------------------------------
@pytest.mark.parametrize("C", [4095, 4096, 4097])
def test_scan_chunk_edges(codec, C):
    """(i) k_scan_reduce / k_scan_apply / k_scan_u64 (compress: record offsets) and k_sizes_reduce / _mid / _apply (decompress: residue
    and atom offsets, the length order) work in chunks of 4 096 chains: one chain under a chunk, a full chunk, one chain into the second.
    out_off, res_off and atom_off against the cumulative sums of the oracle's sizes, then records and coordinates."""
    assert SCAN_CHUNK == SZ_CHUNK == 4096 and _ceil(C, SCAN_CHUNK) == (1 if C <= 4096 else 2)
    lens = np.random.default_rng(C).integers(2, 41, C); lens[-1] = 40; lens[0] = 2
    b = _gen(lens, 1080 + C, 25)
    _roundtrip_dev(codec, b, ("scan chunk edge", C))


def test_sizes_pass_beyond_1024_chunks(codec):
    """(i) k_sizes_mid and k_scan_u64 are single blocks of 1 024 threads that walk the chunk sums 1 024 at a time: 1 024 * 4 096 + 1
    records give 1 025 chunk sums, one into the second round. Three small records tiled on the device; res_off / atom_off against the
    cumulative sums of the oracle's counts, the coordinates of every tile against the oracle's decode of the three."""
    import torch
    unit = _records(codec, _gen([2, 5, 3], 1090, 25))
    blob, off = entries_blob(unit)
    o = H.oracle_decompress(blob, off, n_threads=1)
    n = 1024 * SZ_CHUNK + 1
    tiles = _ceil(n, 3)
    assert _ceil(n, SZ_CHUNK) == 1025
    dev = "cuda:0"
    rec = DevRecords(blob, off)
    rec.blob_t = torch.from_numpy(blob).to(dev).repeat(tiles + 1)
    rel = torch.from_numpy(off[:3].astype(np.int64)).to(dev)
    rec.off_t = (torch.arange(tiles + 1, dtype=torch.int64, device=dev)[:, None] * len(blob) + rel[None, :]).reshape(-1)[:n + 1].contiguous()
    rec.n = n
    rec.res_off_t = torch.zeros(n + 1, dtype=torch.int32, device=dev); rec.atom_off_t = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ro, ao = rec.sizes(codec)
    want_r = np.concatenate([[0], np.cumsum(np.tile(np.diff(o["res_off"].astype(np.int64)), tiles)[:n])])
    want_a = np.concatenate([[0], np.cumsum(np.tile(np.diff(o["atom_off"].astype(np.int64)), tiles)[:n])])
    assert np.array_equal(ro.astype(np.int64), want_r) and np.array_equal(ao.astype(np.int64), want_a)
    d = rec.batch(codec, host=False)
    per_a, per_r = int(o["atom_off"][-1]), int(o["res_off"][-1])
    whole = n // 3
    for k in ("x", "y", "z", "bfac_res", "atom_code", "res_code"):
        per = per_r if k in ("bfac_res", "res_code") else per_a
        as_int = (lambda t: t.view(torch.int32)) if o[k].dtype == np.float32 else (lambda t: t)
        ref = as_int(torch.from_numpy(o[k]).to(dev))
        got = as_int(d[k])
        assert bool((got[:whole * per].reshape(whole, per) == ref[None, :]).all()), k
        rest = got[whole * per:]                                 # the records of the last, partial tile
        assert len(rest) == int((o["res_off"] if k in ("bfac_res", "res_code") else o["atom_off"])[n - 3 * whole]) and torch.equal(rest, ref[:len(rest)]), k
    del rec, d
    torch.cuda.empty_cache()
