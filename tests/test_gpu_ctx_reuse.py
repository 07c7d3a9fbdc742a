"""GPU: what a ctx did before must not show in what it does next. A ctx keeps ~80 device buffers that only grow (stale contents
lie beyond the live range of a smaller batch), a single-use memo of the last sizes pass keyed on pointers, a second stream with a
fork / join event pair for long chains, and counters cleared by memsets in front of some launches. One seeded sequence of calls
of every kind on ONE ctx of the test's own, each result compared with the oracle (per-chain and stateless: it cannot share the
history) or, where the oracle has no such function, with the reference-minted golden the entry point's own test uses."""
import os
import zlib

import numpy as np
import pytest

import _angles as A
import _dense as D
import _harness as H
import _undense as U
from _analysis import bits
from _cases import entries_blob
from _devpath import DevRecords, compress_dev
from _window import same, sweep_starts, window_of
from foldcomp_amd import synthetic
from foldcomp_amd.structure import ChainBatch
from test_gpu_launch_plan import _backbone_dev_per_chain, _segments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
THREADS = 16


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _gen(lens, seed, thr=25, res_code=None, device="cpu"):
    return synthetic.to_chain_batch(synthetic.generate(len(lens), lens, seed=seed, anchor_threshold=thr, res_code=res_code, device=device))


def _no_title(f: bytes) -> bytes:
    na, tl = f[12], int.from_bytes(f[24:28], "little")
    return f[:24] + f[28:76 + 4 * na] + f[76 + 4 * na + tl:]


class _Calls:
    """the kinds of call the sequence draws from; every method runs one call on the ctx and holds its result to the yardstick"""

    def __init__(self, codec, golden):
        self.codec = codec
        self.z, self.index = golden
        large = np.random.default_rng(3).integers(16, 400, 3000)
        self.batches = {
            "large": _gen(large, 2001, device="cuda:0"),                                   # 600 000 residues: every scratch buffer grows
            "tiny": _gen([2, 3, 17], 2002),
            "small": _gen([30, 64, 65, 200], 2003),
            "long": _gen([1024, 1500, 40], 2004),                                          # the second stream
            "rich": _gen([700, 300, 64, 513, 2], 2005, res_code=17),                       # all TRP: the punt lists of both sides
            "deep": _gen([700, 33], 2006, thr=5000),                                       # one long segment: the ring / scratch column grow
        }
        self.oracle = {}
        for k, b in self.batches.items():
            blob, off, st = H.oracle_compress(b, n_threads=THREADS)
            assert (st == 0).all()
            self.oracle[k] = (blob, off, {alt: H.oracle_decompress(blob, off, alt_order=alt, n_threads=THREADS) for alt in (False, True)})
        # a batch in which every chain is refused (one residue; a NaN coordinate), and records none of which decodes
        b = _gen([1, 40, 1, 64], 2007)
        x = b.x.copy(); x[int(b.atom_off[int(b.res_off[1])]) + 4] = np.nan; x[int(b.atom_off[int(b.res_off[3])])] = np.inf
        self.refused = ChainBatch(**{**{f: getattr(b, f) for f in ("res_off", "atom_off", "y", "z", "atom_code", "res_code", "bfac_ca", "first_res_index",
                                                                  "first_atom_index", "chain_id", "titles", "title_off", "anchor_threshold")}, "x": x})
        good = self.z["pdb:test_af/fcz"].tobytes()
        self.unreadable = [b"XXXX" + good[4:], good[:90], good[:40]]
        self.gold_names = [n for n in self.index if f"{n}/pdb0" in self.z.files and f"{n}/fcz" in self.z.files][:12]
        self.gold = [self.z[f"{n}/fcz"].tobytes() for n in self.gold_names]
        self.fast = False
        self.gold_flat = H.oracle_decompress(*entries_blob(self.gold))              # the atoms the dense tensors are filled from
        self.dense_want, self.undense_want = {}, {}

    # -- codec calls against the oracle
    def compress(self, key, dev=False):
        b = self.batches[key]
        blob, off, st = compress_dev(self.codec, b) if dev else self.codec.compress_batch(b)
        oblob, ooff, _ = self.oracle[key]
        assert (st == 0).all() and np.array_equal(off, ooff) and blob.tobytes() == oblob.tobytes()

    def decompress(self, key, alt=False, dev=False):
        oblob, ooff, o = self.oracle[key]
        d = DevRecords(oblob, ooff).decompress(self.codec, alt) if dev else self.codec.decompress_batch(oblob, ooff, alt_order=alt)
        o = o[alt]
        assert np.array_equal(d["res_off"], o["res_off"]) and np.array_equal(d["atom_off"], o["atom_off"])
        assert np.array_equal(d["atom_code"], o["atom_code"]) and np.array_equal(d["res_code"], o["res_code"])
        assert np.array_equal(_bits(d["bfac_res"]), _bits(o["bfac_res"]))
        if not dev:
            assert all(d["info"][i].status == 0 for i in range(len(ooff) - 1))
        if not self.fast:
            for k in ("x", "y", "z"):
                assert np.array_equal(_bits(d[k]), _bits(o[k])), k
        else:
            # the bars of test_gpu_fast_numerics.py: finite; backbone per chain under 2e-3 * max(1, seg / 32) ** 1.5 (default atom order: N, CA, C
            # lead every residue); over a large batch of -b 25 chains median < 1e-4 A and 99.9 % of atoms < 2e-3 A
            assert all(np.isfinite(d[k]).all() for k in ("x", "y", "z"))
            dev_ = np.max(np.abs(np.stack([d[k].astype(np.float64) - o[k] for k in ("x", "y", "z")])), axis=0)
            if not alt:
                per_chain, _ = _backbone_dev_per_chain(o, d)
                seg = np.asarray([_segments(oblob[int(ooff[i]):int(ooff[i + 1])].tobytes())[0] - 1 for i in range(len(ooff) - 1)], np.float64)
                assert (per_chain < 2e-3 * np.maximum(1.0, seg / 32.0) ** 1.5).all(), (key, float(per_chain.max()))
            if key == "large":
                assert float(np.median(dev_)) < 1e-4 and float(np.quantile(dev_, 0.999)) < 2e-3, (float(np.median(dev_)), float(np.quantile(dev_, 0.999)))

    def numerics(self, fast):
        self.codec.set_numerics(fast); self.fast = fast

    def empty(self):
        b = self.batches["tiny"]
        none = ChainBatch(res_off=np.zeros(1, np.uint32), atom_off=np.zeros(1, np.uint32), x=np.zeros(0, np.float32), y=np.zeros(0, np.float32),
                          z=np.zeros(0, np.float32), atom_code=np.zeros(0, np.uint8), res_code=np.zeros(0, np.uint8), bfac_ca=np.zeros(0, np.float32),
                          first_res_index=np.zeros(0, np.int32), first_atom_index=np.zeros(0, np.int32), chain_id=np.zeros(0, np.uint8),
                          titles=np.zeros(0, np.uint8), title_off=np.zeros(1, np.uint32), anchor_threshold=b.anchor_threshold)
        blob, off, st = compress_dev(self.codec, none)             # (the host entry points return before they reach the ctx)
        assert len(blob) == 0 and list(off) == [0] and len(st) == 0
        d = DevRecords(np.zeros(0, np.uint8), np.zeros(1, np.uint64)).decompress(self.codec)
        assert len(d["x"]) == 0 and list(d["res_off"]) == [0] and list(d["atom_off"]) == [0]

    def all_refused(self):
        blob, off, st = self.codec.compress_batch(self.refused, strict=False)
        oblob, ooff, ost = H.oracle_compress(self.refused, n_threads=1)
        assert list(st) == [-7, -9, -7, -9] and list(ost[[0, 2]]) == [-7, -7]       # FCZ_E_TOO_SHORT (the oracle's too), FCZ_E_NONFINITE
        assert np.array_equal(off, ooff) and not blob.any()
        blob, off = entries_blob(self.unreadable)
        d = self.codec.decompress_batch(blob, off)
        o = H.oracle_decompress(blob, off)
        assert [d["info"][i].status for i in range(3)] == [o["info"][i].status for i in range(3)] and all(o["info"][i].status != 0 for i in range(3))
        assert len(d["x"]) == 0 and not d["res_off"].any() and not d["atom_off"].any()
        d = DevRecords(blob, off).decompress(self.codec)                              # R == 0 through the device entry points: sizes, then batch
        assert not d["res_off"].any() and not d["atom_off"].any() and len(d["x"]) == 0

    def encode_dense(self, key, layout):
        """dense tensors in where other entry points stage records; leaves resident records for its fetch"""
        b = self.batches[key]
        L = int(np.diff(b.res_off.astype(np.int64)).max())
        titles = [bytes(b.titles[int(b.title_off[c]):int(b.title_off[c + 1])]).decode("latin-1") for c in range(b.n_chains)]
        d = U.dense_from_batch(b, layout, L)
        if (key, layout) not in self.undense_want:
            eb, refusal = U.batch_expected(d["pos"], d["mask"], d["aatype"], d["length"], layout, plddt=d["plddt"],
                                           first_res_index=d["first_res_index"], chain_id=b.chain_id, titles=titles,
                                           anchor_threshold=int(b.anchor_threshold))
            blob, off, ost = H.oracle_compress(eb, n_threads=1)
            st = U.expected_status(refusal, ost)
            # the expectation comes from the builder + oracle for every layout. Where the tensors hold every atom the records must also be
            # the batch's own; that holds for atom37 only: all_atoms_have_slots lets a chain's closing OXT pass in any layout, but
            # atom14 has no slot for it, so its tensors drop the atom and the records differ from the batch's own
            if layout == "atom37" and U.all_atoms_have_slots(b, layout):
                assert np.array_equal(off, self.oracle[key][1]) and blob.tobytes() == self.oracle[key][0].tobytes()
            self.undense_want[key, layout] = (blob, off, st)
        wblob, woff, wst = self.undense_want[key, layout]
        blob, off, st = self.codec.compress_dense(d["pos"], d["mask"], d["aatype"], d["length"], d["plddt"], layout=layout,
                                                  first_res_index=d["first_res_index"], chain_id=b.chain_id, titles=titles,
                                                  anchor_threshold=int(b.anchor_threshold))
        assert not wst.any() and np.array_equal(st, wst) and np.array_equal(off, woff) and blob.tobytes() == wblob.tobytes()

    # -- the other entry points against the reference's goldens
    def decode_dense(self, layout, crop=False):
        """the golden records as dense tensors; cropped: one row less than the longest entry has (other staging sizes)"""
        fields = [D.record_fields(f) for f in self.gold]
        L = max(len(seq) for seq, _, _ in fields) - (1 if crop else 0)
        if (layout, L) not in self.dense_want:
            o, per = self.gold_flat, []
            for i, (seq, first, has_oxt) in enumerate(fields):
                a0, a1, r0 = int(o["atom_off"][i]), int(o["atom_off"][i + 1]), int(o["res_off"][i])
                xyz = np.stack([o["x"][a0:a1], o["y"][a0:a1], o["z"][a0:a1]], 1)
                per.append(D.dense_expected(xyz, seq, first, has_oxt, layout, L, plddt=o["bfac_res"][r0:r0 + len(seq)]))
            self.dense_want[layout, L] = D.stack_expected(per, L, D.WIDTH[layout])
        want = self.dense_want[layout, L]
        got = self.codec.decompress_dense(*entries_blob(self.gold), layout=layout, max_len=L if crop else None)
        assert not got["status"].any() and got["pos"].shape == (len(self.gold), L, D.WIDTH[layout], 3)
        for k in ("pos", "plddt"):
            assert np.array_equal(bits(got[k]), bits(want[k])), (layout, L, k)
        for k in ("mask", "aatype", "res_index", "length"):
            assert np.array_equal(got[k].astype(np.int64), want[k].astype(np.int64)), (layout, L, k)

    def _gold_full(self, layout):
        """(residues per golden record, the uncropped expectation a decode_dense step left)"""
        lens = np.asarray([len(D.record_fields(f)[0]) for f in self.gold], np.int64)
        return lens, self.dense_want[layout, int(lens.max())]

    def decode_dense_form(self, form, layout="atom37"):
        """the host forms beside fcz_decompress_dense: a window of 64 rows per entry, or the rows without padding"""
        lens, full = self._gold_full(layout)
        if form == "window":
            starts = sweep_starts(lens, 64, 3)
            got = self.codec.decompress_dense(*entries_blob(self.gold), layout=layout, max_len=64, start=starts)
            want = window_of(full, starts, 64)
        else:
            got = self.codec.decompress_dense(*entries_blob(self.gold), layout=layout, packed=True)
            want = {k: np.concatenate([full[k][e, :n] for e, n in enumerate(lens)]) for k in ("pos", "mask", "aatype", "plddt", "res_index")}
            want["length"] = full["length"]
            assert np.array_equal(got["row_off"], np.concatenate([[0], np.cumsum(lens)])) and np.array_equal(got["chain_index"], np.repeat(np.arange(len(lens)), lens))
        assert not got["status"].any()
        same(got, want, f"dense {form}")

    def decode_angles(self, form):
        """the three angle host forms against the numpy restatement tests/test_gpu_angles.py uses"""
        exp = [A.entry_expected(f) for f in self.gold]
        lens, full = self._gold_full("atom37")
        Lf = int(lens.max())
        blob, off = entries_blob(self.gold)
        if form == "packed":
            got = self.codec.decompress_angles(blob, off, packed=True)
            e_ang, e_msk, e_off = A.packed_expected(exp)
            assert np.array_equal(got["row_off"], e_off)
        elif form == "padded":
            got = self.codec.decompress_angles(blob, off)
            e_ang, e_msk = A.padded_expected(exp, Lf)
        else:
            starts = sweep_starts(lens, 64, 5)
            got = self.codec.decompress_angles(blob, off, L=64, start=starts)
            f_ang, f_msk = A.padded_expected(exp, Lf)
            e_ang, e_msk = np.zeros((len(lens), 64, A.COLS), np.float32), np.zeros((len(lens), 64, A.COLS), np.uint8)
            for e, s in enumerate(int(x) for x in starts):
                m = max(min(64, Lf - s), 0)
                e_ang[e, :m] = f_ang[e, s:s + m]; e_msk[e, :m] = f_msk[e, s:s + m]
            assert np.array_equal(got["aatype"], window_of(full, starts, 64)["aatype"])
        assert not got["status"].any() and got["angles"].shape == e_ang.shape
        assert np.array_equal(got["angle_mask"].view(np.uint8), e_msk) and np.array_equal(_bits(got["angles"]), _bits(e_ang)), form

    def pdb_text(self, alt=False):
        blob, off = entries_blob(self.gold)
        texts, status = self.codec.decompress_pdb(blob, off)
        assert (status == 0).all()
        for n, t in zip(self.gold_names, texts):
            assert t == self.z[f"{n}/pdb0"].tobytes(), n

    def extract(self, digits):
        names = [n for n in self.gold_names if f"{n}/plddt{digits}" in self.z.files]
        assert names
        blob, off = entries_blob([self.z[f"{n}/fcz"].tobytes() for n in names])
        for n, got in zip(names, self.codec.extract(blob, off, mode=0, digits=digits)):
            assert got == self.z[f"{n}/plddt{digits}"].tobytes(), (n, digits)

    def inflate(self):
        texts = [self.z[f"{n}/pdb0"].tobytes() for n in self.gold_names[:3]] + [b"", b"x" * 70000]
        members = []
        for t, lvl in zip(texts, (6, 1, 9, 6, 6)):
            c = zlib.compressobj(lvl, zlib.DEFLATED, 31)
            members.append(c.compress(t) + c.flush())
        got, st = self.codec.inflate(members)
        assert (st == 0).all() and got == [zlib.decompress(m, 31) for m in members] and got == texts

    def _texts(self):
        from test_host_cpp import _pdb_text
        cases = ["pdb:test_af", "pdb:test", "syn:len350", "syn:len26", "syn:len129"]
        return cases, [_pdb_text(self.z, n).encode() for n in cases], [f"f{i}.pdb" for i in range(len(cases))]

    def compress_pdb(self):
        cases, texts, names = self._texts()
        r = self.codec.compress_pdb(texts, names)
        assert (r["status"] == 0).all() and (r["file_status"] == 0).all() and len(r["refused"]) == 0
        for i, n in enumerate(cases):
            rec = r["blob"][int(r["off"][i]):int(r["off"][i + 1])].tobytes()
            assert _no_title(rec) == _no_title(self.z[f"{n}/fcz"].tobytes()), n

    def compress_gz(self):
        """three gzip members and two plain texts: the inflate stage writes the text the ingest reads"""
        cases, texts, names = self._texts()
        files, is_gz = [], [1, 0, 1, 1, 0]
        for t, gz, lvl in zip(texts, is_gz, (6, 6, 1, 9, 6)):
            c = zlib.compressobj(lvl, zlib.DEFLATED, 31)
            files.append(c.compress(t) + c.flush() if gz else t)
        r = self.codec.compress_gz(files, names, is_gz=is_gz)
        assert (r["status"] == 0).all() and (r["file_status"] == 0).all() and len(r["refused"]) == 0
        for i, n in enumerate(cases):
            rec = r["blob"][int(r["off"][i]):int(r["off"][i + 1])].tobytes()
            assert _no_title(rec) == _no_title(self.z[f"{n}/fcz"].tobytes()), n

    def ingest_pdb(self):
        cases, texts, names = self._texts()
        b, cfile, cmeta, fstat, refused = self.codec.ingest_pdb(texts, names)
        assert (fstat == 0).all() and len(refused) == 0 and list(cfile) == list(range(len(cases)))
        blob, off, st = H.oracle_compress(b, n_threads=1)                              # the parsed batch -> the reference's records
        assert (st == 0).all()
        for i, n in enumerate(cases):
            assert _no_title(blob[int(off[i]):int(off[i + 1])].tobytes()) == _no_title(self.z[f"{n}/fcz"].tobytes()), n


def _sequence(seed):
    """fixed opening (the orders the issue names), then seeded draws, then the dense and gzip entry points, each beside a call that
    uses the same staging buffers differently: 40 .. 70 calls"""
    seq = [("compress", "large"), ("decompress", "large"), ("decompress", "tiny"), ("compress", "tiny"), ("decompress", "large", True),
           ("decompress", "long"), ("decompress", "small"), ("decompress", "long", True), ("compress", "rich"), ("compress", "small"),
           ("decompress", "rich"), ("decompress", "small", True), ("numerics", True), ("decompress", "large"), ("decompress", "tiny"),
           ("numerics", False), ("decompress", "tiny"), ("empty",), ("decompress", "small"), ("all_refused",), ("decompress", "small", True),
           ("pdb_text",), ("decompress", "long", False, True), ("extract", 2), ("compress", "small", True), ("inflate",), ("decompress", "rich", True, True),
           ("compress_pdb",), ("decompress", "tiny", False, True), ("ingest_pdb",), ("compress", "large", True), ("decompress", "deep"), ("decompress", "small")]
    rng = np.random.default_rng(seed)
    keys = ["large", "tiny", "small", "long", "rich", "deep"]
    fast = False
    for _ in range(20):
        kind = int(rng.integers(0, 10))
        key = keys[int(rng.integers(0, len(keys)))]
        if kind < 4:
            # (fast numerics is held to the quantile rule, which the existing suite states for segments of -b 25 only)
            seq.append(("decompress", "small" if fast and key == "deep" else key, bool(rng.integers(0, 2)), bool(rng.integers(0, 2))))
        elif kind < 6:
            seq.append(("compress", key, bool(rng.integers(0, 2))))
        elif kind == 6:
            fast = not fast; seq.append(("numerics", fast))
        else:
            seq.append([("empty",), ("all_refused",), ("pdb_text",), ("extract", int(rng.integers(1, 5))), ("inflate",), ("compress_pdb",)][int(rng.integers(0, 6))])
    # (not among the draws: the history above stays what it was)
    seq += [("encode_dense", "small", "atom37"), ("decompress", "tiny"), ("decode_dense", "atom37"), ("pdb_text",), ("compress_gz",),
            ("encode_dense", "small", "atom14"), ("decode_dense", "atom14"), ("decode_dense", "atom37", True)]
    # the host forms of the decode the history above lacks, alternating dense and angles (they share ANGLES_OUT / DENSE_OUT and WINDOW_START)
    seq += [("decode_dense_form", "packed"), ("decode_angles", "padded"), ("decode_dense_form", "window"), ("decode_angles", "packed"), ("decode_angles", "window")]
    seq += [("numerics", False), ("decompress", "large", True), ("decompress", "tiny")]
    return seq


def test_results_do_not_depend_on_what_the_ctx_did_before(golden):
    import torch
    torch.cuda.init()
    from foldcomp_amd.codec import Codec
    seq = _sequence(20261016)
    assert 40 <= len(seq) <= 70
    codec = Codec(0)
    try:
        calls = _Calls(codec, golden)
        for i, (name, *args) in enumerate(seq):
            try:
                getattr(calls, name)(*args)
            except Exception as e:
                done = "\n".join(f"{j:3d} {c}" for j, c in enumerate(seq[:i + 1]))
                raise AssertionError(f"call {i} {(name, *args)} failed after this history:\n{done}\n{type(e).__name__}: {e}") from e
    finally:
        codec.close()


@pytest.mark.parametrize("key_lens", [("long", [1024, 1500, 40, 2, 700]), ("short", [350, 2, 64, 65, 129, 16])])
def test_sizes_call_then_batch_call_on_unchanged_records(key_lens):
    """the sequence the sizes memo exists for (include/fcz_hip.h, fcz_decompress_sizes_dev): sizes call, then the batch call on the same
    unchanged records at the same addresses -- the batch call reuses the totals, the length order and the residue codes the sizes call
    left. Its result == a cold batch call on another ctx == the oracle, for a batch with long chains and for one without."""
    import torch
    torch.cuda.init()
    from foldcomp_amd.codec import Codec
    key, lens = key_lens
    blob, off, st = H.oracle_compress(_gen(lens, 2100 + len(lens)), n_threads=4)
    assert (st == 0).all()
    warm, cold = Codec(0), Codec(0)
    try:
        for alt in (False, True):
            o = H.oracle_decompress(blob, off, alt_order=alt, n_threads=4)
            rec = DevRecords(blob, off)
            ro, ao = rec.sizes(warm)                               # remembered ...
            assert np.array_equal(ro, o["res_off"]) and np.array_equal(ao, o["atom_off"])
            d_warm = rec.batch(warm, alt)                          # ... and used: no second sizes pass
            d_cold = cold.decompress_batch(blob, off, alt_order=alt)          # host entry point: always its own sizes pass
            for d in (d_warm, d_cold):
                for k in ("x", "y", "z", "bfac_res"):
                    assert np.array_equal(_bits(d[k]), _bits(o[k])), (key, alt, k)
                assert np.array_equal(d["atom_code"], o["atom_code"]) and np.array_equal(d["res_code"], o["res_code"])
            # the memo is single use: a second batch call on the same pointers runs its own sizes pass and gives the same
            d_again = rec.batch(warm, alt)
            for k in ("x", "y", "z", "bfac_res"):
                assert np.array_equal(_bits(d_again[k]), _bits(o[k])), (key, alt, k, "second batch call")
    finally:
        warm.close(); cold.close()
