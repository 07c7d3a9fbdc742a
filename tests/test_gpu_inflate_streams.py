"""Inflate on the device against streams no zlib encoder writes (tests/_deflate.py: DEFLATE written from explicit tokens). zlib's
inflate() is the oracle and the comparison is on bytes:
  * every designed and every random member that is meant to be valid comes back with status 0 and the builder's text (which zlib's
    inflate() gives too: tests/test_deflate_streams_cpu.py), plain spacer entries come back untouched;
  * every stream zlib rejects is refused; what zlib reads and the device hands back is exactly the two classes fcz_hip.h documents;
  * mutants of the designed streams: the device inflates to zlib's bytes or refuses, never accepts what zlib rejects;
  * a member gives the same bytes and status twice in one call, alone and in a batch;
  * PDB text written with long codes, with a single distance code and in many tiny blocks -> the records of the plain text."""
import collections
import os
import struct

import numpy as np
import pytest

import _deflate as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBG = {0: "ok", 1: "header", 2: "block", 3: "code", 4: "size", 5: "input", 6: "check"}


def _why(st):
    st = int(st)
    return f"{DBG.get(st & 0xff, st & 0xff)}@{st >> 8}" if st >> 8 else DBG.get(st, str(st))


@pytest.fixture(scope="module")
def designed():
    return D.designed()


def _inflate(codec, entries):
    return codec.inflate([e.data for e in entries], [e.kind for e in entries])


def _check_batch(entries, texts, st):
    """the verdict on every entry of a batch -> the names of the members handed back although zlib reads them"""
    wrong, handed = [], []
    for e, got, s in zip(entries, texts, st):
        if e.expect == "reject":
            if s == 0 or got != b" " * len(e.text):
                wrong.append((e.name, "inflated a stream zlib rejects" if s == 0 else "a refused member's range is not blanks"))
        elif s != 0:
            if got != b" " * len(e.text):
                wrong.append((e.name, "a refused member's range is not blanks"))
            (handed if e.expect == "handback" else wrong).append(e.name if e.expect == "handback" else (e.name, "refused: " + _why(s)))
        elif got != e.text:
            k = next((i for i in range(min(len(got), len(e.text))) if got[i] != e.text[i]), min(len(got), len(e.text)))
            wrong.append((e.name, f"text differs at byte {k} of {len(e.text)} (got {len(got)})"))
    assert not wrong, f"{len(wrong)} of {len(entries)} entries: {wrong[:12]}"
    return handed


def test_designed_streams(codec, designed):
    """one call: status 0 and the builder's text for D1 .. D10, spacers untouched, D11 refused, D12 handed back with blanks -- and the
    neighbours of every refused member unharmed (they are among the entries checked)"""
    texts, st = _inflate(codec, designed)
    print({e.name: _why(s) for e, s in zip(designed, st) if s != 0})
    handed = _check_batch(designed, texts, st)
    assert sorted(handed) == sorted(e.name for e in designed if e.expect == "handback")
    assert sorted({n.split(",")[0].rstrip(" 0123456789") for n in handed}) == sorted(D.HANDBACK_CLASSES)
    assert sum(e.expect == "reject" for e in designed) >= 15 and sum(e.kind == 0 for e in designed) >= 20


@pytest.mark.parametrize("seed", (0, 1))
def test_random_streams(codec, seed):
    entries = D.stream_cases(seed)
    texts, st = _inflate(codec, entries)
    print({e.name: _why(s) for e, s in zip(entries, st) if s != 0})
    assert _check_batch(entries, texts, st) == [] and len(entries) == 40


def _mutants(designed):
    """about 600 mutants of the designed streams -> (name, base entry, bytes, first byte touched). The ISIZE bytes stay (they size
    the text buffer) but for the explicit + 1, - 1 and 0"""
    rng = np.random.default_rng(20261022)
    base = [e for e in designed if e.kind and e.expect != "reject" and len(e.data) < 1500]
    out = []
    for i in range(520):
        e = base[i % len(base)]
        b = bytearray(e.data)
        kind = i // len(base) % 4
        if kind < 2:                                    # one bit, two bits
            at = [int(rng.integers(10, len(b) - 4)) for _ in range(kind + 1)]
            for p in at:
                b[p] ^= 1 << int(rng.integers(0, 8))
        elif kind == 2:                                 # a byte replaced
            at = [int(rng.integers(10, len(b) - 4))]
            b[at[0]] = (b[at[0]] + int(rng.integers(1, 256))) & 255
        else:                                           # bytes cut
            at = [int(rng.integers(10, len(b) - 8))]
            del b[at[0]:min(len(b) - 8, at[0] + int(rng.integers(1, 5)))]
        out.append((f"{('one bit', 'two bits', 'byte', 'cut')[kind]}: {e.name}", e, bytes(b), min(at)))
    short = [e for e in designed if e.name in ("D7 empty dynamic", "D9 258 as 284 + 31")]
    assert len(short) == 2
    for e in short:
        out += [(f"truncated at {k}: {e.name}", e, e.data[:k], k) for k in range(1, len(e.data))]
    for e in base[::9]:
        for nm, v in (("+ 1", len(e.text) + 1), ("- 1", (len(e.text) - 1) & 0xffffffff), ("0", 0)):
            if v != len(e.text):
                out.append((f"isize {nm}: {e.name}", e, e.data[:-4] + struct.pack("<I", v), len(e.data) - 4))
    return out


def test_mutated_designed_streams_equal_zlib_or_are_refused(codec, designed):
    muts = _mutants(designed)
    assert 580 <= len(muts) <= 700, len(muts)
    want = [D.zlib_says(m) for _, _, m, _ in muts]
    texts, st = [None] * len(muts), np.zeros(len(muts), np.int32)
    for lo in range(0, len(muts), 64):
        tt, ss = codec.inflate([m for _, _, m, _ in muts[lo:lo + 64]])
        texts[lo:lo + 64] = tt
        st[lo:lo + 64] = ss
    n = collections.Counter()
    handed = []
    for (nm, e, m, at), w, got, s in zip(muts, want, texts, st):
        if s == 0:
            assert w is not None, f"{nm}: the device inflated a stream zlib rejects"
            assert got == w, f"{nm}: text differs from zlib's"
            n["inflated like zlib"] += 1
        elif w is None:
            n["refused like zlib"] += 1
        else:
            # zlib reads it, the device hands it back: only a mutant of one of D12's classes, or one whose gzip header was touched
            documented = e.expect == "handback" or at < e.hdr
            handed.append((nm, _why(s), documented))
    # the condition on the CPU side: what zlib still accepts of the list, and how much of that lies in the documented classes
    accepted = [(nm, e.expect == "handback" or at < e.hdr) for (nm, e, _, at), w in zip(muts, want) if w is not None]
    print(f"{len(muts)} mutants: {dict(n)}, {len(handed)} handed back {handed}; zlib accepts {len(accepted)}, {sum(d for _, d in accepted)} of them in the documented classes")
    assert all(d for _, _, d in handed), [h for h in handed if not h[2]]
    assert len(handed) <= sum(d for _, d in accepted)
    assert n["refused like zlib"] >= 300 and n["inflated like zlib"] >= 10


def test_twice_in_one_call_and_alone(codec, designed):
    pick = [e for e in designed if e.kind][::3]
    texts, st = _inflate(codec, pick + pick)
    k = len(pick)
    assert list(st[:k]) == list(st[k:]) and texts[:k] == texts[k:]
    both, stb = _inflate(codec, designed)
    at = {e.name: i for i, e in enumerate(designed)}
    for e, t, s in zip(pick, texts, st):
        assert (t, s) == (both[at[e.name]], stb[at[e.name]]), e.name
    for e in [e for e in pick if e.group in ("D2", "D3", "D6", "D11", "D12")][:16]:
        t, s = _inflate(codec, [e])
        assert (t[0], int(s[0])) == (both[at[e.name]], int(stb[at[e.name]])), e.name


def _greedy(text, only=None):
    """a trivial greedy LZ77 parse -> tokens; only: the distances it may use"""
    toks, last, i, n = [], {}, 0, len(text)
    while i < n:
        best, bd = 0, 0
        cands = [d for d in only if d <= i] if only else ([i - last[text[i:i + 3]]] if text[i:i + 3] in last else [])
        for d in cands:
            k = 0
            while k < 258 and i + k < n and text[i + k] == text[i + k - d]:
                k += 1
            if k > best and d <= 32768:
                best, bd = k, d
        step = best if best >= 3 else 1
        toks.append(D.match(best, bd) if best >= 3 else D.lit(text[i]))
        for j in range(i, i + step):
            last[text[j:j + 3]] = j
        i += step
    return toks


def _code_sets(rng, toks, llp, ddp):
    freq = collections.Counter(t[1] if t[0] == "lit" else D.EOB if t[0] == "eob" else D.length_symbol(t[1]) for t in toks)
    used = {D.dist_symbol(t[2]) for t in toks if t[0] == "match"}
    return D.random_ll(rng, freq, llp), D.random_dd(rng, used, ddp if used else "none")


def test_written_pdb_text_to_records(codec):
    """the first 20 KB of test_af.pdb, cut at the line end behind its last whole residue, parsed by a trivial greedy matcher and written (a) with long codes, (b) with a
    single one-bit distance code (the parse keeps to the distances of one symbol: a PDB line is 81 bytes), (c) in many tiny blocks"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "reference_ingest.npz"))
    text = z["file:test_af.pdb"].tobytes()[:20 << 10]
    text = text[:text.rindex(b"\n") + 1]
    lines = text.splitlines(keepends=True)
    while lines[-1][22:27] == text.splitlines()[-1][22:27]:                   # (the line end behind the last whole residue: a residue without CA and C has the reader leave the chain out)
        lines.pop()
    text = b"".join(lines)
    rng = np.random.default_rng(3)
    free, lines = _greedy(text), _greedy(text, only=[81] + [d for d in range(65, 97) if d != 81])
    assert {D.dist_symbol(t[2]) for t in lines if t[0] == "match"} == {12} and sum(t[0] == "match" for t in lines) > 200
    ll, dd = _code_sets(rng, free + [D.END], "long", "long")
    a = D.member("long codes", [D.Dynamic(ll, dd, free + [D.END])])
    ll, dd = _code_sets(rng, lines + [D.END], "fast", "single")
    b = D.member("single distance code", [D.Dynamic(ll, dd, lines + [D.END])])
    blocks = []
    for k in range(0, len(free), 23):
        part = free[k:k + 23] + [D.END]
        if k // 23 % 3 == 0:
            blocks.append(D.Fixed(part))
        else:
            ll, dd = _code_sets(rng, part, D.LL_PROFILES[k // 23 % 5], ("fast", "long")[k // 23 % 2])
            blocks.append(D.Dynamic(ll, dd, part))
        if k // 23 % 50 == 7:
            blocks.append(D.Stored(b"", 0xff))
    c = D.member("tiny blocks", blocks)
    assert len(blocks) > 100 and max(t.cl for t in a.layout[0][1]) > D.LBITS and {t.dl for t in b.layout[0][1] if t.kind == "len"} == {1}
    for m in (a, b, c):
        assert m.text == text and D.zlib_says(m.data) == text
    want = codec.compress_pdb([text], ["test_af.pdb"])
    assert int(want["counts"][0]) >= 1 and (want["file_status"] == 0).all()
    for m in (a, b, c):
        got = codec.compress_gz([m.data], ["test_af.pdb"], is_gz=[1])
        assert (got["file_status"] == want["file_status"]).all(), (m.name, got["file_status"])
        assert np.array_equal(got["off"], want["off"]) and got["blob"].tobytes() == want["blob"].tobytes(), m.name
        assert np.array_equal(got["chain_file"], want["chain_file"]) and np.array_equal(got["chain_meta"], want["chain_meta"]), m.name
