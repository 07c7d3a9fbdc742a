"""DEFLATE streams (RFC 1951) written from explicit tokens, for k_inflate (foldcomp_amd/csrc/fcz_inflate.h): the dialect zlib's encoder
never writes. Every stream the other inflate tests hold comes out of zlib's deflate(); the ones here are written bit by bit from a list
of blocks, with the text built alongside (a match copies from the text so far), so a case carries its intended text and no LZ search is
needed. zlib's inflate() stays the oracle of what is valid: tests/test_deflate_streams_cpu.py holds every member here against it.

  deflate(blocks)      stored / fixed / dynamic blocks -> bytes, text, layout (every token's bit position and code lengths)
  gz_wrap              RFC 1952 framing with FEXTRA / FNAME / FCOMMENT of chosen lengths
  stream_cases(seed)   a seeded random family: entries (members and plain spacers) of random code sets and token mixtures
  designed()           named cases, each the smallest that reaches its place in the kernel (D1 .. D12 below)
  mirror               a replay of decode_body's turns from the layout: which path every window takes. It claims nothing about the device's
                       results, only about the place a stream reaches; its constants are parsed out of fcz_inflate.h."""
import collections
import os
import re
import struct
import zlib

import numpy as np

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32
EOB = 256


def kernel_constants():
    """the constants the designed cases are aimed by, read out of fcz_inflate.h as text"""
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "foldcomp_amd", "csrc", "fcz_inflate.h")).read()

    def one(pattern):
        m = re.search(pattern, text)
        assert m, pattern
        return int(m.group(1))
    c = dict(RING_BITS=one(r"#define FCZ_INFLATE_RING_BITS (\d+)"), LBITS=one(r"#define FCZ_INFLATE_LBITS (\d+)"), DBITS=one(r"LBITS = FCZ_INFLATE_LBITS, DBITS = (\d+);"),
             WIN_OUT=one(r"constexpr uint32_t WIN_OUT = (\d+);"), ROUND=one(r"ROUND = (\d+);"), IN_BLOCK=one(r"fetched (\d+) at a time, one dword per lane"))
    assert "constexpr uint32_t REACH = RING - WIN_OUT;" in text and "RING = 1u << FCZ_INFLATE_RING_BITS" in text
    assert "if (__builtin_expect(tot <= 64u &&" in text and "dist >= ex + len &&" in text                 # the choice between the two text paths
    return c


K = kernel_constants()
RING, LBITS, DBITS, WIN_OUT, ROUND, IN_BLOCK = 1 << K["RING_BITS"], K["LBITS"], K["DBITS"], K["WIN_OUT"], K["ROUND"], K["IN_BLOCK"]
REACH = RING - WIN_OUT


# ---- tokens and blocks ---------------------------------------------------------------------------------------------------------------------
def lit(b):
    return ("lit", b)


def match(length, dist, sym=None):
    """a match; sym: the length symbol to code it through (258 as 284 + extra 31)"""
    return ("match", length, dist, sym)


def raw(value, nbits):
    """nbits written as they stand, first bit = bit 0 of value (the rejection cases: a code pattern no symbol has)"""
    return ("raw", value, nbits)


END = ("eob",)
Stored = collections.namedtuple("Stored", "data junk", defaults=(0,))
Fixed = collections.namedtuple("Fixed", "tokens")
# ll / dd: code lengths of the literal/length and the distance alphabet (lists, HLIT / HDIST = their lengths); runs: how the header codes them
# ("greedy" 16 / 17 / 18 runs over the two lists as one, "plain" none, or the (symbol, extra) list itself); hclen: HCLEN (None: the fewest);
# cl: the code-length code's 19 lengths (None: a complete one over the symbols the header uses)
Dynamic = collections.namedtuple("Dynamic", "ll dd tokens runs hclen cl", defaults=("greedy", None, None))
Tok = collections.namedtuple("Tok", "bit nb kind outn dist cl dl")        # kind: lit / len / eob; cl, dl: length of the literal/length and of the distance code


class BitWriter:
    """bits into a list of bytes, first bit of the stream = bit 0 of byte 0 (the accumulator never holds more than a token)"""

    def __init__(self):
        self.buf, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, n):
        assert 0 <= v < (1 << n) or n == 0
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.buf.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c):
        """a Huffman code (value, length): top bit first"""
        self.put(int(format(c[0], "0%db" % c[1])[::-1], 2), c[1])

    def pos(self):
        return len(self.buf) * 8 + self.n

    def align(self, junk=0):
        pad = -self.n % 8
        self.put(junk & ((1 << pad) - 1), pad)

    def data(self, b):
        assert self.n == 0
        self.buf += b


def canon(lens):
    """code lengths -> {symbol: (code, length)}: the canonical code of RFC 1951 section 3.2.2 (a set that is not complete still gets its codes)"""
    count = collections.Counter(l for l in lens if l)
    code, nxt = 0, {}
    for l in range(1, 16):
        code = (code + count.get(l - 1, 0)) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def kraft(lens):
    """sum of 2^(15 - l): 32768 for a complete set"""
    return sum(1 << (15 - l) for l in lens if l)


def length_symbol(n):
    return 285 if n == 258 else max(i for i in range(28) if LBASE[i] <= n) + 257


def dist_symbol(d):
    return max(i for i in range(30) if DBASE[i] <= d)


def header_symbols(seq, hlit, runs):
    """the code-length symbols (symbol, extra) that code seq, and the kinds of run that cross from the literal/length lengths into the distance lengths"""
    out, crossed, i, n = [], set(), 0, len(seq)
    if runs == "plain":
        return [(v, 0) for v in seq], crossed
    while i < n:
        v, run = seq[i], 1
        while i + run < n and seq[i + run] == v:
            run += 1
        if v == 0 and run >= 3:
            r = min(run, 138)
            out.append((17, r - 3) if r <= 10 else (18, r - 11))
            crossed |= {out[-1][0]} if i < hlit < i + r else set()
            i += r
        elif v and run >= 4:
            r = min(run - 1, 6)
            out += [(v, 0), (16, r - 3)]
            crossed |= {16} if i + 1 <= hlit < i + 1 + r else set()
            i += 1 + r
        else:
            out.append((v, 0))
            i += 1
    return out, crossed


def balanced(symbols, nsym):
    """a complete code over `symbols` (two at least): lengths k - 1 and k"""
    symbols = sorted(symbols)
    n = len(symbols)
    k = (n - 1).bit_length()
    short = (1 << k) - n
    lens = [0] * nsym
    for j, s in enumerate(symbols):
        lens[s] = k - 1 if j < short else k
    return lens


def deflate(blocks, strict=True, tail_junk=0):
    """blocks -> (bytes of the DEFLATE stream, text, layout, info). layout: per block ("S", bytes) or ("H", [Tok]); info: per dynamic
    block the header's bit span and the run kinds that cross. strict: every match lies inside the text so far and every symbol has a code"""
    w, text, layout, info = BitWriter(), bytearray(), [], []
    for bi, b in enumerate(blocks):
        w.put(1 if bi == len(blocks) - 1 else 0, 1)
        if isinstance(b, Stored):
            w.put(0, 2)
            w.align(b.junk)
            w.put(len(b.data), 16)
            w.put(len(b.data) ^ 0xffff, 16)
            w.data(b.data)
            text += b.data
            layout.append(("S", len(b.data)))
            continue
        if isinstance(b, Fixed):
            w.put(1, 2)
            ll, dd = canon(FIXED_LL), canon(FIXED_D)
        else:
            w.put(2, 2)
            h0 = w.pos()
            hlit, hdist = len(b.ll), len(b.dd)
            assert 257 <= hlit <= 288 and 1 <= hdist <= 32
            syms, crossed = (list(b.runs), set()) if isinstance(b.runs, list) else header_symbols(list(b.ll) + list(b.dd), hlit, b.runs)
            used = {s for s, _ in syms}
            if b.cl is not None:
                cl = list(b.cl)
            else:
                for s in (0, 8):                                              # (two symbols at least: zlib rejects a code-length code of one)
                    used |= {s} if len(used) < 2 else set()
                cl = balanced(used, 19)
            hclen = b.hclen or max(4, max(i for i in range(19) if cl[ORDER[i]]) + 1)
            w.put(hlit - 257, 5)
            w.put(hdist - 1, 5)
            w.put(hclen - 4, 4)
            for i in range(hclen):
                w.put(cl[ORDER[i]], 3)
            cc = canon(cl)
            for s, x in syms:
                w.code(cc[s])
                if s >= 16:
                    w.put(x, (2, 3, 7)[s - 16])
            info.append(dict(block=bi, bits=(h0 - 3, w.pos()), crossed=crossed, hclen=hclen, cl=cl))
            ll, dd = canon(b.ll), canon(b.dd)
        toks = []
        for t in b.tokens:
            p = w.pos()
            if t[0] == "lit":
                w.code(ll[t[1]])
                text.append(t[1])
                toks.append(Tok(p, w.pos() - p, "lit", 1, 0, ll[t[1]][1], 0))
            elif t[0] == "eob":
                w.code(ll[EOB])
                toks.append(Tok(p, w.pos() - p, "eob", 0, 0, ll[EOB][1], 0))
            elif t[0] == "raw":
                w.put(t[1], t[2])
            else:
                _, n, d, sym = t
                sym = sym or length_symbol(n)
                assert 0 <= n - LBASE[sym - 257] < (1 << LEXT[sym - 257]) or n == LBASE[sym - 257]
                w.code(ll[sym])
                w.put(n - LBASE[sym - 257], LEXT[sym - 257])
                ds = dist_symbol(d)
                w.code(dd[ds])
                w.put(d - DBASE[ds], DEXT[ds])
                if d > len(text):
                    assert not strict, "a match that begins before the text"
                    text += bytes(n)
                elif d >= n:
                    text += text[len(text) - d:len(text) - d + n]
                else:
                    unit = bytes(text[-d:])
                    text += (unit * (n // d + 1))[:n]
                toks.append(Tok(p, w.pos() - p, "len", n, d, ll[sym][1], dd[ds][1]))
        layout.append(("H", toks))
    w.align(tail_junk)
    return bytes(w.buf), bytes(text), layout, info


def gz_wrap(body, text, fextra=None, fname=None, fcomment=None, crc=None, isize=None):
    """RFC 1952 framing; fextra / fname / fcomment: lengths of FEXTRA's field, of FNAME and of FCOMMENT without their terminators (None: absent)"""
    flg = (4 if fextra is not None else 0) | (8 if fname is not None else 0) | (16 if fcomment is not None else 0)
    h = bytes([0x1f, 0x8b, 8, flg, 0, 0, 0, 0, 0, 3])
    if fextra is not None:
        h += struct.pack("<H", fextra) + bytes((7 * k + 1) & 255 for k in range(fextra))
    if fname is not None:
        h += b"n" * fname + b"\0"
    if fcomment is not None:
        h += b"c" * fcomment + b"\0"
    return h + body + struct.pack("<II", zlib.crc32(text) if crc is None else crc, (len(text) if isize is None else isize) & 0xffffffff), len(h)


# expect: "ok" the device must inflate it, "reject" zlib rejects it, "handback" zlib reads it and the device may refuse it (D12)
Entry = collections.namedtuple("Entry", "name kind data text expect group layout hdr info", defaults=("ok", "", None, 0, None))


def member(name, blocks, group="", expect="ok", strict=True, tail_junk=0, **gz):
    body, text, layout, info = deflate(blocks, strict, tail_junk)
    data, hdr = gz_wrap(body, text, **gz)
    return Entry(name, 1, data, text, expect, group, layout, hdr, info)


def spacer(n, salt=0):
    data = bytes((salt + 31 * k) % 251 for k in range(n))
    return Entry(f"spacer {n}", 0, data, data, "ok", "spacer")


def place(entries):
    """(mis, omis) of every entry of a batch: the input's misalignment to 4 bytes and the text's to ROUND (device buffers are aligned to both)"""
    out, i, t = [], 0, 0
    for e in entries:
        out.append((i & 3, t & (ROUND - 1)))
        i += len(e.data)
        t += len(e.text)
    return out


# ---- the mirror of decode_body's turns ------------------------------------------------------------------------------------------------------
def copy_branch(n, d):
    """lz_copy's branch inside the ring"""
    return "lanes" if n <= 64 and d >= n else "chunks" if d >= 64 else "overlap"


def mirror(entry, omis=0):
    """the turns of every Huffman block of a member -> list of dicts: q (text position, counted from the ROUND edge below the member's
    start), ntok, tot, path (fast / slow), cut (what ended the chain: horizon, win_out, sp-lit, sp-len, sp-dist, eob), far (far matches of
    the window), farsp (the uniform symbol's copy read HBM), done (what completed a pending far store: window, flush, long, eob),
    flush (a round left after the turn), copies (lz_copy branches), edge (ex + outn of the symbol the WIN_OUT cut stopped at)"""
    q, flushed, turns = omis, 0, []
    for bi, (kind, body) in enumerate(entry.layout):
        if kind == "S":
            stored_flush = 0
            for j in range(0, body, 64):
                q0 = q
                q = q0 + min(64, body - j)
                if q - flushed >= ROUND:
                    flushed += ROUND
                    stored_flush += 1
            turns.append(dict(block=bi, q=q, path="stored", cut="stored", flush=stored_flush, ntok=0, tot=body, far=0, farsp=False, done=None, copies=[], edge=None, sp=None, on=[], first=None, last=None, ex_last=0))
            continue
        toks, i, pend = body, 0, False
        while i < len(toks):
            t0, on, sp = toks[i].bit, [], None
            while i + len(on) < len(toks) and toks[i + len(on)].bit - t0 < 64:      # the chain: symbols that START within 64 bits
                t = toks[i + len(on)]
                if t.cl > LBITS or t.kind == "eob" or (t.kind == "len" and t.dl > DBITS):
                    sp = t
                    break
                on.append(t)
            ex = [sum(t.outn for t in on[:k]) for k in range(len(on) + 1)]
            tot, cut, edge = ex[-1], "horizon", None
            if tot > WIN_OUT:
                k = next(k for k in range(1, len(on)) if ex[k] + on[k].outn > WIN_OUT)
                edge, on, sp, tot, cut = ex[k] + on[k].outn, on[:k], None, ex[k], "win_out"
            done = "window" if pend else None
            pend = False
            fast = tot <= 64 and all(t.kind == "lit" or t.dist >= e + t.outn for t, e in zip(on, ex))
            far = sum(t.kind == "len" and t.dist > REACH for t in on)
            copies = [] if fast else [copy_branch(t.outn, t.dist) if t.dist <= REACH else "hbm" for t in on if t.kind == "len"]
            pend = fast and far > 0
            i += len(on)
            q += tot
            farsp = False
            if sp is not None:
                if pend:
                    done, pend = ("eob" if sp.kind == "eob" else "long"), False
                cut = "eob" if sp.kind == "eob" else "sp-lit" if sp.kind == "lit" else "sp-len" if sp.cl > LBITS else "sp-dist"
                if sp.kind == "len":
                    farsp = sp.dist > REACH
                    copies.append("hbm" if farsp else copy_branch(sp.outn, sp.dist))
                q += sp.outn
                i += 1
            flush = q - flushed >= ROUND
            if flush:
                if pend:
                    done, pend = "flush", False
                flushed += ROUND
            turns.append(dict(block=bi, q=q, ntok=len(on), tot=tot, path="fast" if fast else "slow", cut=cut, far=far, farsp=farsp, done=done,
                              flush=int(flush), copies=copies, edge=edge, sp=sp, on=on, first=on[0] if on else sp, last=on[-1] if on else None, ex_last=ex[len(on) - 1] if on else 0))
            assert not (pend and cut == "eob")
    return turns


def tally(turns):
    """what a list of turns reaches, as a Counter of names"""
    c = collections.Counter()
    for t in turns:
        c[t["path"]] += 1
        c["cut " + t["cut"]] += 1
        c["far fast"] += t["path"] == "fast" and t["far"] > 0
        c["far slow"] += t["path"] == "slow" and t["far"] > 0
        c["far sp"] += bool(t["farsp"])
        c["two far"] += t["path"] == "fast" and t["far"] >= 2
        c["stored flush"] += t["path"] == "stored" and t["flush"] > 0
        c["flush"] += t["path"] != "stored" and t["flush"]
        if t["done"]:
            c["done " + t["done"]] += 1
        for b in t["copies"]:
            c["copy " + b] += 1
    return +c


# ---- code sets -----------------------------------------------------------------------------------------------------------------------------
def fill(want, nsym, fillers):
    """{symbol: length} -> a complete set of nsym lengths: symbols of `fillers` (unused ones, which still get codes) take up what is left"""
    lens = [0] * nsym
    for s, l in want.items():
        lens[s] = l
    left = (1 << 15) - kraft(lens)
    assert left >= 0, "over-subscribed"
    fillers = [s for s in fillers if s not in want]
    for bit in range(14, -1, -1):
        if left >> bit & 1:
            lens[fillers.pop(0)] = 15 - bit
    assert kraft(lens) == 1 << 15
    return lens


def split_depths(rng, n, maxlen, deep=False):
    """a complete prefix code of n leaves (n >= 2): one leaf, then random leaves of depth under maxlen split in two; deep: a chain down to maxlen first"""
    leaves = (list(range(1, maxlen)) + [maxlen, maxlen]) if deep and n > maxlen else [1, 1]
    while len(leaves) < n:
        cand = [k for k, d in enumerate(leaves) if d < maxlen]
        d = leaves.pop(cand[int(rng.integers(len(cand)))])
        leaves += [d + 1, d + 1]
    return sorted(leaves)


LL_PROFILES = ("fast", "long", "eob short", "eob 15", "unused")


def random_ll(rng, freq, profile):
    """literal/length lengths over the symbols of freq (a Counter that holds EOB): all within the fast table / the frequent symbols at
    10 to 15 bits / EOB the shortest / EOB at 15 bits / unused symbols that still have codes"""
    syms = [s for s, _ in freq.most_common()]
    spare = [s for s in range(285, -1, -1) if s not in freq]
    extra = {"fast": 0, "long": max(0, 24 - len(syms)), "eob short": 0, "eob 15": max(0, 18 - len(syms)), "unused": int(rng.integers(8, 30))}[profile]
    syms += spare[:extra] if profile != "unused" else [spare[int(k)] for k in rng.choice(len(spare), extra, replace=False)]
    if len(syms) < 2:
        syms.append(spare[0])
    depths = split_depths(rng, len(syms), 9 if profile in ("fast", "eob short") else 15, deep=profile in ("long", "eob 15"))
    if profile == "long":
        depths = depths[::-1]
    elif profile == "eob short":
        syms.remove(EOB)
        syms.insert(0, EOB)
    elif profile == "eob 15":
        syms.remove(EOB)
        syms.append(EOB)
    elif profile == "unused":
        syms = [syms[int(k)] for k in rng.permutation(len(syms))]
    lens = [0] * (max(syms) + 1 if max(syms) >= 257 else 257)
    for s, d in zip(syms, depths):
        lens[s] = d
    pad = int(rng.integers(0, 287 - len(lens))) if len(lens) < 286 else 0         # HLIT padded with zeros
    return lens + [0] * pad


def random_dd(rng, used, profile):
    """distance lengths: "none" (no match in the block), "single" (one symbol, a one-bit code), "fast" (all within 8 bits) or "long\""""
    if profile == "none":
        return [0]
    if profile == "single":
        (s,) = used
        return [0] * s + [1]
    syms = sorted(used)
    spare = [s for s in range(30) if s not in used]
    want = max(2, 18 if profile == "long" else 0, len(syms) + int(rng.integers(0, 4)))
    syms += [spare[int(k)] for k in rng.choice(len(spare), min(len(spare), want - len(syms)), replace=False)] if want > len(syms) else []
    depths = split_depths(rng, len(syms), 15 if profile == "long" else 8, deep=profile == "long")
    order = [syms[int(k)] for k in rng.permutation(len(syms))]
    lens = [0] * (max(syms) + 1)
    for s, d in zip(order, depths):
        lens[s] = d
    return lens


# ---- the seeded random family ----------------------------------------------------------------------------------------------------------------
def _draw_tokens(rng, text, budget, alphabet, far):
    """tokens of one Huffman block, about `budget` bytes of text appended to `text`"""
    toks, end = [], len(text) + budget
    while len(text) < end:
        have = len(text)
        if have == 0 or rng.random() < 0.35:
            for _ in range(int(rng.integers(1, 40))):                       # a run of literals
                b = int(alphabet[int(rng.integers(len(alphabet)))])
                toks.append(lit(b))
                text.append(b)
            continue
        if rng.random() < 0.04:                                             # a burst of cheap long matches: more than WIN_OUT bytes within 64 bits
            d = min(have, int(rng.integers(1, 4)))
            for _ in range(int(rng.integers(6, 30))):
                if len(text) >= end:
                    break
                toks.append(match(258, d))
                text += (bytes(text[-d:]) * (258 // d + 1))[:258]
            continue
        n = int(rng.choice([3, 64, 65, 258, int(rng.integers(3, 259)), int(rng.integers(3, 20))]))
        r = rng.random()
        if r < 0.45:
            d = int(rng.integers(1, 70))
        elif r < 0.65:
            d = REACH + int(rng.integers(-3, 4))
        elif r < 0.75 and far:
            d = 32768 - int(rng.integers(0, 4))
        elif r < 0.85:
            d = RING + int(rng.integers(-3, 4))
        else:
            d = int(rng.integers(1, min(have, 32768) + 1))
        d = min(d, have, 32768)
        toks.append(match(n, d))
        if d >= n:
            text += text[have - d:have - d + n]
        else:
            text += (bytes(text[-d:]) * (n // d + 1))[:n]
    return toks


def random_member(rng, name, far=False):
    """1 to 12 blocks of random types; the text is 48 KB at the most (80 KB where far distances need it)"""
    nblocks = int(rng.integers(1, 13))
    size = int(rng.choice([0, 1, 70, 700, 5000, 20000, 47000])) if not far else int(rng.integers(40000, 78000))
    size = int(size * rng.random()) if rng.random() < 0.5 and not far else size
    alphabet = rng.choice(256, int(rng.integers(1, 40)), replace=False)
    text, blocks = bytearray(), []
    for k in range(nblocks):
        budget = max(0, (size - len(text)) // (nblocks - k)) if k < nblocks - 1 else max(0, size - len(text))
        kind = int(rng.integers(0, 4)) if not (far and k == 0) else 0
        if kind == 0:                                                       # stored (a far member begins with one: bulk to reach back into)
            n = min(65535, budget if not far or k else 34000)
            if rng.random() < 0.15:
                n = 0
            data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            blocks.append(Stored(data, int(rng.integers(0, 256))))
            text += data
            continue
        toks = _draw_tokens(rng, text, budget, alphabet, far) if budget and rng.random() < 0.9 else []
        toks.append(END)
        if kind == 1:
            blocks.append(Fixed(toks))
            continue
        freq = collections.Counter(t[1] if t[0] == "lit" else EOB if t[0] == "eob" else length_symbol(t[1]) for t in toks)
        dused = {dist_symbol(t[2]) for t in toks if t[0] == "match"}
        ll = random_ll(rng, freq, LL_PROFILES[int(rng.integers(len(LL_PROFILES)))])
        dprof = "none" if not dused else "single" if len(dused) == 1 and rng.random() < 0.7 else ("fast", "long")[int(rng.integers(2))]
        blocks.append(Dynamic(ll, random_dd(rng, dused, dprof), toks, ("greedy", "greedy", "plain")[int(rng.integers(3))], 19 if rng.random() < 0.2 else None))
    gz = {}
    if rng.random() < 0.3:
        gz = dict(fextra=int(rng.integers(0, 60)) if rng.random() < 0.5 else None, fname=int(rng.integers(0, 60)), fcomment=int(rng.integers(0, 60)) if rng.random() < 0.5 else None)
    m = member(name, blocks, "random", tail_junk=int(rng.integers(0, 256)), **gz)
    assert m.text == bytes(text)
    return m


SPACER_RESIDUES = (1, 63, 64, 4031, 4095)


def stream_cases(seed, n=20):
    """the random family: members with plain spacer entries of 1 to 3 bytes and of lengths = 1, 63, 64, 4031, 4095 (mod 4096) between them,
    so that the members' input misalignment covers 0 .. 3 and their texts start at chosen places of a round"""
    rng = np.random.default_rng([20261021, seed])
    out = []
    for k in range(n):
        s = int(rng.integers(1, 4)) if k % 2 else SPACER_RESIDUES[(k // 2) % 5] + ROUND * int(rng.integers(0, 2))
        out.append(spacer(s, k))
        out.append(random_member(rng, f"random {seed}.{k}", far=k % 7 == 3))
    return out


# ---- designed cases ------------------------------------------------------------------------------------------------------------------------
A, B, Z = 97, 98, 90            # two literals with short codes; Z: a literal with a LONG code, which ends a window: the next starts behind it
BREAK = lit(Z)
FAR_DISTS = (REACH - 1, REACH, REACH + 1, RING - 1, RING, RING + 1, 32767, 32768)


def design_code(ll_want, dd_want, zbits=10):
    """the designed cases' code sets: the wanted lengths, Z at zbits, completed with unused symbols"""
    ll = dict(ll_want)
    ll.setdefault(Z, zbits)
    ll.setdefault(EOB, 6)
    return fill(ll, 286, range(128, 256)), (fill(dd_want, 30, range(29, -1, -1)) if dd_want else [0])


def noise(n, salt):
    return np.random.default_rng([77, salt]).integers(0, 256, n, dtype=np.uint8).tobytes()


def _other(text, back):
    """a literal of {A, B} that differs from the byte `back` bytes in front of the text's end"""
    return lit(B if text[len(text) - back] == A else A)


def bulk(n):
    """tokens of a fixed block that make n bytes of text"""
    toks = [lit(65 + k % 26) for k in range(min(n, 40))]
    n -= len(toks)
    while n >= 3:
        m = min(n, 258)
        m -= 3 if n - m in (1, 2) else 0
        toks.append(match(m, 7))
        n -= m
    return toks + [lit(A)] * n


def _len_syms(lengths, bits):
    return {length_symbol(n): bits for n in lengths}


def designed(omis=0):
    """the designed cases as one batch: entries in order (spacers among them). omis: where the batch's first text byte lies in its round"""
    out = []

    def add(e):
        out.append(e)
        return e

    def at():
        return (omis + sum(len(e.text) for e in out)) & (ROUND - 1)
    LLS = {A: 2, B: 3, 285: 3, 284: 4, 264: 5, 257: 5}                       # short codes (258 as 285; 284 carries 5 extra bits; 264 = length 10; 257 = length 3)
    # D1: every code beyond the fast tables, a 48-bit token; the same tokens with every code inside them
    pre = noise(33000, 1)
    d1 = [lit(A), lit(B), match(250, 30000), match(3, 1), lit(A), match(258, 16385), match(10, 20000), lit(B), match(131, 32768 - 7000), END]
    ll, dd = design_code({A: 10, B: 12, 284: 15, 257: 11, 285: 14, 264: 15, 281: 13, EOB: 13}, {29: 15, 28: 9, 0: 12, 27: 10})
    add(member("D1 long codes", [Stored(pre), Dynamic(ll, dd, d1)], "D1"))
    ll, dd = design_code({A: 2, B: 3, 284: 9, 257: 5, 285: 4, 264: 9, 281: 8, EOB: 7}, {29: 8, 28: 2, 0: 3, 27: 8})
    add(member("D1 fast codes", [Stored(pre), Dynamic(ll, dd, d1)], "D1"))
    ll, dd = design_code({A: 2, B: 3, 284: 9, 257: 5, 285: 4, 264: 9, 281: 8, EOB: 7}, {29: 15, 28: 9, 0: 12, 27: 10})
    add(member("D1 long distance codes", [Stored(pre), Dynamic(ll, dd, d1)], "D1"))
    # D2: distances about the ring's reach, the ring and the window, (i) first in a fast window, (ii) first in a slow window whose
    # literal at ex = WIN_OUT - 1 takes the ring slot one byte in front of REACH, (iii) through a long code
    pre = noise(33000, 2)
    dsyms = {dist_symbol(d) for d in FAR_DISTS}
    dd_far = {**{s: 3 for s in dsyms}, 0: 2}
    for pos in ("fast", "slow", "sp"):
        text, toks = bytearray(pre), []
        for d in FAR_DISTS:
            if pos == "fast":
                seq = [BREAK, match(10, d), lit(A), lit(B), BREAK]
            elif pos == "sp":
                seq = [lit(A), match(9, d), lit(B)]                           # 263 (length 9) has the long code
            else:
                rest = WIN_OUT - 1 - 258 - 2 * 258
                seq = [BREAK, match(258, d), match(258, 1), match(258, 1), match(rest, 1), _other(text, REACH), BREAK]      # (behind Z the window starts at len(text) + 1)
            toks += seq
            for t in seq:                                                     # (the text so far, to choose the literal by)
                if t[0] == "lit":
                    text.append(t[1])
                else:
                    n, d2 = t[1], t[2]
                    text += text[len(text) - d2:len(text) - d2 + n] if d2 >= n else (bytes(text[-d2:]) * (n // d2 + 1))[:n]
        ll, dd = design_code({**LLS, 263: 12}, dd_far)
        add(member(f"D2 {pos}", [Stored(pre), Dynamic(ll, dd, toks + [END])], "D2"))
    # D2: a distance equal to all the text so far, and one byte more, on the three paths, at 5 bytes of text and at 32767
    for have in (5, 32767):
        for pos in ("fast", "slow", "sp"):
            for more in (0, 1):
                d = have + more
                ll, dd = design_code({**LLS, 263: 12}, {dist_symbol(d): 1, 0: 1})
                first = [Stored(noise(have, 3))] if have > 5 else [Fixed([lit(65 + k) for k in range(5)] + [END])]
                toks = {"fast": [match(3, d), lit(A)], "slow": [match(3, d), match(258, 1)], "sp": [match(9, d), lit(A)]}[pos] + [END]
                add(spacer(37 + 101 * (len(out) % 40), len(out)))                   # (the member's text starts anywhere in its round: positions count from the round's edge, distances from the text's start)
                add(member(f"D2 all text {have} {pos}{' + 1' if more else ''}", first + [Dynamic(ll, dd, toks)], "D11" if more else "D2", "reject" if more else "ok", strict=False))
    # D3: a pending far copy and what completes it; two far matches in one window
    pre = noise(9000, 4)
    ll, dd = design_code(LLS, {dist_symbol(REACH + 1): 2, dist_symbol(RING + 40): 2, 0: 2})
    far = match(10, REACH + 1)
    add(member("D3 next window", [Stored(pre), Dynamic(ll, dd, [BREAK, far] + [lit(A)] * 40 + [END])], "D3"))
    add(member("D3 long code", [Stored(pre), Dynamic(ll, dd, [BREAK, far, lit(B), BREAK, lit(A), END])], "D3"))
    add(member("D3 end of block", [Stored(pre), Dynamic(ll, dd, [BREAK, far, lit(B), END]), Fixed([lit(A), END])], "D3"))
    add(member("D3 two far", [Stored(pre), Dynamic(ll, dd, [BREAK, far, lit(B), match(10, RING + 40), lit(A), BREAK, END])], "D3"))
    add(spacer(1, 5))
    n = (ROUND - 21 - at()) % ROUND                                          # stored text, then Z, then the window begins 20 bytes in front of a round's edge
    while n < REACH + 50:
        n += ROUND
    add(member("D3 round flush", [Stored(noise(n, 5)), Dynamic(ll, dd, [BREAK, far] + [lit(A)] * 40 + [END])], "D3"))
    # D4: a window's text of exactly 64 and 65 bytes; dist == ex + len (fast) and ex + len - 1 (slow)
    pre = noise(300, 6)
    ll, dd = design_code({**LLS, **_len_syms((60, 61), 4)}, {dist_symbol(200): 2, dist_symbol(13): 2, dist_symbol(12): 3, 0: 3})
    add(member("D4 text 64", [Stored(pre), Dynamic(ll, dd, [BREAK, match(60, 200)] + [lit(A)] * 4 + [BREAK, END])], "D4"))
    add(member("D4 text 65", [Stored(pre), Dynamic(ll, dd, [BREAK, match(61, 200)] + [lit(A)] * 4 + [BREAK, END])], "D4"))
    add(member("D4 dist = ex + len", [Stored(pre), Dynamic(ll, dd, [BREAK, lit(A), lit(B), lit(A), match(10, 13), BREAK, END])], "D4"))
    add(member("D4 dist = ex + len - 1", [Stored(pre), Dynamic(ll, dd, [BREAK, lit(A), lit(B), lit(A), match(10, 12), BREAK, END])], "D4"))
    # D5: copies that overlap their own output, in a window (the slow path) and through a long length code
    lens5 = (3, 63, 64, 65, 258)
    pairs = [(n, d) for n in lens5 for d in sorted({1, 2, 3, 63, 64, 65, n - 1, n, n + 1})]
    pre = bytes(range(256)) + noise(300, 7)
    for nm, bits in (("slow", 4), ("sp", 11)):
        ll, dd = design_code({A: 2, B: 3, **_len_syms(lens5, bits)}, {dist_symbol(d): 4 for _, d in pairs})
        toks = []
        for n, d in pairs:
            toks += [lit(A), lit(B), match(n, d), BREAK]
        add(member(f"D5 overlap {nm}", [Stored(pre), Dynamic(ll, dd, toks + [END])], "D5"))
    # D6: length 258 and the distance in one bit each, 32 matches a window: the WIN_OUT cut with ex + outn = WIN_OUT and WIN_OUT + 1; the densest stream
    ll6 = fill({285: 1, A: 3, 284: 3, Z: 10, EOB: 4}, 286, range(128, 256))
    for edge in (WIN_OUT, WIN_OUT + 1):
        toks = [lit(A), BREAK] + [match(258, 1)] * 3 + [match(edge - 3 * 258, 1)] + [match(258, 1)] * 60 + [BREAK]
        add(member(f"D6 cut at {edge}", [Dynamic(ll6, [1], toks + [END])], "D6"))
    add(member("D6 window of exactly WIN_OUT", [Dynamic(ll6, [1], [lit(A), BREAK] + [match(258, 1)] * 3 + [match(WIN_OUT - 3 * 258, 1), BREAK, lit(A), END])], "D6"))
    add(member("D6 densest", [Dynamic(fill({285: 1, A: 2, EOB: 2}, 286, []), [1], [lit(A)] + [match(258, 1)] * 300 + [END])], "D6"))
    # D7: where the text ends in its round; a text inside one lane segment shared with both neighbours; empty texts
    for r in (0, 1, 63, 64, ROUND - 1):
        n = (r - at()) % ROUND or ROUND
        add(member(f"D7 ends at {r}", [Fixed(bulk(n) + [END])], "D7"))
    add(spacer((70 - at()) % ROUND or 1, 8))
    for k in range(3):
        add(member(f"D7 shared segment {k}", [Fixed([lit(48 + k)] * (7 + k) + [END])], "D7"))
    add(member("D7 empty stored", [Stored(b"")], "D7"))
    add(member("D7 empty fixed", [Fixed([END])], "D7"))
    add(member("D7 empty dynamic", [Dynamic(fill({A: 1, EOB: 1}, 257, []), [0], [END])], "D7"))
    # D8: stored blocks
    add(member("D8 LEN 0 mid-stream", [Fixed([lit(A), END]), Stored(b"", 0x55), Fixed([lit(B), END]), Stored(b""), Stored(b"xy")], "D8"))
    add(member("D8 LEN 65535", [Stored(noise(65535, 9)), Fixed([match(258, 65535 - 40000), END])], "D8"))
    for k in range(8):                                                        # 3 + 9 k + 7 bits in front: every bit phase
        add(member(f"D8 stored at phase {(3 + 9 * (k + 1) + 7 + 3) % 8}", [Fixed([lit(200)] * (k + 1) + [END]), Stored(b"stored %d" % k, 0xff), Fixed([match(4, 6), END])], "D8"))
    add(member("D8 stored across blocks, then a far match", [Fixed([lit(A), END]), Stored(noise(9000, 10), 0xaa), Fixed([match(20, 8000), match(258, REACH + 1), lit(B), END])], "D8"))
    # D9: header and framing
    add(member("D9 258 as 284 + 31", [Fixed([lit(A), match(258, 1, sym=284), lit(B), match(258, 2, sym=284), END])], "D9"))
    ll = fill({A: 2, B: 2, EOB: 2, 270: 3, 271: 4, 272: 5, 273: 5}, 274, [])       # the last lengths 5, 5 and the first distance lengths 5, 5, 5, 5: a 16-run across
    add(member("D9 16-run across", [Dynamic(ll, [5] * 4 + [3] * 7, [lit(A), lit(B), match(23, 1), END])], "D9"))
    ll = fill({A: 2, B: 2, EOB: 2, 257: 2}, 270, [])                          # zeros from 258 to 269, zeros in front of distance symbol 12: an 18-run across
    add(member("D9 18-run across", [Dynamic(ll, [0] * 12 + [1, 1], [lit(A), lit(B)] * 50 + [match(3, 70), match(3, 97), END])], "D9"))
    ll, dd = design_code(LLS, {0: 1, 1: 1})
    add(member("D9 HCLEN 19", [Dynamic(ll, dd, [lit(A), match(10, 1), END], "greedy", 19)], "D9"))
    ll = fill({A: 2, B: 2, EOB: 3, 257: 3, 284: 3, 285: 3}, 286, [])
    add(member("D9 HLIT 286", [Dynamic(ll, [1, 1], [lit(A), lit(B), match(3, 2), END])], "D9"))
    ll, dd = design_code(LLS, {0: 1, 1: 1})
    for mis in range(4):
        add(spacer((mis - sum(len(e.data) for e in out)) % 4 or 4, 11))
        add(member(f"D9 header across an input block, mis {mis}", [Stored(noise(IN_BLOCK - 10 - 5 - 6 - mis, 12)), Dynamic(ll, dd, [lit(A), match(10, 1), END], "plain")], "D9"))
    add(member("D9 pad bits before the trailer", [Fixed([lit(A), END])], "D9", tail_junk=0xff))
    for hdr in (251, 252, 253):
        for mis in range(4):
            add(spacer((mis - sum(len(e.data) for e in out)) % 4 or 4, 13))
            gz = (dict(fname=hdr - 11), dict(fextra=hdr - 12), dict(fextra=100, fname=20, fcomment=hdr - 12 - 100 - 21 - 1))[(hdr + mis) % 3]
            add(member(f"{'D12 long header' if hdr > 252 else 'D9 header of'} {hdr}, mis {mis}", [Fixed([lit(A), match(5, 1), END])], "D12" if hdr > 252 else "D9", "handback" if hdr > 252 else "ok", **gz))
    # D10: incomplete distance sets zlib accepts
    ll, _ = design_code(LLS, None)
    add(member("D10 single distance code", [Dynamic(ll, [0, 0, 1], [lit(A), lit(B), lit(A), match(10, 3), match(258, 3), BREAK, match(3, 3), END])], "D10"))
    add(member("D10 no distance code", [Dynamic(ll, [0], [lit(A), lit(B), BREAK, lit(A), END])], "D10"))
    # D11: what zlib rejects
    rej = dict(group="D11", expect="reject", strict=False)
    one = canon(ll)[264]
    add(member("D11 the unused one-bit distance pattern", [Dynamic(ll, [0, 0, 1], [lit(A), lit(B), lit(A), raw(int(format(one[0], "0%db" % one[1])[::-1], 2), one[1]), raw(1, 1), lit(A), END])], **rej))
    add(member("D11 a length with no distance code", [Dynamic(ll, [0], [lit(A), lit(B), lit(A), raw(int(format(one[0], "0%db" % one[1])[::-1], 2), one[1]), raw(0, 4), lit(A), END])], **rej))
    inc = [0] * 257
    inc[A], inc[EOB] = 2, 2
    add(member("D11 incomplete literal set", [Dynamic(inc, [1, 1], [lit(A), END])], **rej))
    over = [0] * 257
    over[A], over[B], over[EOB] = 1, 1, 1
    add(member("D11 over-subscribed literal set", [Dynamic(over, [1, 1], [lit(A), END])], **rej))
    add(member("D11 over-subscribed distance set", [Dynamic(ll, [1, 1, 1], [lit(A), END])], **rej))
    add(member("D11 incomplete distance set of two bits", [Dynamic(ll, [2, 2, 2], [lit(A), END])], **rej))
    two = fill({A: 1, EOB: 1}, 257, [])
    add(member("D11 code-length code of one symbol", [Dynamic(two, [0], [lit(A), END], [(0, 0)] * 258, None, [1] + [0] * 18)], **rej))
    add(member("D11 repeat past the end", [Dynamic(two, [0], [lit(A), END], [(0, 0)] * 97 + [(1, 0), (18, 127), (18, 127 - 100)], None, None)], **rej))
    no_eob = fill({A: 1, B: 1}, 257, [])
    add(member("D11 no code for 256", [Dynamic(no_eob, [1, 1], [lit(A), lit(B)])], **rej))
    # D12: what zlib reads and the device may hand back (fcz_hip.h): with the long headers above
    lone = [0] * 257
    lone[EOB] = 1
    add(member("D12 lone one-bit end of block", [Dynamic(lone, [0], [END])], "D12", "handback"))
    add(member("D12 lone one-bit end of block, mid-stream", [Fixed([lit(A), END]), Dynamic(lone, [0], [END]), Fixed([lit(B), END])], "D12", "handback"))
    return out


HANDBACK_CLASSES = ("D12 long header", "D12 lone one-bit end of block")


def crc_of(entries):
    c = 0
    for e in entries:
        c = zlib.crc32(e.data, zlib.crc32(bytes([e.kind]), c))
    return c


def zlib_says(data):
    """the text zlib's inflate() gives for the bytes as a gzip member, or None"""
    d = zlib.decompressobj(31)
    try:
        out = d.decompress(data)
    except zlib.error:
        return None
    return out if d.eof else None
