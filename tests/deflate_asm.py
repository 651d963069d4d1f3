"""A DEFLATE assembler (RFC 1951) and the corpus of hand-made streams the inflater is tested on.

Everything the suite had for xenomapper_amd/csrc/xm_inflate_core.h was written by zlib's encoder or by the project's own; both
are narrow producers.  Here a stream is put together bit by bit: the caller chooses every code length, every symbol, every extra
bit and the code-length symbol sequence of a dynamic header, so that streams other encoders write (and streams with exactly one
defect) can be stated.  The module is written from the RFC's text and tables and shares nothing with the project's C sources:
what a token sequence MEANS is worked out by Stream.token() below (the expected bytes), and zlib is the referee for both
(tests/test_inflate_streams_cpu.py).

    valid_corpus()    -> [Valid(name, stream, expected, rec)]
    invalid_corpus()  -> [Invalid(name, stream, isize, status, rec)]       status: the xmi::ERR_* the decoder must end with

`rec` is the assembler's own record of what the stream exercises (block types, token widths, code lengths, (symbol, extra) pairs
per class of code, stored-block paddings); the coverage assertions read it, never the code under test.

Conventions the two decoder builds rely on for the invalid members: a reader that runs past the end of a stream meets zero bytes
(the host harness pads with zeros, an invalid BGZF member carries a zero CRC field), and every ISIZE is at least 1 (the kernel
does not decode members of ISIZE 0).
"""
import collections
import os
import struct
import subprocess
import zlib

import numpy as np

# ---- the statuses of xm_inflate_core.h (the test pins the numbers: they are ABI, xm_bgzf_strerror) ----------------------------
OK, ERR_BTYPE, ERR_STORED, ERR_LENGTHS, ERR_OVERSUB, ERR_NO_EOB, ERR_CODE, ERR_DIST, ERR_OUT, ERR_IN, ERR_SHORT, ERR_LENSYM = range(12)
ERR_GUARD, ERR_INCOMPLETE = 12, 13

# ---- RFC 1951 3.2.5: the tables as the RFC prints them ---------------------------------------------------------------------------
LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
         12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLC_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32                     # 30 and 31 have codes and no meaning (3.2.6)

MAX_CDATA, MAX_ISIZE = 65510, 65536       # what a BGZF member holds (26 bytes of frame in 65536)

Valid = collections.namedtuple("Valid", "name stream expected rec")
Invalid = collections.namedtuple("Invalid", "name stream isize status rec")


class BitWriter:
    """Fields least significant bit first, Huffman codes most significant bit first (3.1.1)."""

    def __init__(self):
        self.acc, self.n = 0, 0

    def bits(self, value, n):
        assert 0 <= value < (1 << n) or n == 0
        self.acc |= value << self.n
        self.n += n

    def code(self, code, n):
        self.bits(int(format(code, "0%db" % n)[::-1], 2) if n else 0, n)

    def align(self):
        pad = -self.n % 8
        self.n += pad
        return pad

    def raw(self, data):
        assert self.n % 8 == 0
        self.acc |= int.from_bytes(data, "little") << self.n
        self.n += 8 * len(data)

    def finish(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def canonical(lens):
    """Code lengths -> codes, by the algorithm of 3.2.2."""
    count = [0] * 16
    for ln in lens:
        count[ln] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    codes = [0] * len(lens)
    for s, ln in enumerate(lens):
        if ln:
            codes[s] = nxt[ln]
            nxt[ln] += 1
    return codes


def kraft(lens):
    """Code space in use, in units of 2^-15: 32768 is a complete code."""
    return sum(1 << (15 - ln) for ln in lens if ln)


def lens_of(n, table):
    lens = [0] * n
    for s, ln in table.items():
        lens[s] = ln
    return lens


def fill(units, syms, minlen):
    """{symbol: length} that uses exactly `units` x 2^-15 of code space for `syms`, no code shorter than minlen, the first
    symbols the shortest: all at 15 bits, then one symbol after the other is shortened while space is left."""
    got = {s: 15 for s in syms}
    left = units - len(syms)
    assert left >= 0
    for s in syms:
        while left and got[s] > minlen and (1 << (15 - got[s])) <= left:
            left -= 1 << (15 - got[s])
            got[s] -= 1
    assert left == 0, "the symbols cannot fill the space"
    return got


def ladder(short, rest, minlen):
    """A complete code: short[i] gets i + 1 bits, `rest` share the remaining 2^-len(short), none shorter than minlen."""
    table = {s: i + 1 for i, s in enumerate(short)}
    table.update(fill(1 << (15 - len(short)), rest, minlen))
    return table


def flat(syms):
    """A complete code over `syms` with two adjacent lengths."""
    p = len(syms).bit_length() - 1
    longer = 2 * (len(syms) - (1 << p))
    return {s: (p + 1 if i >= len(syms) - longer else p) for i, s in enumerate(syms)}


def one_by_one(lens):
    return [(ln, 0) for ln in lens]


def run_length(lens):
    """The code-length symbols an ordinary encoder would send: runs of zeros as 17 / 18, repeats as 16."""
    out, i = [], 0
    while i < len(lens):
        j = i
        while j < len(lens) and lens[j] == lens[i]:
            j += 1
        run = j - i
        if lens[i] == 0:
            while run >= 11:
                take = min(run, 138)
                out.append((18, take - 11))
                run -= take
            if run >= 3:
                out.append((17, run - 3))
                run = 0
        else:
            out.append((lens[i], 0))
            run -= 1
            while run >= 3:
                take = min(run, 6)
                out.append((16, take - 3))
                run -= take
        out += [(lens[i], 0)] * run
        i = j
    return out


def clc_for(cl_syms):
    """A complete code-length code (<= 7 bits) over the symbols a sequence uses (two at least: zlib refuses a lone one)."""
    used = sorted(set(s for s, _ in cl_syms))
    for s in (0, 18):
        if len(used) < 2 and s not in used:
            used.append(s)
    table = flat(sorted(used))
    assert max(table.values()) <= 7
    return lens_of(19, table)


def hclen_for(clc_lens):
    return max(4, max(i + 1 for i, s in enumerate(CLC_ORDER) if clc_lens[s]))


class Stream:
    """One raw-DEFLATE stream in the making, the bytes its tokens stand for, and the record of what it exercises."""

    def __init__(self, name):
        self.name = name
        self.w = BitWriter()
        self.out = bytearray()
        self.broken = False              # a token had no meaning (invalid streams): `out` ends in front of it
        self.rec = dict(blocks=set(), token_bits=set(), lit_lens=set(), dist_lens=set(), clc_lens=set(), len_pairs=set(),
                        dist_pairs=set(), paddings=set(), hlit=set(), hdist=set(), hclen=set(), n_blocks=0, lit_syms=set())
        self.cls = None

    # -- blocks --
    def header(self, final, btype):
        self.w.bits(1 if final else 0, 1)
        self.w.bits(btype, 2)
        if btype < 3:
            self.rec["blocks"].add(btype)
        self.rec["n_blocks"] += 1

    def stored(self, data, final=False, nlen=None, present=None):
        """present: how many of the data bytes really follow (an invalid stream: fewer than LEN says)."""
        self.header(final, 0)
        self.rec["paddings"].add(self.w.align())
        self.w.bits(len(data), 16)
        self.w.bits((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
        self.w.raw(bytes(data) if present is None else bytes(data[:present]))
        if nlen is None and present is None:
            self.out += data
        else:
            self.broken = True
        return self

    def fixed(self, tokens, final=False):
        self.header(final, 1)
        self.cls = "fixed"
        return self.tokens(tokens, FIXED_LIT, FIXED_DIST)

    def dynamic(self, tokens, lit, dist, final=False, cl_syms=None, clc_lens=None, hclen=None, hlit=None, hdist=None, body=True):
        """lit / dist: {symbol: length}.  hlit / hdist default to the smallest that hold the codes; the code-length symbol
        sequence defaults to the run-length form, the code-length code to a flat complete one over the symbols it uses."""
        hlit = hlit or max(257, max(lit) + 1)
        hdist = hdist or max(1, max(dist) + 1 if dist else 1)
        lit_lens, dist_lens = lens_of(max(hlit, 288), lit), lens_of(32, dist)
        if cl_syms is None:
            cl_syms = run_length(lit_lens[:hlit] + dist_lens[:hdist])
        if clc_lens is None:
            clc_lens = clc_for(cl_syms)
        hclen = hclen or hclen_for(clc_lens)
        self.header(final, 2)
        self.rec["hlit"].add(hlit), self.rec["hdist"].add(hdist), self.rec["hclen"].add(hclen)
        self.rec["clc_lens"] |= set(ln for ln in clc_lens if ln)
        self.w.bits(hlit - 257, 5)
        self.w.bits(hdist - 1, 5)
        self.w.bits(hclen - 4, 4)
        assert all(clc_lens[s] == 0 for s in CLC_ORDER[hclen:]), "a code-length code length that HCLEN does not send"
        for s in CLC_ORDER[:hclen]:
            self.w.bits(clc_lens[s], 3)
        codes = canonical(clc_lens)
        for s, extra in cl_syms:
            assert clc_lens[s], "code-length symbol %d has no code" % s
            self.w.code(codes[s], clc_lens[s])
            if s >= 16:
                self.w.bits(extra, (2, 3, 7)[s - 16])
        self.cls = "dynamic"
        if body:
            self.tokens(tokens, lit_lens, dist_lens)
        return self

    # -- tokens --
    def tokens(self, tokens, lit_lens, dist_lens, eob=True):
        lit_codes, dist_codes = canonical(lit_lens), canonical(dist_lens)
        self.rec["lit_lens"] |= set(ln for ln in lit_lens if ln)
        self.rec["dist_lens"] |= set(ln for ln in dist_lens[:30] if ln)
        for t in tokens:
            self.token(t, lit_lens, lit_codes, dist_lens, dist_codes)
        if eob:
            assert lit_lens[256]
            self.w.code(lit_codes[256], lit_lens[256])
        return self

    def token(self, t, lit_lens, lit_codes, dist_lens, dist_codes):
        """int: a literal.  ('m', length, distance): a match, the symbols chosen as the RFC's tables say.  ('r', length symbol,
        extra, distance symbol, extra): a match by its fields.  ('sym', s): a literal/length code alone.  ('bits', value, n)."""
        if isinstance(t, int):
            assert lit_lens[t], "literal %d has no code" % t
            self.w.code(lit_codes[t], lit_lens[t])
            self.rec["token_bits"].add(lit_lens[t])
            self.rec["lit_syms"].add(t)
            if not self.broken:
                self.out.append(t)
            return
        if t[0] == "bits":
            self.w.bits(t[1], t[2])
            self.broken = True
            return
        if t[0] == "sym":
            self.w.code(lit_codes[t[1]], lit_lens[t[1]])
            self.broken = True
            return
        if t[0] == "m":
            _, length, distance = t
            ls = 28 if length == 258 else max(i for i in range(28) if LBASE[i] <= length)
            ds = max(i for i in range(30) if DBASE[i] <= distance)
            t = ("r", 257 + ls, length - LBASE[ls], ds, distance - DBASE[ds])
        _, lsym, lextra, dsym, dextra = t
        assert lit_lens[lsym] and dist_lens[dsym], "match symbols %d / %d have no code" % (lsym, dsym)
        lbits, dbits = LEXT[lsym - 257], (DEXT[dsym] if dsym < 30 else 0)
        self.w.code(lit_codes[lsym], lit_lens[lsym])
        self.w.bits(lextra, lbits)
        self.w.code(dist_codes[dsym], dist_lens[dsym])
        self.w.bits(dextra, dbits)
        self.rec["lit_syms"].add(lsym)
        if dsym >= 30:
            self.broken = True
            return
        self.rec["token_bits"].add(lit_lens[lsym] + lbits + dist_lens[dsym] + dbits)
        lcls = "fixed" if self.cls == "fixed" else "root" if lit_lens[lsym] <= 10 else "long"
        dcls = "fixed" if self.cls == "fixed" else "root" if dist_lens[dsym] <= 8 else "long"
        for kind, v in (("zero", 0), ("ones", (1 << lbits) - 1)):
            if lextra == v:
                self.rec["len_pairs"].add((lcls, lsym, kind))
        for kind, v in (("zero", 0), ("ones", (1 << dbits) - 1)):
            if dextra == v:
                self.rec["dist_pairs"].add((dcls, dsym, kind))
        length, distance = LBASE[lsym - 257] + lextra, DBASE[dsym] + dextra
        if distance > len(self.out):
            self.broken = True
        if not self.broken:
            for _ in range(length):
                self.out.append(self.out[-distance])

    # -- results --
    def valid(self):
        assert not self.broken
        data = self.w.finish()
        assert len(data) <= MAX_CDATA and 1 <= len(self.out) <= MAX_ISIZE, (self.name, len(data), len(self.out))
        return Valid(self.name, data, bytes(self.out), self.rec)

    def invalid(self, isize, status, cut=0):
        data = self.w.finish()
        return Invalid(self.name, data[:len(data) - cut], isize, status, self.rec)


# ---- the valid families -------------------------------------------------------------------------------------------------------
def _sweep_pairs():
    lens = [(257 + i, v) for i in range(29) for v in sorted({0, (1 << LEXT[i]) - 1})]
    dists = [(d, v) for d in range(30) for v in sorted({0, (1 << DEXT[d]) - 1})]
    return lens, dists


def _sweep_tokens(lens, dists):
    """every length pair and every distance pair in some token; four different literals in front of each, so that a match at a
    wrong short distance copies other bytes (behind a match at distance 1 every short distance would copy the same)"""
    n = max(len(lens), len(dists))
    toks = []
    for i in range(n):
        toks += [0, 1, 2, 3, ("r",) + lens[i % len(lens)] + dists[i % len(dists)]]
    return toks


def _symbol_sweeps(rng):
    history = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()          # distance 32768 needs it
    lens, dists = _sweep_pairs()
    out = [Stream("sweep_fixed").stored(history).fixed(_sweep_tokens(lens, dists), final=True).valid()]
    # the root tables and window_tokens: every length symbol at <= 10 bits, every distance symbol at <= 8
    lit = flat([0, 1, 2, 3] + list(range(256, 286)))
    dist = flat(list(range(30)))
    assert max(lit.values()) <= 10 and max(dist.values()) <= 8
    out.append(Stream("sweep_root").stored(history).dynamic(_sweep_tokens(lens, dists), lit, dist, final=True).valid())
    # long_token (and the host's decode() walk): length symbols at 11 .. 15 bits, distance symbols at 9 .. 15.  Thirty distance
    # symbols of >= 9 bits cannot make a complete code, so two blocks, each with eight short codes for the symbols the other tests
    lit = ladder(list(range(9)), list(range(257, 286)) + [256], 11)
    assert min(lit[s] for s in range(257, 286)) == 11 and lit[284] == 15
    s = Stream("sweep_long").stored(history)
    for final, short in ((False, list(range(8))), (True, list(range(22, 30)))):
        rest = [d for d in range(30) if d not in short]
        dist = ladder(short, rest, 9)
        assert min(dist[d] for d in rest) == 9 and max(dist.values()) == 15
        toks = _sweep_tokens(lens, [p for p in dists if p[0] in rest])
        if not final:
            assert dist[29] == 15
            toks = toks[:35] + [("r", 284, 31, 29, 8191)] + toks[35:]           # the 48-bit token: 258 bytes from 32768 back
        s.dynamic(toks, lit, dist, final=final)
    assert 48 in s.rec["token_bits"]
    out.append(s.valid())
    return out


ONE_BIT = ({97: 1, 256: 1}, {})                                              # 'a' is one bit, and so is the end of the block
RUN = ({97: 1, 285: 2, 256: 2}, {0: 1})                                      # 'a', a 258-byte match (3 bits with its distance), EOB


def _token_widths(rng):
    out = []
    for n in (1, 63, 64, 65, 127, 128, 129, 4000):
        out.append(Stream("one_bit_literals_%d" % n).dynamic([97] * n, *ONE_BIT, final=True).valid())
    # the widest token behind k one-bit literals: it straddles the end of the 64-bit window from k = 17 on
    history = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    lit = ladder([97] + list(range(8)), list(range(257, 286)) + [256], 11)
    dist = ladder(list(range(8)), list(range(8, 30)), 9)
    assert lit[284] == 15 and dist[29] == 15
    s = Stream("widest_token_at_every_window_offset").stored(history)
    for k in list(range(0, 66)) + [127, 128]:
        s.dynamic([97] * k + [("r", 284, 31, 29, 8191), 97], lit, dist)
    out.append(s.fixed([0], final=True).valid())
    for held in (0, 1, 2, 62, 63, 64, 65, 127, 128, 129):
        s = Stream("run_behind_%d_open_bytes" % held)
        if held == 0:
            s.fixed([97])                                                    # the match is its block's first token
        out.append(s.dynamic([97] * held + [("m", 258, 1)] + [97] * 3 + [("m", 258, 1)], *RUN, final=True).valid())
    return out


def _batches(rng):
    out = [Stream("literal_then_258_at_distance_1").fixed([7, ("m", 258, 1)], final=True).valid()]
    for d in (1, 2, 3, 63, 64, 65):
        toks = [int(b) for b in rng.integers(0, 256, d)]
        for ln in range(3, 259):
            toks += [("m", ln, d), int(rng.integers(0, 256))]
        out.append(Stream("every_length_at_distance_%d" % d).fixed(toks[:-1], final=True).valid())   # ends with a match, at ISIZE
    # sources inside the batch the match is dealt into: short literal runs, short matches at short distances
    toks, made = [], 0
    while made < 6000:
        k = int(rng.integers(1, 9))
        toks += [int(b) for b in rng.integers(0, 256, k)]
        made += k
        for _ in range(int(rng.integers(1, 4))):
            ln, d = int(rng.integers(3, 40)), int(rng.integers(1, min(made, 60) + 1))
            toks.append(("m", ln, d))
            made += ln
    out.append(Stream("sources_inside_the_batch").fixed(toks, final=True).valid())
    # sources on both sides of the boundary between the output ring and memory
    toks = []
    for d in range(100, 1101, 7):
        toks += [("m", int(rng.integers(3, 259)), d), int(rng.integers(0, 256))]
    out.append(Stream("sources_around_the_ring").stored(rng.integers(0, 256, 2500, dtype=np.uint8).tobytes())
               .fixed(toks, final=True).valid())
    for k in (1, 5, 63, 64, 65, 1500):
        toks = [int(b) for b in rng.integers(0, 256, k)] + [("m", min(258, k + 7), k)]
        out.append(Stream("distance_reaches_the_first_byte_%d" % k).fixed(toks, final=True).valid())
    # any token after any other, every symbol of both alphabets in use (the tables: eight- and nine-bit codes over all 286
    # literal/length symbols, many of one length in every chunk of 64)
    lit, dist = flat(list(range(286))), flat(list(range(30)))
    toks = [int(b) for b in rng.permutation(256)] + [("m", LBASE[i], 1 + 8 * i) for i in range(29)]
    made = 256 + sum(LBASE)
    while made < 40000:
        if rng.random() < 0.5:
            toks.append(int(rng.integers(0, 256)))
            made += 1
        else:
            ln = int(rng.integers(3, 259))
            d = int(min(made, 32768, rng.geometric(0.002 if rng.random() < 0.5 else 0.05)))
            toks.append(("m", ln, d))
            made += ln
    s = Stream("all_286_symbols").dynamic(toks, lit, dist, final=True)
    assert s.rec["lit_syms"] == set(range(256)) | set(range(257, 286)) and s.rec["hlit"] == {286} and s.rec["hdist"] == {30}
    out.append(s.valid())
    return out


def _tables(rng):
    out = []
    # the smallest header: HLIT 257, HDIST 1, and no distance code at all (a block of literals)
    s = Stream("hlit_257_hdist_1_no_distance_code").dynamic([0, 255, 0], {0: 2, 255: 2, 256: 1}, {}, final=True)
    assert s.rec["hlit"] == {257} and s.rec["hdist"] == {1}
    out.append(s.valid())
    # codes of exactly 10 and 11 bits (the literal/length root table ends at 10), 8 and 9 (distance), and a 7-bit code-length code
    lit = {**{i: i + 1 for i in range(8)}, **{8: 9, 257: 10, 258: 11, 256: 11}}
    dist = {**{i: i + 1 for i in range(7)}, **{7: 8, 8: 9, 9: 9}}
    hist = [int(b) for b in rng.integers(0, 9, 40)]
    toks = hist + [("m", 3, 13), ("m", 4, 16), ("m", 3, 17), ("m", 4, 24), 8, ("m", 4, 1), ("m", 3, 20)]
    cl_syms = one_by_one(lens_of(259, lit) + lens_of(10, dist))
    clc = lens_of(19, {**{0: 1, 1: 2, 2: 3, 3: 4}, **{s: 7 for s in range(4, 12)}})       # the lengths 4 .. 11 are sent with 7 bits
    assert kraft(lens_of(259, lit)) == 32768 and kraft(lens_of(10, dist)) == 32768 and kraft(clc) == 32768
    s = Stream("codes_at_the_root_table_edges").dynamic(toks, lit, dist, final=True, cl_syms=cl_syms, clc_lens=clc)
    assert {10, 11} <= s.rec["lit_lens"] and {8, 9} <= s.rec["dist_lens"] and 7 in s.rec["clc_lens"]
    out.append(s.valid())
    # one distance code of one bit (what an encoder sends when every match is at one distance)
    out.append(Stream("single_distance_code").dynamic([5, ("m", 10, 1), 6, ("m", 3, 1)], {5: 2, 6: 2, 264: 2, 257: 3, 256: 3},
                                                      {0: 1}, final=True).valid())
    # the empty block: a literal/length code that holds the end-of-block symbol alone, at one bit
    out.append(Stream("only_the_end_of_block_code").dynamic([], {256: 1}, {}).fixed([1], final=True).valid())
    # 16 straight after a run of 17 / 18 repeats ZERO; and a 16 that crosses from the literal/length into the distance lengths
    lit, dist = {0: 1, 1: 2, 256: 3, 257: 3}, {d: 3 for d in range(8)}
    cl = [(1, 0), (2, 0), (18, 127), (16, 3), (16, 0), (18, 93), (17, 0), (3, 0), (16, 3), (16, 0)]
    assert _expand(cl) == lens_of(258, lit) + lens_of(8, dist), "the sequence does not spell the lengths"
    out.append(Stream("repeat_after_zero_run_and_across_hlit").dynamic([0, 1, 0, ("m", 3, 1), ("m", 3, 5), ("m", 3, 8)], lit, dist,
                                                                       final=True, cl_syms=cl).valid())
    # a run of zeros from the literal/length lengths into the distance lengths, HLIT at its largest
    lit, dist = flat(list(range(257))), {9: 1}
    lens = lens_of(286, lit) + lens_of(10, dist)
    cl = run_length(lens)
    assert (18, 38 - 11) in cl
    hist = [int(b) for b in rng.integers(0, 256, 30)]
    out.append(Stream("zero_run_across_hlit_286").dynamic(hist + [3, 3], lit, dist, final=True, hlit=286, cl_syms=cl).valid())
    # the longest header: 316 lengths, each sent by itself with a 7-bit code
    lit, dist = flat(list(range(286))), flat(list(range(30)))
    cl = one_by_one(lens_of(286, lit) + lens_of(30, dist))
    clc = lens_of(19, {**{s: 7 for s in range(16)}, **{16: 3, 17: 2, 18: 1}})
    assert len(cl) == 316 and kraft(clc) == 32768
    toks = [int(b) for b in rng.integers(0, 256, 300)] + [("m", 100, 300), ("m", 258, 5)]
    s = Stream("longest_header").dynamic(toks, lit, dist, final=True, cl_syms=cl, clc_lens=clc)
    assert s.rec["hclen"] == {19} and 7 in s.rec["clc_lens"]
    out.append(s.valid())
    return out


def _expand(cl_syms):
    """what a code-length symbol sequence spells (3.2.7)"""
    got = []
    for s, extra in cl_syms:
        if s < 16:
            got.append(s)
        elif s == 16:
            got += [got[-1]] * (3 + extra)
        elif s == 17:
            got += [0] * (3 + extra)
        else:
            got += [0] * (11 + extra)
    return got


def _block_structure(rng):
    out = []
    s = Stream("300_empty_blocks_then_data")
    for _ in range(300):
        s.fixed([])
    out.append(s.fixed([9, 9, ("m", 5, 2)], final=True).valid())
    data = rng.integers(0, 256, 700, dtype=np.uint8).tobytes()
    lit, dist = flat([0, 1, 2, 3, 256, 257, 258, 285]), flat([0, 5, 10, 17])
    s = Stream("stored_fixed_dynamic_stored").stored(data[:300]).fixed([1, 2, ("m", 30, 200), 3])
    s.dynamic([0, 1, ("m", 258, 310), ("m", 4, 40), 2], lit, {0: 2, 5: 2, 10: 2, 16: 2}).stored(data[300:], final=True)
    assert s.rec["blocks"] == {0, 1, 2}
    out.append(s.valid())
    out.append(Stream("stored_of_length_0").fixed([4, 5]).stored(b"").stored(b"xy").stored(b"", final=True).valid())
    # the padding in front of LEN: behind k empty fixed blocks (10 bits each), and behind j nine-bit literals (every count 0 .. 7)
    for k in range(8):
        s = Stream("stored_behind_%d_empty_blocks" % k)
        for _ in range(k):
            s.fixed([])
        out.append(s.stored(data[:50 + k], final=True).valid())
    for j in range(8):
        s = Stream("stored_behind_%d_nine_bit_literals" % j).fixed([200 + i for i in range(j)]).stored(data[:33 + j], final=True)
        assert s.rec["paddings"] == {(3 - j) % 8}
        out.append(s.valid())
    big = rng.integers(0, 256, MAX_CDATA - 5, dtype=np.uint8).tobytes()
    s = Stream("largest_stored_block").stored(big, final=True)
    v = s.valid()
    assert len(v.stream) == MAX_CDATA
    out.append(v)
    s = Stream("end_of_block_on_the_last_bit").fixed([144, 150, 200, 255, 201, 202, 65, 66], final=True)
    assert s.w.n % 8 == 0
    out.append(s.valid())
    return out


def valid_corpus():
    rng = np.random.default_rng(1951)
    out = _symbol_sweeps(rng) + _token_widths(rng) + _batches(rng) + _tables(rng) + _block_structure(rng)
    assert len(set(v.name for v in out)) == len(out)
    return out


# ---- the invalid streams: exactly one defect each ---------------------------------------------------------------------------------
def invalid_corpus():
    out = []
    s = Stream("block_type_3")
    s.header(True, 3)
    s.w.bits(0, 13)
    out.append(s.invalid(1, ERR_BTYPE))
    out.append(Stream("len_nlen_mismatch").stored(b"0123456789", final=True, nlen=(10 ^ 0xFFFF) ^ 0x0100).invalid(10, ERR_STORED))
    # -- the code-length sequence --
    lit, dist = {0: 1, 256: 1}, {0: 1}
    s = Stream("repeat_as_the_first_length")                                  # HCLEN 4: only 16, 17, 18 and 0 have a length field
    s.dynamic([], lit, dist, final=True, cl_syms=[(16, 0), (0, 0)], clc_lens=lens_of(19, {16: 1, 0: 1}), hclen=4, body=False)
    assert s.rec["hclen"] == {4}
    s.w.bits(0, 16)
    out.append(s.invalid(1, ERR_LENGTHS))
    s = Stream("run_past_the_last_length")                                    # 258 lengths; the last run would write the 259th
    cl = [(1, 0), (18, 127), (18, 117 - 11), (1, 0), (17, 0)]
    assert len(_expand(cl)) == 257 + 3 and _expand(cl)[256] == 1
    s.dynamic([], lit, dist, final=True, cl_syms=cl, body=False)
    s.w.bits(0, 16)
    out.append(s.invalid(1, ERR_LENGTHS))
    s = Stream("hlit_287")
    s.header(True, 2)
    s.w.bits(30, 5), s.w.bits(0, 5), s.w.bits(0, 4), s.w.bits(0, 32)
    out.append(s.invalid(1, ERR_LENGTHS))
    # -- codes that claim more than the code space --
    s = Stream("oversubscribed_code_length_code")
    s.dynamic([0], lit, dist, final=True, cl_syms=run_length(lens_of(257, lit) + [1]), clc_lens=lens_of(19, {0: 1, 1: 1, 18: 1}))
    out.append(s.invalid(1, ERR_OVERSUB))
    out.append(Stream("oversubscribed_literal_code").dynamic([0], {0: 1, 1: 1, 256: 1}, dist, final=True).invalid(1, ERR_OVERSUB))
    out.append(Stream("oversubscribed_distance_code").dynamic([0], lit, {0: 1, 1: 1, 2: 1}, final=True).invalid(1, ERR_OVERSUB))
    s = Stream("no_end_of_block_code").dynamic([0, 1], {0: 1, 1: 1}, dist, final=True, hlit=257, body=False)
    s.w.bits(0b10, 2), s.w.bits(0, 14)
    out.append(s.invalid(2, ERR_NO_EOB))
    # -- bits that are no code: possible only where an incomplete code is allowed --
    s = Stream("bits_that_match_no_code").dynamic([97, 97, 97, ("sym", 257), ("bits", 1, 1)], {97: 1, 257: 2, 256: 2}, {0: 1}, final=True)
    out.append(s.invalid(6, ERR_CODE))
    s = Stream("match_in_a_block_without_distance_codes").dynamic([97, 97, ("sym", 257), ("bits", 0, 1)], {97: 1, 257: 2, 256: 2}, {},
                                                                  final=True)
    out.append(s.invalid(5, ERR_CODE))
    out.append(Stream("fixed_distance_symbol_30").fixed([65] * 40 + [("r", 257, 0, 30, 0)], final=True).invalid(43, ERR_CODE))
    out.append(Stream("length_symbol_286").fixed([65, 66, ("sym", 286)], final=True).invalid(5, ERR_LENSYM))
    # -- a distance one beyond the bytes produced --
    out.append(Stream("distance_beyond_as_first_token").fixed([("m", 3, 1), 1, 2, 3, 4, 5, 6, 7], final=True).invalid(10, ERR_DIST))
    out.append(Stream("distance_beyond_mid_batch").fixed([1, 2, 3, 4, 5, ("m", 4, 6), 6, 7], final=True).invalid(11, ERR_DIST))
    lit = {**{i: i + 1 for i in range(8)}, **{8: 9, 257: 10, 258: 11, 256: 11}}
    s = Stream("distance_beyond_behind_a_long_code").dynamic([0, 1, 2, ("m", 4, 4), 3], lit, flat([0, 1, 2, 3]), final=True)
    out.append(s.invalid(8, ERR_DIST))
    # -- the stream and the member's ISIZE disagree --
    ten = list(range(48, 58))
    out.append(Stream("literal_past_isize").fixed(ten, final=True).invalid(9, ERR_OUT))
    out.append(Stream("match_ends_past_isize").fixed(ten[:5] + [("m", 100, 3)], final=True).invalid(104, ERR_OUT))
    out.append(Stream("end_of_block_short_of_isize").fixed(ten, final=True).invalid(11, ERR_SHORT))
    # -- the stream and its length disagree --
    s = Stream("cut_one_byte_short").stored(bytes(range(20))).fixed([], final=True)    # the end-of-block code lies across the cut
    assert s.w.n == 8 * 25 + 10
    out.append(s.invalid(20, ERR_IN, cut=1))
    s = Stream("stored_block_longer_than_the_data").stored(bytes(100), final=True, present=50)
    out.append(s.invalid(100, ERR_IN))
    # -- incomplete codes (zlib: invalid literal/lengths set, invalid distances set, invalid code lengths set) --
    out.append(Stream("incomplete_literal_code").dynamic([97, 97], {97: 2, 256: 2}, {}, final=True).invalid(2, ERR_INCOMPLETE))
    s = Stream("incomplete_distance_code").dynamic([97, ("m", 3, 1)], {97: 1, 257: 2, 256: 2}, {0: 2, 1: 2}, final=True)
    out.append(s.invalid(4, ERR_INCOMPLETE))
    lit = {97: 1, 256: 1}
    s = Stream("incomplete_code_length_code")
    s.dynamic([97], lit, {}, final=True, cl_syms=run_length(lens_of(257, lit) + [0]), clc_lens=lens_of(19, {0: 2, 1: 2, 18: 2}))
    out.append(s.invalid(1, ERR_INCOMPLETE))
    assert len(set(v.name for v in out)) == len(out) and all(v.isize >= 1 for v in out)
    return out


# ---- single-bit damage: no status can be named in advance, but the verdict can -- zlib's ----------------------------------------
Damaged = collections.namedtuple("Damaged", "name stream isize accepted expected")


def damaged_corpus(per_stream=20):
    """Every stream of the two corpora (the very long ones left out) with one bit flipped, `per_stream` times, most flips in the
    first 200 bytes, where the headers are.  accepted: zlib reaches the end of the stream and has made 1 .. 65536 bytes; ISIZE is
    that count then (so the member is a sound one, with other bytes than the original's perhaps), the original's otherwise.
    Bytes the flip left behind the stream's new end are nobody's business: inflate reports them unused, the decoder does not look
    at them (the member's CRC-32 is the check for such a member)."""
    rng = np.random.default_rng(1952)
    out = []
    for e in valid_corpus() + invalid_corpus():
        if len(e.stream) > 20000:
            continue
        isize0 = len(e.expected) if isinstance(e, Valid) else e.isize
        for k in range(per_stream):
            s = bytearray(e.stream)
            at = int(rng.integers(0, min(len(s), 200))) if rng.random() < 0.7 else int(rng.integers(0, len(s)))
            s[at] ^= 1 << int(rng.integers(0, 8))
            d = zlib.decompressobj(-15)
            try:
                got = d.decompress(bytes(s), MAX_ISIZE + 1)
                ok = d.eof and 1 <= len(got) <= MAX_ISIZE
            except zlib.error:
                ok, got = False, b""
            out.append(Damaged("%s/%d" % (e.name, k), bytes(s), len(got) if ok else isize0, ok, got if ok else b""))
    return out


# ---- BGZF members and the host build of the decoder ----------------------------------------------------------------------------------
def bgzf_member(stream, isize, crc):
    assert len(stream) <= MAX_CDATA
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(stream) + 25) + stream +
            struct.pack("<II", crc, isize))


def build_host_decoder(repo, exe, sanitize=True):
    """tests/inflate_core_host.cpp as a stand-alone program (the decoder's source compiled for the host, a chain of one lane)"""
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas"] + (["-fsanitize=address,undefined"] if sanitize else [])
    subprocess.check_call(cmd + [os.path.join(repo, "tests", "inflate_core_host.cpp"), "-o", exe, "-lz"])
    return exe


GUARD, POISON = 64, 0xEE


def run_host_decoder(exe, jobs, workdir):
    """jobs: [(stream, isize, output alignment 0 .. 15, input shift)] -> ([(status, front guard, bytes, back guard)], counters)
    through `inflate_core_host --streams IN OUT`."""
    src, dst = os.path.join(workdir, "streams.in"), os.path.join(workdir, "streams.out")
    with open(src, "wb") as fh:
        fh.write(struct.pack("<I", len(jobs)))
        for stream, isize, align, shift in jobs:
            fh.write(struct.pack("<IIII", len(stream), isize, align, shift) + stream)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    proc = subprocess.run([exe, "--streams", src, dst], capture_output=True, text=True, env=env, timeout=600)
    assert proc.returncode == 0, (proc.stdout + proc.stderr)[-3000:]
    assert "runtime error" not in proc.stderr and "AddressSanitizer" not in proc.stderr, proc.stderr[-3000:]
    words = proc.stdout.split()
    assert words[0] == "streams:" and int(words[1]) == len(jobs), proc.stdout
    counters = dict(stored=int(words[3]), fixed=int(words[5]), dynamic=int(words[7]), long_lit=int(words[9]), long_dist=int(words[13]))
    raw, at, results = open(dst, "rb").read(), 0, []
    for _stream, isize, _align, _shift in jobs:
        status, n = struct.unpack_from("<iI", raw, at)
        assert n == isize + 2 * GUARD
        body = raw[at + 8:at + 8 + n]
        results.append((status, body[:GUARD], body[GUARD:GUARD + isize], body[GUARD + isize:]))
        at += 8 + n
    assert at == len(raw)
    return results, counters


def zlib_verdict(stream, isize):
    """What the reference makes of a stream in a member of this ISIZE -> (accepted, bytes): accepted means that zlib reaches
    the end of the stream inside the data, with nothing unused, having produced exactly ISIZE bytes."""
    d = zlib.decompressobj(-15)
    try:
        got = d.decompress(stream, isize + 1)
    except zlib.error:
        return False, b""
    return d.eof and not d.unused_data and not d.unconsumed_tail and len(got) == isize, got
