"""Deterministic SAM windows on the loop edges of the SAM front end's middle kernels (xm_strip.hip: S4 parse_kernel, S5 start_*,
S6 pair_kernel with same_bytes, S7 cig_scan_kernel / cig_write_kernel) -- what tests/sam_shapes.py leaves out on purpose.  S4 reads
a line in 8-byte words, four words to a 32-byte load step, and carries state from word to word: a tag letter over the word edge, the
open field's hits and its last ':', the split state, a skip path over whole words of a mandatory field.  So every case here places
something on that grid: a line is shifted by a pad record in front of it (a two-field line `P<k>\\tx...`, sized so that the line
begins on a chosen offset; the two files get different offsets), and the claims of a case say, as plain data, which offsets, counts
and forms its text reaches.  tests/test_sam_field_shapes_cpu.py recomputes every claim from the text alone, pins every case to the
oracle and runs the host stripper through the direct check; tests/test_strip_fields_gpu.py runs the catalogue through the C ABI.

A plain helper module (no tests, no fixtures), pure Python.  All windows are whole files (end of file on both sides).  Groups:
grid, not_a_tag, dense, separators, values, cigar, names, stale (all_cases() keeps the two cases of a stale pair next to each
other: the second runs on the slot the first has just used).

A name of length 0 and a line of 0 fields are the same thing, the blank line, which ends the walk: it cannot stand among the names
of 1 .. 70 bytes or the lines of 1 .. 14 fields of one window, so it has windows of its own, separators_end_* (the empty line and
lines of separators only, in one file or both, on every word offset)."""
import functools
import itertools

STEP, WORD = 32, 8                     # xm_strip.hip: bytes per load step of S4, bytes per word
TERMS = {"lf": b"\n", "crlf": b"\r\n", "cr": b"\r"}
SEPARATORS = (9, 11, 12, 28, 29, 30, 31, 32)          # str.split() separators that do not end a line
NOT_SEPARATORS = (0, 1, 8, 14, 27, 0x21, 0x7F)
TAGS = {0: (b"AS", b"XS"), 1: (b"AS", b"ZS"), 2: (b"NM", b"XS")}      # what columns 0 / 1 of a file read in each score mode
GROUPS = ("grid", "not_a_tag", "dense", "separators", "values", "cigar", "names", "stale")

# value text -> must the stripper flag it (it vouches for plain int32 literals of at most 10 digits, never for -2^31)
VALUES = (("0", False), ("-0", False), ("+0", False), ("+7", False), ("007", False), ("2147483647", False), ("2147483648", True),
          ("-2147483647", False), ("-2147483648", True), ("0000000001", False), ("00000000001", True), ("", True), ("-", True),
          ("+", True), ("1.5", True), ("1e2", True), ("inf", True), ("nan", True), ("1_0", True), ("5x", True), ("x", True))
DIFF_AT = (0, 7, 8, 15, 16, 23, 24, 30, 31, 32, 33)                   # same_bytes: both ends of every word of a 32-byte round
RUNS = (1, 2, 3, 57, 1, 1, 63, 64, 63, 1, 1, 255, 256, 257, 65)       # run starts on lines 63, 64, 65, 255, 256, 257, 1025, ...
RUN_LENGTHS = (1, 2, 3, 63, 64, 65, 255, 256, 257)
OP_COUNTS = (0, 1, 253, 254, 255, 256, 257, 600)


class Case(object):
    """name, group, score_mode, paired, skip, windows (two bytes objects), claims (dict of plain data, checked from the text) and
    expect: n (records the walk yields), mismatch (it stops at a name mismatch), flags (sorted (record, column) of the values the
    stripper must decline).  after: the name of the case that runs on the same slot just before (stale pairs)."""
    __slots__ = ("name", "group", "score_mode", "paired", "skip", "windows", "claims", "expect", "after")

    def __init__(self, name, group, windows, score_mode=0, paired=False, skip=False, claims=None, n=None, mismatch=False, flags=(),
                 after=None):
        self.name, self.group, self.windows = name, group, (bytes(windows[0]), bytes(windows[1]))
        self.score_mode, self.paired, self.skip = score_mode, paired, skip
        self.claims = dict(claims or {})
        self.expect = {"n": n, "mismatch": mismatch, "flags": sorted(flags)}
        self.after = after

    def __repr__(self):
        return "Case(%s)" % self.name


def rec(name, opt=(), cigar=b"4M", seq=b"ACGT", qual=b"IIII", rname=b"c"):
    return b"\t".join([name, b"0", rname, b"1", b"9", cigar, b"*", b"0", b"0", seq, qual] + list(opt))


class Win(object):
    """Two windows under construction.  add(l1, l2, at=o): a record whose line begins on offset o modulo `mod` in file 1 and on
    o + shift2 (or at2) in file 2 -- a pad record in front of it in each file takes up the difference; at=None: directly behind
    the line in front.  flags: the columns of this record whose value must be flagged (both files: 0 .. 3)."""

    def __init__(self, term=b"\n", shift2=13, mod=STEP):
        self.term, self.shift2, self.mod = term, shift2, mod
        self.parts, self.len, self.k, self.flags = ([], []), [0, 0], 0, []

    def _put(self, f, line):
        self.parts[f].append(line + self.term)
        self.len[f] += len(line) + len(self.term)

    def add(self, l1, l2=None, at=None, at2=None, flags=()):
        if at is not None:
            name = b"P%d" % self.k
            for f, want in ((0, at), (1, at + self.shift2 if at2 is None else at2)):
                n = (want - self.len[f] - len(name) - 1 - len(self.term)) % self.mod or self.mod
                self._put(f, name + b"\t" + b"x" * n)
                assert self.len[f] % self.mod == want % self.mod
            self.k += 1
        self._put(0, l1)
        self._put(1, l1 if l2 is None else l2)
        self.flags += [(self.k, c) for c in flags]
        self.k += 1
        return self.k - 1

    def windows(self, unterminated=False):
        cut = len(self.term) if unterminated else 0
        return tuple(b"".join(p)[:len(b"".join(p)) - cut] for p in self.parts)


# ---- grid ------------------------------------------------------------------------------------------------------------------------
GRID_VALUES = ("7",) + tuple("-" + "1234567890"[:n - 1] for n in range(2, 12))      # value lengths 1 .. 11, all plain int32


UNTERMINATED_TEMPLATES = (40, 13, 26, 7)           # of grid_templates(): one of each form


def grid_templates(mode):
    """The optional fields of the grid lines: tag in field 11 and in a later field, tag / ':' / value far enough apart to lie in
    three words, the value directly in front of the line's end and not."""
    t0, t1 = TAGS[mode]
    q = b"q" * 9
    out = []
    for i, v in enumerate(GRID_VALUES):
        v, w = v.encode(), GRID_VALUES[(i + 5) % 11].encode()
        out.append([t0 + b":i:" + v, t1 + b":i:" + w])
        out.append([b"YT:Z:CP", t1 + b":i:" + v, t0 + b":i:" + w])
        out.append([t0 + q + b":Z" + q + b":" + v])
        out.append([t1 + q + b":Z" + q + b":" + v, b"YT:Z:CP"])
    return out


def _grid_cases():
    for mode in (0, 1, 2):
        tmpl = grid_templates(mode)
        for tname, term in TERMS.items():
            w = Win(term)
            for j, opt in enumerate(tmpl):
                for at in range(STEP):
                    w.add(rec(b"g%02d_%02d" % (j, at), opt), at=at)         # (names of one length: the shift is the line's alone)
            yield Case("grid_m%d_%s" % (mode, tname), "grid", w.windows(), mode, claims={
                "grid_events": ["opt11", "tag0", "tag1", "colon", "val_first", "val_last", "line_end"], "value_lengths": list(range(1, 12)),
                "three_words": True, "files_differ_mod32": True}, n=w.k)
        # the unterminated last line, one to a window: the window's end takes the terminator's place, directly behind a value
        # (of 11, 4 and 7 bytes; tag in field 11, in a later field, tag / ':' / value in three words) and behind another field.
        # Each of these lines on all 32 offsets, so that each of its events, the window's end among them, lies on every one.
        for j in UNTERMINATED_TEMPLATES:
            for at in range(STEP):
                w = Win(b"\n")
                w.add(rec(b"g%02d_%02d" % (j, at), tmpl[j]), at=at)
                yield Case("grid_m%d_unterminated_t%d_%02d" % (mode, j, at), "grid", w.windows(unterminated=True), mode, claims={
                    "unterminated": [j, at], "value_ends_window": j % 4 != 3}, n=w.k)


# ---- not_a_tag -------------------------------------------------------------------------------------------------------------------
def _not_a_tag_cases():
    for mode in (0, 1, 2):
        t0, t1 = TAGS[mode]
        shapes = [t0 + b":i:5", t1, t1 + b":i:1"]
        for tname, term in TERMS.items():
            w = Win(term)
            # tag text as QNAME, as RNAME and inside QUAL, with and without a harmless optional field behind
            for j, (shape, opt) in enumerate(itertools.product(shapes, ([], [b"YT:Z:CP"]))):
                for at in range(j % 4, STEP, 4):
                    w.add(rec(shape, opt), at=at)
                    w.add(rec(b"n%d" % at, opt, rname=shape), at=at + 1)
                    w.add(rec(b"n%d" % at, opt, seq=b"ACGTACGTACGT", qual=b"II" + shape + b"I" * (10 - len(shape))), at=at + 2)
            # QUAL ends in the first letter of a tag on every offset (its last byte on a word edge: its last word is skipped whole),
            # the next field begins with the second letter
            for at in range(STEP):
                for a, b in ((t0[:1], t0[1:]), (t1[:1], t1[1:])):
                    qual = b"II" + t0 + b":i:5IIIIIII" + a
                    w.add(rec(b"q%d" % at, [b + b":i:3", b"YT:Z:CP"], seq=b"A" * len(qual), qual=qual), at=at)
            # an optional field that ends in the first letter, the next begins with the second: the tab on every offset
            for at in range(STEP):
                for a, b in ((t0[:1], t0[1:]), (t1[:1], t1[1:])):
                    w.add(rec(b"s%d" % at, [b"YT:Z:C" + a, b + b":i:1", b"Y" + a, b]), at=at)
            # the same over a line boundary
            for at in range(STEP):
                for a, b in ((t0[:1], t0[1:]), (t1[:1], t1[1:])):
                    w.add(rec(b"l%d" % at, [b"YT:Z:C" + a]), at=at)
                    w.add(rec(b + b"%d" % at, [b + b":i:2", b"YT:Z:CP"]))
            # lines of 1 .. 14 fields with a tag-shaped field at every index (it counts from index 11 on)
            at = 0
            for nf in range(1, 15):
                for idx in range(nf):
                    for shape in (t0 + b":i:5", t1 + b":i:6"):
                        fields = [b"f%d" % i for i in range(nf)]
                        fields[idx] = shape
                        w.add(b"\t".join(fields), at=at)
                        at = (at + 5) % STEP
            yield Case("not_a_tag_m%d_%s" % (mode, tname), "not_a_tag", w.windows(), mode, claims={
                "qual_end_mod8": list(range(8)), "split_tab_mod8": list(range(8)), "split_line_end_mod8": list(range(8)),
                "tag_shaped_index": [[nf, idx] for nf in range(1, 15) for idx in range(nf)]}, n=w.k)


# ---- dense -----------------------------------------------------------------------------------------------------------------------
def _dense_cases():
    tail = b"\t*\t0\t0\tA\tI\tAS:i:1\tXS:i:2\tZS:i:3\tNM:i:1"
    for mode in (0, 1, 2):
        w = Win(b"\n")
        for at in range(STEP):
            w.add(b"a\t0\tc\t1\t9\t2I" + tail, at=at)
            w.add(b"a\t0\tc\t1\t9\t" + b"1M2I" * 12 + tail, at=at)            # a CIGAR of 48 bytes: whole words of it are skipped
            w.add(b"a\t0\tc\t1\t9\t7S" + tail)                                  # (and one directly behind: no pad in front)
            # the fields in front of the CIGAR are operations themselves: a CIGAR that begins at the word's first field start,
            # not at its own, takes them along ("9\t2I" above reads the same from either start)
            w.add(b"a\t0\tc\t5I\t3S\t2I" + tail, at=at)
        yield Case("dense_m%d" % mode, "dense", w.windows(), mode, claims={
            "nth_set": [0, 1, 2, 3], "cigar_whole_words": 5, "operations_in_front_nth": [1, 2]}, n=w.k)


# ---- separators ------------------------------------------------------------------------------------------------------------------
def _separator_cases():
    for mode in (0, 2):
        w = Win(b"\n")
        for b in SEPARATORS + NOT_SEPARATORS:
            c = bytes([b])
            for off in range(WORD):
                for k, head in enumerate((b"r\t0\tc", b"r\t0\tc\t1\t9\t4M\t*\t0\t0\tACGT\tIIII\tYT:Z:CP")):
                    line = head + c + b"d\t1\t9\t4M2S\t*\t0\t0\tACGT\tIIII\tAS:i:-3\tXS:i:-4\tNM:i:1"
                    w.add(line, at=(off + 8 * k - len(head)) % STEP)
        runs = [b"\t" * n for n in range(2, 10)] + [bytes(SEPARATORS[(n + j) % 8] for j in range(n)) for n in range(2, 10)]
        for run in runs:
            for off in range(WORD):
                for k, head in enumerate((b"r\t0\tc", b"r\t0\tc\t1\t9\t4M\t*\t0\t0\tACGT\tIIII\tYT:Z:CP")):
                    line = head + run + b"d\t1\t9\t4M2S\t*\t0\t0\tACGT\tIIII\tAS:i:-3\tXS:i:-4\tNM:i:1"
                    w.add(line, at=(off + 8 * k - len(head)) % STEP)
        body = rec(b"e", [b"AS:i:-1", b"XS:i:-2", b"NM:i:0"])
        for lead, trail in ((b" ", b""), (b"", b"\t"), (b"\t", b"\t"), (b" \t\x0b", b"\x1c \t"), (b"\t" * 9, b" " * 9)):
            for off in range(WORD):
                w.add(lead + body + trail, at=off)
                w.add(lead + body + trail, at=(off - len(lead + body)) % STEP)     # the trailing run on every offset too
        yield Case("separators_m%d" % mode, "separators", w.windows(), mode, claims={
            "byte_mod8": [[b, o] for b in SEPARATORS + NOT_SEPARATORS for o in range(WORD)], "separator_runs": list(range(2, 10)),
            "leading": True, "trailing": True}, n=w.k)
    # what ends the walk: the empty line and lines of separators only, in one file or both, on every word offset
    body = rec(b"e", [b"AS:i:-1", b"XS:i:-2"])
    for j, blank in enumerate((b"", b" ", b" \t\x0b", b"\t" * 9)):
        for off in range(WORD):
            for where in ("both", "first", "second"):
                w = Win((b"\n", b"\r\n", b"\r")[(j + off) % 3], mod=WORD)
                w.add(body, at=off)
                w.add(body)
                k = w.add(blank if where != "second" else body, blank if where != "first" else body, at=off, at2=(off + 3) % WORD)
                w.add(body)
                yield Case("separators_end_%d_%d_%s" % (j, off, where), "separators", w.windows(), paired=bool(off & 1), claims={
                    "blank_line": [len(blank), off, where]}, n=k)


# ---- values ----------------------------------------------------------------------------------------------------------------------
def _value_lines(mode):
    """-> (optional fields, flag on column 0, flag on column 1) of every line of the values window."""
    t0, t1 = TAGS[mode]
    for col, t in enumerate((t0, t1)):
        fl = lambda yes: (yes and col == 0, yes and col == 1)
        first_wins = mode == 2 and col == 0                            # NM: the first matching field, no duplicate rule
        for v, flagged in VALUES:
            yield ([t + b":i:" + v.encode()],) + fl(flagged)
            yield ([b"YT:Z:CP", t + b":i:" + v.encode(), b"YS:i:1"],) + fl(flagged)
        yield ([t + b"5"],) + fl(True)                                 # no colon: the whole field is the value
        yield ([t],) + fl(True)
        yield ([t + b":"],) + fl(True)
        yield ([t + b":A:+"],) + fl(True)
        yield ([t + b":i:4:5"],) + fl(False)                           # what follows the LAST colon
        yield ([b"RG:Z:B" + t + b"S"],) + fl(True)                     # a tag inside a value
        yield ([b"RG:Z:B" + t + b"S", t + b":i:3"],) + fl(True)        # ... and the tag itself: a duplicate (NM: the first wins)
        yield ([t + b":i:3", b"RG:Z:B" + t + b"S"],) + fl(not first_wins)
        yield ([t + b":i:" + t + b":i:4"],) + fl(False)                # the tag twice in one field: one match
        yield ([t, t],) + fl(True)                                     # two matching fields within five bytes
        yield ([t + b":i:1", t + b":i:2"],) + fl(not first_wins)
        yield ([t + b":i:1", b"YT:Z:" + b"q" * 40, t + b":i:2"],) + fl(not first_wins)
        yield ([t + b":i:x", t + b":i:2"],) + fl(True)
    for two in (b"XSAS", b"ZSAS", b"XSNM", b"NMAS", b"ASXS"):          # one field that holds two tags: a value for each
        yield ([two + b":i:3"], False, False)
    yield ([b"XS:i:7", b"ZS:i:8"], False, False)                       # XS beside ZS: one tag each, whichever the mode reads
    yield ([b"ZS:i:8", b"XS:i:x"], False, mode != 1)
    yield ([b"XS:i:7", b"ZS:i:x"], False, mode == 1)


def _value_cases():
    for mode in (0, 1, 2):
        w = Win(b"\n")
        lines = list(_value_lines(mode))
        for j, (opt, f0, f1) in enumerate(lines):
            for off in range(WORD):
                flags = ([0, 2] if f0 else []) + ([1, 3] if f1 else [])
                w.add(rec(b"v%d" % j, opt, cigar=b"3S10M2I"), at=(off + 8 * j) % STEP, flags=flags)
        yield Case("values_m%d" % mode, "values", w.windows(), mode, claims={
            "values": [v for v, _ in VALUES], "line_start_mod8": list(range(8)), "dup_one_word": True, "dup_two_words": True,
            "dup_two_steps": True}, n=w.k, flags=w.flags)


# ---- cigar -----------------------------------------------------------------------------------------------------------------------
def ops_text(n, salt=0):
    """A CIGAR of n operations (lengths 1 .. 3, all nine letters)."""
    return b"".join(b"%d%c" % (1 + (j + salt) % 3, b"MIDNSHP=X"[(j * 2 + salt) % 9]) for j in range(n)) or b"*"


CIGAR_FORMS = ((b"*", False), (b"12", False), (b"M", False), (b"10Q5S", False), (b"10m5s", False), (b"0010S40M", False), (b"0M", False),
               (b"268435455M", False), (b"268435456M", True), (b"268435455S5I", False), (b"5I268435456S", True),
               (b"12345678901234567890M5S", True), (b"5S12345678901234567890", False), (b"5S0000000000000000000007I", False))


def _cigar_cases():
    w = Win(b"\n")
    forms = list(CIGAR_FORMS) + [(ops_text(n), False) for n in OP_COUNTS]
    for j, (cig, big) in enumerate(forms):
        for at in range(j % 3, STEP, 3):
            w.add(rec(b"c%d" % j, [b"NM:i:2", b"XS:i:-1"], cigar=cig), at=at, flags=[0, 2] if big else [])
        w.add(rec(b"c%d" % j, [b"XS:i:-1"], cigar=cig), at=j)                                      # NM missing: nothing to flag
        w.add(rec(b"c%d" % j, [b"NM:i:1.5"], cigar=cig), at=j + 1, flags=[0, 2])                   # NM not a plain integer
    yield Case("cigar_forms", "cigar", w.windows(), 2, claims={"op_counts": list(OP_COUNTS), "forms": [c.decode() for c, _ in CIGAR_FORMS],
                                                               "nm_missing": True, "nm_not_int": True}, n=w.k, flags=w.flags)
    # records of 255 operations or more on both sides of a 256-record tile edge and as the last record, in a window of more than
    # 1024 records (the scan takes two items a thread); no pad records: a record's index is its line's
    for last in (255, 600):
        w = Win(b"\r\n")
        big = {254: 254, 255: 255, 256: 256, 257: 300, 511: 255, 512: 257, 1099: last}
        for k in range(1100):
            cig = ops_text(big.get(k, k % 7), k)
            name = b"t%d" % (k // 2)                                   # paired: every second record closes a unit
            w.add(rec(name, [b"NM:i:%d" % (k % 5), b"XS:i:-3"], cigar=cig), rec(name, [b"NM:i:%d" % (k % 3)], cigar=ops_text(big.get(k + 1, 2), k)))
        yield Case("cigar_tiles_last%d" % last, "cigar", w.windows(), 2, paired=True, claims={
            "records_over": 1024, "long_records_at": [255, 256, 511, 512, 1099], "last_ops": last}, n=w.k)


# ---- names -----------------------------------------------------------------------------------------------------------------------
NAME_LENGTHS = tuple(range(1, 71))


def _name(n, c):
    return ((b"%d" % c)[::-1] + b"n" * n)[:n]


def _variants(n):
    """What the second name of a pair is against the first: equal, one byte different at a position, shorter, longer."""
    out = ["equal"] + [p for p in DIFF_AT if p < n] + [n - 1, "longer", "equal"]
    return out + (["shorter"] if n > 1 else [])


def _aligned(lines, term):
    """lines: (name, filler byte, alignment modulo 8 the NEXT line begins on) -> text: each line is name '\\t' filler...."""
    out, at = [], 0
    for name, fill, nxt in lines:
        n = (nxt - at - len(name) - 1 - len(term)) % WORD or WORD
        out.append(name + b"\t" + fill * n + term)
        at += len(out[-1])
    return b"".join(out)


@functools.lru_cache(maxsize=None)
def _name_pairs():
    """The names of names_units: per length, 64 pairs (A, B); A begins on alignment a in file 1 and b in file 2, B on b and a."""
    names, al = [], ([], [])
    c = 0
    for n in NAME_LENGTHS:
        var = _variants(n)
        for a in range(WORD):
            for b in range(WORD):
                c += 1
                first = _name(n, c)
                v = var[(a * WORD + b) % len(var)]
                if v == "equal":
                    second = first
                elif v == "longer":
                    second = first + b"z"
                elif v == "shorter":
                    second = first[:-1]
                else:
                    second = first[:v] + b"#" + first[v + 1:]
                names += [first, second]
                al[0].extend([a, b])
                al[1].extend([b, a])
    return names, al


def _names_windows(term):
    names, al = _name_pairs()
    out = []
    for f in (0, 1):
        assert al[f][0] == 0
        nxt = al[f][1:] + [0]
        fills = (b"xy", b"wv")[f]                      # the byte behind a name differs from line to line and from file to file
        out.append(_aligned([(nm, fills[k & 1:(k & 1) + 1], nxt[k]) for k, nm in enumerate(names)], term))
    return out


def _names_cases():
    names, _al = _name_pairs()
    runs = len([1 for _k, _g in itertools.groupby(names)])
    claims = {"name_lengths": list(NAME_LENGTHS), "align_pairs": 64, "diff_at": list(DIFF_AT), "diff_last": True, "prefix": True,
              "equal_then_other_byte": True}
    for tname, paired, skip in (("lf", True, False), ("lf", False, True), ("crlf", True, True)):
        yield Case("names_units_%s_%s" % (tname, "skip" if skip else "plain"), "names", _names_windows(TERMS[tname]), 0, paired, skip,
                   claims=claims, n=runs if skip else len(names))
    # a name mismatch between the files: one differing byte at a chosen position, the two names on chosen alignments
    cases = [(70, p) for p in DIFF_AT] + [(70, 69), (32, 31), (33, 32), (64, 63), (65, 64), (1, 0), (8, 7), (9, 8)]
    for j, (n, p) in enumerate(cases):
        for q, (a1, a2) in enumerate(((0, 0), (j % 8, (3 * j + 5) % 8), (7, 1), ((5 * j + 2) % 8, 7))):
            w = Win(b"\n", mod=WORD)
            first = _name(n, 1000 + j)
            w.add(first + b"\t0", at=a2, at2=a1)
            k = w.add(first + b"\t0", first[:p] + b"#" + first[p + 1:] + b"\t0", at=a1, at2=a2)
            w.add(first + b"\t0")
            yield Case("names_mismatch_%d_at%d_%d" % (n, p, q), "names", w.windows(), paired=bool(q & 1), skip=bool(q & 2),
                       claims={"mismatch": [n, p, a1, a2]}, n=k, mismatch=True)
    for j, (l1, l2) in enumerate(((b"abcdefgh", b"abcdefg"), (b"n" * 32, b"n" * 33), (b"n" * 64 + b"\tn", b"n" * 65))):
        w = Win(b"\n", mod=WORD)
        w.add(b"first\t0", at=j)
        k = w.add(l1, l2, at=3 + j, at2=6)
        yield Case("names_prefix_%d" % j, "names", w.windows(), claims={"prefix_mismatch": True}, n=k, mismatch=True)
    # the skipping walk: runs of equal names of different lengths in the two files, run starts on lanes 63 / 64 and on the edges of the
    # 256-line blocks
    for tname, paired in (("lf", False), ("cr", True)):
        text = []
        for f, runs_f in enumerate((RUNS, RUNS[::-1])):
            lines = []
            for r, n in enumerate(runs_f):
                lines += [(b"run%d" % r, b"xw"[f:f + 1], (len(lines) * (3 + 2 * f) + j) % WORD) for j in range(n)]
            text.append(_aligned(lines, TERMS[tname]))
        yield Case("names_runs_%s" % tname, "names", text, 0, paired, True, claims={
            "run_lengths": list(RUN_LENGTHS), "run_starts": [63, 64, 65, 255, 256, 257, 1025], "runs": len(RUNS)}, n=len(RUNS))


# ---- stale -----------------------------------------------------------------------------------------------------------------------
def _stale_cases():
    """First a long window, then on the same slot a short one whose last line has no terminator: the bytes behind its end, left over
    from the long window, continue that line."""
    head = b"".join(rec(b"h%d" % k, [b"AS:i:-%d" % k, b"XS:i:-7", b"NM:i:%d" % k], cigar=b"5M2I3S") + b"\n" for k in range(5))
    more = b"".join(rec(b"m%d" % k, [b"AS:i:-2", b"NM:i:1"]) + b"\n" for k in range(40))
    forms = (("name", b"rdA", b"longername\t0\tc\t1\t9\t4M2I\t*\t0\t0\tA\tI\tAS:i:9\tNM:i:4"),
             ("tag", rec(b"rdB", [b"YT:Z:CP"], cigar=b"4M2I"), b"\tAS:i:9\tXS:i:8\tZS:i:7\tNM:i:4"),
             ("tag_letters", rec(b"rdC", [b"NM:i:1", b"YT:Z:A"], cigar=b"4M2I"), b"S:i:9\tXS:i:8\tZS:i:7"),
             ("value", rec(b"rdD", [b"XS:i:-1", b"ZS:i:-2", b"NM:i:1", b"AS:i:-1"], cigar=b"4M2I"), b"5"),
             ("cigar", b"rdE\t0\tc\t1\t9\t4M2I", b"7D3S\t*\t0\t0\tA\tI\tAS:i:9\tNM:i:4"))
    for mode in (0, 1, 2):
        for what, last, cont in forms:
            for pad in (0, 5, 19):                                       # the end of the short window on different word offsets
                short = b"P\t" + b"x" * (pad + 1) + b"\n" + head + last
                long_ = short + cont + b"\n" + more
                a = "stale_%s_m%d_%d_long" % (what, mode, pad)
                yield Case(a, "stale", (long_, long_), mode, paired=True, claims={"longer_than_next": True}, n=47)
                yield Case(a[:-5] + "_short", "stale", (short, short), mode, paired=True, claims={"continues": cont.decode()}, n=7, after=a)


@functools.lru_cache(maxsize=None)
def _all():
    out = []
    for make in (_grid_cases, _not_a_tag_cases, _dense_cases, _separator_cases, _value_cases, _cigar_cases, _names_cases, _stale_cases):
        out.extend(make())
    return tuple(out)


def all_cases():
    return list(_all())


def cases_of(group):
    return [c for c in _all() if c.group == group]
