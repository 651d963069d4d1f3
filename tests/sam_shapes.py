"""Deterministic SAM window images at the shapes where the SAM front end on the device (xm_strip.hip: S1 - S8 and the gather
G1 - G3 with xm_gather.h) takes another path: every line length from 1 to 1100 bytes (the copy kernel's 8-byte pieces, its 512-byte
trips and its byte tail), lines longer than a 64 KiB chunk, all three terminators of Python's universal newlines, a last line
without one, lines of different lengths in the two files, lines that are not '\t'.join(fields), terminators on every position of
mark_kernel's 16-byte groups, 1 KiB steps, 16 KiB wave quarters and 64 KiB chunks, and windows of more lines than one trip of the
striding kernels takes.  A plain helper module (no tests, no fixtures): tests/test_sam_shapes_cpu.py pins the images and
expected_bins to the oracle, tests/test_strip_shapes_gpu.py and tests/test_strip_boundaries_gpu.py run them through the C ABI.

Seeded NumPy only.  Names are letters and digits; every tag of a generated line is one of AS:i / XS:i / ZS:i / NM:i / YT:Z, so no
optional field holds "AS", "XS", "ZS" or "NM" by accident (the plugins match a tag as a substring of a field, xenomapper.py:186).
What that leaves out -- the fields themselves on the word and load-step grid of S4, tag text where it must not count, value and CIGAR
forms, names on every alignment for S5 / S6, the long-record form of S7 -- is in tests/sam_field_shapes.py."""
import functools
import re

import numpy as np

CHUNK = 1 << 16                       # xm_strip.hip: bytes of text per workgroup of S1 / S3
QUARTER = 1 << 14                     # ... per wave of that workgroup
STEP = 1 << 10                        # ... per wave instruction
GROUP = 16                            # ... per lane

MAX_PLAIN = 1100                      # every line length 1 .. MAX_PLAIN occurs in each file
LONG_LINES = (70 * 1024 + 3, 200 * 1024 + 5)
SHORT_BELOW = 100                     # a shorter line has fewer than 12 fields: a legal record without scores
MIN_RECORDS = 1500
N_RECORDS = 1600
FILLER = (150, 400)
NEWLINES = ("\n", "\r\n", "\r", "mixed")
SCORE_LAYOUTS = ("spread", "all_unresolved")
ODD_FORMS = ("double_tab", "space", "leading", "trailing", "vt")
ALL = 0b111111

_ALNUM = np.frombuffer(b"0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ", dtype=np.uint8)
_BASES = np.frombuffer(b"ACGTN", dtype=np.uint8)
_QUALS = np.frombuffer(bytes(range(0x21, 0x7F)), dtype=np.uint8)
_TERMS = (b"\n", b"\r\n", b"\r")


def files_of_bin(b):
    """Which files a bin prints from (xenomapper.py:332-350, :423-448, :521-550)."""
    return (0, 1) if b == 4 else (1,) if b in (1, 3) else (0,)


def unit_name(u, n):
    """A name of n characters that differs from the names of units u - 1 and u + 1 at every n."""
    base = _ALNUM.shape[0]
    digits = bytes(int(_ALNUM[(u // base**k) % base]) for k in range(min(n, 3)))
    return digits + b"n" * (n - len(digits))


def _short_line(name, size, rng):
    """A record of `size` bytes with fewer than 12 fields: the name and up to nine fillers, single tabs between them."""
    if size == len(name):
        return name
    parts, rem = [name], size - len(name)
    assert rem >= 2
    while rem > 0:
        take = rem - 1
        if len(parts) < 10 and rem > 4:
            take = int(rng.integers(1, min(rem - 1, 12) + 1))
            if rem - 1 - take == 1:                 # (never a lone tab behind the last field)
                take += 1
        parts.append(_ALNUM[rng.integers(0, _ALNUM.shape[0], size=take)].tobytes())
        rem -= take + 1
    line = b"\t".join(parts)
    assert len(line) == size and len(parts) <= 11
    return line


def _full_line(name, mate, pos, cigar, tags, size, rng):
    """A record of `size` bytes with all 11 mandatory fields and `tags`; SEQ and QUAL take up what is left."""
    head = [name, b"%d" % (83 + 80 * mate), b"chr1", b"%d" % pos, b"42", cigar, b"=", b"%d" % (pos + 200), b"350"]
    fixed = len(b"\t".join(head + [b"", b""] + tags))
    rem = size - fixed
    assert rem >= 2, (size, fixed)
    seq = _BASES[rng.integers(0, _BASES.shape[0], size=(rem + 1) // 2)].tobytes()
    qual = _QUALS[rng.integers(0, _QUALS.shape[0], size=rem // 2)].tobytes()
    line = b"\t".join(head + [seq, qual] + tags)
    assert len(line) == size
    return line


_CIGARS = (b"%dM", b"3S%dM", b"10M2I%dM", b"5M1D%dM4S", b"*", b"%d=")


def _score_tags(rng, always=False):
    """The optional fields of one line: (as, xs, zs, nm) each None or a value, and a CIGAR.  always: AS and NM are there."""
    a = None if rng.integers(0, 12) == 0 and not always else -int(rng.integers(0, 13))
    x = None if rng.integers(0, 3) == 0 else -int(rng.integers(0, 15))
    z = None if rng.integers(0, 2) == 0 else -int(rng.integers(0, 15))
    nm = None if rng.integers(0, 12) == 0 and not always else int(rng.integers(0, 4))
    cigar = _CIGARS[int(rng.integers(0, len(_CIGARS)))]
    return a, x, z, nm, (cigar % int(rng.integers(1, 151))) if b"%d" in cigar else cigar


def _tag_fields(scores):
    a, x, z, nm, _cigar = scores
    out = []
    if a is not None:
        out.append(b"AS:i:%d" % a)
    if x is not None:
        out.append(b"XS:i:%d" % x)
    if z is not None:
        out.append(b"ZS:i:%d" % z)
    if nm is not None:
        out.append(b"NM:i:%d" % nm)
    return out + [b"YT:Z:CP"]


def make_odd(line, form):
    """`line` (single tabs between its fields) with white space that str.split() drops and '\t'.join() does not put back."""
    tabs = [k for k in range(len(line)) if line[k:k + 1] == b"\t"]
    if form == "double_tab":
        return line[:tabs[2]] + b"\t" + line[tabs[2]:]
    if form == "space":
        return line[:tabs[4]] + b" " + line[tabs[4] + 1:]
    if form == "leading":
        return b" " + line
    if form == "trailing":
        return line + b"\t"
    if form == "vt":
        return line[:tabs[7]] + b"\x0b" + line[tabs[7] + 1:]
    raise ValueError(form)


# the units of odd_lines() that hold a line which is not '\t'.join(fields), with scores that put the unit into one bin in every
# mode: (first unit, bin, file of the odd line, mate of the odd line).  Forms take turns from there on.  In bin 0 the odd line is
# always the unit's FIRST mate (record i - 1), in bin 1 always the second: a gather that looked at record i alone would let bin 0 pass.
ODD_UNITS = ((300, 0, 0, 0), (420, 1, 1, 1))
_BIN_SCORES = {0: ((0, None, None, 0, b"50M"), (None, None, None, None, b"*")),        # primary_specific: file 2 has no score
               1: ((None, None, None, None, b"*"), (0, None, None, 0, b"50M"))}        # secondary_specific


def _lengths(paired, seed, together):
    """Line lengths (without terminator) of every record of both files: each value 1 .. MAX_PLAIN and the two long lines once per
    file, fillers for the rest; a record that is shorter than SHORT_BELOW in one file is an ordinary one in the other, and so is
    its mate -- or, `together`, it is short in both files (of j and 100 - j bytes: neither file has its scores) and its mate
    ordinary."""
    rng = np.random.default_rng(seed)
    out = []
    for f in (0, 1):
        sizes = np.zeros(N_RECORDS, dtype=np.int64)
        for j in range(1, SHORT_BELOW):
            k = 100 - j if together and f else j                       # (file 2's line of j bytes lies where file 1's of k does)
            u = (k - 1) + (0 if together else 100 * f)
            sizes[2 * u + ((k + (0 if together else f)) & 1) if paired else u] = j
        rest = list(range(SHORT_BELOW, MAX_PLAIN + 1)) + list(LONG_LINES)
        free = np.flatnonzero(sizes == 0)
        rest += [int(v) for v in rng.integers(FILLER[0], FILLER[1] + 1, size=free.shape[0] - len(rest))]
        sizes[free] = rng.permutation(np.asarray(rest, dtype=np.int64))
        out.append(sizes)
    return out


@functools.lru_cache(maxsize=None)
def _image(paired, scores, newline, odd, seed):
    assert scores in SCORE_LAYOUTS and newline in NEWLINES
    rng = np.random.default_rng(seed)
    sizes = _lengths(paired, seed + 1, scores == "all_unresolved")
    per = 2 if paired else 1
    forced, odd_at = {}, {}                                            # unit -> bin; (file, record) -> form
    if odd:
        for first, b, f, mate in ODD_UNITS:
            for k, form in enumerate(ODD_FORMS * 2):
                u = first + 3 * k
                forced[u] = b
                odd_at[(f, per * u + (mate if paired else 0))] = form
            forced[first + 40] = b                                     # (an odd line in the file the bin does NOT print: harmless)
            odd_at[(1 - f, per * (first + 40))] = "space"
    lines = [[], []]
    for r in range(N_RECORDS):
        u, mate = (r // 2, r & 1) if paired else (r, 0)
        shortest = min(int(sizes[f][q]) for f in (0, 1) for q in range(per * u, per * u + per))
        n = min(shortest, 6)
        if any(int(sizes[f][q]) == n + 1 for f in (0, 1) for q in range(per * u, per * u + per)):
            n -= 1                                                     # (a line is the name alone or the name, a tab and more)
        assert n >= 1
        name = unit_name(u, n)
        same = _score_tags(rng, True)
        for f in (0, 1):
            size = int(sizes[f][r])
            own = _score_tags(rng)
            if size < SHORT_BELOW:
                line = _short_line(name, size, rng)
            else:
                sc = _BIN_SCORES[forced[u]][f] if u in forced else same if scores == "all_unresolved" else own
                line = _full_line(name, mate, 1000 + r, sc[4], _tag_fields(sc), size, rng)
            if (f, r) in odd_at:
                assert size >= SHORT_BELOW
                line = make_odd(line, odd_at[(f, r)])
            lines[f].append(line)
    texts = []
    for f in (0, 1):
        kinds = rng.integers(0, 3, size=N_RECORDS) if newline == "mixed" else np.full(N_RECORDS, NEWLINES.index(newline))
        if newline == "mixed":
            kinds[:3] = (0, 1, 2)
        parts = []
        for r, line in enumerate(lines[f]):
            parts.append(line)
            if f == 1 or r + 1 < N_RECORDS:                            # file 1's last line has no terminator
                parts.append(_TERMS[int(kinds[r])])
        texts.append(b"".join(parts))
    return texts[0], texts[1], tuple(sorted(odd_at.items()))


def shape_text(paired, scores, newline, seed=7):
    """-> (file 1, file 2): N_RECORDS records in the same order with the same names, mates next to each other under one name.
    scores: `spread` draws every line's tags on its own; `all_unresolved` gives a record the same tags in both files (and its short
    lines to the same records of both), so that every paired unit is `unresolved` in liberal mode but the few without any score."""
    return _image(bool(paired), scores, newline, False, seed)[:2]


def odd_lines(paired, scores="spread", newline="\n", seed=7):
    """shape_text with a sprinkling of lines that are not '\t'.join(fields) -> (file 1, file 2, (((file, record), form), ...)).
    The units of ODD_UNITS hold them (bin 0: first mates only, bin 1: second mates only); their scores put them into ODD_UNITS' bin in every mode."""
    return _image(bool(paired), scores, newline, True, seed)


def split_lines(text):
    """The lines of a window under universal newlines, without their terminators -> (lines, offsets, terminated): offsets of the
    lines' first bytes; terminated: the last line has a terminator."""
    a = np.frombuffer(text, dtype=np.uint8)
    cr, lf = a == 13, a == 10
    second = np.zeros(a.shape[0], dtype=bool)
    second[1:] = lf[1:] & cr[:-1]
    ends = np.flatnonzero(cr | (lf & ~second))
    nxt = ends + 1
    nxt += (nxt < a.shape[0]) & second[np.minimum(nxt, a.shape[0] - 1)]
    starts = np.concatenate(([0], nxt)).astype(np.int64)
    stops = np.concatenate((ends, [a.shape[0]])).astype(np.int64)
    terminated = bool(starts[-1] >= a.shape[0])
    if terminated:
        starts, stops = starts[:-1], stops[:-1]
    return [text[s:e] for s, e in zip(starts.tolist(), stops.tolist())], starts, terminated


_SPLIT_BY_STR_ONLY = re.compile(rb"[\x1c-\x1f]")


def printed(line):
    """A line as the reference prints it: '\t'.join(line.split()) + '\n' (xenomapper.py:103 and the print calls).  bytes.split() and
    str.split() agree on ASCII text but for the separators 0x1C .. 0x1F: a line that holds one goes through str."""
    if _SPLIT_BY_STR_ONLY.search(line) is None:
        return b"\t".join(line.split()) + b"\n"
    return "\t".join(line.decode("ascii").split()).encode("ascii") + b"\n"


def bin_parts(lines1, lines2, idx, off, paired, mask, b):
    """[((bin, file, record), printed line)] of bin b in the order the reference prints them."""
    if not (mask >> b) & 1:
        return []
    lines = (lines1, lines2)
    out = []
    for i in idx[int(off[b]):int(off[b + 1])].tolist():
        for f in files_of_bin(b):
            for r in ((i - 1, i) if paired else (i,)):
                out.append(((b, f, r), printed(lines[f][r])))
    return out


def expected_bins(lines1, lines2, idx, off, paired, mask):
    """The six texts from the rule in include/xenomapper_strip.h, as plain Python: for the units idx[off[b]:off[b + 1]] of every bin b
    with a sink (mask bit b), in that order: primary bins file 1's line(s), secondary bins file 2's, `unresolved` file 1's then
    file 2's; a paired unit is records i - 1 and i; each line as '\t'.join(line.split()) + '\n'.  (bin_parts names the same lines
    one by one; this is its order written as one comprehension, for windows of 600 000 records.)"""
    lines = (lines1, lines2)
    out = []
    for b in range(6):
        units = idx[int(off[b]):int(off[b + 1])].tolist() if (mask >> b) & 1 else []
        files = files_of_bin(b)
        if paired:
            out.append(b"".join([printed(lines[f][r]) for i in units for f in files for r in (i - 1, i)]))
        else:
            out.append(b"".join([printed(lines[f][i]) for i in units for f in files]))
    return out


# ---- terminators on every boundary of S1 - S3 -------------------------------------------------------------------------------------

BOUNDARY_VARIANTS = {                                  # name -> (length, how the text ends)
    "x16": (14 * CHUNK - 16 * 37, "lf"),
    "chunk": (14 * CHUNK, "lf"),
    "chunk-1": (14 * CHUNK - 1, "none"),
    "chunk+1": (14 * CHUNK + 1, "lf"),
    "cr_end": (14 * CHUNK - 16 * 37 + 5, "cr"),
    "cr_end_chunk": (14 * CHUNK, "cr"),
    "cr_first_of_chunk": (14 * CHUNK + 1, "cr"),
    "crlf_across_end": (14 * CHUNK + 1, "crlf"),
}
_KINDS = ("lf", "cr", "crlf")
_GRAINS = (("step", STEP), ("quarter", QUARTER), ("chunk", CHUNK))
_LONG_SPANS = ((7 * CHUNK + 100, 9 * CHUNK + 50), (9 * CHUNK + 60, 12 * CHUNK + 300))     # no terminator inside: > 1 and > 2 chunks


def required_boundary_positions():
    """What boundary_text() has to hold: ("group", kind, p): a terminator of `kind` whose first byte is byte p of a 16-byte group;
    (grain, kind, where): one whose first byte is the last / the first byte of a step, quarter or chunk -- a "\r\n" on `last` lies
    across the boundary -- and a "\r\n" whose '\n' is the last byte ("inside")."""
    need = {("group", kind, p) for kind in _KINDS for p in range(GROUP)}
    for grain, _size in _GRAINS:
        need |= {(grain, kind, where) for kind in _KINDS for where in ("last", "first")}
        need.add((grain, "crlf", "inside"))
    return need


def terminators_of(text):
    """[(offset of the first byte, kind)] of every line terminator of `text`."""
    a = np.frombuffer(text, dtype=np.uint8)
    cr, lf = a == 13, a == 10
    out = []
    for p in np.flatnonzero(cr | lf).tolist():
        if lf[p] and p > 0 and cr[p - 1]:
            continue
        out.append((p, "crlf" if cr[p] and p + 1 < a.shape[0] and lf[p + 1] else "cr" if cr[p] else "lf"))
    return out


def _grain_of(q):
    """The coarsest of step, quarter and chunk that begins at offset q (None: none does, or q is 0)."""
    found = [grain for grain, size in _GRAINS if q and q % size == 0]
    return found[-1] if found else None


def boundary_positions(text):
    """The members of required_boundary_positions()'s universe that `text` holds."""
    have = set()
    for p, kind in terminators_of(text):
        have.add(("group", kind, p % GROUP))
        if _grain_of(p + 1):
            have.add((_grain_of(p + 1), kind, "last"))
        if _grain_of(p):
            have.add((_grain_of(p), kind, "first"))
        if kind == "crlf" and _grain_of(p + 2):
            have.add((_grain_of(p + 2), kind, "inside"))
    return have


def _boundary_plan():
    """(offset, kind) of the terminators boundary_text() places on purpose, in chunks 0 .. 6."""
    plan = []
    for t, kind in enumerate(_KINDS):
        for p in range(GROUP):
            plan.append((64 + (t * GROUP + p) * 48 + p, kind))
    cases = [(kind, -1) for kind in _KINDS] + [(kind, 0) for kind in _KINDS] + [("crlf", -2)]
    steps = [4096 + STEP * c for c in range(7)]
    quarters = [QUARTER, 2 * QUARTER, 3 * QUARTER, 5 * QUARTER, 6 * QUARTER, 7 * QUARTER, 9 * QUARTER]
    chunks = [CHUNK * c for c in range(1, 8)]
    for bounds in (steps, quarters, chunks):
        for at, (kind, d) in zip(bounds, cases):
            plan.append((at + d, kind))
    return sorted(plan)


@functools.lru_cache(maxsize=None)
def boundary_text(variant="x16", seed=11):
    """Single-end text whose every record is named `r`: terminators on every position required_boundary_positions() lists,
    ordinary lines of 2 .. 300 bytes between them, one line longer than a chunk and one longer than two (chunks 8, 10 and 11 hold no
    terminator at all), and an end as BOUNDARY_VARIANTS says: a length that is a multiple of 16, of 65 536, that +- 1, a last
    line without a terminator, a '\r' as the last byte."""
    total, end = BOUNDARY_VARIANTS[variant]
    rng = np.random.default_rng(seed)
    plan = _boundary_plan()
    end_len = {"lf": 1, "cr": 1, "crlf": 2, "none": 0}[end]
    if end_len:
        plan.append((total - end_len, end))
    free_from = _LONG_SPANS[-1][1]
    # ordinary lines in the gaps (not inside the long lines): a terminator needs a byte of line in front of it
    placed, taken = [], 0                                              # taken: first byte behind the previous terminator
    width = {"lf": 1, "cr": 1, "crlf": 2}
    plan.append((_LONG_SPANS[0][0] - 1, "lf"))
    plan.append((_LONG_SPANS[0][1], "cr"))
    plan.append((_LONG_SPANS[1][0] - 2, "crlf"))
    plan.append((_LONG_SPANS[1][1], "lf"))
    plan.sort()
    for at, kind in plan:
        assert at >= taken + 1, (at, kind, taken)
        inside = any(lo <= taken and at <= hi for lo, hi in _LONG_SPANS)
        while not inside and at - taken > 340:
            k = _KINDS[int(rng.integers(0, 3))]
            p = taken + int(rng.integers(2, 300))
            placed.append((p, k))
            taken = p + width[k]
        placed.append((at, kind))
        taken = at + width[kind]
    assert taken <= total and (end != "none" or total - taken >= 1) and taken >= free_from
    text = _ALNUM[rng.integers(0, _ALNUM.shape[0], size=total)].copy()
    start = 0
    for at, kind in placed:
        text[start] = ord("r")
        if at - start >= 2:
            text[start + 1] = 9
        text[at] = 13 if kind != "lf" else 10
        if kind == "crlf":
            text[at + 1] = 10
        start = at + width[kind]
    if start < total:
        text[start] = ord("r")
        if total - start >= 2:
            text[start + 1] = 9
    return text.tobytes()


# ---- windows of more lines than one trip of the striding kernels --------------------------------------------------------------------

_MANY_CIGARS = np.frombuffer(b"9M1I7M2D3S7M4M4M", dtype=np.uint8).reshape(4, 4)
_MANY_TAGS = np.frombuffer(b"ASXSZSNM", dtype=np.uint8).reshape(4, 2)


@functools.lru_cache(maxsize=4)
def many_lines(n=600_000, paired=False, repeats=False, seed=3):
    """-> (file 1, file 2): n complete records of 12 fields and 41 bytes each, LF-terminated, built as one character matrix.  The one
    optional field is AS, XS, ZS or NM in turn with a value that varies along the file, the CIGAR varies, and a few values behind
    line 524 288 are not integers (flagged).  paired: two records per name.  repeats: runs of one to three lines per name, of
    different lengths in the two files (the skipping walk pairs run k of file 1 with run k of file 2)."""
    rng = np.random.default_rng(seed)
    out = []
    for f in (0, 1):
        if repeats:
            ids = np.repeat(np.arange(n, dtype=np.int64), rng.integers(1, 4, size=n))[:n]
        else:
            ids = np.arange(n, dtype=np.int64) // (2 if paired else 1)
        m = np.empty((n, 41), dtype=np.uint8)
        m[:] = np.frombuffer(b"r0000000\t0\tc\t1\t9\t0000\t*\t0\t0\tAC\tF\tAS:i:-0\n", dtype=np.uint8)
        m[:, 1:8] = (ids[:, None] // 10 ** np.arange(6, -1, -1)) % 10 + 48
        k = np.arange(n, dtype=np.int64)
        m[:, 17:21] = _MANY_CIGARS[rng.integers(0, 4, size=n)]
        m[:, 33:35] = _MANY_TAGS[(k + (k >> 9) + f) & 3]
        value = rng.integers(0, 10, size=n)
        m[:, 39] = 48 + value
        m[:, 38] = np.where(rng.integers(0, 2, size=n) == 0, ord("-"), ord("1"))
        m[(m[:, 33] == ord("N")), 38] = ord("1")                      # (an NM is a count)
        for line in (524_288 + 5, 524_288 + 1000 + f, n - 3):
            m[line, 39] = ord("x")
        out.append(m.tobytes())
    return tuple(out)


@functools.lru_cache(maxsize=1)
def tiny_lines(n=4_200_000):
    """-> (file 1, file 2): n single-end records without scores, file 1's of 6, 7 and 8 bytes in turn (the name alone), file 2's the
    same names with one more field."""
    assert n % 3 == 0
    g = np.arange(n // 3, dtype=np.int64)
    digits = (g[:, None] // 10 ** np.arange(6, -1, -1)) % 10 + 48
    m = np.empty((n // 3, 24), dtype=np.uint8)
    m[:, 0], m[:, 7], m[:, 15] = ord("a"), ord("b"), ord("c")
    m[:, 1:6], m[:, 8:14], m[:, 16:23] = digits[:, 2:], digits[:, 1:], digits
    m[:, 6] = m[:, 14] = m[:, 23] = 10
    return m.tobytes(), _tiny_second(m)


def _tiny_second(m):
    """File 2 of tiny_lines: every line of file 1 followed by a tab and `q`."""
    rows = m.shape[0]
    w = np.empty((rows, 30), dtype=np.uint8)
    w[:, 0:6], w[:, 6], w[:, 7], w[:, 8] = m[:, 0:6], 9, ord("q"), 10
    w[:, 9:16], w[:, 16], w[:, 17], w[:, 18] = m[:, 7:14], 9, ord("q"), 10
    w[:, 19:27], w[:, 27], w[:, 28], w[:, 29] = m[:, 15:23], 9, ord("q"), 10
    return w.tobytes()
