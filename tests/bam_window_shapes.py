"""Deterministic BAM windows for the BAM input front end (xm_bamdev.hip: xm_bamdev_run with walk_kernel, scan_kernel, gather_kernel,
parse_kernel, run_start_kernel, run_select_kernel, pair_kernel, and the record-walk epilogue of inflate_kernel in xm_inflate.hip) at the
boundaries of its loops: segments per scan thread, records per carried piece, pieces per walk workgroup, pairs per unit-mask word,
BGZF members that are empty, that begin inside a record or that share the header, windows that end inside a record.  A plain helper
module (no tests, no fixtures): tests/test_bam_window_shapes_cpu.py proves the inputs and the model here without a card,
tests/test_bam_window_boundaries_gpu.py runs them through the C ABI.

A case is a pair of files (record lists that hold the same reads), the member boundaries of either file (any byte of the record stream:
a member holds exactly the bytes between two boundaries, it may begin inside a record and it may be empty), and how many members
either file gets per window; its windows follow from each other by `consumed`, exactly as the file path cuts them.  What a window
must report comes from two independent sources:
  (a) builder_expect: the builder's own knowledge -- names, scores, record offsets, which records are complete in the window;
  (b) host_expect: the host's walk of the same bytes (_host.bam_walk), the host printer's text of its records and _host.Parser.parse
      on that text (whose rules tests/test_host_fuzz.py pins to the reference), consumed mapped back from lines to record offsets --
      what the file path does with a window the device declines."""
import collections
import functools
import struct
import zlib

import numpy as np

from tests import bam_shapes as S
from tests.test_host_fuzz import _bam_image_of
from tests.test_inflate_gpu import bgzf_member

ABSENT = -2**31
LINE_NORMAL, EX_A_SHIFT, EX_X_SHIFT = 0x01, 2, 5
LEVELS = (0, 1, 6, 9, 4)                         # zlib level of member j: LEVELS[(j + shift) % 5] -- stored and dynamic blocks mix
CARRY_SEG, WALK_T, SCAN_T = 128, 64, 1024        # xm_bamdev.hip: records per carried piece, pieces per workgroup, scan threads
BIG = 60000                                      # the large record (bam_shapes.MAX_RECORD is 64 000)
BLOCK_DTYPE = np.dtype([("cdata_off", np.uint64), ("out_off", np.uint64), ("cdata_len", np.uint32), ("isize", np.uint32)])

Rec = collections.namedtuple("Rec", "data name a fa x fx")        # fa / fx: 0, 1 (not an integer), 2 (twice)

E_SMALL = (0, 4, 5, 8, 9, 12, 15)                # bytes behind the name: records of 38 .. 60 bytes
E_A = (0, 4, 5, 8, 9, 12, 20, 33, 47, 60, 75)    # 38 .. 120 bytes


def name_of(u, n):
    """n characters that differ from the names of units u - 1 and u + 1: the hex digits of u, the lowest in front."""
    digits = (b"%08x" % (u & 0xFFFFFFFF))[::-1]
    return (digits * (n // 8 + 1))[:n]


def name_len_of(u):
    return 1 + (u * 5) % 8                       # 1 .. 8 characters: with the NUL, a field of 2 .. 9 bytes


def make_rec(name_field, e, a, x, rng, tags=None, model=None):
    """One record of 36 + len(name_field) + e bytes.  Integer AS / XS fields of type c as far as e has room (e = 0, 5 .. 7: none;
    4, 9 .. 11: AS; else both), the rest a Z field.  tags: the optional fields given as bytes (model: the (a, fa, x, fx) they mean)."""
    if tags is None:
        t = 8 if (e == 8 or e >= 12) else 4 if (e == 4 or 9 <= e <= 11) else 0
        tags = (b"ASc" + struct.pack("<b", a) if t >= 4 else b"") + (b"XSc" + struct.pack("<b", x) if t == 8 else b"")
        model = (a if t >= 4 else ABSENT, 0, x if t == 8 else ABSENT, 0)
    data = S.pack_record(name_field, tags=tags, total=36 + len(name_field) + e, pad_rng=rng)
    return Rec(data, name_field.split(b"\0")[0], *model)


def records(ids, f, extra=E_SMALL, seed=1, sizes=None, big_at=None):
    """The records of file f: record i belongs to unit ids[i] (the name), its scores vary with i and f.  sizes: target sizes taken in
    turn (where the unit's name allows them); big_at: the record that has BIG bytes."""
    rng = np.random.default_rng(seed + 100 * f)
    out = []
    for i, u in enumerate(ids):
        field = name_of(u, name_len_of(u)) + b"\0"
        if big_at is not None and i == big_at:
            e = BIG - 36 - len(field)
        elif sizes is not None:
            e = sizes[(i + 3 * f) % len(sizes)] - 36 - len(field)
            e = e if (e == 0 or e >= 4) else 4 + (i % 3)
        else:
            e = extra[(i * 3 + f * 5 + i // 7) % len(extra)]
        a = -((i * 7 + f * 3) % 100)
        out.append(make_rec(field, e, a, a - 1 - (i + f) % 13, rng))
    return out


def mates(n_records, first=0):
    return [first + i // 2 for i in range(n_records)]


def singles(n_records, first=0):
    return [first + i for i in range(n_records)]


def runs(lengths, first=0):
    return [first + k for k, n in enumerate(lengths) for _ in range(n)]


class File(object):
    """A record stream: head (bytes in front of the first record, in the first member), then the records; cut: the file ends there."""

    def __init__(self, recs, head=b"", cut=None):
        self.recs, self.head = recs, len(head)
        self.off = np.concatenate([[0], np.cumsum([len(r.data) for r in recs], dtype=np.int64)]).astype(np.int64) + len(head)
        self.stream = head + b"".join(r.data for r in recs)
        if cut is not None:
            self.stream = self.stream[:cut]
        self.size = len(self.stream)

    def bounds(self, counts):
        """Member boundaries with counts[j] records in member j (the last member takes what is left, a cut record included)."""
        at = np.cumsum(counts)[:-1]
        assert int(np.sum(counts)) == len(self.recs)
        return [0] + [int(self.off[k]) for k in at] + [self.size]


def spread(total, n, pattern, lo, hi):
    """n counts in lo .. hi that follow `pattern` as far as they can and add up to `total`."""
    out, rem = [], total
    for m in range(n):
        left = n - m - 1
        c = min(max(pattern[m % len(pattern)], rem - hi * left, lo), rem - lo * left, hi)
        out.append(c)
        rem -= c
    assert rem == 0 and all(lo <= c <= hi for c in out), (total, n)
    return out


Part = collections.namedtuple("Part", "file lo mid hi bounds eof skip shift")
# one file's share of a window: carried bytes stream[lo:mid], members between the boundaries `bounds` (mid .. hi), skip bytes of head


def members_of(part):
    """[(member bytes, its inflated bytes)] of a part."""
    out = []
    s = part.file.stream
    for j in range(len(part.bounds) - 1):
        raw = s[part.bounds[j]:part.bounds[j + 1]]
        c = zlib.compressobj(LEVELS[(j + part.shift) % len(LEVELS)], zlib.DEFLATED, -15)
        out.append((bgzf_member(c.compress(raw) + c.flush(), raw), raw))
    return out


def device_input(part, carry_slot=0, carry_off=0):
    """-> (compressed bytes, the dict _ffi.BamDev.run takes) of a part."""
    ms = members_of(part)
    blocks = np.zeros(len(ms), dtype=BLOCK_DTYPE)
    crc = np.zeros(len(ms), dtype=np.uint32)
    at = out = 0
    for j, (m, raw) in enumerate(ms):
        assert len(m) <= 65536 and len(raw) <= 65536
        blocks[j] = (at + 18, out, len(m) - 26, len(raw))
        crc[j] = zlib.crc32(raw)
        at += len(m)
        out += len(raw)
    comp = b"".join(m for m, _raw in ms)
    return comp, {"comp_len": len(comp), "blocks": blocks, "crc": crc, "carry_slot": carry_slot, "carry_off": carry_off,
                  "carry_len": part.mid - part.lo, "eof": part.eof, "skip": part.skip}


def window_bytes(part):
    return part.file.stream[part.lo:part.hi]


def segment_starts(part):
    """Where the device's segments begin, the carried pieces behind the first left out (they are cut at record starts the table of the
    window in front lists): byte 0 of a carried tail, and the first byte of every member that is not empty."""
    out = [0] if part.mid > part.lo else []
    for j in range(len(part.bounds) - 1):
        if part.bounds[j + 1] > part.bounds[j]:
            out.append(part.bounds[j] - part.lo + (part.skip if j == 0 else 0))
    return out


def n_block_segments(part):
    return sum(1 for j in range(len(part.bounds) - 1) if part.bounds[j + 1] > part.bounds[j])


Flags = collections.namedtuple("Flags", "paired skip_repeated keep_halo max_records")


def _pairing(tables, stops, wholes, names, n_rec, flags):
    """The walk of xm_bamdev_run / xmh_parse over the records (or runs) the two windows hold.  tables[f]: what file f can pair (offsets
    in its window), names[f]: their names -> the outcome as a dict."""
    n_launch = min(n_rec[0], n_rec[1], flags.max_records)
    by_runs = flags.skip_repeated and n_launch > 0
    n_can = [len(t) for t in tables] if by_runs else list(n_rec)
    n = min(n_launch, n_can[0], n_can[1])
    mismatch = next((k for k in range(n) if names[0][k] != names[1][k]), -1)
    if mismatch >= 0:
        n = mismatch
    open_run = False
    if by_runs:
        cand = [n_can[f] - 1 for f in (0, 1) if not wholes[f] and n_can[f] - 1 < min(n_launch, n_can[0], n_can[1])]
        if cand and min(cand) < n:
            n, mismatch, open_run = min(cand), -1, True
    ended = mismatch < 0 and not open_run and n < flags.max_records and any(n == n_can[f] and wholes[f] for f in (0, 1))
    starved = mismatch < 0 and not ended and n < flags.max_records
    consumed = []
    for f in (0, 1):
        c = tables[f][n] if n < n_can[f] else stops[f]
        if flags.keep_halo and n > 0 and not ended and mismatch < 0:
            c = tables[f][n - 1]
        consumed.append(int(c))
    return {"n": n, "mismatch_at": mismatch, "ended": ended, "starved": starved, "consumed": tuple(consumed)}


def _refusal(parts, rec_offs, stops):
    """(unaligned, bad_block) of a window from its record chains."""
    unaligned = False
    for f, p in enumerate(parts):
        chain = set(int(v) for v in rec_offs[f]) | {int(stops[f])}
        unaligned |= any(s not in chain for s in segment_starts(p))
    bad = 2 if not unaligned and any(p.eof and stops[f] != p.hi - p.lo for f, p in enumerate(parts)) else 0
    return unaligned, bad


def builder_expect(parts, flags):
    """(a): what a window must report, from what the builder knows about its files."""
    out = {"raw_len": tuple(p.hi - p.lo for p in parts)}
    idx, rec_offs, stops = [], [], []
    for p in parts:
        off = p.file.off
        start = p.lo + (p.skip if p.mid == p.lo else 0)
        i0 = int(np.searchsorted(off, start))
        assert int(off[i0]) == start, "a window begins at a record"
        i1 = max(int(np.searchsorted(off, p.hi, side="right")) - 1, i0)
        # (the size word of the record behind the last complete one may be cut: the chain stops in front of it either way)
        idx.append((i0, i1))
        rec_offs.append((off[i0:i1] - p.lo).astype(np.uint32))
        stops.append(int(off[i1]) - p.lo)
    out["n_rec"] = tuple(len(r) for r in rec_offs)
    out["rec_off"], out["stop"] = rec_offs, tuple(stops)
    out["unaligned"], out["bad_block"] = _refusal(parts, rec_offs, stops)
    if out["unaligned"] or out["bad_block"]:
        return out
    units = []
    for f, p in enumerate(parts):
        i0, i1 = idx[f]
        recs = p.file.recs
        units.append([i for i in range(i0, i1) if not flags.skip_repeated or i == i0 or recs[i].name != recs[i - 1].name])
    wholes = [p.eof and stops[f] == p.hi - p.lo for f, p in enumerate(parts)]
    tables = [[int(p.file.off[i]) - p.lo for i in units[f]] for f, p in enumerate(parts)]
    names = [[p.file.recs[i].name for i in units[f]] for f, p in enumerate(parts)]
    out.update(_pairing(tables, stops, wholes, names, out["n_rec"], flags))
    n = out["n"]
    took = [[p.file.recs[i] for i in units[f][:n]] for f, p in enumerate(parts)]
    out["pair_off"] = [np.asarray(tables[f][:n], dtype=np.uint32) for f in (0, 1)]
    out["cols"] = [np.asarray([getattr(r, key) for r in took[f]], dtype=np.int32) for f in (0, 1) for key in ("a", "x")]
    out["flags"] = [np.asarray([LINE_NORMAL | (r.fa << EX_A_SHIFT) | (r.fx << EX_X_SHIFT) for r in took[f]], dtype=np.uint8) for f in (0, 1)]
    out["bits"] = np.asarray([(1 if k > 0 and names[0][k] == names[0][k - 1] else 0) if flags.paired else 1 for k in range(n)], dtype=np.uint8)
    out["n_exceptions"] = int(np.count_nonzero((out["flags"][0] | out["flags"][1]) & 0x7C)) if n else 0
    return out


@functools.lru_cache(maxsize=None)
def _host_tools():
    from xenomapper_amd import _host
    header = _bam_image_of([], refs=S.REFS, aligned=True)
    return _host, _host.BamReader(np.frombuffer(header, dtype=np.uint8), 1, header_only=True), _host.Parser(2)


def host_expect(parts, flags):
    """(b): the host's reading of the same window bytes -- what the file path does with a window the device declines."""
    _host, reader, parser = _host_tools()
    out = {"raw_len": tuple(p.hi - p.lo for p in parts)}
    raws, recs, stops, texts, loffs = [], [], [], [], []
    for p in parts:
        raw = np.frombuffer(window_bytes(p) + bytes(64), dtype=np.uint8)
        n_raw = p.hi - p.lo
        rec = np.empty(n_raw // 36 + 2, dtype=np.uint32)
        n_rec, stop = _host.bam_walk(raw.ctypes.data, n_raw, p.skip if p.mid == p.lo else 0, rec)
        raws.append(raw), recs.append(rec[:n_rec].copy()), stops.append(stop)
    out["n_rec"] = tuple(len(r) for r in recs)
    out["rec_off"], out["stop"] = recs, tuple(stops)
    out["unaligned"], out["bad_block"] = _refusal(parts, recs, stops)
    if out["unaligned"] or out["bad_block"]:
        return out
    for f, p in enumerate(parts):
        n_rec = len(recs[f])
        text = np.empty(8 * (p.hi - p.lo) + (1 << 12), dtype=np.uint8)
        loff, llen = np.empty(n_rec + 1, dtype=np.uint32), np.empty(n_rec + 1, dtype=np.uint32)
        got = reader.print_records(raws[f].ctypes.data, recs[f].ctypes.data, n_rec, text, loff, llen) if n_rec else 0
        assert got >= 0
        texts.append((text, got)), loffs.append(loff[:n_rec].astype(np.int64))
    wholes = [p.eof and stops[f] == p.hi - p.lo for f, p in enumerate(parts)]
    hb = parser.parse(texts[0][0], 0, texts[0][1], wholes[0], texts[1][0], 0, texts[1][1], wholes[1], _host.SCORE_AS_XS,
                      flags.paired, flags.skip_repeated, flags.keep_halo, flags.max_records)
    n = hb.n
    consumed = []
    for f in (0, 1):
        k = int(np.searchsorted(loffs[f], hb.consumed[f]))
        assert hb.consumed[f] == (int(loffs[f][k]) if k < len(loffs[f]) else texts[f][1])
        consumed.append(int(recs[f][k]) if k < len(recs[f]) else stops[f])
    out.update(n=n, mismatch_at=hb.mismatch_at, ended=hb.ended, starved=hb.starved, consumed=tuple(consumed))
    out["pair_off"] = [recs[f][np.searchsorted(loffs[f], hb.line_off[f][:n].astype(np.int64))] if n else np.zeros(0, np.uint32) for f in (0, 1)]
    # The score columns: the parser's, where the device vouches for a value -- the ONE field that matches the tag is the tag's own
    # integer field (tests/test_bam_gpu.py: expected_from_text, the device's contract); every other value the device leaves to the
    # text rules: ABSENT with the flag that says why, whatever the text rules then read there.
    from tests.test_bam_gpu import expected_from_text
    flagged = {(k, col) for k, col, _kind in hb.exc}
    cols = [np.empty(n, dtype=np.int32) for _ in range(4)]
    lf = [np.full(n, LINE_NORMAL, dtype=np.uint8), np.full(n, LINE_NORMAL, dtype=np.uint8)]
    for f in (0, 1):
        text = texts[f][0]
        for k in range(n):
            lo = int(hb.line_off[f][k])
            line = text[lo:lo + int(hb.line_len[f][k])].tobytes()
            for j, tag in enumerate((b"AS", b"XS")):
                v, flag = expected_from_text(line, tag)
                if flag == 0:
                    assert int(hb.cols[2 * f + j][k]) == v and (k, 2 * f + j) not in flagged, (f, k, line)
                cols[2 * f + j][k] = v
                lf[f][k] |= flag << (EX_A_SHIFT if j == 0 else EX_X_SHIFT)
    out["cols"] = cols
    out["flags"] = lf
    out["bits"] = np.unpackbits(hb.unit_bits.view(np.uint8), bitorder="little")[:n].copy() if n else np.zeros(0, np.uint8)
    out["n_exceptions"] = int(np.count_nonzero((lf[0] | lf[1]) & 0x7C)) if n else 0
    return out


def same_expectation(a, b):
    """None, or the first key in which two expectations differ."""
    if set(a) != set(b):
        return "keys %r" % sorted(set(a) ^ set(b))
    for key in sorted(a):
        x, y = a[key], b[key]
        if isinstance(x, list):
            if len(x) != len(y) or not all(np.array_equal(p, q) for p, q in zip(x, y)):
                return key
        elif isinstance(x, np.ndarray):
            if not np.array_equal(x, y):
                return key
        elif x != y:
            return "%s: %r != %r" % (key, x, y)
    return None


class Case(object):
    """Two files, their member boundaries, and how many members either file gets in window w (budgets[f][w]; the last entry goes on).
    slots: the slot of window w (the last entry goes on; "alt": 0 1 0 1 ..).  windows() cuts the files by `consumed` of model (a)."""

    def __init__(self, name, files, bounds, flags, budgets=None, slots="alt", shift=0, limit=400, eof_at=0):
        """eof_at: the first window that may be told that its files end with it (None: none -- the files go on as far as the caller
        knows)."""
        self.name, self.files, self.bounds, self.flags = name, files, bounds, flags
        self.budgets = budgets or [[len(b)] for b in bounds]
        self.slots, self.shift, self.limit, self.eof_at = slots, shift, limit, eof_at

    def slot_of(self, w):
        return w % 2 if self.slots == "alt" else self.slots[min(w, len(self.slots) - 1)]

    def windows(self):
        """-> [(parts, expectation (a))], until a window ends the walk, is refused or has a mismatch."""
        out = []
        cursor = [0, 0]                              # members handed out
        carry = [0, 0]                               # first byte not consumed
        for w in range(self.limit):
            parts = []
            for f in (0, 1):
                b = self.bounds[f]
                take = self.budgets[f][min(w, len(self.budgets[f]) - 1)]
                c1 = min(cursor[f] + take, len(b) - 1)
                mine = b[cursor[f]:c1 + 1] if c1 > cursor[f] else []
                mid = b[cursor[f]]
                first = w == 0 and cursor[f] == 0
                eof = c1 == len(b) - 1 and self.eof_at is not None and w >= self.eof_at
                parts.append(Part(self.files[f], mid if first else carry[f], mid, b[c1], mine, eof,
                                  self.files[f].head if first and mine else 0, self.shift + cursor[f] + f))
                cursor[f] = c1
            exp = builder_expect(parts, self.flags)
            out.append((parts, exp))
            if exp["unaligned"] or exp["bad_block"] or exp["ended"] or exp["mismatch_at"] >= 0:
                return out
            for f in (0, 1):
                carry[f] = parts[f].lo + exp["consumed"][f]
            if all(cursor[f] == len(self.bounds[f]) - 1 for f in (0, 1)) and self.eof_at is None:
                return out
        raise AssertionError("%s: more than %d windows" % (self.name, self.limit))


@functools.lru_cache(maxsize=None)
def windows_of(case):
    return case.windows()


def pieces_of(part, exp_prev_rec_off, carry_off):
    """How many pieces xm_bamdev_run cuts the carried tail into, from the record table of the window in front."""
    if part.mid == part.lo:
        return 0
    j0 = int(np.searchsorted(exp_prev_rec_off, carry_off))
    assert j0 < len(exp_prev_rec_off) and int(exp_prev_rec_off[j0]) == carry_off
    return 1 + len(range(j0 + CARRY_SEG, len(exp_prev_rec_off), CARRY_SEG))


BIG_FLAGS = Flags(True, False, False, 1 << 20)


# ---- A: segments and the scan ---------------------------------------------------------------------------------------------------
A_SEGMENTS = (1, 2, 3, 1023, 1024, 1025, 2047, 2048, 2049, 3001)
A_EMPTY_AT = (0, 5, 6, 1022, 1023, 1024, 2048)                      # of the 2049-member window: first, two in a row, ..., last
A_CARRIED = [(n, p) for n in (1023, 1024, 1025) for p in (1, 2, 3)]


def _two_files(ids, **kw):
    return [File(records(ids, 0, **kw)), File(records(ids, 1, **kw))]


def _counted(files, n_members, patterns=((1, 2, 3, 2), (3, 2, 1, 2)), lo=1, hi=3):
    return [f.bounds(spread(len(f.recs), n_members, patterns[k], lo, hi)) for k, f in enumerate(files)]


def _with_empty(bounds, at):
    """Member boundaries with an empty member at each listed index of the result."""
    out = list(bounds)
    for k in sorted(at):
        out.insert(k, out[k])
    return out


@functools.lru_cache(maxsize=None)
def case_segments(n_seg):
    paired = n_seg % 2 == 1
    files = _two_files(mates(2 * n_seg) if paired else singles(2 * n_seg), extra=E_A, seed=n_seg)
    return Case("A%d" % n_seg, files, _counted(files, n_seg), Flags(paired, False, False, 1 << 20), shift=n_seg)


@functools.lru_cache(maxsize=None)
def case_empty_members():
    n = 2049 - len(A_EMPTY_AT)
    files = _two_files(mates(2 * n), extra=E_A, seed=77)
    b = _counted(files, n)
    return Case("A-empty", files, [_with_empty(b[0], A_EMPTY_AT), _with_empty(b[1], (3,))], BIG_FLAGS)


@functools.lru_cache(maxsize=None)
def case_skip(which):
    """The header shares the first member with records: skip = 1, or all of the member but a 38-byte record."""
    ids = mates(40)
    ids[0] = ids[1] = 8                               # a name of one character: the first record can have 38 bytes
    recs = [records(ids, f, extra=(0, 4, 8, 12), seed=5) for f in (0, 1)]
    assert len(recs[0][0].data) == 38
    head = b"\xff" if which == "one" else bytes(range(256)) * 3
    files = [File(recs[0], head=head), File(recs[1], head=head[:7])]
    first = [1, 3] if which != "one" else [2, 1]
    bounds = [f.bounds([first[k]] + spread(40 - first[k], 9, (4, 5), 1, 9)) for k, f in enumerate(files)]
    return Case("A-skip-" + which, files, bounds, BIG_FLAGS)


@functools.lru_cache(maxsize=None)
def case_segments_behind_carry(n_seg, pieces):
    """Window 1 leaves file 1 a tail of `pieces` pieces; window 2 holds n_seg block segments per file behind it."""
    tail = CARRY_SEG * (pieces - 1) + 5
    k = 6
    total = k + tail + 2 * n_seg
    total += total % 2
    files = _two_files(mates(total), seed=n_seg + pieces)
    rest = [total - k - tail, total - k]
    bounds = [files[0].bounds(spread(k + tail, 8, (40,), 1, 400) + spread(rest[0], n_seg, (1, 2, 3, 2), 1, 3)),
              files[1].bounds(spread(k, 2, (3,), 1, 5) + spread(rest[1], n_seg, (3, 2, 1, 2), 1, 4))]
    return Case("A%d+%d" % (n_seg, pieces), files, bounds, Flags(True, False, False, 1 << 20), budgets=[[8, n_seg], [2, n_seg]])


# ---- B: the alignment check -----------------------------------------------------------------------------------------------------
B_MOVED = (0, 1, 2, 1022, 1023, 1024, 2047)          # the cut between members b and b + 1 lies inside a record
B_TAIL_CUTS = ("1", "2", "3", "4", "body", "short")


@functools.lru_cache(maxsize=None)
def _b_files():
    files = _two_files(mates(2 * 2049), extra=E_A, seed=41)
    return files, _counted(files, 2049)


@functools.lru_cache(maxsize=None)
def case_moved_cut(b):
    """b None: every member begins with a record."""
    files, bounds = _b_files()
    mine = list(bounds[0])
    if b is not None:
        mine[b + 1] += 7
    return Case("B-cut%s" % b, files, [mine, bounds[1]], BIG_FLAGS)


def large_record(size, name_field):
    """A record above bam_shapes.MAX_RECORD (no BGZF member holds it)."""
    body = struct.pack("<iiBBHHHIiii", 0, 100, len(name_field), 30, 4680, 0, 0, 0, -1, -1, 0) + name_field
    body += b"zpZ" + b"q" * (size - 4 - len(body) - 4) + b"\0"
    return Rec(struct.pack("<I", len(body)) + body, name_field[:-1], ABSENT, 0, ABSENT, 0)


@functools.lru_cache(maxsize=None)
def case_record_across_members():
    ids = singles(9)
    files = _two_files(ids, seed=9)
    recs = list(files[0].recs)
    recs[4] = large_record(70000, name_of(4, name_len_of(4)) + b"\0")
    one = File(recs)
    cut = int(one.off[4]) + 50000
    return Case("B-large", [one, files[1]], [[0, int(one.off[2]), int(one.off[4]), cut, int(one.off[5]), one.size], files[1].bounds([4, 5])],
                Flags(False, False, False, 1 << 20))


@functools.lru_cache(maxsize=None)
def case_cut_tail(where, eof):
    """An aligned window whose last record is cut by the window's end."""
    files = _two_files(mates(24), extra=E_A, seed=13)
    last = files[0].recs[-1]
    keep = {"1": 1, "2": 2, "3": 3, "4": 4, "body": len(last.data) // 2, "short": len(last.data) - 1}[where]
    one = File(files[0].recs, cut=int(files[0].off[23]) + keep)
    bounds = [one.bounds(spread(24, 7, (3, 4), 1, 6)), files[1].bounds(spread(24, 5, (5,), 1, 8))]
    return Case("B-tail-%s-%d" % (where, eof), [one, files[1]], bounds, BIG_FLAGS, eof_at=0 if eof else None)


# ---- C: carried tails -----------------------------------------------------------------------------------------------------------
C_TAILS = (1, 2, 127, 128, 129, 255, 256, 257, CARRY_SEG * WALK_T - 1, CARRY_SEG * WALK_T, CARRY_SEG * WALK_T + 1)


def chunks(total, size):
    return spread(total, -(-total // size), (size,), 1, size) if total else []


@functools.lru_cache(maxsize=None)
def case_tail(r, same_slot=False, mixed=False, last="members"):
    """Window 1 leaves file 1 a tail of r records; window 2 carries it.  last: what window 2 adds -- "members" for both files, "none"
    (both files only carry: file 2 the halo record), "one" (file 1 only carries).  mixed: 38- and 42-byte records and the large one."""
    i = C_TAILS.index(r) if r in C_TAILS else 0
    paired = i % 2 == 0 or last == "none"
    halo = paired                                     # (the last yielded record is carried too)
    k = r + 9 + (r + 9) % 2 if same_slot else 6       # pairs of window 1: the tail must fit in front of itself on the same slot
    t = r - (1 if halo else 0)                        # records file 1 has more in window 1
    more = 10 if last == "members" else 0
    totals = [k + t + more, k + (0 if last == "none" else t + more)]
    n1 = [k + t, k]                                   # records in window 1
    files, bounds, budgets = [], [], []
    for f in (0, 1):
        ids = mates(totals[f]) if paired else singles(totals[f])
        files.append(File(records(ids, f, extra=(0, 4) if mixed else E_SMALL, seed=r, big_at=k + 50 if mixed else None)))
        first = chunks(n1[f], 40 if mixed else 300)
        second = chunks(totals[f] - n1[f], 40 if mixed else 250 - 30 * f)
        bounds.append(files[f].bounds(first + second))
        budgets.append([len(first), max(len(second), 1)])
    return Case("C%d%s%s-%s" % (r, "s" if same_slot else "", "m" if mixed else "", last), files, bounds,
                Flags(paired, False, halo, 1 << 20), budgets=budgets, slots=[0, 0] if same_slot else "alt", shift=r, eof_at=1)


# ---- D: the chain adds up -------------------------------------------------------------------------------------------------------
D_COMBOS = ((1, 1, 0), (1, 0, 0), (0, 0, 0), (1, 1, 1), (0, 0, 1))      # (paired, keep_halo, skip_repeated)
D_MAX_RECORDS = (1 << 20, 1000, 64)
D_RUNS = (1, 2, 3, 129)


@functools.lru_cache(maxsize=None)
def _d_files(paired, skip_repeated):
    if skip_repeated:
        # 2400 runs of 1, 2, 3 and 129 equal names, other lengths in the two files; smaller records, so that a window can hold 1000 runs
        lens = [[129 if k % 300 == 7 + 40 * f else 1 + (k + f + k // 7) % 3 for k in range(2400)] for f in (0, 1)]
        ids = [runs(lens[f]) for f in (0, 1)]
        sizes = tuple(range(38, 81)) + (255, 256, 257)
    else:
        ids = [mates(3000) if paired else singles(3000)] * 2
        sizes = tuple(S.SIZES)
    files = [File(records(ids[f], f, sizes=sizes, seed=60 + paired, big_at=1501 + 2 * f)) for f in (0, 1)]
    bounds = [f.bounds(spread(len(f.recs), len(f.recs) // 4, ((2, 6, 3, 5, 4), (5, 2, 6, 4, 3))[k], 1, 6)) for k, f in enumerate(files)]
    for k, f in enumerate(files):                     # the large record gets a member of its own
        big = 1501 + 2 * k
        bounds[k] = sorted(set(bounds[k]) | {int(f.off[big]), int(f.off[big + 1])})
    return files, bounds


@functools.lru_cache(maxsize=None)
def case_chain(combo, max_records):
    paired, halo, skip = combo
    files, bounds = _d_files(bool(paired), bool(skip))
    if max_records == 1000:                           # windows that hold more than 1000 records (runs): max_records binds
        budgets = [[700, 800, 650], [650, 900, 750]] if skip else [[300, 350, 280], [260, 400, 330]]
    else:                                             # 100 .. 280 records (50 .. 140 runs) a window
        budgets = [[40, 55, 30], [25, 70, 45]]
    return Case("D%d%d%d-%d" % (paired, halo, skip, max_records), files, bounds, Flags(bool(paired), bool(skip), bool(halo), max_records),
                budgets=[b * 200 for b in budgets], limit=600)


def whole_file_expect(case):
    """The model's reading of the two whole files as one window."""
    parts = [Part(f, 0, 0, f.size, [0, f.size], True, f.head, 0) for f in case.files]
    return builder_expect(parts, case.flags._replace(keep_halo=False, max_records=1 << 30)), parts


# ---- E: the pair kernel ---------------------------------------------------------------------------------------------------------
E_PAIRS = (1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097)
E_MISMATCH_AT = (0, 1, 63, 64, 255, 256)             # and n - 1
E_KINDS = ("first", "last", "longer")
E_RUN_LENGTHS = (2, 2, 1, 3, 2, 4, 2, 2, 3, 1, 4, 2)


E_FORCED_RUNS = {62: 4, 254: 3}                     # a run of four across records 63 | 64, one of three across 255 | 256


def e_ids(n):
    """Runs of 1 .. 4 equal names."""
    lens, at, k = [], 0, 0
    while at < n:
        if at in E_FORCED_RUNS:
            want = E_FORCED_RUNS[at]
        else:
            want = E_RUN_LENGTHS[k % len(E_RUN_LENGTHS)]
            k += 1
            nxt = min((p for p in E_FORCED_RUNS if p > at), default=None)
            if nxt is not None and at + want > nxt:
                want = nxt - at
        lens.append(want)
        at += want
    return runs(lens)[:n]


def e_name_field(u, f, j):
    """The name of unit u: a length of bam_shapes.NAME_LEN; in every third unit bytes behind the NUL that differ between the files."""
    n = S.NAME_LEN[u % len(S.NAME_LEN)]
    field = name_of(u, n) + b"\0"
    if u % 3 == 1 and n < 200:
        field += bytes([0x41 + f, 0x30 + j % 10, 0x61 + f]) + b"\0"
    return field


def e_record(u, f, i, rng, name_field=None):
    field = e_name_field(u, f, i) if name_field is None else name_field
    a = -((i * 7 + f * 3) % 100)
    x = a - 1 - (i + f) % 13
    if i % 50 == 7 + f:                               # flagged values: AS that is no integer, XS twice
        tags, model = b"ASA5" + b"XSc" + struct.pack("<b", x), (ABSENT, 1, x, 0)
        return make_rec(field, 8, a, x, rng, tags, model)
    if i % 50 == 31 - f:
        tags, model = b"ASc" + struct.pack("<b", a) + b"XSc\x05XSc\x06", (a, 0, ABSENT, 2)
        return make_rec(field, 12, a, x, rng, tags, model)
    return make_rec(field, (8, 12, 17)[(i + f) % 3], a, x, rng)


@functools.lru_cache(maxsize=None)
def _e_records(n):
    ids = e_ids(n)
    out = []
    for f in (0, 1):
        rng = np.random.default_rng(300 + n + f)
        out.append([e_record(u, f, i, rng) for i, u in enumerate(ids)])
    return ids, out


def e_mismatch_field(field, kind):
    name, rest = field.split(b"\0", 1)
    if kind == "first":
        name = bytes([name[0] ^ 1]) + name[1:]
    elif kind == "last":
        name = name[:-1] + bytes([name[-1] ^ 1])
    else:                                             # one character longer (shorter, where the field is full): an equal prefix
        name = name + name[-1:] if len(name) < 254 else name[:-1]
    return name + b"\0" + rest


@functools.lru_cache(maxsize=None)
def case_pairs(n, mismatches=()):
    """mismatches: ((pair, kind), ..) -- file 2's record there has another name."""
    ids, recs = _e_records(n)
    two = list(recs[1])
    rng = np.random.default_rng(7)
    for k, kind in mismatches:
        two[k] = e_record(ids[k], 1, k, rng, e_mismatch_field(e_name_field(ids[k], 1, k), kind))
    files = [File(recs[0]), File(two)]
    m = max(1, n // 40)
    bounds = [f.bounds(spread(n, m, ((37, 44, 40), (45, 36, 41))[k], 1, 80)) for k, f in enumerate(files)]
    return Case("E%d%s" % (n, "".join("-%d%s" % (k, kind[0]) for k, kind in mismatches)), files, bounds, BIG_FLAGS, shift=n)


def e_cases():
    out = [case_pairs(n) for n in E_PAIRS]
    big = E_PAIRS[-1]
    for j, k in enumerate(E_MISMATCH_AT + (big - 1,)):
        out.append(case_pairs(big, ((k, E_KINDS[j % 3]),)))
    out.append(case_pairs(big, ((256, "last"), (64, "longer"))))
    out.append(case_pairs(big, ((255, "first"), (4000, "last"))))
    for n in E_PAIRS[:-1]:
        out.append(case_pairs(n, ((n - 1, E_KINDS[n % 3]),)))
        if n > 1:
            out.append(case_pairs(n, ((0, E_KINDS[(n + 1) % 3]),)))
    return out


@functools.lru_cache(maxsize=None)
def case_flush_name():
    """Both windows end with a record that is its 254-character name and nothing else."""
    ids = mates(10, first=200)
    files = []
    for f in (0, 1):
        rng = np.random.default_rng(90 + f)
        recs = [make_rec(name_of(u, name_len_of(u)) + b"\0", 8 + 4 * (i % 2), -i - f, -i - 20, rng) for i, u in enumerate(ids[:8])]
        recs += [make_rec(name_of(204, 254) + b"\0", 0, 0, 0, rng), make_rec(name_of(204, 254) + b"\0", 0, 0, 0, rng)]
        files.append(File(recs))
    assert files[0].size == files[1].size
    return Case("E-flush", files, [f.bounds([3, 3, 4]) for f in files], BIG_FLAGS)


# ---- the suspected bug: more record starts than a block's slots hold ----------------------------------------------------------------
def zero_member_parts(where, eof):
    """Aligned members of ordinary records with one member of 4096 zero bytes: the window's last, or in its middle."""
    files = _two_files(mates(24), extra=E_A, seed=17)
    parts = []
    for f, fl in enumerate(files):
        b = fl.bounds(spread(24, 6, (4,), 1, 8))
        if f == 0:
            at = int(fl.off[12]) if where == "middle" else fl.size
            zeros = File.__new__(File)
            zeros.recs, zeros.head, zeros.off = fl.recs, 0, fl.off
            zeros.stream = fl.stream[:at] + bytes(4096) + fl.stream[at:]
            zeros.size = len(zeros.stream)
            k = b.index(at)
            b = b[:k + 1] + [v + 4096 for v in b[k:]]
            fl = zeros
        parts.append(Part(fl, 0, 0, fl.size, b, bool(eof), 0, 0))
    return parts


def short_record_parts(block_size):
    """A file whose last member holds two records of `block_size` < 32 bytes: fewer than its slots, and no alignment records."""
    files = [File(records(mates(24), 0, extra=E_A, seed=19)), File(records(mates(26), 1, extra=E_A, seed=19))]
    parts = []
    for f, fl in enumerate(files):
        b = fl.bounds(spread(len(fl.recs), 6, (4,), 1, 8))
        if f == 0:
            bad = (struct.pack("<I", block_size) + bytes(range(1, block_size + 1))) * 2
            short = File.__new__(File)
            short.recs, short.head, short.off = fl.recs, 0, fl.off
            short.stream = fl.stream + bad
            short.size = len(short.stream)
            b = b + [short.size]
            fl = short
        parts.append(Part(fl, 0, 0, fl.size, b, True, 0, 0))
    return parts


# ---- the cases of each group, and a chain's windows put together ---------------------------------------------------------------------
def a_cases():
    return ([case_segments(n) for n in A_SEGMENTS] + [case_segments_behind_carry(n, p) for n, p in A_CARRIED] +
            [case_empty_members(), case_skip("one"), case_skip("most")])


def b_cases():
    return ([case_moved_cut(b) for b in (None,) + B_MOVED] + [case_record_across_members()] +
            [case_cut_tail(where, eof) for where in B_TAIL_CUTS for eof in (0, 1)])


def c_cases():
    return ([case_tail(r, same_slot=i % 2 == 1) for i, r in enumerate(C_TAILS)] +
            [case_tail(200, mixed=True), case_tail(129, last="none"), case_tail(257, last="one")])


def d_cases():
    return [case_chain(combo, m) for combo in D_COMBOS for m in D_MAX_RECORDS]


def concat_chain(case, windows, outcomes):
    """What the windows of a chain yielded, put together: outcomes[w] has n, cols, flags, bits, pair_off of window w (an expectation or
    what the device gave).  With keep_halo, pair 0 of a window behind the first yielded one must be the last pair yielded before it
    and is dropped.  -> {"n", "cols", "flags", "bits", "pair_off" (offsets in the files), "starts" (where the windows' pairs begin)}"""
    cols, flags, offs, bits, starts = [[] for _ in range(4)], [[], []], [[], []], [], []
    total = 0
    for (parts, _exp), o in zip(windows, outcomes):
        n = o["n"]
        absolute = [o["pair_off"][f].astype(np.int64) + parts[f].lo for f in (0, 1)]
        first = 0
        if case.flags.keep_halo and total > 0 and n > 0:
            assert all(int(absolute[f][0]) == int(offs[f][-1][-1]) for f in (0, 1)), "record 0 of a later window is the halo record"
            first = 1
        starts.append(total)
        for j in range(4):
            cols[j].append(np.asarray(o["cols"][j][first:n]))
        for f in (0, 1):
            flags[f].append(np.asarray(o["flags"][f][first:n]))
            if n > first:
                offs[f].append(absolute[f][first:n])
        bits.append(np.asarray(o["bits"][first:n]))
        total += n - first
    cat = lambda parts, dtype: np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype)      # noqa: E731
    return {"n": total, "cols": [cat(c, np.int32) for c in cols], "flags": [cat(x, np.uint8) for x in flags],
            "pair_off": [cat(x, np.int64) for x in offs], "bits": cat(bits, np.uint8), "starts": starts}


def whole_chain_expect(case, windows):
    """What the windows of a chain must add up to: the model's reading of the whole files.  Paired without the halo record, a window
    cannot know the name in front of its first record: that pair's unit bit is 0 whatever the whole file says."""
    exp, _parts = whole_file_expect(case)
    want = {key: exp[key] for key in ("n", "cols", "flags", "bits")}
    want["pair_off"] = [x.astype(np.int64) for x in exp["pair_off"]]
    if case.flags.paired and not case.flags.keep_halo:
        at = 0
        bits = want["bits"].copy()
        for _parts, e in windows:
            if at < len(bits):
                bits[at] = 0
            at += e["n"]
        want["bits"] = bits
    return want
