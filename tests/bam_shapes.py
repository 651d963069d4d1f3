"""Deterministic BAM images at the shapes where the device SAM printer (xm_bamdev.hip: sam_line / WriteChars / fmt_g_f32) and the
BAM framer (record_to_frames) take another path: every loop's trip boundaries, every base code, top-bit qualities, names with an
early NUL, the integer edges, long CIGARs, every optional-field type, records from 38 bytes to 64 KB next to each other in one
wave.  A plain helper module (no tests, no fixtures): tests/test_bam_shapes_cpu.py pins the host printer to the oracle on these
images and checks that every listed value is really in them; tests/test_bam_shapes_gpu.py runs them through the C ABI.

Every image has three references (a 1-byte and a 70-byte name among them), no record above 64 000 bytes, and no white space in
names, A and Z values.  The letter S is kept out of every generated text, so no optional field can hold "AS" or "XS" by accident
(the plugins match a tag as a substring of a field, xenomapper.py:186)."""
import functools
import struct

import numpy as np

from tests.test_host_fuzz import _bam_image_of

REFS = ("c", "chr12", "k" * 70)
N_REF = len(REFS)
MAX_RECORD = 64000

# printable, no white space, no 'S'
ALPHABET = np.frombuffer(bytes(c for c in range(0x21, 0x7F) if c != ord("S")), dtype=np.uint8)
HEX = np.frombuffer(b"0123456789ABCDEF", dtype=np.uint8)
TAG_LETTERS = "abcdefghijklmnopqrtuvwyz0123456789"                     # (lower case and digits: never AS / XS / ZS / NM)

L_SEQ = [0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 255, 256, 257, 383, 384, 385,
         1000, 4097, 20001]
L_SEQ_LARGE = 42200                                                   # 63 300 bytes of bases and qualities: the record has 63 000 .. 64 000
QUAL_MODES = ("low", "high", "ff")
NAME_LEN = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 254]
NUL_AT = [0, 1, 15, 16, 17, 63]                                       # of a 100-byte name field
N_CIGAR = [0, 1, 2, 8, 255, 256, 1000, 10000]
CIGAR_LEN = [0, 1, 9, 10, 99999999, 2**28 - 1]
POS = [-2**31, -2, -1, 0, 9, 2**31 - 2, 2**31 - 1]
TLEN = [-2**31, -1, 0, 1, 2**31 - 1]
FLAG = [0, 9, 10, 4095, 65535]
MAPQ = [0, 9, 10, 99, 100, 255]
REF_IDS = [-2, -1, 0, 1, 2, 3]
INT_TYPES = {"c": (-2**7, 2**7 - 1), "C": (0, 2**8 - 1), "s": (-2**15, 2**15 - 1), "S": (0, 2**16 - 1), "i": (-2**31, 2**31 - 1),
             "I": (0, 2**32 - 1)}
FMT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}
STRING_LEN = [0, 1, 3, 4, 15, 16, 17, 63, 64, 65, 200, 5000]
B_COUNT = [0, 1, 2, 3, 1000]
SIZES = list(range(38, 81)) + [255, 256, 257, 4095, 4096, 4097]       # (63, 64, 65 are in the range)
MIN_RECORDS = 1500
FILLER_SEQ = (60, 220)                                                # l_seq of a filler record: 150 .. 400 bytes
SCORE_LAYOUTS = ("all_unresolved", "spread")


def int_values(t):
    """Minimum, maximum, 0, -1 and every value at which the decimal text gets a digit longer, of an integer field type."""
    lo, hi = INT_TYPES[t]
    vals = {lo, hi, 0}
    p = 10
    while p - 1 <= hi:
        vals.update(v for v in (p - 1, p) if v <= hi)
        p *= 10
    if lo < 0:
        vals.add(-1)
        p = 10
        while -(p - 1) >= lo:
            vals.update(v for v in (-(p - 1), -p) if v >= lo)
            p *= 10
    return sorted(vals)


def chars(rng, n, alphabet=ALPHABET):
    return alphabet[rng.integers(0, alphabet.shape[0], size=n)].tobytes()


def tag_name(k):
    return (TAG_LETTERS[k % len(TAG_LETTERS)] + TAG_LETTERS[(k // len(TAG_LETTERS)) % len(TAG_LETTERS)]).encode()


def unit_name(u, n, rng):
    """A name of n characters that no other unit has (n == 1: none of its neighbours): the unit's number in front, random behind."""
    if n == 0:
        return b""
    base = ALPHABET.shape[0]
    if n == 1:
        return ALPHABET[u % base:u % base + 1].tobytes()
    digits = bytes(int(ALPHABET[(u // base**k) % base]) for k in range(min(n, 3)))
    return digits + chars(rng, n - len(digits))


def pack_record(name_field, ref=0, pos=100, mapq=30, cigar=(), flag=0, l_seq=0, seq=b"", qual=b"", next_ref=-1, next_pos=-1, tlen=0,
                tags=b"", total=None, pad_rng=None):
    """One alignment record with its block_size word.  total: the size it must have, reached with a Z field in front of `tags`."""
    assert 0 < len(name_field) <= 255 and len(seq) == (l_seq + 1) // 2 and len(qual) == l_seq
    words = np.asarray(cigar, dtype="<u4")
    core = struct.pack("<iiBBHHHIiii", ref, pos, len(name_field), mapq, 4680, words.shape[0], flag, l_seq, next_ref, next_pos, tlen)
    body = core + name_field + words.tobytes() + seq + qual
    if total is not None:
        pad = total - 4 - len(body) - len(tags)
        assert pad == 0 or pad >= 4, (total, len(body), len(tags))
        if pad:
            body += b"zpZ" + chars(pad_rng, pad - 4) + b"\0"
    body += tags
    assert len(body) + 4 <= MAX_RECORD
    return struct.pack("<I", len(body)) + body


def bases(rng, l_seq):
    return rng.integers(0, 256, size=(l_seq + 1) // 2, dtype=np.uint8).tobytes()        # uniform over all 16 codes


def qualities(rng, l_seq, mode="low"):
    """low: 0 .. 93; high: 0 .. 93 and 128 .. 222 (the text is 0x21 .. 0x7E and 0xA1 .. 0xFF); ff: the first byte 0xFF (prints `*`)."""
    if mode == "high":
        q = rng.integers(0, 94 + 95, size=l_seq)
        q[q >= 94] += 128 - 94
    else:
        q = rng.integers(0, 94, size=l_seq)
    if mode == "ff" and l_seq:
        q[0] = 0xFF
    return q.astype(np.uint8).tobytes()


def cigar_words(rng, count, shift):
    """`count` operations: the codes 0 .. 15 in turn, the listed lengths among random ones; never the long-CIGAR placeholder in front."""
    k = np.arange(count, dtype=np.int64)
    code = (k + shift) % 16
    length = rng.integers(1, 2**28, size=count, dtype=np.int64)
    small = rng.integers(0, 3, size=count) > 0
    length[small] = rng.integers(1, 200, size=count)[small]
    listed = (k * 7 + shift) % 3 == 0
    length[listed] = np.asarray(CIGAR_LEN, dtype=np.int64)[((k + shift) // 3) % len(CIGAR_LEN)][listed]
    if count and code[0] == 4:
        code[0] = 5
    return ((length << 4) | code).astype("<u4")


# ---- the records of one file, as specifications: what a record holds apart from its name and its scores ---------------------------

def _ordinary(rng, l_seq=None, mode="low", **over):
    l_seq = int(rng.integers(20, 60)) if l_seq is None else l_seq
    spec = {"ref": int(rng.integers(0, N_REF)), "pos": int(rng.integers(0, 10**6)), "mapq": int(rng.integers(0, 61)),
            "cigar": np.asarray([(l_seq << 4) | 0], dtype="<u4") if l_seq else (), "flag": int(rng.integers(0, 4096)), "l_seq": l_seq,
            "seq": bases(rng, l_seq), "qual": qualities(rng, l_seq, mode), "next_ref": int(rng.integers(-1, N_REF)),
            "next_pos": int(rng.integers(0, 10**6)), "tlen": int(rng.integers(-1000, 1000)), "tags": b"", "scores": True}
    spec.update(over)
    return spec


def _int_field(tag, t, v):
    return tag + t.encode() + struct.pack(FMT[t], v)


def _array_field(rng, tag, sub, count):
    if sub == "f":
        body = rng.integers(0, 2**32, size=count, dtype=np.uint64).astype("<u4")
        body = body[(body & 0x7F800000) != 0x7F800000]                # (NaNs: the float image, with their signs)
        body = np.concatenate([body, np.zeros(count - body.shape[0], dtype="<u4")]).tobytes()
    else:
        lo, hi = INT_TYPES[sub]
        v = rng.integers(lo, hi + 1, size=count, dtype=np.int64)
        v[:2] = (lo, hi)[:count]
        body = v.astype(FMT[sub]).tobytes()
    return tag + b"B" + sub.encode() + struct.pack("<I", count) + body


def mixed_fields(rng, count):
    out = []
    for k in range(count):
        kind = "cCsSiIfAZHB"[k % 11]
        tag = tag_name(100 + k)
        if kind in INT_TYPES:
            out.append(_int_field(tag, kind, int(rng.integers(INT_TYPES[kind][0], INT_TYPES[kind][1] + 1))))
        elif kind == "f":
            out.append(tag + b"f" + struct.pack("<f", float(rng.integers(-1000, 1000)) / 8))
        elif kind == "A":
            out.append(tag + b"A" + chars(rng, 1))
        elif kind in "ZH":
            out.append(tag + kind.encode() + chars(rng, 2 * int(rng.integers(0, 20)), ALPHABET if kind == "Z" else HEX) + b"\0")
        else:
            out.append(_array_field(rng, tag, "cCsSiIf"[k % 7], int(rng.integers(0, 6))))
    return b"".join(out)


def free_specs(seed):
    """The sweeps that take whatever name their place in the file gives them (l_seq, CIGAR, fixed fields, optional fields)."""
    rng = np.random.default_rng(seed)
    out = []
    for mode in QUAL_MODES:
        for l_seq in L_SEQ + [L_SEQ_LARGE]:
            out.append(_ordinary(rng, l_seq, mode))
    for j, count in enumerate(N_CIGAR):
        out.append(_ordinary(rng, cigar=cigar_words(rng, count, j + int(rng.integers(0, 16)))))
    for j, v in enumerate(POS):
        out.append(_ordinary(rng, pos=v, next_pos=POS[(j + 3) % len(POS)]))
    out += [_ordinary(rng, tlen=v) for v in TLEN] + [_ordinary(rng, flag=v) for v in FLAG] + [_ordinary(rng, mapq=v) for v in MAPQ]
    out += [_ordinary(rng, ref=a, next_ref=b) for a in REF_IDS for b in REF_IDS]
    k = 0
    for t in INT_TYPES:
        for v in int_values(t):
            out.append(_ordinary(rng, tags=_int_field(tag_name(k), t, v)))
            k += 1
    for v in (0.5, -3.25, 1e10):
        out.append(_ordinary(rng, tags=tag_name(k) + b"f" + struct.pack("<f", v)))
    out += [_ordinary(rng, tags=tag_name(k) + b"A" + c) for c in (b"!", b"~")]
    for t, alphabet in (("Z", ALPHABET), ("H", HEX)):
        for n in STRING_LEN:
            out.append(_ordinary(rng, tags=tag_name(n) + t.encode() + chars(rng, n, alphabet) + b"\0"))
    for sub in "cCsSiIf":
        for count in B_COUNT:
            out.append(_ordinary(rng, tags=_array_field(rng, tag_name(count), sub, count)))
    out.append(_ordinary(rng, tags=mixed_fields(rng, 40)))
    return out


def placed_specs():
    """The sweeps that decide their unit's name or need a short one (name length, early NUL, record size), and the records without
    scores (no optional field at all; a last field of 1, 2, 4 bytes that ends the record): at the same places in both files."""
    out = [{"name_len": n} for n in NAME_LEN] + [{"nul_at": z} for z in NUL_AT]
    out += [{"total": t} for t in SIZES]
    out += [{"bare": t} for t in ("", "C", "S", "I")]
    return out


def _name_field(spec, u, rng):
    """The name field of unit u (with its NUL), as the placed specification of the unit asks for it."""
    default = b"r%d\0" % u
    if spec is None or "bare" in spec:
        return default
    if "name_len" in spec:
        return unit_name(u, spec["name_len"], rng) + b"\0"
    if "nul_at" in spec:
        z = spec["nul_at"]
        behind = rng.integers(1, 256, size=98 - z, dtype=np.uint8).tobytes()
        return unit_name(u, z, rng) + b"\0" + behind + b"\0"
    t = spec["total"]
    if t - 36 - len(default) >= 4 or t - 36 - len(default) == 0:
        return default
    if t >= 42:
        return unit_name(u, 1, rng) + b"\0"
    return unit_name(u, t - 37, rng) + b"\0"


def _score_fields(rng, a, x):
    out = b""
    for tag, v in ((b"AS", a), (b"XS", x)):
        if v is not None:
            t = "csi"[int(rng.integers(0, 3))]
            out += _int_field(tag, t, v)
    return out


@functools.lru_cache(maxsize=None)
def shape_records(paired, scores, seed=20):
    """-> (records of file 1, records of file 2): the same reads in the same order (mates r0 r0 r1 r1 .. when paired, else a name
    per record), every sweep in both files -- in file 2 with other values, at other places -- between 150 .. 400 byte fillers."""
    assert scores in SCORE_LAYOUTS
    common = np.random.default_rng(seed)
    placed = placed_specs()
    free = [free_specs(seed + 1), free_specs(seed + 2)]
    n = max(MIN_RECORDS, len(placed) + len(free[0]))
    n += n & 1
    while n % 64 == 0:                                                # a ragged last workgroup and a ragged last wave
        n += 2
    units = n // 2 if paired else n
    # where the placed specifications go: a unit each; in a pair, either mate
    chosen = common.permutation(units)[:len(placed)]
    spec_of_unit = {int(u): s for u, s in zip(chosen, placed)}
    place_of_unit = {int(u): (2 * int(u) + int(common.integers(0, 2)) if paired else int(u)) for u in chosen}
    names = [_name_field(spec_of_unit.get(u), u, common) for u in range(units)]
    # the scores of a unit's records: spread -- every kind of unit; all_unresolved -- the same AS on both sides
    kind = common.integers(0, 6, size=units)
    files = []
    for f in (0, 1):
        rng = np.random.default_rng(seed + 10 + f)
        rest = list(free[f])
        while len(placed) + len(rest) < n:
            rest.append(_ordinary(rng, int(rng.integers(*FILLER_SEQ))))
        order = rng.permutation(len(rest))
        rest = [rest[int(k)] for k in order]
        taken = {p: u for u, p in place_of_unit.items()}
        recs = []
        for at in range(n):
            u = at // 2 if paired else at
            if at in taken:
                ps = spec_of_unit[u]
                if "total" in ps:
                    spec = {"scores": False, "tags": b"", "total": ps["total"]}
                elif "bare" in ps:
                    spec = _ordinary(rng, tags=_int_field(b"ze", ps["bare"], INT_TYPES[ps["bare"]][1]) if ps["bare"] else b"", scores=False)
                else:
                    spec = _ordinary(rng)
            else:
                spec = dict(rest.pop())
            sc = b""
            if spec.pop("scores"):
                if scores == "all_unresolved":
                    a = -int((u * 7) % 40)
                    x = a - 1 - int(rng.integers(0, 20))
                else:
                    k = int(kind[u])
                    a = (0, -30, -12, -int(rng.integers(0, 40)), -int(rng.integers(0, 40)), -5)[k] if f == 0 else \
                        (-30, 0, -12, -int(rng.integers(0, 40)), -int(rng.integers(0, 40)), -5)[k]
                    x = (None, a - 3, a, a - 10, None, a + 2)[int(rng.integers(0, 6))]
                    if k == 4 and u % 3 == 0:                         # no score on either side: `unassigned`
                        a = x = None
                sc = _score_fields(rng, a, x)
            spec["tags"] = spec["tags"] + sc
            recs.append(pack_record(names[u], pad_rng=rng, **spec))
        assert not rest
        files.append(recs)
    return files[0], files[1]


# ---- floating-point fields ---------------------------------------------------------------------------------------------------------

FLOATS_PER_RECORD = 2000


@functools.lru_cache(maxsize=None)
def float_patterns(seed=30):
    """The binary32 bit patterns of the float image (a uint32 array; about 77 000)."""
    rng = np.random.default_rng(seed)
    out = []
    low, high = np.arange(8, dtype=np.uint32), np.uint32(0x7FFFFF) - np.arange(8, dtype=np.uint32)
    for ex in range(256):
        for sign in (0, 1):
            mant = np.concatenate([low, high, rng.integers(0, 1 << 23, size=16, dtype=np.uint32)])
            out.append(mant | np.uint32(ex << 23) | np.uint32(sign << 31))
    around = np.arange(999980, 1000021, dtype=np.float64)
    out.append(np.concatenate([around, around + 0.5, around + 0.25]).astype("<f4").view(np.uint32))
    for x in (1e-5, 9.99995e-5, 1e-4, 0.001, 99999.95, 999999.5, 1e6, 1e7, 1e10):
        mid = int(np.array([x], dtype="<f4").view(np.uint32)[0])
        out.append(np.arange(mid - 32, mid + 33, dtype=np.uint32))
    k = np.arange(64, dtype=np.uint32)
    out += [k, np.uint32(0x7FFFFF) - k]                               # subnormals (and + 0)
    out.append(np.array([0, 0x80000000, 0x7F800000, 0xFF800000], dtype=np.uint32))
    nan = np.array([0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0x7FA00000, 0x7FC00001, 0x7F812345, 0x7FD55555, 0x7FBFFFFF], dtype=np.uint32)
    out += [nan, nan | np.uint32(0x80000000)]
    out.append(rng.integers(0, 1 << 32, size=60000, dtype=np.uint64).astype(np.uint32))
    return np.concatenate(out).astype(np.uint32)


def g_text(bits):
    """printf("%g") of the binary32 value with these bits promoted to double, as glibc prints it (a NaN with its sign)."""
    bits = int(bits)
    if (bits & 0x7F800000) == 0x7F800000 and bits & 0x7FFFFF:
        return "-nan" if bits >> 31 else "nan"
    return "%g" % struct.unpack("<f", struct.pack("<I", bits))[0]


@functools.lru_cache(maxsize=None)
def float_records(paired=False, seed=31):
    """-> (records of file 1, of file 2): each with a few scalar f fields and one B:f field of 2 000 values, all patterns of
    float_patterns() in either file (in another order in file 2), the same AS on both sides (every record is `unresolved`)."""
    files = []
    pats = float_patterns()
    n = -(-pats.shape[0] // FLOATS_PER_RECORD)
    n += n & 1
    for f in (0, 1):
        rng = np.random.default_rng(seed + f)
        mine = pats[rng.permutation(pats.shape[0])]
        mine = np.concatenate([mine, rng.integers(0, 1 << 32, size=n * FLOATS_PER_RECORD - mine.shape[0], dtype=np.uint64).astype(np.uint32)])
        recs = []
        for k in range(n):
            vals = mine[k * FLOATS_PER_RECORD:(k + 1) * FLOATS_PER_RECORD].astype("<u4")
            tags = b"".join(tag_name(j) + b"f" + vals[j:j + 1].tobytes() for j in range(3))
            tags += b"fvBf" + struct.pack("<I", vals.shape[0]) + vals.tobytes()
            a = -(k % 30)
            spec = _ordinary(rng, tags=tags + _score_fields(rng, a, a - 4))
            spec.pop("scores")
            recs.append(pack_record(b"f%d\0" % (k // 2 if paired else k), **spec))
        files.append(recs)
    return files[0], files[1]


def image_of(records):
    return _bam_image_of(list(records), refs=REFS, aligned=True)


# ---- reading records back -------------------------------------------------------------------------------------------------------------

def parse(rec):
    """One record (the bytes behind its block_size word) -> its fields; `fields`: (tag, type, subtype or "", value bytes) each."""
    ref, pos, l_name, mapq, _bin, n_cigar, flag, l_seq, next_ref, next_pos, tlen = struct.unpack_from("<iiBBHHHIiii", rec, 0)
    p = 32
    out = {"ref": ref, "pos": pos, "mapq": mapq, "flag": flag, "l_seq": l_seq, "next_ref": next_ref, "next_pos": next_pos, "tlen": tlen,
           "name_field": rec[p:p + l_name], "size": len(rec) + 4}
    p += l_name
    out["cigar"] = np.frombuffer(rec, dtype="<u4", count=n_cigar, offset=p)
    p += 4 * n_cigar
    out["seq"] = rec[p:p + (l_seq + 1) // 2]
    p += (l_seq + 1) // 2
    out["qual"] = rec[p:p + l_seq]
    p += l_seq
    fields = []
    while p < len(rec):
        tag, t = rec[p:p + 2], chr(rec[p + 2])
        p += 3
        sub = ""
        if t in "ZH":
            n = rec.index(b"\0", p) - p
            value, step = rec[p:p + n], n + 1
        elif t == "B":
            sub = chr(rec[p])
            count, = struct.unpack_from("<I", rec, p + 1)
            n = count * struct.calcsize(FMT[sub])
            value, step = rec[p + 5:p + 5 + n], 5 + n
        else:
            n = 1 if t == "A" else struct.calcsize(FMT[t])
            value, step = rec[p:p + n], n
        fields.append((tag, t, sub, value))
        p += step
    assert p == len(rec)
    out["fields"] = fields
    return out


def scores_of(fields):
    """(AS, XS) of a record's own integer fields, None where it has none."""
    got = {}
    for tag, t, _sub, value in fields:
        if tag in (b"AS", b"XS"):
            got[tag], = struct.unpack(FMT[t], value)
    return got.get(b"AS"), got.get(b"XS")


def expected_line(rec, line):
    """The oracle's line of a record with its floating-point values as printf("%g") prints them: the oracle formats with Python's
    %g, which is glibc's text for every value but a NaN, whose sign Python drops."""
    fields = parse(rec)["fields"]
    if not any("f" in (t, sub) for _tag, t, sub, _value in fields):
        return line
    head = line.split("\t")
    n_fixed = 11
    tail = []
    for (tag, t, sub, value), text in zip(fields, head[n_fixed:]):
        if t == "f":
            text = "%s:f:%s" % (tag.decode("latin-1"), g_text(struct.unpack("<I", value)[0]))
        elif t == "B" and sub == "f":
            text = "%s:B:f" % tag.decode("latin-1") + "".join("," + g_text(v) for v in np.frombuffer(value, dtype="<u4"))
        tail.append(text)
    assert len(tail) == len(head) - n_fixed
    return "\t".join(head[:n_fixed] + tail)
