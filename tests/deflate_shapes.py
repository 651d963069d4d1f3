"""Payloads for the BGZF encoder (xenomapper_amd/csrc/xm_deflate_core.h), shared by the CPU test (tests/test_deflate_core_host.py:
the core as 64 emulated lanes under ASan / UBSan) and the GPU test (tests/test_deflate_gpu.py).  Pure numpy.

Lengths: fewer bytes than a hash (0 .. 5), fewer than lanes (63 .. 65: segments of 0 or 1 byte), the chunk width of the match phase
(127 .. 129), the longest match (257 .. 261), 4095 .. 4097, the steps of the segment size (64 k - 1, 64 k, 64 k + 1 for k = 16
and, as far as a block may be long, k = 1020), the distance limit (32767 .. 32770) and the longest block (65279, 65280).
"""
import gzip
import os
import struct

import numpy as np

MAX_ISIZE = 65280
LENGTHS = [0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 257, 258, 259, 260, 261, 1023, 1024, 1025, 4095, 4096, 4097,
           32767, 32768, 32769, 32770, 65279, 65280]
PERIODS = list(range(1, 67)) + [127, 128, 129, 130]
PERIOD_LENGTHS = [n for n in LENGTHS if n <= 4097] + [65280]
GENERIC = ("random", "acgtn", "runs", "unit700", "zeros", "one_byte", "no_match")

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAM_FIXTURES = (os.path.join(_GOLDEN, "ref_data", "paired_end_testdata_human.bam"),
                os.path.join(_GOLDEN, "ref_data", "paired_end_testdata_mouse.bam"),
                os.path.join(_GOLDEN, "long_cigar_cg.bam"))


def _de_bruijn(k, n):
    """Every n-gram over k symbols exactly once (cyclically): no match of n bytes anywhere in a prefix."""
    a = [0] * (k * n)
    seq = []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    return np.array(seq, dtype=np.uint8)


_NO_MATCH = None


def no_match(n):
    """16 byte values, no four bytes twice: compressible (4 bits a byte) and yet no match -- an empty distance alphabet."""
    global _NO_MATCH
    if _NO_MATCH is None:
        _NO_MATCH = _de_bruijn(16, 4) + np.uint8(ord("a"))
    assert n <= _NO_MATCH.shape[0]
    return _NO_MATCH[:n].copy()


def generic(rng, kind, n):
    if kind == "random":                                   # incompressible: must come out stored, n + 5 bytes
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "acgtn":
        return rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), n)
    if kind == "runs":                                     # long runs, 10 % interruptions: distance-1 overlaps, length 258
        a = np.full(n, ord("F"), dtype=np.uint8)
        a[rng.random(n) < 0.1] = ord(",")
        return a
    if kind == "unit700":
        unit = rng.integers(0, 256, 700, dtype=np.uint8)
        return np.tile(unit, n // 700 + 1)[:n].copy()
    if kind == "zeros":
        return np.zeros(n, dtype=np.uint8)
    if kind == "one_byte":
        return np.full(n, ord("A"), dtype=np.uint8)
    if kind == "no_match":
        return no_match(n)
    raise ValueError(kind)


def periodic(rng, period, n):
    unit = rng.integers(0, 256, period, dtype=np.uint8)
    return np.tile(unit, n // period + 1)[:n].copy()


def far_repeat(rng):
    """40000 random bytes whose last 3000 repeat the first 3000: a match 37000 back, which must NOT be used."""
    a = rng.integers(0, 256, 40000, dtype=np.uint8)
    a[-3000:] = a[:3000]
    return a


def unit_repeated(rng, unit_len, n=MAX_ISIZE):
    """a unit of 32768 (the farthest distance allowed) or 32769 (one too far) random bytes, repeated"""
    unit = rng.integers(0, 256, unit_len, dtype=np.uint8)
    return np.tile(unit, n // unit_len + 1)[:n].copy()


def fibonacci(rng):
    """22 byte values with Fibonacci frequencies (sum 46367): unrestricted Huffman lengths reach 21 bits"""
    f = [1, 1]
    while len(f) < 22:
        f.append(f[-1] + f[-2])
    assert sum(f) == 46367
    a = np.repeat(np.arange(22, dtype=np.uint8) + np.uint8(ord("A")), f)
    rng.shuffle(a)
    return a


def fibonacci_fenced(rng):
    """The same skew where the parse cannot flatten it.  In `fibonacci` most of the frequent values end up inside matches, and what
    is left of the literals fits 15 bits.  Here 18 byte values with the frequencies 1, 2, 3, 5, 8 ... 4181 (with the end-of-block
    symbol as the other 1 the Huffman tree is one chain, 17 or 18 deep) stand each behind the three base-23 digits of their own
    running number: every four bytes that hold such a value occur once (the digits of j, or of j and j + 1, are among them), so
    it is never inside a match, stays a literal, and the literal / length code is longer than 15 bits until it is limited.
    43776 bytes."""
    f = [1, 2]
    while len(f) < 18:
        f.append(f[-1] + f[-2])
    skew = np.repeat(np.arange(18, dtype=np.uint8) + np.uint8(ord("A")), f)
    rng.shuffle(skew)
    j = np.arange(skew.shape[0])
    digits = np.stack([j % 23, j // 23 % 23, j // 529], axis=1).astype(np.uint8) + np.uint8(100)
    return np.concatenate([digits, skew[:, None]], axis=1).reshape(-1)


def fixture_blocks(path):
    raw = np.frombuffer(gzip.decompress(open(path, "rb").read()), dtype=np.uint8)
    return [raw[i:i + MAX_ISIZE] for i in range(0, raw.shape[0], MAX_ISIZE)]


def all_shapes(seed=20240):
    """-> list of (name, payload): every length x every generic kind, the periods, and the payloads of a size of their own"""
    rng = np.random.default_rng(seed)
    out = []
    for kind in GENERIC:
        for n in LENGTHS:
            out.append(("%s/%d" % (kind, n), generic(rng, kind, n)))
    for period in PERIODS:
        for n in PERIOD_LENGTHS:
            out.append(("period%d/%d" % (period, n), periodic(rng, period, n)))
    out.append(("far_repeat", far_repeat(rng)))
    out.append(("unit32768", unit_repeated(rng, 32768)))
    out.append(("unit32769", unit_repeated(rng, 32769)))
    out.append(("fibonacci", fibonacci(rng)))
    out.append(("fibonacci_fenced", fibonacci_fenced(rng)))
    for path in BAM_FIXTURES:
        for k, b in enumerate(fixture_blocks(path)):
            out.append(("%s/%d" % (os.path.basename(path), k), b))
    return out


def write_blocks(path, payloads):
    """the file tests/deflate_core_host.cpp reads: count, then per block its length and its bytes"""
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(payloads)))
        for p in payloads:
            fh.write(struct.pack("<I", len(p)))
            fh.write(np.ascontiguousarray(p, dtype=np.uint8).tobytes())


def read_streams(path):
    """what `deflate_core_host --emit` wrote: per block the stream's length and its bytes"""
    data = open(path, "rb").read()
    n, = struct.unpack_from("<I", data, 0)
    at, out = 4, []
    for _ in range(n):
        m, = struct.unpack_from("<I", data, at)
        out.append(data[at + 4:at + 4 + m])
        at += 4 + m
    assert at == len(data)
    return out
