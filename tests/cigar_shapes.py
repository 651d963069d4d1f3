"""Inputs for the CIGAR-score kernels (K1p classify_cigp_kernel: xm_classify_*_cigar_packed_dev; K1c classify_cigar_kernel:
xm_classify_cigar_dev / xm_classify_compact_cigar_dev; K3 cigar_kernel: xm_cigar_scores*), shared by the CPU test
(tests/test_cigar_shapes_cpu.py: the catalogue reaches what it claims, the reference scorer against the C oracle and the
golden) and the GPU test (tests/test_cigar_shapes_gpu.py).  Pure numpy: no torch, no library.

The kernels decide wave-uniformly between a fast op-parallel path (a prefix sum of penalty terms in a per-wave LDS table T,
a record's penalty = T[end] - T[begin]) and careful per-record paths.  The catalogue puts a tile (K1p: 256 records, 8 tiles
per workgroup) or a wave (K1c: 256 records, 4 waves per workgroup) on every value at which one of those decisions flips:

  stretch   ops per tile 0, 1, 255..257, 511..513, 767..769, 1020..1027 at the first and the last tile of a workgroup,
            from small per-record counts and once from a few records of 254 ops
  records   records of 0, 3, 4, 254, 255, 256, 511, 512, 513 ops; escaped records (255 ops or more) at the last record of a
            tile, in front of a workgroup, at record n - 1
  end       the last full tile 9, 8, 7, 6, 0 ops in front of the end of the op array; n a multiple of 2048; K1c's last chunk
            ending at, one below and one above the end of the array; a partial workgroup whose last record begins within
            three words of the end
  oplen     ops of length 2^20 - 1 and 2^20 (own and only over-read from the next tile), 2^24, 2^28 - 1; the largest table
            total; penalties of 2^30 - 1, 2^30, 2^30 + 1 and one above 2^32 (on K1p they need an op of 2^20 or an escaped
            record, which its careful path takes first: 254 ops below 2^20 stop at 799 015 420, so K1p's own test of a
            penalty against 2^30 cannot be reached; K1c's op-parallel path takes the kinds of 402 short ops)
  nm        NM = -2^23 - 1, -2^23, 2^23 - 1, 2^23, small negative values, absent
  range     scores of exactly INT32_MAX, INT32_MAX + 1, INT32_MIN + 1, INT32_MIN
  other     op codes 9..15 with large lengths inside fast tiles
  counts    packed columns only: a tile whose count bytes do not add up to its stretch (unused words behind its records)
  sizes     n = 1, 3, 4, 5, 255..257, 1023..1025, 2047..2049 of ordinary records

Every record is an instance of a named KIND (an op list and an NM); score() is the reference's line 255 in Python integers,
and k1p_model / k1c_model say from the columns alone which path a tile or wave must take.  Each shape sits on species 1 with
species 2 ordinary ("s1"), the other way round ("s2"), and on both species of the same wave ("both": they share the table T).
"""
import zlib

import numpy as np

ABSENT = -2**31
INT32_MAX = 2**31 - 1
TILE = 256
GRAN = 2048                              # K1p's workgroup: 8 tiles
CGRAN = 1024                             # K1c's workgroup: 4 waves
MAX_RECORDS = 6500
M, I, D, N_, S, H_, P_, EQ, X = range(9)  # "MIDNSHP=X"
OP_CHARS = "MIDNSHP=X"

STRETCHES = (0, 1, 255, 256, 257, 511, 512, 513, 767, 768, 769) + tuple(range(1020, 1028))
RECORD_OPS = (0, 3, 4, 254, 255, 256, 511, 512, 513)
END_DISTANCES = (9, 8, 7, 6, 0)             # 6: as far as K1p's widest load reaches past a stretch (W = 8 k + 1: words te .. te + 6)
SIZES = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049)
K1P_CLASSES = ("brief", "one_chunk", "two_chunks", "slow_W", "slow_end", "slow_escape", "slow_long_op", "slow_counts",
               "slow_big", "partial")

# ---- record kinds ------------------------------------------------------------------------------------------------------

KINDS = {}                               # name -> (tuple of (length, op code), NM or ABSENT)
_CYCLE = ((3, I), (7, S), (2, D), (40, M), (1, I), (5, S), (4, D), (9, EQ), (2, X), (6, N_), (3, H_))


def _kind(name, ops, nm):
    assert name not in KINDS
    KINDS[name] = (tuple((int(l), int(c)) for l, c in ops), int(nm))
    return name


def _cycle_ops(count, start):
    return [_CYCLE[(start + k) % len(_CYCLE)] for k in range(count)]


for _c in range(6):                      # ordinary records of 0..5 ops: three present variants and an absent one
    for _v in range(3):
        _kind("o%d%s" % (_c, "abc"[_v]), _cycle_ops(_c, 3 * _v + _c), (_c + _v) % 4)
    _kind("a%d" % _c, _cycle_ops(_c, _c + 1), ABSENT)
for _c in (254, 255, 256, 511, 512, 513):
    _kind("k%d" % _c, _cycle_ops(_c, _c % 7), 2)
for _x, _code in (("i", I), ("d", D), ("s", S)):
    _kind("%s_2p20m1" % _x, [(30, M), (2**20 - 1, _code)], 1)
    _kind("%s_2p20" % _x, [(30, M), (2**20, _code)], 1)
    _kind("%s_2p28m1" % _x, [(2**28 - 1, _code), (3, M)], 0)
_kind("s_2p24", [(2**24, S)], 3)
_kind("i_2p24", [(5, S), (2**24, I)], 0)
_kind("first_2p20", [(2**20, D), (1, I)], 1)                  # its first word is what the tile in front over-reads
_kind("d4max", [(2**20 - 1, D)] * 4, 0)                        # 1023 of these ops: the largest table total, 3 218 081 790
_kind("d3max", [(2**20 - 1, D)] * 3, 0)


def _penalty_kind(name, target, many):
    """A record whose I, D and S ops sum to a penalty of exactly `target`: three long ops (lengths of 2^27 and more), or
    `many` = 400 D ops shorter than 2^20 plus an I and an S (the op-parallel path of K1c takes those)."""
    if many:
        rest = target - 400 * 5 - 5                                # 3 (sum D + i) + 2 s
        s = next(s for s in range(1, 4) if (rest - 2 * s) % 3 == 0)
        total = (rest - 2 * s) // 3
        base = total // 401
        ops = [(base, D)] * 400 + [(total - 400 * base, I), (s, S)]
        assert base < 2**20 and total - 400 * base < 2**20
    else:
        rest = target - 10                                         # 3 (i + d) + 2 s
        s = next(s for s in range(2**27, 2**27 + 3) if (rest - 2 * s) % 3 == 0)
        both = (rest - 2 * s) // 3
        ops = [(s, S), (both // 2, I), (both - both // 2, D)]
    return _kind(name, ops, 0)


for _t, _tag in ((2**30 - 1, "m1"), (2**30, ""), (2**30 + 1, "p1")):
    _penalty_kind("pen_2p30%s" % _tag, _t, False)
    _penalty_kind("pen_2p30%s_many" % _tag, _t, True)
_kind("pen_2p32", [(2**28 - 1, D)] * 7, -2**30)               # penalty 5 637 144 590 > 2^32, score 805 306 354
_kind("nm_m2p23m1", [(50, M), (1, I)], -2**23 - 1)
_kind("nm_m2p23", [(50, M), (1, I)], -2**23)
_kind("nm_2p23m1", [(50, M), (2, S)], 2**23 - 1)
_kind("nm_2p23", [(50, M), (2, S)], 2**23)
_kind("nm_m1", [(50, M)], -1)
_kind("nm_m7", [(3, S), (47, M), (2, D)], -7)
_kind("max_exact", [(0, I)], -357913942)                       # 2147483647
_kind("max_plus1", [(2, S)], -357913942)                       # 2147483648: reported
_kind("min_plus1", [(0, I), (1, S)], 357913940)                # -2147483647
_kind("min_exact", [(1, I)], 357913940)                        # -2147483648 = the absent value: reported
_kind("far_below", [(2**28 - 1, D)] * 3, 2**31 - 1)
_kind("far_above", [], -2**31 + 1)
for _code in range(9, 16):                                     # not CIGAR operations: they score nothing
    _kind("x%d" % _code, [(3, I), (2**20 - 1, _code), (4, S)], 1)
_kind("x12_2p27", [(2**27, 12), (2, D)], 0)
_kind("x15_trailer", [(77, 15)], 2)                            # looks like the trailer word of an escaped record

BINARY_ONLY = frozenset(k for k, (ops, _) in KINDS.items() if any(c > 8 for _, c in ops))
BAD_KINDS = ("max_plus1", "min_exact", "far_below", "far_above")


def exact(kind):
    """-6 NM - 5 (#I + #D) - 3 (sum I + sum D) - 2 sum S in Python integers; None when NM is absent."""
    ops, nm = KINDS[kind]
    if nm == ABSENT:
        return None
    n_gaps = sum(1 for _, c in ops if c in (I, D))
    gaps = sum(l for l, c in ops if c in (I, D))
    clips = sum(l for l, c in ops if c == S)
    return -6 * nm - 5 * n_gaps - 3 * gaps - 2 * clips


def score(kind):
    """(the int32 the score column holds, 1 if the score left int32): absent stays absent; a score of INT32_MIN or below, or
    above INT32_MAX, counts as out of range (INT32_MIN itself is the absent value) and is clamped to INT32_MIN + 1 /
    INT32_MAX, as include/xenomapper_hip.h describes for range_flag."""
    s = exact(kind)
    if s is None:
        return ABSENT, 0
    if s <= ABSENT:
        return ABSENT + 1, 1
    if s > INT32_MAX:
        return INT32_MAX, 1
    return s, 0


def sam_fields(kind):
    """The kind as the fields of a SAM line (op codes 0..8 only)."""
    ops, nm = KINDS[kind]
    assert kind not in BINARY_ONLY
    cigar = "".join("%d%s" % (l, OP_CHARS[c]) for l, c in ops) or "*"
    return [""] * 5 + [cigar] + [""] * 5 + ([] if nm == ABSENT else ["NM:i:%d" % nm])


# ---- columns -----------------------------------------------------------------------------------------------------------

_WORDS = {k: np.array([(l << 4) | c for l, c in ops], dtype=np.uint32) for k, (ops, _) in KINDS.items()}
_SCORES = {k: score(k) for k in KINDS}


def csr_columns(kinds):
    """(nm int32[n], cig_off uint32[n + 1], cig_oplen uint32[]) of a list of kind names."""
    n = len(kinds)
    nm = np.array([KINDS[k][1] for k in kinds], dtype=np.int64).astype(np.int32)
    off = np.zeros(n + 1, dtype=np.uint32)
    np.cumsum([_WORDS[k].shape[0] for k in kinds], out=off[1:])
    ops = np.concatenate([_WORDS[k] for k in kinds] + [np.zeros(0, dtype=np.uint32)]).astype(np.uint32)
    return nm, off, ops


def reference_scores(kinds):
    """(score int32[n], bad) of a list of kind names by score()."""
    out = np.array([_SCORES[k][0] for k in kinds], dtype=np.int64).astype(np.int32)
    return out, sum(_SCORES[k][1] for k in kinds)


def pack_with_slack(off, ops, slack):
    """The packed columns of CSR columns none of whose records has 255 ops or more, with slack[t] unused words behind the
    records of tile t: the count bytes of that tile then add up to less than its stretch."""
    off = off.astype(np.int64)
    n = off.shape[0] - 1
    k = np.diff(off)
    assert (k < 255).all()
    parts, tile, pos = [], [], 0
    for t in range((n + TILE - 1) // TILE):
        a, b = int(off[t * TILE]), int(off[min((t + 1) * TILE, n)])
        tile.append(pos)
        parts += [ops[a:b], np.full(slack.get(t, 0), (9 << 4) | I, dtype=np.uint32)]     # a word that would score if read
        pos += b - a + slack.get(t, 0)
    tile.append(pos)
    return k.astype(np.uint8), np.array(tile, dtype=np.uint32), np.concatenate(parts).astype(np.uint32)


def xs_column(scores, salt):
    """XS that makes the state depend on the exact score: XS = AS or AS - 1, by record and tile; a record without a score
    gets a small negative XS or none."""
    r = np.arange(scores.shape[0], dtype=np.int64)
    s = scores.astype(np.int64)
    low = ((r + r // TILE + salt) & 1) == 1
    xs = np.where(low & (s > ABSENT + 1), s - 1, s)
    none = scores == ABSENT
    xs = np.where(none, np.where(r % 3 == 0, ABSENT, -(r % 50) - 1), xs)
    return xs.astype(np.int32)


def pack_bits(flags):
    flags = np.asarray(flags, dtype=np.uint8)
    padded = np.zeros(max((flags.shape[0] + 63) // 64, 1) * 64, dtype=np.uint8)
    padded[:flags.shape[0]] = flags != 0
    return np.packbits(padded, bitorder="little").view(np.uint64)


class Case(object):
    """name, group, the kind names of both species, slack (packed columns only: {species: {tile: words}}) and what the case
    claims to reach: a list of (kernel "p" or "c", species, tile, {property: value}) the CPU test holds against the models."""

    def __init__(self, name, kinds1, kinds2, claims=(), slack=None):
        assert len(kinds1) == len(kinds2) and len(kinds1) >= 1
        self.name, self.group, self.n = name, name.split("/")[0], len(kinds1)
        self.kinds = (list(kinds1), list(kinds2))
        self.claims = list(claims)
        self.slack = slack or {}
        self._cols = None

    def columns(self):
        """Per species a dict: nm, cig_off, cig_oplen (CSR), score, bad, xs, packed (cnt, tile, ops; None = as
        xm_cigar_pack gives them).  Plus the unit flags of the case.  Built once."""
        if self._cols is None:
            rng = np.random.default_rng(zlib.crc32(self.name.encode()))
            sp = []
            for s in (0, 1):
                nm, off, ops = csr_columns(self.kinds[s])
                sc, bad = reference_scores(self.kinds[s])
                packed = pack_with_slack(off, ops, self.slack[s]) if s in self.slack else None
                sp.append({"nm": nm, "cig_off": off, "cig_oplen": ops, "score": sc, "bad": bad, "xs": xs_column(sc, s),
                           "packed": packed})
            flags = rng.random(self.n) < 0.6
            flags[CGRAN::CGRAN] = True                                # the first record of every later workgroup closes a unit
            self._cols = (sp, flags.astype(np.uint8))
        return self._cols

    @property
    def bad(self):
        sp, _ = self.columns()
        return sp[0]["bad"] + sp[1]["bad"]


# ---- what the kernels' waves see, from the columns alone --------------------------------------------------------------

def _terms(words):
    op, length = (words & 15).astype(np.int64), (words >> 4).astype(np.int64)
    return np.where((op == I) | (op == D), 5 + 3 * length, 0) + np.where(op == S, 2 * length, 0)


def k1p_model(n, nm, cnt, tile, ops):
    """Per tile of packed columns: W, full (the tile lies in a full workgroup), dist (from the stretch's end to the end of the
    op array), cls (one of K1P_CLASSES) and, for slow_long_op, long = "own" or "over" (the long op is only over-read)."""
    n_tiles = (n + TILE - 1) // TILE
    n_ops = int(tile[n_tiles])
    words = ops.astype(np.int64)
    out = []
    for t in range(n_tiles):
        tb, te = int(tile[t]), int(tile[t + 1])
        W = te - tb
        row = {"W": W, "full": (t // 8 + 1) * GRAN <= n, "dist": n_ops - te, "long": None}
        c = cnt[t * TILE:(t + 1) * TILE].astype(np.int64)
        if not row["full"]:
            row["cls"] = "partial"
        elif W >= 1024:
            row["cls"] = "slow_W"
        elif te + 8 > n_ops:
            row["cls"] = "slow_end"
        elif (c == 255).any():
            row["cls"] = "slow_escape"
        elif int(c.sum()) != W:
            row["cls"] = "slow_counts"
        else:
            per = 4 if W < 256 else 8                                # op slots per lane and pass
            seen = set()
            for first in ((0,) if W < 512 else (0, 512)):
                lanes = first + per * np.arange(64)
                for s0 in np.where(lanes < W, lanes, 0):
                    seen.update(range(int(s0), int(s0) + per))
            long_own = bool((words[tb:te] >= 2**24).any())
            long_over = any(words[tb + j] >= 2**24 for j in seen if j >= W)
            begin = np.concatenate([[0], np.cumsum(c)])
            cum = np.concatenate([[0], np.cumsum(_terms(ops[tb:te]))])
            pen = cum[begin[1:]] - cum[begin[:-1]]
            nmv = nm[t * TILE:(t + 1) * TILE].astype(np.int64)
            present = nmv != ABSENT
            big = bool((present & ((nmv < -2**23) | (nmv >= 2**23))).any() or (pen >= 2**30).any())
            if long_own or long_over:
                row["cls"], row["long"] = "slow_long_op", "own" if long_own else "over"
            elif big:
                row["cls"] = "slow_big"
            else:
                row["cls"] = "brief" if W < 256 else "one_chunk" if W < 512 else "two_chunks"
        out.append(row)
    return out


def k1c_model(n, off, ops):
    """Per wave of CSR columns: W, full, chunks and last_checked (the op-parallel path's passes; the last one bounds-checked
    against the end of the array), guard (None = the op-parallel path serves the wave; "partial", "stretch", "many_ops",
    "long_op"), and for the per-record path spec_checked (some lane's three-word load would leave the array) and longer
    (a record with more than three ops)."""
    off = off.astype(np.int64)
    n_ops = int(off[n])
    out = []
    for w in range((n + TILE - 1) // TILE):
        a, b = w * TILE, min((w + 1) * TILE, n)
        base, W = int(off[a]), int(off[b] - off[a])
        k = np.diff(off[a:b + 1])
        row = {"W": W, "full": (w // 4 + 1) * CGRAN <= n, "chunks": None, "last_checked": None, "max_ops": int(k.max())}
        if not row["full"]:
            row["guard"] = "partial"
        elif W >= 1024:
            row["guard"] = "stretch"
        elif (k > 512).any():
            row["guard"] = "many_ops"
        else:
            row["chunks"] = W // 256 + 1
            row["last_checked"] = base + row["chunks"] * 256 > n_ops
            row["last_end"] = base + row["chunks"] * 256 - n_ops      # 0: the last pass ends exactly at the end of the array
            row["guard"] = "long_op" if ((ops[base:base + W] >> 4) >= 2**20).any() else None
        lane_last = off[np.minimum(np.arange(a, a + TILE, 4)[:(b - a + 3) // 4] + 3, n)]     # o[3] of every lane that is there
        row["spec_checked"] = bool((lane_last + 3 > n_ops).any())
        row["longer"] = bool((k > 3).any())
        out.append(row)
    return out


def expected_k1p_class(W):
    return "brief" if W < 256 else "one_chunk" if W < 512 else "two_chunks" if W < 1024 else "slow_W"


# ---- tiles -------------------------------------------------------------------------------------------------------------

def tile_of(W, seed, heavy=0, special=None, size=TILE, absent_every=7):
    """`size` kind names whose op counts add up to W: `special` = {record: kind} as given, `heavy` records of 254 ops, the
    rest ordinary records of counts that differ by one at most (spread over the tile), every absent_every-th without NM."""
    special = dict(special or {})
    for j in range(heavy):
        special[(17 + 71 * j) % size] = "k254"
    rest = W - sum(len(KINDS[k][0]) for k in special.values())
    free = [r for r in range(size) if r not in special]
    assert free and 0 <= rest <= 5 * len(free), (W, rest)
    base, extra = divmod(rest, len(free))
    order = sorted(range(len(free)), key=lambda j: (j * 37) % len(free))
    counts = [base] * len(free)
    for j in order[:extra]:
        counts[j] += 1
    out = [None] * size
    for r, k in special.items():
        out[r] = k
    for j, r in enumerate(free):
        out[r] = "a%d" % counts[j] if absent_every and (r + seed) % absent_every == 0 else "o%d%s" % (counts[j], "abc"[(r + seed) % 3])
    return out


def ordinary(n, seed):
    """n ordinary records of 0..3 ops; every other one has no NM, so that the other species' score alone decides its state."""
    return ["a%d" % ((r + seed) % 2) if r % 2 else "o%d%s" % ((r * 7 + seed) % 4, "abc"[(r + seed) % 3]) for r in range(n)]


def _arranged(name, shape, claims, arr, shape2=None, slack=None):
    """The case with `shape` on species 1 (arr "s1"), species 2 ("s2") or both (shape2 on species 2)."""
    n = len(shape)
    if arr == "s1":
        return Case("%s/s1" % name, shape, ordinary(n, 1), [(k, 0, t, p) for k, t, p in claims], {0: slack} if slack else None)
    if arr == "s2":
        return Case("%s/s2" % name, ordinary(n, 2), shape, [(k, 1, t, p) for k, t, p in claims], {1: slack} if slack else None)
    both = [(k, s, t, p) for k, t, p in claims for s in (0, 1)]
    return Case("%s/both" % name, shape, shape2 if shape2 is not None else shape, both, {0: slack, 1: slack} if slack else None)


def _three(name, build, arrs=("s1", "s2", "both")):
    """build(seed) -> (kinds, claims[, slack]); species 2 of "both" is built with another seed."""
    out = []
    for arr in arrs:
        got = build(5)
        shape, claims, slack = got if len(got) == 3 else got + (None,)
        shape2 = build(11)[0] if arr == "both" else None
        out.append(_arranged(name, shape, claims, arr, shape2, slack))
    return out


def _stretch_claims(t, W):
    return [("p", t, {"W": W, "full": True, "cls": expected_k1p_class(W)}),
            ("c", t, {"W": W, "full": True, "guard": "stretch" if W >= 1024 else None})]


def _stretch():
    """Every stretch length at tile 0 and at tile 7 of a granule (= the first and the last wave of a K1c workgroup as well);
    the tiles between hold further lengths; a ragged tail of ordinary records keeps the last tile's over-read in the array."""
    first, last = list(STRETCHES), list(STRETCHES[7:] + STRETCHES[:7])
    out = []
    for k in range(0, len(STRETCHES), 3):
        def build(seed, k=k):
            kinds, claims = [], []
            for g, j in enumerate(range(k, min(k + 3, len(STRETCHES)))):
                widths = [first[j]] + [STRETCHES[(5 * j + q) % len(STRETCHES)] for q in range(6)] + [last[j]]
                for q, W in enumerate(widths):
                    kinds += tile_of(W, seed + q)
                    claims += _stretch_claims(8 * g + q, W)
            return kinds + tile_of(120, seed, size=77), claims
        out += _three("stretch/k%d" % (k // 3), build)

    def heavy(seed):                                                 # the same lengths from a few records of 254 ops
        kinds, claims = [], []
        for t, W in enumerate([w for w in STRETCHES if w >= 255]):
            kinds += tile_of(W, seed + t, heavy=W // 254)
            claims += _stretch_claims(t, W)
        while len(kinds) % GRAN:
            kinds += tile_of(300, seed)
        return kinds + tile_of(120, seed, size=77), claims
    return out + _three("stretch/heavy254", heavy, arrs=("s1", "both"))


def _records():
    """Records of every listed op count; escaped ones (255 ops and more) at the last record of a tile, at the last record in
    front of a workgroup and at record n - 1."""
    out = []
    for rot in (0, 1):
        esc = ["k255", "k256", "k511", "k512", "k513"]
        esc = esc[rot * 2:] + esc[:rot * 2]

        def build(seed, esc=esc):
            tiles = [tile_of(200, seed + t) for t in range(16)]
            claims = []

            def put(t, r, kind):
                tiles[t] = tile_of(200 + len(KINDS[kind][0]), seed + t, special={r: kind})
                many = len(KINDS[kind][0])
                claims.append(("p", t, {"cls": "slow_escape" if many >= 255 else expected_k1p_class(200 + many), "full": True}))
                claims.append(("c", t, {"guard": "many_ops" if many > 512 else "stretch" if 200 + many >= 1024 else None,
                                        "max_ops": many}))
            put(2, 255, esc[0])                                       # the last record of a tile
            put(5, 255, esc[1])
            put(7, 255, esc[2])                                       # record 2047: in front of workgroup 1 (the halo)
            put(9, 255, esc[3])
            put(11, 255, "k254")                                      # the largest plain count
            put(15, 255, esc[4])                                      # record 4095: in front of the partial workgroup
            tail = tile_of(60 + len(KINDS[esc[0]][0]), seed, size=77, special={76: esc[0]})      # record n - 1
            return [k for t in tiles for k in t] + tail, claims
        out += _three("records/escapes%d" % rot, build)

    def per_record(count):
        def build(seed):
            # a partial workgroup (the per-record paths of both kernels) whose records hold 3 ops at most, but for one
            special = {} if count == 3 else {40: "o%da" % count}
            kinds = tile_of(3 * (100 - len(special)) + (count if special else 0), seed, size=100, special=special, absent_every=0)
            return kinds, [("c", 0, {"guard": "partial", "longer": count > 3, "max_ops": max(count, 3)}),
                           ("p", 0, {"cls": "partial"})]
        return _three("records/tail_max%d" % count, build, arrs=("both",))
    return out + per_record(0) + per_record(3) + per_record(4)


def _end():
    out = []
    for d in END_DISTANCES:                                           # the last full tile ends d ops in front of the end
        def build(seed, d=d):
            kinds = [k for t in range(8) for k in tile_of(150 + 37 * t, seed + t)] + tile_of(d, seed, size=5, absent_every=0)
            W = 150 + 37 * 7
            return kinds, [("p", 7, {"W": W, "dist": d, "full": True, "cls": expected_k1p_class(W) if d >= 8 else "slow_end"}),
                           ("p", 8, {"W": d, "cls": "partial"})]
        out += _three("end/dist%d" % d, build)

    def exact_fit(seed):                                              # n a multiple of 2048: the last tile ends with the array
        kinds = [k for t in range(16) for k in tile_of(90 + 61 * t, seed + t)]
        return kinds, [("p", 15, {"dist": 0, "full": True, "cls": "slow_end"}), ("p", 14, {"full": True, "cls": "two_chunks"}),
                       ("c", 15, {"full": True, "guard": None, "last_checked": True})]
    out += _three("end/exact_fit", exact_fit)
    for tag, tail_ops, end in (("at", 212, 0), ("below", 213, -1), ("above", 211, 1)):
        def build(seed, tail_ops=tail_ops, end=end):                  # K1c: wave 3 holds 300 ops, its second pass ends at base + 512
            kinds = [k for t in range(3) for k in tile_of(333, seed + t)] + tile_of(300, seed) + tile_of(tail_ops, seed, size=100)
            return kinds, [("c", 3, {"W": 300, "full": True, "guard": None, "chunks": 2, "last_end": end, "last_checked": end > 0}),
                           ("c", 0, {"full": True, "guard": None, "last_checked": False})]
        out += _three("end/k1c_chunk_%s" % tag, build, arrs=("s1", "both"))
    for last in range(5):                                             # K1c: a partial workgroup of 4 records; the last one owns `last` ops
        def build(seed, last=last):
            kinds = [k for t in range(4) for k in tile_of(280, seed + t)]
            kinds += ["o2a", "o1b", "o3c", "o%d%s" % (last, "abc"[seed % 3])]
            return kinds, [("c", 4, {"guard": "partial", "spec_checked": last < 3, "longer": last > 3}), ("p", 4, {"cls": "partial"})]
        out += _three("end/k1c_last%d" % last, build, arrs=("both",))
    return out


def _oplen():
    out = []

    def edges(seed):
        """2^20 - 1 keeps a tile fast, 2^20 does not: on I, D and S, in tiles of one pass (4 and 8 slots) and of two."""
        kinds, claims = [], []
        plan = [("i_2p20m1", 100), ("i_2p20", 100), ("d_2p20m1", 300), ("d_2p20", 300), ("s_2p20m1", 700), ("s_2p20", 700),
                ("s_2p24", 90), ("d_2p28m1", 400),
                ("s_2p20m1", 255), ("d_2p20m1", 511), ("i_2p20m1", 1023), ("i_2p28m1", 600), ("s_2p28m1", 10), ("i_2p24", 256),
                ("d_2p20", 1023), ("s_2p20", 0 + 2)]
        for t, (kind, W) in enumerate(plan):
            kinds += tile_of(W, seed + t, special={(31 * t + 5) % 256: kind})
            fast = kind.endswith("2p20m1")
            claims.append(("p", t, {"W": W, "full": True, "cls": expected_k1p_class(W) if fast else "slow_long_op",
                                    "long": None if fast else "own"}))
            claims.append(("c", t, {"W": W, "full": True, "guard": None if fast else "long_op"}))
        return kinds + tile_of(120, seed, size=77), claims
    out += _three("oplen/edges", edges)

    def over_read(seed):
        """An op of length 2^20 as the first word of the NEXT tile: the loads of a tile of 101, 301 and 601 ops reach it."""
        kinds, claims = [], []
        for j, W in enumerate((101, 301, 601)):
            kinds += tile_of(W, seed + j) + tile_of(150, seed + j, special={0: "first_2p20"})
            claims.append(("p", 2 * j, {"W": W, "full": True, "cls": "slow_long_op", "long": "over"}))
            claims.append(("p", 2 * j + 1, {"full": True, "cls": "slow_long_op", "long": "own"}))
            claims.append(("c", 2 * j, {"W": W, "full": True, "guard": None}))
        kinds += tile_of(100, seed) + tile_of(200, seed)             # a multiple of four / eight: nothing is over-read ...
        kinds += tile_of(150, seed, size=77, special={0: "first_2p20"})
        claims.append(("p", 7, {"W": 200, "full": True, "cls": "brief"}))
        return kinds, claims
    out += _three("oplen/over_read", over_read)

    def largest_total(seed):
        """1023 D ops of length 2^20 - 1 in one tile: T's total is 3 218 081 790 < 2^32 and every difference exact."""
        full = ["d4max"] * 255 + ["d3max"]
        kinds = tile_of(300, seed) + full + tile_of(10, seed + 1) + full[::-1] + [k for t in range(4) for k in tile_of(100 + t, seed + t)]
        claims = [("p", t, {"W": 1023, "full": True, "cls": "two_chunks"}) for t in (1, 3)]
        claims += [("c", t, {"W": 1023, "full": True, "guard": None, "chunks": 4}) for t in (1, 3)]
        return kinds + tile_of(120, seed, size=77), claims
    out += _three("oplen/largest_total", largest_total)

    def penalties(seed):
        kinds, claims = [], []
        names = ["pen_2p30m1", "pen_2p30", "pen_2p30p1", "pen_2p30m1_many", "pen_2p30_many", "pen_2p30p1_many", "pen_2p32", "o1a"]
        for t, kind in enumerate(names):
            kinds += tile_of(150 + len(KINDS[kind][0]), seed + t, special={(t * 53 + 9) % 256: kind})
            many = kind.endswith("_many")
            claims.append(("p", t, {"full": True, "cls": "slow_escape" if many else "brief" if kind == "o1a" else "slow_long_op"}))
            claims.append(("c", t, {"full": True, "guard": None if many or kind == "o1a" else "long_op"}))
        return kinds + tile_of(120, seed, size=77), claims
    return out + _three("oplen/penalties", penalties)


def _nm():
    def build(seed):
        kinds, claims = [], []
        plan = [(("nm_m2p23", "nm_2p23m1", "nm_m1", "nm_m7"), False), (("nm_2p23",), True), (("nm_m2p23m1",), True),
                (("nm_m1", "nm_m7", "nm_m2p23"), False), (("nm_2p23m1",), False), (("nm_2p23", "nm_m2p23m1"), True),
                (("nm_m7",), False), (("nm_m2p23m1", "nm_m1"), True)]
        for t, (names, big) in enumerate(plan):
            special = {(41 * j + 7 * t + 3) % 256: k for j, k in enumerate(names)}
            W = 180 + 60 * t + sum(len(KINDS[k][0]) for k in names)
            kinds += tile_of(W, seed + t, special=special)
            claims.append(("p", t, {"full": True, "cls": "slow_big" if big else expected_k1p_class(W)}))
        return kinds + tile_of(90, seed, size=77, special={5: "nm_2p23", 70: "nm_m2p23"}), claims
    return _three("nm/edges", build)


def _range():
    out = []

    def ok(seed):
        """INT32_MAX and INT32_MIN + 1 are scores like any other: nothing is reported."""
        kinds = [k for t in range(8) for k in tile_of(200, seed + t, special={9: "max_exact", 200 + t: "min_plus1"})]
        kinds += tile_of(50, seed, size=77, special={3: "min_plus1", 76: "max_exact"})
        return kinds, [("p", 0, {"full": True, "cls": "slow_big"})]
    out += _three("range/accepted", ok)
    for kind in BAD_KINDS:
        for place in ("full", "tail", "halo"):
            def build(seed, kind=kind, place=place):
                at = {"full": (3, 77), "tail": (8, 40), "halo": (7, 255)}[place]
                tiles = [tile_of(200, seed + t) for t in range(8)] + [tile_of(60, seed, size=77)]
                W = (60 if at[0] == 8 else 200) + len(KINDS[kind][0])
                tiles[at[0]] = tile_of(W, seed, size=len(tiles[at[0]]), special={at[1]: kind})
                return [k for t in tiles for k in t], [("p", at[0], {"cls": "partial" if at[0] == 8 else "slow_big" if
                                                                    kind in ("max_plus1", "min_exact", "far_above") else "slow_long_op"})]
            out += _three("range/%s/%s" % (kind, place), build, arrs=("s1", "s2") if place != "halo" else ("both",))
    return out


def _other():
    def build(seed):
        kinds, claims = [], []
        for t in range(8):
            names = ["x%d" % c for c in range(9, 16)] + ["x15_trailer"]
            special = {(29 * j + t) % 256: k for j, k in enumerate(names)}
            if t == 6:
                special[250] = "x12_2p27"
            W = (60, 255, 256, 400, 511, 512, 300, 1023)[t]
            kinds += tile_of(W, seed + t, special=special)
            claims.append(("p", t, {"W": W, "full": True, "cls": "slow_long_op" if t == 6 else expected_k1p_class(W)}))
            claims.append(("c", t, {"W": W, "full": True, "guard": "long_op" if t == 6 else None}))
        return kinds + tile_of(100, seed, size=77, special={4: "x9", 76: "x15"}), claims
    return _three("other/op_codes_9_to_15", build)


def _counts():
    """Unused words behind a tile's records: the careful path places the records forwards from the tile's begin.  Not in the
    last tile of a workgroup: the record in front of a workgroup is found backwards from where the next tile begins (as the
    records of a tile with escapes are), so the layout leaves the result of such columns open."""
    out = []
    for words, t in ((1, 0), (5, 6), (300, 3)):
        def build(seed, words=words, t=t):
            kinds = [k for q in range(8) for k in tile_of(100 + 90 * q, seed + q)] + tile_of(100, seed, size=77)
            return kinds, [("p", t, {"W": 100 + 90 * t + words, "full": True, "cls": "slow_counts"}),
                           ("p", (t + 1) % 8, {"full": True, "cls": expected_k1p_class(100 + 90 * ((t + 1) % 8))})], {t: words}
        out += _three("counts/slack%d_tile%d" % (words, t), build)
    return out


def _sizes():
    return [Case("sizes/n%d" % n, ordinary(n, 3), ordinary(n, 8),
                 [("p", s, (n - 1) // TILE, {"cls": "partial"} if n % GRAN else {"cls": "slow_end", "dist": 0}) for s in (0, 1)] +
                 [("c", s, (n - 1) // TILE, {"guard": "partial"} if n % CGRAN else {"full": True}) for s in (0, 1)]) for n in SIZES]


_BUILDERS = {"stretch": _stretch, "records": _records, "end": _end, "oplen": _oplen, "nm": _nm, "range": _range,
             "other": _other, "counts": _counts, "sizes": _sizes}
GROUPS = tuple(_BUILDERS)
_ALL = None


def all_cases():
    """Every case of the catalogue (built once; the columns of a case are built when first asked for)."""
    global _ALL
    if _ALL is None:
        _ALL = [c for g in GROUPS for c in _BUILDERS[g]()]
        assert len(set(c.name for c in _ALL)) == len(_ALL)
    return _ALL


def used_kinds():
    return set(k for c in all_cases() for s in (0, 1) for k in c.kinds[s])
