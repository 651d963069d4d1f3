"""Where a caller's buffers may lie: the placement contract of include/xenomapper_hip.h as a table, and an arena to test it in.

ROWS has one row per device-resident entry point (every prototype of the header whose name ends in _dev), in the order of the
C parameters behind (ctx, stream): scalars by name and C type, pointers with element type, the alignment the header demands,
whether NULL is allowed, whether the call reads or writes there, and how many bytes it may touch.  csrc/xm_api.hip refuses
what this table forbids (XM_ERR_INVALID_ARG before anything is enqueued); tests/test_abi_placements_cpu.py holds the table
against the header's prototypes, tests/test_abi_placements_gpu.py runs every row at every placement offered here.

HOST names the host-buffer entry points: they copy their data, so element alignment is all they ask for.

Pure Python and NumPy; nothing here needs a GPU.  The arena helpers work alike on a NumPy uint8 array and a torch.uint8 tensor.
"""
from collections import namedtuple

import numpy as np

SIZEOF = {"uint8_t": 1, "uint16_t": 2, "int32_t": 4, "uint32_t": 4, "uint64_t": 8, "double": 8}
NP_TYPE = {"uint8_t": np.uint8, "uint16_t": np.uint16, "int32_t": np.int32, "uint32_t": np.uint32, "uint64_t": np.uint64,
           "double": np.float64}

FILL = 0x5A                     # every arena byte before a call
GUARD = 64                      # bytes of FILL between neighbours, at least
MAX_RECORDS = 0xFFFFF000        # XM_MAX_RECORDS
GRAN = 2048                     # XM_RUNS_GRAN, and the granule of every counting kernel

# role: "in" (read only), "out" (written only), "inout" (range_flag: set, never cleared)
# extent: bytes the call may read / write, an expression in n (records), m (taps), cap (list capacity), ops* (words of a CIGAR
#         op array) and the header's macros below
# count: 1, or 6 for `uint32_t *const idx_out[6]`: a HOST array of six device pointers, each under this rule
Ptr = namedtuple("Ptr", "name ctype align nullable role extent count")
Scalar = namedtuple("Scalar", "name ctype")
Row = namedtuple("Row", "name params one_of")     # one_of: names of which at least one must be given (code_out / bins4)


def bins4_bytes(n):             # XM_BINS4_BYTES
    return (n + 2047) // 2048 * 1024


def runs_granules(n):           # XM_RUNS_GRANULES
    return (n + GRAN - 1) // GRAN


def runs16_entries(n):          # XM_RUNS16_ENTRIES
    return runs_granules(n) * GRAN


def cig_tiles(n):               # XM_CIG_TILES
    return (n + 255) // 256


_MACROS = {"BINS4": bins4_bytes, "GRANULES": runs_granules, "RUNS16": runs16_entries, "TILES": cig_tiles}


def _p(name, ctype, align, extent, role="in", nullable=False, count=1):
    return Ptr(name, ctype, align, nullable, role, extent, count)


MODE, N, MIN_I, MIN_F, CAP = (Scalar("mode", "int"), Scalar("n_records", "uint64_t"), Scalar("min_score_floor", "int32_t"),
                              Scalar("min_score", "double"), Scalar("list_capacity", "uint64_t"))


def _cols(ctype, align, names=("as1", "xs1", "as2", "xs2")):
    return [_p(k, ctype, align, "%d*n" % SIZEOF[ctype]) for k in names]


BITS = _p("unit_bits", "uint64_t", 8, "8*((n+63)//64)")
OFFSETS = _p("bin_offsets", "uint64_t", 8, "64", "out")
N_OUT = _p("n_out", "uint64_t", 8, "64", "out")
COUNTS = _p("counts", "uint64_t", 8, "512", "out")
IDX = _p("idx_out", "uint32_t", 4, "4*n", "out")
LISTS = _p("idx_out", "uint32_t", 4, "4*cap", "out", count=6)
STATE6 = _p("idx_state6", "uint32_t", 4, "4*cap", "out", nullable=True)
FLAG = _p("range_flag", "uint32_t", 4, "4", "inout", nullable=True)
BINS4 = _p("bins4", "uint8_t", 16, "BINS4(n)", "out", nullable=True)
CODE4 = _p("code_out", "uint8_t", 4, "n", "out")                          # the classify-only calls: one dword store a lane
CODE16 = _p("code_out", "uint8_t", 16, "n", "out", nullable=True)         # written by K1, read again 16 bytes a lane by K2
RUNS = [_p("runs16", "uint16_t", 16, "2*RUNS16(n)", "out"), _p("gran_counts", "uint16_t", 16, "16*GRANULES(n)", "out")]


def _csr(s):                    # CSR CIGAR columns of one species as the classify kernels take them
    return [_p("nm" + s, "int32_t", 16, "4*n"), _p("cig_off" + s, "uint32_t", 16, "4*(n+1)"),
            _p("cig_oplen" + s, "uint32_t", 4, "4*ops" + s), _p("xs" + s, "int32_t", 16, "4*n")]


def _packed(s):                 # packed CIGAR columns of one species
    return [_p("nm" + s, "int32_t", 16, "4*n"), _p("cig_cnt" + s, "uint8_t", 4, "n"),
            _p("cig_tile" + s, "uint32_t", 4, "4*(TILES(n)+1)"), _p("cig_oplen" + s, "uint32_t", 4, "4*ops" + s),
            _p("xs" + s, "int32_t", 16, "4*n")]


EITHER = ("code_out", "bins4")

ROWS = [
    Row("xm_classify_dev", [MODE, N] + _cols("int32_t", 16) + [BITS, MIN_I, CODE4], ()),
    Row("xm_classify_f64_dev", [MODE, N] + _cols("double", 32) + [BITS, MIN_F, CODE4], ()),
    Row("xm_classify_cigar_dev", [MODE, N] + _csr("1") + _csr("2") + [BITS, MIN_I, CODE4, FLAG], ()),
    Row("xm_cigar_scores_dev", [N, _p("nm", "int32_t", 4, "4*n"), _p("cig_off", "uint32_t", 4, "4*(n+1)"),
                                _p("cig_oplen", "uint32_t", 4, "4*ops"), _p("as_out", "int32_t", 4, "4*n", "out"), FLAG], ()),
    Row("xm_mate_correlate_dev", [Scalar("n", "uint64_t"), _p("track", "double", 8, "8*n"), Scalar("m", "uint64_t"),
                                  _p("density", "double", 8, "8*m"), _p("out", "double", 8, "8*n", "out")], ()),
    Row("xm_compact_dev", [MODE, N, _p("code", "uint8_t", 16, "n"), IDX, OFFSETS, COUNTS], ()),
    Row("xm_classify_compact_dev", [MODE, N] + _cols("int32_t", 16) + [BITS, MIN_I, CODE16, BINS4, IDX, OFFSETS, COUNTS], EITHER),
    Row("xm_classify_compact_f64_dev", [MODE, N] + _cols("double", 32) + [BITS, MIN_F, CODE16, BINS4, IDX, OFFSETS, COUNTS], EITHER),
    Row("xm_classify_compact_cigar_dev", [MODE, N] + _csr("1") + _csr("2") +
        [BITS, MIN_I, CODE16._replace(nullable=False), FLAG, IDX, OFFSETS, COUNTS], ()),
    Row("xm_classify_compact_cigar_packed_dev", [MODE, N] + _packed("1") + _packed("2") +
        [BITS, MIN_I, CODE16, BINS4, FLAG, IDX, OFFSETS, COUNTS], EITHER),
    Row("xm_classify_place_dev", [MODE, N] + _cols("int32_t", 16) + [BITS, MIN_I, CODE16, BINS4, LISTS, CAP, N_OUT, COUNTS], EITHER),
    Row("xm_classify_place_f64_dev", [MODE, N] + _cols("double", 32) +
        [BITS, MIN_F, CODE16, BINS4, LISTS, STATE6, CAP, N_OUT, COUNTS], EITHER),
    Row("xm_classify_place_cigar_packed_dev", [MODE, N] + _packed("1") + _packed("2") +
        [BITS, MIN_I, CODE16, BINS4, FLAG, LISTS, CAP, N_OUT, COUNTS], EITHER),
    Row("xm_classify_runs_dev", [MODE, N] + _cols("int32_t", 16) + [BITS, MIN_I] + RUNS + [N_OUT, COUNTS], ()),
    Row("xm_classify_runs_f64_dev", [MODE, N] + _cols("double", 32) + [BITS, MIN_F] + RUNS + [N_OUT, COUNTS], ()),
    Row("xm_stream_probe_dev", [N] + _cols("int32_t", 16, ("c0", "c1", "c2", "c3")) + [_p("out", "uint8_t", 2, "2*(n//4)", "out")], ()),
]
ROW = {r.name: r for r in ROWS}

# The host-buffer entry points copy their data to the device: "element alignment only".  name -> {pointer parameter: C type}
_I4 = dict.fromkeys(("as1", "xs1", "as2", "xs2"), "int32_t")
_F8 = dict.fromkeys(("as1", "xs1", "as2", "xs2"), "double")
HOST = {
    "xm_classify": dict(_I4, unit_bits="uint64_t", code_out="uint8_t", counts="uint64_t"),
    "xm_classify_f64": dict(_F8, unit_bits="uint64_t", code_out="uint8_t", counts="uint64_t"),
    "xm_compact": dict(code="uint8_t", idx_out="uint32_t", bin_offsets="uint64_t", counts="uint64_t"),
    "xm_classify_compact": dict(_I4, unit_bits="uint64_t", code_out="uint8_t", idx_out="uint32_t", bin_offsets="uint64_t",
                                counts="uint64_t"),
    "xm_classify_place": dict(_I4, unit_bits="uint64_t", code_out="uint8_t", idx_out="uint32_t", n_out="uint64_t",
                              counts="uint64_t"),
    "xm_runs_expand": dict(runs16="uint16_t", gran_counts="uint16_t", idx_out="uint32_t", n_written="uint64_t"),
}


def pointers(row):
    return [p for p in row.params if isinstance(p, Ptr)]


def buffers(row):
    """The buffers of a row by name: a six-list parameter counts six times, idx_out[0] .. idx_out[5]."""
    out = []
    for p in pointers(row):
        if p.count == 1:
            out.append((p.name, p))
        else:
            out += [("%s[%d]" % (p.name, b), p) for b in range(p.count)]
    return out


def extent(p, **env):
    """Bytes of parameter p for these sizes (n, m, cap, ops, ops1, ops2 as its expression needs them)."""
    return int(eval(p.extent, dict(_MACROS, __builtins__={}), env))         # noqa: S307 -- the expressions are this file's own


def residues(align):
    """Offsets from a 256-byte boundary at which a buffer demanding `align` is placed: 0, align, the largest multiple of align
    below 256 and, for align < 16, every multiple of align below 16 (a 4-byte-aligned list at 4, 8 and 12 past a 16-byte
    boundary)."""
    r = {0, align, (255 // align) * align}
    if align < 16:
        r |= set(range(0, 16, align))
    return sorted(r)


def smallest_nonzero(align):
    return residues(align)[1]


def refused_steps(p):
    """Offsets from a 256-byte boundary at which parameter p must be refused: half its alignment (8 off for a 16-byte column,
    16 for a binary64 one, 4 for unit_bits and counts, 2 for idx_out -- the largest placement that is still wrong) and, where
    that is another one, one element (4 off for an int32 column: the smallest a typed pointer can be off by)."""
    steps = {p.align // 2}
    if SIZEOF[p.ctype] < p.align:
        steps.add(SIZEOF[p.ctype])
    return sorted(steps)


def lay_out(row, sizes, residue=None):
    """Places the buffers of `row` in one arena.  sizes: buffer name -> bytes (idx_out[0] .. by their own names);
    residue: buffer name -> offset from a 256-byte boundary (default 0; anything below 256 may be asked for: the ones the
    contract allows are residues(p.align), the ones it refuses refused_steps(p)).  -> ({name: (offset, bytes)}, arena bytes).
    Every buffer is preceded and followed by at least GUARD bytes that belong to nobody."""
    residue = residue or {}
    at, cursor = {}, 0
    for name, p in buffers(row):
        r = int(residue.get(name, 0))
        assert 0 <= r < 256, (name, r)
        start = (cursor + GUARD + 255) // 256 * 256 + r
        at[name] = (start, int(sizes[name]))
        cursor = start + int(sizes[name])
    return at, (cursor + GUARD + 255) // 256 * 256


def _address(arena):
    return arena.data_ptr() if hasattr(arena, "data_ptr") else arena.ctypes.data


def aligned_arena(raw, total):
    """`total` bytes of the uint8 array / tensor `raw` (total + 255 bytes or more) that begin at a 256-byte boundary."""
    skip = (-_address(raw)) % 256
    arena = raw[skip:skip + total]
    assert _address(arena) % 256 == 0 and arena.shape[0] == total
    return arena


def new_arena(total):
    raw = np.full(total + 256, FILL, dtype=np.uint8)
    return aligned_arena(raw, total)


def view(arena, at, name, ctype):
    """The buffer `name` of the arena as elements of its C type -- by slicing and .view(dtype), on NumPy and torch alike
    (torch has no unsigned 16 / 32 / 64-bit element everywhere: the signed type of the same size stands in there)."""
    off, nbytes = at[name]
    piece = arena[off:off + nbytes]
    if hasattr(arena, "data_ptr"):
        import torch
        return piece.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.float64 if ctype == "double" else torch.int64}
                          [SIZEOF[ctype]])
    return piece.view(NP_TYPE[ctype])


def owned(at, total):
    """Boolean map of the arena: True where a byte belongs to some buffer."""
    m = np.zeros(total, dtype=bool)
    for off, nbytes in at.values():
        assert not m[off:off + nbytes].any(), "buffers overlap"
        m[off:off + nbytes] = True
    return m


# ---- the one input of the GPU test ------------------------------------------------------------------------------------
N_RECORDS = 3 * GRAN + 77       # three whole granules and a ragged one
ABSENT = -2**31
STAGE_MIN_UNITS = 1536          # XM_STAGE_MIN_UNITS of csrc/xm_kernels.hip

# score columns that give mapping state k (k = 0..5) whatever min_score <= -6 is: (as1, xs1, as2, xs2)
_STATE_COLUMNS = {0: (0, 0, -5, ABSENT), 1: (-5, ABSENT, 0, 0), 2: (7, 7, 3, ABSENT), 3: (3, ABSENT, 7, 9), 4: (4, 0, 4, 0),
                  5: (ABSENT, 1, ABSENT, 1)}


def pack_bits(flags):
    flags = np.asarray(flags, dtype=np.uint8)
    padded = np.concatenate([flags, np.zeros((-flags.shape[0]) % 64, np.uint8)])
    return np.packbits(padded, bitorder="little").view(np.uint64)


def draw_states(rng, n=N_RECORDS):
    """Mapping states of n records such that in single-end mode (every record a unit, state = bin) every whole granule has
    two bins of 64 units or more, whose runs begin and end off a 16-byte boundary somewhere, and one bin of fewer than 64:
    head, body, tail and the short run of the staged copy-out."""
    states = np.empty(n, dtype=np.int64)
    for g in range(runs_granules(n)):
        lo, hi = g * GRAN, min(n, (g + 1) * GRAN)
        p = np.array([0.45, 0.35, 0.0, 0.0, 0.19, 0.0])
        p[2 + g % 2] = 0.01                                               # ~20 units of bin 2 or 3: a short run; the other stays empty
        states[lo:hi] = rng.choice(6, size=hi - lo, p=p)
    return states


def unit_flags(mode, n=N_RECORDS):
    """Single-end: every record was yielded.  Paired: name[i] == name[i - 1] -- granule 0 strictly interleaved mates, granule 1
    runs of equal names (three and more records in a row close units: dense), granule 2 mates with unpaired reads in between
    (the parity flips), the ragged granule every other record again."""
    if mode == 0:
        return np.ones(n, dtype=np.uint8)
    f = np.zeros(n, dtype=np.uint8)
    f[1:GRAN:2] = 1
    rng = np.random.default_rng(77)
    f[GRAN:2 * GRAN] = rng.random(GRAN) < 0.8
    i = 2 * GRAN
    while i < 3 * GRAN:
        if rng.random() < 0.2:
            i += 1                                                        # an unpaired read
        else:
            if i + 1 < 3 * GRAN:
                f[i + 1] = 1
            i += 2
    f[3 * GRAN + 1::2] = 1
    f[0] = 1                                                              # record 0 has no predecessor: the kernels must drop this one
    return f


def score_columns(states):
    table = np.array([_STATE_COLUMNS[k] for k in range(6)], dtype=np.int64)
    return [np.ascontiguousarray(table[states, j]).astype(np.int32) for j in range(4)]


def as_doubles(cols, nan_at=()):
    """The same values as binary64 (absent = -inf) with NaN in as1 at the records nan_at: units holding state 6."""
    out = [np.where(c == ABSENT, -np.inf, c.astype(np.float64)) for c in cols]
    for i in nan_at:
        out[0][i] = np.nan
    return out


def random_cigar(rng, n=N_RECORDS, long_record=None):
    """Small random CSR CIGAR columns (NM, offsets, packed ops); long_record gets 300 ops, more than a count byte holds."""
    n_ops = rng.integers(0, 7, n).astype(np.uint32)
    n_ops[rng.random(n) < 0.5] = 1
    if long_record is not None:
        n_ops[long_record] = 300
    off = np.zeros(n + 1, dtype=np.uint32)
    np.cumsum(n_ops, out=off[1:])
    total = int(off[-1])
    ops = (rng.integers(1, 60, total).astype(np.uint32) << 4) | rng.integers(0, 9, total).astype(np.uint32)
    nm = np.where(rng.random(n) < 0.15, ABSENT, rng.integers(0, 6, n)).astype(np.int32)
    return {"nm": nm, "cig_off": off, "cig_oplen": ops}


def staged_runs(code, offsets, n=N_RECORDS):
    """What the staged single-end copy-out (scatter_copy_out) meets for these category bytes: per whole granule with
    STAGE_MIN_UNITS units or more and per bin, (G & 3, N) -- the run's place in idx_out modulo a 16-byte group and its length."""
    runs = []
    before = np.zeros(7, dtype=np.int64)
    for g in range(runs_granules(n)):
        c = code[g * GRAN:(g + 1) * GRAN]
        cnt = np.array([(c == b).sum() for b in range(7)])
        if cnt.sum() >= STAGE_MIN_UNITS:
            runs += [(int((int(offsets[b]) + before[b]) & 3), int(cnt[b])) for b in range(7) if cnt[b]]
        before += cnt
    return runs
