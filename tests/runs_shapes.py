"""Inputs for the segmented-lists kernel (K1r, classify_runs_kernel: xm_classify_runs*_dev), shared by the CPU test
(tests/test_runs_shapes_cpu.py: the catalogue reaches what it claims; the two expanders on the reference segmenter's arrays) and
the GPU test (tests/test_runs_shapes_gpu.py).  Pure numpy: no torch, no library.

K1r ranks a granule's units itself: per wave (256 records, a lane = 4 consecutive records) by ballot + mbcnt per bin, with a
two-slot form for waves whose units sit at records 1 and 3 of every lane only (strictly interleaved mates) and a four-slot form
for all others; an in-lane fix-up for units of one lane that share a bin; cross-wave offsets from per-wave bin counts; and a
copy-out of the sorted slab in 16-byte groups.  The catalogue is built on those edges:

  interleaved     strictly interleaved mates, states flat and 90 % skewed: the two-slot form with many bins
  mixed           interleaved streams with single reads (parity flips), triple runs and unit-free waves: both forms in one granule
  two_bins/mM/kK  per granule the first K units in bin a, the rest in bin b, every ordered pair (a, b)
  one_bin         granules whose units all fall in one bin / in every bin but one
  counts          granules with 0, 1, 7, 8, 9, 15, 16, 17, 2047 and 2048 units side by side, three kinds of tail
  nan             binary64 only: NaN units (bin 6) inside single-bin and many-bin granules
  wave_one_bin    a wave with one bin only inside a granule that holds all six

plus a model of what the kernel's waves see (from the flags alone) and a reference segmenter (from the oracle's lists), which
the tests use to state conditions on the catalogue and the layout without asking the code under test.
"""
import itertools

import numpy as np

ABSENT = -2**31
GRAN = 2048
WAVE = 256
N = 2 * GRAN + 77                       # two granules and a ragged tail: K1r carries nothing between granules but the front record
PREFILL = 0xFFFF                        # what segment() leaves in the entries the header calls "not written"

# one realisation of every state 0..5 (AS1, XS1, AS2, XS2) at min_score = -inf; state 6 needs a NaN (binary64 only)
REAL = {0: (0, 0, -5, ABSENT), 1: (-5, ABSENT, 0, 0), 2: (7, 7, 3, ABSENT), 3: (3, ABSENT, 7, 9),
        4: (4, 0, 4, 0), 5: (ABSENT, 1, ABSENT, 1)}
_TABLE = np.array([REAL[k] for k in range(6)], dtype=np.int64)

TWO_BIN_K = (1, 2, 63, 64, 65, 127, 128, 255, 256, 257, 511, 512, 1023)
UNIT_COUNTS = (0, 1, 7, 8, 9, 15, 16, 17, 2047, 2048)
NAN_PLACES = (0, 1, 255, 256, 1023, 1024, 2047, 2048, N - 1)


def granules(n):
    return (int(n) + GRAN - 1) // GRAN


def columns_of_states(states):
    """Four int32 columns in which record r holds REAL[states[r]]."""
    states = np.asarray(states, dtype=np.int64)
    return [np.ascontiguousarray(_TABLE[states, j]).astype(np.int32) for j in range(4)]


def as_f64(cols):
    """The binary64 twin of int32 columns (absent = -inf)."""
    return [np.where(c == ABSENT, -np.inf, c.astype(np.float64)) for c in cols]


def pack_bits(flags):
    """One flag per record -> little-endian uint64 words (the unit_bits argument)."""
    flags = np.asarray(flags, dtype=np.uint8)
    padded = np.zeros(max((flags.shape[0] + 63) // 64, 1) * 64, dtype=np.uint8)
    padded[:flags.shape[0]] = flags != 0
    return np.packbits(padded, bitorder="little").view(np.uint64)


# ---- what K1r's waves see, from the flags alone ------------------------------------------------------------------------

class WaveModel:
    """unit[r]: record r closes a unit (record 0 closes nothing in the paired modes; nothing past n);
    inter[w]: wave w is strictly interleaved (paired modes; no unit at records 0 or 2 mod 4); has_unit[w];
    lane_units[w][l]: units in lane l of wave w; gran_units[g]."""

    def __init__(self, mode, flags):
        n = len(flags)
        self.n, self.n_gran = n, granules(n)
        unit = np.zeros(max(self.n_gran, 1) * GRAN, dtype=bool)
        unit[:n] = np.asarray(flags) != 0
        if mode != 0 and n:
            unit[0] = False
        self.unit = unit
        lanes = unit.reshape(-1, WAVE // 4, 4)
        self.inter = (~(lanes[:, :, 0] | lanes[:, :, 2]).any(axis=1)) if mode != 0 else np.zeros(lanes.shape[0], dtype=bool)
        self.has_unit = lanes.any(axis=(1, 2))
        self.lane_units = lanes.sum(axis=2)
        self.gran_units = unit.reshape(-1, GRAN).sum(axis=1)[:self.n_gran]

    def wave_orders(self, g):
        """(an interleaved wave with units in front of a non-interleaved one, the other way round) inside granule g."""
        w = np.arange(8 * g, 8 * g + 8)
        a = np.flatnonzero(self.inter[w] & self.has_unit[w])
        b = np.flatnonzero(~self.inter[w])                       # a wave that is not interleaved holds a unit
        if not len(a) or not len(b):
            return False, False
        return bool(a.min() < b.max()), bool(b.min() < a.max())


def bins_of_records(n, want_idx, want_off):
    """The oracle's bin of every record: 0..6, 7 = closes no unit."""
    bins = np.full(n, 7, dtype=np.uint8)
    for b in range(7):
        bins[want_idx[int(want_off[b]):int(want_off[b + 1])]] = b
    return bins


# ---- the layout, from the oracle's lists -------------------------------------------------------------------------------

def segment(n, want_idx, want_off, prefill=PREFILL):
    """(runs16, gran_counts) as include/xenomapper_hip.h describes them, from the oracle's flat lists: per granule the units
    sorted by bin, input order inside a bin, as record numbers counted from the granule's first record; eight counts per
    granule, count 7 = 0; the entries behind a granule's units hold `prefill`."""
    n_gran = granules(n)
    runs16 = np.full(n_gran * GRAN, prefill, dtype=np.uint16)
    counts = np.zeros((n_gran, 8), dtype=np.uint16)
    k = np.diff(np.asarray(want_off[:8], dtype=np.int64))
    idx = np.asarray(want_idx[:int(k.sum())], dtype=np.int64)
    if idx.shape[0]:
        bins = np.repeat(np.arange(7, dtype=np.int64), k)
        g = idx // GRAN
        order = np.lexsort((idx, bins, g))                       # by granule, then bin, then input order
        g_sorted = g[order]
        per_gran = np.bincount(g, minlength=n_gran)
        start = np.cumsum(per_gran) - per_gran
        rank = np.arange(idx.shape[0], dtype=np.int64) - start[g_sorted]
        runs16[g_sorted * GRAN + rank] = (idx[order] % GRAN).astype(np.uint16)
        np.add.at(counts, (g, bins), 1)
    return runs16, counts.reshape(-1)


def np_expand(n, runs16, gran_counts, b):
    """List b from the layout as include/xenomapper_hip.h describes it (NumPy, no library call)."""
    n_gran = (n + GRAN - 1) // GRAN
    c = gran_counts[:8 * n_gran].reshape(n_gran, 8).astype(np.int64)
    start = np.cumsum(c, axis=1) - c                              # where bin b begins inside the granule's slab
    k = c[:, b]
    total = int(k.sum())
    if total == 0:
        return np.zeros(0, dtype=np.uint32)
    g = np.repeat(np.arange(n_gran, dtype=np.int64), k)           # granule of every unit of the list
    first = np.cumsum(k) - k
    within = np.arange(total, dtype=np.int64) - np.repeat(first, k)
    at = g * GRAN + np.repeat(start[:, b], k) + within
    return (g * GRAN + runs16[at].astype(np.int64)).astype(np.uint32)


# ---- the cases ---------------------------------------------------------------------------------------------------------

def interleaved_flags(n):
    return (np.arange(n) % 2 == 1).astype(np.uint8)


def mode_flags(mode, n):
    """Every record a unit (single-end) / strictly interleaved mates."""
    return np.ones(n, dtype=np.uint8) if mode == 0 else interleaved_flags(n)


def pair_states(mode, unit_states, n):
    """Record states from one state per unit: single-end record r = unit r; paired, both mates of pair j hold unit j's state
    (so the pair lands in bin = that state in both paired modes), a last record without a mate repeats the last state."""
    if mode == 0:
        return np.asarray(unit_states)[:n]
    return np.repeat(np.asarray(unit_states), 2)[:n]


def units_per_granule(mode):
    return GRAN if mode == 0 else GRAN // 2


def name_stream_flags(n, singles=(), triples=()):
    """Unit flags of a name-sorted stream of pairs in which a read that begins at a record of `singles` has no mate and one
    at a record of `triples` is a run of three equal names: every record that repeats the name in front of it closes a unit."""
    singles, triples = set(int(x) for x in singles), set(int(x) for x in triples)
    flags = np.zeros(n + 3, dtype=np.uint8)
    at, begun = 0, set()
    while at < n:
        begun.add(at)
        size = 1 if at in singles else 3 if at in triples else 2
        flags[at + 1:at + size] = 1
        at += size
    assert (singles | triples) <= begun, "a chosen record is not the first of a read"
    return flags[:n]


def skewed(rng, n, skew):
    flat = rng.integers(0, 6, n)
    return flat if skew is None else np.where(rng.random(n) < 0.9, skew, flat)


def _interleaved():
    out = []
    for mode in (1, 2):
        for skew in (None, 0, 3):
            rng = np.random.default_rng(100 + 10 * mode + (7 if skew is None else skew))
            out.append(("interleaved/m%d/%s" % (mode, "flat" if skew is None else "skew%d" % skew), mode,
                        columns_of_states(skewed(rng, N, skew)), interleaved_flags(N), ABSENT))
    return out


# where the hand-placed single reads of the mixed cases sit: granule 0 is interleaved up to record 1034 and shifted by one
# behind it; a second single read in granule 1 shifts the stream back.  Records 512..767 (wave 2 of granule 0) and
# 2048 + 1280 .. 2048 + 1535 (wave 5 of granule 1) are single reads throughout: waves without a unit between waves with units.
MIXED_SINGLES = (1034, GRAN + 3 * WAVE + 5)
MIXED_EMPTY_WAVES = (2, 8 + 5)
# two triple runs in a row, the first ending at a record 0 mod 4: the lane behind it holds units at its records 0, 1 and 3, and
# the stream keeps its parity (six records).  In waves 1 and 6 of granule 0 and waves 0 and 4 of granule 1, so that waves 0 and
# 3 of granule 0 and waves 6 and 7 of granule 1 stay interleaved.
MIXED_TRIPLES = (356, 359, 1539, 1542, GRAN + 7, GRAN + 10, GRAN + 1028, GRAN + 1031)


def mixed_flags_placed(triples=()):
    singles = list(MIXED_SINGLES)
    for w in MIXED_EMPTY_WAVES:
        singles += range(w * WAVE, (w + 1) * WAVE)
    return name_stream_flags(N, singles, triples)


def _mixed():
    out = []
    for mode in (1, 2):
        for skew in (None, 0):
            tag = "m%d/%s" % (mode, "flat" if skew is None else "skew%d" % skew)
            rng = np.random.default_rng(200 + 10 * mode + (7 if skew is None else skew))
            out.append(("mixed/placed/" + tag, mode, columns_of_states(skewed(rng, N, skew)), mixed_flags_placed(), ABSENT))
            out.append(("mixed/placed_triples/" + tag, mode, columns_of_states(skewed(rng, N, skew)),
                        mixed_flags_placed(MIXED_TRIPLES), ABSENT))
            # as tests/test_gpu_parity.py::test_paired_input_with_unpaired_reads builds them
            for p_single, p_triple in ((0.0, 0.2), (0.05, 0.002)):
                sizes = rng.choice([1, 2, 3], size=N, p=[p_single, 1.0 - p_single - p_triple, p_triple])
                names = np.repeat(np.arange(N), sizes)[:N]
                flags = np.zeros(N, dtype=np.uint8)
                flags[1:] = names[1:] == names[:-1]
                out.append(("mixed/random_s%g_t%g/%s" % (p_single, p_triple, tag), mode,
                            columns_of_states(skewed(rng, N, skew)), flags, ABSENT))
            # few single reads over five granules: whole waves of either class side by side
            n5 = 5 * GRAN + 77
            sizes = rng.choice([1, 2], size=n5, p=[0.005, 0.995])
            names = np.repeat(np.arange(n5), sizes)[:n5]
            flags = np.zeros(n5, dtype=np.uint8)
            flags[1:] = names[1:] == names[:-1]
            out.append(("mixed/sparse_singles/" + tag, mode, columns_of_states(skewed(rng, n5, skew)), flags, ABSENT))
    return out


def two_bin_unit_states(mode, a, b, k):
    """Per granule the first k units in bin a, the rest in bin b: one state per unit."""
    per = units_per_granule(mode)
    n_units = granules(N) * per
    return np.where(np.arange(n_units) % per < k, a, b)


def _two_bins(mode, k):
    out = []
    for a, b in itertools.permutations(range(6), 2):
        states = pair_states(mode, two_bin_unit_states(mode, a, b, k), N)
        out.append(("two_bins/m%d/k%d/a%db%d" % (mode, k, a, b), mode, columns_of_states(states), mode_flags(mode, N), ABSENT))
    return out


def _one_bin():
    out = []
    for mode in (0, 1, 2):
        per = units_per_granule(mode)
        for b in range(6):
            only = np.full(granules(N) * per, b)
            out.append(("one_bin/only%d/m%d" % (b, mode), mode, columns_of_states(pair_states(mode, only, N)),
                        mode_flags(mode, N), ABSENT))
            rng = np.random.default_rng(300 + 10 * mode + b)
            others = np.array([s for s in range(6) if s != b])
            missing = others[rng.integers(0, 5, granules(N) * per)]
            out.append(("one_bin/missing%d/m%d" % (b, mode), mode, columns_of_states(pair_states(mode, missing, N)),
                        mode_flags(mode, N), ABSENT))
    return out


COUNT_TAILS = {"tail_empty": 77, "tail1": 1, "tail2047": 2047}


def count_flags(rng, mode, tail):
    """Granules with UNIT_COUNTS units at random records, side by side (2047 first: record 0 closes nothing in the paired
    modes); a tail granule without a unit, of one record (a unit), or of 2047 records (all units)."""
    per_gran = [2047] + [c for c in UNIT_COUNTS if c != 2047]
    n = GRAN * len(per_gran) + COUNT_TAILS[tail]
    flags = np.zeros(n, dtype=np.uint8)
    for g, units in enumerate(per_gran):
        at = (rng.choice(GRAN - 1, units, replace=False) + 1) if g == 0 else rng.choice(GRAN, units, replace=False)
        flags[at + GRAN * g] = 1
    if tail != "tail_empty":
        flags[GRAN * len(per_gran):] = 1
    return flags, per_gran + [0 if tail == "tail_empty" else COUNT_TAILS[tail]]


def _counts():
    out = []
    for mode in (0, 1, 2):
        for tail in COUNT_TAILS:
            for skew in (None, 0):
                rng = np.random.default_rng(400 + 10 * mode + len(tail) + (7 if skew is None else skew))
                flags, _ = count_flags(rng, mode, tail)
                out.append(("counts/%s/m%d/%s" % (tail, mode, "flat" if skew is None else "skew%d" % skew), mode,
                            columns_of_states(skewed(rng, flags.shape[0], skew)), flags, ABSENT))
    return out


def _nan():
    out = []
    for mode in (0, 1, 2):
        rng = np.random.default_rng(500 + mode)
        hit = np.concatenate([rng.choice(N, 40, replace=False), NAN_PLACES])
        kinds = [("only%d" % b, np.full(N, b)) for b in (0, 3, 5)]
        kinds.append(("many", pair_states(mode, rng.integers(0, 6, N), N)))
        for kind, states in kinds:
            cols = as_f64(columns_of_states(states))
            cols[0][hit] = np.nan
            cols[2][hit] = np.nan
            out.append(("nan/%s/m%d" % (kind, mode), mode, cols, mode_flags(mode, N), -np.inf))
    return out


WAVE_ONE_BIN = ((3, 2), (8 + 6, 4))     # (wave, its only state): wave 3 of granule 0, wave 6 of granule 1


def _wave_one_bin():
    out = []
    for mode in (0, 1, 2):
        rng = np.random.default_rng(600 + mode)
        states = pair_states(mode, rng.integers(0, 6, N), N).copy()
        for w, s in WAVE_ONE_BIN:
            states[w * WAVE:(w + 1) * WAVE] = s                  # waves begin at even records: both mates of its pairs
        out.append(("wave_one_bin/m%d" % mode, mode, columns_of_states(states), mode_flags(mode, N), ABSENT))
    return out


_BUILDERS = {"interleaved": _interleaved, "mixed": _mixed, "one_bin": _one_bin, "counts": _counts, "nan": _nan,
             "wave_one_bin": _wave_one_bin}
TWO_BIN_GROUPS = ["two_bins/m%d/k%d" % (mode, k) for mode in (0, 1, 2) for k in TWO_BIN_K]
GROUPS = list(_BUILDERS) + TWO_BIN_GROUPS


def group(name):
    """The cases of one group of GROUPS: a list of (name, mode, cols, flags, m).  cols are int32 (the binary64 twin is as_f64's)
    or, in the group "nan", binary64; m is the min_score of the columns' type."""
    if name in _BUILDERS:
        return _BUILDERS[name]()
    _, mode, k = name.split("/")
    return _two_bins(int(mode[1:]), int(k[1:]))


def all_shapes():
    return [case for name in GROUPS for case in group(name)]
