"""Inputs for the scatter kernel's form for skewed, strictly interleaved granules (K2c with the compact stream:
scatter_granule_skew in xm_kernels.hip), shared by the CPU test (tests/test_scatter_skew_cpu.py: the catalogue reaches what it
claims; the oracle's lists are a plain stable split) and the GPU test (tests/test_scatter_skew_gpu.py).  Pure numpy, built on
tests/runs_shapes.py.

That form takes a granule 512 records = 256 units = one TILE at a time, a lane = 4 consecutive units (SLOTS).  The granule has
a dominant bin D; a tile's units of D are ranked by ballots, all other slots go through a table that is read back 64 entries a
round.  The catalogue is built on those edges:

  counts      R slots of a tile that do not hold D, R in RARE_COUNTS, in one bin or over all other bins, at random places
  lanes       every one of the 16 ways a lane's four slots can be D or not, side by side in one tile
  edges       two other bins meeting at a lane edge, and at the table's 64th entry
  d_not_first the first unit's bin is not the dominant one
  d_changes   another bin dominates in later tiles of the granule
  no_flag     odd records without their unit flag inside an interleaved granule (some, and most of a tile)
  fallback    one granule of the two is not strictly interleaved
  random      90 % skewed and flat states

each for both pair rules, on two granules and a ragged tail (N records) and, where it fits, on one single tile.  Model is what
the tests use to state conditions on the catalogue from the oracle's bins alone, without asking the code under test; its
dominant() is the kernel's own rule, which is free: results must not depend on it.
"""
import numpy as np

from tests import runs_shapes as S

GRAN = S.GRAN
TILE = 512                               # records
TILE_UNITS = TILE // 2
TILES = GRAN // TILE
N = S.N                                  # two granules and a ragged tail
RARE_COUNTS = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256)
MODES = (1, 2)                           # the two pair rules


def build(mode, unit_bins, n, flags=None):
    """A case from one bin 0..5 per unit (tests/runs_shapes.py: pair_states)."""
    unit_bins = np.asarray(unit_bins)
    assert unit_bins.shape[0] == (n + 1) // 2
    states = S.pair_states(mode, unit_bins, n)
    return S.columns_of_states(states), (S.interleaved_flags(n) if flags is None else flags)


def tile(d, places=(), bins=()):
    """256 units of bin d, but bins[i] at places[i]."""
    t = np.full(TILE_UNITS, d, dtype=np.int64)
    if len(places):
        t[np.asarray(places, dtype=np.int64)] = np.asarray(bins, dtype=np.int64)
    return t


def stream(tiles, d_tail, n=N):
    """Unit bins of n records from tiles in order, the units behind them in bin d_tail."""
    u = np.full((n + 1) // 2, d_tail, dtype=np.int64)
    body = np.concatenate(tiles)
    u[:body.shape[0]] = body[:u.shape[0]]
    return u


def other_bins(d):
    return [b for b in range(6) if b != d]


def rare_places(rng, r, first_tile):
    """r places of a tile; in a granule's first tile unit 0 and most lanes' first slots keep the dominant bin."""
    if not first_tile:
        return np.sort(rng.choice(TILE_UNITS, r, replace=False))
    assert r <= 128
    slot0 = np.arange(4, TILE_UNITS, 4)                              # first slots of lanes 1..63
    rest = np.setdiff1d(np.arange(TILE_UNITS), np.arange(0, TILE_UNITS, 4))
    k0 = min(r // 8, 31)
    return np.sort(np.concatenate([rng.choice(slot0, k0, replace=False), rng.choice(rest, r - k0, replace=False)]))


def rare_bins(kind, d, k):
    if kind == "one":
        return np.full(k, other_bins(d)[2])
    return np.array(other_bins(d))[np.arange(k) % 5]


def _counts():
    out = []
    for mode in MODES:
        for kind, d in (("one", 0), ("all", 2)):
            for r in RARE_COUNTS:
                rng = np.random.default_rng(1000 * mode + 10 * r + d)
                tiles = []
                for t in range(2 * TILES):
                    first = t % TILES == 0
                    k = r if (not first or r <= 128) else 0
                    tiles.append(tile(d, rare_places(rng, k, first), rare_bins(kind, d, k)))
                out.append(("counts/R%d/%s/m%d" % (r, kind, mode), mode) + build(mode, stream(tiles, d), N) + (S.ABSENT,))
                if r <= 128:
                    one = tile(d, rare_places(rng, r, True), rare_bins(kind, d, r))
                    out.append(("counts/R%d/%s/tile/m%d" % (r, kind, mode), mode) + build(mode, one, TILE) + (S.ABSENT,))
    return out


def lane_pattern_tile(d, kind, shift):
    """Lane l's slot j holds another bin where bit j of (l + shift) % 16 is set: pattern 0 = D D D D ... 15 = r r r r."""
    t = np.full(TILE_UNITS, d, dtype=np.int64)
    k = 0
    for lane in range(64):
        pat = (lane + shift) % 16
        for j in range(4):
            if (pat >> j) & 1:
                t[4 * lane + j] = rare_bins(kind, d, k + 1)[k]
                k += 1
    return t


def _lanes():
    out = []
    for mode in MODES:
        for kind, d in (("one", 1), ("all", 0)):
            # the first tile of a granule begins with pattern 0, and half of its lanes' first slots hold D
            tiles = [lane_pattern_tile(d, kind, 2 * (t % TILES)) for t in range(2 * TILES)]
            out.append(("lanes/%s/m%d" % (kind, mode), mode) + build(mode, stream(tiles, d), N) + (S.ABSENT,))
            out.append(("lanes/%s/tile/m%d" % (kind, mode), mode) + build(mode, tiles[0], TILE) + (S.ABSENT,))
    return out


EDGE_LANE = 10                           # slots 2, 3 of this lane in bin a, slots 0, 1 of the next in bin b


def _edges():
    out = []
    for mode in MODES:
        d, a, b = 0, 3, 5
        at = 4 * EDGE_LANE
        lane_edge = tile(d, [at + 2, at + 3, at + 4, at + 5], [a, a, b, b])
        # 64 units of bin a, then bin b: entry 63 of the table is the last a, the next round begins with b
        places = np.arange(1, 2 * 70, 2)
        table_edge = tile(d, places, [a] * 64 + [b] * 6)
        # the same with a change of bin inside a lane at the 64th entry (places 3 a lane: entries 63 and 64 in one lane)
        places3 = np.setdiff1d(np.arange(TILE_UNITS), np.arange(0, TILE_UNITS, 4))[:66]
        table_edge_in_lane = tile(d, places3, [a] * 64 + [b] * 2)
        tiles = [lane_edge, table_edge, table_edge_in_lane, tile(d), table_edge, lane_edge, tile(d), table_edge_in_lane]
        out.append(("edges/m%d" % mode, mode) + build(mode, stream(tiles, d), N) + (S.ABSENT,))
        for name, one in (("lane", lane_edge), ("table", table_edge), ("table_in_lane", table_edge_in_lane)):
            out.append(("edges/%s/tile/m%d" % (name, mode), mode) + build(mode, one, TILE) + (S.ABSENT,))
    return out


def _d_not_first():
    out = []
    for mode in MODES:
        rng = np.random.default_rng(70 + mode)
        d, r = 1, 3
        # unit 0 and a few lanes' first slots in bin r, bin d everywhere else but 40 random places
        head = [0, 8, 16]
        places = np.setdiff1d(rng.choice(TILE_UNITS, 40, replace=False), head + [4])     # unit 4: the second candidate
        first = tile(d, np.concatenate([head, places]), [r] * 3 + list(rare_bins("all", d, len(places))))
        tiles = [first, tile(d, [7], [4]), tile(d), first] + [first, tile(d), tile(d, [255], [0]), tile(d)]
        out.append(("d_not_first/m%d" % mode, mode) + build(mode, stream(tiles, d), N) + (S.ABSENT,))
        out.append(("d_not_first/tile/m%d" % mode, mode) + build(mode, first, TILE) + (S.ABSENT,))
    return out


def _d_changes():
    out = []
    for mode in MODES:
        rng = np.random.default_rng(80 + mode)
        tiles = []
        for d in (0, 4, 0, 5, 2, 2, 3, 1):
            places = rng.choice(np.arange(1, TILE_UNITS), 30, replace=False)
            tiles.append(tile(d, places, rare_bins("all", d, 30)))
        out.append(("d_changes/m%d" % mode, mode) + build(mode, stream(tiles, 0), N) + (S.ABSENT,))
    return out


NO_FLAG_SOME = (1, 9, 511, 513, 1023, GRAN - 1, GRAN + 1, GRAN + 2 * TILE + 255, N - 2)      # odd records


def _no_flag():
    out = []
    for mode in MODES:
        rng = np.random.default_rng(90 + mode)
        units = np.where(rng.random((N + 1) // 2) < 0.85, 0, rng.integers(0, 6, (N + 1) // 2))
        units[[0, 4, 8]] = 0                                              # the lanes' first slots the choice of D looks at first
        flags = S.interleaved_flags(N)
        flags[list(NO_FLAG_SOME)] = 0
        out.append(("no_flag/some/m%d" % mode, mode) + build(mode, units, N, flags) + (S.ABSENT,))
        # most of a granule's first tile without flags, its first unit included: a dominant "no unit"
        flags = S.interleaved_flags(N)
        gone = np.concatenate([[0], rng.choice(np.arange(1, TILE_UNITS), 200, replace=False)])
        flags[2 * gone + 1] = 0
        flags[GRAN + 2 * gone + 1] = 0
        out.append(("no_flag/most/m%d" % mode, mode) + build(mode, units, N, flags) + (S.ABSENT,))
    return out


FALLBACK_SINGLES = {"second": (GRAN + 300,), "first": (300, 1301)}       # which granule is not strictly interleaved


def _fallback():
    out = []
    for mode in MODES:
        for which, singles in FALLBACK_SINGLES.items():
            rng = np.random.default_rng(110 + mode + len(which))
            flags = S.name_stream_flags(N, singles)
            out.append(("fallback/%s/m%d" % (which, mode), mode, S.columns_of_states(S.skewed(rng, N, 0)), flags, S.ABSENT))
    return out


def _random():
    out = []
    for mode in MODES:
        for skew in (None, 0, 3):
            rng = np.random.default_rng(120 + 10 * mode + (7 if skew is None else skew))
            units = S.skewed(rng, (N + 1) // 2, skew)
            out.append(("random/%s/m%d" % ("flat" if skew is None else "skew%d" % skew, mode), mode) +
                       build(mode, units, N) + (S.ABSENT,))
    return out


_BUILDERS = {"counts": _counts, "lanes": _lanes, "edges": _edges, "d_not_first": _d_not_first, "d_changes": _d_changes,
             "no_flag": _no_flag, "fallback": _fallback, "random": _random}
GROUPS = list(_BUILDERS)


def group(name):
    """The cases of one group: a list of (name, mode, cols, flags, m), int32 columns."""
    return _BUILDERS[name]()


def all_shapes():
    return [case for name in GROUPS for case in group(name)]


# ---- what the skew form sees, from the oracle's bins alone ---------------------------------------------------------------

class Model:
    """bins: the oracle's bin of every record (7 = closes no unit), padded with 7 to whole granules.
    skew[g]: granule g takes the skew form (no unit at an even record); slots[g][t]: the 256 slot bins of tile t (odd records);
    dominant(g): the kernel's choice for granule g; rare(g, t): slots of the tile that do not hold it."""

    def __init__(self, n, bins):
        self.n, self.n_gran = n, S.granules(n)
        padded = np.full(self.n_gran * GRAN, 7, dtype=np.uint8)
        padded[:n] = bins
        recs = padded.reshape(self.n_gran, TILES, TILE_UNITS, 2)
        self.skew = (recs[:, :, :, 0] == 7).all(axis=(1, 2))
        self.slots = recs[:, :, :, 1]

    def dominant(self, g):
        first = self.slots[g, 0, 0::4]                                # the lanes' first slots of the first tile
        d = first[0]
        if (first == d).sum() < 32:
            d = first[first != d][0]
        return int(d)

    def rare(self, g, t):
        return int((self.slots[g, t] != self.dominant(g)).sum())

    def lane_patterns(self, g, t):
        nd = (self.slots[g, t] != self.dominant(g)).reshape(64, 4)
        return set((nd * (1 << np.arange(4))).sum(axis=1).tolist())

    def table(self, g, t):
        """The tile's table: (slot, bin) of the slots that do not hold the dominant bin, in order."""
        at = np.flatnonzero(self.slots[g, t] != self.dominant(g))
        return at, self.slots[g, t][at]
