"""Inputs and references for the mate-density correlation kernel (K4, mate_correlate_kernel: xm_mate_correlate,
xm_mate_correlate_dev), shared by the CPU test (tests/test_correlate_shapes_cpu.py: the references agree, every family
catches the mistake it is named for) and the GPU test (tests/test_correlate_shapes_gpu.py).  Pure numpy: no torch, no library.

K4 gives one output per lane, 256 per workgroup, and walks the taps in passes of PASS = 2048: every pass stages a tile of
256 + mm track values, carries the accumulator over and clips its tap count at the track's end (lim).  A wave whose lanes
all have lim == mm runs a plain loop, any other wave a masked one.  The catalogue is built on those edges:

  M           tap counts around a wave, a workgroup, one pass, two passes and three
  lengths(m)  track lengths that put the end of the track next to every wave and workgroup edge, the tap count and both
              pass boundaries (n < m, n == m, n one more than a pass included)
  TRACKS      value families of the track, DENSITIES those of the taps: each is there for one kind of mistake (a fused
              multiply-add, flushed subnormals, taps run over the padding behind the track, another order, a lost carry)

reference() is the loop of Mappability.single_end_to_paired written column by column; the wrong variants below it are what the
CPU test shows the families to tell apart from it.  What "equal" means is same(): the Python loop does not define the sign or
payload of a NaN (on one host the C and the Python form of it already differ there), so NaNs compare by position only;
everything else compares by bit pattern, the sign of a zero or an infinity included.
"""
import math
from fractions import Fraction

import numpy as np

WAVE = 64
GROUP = 256                             # outputs per workgroup (XM_CORR_T)
PASS = 2048                             # taps per pass (XM_CORR_M)
N_MAX = 9000

M = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 2050, 4095, 4096, 4097, 6145]
DELTAS = (-1, 0, 1, 2)


def lengths(m, deltas=DELTAS):
    """Track lengths for m taps: the end of the track at every offset in `deltas` from each edge, within [1, N_MAX]."""
    bases = {0, 64, 128, 192, 256, 512, m, m + 64, m + 128, m + 256, PASS, PASS + 64, PASS + 256, 2 * PASS, 2 * PASS + 256,
             m + PASS}
    return sorted({b + d for b in bases for d in deltas if 1 <= b + d <= N_MAX})


# ---- the reference and what "equal" means -------------------------------------------------------

def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def reference(track, density):
    """out[i] = 1.0 where track[i] == 1, else sum_j track[i + j] * density[j] over j < min(m, n - i), from the first tap to
    the last, product and sum rounded separately: the Python loop, one tap (column) at a time."""
    track, density = _f64(track), _f64(density)
    n = track.shape[0]
    acc, prod = np.zeros(n, dtype=np.float64), np.empty(n, dtype=np.float64)
    with np.errstate(all="ignore"):
        for j in range(min(density.shape[0], n)):               # acc[:n - j] = acc[:n - j] + track[j:] * density[j]
            np.multiply(track[j:], density[j], out=prod[:n - j])
            np.add(acc[:n - j], prod[:n - j], out=acc[:n - j])
    return np.where(track == 1.0, 1.0, acc)


def same(got, want):
    """NaN in the same places; the same 64 bits everywhere else."""
    got, want = _f64(got), _f64(want)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False
    return np.array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan])


def differing(got, want):
    """How many outputs same() objects to."""
    got, want = _f64(got), _f64(want)
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    return int(np.count_nonzero((nan_g != nan_w) | (~nan_g & ~nan_w & (got.view(np.uint64) != want.view(np.uint64)))))


# ---- wrong variants: each has reference()'s signature -------------------------------------------

def _fma(a, b, c):
    """a * b + c with one rounding."""
    if hasattr(math, "fma"):
        return math.fma(a, b, c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    if exact == 0:                      # then a * b is -c, a binary64 value: the two-rounding form is exact and signs the zero
        return a * b + c
    try:
        return float(exact)             # correctly rounded, subnormal results included
    except OverflowError:
        return math.inf if exact > 0 else -math.inf


def fused(track, density):
    """One rounding per tap (what the compiler's default contraction would make of the loop).  Small shapes only."""
    track, density = _f64(track), _f64(density)
    t, d = track.tolist(), density.tolist()
    n, m = len(t), len(d)
    out = np.empty(n, dtype=np.float64)
    for i in range(n):
        acc = 0.0
        for j in range(min(m, n - i)):
            acc = _fma(t[i + j], d[j], acc)
        out[i] = acc
    return np.where(track == 1.0, 1.0, out)


def _flush(x):
    tiny = np.finfo(np.float64).tiny
    return np.where((np.abs(x) < tiny) & (x != 0.0), np.copysign(0.0, x), x)


def flushed(track, density):
    """Subnormal inputs, products and sums replaced by zeros of the same sign (a denormal mode that flushes)."""
    track, density = _f64(track), _f64(density)
    n = track.shape[0]
    t, d = _flush(track), _flush(density)
    acc = np.zeros(n, dtype=np.float64)
    with np.errstate(all="ignore"):
        for j in range(min(d.shape[0], n)):
            acc[:n - j] = _flush(acc[:n - j] + _flush(t[j:] * d[j]))
    return np.where(track == 1.0, 1.0, acc)


def padded(track, density):
    """All m taps for every output, the track taken as 0.0 behind its end (a loop that forgets to stop there)."""
    track, density = _f64(track), _f64(density)
    n, m = track.shape[0], density.shape[0]
    wide = np.concatenate([track, np.zeros(m, dtype=np.float64)])
    acc = np.zeros(n, dtype=np.float64)
    with np.errstate(all="ignore"):
        for j in range(m):
            acc = acc + wide[j:j + n] * density[j]
    return np.where(track == 1.0, 1.0, acc)


def reversed_order(track, density):
    """From the last tap to the first."""
    track, density = _f64(track), _f64(density)
    n = track.shape[0]
    acc = np.zeros(n, dtype=np.float64)
    with np.errstate(all="ignore"):
        for j in reversed(range(min(density.shape[0], n))):
            acc[:n - j] = acc[:n - j] + track[j:] * density[j]
    return np.where(track == 1.0, 1.0, acc)


def no_carry(track, density):
    """The accumulator restarts at 0.0 with every pass of PASS taps."""
    track, density = _f64(track), _f64(density)
    n = track.shape[0]
    acc = np.zeros(n, dtype=np.float64)
    with np.errstate(all="ignore"):
        for j in range(min(density.shape[0], n)):
            if j % PASS == 0:
                acc[:] = 0.0
            acc[:n - j] = acc[:n - j] + track[j:] * density[j]
    return np.where(track == 1.0, 1.0, acc)


VARIANTS = {"fused": fused, "flushed": flushed, "padded": padded, "reversed_order": reversed_order, "no_carry": no_carry}


# ---- track families: (rng, n) -> float64[n] -----------------------------------------------------

def wiggle(rng, n):
    """What tests/test_mappability.py draws: mostly uniquely mappable, else one of three values."""
    return np.where(rng.random(n) < 0.6, 1.0, rng.choice([0.0, 0.0, 0.25, 0.7], n))


def uniform(rng, n):
    return rng.random(n)


def near_one(rng, n):
    """The neighbours of 1.0 next to the `== 1.0` test, both zeros; the last element is 1.0 in half the draws."""
    values = np.array([1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0), -1.0, 0.0, -0.0, 1.0 / 3.0, 0.1])
    t = values[rng.integers(0, values.shape[0], n)]
    if n and rng.random() < 0.5:
        t[-1] = 1.0
    return t


def subnormal_scaled(rng, n):
    """Normal values so small that a product with a tap of 1e-10 is subnormal."""
    return rng.random(n) * 1e-300


def subnormal_bits(rng, n):
    """Bit patterns below 2^40 (at most 5.4e-312), both signs: subnormal before any arithmetic."""
    bits = rng.integers(0, 1 << 40, n, dtype=np.uint64) | (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63))
    return bits.view(np.float64)


def subnormal(rng, n):
    return (subnormal_scaled, subnormal_bits)[int(rng.integers(0, 2))](rng, n)


def overflow(rng, n):
    big = np.finfo(np.float64).max
    values = np.array([1e308, -1e308, big, -big, 1.0 + 2.0 ** -52])
    return values[rng.integers(0, values.shape[0], n)]


def nonfinite(rng, n, m=1):
    """Uniform values with inf, -inf or nan at every 3 * max(m, 1)-th position: each reaches at most m outputs, so at most a
    third of the outputs, and no output sees two of them."""
    t = rng.random(n)
    at = np.arange(0, n, 3 * max(m, 1))
    t[at] = np.array([np.inf, -np.inf, np.nan])[rng.integers(0, 3, at.shape[0])]
    return t


TRACKS = {"wiggle": wiggle, "uniform": uniform, "near_one": near_one, "subnormal": subnormal, "overflow": overflow,
          "nonfinite": nonfinite}


# ---- density families: (rng, m) -> float64[m] ---------------------------------------------------

def normalised(rng, m):
    d = rng.random(m)
    return d / d.sum() if m else d


def tiny(rng, m):
    return rng.random(m) * 1e-10


def signed(rng, m):
    """+, -, +, ... times 1 + r * 2^-30: sums that cancel, products that need all 53 bits."""
    return np.where(np.arange(m) % 2 == 0, 1.0, -1.0) * (1.0 + rng.random(m) * 2.0 ** -30)


def zeros_and_ones(rng, m):
    return np.array([0.0, -0.0, 1.0, -1.0])[rng.integers(0, 4, m)]


def nonfinite_taps(rng, m):
    """0.3 in the first three taps, inf or nan behind them: a tap applied to the padding behind the track gives NaN."""
    d = np.array([np.inf, np.nan])[rng.integers(0, 2, m)]
    d[:3] = 0.3
    return d


DENSITIES = {"normalised": normalised, "tiny": tiny, "signed": signed, "zeros_and_ones": zeros_and_ones,
             "nonfinite_taps": nonfinite_taps}

# Two pairs are left out: with `signed` taps the `overflow` track's products reach both infinities and nearly every output is
# inf - inf, with `nonfinite_taps` nearly every output is NaN as well -- and a NaN is compared by position alone, so an output
# that is NaN checks next to nothing.  tests/test_correlate_shapes_cpu.py holds every remaining overflow pair to "at least
# half of the outputs are not NaN".
DROPPED = {("overflow", "signed"), ("overflow", "nonfinite_taps")}
PAIRS = [(t, d) for t in TRACKS for d in DENSITIES if (t, d) not in DROPPED]


def draw(track_family, density_family, n, m, seed=0):
    """One (track, density) of the named families; the same arrays for the same arguments."""
    rng = np.random.default_rng([seed, n, m, list(TRACKS).index(track_family), list(DENSITIES).index(density_family)])
    make = TRACKS[track_family]
    track = make(rng, n, m) if make is nonfinite else make(rng, n)
    return _f64(track), _f64(DENSITIES[density_family](rng, m))


# ---- the sweep: every length at every tap count, the families rotating ---------------------------

def sweep(m, deltas=DELTAS):
    """[(n, track family, density family)] for m taps.  The case index runs on from one tap count of M to the next and walks
    PAIRS in steps of 11 (coprime to their number, so that neighbouring lengths change both families): len(PAIRS) cases in
    a row use every pair once."""
    assert math.gcd(11, len(PAIRS)) == 1
    first = sum(len(lengths(k, deltas)) for k in M[:M.index(m)])
    return [(n,) + PAIRS[(first + c) * 11 % len(PAIRS)] for c, n in enumerate(lengths(m, deltas))]


def pairs_of_sweep(deltas=DELTAS):
    return {(t, d) for m in M for _, t, d in sweep(m, deltas)}
