"""The catalogue of tests/correlate_shapes.py without a GPU: its reference is the Python loop and the C oracle bit for bit, every
wrong variant of the loop is told apart from it by the family meant to catch it (and, recorded here, by which families it is
not), the NaN-heavy pairs stay within their caps, the lengths reach the pass edges they claim, and every pair is used by the
sweep.  Then Mappability.single_end_to_paired around a stub context: a track shorter than its chromosome keeps the tail of
integer zeros, as the reference's element-wise assignment does."""
import numpy as np
import pytest

from oracle import mappability_oracle as MO
from tests import correlate_shapes as S
from tests import helpers as H

PYTHON_SHAPES = [(1, 0), (5, 0), (1, 1), (3, 7), (65, 3), (130, 64), (300, 257), (200, 2049)]       # (n, m): n * m small
C_SHAPES = PYTHON_SHAPES + [(2305, 2049), (4353, 4097)]
ALL_PAIRS = [(t, d) for t in S.TRACKS for d in S.DENSITIES]                                        # the dropped ones too
VALUE_SHAPES = [(70, 3), (300, 40), (700, 300), (2305, 2049)]


@pytest.mark.parametrize("track_family", list(S.TRACKS))
def test_the_three_references_agree(track_family):
    assert any(m == 0 for _, m in PYTHON_SHAPES) and any(m > n for n, m in PYTHON_SHAPES)
    assert any(2048 < m <= 4096 for _, m in C_SHAPES) and any(m > 4096 for _, m in C_SHAPES)
    for density_family in S.DENSITIES:
        for n, m in C_SHAPES:
            track, density = S.draw(track_family, density_family, n, m)
            want = S.reference(track, density)
            assert want.shape == (n,) and want.dtype == np.float64
            assert S.same(H.c_mate_correlate(track, density), want), ("C", density_family, n, m)
            if (n, m) in PYTHON_SHAPES:
                got = MO.correlate_track(track.tolist(), density.tolist())
                assert S.same(np.array(got, dtype=np.float64), want), ("Python", density_family, n, m)


def test_same_is_bits_outside_nan_and_positions_inside():
    a = np.array([0.0, 1.5, np.inf, np.nan, 5e-324])
    assert S.same(a, a.copy()) and S.differing(a, a.copy()) == 0
    assert S.same(a, np.array([0.0, 1.5, np.inf, -np.nan, 5e-324]))                 # a NaN's sign and payload are not compared
    quiet = np.array([0x7ff8000000000000, 0xfff8000000000001], dtype=np.uint64).view(np.float64)
    assert S.same(quiet, quiet[::-1])
    for k, other in enumerate((-0.0, np.nextafter(1.5, 2.0), -np.inf, 0.0, 1e-323)):
        b = a.copy()
        b[k] = other
        assert not S.same(b, a) and not S.same(a, b) and S.differing(b, a) == 1, k
    assert not S.same(a[:4], a)


# ---- every wrong variant is caught by the family meant for it -----------------------------------

def _differs(variant, track_family, density_family, n, m):
    track, density = S.draw(track_family, density_family, n, m)
    want = S.reference(track, density)
    got = S.VARIANTS[variant](track, density)
    assert got.shape == want.shape
    return S.differing(got, want)


def test_fused_is_caught_by_uniform_times_normalised():
    # 40 taps, each product and each sum inexact: a tenth of the outputs is far below what one rounding less per tap moves
    assert _differs("fused", "uniform", "normalised", 300, 40) > 30
    assert _differs("fused", "uniform", "signed", 300, 40) > 30


def test_flushed_is_caught_by_both_subnormal_draws():
    rng = np.random.default_rng(11)
    scaled, bits = S.subnormal_scaled(rng, 300), S.subnormal_bits(rng, 300)
    tiny = np.finfo(np.float64).tiny
    assert (scaled[scaled != 0] >= tiny).mean() > 0.9                 # normal inputs: only their products are subnormal
    assert (np.abs(bits) < tiny).all() and (bits < 0).any() and (bits > 0).any()
    taps_tiny, taps_unit = S.tiny(rng, 40), S.zeros_and_ones(rng, 40)
    for track, density in ((scaled, taps_tiny), (bits, taps_unit)):
        want = S.reference(track, density)
        assert not np.isnan(want).any()
        assert S.differing(S.flushed(track, density), want) > 30
    # and both draws come out of the family as the sweep uses it
    drawn = [S.subnormal(np.random.default_rng(s), 50) for s in range(16)]
    assert any((np.abs(t) < tiny).all() for t in drawn) and any((t >= tiny).any() for t in drawn)


def test_padded_is_caught_by_nonfinite_taps_near_the_end_of_the_track():
    for n, m in ((290, 40), (295, 40), (2304, 2049), (30, 40), (40, 40)):
        assert n < m + 256
        assert _differs("padded", "uniform", "nonfinite_taps", n, m) > 0, (n, m)
    assert _differs("padded", "uniform", "normalised", 300, 40) == 0         # on finite taps the padding adds 0.0: invisible


def test_reversed_order_is_caught():
    assert _differs("reversed_order", "uniform", "normalised", 300, 40) > 30
    assert _differs("reversed_order", "overflow", "normalised", 300, 40) > 30
    assert _differs("reversed_order", "overflow", "zeros_and_ones", 300, 40) > 30      # an overflow met early stays, met late may not


@pytest.mark.parametrize("m", [2049, 4097])
def test_no_carry_is_caught_past_a_pass(m):
    n = m + 256
    for track_family, density_family in (("uniform", "normalised"), ("wiggle", "normalised"), ("near_one", "signed")):
        assert _differs("no_carry", track_family, density_family, n, m) > 30, (track_family, density_family)
    assert _differs("no_carry", "uniform", "normalised", 2048, m) == 0                 # no output has more than one pass of taps


def test_where_fused_and_flushed_do_not_show():
    """Why the families are several: a fused multiply-add is invisible where every product is exact (taps of 0 and 1, whatever
    the track), flushing where nothing is subnormal (the normal-range tracks with any finite taps)."""
    for track_family in S.TRACKS:
        if (track_family, "zeros_and_ones") in S.PAIRS:
            assert _differs("fused", track_family, "zeros_and_ones", 120, 40) == 0, track_family
    for track_family in ("wiggle", "uniform", "near_one", "overflow"):
        for density_family in ("normalised", "tiny", "signed", "zeros_and_ones"):
            if (track_family, density_family) in S.PAIRS:
                assert _differs("flushed", track_family, density_family, 300, 40) == 0, (track_family, density_family)


# ---- NaN caps: a NaN is compared by position only, so the families must not drown in them -------

def test_nan_caps():
    for n, m in VALUE_SHAPES:
        for track_family, density_family in S.PAIRS:
            track, density = S.draw(track_family, density_family, n, m)
            share = np.isnan(S.reference(track, density)).mean()
            where = (track_family, density_family, n, m, share)
            if not {track_family, density_family} & {"nonfinite", "nonfinite_taps", "overflow"}:
                assert share == 0, where
            if track_family == "nonfinite" and density_family in ("normalised", "signed"):
                assert share <= 0.5, where
            if track_family == "overflow":
                assert share <= 0.5, where
    assert S.DROPPED == {("overflow", "signed"), ("overflow", "nonfinite_taps")}
    assert len(S.PAIRS) == len(ALL_PAIRS) - len(S.DROPPED) and not set(S.PAIRS) & S.DROPPED


def test_nonfinite_track_touches_at_most_a_third():
    for n, m in VALUE_SHAPES + [(9, 0), (1, 5)]:
        track = S.nonfinite(np.random.default_rng(3), n, m)
        bad = np.flatnonzero(~np.isfinite(track))
        assert bad.tolist() == list(range(0, n, 3 * max(m, 1)))
        touched = np.zeros(n, dtype=bool)
        for p in bad:
            touched[max(0, p - max(m, 1) + 1):p + 1] = True
        assert touched.sum() * 3 <= n + 2 * max(m, 1)


# ---- shapes --------------------------------------------------------------------------------------

def test_lengths_reach_the_edges():
    for m in S.M:
        ns = S.lengths(m)
        assert ns == sorted(set(ns)) and ns[0] >= 1 and ns[-1] <= S.N_MAX
        if m >= 64:
            assert len(ns) >= 30, m
        if 1 <= m <= S.N_MAX - 1:
            assert {m - 1, m, m + 1} - {0} <= set(ns)                           # n < m, n == m, n > m
        for wave_edge in (64, 128, 192, 256, 512):                               # the end of the track at lanes 63, 0 and 1 of a wave
            assert {wave_edge - 1, wave_edge, wave_edge + 1} <= set(ns)
        assert {S.PASS, S.PASS + 1, 2 * S.PASS, 2 * S.PASS + 1} <= set(ns)       # n one more than a pass
    for m in (2049, 4097, 6145):                                                 # the pass edge inside a workgroup
        ns = S.lengths(m)
        for edge in (S.PASS - 1, S.PASS, S.PASS + 1):
            assert any(n >= edge and (n - edge) % S.GROUP == 0 for n in ns), (m, edge)
        # and a workgroup whose waves split between the plain and the masked loop of the second pass: the end of the track
        # between 1 and 255 outputs behind the point where an output has all m taps
        assert any(0 < (n - m) % S.GROUP < S.GROUP - S.WAVE for n in ns if n > m), m


def test_the_sweep_uses_every_pair():
    assert S.pairs_of_sweep() == set(S.PAIRS)
    for m in S.M:
        cases = S.sweep(m)
        assert [n for n, _, _ in cases] == S.lengths(m)
        if m >= 64:
            assert {(t, d) for _, t, d in cases} == set(S.PAIRS), m
    t1, d1 = S.draw("near_one", "signed", 100, 7)
    t2, d2 = S.draw("near_one", "signed", 100, 7)
    assert np.array_equal(t1.view(np.uint64), t2.view(np.uint64)) and np.array_equal(d1.view(np.uint64), d2.view(np.uint64))
    assert any(S.draw("near_one", "normalised", 50, 3, seed=s)[0][-1] == 1.0 for s in range(8))       # a track that ends in 1


# ---- the wrapper ---------------------------------------------------------------------------------

class _StubContext:
    def mate_correlate(self, track, density):
        return S.reference(track, density)


@pytest.fixture
def mp(monkeypatch):
    from xenomapper_amd import mappability
    monkeypatch.setattr(mappability, "default_context", lambda: _StubContext())
    return mappability


def _typed(values):
    return [(type(v), repr(v)) for v in values]


def test_wrapper_keeps_the_integer_tail_of_a_short_track(mp):
    m = mp.Mappability(chromosome_sizes={'a': 5})
    m['a'] = [0, 1, 0.5]
    paired = m.single_end_to_paired([0.5, 0.5])
    assert dict(paired) == {'a': [0.5, 1.0, 0.25, 0, 0]}
    assert _typed(paired['a']) == _typed([0.5, 1.0, 0.25, 0, 0])                 # the tail is the integer 0 of [0] * size
    assert m['a'] == [0, 1, 0.5]


def test_wrapper_raises_for_a_long_track(mp):
    m = mp.Mappability(chromosome_sizes={'a': 2})
    m['a'] = [0, 1, 0.5]
    with pytest.raises(IndexError):
        m.single_end_to_paired([0.5, 0.5])


def test_wrapper_empty_track_and_mixed_types(mp):
    m = mp.Mappability(chromosome_sizes={'a': 0, 'b': 3})
    assert m['a'] == []
    m['b'] = [True, 2, -0.0]
    paired = m.single_end_to_paired([1])
    assert paired['a'] == []
    assert _typed(paired['b']) == _typed([1.0, 2.0, 0.0])
    assert isinstance(paired, mp.Mappability) and paired.chromosome_sizes == {'a': 0, 'b': 3}
