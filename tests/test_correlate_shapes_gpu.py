"""The catalogue of tests/correlate_shapes.py through the mate-density correlation kernel (K4, mate_correlate_kernel), by its
host entry (xm_mate_correlate: Context.mate_correlate) and its device entry (xm_mate_correlate_dev), every result against
the column-wise numpy loop under correlate_shapes.same(): NaN by position, every other output by its 64 bits.

tests/test_correlate_shapes_cpu.py proves, without a GPU, that this reference is the Python loop and the C oracle bit for bit,
that the lengths put the end of the track at the wave, workgroup and pass edges, and that a fused multiply-add, flushed
subnormals, taps run over the padding behind the track, another summation order and a lost carry between passes each change
the outputs of the family named for it -- so a kernel with one of these mistakes fails here."""
import ctypes

import numpy as np
import pytest

from tests import correlate_shapes as S
from tests import helpers as H

pytestmark = pytest.mark.gpu

SENTINEL = 0x5EA71E55C0DED00D            # a finite binary64 pattern no result of these inputs has
GUARD = 300                              # elements of sentinel / NaN on each side: more than a workgroup's 256 outputs


@pytest.fixture(scope="module")
def ctx():
    from xenomapper_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


def check(ctx, track, density, what):
    got = ctx.mate_correlate(track, density)
    want = S.reference(track, density)
    assert got.dtype == np.float64 and got.shape == want.shape, what
    assert S.same(got, want), "%r: %d of %d outputs differ, first at %d" % (
        what, S.differing(got, want), want.shape[0], _first_difference(got, want))


def _first_difference(got, want):
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    bad = (nan_g != nan_w) | (~nan_g & ~nan_w & (got.view(np.uint64) != want.view(np.uint64)))
    return int(np.flatnonzero(bad)[0]) if bad.any() else -1


@pytest.mark.parametrize("m", S.M)
def test_every_length_at_these_taps(ctx, m):
    assert S.pairs_of_sweep() == set(S.PAIRS)                        # over the sweep every pair of families is used
    cases = S.sweep(m)
    assert [n for n, _, _ in cases] == S.lengths(m)
    for n, track_family, density_family in cases:
        track, density = S.draw(track_family, density_family, n, m)
        check(ctx, track, density, (n, m, track_family, density_family))


@pytest.mark.parametrize("n,m", [(700, 300), (2305, 2049)])
def test_value_families(ctx, n, m):
    for track_family in S.TRACKS:
        for density_family in S.DENSITIES:                           # the two NaN-heavy pairs the sweep leaves out as well
            track, density = S.draw(track_family, density_family, n, m, seed=1)
            check(ctx, track, density, (n, m, track_family, density_family))
    rng = np.random.default_rng(2)
    for track in (S.subnormal_scaled(rng, n), S.subnormal_bits(rng, n)):                 # both draws, whatever the family chose
        for density in (S.tiny(rng, m), S.zeros_and_ones(rng, m)):
            check(ctx, track, density, (n, m, "subnormal draws"))
    track = S.near_one(rng, n)
    track[-1] = 1.0                                                  # a track whose last element is 1
    check(ctx, track, S.signed(rng, m), (n, m, "ends in 1"))


# ---- the device entry: caller pointers, a stream of its own, guards all round -------------------

def _bits(t):
    import torch
    return t.view(torch.int64)


class _DeviceCase:
    """out inside a tensor of sentinels; track and density inside tensors of NaN, each `off` elements from its start."""

    def __init__(self, track, density, offs):
        import torch
        n, m = track.shape[0], density.shape[0]
        self.n, self.m, (to, do, oo) = n, m, offs
        host_t = np.full(to + n + GUARD, np.nan)
        host_t[to:to + n] = track
        host_d = np.full(do + m + GUARD, np.nan)
        host_d[do:do + m] = density
        self.buf_t = torch.from_numpy(host_t).cuda()
        self.buf_d = torch.from_numpy(host_d).cuda()
        self.buf_o = torch.full((GUARD + oo + n + GUARD,), SENTINEL, dtype=torch.int64, device="cuda").view(torch.float64)
        self.track, self.density = self.buf_t[to:to + n], self.buf_d[do:do + m]
        self.lo = GUARD + oo
        self.out = self.buf_o[self.lo:self.lo + n]
        assert all(t.data_ptr() % 16 == 0 for t in (self.buf_t, self.buf_d, self.buf_o))
        for t, off in ((self.track, to), (self.density, do), (self.out, self.lo)):
            assert t.data_ptr() % 16 == (8 if off % 2 else 0) and t.is_contiguous()
        self.before_t, self.before_d = _bits(self.buf_t).clone(), _bits(self.buf_d).clone()

    def guards_intact(self, written):
        import torch
        o = _bits(self.buf_o).cpu().numpy()
        assert (o[:self.lo] == SENTINEL).all() and (o[self.lo + written:] == SENTINEL).all(), "sentinels outside out[0:n]"
        assert torch.equal(_bits(self.buf_t), self.before_t) and torch.equal(_bits(self.buf_d), self.before_d), "inputs changed"

    def result(self):
        return self.out.cpu().numpy()


DEVICE_CASES = [((1, 1), "uniform", "normalised", (0, 0, 0)),
                ((257, 65), "near_one", "signed", (1, 3, 1)),
                ((2305, 2049), "nonfinite", "normalised", (3, 1, 3)),
                ((4353, 4097), "uniform", "signed", (1, 0, 3)),
                ((257, 65), "subnormal", "tiny", (3, 3, 0)),
                ((2305, 2049), "uniform", "nonfinite_taps", (0, 1, 1))]


def test_device_entry_with_guards_on_a_side_stream(ctx):
    import torch
    assert {shape for shape, _, _, _ in DEVICE_CASES} == {(1, 1), (257, 65), (2305, 2049), (4353, 4097)}
    assert {o for _, _, _, offs in DEVICE_CASES for o in offs} == {0, 1, 3}
    side = torch.cuda.Stream()
    assert side.cuda_stream != torch.cuda.current_stream().cuda_stream
    for (n, m), track_family, density_family, offs in DEVICE_CASES:
        track, density = S.draw(track_family, density_family, n, m, seed=2)
        case = _DeviceCase(track, density, offs)
        torch.cuda.synchronize()                                    # the buffers were filled on torch's own stream
        ctx.mate_correlate_dev(case.track, case.density, case.out, stream=side)
        side.synchronize()
        what = (n, m, track_family, density_family, offs)
        case.guards_intact(n)
        got, want = case.result(), S.reference(track, density)
        assert S.same(got, want), "%r: %d outputs differ, first at %d" % (what, S.differing(got, want), _first_difference(got, want))
        if "nonfinite" not in track_family + density_family:
            assert not np.isnan(got).any(), what                    # nothing from behind the inputs reached an output


def _raw_call(ctx, stream, n, case, m):
    P = ctypes.c_void_p
    return ctx._L.xm_mate_correlate_dev(ctx._h, P(stream.cuda_stream), n, P(case.track.data_ptr()), m,
                                        P(case.density.data_ptr()), P(case.out.data_ptr()))


def test_device_entry_empty_track_no_taps_and_oversized(ctx):
    import torch
    side = torch.cuda.Stream()
    track, density = S.draw("near_one", "signed", 700, 65, seed=3)
    track[5], track[-1] = 1.0, 1.0
    # n = 0: fine, and nothing is touched
    case = _DeviceCase(track, density, (1, 1, 1))
    torch.cuda.synchronize()
    assert _raw_call(ctx, side, 0, case, 65) == 0
    side.synchronize()
    case.guards_intact(0)
    # n = 2^40 + 1: refused before any launch
    rc = _raw_call(ctx, side, (1 << 40) + 1, case, 65)
    assert rc == -1
    with pytest.raises(ValueError):
        ctx._check(rc, "xm_mate_correlate_dev")
    side.synchronize()
    case.guards_intact(0)
    # m = 0: where(track == 1, 1, 0.0) -- through both entries
    ctx.mate_correlate_dev(case.track, case.density[:0], case.out, stream=side)
    side.synchronize()
    case.guards_intact(700)
    want = np.where(track == 1.0, 1.0, 0.0)
    assert want.sum() >= 2 and S.same(S.reference(track, density[:0]), want)
    assert S.same(case.result(), want)
    assert S.same(ctx.mate_correlate(track, density[:0]), want)
    # and the context is as good as before
    ctx.mate_correlate_dev(case.track, case.density, case.out, stream=side)
    side.synchronize()
    case.guards_intact(700)
    assert S.same(case.result(), S.reference(track, density))


# ---- the host entry's scratch buffers ------------------------------------------------------------

def test_host_entry_scratch_is_reused_cleanly(ctx):
    from xenomapper_amd import _ffi
    big_a = S.draw("uniform", "normalised", 5000, 3000, seed=4)
    small = S.draw("near_one", "signed", 10, 2, seed=4)
    big_b = S.draw("nonfinite", "signed", 5000, 3000, seed=5)
    check(ctx, *big_a, "first large call")                         # sizes the scratch buffers
    pinned = _ffi.pinned_bytes()
    check(ctx, *small, "small call on large buffers")              # stale track, taps and outputs lie behind its own
    check(ctx, *big_b, "large call again, other contents")
    check(ctx, *big_a, "and the first again")
    assert _ffi.pinned_bytes() == pinned


def test_large_track_against_the_c_oracle(ctx):
    """More workgroups (3907) than the chip holds at once, on the family in which a fused multiply-add shows in a third of the
    outputs, not in 1 % of them."""
    n, m = 1000003, 65
    track, density = S.draw("uniform", "normalised", n, m, seed=6)
    got = ctx.mate_correlate(track, density)
    want = H.c_mate_correlate(track, density)
    assert S.same(got, want), "%d outputs differ, first at %d" % (S.differing(got, want), _first_difference(got, want))
    assert S.same(S.reference(track, density), want)
