"""xm_mapp_run (include/xenomapper_mappability.h) through _ffi.Mappability on every window of the catalogue (tests/mapp_shapes.py):
every field of the block against the plain-Python model, with the slot's limits met exactly."""
import numpy as np
import pytest

from tests import mapp_shapes as S

pytestmark = pytest.mark.gpu

_CHAINS = {}


def windows_of(shape):
    if shape.name not in _CHAINS:
        _CHAINS[shape.name] = S.chain(shape)[0]
    return _CHAINS[shape.name]


@pytest.fixture(scope="module")
def front_end():
    from xenomapper_amd import _ffi, xenomapper as xm
    fe = _ffi.Mappability(xm.default_context())
    yield fe
    fe.close()


def as_dict(block):
    names = ("first_line", "n_lines", "key_off", "key_len", "starts", "base", "last_pos", "value_off", "n_values")
    return dict(consumed=block.consumed, n_lines=block.n_lines, status=block.status, reason=block.reason, declined_line=block.declined_line,
                n_segments=block.n_segments, n_values=block.n_values, carry_position=block.carry_position,
                carry_settled=int(block.carry_settled), segments=[tuple(int(row[f]) for f in names) for row in block.segments],
                values=block.values.tobytes())


def run(front_end, slot, shape, window, stale=0xA5):
    max_lines, max_values = S.limits(shape, window.want)
    front_end.reserve(slot, max(1, len(window.data)), max_lines, max_values)
    staging = front_end.staging(slot)
    staging[:] = stale                                                # what an earlier, longer window left behind
    staging[:len(window.data)] = np.frombuffer(window.data, dtype=np.uint8)
    return front_end.run(slot, len(window.data), window.eof, window.carry_key, window.carry_position)


@pytest.mark.parametrize("shape", S.SHAPES, ids=lambda s: s.name)
def test_every_window_of_the_catalogue(front_end, shape):
    windows = windows_of(shape)
    assert windows or not shape.text
    for k, window in enumerate(windows):
        try:
            S.compare(window, as_dict(run(front_end, k % 2, shape, window)))
        except AssertionError as exc:
            raise AssertionError("%s, window %d: %s" % (shape.name, k, exc)) from exc


def test_a_declined_window_says_where_and_why(front_end):
    shape = S.BY_NAME["byte_20_second_window"]
    windows = windows_of(shape)
    declined = [w for w in windows if w.want.status == S.DECLINED]
    assert len(declined) == 1 and declined[0] is not windows[0]
    block = run(front_end, 0, shape, declined[0])
    assert (block.status, block.reason, block.declined_line) == (S.DECLINED, S.R_SEPARATOR, declined[0].want.declined_line)
    assert block.consumed == declined[0].want.consumed > 0 and block.n_segments == 0 and block.n_values == 0
    assert block.carry_position == declined[0].carry_position              # the state carried in: nothing was resolved


def test_a_shorter_window_behind_a_longer_one_and_both_slots(front_end):
    long_shape, short_shape = S.BY_NAME["newline_chunk_+1"], S.BY_NAME["two_chromosomes"]
    long_window, short_window = windows_of(long_shape)[0], windows_of(short_shape)[0]
    for slot in (0, 1):
        S.compare(long_window, as_dict(run(front_end, slot, long_shape, long_window)))
    first = run(front_end, 0, short_shape, short_window, stale=ord("\n"))      # line ends behind the window's end must not count
    kept = as_dict(first)
    S.compare(short_window, kept)
    other = S.BY_NAME["unsettled_65_then_g"]
    S.compare(windows_of(other)[0], as_dict(run(front_end, 1, other, windows_of(other)[0])))
    assert as_dict(first) == kept                                     # slot 0's block is valid until slot 0 runs again


def test_pieces_uploaded_ahead_give_the_same_block(front_end):
    shape = S.BY_NAME["lines_%d" % (2048 * S.TILE + 1)]
    window = windows_of(shape)[0]
    max_lines, max_values = S.limits(shape, window.want)
    front_end.reserve(0, len(window.data), max_lines, max_values)
    staging = front_end.staging(0)
    piece = 5 * S.CHUNK + 100
    for at in range(0, len(window.data), piece):
        n = min(piece, len(window.data) - at)
        staging[at:at + n] = np.frombuffer(window.data, dtype=np.uint8, count=n, offset=at)
        front_end.upload(0, at, n)
    S.compare(window, as_dict(front_end.run(0, len(window.data), True, None, 0)))


def test_refused_arguments(front_end):
    from xenomapper_amd import _ffi
    for args in ((2, 100, 10, 10), (-1, 100, 10, 10), (0, _ffi.MAPP_MAX_WINDOW + 1, 10, 10), (0, 100, 0, 10), (0, 100, 1 << 32, 10),
                 (0, 100, 10, _ffi.MAPP_MAX_WINDOW + 1)):
        with pytest.raises(ValueError):
            front_end.reserve(*args)
    front_end.reserve(0, 100, 10, 10)
    with pytest.raises(ValueError):
        front_end.run(0, 1 << 20, True)                               # longer than the slot's window
    with pytest.raises(ValueError):
        front_end.run(2, 10, True)
    with pytest.raises(ValueError):
        front_end.upload(0, 64, 10)                                   # not in order from offset 0
    with pytest.raises(ValueError):
        front_end.upload(0, 0, 1 << 20)
    fresh = _ffi.Mappability(front_end.ctx)
    with pytest.raises(ValueError):
        fresh.run(0, 0, True)                                         # a slot that was never reserved
    fresh.close()
    assert front_end._L.xm_mapp_staging(front_end._h, 5) is None
    block = front_end.run(0, 0, True)                                 # an empty window is a window
    assert (block.status, block.n_lines, block.consumed, block.n_segments) == (0, 0, 0, 0)
