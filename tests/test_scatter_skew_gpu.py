"""The catalogue of tests/scatter_skew_shapes.py through xm_classify_compact_dev with the compact stream (K1 + K2b + K2c, whose
scatter takes a strictly interleaved granule in its skew form: a dominant bin by ballots, all other slots through a table),
against the C oracle (oracle/xm_oracle.c: xmo_classify_* + xmo_compact) and against the same call made with category bytes,
which goes through the scatter that form does not touch.  Every case, no sampling.  Nothing is stored behind the last unit.
tests/test_scatter_skew_cpu.py proves, without a GPU, that the catalogue reaches the counts and placements it is named after."""
import numpy as np
import pytest

from tests import helpers as H
from tests import runs_shapes as S
from tests import scatter_skew_shapes as K

pytestmark = pytest.mark.gpu

SENTINEL = -0x12345678


@pytest.fixture(scope="module")
def ctx():
    from xenomapper_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


def run(ctx, mode, d, dbits, m, n, with_bins4):
    import torch
    from xenomapper_amd import _ffi
    dev = torch.device("cuda:0")
    code = None if with_bins4 else torch.full((n + 16,), 0xEE, dtype=torch.uint8, device=dev)
    bins4 = torch.full((_ffi.bins4_bytes(n),), 0xEE, dtype=torch.uint8, device=dev) if with_bins4 else None
    idx = torch.full((n,), SENTINEL, dtype=torch.int32, device=dev)
    off = torch.full((8,), -1, dtype=torch.int64, device=dev)
    counts = torch.full((64,), -1, dtype=torch.int64, device=dev)
    ctx.classify_compact_dev(mode, *d, dbits, m, code, idx, off, counts, bins4=bins4)
    torch.cuda.synchronize()
    got_bins = _ffi.unpack_bins4(bins4.cpu().numpy(), n) if with_bins4 else None
    return idx.cpu().numpy(), off.cpu().numpy().astype(np.uint64), counts.cpu().numpy().astype(np.uint64), got_bins


def check_case(ctx, name, mode, cols, flags, m):
    import torch
    dev = torch.device("cuda:0")
    n = flags.shape[0]
    bits = S.pack_bits(flags)
    want_code, want_counts = H.c_classify(mode, *cols, bits, m)
    want_idx, want_off = H.c_compact(mode, want_code)
    want_bins = S.bins_of_records(n, want_idx, want_off)
    units = int(want_off[7])
    d = [torch.from_numpy(np.ascontiguousarray(c)).to(dev) for c in cols]
    dbits = torch.from_numpy(np.ascontiguousarray(bits).view(np.int64)).to(dev)
    idx, off, counts, bins = run(ctx, mode, d, dbits, m, n, True)
    assert np.array_equal(counts, want_counts), name
    assert np.array_equal(off, want_off), name
    assert np.array_equal(bins, want_bins), name
    wrong = np.flatnonzero(idx[:units].view(np.uint32) != want_idx)
    assert wrong.size == 0, (name, "first wrong place", int(wrong[0]), "of", units)
    assert (idx[units:] == SENTINEL).all(), (name, "stored behind the last unit")
    idx_b, off_b, counts_b, _ = run(ctx, mode, d, dbits, m, n, False)        # category bytes: the scatter without the skew form
    assert np.array_equal(off_b, want_off) and np.array_equal(counts_b, want_counts), name
    assert np.array_equal(idx_b, idx), (name, "the two scatter forms differ")


@pytest.mark.parametrize("group", K.GROUPS)
def test_skew_catalogue(ctx, group):
    cases = K.group(group)
    assert cases
    for name, mode, cols, flags, m in cases:
        assert name.startswith(group + "/")
        check_case(ctx, name, mode, cols, flags, m)
    assert ctx.workspace_is_clean()
