"""The catalogue of tests/runs_shapes.py through the segmented-lists kernel (K1r: xm_classify_runs_dev, xm_classify_runs_f64_dev)
and, on the same inputs, through xm_classify_compact*_dev with the compact stream (K1 + K2b + K2c), both against the C oracle
(oracle/xm_oracle.c: xmo_classify_* + xmo_compact).  Every case, no sampling: a case that fails in both forms points at the
classification, one that fails in the runs form alone at K1r's own sort (ranks, cross-wave offsets, copy-out).

check_runs (tests/test_runs_gpu.py) also holds the kernel to the header's write contract: nothing is stored past a granule's
units, count 7 is 0, nothing is touched behind the last granule.  tests/test_runs_shapes_cpu.py proves, without a GPU, that the
catalogue reaches the waves, lanes, bins and unit counts each group is named after."""
import numpy as np
import pytest

from tests import helpers as H
from tests import runs_shapes as S
from tests.test_classify_front_record_gpu import check_flat
from tests.test_runs_gpu import check_runs

pytestmark = pytest.mark.gpu

BINS4_ONLY = ((False, True),)


@pytest.fixture(scope="module")
def ctx():
    from xenomapper_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


def oracle(mode, cols, bits, m):
    want_code, want_counts = H.c_classify(mode, *cols, bits, m)
    want_idx, want_off = H.c_compact(mode, want_code)
    n = cols[0].shape[0]
    return want_code, want_counts, want_idx, want_off, S.bins_of_records(n, want_idx, want_off)


def check_case(ctx, name, mode, cols, flags, m):
    bits = S.pack_bits(flags)
    want = oracle(mode, cols, bits, m)
    forms = [(cols, m)]
    if cols[0].dtype == np.int32:
        forms.append((S.as_f64(cols), H.NEG))                       # binary64 columns: the same lists on integral input
    try:
        for c, mm in forms:
            check_runs(ctx, mode, c, bits, mm, want=(want[1], want[2], want[3]))
            check_flat(ctx, mode, c, bits, mm, want, forms=BINS4_ONLY)
    except AssertionError as e:
        raise AssertionError("%s (%s columns): %s" % (name, c[0].dtype, e)) from e


@pytest.mark.parametrize("group", S.GROUPS)
def test_runs_catalogue(ctx, group):
    cases = S.group(group)
    assert cases
    for name, mode, cols, flags, m in cases:
        assert name.startswith(group + "/") and m in (S.ABSENT, H.NEG)
        check_case(ctx, name, mode, cols, flags, m)
    assert ctx.workspace_is_clean()
