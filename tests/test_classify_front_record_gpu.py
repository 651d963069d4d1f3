"""GPU parity of the classify kernels around the record in front of a workgroup and the unit flags of a wave.

A counting classify workgroup owns 2048 records.  Its first record closes a unit with the LAST record of the workgroup in
front, which the kernel fetches only when that first record's unit flag is set; the flags of a wave's 256 records come
through one scalar 32-byte load in workgroups whose records all exist, and through a byte load per lane in the last,
partial one.  So the cases here sit on the workgroup boundaries (n = 2047 .. 3 * 2048 + 5), with the first records of
workgroups 1 and 2 flagged and not flagged, on int32 and binary64 columns, single-end / liberal / conservative, through
both per-record outputs of the fused call (category bytes, compact stream) and through the segmented-lists call, whose
kernel loads its records the same way.  The checker is the C oracle (oracle/xm_oracle.c: xmo_classify_* + xmo_compact,
restating xenomapper.py:258-289, :402-405, :423-448, :521-550)."""
import numpy as np
import pytest

from tests import helpers as H
from tests.helpers import NEG
from tests.test_runs_gpu import check_runs

pytestmark = pytest.mark.gpu

ABSENT = -2**31
GRAN = 2048
SIZES = [2047, 2048, 2049, 4096, 4097, 3 * GRAN + 5]
# one column row per state 0..5 of get_mapping_state (:258-289) at min_score = -inf
STATE_ROWS = [(5, ABSENT, 1, ABSENT), (1, ABSENT, 5, ABSENT), (5, 5, 1, ABSENT), (1, ABSENT, 5, 5), (5, ABSENT, 5, ABSENT),
              (ABSENT, ABSENT, ABSENT, ABSENT)]


@pytest.fixture(scope="module")
def ctx():
    from xenomapper_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


def random_columns(rng, n, spread=8):
    vals = np.concatenate([[ABSENT, ABSENT], np.arange(-spread, spread + 1)]).astype(np.int64)
    return [vals[rng.integers(0, len(vals), n)].astype(np.int32) for _ in range(4)]


def as_f64(cols):
    return [np.where(c == ABSENT, NEG, c.astype(np.float64)) for c in cols]


def singleton_flags(rng, n, p_single=0.5):
    """Unit flags of a read stream in which a fraction p_single of the reads has no mate: a pair is two adjacent records,
    the second closes the unit; a singleton is one record and closes none."""
    flags = np.zeros(n, dtype=bool)
    at = 0
    while at < n:
        if rng.random() < p_single:
            at += 1
        else:
            if at + 1 < n:
                flags[at + 1] = True
            at += 2
    return flags


def oracle(mode, cols, bits, m):
    want_code, want_counts = H.c_classify(mode, *cols, bits, m)
    want_idx, want_off = H.c_compact(mode, want_code)
    want_bins = np.full(cols[0].shape[0], 7, dtype=np.uint8)
    for b in range(7):
        want_bins[want_idx[int(want_off[b]):int(want_off[b + 1])]] = b
    return want_code, want_counts, want_idx, want_off, want_bins


ALL_FORMS = ((False, True), (True, False), (True, True))           # (category bytes, compact stream bins4)


def check_flat(ctx, mode, cols, bits, m, want, forms=ALL_FORMS):
    """xm_classify_compact*_dev with the compact stream only, the category bytes only, and both, against the oracle."""
    import torch
    from xenomapper_amd import _ffi
    want_code, want_counts, want_idx, want_off, want_bins = want
    dev = torch.device("cuda:0")
    n = cols[0].shape[0]
    d = [torch.from_numpy(np.ascontiguousarray(c)).to(dev) for c in cols]
    dbits = torch.from_numpy(np.ascontiguousarray(bits).view(np.int64)).to(dev)
    for with_code, with_bins4 in forms:
        code = torch.full((n + 16,), 0xEE, dtype=torch.uint8, device=dev) if with_code else None
        bins4 = torch.full((_ffi.bins4_bytes(n),), 0xEE, dtype=torch.uint8, device=dev) if with_bins4 else None
        idx = torch.full((n,), -1, dtype=torch.int32, device=dev)
        off = torch.full((8,), -1, dtype=torch.int64, device=dev)
        counts = torch.full((64,), -1, dtype=torch.int64, device=dev)
        ctx.classify_compact_dev(mode, *d, dbits, m, code, idx, off, counts, bins4=bins4)
        torch.cuda.synchronize()
        what = (mode, n, str(cols[0].dtype), with_code, with_bins4)
        assert np.array_equal(counts.cpu().numpy().astype(np.uint64), want_counts), what
        assert np.array_equal(off.cpu().numpy().astype(np.uint64), want_off), what
        assert np.array_equal(idx[:int(want_off[7])].cpu().numpy().view(np.uint32), want_idx), what
        if with_code:
            assert np.array_equal(code[:n].cpu().numpy(), want_code), what
            assert (code[n:].cpu().numpy() == 0xEE).all(), what
        if with_bins4:
            assert np.array_equal(_ffi.unpack_bins4(bins4.cpu().numpy(), n), want_bins), what
    assert ctx.workspace_is_clean()


def check_everything(ctx, cols, flags, modes=(0, 1, 2), m=NEG):
    bits = H.synth.pack_unit_bits(flags)
    fcols = as_f64(cols)
    for mode in modes:
        mi = H.floor_min_score(m)
        want = oracle(mode, cols, bits, mi)
        check_flat(ctx, mode, cols, bits, mi, want)
        check_flat(ctx, mode, fcols, bits, m, want)                 # binary64 columns: same results on integral input
        check_runs(ctx, mode, cols, bits, mi, want=(want[1], want[2], want[3]))
        check_runs(ctx, mode, fcols, bits, m, want=(want[1], want[2], want[3]))


def masks(rng, n):
    """(name, flags) for one size: singleton streams with every combination of the flags of the first records of
    workgroups 1 and 2, a unit closing at record 1 and none at record 0 (and the flag of record 0 set, which closes
    nothing), all ones, all zero."""
    out = []
    base = singleton_flags(rng, n)
    for first1, first2 in ((0, 0), (1, 0), (0, 1), (1, 1)):
        f = base.copy()
        if n > GRAN:
            f[GRAN] = bool(first1)
        if n > 2 * GRAN:
            f[2 * GRAN] = bool(first2)
        out.append(("singletons first=%d%d" % (first1, first2), f))
        if n <= GRAN:
            break
    f = singleton_flags(rng, n)
    f[0], f[1] = False, True
    out.append(("unit at record 1", f))
    f = f.copy()
    f[0] = True
    out.append(("flag of record 0 set", f))
    out.append(("all ones", np.ones(n, dtype=bool)))
    out.append(("all zero", np.zeros(n, dtype=bool)))
    return out


@pytest.mark.parametrize("n", SIZES)
def test_front_record_sizes(ctx, n):
    rng = np.random.default_rng(n + 7)
    cols = random_columns(rng, n)
    for name, flags in masks(rng, n):
        if n > GRAN and name.startswith("singletons"):
            assert flags[GRAN] == (name[-2] == "1")
        check_everything(ctx, cols, flags, m=NEG if n % 2 else -3.5)


def test_front_record_decides_the_category(ctx):
    """The last record of a workgroup and the first of the next in different states: the unit closed by the first record of
    workgroups 1 and 2 takes its forward state from the fetched record (a fetch left out, or of another record, changes
    the category byte)."""
    n = 3 * GRAN
    state = np.full(n, 4, dtype=np.int64)                          # state 4 everywhere ...
    state[GRAN - 1], state[2 * GRAN - 1] = 1, 3                     # ... but in front of workgroups 1 and 2
    state[GRAN - 2], state[2 * GRAN - 2] = 0, 2
    rows = np.array(STATE_ROWS, dtype=np.int64)
    cols = [rows[state, j].astype(np.int32) for j in range(4)]
    flags = np.zeros(n, dtype=bool)
    flags[[GRAN, 2 * GRAN]] = True
    bits = H.synth.pack_unit_bits(flags)
    want_code, _ = H.c_classify(1, *cols, bits, ABSENT)
    assert int(want_code[GRAN]) == (1 << 3 | 4) and int(want_code[2 * GRAN]) == (3 << 3 | 4)
    check_everything(ctx, cols, flags, modes=(1, 2))
    flags[[GRAN, 2 * GRAN]] = False                                 # and not fetched: nothing closes there
    flags[[GRAN + 1, 2 * GRAN + 1]] = True
    check_everything(ctx, cols, flags, modes=(1, 2))


def test_nan_columns_at_the_boundaries(ctx):
    """binary64 with NaN (state 6, bin 6) in the records around the workgroup boundaries."""
    rng = np.random.default_rng(23)
    n = 2 * GRAN + 9
    cols = as_f64(random_columns(rng, n))
    for c in cols:
        c[rng.random(n) < 0.05] = float("nan")
    cols[0][[GRAN - 1, 2 * GRAN]] = float("nan")
    cols[2][[GRAN - 1, 2 * GRAN]] = float("nan")
    flags = singleton_flags(rng, n)
    flags[[GRAN, 2 * GRAN]] = True
    bits = H.synth.pack_unit_bits(flags)
    for mode in (0, 1, 2):
        want = oracle(mode, cols, bits, NEG)
        assert int(want[3][7] - want[3][6]) > 0                     # the case is exercised
        check_flat(ctx, mode, cols, bits, NEG, want)
        check_runs(ctx, mode, cols, bits, NEG, want=(want[1], want[2], want[3]))


def test_counters_36_slots_three_granules(ctx):
    """Three granules whose units fall into all 36 categories (forward state x reverse state, 0..5 each); the counting
    workspace is in its between-calls state after a normal call and after a call on no records."""
    rng = np.random.default_rng(36)
    n = 3 * GRAN
    rows = np.array(STATE_ROWS, dtype=np.int64)
    cols = [rows[rng.integers(0, 6, n), j].astype(np.int32) for j in range(4)]
    flags = np.ones(n, dtype=bool)
    bits = H.synth.pack_unit_bits(flags)
    for mode in (1, 2):
        want = oracle(mode, cols, bits, ABSENT)
        assert int((want[1] > 0).sum()) == 36 and int(want[1].sum()) == n - 1
        for g in range(3):                                          # every granule holds all 36
            assert len(set(want[0][max(g * GRAN, 1):(g + 1) * GRAN].tolist())) == 36
        check_flat(ctx, mode, cols, bits, ABSENT, want)
        assert ctx.workspace_is_clean()
        empty = [np.zeros(0, dtype=np.int32) for _ in range(4)]
        _, idx, off, counts = ctx.classify_compact(mode, *empty, np.zeros(1, dtype=np.uint64), ABSENT)
        assert idx.shape[0] == 0 and not off.any() and not counts.any()
        assert ctx.workspace_is_clean()
        check_flat(ctx, mode, cols, bits, ABSENT, want)             # and the next call counts from zero
