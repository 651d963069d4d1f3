"""The catalogue of tests/runs_shapes.py without a GPU: it reaches the waves, lanes, bins and unit counts it claims (conditions
on the catalogue, stated with the model of K1r's waves and the C oracle's bins, never with the code under test), and the two
expanders of the segmented form -- xm_runs_expand of the C ABI (host code of libxenomapper_hip.so) and the NumPy one -- give the
oracle's lists from the reference segmenter's arrays.  Then xm_runs_expand's refusals, capacity rule and count-only call."""
import ctypes

import numpy as np
import pytest

from tests import helpers as H
from tests import runs_shapes as S

GRAN, WAVE = S.GRAN, S.WAVE


def _oracle(mode, cols, flags, m):
    want_code, want_counts = H.c_classify(mode, *cols, S.pack_bits(flags), m)
    want_idx, want_off = H.c_compact(mode, want_code)
    return want_counts, want_idx, want_off


@pytest.fixture(scope="module")
def catalogue():
    """name -> what the oracle and the model say about the case (the columns themselves are not kept)."""
    out = {}
    for name, mode, cols, flags, m in S.all_shapes():
        n = flags.shape[0]
        assert name not in out and all(c.shape[0] == n for c in cols)
        assert cols[0].dtype == (np.float64 if name.startswith("nan/") else np.int32)
        want_counts, want_idx, want_off = _oracle(mode, cols, flags, m)
        bins = S.bins_of_records(n, want_idx, want_off)
        model = S.WaveModel(mode, flags)
        assert np.array_equal(bins != 7, model.unit[:n])           # the model's units are the oracle's
        padded = np.full(model.n_gran * GRAN, 7, dtype=np.uint8)
        padded[:n] = bins
        gran_bins = np.stack([np.bincount(g, minlength=8) for g in padded.reshape(-1, GRAN)])      # [granule][bin 0..7]
        assert np.array_equal(gran_bins[:, :7].sum(axis=1), model.gran_units)
        out[name] = dict(mode=mode, n=n, idx=want_idx, off=want_off, bins=padded, gran_bins=gran_bins, model=model)
    return out


def _of(catalogue, prefix):
    hit = {k: v for k, v in catalogue.items() if k.startswith(prefix)}
    assert hit, prefix
    return hit


def test_groups_are_the_catalogue():
    names = [c[0] for c in S.all_shapes()]
    assert len(names) == len(set(names)) == sum(len(S.group(g)) for g in S.GROUPS)
    assert len(S.TWO_BIN_GROUPS) == 3 * len(S.TWO_BIN_K) and all(len(S.group(g)) == 30 for g in S.TWO_BIN_GROUPS)
    assert S.TWO_BIN_K == (1, 2, 63, 64, 65, 127, 128, 255, 256, 257, 511, 512, 1023)
    assert S.UNIT_COUNTS == (0, 1, 7, 8, 9, 15, 16, 17, 2047, 2048)


def test_interleaved_waves_hold_many_bins(catalogue):
    """Every interleaved case (and so both paired modes) has an interleaved wave whose units fall in three bins or more, with a
    lane whose two units share a bin and a lane whose two units differ."""
    for name, c in _of(catalogue, "interleaved/").items():
        m, found = c["model"], 0
        assert m.inter[:8 * (c["n"] // GRAN)].all(), name
        for w in np.flatnonzero(m.inter & m.has_unit):
            lanes = c["bins"][w * WAVE:(w + 1) * WAVE].reshape(-1, 4)
            two = lanes[(lanes[:, 1] != 7) & (lanes[:, 3] != 7)]
            units = lanes[lanes != 7]
            if len(set(units.tolist())) >= 3 and (two[:, 1] == two[:, 3]).any() and (two[:, 1] != two[:, 3]).any():
                found += 1
        assert found >= 1, (name, found)


def test_mixed_cases_hold_both_wave_classes_in_either_order(catalogue):
    for name, c in _of(catalogue, "mixed/placed").items():
        m = c["model"]
        orders = [m.wave_orders(g) for g in range(m.n_gran)]
        assert any(o[0] for o in orders) and any(o[1] for o in orders), (name, orders)
        assert orders[1] == (False, True), name                    # granule 1: the shifted waves in front, purely
        for w in S.MIXED_EMPTY_WAVES:                              # a wave without a unit between two that hold units
            assert not m.has_unit[w] and m.has_unit[w - 1] and m.has_unit[w + 1] and (w - 1) // 8 == (w + 1) // 8, (name, w)
    for name, c in _of(catalogue, "mixed/placed/").items():
        assert c["model"].wave_orders(0) == (True, False), name     # granule 0: the interleaved waves in front, purely
    for prefix in ("mixed/placed_triples/", "mixed/random_s0_t0.2/"):
        for name, c in _of(catalogue, prefix).items():
            assert (c["model"].lane_units == 3).any(), name         # three units in a lane
    for name, c in _of(catalogue, "mixed/sparse_singles/").items():
        m = c["model"]
        assert sum(1 for g in range(m.n_gran) if any(m.wave_orders(g))) >= 2, name
    for name, c in _of(catalogue, "mixed/").items():               # the units of the flat cases fall in many bins
        assert not name.endswith("/flat") or (c["gran_bins"][:2, :6] > 0).sum(axis=1).min() >= 4, name


def test_unit_counts_per_granule(catalogue):
    for name, c in _of(catalogue, "counts/").items():
        tail = name.split("/")[1]
        want = [2047] + [u for u in S.UNIT_COUNTS if u != 2047] + [{"tail_empty": 0, "tail1": 1, "tail2047": 2047}[tail]]
        assert c["model"].gran_units.tolist() == want, name
        assert set(S.UNIT_COUNTS) <= set(want)
        assert c["n"] % GRAN == S.COUNT_TAILS[tail]
    assert {k.split("/")[1] for k in _of(catalogue, "counts/")} == set(S.COUNT_TAILS)
    assert {(k.split("/")[2], k.split("/")[3]) for k in _of(catalogue, "counts/")} == {
        ("m%d" % m, s) for m in (0, 1, 2) for s in ("flat", "skew0")}


def test_two_bin_sweep_gives_the_intended_counts(catalogue):
    seen = set()
    for name, c in _of(catalogue, "two_bins/").items():
        _, mode, k, ab = name.split("/")
        mode, k, a, b = int(mode[1:]), int(k[1:]), int(ab[1]), int(ab[3])
        assert mode == c["mode"] and a != b
        units = c["model"].gran_units
        assert units.tolist() == ([GRAN, GRAN, 77] if mode == 0 else [GRAN // 2, GRAN // 2, 38])
        want = np.zeros((3, 8), dtype=np.int64)
        want[:, a] = np.minimum(k, units)
        want[:, b] = units - want[:, a]
        want[:, 7] = GRAN - units
        assert np.array_equal(c["gran_bins"], want), name
        if mode:
            assert c["model"].inter.all(), name
        seen.add((mode, k, a, b))
    assert seen == {(mode, k, a, b) for mode in (0, 1, 2) for k in S.TWO_BIN_K for a in range(6) for b in range(6) if a != b}


def test_every_bin_alone_and_every_bin_missing(catalogue):
    alone, missing = set(), set()
    for name, c in _of(catalogue, "one_bin/").items():
        for row in c["gran_bins"][:2]:                              # the two full granules
            present = frozenset(np.flatnonzero(row[:7]).tolist())
            if len(present) == 1:
                alone.add((c["mode"], min(present)))
            if len(present) == 5 and present < frozenset(range(6)):
                missing.add((c["mode"], min(frozenset(range(6)) - present)))
    everything = {(mode, b) for mode in (0, 1, 2) for b in range(6)}
    assert alone == everything and missing == everything


def test_bin_6_in_every_mode(catalogue):
    for name, c in _of(catalogue, "nan/").items():
        six = c["gran_bins"][:, 6]
        assert (six > 0).all(), name                                # every granule, the ragged one included
        for r in S.NAN_PLACES:
            assert c["bins"][r] in (6, 7), (name, r)                # a NaN record that closes a unit is in bin 6
        others = (c["gran_bins"][:2, :6] > 0).sum(axis=1)
        assert (others >= 4).all() if "/many/" in name else (others == 1).all(), name
        if c["mode"]:
            assert c["model"].inter.all(), name
    assert {c["mode"] for c in _of(catalogue, "nan/many/").values()} == {0, 1, 2}
    assert {c["mode"] for c in _of(catalogue, "nan/only").values()} == {0, 1, 2}


def test_a_wave_of_one_bin_inside_a_granule_of_many(catalogue):
    for name, c in _of(catalogue, "wave_one_bin/").items():
        for w, s in S.WAVE_ONE_BIN:
            units = c["bins"][w * WAVE:(w + 1) * WAVE]
            assert set(units[units != 7].tolist()) == {s}, (name, w)
            assert (c["gran_bins"][w // 8, :6] > 0).sum() >= 4, (name, w)


def test_both_expanders_on_the_reference_segmenter(catalogue):
    """segment() -> np_expand and xm_runs_expand -> the oracle's lists, every case, every bin 0..6."""
    from xenomapper_amd import _ffi
    for name, c in catalogue.items():
        n = c["n"]
        runs16, gcnt = S.segment(n, c["idx"], c["off"])
        g2 = gcnt.reshape(-1, 8)
        assert np.array_equal(g2, c["gran_bins"][:, :8] * (np.arange(8) < 7)), name
        units = g2.sum(axis=1)
        r2 = runs16.reshape(-1, GRAN)
        behind = np.arange(GRAN)[None, :] >= units[:, None]
        assert (r2[behind] == S.PREFILL).all() and (r2[~behind] < GRAN).all(), name
        for b in range(7):
            want = c["idx"][int(c["off"][b]):int(c["off"][b + 1])]
            assert np.array_equal(S.np_expand(n, runs16, gcnt, b), want), (name, b)
            assert np.array_equal(_ffi.runs_expand(n, runs16, gcnt, b), want), (name, b)


# ---- xm_runs_expand through the C ABI ------------------------------------------------------------------------------------

XM_ERR_INVALID_ARG = -1


def _expand(n, runs16, gcnt, b, out, capacity, written=True):
    from xenomapper_amd import _ffi
    P = ctypes.c_void_p
    k = ctypes.c_uint64(0xDEAD)
    rc = _ffi.lib().xm_runs_expand(n, None if runs16 is None else runs16.ctypes.data_as(P),
                                   None if gcnt is None else gcnt.ctypes.data_as(P), b,
                                   None if out is None else out.ctypes.data_as(P), capacity,
                                   ctypes.byref(k) if written else None)
    return rc, k.value


def _small_layout():
    rng = np.random.default_rng(8)
    n = 2 * GRAN + 77
    cols = S.columns_of_states(rng.integers(0, 6, n))
    want_counts, want_idx, want_off = _oracle(0, cols, np.ones(n, dtype=np.uint8), S.ABSENT)
    return (n, want_idx, want_off) + S.segment(n, want_idx, want_off)


def test_runs_expand_refuses_what_the_kernel_cannot_have_written():
    n, _, _, runs16, gcnt = _small_layout()
    out = np.zeros(n, dtype=np.uint32)
    for b in (-1, 7):
        assert _expand(n, runs16, gcnt, b, out, n) == (XM_ERR_INVALID_ARG, 0xDEAD)
    assert _expand(n, runs16, gcnt, 0, out, n, written=False)[0] == XM_ERR_INVALID_ARG
    assert _expand(n, None, gcnt, 0, out, n)[0] == XM_ERR_INVALID_ARG
    assert _expand(n, runs16, None, 0, out, n)[0] == XM_ERR_INVALID_ARG
    bad = gcnt.copy()
    bad[8 + 2] += GRAN + 1 - bad[8:16].sum()                        # granule 1 now sums to 2049
    assert int(bad[8:16].sum()) == GRAN + 1
    for b in range(7):                                              # whichever list is asked for
        assert _expand(n, runs16, bad, b, out, n) == (XM_ERR_INVALID_ARG, 0xDEAD), b
        assert _expand(n, runs16, bad, b, None, 0) == (XM_ERR_INVALID_ARG, 0xDEAD), b
    assert _expand(n, runs16, gcnt, 2, out, n)[0] == 0              # and the counts as they were are fine


def test_runs_expand_capacity_and_count_only():
    n, want_idx, want_off, runs16, gcnt = _small_layout()
    for b in range(7):
        want = want_idx[int(want_off[b]):int(want_off[b + 1])]
        assert _expand(n, runs16, gcnt, b, None, 0) == (0, want.shape[0])               # idx_out NULL: counts only
        assert _expand(n, runs16, gcnt, b, None, n) == (0, want.shape[0])
        for capacity in sorted({0, min(1, want.shape[0]), want.shape[0] // 2, max(want.shape[0] - 1, 0), want.shape[0]}):
            out = np.full(want.shape[0] + 16, 0xA5A5A5A5, dtype=np.uint32)              # guard words behind `capacity`
            assert _expand(n, runs16, gcnt, b, out, capacity) == (0, want.shape[0]), (b, capacity)
            assert np.array_equal(out[:capacity], want[:capacity]) and (out[capacity:] == 0xA5A5A5A5).all(), (b, capacity)
    assert int(want_off[7] - want_off[6]) == 0 and int(want_off[1]) > 4


def test_runs_expand_no_records():
    out = np.full(4, 0xA5A5A5A5, dtype=np.uint32)
    for b in range(7):
        assert _expand(0, None, None, b, out, 4) == (0, 0)
        empty = np.zeros(0, dtype=np.uint16)
        assert _expand(0, empty, empty, b, None, 0) == (0, 0)
    assert (out == 0xA5A5A5A5).all()
