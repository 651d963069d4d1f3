"""The catalogue of tests/scatter_skew_shapes.py without a GPU: it reaches every count and placement it claims (conditions stated
with the model of the skew form's tiles and the C oracle's bins, never with the code under test), and the oracle's lists on it
are what a plain stable split of the record numbers by bin gives."""
import numpy as np
import pytest

from tests import helpers as H
from tests import runs_shapes as S
from tests import scatter_skew_shapes as K


@pytest.fixture(scope="module")
def catalogue():
    out = {}
    for name, mode, cols, flags, m in K.all_shapes():
        n = flags.shape[0]
        assert name not in out and mode in K.MODES and m == S.ABSENT
        assert all(c.shape[0] == n and c.dtype == np.int32 for c in cols)
        want_code, want_counts = H.c_classify(mode, *cols, S.pack_bits(flags), m)
        want_idx, want_off = H.c_compact(mode, want_code)
        bins = S.bins_of_records(n, want_idx, want_off)
        out[name] = dict(mode=mode, n=n, flags=flags, idx=want_idx, off=want_off, bins=bins, model=K.Model(n, bins))
    return out


def _of(catalogue, prefix, suffix=""):
    hit = {k: v for k, v in catalogue.items() if k.startswith(prefix) and k.endswith(suffix)}
    assert hit, prefix
    return hit


def test_groups_are_the_catalogue(catalogue):
    assert len(catalogue) == sum(len(K.group(g)) for g in K.GROUPS)
    assert K.RARE_COUNTS == (0, 1, 63, 64, 65, 127, 128, 129, 255, 256)
    assert K.N == 2 * 2048 + 77 and K.TILE == 512
    for g in K.GROUPS:
        for mode in K.MODES:                                              # both pair rules in every group
            assert any(c["mode"] == mode for c in _of(catalogue, g + "/").values()), (g, mode)
    sizes = {c["n"] for c in catalogue.values()}
    assert sizes == {K.N, K.TILE}


def test_oracle_lists_are_a_stable_split(catalogue):
    for name, c in catalogue.items():
        off = c["off"].astype(np.int64)
        assert off[0] == 0 and off[7] == (c["bins"] != 7).sum(), name
        for b in range(7):
            assert np.array_equal(c["idx"][off[b]:off[b + 1]], np.flatnonzero(c["bins"] == b).astype(np.uint32)), (name, b)


def test_units_close_where_the_flags_say(catalogue):
    """A unit closes at every flagged record but record 0, in the bin the catalogue chose for it (the interleaved groups)."""
    for name, c in catalogue.items():
        unit = c["flags"].astype(bool).copy()
        unit[0] = False
        assert np.array_equal(c["bins"] != 7, unit), name
        if not name.startswith("fallback/"):
            assert not unit[0::2].any() and c["model"].skew.all(), name


def test_counts_reach_every_rare_count(catalogue):
    for mode in K.MODES:
        for kind, d in (("one", 0), ("all", 2)):
            for r in K.RARE_COUNTS:
                c = catalogue["counts/R%d/%s/m%d" % (r, kind, mode)]
                m = c["model"]
                assert m.n_gran == 3 and m.dominant(0) == d and m.dominant(1) == d
                for g in (0, 1):
                    for t in range(K.TILES):
                        want = r if (t or r <= 128) else 0
                        assert m.rare(g, t) == want, (r, kind, mode, g, t)
                        held = set(m.table(g, t)[1].tolist())
                        assert len(held) == (min(want, 1) if kind == "one" else min(want, 5))
                # the tail: 38 units, and no unit in most lanes' first slots: "no unit" is the dominant bin there
                assert m.dominant(2) == 7 and m.rare(2, 0) == 38 and m.rare(2, 1) == 0
                if r <= 128:
                    one = catalogue["counts/R%d/%s/tile/m%d" % (r, kind, mode)]["model"]
                    assert one.n_gran == 1 and one.dominant(0) == d and one.rare(0, 0) == r
                else:
                    assert "counts/R%d/%s/tile/m%d" % (r, kind, mode) not in catalogue


def test_lanes_reach_every_pattern(catalogue):
    for name, c in _of(catalogue, "lanes/").items():
        m = c["model"]
        d = 1 if "/one/" in name else 0
        for g in range(1 if "/tile/" in name else 2):
            assert m.dominant(g) == d
            for t in range(1 if "/tile/" in name else K.TILES):
                assert m.lane_patterns(g, t) == set(range(16)), (name, g, t)
        bins_held = set(m.table(0, 0)[1].tolist())
        assert len(bins_held) == (1 if "/one/" in name else 5)


def test_edges(catalogue):
    for mode in K.MODES:
        m = catalogue["edges/lane/tile/m%d" % mode]["model"]
        at, bins = m.table(0, 0)
        slots = at[bins != 7]
        assert slots.tolist() == [4 * K.EDGE_LANE + 2, 4 * K.EDGE_LANE + 3, 4 * K.EDGE_LANE + 4, 4 * K.EDGE_LANE + 5]
        assert bins[bins != 7].tolist() == [3, 3, 5, 5]
        for name, in_lane in (("table", False), ("table_in_lane", True)):
            m = catalogue["edges/%s/tile/m%d" % (name, mode)]["model"]
            at, bins = m.table(0, 0)
            assert len(at) > 64 and bins[63] == 3 and bins[64] == 5 and (bins[:64] == 3).all()
            assert (at[63] // 4 == at[64] // 4) == in_lane
        m = catalogue["edges/m%d" % mode]["model"]
        assert [m.rare(g, t) for g in (0, 1) for t in range(K.TILES)] == [4, 70, 66, 0, 70, 4, 0, 66]


def test_dominant_is_not_the_first_units_bin(catalogue):
    for name, c in _of(catalogue, "d_not_first/").items():
        m = c["model"]
        for g in range(1 if "/tile/" in name else 2):
            assert m.slots[g, 0, 0] == 3 and m.dominant(g) == 1
            assert 30 <= m.rare(g, 0) <= 64
            assert np.bincount(m.slots[g, 0], minlength=8).argmax() == 1


def test_dominant_changes_inside_a_granule(catalogue):
    for c in _of(catalogue, "d_changes/").values():
        m = c["model"]
        most = [[int(np.bincount(m.slots[g, t], minlength=8).argmax()) for t in range(K.TILES)] for g in (0, 1)]
        assert most == [[0, 4, 0, 5], [2, 2, 3, 1]]
        assert m.dominant(0) == 0 and m.dominant(1) == 2
        assert [m.rare(0, t) for t in range(K.TILES)] == [30, 250, 30, 250]      # tiles all but without the granule's bin: four rounds
        assert m.rare(1, 1) == 30 and m.rare(1, 2) > 192 and m.rare(1, 3) > 192


def test_odd_records_without_flag(catalogue):
    for mode in K.MODES:
        c = catalogue["no_flag/some/m%d" % mode]
        assert (c["bins"][list(K.NO_FLAG_SOME)] == 7).all() and c["model"].skew.all()
        assert c["model"].dominant(0) == 0                             # record 1 closes nothing: the second candidate
        assert c["model"].slots[0, 0, 0] == 7
        m = catalogue["no_flag/most/m%d" % mode]["model"]
        assert m.skew.all() and m.dominant(0) == 7 and m.dominant(1) == 7
        assert m.rare(0, 0) == K.TILE_UNITS - 201 and m.rare(0, 1) == K.TILE_UNITS


def test_fallback_granules(catalogue):
    for mode in K.MODES:
        assert catalogue["fallback/second/m%d" % mode]["model"].skew.tolist() == [True, False, False]
        assert catalogue["fallback/first/m%d" % mode]["model"].skew.tolist() == [False, True, True]


def test_random_cases_hold_many_bins(catalogue):
    for name, c in _of(catalogue, "random/").items():
        m = c["model"]
        for g in (0, 1):
            for t in range(K.TILES):
                assert len(set(m.table(g, t)[1].tolist())) >= 4, name
        if "skew" in name:
            assert all(10 <= m.rare(g, t) <= 64 for g in (0, 1) for t in range(K.TILES)), name
        else:
            assert all(m.rare(g, t) > 128 for g in (0, 1) for t in range(K.TILES)), name
