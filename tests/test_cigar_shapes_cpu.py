"""The catalogue of tests/cigar_shapes.py reaches what it claims (needs no GPU): the wave models find every class, stretch
length and end-of-array distance on both species and on the claimed side of each comparison; the reference scorer agrees
with the C oracle on every case and with the reference program's recorded scores on every record kind; xm_cigar_pack (host
code) agrees with the plain restatement of the packed layout."""
import numpy as np
import pytest

from tests import cigar_shapes as S
from tests import helpers as H

FAST = ("brief", "one_chunk", "two_chunks")


def packed_of(sp):
    return sp["packed"] if sp["packed"] is not None else H.np_cigar_pack(sp["cig_off"], sp["cig_oplen"])


@pytest.fixture(scope="module")
def models():
    """{case name: (K1p rows of species 1 and 2, K1c rows of species 1 and 2)}"""
    out = {}
    for case in S.all_cases():
        sp, _ = case.columns()
        p = [S.k1p_model(case.n, s["nm"], *packed_of(s)) for s in sp]
        c = [S.k1c_model(case.n, s["cig_off"], s["cig_oplen"]) for s in sp]
        out[case.name] = (p, c)
    return out


def test_cases_are_small_and_named_once():
    names = [c.name for c in S.all_cases()]
    assert len(set(names)) == len(names)
    assert set(c.group for c in S.all_cases()) == set(S.GROUPS)
    for case in S.all_cases():
        assert 1 <= case.n <= S.MAX_RECORDS, case.name
        assert (case.bad != 0) <= (case.group == "range"), case.name     # only `range` cases leave int32
    assert len(S.KINDS) < 400
    assert S.used_kinds() == set(S.KINDS), set(S.KINDS) - S.used_kinds()


def test_every_claim_holds(models):
    for case in S.all_cases():
        p, c = models[case.name]
        assert case.claims, case.name
        for kernel, species, t, props in case.claims:
            row = (p if kernel == "p" else c)[species][t]
            for key, want in props.items():
                assert row[key] == want, (case.name, kernel, species, t, key, row)


def test_model_finds_every_class_on_both_species(models):
    seen_p, seen_long, seen_c, orders = set(), set(), set(), set()
    chunks, last, ends, spec, longer = set(), set(), set(), set(), set()
    for name, (p, c) in models.items():
        for s in (0, 1):
            for row in p[s]:
                seen_p.add((row["cls"], s))
                if row["long"]:
                    seen_long.add((row["long"], s))
            for row in c[s]:
                seen_c.add((row["guard"], s))
                if row["guard"] in (None, "long_op"):
                    chunks.add((row["chunks"], s))
                    last.add((row["last_checked"], s))
                    ends.add((row["last_end"], s))
                if row["guard"] is not None:                            # the per-record path
                    spec.add((row["spec_checked"], s))
                    longer.add((row["longer"], s))
        for a, b in zip(p[0], p[1]):
            if a["full"]:
                orders.add((a["cls"] in FAST, b["cls"] in FAST))
    assert seen_p == {(cls, s) for cls in S.K1P_CLASSES for s in (0, 1)}
    assert seen_long == {(kind, s) for kind in ("own", "over") for s in (0, 1)}
    assert seen_c == {(g, s) for g in (None, "partial", "stretch", "many_ops", "long_op") for s in (0, 1)}
    assert orders == {(True, True), (True, False), (False, True), (False, False)}      # both orders share the table T
    assert chunks >= {(k, s) for k in (1, 2, 3, 4) for s in (0, 1)}
    assert last == {(v, s) for v in (True, False) for s in (0, 1)}
    assert ends >= {(v, s) for v in (-1, 0, 1) for s in (0, 1)}
    assert spec == longer == {(v, s) for v in (True, False) for s in (0, 1)}


def test_every_stretch_length_at_the_first_and_last_tile_of_a_workgroup(models):
    p_seen, c_seen, both = set(), set(), set()
    for name, (p, c) in models.items():
        if not name.startswith("stretch/"):
            continue
        for s in (0, 1):
            for t, row in enumerate(p[s]):
                if row["full"] and t % 8 in (0, 7) and row["cls"] == S.expected_k1p_class(row["W"]):
                    p_seen.add((row["W"], t % 8, s))
            for w, row in enumerate(c[s]):
                if row["full"] and w % 4 in (0, 3) and (row["guard"] == "stretch") == (row["W"] >= 1024):
                    c_seen.add((row["W"], w % 4, s))
        for a, b in zip(p[0], p[1]):
            if a["full"] and a["W"] == b["W"]:
                both.add(a["W"])
    assert p_seen >= {(W, at, s) for W in S.STRETCHES for at in (0, 7) for s in (0, 1)}
    assert c_seen >= {(W, at, s) for W in S.STRETCHES for at in (0, 3) for s in (0, 1)}
    assert both >= set(S.STRETCHES)
    heavy = [c for c in S.all_cases() if c.name.startswith("stretch/heavy254")]
    W = set()
    for case in heavy:
        p, _ = models[case.name]
        for t, row in enumerate(p[0]):
            if "k254" in case.kinds[0][t * 256:(t + 1) * 256]:
                W.add(row["W"])
    assert W >= {w for w in S.STRETCHES if w >= 255}


def test_every_end_of_array_distance_and_record_count(models):
    dists = set()
    for name, (p, c) in models.items():
        for s in (0, 1):
            full = [row for row in p[s] if row["full"]]
            if name.startswith("end/") and full and len(full) < len(p[s]):
                last = full[-1]
                dists.add((last["dist"], last["cls"] in FAST, p[s][-1]["W"], s))
    # 9 and 8 ops in front of the end: fast; 7 and 0: the bounds-checked path; the partial workgroup owns exactly those ops
    assert dists >= {(d, d >= 8, d, s) for d in S.END_DISTANCES for s in (0, 1)}
    assert any(row["full"] and row["dist"] == 0 for name, (p, c) in models.items() for row in p[0][-1:])
    counts = set()
    for case in S.all_cases():
        for s in (0, 1):
            counts.update(len(S.KINDS[k][0]) for k in set(case.kinds[s]))
    assert counts >= set(S.RECORD_OPS)
    sizes = set(c.n for c in S.all_cases() if c.group == "sizes")
    assert sizes == set(S.SIZES)
    # an escaped record at the last record of a tile, in front of a workgroup, and at record n - 1
    places = set()
    for case in S.all_cases():
        for s in (0, 1):
            k = np.array([len(S.KINDS[x][0]) for x in case.kinds[s]])
            for r in np.flatnonzero(k >= 255):
                places.update({("tile", s)} if r % 256 == 255 else set())
                places.update({("workgroup", s)} if r % 2048 == 2047 and r + 1 < case.n else set())
                places.update({("last", s)} if r == case.n - 1 else set())
    assert places == {(w, s) for w in ("tile", "workgroup", "last") for s in (0, 1)}


def test_penalty_and_range_kinds_are_what_their_names_say():
    for tag, want in (("m1", 2**30 - 1), ("", 2**30), ("p1", 2**30 + 1)):
        for many in ("", "_many"):
            kind = "pen_2p30%s%s" % (tag, many)
            assert -S.exact(kind) == want, kind
            assert {c for _, c in S.KINDS[kind][0]} == {S.I, S.D, S.S}
    assert 6 * 2**30 - S.exact("pen_2p32") == 7 * (5 + 3 * (2**28 - 1)) > 2**32 and S.score("pen_2p32") == (805306354, 0)
    assert S.score("max_exact") == (2**31 - 1, 0) and S.exact("max_plus1") == 2**31 and S.score("max_plus1") == (2**31 - 1, 1)
    assert S.score("min_plus1") == (-2**31 + 1, 0) and S.exact("min_exact") == -2**31 and S.score("min_exact") == (-2**31 + 1, 1)
    assert S.score("a3") == (S.ABSENT, 0)
    assert 1023 * (5 + 3 * (2**20 - 1)) == 3218081790 < 2**32
    assert all(l < 2**28 and 0 <= c < 16 for ops, _ in S.KINDS.values() for l, c in ops)


def test_reference_scorer_equals_the_c_oracle_on_every_case():
    for case in S.all_cases():
        sp, _ = case.columns()
        for s in sp:
            want, bad = H.c_cigar_scores(s["nm"], s["cig_off"], s["cig_oplen"])
            assert np.array_equal(s["score"], want), case.name
            assert s["bad"] == bad, case.name


def test_cigar_pack_equals_its_restatement_on_every_case():
    from xenomapper_amd import _ffi
    for case in S.all_cases():
        sp, _ = case.columns()
        for s in sp:
            got = _ffi.cigar_pack(s["cig_off"], s["cig_oplen"])
            want = H.np_cigar_pack(s["cig_off"], s["cig_oplen"])
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), case.name


def test_every_kind_scores_as_the_reference_program_recorded():
    golden = H.golden("g12_cigar_kinds.json")["kinds"]
    assert set(S.KINDS) - set(golden) == S.BINARY_ONLY                  # nothing else is excluded
    assert set(golden) <= set(S.KINDS)
    for kind, want in golden.items():
        got = S.exact(kind)
        assert (want == "-inf") if got is None else (want == got), kind
        assert H.ORACLE.cigar_score(S.sam_fields(kind)) == H.unnum(want), kind
