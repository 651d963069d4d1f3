"""Differential test of the oracle against the reference itself, on the reference's recorded answers: the draws of
the property test that once ran it live (tests/test_host_fuzz.sam_pair and friends, derandomized) and the companion
tool's helper rows, recorded by tools/make_golden.py (G11).  The oracle must raise the same exception type, have
written the same six texts by then and return the same counts."""
import io

from tests import helpers as H
from tests.helpers import ORACLE

SCORERS = {"get_tag": ORACLE.tag_score, "get_tag_with_ZS_as_XS": ORACLE.tag_score_zs,
           "get_cigarbased_AS_tag": ORACLE.cigar_score}
G11 = H.golden("g11_differential.json.gz")


def test_oracle_behaves_like_the_reference():
    cases = G11["cases"]
    assert len(cases) == 300
    for k, case in enumerate(cases):
        t1, t2 = case["text"]
        mode, m, skip = case["mode"], H.unnum(case["min_score"]), case["skip_repeated"]
        outs = [io.StringIO() for _ in range(6)]
        err, counts = None, None
        try:
            pairs = ORACLE.read_pairs(io.StringIO(t1, newline=None), io.StringIO(t2, newline=None), skip)
            if mode == "se":
                res = ORACLE.run_single_end(pairs, outs, m, SCORERS[case["tag_func"]])
            else:
                res = ORACLE.run_paired_end(pairs, outs, m, SCORERS[case["tag_func"]], conservative=mode == "pe_conservative")
            counts = {("|".join(k) if isinstance(k, tuple) else k): v for k, v in res.named_counts(mode != "se").items()}
        except Exception as exc:
            err = type(exc).__name__
        assert err == case["error"], (k, t1, t2)
        assert [o.getvalue() for o in outs] == [case["outputs"][name] for name in H.STATES], (k, t1, t2)
        if err is None:
            assert counts == case["counts"], k


def test_mappability_host_functions_behave_like_the_reference():
    """The text and small-list functions of the companion tool (wiggle and FASTA readers, smoothing, normalisation) side by
    side with the reference's on odd inputs: tracks without values, files without declarations, repeated chromosomes, names
    with '=' in them, nameless FASTA records, text in front of the first header."""
    from xenomapper_amd import mappability as ours
    rows = G11["mappability"]
    for row in rows["wiggle"]:
        b = ours.Mappability(chromosome_sizes={})
        b.from_wiggle(io.StringIO(row["text"]))
        assert dict(b) == {k: v for k, v in row["tracks"]}, row["text"]
        assert b.chromosome_sizes == {k: v for k, v in row["chromosome_sizes"]}, row["text"]
    for row in rows["fasta"]:
        assert [list(r) for r in ours.parse_fasta(io.StringIO(row["text"]))] == row["records"], row["text"]
    for row in rows["lists"]:
        values = row["values"]
        for width in (10, 2, 1):
            assert ours.smoothed_list(values, width) == row["smoothed"][str(width)]
        assert ours.normalised_list(values) == row["normalised"]
