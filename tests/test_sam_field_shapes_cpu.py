"""tests/sam_field_shapes.py held to its word, without a GPU: every claim of every case is recomputed here from the window text
alone (a claim is a condition: a case whose text does not meet it is a bug in the catalogue), the oracle alone gives the outcome
each case expects -- records, mismatch, and exactly the flagged values the case lists -- and the host stripper passes the direct
check of tests/strip_check.py on every case, which also proves that checker against an implementation the CPU suite pins."""
import itertools
import re

import numpy as np
import pytest

from tests import sam_field_shapes as F
from tests.strip_check import direct_check, flag_reason, oracle_walk
from tests.helpers import ORACLE

_TERM = re.compile(rb"\r\n|\n|\r")
_WS = frozenset(F.SEPARATORS)
ALL32, ALL8 = set(range(32)), set(range(8))
_OP = re.compile(rb"([0-9]+)([MIDNSHPX=])")


def lines_of(window):
    """-> [(offset, line without terminator, terminated)] as universal newlines cut the window."""
    out, at = [], 0
    for m in _TERM.finditer(window):
        out.append((at, window[at:m.start()], True))
        at = m.end()
    if at < len(window):
        out.append((at, window[at:], False))
    return out


def spans_of(line):
    """-> [(begin, end)] of line.split()'s fields."""
    out, b = [], None
    for i, c in enumerate(line):
        if c in _WS:
            if b is not None:
                out.append((b, i))
                b = None
        elif b is None:
            b = i
    if b is not None:
        out.append((b, len(line)))
    return out


def test_the_field_splitter_of_this_module_is_str_split():
    for c in F.all_cases()[::7]:
        for w in c.windows:
            for _at, line, _t in lines_of(w)[::5]:
                assert [line[b:e] for b, e in spans_of(line)] == [x.encode() for x in line.decode("ascii").split()]


@pytest.fixture(scope="module")
def parser():
    from xenomapper_amd import _host
    p = _host.Parser(2)
    yield p
    p.close()


def test_names_are_unique_and_every_group_has_cases():
    cases = F.all_cases()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    assert {c.group for c in cases} == set(F.GROUPS)
    for c in cases:
        assert c.score_mode in (0, 1, 2) and c.claims and c.expect["n"] is not None
        assert all(len(w) < (1 << 20) for w in c.windows), c.name
        if c.after is not None:                               # a stale pair: the long window directly in front, on the same settings
            prev = cases[cases.index(c) - 1]
            assert prev.name == c.after and (prev.score_mode, prev.paired, prev.skip) == (c.score_mode, c.paired, c.skip)
    small = [c for c in cases if max(len(w) for w in c.windows) < (64 << 10)]
    assert len(small) > len(cases) // 2


# ---- the claims, each from the text alone ------------------------------------------------------------------------------------------
def _tag_events(at, line, tags):
    """Offsets in the window of the events of one line's tag fields: per matching optional field (tag, first letter, behind the last
    ':' ... ) as the grid group names them."""
    out = []
    sp = spans_of(line)
    for b, e in sp[11:]:
        field = line[b:e]
        for t in tags:
            if t in field:
                colon = b + field.rindex(b":")
                out.append({"tag": t, "tag_at": at + b + field.index(t), "colon": at + colon, "val_first": at + colon + 1, "val_last": at + e - 1,
                            "val_len": e - colon - 1, "field_end": at + e, "later": (b, e) != sp[11]})
    return out


def check_grid_events(c, claim):
    t0, t1 = F.TAGS[c.score_mode]
    starts = []
    for w in c.windows:
        seen = {k: set() for k in claim}
        by_len = {n: [set(), set()] for n in c.claims["value_lengths"]}
        placed = {(t, later): set() for t in (t0, t1) for later in (False, True)}     # a tag in field 11 / in a later field
        three = {t0: set(), t1: set()}                                                # ... its last ':' and the value's end in two more words
        for at, line, _t in lines_of(w):
            if not line.startswith(b"g"):
                continue
            starts.append(at % 32)
            sp = spans_of(line)
            seen["opt11"].add((at + sp[11][0]) % 32)
            seen["line_end"].add((at + len(line)) % 32)
            for ev in _tag_events(at, line, (t0, t1)):
                seen["tag0" if ev["tag"] == t0 else "tag1"].add(ev["tag_at"] % 32)
                for k in ("colon", "val_first", "val_last"):
                    seen[k].add(ev[k] % 32)
                by_len[ev["val_len"]][0].add(ev["val_first"] % 32)
                by_len[ev["val_len"]][1].add(ev["val_last"] % 32)
                placed[(ev["tag"], ev["later"])].add(ev["tag_at"] % 32)
                if ev["tag_at"] // 8 < ev["colon"] // 8 < ev["val_last"] // 8:
                    three[ev["tag"]].add(ev["tag_at"] % 32)
        for k in claim:
            assert seen[k] == ALL32, (c.name, k)
        assert all(v == ALL32 for v in placed.values()), (c.name, {k: len(v) for k, v in placed.items()})
        # a tag whose two letters lie in two words: on every word edge of the step, the step's own edge included
        for k in ("tag0", "tag1"):
            assert {o for o in seen[k] if o % 8 == 7} == {7, 15, 23, 31}
        for n, (first, last) in by_len.items():
            assert first == ALL32 and last == ALL32, (c.name, n)
        assert all(v == ALL32 for v in three.values()) == c.claims["three_words"]
    half = len(starts) // 2
    assert any(a != b for a, b in zip(starts[:half], starts[half:])) == c.claims["files_differ_mod32"]


def unterminated_events(c):
    """The events of an unterminated grid window's last line, per file: {event: offset modulo 32}; the line's end is the window's."""
    t0, t1 = F.TAGS[c.score_mode]
    out = []
    for w in c.windows:
        at, line, terminated = lines_of(w)[-1]
        assert not terminated and line.startswith(b"g") and at + len(line) == len(w)
        evs = _tag_events(at, line, (t0, t1))
        last = max(evs, key=lambda e: e["field_end"])
        one = {"line_start": at, "opt11": at + spans_of(line)[11][0], "window_end": len(w)}
        for ev in evs:
            one["tag0" if ev["tag"] == t0 else "tag1"] = ev["tag_at"]
        one.update({k: last[k] for k in ("colon", "val_first", "val_last")})
        assert (last["field_end"] == len(w)) == c.claims["value_ends_window"]
        out.append({k: v % 32 for k, v in one.items()})
    return out


def check_unterminated(c, claim):
    _template, at = claim
    ev = unterminated_events(c)
    assert ev[0]["line_start"] == at and ev[1]["line_start"] == (at + 13) % 32


def check_not_a_tag(c, _claim):
    qual_end, tab, line_end, shaped = set(), set(), set(), set()
    t0, t1 = F.TAGS[c.score_mode]
    w = c.windows[0]
    ls = lines_of(w)
    for i, (at, line, _t) in enumerate(ls):
        sp = spans_of(line)
        if line.startswith(b"q"):
            b, e = sp[10]
            assert line[e - 1:e] in (t0[:1], t1[:1]) and line[sp[11][0]:sp[11][0] + 1] in (t0[1:], t1[1:]) and e - b >= 16
            qual_end.add((at + e - 1) % 8)
        elif line.startswith(b"s"):
            for (b1, e1), (b2, e2) in zip(sp[11:], sp[12:]):
                if line[e1 - 1:e1] + line[b2:b2 + 1] in (t0, t1):
                    tab.add((at + e1) % 8)
        elif line.startswith(b"l"):
            nxt = ls[i + 1][1]
            assert line[-1:] + nxt[:1] in (t0, t1)
            line_end.add((at + len(line)) % 8)
        elif line.startswith(b"f") or (sp and line[sp[0][0]:sp[0][1]] in (t0 + b":i:5", t1 + b":i:6")):
            idx = [k for k, (b, e) in enumerate(sp) if line[b:e] in (t0 + b":i:5", t1 + b":i:6")]
            if len(idx) == 1 and all(line[b:e].startswith(b"f") for k, (b, e) in enumerate(sp) if k != idx[0]):
                shaped.add((len(sp), idx[0]))
    assert qual_end == set(c.claims["qual_end_mod8"]) == ALL8
    assert tab == set(c.claims["split_tab_mod8"]) == ALL8
    assert line_end == set(c.claims["split_line_end_mod8"]) == ALL8
    assert shaped == {tuple(x) for x in c.claims["tag_shaped_index"]}


def check_nth_set(c, claim):
    """Which of the field starts inside its 8-byte word the CIGAR field (index 5) is."""
    for w in c.windows:
        seen, whole, ops_in_front = set(), [], set()
        for at, line, _t in lines_of(w):
            if not line.startswith(b"a\t"):
                continue
            sp = spans_of(line)
            assert all(e - b <= 2 for b, e in sp[:5])
            cb, ce = at + sp[5][0], at + sp[5][1]
            front = [line[b:e] for b, e in sp[:5] if (at + b) // 8 == cb // 8]
            seen.add(len(front))
            if any(_OP.fullmatch(x) for x in front):           # ... and one of them reads as an operation
                ops_in_front.add(len(front))
            if ce - cb > 8:
                whole.append(ce // 8 - (cb + 7) // 8)
        assert seen == set(claim)
        assert min(whole) >= c.claims["cigar_whole_words"]
        assert ops_in_front == set(c.claims["operations_in_front_nth"])


def check_byte_mod8(c, claim):
    marker = b"d\t1\t9\t4M2S"
    for w in c.windows[:1]:
        seen, runs, lead, trail = set(), {}, set(), set()
        for at, line, _t in lines_of(w):
            if line.startswith(b"r\t"):
                i = line.index(marker)
                j = i
                while line[j - 1] in _WS:
                    j -= 1
                if i - j <= 1:
                    seen.add((line[i - 1], (at + i - 1) % 8))
                if i - j >= 2:
                    runs.setdefault(i - j, set()).add((at + j) % 8)
            elif spans_of(line) and spans_of(line)[0][1] - spans_of(line)[0][0] == 1 and b"e" in line[:12]:
                sp = spans_of(line)
                if sp[0][0] > 0:
                    lead.add(at % 8)
                if sp[-1][1] < len(line):
                    trail.add((at + sp[-1][1]) % 8)
        assert seen == {tuple(x) for x in claim}
        assert sorted(runs) == c.claims["separator_runs"] and all(v == ALL8 for v in runs.values())
        assert lead == ALL8 and trail == ALL8


def check_blank_line(c, claim):
    n, off, where = claim
    for f, w in enumerate(c.windows):
        ls = lines_of(w)
        blank = [(at, line) for at, line, _t in ls if not spans_of(line)]
        if (where == "first" and f == 1) or (where == "second" and f == 0):
            assert not blank
            continue
        assert len(blank) == 1 and len(blank[0][1]) == n and blank[0][0] % 8 == (off if f == 0 else (off + 3) % 8)
        assert ls.index((blank[0][0], blank[0][1], True)) == c.expect["n"]


def check_values(c, claim):
    t0, t1 = F.TAGS[c.score_mode]
    w = c.windows[0]
    have, starts, dup = {t0: set(), t1: set()}, set(), set()
    for at, line, _t in lines_of(w):
        if not line.startswith(b"v"):
            continue
        starts.add(at % 8)
        sp = spans_of(line)
        for t in (t0, t1):
            hits = [(b, e) for b, e in sp[11:] if t in line[b:e]]
            if len(hits) == 1 and line[hits[0][0]:hits[0][1]].startswith(t + b":i:"):
                have[t].add(line[hits[0][0] + 5:hits[0][1]].decode())
            if len(hits) == 2:
                e1, e2 = at + hits[0][1], at + hits[1][1]
                dup.add("one_word" if e1 // 8 == e2 // 8 else "two_words" if e1 // 32 == e2 // 32 else "two_steps")
    assert all(set(claim) <= have[t] for t in (t0, t1))
    assert starts == set(c.claims["line_start_mod8"]) == ALL8
    assert dup == {"one_word", "two_words", "two_steps"}


def check_op_counts(c, claim):
    for w in c.windows:
        counts, forms, nm = set(), set(), set()
        for _at, line, _t in lines_of(w):
            if not line.startswith(b"c"):
                continue
            f = line.split(b"\t")
            counts.add(len(_OP.findall(f[5])))
            forms.add(f[5].decode())
            nm.add(b",".join(x for x in f[11:] if b"NM" in x))
        assert set(claim) <= counts and {254, 255, 256} <= counts
        assert set(c.claims["forms"]) <= forms
        assert b"" in nm and b"NM:i:1.5" in nm and b"NM:i:2" in nm


def check_records_over(c, claim):
    w = c.windows[0]
    ls = lines_of(w)
    assert len(ls) > claim and len(ls) == c.expect["n"]
    n_ops = [len(_OP.findall(line.split(b"\t")[5])) for _at, line, _t in ls]
    assert all(n_ops[k] >= 255 for k in c.claims["long_records_at"])
    assert n_ops[-1] == c.claims["last_ops"] and c.claims["long_records_at"][-1] == len(ls) - 1
    assert n_ops[254] < 255 and {255, 256} <= set(c.claims["long_records_at"])          # both sides of the tile edge, and not in front
    other = [len(_OP.findall(line.split(b"\t")[5])) for _at, line, _t in lines_of(c.windows[1])]
    assert other[255] >= 255 and other[256] >= 255 and other[257] < 255


def check_name_lengths(c, claim):
    per = [lines_of(w) for w in c.windows]
    assert len(per[0]) == len(per[1])
    names = [[line[:spans_of(line)[0][1]] for _at, line, _t in p] for p in per]
    assert names[0] == names[1]
    cross, within = {}, [{}, {}]
    for k, nm in enumerate(names[0]):
        cross.setdefault(len(nm), set()).add((per[0][k][0] % 8, per[1][k][0] % 8))
        for f in (0, 1):
            if k:
                within[f].setdefault(len(names[f][k - 1]), set()).add((per[f][k - 1][0] % 8, per[f][k][0] % 8))
    for n in claim:
        assert len(cross[n]) == c.claims["align_pairs"] == 64, n
        assert len(within[0][n]) == 64 and len(within[1][n]) == 64, n
    diff, last, prefix, equal_other = set(), False, False, False
    for k in range(1, len(names[0])):
        a, b = names[0][k - 1], names[0][k]
        if len(a) == len(b):
            d = [i for i in range(len(a)) if a[i] != b[i]]
            if len(d) == 1:
                diff.add(d[0])
                last |= d[0] == len(a) - 1 and len(a) > 34
            if not d:
                la, lb = per[0][k - 1][1], per[0][k][1]
                equal_other |= la[len(a) + 1] != lb[len(b) + 1]
        elif a.startswith(b) or b.startswith(a):
            prefix = True
    assert set(c.claims["diff_at"]) <= diff and last and prefix and equal_other
    # the bytes right behind a name differ between the files as well (the names are equal there)
    assert all(per[0][k][1][len(nm) + 1] != per[1][k][1][len(nm) + 1] for k, nm in enumerate(names[0]))


def check_mismatch(c, claim):
    n, p, a1, a2 = claim
    k = c.expect["n"]
    (at1, l1, _), (at2, l2, _) = lines_of(c.windows[0])[k], lines_of(c.windows[1])[k]
    n1, n2 = l1.split(b"\t")[0], l2.split(b"\t")[0]
    assert len(n1) == len(n2) == n and [i for i in range(n) if n1[i] != n2[i]] == [p]
    assert (at1 % 8, at2 % 8) == (a1, a2)
    assert all(x[1].split(b"\t")[0] == y[1].split(b"\t")[0] for x, y in zip(lines_of(c.windows[0])[:k], lines_of(c.windows[1])[:k]))


def check_prefix_mismatch(c, _claim):
    k = c.expect["n"]
    n1, n2 = (lines_of(w)[k][1].split(b"\t")[0] for w in c.windows)
    assert n1 != n2 and (n1.startswith(n2) or n2.startswith(n1))


def check_run_lengths(c, claim):
    starts = None
    for f, w in enumerate(c.windows):
        names = [line.split(b"\t")[0] for _at, line, _t in lines_of(w)]
        runs, at, st = [], 0, []
        for _nm, g in itertools.groupby(names):
            n = len(list(g))
            st.append(at)
            runs.append(n)
            at += n
        assert set(claim) <= set(runs) and len(runs) == c.claims["runs"] == c.expect["n"]
        if f == 0:
            starts, first = st, runs
        else:
            assert runs != first                                   # different lengths in the two files
    assert set(c.claims["run_starts"]) <= set(starts)
    assert {63, 0, 1} <= {s % 64 for s in starts} and {255, 0, 1} <= {s % 256 for s in starts}


def check_continues(c, claim):
    """The short window of a stale pair: its text is the beginning of the long one's, its last line has no terminator, and the long
    window goes on with `claim` right behind it."""
    long_ = F.all_cases()[[x.name for x in F.all_cases()].index(c.after)]
    for short, lng in zip(c.windows, long_.windows):
        assert lng.startswith(short + claim.encode()) and len(lng) > len(short) + len(claim)
        assert not lines_of(short)[-1][2]
        assert lng[len(short) + len(claim):len(short) + len(claim) + 1] == b"\n"
    assert "longer_than_next" in long_.claims


CHECKS = {"grid_events": check_grid_events, "unterminated": check_unterminated, "qual_end_mod8": check_not_a_tag,
          "nth_set": check_nth_set, "byte_mod8": check_byte_mod8, "blank_line": check_blank_line, "values": check_values,
          "op_counts": check_op_counts, "records_over": check_records_over, "name_lengths": check_name_lengths,
          "mismatch": check_mismatch, "prefix_mismatch": check_prefix_mismatch, "run_lengths": check_run_lengths,
          "continues": check_continues, "longer_than_next": lambda c, claim: None}
# claims that the check of another claim of the same case covers
COVERED = {"value_ends_window", "operations_in_front_nth", "value_lengths", "three_words", "files_differ_mod32", "split_tab_mod8", "split_line_end_mod8", "tag_shaped_index",
           "cigar_whole_words", "separator_runs", "leading", "trailing", "line_start_mod8", "dup_one_word", "dup_two_words",
           "dup_two_steps", "forms", "nm_missing", "nm_not_int", "long_records_at", "last_ops", "align_pairs", "diff_at", "diff_last",
           "prefix", "equal_then_other_byte", "run_starts", "runs"}


@pytest.mark.parametrize("group", F.GROUPS)
def test_the_catalogue_reaches_what_it_claims(group):
    cases = F.cases_of(group)
    assert cases
    for c in cases:
        checked = 0
        for key, claim in c.claims.items():
            if key in CHECKS:
                CHECKS[key](c, claim)
                checked += 1
            else:
                assert key in COVERED, key
        assert checked, c.name
    if group == "grid":           # the unterminated lines, one to a window: in every mode and file every event on every offset, for
        seen = {}                 # each template by itself -- the window's end directly behind a value among them
        for c in cases:
            if "unterminated" in c.claims:
                for f, ev in enumerate(unterminated_events(c)):
                    for k, o in ev.items():
                        seen.setdefault((c.score_mode, c.claims["unterminated"][0], f, c.claims["value_ends_window"]), {}).setdefault(k, set()).add(o)
        assert len(seen) == 3 * len(F.UNTERMINATED_TEMPLATES) * 2
        assert sum(1 for key in seen if key[3]) == 3 * 3 * 2
        for key, events in seen.items():
            want = {"line_start", "opt11", "window_end", "colon", "val_first", "val_last"} | ({"tag0", "tag1"} if key[1] in (40, 13) else set())
            assert want <= set(events) and all(v == ALL32 for v in events.values()), (key, {k: len(v) for k, v in events.items()})
    if group == "separators":
        got = {tuple(c.claims["blank_line"]) for c in cases if "blank_line" in c.claims}
        assert {(n, o) for n, o, _w in got} == {(n, o) for n in (0, 1, 3, 9) for o in range(8)}
        assert {w for _n, _o, w in got} == {"both", "first", "second"}
    if group == "names":
        got = {tuple(c.claims["mismatch"][:2]) for c in cases if "mismatch" in c.claims}
        assert {(70, p) for p in F.DIFF_AT} | {(70, 69), (32, 31), (33, 32), (64, 63), (65, 64)} <= got
    if group == "stale":
        assert {c.claims["continues"].split("\t")[0][:4] for c in cases if c.after} >= {"long", "", "S:i:", "5", "7D3S"}


# ---- the oracle alone, and the host stripper through the direct check -------------------------------------------------------------
@pytest.mark.parametrize("group", F.GROUPS)
def test_the_oracle_alone_gives_what_every_case_expects(group):
    for c in F.cases_of(group):
        t1, t2 = (w.decode("ascii") for w in c.windows)
        pairs, err = oracle_walk(t1, t2, c.skip)
        assert len(pairs) == c.expect["n"], c.name
        assert (err == "mismatch") == c.expect["mismatch"], c.name
        scorer = [ORACLE.tag_score, ORACLE.tag_score_zs, ORACLE.cigar_score][c.score_mode]
        flags = []
        for k, pr in enumerate(pairs):
            for f, fields in enumerate(pr):
                for col, tag in ((2 * f, "AS"), (2 * f + 1, "XS")):
                    why = flag_reason(fields, tag, c.score_mode)
                    if why is not None:
                        flags.append((k, col))
                    try:                                      # the scorer returns or raises; it raises only where a flag is justified
                        scorer(fields, tag=tag)
                    except (ValueError, IndexError):
                        assert why is not None, (c.name, fields, tag)
        assert flags == [tuple(x) for x in c.expect["flags"]], c.name


def test_exactly_the_listed_value_strings_are_flag_justified():
    from tests.strip_check import plain_int32
    assert len(F.VALUES) == 21
    for v, flagged in F.VALUES:
        assert plain_int32(v) == (not flagged), v
        for mode in (0, 1, 2):
            for col, t in enumerate(F.TAGS[mode]):
                fields = ["r"] * 11 + ["%s:i:%s" % (t.decode(), v)]
                assert (flag_reason(fields, ("AS", "XS")[col], mode) is not None) == flagged, (v, mode, col)


@pytest.mark.parametrize("group", F.GROUPS)
def test_the_host_stripper_passes_the_direct_check_on_every_case(parser, group):
    for c in F.cases_of(group):
        r1, r2 = (np.frombuffer(w, dtype=np.uint8) for w in c.windows)
        block = parser.parse(r1, 0, len(r1), True, r2, 0, len(r2), True, c.score_mode, c.paired, c.skip, False, 1 << 20)
        pairs, err = direct_check(block, c.windows[0], c.windows[1], c.score_mode, c.paired, c.skip)
        assert len(pairs) == c.expect["n"] and (err == "mismatch") == c.expect["mismatch"], c.name
        assert sorted({(k, col) for k, col, _kind in block.exc}) == [tuple(x) for x in c.expect["flags"]], c.name
