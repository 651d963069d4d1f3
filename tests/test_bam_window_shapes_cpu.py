"""The windows of tests/bam_window_shapes.py on the CPU: for every window the GPU test runs, the builder's own expectation (a) equals
the host's reading of the same bytes (b: _host.bam_walk, the host printer, _host.Parser.parse), and every boundary the GPU test is
about is really in the inputs -- segments per scan thread, records per carried piece, pieces per walk workgroup, empty members, cut
records, runs of equal names, pairs per unit-mask word.  No GPU: this proves the inputs and the model before a card sees them."""
import struct

import numpy as np
import pytest

from tests import bam_shapes as S
from tests import bam_window_shapes as W

GROUPS = {"A": W.a_cases, "B": W.b_cases, "C": W.c_cases, "D": W.d_cases, "E": lambda: W.e_cases() + [W.case_flush_name()]}


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_the_builder_and_the_host_expect_the_same_of_every_window(group):
    for case in GROUPS[group]():
        windows = W.windows_of(case)
        assert windows
        for w, (parts, exp) in enumerate(windows):
            assert W.same_expectation(exp, W.host_expect(parts, case.flags)) is None, (case.name, w)
            for p in parts:
                assert p.hi - p.lo <= (1 << 20) + (1 << 19), (case.name, w)               # about a megabyte a window
                assert all(len(raw) <= 65536 and len(m) <= 65536 for m, raw in W.members_of(p)) or case.name.startswith("D")


def _sizes(part):
    """Records per member of a part (members that begin and end at records)."""
    off = part.file.off
    at = np.searchsorted(off, np.asarray(part.bounds))
    assert all(int(off[a]) == b for a, b in zip(at, part.bounds))
    return np.diff(at)


def test_group_a_segments_carried_pieces_empty_members_and_skip():
    per = set()
    for n_seg in W.A_SEGMENTS:
        case = W.case_segments(n_seg)
        (parts, exp), = W.windows_of(case)
        assert not exp["unaligned"] and exp["ended"] and exp["n"] == 2 * n_seg
        for p in parts:
            assert W.n_block_segments(p) == n_seg and len(W.segment_starts(p)) == n_seg
            counts = _sizes(p)
            assert counts.min() >= 1 and counts.max() <= 3 and (n_seg < 3 or len(set(counts.tolist())) == 3)
            sizes = [len(r.data) for r in p.file.recs]
            assert min(sizes) >= 38 and max(sizes) <= 120 and len(set(sizes)) > min(20, n_seg)
            assert {W.LEVELS[(j + p.shift) % 5] for j in range(len(p.bounds) - 1)} == set(W.LEVELS[:max(1, min(5, n_seg))]) or n_seg < 5
        assert parts[0].bounds != parts[1].bounds
        per.add(-(-n_seg // W.SCAN_T))
    assert per == {1, 2, 3}
    switch = set()
    for n_seg, pieces in W.A_CARRIED:
        case = W.case_segments_behind_carry(n_seg, pieces)
        (p1, e1), (p2, e2) = W.windows_of(case)
        assert e1["starved"] and not e1["ended"] and e2["ended"]
        assert W.pieces_of(p2[0], e1["rec_off"][0], e1["consumed"][0]) == pieces and p2[1].mid == p2[1].lo
        assert W.n_block_segments(p2[0]) == W.n_block_segments(p2[1]) == n_seg
        switch.add((-(-(n_seg + pieces) // W.SCAN_T), pieces))
    # with two segments per scan thread the first block segment (number `pieces`) lies inside thread 0's range, at its end, in thread 1's
    assert {(2, 1), (2, 2), (2, 3), (1, 1)} <= switch
    (parts, exp), = W.windows_of(W.case_empty_members())
    empty = [j for j in range(len(parts[0].bounds) - 1) if parts[0].bounds[j] == parts[0].bounds[j + 1]]
    assert tuple(empty) == W.A_EMPTY_AT and len(parts[0].bounds) - 1 == 2049 and {0, 2048, 1022, 1023, 1024} <= set(empty)
    assert any(b - a == 1 for a, b in zip(empty, empty[1:])) and W.n_block_segments(parts[0]) == 2049 - len(empty)
    assert exp["ended"] and exp["n"] == len(parts[0].file.recs)
    skips = []
    for which in ("one", "most"):
        (parts, exp), = W.windows_of(W.case_skip(which))
        assert exp["ended"] and exp["n"] == 40 and parts[0].skip == parts[0].file.head > 0
        skips.append((parts[0].skip, parts[0].bounds[1] - parts[0].bounds[0]))
    assert skips[0][0] == 1 and skips[1][0] == skips[1][1] - 38


def test_group_b_members_that_begin_inside_a_record_and_windows_that_end_inside_one():
    (parts, exp), = W.windows_of(W.case_moved_cut(None))
    assert not exp["unaligned"] and W.n_block_segments(parts[0]) == 2049 and -(-2049 // W.SCAN_T) == 3
    kinds = set()
    for b in W.B_MOVED:
        (parts, exp), = W.windows_of(W.case_moved_cut(b))
        starts = W.segment_starts(parts[0])
        assert exp["unaligned"] and not exp["bad_block"] and len(starts) == 2049
        inside = [s for s, at in enumerate(starts) if at not in set(parts[0].file.off.tolist())]
        assert inside == [b + 1]
        kinds.add((b + 1) % 3 == 0)                   # the pair (b, b + 1) lies in one thread's three segments, or across two threads'
    assert kinds == {True, False}
    (parts, exp), = W.windows_of(W.case_record_across_members())
    assert exp["unaligned"] and max(len(r.data) for r in parts[0].file.recs) > 65536
    left = set()
    for where in W.B_TAIL_CUTS:
        for eof in (0, 1):
            (parts, exp), = W.windows_of(W.case_cut_tail(where, eof))
            assert not exp["unaligned"] and exp["bad_block"] == (2 if eof else 0) and exp["n_rec"] == (23, 24)
            left.add(exp["raw_len"][0] - exp["stop"][0])
            if not eof:
                assert exp["n"] == 23 and exp["starved"] and exp["consumed"][0] == exp["stop"][0] == int(parts[0].file.off[23])
    size = len(W.case_cut_tail("1", 0).files[0].recs[-1].data)
    assert left == {1, 2, 3, 4, size // 2, size - 1}


def test_group_c_tails_of_every_piece_count():
    seen_same, seen_other = 0, 0
    for i, r in enumerate(W.C_TAILS):
        case = W.case_tail(r, same_slot=i % 2 == 1)
        (p1, e1), (p2, e2) = W.windows_of(case)
        tail = e1["n_rec"][0] - int(np.searchsorted(e1["rec_off"][0], e1["consumed"][0]))
        assert tail == r and W.pieces_of(p2[0], e1["rec_off"][0], e1["consumed"][0]) == -(-r // W.CARRY_SEG)
        assert p2[0].mid - p2[0].lo < 500_000 and e1["starved"] and e2["ended"] and e2["n"] == e2["n_rec"][0] == e2["n_rec"][1]
        sizes = [len(x.data) for x in p2[0].file.recs]
        assert min(sizes) == 38 and max(sizes) <= 60
        if case.slot_of(1) == case.slot_of(0):
            assert e1["consumed"][0] >= p2[0].mid - p2[0].lo            # the tail lies behind the bytes it is copied to
            seen_same += 1
        else:
            seen_other += 1
    assert seen_same >= 5 and seen_other >= 5
    assert [-(-r // W.CARRY_SEG) for r in W.C_TAILS[-3:]] == [W.WALK_T, W.WALK_T, W.WALK_T + 1]
    (p1, e1), (p2, e2) = W.windows_of(W.case_tail(200, mixed=True))
    j0 = int(np.searchsorted(e1["rec_off"][0], e1["consumed"][0]))
    cuts = e1["rec_off"][0][j0::W.CARRY_SEG].astype(np.int64)
    assert len(cuts) == 2 and e1["n_rec"][0] - j0 == 200 and int(cuts[1] - cuts[0]) > W.BIG          # a piece with the large record
    (p1, e1), (p2, e2) = W.windows_of(W.case_tail(129, last="none"))
    assert all(p.mid == p.hi and p.mid > p.lo and p.eof and not p.bounds for p in p2) and e2["n_rec"] == (129, 1) and e2["ended"]
    (p1, e1), (p2, e2) = W.windows_of(W.case_tail(257, last="one"))
    assert p2[0].mid == p2[0].hi and not p2[0].bounds and p2[1].bounds and e2["n_rec"] == (257, 257) and e2["ended"]


def test_group_d_chains_add_up_to_the_whole_files():
    for case in W.d_cases():
        windows = W.windows_of(case)
        exps = [e for _p, e in windows]
        assert all(not e["unaligned"] and not e["bad_block"] and e["mismatch_at"] < 0 for e in exps)
        assert [e["ended"] for e in exps] == [False] * (len(exps) - 1) + [True]
        got, want = W.concat_chain(case, windows, exps), W.whole_chain_expect(case, windows)
        assert got["n"] == want["n"] > 700
        for key in ("cols", "flags", "pair_off"):
            assert all(np.array_equal(a, b) for a, b in zip(got[key], want[key])), (case.name, key)
        assert np.array_equal(got["bits"], want["bits"]), case.name
        carried = [(p[0].mid > p[0].lo, p[1].mid > p[1].lo) for p, _e in windows]
        if case.flags.max_records == 1 << 20:         # windows that run out of one file's records: it starves, the other carries
            assert sum(1 for e in exps if e["starved"]) >= 5
            # (the halo record and an open run are carried by both files)
            assert (True, False) in carried or (False, True) in carried or case.flags.keep_halo or case.flags.skip_repeated
        if case.flags.max_records < 1 << 20:
            assert sum(1 for e in exps if e["n"] == case.flags.max_records and not e["starved"] and not e["ended"]) >= 2
        sizes = {len(r.data) for f in case.files for r in f.recs}
        assert W.BIG in sizes and (set(S.SIZES) <= sizes or case.flags.skip_repeated)
        for f in case.files:
            counts = np.diff(np.searchsorted(f.off, np.asarray(W._d_files(case.flags.paired, case.flags.skip_repeated)[1][case.files.index(f)])))
            assert counts.min() >= 1 and counts.max() <= 6
        if case.flags.skip_repeated:
            crossed = 0
            for f, fl in enumerate(case.files):
                names = [r.name for r in fl.recs]
                lens = np.diff(np.flatnonzero([True] + [names[i] != names[i - 1] for i in range(1, len(names))] + [True]))
                assert set(W.D_RUNS) <= set(lens.tolist())
                for parts, e in windows:
                    p = parts[f]
                    i = int(np.searchsorted(fl.off, p.hi))
                    if not p.eof and 0 < i < len(names) and int(fl.off[i]) == p.hi and names[i] == names[i - 1]:
                        crossed += 1                  # a run goes on behind the window: it is not yielded, its first record is kept
                        start = i - 1
                        while start > 0 and names[start - 1] == names[i]:
                            start -= 1
                        assert p.lo + e["consumed"][f] <= int(fl.off[start])
            assert crossed >= 1
    assert W.whole_file_expect(W.case_chain((1, 1, 0), 64))[0]["n"] == 3000


def test_group_e_pairs_names_and_mismatches():
    assert [W.windows_of(W.case_pairs(n))[0][1]["n"] for n in W.E_PAIRS] == list(W.E_PAIRS)
    cases = W.e_cases()
    big = W.E_PAIRS[-1]
    at = {}
    for case in cases:
        (parts, exp), = W.windows_of(case)
        n = len(case.files[0].recs)
        names = [[r.name for r in f.recs] for f in case.files]
        differ = [k for k in range(n) if names[0][k] != names[1][k]]
        assert exp["mismatch_at"] == (differ[0] if differ else -1) and exp["n"] == (differ[0] if differ else n)
        assert not exp["ended"] or not differ
        at.setdefault(n, set()).add(exp["mismatch_at"])
        for k in differ:
            a, b = names[0][k], names[1][k]
            assert (a[1:] == b[1:] and a[0] != b[0]) or (a[:-1] == b[:-1] and a[-1] != b[-1]) or \
                (abs(len(a) - len(b)) == 1 and a[:min(len(a), len(b))] == b[:min(len(a), len(b))])
        flagged = np.flatnonzero([(r.fa or r.fx) or (q.fa or q.fx) for r, q in zip(*[f.recs for f in case.files])])
        assert exp["n_exceptions"] == int(np.count_nonzero(flagged < exp["n"]))
        if n == big and 63 <= exp["n"] < big - 100:
            assert (flagged < exp["n"]).any() and (flagged > exp["n"]).any()           # flagged values on both sides of the cut
    assert at[big] == {-1, 0, 1, 63, 64, 255, 256, big - 1}
    assert all({-1, 0, n - 1} <= at[n] for n in W.E_PAIRS)
    ids, recs = W._e_records(big)
    lens = {len(r.name) for r in recs[0]}
    assert set(S.NAME_LEN) <= lens and max(lens) == 254
    # runs of 1 .. 4 equal names, one across records 63 | 64 and one across 255 | 256; bits from both sides of a 64-pair word
    bits = W.windows_of(W.case_pairs(big))[0][1]["bits"]
    run = np.diff(np.flatnonzero(np.concatenate([bits == 0, [True]])))
    assert set(run.tolist()) == {1, 2, 3, 4} and bits[62:66].tolist() == [0, 1, 1, 1] and bits[254:258].tolist()[:3] == [0, 1, 1]
    # equal names are followed by bytes that differ between the files
    behind = 0
    for r, q in zip(*recs):
        a = r.data[36 + len(r.name):52 + len(r.name)]
        b = q.data[36 + len(q.name):52 + len(q.name)]
        assert r.name == q.name and a[0] == b[0] == 0
        behind += a[:4] != b[:4] and len(r.name) % 16 != 15
    assert behind > big // 4
    (parts, exp), = W.windows_of(W.case_flush_name())
    for p in parts:
        last = p.file.recs[-1]
        assert len(last.name) == 254 and p.file.stream.endswith(last.name + b"\0") and p.hi == p.file.size
    assert parts[0].file.size == parts[1].file.size and exp["n"] == 10 and exp["bits"][-1] == 1


def test_the_members_the_slots_cannot_hold_and_the_records_that_are_none():
    for where, eof in (("last", 0), ("last", 1), ("middle", 0)):
        parts = W.zero_member_parts(where, eof)
        zero = [raw for _m, raw in W.members_of(parts[0]) if raw == bytes(4096)]
        assert len(zero) == 1 and 4096 // 4 > 4096 // 36 + 2                 # more record starts than slot_of() leaves the block
        assert (W.members_of(parts[0])[-1][1] == bytes(4096)) == (where == "last")
        assert sum(len(raw) for _m, raw in W.members_of(parts[0])) == parts[0].hi
    for size in (0, 1, 31):
        parts = W.short_record_parts(size)
        raw = W.members_of(parts[0])[-1][1]
        assert len(raw) == 2 * (4 + size) and struct.unpack_from("<I", raw)[0] == size and 2 <= len(raw) // 36 + 2
        assert len(parts[1].file.recs) == len(parts[0].file.recs) + 2        # the pair kernel looks at both of them
