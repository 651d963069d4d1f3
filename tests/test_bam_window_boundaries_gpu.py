"""The BAM input front end (xm_bamdev.hip: xm_bamdev_run -- walk_kernel, scan_kernel, gather_kernel, parse_kernel, run_start_kernel,
run_select_kernel, pair_kernel -- and the record-walk epilogue of inflate_kernel, xm_inflate.hip) on the windows of
tests/bam_window_shapes.py, through the C ABI, window chains with carried tails included: every boundary of its loops.  Every
comparison is exact, against the host's reading of the same bytes (host_expect; tests/test_bam_window_shapes_cpu.py proves it equal
to the builder's own expectation on every window used here).  A window the model calls aligned and well formed must come back with
bad_block == 0, unaligned == 0 and weird == 0: a declined window never counts as a pass.

Figures: none -- everything is byte- and bit-exact."""
import numpy as np
import pytest

from tests import bam_window_shapes as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from xenomapper_amd import xenomapper as xm
    return xm.default_context()


def reserve_for(dev, case, windows, exact_raw=False):
    """Room for the largest window of the case on every slot it uses; -> the record capacity (what max_records may be at most)."""
    from xenomapper_amd import _ffi
    comp = raw = blocks = records = 1
    for parts, exp in windows:
        for f, p in enumerate(parts):
            comp = max(comp, sum(len(m) for m, _raw in W.members_of(p)))
            raw = max(raw, p.hi - p.lo)
            blocks = max(blocks, len(p.bounds))
            records = max(records, exp["n_rec"][f])
    pieces = records // W.CARRY_SEG + 4
    for slot in sorted({case.slot_of(w) for w in range(len(windows))}):
        dev.reserve(slot, comp + _ffi.BGZF_COMP_PAD, raw if exact_raw else raw + 64, blocks + pieces, records + 64)
    return records + 64


def run_window(dev, slot, parts, flags, cap, carry=None):
    """carry: (slot, (consumed1, consumed2)) of the window in front."""
    inputs = []
    for f, p in enumerate(parts):
        comp, x = W.device_input(p, carry[0] if carry else 0, carry[1][f] if carry else 0)
        if comp:
            dev.staging(slot, f)[:len(comp)] = np.frombuffer(comp, dtype=np.uint8)
        inputs.append(x)
    return dev.run(slot, inputs, 0, flags.paired, flags.keep_halo, min(flags.max_records, cap), skip_repeated=flags.skip_repeated)


def check_window(blk, exp, flags, what):
    """The device's block against the model's expectation of the window; -> what the window yielded (concat_chain's form)."""
    from xenomapper_amd import _ffi
    assert (blk.bad_block, blk.unaligned) == (exp["bad_block"], exp["unaligned"]), what
    if exp["bad_block"] or exp["unaligned"]:
        return None
    assert not blk.weird, what
    assert blk.raw_len == exp["raw_len"] and blk.n_rec == exp["n_rec"], what
    n = exp["n"]
    assert (blk.n, blk.mismatch_at, blk.ended, blk.starved) == (n, exp["mismatch_at"], exp["ended"], exp["starved"]), what
    assert blk.consumed == exp["consumed"], what
    assert blk.n_exceptions == exp["n_exceptions"], what
    pair_off = []
    for f in (0, 1):
        if flags.skip_repeated:                       # the table of the run starts
            pair_off.append(_ffi._host_view(blk.rec_off_addr[f], n, np.uint32).copy())
        else:                                         # the whole record table
            table = _ffi._host_view(blk.rec_off_addr[f], exp["n_rec"][f], np.uint32).copy()
            assert np.array_equal(table, exp["rec_off"][f]), (what, f, int(np.flatnonzero(table != exp["rec_off"][f])[0]))
            pair_off.append(table[:n])
        assert np.array_equal(pair_off[f], exp["pair_off"][f]), (what, f)
        assert np.array_equal(blk.line_flags[f], exp["flags"][f]), (what, f)
    cols = [c.copy() for c in blk.cols]
    for j in range(4):
        assert np.array_equal(cols[j], exp["cols"][j]), (what, j, int(np.flatnonzero(cols[j] != exp["cols"][j])[0]))
    words = blk.unit_bits
    assert words.shape[0] == (n + 63) // 64
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")
    assert np.array_equal(bits[:n], exp["bits"]), what
    if not flags.skip_repeated and exp["mismatch_at"] < 0:          # (the pair kernel also marks pairs behind a cut; nobody reads them)
        assert not bits[n:].any(), what
    return {"n": n, "cols": cols, "flags": [x.copy() for x in blk.line_flags], "bits": bits[:n].copy(), "pair_off": pair_off}


def run_case(ctx, case, dev=None, exact_raw=False):
    """All windows of a case on a front end of its own (or on `dev`), each against the host's reading; -> the device's yields."""
    from xenomapper_amd import _ffi
    windows = W.windows_of(case)
    own = dev is None
    dev = _ffi.BamDev(ctx) if own else dev
    try:
        cap = reserve_for(dev, case, windows, exact_raw)
        outcomes, carry = [], None
        for w, (parts, _exp) in enumerate(windows):
            exp = W.host_expect(parts, case.flags)
            slot = case.slot_of(w)
            blk = run_window(dev, slot, parts, case.flags, cap, carry)
            outcomes.append(check_window(blk, exp, case.flags, (case.name, w)))
            carry = (slot, blk.consumed)
        return windows, outcomes
    finally:
        if own:
            dev.close()


# ---- A: segments and the scan ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_seg", W.A_SEGMENTS)
def test_a_windows_of_so_many_segments(ctx, n_seg):
    """1 .. 3001 block segments, 1 .. 3 records each: scan_kernel with 1, 2 and 3 segments a thread, gather_kernel's waves, the record
    table, the columns, the line flags and the unit bits."""
    windows, outcomes = run_case(ctx, W.case_segments(n_seg))
    assert outcomes[0]["n"] == 2 * n_seg


@pytest.mark.parametrize("n_seg,pieces", W.A_CARRIED)
def test_a_block_segments_behind_carried_pieces(ctx, n_seg, pieces):
    """1, 2 and 3 carried pieces in front of 1023 / 1024 / 1025 block segments: where the pieces end and the blocks begin lies inside
    a scan thread's range and between two threads' ranges."""
    windows, outcomes = run_case(ctx, W.case_segments_behind_carry(n_seg, pieces))
    assert len(outcomes) == 2 and outcomes[1]["n"] == windows[1][1]["n_rec"][0]


def test_a_empty_members_take_no_segment(ctx):
    windows, outcomes = run_case(ctx, W.case_empty_members())
    assert outcomes[0]["n"] == 2 * (2049 - len(W.A_EMPTY_AT))


@pytest.mark.parametrize("which", ["one", "most"])
def test_a_the_header_shares_the_first_member(ctx, which):
    """skip = 1 and skip = isize - 38; skip >= isize, and skip together with a carried tail, are refused."""
    from xenomapper_amd import _ffi
    case = W.case_skip(which)
    dev = _ffi.BamDev(ctx)
    try:
        windows, outcomes = run_case(ctx, case, dev)
        assert outcomes[0]["n"] == 40
        parts = windows[0][0]
        cap = dev.capacity(0)[3]
        isize = parts[0].bounds[1] - parts[0].bounds[0]
        for skip, carried in ((isize, False), (isize + 1, False), (1, True)):
            bad = [parts[0]._replace(skip=skip), parts[1]]
            inputs = []
            for f, p in enumerate(bad):
                comp, x = W.device_input(p, 0, 0)
                dev.staging(0, f)[:len(comp)] = np.frombuffer(comp, dtype=np.uint8)
                inputs.append(x)
            if carried:
                inputs[0]["carry_len"], inputs[0]["carry_off"] = 38, 100
            with pytest.raises(ValueError):
                dev.run(0, inputs, 0, True, False, cap)
        blk = run_window(dev, 0, parts, case.flags, cap)                     # and the slot is none the worse for it
        check_window(blk, W.host_expect(parts, case.flags), case.flags, case.name)
    finally:
        dev.close()


# ---- B: the alignment check --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", (None,) + W.B_MOVED)
def test_b_a_member_that_begins_inside_a_record_is_reported(ctx, b):
    """2049 members, three segments a scan thread: the cut between members b and b + 1 moved into a record -- inside a thread's range
    and between two threads' ranges -- is `unaligned`; the same image with the cut where it belongs is not."""
    case = W.case_moved_cut(b)
    assert W.windows_of(case)[0][1]["unaligned"] == (b is not None)
    windows, outcomes = run_case(ctx, case)
    assert (outcomes[0] is None) == (b is not None)


def test_b_a_record_larger_than_a_member_is_reported(ctx):
    windows, outcomes = run_case(ctx, W.case_record_across_members())
    assert windows[0][1]["unaligned"] and outcomes == [None]


@pytest.mark.parametrize("eof", [0, 1])
@pytest.mark.parametrize("where", W.B_TAIL_CUTS)
def test_b_a_window_that_ends_inside_its_last_record(ctx, where, eof):
    """1 .. 4 bytes of the size word, half of the record, all but a byte: without eof the complete records and no byte of the cut
    one; with eof bad_block == 2."""
    windows, outcomes = run_case(ctx, W.case_cut_tail(where, eof))
    exp = windows[0][1]
    assert exp["bad_block"] == (2 if eof else 0)
    if not eof:
        assert outcomes[0]["n"] == 23


# ---- C: carried tails --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(W.C_TAILS)))
def test_c_a_tail_of_so_many_records_is_carried(ctx, i):
    """Two windows; the second carries file 1's tail of r records from the other slot (even i) or from its own (odd i): the pieces
    of 128 records, 64 pieces a workgroup of walk_kernel, parse_kernel with the device-side count."""
    case = W.case_tail(W.C_TAILS[i], same_slot=i % 2 == 1)
    windows, outcomes = run_case(ctx, case)
    assert len(outcomes) == 2 and outcomes[1]["n"] == windows[1][1]["n_rec"][0] and (case.slot_of(0) == case.slot_of(1)) == (i % 2 == 1)


@pytest.mark.parametrize("kind", ["mixed", "none", "one"])
def test_c_other_tails(ctx, kind):
    """A tail of 38-byte records with the 60 KB record among them (the pieces come from the record table); a last window that only
    carries, for both files and for one."""
    case = {"mixed": lambda: W.case_tail(200, mixed=True), "none": lambda: W.case_tail(129, last="none"),
            "one": lambda: W.case_tail(257, last="one")}[kind]()
    windows, outcomes = run_case(ctx, case)
    assert len(outcomes) == 2 and windows[1][1]["ended"]


def test_c_a_tail_that_would_overlap_itself_is_refused(ctx):
    """The same slot, carry_off < carry_len."""
    from xenomapper_amd import _ffi
    case = W.case_tail(129)                           # window 1: 6 pairs in front of a tail of 129 records
    windows = W.windows_of(case)
    dev = _ffi.BamDev(ctx)
    try:
        cap = reserve_for(dev, case, windows)
        (p1, e1), (p2, e2) = windows
        blk = run_window(dev, 0, p1, case.flags, cap)
        check_window(blk, W.host_expect(p1, case.flags), case.flags, case.name)
        assert blk.consumed[0] < p2[0].mid - p2[0].lo
        with pytest.raises(ValueError):
            run_window(dev, 0, p2, case.flags, cap, (0, blk.consumed))
        blk2 = run_window(dev, 1, p2, case.flags, cap, (0, blk.consumed))     # from the other slot it is carried
        check_window(blk2, W.host_expect(p2, case.flags), case.flags, case.name)
    finally:
        dev.close()


# ---- D: the chain adds up ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_records", W.D_MAX_RECORDS)
@pytest.mark.parametrize("combo", W.D_COMBOS)
def test_d_the_windows_of_a_file_pair_add_up(ctx, combo, max_records):
    """(paired, keep_halo, skip_repeated) x max_records: the files cut into windows by `consumed`, the slots in turn, other member
    budgets for the two files.  Every window is the model's (ended and starved too, only the last one ends); put together, the
    columns, unit bits, line flags and yielded record offsets are the model's of the whole files."""
    case = W.case_chain(combo, max_records)
    windows, outcomes = run_case(ctx, case)
    assert all(o is not None for o in outcomes)
    assert [e["ended"] for _p, e in windows] == [False] * (len(windows) - 1) + [True]
    got, want = W.concat_chain(case, windows, outcomes), W.whole_chain_expect(case, windows)
    assert got["n"] == want["n"]
    for key in ("cols", "flags", "pair_off"):
        assert all(np.array_equal(a, b) for a, b in zip(got[key], want[key])), key
    assert np.array_equal(got["bits"], want["bits"])


# ---- E: the pair kernel ------------------------------------------------------------------------------------------------------------
def test_e_pairs_on_both_sides_of_every_mask_word(ctx):
    """1 .. 4097 pairs a window, the largest first on one front end (a unit mask word or a column entry that a smaller window does
    not write keeps the larger one's): names of 1 .. 254 characters followed by bytes that differ between the files, runs of 1 .. 4
    equal names across records 63 | 64 and 255 | 256, flagged values, no mismatch."""
    from xenomapper_amd import _ffi
    dev = _ffi.BamDev(ctx)
    try:
        for n in sorted(W.E_PAIRS, reverse=True):
            windows, outcomes = run_case(ctx, W.case_pairs(n), dev)
            assert outcomes[0]["n"] == n and windows[0][1]["mismatch_at"] == -1
    finally:
        dev.close()


def test_e_the_first_mismatch_cuts_the_window(ctx):
    """Names that differ in the first byte only, in the last byte only, in length by one: at pairs 0, 1, 63, 64, 255, 256 and n - 1;
    of two the smaller; n and n_exceptions stop in front of it."""
    from xenomapper_amd import _ffi
    dev = _ffi.BamDev(ctx)
    try:
        seen = set()
        for case in W.e_cases():
            exp = W.windows_of(case)[0][1]
            if exp["mismatch_at"] < 0:
                continue
            windows, outcomes = run_case(ctx, case, dev)
            assert outcomes[0]["n"] == exp["mismatch_at"]
            seen.add((len(case.files[0].recs), exp["mismatch_at"]))
        assert {(4097, k) for k in W.E_MISMATCH_AT + (4096,)} <= seen and len(seen) >= 25
    finally:
        dev.close()


def test_e_a_name_that_ends_flush_with_the_reserved_window(ctx):
    """raw_bytes reserved = the window's bytes, whose last record is its 254-character name: the 16-byte compare reads behind the
    name, inside the 64 bytes the buffer has behind raw_bytes."""
    case = W.case_flush_name()
    windows, outcomes = run_case(ctx, case, exact_raw=True)
    assert outcomes[0]["n"] == 10 and windows[0][0][0].hi == windows[0][0][1].hi


# ---- more record starts than a block's slots hold ----------------------------------------------------------------------------------
@pytest.mark.parametrize("where,eof", [("last", 0), ("last", 1), ("middle", 0)])
def test_a_member_of_zero_bytes_is_reported_wherever_it_lies(ctx, where, eof):
    """A validly framed member of 4096 zero bytes is 1024 record starts where slot_of() leaves the block 115 slots: the inflate
    launch stops noting them (exit 0xFFFFFFFF) and fills no field.  scan_kernel must report that for every segment, the window's
    last one too -- `unaligned`, the host decoder names the file -- and an ordinary window on the same slot afterwards is exact."""
    from xenomapper_amd import _ffi
    parts = W.zero_member_parts(where, eof)
    after = W.case_segments(3)
    dev = _ffi.BamDev(ctx)
    try:
        cap = reserve_for(dev, after, W.windows_of(after))
        dev.reserve(0, 1 << 16, max(p.hi for p in parts) + 64, 64, 4096)
        blk = run_window(dev, 0, parts, W.BIG_FLAGS, dev.capacity(0)[3])
        assert (blk.bad_block, blk.unaligned) == (0, True)
        windows, outcomes = run_case(ctx, after, dev)
        assert outcomes[0]["n"] == 6 and cap <= dev.capacity(0)[3]
    finally:
        dev.close()


@pytest.mark.parametrize("block_size", [0, 1, 31])
def test_records_shorter_than_their_fixed_fields_are_malformed(ctx, block_size):
    """Two records of block_size < 32 in a member of their own (fewer than its slots): bad_block == 3."""
    from xenomapper_amd import _ffi
    parts = W.short_record_parts(block_size)
    dev = _ffi.BamDev(ctx)
    try:
        dev.reserve(0, 1 << 16, max(p.hi for p in parts) + 64, 64, 4096)
        blk = run_window(dev, 0, parts, W.BIG_FLAGS, 4096)
        assert (blk.bad_block, blk.unaligned) == (3, False)
    finally:
        dev.close()
