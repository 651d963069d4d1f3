"""SAM lines encoded as BAM alignment records ON the device (xm_strip_set_refs / xm_strip_fetch_bins_bam: E1 sizes, E2 writes, F frames;
include/xenomapper_strip.h) against the host encoder (xmh_sam_encode), which test_sam_records_cpu.py pins to the Python model and
the reference's fixture pairs.  Every stream is de-framed member by member (tests/sam_records.deframe: header, BSIZE, LEN / NLEN,
CRC-32, ISIZE) and the payload of every bin must equal the host's records of the bin's lines in bin_parts order.  Every check
counts the records and bytes it compared."""
import struct

import numpy as np
import pytest

from tests import sam_records as R
from tests import sam_shapes as S
from tests.test_sam_records_cpu import FIXTURES, bam_parts, sam_lines
from tests.test_strip_gpu import compare, strip                                    # noqa: F401  (run_block is built on them)
from tests.test_strip_shapes_gpu import MASKS, MODES, _STATE_TAGS, check_gather, run_block

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rig():
    from xenomapper_amd import _ffi, _host
    from xenomapper_amd.xenomapper import default_context
    s = _ffi.Stripper(default_context())
    p = _host.Parser(4)
    yield None, s, p
    s.close()
    p.close()


def expected_payload(parts, b, names, ref_shift):
    """the host's records of the lines of bin_parts, in that order; file 2's records of bin 4 with ref_shift"""
    from xenomapper_amd import _host
    out = []
    for f in (0, 1):
        mine = [text[:-1] for (_b, pf, _r), text in parts if pf == f]
        if not mine:
            out.append([])
            continue
        blob = b"\n".join(mine)
        off = np.cumsum([0] + [len(x) + 1 for x in mine[:-1]])
        rec, sizes, bad, reason = _host.sam_encode(blob, off, [len(x) for x in mine], names[f], ref_shift=ref_shift if (f == 1 and b == 4) else 0,
                                                   device_forms=True)
        assert bad is None, (bad, reason)
        cuts = np.concatenate(([0], np.cumsum(sizes.astype(np.int64))))
        out.append([rec[cuts[k]:cuts[k + 1]] for k in range(len(mine))])
    at = [0, 0]
    joined = []
    for (_b, f, _r), _text in parts:
        joined.append(out[f][at[f]])
        at[f] += 1
    return b"".join(joined), len(joined)


def check_bam(s, slot, n, paired, mask, lines, idx, off, names, P=0, ref_shift=0, guard=False):
    """One xm_strip_fetch_bins_bam against the host encoder -> (records compared, payload bytes compared, members)."""
    painted = None
    if guard:
        status, painted, ball, _ = s.fetch_bins_bam(slot, n, paired, S.ALL, P, ref_shift)
        assert status == 0
        s.out_wait(slot)
        painted[:] = 0xEE
    status, stream, boff, declined = s.fetch_bins_bam(slot, n, paired, mask, P, ref_shift)
    assert status == 0 and declined is None, (status, declined, mask)
    s.out_wait(slot)
    if guard:
        assert boff[7] <= ball[7] and (boff[7] == 0 or stream.ctypes.data == painted.ctypes.data)
        assert (painted[(boff[7] + 15) // 16 * 16:] == 0xEE).all()
    got = bytes(stream)
    assert boff[0] == 0 and boff[6] == boff[7] == len(got) and all(boff[b] <= boff[b + 1] for b in range(7)), boff
    n_rec = n_bytes = n_members = 0
    for b in range(6):
        parts = S.bin_parts(lines[0], lines[1], idx, off, paired, mask, b)
        piece = got[boff[b]:boff[b + 1]]
        if not parts:
            assert piece == b"", (b, boff)                                  # a bin without a sink or without units: no member at all
            continue
        payload, members = R.deframe(piece, P or 65280)
        want, k = expected_payload(parts, b, names, ref_shift)
        if payload != want:
            j = next((x for x in range(min(len(payload), len(want))) if payload[x] != want[x]), min(len(payload), len(want)))
            pytest.fail("bin %d: payload of %d bytes, want %d; first difference at byte %d: got %r, want %r" %
                        (b, len(payload), len(want), j, payload[max(0, j - 8):j + 24], want[max(0, j - 8):j + 24]))
        assert members == (len(want) + (P or 65280) - 1) // (P or 65280)
        n_rec += k
        n_bytes += len(want)
        n_members += members
    return n_rec, n_bytes, n_members


@pytest.fixture(scope="module")
def fixture_pair():
    (n1, _), (n2, _) = bam_parts(FIXTURES[0] + ".bam"), bam_parts(FIXTURES[1] + ".bam")
    l1, l2 = sam_lines(FIXTURES[0] + ".sam"), sam_lines(FIXTURES[1] + ".sam")
    return (n1, n2), b"\n".join(l1) + b"\n", b"\n".join(l2) + b"\n"


@pytest.mark.parametrize("mode", ["liberal", "conservative", "single"])
def test_fixture_pairs_in_every_mode_mask_slot_and_walk(rig, fixture_pair, mode):
    _ctx, s, _p = rig
    names, b1, b2 = fixture_pair
    for f in (0, 1):
        s.set_refs(f, names[f])
    paired = MODES[mode][1]
    records = nbytes = 0
    # (the skipping walk keeps one line of every name: no two records of a name are left for a paired unit -- single-end only)
    for slot, skip in ((0, False), (1, False)) + (((1, True), (0, True)) if mode == "single" else ()):
        got, lines, _line_off, idx, off = run_block(rig, slot, b1, b2, mode, 0, skip=skip)
        assert got.n > 200 and off[7] > 50
        for mask in MASKS:
            r, nb, _m = check_bam(s, slot, got.n, paired, mask, lines, idx, off, names, guard=mask != S.ALL)
            want = sum((off[b + 1] - off[b]) * (2 if paired else 1) * len(S.files_of_bin(b)) for b in range(6) if (mask >> b) & 1)
            assert r == want
            records += r
            nbytes += nb
    assert records > 1500 and nbytes > 300_000


def catalogue_block(states=(0, 1, 2, 3, 4, 5, 4, 4)):
    """the device-eligible catalogue lines as single-end records, the same line in both files but for the tags that decide the bin"""
    cat = [e for e in R.catalogue() if e[2] == 0 and not any(c in e[1] for c in b" \x0b\x0c\r\n")]
    out, state = [[], []], []
    for k, e in enumerate(cat):
        st = states[k % len(states)]
        state.append(st)
        for f in (0, 1):
            out[f].append(e[1] + _STATE_TAGS[st][f])
    return b"\n".join(out[0]) + b"\n", b"\r\n".join(out[1]) + b"\r\n", state, cat


def test_the_catalogue_on_the_device(rig):
    _ctx, s, _p = rig
    for f in (0, 1):
        s.set_refs(f, R.REFS)
    b1, b2, state, cat = catalogue_block()
    assert len(cat) > 150
    # a record can be larger than its line (a CIGAR operation of two characters is a word of four bytes: the 65535-operation line,
    # twice where its unit is unresolved): the stream is sized by the window, so the window is reserved for the records (else status 2)
    s.reserve(0, 1 << 20, 1 << 16)
    got, lines, _lo, idx, off = run_block(rig, 0, b1, b2, "single", 0)
    assert got.n == len(cat) and [off[b + 1] - off[b] for b in range(6)] == [state.count(b) for b in range(6)]
    total = 0
    for mask in (S.ALL, 0b010000, 0b000011):
        r, nb, _m = check_bam(s, 0, got.n, False, mask, lines, idx, off, (R.REFS, R.REFS))
        total += r
    assert total > 2 * len(cat)
    # every catalogue line was encoded from file 1 or file 2 (or both) under ALL, and prints back (CPU suite) as itself
    r, nb, members = check_bam(s, 0, got.n, False, S.ALL, lines, idx, off, (R.REFS, R.REFS), P=64)
    assert r == sum(len(S.files_of_bin(b)) * state.count(b) for b in range(6)) and members > nb // 64 - 6


@pytest.mark.parametrize("P", [64, 65, 4096, 0])
def test_member_seams(rig, fixture_pair, P):
    _ctx, s, _p = rig
    names, b1, b2 = fixture_pair
    for f in (0, 1):
        s.set_refs(f, names[f])
    got, lines, _lo, idx, off = run_block(rig, 1, b1, b2, "liberal", 0)
    r, nb, members = check_bam(s, 1, got.n, True, S.ALL, lines, idx, off, names, P=P)
    assert r > 400 and members >= (nb + (P or 65280) - 1) // (P or 65280)


def test_bins_of_exactly_k_members_and_of_one_record(rig):
    _ctx, s, _p = rig
    for f in (0, 1):
        s.set_refs(f, R.REFS)
    base = [R.make(qname=b"u%d" % k, l_seq=40, pos=1000 + k) for k in range(3)]
    state = [0, 0, 1]
    b1 = b"\n".join(base[k] + _STATE_TAGS[state[k]][0] for k in range(3)) + b"\n"
    b2 = b"\n".join(base[k] + _STATE_TAGS[state[k]][1] for k in range(3)) + b"\n"
    size = len(R.encode(base[0] + _STATE_TAGS[0][0], R.REFS))
    assert size == len(R.encode(base[2] + _STATE_TAGS[1][1], R.REFS)) and 64 <= size
    got, lines, _lo, idx, off = run_block(rig, 0, b1, b2, "single", 0)
    assert [off[b + 1] - off[b] for b in range(6)] == [2, 1, 0, 0, 0, 0]
    for P, want_members in ((size, 3), (2 * size, 2), (size - 1, 5), (size + 1, 3)):
        r, nb, members = check_bam(s, 0, 3, False, S.ALL, lines, idx, off, (R.REFS, R.REFS), P=P)
        assert (r, nb, members) == (3, 3 * size, want_members)
    r, nb, members = check_bam(s, 0, 3, False, 0b000010, lines, idx, off, (R.REFS, R.REFS))
    assert (r, nb, members) == (1, size, 1)


def test_ref_shift_only_on_file_two_in_unresolved_and_only_on_named_references(rig):
    _ctx, s, _p = rig
    for f in (0, 1):
        s.set_refs(f, R.REFS)
    rows = [(4, R.make(qname=b"a", rname=R.REFS[3], rnext=R.REFS[9])), (4, R.make(qname=b"b", rname=b"*", rnext=b"*", pos=0, pnext=0)),
            (4, R.make(qname=b"c", rname=R.REFS[4999], rnext=b"*")), (1, R.make(qname=b"d", rname=R.REFS[5])), (0, R.make(qname=b"e", rname=R.REFS[6]))]
    b1 = b"\n".join(line + _STATE_TAGS[st][0] for st, line in rows) + b"\n"
    b2 = b"\n".join(line + _STATE_TAGS[st][1] for st, line in rows) + b"\n"
    got, lines, _lo, idx, off = run_block(rig, 1, b1, b2, "single", 0)
    assert [off[b + 1] - off[b] for b in range(6)] == [1, 1, 0, 0, 3, 0]
    r, nb, _m = check_bam(s, 1, 5, False, S.ALL, lines, idx, off, (R.REFS, R.REFS), ref_shift=5000)
    assert r == 8
    status, stream, boff, _ = s.fetch_bins_bam(1, 5, False, S.ALL, 0, 5000)
    s.out_wait(1)
    recs = R.split_records(R.deframe(bytes(stream[boff[4]:boff[5]]))[0])
    ids = [(struct.unpack_from("<i", x, 0)[0], struct.unpack_from("<i", x, 20)[0]) for x in recs]
    assert ids == [(3, 9), (5003, 5009), (-1, -1), (-1, -1), (4999, -1), (9999, -1)]
    recs = R.split_records(R.deframe(bytes(stream[boff[1]:boff[2]]))[0])
    assert struct.unpack_from("<i", recs[0], 0)[0] == 5


DECLINED = [("aux_f", R.HOST_FLOAT), ("seq_lower", R.HOST_SEQ_CODE), ("aux_i_plus", R.HOST_NUMBER), ("cigar65536", R.HOST_LONG_CIGAR),
            ("rname_unknown", R.RNAME), ("qual_short", R.QUAL), ("aux_i_above", R.AUX_RANGE), ("qname255", R.QNAME), ("cigar_len_over", R.CIGAR)]


def test_declined_windows_and_an_ordinary_one_behind_them(rig):
    _ctx, s, _p = rig
    for f in (0, 1):
        s.set_refs(f, R.REFS)
    by_name = {e[0]: e for e in R.catalogue()}
    good = [R.make(qname=b"g%d" % k, l_seq=30 + k) for k in range(8)]
    seen = compared = 0
    for case, (name, reason) in enumerate(DECLINED):
        bad = by_name[name]
        assert bad[2] == reason
        at, slot = 2 + case % 5, case & 1
        for bad_file, st in ((0, 0), (1, 4)):
            if name == "qname255" and bad_file == 1:                      # (the mate in file 1 has the name too: it declines first)
                continue
            # the bad line in file `bad_file` only; its unit in bin st; the other file holds a good line of the same name
            qname = bad[1].split(b"\t")[0]
            mate = R.make(qname=qname, l_seq=12)
            rows = [(k % 2, g, g) for k, g in enumerate(good)]
            rows.insert(at, (st, bad[1], mate) if bad_file == 0 else (st, mate, bad[1]))
            b1 = b"\n".join(r[1] + _STATE_TAGS[r[0]][0] for r in rows) + b"\n"
            b2 = b"\n".join(r[2] + _STATE_TAGS[r[0]][1] for r in rows) + b"\n"
            got, lines, line_off, idx, off = run_block(rig, slot, b1, b2, "single", 0)
            status, stream, boff, declined = s.fetch_bins_bam(slot, got.n, False, S.ALL)
            assert status == 1 and stream is None and declined == (at, bad_file, reason), (name, bad_file, status, declined)
            # the same line in a bin without a sink: the window is encoded
            r, nb, _m = check_bam(s, slot, got.n, False, S.ALL & ~(1 << st), lines, idx, off, (R.REFS, R.REFS))
            compared += r
            seen += 1
    assert seen == 2 * len(DECLINED) - 1 and compared >= 4 * seen
    # a line with two tabs between fields: status 3, whatever else the window holds
    odd = good[3].replace(b"\t", b"\t\t", 1)
    b1 = b"\n".join((odd if k == 3 else g) + _STATE_TAGS[0][0] for k, g in enumerate(good)) + b"\n"
    b2 = b"\n".join(g + _STATE_TAGS[0][1] for g in good) + b"\n"
    _ctx2, _s2, p = rig
    got = strip(s, 0, b1, b2, True, True, 0, False, False, 1 << 16)
    _code, idx, off, _counts = s.classify(0, 0, got.n, -2 ** 31)
    status, stream, _boff, declined = s.fetch_bins_bam(0, got.n, False, S.ALL)
    assert status == 3 and stream is None and declined is None
    status, stream, boff, declined = s.fetch_bins_bam(0, got.n, False, 0b000010)
    assert status == 0 and boff[7] == 0
    # an ordinary window on the same slot afterwards is exact
    b1 = b"\n".join(g + _STATE_TAGS[k % 6][0] for k, g in enumerate(good)) + b"\n"
    b2 = b"\n".join(g + _STATE_TAGS[k % 6][1] for k, g in enumerate(good)) + b"\n"
    got, lines, _lo, idx, off = run_block(rig, 0, b1, b2, "single", 0)
    r, nb, _m = check_bam(s, 0, got.n, False, S.ALL, lines, idx, off, (R.REFS, R.REFS))
    assert r == 8 + 1 and nb > 800                                       # (one of the eight units is unresolved: both files)


def test_text_and_bam_fetches_in_either_order_on_one_block(rig, fixture_pair):
    _ctx, s, _p = rig
    names, b1, b2 = fixture_pair
    for f in (0, 1):
        s.set_refs(f, names[f])
    got, lines, line_off, idx, off = run_block(rig, 0, b1, b2, "conservative", 0)
    first = check_bam(s, 0, got.n, True, S.ALL, lines, idx, off, names)
    _pieces, n_lines, n_bytes = check_gather(s, 0, got.n, True, S.ALL, lines, line_off, idx, off)
    again = check_bam(s, 0, got.n, True, S.ALL, lines, idx, off, names, P=4096)
    _pieces, n_lines2, n_bytes2 = check_gather(s, 0, got.n, True, 0b010110, lines, line_off, idx, off)
    assert first[0] == again[0] == n_lines > 400 and first[1] == again[1] and n_bytes > first[1] and 0 < n_lines2 < n_lines


def test_without_references_the_call_is_refused():
    from xenomapper_amd import _ffi
    from xenomapper_amd.xenomapper import default_context
    s = _ffi.Stripper(default_context())
    try:
        good = [R.make(qname=b"g%d" % k) + _STATE_TAGS[0][0] for k in range(4)]
        text = b"\n".join(good) + b"\n"
        got = strip(s, 0, text, text.replace(b"\tAS:i:0", b""), True, True, 0, False, False, 64)
        s.classify(0, 0, got.n, -2 ** 31)
        with pytest.raises(Exception):
            s.fetch_bins_bam(0, got.n, False, S.ALL)
        s.set_refs(1, R.REFS)                                               # file 2's alone do not serve bin 0
        with pytest.raises(Exception):
            s.fetch_bins_bam(0, got.n, False, 0b000001)
        status, _stream, boff, _ = s.fetch_bins_bam(0, got.n, False, 0b000010)     # bin 1 is file 2's (and empty here)
        assert status == 0 and boff[7] == 0
        with pytest.raises(Exception):
            s.set_refs(0, [b"chr1", b"chr1"])
        s.set_refs(0, R.REFS)
        status, stream, boff, _ = s.fetch_bins_bam(0, got.n, False, S.ALL)
        s.out_wait(0)
        assert status == 0 and len(R.split_records(R.deframe(bytes(stream))[0])) == 4
    finally:
        s.close()
