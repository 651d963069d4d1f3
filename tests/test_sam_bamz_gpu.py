"""SAM lines encoded as BAM records AND deflated on the device (xm_strip_fetch_bins_bamz: E1 sizes, E2 writes, then the member
descriptors, the DEFLATE encoder, the CRC kernel, the place scan and the pack kernel of the compressed BAM route;
include/xenomapper_strip.h).  Three checks per bin: its bytes equal what Context.bgzf_compress makes of the expected records at the
same payload, byte for byte; every member, read here with zlib and without the library, inflates, carries the right CRC-32 and ISIZE
and -- but a bin's last -- holds exactly P bytes; the payloads put together are the host encoder's records.  Every check counts what it
compared."""
import struct
import zlib

import numpy as np
import pytest

from tests import sam_records as R
from tests import sam_shapes as S
from tests.test_sam_records_gpu import DECLINED, catalogue_block, check_bam, expected_payload, fixture_pair, rig    # noqa: F401
from tests.test_strip_gpu import compare, strip                                    # noqa: F401  (run_block is built on them)
from tests.test_strip_shapes_gpu import MASKS, MODES, _STATE_TAGS, check_gather, run_block

pytestmark = pytest.mark.gpu


def members_of(piece):
    """the BGZF members of `piece`, read by hand: [(payload bytes, member bytes)]; header, BSIZE, CRC-32 and ISIZE are checked"""
    out, at = [], 0
    while at < len(piece):
        assert len(piece) - at >= 26, "a member is cut short"
        assert piece[at:at + 16] == bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]), piece[at:at + 16]
        size = struct.unpack_from("<H", piece, at + 16)[0] + 1
        assert at + size <= len(piece)
        inflater = zlib.decompressobj(-15)
        payload = inflater.decompress(piece[at + 18:at + size - 8])
        assert inflater.eof and inflater.unused_data == b""
        crc, isize = struct.unpack_from("<II", piece, at + size - 8)
        assert isize == len(payload) and crc == zlib.crc32(payload) & 0xFFFFFFFF
        out.append((payload, size))
        at += size
    return out


def check_bamz(s, slot, n, paired, mask, lines, idx, off, names, P=0, ref_shift=0, guard=False):
    """One xm_strip_fetch_bins_bamz against Context.bgzf_compress of the host's records
    -> (records, payload bytes, members, stream bytes) compared."""
    from xenomapper_amd.xenomapper import default_context
    ctx = default_context()
    painted = None
    if guard:                                                           # the stored stream of all bins is longer than any deflated one
        status, painted, ball, _ = s.fetch_bins_bam(slot, n, paired, S.ALL, P, ref_shift)
        assert status == 0
        s.out_wait(slot)
        painted[:] = 0xEE
    status, stream, boff, declined = s.fetch_bins_bamz(slot, n, paired, mask, P, ref_shift)
    assert status == 0 and declined is None, (status, declined, mask)
    s.out_wait(slot)
    if guard:
        assert boff[7] <= ball[7] and (boff[7] == 0 or stream.ctypes.data == painted.ctypes.data)
        assert (painted[(boff[7] + 15) // 16 * 16:] == 0xEE).all()     # nothing is written past bin_off[7]
    got = bytes(stream)
    assert boff[0] == 0 and boff[6] == boff[7] == len(got) and all(boff[b] <= boff[b + 1] for b in range(7)), boff
    payload_of_member = P or 65280
    n_rec = n_bytes = n_members = n_stream = 0
    for b in range(6):
        parts = S.bin_parts(lines[0], lines[1], idx, off, paired, mask, b)
        piece = got[boff[b]:boff[b + 1]]
        if not parts:
            assert piece == b"", (b, boff)                              # a bin without a sink or without units: no member at all
            continue
        want, k = expected_payload(parts, b, names, ref_shift)
        # (1) the bytes: xm_bgzf_compress of the bin's records, member for member
        ref = bytes(ctx.bgzf_compress(want, P))
        if piece != ref:
            j = next((x for x in range(min(len(piece), len(ref))) if piece[x] != ref[x]), min(len(piece), len(ref)))
            pytest.fail("bin %d: %d bytes, xm_bgzf_compress makes %d; first difference at byte %d" % (b, len(piece), len(ref), j))
        # (2) the members, read without the library
        members = members_of(piece)
        assert len(members) == (len(want) + payload_of_member - 1) // payload_of_member
        assert all(len(m[0]) == payload_of_member for m in members[:-1]) and 0 < len(members[-1][0]) <= payload_of_member
        assert all(size <= len(m) + 31 for m, size in members)         # never longer than the stored form
        # (3) the payload: the host encoder's records
        payload = b"".join(m[0] for m in members)
        if payload != want:
            j = next((x for x in range(min(len(payload), len(want))) if payload[x] != want[x]), min(len(payload), len(want)))
            pytest.fail("bin %d: payload of %d bytes, want %d; first difference at byte %d" % (b, len(payload), len(want), j))
        n_rec += k
        n_bytes += len(want)
        n_members += len(members)
        n_stream += len(piece)
    return n_rec, n_bytes, n_members, n_stream


@pytest.mark.parametrize("mode", ["liberal", "single"])
def test_fixture_pair_in_both_slots_and_every_mask(rig, fixture_pair, mode):
    _ctx, s, _p = rig
    names, b1, b2 = fixture_pair
    for f in (0, 1):
        s.set_refs(f, names[f])
    paired = MODES[mode][1]
    records = nbytes = zbytes = 0
    for slot in (0, 1):
        got, lines, _line_off, idx, off = run_block(rig, slot, b1, b2, mode, 0)
        assert got.n > 200 and off[7] > 50
        for mask in MASKS:
            r, nb, _m, zb = check_bamz(s, slot, got.n, paired, mask, lines, idx, off, names, guard=mask != S.ALL)
            want = sum((off[b + 1] - off[b]) * (2 if paired else 1) * len(S.files_of_bin(b)) for b in range(6) if (mask >> b) & 1)
            assert r == want
            records += r
            nbytes += nb
            zbytes += zb
    assert records > 1000 and nbytes > 200_000 and 0 < zbytes < nbytes


@pytest.mark.parametrize("P", [64, 65, 4096, 0])
def test_member_seams(rig, fixture_pair, P):
    _ctx, s, _p = rig
    names, b1, b2 = fixture_pair
    for f in (0, 1):
        s.set_refs(f, names[f])
    got, lines, _lo, idx, off = run_block(rig, 1, b1, b2, "liberal", 0)
    r, nb, members, _zb = check_bamz(s, 1, got.n, True, S.ALL, lines, idx, off, names, P=P)
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
        r, nb, members, _zb = check_bamz(s, 0, 3, False, S.ALL, lines, idx, off, (R.REFS, R.REFS), P=P)
        assert (r, nb, members) == (3, 3 * size, want_members)
    r, nb, members, _zb = check_bamz(s, 0, 3, False, 0b000010, lines, idx, off, (R.REFS, R.REFS))
    assert (r, nb, members) == (1, size, 1)


def test_the_catalogue_on_the_device(rig):
    _ctx, s, _p = rig
    for f in (0, 1):
        s.set_refs(f, R.REFS)
    b1, b2, state, cat = catalogue_block()
    assert len(cat) > 150
    s.reserve(0, 1 << 20, 1 << 16)              # (a record can be larger than its line: the window is reserved for the records)
    got, lines, _lo, idx, off = run_block(rig, 0, b1, b2, "single", 0)
    assert got.n == len(cat) and [off[b + 1] - off[b] for b in range(6)] == [state.count(b) for b in range(6)]
    want_records = sum(len(S.files_of_bin(b)) * state.count(b) for b in range(6))
    r, nb, members, _zb = check_bamz(s, 0, got.n, False, S.ALL, lines, idx, off, (R.REFS, R.REFS), P=64)
    assert r == want_records and members > nb // 64 - 6
    r, nb0, members0, _zb = check_bamz(s, 0, got.n, False, S.ALL, lines, idx, off, (R.REFS, R.REFS), P=0)
    # the 65535-operation line alone is 4 x 65535 bytes of CIGAR words: it spans several members at the largest payload too
    assert r == want_records and nb0 == nb and nb0 > 4 * 65535 and members0 >= nb0 // 65280 and members0 > 4


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
    r, _nb, _m, _zb = check_bamz(s, 1, 5, False, S.ALL, lines, idx, off, (R.REFS, R.REFS), ref_shift=5000)
    assert r == 8
    status, stream, boff, _ = s.fetch_bins_bamz(1, 5, False, S.ALL, 0, 5000)
    assert status == 0
    s.out_wait(1)
    got_bytes = bytes(stream)
    recs = R.split_records(b"".join(m[0] for m in members_of(got_bytes[boff[4]:boff[5]])))
    ids = [(struct.unpack_from("<i", x, 0)[0], struct.unpack_from("<i", x, 20)[0]) for x in recs]
    assert ids == [(3, 9), (5003, 5009), (-1, -1), (-1, -1), (4999, -1), (9999, -1)]
    recs = R.split_records(b"".join(m[0] for m in members_of(got_bytes[boff[1]:boff[2]])))
    assert struct.unpack_from("<i", recs[0], 0)[0] == 5


def test_declined_windows_and_an_ordinary_one_behind_them(rig):
    _ctx, s, _p = rig
    for f in (0, 1):
        s.set_refs(f, R.REFS)
    by_name = {e[0]: e for e in R.catalogue()}
    good = [R.make(qname=b"g%d" % k, l_seq=30 + k) for k in range(8)]
    seen = compared = 0
    for case, (name, reason) in enumerate(DECLINED):
        bad = by_name[name]
        at, slot = 2 + case % 5, case & 1
        bad_file, st = ((0, 0), (1, 4))[case % 2 if name != "qname255" else 0]
        qname = bad[1].split(b"\t")[0]
        mate = R.make(qname=qname, l_seq=12)
        rows = [(k % 2, g, g) for k, g in enumerate(good)]
        rows.insert(at, (st, bad[1], mate) if bad_file == 0 else (st, mate, bad[1]))
        b1 = b"\n".join(r[1] + _STATE_TAGS[r[0]][0] for r in rows) + b"\n"
        b2 = b"\n".join(r[2] + _STATE_TAGS[r[0]][1] for r in rows) + b"\n"
        got, lines, _line_off, idx, off = run_block(rig, slot, b1, b2, "single", 0)
        stored = s.fetch_bins_bam(slot, got.n, False, S.ALL)
        deflated = s.fetch_bins_bamz(slot, got.n, False, S.ALL)
        assert stored[0] == 1 and stored[1] is None and stored[3] == (at, bad_file, reason), (name, stored)
        assert deflated[0] == stored[0] and deflated[1] is None and deflated[2] is None and deflated[3] == stored[3], (name, deflated, stored)
        # the same line in a bin without a sink: the window is encoded
        r, _nb, _m, _zb = check_bamz(s, slot, got.n, False, S.ALL & ~(1 << st), lines, idx, off, (R.REFS, R.REFS))
        compared += r
        seen += 1
    assert seen == len(DECLINED) and compared >= 4 * seen
    # a line with two tabs between fields: status 3 as the stored call says, whatever else the window holds
    odd = good[3].replace(b"\t", b"\t\t", 1)
    b1 = b"\n".join((odd if k == 3 else g) + _STATE_TAGS[0][0] for k, g in enumerate(good)) + b"\n"
    b2 = b"\n".join(g + _STATE_TAGS[0][1] for g in good) + b"\n"
    got = strip(s, 0, b1, b2, True, True, 0, False, False, 1 << 16)
    s.classify(0, 0, got.n, -2 ** 31)
    stored = s.fetch_bins_bam(0, got.n, False, S.ALL)
    deflated = s.fetch_bins_bamz(0, got.n, False, S.ALL)
    assert stored[0] == 3 and deflated[0] == 3 and deflated[1] is None and deflated[3] is None
    status, _stream, boff, _declined = s.fetch_bins_bamz(0, got.n, False, 0b000010)
    assert status == 0 and boff[7] == 0
    # an ordinary window on the same slot afterwards is exact
    b1 = b"\n".join(g + _STATE_TAGS[k % 6][0] for k, g in enumerate(good)) + b"\n"
    b2 = b"\n".join(g + _STATE_TAGS[k % 6][1] for k, g in enumerate(good)) + b"\n"
    got, lines, _lo, idx, off = run_block(rig, 0, b1, b2, "single", 0)
    r, nb, _m, _zb = check_bamz(s, 0, got.n, False, S.ALL, lines, idx, off, (R.REFS, R.REFS))
    assert r == 8 + 1 and nb > 800                                       # (one of the eight units is unresolved: both files)


def test_stored_text_and_deflated_fetches_in_either_order_on_one_block(rig, fixture_pair):
    _ctx, s, _p = rig
    names, b1, b2 = fixture_pair
    for f in (0, 1):
        s.set_refs(f, names[f])
    got, lines, line_off, idx, off = run_block(rig, 0, b1, b2, "conservative", 0)
    first = check_bamz(s, 0, got.n, True, S.ALL, lines, idx, off, names)
    stored = check_bam(s, 0, got.n, True, S.ALL, lines, idx, off, names)
    _pieces, n_lines, n_bytes = check_gather(s, 0, got.n, True, S.ALL, lines, line_off, idx, off)
    again = check_bamz(s, 0, got.n, True, S.ALL, lines, idx, off, names, P=4096)
    stored2 = check_bam(s, 0, got.n, True, 0b010110, lines, idx, off, names, P=4096)
    last = check_bamz(s, 0, got.n, True, 0b010110, lines, idx, off, names)
    assert first[0] == again[0] == stored[0] == n_lines > 400 and first[1] == again[1] == stored[1] and n_bytes > first[1]
    assert 0 < last[0] == stored2[0] < n_lines and first[3] < stored[1]


def test_refused_arguments():
    from xenomapper_amd import _ffi
    from xenomapper_amd.xenomapper import default_context
    s = _ffi.Stripper(default_context())
    try:
        good = [R.make(qname=b"g%d" % k) + _STATE_TAGS[0][0] for k in range(4)]
        text = b"\n".join(good) + b"\n"
        got = strip(s, 0, text, text.replace(b"\tAS:i:0", b""), True, True, 0, False, False, 64)
        s.classify(0, 0, got.n, -2 ** 31)
        with pytest.raises(ValueError):                                     # XM_ERR_INVALID_ARG: no references set
            s.fetch_bins_bamz(0, got.n, False, S.ALL)
        s.set_refs(1, R.REFS)                                               # file 2's alone do not serve bin 0
        with pytest.raises(ValueError):
            s.fetch_bins_bamz(0, got.n, False, 0b000001)
        status, _stream, boff, _ = s.fetch_bins_bamz(0, got.n, False, 0b000010)    # bin 1 is file 2's (and empty here)
        assert status == 0 and boff[7] == 0
        s.set_refs(0, R.REFS)
        for P in (63, 65281):
            with pytest.raises(ValueError):
                s.fetch_bins_bamz(0, got.n, False, S.ALL, P)
        status, stream, boff, _ = s.fetch_bins_bamz(0, got.n, False, S.ALL, 64)
        s.out_wait(0)
        assert status == 0 and len(R.split_records(b"".join(m[0] for m in members_of(bytes(stream))))) == 4
    finally:
        s.close()
