"""The hand-made DEFLATE corpus (tests/deflate_asm.py) against the reference, zlib, and through the decoder's host build.

zlib accepts a member <=> the decoder's status is 0, and then the bytes are equal; a member with one defect ends with the status
that names the defect.  First the corpus itself is held to zlib and to its own record of what it covers (a corpus that silently
lost its 48-bit token would test nothing); then every stream goes through xenomapper_amd/csrc/xm_inflate_core.h compiled for the
host as a chain of one lane (tests/inflate_core_host.cpp --streams, a stand-alone program under ASan + UBSan), at two output
alignments and two input shifts.  The kernel's own run of the same members is tests/test_inflate_streams_gpu.py."""
import functools

from tests import deflate_asm as A
from tests import helpers as H


@functools.lru_cache(maxsize=None)
def corpus():
    return A.valid_corpus(), A.invalid_corpus()


def union(entries, key):
    got = set()
    for e in entries:
        got |= e.rec[key]
    return got


def test_zlib_inflates_every_valid_stream_to_the_interpreters_bytes():
    valid, _ = corpus()
    assert len(valid) >= 60
    import zlib
    for v in valid:
        d = zlib.decompressobj(-15)
        got = d.decompress(v.stream)
        assert got == v.expected, v.name
        assert d.eof and d.unused_data == b"" and d.unconsumed_tail == b"", v.name
        assert len(v.stream) <= A.MAX_CDATA and 1 <= len(v.expected) <= A.MAX_ISIZE, v.name
        assert A.zlib_verdict(v.stream, len(v.expected)) == (True, v.expected), v.name


def test_zlib_refuses_every_invalid_member():
    """zlib raises, or does not reach the end of the stream within the data -- or, for the three members whose one defect is the
    ISIZE beside a sound stream, reaches it with another byte count than the member states (the defect is the member's then, and
    inflate alone cannot see it)."""
    import zlib
    _, invalid = corpus()
    by_isize = {"literal_past_isize", "match_ends_past_isize", "end_of_block_short_of_isize"}
    for v in invalid:
        d = zlib.decompressobj(-15)
        try:
            got = d.decompress(v.stream)
        except zlib.error:
            assert v.name not in by_isize, v.name
            continue
        if v.name in by_isize:
            assert d.eof and len(got) != v.isize, v.name
        else:
            assert not d.eof, v.name
        assert A.zlib_verdict(v.stream, v.isize)[0] is False, v.name


def test_the_corpus_covers_what_it_claims():
    valid, invalid = corpus()
    lens = union(valid, "len_pairs")
    dists = union(valid, "dist_pairs")
    for cls in ("fixed", "root", "long"):
        assert {(s, k) for c, s, k in lens if c == cls} == {(s, k) for s in range(257, 286) for k in ("zero", "ones")}, cls
        assert {(s, k) for c, s, k in dists if c == cls} == {(s, k) for s in range(30) for k in ("zero", "ones")}, cls
    bits = union(valid, "token_bits")
    assert 1 in bits and 48 in bits and max(bits) == 48
    assert {10, 11, 15} <= union(valid, "lit_lens") and {1, 8, 9, 15} <= union(valid, "dist_lens") and 7 in union(valid, "clc_lens")
    assert {257, 286} <= union(valid, "hlit") and {1, 30} <= union(valid, "hdist") and 19 in union(valid, "hclen")
    assert 4 in union(invalid, "hclen")                                   # HCLEN 4 cannot send a length other than 0
    assert union(valid, "paddings") == set(range(8)) and union(valid, "blocks") == {0, 1, 2}
    assert max(v.rec["n_blocks"] for v in valid) >= 301
    assert max(len(v.stream) for v in valid) == A.MAX_CDATA
    want = set(range(1, 12)) | {A.ERR_INCOMPLETE}
    assert {v.status for v in invalid} == want
    assert sum(v.status == A.ERR_INCOMPLETE for v in invalid) == 3 and sum(v.status == A.ERR_OVERSUB for v in invalid) == 3
    assert sum(v.status == A.ERR_DIST for v in invalid) == 3


def test_the_host_build_of_the_decoder_on_every_stream(tmp_path):
    valid, invalid = corpus()
    exe = A.build_host_decoder(H.REPO, str(tmp_path / "inflate_core_host"))
    jobs, names = [], []
    for rnd, (align0, shift0) in enumerate(((0, 0), (5, 77))):
        for k, v in enumerate(valid):
            jobs.append((v.stream, len(v.expected), (align0 + 3 * k) % 16, shift0 + (29 * k) % 128 * rnd))
            names.append(v)
        for k, v in enumerate(invalid):
            jobs.append((v.stream, v.isize, (align0 + 7 * k) % 16, shift0 + (13 * k) % 128 * rnd))
            names.append(v)
    results, counters = A.run_host_decoder(exe, jobs, str(tmp_path))
    assert len({j[2] for j in jobs}) == 16
    poison = bytes([A.POISON]) * A.GUARD
    wrong = []
    for v, (status, front, body, back) in zip(names, results):
        assert front == poison and back == poison, "%s: wrote outside its output" % v.name
        if isinstance(v, A.Valid):
            if status != 0 or body != v.expected:
                wrong.append((v.name, status, "bytes differ" if status == 0 else ""))
        elif status != v.status:
            wrong.append((v.name, status, "want %d" % v.status))
    assert not wrong, wrong
    assert counters["stored"] and counters["fixed"] and counters["dynamic"] and counters["long_lit"] and counters["long_dist"], counters


def test_single_bit_damage_the_host_builds_verdict_is_zlibs(tmp_path):
    """One flipped bit in every stream of the corpus, twenty times: the decoder accepts the member exactly when zlib reaches the
    end of the stream, and then their bytes are equal (a flip that leaves a sound stream is as good a test as one that does not)."""
    damaged = A.damaged_corpus()
    assert len(damaged) > 1500 and 300 < sum(d.accepted for d in damaged) < len(damaged) - 300
    exe = A.build_host_decoder(H.REPO, str(tmp_path / "inflate_core_host"))
    results, _ = A.run_host_decoder(exe, [(d.stream, d.isize, (5 * k) % 16, (37 * k) % 128) for k, d in enumerate(damaged)], str(tmp_path))
    poison = bytes([A.POISON]) * A.GUARD
    wrong = []
    for d, (status, front, body, back) in zip(damaged, results):
        assert front == poison and back == poison, "%s: wrote outside its output" % d.name
        if (status == 0) != d.accepted or (d.accepted and body != d.expected):
            wrong.append((d.name, status, d.accepted))
    assert not wrong, wrong[:12]
