"""The SAM front end's middle kernels (xm_strip.hip: S4 parse_kernel, S5 start_*, S6 pair_kernel with same_bytes, S7 cig_scan_kernel /
cig_write_kernel) on the catalogue of tests/sam_field_shapes.py, through xm_strip_run on the C ABI: tag letters, colons and values on
every offset of the 32-byte load step, text that must not count as a tag, one-character fields, every separator, every value form,
CIGARs of 255 operations and more on the tile edges, names of every length on every pair of alignments, and short windows on a slot
that still holds a longer window's text.  Every case is compared twice, exactly: with the host stripper field by field (compare() of
tests/test_strip_gpu.py) and with the oracle through the direct check of tests/strip_check.py; tests/test_sam_field_shapes_cpu.py
holds the catalogue to its claims and the host stripper to the same check."""
import numpy as np
import pytest

from tests import sam_field_shapes as F
from tests.strip_check import direct_check
from tests.test_strip_gpu import compare, device_cigar, rig        # noqa: F401 (rig: the module's fixture, one per importing module)

pytestmark = pytest.mark.gpu

MAX_RECORDS = 1 << 14


def run_case(rig, c, slot):
    """One case on one slot: the device block against the host stripper's and against the oracle, then against what the case expects."""
    from xenomapper_amd import _ffi
    _ctx, s, p = rig
    b1, b2 = c.windows
    got, want = compare(s, p, b1, b2, True, True, c.score_mode, c.paired, False, MAX_RECORDS, slot=slot, skip=c.skip)
    assert want is not None and not got.overflow, c.name
    cig = device_cigar(s, slot, got.n) if c.score_mode == 2 else None
    pairs, err = direct_check(got, b1, b2, c.score_mode, c.paired, c.skip, cig)
    assert len(pairs) == c.expect["n"] and (err == "mismatch") == c.expect["mismatch"], c.name
    assert sorted({(k, col) for k, col, _kind in got.exc}) == [tuple(x) for x in c.expect["flags"]], c.name
    if c.score_mode == 2 and got.n:                   # the packed columns against the host packer on the host stripper's CSR, trailers included
        for f in (0, 1):
            nm, off, ops = want.csr[f]
            cnt, tile, packed = _ffi.cigar_pack(off, ops)
            gnm, gcnt, gtile, gops = s.cigar_columns(slot, f, got.n)
            assert np.array_equal(gnm, nm) and np.array_equal(gcnt, cnt), c.name
            assert np.array_equal(gtile[:_ffi.cigar_tiles(got.n) + 1], tile[:_ffi.cigar_tiles(got.n) + 1]), c.name
            assert gops.shape[0] == packed.shape[0] == int(off[-1]) + int((cnt == 255).sum()) and np.array_equal(gops, packed), c.name
    return got, want


@pytest.mark.parametrize("group", [g for g in F.GROUPS if g != "stale"])
def test_every_case_of_the_group_equals_the_host_stripper_and_the_oracle(rig, group):
    ctx, s, _p = rig
    from xenomapper_amd import _ffi
    cases = F.cases_of(group)
    assert cases
    for j, c in enumerate(cases):
        got, want = run_case(rig, c, j & 1)
        if "records_over" in c.claims:                # the tile-edge window: the fused pass on the device's packed columns
            code, idx, off, counts = s.classify(j & 1, _ffi.MODE_PE_LIBERAL, got.n, -2**31)
            h = ctx.classify_compact_cigar(_ffi.MODE_PE_LIBERAL, want.csr[0][0], want.csr[0][1], want.csr[0][2], want.cols[1],
                                           want.csr[1][0], want.csr[1][1], want.csr[1][2], want.cols[3], want.unit_bits, -2**31)
            assert np.array_equal(code, h[0]) and np.array_equal(idx, h[1]) and np.array_equal(off, h[2]) and np.array_equal(counts, h[3])
            assert int(counts.sum()) == got.n // 2


def test_a_short_window_on_a_slot_that_holds_a_longer_windows_text(rig):
    """The stale pairs in order, both windows of a pair on one slot: the short window's last line has no terminator and the slot's
    buffers go on behind it with the long window's text -- a longer name, more optional fields, the rest of a tag, another digit,
    more CIGAR operations.  S4 and S6 read past a line's end; their masks must not let a byte of it count."""
    _ctx, s, _p = rig
    cases = F.cases_of("stale")
    assert len(cases) >= 30 and len(cases) % 2 == 0
    for j in range(0, len(cases), 2):
        long_, short = cases[j], cases[j + 1]
        assert short.after == long_.name
        slot = (j >> 1) & 1
        run_case(rig, long_, slot)
        got, _want = run_case(rig, short, slot)
        cont = short.claims["continues"].encode()
        for f in (0, 1):                              # the short run has left the text behind its end where it was
            n = len(short.windows[f])
            assert bytes(s.staging(slot, f)[n:n + len(cont)]) == cont
        assert got.n == 7 and got.ended
