"""The CIGAR-score kernels on the catalogue of tests/cigar_shapes.py: every case through every entry point that scores CIGARs,
in the three modes, with min_score absent and -41, bit for bit against the oracle's classify and compact applied to the scores
of cigar_shapes.score (plain Python integers); K3's column against those scores directly.  Every output sits between 64 guard
entries of a poison value; the inputs are compared with what was uploaded; range_flag is non-zero exactly when the reference
clamped a score, which only the cases of the group `range` do (the outputs then hold the clamped scores' results)."""
import itertools

import numpy as np
import pytest

from tests import cigar_shapes as S
from tests import helpers as H

pytestmark = pytest.mark.gpu

ABSENT = -2**31
GUARD = 64
POISON = {np.dtype(np.uint8): 0x5A, np.dtype(np.int32): 0x5A5A5A5A, np.dtype(np.int64): 0x5A5A5A5A5A5A5A5A}
M_FLOORS = (ABSENT, -41)


@pytest.fixture(scope="module")
def ctx():
    from xenomapper_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


class Guarded(object):
    """A device buffer of `size` entries between GUARD entries of poison on either side (the buffer itself holds poison too)."""

    def __init__(self, size, dtype):
        import torch
        self.size, self.dtype = int(size), np.dtype(dtype)
        tdtype = {np.dtype(np.uint8): torch.uint8, np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64}[self.dtype]
        self.whole = torch.full((self.size + 2 * GUARD,), POISON[self.dtype], dtype=tdtype, device="cuda:0")
        self.t = self.whole[GUARD:GUARD + self.size]

    def host(self, what):
        """The buffer's entries, once the guards on both sides are seen to hold the poison still."""
        h = self.whole.cpu().numpy()
        assert (h[:GUARD] == POISON[self.dtype]).all(), "%s: written in front of the buffer" % what
        assert (h[GUARD + self.size:] == POISON[self.dtype]).all(), "%s: written behind the buffer" % what
        return h[GUARD:GUARD + self.size]


def upload(arrays):
    import torch
    out = []
    for a in arrays:
        if a.shape[0] == 0:
            a = np.zeros(4, dtype=a.dtype)
        signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
        out.append(torch.from_numpy(np.ascontiguousarray(a.view(signed) if signed else a)).to("cuda:0"))
    return out


def unchanged(dev, host, what):
    for k, (d, h) in enumerate(zip(dev, host)):
        got = d.cpu().numpy().view(h.dtype)[:h.shape[0]]
        assert np.array_equal(got, h), "%s: input column %d was written" % (what, k)


class Want(object):
    def __init__(self, mode, sp, bits, m):
        self.code, self.counts = H.c_classify(mode, sp[0]["score"], sp[0]["xs"], sp[1]["score"], sp[1]["xs"], bits, m)
        self.idx, self.off = H.c_compact(mode, self.code)
        self.bins = np.full(self.code.shape[0], 7, dtype=np.uint8)
        for b in range(7):
            self.bins[self.idx[int(self.off[b]):int(self.off[b + 1])]] = b


def check_flag(flag, bad, what):
    f = flag.host(what + " range_flag")
    assert (int(f[0]) != 0) == (bad != 0), "%s: range_flag %d, the reference clamped %d scores" % (what, int(f[0]), bad)


def check_compact(want, n, code, bins4, idx, off, counts, what):
    from xenomapper_amd import _ffi
    if code is not None:
        assert np.array_equal(code.host(what + " code"), want.code), what + " code"
    if bins4 is not None:
        assert np.array_equal(_ffi.unpack_bins4(bins4.host(what + " bins4"), n), want.bins), what + " bins4"
    assert np.array_equal(counts.host(what + " counts").astype(np.uint64), want.counts), what + " counts"
    h_off = off.host(what + " offsets").astype(np.uint64)
    assert np.array_equal(h_off, want.off), what + " offsets"
    assert np.array_equal(idx.host(what + " idx")[:int(h_off[7])].view(np.uint32), want.idx), what + " idx"


def new_flag():
    f = Guarded(1, np.int32)
    f.t.zero_()
    return f


@pytest.mark.parametrize("case", S.all_cases(), ids=lambda c: c.name)
def test_cigar_case(ctx, case):
    import torch
    from xenomapper_amd import _ffi
    sp, flags = case.columns()
    n, bad = case.n, case.bad
    assert (bad != 0) <= (case.group == "range")
    bits = S.pack_bits(flags)
    csr_host = [a for s in sp for a in (s["nm"], s["cig_off"], s["cig_oplen"], s["xs"])] + [bits]
    packed = [s["packed"] if s["packed"] is not None else _ffi.cigar_pack(s["cig_off"], s["cig_oplen"]) for s in sp]
    pk_host = [a for s, (cnt, tile, ops) in zip(sp, packed) for a in (s["nm"], cnt, tile, ops, s["xs"])] + [bits]
    csr_host = [a.copy() for a in csr_host]
    pk_host = [a.copy() for a in pk_host]
    d_csr, d_pk = upload(csr_host), upload(pk_host)
    nb = _ffi.bins4_bytes(n)

    for mode, m in itertools.product((0, 1, 2), M_FLOORS):
        want = Want(mode, sp, bits, m)
        tag = "%s mode %d m %d" % (case.name, mode, m)
        # K1p: the fused call on packed columns in its three output forms ...
        for form in ("code", "bins4", "both"):
            what = "%s packed/%s" % (tag, form)
            code = Guarded(n, np.uint8) if form != "bins4" else None
            bins4 = Guarded(nb, np.uint8) if form != "code" else None
            idx, off, counts, flag = Guarded(n, np.int32), Guarded(8, np.int64), Guarded(64, np.int64), new_flag()
            ctx.classify_compact_cigar_packed_dev(mode, *d_pk, m, code.t if code else None, idx.t, off.t, counts.t,
                                                  bins4=bins4.t if bins4 else None, range_flag=flag.t)
            torch.cuda.synchronize()
            check_flag(flag, bad, what)
            check_compact(want, n, code, bins4, idx, off, counts, what)
        # ... and with the six lists
        what = tag + " packed/place"
        lists = [Guarded(n, np.int32) for _ in range(6)]
        code, bins4, n_out, counts, flag = Guarded(n, np.uint8), Guarded(nb, np.uint8), Guarded(8, np.int64), Guarded(64, np.int64), new_flag()
        ctx.classify_place_cigar_packed_dev(mode, *d_pk, m, [l.t for l in lists], n_out.t, counts.t, code_out=code.t, bins4=bins4.t,
                                            range_flag=flag.t, capacity=n)
        torch.cuda.synchronize()
        check_flag(flag, bad, what)
        assert np.array_equal(code.host(what + " code"), want.code), what + " code"
        assert np.array_equal(_ffi.unpack_bins4(bins4.host(what + " bins4"), n), want.bins), what + " bins4"
        assert np.array_equal(counts.host(what + " counts").astype(np.uint64), want.counts), what + " counts"
        h_n = n_out.host(what + " n_out").astype(np.uint64)
        assert np.array_equal(h_n[:6], np.diff(want.off)[:6]) and int(h_n[7]) == int(want.off[7]), what + " n_out"
        for b in range(6):
            w = want.idx[int(want.off[b]):int(want.off[b + 1])]
            assert np.array_equal(lists[b].host("%s list %d" % (what, b))[:w.shape[0]].view(np.uint32), w), "%s list %d" % (what, b)
        # K1c: CSR columns
        what = tag + " csr/classify"
        code, flag = Guarded(n, np.uint8), new_flag()
        ctx.classify_cigar_dev(mode, *d_csr, m, code.t, range_flag=flag.t)
        torch.cuda.synchronize()
        check_flag(flag, bad, what)
        assert np.array_equal(code.host(what + " code"), want.code), what + " code"
        what = tag + " csr/compact"
        code, idx, off, counts, flag = Guarded(n, np.uint8), Guarded(n, np.int32), Guarded(8, np.int64), Guarded(64, np.int64), new_flag()
        ctx.classify_compact_cigar_dev(mode, *d_csr, m, code.t, idx.t, off.t, counts.t, range_flag=flag.t)
        torch.cuda.synchronize()
        check_flag(flag, bad, what)
        check_compact(want, n, code, None, idx, off, counts, what)

    # K3: the score column itself
    for s in (0, 1):
        what = "%s K3 species %d" % (case.name, s + 1)
        out, flag = Guarded(n, np.int32), new_flag()
        ctx.cigar_scores_dev(d_csr[4 * s], d_csr[4 * s + 1], d_csr[4 * s + 2], out.t, range_flag=flag.t)
        torch.cuda.synchronize()
        check_flag(flag, sp[s]["bad"], what)
        assert np.array_equal(out.host(what), sp[s]["score"]), what
    unchanged(d_csr, csr_host, case.name + " csr")
    unchanged(d_pk, pk_host, case.name + " packed")

    # the host-buffer calls, once: they raise exactly when a score left int32
    want = Want(1, sp, bits, ABSENT)
    csr = csr_host[:8]
    if bad:
        with pytest.raises(OverflowError):
            ctx.classify_cigar(1, *csr, bits, ABSENT)
        with pytest.raises(OverflowError):
            ctx.classify_compact_cigar(1, *csr, bits, ABSENT)
    else:
        code, counts = ctx.classify_cigar(1, *csr, bits, ABSENT)
        assert np.array_equal(code, want.code) and np.array_equal(counts, want.counts), case.name + " host classify_cigar"
        code, idx, off, counts = ctx.classify_compact_cigar(1, *csr, bits, ABSENT)
        assert np.array_equal(code, want.code) and np.array_equal(counts, want.counts), case.name + " host classify_compact_cigar"
        assert np.array_equal(off, want.off) and np.array_equal(idx, want.idx), case.name + " host classify_compact_cigar"
    for s in sp:
        if s["bad"]:
            with pytest.raises(OverflowError):
                ctx.cigar_scores(s["nm"], s["cig_off"], s["cig_oplen"])
        else:
            assert np.array_equal(ctx.cigar_scores(s["nm"], s["cig_off"], s["cig_oplen"]), s["score"]), case.name + " host cigar_scores"
    for a, b in zip(csr_host, [x for s in sp for x in (s["nm"], s["cig_off"], s["cig_oplen"], s["xs"])] + [bits]):
        assert np.array_equal(a, b), case.name + ": a host-buffer call wrote an input column"
