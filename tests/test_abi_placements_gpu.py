"""Every device-resident entry point of include/xenomapper_hip.h at every buffer placement the header allows, and every
refusal it promises -- through the C ABI (_ffi.Context's library handle), on buffers that are NOT the start of an allocation.

tests/abi_placements.py is the contract as a table; this module runs it.  For one call all buffers lie in ONE byte arena
filled with 0x5A, each at a chosen residue past a 256-byte boundary with guards between neighbours.  The arena is built on the
host (inputs in place), copied to the device, the call made on pointers into it, and the whole arena copied back and compared
byte for byte with the arena the oracle predicts: outputs hold the oracle's bytes (tests.helpers.c_classify / c_compact /
c_cigar_scores / c_mate_correlate -- never another GPU result), and every other byte -- guards, inputs, the unwritten ends of
index lists and runs, buffers passed as NULL -- is what it was.  A refused call must leave the whole arena as it was.

The input (abi_placements.N_RECORDS = 3 * 2048 + 77 records: three whole granules and a ragged one) and what it reaches are
described, and proved without a GPU, in tests/test_abi_placements_cpu.py.

No call here hands the device a pointer the contract forbids: the refusals are made by csrc/xm_api.hip before anything is
enqueued, which is exactly what these tests assert."""
import ctypes

import numpy as np
import pytest

from tests import abi_placements as A
from tests import helpers as H

pytestmark = pytest.mark.gpu

N = A.N_RECORDS
M_TAPS = 65
NEG = float("-inf")
MODES = (0, 1, 2)
NAN_AT = (5, 2047, 2048, 4100, N - 1)
LONG_RECORD = 2500


@pytest.fixture(scope="module")
def ctx():
    from xenomapper_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


# ---- the input and what the oracle makes of it, computed once ----------------------------------------------------------

def _bins_of(idx, off, n=N):
    bins = np.full(n, 7, dtype=np.uint8)
    for b in range(7):
        bins[idx[int(off[b]):int(off[b + 1])]] = b
    return bins


def _pack_nibbles(bins):
    padded = np.full(A.bins4_bytes(bins.shape[0]) * 2, 7, dtype=np.uint8)          # records past the end close no unit
    padded[:bins.shape[0]] = bins
    return (padded[0::2] | (padded[1::2] << 4)).astype(np.uint8)


def _runs_of(bins, n=N):
    """The segmented form as the header words it: per granule its units as record numbers counted from the granule's first
    record, sorted by bin, input order inside a bin; entries past the granule's units are not written (None here)."""
    runs, counts = [], np.zeros(A.runs_granules(n) * 8, dtype=np.uint16)
    for g in range(A.runs_granules(n)):
        b = bins[g * A.GRAN:(g + 1) * A.GRAN]
        order = np.concatenate([np.flatnonzero(b == k) for k in range(7)]).astype(np.uint16)
        runs.append(order)
        counts[8 * g:8 * g + 7] = [(b == k).sum() for k in range(7)]
    return runs, counts


class _Want(object):
    def __init__(self, mode, code, counts):
        self.code, self.counts = code, counts
        self.idx, self.off = H.c_compact(mode, code)
        self.bins = _bins_of(self.idx, self.off)
        self.bins4 = _pack_nibbles(self.bins)
        self.lengths = np.concatenate([np.diff(self.off.astype(np.int64))[:7], [int(self.off[7])]]).astype(np.uint64)
        self.runs, self.gran_counts = _runs_of(self.bins)

    def list(self, b):
        return self.idx[int(self.off[b]):int(self.off[b + 1])]


class _Data(object):
    def __init__(self):
        from xenomapper_amd import _ffi
        rng = np.random.default_rng(6)
        self.bits = {mode: A.pack_bits(A.unit_flags(mode)) for mode in MODES}
        self.i32 = A.score_columns(A.draw_states(np.random.default_rng(5)))
        self.f64 = A.as_doubles(self.i32, nan_at=NAN_AT)
        self.csr = [A.random_cigar(rng, long_record=LONG_RECORD), A.random_cigar(rng)]
        vals = np.concatenate([[A.ABSENT, A.ABSENT, 0], np.arange(-40, 1)]).astype(np.int64)
        self.xs = [vals[rng.integers(0, len(vals), N)].astype(np.int32) for _ in range(2)]
        self.packed = []
        for c in self.csr:
            cnt, tile, ops = _ffi.cigar_pack(c["cig_off"], c["cig_oplen"])             # xm_cigar_pack itself ...
            for got, want in zip((cnt, tile, ops), H.np_cigar_pack(c["cig_off"], c["cig_oplen"])):
                assert np.array_equal(got, want)                                       # ... held against the plain restatement
            self.packed.append({"cig_cnt": cnt, "cig_tile": tile, "cig_oplen": ops})
        assert self.packed[0]["cig_cnt"][LONG_RECORD] == 255
        self.scores = []
        for c in self.csr:
            a, bad = H.c_cigar_scores(c["nm"], c["cig_off"], c["cig_oplen"])
            assert bad == 0
            self.scores.append(a)
        self.want = {}
        for mode in MODES:
            self.want["i32", mode] = _Want(mode, *H.c_classify(mode, *self.i32, self.bits[mode], A.ABSENT))
            self.want["f64", mode] = _Want(mode, *H.c_classify(mode, *self.f64, self.bits[mode], NEG))
            self.want["cigar", mode] = _Want(mode, *H.c_classify(mode, self.scores[0], self.xs[0], self.scores[1], self.xs[1],
                                                                 self.bits[mode], A.ABSENT))
            assert int(self.want["f64", mode].lengths[6]) > 0                          # units holding state 6
        rng = np.random.default_rng(7)
        self.track = np.where(rng.random(N) < 0.1, 1.0, rng.random(N))
        self.density = rng.random(M_TAPS) / M_TAPS
        self.correlated = H.c_mate_correlate(self.track, self.density)
        x = self.i32[0] ^ self.i32[1] ^ self.i32[2] ^ self.i32[3]
        q = x[:N // 4 * 4].reshape(-1, 4)
        self.probed = (q[:, 0] ^ q[:, 1] ^ q[:, 2] ^ q[:, 3]).astype(np.uint32).astype(np.uint16)


@pytest.fixture(scope="module")
def data():
    return _Data()


def _family(row):
    name = row.name
    if name == "xm_compact_dev":
        return "i32"
    if "_f64_" in name:
        return "f64"
    if "cigar" in name and name != "xm_cigar_scores_dev":
        return "cigar"
    return "i32"


def _inputs(row, mode, D):
    """Buffer name -> the array the call reads there."""
    name = row.name
    if name == "xm_cigar_scores_dev":
        return dict(D.csr[0])
    if name == "xm_mate_correlate_dev":
        return {"track": D.track, "density": D.density}
    if name == "xm_stream_probe_dev":
        return dict(zip(("c0", "c1", "c2", "c3"), D.i32))
    if name == "xm_compact_dev":
        return {"code": D.want["i32", mode].code}
    out = {"unit_bits": D.bits[mode]}
    if _family(row) == "cigar":
        for s in (0, 1):
            cols = dict(D.csr[s], **(D.packed[s] if "packed" in name else {}))
            cols["xs"] = D.xs[s]
            out.update({k + str(s + 1): v for k, v in cols.items() if any(p.name == k + str(s + 1) for p in A.pointers(row))})
    else:
        out.update(zip(("as1", "xs1", "as2", "xs2"), D.f64 if _family(row) == "f64" else D.i32))
    return out


def _outputs(row, mode, form, cap, D):
    """Buffer name -> what the call must leave at the START of that buffer (the rest of the buffer stays as it was); a list of
    (element offset, array) pairs where the written places are not one stretch (runs16)."""
    name = row.name
    if name == "xm_cigar_scores_dev":
        return {"as_out": D.scores[0], "range_flag": np.zeros(1, np.uint32)}
    if name == "xm_mate_correlate_dev":
        return {"out": D.correlated}
    if name == "xm_stream_probe_dev":
        return {"out": D.probed.view(np.uint8)}
    w = D.want[_family(row), mode]
    out = {}
    names = {p.name for p in A.pointers(row)}
    if "code_out" in names and form != "bins4":
        out["code_out"] = w.code
    if "bins4" in names and form != "code":
        out["bins4"] = w.bins4
    if "range_flag" in names:
        out["range_flag"] = np.zeros(1, np.uint32)                                     # no score of this input leaves int32
    if "counts" in names:
        out["counts"] = w.counts
    if "bin_offsets" in names:
        out["bin_offsets"], out["idx_out"] = w.off, w.idx
    if "n_out" in names:
        out["n_out"] = w.lengths
    if "place" in name:
        for b in range(6):
            out["idx_out[%d]" % b] = w.list(b)[:cap]
        if "idx_state6" in names:
            out["idx_state6"] = w.list(6)[:cap]
    if "runs16" in names:
        out["runs16"] = [(g * A.GRAN, r) for g, r in enumerate(w.runs)]
        out["gran_counts"] = w.gran_counts
    return out


class _Call(object):
    """One call of `row` laid out in an arena: host image before, host image the oracle predicts, the device copy."""

    def __init__(self, row, mode, D, residue=None, form="both", cap=N, null=()):
        import torch
        self.row, self.mode, self.cap, self.null = row, mode, cap, set(null)
        if form == "code":
            self.null.add("bins4")
        if form == "bins4":
            self.null.add("code_out")
        ins = _inputs(row, mode, D)
        env = {"n": N, "m": M_TAPS, "cap": cap}
        for k, v in ins.items():
            if k.startswith("cig_oplen"):
                env["ops" + k[len("cig_oplen"):]] = v.shape[0]
        sizes = {name: A.extent(p, **env) for name, p in A.buffers(row)}
        for k, v in ins.items():
            assert np.ascontiguousarray(v).nbytes == sizes[k], (row.name, k)           # the table's extents are the arrays' sizes
        self.at, self.total = A.lay_out(row, sizes, residue)
        self.before = A.new_arena(self.total)
        for name, p in A.buffers(row):
            if p.role == "in":
                A.view(self.before, self.at, name, p.ctype)[...] = ins[name]
            elif p.role == "inout":
                A.view(self.before, self.at, name, p.ctype)[...] = 0
        self.want = self.before.copy()
        for name, value in _outputs(row, mode, form, cap, D).items():
            if name in self.null:
                continue
            ctype = dict(A.buffers(row))[name].ctype
            dst = A.view(self.want, self.at, name, ctype)
            for at, piece in (value if isinstance(value, list) else [(0, value)]):
                piece = np.ascontiguousarray(piece).view(A.NP_TYPE[ctype])
                assert at + piece.shape[0] <= dst.shape[0], (row.name, name)           # no more than the documented extent
                dst[at:at + piece.shape[0]] = piece
        self.raw = torch.empty(self.total + 256, dtype=torch.uint8, device="cuda")
        self.dev = A.aligned_arena(self.raw, self.total)
        self.upload()

    def upload(self):
        import torch
        self.dev.copy_(torch.from_numpy(self.before))
        torch.cuda.synchronize()

    def pointer(self, name):
        return None if name in self.null else self.dev.data_ptr() + self.at[name][0]

    def args(self, **scalars):
        """The C arguments behind (ctx, stream).  scalars: overrides by parameter name (mode, n_records ...)."""
        values = {"mode": self.mode, "n_records": N, "n": N, "m": M_TAPS, "min_score_floor": A.ABSENT, "min_score": NEG,
                  "list_capacity": self.cap}
        values.update(scalars)
        out = []
        self.keep = []
        for p in self.row.params:
            if isinstance(p, A.Scalar):
                out.append(values[p.name])
            elif p.count == 1:
                out.append(self.pointer(p.name))
            elif p.name in self.null:
                out.append(None)
            else:
                six = (ctypes.c_void_p * p.count)(*[self.pointer("%s[%d]" % (p.name, b)) for b in range(p.count)])
                self.keep.append(six)
                out.append(six)
        return out

    def run(self, ctx, **scalars):
        import torch
        rc = getattr(ctx._L, self.row.name)(ctx._h, None, *self.args(**scalars))
        torch.cuda.synchronize()
        return rc

    def owner(self, byte):
        for name, (off, nbytes) in self.at.items():
            if off <= byte < off + nbytes:
                return "%s + %d" % (name, byte - off)
            if off - A.GUARD <= byte < off:
                return "guard in front of %s, %d bytes before it" % (name, off - byte)
            if off + nbytes <= byte < off + nbytes + A.GUARD:
                return "guard behind %s, %d bytes past it" % (name, byte - off - nbytes)
        return "padding"

    def check(self, want, what):
        got = self.dev.cpu().numpy()
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            residues = {k: off % 256 for k, (off, _) in self.at.items()}
            pytest.fail("%s %r: %d bytes differ from the oracle's arena, first at %s (got 0x%02X, want 0x%02X); residues %r" % (
                self.row.name, what, bad.shape[0], self.owner(int(bad[0])), got[bad[0]], want[bad[0]], residues))


def _forms(row):
    return ("both", "code", "bins4") if row.one_of else ("both",)


def _ok(ctx, call, what):
    rc = call.run(ctx)
    assert rc == 0, (call.row.name, what, rc)
    call.check(call.want, what)
    assert ctx.workspace_is_clean(), (call.row.name, what)


def _modes(row):
    return MODES if any(p.name == "mode" for p in row.params) else (0,)


# ---- a. allowed placements give the oracle's bytes and touch nothing else -----------------------------------------------

@pytest.mark.parametrize("row", A.ROWS, ids=lambda r: r.name)
def test_allowed_placements(ctx, data, row):
    bufs = A.buffers(row)
    for mode in _modes(row):
        for form in _forms(row):
            _ok(ctx, _Call(row, mode, data, {}, form), (mode, form, "all at 0"))                               # (i)
            smallest = {name: A.smallest_nonzero(p.align) for name, p in bufs}
            _ok(ctx, _Call(row, mode, data, smallest, form), (mode, form, "all at the smallest residue"))      # (ii)
    # (iii) one parameter at a time through all its residues, the others at 0; the mode and the output form go round with
    # the calls, so every mode and form meets placements of this kind
    k = 0
    for name, p in bufs:
        for r in A.residues(p.align)[1:]:
            mode, form = _modes(row)[k % len(_modes(row))], _forms(row)[(k // 3) % len(_forms(row))]
            if form == "code" and name == "bins4" or form == "bins4" and name == "code_out":
                form = "both"
            _ok(ctx, _Call(row, mode, data, {name: r}, form), (mode, form, name, r))
            k += 1


@pytest.mark.parametrize("name", ["xm_classify_place_dev", "xm_classify_place_f64_dev", "xm_classify_place_cigar_packed_dev"])
def test_six_lists_at_six_different_residues(ctx, data, name):
    row = A.ROW[name]
    lists = [k for k, p in A.buffers(row) if p.name in ("idx_out", "idx_state6")]
    spread = [4, 8, 12, 0, 252, 16, 20][:len(lists)]                      # 4, 8 and 12 past a 16-byte boundary among them
    assert len(set(spread[:6])) == 6
    for mode in MODES:
        for turn in range(2 if mode else len(lists)):                     # single-end (the staged 16-byte stores): every list at every residue
            residue = {k: spread[(j + turn) % len(lists)] for j, k in enumerate(lists)}
            for form in ("bins4", "code"):                                # the scatter from nibbles and from category bytes
                _ok(ctx, _Call(row, mode, data, residue, form), (mode, form, "lists", turn))
    # lists shorter than their bins: truncated at list_capacity, the lengths reported in full, nothing behind the capacity
    call = _Call(row, 0, data, {k: 12 for k in lists}, "both", cap=100)
    assert max(int(v) for v in data.want[_family(row), 0].lengths[:6]) > 100
    _ok(ctx, call, "capacity 100")


# ---- b. every promised refusal ------------------------------------------------------------------------------------------

def _refused(ctx, call, what, **scalars):
    rc = call.run(ctx, **scalars)
    assert rc == -1, (call.row.name, what, rc)                            # XM_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        ctx._check(rc, call.row.name)
    call.check(call.before, what)                                         # nothing enqueued: the whole arena as it was
    assert ctx.workspace_is_clean(), (call.row.name, what)


@pytest.mark.parametrize("row", A.ROWS, ids=lambda r: r.name)
def test_refusals(ctx, data, row):
    mode = _modes(row)[-1]
    made = []
    for name, p in A.buffers(row):
        if not p.nullable and p.count == 1:
            _refused(ctx, _Call(row, mode, data, null=[name]), (name, "NULL"))
            made.append((p.name, "NULL"))
        elif not p.nullable:                                              # the six lists: no array at all (once), one pointer of it NULL
            if name.endswith("[0]"):
                _refused(ctx, _Call(row, mode, data, null=[p.name]), (p.name, "NULL"))
                made.append((p.name, "NULL"))
            call = _Call(row, mode, data)
            call.pointer = lambda k, skip=name, inner=call.pointer: None if k == skip else inner(k)
            _refused(ctx, call, (name, "NULL in the array"))
        for step in A.refused_steps(p):                                   # half the alignment, and one element where that differs
            _refused(ctx, _Call(row, mode, data, {name: step}), (name, "off by %d" % step))
            made.append((p.name, "off"))
    if row.one_of:
        _refused(ctx, _Call(row, mode, data, null=row.one_of), "neither code_out nor bins4")
    call = _Call(row, mode, data)
    if any(p.name == "mode" for p in row.params):
        _refused(ctx, call, "mode 3", mode=3)
        _refused(ctx, call, "mode -1", mode=-1)
    size = "n" if row.name == "xm_mate_correlate_dev" else "n_records"
    _refused(ctx, call, "too many records", **{size: (1 << 40) + 1 if size == "n" else A.MAX_RECORDS + 1})
    # every pointer parameter was refused misplaced, every one that must be given was refused NULL
    assert {k for k, how in made if how == "off"} == {p.name for p in A.pointers(row)}
    assert {k for k, how in made if how == "NULL"} == {p.name for p in A.pointers(row) if not p.nullable}
    # and the context is as good as before
    _ok(ctx, call, "the next correct call")


def test_the_refusals_this_contract_added_are_made(ctx, data):
    """By name, the checks csrc/xm_api.hip did not make before the placement contract was written down: taking any one of
    them out again fails here (and in test_refusals)."""
    def off(row, name, by):
        call = _Call(A.ROW[row], 0, data)
        call.pointer = lambda k, inner=call.pointer: inner(k) + by if k == name else inner(k)
        _refused(ctx, call, (name, by))

    for row in A.ROWS:
        names = {p.name for p in A.pointers(row)}
        if "unit_bits" in names:
            off(row.name, "unit_bits", 4)
        for k in ("bin_offsets", "n_out", "counts"):
            if k in names:
                off(row.name, k, 4)
        if "range_flag" in names:
            off(row.name, "range_flag", 2)
        if "idx_out" in names and "place" not in row.name:
            off(row.name, "idx_out", 2)
    for k in ("nm", "cig_off", "cig_oplen", "as_out"):
        off("xm_cigar_scores_dev", k, 2)
    for k in ("cig_oplen1", "cig_oplen2"):
        off("xm_classify_cigar_dev", k, 2)
        off("xm_classify_compact_cigar_dev", k, 2)
    for k in ("track", "density", "out"):
        off("xm_mate_correlate_dev", k, 4)


@pytest.mark.parametrize("row", A.ROWS, ids=lambda r: r.name)
def test_no_records_with_null_columns(ctx, data, row):
    """n_records == 0: XM_OK with every column NULL; the calls that count zero their two 64-bit outputs and touch nothing else."""
    totals = [p.name for p in A.pointers(row) if p.name in ("bin_offsets", "n_out", "counts")]
    keep = set(totals) | {k for k, p in A.buffers(row) if p.count > 1}    # the six list pointers are looked at whatever n is
    call = _Call(row, _modes(row)[0], data, {k: 8 for k in totals}, null=[k for k, _ in A.buffers(row) if k not in keep])
    size = "n" if row.name == "xm_mate_correlate_dev" else "n_records"
    rc = call.run(ctx, **{size: 0})
    assert rc == 0, row.name
    want = call.before.copy()
    for k in totals:
        A.view(want, call.at, k, "uint64_t")[...] = 0
    call.check(want, "n = 0")
    assert ctx.workspace_is_clean()
    for k in totals:                                                      # ... but not at a misplaced one
        bad = _Call(row, _modes(row)[0], data, null=[q for q, _ in A.buffers(row) if q not in keep])
        bad.pointer = lambda q, skip=k, inner=bad.pointer: inner(q) + 4 if q == skip else inner(q)
        _refused(ctx, bad, (k, "off by 4 with n = 0"), **{size: 0})


# ---- c. the host-buffer entry points take NumPy slices ------------------------------------------------------------------

def _slid(a):
    """The same values in a view that begins one element into its allocation: element-aligned, nothing more."""
    big = np.empty(a.shape[0] + 1, dtype=a.dtype)
    big[1:] = a
    view = big[1:]
    assert view.ctypes.data - big.ctypes.data == a.itemsize and big.ctypes.data % 16 == 0 and view.flags.c_contiguous
    return big, view


@pytest.mark.parametrize("locked", [False, True], ids=["pageable", "registered"])
def test_host_entry_points_on_element_aligned_slices(ctx, data, locked):
    import contextlib
    for mode in MODES:
        w, wf = data.want["i32", mode], data.want["f64", mode]
        parts = [_slid(c) for c in data.i32] + [_slid(c) for c in data.f64] + [_slid(data.bits[mode]), _slid(w.code)]
        views = [v for _, v in parts]
        cols, fcols, bits, code_in = views[0:4], views[4:8], views[8], views[9]
        with (ctx.registered(*[big for big, _ in parts]) if locked else contextlib.nullcontext()):
            code, counts = ctx.classify(mode, *cols, bits, A.ABSENT)
            assert np.array_equal(code, w.code) and np.array_equal(counts, w.counts)
            code, counts = ctx.classify_f64(mode, *fcols, bits, NEG)
            assert np.array_equal(code, wf.code) and np.array_equal(counts, wf.counts)
            idx, off, counts = ctx.compact(mode, code_in)
            assert np.array_equal(idx, w.idx) and np.array_equal(off, w.off) and np.array_equal(counts, w.counts)
            code, idx, off, counts = ctx.classify_compact(mode, *cols, bits, A.ABSENT)
            assert np.array_equal(code, w.code) and np.array_equal(idx, w.idx) and np.array_equal(off, w.off)
            assert np.array_equal(counts, w.counts)
            code, lists, n_out, counts = ctx.classify_place(mode, *cols, bits, A.ABSENT)
            assert np.array_equal(code, w.code) and np.array_equal(counts, w.counts)
            for b in range(6):
                assert np.array_equal(lists[b], w.list(b)), (mode, b)
            assert [int(v) for v in n_out[:8]] == [int(v) for v in w.lengths]
        assert ctx.workspace_is_clean()
    # the segmented form's host half on slices, too (no device): xm_runs_expand
    from xenomapper_amd import _ffi
    w = data.want["i32", 0]
    runs16 = np.zeros(A.runs16_entries(N), dtype=np.uint16)
    for at, r in [(g * A.GRAN, r) for g, r in enumerate(w.runs)]:
        runs16[at:at + r.shape[0]] = r
    (_, r16), (_, gc) = _slid(runs16), _slid(w.gran_counts)
    for b in range(7):
        assert np.array_equal(_ffi.runs_expand(N, r16, gc, b), w.list(b)), b
