"""tests/abi_placements.py against include/xenomapper_hip.h, and the arena helper against itself -- no GPU.

The table is the placement contract the GPU test runs; here it is shown to be complete (every *_dev prototype of the header
has a row, with every parameter in the C order and every pointer with the element size of its C type), the arena to be sound
(no overlap, the residue asked for, guards all round, NumPy and torch alike), and the one input of the GPU test to reach what
it is drawn for: every branch of the staged copy-out in single-end mode, the three lane layouts of the scatter in the paired
modes, units holding state 6 and a record of more than 255 CIGAR operations."""
import os
import re

import numpy as np
import pytest

from tests import abi_placements as A
from tests import helpers as H

HEADER = os.path.join(H.REPO, "include", "xenomapper_hip.h")
HANDLES = {("xm_ctx", "ctx"), ("void", "stream")}          # pointers that are no buffers: the context and the hipStream_t


def prototypes():
    """name -> [(C type, is pointer, array length or 0, name)] for every `int xm_...(...);` of the header."""
    with open(HEADER) as fh:
        text = re.sub(r"/\*.*?\*/", " ", fh.read(), flags=re.S)
    out = {}
    for name, args in re.findall(r"^int\s+(xm_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.M | re.S):
        params = []
        for arg in (a.strip() for a in args.split(",")):
            if arg == "void":
                continue
            m = re.fullmatch(r"(?:const\s+)?(\w+)\s*(\**)\s*(?:const\s+)?(\w+)\s*(?:\[(\w+)\])?", " ".join(arg.split()))
            assert m, (name, arg)
            array = int(m.group(4)) if m.group(2) and m.group(4) else 0     # `T *const x[6]`: six pointers; `T x[8]` is a pointer
            params.append((m.group(1), bool(m.group(2)) or bool(m.group(4)), array, m.group(3)))
        out[name] = params
    return out


def test_every_device_entry_point_has_its_row_parameter_by_parameter():
    protos = prototypes()
    dev = [k for k in protos if k.endswith("_dev")]
    assert len(dev) == 16 and set(dev) == set(A.ROW), set(dev) ^ set(A.ROW)
    assert [r.name for r in A.ROWS] == sorted(A.ROW, key=[r.name for r in A.ROWS].index) and len(A.ROWS) == len(A.ROW)
    for name in dev:
        want = [p for p in protos[name] if (p[0], p[3]) not in HANDLES]
        assert [(p[0], p[3]) for p in protos[name][:2]] == [("xm_ctx", "ctx"), ("void", "stream")], name
        row = A.ROW[name]
        assert [p.name for p in row.params] == [p[3] for p in want], name
        for have, (ctype, is_ptr, array, pname) in zip(row.params, want):
            assert have.ctype == ctype, (name, pname)
            assert isinstance(have, A.Ptr) == is_ptr, (name, pname)
            if is_ptr:
                assert have.count == (array or 1), (name, pname)
                assert A.SIZEOF[have.ctype] == np.dtype(A.NP_TYPE[ctype]).itemsize
                assert have.align % A.SIZEOF[ctype] == 0 and have.align in (2, 4, 8, 16, 32), (name, pname)
                assert have.role in ("in", "out", "inout")
                assert A.extent(have, n=A.N_RECORDS, m=65, cap=A.N_RECORDS, ops=9, ops1=9, ops2=9) > 0
        for k in row.one_of:
            assert A.Ptr in map(type, [p for p in row.params if p.name == k]) and [p for p in row.params if p.name == k][0].nullable


def test_one_rule_per_kind_of_parameter():
    """The header states ONE alignment per kind of parameter; so does the table, row by row."""
    for row in A.ROWS:
        f64 = "_f64_" in row.name
        for p in A.pointers(row):
            where = (row.name, p.name)
            if p.name in ("unit_bits", "bin_offsets", "n_out", "counts"):
                assert (p.ctype, p.align, p.nullable) == ("uint64_t", 8, False), where
            elif p.name in ("as1", "xs1", "as2", "xs2") and f64:
                assert (p.ctype, p.align) == ("double", 32), where
            elif p.name in ("idx_out", "idx_state6", "range_flag"):
                assert (p.ctype, p.align) == ("uint32_t", 4), where
            elif p.name in ("bins4", "runs16", "gran_counts", "code"):
                assert p.align == 16, where
            elif p.name == "code_out":
                assert p.align == (16 if "compact" in row.name or "place" in row.name else 4), where
            elif row.name in ("xm_cigar_scores_dev", "xm_mate_correlate_dev") or p.name[:7] in ("cig_opl", "cig_cnt", "cig_til"):
                assert p.align == max(4, A.SIZEOF[p.ctype]), where        # a dword, or an element, at a time
            elif row.name == "xm_stream_probe_dev" and p.name == "out":
                assert p.align == 2, where
            else:
                assert (A.SIZEOF[p.ctype], p.align) == (4, 16), where      # 32-bit columns read four records a lane
            assert (p.role == "in") == (p.name not in ("code_out", "bins4", "idx_out", "idx_state6", "bin_offsets", "n_out", "counts",
                                                        "runs16", "gran_counts", "as_out", "out", "range_flag")), where


def test_the_header_says_what_the_table_says():
    with open(HEADER) as fh:
        text = " ".join(fh.read().split())
    assert "Column base pointers must be 16-byte aligned" not in text               # the paragraph this contract replaced
    for phrase in ("unit_bits (32-byte scalar loads of 64-bit words) 8 bytes", "bin_offsets, n_out, counts 8 bytes",
                   "as1 xs1 as2 xs2 of every *_f64_dev call 32 bytes", "idx_out, the six idx_out[b], idx_state6 4 bytes",
                   "bins4, runs16, gran_counts 16 bytes", "track, density, out 8 bytes", "tests/abi_placements.py"):
        assert phrase in text, phrase


def test_host_buffer_entry_points_are_named_with_their_element_types():
    protos = prototypes()
    assert set(A.HOST) == {"xm_classify", "xm_classify_f64", "xm_compact", "xm_classify_compact", "xm_classify_place", "xm_runs_expand"}
    for name, table in A.HOST.items():
        want = {p[3]: p[0] for p in protos[name] if p[1] and (p[0], p[3]) not in HANDLES}
        assert table == want, name


def test_residues_offered():
    assert A.residues(32) == [0, 32, 224] and A.residues(16) == [0, 16, 240]
    assert A.residues(8) == [0, 8, 248] and A.residues(4) == [0, 4, 8, 12, 252]
    assert A.residues(2) == [0, 2, 4, 6, 8, 10, 12, 14, 254]
    for a in (2, 4, 8, 16, 32):
        assert all(r % a == 0 and r < 256 for r in A.residues(a)) and A.smallest_nonzero(a) == a
    off = {(p.name, p.ctype, tuple(A.refused_steps(p))) for row in A.ROWS for p in A.pointers(row)}
    assert {("as1", "int32_t", (4, 8)), ("as1", "double", (8, 16)), ("unit_bits", "uint64_t", (4,)), ("idx_out", "uint32_t", (2,)),
            ("counts", "uint64_t", (4,)), ("code_out", "uint8_t", (1, 2)), ("code_out", "uint8_t", (1, 8)), ("bins4", "uint8_t", (1, 8)),
            ("cig_cnt1", "uint8_t", (1, 2)), ("cig_oplen1", "uint32_t", (2,)), ("runs16", "uint16_t", (2, 8)), ("out", "uint8_t", (1,)),
            ("track", "double", (4,)), ("range_flag", "uint32_t", (2,))} <= off
    for row in A.ROWS:
        for p in A.pointers(row):
            assert all(0 < s < p.align and s % p.align != 0 for s in A.refused_steps(p)) and p.align // 2 in A.refused_steps(p)


def _sizes(row, n=A.N_RECORDS):
    return {name: A.extent(p, n=n, m=65, cap=n, ops=1234, ops1=1234, ops2=777) for name, p in A.buffers(row)}


@pytest.mark.parametrize("row", A.ROWS, ids=lambda r: r.name)
def test_arena_is_sound(row):
    sizes = _sizes(row)
    names = [name for name, _ in A.buffers(row)]
    plans = [{}, {name: A.smallest_nonzero(p.align) for name, p in A.buffers(row)},
             {name: A.residues(p.align)[(k + 1) % len(A.residues(p.align))] for k, (name, p) in enumerate(A.buffers(row))}]
    plans += [{name: s} for name, p in A.buffers(row) for s in A.refused_steps(p)]                # what the refusal tests ask for
    for residue in plans:
        at, total = A.lay_out(row, sizes, residue)
        assert list(at) == names and total % 256 == 0
        own = A.owned(at, total)                                          # asserts that no two buffers overlap
        for name, p in A.buffers(row):
            off, nbytes = at[name]
            assert nbytes == sizes[name] and off % 256 == residue.get(name, 0)
            assert not own[off - A.GUARD:off].any() and not own[off + nbytes:off + nbytes + A.GUARD].any(), name
            assert off >= A.GUARD and off + nbytes + A.GUARD <= total
        arena = A.new_arena(total)
        assert arena.ctypes.data % 256 == 0 and (arena == A.FILL).all()
        for name, p in A.buffers(row):
            v = A.view(arena, at, name, p.ctype)
            assert v.dtype == A.NP_TYPE[p.ctype] and v.nbytes == sizes[name]
            assert v.ctypes.data % 256 == residue.get(name, 0) and v.ctypes.data - arena.ctypes.data == at[name][0]
            v[...] = 0                                                    # writing through the view reaches the arena, nothing else
        assert (arena[own] == 0).all() and (arena[~own] == A.FILL).all()


def test_arena_on_a_torch_tensor_is_the_same_arena():
    import torch
    row = A.ROW["xm_classify_place_f64_dev"]
    sizes = _sizes(row, 300)
    residue = {name: A.residues(p.align)[-1] for name, p in A.buffers(row)}
    at, total = A.lay_out(row, sizes, residue)
    arena = A.aligned_arena(torch.full((total + 256,), A.FILL, dtype=torch.uint8), total)
    assert arena.data_ptr() % 256 == 0
    for name, p in A.buffers(row):
        v = A.view(arena, at, name, p.ctype)
        assert v.element_size() == A.SIZEOF[p.ctype] and v.numel() * v.element_size() == sizes[name]
        assert v.data_ptr() % 256 == residue[name] and v.data_ptr() - arena.data_ptr() == at[name][0]
        v.zero_()
    own = A.owned(at, total)
    host = arena.numpy()
    assert (host[own] == 0).all() and (host[~own] == A.FILL).all()


# ---- the input of the GPU test reaches what it is drawn for -----------------------------------------------------------

def test_single_end_input_runs_every_branch_of_the_staged_copy_out():
    n = A.N_RECORDS
    assert n == 3 * 2048 + 77
    states = A.draw_states(np.random.default_rng(5))
    cols = A.score_columns(states)
    code, _ = H.c_classify(0, *cols, A.pack_bits(A.unit_flags(0)), A.ABSENT)
    assert np.array_equal(code, states.astype(np.uint8))                  # single-end: the category byte is the state, the bin
    _, off = H.c_compact(0, code)
    for g in range(3):
        cnt = np.bincount(code[g * 2048:(g + 1) * 2048], minlength=7)
        assert cnt.sum() == 2048 >= A.STAGE_MIN_UNITS
        assert (cnt >= 64).sum() >= 2 and ((cnt > 0) & (cnt < 64)).sum() >= 1, cnt
    runs = A.staged_runs(code, off)
    long_runs = [(g4, k) for g4, k in runs if k >= 64]
    assert any(k < 64 for _, k in runs)                                   # the short run: dword stores only
    assert any(g4 != 0 for g4, _ in long_runs)                            # a head: the run begins off a 16-byte group
    assert any((k - ((-g4) & 3)) % 4 != 0 for g4, k in long_runs)         # a tail behind the last whole group
    assert any((k - ((-g4) & 3)) // 4 > 64 for g4, k in long_runs)        # a body of more than one pass of the wave
    assert 0 < 77 < A.STAGE_MIN_UNITS                                     # the ragged granule goes straight to idx_out


def test_paired_input_has_the_three_lane_layouts_and_a_unit_at_a_workgroup_front():
    f = A.unit_flags(1)
    assert np.array_equal(f, A.unit_flags(2)) and f.shape[0] == A.N_RECORDS
    per_lane = f.reshape(-1)[:3 * 2048].reshape(-1, 4)
    g0, g1, g2 = per_lane[:512], per_lane[512:1024], per_lane[1024:]
    assert (g0[1:, (0, 2)] == 0).all() and (g0[:, (1, 3)] == 1).all()     # strictly interleaved: positions 1 and 3 only
    assert (g1.sum(axis=1) > 2).any()                                     # three units of one lane: the general form
    assert (g2.sum(axis=1) <= 2).all() and g2[:, (0, 2)].any()            # parity flipped, two units a lane at most
    assert f[0] == 1                                                      # set, and to be dropped: record 0 has no predecessor
    assert f[2048] == 1 or f[4096] == 1                                   # a workgroup whose first record closes a unit: the halo fetch
    code, _ = H.c_classify(1, *A.score_columns(A.draw_states(np.random.default_rng(5))), A.pack_bits(f), A.ABSENT)
    assert code[0] == 0xFF


def test_binary64_and_cigar_inputs():
    cols = A.as_doubles(A.score_columns(A.draw_states(np.random.default_rng(5))), nan_at=(5, 2047, 2048, 4100, A.N_RECORDS - 1))
    code, counts = H.c_classify(0, *cols, A.pack_bits(A.unit_flags(0)), float("-inf"))
    assert (code == 6).sum() == 5 and counts[6] == 5
    c = A.random_cigar(np.random.default_rng(6), long_record=2500)
    cnt, tile, ops = H.np_cigar_pack(c["cig_off"], c["cig_oplen"])
    assert cnt[2500] == 255 and ops.shape[0] == c["cig_oplen"].shape[0] + 1 and tile.shape[0] == A.cig_tiles(A.N_RECORDS) + 1
    assert H.c_cigar_scores(c["nm"], c["cig_off"], c["cig_oplen"])[1] == 0
