"""Every launcher of xm_kernels.hip that tests/test_lockstep_place_cpu.py does not run, executed on the CPU, lane by lane, under
ASan + UBSan: K1r (classify_runs_kernel, runs_finish_kernel), K3 (cigar_kernel), K1c (classify_cigar_kernel), K1p
(classify_cigp_kernel, then scan_kernel and scatter_kernel as in the fused step), the plain classify_kernel,
mate_correlate_kernel and stream_probe_kernel.  xm_kernels.hip is compiled for the host through the lockstep shim
(tests/lockstep) by tests/lockstep_kernels_host.cpp with ROCm's host clang++.  This file writes the cases from the catalogues
the GPU tests use (runs_shapes, cigar_shapes, correlate_shapes), that program runs each twice (outputs and workspace filled
with 0xA5 and the LDS with 0x00, then the other way round) in heap blocks of exactly the sizes include/xenomapper_hip.h promises, placed no better than its
table of placements asks for, and what it dumps is compared here with the oracle the GPU test of the same kernel uses, exactly.

Why: the GPU tests hand the kernels torch tensors, which are rounded up to 512 bytes inside 2 MB segments, so a kernel that
reads up to 7 words over a stretch on purpose (K1p), gathers 12 bytes per record into the next record's ops (K1c) or copies an
LDS slab out 16 bytes a thread (K1r) may read or write a little past a buffer, or read stale LDS, and pass them all.  Here the
first byte past a buffer is ASan's, and a result that depends on what LDS or the outputs held before shows as a difference
between the two runs.  A run that ends with a sanitizer report, with a `lockstep:` message (divergence: lanes of a wave at
different cross-lane operations outside a declared XM_IF_LANES; watchdog) or with another status fails its test.

Time: 400 s for the file on eight cores, 71 s of it the one build of the program (once per pytest session).  What was cut: K1c
and K1p run both min_score floors of tests/test_cigar_shapes_gpu.py in mode 1 and one each in modes 0 and 2 (with both floors in
every mode the file took 684 s).  Nothing of correlate_shapes is cut: its slowest tap count, 6145, takes 7 s.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import cigar_shapes as C
from tests import correlate_shapes as K
from tests import helpers as H
from tests import lockstep_build as L
from tests import runs_shapes as S

ABSENT = -2**31
GRAN = 2048
CMD_RUNS, CMD_CIGAR, CMD_K1C, CMD_K1P, CMD_CLASSIFY, CMD_CORRELATE, CMD_PROBE = range(1, 8)
AGREE, CLEAN, UNTOUCHED = 1, 2, 4
FORM_BINS4, FORM_CODE = 0, 1
# min_score floors per mode: the two of tests/test_cigar_shapes_gpu.py, both in mode 1 and one each in modes 0 and 2 (the floor
# enters the state function only, which the plain classify and K1r cases run at both kinds of floor as well)
FLOORS = {0: (ABSENT,), 1: (ABSENT, -41), 2: (-41,)}
SMALL = (1, 2047, 2048, 2049)
CLASSIFY_SIZES = (1, 3, 4, 5, 2047, 2048, 2049)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return L.host_program(tmp_path_factory, "lockstep_kernels_host")


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def case(cmd, *params, arrays=()):
    par = [cmd] + [int(p) for p in params]
    return par + [0] * (8 - len(par)), list(arrays)


def run_host(exe, tmp_path, tag, cases, dumps):
    """cases: what case() gives; dumps: the dtypes of one case's dumped arrays behind its flags -> per case (flags, arrays)."""
    path_in, path_out = str(tmp_path / (tag + ".cases")), str(tmp_path / (tag + ".out"))
    with open(path_in, "wb") as fh:
        for par, arrays in cases:
            fh.write(struct.pack("<Q", 8 * len(par)) + struct.pack("<%dQ" % len(par), *par))
            for a in arrays:
                b = np.ascontiguousarray(a).tobytes()
                fh.write(struct.pack("<Q", len(b)) + b)
    proc = subprocess.run([exe, path_in, path_out], capture_output=True, text=True, env=L.ENV, timeout=1200)
    assert "lockstep:" not in proc.stderr, (tag, proc.stderr[-3000:])           # divergence, watchdog
    assert "AddressSanitizer" not in proc.stderr and "runtime error" not in proc.stderr, (tag, proc.stderr[-4000:])
    assert proc.returncode == 0, (tag, (proc.stdout + proc.stderr)[-3000:])
    blob = open(path_out, "rb").read()
    os.remove(path_in)
    os.remove(path_out)
    at, res = 0, []

    def take(dtype):
        nonlocal at
        k, = struct.unpack_from("<Q", blob, at)
        a = np.frombuffer(blob, dtype=dtype, count=k // np.dtype(dtype).itemsize, offset=at + 8)
        at += 8 + k
        return a

    for _ in cases:
        flags = int(take(np.uint32)[0])
        res.append((flags, [take(d) for d in dumps]))
    assert at == len(blob)
    return res


def check_flags(flags, what, fill_independent=True):
    assert flags & AGREE or not fill_independent, ("the two runs differ", what)
    assert flags & CLEAN, ("part_tot or the count replicas are not all zero afterwards", what)
    assert flags & UNTOUCHED, ("written outside what the call writes", what)


# ---- K1r ---------------------------------------------------------------------------------------------------------------

RUNS_DUMPS = (np.uint16, np.uint16, np.uint16, np.uint64, np.uint64)


def runs_case(mode, cols, bits, m):
    n = cols[0].shape[0]
    return case(CMD_RUNS, cols[0].dtype == np.float64, mode, n, f64_bits(m), arrays=list(cols) + [np.asarray(bits, dtype=np.uint64)[:(n + 63) // 64]])


def check_runs(what, n, mode, cols, bits, m, got):
    """The layout against S.segment of the oracle's lists, entry by entry: behind a granule's units the first run holds 0xA5A5
    and the second 0x0000, so a stray store of either value shows in the other run, and a stale LDS entry (the other pattern
    than the memory's in either run) in both."""
    flags, (runs_a5, runs_00, gran_counts, n_out, counts) = got
    check_flags(flags, what)
    want_code, want_counts = H.c_classify(mode, *cols, bits, m)
    want_idx, want_off = H.c_compact(mode, want_code)
    for runs16, prefill in ((runs_00, 0x0000), (runs_a5, 0xA5A5)):
        want_runs, want_gc = S.segment(n, want_idx, want_off, prefill=prefill)
        assert np.array_equal(gran_counts, want_gc), what
        assert runs16.shape == want_runs.shape, what
        bad = np.flatnonzero(runs16 != want_runs)
        assert bad.shape[0] == 0, (what, "fill %04x: entry %d of granule %d holds %d, expected %d (units %d)" % (
            prefill, bad[0] % GRAN, bad[0] // GRAN, runs16[bad[0]], want_runs[bad[0]], int(want_gc.reshape(-1, 8)[bad[0] // GRAN].sum())) if bad.shape[0] else "")
    lens = np.diff(want_off.astype(np.int64))
    assert np.array_equal(n_out[:7], lens.astype(np.uint64)) and int(n_out[7]) == int(want_off[7]), what
    assert np.array_equal(counts, want_counts), what


def run_runs_cases(exe, tmp_path, tag, shapes):
    """shapes: (name, mode, cols, bits, m).  int32 columns also run as their binary64 twin (the same lists on integral input)."""
    todo = []
    for name, mode, cols, bits, m in shapes:
        todo.append((name, mode, cols, bits, m))
        if cols[0].dtype == np.int32:
            todo.append((name + " as binary64", mode, S.as_f64(cols), bits, H.NEG if m == ABSENT else float(m)))
    res = run_host(exe, tmp_path, tag, [runs_case(mode, cols, bits, m) for _, mode, cols, bits, m in todo], RUNS_DUMPS)
    for (name, mode, cols, bits, m), got in zip(todo, res):
        check_runs(name, cols[0].shape[0], mode, cols, bits, m, got)


@pytest.mark.parametrize("group", S.GROUPS)
def test_runs_catalogue(exe, tmp_path, group):
    shapes = S.group(group)
    assert shapes
    run_runs_cases(exe, tmp_path, "runs", [(name, mode, cols, S.pack_bits(flags), m) for name, mode, cols, flags, m in shapes])


def test_runs_one_and_two_granules(exe, tmp_path):
    """n = 1, 2047, 2048, 2049 in the three modes: random states and unit masks, and strictly interleaved mates."""
    shapes = []
    for n in SMALL:
        rng = np.random.default_rng(900 + n)
        for mode in (0, 1, 2):
            cols = S.columns_of_states(rng.integers(0, 6, n))
            shapes.append(("n%d/m%d/random" % (n, mode), mode, cols, S.pack_bits(rng.random(n) < (0.55 if mode else 0.9)), ABSENT))
            shapes.append(("n%d/m%d/mode_flags" % (n, mode), mode, cols, S.pack_bits(S.mode_flags(mode, n)), -2))
    run_runs_cases(exe, tmp_path, "runs_small", shapes)


# ---- K3, K1c, K1p on the catalogue of cigar_shapes ---------------------------------------------------------------------

CIGAR_DUMPS = (np.int32, np.uint32)
K1C_DUMPS = (np.uint8, np.uint32)
K1P_DUMPS = (np.uint8, np.uint8, np.uint32, np.uint64, np.uint64, np.uint32, np.uint64, np.uint64)


class Want(object):
    def __init__(self, mode, sp, bits, m):
        self.code, self.counts = H.c_classify(mode, sp[0]["score"], sp[0]["xs"], sp[1]["score"], sp[1]["xs"], bits, m)
        self.idx, self.off = H.c_compact(mode, self.code)
        self.bins = S.bins_of_records(self.code.shape[0], self.idx, self.off)


def packed_of(s):
    return s["packed"] if s["packed"] is not None else H.np_cigar_pack(s["cig_off"], s["cig_oplen"])


def csr_arrays(sp, bits, n):
    return [a for s in sp for a in (s["nm"], s["cig_off"], s["cig_oplen"][:int(s["cig_off"][n])], s["xs"])] + [bits[:(n + 63) // 64]]


def packed_arrays(sp, packed, bits, n):
    out = []
    for s, (cnt, tile, ops) in zip(sp, packed):
        assert cnt.shape[0] == n and tile.shape[0] == (n + 255) // 256 + 1
        out += [s["nm"], cnt, tile, ops[:int(tile[-1])], s["xs"]]              # exactly cig_tile[last] words, not one more
    return out + [bits[:(n + 63) // 64]]


def check_flag(flag, bad, null_flag, what):
    """As check_flag of tests/test_cigar_shapes_gpu.py; without a flag the caller's word stays as it was."""
    if null_flag:
        assert int(flag[0]) == 0, what
    else:
        assert (int(flag[0]) != 0) == (bad != 0), "%s: range_flag %d, the reference clamped %d scores" % (what, int(flag[0]), bad)


def check_k1p(what, n, form, want, got, bad, null_flag):
    from xenomapper_amd import _ffi
    flags, (code, bins4, idx, off, counts, flag, _, _) = got
    check_flags(flags, what)
    check_flag(flag, bad, null_flag, what)
    if form == FORM_CODE:
        assert bins4.shape[0] == 0 and np.array_equal(code, want.code), what + " code"
    else:
        assert code.shape[0] == 0 and bins4.shape[0] == _ffi.bins4_bytes(n), what
        assert np.array_equal(_ffi.unpack_bins4(bins4, n), want.bins), what + " bins4"
        every = np.stack([bins4 & 7, (bins4 >> 4) & 7], axis=1).reshape(-1)
        assert bool((every[n:] == 7).all()), what + ": a record behind n_records closes a unit"
    assert np.array_equal(counts, want.counts), what + " counts"
    assert np.array_equal(off, want.off), what + " offsets"
    assert np.array_equal(idx, want.idx), what + " idx"


def cigar_cases(c, null_flag=0, modes=(0, 1, 2), floors=None):
    """The launches of one catalogue case, and how to check each: K3 on both species with max_blocks 1 and 3 (the grid-stride
    loop wraps from 257 and from 769 records on), K1c and K1p (both output forms) in every mode at the floors of FLOORS."""
    sp, flags = c.columns()
    n, bits = c.n, C.pack_bits(flags)
    packed = [packed_of(s) for s in sp]
    todo = []
    for s in (0, 1):
        for max_blocks in (1, 3):
            def check(got, s=s, what="%s K3 species %d, %d blocks" % (c.name, s + 1, max_blocks)):
                flags_, (as_out, flag) = got
                check_flags(flags_, what)
                check_flag(flag, sp[s]["bad"], null_flag, what)
                assert np.array_equal(as_out, sp[s]["score"]), what
            todo.append((case(CMD_CIGAR, n, max_blocks, null_flag, arrays=csr_arrays(sp, bits, n)[4 * s:4 * s + 3]), CIGAR_DUMPS, check))
    for mode in modes:
        for m in (floors or FLOORS[mode]):
            want = Want(mode, sp, bits, m)
            tag = "%s mode %d m %d" % (c.name, mode, m)

            def check_c(got, want=want, what=tag + " K1c"):
                flags_, (code, flag) = got
                check_flags(flags_, what)
                check_flag(flag, c.bad, null_flag, what)
                assert np.array_equal(code, want.code), what
            todo.append((case(CMD_K1C, n, mode, f64_bits(m), null_flag, arrays=csr_arrays(sp, bits, n)), K1C_DUMPS, check_c))
            for form in (FORM_BINS4, FORM_CODE):
                def check_p(got, want=want, form=form, what="%s K1p form %d" % (tag, form)):
                    check_k1p(what, n, form, want, got, c.bad, null_flag)
                todo.append((case(CMD_K1P, n, mode, f64_bits(m), null_flag, form, int(want.off[7]),
                                  arrays=packed_arrays(sp, packed, bits, n)), K1P_DUMPS, check_p))
    return todo


def run_todo(exe, tmp_path, tag, todo):
    """One run of the program per kind of dump (the cases of a kind in one file)."""
    for dumps in sorted(set(d for _, d, _ in todo), key=len):
        mine = [(cs, check) for cs, d, check in todo if d == dumps]
        for (_, check), got in zip(mine, run_host(exe, tmp_path, "%s_%d" % (tag, len(dumps)), [cs for cs, _ in mine], dumps)):
            check(got)


@pytest.mark.parametrize("c", C.all_cases(), ids=lambda c: c.name)
def test_cigar_case(exe, tmp_path, c):
    assert (c.bad != 0) <= (c.group == "range")
    run_todo(exe, tmp_path, "cigar", cigar_cases(c))


def test_cigar_without_a_range_flag(exe, tmp_path):
    """range_flag == nullptr on cases whose scores leave int32: the outputs hold the clamped scores' results all the same."""
    names = ("range/max_plus1/full/s1", "range/far_below/tail/s2", "range/min_exact/halo/both")
    cases = [c for c in C.all_cases() if c.name in names]
    assert len(cases) == len(names) and all(c.bad for c in cases)
    for c in cases:
        run_todo(exe, tmp_path, "noflag", cigar_cases(c, null_flag=1, floors=(ABSENT,)))


def test_k1p_inconsistent_columns_stay_in_bounds(exe, tmp_path):
    """The six trials of test_classify_cigar_packed_inconsistent_columns_stay_in_bounds (tests/test_gpu_parity.py; the same
    generator and seeds) on exact-size blocks: random count bytes, a tile table that is not monotone or points past the op array,
    escape bytes without trailers.  The results mean nothing and may depend on the fill (a table slot nobody wrote may be
    read); no read leaves the columns, nothing is written outside the outputs, the bookkeeping stays consistent."""
    n = 4 * 2048 + 77
    rng = np.random.default_rng(5)
    n_ops = 5000
    cases = []
    for trial in range(6):
        arrays = []
        for _ in range(2):
            cnt = rng.integers(0, 256, n).astype(np.uint8) if trial % 2 == 0 else np.full(n, 255, dtype=np.uint8)
            tile = rng.integers(0, 2 * n_ops, (n + 255) // 256 + 1).astype(np.uint32)
            if trial >= 3:
                tile.sort()
            tile[-1] = n_ops                                             # the length of the op array is honest
            ops = rng.integers(0, 2**32, n_ops, dtype=np.uint64).astype(np.uint32)
            nm = rng.integers(0, 5, n).astype(np.int32)
            arrays += [nm, cnt, tile, ops, np.full(n, ABSENT, dtype=np.int32)]
        bits = H.synth.pack_unit_bits(rng.random(n) < 0.7)
        for form in (FORM_BINS4, FORM_CODE):
            cases.append(case(CMD_K1P, n, 1, f64_bits(ABSENT), 0, form, n, arrays=arrays + [bits[:(n + 63) // 64]]))
    for k, (flags, (_, _, _, off, counts, _, off_2, counts_2)) in enumerate(run_host(exe, tmp_path, "inconsistent", cases, K1P_DUMPS)):
        check_flags(flags, ("trial", k // 2, "form", k % 2), fill_independent=False)
        for o, cn in ((off, counts), (off_2, counts_2)):
            o = o.astype(np.int64)
            assert int(o[7]) == int(cn.sum()) <= n and (np.diff(o) >= 0).all(), (k, o)


# ---- the plain classify ------------------------------------------------------------------------------------------------

def test_plain_classify(exe, tmp_path):
    """launch_classify<T> without a count plan (xm_classify_dev, xm_classify_f64_dev): int32 columns, and binary64 columns
    with NaNs, modes 0 to 2, sizes around one lane and one workgroup."""
    todo = []
    for n in CLASSIFY_SIZES:
        rng = np.random.default_rng(70 + n)
        vals = np.concatenate([[ABSENT, ABSENT], np.arange(-8, 9)]).astype(np.int64)
        cols = [vals[rng.integers(0, len(vals), n)].astype(np.int32) for _ in range(4)]
        fcols = [rng.integers(-5, 6, n).astype(np.float64) for _ in range(4)]
        fcols[0][rng.random(n) < 0.2] = np.nan
        fcols[2][rng.random(n) < 0.1] = np.nan
        fcols[1][rng.random(n) < 0.1] = -np.inf
        for mode in (0, 1, 2):
            bits = H.synth.pack_unit_bits(rng.random(n) < (0.55 if mode else 0.9))
            for c, m in ((cols, ABSENT), (cols, -2), (fcols, H.NEG), (fcols, 0.5)):
                want_code, _ = H.c_classify(mode, *c, bits, m)
                todo.append(((n, mode, str(c[0].dtype), m), want_code,
                             case(CMD_CLASSIFY, c[0].dtype == np.float64, mode, n, f64_bits(m), arrays=c + [bits[:(n + 63) // 64]])))
    for (what, want_code, _), (flags, (code,)) in zip(todo, run_host(exe, tmp_path, "classify", [t[2] for t in todo], (np.uint8,))):
        check_flags(flags, what)
        assert np.array_equal(code, want_code), what


# ---- K4 ----------------------------------------------------------------------------------------------------------------

def run_correlate(exe, tmp_path, tag, inputs):
    """inputs: (what, track, density) -> bit-exact against the column-wise loop (NaN by position)."""
    cases = [case(CMD_CORRELATE, t.shape[0], d.shape[0], arrays=[t, d]) for _, t, d in inputs]
    for (what, t, d), (flags, (out,)) in zip(inputs, run_host(exe, tmp_path, tag, cases, (np.float64,))):
        check_flags(flags, what)
        want = K.reference(t, d)
        assert K.same(out, want), "%r: %d of %d outputs differ" % (what, K.differing(out, want), want.shape[0])


@pytest.mark.parametrize("m", K.M)
def test_correlate_every_length_at_these_taps(exe, tmp_path, m):
    inputs = []
    for n, track_family, density_family in K.sweep(m):
        inputs.append(((n, m, track_family, density_family),) + K.draw(track_family, density_family, n, m))
    run_correlate(exe, tmp_path, "corr%d" % m, inputs)


@pytest.mark.parametrize("n,m", [(700, 300), (2305, 2049)])
def test_correlate_value_families(exe, tmp_path, n, m):
    inputs = [((n, m, t, d),) + K.draw(t, d, n, m, seed=1) for t, d in K.PAIRS]
    run_correlate(exe, tmp_path, "corr_pairs", inputs)


# ---- the streaming probe ------------------------------------------------------------------------------------------------

def test_stream_probe_stays_inside_its_buffers(exe, tmp_path):
    """Four columns of n int32 and XM_BINS4_BYTES(n) bytes of output: no report, nothing behind the n / 4 values written."""
    sizes = (0, 3, 4, 5, 2047, 2048, 2049, 4099)
    rng = np.random.default_rng(3)
    cases = [case(CMD_PROBE, n, arrays=[rng.integers(-2**31, 2**31, n).astype(np.int32) for _ in range(4)]) for n in sizes]
    for n, (flags, _) in zip(sizes, run_host(exe, tmp_path, "probe", cases, ())):
        check_flags(flags, ("probe", n))
