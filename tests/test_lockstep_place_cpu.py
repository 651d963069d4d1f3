"""The fused step's launches (counting classify_kernel or hist_kernel, scan_kernel, scatter_kernel) executed on the CPU, lane by
lane, under ASan + UBSan: xm_kernels.hip compiled for the host through the lockstep shim (tests/lockstep) by
tests/lockstep_place_host.cpp, with ROCm's host clang++.  This file writes the cases, that program runs each twice (workspace,
outputs and LDS filled with 0x00, then 0xA5) in heap blocks of exactly the sizes include/xenomapper_hip.h promises, and what it
dumps is compared here with the oracle, exactly.  Why: the GPU tests hand the kernels torch tensors, which are rounded up to 512
bytes inside 2 MB segments, so a kernel may read or write a little past a buffer, or read stale workspace, and pass them all.

Sizes: 1, 2047, 2048, 2049 (one or two granules: every destination, both scatter inputs, K2a), 81 923 (40 granules + 3 records:
XM_SCATTER_WAVES 7 and 100 give runs of 6 granules with a short last run, and one granule per wave), 2 097 157 (1024 granules + 5:
the scan's part carry) and 4 196 357 (2049 granules + 5: the chunked order of place_steps at XM_PLACE_CHUNK_PARTS=1)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import lockstep_build as L
from tests import runs_shapes as S

GRAN = 2048
ENV = L.ENV
ABSENT = -2**31
IN_BINS4, IN_CODE, IN_HIST = 0, 1, 2
TO_FLAT, TO_LISTS, TO_LISTS_STATE6 = 0, 1, 2
SMALL = (1, 2047, 2048, 2049)
RUNS_N = 81_923
CARRY_N = 1024 * GRAN + 5
CHUNKED_N = 2049 * GRAN + 5
MASKS = ("interleaved", "pe2_p55", "se_all", "pe1_p30", "se_staged_then_not", "skew85")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return L.host_program(tmp_path_factory, "lockstep_place_host")


def random_columns(rng, n, spread=8):
    vals = np.concatenate([[ABSENT, ABSENT], np.arange(-spread, spread + 1)]).astype(np.int64)
    return [vals[rng.integers(0, len(vals), n)].astype(np.int32) for _ in range(4)]


def dataset(mask, n, seed=777):
    """(mode, cols, unit_bits, min_score): the loops and unit masks of test_scatter_runs_of_granules_equal_one_granule_per_wave,
    and strictly interleaved mates with 85 % of the units in one bin, one read without a mate in the second granule (so the
    flagship body's skew form and its fallback both run)."""
    rng = np.random.default_rng(seed + n % 1000 + 13 * MASKS.index(mask))
    if mask == "skew85":
        units = np.where(rng.random((n + 1) // 2) < 0.85, 0, rng.integers(0, 6, (n + 1) // 2))
        flags = S.name_stream_flags(n, (GRAN + 300,))[:n] if n > GRAN + 302 else S.interleaved_flags(n)
        return 1, S.columns_of_states(S.pair_states(1, units, n)), S.pack_bits(flags), ABSENT
    cols = random_columns(rng, n)
    if mask == "interleaved":
        return 1, cols, H.synth.interleaved_unit_bits(n), -2
    mode, p = {"pe2_p55": (2, 0.55), "se_all": (0, 1.0), "pe1_p30": (1, 0.3), "se_staged_then_not": (0, 0.8)}[mask]
    flags = rng.random(n) < p
    if mask == "se_staged_then_not":
        flags[: n // 2] = True                                        # staged granules in front, unstaged ones behind
    return mode, cols, H.synth.pack_unit_bits(flags), -2


def bin_table(mode):
    lib = H.c_oracle()
    t = np.full(256, 7, dtype=np.uint8)
    for c in range(64):
        t[c] = lib.xmo_bin(mode, c >> 3, c & 7)
    return t


def run_host(exe, tmp_path, tag, cols, bits, m, want_code, variants):
    """variants: dicts with mode, input, dest, waves, chunk_parts, flat_units, cap -> one dict of outputs per variant."""
    n = cols[0].shape[0]
    is_f64 = cols[0].dtype == np.float64
    cases, out = str(tmp_path / (tag + ".cases")), str(tmp_path / (tag + ".out"))
    with open(cases, "wb") as fh:
        fh.write(struct.pack("<IIQd", int(is_f64), len(variants), n, float(m)))
        for c in cols:
            fh.write(np.ascontiguousarray(c).tobytes())
        fh.write(np.ascontiguousarray(bits, dtype=np.uint64)[: (n + 63) // 64].tobytes())
        fh.write(want_code.tobytes())
        for v in variants:
            fh.write(struct.pack("<IIIIIIQ", v["mode"], v["input"], v["dest"], v["waves"], v["chunk_parts"], v["flat_units"], v["cap"]))
    proc = subprocess.run([exe, cases, out], capture_output=True, text=True, env=ENV, timeout=1200)
    assert "lockstep:" not in proc.stderr, (tag, proc.stderr[-3000:])           # divergence, watchdog
    assert "AddressSanitizer" not in proc.stderr and "runtime error" not in proc.stderr, (tag, proc.stderr[-4000:])
    assert proc.returncode == 0, (tag, (proc.stdout + proc.stderr)[-3000:])
    blob = open(out, "rb").read()
    os.remove(cases)
    os.remove(out)
    at, res = 0, []

    def take(dtype):
        nonlocal at
        k, = struct.unpack_from("<Q", blob, at)
        a = np.frombuffer(blob, dtype=dtype, count=k, offset=at + 8)
        at += 8 + k * a.itemsize
        return a

    for _ in variants:
        flags, = struct.unpack_from("<I", blob, at)
        at += 4
        r = dict(flags=flags, counts=take(np.uint64), totals=take(np.uint64), code=take(np.uint8), bins4=take(np.uint8), flat=take(np.uint32))
        r["lists"] = [take(np.uint32) for _ in range(7)]
        res.append(r)
    assert at == len(blob)
    return res


def check(tag, n, v, r, want_code, want_counts, want_idx, want_off, bins):
    """One variant's dump against the oracle: integers, so no tolerance."""
    what = (tag, v)
    assert r["flags"] & 1, ("the 0x00 and the 0xA5 run differ", what)
    assert r["flags"] & 2, ("part_tot or the count replicas are not all zero afterwards", what)
    assert r["flags"] & 4, ("written behind a list's entries", what)
    assert np.array_equal(r["counts"], want_counts), what
    lens = np.diff(want_off.astype(np.int64))
    if v["dest"] == TO_FLAT:
        assert np.array_equal(r["totals"], want_off), what
        assert np.array_equal(r["flat"], want_idx), what
    else:
        assert np.array_equal(r["totals"][:7], lens.astype(np.uint64)) and r["totals"][7] == want_off[7], what     # the full lengths
        for b in range(7):
            keep = min(int(lens[b]), v["cap"]) if (b < 6 or v["dest"] == TO_LISTS_STATE6) else 0
            assert np.array_equal(r["lists"][b], want_idx[int(want_off[b]):int(want_off[b]) + keep]), (what, b)
    if v["input"] == IN_BINS4:
        got = np.stack([r["bins4"] & 15, r["bins4"] >> 4], axis=1).reshape(-1)
        assert got.shape[0] == S.granules(n) * GRAN
        assert np.array_equal(got[:n] & 7, bins) and bool((got[n:] & 7 == 7).all()), what
    else:
        assert np.array_equal(r["code"], want_code), what


def variants_of(mode, n, want_off, waves_list, inputs=(IN_BINS4, IN_CODE), dests=("flat", "full", "half"), hist=False, chunk_parts=0):
    lens = np.diff(want_off.astype(np.int64))
    out = []
    for waves in waves_list:
        for inp in inputs:
            for dest in dests:
                v = dict(mode=mode, input=inp, waves=waves, chunk_parts=chunk_parts, flat_units=int(want_off[7]), cap=0, dest=TO_FLAT)
                if dest == "full":
                    v.update(dest=TO_LISTS, cap=n)
                elif dest == "half":
                    v.update(dest=TO_LISTS, cap=int(lens.max()) // 2)      # comes back truncated, the full lengths in n_out
                out.append(v)
    if hist:                                                             # K2a on given category bytes (xm_compact*)
        out.append(dict(mode=mode, input=IN_HIST, waves=0, chunk_parts=0, flat_units=int(want_off[7]), cap=0, dest=TO_FLAT))
    return out


def oracle(mode, cols, bits, m):
    want_code, want_counts = H.c_classify(mode, *cols, bits, m)
    want_idx, want_off = H.c_compact(mode, want_code)
    return want_code, want_counts, want_idx, want_off, bin_table(mode)[want_code]


def run_and_check(exe, tmp_path, tag, mode, cols, bits, m, variants_from):
    n = cols[0].shape[0]
    want = oracle(mode, cols, bits, m)
    variants = variants_from(want[3])
    res = run_host(exe, tmp_path, tag, cols, bits, m, want[0], variants)
    for v, r in zip(variants, res):
        check(tag, n, v, r, *want)
    return len(variants)


@pytest.mark.parametrize("mask", MASKS)
def test_one_and_two_granules_every_form(exe, tmp_path, mask):
    """n = 1, 2047, 2048, 2049: both scatter inputs and K2a, flat list, six lists with room and truncating ones.  The
    run-of-granules form cannot occur, so XM_SCATTER_WAVES stays unset."""
    for n in SMALL:
        mode, cols, bits, m = dataset(mask, n)
        run_and_check(exe, tmp_path, "%s_%d" % (mask, n), mode, cols, bits, m,
                      lambda off: variants_of(mode, n, off, (0,), hist=True))


@pytest.mark.parametrize("mask", MASKS)
def test_runs_of_granules_and_one_granule_per_wave(exe, tmp_path, mask):
    """81 923 records = 40 granules + 3: XM_SCATTER_WAVES = 7 and 100 (runs of 6 granules, the last run short, the last granule
    partial; 100: one granule per wave, as with the variable unset)."""
    mode, cols, bits, m = dataset(mask, RUNS_N)
    k = run_and_check(exe, tmp_path, mask, mode, cols, bits, m,
                      lambda off: variants_of(mode, RUNS_N, off, (7, 100, 0), hist=True))
    assert k == 19


def test_binary64_with_nan_and_the_state6_list(exe, tmp_path):
    """binary64 columns with NaNs, the seventh list, runs of granules and one granule per wave."""
    rng = np.random.default_rng(4242)
    n = RUNS_N
    f = [rng.integers(-5, 6, n).astype(np.float64) for _ in range(4)]
    f[0][rng.random(n) < 0.1] = np.nan
    f[2][rng.random(n) < 0.05] = np.nan
    bits = H.synth.pack_unit_bits(rng.random(n) < 0.7)
    want = oracle(2, f, bits, 0.5)
    assert int(want[3][7] - want[3][6]) > 100                           # units holding state 6 exist
    variants = [dict(mode=2, input=inp, dest=TO_LISTS_STATE6, waves=w, chunk_parts=0, flat_units=0, cap=n) for inp in (IN_BINS4, IN_CODE) for w in (7, 0)]
    variants.append(dict(mode=2, input=IN_BINS4, dest=TO_FLAT, waves=0, chunk_parts=0, flat_units=int(want[3][7]), cap=0))
    res = run_host(exe, tmp_path, "f64", f, bits, 0.5, want[0], variants)
    for v, r in zip(variants, res):
        check("f64", n, v, r, *want)


def test_part_carry_and_chunked_order(exe, tmp_path):
    """The two large sizes, cut to what their purpose needs (the whole file was measured first): 1024 granules + 5
    records, where scan_kernel's second part takes its carry from the part totals (flat list and six lists, compact stream);
    2049 granules + 5 with XM_PLACE_CHUNK_PARTS=1, the smallest input place_steps goes over in chunks (three of them)."""
    mode, cols, bits, m = dataset("pe2_p55", CARRY_N)
    run_and_check(exe, tmp_path, "carry", mode, cols, bits, m,
                  lambda off: variants_of(mode, CARRY_N, off, (0,), inputs=(IN_BINS4,), dests=("flat", "full")))
    mode, cols, bits, m = dataset("se_staged_then_not", CHUNKED_N)
    run_and_check(exe, tmp_path, "chunked", mode, cols, bits, m,
                  lambda off: variants_of(mode, CHUNKED_N, off, (0,), inputs=(IN_BINS4,), dests=("full",), chunk_parts=1))
