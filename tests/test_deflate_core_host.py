"""The DEFLATE encoder's logic (xenomapper_amd/csrc/xm_deflate_core.h) without a GPU: the same source compiled for the host with
its 64 lanes emulated one after the other (tests/deflate_core_host.cpp), under ASan + UBSan.  For every payload of
tests/deflate_shapes.py and a few hundred seeded random mixes: zlib inflates the stream to the input, the project's own decoder
(xm_inflate_core.h) does too, the stream is no longer than n + 5, guard bytes around the slot and the scratch are intact, the
input is unchanged, two runs give equal bytes.  The code-length builder by itself on Fibonacci and on equal frequencies; the
compression conditions on the two paired-end BAM fixtures.  The device build of the same source: tests/test_deflate_gpu.py."""
import os
import re
import subprocess
import zlib

import pytest

from tests import deflate_shapes as S
from tests import helpers as H

ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("deflate_core") / "deflate_core_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-Wall", "-Wextra", "-Wno-unknown-pragmas",
                           os.path.join(H.REPO, "tests", "deflate_core_host.cpp"), "-o", path, "-lz"])
    return path


def run(exe, *args):
    proc = subprocess.run([exe] + list(args), capture_output=True, text=True, env=ENV, timeout=600)
    assert proc.returncode == 0, (proc.stdout + proc.stderr)[-3000:]
    assert "runtime error" not in proc.stderr and "AddressSanitizer" not in proc.stderr, proc.stderr[-3000:]
    return proc.stdout


def test_every_shape_and_kind_round_trips_inside_its_slot(exe, tmp_path):
    shapes = S.all_shapes()
    assert len(shapes) > 1500
    blocks, emit = str(tmp_path / "blocks.bin"), str(tmp_path / "streams.bin")
    S.write_blocks(blocks, [p for _, p in shapes])
    out = run(exe, "--blocks", blocks, "--emit", emit)
    m = re.search(r"blocks: (\d+), (\d+) failures, stored (\d+), limited (\d+), forced (\d+)", out)
    assert m, out
    n, bad, stored, limited, forced = (int(g) for g in m.groups())
    assert n == len(shapes) and bad == 0
    assert stored >= 1 and limited >= 1 and forced >= 1, out          # each of the three side paths was taken
    # the streams the program wrote, against Python's zlib too; uniform random bytes come out stored, n + 5 bytes
    streams = S.read_streams(emit)
    assert len(streams) == len(shapes)
    for (name, p), s in zip(shapes, streams):
        assert len(s) <= len(p) + 5, name
        d = zlib.decompressobj(-15)
        assert d.decompress(s) == p.tobytes() and d.eof and not d.unused_data, name
        if name.startswith("random/"):
            assert len(s) == len(p) + 5 and s[:1] == b"\x01", name
    # the distance limit from both sides: matches 32768 back are used (where no later position has taken their place in the hash
    # table: the table keeps one position per hash), matches 32769 back are not -- random bytes otherwise, so: stored
    by_name = {name: (len(p), len(s)) for (name, p), s in zip(shapes, streams)}
    assert by_name["unit32768"][1] < 65000 and by_name["unit32769"][1] == 65285
    assert by_name["far_repeat"][1] == 40005


def test_seeded_random_mixes(exe):
    assert "mix: 300 blocks, 0 failures" in run(exe, "--mix", "300", "17")


def test_code_length_builder_limits_to_15_bits_with_a_full_kraft_sum(exe):
    out = run(exe, "--builder")
    assert out.count(": ok") == 4 and "BAD" not in out
    assert re.search(r"Fibonacci x 22: longest (\d+), Kraft sum 32768 / 32768, limited 1", out)
    assert re.search(r"286 equal: longest 9, Kraft sum 32768 / 32768, limited 0", out)


@pytest.mark.parametrize("which", [0, 1])
def test_compression_conditions_on_the_bam_fixtures(exe, tmp_path, which):
    """smaller than zlib's Z_HUFFMAN_ONLY (matches are found and used), at most 1.15 x zlib level 1; the program computes all
    totals with zlib at run time and prints them (DESIGN.md quotes them)"""
    blocks = str(tmp_path / "fixture.bin")
    S.write_blocks(blocks, S.fixture_blocks(S.BAM_FIXTURES[which]))
    out = run(exe, "--ratio", blocks)
    print(out)
    m = re.search(r"in (\d+), encoder (\d+) .*zlib level 1 (\d+) .*Z_HUFFMAN_ONLY (\d+) ", out)
    assert m, out
    total, ours, level1, huffman = (int(g) for g in m.groups())
    assert total > 100_000 and ours < huffman and ours <= 1.15 * level1


def test_the_order_of_the_emulated_lanes_does_not_matter(tmp_path):
    """R1 / R3 of xm_deflate_core.h: no lane reads what another lane writes in the same phase, so lanes 63 .. 0 in turn give the
    bytes lanes 0 .. 63 give (plain g++: this is about the bytes, the sanitizers ran above)"""
    shapes = S.all_shapes()
    blocks = str(tmp_path / "blocks.bin")
    S.write_blocks(blocks, [p for _, p in shapes])
    emitted = []
    for flag in ([], ["-DXMD_HOST_LANES_REVERSED"]):
        exe, emit = str(tmp_path / ("host%d" % len(flag))), str(tmp_path / ("streams%d.bin" % len(flag)))
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas"] + flag +
                              [os.path.join(H.REPO, "tests", "deflate_core_host.cpp"), "-o", exe, "-lz"])
        proc = subprocess.run([exe, "--blocks", blocks, "--emit", emit], capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0 and ", 0 failures" in proc.stdout, (proc.stdout + proc.stderr)[-2000:]
        emitted.append(open(emit, "rb").read())
    assert emitted[0] == emitted[1]
