"""The SAM-line-to-BAM-record core (xenomapper_amd/csrc/xm_samrec.h) without a GPU: the header compiled for the host in a stand-alone
program (tests/samrec_core_host.cpp) under ASan + UBSan.  Every catalogue line of tests/sam_records.py lies in a heap buffer of
exactly its length plus the header's read margin, the record goes into a buffer of exactly the size step 1 gave, between guard
bytes, once whole and once with SEQ / QUAL packed in 64 interleaved shares as the device's wave packs them; the records and the
reasons, for the device's form and the host's, are compared here with the Python model.  The device build: test_sam_records_gpu.py."""
import os
import struct
import subprocess

import pytest

from tests import helpers as H
from tests import sam_records as R

ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")


def write_items(path, items):
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(items)))
        for it in items:
            fh.write(struct.pack("<I", len(it)) + it)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("samrec_core") / "samrec_core_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           os.path.join(H.REPO, "tests", "samrec_core_host.cpp"), "-o", path])
    return path


def test_every_catalogue_line_in_exact_buffers_equals_the_model(exe, tmp_path):
    cat = R.catalogue()
    extra = [b"", b"\t", b"\t" * 10, b"\t" * 12, R.make() + b"\t", R.make()[:-1], b"a\t0\t*\t0\t0\t*\t*\t0\t0\t*\t*"]
    lines = [e[1] for e in cat] + extra
    lines_bin, refs_bin, out_bin = (str(tmp_path / n) for n in ("lines.bin", "refs.bin", "out.bin"))
    write_items(lines_bin, lines)
    write_items(refs_bin, R.REFS)
    proc = subprocess.run([exe, lines_bin, refs_bin, out_bin], capture_output=True, text=True, env=ENV, timeout=600)
    assert proc.returncode == 0, (proc.stdout + proc.stderr)[-3000:]
    assert "runtime error" not in proc.stderr and "AddressSanitizer" not in proc.stderr, proc.stderr[-3000:]
    assert "lines: %d, 0 failures, names: 5000" % len(lines) in proc.stdout, proc.stdout
    displaced = int(proc.stdout.split("displaced ")[1].split(",")[0])
    assert displaced > 100, proc.stdout                  # probes run past their home entry
    blob = open(out_bin, "rb").read()
    p = compared = nbytes = 0
    for line in lines:
        for host in (False, True):
            reason, size = struct.unpack_from("<iI", blob, p)
            rec = blob[p + 8:p + 8 + size]
            p += 8 + size
            want, why = R.try_encode(line, R.REFS, host=host)
            assert reason == why, (line[:60], host, reason, why)
            assert rec == (want or b""), (line[:60], host)
            compared += 1
            nbytes += size
    assert p == len(blob) and compared == 2 * len(lines) and nbytes > 500_000
