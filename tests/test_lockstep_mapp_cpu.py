"""The launches of the single-end mappability front end (xm_mapp_kernels.h: M1 .. M6) executed on the CPU, lane by lane, under ASan +
UBSan: the header compiled for the host through the lockstep shim (tests/lockstep) by tests/lockstep_mapp_host.cpp, a stand-alone
program.  This file writes every window of the catalogue (tests/mapp_shapes.py) with the state carried into it; the program runs each
twice (all buffers and LDS filled with 0x00, then 0xA5) in heap blocks of exactly the sizes the front end reserves for the window's
limits, which are met exactly; what it dumps is compared here with the model, field by field.  Why: the GPU runs hand the kernels
hipMalloc blocks, which are rounded up, so a kernel may read or write a little past a buffer, or read memory it has not written,
and pass them all."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import lockstep_build as L
from tests import mapp_shapes as S

SEG = np.dtype([("first_line", "<u4"), ("n_lines", "<u4"), ("key_off", "<u4"), ("key_len", "<u4"), ("starts", "<u4"), ("base", "<u4"),
                ("last_pos", "<u4"), ("reserved", "<u4"), ("value_off", "<u8"), ("n_values", "<u8")])
NAMES = ("consumed", "n_lines", "n_segments", "n_values", "status", "reason", "declined_line", "carry_position", "carry_settled")
GROUPS = 6


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return L.host_program(tmp_path_factory, "lockstep_mapp_host")


def cases():
    """(shape name, window index, shape, Window) of every window the lane-by-lane run takes."""
    out = []
    for shape in S.SHAPES:
        if not shape.big:
            out.extend((shape.name, k, shape, w) for k, w in enumerate(S.chain(shape)[0]))
    return out


def run_host(exe, tmp_path, batch):
    path, dump = str(tmp_path / "mapp.cases"), str(tmp_path / "mapp.out")
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(batch)))
        for _, _, shape, w in batch:
            max_lines, max_values = S.limits(shape, w.want)
            key = w.carry_key or b""
            fh.write(struct.pack("<QQIIIII", max_lines, max_values, len(w.data), int(w.eof), int(w.carry_key is not None),
                                 w.carry_position, len(key)))
            fh.write(key)
            fh.write(w.data)
    proc = subprocess.run([exe, path, dump], capture_output=True, text=True, env=L.ENV, timeout=1200)
    assert "lockstep:" not in proc.stderr, proc.stderr[-3000:]                       # divergence, watchdog
    assert "AddressSanitizer" not in proc.stderr and "runtime error" not in proc.stderr, proc.stderr[-4000:]
    assert proc.returncode == 0, (proc.stdout + proc.stderr)[-3000:]
    blob = open(dump, "rb").read()
    os.remove(path)
    os.remove(dump)
    at, out = 0, []
    for _ in batch:
        flags, = struct.unpack_from("<I", blob, at)
        got = dict(zip(NAMES, struct.unpack_from("<9Q", blob, at + 4)), same=flags & 1)
        at += 4 + 72
        rows = np.frombuffer(blob, dtype=SEG, count=got["n_segments"], offset=at)
        at += rows.nbytes
        got["segments"] = [tuple(int(r[f]) for f in SEG.names if f != "reserved") for r in rows]
        got["values"] = blob[at:at + got["n_values"]]
        at += got["n_values"]
        out.append(got)
    assert at == len(blob)
    return out


@pytest.mark.parametrize("group", range(GROUPS))
def test_every_launch_lane_by_lane(exe, tmp_path, group):
    batch = cases()[group::GROUPS]
    assert batch
    for (name, k, _, window), got in zip(batch, run_host(exe, tmp_path, batch)):
        try:
            assert got["same"], "the 0x00 and the 0xA5 run differ"
            S.compare(window, got)
        except AssertionError as exc:
            raise AssertionError("%s, window %d: %s" % (name, k, exc)) from exc


def test_the_catalogue_reaches_every_outcome():
    """What the lane-by-lane run covers: every status, every reason, carried states of both kinds, windows without a line end."""
    seen = [w.want for _, _, _, w in cases()]
    assert {b.status for b in seen} == {S.OK, S.DECLINED, S.TOO_MANY_LINES, S.TOO_MANY_VALUES}
    assert {b.reason for b in seen} == set(range(7))
    assert {b.carry_settled for b in seen if b.status == S.OK and b.n_lines} == {True, False}
    assert any(b.consumed == 0 and b.n_lines == 0 for b in seen)
    assert any(s.starts == 0 for b in seen for s in b.segments)
