"""Pins the catalogue of tests/mapp_shapes.py, without a GPU.  For every text, the tracks the MODEL gives -- its blocks chained over
the text's windows by the package's own window loop (mappability._tracks_on_device, handed a front end that answers from the model),
the windows it declines going through _TrackBuilder -- must be the wiggle text of the oracle (oracle.mappability_oracle) and of the
package's host route, or end in the same exception.  And the _TrackBuilder refactor is held against the E. coli fixture's digest."""
import hashlib
import io
import os
import types

import numpy as np
import pytest

from oracle import mappability_oracle as O
from tests import helpers as H
from tests import mapp_shapes as S
from xenomapper_amd import _ffi
from xenomapper_amd import mappability as mp

ECOLI = os.path.join(H.GOLDEN, "ref_data", "test_from_EcoliK12DH10B_150reads.sam")
ECOLI_SHA224 = "e8e8557a16c05aaa436c2c0fe616450d82a955e0f6de8eb3d190cdf4"        # tests/test_mappability.py
ECOLI_SIZES = {"Chromosome": 2752, "A_Repeat": 991}
LIGHT = [s for s in S.SHAPES if not s.heavy]


class ModelFrontEnd(object):
    """What _tracks_on_device asks of _ffi.Mappability, answered by the model; the windows it was given are kept."""

    def __init__(self, shape=None):
        self.shape, self.seen = shape, []

    def reserve(self, slot, window, max_lines, max_values):
        self.buffer = np.zeros(window, dtype=np.uint8)
        # (a catalogue text comes with its own limits: the package's are sized for lines of real reads)
        self.limits = (self.shape.max_lines, self.shape.max_values) if self.shape else (max_lines, max_values)

    def staging(self, slot):
        return self.buffer

    def run(self, slot, length, eof, carry_key, carry_position):
        data = self.buffer[:length].tobytes()
        want = S.model_window(data, eof, carry_key, carry_position, *self.limits)
        self.seen.append(S.Window(data, bool(eof), carry_key, carry_position if carry_key is not None else 0, want))
        rows = np.zeros(len(want.segments), dtype=_ffi.MAPP_SEGMENT)
        for row, s in zip(rows, want.segments):
            row["first_line"], row["n_lines"], row["key_off"], row["key_len"] = s.first_line, s.n_lines, s.key_off, len(s.key)
            row["starts"], row["base"], row["last_pos"], row["value_off"], row["n_values"] = s.starts, s.base, s.last_pos, s.value_off, s.n_values
        return types.SimpleNamespace(consumed=want.consumed, n_lines=want.n_lines, n_segments=len(rows), n_values=len(want.values),
                                     status=want.status, reason=want.reason, declined_line=want.declined_line, segments=rows,
                                     values=np.frombuffer(want.values, dtype=np.uint8), carry_position=want.carry_position,
                                     carry_settled=want.carry_settled, ms_upload=0.0, ms_kernels=0.0)


def outcome(call):
    """The text a route writes, or the type of what it raises."""
    try:
        return call()
    except Exception as exc:                                          # noqa: the type is what is compared
        return type(exc)


def by_oracle(path):
    with open(path, encoding="utf-8") as fh:
        return O.wiggle_text(O.single_end_track_from_sam(fh))


def by_host(path, sizes={}):
    out = io.StringIO()
    with open(path, encoding="utf-8") as fh:
        mp.single_end_mappability_from_sam(fh, outfile=out, chromosome_sizes=sizes)
    return out.getvalue()


def by_model(path, front_end, sizes={}):
    out = io.StringIO()
    stats = mp._new_stats()
    with open(path, encoding="utf-8") as fh:
        mp.get_sam_header(fh)
        tracks = mp._tracks_on_device(fh, mp._trusted_offset(fh), sizes, front_end, stats)
    mp._write_tracks(tracks, out)
    return out.getvalue(), stats


@pytest.mark.parametrize("shape", LIGHT, ids=lambda s: s.name)
def test_model_tracks_are_the_oracles_and_the_host_routes(shape, tmp_path, monkeypatch):
    path = str(tmp_path / "reads.sam")
    with open(path, "wb") as fh:
        fh.write(shape.text)
    monkeypatch.setattr(mp, "_window_bytes", lambda: min(shape.window, max(1, len(shape.text))))
    front_end = ModelFrontEnd(shape)
    host, model, oracle = outcome(lambda: by_host(path)), outcome(lambda: by_model(path, front_end)), outcome(lambda: by_oracle(path))
    windows, raised = S.chain(shape)
    if not shape.text.decode("utf-8").replace("\r", "\n").split("\n")[0]:
        # no text, or an empty first line: get_sam_header ends both routes of the package before any window is read
        assert host is IndexError and model is IndexError
        return
    if isinstance(host, type):
        # (the oracle indexes the fields, the package unpacks a slice of them: a line of fewer than five is IndexError there, ValueError here)
        assert model is host and raised is host and (oracle is host or (oracle, host) == (IndexError, ValueError))
    else:
        assert raised is None and model[0] == host == oracle
        stats = model[1]
        assert stats["windows_device"] == sum(1 for w in windows if w.want.status == S.OK and (w.want.consumed or w.eof))
        assert stats["windows_host"] == sum(1 for w in windows if w.want.status != S.OK)
        assert stats["lines"] == shape.text.decode("utf-8").replace("\r\n", "\n").replace("\r", "\n").count("\n") + \
            (0 if shape.text.endswith((b"\n", b"\r")) or not shape.text else 1)
    # the windows the package's loop cut are the catalogue's, with the same carried state
    assert [w[:4] for w in front_end.seen] == [w[:4] for w in windows]


def test_track_builder_on_the_ecoli_fixture(monkeypatch):
    """The refactored loop writes what the loop wrote before; the model's route, cut into 1 KiB windows, writes it too."""
    for sizes in (ECOLI_SIZES, {}):
        host = by_host(ECOLI, sizes)
        if sizes:
            assert hashlib.sha224(host.encode("latin-1")).hexdigest() == ECOLI_SHA224
        monkeypatch.setattr(mp, "_window_bytes", lambda: 1024)
        out = io.StringIO()
        stats = mp._new_stats()
        with open(ECOLI, encoding="utf-8") as fh:
            mp.get_sam_header(fh)
            tracks = mp._tracks_on_device(fh, mp._trusted_offset(fh), sizes, ModelFrontEnd(), stats)
        mp._write_tracks(tracks, out)
        assert out.getvalue() == host
        assert stats["windows_host"] == 0 and stats["windows_device"] > 100 and stats["lines"] == 3462


def test_track_builder_carries_its_state():
    """feed() in two parts is feed() of the whole."""
    text = (S.reads("c", range(1, 6)) + S.reads("d", (2, 3))).splitlines(True)
    whole, parts = mp._TrackBuilder(), mp._TrackBuilder()
    whole.feed(text)
    parts.feed(text[:3])
    parts.feed(text[3:])
    assert dict(whole.finish()) == dict(parts.finish()) == {"c": [1] * 5, "d": [0, 1, 1]}
