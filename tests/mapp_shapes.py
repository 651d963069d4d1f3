"""The catalogue of the single-end mappability front end (include/xenomapper_mappability.h): small SAM bodies built from parts,
each with the windows it is cut into and the block every window must give, computed by a plain-Python model of the C ABI's
contract.  The model follows the reference's LOOP (cur, position), not the kernels' automaton, so it checks that too.

tests/test_mapp_shapes_cpu.py pins the catalogue against the oracle and the package's host route; tests/test_lockstep_mapp_cpu.py
runs the kernels on it lane by lane on the CPU; tests/test_mapp_gpu.py runs xm_mapp_run on it."""
import io
from collections import namedtuple

OK, DECLINED, TOO_MANY_LINES, TOO_MANY_VALUES = 0, 1, 2, 3
R_NONE, R_NON_ASCII, R_SEPARATOR, R_FIELDS, R_NAME_NUMBER, R_POS_NUMBER, R_NOT_SEQUENTIAL = range(7)
SEPARATORS = (0x20, 0x0B, 0x0C, 0x0D, 0x1C, 0x1D, 0x1E, 0x1F)         # what str.split() splits at besides '\t' and '\n' (ASCII)
TILE = 256                                                            # lines per workgroup of M4 / M5 (xm_mapp_kernels.h: MB)
GROUP, CHUNK = 16, 1 << 16                                            # M1: bytes per lane, bytes per workgroup
BIG = 1 << 30                                                         # "no limit" for max_lines / max_values / the window

Segment = namedtuple("Segment", "first_line n_lines key_off key starts base last_pos value_off n_values")
Block = namedtuple("Block", "consumed n_lines status reason declined_line segments values carry_position carry_settled")
# text: the SAM body (bytes, no header); window: bytes per window; max_lines / max_values: the slot's limits;
# heavy: a position near 2^32 -- the ABI tests run it, the track comparisons do not (the host's list would hold 2^32 zeros);
# big: too many lines for the lane-by-lane run on the CPU
Shape = namedtuple("Shape", "name text window max_lines max_values heavy big")
Window = namedtuple("Window", "data eof carry_key carry_position want")


def line(name, rname, pos, mapq="42", tail=("4M", "*", "0", "0", "ACGT", "IIII")):
    return "\t".join((name, "0", rname, str(pos), mapq) + tuple(tail)) + "\n"


def reads(chrom, positions, rname=None, mapq="42", shift=0):
    """One line per position: read chrom_p mapped to rname (default: where it came from) at p + shift."""
    return "".join(line("%s_%d" % (chrom, p), chrom if rname is None else rname, p + shift, mapq) for p in positions)


def padded(text, newline_at):
    """`text` plus one more line of read pad_1 whose '\\n' is byte `newline_at` of the result (an optional field is stretched)."""
    head = line("pad_1", "pad", 1)[:-1] + "\tXX:Z:"
    fill = newline_at - len(text) - len(head)
    assert fill >= 0, (len(text), newline_at)
    return text + head + "x" * fill + "\n"


# ---- the model --------------------------------------------------------------------------------------------------------------------
def _number(field):
    if not 1 <= len(field) <= 10 or any(c not in b"0123456789" for c in field):
        return None
    value = int(field)
    return value if value <= 0xFFFFFFFF else None


_TAKEN = bytes(c for c in range(0x80) if c not in SEPARATORS)          # the bytes the device takes


def parse(text_line):
    """(reason, T, R, name_pos, value) of one line (bytes without its '\\n') under the device's grammar."""
    if text_line.translate(None, _TAKEN):                              # the line's first byte of another kind decides
        first = next(c for c in text_line if c >= 0x80 or c in SEPARATORS)
        return (R_NON_ASCII if first >= 0x80 else R_SEPARATOR), None, None, 0, 0
    f = text_line.split(b"\t")
    if len(f) < 11 or any(x == b"" for x in f[:11]):
        return R_FIELDS, None, None, 0, 0
    name, rname, pos, mapq = f[0], f[2], f[3], f[4]
    cut = name.rfind(b"_")
    true_chrom = name[:cut] if cut >= 0 else b""
    name_pos = _number(name[cut + 1:])
    if name_pos is None:
        return R_NAME_NUMBER, None, None, 0, 0
    at = _number(pos)
    if at is None:
        return R_POS_NUMBER, None, None, 0, 0
    return R_NONE, true_chrom, rname, name_pos, int(true_chrom == rname and name_pos == at and mapq == b"42")


def _rname_at(text_line):
    return len(text_line.split(b"\t", 2)[0]) + len(text_line.split(b"\t", 2)[1]) + 2


def model_window(data, eof, carry_key, carry_position, max_lines=BIG, max_values=BIG):
    """What xm_mapp_run reports for one window.  carry_key: bytes, or None when the loop holds no key yet."""
    carry_position = carry_position if carry_key is not None else 0
    consumed = len(data) if eof else data.rfind(b"\n") + 1
    body = data[:consumed]
    lines = body.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    n = len(lines)

    def failed(status, reason=R_NONE, declined=0):
        return Block(consumed, n, status, reason, declined, [], b"", carry_position, True)
    if n > max_lines:
        return failed(TOO_MANY_LINES)
    parsed = [parse(x) for x in lines]
    begins = [0]
    for x in lines:
        begins.append(begins[-1] + len(x) + 1)
    for i, p in enumerate(parsed):
        if p[0]:
            return failed(DECLINED, p[0], i)
    cur, position = carry_key, carry_position
    segments, offset, last_true = [], 0, None
    for i, (_, true_chrom, rname, name_pos, value) in enumerate(parsed):
        if cur != true_chrom:
            cur, position = rname, 0
            segments.append(dict(first_line=i, key=rname, key_off=begins[i] + _rname_at(lines[i]), starts=1, base=name_pos - 1, cells={}))
        elif not segments:
            segments.append(dict(first_line=0, key=b"", key_off=0, starts=0, base=carry_position, cells={}))
        position += 1
        if name_pos < position:
            return failed(DECLINED, R_NOT_SEQUENTIAL, i)
        position = name_pos
        segments[-1]["cells"][name_pos] = value
        segments[-1]["last_pos"] = name_pos
        last_true = true_chrom
    table, values = [], bytearray()
    for k, s in enumerate(segments):
        behind = segments[k + 1]["first_line"] if k + 1 < len(segments) else n
        count = s["last_pos"] - s["base"]
        table.append(Segment(s["first_line"], behind - s["first_line"], s["key_off"], s["key"], s["starts"], s["base"], s["last_pos"], offset, count))
        offset += count
    if offset > max_values:
        return failed(TOO_MANY_VALUES)
    for s in segments:
        cells = bytearray(s["last_pos"] - s["base"])
        for name_pos, value in s["cells"].items():
            cells[name_pos - s["base"] - 1] = value
        values += cells
    return Block(consumed, n, OK, R_NONE, 0, table, bytes(values), position, (cur == last_true) if n else True)


def host_feed(cur, position, lines):
    """The reference's loop on decoded lines, from a carried state: -> (cur, position); raises what the loop raises."""
    for text in lines:
        name, _flag, chrom, pos, mapq = text.strip("\n").split()[:5]
        true_chrom = "_".join(name.split("_")[:-1])
        if cur != true_chrom:
            cur, position = chrom, 0
        position += 1
        name_pos = int(name.split("_")[-1])
        if name_pos != position:
            if not name_pos > position:
                raise ValueError("Name is not sequential")
            position = name_pos
        int(pos)
    return cur, position


def decoded_lines(raw):
    return io.TextIOWrapper(io.BytesIO(raw), encoding="utf-8", newline=None)


def chain(shape):
    """The windows of a shape as the file route cuts them -> ([Window], the exception type the host loop ends the chain with or
    None).  A window without a line end that is not the file's last is listed, then tried again at twice the size; a window the
    device does not resolve goes through the host loop, which carries the state on."""
    text, size, at = shape.text, shape.window, 0
    cur, position = None, 0
    out = []
    while at < len(text):
        data = text[at:at + size]
        eof = at + size >= len(text)
        key = cur.encode("utf-8") if cur is not None else None
        if position > 0xFFFFFFFF:
            return out, None                                    # (no catalogue text goes on from here)
        want = model_window(data, eof, key, position, shape.max_lines, shape.max_values)
        out.append(Window(data, eof, key, position, want))
        if want.consumed == 0 and not eof:
            size *= 2
            continue
        if want.status == OK:
            if want.segments:
                last = [s for s in want.segments if s.starts]
                if last:
                    cur = last[-1].key.decode("utf-8")
                position = want.carry_position
        else:
            try:
                cur, position = host_feed(cur, position, decoded_lines(data[:want.consumed]))
            except Exception as exc:                            # noqa: the type is what the tests compare
                return out, type(exc)
        at += want.consumed
    return out, None


def limits(shape, want):
    """(max_lines, max_values) to reserve for one window: the shape's own, else what the window needs, met exactly."""
    max_lines = shape.max_lines if shape.max_lines < BIG else max(1, want.n_lines)
    max_values = shape.max_values if shape.max_values < BIG else sum(s.n_values for s in want.segments)
    return max_lines, max_values


def compare(window, got):
    """A block as a front end reported it against the model's.  got: dict with the fields of xm_mapp_block; segments as tuples
    (first_line, n_lines, key_off, key_len, starts, base, last_pos, value_off, n_values), values as bytes."""
    want = window.want
    scalars = dict(consumed=want.consumed, n_lines=want.n_lines, status=want.status, reason=want.reason, declined_line=want.declined_line,
                   n_segments=len(want.segments), n_values=len(want.values), carry_position=want.carry_position,
                   carry_settled=int(want.carry_settled))
    assert {k: int(got[k]) for k in scalars} == scalars
    rows = []
    for first_line, n_lines, key_off, key_len, starts, base, last_pos, value_off, n_values in got["segments"]:
        assert starts or (key_off, key_len) == (0, 0)
        rows.append(Segment(first_line, n_lines, key_off, bytes(window.data[key_off:key_off + key_len]), starts, base, last_pos, value_off,
                            n_values))
    assert rows == want.segments
    assert bytes(got["values"]) == want.values


# ---- the catalogue ----------------------------------------------------------------------------------------------------------------
def _shapes():
    S = []

    def add(name, text, window=BIG, max_lines=BIG, max_values=BIG, heavy=False, big=False):
        S.append(Shape(name, text if isinstance(text, bytes) else text.encode("utf-8"), window, max_lines, max_values, heavy, big))

    # line counts around a wave, a workgroup and M4 / M5's tile; the last line with and without its '\n'
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 2 * TILE + 1):
        add("lines_%d" % n, reads("c", range(1, n + 1)))
    add("last_line_open", reads("c", range(1, 6))[:-1])
    add("two_chromosomes", reads("c", range(1, 70)) + reads("d", range(1, 9)))
    # a line end at byte -1 / 0 / +1 of a 16-byte group and of a 64 KiB chunk
    head = reads("c", (1,))
    for edge, unit in (("group", 8 * GROUP), ("chunk", CHUNK)):
        for delta in (-1, 0, 1):
            add("newline_%s_%+d" % (edge, delta), padded(head, unit + delta) + reads("pad", (2, 3)))
    # windows: every cut, a window smaller than a line (no line end: tried again at twice the size), the last line open
    body = reads("c", range(1, 4)) + reads("d", range(1, 4))
    for size in (16, 31, 32, 33, 34, 35, 66, 100):
        add("window_%d" % size, body, window=size)
    add("window_64_last_open", body[:-1], window=64)
    # segments beginning on lane 0, lane 63 and the first lane of a workgroup
    add("starts_0_63_256", reads("a", range(1, 64)) + reads("b", range(1, 194)) + reads("c", range(1, 10)))
    # runs of reads that are not mapped (RNAME "*"): every one begins a segment until a line has g (its RNAME is its own origin) or x
    # (its origin is the RNAME of the line in front); the run may reach the window's end
    for k in (1, 2, 63, 64, 65):
        run = reads("c", range(1, k + 1), rname="*")
        add("unsettled_%d_then_g" % k, reads("b", (1, 2)) + run + reads("c", range(k + 1, k + 4)))
        add("unsettled_%d_then_x" % k, run + line("c_%d" % (k + 1), "d", 7) + reads("d", range(k + 5, k + 8)))
        add("unsettled_%d_to_the_end" % k, reads("b", (1, 2)) + run)
    front = reads("b", range(1, TILE - 5))
    add("unsettled_over_a_workgroup_edge", front + reads("c", range(1, 12), rname="*") + reads("c", range(12, 15)))
    # the same over windows: the state carried is settled, or unsettled
    run = reads("c", range(1, 6), rname="*")
    for size in (90, 130, 170, 210):
        add("unsettled_windows_%d" % size, reads("b", (1, 2)) + run + reads("c", range(6, 9)), window=size)
        add("unsettled_x_windows_%d" % size, run + line("c_6", "d", 7) + reads("d", range(8, 11)), window=size)
    add("settled_windows", reads("c", range(1, 20)) + reads("d", range(1, 20)), window=256)
    # keys: one byte, more than 64 bytes; a name without '_'; origins that differ in the last byte or in length only
    add("key_1_byte", reads("c", (1, 2)) + reads("d", (1,)))
    add("key_70_bytes", reads("k" * 70, (1, 2, 3)) + reads("k" * 69 + "j", (1, 2)))
    add("key_70_bytes_windows", reads("k" * 70, (1, 2, 3)) + reads("k" * 69 + "j", (1, 2)), window=150)
    add("name_without_underscore", line("12", "c", 12) + line("13", "c", 13) + reads("c", (14,)))
    add("near_origins", reads("chr1a", (1, 2)) + reads("chr1b", (1, 2)) + reads("chr1", (1, 2)) + reads("chr11", (1, 2)) +
        reads("chr1", (3,)))
    # numbers
    add("digits_1_and_10", line("c_5", "c", 5) + line("c_0000000006", "c", "0000000006") + line("c_07", "c", 7) + line("c_8", "c", "08"))
    add("name_pos_2_32_minus_1", line("c_4294967295", "c", 4294967295), heavy=True)
    add("name_pos_2_32", line("c_4294967296", "c", 4294967296), heavy=True)
    add("pos_2_32_minus_1", line("c_1", "c", 4294967295))
    add("pos_2_32", line("c_1", "c", 4294967296))
    add("name_suffix_empty", reads("c", (1,)) + line("c_", "c", 2))
    add("name_suffix_signed", reads("c", (1,)) + line("c_+2", "c", 2))
    add("name_suffix_blank", reads("c", (1,)) + line("c_ 2", "c", 2))
    add("pos_empty", reads("c", (1,)) + line("c_2", "c", ""))
    add("pos_signed", reads("c", (1,)) + line("c_2", "c", "+2"))
    add("pos_blank", reads("c", (1,)) + line("c_2", "c", " 2"))
    add("pos_underscore", reads("c", range(1, 10)) + line("c_10", "c", "1_0"))
    add("pos_equal_and_not", reads("c", (1, 2)) + reads("c", (3, 4), shift=1) + reads("c", (5,)))
    add("mapq_values", "".join(line("c_%d" % (k + 1), "c", k + 1, mapq) for k, mapq in enumerate(("42", "4", "420", "042", "42"))))
    # the line grammar
    add("fields_10", reads("c", (1,)) + line("c_2", "c", 2, tail=("4M", "*", "0", "0", "ACGT")))
    add("fields_11", reads("c", (1,)) + line("c_2", "c", 2, tail=("4M", "*", "0", "0", "ACGT", "I")))
    add("fields_12", reads("c", (1,)) + line("c_2", "c", 2, tail=("4M", "*", "0", "0", "ACGT", "IIII", "NM:i:0")))
    add("field_empty", reads("c", (1,)) + line("c_2", "c", 2, tail=("", "*", "0", "0", "ACGT", "IIII")))
    add("field_11_empty", reads("c", (1,)) + line("c_2", "c", 2, tail=("4M", "*", "0", "0", "ACGT", "", "NM:i:0")))
    add("field_5_missing", reads("c", (1,)) + "c_2\t0\tc\t2\n")
    add("line_empty", reads("c", (1,)) + "\n" + reads("c", (2,)))
    # every separator, and a character beyond ASCII, as the first, a middle and the last byte of a window
    three = reads("c", (1, 2, 3))[:-1]
    for code in SEPARATORS + (0xE9,):
        mark = chr(code).encode("utf-8")                                     # U+00E9: two bytes, both >= 0x80
        raw = three.encode("utf-8")
        add("byte_%02x_first" % code, mark + raw)
        add("byte_%02x_middle" % code, raw[:60] + mark + raw[60:])
        add("byte_%02x_last" % code, raw + mark)
        later = reads("c", (3, 4, 5)).encode("utf-8")
        add("byte_%02x_second_window" % code, reads("c", (1, 2)).encode("utf-8") + later[:80] + mark + later[80:], window=100)
    # gaps, and the limits met and exceeded by one
    add("gap_1", reads("c", (1, 3, 4)))
    add("gap_100000", reads("c", (1, 2, 100003, 100004)))
    gaps = reads("c", (3, 4, 9)) + reads("d", (2, 5))                        # 7 + 4 values, 5 lines
    add("max_values_met", gaps, max_values=11)
    add("max_values_exceeded", gaps, max_values=10)
    add("max_lines_met", gaps, max_lines=5)
    add("max_lines_exceeded", gaps, max_lines=4)
    add("max_lines_exceeded_last_open", gaps[:-1], max_lines=4)
    # a name_pos that does not go up: in a later line, and in a window's first line against the state carried in
    for what, p in (("equal", 3), ("smaller", 2), ("zero", 0)):
        add("not_sequential_%s" % what, reads("c", (1, 2, 3)) + reads("c", (p, 5)))
        add("not_sequential_%s_first_of_window" % what, reads("c", (1, 2, 3)) + reads("c", (p, 5)), window=len(reads("c", (1, 2, 3))))
    add("not_sequential_zero_begins_a_segment", reads("c", (1,)) + reads("d", (0, 1)))
    # more lines than M4 / M5's grids cover at one line a lane (2048 workgroups), and than the part scans take one tile a lane
    n = 2048 * TILE + 1
    add("lines_%d" % n, "".join("c_%d\t0\tc\t%d\t42\tM\t*\t0\t0\tA\tI\n" % (p, p) for p in range(1, n + 1)), big=True)
    return S


SHAPES = _shapes()
BY_NAME = {s.name: s for s in SHAPES}
assert len(BY_NAME) == len(SHAPES)
