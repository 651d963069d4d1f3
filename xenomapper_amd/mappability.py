"""Drop-in for the reference's experimental `xenomappability` tool (xenomapper/mappability.py, v1.0.2;
SURVEY.md 8f-4): paired-end mappability estimated from single-end mappability and the observed insert-size
distribution.  Same names and behaviour; the one numeric loop -- Mappability.single_end_to_paired, a
correlation of every chromosome track with the mate density (ref :94-124) -- runs on the GPU through
xm_mate_correlate (bit-identical to the Python loop: binary64, multiply and add rounded separately, left to
right).  Step 3, single_end_mappability_from_sam, runs on the GPU too when asked to (on_device=True, --on_device): windows of
the name-sorted SAM are read into page-locked memory, and the kernels of csrc/xm_mapp_kernels.h index the lines, parse the five
fields that decide a value, resolve where the reference's loop begins a new track (a prefix scan of two-bit maps) and scatter
one byte per line (include/xenomapper_mappability.h); a window outside the device's grammar goes through the same loop as
without the keyword (_TrackBuilder), from the state the windows in front left.  Without the keyword nothing runs on the device.
Everything else here is text handling and small-list statistics and stays on the host.
"""
from __future__ import annotations

import argparse
import io
import itertools
import os
import sys
import time
from collections import Counter
from statistics import mean

import numpy as np

from . import _ffi
from .xenomapper import default_context, get_sam_header

__version__ = "1.0.2"


class Mappability(dict):
    """{chromosome: per-position mappability list}, with wiggle I/O (ref :38-124)."""

    def __init__(self, chromosome_sizes={}):
        if chromosome_sizes:
            for chrom in chromosome_sizes:
                self[chrom] = [0] * chromosome_sizes[chrom]
        self.chromosome_sizes = chromosome_sizes

    def to_wiggle(self, wigglefile=sys.stdout, chromosomes=[]):
        """fixedStep wiggle, start=1 step=1, chromosomes in sorted order (ref :46-57)."""
        for chrom in sorted(self):
            if not chromosomes or chrom in chromosomes:
                wigglefile.write("fixedStep\tchrom={0}\tstart=1\tstep=1\n".format(chrom))
                wigglefile.write("".join(str(score) + "\n" for score in self[chrom]))

    def from_wiggle(self, wigglefile=sys.stdin, datatype=float):
        """Load chromosomes from a fixedStep wiggle (declaration lines "fixedStep<TAB>chrom=NAME<TAB>start=1<TAB>step=1",
        one value per line after them), replacing tracks of the same name; may be called again for more files.
        Behaviour pinned by the reference's tests (ref :59-92): a declared track that stays empty is dropped unless it is
        the last one of the file, which is always stored -- under the key None when the file declares nothing."""
        tracks = [(None, [])]                         # (name, values) in file order; values go to the last one
        for text in wigglefile:
            if not text.startswith("fixedStep"):
                tracks[-1][1].append(datatype(text))
                continue
            declared = text.strip().split("\t")
            key_and_name = declared[1].split("=")
            if key_and_name[0] != "chrom" or declared[2] != "start=1" or declared[3] != "step=1":
                raise ValueError('Unsupported wiggle fixed step format [must be in the format "fixedStep '
                                 'chrom=chrX start=1 step=1"] {0}'.format(declared))
            tracks.append((key_and_name[1], []))
        for name, values in tracks[:-1]:
            if name and values:
                self[name] = values
        self[tracks[-1][0]] = tracks[-1][1]
        self.chromosome_sizes.update((name, len(track)) for name, track in self.items())

    def single_end_to_paired(self, mate_density=[1]):
        """Paired-end mappability: a uniquely mappable position stays 1.0, any other gets the density-weighted
        mappability of where its mate may fall (ref :94-124).  One GPU launch per chromosome."""
        assert abs(sum(mate_density) - 1.0) < 0.000001
        ctx = default_context()
        density = np.asarray(mate_density, dtype=np.float64)
        paired = Mappability(chromosome_sizes=self.chromosome_sizes)
        for chrom in self:
            track = np.asarray(self[chrom], dtype=np.float64)
            values = ctx.mate_correlate(track, density).tolist()
            # the reference assigns element by element into [0] * size: a longer track raises IndexError on the way, a
            # shorter one leaves the integer zeros behind it
            if len(values) > len(paired[chrom]):
                raise IndexError("list assignment index out of range")
            paired[chrom][:len(values)] = values
        return paired


def parse_fasta(fastafile, token=">"):
    """(name, sequence) of every record of a (multi-)FASTA handle, streamed record by record; the handle is closed when
    the generator finishes.  As the reference's parser (ref :127-146): lines are stripped, a header is a line that starts
    with `token` and its name is that line without its first character, lines in front of the first header are ignored,
    and a record whose name is empty is not reported."""
    def numbered(handle):                                  # every line with the number of headers seen so far
        seen = 0
        for raw in handle:
            line = raw.strip()
            seen += line.startswith(token)
            yield seen, line
    with fastafile as handle:
        for record, lines in itertools.groupby(numbered(handle), key=lambda pair: pair[0]):
            if record == 0:
                continue
            header = next(lines)[1]
            sequence = "".join(line for _, line in lines)
            if header[1:]:
                yield (header[1:], sequence)


def make_blocklist(seqstring, block_size=80):
    """The sequence cut into block_size pieces (ref :148-157)."""
    return [seqstring[start:start + block_size] for start in range(0, len(seqstring), block_size)]


def slice_string_in_blocks(seqstring, block_size=80):
    return "\n".join(make_blocklist(seqstring, block_size)) + "\n"


def format_fasta(name, seq, block_size=80):
    return ">" + name + "\n" + slice_string_in_blocks(seq, block_size)


def simulate_reads(fastafile, readlength=100, outfile=sys.stdout):
    """Every readlength window of every sequence as a FASTA read named chrom_<1-based start> (ref :168-173)."""
    for name, seq in parse_fasta(fastafile):
        chrom = name.split()[0]
        for start in range(len(seq) - readlength + 1):
            outfile.write(format_fasta("{0}_{1}".format(chrom, start + 1), seq[start:start + readlength]))


class _TrackBuilder(object):
    """The state of the reference's loop (ref :181-211) -- the key it is filling, the position reached, the values so far -- and
    the loop itself, so that a stretch of lines can go through it from whatever state the stretch in front left."""

    def __init__(self, chromosome_sizes={}, new_values=list):
        self.tracks = Mappability(chromosome_sizes=chromosome_sizes)
        self.new_values = new_values
        self.current, self.position, self.values = None, 0, new_values()

    def flush(self):
        if self.current and self.values:
            self.tracks[self.current] = self.values

    def feed(self, lines):
        current, position, values = self.current, self.position, self.values
        try:
            for line in lines:
                name, _flag, chrom, pos, mapq = line.strip("\n").split()[:5]
                true_chrom = "_".join(name.split("_")[:-1])
                if current != true_chrom:
                    if current and values:
                        self.tracks[current] = values
                    current, position, values = chrom, 0, self.new_values()      # keyed by RNAME, as the reference does (:189)
                position += 1
                name_pos = int(name.split("_")[-1])
                if name_pos != position:
                    if not name_pos > position:
                        raise ValueError("Name is not sequential.  SAM must be in name sorted order Name: {0} Expected: "
                                         "{1}_{2}".format(name, current, position))
                    values.extend([0] * (name_pos - position))
                    position = name_pos
                values.append(1 if (true_chrom, name_pos) == (chrom, int(pos)) and mapq == "42" else 0)
        finally:
            self.current, self.position, self.values = current, position, values

    def finish(self):
        self.flush()
        return self.tracks


class _Track(object):
    """A track's values as the device route keeps them: `lead` implied zeros, then uint8 arrays copied out of the front end's
    page-locked buffer, then a list the host loop appends to (a window the device declined)."""
    __slots__ = ("lead", "chunks", "tail", "n")

    def __init__(self, lead=0):
        self.lead, self.chunks, self.tail, self.n = lead, [], [], lead

    def __len__(self):
        return self.n

    def append(self, value):
        self.tail.append(value)
        self.n += 1

    def extend(self, values):
        self.tail.extend(values)
        self.n += len(values)

    def add_chunk(self, array):
        self._seal()
        self.chunks.append(array)
        self.n += array.shape[0]

    def _seal(self):
        if self.tail:
            self.chunks.append(np.asarray(self.tail, dtype=np.uint8))
            self.tail = []

    def pieces(self, limit=1 << 22):
        """The values as uint8 arrays of at most `limit` entries."""
        self._seal()
        for start in range(0, self.lead, limit):
            yield np.zeros(min(limit, self.lead - start), dtype=np.uint8)
        for chunk in self.chunks:
            for start in range(0, chunk.shape[0], limit):
                yield chunk[start:start + limit]


def _write_tracks(tracks, outfile):
    """Mappability.to_wiggle for tracks that are lists or _Track: the text of a stretch of values is made in one piece (every
    value is 0 or 1: the two bytes '0' + v, '\\n' as one little-endian uint16)."""
    for chrom in sorted(tracks):
        outfile.write("fixedStep\tchrom={0}\tstart=1\tstep=1\n".format(chrom))
        values = tracks[chrom]
        pieces = values.pieces() if isinstance(values, _Track) else \
            (np.asarray(values[start:start + (1 << 22)], dtype=np.uint8) for start in range(0, len(values), 1 << 22))
        for piece in pieces:
            outfile.write((piece.astype("<u2") + np.uint16(0x0A30)).tobytes().decode("ascii"))


_BYTE_TRANSPARENT = ("utf8", "ascii", "usascii", "latin1", "iso88591")
last_run = {}                      # what the last on_device=True call did (_new_stats)


def _trusted_offset(samfile):
    """The byte offset of a text-mode handle on a regular file, when it can be trusted (the test of _ReadPairs.file_backed in
    xenomapper.py); else ValueError."""
    why = None
    name = getattr(samfile, "name", None)
    if not isinstance(samfile, io.TextIOWrapper) or not isinstance(name, str) or not os.path.isfile(name):
        why = "it is not a text-mode handle on a regular file"
    elif samfile.newlines not in (None, "\n"):
        why = "it has met line ends other than '\\n'"
    elif (samfile.encoding or "").lower().replace("-", "").replace("_", "") not in _BYTE_TRANSPARENT:
        why = "its encoding %r does not keep ASCII bytes as they are" % samfile.encoding
    else:
        try:
            offset = samfile.tell()
        except (OSError, ValueError):
            offset = -1
        if not 0 <= offset <= os.path.getsize(name):
            why = "its position is not a byte offset"
    if why:
        raise ValueError("on_device=True needs a text-mode handle on a regular file at a byte offset that can be trusted: " + why)
    return offset


_front_end = None


def _default_front_end():
    """The process-wide GPU front end of this step (xm_mapp) on the default context; its buffers are kept between calls."""
    global _front_end
    ctx = default_context()
    if _front_end is None or _front_end.ctx is not ctx or not _front_end._h:
        _front_end = _ffi.Mappability(ctx)
    return _front_end


def release_front_end():
    """Destroy the front end and with it its page-locked buffers (xenomapper.release_buffers calls this)."""
    global _front_end
    if _front_end is not None:
        _front_end.close()
        _front_end = None


def _window_bytes():
    kb = os.environ.get("XENOMAPPER_MAPP_WINDOW_KB")
    size = int(kb) << 10 if kb else int(os.environ.get("XENOMAPPER_WINDOW_MB", "128")) << 20
    return max(1, min(size, _ffi.MAPP_MAX_WINDOW))


def _limits(window):
    """(max_lines, max_values) of a window: a line of simulated reads is some hundred bytes and gives one value, so these are
    generous; a window beyond them is the host's (status 2 / 3), never wrong."""
    max_lines = window // 64 + 256
    return max_lines, min(_ffi.MAPP_MAX_WINDOW, 4 * max_lines + (1 << 20))


def _tracks_on_device(samfile, offset, chromosome_sizes, front_end, stats):
    """The tracks of the records behind byte `offset`, window by window through `front_end` (an _ffi.Mappability, or anything
    with its reserve / staging / run): segments the device resolved are walked here, a window it declined goes through
    _TrackBuilder.feed from the state the windows in front left -- one state for both: key, position and values."""
    builder = _TrackBuilder(chromosome_sizes, new_values=_Track)
    fd, size = samfile.fileno(), os.fstat(samfile.fileno()).st_size
    encoding, errors = samfile.encoding, samfile.errors
    window = _window_bytes()
    reserved = None
    while offset < size:
        if reserved != window:
            front_end.reserve(0, window, *_limits(window))
            staging, reserved = front_end.staging(0), window
        length = min(window, size - offset)
        got, t0 = 0, time.perf_counter()
        while got < length:
            k = os.preadv(fd, [memoryview(staging)[got:length]], offset + got)
            if k <= 0:
                raise OSError("%s: short read at byte %d" % (samfile.name, offset + got))
            got += k
        eof = offset + length >= size
        t1 = time.perf_counter()
        stats["s_read"] += t1 - t0
        block = None
        if builder.position <= 0xFFFFFFFF:                             # (a position the device's 32 bits do not hold: the host's)
            key = builder.current.encode(encoding) if builder.current is not None else None
            block = front_end.run(0, length, eof, key, builder.position)
            consumed = block.consumed
            stats["ms_upload"] += block.ms_upload
            stats["ms_kernels"] += block.ms_kernels
        else:
            consumed = length if eof else staging[:length].tobytes().rfind(b"\n") + 1
        if consumed == 0 and not eof:                                  # no line end in the window: twice the size
            if window >= _ffi.MAPP_MAX_WINDOW:
                raise ValueError("%s: a line longer than %d bytes at byte %d" % (samfile.name, window, offset))
            window = min(2 * window, _ffi.MAPP_MAX_WINDOW)
            continue
        t2 = time.perf_counter()
        stats["s_device"] += t2 - t1
        if block is not None and block.status == _ffi.MAPP_OK:
            stats["windows_device"] += 1
            stats["lines"] += block.n_lines
            for seg in block.segments:
                if seg["starts"]:
                    builder.flush()
                    key_at = int(seg["key_off"])
                    builder.current = staging[key_at:key_at + int(seg["key_len"])].tobytes().decode(encoding, errors)
                    builder.values = _Track(lead=int(seg["base"]))
                at, n = int(seg["value_off"]), int(seg["n_values"])
                builder.values.add_chunk(block.values[at:at + n].copy())
                builder.position = int(seg["last_pos"])
        else:
            stats["windows_host"] += 1
            if block is None:
                why = "position"
            elif block.status == _ffi.MAPP_DECLINED:
                why = _ffi.MAPP_REASONS[block.reason]
            else:
                why = {_ffi.MAPP_TOO_MANY_LINES: "too_many_lines", _ffi.MAPP_TOO_MANY_VALUES: "too_many_values"}[block.status]
            stats["reasons"][why] = stats["reasons"].get(why, 0) + 1
            # the window's lines as the handle would have given them: its encoding, its errors mode, universal newlines
            text = io.TextIOWrapper(io.BytesIO(staging[:consumed].tobytes()), encoding=encoding, errors=errors, newline=None)
            builder.feed(_counted(text, stats))
        stats["s_walk"] += time.perf_counter() - t2
        offset += consumed
    return builder.finish()


def _new_stats():
    """windows_device / windows_host: windows the device resolved / the host loop took, reasons: why (a count per reason), lines;
    ms_upload / ms_kernels: device time (HIP events); s_read / s_device / s_walk: wall time reading windows, inside xm_mapp_run
    (the window without a line end included) and walking segments or running the host loop."""
    return dict(windows_device=0, windows_host=0, reasons={}, lines=0, ms_upload=0.0, ms_kernels=0.0, s_read=0.0, s_device=0.0, s_walk=0.0)


def _counted(lines, stats):
    for line in lines:
        stats["lines"] += 1
        yield line


def single_end_mappability_from_sam(samfile, outfile=sys.stdout, fill_sequence_gaps=True, chromosome_sizes={}, on_device=False):
    """Single-end mappability wiggle from the name-sorted SAM of simulated reads: 1 where the read maps back to
    its origin with MAPQ 42 (ref :175-214).  on_device=True: the lines are indexed, parsed and resolved into tracks by the
    kernels of csrc/xm_mapp_kernels.h, window by window; needs a regular file and the GPU (no fallback), writes the same text."""
    global last_run
    if not on_device:
        builder = _TrackBuilder(chromosome_sizes)
        get_sam_header(samfile)
        builder.feed(samfile)
        builder.finish().to_wiggle(wigglefile=outfile)
        return
    _trusted_offset(samfile)
    front_end = _default_front_end()                       # RuntimeError naming gfx950 without a device
    get_sam_header(samfile)
    stats = _new_stats()
    last_run = stats
    tracks = _tracks_on_device(samfile, _trusted_offset(samfile), chromosome_sizes, front_end, stats)
    samfile.seek(0, os.SEEK_END)
    _write_tracks(tracks, outfile)


def paired_end_mappability(wiggle, mate_density, outfile=sys.stdout, chromosome_sizes={}):
    """Paired-end mappability wiggle from a single-end wiggle and a mate density (ref :216-235).  Only the chromosomes
    named in chromosome_sizes BEFORE the wiggle is read are written (all of them when it is empty): reading adds the
    wiggle's own chromosomes to that dictionary."""
    wanted = [*chromosome_sizes]
    single_end = Mappability(chromosome_sizes=chromosome_sizes)
    single_end.from_wiggle(wiggle, datatype=float)
    paired = single_end.single_end_to_paired(mate_density=mate_density)        # the GPU part
    paired.to_wiggle(wigglefile=outfile, chromosomes=wanted)


def smoothed_list(the_list, width=10):
    """Running mean over the window [x - width - 1, x + width) clipped at the front (ref :237-238); statistics.mean, i.e.
    the exactly rounded mean, as there."""
    out = []
    for x in range(len(the_list)):
        first = x - width - 1
        out.append(mean(the_list[first if first > 0 else 0:x + width]))
    return out


def normalised_list(the_list):
    """Every value divided by the sum of all (ref :240-242)."""
    scale = sum(the_list)
    return [value / scale for value in the_list]


def remove_small_values(the_list, relative_limit=0.1):
    """Values not above relative_limit * max become 0 (ref :244-253)."""
    floor = max(the_list) * relative_limit
    return [x if x > floor else 0 for x in the_list]


def mate_distribution_from_sam(samfile=sys.stdin, sample_size=10000):
    """Mate density from the |TLEN| of the first sample_size + 1 records with a non-zero TLEN (ref :255-273)."""
    sizes = []
    for line in samfile:
        if not line or line[0] == "@":
            continue
        insert_size = line.strip("\n").split()[8]
        if insert_size != "0":
            sizes.append(abs(int(insert_size)))
        if sample_size and len(sizes) > sample_size:
            break
    frequencies = Counter(sizes)
    histogram = [frequencies[i] if i in frequencies else 0 for i in range(0, max(sizes))]
    return normalised_list(remove_small_values(smoothed_list(histogram)))


def command_line_interface():
    parser = argparse.ArgumentParser(
        description="Caution: experimental.  Paired end mappability inferred from single end mappability: (1) --fasta "
                    "turns a genome into simulated reads, (2) map them, (3) --mapped_test_data turns the name sorted SAM "
                    "into a single end mappability wiggle, (4) --single_end_wiggle with --sam_for_sizes gives the paired "
                    "end wiggle.")
    parser.add_argument("--fasta", type=argparse.FileType("rt"), help="genome FASTA to cut into simulated reads (to stdout)")
    parser.add_argument("--readlength", type=int, default=100, help="the readlength to simulate")
    parser.add_argument("--mapped_test_data", type=argparse.FileType("rt"),
                        help="name sorted SAM of the mapped simulated reads; writes a fixed step wiggle to stdout")
    parser.add_argument("--single_end_wiggle", type=argparse.FileType("rt"), help="wiggle file of single end mappabilities")
    parser.add_argument("--sam_for_sizes", type=argparse.FileType("rt"), help="SAM file for the insert size distribution")
    parser.add_argument("--on_device", action="store_true",
                        help="with --mapped_test_data: read, parse and resolve the SAM on the GPU (a regular file; no fallback)")
    parser.add_argument("--version", action="store_true", help="print version information and exit")
    args = parser.parse_args()
    if args.version:
        print(__version__)
        sys.exit()
    if args.on_device and (not args.mapped_test_data or args.fasta or args.single_end_wiggle or args.sam_for_sizes):
        parser.error("--on_device goes with --mapped_test_data and no other step")
    if (not args.fasta) and (not args.mapped_test_data) and (not args.single_end_wiggle):
        print("ERROR: Insufficient arguments provided")
        parser.print_help()
        sys.exit(1)
    return args


def main(args=None):
    if not args:
        args = command_line_interface()
    out = sys.stdout                       # looked up now: the functions' defaults were bound when the module was imported
    if args.fasta:
        simulate_reads(fastafile=args.fasta, readlength=args.readlength, outfile=out)
    elif args.mapped_test_data:
        single_end_mappability_from_sam(samfile=args.mapped_test_data, outfile=out, on_device=getattr(args, "on_device", False))
    elif args.single_end_wiggle:
        if not args.sam_for_sizes:
            raise RuntimeError("You must provide a sam file to estimate the mate pair distance distribution")
        paired_end_mappability(wiggle=args.single_end_wiggle, mate_density=mate_distribution_from_sam(args.sam_for_sizes),
                               outfile=out)


if __name__ == "__main__":  # pragma: no cover
    main()
