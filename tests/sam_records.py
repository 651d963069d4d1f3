"""SAM line -> BAM alignment record: a plain-Python model of the rule (SAM specification 4.2 as htslib's SAM parser applies it; the
native statement is xenomapper_amd/csrc/xm_samrec.h), a catalogue of lines at the edges of that rule, and a de-framer for streams of
BGZF members of stored blocks.  Shares no code with oracle/bam_oracle.py, which prints records back and is the other side of the
check.  Used by test_sam_records_cpu.py, test_samrec_core_host.py and test_sam_records_gpu.py."""
import re
import struct
import zlib

# reasons (XMH_ENC_* / XMS_ENC_*)
FIELDS, QNAME, FLAG, RNAME, POS, MAPQ, CIGAR, RNEXT, PNEXT, TLEN, SEQ, QUAL, AUX, AUX_RANGE, SIZE = range(1, 16)
HOST_FLOAT, HOST_LONG_CIGAR, HOST_SEQ_CODE, HOST_NUMBER = 32, 33, 34, 35

SEQ_TABLE = b"=ACMGRSVTWYHKDBN"
CIGAR_OPS = b"MIDNSHP=X"
_NUM = re.compile(rb"[+-]?[0-9]+\Z")
_CIG = re.compile(rb"([0-9]+)([MIDNSHP=X])")
_INT_TYPES = {"c": (-128, 127, "<b"), "C": (0, 255, "<B"), "s": (-32768, 32767, "<h"), "S": (0, 65535, "<H"),
              "i": (-2 ** 31, 2 ** 31 - 1, "<i"), "I": (0, 2 ** 32 - 1, "<I")}


class Declined(Exception):
    def __init__(self, reason):
        Exception.__init__(self, reason)
        self.reason = reason


def _number(text, bad, host):
    """value of [+-]?digits; not canonical ('+', a leading zero, '-0'): the host's"""
    if not _NUM.match(text):
        raise Declined(bad)
    digits = text.lstrip(b"+-")
    canonical = not text.startswith(b"+") and (digits == b"0" or not digits.startswith(b"0")) and text != b"-0"
    if not canonical and not host:
        raise Declined(HOST_NUMBER)
    return int(text)


def _ranged(text, lo, hi, bad, host):
    v = _number(text, bad, host)
    if not lo <= v <= hi:
        raise Declined(bad)
    return v


def reg2bin(beg, end):
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


def _float(text):
    try:
        if not text or text[:1] <= b" ":
            raise ValueError
        return struct.pack("<f", float(text.decode("ascii")))
    except (ValueError, OverflowError, UnicodeDecodeError):
        raise Declined(AUX)


def _nibble(c):
    u = bytes([c]).upper()
    return SEQ_TABLE.index(u) if u in SEQ_TABLE else 15


def _aux(field, host):
    if len(field) < 5 or field[2:3] != b":" or field[4:5] != b":" or not re.match(rb"[A-Za-z][A-Za-z0-9]\Z", field[:2]):
        raise Declined(AUX)
    tag, t, v = field[:2], chr(field[3]), field[5:]
    if t == "A":
        if len(v) != 1 or not 33 <= v[0] <= 126:
            raise Declined(AUX)
        return tag + b"A" + v
    if t == "i":
        x = _number(v, AUX, host)
        if not -2 ** 31 <= x <= 2 ** 32 - 1:
            raise Declined(AUX_RANGE)
        if x < 0:
            code = "c" if x >= -128 else "s" if x >= -32768 else "i"
        else:
            code = "C" if x <= 255 else "S" if x <= 65535 else "I"
        return tag + code.encode() + struct.pack(_INT_TYPES[code][2], x)
    if t == "f":
        if not host:
            raise Declined(HOST_FLOAT)
        return tag + b"f" + _float(v)
    if t == "Z":
        if any(c < 32 or c > 126 for c in v):
            raise Declined(AUX)
        return tag + b"Z" + v + b"\0"
    if t == "H":
        if len(v) % 2 or not re.match(rb"[0-9A-Fa-f]*\Z", v):
            raise Declined(AUX)
        return tag + b"H" + v + b"\0"
    if t == "B":
        if not v:
            raise Declined(AUX)
        sub = chr(v[0])
        if sub != "f" and sub not in _INT_TYPES:
            raise Declined(AUX)
        if sub == "f" and not host:
            raise Declined(HOST_FLOAT)
        rest = v[1:]
        out = tag + b"B" + v[:1] + struct.pack("<I", rest.count(b","))
        if rest and not rest.startswith(b","):
            raise Declined(AUX)
        for item in (rest[1:].split(b",") if rest else []):
            if sub == "f":
                out += _float(item)
            else:
                lo, hi, fmt = _INT_TYPES[sub]
                x = _number(item, AUX, host)
                if not lo <= x <= hi:
                    raise Declined(AUX_RANGE)
                out += struct.pack(fmt, x)
        return out
    raise Declined(AUX)


def encode(line, names, host=True, ref_shift=0):
    """line: bytes without terminator; names: list of bytes.  -> the record with its block_size word; raises Declined(reason)."""
    f = line.split(b"\t")
    if len(f) < 11:
        raise Declined(FIELDS)
    index = {n: k for k, n in enumerate(names)}
    if not 1 <= len(f[0]) <= 254:
        raise Declined(QNAME)
    flag = _ranged(f[1], 0, 65535, FLAG, host)
    if f[2] == b"*":
        ref_id = -1
    elif f[2] in index:
        ref_id = index[f[2]]
    else:
        raise Declined(RNAME)
    pos = _ranged(f[3], 0, 2 ** 31 - 1, POS, host)
    mapq = _ranged(f[4], 0, 255, MAPQ, host)
    ops = []
    if f[5] != b"*":
        found = _CIG.findall(f[5])
        if not f[5] or b"".join(a + b for a, b in found) != f[5]:
            raise Declined(CIGAR)
        for length, op in found:
            if int(length) >= 1 << 28:
                raise Declined(CIGAR)
            _number(length, CIGAR, host)
            ops.append((int(length), CIGAR_OPS.index(op)))
    if len(ops) > 65535 and not host:
        raise Declined(HOST_LONG_CIGAR)
    if f[6] == b"=":
        next_id = ref_id
    elif f[6] == b"*":
        next_id = -1
    elif f[6] in index:
        next_id = index[f[6]]
    else:
        raise Declined(RNEXT)
    pnext = _ranged(f[7], 0, 2 ** 31 - 1, PNEXT, host)
    tlen = _ranged(f[8], -2 ** 31, 2 ** 31 - 1, TLEN, host)
    if not f[9]:
        raise Declined(SEQ)
    seq = b"" if f[9] == b"*" else f[9]
    if any(c not in SEQ_TABLE for c in seq) and not host:
        raise Declined(HOST_SEQ_CODE)
    if f[10] == b"*":
        qual = b"\xff" * len(seq)
    else:
        if len(f[10]) != len(seq) or not seq or any(c < 33 or c > 126 for c in f[10]):
            raise Declined(QUAL)
        qual = bytes(c - 33 for c in f[10])
    ref_len = sum(n for n, op in ops if op in (0, 2, 3, 7, 8))
    span = ref_len if ref_len > 0 and not flag & 4 else 1
    nib = [_nibble(c) for c in seq]
    if len(nib) & 1:
        nib.append(0)
    packed = bytes((nib[k] << 4) | nib[k + 1] for k in range(0, len(nib), 2))
    long_cigar = len(ops) > 65535
    words = [(len(seq) << 4) | 4, ((ref_len << 4) | 3) & 0xFFFFFFFF] if long_cigar else [(n << 4) | op for n, op in ops]
    if ref_shift:
        ref_id += ref_shift if ref_id >= 0 else 0
        next_id += ref_shift if next_id >= 0 else 0
    body = struct.pack("<iiBBHHHIiii", ref_id, pos - 1, len(f[0]) + 1, mapq, reg2bin(pos - 1, pos - 1 + span) & 0xFFFF, len(words), flag,
                       len(seq), next_id, pnext - 1, tlen)
    body += f[0] + b"\0" + struct.pack("<%dI" % len(words), *words) + packed + qual
    for field in f[11:]:
        body += _aux(field, host)
    if long_cigar:
        body += b"CGBI" + struct.pack("<I", len(ops)) + struct.pack("<%dI" % len(ops), *[(n << 4) | op for n, op in ops])
    return struct.pack("<i", len(body)) + body


def try_encode(line, names, host=True, ref_shift=0):
    """-> (record, 0) or (None, reason)"""
    try:
        return encode(line, names, host, ref_shift), 0
    except Declined as e:
        return None, e.reason


def split_records(blob):
    """records (without their block_size words) of a payload"""
    out, p = [], 0
    while p < len(blob):
        size, = struct.unpack_from("<i", blob, p)
        assert size >= 32 and p + 4 + size <= len(blob), (p, size, len(blob))
        out.append(blob[p + 4:p + 4 + size])
        p += 4 + size
    return out


def deframe(stream, block_payload=65280):
    """Payload of a range of BGZF members of stored blocks; every member checked: the 18 header bytes and BSIZE, 01 LEN NLEN,
    CRC-32, ISIZE; every member but the last holds exactly block_payload bytes.  -> (payload, members)"""
    stream = bytes(stream)
    out, p, members = [], 0, 0
    while p < len(stream):
        assert len(stream) - p >= 31, "a member is cut short"
        head = stream[p:p + 18]
        assert head[:16] == bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 66, 67, 2, 0]), head
        bsize, = struct.unpack_from("<H", head, 16)
        assert stream[p + 18] == 1
        ln, nln = struct.unpack_from("<HH", stream, p + 19)
        assert ln ^ nln == 0xFFFF and bsize + 1 == ln + 31 and 1 <= ln <= block_payload, (bsize, ln, nln)
        data = stream[p + 23:p + 23 + ln]
        assert len(data) == ln
        crc, isize = struct.unpack_from("<II", stream, p + 23 + ln)
        assert crc == zlib.crc32(data) and isize == ln, (members, crc, isize)
        out.append(data)
        p += ln + 31
        members += 1
        assert ln == block_payload or p == len(stream), "only a range's last member may be short"
    return b"".join(out), members


# ---- the catalogue ---------------------------------------------------------------------------------------------------------------
REFS = [b"chr%d" % k for k in range(1, 23)] + [b"chrX", b"chrY", b"chrM"] + [b"contig_%05d|len=%d" % (k, 1000 + 7 * k) for k in range(4975)]
assert len(REFS) == 5000
FIRST, LAST = REFS[0], REFS[-1]


def _bases(n, k=0):
    return bytes(b"ACGTNACCGGTTAAGCTMRSVWYHKDB="[(k + 3 * j) % 28] for j in range(n))


def _quals(n, k=0):
    return bytes(33 + (k + 7 * j) % 94 for j in range(n))


def make(qname=b"r", flag=0, rname=FIRST, pos=100, mapq=30, cigar=None, rnext=b"=", pnext=200, tlen=-50, seq=None, qual=None, aux=(), l_seq=10):
    seq = _bases(l_seq) if seq is None else seq
    qual = (_quals(len(seq)) if seq != b"*" else b"*") if qual is None else qual
    if cigar is None:
        cigar = b"%dM" % len(seq) if seq != b"*" else b"*"
    fields = [qname, b"%d" % flag if isinstance(flag, int) else flag, rname, b"%d" % pos if isinstance(pos, int) else pos,
              b"%d" % mapq if isinstance(mapq, int) else mapq, cigar, rnext, b"%d" % pnext if isinstance(pnext, int) else pnext,
              b"%d" % tlen if isinstance(tlen, int) else tlen, seq, qual] + list(aux)
    return b"\t".join(fields)


def _cigar_of(n_ops):
    return b"".join(b"1M1I" for _ in range(n_ops // 2)) + (b"1M" if n_ops & 1 else b"")


def catalogue():
    """[(name, line, device reason, host reason)]: 0 = encoded.  The smallest shapes at which the encoder can go wrong; the step widths
    of the device kernels (64 QUAL bytes and 128 bases per wave step in E2, 16 bytes per lane in F) are among the lengths."""
    c = []

    def add(name, line, dev=0, host=0):
        c.append((name, line, dev, host))
    for n in (1, 2, 254):
        add("qname%d" % n, make(qname=b"q" * n))
    add("qname255", make(qname=b"q" * 255), QNAME, QNAME)
    for n in (1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025):
        add("lseq%d" % n, make(l_seq=n, qname=b"s%d" % n))
        add("lseq%d_noqual" % n, make(l_seq=n, qual=b"*"))
    add("lseq0", make(seq=b"*", qual=b"*"))
    add("lseq0_cigar", make(seq=b"*", qual=b"*", cigar=b"5M"))
    add("cigar_star", make(cigar=b"*"))
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 65535):
        add("cigar%d" % n, make(cigar=_cigar_of(n), l_seq=5))
    add("cigar65536", make(cigar=_cigar_of(65536), l_seq=5), HOST_LONG_CIGAR, 0)
    add("cigar_len1", make(cigar=b"1M"))
    add("cigar_len_max", make(cigar=b"%dN" % (2 ** 28 - 1)))
    add("cigar_len_over", make(cigar=b"%dN" % 2 ** 28), CIGAR, CIGAR)
    add("cigar_all_ops", make(cigar=b"1M2I3D4N5S6H7P8=9X"))
    add("cigar_zero_len", make(cigar=b"0M10S"))
    for bad in (b"M", b"10", b"10Q", b"1M1", b"-1M", b"1M 2I"):
        add("cigar_bad_%s" % bad.decode(), make(cigar=bad), CIGAR, CIGAR)
    add("cigar_leading_zero", make(cigar=b"010M"), HOST_NUMBER, 0)
    # optional fields
    add("aux_A", make(aux=[b"XA:A:!", b"XB:A:~", b"XC:A:Q"]))
    add("aux_A_two", make(aux=[b"XA:A:ab"]), AUX, AUX)
    add("aux_A_empty", make(aux=[b"XA:A:"]), AUX, AUX)
    for v in (-2 ** 31, -32769, -32768, -129, -128, -1, 0, 255, 256, 65535, 65536, 2 ** 32 - 1):
        add("aux_i_%d" % v, make(aux=[b"NM:i:%d" % v]))
    add("aux_i_below", make(aux=[b"NM:i:%d" % (-2 ** 31 - 1)]), AUX_RANGE, AUX_RANGE)
    add("aux_i_above", make(aux=[b"NM:i:%d" % 2 ** 32]), AUX_RANGE, AUX_RANGE)
    add("aux_i_plus", make(aux=[b"NM:i:+5"]), HOST_NUMBER, 0)
    add("aux_i_zeros", make(aux=[b"NM:i:007"]), HOST_NUMBER, 0)
    add("aux_i_minus_zero", make(aux=[b"NM:i:-0"]), HOST_NUMBER, 0)
    add("aux_i_empty", make(aux=[b"NM:i:"]), AUX, AUX)
    add("aux_i_text", make(aux=[b"NM:i:1e3"]), AUX, AUX)
    for n in (0, 1, 15, 16, 17, 200):
        add("aux_Z%d" % n, make(aux=[b"RG:Z:" + bytes(33 + (5 * j) % 94 for j in range(n)), b"NM:i:1"]))
    add("aux_Z_ctrl", make(aux=[b"RG:Z:a\x01b"]), AUX, AUX)
    add("aux_H", make(aux=[b"XH:H:", b"YH:H:1AE301", b"ZH:H:ff00"]))
    add("aux_H_odd", make(aux=[b"XH:H:1AE"]), AUX, AUX)
    add("aux_H_bad", make(aux=[b"XH:H:1G"]), AUX, AUX)
    for sub, (lo, hi, _) in sorted(_INT_TYPES.items()):
        for n in (0, 1, 63, 64, 65):
            vals = [(lo, hi, 0, lo + 1, hi - 1)[j % 5] for j in range(n)]
            add("aux_B%s%d" % (sub, n), make(aux=[b"XB:B:" + sub.encode() + b"".join(b",%d" % v for v in vals), b"NM:i:3"]))
        add("aux_B%s_below" % sub, make(aux=[b"XB:B:%s,%d" % (sub.encode(), lo - 1)]), AUX_RANGE, AUX_RANGE)
        add("aux_B%s_above" % sub, make(aux=[b"XB:B:%s,%d" % (sub.encode(), hi + 1)]), AUX_RANGE, AUX_RANGE)
    add("aux_B_empty_item", make(aux=[b"XB:B:c,1,,2"]), AUX, AUX)
    add("aux_B_trailing_comma", make(aux=[b"XB:B:c,1,"]), AUX, AUX)
    add("aux_B_no_subtype", make(aux=[b"XB:B:"]), AUX, AUX)
    add("aux_B_bad_subtype", make(aux=[b"XB:B:d,1"]), AUX, AUX)
    add("aux_B_no_comma", make(aux=[b"XB:B:c1"]), AUX, AUX)
    add("aux_f", make(aux=[b"XF:f:1.5"]), HOST_FLOAT, 0)
    add("aux_Bf", make(aux=[b"XF:B:f,0.25,-3"]), HOST_FLOAT, 0)
    add("aux_f_bad", make(aux=[b"XF:f:abc"]), HOST_FLOAT, AUX)
    add("aux_short", make(aux=[b"XF:i"]), AUX, AUX)
    add("aux_tag_digit_first", make(aux=[b"1F:i:1"]), AUX, AUX)
    add("aux_unknown_type", make(aux=[b"XF:d:1.5"]), AUX, AUX)
    for n in (0, 1, 62, 63, 64, 65):                    # (62: 63 fields once the GPU test has added the tag that decides the bin)
        add("aux_fields%d" % n, make(aux=[b"%c%c:i:%d" % (65 + j // 26, 97 + j % 26, j * 37) for j in range(n)]))
    # positions and bins
    for pos in (0, 1, 2 ** 31 - 1):
        add("pos%d" % pos, make(pos=pos, pnext=pos))
    add("pos_over", make(pos=2 ** 31), POS, POS)
    add("pnext_over", make(pnext=2 ** 31), PNEXT, PNEXT)
    add("pos_negative", make(pos=b"-1"), POS, POS)
    for level in (14, 17, 20, 23, 26):
        edge = 1 << level
        for flag in (0, 4):
            add("bin_edge%d_below_f%d" % (level, flag), make(pos=edge - 9, flag=flag, l_seq=10))       # pos0 + 10 == edge: inside
            add("bin_edge%d_across_f%d" % (level, flag), make(pos=edge - 8, flag=flag, l_seq=10))      # one base over the edge
            add("bin_edge%d_above_f%d" % (level, flag), make(pos=edge + 1, flag=flag, l_seq=10))
    add("rname_star", make(rname=b"*", rnext=b"*", pos=0, pnext=0))
    add("rname_last", make(rname=LAST))
    add("rname_unknown", make(rname=b"chr99"), RNAME, RNAME)
    add("rname_prefix", make(rname=FIRST[:-1]), RNAME, RNAME)
    add("rnext_eq_star", make(rname=b"*", rnext=b"="))
    add("rnext_star", make(rnext=b"*"))
    add("rnext_name", make(rnext=REFS[24]))
    add("rnext_same_name", make(rname=REFS[24], rnext=REFS[24]), 0, 0)
    add("rnext_unknown", make(rnext=b"nowhere"), RNEXT, RNEXT)
    for k in range(25, 5000, 331):
        add("ref%d" % k, make(rname=REFS[k], rnext=REFS[4999 - k]))
    # the core fields' ranges
    add("flag_max", make(flag=65535))
    add("flag_over", make(flag=65536), FLAG, FLAG)
    add("flag_text", make(flag=b"0x10"), FLAG, FLAG)
    add("flag_plus", make(flag=b"+16"), HOST_NUMBER, 0)
    add("mapq_max", make(mapq=255))
    add("mapq_over", make(mapq=256), MAPQ, MAPQ)
    add("tlen_min", make(tlen=-2 ** 31))
    add("tlen_max", make(tlen=2 ** 31 - 1))
    add("tlen_over", make(tlen=2 ** 31), TLEN, TLEN)
    add("tlen_under", make(tlen=-2 ** 31 - 1), TLEN, TLEN)
    add("tlen_zeros", make(tlen=b"00"), HOST_NUMBER, 0)
    add("ten_fields", b"\t".join(make().split(b"\t")[:10]), FIELDS, FIELDS)
    add("one_field", b"lonely", FIELDS, FIELDS)
    # SEQ and QUAL
    add("seq_all_codes", make(seq=SEQ_TABLE))
    add("seq_lower", make(seq=b"acgtn"), HOST_SEQ_CODE, 0)
    add("seq_other", make(seq=b"AC.GU"), HOST_SEQ_CODE, 0)
    add("qual_short", make(seq=b"ACGT", qual=b"III"), QUAL, QUAL)
    add("qual_long", make(seq=b"ACGT", qual=b"IIIII"), QUAL, QUAL)
    add("qual_without_seq", make(seq=b"*", qual=b"II"), QUAL, QUAL)
    add("qual_space", make(seq=b"ACGT", qual=b"II I"), QUAL, QUAL)
    add("qual_star_one_base", make(seq=b"A", qual=b"*"))
    add("qual_edges", make(seq=b"ACGT", qual=b"!~!~"))
    return c


def printable(entry):
    """device-eligible and printed back as itself.  Two spellings of RNEXT give the record of another spelling, as in htslib, and
    print back as that one: the name RNAME has (the record of '='), and '=' beside RNAME '*' (the record of '*')."""
    return entry[2] == 0 and entry[0] not in ("rnext_same_name", "rnext_eq_star")
