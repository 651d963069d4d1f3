"""The direct check of a stripped pair of windows against the oracle -- not through another stripper: the oracle's restatement of
getReadPairs and of the three plugins on the same text gives the record count, the walk's outcome, the unit mask, every score the
stripper vouches for (and a flag exactly where the text justifies one) and the line spans.  A plain helper module (no tests, no
fixtures): tests/test_strip_gpu.py and tests/test_strip_fields_gpu.py run the device block through it, tests/
test_sam_field_shapes_cpu.py the host stripper's Block, which proves the checker itself against an implementation the CPU suite
pins already."""
import io
import re

import numpy as np

from tests.helpers import ORACLE, NEG

ABSENT = -2**31
LINE_NORMAL = 0x01                    # include/xenomapper_strip.h XMS_LINE_NORMAL: the line is '\t'.join(fields)


def unpack_cigar(cnt, ops):
    """Packed CIGAR columns -> the operations of every record (xenomapper_hip.h: a count byte of 255 means "255 or more", the
    record's operations are then followed by one trailer word n_ops << 4 | 15)."""
    out, pos = [], 0
    for c in cnt.tolist():
        n = c
        if c == 255:
            while not ((int(ops[pos + n]) & 15) == 15 and (int(ops[pos + n]) >> 4) == n):
                n += 1
        out.append([int(v) for v in ops[pos:pos + n]])
        pos += n + (1 if c == 255 else 0)
    return out


_PLAIN_INT = re.compile(r"^[+-]?[0-9]{1,10}$")


def plain_int32(text):
    return bool(_PLAIN_INT.match(text)) and int(text) <= 2**31 - 1 and int(text) >= -(2**31 - 1)


def flag_reason(fields, tag, score_mode):
    """Why the stripper may (and must) decline to vouch for column `tag` of this line, from the text alone -- None: it must
    deliver the value.  The plugins' rules (xenomapper.py:176-191, :193-206, :228-256): optional fields fields[11:] that CONTAIN
    the tag; two of them raise; the value is what follows the last ':'.  The kernels vouch for plain int32 literals only."""
    opt = fields[11:]
    if score_mode == 2 and tag == "AS":                               # get_cigarbased_AS_tag: NM (first match) + fields[5]
        nm = [x for x in opt if "NM" in x]
        if not nm:
            return None
        if len(fields) < 6:
            return "short"
        if not plain_int32(nm[0].split(":")[-1]):
            return "nonint"
        if any(int(n) >= 2**28 for n, _op in re.findall(r"([0-9]+)([MIDNSHPX=])", fields[5])):
            return "biglen"
        return None
    name = "ZS" if (score_mode == 1 and tag == "XS") else tag
    hits = [x for x in opt if name in x]
    if not hits:
        return None
    if len(hits) > 1:
        return "dup"
    return None if plain_int32(hits[0].split(":")[-1]) else "nonint"


def oracle_walk(t1, t2, skip):
    """ORACLE.read_pairs on two texts -> (pairs, None or "mismatch")."""
    pairs, err = [], None
    try:
        for pr in ORACLE.read_pairs(io.StringIO(t1, newline=None), io.StringIO(t2, newline=None), skip):
            pairs.append(pr)
    except AssertionError:
        err = "mismatch"
    return pairs, err


def cigar_of_block(block):
    """The host stripper's CSR columns -> [(nm, operations of every record)] per file."""
    out = []
    for nm, off, ops in block.csr:
        off = [int(v) for v in off]
        out.append((nm, [[int(v) for v in ops[off[k]:off[k + 1]]] for k in range(len(off) - 1)]))
    return out


def direct_check(got, b1, b2, score_mode, paired, skip, cigar=None):
    """`got`: the device's StrippedBlock or the host stripper's Block of the whole files b1, b2 (both at their end).  cigar:
    [(nm, operations of every record)] per file in CIGAR mode -- from unpack_cigar on the device's packed columns, or None for a
    Block, whose CSR columns are taken.  A field only one of the two result objects has (norm_len, line_flags: the device block) is
    checked where it is.  -> (pairs, err) of the oracle's walk."""
    t1, t2 = b1.decode("ascii"), b2.decode("ascii")
    pairs, err = oracle_walk(t1, t2, skip)
    assert got.n == len(pairs) and (got.mismatch_at >= 0) == (err == "mismatch")
    if err != "mismatch":
        assert got.ended
    names = [p[0][0] for p in pairs]
    cols = got.cols
    flags = np.unpackbits(np.ascontiguousarray(got.unit_bits).view(np.uint8), bitorder="little")[:got.n].tolist()
    assert flags == ([1] * len(pairs) if not paired else [int(i > 0 and names[i] == names[i - 1]) for i in range(len(names))])
    scorer = [ORACLE.tag_score, ORACLE.tag_score_zs, ORACLE.cigar_score][score_mode]
    exc = {(k, c) for k, c, _ in got.exc}
    if score_mode == 2 and got.n and cigar is None:
        cigar = cigar_of_block(got)
    norm_len, line_flags = getattr(got, "norm_len", None), getattr(got, "line_flags", None)
    raws = (b1, b2)
    for k, (f1, f2) in enumerate(pairs):
        for f, fields in enumerate((f1, f2)):
            st0 = int(got.line_off[f][k])
            line = raws[f][st0:st0 + int(got.line_len[f][k])].decode()
            assert line.split() == fields
            if norm_len is not None:
                assert int(norm_len[f][k]) == len("\t".join(fields))
            if line_flags is not None:
                assert bool(int(line_flags[f][k]) & LINE_NORMAL) == ("\t".join(fields) == line), (line, f, k)
            for c, tag in ((2 * f, "AS"), (2 * f + 1, "XS")):
                try:
                    want, failed = scorer(fields, tag=tag), False
                except Exception:
                    want, failed = None, True
                # a flag must be JUSTIFIED by the text, and a justified flag must be there (an over-flagging stripper -- which the
                # host path would quietly absorb by re-reading the line -- fails here)
                why = flag_reason(fields, tag, score_mode)
                assert ((k, c) in exc) == (why is not None), (fields, tag, why)
                if (k, c) in exc:
                    if why in ("dup", "short"):
                        assert failed, (fields, tag, why)               # the reference raises (ValueError :189-190 / IndexError)
                    continue
                assert not failed, (fields, tag)
                if score_mode == 2 and tag == "AS":
                    nm, ops = cigar[f][0][k], cigar[f][1][k]
                    have = NEG if nm == ABSENT else -6 * int(nm) - sum(
                        (5 + 3 * (v >> 4)) if (v & 15) in (1, 2) else (2 * (v >> 4) if (v & 15) == 4 else 0) for v in ops)
                else:
                    have = NEG if cols[c][k] == ABSENT else int(cols[c][k])
                assert have == want, (fields, tag, have, want)
    return pairs, err
