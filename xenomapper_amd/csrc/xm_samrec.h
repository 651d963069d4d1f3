// xm_samrec.h -- ONE SAM line -> ONE BAM alignment record (SAM specification 4.2), the rule htslib's SAM parser applies to a line whose
// fields are separated by single tabs.  One source for the device (xm_strip.hip: E1 sizes, E2 writes) and the host (xm_samenc.cpp:
// xmh_sam_encode; tests/samrec_core_host.cpp under ASan + UBSan), as xm_bamrec.h, xm_fmtg.h and xm_deflate_core.h are.
//
// Two steps.  size_of() reads the whole line, checks every field against the grammar and returns the record's size (its block_size
// word included) or the reason why the line is declined; write() writes the record of a line size_of() accepted.  No allocation, no
// I/O; every loop is bounded by the line's length, every store by the size step 1 returned (Sink::put).
//
// READ MARGIN: 0.  Both steps read line[0, n) and nothing behind it (every access is an index below a field's end, and a field ends
// at a tab or at n).  The strip buffers' 64 spare bytes are not needed by this header.
//
// HOST = false is what the device encodes.  Four forms are left to the host (HOST = true; the device declines them with a reason of
// their own, ENC_HOST_*): binary32 fields (f, B:f -- strtof), a CIGAR of more than 65535 operations (4.2.2: "<l_seq>S<L>N" and a
// CG:B:I field behind the others), SEQ bytes outside the 16 upper-case codes (a lower-case letter of the table takes the upper-case
// code, anything else 15), and numbers that are not canonical (a '+', a leading zero, "-0": their value is taken).  Everything else
// outside the grammar is an error on both sides: declined with its reason, never guessed.
//
// Invariant (tests/test_sam_records_cpu.py): for every line HOST = false encodes, printing the record gives the line back -- but for
// two spellings of RNEXT whose record is another spelling's, as in htslib: RNAME's own name (the record of '=') and '=' beside an
// RNAME of '*' (the record of '*').
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define XSR_HD __host__ __device__ inline
#else
#define XSR_HD inline
#endif
#include <stdlib.h>
#include <vector>

namespace xmsam {

// why a line is declined (XMS_ENC_* of xenomapper_strip.h, XMH_ENC_* of xenomapper_host.h)
enum : int32_t {
    ENC_OK = 0,
    ENC_FIELDS = 1,        // fewer than 11 fields
    ENC_QNAME = 2,         // not 1 - 254 bytes
    ENC_FLAG = 3,          // not a number in 0 - 65535
    ENC_RNAME = 4,         // not '*' and not a name of the reference list
    ENC_POS = 5,           // not a number in 0 - 2^31 - 1
    ENC_MAPQ = 6,          // not a number in 0 - 255
    ENC_CIGAR = 7,         // not '*' and not (digits op)+ with every length below 2^28
    ENC_RNEXT = 8,         // not '*', '=' or a name of the reference list
    ENC_PNEXT = 9,
    ENC_TLEN = 10,         // not a number inside int32
    ENC_SEQ = 11,          // empty
    ENC_QUAL = 12,         // not '*' and not l_seq bytes in '!' - '~'
    ENC_AUX = 13,          // an optional field that is not TG:T:V of a known type
    ENC_AUX_RANGE = 14,    // a value outside its type's range
    ENC_SIZE = 15,         // the record would not fit block_size (int32)
    ENC_HOST_FLOAT = 32,   // the host-only forms
    ENC_HOST_LONG_CIGAR = 33,
    ENC_HOST_SEQ_CODE = 34,
    ENC_HOST_NUMBER = 35
};

constexpr uint32_t READ_MARGIN = 0;                    // bytes either step may read behind line[n - 1]
constexpr uint32_t MAX_CIGAR_OPS = 65535u;

// ---- the reference list as an open-addressed table: entry s = {hash, index + 1} (0: empty), load factor at most 1/2 ------------------
struct RefHash {
    const uint8_t *names;                              // the names back to back
    const uint32_t *at;                                // n_refs + 1 positions
    const uint32_t *table;                             // 2 * (mask + 1) words
    uint32_t mask, n_refs;

    static XSR_HD uint32_t hash(const uint8_t *p, uint32_t len)                    // FNV-1a
    {
        uint32_t h = 2166136261u;
        for (uint32_t k = 0; k < len; ++k) h = (h ^ p[k]) * 16777619u;
        return h;
    }
    // the index of the name p[0, len) or -1: at most table-size probes, the whole name compared before it is accepted
    XSR_HD int32_t find(const uint8_t *p, uint32_t len) const
    {
        if (n_refs == 0u) return -1;
        const uint32_t h = hash(p, len);
        uint32_t s = h & mask;
        for (uint32_t step = 0; step <= mask; ++step, s = (s + 1u) & mask) {
            const uint32_t idx1 = table[2u * s + 1u];
            if (idx1 == 0u) return -1;
            if (table[2u * s] != h || idx1 > n_refs) continue;
            const uint32_t a = at[idx1 - 1u];
            if (at[idx1] - a != len) continue;
            uint32_t k = 0;
            while (k < len && names[a + k] == p[k]) ++k;
            if (k == len) return (int32_t)(idx1 - 1u);
        }
        return -1;
    }
};

// the table of a list (host); false: a name occurs twice
inline bool build_ref_table(const uint8_t *names, const uint32_t *at, uint32_t n_refs, std::vector<uint32_t> &table, uint32_t &mask)
{
    uint64_t size = 2;
    while (size < 2ull * n_refs) size <<= 1;
    mask = (uint32_t)(size - 1u);
    table.assign((size_t)size * 2u, 0u);
    for (uint32_t i = 0; i < n_refs; ++i) {
        const uint32_t len = at[i + 1u] - at[i], h = RefHash::hash(names + at[i], len);
        const RefHash so_far{names, at, table.data(), mask, n_refs};
        if (so_far.find(names + at[i], len) >= 0) return false;
        uint32_t s = h & mask;
        while (table[2u * s + 1u] != 0u) s = (s + 1u) & mask;
        table[2u * s] = h;
        table[2u * s + 1u] = i + 1u;
    }
    return true;
}

// ---- small pieces ---------------------------------------------------------------------------------------------------------------
struct Num { uint64_t mag; bool neg, ok, canon; };     // ok: [+-]?digits+; canon: no '+', no leading zero but "0", not "-0"

XSR_HD Num number(const uint8_t *p, uint32_t b, uint32_t e)
{
    Num r{0, false, false, true};
    uint32_t i = b;
    if (i < e && (p[i] == '-' || p[i] == '+')) { r.neg = p[i] == '-'; r.canon = r.neg; ++i; }
    if (i >= e) return r;
    if (p[i] == '0' && e - i > 1u) r.canon = false;
    for (; i < e; ++i) {
        const uint32_t c = p[i];
        if (c < '0' || c > '9') return r;
        if (r.mag < (1ull << 40)) r.mag = r.mag * 10u + (uint64_t)(c - '0');        // (saturates above every range asked about)
    }
    if (r.neg && r.mag == 0u) r.canon = false;
    r.ok = true;
    return r;
}

XSR_HD int64_t value_of(const Num &v) { return v.neg ? -(int64_t)v.mag : (int64_t)v.mag; }

// the specification's 5.3 reg2bin on signed 64-bit values (arithmetic shifts: POS 0 is beg -1, bin 4680)
XSR_HD uint32_t reg2bin(int64_t beg, int64_t end)
{
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0u;
}

XSR_HD int cigar_code(uint32_t c)
{
    switch (c) {
    case 'M': return 0; case 'I': return 1; case 'D': return 2; case 'N': return 3; case 'S': return 4;
    case 'H': return 5; case 'P': return 6; case '=': return 7; case 'X': return 8; default: return -1;
    }
}

// "=ACMGRSVTWYHKDBN": 0 - 15 an upper-case code; 16 + code a lower-case letter of the table; 255 anything else
XSR_HD uint32_t seq_code(uint32_t c)
{
    switch (c) {
    case '=': return 0; case 'A': return 1; case 'C': return 2; case 'M': return 3; case 'G': return 4; case 'R': return 5;
    case 'S': return 6; case 'V': return 7; case 'T': return 8; case 'W': return 9; case 'Y': return 10; case 'H': return 11;
    case 'K': return 12; case 'D': return 13; case 'B': return 14; case 'N': return 15;
    case 'a': return 17; case 'c': return 18; case 'm': return 19; case 'g': return 20; case 'r': return 21;
    case 's': return 22; case 'v': return 23; case 't': return 24; case 'w': return 25; case 'y': return 26; case 'h': return 27;
    case 'k': return 28; case 'd': return 29; case 'b': return 30; case 'n': return 31;
    default: return 255;
    }
}
XSR_HD uint32_t seq_nibble(uint32_t c) { const uint32_t k = seq_code(c); return k == 255u ? 15u : (k & 15u); }

// SEQ and QUAL are most of a record and every output byte depends on one or two input bytes only: output bytes first, first + step,
// ... (the host: 0, 1; the device: a lane each, 64 apart)
XSR_HD void pack_seq(const uint8_t *seq, uint32_t l_seq, uint8_t *dst, uint32_t first, uint32_t step)
{
    for (uint32_t j = first; j < (l_seq + 1u) / 2u; j += step) {
        const uint32_t hi = seq_nibble(seq[2u * j]), lo = 2u * j + 1u < l_seq ? seq_nibble(seq[2u * j + 1u]) : 0u;
        dst[j] = (uint8_t)((hi << 4) | lo);
    }
}
XSR_HD void pack_qual(const uint8_t *qual, uint32_t l_seq, uint8_t *dst, uint32_t first, uint32_t step)    // qual == nullptr: '*'
{
    for (uint32_t j = first; j < l_seq; j += step) dst[j] = qual ? (uint8_t)(qual[j] - 33u) : (uint8_t)0xFFu;
}

struct Sized { uint32_t size; int32_t reason; uint32_t seq_off, l_seq; };   // step 1: size with the block_size word (0 when declined)
struct Bulk { uint32_t seq_src, l_seq, seq_dst, qual_src, qual_dst; };      // write(): where SEQ / QUAL lie (qual_src ~0u: '*')

struct Sink {                                          // counts, and stores below `cap` only
    uint8_t *out;
    uint64_t cap, at;
    XSR_HD void put8(uint32_t v) { if (out && at < cap) out[at] = (uint8_t)v; ++at; }
    XSR_HD void put16(uint32_t v) { put8(v); put8(v >> 8); }
    XSR_HD void put32(uint32_t v) { put16(v); put16(v >> 16); }
    XSR_HD void poke32(uint64_t where, uint32_t v)
    {
        for (uint32_t k = 0; k < 4u; ++k)
            if (out && where + k < cap) out[where + k] = (uint8_t)(v >> (8u * k));
    }
};

inline bool host_float(const uint8_t *p, uint32_t b, uint32_t e, uint32_t &bits)
{
    char buf[64];
    const uint32_t len = e - b;
    if (len == 0u || len >= sizeof buf || p[b] <= ' ') return false;
    for (uint32_t k = 0; k < len; ++k) buf[k] = (char)p[b + k];
    buf[len] = 0;
    char *end = nullptr;
    const float f = strtof(buf, &end);
    if (end != buf + len) return false;
    __builtin_memcpy(&bits, &f, 4);
    return true;
}

template <bool HOST> XSR_HD bool float_bits(const uint8_t *p, uint32_t b, uint32_t e, uint32_t &bits)
{
#if defined(__HIP_DEVICE_COMPILE__)
    (void)p; (void)b; (void)e; (void)bits;
    return false;
#else
    if (!HOST) return false;
    return host_float(p, b, e, bits);
#endif
}

// range of a B subtype / the stored type of an 'i' value
XSR_HD bool int_range(uint32_t t, int64_t &lo, int64_t &hi, uint32_t &bytes)
{
    switch (t) {
    case 'c': lo = -128; hi = 127; bytes = 1; return true;
    case 'C': lo = 0; hi = 255; bytes = 1; return true;
    case 's': lo = -32768; hi = 32767; bytes = 2; return true;
    case 'S': lo = 0; hi = 65535; bytes = 2; return true;
    case 'i': lo = -2147483648ll; hi = 2147483647ll; bytes = 4; return true;
    case 'I': lo = 0; hi = 4294967295ll; bytes = 4; return true;
    default: return false;
    }
}

XSR_HD uint32_t next_tab(const uint8_t *line, uint32_t from, uint32_t n)
{
    while (from < n && line[from] != '\t') ++from;
    return from;
}

// one optional field line[b, e) into the sink
template <bool HOST> XSR_HD int32_t aux_field(const uint8_t *line, uint32_t b, uint32_t e, Sink &o)
{
    if (e - b < 5u || line[b + 2u] != ':' || line[b + 4u] != ':') return ENC_AUX;
    const uint32_t t0 = line[b], t1 = line[b + 1u], type = line[b + 3u], v = b + 5u;
    const bool alpha0 = (t0 >= 'A' && t0 <= 'Z') || (t0 >= 'a' && t0 <= 'z');
    const bool alnum1 = (t1 >= 'A' && t1 <= 'Z') || (t1 >= 'a' && t1 <= 'z') || (t1 >= '0' && t1 <= '9');
    if (!alpha0 || !alnum1) return ENC_AUX;
    o.put8(t0); o.put8(t1);
    switch (type) {
    case 'A':
        if (e - v != 1u || line[v] < '!' || line[v] > '~') return ENC_AUX;
        o.put8('A'); o.put8(line[v]);
        return ENC_OK;
    case 'i': {
        const Num x = number(line, v, e);
        if (!x.ok) return ENC_AUX;
        if (!HOST && !x.canon) return ENC_HOST_NUMBER;
        const int64_t val = value_of(x);
        if (val < -2147483648ll || val > 4294967295ll) return ENC_AUX_RANGE;
        if (val < 0) {
            if (val >= -128) { o.put8('c'); o.put8((uint32_t)val); }
            else if (val >= -32768) { o.put8('s'); o.put16((uint32_t)val); }
            else { o.put8('i'); o.put32((uint32_t)val); }
        } else {
            if (val <= 255) { o.put8('C'); o.put8((uint32_t)val); }
            else if (val <= 65535) { o.put8('S'); o.put16((uint32_t)val); }
            else { o.put8('I'); o.put32((uint32_t)val); }
        }
        return ENC_OK;
    }
    case 'f': {
        if (!HOST) return ENC_HOST_FLOAT;
        uint32_t bits = 0;
        if (!float_bits<HOST>(line, v, e, bits)) return ENC_AUX;
        o.put8('f'); o.put32(bits);
        return ENC_OK;
    }
    case 'Z':
        o.put8('Z');
        for (uint32_t k = v; k < e; ++k) {
            if (line[k] < ' ' || line[k] > '~') return ENC_AUX;
            o.put8(line[k]);
        }
        o.put8(0);
        return ENC_OK;
    case 'H':
        if ((e - v) & 1u) return ENC_AUX;
        o.put8('H');
        for (uint32_t k = v; k < e; ++k) {
            const uint32_t c = line[k];
            if (!((c >= '0' && c <= '9') || (c >= 'A' && c <= 'F') || (c >= 'a' && c <= 'f'))) return ENC_AUX;
            o.put8(c);
        }
        o.put8(0);
        return ENC_OK;
    case 'B': {
        if (v >= e) return ENC_AUX;
        const uint32_t sub = line[v];
        int64_t lo = 0, hi = 0;
        uint32_t bytes = 0;
        const bool is_float = sub == 'f';
        if (!is_float && !int_range(sub, lo, hi, bytes)) return ENC_AUX;
        if (is_float && !HOST) return ENC_HOST_FLOAT;
        uint32_t count = 0;
        for (uint32_t k = v + 1u; k < e; ++k) count += line[k] == ',' ? 1u : 0u;
        o.put8('B'); o.put8(sub); o.put32(count);
        uint32_t p = v + 1u;
        while (p < e) {
            if (line[p] != ',') return ENC_AUX;
            uint32_t q = p + 1u;
            while (q < e && line[q] != ',') ++q;
            if (is_float) {
                uint32_t bits = 0;
                if (!float_bits<HOST>(line, p + 1u, q, bits)) return ENC_AUX;
                o.put32(bits);
            } else {
                const Num x = number(line, p + 1u, q);
                if (!x.ok) return ENC_AUX;
                if (!HOST && !x.canon) return ENC_HOST_NUMBER;
                const int64_t val = value_of(x);
                if (val < lo || val > hi) return ENC_AUX_RANGE;
                if (bytes == 1u) o.put8((uint32_t)val); else if (bytes == 2u) o.put16((uint32_t)val); else o.put32((uint32_t)val);
            }
            p = q;
        }
        return ENC_OK;
    }
    default:
        return ENC_AUX;
    }
}

// The whole rule.  o.out == nullptr: step 1 (SEQ and QUAL are read and checked; sz.seq_off / l_seq are set).  Otherwise step 2 of a
// line step 1 accepted: SEQ and QUAL are found through sz, and left to the caller (bulk != nullptr) or packed here.
template <bool HOST, class Refs>
XSR_HD int32_t run(const uint8_t *line, uint32_t n, const Refs &refs, int32_t ref_shift, Sized &sz, Sink &o, Bulk *bulk)
{
    const bool writing = o.out != nullptr;
    uint32_t fb[9], fe[9];                             // fields 0 - 8
    uint32_t pos = 0;
    for (uint32_t k = 0; k < 9u; ++k) {
        if (pos > n) return ENC_FIELDS;
        fb[k] = pos;
        fe[k] = next_tab(line, pos, n);
        pos = fe[k] + 1u;
    }
    if (pos > n) return ENC_FIELDS;
    if (!writing && next_tab(line, pos, n) >= n) return ENC_FIELDS;                // no QUAL behind SEQ: ten fields
    const uint32_t l_name = fe[0] - fb[0];
    if (l_name < 1u || l_name > 254u) return ENC_QNAME;
    const Num flag = number(line, fb[1], fe[1]);
    if (!flag.ok) return ENC_FLAG;
    if (!HOST && !flag.canon) return ENC_HOST_NUMBER;
    if (flag.neg ? flag.mag != 0u : flag.mag > 65535u) return ENC_FLAG;
    int32_t ref_id = -1;
    if (fe[2] == fb[2]) return ENC_RNAME;
    if (!(fe[2] - fb[2] == 1u && line[fb[2]] == '*')) {
        ref_id = refs.find(line + fb[2], fe[2] - fb[2]);
        if (ref_id < 0) return ENC_RNAME;
    }
    const Num p1 = number(line, fb[3], fe[3]);
    if (!p1.ok) return ENC_POS;
    if (!HOST && !p1.canon) return ENC_HOST_NUMBER;
    if (p1.neg ? p1.mag != 0u : p1.mag > 2147483647ull) return ENC_POS;
    const Num mapq = number(line, fb[4], fe[4]);
    if (!mapq.ok) return ENC_MAPQ;
    if (!HOST && !mapq.canon) return ENC_HOST_NUMBER;
    if (mapq.neg ? mapq.mag != 0u : mapq.mag > 255u) return ENC_MAPQ;
    // CIGAR: the operations counted, their reference length
    uint32_t n_ops = 0;
    uint64_t ref_len = 0;
    if (fe[5] == fb[5]) return ENC_CIGAR;
    if (!(fe[5] - fb[5] == 1u && line[fb[5]] == '*')) {
        uint32_t p = fb[5];
        while (p < fe[5]) {
            uint32_t q = p;
            while (q < fe[5] && line[q] >= '0' && line[q] <= '9') ++q;
            if (q == p || q == fe[5]) return ENC_CIGAR;
            const int op = cigar_code(line[q]);
            if (op < 0) return ENC_CIGAR;
            const Num len = number(line, p, q);
            if (len.mag >= (1ull << 28)) return ENC_CIGAR;
            if (!HOST && !len.canon) return ENC_HOST_NUMBER;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ref_len += len.mag;
            ++n_ops;
            p = q + 1u;
        }
    }
    const bool long_cigar = n_ops > MAX_CIGAR_OPS;
    if (long_cigar && !HOST) return ENC_HOST_LONG_CIGAR;
    int32_t next_id = -1;
    if (fe[6] == fb[6]) return ENC_RNEXT;
    if (fe[6] - fb[6] == 1u && line[fb[6]] == '=') next_id = ref_id;
    else if (!(fe[6] - fb[6] == 1u && line[fb[6]] == '*')) {
        next_id = refs.find(line + fb[6], fe[6] - fb[6]);
        if (next_id < 0) return ENC_RNEXT;
    }
    const Num pn = number(line, fb[7], fe[7]);
    if (!pn.ok) return ENC_PNEXT;
    if (!HOST && !pn.canon) return ENC_HOST_NUMBER;
    if (pn.neg ? pn.mag != 0u : pn.mag > 2147483647ull) return ENC_PNEXT;
    const Num tl = number(line, fb[8], fe[8]);
    if (!tl.ok) return ENC_TLEN;
    if (!HOST && !tl.canon) return ENC_HOST_NUMBER;
    if (value_of(tl) < -2147483648ll || value_of(tl) > 2147483647ll) return ENC_TLEN;
    // SEQ and QUAL
    uint32_t seq_b = pos, seq_e, qual_b, qual_e, l_seq;
    bool qual_star;
    if (!writing) {
        seq_e = next_tab(line, seq_b, n);
        if (seq_e >= n) return ENC_FIELDS;
        if (seq_e == seq_b) return ENC_SEQ;
        const bool seq_star = seq_e - seq_b == 1u && line[seq_b] == '*';
        l_seq = seq_star ? 0u : seq_e - seq_b;
        if (!seq_star)
            for (uint32_t k = seq_b; k < seq_e; ++k)
                if (seq_code(line[k]) > 15u) {
                    if (!HOST) return ENC_HOST_SEQ_CODE;
                    break;
                }
        qual_b = seq_e + 1u;
        qual_e = next_tab(line, qual_b, n);
        qual_star = qual_e - qual_b == 1u && line[qual_b] == '*';
        if (!qual_star) {
            if (qual_e - qual_b != l_seq || l_seq == 0u) return ENC_QUAL;
            for (uint32_t k = qual_b; k < qual_e; ++k)
                if (line[k] < '!' || line[k] > '~') return ENC_QUAL;
        }
        sz.seq_off = seq_b;
        sz.l_seq = l_seq;
    } else {
        if (sz.seq_off != seq_b) return ENC_FIELDS;     // (not the line step 1 saw)
        l_seq = sz.l_seq;
        seq_e = seq_b + (l_seq ? l_seq : 1u);
        qual_b = seq_e + 1u;
        if (qual_b >= n) return ENC_FIELDS;
        qual_star = l_seq == 0u || (line[qual_b] == '*' && (qual_b + 1u >= n || line[qual_b + 1u] == '\t'));
        qual_e = qual_b + (qual_star ? 1u : l_seq);
        if (qual_e > n) return ENC_FIELDS;
    }
    // the record
    const int64_t pos0 = (int64_t)p1.mag - 1;
    const uint32_t fl = (uint32_t)flag.mag;
    const int64_t span = (ref_len > 0u && (fl & 4u) == 0u) ? (int64_t)ref_len : 1;
    const uint32_t bin = reg2bin(pos0, pos0 + span) & 0xFFFFu;
    const uint32_t stored_ops = long_cigar ? 2u : n_ops;
    if (ref_shift != 0) {
        if (ref_id >= 0) ref_id += ref_shift;
        if (next_id >= 0) next_id += ref_shift;
    }
    o.put32(0);                                        // block_size: known at the end
    o.put32((uint32_t)ref_id);
    o.put32((uint32_t)(int32_t)pos0);
    o.put8(l_name + 1u);
    o.put8((uint32_t)mapq.mag);
    o.put16(bin);
    o.put16(stored_ops);
    o.put16(fl);
    o.put32(l_seq);
    o.put32((uint32_t)next_id);
    o.put32((uint32_t)(int32_t)((int64_t)pn.mag - 1));
    o.put32((uint32_t)(int32_t)value_of(tl));
    for (uint32_t k = fb[0]; k < fe[0]; ++k) o.put8(line[k]);
    o.put8(0);
    if (long_cigar) {
        o.put32((l_seq << 4) | 4u);
        o.put32(((uint32_t)ref_len << 4) | 3u);
    } else if (n_ops) {
        uint32_t p = fb[5];
        while (p < fe[5]) {
            uint32_t q = p, len = 0;
            while (q < fe[5] && line[q] >= '0' && line[q] <= '9') { len = len * 10u + (line[q] - '0'); ++q; }
            o.put32((len << 4) | (uint32_t)cigar_code(line[q]));
            p = q + 1u;
        }
    }
    const uint64_t seq_dst = o.at, qual_dst = seq_dst + (l_seq + 1u) / 2u;
    o.at = qual_dst + l_seq;
    if (writing) {
        if (o.at > o.cap) return ENC_SIZE;              // (step 1 gave the size: cannot happen for the line it saw)
        if (bulk) {
            bulk->seq_src = seq_b; bulk->l_seq = l_seq; bulk->seq_dst = (uint32_t)seq_dst;
            bulk->qual_src = qual_star ? ~0u : qual_b; bulk->qual_dst = (uint32_t)qual_dst;
        } else {
            pack_seq(line + seq_b, l_seq, o.out + seq_dst, 0u, 1u);
            pack_qual(qual_star ? nullptr : line + qual_b, l_seq, o.out + qual_dst, 0u, 1u);
        }
    }
    // the optional fields
    pos = qual_e + 1u;
    while (pos <= n && qual_e < n) {
        const uint32_t e = next_tab(line, pos, n);
        const int32_t rc = aux_field<HOST>(line, pos, e, o);
        if (rc != ENC_OK) return rc;
        if (e >= n) break;
        pos = e + 1u;
    }
    if (long_cigar) {                                  // 4.2.2: the real operations as CG:B:I behind the other fields
        o.put8('C'); o.put8('G'); o.put8('B'); o.put8('I'); o.put32(n_ops);
        uint32_t p = fb[5];
        while (p < fe[5]) {
            uint32_t q = p, len = 0;
            while (q < fe[5] && line[q] >= '0' && line[q] <= '9') { len = len * 10u + (line[q] - '0'); ++q; }
            o.put32((len << 4) | (uint32_t)cigar_code(line[q]));
            p = q + 1u;
        }
    }
    if (o.at > 0x7FFFFFFFull) return ENC_SIZE;
    o.poke32(0, (uint32_t)o.at - 4u);
    if (!writing) sz.size = (uint32_t)o.at;
    return ENC_OK;
}

// step 1: the size of the line's record (sz.size, with the block_size word), or why it is declined (sz.reason; sz.size = 0)
template <bool HOST, class Refs> XSR_HD Sized size_of(const uint8_t *line, uint32_t n, const Refs &refs)
{
    Sized sz{0, ENC_OK, 0, 0};
    Sink o{nullptr, 0, 0};
    sz.reason = run<HOST>(line, n, refs, 0, sz, o, nullptr);
    if (sz.reason != ENC_OK) sz.size = 0;
    return sz;
}

// step 2: the record into out[0, sz.size).  bulk == nullptr: all of it; else everything but SEQ and QUAL, which the caller packs
// (pack_seq / pack_qual) from where *bulk says.  Returns ENC_OK, or a reason when the line is not the one step 1 sized.
template <bool HOST, class Refs>
XSR_HD int32_t write(const uint8_t *line, uint32_t n, const Refs &refs, int32_t ref_shift, const Sized &sz, uint8_t *out, Bulk *bulk)
{
    Sized s = sz;
    Sink o{out, sz.size, 0};
    const int32_t rc = run<HOST>(line, n, refs, ref_shift, s, o, bulk);
    if (rc == ENC_OK && o.at != sz.size) return ENC_SIZE;
    return rc;
}

}  // namespace xmsam
