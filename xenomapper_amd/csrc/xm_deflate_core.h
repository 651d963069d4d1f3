// xm_deflate_core.h -- raw-DEFLATE encoder of one BGZF block (RFC 1951, one dynamic-Huffman or one stored block, BFINAL = 1),
// the sibling of xm_inflate_core.h: one source for the device, where a CHAIN is one whole wave of 64 lanes, and for the host
// (tests/deflate_core_host.cpp), where the 64 lanes are emulated ONE AFTER THE OTHER, phase by phase.  Nothing here is taken
// from zlib or any other encoder; the format is restated from the RFC for the execution model below.
//
// One chain encodes one block of n <= 65280 bytes:
//   M  match candidates: a wave-uniform loop over chunks of 64 positions, lane i takes position p = 64 c + i, hashes the 4 bytes
//      at p into an LDS table (entry = position + 1, 0 = empty), READS its candidate, and only after every lane of the chunk has
//      read inserts with atomicMax -- the table is a function of the input alone, and a candidate always lies in an earlier chunk
//      (so it is < p without a race check).  The lane compares up to min(258, n - p) bytes, 16 at a time, and leaves one word per
//      position in the chain's scratch: the byte | (len - 3) << 8 | (dist - 1) << 16, len field 0 = no match of 4 or more.
//   P  parse: lane l owns the segment [l S, min(n, (l + 1) S)), S = ceil(n / 64), and walks it greedily: a match is taken when,
//      cut at the segment's end, it is still 4 bytes or longer, else a literal.  Symbol frequencies go to LDS histograms.
//      Nothing is stored per token: the walk is repeated twice in E.
//   H  codes: at least two symbols per alphabet (as zlib forces them), Huffman code lengths from the sorted frequencies (two
//      queues, one lane), limited to 15 bits by rebuilding with every frequency f replaced by (f + 1) / 2 until the depth fits
//      (at most 17 rounds: 65281 < 2^17), canonical codes bit-reversed for the LSB-first stream.
//   header: BTYPE = 2, HCLEN = 19, the code-length code gives 0 .. 15 four bits each and 16 / 17 / 18 none -- a complete code;
//      no run-length coding of the lengths: 17 + 57 + 4 (HLIT + HDIST) bits.
//   E  emit: every lane sums the bits of its segment, the lanes' offsets are the sums in front of them, and a third walk writes
//      the bits: words that are wholly a lane's own are stored, the words at either end of a lane's range, which neighbours
//      share, go by atomic OR into words zeroed beforehand (the stream's last, partial word is collected in LDS and stored byte
//      by byte: nothing is written behind the stream's last byte).  If the dynamic stream would not be smaller than n + 5
//      bytes, ONE STORED BLOCK is written instead (01 LEN NLEN + the bytes): the result is never longer than n + 5.
//
// Rules (the host emulation is legal only because of the first):
//   R1  no lane ever waits for another lane: inside a lane-dependent loop (the compare loop of M, the walks of P and E) a lane
//       touches its own state, memory nobody writes in that phase, and commutative atomics; there are no ballots, shuffles or
//       scans anywhere -- what crosses lanes goes through LDS between two phases (sync()).  xm_inflate.hip records what happened
//       to chains that did otherwise.
//   R2  every loop is bounded by n, 258, 64, 17 or the alphabet sizes, whatever the data holds.
//   R3  the output is a pure function of the input bytes: not of alignment, chain, or a race; device and host give the same bytes.
//   R4  reads: [in, in + n + 16) -- the unaligned 16-byte loads of M may reach 15 bytes behind the block; what they read there
//       does not matter (the compared length is cut at n).  Writes: the block's own [out, out + n + 5) and the chain's own scratch
//       words [0, n).  `in` may have any alignment; `out` and `scratch` are 16-byte aligned.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
#define XMD_HD __device__ __forceinline__
#define XMD_DEVICE 1
#else
#define XMD_HD inline
#define XMD_DEVICE 0
#endif

// a phase: the statement that follows runs once per lane -- on the device by the lane itself, on the host for l = 0 .. 63 in turn
#if XMD_DEVICE
#define XMD_LANES(l) for (uint32_t l = threadIdx.x, xmd_once_ = 1u; xmd_once_; xmd_once_ = 0u)
#define XMD_LANE0 if (threadIdx.x == 0u)
#elif defined(XMD_HOST_LANES_REVERSED)                      // tests: R1 makes the order of the emulated lanes immaterial
#define XMD_LANES(l) for (uint32_t l = 63u; l < 64u; --l)
#define XMD_LANE0
#else
#define XMD_LANES(l) for (uint32_t l = 0; l < 64u; ++l)
#define XMD_LANE0
#endif

// what a lane carries from one phase of M to the next: registers on the device, an array of 64 on the host
#if XMD_DEVICE
#define XMD_MLANE_DECL(name) MLane name
#define XMD_MLANE(name, l) name
#else
#define XMD_MLANE_DECL(name) MLane name[64]
#define XMD_MLANE(name, l) name[l]
#endif

namespace xmd {

constexpr uint32_t MAX_ISIZE = 65280u;
constexpr uint32_t HASH_BITS = 12u;
constexpr uint32_t MIN_MATCH = 4u, MAX_MATCH = 258u, MAX_DIST = 32768u;
constexpr uint32_t N_LIT = 286u, N_DIST = 30u, EOB = 256u;
constexpr uint32_t SCRATCH_WORDS = MAX_ISIZE;          // one word per input byte (a multiple of 4: groups of four are read whole)
constexpr uint32_t MAX_BITS = 15u;

// what a block's encoding went through (host build: the test counts them; the device ignores it)
enum : uint32_t { F_STORED = 1u, F_LIMITED = 2u, F_FORCED = 4u };

struct alignas(16) ChainMem {
    uint32_t hash[1u << HASH_BITS];     // position + 1 of the latest insert, 0 = empty
    uint32_t lfreq[288];                // literal / length frequencies, then (code bit-reversed) | length << 16
    uint32_t dfreq[32];
    uint32_t node_freq[2 * 288];        // Huffman tree: leaves in sorted order, then the internal nodes in the order they are made
    uint16_t parent[2 * 288];
    uint16_t order[288];                // symbols of non-zero frequency, by (frequency, symbol)
    uint8_t depth[2 * 288];
    uint8_t llen[288], dlen[32];        // code lengths
    uint32_t lane_bits[64];             // bits of every lane's segment
    uint32_t tail;                      // the stream's last, partial word
    uint32_t n_used;                    // symbols of non-zero frequency in the alphabet being built
    uint32_t flags;
};

struct u128 { uint32_t w[4]; };
struct MLane { u128 a; uint32_t h, cand; bool hashed; };     // the 16 bytes at the lane's position, their hash, the candidate read

#if XMD_DEVICE
typedef uint32_t v4u32_any __attribute__((ext_vector_type(4), aligned(1)));
#endif

XMD_HD u128 loadu16(const uint8_t *p)               // any alignment
{
    u128 v;
#if XMD_DEVICE
    const v4u32_any q = *reinterpret_cast<const v4u32_any *>(p);
    v.w[0] = q.x; v.w[1] = q.y; v.w[2] = q.z; v.w[3] = q.w;
#else
    memcpy(&v, p, 16);
#endif
    return v;
}
XMD_HD u128 load16(const void *p)                   // 16-byte aligned
{
    u128 v;
#if XMD_DEVICE
    const uint4 q = *reinterpret_cast<const uint4 *>(p);
    v.w[0] = q.x; v.w[1] = q.y; v.w[2] = q.z; v.w[3] = q.w;
#else
    memcpy(&v, p, 16);
#endif
    return v;
}
XMD_HD void store16(void *p, const u128 &v)         // 16-byte aligned
{
#if XMD_DEVICE
    *reinterpret_cast<uint4 *>(p) = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]);
#else
    memcpy(p, &v, 16);
#endif
}
XMD_HD uint32_t ctz32(uint32_t v) { return (uint32_t)__builtin_ctz(v); }      // v != 0
XMD_HD uint32_t log2_32(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }   // v != 0
XMD_HD uint32_t bitrev32(uint32_t v)
{
#if XMD_DEVICE
    return __brev(v);
#else
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0F0F0F0Fu) | ((v & 0x0F0F0F0Fu) << 4);
    v = ((v >> 8) & 0x00FF00FFu) | ((v & 0x00FF00FFu) << 8);
    return (v >> 16) | (v << 16);
#endif
}
// commutative atomics: LDS or global on the device, plain on the host (the lanes run in turn)
XMD_HD void atomic_max(uint32_t *p, uint32_t v)
{
#if XMD_DEVICE
    atomicMax(p, v);
#else
    if (v > *p) *p = v;
#endif
}
XMD_HD void atomic_add(uint32_t *p, uint32_t v)
{
#if XMD_DEVICE
    atomicAdd(p, v);
#else
    *p += v;
#endif
}
XMD_HD void atomic_or(uint32_t *p, uint32_t v)
{
#if XMD_DEVICE
    atomicOr(p, v);
#else
    *p |= v;
#endif
}
// between two phases: what the lanes wrote -- LDS, scratch, the slot -- is where the other lanes read it.  A chain is one wave and
// a workgroup of its own, so nothing is waited FOR except the wave's own outstanding memory operations.
XMD_HD void sync()
{
#if XMD_DEVICE
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
#endif
}

// ---- symbols (RFC 1951 3.2.5 as arithmetic) ---------------------------------------------------------------------------------------
struct Sym { uint32_t code, extra_bits, extra; };
XMD_HD Sym length_symbol(uint32_t len)              // 3 .. 258
{
    const uint32_t l = len - 3u;
    if (l < 8u) return {257u + l, 0u, 0u};
    if (len == 258u) return {285u, 0u, 0u};
    const uint32_t eb = log2_32(l) - 2u;
    return {257u + 4u * eb + 4u + ((l >> eb) & 3u), eb, l & ((1u << eb) - 1u)};
}
XMD_HD Sym dist_symbol(uint32_t dist)               // 1 .. 32768
{
    const uint32_t d = dist - 1u;
    if (d < 4u) return {d, 0u, 0u};
    const uint32_t hb = log2_32(d), eb = hb - 1u;
    return {2u * hb + ((d >> eb) & 1u), eb, d & ((1u << eb) - 1u)};
}

// ---- the greedy walk of one lane's segment (P, and twice in E) -----------------------------------------------------------------------
// Four scratch words are fetched at a time (aligned), so a run of literals costs one load per four steps.
template <class Lit, class Match>
XMD_HD void walk(const uint32_t *scratch, uint32_t n, uint32_t lane, Lit on_literal, Match on_match)
{
    const uint32_t S = (n + 63u) / 64u;
    uint32_t pos = lane * S;
    const uint32_t end = pos + S < n ? pos + S : n;
    uint32_t base = 0xFFFFFFFFu;
    u128 q = {{0u, 0u, 0u, 0u}};
    while (pos < end) {                                 // R2: every pass moves pos on
        if ((pos & ~3u) != base) { base = pos & ~3u; q = load16(scratch + base); }
        const uint32_t k = pos & 3u;
        const uint32_t e = k == 0u ? q.w[0] : k == 1u ? q.w[1] : k == 2u ? q.w[2] : q.w[3];
        uint32_t len = (e >> 8) & 0xFFu;
        if (len) { len += 3u; if (len > end - pos) len = end - pos; }
        if (len >= MIN_MATCH) { on_match(len, (e >> 16) + 1u); pos += len; }
        else { on_literal(e & 0xFFu); pos += 1u; }
    }
}

// ---- bits into the slot ------------------------------------------------------------------------------------------------------------
// A writer owns the bits [at, at + what it puts).  Words that are wholly its own are stored; the first word when it begins inside
// one, and the last when it ends inside one, are OR-ed (zeroed in the phase before: zero_edges).  The stream's last word, when the
// stream ends inside it, lives in LDS until store_tail.
struct Writer {
    uint32_t *out;
    ChainMem *m;
    uint32_t tail_word;                 // index of the partial last word, 0xFFFFFFFF: the stream ends on a word boundary
    uint32_t word;                      // next word to write
    uint64_t buf;
    uint32_t nbuf;
    bool shared;                        // the next word written begins in front of this writer's first bit

    XMD_HD void begin(uint32_t *o, ChainMem *mem, uint32_t tw, uint32_t at)
    {
        out = o; m = mem; tail_word = tw;
        word = at >> 5; nbuf = at & 31u; buf = 0; shared = nbuf != 0u;
    }
    XMD_HD void or_word(uint32_t w, uint32_t v)
    {
        if (w == tail_word) atomic_or(&m->tail, v);
        else atomic_or(out + w, v);
    }
    XMD_HD void put(uint32_t v, uint32_t nb)           // nb <= 28, v < 2^nb
    {
        buf |= (uint64_t)v << nbuf;
        nbuf += nb;
        if (nbuf >= 32u) {
            if (shared) or_word(word, (uint32_t)buf);
            else out[word] = (uint32_t)buf;             // (never the tail word: that one is not filled)
            shared = false;
            ++word; buf >>= 32; nbuf -= 32u;
        }
    }
    XMD_HD void end()
    {
        if (buf != 0u) or_word(word, (uint32_t)buf);       // (zero bits: the word was zeroed, and a writer that put nothing touches nothing)
    }
};
// the words at either end of the bits [at, at + nbits) are zero before anybody ORs into them
XMD_HD void zero_edges(uint32_t *out, uint32_t tail_word, uint32_t at, uint32_t nbits)
{
    if (nbits == 0u) return;
    const uint32_t a = at >> 5, b = (at + nbits - 1u) >> 5;
    if (a != tail_word) out[a] = 0u;
    if (b != tail_word) out[b] = 0u;
}

// ---- code lengths ------------------------------------------------------------------------------------------------------------------
// freq[0 .. n_sym) -> len[0 .. n_sym), every length <= 15, Kraft sum exactly 1 (two symbols at least are given a code: a symbol of
// zero frequency is added when fewer are used).  All lanes call it; freq is changed only by the forced symbols.
XMD_HD void code_lengths(ChainMem *m, uint32_t *freq, uint32_t n_sym, uint8_t *len)
{
    XMD_LANE0 {
        uint32_t used = 0;
        for (uint32_t s = 0; s < n_sym; ++s) used += freq[s] != 0u;
        if (used < 2u) m->flags |= F_FORCED;
        for (uint32_t s = 0; s < 2u && used < 2u; ++s) if (freq[s] == 0u) { freq[s] = 1u; ++used; }
        m->n_used = used;
    }
    sync();
    // rank sort by (frequency, symbol): a lane per symbol, every lane the same 288 comparisons
    XMD_LANES(l) {
        for (uint32_t s = l; s < n_sym; s += 64u) {
            const uint32_t f = freq[s];
            len[s] = 0;
            if (f == 0u) continue;
            uint32_t rank = 0;
            for (uint32_t t = 0; t < n_sym; ++t) {
                const uint32_t g = freq[t];
                rank += (g != 0u && (g < f || (g == f && t < s))) ? 1u : 0u;
            }
            m->order[rank] = (uint16_t)s;
            m->node_freq[rank] = f;
        }
    }
    sync();
    XMD_LANE0 {
        const uint32_t k = m->n_used;                       // 2 .. 286 leaves: nodes [0, k), internal nodes [k, 2k - 1)
        for (uint32_t round = 0; round < 18u; ++round) {    // R2: frequencies <= 65281 are all 1 after 17 halvings: depth <= 9
            uint32_t leaf = 0, inner = k, made = k;
            while (made < 2u * k - 1u) {
                uint32_t pick[2];
                for (uint32_t j = 0; j < 2u; ++j) {         // the smaller head of the two queues; a leaf on a tie
                    const bool take_leaf = leaf < k && (inner >= made || m->node_freq[leaf] <= m->node_freq[inner]);
                    pick[j] = take_leaf ? leaf++ : inner++;
                }
                m->node_freq[made] = m->node_freq[pick[0]] + m->node_freq[pick[1]];
                m->parent[pick[0]] = (uint16_t)made;
                m->parent[pick[1]] = (uint16_t)made;
                ++made;
            }
            m->depth[2u * k - 2u] = 0;
            uint32_t deepest = 0;
            for (uint32_t t = 2u * k - 2u; t-- > 0u;) {     // a parent is made after its children: its depth is known first
                const uint32_t d = m->depth[m->parent[t]] + 1u;
                m->depth[t] = (uint8_t)d;
                if (t < k && d > deepest) deepest = d;
            }
            if (deepest <= MAX_BITS) break;
            m->flags |= F_LIMITED;
            for (uint32_t t = 0; t < k; ++t) m->node_freq[t] = (m->node_freq[t] + 1u) / 2u;    // the order stays sorted
        }
        for (uint32_t t = 0; t < k; ++t) len[m->order[t]] = m->depth[t];
    }
    sync();
}
// canonical codes of len[0 .. n_sym) into code[]: (the code, first bit lowest) | length << 16.  One lane.
XMD_HD void assign_codes(uint32_t *code, const uint8_t *len, uint32_t n_sym)
{
    XMD_LANE0 {
        uint32_t count[MAX_BITS + 1u], next[MAX_BITS + 1u];
        for (uint32_t b = 0; b <= MAX_BITS; ++b) count[b] = 0;
        for (uint32_t s = 0; s < n_sym; ++s) ++count[len[s]];
        uint32_t c = 0;
        count[0] = 0;
        next[0] = 0;
        for (uint32_t b = 1; b <= MAX_BITS; ++b) { c = (c + count[b - 1u]) << 1; next[b] = c; }
        for (uint32_t s = 0; s < n_sym; ++s) {
            const uint32_t L = len[s];
            code[s] = L ? ((bitrev32(next[L]++) >> (32u - L)) | (L << 16)) : 0u;
        }
    }
    sync();
}

// ---- the block ---------------------------------------------------------------------------------------------------------------------
// in[0 .. n) -> out, returns the stream's length in bytes (<= n + 5).  Every lane of the chain calls it with the same arguments
// (the host: one call).  n <= MAX_ISIZE.
XMD_HD uint32_t deflate_block(ChainMem *m, const uint8_t *in, uint32_t n, uint8_t *out, uint32_t *scratch)
{
    uint32_t *out32 = reinterpret_cast<uint32_t *>(out);
    // ---- M ----
    XMD_LANES(l) {
        const u128 zero = {{0u, 0u, 0u, 0u}};
        for (uint32_t i = l * 4u; i < (1u << HASH_BITS); i += 256u) store16(m->hash + i, zero);
        for (uint32_t i = l; i < 288u; i += 64u) m->lfreq[i] = 0u;
        if (l < 32u) m->dfreq[l] = 0u;
        if (l == 0u) { m->tail = 0u; m->flags = 0u; }
    }
    sync();
    for (uint32_t c = 0; c * 64u < n; ++c) {
        XMD_MLANE_DECL(mine);
        XMD_LANES(l) {
            const uint32_t p = c * 64u + l;
            MLane &s = XMD_MLANE(mine, l);
            s.hashed = p + MIN_MATCH <= n;                  // the block's last 3 positions get no candidate
            s.cand = 0u;
            s.h = 0u;
            if (p < n) s.a = loadu16(in + p);
            if (s.hashed) {
                s.h = (s.a.w[0] * 2654435761u) >> (32u - HASH_BITS);
                s.cand = m->hash[s.h];
            }
        }
        sync();                                             // every lane of the chunk has read
        XMD_LANES(l) {
            const uint32_t p = c * 64u + l;
            const MLane &s = XMD_MLANE(mine, l);
            const u128 a = s.a;
            if (s.hashed) atomic_max(&m->hash[s.h], p + 1u);
            if (p < n) {
                uint32_t len = 0, dist = 1u;
                if (s.cand != 0u && p - (s.cand - 1u) <= MAX_DIST) {
                    const uint32_t q = s.cand - 1u;
                    dist = p - q;
                    const uint32_t limit = n - p < MAX_MATCH ? n - p : MAX_MATCH;
                    u128 x = a;
                    for (uint32_t k = 0; k < limit; k += 16u) {     // R1: own registers and the input, which nobody writes
                        if (k) x = loadu16(in + p + k);
                        const u128 y = loadu16(in + q + k);
                        const uint32_t d0 = x.w[0] ^ y.w[0], d1 = x.w[1] ^ y.w[1], d2 = x.w[2] ^ y.w[2], d3 = x.w[3] ^ y.w[3];
                        if (d0 | d1 | d2 | d3) {
                            len = k + (d0 ? ctz32(d0) >> 3 : d1 ? 4u + (ctz32(d1) >> 3) : d2 ? 8u + (ctz32(d2) >> 3) : 12u + (ctz32(d3) >> 3));
                            break;
                        }
                        len = k + 16u;
                    }
                    if (len > limit) len = limit;
                }
                scratch[p] = (a.w[0] & 0xFFu) | (len >= MIN_MATCH ? ((len - 3u) << 8) | ((dist - 1u) << 16) : 0u);
            }
        }
        sync();                                             // the inserts are in the table before the next chunk reads it
    }
    // ---- P ----
    XMD_LANES(l) {
        walk(scratch, n, l,
             [&](uint32_t byte) { atomic_add(&m->lfreq[byte], 1u); },
             [&](uint32_t len, uint32_t dist) {
                 atomic_add(&m->lfreq[length_symbol(len).code], 1u);
                 atomic_add(&m->dfreq[dist_symbol(dist).code], 1u);
             });
        if (l == 0u) atomic_add(&m->lfreq[EOB], 1u);
    }
    sync();
    // ---- H ----
    code_lengths(m, m->lfreq, N_LIT, m->llen);
    code_lengths(m, m->dfreq, N_DIST, m->dlen);
    assign_codes(m->lfreq, m->llen, N_LIT);                 // the frequencies are done with: the codes take their place
    assign_codes(m->dfreq, m->dlen, N_DIST);
    uint32_t hlit = N_LIT, hdist = N_DIST;
    while (hlit > 257u && m->llen[hlit - 1u] == 0) --hlit;
    while (hdist > 1u && m->dlen[hdist - 1u] == 0) --hdist;
    const uint32_t n_len = hlit + hdist, head_bits = 17u + 57u + 4u * n_len;
    // ---- E: count ----
    XMD_LANES(l) {
        uint32_t bits = 0;
        walk(scratch, n, l,
             [&](uint32_t byte) { bits += m->lfreq[byte] >> 16; },
             [&](uint32_t len, uint32_t dist) {
                 const Sym ls = length_symbol(len), ds = dist_symbol(dist);
                 bits += (m->lfreq[ls.code] >> 16) + ls.extra_bits + (m->dfreq[ds.code] >> 16) + ds.extra_bits;
             });
        if (l == 63u) bits += m->lfreq[EOB] >> 16;
        m->lane_bits[l] = bits;
    }
    sync();
    uint32_t total_bits = head_bits;
    for (uint32_t i = 0; i < 64u; ++i) total_bits += m->lane_bits[i];
    const uint32_t clen = (total_bits + 7u) / 8u;
    if (clen >= n + 5u) {
        // ---- one stored block: 01 LEN NLEN and the bytes; whole 16-byte lines of the slot where they are wholly payload ----
        XMD_LANE0 m->flags |= F_STORED;
        const uint32_t total = n + 5u, lines = total / 16u;
        XMD_LANES(l) {
            for (uint32_t j = 1u + l; j < lines; j += 64u) store16(out + 16u * j, loadu16(in + 16u * j - 5u));
            // the first line (the header and 11 bytes) and what is left behind the last whole line: a byte per lane
            const uint32_t head[5] = {1u, n & 0xFFu, n >> 8, ~n & 0xFFu, (~n >> 8) & 0xFFu};
            const uint32_t first_end = total < 16u ? total : 16u;
            if (l < first_end) out[l] = (uint8_t)(l < 5u ? head[l] : in[l - 5u]);
            const uint32_t t = 16u * lines + l;
            if (lines >= 1u && l < 16u && t < total) out[t] = in[t - 5u];
        }
        sync();
        return total;
    }
    // ---- E: emit ----
    const uint32_t tail_word = (clen & 3u) ? clen >> 2 : 0xFFFFFFFFu;
    const uint32_t per = (n_len + 63u) / 64u;               // code lengths of the header per lane (<= 5)
    XMD_LANES(l) {
        uint32_t at = head_bits;
        for (uint32_t i = 0; i < l; ++i) at += m->lane_bits[i];
        zero_edges(out32, tail_word, at, m->lane_bits[l]);
        const uint32_t h0 = l * per < n_len ? l * per : n_len, h1 = h0 + per < n_len ? h0 + per : n_len;
        zero_edges(out32, tail_word, 74u + 4u * h0, 4u * (h1 - h0));
        if (l == 0u) zero_edges(out32, tail_word, 0u, 74u);
    }
    sync();
    XMD_LANES(l) {
        Writer w;
        if (l == 0u) {
            // BFINAL = 1, BTYPE = 2 | HLIT | HDIST | HCLEN = 19; the code-length code's lengths in the order 16 17 18 0 8 7 ...
            w.begin(out32, m, tail_word, 0u);
            w.put(5u | (hlit - 257u) << 3 | (hdist - 1u) << 8 | 15u << 13, 17u);
            w.put(0u, 9u);
            for (uint32_t i = 0; i < 4u; ++i) w.put(0x924u, 12u);          // four times 4 4 4 4 in three bits each
            w.end();
        }
        const uint32_t h0 = l * per < n_len ? l * per : n_len, h1 = h0 + per < n_len ? h0 + per : n_len;
        w.begin(out32, m, tail_word, 74u + 4u * h0);
        for (uint32_t i = h0; i < h1; ++i) {
            const uint32_t L = i < hlit ? m->llen[i] : m->dlen[i - hlit];
            w.put(bitrev32(L) >> 28, 4u);                                   // symbol L of the code-length code: L in four bits, first bit lowest
        }
        w.end();
        uint32_t at = head_bits;
        for (uint32_t i = 0; i < l; ++i) at += m->lane_bits[i];
        w.begin(out32, m, tail_word, at);
        walk(scratch, n, l,
             [&](uint32_t byte) { const uint32_t c = m->lfreq[byte]; w.put(c & 0xFFFFu, c >> 16); },
             [&](uint32_t len, uint32_t dist) {
                 const Sym ls = length_symbol(len), ds = dist_symbol(dist);
                 const uint32_t lc = m->lfreq[ls.code], dc = m->dfreq[ds.code];
                 w.put((lc & 0xFFFFu) | ls.extra << (lc >> 16), (lc >> 16) + ls.extra_bits);
                 w.put((dc & 0xFFFFu) | ds.extra << (dc >> 16), (dc >> 16) + ds.extra_bits);
             });
        if (l == 63u) { const uint32_t c = m->lfreq[EOB]; w.put(c & 0xFFFFu, c >> 16); }
        w.end();
    }
    sync();
    XMD_LANES(l) {
        if (tail_word != 0xFFFFFFFFu && l < (clen & 3u)) out[4u * tail_word + l] = (uint8_t)(m->tail >> (8u * l));
    }
    sync();
    return clen;
}

}  // namespace xmd
