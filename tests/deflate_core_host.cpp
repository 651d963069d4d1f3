// deflate_core_host.cpp -- TEST INFRASTRUCTURE (never linked into a library): the encoder of xenomapper_amd/csrc/xm_deflate_core.h
// compiled for the host, its 64 lanes emulated one after the other, against zlib's inflate and the project's own decoder
// (xm_inflate_core.h as a chain of one lane).  The device build of the same source is tests/test_deflate_gpu.py, which also
// compares its bytes with the ones this program writes (--emit).
//   usage: deflate_core_host --blocks FILE [--emit OUT]   every block of FILE (count, then length + bytes per block: tests/deflate_shapes.py)
//          deflate_core_host --mix N SEED                 N seeded random mixes of the payload kinds
//          deflate_core_host --builder                    the code-length builder on Fibonacci and on equal frequencies
//          deflate_core_host --ratio FILE                 the encoder's total against zlib level 1 and Z_HUFFMAN_ONLY on FILE's blocks
// Per block: zlib inflates the stream to the input; so does the project's decoder, with status 0; the stream is no longer than
// n + 5; 64 poisoned guard bytes on either side of the slot and of the scratch are intact; the input is unchanged; a second run
// gives the same bytes.
#include "../xenomapper_amd/csrc/xm_deflate_core.h"
#include "../xenomapper_amd/csrc/xm_inflate_core.h"

#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

static const uint32_t GUARD = 64;
static unsigned long n_stored, n_limited, n_forced;

struct Aligned {                                   // 16-byte aligned storage with guard bytes on either side
    std::vector<uint8_t> mem;
    uint8_t *p;
    size_t len;
    Aligned(size_t bytes, uint8_t fill) : mem(bytes + 2 * GUARD + 16, fill), len(bytes)
    {
        p = mem.data() + GUARD;
        p += (16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15;
    }
    bool guards_intact(uint8_t fill) const
    {
        for (const uint8_t *q = mem.data(); q < p; ++q) if (*q != fill) return false;
        for (const uint8_t *q = p + len; q < mem.data() + mem.size(); ++q) if (*q != fill) return false;
        return true;
    }
};

// -> the stream; false: a check failed
static bool encode_checked(const std::vector<uint8_t> &payload, unsigned shift, std::vector<uint8_t> &stream, const char *what)
{
    static xmd::ChainMem mem;
    const uint32_t n = (uint32_t)payload.size();
    // the input at an arbitrary alignment, 16 readable bytes behind it (xm_deflate_core.h R4) -- and not one more
    std::vector<uint8_t> in(shift + n + 16, 0x5A);
    if (n) memcpy(in.data() + shift, payload.data(), n);
    const std::vector<uint8_t> in_before = in;
    std::vector<uint8_t> runs[2];
    for (int r = 0; r < 2; ++r) {
        Aligned slot(n + 5, 0xEE), scratch(4 * (size_t)((n + 3u) & ~3u), 0xDD);
        memset(slot.p, r ? 0xFF : 0x00, n + 5);                              // what the slot held before does not matter
        const uint32_t clen = xmd::deflate_block(&mem, in.data() + shift, n, slot.p, reinterpret_cast<uint32_t *>(scratch.p));
        if (clen > n + 5) { fprintf(stderr, "%s: %u bytes for %u\n", what, clen, n); return false; }
        if (!slot.guards_intact(0xEE) || !scratch.guards_intact(0xDD)) { fprintf(stderr, "%s: wrote outside the slot or the scratch\n", what); return false; }
        if (in != in_before) { fprintf(stderr, "%s: the input changed\n", what); return false; }
        runs[r].assign(slot.p, slot.p + clen);
        if (r == 0) {
            if (mem.flags & xmd::F_STORED) ++n_stored;
            if (mem.flags & xmd::F_LIMITED) ++n_limited;
            if (mem.flags & xmd::F_FORCED) ++n_forced;
            if (((mem.flags & xmd::F_STORED) != 0) != (clen == n + 5)) { fprintf(stderr, "%s: stored form and length disagree\n", what); return false; }
        }
    }
    if (runs[0] != runs[1]) { fprintf(stderr, "%s: two runs differ\n", what); return false; }
    stream = runs[0];
    // zlib
    std::vector<uint8_t> back(n + 16, 0);
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    inflateInit2(&zs, -15);
    zs.next_in = stream.data(); zs.avail_in = (uInt)stream.size();
    zs.next_out = back.data(); zs.avail_out = (uInt)back.size();
    const int rc = inflate(&zs, Z_FINISH);
    const bool z_ok = rc == Z_STREAM_END && zs.total_out == n && zs.avail_in == 0 && (n == 0 || memcmp(back.data(), payload.data(), n) == 0);
    if (!z_ok) fprintf(stderr, "%s: zlib: rc %d (%s), %lu of %u bytes, %u input bytes left\n", what, rc, zs.msg ? zs.msg : "-", zs.total_out, n, zs.avail_in);
    inflateEnd(&zs);
    if (!z_ok) return false;
    // the project's decoder
    static xmi::ChainMem imem;
    std::vector<uint8_t> comp(stream.size() + 2048, 0xA5);
    memcpy(comp.data() + 3, stream.data(), stream.size());
    std::vector<uint8_t> out(32 + n + 32, 0xEE);
    xmi::Chain<1> ch;
    const int st = n ? ch.run(&imem, 0u, comp.data(), 3, (uint32_t)stream.size(), out.data(), 16, n) : 0;
    if (st != 0 || (n && memcmp(out.data() + 16, payload.data(), n) != 0)) { fprintf(stderr, "%s: xm_inflate_core: status %d\n", what, st); return false; }
    return true;
}

static bool read_blocks(const char *path, std::vector<std::vector<uint8_t>> &blocks)
{
    FILE *fh = fopen(path, "rb");
    if (!fh) { perror(path); return false; }
    uint32_t count = 0;
    bool ok = fread(&count, 4, 1, fh) == 1;
    for (uint32_t b = 0; ok && b < count; ++b) {
        uint32_t n = 0;
        ok = fread(&n, 4, 1, fh) == 1 && n <= xmd::MAX_ISIZE;
        if (!ok) break;
        blocks.emplace_back(n);
        ok = n == 0 || fread(blocks.back().data(), 1, n, fh) == n;
    }
    fclose(fh);
    if (!ok) fprintf(stderr, "%s: not a block file\n", path);
    return ok;
}

static int run_blocks(const char *path, const char *emit)
{
    std::vector<std::vector<uint8_t>> blocks;
    if (!read_blocks(path, blocks)) return 1;
    FILE *out = emit ? fopen(emit, "wb") : nullptr;
    if (emit && !out) { perror(emit); return 1; }
    const uint32_t count = (uint32_t)blocks.size();
    if (out) fwrite(&count, 4, 1, out);
    int bad = 0;
    for (uint32_t b = 0; b < count; ++b) {
        char what[64];
        snprintf(what, sizeof what, "block %u (%zu bytes)", b, blocks[b].size());
        std::vector<uint8_t> stream;
        if (!encode_checked(blocks[b], b % 16u, stream, what)) ++bad;
        const uint32_t clen = (uint32_t)stream.size();
        if (out) { fwrite(&clen, 4, 1, out); fwrite(stream.data(), 1, clen, out); }
    }
    if (out) fclose(out);
    printf("blocks: %u, %d failures, stored %lu, limited %lu, forced %lu\n", count, bad, n_stored, n_limited, n_forced);
    return bad;
}

static int run_mix(int count, unsigned seed)
{
    std::mt19937 rng(seed);
    int bad = 0;
    for (int it = 0; it < count; ++it) {
        const size_t len = (it % 7 == 0) ? rng() % 300 : (it % 5 == 0) ? 60000 + rng() % 5281 : rng() % 20000;
        std::vector<uint8_t> raw(len);
        // pieces of several kinds in one block
        size_t at = 0;
        while (at < len) {
            const size_t piece = 1 + rng() % (len / 3 + 1), end = at + piece < len ? at + piece : len;
            const int kind = (int)(rng() % 6);
            const size_t back = at ? 1 + rng() % at : 0;
            for (size_t i = at; i < end; ++i) {
                switch (kind) {
                case 0: raw[i] = (uint8_t)rng(); break;
                case 1: raw[i] = (uint8_t)("ACGTN"[rng() % 5]); break;
                case 2: raw[i] = (uint8_t)(i % 37 < 30 ? 'F' : ',' + rng() % 40); break;
                case 3: raw[i] = back ? raw[i - back] : (uint8_t)(i * 7); break;          // a copy from anywhere in front
                case 4: raw[i] = (uint8_t)(rng() % 3 == 0 ? rng() : 0); break;
                default: raw[i] = (uint8_t)(i & 0xFF); break;
                }
            }
            at = end;
        }
        char what[64];
        snprintf(what, sizeof what, "mix %d (%zu bytes)", it, len);
        std::vector<uint8_t> stream;
        if (!encode_checked(raw, (unsigned)(rng() % 16), stream, what)) ++bad;
    }
    printf("mix: %d blocks, %d failures\n", count, bad);
    return bad;
}

static int check_lengths(const char *what, std::vector<uint32_t> freq, bool want_limited)
{
    static xmd::ChainMem mem;
    mem.flags = 0;
    std::vector<uint8_t> len(freq.size(), 0xFF);
    xmd::code_lengths(&mem, freq.data(), (uint32_t)freq.size(), len.data());
    uint32_t kraft = 0, longest = 0;
    int bad = 0;
    for (size_t s = 0; s < freq.size(); ++s) {
        if ((freq[s] != 0) != (len[s] != 0)) ++bad;
        if (len[s] > 15) ++bad;
        if (len[s] && len[s] <= 15) kraft += 1u << (15 - len[s]);
        if (len[s] > longest) longest = len[s];
    }
    if (kraft != 1u << 15) ++bad;
    if (want_limited != ((mem.flags & xmd::F_LIMITED) != 0)) ++bad;
    printf("builder %s: longest %u, Kraft sum %u / 32768, limited %d: %s\n", what, longest, kraft, (mem.flags & xmd::F_LIMITED) != 0, bad ? "BAD" : "ok");
    return bad;
}

static int run_builder()
{
    int bad = 0;
    std::vector<uint32_t> fib(286, 0);
    uint32_t a = 1, b = 1;
    for (int i = 0; i < 22; ++i) { fib[65 + 3 * i] = a; const uint32_t c = a + b; a = b; b = c; }
    bad += check_lengths("Fibonacci x 22", fib, true);
    bad += check_lengths("286 equal", std::vector<uint32_t>(286, 7), false);
    std::vector<uint32_t> one(30, 0);
    one[9] = 5;
    bad += check_lengths("one distance symbol", one, false);
    bad += check_lengths("no distance symbol", std::vector<uint32_t>(30, 0), false);
    return bad;
}

static size_t zlib_raw(const std::vector<uint8_t> &raw, int level, int strategy)
{
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    deflateInit2(&zs, level, Z_DEFLATED, -15, 8, strategy);
    std::vector<uint8_t> out(deflateBound(&zs, raw.size()) + 64);
    zs.next_in = const_cast<Bytef *>(raw.data()); zs.avail_in = (uInt)raw.size();
    zs.next_out = out.data(); zs.avail_out = (uInt)out.size();
    deflate(&zs, Z_FINISH);
    const size_t got = zs.total_out;
    deflateEnd(&zs);
    return got;
}

static int run_ratio(const char *path)
{
    std::vector<std::vector<uint8_t>> blocks;
    if (!read_blocks(path, blocks)) return 1;
    size_t in = 0, ours = 0, level1 = 0, huffman = 0;
    int bad = 0;
    for (size_t b = 0; b < blocks.size(); ++b) {
        std::vector<uint8_t> stream;
        if (!encode_checked(blocks[b], 0, stream, "ratio")) ++bad;
        in += blocks[b].size();
        ours += stream.size();
        level1 += zlib_raw(blocks[b], 1, Z_DEFAULT_STRATEGY);
        huffman += zlib_raw(blocks[b], 6, Z_HUFFMAN_ONLY);
    }
    const bool ok = !bad && ours < huffman && (double)ours <= 1.15 * (double)level1;
    printf("ratio: in %zu, encoder %zu (%.4f), zlib level 1 %zu (%.4f), Z_HUFFMAN_ONLY %zu (%.4f), encoder / level 1 = %.4f: %s\n",
           in, ours, (double)ours / in, level1, (double)level1 / in, huffman, (double)huffman / in, (double)ours / level1, ok ? "ok" : "BAD");
    return ok ? 0 : 1;
}

int main(int argc, char **argv)
{
    int bad = 0;
    for (int a = 1; a < argc; ++a) {
        const std::string arg = argv[a];
        if (arg == "--blocks" && a + 1 < argc) {
            const char *path = argv[++a], *emit = nullptr;
            if (a + 2 < argc && std::string(argv[a + 1]) == "--emit") { emit = argv[a + 2]; a += 2; }
            bad += run_blocks(path, emit);
        } else if (arg == "--mix" && a + 2 < argc) { bad += run_mix(atoi(argv[a + 1]), (unsigned)atoi(argv[a + 2])); a += 2; }
        else if (arg == "--builder") bad += run_builder();
        else if (arg == "--ratio" && a + 1 < argc) bad += run_ratio(argv[++a]);
        else { fprintf(stderr, "unknown argument %s\n", argv[a]); return 2; }
    }
    return bad ? 1 : 0;
}
