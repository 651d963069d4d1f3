// xm_samrec.h compiled for the host, alone, under ASan + UBSan (tests/test_samrec_core_host.py).  Reads a file of lines and a file of
// reference names (each: uint32 count, then per item uint32 length + bytes); every line is copied into a heap buffer of exactly its
// length plus the header's documented read margin, sized (step 1), and written (step 2) into a heap buffer of exactly that size
// between guard bytes -- whole, and again with SEQ / QUAL packed the way the device's wave does (64 interleaved shares).  Emits, per
// line and form (device, host): int32 reason, uint32 size, the record.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../xenomapper_amd/csrc/xm_samrec.h"

static std::vector<std::string> read_items(const char *path)
{
    std::vector<std::string> items;
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    uint32_t n = 0;
    if (fread(&n, 4, 1, f) != 1) exit(2);
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t len = 0;
        if (fread(&len, 4, 1, f) != 1) exit(2);
        std::string s(len, '\0');
        if (len && fread(&s[0], 1, len, f) != len) exit(2);
        items.push_back(s);
    }
    fclose(f);
    return items;
}

constexpr uint32_t GUARD = 32;

template <bool HOST> static int one(const std::string &text, const xmsam::RefHash &refs, FILE *out)
{
    const uint32_t n = (uint32_t)text.size();
    uint8_t *line = (uint8_t *)malloc(n + xmsam::READ_MARGIN + (n + xmsam::READ_MARGIN == 0 ? 1 : 0));
    memcpy(line, text.data(), n);
    const xmsam::Sized sz = xmsam::size_of<HOST>(line, n, refs);
    int bad = 0;
    std::vector<uint8_t> rec;
    if (sz.reason == xmsam::ENC_OK) {
        for (int wave = 0; wave < 2; ++wave) {
            uint8_t *buf = (uint8_t *)malloc(sz.size + 2 * GUARD);
            memset(buf, 0xA5, sz.size + 2 * GUARD);
            uint8_t *dst = buf + GUARD;
            xmsam::Bulk bulk;
            const int32_t rc = xmsam::write<HOST>(line, n, refs, 0, sz, dst, wave ? &bulk : nullptr);
            if (rc != xmsam::ENC_OK) { fprintf(stderr, "write: reason %d behind size_of's 0\n", rc); ++bad; }
            if (wave && rc == xmsam::ENC_OK)
                for (uint32_t lane = 0; lane < 64; ++lane) {
                    xmsam::pack_seq(line + bulk.seq_src, bulk.l_seq, dst + bulk.seq_dst, lane, 64);
                    xmsam::pack_qual(bulk.qual_src == ~0u ? nullptr : line + bulk.qual_src, bulk.l_seq, dst + bulk.qual_dst, lane, 64);
                }
            for (uint32_t k = 0; k < GUARD; ++k)
                if (buf[k] != 0xA5 || buf[GUARD + sz.size + k] != 0xA5) { fprintf(stderr, "guard byte %u overwritten\n", k); ++bad; break; }
            if (!wave) rec.assign(dst, dst + sz.size);
            else if (rec.size() != sz.size || memcmp(rec.data(), dst, sz.size) != 0) { fprintf(stderr, "the wave's shares differ\n"); ++bad; }
            free(buf);
        }
    }
    if (memcmp(line, text.data(), n) != 0) { fprintf(stderr, "the line was written to\n"); ++bad; }
    free(line);
    const int32_t reason = sz.reason;
    const uint32_t size = sz.size;
    fwrite(&reason, 4, 1, out);
    fwrite(&size, 4, 1, out);
    if (size) fwrite(rec.data(), 1, size, out);
    return bad;
}

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: %s lines.bin refs.bin out.bin\n", argv[0]); return 2; }
    const std::vector<std::string> lines = read_items(argv[1]), names = read_items(argv[2]);
    std::vector<uint8_t> blob;
    std::vector<uint32_t> at(1, 0u), table;
    for (const std::string &s : names) { blob.insert(blob.end(), s.begin(), s.end()); at.push_back((uint32_t)blob.size()); }
    uint32_t mask = 0;
    if (!xmsam::build_ref_table(blob.data(), at.data(), (uint32_t)names.size(), table, mask)) { fprintf(stderr, "duplicate name\n"); return 2; }
    const xmsam::RefHash refs{blob.data(), at.data(), table.data(), mask, (uint32_t)names.size()};
    // every name is found at its index, through the table (some past their home entry), and a name cut short is not
    uint32_t displaced = 0;
    for (uint32_t i = 0; i < names.size(); ++i) {
        const uint8_t *p = blob.data() + at[i];
        const uint32_t len = at[i + 1] - at[i];
        if (refs.find(p, len) != (int32_t)i) return 3;
        const int32_t cut = refs.find(p, len - 1);                          // a name cut short: another name of that length, or none
        if (cut >= 0 && (names[cut].size() != len - 1 || memcmp(names[cut].data(), p, len - 1) != 0)) return 3;
        const uint32_t home = xmsam::RefHash::hash(p, len) & mask;
        displaced += table[2 * home + 1] != i + 1 ? 1u : 0u;
    }
    FILE *out = fopen(argv[3], "wb");
    if (!out) { perror(argv[3]); return 2; }
    int bad = 0;
    for (const std::string &s : lines) { bad += one<false>(s, refs, out); bad += one<true>(s, refs, out); }
    fclose(out);
    printf("lines: %zu, %d failures, names: %zu, displaced %u, table %u\n", lines.size(), bad, names.size(), displaced, mask + 1);
    return bad ? 1 : 0;
}
