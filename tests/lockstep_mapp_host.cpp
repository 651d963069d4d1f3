// The launches of the single-end mappability front end (xenomapper_amd/csrc/xm_mapp_kernels.h: M1 .. M6) executed on the CPU, lane by
// lane, under ASan + UBSan, through the lockstep shim (tests/lockstep).  tests/test_lockstep_mapp_cpu.py writes the windows of the
// catalogue (tests/mapp_shapes.py) and compares what this program dumps with the model.
//
//   lockstep_mapp_host <cases> <out>
//
// cases: u32 n, then per window: u64 max_lines, u64 max_values, u32 len, u32 eof, u32 has_carry, u32 carry_position, u32 key_len,
// the key, the window.  Every buffer is a heap block of exactly the size xmm::sizes_for() gives for (len, max_lines, max_values), as
// xm_mapp.hip reserves them (which rounds small ones up); each window runs twice, all buffers and LDS filled with 0x00, then 0xA5.
// out, per window: u32 flags (1: both runs gave the same), the SUM_WORDS summary words, the segment rows, the values.
#define XM_LOCKSTEP_HOST 1
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <string.h>

#include <vector>

// ---- what the shim does not model, in its terms ---------------------------------------------------------------------------------
template <typename T>
static inline T ls_shfl_up(T v, unsigned delta, int line)
{
    ls::rendezvous(ls::OP_SHFL, line, ls::to_bits(v));
    const int from = ls::cur->id - (int)delta;
    return from < 0 ? v : ls::from_bits<T>(ls::value_of(from, "__shfl_up", line));
}
#define __shfl_up(v, d) ls_shfl_up((v), (d), __builtin_LINE())

static inline uint32_t atomicMax(uint32_t *p, uint32_t v)
{
    uint32_t old = __atomic_load_n(p, __ATOMIC_SEQ_CST);
    while (old < v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {}
    return old;
}
static inline unsigned long long atomicMin(unsigned long long *p, unsigned long long v)
{
    unsigned long long old = __atomic_load_n(p, __ATOMIC_SEQ_CST);
    while (old > v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {}
    return old;
}

#include "../xenomapper_amd/csrc/xm_mapp_kernels.h"

namespace {

struct Reader {
    FILE *fh;
    template <typename T> T get()
    {
        T v;
        if (fread(&v, sizeof v, 1, fh) != 1) { fprintf(stderr, "short case file\n"); exit(2); }
        return v;
    }
    std::vector<uint8_t> bytes(size_t n)
    {
        std::vector<uint8_t> v(n);
        if (n && fread(v.data(), 1, n, fh) != n) { fprintf(stderr, "short case file\n"); exit(2); }
        return v;
    }
};

template <typename T>
T *block_of(size_t count, int fill)                        // exactly `count` elements (one byte when there are none), all `fill`
{
    const size_t bytes = count * sizeof(T);
    void *p = malloc(bytes ? bytes : 1);                   // (ASan's redzone begins at the block's last byte)
    if (!p) { fprintf(stderr, "out of memory\n"); exit(2); }
    memset(p, fill, bytes);
    return (T *)p;
}

struct Result {
    std::vector<xmm::u64> summary;
    std::vector<xmm::Seg> segs;
    std::vector<uint8_t> values;
    bool operator==(const Result &o) const
    {
        return summary == o.summary && values == o.values && segs.size() == o.segs.size() &&
               (segs.empty() || memcmp(segs.data(), o.segs.data(), segs.size() * sizeof(xmm::Seg)) == 0);
    }
};

Result run_window(const std::vector<uint8_t> &window, uint32_t eof, const std::vector<uint8_t> &key, uint32_t has_carry,
                  uint32_t carry_position, uint64_t max_lines, uint64_t max_values, int fill)
{
    ls::set_fill(fill);
    const uint32_t len = (uint32_t)window.size();
    const xmm::Sizes z = xmm::sizes_for(len ? len : 1, max_lines, max_values);
    uint8_t *staging = block_of<uint8_t>(z.text, fill), *text = block_of<uint8_t>(z.text, fill);
    memcpy(staging, window.data(), len);
    xmm::Job job;
    memset(&job, 0, sizeof job);
    job.text = text;
    job.len = len;
    job.eof = eof;
    job.n_chunks = (len + xmm::CHUNK - 1) / xmm::CHUNK;
    job.mask16 = block_of<uint16_t>(z.mask16, fill);
    job.chunk_cnt = block_of<uint32_t>(z.chunk_cnt, fill);
    job.chunk_base = block_of<uint32_t>(z.chunk_cnt, fill);
    job.cap_lines = (uint32_t)max_lines;
    job.lend = block_of<uint32_t>(z.lines, fill);
    job.np = block_of<uint32_t>(z.lines, fill);
    job.tlen = block_of<uint32_t>(z.lines, fill);
    job.roff = block_of<uint32_t>(z.lines, fill);
    job.rlen = block_of<uint32_t>(z.lines, fill);
    job.seg_of = block_of<uint32_t>(z.lines, fill);
    job.flags = block_of<uint8_t>(z.lines, fill);
    job.part = block_of<uint32_t>(z.tiles, fill);
    job.part_base = block_of<uint32_t>(z.tiles, fill);
    job.vpart = block_of<xmm::u64>(z.tiles, fill);
    job.vbase = block_of<xmm::u64>(z.tiles, fill);
    job.segs = block_of<xmm::Seg>(z.lines, fill);
    job.values = block_of<uint8_t>(z.values, fill);
    job.max_values = max_values;
    job.state = block_of<uint32_t>(xmm::ST_WORDS, 0);              // (the front end clears these in front of M1)
    job.keys = block_of<xmm::u64>(xmm::K_WORDS, fill);
    job.summary = block_of<xmm::u64>(xmm::SUM_WORDS, fill);
    uint8_t *carry = block_of<uint8_t>(key.size(), fill);
    if (!key.empty()) memcpy(carry, key.data(), key.size());
    job.carry_key = carry;
    job.carry_key_len = has_carry ? (uint32_t)key.size() : 0u;
    job.has_carry = has_carry;
    job.carry_position = has_carry ? carry_position : 0u;

    if (job.n_chunks) {
        xmm::MarkArgs a;
        a.src = staging; a.copy = text; a.mask16 = job.mask16; a.chunk_cnt = job.chunk_cnt; a.state = job.state;
        a.len = len; a.chunk0 = 0; a.n_chunks = job.n_chunks;
        XMM_LAUNCH(xmm::mark_kernel, dim3(a.n_chunks), dim3(xmm::MB), nullptr, a);
    }
    xmm::enqueue_behind_mark(job, nullptr);

    Result r;
    r.summary.assign(job.summary, job.summary + xmm::SUM_CONSUMED + 9);
    const xmm::u64 n_seg = job.summary[xmm::SUM_NSEG], n_values = job.summary[xmm::SUM_NVALUES];
    if (n_seg > max_lines || n_values > max_values) { fprintf(stderr, "the summary exceeds the limits\n"); exit(1); }
    r.segs.assign(job.segs, job.segs + n_seg);
    r.values.assign(job.values, job.values + n_values);
    void *all[] = {staging, text, job.mask16, job.chunk_cnt, job.chunk_base, job.lend, job.np, job.tlen, job.roff, job.rlen, job.seg_of,
                   job.flags, job.part, job.part_base, job.vpart, job.vbase, job.segs, job.values, job.state, job.keys, job.summary, carry};
    for (void *p : all) free(p);
    return r;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: lockstep_mapp_host <cases> <out>\n"); return 2; }
    Reader in{fopen(argv[1], "rb")};
    FILE *out = fopen(argv[2], "wb");
    if (!in.fh || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    const uint32_t n_cases = in.get<uint32_t>();
    for (uint32_t c = 0; c < n_cases; ++c) {
        const uint64_t max_lines = in.get<uint64_t>(), max_values = in.get<uint64_t>();
        const uint32_t len = in.get<uint32_t>(), eof = in.get<uint32_t>(), has_carry = in.get<uint32_t>(), carry_position = in.get<uint32_t>(),
                       key_len = in.get<uint32_t>();
        const std::vector<uint8_t> key = in.bytes(key_len), window = in.bytes(len);
        const Result a = run_window(window, eof, key, has_carry, carry_position, max_lines, max_values, 0x00);
        const Result b = run_window(window, eof, key, has_carry, carry_position, max_lines, max_values, 0xA5);
        const uint32_t flags = a == b ? 1u : 0u;
        fwrite(&flags, sizeof flags, 1, out);
        fwrite(b.summary.data(), sizeof(xmm::u64), b.summary.size(), out);
        if (!b.segs.empty()) fwrite(b.segs.data(), sizeof(xmm::Seg), b.segs.size(), out);
        if (!b.values.empty()) fwrite(b.values.data(), 1, b.values.size(), out);
    }
    fclose(in.fh);
    fclose(out);
    return 0;
}
