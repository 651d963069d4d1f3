// The fused step's three launches -- counting classify_kernel (or hist_kernel on given category bytes), scan_kernel,
// scatter_kernel -- executed on the CPU, lane by lane, under ASan + UBSan: xm_kernels.hip itself, compiled for the host through
// the lockstep shim (tests/lockstep/hip/hip_runtime.h: what it executes, what it cannot see).  Driven by
// tests/test_lockstep_place_cpu.py, which writes the cases and compares what this program dumps with the oracle.
//
// Per case this program does what fused_step / place_steps / compact_tail of xm_api.hip do (the chunk loop of place_steps is
// restated below); the launch geometry is the launchers' own.  Every buffer is a heap block of its own of exactly the size
// include/xenomapper_hip.h promises, so ASan sees the first byte past it.  Every case runs twice, the workspace
// (gran_counts, gran_off), the outputs and the LDS filled with 0x00 and with 0xA5 first: both runs must agree in every byte a
// call writes, leave everything else alone, and leave part_tot and the count replicas all zero (xm_workspace_is_clean).
//
//   lockstep_place_host cases.bin out.bin
#define XM_LOCKSTEP_HOST 1
#include "../xenomapper_amd/csrc/xm_kernels.hip"

#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

namespace {

const size_t COUNTS_REP_BYTES = (XM_COUNT_REPLICAS * 64 + 8) * sizeof(uint64_t);                 // as in xm_api.hip
const size_t PART_TOT_BYTES = (size_t)XM_PART_REPLICAS * 8 * XM_PART_STRIDE * sizeof(uint32_t);

enum { IN_BINS4 = 0, IN_CODE = 1, IN_HIST = 2 };
enum { TO_FLAT = 0, TO_LISTS = 1, TO_LISTS_STATE6 = 2 };

struct Variant {
    uint32_t mode, input, dest, waves, chunk_parts, flat_units;
    uint64_t cap;
};

// a heap block of exactly `bytes`, 64-byte aligned (the entry points ask for 4 to 32), filled
struct Block {
    void *p = nullptr;
    size_t bytes = 0;
    Block(size_t n, int fill) : bytes(n)
    {
        if (n == 0) return;
        if (posix_memalign(&p, 64, n) != 0) { fprintf(stderr, "out of memory\n"); exit(2); }
        memset(p, fill, n);
    }
    ~Block() { free(p); }
    Block(const Block &) = delete;
    template <typename T> T *as() const { return static_cast<T *>(p); }
};

struct Result {
    std::vector<uint64_t> counts, totals;
    std::vector<uint8_t> code, bins4;
    std::vector<uint32_t> flat, gran_counts, gran_off;
    std::vector<uint32_t> list[7];
    bool clean = true, untouched = true;
    bool operator==(const Result &o) const
    {
        for (int b = 0; b < 7; ++b)
            if (list[b] != o.list[b]) return false;
        return counts == o.counts && totals == o.totals && code == o.code && bins4 == o.bins4 && flat == o.flat &&
               gran_counts == o.gran_counts && gran_off == o.gran_off;
    }
};

template <typename T>
void run(const Variant &v, uint64_t n, const T *const col[4], const uint64_t *bits, T m, const uint8_t *given_code, int fill, Result &r)
{
    ls::set_fill(fill);
    if (v.waves) setenv("XM_SCATTER_WAVES", std::to_string(v.waves).c_str(), 1);
    else unsetenv("XM_SCATTER_WAVES");
    const bool lists = v.dest != TO_FLAT;
    xm::CountPlan cp;
    cp.plan = xm::plan_granules(n);
    const size_t gran_words = (size_t)8 * cp.plan.gran_stride;
    Block gran_counts(gran_words * 4, fill), gran_off(gran_words * 4, fill);
    Block counts_rep(COUNTS_REP_BYTES, 0), part_tot(PART_TOT_BYTES, 0);
    Block code(v.input == IN_BINS4 ? 0 : n, fill), bins4(v.input == IN_BINS4 ? XM_BINS4_BYTES(n) : 0, fill);
    Block totals(8 * 8, fill), counts(64 * 8, fill);
    Block flat(lists ? 0 : (size_t)v.flat_units * 4, fill);
    Block l0(lists ? v.cap * 4 : 0, fill), l1(lists ? v.cap * 4 : 0, fill), l2(lists ? v.cap * 4 : 0, fill), l3(lists ? v.cap * 4 : 0, fill),
        l4(lists ? v.cap * 4 : 0, fill), l5(lists ? v.cap * 4 : 0, fill), l6(v.dest == TO_LISTS_STATE6 ? v.cap * 4 : 0, fill);
    const Block *lb[7] = {&l0, &l1, &l2, &l3, &l4, &l5, &l6};
    xm::ListOut lo;
    for (int b = 0; b < 7; ++b) lo.p[b] = lb[b]->as<uint32_t>();
    lo.cap = (uint32_t)v.cap;
    if (v.input == IN_HIST) memcpy(code.p, given_code, n);

    cp.gran_counts = gran_counts.as<uint32_t>();
    cp.counts_rep = counts_rep.as<uint64_t>();
    cp.part_tot = part_tot.as<uint32_t>();
    cp.bins4 = bins4.as<uint8_t>();
    uint64_t *bin_totals = cp.counts_rep + XM_COUNT_REPLICAS * 64;
    const bool from_bins4 = cp.bins4 != nullptr;

    // place_steps: one pass over all granules, or (six lists, when asked for, more than two chunks) a chunk at a time
    const uint32_t n_gran = cp.plan.n_gran, chunk = lists ? v.chunk_parts * (uint32_t)XM_PART_GRAN : 0u;
    const bool chunked = chunk != 0u && n_gran > 2u * chunk;
    for (uint32_t g0 = 0; g0 < n_gran; g0 += chunked ? chunk : n_gran) {
        if (chunked) {
            cp.gran0 = g0;
            cp.gran1 = n_gran - g0 > chunk ? g0 + chunk : n_gran;
        }
        if (v.input == IN_HIST) xm::launch_hist(nullptr, (int)v.mode, n, code.as<uint8_t>(), cp);
        else xm::launch_classify<T>(nullptr, (int)v.mode, n, col[0], col[1], col[2], col[3], bits, m, code.as<uint8_t>(), &cp);
        xm::launch_scan(nullptr, cp, gran_off.as<uint32_t>(), bin_totals, counts.as<uint64_t>());
        xm::launch_scatter(nullptr, cp.plan, (int)v.mode, n, from_bins4 ? cp.bins4 : code.as<uint8_t>(), from_bins4, cp.gran_counts,
                           gran_off.as<uint32_t>(), bin_totals, totals.as<uint64_t>(), flat.as<uint32_t>(), cp.part_tot,
                           lists ? &lo : nullptr, cp.gran0, cp.gran1);
    }

    r.counts.assign(counts.as<uint64_t>(), counts.as<uint64_t>() + 64);
    r.totals.assign(totals.as<uint64_t>(), totals.as<uint64_t>() + 8);
    r.code.assign(code.as<uint8_t>(), code.as<uint8_t>() + code.bytes);
    r.bins4.assign(bins4.as<uint8_t>(), bins4.as<uint8_t>() + bins4.bytes);
    r.flat.assign(flat.as<uint32_t>(), flat.as<uint32_t>() + flat.bytes / 4);
    for (uint32_t b = 0; b < 8; ++b) {
        const uint32_t *c = gran_counts.as<uint32_t>() + (size_t)b * cp.plan.gran_stride, *o = gran_off.as<uint32_t>() + (size_t)b * cp.plan.gran_stride;
        r.gran_counts.insert(r.gran_counts.end(), c, c + n_gran);
        r.gran_off.insert(r.gran_off.end(), o, o + n_gran);
    }
    const uint32_t pattern = 0x01010101u * (uint32_t)fill;
    for (int b = 0; b < 7; ++b) {
        const uint64_t have = lb[b]->bytes / 4, len = r.totals[b] < have ? r.totals[b] : have;
        const uint32_t *p = lb[b]->as<uint32_t>();
        r.list[b].assign(p, p + len);
        for (uint64_t k = len; k < have; ++k)
            if (p[k] != pattern) r.untouched = false;                     // behind a list's entries nothing is written
    }
    for (size_t k = 0; k < PART_TOT_BYTES / 4; ++k)
        if (part_tot.as<uint32_t>()[k] != 0u) r.clean = false;
    for (size_t k = 0; k < XM_COUNT_REPLICAS * 64; ++k)
        if (counts_rep.as<uint64_t>()[k] != 0ull) r.clean = false;
}

template <typename V>
void put(FILE *fh, const std::vector<V> &v)
{
    const uint64_t k = v.size();
    fwrite(&k, 8, 1, fh);
    if (k) fwrite(v.data(), sizeof(V), k, fh);
}

template <typename T>
std::vector<T> get(FILE *fh, size_t k)
{
    std::vector<T> v(k);
    if (k && fread(v.data(), sizeof(T), k, fh) != k) { fprintf(stderr, "short case file\n"); exit(2); }
    return v;
}

template <typename T>
void run_cases(FILE *in, FILE *out, uint64_t n, double min_score, uint32_t n_variants)
{
    // the inputs too lie in blocks of exactly their size
    Block c0(n * sizeof(T), 0), c1(n * sizeof(T), 0), c2(n * sizeof(T), 0), c3(n * sizeof(T), 0), bits(((n + 63) / 64) * 8, 0), given(n, 0);
    const Block *cb[4] = {&c0, &c1, &c2, &c3};
    for (int k = 0; k < 4; ++k)
        if (fread(cb[k]->p, sizeof(T), n, in) != n) exit(2);
    if (fread(bits.p, 8, (n + 63) / 64, in) != (n + 63) / 64 || fread(given.p, 1, n, in) != n) exit(2);
    const T *col[4] = {c0.as<T>(), c1.as<T>(), c2.as<T>(), c3.as<T>()};
    const std::vector<Variant> vars = get<Variant>(in, n_variants);
    for (const Variant &v : vars) {
        Result a, b;
        run<T>(v, n, col, bits.as<uint64_t>(), (T)min_score, given.as<uint8_t>(), 0x00, a);
        run<T>(v, n, col, bits.as<uint64_t>(), (T)min_score, given.as<uint8_t>(), 0xA5, b);
        const uint32_t flags = (a == b ? 1u : 0u) | (a.clean && b.clean ? 2u : 0u) | (a.untouched && b.untouched ? 4u : 0u);
        fwrite(&flags, 4, 1, out);
        put(out, a.counts);
        put(out, a.totals);
        put(out, a.code);
        put(out, a.bins4);
        put(out, a.flat);
        for (int k = 0; k < 7; ++k) put(out, a.list[k]);
    }
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s cases.bin out.bin\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { perror("open"); return 2; }
    struct { uint32_t is_f64, n_variants; uint64_t n; double min_score; } h;
    static_assert(sizeof(Variant) == 32, "the case file's layout");
    if (fread(&h, sizeof h, 1, in) != 1) return 2;
    if (h.is_f64) run_cases<double>(in, out, h.n, h.min_score, h.n_variants);
    else run_cases<int32_t>(in, out, h.n, h.min_score, h.n_variants);
    fclose(in);
    if (fclose(out) != 0) return 2;
    printf("variants: %u, each run twice\n", h.n_variants);
    return 0;
}
