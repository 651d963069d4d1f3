// Every launcher of xm_kernels.hip that tests/lockstep_place_host.cpp does not run -- K1r (classify_runs_kernel + runs_finish_kernel),
// K3 (cigar_kernel), K1c (classify_cigar_kernel), K1p (classify_cigp_kernel, followed by scan_kernel and scatter_kernel as the fused
// step of xm_api.hip follows it), the non-counting classify_kernel, mate_correlate_kernel and stream_probe_kernel -- executed on the
// CPU, lane by lane, under ASan + UBSan: xm_kernels.hip itself, compiled for the host through the lockstep shim
// (tests/lockstep/hip/hip_runtime.h: what it executes, what it cannot see).  Driven by tests/test_lockstep_kernels_cpu.py, which
// writes the cases and compares what this program dumps with the oracles.
//
// The launch geometry is the launchers' own.  Every input and output is a heap block of its own of exactly the size
// include/xenomapper_hip.h promises, placed as its table of placements allows and no better (a block that must be 4-byte aligned
// lies 4 bytes off a multiple of 8, and so on), so ASan sees the first byte past it and UBSan a load that assumes more alignment
// than promised.  Every case runs twice: outputs and workspace filled with 0xA5 and the LDS with 0x00 first, then the other way
// round (never the same byte in both: a stale LDS word stored behind an output's last entry would look like the fill).  Per case
// the program dumps what the calls wrote and a word of flags: 1 = both runs agree in every byte a call writes, 2 = part_tot and
// the count replicas are all zero afterwards, 4 = everything else still holds the fill.
//
//   lockstep_kernels_host cases.bin out.bin
//
// Both files are sequences of blobs (a uint64 byte count, then the bytes).  A case is a blob of uint64 parameters -- the first one
// names the kernel family -- followed by its input arrays; see the run_* functions for the order.
#define XM_LOCKSTEP_HOST 1
#include "../xenomapper_amd/csrc/xm_kernels.hip"

#include <stdio.h>
#include <string.h>

#include <vector>

#ifdef LS_ASAN
#include <sanitizer/asan_interface.h>
#endif

namespace {

const size_t COUNTS_REP_BYTES = (XM_COUNT_REPLICAS * 64 + 8) * sizeof(uint64_t);                 // as in xm_api.hip
const size_t PART_TOT_BYTES = (size_t)XM_PART_REPLICAS * 8 * XM_PART_STRIDE * sizeof(uint32_t);

enum { CMD_RUNS = 1, CMD_CIGAR = 2, CMD_K1C = 3, CMD_K1P = 4, CMD_CLASSIFY = 5, CMD_CORRELATE = 6, CMD_PROBE = 7 };
enum { AGREE = 1u, CLEAN = 2u, UNTOUCHED = 4u };

typedef std::vector<uint8_t> Bytes;

// a heap block of exactly `bytes` that is `align`-byte aligned and not 2 * align-byte aligned (align <= 32); the bytes in front
// of it inside the allocation are poisoned, the allocation ends with the block
struct Block {
    char *raw = nullptr;
    void *p = nullptr;
    size_t bytes = 0, pad = 0;
    Block(size_t n, size_t align, int fill) : bytes(n), pad(align)
    {
        if (posix_memalign((void **)&raw, 64, n + pad) != 0) { fprintf(stderr, "out of memory\n"); exit(2); }
        p = raw + pad;
        if (n) memset(p, fill, n);
#ifdef LS_ASAN
        __asan_poison_memory_region(raw, pad);
#endif
    }
    Block(const Bytes &src, size_t align) : Block(src.size(), align, 0)
    {
        if (bytes) memcpy(p, src.data(), bytes);
    }
    ~Block()
    {
#ifdef LS_ASAN
        __asan_unpoison_memory_region(raw, pad);
#endif
        free(raw);
    }
    Block(const Block &) = delete;
    template <typename T> T *as() const { return static_cast<T *>(p); }
    Bytes copy() const { return Bytes(as<uint8_t>(), as<uint8_t>() + bytes); }
    bool holds(int fill, size_t from = 0) const
    {
        for (size_t k = from; k < bytes; ++k)
            if (as<uint8_t>()[k] != (uint8_t)fill) return false;
        return true;
    }
};

// the context's counting workspace, as xm_api.hip keeps it: all zero between calls
struct Workspace {
    Block counts_rep, part_tot;
    explicit Workspace(bool parts) : counts_rep(COUNTS_REP_BYTES, 8, 0), part_tot(parts ? PART_TOT_BYTES : 0, 4, 0) {}   // K1r has no part totals
    bool clean() const
    {
        for (size_t k = 0; k < XM_COUNT_REPLICAS * 64; ++k)
            if (counts_rep.as<uint64_t>()[k] != 0ull) return false;
        return part_tot.holds(0);
    }
};

FILE *g_in, *g_out;

bool get(Bytes &b)
{
    uint64_t k;
    if (fread(&k, 8, 1, g_in) != 1) return false;
    b.resize(k);
    if (k && fread(b.data(), 1, k, g_in) != k) { fprintf(stderr, "short case file\n"); exit(2); }
    return true;
}

Bytes need()
{
    Bytes b;
    if (!get(b)) { fprintf(stderr, "short case file\n"); exit(2); }
    return b;
}

void put(const Bytes &b)
{
    const uint64_t k = b.size();
    fwrite(&k, 8, 1, g_out);
    if (k) fwrite(b.data(), 1, k, g_out);
}

void put_flags(uint32_t flags)
{
    put(Bytes((const uint8_t *)&flags, (const uint8_t *)&flags + 4));
}

double as_double(uint64_t bits)
{
    double d;
    memcpy(&d, &bits, 8);
    return d;
}

template <typename T> T min_score_of(uint64_t bits) { return (T)as_double(bits); }

void check_size(const Bytes &b, size_t want, const char *what)
{
    if (b.size() != want) { fprintf(stderr, "%s: %zu bytes, expected %zu\n", what, b.size(), want); exit(2); }
}

// ---- K1r: launch_classify_runs<T>, launch_runs_finish --------------------------------------------------------------------
// parameters: is_f64, mode, n, min_score (binary64 bits); arrays: as1, xs1, as2, xs2, unit_bits
// dumps: flags, runs16 of the run on 0xA5 memory, runs16 of the run on 0x00 memory (all of it: the test looks at the entries nobody wrote too),
//        gran_counts, n_out, counts
template <typename T>
void run_runs(const uint64_t *par)
{
    const int mode = (int)par[2];
    const uint64_t n = par[3];
    const T m = min_score_of<T>(par[4]);
    const Bytes c[4] = {need(), need(), need(), need()}, bits = need();
    for (int k = 0; k < 4; ++k) check_size(c[k], n * sizeof(T), "score column");
    check_size(bits, ((n + 63) / 64) * 8, "unit_bits");
    const Block c0(c[0], 4 * sizeof(T)), c1(c[1], 4 * sizeof(T)), c2(c[2], 4 * sizeof(T)), c3(c[3], 4 * sizeof(T)), ub(bits, 8);
    const uint64_t n_gran = XM_RUNS_GRANULES(n);
    Bytes runs[2], gc[2], n_out[2], counts[2];
    uint32_t flags = AGREE | CLEAN | UNTOUCHED;
    for (int r = 0; r < 2; ++r) {
        const int fill = r ? 0x00 : 0xA5;                                   // memory; the LDS holds the other pattern
        ls::set_fill(fill ^ 0xA5);
        Workspace ws(false);
        Block runs16(XM_RUNS16_ENTRIES(n) * 2, 16, fill), gran_counts(n_gran * 8 * 2, 16, fill), no(8 * 8, 8, fill), cn(64 * 8, 8, fill);
        const xm::RunsOut ro = {runs16.as<uint16_t>(), gran_counts.as<uint16_t>(), ws.counts_rep.as<uint64_t>()};
        xm::launch_classify_runs<T>(nullptr, mode, n, c0.as<T>(), c1.as<T>(), c2.as<T>(), c3.as<T>(), ub.as<uint64_t>(), m, ro);
        xm::launch_runs_finish(nullptr, mode, ws.counts_rep.as<uint64_t>(), cn.as<uint64_t>(), no.as<uint64_t>());
        runs[r] = runs16.copy(); gc[r] = gran_counts.copy(); n_out[r] = no.copy(); counts[r] = cn.copy();
        if (!ws.clean()) flags &= ~CLEAN;
        const uint16_t pattern = (uint16_t)(0x0101 * fill);
        for (uint64_t g = 0; g < n_gran; ++g) {
            uint32_t units = 0;
            for (int b = 0; b < 8; ++b) units += gran_counts.as<uint16_t>()[g * 8 + b];
            for (uint64_t e = units; e < XM_RUNS_GRAN; ++e)
                if (runs16.as<uint16_t>()[g * XM_RUNS_GRAN + e] != pattern) flags &= ~UNTOUCHED;
        }
    }
    if (gc[0] != gc[1] || n_out[0] != n_out[1] || counts[0] != counts[1]) flags &= ~AGREE;
    for (uint64_t g = 0; g < n_gran; ++g) {
        uint32_t units = 0;
        for (int b = 0; b < 8; ++b) units += ((const uint16_t *)gc[0].data())[g * 8 + b];
        if (units > XM_RUNS_GRAN) units = XM_RUNS_GRAN;
        if (memcmp(runs[0].data() + g * XM_RUNS_GRAN * 2, runs[1].data() + g * XM_RUNS_GRAN * 2, units * 2) != 0) flags &= ~AGREE;
    }
    put_flags(flags);
    put(runs[0]); put(runs[1]); put(gc[0]); put(n_out[0]); put(counts[0]);
}

// the caller's range_flag: a 4-byte block of its own, zero before the call (the library never clears it), or none
struct Flag {
    Block b;
    bool none;
    explicit Flag(bool none_) : b(4, 4, 0), none(none_) {}
    uint32_t *ptr() const { return none ? nullptr : b.as<uint32_t>(); }
};

// ---- K3: launch_cigar ----------------------------------------------------------------------------------------------------
// parameters: n, max_blocks, range_flag is null; arrays: nm, cig_off (n + 1 words), cig_oplen (cig_off[n] words)
// dumps: flags, as_out, range_flag
void run_cigar(const uint64_t *par)
{
    const uint64_t n = par[1];
    const Bytes nm = need(), off = need(), ops = need();
    check_size(nm, n * 4, "nm");
    check_size(off, (n + 1) * 4, "cig_off");
    check_size(ops, (size_t)((const uint32_t *)off.data())[n] * 4, "cig_oplen");
    const Block b_nm(nm, 4), b_off(off, 4), b_ops(ops, 4);
    Bytes out[2], fl[2];
    uint32_t flags = AGREE | CLEAN | UNTOUCHED;
    for (int r = 0; r < 2; ++r) {
        const int fill = r ? 0x00 : 0xA5;                                   // memory; the LDS holds the other pattern
        ls::set_fill(fill ^ 0xA5);
        Block as_out(n * 4, 4, fill);
        const Flag flag(par[3] != 0);
        xm::launch_cigar(nullptr, (uint32_t)par[2], n, b_nm.as<int32_t>(), b_off.as<uint32_t>(), b_ops.as<uint32_t>(), as_out.as<int32_t>(), flag.ptr());
        out[r] = as_out.copy(); fl[r] = flag.b.copy();
    }
    if (out[0] != out[1] || fl[0] != fl[1]) flags &= ~AGREE;
    put_flags(flags);
    put(out[0]); put(fl[0]);
}

// ---- K1c: launch_classify_cigar ------------------------------------------------------------------------------------------
// parameters: n, mode, min_score_floor (binary64 bits), range_flag is null
// arrays: nm1, cig_off1, cig_oplen1, xs1, nm2, cig_off2, cig_oplen2, xs2, unit_bits
// dumps: flags, code, range_flag
void run_k1c(const uint64_t *par)
{
    const uint64_t n = par[1];
    const int mode = (int)par[2];
    const int32_t m = min_score_of<int32_t>(par[3]);
    Bytes a[8];
    for (int k = 0; k < 8; ++k) a[k] = need();
    const Bytes bits = need();
    for (int s = 0; s < 2; ++s) {
        check_size(a[4 * s], n * 4, "nm");
        check_size(a[4 * s + 1], (n + 1) * 4, "cig_off");
        check_size(a[4 * s + 2], (size_t)((const uint32_t *)a[4 * s + 1].data())[n] * 4, "cig_oplen");
        check_size(a[4 * s + 3], n * 4, "xs");
    }
    check_size(bits, ((n + 63) / 64) * 8, "unit_bits");
    // nm, xs and cig_off are read four records a lane: 16 bytes; cig_oplen a dword at a time: 4
    const Block nm1(a[0], 16), off1(a[1], 16), ops1(a[2], 4), xs1(a[3], 16), nm2(a[4], 16), off2(a[5], 16), ops2(a[6], 4), xs2(a[7], 16), ub(bits, 8);
    Bytes out[2], fl[2];
    uint32_t flags = AGREE | CLEAN | UNTOUCHED;
    for (int r = 0; r < 2; ++r) {
        const int fill = r ? 0x00 : 0xA5;                                   // memory; the LDS holds the other pattern
        ls::set_fill(fill ^ 0xA5);
        Block code(n, 4, fill);
        const Flag flag(par[4] != 0);
        xm::launch_classify_cigar(nullptr, mode, n, nm1.as<int32_t>(), off1.as<uint32_t>(), ops1.as<uint32_t>(), xs1.as<int32_t>(),
                                  nm2.as<int32_t>(), off2.as<uint32_t>(), ops2.as<uint32_t>(), xs2.as<int32_t>(), ub.as<uint64_t>(), m,
                                  code.as<uint8_t>(), flag.ptr());
        out[r] = code.copy(); fl[r] = flag.b.copy();
    }
    if (out[0] != out[1] || fl[0] != fl[1]) flags &= ~AGREE;
    put_flags(flags);
    put(out[0]); put(fl[0]);
}

// ---- K1p: launch_classify_cigp, launch_scan, launch_scatter (the fused step on packed columns, one flat list) ------------------
// parameters: n, mode, min_score_floor (binary64 bits), range_flag is null, form (0: the compact stream only, 1: category bytes
//             only), entries of idx_out
// arrays: per species nm, cig_cnt (n bytes), cig_tile (XM_CIG_TILES(n) + 1 words), cig_oplen (cig_tile[last] words), xs; unit_bits
// dumps: flags, code, bins4, idx_out[0 .. bin_offsets[7]), bin_offsets, counts, range_flag, and of the second run bin_offsets, counts
void run_k1p(const uint64_t *par)
{
    const uint64_t n = par[1], idx_entries = par[6];
    const int mode = (int)par[2];
    const int32_t m = min_score_of<int32_t>(par[3]);
    const bool with_bins4 = par[5] == 0;
    Bytes a[10];
    for (int k = 0; k < 10; ++k) a[k] = need();
    const Bytes bits = need();
    const uint64_t n_tiles = XM_CIG_TILES(n);
    for (int s = 0; s < 2; ++s) {
        check_size(a[5 * s], n * 4, "nm");
        check_size(a[5 * s + 1], n, "cig_cnt");
        check_size(a[5 * s + 2], (n_tiles + 1) * 4, "cig_tile");
        check_size(a[5 * s + 3], (size_t)((const uint32_t *)a[5 * s + 2].data())[n_tiles] * 4, "cig_oplen");
        check_size(a[5 * s + 4], n * 4, "xs");
    }
    check_size(bits, ((n + 63) / 64) * 8, "unit_bits");
    const Block nm1(a[0], 16), cnt1(a[1], 4), tile1(a[2], 4), ops1(a[3], 4), xs1(a[4], 16);
    const Block nm2(a[5], 16), cnt2(a[6], 4), tile2(a[7], 4), ops2(a[8], 4), xs2(a[9], 16), ub(bits, 8);
    const xm::CigCols s1 = {nm1.as<int32_t>(), xs1.as<int32_t>(), cnt1.as<uint8_t>(), tile1.as<uint32_t>(), ops1.as<uint32_t>()};
    const xm::CigCols s2 = {nm2.as<int32_t>(), xs2.as<int32_t>(), cnt2.as<uint8_t>(), tile2.as<uint32_t>(), ops2.as<uint32_t>()};
    Bytes o_code[2], o_bins4[2], o_idx[2], o_tot[2], o_counts[2], o_flag[2];
    uint32_t flags = AGREE | CLEAN | UNTOUCHED;
    for (int r = 0; r < 2; ++r) {
        const int fill = r ? 0x00 : 0xA5;                                   // memory; the LDS holds the other pattern
        ls::set_fill(fill ^ 0xA5);
        Workspace ws(true);
        xm::CountPlan cp;
        cp.plan = xm::plan_granules(n);
        const size_t gran_words = (size_t)8 * cp.plan.gran_stride;
        Block gran_counts(gran_words * 4, 4, fill), gran_off(gran_words * 4, 4, fill);
        Block code(with_bins4 ? 0 : n, 16, fill), bins4(with_bins4 ? XM_BINS4_BYTES(n) : 0, 16, fill);
        Block idx(idx_entries * 4, 4, fill), totals(8 * 8, 8, fill), counts(64 * 8, 8, fill);
        const Flag flag(par[4] != 0);
        cp.gran_counts = gran_counts.as<uint32_t>();
        cp.counts_rep = ws.counts_rep.as<uint64_t>();
        cp.part_tot = ws.part_tot.as<uint32_t>();
        cp.bins4 = with_bins4 ? bins4.as<uint8_t>() : nullptr;
        uint8_t *code_out = with_bins4 ? nullptr : code.as<uint8_t>();
        uint64_t *bin_totals = cp.counts_rep + XM_COUNT_REPLICAS * 64;
        xm::launch_classify_cigp(nullptr, mode, n, s1, s2, ub.as<uint64_t>(), m, code_out, flag.ptr(), cp);
        xm::launch_scan(nullptr, cp, gran_off.as<uint32_t>(), bin_totals, counts.as<uint64_t>());
        xm::launch_scatter(nullptr, cp.plan, mode, n, with_bins4 ? cp.bins4 : code_out, with_bins4, cp.gran_counts, gran_off.as<uint32_t>(),
                           bin_totals, totals.as<uint64_t>(), idx.as<uint32_t>(), cp.part_tot, nullptr, 0, 0);
        o_code[r] = code.copy(); o_bins4[r] = bins4.copy(); o_tot[r] = totals.copy(); o_counts[r] = counts.copy(); o_flag[r] = flag.b.copy();
        const uint64_t units = totals.as<uint64_t>()[7] < idx_entries ? totals.as<uint64_t>()[7] : idx_entries;
        o_idx[r].assign(idx.as<uint8_t>(), idx.as<uint8_t>() + units * 4);
        if (!idx.holds(fill, units * 4)) flags &= ~UNTOUCHED;                // behind the list's entries nothing is written
        if (!ws.clean()) flags &= ~CLEAN;
    }
    if (o_code[0] != o_code[1] || o_bins4[0] != o_bins4[1] || o_idx[0] != o_idx[1] || o_tot[0] != o_tot[1] || o_counts[0] != o_counts[1] ||
        o_flag[0] != o_flag[1])
        flags &= ~AGREE;
    put_flags(flags);
    put(o_code[0]); put(o_bins4[0]); put(o_idx[0]); put(o_tot[0]); put(o_counts[0]); put(o_flag[0]); put(o_tot[1]); put(o_counts[1]);
}

// ---- the plain classify: launch_classify<T> without a count plan (xm_classify_dev, xm_classify_f64_dev) -----------------------
// parameters: is_f64, mode, n, min_score (binary64 bits); arrays: as1, xs1, as2, xs2, unit_bits; dumps: flags, code
template <typename T>
void run_classify(const uint64_t *par)
{
    const int mode = (int)par[2];
    const uint64_t n = par[3];
    const T m = min_score_of<T>(par[4]);
    const Bytes c[4] = {need(), need(), need(), need()}, bits = need();
    for (int k = 0; k < 4; ++k) check_size(c[k], n * sizeof(T), "score column");
    check_size(bits, ((n + 63) / 64) * 8, "unit_bits");
    const Block c0(c[0], 4 * sizeof(T)), c1(c[1], 4 * sizeof(T)), c2(c[2], 4 * sizeof(T)), c3(c[3], 4 * sizeof(T)), ub(bits, 8);
    Bytes out[2];
    for (int r = 0; r < 2; ++r) {
        const int fill = r ? 0x00 : 0xA5;                                   // memory; the LDS holds the other pattern
        ls::set_fill(fill ^ 0xA5);
        Block code(n, 4, fill);
        xm::launch_classify<T>(nullptr, mode, n, c0.as<T>(), c1.as<T>(), c2.as<T>(), c3.as<T>(), ub.as<uint64_t>(), m, code.as<uint8_t>(), nullptr);
        out[r] = code.copy();
    }
    put_flags((out[0] == out[1] ? AGREE : 0u) | CLEAN | UNTOUCHED);
    put(out[0]);
}

// ---- K4: launch_mate_correlate -------------------------------------------------------------------------------------------
// parameters: n, m; arrays: track (n binary64), density (m: a block of no bytes when m == 0); dumps: flags, out
void run_correlate(const uint64_t *par)
{
    const uint64_t n = par[1], m = par[2];
    const Bytes track = need(), density = need();
    check_size(track, n * 8, "track");
    check_size(density, m * 8, "density");
    const Block t(track, 8), d(density, 8);
    Bytes out[2];
    for (int r = 0; r < 2; ++r) {
        const int fill = r ? 0x00 : 0xA5;                                   // memory; the LDS holds the other pattern
        ls::set_fill(fill ^ 0xA5);
        Block o(n * 8, 8, fill);
        xm::launch_mate_correlate(nullptr, n, t.as<double>(), (uint32_t)m, d.as<double>(), o.as<double>());
        out[r] = o.copy();
    }
    put_flags((out[0] == out[1] ? AGREE : 0u) | CLEAN | UNTOUCHED);
    put(out[0]);
}

// ---- launch_stream_probe ---------------------------------------------------------------------------------------------------
// parameters: n; arrays: c0..c3 (n int32 each); dumps: flags (4 = nothing behind the n / 4 values it writes; ASan watches the
// end of the XM_BINS4_BYTES(n) bytes).  The values mean nothing.
void run_probe(const uint64_t *par)
{
    const uint64_t n = par[1];
    const Bytes c[4] = {need(), need(), need(), need()};
    for (int k = 0; k < 4; ++k) check_size(c[k], n * 4, "column");
    const Block c0(c[0], 16), c1(c[1], 16), c2(c[2], 16), c3(c[3], 16);
    uint32_t flags = AGREE | CLEAN | UNTOUCHED;
    Bytes out[2];
    for (int r = 0; r < 2; ++r) {
        const int fill = r ? 0x00 : 0xA5;                                   // memory; the LDS holds the other pattern
        ls::set_fill(fill ^ 0xA5);
        Block o(XM_BINS4_BYTES(n), 2, fill);
        xm::launch_stream_probe(nullptr, n, c0.as<int32_t>(), c1.as<int32_t>(), c2.as<int32_t>(), c3.as<int32_t>(), o.as<uint8_t>());
        if (!o.holds(fill, (n / 4) * 2)) flags &= ~UNTOUCHED;
        out[r].assign(o.as<uint8_t>(), o.as<uint8_t>() + (n / 4) * 2);
    }
    if (out[0] != out[1]) flags &= ~AGREE;
    put_flags(flags);
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s cases.bin out.bin\n", argv[0]); return 2; }
    g_in = fopen(argv[1], "rb");
    g_out = fopen(argv[2], "wb");
    if (!g_in || !g_out) { perror("open"); return 2; }
    Bytes head;
    unsigned cases = 0;
    while (get(head)) {
        if (head.size() < 8 * 8 || head.size() % 8) { fprintf(stderr, "a case begins with eight parameters at least\n"); return 2; }
        std::vector<uint64_t> par(head.size() / 8);
        memcpy(par.data(), head.data(), head.size());
        switch (par[0]) {
        case CMD_RUNS: if (par[1]) run_runs<double>(par.data()); else run_runs<int32_t>(par.data()); break;
        case CMD_CIGAR: run_cigar(par.data()); break;
        case CMD_K1C: run_k1c(par.data()); break;
        case CMD_K1P: run_k1p(par.data()); break;
        case CMD_CLASSIFY: if (par[1]) run_classify<double>(par.data()); else run_classify<int32_t>(par.data()); break;
        case CMD_CORRELATE: run_correlate(par.data()); break;
        case CMD_PROBE: run_probe(par.data()); break;
        default: fprintf(stderr, "unknown kernel family %llu\n", (unsigned long long)par[0]); return 2;
        }
        ++cases;
    }
    fclose(g_in);
    if (fclose(g_out) != 0) return 2;
    printf("cases: %u, each run twice\n", cases);
    return 0;
}
